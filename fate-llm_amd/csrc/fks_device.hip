// fks_device.hip -- gfx950 kernels of the FedKSeed codec: the device translation unit.  The
// kernels live in the fks_kern_*.h files it includes, their shared layers in fks_dev_*.h.
//
// Work decomposition (DESIGN.md "Kernels"):
//   * the parameter stream (all tensors in param-group order, the order
//     zo_utils.directional_derivative_step draws z in, zo_utils.py:43-47) is cut into
//     `nchunks` runs of whole 624-word MT19937 blocks, one workgroup each;
//   * fks_jump_kernel gives every (seed, chunk) its generator window at the chunk
//     start (GF(2) jump-ahead, see fks_gf2.cpp);
//   * fks_apply_kernel holds up to kMaxSeedsPerPass seed windows in LDS, and for each
//     MT block twists them all (in place, 3 dependency phases), then lets thread q
//     own Box-Muller pair q of the block: it loads its two parameters once, runs
//     every seed in order (temper -> uniform -> z -> update, all in registers), and
//     stores them once.  Seeds run sequentially per element, exactly as the
//     reference's per-seed loop rounds them (fedkseed.py:136-141).
//
// Numerics are restated op for op from torch's CPU kernels (file:line in the
// comments); -ffp-contract=off is required, every fused multiply-add is explicit.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <type_traits>

#include "fks_internal.h"
#include "fks_bitslice.h"
#define FKS_HD __device__ __forceinline__
#include "fks_libm.h"

// Design choices measured on MI355X in rounds 1-2 are fixed in the code; the A/B knobs
// and the wrong-result timing diagnostics of those rounds were removed (their logs are
// under profiles/, their code in the git history).
constexpr int kDbMinWaves = 4;   // launch-bounds waves per SIMD of the double-buffered small-K kernel (6 WGs/CU measured 19 % slower than 5)
constexpr int kZrUnroll = 2;     // z-index replay: tiles per loop iteration (in flight per wave)
constexpr int kSm2MinWaves = 8;  // launch-bounds waves per SIMD of fks_small2_kernel (8 workgroups of 4 waves per CU: <= 64 VGPRs)
constexpr int kBsFence = 8;      // slice kernel: compiler fence after every 8 seeds' table lookups
#ifndef FKS_BS_LAG               // slice kernel, two-slice passes: half 0 twists task n only once half 1
#define FKS_BS_LAG 36            // has applied task n - FKS_BS_LAG (0: unbounded; must exceed 12)
#endif
#ifndef FKS_BS_R_VMEM            // slice kernel, wd 0 chain: of every byte column's 8 seeds, this many take R
#define FKS_BS_R_VMEM 3          // from the device-global table through the vector-memory path, loaded ahead
#endif                           // (0..8).  3: 2.3 % faster; 0, 1, 2, 4: no gain (profiles/r07_bs_colimit_ab.log)
// slice kernel, wd 0 chain: the task path without lane-mask selects, neighbour exchanges and SGPR spills
// (fks_kern_slice.h).  Kept as a set: 1.8 % faster than the parent together, while alone or in smaller sets
// each of them is within +-1.7 % either way (profiles/r09_bs_taskpath_ab.log)
#ifndef FKS_BS_D16               // 1: a lane loads and stores its two bf16 parameters as 16-bit halves,
#define FKS_BS_D16 1             // no pair exchange with the neighbour lane
#endif
#ifndef FKS_BS_G32               // 1: two seeds' g per SGPR pair, the half chosen by op_sel on the packed
#define FKS_BS_G32 1             // multiply (32 SGPRs instead of 64: no SGPR spills)
#endif
#ifndef FKS_BS_ROWMIN            // 1: the twist's row indices wrapped by unsigned min, the flip folded into
#define FKS_BS_ROWMIN 1          // per-lane constants, no compare-and-select
#endif
#ifndef FKS_BS_FLIPMUX           // 1: the flip of the tempered planes as v_bitop3_b32 on a per-lane mask
#define FKS_BS_FLIPMUX 1
#endif
// slice kernel, the fma-free wd +0 chain (kModeUpdateWdPos0, the host's choice: fks_run.cpp).  Kept as a set with it:
// -4.1 % per launch against the parent; the fma-free chain alone gains nothing, D = 8 with it 1.1 %, D = 8 and H1
// 2.2-2.5 % (profiles/r10_bs_pos0_ab.log)
#ifndef FKS_BS_LOOK              // D: the table lookups (loads only) of seed k + D are issued ahead of seed k's
#define FKS_BS_LOOK 16           // arithmetic (0: at their seed; at most 32)
#endif
#ifndef FKS_BS_H1                // 1: the twist's row and address arithmetic ahead of the flag poll, pinned in
#define FKS_BS_H1 1              // VGPRs
#endif
#ifndef FKS_PHX_VEC_ITEMS        // torch_rocm few-seed kernel: work items per thread (8; A/B: 4), see
#define FKS_PHX_VEC_ITEMS 8      // kPhxVec in fks_kern_philox.h
#endif
#ifndef FKS_BS_WGTIME            // slice kernel, diagnostic build (tools/bs_wgtime.py): per-workgroup start
#define FKS_BS_WGTIME 0          // and per-wave end times
#endif

// The device code, one translation unit (c_tab_bf16 and ensure_tables() are shared by four
// kernel families; no -fgpu-rdc): the shared layers, then one file per kernel family -- a
// kernel file includes layers only, never another kernel file.  This file keeps the
// tunables above and the launchers; the once-per-device host setup is fks_dev_host.h.
#include "fks_dev_lds.h"
#include "fks_dev_update.h"
#include "fks_dev_mt.h"
#include "fks_dev_zgen.h"
#include "fks_dev_irr.h"
#include "fks_dev_host.h"
#include "fks_kern_jump.h"
#include "fks_kern_apply.h"
#include "fks_kern_slice.h"
#include "fks_kern_irregular.h"
#include "fks_kern_philox.h"
#include "fks_kern_selfcheck.h"

namespace fks {

// ------------------------------------------------------------------ launchers
int launch_delta_apply(const DeltaApplyDesc* d, int n, int64_t max_numel, const float* delta, void* stream) {
  const int64_t blocks = std::min<int64_t>(std::max<int64_t>(1, (max_numel + 255) / 256), 2048);
  hipLaunchKernelGGL(fks_delta_apply_kernel, dim3((unsigned)blocks, (unsigned)n), dim3(256), 0, (hipStream_t)stream,
                     d, delta);
  return (int)hipGetLastError();
}

static size_t apply_lds_bytes() { return (size_t)kLdsTabBytes + (size_t)kLdsStBytes; }

int device_cu_count() {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return 256;
  return n;
}

// A runtime value to a template argument: f(std::integral_constant<int, V>{}) for the V of
// the list that equals v; -FKS_ENOTSUP for a value the list does not hold.  Every launcher's
// set of instantiated kernels is its list.
template <int... Vs>
struct IntList {};
template <int... Vs, class F>
static int dispatch(IntList<Vs...>, int v, F&& f) {
  int r = -FKS_ENOTSUP;
  (void)((v == Vs && (r = f(std::integral_constant<int, Vs>{}), true)) || ...);
  return r;
}

int launch_jump(const JumpArgs& a, int nseeds, void* stream) {
  const size_t lds = sizeof(uint32_t) * (size_t)kJumpLds2Words;
  static PerDevice attr;
  if (int e = ensure_lds_attr(attr, &fks_jump_kernel, (int)lds)) return e;
  dim3 grid((unsigned)nseeds, (unsigned)((a.nchunks + a.chunks_per_wg - 1) / a.chunks_per_wg));
  hipLaunchKernelGGL(fks_jump_kernel, grid, dim3(kJumpThreads), lds, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

template <int DT, int MODE, bool FULL, bool DB = false>
static int launch_apply_f(const ApplyArgs& a, void* stream) {
  // a partial pass allocates only its own windows (+1 spare: the twist's last-phase lanes
  // read past a window), so calls of few seeds fit more workgroups per CU
  const size_t lds = FULL ? apply_lds_bytes()
                          : (size_t)kLdsTabBytes + (size_t)((DB ? 2 : 1) * a.nseeds + 1) * kWinBytes;
  static PerDevice attr;
  if (int e = ensure_lds_attr(attr, &fks_apply_kernel<DT, MODE, FULL, DB>, (int)apply_lds_bytes())) return e;
  hipLaunchKernelGGL((fks_apply_kernel<DT, MODE, FULL, DB>), dim3((unsigned)a.nchunks),
                     dim3(DB ? kDbThreads : kApplyThreads), lds, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

template <int DT, int MODE, int ZM = 0>
static int launch_small2(const ApplyArgs& a, void* stream) {
  const size_t lds = (size_t)kLdsTabBytes + (size_t)(2 * a.nseeds + 1) * kWinBytes;
  static PerDevice attr;
  // the attribute is set once per device: for the largest pass this kernel takes
  constexpr int kMaxLds = kLdsTabBytes + (2 * kSmallK + 1) * kWinBytes;
  if (int e = ensure_lds_attr(attr, &fks_small2_kernel<DT, MODE, ZM>, kMaxLds)) return e;
  hipLaunchKernelGGL((fks_small2_kernel<DT, MODE, ZM>), dim3((unsigned)a.nchunks), dim3(kSm2Threads), lds,
                     (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

template <int DT, int MODE>
static int launch_apply_t(const ApplyArgs& a, void* stream) {
  if (a.nseeds == kMaxSeedsPerPass) return launch_apply_f<DT, MODE, true>(a, stream);
  if constexpr (DT == FKS_BF16) {
    // one-seed bf16 passes with a z-index buffer (fks_cache.cpp ZCache): store / replay
    if (a.zmode == 1 && a.nseeds == 1 && MODE == kModePerturb) return launch_small2<DT, MODE, 1>(a, stream);
    if (a.zmode == 2 && a.nseeds == 1 &&
        (MODE == kModePerturb || MODE == kModePerturbUpdate || MODE == kModeUpdate || MODE == kModeUpdateWd ||
         MODE == kModeUpdateNoWd || MODE == kModeUpdateWd0)) {
      hipLaunchKernelGGL((fks_zreplay_kernel<MODE>), dim3((unsigned)a.nchunks), dim3(kZrThreads), (size_t)3 * 1024,
                         (hipStream_t)stream, a);
      return (int)hipGetLastError();
    }
  }
  if (a.zmode == 2) return -FKS_ENOTSUP;  // replay without a replay kernel: a host bug
  if (a.nseeds <= kSmallK && DT != FKS_F16) return launch_small2<DT == FKS_F16 ? FKS_F32 : DT, MODE>(a, stream);
  if (a.nseeds <= kSmallK) return launch_apply_f<DT, MODE, false, true>(a, stream);  // f16
  return launch_apply_f<DT, MODE, false>(a, stream);
}

int launch_apply(int dtype, const ApplyArgs& a, void* stream) {
  if (a.nseeds < 1 || a.nseeds > kMaxSeedsPerPass || a.nchunks < 1) return -FKS_EINVAL;
  if (dtype == FKS_BF16) {
    int e = ensure_tables();
    if (e) return e;
  }
  using Modes = IntList<kModeUpdate, kModeUpdateWd, kModeUpdateNoWd, kModeUpdateWd0, kModePerturb, kModePerturbUpdate,
                        kModeWriteZ, kModeDelta>;
  return dispatch(IntList<FKS_F32, kDtF32Libm, FKS_BF16>{}, dtype, [&](auto dt) {
    return dispatch(Modes{}, a.mode,
                    [&](auto m) { return launch_apply_t<decltype(dt)::value, decltype(m)::value>(a, stream); });
  });
}

template <int MODE, bool FULL>
static int launch_apply_bs_m(const ApplyBsArgs& a, void* stream) {
  static PerDevice attr;
  if (int e = ensure_lds_attr(attr, &fks_apply_bs_kernel<MODE, FULL>, kBsLdsBytes)) return e;
  hipLaunchKernelGGL((fks_apply_bs_kernel<MODE, FULL>), dim3((unsigned)(a.split ? a.nchunks / 2 : a.nchunks)),
                     dim3(kBsThreads), kBsLdsBytes, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

template <int MODE>
static int launch_apply_bs_t(const ApplyBsArgs& a, void* stream) {
  // FULL: 32 seeds in each half (a split pass of 32, a two-slice pass of 64)
  const bool full = a.nseeds == (a.split ? kBsSeeds : kBsPassSeeds);
  return full ? launch_apply_bs_m<MODE, true>(a, stream) : launch_apply_bs_m<MODE, false>(a, stream);
}

int launch_apply_bs(const ApplyBsArgs& a, void* stream) {
  if (a.nseeds < 1 || a.nseeds > (a.split ? kBsSeeds : kBsPassSeeds) || a.nchunks < 1 ||
      (a.split && a.nchunks % 2))
    return -FKS_EINVAL;
  int e = ensure_tables();
  if (e) return e;
  return dispatch(IntList<kModeUpdate, kModeUpdateWd, kModeUpdateNoWd, kModeUpdateWd0, kModeUpdateWdPos0, kModeDelta>{}, a.mode,
                  [&](auto m) { return launch_apply_bs_t<decltype(m)::value>(a, stream); });
}

template <int MODE>
static int launch_irregular_m(const IrrArgs& a, void* stream) {
  const size_t lds = (size_t)kIrrLogfOff + kLdsLogfBytes;  // tables | windows | wave counters | logf table
  static PerDevice attr;
  if (int e = ensure_lds_attr(attr, &fks_irregular_kernel<MODE>, (int)lds)) return e;
  hipLaunchKernelGGL((fks_irregular_kernel<MODE>), dim3((unsigned)a.nchunks), dim3(kApplyThreads), lds,
                     (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int launch_philox_fast_radius_check(uint32_t* counts, void* stream) {
  hipLaunchKernelGGL(fks_philox_fast_radius_kernel, dim3(kSqrtDomainBlocks), dim3(256), 0, (hipStream_t)stream, counts);
  return (int)hipGetLastError();
}

int launch_philox_radius_check(uint32_t* counts, void* stream) {
  hipLaunchKernelGGL(fks_philox_radius_kernel, dim3(kSqrtDomainBlocks), dim3(256), 0, (hipStream_t)stream, counts);
  return (int)hipGetLastError();
}

int launch_sqrt_domain_check(uint32_t* counts, void* stream) {
  hipLaunchKernelGGL(fks_sqrt_domain_kernel, dim3(kSqrtDomainBlocks), dim3(256), 0, (hipStream_t)stream, counts);
  return (int)hipGetLastError();
}

int device_max_threads_per_cu() {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 2048;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMaxThreadsPerMultiProcessor, dev) != hipSuccess || n <= 0) return 2048;
  return n;
}

// launches of at most this many seeds take fks_philox_vec_kernel: every launch by default
// (7B bf16 wd 0, 32-seed launches: 4.39 against 4.57 ms per seed in the item loop;
// profiles/r05i_rocm_rate_vec_ab.log); FKS_PHX_VEC_MAXK=0 restores the item loop (A/B)
static int phx_vec_maxk() {
  static const int v = [] {
    const char* s = std::getenv("FKS_PHX_VEC_MAXK");
    return (s && *s) ? std::atoi(s) : kPhxSeeds;
  }();
  return v;
}

template <int MODE>
static int launch_philox_m(const PhiloxArgs& a, void* stream) {
  const int64_t items = a.item_hi - a.item_lo;
  if (items <= 0) return 0;
  if (a.nseeds <= phx_vec_maxk() && a.item_lo % kPhxVec == 0 && items % kPhxVec == 0) {
    const int64_t vitems = items / kPhxVec;
    const int64_t blocks = std::min<int64_t>((vitems + 255) / 256, (int64_t)device_cu_count() * 16);
    const size_t lds = a.nt <= kPhxLdsTensors ? sizeof(PhxTensor) * (size_t)a.nt : 0;
    hipLaunchKernelGGL((fks_philox_vec_kernel<MODE>), dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, a);
    return (int)hipGetLastError();
  }
  const int64_t blocks = std::min<int64_t>((items + 255) / 256, (int64_t)device_cu_count() * 16);
  hipLaunchKernelGGL((fks_philox_kernel<MODE>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int launch_philox(const PhiloxArgs& a, void* stream) {
  if (a.nseeds < 1 || a.nt < 1) return -FKS_EINVAL;
  using Modes = IntList<kModeUpdate, kModeUpdateWd, kModeUpdateNoWd, kModeUpdateWd0, kModeUpdateWdPos0, kModePerturb,
                        kModePerturbUpdate, kModeWriteZ, kModeDelta>;
  return dispatch(Modes{}, a.mode, [&](auto m) { return launch_philox_m<decltype(m)::value>(a, stream); });
}

int launch_irregular(const IrrArgs& a, void* stream) {
  if (a.nseeds < 1 || a.nseeds > kMaxSeedsPerPass) return -FKS_EINVAL;
  int e = ensure_tables();
  if (e) return e;
  return dispatch(IntList<kModeUpdate, kModePerturb, kModePerturbUpdate, kModeWriteZ, kModeDelta>{}, a.mode,
                  [&](auto m) { return launch_irregular_m<decltype(m)::value>(a, stream); });
}

}  // namespace fks
