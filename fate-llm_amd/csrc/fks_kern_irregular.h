// fks_kern_irregular.h -- fks_irregular_kernel: everything the fast kernels do not take.
#pragma once
#include <hip/hip_runtime.h>

#include "fks_internal.h"
#include "fks_libm.h"
#include "fks_dev_update.h"
#include "fks_dev_mt.h"
#include "fks_dev_zgen.h"

namespace fks {
namespace {

// ------------------------------------------------------------------ irregular kernel
// Everything the fast kernel does not take (DESIGN.md "Irregular layouts"):
//   * runs of whole 16-blocks at any stream phase (a tensor after a ragged one, a
//     ragged tensor's head with its overwritten elements masked, its 16-word tail
//     recompute, f16 tensors, parameters not 2-element aligned), and
//   * single elements of numel < 16 tensors (serial normal_distribution<double>,
//     DistributionsHelper.h:189-221, with the cached second sample).
// A work item is handled in the MT block holding its LAST word; its first words may
// lie up to 15 words back, in the previous block, so every seed window carries the
// previous block's last 16 raw words in front of it: [carry 16 | 624].
__constant__ float c_tab_f16[3 * 2048];  // R | C | S of the 11-bit f16 uniforms

constexpr int kIrrCarry = 16;
constexpr int kIrrWin = kIrrCarry + kMtN;  // words per seed window

__device__ __forceinline__ uint32_t win_word(const uint32_t* win, int k, int w) {  // w in [-16, 624)
  return win[k * kIrrWin + kIrrCarry + w];
}

// in-place twist of every window, phase PH of 3 (i in [0,227) / [227,454) / [454,624));
// phase 0 also saves the old words 608..623 as the next block's carry
template <int PH>
__device__ __forceinline__ void irr_twist_phase(uint32_t* win, int nseeds, int tid) {
  constexpr int lo = PH == 0 ? 0 : (PH == 1 ? 227 : 454);
  constexpr int hi = PH == 0 ? 227 : (PH == 1 ? 454 : kMtN);
  constexpr int len = hi - lo;
  constexpr int per = (kMaxSeedsPerPass * len + kApplyThreads - 1) / kApplyThreads;
  uint32_t v[per];
#pragma unroll
  for (int j = 0; j < per; j++) {
    const int idx = tid + j * kApplyThreads;
    if (idx < nseeds * len) {
      const int k = idx / len, i = lo + idx % len;
      const uint32_t* w = win + k * kIrrWin + kIrrCarry;
      const uint32_t nx = i == kMtN - 1 ? w[0] : w[i + 1];
      const uint32_t m = i < kMtN - kMtM ? w[i + kMtM] : w[i - (kMtN - kMtM)];
      v[j] = m ^ mt_twist(w[i], nx);
    }
  }
  uint32_t cv = 0;
  if (PH == 0 && tid < nseeds * kIrrCarry) cv = win[(tid / kIrrCarry) * kIrrWin + kIrrCarry + kMtN - kIrrCarry + tid % kIrrCarry];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < per; j++) {
    const int idx = tid + j * kApplyThreads;
    if (idx < nseeds * len) win[(idx / len) * kIrrWin + kIrrCarry + lo + idx % len] = v[j];
  }
  if (PH == 0 && tid < nseeds * kIrrCarry) win[(tid / kIrrCarry) * kIrrWin + tid % kIrrCarry] = cv;
  __syncthreads();
}

// z pair from two raw words, any dtype (f16 through its 11-bit tables in constant memory)
constexpr int kIrrLogfOff = kLdsTabBytes + 4 * (kIrrWin * kMaxSeedsPerPass + 16);  // after the wave counters
static_assert(kIrrLogfOff % 16 == 0, "logf table alignment");

template <int DT>
__device__ __forceinline__ void irr_z_pair(const uint8_t* lds, uint32_t r1, uint32_t r2, float& z1, float& z2) {
  if constexpr (DT == kDtF32Libm) {
    z_pair_f32_libm((uint32_t)kIrrLogfOff, r1, r2, z1, z2);
  } else if constexpr (DT == FKS_F16) {
    const uint32_t a = mt_temper(r1) & 0x7FFu, b = mt_temper(r2) & 0x7FFu;
    z1 = rhf(__fmaf_rn(c_tab_f16[a], c_tab_f16[2048 + b], 0.0f));
    z2 = rhf(__fmaf_rn(c_tab_f16[a], c_tab_f16[4096 + b], 0.0f));
  } else {
    z_pair<DT>(lds, r1, r2, z1, z2);
  }
}

template <int DT, int MODE>
__device__ __forceinline__ void irr_run_lane(const uint8_t* lds, const uint32_t* win, const IrrArgs& a, const DevRun& R,
                                             int64_t e1, int w1) {
  using TR = Traits<MODE == kModeDelta ? FKS_F32 : DT>;  // storage (kModeDelta: the f32 delta)
  const bool on1 = e1 < R.limit, on2 = e1 + 8 < R.limit;
  float p1 = 0.0f, p2 = 0.0f;
  if (MODE != kModeWriteZ) {
    if (on1) p1 = TR::load(R.ptr, e1);
    if (on2) p2 = TR::load(R.ptr, e1 + 8);
  }
  const bool has_wd = (R.flags & FKS_HAS_WD) != 0;
  const float* g = a.g[DT == kDtF32Libm ? FKS_F32 : DT];
  const bool dv = MODE == kModePerturbUpdate && a.gdev;
  const bool upd = dv ? dev_value_apply(a.gdev) : true;
  for (int k = 0; k < a.nseeds; k++) {
    float z1, z2;
    irr_z_pair<DT>(lds, win_word(win, k, w1), win_word(win, k, w1 + 8), z1, z2);
    const float gv = dv ? dev_value_g<DT>(a.gdev) : g[k];
    p1 = apply_one<DT>(p1, z1, gv, R.lr, R.wd, has_wd, MODE, R.ps, upd);
    p2 = apply_one<DT>(p2, z2, gv, R.lr, R.wd, has_wd, MODE, R.ps, upd);
  }
  if (on1) TR::store(R.ptr, e1, p1);
  if (on2) TR::store(R.ptr, e1 + 8, p2);
}

__device__ __forceinline__ double u53(uint32_t hi, uint32_t lo) {  // uniform_real_distribution<double>
  const uint64_t x = (((uint64_t)hi << 32) | lo) & ((1ull << 53) - 1);
  return (double)x * (1.0 / 9007199254740992.0);
}

template <int DT, int MODE>
__device__ __forceinline__ void irr_tiny_lane(const uint32_t* win, const IrrArgs& a, const DevTiny& T, int w) {
  using TR = Traits<MODE == kModeDelta ? FKS_F32 : DT>;  // storage (kModeDelta: the f32 delta)
  float p = MODE != kModeWriteZ ? TR::load(T.ptr, 0) : 0.0f;
  const bool has_wd = (T.flags & FKS_HAS_WD) != 0;
  const bool sin_half = (T.flags & kTinySin) != 0;
  const float* g = a.g[DT];
  const bool dv = MODE == kModePerturbUpdate && a.gdev;
  const bool upd = dv ? dev_value_apply(a.gdev) : true;
  for (int k = 0; k < a.nseeds; k++) {
    const double u1 = u53(mt_temper(win_word(win, k, w)), mt_temper(win_word(win, k, w + 1)));
    const double u2 = u53(mt_temper(win_word(win, k, w + 2)), mt_temper(win_word(win, k, w + 3)));
    // glibc's log1p and correctly rounded sin / cos (fks_libm.h): ocml's differ from the
    // host libm by an ulp often enough to flip fp32 midpoint cases
    const double r = sqrt(-2.0 * fks_libm::log1p(-u2));
    const double theta = 2.0 * 3.14159265358979323846 * u1;
    const double v = r * fks_libm::sin_or_cos(theta, sin_half) * 1.0 + 0.0;
    const float zf = (float)v;  // static_cast<scalar_t>(double): via float for bf16 / f16
    const float z = DT == FKS_F32 ? zf : Traits<DT>::rnd(zf);
    p = apply_one<DT>(p, z, dv ? dev_value_g<DT>(a.gdev) : g[k], T.lr, T.wd, has_wd, MODE, T.ps, upd);
  }
  TR::store(T.ptr, 0, p);
}

template <int MODE>
__global__ __launch_bounds__(kApplyThreads) void fks_irregular_kernel(IrrArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds32[];
  uint8_t* lds = reinterpret_cast<uint8_t*>(lds32);
  uint32_t* win = reinterpret_cast<uint32_t*>(lds + kLdsTabBytes);
  uint32_t* cnt = win + kIrrWin * kMaxSeedsPerPass;  // per-wave counters
  if ((uint32_t)(size_t)(lds_u32_t*)lds32 != 0u) __builtin_trap();  // z_pair reads the tables at LDS 0
  const int tid = threadIdx.x;
  const int c = blockIdx.x;
  const int nseeds = a.nseeds;
  const int64_t b0 = a.chunk_lo[c], b1 = a.chunk_hi[c];
  {
    float2* tabCS = reinterpret_cast<float2*>(lds + kLdsCsOff);
    for (int i = tid; i < 256; i += kApplyThreads) {
      reinterpret_cast<float*>(lds)[i] = c_tab_bf16[i];
      tabCS[i] = make_float2(c_tab_bf16[256 + i], c_tab_bf16[512 + i]);
    }
  }
  if (a.libm) logf_tab_fill((uint32_t)kIrrLogfOff, tid, kApplyThreads);
  for (int idx = tid; idx < nseeds * kMtN; idx += kApplyThreads) {
    const int k = idx / kMtN, i = idx - k * kMtN;
    win[k * kIrrWin + kIrrCarry + i] = a.states[((size_t)k * a.nchunks + c) * kMtN + i];
  }
  // first run whose last word is in or after block b0; first single element likewise
  int ri, ti;
  {
    int lo = 0, hi = a.nruns;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (a.runs[mid].start + a.runs[mid].numel - 1 < (int64_t)kMtN * b0) lo = mid + 1; else hi = mid;
    }
    ri = lo;
    lo = 0, hi = a.ntiny;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (a.tiny[mid].word + 3 < (int64_t)kMtN * b0) lo = mid + 1; else hi = mid;
    }
    ti = lo;
  }
  __syncthreads();
  const int m = tid >> 3, r8 = tid & 7;
  for (int64_t b = b0; b < b1; b++) {
    irr_twist_phase<0>(win, nseeds, tid);
    irr_twist_phase<1>(win, nseeds, tid);
    irr_twist_phase<2>(win, nseeds, tid);
    const int64_t base = (int64_t)kMtN * b, end = base + kMtN;
    // runs with a 16-block ending in this block (disjoint, sorted: a contiguous range)
    while (ri < a.nruns && a.runs[ri].start + 15 < end) {
      const DevRun R = a.runs[ri];
      const int ph = (int)(R.start & 15);
      const int64_t s0 = base + 16 * m + (ph ? ph - 16 : 0);  // this lane's 16-block start
      if (tid < kMtN / 2 && s0 >= R.start && s0 < R.start + R.numel) {
        const int64_t e1 = s0 - R.start + r8;
        const int w1 = (int)(s0 - base) + r8;
        switch (R.dtype) {
          case FKS_F32:
            if (a.libm) irr_run_lane<kDtF32Libm, MODE>(lds, win, a, R, e1, w1);
            else irr_run_lane<FKS_F32, MODE>(lds, win, a, R, e1, w1);
            break;
          case FKS_BF16: irr_run_lane<FKS_BF16, MODE>(lds, win, a, R, e1, w1); break;
          default: irr_run_lane<FKS_F16, MODE>(lds, win, a, R, e1, w1); break;
        }
      }
      if (R.start + R.numel - 1 < end) ri++; else break;
    }
    // single elements whose draw pair ends in this block (sorted: a prefix from ti)
    for (;;) {
      const int idx = ti + tid;
      const bool mine = idx < a.ntiny && a.tiny[idx].word + 3 < end;
      if (mine) {
        const DevTiny T = a.tiny[idx];
        const int w = (int)(T.word - base);
        switch (T.dtype) {
          case FKS_F32: irr_tiny_lane<FKS_F32, MODE>(win, a, T, w); break;
          case FKS_BF16: irr_tiny_lane<FKS_BF16, MODE>(win, a, T, w); break;
          default: irr_tiny_lane<FKS_F16, MODE>(win, a, T, w); break;
        }
      }
      // block-wide count of `mine` through a few dynamic-LDS words (__syncthreads_count
      // would add static LDS and move the dynamic block off address 0)
      const uint64_t bal = __ballot(mine);
      if ((tid & 63) == 0) cnt[tid >> 6] = (uint32_t)__popcll(bal);
      __syncthreads();
      int n = 0;
#pragma unroll
      for (int w = 0; w < kApplyThreads / 64; w++) n += (int)cnt[w];
      __syncthreads();
      ti += n;
      if (n < kApplyThreads) break;
    }
  }
}

}  // namespace
}  // namespace fks
