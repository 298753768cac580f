// fks_project_mt.hip -- seed-basis projection on the CPU generator's MT19937 stream
// (include/fks.h fks_project_mt): out[s] = <vec, z_s> over the elements one element shard owns,
// the adjoint of fks_delta_accumulate on that stream.  The plan is the kModeDelta plan, whose
// segments, runs and single elements point into the f32 vector; where the delta kernels run
// `delta += c z` and store, these kernels run `sum += v z` and reduce.
//
// fks_project_mt_kernel<DT, FULL> takes the fast segments of one dtype on fks_apply_kernel's
// frame (fks_kern_apply.h): one workgroup of kApplyThreads per plan chunk, the chunk-start
// windows of the pass's seeds in LDS, twist_all per MT block, lane q < 312 owning the Box-Muller
// pair (j1, j1 + 8) of every block.  Per block a lane loads its two vector elements, widens them
// to f64 once, and per seed adds the two exact products (24 + 24 significand bits) to that
// seed's own f64 accumulator by fma: kMaxSeedsPerPass accumulators per lane, alive across the
// chunk.  A lane off every segment, and the 8 idle lanes, multiply z by +0.
// fks_project_mt_irr_kernel takes the rest on fks_irregular_kernel's frame
// (fks_kern_irregular.h): runs of 16-blocks at any stream phase with their limit mask, the
// 16-word tail recompute, every f16 tensor and the serial double Box-Muller elements of
// numel < 16 tensors.  Its seed loop is dynamic, so a lane keeps no array: the lanes' terms of
// seed k are summed over the wave at once and lane k adds the total to its one running sum.
//
// The reduction uses no floating-point atomic and has one fixed order: per seed a 64-lane xor
// butterfly, the five waves in wave order through LDS (the space of the windows, which nothing
// reads any more), partial[chunk][kPhxSeeds]; fks_project_reduce_kernel (fks_project.hip) adds
// the rows of all launches of the pass in row order.
//
// A translation unit of its own, so that fks_device.o and fks_build_id() do not move: it has
// its own copies of the __constant__ tables and fills them per device itself.
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>

#include "fks_internal.h"
#include "fks_dev_lds.h"
#include "fks_dev_mt.h"
#include "fks_dev_zgen.h"
#include "fks_libm.h"

namespace fks {
namespace {

__constant__ float c_pmt_tab_f16[3 * 2048];  // R | C | S of the 11-bit f16 uniforms

typedef __attribute__((address_space(1))) const float pmt_gf32;

__device__ __forceinline__ double pmt_wave_sum(double x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
  return x;
}

// the waves' sums of one workgroup, [kWaves][kMaxSeedsPerPass] f64, go where window 0 was:
// the reduction adds nothing to the LDS footprint
constexpr int kPmtRedBytes = kWaves * kMaxSeedsPerPass * 8;
static_assert(kPmtRedBytes <= kWinBytes, "the waves' sums fit in the first window");

// ------------------------------------------------------------------ fast segments
template <int DT, bool FULL>
__global__ __launch_bounds__(kApplyThreads, (kApplyWgPerCu * kApplyThreads + 255) / 256) void fks_project_mt_kernel(
    ProjMtArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds32[];
  uint8_t* lds = reinterpret_cast<uint8_t*>(lds32);
  // the lds_* accessors address LDS by offset from 0: the dynamic block must start there
  if ((uint32_t)(size_t)(lds_u32_t*)lds32 != 0u) __builtin_trap();
  const int tid = threadIdx.x;
  const int c = blockIdx.x;
  const int nseeds = FULL ? kMaxSeedsPerPass : a.nseeds;
  const int64_t b0 = a.chunk_block[c], b1 = a.chunk_block[c + 1];

  if constexpr (DT == FKS_BF16) {
    float2* tabCS = reinterpret_cast<float2*>(lds + kLdsCsOff);
    for (int i = tid; i < 256; i += kApplyThreads) {
      reinterpret_cast<float*>(lds)[i] = c_tab_bf16[i];
      tabCS[i] = make_float2(c_tab_bf16[256 + i], c_tab_bf16[512 + i]);
    }
  } else if constexpr (DT == kDtF32Libm) {
    logf_tab_fill(0u, tid, kApplyThreads);
  }
  for (int idx = tid; idx < nseeds * kMtN; idx += kApplyThreads) {
    const int k = idx / kMtN, i = idx - k * kMtN;
    lds_st(kLdsTabBytes + k * kWinBytes + 4 * wperm(i), a.states[((size_t)k * a.nchunks + c) * kMtN + i]);
  }
  TwistPlan plan;
  twist_plan(plan, tid, kLdsTabBytes);
  __syncthreads();

  // Thread q < 312 owns Box-Muller pair q of every block: block words j1 = 16 (q / 8) + q % 8
  // and j1 + 8, which lie in one 16-block and so in one segment
  const bool lane_on = tid < kMtN / 2;
  const int j1 = 16 * (tid >> 3) + (tid & 7);
  const int st_off = kLdsTabBytes + 4 * wperm(j1);  // the (j1, j1 + 8) word pair

  // The lane's current segment, cached in registers; positions only grow.
  int cur;
  {
    const int64_t s1 = (int64_t)kMtN * b0 + j1;
    int lo = 0, hi = a.nsegs;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (a.segs[mid].start + a.segs[mid].numel <= s1) lo = mid + 1; else hi = mid;
    }
    cur = lo;
  }
  int64_t seg_start = INT64_MAX, seg_end = INT64_MAX;
  uint64_t seg_ptr = 0;
  auto load_seg = [&]() {  // (selects, not branches: the launcher refuses a launch without segments)
    const bool have = cur < a.nsegs;
    const DevSeg& sg = a.segs[have ? cur : 0];
    const int64_t st = sg.start, n = sg.numel;
    seg_start = have ? st : INT64_MAX;
    seg_end = have ? st + n : INT64_MAX;
    seg_ptr = sg.ptr;
  };
  load_seg();

  // software pipeline: block b+1's elements are fetched before block b's Box-Muller.  An off
  // lane loads the workspace sink, so the loads are unconditional; its values are dropped.
  struct Slot { float x1, x2; uint32_t on; };
  auto fetch = [&](int64_t b) -> Slot {
    Slot sl;
    const int64_t s1 = (int64_t)kMtN * b + j1;
    while (s1 >= seg_end) { cur++; load_seg(); }
    const bool on = lane_on && s1 >= seg_start;
    const uint64_t addr = on ? seg_ptr + (uint64_t)(s1 - seg_start) * 4u : (uint64_t)(uintptr_t)a.sink;
    sl.on = on;
    sl.x1 = *reinterpret_cast<pmt_gf32*>(addr);
    sl.x2 = *reinterpret_cast<pmt_gf32*>(addr + 32u);
    return sl;
  };

  double acc[kMaxSeedsPerPass];  // seed k's sum over this lane's elements of the chunk
#pragma unroll
  for (int k = 0; k < kMaxSeedsPerPass; k++) acc[k] = 0.0;

  Slot sa = fetch(b0);
  for (int64_t b = b0; b < b1; b++) {
    __syncthreads();          // every wave is done reading block b-1's words
    twist_all(plan, nseeds);  // the raw words of stream block b
    __syncthreads();          // every window holds block b
    const Slot nxt = fetch(b + 1 < b1 ? b + 1 : b);  // (the last block re-reads itself, unused)
    // an off lane enters +0: its products are zeros whatever its z, and its sums stay +0
    const double v1 = sa.on ? (double)sa.x1 : 0.0, v2 = sa.on ? (double)sa.x2 : 0.0;
    // unrolled with wave-uniform guards: a dynamic seed index would put acc[] in scratch
#pragma unroll
    for (int k = 0; k < kMaxSeedsPerPass; k++) {
      if (FULL || k < nseeds) {
        const uint64_t w = lds_u64(st_off + k * kWinBytes);  // (word j1, word j1+8), permuted window
        const f32x2_t z = z_pair2<DT>(lds, (uint32_t)w, (uint32_t)(w >> 32));
        acc[k] = __fma_rn(v1, (double)z.x, acc[k]);  // exact product, one rounding per addition
        acc[k] = __fma_rn(v2, (double)z.y, acc[k]);
      }
    }
    sa = nxt;
  }

  __syncthreads();  // the windows are free: the waves' sums go where window 0 was
  double* red = reinterpret_cast<double*>(lds + kLdsTabBytes);  // [kWaves][kMaxSeedsPerPass]
#pragma unroll
  for (int k = 0; k < kMaxSeedsPerPass; k++) {
    if (FULL || k < nseeds) {
      const double s = pmt_wave_sum(acc[k]);
      if (plan.lane == 0) red[plan.wave * kMaxSeedsPerPass + k] = s;
    }
  }
  __syncthreads();
  if (tid < nseeds) {
    double s = red[tid];
#pragma unroll
    for (int w = 1; w < kWaves; w++) s += red[w * kMaxSeedsPerPass + tid];
    a.partial[(size_t)c * kPhxSeeds + tid] = s;
  }
}

// ------------------------------------------------------------------ irregular work
// The frame of fks_irregular_kernel: a work item is handled in the MT block holding its LAST
// word, so every seed window carries the previous block's last 16 raw words in front of it:
// [carry 16 | 624].
constexpr int kPmtCarry = 16;
constexpr int kPmtWin = kPmtCarry + kMtN;  // words per seed window
constexpr int kPmtLogfOff = kLdsTabBytes + 4 * (kPmtWin * kMaxSeedsPerPass + 16);  // after the wave counters
static_assert(kPmtLogfOff % 16 == 0, "logf table alignment");

__device__ __forceinline__ uint32_t pmt_word(const uint32_t* win, int k, int w) {  // w in [-16, 624)
  return win[k * kPmtWin + kPmtCarry + w];
}

// in-place twist of every window, phase PH of 3 (i in [0,227) / [227,454) / [454,624));
// phase 0 also saves the old words 608..623 as the next block's carry
template <int PH>
__device__ __forceinline__ void pmt_twist_phase(uint32_t* win, int nseeds, int tid) {
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
      const uint32_t* w = win + k * kPmtWin + kPmtCarry;
      const uint32_t nx = i == kMtN - 1 ? w[0] : w[i + 1];
      const uint32_t m = i < kMtN - kMtM ? w[i + kMtM] : w[i - (kMtN - kMtM)];
      v[j] = m ^ mt_twist(w[i], nx);
    }
  }
  uint32_t cv = 0;
  if (PH == 0 && tid < nseeds * kPmtCarry)
    cv = win[(tid / kPmtCarry) * kPmtWin + kPmtCarry + kMtN - kPmtCarry + tid % kPmtCarry];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < per; j++) {
    const int idx = tid + j * kApplyThreads;
    if (idx < nseeds * len) win[(idx / len) * kPmtWin + kPmtCarry + lo + idx % len] = v[j];
  }
  if (PH == 0 && tid < nseeds * kPmtCarry) win[(tid / kPmtCarry) * kPmtWin + tid % kPmtCarry] = cv;
  __syncthreads();
}

// z pair from two raw words, any dtype, as fks_irregular_kernel's irr_z_pair computes it
template <int DT>
__device__ __forceinline__ void pmt_z_pair(const uint8_t* lds, uint32_t r1, uint32_t r2, float& z1, float& z2) {
  if constexpr (DT == kDtF32Libm) {
    z_pair_f32_libm((uint32_t)kPmtLogfOff, r1, r2, z1, z2);
  } else if constexpr (DT == FKS_F16) {
    const uint32_t a = mt_temper(r1) & 0x7FFu, b = mt_temper(r2) & 0x7FFu;
    z1 = rhf(__fmaf_rn(c_pmt_tab_f16[a], c_pmt_tab_f16[2048 + b], 0.0f));
    z2 = rhf(__fmaf_rn(c_pmt_tab_f16[a], c_pmt_tab_f16[4096 + b], 0.0f));
  } else {
    z_pair<DT>(lds, r1, r2, z1, z2);
  }
}

// Every seed of the pass over one 16-block pair per lane (the whole wave runs this; a lane
// without work has x1 = x2 = +0 and reads the window's word 0): lane k collects seed k's sum.
template <int DT>
__device__ __forceinline__ void pmt_run_seeds(const uint8_t* lds, const uint32_t* win, int nseeds, int w1, float x1,
                                              float x2, int lane, double& acc) {
  const double v1 = (double)x1, v2 = (double)x2;
  for (int k = 0; k < nseeds; k++) {
    float z1, z2;
    pmt_z_pair<DT>(lds, pmt_word(win, k, w1), pmt_word(win, k, w1 + 8), z1, z2);
    double part = __fma_rn(v1, (double)z1, 0.0);
    part = __fma_rn(v2, (double)z2, part);
    const double total = pmt_wave_sum(part);
    acc += lane == k ? total : 0.0;
  }
}

__device__ __forceinline__ double pmt_u53(uint32_t hi, uint32_t lo) {  // uniform_real_distribution<double>
  const uint64_t x = (((uint64_t)hi << 32) | lo) & ((1ull << 53) - 1);
  return (double)x * (1.0 / 9007199254740992.0);
}

static_assert(kMaxSeedsPerPass <= 64, "lane k of a wave keeps seed k's sum");

__global__ __launch_bounds__(kApplyThreads) void fks_project_mt_irr_kernel(ProjMtIrrArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds32[];
  uint8_t* lds = reinterpret_cast<uint8_t*>(lds32);
  uint32_t* win = reinterpret_cast<uint32_t*>(lds + kLdsTabBytes);
  uint32_t* cnt = win + kPmtWin * kMaxSeedsPerPass;  // per-wave counters
  if ((uint32_t)(size_t)(lds_u32_t*)lds32 != 0u) __builtin_trap();  // z_pair reads the tables at LDS 0
  const int tid = threadIdx.x;
  const int lane = tid & 63;
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
  if (a.libm) logf_tab_fill((uint32_t)kPmtLogfOff, tid, kApplyThreads);
  for (int idx = tid; idx < nseeds * kMtN; idx += kApplyThreads) {
    const int k = idx / kMtN, i = idx - k * kMtN;
    win[k * kPmtWin + kPmtCarry + i] = a.states[((size_t)k * a.nchunks + c) * kMtN + i];
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
  double acc = 0.0;  // lane k < nseeds: this wave's sum for seed k
  const int m = tid >> 3, r8 = tid & 7;
  for (int64_t b = b0; b < b1; b++) {
    pmt_twist_phase<0>(win, nseeds, tid);
    pmt_twist_phase<1>(win, nseeds, tid);
    pmt_twist_phase<2>(win, nseeds, tid);
    const int64_t base = (int64_t)kMtN * b, end = base + kMtN;
    // runs with a 16-block ending in this block (disjoint, sorted: a contiguous range)
    while (ri < a.nruns && a.runs[ri].start + 15 < end) {
      const DevRun R = a.runs[ri];
      const int ph = (int)(R.start & 15);
      const int64_t s0 = base + 16 * m + (ph ? ph - 16 : 0);  // this lane's 16-block start
      const bool mine = tid < kMtN / 2 && s0 >= R.start && s0 < R.start + R.numel;
      if (__any(mine)) {  // wave-uniform: every lane of the wave reaches the butterflies
        const int64_t e1 = mine ? s0 - R.start + r8 : 0;
        const int w1 = mine ? (int)(s0 - base) + r8 : 0;
        float x1 = 0.0f, x2 = 0.0f;  // elements at or past the limit are another run's: not read
        if (mine && e1 < R.limit) x1 = reinterpret_cast<pmt_gf32*>(R.ptr)[e1];
        if (mine && e1 + 8 < R.limit) x2 = reinterpret_cast<pmt_gf32*>(R.ptr)[e1 + 8];
        switch (R.dtype) {
          case FKS_F32:
            if (a.libm) pmt_run_seeds<kDtF32Libm>(lds, win, nseeds, w1, x1, x2, lane, acc);
            else pmt_run_seeds<FKS_F32>(lds, win, nseeds, w1, x1, x2, lane, acc);
            break;
          case FKS_BF16: pmt_run_seeds<FKS_BF16>(lds, win, nseeds, w1, x1, x2, lane, acc); break;
          default: pmt_run_seeds<FKS_F16>(lds, win, nseeds, w1, x1, x2, lane, acc); break;
        }
      }
      if (R.start + R.numel - 1 < end) ri++; else break;
    }
    // single elements whose draw pair ends in this block (sorted: a prefix from ti)
    for (;;) {
      const int idx = ti + tid;
      const bool mine = idx < a.ntiny && a.tiny[idx].word + 3 < end;
      if (__any(mine)) {
        int w = 0, dtype = FKS_F32;
        bool sin_half = false;
        double v = 0.0;
        if (mine) {
          const DevTiny T = a.tiny[idx];
          w = (int)(T.word - base);
          dtype = T.dtype;
          sin_half = (T.flags & kTinySin) != 0;
          v = (double)*reinterpret_cast<pmt_gf32*>(T.ptr);
        }
        for (int k = 0; k < nseeds; k++) {
          // the draw of fks_irregular_kernel's irr_tiny_lane: glibc's log1p and correctly
          // rounded sin / cos (fks_libm.h), static_cast<scalar_t>(double) via float
          const double u1 = pmt_u53(mt_temper(pmt_word(win, k, w)), mt_temper(pmt_word(win, k, w + 1)));
          const double u2 = pmt_u53(mt_temper(pmt_word(win, k, w + 2)), mt_temper(pmt_word(win, k, w + 3)));
          const double r = sqrt(-2.0 * fks_libm::log1p(-u2));
          const double theta = 2.0 * 3.14159265358979323846 * u1;
          const double zd = r * fks_libm::sin_or_cos(theta, sin_half) * 1.0 + 0.0;
          const float zf = (float)zd;
          const float zb = rbf(zf), zh = rhf(zf);
          const float z = dtype == FKS_F32 ? zf : (dtype == FKS_BF16 ? zb : zh);
          const double total = pmt_wave_sum(__fma_rn(v, (double)z, 0.0));
          acc += lane == k ? total : 0.0;
        }
      }
      // block-wide count of `mine` through a few dynamic-LDS words
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
  __syncthreads();  // the windows are free
  double* red = reinterpret_cast<double*>(win);  // [kWaves][kMaxSeedsPerPass]
  if (lane < nseeds) red[(tid >> 6) * kMaxSeedsPerPass + lane] = acc;
  __syncthreads();
  if (tid < nseeds) {
    double s = red[tid];
#pragma unroll
    for (int w = 1; w < kWaves; w++) s += red[w * kMaxSeedsPerPass + tid];
    a.partial[(size_t)c * kPhxSeeds + tid] = s;
  }
}

// ------------------------------------------------------------------ host side
// Once-per-device host setup, as fks_device.hip's: __constant__ memory and function attributes
// belong to the device a call runs on.
class PmtPerDevice {
 public:
  template <class F>
  int run(F&& f) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -FKS_EINVAL;
    const uint64_t bit = 1ull << dev;
    if (done_.load(std::memory_order_acquire) & bit) return 0;
    std::lock_guard<std::mutex> lk(mu_);
    if (done_.load(std::memory_order_relaxed) & bit) return 0;
    const int e = f();
    if (e == 0) done_.fetch_or(bit, std::memory_order_release);
    return e;
  }

 private:
  std::mutex mu_;
  std::atomic<uint64_t> done_{0};
};

// this translation unit's copies of the Box-Muller tables
int pmt_ensure_tables() {
  static PmtPerDevice once;
  return once.run([] {
    const Tables& t = tables();
    static float buf[3 * 2048];  // used under the PmtPerDevice mutex only
    for (int i = 0; i < 256; i++) {
      buf[i] = t.r_bf16[i];
      buf[256 + i] = t.c_bf16[i];
      buf[512 + i] = t.s_bf16[i];
    }
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(c_tab_bf16), buf, sizeof(float) * 768, 0, hipMemcpyHostToDevice);
    if (e != hipSuccess) return (int)e;
    for (int i = 0; i < 2048; i++) {
      buf[i] = t.r_f16[i];
      buf[2048 + i] = t.c_f16[i];
      buf[4096 + i] = t.s_f16[i];
    }
    e = hipMemcpyToSymbol(HIP_SYMBOL(c_pmt_tab_f16), buf, sizeof(buf), 0, hipMemcpyHostToDevice);
    return (int)e;
  });
}

template <class K>
int pmt_lds_attr(PmtPerDevice& once, K* fn, int bytes) {
  return once.run([&] {
    return (int)hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    bytes);
  });
}

template <int DT, bool FULL>
int pmt_launch(const ProjMtArgs& a, void* stream) {
  // a partial pass allocates only its own windows (+1 spare: the twist's last-phase lanes and
  // the idle lanes read past a window)
  const size_t full = (size_t)kLdsTabBytes + (size_t)kLdsStBytes;
  const size_t lds = FULL ? full : (size_t)kLdsTabBytes + (size_t)(a.nseeds + 1) * kWinBytes;
  static PmtPerDevice attr;
  if (int e = pmt_lds_attr(attr, &fks_project_mt_kernel<DT, FULL>, (int)full)) return e;
  hipLaunchKernelGGL((fks_project_mt_kernel<DT, FULL>), dim3((unsigned)a.nchunks), dim3(kApplyThreads), lds,
                     (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

template <int DT>
int pmt_launch_t(const ProjMtArgs& a, void* stream) {
  return a.nseeds == kMaxSeedsPerPass ? pmt_launch<DT, true>(a, stream) : pmt_launch<DT, false>(a, stream);
}

}  // namespace

int launch_project_mt(int dtype, const ProjMtArgs& a, void* stream) {
  if (a.nseeds < 1 || a.nseeds > kMaxSeedsPerPass || a.nchunks < 1 || a.nsegs < 1 || !a.partial || !a.sink)
    return -FKS_EINVAL;
  if (dtype == FKS_BF16) {
    if (int e = pmt_ensure_tables()) return e;
    return pmt_launch_t<FKS_BF16>(a, stream);
  }
  if (dtype == FKS_F32) return pmt_launch_t<FKS_F32>(a, stream);
  if (dtype == kDtF32Libm) return pmt_launch_t<kDtF32Libm>(a, stream);
  return -FKS_ENOTSUP;  // f16 tensors have no fast segments
}

int launch_project_mt_irr(const ProjMtIrrArgs& a, void* stream) {
  if (a.nseeds < 1 || a.nseeds > kMaxSeedsPerPass || a.nchunks < 1 || !a.partial) return -FKS_EINVAL;
  if (int e = pmt_ensure_tables()) return e;
  const size_t lds = (size_t)kPmtLogfOff + kLdsLogfBytes;  // tables | windows | wave counters | logf table
  static PmtPerDevice attr;
  if (int e = pmt_lds_attr(attr, &fks_project_mt_irr_kernel, (int)lds)) return e;
  hipLaunchKernelGGL(fks_project_mt_irr_kernel, dim3((unsigned)a.nchunks), dim3(kApplyThreads), lds,
                     (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // namespace fks
