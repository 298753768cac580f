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
// fks_project_mt_multi_kernel<DT, FULL, NV, NS> and fks_project_mt_irr_multi_kernel<NV>
// (include/fks.h fks_project_mt_multi, fks_project_mt.h) are the same two kernels for NV vectors
// read where they lie, each in its own dtype: the plan is the geometry-only one and a per-call
// table names every vector's piece under every segment, run and single element.  The generator
// runs once per seed for all NV vectors; every vector keeps the order above, so its row is what
// the one-buffer kernels return for it.  A pass of NV vectors carries NS seeds (fks_project_mt.h).
//
// A translation unit of its own (no -fgpu-rdc), so that the hot kernels' device object is not
// rebuilt with these.  What it has in common with the update kernels exists once as text, in
// the layers both units include: the irregular frame (fks_dev_irr.h: the carry windows, the
// in-place twist, the run and single-element cursors, the serial draw), the fast-segment
// prologue pieces (fks_dev_mt.h, fks_dev_zgen.h) and the once-per-device host setup
// (fks_dev_host.h).  What is per unit are the instances: this unit's own c_tab_bf16 and
// c_tab_f16 in constant memory, filled per device by its own ensure_tables().
#include <hip/hip_runtime.h>

#include "fks_internal.h"
#include "fks_project_mt.h"
#include "fks_dev_lds.h"
#include "fks_dev_mt.h"
#include "fks_dev_zgen.h"
#include "fks_dev_irr.h"
#include "fks_dev_host.h"

namespace fks {
namespace {

typedef __attribute__((address_space(1))) const float pmt_gf32;

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
    tab_bf16_fill(lds, tid, kApplyThreads);
  } else if constexpr (DT == kDtF32Libm) {
    logf_tab_fill(0u, tid, kApplyThreads);
  }
  // (this loop and the bisection below are fks_apply_kernel's lines, kept as text in both: as a
  // shared function either of them reorders both kernels' instructions, and this kernel then
  // measured 0.7 % (bf16) to 2 % (fp32) slower, profiles/r12_irr_frame_ab.log)
  for (int idx = tid; idx < nseeds * kMtN; idx += kApplyThreads) {
    const int k = idx / kMtN, i = idx - k * kMtN;
    lds_st(kLdsTabBytes + k * kWinBytes + 4 * wperm(i), a.states[((size_t)k * a.nchunks + c) * kMtN + i]);
  }
  TwistPlan plan;
  twist_plan(plan, tid, kLdsTabBytes);
  __syncthreads();

  // Thread q < 312 owns Box-Muller pair q of every block: block words j1 and j1 + 8 (pair_word)
  const bool lane_on = tid < kMtN / 2;
  const int j1 = pair_word(tid);
  const int st_off = pair_off(j1);  // the (j1, j1 + 8) word pair

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
      const double s = wave_sum(acc[k]);
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

// ------------------------------------------------------------------ fast segments, in place
// fks_project_mt_multi (fks_project_mt.h): NV vectors share the pass, each read where it lies.
// The plan is the geometry-only one -- its segments' pointers are not read -- and a.pv names
// vector m's piece under segment `cur` and its dtype, looked up when the lane's segment
// advances.  The twist, the window reads and z_pair2 run once per seed for all vectors; every
// vector has the kernel above's fma chain, butterfly and wave order of its own, so row m is
// what the kernel above returns for vector m laid out as one f32 buffer.  NS is the seeds such
// a pass carries (FULL: exactly NS): NV x NS f64 sums per lane.
// (The kernel above is not the NV = 1 instance of this template with a second fetch policy:
// built that way its own instructions moved -- loads swapped, 83 to 2,053 lines of each
// instance -- and it is the kernel the pinned bits and the published rates belong to.)
typedef __attribute__((address_space(1))) const uint16_t pmt_gu16;

static_assert(kProjMtMaxVec * kPmtRedBytes <= 2 * kWinBytes, "the vectors' sums fit in the first two windows");

// element `e` of a vector piece, widened to f32 exactly
__device__ __forceinline__ float pmt_load(uint64_t ptr, int dtype, int64_t e) {
  if (dtype == FKS_F32) return *reinterpret_cast<pmt_gf32*>(ptr + (uint64_t)e * 4u);
  const uint32_t h = *reinterpret_cast<pmt_gu16*>(ptr + (uint64_t)e * 2u);
  const _Float16 f = __builtin_bit_cast(_Float16, (uint16_t)h);
  return dtype == FKS_BF16 ? __uint_as_float(h << 16) : (float)f;
}

template <int DT, bool FULL, int NV, int NS>
__global__ __launch_bounds__(kApplyThreads, (kApplyWgPerCu * kApplyThreads + 255) / 256) void fks_project_mt_multi_kernel(
    ProjMtMultiArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds32[];
  uint8_t* lds = reinterpret_cast<uint8_t*>(lds32);
  if ((uint32_t)(size_t)(lds_u32_t*)lds32 != 0u) __builtin_trap();
  const int tid = threadIdx.x;
  const int c = blockIdx.x;
  const int nseeds = FULL ? NS : a.nseeds;
  const int64_t b0 = a.chunk_block[c], b1 = a.chunk_block[c + 1];

  if constexpr (DT == FKS_BF16) {
    tab_bf16_fill(lds, tid, kApplyThreads);
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

  const bool lane_on = tid < kMtN / 2;
  const int j1 = pair_word(tid);
  const int st_off = pair_off(j1);

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
  uint64_t seg_ptr[NV];  // vector m's piece under segment `cur`
  int seg_dt[NV];
  auto load_seg = [&]() {
    const bool have = cur < a.nsegs;
    const DevSeg& sg = a.segs[have ? cur : 0];
    const int64_t st = sg.start, n = sg.numel;
    seg_start = have ? st : INT64_MAX;
    seg_end = have ? st + n : INT64_MAX;
#pragma unroll
    for (int m = 0; m < NV; m++) {
      const ProjMtVecEntry& e = a.pv[(int64_t)m * a.stride + (have ? cur : 0)];
      seg_ptr[m] = e.ptr;
      seg_dt[m] = e.dtype;
    }
  };
  load_seg();

  // The same software pipeline: block b+1's elements are fetched before block b's Box-Muller and
  // widened one iteration later.  The loads must not depend on the dtype by a branch -- a load
  // under a branch is waited for where the branch ends, which puts the memory latency of every
  // vector on every block (one f32 vector in place then measured 1.29 of fks_project_mt, two
  // vectors 1.21 of two launches) -- so every element is two 16-bit loads whatever its dtype: the
  // halves of an f32 element, or a 2-byte element twice.  A lane off every segment loads the sink
  // as f32 and enters +0.
  struct Raw { uint32_t lo1[NV], hi1[NV], lo2[NV], hi2[NV]; uint32_t meta; };  // meta: on | dtype m << (1 + 2 m)
  auto fetch = [&](int64_t b) -> Raw {
    Raw r;
    const int64_t s1 = (int64_t)kMtN * b + j1;
    while (s1 >= seg_end) { cur++; load_seg(); }
    const bool on = lane_on && s1 >= seg_start;
    const uint64_t e = on ? (uint64_t)(s1 - seg_start) : 0u;
    r.meta = on;
#pragma unroll
    for (int m = 0; m < NV; m++) {
      const uint64_t ptr = on ? seg_ptr[m] : (uint64_t)(uintptr_t)a.sink;
      const uint32_t dt = on ? (uint32_t)seg_dt[m] : (uint32_t)FKS_F32;
      const bool wide = dt == (uint32_t)FKS_F32;
      const uint64_t p1 = ptr + (e << (wide ? 2 : 1)), p2 = p1 + (wide ? 32u : 16u), half = wide ? 2u : 0u;
      r.lo1[m] = *reinterpret_cast<pmt_gu16*>(p1);
      r.hi1[m] = *reinterpret_cast<pmt_gu16*>(p1 + half);
      r.lo2[m] = *reinterpret_cast<pmt_gu16*>(p2);
      r.hi2[m] = *reinterpret_cast<pmt_gu16*>(p2 + half);
      r.meta |= dt << (1 + 2 * m);
    }
    return r;
  };
  auto widen = [](uint32_t lo, uint32_t hi, uint32_t dt) -> float {  // exact, by selects
    const float hf = (float)__builtin_bit_cast(_Float16, (uint16_t)lo);
    const float w = __uint_as_float(dt == (uint32_t)FKS_F32 ? (lo | (hi << 16)) : (lo << 16));
    return dt == (uint32_t)FKS_F16 ? hf : w;
  };

  double acc[NV][NS];  // vector m's sum for seed k over this lane's elements of the chunk
#pragma unroll
  for (int m = 0; m < NV; m++)
#pragma unroll
    for (int k = 0; k < NS; k++) acc[m][k] = 0.0;

  Raw nxt = fetch(b0);
  for (int64_t b = b0; b < b1; b++) {
    __syncthreads();
    twist_all(plan, nseeds);
    __syncthreads();
    const Raw sa = nxt;
    double v1[NV], v2[NV];
#pragma unroll
    for (int m = 0; m < NV; m++) {
      const uint32_t dt = (sa.meta >> (1 + 2 * m)) & 3u;
      v1[m] = (sa.meta & 1u) ? (double)widen(sa.lo1[m], sa.hi1[m], dt) : 0.0;
      v2[m] = (sa.meta & 1u) ? (double)widen(sa.lo2[m], sa.hi2[m], dt) : 0.0;
    }
    nxt = fetch(b + 1 < b1 ? b + 1 : b);  // (the last block re-reads itself, unused)
#pragma unroll
    for (int k = 0; k < NS; k++) {
      if (FULL || k < nseeds) {
        const uint64_t w = lds_u64(st_off + k * kWinBytes);
        const f32x2_t z = z_pair2<DT>(lds, (uint32_t)w, (uint32_t)(w >> 32));  // once for every vector
#pragma unroll
        for (int m = 0; m < NV; m++) {
          acc[m][k] = __fma_rn(v1[m], (double)z.x, acc[m][k]);
          acc[m][k] = __fma_rn(v2[m], (double)z.y, acc[m][k]);
        }
      }
    }
  }

  __syncthreads();  // the windows are free (a launch has its seeds' and a spare one: two at least)
  double* red = reinterpret_cast<double*>(lds + kLdsTabBytes);  // [NV][kWaves][NS]
#pragma unroll
  for (int m = 0; m < NV; m++)
#pragma unroll
    for (int k = 0; k < NS; k++) {
      if (FULL || k < nseeds) {
        const double s = wave_sum(acc[m][k]);
        if (plan.lane == 0) red[(m * kWaves + plan.wave) * NS + k] = s;
      }
    }
  __syncthreads();
  if (tid < nseeds) {
#pragma unroll
    for (int m = 0; m < NV; m++) {
      double s = red[m * kWaves * NS + tid];
#pragma unroll
      for (int w = 1; w < kWaves; w++) s += red[(m * kWaves + w) * NS + tid];
      a.partial[((size_t)c * NV + m) * kPhxSeeds + tid] = s;
    }
  }
}

// ------------------------------------------------------------------ irregular work
// fks_irregular_kernel's frame (fks_dev_irr.h irr_walk), visited to sum instead of to update.
// Every seed of the pass over one 16-block pair per lane (the whole wave runs this; a lane
// without work has x1 = x2 = +0 and reads the window's word 0): lane k collects seed k's sum.
template <int DT>
__device__ __forceinline__ void pmt_run_seeds(const uint8_t* lds, const uint32_t* win, int nseeds, int w1, float x1,
                                              float x2, int lane, double& acc) {
  const double v1 = (double)x1, v2 = (double)x2;
  for (int k = 0; k < nseeds; k++) {
    float z1, z2;
    irr_z_pair<DT>(lds, win_word(win, k, w1), win_word(win, k, w1 + 8), z1, z2);
    double part = __fma_rn(v1, (double)z1, 0.0);
    part = __fma_rn(v2, (double)z2, part);
    const double total = wave_sum(part);
    acc += lane == k ? total : 0.0;
  }
}

static_assert(kMaxSeedsPerPass <= 64, "lane k of a wave keeps seed k's sum");

// The projection visitor: the whole wave runs when any of its lanes has work (every lane
// reaches the butterflies); a lane without work enters +0 and reads word 0 of the window.
struct PmtIrrProject {
  const ProjMtIrrArgs& a;
  int lane;
  double acc;  // lane k < nseeds: this wave's sum for seed k
  __device__ __forceinline__ void run(const uint8_t* lds, const uint32_t* win, const DevRun& R, bool mine, int64_t e1m,
                                      int w1m) {
    if (__any(mine)) {  // wave-uniform
      const int64_t e1 = mine ? e1m : 0;
      const int w1 = mine ? w1m : 0;
      float x1 = 0.0f, x2 = 0.0f;  // elements at or past the limit are another run's: not read
      if (mine && e1 < R.limit) x1 = reinterpret_cast<pmt_gf32*>(R.ptr)[e1];
      if (mine && e1 + 8 < R.limit) x2 = reinterpret_cast<pmt_gf32*>(R.ptr)[e1 + 8];
      switch (R.dtype) {
        case FKS_F32:
          if (a.libm) pmt_run_seeds<kDtF32Libm>(lds, win, a.nseeds, w1, x1, x2, lane, acc);
          else pmt_run_seeds<FKS_F32>(lds, win, a.nseeds, w1, x1, x2, lane, acc);
          break;
        case FKS_BF16: pmt_run_seeds<FKS_BF16>(lds, win, a.nseeds, w1, x1, x2, lane, acc); break;
        default: pmt_run_seeds<FKS_F16>(lds, win, a.nseeds, w1, x1, x2, lane, acc); break;
      }
    }
  }
  __device__ __forceinline__ void tiny(const uint8_t*, const uint32_t* win, bool mine, int idx, int64_t base) {
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
      for (int k = 0; k < a.nseeds; k++) {
        const float zf = irr_tiny_z(win, k, w, sin_half);  // static_cast<scalar_t>(double) via float
        const float zb = rbf(zf), zh = rhf(zf);
        const float z = dtype == FKS_F32 ? zf : (dtype == FKS_BF16 ? zb : zh);
        const double total = wave_sum(__fma_rn(v, (double)z, 0.0));
        acc += lane == k ? total : 0.0;
      }
    }
  }
};

__global__ __launch_bounds__(kApplyThreads) void fks_project_mt_irr_kernel(ProjMtIrrArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds32[];
  const int tid = threadIdx.x;
  const int c = blockIdx.x;
  const int nseeds = a.nseeds;
  PmtIrrProject vis{a, tid & 63, 0.0};
  irr_walk(lds32, a, vis);
  __syncthreads();  // the windows are free
  double* red = reinterpret_cast<double*>(reinterpret_cast<uint8_t*>(lds32) + kLdsTabBytes);  // [kWaves][kMaxSeedsPerPass]
  if (vis.lane < nseeds) red[(tid >> 6) * kMaxSeedsPerPass + vis.lane] = vis.acc;
  __syncthreads();
  if (tid < nseeds) {
    double s = red[tid];
#pragma unroll
    for (int w = 1; w < kWaves; w++) s += red[w * kMaxSeedsPerPass + tid];
    a.partial[(size_t)c * kPhxSeeds + tid] = s;
  }
}

// ------------------------------------------------------------------ irregular work, in place
// The same walk for NV vectors read where they lie: a.rv / a.tv name every vector's piece under
// every run / single element.  The z of a seed are drawn once; every vector has its own
// butterfly per seed, and lane k keeps one f64 per vector.
template <int DT, int NV>
__device__ __forceinline__ void pmt_run_seeds_multi(const uint8_t* lds, const uint32_t* win, int nseeds, int w1,
                                                    const float (&x1)[NV], const float (&x2)[NV], int lane,
                                                    double (&acc)[NV]) {
  double v1[NV], v2[NV];
#pragma unroll
  for (int m = 0; m < NV; m++) v1[m] = (double)x1[m], v2[m] = (double)x2[m];
  for (int k = 0; k < nseeds; k++) {
    float z1, z2;
    irr_z_pair<DT>(lds, win_word(win, k, w1), win_word(win, k, w1 + 8), z1, z2);
#pragma unroll
    for (int m = 0; m < NV; m++) {
      double part = __fma_rn(v1[m], (double)z1, 0.0);
      part = __fma_rn(v2[m], (double)z2, part);
      const double total = wave_sum(part);
      acc[m] += lane == k ? total : 0.0;
    }
  }
}

template <int NV>
struct PmtIrrProjectMulti {
  const ProjMtIrrMultiArgs& a;
  int lane;
  int rcur;        // no run before this one starts at or after the last run visited
  double acc[NV];  // lane k < nseeds: this wave's sum for seed k, per vector
  __device__ __forceinline__ void run(const uint8_t* lds, const uint32_t* win, const DevRun& R, bool mine, int64_t e1m,
                                      int w1m) {
    if (__any(mine)) {  // wave-uniform
      const int64_t e1 = mine ? e1m : 0;
      const int w1 = mine ? w1m : 0;
      // the walk hands over a copy of the run: its index is found by its start (the runs are
      // disjoint, sorted by start, and visited in that order)
      int lo = rcur, hi = a.nruns;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.runs[mid].start < R.start) lo = mid + 1; else hi = mid;
      }
      rcur = lo;
      float x1[NV], x2[NV];  // elements at or past the limit are another run's: not read
#pragma unroll
      for (int m = 0; m < NV; m++) {
        x1[m] = x2[m] = 0.0f;
        if (lo < a.nruns) {
          const ProjMtVecEntry e = a.rv[(int64_t)m * a.stride + lo];
          if (mine && e1 < R.limit) x1[m] = pmt_load(e.ptr, e.dtype, e1);
          if (mine && e1 + 8 < R.limit) x2[m] = pmt_load(e.ptr, e.dtype, e1 + 8);
        }
      }
      switch (R.dtype) {
        case FKS_F32:
          if (a.libm) pmt_run_seeds_multi<kDtF32Libm, NV>(lds, win, a.nseeds, w1, x1, x2, lane, acc);
          else pmt_run_seeds_multi<FKS_F32, NV>(lds, win, a.nseeds, w1, x1, x2, lane, acc);
          break;
        case FKS_BF16: pmt_run_seeds_multi<FKS_BF16, NV>(lds, win, a.nseeds, w1, x1, x2, lane, acc); break;
        default: pmt_run_seeds_multi<FKS_F16, NV>(lds, win, a.nseeds, w1, x1, x2, lane, acc); break;
      }
    }
  }
  __device__ __forceinline__ void tiny(const uint8_t*, const uint32_t* win, bool mine, int idx, int64_t base) {
    if (__any(mine)) {
      int w = 0, dtype = FKS_F32;
      bool sin_half = false;
      double v[NV];
#pragma unroll
      for (int m = 0; m < NV; m++) v[m] = 0.0;
      if (mine) {
        const DevTiny T = a.tiny[idx];
        w = (int)(T.word - base);
        dtype = T.dtype;
        sin_half = (T.flags & kTinySin) != 0;
#pragma unroll
        for (int m = 0; m < NV; m++) {
          const ProjMtVecEntry e = a.tv[(int64_t)m * a.stride + idx];
          v[m] = (double)pmt_load(e.ptr, e.dtype, 0);
        }
      }
      for (int k = 0; k < a.nseeds; k++) {
        const float zf = irr_tiny_z(win, k, w, sin_half);
        const float zb = rbf(zf), zh = rhf(zf);
        const float z = dtype == FKS_F32 ? zf : (dtype == FKS_BF16 ? zb : zh);
#pragma unroll
        for (int m = 0; m < NV; m++) {
          const double total = wave_sum(__fma_rn(v[m], (double)z, 0.0));
          acc[m] += lane == k ? total : 0.0;
        }
      }
    }
  }
};

template <int NV>
__global__ __launch_bounds__(kApplyThreads) void fks_project_mt_irr_multi_kernel(ProjMtIrrMultiArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds32[];
  const int tid = threadIdx.x;
  const int c = blockIdx.x;
  const int nseeds = a.nseeds;
  PmtIrrProjectMulti<NV> vis{a, tid & 63, 0, {}};
  irr_walk(lds32, a, vis);
  __syncthreads();  // the windows are free
  double* red = reinterpret_cast<double*>(reinterpret_cast<uint8_t*>(lds32) + kLdsTabBytes);  // [NV][kWaves][kMaxSeedsPerPass]
#pragma unroll
  for (int m = 0; m < NV; m++)
    if (vis.lane < nseeds) red[(m * kWaves + (tid >> 6)) * kMaxSeedsPerPass + vis.lane] = vis.acc[m];
  __syncthreads();
  if (tid < nseeds) {
#pragma unroll
    for (int m = 0; m < NV; m++) {
      double s = red[m * kWaves * kMaxSeedsPerPass + tid];
#pragma unroll
      for (int w = 1; w < kWaves; w++) s += red[(m * kWaves + w) * kMaxSeedsPerPass + tid];
      a.partial[((size_t)c * NV + m) * kPhxSeeds + tid] = s;
    }
  }
}

// ------------------------------------------------------------------ host side
template <int DT, bool FULL>
int pmt_launch(const ProjMtArgs& a, void* stream) {
  // a partial pass allocates only its own windows (+1 spare: the twist's last-phase lanes and
  // the idle lanes read past a window)
  const size_t full = (size_t)kLdsTabBytes + (size_t)kLdsStBytes;
  const size_t lds = FULL ? full : (size_t)kLdsTabBytes + (size_t)(a.nseeds + 1) * kWinBytes;
  static PerDevice attr;
  if (int e = ensure_lds_attr(attr, &fks_project_mt_kernel<DT, FULL>, (int)full)) return e;
  hipLaunchKernelGGL((fks_project_mt_kernel<DT, FULL>), dim3((unsigned)a.nchunks), dim3(kApplyThreads), lds,
                     (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

template <int DT>
int pmt_launch_t(const ProjMtArgs& a, void* stream) {
  return a.nseeds == kMaxSeedsPerPass ? pmt_launch<DT, true>(a, stream) : pmt_launch<DT, false>(a, stream);
}

template <int DT, bool FULL, int NV>
int pmt_multi_launch(const ProjMtMultiArgs& a, void* stream) {
  constexpr int NS = proj_mt_pass_seeds(NV);
  const size_t full = (size_t)kLdsTabBytes + (size_t)(NS + 1) * kWinBytes;
  const size_t lds = (size_t)kLdsTabBytes + (size_t)(a.nseeds + 1) * kWinBytes;  // its own windows + 1 spare
  static PerDevice attr;
  if (int e = ensure_lds_attr(attr, &fks_project_mt_multi_kernel<DT, FULL, NV, NS>, (int)full)) return e;
  hipLaunchKernelGGL((fks_project_mt_multi_kernel<DT, FULL, NV, NS>), dim3((unsigned)a.nchunks), dim3(kApplyThreads),
                     lds, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

template <int NV>
int pmt_multi_launch_d(int dtype, const ProjMtMultiArgs& a, void* stream) {
  constexpr int NS = proj_mt_pass_seeds(NV);
  if (a.nseeds < 1 || a.nseeds > NS || a.nchunks < 1 || a.nsegs < 1 || !a.partial || !a.sink || !a.pv ||
      a.stride < a.nsegs)
    return -FKS_EINVAL;
  const bool full = a.nseeds == NS;
  if (dtype == FKS_BF16) {
    if (int e = ensure_tables()) return e;
    return full ? pmt_multi_launch<FKS_BF16, true, NV>(a, stream) : pmt_multi_launch<FKS_BF16, false, NV>(a, stream);
  }
  if (dtype == FKS_F32)
    return full ? pmt_multi_launch<FKS_F32, true, NV>(a, stream) : pmt_multi_launch<FKS_F32, false, NV>(a, stream);
  if (dtype == kDtF32Libm)
    return full ? pmt_multi_launch<kDtF32Libm, true, NV>(a, stream)
                : pmt_multi_launch<kDtF32Libm, false, NV>(a, stream);
  return -FKS_ENOTSUP;  // f16 tensors have no fast segments
}

template <int NV>
int pmt_multi_launch_irr(const ProjMtIrrMultiArgs& a, void* stream) {
  if (a.nseeds < 1 || a.nseeds > proj_mt_pass_seeds(NV) || a.nchunks < 1 || !a.partial ||
      (a.nruns > 0 && !a.rv) || (a.ntiny > 0 && !a.tv))
    return -FKS_EINVAL;
  if (int e = ensure_tables()) return e;
  const size_t lds = (size_t)kIrrLogfOff + kLdsLogfBytes;  // tables | windows | wave counters | logf table
  static PerDevice attr;
  if (int e = ensure_lds_attr(attr, &fks_project_mt_irr_multi_kernel<NV>, (int)lds)) return e;
  hipLaunchKernelGGL((fks_project_mt_irr_multi_kernel<NV>), dim3((unsigned)a.nchunks), dim3(kApplyThreads), lds,
                     (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // namespace

// the in-place instances, by the number of vectors in the pass
int launch_project_mt_multi(int dtype, const ProjMtMultiArgs& a, void* stream) {
  switch (a.nvec) {
    case 1: return pmt_multi_launch_d<1>(dtype, a, stream);
#if FKS_PMT_MAX_VEC >= 2
    case 2: return pmt_multi_launch_d<2>(dtype, a, stream);
#endif
#if FKS_PMT_MAX_VEC >= 3
    case 3: return pmt_multi_launch_d<3>(dtype, a, stream);
#endif
#if FKS_PMT_MAX_VEC >= 4
    case 4: return pmt_multi_launch_d<4>(dtype, a, stream);
#endif
    default: return -FKS_EINVAL;
  }
}

int launch_project_mt_irr_multi(const ProjMtIrrMultiArgs& a, void* stream) {
  switch (a.nvec) {
    case 1: return pmt_multi_launch_irr<1>(a, stream);
#if FKS_PMT_MAX_VEC >= 2
    case 2: return pmt_multi_launch_irr<2>(a, stream);
#endif
#if FKS_PMT_MAX_VEC >= 3
    case 3: return pmt_multi_launch_irr<3>(a, stream);
#endif
#if FKS_PMT_MAX_VEC >= 4
    case 4: return pmt_multi_launch_irr<4>(a, stream);
#endif
    default: return -FKS_EINVAL;
  }
}

int launch_project_mt(int dtype, const ProjMtArgs& a, void* stream) {
  if (a.nseeds < 1 || a.nseeds > kMaxSeedsPerPass || a.nchunks < 1 || a.nsegs < 1 || !a.partial || !a.sink)
    return -FKS_EINVAL;
  if (dtype == FKS_BF16) {
    if (int e = ensure_tables()) return e;
    return pmt_launch_t<FKS_BF16>(a, stream);
  }
  if (dtype == FKS_F32) return pmt_launch_t<FKS_F32>(a, stream);
  if (dtype == kDtF32Libm) return pmt_launch_t<kDtF32Libm>(a, stream);
  return -FKS_ENOTSUP;  // f16 tensors have no fast segments
}

int launch_project_mt_irr(const ProjMtIrrArgs& a, void* stream) {
  if (a.nseeds < 1 || a.nseeds > kMaxSeedsPerPass || a.nchunks < 1 || !a.partial) return -FKS_EINVAL;
  if (int e = ensure_tables()) return e;
  const size_t lds = (size_t)kIrrLogfOff + kLdsLogfBytes;  // tables | windows | wave counters | logf table
  static PerDevice attr;
  if (int e = ensure_lds_attr(attr, &fks_project_mt_irr_kernel, (int)lds)) return e;
  hipLaunchKernelGGL(fks_project_mt_irr_kernel, dim3((unsigned)a.nchunks), dim3(kApplyThreads), lds,
                     (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // namespace fks
