// fks_gram_mt.hip -- the seed-basis Gram matrix on the CPU generator's MT19937 stream
// (include/fks.h fks_gram_mt): out[r][c] = <z_r, z_c> over the elements one element shard owns,
// both sides drawn in the kernel.  No vector is read and no pointer of the plan is followed: the
// plan is fks_project_mt_multi's geometry-only one.
//
// fks_gram_mt_kernel<DT, FULL> is fks_project_mt_multi_kernel's frame (fks_project_mt.hip): one
// workgroup of kApplyThreads per plan chunk, the chunk-start windows of the pass's seeds in LDS
// -- kGramMtRows row seeds, then kGramMtCols column seeds --, twist_all per MT block, lane
// q < 312 owning the Box-Muller pair (j1, j1 + 8).  Per block a lane draws its row pairs once
// and widens them to f64 -- they stand where that kernel's loaded vectors stand -- and per
// column seed draws one pair and runs that kernel's chain on every row: acc = fma(v1, z.x, acc),
// acc = fma(v2, z.y, acc).  A lane off every segment, and the 8 idle lanes, enter +0 for the row
// values.  fks_gram_mt_irr_kernel visits the irregular frame (fks_dev_irr.h irr_walk) as
// PmtIrrProjectMulti does, the row values drawn: per 16-block pair step and cell the two
// products, the wave's butterfly, and lane m * kGramMtCols + k keeps cell (m, k)'s running sum.
//
// The reduction is the projection's: per cell the 64-lane butterfly, the waves in wave order
// through the LDS the windows occupied, one partial row [kGramRows][kPhxSeeds] per chunk, and
// launch_gram_reduce (fks_project.hip) over the rows of the pass's launches in row order.  So
// element (r, c) is, bit for bit, fks_project_mt_multi of the vector that holds row seed r's
// draw, for column seed c; <z_r, z_c> and <z_c, z_r> are the same products in the same order.
//
// A translation unit of its own (no -fgpu-rdc) with its own instances of the __constant__
// tables, as fks_project_mt.hip.
#include <hip/hip_runtime.h>

#include "fks_internal.h"
#include "fks_gram_mt.h"
#include "fks_dev_lds.h"
#include "fks_dev_mt.h"
#include "fks_dev_zgen.h"
#include "fks_dev_irr.h"
#include "fks_dev_host.h"

namespace fks {
namespace {

constexpr int NR = kGramMtRows, NC = kGramMtCols;

// the waves' sums of one workgroup, [NR][kWaves][NC] f64, go where the first windows were (a
// launch has two windows and a spare one at least)
static_assert(NR * NC * kWaves * 8 <= 3 * kWinBytes, "the waves' sums fit in the first three windows");

// ------------------------------------------------------------------ fast segments
template <int DT, bool FULL>
__global__ __launch_bounds__(kApplyThreads, (kApplyWgPerCu * kApplyThreads + 255) / 256) void fks_gram_mt_kernel(
    GramMtArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds32[];
  uint8_t* lds = reinterpret_cast<uint8_t*>(lds32);
  // the lds_* accessors address LDS by offset from 0: the dynamic block must start there
  if ((uint32_t)(size_t)(lds_u32_t*)lds32 != 0u) __builtin_trap();
  const int tid = threadIdx.x;
  const int c = blockIdx.x;
  const int nr = FULL ? NR : a.nrows, nc = FULL ? NC : a.ncols;
  const int nwin = nr + nc;  // rows' windows first
  const int64_t b0 = a.chunk_block[c], b1 = a.chunk_block[c + 1];

  if constexpr (DT == FKS_BF16) {
    tab_bf16_fill(lds, tid, kApplyThreads);
  } else if constexpr (DT == kDtF32Libm) {
    logf_tab_fill(0u, tid, kApplyThreads);
  }
  for (int idx = tid; idx < nwin * kMtN; idx += kApplyThreads) {
    const int k = idx / kMtN, i = idx - k * kMtN;
    lds_st(kLdsTabBytes + k * kWinBytes + 4 * wperm(i), a.states[((size_t)k * a.nchunks + c) * kMtN + i]);
  }
  TwistPlan plan;
  twist_plan(plan, tid, kLdsTabBytes);
  __syncthreads();

  // Thread q < 312 owns Box-Muller pair q of every block: block words j1 and j1 + 8 (pair_word)
  const bool lane_on = tid < kMtN / 2;
  const int j1 = pair_word(tid);
  const int st_off = pair_off(j1);

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
  auto load_seg = [&]() {  // (selects, not branches: the launcher refuses a launch without segments)
    const bool have = cur < a.nsegs;
    const DevSeg& sg = a.segs[have ? cur : 0];
    const int64_t st = sg.start, n = sg.numel;
    seg_start = have ? st : INT64_MAX;
    seg_end = have ? st + n : INT64_MAX;
  };
  load_seg();

  double acc[NR][NC];  // cell (m, k)'s sum over this lane's elements of the chunk
#pragma unroll
  for (int m = 0; m < NR; m++)
#pragma unroll
    for (int k = 0; k < NC; k++) acc[m][k] = 0.0;

  for (int64_t b = b0; b < b1; b++) {
    __syncthreads();        // every wave is done reading block b-1's words
    twist_all(plan, nwin);  // the raw words of stream block b
    __syncthreads();        // every window holds block b
    const int64_t s1 = (int64_t)kMtN * b + j1;
    while (s1 >= seg_end) { cur++; load_seg(); }
    const bool on = lane_on && s1 >= seg_start;
    // the row values, drawn where the projection loads them; an off lane enters +0
    double v1[NR], v2[NR];
#pragma unroll
    for (int m = 0; m < NR; m++) {
      v1[m] = v2[m] = 0.0;
      if (FULL || m < nr) {
        const uint64_t w = lds_u64(st_off + m * kWinBytes);
        const f32x2_t z = z_pair2<DT>(lds, (uint32_t)w, (uint32_t)(w >> 32));
        v1[m] = on ? (double)z.x : 0.0;
        v2[m] = on ? (double)z.y : 0.0;
      }
    }
    // unrolled with wave-uniform guards: a dynamic index would put acc[] in scratch
#pragma unroll
    for (int k = 0; k < NC; k++) {
      if (FULL || k < nc) {
        const uint64_t w = lds_u64(st_off + (nr + k) * kWinBytes);
        const f32x2_t z = z_pair2<DT>(lds, (uint32_t)w, (uint32_t)(w >> 32));  // once for every row
#pragma unroll
        for (int m = 0; m < NR; m++) {
          if (FULL || m < nr) {
            acc[m][k] = __fma_rn(v1[m], (double)z.x, acc[m][k]);  // exact product, one rounding per addition
            acc[m][k] = __fma_rn(v2[m], (double)z.y, acc[m][k]);
          }
        }
      }
    }
  }

  __syncthreads();  // the windows are free
  double* red = reinterpret_cast<double*>(lds + kLdsTabBytes);  // [NR][kWaves][NC]
#pragma unroll
  for (int m = 0; m < NR; m++)
#pragma unroll
    for (int k = 0; k < NC; k++) {
      if (FULL || (m < nr && k < nc)) {
        const double s = wave_sum(acc[m][k]);
        if (plan.lane == 0) red[(m * kWaves + plan.wave) * NC + k] = s;
      }
    }
  __syncthreads();
  if (tid < NR * NC) {
    const int m = tid / NC, k = tid - m * NC;
    if (m < nr && k < nc) {
      double s = red[m * kWaves * NC + k];
#pragma unroll
      for (int w = 1; w < kWaves; w++) s += red[(m * kWaves + w) * NC + k];
      a.partial[((size_t)c * kGramRows + m) * kPhxSeeds + k] = s;
    }
  }
}

// ------------------------------------------------------------------ irregular work
// One 16-block pair step per lane for every cell of the pass (the whole wave runs this; a lane
// without work draws from the window's word 0 and enters +0 for the row values).  `lim1` / `lim2`
// say that the lane's two elements lie before the run's limit: an element at or past it is
// another run's, and its row value is the +0 the projection enters without reading it.
template <int DT>
__device__ __forceinline__ void gmt_run_cells(const uint8_t* lds, const uint32_t* win, int nr, int nc, int w1, bool lim1,
                                              bool lim2, int lane, double& acc) {
  double v1[NR], v2[NR];
#pragma unroll
  for (int m = 0; m < NR; m++) {
    v1[m] = v2[m] = 0.0;
    if (m < nr) {  // wave-uniform
      float z1, z2;
      irr_z_pair<DT>(lds, win_word(win, m, w1), win_word(win, m, w1 + 8), z1, z2);
      v1[m] = lim1 ? (double)z1 : 0.0;
      v2[m] = lim2 ? (double)z2 : 0.0;
    }
  }
  for (int k = 0; k < nc; k++) {
    float z1, z2;
    irr_z_pair<DT>(lds, win_word(win, nr + k, w1), win_word(win, nr + k, w1 + 8), z1, z2);
#pragma unroll
    for (int m = 0; m < NR; m++) {
      if (m < nr) {
        double part = __fma_rn(v1[m], (double)z1, 0.0);
        part = __fma_rn(v2[m], (double)z2, part);
        const double total = wave_sum(part);
        acc += lane == m * NC + k ? total : 0.0;
      }
    }
  }
}

// The visitor: the whole wave runs when any of its lanes has work (every lane reaches the
// butterflies).
struct GmtIrrGram {
  const GramMtIrrArgs& a;
  int lane;
  double acc;  // lane m * NC + k: this wave's sum for cell (m, k)
  __device__ __forceinline__ void run(const uint8_t* lds, const uint32_t* win, const DevRun& R, bool mine, int64_t e1m,
                                      int w1m) {
    if (__any(mine)) {  // wave-uniform
      const int64_t e1 = mine ? e1m : 0;
      const int w1 = mine ? w1m : 0;
      const bool lim1 = mine && e1 < R.limit, lim2 = mine && e1 + 8 < R.limit;
      switch (R.dtype) {
        case FKS_F32:
          if (a.libm) gmt_run_cells<kDtF32Libm>(lds, win, a.nrows, a.ncols, w1, lim1, lim2, lane, acc);
          else gmt_run_cells<FKS_F32>(lds, win, a.nrows, a.ncols, w1, lim1, lim2, lane, acc);
          break;
        case FKS_BF16: gmt_run_cells<FKS_BF16>(lds, win, a.nrows, a.ncols, w1, lim1, lim2, lane, acc); break;
        default: gmt_run_cells<FKS_F16>(lds, win, a.nrows, a.ncols, w1, lim1, lim2, lane, acc); break;
      }
    }
  }
  // the serial draw in the element's dtype: static_cast<scalar_t>(double) via float
  __device__ __forceinline__ float tiny_z(const uint32_t* win, int k, int w, bool sin_half, int dtype) const {
    const float zf = irr_tiny_z(win, k, w, sin_half);
    const float zb = rbf(zf), zh = rhf(zf);
    return dtype == FKS_F32 ? zf : (dtype == FKS_BF16 ? zb : zh);
  }
  __device__ __forceinline__ void tiny(const uint8_t*, const uint32_t* win, bool mine, int idx, int64_t base) {
    if (__any(mine)) {
      int w = 0, dtype = FKS_F32;
      bool sin_half = false;
      if (mine) {
        const DevTiny T = a.tiny[idx];
        w = (int)(T.word - base);
        dtype = T.dtype;
        sin_half = (T.flags & kTinySin) != 0;
      }
      double v[NR];
#pragma unroll
      for (int m = 0; m < NR; m++) {
        v[m] = 0.0;
        if (m < a.nrows) {
          const float z = tiny_z(win, m, w, sin_half, dtype);
          v[m] = mine ? (double)z : 0.0;
        }
      }
      for (int k = 0; k < a.ncols; k++) {
        const float z = tiny_z(win, a.nrows + k, w, sin_half, dtype);
#pragma unroll
        for (int m = 0; m < NR; m++) {
          if (m < a.nrows) {
            const double total = wave_sum(__fma_rn(v[m], (double)z, 0.0));
            acc += lane == m * NC + k ? total : 0.0;
          }
        }
      }
    }
  }
};

__global__ __launch_bounds__(kApplyThreads) void fks_gram_mt_irr_kernel(GramMtIrrArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds32[];
  const int tid = threadIdx.x;
  const int c = blockIdx.x;
  GmtIrrGram vis{a, tid & 63, 0.0};
  irr_walk(lds32, a, vis);
  __syncthreads();  // the windows are free
  double* red = reinterpret_cast<double*>(reinterpret_cast<uint8_t*>(lds32) + kLdsTabBytes);  // [kWaves][64]
  red[(tid >> 6) * 64 + vis.lane] = vis.acc;
  __syncthreads();
  if (tid < NR * NC) {
    const int m = tid / NC, k = tid - m * NC;
    if (m < a.nrows && k < a.ncols) {
      double s = red[tid];
#pragma unroll
      for (int w = 1; w < kWaves; w++) s += red[w * 64 + tid];
      a.partial[((size_t)c * kGramRows + m) * kPhxSeeds + k] = s;
    }
  }
}
static_assert(kWaves * 64 * 8 <= kIrrWin * 4 * 2, "the waves' sums fit in the irregular frame's first windows");

// ------------------------------------------------------------------ host side
template <int DT, bool FULL>
int gmt_launch(const GramMtArgs& a, void* stream) {
  // a pass allocates its own windows + 1 spare (the twist's last-phase lanes and the idle lanes
  // read past a window)
  const size_t full = (size_t)kLdsTabBytes + (size_t)(NR + NC + 1) * kWinBytes;
  const size_t lds = (size_t)kLdsTabBytes + (size_t)(a.nrows + a.ncols + 1) * kWinBytes;
  static PerDevice attr;
  if (int e = ensure_lds_attr(attr, &fks_gram_mt_kernel<DT, FULL>, (int)full)) return e;
  hipLaunchKernelGGL((fks_gram_mt_kernel<DT, FULL>), dim3((unsigned)a.nchunks), dim3(kApplyThreads), lds,
                     (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

template <int DT>
int gmt_launch_t(const GramMtArgs& a, void* stream) {
  return a.nrows == NR && a.ncols == NC ? gmt_launch<DT, true>(a, stream) : gmt_launch<DT, false>(a, stream);
}

}  // namespace

int launch_gram_mt(int dtype, const GramMtArgs& a, void* stream) {
  if (a.nrows < 1 || a.nrows > NR || a.ncols < 1 || a.ncols > NC || a.nchunks < 1 || a.nsegs < 1 || !a.partial ||
      !a.states)
    return -FKS_EINVAL;
  if (dtype == FKS_BF16) {
    if (int e = ensure_tables()) return e;
    return gmt_launch_t<FKS_BF16>(a, stream);
  }
  if (dtype == FKS_F32) return gmt_launch_t<FKS_F32>(a, stream);
  if (dtype == kDtF32Libm) return gmt_launch_t<kDtF32Libm>(a, stream);
  return -FKS_ENOTSUP;  // f16 tensors have no fast segments
}

int launch_gram_mt_irr(const GramMtIrrArgs& a, void* stream) {
  if (a.nrows < 1 || a.nrows > NR || a.ncols < 1 || a.ncols > NC || a.nseeds != a.nrows + a.ncols || a.nchunks < 1 ||
      !a.partial || !a.states)
    return -FKS_EINVAL;
  if (int e = ensure_tables()) return e;
  const size_t lds = (size_t)kIrrLogfOff + kLdsLogfBytes;  // tables | windows | wave counters | logf table
  static PerDevice attr;
  if (int e = ensure_lds_attr(attr, &fks_gram_mt_irr_kernel, (int)lds)) return e;
  hipLaunchKernelGGL(fks_gram_mt_irr_kernel, dim3((unsigned)a.nchunks), dim3(kApplyThreads), lds, (hipStream_t)stream,
                     a);
  return (int)hipGetLastError();
}

}  // namespace fks
