// fks_gram_mt_tiled.hip -- the tiled seed-basis Gram matrix on the CPU generator's MT19937 stream
// (include/fks.h fks_gram_mt_tiled, fks_gram_mt_tiled.h): G[r][c] = <z_r, z_c> for a tile of 16
// row seeds by 16 column seeds per pass, the 256 sums on the f64 matrix unit.
//
// fks_gram_mt_tiled_kernel<DT> is fks_gram_mt_kernel's frame (fks_gram_mt.hip): one workgroup of
// kApplyThreads per plan chunk, the chunk-start windows of the pass's seeds in LDS -- the row
// block's, then the column block's; a diagonal tile has the row block's only --, twist_all per MT
// block, lane q < 312 drawing the Box-Muller pair (j1, j1 + 8) of every seed.  That leaves a lane
// with all seeds of its own two elements, and v_mfma_f64_16x16x4_f64 wants lane l to hold seed
// l & 15 of element l >> 4 (A[l & 15][l >> 4] and B[l >> 4][l & 15], one f64 each): the transpose
// goes through a wave-private staging area in LDS.
//   * A wave stages the z of its own 64 lanes as f32 (exact for every dtype), one row of 64 + 4
//     words per (half of the pair, seed): lane e writes word e of row h * 16 + m, consecutive
//     words, no bank conflict.  A lane off every segment, and the 8 idle lanes, stage +0.
//   * Lane l reads words 16 q + 4 (l >> 4) .. + 3, q < 4, of the two rows of seed l & 15 with
//     ds_read_b128: 32 values, the operands of 32 MFMAs.  The rows' pitch of 68 words puts the 16
//     seeds of a quarter wave on the 64 banks once.  Which element meets which MFMA and k is the
//     same for the row and the column operand, and that is all a sum needs.
//   * The row block is staged and read into registers first; the column block then takes the same
//     area (a diagonal tile takes the row block's registers and draws 16 windows, not 32).
// A wave's LDS operations execute in order, so the hand-off between its lanes needs no barrier:
// a compiler fence keeps the program order.  No cross-wave traffic before the final reduction.
//
// The accumulators (4 f64 per lane) stay in registers over the chunk's blocks.  At the end the
// waves are added in wave order through LDS and the workgroup leaves one partial tile per chunk in
// the f64 result map's order (col = lane & 15, row = (lane >> 4) + 4 reg);
// fks_gram_mt_tiled_reduce_kernel adds the chunks' partials of the pass's launches, then those of
// the irregular sub-passes (fks_gram_mt_irr_kernel over the tile, fks_run_basis.cpp), in one fixed
// order.  Every accumulator sees the same sequence of operations whatever its place in the tile
// and whatever the other seeds, so an element depends on the device, the tensor list, the shard
// and its two seeds only; <z_r, z_c> and <z_c, z_r> are the same products in the same order.
//
// A translation unit of its own (no -fgpu-rdc) with its own instances of the __constant__
// tables, as fks_gram_mt.hip.
#include <hip/hip_runtime.h>

#include "fks_internal.h"
#include "fks_gram_mt_tiled.h"
#include "fks_dev_lds.h"
#include "fks_dev_mt.h"
#include "fks_dev_zgen.h"
#include "fks_dev_irr.h"
#include "fks_dev_host.h"

namespace fks {
namespace {

typedef double f64x4_t __attribute__((ext_vector_type(4)));

constexpr int T = kGmtTile;
// twist_all serves kWinPerWave windows per wave: the windows past the first kTwistWindows take a
// second plan whose window 0 is window kTwistWindows
constexpr int kTwistWindows = kWinPerWave * kWaves;
static_assert(kGmtWindows <= 2 * kTwistWindows, "two twist plans cover the tile's windows");
// LDS: tables | kGmtWindows windows + 1 spare (the twist's last-phase lanes and the idle lanes
// read past a window) | one staging area per wave
constexpr int kStageRowWords = 64 + 4;
constexpr int kStageRowBytes = 4 * kStageRowWords;
constexpr int kStageWaveBytes = 2 * T * kStageRowBytes;  // (half, seed) rows of one 16-seed block
constexpr int kStageOff = kLdsTabBytes + (kGmtWindows + 1) * kWinBytes;
constexpr int kGmtLdsBytes = kStageOff + kWaves * kStageWaveBytes;
static_assert(kStageOff % 16 == 0 && kStageRowBytes % 16 == 0, "ds_read_b128 alignment");
static_assert(kGmtLdsBytes <= 160 * 1024, "one workgroup fits the CU's LDS");
static_assert(4 * 64 * 8 <= kStageWaveBytes, "a wave's accumulators fit its staging area");
static_assert(kGmtCells <= kApplyThreads, "one thread per cell writes the partial");

__device__ __forceinline__ void wave_fence() { asm volatile("" ::: "memory"); }

// the z of `n` seeds from window win0 on, staged by this lane: word `lane` of rows h * 16 + m
template <int DT>
__device__ __forceinline__ void gmt_stage(const uint8_t* lds, int st_off, int win0, int n, bool on, int stage_w) {
  // two seeds per step, for two independent chains; an odd count's last step takes its seed twice
#pragma unroll 1
  for (int m = 0; m < n; m += 2) {
    const int m2 = m + 1 < n ? m + 1 : m;
    const uint64_t w = lds_u64(st_off + (win0 + m) * kWinBytes);
    const uint64_t w2 = lds_u64(st_off + (win0 + m2) * kWinBytes);
    const f32x2_t z = z_pair2<DT>(lds, (uint32_t)w, (uint32_t)(w >> 32));
    const f32x2_t z2 = z_pair2<DT>(lds, (uint32_t)w2, (uint32_t)(w2 >> 32));
    lds_st(stage_w + m * kStageRowBytes, __float_as_uint(on ? z.x : 0.0f));
    lds_st(stage_w + (T + m) * kStageRowBytes, __float_as_uint(on ? z.y : 0.0f));
    lds_st(stage_w + m2 * kStageRowBytes, __float_as_uint(on ? z2.x : 0.0f));
    lds_st(stage_w + (T + m2) * kStageRowBytes, __float_as_uint(on ? z2.y : 0.0f));
  }
}

// the 32 staged values of seed lane & 15 this lane feeds the matrix unit with, widened exactly
__device__ __forceinline__ void gmt_operand(int stage_r, double (&v)[32]) {
#pragma unroll
  for (int h = 0; h < 2; h++)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const u32x4_t x = lds_u4((uint32_t)(stage_r + h * T * kStageRowBytes + 64 * q));
      v[(h * 4 + q) * 4 + 0] = (double)__uint_as_float(x.x);
      v[(h * 4 + q) * 4 + 1] = (double)__uint_as_float(x.y);
      v[(h * 4 + q) * 4 + 2] = (double)__uint_as_float(x.z);
      v[(h * 4 + q) * 4 + 3] = (double)__uint_as_float(x.w);
    }
}

template <int DT>
__global__ __launch_bounds__(kApplyThreads) void fks_gram_mt_tiled_kernel(GramMtTiledArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds32[];
  uint8_t* lds = reinterpret_cast<uint8_t*>(lds32);
  // the lds_* accessors address LDS by offset from 0: the dynamic block must start there
  if ((uint32_t)(size_t)(lds_u32_t*)lds32 != 0u) __builtin_trap();
  const int tid = threadIdx.x;
  const int c = blockIdx.x;
  const int nr = a.nrows, nc = a.ncols;
  const bool diag = a.diag != 0;
  const int nwin = diag ? nr : nr + nc;  // rows' windows first
  const int64_t b0 = a.chunk_block[c], b1 = a.chunk_block[c + 1];

  if constexpr (DT == FKS_BF16) {
    tab_bf16_fill(lds, tid, kApplyThreads);
  } else if constexpr (DT == kDtF32Libm) {
    logf_tab_fill(0u, tid, kApplyThreads);
  }
  for (int idx = tid; idx < nwin * kMtN; idx += kApplyThreads) {
    const int k = idx / kMtN, i = idx - k * kMtN;
    const uint32_t* src = k < nr ? a.row_states + ((size_t)k * a.nchunks + c) * kMtN
                                 : a.col_states + ((size_t)(k - nr) * a.nchunks + c) * kMtN;
    lds_st(kLdsTabBytes + k * kWinBytes + 4 * wperm(i), src[i]);
  }
  // rows of seeds past the pass's counts stay +0: they meet padding cells only, never written out
  for (int i = tid; i < kWaves * kStageWaveBytes / 4; i += kApplyThreads) lds_st(kStageOff + 4 * i, 0u);
  TwistPlan plan, plan2;
  twist_plan(plan, tid, kLdsTabBytes);
  twist_plan(plan2, tid, kLdsTabBytes + kTwistWindows * kWinBytes);
  __syncthreads();

  // Thread q < 312 owns Box-Muller pair q of every block: block words j1 and j1 + 8 (pair_word)
  const bool lane_on = tid < kMtN / 2;
  const int j1 = pair_word(tid);
  const int st_off = pair_off(j1);
  const int stage = kStageOff + plan.wave * kStageWaveBytes;
  const int stage_w = stage + 4 * plan.lane;
  const int stage_r = stage + (plan.lane & 15) * kStageRowBytes + 16 * (plan.lane >> 4);

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

  f64x4_t acc = (f64x4_t){0.0, 0.0, 0.0, 0.0};  // cell ((lane >> 4) + 4 g, lane & 15) in acc[g]
  for (int64_t b = b0; b < b1; b++) {
    __syncthreads();                          // every wave is done reading block b-1's words
    twist_all(plan, nwin);                    // the raw words of stream block b
    twist_all(plan2, nwin - kTwistWindows);
    __syncthreads();                          // every window holds block b
    const int64_t s1 = (int64_t)kMtN * b + j1;
    while (s1 >= seg_end) { cur++; load_seg(); }
    const bool on = lane_on && s1 >= seg_start;
    double za[32], zb[32];
    gmt_stage<DT>(lds, st_off, 0, nr, on, stage_w);
    wave_fence();
    gmt_operand(stage_r, za);
    if (diag) {  // wave-uniform
#pragma unroll
      for (int i = 0; i < 32; i++) zb[i] = za[i];
    } else {
      wave_fence();  // the row operand is read before the column block takes its place
      gmt_stage<DT>(lds, st_off, nr, nc, on, stage_w);
      wave_fence();
      gmt_operand(stage_r, zb);
    }
    wave_fence();
#pragma unroll
    for (int i = 0; i < 32; i++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(za[i], zb[i], acc, 0, 0, 0);
  }

  // the waves in wave order: every wave leaves its accumulators in its own staging area
  wave_fence();
  double* mine = reinterpret_cast<double*>(lds + stage);  // [4][64]
#pragma unroll
  for (int g = 0; g < 4; g++) mine[g * 64 + plan.lane] = acc[g];
  __syncthreads();
  if (tid < kGmtCells) {
    double s = reinterpret_cast<const double*>(lds + kStageOff)[tid];
#pragma unroll
    for (int w = 1; w < kWaves; w++) s += reinterpret_cast<const double*>(lds + kStageOff + w * kStageWaveBytes)[tid];
    a.partial[(size_t)c * kGmtCells + tid] = s;
  }
}

// One workgroup per row m of the pass.  Thread t adds, for column t & 15, the partials t >> 4,
// (t >> 4) + 16, ... of the sequence [fast launches' chunks | the cell's irregular sub-pass's
// chunks] in order; the 16 sums of a column are then added in order.
__global__ __launch_bounds__(256) void fks_gram_mt_tiled_reduce_kernel(const double* reg, int nreg, const double* irr,
                                                                       int nirr, int ncols, double* out, int64_t ld,
                                                                       int row0, int col0, int mirror) {
  __shared__ double s[16][T];
  const int m = (int)blockIdx.x;
  const int n = (int)(threadIdx.x & 15u), bs = (int)(threadIdx.x >> 4);
  const size_t at = (size_t)((m >> 2) * 64 + ((m & 3) << 4) + n);
  const int sub = (m / kGramMtRows) * kGmtSubCols + n / kGramMtCols;
  const size_t iat = (size_t)(m % kGramMtRows) * kPhxSeeds + (size_t)(n % kGramMtCols);
  double sum = 0.0;
  if (n < ncols) {  // (a column past the pass's has no irregular sub-pass)
    for (int b = bs; b < nreg + nirr; b += 16)
      sum += b < nreg ? reg[(size_t)b * kGmtCells + at]
                      : irr[((size_t)sub * (size_t)nirr + (size_t)(b - nreg)) * kGmtIrrCells + iat];
  }
  s[bs][n] = sum;
  __syncthreads();
  if (threadIdx.x < 16u && n < ncols) {
    double v = s[0][n];
#pragma unroll
    for (int k = 1; k < 16; k++) v += s[k][n];
    out[(int64_t)(row0 + m) * ld + col0 + n] = v;
    if (mirror) out[(int64_t)(col0 + n) * ld + row0 + m] = v;
  }
}

template <int DT>
int gmtt_launch(const GramMtTiledArgs& a, void* stream) {
  static PerDevice attr;
  if (int e = ensure_lds_attr(attr, &fks_gram_mt_tiled_kernel<DT>, kGmtLdsBytes)) return e;
  hipLaunchKernelGGL((fks_gram_mt_tiled_kernel<DT>), dim3((unsigned)a.nchunks), dim3(kApplyThreads), kGmtLdsBytes,
                     (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // namespace

int launch_gram_mt_tiled(int dtype, const GramMtTiledArgs& a, void* stream) {
  if (a.nrows < 1 || a.nrows > T || a.ncols < 1 || a.ncols > T || a.nchunks < 1 || a.nsegs < 1 || !a.partial ||
      !a.row_states || (!a.diag && !a.col_states) || (a.diag && a.nrows != a.ncols))
    return -FKS_EINVAL;
  if (dtype == FKS_BF16) {
    if (int e = ensure_tables()) return e;
    return gmtt_launch<FKS_BF16>(a, stream);
  }
  if (dtype == FKS_F32) return gmtt_launch<FKS_F32>(a, stream);
  if (dtype == kDtF32Libm) return gmtt_launch<kDtF32Libm>(a, stream);
  return -FKS_ENOTSUP;  // f16 tensors have no fast segments
}

int launch_gram_mt_tiled_reduce(const double* reg, int nreg, const double* irr, int nirr, int nrows, int ncols,
                                double* out, int64_t ld, int row0, int col0, bool mirror, void* stream) {
  if (nrows < 1 || nrows > T || ncols < 1 || ncols > T || nreg < 0 || nirr < 0 || nreg + nirr < 1 || (nreg && !reg) ||
      (nirr && !irr) || row0 < 0 || col0 < 0 || !out || (int64_t)col0 + ncols > ld ||
      (mirror && (int64_t)row0 + nrows > ld))  // mirror: square, side ld
    return -FKS_EINVAL;
  hipLaunchKernelGGL(fks_gram_mt_tiled_reduce_kernel, dim3((unsigned)nrows), dim3(256), 0, (hipStream_t)stream, reg,
                     nreg, irr, nirr, ncols, out, ld, row0, col0, mirror ? 1 : 0);
  return (int)hipGetLastError();
}

}  // namespace fks
