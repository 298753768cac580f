// fks_gram_tiled.hip -- the seed-basis Gram matrix on the f64 matrix unit (include/fks.h
// fks_gram_tiled, fks_gram_tiled.h; torch_rocm stream): G[r][c] = <z_r, z_c> for a tile of
// 16 kGtR row seeds by 16 kGtC column seeds per pass.
//
// v_mfma_f64_16x16x4_f64 forms D[m][n] += sum over k < 4 of A[m][k] B[k][n]; lane l supplies
// A[l & 15][l >> 4] and B[l >> 4][l & 15], one f64 each.  Here m and n are SEEDS of a 16-seed
// block and k is a work item (one Philox call, four elements; fks_internal.h PhxTensor): lane l
// draws, for seed l & 15 of a block and item l >> 4 of four consecutive items, the four z of the
// item in the tensor's dtype -- the values fks_normal writes, +0 past the tensor's end -- and
// widens them to f64.  The four z feed four MFMAs, one per sub-index i, and the SAME registers
// serve as A for a row block and as B for a column block: no cross-lane movement, no LDS.  A wave
// that owns the whole tile draws 16 (kGtR + kGtC) seeds per element for 256 kGtR kGtC cells, and
// round 1 of Philox, which multiplies the counter only, once for all of them.  Every product is
// exact (24 x 24 significand bits) and every addition is f64.
//
// The walk: a wave takes CHUNKS of kGtChunk = 256 consecutive items (every boundary of the table
// and of a shard is a multiple of 256 items, so a chunk lies in one row j of one tensor and its
// dtype is wave-uniform), chunk g + n * (waves of the grid) for n = 0, 1, ..., and inside a chunk
// the quads of four items in order.  The accumulators (kGtR x kGtC x 4 f64 per lane) stay in
// registers over the whole walk.  At the end the workgroup's waves are added in wave order
// through LDS and the sum goes to partial[block]; fks_gram_tiled_reduce_kernel adds the blocks in
// a fixed order.  The grid is a function of the device and the item count alone, and every
// accumulator sees the same sequence of MFMAs whatever its place in the tile, so an element
// depends on the device, the tensor list, the shard and its two seeds only.  No floating-point
// atomic.  Blocks past the pass's seed counts are neither drawn nor multiplied.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fks_internal.h"
#include "fks_gram_tiled.h"
#include "fks_dev_zgen.h"

namespace fks {
namespace {

typedef double f64x4_t __attribute__((ext_vector_type(4)));

constexpr int kGtLdsTensors = 512;            // tables of at most this many entries are copied to LDS
constexpr int kGtAccBytes = kGtTile * 8;      // the workgroup's sum, in front of the table
constexpr int kGtQuads = kGtChunk / 4;        // MFMA steps of a chunk
static_assert(kGtAccBytes % 16 == 0, "the LDS table starts 16-byte aligned");

// the last table entry whose first item is <= it, at or after lo (a wave's chunks only grow)
template <class Tab>
__device__ __forceinline__ int gt_find_t(Tab tab, int nt, int64_t it, int lo) {
  for (int p = 0; p < 2; p++) {
    if (lo + 1 >= nt || tab[lo + 1].item0 > it) return lo;
    ++lo;
  }
  int hi = nt - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].item0 <= it) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// the four z of one item for one seed, in dtype DT, as ProjFetchDraw forms them
template <int DT>
__device__ __forceinline__ void gt_z(const uint4 w, f32x2_t& zA, f32x2_t& zB) {
  if constexpr (DT == FKS_BF16) {
    phx_z_bf16(w, zA, zB);
  } else {
    phx_box_muller2(w, zA, zB);
    zA = (f32x2_t){phx_cast<DT>(zA.x), phx_cast<DT>(zA.y)};
    zB = (f32x2_t){phx_cast<DT>(zB.x), phx_cast<DT>(zB.y)};
  }
}

// ... in the (wave-uniform) dtype of the chunk's tensor, widened to f64; +0 for an element past
// the tensor's end.  The dtype branches here, around the draw alone, and not around the chunk:
// one copy of the MFMAs, and one generator live at a time.
__device__ __forceinline__ void gt_draw(int dtype, const PhxRound1& r1, uint64_t seed, const bool (&live)[4],
                                        double (&z)[4]) {
  const uint4 w = philox4x32_10(r1, seed);
  f32x2_t zA, zB;
  if (dtype == FKS_BF16) gt_z<FKS_BF16>(w, zA, zB);
  else if (dtype == FKS_F32) gt_z<FKS_F32>(w, zA, zB);
  else gt_z<FKS_F16>(w, zA, zB);
  z[0] = live[0] ? (double)zA.x : 0.0;
  z[1] = live[1] ? (double)zA.y : 0.0;
  z[2] = live[2] ? (double)zB.x : 0.0;
  z[3] = live[3] ? (double)zB.y : 0.0;
  __builtin_amdgcn_sched_barrier(0);
}

// one chunk: the items r0 .. r0 + 255 of T (r0 a multiple of 256, counted from the tensor's first
// item), all in row j = r0 / stride.  Everything but the lane's seeds and items is wave-uniform.
__device__ __forceinline__ void gt_chunk(const PhxTensor& T, int64_t r0, const uint64_t (&rs)[kGtR],
                                         const uint64_t (&cs)[kGtC], int nrb, int ncb, bool diag, int lane,
                                         f64x4_t (&acc)[kGtR][kGtC]) {
  const int64_t S = (int64_t)T.stride;
  const uint32_t idx0 = (uint32_t)(r0 % S);
  const uint64_t j = (uint64_t)(r0 / S);
  const uint64_t ctr = T.off4 + j;
  const int dtype = T.dtype;
  const int64_t e0 = (int64_t)idx0 + S * (int64_t)(4 * j);  // sub-index 0 of the chunk's first item
  // quads whose first element lies inside the tensor (sub-index 0 is the lowest element of an item)
  const int64_t left = T.numel - e0;
  const int nq = left <= 0 ? 0 : (int)std::min<int64_t>((left + 3) / 4, kGtQuads);
  const int kk = lane >> 4;
#pragma unroll 1
  for (int q = 0; q < nq; q++) {
    const uint32_t idx = idx0 + (uint32_t)(4 * q + kk);
    const int64_t e = e0 + 4 * q + kk;
    bool live[4];
#pragma unroll
    for (int i = 0; i < 4; i++) live[i] = e + S * i < T.numel;
    const PhxRound1 r1 = philox_round1(ctr, idx);
    double za[kGtR][4];
#pragma unroll
    for (int rb = 0; rb < kGtR; rb++)
      if (rb < nrb) gt_draw(dtype, r1, rs[rb], live, za[rb]);
#pragma unroll
    for (int cb = 0; cb < kGtC; cb++) {
      if (cb >= ncb) continue;
      double zb[4];
      if (cb < kGtR && diag && cb < nrb) {
        // (the index below is clamped for the compiler only: with C > R the unrolled body exists
        // for cb >= kGtR too, dead, and za[cb] there would be a constant index out of range)
#pragma unroll
        for (int i = 0; i < 4; i++) zb[i] = za[cb < kGtR ? cb : 0][i];
      } else {
        gt_draw(dtype, r1, cs[cb], live, zb);
      }
#pragma unroll
      for (int rb = 0; rb < kGtR; rb++) {
        if (rb >= nrb) continue;
#pragma unroll
        for (int i = 0; i < 4; i++)
          acc[rb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(za[rb][i], zb[i], acc[rb][cb], 0, 0, 0);
      }
    }
  }
}

template <class Tab>
__device__ __forceinline__ void gt_walk(const GramTiledArgs& a, Tab tab, int lane, f64x4_t (&acc)[kGtR][kGtC]) {
  uint64_t rs[kGtR], cs[kGtC];
#pragma unroll
  for (int b = 0; b < kGtR; b++) rs[b] = a.rseeds[b * kGtSeeds + (lane & 15)];
#pragma unroll
  for (int b = 0; b < kGtC; b++) cs[b] = a.cseeds[b * kGtSeeds + (lane & 15)];
  const int nrb = a.nrb, ncb = a.ncb;
  const bool diag = a.diag != 0;
  const int64_t step = (int64_t)gridDim.x * kGtWaves * kGtChunk;
  int64_t wb = rfl64(a.item_lo + ((int64_t)blockIdx.x * kGtWaves + (int64_t)(threadIdx.x >> 6)) * kGtChunk);
  int ts = 0;
  for (; wb < a.item_hi; wb += step) {  // wave-uniform
    ts = __builtin_amdgcn_readfirstlane(gt_find_t(tab, a.nt, wb, ts));
    const PhxTensor T = tab[ts];
    gt_chunk(T, wb - T.item0, rs, cs, nrb, ncb, diag, lane, acc);
  }
}

__global__ __launch_bounds__(kGtThreads, kGtWgPerCu) void fks_gram_tiled_kernel(GramTiledArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_gt[];
  double* s_acc = reinterpret_cast<double*>(s_gt);  // [kGtR][kGtC][4][64]
  PhxTensor* s_tab = reinterpret_cast<PhxTensor*>(s_gt + kGtAccBytes);
  const int lane = (int)(threadIdx.x & 63u);
  const int wave = (int)(threadIdx.x >> 6);
  f64x4_t acc[kGtR][kGtC];
#pragma unroll
  for (int rb = 0; rb < kGtR; rb++)
#pragma unroll
    for (int cb = 0; cb < kGtC; cb++) acc[rb][cb] = (f64x4_t){0.0, 0.0, 0.0, 0.0};
  if (a.nt <= kGtLdsTensors) {
    constexpr int W = (int)(sizeof(PhxTensor) / 4);
    for (int i = (int)threadIdx.x; i < a.nt * W; i += kGtThreads)
      reinterpret_cast<uint32_t*>(s_tab)[i] = reinterpret_cast<const uint32_t*>(a.t)[i];
    __syncthreads();
    gt_walk(a, (const PhxTensor*)s_tab, lane, acc);
  } else {
    gt_walk(a, a.t, lane, acc);
  }
  // the waves in wave order: ((w0 + w1) + w2) + w3, every lane on its own words
  for (int w = 0; w < kGtWaves; w++) {
    if (wave == w) {
#pragma unroll
      for (int rb = 0; rb < kGtR; rb++)
#pragma unroll
        for (int cb = 0; cb < kGtC; cb++)
#pragma unroll
          for (int g = 0; g < 4; g++) {
            const int at = ((rb * kGtC + cb) * 4 + g) * 64 + lane;
            s_acc[at] = w == 0 ? acc[rb][cb][g] : s_acc[at] + acc[rb][cb][g];
          }
    }
    __syncthreads();
  }
  double* const out = a.partial + (size_t)blockIdx.x * kGtTile;
  for (int i = (int)threadIdx.x; i < kGtTile; i += kGtThreads) out[i] = s_acc[i];
}

// One workgroup per (row m of the pass, 16-seed column block cb): the 16 results of that row and
// block are 16 consecutive doubles of a partial (the f64 MFMA's result map: col = lane & 15,
// row = (lane >> 4) + 4 * register).  Thread t adds, for column t & 15, the blocks t >> 4,
// (t >> 4) + 16, ... in order; the 16 sums of a column are then added in order.  Written to the
// element of the matrix and, for a symmetric call, to the transposed one: <z_r, z_c> and
// <z_c, z_r> are the same products in the same order, so an element two passes (or the two halves
// of a diagonal pass) write receives the same bits from both.
__global__ __launch_bounds__(256) void fks_gram_tiled_reduce_kernel(const double* partial, int nblocks, double* out,
                                                                    int64_t ld, int row0, int col0, int ncols, int mirror) {
  __shared__ double s[16][16];
  const int cb = (int)blockIdx.x, m = (int)blockIdx.y;
  const int ni = (int)(threadIdx.x & 15u), bs = (int)(threadIdx.x >> 4);
  const int rb = m >> 4, mi = m & 15;
  const size_t at = (size_t)(((rb * kGtC + cb) * 4 + (mi >> 2)) * 64 + ((mi & 3) << 4) + ni);
  double sum = 0.0;
  for (int b = bs; b < nblocks; b += 16) sum += partial[(size_t)b * kGtTile + at];
  s[bs][ni] = sum;
  __syncthreads();
  if (threadIdx.x < 16u) {
    double v = s[0][ni];
#pragma unroll
    for (int k = 1; k < 16; k++) v += s[k][ni];
    const int n = cb * kGtSeeds + ni;
    if (n < ncols) {
      out[(int64_t)(row0 + m) * ld + col0 + n] = v;
      if (mirror) out[(int64_t)(col0 + n) * ld + row0 + m] = v;
    }
  }
}

}  // namespace

int gram_tiled_grid(int64_t items) {
  const int64_t chunks = (items + kGtChunk - 1) / kGtChunk;
  const int64_t want = (chunks + kGtWaves - 1) / kGtWaves;
  return (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)kGtWgPerCu * device_cu_count()));
}

int launch_gram_tiled(const GramTiledArgs& a, void* stream) {
  const int64_t items = a.item_hi - a.item_lo;
  if (a.nrb < 1 || a.nrb > kGtR || a.ncb < 1 || a.ncb > kGtC || a.nt < 1 || items <= 0 || !a.partial || !a.t)
    return -FKS_EINVAL;
  // a chunk never straddles a tensor or the shard: every boundary is a multiple of 256 items
  if (a.item_lo % kGtChunk != 0 || items % kGtChunk != 0) return -FKS_EINVAL;
  const size_t lds = (size_t)kGtAccBytes + (a.nt <= kGtLdsTensors ? sizeof(PhxTensor) * (size_t)a.nt : 0);
  if constexpr (kGtAccBytes + kGtLdsTensors * sizeof(PhxTensor) > 64 * 1024) {  // a tile past 4 x 4 (A/B builds)
    const hipError_t rc = hipFuncSetAttribute(reinterpret_cast<const void*>(fks_gram_tiled_kernel),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (rc != hipSuccess) return (int)rc;
  }
  hipLaunchKernelGGL(fks_gram_tiled_kernel, dim3((unsigned)gram_tiled_grid(items)), dim3(kGtThreads), lds,
                     (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int launch_gram_tiled_reduce(const double* partial, int nblocks, int nrows, int ncols, double* out, int64_t ld,
                             int row0, int col0, bool mirror, void* stream) {
  if (ncols < 1 || ncols > kGtCols || nrows < 1 || nrows > kGtRows || nblocks < 1 || row0 < 0 || col0 < 0 ||
      !partial || !out || (int64_t)col0 + ncols > ld || (mirror && (int64_t)row0 + nrows > ld))  // mirror: square, side ld
    return -FKS_EINVAL;
  hipLaunchKernelGGL(fks_gram_tiled_reduce_kernel, dim3((unsigned)((ncols + kGtSeeds - 1) / kGtSeeds), (unsigned)nrows),
                     dim3(256), 0, (hipStream_t)stream, partial, nblocks, out, ld, row0, col0, ncols, mirror ? 1 : 0);
  return (int)hipGetLastError();
}

}  // namespace fks
