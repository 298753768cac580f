// fks_gram_mt_bs.hip -- the bit-sliced seed-basis Gram matrix on the CPU generator's MT19937 stream
// (include/fks.h fks_gram_mt_bs, fks_gram_mt_bs.h): G[r][c] = <z_r, z_c> over the bf16 fast
// segments, 32 seeds per generator state, the sums on the f64 matrix unit.
//
// fks_gram_mt_bs_kernel<DIAG, FULL> is fks_project_mt_bs_kernel's generator (fks_project_mt_bs.hip,
// fks_bitslice.h) with the matrix unit in the place of the projection's chain.  One workgroup per
// CU takes one plan chunk and holds ONE bit-sliced 32-seed state in LDS beside the bf16 tables R
// and (C,S); its kGmbsWaves waves take the chunk's TASKS of 128 stream words round-robin and hand
// the twist chain from wave to wave through an LDS flag.  Lane L owns the Box-Muller pair (j, j +
// 8), j = 16 (L >> 3) + (L & 7), of its task: twist, temper_low8, transpose8, the R and (C,S)
// lookups and the bf16 rounding exactly as there.  That leaves a lane with z of its two elements
// for all 32 seeds, every one bf16-exact, and v_mfma_f64_16x16x4_f64 wants lane l to hold seed
// l & 15 of element-slot l >> 4: the transpose goes through a wave-private staging area, the z
// kept as their 16 bits.
//   * The 128 elements of a task feed 32 matrix steps of 4: element 16 g + 8 h + j (h the half of
//     the lane's pair, j < 8) is slot k = j & 3 of step t = 4 g + 2 (j >> 2) + h.  A lane's two
//     elements are the steps 2 u, 2 u + 1 of one slot, so they are staged as ONE 32-bit word:
//     word u = 2 g + (j >> 2) of row (seed, k), rows of 16 words, a seed's four rows behind each
//     other and seeds 68 words apart.  The 64 lanes of a write cover 64 consecutive words; lane l
//     of a read takes row (16 m + (l & 15), l >> 4) with four ds_read_b128, the 16 seeds of a
//     quarter wave 4 banks apart: neither conflicts.
//   * The operand of block m -- 16 seeds x 4 slots per step, widened to f64 exactly -- is the A
//     operand of a product with block m in the rows and the B operand of one with it in the
//     columns: the pair form runs one MFMA per step (block 0 x block 1), the diagonal form three
//     ((0,0), (0,1), (1,1): 12 f64 accumulators per lane).
//   * A lane off every bf16 fast segment, or past the chunk, stages +0.  A seed past its block's
//     count is never drawn: its rows stay the +0 they were cleared to, and its cells are not read.
// Which step and slot an element takes depends on its place in the stream only, so <z_r, z_c> is
// the same sequence of products and additions whatever planes r and c ride in, whatever the other
// seeds, and in either form; <z_c, z_r> is the same products in the same order.
//
// A wave accumulates its tasks in task order.  At the chunk's end the waves add their tiles in
// wave order through one LDS tile (wave w adds to what the waves below it left and passes it on;
// a wave without a task enters +0); the last writes partial[chunk][tile][cell].  No floating-point
// atomic.  fks_gram_mt_bs_reduce_kernel adds a cell's partials -- the chunks in chunk order, then
// the partials of the launches that took the rest of the list (fks_run_basis.cpp gram_mt_bs) --
// in one fixed order and mirrors a symmetric call's cells.
//
// No vector is read.  A translation unit of its own (no -fgpu-rdc) with its own instances of the
// __constant__ tables.
#include <hip/hip_runtime.h>

#include "fks_internal.h"
#include "fks_gram_mt_bs.h"
#include "fks_bitslice.h"
#include "fks_dev_lds.h"
#include "fks_dev_update.h"
#include "fks_dev_zgen.h"
#include "fks_dev_irr.h"
#include "fks_dev_host.h"

namespace fks {
namespace {

typedef double f64x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) double lds_f64_t;

constexpr int W = kGmbsWaves;
constexpr int T = kGmtTile;
constexpr int kTaskWords = 128;                    // stream words per task
constexpr int kPlaneBytes = kMtN * 16;             // one chunk array: planes 4q..4q+3 of all 624 rows
constexpr int kStateBytes = 8 * kPlaneBytes;       // 79,872
constexpr int kTabBytes = 256 * 4 + 256 * 8;       // R f32 | (C,S) f32 pairs
constexpr int kSeedPitch = 4 * (4 * 16 + 4);       // bytes between two seeds' rows of a staging area
constexpr int kStageBytes = kBsSeeds * kSeedPitch; // 8,704 per wave
// LDS: [tables | state | one staging area per wave | twisted-task count | waves-summed count | the
// workgroup's tile(s) of sums]
constexpr uint32_t kStageOff = kTabBytes + kStateBytes;
constexpr uint32_t kFlagOff = kStageOff + W * kStageBytes;
constexpr uint32_t kDoneOff = kFlagOff + 4;
constexpr uint32_t kRedOff = kDoneOff + 4;
constexpr int kLdsBytes = (int)kRedOff + kGmbsDiagTiles * kGmtCells * 8;  // 158,728 at W = 8
static_assert(kStageOff % 16 == 0 && kSeedPitch % 16 == 0 && kStageBytes % 16 == 0, "ds_read_b128 alignment");
static_assert(kRedOff % 8 == 0 && kLdsBytes <= 160 * 1024, "one workgroup fits the CU's LDS");

// The hand-off words need no memory fence: one wave's LDS operations are performed in order, so a
// wave that reads the new count issues its loads after the writer's stores were performed.  The
// lgkmcnt(0) keeps the count from running ahead of stores still queued; the asm barriers keep the
// compiler from moving LDS accesses across.
__device__ __forceinline__ uint32_t flag_load(uint32_t off) { return *(volatile const lds_u32_t*)(size_t)off; }
__device__ __forceinline__ void flag_store(uint32_t off, uint32_t v) {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
  *(volatile lds_u32_t*)(size_t)off = v;
}

// byte c of w times 2^S with a compile-time c (SDWA)
template <int S>
__device__ __forceinline__ uint32_t byte_index(uint32_t w, int c) {
  switch (c) {
    case 0: return bs::byte_x<0, S>(w);
    case 1: return bs::byte_x<1, S>(w);
    case 2: return bs::byte_x<2, S>(w);
    default: return bs::byte_x<3, S>(w);
  }
}

// the two 16-bit values of a staged word, widened exactly
__device__ __forceinline__ double stage_lo(uint32_t w) { return (double)__uint_as_float(w << 16); }
__device__ __forceinline__ double stage_hi(uint32_t w) { return (double)__uint_as_float(w & 0xFFFF0000u); }

template <bool DIAG, bool FULL>
__global__ __launch_bounds__(kGmbsThreads, 1) void fks_gram_mt_bs_kernel(GramMtBsArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds32[];
  // the lds_* accessors address LDS by offset from 0: the dynamic block must start there
  if ((uint32_t)(size_t)(lds_u32_t*)lds32 != 0u) __builtin_trap();
  constexpr int NT = DIAG ? kGmbsDiagTiles : 1;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int hw = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = (int)blockIdx.x;
  const int n0 = FULL ? T : a.n0, n1 = FULL ? T : a.n1;
  const int64_t b0 = a.chunk_block[c], b1 = a.chunk_block[c + 1];
  const int nwords = (int)(kMtN * (b1 - b0));  // < 2^31 (the host's plan keeps chunks shorter)
  const int ntask = (nwords + kTaskWords - 1) / kTaskWords;
  constexpr uint32_t sbase = kTabBytes;

  for (int i = tid; i < 256; i += kGmbsThreads) {
    reinterpret_cast<float*>((uint8_t*)lds32)[i] = c_tab_bf16[i];
    reinterpret_cast<float2*>((uint8_t*)lds32 + 1024)[i] = make_float2(c_tab_bf16[256 + i], c_tab_bf16[512 + i]);
  }
  // prologue: the jump windows of this chunk (the state before block b0), as planes
  for (int i = tid; i < kMtN; i += kGmbsThreads) {
    uint32_t w[32];
#pragma unroll
    for (int k = 0; k < 32; k++) {
      if (k < T) w[k] = k < n0 ? a.blk0[((size_t)k * a.nchunks + c) * kMtN + i] : 0u;
      else w[k] = k - T < n1 ? a.blk1[((size_t)(k - T) * a.nchunks + c) * kMtN + i] : 0u;
    }
    bs::transpose32(w);
#pragma unroll
    for (int q = 0; q < 8; q++)
      lds_st4(sbase + 16u * (uint32_t)i + q * kPlaneBytes, u32x4_t{w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]});
  }
  // the rows of seeds past the blocks' counts stay +0
  for (int i = tid; i < W * kStageBytes / 4; i += kGmbsThreads) lds_st((int)kStageOff + 4 * i, 0u);
  if (tid == 0) {
    lds32[kFlagOff / 4] = 0u;
    lds32[kDoneOff / 4] = 0u;
  }
  __syncthreads();  // the only workgroup barrier

  const int toff = 16 * (lane >> 3) + (lane & 7);  // the lane's words toff, toff + 8 of a task
  // the lane's first row is toff + 8 where (lane >> 3) is odd: every 16-lane group of a
  // ds_read_b128 (8-lane group of a ds_write_b128) then touches distinct rows mod 16
  const bool flip = ((lane >> 3) & 1) != 0;
  const uint32_t stage = kStageOff + (uint32_t)(hw * kStageBytes);
  // the lane's word of a seed's rows: row k = j & 3, word 2 g + (j >> 2)
  const uint32_t stage_w = stage + 4u * (uint32_t)(16 * (lane & 3) + 2 * (lane >> 3) + ((lane >> 2) & 1));
  // the lane's operand row: seed l & 15 of a block, slot l >> 4
  const uint32_t stage_r = stage + (uint32_t)((lane & 15) * kSeedPitch + (lane >> 4) * 64);

  // the lane's current segment (positions only grow)
  const int64_t wbase = (int64_t)kMtN * b0;  // stream position of the chunk's first word
  int cur;
  {
    const int64_t s1 = wbase + (int64_t)kTaskWords * hw + toff;
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

  // ---- the twist of task n: the lane's two rows in place, block b -> b + 1 on 32 seeds at once;
  // returns the tempered radius bytes (row toff) and angle bytes (row toff + 8) as planes.  Streamed
  // over the 8 chunk arrays: chunk q of every row of the task is loaded (V, M) before any lane stores
  // it -- through data dependence, since new plane 4q+3 needs V plane 4q+4 of chunk q+1, loaded one
  // step ahead; U31 and V plane 0 are loaded first.  M rows lie 227 words back, outside the task.
  auto twist = [&](const int n, uint32_t (&oa)[8], uint32_t (&ob)[8]) {
    const int u1 = kTaskWords * n + toff;
    const bool valid = u1 < nwords;
    const int i1 = valid ? u1 % kMtN : 0;
    // first / second row (i1 + 8 < 624: 624 is a multiple of 16 and i1 mod 16 < 8)
    const int ia = flip ? i1 + 8 : i1, ib = flip ? i1 : i1 + 8;
    auto rows = [&](int i, uint32_t& av, uint32_t& am, uint32_t& au) {
      const int iv = i + 1 < kMtN ? i + 1 : 0;
      const int im = i < kMtN - kMtM ? i + kMtM : i - (kMtN - kMtM);
      av = sbase + 16u * (uint32_t)iv;
      am = sbase + 16u * (uint32_t)im;
      au = sbase + 7u * kPlaneBytes + 16u * (uint32_t)i + 12u;
    };
    uint32_t av1, am1, au1, av2, am2, au2;
    rows(ia, av1, am1, au1);
    rows(ib, av2, am2, au2);
    uint32_t M1[32], M2[32];  // the new rows
    const uint32_t U1 = lds_u32((int)au1), U2 = lds_u32((int)au2);
    u32x4_t va = lds_u4(av1), vb = lds_u4(av2), ma = lds_u4(am1), mb = lds_u4(am2);
    const uint32_t v0a = va.x, v0b = vb.x;
#pragma unroll
    for (int q = 0; q < 8; q++) {
      u32x4_t va2 = va, vb2 = vb, ma2 = ma, mb2 = mb;
      if (q < 7) {
        va2 = lds_u4(av1 + (q + 1) * kPlaneBytes);
        vb2 = lds_u4(av2 + (q + 1) * kPlaneBytes);
        ma2 = lds_u4(am1 + (q + 1) * kPlaneBytes);
        mb2 = lds_u4(am2 + (q + 1) * kPlaneBytes);
      }
      const uint32_t Va[5] = {va.x, va.y, va.z, va.w, va2.x};
      const uint32_t Vb[5] = {vb.x, vb.y, vb.z, vb.w, vb2.x};
      const uint32_t Ma[4] = {ma.x, ma.y, ma.z, ma.w}, Mb[4] = {mb.x, mb.y, mb.z, mb.w};
#pragma unroll
      for (int t = 0; t < 4; t++) {
        // bs::twist_row plane by plane: plane b of y >> 1 is V plane b+1 (b < 30; t = 3 reads chunk
        // q+1's plane 0), U31 (b = 30), none (b = 31)
        const int b = 4 * q + t;
        const bool am = ((bs::kMatrixA >> b) & 1u) != 0;
        uint32_t xa, xb;
        if (b < 30) { xa = Va[t + 1]; xb = Vb[t + 1]; }
        else if (b == 30) { xa = U1; xb = U2; }
        else { xa = 0u; xb = 0u; }
        M1[b] = am ? bs::xor3(Ma[t], xa, v0a) : (Ma[t] ^ xa);
        M2[b] = am ? bs::xor3(Mb[t], xb, v0b) : (Mb[t] ^ xb);
      }
      if (valid) {
        lds_st4(sbase + 16u * (uint32_t)ia + q * kPlaneBytes, u32x4_t{M1[4 * q], M1[4 * q + 1], M1[4 * q + 2], M1[4 * q + 3]});
        lds_st4(sbase + 16u * (uint32_t)ib + q * kPlaneBytes, u32x4_t{M2[4 * q], M2[4 * q + 1], M2[4 * q + 2], M2[4 * q + 3]});
      }
      va = va2; vb = vb2; ma = ma2; mb = mb2;
    }
    uint32_t o1[8], o2[8];
    bs::temper_low8(M1, o1);
    bs::temper_low8(M2, o2);
#pragma unroll
    for (int j = 0; j < 8; j++) {  // row toff: the radius uniforms; row toff + 8: the angle uniforms
      oa[j] = flip ? o2[j] : o1[j];
      ob[j] = flip ? o1[j] : o2[j];
    }
  };

  // cell ((lane >> 4) + 4 g, lane & 15) of tile i in acc[i][g]
  f64x4_t acc[NT];
#pragma unroll
  for (int i = 0; i < NT; i++) acc[i] = (f64x4_t){0.0, 0.0, 0.0, 0.0};

  // ---- the chain of the lane's two elements through the seeds: z staged as 16 + 16 bits
  auto chain = [&](const bool on, uint32_t (&oa)[8], uint32_t (&ob)[8]) {
    bs::transpose8(oa);
    bs::transpose8(ob);
    const uint32_t keep = on ? 0xFFFFFFFFu : 0u;  // an off lane stages +0
#pragma unroll
    for (int k = 0; k < kBsSeeds; k++) {
      if (FULL || (k < T ? k < n0 : k - T < n1)) {
        // z = bf16(R[a] C[b]) + 0, bf16(R[a] S[b]) + 0 (normal_fill_16<BFloat16>: an exact f32
        // product, one rounding; the fma's +0 turns -0 into +0 like "+ mean")
        const float r = lds_f32(byte_index<2>(oa[k & 7], k >> 3));
        const f32x2_t rr = {r, r}, zero = {0.0f, 0.0f};
        const f32x2_t cs = lds_f32x2(1024u + byte_index<3>(ob[k & 7], k >> 3));
        const f32x2_t z = rnd2<FKS_BF16>(__builtin_elementwise_fma(rr, cs, zero));
        const uint32_t word = (__float_as_uint(z.x) >> 16) | (__float_as_uint(z.y) & 0xFFFF0000u);
        lds_st((int)(stage_w + (uint32_t)(k * kSeedPitch)), word & keep);
      }
      // the lookups of one byte column (8 seeds) at a time
      if ((k & 7) == 7) asm volatile("" ::: "memory");
    }
  };

  // ---- the 32 matrix steps of a staged task, eight (one ds_read_b128 per block) at a time
  auto matrix = [&]() {
    const bool two = !DIAG || FULL || n1 > 0;  // wave-uniform: block 1 holds a seed
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const u32x4_t x0 = lds_u4(stage_r + 16u * (uint32_t)q);
      const uint32_t w0[4] = {x0.x, x0.y, x0.z, x0.w};
      double z0[8], z1[8];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        z0[2 * i] = stage_lo(w0[i]);
        z0[2 * i + 1] = stage_hi(w0[i]);
      }
      if (two) {
        const u32x4_t x1 = lds_u4(stage_r + (uint32_t)(T * kSeedPitch) + 16u * (uint32_t)q);
        const uint32_t w1[4] = {x1.x, x1.y, x1.z, x1.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
          z1[2 * i] = stage_lo(w1[i]);
          z1[2 * i + 1] = stage_hi(w1[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < 8; i++) {
        if constexpr (DIAG) {
          acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(z0[i], z0[i], acc[0], 0, 0, 0);
          if (two) {
            acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(z0[i], z1[i], acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(z1[i], z1[i], acc[2], 0, 0, 0);
          }
        } else {
          acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(z0[i], z1[i], acc[0], 0, 0, 0);
        }
      }
    }
  };

  // ---- task n: wait for task n-1's twist, twist, publish, stage, multiply.  A wave's LDS
  // operations execute in order, so the hand-off between its lanes through the staging area needs
  // no barrier: a compiler fence keeps the program order.
  for (int n = hw; n < ntask; n += W) {
    uint32_t oa[8], ob[8];
    __builtin_amdgcn_s_setprio(2);
    while (__builtin_amdgcn_readfirstlane(flag_load(kFlagOff)) < (uint32_t)n) __builtin_amdgcn_s_sleep(0);
    asm volatile("" ::: "memory");
    twist(n, oa, ob);
    if (lane == 0) flag_store(kFlagOff, (uint32_t)n + 1u);
    __builtin_amdgcn_s_setprio(0);
    const int u1 = kTaskWords * n + toff;
    const int64_t s1 = wbase + u1;
    while (s1 >= seg_end) { cur++; load_seg(); }
    chain(u1 < nwords && s1 >= seg_start, oa, ob);
    asm volatile("" ::: "memory");
    matrix();
    asm volatile("" ::: "memory");  // the next task's stores follow this task's operand reads
  }

  // ---- the chunk's sums: the waves in wave order through the workgroup's tile(s)
  while (__builtin_amdgcn_readfirstlane(flag_load(kDoneOff)) < (uint32_t)hw) __builtin_amdgcn_s_sleep(1);
  asm volatile("" ::: "memory");
  const int ntile = DIAG && !FULL && n1 == 0 ? 1 : NT;
#pragma unroll
  for (int i = 0; i < NT; i++) {
    if (i < ntile) {
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const int cell = (i * 4 + g) * 64 + lane;
        lds_f64_t* slot = (lds_f64_t*)(size_t)(kRedOff + 8u * (uint32_t)cell);
        const double sum = hw ? *slot + acc[i][g] : acc[i][g];
        if (hw + 1 < W) *slot = sum;
        else a.partial[(size_t)c * (size_t)(NT * kGmtCells) + (size_t)cell] = sum;
      }
    }
  }
  if (lane == 0) flag_store(kDoneOff, (uint32_t)hw + 1u);
}

// One workgroup per row m of the tile.  Thread t adds, for column t & 15, the partials t >> 4,
// (t >> 4) + 16, ... of the sequence [bit-sliced chunks | fast launches' chunks | the cell's
// irregular sub-pass's chunks] in order; the 16 sums of a column are then added in order.
__global__ __launch_bounds__(256) void fks_gram_mt_bs_reduce_kernel(const double* bs, int nbs, int64_t bs_stride,
                                                                    const double* reg, int nreg, const double* irr,
                                                                    int nirr, int ncols, double* out, int64_t ld,
                                                                    int row0, int col0, int mirror) {
  __shared__ double s[16][T];
  const int m = (int)blockIdx.x;
  const int n = (int)(threadIdx.x & 15u), run = (int)(threadIdx.x >> 4);
  const size_t at = (size_t)((m >> 2) * 64 + ((m & 3) << 4) + n);
  const int sub = (m / kGramMtRows) * kGmtSubCols + n / kGramMtCols;
  const size_t iat = (size_t)(m % kGramMtRows) * kPhxSeeds + (size_t)(n % kGramMtCols);
  double sum = 0.0;
  if (n < ncols) {  // (a column past the tile's has no irregular sub-pass)
    for (int b = run; b < nbs + nreg + nirr; b += 16) {
      if (b < nbs) sum += bs[(size_t)b * (size_t)bs_stride + at];
      else if (b < nbs + nreg) sum += reg[(size_t)(b - nbs) * kGmtCells + at];
      else sum += irr[((size_t)sub * (size_t)nirr + (size_t)(b - nbs - nreg)) * kGmtIrrCells + iat];
    }
  }
  s[run][n] = sum;
  __syncthreads();
  if (threadIdx.x < 16u && n < ncols) {
    double v = s[0][n];
#pragma unroll
    for (int k = 1; k < 16; k++) v += s[k][n];
    out[(int64_t)(row0 + m) * ld + col0 + n] = v;
    if (mirror) out[(int64_t)(col0 + n) * ld + row0 + m] = v;
  }
}

template <bool DIAG, bool FULL>
int gmbs_launch(const GramMtBsArgs& a, void* stream) {
  static PerDevice attr;
  if (int e = ensure_lds_attr(attr, &fks_gram_mt_bs_kernel<DIAG, FULL>, kLdsBytes)) return e;
  hipLaunchKernelGGL((fks_gram_mt_bs_kernel<DIAG, FULL>), dim3((unsigned)a.nchunks), dim3(kGmbsThreads), kLdsBytes,
                     (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // namespace

int launch_gram_mt_bs(const GramMtBsArgs& a, void* stream) {
  if (a.n0 < 1 || a.n0 > T || a.n1 < 0 || a.n1 > T || (a.n1 == 0 && !a.diag) || (a.n1 > 0 && a.n0 != T && a.diag) ||
      a.nchunks < 1 || a.nsegs < 1 || !a.blk0 || (a.n1 > 0 && !a.blk1) || !a.segs || !a.chunk_block || !a.partial)
    return -FKS_EINVAL;
  if (int e = ensure_tables()) return e;
  const bool full = a.n0 == T && a.n1 == T;
  if (a.diag) return full ? gmbs_launch<true, true>(a, stream) : gmbs_launch<true, false>(a, stream);
  return full ? gmbs_launch<false, true>(a, stream) : gmbs_launch<false, false>(a, stream);
}

int launch_gram_mt_bs_reduce(const double* bs, int nbs, int64_t bs_stride, const double* reg, int nreg,
                             const double* irr, int nirr, int nrows, int ncols, double* out, int64_t ld, int row0,
                             int col0, bool mirror, void* stream) {
  if (nrows < 1 || nrows > T || ncols < 1 || ncols > T || nbs < 0 || nreg < 0 || nirr < 0 || nbs + nreg + nirr < 1 ||
      (nbs && (!bs || bs_stride < kGmtCells)) || (nreg && !reg) || (nirr && !irr) || row0 < 0 || col0 < 0 || !out ||
      (int64_t)col0 + ncols > ld || (mirror && (int64_t)row0 + nrows > ld))  // mirror: square, side ld
    return -FKS_EINVAL;
  hipLaunchKernelGGL(fks_gram_mt_bs_reduce_kernel, dim3((unsigned)nrows), dim3(256), 0, (hipStream_t)stream, bs, nbs,
                     bs_stride, reg, nreg, irr, nirr, ncols, out, ld, row0, col0, mirror ? 1 : 0);
  return (int)hipGetLastError();
}

}  // namespace fks
