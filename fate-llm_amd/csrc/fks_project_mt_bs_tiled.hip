// fks_project_mt_bs_tiled.hip -- the bit-sliced seed-basis projection of many vectors per draw on
// the CPU generator's MT19937 stream (include/fks.h fks_project_mt_bs_tiled,
// fks_project_mt_bs_tiled.h): out[m][s] = <vec_m, z_s> over the bf16 fast segments, 32 seeds per
// generator state against 16 vectors, the sums on the f64 matrix unit.
//
// fks_project_mt_bs_tiled_kernel<FULL> is fks_gram_mt_bs_kernel's frame (fks_gram_mt_bs.hip) with
// loaded vectors in the place of the second drawn block: Z^T V, one draw for 16 vectors.  One
// workgroup per CU takes one plan chunk and holds ONE bit-sliced 32-seed state in LDS beside the
// bf16 tables R and (C,S); its kPmbtWaves waves take the chunk's TASKS of 128 stream words
// round-robin and hand the twist chain from wave to wave through an LDS flag.  Lane L owns the
// Box-Muller pair (j, j + 8), j = 16 (L >> 3) + (L & 7), of its task: twist, temper_low8,
// transpose8, the R and (C,S) lookups and the bf16 rounding exactly as there.  That leaves a lane
// with z of its two elements for all 32 seeds, every one bf16-exact, kept as their 16 bits and
// transposed through a wave-private staging area into the A operands of v_mfma_f64_16x16x4_f64:
// lane l holds seed l & 15 of a block, element slot l >> 4.  The B operand is 4 element slots x
// 16 vectors: lane l holds vector l & 15, slot l >> 4, widened to f64 exactly from bf16, f16 or
// f32.  A step is two MFMAs, seed block 0 and block 1 against the same B: 8 f64 accumulators per
// lane, held over the chunk's tasks.
//   * Slot k takes the elements [32 k, 32 k + 32) of a task, so lane (vector, k) reads 32
//     contiguous elements: per half of 16 (one 16-block: one segment) with 16-byte loads where the
//     piece is 16-byte aligned and element loads where it is not -- the same values either way.
//   * Element 16 a + 8 h + j of a slot (h the half of the owning lane's pair, j < 8) is step
//     t = 16 a + 2 j + h: a lane's two z are the steps 2 u, 2 u + 1, u = 8 a + j, of one slot and
//     are staged as ONE 32-bit word, word u of row (seed, k); rows of 16 words, a seed's four rows
//     behind each other and seeds 68 words apart.  Lane L writes word L & 15 of row L >> 4: the 64
//     lanes of a write cover 64 consecutive words; lane l of a read takes row (16 m + (l & 15),
//     l >> 4) with four ds_read_b128, the 16 seeds of a quarter wave 4 banks apart.
//   * A lane off every bf16 fast segment or past the chunk, and a vector column past the pass's
//     count, loads the workspace sink and enters +0: its products are zeros whatever its (finite)
//     z.  A seed past the pass's count is never drawn: its rows stay the +0 they were cleared to.
// Which step and slot an element takes depends on its place in the stream only, and is the same
// for both operands, so <vec_m, z_s> is the same sequence of products and additions whatever plane
// s rides in, whatever column m takes, whatever the other seeds and vectors.
//
// A wave accumulates its tasks in task order.  At the chunk's end the waves add their tiles in
// wave order through one LDS tile (wave w adds to what the waves below it left and passes it on;
// a wave without a task enters +0); the last writes partial[chunk][vector][seed].  No
// floating-point atomic.  fks_project_mt_bs_tiled_reduce_kernel adds, per (vector, seed), the
// chunks in chunk order and then the rows of the 19-seed launches that took the rest of the list
// (fks_run_basis.cpp project_mt_bs_tiled).
//
// A translation unit of its own (no -fgpu-rdc) with its own instances of the __constant__ tables.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "fks_internal.h"
#include "fks_project_mt_bs_tiled.h"
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
typedef __attribute__((address_space(1))) const uint16_t pmbt_gu16;
typedef __attribute__((address_space(1))) const uint32_t pmbt_gu32;
typedef __attribute__((address_space(1))) const u32x4_t pmbt_gu4;

constexpr int W = kPmbtWaves;
constexpr int T = 16;                              // seeds of a block: the rows of one MFMA
constexpr int NB = kBsSeeds / T;                   // seed blocks of the state
constexpr int kTaskWords = 128;                    // stream words per task
constexpr int kPlaneBytes = kMtN * 16;             // one chunk array: planes 4q..4q+3 of all 624 rows
constexpr int kStateBytes = 8 * kPlaneBytes;       // 79,872
constexpr int kTabBytes = 256 * 4 + 256 * 8;       // R f32 | (C,S) f32 pairs
constexpr int kSeedPitch = 4 * (4 * 16 + 4);       // bytes between two seeds' rows of a staging area
constexpr int kStageBytes = kBsSeeds * kSeedPitch; // 8,704 per wave
// LDS: [tables | state | one staging area per wave | twisted-task count | waves-summed count | the
// workgroup's two tiles of sums]
constexpr uint32_t kStageOff = kTabBytes + kStateBytes;
constexpr uint32_t kFlagOff = kStageOff + W * kStageBytes;
constexpr uint32_t kDoneOff = kFlagOff + 4;
constexpr uint32_t kRedOff = kDoneOff + 4;
constexpr int kLdsBytes = (int)kRedOff + kPmbtCells * 8;  // 156,680 at W = 8
static_assert(NB == 2 && kPmbtVec == 16, "two MFMAs of 16 seeds x 16 vectors per step");
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

// The 16 elements of one vector piece as they lie in memory: 16 words of an f32 piece, 8 words (two
// elements each) of a bf16 or f16 piece.  meta: on | dtype << 1.
struct Half {
  uint32_t r[16];
  uint32_t meta;
};

// 16 elements of dtype dt at p (aligned to the element): 16-byte loads where p allows them
__device__ __forceinline__ void load_half(Half& h, uint64_t p, uint32_t dt) {
  const bool wide = (p & 15u) == 0;
  if (dt == (uint32_t)FKS_F32) {
    if (wide) {
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const u32x4_t x = *reinterpret_cast<pmbt_gu4*>(p + 16u * (uint32_t)i);
        h.r[4 * i] = x.x; h.r[4 * i + 1] = x.y; h.r[4 * i + 2] = x.z; h.r[4 * i + 3] = x.w;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; i++) h.r[i] = *reinterpret_cast<pmbt_gu32*>(p + 4u * (uint32_t)i);
    }
  } else {
    if (wide) {
#pragma unroll
      for (int i = 0; i < 2; i++) {
        const u32x4_t x = *reinterpret_cast<pmbt_gu4*>(p + 16u * (uint32_t)i);
        h.r[4 * i] = x.x; h.r[4 * i + 1] = x.y; h.r[4 * i + 2] = x.z; h.r[4 * i + 3] = x.w;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const uint32_t lo = *reinterpret_cast<pmbt_gu16*>(p + 4u * (uint32_t)i);
        const uint32_t hi = *reinterpret_cast<pmbt_gu16*>(p + 4u * (uint32_t)i + 2u);
        h.r[i] = lo | (hi << 16);
      }
    }
#pragma unroll
    for (int i = 8; i < 16; i++) h.r[i] = 0u;
  }
}

// element e (compile-time) of a piece, widened to f32 exactly; +0 from an off lane
template <int E>
__device__ __forceinline__ float half_value(const Half& h) {
  const uint32_t dt = h.meta >> 1;
  const uint32_t pair = h.r[E >> 1];
  const uint32_t bits16 = (E & 1) ? pair >> 16 : pair & 0xFFFFu;
  const float f16 = (float)__builtin_bit_cast(_Float16, (uint16_t)bits16);
  const float bf = __uint_as_float(bits16 << 16);
  const float v = dt == (uint32_t)FKS_F32 ? __uint_as_float(h.r[E]) : dt == (uint32_t)FKS_F16 ? f16 : bf;
  return (h.meta & 1u) ? v : 0.0f;
}

template <bool FULL>
__global__ __launch_bounds__(kPmbtThreads, 1) void fks_project_mt_bs_tiled_kernel(ProjMtBsTiledArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds32[];
  // the lds_* accessors address LDS by offset from 0: the dynamic block must start there
  if ((uint32_t)(size_t)(lds_u32_t*)lds32 != 0u) __builtin_trap();
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int hw = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = (int)blockIdx.x;
  const int nseeds = FULL ? kBsSeeds : a.nseeds;
  const int64_t b0 = a.chunk_block[c], b1 = a.chunk_block[c + 1];
  const int nwords = (int)(kMtN * (b1 - b0));  // < 2^31 (the host's plan keeps chunks shorter)
  const int ntask = (nwords + kTaskWords - 1) / kTaskWords;
  constexpr uint32_t sbase = kTabBytes;

  for (int i = tid; i < 256; i += kPmbtThreads) {
    reinterpret_cast<float*>((uint8_t*)lds32)[i] = c_tab_bf16[i];
    reinterpret_cast<float2*>((uint8_t*)lds32 + 1024)[i] = make_float2(c_tab_bf16[256 + i], c_tab_bf16[512 + i]);
  }
  // prologue: the jump windows of this chunk (the state before block b0), as planes
  for (int i = tid; i < kMtN; i += kPmbtThreads) {
    uint32_t w[32];
#pragma unroll
    for (int k = 0; k < 32; k++) w[k] = k < nseeds ? a.states[((size_t)k * a.nchunks + c) * kMtN + i] : 0u;
    bs::transpose32(w);
#pragma unroll
    for (int q = 0; q < 8; q++)
      lds_st4(sbase + 16u * (uint32_t)i + q * kPlaneBytes, u32x4_t{w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]});
  }
  // the rows of seeds past the pass's count stay +0
  for (int i = tid; i < W * kStageBytes / 4; i += kPmbtThreads) lds_st((int)kStageOff + 4 * i, 0u);
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
  // the lane's word of a seed's rows: row (slot) toff >> 5 = lane >> 4, word 8 a + j = lane & 15
  const uint32_t stage_w = stage + 4u * (uint32_t)lane;
  // the lane's operand row: seed l & 15 of a block, slot l >> 4
  const uint32_t stage_r = stage + (uint32_t)((lane & 15) * kSeedPitch + (lane >> 4) * 64);

  // the vector side: column lane & 15, the elements [32 slot, 32 slot + 32) of a task
  const int col = lane & 15, slot = lane >> 4;
  const bool col_on = col < a.nvec;
  const ProjMtVecEntry* const pv = a.pv + (col_on ? (int64_t)col * a.pv_stride : 0);
  const int64_t wbase = (int64_t)kMtN * b0;  // stream position of the chunk's first word
  // the column's current segment and the vector's piece under it (positions only grow)
  int cur;
  {
    const int64_t s1 = wbase + (int64_t)kTaskWords * hw + 32 * slot;
    int lo = 0, hi = a.nsegs;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (a.segs[mid].start + a.segs[mid].numel <= s1) lo = mid + 1; else hi = mid;
    }
    cur = lo;
  }
  int64_t seg_start = INT64_MAX, seg_end = INT64_MAX;
  uint64_t seg_ptr = 0;
  uint32_t seg_dt = FKS_BF16;
  auto load_seg = [&]() {
    if (cur < a.nsegs) {
      const DevSeg sg = a.segs[cur];
      const ProjMtVecEntry e = pv[cur];
      seg_start = sg.start;
      seg_end = sg.start + sg.numel;
      seg_ptr = e.ptr;
      seg_dt = (uint32_t)e.dtype;
    } else {
      seg_start = seg_end = INT64_MAX;
    }
  };
  load_seg();

  // the 16 elements [32 slot + 16 h, + 16) of task n (one 16-block: one segment, numel a multiple
  // of 16); off every segment, past the chunk or past the pass's vectors: the sink
  auto fetch = [&](const int n, const int h, Half& out) {
    const int u = kTaskWords * n + 32 * slot + 16 * h;
    const int64_t s = wbase + u;
    while (s >= seg_end) { cur++; load_seg(); }
    const bool on = col_on && u < nwords && s >= seg_start;
    const uint32_t dt = on ? seg_dt : (uint32_t)FKS_BF16;
    const uint64_t e = on ? (uint64_t)(s - seg_start) : 0u;
    const uint64_t p = on ? seg_ptr + (e << (dt == (uint32_t)FKS_F32 ? 2 : 1)) : (uint64_t)(uintptr_t)a.sink;
    load_half(out, p, dt);
    out.meta = (on ? 1u : 0u) | (dt << 1);
  };

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

  // cell (seed 16 i + 4 g + (lane >> 4), vector lane & 15) in acc[i][g]
  f64x4_t acc[NB];
#pragma unroll
  for (int i = 0; i < NB; i++) acc[i] = (f64x4_t){0.0, 0.0, 0.0, 0.0};

  // ---- the chain of the lane's two elements through the seeds: z staged as 16 + 16 bits
  auto chain = [&](uint32_t (&oa)[8], uint32_t (&ob)[8]) {
    bs::transpose8(oa);
    bs::transpose8(ob);
#pragma unroll
    for (int k = 0; k < kBsSeeds; k++) {
      if (FULL || k < nseeds) {
        // z = bf16(R[a] C[b]) + 0, bf16(R[a] S[b]) + 0 (normal_fill_16<BFloat16>: an exact f32
        // product, one rounding; the fma's +0 turns -0 into +0 like "+ mean")
        const float r = lds_f32(byte_index<2>(oa[k & 7], k >> 3));
        const f32x2_t rr = {r, r}, zero = {0.0f, 0.0f};
        const f32x2_t cs = lds_f32x2(1024u + byte_index<3>(ob[k & 7], k >> 3));
        const f32x2_t z = rnd2<FKS_BF16>(__builtin_elementwise_fma(rr, cs, zero));
        const uint32_t word = (__float_as_uint(z.x) >> 16) | (__float_as_uint(z.y) & 0xFFFF0000u);
        lds_st((int)(stage_w + (uint32_t)(k * kSeedPitch)), word);
      }
      // the lookups of one byte column (8 seeds) at a time
      if ((k & 7) == 7) asm volatile("" ::: "memory");
    }
  };

  // ---- the 32 matrix steps of a staged task, eight (one ds_read_b128 per block) at a time: step
  // 8 q + 2 i + h meets element 16 (q >> 1) + 8 h + 4 (q & 1) + i of the slot on both sides
  auto matrix = [&](const Half& h0, const Half& h1) {
    const bool two = FULL || nseeds > T;  // wave-uniform: block 1 holds a seed
    auto steps = [&](auto Q, const Half& hv) {
      constexpr int q = decltype(Q)::value;
      constexpr int e0 = 4 * (q & 1);
      const double v[8] = {(double)half_value<e0>(hv),     (double)half_value<e0 + 8>(hv),
                           (double)half_value<e0 + 1>(hv), (double)half_value<e0 + 9>(hv),
                           (double)half_value<e0 + 2>(hv), (double)half_value<e0 + 10>(hv),
                           (double)half_value<e0 + 3>(hv), (double)half_value<e0 + 11>(hv)};
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
        acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(z0[i], v[i], acc[0], 0, 0, 0);
        if (two) acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(z1[i], v[i], acc[1], 0, 0, 0);
      }
    };
    steps(std::integral_constant<int, 0>{}, h0);
    steps(std::integral_constant<int, 1>{}, h0);
    steps(std::integral_constant<int, 2>{}, h1);
    steps(std::integral_constant<int, 3>{}, h1);
  };

  // ---- task n: wait for task n-1's twist, twist, publish, fetch the vectors' pieces (in flight
  // under the chain), stage, multiply.  A wave's LDS operations execute in order, so the hand-off
  // between its lanes through the staging area needs no barrier: a compiler fence keeps the
  // program order.
  for (int n = hw; n < ntask; n += W) {
    uint32_t oa[8], ob[8];
    __builtin_amdgcn_s_setprio(2);
    while (__builtin_amdgcn_readfirstlane(flag_load(kFlagOff)) < (uint32_t)n) __builtin_amdgcn_s_sleep(0);
    asm volatile("" ::: "memory");
    twist(n, oa, ob);
    if (lane == 0) flag_store(kFlagOff, (uint32_t)n + 1u);
    __builtin_amdgcn_s_setprio(0);
    Half h0, h1;
    fetch(n, 0, h0);
    fetch(n, 1, h1);
    chain(oa, ob);
    asm volatile("" ::: "memory");
    matrix(h0, h1);
    asm volatile("" ::: "memory");  // the next task's stores follow this task's operand reads
  }

  // ---- the chunk's sums: the waves in wave order through the workgroup's tiles
  while (__builtin_amdgcn_readfirstlane(flag_load(kDoneOff)) < (uint32_t)hw) __builtin_amdgcn_s_sleep(1);
  asm volatile("" ::: "memory");
#pragma unroll
  for (int i = 0; i < NB; i++) {
    if (i == 0 || FULL || nseeds > T) {
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const int cell = (i * 4 + g) * 64 + lane;
        lds_f64_t* slot_p = (lds_f64_t*)(size_t)(kRedOff + 8u * (uint32_t)cell);
        const double sum = hw ? *slot_p + acc[i][g] : acc[i][g];
        const int seed = T * i + 4 * g + (lane >> 4);
        if (hw + 1 < W) *slot_p = sum;
        else if (col_on && seed < nseeds)
          a.partial[(size_t)c * kPmbtCells + (size_t)(col * kBsSeeds + seed)] = sum;
      }
    }
  }
  if (lane == 0) flag_store(kDoneOff, (uint32_t)hw + 1u);
}

// One workgroup per (seed, vector) of the pass: thread t adds rows t, t + 64, ... of the sequence
// [the bit-sliced launch's chunks | the rows of the 19-seed launches of the vector and the seed's
// sub-pass] in order; the 64 sums are then added in order.
__global__ __launch_bounds__(64) void fks_project_mt_bs_tiled_reduce_kernel(const double* bs, int nbs, const double* sub,
                                                                            int nrows, int64_t sub_stride,
                                                                            int64_t vec_stride, double* out, int64_t ld) {
  __shared__ double sh[64];
  const int s = (int)blockIdx.x, m = (int)blockIdx.y, t = (int)threadIdx.x;
  const double* const brow = bs + (size_t)(m * kBsSeeds + s);
  const double* const srow = sub + (int64_t)m * vec_stride + (int64_t)(s / kMaxSeedsPerPass) * sub_stride + s % kMaxSeedsPerPass;
  double sum = 0.0;
  for (int b = t; b < nbs + nrows; b += 64)
    sum += b < nbs ? brow[(size_t)b * kPmbtCells] : srow[(size_t)(b - nbs) * kPhxSeeds];
  sh[t] = sum;
  __syncthreads();
  if (t == 0) {
    double v = sh[0];
#pragma unroll
    for (int k = 1; k < 64; k++) v += sh[k];
    out[(int64_t)m * ld + s] = v;
  }
}

template <bool FULL>
int pmbt_launch(const ProjMtBsTiledArgs& a, void* stream) {
  static PerDevice attr;
  if (int e = ensure_lds_attr(attr, &fks_project_mt_bs_tiled_kernel<FULL>, kLdsBytes)) return e;
  hipLaunchKernelGGL((fks_project_mt_bs_tiled_kernel<FULL>), dim3((unsigned)a.nchunks), dim3(kPmbtThreads), kLdsBytes,
                     (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // namespace

int launch_project_mt_bs_tiled(const ProjMtBsTiledArgs& a, void* stream) {
  if (a.nseeds < 1 || a.nseeds > kBsSeeds || a.nvec < 1 || a.nvec > kPmbtVec || a.nchunks < 1 || a.nsegs < 1 ||
      a.pv_stride < a.nsegs || !a.states || !a.segs || !a.chunk_block || !a.sink || !a.partial || !a.pv)
    return -FKS_EINVAL;
  if (int e = ensure_tables()) return e;
  return a.nseeds == kBsSeeds ? pmbt_launch<true>(a, stream) : pmbt_launch<false>(a, stream);
}

int launch_project_mt_bs_tiled_reduce(const double* bs, int nbs, const double* sub, int nrows, int64_t sub_stride,
                                      int64_t vec_stride, int nseeds, int nvec, double* out, int64_t ld, void* stream) {
  if (nseeds < 1 || nseeds > kBsSeeds || nvec < 1 || nvec > kPmbtVec || nbs < 0 || nrows < 0 || nbs + nrows < 1 ||
      (nbs && !bs) || (nrows && !sub) || !out || ld < nseeds)
    return -FKS_EINVAL;
  hipLaunchKernelGGL(fks_project_mt_bs_tiled_reduce_kernel, dim3((unsigned)nseeds, (unsigned)nvec), dim3(64), 0,
                     (hipStream_t)stream, bs, nbs, sub, nrows, sub_stride, vec_stride, out, ld);
  return (int)hipGetLastError();
}

}  // namespace fks
