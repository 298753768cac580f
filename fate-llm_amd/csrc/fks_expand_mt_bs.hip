// fks_expand_mt_bs.hip -- the bit-sliced seed-basis expansion on the CPU generator's MT19937 stream
// (include/fks.h fks_expand_mt_bs, fks_expand_mt_bs.h): out = cast(beta out + sum_s f32(c_s) z_s)
// over the bf16 fast segments, 32 seeds per generator state, with fks_expand_mt_multi's bits.
//
// fks_expand_mt_bs_kernel<FULL, CARRY, FINAL> is fks_project_mt_bs_kernel's generator
// (fks_project_mt_bs.hip, fks_bitslice.h) with the expansion's chain in the place of the f64 sums.
// One workgroup per CU holds two bit-sliced 32-seed states in LDS, one per HALF of kEmbsWaves waves,
// beside one copy of the bf16 tables R and (C,S): row i of a state is state word i of its 32 seeds
// as 32 bit planes, kept as 8 chunk arrays of 4 planes.  Workgroup w runs the pass's at most 32
// seeds on plan chunk 2 w + h in half h (always the split form: the halves work on different
// elements and never wait for each other).  A chunk is cut into TASKS of 128 stream words that the
// half's waves take round-robin; lane L owns the Box-Muller pair (j, j + 8), j = 16 (L >> 3) +
// (L & 7), of its task: it twists exactly those two rows in place, tempers their low bytes and
// transposes them to one byte per seed.  The twists of a half form one serial chain handed from
// wave to wave through an LDS flag -- the only spin in the kernel.
//
// The lane's chain over its two elements: the two f32 sums start from +0, or with CARRY from the
// f32 the pass before staged; per seed of the pass, in order, two table lookups, the v_pk_fma_f32
// and the bf16 rounding that make z = bf16(R[a] C[b]) + 0, bf16(R[a] S[b]) + 0, and one packed fma
// acc = fma({c_s, c_s}, z, acc) -- fks_expand_mt_kernel's chain, the coefficients wave-uniform out
// of the launch arguments.  A seed past nseeds takes no part (a sum can be -0, which a zero product
// would turn into +0).  Without FINAL the sums go to the staging area as f32 (ExpMtPass's
// addresses); with FINAL through fma(beta, old, acc) where the output is read, then through the
// cast to the output's dtype: per element, 2 or 4 bytes, an output being aligned to its element
// only.  An f32 store between two seeds loses nothing, so the bits do not depend on how the seeds
// are cut into passes of 32 or 19.
//
// The output's piece under a segment comes from the per-call table (ProjMtVecEntry).  The old
// output is two 16-bit loads per element whatever its dtype and the carry two f32 loads, both
// fetched one task of the wave ahead, so no load waits under a branch; with beta 0 the output is
// never read.  A lane off every fast segment or past the chunk loads the workspace sink and
// stores nothing; a frozen tensor has no segment.  No floating-point atomic, no wave-wide operation
// over the sums, one workgroup barrier.
//
// A translation unit of its own (no -fgpu-rdc) with its own instances of the __constant__ tables.
#include <hip/hip_runtime.h>

#include "fks_internal.h"
#include "fks_expand_mt_bs.h"
#include "fks_bitslice.h"
#include "fks_dev_lds.h"
#include "fks_dev_update.h"
#include "fks_dev_zgen.h"
#include "fks_dev_irr.h"
#include "fks_dev_host.h"

namespace fks {
namespace {

constexpr int W = kEmbsWaves;
constexpr int kHalfThreads = 64 * W;
constexpr int kTaskWords = 128;                    // stream words per task
constexpr int kPlaneBytes = kMtN * 16;             // one chunk array: planes 4q..4q+3 of all 624 rows
constexpr int kStateBytes = 8 * kPlaneBytes;       // 79,872
constexpr int kTabBytes = 256 * 4 + 256 * 8;       // R f32 | (C,S) f32 pairs
// LDS: [tables | state half 0 | state half 1 | twisted-task count per half]
constexpr uint32_t kFlagOff = kTabBytes + 2 * kStateBytes;
constexpr int kLdsBytes = (int)kFlagOff + 8;       // 162,824
static_assert(kLdsBytes <= 160 * 1024, "one workgroup fits the CU's LDS");

typedef __attribute__((address_space(1))) const uint16_t embs_cgu16;
typedef __attribute__((address_space(1))) const float embs_cgf32;
typedef __attribute__((address_space(1))) uint16_t embs_gu16;
typedef __attribute__((address_space(1))) float embs_gf32;

// The hand-off word needs no memory fence: one wave's LDS operations are performed in order, so a
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

// the 16 bits of v rounded to nearest even to bf16 / f16 (fks_expand_mt.hip emt_bits16)
__device__ __forceinline__ uint32_t bits16(float v, bool bf) {
  const uint32_t b = __float_as_uint(rbf_cvt(v)) >> 16;
  const uint32_t h = Traits<FKS_F16>::bits(Traits<FKS_F16>::rnd(v));
  return bf ? b : h;
}

template <bool FULL, bool CARRY, bool FINAL>
__global__ __launch_bounds__(kEmbsThreads, 1) void fks_expand_mt_bs_kernel(ExpMtBsArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds32[];
  // the lds_* accessors address LDS by offset from 0: the dynamic block must start there
  if ((uint32_t)(size_t)(lds_u32_t*)lds32 != 0u) __builtin_trap();
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int half = __builtin_amdgcn_readfirstlane(tid >= kHalfThreads ? 1 : 0);
  const int ht = tid - half * kHalfThreads;
  const int hw = __builtin_amdgcn_readfirstlane(ht >> 6);
  const int c = 2 * (int)blockIdx.x + half;  // this half's plan chunk
  const int nseeds = FULL ? kBsSeeds : a.nseeds;
  const int64_t b0 = a.chunk_block[c], b1 = a.chunk_block[c + 1];
  const int nwords = (int)(kMtN * (b1 - b0));  // < 2^31 (the host's plan keeps chunks shorter)
  const int ntask = (nwords + kTaskWords - 1) / kTaskWords;
  const uint32_t sbase = kTabBytes + (uint32_t)half * kStateBytes;
  const uint32_t flag = kFlagOff + 4u * (uint32_t)half;

  for (int i = tid; i < 256; i += kEmbsThreads) {
    reinterpret_cast<float*>((uint8_t*)lds32)[i] = c_tab_bf16[i];
    reinterpret_cast<float2*>((uint8_t*)lds32 + 1024)[i] = make_float2(c_tab_bf16[256 + i], c_tab_bf16[512 + i]);
  }
  // prologue: the jump windows of this chunk (the state before block b0), as planes
  for (int i = ht; i < kMtN; i += kHalfThreads) {
    uint32_t w[32];
#pragma unroll
    for (int k = 0; k < 32; k++) w[k] = k < nseeds ? a.states[((size_t)k * a.nchunks + c) * kMtN + i] : 0u;
    bs::transpose32(w);
#pragma unroll
    for (int q = 0; q < 8; q++)
      lds_st4(sbase + 16u * (uint32_t)i + q * kPlaneBytes, u32x4_t{w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]});
  }
  if (ht == 0) lds32[flag / 4] = 0u;
  __syncthreads();  // the only workgroup barrier

  const int toff = 16 * (lane >> 3) + (lane & 7);  // the lane's words toff, toff + 8 of a task
  // the lane's first row is toff + 8 where (lane >> 3) is odd: every 16-lane group of a
  // ds_read_b128 (8-lane group of a ds_write_b128) then touches distinct rows mod 16
  const bool flip = ((lane >> 3) & 1) != 0;

  // the lane's current segment, where its element 0 is staged and the output's piece under it
  // (positions only grow)
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
  uint64_t seg_stage = 0, seg_out = 0;
  uint32_t seg_dt = FKS_F32;  // the output's dtype
  auto load_seg = [&]() {
    if (cur < a.nsegs) {
      const DevSeg sg = a.segs[cur];
      const ProjMtVecEntry e = a.pv[cur];
      seg_start = sg.start;
      seg_end = sg.start + sg.numel;
      seg_stage = a.stage_bias + sg.ptr;
      seg_out = e.ptr;
      seg_dt = (uint32_t)e.dtype;
    } else {
      seg_start = seg_end = INT64_MAX;
    }
    // drained here (rare), so that the cached segment registers are never "possibly pending" later
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
  };
  load_seg();

  // What the lane needs of task n beside its z: where its two elements toff and toff + 8 of the task
  // (one 16-block: the same segment) go, the carry, and FINAL the old output as two 16-bit loads per
  // element: the halves of an f32 element, or a 2-byte element twice.
  struct Slot {
    uint64_t dst;   // the lane's first element: in the staging area, or FINAL in the output's piece
    uint32_t meta;  // on | output dtype << 1
    float c1, c2;
    uint32_t lo1, hi1, lo2, hi2;
  };
  const uint64_t sink = (uint64_t)(uintptr_t)a.sink;
  auto fetch = [&](const int n) -> Slot {
    Slot sl;
    const int u1 = kTaskWords * n + toff;
    const int64_t s1 = wbase + u1;
    while (s1 >= seg_end) { cur++; load_seg(); }
    const bool on = u1 < nwords && s1 >= seg_start;
    const uint64_t e = on ? (uint64_t)(s1 - seg_start) : 0u;
    const uint32_t dt = on ? seg_dt : (uint32_t)FKS_F32;
    const bool wide = dt == (uint32_t)FKS_F32;
    const uint64_t stage = seg_stage + 4u * e, out = seg_out + (e << (wide ? 2 : 1));
    sl.meta = (on ? 1u : 0u) | (dt << 1);
    sl.dst = FINAL ? out : stage;
    sl.c1 = sl.c2 = 0.0f;
    if constexpr (CARRY) {
      const uint64_t ca = on ? stage : sink;
      sl.c1 = *reinterpret_cast<embs_cgf32*>(ca);
      sl.c2 = *reinterpret_cast<embs_cgf32*>(ca + 32u);
    }
    sl.lo1 = sl.hi1 = sl.lo2 = sl.hi2 = 0u;
    if constexpr (FINAL) {
      const bool rd = on && a.read_old != 0;
      const bool w2 = rd ? wide : true;
      const uint64_t p1 = rd ? out : sink, p2 = p1 + (w2 ? 32u : 16u), hi = w2 ? 2u : 0u;
      sl.lo1 = *reinterpret_cast<embs_cgu16*>(p1);
      sl.hi1 = *reinterpret_cast<embs_cgu16*>(p1 + hi);
      sl.lo2 = *reinterpret_cast<embs_cgu16*>(p2);
      sl.hi2 = *reinterpret_cast<embs_cgu16*>(p2 + hi);
    }
    return sl;
  };
  auto widen = [](uint32_t lo, uint32_t hi, uint32_t dt) -> float {  // exact, by selects
    const float hf = (float)__builtin_bit_cast(_Float16, (uint16_t)lo);
    const float w = __uint_as_float(dt == (uint32_t)FKS_F32 ? (lo | (hi << 16)) : (lo << 16));
    return dt == (uint32_t)FKS_F16 ? hf : w;
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

  // ---- the chain of the lane's two elements through the pass's seeds, and the store
  auto chain = [&](const Slot& sl, uint32_t (&oa)[8], uint32_t (&ob)[8]) {
    bs::transpose8(oa);
    bs::transpose8(ob);
    f32x2_t acc = {sl.c1, sl.c2};  // +0 without CARRY
#pragma unroll
    for (int k = 0; k < kBsSeeds; k++) {
      if (FULL || k < nseeds) {
        // z = bf16(R[a] C[b]) + 0, bf16(R[a] S[b]) + 0 (normal_fill_16<BFloat16>: an exact f32
        // product, one rounding; the fma's +0 turns -0 into +0 like "+ mean")
        const float r = lds_f32(byte_index<2>(oa[k & 7], k >> 3));
        const f32x2_t rr = {r, r}, zero = {0.0f, 0.0f};
        const f32x2_t cs = lds_f32x2(1024u + byte_index<3>(ob[k & 7], k >> 3));
        const f32x2_t z = rnd2<FKS_BF16>(__builtin_elementwise_fma(rr, cs, zero));
        const f32x2_t gg = {a.g[k], a.g[k]};  // wave-uniform, out of the arguments
        acc = __builtin_elementwise_fma(gg, z, acc);  // fks_expand_mt_kernel's fma, both elements
      }
      // the lookups of one byte column (8 seeds) at a time
      if ((k & 7) == 7) asm volatile("" ::: "memory");
    }
    if (sl.meta & 1u) {  // a lane off every segment or past the chunk stores nothing
      float acc1 = acc.x, acc2 = acc.y;
      if constexpr (FINAL) {
        const uint32_t dt = (sl.meta >> 1) & 3u;
        if (a.read_old) {
          acc1 = __fmaf_rn(a.beta, widen(sl.lo1, sl.hi1, dt), acc1);
          acc2 = __fmaf_rn(a.beta, widen(sl.lo2, sl.hi2, dt), acc2);
        }
        if (dt == (uint32_t)FKS_F32) {
          *reinterpret_cast<embs_gf32*>(sl.dst) = acc1;
          *reinterpret_cast<embs_gf32*>(sl.dst + 32u) = acc2;
        } else {
          const bool bf = dt == (uint32_t)FKS_BF16;
          *reinterpret_cast<embs_gu16*>(sl.dst) = (uint16_t)bits16(acc1, bf);
          *reinterpret_cast<embs_gu16*>(sl.dst + 16u) = (uint16_t)bits16(acc2, bf);
        }
      } else {
        *reinterpret_cast<embs_gf32*>(sl.dst) = acc1;
        *reinterpret_cast<embs_gf32*>(sl.dst + 32u) = acc2;
      }
    }
  };

  // ---- task n: wait for task n-1's twist, twist, publish, chain; fetches task n + W into nx
  // (past the last task: the sink)
  auto task = [&](const int n, const Slot& sl, Slot& nx) {
    uint32_t oa[8], ob[8];
    __builtin_amdgcn_s_setprio(2);
    while (__builtin_amdgcn_readfirstlane(flag_load(flag)) < (uint32_t)n) __builtin_amdgcn_s_sleep(0);
    asm volatile("" ::: "memory");
    twist(n, oa, ob);
    if (lane == 0) flag_store(flag, (uint32_t)n + 1u);
    __builtin_amdgcn_s_setprio(0);
    nx = fetch(n + W);
    chain(sl, oa, ob);
  };

  // two named slots and a loop unrolled by two: a slot copy on the back edge would wait for the
  // load at the top of every task
  if (hw < ntask) {
    Slot s0 = fetch(hw), s1;
    int n = hw;
    for (;;) {
      task(n, s0, s1);
      if (n + W >= ntask) break;
      n += W;
      task(n, s1, s0);
      if (n + W >= ntask) break;
      n += W;
    }
  }
}

template <bool FULL, bool CARRY, bool FINAL>
int embs_launch(const ExpMtBsArgs& a, void* stream) {
  static PerDevice attr;
  if (int e = ensure_lds_attr(attr, &fks_expand_mt_bs_kernel<FULL, CARRY, FINAL>, kLdsBytes)) return e;
  hipLaunchKernelGGL((fks_expand_mt_bs_kernel<FULL, CARRY, FINAL>), dim3((unsigned)(a.nchunks / 2)), dim3(kEmbsThreads),
                     kLdsBytes, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // namespace

// the six instances: a pass that stages is a full one
int launch_expand_mt_bs(const ExpMtBsArgs& a, void* stream) {
  if (a.nseeds < 1 || a.nseeds > kBsSeeds || a.nchunks < 2 || a.nchunks % 2 || a.nsegs < 1 || !a.states || !a.segs ||
      !a.chunk_block || !a.sink || !a.pv)
    return -FKS_EINVAL;
  const bool full = a.nseeds == kBsSeeds, carry = a.carry_in != 0;
  if (a.to_stage && !full) return -FKS_EINVAL;
  if (int e = ensure_tables()) return e;
  if (a.to_stage) return carry ? embs_launch<true, true, false>(a, stream) : embs_launch<true, false, false>(a, stream);
  if (carry) return full ? embs_launch<true, true, true>(a, stream) : embs_launch<false, true, true>(a, stream);
  return full ? embs_launch<true, false, true>(a, stream) : embs_launch<false, false, true>(a, stream);
}

}  // namespace fks
