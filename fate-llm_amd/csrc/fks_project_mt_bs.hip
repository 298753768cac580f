// fks_project_mt_bs.hip -- the bit-sliced seed-basis projection on the CPU generator's MT19937
// stream (include/fks.h fks_project_mt_bs, fks_project_mt_bs.h): out[s] = <vec, z_s> over the bf16
// fast segments, 32 seeds per generator state.
//
// fks_project_mt_bs_kernel<FULL> is the bf16 slice kernel's generator (fks_kern_slice.h,
// fks_bitslice.h) with the projection's chain in the place of the update.  One workgroup per CU
// holds two bit-sliced 32-seed states in LDS, one per HALF of kPmbsWaves waves, beside one copy of
// the bf16 tables R and (C,S): row i of a state is state word i of its 32 seeds as 32 bit planes,
// kept as 8 chunk arrays of 4 planes (16 B per row, one ds_read_b128 / ds_write_b128).  The work of
// a plan chunk is cut into TASKS of 128 stream words that the half's waves take round-robin.  Lane
// L owns the Box-Muller pair (j, j + 8), j = 16 (L >> 3) + (L & 7), of its task: it twists exactly
// those two rows in place (one 2- or 3-input xor per plane), tempers their low bytes, transposes
// them to one byte per seed, and then runs, per seed, two table lookups, the v_pk_fma_f32 and the
// bf16 rounding that make z = bf16(R[a] C[b]) + 0, bf16(R[a] S[b]) + 0, two v_cvt_f64_f32 and two
// v_fma_f64 into that seed's f64 accumulator: exact products of the lane's two vector elements,
// widened to f64 once per task, one rounding per addition.  The twists of a half form one serial
// chain (a task's M rows were written by the task before it) handed from wave to wave through an
// LDS flag; the chains of different tasks overlap freely.
//
// Unlike the update, nothing is stored, so the two halves never wait for each other: a pass of more
// than 32 seeds runs seeds [0, 32) and [32, n) on the SAME plan chunk (the vector is read twice, the
// second time from L2), a pass of at most 32 runs every seed on two neighbouring chunks.  Every plan
// chunk boundary is jumped in both forms, so a (seed, chunk) sum is the same sequence of operations
// whichever form, half and plane the seed rides in: the result depends on the seed, not on the call.
//
// The 32 accumulators (64 VGPRs) live across the tasks of a chunk.  At its end, per seed: the
// 64-lane xor butterfly, lane k keeping seed k's sum; then the half's waves in wave order through a
// 256-byte row of LDS (wave w adds its sums to what waves < w left and passes the row on; the last
// writes partial[chunk][seed]).  A wave without a task enters +0.  No floating-point atomic.
// fks_project_mt_bs_reduce_kernel adds, per seed, the chunks' rows in chunk order and then the rows
// of the 19-seed launches that took the rest of the list (fks_run_basis.cpp project_mt_bs).
//
// The vector is read in place through the per-call table (ProjMtVecEntry: f32, bf16 or f16, aligned
// to its element only): every element as two 16-bit loads whatever its dtype, so no load sits under
// a branch, prefetched one task ahead.  A lane off every fast segment or past the chunk loads the
// workspace sink and enters +0; a frozen tensor has no segment and is never read.
//
// A translation unit of its own (no -fgpu-rdc) with its own instances of the __constant__ tables.
#include <hip/hip_runtime.h>

#include "fks_internal.h"
#include "fks_project_mt_bs.h"
#include "fks_bitslice.h"
#include "fks_dev_lds.h"
#include "fks_dev_update.h"
#include "fks_dev_zgen.h"
#include "fks_dev_irr.h"
#include "fks_dev_host.h"

namespace fks {
namespace {

constexpr int W = kPmbsWaves;
constexpr int kHalfThreads = 64 * W;
constexpr int kTaskWords = 128;                    // stream words per task
constexpr int kPlaneBytes = kMtN * 16;             // one chunk array: planes 4q..4q+3 of all 624 rows
constexpr int kStateBytes = 8 * kPlaneBytes;       // 79,872
constexpr int kTabBytes = 256 * 4 + 256 * 8;       // R f32 | (C,S) f32 pairs
// LDS: [tables | state half 0 | state half 1 | twisted-task count per half | waves-summed count per
// half | one row of kBsSeeds f64 per half]
constexpr uint32_t kFlagOff = kTabBytes + 2 * kStateBytes;
constexpr uint32_t kDoneOff = kFlagOff + 8;
constexpr uint32_t kRedOff = kDoneOff + 8;
constexpr int kRedRowBytes = kBsSeeds * 8;
constexpr int kLdsBytes = (int)kRedOff + 2 * kRedRowBytes;  // 163,344
static_assert(kRedOff % 8 == 0 && kLdsBytes <= 160 * 1024, "one workgroup fits the CU's LDS");

typedef __attribute__((address_space(1))) const uint16_t pmbs_gu16;
typedef __attribute__((address_space(3))) double lds_f64_t;

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

template <bool FULL>
__global__ __launch_bounds__(kPmbsThreads, 1) void fks_project_mt_bs_kernel(ProjMtBsArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds32[];
  // the lds_* accessors address LDS by offset from 0: the dynamic block must start there
  if ((uint32_t)(size_t)(lds_u32_t*)lds32 != 0u) __builtin_trap();
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int half = __builtin_amdgcn_readfirstlane(tid >= kHalfThreads ? 1 : 0);
  const int ht = tid - half * kHalfThreads;
  const int hw = __builtin_amdgcn_readfirstlane(ht >> 6);
  const bool split = a.split != 0;  // FULL: 32 seeds in each half either way
  const int c = split ? 2 * (int)blockIdx.x + half : (int)blockIdx.x;  // this half's plan chunk
  const int sfirst = half && !split ? kBsSeeds : 0;                    // this half's first seed of the pass
  const int nseeds = FULL ? kBsSeeds : split ? a.nseeds : (half ? a.nseeds - kBsSeeds : kBsSeeds);
  const int64_t b0 = a.chunk_block[c], b1 = a.chunk_block[c + 1];
  const int nwords = (int)(kMtN * (b1 - b0));  // < 2^31 (the host's plan keeps chunks shorter)
  const int ntask = (nwords + kTaskWords - 1) / kTaskWords;
  const uint32_t sbase = kTabBytes + (uint32_t)half * kStateBytes;
  const uint32_t flag = kFlagOff + 4u * (uint32_t)half;
  const uint32_t done = kDoneOff + 4u * (uint32_t)half;
  const uint32_t red = kRedOff + (uint32_t)(half * kRedRowBytes);

  for (int i = tid; i < 256; i += kPmbsThreads) {
    reinterpret_cast<float*>((uint8_t*)lds32)[i] = c_tab_bf16[i];
    reinterpret_cast<float2*>((uint8_t*)lds32 + 1024)[i] = make_float2(c_tab_bf16[256 + i], c_tab_bf16[512 + i]);
  }
  // prologue: the jump windows of this chunk (the state before block b0), as planes
  for (int i = ht; i < kMtN; i += kHalfThreads) {
    uint32_t w[32];
#pragma unroll
    for (int k = 0; k < 32; k++)
      w[k] = k < nseeds ? a.states[((size_t)(sfirst + k) * a.nchunks + c) * kMtN + i] : 0u;
    bs::transpose32(w);
#pragma unroll
    for (int q = 0; q < 8; q++)
      lds_st4(sbase + 16u * (uint32_t)i + q * kPlaneBytes, u32x4_t{w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]});
  }
  if (ht == 0) {
    lds32[flag / 4] = 0u;
    lds32[done / 4] = 0u;
  }
  __syncthreads();  // the only workgroup barrier

  const int toff = 16 * (lane >> 3) + (lane & 7);  // the lane's words toff, toff + 8 of a task
  // the lane's first row is toff + 8 where (lane >> 3) is odd: every 16-lane group of a
  // ds_read_b128 (8-lane group of a ds_write_b128) then touches distinct rows mod 16
  const bool flip = ((lane >> 3) & 1) != 0;

  // the lane's current segment and the vector's piece under it (positions only grow)
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
  uint64_t seg_ptr = 0;
  uint32_t seg_dt = FKS_F32;
  auto load_seg = [&]() {
    if (cur < a.nsegs) {
      const DevSeg sg = a.segs[cur];
      const ProjMtVecEntry e = a.pv[cur];
      seg_start = sg.start;
      seg_end = sg.start + sg.numel;
      seg_ptr = e.ptr;
      seg_dt = (uint32_t)e.dtype;
    } else {
      seg_start = seg_end = INT64_MAX;
    }
    // drained here (rare), so that the cached segment registers are never "possibly pending" later
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
  };
  load_seg();

  // The lane's two vector elements of task n, toff and toff + 8 of the task (one 16-block: the same
  // segment), each as two 16-bit loads: the halves of an f32 element, or a 2-byte element twice.
  struct Slot { uint32_t lo1, hi1, lo2, hi2, meta; };  // meta: on | dtype << 1
  auto fetch = [&](const int n) -> Slot {
    Slot sl;
    const int u1 = kTaskWords * n + toff;
    const int64_t s1 = wbase + u1;
    while (s1 >= seg_end) { cur++; load_seg(); }
    const bool on = u1 < nwords && s1 >= seg_start;
    const uint64_t ptr = on ? seg_ptr : (uint64_t)(uintptr_t)a.sink;
    const uint32_t dt = on ? seg_dt : (uint32_t)FKS_F32;
    const uint64_t e = on ? (uint64_t)(s1 - seg_start) : 0u;
    const bool wide = dt == (uint32_t)FKS_F32;
    const uint64_t p1 = ptr + (e << (wide ? 2 : 1)), p2 = p1 + (wide ? 32u : 16u), hi = wide ? 2u : 0u;
    sl.lo1 = *reinterpret_cast<pmbs_gu16*>(p1);
    sl.hi1 = *reinterpret_cast<pmbs_gu16*>(p1 + hi);
    sl.lo2 = *reinterpret_cast<pmbs_gu16*>(p2);
    sl.hi2 = *reinterpret_cast<pmbs_gu16*>(p2 + hi);
    sl.meta = (on ? 1u : 0u) | (dt << 1);
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

  double acc[kBsSeeds];  // seed k's sum over this lane's elements of the chunk
#pragma unroll
  for (int k = 0; k < kBsSeeds; k++) acc[k] = 0.0;

  // ---- the chain of the lane's two elements through the half's seeds
  auto chain = [&](const Slot& sl, uint32_t (&oa)[8], uint32_t (&ob)[8]) {
    bs::transpose8(oa);
    bs::transpose8(ob);
    const uint32_t dt = sl.meta >> 1;
    // an off lane enters +0: its products are zeros whatever its z, and its sums stay +0
    const double v1 = (sl.meta & 1u) ? (double)widen(sl.lo1, sl.hi1, dt) : 0.0;
    const double v2 = (sl.meta & 1u) ? (double)widen(sl.lo2, sl.hi2, dt) : 0.0;
#pragma unroll
    for (int k = 0; k < kBsSeeds; k++) {
      if (FULL || k < nseeds) {
        // z = bf16(R[a] C[b]) + 0, bf16(R[a] S[b]) + 0 (normal_fill_16<BFloat16>: an exact f32
        // product, one rounding; the fma's +0 turns -0 into +0 like "+ mean")
        const float r = lds_f32(byte_index<2>(oa[k & 7], k >> 3));
        const f32x2_t rr = {r, r}, zero = {0.0f, 0.0f};
        const f32x2_t cs = lds_f32x2(1024u + byte_index<3>(ob[k & 7], k >> 3));
        const f32x2_t z = rnd2<FKS_BF16>(__builtin_elementwise_fma(rr, cs, zero));
        acc[k] = __fma_rn(v1, (double)z.x, acc[k]);  // exact product, one rounding per addition
        acc[k] = __fma_rn(v2, (double)z.y, acc[k]);
      }
      // the lookups of one byte column (8 seeds) at a time
      if ((k & 7) == 7) asm volatile("" ::: "memory");
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

  // ---- the chunk's sums: per seed the 64-lane butterfly (lane k keeps seed k's), then the half's
  // waves in wave order through the half's row
  double mine = 0.0;
#pragma unroll
  for (int k = 0; k < kBsSeeds; k++) {
    if (FULL || k < nseeds) {
      const double s = wave_sum(acc[k]);
      mine = lane == k ? s : mine;
    }
  }
  while (__builtin_amdgcn_readfirstlane(flag_load(done)) < (uint32_t)hw) __builtin_amdgcn_s_sleep(1);
  asm volatile("" ::: "memory");
  if (lane < kBsSeeds) {
    lds_f64_t* slot = (lds_f64_t*)(size_t)(red + 8u * (uint32_t)lane);
    const double sum = hw ? *slot + mine : mine;
    if (hw + 1 < W) *slot = sum;
    else if (lane < nseeds) a.partial[(size_t)c * kBsPassSeeds + (size_t)(sfirst + lane)] = sum;
  }
  if (lane == 0) flag_store(done, (uint32_t)hw + 1u);
}

// One workgroup per seed of the pass: thread t adds rows t, t + 64, ... of the sequence [the
// bit-sliced launch's chunks | the rows of the seed's 19-seed sub-pass] in order; the 64 sums are
// then added in order.
__global__ __launch_bounds__(64) void fks_project_mt_bs_reduce_kernel(const double* bs, int nbs, const double* sub,
                                                                      int nrows, int64_t sub_stride, double* out) {
  __shared__ double sh[64];
  const int s = (int)blockIdx.x, t = (int)threadIdx.x;
  const double* const srow = sub + (int64_t)(s / kMaxSeedsPerPass) * sub_stride + s % kMaxSeedsPerPass;
  double sum = 0.0;
  for (int b = t; b < nbs + nrows; b += 64)
    sum += b < nbs ? bs[(size_t)b * kBsPassSeeds + (size_t)s] : srow[(size_t)(b - nbs) * kPhxSeeds];
  sh[t] = sum;
  __syncthreads();
  if (t == 0) {
    double v = sh[0];
#pragma unroll
    for (int k = 1; k < 64; k++) v += sh[k];
    out[s] = v;
  }
}

template <bool FULL>
int pmbs_launch(const ProjMtBsArgs& a, void* stream) {
  static PerDevice attr;
  if (int e = ensure_lds_attr(attr, &fks_project_mt_bs_kernel<FULL>, kLdsBytes)) return e;
  hipLaunchKernelGGL((fks_project_mt_bs_kernel<FULL>), dim3((unsigned)(a.split ? a.nchunks / 2 : a.nchunks)),
                     dim3(kPmbsThreads), kLdsBytes, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // namespace

int launch_project_mt_bs(const ProjMtBsArgs& a, void* stream) {
  if (a.nseeds < 1 || a.nseeds > kBsPassSeeds || (a.split != 0) != (a.nseeds <= kBsSeeds) || a.nchunks < 2 ||
      a.nchunks % 2 || a.nsegs < 1 || !a.states || !a.segs || !a.chunk_block || !a.sink || !a.partial || !a.pv)
    return -FKS_EINVAL;
  if (int e = ensure_tables()) return e;
  // FULL: 32 seeds in each half (a split pass of 32, a two-half pass of 64)
  return a.nseeds % kBsSeeds == 0 ? pmbs_launch<true>(a, stream) : pmbs_launch<false>(a, stream);
}

int launch_project_mt_bs_reduce(const double* bs, int nbs, const double* sub, int nrows, int64_t sub_stride,
                                int nseeds, double* out, void* stream) {
  if (nseeds < 1 || nseeds > kBsPassSeeds || nbs < 0 || nrows < 0 || nbs + nrows < 1 || (nbs && !bs) ||
      (nrows && !sub) || !out)
    return -FKS_EINVAL;
  hipLaunchKernelGGL(fks_project_mt_bs_reduce_kernel, dim3((unsigned)nseeds), dim3(64), 0, (hipStream_t)stream, bs,
                     nbs, sub, nrows, sub_stride, out);
  return (int)hipGetLastError();
}

}  // namespace fks
