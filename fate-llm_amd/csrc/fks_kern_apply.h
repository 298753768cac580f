// fks_kern_apply.h -- the CPU stream's apply kernels over fast segments: fks_apply_kernel
// (19-seed passes, and the double-buffered partial passes), fks_small2_kernel (passes of at
// most kSmallK seeds) and fks_zreplay_kernel (one-seed bf16 passes replaying stored z indices).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "fks_internal.h"
#include "fks_dev_lds.h"
#include "fks_dev_update.h"
#include "fks_dev_mt.h"
#include "fks_dev_zgen.h"

namespace fks {
namespace {

// ------------------------------------------------------------------ apply kernel
// All seeds of the pass: every state-word read of the block is issued up front
// (latency hidden behind the z math of earlier seeds), z for every seed next, then
// the sequential per-element update chain in seed order.  (Staging every table index,
// then every lookup, then the products measured no faster.)
template <int DT, int MODE, int NS>
__device__ __forceinline__ void pair_all(const uint8_t* lds, int st_off, const float* g, float lr, float wd,
                                         bool has_wd, float ps, float& p1, float& p2) {
  uint32_t r1[NS], r2[NS];
#pragma unroll
  for (int k = 0; k < NS; k++) {
    const uint64_t w = lds_u64(st_off + k * kWinBytes);  // (word j, word j+8), permuted window
    r1[k] = (uint32_t)w;
    r2[k] = (uint32_t)(w >> 32);
  }
  f32x2_t z[NS];
#pragma unroll
  for (int k = 0; k < NS; k++) z[k] = z_pair2<DT>(lds, r1[k], r2[k]);
  f32x2_t p = {p1, p2};
#pragma unroll
  for (int k = 0; k < NS; k++) p = apply_pair<DT, MODE>(p, z[k], g[k], lr, wd, has_wd, ps);
  p1 = p.x;
  p2 = p.y;
}

// one seed (partial passes)
template <int DT, int MODE>
__device__ __forceinline__ void pair_one(const uint8_t* lds, int st_off, int k, float g, float lr, float wd,
                                         bool has_wd, float ps, float& p1, float& p2, bool upd = true) {
  const uint64_t w = lds_u64(st_off + k * kWinBytes);
  const f32x2_t z = z_pair2<DT>(lds, (uint32_t)w, (uint32_t)(w >> 32));
  f32x2_t p = {p1, p2};
  p = apply_pair<DT, MODE>(p, z, g, lr, wd, has_wd, ps, upd);
  p1 = p.x;
  p2 = p.y;
}

// DB (partial passes of <= kSmallK seeds): the windows are double-buffered -- window k
// of buffer s at kLdsTabBytes + (s * nseeds + k) * kWinBytes, + one spare for the twist's
// over-read -- and a sixth wave (kDbThreads) twists window 0 of block b+1 out of place
// while the five pair waves run block b (windows 1..3 are twisted by pair waves 4..2):
// one barrier per block instead of two, and for K=1 the twist leaves the pair waves'
// critical path (it was a third of a K=1 pass).
constexpr int kDbThreads = kApplyThreads + 64;
template <int DT, int MODE, bool FULL, bool DB = false>
__global__ __launch_bounds__(DB ? kDbThreads : kApplyThreads,
                             DB ? kDbMinWaves : (kApplyWgPerCu * kApplyThreads + 255) / 256) void fks_apply_kernel(ApplyArgs a) {
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
    logf_tab_fill(0u, tid, DB ? kDbThreads : kApplyThreads);
  }
  const int buf1 = DB ? nseeds * kWinBytes : 0;  // DB: the jump windows go to buffer 1
  for (int idx = tid; idx < nseeds * kMtN; idx += (DB ? kDbThreads : kApplyThreads)) {
    const int k = idx / kMtN, i = idx - k * kMtN;
    lds_st(kLdsTabBytes + buf1 + k * kWinBytes + 4 * wperm(i), a.states[((size_t)k * a.nchunks + c) * kMtN + i]);
  }
  TwistPlan plan;
  twist_plan(plan, tid, kLdsTabBytes);
  // per-seed multipliers: wave-uniform, kept in SGPRs for the whole kernel
  float gk[kMaxSeedsPerPass];
#pragma unroll
  for (int k = 0; k < kMaxSeedsPerPass; k++)
    gk[k] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(k < nseeds ? a.g[k] : 0.0f)));
  // a device-side perturb_step (one seed): g and the apply decision from device memory
  bool upd = true;
  float g0 = gk[0];
  if (MODE == kModePerturbUpdate && a.gdev) {
    g0 = dev_value_g<DT == FKS_F16 ? FKS_F16 : DT>(a.gdev);
    upd = dev_value_apply(a.gdev);
  }
  __syncthreads();
  // DB: window tw is twisted by wave kWaves - tw (window 0 by the sixth, twist-only wave)
  const int tw = kWaves - plan.wave;
  const bool twister = DB && tw >= 0 && tw < nseeds;
  if constexpr (DB) {  // block b0 into buffer 0
    if (twister && b0 < b1) twist_oop(plan, buf1 + tw * kWinBytes, tw * kWinBytes);
    __syncthreads();
  }

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
  float seg_lr = 0.0f, seg_wd = 0.0f, seg_ps = 0.0f;
  bool seg_wdf = false;
  auto load_seg = [&]() {
    if (cur < a.nsegs) {
      const DevSeg sg = a.segs[cur];
      seg_start = sg.start;
      seg_end = sg.start + sg.numel;
      seg_ptr = sg.ptr;
      seg_lr = sg.lr;
      seg_ps = sg.ps;
      seg_wd = sg.wd;
      seg_wdf = (sg.flags & FKS_HAS_WD) != 0;
    } else {
      seg_start = seg_end = INT64_MAX;
    }
    // Drain here (rare: once per segment change), so the cached segment registers are
    // never "possibly pending" later: otherwise every block's address computation would
    // carry a vmcnt(0) that also waits for the previous block's stores.
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), expcnt/lgkmcnt untouched
  };
  load_seg();

  // software pipeline: block b+1's parameters are fetched before block b's Box-Muller
  // Parameter traffic in pairs of ADJACENT elements: lane q (slot r = q%8 of its
  // 16-block) owns elements j1 = 16m + r and j1 + 8; an even lane moves the pair
  // (j1, j1+1), an odd lane the pair (j1+7, j1+8), and the two lanes swap the halves
  // that belong to each other (one DPP op) -- one dword (bf16) / dwordx2 (f32) access
  // per lane instead of two scattered ones.
  const bool odd = (tid & 1) != 0;
  // storage: the parameters, or (kModeDelta) the f32 delta buffer the z of dtype DT is
  // accumulated into
  using ST = Traits<MODE == kModeDelta ? FKS_F32 : DT>;
  constexpr int kEs = (is_f32(DT) || MODE == kModeDelta) ? 4 : 2;
  typedef typename ST::Pair Pair;
  struct Slot { uint64_t addr; float lr, wd, ps; uint32_t wdf, on; Pair raw; };
  auto fetch = [&](int64_t b) -> Slot {
    Slot sl;
    const int64_t s1 = (int64_t)kMtN * b + j1;
    while (s1 >= seg_end) { cur++; load_seg(); }
    const bool on = lane_on && s1 >= seg_start;
    sl.on = on;
    sl.lr = seg_lr; sl.wd = seg_wd; sl.ps = seg_ps; sl.wdf = seg_wdf;
    // off lanes read and write a workspace sink, so the load and the store are
    // unconditional: the store is then always counted in vmcnt and the next wait for a
    // prefetched pair can leave it outstanding (a maybe-executed store makes the
    // compiler wait for it)
    sl.addr = on ? seg_ptr + (uint64_t)(s1 - seg_start + (odd ? 7 : 0)) * kEs : (uint64_t)(uintptr_t)a.sink;
    sl.raw = 0;
    if (MODE != kModeWriteZ) sl.raw = ST::load_pair(sl.addr);
    return sl;
  };
  // One block: twist, prefetch block b+1 (returned), Box-Muller + update chain, store.
  auto step = [&](Slot sl, int64_t b) -> Slot {
    int buf = 0;  // byte offset of the buffer holding block b (DB)
    if constexpr (DB) {
      buf = (int)((b - b0) & 1) * nseeds * kWinBytes;
      const int other = nseeds * kWinBytes - buf;
      if (twister && b + 1 < b1)  // block b+1, out of place
        twist_oop(plan, buf + tw * kWinBytes, other + tw * kWinBytes);
      if (plan.wave == kWaves) {  // the twist-only wave
        __syncthreads();
        return sl;
      }
    } else {
      __syncthreads();  // every wave is done reading block b-1's words
      twist_all(plan, nseeds);  // the raw words of stream block b
      __syncthreads();  // every window holds block b
    }
    const Slot nxt = fetch(b + 1 < b1 ? b + 1 : b);  // (the last block re-reads itself, unused)
    {  // every lane: off lanes compute garbage into the sink
      // even lane holds (p1, partner's p1), odd lane (partner's p2, p2)
      const uint32_t keep = odd ? ST::hi(sl.raw) : ST::lo(sl.raw);
      const uint32_t got = swap_adjacent(odd ? ST::lo(sl.raw) : ST::hi(sl.raw));
      float p1 = ST::cvt(odd ? got : keep), p2 = ST::cvt(odd ? keep : got);
      if constexpr (FULL) {
        pair_all<DT, MODE, kMaxSeedsPerPass>(lds, st_off, gk, sl.lr, sl.wd, sl.wdf != 0, sl.ps, p1, p2);
      } else {
        // a.g[k] straight from the kernel-argument segment (one s_load per seed): a
        // dynamically indexed gk[] would be copied to VGPRs and indexed per seed
        for (int k = 0; k < nseeds; k++)
          pair_one<DT, MODE>(lds, st_off + buf, k, MODE == kModePerturbUpdate ? g0 : a.g[k], sl.lr, sl.wd,
                             sl.wdf != 0, sl.ps, p1, p2, upd);
      }
      const uint32_t b1v = ST::bits(p1), b2v = ST::bits(p2);
      const uint32_t back = swap_adjacent(odd ? b1v : b2v);  // even gets partner's p1, odd partner's p2
      const Pair out = odd ? ST::pack(back, b2v) : ST::pack(b1v, back);
      ST::store_pair(sl.addr, out);
    }
    if constexpr (DB) __syncthreads();  // block b+1 is twisted; block b's buffer is free
    return nxt;
  };
  Slot sa = fetch(b0);
  // a store after the first prefetch, so the loop is entered with the same pending
  // (load, store) shape as the back edge and the first wait can leave a store in flight
  *reinterpret_cast<volatile uint32_t*>(a.sink + 1) = 0u;
  for (int64_t b = b0; b < b1; b++) sa = step(sa, b);
}

// ------------------------------------------------------------------ small-K kernel v2
// (Other bf16 table layouts for the small-K kernel -- R|C|S f32, (C,S) packed as bf16 --
// measured within noise or slower: profiles/r02_smallk_ab.log.)
// bf16 z pair from the two table byte offsets (x8) of temper_pair_u8x8: the lookups and
// the rounding of z_pair_bf16_raw (default table layout)
__device__ __forceinline__ f32x2_t z_bf16_idx8(uint32_t a8, uint32_t b8) {
  const float r = lds_f32(a8 >> 1);
  const f32x2_t rr = {r, r}, zero = {0.0f, 0.0f};
  return rnd2<FKS_BF16>(__builtin_elementwise_fma(rr, lds_f32x2(kLdsCsOff + b8), zero));
}

// fks_small2_kernel<DT, MODE>: passes of <= kSmallK seeds over fast segments (the ZO
// step's perturb / restore + update / K=1 update, optimizer.py:152-173, :146-148).
// 3 pair waves + 1 twist wave per chunk.  Pair lane q < 156 owns TWO Box-Muller pairs of
// every block, (j, j+8) and (j+1, j+9) with j = 16 (q/4) + 2 (q%4):
//   * the four raw words are adjacent in the permuted window (wperm): one ds_read_b128
//     per seed;
//   * the four parameters are two aligned element pairs (j, j+1) and (j+8, j+9): two
//     dword (bf16) / dwordx2 (f32) accesses, no exchange between lanes.
// The twist wave twists every window of block b+1 out of place while the pair waves
// run block b (double-buffered windows, one barrier per block).  Window k of buffer B
// sits at window slot 2k + B and the loops are unrolled by two blocks, so every LDS
// offset of a block is an immediate.
// Segment walk: a block lying inside one segment (all but a few hundred blocks of a
// model) is addressed from a WAVE-UNIFORM base (scalar registers: segment cursor, block
// range, base address and the segment's scalars) plus the lane's fixed byte offset, so
// it costs no vector instruction; a block that straddles segments or a gap takes a
// per-lane path (segment scan, no prefetch).  Lanes q >= 156 mirror lane 155 (same
// loads, same values stored to the same addresses).
constexpr int kSm2Threads = 256;
constexpr int kSm2PairLanes = kMtN / 4;  // 156
constexpr int kSm2TwistWave = 3;


// ZM 1 (bf16, one seed): also store every block's table indices, one u32 per pair lane
// (bytes a_j, b_j, a_j+1, b_j+1: 1 B per parameter) at zidx[(block - zlo) * 156 + q],
// for fks_zreplay_kernel to replay (the ZO step's second and third calls).  (A replay
// through this kernel's own structure -- ZM 2, 3 waves, no twist -- streamed at 3.8
// TB/s against 5.6 for the flat kernel: profiles/r02_smallk_ab.log.)
constexpr int kZidxPerBlock = kSm2ZidxPerBlock;  // u32 per block
static_assert(kSm2ZidxPerBlock == kSm2PairLanes, "one z-index word per pair lane");
template <int DT, int MODE, int ZM = 0>
__global__ __launch_bounds__(kSm2Threads, kSm2MinWaves) void fks_small2_kernel(ApplyArgs a) {
  static_assert(ZM == 0 || (ZM == 1 && DT == FKS_BF16), "z-index store: bf16");
  extern __shared__ __attribute__((aligned(16))) uint32_t lds32[];
  uint8_t* lds = reinterpret_cast<uint8_t*>(lds32);
  if ((uint32_t)(size_t)(lds_u32_t*)lds32 != 0u) __builtin_trap();
  const int tid = threadIdx.x;
  const int c = blockIdx.x;
  const int nseeds = a.nseeds;
  const int64_t b0 = a.chunk_block[c];
  const int nblk = (int)(a.chunk_block[c + 1] - b0);  // host: a chunk is far below 2^31 blocks

  if constexpr (DT == FKS_BF16) {
    tab_bf16_fill(lds, tid, (int)blockDim.x);
  } else if constexpr (DT == kDtF32Libm) {
    logf_tab_fill(0u, tid, kSm2Threads);
  }
  // the chunk-start windows go to buffer 1, twisted into buffer 0 for block b0
  for (int idx = tid; idx < nseeds * kMtN; idx += kSm2Threads) {
    const int k = idx / kMtN, i = idx - k * kMtN;
    lds_st(kLdsTabBytes + (2 * k + 1) * kWinBytes + 4 * wperm(i), a.states[((size_t)k * a.nchunks + c) * kMtN + i]);
  }
  TwistPlan plan;
  twist_plan(plan, tid, kLdsTabBytes);
  // (rotating the twist role across the workgroups' waves, so that twist waves do not
  // share a SIMD, measured no different: profiles/r02_smallk_ab.log)
  const int vw = plan.wave;
  __syncthreads();
  if (vw == kSm2TwistWave) {
    auto twist_into = [&](auto dst_c) __attribute__((always_inline)) {
      constexpr int D = decltype(dst_c)::value;
#pragma unroll
      for (int k = 0; k < kSmallK; k++)
        if (k < nseeds) twist_oop_reg(plan, (2 * k + 1 - D) * kWinBytes, (2 * k + D) * kWinBytes);
    };
    if (nblk > 0) twist_into(std::integral_constant<int, 0>{});
    __syncthreads();
    for (int t = 0; t < nblk; t += 2) {
      if (t + 1 < nblk) twist_into(std::integral_constant<int, 1>{});
      __syncthreads();  // block t+1 is in buffer 1; block t's buffer 0 is free
      if (t + 1 >= nblk) break;
      if (t + 2 < nblk) twist_into(std::integral_constant<int, 0>{});
      __syncthreads();
    }
    return;
  }
  __syncthreads();  // block b0 is in buffer 0

  const int vt = 64 * vw + (tid & 63);
  const int q = vt < kSm2PairLanes ? vt : kSm2PairLanes - 1;
  const int j = 16 * (q >> 2) + 2 * (q & 3);
  const uint32_t st_off = kLdsTabBytes + 4 * wperm(j);  // words (j, j+8, j+1, j+9), 16-byte aligned
  float gk[kSmallK];
#pragma unroll
  for (int k = 0; k < kSmallK; k++) gk[k] = rflf(k < nseeds ? a.g[k] : 0.0f);
  bool upd = true;  // a device-side perturb_step: g and the apply decision from device memory
  if (MODE == kModePerturbUpdate && a.gdev) {
    gk[0] = dev_value_g<DT>(a.gdev);
    upd = dev_value_apply(a.gdev);
  }

  using ST = Traits<MODE == kModeDelta ? FKS_F32 : DT>;
  constexpr int kEs = (is_f32(DT) || MODE == kModeDelta) ? 4 : 2;
  constexpr uint32_t kBlockBytes = kMtN * kEs;
  typedef typename ST::Pair Pair;
  const uint32_t joff = (uint32_t)j * kEs;

  // wave-uniform segment cursor; block t of the chunk (t relative to b0) is fast when
  // t in [fb, eb): it starts at or after the segment's start and ends within it
  int cur = 0;
  {
    const int64_t s0 = (int64_t)kMtN * b0;
    int lo = 0, hi = a.nsegs;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const DevSeg& sm = a.segs[mid];
      if ((int64_t)rfl64((uint64_t)(sm.start + sm.numel)) <= s0) lo = mid + 1; else hi = mid;
    }
    cur = lo;
  }
  int fb = 0, eb = 0, nb = 0;
  uint64_t base0 = 0;
  float u_lr = 0.0f, u_wd = 0.0f, u_ps = 0.0f;
  bool u_wdf = false;
  auto load_seg = [&]() __attribute__((always_inline)) {
    if (cur < a.nsegs) {
      const DevSeg& sg = a.segs[cur];
      const int64_t st = (int64_t)rfl64((uint64_t)sg.start);
      const int64_t en = st + (int64_t)rfl64((uint64_t)sg.numel);
      const int64_t lim = (int64_t)nblk + 1;
      auto rel = [&](int64_t blk) __attribute__((always_inline)) -> int { const int64_t r = blk - b0; return (int)(r < -1 ? -1 : (r > lim ? lim : r)); };
      fb = rel((st + kMtN - 1) / kMtN);
      eb = rel(en / kMtN);
      nb = rel((en + kMtN - 1) / kMtN);
      base0 = rfl64(sg.ptr) + (uint64_t)((int64_t)kMtN * b0 - st) * kEs;
      u_lr = rflf(sg.lr);
      u_wd = rflf(sg.wd);
      u_ps = rflf(sg.ps);
      u_wdf = (rfl(sg.flags) & FKS_HAS_WD) != 0;
    } else {
      fb = eb = 0;
      nb = INT32_MAX;
    }
  };
  load_seg();

  // (cur at fetch time: the first segment ending after block t's start, where a
  // straddling block's lanes start their scan; fetching block t+1 may move cur on)
  struct Slot { uint64_t base; int cur; bool fast; Pair r0, r1; };
  auto fetch = [&](int t) __attribute__((always_inline)) -> Slot {
    Slot sl;
    while (t >= nb) { cur++; load_seg(); }
    sl.cur = cur;
    sl.fast = t >= fb && t < eb;
    // a block that is not fast prefetches from the sink (4 KB, any lane's offset fits):
    // the loads stay unconditional, so no register is reset under a pending load
    sl.base = sl.fast ? base0 + (uint64_t)(uint32_t)t * kBlockBytes : (uint64_t)(uintptr_t)a.sink;
    if (MODE != kModeWriteZ) {
      sl.r0 = ST::load_pair(sl.base + joff);
      sl.r1 = ST::load_pair(sl.base + joff + 8 * kEs);
    } else {
      sl.r0 = 0;
      sl.r1 = 0;
    }
    return sl;
  };

  // the block's four parameters through every seed of the pass, in seed order
  // ZM 1: the block's seed-0 table offsets, computed once per block for every lane
  u32x2_t zab = {0u, 0u}, zcd = {0u, 0u};
  auto run = [&](auto buf_c, Pair& r0, Pair& r1, float lr, float wd, bool wdf, float ps) __attribute__((always_inline)) {
    constexpr int B = decltype(buf_c)::value;
    // pA = (p_j, p_j+8), pB = (p_j+1, p_j+9): the two Box-Muller pairs' parameters
    f32x2_t pA = {ST::cvt(ST::lo(r0)), ST::cvt(ST::lo(r1))};
    f32x2_t pB = {ST::cvt(ST::hi(r0)), ST::cvt(ST::hi(r1))};
#pragma unroll
    for (int k = 0; k < kSmallK; k++) {
      if (k < nseeds) {  // wave-uniform
        f32x2_t zA, zB;
        if (ZM == 1 && k == 0) {
          zA = z_bf16_idx8(zab.x, zab.y);
          zB = z_bf16_idx8(zcd.x, zcd.y);
        } else {
          const u32x4_t w = lds_u4(st_off + (uint32_t)((2 * k + B) * kWinBytes));
          zA = z_pair2<DT>(lds, w.x, w.y);
          zB = z_pair2<DT>(lds, w.z, w.w);
        }
        pA = apply_pair<DT, MODE>(pA, zA, gk[k], lr, wd, wdf, ps, upd);
        pB = apply_pair<DT, MODE>(pB, zB, gk[k], lr, wd, wdf, ps, upd);
      }
    }
    if constexpr (sizeof(Pair) == 4) {  // bf16: the high halves of the bf16-exact results
      r0 = __builtin_amdgcn_perm(__float_as_uint(pB.x), __float_as_uint(pA.x), 0x07060302u);
      r1 = __builtin_amdgcn_perm(__float_as_uint(pB.y), __float_as_uint(pA.y), 0x07060302u);
    } else {
      r0 = ST::pack(ST::bits(pA.x), ST::bits(pB.x));
      r1 = ST::pack(ST::bits(pA.y), ST::bits(pB.y));
    }
  };

  auto block = [&](auto buf_c, Slot& sl, int t) __attribute__((always_inline)) {
    if constexpr (ZM == 1) {
      constexpr int B = decltype(buf_c)::value;
      const u32x4_t w = lds_u4(st_off + (uint32_t)(B * kWinBytes));
      u32x2_t w0, w1;
      w0.x = w.x;
      w0.y = w.y;
      w1.x = w.z;
      w1.y = w.w;
      zab = temper_pair_u8x8(w0);
      zcd = temper_pair_u8x8(w1);
      a.zidx[((size_t)(b0 + t - a.zlo)) * kZidxPerBlock + q] =
          (zab.x >> 3) | (zab.y << 5) | (zcd.x << 13) | (zcd.y << 21);
    }
    {
      if (sl.fast) {
        run(buf_c, sl.r0, sl.r1, u_lr, u_wd, u_wdf, u_ps);
        ST::store_pair(sl.base + joff, sl.r0);
        ST::store_pair(sl.base + joff + 8 * kEs, sl.r1);
      } else {
        // straddling block: each lane finds its own segment from the cursor on
        const int64_t s1 = (int64_t)kMtN * (b0 + t) + j;
        int cc = sl.cur;
        bool in = false;
        DevSeg sg;
        while (cc < a.nsegs) {
          sg = a.segs[cc];
          if (s1 < sg.start + sg.numel) { in = s1 >= sg.start; break; }
          cc++;
        }
        if (in) {
          const uint64_t addr = sg.ptr + (uint64_t)(s1 - sg.start) * kEs;
          Pair r0 = 0, r1 = 0;
          if (MODE != kModeWriteZ) {
            r0 = ST::load_pair(addr);
            r1 = ST::load_pair(addr + 8 * kEs);
          }
          run(buf_c, r0, r1, sg.lr, sg.wd, (sg.flags & FKS_HAS_WD) != 0, sg.ps);
          ST::store_pair(addr, r0);
          ST::store_pair(addr + 8 * kEs, r1);
        }
      }
    }
    __syncthreads();  // the twist wave has block t+1 in place
  };

  // (fetching two blocks ahead measured slower: profiles/r02_smallk_ab.log)
  Slot s0 = fetch(0);
  // a store after the first prefetch, so the loop is entered with the same pending
  // (load, store) shape as the back edge
  *reinterpret_cast<volatile uint32_t*>(a.sink + 1) = 0u;
  for (int t = 0; t < nblk; t += 2) {
    Slot s1 = fetch(t + 1 < nblk ? t + 1 : t);  // (the last block re-reads itself, unused)
    block(std::integral_constant<int, 0>{}, s0, t);
    if (t + 1 >= nblk) break;
    s0 = fetch(t + 2 < nblk ? t + 2 : t + 1);
    block(std::integral_constant<int, 1>{}, s1, t + 1);
  }
}

// ------------------------------------------------------------------ z-index replay
// fks_zreplay_kernel<MODE>: a one-seed bf16 pass whose z comes from the table indices a
// fks_small2_kernel<.., ZM 1> pass stored for the same seed (ZCache): no generator, no
// windows, no barriers -- a streaming pass.  Each thread takes 8 consecutive stream
// positions (half a 16-block: 16 B of parameters, one dwordx4 load and store; a wave
// covers 1 KB contiguously) and the 16-block's index record (16 B: a_i, b_i for its 8
// Box-Muller pairs, at the record's stream offset: 1 byte per position), which both
// halves of the 16-block read.  The first half takes z_i = R[a_i] C[b_i], the second
// z_{i+8} = R[a_i] S[b_i] (DistributionTemplates.h:141-146), each rounded once as
// z_pair_bf16_raw; then the update chain of apply_pair, element pairs (i, i+1).
// Workgroup c walks the stream positions of chunk c in tiles of 256 x 8; a tile inside
// one segment is addressed from a wave-uniform base, a straddling tile per lane.
constexpr int kZrThreads = 256;
typedef __attribute__((address_space(1))) u32x4_t gu32x4_t;
__device__ __forceinline__ u32x4_t gload4(uint64_t addr) { return *reinterpret_cast<const gu32x4_t*>(addr); }
__device__ __forceinline__ void gstore4(uint64_t addr, u32x4_t v) { *reinterpret_cast<gu32x4_t*>(addr) = v; }
constexpr int kZrTile = kZrThreads * 8;  // stream positions per tile

template <int MODE>
__global__ __launch_bounds__(kZrThreads) void fks_zreplay_kernel(ApplyArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds32[];
  if ((uint32_t)(size_t)(lds_u32_t*)lds32 != 0u) __builtin_trap();
  const int tid = threadIdx.x;
  const int c = blockIdx.x;
  // R | C | S as three f32[256]: one b32 lookup per table
  for (int i = tid; i < 256; i += kZrThreads) {
    reinterpret_cast<float*>(lds32)[i] = c_tab_bf16[i];
    reinterpret_cast<float*>(lds32)[256 + i] = c_tab_bf16[256 + i];
    reinterpret_cast<float*>(lds32)[512 + i] = c_tab_bf16[512 + i];
  }
  __syncthreads();
  // tiles of the whole call are dealt round-robin over the workgroups, so the workgroups
  // in flight stream neighbouring addresses (few pages live at a time, as a grid-stride
  // elementwise kernel; one chunk per workgroup measured slower)
  const int64_t p0 = (int64_t)kMtN * a.chunk_block[0] + (int64_t)c * kZrTile;
  const int64_t p1 = (int64_t)kMtN * a.chunk_block[a.nchunks];
  const int64_t tstep = (int64_t)gridDim.x * kZrTile;
  const int64_t zbase = (int64_t)kMtN * a.zlo;
  const uint64_t zb = (uint64_t)(uintptr_t)a.zidx;
  float g = rflf(a.g[0]);
  bool upd = true;
  if (MODE == kModePerturbUpdate && a.gdev) {
    g = dev_value_g<FKS_BF16>(a.gdev);
    upd = dev_value_apply(a.gdev);
  }
  const uint32_t half = (uint32_t)tid & 1u;  // 0: first half of the 16-block (cos), 1: second (sin)
  const uint32_t cs_tab = half ? 2048u : 1024u;

  int cur = 0;
  {
    int lo = 0, hi = a.nsegs;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const DevSeg& sm = a.segs[mid];
      if ((int64_t)rfl64((uint64_t)(sm.start + sm.numel)) <= p0) lo = mid + 1; else hi = mid;
    }
    cur = lo;
  }
  // the 8 elements e[0..7] through the seed; z from the record's bytes
  auto chain = [&](u32x4_t pv, u32x4_t rec, float lr, float wd, bool wdf, float ps) __attribute__((always_inline)) -> u32x4_t {
    const uint32_t w[4] = {pv.x, pv.y, pv.z, pv.w};
    const uint32_t r[4] = {rec.x, rec.y, rec.z, rec.w};
    uint32_t o[4];
#pragma unroll
    for (int m = 0; m < 4; m++) {  // elements 2m, 2m+1: pairs 2m (bytes 0,1 of r[m]) and 2m+1 (bytes 2,3)
      const uint32_t ri = r[m];
      const float ra = lds_f32((ri << 2) & 0x3FCu), rb = lds_f32((ri >> 14) & 0x3FCu);
      const float ca = lds_f32(cs_tab + ((ri >> 6) & 0x3FCu)), cb = lds_f32(cs_tab + ((ri >> 22) & 0x3FCu));
      const f32x2_t rr = {ra, rb}, cc = {ca, cb}, zero = {0.0f, 0.0f};
      const f32x2_t z = rnd2<FKS_BF16>(__builtin_elementwise_fma(rr, cc, zero));
      f32x2_t pe = {__uint_as_float(w[m] << 16), __uint_as_float(w[m] & 0xffff0000u)};
      pe = apply_pair<FKS_BF16, MODE>(pe, z, g, lr, wd, wdf, ps, upd);
      o[m] = __builtin_amdgcn_perm(__float_as_uint(pe.y), __float_as_uint(pe.x), 0x07060302u);
    }
    const u32x4_t out = {o[0], o[1], o[2], o[3]};
    return out;
  };
  const u32x4_t zero4 = {0u, 0u, 0u, 0u};
  // kZrUnroll tiles per iteration: every tile's index records and parameters are
  // loaded before the first is computed, so a wave keeps that many tiles in flight (a
  // straddling tile loads its parameters when it runs)
  struct ZSlot { int64_t t0; uint64_t base; float lr, wd, ps; int cur; bool fast, wdf; u32x4_t rec, pv; };
  // the current segment's scalars, re-read only when the walk moves on (a global load
  // here would wait for every load in flight, the prefetched tile's included)
  int64_t seg_st = INT64_MAX, seg_en = INT64_MAX;
  uint64_t seg_ptr = 0;
  float seg_lr = 0.0f, seg_wd = 0.0f, seg_ps = 0.0f;
  bool seg_wdf = false;
  auto load_seg = [&]() __attribute__((always_inline)) {
    if (cur < a.nsegs) {
      const DevSeg& sg = a.segs[cur];
      seg_st = (int64_t)rfl64((uint64_t)sg.start);
      seg_en = seg_st + (int64_t)rfl64((uint64_t)sg.numel);
      seg_ptr = rfl64(sg.ptr);
      seg_lr = rflf(sg.lr);
      seg_wd = rflf(sg.wd);
      seg_ps = rflf(sg.ps);
      seg_wdf = (rfl(sg.flags) & FKS_HAS_WD) != 0;
    } else {
      seg_st = seg_en = INT64_MAX;
    }
  };
  load_seg();
  auto zfetch = [&](int64_t t0) __attribute__((always_inline)) -> ZSlot {
    ZSlot z;
    z.t0 = t0;
    while (seg_en <= t0) {  // wave-uniform: the first segment ending after the tile's start
      cur++;
      load_seg();
    }
    z.cur = cur;
    const int64_t tend = t0 + kZrTile < p1 ? t0 + kZrTile : p1;
    z.fast = seg_st <= t0 && tend <= seg_en;
    z.base = seg_ptr + (uint64_t)(t0 - seg_st) * 2u;
    z.lr = seg_lr;
    z.wd = seg_wd;
    z.ps = seg_ps;
    z.wdf = seg_wdf;
    const int64_t pos = t0 + 8 * (int64_t)tid;
    const bool live = pos < p1;  // (lanes past the chunk's end load lane 0's addresses)
    z.rec = zero4;
    z.pv = zero4;
    if (t0 < p1) {  // wave-uniform
      z.rec = gload4(zb + (uint64_t)(((live ? pos : t0) - zbase) & ~(int64_t)15));
      if (MODE != kModeWriteZ && z.fast) z.pv = gload4(z.base + (live ? 16u * (uint32_t)tid : 0u));
    }
    return z;
  };
  auto zblock = [&](ZSlot& z) __attribute__((always_inline)) {
    const int64_t pos = z.t0 + 8 * (int64_t)tid;
    if (pos >= p1) return;
    if (z.fast) {
      gstore4(z.base + 16u * (uint32_t)tid, chain(z.pv, z.rec, z.lr, z.wd, z.wdf, z.ps));
    } else {
      int cc = z.cur;
      bool in = false;
      DevSeg sg;
      while (cc < a.nsegs) {
        sg = a.segs[cc];
        if (pos < sg.start + sg.numel) { in = pos >= sg.start; break; }
        cc++;
      }
      if (in) {
        const uint64_t ptr = sg.ptr + (uint64_t)(pos - sg.start) * 2u;
        const u32x4_t pv = MODE == kModeWriteZ ? zero4 : gload4(ptr);
        gstore4(ptr, chain(pv, z.rec, sg.lr, sg.wd, (sg.flags & FKS_HAS_WD) != 0, sg.ps));
      }
    }
  };
  constexpr int kU = kZrUnroll;
  for (int64_t t0 = p0; t0 < p1; t0 += kU * tstep) {
    ZSlot z[kU];
#pragma unroll
    for (int u = 0; u < kU; u++) z[u] = zfetch(t0 + u * tstep);
#pragma unroll
    for (int u = 0; u < kU; u++) zblock(z[u]);
  }
}

}  // namespace
}  // namespace fks
