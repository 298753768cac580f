// fks_expand_mt.hip -- seed-basis expansion on the CPU generator's MT19937 stream (include/fks.h
// fks_expand_mt_multi): out = cast(beta out + sum_s f32(c_s) z_s), the dense vector Z c of (seed,
// scalar) pairs written where the caller's tensors lie and in their dtype; the other direction of
// fks_project_mt_multi and fks_delta_accumulate's sum on this stream without its f32 buffer.  The
// plan is the geometry-only one of fks_project_mt_multi (fks_project_mt.h kProjMtGeoBase) and a
// per-call table names the output's piece under every segment, run and single element.
//
// fks_expand_mt_kernel<DT, FULL, CARRY, FINAL> takes the fast segments of one dtype on
// fks_project_mt_multi_kernel's frame: one workgroup of kApplyThreads per plan chunk, the pass's
// windows in LDS, twist_all per MT block, lane q < 312 owning the Box-Muller pair (j1, j1 + 8) of
// every block, the lane's segment looked up as it advances, the next block's elements fetched one
// iteration ahead.  Per block the lane's two sums start from the carry -- +0, or with CARRY the
// f32 the pass before staged --, the pass's at most kMaxSeedsPerPass seeds run as f32 fmas
// acc = fma(g_s, z_s, acc) in seed order (fks_delta_accumulate's chain, the coefficients by value
// in the arguments), and the sums go to the staging area as f32 or, with FINAL, through
// fma(beta, old, acc) and the cast into the output's piece: per element, 2 or 4 bytes, since an
// output is aligned to its element only.  A lane off every segment, and the 8 idle lanes, load
// the workspace sink and store nothing.  One output per pass.
// fks_expand_mt_irr_kernel takes the rest as a store visitor of the irregular frame
// (fks_dev_irr.h irr_walk): a lane with work runs the same carry, chain and store over its two
// elements of a run under the run's limit, or over its single element; no wave-wide operation.
//
// A call of k <= kMaxSeedsPerPass seeds is one pass (CARRY 0, FINAL 1): no staging area, every
// output element written once.  A longer call runs passes of kMaxSeedsPerPass through the staging
// area (fks_expand_mt.h): f32 stores lose nothing, so the chain is the one-pass chain.
//
// Compiler report (-Rpass-analysis=kernel-resource-usage, gfx950, 320-thread workgroups; every
// instance 0 B scratch and 0 AGPRs; LDS is dynamic: the tables + (seeds + 1) x 2,496 B of windows,
// at most 53,760 B, three workgroups per CU; the irregular kernel's is the irregular frame's).
// VGPRs (waves per SIMD the registers would allow) of the six instances of a dtype --
// single = one pass, +0 in, output out; first / middle / last = the passes of a staged call:
//              single full  single partial  first    middle   last full  last partial
//   bf16       108 (4)      67 (7)          98 (4)   100 (4)  114 (4)    69 (7)
//   f32        64 (8)       64 (8)          60 (8)   62 (8)   72 (7)     64 (8)
//   f32 libm   80 (6)       80 (6)          68 (7)   70 (7)   84 (5)     84 (5)
//   fks_expand_mt_irr_kernel: 121 VGPRs (4)
// The bf16 seed loop is unrolled, with a scheduling barrier every four seeds of a full pass
// (without it 68 to 144 bytes of scratch per lane); the f32 kinds keep a rolled seed loop
// (unrolled they spill 12 to 48 bytes per lane under the 128 VGPRs of three workgroups per CU).
#include <hip/hip_runtime.h>

#include "fks_internal.h"
#include "fks_expand_mt.h"
#include "fks_dev_lds.h"
#include "fks_dev_mt.h"
#include "fks_dev_zgen.h"
#include "fks_dev_irr.h"
#include "fks_dev_host.h"

namespace fks {
namespace {

typedef __attribute__((address_space(1))) float emt_gf32;
typedef __attribute__((address_space(1))) uint16_t emt_gu16;
typedef __attribute__((address_space(1))) const float emt_cgf32;
typedef __attribute__((address_space(1))) const uint16_t emt_cgu16;

#ifndef FKS_EMT_SEEDS_IN_FLIGHT  // A/B switch: seeds of a full pass between two scheduling barriers
#define FKS_EMT_SEEDS_IN_FLIGHT 4
#endif
constexpr int kEmtSeedsInFlight = FKS_EMT_SEEDS_IN_FLIGHT;

// a bf16 / f16 element widened to f32 (exact)
__device__ __forceinline__ float emt_widen16(uint32_t h, bool bf) {
  const _Float16 f = __builtin_bit_cast(_Float16, (uint16_t)h);
  return bf ? __uint_as_float(h << 16) : (float)f;
}
// the 16 bits of v rounded to nearest even to bf16 / f16 (the f32 value first, then the cast)
__device__ __forceinline__ uint32_t emt_bits16(float v, bool bf) {
  const uint32_t b = __float_as_uint(rbf_cvt(v)) >> 16;
  const uint32_t h = Traits<FKS_F16>::bits(Traits<FKS_F16>::rnd(v));
  return bf ? b : h;
}

// ------------------------------------------------------------------ fast segments
template <int DT, bool FULL, bool CARRY, bool FINAL>
__global__ __launch_bounds__(kApplyThreads, (kApplyWgPerCu * kApplyThreads + 255) / 256) void fks_expand_mt_kernel(
    ExpMtArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds32[];
  uint8_t* lds = reinterpret_cast<uint8_t*>(lds32);
  // the lds_* accessors address LDS by offset from 0: the dynamic block must start there
  if ((uint32_t)(size_t)(lds_u32_t*)lds32 != 0u) __builtin_trap();
  const int tid = threadIdx.x;
  const int c = blockIdx.x;
  const int nseeds = FULL ? kMaxSeedsPerPass : a.p.nseeds;
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
  uint64_t seg_stage = 0, seg_out = 0;  // where the segment's element 0 is staged / lies in the output
  int seg_dt = FKS_F32;                 // the output's dtype
  auto load_seg = [&]() {  // (selects, not branches: the launcher refuses a launch without segments)
    const bool have = cur < a.nsegs;
    const DevSeg& sg = a.segs[have ? cur : 0];
    const int64_t st = sg.start, n = sg.numel;
    seg_start = have ? st : INT64_MAX;
    seg_end = have ? st + n : INT64_MAX;
    seg_stage = a.p.stage_bias + sg.ptr;
    const ProjMtVecEntry& e = a.pv[have ? cur : 0];
    seg_out = e.ptr;
    seg_dt = e.dtype;
  };
  load_seg();

  // software pipeline: block b+1's carry and old output are fetched before block b's Box-Muller.
  // The loads are unconditional: a lane off every segment loads the workspace sink, and so does
  // the old-output load of a pass that does not read the output (beta == 0: the output is never
  // read).  The old output is two 16-bit loads per element whatever its dtype -- the halves of an
  // f32 element, or a 2-byte element twice -- so that no load waits under a branch on the dtype
  // (fks_project_mt_multi_kernel's fetch).
  struct Slot {
    uint64_t dst;   // where the lane's first element goes: the staging area, or FINAL the output's piece
    uint32_t meta;  // on | output dtype << 1
    float c1, c2;   // the carry
    uint32_t lo1, hi1, lo2, hi2;  // FINAL: the old output
  };
  const uint64_t sink = (uint64_t)(uintptr_t)a.sink;
  auto fetch = [&](int64_t b) -> Slot {
    Slot sl;
    const int64_t s1 = (int64_t)kMtN * b + j1;
    while (s1 >= seg_end) { cur++; load_seg(); }
    const bool on = lane_on && s1 >= seg_start;
    const uint64_t e = on ? (uint64_t)(s1 - seg_start) : 0u;
    const uint32_t dt = on ? (uint32_t)seg_dt : (uint32_t)FKS_F32;
    const bool wide = dt == (uint32_t)FKS_F32;
    const uint64_t stage = seg_stage + 4u * e, out = seg_out + (e << (wide ? 2 : 1));
    sl.meta = (uint32_t)on | (dt << 1);
    sl.dst = FINAL ? out : stage;
    sl.c1 = sl.c2 = 0.0f;
    if constexpr (CARRY) {
      const uint64_t ca = on ? stage : sink;
      sl.c1 = *reinterpret_cast<emt_cgf32*>(ca);
      sl.c2 = *reinterpret_cast<emt_cgf32*>(ca + 32u);
    }
    sl.lo1 = sl.hi1 = sl.lo2 = sl.hi2 = 0u;
    if constexpr (FINAL) {
      const bool rd = on && a.p.read_old != 0;
      const bool w2 = rd ? wide : true;
      const uint64_t p1 = rd ? out : sink, p2 = p1 + (w2 ? 32u : 16u), half = w2 ? 2u : 0u;
      sl.lo1 = *reinterpret_cast<emt_cgu16*>(p1);
      sl.hi1 = *reinterpret_cast<emt_cgu16*>(p1 + half);
      sl.lo2 = *reinterpret_cast<emt_cgu16*>(p2);
      sl.hi2 = *reinterpret_cast<emt_cgu16*>(p2 + half);
    }
    return sl;
  };
  auto widen = [](uint32_t lo, uint32_t hi, uint32_t dt) -> float {  // exact, by selects
    const float hf = (float)__builtin_bit_cast(_Float16, (uint16_t)lo);
    const float w = __uint_as_float(dt == (uint32_t)FKS_F32 ? (lo | (hi << 16)) : (lo << 16));
    return dt == (uint32_t)FKS_F16 ? hf : w;
  };

  Slot nxt = fetch(b0);
  for (int64_t b = b0; b < b1; b++) {
    __syncthreads();          // every wave is done reading block b-1's words
    twist_all(plan, nseeds);  // the raw words of stream block b
    __syncthreads();          // every window holds block b
    const Slot sa = nxt;
    nxt = fetch(b + 1 < b1 ? b + 1 : b);  // (the last block re-reads itself, unused)
    float acc1 = sa.c1, acc2 = sa.c2;
    auto seed = [&](int k) {
      const uint64_t w = lds_u64(st_off + k * kWinBytes);  // (word j1, word j1+8), permuted window
      const f32x2_t z = z_pair2<DT>(lds, (uint32_t)w, (uint32_t)(w >> 32));
      acc1 = __fmaf_rn(a.p.g[k], z.x, acc1);  // fks_delta_accumulate's fma (apply_pair<DT, kModeDelta>)
      acc2 = __fmaf_rn(a.p.g[k], z.y, acc2);
    };
    if constexpr (DT == FKS_BF16) {
      // unrolled with wave-uniform guards, the coefficients scalar operands out of the arguments.
      // Two sums per lane leave the scheduler free to draw every seed's z before the first fma,
      // which spills: a full pass draws its seeds kEmtSeedsInFlight at a time
#pragma unroll
      for (int k = 0; k < kMaxSeedsPerPass; k++) {
        if (FULL || k < nseeds) seed(k);
        if (FULL && k % kEmtSeedsInFlight == kEmtSeedsInFlight - 1) __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      // the f32 Box-Muller is some hundred instructions a seed: unrolled over a full pass it
      // spills under the 128 VGPRs of three workgroups per CU (12 to 48 bytes per lane already
      // at a factor of 2), so the seed loop stays a loop
#pragma unroll 1
      for (int k = 0; k < nseeds; k++) seed(k);
    }
    if (sa.meta & 1u) {  // a lane off every segment stores nothing
      if constexpr (FINAL) {
        const uint32_t dt = (sa.meta >> 1) & 3u;
        if (a.p.read_old) {
          acc1 = __fmaf_rn(a.p.beta, widen(sa.lo1, sa.hi1, dt), acc1);
          acc2 = __fmaf_rn(a.p.beta, widen(sa.lo2, sa.hi2, dt), acc2);
        }
        if (dt == (uint32_t)FKS_F32) {
          *reinterpret_cast<emt_gf32*>(sa.dst) = acc1;
          *reinterpret_cast<emt_gf32*>(sa.dst + 32u) = acc2;
        } else {
          const bool bf = dt == (uint32_t)FKS_BF16;
          *reinterpret_cast<emt_gu16*>(sa.dst) = (uint16_t)emt_bits16(acc1, bf);
          *reinterpret_cast<emt_gu16*>(sa.dst + 16u) = (uint16_t)emt_bits16(acc2, bf);
        }
      } else {
        *reinterpret_cast<emt_gf32*>(sa.dst) = acc1;
        *reinterpret_cast<emt_gf32*>(sa.dst + 32u) = acc2;
      }
    }
  }
}

// ------------------------------------------------------------------ irregular work
// element e of the output's piece E, staged at `stage`: the carry in ...
__device__ __forceinline__ float emt_carry(const ExpMtPass& p, uint64_t stage) {
  return p.carry_in ? *reinterpret_cast<emt_cgf32*>(stage) : 0.0f;
}
// ... and the sum out: to the staging area, or through beta and the cast to the output
__device__ __forceinline__ void emt_finish(const ExpMtPass& p, uint64_t stage, const ProjMtVecEntry& E, int64_t e,
                                           float acc) {
  if (p.to_stage) {
    *reinterpret_cast<emt_gf32*>(stage) = acc;
  } else if (E.dtype == FKS_F32) {
    emt_gf32* o = reinterpret_cast<emt_gf32*>(E.ptr + (uint64_t)e * 4u);
    if (p.read_old) acc = __fmaf_rn(p.beta, *o, acc);
    *o = acc;
  } else {
    const bool bf = E.dtype == FKS_BF16;
    emt_gu16* o = reinterpret_cast<emt_gu16*>(E.ptr + (uint64_t)e * 2u);
    if (p.read_old) acc = __fmaf_rn(p.beta, emt_widen16(*o, bf), acc);
    *o = (uint16_t)emt_bits16(acc, bf);
  }
}

template <int DT>
__device__ __forceinline__ void emt_run_chain(const uint8_t* lds, const uint32_t* win, const ExpMtPass& p, int w1,
                                              float& acc1, float& acc2) {
  for (int k = 0; k < p.nseeds; k++) {
    float z1, z2;
    irr_z_pair<DT>(lds, win_word(win, k, w1), win_word(win, k, w1 + 8), z1, z2);
    acc1 = __fmaf_rn(p.g[k], z1, acc1);  // apply_one<DT>(.., kModeDelta, ..)
    acc2 = __fmaf_rn(p.g[k], z2, acc2);
  }
}

// The store visitor: a lane with work runs every seed of the pass over its own elements in
// registers and stores them once; a lane without work does nothing.
struct EmtIrrExpand {
  const ExpMtIrrArgs& a;
  int rcur;  // no run before this one starts at or after the last run visited
  __device__ __forceinline__ void run(const uint8_t* lds, const uint32_t* win, const DevRun& R, bool mine, int64_t e1,
                                      int w1) {
    // the walk hands over a copy of the run: its index is found by its start (the runs are
    // disjoint, sorted by start, and visited in that order), as PmtIrrProjectMulti does
    int lo = rcur, hi = a.nruns;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (a.runs[mid].start < R.start) lo = mid + 1; else hi = mid;
    }
    rcur = lo;
    if (mine && lo < a.nruns) {
      const ProjMtVecEntry E = a.rv[lo];
      // elements at or past the limit are another run's: neither read nor written
      const bool on1 = e1 < R.limit, on2 = e1 + 8 < R.limit;
      const uint64_t s1 = a.p.stage_bias + R.ptr + (uint64_t)e1 * 4u, s2 = s1 + 32u;
      float acc1 = on1 ? emt_carry(a.p, s1) : 0.0f, acc2 = on2 ? emt_carry(a.p, s2) : 0.0f;
      switch (R.dtype) {
        case FKS_F32:
          if (a.libm) emt_run_chain<kDtF32Libm>(lds, win, a.p, w1, acc1, acc2);
          else emt_run_chain<FKS_F32>(lds, win, a.p, w1, acc1, acc2);
          break;
        case FKS_BF16: emt_run_chain<FKS_BF16>(lds, win, a.p, w1, acc1, acc2); break;
        default: emt_run_chain<FKS_F16>(lds, win, a.p, w1, acc1, acc2); break;
      }
      if (on1) emt_finish(a.p, s1, E, e1, acc1);
      if (on2) emt_finish(a.p, s2, E, e1 + 8, acc2);
    }
  }
  __device__ __forceinline__ void tiny(const uint8_t*, const uint32_t* win, bool mine, int idx, int64_t base) {
    if (mine) {
      const DevTiny T = a.tiny[idx];
      const ProjMtVecEntry E = a.tv[idx];
      const int w = (int)(T.word - base);
      const bool sin_half = (T.flags & kTinySin) != 0;
      const uint64_t s = a.p.stage_bias + T.ptr;
      float acc = emt_carry(a.p, s);
      for (int k = 0; k < a.p.nseeds; k++) {
        const float zf = irr_tiny_z(win, k, w, sin_half);  // static_cast<scalar_t>(double) via float
        const float zb = rbf(zf), zh = rhf(zf);
        const float z = T.dtype == FKS_F32 ? zf : (T.dtype == FKS_BF16 ? zb : zh);
        acc = __fmaf_rn(a.p.g[k], z, acc);
      }
      emt_finish(a.p, s, E, 0, acc);
    }
  }
};

__global__ __launch_bounds__(kApplyThreads) void fks_expand_mt_irr_kernel(ExpMtIrrArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds32[];
  EmtIrrExpand vis{a, 0};
  irr_walk(lds32, a, vis);
}

// ------------------------------------------------------------------ host side
template <int DT, bool FULL, bool CARRY, bool FINAL>
int emt_launch(const ExpMtArgs& a, void* stream) {
  // a partial pass allocates only its own windows (+1 spare: the twist's last-phase lanes and
  // the idle lanes read past a window)
  const size_t full = (size_t)kLdsTabBytes + (size_t)kLdsStBytes;
  const size_t lds = FULL ? full : (size_t)kLdsTabBytes + (size_t)(a.p.nseeds + 1) * kWinBytes;
  static PerDevice attr;
  if (int e = ensure_lds_attr(attr, &fks_expand_mt_kernel<DT, FULL, CARRY, FINAL>, (int)full)) return e;
  hipLaunchKernelGGL((fks_expand_mt_kernel<DT, FULL, CARRY, FINAL>), dim3((unsigned)a.nchunks), dim3(kApplyThreads),
                     lds, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

// the six instances of a dtype: a pass that stages is a full one
template <int DT>
int emt_launch_t(const ExpMtArgs& a, void* stream) {
  const bool full = a.p.nseeds == kMaxSeedsPerPass, carry = a.p.carry_in != 0;
  if (a.p.to_stage) {
    if (!full) return -FKS_EINVAL;
    return carry ? emt_launch<DT, true, true, false>(a, stream) : emt_launch<DT, true, false, false>(a, stream);
  }
  if (carry) return full ? emt_launch<DT, true, true, true>(a, stream) : emt_launch<DT, false, true, true>(a, stream);
  return full ? emt_launch<DT, true, false, true>(a, stream) : emt_launch<DT, false, false, true>(a, stream);
}

}  // namespace

int launch_expand_mt(int dtype, const ExpMtArgs& a, void* stream) {
  if (a.p.nseeds < 0 || a.p.nseeds > kMaxSeedsPerPass || a.nchunks < 1 || a.nsegs < 1 || !a.sink || !a.pv || !a.segs ||
      !a.chunk_block || (a.p.nseeds > 0 && !a.states))
    return -FKS_EINVAL;
  if (dtype == FKS_BF16) {
    if (int e = ensure_tables()) return e;
    return emt_launch_t<FKS_BF16>(a, stream);
  }
  if (dtype == FKS_F32) return emt_launch_t<FKS_F32>(a, stream);
  if (dtype == kDtF32Libm) return emt_launch_t<kDtF32Libm>(a, stream);
  return -FKS_ENOTSUP;  // f16 tensors have no fast segments
}

int launch_expand_mt_irr(const ExpMtIrrArgs& a, void* stream) {
  if (a.p.nseeds < 0 || a.p.nseeds > kMaxSeedsPerPass || a.nseeds != a.p.nseeds || a.nchunks < 1 ||
      (a.nruns > 0 && (!a.runs || !a.rv)) || (a.ntiny > 0 && (!a.tiny || !a.tv)) || (a.p.nseeds > 0 && !a.states))
    return -FKS_EINVAL;
  if (int e = ensure_tables()) return e;
  const size_t lds = (size_t)kIrrLogfOff + kLdsLogfBytes;  // tables | windows | wave counters | logf table
  static PerDevice attr;
  if (int e = ensure_lds_attr(attr, &fks_expand_mt_irr_kernel, (int)lds)) return e;
  hipLaunchKernelGGL(fks_expand_mt_irr_kernel, dim3((unsigned)a.nchunks), dim3(kApplyThreads), lds,
                     (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // namespace fks
