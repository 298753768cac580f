// fks_dev_mt.h -- MT19937 on the device: twist and tempering of single words and of word
// pairs, the permuted seed windows in LDS and their wave-local twists (TwistPlan).
#pragma once
#include <hip/hip_runtime.h>

#include "fks_internal.h"
#include "fks_dev_lds.h"

namespace fks {
namespace {

// ------------------------------------------------------------------ MT19937 pieces
__device__ __forceinline__ uint32_t mt_twist(uint32_t u, uint32_t v) {
  return (((u & 0x80000000u) | (v & 0x7fffffffu)) >> 1) ^ ((v & 1u) ? kMatrixA : 0u);
}

// v_bitop3_b32 truth tables (LOP3 convention: f(0xF0, 0xCC, 0xAA))
constexpr unsigned kXorAnd = 0x78;  // a ^ (b & c)
constexpr unsigned kXorMask = 0x28; // (a ^ b) & c
constexpr unsigned kXorNotAnd = 0xD2;  // a ^ (~b & c)

// tempering, MT19937RNGEngine.h:141-145; each "y ^= (y << s) & M" is one shift + one bitop3
__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
  y ^= (y >> 11);
  y = __builtin_amdgcn_bitop3_b32(y, y << 7, 0x9d2c5680u, kXorAnd);
  y = __builtin_amdgcn_bitop3_b32(y, y << 15, 0xefc60000u, kXorAnd);
  y ^= (y >> 18);
  return y;
}

// next raw MT word from old words u = x[i], v = x[i+1] and m = x[i+397] (or the new
// x[i-227]): m ^ (((u & UPPER) | (v & LOWER)) >> 1) ^ (v & 1 ? MATRIX_A : 0)
// (MT19937RNGEngine.h:172-175), as 5 VALU ops: bitop3 mux, shift, 1-bit sign
// extract, bitop3 "(s & A) ^ m", xor.
constexpr unsigned kMux = 0xCA;     // a ? b : c, bitwise
constexpr unsigned kAndXor = 0x6A;  // (a & b) ^ c
__device__ __forceinline__ uint32_t mt_next(uint32_t u, uint32_t v, uint32_t m) {
  const uint32_t y = __builtin_amdgcn_bitop3_b32(0x80000000u, u, v, kMux);
  const uint32_t s = (uint32_t)__builtin_amdgcn_sbfe((int)v, 0, 1);
  return __builtin_amdgcn_bitop3_b32(s, kMatrixA, m, kAndXor) ^ (y >> 1);
}

// Seed windows in LDS: window k at kLdsTabBytes + 2496 k, its words PERMUTED inside each
// 16-block so that the Box-Muller pair (j, j+8) is one aligned 8-byte word pair: one
// conflict-free ds_read_b64 per seed and lane in the pair phase.
__host__ __device__ constexpr int wperm(int i) { return (i & ~15) | ((i & 7) << 1) | ((i >> 3) & 1); }
constexpr int kWinBytes = kMtN * 4;

// In-place twist of the windows (MT19937RNGEngine.h:164-175), WAVE-LOCAL: wave w owns
// windows w, w+5, w+10, w+15.  Word i of the new block needs OLD words i, i+1 and
// i+397 (i < 227) or the NEW word i-227, so the 624 words form 3 dependency phases
// [0,227) [227,454) [454,624); word 623 pairs with the NEW word 0.  A wave reads all
// its items of a phase into registers before writing any, and a wave's LDS
// operations execute in order, so no workgroup barrier is needed inside the twist.
// Lane l handles i = lo + l + 64 j: wperm(i + 64 j) = wperm(i) + 64 j, so each phase
// needs three per-lane byte offsets (u, v, m) and immediates for j and the window.
constexpr int kWaves = kApplyThreads / 64;
constexpr int kWinPerWave = (kMaxSeedsPerPass + kWaves - 1) / kWaves;

struct TwistPlan {
  int u[3], v[3], m[3];  // byte offsets in window 0 of words i, i+1, m-index for j = 0
  int v3last;            // phase 3, j = 2: lane 41 (i = 623) pairs with the new x[0]
  int wave;
  int lane;
};

__device__ __forceinline__ void twist_plan(TwistPlan& P, int tid, int st_base) {
  P.wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  P.lane = tid & 63;
  const int lo[3] = {0, 227, 454};
#pragma unroll
  for (int ph = 0; ph < 3; ph++) {
    const int i = lo[ph] + P.lane;
    P.u[ph] = st_base + 4 * wperm(i);
    P.v[ph] = st_base + 4 * wperm(i + 1);
    P.m[ph] = st_base + 4 * wperm(ph == 0 ? i + kMtM : i - (kMtN - kMtM));
  }
  // i = 454 + 41 + 128 = 623: its next word is the new x[0]; expressed relative to j = 2
  P.v3last = P.lane == 41 ? st_base + 4 * wperm(0) - 2 * 256 : P.v[2];
}

template <int PH>
__device__ __forceinline__ void twist_phase(const TwistPlan& P, int nseeds) {
  constexpr int len = PH == 2 ? kMtN - 454 : 227;
  constexpr int nj = (len + 63) / 64;
  uint32_t nv[kWinPerWave][nj];
#pragma unroll
  for (int t = 0; t < kWinPerWave; t++) {
    const int k = P.wave + kWaves * t;
    if (k < nseeds) {  // wave-uniform
#pragma unroll
      for (int j = 0; j < nj; j++) {
        const int w = k * kWinBytes + 256 * j;
        const int vo = (PH == 2 && j == nj - 1) ? P.v3last : P.v[PH];
        nv[t][j] = mt_next(lds_u32(P.u[PH] + w), lds_u32(vo + w), lds_u32(P.m[PH] + w));
      }
    }
  }
  asm volatile("" ::: "memory");  // every read of the phase is issued before any write
#pragma unroll
  for (int t = 0; t < kWinPerWave; t++) {
    const int k = P.wave + kWaves * t;
    if (k < nseeds) {
#pragma unroll
      for (int j = 0; j < nj; j++) {
        if (j < nj - 1 || P.lane + 64 * j < len) lds_st(P.u[PH] + k * kWinBytes + 256 * j, nv[t][j]);
      }
    }
  }
  asm volatile("" ::: "memory");
}

__device__ __forceinline__ void twist_all(const TwistPlan& P, int nseeds) {
  twist_phase<0>(P, nseeds);
  twist_phase<1>(P, nseeds);
  twist_phase<2>(P, nseeds);
}

// Out-of-place twist of ONE window by its owner wave (double-buffered small-K kernel):
// old words from the window at byte offset `src`, new words to the window at `dst`
// (offsets relative to window 0 of the plan).  Phase 0 reads old words only; phases 1
// and 2 read the new words i-227 (and word 623 the new word 0) that this wave wrote in
// earlier phases -- a wave's LDS operations execute in order, so no barrier.  Nothing
// else reads `dst` or writes `src` while this runs.
template <int PH>
__device__ __forceinline__ void twist_phase_oop(const TwistPlan& P, int src, int dst) {
  constexpr int len = PH == 2 ? kMtN - 454 : 227;
  constexpr int nj = (len + 63) / 64;
  uint32_t nv[nj];
#pragma unroll
  for (int j = 0; j < nj; j++) {
    const int vo = (PH == 2 && j == nj - 1 && P.lane == 41) ? P.v3last + dst : P.v[PH] + src;
    const int mo = P.m[PH] + (PH == 0 ? src : dst);
    nv[j] = mt_next(lds_u32(P.u[PH] + src + 256 * j), lds_u32(vo + 256 * j), lds_u32(mo + 256 * j));
  }
#pragma unroll
  for (int j = 0; j < nj; j++)
    if (j < nj - 1 || P.lane + 64 * j < len) lds_st(P.u[PH] + dst + 256 * j, nv[j]);
}

__device__ __forceinline__ void twist_oop(const TwistPlan& P, int src, int dst) {
  twist_phase_oop<0>(P, src, dst);
  twist_phase_oop<1>(P, src, dst);
  twist_phase_oop<2>(P, src, dst);
}

// The same out-of-place twist with the phases chained in REGISTERS: lane l's word
// i = lo + l + 64 j of phase 1 (2) takes as m the new word i - 227, which is this lane's
// own word (l, j) of phase 0 (1); only word 623's partner, the new word 0, crosses lanes
// (lane 0's first word, broadcast with v_readlane).  So every LDS read of the window is
// issued up front, against the old words only, and there is one LDS round trip per
// window instead of three dependent ones.
__device__ __forceinline__ void twist_oop_reg(const TwistPlan& P, int src, int dst) {
  uint32_t u0[4], v0[4], m0[4], u1[4], v1[4], u2[3], v2[3];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    u0[j] = lds_u32(P.u[0] + src + 256 * j);
    v0[j] = lds_u32(P.v[0] + src + 256 * j);
    m0[j] = lds_u32(P.m[0] + src + 256 * j);
    u1[j] = lds_u32(P.u[1] + src + 256 * j);
    v1[j] = lds_u32(P.v[1] + src + 256 * j);
  }
#pragma unroll
  for (int j = 0; j < 3; j++) {
    u2[j] = lds_u32(P.u[2] + src + 256 * j);
    v2[j] = lds_u32(P.v[2] + src + 256 * j);  // lane 41, j = 2 (i = 623): replaced below
  }
  uint32_t n0[4], n1[4], n2[3];
#pragma unroll
  for (int j = 0; j < 4; j++) n0[j] = mt_next(u0[j], v0[j], m0[j]);
#pragma unroll
  for (int j = 0; j < 4; j++) n1[j] = mt_next(u1[j], v1[j], n0[j]);
  const uint32_t x0 = __builtin_amdgcn_readlane(n0[0], 0);
#pragma unroll
  for (int j = 0; j < 3; j++) n2[j] = mt_next(u2[j], (j == 2 && P.lane == 41) ? x0 : v2[j], n1[j]);
#pragma unroll
  for (int j = 0; j < 4; j++) {
    if (j < 3 || P.lane + 192 < 227) {
      lds_st(P.u[0] + dst + 256 * j, n0[j]);
      lds_st(P.u[1] + dst + 256 * j, n1[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < 3; j++)
    if (j < 2 || P.lane + 128 < kMtN - 454) lds_st(P.u[2] + dst + 256 * j, n2[j]);
}

// 64-bit shifts of a word pair held in one VGPR pair (full rate on gfx950, measured
// tools/ubench): the bits one word shifts into the other are masked off afterwards
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
template <int S>
__device__ __forceinline__ u32x2_t shr64(u32x2_t x) {
  u32x2_t r;
  asm("v_lshrrev_b64 %0, %2, %1" : "=v"(r) : "v"(x), "i"(S));
  return r;
}
template <int S>
__device__ __forceinline__ u32x2_t shl64(u32x2_t x) {
  u32x2_t r;
  asm("v_lshlrev_b64 %0, %2, %1" : "=v"(r) : "v"(x), "i"(S));
  return r;
}

// Both table byte offsets (x8) of a Box-Muller word pair y = (word j, word j+8):
// MT19937RNGEngine.h:141-145 tempering of both words, then ((y ^ (y >> 18)) & 0xFF) << 3,
// 13 VALU ops for the two words instead of 18.  y >> 11 pulls 11 bits of the high word
// into the top of the low one (mask 0x001FFFFF); y << 7 and y << 15 push the low word's
// top bits into the high word's bits 0..6 / 0..14, which the tempering masks already
// clear; the final shifts' spill lies outside 0x7F8.
__device__ __forceinline__ u32x2_t temper_pair_u8x8(u32x2_t y) {
  u32x2_t t = shr64<11>(y);
  y.x = __builtin_amdgcn_bitop3_b32(y.x, t.x, 0x001FFFFFu, kXorAnd);
  y.y ^= t.y;
  t = shl64<7>(y);
  y.x = __builtin_amdgcn_bitop3_b32(y.x, t.x, 0x9d2c5680u, kXorAnd);
  y.y = __builtin_amdgcn_bitop3_b32(y.y, t.y, 0x9d2c5680u, kXorAnd);
  // the third step y ^= (y << 15) & 0xefc60000 changes bits 17..31 only; of those the
  // index reads bits 18..25, where it adds y bits 3..10 under 0xF1 (= 0xefc60000 >> 18):
  // idx8 = ((y << 3) ^ (y >> 15) ^ (y & 0x788)) & 0x7F8 on the second step's y -- 6 ops
  // for the pair instead of 7 (checked against the four-step tempering in
  // tests/test_temper_fold.py)
  const u32x2_t t1 = shl64<3>(y), t2 = shr64<15>(y);
  u32x2_t o;
  o.x = __builtin_amdgcn_bitop3_b32(t1.x, t2.x, 0x7F8u, kXorMask);
  o.y = __builtin_amdgcn_bitop3_b32(t1.y, t2.y, 0x7F8u, kXorMask);
  o.x = __builtin_amdgcn_bitop3_b32(o.x, y.x, 0x788u, kXorAnd);
  o.y = __builtin_amdgcn_bitop3_b32(o.y, y.y, 0x788u, kXorAnd);
  return o;
}

}  // namespace
}  // namespace fks
