// fks_dev_irr.h -- the irregular MT-stream frame: everything the fast kernels do not take
// (DESIGN.md "Irregular layouts"), walked once for any consumer:
//   * runs of whole 16-blocks at any stream phase (a tensor after a ragged one, a
//     ragged tensor's head with its overwritten elements masked, its 16-word tail
//     recompute, f16 tensors, parameters not 2-element aligned), and
//   * single elements of numel < 16 tensors (serial normal_distribution<double>,
//     DistributionsHelper.h:189-221, with the cached second sample).
// A work item is handled in the MT block holding its LAST word; its first words may
// lie up to 15 words back, in the previous block, so every seed window carries the
// previous block's last 16 raw words in front of it: [carry 16 | 624].
// fks_irregular_kernel (fks_kern_irregular.h) visits the work to update it,
// fks_project_mt_irr_kernel (fks_project_mt.hip) to project on it: irr_walk is the one text
// of the frame, so the two stay adjoint.
#pragma once
#include <hip/hip_runtime.h>

#include "fks_internal.h"
#include "fks_libm.h"
#include "fks_dev_lds.h"
#include "fks_dev_mt.h"
#include "fks_dev_zgen.h"

namespace fks {
namespace {

__constant__ float c_tab_f16[3 * 2048];  // R | C | S of the 11-bit f16 uniforms

constexpr int kIrrCarry = 16;
constexpr int kIrrWin = kIrrCarry + kMtN;  // words per seed window

__device__ __forceinline__ uint32_t win_word(const uint32_t* win, int k, int w) {  // w in [-16, 624)
  return win[k * kIrrWin + kIrrCarry + w];
}

// in-place twist of every window, phase PH of 3 (i in [0,227) / [227,454) / [454,624));
// phase 0 also saves the old words 608..623 as the next block's carry
template <int PH>
__device__ __forceinline__ void irr_twist_phase(uint32_t* win, int nseeds, int tid) {
  constexpr int lo = PH == 0 ? 0 : (PH == 1 ? 227 : 454);
  constexpr int hi = PH == 0 ? 227 : (PH == 1 ? 454 : kMtN);
  constexpr int len = hi - lo;
  constexpr int per = (kMaxSeedsPerPass * len + kApplyThreads - 1) / kApplyThreads;
  uint32_t v[per];
#pragma unroll
  for (int j = 0; j < per; j++) {
    const int idx = tid + j * kApplyThreads;
    if (idx < nseeds * len) {
      const int k = idx / len, i = lo + idx % len;
      const uint32_t* w = win + k * kIrrWin + kIrrCarry;
      const uint32_t nx = i == kMtN - 1 ? w[0] : w[i + 1];
      const uint32_t m = i < kMtN - kMtM ? w[i + kMtM] : w[i - (kMtN - kMtM)];
      v[j] = m ^ mt_twist(w[i], nx);
    }
  }
  uint32_t cv = 0;
  if (PH == 0 && tid < nseeds * kIrrCarry) cv = win[(tid / kIrrCarry) * kIrrWin + kIrrCarry + kMtN - kIrrCarry + tid % kIrrCarry];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < per; j++) {
    const int idx = tid + j * kApplyThreads;
    if (idx < nseeds * len) win[(idx / len) * kIrrWin + kIrrCarry + lo + idx % len] = v[j];
  }
  if (PH == 0 && tid < nseeds * kIrrCarry) win[(tid / kIrrCarry) * kIrrWin + tid % kIrrCarry] = cv;
  __syncthreads();
}

// z pair from two raw words, any dtype (f16 through its 11-bit tables in constant memory)
constexpr int kIrrLogfOff = kLdsTabBytes + 4 * (kIrrWin * kMaxSeedsPerPass + 16);  // after the wave counters
static_assert(kIrrLogfOff % 16 == 0, "logf table alignment");

template <int DT>
__device__ __forceinline__ void irr_z_pair(const uint8_t* lds, uint32_t r1, uint32_t r2, float& z1, float& z2) {
  if constexpr (DT == kDtF32Libm) {
    z_pair_f32_libm((uint32_t)kIrrLogfOff, r1, r2, z1, z2);
  } else if constexpr (DT == FKS_F16) {
    const uint32_t a = mt_temper(r1) & 0x7FFu, b = mt_temper(r2) & 0x7FFu;
    z1 = rhf(__fmaf_rn(c_tab_f16[a], c_tab_f16[2048 + b], 0.0f));
    z2 = rhf(__fmaf_rn(c_tab_f16[a], c_tab_f16[4096 + b], 0.0f));
  } else {
    z_pair<DT>(lds, r1, r2, z1, z2);
  }
}

__device__ __forceinline__ double u53(uint32_t hi, uint32_t lo) {  // uniform_real_distribution<double>
  const uint64_t x = (((uint64_t)hi << 32) | lo) & ((1ull << 53) - 1);
  return (double)x * (1.0 / 9007199254740992.0);
}

// The serial draw of seed k's single element whose Box-Muller pair starts at block word w,
// as static_cast<float>(double): the caller rounds it on to bf16 / f16.
__device__ __forceinline__ float irr_tiny_z(const uint32_t* win, int k, int w, bool sin_half) {
  const double u1 = u53(mt_temper(win_word(win, k, w)), mt_temper(win_word(win, k, w + 1)));
  const double u2 = u53(mt_temper(win_word(win, k, w + 2)), mt_temper(win_word(win, k, w + 3)));
  // glibc's log1p and correctly rounded sin / cos (fks_libm.h): ocml's differ from the
  // host libm by an ulp often enough to flip fp32 midpoint cases
  const double r = sqrt(-2.0 * fks_libm::log1p(-u2));
  const double theta = 2.0 * 3.14159265358979323846 * u1;
  const double v = r * fks_libm::sin_or_cos(theta, sin_half) * 1.0 + 0.0;
  return (float)v;
}

// The walk of one chunk (one workgroup of kApplyThreads; `lds32` is the kernel's dynamic LDS
// block: tables | windows | wave counters | logf table, kIrrLogfOff + kLdsLogfBytes bytes).
// Args is IrrArgs or ProjMtIrrArgs, read by their common field names.  Per MT block of the
// chunk, after the twist, every thread of the workgroup calls
//   vis.run(lds, win, R, mine, e1, w1)    once per run R with a 16-block ending in the block:
//     `mine` says that this lane owns the pair (e1, e1 + 8) of R's elements, drawn from the
//     window words (w1, w1 + 8); e1 and w1 mean nothing on a lane that is not `mine`;
//   vis.tiny(lds, win, mine, idx, base)   per batch of kApplyThreads single elements:
//     `mine` says that a.tiny[idx] is this lane's, its draw at window word tiny[idx].word - base.
// Both calls are workgroup-uniform, so a visitor may use wave-wide operations, but no barrier.
template <class Args, class V>
__device__ __forceinline__ void irr_walk(uint32_t* lds32, const Args& a, V& vis) {
  uint8_t* lds = reinterpret_cast<uint8_t*>(lds32);
  uint32_t* win = reinterpret_cast<uint32_t*>(lds + kLdsTabBytes);
  uint32_t* cnt = win + kIrrWin * kMaxSeedsPerPass;  // per-wave counters
  if ((uint32_t)(size_t)(lds_u32_t*)lds32 != 0u) __builtin_trap();  // z_pair reads the tables at LDS 0
  const int tid = threadIdx.x;
  const int c = blockIdx.x;
  const int nseeds = a.nseeds;
  const int64_t b0 = a.chunk_lo[c], b1 = a.chunk_hi[c];
  tab_bf16_fill(lds, tid, kApplyThreads);
  if (a.libm) logf_tab_fill((uint32_t)kIrrLogfOff, tid, kApplyThreads);
  for (int idx = tid; idx < nseeds * kMtN; idx += kApplyThreads) {
    const int k = idx / kMtN, i = idx - k * kMtN;
    win[k * kIrrWin + kIrrCarry + i] = a.states[((size_t)k * a.nchunks + c) * kMtN + i];
  }
  // first run whose last word is in or after block b0; first single element likewise
  int ri, ti;
  {
    int lo = 0, hi = a.nruns;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (a.runs[mid].start + a.runs[mid].numel - 1 < (int64_t)kMtN * b0) lo = mid + 1; else hi = mid;
    }
    ri = lo;
    lo = 0, hi = a.ntiny;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (a.tiny[mid].word + 3 < (int64_t)kMtN * b0) lo = mid + 1; else hi = mid;
    }
    ti = lo;
  }
  __syncthreads();
  const int m = tid >> 3, r8 = tid & 7;
  for (int64_t b = b0; b < b1; b++) {
    irr_twist_phase<0>(win, nseeds, tid);
    irr_twist_phase<1>(win, nseeds, tid);
    irr_twist_phase<2>(win, nseeds, tid);
    const int64_t base = (int64_t)kMtN * b, end = base + kMtN;
    // runs with a 16-block ending in this block (disjoint, sorted: a contiguous range)
    while (ri < a.nruns && a.runs[ri].start + 15 < end) {
      const DevRun R = a.runs[ri];
      const int ph = (int)(R.start & 15);
      const int64_t s0 = base + 16 * m + (ph ? ph - 16 : 0);  // this lane's 16-block start
      const bool mine = tid < kMtN / 2 && s0 >= R.start && s0 < R.start + R.numel;
      vis.run(lds, win, R, mine, s0 - R.start + r8, (int)(s0 - base) + r8);
      if (R.start + R.numel - 1 < end) ri++; else break;
    }
    // single elements whose draw pair ends in this block (sorted: a prefix from ti)
    for (;;) {
      const int idx = ti + tid;
      const bool mine = idx < a.ntiny && a.tiny[idx].word + 3 < end;
      vis.tiny(lds, win, mine, idx, base);
      // block-wide count of `mine` through a few dynamic-LDS words (__syncthreads_count
      // would add static LDS and move the dynamic block off address 0)
      const uint64_t bal = __ballot(mine);
      if ((tid & 63) == 0) cnt[tid >> 6] = (uint32_t)__popcll(bal);
      __syncthreads();
      int n = 0;
#pragma unroll
      for (int w = 0; w < kApplyThreads / 64; w++) n += (int)cnt[w];
      __syncthreads();
      ti += n;
      if (n < kApplyThreads) break;
    }
  }
}

}  // namespace
}  // namespace fks
