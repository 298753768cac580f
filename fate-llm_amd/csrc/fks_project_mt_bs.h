// fks_project_mt_bs.h -- the bit-sliced seed-basis projection on the CPU generator's MT19937 stream
// (include/fks.h fks_project_mt_bs): the constants and launch arguments fks_project_mt_bs.hip (the
// kernels), fks_run_basis.cpp (the driver) and the planning share.  A header of its own for
// fks_project_mt.h's reason: fks_device.hip does not include it, so its object -- and
// fks_build_id() -- do not move with it.
#pragma once

#include "fks_internal.h"
#include "fks_project_mt.h"

namespace fks {

// Waves per half of fks_project_mt_bs_kernel.  The twist peaks near 120 VGPRs and a lane keeps 32
// f64 sums (64 VGPRs) across the tasks of a chunk: two waves per SIMD (256 VGPRs each), eight per
// workgroup, four per half.  Three per SIMD (168 VGPRs) would spill.
#ifndef FKS_PMBS_WAVES
#define FKS_PMBS_WAVES 4
#endif
constexpr int kPmbsWaves = FKS_PMBS_WAVES;
static_assert(kPmbsWaves >= 1 && kPmbsWaves <= 4, "two waves per SIMD at most: 256 VGPRs each");
constexpr int kPmbsThreads = 2 * 64 * kPmbsWaves;
// seeds of the 19-seed launches' sub-passes under one bit-sliced pass of kBsPassSeeds
constexpr int kPmbsSubs = (kBsPassSeeds + kMaxSeedsPerPass - 1) / kMaxSeedsPerPass;

// One pass of at most kBsPassSeeds seeds over the bf16 fast segments of the geometry-only plan
// (kProjMtGeoBase), on the slice kernel's chunk table (HdrLayout::off_bs_cb), every chunk start
// jumped (stride 1): states is [nseeds][nchunks][624].  split (nseeds <= 32): workgroup w runs
// every seed on plan chunk 2 w + h in half h; otherwise workgroup w runs plan chunk w, seeds
// [0, 32) in half 0 and [32, nseeds) in half 1.  Either way the half that ran seed s on chunk c
// leaves partial[c][s], s the seed's index in the pass, and that value does not depend on which
// form ran it.  pv[j] is the vector's piece under segment j.
struct ProjMtBsArgs {
  const uint32_t* states;
  const DevSeg* segs;           // bf16 fast segments, sorted by start
  const int64_t* chunk_block;   // [nchunks + 1] first MT block of each plan chunk
  const uint64_t* sink;         // 4 KB of workspace: what lanes off every segment load (never summed)
  double* partial;              // [nchunks][kBsPassSeeds]
  const ProjMtVecEntry* pv;     // [nsegs]
  int32_t nsegs;
  int32_t nchunks;              // plan chunks: even
  int32_t nseeds;               // 1 .. kBsPassSeeds
  int32_t split;
};
int launch_project_mt_bs(const ProjMtBsArgs& a, void* stream);

// The reduce of one pass: out[s], s < nseeds, is the sum of bs[c][s], c < nbs (the bit-sliced
// launch's chunks), then of sub[s / kMaxSeedsPerPass][r][s % kMaxSeedsPerPass], r < nrows (the rows
// of the 19-seed launches of the seed's sub-pass, [nrows][kPhxSeeds] each, sub_stride doubles
// apart) -- 64 interleaved runs of that sequence, then the runs in order.  Overwrites out.
int launch_project_mt_bs_reduce(const double* bs, int nbs, const double* sub, int nrows, int64_t sub_stride,
                                int nseeds, double* out, void* stream);

}  // namespace fks
