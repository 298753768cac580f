// fks_project_mt_bs_tiled.h -- the bit-sliced seed-basis projection of many vectors per draw on the
// CPU generator's MT19937 stream (include/fks.h fks_project_mt_bs_tiled): the constants and launch
// arguments fks_project_mt_bs_tiled.hip (the kernels), fks_run_basis.cpp (the driver) and the
// planning share.  A header of its own for fks_project_mt.h's reason: fks_device.hip does not
// include it, so its object -- and fks_build_id() -- do not move with it.
#pragma once

#include "fks_internal.h"
#include "fks_project_mt.h"

namespace fks {

// Waves of fks_project_mt_bs_tiled_kernel's workgroup, all on ONE bit-sliced state and one twist
// chain (fks_gram_mt_bs_kernel's frame): two waves per SIMD, eight per workgroup.
#ifndef FKS_PMBT_WAVES
#define FKS_PMBT_WAVES 8
#endif
constexpr int kPmbtWaves = FKS_PMBT_WAVES;
static_assert(kPmbtWaves >= 1 && kPmbtWaves <= 8, "two waves per SIMD at most; the staging areas fit the LDS");
constexpr int kPmbtThreads = 64 * kPmbtWaves;
// A pass is a tile of kBsSeeds seeds (two blocks of 16 rows) by kPmbtVec vectors (16 columns) on
// v_mfma_f64_16x16x4_f64; a chunk leaves kPmbtCells sums, [vector][seed].
constexpr int kPmbtVec = 16;
constexpr int kPmbtCells = kPmbtVec * kBsSeeds;
// 19-seed sub-passes of the launches that take the rest of the list under one pass of kBsSeeds
constexpr int kPmbtSubs = (kBsSeeds + kMaxSeedsPerPass - 1) / kMaxSeedsPerPass;

// One pass of at most kBsSeeds seeds by at most kPmbtVec vectors over the bf16 fast segments of the
// geometry-only plan (kProjMtGeoBase), on the slice kernel's chunk table (HdrLayout::off_bs_cb),
// every chunk start jumped (stride 1): states is [nseeds][nchunks][624].  pv[m * pv_stride + j] is
// the piece of the pass's vector m under segment j.  The workgroup of chunk c leaves
// partial[c][m][s], m < nvec, s < nseeds (the other cells are not written); a value depends on
// the chunk, the seed and the vector's values only.
struct ProjMtBsTiledArgs {
  const uint32_t* states;
  const DevSeg* segs;           // bf16 fast segments, sorted by start
  const int64_t* chunk_block;   // [nchunks + 1] first MT block of each plan chunk
  const uint64_t* sink;         // 4 KB of workspace: what lanes off every segment load (never summed)
  double* partial;              // [nchunks][kPmbtVec][kBsSeeds]
  const ProjMtVecEntry* pv;
  int64_t pv_stride;            // entries between two vectors' rows
  int32_t nsegs;
  int32_t nchunks;
  int32_t nseeds;               // 1 .. kBsSeeds
  int32_t nvec;                 // 1 .. kPmbtVec
};
int launch_project_mt_bs_tiled(const ProjMtBsTiledArgs& a, void* stream);

// The reduce of one pass: out[m * ld + s], m < nvec, s < nseeds, is the sum of bs[c][m][s],
// c < nbs (the bit-sliced launch's chunks), then of sub[m][s / kMaxSeedsPerPass][r][s %
// kMaxSeedsPerPass], r < nrows (the rows of the 19-seed launches of vector m and the seed's
// sub-pass, [nrows][kPhxSeeds] each; sub-passes sub_stride doubles apart, vectors vec_stride) -- 64
// interleaved runs of that sequence, then the runs in order.  Overwrites out.
int launch_project_mt_bs_tiled_reduce(const double* bs, int nbs, const double* sub, int nrows, int64_t sub_stride,
                                      int64_t vec_stride, int nseeds, int nvec, double* out, int64_t ld, void* stream);

}  // namespace fks
