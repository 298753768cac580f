// fks_gram_mt.h -- the seed-basis Gram matrix on the CPU generator's MT19937 stream
// (include/fks.h fks_gram_mt): what fks_gram_mt.hip (the kernels), the launch driver and the
// planning share of it.  A header of its own, as fks_project_mt.h and fks_gram.h are: neither
// fks_internal.h nor fks_device.hip includes it, so the hot kernels' object -- and
// fks_build_id() -- do not move with it.
#pragma once

#include "fks_internal.h"
#include "fks_gram.h"

namespace fks {

// A pass carries FKS_GMT_ROWS row seeds and FKS_GMT_COLS column seeds, each with its own window
// in LDS, and a lane keeps one f64 sum (two VGPRs) per cell under the 128 VGPRs three workgroups
// per CU leave a wave.  The order of one cell's additions does not depend on the seeds that
// share its pass, so no bit depends on the tile.  Kept: 4 x 5 (DESIGN.md 4.2 has the resource
// usage of the candidates; every instance is free of scratch).
//   * rows + cols <= kMaxSeedsPerPass: the windows of a pass share the LDS of a 19-seed pass;
//   * rows x cols <= 64: in the irregular kernel lane m * cols + k of a wave keeps cell (m, k);
//   * rows <= kGramRows, cols <= kPhxSeeds: a chunk leaves partial[kGramRows][kPhxSeeds], the
//     rows launch_gram_reduce (fks_project.hip) adds;
//   * cols >= rows: a symmetric call's diagonal pass holds every cell below the diagonal of its
//     row tile.
#ifndef FKS_GMT_ROWS
#define FKS_GMT_ROWS 4
#endif
#ifndef FKS_GMT_COLS
#define FKS_GMT_COLS 5
#endif
constexpr int kGramMtRows = FKS_GMT_ROWS;
constexpr int kGramMtCols = FKS_GMT_COLS;
static_assert(kGramMtRows >= 1 && kGramMtCols >= kGramMtRows, "a diagonal tile holds its row tile's lower cells");
static_assert(kGramMtRows + kGramMtCols <= kMaxSeedsPerPass, "the windows of a pass fit the LDS of a 19-seed pass");
static_assert(kGramMtRows * kGramMtCols <= 64, "one lane of a wave per cell in the irregular kernel");
static_assert(kGramMtRows <= kGramRows && kGramMtCols <= kPhxSeeds, "launch_gram_reduce's partial rows");

// One pass over the geometry-only plan (fks_project_mt.h kProjMtGeoBase; no pointer of a
// descriptor is read).  `states` holds the windows of the pass at the chunk starts, the row
// seeds' first and the column seeds' behind them: [nrows + ncols][nchunks][624].  The workgroup
// of chunk c leaves partial[c][kGramRows][kPhxSeeds] (cell (m, k) at [m][k]).
struct GramMtArgs {
  const uint32_t* states;
  const DevSeg* segs;           // fast segments of this launch's dtype, sorted by start
  const int64_t* chunk_block;   // [nchunks + 1] first MT block of each chunk
  double* partial;
  int32_t nsegs;
  int32_t nchunks;
  int32_t nrows;
  int32_t ncols;
};
struct GramMtIrrArgs {          // (irr_walk reads states .. libm by these names)
  const uint32_t* states;
  const DevRun* runs;           // sorted by start (disjoint)
  const DevTiny* tiny;          // sorted by word
  const int64_t* chunk_lo;      // [nchunks] chunk c twists MT blocks [chunk_lo[c], chunk_hi[c])
  const int64_t* chunk_hi;
  double* partial;
  int32_t nruns;
  int32_t ntiny;
  int32_t nchunks;
  int32_t nseeds;               // nrows + ncols: the windows irr_walk loads and twists
  int32_t libm;                 // fp32 runs draw the libm flavour (FKS_LIBM: kDtF32Libm)
  int32_t nrows;
  int32_t ncols;
  int32_t pad;
};
int launch_gram_mt(int dtype, const GramMtArgs& a, void* stream);  // dtype as launch_project_mt
int launch_gram_mt_irr(const GramMtIrrArgs& a, void* stream);

}  // namespace fks
