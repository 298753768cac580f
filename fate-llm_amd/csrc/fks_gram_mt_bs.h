// fks_gram_mt_bs.h -- the bit-sliced seed-basis Gram matrix on the CPU generator's MT19937 stream
// (include/fks.h fks_gram_mt_bs): the constants and launch arguments fks_gram_mt_bs.hip (the
// kernels), fks_run_basis.cpp (the driver) and the planning share.  A header of its own for
// fks_gram_mt.h's reason: fks_device.hip does not include it, so its object -- and
// fks_build_id() -- do not move with it.
#pragma once

#include "fks_internal.h"
#include "fks_gram_mt_tiled.h"

namespace fks {

// Waves of fks_gram_mt_bs_kernel's workgroup, all on ONE bit-sliced state and one twist chain.  The
// twist peaks near 120 VGPRs, the operands of a matrix step and the 12 f64 accumulators of the
// diagonal form come after it: two waves per SIMD (256 VGPRs each), eight per workgroup.
#ifndef FKS_GMBS_WAVES
#define FKS_GMBS_WAVES 8
#endif
constexpr int kGmbsWaves = FKS_GMBS_WAVES;
static_assert(kGmbsWaves >= 1 && kGmbsWaves <= 8, "two waves per SIMD at most; the staging areas fit the LDS");
constexpr int kGmbsThreads = 64 * kGmbsWaves;
// A pass holds two blocks of kGmtTile seeds, block 0 in planes 0-15 and block 1 in planes 16-31.
// The pair form leaves one tile, block 0 x block 1; the diagonal form the tiles (0,0), (0,1), (1,1).
constexpr int kGmbsDiagTiles = 3;
constexpr int kGmbsPassSeeds = 2 * kGmtTile;
static_assert(kGmbsPassSeeds == kBsSeeds, "one 32-seed state");

// One pass over the bf16 fast segments of the geometry-only plan (kProjMtGeoBase), on the slice
// kernel's chunk table (HdrLayout::off_bs_cb), every chunk start jumped (stride 1): blk0 / blk1 are
// the windows of the two blocks' seeds, [seed][nchunks][624]; blk1 is not read when n1 == 0 (a
// diagonal pass of at most kGmtTile seeds).  The workgroup of chunk c leaves
// partial[c][tiles][kGmtCells], tiles = diag ? kGmbsDiagTiles : 1, a tile in fks_gram_mt_tiled's
// cell order (fks_gram_mt_tiled.h); the tiles (0,1) and (1,1) of a diagonal pass with n1 == 0 are
// left unwritten.  A cell's value depends on the chunk and the cell's two seeds only.
struct GramMtBsArgs {
  const uint32_t* blk0;
  const uint32_t* blk1;
  const DevSeg* segs;           // bf16 fast segments, sorted by start
  const int64_t* chunk_block;   // [nchunks + 1] first MT block of each plan chunk
  double* partial;
  int32_t nsegs;
  int32_t nchunks;
  int32_t n0;                   // seeds of block 0: 1 .. kGmtTile
  int32_t n1;                   // seeds of block 1: 0 .. kGmtTile (0: diagonal form only)
  int32_t diag;
  int32_t pad;
};
int launch_gram_mt_bs(const GramMtBsArgs& a, void* stream);

// The reduce of one 16 x 16 tile of a pass: fks_gram_mt_tiled's reduce with the bit-sliced
// launch's chunks in front.  Cell (m, n), m < nrows, n < ncols, is the sum of bs[b * bs_stride +
// cell], b < nbs, in chunk order, then of reg[b][cell], b < nreg, then of the nirr chunks of the
// irregular sub-pass that holds the cell (launch_gram_mt_tiled_reduce) -- 16 interleaved runs of
// that sequence, then the runs in order.  Written to out[(row0 + m) * ld + col0 + n] and (mirror)
// to the transposed element.
int launch_gram_mt_bs_reduce(const double* bs, int nbs, int64_t bs_stride, const double* reg, int nreg,
                             const double* irr, int nirr, int nrows, int ncols, double* out, int64_t ld, int row0,
                             int col0, bool mirror, void* stream);

}  // namespace fks
