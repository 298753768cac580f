// fks_gram_mt_tiled.h -- the tiled seed-basis Gram matrix on the CPU generator's MT19937 stream
// (include/fks.h fks_gram_mt_tiled): the tile constants and launch arguments fks_gram_mt_tiled.hip
// (the kernels), fks_run_basis.cpp (the driver) and the planning share.  A header of its own for
// fks_gram_mt.h's reason: fks_device.hip does not include it, so its object -- and
// fks_build_id() -- do not move with it.
#pragma once

#include "fks_internal.h"
#include "fks_gram_mt.h"

namespace fks {

// A pass is ONE block of 16 row seeds against ONE block of 16 column seeds: the M and N of
// v_mfma_f64_16x16x4_f64, whose 256 accumulators are 4 registers per lane.  Every seed of the
// pass has its chunk-start window in LDS (the rows' first, the columns' behind them; a diagonal
// tile has the rows' only), so the tile is bounded by the LDS, not by registers: 3 KB of tables,
// 32 + 1 windows of 2,496 B and the waves' staging areas are 128,960 B of the 160 KB.
constexpr int kGmtTile = 16;                      // seeds of a row block and of a column block
constexpr int kGmtCells = kGmtTile * kGmtTile;    // doubles of a chunk's partial, in the f64 result map's order
constexpr int kGmtWindows = 2 * kGmtTile;
// the irregular work of a tile goes through fks_gram_mt_irr_kernel in sub-passes of its own tile
constexpr int kGmtSubRows = (kGmtTile + kGramMtRows - 1) / kGramMtRows;
constexpr int kGmtSubCols = (kGmtTile + kGramMtCols - 1) / kGramMtCols;
constexpr int kGmtSubs = kGmtSubRows * kGmtSubCols;
constexpr int kGmtIrrCells = kGramRows * kPhxSeeds;  // doubles of an irregular chunk's partial (fks_gram_mt.h)

// One pass over the fast segments of one dtype (the geometry-only plan, fks_project_mt.h
// kProjMtGeoBase).  row_states / col_states hold the windows of the pass's seeds at the chunk
// starts, [seed][nchunks][624]; col_states is not read when diag is set (the column block holds
// the row block's seeds: nrows == ncols).  The workgroup of chunk c leaves partial[c][kGmtCells],
// cell (m, n) at ((m >> 2) * 64 + ((m & 3) << 4) + n): register m >> 2 of lane ((m & 3) << 4) + n.
struct GramMtTiledArgs {
  const uint32_t* row_states;
  const uint32_t* col_states;
  const DevSeg* segs;           // fast segments of this launch's dtype, sorted by start
  const int64_t* chunk_block;   // [nchunks + 1] first MT block of each chunk
  double* partial;
  int32_t nsegs;
  int32_t nchunks;
  int32_t nrows;                // 1 .. kGmtTile
  int32_t ncols;
  int32_t diag;
  int32_t pad;
};
int launch_gram_mt_tiled(int dtype, const GramMtTiledArgs& a, void* stream);  // dtype as launch_project_mt

// The reduce of one pass: cell (m, n), m < nrows, n < ncols, is the sum of reg[b][cell], b <
// nreg (the chunks' partials of the pass's fast launches, in launch order), then of the nirr
// chunks of the irregular sub-pass that holds the cell, irr[sub][c][m % rows][n % cols] with sub =
// (m / kGramMtRows) * kGmtSubCols + n / kGramMtCols -- 16 interleaved runs in that order, then
// the runs in order.  Written to out[(row0 + m) * ld + col0 + n] and (mirror) to the transposed
// element.
int launch_gram_mt_tiled_reduce(const double* reg, int nreg, const double* irr, int nirr, int nrows, int ncols,
                                double* out, int64_t ld, int row0, int col0, bool mirror, void* stream);

}  // namespace fks
