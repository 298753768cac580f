// fks_gram.h -- the seed-basis Gram matrix on the torch_rocm stream (include/fks.h fks_gram): the
// launch arguments fks_project.hip (the kernels) and fks_run.cpp (the driver) share, and the pass
// size the planning of fks_phx.cpp tiles by.  A header of its own, not part of fks_internal.h:
// fks_device.hip does not include it, so its object -- and fks_build_id() -- do not move with it.
#pragma once

#include "fks_internal.h"

namespace fks {

// A pass of the projection whose vectors are DRAWN, not read: at most kGramRows row seeds (the 32 z
// of a group per row seed stay in registers as fks_project_multi's loaded vectors do) against at
// most kPhxSeeds column seeds, over the geometry-only table.  Block b leaves
// partial[b][kGramRows][kPhxSeeds]; launch_gram_reduce adds the blocks in block order into
// out[(row0 + m) * ld + col0 + s], m < nrows, s < ncols, and (mirror) into the transposed element too.
constexpr int kGramRows = 4;
struct GramArgs {
  uint64_t seeds[kPhxSeeds];     // the column seeds
  uint64_t rseeds[kGramRows];    // the row seeds
  const PhxTensor* t;            // sorted by item0
  double* partial;               // [project_grid(item_hi - item_lo)][kGramRows][kPhxSeeds]
  int64_t item_lo;
  int64_t item_hi;
  int32_t nt;
  int32_t nseeds;                // column seeds of the pass
  int32_t nrows;                 // row seeds of the pass
  int32_t pad;
};
int launch_gram(const GramArgs& a, void* stream);
int launch_gram_reduce(const double* partial, int nblocks, int nrows, int ncols, double* out, int64_t ld, int row0,
                       int col0, bool mirror, void* stream);

}  // namespace fks
