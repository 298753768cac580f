// fks_gram_tiled.h -- the tiled seed-basis Gram matrix on the f64 matrix unit (include/fks.h
// fks_gram_tiled; torch_rocm stream): the tile constants and launch arguments fks_gram_tiled.hip
// (the kernels) and fks_run.cpp / fks_phx.cpp (the driver, the passes) share.  A header of its own
// for fks_gram.h's reason: fks_device.hip does not include it, so its object -- and
// fks_build_id() -- do not move with it.
#pragma once

#include "fks_internal.h"

// the tile of a pass in 16-seed blocks (A/B: make variant_gram_tiled NAME=x DEFS="-DFKS_GT_R=2 -DFKS_GT_C=2";
// tools/gram_tiled_rate.py times it; DESIGN §4.2 has the table).  Columns >= rows, so that the
// diagonal tile of a symmetric call holds every cell below the diagonal of its row tile.
#ifndef FKS_GT_R
#define FKS_GT_R 4
#endif
#ifndef FKS_GT_C
#define FKS_GT_C 4
#endif
// grid cap in workgroups per CU: the kernel's own residency (a workgroup is one wave per SIMD, and
// the accumulators of a 4 x 4 tile alone are 128 registers per lane), not FKS_PROJ_WG_PER_CU
#ifndef FKS_GT_WG_PER_CU
#define FKS_GT_WG_PER_CU 1
#endif

namespace fks {

constexpr int kGtSeeds = 16;                  // seeds of a block: the M and N of v_mfma_f64_16x16x4_f64
constexpr int kGtR = FKS_GT_R, kGtC = FKS_GT_C;
constexpr int kGtRows = kGtSeeds * kGtR;      // row seeds of a pass
constexpr int kGtCols = kGtSeeds * kGtC;      // column seeds of a pass
constexpr int kGtTile = kGtRows * kGtCols;    // doubles of a workgroup's partial
constexpr int kGtThreads = 256;
constexpr int kGtWaves = kGtThreads / 64;
constexpr int kGtChunk = 256;                 // work items a wave takes at a time: 64 MFMA steps of 4 items
constexpr int kGtWgPerCu = FKS_GT_WG_PER_CU;
static_assert(kGtR >= 1 && kGtC >= kGtR && kGtR * kGtC <= 32, "tile: columns >= rows, at most 256 accumulator registers");

// One pass: the 16 kGtR row seeds against the 16 kGtC column seeds over the items [item_lo, item_hi)
// of the geometry-only table.  Seeds past the pass's counts are padding (any value: drawn where
// their block is live, never written out); nrb x ncb blocks are live.  diag: column block b holds
// row block b's seeds for every b < min(nrb, ncb), so its operand is the row block's.  Block b
// leaves partial[b][kGtTile] in the accumulators' own order ([row block][column block][register]
// [lane]); launch_gram_tiled_reduce adds the blocks in a fixed order into out[(row0 + m) * ld +
// col0 + n], m < nrows, n < ncols, and (mirror) into the transposed element too.
struct GramTiledArgs {
  uint64_t rseeds[kGtRows];
  uint64_t cseeds[kGtCols];
  const PhxTensor* t;   // sorted by item0
  double* partial;      // [gram_tiled_grid(item_hi - item_lo)][kGtTile]
  int64_t item_lo;
  int64_t item_hi;
  int32_t nt;
  int32_t nrb;          // live row blocks, 1 .. kGtR
  int32_t ncb;          // live column blocks, 1 .. kGtC
  int32_t diag;
};
// workgroups of a launch over `items` work items on the current device: a function of the device
// and the item count alone
int gram_tiled_grid(int64_t items);
int launch_gram_tiled(const GramTiledArgs& a, void* stream);
int launch_gram_tiled_reduce(const double* partial, int nblocks, int nrows, int ncols, double* out, int64_t ld,
                             int row0, int col0, bool mirror, void* stream);

}  // namespace fks
