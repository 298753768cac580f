// fks_expand_mt.h -- seed-basis expansion on the CPU generator's stream (fks_expand_mt.hip;
// include/fks.h fks_expand_mt_multi): what the kernels, their launchers, the launch driver and the
// planning share.  A header of its own -- fks_device.hip does not read it, so the device object
// and fks_build_id() stay put.
#pragma once

#include "fks_internal.h"
#include "fks_project_mt.h"

namespace fks {

// One pass of at most kMaxSeedsPerPass seeds over the geometry-only plan (kProjMtGeoBase: a
// descriptor's ptr is kProjMtGeoBase + 4 x its first element's index in the concatenation), ONE
// output.  A call of k <= kMaxSeedsPerPass seeds is one pass, +0 in and the output out.  A longer
// call runs ceil(k / kMaxSeedsPerPass) passes through the f32 staging area: the first carries +0
// in, every pass but the last leaves its sums in the staging area, every pass but the first
// starts from them, the last writes the output.  Element e of the concatenation is staged at
// stage_bias + kProjMtGeoBase + 4 e, i.e. at stage_bias + (a descriptor's ptr) + 4 x (the
// element's index under the descriptor).
struct ExpMtPass {
  float g[kMaxSeedsPerPass];    // f32(coefs[m * k + s]) of the pass's seeds
  uint64_t stage_bias;          // (staging area) - kProjMtGeoBase - 4 x (its first element), mod 2^64
  float beta;                   // f32(betas[m])
  int32_t nseeds;               // 0 (a call without seeds) .. kMaxSeedsPerPass
  int32_t carry_in;             // the sums start from the staging area, else from +0
  int32_t to_stage;             // the sums go to the staging area, else through beta and the cast to the output
  int32_t read_old;             // betas[m] != 0: the output is read and scaled; 0: never read
  int32_t pad;
};

// the fast segments of one dtype; pv[j] is the output's piece under segs[j]
struct ExpMtArgs {
  ExpMtPass p;
  const uint32_t* states;       // [nseeds][nchunks][624] generator windows at chunk starts
  const DevSeg* segs;           // sorted by start; ptr as above
  const int64_t* chunk_block;   // [nchunks + 1] first MT block of each chunk
  const uint64_t* sink;         // 4 KB of workspace: what a lane off every segment loads (never stored to)
  const ProjMtVecEntry* pv;
  int32_t nsegs;
  int32_t nchunks;
};
// the irregular work; rv[j] / tv[j] is the output's piece under runs[j] / tiny[j]
struct ExpMtIrrArgs {
  ExpMtPass p;
  const uint32_t* states;       // [nseeds][nchunks][624]
  const DevRun* runs;           // sorted by start (disjoint)
  const DevTiny* tiny;          // sorted by word
  const int64_t* chunk_lo;      // [nchunks] chunk c twists MT blocks [chunk_lo[c], chunk_hi[c])
  const int64_t* chunk_hi;
  const ProjMtVecEntry* rv;
  const ProjMtVecEntry* tv;
  int32_t nruns;
  int32_t ntiny;
  int32_t nchunks;
  int32_t nseeds;               // p.nseeds (irr_walk reads the frame's fields by name)
  int32_t libm;                 // fp32 runs draw the libm flavour (FKS_LIBM: kDtF32Libm)
  int32_t pad;
};
int launch_expand_mt(int dtype, const ExpMtArgs& a, void* stream);  // dtype: FKS_F32, FKS_BF16 or kDtF32Libm
int launch_expand_mt_irr(const ExpMtIrrArgs& a, void* stream);

}  // namespace fks
