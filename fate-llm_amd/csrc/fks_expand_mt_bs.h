// fks_expand_mt_bs.h -- the bit-sliced seed-basis expansion on the CPU generator's MT19937 stream
// (include/fks.h fks_expand_mt_bs): the constants and launch arguments fks_expand_mt_bs.hip (the
// kernel), fks_run_basis.cpp (the driver) and the planning share.  A header of its own for
// fks_expand_mt.h's reason: fks_device.hip does not include it, so its object -- and
// fks_build_id() -- do not move with it.
#pragma once

#include "fks_internal.h"
#include "fks_expand_mt.h"

namespace fks {

// Waves per half of fks_expand_mt_bs_kernel.  A lane keeps two f32 sums and two prefetch slots
// beside the twist's registers: the full-pass instances take 147 to 162 VGPRs, which fits four and
// six waves per half (two and three per SIMD: 256 and 168 VGPRs) and spills at eight (128 VGPRs:
// 88 to 144 bytes of scratch per lane).  Measured, four is the faster of the two that fit (780.9 ms
// against 792.7 at K = 256 on the 7B layout; DESIGN.md 4.2 has the compiler's table and the log).
#ifndef FKS_EMBS_WAVES
#define FKS_EMBS_WAVES 4
#endif
constexpr int kEmbsWaves = FKS_EMBS_WAVES;
static_assert(kEmbsWaves >= 1 && kEmbsWaves <= 8, "four waves per SIMD at most: 1024 threads per workgroup");
constexpr int kEmbsThreads = 2 * 64 * kEmbsWaves;

// One pass of at most kBsSeeds seeds over the bf16 fast segments of the geometry-only plan
// (kProjMtGeoBase), ONE output, on the slice kernel's chunk table (HdrLayout::off_bs_cb), every
// chunk start jumped (stride 1): states is [nseeds][nchunks][624].  Workgroup w runs every seed of
// the pass on plan chunk 2 w + h in half h.  The passes of a call chain through the f32 staging
// area exactly as ExpMtPass documents it (the same addresses: the two kernels' passes share one
// area): the first carries +0 in, every pass but the last is a full one and leaves its sums there,
// the last goes through beta and the cast into the output's piece pv[j] under segment j.
struct ExpMtBsArgs {
  float g[kBsSeeds];            // f32(coefs[m * k + s]) of the pass's seeds
  const uint32_t* states;
  const DevSeg* segs;           // bf16 fast segments, sorted by start; ptr as in fks_expand_mt.h
  const int64_t* chunk_block;   // [nchunks + 1] first MT block of each plan chunk
  const uint64_t* sink;         // 4 KB of workspace: what a lane off every segment loads (never stored to)
  const ProjMtVecEntry* pv;     // [nsegs]
  uint64_t stage_bias;          // ExpMtPass::stage_bias
  float beta;                   // f32(betas[m])
  int32_t nseeds;               // 1 .. kBsSeeds
  int32_t carry_in;             // the sums start from the staging area, else from +0
  int32_t to_stage;             // the sums go to the staging area (a full pass), else to the output
  int32_t read_old;             // betas[m] != 0: the output is read and scaled; 0: never read
  int32_t nsegs;
  int32_t nchunks;              // plan chunks: even
  int32_t pad;
};
int launch_expand_mt_bs(const ExpMtBsArgs& a, void* stream);

}  // namespace fks
