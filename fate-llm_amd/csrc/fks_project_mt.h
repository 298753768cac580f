// fks_project_mt.h -- the several-vector, read-in-place form of the seed-basis projection on the
// CPU generator's stream (include/fks.h fks_project_mt_multi): what fks_project_mt.hip, the launch
// driver and the planning share of it.  A header of its own, so that fks_internal.h -- which the
// hot kernels' unit includes -- does not move with it.
#pragma once

#include "fks_internal.h"

namespace fks {

// Vectors that share one pass of the generator, and the seeds such a pass carries: a lane keeps
// two VGPRs of f64 sum per (vector, seed), under the 128 VGPRs three workgroups per CU leave a
// wave.  The order of one seed's additions does not depend on the seeds that share its pass, so
// a several-vector pass may carry fewer seeds than fks_project_mt's 19 and return the same bits.
// Kept: two vectors, 10 seeds (19 seeds of two bf16 vectors on the 7B layout in
// 0.826 of two fks_project_mt calls; 12 seeds per pass: 0.861).  Three and four vectors stay
// behind FKS_PMT_MAX_VEC: at 6 and 4 seeds per pass their full-pass instances still spill to
// scratch (32 to 76 bytes per lane), which no instance of the library may.
#ifndef FKS_PMT_MAX_VEC
#define FKS_PMT_MAX_VEC 2
#endif
#ifndef FKS_PMT_SEEDS2
#define FKS_PMT_SEEDS2 10
#endif
#ifndef FKS_PMT_SEEDS3
#define FKS_PMT_SEEDS3 6
#endif
#ifndef FKS_PMT_SEEDS4
#define FKS_PMT_SEEDS4 4
#endif
constexpr int kProjMtMaxVec = FKS_PMT_MAX_VEC;
static_assert(kProjMtMaxVec >= 1 && kProjMtMaxVec <= 4 && kProjMtMaxVec <= kProjMaxVec, "vectors per pass");
constexpr int proj_mt_pass_seeds(int nv) {
  return nv <= 1 ? kMaxSeedsPerPass : (nv == 2 ? FKS_PMT_SEEDS2 : (nv == 3 ? FKS_PMT_SEEDS3 : FKS_PMT_SEEDS4));
}

// One vector's piece under one descriptor of the geometry-only plan (a fast segment, a run or a
// single element): where the descriptor's element 0 lies in the vector, and the vector's dtype.
struct ProjMtVecEntry {
  uint64_t ptr;    // device address, aligned to the element size
  int32_t dtype;   // FKS_F32 / FKS_BF16 / FKS_F16, the vector's own
  uint32_t pad;
};
static_assert(sizeof(ProjMtVecEntry) == 16, "ProjMtVecEntry layout");

// The geometry-only plan is the kModeDelta plan of this base: its descriptors' pointers are not
// read by the in-place kernels, (ptr - base) / 4 is the element's index in the concatenation.
constexpr uint64_t kProjMtGeoBase = 256;

// ProjMtArgs / ProjMtIrrArgs with the per-call table: row m of `pv` (`rv`, `tv`), `stride`
// entries long, holds vector m's pieces under the launch's segments (runs, single elements) in
// their order.  The workgroup of chunk c leaves partial[c][nvec][kPhxSeeds].
struct ProjMtMultiArgs {
  const uint32_t* states;
  const DevSeg* segs;
  const int64_t* chunk_block;
  const uint64_t* sink;
  double* partial;
  const ProjMtVecEntry* pv;
  int64_t stride;
  int32_t nsegs;
  int32_t nchunks;
  int32_t nseeds;
  int32_t nvec;
};
struct ProjMtIrrMultiArgs {
  const uint32_t* states;
  const DevRun* runs;
  const DevTiny* tiny;
  const int64_t* chunk_lo;
  const int64_t* chunk_hi;
  double* partial;
  const ProjMtVecEntry* rv;
  const ProjMtVecEntry* tv;
  int64_t stride;
  int32_t nruns;
  int32_t ntiny;
  int32_t nchunks;
  int32_t nseeds;
  int32_t libm;
  int32_t nvec;
};
int launch_project_mt_multi(int dtype, const ProjMtMultiArgs& a, void* stream);  // dtype as launch_project_mt
int launch_project_mt_irr_multi(const ProjMtIrrMultiArgs& a, void* stream);

}  // namespace fks
