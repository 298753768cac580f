// fks_expand.h -- seed-basis expansion on the torch_rocm stream (fks_expand.hip; include/fks.h
// fks_expand_multi): what the kernel, its launcher and the launch driver share.  A header of its
// own -- fks_device.hip does not read it, so the device object and fks_build_id() stay put.
#pragma once

#include "fks_internal.h"

namespace fks {

// outputs that share one pass of the generator (one kernel instance per count; a larger nvec runs
// in batches).  Every instance holds its 32 accumulators per output in registers with no scratch:
// fks_expand.hip has the compiler's report.
constexpr int kExpMaxVec = 4;
// seed-elements (seeds x the elements of the launch's rows) one launch holds at most, unless it is
// a single row: the order of one 32-seed fks_delta_accumulate launch over a 7B layout
// (32 x 6.74e9 = 2^37.65).  FKS_EXPAND_WORK overrides it per call (tests, A/B).
constexpr int64_t kExpLaunchWork = (int64_t)1 << 37;

// One launch: the items [item_lo, item_hi) of the geometry-only table (whole rows), every seed of
// the call, nvec <= kExpMaxVec outputs.  ot[m * nt + e] is output m's piece for table entry e
// (ProjVecEntry: pointer, the output's own dtype, kPhxP16); seeds[s] and coef[s * nvec + m] are
// read with wave-uniform indices.
struct ExpandArgs {
  const PhxTensor* t;        // sorted by item0; its pointers are not read
  const ProjVecEntry* ot;    // [nvec][nt]
  const uint64_t* seeds;     // [nseeds]
  const float* coef;         // [nseeds][nvec]
  float beta[kExpMaxVec];    // f32(betas[m])
  int64_t item_lo;
  int64_t item_hi;
  int32_t nt;
  int32_t nseeds;            // all the seeds of the call (>= 0)
  int32_t nvec;
  uint32_t read_old;         // bit m: betas[m] != 0, output m is read and scaled; clear: never read
};
int launch_expand_multi(const ExpandArgs& a, void* stream);

}  // namespace fks
