// fks_run.h -- what the launch drivers share: fks_run.cpp (the codec's calls) and fks_run_basis.cpp
// (the seed-basis calls).  Host only, and only for files that call the HIP runtime.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "fks_host.h"

namespace fks {

// launch-time instrumentation (fks_profile_begin/end): events around every launch
struct Prof {
  bool on = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[2];  // 0 = apply, 1 = jump
};
extern Prof g_prof;  // fks_run.cpp
extern std::mutex g_prof_mu;

template <class F>
int timed(int which, void* stream, F&& launch) {
  std::unique_lock<std::mutex> lk(g_prof_mu);
  if (!g_prof.on) {
    lk.unlock();
    return launch();
  }
  hipEvent_t a, b;
  (void)hipEventCreate(&a);
  (void)hipEventCreate(&b);
  (void)hipEventRecord(a, (hipStream_t)stream);
  const int rc = launch();
  (void)hipEventRecord(b, (hipStream_t)stream);
  g_prof.ev[which].emplace_back(a, b);
  return rc;
}

// a launcher's result: 0, a hipError_t, or a negative FKS code (`neg` says what it means)
inline void check_launch(int rc, const char* what, const char* neg = "unsupported") {
  if (rc) throw Error(rc < 0 ? rc : -FKS_EHIP, std::string(what) + " launch: " +
                                                 (rc > 0 ? hipGetErrorString((hipError_t)rc) : neg));
}
inline void check_hip(hipError_t e, const char* what) {
  if (e != hipSuccess) throw Error(-FKS_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

// the jump of nb seeds to the chunk starts of the header's table at off_cb (its polynomials at off_polys)
inline JumpArgs jump_args(const uint64_t* seeds, int nb, const uint8_t* hdr, size_t off_polys, size_t off_cb,
                          uint32_t* states, int nchunks) {
  JumpArgs ja{};
  for (int j = 0; j < nb; j++) ja.seeds[j] = seeds[j];
  ja.polys = reinterpret_cast<const uint64_t*>(hdr + off_polys);
  ja.chunk_block = reinterpret_cast<const int64_t*>(hdr + off_cb);
  ja.states = states;
  ja.nchunks = nchunks;
  return ja;
}

// Chunks per jump workgroup (one chunk per wave, 16 waves, one workgroup per CU by
// LDS): enough workgroups to cover every CU before packing chunks into fewer groups.
inline int jump_chunks_per_wg(int nseeds, int nchunks, int cus) {
  const int per_cu = (int)(((int64_t)nseeds * nchunks + cus - 1) / cus);
  return std::max(1, std::min({kJumpMaxCpw, per_cu, nchunks}));
}

// The launches every call on the CPU generator's stream makes over its plan.  The caller holds
// g_cache_mu while it uses one (no eviction of C meanwhile).
struct MtPlan {
  const CachedPlan& C;
  int cus;
  bool libm;  // fp32 z in the libm flavour (libm_flavour)
  void* stream;

  template <class T>
  const T* at(size_t off) const { return reinterpret_cast<const T*>(static_cast<const uint8_t*>(C.dev) + off); }

  // The jump of n seeds to the regular (irregular) chunk starts, seed j's windows from window j
  // of `states` on.  Nothing for n <= 0: a pass without seeds (fks_expand_mt_multi with k == 0)
  // has no windows.
  void jump_regular(const uint64_t* seeds, int n, uint32_t* states) const {
    jump(seeds, n, C.H.off_polys, C.H.off_cb, states, C.Z.reg_chunks, jump_chunks_per_wg(n, C.Z.reg_chunks, cus));
  }
  void jump_irregular(const uint64_t* seeds, int n, uint32_t* states) const {
    jump(seeds, n, C.H.off_ipolys, C.H.off_ilo, states, C.Z.irr_chunks, std::max(1, std::min(32, C.Z.irr_chunks)));
  }

  // f(d, dd, first) per dtype d with fast segments: dd the launchers' dtype (kDtF32Libm for fp32 in
  // the libm flavour), first the dtype's first segment among all the plan's fast segments
  template <class F>
  void each_fast_dtype(F&& f) const {
    size_t first = 0;
    for (int d = 0; d < 3; first += (size_t)C.nsegs[d], d++)
      if (C.nsegs[d]) f(d, (d == FKS_F32 && libm) ? kDtF32Libm : d, first);
  }
  // what every fast-segment launch of dtype d (every irregular launch) takes from the plan; the
  // args structs share these names (fks_dev_irr.h's irr_walk reads the irregular ones by name)
  template <class A>
  void fill_fast(A& a, int d, const uint32_t* states) const {
    a.states = states;
    a.segs = at<DevSeg>(C.seg_off[d]);
    a.chunk_block = at<int64_t>(C.H.off_cb);
    a.nsegs = C.nsegs[d];
    a.nchunks = C.Z.reg_chunks;
  }
  template <class A>
  void fill_irregular(A& a, const uint32_t* states) const {
    a.states = states;
    a.runs = at<DevRun>(C.H.off_runs);
    a.tiny = at<DevTiny>(C.H.off_tiny);
    a.chunk_lo = at<int64_t>(C.H.off_ilo);
    a.chunk_hi = at<int64_t>(C.H.off_ihi);
    a.nruns = C.Z.nruns;
    a.ntiny = C.Z.ntiny;
    a.nchunks = C.Z.irr_chunks;
    a.libm = libm ? 1 : 0;
  }
  // partial rows one pass of a projection leaves: a row per chunk of every launch
  int partial_rows() const {
    int rows = C.have_irr ? C.Z.irr_chunks : 0;
    for (int d = 0; d < 3; d++) rows += C.nsegs[d] ? C.Z.reg_chunks : 0;
    return rows;
  }

 private:
  void jump(const uint64_t* seeds, int n, size_t off_polys, size_t off_cb, uint32_t* states, int nchunks,
            int chunks_per_wg) const {
    if (n <= 0) return;
    JumpArgs ja = jump_args(seeds, n, static_cast<const uint8_t*>(C.dev), off_polys, off_cb, states, nchunks);
    ja.chunks_per_wg = chunks_per_wg;
    check_launch(timed(1, stream, [&] { return launch_jump(ja, n, stream); }), "fks_jump_kernel");
  }
};

}  // namespace fks
