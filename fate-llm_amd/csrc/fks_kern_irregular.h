// fks_kern_irregular.h -- fks_irregular_kernel: everything the fast kernels do not take, as
// the update visitor of the irregular frame (fks_dev_irr.h).
#pragma once
#include <hip/hip_runtime.h>

#include "fks_internal.h"
#include "fks_dev_update.h"
#include "fks_dev_irr.h"

namespace fks {
namespace {

// ------------------------------------------------------------------ irregular kernel
template <int DT, int MODE>
__device__ __forceinline__ void irr_run_lane(const uint8_t* lds, const uint32_t* win, const IrrArgs& a, const DevRun& R,
                                             int64_t e1, int w1) {
  using TR = Traits<MODE == kModeDelta ? FKS_F32 : DT>;  // storage (kModeDelta: the f32 delta)
  const bool on1 = e1 < R.limit, on2 = e1 + 8 < R.limit;
  float p1 = 0.0f, p2 = 0.0f;
  if (MODE != kModeWriteZ) {
    if (on1) p1 = TR::load(R.ptr, e1);
    if (on2) p2 = TR::load(R.ptr, e1 + 8);
  }
  const bool has_wd = (R.flags & FKS_HAS_WD) != 0;
  const float* g = a.g[DT == kDtF32Libm ? FKS_F32 : DT];
  const bool dv = MODE == kModePerturbUpdate && a.gdev;
  const bool upd = dv ? dev_value_apply(a.gdev) : true;
  for (int k = 0; k < a.nseeds; k++) {
    float z1, z2;
    irr_z_pair<DT>(lds, win_word(win, k, w1), win_word(win, k, w1 + 8), z1, z2);
    const float gv = dv ? dev_value_g<DT>(a.gdev) : g[k];
    p1 = apply_one<DT>(p1, z1, gv, R.lr, R.wd, has_wd, MODE, R.ps, upd);
    p2 = apply_one<DT>(p2, z2, gv, R.lr, R.wd, has_wd, MODE, R.ps, upd);
  }
  if (on1) TR::store(R.ptr, e1, p1);
  if (on2) TR::store(R.ptr, e1 + 8, p2);
}

template <int DT, int MODE>
__device__ __forceinline__ void irr_tiny_lane(const uint32_t* win, const IrrArgs& a, const DevTiny& T, int w) {
  using TR = Traits<MODE == kModeDelta ? FKS_F32 : DT>;  // storage (kModeDelta: the f32 delta)
  float p = MODE != kModeWriteZ ? TR::load(T.ptr, 0) : 0.0f;
  const bool has_wd = (T.flags & FKS_HAS_WD) != 0;
  const bool sin_half = (T.flags & kTinySin) != 0;
  const float* g = a.g[DT];
  const bool dv = MODE == kModePerturbUpdate && a.gdev;
  const bool upd = dv ? dev_value_apply(a.gdev) : true;
  for (int k = 0; k < a.nseeds; k++) {
    const float zf = irr_tiny_z(win, k, w, sin_half);  // static_cast<scalar_t>(double): via float for bf16 / f16
    const float z = DT == FKS_F32 ? zf : Traits<DT>::rnd(zf);
    p = apply_one<DT>(p, z, dv ? dev_value_g<DT>(a.gdev) : g[k], T.lr, T.wd, has_wd, MODE, T.ps, upd);
  }
  TR::store(T.ptr, 0, p);
}

// The update visitor: a lane with work runs every seed over its own elements in registers and
// stores them once; a lane without work does nothing.
template <int MODE>
struct IrrUpdate {
  const IrrArgs& a;
  __device__ __forceinline__ void run(const uint8_t* lds, const uint32_t* win, const DevRun& R, bool mine, int64_t e1,
                                      int w1) {
    if (mine) {
      switch (R.dtype) {
        case FKS_F32:
          if (a.libm) irr_run_lane<kDtF32Libm, MODE>(lds, win, a, R, e1, w1);
          else irr_run_lane<FKS_F32, MODE>(lds, win, a, R, e1, w1);
          break;
        case FKS_BF16: irr_run_lane<FKS_BF16, MODE>(lds, win, a, R, e1, w1); break;
        default: irr_run_lane<FKS_F16, MODE>(lds, win, a, R, e1, w1); break;
      }
    }
  }
  __device__ __forceinline__ void tiny(const uint8_t*, const uint32_t* win, bool mine, int idx, int64_t base) {
    if (mine) {
      const DevTiny T = a.tiny[idx];
      const int w = (int)(T.word - base);
      switch (T.dtype) {
        case FKS_F32: irr_tiny_lane<FKS_F32, MODE>(win, a, T, w); break;
        case FKS_BF16: irr_tiny_lane<FKS_BF16, MODE>(win, a, T, w); break;
        default: irr_tiny_lane<FKS_F16, MODE>(win, a, T, w); break;
      }
    }
  }
};

template <int MODE>
__global__ __launch_bounds__(kApplyThreads) void fks_irregular_kernel(IrrArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds32[];
  IrrUpdate<MODE> vis{a};
  irr_walk(lds32, a, vis);
}

}  // namespace
}  // namespace fks
