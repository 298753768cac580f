// fks_kern_philox.h -- the torch_rocm stream's kernels (fks_philox_kernel, fks_philox_vec_kernel)
// and fks_delta_apply_kernel, the last step of the seed-sharded variant.
#pragma once
#include <hip/hip_runtime.h>

#include "fks_internal.h"
#include "fks_dev_lds.h"
#include "fks_dev_update.h"
#include "fks_dev_zgen.h"

namespace fks {
namespace {

// ------------------------------------------------------------------ torch_rocm stream
// fks_philox_kernel<MODE>: the z stream torch.normal draws on a HIP device (FKS_STREAM_ROCM;
// PhxTensor in fks_internal.h has the mapping), then the same per-op-rounded update as the
// CPU stream.  One thread per work item (tensor, idx, j): for every seed in order one
// Philox4x32-10 call at counter (off4 + j, idx, 0) and key (seed), two rocrand Box-Muller
// pairs, four elements idx + stride (4 j + i).  Counter-mode: no generator state, no jump.

// The item's four elements through every seed of the pass, in seed order, as two packed
// pairs (apply_pair: the values of apply_one); MODE may be a launch-wide weight-decay
// specialisation of kModeUpdate (kModeUpdateWd / NoWd / Wd0, as the CPU stream's kernels).
// (phx_seeds: the seed loop of work item (idx, j) on its four elements e[i], values p[i])
template <int DT, int MODE_>
__device__ __forceinline__ void phx_seeds(const PhiloxArgs& a, const PhxTensor& T, uint32_t idx, uint64_t j,
                                          const int64_t e[4], float p[4]) {
  // (the host gives kModeUpdateWdPos0 launches bf16 / f32 tensors only)
  constexpr int MODE = (MODE_ == kModeUpdateWdPos0 && DT == FKS_F16) ? (int)kModeUpdateWd0 : MODE_;
#pragma unroll
  for (int i = 0; i < 4; i++)  // kModeUpdateWdPos0: a +-inf parameter is NaN after the reference's first seed (wd p)
    if (MODE == kModeUpdateWdPos0 && __builtin_isinf(p[i])) p[i] = __builtin_nanf("");
  const bool has_wd = (T.flags & FKS_HAS_WD) != 0;
  const bool dv = MODE == kModePerturbUpdate && a.gdev;
  const bool upd = dv ? dev_value_apply(a.gdev) : true;
  const float gd = dv ? dev_value_g<DT>(a.gdev) : 0.0f;
  const PhxRound1 r1 = philox_round1(T.off4 + j, idx);
  f32x2_t pA = {p[0], p[1]}, pB = {p[2], p[3]};
  // f16: which elements torch's unrolled path (one rounding) takes (mul_f16_ref): the
  // partial last block of the launch, or every element of a launch whose fresh tensors do
  // not start 16-byte aligned (a later 32-bit piece of a tensor past 2^31 bytes)
  bool tail[4] = {false, false, false, false};
  const bool p16 = (T.flags & kPhxWdP16) != 0;  // the first wd * p's operand, in the reference
  if (DT == FKS_F16) {
    const bool fresh16 = (T.flags & kPhxFresh16) != 0;
#pragma unroll
    for (int i = 0; i < 4; i++) tail[i] = !fresh16 || e[i] >= T.numel - T.numel % kTorchHalfBlockWork;
  }
  for (int k = 0; k < a.nseeds; k++) {
    const uint64_t seed = a.seeds[k];  // wave-uniform: scalar loads
    const float g = dv ? gd : a.g[3 * k + DT];
    const uint4 w = philox4x32_10(r1, seed);
    f32x2_t zA, zB;
    if constexpr (DT == FKS_BF16) {
      phx_z_bf16(w, zA, zB);
    } else {
      phx_box_muller2(w, zA, zB);
      zA = (f32x2_t){phx_cast<DT>(zA.x), phx_cast<DT>(zA.y)};
      zB = (f32x2_t){phx_cast<DT>(zB.x), phx_cast<DT>(zB.y)};
    }
    if (MODE == kModeWriteZ) {
      pA = zA;
      pB = zB;
    } else if constexpr (DT == FKS_F16 && MODE != kModeDelta) {  // torch's device rounding of the products (mul_f16_ref)
      // wd p at the call's first seed reads the caller's parameter (its alignment); later
      // seeds read the reference's freshly allocated, aligned result.  (kModePerturbUpdate's
      // update follows the restore perturbation, whose result is fresh.)
      const bool first = a.call_first && k == 0 && MODE != kModePerturbUpdate;
      const bool wA[2] = {tail[0] || (first && !p16), tail[1] || (first && !p16)};
      const bool wB[2] = {tail[2] || (first && !p16), tail[3] || (first && !p16)};
      const bool oA[2] = {tail[0], tail[1]}, oB[2] = {tail[2], tail[3]};
      pA = apply_pair_f16dev<MODE>(pA, zA, g, T.lr, T.wd, has_wd, T.ps, upd, oA, wA);
      pB = apply_pair_f16dev<MODE>(pB, zB, g, T.lr, T.wd, has_wd, T.ps, upd, oB, wB);
    } else {
      pA = apply_pair<DT, MODE>(pA, zA, g, T.lr, T.wd, has_wd, T.ps, upd);
      pB = apply_pair<DT, MODE>(pB, zB, g, T.lr, T.wd, has_wd, T.ps, upd);
    }
  }
  p[0] = pA.x; p[1] = pA.y; p[2] = pB.x; p[3] = pB.y;
}

template <int DT, int MODE>
__device__ __forceinline__ void phx_item(const PhiloxArgs& a, const PhxTensor& T, int64_t r) {
  using TR = Traits<MODE == kModeDelta ? FKS_F32 : DT>;  // storage (kModeDelta: the f32 delta)
  const uint32_t S = T.stride;
  const uint32_t idx = (uint32_t)(r % S);
  const uint64_t j = (uint64_t)(r / S);
  int64_t e[4];
  bool on[4];
  float p[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    e[i] = (int64_t)idx + (int64_t)S * (int64_t)(4 * j + i);
    on[i] = e[i] < T.numel;
    p[i] = (MODE != kModeWriteZ && on[i]) ? TR::load(T.ptr, e[i]) : 0.0f;
  }
  phx_seeds<DT, MODE>(a, T, idx, j, e, p);
#pragma unroll
  for (int i = 0; i < 4; i++)
    if (on[i]) TR::store(T.ptr, e[i], p[i]);
}

// kPhxVec consecutive work items (idx0 .. idx0 + 7 of one row j; item boundaries of
// tensors and shards are multiples of 256): element i of each lies in the 8-element run
// idx0 + S (4 j + i) + [0, 8), so the eight items load and store as four 16-byte runs
// (bf16 / f16; two each for f32) instead of 32 single-element accesses.  A call of few
// seeds is bound by the memory accesses in flight, not by the VALU (the item loop above
// issues 2-byte loads, 128 bytes per wave instruction: a one-seed perturb of the 7B layout
// took 20.9 ms there, 7.2 ms here; profiles/r05h_smallk_rocm_maxk*.log).
constexpr int kPhxVec = FKS_PHX_VEC_ITEMS;  // 8 (A/B: 4)
static_assert(kPhxVec == 4 || kPhxVec == 8, "16- or 8-byte runs of 2-byte elements");
typedef __attribute__((address_space(1))) u32x4_t gu128;

typedef __attribute__((address_space(1))) u32x2_t gu64v;

template <int DT>
__device__ __forceinline__ void phx_load8(uint64_t ptr, int64_t e, float v[kPhxVec]) {
  const gu128* q = reinterpret_cast<const gu128*>(ptr + (uint64_t)e * (DT == FKS_F32 ? 4 : 2));
  if constexpr (kPhxVec == 4) {
    if constexpr (DT == FKS_F32) {
      const u32x4_t x = q[0];
      v[0] = __uint_as_float(x.x); v[1] = __uint_as_float(x.y); v[2] = __uint_as_float(x.z); v[3] = __uint_as_float(x.w);
    } else {
      const u32x2_t x = *reinterpret_cast<const gu64v*>(q);
      v[0] = Traits<DT>::cvt(x.x & 0xffffu); v[1] = Traits<DT>::cvt(x.x >> 16);
      v[2] = Traits<DT>::cvt(x.y & 0xffffu); v[3] = Traits<DT>::cvt(x.y >> 16);
    }
  } else if constexpr (DT == FKS_F32) {
    const u32x4_t x = q[0], y = q[1];
    const uint32_t w[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = __uint_as_float(w[i]);
  } else {
    const u32x4_t x = q[0];
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int i = 0; i < 4; i++) {
      v[2 * i] = Traits<DT>::cvt(w[i] & 0xffffu);
      v[2 * i + 1] = Traits<DT>::cvt(w[i] >> 16);
    }
  }
}

template <int DT>
__device__ __forceinline__ void phx_store8(uint64_t ptr, int64_t e, const float v[kPhxVec]) {
  gu128* q = reinterpret_cast<gu128*>(ptr + (uint64_t)e * (DT == FKS_F32 ? 4 : 2));
  if constexpr (kPhxVec == 4) {
    if constexpr (DT == FKS_F32) {
      q[0] = (u32x4_t){__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
    } else {
      *reinterpret_cast<gu64v*>(q) = (u32x2_t){Traits<DT>::pack(Traits<DT>::bits(v[0]), Traits<DT>::bits(v[1])),
                                               Traits<DT>::pack(Traits<DT>::bits(v[2]), Traits<DT>::bits(v[3]))};
    }
  } else if constexpr (DT == FKS_F32) {
    q[0] = (u32x4_t){__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
    q[1] = (u32x4_t){__float_as_uint(v[4]), __float_as_uint(v[5]), __float_as_uint(v[6]), __float_as_uint(v[7])};
  } else {
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = Traits<DT>::pack(Traits<DT>::bits(v[2 * i]), Traits<DT>::bits(v[2 * i + 1]));
    q[0] = (u32x4_t){w[0], w[1], w[2], w[3]};
  }
}

template <int DT, int MODE>
__device__ __forceinline__ void phx_vitem(const PhiloxArgs& a, const PhxTensor& T, int64_t r0) {
  constexpr int ST = MODE == kModeDelta ? FKS_F32 : DT;  // storage (kModeDelta: the f32 delta)
  const uint32_t S = T.stride;
  const uint32_t idx0 = (uint32_t)(r0 % S);
  const uint64_t j = (uint64_t)(r0 / S);
  const int64_t e0 = (int64_t)idx0 + (int64_t)S * (int64_t)(4 * j);
  // whole runs only: 16-byte aligned data (idx0 and S are multiples of 8) and every element
  // of the four runs inside the tensor; else (a tensor's last row, unaligned data) per item
  if (!(T.flags & kPhxP16) || e0 + 3 * (int64_t)S + kPhxVec > T.numel) {
    for (int q = 0; q < kPhxVec; q++) phx_item<DT, MODE>(a, T, r0 + q);
    return;
  }
  float v[4][kPhxVec];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (MODE == kModeWriteZ) {
#pragma unroll
      for (int q = 0; q < kPhxVec; q++) v[i][q] = 0.0f;
    } else {
      phx_load8<ST>(T.ptr, e0 + (int64_t)S * i, v[i]);
    }
  }
#pragma unroll
  for (int q = 0; q < kPhxVec; q++) {
    int64_t e[4];
    float p[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      e[i] = e0 + (int64_t)S * i + q;
      p[i] = v[i][q];
    }
    phx_seeds<DT, MODE>(a, T, idx0 + (uint32_t)q, j, e, p);
#pragma unroll
    for (int i = 0; i < 4; i++) v[i][q] = p[i];
  }
#pragma unroll
  for (int i = 0; i < 4; i++) phx_store8<ST>(T.ptr, e0 + (int64_t)S * i, v[i]);
}

template <int MODE>
__global__ __launch_bounds__(256) void fks_philox_kernel(PhiloxArgs a) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  int t0 = 0;  // items only grow: the search starts at the previous item's tensor
  for (int64_t it = a.item_lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < a.item_hi; it += step) {
    int lo = t0, hi = a.nt - 1;  // the last tensor whose first item is <= it
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (a.t[mid].item0 <= it) lo = mid; else hi = mid - 1;
    }
    t0 = lo;
    const PhxTensor T = a.t[lo];
    switch (T.dtype) {
      case FKS_F32: phx_item<FKS_F32, MODE>(a, T, it - T.item0); break;
      case FKS_BF16: phx_item<FKS_BF16, MODE>(a, T, it - T.item0); break;
      default: phx_item<FKS_F16, MODE>(a, T, it - T.item0); break;
    }
  }
}

// fks_philox_kernel over kPhxVec-item groups (phx_vitem): the launch form of calls of few
// seeds (the ZO step's perturb / restore + update, K-small reconstructs)
// The tensor of a wave's 64 groups is looked up once per wave, with
// wave-uniform indices, instead of a per-lane binary search whose dependent vector loads
// each wait for every load and store in flight (vmcnt is in order), from a
// copy of the tensor table in LDS (launches of at most kPhxLdsTensors tensors; device
// memory for longer tables).  One-seed
// perturb of the 7B layout: 7.07 (per-lane search) / 6.86-7.30 (every lookup in device
// memory) / 6.41-6.45 ms (this form),
// 32-seed launches unchanged (profiles/r05k_phx_vec_uniform_ab.log)
constexpr int kPhxLdsTensors = 512;
template <class Tab>
__device__ __forceinline__ int phx_find_t(Tab tab, int nt, int64_t it, int lo, int probes) {
  // the last tensor whose first item is <= it, at or after lo (items only grow; a wave's
  // next groups lie mostly in the same or the next tensor: a few probes, then bisection)
  for (int p = 0; p < probes; p++) {
    if (lo + 1 >= nt || tab[lo + 1].item0 > it) return lo;
    ++lo;
  }
  int hi = nt - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].item0 <= it) lo = mid; else hi = mid - 1;
  }
  return lo;
}
template <int MODE, class Tab>
__device__ __forceinline__ void phx_vec_uniform(const PhiloxArgs& a, Tab tab, int64_t step) {
  const int lane = (int)(threadIdx.x & 63u);
  int64_t wb = rfl64(a.item_lo + ((int64_t)blockIdx.x * blockDim.x + (int64_t)(threadIdx.x & ~63u)) * kPhxVec);
  int ts = 0;
  // this lane's group of the wave's groups from wb, and its tensor (ts: the wave's first)
  auto lane_tensor = [&](int64_t w, int t, int64_t& it) {
    const int64_t wend = w + 64 * kPhxVec < a.item_hi ? w + 64 * kPhxVec : a.item_hi;
    const bool one = t + 1 >= a.nt || tab[t + 1].item0 >= wend;  // the whole wave in tensor t
    it = w + (int64_t)lane * kPhxVec;
    return one ? t : phx_find_t(tab, a.nt, it < a.item_hi ? it : a.item_hi - 1, t, 0);
  };
  for (; wb < a.item_hi; wb += step) {
    ts = __builtin_amdgcn_readfirstlane(phx_find_t(tab, a.nt, wb, ts, 2));
    int64_t it;
    const int ti = lane_tensor(wb, ts, it);
    if (it >= a.item_hi) continue;
    const PhxTensor T = tab[ti];
    switch (T.dtype) {
      case FKS_F32: phx_vitem<FKS_F32, MODE>(a, T, it - T.item0); break;
      case FKS_BF16: phx_vitem<FKS_BF16, MODE>(a, T, it - T.item0); break;
      default: phx_vitem<FKS_F16, MODE>(a, T, it - T.item0); break;
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void fks_philox_vec_kernel(PhiloxArgs a) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x * kPhxVec;
  extern __shared__ PhxTensor s_tab[];
  if (a.nt <= kPhxLdsTensors) {
    constexpr int W = (int)(sizeof(PhxTensor) / 4);
    for (int i = (int)threadIdx.x; i < a.nt * W; i += (int)blockDim.x)
      reinterpret_cast<uint32_t*>(s_tab)[i] = reinterpret_cast<const uint32_t*>(a.t)[i];
    __syncthreads();
    phx_vec_uniform<MODE>(a, s_tab, step);
    return;
  }
  phx_vec_uniform<MODE>(a, a.t, step);
}

// ------------------------------------------------------------------ delta apply
// Seed-sharded variant, last step: p_K = a^K p_0 - delta (delta = sum_k lr g_k
// a^(K-1-k) z_k, a = 1 - lr wd, all-reduced over the ranks), one fma in f32 and one
// rounding to the parameter dtype.  grid (x, tensors): each row walks one tensor.
template <int DT>
__device__ __forceinline__ void delta_apply_one(const DeltaApplyDesc& D, const float* delta, int64_t e) {
  using TR = Traits<DT>;
  const float p = TR::load(D.ptr, e);
  TR::store(D.ptr, e, TR::rnd(__fmaf_rn(D.decay, p, -delta[D.delta_off + e])));
}

__global__ __launch_bounds__(256) void fks_delta_apply_kernel(const DeltaApplyDesc* d, const float* delta) {
  const DeltaApplyDesc D = d[blockIdx.y];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < D.numel; e += stride) {
    switch (D.dtype) {
      case FKS_F32: delta_apply_one<FKS_F32>(D, delta, e); break;
      case FKS_BF16: delta_apply_one<FKS_BF16>(D, delta, e); break;
      default: delta_apply_one<FKS_F16>(D, delta, e); break;
    }
  }
}

}  // namespace
}  // namespace fks
