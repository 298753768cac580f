// fks_dev_update.h -- rounding to the parameter dtypes, the per-dtype Traits, and the
// per-op-rounded update chain (apply_one / apply_tail / apply_pair / apply_pair_f16dev).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include "fks_internal.h"
#include "fks_dev_lds.h"

namespace fks {
namespace {

// ------------------------------------------------------------------ rounding
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
// RNE to bf16, result kept as the f32 with the same value: ONE v_cvt_pk_bf16_f32 with
// a zero low half (hi = bf16(x), lo = bf16(0) = 0x0000).  NaN stays NaN.
__device__ __forceinline__ float rbf_cvt(float x) {
  const f32x2_t v = {0.0f, x};
  return __builtin_bit_cast(float, __builtin_convertvector(v, bf16x2_t));
}
__device__ __forceinline__ float rbf(float x) { return rbf_cvt(x); }
__device__ __forceinline__ float rhf(float x) {  // RNE to f16 and back
  // The empty asm pins x as an f32 VALUE: without it the backend folds the producing
  // f32 multiply into v_fma_mixlo_f16 (one rounding of the exact product straight to
  // f16), while c10::Half rounds the f32 product first (double rounding).
  asm volatile("" : "+v"(x));
  return static_cast<float>(static_cast<_Float16>(x));
}

// ------------------------------------------------------------------ per-dtype traits
template <int DT>
struct Traits;

typedef __attribute__((address_space(1))) float gf32;
typedef __attribute__((address_space(1))) uint16_t gu16;
typedef __attribute__((address_space(1))) _Float16 gf16;

// load_raw returns the element's bits (kept raw in the software pipeline so that the
// load's wait lands at first use, a block later); cvt turns them into the f32 value.
typedef __attribute__((address_space(1))) uint32_t gu32;

typedef __attribute__((address_space(1))) uint64_t gu64;
typedef uint16_t u16x2_t __attribute__((ext_vector_type(2)));

template <>
struct Traits<FKS_F32> {
  typedef uint64_t Pair;  // two adjacent elements
  __device__ static Pair load_pair(uint64_t a) { return *reinterpret_cast<const gu64*>(a); }
  __device__ static void store_pair(uint64_t a, Pair v) { *reinterpret_cast<gu64*>(a) = v; }
  __device__ static uint32_t lo(Pair v) { return (uint32_t)v; }
  __device__ static uint32_t hi(Pair v) { return (uint32_t)(v >> 32); }
  __device__ static Pair pack(uint32_t l, uint32_t h) { return (uint64_t)l | ((uint64_t)h << 32); }
  __device__ static uint32_t bits(float v) { return __float_as_uint(v); }
  __device__ static uint32_t load_raw(uint64_t p, int64_t i) { return reinterpret_cast<const gu32*>(p)[i]; }
  __device__ static float cvt(uint32_t r) { return __uint_as_float(r); }
  __device__ static float load(uint64_t p, int64_t i) { return reinterpret_cast<const gf32*>(p)[i]; }
  __device__ static void store(uint64_t p, int64_t i, float v) { reinterpret_cast<gf32*>(p)[i] = v; }
  __device__ static float rnd(float x) { return x; }
};

template <>
struct Traits<FKS_BF16> {
  typedef uint32_t Pair;  // two adjacent elements
  __device__ static Pair load_pair(uint64_t a) { return *reinterpret_cast<const gu32*>(a); }
  __device__ static void store_pair(uint64_t a, Pair v) { *reinterpret_cast<gu32*>(a) = v; }
  __device__ static uint32_t lo(Pair v) { return v & 0xffffu; }
  __device__ static uint32_t hi(Pair v) { return v >> 16; }
  __device__ static Pair pack(uint32_t l, uint32_t h) { return (l & 0xffffu) | (h << 16); }
  // one element as the bits of its f32 value: a 16-bit load into the high half of a zeroed
  // register (global_load_short_d16_hi), a 16-bit store of the high half (v is bf16-exact)
  __device__ static uint32_t load_hi(uint64_t a) {
    const u16x2_t v = {(uint16_t)0, *reinterpret_cast<const gu16*>(a)};
    return __builtin_bit_cast(uint32_t, v);
  }
  __device__ static void store_hi(uint64_t a, uint32_t v) { *reinterpret_cast<gu16*>(a) = (uint16_t)(v >> 16); }
  __device__ static uint32_t bits(float v) { return __float_as_uint(v) >> 16; }  // v is bf16-exact
  __device__ static uint32_t load_raw(uint64_t p, int64_t i) { return reinterpret_cast<const gu16*>(p)[i]; }
  __device__ static float cvt(uint32_t r) { return __uint_as_float(r << 16); }
  __device__ static float load(uint64_t p, int64_t i) {
    return __uint_as_float((uint32_t)reinterpret_cast<const gu16*>(p)[i] << 16);
  }
  __device__ static void store(uint64_t p, int64_t i, float v) {  // v is bf16-exact
    reinterpret_cast<gu16*>(p)[i] = (uint16_t)(__float_as_uint(v) >> 16);
  }
  __device__ static float rnd(float x) { return rbf(x); }
};

template <>
struct Traits<FKS_F16> {
  typedef uint32_t Pair;
  __device__ static Pair load_pair(uint64_t a) { return *reinterpret_cast<const gu32*>(a); }
  __device__ static void store_pair(uint64_t a, Pair v) { *reinterpret_cast<gu32*>(a) = v; }
  __device__ static uint32_t lo(Pair v) { return v & 0xffffu; }
  __device__ static uint32_t hi(Pair v) { return v >> 16; }
  __device__ static Pair pack(uint32_t l, uint32_t h) { return (l & 0xffffu) | (h << 16); }
  __device__ static uint32_t bits(float v) { return __builtin_bit_cast(uint16_t, static_cast<_Float16>(v)); }
  __device__ static uint32_t load_raw(uint64_t p, int64_t i) { return reinterpret_cast<const gu16*>(p)[i]; }
  __device__ static float cvt(uint32_t r) { return static_cast<float>(__builtin_bit_cast(_Float16, (uint16_t)r)); }
  __device__ static float load(uint64_t p, int64_t i) { return static_cast<float>(reinterpret_cast<const gf16*>(p)[i]); }
  __device__ static void store(uint64_t p, int64_t i, float v) { reinterpret_cast<gf16*>(p)[i] = static_cast<_Float16>(v); }
  __device__ static float rnd(float x) { return rhf(x); }
};

// fp32 tensors of the libm flavour (kDtF32Libm): fp32 in every respect but their z
template <>
struct Traits<kDtF32Libm> : Traits<FKS_F32> {};
constexpr bool is_f32(int dt) { return dt == FKS_F32 || dt == kDtF32Libm; }

// One parameter through one seed.  zo_utils.py:49 (has_wd) / :52 ; optimizer.py:173
// (perturb: p + ps*z, ps = f32(scaling_factor * eps)).
// Each statement is one torch op rounded to the parameter dtype (fp32 opmath).
template <int DT>
__device__ __forceinline__ float apply_one(float p, float z, float g, float lr, float wd, bool has_wd, int mode,
                                           float ps, bool upd = true) {
  using TR = Traits<DT>;
  if (mode == kModeDelta) return __fmaf_rn(g, z, p);   // seed-sharded variant: delta += c_k * z (f32)
  if (mode == kModePerturb || mode == kModePerturbUpdate) {
    p = TR::rnd(p + TR::rnd(ps * z));                  // param.data + scaling_factor * eps * z
    if (mode == kModePerturb || !upd) return p;         // (upd: the device-side apply decision)
  }
  if (mode == kModeUpdate || mode == kModePerturbUpdate) {
    const float gz = TR::rnd(g * z);                    // directional_derivative_value * z
    const float t2 = TR::rnd(gz + TR::rnd(wd * p));     // + weight_decay * param.data
    const float t = has_wd ? t2 : gz;                   // (select: keeps the seed loop branch-free)
    return TR::rnd(p - TR::rnd(lr * t));                // param.data - lr * (...)
  }
  return z;
}

// The directional value of a device-side perturb_step (fks_perturb_step_dev): v[0] = g
// (f32) rounded to the parameter dtype like a VALUE_TENSOR host value, v[1] != 0 applies
// the update.  Read once per workgroup, wave-uniform.
template <int DT>
__device__ __forceinline__ float dev_value_g(const float* v) {
  const float g = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v[0])));
  return is_f32(DT) ? g : Traits<DT>::rnd(g);
}
__device__ __forceinline__ bool dev_value_apply(const float* v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v[1]))) != 0.0f;
}

// The update of an element PAIR (p1, p2) through one seed, zo_utils.py:49 / :52 and
// optimizer.py:173, in packed f32 (v_pk_mul_f32 / v_pk_add_f32: both elements per
// instruction); every op is still rounded to the parameter dtype per element, so the
// values are those of apply_one.
template <int DT>
__device__ __forceinline__ f32x2_t rnd2(f32x2_t x) {
  f32x2_t r;
  r.x = Traits<DT>::rnd(x.x);
  r.y = Traits<DT>::rnd(x.y);
  return r;
}

// g z with g one half of the SGPR pair gg = {g of the even seed, g of the odd seed}: op_sel
// picks half H for both result lanes, so two seeds' scalars share one SGPR pair (a pure
// VALU instruction: no counter, nothing the compiler has to wait for)
template <int H>
__device__ __forceinline__ f32x2_t pk_mul_half(uint64_t gg, f32x2_t z) {
  f32x2_t r;
  if (H == 0)
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1]" : "=v"(r) : "s"(gg), "v"(z));
  else
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(r) : "s"(gg), "v"(z));
  return r;
}

// The update modes' p-dependent part, given gz = rnd(g z): t = gz + rnd(wd p) (or the
// form the launch's weight decay allows), p - rnd(lr t), each op rounded to the dtype.
template <int DT, int MODE>
__device__ __forceinline__ f32x2_t apply_tail(f32x2_t p, f32x2_t gz, float lr, float wd, bool has_wd) {
  f32x2_t t;
  if (MODE == kModeUpdateNoWd || MODE == kModeUpdateWdPos0) {
    t = gz;
  } else if (MODE == kModeUpdateWd0) {
    // wd = +-0: rnd(gz + rnd(wd*p)) == fma(wd, p, gz) (fks_internal.h)
    const f32x2_t ww = {wd, wd};
    t = __builtin_elementwise_fma(ww, p, gz);
  } else {
    const f32x2_t t2 = rnd2<DT>(gz + rnd2<DT>(wd * p));
    if (MODE == kModeUpdateWd) {
      t = t2;
    } else {
      t.x = has_wd ? t2.x : gz.x;
      t.y = has_wd ? t2.y : gz.y;
    }
  }
  return rnd2<DT>(p - rnd2<DT>(lr * t));
}

template <int DT, int MODE>
__device__ __forceinline__ f32x2_t apply_pair(f32x2_t p, f32x2_t z, float g, float lr, float wd, bool has_wd,
                                              float ps, bool upd = true) {
  if (MODE == kModeDelta) {  // delta += c_k * z: one v_pk_fma_f32 per element pair and seed
    const f32x2_t gg = {g, g};
    return __builtin_elementwise_fma(gg, z, p);
  }
  if (MODE == kModePerturb || MODE == kModePerturbUpdate) {
    p = rnd2<DT>(p + rnd2<DT>(ps * z));
    if (MODE == kModePerturb || !upd) return p;
  }
  if (MODE == kModeUpdate || MODE == kModeUpdateWd || MODE == kModeUpdateNoWd || MODE == kModePerturbUpdate ||
      MODE == kModeUpdateWd0 || MODE == kModeUpdateWdPos0)
    return apply_tail<DT, MODE>(p, rnd2<DT>(g * z), lr, wd, has_wd);
  return z;
}

// f16 parameters in the torch_rocm stream.  The reference then runs torch's DEVICE
// elementwise kernels (ATen/native/cuda/CUDALoops.cuh), and how those round a Half
// "f32 scalar * f16 tensor" product depends on the code path (measured on this image,
// tools/diag_f16_tail.py, profiles/r05_f16_rounding.log):
//   * the 8-wide vectorized path -- every pointer 16-byte aligned, elements below
//     N - N % 2048 (full blocks of 256 threads x 8) -- rounds the f32 product to f16:
//     TWICE, like c10::Half on the CPU;
//   * the unrolled path -- the partial last block, or a tensor that is not 16-byte aligned
//     -- is compiled to v_fma_mixlo_f16 a, b, 0: ONE rounding of the exact product.
// The two differ when the f32 product lands on an f16 rounding midpoint (and in the sign of
// a zero product).  The chain's products: g z, lr t and the perturbation's ps z read fresh,
// aligned tensors (z, t); wd p reads the parameter -- its own alignment at the call's first
// seed, a fresh aligned tensor after it (the reference rebinds param.data every step,
// zo_utils.py:49).  The sums of two f16 values round the same either way.
__device__ __forceinline__ float mul_f16_ref(float a, float b, bool once) {  // b f16-exact
  if (once) {
    uint32_t r = 0;
    asm volatile("v_fma_mixlo_f16 %0, %1, %2, 0" : "+v"(r) : "v"(a), "v"(b));
    return (float)__builtin_bit_cast(_Float16, (uint16_t)(r & 0xffffu));
  }
  return rhf(a * b);
}
template <int MODE>
__device__ __forceinline__ f32x2_t apply_pair_f16dev(f32x2_t p, f32x2_t z, float g, float lr, float wd, bool has_wd,
                                                     float ps, bool upd, const bool (&once)[2],
                                                     const bool (&wd_once)[2]) {
  float q[2] = {p.x, p.y};
  const float zz[2] = {z.x, z.y};
  const bool use_wd = MODE == kModeUpdateNoWd ? false
                      : (MODE == kModeUpdateWd || MODE == kModeUpdateWd0 || MODE == kModeUpdateWdPos0) ? true
                                                                                                          : has_wd;
#pragma unroll
  for (int i = 0; i < 2; i++) {
    if (MODE == kModePerturb || MODE == kModePerturbUpdate) {
      q[i] = rhf(q[i] + mul_f16_ref(ps, zz[i], once[i]));
      if (MODE == kModePerturb || !upd) continue;
    }
    const float gz = mul_f16_ref(g, zz[i], once[i]);
    const float t = use_wd ? rhf(gz + mul_f16_ref(wd, q[i], wd_once[i])) : gz;
    q[i] = rhf(q[i] - mul_f16_ref(lr, t, once[i]));
  }
  return (f32x2_t){q[0], q[1]};
}

}  // namespace
}  // namespace fks
