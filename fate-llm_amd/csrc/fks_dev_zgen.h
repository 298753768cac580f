// fks_dev_zgen.h -- the z generators: the CPU stream's Box-Muller from MT19937 words (fp32
// Cephes, fp32 glibc, bf16 through the R | C | S tables) and the torch_rocm stream's
// Philox4x32-10 + rocrand Box-Muller.
#pragma once
#include <hip/hip_runtime.h>

#include "fks_internal.h"
#include "fks_bitslice.h"
#ifndef FKS_HD
#define FKS_HD __device__ __forceinline__
#endif
#include "fks_libm.h"
#include "fks_dev_lds.h"
#include "fks_dev_update.h"
#include "fks_dev_mt.h"

namespace fks {
namespace {

__constant__ float c_tab_bf16[3 * 256];  // R | C | S, set once from fks::tables()

// LDS: [R[256] f32 | (C,S)[256] f32x2 | windows (kMaxSeedsPerPass + 1) x 624 u32]
// ((R,R) pairs at the (C,S) index scale measured 8 % slower: the radius lookup moves
// twice the LDS bytes)
constexpr int kLdsRBytes = 256 * 4;
constexpr int kLdsTabBytes = kLdsRBytes + 256 * 8;
constexpr int kLdsCsOff = kLdsRBytes;
constexpr int kLdsStBytes = (kMaxSeedsPerPass + 1) * kMtN * 4;

// the bf16 tables from constant memory to the LDS at `lds` (the kernel's LDS 0): R, then (C,S)
__device__ __forceinline__ void tab_bf16_fill(uint8_t* lds, int tid, int nthreads) {
  float2* tabCS = reinterpret_cast<float2*>(lds + kLdsCsOff);
  for (int i = tid; i < 256; i += nthreads) {
    reinterpret_cast<float*>(lds)[i] = c_tab_bf16[i];
    tabCS[i] = make_float2(c_tab_bf16[256 + i], c_tab_bf16[512 + i]);
  }
}

// Thread q < 312 of a fast-segment workgroup owns Box-Muller pair q of every block: 16-block
// q/8, slot q%8, i.e. block words j1 = 16*(q/8) + q%8 and j1 + 8 (DistributionTemplates.h:141-146),
// which lie in one 16-block and so in one segment; pair_off is the LDS byte of that word pair in
// window 0.  (Two functions returning values: as one function with two reference results the
// compiler orders fks_apply_kernel's address arithmetic differently.)
__device__ __forceinline__ int pair_word(int tid) { return 16 * (tid >> 3) + (tid & 7); }
__device__ __forceinline__ int pair_off(int j1) { return kLdsTabBytes + 4 * wperm(j1); }

// ------------------------------------------------------------------ fp32 Box-Muller
// normal_fill_16_AVX2 (DistributionTemplates.h:88-106) with log256_ps / sincos256_ps
// (avx_mathfun.h:90-160, 426-520) restated lane by lane; the fmaf()s are the
// contractions GCC applies in libtorch's AVX2/AVX512 build (pinned bit-exact by
// oracle/fks_oracle.c against the reference's golden streams).
__device__ __forceinline__ float cephes_logf(float x) {  // x in [2^-24, 1]
  // the "x < sqrt(1/2)" select as integer arithmetic: x is a normal float in [0.5, 1)
  // (ordered like its bits), the mask the sign of bits(x) - bits(0.70710678f); "mask ? x :
  // 0" is bits(x) & mask and e = float(imm0 - 126 + mask) the exact integer
  // (imm0 - 0x7f) + 1 - (mask ? 1 : 0): no compare, no select, no hazard wait
  const uint32_t xb0 = __float_as_uint(x);
  const uint32_t xb = (xb0 & ~0x7f800000u) | 0x3f000000u;
  const int32_t m = (int32_t)(xb - 0x3F3504F3u) >> 31;
  const float e = (float)((int32_t)(xb0 >> 23) - 126 + m);
  const float tmp = __uint_as_float(xb & (uint32_t)m);
  x = __uint_as_float(xb) - 1.0f;
  x = x + tmp;
  const float z = x * x;
  float y = 7.0376836292E-2f;
  y = __fmaf_rn(y, x, -1.1514610310E-1f);
  y = __fmaf_rn(y, x, 1.1676998740E-1f);
  y = __fmaf_rn(y, x, -1.2420140846E-1f);
  y = __fmaf_rn(y, x, +1.4249322787E-1f);
  y = __fmaf_rn(y, x, -1.6668057665E-1f);
  y = __fmaf_rn(y, x, +2.0000714765E-1f);
  y = __fmaf_rn(y, x, -2.4999993993E-1f);
  y = __fmaf_rn(y, x, +3.3333331174E-1f);
  y = y * x;
  y = __fmaf_rn(y, z, e * -2.12194440e-4f);
  y = __fmaf_rn(-z, 0.5f, y);
  x = x + y;
  x = __fmaf_rn(e, 0.693359375f, x);
  return x;
}

// fp32 z pair from the two RAW words of a 16-block: normal_fill_16_AVX2
// (DistributionTemplates.h:88-106) with log256_ps / sincos256_ps (avx_mathfun.h:90-160,
// 426-520), as oracle/fks_oracle.c restates it literally, with fewer instructions -- all
// exact rewrites on this input domain (pinned by the golden fp32 streams):
//   * both words tempered on the 64-bit pair (masks clear the bits one word shifts into
//     the other; only the low 24 bits are kept);
//   * theta = 2*pi*d2 >= +0, so sincos256_ps's sign extraction and abs are identities;
//   * its select-and-add merge of the two polynomials is a swap (the adds involve an
//     exact zero; a zero's sign cannot reach z, which is rounded as radius*s + 0);
//   * radius*c + 0 (mul, then the fmadd with std 1, mean 0) is fma(radius, c, 0): the
//     exact product is never a nonzero below the subnormal range here.
__device__ __forceinline__ u32x2_t temper_pair_u24(u32x2_t y) {
  u32x2_t t = shr64<11>(y);
  y.x = __builtin_amdgcn_bitop3_b32(y.x, t.x, 0x001FFFFFu, kXorAnd);
  y.y ^= t.y;
  t = shl64<7>(y);
  y.x = __builtin_amdgcn_bitop3_b32(y.x, t.x, 0x9d2c5680u, kXorAnd);
  y.y = __builtin_amdgcn_bitop3_b32(y.y, t.y, 0x9d2c5680u, kXorAnd);
  t = shl64<15>(y);
  y.x = __builtin_amdgcn_bitop3_b32(y.x, t.x, 0xefc60000u, kXorAnd);
  y.y = __builtin_amdgcn_bitop3_b32(y.y, t.y, 0xefc60000u, kXorAnd);
  t = shr64<18>(y);
  y.x = __builtin_amdgcn_bitop3_b32(y.x, t.x, 0x3FFFu, kXorAnd) & 0xFFFFFFu;
  y.y = __builtin_amdgcn_bitop3_b32(y.y, t.y, 0xFFFFFFu, kXorMask);
  return y;
}

__device__ __forceinline__ void cephes_sincosf_nonneg(float x, float& s, float& c) {
  float y = x * 1.27323954473516f;
  int32_t imm2 = (int32_t)y;
  imm2 = (imm2 + 1) & ~1;
  y = (float)imm2;
  const bool poly_mask = (imm2 & 2) == 0;
  x = __fmaf_rn(y, -0.78515625f, x);
  x = __fmaf_rn(y, -2.4187564849853515625e-4f, x);
  x = __fmaf_rn(y, -3.77489497744594108e-8f, x);
  const float z = x * x;
  float yc = 2.443315711809948E-005f;
  yc = __fmaf_rn(yc, z, -1.388731625493765E-003f);
  yc = __fmaf_rn(yc, z, 4.166664568298827E-002f);
  yc = yc * z;
  yc = __fmaf_rn(yc, z, -(z * 0.5f));
  yc = yc + 1.0f;
  float ys = -1.9515295891E-4f;
  ys = __fmaf_rn(ys, z, 8.3321608736E-3f);
  ys = __fmaf_rn(ys, z, -1.6666654611E-1f);
  ys = ys * z;
  ys = __fmaf_rn(ys, x, x);
  const float xmm1 = poly_mask ? ys : yc;
  const float xmm2 = poly_mask ? yc : ys;
  // sign_bit_sin = bit 2 of imm2 at bit 31; sign_bit_cos = bit 2 of ~(imm2 - 2), i.e. the
  // complement of bit 31 of (imm2 << 29) - (2 << 29): one v_bitop3 each
  const uint32_t sh = (uint32_t)imm2 << 29;
  s = __uint_as_float(__builtin_amdgcn_bitop3_b32(__float_as_uint(xmm1), sh, 0x80000000u, kXorAnd));
  c = __uint_as_float(__builtin_amdgcn_bitop3_b32(__float_as_uint(xmm2), sh - 0x40000000u, 0x80000000u, kXorNotAnd));
}

// Correctly rounded sqrt of the radius input x = -2 log(u1), as _mm256_sqrt_ps: the
// compiler's correctly rounded expansion (a bare v_sqrt_f32 is NOT correctly rounded on
// this domain), checked on all 2^24 inputs against the exact midpoint criterion
// (fks_device_selfcheck FKS_CHECK_SQRT_DOMAIN, a GPU test).  (Restricting it to the
// domain -- x is +-0 or in [1.19e-7, 33.3], so the rescaling and class select are dead,
// as phx_radius2 does for the Philox stream -- issues 14 % fewer VALU instructions in the
// fp32 19-seed kernel but 50 % more hazard s_nops between its compares and selects, and
// measured 3 % slower: profiles/r04h_sqrt_ab.log.  v_sqrt_f64 rounded to f32 -- three
// instructions, no select -- is 4.7 % faster but NOT correctly rounded: the self check
// counts 1,326,243 of the 2^24 inputs wrong, profiles/r04i_sqrt64.log.)
__device__ __forceinline__ float radius_sqrt(float x) { return sqrtf(x); }

__device__ __forceinline__ void z_pair_f32_raw(uint32_t r1, uint32_t r2, float& z1, float& z2) {
  u32x2_t w;
  w.x = r1;
  w.y = r2;
  const u32x2_t t = temper_pair_u24(w);
  // u1 = 1 - d1 (exact: d1 = t.x 2^-24) as one fma; theta = RN(2pi_f * t.y 2^-24) =
  // RN((2pi_f 2^-24) * t.y), the power-of-two scaling exact: one multiply
  const float u1 = __fmaf_rn((float)t.x, -1.0f / 16777216.0f, 1.0f);
  const float theta = (float)t.y * (6.28318548202514648438f / 16777216.0f);
  const float radius = radius_sqrt(-2.0f * cephes_logf(u1));
  float s, c;
  cephes_sincosf_nonneg(theta, s, c);
  z1 = __fmaf_rn(radius, c, 0.0f);
  z2 = __fmaf_rn(radius, s, 0.0f);
}

// The libm flavour of the same pair (kDtF32Libm; normal_fill_16<float>,
// DistributionTemplates.h:139-149, under ATen's DEFAULT CPU capability): glibc's logf / sinf
// / cosf in double as fks_libm.h restates them, e_logf.c's 16 {invc, logc} pairs read from
// LDS at byte `tab`; radius * cos(theta) * std + mean with std 1, mean 0 is one rounding of
// the product and -0 -> +0, the fma with a +0 addend.
typedef double f64x2_t __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) f64x2_t lds_f64x2_t;
constexpr int kLdsLogfBytes = 16 * 16;
__device__ __forceinline__ void logf_tab_fill(uint32_t tab, int tid, int nthreads) {
  for (int i = tid; i < 16; i += nthreads)
    *(lds_f64x2_t*)(size_t)(tab + 16u * (uint32_t)i) = (f64x2_t){fks_libm::kLogfTab[i][0], fks_libm::kLogfTab[i][1]};
}
__device__ __forceinline__ void z_pair_f32_libm(uint32_t tab, uint32_t r1, uint32_t r2, float& z1, float& z2) {
  u32x2_t w;
  w.x = r1;
  w.y = r2;
  const u32x2_t t = temper_pair_u24(w);
  const float u1 = __fmaf_rn((float)t.x, -1.0f / 16777216.0f, 1.0f);  // 1 - data[j], exact
  const f64x2_t e = *(const lds_f64x2_t*)(size_t)(tab + 16u * (uint32_t)fks_libm::logf_index(u1));
  const float radius = radius_sqrt(-2.0f * fks_libm::logf_core<true>(u1, e.x, e.y));
  const float theta = fks_libm::theta_of(t.y);  // 2.0f * c10::pi<double> * data[j + 8]
  float s, c;
  fks_libm::sincosf_glibc<true>(theta, s, c);
  z1 = __fmaf_rn(radius, c, 0.0f);
  z2 = __fmaf_rn(radius, s, 0.0f);
}

// bf16 Box-Muller pair before the final rounding: (R[a] * C[b], R[a] * S[b]) + 0 as ONE
// v_pk_fma_f32 (R*C is exact in f32: 8-bit x 8-bit significands; the +0 addend turns
// -0 into +0 like normal_fill_16's "+ mean").  (R,R) pairs at LDS 0, (C,S) pairs at 2048.
__device__ __forceinline__ f32x2_t z_pair_bf16_raw(uint32_t r1, uint32_t r2) {
  u32x2_t w;
  w.x = r1;
  w.y = r2;
  const u32x2_t ab = temper_pair_u8x8(w);
  const float r = lds_f32(ab.x >> 1);
  const f32x2_t rr = {r, r};
  const f32x2_t cs = lds_f32x2(kLdsCsOff + ab.y);
  const f32x2_t zero = {0.0f, 0.0f};
  return __builtin_elementwise_fma(rr, cs, zero);
}

// z pair of seed k for this lane's 16-block slot: raw words j1, j1+8 -> (z_j, z_{j+8})
template <int DT>
__device__ __forceinline__ void z_pair(const uint8_t* lds, uint32_t r1, uint32_t r2, float& z1, float& z2) {
  if constexpr (DT == FKS_F32) {
    z_pair_f32_raw(r1, r2, z1, z2);
  } else if constexpr (DT == kDtF32Libm) {  // the logf table at `lds` (kernels of this dtype: LDS 0)
    z_pair_f32_libm((uint32_t)(size_t)(const __attribute__((address_space(3))) uint8_t*)lds, r1, r2, z1, z2);
  } else {
    // normal_fill_16<BFloat16>: z = bf16(R[a] * C[b]) * 1 + 0 (std, mean).  R*C is exact
    // in f32 (8-bit x 8-bit significands) and fma(R, C, +0) turns -0 into +0 like "+ mean".
    const f32x2_t zz = z_pair_bf16_raw(r1, r2);
    z1 = rbf(zz.x);
    z2 = rbf(zz.y);
  }
}

template <int DT>
__device__ __forceinline__ f32x2_t z_pair2(const uint8_t* lds, uint32_t r1, uint32_t r2) {
  f32x2_t z;
  if constexpr (DT == FKS_BF16) {
    z = rnd2<DT>(z_pair_bf16_raw(r1, r2));
  } else {
    float z1, z2;
    z_pair<DT>(lds, r1, r2, z1, z2);
    z.x = z1;
    z.y = z2;
  }
  return z;
}

// ------------------------------------------------------------------ torch_rocm stream
// Round 1 of Philox4x32-10 multiplies the COUNTER only (the key enters by xor), so an
// item computes it once for all the seeds of a pass.
struct PhxRound1 {
  uint32_t a0, a2;  // hi(M1 c2) ^ c1, hi(M0 c0) ^ c3: xored with the key halves
  uint32_t c1, c3;  // lo(M1 c2), lo(M0 c0)
};
__device__ __forceinline__ PhxRound1 philox_round1(uint64_t ctr, uint32_t idx) {
  const uint64_t m0 = (uint64_t)0xD2511F53u * (uint32_t)ctr, m1 = (uint64_t)0xCD9E8D57u * idx;
  return PhxRound1{(uint32_t)(m1 >> 32) ^ (uint32_t)(ctr >> 32), (uint32_t)(m0 >> 32), (uint32_t)m1, (uint32_t)m0};
}
__device__ __forceinline__ uint4 philox4x32_10(const PhxRound1& r1, uint64_t seed) {
  // Random123 Philox4x32-10 as rocrand_philox4x32_10.h:270-303 (counter (x, y, z, w) =
  // (ctr lo, ctr hi, subsequence lo, hi), key (seed lo, hi), bumped by the Weyl constants)
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  uint32_t c0 = r1.a0 ^ k0, c1 = r1.c1, c2 = r1.a2 ^ k1, c3 = r1.c3;
  k0 += 0x9E3779B9u;
  k1 += 0xBB67AE85u;
#pragma unroll
  for (int r = 1; r < 10; r++) {
    const uint64_t m0 = (uint64_t)0xD2511F53u * c0, m1 = (uint64_t)0xCD9E8D57u * c2;
    // one v_bitop3_b32 per three-input xor (two v_xor_b32 otherwise)
    const uint32_t n0 = bs::xor3((uint32_t)(m1 >> 32), c1, k0), n2 = bs::xor3((uint32_t)(m0 >> 32), c3, k1);
    c1 = (uint32_t)m1;
    c3 = (uint32_t)m0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return make_uint4(c0, c1, c2, c3);
}

// rocrand_normal.h:53-68 box_muller as torch's ROCm build compiles it (hipcc's default
// fp-contract: the uniforms' multiply-add is one fma): (sin * s, cos * s) -- then torch's
// transformation::normal, val * std + mean with std 1, mean 0 (one fma: -0 becomes +0).
__device__ __forceinline__ float2 rocrand_box_muller(uint32_t x, uint32_t y) {
  const float u = __fmaf_rn((float)x, 2.3283064e-10f, 2.3283064e-10f);
  const float v = __fmaf_rn((float)y, 1.46291807e-09f, 1.46291807e-09f);
  const float s = sqrtf(-2.0f * logf(u));
  float sn, cs;
  __sincosf(v, &sn, &cs);
  return make_float2(__fmaf_rn(sn * s, 1.0f, 0.0f), __fmaf_rn(cs * s, 1.0f, 0.0f));
}

template <int DT>
__device__ __forceinline__ float phx_cast(float v) {  // static_cast<scalar_t>(float)
  return DT == FKS_F32 ? v : Traits<DT>::rnd(v);
}

// Both Box-Muller pairs of one Philox output, (w.x, w.y) and (w.z, w.w), as the
// instructions rocrand_box_muller compiles to, restricted to the inputs Philox can give
// them and with the two pairs' float arithmetic packed (v_pk_*_f32):
//   u = fma(x, 2^-32, 2^-32) lies in [2^-32, 1]: ocml's logf takes its normal-input path
//     -- v_log_f32, then y ln2 in extended precision, r + e with r = RN(y ln2_hi),
//     e = fma(y, ln2_hi, -r) + y ln2_lo -- with no denormal rescaling and no infinity
//     select; the -2 (an exact scaling) is folded into ln2_hi / ln2_lo (RN(-2 a) = -2 RN(a)
//     without underflow; only the sign of a zero can change, and a zero radius becomes +0
//     in the final "+ 0" either way);
//   x = -2 log u is 0 or >= 1.19e-7: the correctly rounded sqrtf takes its unscaled path
//     -- v_sqrt_f32 and the +-1 ulp correction by two fma residuals (sqrt(+-0) = +-0
//     falls out of the correction unchanged, so the +-0 / inf class select is dead);
//   (sin(v) s, cos(v) s) + 0 as one fma with a +0 addend (no product underflows: |s| >=
//     3.4e-4 or s = 0, |sin|, |cos| >= 1e-9 or exactly 0).
// fks_device_selfcheck(FKS_CHECK_PHILOX_RADIUS) compares phx_radius2 with ocml's
// sqrtf(-2 logf(u)) on all 2^32 words; tests/test_gpu_torch_rocm.py the whole stream with
// torch.normal on the device.
// The bf16 fast path's radius: x = RN(log2(u) RN(-2 ln 2)) in ONE rounding instead of
// ocml's extended-precision r + e, then the raw v_sqrt_f32.  Within kPhxFastUlps ulps of
// the exact radius on every one of the 2^32 words (fks_device_selfcheck
// FKS_CHECK_PHILOX_BF16_RADIUS reports the largest distance; tests/test_gpu_selfcheck.py).
constexpr uint32_t kPhxFastUlps = 2;
__device__ __forceinline__ f32x2_t phx_radius2_fast(const f32x2_t u) {
  const f32x2_t y = {__builtin_amdgcn_logf(u.x), __builtin_amdgcn_logf(u.y)};
  const f32x2_t x = y * (f32x2_t){__uint_as_float(0xbfb17218u), __uint_as_float(0xbfb17218u)};  // RN(-2 ln 2)
  return (f32x2_t){__builtin_amdgcn_sqrtf(x.x), __builtin_amdgcn_sqrtf(x.y)};
}

__device__ __forceinline__ f32x2_t phx_radius2(const f32x2_t u) {
  const f32x2_t y = {__builtin_amdgcn_logf(u.x), __builtin_amdgcn_logf(u.y)};
  const f32x2_t m2hi = {__uint_as_float(0xbfb17217u), __uint_as_float(0xbfb17217u)};  // -2 x 0x3f317217
  const f32x2_t m2lo = {__uint_as_float(0xb3f7d1cfu), __uint_as_float(0xb3f7d1cfu)};  // -2 x 0x3377d1cf
  const f32x2_t r = y * m2hi;
  f32x2_t e = __builtin_elementwise_fma(y, m2hi, -r);
  e = __builtin_elementwise_fma(m2lo, y, e);
  const f32x2_t x = r + e;
  f32x2_t sq = {__builtin_amdgcn_sqrtf(x.x), __builtin_amdgcn_sqrtf(x.y)};
  const f32x2_t sm = {__int_as_float(__float_as_int(sq.x) - 1), __int_as_float(__float_as_int(sq.y) - 1)};
  const f32x2_t sp = {__int_as_float(__float_as_int(sq.x) + 1), __int_as_float(__float_as_int(sq.y) + 1)};
  const f32x2_t rm = __builtin_elementwise_fma(-sm, sq, x), rp = __builtin_elementwise_fma(-sp, sq, x);
  sq.x = rm.x <= 0.0f ? sm.x : sq.x;
  sq.y = rm.y <= 0.0f ? sm.y : sq.y;
  sq.x = rp.x > 0.0f ? sp.x : sq.x;
  sq.y = rp.y > 0.0f ? sp.y : sq.y;
  return sq;
}

template <bool kFast = false>  // kFast: the bf16 fast path's radius (phx_radius2_fast)
__device__ __forceinline__ void phx_box_muller2(const uint4 w, f32x2_t& zA, f32x2_t& zB) {
  const f32x2_t cu = {2.3283064e-10f, 2.3283064e-10f}, cv = {1.46291807e-09f, 1.46291807e-09f};
  const f32x2_t fx = {(float)w.x, (float)w.z}, fy = {(float)w.y, (float)w.w};
  const f32x2_t u = __builtin_elementwise_fma(fx, cu, cu);
  const f32x2_t sq = kFast ? phx_radius2_fast(u) : phx_radius2(u);
  const f32x2_t v = __builtin_elementwise_fma(fy, cv, cv);
  const f32x2_t rev = v * (f32x2_t){__uint_as_float(0x3e22f983u), __uint_as_float(0x3e22f983u)};  // 1/(2 pi)
  const f32x2_t sc1 = {__builtin_amdgcn_sinf(rev.x), __builtin_amdgcn_cosf(rev.x)};
  const f32x2_t sc2 = {__builtin_amdgcn_sinf(rev.y), __builtin_amdgcn_cosf(rev.y)};
  const f32x2_t zero = {0.0f, 0.0f};
  zA = __builtin_elementwise_fma(sc1, (f32x2_t){sq.x, sq.x}, zero);
  zB = __builtin_elementwise_fma(sc2, (f32x2_t){sq.y, sq.y}, zero);
}

// The four z of one Philox output rounded to bf16.  Only the bf16 value matters here, so
// the radius's +-1 ulp correction (a third of phx_radius2's instructions) is skipped
// unless it could change it: with the root within 1 ulp, z = (sin or cos) s moves by at
// most 3 f32 ulps, which changes the bf16 rounding only for a product within 3 ulps of a
// rounding midpoint (low 16 bits 0x8000; across a binade both round to the power of two).
// Lanes with any of their four products within 4 ulps of one redo the pair exactly (about
// 3.5 % of the waves' iterations branch).
// Window half-width W in f32 ulps around a bf16 rounding midpoint: a radius within k ulps
// of the exact one moves z = RN(sc s) by at most 2k + 1 ulps (|sc| <= 1, the product's
// ulp at most twice sc's ulp times s's), so W = 2k + 2: k = 1 for the raw root of the
// exact x (W = 4), k = kPhxFastUlps for the one-rounding x (phx_radius2_fast,
// the form in use).
constexpr uint32_t kPhxMidW = 2 * kPhxFastUlps + 2;
__device__ __forceinline__ bool phx_near_bf16_mid(float z) {
  return ((__float_as_uint(z) & 0xFFFFu) - (0x8000u - kPhxMidW)) <= 2 * kPhxMidW;
}
__device__ __forceinline__ void phx_z_bf16(const uint4 w, f32x2_t& zA, f32x2_t& zB) {
  phx_box_muller2</*kFast=*/true>(w, zA, zB);
  const bool near = (int)phx_near_bf16_mid(zA.x) | (int)phx_near_bf16_mid(zA.y) | (int)phx_near_bf16_mid(zB.x) |
                    (int)phx_near_bf16_mid(zB.y);
  if (__builtin_expect(near, 0)) phx_box_muller2(w, zA, zB);  // the corrected radius
  zA = rnd2<FKS_BF16>(zA);
  zB = rnd2<FKS_BF16>(zB);
}

// the radius of one word as ocml computes it (the reference's instructions), for the
// self check of phx_radius2
__device__ __forceinline__ float phx_radius_ocml(uint32_t x) {
  return sqrtf(-2.0f * logf(__fmaf_rn((float)x, 2.3283064e-10f, 2.3283064e-10f)));
}

}  // namespace
}  // namespace fks
