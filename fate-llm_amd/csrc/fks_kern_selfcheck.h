// fks_kern_selfcheck.h -- the device self-check kernels (fks_device_selfcheck): exhaustive
// checks of the fp32 radius square root and of the torch_rocm stream's radius forms.
#pragma once
#include <hip/hip_runtime.h>

#include "fks_internal.h"
#include "fks_dev_zgen.h"

namespace fks {

// Device self check FKS_CHECK_SQRT_DOMAIN: for every u1 = 1 - k 2^-24 the fp32
// Box-Muller can draw, x = -2 cephes_logf(u1); counts the k where radius_sqrt(x) is not
// the correctly rounded square root.  The criterion is exact and uses no square root:
// s = RN(sqrt(x)) iff m_lo^2 < x < m_hi^2 for the midpoints m to s's neighbours (25-bit
// values, squared exactly in double; a 24-bit x never equals such a square).  One count
// per workgroup of 256.
__global__ __launch_bounds__(256) void fks_sqrt_domain_kernel(uint32_t* counts) {
  __shared__ uint32_t bad;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  const float x = -2.0f * cephes_logf(1.0f - (float)k * (1.0f / 16777216.0f));
  const float s = radius_sqrt(x);
  bool ok;
  if (x > 0.0f) {
    const double sd = (double)s;
    const double lo = 0.5 * (sd + (double)__int_as_float(__float_as_int(s) - 1));
    const double hi = 0.5 * (sd + (double)__int_as_float(__float_as_int(s) + 1));
    ok = lo * lo < (double)x && (double)x < hi * hi;
  } else {
    ok = __float_as_uint(s) == __float_as_uint(x);  // sqrt(+-0) = +-0
  }
  if (!ok) atomicAdd(&bad, 1u);
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = bad;
}

// Device self check FKS_CHECK_PHILOX_RADIUS: the torch_rocm stream's radius
// (phx_radius2, the trimmed logf + correctly rounded sqrtf) against ocml's general
// sqrtf(-2 logf(u)) -- the reference's instructions -- on every one of the 2^32 Philox
// words, bit for bit except the sign of a zero radius (the "+ 0" that follows erases
// it).  kSqrtDomainBlocks workgroups of 256, 256 words per thread, one count each.
__global__ __launch_bounds__(256) void fks_philox_radius_kernel(uint32_t* counts) {
  __shared__ uint32_t bad;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  uint32_t n = 0;
  const uint32_t base = (blockIdx.x * 256u + threadIdx.x) * 256u;
  for (uint32_t i = 0; i < 256u; i += 2) {
    const uint32_t x0 = base + i, x1 = base + i + 1;
    const f32x2_t u = {__fmaf_rn((float)x0, 2.3283064e-10f, 2.3283064e-10f),
                       __fmaf_rn((float)x1, 2.3283064e-10f, 2.3283064e-10f)};
    const f32x2_t s = phx_radius2(u);
    const float r0 = phx_radius_ocml(x0), r1 = phx_radius_ocml(x1);
    n += (__float_as_uint(s.x + 0.0f) != __float_as_uint(r0 + 0.0f)) ? 1u : 0u;
    n += (__float_as_uint(s.y + 0.0f) != __float_as_uint(r1 + 0.0f)) ? 1u : 0u;
  }
  if (n) atomicAdd(&bad, n);
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = bad;
}

// Device self check FKS_CHECK_PHILOX_BF16_RADIUS: the largest distance, in f32 ulps, of
// the bf16 fast path's radius (phx_radius2_fast) from ocml's sqrtf(-2 logf(u)) over all
// 2^32 words (both are >= +0, so the distance is the difference of the bit patterns);
// one maximum per workgroup.
__global__ __launch_bounds__(256) void fks_philox_fast_radius_kernel(uint32_t* counts) {
  __shared__ uint32_t worst;
  if (threadIdx.x == 0) worst = 0;
  __syncthreads();
  uint32_t m = 0;
  const uint32_t base = (blockIdx.x * 256u + threadIdx.x) * 256u;
  for (uint32_t i = 0; i < 256u; i += 2) {
    const uint32_t x0 = base + i, x1 = base + i + 1;
    const f32x2_t u = {__fmaf_rn((float)x0, 2.3283064e-10f, 2.3283064e-10f),
                       __fmaf_rn((float)x1, 2.3283064e-10f, 2.3283064e-10f)};
    const f32x2_t s = phx_radius2_fast(u);
    const uint32_t a0 = __float_as_uint(s.x + 0.0f), b0 = __float_as_uint(phx_radius_ocml(x0) + 0.0f);
    const uint32_t a1 = __float_as_uint(s.y + 0.0f), b1 = __float_as_uint(phx_radius_ocml(x1) + 0.0f);
    m = max(m, max(a0 > b0 ? a0 - b0 : b0 - a0, a1 > b1 ? a1 - b1 : b1 - a1));
  }
  atomicMax(&worst, m);
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = worst;
}

}  // namespace fks
