// fks_dev_lds.h -- the packed f32 pair type, the adjacent-lane exchange, and the LDS and
// readfirstlane accessors of the gfx950 kernels.  Part of the one device translation unit
// (fks_device.hip includes the fks_dev_*.h layers, then the fks_kern_*.h kernel families).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fks {
namespace {

typedef float f32x2_t __attribute__((ext_vector_type(2)));

// value of the adjacent lane (lane ^ 1): DPP quad_perm [1,0,3,2]
__device__ __forceinline__ uint32_t swap_adjacent(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false);
}

// sum of x over the 64 lanes of the wave, in every lane: the xor butterfly, one fixed order
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
  return x;
}

// ------------------------------------------------------------------ LDS accessors
// LDS accessors by byte offset.  The apply kernel's only LDS is its dynamic block,
// which starts at LDS address 0 (no static __shared__; checked at kernel entry), so an
// offset IS the address: immediates fold into ds_read/ds_write and no base add is
// spent per access.
typedef __attribute__((address_space(3))) uint32_t lds_u32_t;
typedef __attribute__((address_space(3))) uint64_t lds_u64_t;
typedef __attribute__((address_space(3))) float lds_f32_t;
typedef __attribute__((address_space(3))) f32x2_t lds_f32x2_t;
__device__ __forceinline__ uint32_t lds_u32(int off) { return *(const lds_u32_t*)(size_t)off; }
__device__ __forceinline__ uint64_t lds_u64(int off) { return *(const lds_u64_t*)(size_t)off; }
__device__ __forceinline__ void lds_st(int off, uint32_t v) { *(lds_u32_t*)(size_t)off = v; }
__device__ __forceinline__ float lds_f32(uint32_t off) { return *(const lds_f32_t*)(size_t)off; }
__device__ __forceinline__ f32x2_t lds_f32x2(uint32_t off) { return *(const lds_f32x2_t*)(size_t)off; }

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) u32x4_t lds_u4_t;
__device__ __forceinline__ u32x4_t lds_u4(uint32_t off) { return *(const lds_u4_t*)(size_t)off; }
__device__ __forceinline__ void lds_st4(uint32_t off, u32x4_t v) { *(lds_u4_t*)(size_t)off = v; }

// ------------------------------------------------------------------ readfirstlane
__device__ __forceinline__ uint32_t rfl(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t rfl64(uint64_t v) {
  return (uint64_t)rfl((uint32_t)v) | ((uint64_t)rfl((uint32_t)(v >> 32)) << 32);
}
__device__ __forceinline__ float rflf(float v) { return __uint_as_float(rfl(__float_as_uint(v))); }
__device__ __forceinline__ int64_t rfl64(int64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

}  // namespace
}  // namespace fks
