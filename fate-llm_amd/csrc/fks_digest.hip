// fks_digest.hip -- FKSD-1, the model fingerprint (include/fks.h fks_digest): one streaming
// read of the parameters a reconstruct has just written.
//
// Element e of tensor i sits at position q = pos0 + (numel of the tensors before i) + e of
// the list laid end to end; with b its raw bits (16 or 32, zero-extended) and all
// arithmetic mod 2^64
//     x = ((q + 1) * G) ^ b,   z = splitmix64's finaliser of x,
//     digest = (sum of z, xor of z).
// Both combiners are associative and commutative, so the result depends neither on the
// grid nor on the arrival order of the blocks' atomics, and digests of disjoint element
// ranges combine by (add, xor).
//
// Work decomposition: every non-empty tensor is cut into TILES of kDigVecPerTile 16-byte
// vectors of its 16-byte aligned body; a wave takes one tile at a time (grid-stride) and
// finds the tile's tensor with wave-uniform indices in the table that travels by value
// in the kernel arguments (scalar loads; no device table, no workspace).  The elements
// before the first aligned vector and after the last whole one (fewer than 16 bytes
// each) are hashed one per lane by the tensor's first tile.  Per lane, then per wave
// (cross-lane shuffles), then per block (LDS); one 64-bit integer atomic add and one
// atomic xor per block, at device scope.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fks_internal.h"

namespace fks {
namespace {

// the parameters are global memory (global_load, not flat)
typedef __attribute__((address_space(1))) const uint8_t dig_gu8;
typedef __attribute__((address_space(1))) const uint16_t dig_gu16;
typedef __attribute__((address_space(1))) const uint32_t dig_gu32;
typedef uint32_t dig_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const dig_u32x4 dig_gu32x4;

constexpr uint64_t kDigG = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kDigM1 = 0xBF58476D1CE4E5B9ull;
constexpr uint64_t kDigM2 = 0x94D049BB133111EBull;

__device__ __forceinline__ uint64_t dig_mix(uint64_t x) {
  uint64_t z = (x ^ (x >> 30)) * kDigM1;
  z = (z ^ (z >> 27)) * kDigM2;
  return z ^ (z >> 31);
}

struct DigAcc {
  uint64_t sum = 0, xr = 0;
  __device__ __forceinline__ void add(uint64_t pg, uint32_t bits) {
    const uint64_t z = dig_mix(pg ^ (uint64_t)bits);
    sum += z;
    xr ^= z;
  }
};

// the tensor's split into [head elements | nv aligned vectors | tail elements]
struct DigSplit {
  int64_t head, nv, tail;
};
template <int ES>
__device__ __forceinline__ DigSplit dig_split(uint64_t ptr, int64_t numel) {
  constexpr int EPV = 16 / ES;
  const int64_t to16 = (int64_t)(((16u - (uint32_t)(ptr & 15u)) & 15u) / (uint32_t)ES);
  DigSplit s;
  s.head = to16 < numel ? to16 : numel;
  s.nv = (numel - s.head) / EPV;
  s.tail = numel - s.head - s.nv * EPV;
  return s;
}

// One tile of tensor T: vectors [tile * kDigVecPerTile, ...) of its body, plus, for tile 0,
// its head (lanes 0..7) and tail (lanes 8..15) elements.  ES = bytes per element.
template <int ES>
__device__ __forceinline__ void dig_tile(const DigestTensor& T, int64_t tile, int lane, DigAcc& acc) {
  constexpr int EPV = 16 / ES;
  const DigSplit S = dig_split<ES>(T.ptr, T.numel);
  dig_gu8* base = (dig_gu8*)T.ptr;
  if (tile == 0) {
    // element index of this lane's head / tail element, or -1
    int64_t e = -1;
    if (lane < 8) {
      if (lane < S.head) e = lane;
    } else if (lane < 16) {
      if (lane - 8 < S.tail) e = S.head + S.nv * EPV + (lane - 8);
    }
    if (e >= 0) {
      uint32_t b;
      if constexpr (ES == 2) b = *(dig_gu16*)(base + 2 * e);
      else b = *(dig_gu32*)(base + 4 * e);
      acc.add((T.q1 + (uint64_t)e) * kDigG, b);
    }
  }
  dig_gu32x4* body = (dig_gu32x4*)(base + (size_t)S.head * ES);
  const int64_t v0 = tile * kDigVecPerTile + lane;
  dig_u32x4 w[kDigUnroll];
#pragma unroll
  for (int u = 0; u < kDigUnroll; u++) {
    const int64_t v = v0 + 64 * u;
    w[u] = v < S.nv ? body[v] : dig_u32x4{0u, 0u, 0u, 0u};
  }
  // (q + 1) * G of the lane's first element, then advanced by additions only
  uint64_t pg = (T.q1 + (uint64_t)(S.head + v0 * EPV)) * kDigG;
#pragma unroll
  for (int u = 0; u < kDigUnroll; u++) {
    if (v0 + 64 * u < S.nv) {
      const uint32_t d[4] = {w[u].x, w[u].y, w[u].z, w[u].w};
#pragma unroll
      for (int j = 0; j < EPV; j++) {
        const uint32_t b = ES == 2 ? ((d[j >> 1] >> (16 * (j & 1))) & 0xFFFFu) : d[j];
        acc.add(pg + (uint64_t)j * kDigG, b);
      }
    }
    pg += (uint64_t)(64 * EPV) * kDigG;
  }
}

__device__ __forceinline__ uint64_t dig_shfl_xor(uint64_t v, int m) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
  return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(kDigThreads) void fks_digest_kernel(DigestArgs a) {
  __shared__ uint64_t s_sum[kDigThreads / 64], s_xor[kDigThreads / 64];
  const int lane = (int)(threadIdx.x & 63u);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  constexpr int kWaves = kDigThreads / 64;
  DigAcc acc;
  int ti = 0;  // tiles only grow: the search starts at the previous tile's tensor
  const int64_t step = (int64_t)gridDim.x * kWaves;
  for (int64_t w = (int64_t)blockIdx.x * kWaves + wave; w < a.ntiles; w += step) {
    // the last tensor whose first tile is <= w (wave-uniform: scalar loads of the arguments)
    if (ti + 1 < a.nt && a.t[ti + 1].tile0 <= w) {
      int lo = ti + 1, hi = a.nt - 1;
      if (lo < hi && a.t[lo + 1].tile0 <= w) {  // not the next one either: bisect
        ++lo;
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (a.t[mid].tile0 <= w) lo = mid; else hi = mid - 1;
        }
      }
      ti = lo;
    }
    ti = __builtin_amdgcn_readfirstlane(ti);
    const DigestTensor T = a.t[ti];
    if (T.dtype == FKS_F32) dig_tile<4>(T, w - T.tile0, lane, acc);
    else dig_tile<2>(T, w - T.tile0, lane, acc);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    acc.sum += dig_shfl_xor(acc.sum, m);
    acc.xr ^= dig_shfl_xor(acc.xr, m);
  }
  if (lane == 0) {
    s_sum[wave] = acc.sum;
    s_xor[wave] = acc.xr;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t s = 0, x = 0;
#pragma unroll
    for (int i = 0; i < kWaves; i++) {
      s += s_sum[i];
      x ^= s_xor[i];
    }
    // identities of the two combiners: nothing to add
    if (s) __hip_atomic_fetch_add(&a.out[0], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (x) __hip_atomic_fetch_xor(&a.out[1], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace

int launch_digest(const DigestArgs& a, void* stream) {
  if (a.nt <= 0 || a.ntiles <= 0) return 0;
  constexpr int kWaves = kDigThreads / 64;
  const int64_t want = (a.ntiles + kWaves - 1) / kWaves;
  const int64_t blocks = std::min<int64_t>(want, (int64_t)kDigWgPerCu * device_cu_count());
  hipLaunchKernelGGL(fks_digest_kernel, dim3((unsigned)blocks), dim3(kDigThreads), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // namespace fks
