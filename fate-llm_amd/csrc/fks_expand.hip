// fks_expand.hip -- seed-basis expansion on the torch_rocm stream (include/fks.h
// fks_expand_multi): out_m = cast(beta_m out_m + sum_s f32(c[m][s]) z_s), the dense vector Z c of
// (seed, scalar) pairs, written where the caller's tensors lie and in their dtype; the other
// direction of fks_project_multi (Z^T v) and fks_delta_accumulate's sum without its f32 buffer.
//
// fks_expand_multi_kernel<NV> walks the work items of the geometry-only PhxTensor table as
// fks_project_multi_kernel does: a thread takes a GROUP of kExpVec consecutive items (idx0 ..
// idx0 + 7 of one row j), 32 elements in four 8-element runs; a wave's 64 groups are consecutive
// and their tensor is looked up with wave-uniform indices in the LDS copy of the table.  Per group
// the 32 sums of each of the NV outputs live in registers, +0 at the start, and ALL the seeds of
// the call run in order: eight Philox4x32-10 calls (round 1, which multiplies the counter only,
// hoisted out of the seed loop), the four z of each in the tensor's dtype -- the values fks_normal
// writes --, and per output one f32 fma per element, acc = fma(c, z, acc), packed in pairs
// (v_pk_fma_f32): fks_delta_accumulate's chain with no store in between.  Seeds and coefficients
// come from a device table ([k] u64, [k][NV] f32) read with wave-uniform indices through the
// constant address space: scalar loads.  Then the epilogue: with beta != 0 the old output is read
// and widened (exact) and out = cast(fma(beta, old, acc)), else out = cast(acc) and nothing is
// read; whole 16-byte runs where the output's piece is 16-byte aligned and the four runs lie
// inside the tensor (two stores per f32 run, one per 2-byte run), per element otherwise (a
// tensor's last row, an unaligned output), never past the tensor's end.  No element depends on
// another: a result does not depend on the grid, the launch cuts or the batching of outputs.
//
// Compiler report (-Rpass-analysis=kernel-resource-usage, gfx950, 256-thread workgroups):
//   NV 1: 109 VGPRs, 0 AGPRs, 0 B scratch, 4 waves per SIMD
//   NV 2: 141 VGPRs, 0 AGPRs, 0 B scratch, 3 waves per SIMD
//   NV 3: 173 VGPRs, 0 AGPRs, 0 B scratch, 2 waves per SIMD
//   NV 4: 205 VGPRs, 0 AGPRs, 0 B scratch, 2 waves per SIMD
// (32 accumulators per output on top of the generator's 77; the seed and coefficient loads of the
// seed loop are s_load_dwordx2 / s_load_dword, the fmas v_pk_fma_f32)
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fks_expand.h"
#include "fks_dev_zgen.h"

namespace fks {
namespace {

constexpr int kExpVec = 8;  // work items per thread (fks_kern_philox.h kPhxVec)
constexpr int kExpThreads = 256;
// A/B switches (make variant_expand NAME=x DEFS="-D..."; tools/expand_rate.py times them)
#ifndef FKS_EXP_WG_PER_CU   // grid cap: workgroups per CU, as fks_project_kernel's
#define FKS_EXP_WG_PER_CU 16
#endif
#ifndef FKS_EXP_SCHED_FENCE   // 1: a scheduling barrier after each of a group's eight items for NV >= 2, so that
#define FKS_EXP_SCHED_FENCE 1 // one item's generator is live at a time (fks_project_multi_kernel's device)
#endif
constexpr int kExpWgPerCu = FKS_EXP_WG_PER_CU;
constexpr int kExpLdsTensors = 512;  // tables of at most this many entries are copied to LDS

typedef __attribute__((address_space(1))) u32x4_t exp_gu128;
typedef __attribute__((address_space(1))) float exp_gf32;
typedef __attribute__((address_space(1))) uint16_t exp_gu16;
// the call's seed table is written before the launch and never during it: constant address space
typedef __attribute__((address_space(4))) const uint64_t exp_cu64;
typedef __attribute__((address_space(4))) const float exp_cf32;

// the last table entry whose first item is <= it, at or after lo (fks_project.hip proj_find_t)
template <class Tab>
__device__ __forceinline__ int exp_find_t(Tab tab, int nt, int64_t it, int lo, int probes) {
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

// a bf16 / f16 element widened to f32 (exact)
__device__ __forceinline__ float exp_widen(uint32_t h, bool bf) {
  const _Float16 f = __builtin_bit_cast(_Float16, (uint16_t)h);
  return bf ? __uint_as_float(h << 16) : (float)f;
}
// the 16 bits of v rounded to nearest even to bf16 / f16.  (Traits<FKS_F16>::rnd pins v as an f32
// value first: the fma that produced it is rounded to f32, then to f16, as the contract says.)
__device__ __forceinline__ uint32_t exp_bits16(float v, bool bf) {
  const uint32_t b = __float_as_uint(rbf_cvt(v)) >> 16;
  const uint32_t h = Traits<FKS_F16>::bits(Traits<FKS_F16>::rnd(v));
  return bf ? b : h;
}

// Every seed of the call over one group of a tensor that draws dtype DT: acc[m][i][q] is output
// m's sum for element idx0 + q + S (4 j + i), kept as the pairs (i = 0, 1) and (i = 2, 3).
template <int DT, int NV>
__device__ __forceinline__ void exp_seeds(const ExpandArgs& a, uint64_t ctr, uint32_t idx0,
                                          f32x2_t (&accA)[NV][kExpVec], f32x2_t (&accB)[NV][kExpVec]) {
  exp_cu64* const seeds = (exp_cu64*)a.seeds;
  exp_cf32* const coef = (exp_cf32*)a.coef;
  PhxRound1 r1[kExpVec];
#pragma unroll
  for (int q = 0; q < kExpVec; q++) r1[q] = philox_round1(ctr, idx0 + (uint32_t)q);
  for (int s = 0; s < a.nseeds; s++) {
    const uint64_t seed = seeds[s];  // wave-uniform: scalar loads
    f32x2_t c[NV];
#pragma unroll
    for (int m = 0; m < NV; m++) {
      const float x = coef[(size_t)s * NV + m];
      c[m] = (f32x2_t){x, x};
    }
#pragma unroll
    for (int q = 0; q < kExpVec; q++) {
      const uint4 w = philox4x32_10(r1[q], seed);
      f32x2_t zA, zB;
      if constexpr (DT == FKS_BF16) {
        phx_z_bf16(w, zA, zB);
      } else {
        phx_box_muller2(w, zA, zB);
        zA = (f32x2_t){phx_cast<DT>(zA.x), phx_cast<DT>(zA.y)};
        zB = (f32x2_t){phx_cast<DT>(zB.x), phx_cast<DT>(zB.y)};
      }
#pragma unroll
      for (int m = 0; m < NV; m++) {  // fks_delta_accumulate's fma (apply_pair<DT, kModeDelta>)
        accA[m][q] = __builtin_elementwise_fma(c[m], zA, accA[m][q]);
        accB[m][q] = __builtin_elementwise_fma(c[m], zB, accB[m][q]);
      }
#if FKS_EXP_SCHED_FENCE
      if constexpr (NV > 1) __builtin_amdgcn_sched_barrier(0);  // one item's generator at a time
#endif
    }
  }
}

// One output's 32 elements of a group: v[i][q] = the sum for element e0 + S i + q of the table
// entry (numel elements), E the output's piece for that entry.
__device__ __forceinline__ void exp_store(const ProjVecEntry& E, int64_t numel, int64_t S, int64_t e0, float beta,
                                          bool read_old, float (&v)[4][kExpVec]) {
  const bool whole = (E.flags & kPhxP16) && e0 + 3 * S + kExpVec <= numel;
  if (E.dtype == FKS_F32) {
    if (whole) {
#pragma unroll
      for (int i = 0; i < 4; i++) {
        exp_gu128* p = reinterpret_cast<exp_gu128*>(E.ptr + (uint64_t)(e0 + S * i) * 4u);
        if (read_old) {
          const u32x4_t x = p[0], y = p[1];
          const uint32_t w[kExpVec] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
#pragma unroll
          for (int q = 0; q < kExpVec; q++) v[i][q] = __fmaf_rn(beta, __uint_as_float(w[q]), v[i][q]);
        }
        p[0] = (u32x4_t){__float_as_uint(v[i][0]), __float_as_uint(v[i][1]), __float_as_uint(v[i][2]),
                         __float_as_uint(v[i][3])};
        p[1] = (u32x4_t){__float_as_uint(v[i][4]), __float_as_uint(v[i][5]), __float_as_uint(v[i][6]),
                         __float_as_uint(v[i][7])};
      }
      return;
    }
    exp_gf32* p = reinterpret_cast<exp_gf32*>(E.ptr);
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int q = 0; q < kExpVec; q++) {
        const int64_t e = e0 + S * i + q;
        if (e < numel) p[e] = read_old ? __fmaf_rn(beta, p[e], v[i][q]) : v[i][q];
      }
    return;
  }
  const bool bf = E.dtype == FKS_BF16;
  if (whole) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      exp_gu128* p = reinterpret_cast<exp_gu128*>(E.ptr + (uint64_t)(e0 + S * i) * 2u);
      if (read_old) {
        const u32x4_t x = p[0];
        const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int q = 0; q < 4; q++) {
          v[i][2 * q] = __fmaf_rn(beta, exp_widen(w[q] & 0xFFFFu, bf), v[i][2 * q]);
          v[i][2 * q + 1] = __fmaf_rn(beta, exp_widen(w[q] >> 16, bf), v[i][2 * q + 1]);
        }
      }
      uint32_t w[4];
#pragma unroll
      for (int q = 0; q < 4; q++) w[q] = exp_bits16(v[i][2 * q], bf) | (exp_bits16(v[i][2 * q + 1], bf) << 16);
      p[0] = (u32x4_t){w[0], w[1], w[2], w[3]};
    }
    return;
  }
  exp_gu16* p = reinterpret_cast<exp_gu16*>(E.ptr);
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int q = 0; q < kExpVec; q++) {
      const int64_t e = e0 + S * i + q;
      if (e < numel) {
        const float x = read_old ? __fmaf_rn(beta, exp_widen(p[e], bf), v[i][q]) : v[i][q];
        p[e] = (uint16_t)exp_bits16(x, bf);
      }
    }
}

template <int NV, class Tab>
__device__ __forceinline__ void exp_walk(const ExpandArgs& a, Tab tab) {
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t step = (int64_t)gridDim.x * kExpThreads * kExpVec;
  int64_t wb = rfl64(a.item_lo + ((int64_t)blockIdx.x * kExpThreads + (int64_t)(threadIdx.x & ~63u)) * kExpVec);
  int ts = 0;
  for (; wb < a.item_hi; wb += step) {  // wb and the loop are wave-uniform
    ts = __builtin_amdgcn_readfirstlane(exp_find_t(tab, a.nt, wb, ts, 2));
    const int64_t wend = wb + 64 * kExpVec < a.item_hi ? wb + 64 * kExpVec : a.item_hi;
    const bool one = ts + 1 >= a.nt || tab[ts + 1].item0 >= wend;  // the whole wave in tensor ts
    const int64_t it = wb + (int64_t)lane * kExpVec;
    if (it >= a.item_hi) continue;
    const int ti = one ? ts : exp_find_t(tab, a.nt, it, ts, 0);
    const PhxTensor T = tab[ti];
    const int64_t S = (int64_t)T.stride;
    const int64_t r0 = it - T.item0;
    const uint32_t idx0 = (uint32_t)(r0 % S);
    const uint64_t j = (uint64_t)(r0 / S);
    f32x2_t accA[NV][kExpVec], accB[NV][kExpVec];
#pragma unroll
    for (int m = 0; m < NV; m++)
#pragma unroll
      for (int q = 0; q < kExpVec; q++) accA[m][q] = accB[m][q] = (f32x2_t){0.0f, 0.0f};
    switch (T.dtype) {
      case FKS_F32: exp_seeds<FKS_F32, NV>(a, T.off4 + j, idx0, accA, accB); break;
      case FKS_BF16: exp_seeds<FKS_BF16, NV>(a, T.off4 + j, idx0, accA, accB); break;
      default: exp_seeds<FKS_F16, NV>(a, T.off4 + j, idx0, accA, accB); break;
    }
    const int64_t e0 = (int64_t)idx0 + S * (int64_t)(4 * j);
#pragma unroll
    for (int m = 0; m < NV; m++) {
      const ProjVecEntry E = a.ot[(size_t)m * (size_t)a.nt + (size_t)ti];
      float v[4][kExpVec];
#pragma unroll
      for (int q = 0; q < kExpVec; q++) {
        v[0][q] = accA[m][q].x;
        v[1][q] = accA[m][q].y;
        v[2][q] = accB[m][q].x;
        v[3][q] = accB[m][q].y;
      }
      exp_store(E, T.numel, S, e0, a.beta[m], ((a.read_old >> m) & 1) != 0, v);
    }
  }
}

template <int NV>
__global__ __launch_bounds__(kExpThreads) void fks_expand_multi_kernel(ExpandArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_exp[];
  PhxTensor* s_tab = reinterpret_cast<PhxTensor*>(s_exp);
  if (a.nt <= kExpLdsTensors) {
    constexpr int W = (int)(sizeof(PhxTensor) / 4);
    for (int i = (int)threadIdx.x; i < a.nt * W; i += kExpThreads)
      reinterpret_cast<uint32_t*>(s_tab)[i] = reinterpret_cast<const uint32_t*>(a.t)[i];
    __syncthreads();
    exp_walk<NV>(a, (const PhxTensor*)s_tab);
  } else {
    exp_walk<NV>(a, a.t);
  }
}

template <int NV>
void expand_launch(const ExpandArgs& a, unsigned grid, size_t lds, hipStream_t stream) {
  hipLaunchKernelGGL(fks_expand_multi_kernel<NV>, dim3(grid), dim3(kExpThreads), lds, stream, a);
}

}  // namespace

int launch_expand_multi(const ExpandArgs& a, void* stream) {
  static_assert(kExpMaxVec == 4, "one instance per output count");
  const int64_t items = a.item_hi - a.item_lo;
  if (a.nseeds < 0 || a.nt < 1 || items <= 0 || !a.t || !a.ot || a.nvec < 1 || a.nvec > kExpMaxVec ||
      (a.nseeds > 0 && (!a.seeds || !a.coef)))
    return -FKS_EINVAL;
  // groups never straddle a tensor or a cut: every row boundary is a multiple of 256 items
  if (a.item_lo % kExpVec != 0 || items % kExpVec != 0) return -FKS_EINVAL;
  const int64_t groups = items / kExpVec;
  const int64_t want = (groups + kExpThreads - 1) / kExpThreads;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)kExpWgPerCu * device_cu_count()));
  const size_t lds = a.nt <= kExpLdsTensors ? sizeof(PhxTensor) * (size_t)a.nt : 0;
  switch (a.nvec) {
    case 1: expand_launch<1>(a, grid, lds, (hipStream_t)stream); break;
    case 2: expand_launch<2>(a, grid, lds, (hipStream_t)stream); break;
    case 3: expand_launch<3>(a, grid, lds, (hipStream_t)stream); break;
    default: expand_launch<4>(a, grid, lds, (hipStream_t)stream); break;
  }
  return (int)hipGetLastError();
}

}  // namespace fks
