// fks_project.hip -- seed-basis projection on the torch_rocm stream (include/fks.h
// fks_project): out[s] = <vec, z_s> over the elements one element shard owns, the adjoint of
// fks_delta_accumulate (delta = Z c; this is Z^T v).
//
// fks_project_kernel walks the work items of the call's PhxTensor table (fks_internal.h; the
// table of a kModeDelta call, whose entries point into the f32 vector) as
// fks_philox_vec_kernel does: a thread takes a GROUP of kProjVec consecutive items (idx0 ..
// idx0 + 7 of one row j), 32 elements that lie in four 8-element runs of the vector; a
// wave's 64 groups are consecutive and their tensor is looked up with wave-uniform indices
// from the LDS copy of the table.  Per group the seeds of the pass run in order: eight
// Philox4x32-10 calls (round 1, which multiplies the counter only, computed once per item
// for all the seeds), the four z of each in the tensor's dtype -- the values fks_normal
// writes --, and 32 products (double)v * (double)z, each EXACT (24 + 24 significand bits),
// summed into one f64 partial by fma (one rounding per addition).
//
// The reduction uses no floating-point atomic and has one fixed order: the group partial of
// seed k is summed over the wave by an xor butterfly (every lane ends with the same bits;
// lanes without a group, or whose group belongs to another dtype's pass, enter +0), lane k
// adds the wave's total to its running sum, so a wave carries one f64 per seed instead of
// 32 per lane; at the end the block's waves are added in wave order through LDS into
// partial[block][k], and fks_project_reduce_kernel adds the blocks' partials in block order.
// The grid is a function of the device and the item range only, so a call's result depends
// on the device, the tensor list, the shard and the seeds, and on nothing else.
//
// fks_project_multi_kernel<NV> (include/fks.h fks_project_multi) is the same walk over NV
// vectors at once, each read where it lies: the table is the geometry-only one and a second
// table (ProjVecEntry, [NV][nt]) names every vector's piece per table entry and its dtype
// (f32, bf16 or f16, widened to f32 exactly when loaded).  Per seed the eight Philox calls
// and the 32 z are computed once; every vector runs its own fma chain, in fks_project's
// order, into its own partial, and the reduction carries NV sums per seed (LDS
// [NV][kProjWaves][kPhxSeeds], partial[block][NV][kPhxSeeds]).  The walk, the seed loop and
// the block's reduction are templates on NV and on the vector-fetch policy; fks_project_kernel
// is their NV = 1, one-f32-buffer instance (156 VGPRs, no spill, as before the templates).
//
// fks_gram_kernel<NR> (include/fks.h fks_gram, fks_gram.h) is fks_project_multi_kernel<NR> with a
// third fetch policy, ProjFetchDraw: the NR vectors of a group are not loaded but drawn, vector m
// being the z of row seed m in the lane's tensor dtype.  Everything after the fetch -- the column
// seeds' loop, the chains, the butterfly, the block's reduction -- is the projection's own code, so
// <z_r, z_c> is, bit for bit, the projection of z_r on seed c (219 VGPRs, no scratch, two waves
// per SIMD).  fks_gram_reduce_kernel is the reduce with the matrix's addressing and the mirror.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fks_internal.h"
#include "fks_gram.h"
#include "fks_dev_zgen.h"

namespace fks {
namespace {

constexpr int kProjVec = 8;           // work items per thread (fks_kern_philox.h kPhxVec)
constexpr int kProjThreads = 256;
constexpr int kProjWaves = kProjThreads / 64;
// A/B switches (make variant_project NAME=x DEFS="-D..."; profiles/r08_project_ab.log has the runs):
#ifndef FKS_PROJ_WG_PER_CU   // grid cap: workgroups per CU, as fks_philox_vec_kernel's.  7B bf16 layout, one
#define FKS_PROJ_WG_PER_CU 16  // 32-seed launch: 3 (the residency at 156 VGPRs) 135.0 ms, 8 125.8-126.3, 16 123.1
#endif
#ifndef FKS_PROJ_LEAN        // 1: the vector stays f32 (converted inside the seed loop) and round 1 is redone per
#define FKS_PROJ_LEAN 0      // seed: 126 VGPRs and four waves per SIMD instead of 156 and three, but 140.0 ms
#endif
#ifndef FKS_PROJ_MIN_WAVES   // launch-bounds waves per SIMD (0: none).  4 with FKS_PROJ_LEAN: 147.2 ms; 4 or 5
#define FKS_PROJ_MIN_WAVES 0 // on the kept form spill to scratch
#endif
// fks_project_multi_kernel<NV> (profiles/r10_project_multi_ab.log; same layout, bf16 vectors, against NV launches of
// the parent build's fks_project_kernel at 122.7 ms each).  The NV x 32 values of a lane stay in registers:
#ifndef FKS_PROJ_MULTI_CVT_FROM    // vector counts from this one on keep them f32 (32 NV VGPRs) and widen to f64 inside
#define FKS_PROJ_MULTI_CVT_FROM 3  // the seed loop (an OR with a scalar zero the compiler cannot see through, then the
#endif                             // conversion); below it the f64 forms are hoisted (64 NV VGPRs).  With the fence:
                                   // 3 (kept): NV 2 222 VGPRs 0.585, NV 3 192 0.515, NV 4 228 0.436 of NV launches;
                                   // 2: NV 2 158 VGPRs, three waves per SIMD, but 0.646; never (f64 always): NV 3 and
                                   // 4 go past 256 VGPRs into AGPR copies at one wave per SIMD, 0.670 and 0.622;
                                   // per-value "+v" barriers instead of the scalar zero: 40 to 50 VGPRs more
                                   // (without the fence NV 4 takes 347 registers, 0.635)
#ifndef FKS_PROJ_MULTI_SCHED_FENCE   // 1: a scheduling barrier after each of a group's eight items, so that one
#define FKS_PROJ_MULTI_SCHED_FENCE 1 // item's generator is live at a time.  0: NV 3 and 4 need 283 and 268 registers,
#endif                               // one wave per SIMD (not timed; the f64 forms without it, two-wave bound: NV 4 1.576)
#ifndef FKS_PROJ_MULTI_MIN_WAVES   // launch-bounds waves per SIMD for NV >= 2.  1 (none): the kept forms hold two
#define FKS_PROJ_MULTI_MIN_WAVES 1 // waves unforced.  2 on the f64 forms spills to scratch: NV 3 0.539, NV 4 1.448
#endif
// Not measured: 2-byte vectors kept packed (16 VGPRs per vector, widened in the loop) and the vectors in LDS
// (32 KB per f32 vector and workgroup: one workgroup per CU at NV 4, no better than the registers' two waves).
constexpr int kProjWgPerCu = FKS_PROJ_WG_PER_CU;
constexpr int kProjLdsTensors = 512;  // tables of at most this many entries are copied to LDS
constexpr int kProjAccBytes = kProjWaves * kPhxSeeds * 8;  // the waves' sums, in front of the table
static_assert(kPhxSeeds <= 64, "lane k of a wave keeps seed k's sum");
static_assert(kProjAccBytes % 16 == 0, "the LDS table starts 16-byte aligned");

typedef __attribute__((address_space(1))) const u32x4_t proj_gu128;
typedef __attribute__((address_space(1))) const float proj_gf32;
typedef __attribute__((address_space(1))) const uint16_t proj_gu16;

// the last table entry whose first item is <= it, at or after lo (items only grow; a wave's
// next groups lie mostly in the same or the next tensor: a few probes, then bisection)
template <class Tab>
__device__ __forceinline__ int proj_find_t(Tab tab, int nt, int64_t it, int lo, int probes) {
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

// the 32 vector elements of the group at items r0 .. r0 + 7 of T: v[i][q] = element
// idx0 + q + S (4 j + i), +0 for an element past the tensor's end.  Whole 16-byte runs where
// the data is 16-byte aligned (idx0 and S are multiples of 8) and the four runs lie inside
// the tensor; per element otherwise (a tensor's last row, an unaligned vector).
__device__ __forceinline__ void proj_load(const PhxTensor& T, uint32_t idx0, uint64_t j, float v[4][kProjVec]) {
  const int64_t S = (int64_t)T.stride;
  const int64_t e0 = (int64_t)idx0 + S * (int64_t)(4 * j);
  if ((T.flags & kPhxP16) && e0 + 3 * S + kProjVec <= T.numel) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      proj_gu128* q = reinterpret_cast<proj_gu128*>(T.ptr + (uint64_t)(e0 + S * i) * 4u);
      const u32x4_t x = q[0], y = q[1];
      const uint32_t w[kProjVec] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
#pragma unroll
      for (int k = 0; k < kProjVec; k++) v[i][k] = __uint_as_float(w[k]);
    }
    return;
  }
  proj_gf32* p = reinterpret_cast<proj_gf32*>(T.ptr);
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int k = 0; k < kProjVec; k++) {
      const int64_t e = e0 + S * i + k;
      v[i][k] = e < T.numel ? p[e] : 0.0f;
    }
}

// a bf16 / f16 element widened to f32 (exact)
__device__ __forceinline__ float proj_widen(uint32_t h, bool bf) {
  const _Float16 f = __builtin_bit_cast(_Float16, (uint16_t)h);
  return bf ? __uint_as_float(h << 16) : (float)f;
}

// proj_load for a vector that lies on its own (E: its piece for table entry T, and its
// dtype): the same 32 elements in the same places.  An f32 vector loads as proj_load does; a
// 2-byte vector takes one 16-byte load per 8-element run where proj_load takes two; per
// element where the piece is not 16-byte aligned or the four runs do not lie inside it.
__device__ __forceinline__ void proj_load_any(const ProjVecEntry& E, const PhxTensor& T, uint32_t idx0, uint64_t j,
                                              float v[4][kProjVec]) {
  const int64_t S = (int64_t)T.stride;
  const int64_t e0 = (int64_t)idx0 + S * (int64_t)(4 * j);
  const bool whole = (E.flags & kPhxP16) && e0 + 3 * S + kProjVec <= T.numel;
  if (E.dtype == FKS_F32) {
    if (whole) {
#pragma unroll
      for (int i = 0; i < 4; i++) {
        proj_gu128* q = reinterpret_cast<proj_gu128*>(E.ptr + (uint64_t)(e0 + S * i) * 4u);
        const u32x4_t x = q[0], y = q[1];
        const uint32_t w[kProjVec] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
#pragma unroll
        for (int k = 0; k < kProjVec; k++) v[i][k] = __uint_as_float(w[k]);
      }
      return;
    }
    proj_gf32* p = reinterpret_cast<proj_gf32*>(E.ptr);
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int k = 0; k < kProjVec; k++) {
        const int64_t e = e0 + S * i + k;
        v[i][k] = e < T.numel ? p[e] : 0.0f;
      }
    return;
  }
  const bool bf = E.dtype == FKS_BF16;
  if (whole) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const u32x4_t x = *reinterpret_cast<proj_gu128*>(E.ptr + (uint64_t)(e0 + S * i) * 2u);
      const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int k = 0; k < 4; k++) {
        v[i][2 * k] = proj_widen(w[k] & 0xFFFFu, bf);
        v[i][2 * k + 1] = proj_widen(w[k] >> 16, bf);
      }
    }
    return;
  }
  proj_gu16* p = reinterpret_cast<proj_gu16*>(E.ptr);
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int k = 0; k < kProjVec; k++) {
      const int64_t e = e0 + S * i + k;
      v[i][k] = e < T.numel ? proj_widen(p[e], bf) : 0.0f;
    }
}

// Vector-fetch policies: where the NV vectors of a pass lie and how a group's elements reach
// the registers.  ProjFetchBuffer: fks_project's one f32 buffer, which the table entries
// themselves point into.  ProjFetchTable: fks_project_multi's vectors, each where it lies.
struct ProjFetchBuffer {
  static constexpr int NV = 1;
  __device__ __forceinline__ void load(const PhxTensor& T, int, uint32_t idx0, uint64_t j,
                                       float v[1][4][kProjVec]) const {
    proj_load(T, idx0, j, v[0]);
  }
};
template <int N>
struct ProjFetchTable {
  static constexpr int NV = N;
  const ProjVecEntry* vt;  // [NV][nt]
  int nt;
  __device__ __forceinline__ void load(const PhxTensor& T, int ti, uint32_t idx0, uint64_t j,
                                       float v[N][4][kProjVec]) const {
#pragma unroll
    for (int m = 0; m < N; m++) {
      const ProjVecEntry E = vt[(size_t)m * (size_t)nt + (size_t)ti];
      proj_load_any(E, T, idx0, j, v[m]);
    }
  }
};

// ProjFetchDraw: fks_gram's rows, drawn and not fetched.  Vector m of the group is the z of row
// seed m in the lane's tensor dtype -- the values fks_normal writes, which are the values
// proj_load_any reads from a buffer torch.normal filled --, in proj_load's places: v[m][i][q] =
// z(element idx0 + q + S (4 j + i)), +0 for an element past the tensor's end.  The row loop is
// not unrolled (one copy of the generator per item; the row's 32 values reach their registers
// through selects on the wave-uniform m); rows past the pass's count are +0 and never reduced.
// philox_round1 is written inside the row loop and not into an array above it: ctr and idx0 are
// invariant there, so the compiler hoists what it has registers for, and an explicit r1[8] would
// pin 32 VGPRs across the draw at 219 of 256 (the rows are 4 draws against a pass's 32 columns).
template <int N>
struct ProjFetchDraw {
  static constexpr int NV = N;
  const GramArgs& a;
  __device__ __forceinline__ void load(const PhxTensor& T, int, uint32_t idx0, uint64_t j,
                                       float v[N][4][kProjVec]) const {
    const int64_t S = (int64_t)T.stride;
    const int64_t e0 = (int64_t)idx0 + S * (int64_t)(4 * j);
    const uint64_t ctr = T.off4 + j;
    int room[4];  // run i holds elements q < room[i] of the tensor
#pragma unroll
    for (int i = 0; i < 4; i++)
      room[i] = (int)std::min<int64_t>(std::max<int64_t>(T.numel - (e0 + S * i), 0), kProjVec);
#pragma unroll
    for (int m = 0; m < N; m++)
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int q = 0; q < kProjVec; q++) v[m][i][q] = 0.0f;
#pragma unroll 1
    for (int m = 0; m < a.nrows; m++) {
      const uint64_t seed = a.rseeds[m];  // wave-uniform: a scalar load
#pragma unroll
      for (int q = 0; q < kProjVec; q++) {
        const uint4 w = philox4x32_10(philox_round1(ctr, idx0 + (uint32_t)q), seed);
        f32x2_t zA, zB;
        if (T.dtype == FKS_BF16) {
          phx_z_bf16(w, zA, zB);
        } else {
          phx_box_muller2(w, zA, zB);
          if (T.dtype != FKS_F32) {
            zA = (f32x2_t){phx_cast<FKS_F16>(zA.x), phx_cast<FKS_F16>(zA.y)};
            zB = (f32x2_t){phx_cast<FKS_F16>(zB.x), phx_cast<FKS_F16>(zB.y)};
          }
        }
        const float z[4] = {zA.x, zA.y, zB.x, zB.y};
#pragma unroll
        for (int mm = 0; mm < N; mm++)
#pragma unroll
          for (int i = 0; i < 4; i++) v[mm][i][q] = mm == m ? (q < room[i] ? z[i] : 0.0f) : v[mm][i][q];
        __builtin_amdgcn_sched_barrier(0);  // one item's generator at a time
      }
    }
  }
};

// Every seed of the pass over the wave's groups whose tensors draw dtype DT (`mine`: this
// lane has such a group): the whole wave runs this, lanes that are not `mine` enter +0.
// The z of a seed are drawn once; each of the NV vectors runs its own chain, q then i.
template <int DT, int NV, bool CVT_IN_LOOP, class Args>
__device__ __forceinline__ void proj_seeds(const Args& a, uint64_t ctr, uint32_t idx0,
                                           const float (&v)[NV][4][kProjVec], bool mine, int lane, double (&acc)[NV]) {
  PhxRound1 r1[kProjVec];
#pragma unroll
  for (int q = 0; q < kProjVec; q++) r1[q] = philox_round1(ctr, idx0 + (uint32_t)q);
  for (int k = 0; k < a.nseeds; k++) {
    const uint64_t seed = a.seeds[k];  // wave-uniform: scalar loads
    uint32_t zero = 0;
    if constexpr (CVT_IN_LOOP) asm volatile("" : "+s"(zero));  // one opaque scalar per seed
    double part[NV];
#pragma unroll
    for (int m = 0; m < NV; m++) part[m] = 0.0;
#pragma unroll
    for (int q = 0; q < kProjVec; q++) {
#if FKS_PROJ_LEAN
      uint32_t iq = idx0 + (uint32_t)q;
      asm volatile("" : "+v"(iq));  // opaque: keeps round 1 inside the loop
      const uint4 w = philox4x32_10(philox_round1(ctr, iq), seed);
#else
      const uint4 w = philox4x32_10(r1[q], seed);
#endif
      f32x2_t zA, zB;
      if constexpr (DT == FKS_BF16) {
        phx_z_bf16(w, zA, zB);
      } else {
        phx_box_muller2(w, zA, zB);
        zA = (f32x2_t){phx_cast<DT>(zA.x), phx_cast<DT>(zA.y)};
        zB = (f32x2_t){phx_cast<DT>(zB.x), phx_cast<DT>(zB.y)};
      }
      // exact products, one rounding per addition
#pragma unroll
      for (int m = 0; m < NV; m++) {
        float x0 = v[m][0][q], x1 = v[m][1][q], x2 = v[m][2][q], x3 = v[m][3][q];
#if FKS_PROJ_LEAN
        asm volatile("" : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3));  // opaque: the f64 conversions stay in the loop
#endif
        if constexpr (CVT_IN_LOOP) {  // | 0, a zero the compiler cannot see through: the conversions stay in the loop
          x0 = __uint_as_float(__float_as_uint(x0) | zero);
          x1 = __uint_as_float(__float_as_uint(x1) | zero);
          x2 = __uint_as_float(__float_as_uint(x2) | zero);
          x3 = __uint_as_float(__float_as_uint(x3) | zero);
        }
        part[m] = __fma_rn((double)x0, (double)zA.x, part[m]);
        part[m] = __fma_rn((double)x1, (double)zA.y, part[m]);
        part[m] = __fma_rn((double)x2, (double)zB.x, part[m]);
        part[m] = __fma_rn((double)x3, (double)zB.y, part[m]);
      }
#if FKS_PROJ_MULTI_SCHED_FENCE
      if constexpr (NV > 1) __builtin_amdgcn_sched_barrier(0);  // one item's generator at a time
#endif
    }
#pragma unroll
    for (int m = 0; m < NV; m++) {
      const double total = wave_sum(mine ? part[m] : 0.0);
      acc[m] += lane == k ? total : 0.0;
    }
  }
}

template <bool CVT_IN_LOOP, class Args, class Tab, class Fetch>
__device__ __forceinline__ void proj_walk(const Args& a, Tab tab, const Fetch& fetch, int lane,
                                          double (&acc)[Fetch::NV]) {
  constexpr int NV = Fetch::NV;
  const int64_t step = (int64_t)gridDim.x * kProjThreads * kProjVec;
  int64_t wb = rfl64(a.item_lo + ((int64_t)blockIdx.x * kProjThreads + (int64_t)(threadIdx.x & ~63u)) * kProjVec);
  int ts = 0;
  // wb and the loop are wave-uniform: every lane of the wave reaches the butterflies
  for (; wb < a.item_hi; wb += step) {
    ts = __builtin_amdgcn_readfirstlane(proj_find_t(tab, a.nt, wb, ts, 2));
    const int64_t wend = wb + 64 * kProjVec < a.item_hi ? wb + 64 * kProjVec : a.item_hi;
    const bool one = ts + 1 >= a.nt || tab[ts + 1].item0 >= wend;  // the whole wave in tensor ts
    const int64_t it = wb + (int64_t)lane * kProjVec;
    const bool active = it < a.item_hi;
    const int ti = one ? ts : proj_find_t(tab, a.nt, active ? it : a.item_hi - 1, ts, 0);
    const PhxTensor T = tab[ti];
    // (a lane without a group keeps a valid entry; its idx0 and j only feed a discarded z)
    const int64_t r0 = active ? it - T.item0 : 0;
    const uint32_t idx0 = (uint32_t)(r0 % (int64_t)T.stride);
    const uint64_t j = (uint64_t)(r0 / (int64_t)T.stride);
    float v[NV][4][kProjVec];
    if (active) {
      fetch.load(T, ti, idx0, j, v);
    } else {
#pragma unroll
      for (int m = 0; m < NV; m++)
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
          for (int k = 0; k < kProjVec; k++) v[m][i][k] = 0.0f;
    }
    // one pass per dtype present in the wave (wave-uniform branches: a wave lies in one
    // tensor, or in neighbours of one dtype, nearly always)
    const bool m32 = active && T.dtype == FKS_F32, mbf = active && T.dtype == FKS_BF16,
               m16 = active && T.dtype != FKS_F32 && T.dtype != FKS_BF16;
    if (__any(m32)) proj_seeds<FKS_F32, NV, CVT_IN_LOOP>(a, T.off4 + j, idx0, v, m32, lane, acc);
    if (__any(mbf)) proj_seeds<FKS_BF16, NV, CVT_IN_LOOP>(a, T.off4 + j, idx0, v, mbf, lane, acc);
    if (__any(m16)) proj_seeds<FKS_F16, NV, CVT_IN_LOOP>(a, T.off4 + j, idx0, v, m16, lane, acc);
  }
}

// One block's part of a pass: the table to LDS (behind the waves' sums), the walk, and the
// waves' sums added in wave order into partial[block][NV][kPhxSeeds].
template <bool CVT_IN_LOOP, class Args, class Fetch>
__device__ __forceinline__ void proj_block(const Args& a, const Fetch& fetch) {
  constexpr int NV = Fetch::NV;
  extern __shared__ __attribute__((aligned(16))) uint8_t s_proj[];
  double* s_acc = reinterpret_cast<double*>(s_proj);                              // [NV][kProjWaves][kPhxSeeds]
  PhxTensor* s_tab = reinterpret_cast<PhxTensor*>(s_proj + NV * kProjAccBytes);
  const int lane = (int)(threadIdx.x & 63u);
  const int wave = (int)(threadIdx.x >> 6);
  double acc[NV];  // lane k < kPhxSeeds: the wave's sum for seed k, per vector
#pragma unroll
  for (int m = 0; m < NV; m++) acc[m] = 0.0;
  if (a.nt <= kProjLdsTensors) {
    constexpr int W = (int)(sizeof(PhxTensor) / 4);
    for (int i = (int)threadIdx.x; i < a.nt * W; i += kProjThreads)
      reinterpret_cast<uint32_t*>(s_tab)[i] = reinterpret_cast<const uint32_t*>(a.t)[i];
    __syncthreads();
    proj_walk<CVT_IN_LOOP>(a, (const PhxTensor*)s_tab, fetch, lane, acc);
  } else {
    proj_walk<CVT_IN_LOOP>(a, a.t, fetch, lane, acc);
  }
#pragma unroll
  for (int m = 0; m < NV; m++)
    if (lane < kPhxSeeds) s_acc[(m * kProjWaves + wave) * kPhxSeeds + lane] = acc[m];
  __syncthreads();
  if (threadIdx.x < (unsigned)kPhxSeeds) {
#pragma unroll
    for (int m = 0; m < NV; m++) {
      double s = s_acc[m * kProjWaves * kPhxSeeds + (int)threadIdx.x];
#pragma unroll
      for (int w = 1; w < kProjWaves; w++) s += s_acc[(m * kProjWaves + w) * kPhxSeeds + (int)threadIdx.x];
      a.partial[((size_t)blockIdx.x * NV + m) * kPhxSeeds + threadIdx.x] = s;
    }
  }
}

#if FKS_PROJ_MIN_WAVES
__global__ __launch_bounds__(kProjThreads, FKS_PROJ_MIN_WAVES) void fks_project_kernel(ProjectArgs a) {
#else
__global__ __launch_bounds__(kProjThreads) void fks_project_kernel(ProjectArgs a) {
#endif
  proj_block<false>(a, ProjFetchBuffer{});
}

template <int NV>
__global__ __launch_bounds__(kProjThreads, NV == 1 ? 1 : FKS_PROJ_MULTI_MIN_WAVES) void fks_project_multi_kernel(
    ProjectMultiArgs a) {
  proj_block<(NV >= FKS_PROJ_MULTI_CVT_FROM)>(a, ProjFetchTable<NV>{a.vt, a.nt});
}

// fks_gram's pass: fks_project_multi_kernel<NR> with the vectors drawn (ProjFetchDraw), so row m
// of the pass equals, bit for bit, fks_project_multi on a vector that holds row seed m's draw
template <int NR>
__global__ __launch_bounds__(kProjThreads, FKS_PROJ_MULTI_MIN_WAVES) void fks_gram_kernel(GramArgs a) {
  proj_block<true>(a, ProjFetchDraw<NR>{a});
}

// fks_project_reduce_kernel's sum (the same lanes, blocks and butterfly) for one (column, row) of
// a Gram pass, written to its element of the matrix and, for a symmetric call, to the transposed
// one: <z_r, z_c> and <z_c, z_r> are the same products in the same order, so an element two
// passes (or two blocks of a diagonal pass) write receives the same bits from both
__global__ __launch_bounds__(64) void fks_gram_reduce_kernel(const double* partial, int nblocks, double* out,
                                                             int64_t ld, int row0, int col0, int mirror) {
  const int k = (int)blockIdx.x, m = (int)blockIdx.y;
  double s = 0.0;
  for (int b = (int)threadIdx.x; b < nblocks; b += 64) s += partial[((size_t)b * kGramRows + m) * kPhxSeeds + k];
  s = wave_sum(s);
  if (threadIdx.x == 0) {
    out[(int64_t)(row0 + m) * ld + col0 + k] = s;
    if (mirror) out[(int64_t)(col0 + k) * ld + row0 + m] = s;
  }
}

// one wave per (seed, vector): lane l adds the partials of blocks l, l + 64, ... in order,
// then the lanes' sums meet in the butterfly
__global__ __launch_bounds__(64) void fks_project_reduce_kernel(const double* partial, int nblocks, double* out,
                                                                int64_t out_stride) {
  const int k = (int)blockIdx.x, m = (int)blockIdx.y, nv = (int)gridDim.y;
  double s = 0.0;
  for (int b = (int)threadIdx.x; b < nblocks; b += 64) s += partial[((size_t)b * nv + m) * kPhxSeeds + k];
  s = wave_sum(s);
  if (threadIdx.x == 0) out[(int64_t)m * out_stride + k] = s;
}

}  // namespace

int project_grid(int64_t items) {
  const int64_t groups = (items + kProjVec - 1) / kProjVec;
  const int64_t want = (groups + kProjThreads - 1) / kProjThreads;
  return (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)kProjWgPerCu * device_cu_count()));
}

int launch_project(const ProjectArgs& a, void* stream) {
  const int64_t items = a.item_hi - a.item_lo;
  if (a.nseeds < 1 || a.nseeds > kPhxSeeds || a.nt < 1 || items <= 0 || !a.partial) return -FKS_EINVAL;
  // groups never straddle a tensor or the shard: every boundary is a multiple of 256 items
  if (a.item_lo % kProjVec != 0 || items % kProjVec != 0) return -FKS_EINVAL;
  const size_t lds = (size_t)kProjAccBytes + (a.nt <= kProjLdsTensors ? sizeof(PhxTensor) * (size_t)a.nt : 0);
  hipLaunchKernelGGL(fks_project_kernel, dim3((unsigned)project_grid(items)), dim3(kProjThreads), lds,
                     (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

namespace {
template <int NV>
void project_multi_launch(const ProjectMultiArgs& a, unsigned grid, size_t lds, hipStream_t stream) {
  hipLaunchKernelGGL(fks_project_multi_kernel<NV>, dim3(grid), dim3(kProjThreads), lds, stream, a);
}
}  // namespace

int launch_project_multi(const ProjectMultiArgs& a, void* stream) {
  static_assert(kProjMaxVec == 4, "one instance per vector count");
  const int64_t items = a.item_hi - a.item_lo;
  if (a.nseeds < 1 || a.nseeds > kPhxSeeds || a.nt < 1 || items <= 0 || !a.partial || !a.vt || a.nvec < 1 ||
      a.nvec > kProjMaxVec)
    return -FKS_EINVAL;
  if (a.item_lo % kProjVec != 0 || items % kProjVec != 0) return -FKS_EINVAL;
  const size_t lds =
      (size_t)kProjAccBytes * (size_t)a.nvec + (a.nt <= kProjLdsTensors ? sizeof(PhxTensor) * (size_t)a.nt : 0);
  const unsigned grid = (unsigned)project_grid(items);
  switch (a.nvec) {
    case 1: project_multi_launch<1>(a, grid, lds, (hipStream_t)stream); break;
    case 2: project_multi_launch<2>(a, grid, lds, (hipStream_t)stream); break;
    case 3: project_multi_launch<3>(a, grid, lds, (hipStream_t)stream); break;
    default: project_multi_launch<4>(a, grid, lds, (hipStream_t)stream); break;
  }
  return (int)hipGetLastError();
}

int launch_gram(const GramArgs& a, void* stream) {
  const int64_t items = a.item_hi - a.item_lo;
  if (a.nseeds < 1 || a.nseeds > kPhxSeeds || a.nrows < 1 || a.nrows > kGramRows || a.nt < 1 || items <= 0 ||
      !a.partial)
    return -FKS_EINVAL;
  if (a.item_lo % kProjVec != 0 || items % kProjVec != 0) return -FKS_EINVAL;
  const size_t lds =
      (size_t)kProjAccBytes * (size_t)kGramRows + (a.nt <= kProjLdsTensors ? sizeof(PhxTensor) * (size_t)a.nt : 0);
  hipLaunchKernelGGL(fks_gram_kernel<kGramRows>, dim3((unsigned)project_grid(items)), dim3(kProjThreads), lds,
                     (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int launch_gram_reduce(const double* partial, int nblocks, int nrows, int ncols, double* out, int64_t ld, int row0,
                       int col0, bool mirror, void* stream) {
  if (ncols < 1 || ncols > kPhxSeeds || nrows < 1 || nrows > kGramRows || nblocks < 1 || row0 < 0 || col0 < 0 ||
      (int64_t)col0 + ncols > ld || (mirror && (int64_t)row0 + nrows > ld))  // mirror: a square matrix of side ld
    return -FKS_EINVAL;
  hipLaunchKernelGGL(fks_gram_reduce_kernel, dim3((unsigned)ncols, (unsigned)nrows), dim3(64), 0, (hipStream_t)stream,
                     partial, nblocks, out, ld, row0, col0, mirror ? 1 : 0);
  return (int)hipGetLastError();
}

int launch_project_reduce(const double* partial, int nblocks, int nseeds, int nvec, double* out, int64_t out_stride,
                          void* stream) {
  if (nseeds < 1 || nseeds > kPhxSeeds || nblocks < 1 || nvec < 1 || nvec > kProjMaxVec) return -FKS_EINVAL;
  hipLaunchKernelGGL(fks_project_reduce_kernel, dim3((unsigned)nseeds, (unsigned)nvec), dim3(64), 0,
                     (hipStream_t)stream, partial, nblocks, out, out_stride);
  return (int)hipGetLastError();
}

}  // namespace fks
