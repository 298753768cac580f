// fks_kern_slice.h -- fks_apply_bs_kernel, the bit-sliced bf16 reconstruct kernel.
#pragma once
#include <hip/hip_runtime.h>

#include "fks_internal.h"
#include "fks_bitslice.h"
#include "fks_dev_lds.h"
#include "fks_dev_update.h"
#include "fks_dev_zgen.h"

namespace fks {
namespace {

// ------------------------------------------------------------------ bf16 slice kernel
// fks_apply_bs_kernel<MODE>: the bf16 fast segments of a reconstruct, 64 seeds per pass
// as two SLICES of 32, generator state BIT-SLICED (fks_bitslice.h): row i of a slice's
// state is state word i of its 32 seeds as 32 bit planes.  One workgroup per CU takes one
// chunk and holds both slices' states in LDS, one per half.  The work of a chunk is cut
// into TASKS of 128 consecutive stream words (64 Box-Muller pairs: one wave), and the six
// waves of a half take the half's tasks round-robin.  A wave runs the whole of its task:
//   * twist: lane L owns the pair (j, j+8), j = 16 (L >> 3) + (L & 7) of the task, and
//     twists exactly those two rows in place, block b -> b+1 (MT19937RNGEngine.h:164-175
//     on 32 seeds at once): word u of the stream is f(word u-624 (plane 31 only: U31),
//     word u-623 (V, the next slot), word u-227 (M));
//   * the two new rows are still in registers: temper their low bytes (temper_low8),
//     transpose them to one byte per seed, and run the 32-seed update chain of the lane's
//     two parameters (thread owns Box-Muller pair (j, j+8): two table lookups, the z
//     product and its rounding, the per-op-rounded update chain).
// The twists of a half form one serial chain -- M of a task's last 29 words are words the
// previous task wrote -- so a wave waits until the half's LDS flag counts n twisted
// tasks, twists task n, and publishes n+1; the chains of different tasks overlap freely.
// Half 1 applies its seeds to what half 0 stored: its wave for task n waits until the
// half-0 wave of task n+6 has published that store as complete before it prefetches
// task n+6's parameters (half 0 publishes task m at its task m+6, after s_waitcnt
// vmcnt(0): workgroup-scope release; half 0 never waits for half 1).  Two slices per
// workgroup instead of two chunks halve the jumps (one per seed and chunk) and the HBM
// passes of a reconstruct.
// Against the round-2 form (five pair waves + one twist wave per half, two workgroup
// barriers per MT block): no pair wave re-reads the rows the twist wave wrote (a quarter
// of the LDS traffic), every wave carries the same instruction mix (no SIMD with three
// pair waves beside one with the twist wave), no barrier per block; with that LDS time
// freed, the (C,S) table is read as f32 pairs (one ds_read_b64, no unpack instructions):
// 3.83 -> 3.39 ms per 32-seed launch over 2^28 params (profiles/r03s_ab.log; the
// variants measured on the way are in profiles/r03k..r03s_ab.log).
// LDS: [R f32 x 256 | (C,S) f32 pairs x 256 | state half 0 | state half 1 | 2 twist flags |
// 6 half-0 progress words]; a
// half's state is 8 CHUNK arrays (planes 4q..4q+3 of all 624 rows, 16 B per row), so a
// row's chunk q is one ds_read_b128 / ds_write_b128.  The lane's first row is j+8 where
// (L >> 3) is odd, which makes every 16-lane group of a ds_read_b128 (8-lane group of a
// ds_write_b128) touch distinct rows mod 16: conflict free.
constexpr int kBsChunkBytes = kMtN * 16;               // 9,984
constexpr int kBsStateBytes = 8 * kBsChunkBytes;       // 79,872
constexpr int kBsTabBytes = 256 * 4 + 256 * 8;         // 3,072
constexpr uint32_t kBsFlagOff = kBsTabBytes + 2 * kBsStateBytes;  // u32 twisted-task count per half
constexpr uint32_t kBsProgOff = kBsFlagOff + 8;        // u32 per half-0 wave: its tasks < value are stored
constexpr uint32_t kBsProg1Off = kBsProgOff + 4 * 6;   // u32 per half-1 wave: its tasks < value are done
constexpr int kBsLdsBytes = (int)kBsProg1Off + 4 * 6;  // 162,872 <= 163,840
static_assert(kBsLdsBytes <= 163840, "slice kernel LDS");
constexpr int kBsWaves = kBsHalfThreads / 64;          // waves per half (6)
constexpr int kBsTaskWords = 128;                      // stream words per task

// the 32 planes of row i (row byte address ra = state base + 16 i)
__device__ __forceinline__ void bs_store_row(uint32_t ra, const uint32_t (&x)[32]) {
#pragma unroll
  for (int q = 0; q < 8; q++) {
    const u32x4_t v = {x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]};
    lds_st4(ra + q * kBsChunkBytes, v);
  }
}

// The flag hand-off needs no memory fence: one wave's LDS operations are performed in
// order, so a wave that reads the new count issues its row loads after the writer's row
// stores were performed.  (A release fence would also wait for the writer's global
// stores.)  The lgkmcnt(0) keeps the count from running ahead of stores still queued;
// the asm barriers keep the compiler from moving LDS accesses across.
__device__ __forceinline__ uint32_t bs_flag_load(uint32_t off) {
  return *(volatile const lds_u32_t*)(size_t)off;
}
__device__ __forceinline__ void bs_flag_store(uint32_t off, uint32_t v) {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
  *(volatile lds_u32_t*)(size_t)off = v;
}

// byte c of w times 2^S with a compile-time c (SDWA)
template <int S>
__device__ __forceinline__ uint32_t bs_index(uint32_t w, int c) {
  switch (c) {
    case 0: return bs::byte_x<0, S>(w);
    case 1: return bs::byte_x<1, S>(w);
    case 2: return bs::byte_x<2, S>(w);
    default: return bs::byte_x<3, S>(w);
  }
}

#if FKS_BS_WGTIME  // diagnostic build: per-workgroup start and per-wave end times (100 MHz)
__device__ uint64_t g_bs_wgtime[4096][16];
extern "C" int fks_debug_bs_wgtime(uint64_t* out, int nblocks) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bs_wgtime), sizeof(uint64_t) * 16 * (size_t)nblocks, 0,
                                  hipMemcpyDeviceToHost);
}
#endif

template <int MODE, bool FULL>
__global__ __launch_bounds__(kBsThreads, 1) void fks_apply_bs_kernel(ApplyBsArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds32[];
  if ((uint32_t)(size_t)(lds_u32_t*)lds32 != 0u) __builtin_trap();
  const int tid = threadIdx.x;
  const int lane = tid & 63;
#if FKS_BS_WGTIME
  if (tid == 0) g_bs_wgtime[blockIdx.x][0] = __builtin_amdgcn_s_memrealtime();
  auto stamp = [&]() { if (lane == 0) g_bs_wgtime[blockIdx.x][1 + (tid >> 6)] = __builtin_amdgcn_s_memrealtime(); };
#else
  auto stamp = [&]() {};
#endif
  const int half = __builtin_amdgcn_readfirstlane(tid >= kBsHalfThreads ? 1 : 0);
  const int ht = tid - half * kBsHalfThreads;
  const int hw = __builtin_amdgcn_readfirstlane(ht >> 6);
  // slices (a pass of 33..64 seeds): both halves on plan chunks 2w, 2w+1, slice 0 with
  // seeds [0, nA), slice 1 with [nA, nseeds) applied after slice 0's; split (<= 32 seeds):
  // half h alone on plan chunk 2w+h with every seed
  const bool split = a.split != 0;  // FULL: 32 seeds in each half either way
  const int c = split ? 2 * (int)blockIdx.x + half : (int)blockIdx.x;  // index into the states
  const int nA = FULL ? kBsSeeds : split ? a.nseeds : (a.nseeds + 1) / 2;
  const int nseeds = FULL ? kBsSeeds : (half && !split ? a.nseeds - nA : nA);  // this half's seeds
  const int sfirst = half && !split ? nA : 0;
  const int64_t b0 = a.chunk_block[split ? c : 2 * c], b1 = a.chunk_block[split ? c + 1 : 2 * c + 2];
  const int nwords = (int)(kMtN * (b1 - b0));  // < 2^31 (the host's plan keeps chunks shorter)
  const int ntask = (nwords + kBsTaskWords - 1) / kBsTaskWords;
  const uint32_t sbase = kBsTabBytes + (uint32_t)half * kBsStateBytes;
  const uint32_t flag = kBsFlagOff + 4u * (uint32_t)half;

  for (int i = tid; i < 256; i += kBsThreads) {
    reinterpret_cast<float*>((uint8_t*)lds32)[i] = c_tab_bf16[i];
    reinterpret_cast<float2*>((uint8_t*)lds32 + 1024)[i] = make_float2(c_tab_bf16[256 + i], c_tab_bf16[512 + i]);
  }
  // prologue: the jump windows of this chunk (the state before block b0), as planes
  for (int i = ht; i < kMtN; i += kBsHalfThreads) {
    uint32_t w[32];
#pragma unroll
    for (int k = 0; k < 32; k++)
      w[k] = k < nseeds ? a.states[((size_t)(a.use_slot ? a.slot[sfirst + k] : (uint32_t)(sfirst + k)) * a.nchunks + c) *
                                       kMtN + i]
                        : 0u;
    bs::transpose32(w);
    bs_store_row(sbase + 16u * (uint32_t)i, w);
  }
  if (ht == 0) lds32[flag / 4] = 0u;
  if (ht < kBsWaves) lds32[(half ? kBsProg1Off : kBsProgOff) / 4 + ht] = 0u;
  __syncthreads();  // the only workgroup barrier
  if (nseeds == 0) return;  // a one-seed pass: slice 1 is empty

  const int toff = 16 * (lane >> 3) + (lane & 7);  // the lane's words toff, toff + 8 of a task
  const bool flip = ((lane >> 3) & 1) != 0;
  const bool odd = (lane & 1) != 0;

  // The wd 0 chain's task path without lane-mask selects and neighbour exchanges, each lever
  // with its switch (fks_device.hip; measured in profiles/r09_bs_taskpath_ab.log)
  // (kModeUpdateWdPos0 is the same chain without the tail's fma: the host chose it, fks_run.cpp)
  constexpr bool kPos0 = MODE == kModeUpdateWdPos0;
  constexpr bool kWd0 = MODE == kModeUpdateWd0 || kPos0;
  constexpr bool kD16 = kWd0 && FKS_BS_D16 != 0;          // parameters as 16-bit halves, no pair exchange
  constexpr bool kG32 = kWd0 && FKS_BS_G32 != 0;          // two seeds' g per SGPR pair
  constexpr bool kRowMin = kWd0 && FKS_BS_ROWMIN != 0;    // row indices wrapped by unsigned min
  constexpr bool kFlipMux = kWd0 && FKS_BS_FLIPMUX != 0;  // the planes' flip as a bitwise mux
  // all ones in the lanes whose first row is toff + 8 (pinned in a VGPR: a value the compiler
  // sees through becomes the compare-and-select again)
  uint32_t flipm = flip ? ~0u : 0u;
  if (kFlipMux) asm volatile("" : "+v"(flipm));

  float gk[kBsSeeds];
#pragma unroll
  for (int k = 0; k < kBsSeeds; k++) gk[k] = a.g[half ? k + sfirst : k];
  uint64_t gg[kBsSeeds / 2];  // kG32: {g of seed 2k, g of seed 2k+1}
#pragma unroll
  for (int k = 0; k < kBsSeeds / 2; k++)
    gg[k] = (uint64_t)rfl(__float_as_uint(gk[2 * k])) | ((uint64_t)rfl(__float_as_uint(gk[2 * k + 1])) << 32);

  // the lane's current segment (positions only grow)
  const int64_t wbase = (int64_t)kMtN * b0;  // stream position of the chunk's first word
  int cur;
  {
    const int64_t s1 = wbase + (int64_t)kBsTaskWords * hw + toff;
    int lo = 0, hi = a.nsegs;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (a.segs[mid].start + a.segs[mid].numel <= s1) lo = mid + 1; else hi = mid;
    }
    cur = lo;
  }
  int64_t seg_start = INT64_MAX, seg_end = INT64_MAX;
  uint64_t seg_ptr = 0;
  float seg_lr = 0.0f, seg_wd = 0.0f;
  bool seg_wdf = false;
  constexpr int kEs = MODE == kModeDelta ? 4 : 2;  // bytes per parameter (the delta buffer is f32)
  // The wd 0 chain (kInc) addresses a task without division or 64-bit compares: the segment
  // as 32-bit word offsets into this chunk, [seg_lo, seg_hi) clamped to int (a task word
  // offset u1 stays below 2^31), and the address of chunk word 0 in the segment's tensor, so
  // that a lane's address is seg_org + 2 or 4 u1: one 32-bit offset added; and the state row
  // carried from task to task (next_row()).  The other chains keep the 64-bit form: with the
  // 32-bit one the weight-decay chain measured 0.4 % and the no-wd chain 0.6 % slower
  // (profiles/r07_bs_colimit_ab.log, profiles/r07_bench_parent_vs_v1all.log).
  constexpr bool kInc = kWd0;
  int seg_lo = INT32_MAX, seg_hi = INT32_MAX;
  uint64_t seg_org = 0;
  auto load_seg = [&]() {
    if (cur < a.nsegs) {
      const DevSeg sg = a.segs[cur];
      seg_start = sg.start;
      seg_end = sg.start + sg.numel;
      seg_ptr = sg.ptr;
      seg_lr = sg.lr;
      seg_wd = sg.wd;
      seg_wdf = (sg.flags & FKS_HAS_WD) != 0;
    } else {
      seg_start = seg_end = INT64_MAX;
    }
    if (kInc) {
      const int64_t lo = seg_start - wbase, hi = seg_end - wbase;  // past the last segment: >= INT32_MAX
      seg_lo = (int)(lo < INT32_MIN ? INT32_MIN : lo > INT32_MAX ? INT32_MAX : lo);
      seg_hi = (int)(hi < INT32_MIN ? INT32_MIN : hi > INT32_MAX ? INT32_MAX : hi);
      seg_org = seg_ptr - (uint64_t)lo * kEs;  // only used where seg_lo <= u1 < seg_hi
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): see fks_apply_kernel
  };
  load_seg();

  // The lane's parameters of task n: elements toff, toff + 8 of the task, loaded as the
  // aligned pairs (j, j+1) (even lane j) and (j+7, j+8) (odd lane j+1) and exchanged with
  // the neighbour lane (swap_adjacent).  Lanes past the chunk or off every fast segment
  // read and write the sink.
  using ST = Traits<MODE == kModeDelta ? FKS_F32 : FKS_BF16>;
  typedef typename ST::Pair Pair;
  // kD16: every lane loads its own two elements instead, each as a 16-bit load whose value
  // becomes the high half of a register -- the bits of the f32 value -- from one address
  // (element toff; element toff + 8 lies 16 bytes on, the sink included: 4 KB), and stores the
  // high halves back (global_store_short_d16_hi).  No exchange, no halves to pick or pack, no
  // divergent pack; plain loads and stores, so the compiler counts vmcnt for them as for the
  // pair (one more load per task behind the R loads' counted waits, one more store under
  // publish_stored()'s vmcnt(0)).  The load is global_load_ushort and a shift, not
  // global_load_short_d16_hi: with SRAM ECC a d16 load does not keep the register's other
  // half, so the compiler does not select it.
  struct Slot { uint64_t addr; float lr, wd; uint32_t wdf; Pair raw; uint32_t hi0, hi1; };
  auto fetch = [&](int n) -> Slot {
    Slot sl;
    const int u1 = kBsTaskWords * n + toff;
    if (kInc) {
      while (u1 >= seg_hi) { cur++; load_seg(); }
      const bool on = u1 < nwords && u1 >= seg_lo;
      sl.lr = seg_lr; sl.wd = seg_wd; sl.wdf = seg_wdf;
      sl.addr = on ? seg_org + (uint64_t)(uint32_t)(u1 + (odd && !kD16 ? 7 : 0)) * kEs : (uint64_t)(uintptr_t)a.sink;
      if (kD16) {
        sl.hi0 = Traits<FKS_BF16>::load_hi(sl.addr);
        sl.hi1 = Traits<FKS_BF16>::load_hi(sl.addr + 16);
        return sl;
      }
    } else {
      const int64_t s1 = wbase + u1;
      while (s1 >= seg_end) { cur++; load_seg(); }
      const bool on = u1 < nwords && s1 >= seg_start;
      sl.lr = seg_lr; sl.wd = seg_wd; sl.wdf = seg_wdf;
      sl.addr = on ? seg_ptr + (uint64_t)(s1 - seg_start + (odd ? 7 : 0)) * kEs : (uint64_t)(uintptr_t)a.sink;
    }
    sl.raw = ST::load_pair(sl.addr);
    return sl;
  };

  // ---- the twist of task n: the lane's two rows in place; returns the tempered radius
  // bytes (row toff) and angle bytes (row toff + 8) as planes.  Streamed over the 8 chunk
  // arrays (planes 4q..4q+3): chunk q of every row of the task is loaded (V, M) before
  // any lane stores it -- through data dependence, since new plane 4q+3 needs V plane
  // 4q+4 of chunk q+1, loaded one step ahead; U31 and V plane 0 are loaded first.  M
  // rows lie 227 words back, outside the task, so the task never stores them.
  // The state row of the lane's word toff of the wave's current task, (128 n + toff) mod 624.
  // A wave's tasks lie kBsWaves * 128 = 768 words apart, so the row moves on by 144 mod 624:
  // divided out once here and carried by next_row() from then on.
  constexpr int kRowStep = kBsWaves * kBsTaskWords % kMtN;
  int row = (kBsTaskWords * hw + toff) % kMtN;
  // kRowMin: the wraps as unsigned min -- x in [0, 2 * 624): min(x, x - 624) is x below 624
  // (x - 624 wraps to a huge value) and x - 624 from there on -- and the flip as the lane's
  // two row offsets (8, 0) or (0, 8), so that no row index takes a compare and a select.
  // The carried row is a valid row in every lane, also past the chunk's end: those lanes
  // load rows nobody uses and only their stores are masked.
  auto wrap = [](uint32_t x) -> uint32_t {
    const uint32_t y = x - (uint32_t)kMtN;
    return x < y ? x : y;
  };
  uint32_t rofa = flip ? 8u : 0u, rofb = flip ? 0u : 8u;
  if (kRowMin) asm volatile("" : "+v"(rofa), "+v"(rofb));
  auto next_row = [&]() {
    if (!kInc) return;
    if (kRowMin) {
      row = (int)wrap((uint32_t)row + kRowStep);
      return;
    }
    row += kRowStep;
    if (row >= kMtN) row -= kMtN;
  };
  // FKS_BS_H1 (the fma-free wd +0 chain): the row indices and LDS addresses of a task's twist depend
  // on the carried row only, not on the hand-off flag: task() computes them BEFORE it polls the flag
  // and pins them in VGPRs, so that the serial section between two flag values starts with its loads
  // (about 26 VALU instructions at priority 2 leave it).
  // (FKS_BS_H2, measured and removed: U31 and V of chunk arrays 0 and 1 loaded once the flag shows task
  // n - 4 twisted, ahead of the poll for task n - 1 -- those rows were last written by tasks n - 5 and
  // n - 4 -- was bit-exact and 4 % SLOWER on top of H1: profiles/r10_bs_pos0_ab.log)
  struct TwAddr { uint32_t av1, am1, au1, av2, am2, au2, sa, sb; };
  constexpr bool kH1 = kPos0 && kRowMin && FKS_BS_H1 != 0;
  TwAddr pre{};
  auto tw_pre = [&]() {
    const uint32_t ia = (uint32_t)row + rofa, ib = (uint32_t)row + rofb;
    pre.av1 = sbase + 16u * wrap(ia + 1u);
    pre.am1 = sbase + 16u * wrap(ia + kMtM);
    pre.au1 = sbase + 7u * kBsChunkBytes + 16u * ia + 12u;
    pre.av2 = sbase + 16u * wrap(ib + 1u);
    pre.am2 = sbase + 16u * wrap(ib + kMtM);
    pre.au2 = sbase + 7u * kBsChunkBytes + 16u * ib + 12u;
    pre.sa = sbase + 16u * ia;
    pre.sb = sbase + 16u * ib;
    asm volatile("" : "+v"(pre.av1), "+v"(pre.am1), "+v"(pre.au1), "+v"(pre.av2), "+v"(pre.am2), "+v"(pre.au2),
                 "+v"(pre.sa), "+v"(pre.sb));
  };
  auto twist = [&](const int n, uint32_t (&oa)[8], uint32_t (&ob)[8]) {
    const int u1 = kBsTaskWords * n + toff;
    const bool valid = u1 < nwords;
    const int i1 = kRowMin ? row : valid ? (kInc ? row : u1 % kMtN) : 0;
    // first / second row (i1 + 8 < 624: 624 is a multiple of 16 and i1 mod 16 < 8)
    const int ia = kRowMin ? i1 + (int)rofa : flip ? i1 + 8 : i1, ib = kRowMin ? i1 + (int)rofb : flip ? i1 : i1 + 8;
    auto rows = [&](int i, uint32_t& av, uint32_t& am, uint32_t& au) {
      const int iv = kRowMin ? (int)wrap((uint32_t)i + 1u) : i + 1 < kMtN ? i + 1 : 0;
      const int im = kRowMin ? (int)wrap((uint32_t)i + kMtM) : i < kMtN - kMtM ? i + kMtM : i - (kMtN - kMtM);
      av = sbase + 16u * (uint32_t)iv;
      am = sbase + 16u * (uint32_t)im;
      au = sbase + 7u * kBsChunkBytes + 16u * (uint32_t)i + 12u;
    };
    uint32_t av1, am1, au1, av2, am2, au2;
    rows(ia, av1, am1, au1);
    rows(ib, av2, am2, au2);
    if (kH1) {
      av1 = pre.av1; am1 = pre.am1; au1 = pre.au1;
      av2 = pre.av2; am2 = pre.am2; au2 = pre.au2;
    }
    uint32_t M1[32], M2[32];  // the new rows
    const uint32_t U1 = lds_u32((int)au1), U2 = lds_u32((int)au2);
    // (issuing all 34 loads of the task at once -- 164 VGPRs -- measured 5 % slower per
    // pass: profiles/r03v_ab.log)
    // (loads two or three chunk arrays ahead measured no faster: profiles/r03x_ab.log)
    u32x4_t va = lds_u4(av1), vb = lds_u4(av2), ma = lds_u4(am1), mb = lds_u4(am2);
    const uint32_t v0a = va.x, v0b = vb.x;
#pragma unroll
    for (int q = 0; q < 8; q++) {
      u32x4_t va2 = va, vb2 = vb, ma2 = ma, mb2 = mb;
      if (q < 7) {
        va2 = lds_u4(av1 + (q + 1) * kBsChunkBytes);
        vb2 = lds_u4(av2 + (q + 1) * kBsChunkBytes);
        ma2 = lds_u4(am1 + (q + 1) * kBsChunkBytes);
        mb2 = lds_u4(am2 + (q + 1) * kBsChunkBytes);
      }
      const uint32_t Va[5] = {va.x, va.y, va.z, va.w, va2.x};
      const uint32_t Vb[5] = {vb.x, vb.y, vb.z, vb.w, vb2.x};
      const uint32_t Ma[4] = {ma.x, ma.y, ma.z, ma.w}, Mb[4] = {mb.x, mb.y, mb.z, mb.w};
#pragma unroll
      for (int t = 0; t < 4; t++) {
        // bs::twist_row plane by plane: plane b of y >> 1 is V plane b+1 (b < 30; t = 3
        // reads chunk q+1's plane 0), U31 (b = 30), none (b = 31)
        const int b = 4 * q + t;
        const bool am = ((bs::kMatrixA >> b) & 1u) != 0;
        uint32_t xa, xb;
        if (b < 30) { xa = Va[t + 1]; xb = Vb[t + 1]; }
        else if (b == 30) { xa = U1; xb = U2; }
        else { xa = 0u; xb = 0u; }
        M1[b] = am ? bs::xor3(Ma[t], xa, v0a) : (Ma[t] ^ xa);
        M2[b] = am ? bs::xor3(Mb[t], xb, v0b) : (Mb[t] ^ xb);
      }
      if (valid) {
        lds_st4((kH1 ? pre.sa : sbase + 16u * (uint32_t)ia) + q * kBsChunkBytes, u32x4_t{M1[4 * q], M1[4 * q + 1], M1[4 * q + 2], M1[4 * q + 3]});
        lds_st4((kH1 ? pre.sb : sbase + 16u * (uint32_t)ib) + q * kBsChunkBytes, u32x4_t{M2[4 * q], M2[4 * q + 1], M2[4 * q + 2], M2[4 * q + 3]});
      }
      va = va2; vb = vb2; ma = ma2; mb = mb2;
    }
    uint32_t o1[8], o2[8];
    bs::temper_low8(M1, o1);
    bs::temper_low8(M2, o2);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      // row toff: the radius uniforms; row toff + 8: the angle uniforms (kFlipMux: the same
      // choice as v_bitop3_b32 on the lane's mask)
      oa[j] = kFlipMux ? bs::mux(flipm, o2[j], o1[j]) : flip ? o2[j] : o1[j];
      ob[j] = kFlipMux ? bs::mux(flipm, o1[j], o2[j]) : flip ? o1[j] : o2[j];
    }
  };

  // ---- the 32-seed chain of the lane's two parameters (slot sl), z from the bytes of
  // twist(): z = bf16(R[a] C[b]) + 0, bf16(R[a] S[b]) + 0 (normal_fill_16<BFloat16>: an
  // exact f32 product, one rounding; the fma's +0 turns -0 into +0 like "+ mean")
  // In the wd 0 chain, with FKS_BS_R_VMEM = m > 0, the first m seeds of every byte column take
  // R from the device-global table (c_tab_bf16, L1-resident) instead of the LDS: chain_head()
  // issues all 4 m loads of the task, BEFORE the task's parameter prefetch and after half 0's
  // vmcnt(0) of publish_stored().  Vector-memory loads return in order, so a column's radii
  // never wait for the prefetch behind them, and the compiler counts every vmcnt itself (plain
  // loads: vmcnt(4 m) down to vmcnt(1) through the chain, the prefetch last).  All at the task
  // head rather than one column ahead: issued inside the chain they would queue behind the
  // prefetch, whose HBM latency every column would then wait out; the price is 4 m live VGPRs
  // (126 against 121 for m = 3, no spill).  A segment walk inside fetch() (rare) drains them
  // early through load_seg()'s vmcnt(0), which costs time, not correctness.
  // Only the wd 0 chain: the weight-decay chain measured 2 % and the no-wd chain 0.9 % slower
  // with it (profiles/r07_bs_colimit_ab.log); the delta chain was not measured.
  constexpr int kRv = kInc ? FKS_BS_R_VMEM : 0;
  static_assert(kRv >= 0 && kRv <= 8, "FKS_BS_R_VMEM");
  // seed k's slot in rv, or -1 where it reads the LDS
  auto rv_slot = [](const int k) __attribute__((always_inline)) -> int {
    return (k & 7) < kRv ? (k >> 3) * kRv + (k & 7) : -1;
  };
  auto chain_head = [&](uint32_t (&oa)[8], uint32_t (&ob)[8], float (&rv)[4 * kRv + 1]) {
    bs::transpose8(oa);
    bs::transpose8(ob);
#pragma unroll
    for (int k = 0; k < kBsSeeds; k++)
      if (rv_slot(k) >= 0)
        rv[rv_slot(k)] =
            *reinterpret_cast<const float*>(reinterpret_cast<const char*>(c_tab_bf16) + bs_index<2>(oa[k & 7], k >> 3));
  };
  auto chain = [&](const Slot& sl, uint32_t (&oa)[8], uint32_t (&ob)[8], const float (&rv)[4 * kRv + 1]) {
    if (kRv == 0) {
      bs::transpose8(oa);
      bs::transpose8(ob);
    }
    f32x2_t p;
    if (kD16) {
      p.x = __uint_as_float(sl.hi0);
      p.y = __uint_as_float(sl.hi1);
    } else {
      const uint32_t keep = odd ? ST::hi(sl.raw) : ST::lo(sl.raw);
      const uint32_t got = swap_adjacent(odd ? ST::lo(sl.raw) : ST::hi(sl.raw));
      p.x = ST::cvt(odd ? got : keep);
      p.y = ST::cvt(odd ? keep : got);
    }
    if (kPos0) {
      // The chain without the tail's fma (apply_tail: t = gz) needs a +-inf parameter to be the
      // NaN the fma form makes of it at the first seed (0 * inf).  One packed fma(0, p, p) per
      // task does that with the same instruction, so with the same bits: inf gives the default
      // NaN, a NaN comes out quieted with its sign and payload (as fma(wd, p, gz) leaves it, and
      // every later p - w keeps it), and a finite p, zeros of either sign and denormals included,
      // comes out as itself (0 * p is a zero of p's sign, and p + that zero is p).
      const f32x2_t zero = {0.0f, 0.0f};
      p = __builtin_elementwise_fma(zero, p, p);
    }
    auto z_of = [&](const int k) __attribute__((always_inline)) -> f32x2_t {
      // (all 32 R reads through the vector-memory path, each issued at its seed and waited
      // for there: 13 % slower, profiles/r04rg_r_global_ab.log.  R as bf16, two entries per
      // LDS dword, read by ds_read_u16_d16_hi into a zeroed register: 0.2 % slower alone, 2.6 %
      // slower beside the vector-memory radii, profiles/r07_bs_colimit_ab.log)
      const float r = rv_slot(k) >= 0 ? rv[rv_slot(k)] : lds_f32(bs_index<2>(oa[k & 7], k >> 3));
      const f32x2_t rr = {r, r}, zero = {0.0f, 0.0f};
      const f32x2_t cs = lds_f32x2(1024u + bs_index<3>(ob[k & 7], k >> 3));
      return rnd2<FKS_BF16>(__builtin_elementwise_fma(rr, cs, zero));
    };
#if FKS_BS_LOOK > 0
    // FKS_BS_LOOK = D > 0 (the fma-free wd +0 chain): a rolling window of D seeds' lookups, loads
    // only -- those of seeds 0..D-1 issued before the seed loop, those of seed k + D in iteration k
    // ahead of seed k's arithmetic -- so that a seed's LDS round trip passes behind D seeds' VALU
    // work.  Plain loads: the compiler counts lgkmcnt.
    constexpr int kLook = kPos0 ? FKS_BS_LOOK : 0;
    static_assert(kLook <= kBsSeeds, "FKS_BS_LOOK");
    float wr[kLook + 1];
    f32x2_t wcs[kLook + 1];
    auto look = [&](const int k, const int s) __attribute__((always_inline)) {
      wr[s] = rv_slot(k) >= 0 ? rv[rv_slot(k)] : lds_f32(bs_index<2>(oa[k & 7], k >> 3));
      wcs[s] = lds_f32x2(1024u + bs_index<3>(ob[k & 7], k >> 3));
    };
#pragma unroll
    for (int k = 0; k < kLook; k++) {
      wr[k] = 0.0f;
      wcs[k] = f32x2_t{0.0f, 0.0f};
      if (FULL || k < nseeds) look(k, k);
    }
    auto z_la = [&](const int k) __attribute__((always_inline)) -> f32x2_t {
      const int s = k % (kLook > 0 ? kLook : 1);
      const f32x2_t rr = {wr[s], wr[s]}, zero = {0.0f, 0.0f}, cs = wcs[s];
      if (k + kLook < kBsSeeds && (FULL || k + kLook < nseeds)) {
        look(k + kLook, s);
      }
      return rnd2<FKS_BF16>(__builtin_elementwise_fma(rr, cs, zero));
    };
#define FKS_BS_Z(k) (kLook > 0 ? z_la(k) : z_of(k))
#else
#define FKS_BS_Z(k) z_of(k)
#endif
    // (issuing seed k+1's lookups, z and g z ahead of seed k's p-dependent tail, which
    // removes the wait state between the tail's dependent packed ops, measured 1 % slower:
    // profiles/r04d_pipe_ab.log; dropping the wd0 tail's fma -- t = gz for wd = +0 and a
    // finite p, with the chain redone exactly for the lanes that end non-finite -- issues one
    // packed op per element pair and seed fewer but measured 1.5 % slower, its lr*gz waiting
    // on gz's conversions: profiles/r04o_wd0_nofma_ab.log.  The host-decided form, kModeUpdateWdPos0,
    // has no redo path; alone it gains nothing either, with the look-ahead window it does: §10 round 10)
    {
#pragma unroll
      for (int k = 0; k < kBsSeeds; k++) {
        if (FULL || k < nseeds) {
          if (kG32)  // apply_pair's statements with g z from the shared SGPR pair
            p = apply_tail<FKS_BF16, MODE>(p, rnd2<FKS_BF16>(k & 1 ? pk_mul_half<1>(gg[k >> 1], FKS_BS_Z(k)) : pk_mul_half<0>(gg[k >> 1], FKS_BS_Z(k))),
                                           sl.lr, sl.wd, sl.wdf != 0);
          else
            p = apply_pair<FKS_BF16, MODE>(p, FKS_BS_Z(k), gk[k], sl.lr, sl.wd, sl.wdf != 0, 0.0f);
        }
        // the lookups of one byte column (8 seeds) at a time: hoisting all 64 table reads
        // ahead of the chain would spill
        if ((k % kBsFence) == kBsFence - 1) asm volatile("" ::: "memory");
      }
    }
#undef FKS_BS_Z
    if (kD16) {  // p is bf16-exact: the high halves are the elements
      Traits<FKS_BF16>::store_hi(sl.addr, __float_as_uint(p.x));
      Traits<FKS_BF16>::store_hi(sl.addr + 16, __float_as_uint(p.y));
      return;
    }
    const uint32_t b1v = ST::bits(p.x), b2v = ST::bits(p.y);
    const uint32_t back = swap_adjacent(odd ? b1v : b2v);
    const Pair out = odd ? ST::pack(back, b2v) : ST::pack(b1v, back);
    ST::store_pair(sl.addr, out);
  };

  const bool ordered = !split;  // half 1 depends on half 0's stores
  // ---- half 0 publishes its task m's parameters as stored (the wave's global stores
  // done: vmcnt(0), the workgroup-scope release); half 1 waits for that before loading them
  const uint32_t prog = kBsProgOff + 4u * (uint32_t)hw;
  auto publish_stored = [&](const int m) {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    if (lane == 0) *(volatile lds_u32_t*)(size_t)prog = (uint32_t)m + 1u;
  };
  auto await_stored = [&](const int m) {
    if (m >= ntask) return;
    const uint32_t pm = kBsProgOff + 4u * (uint32_t)(m % kBsWaves);
    while (__builtin_amdgcn_readfirstlane(bs_flag_load(pm)) < (uint32_t)m + 1u) __builtin_amdgcn_s_sleep(1);
    asm volatile("" ::: "memory");
  };
  // The lag bound.  Nothing else keeps half 0 from running ahead of half 1 (it wins the
  // VALU arbitration by age), and with the longer weight-decay chain half 1 fell so far
  // behind that its loads of half 0's output came back from HBM (7.9 B/param per launch,
  // profiles/pmc_apply_r04_full.json).  Half 1 publishes each task as applied; half 0 waits
  // for task n - FKS_BS_LAG before twisting task n.  Half 1's task m needs half 0's task
  // m + 2 kBsWaves (publish_stored), so the bound must exceed 2 kBsWaves = 12.
  static_assert(FKS_BS_LAG == 0 || FKS_BS_LAG > 2 * kBsWaves, "FKS_BS_LAG: half 1 trails by 12 tasks");
  // only the weight-decay chains need it: the wd 0 / None chains keep half 1 within L2 reach
  // unaided (4.17 B/param), and there the bound measured 1.4 % slower (profiles/r05d_ab_lag.log)
  constexpr bool kLag = FKS_BS_LAG > 0 && (MODE == kModeUpdateWd || MODE == kModeUpdate);
  const uint32_t prog1 = kBsProg1Off + 4u * (uint32_t)hw;
  auto publish_applied = [&](const int m) {
    if (lane == 0) *(volatile lds_u32_t*)(size_t)prog1 = (uint32_t)m + 1u;
  };
  auto await_applied = [&](const int m) {
    if (m < 0) return;
    const uint32_t pm = kBsProg1Off + 4u * (uint32_t)(m % kBsWaves);
    while (__builtin_amdgcn_readfirstlane(bs_flag_load(pm)) < (uint32_t)m + 1u) __builtin_amdgcn_s_sleep(1);
  };

  // ---- task n: wait for task n-1's twist, twist, publish, chain; fetches task n + 6
  // into nx (past the last task: the sink)
  auto task = [&](const int n, const Slot& sl, Slot& nx) {
    uint32_t oa[8], ob[8];
    if (kLag && ordered && half == 0) await_applied(n - FKS_BS_LAG);
    if (kH1) tw_pre();
    __builtin_amdgcn_s_setprio(2);
    while (__builtin_amdgcn_readfirstlane(bs_flag_load(flag)) < (uint32_t)n) __builtin_amdgcn_s_sleep(0);
    asm volatile("" ::: "memory");
    twist(n, oa, ob);
    if (lane == 0) bs_flag_store(flag, (uint32_t)n + 1u);
    __builtin_amdgcn_s_setprio(0);
    if (ordered && half == 0) {
      if (n >= kBsWaves) publish_stored(n - kBsWaves);  // the store of the wave's previous task
    } else if (ordered) {
      await_stored(n + kBsWaves);
    }
    float rv[4 * kRv + 1];
    if (kRv > 0) chain_head(oa, ob, rv);
    nx = fetch(n + kBsWaves);
    chain(sl, oa, ob, rv);
    if (kLag && ordered && half) publish_applied(n);
  };

  // two named slots and a loop unrolled by two: a slot copy on the back edge would wait
  // for the load -- and the store before it -- at the top of every task
  if (hw >= ntask) { stamp(); return; }
  if (ordered && half) await_stored(hw);
  Slot s0 = fetch(hw), s1;
  int n = hw;
  for (;;) {
    task(n, s0, s1);
    if (n + kBsWaves >= ntask) break;
    n += kBsWaves;
    next_row();
    task(n, s1, s0);
    if (n + kBsWaves >= ntask) break;
    n += kBsWaves;
    next_row();
  }
  if (ordered && half == 0) publish_stored(n);  // the wave's last task
  stamp();
}

}  // namespace
}  // namespace fks
