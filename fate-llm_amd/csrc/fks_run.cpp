// fks_run.cpp -- the launch driver of libfks.so: seed batching, workspace carving and the
// kernel launches of every call, with fks_profile_begin/end's events around them.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>

#include "fks_host.h"

namespace fks {
namespace {

// launch-time instrumentation (fks_profile_begin/end): events around every launch
struct Prof {
  bool on = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[2];  // 0 = apply, 1 = jump
};
Prof g_prof;
std::mutex g_prof_mu;

template <class F>
int timed(int which, void* stream, F&& launch) {
  std::unique_lock<std::mutex> lk(g_prof_mu);
  if (!g_prof.on) {
    lk.unlock();
    return launch();
  }
  hipEvent_t a, b;
  (void)hipEventCreate(&a);
  (void)hipEventCreate(&b);
  (void)hipEventRecord(a, (hipStream_t)stream);
  const int rc = launch();
  (void)hipEventRecord(b, (hipStream_t)stream);
  g_prof.ev[which].emplace_back(a, b);
  return rc;
}

// a launcher's result: 0, a hipError_t, or a negative FKS code (`neg` says what it means)
void check_launch(int rc, const char* what, const char* neg = "unsupported") {
  if (rc) throw Error(rc < 0 ? rc : -FKS_EHIP, std::string(what) + " launch: " +
                                                 (rc > 0 ? hipGetErrorString((hipError_t)rc) : neg));
}
void check_hip(hipError_t e, const char* what) {
  if (e != hipSuccess) throw Error(-FKS_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

// Records a cache buffer's event on the call's stream after the call's launches: by record()
// where the call succeeded, by the destructor where it throws -- a launch error still orders the
// buffer after the launches already queued, so a next call on another stream cannot overtake them.
struct RecordAfter {
  DevBuf* b;
  void* stream;
  JWin* drop_on_throw = nullptr;  // a failed launch leaves sets assigned but not jumped: drop them all
  int record() {
    DevBuf* const x = b;
    b = nullptr;
    drop_on_throw = nullptr;
    return x ? buf_record(*x, stream) : 0;
  }
  ~RecordAfter() {
    if (drop_on_throw) jw_drop(*drop_on_throw);
    (void)record();
  }
};

// the jump of nb seeds to the chunk starts of the header's table at off_cb (its polynomials at off_polys)
JumpArgs jump_args(const uint64_t* seeds, int nb, const uint8_t* hdr, size_t off_polys, size_t off_cb, uint32_t* states,
                   int nchunks) {
  JumpArgs ja{};
  for (int j = 0; j < nb; j++) ja.seeds[j] = seeds[j];
  ja.polys = reinterpret_cast<const uint64_t*>(hdr + off_polys);
  ja.chunk_block = reinterpret_cast<const int64_t*>(hdr + off_cb);
  ja.states = states;
  ja.nchunks = nchunks;
  return ja;
}

// Chunks per jump workgroup (one chunk per wave, 16 waves, one workgroup per CU by
// LDS): enough workgroups to cover every CU before packing chunks into fewer groups.
int jump_chunks_per_wg(int nseeds, int nchunks, int cus) {
  const int per_cu = (int)(((int64_t)nseeds * nchunks + cus - 1) / cus);
  return std::max(1, std::min({kJumpMaxCpw, per_cu, nchunks}));
}

// the torch_rocm stream: seeds in passes of kPhxSeeds (by value in the kernel arguments);
// element shards split the work items
void run_philox(const fks_tensor* t, int nt, const uint64_t* seeds, const double* values, int k, int value_kind,
                int mode, void* stream, const double* scales, int shard, int nshards, const float* gdev,
                uint64_t delta_base) {
  if (mode != kModeUpdate && mode != kModePerturb && mode != kModePerturbUpdate && mode != kModeWriteZ &&
      mode != kModeDelta)
    throw Error(-FKS_ENOTSUP, "the torch_rocm stream supports the reconstruct, perturb, normal and delta calls only");
  std::lock_guard<std::mutex> lk(g_cache_mu);
  const PhxPlan* P = get_phx_plan(t, nt, scales, mode == kModeDelta ? delta_base : 0, device_caps());
  PhiloxArgs a{};
  a.t = static_cast<const PhxTensor*>(P->dev);
  a.nt = P->nt;
  a.gdev = gdev;
  a.mode = mode == kModeUpdate ? P->wd_mode : mode;
  a.item_lo = phx_boundary(*P, shard, nshards);
  a.item_hi = phx_boundary(*P, shard + 1, nshards);
  if (a.item_lo >= a.item_hi) return;
  if (a.mode == kModeUpdateWd0 && P->wd_pos0 && !env_on("FKS_PHX_KEEP_WD_FMA")) {
    // kModeUpdateWdPos0 when |lr g z| stays <= 1e30 for every seed (|z| <= 6.67: the
    // largest Box-Muller radius is sqrt(-2 ln 2^-32) = 6.66): no overflow, so t = gz
    double gmax = 0.0;
    bool finite = std::isfinite((double)P->max_lr);
    for (int j = 0; j < k && finite; j++)
      for (int d = 0; d < 2; d++) {  // FKS_F32, FKS_BF16: the g the kernels see
        const float g = g_value(value_kind, values[j], d);
        finite = finite && std::isfinite(g);
        gmax = std::max(gmax, (double)std::fabs(g));
      }
    if (finite && gmax * 6.67 <= 1e37 && gmax * 6.67 * (double)P->max_lr <= 1e30) a.mode = kModeUpdateWdPos0;
  }
  for (int s0 = 0; s0 < k; s0 += kPhxSeeds) {
    const int nb = std::min(kPhxSeeds, k - s0);
    for (int j = 0; j < nb; j++) {
      a.seeds[j] = seeds[s0 + j];
      for (int d = 0; d < 3; d++) a.g[3 * j + d] = g_value(value_kind, values[s0 + j], d);
    }
    a.nseeds = nb;
    a.call_first = s0 == 0 ? 1 : 0;
    check_launch(timed(0, stream, [&] { return launch_philox(a, stream); }), "fks_philox_kernel");
  }
}

}  // namespace

// Core: run `k` seeds (update / perturb / write-z) over the tensor list.
void run(const fks_tensor* t, int nt, const uint64_t* seeds, const double* values, int k, int value_kind, int mode,
         void* workspace, size_t ws_bytes, void* stream, const double* tensor_scales, int shard, int nshards,
         uint64_t delta_base, const float* gdev) {
  validate(t, nt);
  check_shard(shard, nshards);
  if (k < 0 || (k > 0 && (!seeds || !values))) throw Error(-FKS_EINVAL, "bad seed/value arrays");
  if (value_kind != FKS_VALUE_SCALAR && value_kind != FKS_VALUE_TENSOR) throw Error(-FKS_EINVAL, "bad value_kind");
  if (k == 0 || nt == 0) return;
  if (rocm_stream(t, nt)) {
    run_philox(t, nt, seeds, values, k, value_kind, mode, stream, tensor_scales, shard, nshards, gdev, delta_base);
    return;
  }
  const bool small = k <= kSmallK;
  const bool libm = libm_flavour(t, nt);
  const DevCaps dc = device_caps();
  std::lock_guard<std::mutex> lk(g_cache_mu);  // no eviction while this call uses its entry
  const CachedPlan* C = get_plan(t, nt, tensor_scales, delta_base, shard, nshards, small, dc);
  if (!C->have_reg && !C->have_irr) return;
  const int per_pass = small ? kSmallK : kMaxSeedsPerPass;
  // bf16 fast segments of a reconstruct (or delta accumulation) of more than one
  // 19-seed pass go to the bit-sliced slice kernel, 32 seeds per pass
  const bool use_bs = C->have_bs && k >= kBsMinSeeds && (mode == kModeUpdate || mode == kModeDelta);
  // what this plan's launches need (fks_workspace_size's upper bound plays no part here)
  size_t need = ws_bytes_for(std::max(C->Z.reg_chunks, C->Z.irr_chunks), std::min(per_pass, k));
  // (a slice pass holds <= 64 seeds x half the plan chunks, a split pass <= 32 x all of them)
  if (use_bs) need = std::max(need, ws_bytes_for(C->Z.bs_chunks, std::min(kBsSeeds, k)));
  if (!workspace || ws_bytes < need)
    throw Error(-FKS_EINVAL, "workspace too small: need " + std::to_string(need) + " bytes, got " +
                                 std::to_string(ws_bytes));
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  const uint8_t* hdr = static_cast<const uint8_t*>(C->dev);
  uint32_t* states = reinterpret_cast<uint32_t*>(ws + kWsStatesOff);
  // one-seed bf16 calls: store the table indices (a perturb) or replay them (a later call
  // with the same seed inside the stored block range): ZCache
  ZCache* Zc = nullptr;
  int zmode = 0;
  const bool z_mode_ok = mode == kModePerturb || mode == kModePerturbUpdate || mode == kModeUpdate;
  if (k == 1 && small && !use_bs && C->have_reg && C->nsegs[FKS_BF16] > 0 && z_mode_ok) {
    Zc = z_cache(stream, (size_t)kSm2ZidxBytesPerBlock * (size_t)(C->reg_hi - C->reg_lo));
    if (Zc) {
      if (Zc->valid && Zc->seed == seeds[0] && Zc->bf16_hash == C->bf16_hash && Zc->lo <= C->reg_lo &&
          C->reg_hi <= Zc->hi) {
        zmode = 2;
      } else if (mode == kModePerturb) {
        zmode = 1;
        Zc->valid = false;  // until this call's store is launched
        Zc->lo = C->reg_lo;
        Zc->hi = C->reg_hi;
        Zc->bf16_hash = C->bf16_hash;
      } else {
        Zc = nullptr;
      }
    }
  }
  // one-seed calls: the regular and irregular windows in the per-device window cache,
  // jumped only when the seed or the chunk starts changed since the last call
  uint32_t* reg_states = states;
  uint32_t* irr_states = states;
  bool reg_cached = false, irr_cached = false, reg_jumped = false;
  WinCache* W = nullptr;
  if (k == 1 && !use_bs) {
    const size_t reg_words = (size_t)kMtN * (C->have_reg ? C->Z.reg_chunks : 0);
    const size_t irr_words = (size_t)kMtN * (C->have_irr ? C->Z.irr_chunks : 0);
    W = win_cache(stream, sizeof(uint32_t) * std::max<size_t>(reg_words + irr_words, 1));
    if (W) {
      reg_states = static_cast<uint32_t*>(W->b.buf);
      irr_states = reg_states + reg_words;
      const bool hit = W->valid && W->seed == seeds[0] && W->chunk_hash == C->chunk_hash;
      reg_cached = irr_cached = hit;
      W->valid = false;  // until this call's jumps are launched
    }
  }
  RecordAfter z_after{Zc ? &Zc->b : nullptr, stream}, w_after{W ? &W->b : nullptr, stream};
  auto gval = [&](int s, int d) { return g_value(value_kind, values[s], d); };
  if (use_bs) {
    // Passes of 64 seeds as two slices per chunk pair (one jump per seed and chunk PAIR),
    // the remainder of <= 32 seeds one slice per plan chunk.  The apply costs the same per
    // seed either way (6.785 ms per 64 seeds against 2 x 3.388 ms over 2^28 parameters,
    // profiles/r03y_*ab.log) and half the jumps go: the 7B bench 10.92 s against 11.03 s
    // for 32-seed passes on one box (profiles/r03g_*.log).  FKS_BS_SLICES=1 forces 32-seed
    // passes (diagnostics, A/B).
    int slices = 2;
    if (const char* e = std::getenv("FKS_BS_SLICES")) slices = (e[0] == '1') ? 1 : 2;
    const int per_pass = slices == 2 ? kBsPassSeeds : kBsSeeds;
    // two-slice passes keep their windows in the reconstruct window cache when one is
    // attached (fks_jwin_attach): a seed already there skips its jump
    JWin* J = (slices == 2 && k > kBsSeeds) ? jw_cache(stream, C->bs_hash, C->Z.bs_chunks / kBsChunksPerWg) : nullptr;
    RecordAfter j_after{J ? &J->b : nullptr, stream, J};
    // kModeUpdateWdPos0 under run_philox's conditions (fks_internal.h): every bf16 fast segment has
    // wd = +0.0 and a finite lr, and |lr g z| stays <= 1e30 for every seed of the call (|z| <= 6.67
    // bounds the bf16 table's radii too).  FKS_BS_KEEP_WD_FMA=1 keeps the fma form (tests, A/B).
    int bs_mode = mode == kModeUpdate ? C->wd_mode[FKS_BF16] : mode;
    if (bs_mode == kModeUpdateWd0 && C->bs_wd_pos0 && !env_on("FKS_BS_KEEP_WD_FMA")) {
      double gmax = 0.0;
      bool finite = std::isfinite((double)C->bs_max_lr);
      for (int j = 0; j < k && finite; j++) {
        const float g = gval(j, FKS_BF16);
        finite = finite && std::isfinite(g);
        gmax = std::max(gmax, (double)std::fabs(g));
      }
      if (finite && gmax * 6.67 <= 1e37 && gmax * 6.67 * (double)C->bs_max_lr <= 1e30) bs_mode = kModeUpdateWdPos0;
    }
    for (int s0 = 0; s0 < k; s0 += per_pass) {
      const int nb = std::min(per_pass, k - s0);
      // > 32 seeds: two slices per chunk pair (jumps to every other plan boundary);
      // <= 32: one slice per plan chunk
      const bool split = nb <= kBsSeeds;
      const int nch = split ? C->Z.bs_chunks : C->Z.bs_chunks / kBsChunksPerWg;
      JumpArgs ja = jump_args(seeds + s0, nb, hdr, C->H.off_bs_polys, C->H.off_bs_cb, states, nch);
      ApplyBsArgs ba{};
      int njump = nb;
      ba.states = states;
      if (J && !split) {
        jw_assign(J->sets, seeds + s0, nb, ba.slot, ja.seeds, ja.slot, njump);
        ja.states = static_cast<uint32_t*>(J->b.buf);
        ba.states = ja.states;
        ja.use_slot = ba.use_slot = 1;
      }
      ja.stride = split ? 1 : kBsChunksPerWg;
      ja.chunks_per_wg = std::max(1, std::min(njump * nch >= 4096 ? 32 : 16, nch));
      if (njump > 0) check_launch(timed(1, stream, [&] { return launch_jump(ja, njump, stream); }), "fks_jump_kernel");
      for (int j = 0; j < nb; j++) ba.g[j] = gval(s0 + j, FKS_BF16);
      ba.segs = reinterpret_cast<const DevSeg*>(hdr + C->seg_off[FKS_BF16]);
      ba.chunk_block = ja.chunk_block;
      ba.sink = reinterpret_cast<uint64_t*>(ws);
      ba.nsegs = C->nsegs[FKS_BF16];
      ba.nchunks = nch;
      ba.split = split ? 1 : 0;
      ba.nseeds = nb;
      ba.mode = bs_mode;
      check_launch(timed(0, stream, [&] { return launch_apply_bs(ba, stream); }), "fks_apply_bs_kernel");
    }
    (void)j_after.record();
  }
  // the 19-seed kernels: every other regular dtype (all of them without the slice kernel)
  bool reg_rest = false;
  for (int d = 0; d < 3; d++) reg_rest = reg_rest || (C->nsegs[d] && !(use_bs && d == FKS_BF16));
  for (int s0 = 0; s0 < k; s0 += kMaxSeedsPerPass) {
    const int nb = std::min(kMaxSeedsPerPass, k - s0);
    if (reg_rest) {
      JumpArgs ja = jump_args(seeds + s0, nb, hdr, C->H.off_polys, C->H.off_cb, reg_states, C->Z.reg_chunks);
      ja.chunks_per_wg = jump_chunks_per_wg(nb, C->Z.reg_chunks, dc.cus);
      // a replay needs no windows unless another dtype's segments still generate
      const bool need_windows = zmode != 2 || C->nsegs[FKS_F32] > 0 || C->nsegs[FKS_F16] > 0;
      if (!reg_cached && need_windows) {
        check_launch(timed(1, stream, [&] { return launch_jump(ja, nb, stream); }), "fks_jump_kernel");
        reg_jumped = true;
      }
      for (int d = 0; d < 3; d++) {
        if (!C->nsegs[d] || (use_bs && d == FKS_BF16)) continue;
        ApplyArgs aa{};
        aa.states = reg_states;
        for (int j = 0; j < nb; j++) aa.g[j] = gval(s0 + j, d);
        aa.segs = reinterpret_cast<const DevSeg*>(hdr + C->seg_off[d]);
        aa.chunk_block = ja.chunk_block;
        aa.sink = reinterpret_cast<uint64_t*>(ws);
        aa.gdev = gdev;
        if (Zc && d == FKS_BF16) {
          aa.zidx = static_cast<uint32_t*>(Zc->b.buf);
          aa.zlo = Zc->lo;
          aa.zmode = zmode;
        }
        aa.nsegs = C->nsegs[d];
        aa.nchunks = C->Z.reg_chunks;
        aa.nseeds = nb;
        aa.mode = mode == kModeUpdate ? C->wd_mode[d] : mode;  // weight-decay select specialised away
        const int dd = (d == FKS_F32 && libm) ? kDtF32Libm : d;
        check_launch(timed(0, stream, [&] { return launch_apply(dd, aa, stream); }), "fks_apply_kernel");
      }
    }
    if (C->have_irr) {
      JumpArgs ja = jump_args(seeds + s0, nb, hdr, C->H.off_ipolys, C->H.off_ilo, irr_states, C->Z.irr_chunks);
      ja.chunks_per_wg = std::max(1, std::min(32, C->Z.irr_chunks));
      if (!irr_cached) check_launch(timed(1, stream, [&] { return launch_jump(ja, nb, stream); }), "fks_jump_kernel");
      IrrArgs ia{};
      ia.states = irr_states;
      for (int d = 0; d < 3; d++)
        for (int j = 0; j < nb; j++) ia.g[d][j] = gval(s0 + j, d);
      ia.runs = reinterpret_cast<const DevRun*>(hdr + C->H.off_runs);
      ia.tiny = reinterpret_cast<const DevTiny*>(hdr + C->H.off_tiny);
      ia.chunk_lo = ja.chunk_block;
      ia.chunk_hi = reinterpret_cast<const int64_t*>(hdr + C->H.off_ihi);
      ia.gdev = gdev;
      ia.nruns = C->Z.nruns;
      ia.ntiny = C->Z.ntiny;
      ia.nchunks = C->Z.irr_chunks;
      ia.nseeds = nb;
      ia.mode = mode;
      ia.libm = libm ? 1 : 0;
      check_launch(timed(0, stream, [&] { return launch_irregular(ia, stream); }), "fks_irregular_kernel");
    }
  }
  if (W) {  // this call's windows are in the cache (jumped now or reused), stream-ordered
    // (a replay that skipped the jump did not write the regular windows)
    W->valid = reg_cached || reg_jumped || !C->have_reg;
    W->seed = seeds[0];
    W->chunk_hash = C->chunk_hash;
  }
  if (Zc && zmode == 1) {  // stored now (zmode 1) or read (zmode 2): stream-ordered like the windows
    Zc->valid = true;
    Zc->seed = seeds[0];
  }
  const int w_rc = w_after.record(), z_rc = z_after.record();
  if (w_rc) throw Error(-FKS_EHIP, "window cache event");
  if (z_rc) throw Error(-FKS_EHIP, "z-index cache event");
}

void profile_begin() {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof.on = true;
}

void profile_end(double* apply_ms, int64_t* n_apply, double* jump_ms, int64_t* n_jump) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  double tot[2] = {0.0, 0.0};
  for (int w = 0; w < 2; w++) {
    for (auto& e : g_prof.ev[w]) {
      (void)hipEventSynchronize(e.second);
      float ms = 0.0f;
      (void)hipEventElapsedTime(&ms, e.first, e.second);
      tot[w] += ms;
      (void)hipEventDestroy(e.first);
      (void)hipEventDestroy(e.second);
    }
  }
  if (apply_ms) *apply_ms = tot[0];
  if (jump_ms) *jump_ms = tot[1];
  if (n_apply) *n_apply = (int64_t)g_prof.ev[0].size();
  if (n_jump) *n_jump = (int64_t)g_prof.ev[1].size();
  g_prof.ev[0].clear();
  g_prof.ev[1].clear();
  g_prof.on = false;
}

void delta_apply(const fks_tensor* t, int nt, const float* delta, const double* decay, void* workspace,
                 size_t ws_bytes, void* stream) {
  thread_local std::vector<DeltaApplyDesc> d;  // the upload's source outlives the call
  d.clear();
  int64_t cum = 0, maxn = 0;
  for (int i = 0; i < nt; i++) {
    if (t[i].numel > 0 && !(t[i].flags & FKS_FROZEN)) {
      DeltaApplyDesc x{};
      x.ptr = (uint64_t)(uintptr_t)t[i].data;
      x.numel = t[i].numel;
      x.delta_off = cum;
      x.dtype = t[i].dtype;
      x.decay = (float)decay[i];
      d.push_back(x);
      maxn = std::max(maxn, t[i].numel);
    }
    cum += t[i].numel;
  }
  if (d.empty()) return;
  const size_t need = sizeof(DeltaApplyDesc) * d.size();
  if (ws_bytes < need) throw Error(-FKS_EINVAL, "workspace too small");
  check_hip(hipMemcpyAsync(workspace, d.data(), need, hipMemcpyHostToDevice, (hipStream_t)stream), "hipMemcpyAsync");
  const int rc = launch_delta_apply(static_cast<const DeltaApplyDesc*>(workspace), (int)d.size(), maxn, delta, stream);
  check_hip((hipError_t)rc, "fks_delta_apply_kernel launch");
}

void digest(const fks_tensor* t, int nt, uint64_t pos0, uint64_t* dev_out2, void* stream) {
  check_hip(hipMemsetAsync(dev_out2, 0, 2 * sizeof(uint64_t), (hipStream_t)stream), "hipMemsetAsync");
  // the non-empty tensors in launches of kDigTensors, each adding its part to dev_out2
  // (digests of disjoint element ranges combine by add and xor)
  DigestArgs a{};
  a.out = dev_out2;
  auto flush = [&] {
    if (a.nt == 0) return;
    check_hip((hipError_t)launch_digest(a, stream), "fks_digest_kernel launch");
    a.nt = 0;
    a.ntiles = 0;
  };
  uint64_t q = pos0;
  for (int i = 0; i < nt; i++) {
    const fks_tensor& x = t[i];
    if (x.numel == 0) continue;
    const int64_t es = (int64_t)elem_size(x.dtype), epv = 16 / es;
    const int64_t to16 = (int64_t)((16 - (uintptr_t)x.data % 16) % 16) / es;
    const int64_t nv = (x.numel - std::min(to16, x.numel)) / epv;  // whole aligned 16-byte vectors
    DigestTensor& d = a.t[a.nt++];
    d.ptr = (uint64_t)(uintptr_t)x.data;
    d.numel = x.numel;
    d.q1 = q + 1;
    d.tile0 = a.ntiles;
    d.dtype = x.dtype;
    a.ntiles += std::max<int64_t>(1, (nv + kDigVecPerTile - 1) / kDigVecPerTile);
    q += (uint64_t)x.numel;
    if (a.nt == kDigTensors) flush();
  }
  flush();
}

void device_selfcheck(int which, uint64_t* result, void* workspace, size_t ws_bytes, void* stream) {
  const size_t need = sizeof(uint32_t) * (size_t)kSqrtDomainBlocks;
  if (!workspace || ws_bytes < need) throw Error(-FKS_EINVAL, "workspace too small");
  uint32_t* counts = static_cast<uint32_t*>(workspace);
  const int rc = which == FKS_CHECK_SQRT_DOMAIN     ? launch_sqrt_domain_check(counts, stream)
                 : which == FKS_CHECK_PHILOX_RADIUS ? launch_philox_radius_check(counts, stream)
                                                    : launch_philox_fast_radius_check(counts, stream);
  check_hip((hipError_t)rc, "self check launch");
  std::vector<uint32_t> h((size_t)kSqrtDomainBlocks);
  if (hipMemcpyAsync(h.data(), counts, need, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
      hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
    throw Error(-FKS_EHIP, "sqrt domain check copy");
  uint64_t bad = 0;
  for (uint32_t v : h) bad = which == FKS_CHECK_PHILOX_BF16_RADIUS ? std::max<uint64_t>(bad, v) : bad + v;
  *result = bad;
}

// ---- seed-basis projection (torch_rocm stream) ----
// fks_project_multi's workspace: the vector table of the whole call ([nvec][entries], uploaded
// once per call) in front, then the block partials of one pass of at most kProjMaxVec vectors
static size_t project_table_bytes(int entries, int nvec) {
  return align_up(sizeof(ProjVecEntry) * (size_t)std::max(entries, 0) * (size_t)std::max(nvec, 0), 256);
}
// ... and the block partials a launch over `items` work items writes (fks_project.hip)
static size_t project_need(int64_t items, int entries, int nvec, bool multi) {
  const size_t part = std::max<size_t>(sizeof(double) * (size_t)kPhxSeeds * (size_t)project_grid(items), 256);
  return multi ? project_table_bytes(entries, nvec) + (size_t)std::min(std::max(nvec, 1), kProjMaxVec) * part : part;
}

// a shard walks at most the whole list's items; the passes of kPhxSeeds seeds follow
// each other on the stream and share the partials
size_t project_ws_bytes(const fks_tensor* t, int nt, int nvec, bool multi) {
  const PhxGeo geo = phx_geometry(t, nt, nullptr, 0, device_caps().max_grid);
  return project_need(geo.items, geo.nt, nvec, multi);
}

void project(const fks_tensor* t, int nt, const uint64_t* seeds, int k, const float* vec, const fks_vec* vecs,
             int nvec, int shard, int nshards, double* dev_out, void* workspace, size_t ws_bytes, void* stream) {
  const bool multi = vec == nullptr;
  // the geometry on the host first: the workspace is checked before anything is allocated or launched.
  // fks_project's table is fks_delta_accumulate's for this base; fks_project_multi's is geometry only
  const uint64_t base = (uint64_t)(uintptr_t)vec;
  const DevCaps dc = device_caps();
  PhxGeo geo;
  int64_t lo = 0, hi = 0;
  if (nt > 0) {
    geo = phx_geometry(t, nt, nullptr, base, dc.max_grid);
    lo = phx_boundary(geo, shard, nshards);
    hi = phx_boundary(geo, shard + 1, nshards);
  }
  if (lo >= hi) {  // nothing in this shard: every projection is +0
    const size_t bytes = sizeof(double) * (size_t)k * (size_t)nvec;
    check_hip(hipMemsetAsync(dev_out, 0, bytes, (hipStream_t)stream), "hipMemsetAsync");
    return;
  }
  const size_t tab_bytes = multi ? project_table_bytes(geo.nt, nvec) : 0;
  const size_t need = project_need(hi - lo, geo.nt, nvec, multi);
  if (!workspace || ((uintptr_t)workspace % 8) != 0 || ws_bytes < need)
    throw Error(-FKS_EINVAL, "workspace too small or misaligned: need " + std::to_string(need) + " bytes, got " +
                                 std::to_string(ws_bytes));
  thread_local std::vector<ProjVecEntry> host;
  if (multi) {  // every vector's piece per table entry (a tensor past 2^31 bytes has several entries)
    std::vector<int64_t> start((size_t)nt, 0);  // the tensors' first elements in the concatenation
    for (int i = 1; i < nt; i++) start[i] = start[i - 1] + t[i - 1].numel;
    host.assign((size_t)nvec * (size_t)geo.nt, ProjVecEntry{});
    for (int m = 0; m < nvec; m++)
      for (int e = 0; e < geo.nt; e++) {
        const int i = geo.tensor_of[e];
        const fks_vec& v = vecs[(size_t)m * (size_t)nt + (size_t)i];
        ProjVecEntry& x = host[(size_t)m * (size_t)geo.nt + (size_t)e];
        x.ptr = (uint64_t)(uintptr_t)v.data + (uint64_t)(geo.elem0[e] - start[i]) * elem_size(v.dtype);
        x.dtype = v.dtype;
        x.flags = (x.ptr % 16u) == 0 ? kPhxP16 : 0u;
      }
  }
  std::lock_guard<std::mutex> lk(g_cache_mu);  // no eviction while this call uses its entry
  const PhxPlan* P = get_phx_plan(t, nt, nullptr, base, dc);
  if (multi) {
    if (P->nt != geo.nt) throw Error(-FKS_EINVAL, "torch_rocm plan does not match the call's geometry");
    check_hip(hipMemcpyAsync(workspace, host.data(), sizeof(ProjVecEntry) * host.size(), hipMemcpyHostToDevice,
                             (hipStream_t)stream), "hipMemcpyAsync");
  }
  double* const partial = reinterpret_cast<double*>(static_cast<uint8_t*>(workspace) + tab_bytes);
  const int grid = project_grid(hi - lo);
  auto fill = [&](auto& a, int s0, int nb) {
    a.t = static_cast<const PhxTensor*>(P->dev);
    a.nt = P->nt;
    a.partial = partial;
    a.item_lo = lo;
    a.item_hi = hi;
    for (int j = 0; j < nb; j++) a.seeds[j] = seeds[s0 + j];
    a.nseeds = nb;
  };
  for (int m0 = 0; m0 < nvec; m0 += kProjMaxVec) {  // batches of vectors over the same seeds
    const int nv = std::min(kProjMaxVec, nvec - m0);
    for (int s0 = 0; s0 < k; s0 += kPhxSeeds) {
      const int nb = std::min(kPhxSeeds, k - s0);
      if (multi) {
        ProjectMultiArgs a{};
        fill(a, s0, nb);
        a.nvec = nv;
        a.vt = static_cast<const ProjVecEntry*>(workspace) + (size_t)m0 * (size_t)P->nt;
        check_launch(timed(0, stream, [&] { return launch_project_multi(a, stream); }), "fks_project_multi_kernel",
                     "bad arguments");
      } else {
        ProjectArgs a{};
        fill(a, s0, nb);
        check_launch(timed(0, stream, [&] { return launch_project(a, stream); }), "fks_project_kernel",
                     "bad arguments");
      }
      double* const out = dev_out + (size_t)m0 * (size_t)k + s0;
      check_launch(launch_project_reduce(partial, grid, nb, nv, out, multi ? k : 0, stream),
                   "fks_project_reduce_kernel", "bad arguments");
    }
  }
}

// ---- seed-basis Gram matrix (torch_rocm stream) ----
// fks_gram's workspace: the block partials of ONE pass, kGramRows x kPhxSeeds doubles per workgroup
// of a launch over `items` work items (1 KiB x project_grid(items)); the passes follow each other
// on the stream and share them.  Nothing depends on the seed counts or has the model's size.
static size_t gram_need(int64_t items) {
  return std::max<size_t>(sizeof(double) * (size_t)kGramRows * (size_t)kPhxSeeds * (size_t)project_grid(items), 256);
}

size_t gram_ws_bytes(const fks_tensor* t, int nt) {
  return gram_need(phx_geometry(t, nt, nullptr, 0, device_caps().max_grid).items);
}

void gram(const fks_tensor* t, int nt, const uint64_t* rows, int kr, const uint64_t* cols, int kc, int shard,
          int nshards, double* dev_out, void* workspace, size_t ws_bytes, void* stream) {
  const bool symmetric = cols == nullptr;
  if (symmetric) {
    cols = rows;
    kc = kr;
  }
  // the geometry on the host first: the workspace is checked before anything is allocated or launched
  // (device_caps() reads the device's properties only and falls back to an MI355X's without a
  // device, so the check below is made from the arguments alone, as tests/test_gram_host.py runs it)
  const DevCaps dc = device_caps();
  PhxGeo geo;
  int64_t lo = 0, hi = 0;
  if (nt > 0) {
    geo = phx_geometry(t, nt, nullptr, 0, dc.max_grid);
    lo = phx_boundary(geo, shard, nshards);
    hi = phx_boundary(geo, shard + 1, nshards);
  }
  if (lo >= hi) {  // nothing in this shard: every inner product is +0
    check_hip(hipMemsetAsync(dev_out, 0, sizeof(double) * (size_t)kr * (size_t)kc, (hipStream_t)stream),
              "hipMemsetAsync");
    return;
  }
  const size_t need = gram_need(hi - lo);
  if (!workspace || ((uintptr_t)workspace % 8) != 0 || ws_bytes < need)
    throw Error(-FKS_EINVAL, "workspace too small or misaligned: need " + std::to_string(need) + " bytes, got " +
                                 std::to_string(ws_bytes));
  std::lock_guard<std::mutex> lk(g_cache_mu);  // no eviction while this call uses its entry
  const PhxPlan* P = get_phx_plan(t, nt, nullptr, 0, dc);
  if (P->nt != geo.nt) throw Error(-FKS_EINVAL, "torch_rocm plan does not match the call's geometry");
  const int grid = project_grid(hi - lo);
  GramArgs a{};
  a.t = static_cast<const PhxTensor*>(P->dev);
  a.nt = P->nt;
  a.partial = static_cast<double*>(workspace);
  a.item_lo = lo;
  a.item_hi = hi;
  for (const GramPass& p : gram_passes(kr, kc, symmetric)) {
    for (int m = 0; m < kGramRows; m++) a.rseeds[m] = m < p.nrows ? rows[p.row0 + m] : 0;
    for (int j = 0; j < p.ncols; j++) a.seeds[j] = cols[p.col0 + j];
    a.nrows = p.nrows;
    a.nseeds = p.ncols;
    check_launch(timed(0, stream, [&] { return launch_gram(a, stream); }), "fks_gram_kernel", "bad arguments");
    check_launch(launch_gram_reduce(a.partial, grid, p.nrows, p.ncols, dev_out, kc, p.row0, p.col0, symmetric, stream),
                 "fks_gram_reduce_kernel", "bad arguments");
  }
}

// ---- tiled seed-basis Gram matrix (torch_rocm stream, f64 matrix unit) ----
// fks_gram_tiled's workspace: the block partials of ONE pass, kGtRows x kGtCols doubles per workgroup
// of a launch over `items` work items; the passes follow each other on the stream and share them.
// Nothing depends on the seed counts or has the model's size.
static size_t gram_tiled_need(int64_t items) {
  return std::max<size_t>(sizeof(double) * (size_t)kGtTile * (size_t)gram_tiled_grid(items), 256);
}

size_t gram_tiled_ws_bytes(const fks_tensor* t, int nt) {
  return gram_tiled_need(phx_geometry(t, nt, nullptr, 0, device_caps().max_grid).items);
}

// gram()'s driver over the tile of fks_gram_tiled.h: geometry first, the workspace check before any
// allocation, the geometry-only plan, then per pass the kernel and the reduce with the matrix's
// addressing and the mirror.  Seeds past a pass's counts are padded with 0 (drawn only where their
// 16-block is live, never written out).
void gram_tiled(const fks_tensor* t, int nt, const uint64_t* rows, int kr, const uint64_t* cols, int kc, int shard,
                int nshards, double* dev_out, void* workspace, size_t ws_bytes, void* stream) {
  const bool symmetric = cols == nullptr;
  if (symmetric) {
    cols = rows;
    kc = kr;
  }
  const DevCaps dc = device_caps();
  PhxGeo geo;
  int64_t lo = 0, hi = 0;
  if (nt > 0) {
    geo = phx_geometry(t, nt, nullptr, 0, dc.max_grid);
    lo = phx_boundary(geo, shard, nshards);
    hi = phx_boundary(geo, shard + 1, nshards);
  }
  if (lo >= hi) {  // nothing in this shard: every inner product is +0
    check_hip(hipMemsetAsync(dev_out, 0, sizeof(double) * (size_t)kr * (size_t)kc, (hipStream_t)stream),
              "hipMemsetAsync");
    return;
  }
  const size_t need = gram_tiled_need(hi - lo);
  if (!workspace || ((uintptr_t)workspace % 8) != 0 || ws_bytes < need)
    throw Error(-FKS_EINVAL, "workspace too small or misaligned: need " + std::to_string(need) + " bytes, got " +
                                 std::to_string(ws_bytes));
  std::lock_guard<std::mutex> lk(g_cache_mu);  // no eviction while this call uses its entry
  const PhxPlan* P = get_phx_plan(t, nt, nullptr, 0, dc);
  if (P->nt != geo.nt) throw Error(-FKS_EINVAL, "torch_rocm plan does not match the call's geometry");
  const int grid = gram_tiled_grid(hi - lo);
  GramTiledArgs a{};
  a.t = static_cast<const PhxTensor*>(P->dev);
  a.nt = P->nt;
  a.partial = static_cast<double*>(workspace);
  a.item_lo = lo;
  a.item_hi = hi;
  for (const GramPass& p : gram_tiled_passes(kr, kc, symmetric)) {
    for (int m = 0; m < kGtRows; m++) a.rseeds[m] = m < p.nrows ? rows[p.row0 + m] : 0;
    for (int j = 0; j < kGtCols; j++) a.cseeds[j] = j < p.ncols ? cols[p.col0 + j] : 0;
    a.nrb = (p.nrows + kGtSeeds - 1) / kGtSeeds;
    a.ncb = (p.ncols + kGtSeeds - 1) / kGtSeeds;
    // a column block that holds its row block's seeds takes the row block's operand (the diagonal
    // tile of a symmetric call; the same values either way)
    const int shared = std::min(a.nrb, a.ncb) * kGtSeeds;
    a.diag = std::equal(a.rseeds, a.rseeds + shared, a.cseeds) ? 1 : 0;
    check_launch(timed(0, stream, [&] { return launch_gram_tiled(a, stream); }), "fks_gram_tiled_kernel",
                 "bad arguments");
    check_launch(launch_gram_tiled_reduce(a.partial, grid, p.nrows, p.ncols, dev_out, kc, p.row0, p.col0, symmetric,
                                          stream),
                 "fks_gram_tiled_reduce_kernel", "bad arguments");
  }
}

// ---- seed-basis expansion (torch_rocm stream) ----
// fks_expand_multi's workspace, one per-call table uploaded in stream order: the outputs' pieces
// ([nvec][entries] ProjVecEntry, a tensor past 2^31 bytes has several entries), the seeds ([k] u64),
// then the coefficients as f32, per batch of kExpMaxVec outputs a block [k][outputs of the batch]
struct ExpandWs {
  size_t seeds_off = 0, coef_off = 0, total = 0;
};
static ExpandWs expand_ws(int entries, int k, int nvec) {
  ExpandWs W;
  W.seeds_off = project_table_bytes(entries, nvec);
  W.coef_off = W.seeds_off + align_up(sizeof(uint64_t) * (size_t)std::max(k, 0), 256);
  W.total = W.coef_off + align_up(sizeof(float) * (size_t)std::max(k, 0) * (size_t)std::max(nvec, 0), 256);
  return W;
}

size_t expand_ws_bytes(const fks_tensor* t, int nt, int k, int nvec) {
  return expand_ws(phx_geometry(t, nt, nullptr, 0, device_caps().max_grid).nt, k, nvec).total;
}

// FKS_EXPAND_WORK (read per call): the seed-elements of one launch, an A/B and test switch
int64_t expand_launch_work() {
  if (const char* e = std::getenv("FKS_EXPAND_WORK")) {
    char* end = nullptr;
    const long long v = std::strtoll(e, &end, 10);
    if (end != e && v > 0) return (int64_t)v;
  }
  return kExpLaunchWork;
}

void expand(const fks_tensor* t, int nt, const uint64_t* seeds, const double* coefs, int k, const fks_vec* outs,
            const double* betas, int nvec, int shard, int nshards, void* workspace, size_t ws_bytes, void* stream) {
  // the geometry on the host first: the workspace is checked before anything is allocated or launched
  const DevCaps dc = device_caps();
  const PhxGeo geo = phx_geometry(t, nt, nullptr, 0, dc.max_grid);
  const int64_t lo = phx_boundary(geo, shard, nshards), hi = phx_boundary(geo, shard + 1, nshards);
  if (lo >= hi) return;  // nothing in this shard
  const ExpandWs W = expand_ws(geo.nt, k, nvec);
  if (!workspace || ((uintptr_t)workspace % 8) != 0 || ws_bytes < W.total)
    throw Error(-FKS_EINVAL, "workspace too small or misaligned: need " + std::to_string(W.total) + " bytes, got " +
                                 std::to_string(ws_bytes));
  const std::vector<int64_t> cuts = phx_expand_cuts(geo, lo, hi, k, expand_launch_work());
  thread_local std::vector<uint8_t> host;  // the upload's source outlives the call
  host.assign(W.total, 0);
  {
    std::vector<int64_t> start((size_t)nt, 0);  // the tensors' first elements in the concatenation
    for (int i = 1; i < nt; i++) start[i] = start[i - 1] + t[i - 1].numel;
    ProjVecEntry* ot = reinterpret_cast<ProjVecEntry*>(host.data());
    for (int m = 0; m < nvec; m++)
      for (int e = 0; e < geo.nt; e++) {
        const int i = geo.tensor_of[e];
        const fks_vec& v = outs[(size_t)m * (size_t)nt + (size_t)i];
        ProjVecEntry& x = ot[(size_t)m * (size_t)geo.nt + (size_t)e];
        x.ptr = (uint64_t)(uintptr_t)v.data + (uint64_t)(geo.elem0[e] - start[i]) * elem_size(v.dtype);
        x.dtype = v.dtype;
        x.flags = (x.ptr % 16u) == 0 ? kPhxP16 : 0u;
      }
    if (k > 0) std::memcpy(host.data() + W.seeds_off, seeds, sizeof(uint64_t) * (size_t)k);
    float* c = reinterpret_cast<float*>(host.data() + W.coef_off);
    for (int m0 = 0; m0 < nvec; m0 += kExpMaxVec) {
      const int nv = std::min(kExpMaxVec, nvec - m0);
      float* blk = c + (size_t)k * (size_t)m0;
      for (int s = 0; s < k; s++)
        for (int m = 0; m < nv; m++) blk[(size_t)s * nv + m] = (float)coefs[(size_t)(m0 + m) * (size_t)k + s];
    }
  }
  std::lock_guard<std::mutex> lk(g_cache_mu);  // no eviction while this call uses its entry
  const PhxPlan* P = get_phx_plan(t, nt, nullptr, 0, dc);
  if (P->nt != geo.nt) throw Error(-FKS_EINVAL, "torch_rocm plan does not match the call's geometry");
  check_hip(hipMemcpyAsync(workspace, host.data(), W.total, hipMemcpyHostToDevice, (hipStream_t)stream),
            "hipMemcpyAsync");
  const uint8_t* ws = static_cast<const uint8_t*>(workspace);
  for (int m0 = 0; m0 < nvec; m0 += kExpMaxVec) {  // batches of outputs over the same seeds
    ExpandArgs a{};
    a.t = static_cast<const PhxTensor*>(P->dev);
    a.nt = P->nt;
    a.nvec = std::min(kExpMaxVec, nvec - m0);
    a.ot = reinterpret_cast<const ProjVecEntry*>(ws) + (size_t)m0 * (size_t)P->nt;
    a.seeds = reinterpret_cast<const uint64_t*>(ws + W.seeds_off);
    a.coef = reinterpret_cast<const float*>(ws + W.coef_off) + (size_t)k * (size_t)m0;
    a.nseeds = k;
    for (int m = 0; m < a.nvec; m++) {
      const double beta = betas ? betas[m0 + m] : 0.0;
      a.beta[m] = (float)beta;
      a.read_old |= beta != 0.0 ? 1u << m : 0u;
    }
    for (size_t c = 0; c + 1 < cuts.size(); c++) {  // launches of at most expand_launch_work() seed-elements
      a.item_lo = cuts[c];
      a.item_hi = cuts[c + 1];
      check_launch(timed(0, stream, [&] { return launch_expand_multi(a, stream); }), "fks_expand_multi_kernel",
                   "bad arguments");
    }
  }
}

// ---- seed-basis projection (CPU generator's stream) ----
// The plan fks_delta_accumulate launches for `vec` as its delta buffer; per pass of
// kMaxSeedsPerPass seeds the regular jump, one launch per dtype with fast segments, the irregular
// jump and launch, then the reduce over the rows all of them left.  No window, z-index or
// reconstruct-window cache: the workspace holds the windows, the sink and the partial rows.
void project_mt(const fks_tensor* t, int nt, const uint64_t* seeds, int k, const float* vec, int shard, int nshards,
                double* dev_out, void* workspace, size_t ws_bytes, void* stream) {
  // the layout on the host first: the workspace is checked before anything is allocated or launched
  const DevCaps dc = device_caps();
  const ProjMtWs W = project_mt_ws(t, nt, k, shard, nshards, dc.cus);
  if (!W.work) {  // nothing in this shard: every projection is +0
    check_hip(hipMemsetAsync(dev_out, 0, sizeof(double) * (size_t)k, (hipStream_t)stream), "hipMemsetAsync");
    return;
  }
  if (!workspace || ((uintptr_t)workspace % 8) != 0 || ws_bytes < W.total)
    throw Error(-FKS_EINVAL, "workspace too small or misaligned: need " + std::to_string(W.total) + " bytes, got " +
                                 std::to_string(ws_bytes));
  const bool libm = libm_flavour(t, nt);
  std::lock_guard<std::mutex> lk(g_cache_mu);  // no eviction while this call uses its entry
  const CachedPlan* C = get_plan(t, nt, nullptr, (uint64_t)(uintptr_t)vec, shard, nshards, /*small=*/false, dc);
  int rows = C->have_irr ? C->Z.irr_chunks : 0;
  for (int d = 0; d < 3; d++) rows += C->nsegs[d] ? C->Z.reg_chunks : 0;
  if (rows < 1 || rows > W.rows ||
      ws_bytes_for(std::max(C->Z.reg_chunks, C->Z.irr_chunks), std::min(k, kMaxSeedsPerPass)) > W.partial_off)
    throw Error(-FKS_EINVAL, "the plan does not match the call's workspace layout");
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  const uint8_t* hdr = static_cast<const uint8_t*>(C->dev);
  uint32_t* states = reinterpret_cast<uint32_t*>(ws + kWsStatesOff);
  double* const partial = reinterpret_cast<double*>(ws + W.partial_off);
  for (int s0 = 0; s0 < k; s0 += kMaxSeedsPerPass) {
    const int nb = std::min(kMaxSeedsPerPass, k - s0);
    double* row = partial;
    if (C->have_reg) {
      JumpArgs ja = jump_args(seeds + s0, nb, hdr, C->H.off_polys, C->H.off_cb, states, C->Z.reg_chunks);
      ja.chunks_per_wg = jump_chunks_per_wg(nb, C->Z.reg_chunks, dc.cus);
      check_launch(timed(1, stream, [&] { return launch_jump(ja, nb, stream); }), "fks_jump_kernel");
      for (int d = 0; d < 3; d++) {
        if (!C->nsegs[d]) continue;
        ProjMtArgs pa{};
        pa.states = states;
        pa.segs = reinterpret_cast<const DevSeg*>(hdr + C->seg_off[d]);
        pa.chunk_block = ja.chunk_block;
        pa.sink = reinterpret_cast<const uint64_t*>(ws);
        pa.partial = row;
        pa.nsegs = C->nsegs[d];
        pa.nchunks = C->Z.reg_chunks;
        pa.nseeds = nb;
        const int dd = (d == FKS_F32 && libm) ? kDtF32Libm : d;
        check_launch(timed(0, stream, [&] { return launch_project_mt(dd, pa, stream); }), "fks_project_mt_kernel",
                     "bad arguments");
        row += (size_t)kPhxSeeds * (size_t)C->Z.reg_chunks;
      }
    }
    if (C->have_irr) {
      JumpArgs ja = jump_args(seeds + s0, nb, hdr, C->H.off_ipolys, C->H.off_ilo, states, C->Z.irr_chunks);
      ja.chunks_per_wg = std::max(1, std::min(32, C->Z.irr_chunks));
      check_launch(timed(1, stream, [&] { return launch_jump(ja, nb, stream); }), "fks_jump_kernel");
      ProjMtIrrArgs ia{};
      ia.states = states;
      ia.runs = reinterpret_cast<const DevRun*>(hdr + C->H.off_runs);
      ia.tiny = reinterpret_cast<const DevTiny*>(hdr + C->H.off_tiny);
      ia.chunk_lo = ja.chunk_block;
      ia.chunk_hi = reinterpret_cast<const int64_t*>(hdr + C->H.off_ihi);
      ia.partial = row;
      ia.nruns = C->Z.nruns;
      ia.ntiny = C->Z.ntiny;
      ia.nchunks = C->Z.irr_chunks;
      ia.nseeds = nb;
      ia.libm = libm ? 1 : 0;
      check_launch(timed(0, stream, [&] { return launch_project_mt_irr(ia, stream); }), "fks_project_mt_irr_kernel",
                   "bad arguments");
    }
    check_launch(launch_project_reduce(partial, rows, nb, 1, dev_out + s0, 0, stream), "fks_project_reduce_kernel",
                 "bad arguments");
  }
}

// ---- ... of several vectors, each read where it lies ----
// project_mt over the geometry-only plan (the kModeDelta plan of kProjMtGeoBase: one cache entry
// per tensor list and shard, whatever the vectors' addresses) and a per-call table at the front of
// the workspace, uploaded in stream order: per vector, its piece under every fast segment (the
// dtypes' segments behind each other, as in the plan), run and single element.  The vectors go in
// batches of kProjMtMaxVec over the same seeds; a batch of nv vectors takes its seeds in passes of
// proj_mt_pass_seeds(nv), each the launches of a project_mt pass with rows of nv sums per seed.
void project_mt_multi(const fks_tensor* t, int nt, const uint64_t* seeds, int k, const fks_vec* vecs, int nvec,
                      int shard, int nshards, double* dev_out, void* workspace, size_t ws_bytes, void* stream) {
  const DevCaps dc = device_caps();
  const ProjMtMultiWs W = project_mt_multi_ws(t, nt, k, nvec, shard, nshards, dc.cus);
  if (!W.one.work) {  // nothing in this shard: every projection is +0
    const size_t bytes = sizeof(double) * (size_t)k * (size_t)nvec;
    check_hip(hipMemsetAsync(dev_out, 0, bytes, (hipStream_t)stream), "hipMemsetAsync");
    return;
  }
  if (!workspace || ((uintptr_t)workspace % 8) != 0 || ws_bytes < W.total)
    throw Error(-FKS_EINVAL, "workspace too small or misaligned: need " + std::to_string(W.total) + " bytes, got " +
                                 std::to_string(ws_bytes));
  // the table on the host, from the layout the plan is built from
  Layout L = make_layout(t, nt, nullptr, kProjMtGeoBase);
  clip_segments(L, shard_blocks(L.stream_len, shard, nshards));
  const size_t nsegs = L.segs[0].size() + L.segs[1].size() + L.segs[2].size();
  const size_t E = nsegs + L.runs.size() + L.tiny.size();
  if (E != (size_t)W.one.entries) throw Error(-FKS_EINVAL, "the layout does not match the call's workspace layout");
  std::vector<int64_t> start((size_t)nt, 0);  // the tensors' first elements in the concatenation
  for (int i = 1; i < nt; i++) start[i] = start[i - 1] + t[i - 1].numel;
  thread_local std::vector<ProjMtVecEntry> host;  // the upload's source outlives the call
  host.assign((size_t)nvec * E, ProjMtVecEntry{});
  for (int m = 0; m < nvec; m++) {
    ProjMtVecEntry* x = host.data() + (size_t)m * E;
    // a descriptor of tensor i whose element 0 is element (ptr - base) / 4 of the concatenation
    auto put = [&](int i, uint64_t ptr) {
      const fks_vec& v = vecs[(size_t)m * (size_t)nt + (size_t)i];
      const int64_t e = (int64_t)((ptr - kProjMtGeoBase) / 4) - start[i];
      x->ptr = (uint64_t)(uintptr_t)v.data + (uint64_t)e * elem_size(v.dtype);
      x->dtype = v.dtype;
      x++;
    };
    for (int d = 0; d < 3; d++)
      for (size_t j = 0; j < L.segs[d].size(); j++) put(L.seg_tensor[d][j], L.segs[d][j].ptr);
    for (size_t j = 0; j < L.runs.size(); j++) put(L.run_tensor[j], L.runs[j].ptr);
    for (size_t j = 0; j < L.tiny.size(); j++) put(L.tiny_tensor[j], L.tiny[j].ptr);
  }
  const bool libm = libm_flavour(t, nt);
  std::lock_guard<std::mutex> lk(g_cache_mu);  // no eviction while this call uses its entry
  const CachedPlan* C = get_plan(t, nt, nullptr, kProjMtGeoBase, shard, nshards, /*small=*/false, dc);
  int rows = C->have_irr ? C->Z.irr_chunks : 0;
  for (int d = 0; d < 3; d++) rows += C->nsegs[d] ? C->Z.reg_chunks : 0;
  bool same = (size_t)C->Z.nsegs == nsegs && (size_t)C->Z.nruns == L.runs.size() && (size_t)C->Z.ntiny == L.tiny.size();
  for (int d = 0; d < 3; d++) same = same && (size_t)C->nsegs[d] == L.segs[d].size();
  if (!same || rows < 1 || rows > W.one.rows ||
      ws_bytes_for(std::max(C->Z.reg_chunks, C->Z.irr_chunks), std::min(k, kMaxSeedsPerPass)) > W.one.partial_off)
    throw Error(-FKS_EINVAL, "the plan does not match the call's workspace layout");
  check_hip(hipMemcpyAsync(workspace, host.data(), sizeof(ProjMtVecEntry) * host.size(), hipMemcpyHostToDevice,
                           (hipStream_t)stream), "hipMemcpyAsync");
  const ProjMtVecEntry* table = static_cast<const ProjMtVecEntry*>(workspace);
  uint8_t* ws = static_cast<uint8_t*>(workspace) + W.inner_off;
  const uint8_t* hdr = static_cast<const uint8_t*>(C->dev);
  uint32_t* states = reinterpret_cast<uint32_t*>(ws + kWsStatesOff);
  double* const partial = reinterpret_cast<double*>(ws + W.one.partial_off);
  for (int m0 = 0; m0 < nvec; m0 += kProjMtMaxVec) {  // batches of vectors over the same seeds
    const int nv = std::min(kProjMtMaxVec, nvec - m0);
    const int per_pass = proj_mt_pass_seeds(nv);
    const ProjMtVecEntry* tab = table + (size_t)m0 * E;
    for (int s0 = 0; s0 < k; s0 += per_pass) {
      const int nb = std::min(per_pass, k - s0);
      double* row = partial;
      if (C->have_reg) {
        JumpArgs ja = jump_args(seeds + s0, nb, hdr, C->H.off_polys, C->H.off_cb, states, C->Z.reg_chunks);
        ja.chunks_per_wg = jump_chunks_per_wg(nb, C->Z.reg_chunks, dc.cus);
        check_launch(timed(1, stream, [&] { return launch_jump(ja, nb, stream); }), "fks_jump_kernel");
        size_t seg0 = 0;  // the dtype's first segment in the table row
        for (int d = 0; d < 3; d++) {
          const size_t first = seg0;
          seg0 += (size_t)C->nsegs[d];
          if (!C->nsegs[d]) continue;
          ProjMtMultiArgs pa{};
          pa.states = states;
          pa.segs = reinterpret_cast<const DevSeg*>(hdr + C->seg_off[d]);
          pa.chunk_block = ja.chunk_block;
          pa.sink = reinterpret_cast<const uint64_t*>(ws);
          pa.partial = row;
          pa.pv = tab + first;
          pa.stride = (int64_t)E;
          pa.nsegs = C->nsegs[d];
          pa.nchunks = C->Z.reg_chunks;
          pa.nseeds = nb;
          pa.nvec = nv;
          const int dd = (d == FKS_F32 && libm) ? kDtF32Libm : d;
          check_launch(timed(0, stream, [&] { return launch_project_mt_multi(dd, pa, stream); }),
                       "fks_project_mt_multi_kernel", "bad arguments");
          row += (size_t)kPhxSeeds * (size_t)nv * (size_t)C->Z.reg_chunks;
        }
      }
      if (C->have_irr) {
        JumpArgs ja = jump_args(seeds + s0, nb, hdr, C->H.off_ipolys, C->H.off_ilo, states, C->Z.irr_chunks);
        ja.chunks_per_wg = std::max(1, std::min(32, C->Z.irr_chunks));
        check_launch(timed(1, stream, [&] { return launch_jump(ja, nb, stream); }), "fks_jump_kernel");
        ProjMtIrrMultiArgs ia{};
        ia.states = states;
        ia.runs = reinterpret_cast<const DevRun*>(hdr + C->H.off_runs);
        ia.tiny = reinterpret_cast<const DevTiny*>(hdr + C->H.off_tiny);
        ia.chunk_lo = ja.chunk_block;
        ia.chunk_hi = reinterpret_cast<const int64_t*>(hdr + C->H.off_ihi);
        ia.partial = row;
        ia.rv = tab + nsegs;
        ia.tv = tab + nsegs + L.runs.size();
        ia.stride = (int64_t)E;
        ia.nruns = C->Z.nruns;
        ia.ntiny = C->Z.ntiny;
        ia.nchunks = C->Z.irr_chunks;
        ia.nseeds = nb;
        ia.libm = libm ? 1 : 0;
        ia.nvec = nv;
        check_launch(timed(0, stream, [&] { return launch_project_mt_irr_multi(ia, stream); }),
                     "fks_project_mt_irr_multi_kernel", "bad arguments");
      }
      check_launch(launch_project_reduce(partial, rows, nb, nv, dev_out + (size_t)m0 * (size_t)k + s0, k, stream),
                   "fks_project_reduce_kernel", "bad arguments");
    }
  }
}

// ---- seed-basis Gram matrix (CPU generator's stream) ----
// gram's passes over project_mt_multi's geometry-only plan.  The windows of a pass lie in the
// workspace as the kernels read them, the row tile's first and the column tile's behind them,
// once at the regular and once at the irregular chunk starts: the row tile's are jumped when the
// row tile begins and stay while its column tiles pass, the column tile's are jumped per pass.
// Then the launches of a project_mt pass -- one per dtype with fast segments, the irregular one
// -- and gram's reduce over the rows they left.  No per-call table: nothing is read.
void gram_mt(const fks_tensor* t, int nt, const uint64_t* rows, int kr, const uint64_t* cols, int kc, int shard,
             int nshards, double* dev_out, void* workspace, size_t ws_bytes, void* stream) {
  const bool symmetric = cols == nullptr;
  if (symmetric) {
    cols = rows;
    kc = kr;
  }
  // the layout on the host first: the workspace is checked before anything is allocated or launched
  const DevCaps dc = device_caps();
  GramMtWs W;
  if (nt > 0) W = gram_mt_ws(t, nt, shard, nshards, dc.cus);
  if (!W.work) {  // nothing in this shard: every inner product is +0
    check_hip(hipMemsetAsync(dev_out, 0, sizeof(double) * (size_t)kr * (size_t)kc, (hipStream_t)stream),
              "hipMemsetAsync");
    return;
  }
  if (!workspace || ((uintptr_t)workspace % 8) != 0 || ws_bytes < W.total)
    throw Error(-FKS_EINVAL, "workspace too small or misaligned: need " + std::to_string(W.total) + " bytes, got " +
                                 std::to_string(ws_bytes));
  const bool libm = libm_flavour(t, nt);
  std::lock_guard<std::mutex> lk(g_cache_mu);  // no eviction while this call uses its entry
  const CachedPlan* C = get_plan(t, nt, nullptr, kProjMtGeoBase, shard, nshards, /*small=*/false, dc);
  int prows = C->have_irr ? C->Z.irr_chunks : 0;
  for (int d = 0; d < 3; d++) prows += C->nsegs[d] ? C->Z.reg_chunks : 0;
  if (prows < 1 || prows > W.rows || (C->have_reg && C->Z.reg_chunks > W.reg_chunks) ||
      (C->have_irr && C->Z.irr_chunks > W.irr_chunks))
    throw Error(-FKS_EINVAL, "the plan does not match the call's workspace layout");
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  const uint8_t* hdr = static_cast<const uint8_t*>(C->dev);
  uint32_t* const reg_states = reinterpret_cast<uint32_t*>(ws);
  uint32_t* const irr_states = reinterpret_cast<uint32_t*>(ws + W.irr_off);
  double* const partial = reinterpret_cast<double*>(ws + W.partial_off);
  const size_t reg_win = (size_t)kMtN * (size_t)C->Z.reg_chunks, irr_win = (size_t)kMtN * (size_t)C->Z.irr_chunks;
  // the jump of n seeds to the regular (irregular) chunk starts, their windows from window `first` on
  auto jump_reg = [&](const uint64_t* seeds, int n, int first) {
    JumpArgs ja = jump_args(seeds, n, hdr, C->H.off_polys, C->H.off_cb, reg_states + (size_t)first * reg_win,
                            C->Z.reg_chunks);
    ja.chunks_per_wg = jump_chunks_per_wg(n, C->Z.reg_chunks, dc.cus);
    check_launch(timed(1, stream, [&] { return launch_jump(ja, n, stream); }), "fks_jump_kernel");
  };
  auto jump_irr = [&](const uint64_t* seeds, int n, int first) {
    JumpArgs ja = jump_args(seeds, n, hdr, C->H.off_ipolys, C->H.off_ilo, irr_states + (size_t)first * irr_win,
                            C->Z.irr_chunks);
    ja.chunks_per_wg = std::max(1, std::min(32, C->Z.irr_chunks));
    check_launch(timed(1, stream, [&] { return launch_jump(ja, n, stream); }), "fks_jump_kernel");
  };
  int tile_row0 = -1;
  for (const GramPass& p : gram_mt_passes(kr, kc, symmetric)) {
    if (p.row0 != tile_row0) {  // a new row tile: its windows, once
      tile_row0 = p.row0;
      if (C->have_reg) jump_reg(rows + p.row0, p.nrows, 0);
      if (C->have_irr) jump_irr(rows + p.row0, p.nrows, 0);
    }
    double* row = partial;
    if (C->have_reg) {
      jump_reg(cols + p.col0, p.ncols, p.nrows);
      for (int d = 0; d < 3; d++) {
        if (!C->nsegs[d]) continue;
        GramMtArgs ga{};
        ga.states = reg_states;
        ga.segs = reinterpret_cast<const DevSeg*>(hdr + C->seg_off[d]);
        ga.chunk_block = reinterpret_cast<const int64_t*>(hdr + C->H.off_cb);
        ga.partial = row;
        ga.nsegs = C->nsegs[d];
        ga.nchunks = C->Z.reg_chunks;
        ga.nrows = p.nrows;
        ga.ncols = p.ncols;
        const int dd = (d == FKS_F32 && libm) ? kDtF32Libm : d;
        check_launch(timed(0, stream, [&] { return launch_gram_mt(dd, ga, stream); }), "fks_gram_mt_kernel",
                     "bad arguments");
        row += (size_t)kGramRows * (size_t)kPhxSeeds * (size_t)C->Z.reg_chunks;
      }
    }
    if (C->have_irr) {
      jump_irr(cols + p.col0, p.ncols, p.nrows);
      GramMtIrrArgs ia{};
      ia.states = irr_states;
      ia.runs = reinterpret_cast<const DevRun*>(hdr + C->H.off_runs);
      ia.tiny = reinterpret_cast<const DevTiny*>(hdr + C->H.off_tiny);
      ia.chunk_lo = reinterpret_cast<const int64_t*>(hdr + C->H.off_ilo);
      ia.chunk_hi = reinterpret_cast<const int64_t*>(hdr + C->H.off_ihi);
      ia.partial = row;
      ia.nruns = C->Z.nruns;
      ia.ntiny = C->Z.ntiny;
      ia.nchunks = C->Z.irr_chunks;
      ia.nseeds = p.nrows + p.ncols;
      ia.libm = libm ? 1 : 0;
      ia.nrows = p.nrows;
      ia.ncols = p.ncols;
      check_launch(timed(0, stream, [&] { return launch_gram_mt_irr(ia, stream); }), "fks_gram_mt_irr_kernel",
                   "bad arguments");
    }
    check_launch(launch_gram_reduce(partial, prows, p.nrows, p.ncols, dev_out, kc, p.row0, p.col0, symmetric, stream),
                 "fks_gram_reduce_kernel", "bad arguments");
  }
}

// ---- seed-basis expansion (CPU generator's stream) ----
// project_mt_multi's frame run the other way: the geometry-only plan, the per-call table of the
// outputs' pieces at the front of the workspace, then per output the passes of kMaxSeedsPerPass
// seeds -- the regular jump, one launch per dtype with fast segments, the irregular jump and
// launch.  A call of more than one pass keeps one output's f32 sums in the staging area at the
// back of the workspace between its passes (fks_expand_mt.h); k == 0 is one pass without seeds.
void expand_mt_multi(const fks_tensor* t, int nt, const uint64_t* seeds, const double* coefs, int k, const fks_vec* outs,
                     const double* betas, int nvec, int shard, int nshards, void* workspace, size_t ws_bytes,
                     void* stream) {
  // the layout on the host first: the workspace is checked before anything is allocated or launched
  const DevCaps dc = device_caps();
  const ExpMtWs W = expand_mt_ws(t, nt, k, nvec, shard, nshards, dc.cus);
  if (!W.work) return;  // nothing in this shard
  if (!workspace || ((uintptr_t)workspace % 8) != 0 || ws_bytes < W.total)
    throw Error(-FKS_EINVAL, "workspace too small or misaligned: need " + std::to_string(W.total) + " bytes, got " +
                                 std::to_string(ws_bytes));
  // the table on the host, from the layout the plan is built from
  Layout L = make_layout(t, nt, nullptr, kProjMtGeoBase);
  clip_segments(L, shard_blocks(L.stream_len, shard, nshards));
  const size_t nsegs = L.segs[0].size() + L.segs[1].size() + L.segs[2].size();
  const size_t E = nsegs + L.runs.size() + L.tiny.size();
  if (E != (size_t)W.entries) throw Error(-FKS_EINVAL, "the layout does not match the call's workspace layout");
  std::vector<int64_t> start((size_t)nt, 0);  // the tensors' first elements in the concatenation
  for (int i = 1; i < nt; i++) start[i] = start[i - 1] + t[i - 1].numel;
  thread_local std::vector<ProjMtVecEntry> host;  // the upload's source outlives the call
  host.assign((size_t)nvec * E, ProjMtVecEntry{});
  for (int m = 0; m < nvec; m++) {
    ProjMtVecEntry* x = host.data() + (size_t)m * E;
    // a descriptor of tensor i whose element 0 is element (ptr - base) / 4 of the concatenation
    auto put = [&](int i, uint64_t ptr) {
      const fks_vec& v = outs[(size_t)m * (size_t)nt + (size_t)i];
      const int64_t e = (int64_t)((ptr - kProjMtGeoBase) / 4) - start[i];
      x->ptr = (uint64_t)(uintptr_t)v.data + (uint64_t)e * elem_size(v.dtype);
      x->dtype = v.dtype;
      x++;
    };
    for (int d = 0; d < 3; d++)
      for (size_t j = 0; j < L.segs[d].size(); j++) put(L.seg_tensor[d][j], L.segs[d][j].ptr);
    for (size_t j = 0; j < L.runs.size(); j++) put(L.run_tensor[j], L.runs[j].ptr);
    for (size_t j = 0; j < L.tiny.size(); j++) put(L.tiny_tensor[j], L.tiny[j].ptr);
  }
  const bool libm = libm_flavour(t, nt);
  std::lock_guard<std::mutex> lk(g_cache_mu);  // no eviction while this call uses its entry
  const CachedPlan* C = get_plan(t, nt, nullptr, kProjMtGeoBase, shard, nshards, /*small=*/false, dc);
  bool same = (size_t)C->Z.nsegs == nsegs && (size_t)C->Z.nruns == L.runs.size() && (size_t)C->Z.ntiny == L.tiny.size();
  for (int d = 0; d < 3; d++) same = same && (size_t)C->nsegs[d] == L.segs[d].size();
  if (!same || (!C->have_reg && !C->have_irr) || (C->have_reg && C->Z.reg_chunks > W.reg_chunks) ||
      (C->have_irr && C->Z.irr_chunks > W.irr_chunks))
    throw Error(-FKS_EINVAL, "the plan does not match the call's workspace layout");
  check_hip(hipMemcpyAsync(workspace, host.data(), sizeof(ProjMtVecEntry) * host.size(), hipMemcpyHostToDevice,
                           (hipStream_t)stream), "hipMemcpyAsync");
  const ProjMtVecEntry* table = static_cast<const ProjMtVecEntry*>(workspace);
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  const uint8_t* hdr = static_cast<const uint8_t*>(C->dev);
  uint32_t* states = reinterpret_cast<uint32_t*>(ws + W.win_off);
  const uint64_t* sink = reinterpret_cast<const uint64_t*>(ws + W.sink_off);
  const int passes = std::max(1, (k + kMaxSeedsPerPass - 1) / kMaxSeedsPerPass);
  for (int m = 0; m < nvec; m++) {  // one output per pass of the generator
    const ProjMtVecEntry* tab = table + (size_t)m * E;
    const double beta = betas ? betas[m] : 0.0;
    for (int p = 0; p < passes; p++) {
      const int s0 = p * kMaxSeedsPerPass, nb = std::min(kMaxSeedsPerPass, k - s0);
      ExpMtPass ps{};
      for (int j = 0; j < nb; j++) ps.g[j] = (float)coefs[(size_t)m * (size_t)k + (size_t)(s0 + j)];
      ps.stage_bias = (uint64_t)(uintptr_t)(ws + W.stage_off) - kProjMtGeoBase - 4u * (uint64_t)W.elem_lo;
      ps.beta = (float)beta;
      ps.nseeds = nb;
      ps.carry_in = p > 0 ? 1 : 0;
      ps.to_stage = p + 1 < passes ? 1 : 0;
      ps.read_old = beta != 0.0 ? 1 : 0;
      if (C->have_reg) {
        JumpArgs ja = jump_args(seeds + s0, nb, hdr, C->H.off_polys, C->H.off_cb, states, C->Z.reg_chunks);
        ja.chunks_per_wg = jump_chunks_per_wg(std::max(nb, 1), C->Z.reg_chunks, dc.cus);
        if (nb > 0) check_launch(timed(1, stream, [&] { return launch_jump(ja, nb, stream); }), "fks_jump_kernel");
        size_t seg0 = 0;  // the dtype's first segment in the table row
        for (int d = 0; d < 3; d++) {
          const size_t first = seg0;
          seg0 += (size_t)C->nsegs[d];
          if (!C->nsegs[d]) continue;
          ExpMtArgs ea{};
          ea.p = ps;
          ea.states = states;
          ea.segs = reinterpret_cast<const DevSeg*>(hdr + C->seg_off[d]);
          ea.chunk_block = ja.chunk_block;
          ea.sink = sink;
          ea.pv = tab + first;
          ea.nsegs = C->nsegs[d];
          ea.nchunks = C->Z.reg_chunks;
          const int dd = (d == FKS_F32 && libm) ? kDtF32Libm : d;
          check_launch(timed(0, stream, [&] { return launch_expand_mt(dd, ea, stream); }), "fks_expand_mt_kernel",
                       "bad arguments");
        }
      }
      if (C->have_irr) {
        JumpArgs ja = jump_args(seeds + s0, nb, hdr, C->H.off_ipolys, C->H.off_ilo, states, C->Z.irr_chunks);
        ja.chunks_per_wg = std::max(1, std::min(32, C->Z.irr_chunks));
        if (nb > 0) check_launch(timed(1, stream, [&] { return launch_jump(ja, nb, stream); }), "fks_jump_kernel");
        ExpMtIrrArgs ia{};
        ia.p = ps;
        ia.states = states;
        ia.runs = reinterpret_cast<const DevRun*>(hdr + C->H.off_runs);
        ia.tiny = reinterpret_cast<const DevTiny*>(hdr + C->H.off_tiny);
        ia.chunk_lo = ja.chunk_block;
        ia.chunk_hi = reinterpret_cast<const int64_t*>(hdr + C->H.off_ihi);
        ia.rv = tab + nsegs;
        ia.tv = tab + nsegs + L.runs.size();
        ia.nruns = C->Z.nruns;
        ia.ntiny = C->Z.ntiny;
        ia.nchunks = C->Z.irr_chunks;
        ia.nseeds = nb;
        ia.libm = libm ? 1 : 0;
        check_launch(timed(0, stream, [&] { return launch_expand_mt_irr(ia, stream); }), "fks_expand_mt_irr_kernel",
                     "bad arguments");
      }
    }
  }
}

}  // namespace fks
