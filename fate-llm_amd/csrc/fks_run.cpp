// fks_run.cpp -- the launch driver of the codec's calls: seed batching, workspace carving and the
// kernel launches of the update, perturb, normal and delta calls, fks_profile_begin/end's events
// around them, the digest and the device self-checks.  fks_run_basis.cpp drives the seed-basis calls.
#include <cmath>
#include <cstdlib>

#include "fks_run.h"

namespace fks {

Prof g_prof;
std::mutex g_prof_mu;

namespace {

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
  const MtPlan V{*C, dc.cus, libm, stream};
  for (int s0 = 0; s0 < k; s0 += kMaxSeedsPerPass) {
    const int nb = std::min(kMaxSeedsPerPass, k - s0);
    if (reg_rest) {
      // a replay needs no windows unless another dtype's segments still generate
      const bool need_windows = zmode != 2 || C->nsegs[FKS_F32] > 0 || C->nsegs[FKS_F16] > 0;
      if (!reg_cached && need_windows) {
        V.jump_regular(seeds + s0, nb, reg_states);
        reg_jumped = true;
      }
      V.each_fast_dtype([&](int d, int dd, size_t) {
        if (use_bs && d == FKS_BF16) return;
        ApplyArgs aa{};
        V.fill_fast(aa, d, reg_states);
        for (int j = 0; j < nb; j++) aa.g[j] = gval(s0 + j, d);
        aa.sink = reinterpret_cast<uint64_t*>(ws);
        aa.gdev = gdev;
        if (Zc && d == FKS_BF16) {
          aa.zidx = static_cast<uint32_t*>(Zc->b.buf);
          aa.zlo = Zc->lo;
          aa.zmode = zmode;
        }
        aa.nseeds = nb;
        aa.mode = mode == kModeUpdate ? C->wd_mode[d] : mode;  // weight-decay select specialised away
        check_launch(timed(0, stream, [&] { return launch_apply(dd, aa, stream); }), "fks_apply_kernel");
      });
    }
    if (C->have_irr) {
      if (!irr_cached) V.jump_irregular(seeds + s0, nb, irr_states);
      IrrArgs ia{};
      V.fill_irregular(ia, irr_states);
      for (int d = 0; d < 3; d++)
        for (int j = 0; j < nb; j++) ia.g[d][j] = gval(s0 + j, d);
      ia.gdev = gdev;
      ia.nseeds = nb;
      ia.mode = mode;
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

}  // namespace fks
