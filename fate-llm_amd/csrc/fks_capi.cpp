// fks_capi.cpp -- the C ABI of libfks.so (include/fks.h): argument checks and one call each into
// fks_layout / fks_phx / fks_cache / fks_run.cpp.  Exceptions never cross it: guarded() returns codes.
// Reference routines replaced (include/fks.h lists them): zo_utils.directional_derivative_step
// (zo_utils.py:23-54), ZerothOrderOptimizer.random_perturb_parameters (optimizer.py:152-173),
// and the per-seed reconstruct loop of ClientTrainer.train_once (fedkseed.py:136-141).
#include "fks_host.h"

using namespace fks;

static thread_local std::string g_last_error;

template <class F>
static int guarded(F&& f) {
  try {
    g_last_error.clear();
    f();
    return 0;
  } catch (const Error& e) {
    g_last_error = e.what();
    return e.code;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return -FKS_EINVAL;
  } catch (...) {
    g_last_error = "unknown error";
    return -FKS_EINVAL;
  }
}

extern "C" {

int fks_workspace_size(const fks_tensor* t, int32_t nt, int32_t k, size_t* bytes) {
  return guarded([&] {
    validate(t, nt);
    if (!bytes || k < 0) throw Error(-FKS_EINVAL, "bad arguments");
    *bytes = workspace_total(t, nt, k, 0, device_cu_count());
  });
}

int fks_zindex_size(const fks_tensor* t, int32_t nt, size_t* bytes) {
  return guarded([&] {
    validate(t, nt);
    if (!bytes) throw Error(-FKS_EINVAL, "bad arguments");
    *bytes = zindex_bytes(t, nt);
  });
}

int fks_zindex_attach(void* buf, size_t bytes) {
  return guarded([&] {
    std::lock_guard<std::mutex> lk(g_cache_mu);
    ZCache* Z = z_entry();
    if (!Z) throw Error(-FKS_EHIP, "z-index cache event");
    buf_attach(Z->b, buf, bytes, "z-index cache");
    Z->valid = false;
  });
}

int fks_jwin_size_shard(const fks_tensor* t, int32_t nt, int32_t k, int32_t shard, int32_t nshards, size_t* bytes) {
  return guarded([&] {
    validate(t, nt);
    if (!bytes || k < 0) throw Error(-FKS_EINVAL, "bad arguments");
    check_shard(shard, nshards);
    *bytes = 0;  // also when the plan cannot be built
    *bytes = jwin_bytes(t, nt, k, shard, nshards);
  });
}

int fks_jwin_size(const fks_tensor* t, int32_t nt, int32_t k, size_t* bytes) {
  return fks_jwin_size_shard(t, nt, k, 0, 1, bytes);
}

int fks_jwin_attach(void* buf, size_t bytes) {
  return guarded([&] {
    std::lock_guard<std::mutex> lk(g_cache_mu);
    JWin* J = jw_entry();
    if (!J) throw Error(-FKS_EHIP, "window cache event");
    buf_attach(J->b, buf, bytes, "window cache");
    jw_drop(*J);
  });
}

int fks_jwin_stats(uint64_t* hits, uint64_t* misses) {
  return guarded([&] {
    if (!hits || !misses) throw Error(-FKS_EINVAL, "bad arguments");
    std::lock_guard<std::mutex> lk(g_cache_mu);
    JWin* J = jw_entry();
    *hits = J ? J->sets.hits : 0;
    *misses = J ? J->sets.misses : 0;
  });
}

int fks_delta_workspace_size(const fks_tensor* t, int32_t nt, int32_t k, size_t* bytes) {
  return guarded([&] {
    validate(t, nt);
    if (!bytes || k < 0) throw Error(-FKS_EINVAL, "bad arguments");
    // any 8-byte aligned delta base gives the same layout; fks_delta_apply's tensor
    // descriptors fit in the same workspace
    *bytes = std::max(workspace_total(t, nt, k, 256, device_cu_count()),
                      sizeof(DeltaApplyDesc) * (size_t)std::max(nt, 1) + 256);
  });
}

int fks_delta_accumulate(const fks_tensor* t, int32_t nt, const uint64_t* seeds, const double* coefs, int32_t k,
                         float* delta, void* workspace, size_t ws_bytes, void* stream) {
  return guarded([&] {
    if (k > 0 && (!delta || ((uintptr_t)delta % 8) != 0)) throw Error(-FKS_EINVAL, "null or misaligned delta buffer");
    run(t, nt, seeds, coefs, k, FKS_VALUE_SCALAR, kModeDelta, workspace, ws_bytes, stream, nullptr, 0, 1,
        (uint64_t)(uintptr_t)delta);
  });
}

int fks_delta_apply(const fks_tensor* t, int32_t nt, const float* delta, const double* decay, void* workspace,
                    size_t ws_bytes, void* stream) {
  return guarded([&] {
    validate(t, nt);
    if (nt == 0) return;
    if (!delta || !decay || !workspace) throw Error(-FKS_EINVAL, "null argument");
    delta_apply(t, nt, delta, decay, workspace, ws_bytes, stream);
  });
}

// ---- seed-basis projection (torch_rocm stream) ----
// the calls take the torch_rocm stream only: every error is raised from the arguments alone
static void project_check_stream(const fks_tensor* t, int nt) {
  if (nt == 0 || rocm_stream(t, nt)) return;
  throw Error(-FKS_ENOTSUP, std::string("fks_project: the torch_cpu stream (the CPU generator's MT19937 stream") +
                                (libm_flavour(t, nt) ? ", FKS_LIBM flavour" : "") +
                                ") is not supported; projection is built for FKS_STREAM_ROCM (torch_rocm) only");
}

int fks_project_workspace_size(const fks_tensor* t, int32_t nt, int32_t k, size_t* bytes) {
  return guarded([&] {
    validate(t, nt);
    if (!bytes || k < 0) throw Error(-FKS_EINVAL, "bad arguments");
    project_check_stream(t, nt);
    *bytes = project_ws_bytes(t, nt, 1, false);
  });
}

int fks_project(const fks_tensor* t, int32_t nt, const uint64_t* seeds, int32_t k, const float* vec, int32_t shard,
                int32_t nshards, double* dev_out, void* workspace, size_t ws_bytes, void* stream) {
  return guarded([&] {
    validate(t, nt);
    check_shard(shard, nshards);
    if (k < 0 || (k > 0 && !seeds)) throw Error(-FKS_EINVAL, "bad seed array");
    if (k > 0 && (!vec || ((uintptr_t)vec % 8) != 0)) throw Error(-FKS_EINVAL, "null or misaligned vector");
    if (k > 0 && (!dev_out || ((uintptr_t)dev_out % 8) != 0))
      throw Error(-FKS_EINVAL, "null or misaligned projection output");
    project_check_stream(t, nt);
    if (k == 0) return;
    project(t, nt, seeds, k, vec, nullptr, 1, shard, nshards, dev_out, workspace, ws_bytes, stream);
  });
}

int fks_project_multi_workspace_size(const fks_tensor* t, int32_t nt, int32_t k, int32_t nvec, size_t* bytes) {
  return guarded([&] {
    validate(t, nt);
    if (!bytes || k < 0 || nvec < 0) throw Error(-FKS_EINVAL, "bad arguments");
    project_check_stream(t, nt);
    *bytes = project_ws_bytes(t, nt, nvec, true);
  });
}

int fks_project_multi(const fks_tensor* t, int32_t nt, const uint64_t* seeds, int32_t k, const fks_vec* vecs, int32_t nvec,
                      int32_t shard, int32_t nshards, double* dev_out, void* workspace, size_t ws_bytes, void* stream) {
  return guarded([&] {
    validate(t, nt);
    if (nvec < 0) throw Error(-FKS_EINVAL, "negative vector count");
    check_shard(shard, nshards);
    if (k < 0 || (k > 0 && !seeds)) throw Error(-FKS_EINVAL, "bad seed array");
    if (nvec > 0 && nt > 0 && !vecs) throw Error(-FKS_EINVAL, "null vector list");
    for (int m = 0; m < nvec; m++)
      for (int i = 0; i < nt; i++) {
        if (t[i].numel == 0 || (t[i].flags & FKS_FROZEN)) continue;  // ignored: may be NULL
        const fks_vec& v = vecs[(size_t)m * (size_t)nt + (size_t)i];
        if (v.dtype != FKS_F32 && v.dtype != FKS_BF16 && v.dtype != FKS_F16)
          throw Error(-FKS_EINVAL, "vector " + std::to_string(m) + ", tensor " + std::to_string(i) + ": bad vector dtype " +
                                       std::to_string(v.dtype));
        if (!v.data || ((uintptr_t)v.data % elem_size(v.dtype)) != 0)
          throw Error(-FKS_EINVAL, "vector " + std::to_string(m) + ", tensor " + std::to_string(i) +
                                       ": null or misaligned vector pointer");
      }
    if (k > 0 && nvec > 0 && (!dev_out || ((uintptr_t)dev_out % 8) != 0))
      throw Error(-FKS_EINVAL, "null or misaligned projection output");
    project_check_stream(t, nt);
    if (k == 0 || nvec == 0) return;
    project(t, nt, seeds, k, nullptr, vecs, nvec, shard, nshards, dev_out, workspace, ws_bytes, stream);
  });
}

// ---- seed-basis Gram matrix (torch_rocm stream) ----
static void gram_check_stream(const fks_tensor* t, int nt) {
  if (nt == 0 || rocm_stream(t, nt)) return;
  throw Error(-FKS_ENOTSUP, std::string("fks_gram: the torch_cpu stream (the CPU generator's MT19937 stream") +
                                (libm_flavour(t, nt) ? ", FKS_LIBM flavour" : "") +
                                ") is not supported; the Gram matrix is built for FKS_STREAM_ROCM (torch_rocm) only "
                                "here, fks_gram_mt is the call for this stream");
}
// the seed counts of a call: col_seeds NULL is the symmetric form, whose kcols is 0 or krows
static void gram_check_counts(int32_t krows, int32_t kcols, bool symmetric) {
  if (krows < 0 || kcols < 0) throw Error(-FKS_EINVAL, "negative seed count");
  if (symmetric && kcols != 0 && kcols != krows)
    throw Error(-FKS_EINVAL, "kcols must be 0 or krows without column seeds (the symmetric Gram matrix), got " +
                                 std::to_string(kcols) + " for krows " + std::to_string(krows));
}

int fks_gram_workspace_size(const fks_tensor* t, int32_t nt, int32_t krows, int32_t kcols, size_t* bytes) {
  return guarded([&] {
    validate(t, nt);
    if (!bytes || krows < 0 || kcols < 0) throw Error(-FKS_EINVAL, "bad arguments");
    gram_check_stream(t, nt);
    *bytes = gram_ws_bytes(t, nt);
  });
}

int fks_gram(const fks_tensor* t, int32_t nt, const uint64_t* row_seeds, int32_t krows, const uint64_t* col_seeds,
             int32_t kcols, int32_t shard, int32_t nshards, double* dev_out, void* workspace, size_t ws_bytes,
             void* stream) {
  return guarded([&] {
    validate(t, nt);
    check_shard(shard, nshards);
    gram_check_counts(krows, kcols, col_seeds == nullptr);
    if (krows > 0 && !row_seeds) throw Error(-FKS_EINVAL, "null row seed array");
    const int32_t kc = col_seeds ? kcols : krows;
    if (krows > 0 && kc > 0 && (!dev_out || ((uintptr_t)dev_out % 8) != 0))
      throw Error(-FKS_EINVAL, "null or misaligned Gram output");
    gram_check_stream(t, nt);
    if (krows == 0 || kc == 0) return;
    gram(t, nt, row_seeds, krows, col_seeds, kc, shard, nshards, dev_out, workspace, ws_bytes, stream);
  });
}

int fks_gram_passes(int32_t krows, int32_t kcols, int32_t symmetric, int32_t* passes, int32_t cap, int32_t* n) {
  return guarded([&] {
    if (cap < 0 || !n || (cap > 0 && !passes)) throw Error(-FKS_EINVAL, "bad arguments");
    gram_check_counts(krows, kcols, symmetric != 0);
    const std::vector<GramPass> p = gram_passes(krows, symmetric ? krows : kcols, symmetric != 0);
    *n = (int32_t)std::min<size_t>(p.size(), (size_t)INT32_MAX);
    for (size_t i = 0; i < p.size() && i < (size_t)cap; i++) {
      passes[4 * i + 0] = p[i].row0;
      passes[4 * i + 1] = p[i].nrows;
      passes[4 * i + 2] = p[i].col0;
      passes[4 * i + 3] = p[i].ncols;
    }
  });
}

// ---- tiled seed-basis Gram matrix (torch_rocm stream) ----
static void gram_tiled_check_stream(const fks_tensor* t, int nt) {
  if (nt == 0 || rocm_stream(t, nt)) return;
  throw Error(-FKS_ENOTSUP, std::string("fks_gram_tiled: the torch_cpu stream (the CPU generator's MT19937 stream") +
                                (libm_flavour(t, nt) ? ", FKS_LIBM flavour" : "") +
                                ") is not supported; the tiled Gram matrix is built for FKS_STREAM_ROCM (torch_rocm) "
                                "only, fks_gram_mt is the call for this stream");
}

int fks_gram_tiled_workspace_size(const fks_tensor* t, int32_t nt, int32_t krows, int32_t kcols, size_t* bytes) {
  return guarded([&] {
    validate(t, nt);
    if (!bytes || krows < 0 || kcols < 0) throw Error(-FKS_EINVAL, "bad arguments");
    gram_tiled_check_stream(t, nt);
    *bytes = gram_tiled_ws_bytes(t, nt);
  });
}

int fks_gram_tiled(const fks_tensor* t, int32_t nt, const uint64_t* row_seeds, int32_t krows, const uint64_t* col_seeds,
                   int32_t kcols, int32_t shard, int32_t nshards, double* dev_out, void* workspace, size_t ws_bytes,
                   void* stream) {
  return guarded([&] {
    validate(t, nt);
    check_shard(shard, nshards);
    gram_check_counts(krows, kcols, col_seeds == nullptr);
    if (krows > 0 && !row_seeds) throw Error(-FKS_EINVAL, "null row seed array");
    const int32_t kc = col_seeds ? kcols : krows;
    if (krows > 0 && kc > 0 && (!dev_out || ((uintptr_t)dev_out % 8) != 0))
      throw Error(-FKS_EINVAL, "null or misaligned Gram output");
    gram_tiled_check_stream(t, nt);
    if (krows == 0 || kc == 0) return;
    gram_tiled(t, nt, row_seeds, krows, col_seeds, kc, shard, nshards, dev_out, workspace, ws_bytes, stream);
  });
}

int fks_gram_tiled_passes(int32_t krows, int32_t kcols, int32_t symmetric, int32_t* passes, int32_t cap, int32_t* n) {
  return guarded([&] {
    if (cap < 0 || !n || (cap > 0 && !passes)) throw Error(-FKS_EINVAL, "bad arguments");
    gram_check_counts(krows, kcols, symmetric != 0);
    const std::vector<GramPass> p = gram_tiled_passes(krows, symmetric ? krows : kcols, symmetric != 0);
    *n = (int32_t)std::min<size_t>(p.size(), (size_t)INT32_MAX);
    for (size_t i = 0; i < p.size() && i < (size_t)cap; i++) {
      passes[4 * i + 0] = p[i].row0;
      passes[4 * i + 1] = p[i].nrows;
      passes[4 * i + 2] = p[i].col0;
      passes[4 * i + 3] = p[i].ncols;
    }
  });
}

// ---- seed-basis expansion (torch_rocm stream) ----
static void expand_check_stream(const fks_tensor* t, int nt) {
  if (nt == 0 || rocm_stream(t, nt)) return;
  throw Error(-FKS_ENOTSUP, std::string("fks_expand_multi: the torch_cpu stream (the CPU generator's MT19937 stream") +
                                (libm_flavour(t, nt) ? ", FKS_LIBM flavour" : "") +
                                ") is not supported here; fks_expand_multi takes FKS_STREAM_ROCM (torch_rocm) lists, "
                                "fks_expand_mt_multi is the call for this stream (fks_delta_accumulate sums either "
                                "stream into an f32 buffer)");
}

int fks_expand_multi_workspace_size(const fks_tensor* t, int32_t nt, int32_t k, int32_t nvec, size_t* bytes) {
  return guarded([&] {
    validate(t, nt);
    if (!bytes || k < 0 || nvec < 0) throw Error(-FKS_EINVAL, "bad arguments");
    expand_check_stream(t, nt);
    *bytes = expand_ws_bytes(t, nt, k, nvec);
  });
}

int fks_expand_multi(const fks_tensor* t, int32_t nt, const uint64_t* seeds, const double* coefs, int32_t k,
                     const fks_vec* outs, const double* betas, int32_t nvec, int32_t shard, int32_t nshards,
                     void* workspace, size_t ws_bytes, void* stream) {
  return guarded([&] {
    validate(t, nt);
    if (nvec < 0) throw Error(-FKS_EINVAL, "negative output count");
    check_shard(shard, nshards);
    if (k < 0 || (k > 0 && !seeds)) throw Error(-FKS_EINVAL, "bad seed array");
    if (k > 0 && nvec > 0 && !coefs) throw Error(-FKS_EINVAL, "null coefficient array");
    if (nvec > 0 && nt > 0 && !outs) throw Error(-FKS_EINVAL, "null output list");
    for (int m = 0; m < nvec; m++)
      for (int i = 0; i < nt; i++) {
        if (t[i].numel == 0 || (t[i].flags & FKS_FROZEN)) continue;  // ignored: may be NULL
        const fks_vec& v = outs[(size_t)m * (size_t)nt + (size_t)i];
        if (v.dtype != FKS_F32 && v.dtype != FKS_BF16 && v.dtype != FKS_F16)
          throw Error(-FKS_EINVAL, "output " + std::to_string(m) + ", tensor " + std::to_string(i) + ": bad output dtype " +
                                       std::to_string(v.dtype));
        if (!v.data || ((uintptr_t)v.data % elem_size(v.dtype)) != 0)
          throw Error(-FKS_EINVAL, "output " + std::to_string(m) + ", tensor " + std::to_string(i) +
                                       ": null or misaligned output pointer");
      }
    expand_check_stream(t, nt);
    if (nvec == 0 || nt == 0) return;
    expand(t, nt, seeds, coefs, k, outs, betas, nvec, shard, nshards, workspace, ws_bytes, stream);
  });
}

int fks_expand_launch_cuts(const fks_tensor* t, int32_t nt, int32_t k, int32_t shard, int32_t nshards, int64_t work,
                           int64_t max_grid, int64_t* cuts, int32_t cap, int32_t* ncuts) {
  return guarded([&] {
    validate(t, nt);
    check_shard(shard, nshards);
    if (k < 0 || cap < 0 || !ncuts || (cap > 0 && !cuts)) throw Error(-FKS_EINVAL, "bad arguments");
    expand_check_stream(t, nt);
    const PhxGeo geo = phx_geometry(t, nt, nullptr, 0, max_grid > 0 ? max_grid : device_caps().max_grid);
    const std::vector<int64_t> b = phx_expand_cuts(geo, phx_boundary(geo, shard, nshards),
                                                   phx_boundary(geo, shard + 1, nshards), k,
                                                   work > 0 ? work : expand_launch_work());
    *ncuts = (int32_t)std::min<size_t>(b.size(), (size_t)INT32_MAX);
    for (size_t i = 0; i < b.size() && i < (size_t)cap; i++) cuts[i] = b[i];
  });
}

// ---- seed-basis projection (CPU generator's stream) ----
static void project_mt_check_stream(const fks_tensor* t, int nt) {
  if (rocm_stream(t, nt))
    throw Error(-FKS_ENOTSUP, "fks_project_mt: the torch_rocm stream (FKS_STREAM_ROCM) is not supported here; "
                              "fks_project is the call for that stream");
}

int fks_project_mt_workspace_size(const fks_tensor* t, int32_t nt, int32_t k, size_t* bytes) {
  return guarded([&] {
    validate(t, nt);
    if (!bytes || k < 0) throw Error(-FKS_EINVAL, "bad arguments");
    project_mt_check_stream(t, nt);
    *bytes = project_mt_ws(t, nt, k, 0, 1, device_cu_count()).total;
  });
}

int fks_project_mt(const fks_tensor* t, int32_t nt, const uint64_t* seeds, int32_t k, const float* vec, int32_t shard,
                   int32_t nshards, double* dev_out, void* workspace, size_t ws_bytes, void* stream) {
  return guarded([&] {
    validate(t, nt);
    check_shard(shard, nshards);
    if (k < 0 || (k > 0 && !seeds)) throw Error(-FKS_EINVAL, "bad seed array");
    if (k > 0 && (!vec || ((uintptr_t)vec % 8) != 0)) throw Error(-FKS_EINVAL, "null or misaligned vector");
    if (k > 0 && (!dev_out || ((uintptr_t)dev_out % 8) != 0))
      throw Error(-FKS_EINVAL, "null or misaligned projection output");
    project_mt_check_stream(t, nt);
    if (k == 0) return;
    project_mt(t, nt, seeds, k, vec, shard, nshards, dev_out, workspace, ws_bytes, stream);
  });
}

// ... several vectors, each read where it lies
static void project_mt_multi_check_stream(const fks_tensor* t, int nt) {
  if (rocm_stream(t, nt))
    throw Error(-FKS_ENOTSUP, "fks_project_mt_multi: the torch_rocm stream (FKS_STREAM_ROCM) is not supported here; "
                              "fks_project_multi is the call for that stream");
}

int fks_project_mt_multi_workspace_size(const fks_tensor* t, int32_t nt, int32_t k, int32_t nvec, size_t* bytes) {
  return guarded([&] {
    validate(t, nt);
    if (!bytes || k < 0 || nvec < 0) throw Error(-FKS_EINVAL, "bad arguments");
    project_mt_multi_check_stream(t, nt);
    *bytes = project_mt_multi_ws(t, nt, k, nvec, 0, 1, device_cu_count()).total;
  });
}

int fks_project_mt_multi(const fks_tensor* t, int32_t nt, const uint64_t* seeds, int32_t k, const fks_vec* vecs,
                         int32_t nvec, int32_t shard, int32_t nshards, double* dev_out, void* workspace,
                         size_t ws_bytes, void* stream) {
  return guarded([&] {
    validate(t, nt);
    if (nvec < 0) throw Error(-FKS_EINVAL, "negative vector count");
    check_shard(shard, nshards);
    if (k < 0 || (k > 0 && !seeds)) throw Error(-FKS_EINVAL, "bad seed array");
    if (nvec > 0 && nt > 0 && !vecs) throw Error(-FKS_EINVAL, "null vector list");
    for (int m = 0; m < nvec; m++)
      for (int i = 0; i < nt; i++) {
        if (t[i].numel == 0 || (t[i].flags & FKS_FROZEN)) continue;  // ignored: may be NULL
        const fks_vec& v = vecs[(size_t)m * (size_t)nt + (size_t)i];
        if (v.dtype != FKS_F32 && v.dtype != FKS_BF16 && v.dtype != FKS_F16)
          throw Error(-FKS_EINVAL, "vector " + std::to_string(m) + ", tensor " + std::to_string(i) + ": bad vector dtype " +
                                       std::to_string(v.dtype));
        if (!v.data || ((uintptr_t)v.data % elem_size(v.dtype)) != 0)
          throw Error(-FKS_EINVAL, "vector " + std::to_string(m) + ", tensor " + std::to_string(i) +
                                       ": null or misaligned vector pointer");
      }
    if (k > 0 && nvec > 0 && (!dev_out || ((uintptr_t)dev_out % 8) != 0))
      throw Error(-FKS_EINVAL, "null or misaligned projection output");
    project_mt_multi_check_stream(t, nt);
    if (k == 0 || nvec == 0) return;
    project_mt_multi(t, nt, seeds, k, vecs, nvec, shard, nshards, dev_out, workspace, ws_bytes, stream);
  });
}

// ---- seed-basis Gram matrix (CPU generator's stream) ----
static void gram_mt_check_stream(const fks_tensor* t, int nt) {
  if (rocm_stream(t, nt))
    throw Error(-FKS_ENOTSUP, "fks_gram_mt: the torch_rocm stream (FKS_STREAM_ROCM) is not supported here; "
                              "fks_gram is the call for that stream");
}

int fks_gram_mt_workspace_size(const fks_tensor* t, int32_t nt, int32_t krows, int32_t kcols, size_t* bytes) {
  return guarded([&] {
    validate(t, nt);
    if (!bytes || krows < 0 || kcols < 0) throw Error(-FKS_EINVAL, "bad arguments");
    gram_mt_check_stream(t, nt);
    *bytes = gram_mt_ws(t, nt, 0, 1, device_cu_count()).total;
  });
}

int fks_gram_mt(const fks_tensor* t, int32_t nt, const uint64_t* row_seeds, int32_t krows, const uint64_t* col_seeds,
                int32_t kcols, int32_t shard, int32_t nshards, double* dev_out, void* workspace, size_t ws_bytes,
                void* stream) {
  return guarded([&] {
    validate(t, nt);
    check_shard(shard, nshards);
    gram_check_counts(krows, kcols, col_seeds == nullptr);
    if (krows > 0 && !row_seeds) throw Error(-FKS_EINVAL, "null row seed array");
    const int32_t kc = col_seeds ? kcols : krows;
    if (krows > 0 && kc > 0 && (!dev_out || ((uintptr_t)dev_out % 8) != 0))
      throw Error(-FKS_EINVAL, "null or misaligned Gram output");
    gram_mt_check_stream(t, nt);
    if (krows == 0 || kc == 0) return;
    gram_mt(t, nt, row_seeds, krows, col_seeds, kc, shard, nshards, dev_out, workspace, ws_bytes, stream);
  });
}

int fks_gram_mt_passes(int32_t krows, int32_t kcols, int32_t symmetric, int32_t* passes, int32_t cap, int32_t* n) {
  return guarded([&] {
    if (cap < 0 || !n || (cap > 0 && !passes)) throw Error(-FKS_EINVAL, "bad arguments");
    gram_check_counts(krows, kcols, symmetric != 0);
    const std::vector<GramPass> p = gram_mt_passes(krows, symmetric ? krows : kcols, symmetric != 0);
    *n = (int32_t)std::min<size_t>(p.size(), (size_t)INT32_MAX);
    for (size_t i = 0; i < p.size() && i < (size_t)cap; i++) {
      passes[4 * i + 0] = p[i].row0;
      passes[4 * i + 1] = p[i].nrows;
      passes[4 * i + 2] = p[i].col0;
      passes[4 * i + 3] = p[i].ncols;
    }
  });
}

// ---- seed-basis expansion (CPU generator's stream) ----
static void expand_mt_check_stream(const fks_tensor* t, int nt) {
  if (rocm_stream(t, nt))
    throw Error(-FKS_ENOTSUP, "fks_expand_mt_multi: the torch_rocm stream (FKS_STREAM_ROCM) is not supported here; "
                              "fks_expand_multi is the call for that stream");
}

int fks_expand_mt_multi_workspace_size(const fks_tensor* t, int32_t nt, int32_t k, int32_t nvec, int32_t shard,
                                       int32_t nshards, size_t* bytes) {
  return guarded([&] {
    validate(t, nt);
    if (!bytes || k < 0 || nvec < 0) throw Error(-FKS_EINVAL, "bad arguments");
    check_shard(shard, nshards);
    expand_mt_check_stream(t, nt);
    *bytes = expand_mt_ws(t, nt, k, nvec, shard, nshards, device_cu_count()).total;
  });
}

int fks_expand_mt_multi(const fks_tensor* t, int32_t nt, const uint64_t* seeds, const double* coefs, int32_t k,
                        const fks_vec* outs, const double* betas, int32_t nvec, int32_t shard, int32_t nshards,
                        void* workspace, size_t ws_bytes, void* stream) {
  return guarded([&] {
    validate(t, nt);
    if (nvec < 0) throw Error(-FKS_EINVAL, "negative output count");
    check_shard(shard, nshards);
    if (k < 0 || (k > 0 && !seeds)) throw Error(-FKS_EINVAL, "bad seed array");
    if (k > 0 && nvec > 0 && !coefs) throw Error(-FKS_EINVAL, "null coefficient array");
    if (nvec > 0 && nt > 0 && !outs) throw Error(-FKS_EINVAL, "null output list");
    for (int m = 0; m < nvec; m++)
      for (int i = 0; i < nt; i++) {
        if (t[i].numel == 0 || (t[i].flags & FKS_FROZEN)) continue;  // ignored: may be NULL
        const fks_vec& v = outs[(size_t)m * (size_t)nt + (size_t)i];
        if (v.dtype != FKS_F32 && v.dtype != FKS_BF16 && v.dtype != FKS_F16)
          throw Error(-FKS_EINVAL, "output " + std::to_string(m) + ", tensor " + std::to_string(i) + ": bad output dtype " +
                                       std::to_string(v.dtype));
        if (!v.data || ((uintptr_t)v.data % elem_size(v.dtype)) != 0)
          throw Error(-FKS_EINVAL, "output " + std::to_string(m) + ", tensor " + std::to_string(i) +
                                       ": null or misaligned output pointer");
      }
    expand_mt_check_stream(t, nt);
    if (nvec == 0 || nt == 0) return;
    expand_mt_multi(t, nt, seeds, coefs, k, outs, betas, nvec, shard, nshards, workspace, ws_bytes, stream);
  });
}

int fks_directional_step(const fks_tensor* t, int32_t nt, const uint64_t* seeds, const double* values, int32_t k,
                         int32_t value_kind, void* workspace, size_t ws_bytes, void* stream) {
  return guarded([&] { run(t, nt, seeds, values, k, value_kind, kModeUpdate, workspace, ws_bytes, stream); });
}

int fks_directional_step_shard(const fks_tensor* t, int32_t nt, const uint64_t* seeds, const double* values,
                               int32_t k, int32_t value_kind, int32_t shard, int32_t nshards, void* workspace,
                               size_t ws_bytes, void* stream) {
  return guarded([&] {
    run(t, nt, seeds, values, k, value_kind, kModeUpdate, workspace, ws_bytes, stream, nullptr, shard, nshards);
  });
}

int fks_digest(const fks_tensor* t, int32_t nt, uint64_t pos0, uint64_t* dev_out2, void* stream) {
  return guarded([&] {
    // flags, lr and wd play no part here: the list is checked for what the digest reads
    if (nt < 0 || (nt > 0 && !t)) throw Error(-FKS_EINVAL, "bad tensor list");
    if (!dev_out2 || ((uintptr_t)dev_out2 % 8) != 0) throw Error(-FKS_EINVAL, "null or misaligned digest output");
    validate_basics(t, nt);
    digest(t, nt, pos0, dev_out2, stream);
  });
}

int fks_stream_length(const fks_tensor* t, int32_t nt, int64_t* words) {
  return guarded([&] {
    validate(t, nt);
    if (!words) throw Error(-FKS_EINVAL, "null output");
    *words = make_layout(t, nt).stream_len;
  });
}

int fks_cpu_generator_end(const fks_tensor* t, int32_t nt, uint64_t seed, uint32_t* state624, int32_t* left,
                          uint32_t* next, int32_t* normal_valid, double* normal) {
  return guarded([&] {
    validate(t, nt);
    if (!state624 || !left || !next || !normal_valid || !normal) throw Error(-FKS_EINVAL, "null output");
    cpu_generator_end(t, nt, seed, state624, left, next, normal_valid, normal);
  });
}

int fks_rocm_grid_cap(int64_t* blocks) {
  return guarded([&] {
    if (!blocks) throw Error(-FKS_EINVAL, "null output");
    *blocks = device_caps(true).max_grid;
  });
}

int fks_rocm_offset(const fks_tensor* t, int32_t nt, uint64_t* offset) {
  return guarded([&] {
    validate(t, nt);
    if (!offset) throw Error(-FKS_EINVAL, "null output");
    *offset = 4 * phx_geometry(t, nt, nullptr, 0, device_caps(true).max_grid).off4_total;
  });
}

int fks_shard_census(const fks_tensor* t, int32_t nt, int32_t shard, int32_t nshards, int64_t* word_range,
                     int64_t* written) {
  return guarded([&] {
    validate(t, nt);
    check_shard(shard, nshards);
    // torch_rocm: host geometry only, no plan cache entry, no device allocation (the scales
    // do not move row boundaries)
    if (rocm_stream(t, nt))
      phx_census(phx_geometry(t, nt, nullptr, 0, device_caps().max_grid), nt, shard, nshards, word_range, written);
    else
      mt_census(t, nt, shard, nshards, word_range, written);
  });
}

int fks_profile_begin(void) {
  profile_begin();
  return 0;
}

int fks_profile_end(double* apply_ms, int64_t* n_apply, double* jump_ms, int64_t* n_jump) {
  return guarded([&] { profile_end(apply_ms, n_apply, jump_ms, n_jump); });
}

int fks_perturb(const fks_tensor* t, int32_t nt, uint64_t seed, const double* scales, void* workspace,
                size_t ws_bytes, void* stream) {
  // optimizer.py:173: scaling_factor * eps is a python double, cast to fp32 opmath
  return fks_perturb_step(t, nt, seed, scales, 1.0, FKS_VALUE_SCALAR, 0, workspace, ws_bytes, stream);
}

int fks_perturb_step(const fks_tensor* t, int32_t nt, uint64_t seed, const double* scales, double value,
                     int32_t value_kind, int32_t update, void* workspace, size_t ws_bytes, void* stream) {
  return guarded([&] {
    if (nt > 0 && !scales) throw Error(-FKS_EINVAL, "null scales");
    run(t, nt, &seed, &value, 1, value_kind, update ? kModePerturbUpdate : kModePerturb, workspace, ws_bytes, stream,
        scales);
  });
}

int fks_perturb_step_dev(const fks_tensor* t, int32_t nt, uint64_t seed, const double* scales, const float* dev_value,
                         void* workspace, size_t ws_bytes, void* stream) {
  return guarded([&] {
    if (nt > 0 && (!scales || !dev_value)) throw Error(-FKS_EINVAL, "null scales or device value");
    const double unused = 0.0;
    run(t, nt, &seed, &unused, 1, FKS_VALUE_TENSOR, kModePerturbUpdate, workspace, ws_bytes, stream, scales, 0, 1, 0,
        dev_value);
  });
}

int fks_normal(const fks_tensor* t, int32_t nt, uint64_t seed, void* workspace, size_t ws_bytes, void* stream) {
  return guarded([&] {
    const double v = 0.0;
    run(t, nt, &seed, &v, 1, FKS_VALUE_SCALAR, kModeWriteZ, workspace, ws_bytes, stream);
  });
}

int fks_plan_cache_clear(void) {
  return guarded([&] { clear_plan_cache(); });
}

const char* fks_last_error(void) { return g_last_error.c_str(); }

int32_t fks_abi_version(void) { return FKS_ABI_VERSION; }

const char* fks_build_target(void) { return "gfx950"; }

int fks_host_jump_window(uint64_t seed, int64_t block, uint32_t* out624) {
  return guarded([&] {
    if (!out624 || block < 0) throw Error(-FKS_EINVAL, "bad arguments");
    host_jump_window(seed, block, out624);
  });
}

int fks_device_selfcheck(int32_t which, uint64_t* result, void* workspace, size_t ws_bytes, void* stream) {
  return guarded([&] {
    if (!result || (which != FKS_CHECK_SQRT_DOMAIN && which != FKS_CHECK_PHILOX_RADIUS &&
                    which != FKS_CHECK_PHILOX_BF16_RADIUS))
      throw Error(-FKS_EINVAL, "bad arguments");
    device_selfcheck(which, result, workspace, ws_bytes, stream);
  });
}

int fks_host_tables(int32_t dtype, float* radius, float* cosv, float* sinv, int32_t n) {
  return guarded([&] {
    const Tables& T = tables();
    const int need = dtype == FKS_BF16 ? 256 : (dtype == FKS_F16 ? 2048 : -1);
    if (need < 0 || n < need || !radius || !cosv || !sinv) throw Error(-FKS_EINVAL, "bad arguments");
    const float* r = dtype == FKS_BF16 ? T.r_bf16 : T.r_f16;
    const float* c = dtype == FKS_BF16 ? T.c_bf16 : T.c_f16;
    const float* s = dtype == FKS_BF16 ? T.s_bf16 : T.s_f16;
    std::memcpy(radius, r, sizeof(float) * (size_t)need);
    std::memcpy(cosv, c, sizeof(float) * (size_t)need);
    std::memcpy(sinv, s, sizeof(float) * (size_t)need);
  });
}

}  // extern "C"
