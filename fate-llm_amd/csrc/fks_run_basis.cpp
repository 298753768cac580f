// fks_run_basis.cpp -- the launch drivers of the seed-basis calls (projection, Gram matrix and
// expansion, each on the torch_rocm stream and on the CPU generator's).  Every driver keeps one
// order: the geometry or layout on the host, the empty shard's exit, the workspace check, the
// host tables -- so that every argument error is raised from the arguments alone, before anything
// is allocated or launched (device_caps() reads the device's properties only and falls back to an
// MI355X's without a device; tests/test_*_host.py run the calls that way) -- and only then
// g_cache_mu, the plan, the upload and the launches, the lock held to the last of them.
#include <cstdlib>

#include "fks_run.h"

namespace fks {
namespace {

void require_workspace(const void* workspace, size_t ws_bytes, size_t need) {
  if (!workspace || ((uintptr_t)workspace % 8) != 0 || ws_bytes < need)
    throw Error(-FKS_EINVAL, "workspace too small or misaligned: need " + std::to_string(need) + " bytes, got " +
                                 std::to_string(ws_bytes));
}

// nothing in this shard: every sum is +0
void zero_result(double* dev_out, size_t count, void* stream) {
  check_hip(hipMemsetAsync(dev_out, 0, sizeof(double) * count, (hipStream_t)stream), "hipMemsetAsync");
}

// the tensors' first elements in the concatenation
std::vector<int64_t> tensor_starts(const fks_tensor* t, int nt) {
  std::vector<int64_t> start((size_t)nt, 0);
  for (int i = 1; i < nt; i++) start[i] = start[i - 1] + t[i - 1].numel;
  return start;
}

// ---- the torch_rocm stream ----
// A call's element shard: the geometry on the host and the work items [lo, hi) the shard owns.
struct PhxShard {
  DevCaps dc;
  PhxGeo geo;
  int64_t lo = 0, hi = 0;
  bool empty() const { return lo >= hi; }
  int64_t items() const { return hi - lo; }
  // the cached plan of the same geometry; under g_cache_mu, which the caller holds to its last launch
  const PhxPlan* plan(const fks_tensor* t, int nt, uint64_t base) const {
    const PhxPlan* P = get_phx_plan(t, nt, nullptr, base, dc);
    if (P->nt != geo.nt) throw Error(-FKS_EINVAL, "torch_rocm plan does not match the call's geometry");
    return P;
  }
};
PhxShard phx_shard(const fks_tensor* t, int nt, uint64_t base, int shard, int nshards) {
  PhxShard S;
  S.dc = device_caps();
  if (nt > 0) {
    S.geo = phx_geometry(t, nt, nullptr, base, S.dc.max_grid);
    S.lo = phx_boundary(S.geo, shard, nshards);
    S.hi = phx_boundary(S.geo, shard + 1, nshards);
  }
  return S;
}

// Row m of out[nvec][geo.nt]: the piece of vector (output) m under every table entry -- a tensor
// past 2^31 bytes has several entries.  vecs is [nvec][nt].
void phx_vec_table(ProjVecEntry* out, const PhxGeo& geo, const fks_tensor* t, int nt, const fks_vec* vecs, int nvec) {
  const std::vector<int64_t> start = tensor_starts(t, nt);
  for (int m = 0; m < nvec; m++)
    for (int e = 0; e < geo.nt; e++) {
      const int i = geo.tensor_of[e];
      const fks_vec& v = vecs[(size_t)m * (size_t)nt + (size_t)i];
      ProjVecEntry& x = out[(size_t)m * (size_t)geo.nt + (size_t)e];
      x.ptr = (uint64_t)(uintptr_t)v.data + (uint64_t)(geo.elem0[e] - start[i]) * elem_size(v.dtype);
      x.dtype = v.dtype;
      x.flags = (x.ptr % 16u) == 0 ? kPhxP16 : 0u;
    }
}

// ---- seed-basis projection (torch_rocm stream) ----
// fks_project_multi's workspace: the vector table of the whole call ([nvec][entries], uploaded
// once per call) in front, then the block partials of one pass of at most kProjMaxVec vectors
size_t project_table_bytes(int entries, int nvec) {
  return align_up(sizeof(ProjVecEntry) * (size_t)std::max(entries, 0) * (size_t)std::max(nvec, 0), 256);
}
// ... and the block partials a launch over `items` work items writes (fks_project.hip)
size_t project_need(int64_t items, int entries, int nvec, bool multi) {
  const size_t part = std::max<size_t>(sizeof(double) * (size_t)kPhxSeeds * (size_t)project_grid(items), 256);
  return multi ? project_table_bytes(entries, nvec) + (size_t)std::min(std::max(nvec, 1), kProjMaxVec) * part : part;
}

}  // namespace

// a shard walks at most the whole list's items; the passes of kPhxSeeds seeds follow
// each other on the stream and share the partials
size_t project_ws_bytes(const fks_tensor* t, int nt, int nvec, bool multi) {
  const PhxGeo geo = phx_geometry(t, nt, nullptr, 0, device_caps().max_grid);
  return project_need(geo.items, geo.nt, nvec, multi);
}

void project(const fks_tensor* t, int nt, const uint64_t* seeds, int k, const float* vec, const fks_vec* vecs,
             int nvec, int shard, int nshards, double* dev_out, void* workspace, size_t ws_bytes, void* stream) {
  const bool multi = vec == nullptr;
  // fks_project's table is fks_delta_accumulate's for this base; fks_project_multi's is geometry only
  const uint64_t base = (uint64_t)(uintptr_t)vec;
  const PhxShard S = phx_shard(t, nt, base, shard, nshards);
  if (S.empty()) return zero_result(dev_out, (size_t)k * (size_t)nvec, stream);
  const size_t tab_bytes = multi ? project_table_bytes(S.geo.nt, nvec) : 0;
  require_workspace(workspace, ws_bytes, project_need(S.items(), S.geo.nt, nvec, multi));
  thread_local std::vector<ProjVecEntry> host;  // the upload's source outlives the call
  if (multi) {
    host.assign((size_t)nvec * (size_t)S.geo.nt, ProjVecEntry{});
    phx_vec_table(host.data(), S.geo, t, nt, vecs, nvec);
  }
  std::lock_guard<std::mutex> lk(g_cache_mu);  // no eviction while this call uses its entry
  const PhxPlan* P = S.plan(t, nt, base);
  if (multi)
    check_hip(hipMemcpyAsync(workspace, host.data(), sizeof(ProjVecEntry) * host.size(), hipMemcpyHostToDevice,
                             (hipStream_t)stream), "hipMemcpyAsync");
  double* const partial = reinterpret_cast<double*>(static_cast<uint8_t*>(workspace) + tab_bytes);
  const int grid = project_grid(S.items());
  auto fill = [&](auto& a, int s0, int nb) {
    a.t = static_cast<const PhxTensor*>(P->dev);
    a.nt = P->nt;
    a.partial = partial;
    a.item_lo = S.lo;
    a.item_hi = S.hi;
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
// fks_gram and fks_gram_tiled are one driver over what differs: the tile.  The workspace holds the
// block partials of ONE pass, Tile::cells doubles per workgroup of a launch over `items` work
// items; the passes follow each other on the stream and share them.  Nothing depends on the seed
// counts or has the model's size.
namespace {

struct GramTile {  // kGramRows x kPhxSeeds seeds (fks_gram.h), 1 KiB of partials per workgroup
  using Args = GramArgs;
  static constexpr size_t cells = (size_t)kGramRows * (size_t)kPhxSeeds;
  static constexpr const char *kernel = "fks_gram_kernel", *reduce_kernel = "fks_gram_reduce_kernel";
  static int grid(int64_t items) { return project_grid(items); }
  static std::vector<GramPass> passes(int kr, int kc, bool symmetric) { return gram_passes(kr, kc, symmetric); }
  static void pack(Args& a, const GramPass& p, const uint64_t* rows, const uint64_t* cols) {
    for (int m = 0; m < kGramRows; m++) a.rseeds[m] = m < p.nrows ? rows[p.row0 + m] : 0;
    for (int j = 0; j < p.ncols; j++) a.seeds[j] = cols[p.col0 + j];
    a.nrows = p.nrows;
    a.nseeds = p.ncols;
  }
  static int launch(const Args& a, void* stream) { return launch_gram(a, stream); }
  static constexpr auto reduce = launch_gram_reduce;
};

struct GramMatrixTile {  // kGtRows x kGtCols seeds on the f64 matrix unit (fks_gram_tiled.h)
  using Args = GramTiledArgs;
  static constexpr size_t cells = (size_t)kGtTile;
  static constexpr const char *kernel = "fks_gram_tiled_kernel", *reduce_kernel = "fks_gram_tiled_reduce_kernel";
  static int grid(int64_t items) { return gram_tiled_grid(items); }
  static std::vector<GramPass> passes(int kr, int kc, bool symmetric) { return gram_tiled_passes(kr, kc, symmetric); }
  // seeds past a pass's counts are padded with 0 (drawn only where their 16-block is live, never written out)
  static void pack(Args& a, const GramPass& p, const uint64_t* rows, const uint64_t* cols) {
    for (int m = 0; m < kGtRows; m++) a.rseeds[m] = m < p.nrows ? rows[p.row0 + m] : 0;
    for (int j = 0; j < kGtCols; j++) a.cseeds[j] = j < p.ncols ? cols[p.col0 + j] : 0;
    a.nrb = (p.nrows + kGtSeeds - 1) / kGtSeeds;
    a.ncb = (p.ncols + kGtSeeds - 1) / kGtSeeds;
    // a column block that holds its row block's seeds takes the row block's operand (the diagonal
    // tile of a symmetric call; the same values either way)
    const int shared = std::min(a.nrb, a.ncb) * kGtSeeds;
    a.diag = std::equal(a.rseeds, a.rseeds + shared, a.cseeds) ? 1 : 0;
  }
  static int launch(const Args& a, void* stream) { return launch_gram_tiled(a, stream); }
  static constexpr auto reduce = launch_gram_tiled_reduce;
};

template <class Tile>
size_t gram_need(int64_t items) {
  return std::max<size_t>(sizeof(double) * Tile::cells * (size_t)Tile::grid(items), 256);
}

// per pass the kernel and the reduce with the matrix's addressing and the mirror
template <class Tile>
void gram_over(const fks_tensor* t, int nt, const uint64_t* rows, int kr, const uint64_t* cols, int kc, int shard,
               int nshards, double* dev_out, void* workspace, size_t ws_bytes, void* stream) {
  const bool symmetric = cols == nullptr;
  if (symmetric) {
    cols = rows;
    kc = kr;
  }
  const PhxShard S = phx_shard(t, nt, 0, shard, nshards);
  if (S.empty()) return zero_result(dev_out, (size_t)kr * (size_t)kc, stream);
  require_workspace(workspace, ws_bytes, gram_need<Tile>(S.items()));
  std::lock_guard<std::mutex> lk(g_cache_mu);  // no eviction while this call uses its entry
  const PhxPlan* P = S.plan(t, nt, 0);
  const int grid = Tile::grid(S.items());
  typename Tile::Args a{};
  a.t = static_cast<const PhxTensor*>(P->dev);
  a.nt = P->nt;
  a.partial = static_cast<double*>(workspace);
  a.item_lo = S.lo;
  a.item_hi = S.hi;
  for (const GramPass& p : Tile::passes(kr, kc, symmetric)) {
    Tile::pack(a, p, rows, cols);
    check_launch(timed(0, stream, [&] { return Tile::launch(a, stream); }), Tile::kernel, "bad arguments");
    check_launch(Tile::reduce(a.partial, grid, p.nrows, p.ncols, dev_out, kc, p.row0, p.col0, symmetric, stream),
                 Tile::reduce_kernel, "bad arguments");
  }
}

}  // namespace

size_t gram_ws_bytes(const fks_tensor* t, int nt) {
  return gram_need<GramTile>(phx_geometry(t, nt, nullptr, 0, device_caps().max_grid).items);
}
size_t gram_tiled_ws_bytes(const fks_tensor* t, int nt) {
  return gram_need<GramMatrixTile>(phx_geometry(t, nt, nullptr, 0, device_caps().max_grid).items);
}

void gram(const fks_tensor* t, int nt, const uint64_t* rows, int kr, const uint64_t* cols, int kc, int shard,
          int nshards, double* dev_out, void* workspace, size_t ws_bytes, void* stream) {
  gram_over<GramTile>(t, nt, rows, kr, cols, kc, shard, nshards, dev_out, workspace, ws_bytes, stream);
}
void gram_tiled(const fks_tensor* t, int nt, const uint64_t* rows, int kr, const uint64_t* cols, int kc, int shard,
                int nshards, double* dev_out, void* workspace, size_t ws_bytes, void* stream) {
  gram_over<GramMatrixTile>(t, nt, rows, kr, cols, kc, shard, nshards, dev_out, workspace, ws_bytes, stream);
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
  const PhxShard S = phx_shard(t, nt, 0, shard, nshards);
  if (S.empty()) return;  // nothing in this shard
  const ExpandWs W = expand_ws(S.geo.nt, k, nvec);
  require_workspace(workspace, ws_bytes, W.total);
  const std::vector<int64_t> cuts = phx_expand_cuts(S.geo, S.lo, S.hi, k, expand_launch_work());
  thread_local std::vector<uint8_t> host;  // the upload's source outlives the call
  host.assign(W.total, 0);
  phx_vec_table(reinterpret_cast<ProjVecEntry*>(host.data()), S.geo, t, nt, outs, nvec);
  if (k > 0) std::memcpy(host.data() + W.seeds_off, seeds, sizeof(uint64_t) * (size_t)k);
  float* c = reinterpret_cast<float*>(host.data() + W.coef_off);
  for (int m0 = 0; m0 < nvec; m0 += kExpMaxVec) {
    const int nv = std::min(kExpMaxVec, nvec - m0);
    float* blk = c + (size_t)k * (size_t)m0;
    for (int s = 0; s < k; s++)
      for (int m = 0; m < nv; m++) blk[(size_t)s * nv + m] = (float)coefs[(size_t)(m0 + m) * (size_t)k + s];
  }
  std::lock_guard<std::mutex> lk(g_cache_mu);  // no eviction while this call uses its entry
  const PhxPlan* P = S.plan(t, nt, 0);
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

// ---- the CPU generator's stream ----
namespace {

// The per-call table of the in-place calls over the geometry-only plan (the kModeDelta plan of
// kProjMtGeoBase: one cache entry per tensor list and shard, whatever the vectors' addresses):
// row m holds the piece of vector (output) m under every fast segment (the dtypes' segments
// behind each other, as in the plan), run and single element of the shard's clipped layout.
struct MtVecTable {
  size_t segs[3] = {0, 0, 0}, nsegs = 0, nruns = 0, ntiny = 0;
  size_t E = 0;  // entries of a row: nsegs + nruns + ntiny
  // the cached plan has the descriptors the table was built for
  bool matches(const CachedPlan& C) const {
    bool same = (size_t)C.Z.nsegs == nsegs && (size_t)C.Z.nruns == nruns && (size_t)C.Z.ntiny == ntiny;
    for (int d = 0; d < 3; d++) same = same && (size_t)C.nsegs[d] == segs[d];
    return same;
  }
};
// the table on the host, from the layout the plan is built from; vecs is [nvec][nt], `entries` what
// the call's workspace layout allows a row
MtVecTable mt_vec_table(std::vector<ProjMtVecEntry>& host, const fks_tensor* t, int nt, const fks_vec* vecs, int nvec,
                        int shard, int nshards, int entries) {
  Layout L = make_layout(t, nt, nullptr, kProjMtGeoBase);
  clip_segments(L, shard_blocks(L.stream_len, shard, nshards));
  MtVecTable T;
  for (int d = 0; d < 3; d++) T.nsegs += T.segs[d] = L.segs[d].size();
  T.nruns = L.runs.size();
  T.ntiny = L.tiny.size();
  T.E = T.nsegs + T.nruns + T.ntiny;
  if (T.E != (size_t)entries) throw Error(-FKS_EINVAL, "the layout does not match the call's workspace layout");
  const std::vector<int64_t> start = tensor_starts(t, nt);
  host.assign((size_t)nvec * T.E, ProjMtVecEntry{});
  for (int m = 0; m < nvec; m++) {
    ProjMtVecEntry* x = host.data() + (size_t)m * T.E;
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
  return T;
}

const char* const kPlanMismatch = "the plan does not match the call's workspace layout";

}  // namespace

// ---- seed-basis projection (CPU generator's stream) ----
// The plan fks_delta_accumulate launches for `vec` as its delta buffer; per pass of
// kMaxSeedsPerPass seeds the regular jump, one launch per dtype with fast segments, the irregular
// jump and launch, then the reduce over the rows all of them left.  No window, z-index or
// reconstruct-window cache: the workspace holds the windows, the sink and the partial rows.
void project_mt(const fks_tensor* t, int nt, const uint64_t* seeds, int k, const float* vec, int shard, int nshards,
                double* dev_out, void* workspace, size_t ws_bytes, void* stream) {
  const DevCaps dc = device_caps();
  const ProjMtWs W = project_mt_ws(t, nt, k, shard, nshards, dc.cus);
  if (!W.work) return zero_result(dev_out, (size_t)k, stream);
  require_workspace(workspace, ws_bytes, W.total);
  const bool libm = libm_flavour(t, nt);
  std::lock_guard<std::mutex> lk(g_cache_mu);  // no eviction while this call uses its entry
  const CachedPlan* C = get_plan(t, nt, nullptr, (uint64_t)(uintptr_t)vec, shard, nshards, /*small=*/false, dc);
  const MtPlan V{*C, dc.cus, libm, stream};
  const int rows = V.partial_rows();
  if (rows < 1 || rows > W.rows ||
      ws_bytes_for(std::max(C->Z.reg_chunks, C->Z.irr_chunks), std::min(k, kMaxSeedsPerPass)) > W.partial_off)
    throw Error(-FKS_EINVAL, kPlanMismatch);
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  uint32_t* states = reinterpret_cast<uint32_t*>(ws + kWsStatesOff);
  double* const partial = reinterpret_cast<double*>(ws + W.partial_off);
  for (int s0 = 0; s0 < k; s0 += kMaxSeedsPerPass) {
    const int nb = std::min(kMaxSeedsPerPass, k - s0);
    double* row = partial;
    if (C->have_reg) {
      V.jump_regular(seeds + s0, nb, states);
      V.each_fast_dtype([&](int d, int dd, size_t) {
        ProjMtArgs pa{};
        V.fill_fast(pa, d, states);
        pa.sink = reinterpret_cast<const uint64_t*>(ws);
        pa.partial = row;
        pa.nseeds = nb;
        check_launch(timed(0, stream, [&] { return launch_project_mt(dd, pa, stream); }), "fks_project_mt_kernel",
                     "bad arguments");
        row += (size_t)kPhxSeeds * (size_t)C->Z.reg_chunks;
      });
    }
    if (C->have_irr) {
      V.jump_irregular(seeds + s0, nb, states);
      ProjMtIrrArgs ia{};
      V.fill_irregular(ia, states);
      ia.partial = row;
      ia.nseeds = nb;
      check_launch(timed(0, stream, [&] { return launch_project_mt_irr(ia, stream); }), "fks_project_mt_irr_kernel",
                   "bad arguments");
    }
    check_launch(launch_project_reduce(partial, rows, nb, 1, dev_out + s0, 0, stream), "fks_project_reduce_kernel",
                 "bad arguments");
  }
}

// ---- ... of several vectors, each read where it lies ----
// project_mt over the geometry-only plan and the per-call table at the front of the workspace,
// uploaded in stream order.  The vectors go in batches of kProjMtMaxVec over the same seeds; a
// batch of nv vectors takes its seeds in passes of proj_mt_pass_seeds(nv), each the launches of a
// project_mt pass with rows of nv sums per seed.
void project_mt_multi(const fks_tensor* t, int nt, const uint64_t* seeds, int k, const fks_vec* vecs, int nvec,
                      int shard, int nshards, double* dev_out, void* workspace, size_t ws_bytes, void* stream) {
  const DevCaps dc = device_caps();
  const ProjMtMultiWs W = project_mt_multi_ws(t, nt, k, nvec, shard, nshards, dc.cus);
  if (!W.one.work) return zero_result(dev_out, (size_t)k * (size_t)nvec, stream);
  require_workspace(workspace, ws_bytes, W.total);
  thread_local std::vector<ProjMtVecEntry> host;  // the upload's source outlives the call
  const MtVecTable T = mt_vec_table(host, t, nt, vecs, nvec, shard, nshards, W.one.entries);
  const bool libm = libm_flavour(t, nt);
  std::lock_guard<std::mutex> lk(g_cache_mu);  // no eviction while this call uses its entry
  const CachedPlan* C = get_plan(t, nt, nullptr, kProjMtGeoBase, shard, nshards, /*small=*/false, dc);
  const MtPlan V{*C, dc.cus, libm, stream};
  const int rows = V.partial_rows();
  if (!T.matches(*C) || rows < 1 || rows > W.one.rows ||
      ws_bytes_for(std::max(C->Z.reg_chunks, C->Z.irr_chunks), std::min(k, kMaxSeedsPerPass)) > W.one.partial_off)
    throw Error(-FKS_EINVAL, kPlanMismatch);
  check_hip(hipMemcpyAsync(workspace, host.data(), sizeof(ProjMtVecEntry) * host.size(), hipMemcpyHostToDevice,
                           (hipStream_t)stream), "hipMemcpyAsync");
  const ProjMtVecEntry* table = static_cast<const ProjMtVecEntry*>(workspace);
  uint8_t* ws = static_cast<uint8_t*>(workspace) + W.inner_off;
  uint32_t* states = reinterpret_cast<uint32_t*>(ws + kWsStatesOff);
  double* const partial = reinterpret_cast<double*>(ws + W.one.partial_off);
  for (int m0 = 0; m0 < nvec; m0 += kProjMtMaxVec) {  // batches of vectors over the same seeds
    const int nv = std::min(kProjMtMaxVec, nvec - m0);
    const int per_pass = proj_mt_pass_seeds(nv);
    const ProjMtVecEntry* tab = table + (size_t)m0 * T.E;
    for (int s0 = 0; s0 < k; s0 += per_pass) {
      const int nb = std::min(per_pass, k - s0);
      double* row = partial;
      if (C->have_reg) {
        V.jump_regular(seeds + s0, nb, states);
        V.each_fast_dtype([&](int d, int dd, size_t first) {
          ProjMtMultiArgs pa{};
          V.fill_fast(pa, d, states);
          pa.sink = reinterpret_cast<const uint64_t*>(ws);
          pa.partial = row;
          pa.pv = tab + first;
          pa.stride = (int64_t)T.E;
          pa.nseeds = nb;
          pa.nvec = nv;
          check_launch(timed(0, stream, [&] { return launch_project_mt_multi(dd, pa, stream); }),
                       "fks_project_mt_multi_kernel", "bad arguments");
          row += (size_t)kPhxSeeds * (size_t)nv * (size_t)C->Z.reg_chunks;
        });
      }
      if (C->have_irr) {
        V.jump_irregular(seeds + s0, nb, states);
        ProjMtIrrMultiArgs ia{};
        V.fill_irregular(ia, states);
        ia.partial = row;
        ia.rv = tab + T.nsegs;
        ia.tv = tab + T.nsegs + T.nruns;
        ia.stride = (int64_t)T.E;
        ia.nseeds = nb;
        ia.nvec = nv;
        check_launch(timed(0, stream, [&] { return launch_project_mt_irr_multi(ia, stream); }),
                     "fks_project_mt_irr_multi_kernel", "bad arguments");
      }
      check_launch(launch_project_reduce(partial, rows, nb, nv, dev_out + (size_t)m0 * (size_t)k + s0, k, stream),
                   "fks_project_reduce_kernel", "bad arguments");
    }
  }
}

// ---- ... bit-sliced, in passes of kBsPassSeeds seeds ----
// project_mt_multi's plan and per-call table, the vectors one at a time over the same seeds.  A
// pass of at most kBsPassSeeds seeds is one jump to EVERY chunk start of the slice kernel's plan
// and one fks_project_mt_bs_kernel launch over the bf16 fast segments, whatever k; everything else
// -- the other dtypes' fast segments and the irregular work (and the bf16 fast segments of a plan
// without the slice kernel's chunk table) -- goes through project_mt_multi's one-vector launches
// in sub-passes of kMaxSeedsPerPass seeds, each with its own jumps and its own partial rows.  One
// reduce per pass adds a seed's rows in one order and overwrites its output.  No window, z-index
// or reconstruct-window cache is read or written: every window lives in the workspace.
void project_mt_bs(const fks_tensor* t, int nt, const uint64_t* seeds, int k, const fks_vec* vecs, int nvec, int shard,
                   int nshards, double* dev_out, void* workspace, size_t ws_bytes, void* stream) {
  const DevCaps dc = device_caps();
  const ProjMtBsWs W = project_mt_bs_ws(t, nt, k, nvec, shard, nshards, dc.cus);
  if (!W.one.work) return zero_result(dev_out, (size_t)k * (size_t)nvec, stream);
  require_workspace(workspace, ws_bytes, W.total);
  thread_local std::vector<ProjMtVecEntry> host;  // the upload's source outlives the call
  const MtVecTable T = mt_vec_table(host, t, nt, vecs, nvec, shard, nshards, W.one.entries);
  const bool libm = libm_flavour(t, nt);
  std::lock_guard<std::mutex> lk(g_cache_mu);  // no eviction while this call uses its entry
  const CachedPlan* C = get_plan(t, nt, nullptr, kProjMtGeoBase, shard, nshards, /*small=*/false, dc);
  const MtPlan V{*C, dc.cus, libm, stream};
  const bool bs = C->have_bs;  // the bf16 fast segments take the bit-sliced kernel
  const int nbs = bs ? C->Z.bs_chunks : 0;
  // the rows of one sub-pass: the other dtypes' fast launches, then the irregular one
  int rows = C->have_irr ? C->Z.irr_chunks : 0;
  bool reg_rest = false;
  size_t bf16_first = 0;
  V.each_fast_dtype([&](int d, int, size_t first) {
    if (bs && d == FKS_BF16) {
      bf16_first = first;
      return;
    }
    rows += C->Z.reg_chunks;
    reg_rest = true;
  });
  if (!T.matches(*C) || nbs + rows < 1 || nbs % 2 || nbs > W.bs_chunks || rows > W.one.rows ||
      ws_bytes_for(std::max(C->Z.reg_chunks, C->Z.irr_chunks), std::min(k, kMaxSeedsPerPass)) > W.one.partial_off)
    throw Error(-FKS_EINVAL, kPlanMismatch);
  check_hip(hipMemcpyAsync(workspace, host.data(), sizeof(ProjMtVecEntry) * host.size(), hipMemcpyHostToDevice,
                           (hipStream_t)stream), "hipMemcpyAsync");
  const ProjMtVecEntry* table = static_cast<const ProjMtVecEntry*>(workspace);
  const uint8_t* hdr = static_cast<const uint8_t*>(C->dev);
  uint8_t* ws = static_cast<uint8_t*>(workspace) + W.inner_off;
  const uint64_t* sink = reinterpret_cast<const uint64_t*>(ws);
  uint32_t* states = reinterpret_cast<uint32_t*>(ws + kWsStatesOff);
  double* const bs_partial = reinterpret_cast<double*>(ws + W.bs_partial_off);
  double* const sub_partial = reinterpret_cast<double*>(ws + W.sub_partial_off);
  for (int m = 0; m < nvec; m++) {  // one vector per pass of the generator: the sums leave no room for two
    const ProjMtVecEntry* tab = table + (size_t)m * T.E;
    for (int s0 = 0; s0 < k; s0 += kBsPassSeeds) {
      const int nb = std::min(kBsPassSeeds, k - s0);
      if (bs) {
        JumpArgs ja = jump_args(seeds + s0, nb, hdr, C->H.off_bs_polys, C->H.off_bs_cb, states, nbs);
        ja.stride = 1;  // every plan chunk, in both pass shapes: a (seed, chunk) sum has one form
        ja.chunks_per_wg = std::max(1, std::min(nb * nbs >= 4096 ? 32 : 16, nbs));
        check_launch(timed(1, stream, [&] { return launch_jump(ja, nb, stream); }), "fks_jump_kernel");
        ProjMtBsArgs ba{};
        ba.states = states;
        ba.segs = V.at<DevSeg>(C->seg_off[FKS_BF16]);
        ba.chunk_block = ja.chunk_block;
        ba.sink = sink;
        ba.partial = bs_partial;
        ba.pv = tab + bf16_first;
        ba.nsegs = C->nsegs[FKS_BF16];
        ba.nchunks = nbs;
        ba.nseeds = nb;
        ba.split = nb <= kBsSeeds ? 1 : 0;
        check_launch(timed(0, stream, [&] { return launch_project_mt_bs(ba, stream); }), "fks_project_mt_bs_kernel",
                     "bad arguments");
      }
      for (int u0 = 0; u0 < nb && rows > 0; u0 += kMaxSeedsPerPass) {  // the 19-seed launches' sub-passes
        const int nu = std::min(kMaxSeedsPerPass, nb - u0);
        const uint64_t* const sub_seeds = seeds + s0 + u0;
        double* row = sub_partial + W.sub_stride * (size_t)(u0 / kMaxSeedsPerPass);
        if (reg_rest) {
          V.jump_regular(sub_seeds, nu, states);
          V.each_fast_dtype([&](int d, int dd, size_t first) {
            if (bs && d == FKS_BF16) return;
            ProjMtMultiArgs pa{};
            V.fill_fast(pa, d, states);
            pa.sink = sink;
            pa.partial = row;
            pa.pv = tab + first;
            pa.stride = (int64_t)T.E;
            pa.nseeds = nu;
            pa.nvec = 1;
            check_launch(timed(0, stream, [&] { return launch_project_mt_multi(dd, pa, stream); }),
                         "fks_project_mt_multi_kernel", "bad arguments");
            row += (size_t)kPhxSeeds * (size_t)C->Z.reg_chunks;
          });
        }
        if (C->have_irr) {
          V.jump_irregular(sub_seeds, nu, states);
          ProjMtIrrMultiArgs ia{};
          V.fill_irregular(ia, states);
          ia.partial = row;
          ia.rv = tab + T.nsegs;
          ia.tv = tab + T.nsegs + T.nruns;
          ia.stride = (int64_t)T.E;
          ia.nseeds = nu;
          ia.nvec = 1;
          check_launch(timed(0, stream, [&] { return launch_project_mt_irr_multi(ia, stream); }),
                       "fks_project_mt_irr_multi_kernel", "bad arguments");
        }
      }
      check_launch(launch_project_mt_bs_reduce(bs_partial, nbs, sub_partial, rows, (int64_t)W.sub_stride, nb,
                                               dev_out + (size_t)m * (size_t)k + s0, stream),
                   "fks_project_mt_bs_reduce_kernel", "bad arguments");
    }
  }
}

// ---- ... bit-sliced, in passes of kBsSeeds seeds by kPmbtVec vectors ----
// project_mt_bs's plan and per-call table, one draw for the vectors of a tile.  A seed pass of at
// most kBsSeeds seeds is one jump to EVERY chunk start of the slice kernel's plan, kept while the
// vector tiles of that pass go by; a tile is one fks_project_mt_bs_tiled_kernel launch over the
// bf16 fast segments.  Everything else -- the other dtypes' fast segments and the irregular work
// (and the bf16 fast segments of a plan without the slice kernel's chunk table) -- goes through
// project_mt_multi's one-vector launches in sub-passes of kMaxSeedsPerPass seeds: a sub-pass's
// windows are jumped once per tile and serve the tile's vectors one after the other, each
// (vector, sub-pass) with partial rows of its own.  One reduce per tile adds an entry's rows in
// one order and overwrites it.  No window, z-index or reconstruct-window cache is read or written.
void project_mt_bs_tiled(const fks_tensor* t, int nt, const uint64_t* seeds, int k, const fks_vec* vecs, int nvec,
                         int shard, int nshards, double* dev_out, void* workspace, size_t ws_bytes, void* stream) {
  const DevCaps dc = device_caps();
  const ProjMtBsTiledWs W = project_mt_bs_tiled_ws(t, nt, k, nvec, shard, nshards, dc.cus);
  if (!W.one.work) return zero_result(dev_out, (size_t)k * (size_t)nvec, stream);
  require_workspace(workspace, ws_bytes, W.total);
  thread_local std::vector<ProjMtVecEntry> host;  // the upload's source outlives the call
  const MtVecTable T = mt_vec_table(host, t, nt, vecs, nvec, shard, nshards, W.one.entries);
  const bool libm = libm_flavour(t, nt);
  std::lock_guard<std::mutex> lk(g_cache_mu);  // no eviction while this call uses its entry
  const CachedPlan* C = get_plan(t, nt, nullptr, kProjMtGeoBase, shard, nshards, /*small=*/false, dc);
  const MtPlan V{*C, dc.cus, libm, stream};
  const bool bs = C->have_bs;  // the bf16 fast segments take the bit-sliced kernel
  const int nbs = bs ? C->Z.bs_chunks : 0;
  // the rows of one sub-pass: the other dtypes' fast launches, then the irregular one
  int rows = C->have_irr ? C->Z.irr_chunks : 0;
  bool reg_rest = false;
  size_t bf16_first = 0;
  V.each_fast_dtype([&](int d, int, size_t first) {
    if (bs && d == FKS_BF16) {
      bf16_first = first;
      return;
    }
    rows += C->Z.reg_chunks;
    reg_rest = true;
  });
  if (!T.matches(*C) || nbs + rows < 1 || nbs > W.bs_chunks || rows > W.one.rows ||
      ws_bytes_for(std::max(C->Z.reg_chunks, C->Z.irr_chunks), std::min(k, kMaxSeedsPerPass)) > W.one.partial_off)
    throw Error(-FKS_EINVAL, kPlanMismatch);
  check_hip(hipMemcpyAsync(workspace, host.data(), sizeof(ProjMtVecEntry) * host.size(), hipMemcpyHostToDevice,
                           (hipStream_t)stream), "hipMemcpyAsync");
  const ProjMtVecEntry* table = static_cast<const ProjMtVecEntry*>(workspace);
  const uint8_t* hdr = static_cast<const uint8_t*>(C->dev);
  uint8_t* ws = static_cast<uint8_t*>(workspace) + W.inner_off;
  const uint64_t* sink = reinterpret_cast<const uint64_t*>(ws);
  uint32_t* states = reinterpret_cast<uint32_t*>(ws + kWsStatesOff);
  uint32_t* const bs_states = reinterpret_cast<uint32_t*>(ws + W.bs_states_off);
  double* const bs_partial = reinterpret_cast<double*>(ws + W.bs_partial_off);
  double* const sub_partial = reinterpret_cast<double*>(ws + W.sub_partial_off);
  const size_t vec_stride = W.sub_stride * (size_t)W.subs;  // doubles between two vectors' sub-pass rows
  for (int s0 = 0; s0 < k; s0 += kBsSeeds) {
    const int nb = std::min(kBsSeeds, k - s0);
    const int64_t* bs_cb = nullptr;
    if (bs) {  // the pass's windows, once
      JumpArgs ja = jump_args(seeds + s0, nb, hdr, C->H.off_bs_polys, C->H.off_bs_cb, bs_states, nbs);
      ja.stride = 1;  // every plan chunk
      ja.chunks_per_wg = std::max(1, std::min(nb * nbs >= 4096 ? 32 : 16, nbs));
      check_launch(timed(1, stream, [&] { return launch_jump(ja, nb, stream); }), "fks_jump_kernel");
      bs_cb = ja.chunk_block;
    }
    for (int m0 = 0; m0 < nvec; m0 += kPmbtVec) {  // tiles of vectors over the same windows
      const int nv = std::min(kPmbtVec, nvec - m0);
      const ProjMtVecEntry* tab = table + (size_t)m0 * T.E;
      if (bs) {
        ProjMtBsTiledArgs ba{};
        ba.states = bs_states;
        ba.segs = V.at<DevSeg>(C->seg_off[FKS_BF16]);
        ba.chunk_block = bs_cb;
        ba.sink = sink;
        ba.partial = bs_partial;
        ba.pv = tab + bf16_first;
        ba.pv_stride = (int64_t)T.E;
        ba.nsegs = C->nsegs[FKS_BF16];
        ba.nchunks = nbs;
        ba.nseeds = nb;
        ba.nvec = nv;
        check_launch(timed(0, stream, [&] { return launch_project_mt_bs_tiled(ba, stream); }),
                     "fks_project_mt_bs_tiled_kernel", "bad arguments");
      }
      for (int u0 = 0; u0 < nb && rows > 0; u0 += kMaxSeedsPerPass) {  // the 19-seed launches' sub-passes
        const int nu = std::min(kMaxSeedsPerPass, nb - u0);
        const uint64_t* const sub_seeds = seeds + s0 + u0;
        // vector m's rows of this sub-pass; the fast launches' first
        auto rows_of = [&](int m) { return sub_partial + vec_stride * (size_t)m + W.sub_stride * (size_t)(u0 / kMaxSeedsPerPass); };
        size_t fast_rows = 0;
        if (reg_rest) {
          V.jump_regular(sub_seeds, nu, states);
          for (int m = 0; m < nv; m++) {
            double* row = rows_of(m);
            V.each_fast_dtype([&](int d, int dd, size_t first) {
              if (bs && d == FKS_BF16) return;
              ProjMtMultiArgs pa{};
              V.fill_fast(pa, d, states);
              pa.sink = sink;
              pa.partial = row;
              pa.pv = tab + (size_t)m * T.E + first;
              pa.stride = (int64_t)T.E;
              pa.nseeds = nu;
              pa.nvec = 1;
              check_launch(timed(0, stream, [&] { return launch_project_mt_multi(dd, pa, stream); }),
                           "fks_project_mt_multi_kernel", "bad arguments");
              row += (size_t)kPhxSeeds * (size_t)C->Z.reg_chunks;
            });
            fast_rows = (size_t)(row - rows_of(m));
          }
        }
        if (C->have_irr) {
          V.jump_irregular(sub_seeds, nu, states);
          for (int m = 0; m < nv; m++) {
            ProjMtIrrMultiArgs ia{};
            V.fill_irregular(ia, states);
            ia.partial = rows_of(m) + fast_rows;
            ia.rv = tab + (size_t)m * T.E + T.nsegs;
            ia.tv = tab + (size_t)m * T.E + T.nsegs + T.nruns;
            ia.stride = (int64_t)T.E;
            ia.nseeds = nu;
            ia.nvec = 1;
            check_launch(timed(0, stream, [&] { return launch_project_mt_irr_multi(ia, stream); }),
                         "fks_project_mt_irr_multi_kernel", "bad arguments");
          }
        }
      }
      check_launch(launch_project_mt_bs_tiled_reduce(bs_partial, nbs, sub_partial, rows, (int64_t)W.sub_stride,
                                                     (int64_t)vec_stride, nb, nv,
                                                     dev_out + (size_t)m0 * (size_t)k + s0, k, stream),
                   "fks_project_mt_bs_tiled_reduce_kernel", "bad arguments");
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
  const DevCaps dc = device_caps();
  GramMtWs W;
  if (nt > 0) W = gram_mt_ws(t, nt, shard, nshards, dc.cus);
  if (!W.work) return zero_result(dev_out, (size_t)kr * (size_t)kc, stream);
  require_workspace(workspace, ws_bytes, W.total);
  const bool libm = libm_flavour(t, nt);
  std::lock_guard<std::mutex> lk(g_cache_mu);  // no eviction while this call uses its entry
  const CachedPlan* C = get_plan(t, nt, nullptr, kProjMtGeoBase, shard, nshards, /*small=*/false, dc);
  const MtPlan V{*C, dc.cus, libm, stream};
  const int prows = V.partial_rows();
  if (prows < 1 || prows > W.rows || (C->have_reg && C->Z.reg_chunks > W.reg_chunks) ||
      (C->have_irr && C->Z.irr_chunks > W.irr_chunks))
    throw Error(-FKS_EINVAL, kPlanMismatch);
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  uint32_t* const reg_states = reinterpret_cast<uint32_t*>(ws);
  uint32_t* const irr_states = reinterpret_cast<uint32_t*>(ws + W.irr_off);
  double* const partial = reinterpret_cast<double*>(ws + W.partial_off);
  // one seed's windows at the regular (irregular) chunk starts, in words
  const size_t reg_win = (size_t)kMtN * (size_t)C->Z.reg_chunks, irr_win = (size_t)kMtN * (size_t)C->Z.irr_chunks;
  int tile_row0 = -1;
  for (const GramPass& p : gram_mt_passes(kr, kc, symmetric)) {
    if (p.row0 != tile_row0) {  // a new row tile: its windows, once
      tile_row0 = p.row0;
      if (C->have_reg) V.jump_regular(rows + p.row0, p.nrows, reg_states);
      if (C->have_irr) V.jump_irregular(rows + p.row0, p.nrows, irr_states);
    }
    double* row = partial;
    if (C->have_reg) {
      V.jump_regular(cols + p.col0, p.ncols, reg_states + (size_t)p.nrows * reg_win);
      V.each_fast_dtype([&](int d, int dd, size_t) {
        GramMtArgs ga{};
        V.fill_fast(ga, d, reg_states);
        ga.partial = row;
        ga.nrows = p.nrows;
        ga.ncols = p.ncols;
        check_launch(timed(0, stream, [&] { return launch_gram_mt(dd, ga, stream); }), "fks_gram_mt_kernel",
                     "bad arguments");
        row += (size_t)kGramRows * (size_t)kPhxSeeds * (size_t)C->Z.reg_chunks;
      });
    }
    if (C->have_irr) {
      V.jump_irregular(cols + p.col0, p.ncols, irr_states + (size_t)p.nrows * irr_win);
      GramMtIrrArgs ia{};
      V.fill_irregular(ia, irr_states);
      ia.partial = row;
      ia.nseeds = p.nrows + p.ncols;
      ia.nrows = p.nrows;
      ia.ncols = p.ncols;
      check_launch(timed(0, stream, [&] { return launch_gram_mt_irr(ia, stream); }), "fks_gram_mt_irr_kernel",
                   "bad arguments");
    }
    check_launch(launch_gram_reduce(partial, prows, p.nrows, p.ncols, dev_out, kc, p.row0, p.col0, symmetric, stream),
                 "fks_gram_reduce_kernel", "bad arguments");
  }
}

// ---- tiled seed-basis Gram matrix (CPU generator's stream) ----
// gram_mt's frame with a tile of kGmtTile x kGmtTile seeds: the row block's windows are jumped
// when a row tile begins and kept while its column tiles pass, the column block's per pass; the
// diagonal tile of a symmetric call has no column block of its own.  The fast segments go through
// fks_gram_mt_tiled_kernel, one launch per dtype.  The irregular work goes through
// fks_gram_mt_irr_kernel in sub-passes of ITS tile over the same windows -- jumped once per tile;
// a sub-pass's windows are copied side by side, rows then columns, as that kernel reads them --,
// each sub-pass into partial rows of its own.  The reduce adds a cell's partials in one order.
void gram_mt_tiled(const fks_tensor* t, int nt, const uint64_t* rows, int kr, const uint64_t* cols, int kc, int shard,
                   int nshards, double* dev_out, void* workspace, size_t ws_bytes, void* stream) {
  const bool symmetric = cols == nullptr;
  if (symmetric) {
    cols = rows;
    kc = kr;
  }
  const DevCaps dc = device_caps();
  GramMtTiledWs W;
  if (nt > 0) W = gram_mt_tiled_ws(t, nt, shard, nshards, dc.cus);
  if (!W.work) return zero_result(dev_out, (size_t)kr * (size_t)kc, stream);
  require_workspace(workspace, ws_bytes, W.total);
  const bool libm = libm_flavour(t, nt);
  std::lock_guard<std::mutex> lk(g_cache_mu);  // no eviction while this call uses its entry
  const CachedPlan* C = get_plan(t, nt, nullptr, kProjMtGeoBase, shard, nshards, /*small=*/false, dc);
  const MtPlan V{*C, dc.cus, libm, stream};
  const int nirr = C->have_irr ? C->Z.irr_chunks : 0;
  const int nreg = V.partial_rows() - nirr;
  if (nreg + nirr < 1 || nreg > W.reg_rows || (C->have_reg && C->Z.reg_chunks > W.reg_chunks) || nirr > W.irr_chunks)
    throw Error(-FKS_EINVAL, kPlanMismatch);
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  // one seed's windows at the regular (irregular) chunk starts, in words
  const size_t reg_win = (size_t)kMtN * (size_t)C->Z.reg_chunks, irr_win = (size_t)kMtN * (size_t)nirr;
  uint32_t* const reg_rows = reinterpret_cast<uint32_t*>(ws);
  uint32_t* const reg_cols = reg_rows + (size_t)kGmtTile * reg_win;
  uint32_t* const irr_rows = reinterpret_cast<uint32_t*>(ws + W.irr_off);
  uint32_t* const irr_cols = irr_rows + (size_t)kGmtTile * irr_win;
  uint32_t* const sub = reinterpret_cast<uint32_t*>(ws + W.sub_off);
  double* const partial = reinterpret_cast<double*>(ws + W.partial_off);
  double* const irr_partial = reinterpret_cast<double*>(ws + W.irr_partial_off);
  auto copy_windows = [&](uint32_t* dst, const uint32_t* src, int n) {
    check_hip(hipMemcpyAsync(dst, src, sizeof(uint32_t) * irr_win * (size_t)n, hipMemcpyDeviceToDevice,
                             (hipStream_t)stream), "hipMemcpyAsync");
  };
  int tile_row0 = -1;
  for (const GramPass& p : gram_mt_tiled_passes(kr, kc, symmetric)) {
    const bool diag = symmetric && p.col0 == p.row0;  // the column block holds the row block's seeds
    if (p.row0 != tile_row0) {  // a new row tile: its windows, once
      tile_row0 = p.row0;
      if (C->have_reg) V.jump_regular(rows + p.row0, p.nrows, reg_rows);
      if (C->have_irr) V.jump_irregular(rows + p.row0, p.nrows, irr_rows);
    }
    if (C->have_reg) {
      if (!diag) V.jump_regular(cols + p.col0, p.ncols, reg_cols);
      double* tile = partial;
      V.each_fast_dtype([&](int d, int dd, size_t) {
        GramMtTiledArgs ga{};
        ga.row_states = reg_rows;
        ga.col_states = diag ? nullptr : reg_cols;
        ga.segs = V.at<DevSeg>(C->seg_off[d]);
        ga.chunk_block = V.at<int64_t>(C->H.off_cb);
        ga.partial = tile;
        ga.nsegs = C->nsegs[d];
        ga.nchunks = C->Z.reg_chunks;
        ga.nrows = p.nrows;
        ga.ncols = p.ncols;
        ga.diag = diag ? 1 : 0;
        check_launch(timed(0, stream, [&] { return launch_gram_mt_tiled(dd, ga, stream); }),
                     "fks_gram_mt_tiled_kernel", "bad arguments");
        tile += (size_t)kGmtCells * (size_t)C->Z.reg_chunks;
      });
    }
    if (C->have_irr) {
      if (!diag) V.jump_irregular(cols + p.col0, p.ncols, irr_cols);
      const uint32_t* const col_src = diag ? irr_rows : irr_cols;
      for (int m0 = 0; m0 < p.nrows; m0 += kGramMtRows) {
        const int nr = std::min(kGramMtRows, p.nrows - m0);
        copy_windows(sub, irr_rows + (size_t)m0 * irr_win, nr);
        for (int n0 = 0; n0 < p.ncols; n0 += kGramMtCols) {
          const int nc = std::min(kGramMtCols, p.ncols - n0);
          copy_windows(sub + (size_t)nr * irr_win, col_src + (size_t)n0 * irr_win, nc);
          GramMtIrrArgs ia{};
          V.fill_irregular(ia, sub);
          ia.partial = irr_partial + (size_t)kGmtIrrCells * (size_t)nirr *
                                         (size_t)((m0 / kGramMtRows) * kGmtSubCols + n0 / kGramMtCols);
          ia.nseeds = nr + nc;
          ia.nrows = nr;
          ia.ncols = nc;
          check_launch(timed(0, stream, [&] { return launch_gram_mt_irr(ia, stream); }), "fks_gram_mt_irr_kernel",
                       "bad arguments");
        }
      }
    }
    check_launch(launch_gram_mt_tiled_reduce(partial, nreg, irr_partial, nirr, p.nrows, p.ncols, dev_out, kc, p.row0,
                                             p.col0, symmetric, stream),
                 "fks_gram_mt_tiled_reduce_kernel", "bad arguments");
  }
}

// ---- bit-sliced seed-basis Gram matrix (CPU generator's stream) ----
// A pass holds two blocks of kGmtTile seeds (fks_gram_mt_bs_passes): their windows are jumped to
// EVERY chunk start of the slice kernel's plan -- a diagonal pass's seeds in one launch, a pair
// pass's row block when the row block begins and its column block per pass -- and one
// fks_gram_mt_bs_kernel launch over the bf16 fast segments leaves the pass's tile(s).  Everything
// else -- the other dtypes' fast segments and the irregular work (and the bf16 fast segments of a
// plan without the slice kernel's chunk table) -- goes through gram_mt_tiled's launches, one 16 x
// 16 tile of the pass at a time over that call's window and partial areas, and the tile's reduce
// adds the bit-sliced chunks in front of them.
void gram_mt_bs(const fks_tensor* t, int nt, const uint64_t* rows, int kr, const uint64_t* cols, int kc, int shard,
                int nshards, double* dev_out, void* workspace, size_t ws_bytes, void* stream) {
  const bool symmetric = cols == nullptr;
  if (symmetric) {
    cols = rows;
    kc = kr;
  }
  const DevCaps dc = device_caps();
  GramMtBsWs W;
  if (nt > 0) W = gram_mt_bs_ws(t, nt, shard, nshards, dc.cus);
  if (!W.one.work) return zero_result(dev_out, (size_t)kr * (size_t)kc, stream);
  require_workspace(workspace, ws_bytes, W.total);
  const bool libm = libm_flavour(t, nt);
  std::lock_guard<std::mutex> lk(g_cache_mu);  // no eviction while this call uses its entry
  const CachedPlan* C = get_plan(t, nt, nullptr, kProjMtGeoBase, shard, nshards, /*small=*/false, dc);
  const MtPlan V{*C, dc.cus, libm, stream};
  const bool bs = C->have_bs;  // the bf16 fast segments take the bit-sliced kernel
  const int nbs = bs ? C->Z.bs_chunks : 0;
  const int nirr = C->have_irr ? C->Z.irr_chunks : 0;
  int nreg = 0;  // partial tiles of one tile's other fast launches
  V.each_fast_dtype([&](int d, int, size_t) { nreg += bs && d == FKS_BF16 ? 0 : C->Z.reg_chunks; });
  if (nbs + nreg + nirr < 1 || nbs > W.bs_chunks || nreg > W.one.reg_rows ||
      (nreg && C->Z.reg_chunks > W.one.reg_chunks) || nirr > W.one.irr_chunks)
    throw Error(-FKS_EINVAL, kPlanMismatch);
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  // one seed's windows at the regular (irregular, slice plan's) chunk starts, in words
  const size_t reg_win = (size_t)kMtN * (size_t)C->Z.reg_chunks, irr_win = (size_t)kMtN * (size_t)nirr;
  const size_t bs_win = (size_t)kMtN * (size_t)nbs;
  uint32_t* const reg_rows = reinterpret_cast<uint32_t*>(ws);
  uint32_t* const reg_cols = reg_rows + (size_t)kGmtTile * reg_win;
  uint32_t* const irr_rows = reinterpret_cast<uint32_t*>(ws + W.one.irr_off);
  uint32_t* const irr_cols = irr_rows + (size_t)kGmtTile * irr_win;
  uint32_t* const sub = reinterpret_cast<uint32_t*>(ws + W.one.sub_off);
  double* const partial = reinterpret_cast<double*>(ws + W.one.partial_off);
  double* const irr_partial = reinterpret_cast<double*>(ws + W.one.irr_partial_off);
  uint32_t* const bs_blk0 = reinterpret_cast<uint32_t*>(ws + W.bs_states_off);
  uint32_t* const bs_blk1 = bs_blk0 + (size_t)kGmtTile * bs_win;
  double* const bs_partial = reinterpret_cast<double*>(ws + W.bs_partial_off);
  auto copy_windows = [&](uint32_t* dst, const uint32_t* src, int n) {
    check_hip(hipMemcpyAsync(dst, src, sizeof(uint32_t) * irr_win * (size_t)n, hipMemcpyDeviceToDevice,
                             (hipStream_t)stream), "hipMemcpyAsync");
  };
  auto jump_bs = [&](const uint64_t* seeds, int n, uint32_t* states) {
    JumpArgs ja = jump_args(seeds, n, static_cast<const uint8_t*>(C->dev), C->H.off_bs_polys, C->H.off_bs_cb, states, nbs);
    ja.stride = 1;  // every plan chunk
    ja.chunks_per_wg = std::max(1, std::min(n * nbs >= 4096 ? 32 : 16, nbs));
    check_launch(timed(1, stream, [&] { return launch_jump(ja, n, stream); }), "fks_jump_kernel");
  };
  int tile_row0 = -1;  // the row block whose windows the regular and irregular areas hold
  // one 16 x 16 tile: gram_mt_tiled's pass without the launches the bit-sliced kernel stands for,
  // then the reduce over the bit-sliced launch's tile `bs_tile` (of `bs_tiles`) and their partials
  auto tile = [&](int row0, int nr, int col0, int nc, int bs_tile, int bs_tiles) {
    const bool diag = symmetric && col0 == row0;  // the column block holds the row block's seeds
    if (nreg + nirr > 0 && row0 != tile_row0) {
      tile_row0 = row0;
      if (nreg) V.jump_regular(rows + row0, nr, reg_rows);
      if (nirr) V.jump_irregular(rows + row0, nr, irr_rows);
    }
    if (nreg) {
      if (!diag) V.jump_regular(cols + col0, nc, reg_cols);
      double* out = partial;
      V.each_fast_dtype([&](int d, int dd, size_t) {
        if (bs && d == FKS_BF16) return;
        GramMtTiledArgs ga{};
        ga.row_states = reg_rows;
        ga.col_states = diag ? nullptr : reg_cols;
        ga.segs = V.at<DevSeg>(C->seg_off[d]);
        ga.chunk_block = V.at<int64_t>(C->H.off_cb);
        ga.partial = out;
        ga.nsegs = C->nsegs[d];
        ga.nchunks = C->Z.reg_chunks;
        ga.nrows = nr;
        ga.ncols = nc;
        ga.diag = diag ? 1 : 0;
        check_launch(timed(0, stream, [&] { return launch_gram_mt_tiled(dd, ga, stream); }),
                     "fks_gram_mt_tiled_kernel", "bad arguments");
        out += (size_t)kGmtCells * (size_t)C->Z.reg_chunks;
      });
    }
    if (nirr) {
      if (!diag) V.jump_irregular(cols + col0, nc, irr_cols);
      const uint32_t* const col_src = diag ? irr_rows : irr_cols;
      for (int m0 = 0; m0 < nr; m0 += kGramMtRows) {
        const int mr = std::min(kGramMtRows, nr - m0);
        copy_windows(sub, irr_rows + (size_t)m0 * irr_win, mr);
        for (int n0 = 0; n0 < nc; n0 += kGramMtCols) {
          const int mc = std::min(kGramMtCols, nc - n0);
          copy_windows(sub + (size_t)mr * irr_win, col_src + (size_t)n0 * irr_win, mc);
          GramMtIrrArgs ia{};
          V.fill_irregular(ia, sub);
          ia.partial = irr_partial + (size_t)kGmtIrrCells * (size_t)nirr *
                                         (size_t)((m0 / kGramMtRows) * kGmtSubCols + n0 / kGramMtCols);
          ia.nseeds = mr + mc;
          ia.nrows = mr;
          ia.ncols = mc;
          check_launch(timed(0, stream, [&] { return launch_gram_mt_irr(ia, stream); }), "fks_gram_mt_irr_kernel",
                       "bad arguments");
        }
      }
    }
    check_launch(launch_gram_mt_bs_reduce(bs_partial + (size_t)bs_tile * kGmtCells, nbs, (int64_t)bs_tiles * kGmtCells,
                                          partial, nreg, irr_partial, nirr, nr, nc, dev_out, kc, row0, col0, symmetric,
                                          stream),
                 "fks_gram_mt_bs_reduce_kernel", "bad arguments");
  };
  int bs_row0 = -1;  // the row block whose windows bs_blk0 holds
  for (const GramPass& p : gram_mt_bs_passes(kr, kc, symmetric)) {
    const bool diag = symmetric && p.col0 == p.row0;  // up to kGmbsPassSeeds consecutive seeds
    const int n0 = std::min<int>(p.nrows, kGmtTile), n1 = diag ? p.nrows - n0 : p.ncols;
    if (bs) {
      if (diag) {
        jump_bs(rows + p.row0, p.nrows, bs_blk0);  // (bs_blk1 lies kGmtTile seeds behind bs_blk0)
        bs_row0 = -1;
      } else {
        if (p.row0 != bs_row0) {  // a new row block: its windows, once
          bs_row0 = p.row0;
          jump_bs(rows + p.row0, n0, bs_blk0);
        }
        jump_bs(cols + p.col0, n1, bs_blk1);
      }
      GramMtBsArgs ba{};
      ba.blk0 = bs_blk0;
      ba.blk1 = bs_blk1;
      ba.segs = V.at<DevSeg>(C->seg_off[FKS_BF16]);
      ba.chunk_block = V.at<int64_t>(C->H.off_bs_cb);
      ba.partial = bs_partial;
      ba.nsegs = C->nsegs[FKS_BF16];
      ba.nchunks = nbs;
      ba.n0 = n0;
      ba.n1 = n1;
      ba.diag = diag ? 1 : 0;
      check_launch(timed(0, stream, [&] { return launch_gram_mt_bs(ba, stream); }), "fks_gram_mt_bs_kernel",
                   "bad arguments");
    }
    if (!diag) {
      tile(p.row0, p.nrows, p.col0, p.ncols, 0, 1);
    } else {
      // the second block's diagonal tile first: the first block's windows then stay for the pair
      // passes of its row block, which follow
      if (n1) tile(p.row0 + kGmtTile, n1, p.col0 + kGmtTile, n1, 2, kGmbsDiagTiles);
      tile(p.row0, n0, p.col0, n0, 0, kGmbsDiagTiles);
      if (n1) tile(p.row0, n0, p.col0 + kGmtTile, n1, 1, kGmbsDiagTiles);
    }
  }
}

// ---- seed-basis expansion (CPU generator's stream) ----
// project_mt_multi's frame run the other way: the geometry-only plan, the per-call table of the
// outputs' pieces at the front of the workspace, then per output the passes of kMaxSeedsPerPass
// seeds -- the regular jump, one launch per dtype with fast segments, the irregular jump and
// launch.  A call of more than one pass keeps one output's f32 sums in the staging area at the
// back of the workspace between its passes (fks_expand_mt.h); k == 0 is one pass without seeds
// (and so without jumps: MtPlan's jumps launch nothing for no seed).
void expand_mt_multi(const fks_tensor* t, int nt, const uint64_t* seeds, const double* coefs, int k, const fks_vec* outs,
                     const double* betas, int nvec, int shard, int nshards, void* workspace, size_t ws_bytes,
                     void* stream) {
  const DevCaps dc = device_caps();
  const ExpMtWs W = expand_mt_ws(t, nt, k, nvec, shard, nshards, dc.cus);
  if (!W.work) return;  // nothing in this shard
  require_workspace(workspace, ws_bytes, W.total);
  thread_local std::vector<ProjMtVecEntry> host;  // the upload's source outlives the call
  const MtVecTable T = mt_vec_table(host, t, nt, outs, nvec, shard, nshards, W.entries);
  const bool libm = libm_flavour(t, nt);
  std::lock_guard<std::mutex> lk(g_cache_mu);  // no eviction while this call uses its entry
  const CachedPlan* C = get_plan(t, nt, nullptr, kProjMtGeoBase, shard, nshards, /*small=*/false, dc);
  if (!T.matches(*C) || (!C->have_reg && !C->have_irr) || (C->have_reg && C->Z.reg_chunks > W.reg_chunks) ||
      (C->have_irr && C->Z.irr_chunks > W.irr_chunks))
    throw Error(-FKS_EINVAL, kPlanMismatch);
  check_hip(hipMemcpyAsync(workspace, host.data(), sizeof(ProjMtVecEntry) * host.size(), hipMemcpyHostToDevice,
                           (hipStream_t)stream), "hipMemcpyAsync");
  const MtPlan V{*C, dc.cus, libm, stream};
  const ProjMtVecEntry* table = static_cast<const ProjMtVecEntry*>(workspace);
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  uint32_t* states = reinterpret_cast<uint32_t*>(ws + W.win_off);
  const uint64_t* sink = reinterpret_cast<const uint64_t*>(ws + W.sink_off);
  const int passes = std::max(1, (k + kMaxSeedsPerPass - 1) / kMaxSeedsPerPass);
  for (int m = 0; m < nvec; m++) {  // one output per pass of the generator
    const ProjMtVecEntry* tab = table + (size_t)m * T.E;
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
        V.jump_regular(seeds + s0, nb, states);
        V.each_fast_dtype([&](int d, int dd, size_t first) {
          ExpMtArgs ea{};
          ea.p = ps;
          V.fill_fast(ea, d, states);
          ea.sink = sink;
          ea.pv = tab + first;
          check_launch(timed(0, stream, [&] { return launch_expand_mt(dd, ea, stream); }), "fks_expand_mt_kernel",
                       "bad arguments");
        });
      }
      if (C->have_irr) {
        V.jump_irregular(seeds + s0, nb, states);
        ExpMtIrrArgs ia{};
        ia.p = ps;
        V.fill_irregular(ia, states);
        ia.rv = tab + T.nsegs;
        ia.tv = tab + T.nsegs + T.nruns;
        ia.nseeds = nb;
        check_launch(timed(0, stream, [&] { return launch_expand_mt_irr(ia, stream); }), "fks_expand_mt_irr_kernel",
                     "bad arguments");
      }
    }
  }
}

// ---- ... bit-sliced, the bf16 fast segments in passes of kBsSeeds seeds ----
// expand_mt_multi's frame -- the geometry-only plan, the per-call table, one output at a time --
// with two independent pass sequences over disjoint elements of the output: the bf16 fast segments
// under the slice kernel's chunk table in passes of kBsSeeds (one jump to EVERY chunk start, one
// fks_expand_mt_bs_kernel launch), everything else in passes of kMaxSeedsPerPass through
// expand_mt_multi's own launches.  Each sequence has its own carry_in / to_stage; both stage at
// ExpMtPass's addresses, so one area serves, and one window area, since the launches follow each
// other on the stream.  Without seeds, or without the chunk table, the bf16 fast segments take the
// 19-seed launches too: expand_mt_multi's path.
void expand_mt_bs(const fks_tensor* t, int nt, const uint64_t* seeds, const double* coefs, int k, const fks_vec* outs,
                  const double* betas, int nvec, int shard, int nshards, void* workspace, size_t ws_bytes, void* stream) {
  const DevCaps dc = device_caps();
  const ExpMtBsWs W = expand_mt_bs_ws(t, nt, k, nvec, shard, nshards, dc.cus);
  if (!W.one.work) return;  // nothing in this shard
  require_workspace(workspace, ws_bytes, W.total);
  thread_local std::vector<ProjMtVecEntry> host;  // the upload's source outlives the call
  const MtVecTable T = mt_vec_table(host, t, nt, outs, nvec, shard, nshards, W.one.entries);
  const bool libm = libm_flavour(t, nt);
  std::lock_guard<std::mutex> lk(g_cache_mu);  // no eviction while this call uses its entry
  const CachedPlan* C = get_plan(t, nt, nullptr, kProjMtGeoBase, shard, nshards, /*small=*/false, dc);
  const bool bs = C->have_bs && k > 0;  // the bf16 fast segments take the bit-sliced kernel
  const int nbs = bs ? C->Z.bs_chunks : 0;
  if (!T.matches(*C) || (!C->have_reg && !C->have_irr) || (C->have_reg && C->Z.reg_chunks > W.one.reg_chunks) ||
      (C->have_irr && C->Z.irr_chunks > W.one.irr_chunks) || nbs % 2 || nbs > W.bs_chunks || (bs && nbs < 2))
    throw Error(-FKS_EINVAL, kPlanMismatch);
  check_hip(hipMemcpyAsync(workspace, host.data(), sizeof(ProjMtVecEntry) * host.size(), hipMemcpyHostToDevice,
                           (hipStream_t)stream), "hipMemcpyAsync");
  const MtPlan V{*C, dc.cus, libm, stream};
  const ProjMtVecEntry* table = static_cast<const ProjMtVecEntry*>(workspace);
  const uint8_t* hdr = static_cast<const uint8_t*>(C->dev);
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  uint32_t* states = reinterpret_cast<uint32_t*>(ws + W.win_off);
  const uint64_t* sink = reinterpret_cast<const uint64_t*>(ws + W.sink_off);
  const uint64_t stage_bias = (uint64_t)(uintptr_t)(ws + W.stage_off) - kProjMtGeoBase - 4u * (uint64_t)W.one.elem_lo;
  // the 19-seed launches' share of the fast segments, and whether they have any work at all
  bool reg_rest = false;
  size_t bf16_first = 0;
  V.each_fast_dtype([&](int d, int, size_t first) {
    if (bs && d == FKS_BF16) bf16_first = first;
    else reg_rest = true;
  });
  const bool rest = reg_rest || C->have_irr;
  if ((bs && k > kBsSeeds && !W.stage_bytes) || (rest && k > kMaxSeedsPerPass && !W.stage_bytes))
    throw Error(-FKS_EINVAL, kPlanMismatch);
  const int bs_passes = bs ? (k + kBsSeeds - 1) / kBsSeeds : 0;
  const int passes = rest ? std::max(1, (k + kMaxSeedsPerPass - 1) / kMaxSeedsPerPass) : 0;
  for (int m = 0; m < nvec; m++) {  // one output per pass of the generator
    const ProjMtVecEntry* tab = table + (size_t)m * T.E;
    const double beta = betas ? betas[m] : 0.0;
    const double* const cm = coefs + (size_t)m * (size_t)k;
    for (int p = 0; p < bs_passes; p++) {  // the bf16 fast segments, kBsSeeds seeds a pass
      const int s0 = p * kBsSeeds, nb = std::min(kBsSeeds, k - s0);
      JumpArgs ja = jump_args(seeds + s0, nb, hdr, C->H.off_bs_polys, C->H.off_bs_cb, states, nbs);
      ja.stride = 1;  // every plan chunk: a half runs one
      ja.chunks_per_wg = std::max(1, std::min(nb * nbs >= 4096 ? 32 : 16, nbs));
      check_launch(timed(1, stream, [&] { return launch_jump(ja, nb, stream); }), "fks_jump_kernel");
      ExpMtBsArgs ba{};
      for (int j = 0; j < nb; j++) ba.g[j] = (float)cm[s0 + j];
      ba.states = states;
      ba.segs = V.at<DevSeg>(C->seg_off[FKS_BF16]);
      ba.chunk_block = ja.chunk_block;
      ba.sink = sink;
      ba.pv = tab + bf16_first;
      ba.stage_bias = stage_bias;
      ba.beta = (float)beta;
      ba.nseeds = nb;
      ba.carry_in = p > 0 ? 1 : 0;
      ba.to_stage = p + 1 < bs_passes ? 1 : 0;
      ba.read_old = beta != 0.0 ? 1 : 0;
      ba.nsegs = C->nsegs[FKS_BF16];
      ba.nchunks = nbs;
      check_launch(timed(0, stream, [&] { return launch_expand_mt_bs(ba, stream); }), "fks_expand_mt_bs_kernel",
                   "bad arguments");
    }
    for (int p = 0; p < passes; p++) {  // everything else, exactly as expand_mt_multi issues it
      const int s0 = p * kMaxSeedsPerPass, nb = std::min(kMaxSeedsPerPass, k - s0);
      ExpMtPass ps{};
      for (int j = 0; j < nb; j++) ps.g[j] = (float)cm[s0 + j];
      ps.stage_bias = stage_bias;
      ps.beta = (float)beta;
      ps.nseeds = nb;
      ps.carry_in = p > 0 ? 1 : 0;
      ps.to_stage = p + 1 < passes ? 1 : 0;
      ps.read_old = beta != 0.0 ? 1 : 0;
      if (reg_rest) {
        V.jump_regular(seeds + s0, nb, states);
        V.each_fast_dtype([&](int d, int dd, size_t first) {
          if (bs && d == FKS_BF16) return;
          ExpMtArgs ea{};
          ea.p = ps;
          V.fill_fast(ea, d, states);
          ea.sink = sink;
          ea.pv = tab + first;
          check_launch(timed(0, stream, [&] { return launch_expand_mt(dd, ea, stream); }), "fks_expand_mt_kernel",
                       "bad arguments");
        });
      }
      if (C->have_irr) {
        V.jump_irregular(seeds + s0, nb, states);
        ExpMtIrrArgs ia{};
        ia.p = ps;
        V.fill_irregular(ia, states);
        ia.rv = tab + T.nsegs;
        ia.tv = tab + T.nsegs + T.nruns;
        ia.nseeds = nb;
        check_launch(timed(0, stream, [&] { return launch_expand_mt_irr(ia, stream); }), "fks_expand_mt_irr_kernel",
                     "bad arguments");
      }
    }
  }
}

}  // namespace fks
