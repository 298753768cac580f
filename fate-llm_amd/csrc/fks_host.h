// fks_host.h -- host-internal declarations of libfks.so: fks_layout.cpp and fks_phx.cpp (pure
// planning: no HIP, the device's CU count and grid cap are arguments), fks_cache.cpp, fks_run.cpp
// and fks_capi.cpp.  Never included by a .hip file.
#pragma once

#include <algorithm>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <utility>

#include "fks_internal.h"
#include "fks_project_mt.h"
#include "fks_expand.h"
#include "fks_expand_mt.h"
#include "fks_gram.h"
#include "fks_gram_mt.h"
#include "fks_gram_tiled.h"

namespace fks {

inline size_t elem_size(int dtype) { return dtype == FKS_F32 ? 4 : 2; }
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
inline bool rocm_stream(const fks_tensor* t, int nt) { return nt > 0 && (t[0].flags & FKS_STREAM_ROCM) != 0; }
// (fp32 z of the CPU stream from normal_fill_16<float> with glibc's functions: kDtF32Libm)
inline bool libm_flavour(const fks_tensor* t, int nt) { return nt > 0 && (t[0].flags & FKS_LIBM) != 0; }

// ================================================================== fks_layout.cpp
// validate_basics: numel, dtype and pointer alignment only (all fks_digest reads)
void validate_basics(const fks_tensor* t, int nt);
void validate(const fks_tensor* t, int nt);
void check_shard(int shard, int nshards);

// Stream layout: where every tensor's draws sit in the per-seed MT19937 stream.
struct Layout {
  int64_t stream_len = 0;
  std::vector<DevSeg> segs[3];  // fast-path segments per dtype (non-frozen tensors only)
  std::vector<DevRun> runs;     // irregular 16-block runs (all dtypes), sorted by start
  std::vector<DevTiny> tiny;    // single elements of numel < 16 tensors, sorted by word
  // host-only: the tensor index of every segment / run / element (fks_shard_census)
  std::vector<int> seg_tensor[3], run_tensor, tiny_tensor;
  // seed-sharded variant (fks_delta_accumulate): the descriptors address the f32 delta
  // buffer (element e of tensor i at delta[cum_numel(i) + e]) instead of the parameters;
  // the dtype still selects the z generator
  bool delta = false;
  // the generator after the list's draws: CPUGeneratorImpl::next_double_normal_sample holds
  // the second value of the Box-Muller pair at stream word end_pair (fks_cpu_generator_end)
  bool end_cached = false;
  int64_t end_pair = 0;
};
// bytes per element of what the kernels load and store
inline size_t stor_size(const Layout& L, int dtype) { return L.delta ? 4 : elem_size(dtype); }
Layout make_layout(const fks_tensor* t, int nt, const double* scales = nullptr, uint64_t delta_base = 0);

// MT blocks of the whole stream and the [lo, hi) range shard `shard` of `nshards` owns
struct BlockRange { int64_t lo, hi; };
BlockRange shard_blocks(int64_t stream_len, int shard, int nshards);
void clip_segments(Layout& L, BlockRange r);
inline int64_t block_of(int64_t w) { return w / kMtN; }  // MT block holding stream word w

// chunks of the apply kernels' / the slice kernel's plan on a device of `cus` CUs
int plan_nchunks(int64_t nblocks, bool small, int cus);
int bs_nchunks(int64_t nblocks, int cus);
std::vector<int64_t> chunk_table(BlockRange r, int nchunks);  // MT blocks [cb[c], cb[c + 1]) per workgroup

// Chunks of the irregular kernel: chunk c twists blocks [lo[c], hi[c])
struct IrrChunks { std::vector<int64_t> lo, hi; };
std::vector<std::pair<int64_t, int64_t>> irregular_owner_intervals(const Layout& L);  // merged, [a, b)
IrrChunks irregular_chunks(const Layout& L, int cus);

// Static header of a call: everything that depends only on the tensor list, the
// perturbation scales, the shard and the chunk policy -- the chunk table, the jump
// polynomials and the segment / run / element descriptors.  It lives on the device in
// the plan cache and is uploaded once per distinct tensor list; the per-pass seeds and
// multipliers travel by value in the kernel arguments.
struct HdrSizes {
  int reg_chunks = 0, irr_chunks = 0, nsegs = 0, nruns = 0, ntiny = 0;
  int bs_chunks = 0;  // the bf16 slice kernel's own chunk plan (0: not used)
};
struct HdrLayout {
  size_t off_polys = 0, off_cb = 0, off_ipolys = 0, off_ilo = 0, off_ihi = 0, off_segs = 0, off_runs = 0,
         off_tiny = 0, off_bs_polys = 0, off_bs_cb = 0;
  size_t total = 0;
};

// what the launch driver reads of a header besides its device copy
struct PlanInfo {
  HdrLayout H;
  HdrSizes Z;
  size_t seg_off[3] = {0, 0, 0};
  int nsegs[3] = {0, 0, 0};
  int wd_mode[3] = {kModeUpdate, kModeUpdate, kModeUpdate};  // kModeUpdateWd / NoWd when uniform
  bool have_reg = false, have_irr = false;
  bool have_bs = false;  // bf16 fast segments with their slice-kernel plan (non-small calls)
  // the bf16 fast segments' analogue of PhxPlan::wd_pos0 / max_lr: every one of them has wd = +0.0
  // exactly and a finite lr (the slice kernel's kModeUpdateWdPos0 candidate), and max |lr| over them
  bool bs_wd_pos0 = false;
  float bs_max_lr = 0.0f;
  uint64_t chunk_hash = 0;  // the chunk starts (regular + irregular): what a seed's windows depend on
  int64_t reg_lo = 0, reg_hi = 0;  // MT blocks [reg_lo, reg_hi) the regular chunks cover
  uint64_t bf16_hash = 0;  // the bf16 segments' stream ranges: which blocks a z-index store covers
  uint64_t bs_hash = 0;    // the slice-kernel plan's chunk starts: what its seeds' windows depend on
};
// the header's H.total bytes and the fields derived from them, on the host
struct PlanImage { std::vector<uint8_t> bytes; PlanInfo info; };
PlanImage plan_image(const fks_tensor* t, int nt, const double* scales, uint64_t delta_base, int shard, int nshards,
                     bool small, int cus);

// Caller's workspace: [sink 4 KB | generator windows of one pass]; the small-K kernel's
// lanes read a whole block's worth of sink when their block is not a fast one
constexpr size_t kWsStatesOff = 4096;
size_t ws_bytes_for(int chunks, int seeds_per_pass);
size_t workspace_total(const fks_tensor* t, int nt, int k, uint64_t delta_base, int cus);
// fks_project_mt's workspace for one shard's plan (bounds; shard 0 of 1 bounds every shard)
struct ProjMtWs {
  size_t partial_off = 0, total = 0;  // where the partial rows start; bytes in all
  int rows = 0;                       // partial rows of one pass, at most
  bool work = false;                  // the shard holds an element of a non-frozen tensor
  int entries = 0;                    // descriptors of the shard's plan: fast segments + runs + single elements
};
ProjMtWs project_mt_ws(const fks_tensor* t, int nt, int k, int shard, int nshards, int cus);
// fks_project_mt_multi's: [vector table: nvec x entries pieces | fks_project_mt's layout, its
// partial rows widened to the vectors of one pass]
struct ProjMtMultiWs {
  ProjMtWs one;            // the one-vector layout behind the table (offsets from inner_off)
  size_t inner_off = 0;    // bytes of the table, 256-aligned
  size_t total = 0;
  int pass_vec = 0;        // vectors per pass: min(nvec, kProjMtMaxVec), at least 1
};
ProjMtMultiWs project_mt_multi_ws(const fks_tensor* t, int nt, int k, int nvec, int shard, int nshards, int cus);
// fks_expand_mt_multi's, for one shard's plan: [output table: nvec x entries pieces | generator
// windows of one pass | sink 4 KB | f32 staging area of one output].  The staging area exists for
// k > kMaxSeedsPerPass only and holds the elements of the concatenation from the first to the last
// one any descriptor of the shard's clipped layout touches.
struct ExpMtWs {
  bool work = false;       // the shard holds an element of a non-frozen tensor
  int entries = 0;         // descriptors of the shard's plan: fast segments + runs + single elements
  int reg_chunks = 0, irr_chunks = 0;  // chunks of the plan's launches, at most
  int64_t elem_lo = 0, elem_hi = 0;    // the span [elem_lo, elem_hi) of the concatenation the shard touches
  size_t win_off = 0, sink_off = 0, stage_off = 0, stage_bytes = 0, total = 0;
};
ExpMtWs expand_mt_ws(const fks_tensor* t, int nt, int k, int nvec, int shard, int nshards, int cus);
// fks_gram_mt's, for one shard's plan (bounds; shard 0 of 1 bounds every shard): [row tile's and
// column tile's windows at the regular chunk starts | the same at the irregular chunk starts |
// partial rows of one pass].  The seed counts enter as min(k, tile) only.
struct GramMtWs {
  bool work = false;                   // the shard holds an element of a non-frozen tensor
  int reg_chunks = 0, irr_chunks = 0;  // chunks of the plan's launches, at most
  int rows = 0;                        // partial rows of one pass, at most
  size_t irr_off = 0, partial_off = 0, total = 0;
};
GramMtWs gram_mt_ws(const fks_tensor* t, int nt, int shard, int nshards, int cus);

// the weight-decay form all of a launch's descriptors (segments, Philox entries) share, or kModeUpdate
template <class D>
int wd_form(const std::vector<D>& v, bool allow_wd0 = true) {
  size_t nwd = 0, nwd0 = 0;
  for (const D& x : v) {
    nwd += (x.flags & FKS_HAS_WD) ? 1 : 0;
    nwd0 += ((x.flags & FKS_HAS_WD) && x.wd == 0.0f) ? 1 : 0;  // +0.0 or -0.0
  }
  if (v.empty()) return kModeUpdate;
  if (nwd0 == v.size() && allow_wd0) return kModeUpdateWd0;
  return nwd == v.size() ? kModeUpdateWd : (nwd == 0 ? kModeUpdateNoWd : kModeUpdate);
}

// a 0-dim fp32 tensor g enters `g * z` as the first operand: torch casts it to the
// parameter dtype first (zo step's g, optimizer.py:147)
float round_to_dtype(double v, int dtype);
// the multiplier the kernels of dtype `dtype` see for the caller's value v
inline float g_value(int value_kind, double v, int dtype) {
  return value_kind == FKS_VALUE_TENSOR ? round_to_dtype(v, dtype) : (float)v;
}

template <class T>
void key_put(std::vector<uint8_t>& k, const T& v) {
  const uint8_t* p = reinterpret_cast<const uint8_t*>(&v);
  k.insert(k.end(), p, p + sizeof(T));
}
uint64_t fnv1a(const std::vector<uint8_t>& b);

void mt_census(const fks_tensor* t, int nt, int shard, int nshards, int64_t* word_range, int64_t* written);
void cpu_generator_end(const fks_tensor* t, int nt, uint64_t seed, uint32_t* state624, int32_t* left, uint32_t* next,
                       int32_t* normal_valid, double* normal);

// The sets of the reconstruct window cache (JWin below): which window set holds which seed;
// sets are recycled in clock order, never one the current pass still needs.
struct JwSets {
  uint32_t nsets = 0, clock = 0;
  uint64_t pass = 0;                       // passes seen (stamps the sets a pass uses)
  std::unordered_map<uint64_t, uint32_t> where;  // seed -> set
  std::vector<uint64_t> set_seed;          // set -> seed (valid when set_used[s])
  std::vector<uint8_t> set_used;
  std::vector<uint64_t> set_pass;          // the last pass that used the set
  uint64_t hits = 0, misses = 0;
};
void jw_reset(JwSets& S, uint32_t nsets);  // every set free (the counters stay)
// Sets for the nb seeds of one two-slice pass: slot[j] = seed j's set; the seeds that
// missed (their windows still to be jumped) are listed in miss / miss_slot.
void jw_assign(JwSets& S, const uint64_t* seeds, int nb, uint32_t* slot, uint64_t* miss, uint32_t* miss_slot,
               int& nmiss);

// ================================================================== fks_phx.cpp
// The tensor table of a FKS_STREAM_ROCM call (PhxTensor) and its geometry: torch's
// calc_execution_policy (ATen/native/cuda/DistributionTemplates.h:50-62) under a grid cap.
struct PhxGeo {
  int nt = 0;           // table entries (tensors with work items)
  int64_t items = 0;    // work items of all tensors
  int wd_mode = kModeUpdate;  // kModeUpdateWd / NoWd / Wd0 when every tensor shares the form
  bool wd_pos0 = false;        // Wd0 with wd = +0.0 on bf16 / f32 tensors only (kModeUpdateWdPos0 candidate)
  float max_lr = 0.0f;         // max |lr| over the table (the WdPos0 bound)
  std::vector<PhxTensor> tab;  // host copy of the table
  std::vector<int64_t> elem0;  // per entry: its first element in the concatenation of ALL the call's tensors
  std::vector<int> tensor_of;  // per entry: the tensor it belongs to (a tensor past 2^31 bytes has several)
  int64_t elems = 0;           // elements of all the call's tensors
  uint64_t off4_total = 0;     // the Philox offset / 4 one seed's draws advance the generator by
};
bool phx_fits32(int64_t m, size_t es);
void phx_policy(int64_t m, int64_t max_grid, int64_t& stride, int64_t& J);
PhxGeo phx_geometry(const fks_tensor* t, int nt, const double* scales, uint64_t delta_base, int64_t max_grid);
int64_t phx_boundary(const PhxGeo& P, int shard, int nshards);  // shard's first work item
int64_t phx_boundary_elem(const PhxGeo& P, int64_t b);
void phx_census(const PhxGeo& P, int nt, int shard, int nshards, int64_t* word_range, int64_t* written);
// fks_expand_multi's launch cuts of the items [lo, hi): row boundaries lo = b[0] < ... < b[n] = hi, each
// launch at most `work` seed-elements (4 per item x max(k, 1)) or a single row
std::vector<int64_t> phx_expand_cuts(const PhxGeo& P, int64_t lo, int64_t hi, int k, int64_t work);
// fks_gram's passes, in launch order: rows [row0, row0 + nrows) against columns [col0, col0 + ncols),
// at most kGramRows x kPhxSeeds; a symmetric call covers the pairs col >= row (and its diagonal tiles whole)
struct GramPass { int32_t row0, nrows, col0, ncols; };
std::vector<GramPass> gram_passes(int krows, int kcols, bool symmetric);
// fks_gram_mt's: the same order for its tile of kGramMtRows x kGramMtCols (fks_gram_mt.h)
std::vector<GramPass> gram_mt_passes(int krows, int kcols, bool symmetric);
// fks_gram_tiled's: the same order for its tile of kGtRows x kGtCols (fks_gram_tiled.h)
std::vector<GramPass> gram_tiled_passes(int krows, int kcols, bool symmetric);

// ================================================================== fks_cache.cpp
// the current device and what the planning reads of it, read once per call
struct DevCaps {
  int device = 0, cus = 0, threads_per_cu = 0;
  int64_t max_grid = 0;  // torch's grid cap: cus x (threads_per_cu / 256) blocks
};
DevCaps device_caps(bool require = false);  // require: throws when there is no current HIP device

// A device-resident table in a bounded LRU, keyed by every input it depends on (the full
// key is compared, not only its hash).
struct Resident {
  std::vector<uint8_t> key;
  uint64_t hash = 0, last_use = 0;
  void* dev = nullptr;
  int device = 0;  // the HIP device `dev` lives on
};
struct CachedPlan : Resident, PlanInfo {};
struct PhxPlan : Resident, PhxGeo {};
// guards every cache; a call holds it from its plan lookup to its last launch (no eviction meanwhile)
extern std::mutex g_cache_mu;
const CachedPlan* get_plan(const fks_tensor* t, int nt, const double* scales, uint64_t delta_base, int shard,
                           int nshards, bool small, const DevCaps& dc);
const PhxPlan* get_phx_plan(const fks_tensor* t, int nt, const double* scales, uint64_t delta_base, const DevCaps& dc);
void clear_plan_cache();
bool env_on(const char* name);

// A per-device buffer shared by calls on any stream: every call that uses it records
// `done` on its stream after its launches, and a call on another stream first makes its
// stream wait for that event (no host synchronisation).
struct DevBuf {
  int device = -1;
  void* buf = nullptr;
  size_t bytes = 0;
  void* stream = nullptr;  // the stream of the last call that used the buffer
  void* done = nullptr;    // hipEvent_t recorded on `stream` after that call's launches
};
int buf_record(DevBuf& b, void* stream);  // hipError_t
// swap the caller's buffer of a cache entry (after waiting for the old one's last user)
void buf_attach(DevBuf& b, void* buf, size_t bytes, const char* what);

// Jumped windows of the last one-seed call, per device.  The ZO step makes three calls
// with the same seed over the same parameters (perturb +eps, perturb -2 eps, restore +
// update), whose plans differ (the perturbation scales) but whose chunk starts -- and
// so the jump-ahead windows -- are the same: the second and third calls skip the jump.
// The windows live in a library-owned buffer, freed by fks_plan_cache_clear.
struct WinCache {
  DevBuf b;
  bool valid = false;
  uint64_t seed = 0, chunk_hash = 0;
};
// Table indices of the last one-seed bf16 perturb, per device (ZO step: the second and
// third calls replay them, fks_small2_kernel ZM 2).  A block's indices depend only on
// the seed and the block's stream position, not on the tensors, so any later one-seed
// call with the same seed and the same bf16 segment ranges (a store covers the blocks of
// its own bf16 segments only) whose regular blocks lie inside the stored range replays them.
// The buffer is the CALLER's (fks_zindex_attach: the Python codec allocates it through
// torch's allocator under a memory budget), 1 byte per parameter; without one attached,
// or with FKS_ZCACHE=0, every call generates.
struct ZCache {
  DevBuf b;
  bool valid = false;
  uint64_t seed = 0, bf16_hash = 0;
  int64_t lo = 0, hi = 0;
};
// The reconstruct window cache (fks_jwin_attach): the jumped windows of the slice
// kernel's two-slice passes, per seed, in a CALLER-owned device buffer of window SETS
// (one seed's windows at the pass's chunk-pair starts: nch x 624 words).  A client
// reconstructs the same (seed, sum) list from model_0 every round (fedkseed.py:57-68:
// the arbiter keeps the K seed candidates; :132-141), so the windows of one round are the
// next round's: a seed found in the cache skips its jump.  Keyed by the plan's chunk
// starts (bs_hash) -- another layout or shard resets it.
struct JWin {
  DevBuf b;
  uint64_t key = 0;  // bs_hash of the plan the sets belong to (0: none)
  int nch = 0;       // chunk pairs per set
  JwSets sets;
};
inline void jw_drop(JWin& J) {  // forget every set (a new key resets the rest)
  J.key = 0;
  J.sets.where.clear();
}
// the entry of the current device (created on first use), or nullptr without an event
ZCache* z_entry();
JWin* jw_entry();
// The cache of the current device, ordered after its last user on `stream`, or nullptr
// when it cannot serve the call (switched off, nothing attached, too small, no memory).
WinCache* win_cache(void* stream, size_t bytes);
ZCache* z_cache(void* stream, size_t bytes);
JWin* jw_cache(void* stream, uint64_t key, int nch);
size_t zindex_bytes(const fks_tensor* t, int nt);
size_t jwin_bytes(const fks_tensor* t, int nt, int k, int shard, int nshards);

// ================================================================== fks_run.cpp
void run(const fks_tensor* t, int nt, const uint64_t* seeds, const double* values, int k, int value_kind, int mode,
         void* workspace, size_t ws_bytes, void* stream, const double* tensor_scales = nullptr, int shard = 0,
         int nshards = 1, uint64_t delta_base = 0, const float* gdev = nullptr);
void profile_begin();
void profile_end(double* apply_ms, int64_t* n_apply, double* jump_ms, int64_t* n_jump);
void delta_apply(const fks_tensor* t, int nt, const float* delta, const double* decay, void* workspace,
                 size_t ws_bytes, void* stream);
void digest(const fks_tensor* t, int nt, uint64_t pos0, uint64_t* dev_out2, void* stream);
void device_selfcheck(int which, uint64_t* result, void* workspace, size_t ws_bytes, void* stream);
// fks_project (vec: its one f32 vector, nvec 1) and fks_project_multi (vec null: vecs[nvec][nt])
size_t project_ws_bytes(const fks_tensor* t, int nt, int nvec, bool multi);
void project(const fks_tensor* t, int nt, const uint64_t* seeds, int k, const float* vec, const fks_vec* vecs,
             int nvec, int shard, int nshards, double* dev_out, void* workspace, size_t ws_bytes, void* stream);
// fks_gram: out[r][c] = <z_rows[r], z_cols[c]> (cols null: the symmetric Gram of rows, kc == kr)
size_t gram_ws_bytes(const fks_tensor* t, int nt);
void gram(const fks_tensor* t, int nt, const uint64_t* rows, int kr, const uint64_t* cols, int kc, int shard,
          int nshards, double* dev_out, void* workspace, size_t ws_bytes, void* stream);
// fks_gram_tiled: fks_gram's matrix in passes of kGtRows x kGtCols seeds on the f64 matrix unit
size_t gram_tiled_ws_bytes(const fks_tensor* t, int nt);
void gram_tiled(const fks_tensor* t, int nt, const uint64_t* rows, int kr, const uint64_t* cols, int kc, int shard,
                int nshards, double* dev_out, void* workspace, size_t ws_bytes, void* stream);
// fks_project_mt: the same projection on the CPU generator's stream (the kModeDelta plan of vec)
void project_mt(const fks_tensor* t, int nt, const uint64_t* seeds, int k, const float* vec, int shard, int nshards,
                double* dev_out, void* workspace, size_t ws_bytes, void* stream);
// fks_project_mt_multi: nvec vectors read in place (vecs[nvec][nt]) over the geometry-only plan
void project_mt_multi(const fks_tensor* t, int nt, const uint64_t* seeds, int k, const fks_vec* vecs, int nvec,
                      int shard, int nshards, double* dev_out, void* workspace, size_t ws_bytes, void* stream);
// fks_gram_mt: fks_gram on the CPU generator's stream, over the geometry-only plan
void gram_mt(const fks_tensor* t, int nt, const uint64_t* rows, int kr, const uint64_t* cols, int kc, int shard,
             int nshards, double* dev_out, void* workspace, size_t ws_bytes, void* stream);
// fks_expand_multi: nvec outputs written in place (outs[nvec][nt]), coefs[nvec][k], betas[nvec] or null
int64_t expand_launch_work();  // kExpLaunchWork, or FKS_EXPAND_WORK where it is set to a positive number
size_t expand_ws_bytes(const fks_tensor* t, int nt, int k, int nvec);
void expand(const fks_tensor* t, int nt, const uint64_t* seeds, const double* coefs, int k, const fks_vec* outs,
            const double* betas, int nvec, int shard, int nshards, void* workspace, size_t ws_bytes, void* stream);
// fks_expand_mt_multi: the same on the CPU generator's stream, over the geometry-only plan
void expand_mt_multi(const fks_tensor* t, int nt, const uint64_t* seeds, const double* coefs, int k, const fks_vec* outs,
                     const double* betas, int nvec, int shard, int nshards, void* workspace, size_t ws_bytes,
                     void* stream);

}  // namespace fks
