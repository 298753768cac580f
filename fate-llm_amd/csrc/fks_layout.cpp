// fks_layout.cpp -- the MT19937 stream of a tensor list without HIP (the CU count is an
// argument; tools/plan/plan_selftest.cpp links this file with fks_phx.cpp and fks_gf2.cpp alone):
// validation, layout, shard clipping, chunk plans, the plan cache's header image, workspace sizes.
#include <cmath>

#include "fks_host.h"

namespace fks {

static void check_list(const fks_tensor* t, int nt) {
  if (nt < 0 || (nt > 0 && !t)) throw Error(-FKS_EINVAL, "bad tensor list");
}
static void check_basics(const fks_tensor& x, int i) {
  if (x.numel < 0) throw Error(-FKS_EINVAL, "tensor " + std::to_string(i) + ": negative numel");
  if (x.dtype != FKS_F32 && x.dtype != FKS_BF16 && x.dtype != FKS_F16)
    throw Error(-FKS_EINVAL, "tensor " + std::to_string(i) + ": unsupported dtype code " + std::to_string(x.dtype));
  if (x.numel > 0 && (!x.data || ((uintptr_t)x.data % elem_size(x.dtype)) != 0))
    throw Error(-FKS_EINVAL, "tensor " + std::to_string(i) + ": null or misaligned data pointer");
}

void validate_basics(const fks_tensor* t, int nt) {
  check_list(t, nt);
  for (int i = 0; i < nt; i++) check_basics(t[i], i);
}

void validate(const fks_tensor* t, int nt) {
  check_list(t, nt);
  for (int i = 0; i < nt; i++) {
    const fks_tensor& x = t[i];
    check_basics(x, i);
    if (x.flags & ~(FKS_HAS_WD | FKS_FROZEN | FKS_STREAM_ROCM | FKS_FRESH | FKS_LIBM))
      throw Error(-FKS_EINVAL, "tensor " + std::to_string(i) + ": unknown flags");
    if ((x.flags & (FKS_STREAM_ROCM | FKS_LIBM)) != (t[0].flags & (FKS_STREAM_ROCM | FKS_LIBM)))
      throw Error(-FKS_EINVAL, "tensor " + std::to_string(i) + ": every tensor of a call must use the same z stream");
    if ((x.flags & FKS_STREAM_ROCM) && (x.flags & FKS_LIBM))
      throw Error(-FKS_EINVAL, "tensor " + std::to_string(i) + ": FKS_LIBM is a flavour of the CPU generator's stream");
  }
}

void check_shard(int shard, int nshards) {
  if (nshards < 1 || shard < 0 || shard >= nshards) throw Error(-FKS_EINVAL, "bad shard");
}

// what every descriptor of tensor x carries
template <class D>
static D desc(const fks_tensor& x, float ps, uint32_t flags) {
  D d{};
  d.lr = x.lr;
  d.wd = x.wd;
  d.flags = flags;
  d.dtype = x.dtype;
  d.ps = ps;
  return d;
}

// Consumption per tensor follows normal_kernel (DistributionTemplates.h:231-256):
//   numel >= 16: numel words (+16 fresh words for the tail recompute if numel % 16 != 0)
//   0 < numel < 16: serial normal_distribution<double>: 4 words (two random64) per NEW
//                   Box-Muller pair, the second value of a pair is cached in the
//                   generator and consumed by the next serial draw (DistributionsHelper.h:189-221)
// The fast kernel takes a tensor whose 16-blocks sit on 16-aligned stream words (so
// none straddles an MT block), with no tail recompute, f32/bf16, 2-element aligned
// (it moves adjacent element pairs); everything else goes to the irregular kernel.
Layout make_layout(const fks_tensor* t, int nt, const double* scales, uint64_t delta_base) {
  Layout L;
  L.delta = delta_base != 0;
  int64_t cum = 0;  // concatenated element offset (delta layout)
  bool cached = false;   // CPUGeneratorImpl::next_double_normal_sample
  int64_t cached_pair = 0;
  int64_t pos = 0;
  for (int i = 0; i < nt; i++) {
    const fks_tensor& x = t[i];
    const int64_t n = x.numel;
    const bool live = (x.flags & FKS_FROZEN) == 0;
    const uint64_t ptr = L.delta ? delta_base + 4 * (uint64_t)cum : (uint64_t)(uintptr_t)x.data;
    const size_t es = stor_size(L, x.dtype);
    cum += n;
    // optimizer.py:173: scaling_factor * eps is a python double, cast to the fp32 opmath
    const float ps = scales ? (float)scales[i] : 0.0f;
    if (n >= 16) {
      const bool fast = n % 16 == 0 && pos % 16 == 0 && x.dtype != FKS_F16 && ptr % (2 * es) == 0;
      if (live && fast) {
        DevSeg s = desc<DevSeg>(x, ps, x.flags);
        s.start = pos;
        s.numel = n;
        s.ptr = ptr;
        L.segs[x.dtype].push_back(s);
        L.seg_tensor[x.dtype].push_back(i);
      } else if (live) {
        // words [pos, pos + 16F) hold F = n / 16 whole 16-blocks; if n % 16 != 0 the last
        // 16 elements are redrawn from 16 fresh words [pos + n, pos + n + 16) and the head
        // run must not write them (DistributionTemplates.h:118-124 / :221-228)
        const int64_t F = n / 16;
        DevRun r = desc<DevRun>(x, ps, x.flags);
        r.start = pos;
        r.numel = 16 * F;
        r.ptr = ptr;
        r.limit = n % 16 ? n - 16 : n;
        L.runs.push_back(r);
        L.run_tensor.push_back(i);
        if (n % 16) {
          DevRun tl = r;
          tl.start = pos + n;
          tl.numel = 16;
          tl.ptr = ptr + (uint64_t)(n - 16) * es;
          tl.limit = 16;
          L.runs.push_back(tl);
          L.run_tensor.push_back(i);
        }
      }
      pos += n + (n % 16 ? 16 : 0);
    } else if (n > 0) {
      for (int64_t e = 0; e < n; e++) {
        DevTiny d = desc<DevTiny>(x, ps, x.flags & FKS_HAS_WD);
        if (cached) {
          cached = false;
          d.word = cached_pair;
          d.flags |= kTinySin;
        } else {
          cached = true;
          cached_pair = d.word = pos;
          pos += 4;
        }
        if (!live) continue;
        d.ptr = ptr + (uint64_t)e * es;
        L.tiny.push_back(d);
        L.tiny_tensor.push_back(i);
      }
    }
  }
  L.stream_len = pos;
  L.end_cached = cached;
  L.end_pair = cached_pair;
  // runs are disjoint and already in stream order, and so are the single elements: one takes
  // the word of a pair drawn before it, or a new pair's at the stream's end (the order the
  // kernel walks them in; tools/plan/plan_selftest.cpp checks it)
  return L;
}

BlockRange shard_blocks(int64_t stream_len, int shard, int nshards) {
  const int64_t nb = std::max<int64_t>(1, (stream_len + kMtN - 1) / kMtN);
  return {(int64_t)((__int128)nb * shard / nshards), (int64_t)((__int128)nb * (shard + 1) / nshards)};
}

// one wave of apply workgroups: kApplyWgPerCu per CU for the 19-seed passes, more for
// calls of at most kSmallK seeds (little LDS per workgroup, so more independent streams
// per CU hide the per-block latency chain)
int plan_nchunks(int64_t nblocks, bool small, int cus) {
  const int64_t target = (int64_t)(small ? kSmallWgPerCu : kApplyWgPerCu) * cus;
  return (int)std::max<int64_t>(1, std::min<int64_t>(nblocks, target));
}

// the slice kernel's plan: two chunks per workgroup, one workgroup per CU (a pass of
// > 32 seeds runs two seed slices on each chunk PAIR, a pass of <= 32 one slice per chunk)
int bs_nchunks(int64_t nblocks, int cus) {
  const int64_t wgs = std::max<int64_t>(1, std::min<int64_t>(cus, (nblocks + 1) / 2));
  return (int)(kBsChunksPerWg * wgs);
}

std::vector<int64_t> chunk_table(BlockRange r, int nchunks) {
  const int64_t nblocks = std::max<int64_t>(1, r.hi - r.lo);
  std::vector<int64_t> cb((size_t)nchunks + 1);
  for (int c = 0; c <= nchunks; c++) cb[(size_t)c] = r.lo + (int64_t)((__int128)nblocks * c / nchunks);
  return cb;
}

// keep the entries cut() keeps (it may shorten them), with their tensor indices
template <class D, class F>
static void filter(std::vector<D>& v, std::vector<int>& tensor, F&& cut) {
  size_t n = 0;
  for (size_t j = 0; j < v.size(); j++)
    if (cut(v[j])) {
      v[n] = v[j];
      tensor[n++] = tensor[j];
    }
  v.resize(n);
  tensor.resize(n);
}

// keep only the work whose owner block lies in the range: fast segments are cut at
// block boundaries (16-aligned), a run keeps the 16-blocks whose last word is inside,
// a single element stays where its draw pair ends
void clip_segments(Layout& L, BlockRange r) {
  const int64_t lo = r.lo * kMtN, hi = r.hi * kMtN;
  for (int d = 0; d < 3; d++)
    filter(L.segs[d], L.seg_tensor[d], [&](DevSeg& s) {
      const int64_t a = std::max(s.start, lo), b = std::min(s.start + s.numel, hi);
      if (a >= b) return false;
      s.ptr += (uint64_t)(a - s.start) * stor_size(L, s.dtype);
      s.start = a;
      s.numel = b - a;
      return true;
    });
  filter(L.runs, L.run_tensor, [&](DevRun& R) {
    const int64_t nb = R.numel / 16;
    // 16-block i ends at word R.start + 16 i + 15
    auto first_at_or_after = [&](int64_t w) {
      const int64_t d = w - (R.start + 15);
      return std::min(nb, std::max<int64_t>(0, (d + 15) / 16 * (d > 0)));
    };
    const int64_t i0 = first_at_or_after(lo), i1 = first_at_or_after(hi);
    if (i0 >= i1) return false;
    R.start += 16 * i0;
    R.numel = 16 * (i1 - i0);
    R.ptr += (uint64_t)(16 * i0) * stor_size(L, R.dtype);
    R.limit -= 16 * i0;
    return true;
  });
  filter(L.tiny, L.tiny_tensor, [&](DevTiny& T) { return T.word + 3 >= lo && T.word + 3 < hi; });
}

// Chunks of the irregular kernel: the MT blocks that own irregular work, split into at
// most plan_nchunks() groups of about equal work; a chunk twists through the blocks
// between its first and last owner block.
std::vector<std::pair<int64_t, int64_t>> irregular_owner_intervals(const Layout& L) {
  std::vector<std::pair<int64_t, int64_t>> iv;  // owner block intervals [a, b)
  for (const DevRun& R : L.runs) iv.emplace_back(block_of(R.start + 15), block_of(R.start + R.numel - 1) + 1);
  for (const DevTiny& T : L.tiny) iv.emplace_back(block_of(T.word + 3), block_of(T.word + 3) + 1);
  std::sort(iv.begin(), iv.end());
  std::vector<std::pair<int64_t, int64_t>> merged;
  for (auto& x : iv) {
    if (!merged.empty() && x.first <= merged.back().second) merged.back().second = std::max(merged.back().second, x.second);
    else merged.push_back(x);
  }
  return merged;
}

IrrChunks irregular_chunks(const Layout& L, int cus) {
  const auto merged = irregular_owner_intervals(L);
  if (merged.empty()) return IrrChunks{};
  int64_t covered = 0;
  for (auto& x : merged) covered += x.second - x.first;
  const int cap = plan_nchunks(covered, false, cus);
  const int64_t q = (covered + cap - 1) / cap;  // owner blocks per chunk
  IrrChunks out;
  int64_t in_chunk = 0, chunk_lo = -1, last_hi = -1;
  auto close = [&] {
    out.lo.push_back(chunk_lo);
    out.hi.push_back(last_hi);
    chunk_lo = -1;
    in_chunk = 0;
  };
  for (auto& x : merged) {
    int64_t a = x.first;
    while (a < x.second) {
      if (chunk_lo < 0) chunk_lo = a;
      const int64_t take = std::min(x.second - a, q - in_chunk);
      a += take;
      in_chunk += take;
      last_hi = a;
      if (in_chunk == q) close();
    }
  }
  if (chunk_lo >= 0) close();
  return out;
}

size_t ws_bytes_for(int chunks, int seeds_per_pass) {
  return kWsStatesOff + sizeof(uint32_t) * kMtN * (size_t)seeds_per_pass * (size_t)std::max(chunks, 1);
}

static int nsegs_total(const Layout& L) { return (int)(L.segs[0].size() + L.segs[1].size() + L.segs[2].size()); }

size_t workspace_total(const fks_tensor* t, int nt, int k, uint64_t delta_base, int cus) {
  if (rocm_stream(t, nt)) return kWsStatesOff;  // counter-mode: no generator windows
  // upper bound over every shard count: a shard never needs more chunks than the whole
  // stream; the header itself lives in the plan cache, not in the workspace
  const Layout L = make_layout(t, nt, nullptr, delta_base);
  const bool small = k <= kSmallK;
  int chunks = 0;
  const int64_t nblocks = shard_blocks(L.stream_len, 0, 1).hi;
  if (nsegs_total(L)) chunks = plan_nchunks(nblocks, small, cus);
  int64_t covered = 0;  // owner blocks of the irregular work
  for (auto& x : irregular_owner_intervals(L)) covered += x.second - x.first;
  if (covered) chunks = std::max(chunks, plan_nchunks(covered, false, cus));
  size_t bytes = ws_bytes_for(chunks, std::max(1, std::min(k, small ? kSmallK : kMaxSeedsPerPass)));
  if (!small && k >= kBsMinSeeds && !L.segs[FKS_BF16].empty())  // the slice kernel's windows
    bytes = std::max(bytes, ws_bytes_for(bs_nchunks(nblocks, cus), std::min(k, kBsSeeds)));
  return bytes;
}

// fks_project_mt's workspace: [sink 4 KB | generator windows of one pass | partial rows], the
// rows of a pass's launches -- one per dtype with fast segments, then the irregular one -- one
// after another.  Bounds of what shard `shard`'s plan launches; the whole list's (shard 0 of 1)
// bound every shard's, since each term grows with the blocks a shard holds.
ProjMtWs project_mt_ws(const fks_tensor* t, int nt, int k, int shard, int nshards, int cus) {
  Layout L = make_layout(t, nt, nullptr, 256);  // any 8-byte aligned base gives the same layout
  const BlockRange br = shard_blocks(L.stream_len, shard, nshards);
  clip_segments(L, br);
  ProjMtWs w;
  int reg = 0, ndt = 0;
  for (int d = 0; d < 3; d++) ndt += L.segs[d].empty() ? 0 : 1;
  if (ndt) reg = plan_nchunks(std::max<int64_t>(1, br.hi - br.lo), false, cus);
  int64_t covered = 0;  // owner blocks of the irregular work
  for (auto& x : irregular_owner_intervals(L)) covered += x.second - x.first;
  const int irr = covered ? plan_nchunks(covered, false, cus) : 0;
  w.work = ndt > 0 || irr > 0;
  w.entries = nsegs_total(L) + (int)L.runs.size() + (int)L.tiny.size();
  w.rows = ndt * reg + irr;
  w.partial_off = align_up(ws_bytes_for(std::max(reg, irr), std::max(1, std::min(k, kMaxSeedsPerPass))), 256);
  w.total = w.partial_off + sizeof(double) * (size_t)kPhxSeeds * (size_t)std::max(w.rows, 1);
  return w;
}

// fks_project_mt_multi's workspace: the per-call table of vector pieces in front -- one entry per
// vector and descriptor of the shard's plan (clipping drops or shortens descriptors, it never
// splits one: the whole list's count bounds every shard's) --, then fks_project_mt's layout with
// the partial rows of the vectors of one pass, [row][vector][kPhxSeeds].
ProjMtMultiWs project_mt_multi_ws(const fks_tensor* t, int nt, int k, int nvec, int shard, int nshards, int cus) {
  ProjMtMultiWs w;
  w.one = project_mt_ws(t, nt, k, shard, nshards, cus);
  w.pass_vec = std::max(1, std::min(nvec, kProjMtMaxVec));
  w.inner_off = align_up(sizeof(ProjMtVecEntry) * (size_t)std::max(nvec, 0) * (size_t)w.one.entries, 256);
  w.total = w.inner_off + w.one.partial_off +
            sizeof(double) * (size_t)kPhxSeeds * (size_t)w.pass_vec * (size_t)std::max(w.one.rows, 1);
  return w;
}

// fks_expand_mt_multi's workspace: the per-call table of output pieces in front, as
// fks_project_mt_multi's, then the windows of one pass, the sink, and for k > kMaxSeedsPerPass
// the f32 staging area of one output: 4 bytes per element of the span of the concatenation that
// the shard's clipped layout touches (a run's elements at or past its limit are not touched).
ExpMtWs expand_mt_ws(const fks_tensor* t, int nt, int k, int nvec, int shard, int nshards, int cus) {
  Layout L = make_layout(t, nt, nullptr, kProjMtGeoBase);
  const BlockRange br = shard_blocks(L.stream_len, shard, nshards);
  clip_segments(L, br);
  ExpMtWs w;
  int64_t lo = INT64_MAX, hi = 0;
  auto touch = [&](uint64_t ptr, int64_t n) {  // elements [e, e + n) under a descriptor at ptr
    if (n <= 0) return;
    const int64_t e = (int64_t)((ptr - kProjMtGeoBase) / 4);
    lo = std::min(lo, e);
    hi = std::max(hi, e + n);
  };
  bool reg = false;
  for (int d = 0; d < 3; d++)
    for (const DevSeg& s : L.segs[d]) {
      reg = true;
      touch(s.ptr, s.numel);
    }
  for (const DevRun& R : L.runs) touch(R.ptr, std::min(R.limit, R.numel));
  for (const DevTiny& T : L.tiny) touch(T.ptr, 1);
  if (reg) w.reg_chunks = plan_nchunks(std::max<int64_t>(1, br.hi - br.lo), false, cus);
  int64_t covered = 0;  // owner blocks of the irregular work
  for (auto& x : irregular_owner_intervals(L)) covered += x.second - x.first;
  if (covered) w.irr_chunks = plan_nchunks(covered, false, cus);
  w.work = reg || covered > 0;
  w.entries = nsegs_total(L) + (int)L.runs.size() + (int)L.tiny.size();
  if (lo < hi) {
    w.elem_lo = lo;
    w.elem_hi = hi;
  }
  w.win_off = align_up(sizeof(ProjMtVecEntry) * (size_t)std::max(nvec, 0) * (size_t)w.entries, 256);
  const size_t win = sizeof(uint32_t) * kMtN * (size_t)std::max(0, std::min(k, kMaxSeedsPerPass)) *
                     (size_t)std::max({w.reg_chunks, w.irr_chunks, 1});
  w.sink_off = w.win_off + align_up(win, 256);
  w.stage_off = w.sink_off + kWsStatesOff;
  w.stage_bytes = k > kMaxSeedsPerPass ? sizeof(float) * (size_t)(w.elem_hi - w.elem_lo) : 0;
  w.total = w.stage_off + w.stage_bytes;
  return w;
}

// fks_gram_mt's workspace: the windows of a row tile and of a column tile at the regular chunk
// starts, the same at the irregular chunk starts (the row tile's stay while its column tiles
// pass, so the two chunk tables cannot share one area as they do in fks_project_mt), then one
// pass's partial rows [row][kGramRows][kPhxSeeds].  Sized for a full tile whatever the seed
// counts: nothing depends on them, and nothing has the model's size.
GramMtWs gram_mt_ws(const fks_tensor* t, int nt, int shard, int nshards, int cus) {
  Layout L = make_layout(t, nt, nullptr, kProjMtGeoBase);
  const BlockRange br = shard_blocks(L.stream_len, shard, nshards);
  clip_segments(L, br);
  GramMtWs w;
  int ndt = 0;
  for (int d = 0; d < 3; d++) ndt += L.segs[d].empty() ? 0 : 1;
  if (ndt) w.reg_chunks = plan_nchunks(std::max<int64_t>(1, br.hi - br.lo), false, cus);
  int64_t covered = 0;  // owner blocks of the irregular work
  for (auto& x : irregular_owner_intervals(L)) covered += x.second - x.first;
  if (covered) w.irr_chunks = plan_nchunks(covered, false, cus);
  w.work = ndt > 0 || w.irr_chunks > 0;
  w.rows = ndt * w.reg_chunks + w.irr_chunks;
  const size_t win = sizeof(uint32_t) * kMtN * (size_t)(kGramMtRows + kGramMtCols);
  w.irr_off = align_up(win * (size_t)std::max(w.reg_chunks, 1), 256);
  w.partial_off = w.irr_off + align_up(win * (size_t)std::max(w.irr_chunks, 1), 256);
  w.total = w.partial_off + sizeof(double) * (size_t)kGramRows * (size_t)kPhxSeeds * (size_t)std::max(w.rows, 1);
  return w;
}

uint64_t fnv1a(const std::vector<uint8_t>& b) {
  uint64_t h = 1469598103934665603ull;
  for (uint8_t c : b) h = (h ^ c) * 1099511628211ull;
  return h;
}

// fp32 launches with wd = +-0 keep kModeUpdateWd (the same bits as kModeUpdateWd0, and
// 2.21 vs 2.28 ms per 19-seed launch: profiles/r02n_ab_f32wd0.log)
constexpr bool kWd0F32Mode = false;

PlanImage plan_image(const fks_tensor* t, int nt, const double* scales, uint64_t delta_base, int shard, int nshards,
                     bool small, int cus) {
  Layout L = make_layout(t, nt, scales, delta_base);
  const BlockRange br = shard_blocks(L.stream_len, shard, nshards);
  clip_segments(L, br);
  PlanImage img;
  PlanInfo& C = img.info;
  C.have_reg = nsegs_total(L) > 0;
  C.have_irr = !L.runs.empty() || !L.tiny.empty();
  std::vector<int64_t> cb, bcb;  // the regular and the slice kernel's chunk tables
  if (C.have_reg) cb = chunk_table(br, plan_nchunks(std::max<int64_t>(1, br.hi - br.lo), small, cus));
  C.have_bs = !small && !L.segs[FKS_BF16].empty();
  if (C.have_bs) {
    bcb = chunk_table(br, bs_nchunks(br.hi - br.lo, cus));
    // the slice kernel indexes a chunk's stream words in 32 bits (< 2^31: 3.4 M blocks
    // per plan chunk pair, a 5.6e11-parameter stream at 512 chunks); longer chunks take the 19-seed kernel
    const int n = (int)bcb.size() - 1;
    for (int c = 0; C.have_bs && c < n; c++)
      if ((bcb[(size_t)std::min(c + 2, n)] - bcb[(size_t)c]) * kMtN >= ((int64_t)1 << 31)) C.have_bs = false;
    if (!C.have_bs) bcb.clear();
  }
  const IrrChunks IC = irregular_chunks(L, cus);
  std::vector<uint64_t> polys, ipolys, bpolys;  // one jump polynomial per chunk start
  if (!cb.empty()) jump_polys_for_blocks(std::vector<int64_t>(cb.begin(), cb.end() - 1), polys);
  if (C.have_irr) jump_polys_for_blocks(IC.lo, ipolys);
  if (!bcb.empty()) jump_polys_for_blocks(std::vector<int64_t>(bcb.begin(), bcb.end() - 1), bpolys);
  C.Z.reg_chunks = cb.empty() ? 0 : (int)cb.size() - 1;
  C.Z.irr_chunks = (int)IC.lo.size();
  C.Z.nsegs = nsegs_total(L);
  C.Z.nruns = (int)L.runs.size();
  C.Z.ntiny = (int)L.tiny.size();
  C.Z.bs_chunks = bcb.empty() ? 0 : (int)bcb.size() - 1;
  // the image: every array in a 256-aligned region of its own (at least one), in this order
  auto put = [&](size_t& off, const auto& v) {
    off = img.bytes.size();
    const size_t bytes = sizeof(v[0]) * v.size();
    img.bytes.resize(align_up(off + std::max<size_t>(bytes, 1), 256), 0);
    if (bytes) std::memcpy(img.bytes.data() + off, v.data(), bytes);
  };
  std::vector<DevSeg> segs;  // the three dtypes' segments behind each other
  for (int d = 0; d < 3; d++) {
    C.nsegs[d] = (int)L.segs[d].size();
    C.wd_mode[d] = wd_form(L.segs[d], d != FKS_F32 || kWd0F32Mode);
    segs.insert(segs.end(), L.segs[d].begin(), L.segs[d].end());
  }
  C.bs_wd_pos0 = C.wd_mode[FKS_BF16] == kModeUpdateWd0;
  for (const DevSeg& sg : L.segs[FKS_BF16]) {
    uint32_t wb;
    std::memcpy(&wb, &sg.wd, 4);
    C.bs_wd_pos0 = C.bs_wd_pos0 && wb == 0u && std::isfinite(sg.lr);
    C.bs_max_lr = std::max(C.bs_max_lr, std::fabs(sg.lr));
  }
  put(C.H.off_polys, polys);
  put(C.H.off_cb, cb);
  put(C.H.off_ipolys, ipolys);
  put(C.H.off_ilo, IC.lo);
  put(C.H.off_ihi, IC.hi);
  put(C.H.off_segs, segs);
  put(C.H.off_runs, L.runs);
  put(C.H.off_tiny, L.tiny);
  put(C.H.off_bs_polys, bpolys);
  put(C.H.off_bs_cb, bcb);
  C.H.total = img.bytes.size();
  C.seg_off[0] = C.H.off_segs;
  for (int d = 1; d < 3; d++) C.seg_off[d] = C.seg_off[d - 1] + sizeof(DevSeg) * L.segs[d - 1].size();
  std::vector<uint8_t> ck;
  for (int64_t b : cb) key_put(ck, b);
  key_put(ck, (int64_t)-1);
  for (int64_t b : IC.lo) key_put(ck, b);
  C.chunk_hash = fnv1a(ck);
  std::vector<uint8_t> bk;
  for (const DevSeg& sg : L.segs[FKS_BF16]) {
    key_put(bk, sg.start);
    key_put(bk, sg.numel);
  }
  C.bf16_hash = fnv1a(bk);
  std::vector<uint8_t> sk;
  for (int64_t b : bcb) key_put(sk, b);
  C.bs_hash = bcb.empty() ? 0 : (fnv1a(sk) | 1u);
  if (C.have_reg && !cb.empty()) {
    C.reg_lo = cb.front();
    C.reg_hi = cb.back();
  }
  return img;
}

void mt_census(const fks_tensor* t, int nt, int shard, int nshards, int64_t* word_range, int64_t* written) {
  Layout L = make_layout(t, nt);
  const BlockRange br = shard_blocks(L.stream_len, shard, nshards);
  clip_segments(L, br);
  if (word_range) {
    word_range[0] = br.lo * kMtN;
    word_range[1] = br.hi * kMtN;
  }
  if (!written) return;
  for (int i = 0; i < nt; i++) written[i] = 0;
  for (int d = 0; d < 3; d++)
    for (size_t j = 0; j < L.segs[d].size(); j++) written[L.seg_tensor[d][j]] += L.segs[d][j].numel;
  for (size_t j = 0; j < L.runs.size(); j++)
    written[L.run_tensor[j]] += std::max<int64_t>(0, std::min(L.runs[j].limit, L.runs[j].numel));
  for (size_t j = 0; j < L.tiny.size(); j++) written[L.tiny_tensor[j]] += 1;
}

void cpu_generator_end(const fks_tensor* t, int nt, uint64_t seed, uint32_t* state624, int32_t* left, uint32_t* next,
                       int32_t* normal_valid, double* normal) {
  const Layout L = make_layout(t, nt);
  const int64_t W = L.stream_len;
  // at::mt19937::operator() (MT19937RNGEngine.h): a word first decrements left_ and twists
  // the whole state when it reaches 0 (left_ = 624, next_ = 0), then returns state_[next_++];
  // manual_seed leaves left_ = 1, next_ = 0.  After W >= 1 words the state has been twisted
  // ceil(W / 624) times -- the untempered words x[624 t, 624 t + 624) -- and next_ words of it used.
  const int64_t tw = (W + 623) / 624;
  host_jump_window(seed, tw, state624);
  *next = W ? (uint32_t)(W - 624 * (tw - 1)) : 0u;
  *left = W ? 625 - (int32_t)*next : 1;
  *normal_valid = 0;
  *normal = 0.0;
  if (L.end_cached) {  // normal_distribution<double> (DistributionsHelper.h:189-221): r sin(theta) cached
    uint32_t w[4];
    host_x_words(seed, 624 + L.end_pair, 4, w);  // output word k is temper(x[624 + k])
    for (uint32_t& y : w) {
      y ^= (y >> 11);
      y ^= (y << 7) & 0x9d2c5680u;
      y ^= (y << 15) & 0xefc60000u;
      y ^= (y >> 18);
    }
    // random64() = (first word << 32) | second; uniform_real_distribution<double>: 53 bits
    const uint64_t m53 = (1ull << 53) - 1;
    const double u1 = (double)((((uint64_t)w[0] << 32) | w[1]) & m53) * (1.0 / 9007199254740992.0);
    const double u2 = (double)((((uint64_t)w[2] << 32) | w[3]) & m53) * (1.0 / 9007199254740992.0);
    const double r = std::sqrt(-2.0 * std::log1p(-u2));
    const double theta = 2.0 * 3.14159265358979323846 * u1;
    *normal = r * std::sin(theta);
    *normal_valid = 1;
  }
}

// float -> binary16 -> float, round to nearest even (c10::Half)
static float round_f16(float f) {
  uint32_t x;
  std::memcpy(&x, &f, 4);
  const uint32_t sign = x & 0x80000000u, ax = x & 0x7fffffffu;
  float r;
  if (ax >= 0x477ff000u) {
    x = sign | 0x7f800000u;
  } else if (ax < 0x38800000u) {  // half subnormal: quantum 2^-24
    std::memcpy(&r, &ax, 4);
    r = std::nearbyint(r * 16777216.0f) / 16777216.0f;
    std::memcpy(&x, &r, 4);
    x |= sign;
  } else {
    uint32_t keep = ax & ~0x1fffu;
    const uint32_t rem = ax & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (keep & 0x2000u))) keep += 0x2000u;
    x = sign | keep;
  }
  std::memcpy(&r, &x, 4);
  return r;
}

float round_to_dtype(double v, int dtype) {
  float f = (float)v;
  if (dtype == FKS_F32 || f != f) return f;
  if (dtype == FKS_F16) return round_f16(f);
  uint32_t u;
  std::memcpy(&u, &f, 4);
  u = (u + (((u >> 16) & 1u) + 0x7FFFu)) & 0xFFFF0000u;
  std::memcpy(&f, &u, 4);
  return f;
}

void jw_reset(JwSets& S, uint32_t nsets) {
  S.nsets = nsets;
  S.clock = 0;
  S.where.clear();
  S.set_seed.assign(nsets, 0);
  S.set_used.assign(nsets, 0);
  S.set_pass.assign(nsets, 0);
}

// A missing seed takes the next set in clock order that this pass does not use.
void jw_assign(JwSets& S, const uint64_t* seeds, int nb, uint32_t* slot, uint64_t* miss, uint32_t* miss_slot,
               int& nmiss) {
  const uint64_t pass = ++S.pass;
  nmiss = 0;
  for (int j = 0; j < nb; j++) {
    auto it = S.where.find(seeds[j]);
    if (it != S.where.end()) {
      slot[j] = it->second;
      S.set_pass[it->second] = pass;
      S.hits++;
      continue;
    }
    uint32_t s = S.clock;
    while (S.set_pass[s] == pass) s = (s + 1) % S.nsets;  // nsets >= 64 > nb: terminates
    S.clock = (s + 1) % S.nsets;
    if (S.set_used[s]) S.where.erase(S.set_seed[s]);
    S.set_seed[s] = seeds[j];
    S.set_used[s] = 1;
    S.set_pass[s] = pass;
    S.where[seeds[j]] = s;
    slot[j] = s;
    miss[nmiss] = seeds[j];
    miss_slot[nmiss] = s;
    nmiss++;
    S.misses++;
  }
}

}  // namespace fks
