// Host self-test of the planning code of libfks.so (fate-llm_amd/csrc/fks_layout.cpp and
// fks_phx.cpp, linked with fks_gf2.cpp alone: no HIP): invariants of the MT stream layout,
// the shard clipping, the chunk plans, the header image, the torch_rocm geometry and the
// window-set bookkeeping, over hand-written and LCG-drawn tensor lists.  Meant to be built
// with sanitizers (tests/test_plan_host.py):
//   g++ -O1 -g -std=c++17 -mpclmul -msse4.1 -fsanitize=address,undefined -fno-sanitize-recover=undefined
//     -I include -I fate-llm_amd/csrc tools/plan/plan_selftest.cpp fate-llm_amd/csrc/fks_layout.cpp
//     fate-llm_amd/csrc/fks_phx.cpp fate-llm_amd/csrc/fks_gf2.cpp -o /tmp/plan_selftest && /tmp/plan_selftest
#include <cstdio>
#include <cstdlib>
#include <map>

#include "fks_host.h"

using namespace fks;

static int g_fails = 0;
static long g_checks = 0;
static std::string g_ctx;
#define CHECK(c)                                                                     \
  do {                                                                               \
    g_checks++;                                                                      \
    if (!(c)) {                                                                      \
      printf("FAIL line %d: %s  [%s]\n", __LINE__, #c, g_ctx.c_str());               \
      if (++g_fails >= 20) exit(1);                                                  \
    }                                                                                \
  } while (0)

struct T {
  int64_t n;
  int32_t dtype;
  uint32_t flags;
  uint64_t addr;
};
using List = std::vector<T>;

static std::vector<fks_tensor> tensors(const List& l, uint32_t extra_flags = 0) {
  std::vector<fks_tensor> t(l.size());
  for (size_t i = 0; i < l.size(); i++)
    t[i] = fks_tensor{l[i].n ? (void*)(uintptr_t)l[i].addr : nullptr, l[i].n, l[i].dtype, l[i].flags | extra_flags, 0.0f, 0.0f};
  return t;
}

// the lists of tests/test_capi_host.py (stream length, generator end, torch_rocm pieces)
static std::vector<List> hand_lists() {
  std::vector<List> out;
  for (std::vector<int64_t> s : {std::vector<int64_t>{16, 32, 624}, {37, 5, 3, 16}, {5, 3, 1, 7, 100}, {1, 1, 1, 15, 17}}) {
    List l;
    for (int64_t n : s) l.push_back({n, FKS_BF16, 0, 16});
    out.push_back(l);
  }
  using P = std::pair<int64_t, int>;
  for (std::vector<P> s : {std::vector<P>{{3, 0}, {20, 0}}, {{5, 1}, {7, 2}, {1000, 1}, {1, 0}}, {{4096, 0}, {5, 0}}, {{16, 1}},
                           {{100000, 0}, {3, 1}, {17, 2}}, {{0, 0}}, {{624 * 3, 1}}, {{30000005, 0}, {2, 1}}}) {
    List l;
    for (P x : s) l.push_back({x.first, x.second, 0, 16});
    out.push_back(l);
  }
  for (std::vector<P> s : {std::vector<P>{{600000000, 0}}, {{1100000003, 0}, {5, 1}}, {{(1ll << 30) + 4099, 2}, {1ll << 29, 0}}}) {
    List l;
    for (P x : s) l.push_back({x.first, x.second, 0, 4096});
    out.push_back(l);
  }
  return out;
}

// 200 lists from a fixed LCG (tests/test_plan_host.py lcg_lists draws the same)
static uint64_t g_lcg = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(uint64_t n) {
  g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull;
  return (g_lcg >> 33) % n;
}
static std::vector<List> lcg_lists(int count) {
  std::vector<List> out;
  for (int i = 0; i < count; i++) {
    List l;
    const int nt = 1 + (int)rnd(12);
    for (int j = 0; j < nt; j++) {
      int64_t n = 0;
      const int c = (int)rnd(8);
      if (c == 1) n = 1 + (int64_t)rnd(15);
      else if (c == 2) n = 16;
      else if (c == 3) n = 17 + (int64_t)rnd(24);
      else if (c == 4) n = 624 * (1 + (int64_t)rnd(6));
      else if (c == 5) {
        n = 624 * (1 + (int64_t)rnd(6));
        n += rnd(2) ? 3 : -3;
      } else if (c >= 6) n = c == 6 ? 4096 : 100003;
      const int d = (int)rnd(3);
      const uint32_t flags = rnd(6) == 0 ? FKS_FROZEN : 0;
      const uint64_t addr = 4096 + (d == 0 ? 4 : 2) * rnd(64);
      l.push_back({n, d, flags, addr});
    }
    out.push_back(l);
  }
  return out;
}

static uint32_t crc32(uint32_t c, const void* p, size_t n) {
  c = ~c;
  for (size_t i = 0; i < n; i++) {
    c ^= ((const uint8_t*)p)[i];
    for (int b = 0; b < 8; b++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  }
  return ~c;
}

template <class V>
static bool nondecreasing(const V& v) {
  for (size_t i = 1; i < v.size(); i++)
    if (v[i] < v[i - 1]) return false;
  return true;
}

// ---- the MT stream ----
static void check_chunk_table(BlockRange br, int n) {
  const std::vector<int64_t> cb = chunk_table(br, n);
  CHECK(n >= 1 && (int)cb.size() == n + 1);
  CHECK(cb.front() == br.lo && cb.back() == br.hi && nondecreasing(cb));
}

static void check_image(const std::vector<fks_tensor>& t, int shard, int nshards, bool small, int cus) {
  const int nt = (int)t.size();
  const PlanImage img = plan_image(t.data(), nt, nullptr, 0, shard, nshards, small, cus);
  const PlanInfo& C = img.info;
  Layout L = make_layout(t.data(), nt);
  const BlockRange br = shard_blocks(L.stream_len, shard, nshards);
  clip_segments(L, br);
  const size_t off[] = {C.H.off_polys, C.H.off_cb, C.H.off_ipolys, C.H.off_ilo, C.H.off_ihi,
                        C.H.off_segs,  C.H.off_runs, C.H.off_tiny,  C.H.off_bs_polys, C.H.off_bs_cb, C.H.total};
  const size_t bytes[] = {8u * 312 * C.Z.reg_chunks, 8u * (C.Z.reg_chunks + 1), 8u * 312 * C.Z.irr_chunks, 8u * C.Z.irr_chunks,
                          8u * C.Z.irr_chunks, sizeof(DevSeg) * C.Z.nsegs, sizeof(DevRun) * C.Z.nruns,
                          sizeof(DevTiny) * C.Z.ntiny, 8u * 312 * C.Z.bs_chunks, 8u * (C.Z.bs_chunks + 1)};
  CHECK(off[0] == 0 && img.bytes.size() == C.H.total);
  for (int i = 0; i < 10; i++) CHECK(off[i] % 256 == 0 && off[i] + bytes[i] <= off[i + 1]);  // aligned, disjoint
  CHECK(C.H.total % 256 == 0);
  CHECK(C.Z.nsegs == (int)(L.segs[0].size() + L.segs[1].size() + L.segs[2].size()));
  CHECK(C.Z.nruns == (int)L.runs.size() && C.Z.ntiny == (int)L.tiny.size());
  CHECK(C.have_reg == (C.Z.nsegs > 0) && C.have_irr == (C.Z.nruns + C.Z.ntiny > 0));
  CHECK(C.have_bs == (!small && !L.segs[FKS_BF16].empty()));  // (no chunk pair here reaches 2^31 words)
  CHECK((C.bs_hash != 0) == C.have_bs && (C.Z.bs_chunks > 0) == C.have_bs);
  size_t so = C.H.off_segs;
  for (int d = 0; d < 3; d++) {
    CHECK(C.seg_off[d] == so && C.nsegs[d] == (int)L.segs[d].size());
    if (!L.segs[d].empty()) {
      CHECK(std::memcmp(img.bytes.data() + so, L.segs[d].data(), sizeof(DevSeg) * L.segs[d].size()) == 0);
      CHECK(C.wd_mode[d] == kModeUpdateNoWd);  // the lists carry no weight-decay term
    } else {
      CHECK(C.wd_mode[d] == kModeUpdate);
    }
    so += sizeof(DevSeg) * L.segs[d].size();
  }
  if (C.have_reg) {
    const std::vector<int64_t> cb = chunk_table(br, plan_nchunks(br.hi - br.lo, small, cus));
    CHECK((int)cb.size() == C.Z.reg_chunks + 1 && C.reg_lo == br.lo && C.reg_hi == br.hi);
    CHECK(std::memcmp(img.bytes.data() + C.H.off_cb, cb.data(), 8 * cb.size()) == 0);
  }
  if (C.have_bs) {
    const std::vector<int64_t> cb = chunk_table(br, bs_nchunks(br.hi - br.lo, cus));
    CHECK((int)cb.size() == C.Z.bs_chunks + 1);
    CHECK(std::memcmp(img.bytes.data() + C.H.off_bs_cb, cb.data(), 8 * cb.size()) == 0);
  }
  const IrrChunks IC = irregular_chunks(L, cus);
  CHECK((int)IC.lo.size() == C.Z.irr_chunks);
  if (C.Z.irr_chunks) {
    CHECK(std::memcmp(img.bytes.data() + C.H.off_ilo, IC.lo.data(), 8 * IC.lo.size()) == 0);
    CHECK(std::memcmp(img.bytes.data() + C.H.off_ihi, IC.hi.data(), 8 * IC.hi.size()) == 0);
  }
}

static void check_mt(const List& l, int cus, int nshards, bool with_image) {
  const std::vector<fks_tensor> t = tensors(l);
  const int nt = (int)t.size();
  validate(t.data(), nt);
  const Layout L0 = make_layout(t.data(), nt);
  {  // the single elements come out in stream order (make_layout relies on it)
    std::vector<int64_t> w;
    for (const DevTiny& d : L0.tiny) w.push_back(d.word);
    CHECK(nondecreasing(w));
  }
  const int64_t nblocks = std::max<int64_t>(1, (L0.stream_len + kMtN - 1) / kMtN);
  std::vector<int64_t> written(l.size(), 0);
  int64_t next_lo = 0;
  for (int shard = 0; shard < nshards; shard++) {
    const BlockRange br = shard_blocks(L0.stream_len, shard, nshards);
    CHECK(br.lo == next_lo && br.hi >= br.lo);  // the shards tile the blocks
    next_lo = br.hi;
    Layout L = make_layout(t.data(), nt);
    clip_segments(L, br);
    int nsegs = 0;
    for (int d = 0; d < 3; d++)
      for (size_t j = 0; j < L.segs[d].size(); j++) {
        const DevSeg& s = L.segs[d][j];
        nsegs++;
        written[L.seg_tensor[d][j]] += s.numel;
        CHECK(s.numel > 0 && s.start % 16 == 0 && s.numel % 16 == 0);
        CHECK(s.start >= br.lo * kMtN && s.start + s.numel <= br.hi * kMtN);
        CHECK(s.ptr % (2 * elem_size(s.dtype)) == 0);
      }
    for (size_t j = 0; j < L.runs.size(); j++)
      written[L.run_tensor[j]] += std::max<int64_t>(0, std::min(L.runs[j].limit, L.runs[j].numel));
    for (size_t j = 0; j < L.tiny.size(); j++) written[L.tiny_tensor[j]] += 1;
    if (nsegs) {  // (a shard with segments owns at least one block)
      for (int small = 0; small < 2; small++) check_chunk_table(br, plan_nchunks(br.hi - br.lo, small != 0, cus));
      check_chunk_table(br, bs_nchunks(br.hi - br.lo, cus));
    }
    // the irregular chunks: at most plan_nchunks(covered), ascending, non-empty, and every owner block in one
    const IrrChunks IC = irregular_chunks(L, cus);
    int64_t covered = 0;
    for (auto& x : irregular_owner_intervals(L)) covered += x.second - x.first;
    CHECK(IC.lo.size() == IC.hi.size());
    CHECK(covered ? (int64_t)IC.lo.size() <= plan_nchunks(covered, false, cus) && !IC.lo.empty() : IC.lo.empty());
    for (size_t c = 0; c < IC.lo.size(); c++) {
      CHECK(IC.lo[c] < IC.hi[c]);
      if (c) CHECK(IC.hi[c - 1] <= IC.lo[c]);
    }
    auto in_one_chunk = [&](int64_t b) {  // (the chunks are ascending and disjoint: at most one holds b)
      const size_t c = (size_t)(std::upper_bound(IC.lo.begin(), IC.lo.end(), b) - IC.lo.begin());
      return c > 0 && b < IC.hi[c - 1];
    };
    for (const DevRun& R : L.runs) {
      // every MT block from the one its first 16-block ends in to the one its last ends in is an
      // owner block (16-blocks end every 16 words); past 4,096 blocks a stride of them is checked
      const int64_t a = block_of(R.start + 15), b = block_of(R.start + R.numel - 1);
      const int64_t step = std::max<int64_t>(1, (b - a) / 4096);
      for (int64_t x = a; x <= b; x += step) CHECK(in_one_chunk(x));
      CHECK(in_one_chunk(b));
      CHECK(a >= br.lo && b < br.hi);
    }
    for (const DevTiny& d : L.tiny) CHECK(in_one_chunk(block_of(d.word + 3)) && block_of(d.word + 3) >= br.lo);
    if (with_image)
      for (int small = 0; small < 2; small++) check_image(t, shard, nshards, small != 0, cus);
  }
  CHECK(next_lo == nblocks);
  for (size_t i = 0; i < l.size(); i++) CHECK(written[i] == ((l[i].flags & FKS_FROZEN) ? 0 : l[i].n));
}

// ---- the torch_rocm stream ----
static int64_t policy_J(int64_t m, int64_t max_grid) {
  int64_t stride = 0, J = 0;
  phx_policy(m, max_grid, stride, J);
  return J;
}
// the offset / 4 a tensor of n elements reserves: its own draw, plus (when it is split) every piece's
static uint64_t pieces_off4(int64_t m, size_t es, int64_t max_grid) {
  if (phx_fits32(m, es)) return (uint64_t)policy_J(m, max_grid);
  return pieces_off4(m / 2, es, max_grid) + pieces_off4(m - m / 2, es, max_grid);
}
static uint64_t tensor_off4(int64_t n, size_t es, int64_t max_grid) {
  return phx_fits32(n, es) ? (uint64_t)policy_J(n, max_grid) : (uint64_t)policy_J(n, max_grid) + pieces_off4(n, es, max_grid);
}

static void check_phx(const List& l, int cus) {
  const std::vector<fks_tensor> t = tensors(l, FKS_STREAM_ROCM);
  const int nt = (int)t.size();
  validate(t.data(), nt);
  const int64_t max_grid = (int64_t)cus * (2048 / 256);
  const PhxGeo P = phx_geometry(t.data(), nt, nullptr, 0, max_grid);
  CHECK(P.nt == (int)P.tab.size() && P.tab.size() == P.elem0.size() && P.tab.size() == P.tensor_of.size());
  // the pieces tile each live tensor in order; off4 and item0 advance as torch's launches do
  int e = 0;
  int64_t start = 0, items = 0;
  uint64_t off4 = 0;
  for (int i = 0; i < nt; i++) {
    const int64_t n = l[(size_t)i].n;
    const size_t es = elem_size(l[(size_t)i].dtype);
    if (n > 0 && !(l[(size_t)i].flags & FKS_FROZEN)) {
      const bool split = !phx_fits32(n, es);
      uint64_t o = off4 + (split ? (uint64_t)policy_J(n, max_grid) : 0);  // the whole tensor's reservation first
      int64_t done = 0;
      while (done < n) {
        CHECK(e < P.nt && P.tensor_of[(size_t)e] == i);
        if (e >= P.nt) return;
        const PhxTensor& x = P.tab[(size_t)e];
        int64_t stride = 0, J = 0;
        phx_policy(x.numel, max_grid, stride, J);
        CHECK(x.numel > 0 && phx_fits32(x.numel, es) && P.elem0[(size_t)e] == start + done);
        CHECK(x.ptr == l[(size_t)i].addr + (uint64_t)done * es && x.stride == (uint32_t)stride);
        CHECK(x.off4 == o && x.item0 == items);
        o += (uint64_t)J;
        items += stride * J;
        done += x.numel;
        e++;
      }
      CHECK(done == n);
      CHECK(o == off4 + tensor_off4(n, es, max_grid));
    }
    if (n > 0) off4 += tensor_off4(n, es, max_grid);
    start += n;
  }
  CHECK(e == P.nt && items == P.items && start == P.elems && off4 == P.off4_total);
  if (P.nt == 0) return;
  for (int nshards : {1, 2, 3, 8, 13}) {
    std::vector<int64_t> written(l.size(), 0), we(l.size(), 0);
    int64_t prev = 0, prev_elem = 0;
    for (int r = 0; r <= nshards; r++) {
      const int64_t b = phx_boundary(P, r, nshards);
      CHECK(b >= prev && (r > 0 || b == 0) && (r < nshards || b == P.items));
      bool row_start = b == P.items;
      for (const PhxTensor& x : P.tab)
        row_start = row_start || (b >= x.item0 && (b - x.item0) % x.stride == 0 &&
                                  b <= x.item0 + (int64_t)x.stride * policy_J(x.numel, max_grid));
      CHECK(row_start);
      const int64_t el = phx_boundary_elem(P, b);
      CHECK(el >= prev_elem && el <= P.elems && (b < P.items || el == P.elems));
      prev = b;
      prev_elem = el;
      if (r < nshards) {
        int64_t range[2];
        phx_census(P, nt, r, nshards, range, we.data());
        CHECK(range[0] == el && range[1] >= range[0]);
        for (size_t i = 0; i < l.size(); i++) written[i] += we[i];
      }
    }
    for (size_t i = 0; i < l.size(); i++) CHECK(written[i] == ((l[i].flags & FKS_FROZEN) ? 0 : l[i].n));
  }
}

// ---- the window sets of the reconstruct window cache ----
static void check_jw(uint32_t nsets) {
  JwSets S;
  jw_reset(S, nsets);
  uint64_t pool[150];
  for (uint64_t& s : pool) s = (rnd(1u << 30) << 20) ^ rnd(1u << 30);
  for (int pass = 0; pass < 60; pass++) {
    uint64_t seeds[64], miss[64];
    uint32_t slot[64], miss_slot[64];
    int nmiss = 0;
    for (uint64_t& s : seeds) s = pool[rnd(150)];
    for (int j = 1; j < 64; j += 9) seeds[j] = seeds[j - 1];  // repeats within the pass for certain
    const auto before = S.where;
    const uint64_t counted = S.hits + S.misses;
    jw_assign(S, seeds, 64, slot, miss, miss_slot, nmiss);
    CHECK(S.hits + S.misses == counted + 64 && nmiss >= 0 && nmiss <= 64);
    std::map<uint32_t, uint64_t> seed_of;
    std::map<uint64_t, uint32_t> set_of, missed;
    for (int m = 0; m < nmiss; m++) {
      CHECK(!missed.count(miss[m]));
      missed[miss[m]] = miss_slot[m];
    }
    for (int j = 0; j < 64; j++) {
      CHECK(slot[j] < nsets);
      if (seed_of.count(slot[j])) CHECK(seed_of[slot[j]] == seeds[j]);  // no two distinct seeds share a set
      if (set_of.count(seeds[j])) CHECK(set_of[seeds[j]] == slot[j]);   // a repeated seed gets the same set
      seed_of[slot[j]] = seeds[j];
      set_of[seeds[j]] = slot[j];
      if (missed.count(seeds[j])) CHECK(missed[seeds[j]] == slot[j]);
      else CHECK(before.count(seeds[j]) && before.at(seeds[j]) == slot[j]);  // a hit returns the set it was given
    }
    size_t used = 0;  // where and set_seed stay inverse to each other
    for (uint32_t s = 0; s < nsets; s++)
      if (S.set_used[s]) {
        used++;
        CHECK(S.where.count(S.set_seed[s]) && S.where.at(S.set_seed[s]) == s);
      }
    CHECK(used == S.where.size());
    for (auto& kv : S.where) CHECK(kv.second < nsets && S.set_used[kv.second] && S.set_seed[kv.second] == kv.first);
  }
}

int main() {
  const std::vector<List> hand = hand_lists(), lcg = lcg_lists(200);
  uint32_t crc = 0;
  for (const List& l : lcg)
    for (const T& x : l) {
      uint8_t rec[24];
      std::memcpy(rec, &x.n, 8);
      std::memcpy(rec + 8, &x.dtype, 4);
      std::memcpy(rec + 12, &x.flags, 4);
      std::memcpy(rec + 16, &x.addr, 8);
      crc = crc32(crc, rec, 24);
    }
  printf("lcg lists crc %08x\n", crc);
  for (int g = 0; g < 2; g++) {
    const std::vector<List>& lists = g ? lcg : hand;
    for (size_t i = 0; i < lists.size(); i++)
      for (int cus : {1, 256, 304}) {
        for (int nshards : {1, 2, 3, 8, 13}) {
          g_ctx = std::string(g ? "lcg " : "hand ") + std::to_string(i) + " cus " + std::to_string(cus) + " nshards " +
                  std::to_string(nshards);
          // the header image (it holds one jump polynomial per chunk) for the lists of few blocks
          const bool small_list = g ? i < 24 : i < 11;
          check_mt(lists[i], cus, nshards, small_list && nshards <= 3 && cus != 304);
        }
        g_ctx = std::string(g ? "lcg " : "hand ") + std::to_string(i) + " torch_rocm, cus " + std::to_string(cus);
        check_phx(lists[i], cus);
      }
  }
  for (uint32_t nsets : {64u, 65u, 200u}) {
    g_ctx = "jw_assign, nsets " + std::to_string(nsets);
    check_jw(nsets);
  }
  if (g_fails) return 1;
  printf("plan_selftest ok (%ld checks)\n", g_checks);
  return 0;
}
