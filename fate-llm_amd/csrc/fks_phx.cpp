// fks_phx.cpp -- host geometry of the torch_rocm stream (FKS_STREAM_ROCM) without HIP (the grid
// cap is an argument): a call's tensor table, torch's launch policy, element shards, their census.
#include <cmath>

#include "fks_host.h"

namespace fks {

// torch's TensorIteratorBase::can_use_32bit_indexing for a contiguous 1-D draw of m elements of
// es bytes: numel and the largest byte offset + 1 both within INT32_MAX
bool phx_fits32(int64_t m, size_t es) {
  return m <= (int64_t)INT32_MAX && 1 + (m - 1) * (int64_t)es <= (int64_t)INT32_MAX;
}
// calc_execution_policy (DistributionTemplates.h:50-62) for m elements: (stride, loop iterations)
void phx_policy(int64_t m, int64_t max_grid, int64_t& stride, int64_t& J) {
  const uint32_t grid0 = (uint32_t)(((uint64_t)m + 255u) / 256u);  // dim3 grid((numel + 255) / 256)
  const int64_t grid = std::min<int64_t>(grid0, max_grid);
  stride = 256 * grid;
  J = (m - 1) / (4 * stride) + 1;  // counter_offset / 4
}

// The table and geometry alone (nothing cached, nothing uploaded): what fks_shard_census
// reads; get_phx_plan adds the device copy.
PhxGeo phx_geometry(const fks_tensor* t, int nt, const double* scales, uint64_t delta_base, int64_t max_grid) {
  PhxGeo P;
  uint64_t off4 = 0;
  int64_t items = 0, elems = 0;
  for (int i = 0; i < nt; i++) {
    const int64_t n = t[i].numel;
    elems += n;
    if (n == 0) continue;  // torch draws nothing for an empty tensor (the offset stays)
    const size_t es = elem_size(t[i].dtype);
    const bool live = !(t[i].flags & FKS_FROZEN);
    const uint64_t base = delta_base ? delta_base + 4 * (uint64_t)(elems - n) : (uint64_t)(uintptr_t)t[i].data;
    const size_t ses = delta_base ? 4 : es;  // bytes per stored element
    // distribution_nullary_kernel (DistributionTemplates.h:111-133) first reserves the
    // offset increment of the whole tensor; when the iterator cannot use 32-bit indexing it
    // then draws each piece TensorIterator::with_32bit_indexing yields -- halves split until
    // they fit, first floor(m / 2) elements then the rest, in order -- as a call of its own,
    // which reserves that piece's increment.  A piece is a table entry of its own (its
    // elements, stride and offset).
    auto emit = [&](int64_t start, int64_t m) {
      int64_t stride = 0, J = 0;
      phx_policy(m, max_grid, stride, J);
      const uint64_t my_off4 = off4;
      off4 += (uint64_t)J;
      if (!live) return;
      PhxTensor x{};
      x.ptr = base + (uint64_t)start * ses;
      x.numel = m;
      x.item0 = items;
      x.off4 = my_off4;
      x.stride = (uint32_t)stride;
      x.dtype = t[i].dtype;
      x.lr = t[i].lr;
      x.wd = t[i].wd;
      const bool fresh16 = ((uint64_t)start * es) % 16u == 0;
      // the alignment of the p the call's first wd * p reads in the reference: this buffer's,
      // or (FKS_FRESH) that of the tensor an earlier reference step rebound param.data to
      const bool wd16 = (t[i].flags & FKS_FRESH) ? fresh16 : (x.ptr % 16u) == 0;
      x.flags = (t[i].flags & FKS_HAS_WD) | ((x.ptr % 16u) == 0 ? kPhxP16 : 0u) | (fresh16 ? kPhxFresh16 : 0u) |
                (wd16 ? kPhxWdP16 : 0u);
      x.ps = scales ? (float)scales[i] : 0.0f;
      P.tab.push_back(x);
      P.elem0.push_back(elems - n + start);
      P.tensor_of.push_back(i);
      items += stride * J;
    };
    auto pieces = [&](auto&& self, int64_t start, int64_t m) -> void {
      if (phx_fits32(m, es)) {
        emit(start, m);
        return;
      }
      const int64_t h = m / 2;
      self(self, start, h);
      self(self, start + h, m - h);
    };
    if (phx_fits32(n, es)) {
      emit(0, n);
    } else {
      int64_t stride = 0, J = 0;
      phx_policy(n, max_grid, stride, J);
      off4 += (uint64_t)J;  // the whole tensor's reservation, before the pieces' own
      pieces(pieces, 0, n);
    }
  }
  P.off4_total = off4;
  P.nt = (int)P.tab.size();
  P.items = items;
  P.elems = elems;
  P.wd_mode = wd_form(P.tab);  // the launch-wide weight-decay form of a reconstruct (as PlanInfo::wd_mode)
  bool pos0 = P.wd_mode == kModeUpdateWd0;
  for (const PhxTensor& x : P.tab) {
    uint32_t wb;
    std::memcpy(&wb, &x.wd, 4);
    pos0 = pos0 && wb == 0u && x.dtype != FKS_F16 && std::isfinite(x.lr);
    P.max_lr = std::max(P.max_lr, std::fabs(x.lr));
  }
  P.wd_pos0 = pos0;
  return P;
}

// Element shards of the torch_rocm stream.  Work item r of a tensor is (idx, j) =
// (r % S, r / S) and covers elements idx + S (4 j + i), i < 4: a ROW of S items (one j)
// covers the 4 S consecutive elements [4 j S, 4 (j + 1) S).  Shard boundaries are the
// equal item splits rounded to the nearest row start, so every shard updates whole rows:
// one contiguous run of elements of the call's tensors laid end to end (fks_shard_census).
static int phx_entry(const PhxGeo& P, int64_t b) {  // the last entry whose first item is <= b
  int lo = 0, hi = P.nt - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (P.tab[mid].item0 <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}
int64_t phx_boundary(const PhxGeo& P, int shard, int nshards) {  // (0 for every shard of an empty table)
  const int64_t b = (int64_t)((__int128)P.items * shard / nshards);
  if (b <= 0 || b >= P.items) return std::max<int64_t>(0, std::min(b, P.items));
  const PhxTensor& T = P.tab[phx_entry(P, b)];
  const int64_t S = T.stride, rows = (T.numel - 1) / (4 * S) + 1;
  const int64_t j = std::min(rows, (b - T.item0 + S / 2) / S);
  return T.item0 + j * S;
}
// the first element (in the concatenation of all the call's tensors) of item boundary b
int64_t phx_boundary_elem(const PhxGeo& P, int64_t b) {
  if (b >= P.items) return P.elems;
  const int k = phx_entry(P, b);
  const PhxTensor& T = P.tab[k];
  return P.elem0[k] + std::min<int64_t>(T.numel, 4 * ((b - T.item0) / T.stride) * (int64_t)T.stride);
}

// Launch cuts of fks_expand_multi, whose one launch would otherwise carry every seed of the call
// over the whole shard: the items [lo, hi) (row boundaries, phx_boundary) as b[0] = lo < b[1] < ...
// < b[n] = hi, every b a row boundary, a launch [b[i], b[i + 1]) holding at most `work`
// seed-elements -- 4 elements per item (a row's ragged end counts whole) times max(k, 1) seeds --
// or else exactly one row.  Greedy: each launch takes as many whole rows as fit.  Empty for lo >= hi.
std::vector<int64_t> phx_expand_cuts(const PhxGeo& P, int64_t lo, int64_t hi, int k, int64_t work) {
  std::vector<int64_t> b;
  if (lo >= hi || P.nt == 0) return b;
  const int64_t per_item = 4 * (int64_t)std::max(k, 1);
  const int64_t budget = std::max<int64_t>(1, work / per_item);  // items per launch
  b.push_back(lo);
  for (int64_t cur = lo; cur < hi;) {
    int64_t next = hi;
    if (hi - cur > budget) {
      const PhxTensor& T = P.tab[phx_entry(P, cur + budget)];  // cur + budget < hi <= P.items: inside T
      const int64_t S = T.stride;
      next = T.item0 + (cur + budget - T.item0) / S * S;  // the last row boundary within the budget
      if (next <= cur) {  // one row is past the budget: that row alone
        const PhxTensor& C = P.tab[phx_entry(P, cur)];
        next = C.item0 + ((cur - C.item0) / C.stride + 1) * (int64_t)C.stride;
      }
      next = std::min(next, hi);
    }
    b.push_back(next);
    cur = next;
  }
  return b;
}

// Passes of fks_gram: tiles of at most kGramRows rows by at most kPhxSeeds columns, row tiles
// outermost.  A rectangular call tiles its krows x kcols cells, every cell once.  A symmetric one
// (kcols == krows) starts the columns of the row tile [r0, r0 + nr) at r0: its first pass is the
// DIAGONAL tile, the only one that holds cells below the diagonal (c < r, both inside [r0, r0 + nr):
// computed twice, with the same bits); every later pass of the row tile lies at c >= r0 + kPhxSeeds,
// above every row.  So each pair c >= r is computed once and the reduce mirrors it.
static std::vector<GramPass> gram_tile_passes(int krows, int kcols, bool symmetric, int tile_rows, int tile_cols) {
  std::vector<GramPass> p;
  for (int r0 = 0; r0 < krows; r0 += tile_rows) {
    const int nr = std::min(tile_rows, krows - r0);
    for (int c0 = symmetric ? r0 : 0; c0 < kcols; c0 += tile_cols)
      p.push_back(GramPass{r0, nr, c0, std::min(tile_cols, kcols - c0)});
  }
  return p;
}

std::vector<GramPass> gram_passes(int krows, int kcols, bool symmetric) {
  return gram_tile_passes(krows, kcols, symmetric, kGramRows, kPhxSeeds);
}

// fks_gram_mt's passes: the same tiling by kGramMtRows x kGramMtCols (columns >= rows, so the
// diagonal tile still holds every cell below the diagonal of its row tile)
std::vector<GramPass> gram_mt_passes(int krows, int kcols, bool symmetric) {
  return gram_tile_passes(krows, kcols, symmetric, kGramMtRows, kGramMtCols);
}

// fks_gram_tiled's passes: the same tiling by its tile of kGtRows x kGtCols seeds (fks_gram_tiled.h;
// columns >= rows)
std::vector<GramPass> gram_tiled_passes(int krows, int kcols, bool symmetric) {
  return gram_tile_passes(krows, kcols, symmetric, kGtRows, kGtCols);
}

// element runs of whole Philox rows (phx_boundary)
void phx_census(const PhxGeo& P, int nt, int shard, int nshards, int64_t* word_range, int64_t* written) {
  const int64_t lo = phx_boundary(P, shard, nshards), hi = phx_boundary(P, shard + 1, nshards);
  if (word_range) {
    word_range[0] = phx_boundary_elem(P, lo);
    word_range[1] = phx_boundary_elem(P, hi);
  }
  if (!written) return;
  for (int i = 0; i < nt; i++) written[i] = 0;
  for (int k = 0; k < P.nt; k++) {  // table entries: the pieces of the non-empty, non-frozen tensors
    const PhxTensor& T = P.tab[k];
    const int64_t a0 = std::max(lo, T.item0), a1 = std::min(hi, T.item0 + T.stride * ((T.numel - 1) / (4 * (int64_t)T.stride) + 1));
    if (a1 > a0)
      written[P.tensor_of[k]] += std::min<int64_t>(T.numel, 4 * ((a1 - T.item0) / T.stride) * (int64_t)T.stride) -
                                  std::min<int64_t>(T.numel, 4 * ((a0 - T.item0) / T.stride) * (int64_t)T.stride);
  }
}

}  // namespace fks
