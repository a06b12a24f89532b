// The names of a snapshot beside a tree whose leaves stay in file order, and the report of the names that occur more than once
// (mst_names.cuh has the kernels; ss_mst_csv_name_index_dev, ss_mst_find_leaves and ss_mst_duplicate_names_dev in abi_mst.hip
// launch them).  Both work over what the sort of mst_sort.h leaves: name_spans[i], the name at sorted position i, and order[i],
// the file row it stands in.  The sort moves row indices alone, so the index costs the leaves nothing: a tree built in file
// order (mst.rs:74-87, the only order whose root equals a commitment made from the same file) keeps its leaves, and a lookup
// goes position -> order[position].
//
// First match: the sort is stable and mst_find_name is a lower bound, so the position found for a name that occurs k times is
// the head of a run of k equal names in file order, and order[head] is its lowest file row -- the reference's position()
// (mst.rs:207-223).  The k - 1 rows behind the head are *shadowed*: leaves that no lookup, update or proof by name can reach,
// whose balances still sit in the committed sums.  The reference accepts such a file silently (mst.rs:103-134).
//
//   shadowed   sorted position i >= 1 whose name equals the name at i - 1: equal length and equal bytes, every span cut to the
//              body as mst_find_name cuts it
//   repeated   a name that occurs more than once: a shadowed position whose predecessor is not shadowed
//   list       the shadowed leaves in sorted-position order (by name, within a name by file row), the first `cap` of them, and
//              beside each the leaf a lookup of its name finds: the run's head, found by the lower-bound search with the row's
//              own name as the query -- a run is never walked, a file of 2^20 equal names is a legitimate input
//
// Steps, stream order the only barrier between them, no atomic decides where an output goes (the compaction of mst_audit.h):
//   marks     a position per thread: the adjacent compare; a wave's MST_NAMES_TILE positions are a tile: tile_count[tile]; the
//             wave's repeated names by ballot, one atomic add per wave
//   groups    mst_audit_groups_kernel as it stands: MST_NAMES_GROUP tile counts a workgroup, exclusive in place, the total aside
//   scatter   a position per thread: its place = the totals of the groups before + the tile's prefix + its rank in the wave's
//             ballot; the head search for the positions that are listed
// Plain C++ below, so that the rules and the tile and group edges are tested without a GPU (tests/cpp/mst_names_check.cpp runs
// mst_names_host behind mst_csv_host and mst_sort_host).
#pragma once
#include <string>

#include "mst_audit.h"   // the tile and group geometry of the compaction
#include "mst_sort.h"

namespace sg {

static constexpr uint32_t MST_NAMES_THREADS = MST_AUDIT_THREADS;
static constexpr uint32_t MST_NAMES_TILE = MST_AUDIT_TILE;      // positions whose count is one word of the scan: a wave's
static constexpr uint32_t MST_NAMES_GROUP = MST_AUDIT_GROUP;    // tile counts a workgroup of the groups step scans

// the span of sorted position i, cut to the body: whatever the pairs hold, nothing outside the body is read
SG_HD void mst_names_span(const uint32_t* name_spans, uint64_t body_len, uint32_t i, uint64_t* begin, uint64_t* end) {
  uint64_t e = name_spans[2 * (uint64_t)i + 1], b = name_spans[2 * (uint64_t)i];
  if (e > body_len) e = body_len;
  if (b > e) b = e;
  *begin = b;
  *end = e;
}
// equal names: equal length and equal bytes
SG_HD bool mst_names_equal(const uint8_t* body, uint64_t b0, uint64_t e0, uint64_t b1, uint64_t e1) {
  if (e0 - b0 != e1 - b1) return false;
  for (uint64_t k = 0; k < e0 - b0; k++)
    if (body[b0 + k] != body[b1 + k]) return false;
  return true;
}
// is sorted position i (i < n) shadowed?
SG_HD bool mst_names_shadowed(const uint8_t* body, uint64_t body_len, const uint32_t* name_spans, uint32_t i) {
  if (i == 0) return false;
  uint64_t b0, e0, b1, e1;
  mst_names_span(name_spans, body_len, i - 1, &b0, &e0);
  mst_names_span(name_spans, body_len, i, &b1, &e1);
  return mst_names_equal(body, b0, e0, b1, e1);
}
// the head of the run position i stands in: the lower bound of its own name (i itself for a name that is not in order, which
// only spans the sort did not make can hold)
SG_HD uint32_t mst_names_head(const uint8_t* body, uint64_t body_len, const uint32_t* name_spans, uint32_t n, uint32_t i) {
  uint64_t b, e;
  mst_names_span(name_spans, body_len, i, &b, &e);
  const uint32_t head = mst_find_name(body, body_len, name_spans, n, body + b, e - b);
  return head == MST_FIND_ABSENT ? i : head;
}

// The work space in 32-bit words: what the host reads (repeated names, shadowed rows, two spares), the tiles' counts, the groups'
// totals.
static constexpr uint32_t MST_NAMES_AT_REPEATED = 0, MST_NAMES_AT_SHADOWED = 1, MST_NAMES_FRONT_WORDS = 4;
SG_HD uint32_t mst_names_tiles(uint64_t n_rows) { return (uint32_t)((n_rows + MST_NAMES_TILE - 1) / MST_NAMES_TILE); }
SG_HD uint32_t mst_names_groups(uint64_t n_rows) { return (mst_names_tiles(n_rows) + MST_NAMES_GROUP - 1) / MST_NAMES_GROUP; }
SG_HD uint32_t mst_names_at_tiles() { return MST_NAMES_FRONT_WORDS; }
SG_HD uint32_t mst_names_at_groups(uint64_t n_rows) { return mst_names_at_tiles() + mst_names_tiles(n_rows); }
// the size of d_scratch in bytes: 4 * (4 + tiles + groups), tiles = ceil(n_rows / 64), groups = ceil(tiles / 256); n_rows < 2^32
SG_HD uint64_t mst_names_scratch_bytes(uint64_t n_rows) { return 4ull * (mst_names_at_groups(n_rows) + mst_names_groups(n_rows)); }

// What ss_mst_duplicate_names_dev refuses before it touches a device: "" or what is wrong with the call.
inline std::string mst_names_problem(const void* d_bytes, uint64_t len, uint64_t body_off, const void* d_name_spans, const void* d_order,
                                     uint64_t n_rows, const void* d_shadowed, const void* d_first, uint64_t cap, const void* d_scratch,
                                     const void* summary_out) {
  if (!d_bytes || !d_name_spans || !d_scratch || !summary_out) return "null argument";
  if ((!d_shadowed || !d_first) && cap) return "null d_shadowed or d_first with a non-zero cap";
  if (n_rows == 0 || n_rows >= (1ull << 32)) return "n_rows outside 1..2^32-1";
  if (body_off > len || len - body_off >= (1ull << 32)) return "body_off behind len, or a body of 2^32 bytes or more";
  if ((uintptr_t)d_name_spans & 3) return "d_name_spans is not 4-byte aligned";
  if ((uintptr_t)d_order & 3) return "d_order is not 4-byte aligned";
  if ((uintptr_t)d_shadowed & 3) return "d_shadowed is not 4-byte aligned";
  if ((uintptr_t)d_first & 3) return "d_first is not 4-byte aligned";
  if ((uintptr_t)d_scratch & 3) return "d_scratch is not 4-byte aligned";
  return "";
}

// ------------------------------------------------------------------ the steps on the host, one after the other
struct MstNamesHost {
  std::vector<uint32_t> shadowed;       // the first cap shadowed leaves, in sorted-position order
  std::vector<uint32_t> first;          // beside each, the leaf a lookup of its name finds
  uint64_t summary[3] = {0, 0, 0};      // repeated names, shadowed rows, rows listed
};
// name_spans and order as mst_sort_host returns them (order nullptr: leaf i is sorted position i), over the same tiles and groups
inline MstNamesHost mst_names_host(const uint8_t* body, uint64_t body_len, const uint32_t* name_spans, const uint32_t* order, uint64_t n_rows,
                                   uint64_t cap) {
  MstNamesHost r;
  const uint32_t n = (uint32_t)n_rows, tiles = mst_names_tiles(n_rows), groups = mst_names_groups(n_rows);
  std::vector<uint32_t> work(mst_names_scratch_bytes(n_rows) / 4, 0);
  uint32_t *tile_count = work.data() + mst_names_at_tiles(), *group_total = work.data() + mst_names_at_groups(n_rows);
  std::vector<uint8_t> mark(n);
  for (uint32_t i = 0; i < n; i++) {                           // marks
    mark[i] = mst_names_shadowed(body, body_len, name_spans, i);
    tile_count[i / MST_NAMES_TILE] += mark[i];
    if (mark[i] && !mark[i - 1]) work[MST_NAMES_AT_REPEATED]++;
  }
  for (uint32_t g = 0; g < groups; g++) {                      // groups: exclusive in place, the total aside
    uint32_t before = 0;
    for (uint32_t t = g * MST_NAMES_GROUP; t < tiles && t < (g + 1) * MST_NAMES_GROUP; t++) {
      const uint32_t count = tile_count[t];
      tile_count[t] = before;
      before += count;
    }
    group_total[g] = before;
  }
  uint32_t rank = 0;                                           // scatter
  for (uint32_t i = 0; i < n; i++) {
    if (i % MST_NAMES_TILE == 0) rank = 0;
    if (!mark[i]) continue;
    const uint32_t tile = i / MST_NAMES_TILE, group = tile / MST_NAMES_GROUP;
    uint64_t at = (uint64_t)tile_count[tile] + rank++;
    for (uint32_t g = 0; g < group; g++) at += group_total[g];
    if (at >= cap) continue;
    if (r.shadowed.size() <= at) {
      r.shadowed.resize(at + 1, 0xffffffffu);
      r.first.resize(at + 1, 0xffffffffu);
    }
    const uint32_t head = mst_names_head(body, body_len, name_spans, n, i);
    r.shadowed[at] = order ? order[i] : i;
    r.first[at] = order ? order[head] : head;
  }
  for (uint32_t g = 0; g < groups; g++) work[MST_NAMES_AT_SHADOWED] += group_total[g];
  r.summary[0] = work[MST_NAMES_AT_REPEATED];
  r.summary[1] = work[MST_NAMES_AT_SHADOWED];
  r.summary[2] = r.summary[1] < cap ? r.summary[1] : cap;
  return r;
}

#if defined(__HIPCC__)
// the split's name spans (file order, 64-bit) as n_rows x 2 uint32: d_leaf_name_spans[2 r], [2 r + 1] = begin and end of row r's name
hipError_t mst_names_leaf_spans_launch(const uint64_t* d_words, uint64_t n_rows, uint32_t nc, uint32_t* d_leaf_name_spans, hipStream_t stream);
// the three steps on `stream`; d_work: mst_names_scratch_bytes(n_rows), its front zeroed by the caller in stream order
hipError_t mst_names_launch(const uint8_t* d_body, uint64_t body_len, const uint32_t* d_name_spans, const uint32_t* d_order, uint64_t n_rows,
                            uint32_t* d_shadowed, uint32_t* d_first, uint64_t cap, uint32_t* d_work, hipStream_t stream);
#endif

}  // namespace sg
