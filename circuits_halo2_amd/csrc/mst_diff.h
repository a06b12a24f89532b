// The next round's snapshot against a tree in HBM (mst_diff.cuh has the kernels, sr_mst_csv_diff_dev and sr_mst_apply_diff_dev in
// abi_rounds.hip launch them): the join of a new file B with the named leaves of a built tree T by username, where both texts
// lie, the report of who changed, who is new and who is gone, and the changed balances folded for the in-place update.
//
// T has n_tree named leaves and the sorted order of their names: name_spans[i], the name at sorted position i, and order[i], the
// leaf it stands in (nullptr: leaf i is sorted position i, a sorted tree) -- what mst_sort.h and mst_names.h leave.  B is n_rows
// rows of nc balances, split where its text lies (mst_csv.h).
//
// Lookup of a name in T is mst_find_name: the head of the name's run in the sorted order, its first leaf (mst.rs:207-223).
//   row r    row_leaf[r] = the lookup of its name, or MST_DIFF_ABSENT; a name of more than 64 bytes, or the empty name where T has
//            none, is simply not found.  owner[leaf] = the LOWEST row that found the leaf (an atomic minimum: the value, not the
//            arrival, decides).  Row states: NEW (not found), SHADOWED_ROW (a lower row of B found the same leaf: the first row in
//            file order wins), CHANGED / SAME (the owner row; some / none of its nc balances differ from the leaf's)
//   leaf i   of all 2^depth: PADDING (no name, i >= n_tree), SAME / CHANGED (owned by a row), GONE (a run's head that no row found),
//            UNREACHABLE (a shadowed leaf of T: no lookup reaches it, so no row can own it; it is neither changed nor gone)
// Balances compare AS FIELD ELEMENTS: the row's decimal text folded as mst_decimal_words folds it against the eight Montgomery
// words of the leaf's balance.  So 007 equals 7, and an integer >= r equals its residue.
//
// Lists, each in increasing order with places from prefix sums over the data, never from the order in which workgroups finish
// (the compaction of mst_audit.h: a ballot per wave of MST_DIFF_TILE items, a scan per workgroup over MST_DIFF_GROUP tile counts,
// the groups' totals): the CHANGED leaves, all of them (at most min(n_rows, 2^depth)); the NEW rows and the GONE leaves, the first
// `cap` of each.
//
// Steps, stream order the only barrier between them:
//   match     a row per thread: the lookup through B's span into T's text, row_leaf, the minimum into owner
//   judge     a row per thread: its state; the owner folds its balances and sets its leaf SAME or CHANGED; counts by ballot
//   tree      a sorted position per thread: UNREACHABLE by the adjacent compare (mst_names_shadowed), GONE for an unowned head
//   marks, groups, scatter   three times over a state array: CHANGED and GONE over the leaves, NEW over the rows
// Apply: pack, a thread per changed leaf and currency, folds the owner row's balance text once more into j x nc field elements,
// which go through the listed leaf kernel and the listed level kernels as sg_mst_update_dev drives them.  The plan of the levels
// is made on the HOST (mst_update_plan.h) from the list of changed leaves, 4 bytes a changed leaf; the balances never leave HBM.
// Plain C++ below, so that the rules and the tile and group edges are tested without a GPU (tests/cpp/mst_diff_check.cpp runs
// mst_diff_host behind mst_csv_host and mst_sort_host).
#pragma once
#include <string>

#include "mst_entries.h"   // mst_decimal_words
#include "mst_names.h"     // mst_names_shadowed, the tile and group geometry

namespace sg {

static constexpr uint32_t MST_DIFF_THREADS = MST_AUDIT_THREADS;
static constexpr uint32_t MST_DIFF_TILE = MST_AUDIT_TILE;       // items whose count is one word of the scan: a wave's
static constexpr uint32_t MST_DIFF_GROUP = MST_AUDIT_GROUP;     // tile counts a workgroup of the groups step scans
static constexpr uint32_t MST_DIFF_ABSENT = MST_FIND_ABSENT;
enum : uint8_t { MST_DIFF_LEAF_PADDING = 0, MST_DIFF_LEAF_SAME = 1, MST_DIFF_LEAF_CHANGED = 2, MST_DIFF_LEAF_GONE = 3, MST_DIFF_LEAF_UNREACHABLE = 4 };
enum : uint8_t { MST_DIFF_ROW_SAME = 1, MST_DIFF_ROW_CHANGED = 2, MST_DIFF_ROW_NEW = 3, MST_DIFF_ROW_SHADOWED = 4 };
// the summary the host gets: the four row states, the gone and the unreachable leaves, the new rows and the gone leaves listed
enum : uint32_t {
  MST_DIFF_SUM_NEW = 0, MST_DIFF_SUM_SHADOWED = 1, MST_DIFF_SUM_CHANGED = 2, MST_DIFF_SUM_SAME = 3, MST_DIFF_SUM_GONE = 4,
  MST_DIFF_SUM_UNREACHABLE = 5, MST_DIFF_SUM_NEW_LISTED = 6, MST_DIFF_SUM_GONE_LISTED = 7, MST_DIFF_SUMMARY_WORDS = 8
};

// The work space in 32-bit words: the six counts the host reads (as the summary's first six, two spares), then tile counts and
// group totals of the three compactions: CHANGED and GONE over the 2^depth leaves, NEW over the n_rows rows.
static constexpr uint32_t MST_DIFF_FRONT_WORDS = 8;
SG_HD uint32_t mst_diff_tiles(uint64_t items) { return (uint32_t)((items + MST_DIFF_TILE - 1) / MST_DIFF_TILE); }
SG_HD uint32_t mst_diff_groups(uint64_t items) { return (mst_diff_tiles(items) + MST_DIFF_GROUP - 1) / MST_DIFF_GROUP; }
SG_HD uint32_t mst_diff_list_words(uint64_t items) { return mst_diff_tiles(items) + mst_diff_groups(items); }
SG_HD uint32_t mst_diff_at_changed() { return MST_DIFF_FRONT_WORDS; }
SG_HD uint32_t mst_diff_at_gone(uint32_t depth) { return mst_diff_at_changed() + mst_diff_list_words((uint64_t)1 << depth); }
SG_HD uint32_t mst_diff_at_new(uint32_t depth) { return mst_diff_at_gone(depth) + mst_diff_list_words((uint64_t)1 << depth); }
// the size of d_scratch in bytes: 4 * (8 + 2 * (leaf tiles + leaf groups) + row tiles + row groups), tiles = ceil(items / 64),
// groups = ceil(tiles / 256); n_rows < 2^32, depth <= 30
SG_HD uint64_t mst_diff_scratch_bytes(uint64_t n_rows, uint32_t depth) { return 4ull * (mst_diff_at_new(depth) + mst_diff_list_words(n_rows)); }

// the name of row r of B from the split's 64-bit spans, cut to the body: whatever the spans hold, nothing outside the body is read
SG_HD void mst_diff_span(const uint64_t* begin, const uint64_t* end, uint64_t at, uint64_t body_len, uint64_t* b, uint64_t* e) {
  uint64_t hi = end[at], lo = begin[at];
  if (hi > body_len) hi = body_len;
  if (lo > hi) lo = hi;
  *b = lo;
  *e = hi;
}
// the leaf a lookup of q finds in T, or MST_DIFF_ABSENT; a leaf outside the tree (only an order the sort did not make holds one)
// is no leaf
SG_HD uint32_t mst_diff_lookup(const uint8_t* body_t, uint64_t body_t_len, const uint32_t* name_spans, const uint32_t* order, uint32_t n_tree,
                               uint32_t depth, const uint8_t* q, uint64_t q_len) {
  const uint32_t at = mst_find_name(body_t, body_t_len, name_spans, n_tree, q, q_len);
  if (at == MST_FIND_ABSENT) return MST_DIFF_ABSENT;
  const uint32_t leaf = order ? order[at] : at;
  return leaf < ((uint32_t)1 << depth) ? leaf : MST_DIFF_ABSENT;
}
// does the decimal text body[b .. e) stand for the field element whose Montgomery words are `leaf`?
SG_HD bool mst_diff_balance_equal(const uint8_t* body, uint64_t b, uint64_t e, const uint32_t* leaf) {
  uint32_t w[8];
  mst_decimal_words(body + b, (size_t)(e - b), w);
  uint32_t differ = 0;
#pragma unroll
  for (uint32_t k = 0; k < 8; k++) differ |= w[k] ^ leaf[k];
  return differ == 0;
}

// What sr_mst_csv_diff_dev refuses before it touches a device: "" or what is wrong with the call.  b_*: the new file, t_*: the tree's.
struct MstDiffArgs {
  const void *b_bytes, *b_tiles, *b_spans, *t_bytes, *t_name_spans, *t_order, *leaf_balances;
  const void *row_leaf, *row_state, *leaf_state, *owner, *changed, *new_rows, *gone, *scratch, *problem_out, *summary_out;
  uint64_t b_len, b_body_off, n_rows, t_len, t_body_off, n_tree, cap;
  uint32_t delimiter, nc, depth;
};
inline std::string mst_diff_problem(const MstDiffArgs& a) {
  if (!a.b_bytes || !a.b_tiles || !a.b_spans || !a.t_bytes || !a.t_name_spans || !a.leaf_balances || !a.row_leaf || !a.row_state ||
      !a.leaf_state || !a.owner || !a.changed || !a.scratch || !a.problem_out || !a.summary_out)
    return "null argument";
  if ((!a.new_rows || !a.gone) && a.cap) return "null d_new_rows or d_gone with a non-zero cap";
  if (a.nc == 0 || a.nc > 64) return "n_currencies outside 1..64";
  if (a.depth > MST_AUDIT_MAX_DEPTH) return "depth above 30";
  const uint32_t d = a.delimiter;
  if (d >= 256 || d == '\n' || d == '\r' || (d >= '0' && d <= '9') || mst_csv_forbidden((uint8_t)d)) return "a delimiter the reader does not take";
  if (a.b_body_off >= a.b_len || a.b_len - a.b_body_off >= (1ull << 32)) return "the file's body_off at or behind len, or a body of 2^32 bytes or more";
  if (a.n_rows == 0 || a.n_rows > a.b_len - a.b_body_off) return "n_rows outside 1..the body's bytes";
  if (a.t_body_off > a.t_len || a.t_len - a.t_body_off >= (1ull << 32)) return "the tree's body_off behind len, or a body of 2^32 bytes or more";
  if (a.n_tree == 0 || a.n_tree > ((uint64_t)1 << a.depth)) return "n_tree outside 1..2^depth";
  if ((uintptr_t)a.b_tiles & 3) return "d_tile_scratch is not 4-byte aligned";
  if ((uintptr_t)a.b_spans & 7) return "d_span_scratch is not 8-byte aligned";
  if ((uintptr_t)a.t_name_spans & 3) return "d_name_spans is not 4-byte aligned";
  if ((uintptr_t)a.t_order & 3) return "d_order is not 4-byte aligned";
  if ((uintptr_t)a.leaf_balances & 15) return "d_leaf_balances is not 16-byte aligned";
  if ((uintptr_t)a.row_leaf & 3) return "d_row_leaf is not 4-byte aligned";
  if ((uintptr_t)a.owner & 3) return "d_owner is not 4-byte aligned";
  if ((uintptr_t)a.changed & 3) return "d_changed is not 4-byte aligned";
  if ((uintptr_t)a.new_rows & 3) return "d_new_rows is not 4-byte aligned";
  if ((uintptr_t)a.gone & 3) return "d_gone is not 4-byte aligned";
  if ((uintptr_t)a.scratch & 3) return "d_scratch is not 4-byte aligned";
  return "";
}
// What sr_mst_apply_diff_dev refuses before it touches a device (the overlap of the two balance arrays is the entry point's own)
inline std::string mst_diff_apply_problem(const void* b_bytes, uint64_t b_len, uint64_t b_body_off, const void* b_spans, uint64_t n_rows,
                                          const void* owner, const void* changed, uint64_t n_changed, uint32_t depth, uint32_t nc,
                                          const void* usernames, const void* leaf_balances, const void* node_hashes, const void* node_balances) {
  if (!b_bytes || !b_spans || !owner || !changed || !usernames || !leaf_balances || !node_hashes || !node_balances) return "null argument";
  if (nc == 0 || nc > 64) return "n_currencies outside 1..64";
  if (depth > MST_AUDIT_MAX_DEPTH) return "depth above 30";
  if (b_body_off >= b_len || b_len - b_body_off >= (1ull << 32)) return "the file's body_off at or behind len, or a body of 2^32 bytes or more";
  if (n_rows == 0 || n_rows > b_len - b_body_off) return "n_rows outside 1..the body's bytes";
  if (n_changed > n_rows || n_changed > ((uint64_t)1 << depth)) return "more changed leaves than rows or leaves";
  if ((uintptr_t)b_spans & 7) return "d_span_scratch is not 8-byte aligned";
  if ((uintptr_t)owner & 3) return "d_owner is not 4-byte aligned";
  if ((uintptr_t)changed & 3) return "d_changed is not 4-byte aligned";
  if (((uintptr_t)usernames | (uintptr_t)leaf_balances | (uintptr_t)node_hashes | (uintptr_t)node_balances) & 15)
    return "a tree array is not 16-byte aligned";
  return "";
}

// ------------------------------------------------------------------ the steps on the host, one after the other
struct MstDiffHost {
  std::vector<uint32_t> row_leaf, owner;                  // n_rows; 2^depth
  std::vector<uint8_t> row_state, leaf_state;             // n_rows; 2^depth
  std::vector<uint32_t> changed, new_rows, gone;          // all changed leaves; the first cap new rows and gone leaves
  std::vector<uint32_t> packed;                           // the apply's field elements: changed x nc x 8 Montgomery words
  uint64_t summary[MST_DIFF_SUMMARY_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
};
// The ordered compaction of the items whose state is `code`, over the same tiles and groups as the kernels: the first `cap` of
// them into `out` (entries between listed ones never stay unwritten: places are dense); returns how many there are.
inline uint64_t mst_diff_compact_host(const std::vector<uint8_t>& state, uint8_t code, uint64_t cap, std::vector<uint32_t>* out) {
  const uint64_t n = state.size();
  const uint32_t tiles = mst_diff_tiles(n), groups = mst_diff_groups(n);
  std::vector<uint32_t> tile_count(tiles, 0), group_total(groups, 0);
  for (uint64_t i = 0; i < n; i++) tile_count[i / MST_DIFF_TILE] += state[i] == code;          // marks
  for (uint32_t g = 0; g < groups; g++) {                                                      // groups: exclusive in place
    uint32_t before = 0;
    for (uint32_t t = g * MST_DIFF_GROUP; t < tiles && t < (g + 1) * MST_DIFF_GROUP; t++) {
      const uint32_t count = tile_count[t];
      tile_count[t] = before;
      before += count;
    }
    group_total[g] = before;
  }
  uint32_t rank = 0;                                                                           // scatter
  for (uint64_t i = 0; i < n; i++) {
    if (i % MST_DIFF_TILE == 0) rank = 0;
    if (state[i] != code) continue;
    const uint32_t tile = (uint32_t)(i / MST_DIFF_TILE), group = tile / MST_DIFF_GROUP;
    uint64_t at = (uint64_t)tile_count[tile] + rank++;
    for (uint32_t g = 0; g < group; g++) at += group_total[g];
    if (at >= cap) continue;
    if (out->size() <= at) out->resize(at + 1, 0xffffffffu);
    (*out)[at] = (uint32_t)i;
  }
  uint64_t all = 0;
  for (uint32_t g = 0; g < groups; g++) all += group_total[g];
  return all;
}
// words_b: B's row starts and spans as mst_csv_host leaves them (no problem); name_spans and order as mst_sort_host returns them for
// T (order nullptr: a sorted tree); leaf_bal: 2^depth x nc x 8 Montgomery words, the tree's leaf balances
inline MstDiffHost mst_diff_host(const uint8_t* body_b, uint64_t body_b_len, const uint64_t* words_b, uint64_t n_rows, uint32_t nc,
                                 const uint8_t* body_t, uint64_t body_t_len, const uint32_t* name_spans, const uint32_t* order, uint64_t n_tree,
                                 uint32_t depth, const uint32_t* leaf_bal, uint64_t cap) {
  MstDiffHost r;
  const uint32_t n = (uint32_t)n_rows, nt = (uint32_t)n_tree, leaves = (uint32_t)1 << depth;
  const MstCsvSpans s = mst_csv_spans(const_cast<uint64_t*>(words_b), n_rows, nc);
  r.row_leaf.assign(n, MST_DIFF_ABSENT);
  r.owner.assign(leaves, MST_DIFF_ABSENT);
  r.row_state.assign(n, 0);
  r.leaf_state.assign(leaves, MST_DIFF_LEAF_PADDING);
  for (uint32_t row = 0; row < n; row++) {                     // match
    uint64_t b, e;
    mst_diff_span(s.name_begin, s.name_end, row, body_b_len, &b, &e);
    const uint32_t leaf = mst_diff_lookup(body_t, body_t_len, name_spans, order, nt, depth, body_b + b, e - b);
    r.row_leaf[row] = leaf;
    if (leaf != MST_DIFF_ABSENT && row < r.owner[leaf]) r.owner[leaf] = row;
  }
  auto differs = [&](uint32_t row, uint32_t leaf) {
    for (uint32_t c = 0; c < nc; c++) {
      uint64_t b, e;
      mst_diff_span(s.bal_begin, s.bal_end, (uint64_t)row * nc + c, body_b_len, &b, &e);
      if (!mst_diff_balance_equal(body_b, b, e, leaf_bal + 8 * ((size_t)leaf * nc + c))) return true;
    }
    return false;
  };
  for (uint32_t row = 0; row < n; row++) {                     // judge
    const uint32_t leaf = r.row_leaf[row];
    uint8_t state = MST_DIFF_ROW_NEW;
    if (leaf != MST_DIFF_ABSENT) {
      state = MST_DIFF_ROW_SHADOWED;
      if (r.owner[leaf] == row) {
        state = differs(row, leaf) ? MST_DIFF_ROW_CHANGED : MST_DIFF_ROW_SAME;
        r.leaf_state[leaf] = state == MST_DIFF_ROW_CHANGED ? MST_DIFF_LEAF_CHANGED : MST_DIFF_LEAF_SAME;
      }
    }
    r.row_state[row] = state;
    const uint32_t at = state == MST_DIFF_ROW_NEW ? 0u : state == MST_DIFF_ROW_SHADOWED ? 1u : state == MST_DIFF_ROW_CHANGED ? 2u : 3u;
    r.summary[MST_DIFF_SUM_NEW + at]++;                        // the summary's first four, in this order
  }
  for (uint32_t i = 0; i < nt; i++) {                          // tree
    const uint32_t leaf = order ? order[i] : i;
    if (leaf >= leaves) continue;
    if (mst_names_shadowed(body_t, body_t_len, name_spans, i)) {
      r.leaf_state[leaf] = MST_DIFF_LEAF_UNREACHABLE;
      r.summary[MST_DIFF_SUM_UNREACHABLE]++;
    } else if (r.owner[leaf] == MST_DIFF_ABSENT) {
      r.leaf_state[leaf] = MST_DIFF_LEAF_GONE;
      r.summary[MST_DIFF_SUM_GONE]++;
    }
  }
  mst_diff_compact_host(r.leaf_state, MST_DIFF_LEAF_CHANGED, ~0ull, &r.changed);
  const uint64_t gone = mst_diff_compact_host(r.leaf_state, MST_DIFF_LEAF_GONE, cap, &r.gone);
  const uint64_t fresh = mst_diff_compact_host(r.row_state, MST_DIFF_ROW_NEW, cap, &r.new_rows);
  r.summary[MST_DIFF_SUM_NEW_LISTED] = fresh < cap ? fresh : cap;
  r.summary[MST_DIFF_SUM_GONE_LISTED] = gone < cap ? gone : cap;
  for (uint32_t leaf : r.changed)                              // pack
    for (uint32_t c = 0; c < nc; c++) {
      uint64_t b, e;
      mst_diff_span(s.bal_begin, s.bal_end, (uint64_t)r.owner[leaf] * nc + c, body_b_len, &b, &e);
      uint32_t w[8];
      mst_decimal_words(body_b + b, (size_t)(e - b), w);
      r.packed.insert(r.packed.end(), w, w + 8);
    }
  return r;
}

#if defined(__HIPCC__)
// the steps of the diff on `stream`; d_words: B's spans as mst_csv_split_launch left them without a problem; d_work:
// mst_diff_scratch_bytes(n_rows, depth).  Zeroes the front, the leaf states and fills the owners itself, in stream order.
hipError_t mst_diff_launch(const uint8_t* d_body_b, uint64_t body_b_len, const uint64_t* d_words, uint64_t n_rows, uint32_t nc,
                           const uint8_t* d_body_t, uint64_t body_t_len, const uint32_t* d_name_spans, const uint32_t* d_order, uint64_t n_tree,
                           uint32_t depth, const void* d_leaf_balances, uint32_t* d_row_leaf, uint8_t* d_row_state, uint8_t* d_leaf_state,
                           uint32_t* d_owner, uint32_t* d_changed, uint32_t* d_new_rows, uint32_t* d_gone, uint64_t cap, uint32_t* d_work,
                           hipStream_t stream);
// pack: d_packed[j * nc + c] = balance c of row d_owner[d_changed[j]] of B, j < n_changed; a list entry or an owner outside its
// range packs zeros
hipError_t mst_diff_pack_launch(const uint8_t* d_body_b, uint64_t body_b_len, const uint64_t* d_words, uint64_t n_rows, uint32_t nc,
                                const uint32_t* d_owner, const uint32_t* d_changed, uint64_t n_changed, uint32_t depth, void* d_packed,
                                hipStream_t stream);
#endif

}  // namespace sg
