// A round settled in full on a tree in HBM (mst_admit.cuh has the kernels, sa_mst_admit_measure_dev and sa_mst_settle_dev in
// abi_admit.hip launch them): behind the diff of mst_diff.h the NEW rows of the next round's file B become leaves in the tree's
// padding, the name index grows by them, the GONE leaves' balances become zero, and the CHANGED, GONE and admitted leaves go
// through ONE run of the listed leaf kernel and the listed level kernels.
//
// The rules:
//   zero     every listed GONE leaf gets nc zero balances.  Its username, its place and its entry in the name index stay: a lookup
//            still finds it, the export writes it as name,0,0 and a later diff of the same file still calls it GONE.  UNREACHABLE
//            leaves are not touched.  The liabilities leave the committed sums; the row stays until a rebuild drops it.
//   admit    the j-th NEW row of B in file order becomes leaf n_tree + j: username = the row's name hashed as Entry::new hashes
//            it, balances = the row's, folded where the text lies.  A name twice among the NEW rows gets two leaves, the later one
//            shadowed (mst_names.h).  Whatever the padding leaf held is overwritten.  Only a tree in FILE order with a name index
//            admits: a sorted tree's leaves are its order.
//   text     the tree's text afterwards is the old text followed by the admitted names, one after the other in leaf order, no
//            separator: names are only ever read through spans.  Old spans keep their values.
//   index    the sorted order over all n_tree + n_new named leaves is the stable order by the names' bytes, equal names in leaf
//            order: bit for bit what mst_sort_host makes of a file that holds those names in leaf order.
// Refused, with nothing written: n_tree + n_new > 2^depth (the depth has to grow: the rebuild that really is due); a NEW row with
// a name of more than MST_SORT_NAME_CAP bytes (the sort's report: lowest row, code MST_SORT_NAME_TOO_LONG); a tree body that would
// reach 2^32 bytes with the names appended; lists the diff's cap left incomplete.
//
// Steps, stream order the only barrier between them; no atomic or finishing order decides a position:
//   lengths   mst_sort_lengths_launch over all rows of B: the over-long name and the longest
//   measure   a NEW row per thread, in leaf order: its name's length; a wave's sum is a tile, mst_audit_groups_kernel scans
//             MST_ADMIT_GROUP tile sums, offsets gives every name its place behind the old text and the host the total; the rank
//             j of row new_rows[j] goes into row_rank
//     -- the one copy and wait of the measure call: the total, the problem word, the longest name --
//   sort      mst_sort_launch over all rows of B
//   list      marks, groups, scatter over the sorted positions whose row is NEW: the sorted NEW list, ordered by name and within
//             a name by file row, because the sort is stable
//   merge     the k-th sorted NEW name goes to merged position k + (old sorted names below it), a lower bound over the tree's
//             spans; old sorted position i goes to i + (sorted NEW names below its name), a lower bound over the sorted NEW list.
//             A NEW name is absent from the tree, so there are no ties across the lists and the mapping is a bijection
//   names     an admitted leaf per thread: its name copied behind the old text, its leaf span, its username
//   pack      a leaf of the union of CHANGED, GONE and admitted leaves (increasing) and a currency per thread: the owner row's
//             text, zero, or the leaf's own row's text, folded
//   leaves, levels   witness.leaves and witness.level over the union; the plan of the levels is the host's (mst_update_plan.h)
// Plain C++ below, so that the rules and the tile and group edges are tested without a GPU (tests/cpp/mst_admit_check.cpp runs
// mst_admit_host behind mst_csv_host, mst_sort_host and mst_diff_host).
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "mst_diff.h"

namespace sg {

static constexpr uint32_t MST_ADMIT_THREADS = MST_AUDIT_THREADS;
static constexpr uint32_t MST_ADMIT_TILE = MST_AUDIT_TILE;      // items whose count or sum is one word of the scan: a wave's
static constexpr uint32_t MST_ADMIT_GROUP = MST_AUDIT_GROUP;    // tile words a workgroup of the groups step scans
static constexpr uint32_t MST_ADMIT_NAME_CAP = MST_SORT_NAME_CAP;

// The work space in 32-bit words, every part on a 16-byte boundary: what the host reads of the measure (the names' bytes, low and
// high word; two spares), DIRECTLY behind it the sort's work space, whose front holds the problem word and the longest name -- one
// copy of MST_ADMIT_RESULT_WORDS words brings all three --, the sorted order of B and its names' spans, the rank of every NEW row,
// the sorted NEW list, the admitted names' places, tiles and groups of the list's compaction and of the text's scan, and the
// sort's second block of spans (64-bit words).
static constexpr uint32_t MST_ADMIT_AT_TOTAL = 0, MST_ADMIT_FRONT_WORDS = 4, MST_ADMIT_RESULT_WORDS = MST_ADMIT_FRONT_WORDS + 4;
SG_HD uint64_t mst_admit_round4(uint64_t words) { return (words + 3) & ~3ull; }
SG_HD uint64_t mst_admit_at_sort() { return MST_ADMIT_FRONT_WORDS; }
SG_HD uint64_t mst_admit_at_order(uint64_t n_rows) { return mst_admit_at_sort() + mst_admit_round4(mst_sort_work_words(n_rows)); }
SG_HD uint64_t mst_admit_at_spans(uint64_t n_rows) { return mst_admit_at_order(n_rows) + mst_admit_round4(n_rows); }
SG_HD uint64_t mst_admit_at_rank(uint64_t n_rows) { return mst_admit_at_spans(n_rows) + mst_admit_round4(2 * n_rows); }
SG_HD uint64_t mst_admit_at_list(uint64_t n_rows) { return mst_admit_at_rank(n_rows) + mst_admit_round4(n_rows); }
SG_HD uint64_t mst_admit_at_places(uint64_t n_rows, uint64_t n_new) { return mst_admit_at_list(n_rows) + mst_admit_round4(n_new); }
SG_HD uint64_t mst_admit_at_list_scan(uint64_t n_rows, uint64_t n_new) { return mst_admit_at_places(n_rows, n_new) + mst_admit_round4(n_new); }
SG_HD uint64_t mst_admit_at_text_scan(uint64_t n_rows, uint64_t n_new) {
  return mst_admit_at_list_scan(n_rows, n_new) + mst_admit_round4(mst_diff_list_words(n_rows));
}
SG_HD uint64_t mst_admit_at_sorted_words(uint64_t n_rows, uint64_t n_new) {
  return mst_admit_at_text_scan(n_rows, n_new) + mst_admit_round4(mst_diff_list_words(n_new));
}
// the size of d_scratch in bytes; n_rows < 2^32, n_new <= n_rows
SG_HD uint64_t mst_admit_scratch_bytes(uint64_t n_rows, uint32_t nc, uint64_t n_new) {
  return 4 * mst_admit_at_sorted_words(n_rows, n_new) + 8 * mst_csv_span_words(n_rows, nc);
}

// how many of the n sorted names of a tree lie below the query: the loop of mst_find_name, every span cut to the body
SG_HD uint32_t mst_admit_tree_below(const uint8_t* body, uint64_t body_len, const uint32_t* name_spans, uint32_t n, const uint8_t* q,
                                    uint64_t q_len) {
  uint32_t first = 0, last = n;
  while (first < last) {
    const uint32_t mid = first + (last - first) / 2;
    uint64_t b, e;
    mst_names_span(name_spans, body_len, mid, &b, &e);
    if (mst_sort_compare(body, b, e, q, q_len) < 0) first = mid + 1; else last = mid;
  }
  return first;
}
// the name of row `row` of B cut to the body and to the cap; a row outside the file has the empty name at 0
SG_HD void mst_admit_row_name(const uint64_t* name_begin, const uint64_t* name_end, uint64_t n_rows, uint64_t row, uint64_t body_len,
                              uint64_t* b, uint64_t* e) {
  *b = *e = 0;
  if (row >= n_rows) return;
  mst_diff_span(name_begin, name_end, row, body_len, b, e);
  if (*e - *b > MST_ADMIT_NAME_CAP) *e = *b + MST_ADMIT_NAME_CAP;
}
// how many of the m names of the sorted NEW list (rows of B, through B's spans) lie below the query
SG_HD uint32_t mst_admit_list_below(const uint8_t* body_b, uint64_t body_b_len, const uint64_t* name_begin, const uint64_t* name_end,
                                    uint64_t n_rows, const uint32_t* list, uint32_t m, const uint8_t* q, uint64_t q_len) {
  uint32_t first = 0, last = m;
  while (first < last) {
    const uint32_t mid = first + (last - first) / 2;
    uint64_t b, e;
    mst_admit_row_name(name_begin, name_end, n_rows, list[mid], body_b_len, &b, &e);
    if (mst_sort_compare(body_b, b, e, q, q_len) < 0) first = mid + 1; else last = mid;
  }
  return first;
}
// which text a leaf of the union takes its balances from: the row of B, or MST_DIFF_ABSENT for zeros.  An admitted leaf its own
// row, a GONE leaf none, any other leaf its owner row; a row outside the file is none.
SG_HD uint32_t mst_admit_source_row(uint32_t leaf, uint32_t depth, uint32_t n_tree, uint32_t n_new, const uint32_t* new_rows,
                                    const uint8_t* leaf_state, const uint32_t* owner, uint32_t n_rows) {
  if (leaf >= ((uint32_t)1 << depth)) return MST_DIFF_ABSENT;
  uint32_t row;
  if (leaf >= n_tree && leaf - n_tree < n_new) row = new_rows[leaf - n_tree];
  else if (leaf_state[leaf] == MST_DIFF_LEAF_GONE) return MST_DIFF_ABSENT;
  else row = owner[leaf];
  return row < n_rows ? row : MST_DIFF_ABSENT;
}

// What sa_mst_admit_measure_dev refuses before it touches a device: "" or what is wrong with the call.
inline std::string mst_admit_measure_problem(const void* b_bytes, uint64_t b_len, uint64_t b_body_off, const void* b_spans, uint64_t n_rows,
                                             uint32_t nc, const void* row_state, const void* new_rows, uint64_t n_new, uint64_t n_tree,
                                             uint32_t depth, const void* scratch, const void* name_bytes_out, const void* problem_out) {
  if (!b_bytes || !b_spans || !row_state || !new_rows || !scratch || !name_bytes_out || !problem_out) return "null argument";
  if (nc == 0 || nc > 64) return "n_currencies outside 1..64";
  if (depth > MST_AUDIT_MAX_DEPTH) return "depth above 30";
  if (b_body_off >= b_len || b_len - b_body_off >= (1ull << 32)) return "the file's body_off at or behind len, or a body of 2^32 bytes or more";
  if (n_rows == 0 || n_rows > b_len - b_body_off) return "n_rows outside 1..the body's bytes";
  if (n_new == 0 || n_new > n_rows) return "n_new outside 1..n_rows";
  if (n_tree == 0 || n_tree > ((uint64_t)1 << depth)) return "n_tree outside 1..2^depth";
  if (n_tree + n_new > ((uint64_t)1 << depth)) return "n_tree + n_new above 2^depth: the tree has no room, a rebuild is due";
  if ((uintptr_t)b_spans & 7) return "d_span_scratch is not 8-byte aligned";
  if ((uintptr_t)new_rows & 3) return "d_new_rows is not 4-byte aligned";
  if ((uintptr_t)scratch & 15) return "d_scratch is not 16-byte aligned";
  return "";
}
// What sa_mst_settle_dev refuses before it touches a device (the overlap of the two balance arrays is the entry point's own)
struct MstSettleArgs {
  const void *b_bytes, *b_spans, *owner, *leaf_state, *changed, *gone, *new_rows, *scratch;
  const void *t_bytes, *t_name_spans, *t_order, *t_leaf_name_spans;
  const void *out_bytes, *out_name_spans, *out_order, *out_leaf_name_spans;
  const void *usernames, *leaf_balances, *node_hashes, *node_balances;
  uint64_t b_len, b_body_off, n_rows, n_changed, n_gone, n_new, t_len, t_body_off, n_tree, name_bytes;
  uint32_t nc, depth;
};
inline std::string mst_settle_problem(const MstSettleArgs& a) {
  if (!a.b_bytes || !a.b_spans || !a.owner || !a.leaf_state || !a.usernames || !a.leaf_balances || !a.node_hashes || !a.node_balances)
    return "null argument";
  if (a.n_changed && !a.changed) return "null d_changed with changed leaves";
  if (a.n_gone && !a.gone) return "null d_gone with gone leaves";
  if (a.n_new && (!a.new_rows || !a.scratch || !a.t_bytes || !a.t_name_spans || !a.t_order || !a.t_leaf_name_spans || !a.out_bytes ||
                  !a.out_name_spans || !a.out_order || !a.out_leaf_name_spans))
    return "null argument with rows to admit";
  if (a.nc == 0 || a.nc > 64) return "n_currencies outside 1..64";
  if (a.depth > MST_AUDIT_MAX_DEPTH) return "depth above 30";
  if (a.b_body_off >= a.b_len || a.b_len - a.b_body_off >= (1ull << 32)) return "the file's body_off at or behind len, or a body of 2^32 bytes or more";
  if (a.n_rows == 0 || a.n_rows > a.b_len - a.b_body_off) return "n_rows outside 1..the body's bytes";
  const uint64_t leaves = (uint64_t)1 << a.depth;
  if (a.n_changed > a.n_rows || a.n_changed > leaves) return "more changed leaves than rows or leaves";
  if (a.n_gone > leaves) return "more gone leaves than leaves";
  if (a.n_new > a.n_rows) return "more new rows than rows";
  if (a.n_tree == 0 || a.n_tree > leaves) return "n_tree outside 1..2^depth";
  if (a.n_tree + a.n_new > leaves) return "n_tree + n_new above 2^depth: the tree has no room, a rebuild is due";
  if (a.n_changed + a.n_gone > a.n_tree) return "more changed and gone leaves than named leaves";
  if (a.n_new) {
    if (a.t_body_off > a.t_len || a.t_len - a.t_body_off >= (1ull << 32)) return "the tree's body_off behind len, or a body of 2^32 bytes or more";
    if (a.name_bytes > MST_ADMIT_NAME_CAP * a.n_new) return "name_bytes above 64 a new row";
    if (a.t_len - a.t_body_off + a.name_bytes >= (1ull << 32)) return "the tree's body would reach 2^32 bytes with the names appended";
  }
  if ((uintptr_t)a.b_spans & 7) return "d_span_scratch is not 8-byte aligned";
  if (((uintptr_t)a.owner | (uintptr_t)a.changed | (uintptr_t)a.gone | (uintptr_t)a.new_rows) & 3) return "a list of the diff is not 4-byte aligned";
  if ((uintptr_t)a.scratch & 15) return "d_scratch is not 16-byte aligned";
  if (((uintptr_t)a.t_name_spans | (uintptr_t)a.t_order | (uintptr_t)a.t_leaf_name_spans | (uintptr_t)a.out_name_spans | (uintptr_t)a.out_order |
       (uintptr_t)a.out_leaf_name_spans) & 3)
    return "an index array is not 4-byte aligned";
  if (((uintptr_t)a.usernames | (uintptr_t)a.leaf_balances | (uintptr_t)a.node_hashes | (uintptr_t)a.node_balances) & 15)
    return "a tree array is not 16-byte aligned";
  return "";
}
// The union of the CHANGED leaves, the GONE leaves and the admitted range n_tree .. n_tree + n_new in increasing order, or what is
// wrong with the lists: each strictly increasing, below n_tree, and no leaf in both.
inline std::string mst_admit_union(const uint32_t* changed, uint64_t n_changed, const uint32_t* gone, uint64_t n_gone, uint64_t n_tree,
                                   uint64_t n_new, std::vector<uint32_t>* out) {
  for (uint64_t j = 0; j < n_changed; j++) {
    if (changed[j] >= n_tree) return "changed leaf at position " + std::to_string(j) + " is no named leaf";
    if (j && changed[j] <= changed[j - 1]) return "changed leaves do not strictly increase at position " + std::to_string(j);
  }
  for (uint64_t j = 0; j < n_gone; j++) {
    if (gone[j] >= n_tree) return "gone leaf at position " + std::to_string(j) + " is no named leaf";
    if (j && gone[j] <= gone[j - 1]) return "gone leaves do not strictly increase at position " + std::to_string(j);
  }
  out->resize(n_changed + n_gone + n_new);
  std::merge(changed, changed + n_changed, gone, gone + n_gone, out->begin());
  for (uint64_t j = 1; j < n_changed + n_gone; j++)
    if ((*out)[j] == (*out)[j - 1]) return "leaf " + std::to_string((*out)[j]) + " is both changed and gone";
  for (uint64_t j = 0; j < n_new; j++) (*out)[n_changed + n_gone + j] = (uint32_t)(n_tree + j);
  return "";
}

// ------------------------------------------------------------------ the steps on the host, one after the other
struct MstAdmitHost {
  std::string refused;                    // "" or why nothing was written
  uint64_t problem = 0;                   // 0, or the sort's problem word of B (a name over the cap)
  uint64_t name_bytes = 0;                // what the admitted names add to the text
  std::vector<uint8_t> text;              // the tree's body afterwards
  std::vector<uint32_t> order, name_spans, leaf_name_spans;   // n_tree + n_new; twice that; twice that
  std::vector<uint32_t> sorted_new;       // the sorted NEW list: rows of B
  std::vector<uint32_t> leaves;           // the union
  std::vector<uint32_t> packed;           // its field elements: union x nc x 8 Montgomery words
};
// diff: mst_diff_host's result with complete lists; sorted_b: mst_sort_host of B; the tree's index as mst_sort_host made it of A
// (order: the file row = the leaf of every sorted position) and leaf_name_spans, begin and end of every leaf's name.  admit / zero:
// the two keywords.  Over the same tiles and groups as the kernels.
inline MstAdmitHost mst_admit_host(const uint8_t* body_b, uint64_t body_b_len, const uint64_t* words_b, uint64_t n_rows, uint32_t nc,
                                   const MstDiffHost& diff, const MstSortHost& sorted_b, const uint8_t* body_t, uint64_t body_t_len,
                                   const uint32_t* name_spans, const uint32_t* order, const uint32_t* leaf_name_spans, uint64_t n_tree,
                                   uint32_t depth, bool admit, bool zero) {
  MstAdmitHost r;
  const MstCsvSpans s = mst_csv_spans(const_cast<uint64_t*>(words_b), n_rows, nc);
  const uint32_t nt = (uint32_t)n_tree, m = admit ? (uint32_t)diff.new_rows.size() : 0u;
  if (admit && diff.new_rows.size() != diff.summary[MST_DIFF_SUM_NEW]) return r.refused = "the NEW list is incomplete", r;
  if (zero && diff.gone.size() != diff.summary[MST_DIFF_SUM_GONE]) return r.refused = "the GONE list is incomplete", r;
  if (n_tree + m > ((uint64_t)1 << depth)) return r.refused = "n_tree + n_new above 2^depth", r;
  if (m) {
    if (sorted_b.problem) return r.problem = sorted_b.problem, r;
    // measure: lengths in leaf order, tile sums, groups, offsets
    std::vector<uint32_t> place(m), rank(n_rows, MST_DIFF_ABSENT);
    const uint32_t tiles = mst_diff_tiles(m), groups = mst_diff_groups(m);
    std::vector<uint32_t> tile_sum(tiles, 0), group_total(groups, 0);
    for (uint32_t j = 0; j < m; j++) {
      uint64_t b, e;
      mst_admit_row_name(s.name_begin, s.name_end, n_rows, diff.new_rows[j], body_b_len, &b, &e);
      place[j] = (uint32_t)(e - b);
      tile_sum[j / MST_ADMIT_TILE] += place[j];
      if (diff.new_rows[j] < n_rows) rank[diff.new_rows[j]] = j;
    }
    for (uint32_t g = 0; g < groups; g++) {
      uint32_t before = 0;
      for (uint32_t t = g * MST_ADMIT_GROUP; t < tiles && t < (g + 1) * MST_ADMIT_GROUP; t++) {
        const uint32_t sum = tile_sum[t];
        tile_sum[t] = before;
        before += sum;
      }
      group_total[g] = before;
    }
    uint32_t below = 0;
    for (uint32_t j = 0; j < m; j++) {
      if (j % MST_ADMIT_TILE == 0) below = 0;
      const uint32_t tile = j / MST_ADMIT_TILE, group = tile / MST_ADMIT_GROUP, len = place[j];
      uint32_t before = 0;
      for (uint32_t g = 0; g < group; g++) before += group_total[g];
      place[j] = before + tile_sum[tile] + below;
      below += len;
    }
    for (uint32_t g = 0; g < groups; g++) r.name_bytes += group_total[g];
    if (body_t_len + r.name_bytes >= (1ull << 32)) return r.refused = "the tree's body would reach 2^32 bytes", r;
    // list: the sorted positions of B whose row is NEW, by the diff's compaction
    std::vector<uint8_t> state(n_rows);
    for (uint64_t i = 0; i < n_rows; i++) state[i] = sorted_b.order[i] < n_rows ? diff.row_state[sorted_b.order[i]] : 0;
    std::vector<uint32_t> at;
    mst_diff_compact_host(state, MST_DIFF_ROW_NEW, m, &at);
    r.sorted_new.resize(at.size());
    for (size_t k = 0; k < at.size(); k++) r.sorted_new[k] = sorted_b.order[at[k]];
    // merge
    const uint32_t all = nt + m;
    r.order.assign(all, MST_DIFF_ABSENT);
    r.name_spans.assign(2 * (size_t)all, 0);
    for (uint32_t k = 0; k < r.sorted_new.size(); k++) {
      const uint32_t row = r.sorted_new[k], j = row < n_rows ? rank[row] : MST_DIFF_ABSENT;
      uint64_t b, e;
      mst_admit_row_name(s.name_begin, s.name_end, n_rows, row, body_b_len, &b, &e);
      const uint64_t to = (uint64_t)k + mst_admit_tree_below(body_t, body_t_len, name_spans, nt, body_b + b, e - b);
      if (to >= all || j >= m) continue;
      r.order[to] = nt + j;
      r.name_spans[2 * to] = (uint32_t)(body_t_len + place[j]);
      r.name_spans[2 * to + 1] = (uint32_t)(body_t_len + place[j] + (e - b));
    }
    for (uint32_t i = 0; i < nt; i++) {
      uint64_t b, e;
      mst_names_span(name_spans, body_t_len, i, &b, &e);
      const uint64_t to = (uint64_t)i + mst_admit_list_below(body_b, body_b_len, s.name_begin, s.name_end, n_rows, r.sorted_new.data(),
                                                             (uint32_t)r.sorted_new.size(), body_t + b, e - b);
      if (to >= all) continue;
      r.order[to] = order[i];
      r.name_spans[2 * to] = name_spans[2 * (size_t)i];
      r.name_spans[2 * to + 1] = name_spans[2 * (size_t)i + 1];
    }
    // names
    r.text.assign(body_t, body_t + body_t_len);
    r.text.resize(body_t_len + r.name_bytes, 0);
    r.leaf_name_spans.assign(leaf_name_spans, leaf_name_spans + 2 * (size_t)nt);
    r.leaf_name_spans.resize(2 * (size_t)all, 0);
    for (uint32_t j = 0; j < m; j++) {
      uint64_t b, e;
      mst_admit_row_name(s.name_begin, s.name_end, n_rows, diff.new_rows[j], body_b_len, &b, &e);
      const uint64_t to = body_t_len + place[j];
      for (uint64_t k = b; k < e; k++)
        if (to + (k - b) < r.text.size()) r.text[to + (k - b)] = body_b[k];
      r.leaf_name_spans[2 * (size_t)(nt + j)] = (uint32_t)to;
      r.leaf_name_spans[2 * (size_t)(nt + j) + 1] = (uint32_t)(to + (e - b));
    }
  }
  r.refused = mst_admit_union(diff.changed.data(), diff.changed.size(), diff.gone.data(), zero ? diff.gone.size() : 0, n_tree, m, &r.leaves);
  if (!r.refused.empty()) return r;
  for (uint32_t leaf : r.leaves) {                             // pack
    const uint32_t row = mst_admit_source_row(leaf, depth, nt, m, diff.new_rows.data(), diff.leaf_state.data(), diff.owner.data(), (uint32_t)n_rows);
    for (uint32_t c = 0; c < nc; c++) {
      uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (row != MST_DIFF_ABSENT) {
        uint64_t b, e;
        mst_diff_span(s.bal_begin, s.bal_end, (uint64_t)row * nc + c, body_b_len, &b, &e);
        mst_decimal_words(body_b + b, (size_t)(e - b), w);
      }
      r.packed.insert(r.packed.end(), w, w + 8);
    }
  }
  return r;
}

#if defined(__HIPCC__)
// the measure of the admitted names on `stream`, behind mst_sort_lengths_launch: places into d_work's part, the rank of every NEW
// row, and the total at d_work[MST_ADMIT_AT_TOTAL]
hipError_t mst_admit_measure_launch(const uint64_t* d_words, uint64_t n_rows, uint32_t nc, uint64_t body_b_len, const uint32_t* d_new_rows,
                                    uint64_t n_new, uint32_t* d_work, hipStream_t stream);
// the sorted NEW list on `stream`, behind mst_sort_launch into d_work's parts
hipError_t mst_admit_list_launch(const uint8_t* d_row_state, uint64_t n_rows, uint64_t n_new, uint32_t* d_work, hipStream_t stream);
// merge and names on `stream`: the three index arrays of n_tree + n_new entries, the names behind d_text_out[body_t_len ..) (the
// old text and the old leaf spans are the caller's to copy), d_users[n_tree + j]
hipError_t mst_admit_merge_launch(const uint8_t* d_body_b, uint64_t body_b_len, const uint64_t* d_words, uint64_t n_rows, uint32_t nc,
                                  const uint32_t* d_new_rows, uint64_t n_new, const uint32_t* d_work, const uint8_t* d_body_t,
                                  uint64_t body_t_len, const uint32_t* d_name_spans, const uint32_t* d_order, uint64_t n_tree, uint32_t depth,
                                  uint8_t* d_body_out, uint64_t name_bytes, uint32_t* d_name_spans_out, uint32_t* d_order_out,
                                  uint32_t* d_leaf_name_spans_out, void* d_users, hipStream_t stream);
// pack: d_packed[j * nc + c] = balance c of the source row of leaf d_leaves[j] (mst_admit_source_row), or zero
hipError_t mst_admit_pack_launch(const uint8_t* d_body_b, uint64_t body_b_len, const uint64_t* d_words, uint64_t n_rows, uint32_t nc,
                                 const uint32_t* d_owner, const uint8_t* d_leaf_state, const uint32_t* d_new_rows, uint64_t n_new,
                                 uint64_t n_tree, const uint32_t* d_leaves, uint64_t n_leaves, uint32_t depth, void* d_packed,
                                 hipStream_t stream);
#endif

}  // namespace sg
