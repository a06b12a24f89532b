// A snapshot's usernames sorted on the device (mst_sort.hip has the kernels, ss_mst_csv_entries_sorted_dev / ss_mst_find_names in
// abi_mst.hip launch them): from the spans that pass 4 of the CSV reader leaves (mst_csv.h, mst_csv_spans) to order[i], the file
// row of leaf i, as the reference's sorted constructor orders its leaves (mst.rs:89-100), and a binary search over the result.
//
// Order: names compare byte by byte and a proper prefix comes first; equal names keep file order (Rust's sort_by and Python's
// list.sort are stable, and a tree with a name twice must come out as theirs).  Inside the reader's subset a name holds no byte
// 0x00 (mst_csv_forbidden), so a name padded with zeros to a fixed width compares as the name itself: a shorter name's padding
// is below every byte the longer one can hold there.  That is what makes a fixed-width radix sort exact, and it is the only
// place where the width matters: a name of more than MST_SORT_NAME_CAP bytes puts the file outside what the device sorts
// (row problem MST_SORT_NAME_TOO_LONG behind the reader's six, the rule still "lowest row, in it the lowest code").
//
// The sort is a stable LSD radix sort over byte positions, the last one first, 8 bits a pass, after the lookup sort's pass
// (poly_lookup_sort.cuh: histogram, one-workgroup scan, scatter with per-wave ballot ranks).  What moves is the row index alone:
// the key of row r at position p is read where the file has it, body[name_begin[r] + p], or 0 behind the name's end.  Kept from
// the model: ordering between the steps is by kernel boundaries alone, and a pass whose digit is the same in every key returns
// at its first instruction (head[]: the OR of all keys and the OR of their complements, a bit varies when both have it).  The
// host launches only as many passes as the longest name has bytes: that length rides on the copy of the problem word.
//
// Steps, stream order the only barrier between them:
//   lengths   a row per thread: a name over the cap into the problem word, else its length into the longest
//   head      a row per thread: head[] and order[0][i] = i
//   pass p    hist[digit][tile], its exclusive scan, the scatter of a tile's rows: order[side] -> order[side ^ 1]
//   gather    a field per thread: the spans in leaf order into a second block laid out as the first, order and the names' spans out
// Plain C++ below, so that the rules and the tile edges are tested without a GPU (tests/cpp/mst_sort_check.cpp runs
// mst_sort_host, the same passes over the same tiles one after the other).
#pragma once
#include "mst_csv.h"

namespace sg {

static constexpr uint32_t MST_SORT_NAME_CAP = 64;     // a UUID has 36 bytes, a hex SHA-256 64: a condition of the interface
static constexpr uint32_t MST_SORT_THREADS = 256;
static constexpr uint32_t MST_SORT_ITEMS = 8;         // rows a thread ranks in one pass
static constexpr uint32_t MST_SORT_TILE = MST_SORT_THREADS * MST_SORT_ITEMS;   // rows a workgroup ranks in one pass
static constexpr uint32_t MST_SORT_BINS = 256;
static constexpr uint32_t MST_SORT_KEY_WORDS = MST_SORT_NAME_CAP / 4;          // a padded name as little-endian words
static constexpr uint32_t MST_SORT_NAME_TOO_LONG = 7;                          // the row problem behind MST_CSV_ROW_START
static constexpr uint32_t MST_FIND_ABSENT = 0xffffffffu;
static_assert(MST_SORT_BINS == MST_SORT_THREADS, "a thread owns a digit's counter in the histogram and the scatter");

// The work space in 32-bit words: the result the host reads (problem word, longest name), head[], the two sides of the order,
// the histogram in [digit][tile] order.  Every part starts on a 16-byte boundary.
static constexpr uint32_t MST_SORT_AT_PROBLEM = 0, MST_SORT_AT_LONGEST = 2, MST_SORT_AT_HEAD = 4, MST_SORT_FRONT_WORDS = 64;
SG_HD uint64_t mst_sort_tiles(uint64_t n_rows) { return (n_rows + MST_SORT_TILE - 1) / MST_SORT_TILE; }
SG_HD uint64_t mst_sort_side_words(uint64_t n_rows) { return (n_rows + 3) & ~3ull; }
SG_HD uint64_t mst_sort_at_order(uint64_t n_rows, uint32_t side) { return MST_SORT_FRONT_WORDS + side * mst_sort_side_words(n_rows); }
SG_HD uint64_t mst_sort_at_hist(uint64_t n_rows) { return mst_sort_at_order(n_rows, 2); }
SG_HD uint64_t mst_sort_work_words(uint64_t n_rows) { return mst_sort_at_hist(n_rows) + MST_SORT_BINS * mst_sort_tiles(n_rows); }
// A pass scans its histogram with one workgroup of MST_SORT_SCAN_BLOCK threads, MST_SORT_SCAN_ITEMS words a thread and step,
// in [digit][tile] order: its steps over the histogram of n_rows.  A step's words are the tiles of some digits, not some tiles.
static constexpr uint32_t MST_SORT_SCAN_BLOCK = 1024, MST_SORT_SCAN_ITEMS = 4;
SG_HD uint64_t mst_sort_scan_steps(uint64_t n_rows) {
  const uint64_t step = (uint64_t)MST_SORT_SCAN_ITEMS * MST_SORT_SCAN_BLOCK;
  return (MST_SORT_BINS * mst_sort_tiles(n_rows) + step - 1) / step;
}

// the key byte of a name at position pos: zero behind its end
SG_HD uint32_t mst_sort_digit(const uint8_t* body, uint64_t begin, uint64_t end, uint32_t pos) {
  return begin + pos < end ? body[begin + pos] : 0u;
}
// head[w] is the OR of key word w over all names, head[MST_SORT_KEY_WORDS + w] that of its complement: position pos varies
// where some bit of its byte is in both
SG_HD bool mst_sort_varies(const uint32_t* head, uint32_t pos) {
  return (((head[pos >> 2] & head[MST_SORT_KEY_WORDS + (pos >> 2)]) >> ((pos & 3) * 8)) & 0xffu) != 0;
}
// Which side of the order holds the rows before the pass over position pos: every pass that ran -- the varying positions
// behind pos -- swapped; mst_sort_final_side: after the last pass.
SG_HD uint32_t mst_sort_ran(const uint32_t* head, uint32_t from) {
  uint32_t ran = 0;
  for (uint32_t p = from; p < MST_SORT_NAME_CAP; p++) ran += mst_sort_varies(head, p) ? 1u : 0u;
  return ran;
}
SG_HD uint32_t mst_sort_side(const uint32_t* head, uint32_t pos) { return mst_sort_ran(head, pos + 1) & 1u; }
SG_HD uint32_t mst_sort_final_side(const uint32_t* head) { return mst_sort_ran(head, 0) & 1u; }
// what the lengths step reports of a row whose name has len bytes
SG_HD bool mst_sort_name_too_long(uint64_t len) { return len > MST_SORT_NAME_CAP; }
// three-way compare of the name body[begin .. end) with the query q[0 .. q_len): bytes, a proper prefix first
SG_HD int mst_sort_compare(const uint8_t* body, uint64_t begin, uint64_t end, const uint8_t* q, uint64_t q_len) {
  const uint64_t len = end - begin, common = len < q_len ? len : q_len;
  for (uint64_t k = 0; k < common; k++) {
    const uint8_t a = body[begin + k], b = q[k];
    if (a != b) return a < b ? -1 : 1;
  }
  return len < q_len ? -1 : len > q_len ? 1 : 0;
}
// The lowest leaf whose name equals the query, or MST_FIND_ABSENT: a lower bound over the sorted names' (begin, end) pairs.
// A pair that does not lie in the body is cut to it, so that whatever the pairs hold nothing outside the body is read.
SG_HD uint32_t mst_find_name(const uint8_t* body, uint64_t body_len, const uint32_t* name_spans, uint32_t n, const uint8_t* q,
                             uint64_t q_len) {
  uint32_t first = 0, last = n;                     // the first leaf whose name is not below the query
  while (first < last) {
    const uint32_t mid = first + (last - first) / 2;
    uint64_t e = name_spans[2 * (uint64_t)mid + 1], b = name_spans[2 * (uint64_t)mid];
    if (e > body_len) e = body_len;
    if (b > e) b = e;
    if (mst_sort_compare(body, b, e, q, q_len) < 0) first = mid + 1; else last = mid;
  }
  if (first == n) return MST_FIND_ABSENT;
  uint64_t e = name_spans[2 * (uint64_t)first + 1], b = name_spans[2 * (uint64_t)first];
  if (e > body_len) e = body_len;
  if (b > e) b = e;
  return mst_sort_compare(body, b, e, q, q_len) == 0 ? first : MST_FIND_ABSENT;
}

// ------------------------------------------------------------------ the steps on the host, tile by tile
struct MstSortHost {
  uint64_t problem = 0;                 // 0, or mst_csv_problem_word of the lowest offending row, code 7 included
  uint32_t longest = 0;                 // bytes of the longest name: the passes the host launches
  uint32_t passes_run = 0;              // ... and how many of them found their digit varying
  std::vector<uint32_t> order;          // order[i]: the file row of leaf i (empty with a problem)
  std::vector<uint32_t> name_spans;     // begin and end of leaf i's name
};
// After mst_csv_host: `csv` as it returned for the same body (no flag up, a row at least).  The lengths step takes a row whose
// name span the split left unwritten as an empty name -- the device zeroes the name spans before the split, the host's words
// start as ~0 in both -- and a row that has a lower code keeps it under the minimum.
inline MstSortHost mst_sort_host(const uint8_t* body, const MstCsvHost& csv, uint32_t nc) {
  MstSortHost r;
  const uint64_t n = csv.n_rows;
  std::vector<uint64_t> words = csv.words;
  const MstCsvSpans s = mst_csv_spans(words.data(), n, nc);
  uint64_t problem = csv.problem ? csv.problem : MST_CSV_NO_PROBLEM;
  for (uint64_t row = 0; row < n; row++) {             // lengths
    const uint64_t len = s.name_end[row] - s.name_begin[row];
    if (mst_sort_name_too_long(len)) {
      const uint64_t word = mst_csv_problem_word(row, MST_SORT_NAME_TOO_LONG);
      if (word < problem) problem = word;
    } else if (len > r.longest) {
      r.longest = (uint32_t)len;
    }
  }
  r.problem = problem == MST_CSV_NO_PROBLEM ? 0 : problem;
  if (r.problem) return r;
  std::vector<uint32_t> work(mst_sort_work_words(n), 0);
  uint32_t* head = work.data() + MST_SORT_AT_HEAD;
  uint32_t* side[2] = {work.data() + mst_sort_at_order(n, 0), work.data() + mst_sort_at_order(n, 1)};
  uint32_t* hist = work.data() + mst_sort_at_hist(n);
  const uint64_t tiles = mst_sort_tiles(n);
  for (uint64_t row = 0; row < n; row++) {             // head
    for (uint32_t p = 0; p < MST_SORT_NAME_CAP; p++) {
      const uint32_t d = mst_sort_digit(body, s.name_begin[row], s.name_end[row], p);
      head[p >> 2] |= d << ((p & 3) * 8);
      head[MST_SORT_KEY_WORDS + (p >> 2)] |= (~d & 0xffu) << ((p & 3) * 8);
    }
    side[0][row] = (uint32_t)row;
  }
  for (uint32_t pos = r.longest; pos-- != 0;) {        // the passes, the last position first
    if (!mst_sort_varies(head, pos)) continue;
    r.passes_run++;
    const uint32_t* src = side[mst_sort_side(head, pos)];
    uint32_t* dst = side[mst_sort_side(head, pos) ^ 1u];
    auto digit = [&](uint64_t i) { return mst_sort_digit(body, s.name_begin[src[i]], s.name_end[src[i]], pos); };
    for (uint64_t i = 0; i < MST_SORT_BINS * tiles; i++) hist[i] = 0;
    for (uint64_t i = 0; i < n; i++) hist[digit(i) * tiles + i / MST_SORT_TILE]++;
    uint32_t before = 0;
    for (uint64_t i = 0; i < MST_SORT_BINS * tiles; i++) {   // the scan, in [digit][tile] order
      const uint32_t count = hist[i];
      hist[i] = before;
      before += count;
    }
    for (uint64_t i = 0; i < n; i++) dst[hist[digit(i) * tiles + i / MST_SORT_TILE]++] = src[i];   // a tile's rows in tile order
  }
  const uint32_t* sorted = side[mst_sort_final_side(head)];
  r.order.assign(sorted, sorted + n);
  for (uint64_t i = 0; i < n; i++) {                   // gather
    r.name_spans.push_back((uint32_t)s.name_begin[sorted[i]]);
    r.name_spans.push_back((uint32_t)s.name_end[sorted[i]]);
  }
  return r;
}

#if defined(__HIPCC__)
// the lengths step over the spans in d_words: d_result (the work space's front) holds the problem word the split left and gets
// the longest name beside it
hipError_t mst_sort_lengths_launch(const uint64_t* d_words, uint64_t n_rows, uint32_t nc, uint32_t* d_result, hipStream_t stream);
// head, `longest` passes and the gather: d_order (n_rows u32), d_name_spans (n_rows x 2 u32) and the spans in leaf order in
// d_sorted_words, laid out as d_words is (its row starts stay unwritten)
hipError_t mst_sort_launch(const uint8_t* d_body, const uint64_t* d_words, uint64_t n_rows, uint32_t nc, uint32_t longest,
                           uint32_t* d_work, uint32_t* d_order, uint32_t* d_name_spans, uint64_t* d_sorted_words, hipStream_t stream);
// out[j] = mst_find_name of query j = d_query[d_query_off[j] .. d_query_off[j + 1]); with d_order (n_rows u32, else nullptr) the
// position found goes through it: out[j] = d_order[position]
hipError_t mst_find_names_launch(const uint8_t* d_body, uint64_t body_len, const uint32_t* d_name_spans, const uint32_t* d_order,
                                 uint32_t n_rows, const uint8_t* d_query, const uint64_t* d_query_off, size_t m, uint32_t* d_out,
                                 hipStream_t stream);
#endif

}  // namespace sg
