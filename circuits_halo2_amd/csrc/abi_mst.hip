// C ABI, Merkle sum tree family: the inclusion circuit's keygen columns and sg_mst_* -- leaves, levels and whole trees, entries from
// names and decimal balances, the in-place update, the range audit, the index and report of the names and the circuit's witness
// (summa_gpu.hip holds the core).
#include "abi_internal.h"
#include "../../include/summa_snapshot.h"
#include "mst_csv.h"
#include "mst_sort.h"
#include "mst_audit.h"
#include "mst_names.h"
#include "mst_entries.h"
#include "mst_update_plan.h"

using namespace sg;
namespace {

constexpr uint32_t kMaxDepth = 30;   // 2^31 - 1 nodes: a node's number in the level-major arrays fits 32 bits
// What is wrong with the shape of a call (nullptr: nothing): n_currencies balances a node, a tree of 2^depth leaves (0 where
// the entry point takes no depth), and `rest_ok`, the bounds that are the entry point's own.  The caller puts its name in front.
const char* shape_problem(uint32_t n_currencies, uint32_t depth, bool rest_ok = true) {
  return n_currencies == 0 || n_currencies > 64 || depth > kMaxDepth || !rest_ok ? "bad size" : nullptr;
}
int refuse(const char* who, const char* problem) { return fail(SG_ERR_INVALID, (std::string(who) + ": " + problem).c_str()); }
// The lookup by name of `who`, ss_mst_find_names (d_order nullptr: the position found is the leaf) or ss_mst_find_leaves (the
// position goes through d_order, in the kernel).  The queries travel in one work space of the caller's stream: the offsets, the
// answers, then the bytes.
int find_names(const std::string& who, const void* d_bytes, uint64_t len, uint64_t body_off, const void* d_name_spans, const void* d_order,
               uint64_t n_rows, const uint8_t* name_bytes, const uint64_t* name_off, size_t m, uint32_t* index_out, void* stream) {
  if (m == 0 || m >= (1ull << 32) || n_rows == 0 || n_rows >= (1ull << 32) || body_off > len || len - body_off >= (1ull << 32) ||
      ((uintptr_t)d_name_spans & 3) || ((uintptr_t)d_order & 3))
    return refuse(who.c_str(), "bad size");
  if (name_off[0] != 0) return refuse(who.c_str(), "offsets do not start at 0");
  for (size_t j = 0; j < m; j++)
    if (name_off[j + 1] < name_off[j]) return refuse(who.c_str(), "offsets decrease");
  const size_t query_len = name_off[m], at_out = 8 * (m + 1), at_bytes = (at_out + 4 * m + 7) & ~(size_t)7;
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  uint8_t* d = nullptr;
  CHECK_HIP(scratch_for(s, 14, at_bytes + query_len + 1, &d), (who + ": work space").c_str());
  CHECK_HIP(hipMemcpyAsync(d, name_off, 8 * (m + 1), hipMemcpyHostToDevice, s), (who + ": offsets").c_str());
  if (query_len) CHECK_HIP(hipMemcpyAsync(d + at_bytes, name_bytes, query_len, hipMemcpyHostToDevice, s), (who + ": names").c_str());
  CHECK_HIP(mst_find_names_launch(static_cast<const uint8_t*>(d_bytes) + body_off, len - body_off, static_cast<const uint32_t*>(d_name_spans),
                                  static_cast<const uint32_t*>(d_order), (uint32_t)n_rows, d + at_bytes,
                                  reinterpret_cast<const uint64_t*>(d), m, reinterpret_cast<uint32_t*>(d + at_out), s),
            who.c_str());
  TRY(download(reinterpret_cast<uint8_t*>(index_out), d + at_out, 4 * m, s));   // waits for the stream
  return SG_OK;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------ keygen's circuit side
// What `keygen_vk` / `keygen_pk` need of `MstInclusionCircuit::synthesize` over 2^k rows [REF zk_prover/src/circuits/
// merkle_sum_tree.rs:228-520 replayed over halo2's SimpleFloorPlanner: include/summa_circuit.hpp]: the 11 fixed columns (round
// constants, range table, compressed selectors, constants) and the 6 permutation columns sigma_c[row] = the label delta^c' omega^row'
// of the cell (c, row) is copy-constrained to.  Host only (no device needed); Montgomery words, column-major.
int sg_mst_inclusion_keygen_columns(uint32_t k, uint32_t levels, uint32_t n_currencies, uint32_t n_bytes, uint8_t* fixed_out,
                                    uint8_t* sigma_out, uint32_t* rows_used_out) {
  if (!fixed_out || !sigma_out || k < 4 || k > 25 || levels == 0 || levels > 48 || n_currencies == 0 || n_currencies > 16 || n_bytes == 0 ||
      n_bytes > 31)
    return fail(SG_ERR_INVALID, "sg_mst_inclusion_keygen_columns: bad argument");
  try {
    using summa::prover::Fr;
    const summa::circuit::FloorPlan fp(k, levels, n_currencies, n_bytes);
    const size_t n = (size_t)1 << k;
    if (fp.rows_used + summa::circuit::BLINDING_FACTORS + 1 > n) return fail(SG_ERR_INVALID, "sg_mst_inclusion_keygen_columns: not enough rows");
    static const uint8_t root_2_28[32] = {0x03, 0xdd, 0xb9, 0xf5, 0x16, 0x6d, 0x18, 0xb7, 0x98, 0x86, 0x5e, 0xa9, 0x3d, 0xd3, 0x1f, 0x74,
                                          0x32, 0x15, 0xcf, 0x6d, 0xd3, 0x93, 0x29, 0xc8, 0xd3, 0x4f, 0x1e, 0xd9, 0x60, 0xc3, 0x7c, 0x9c};
    Fr omega = Fr::from_be_bytes_reduced(root_2_28);
    for (uint32_t i = k; i < 28; i++) omega = omega * omega;
    for (uint32_t c = 0; c < summa::circuit::NUM_FIXED; c++) std::memcpy(fixed_out + 32 * n * c, fp.fixed[c].data(), 32 * n);
    const auto sigma = fp.sigma(omega);
    for (uint32_t c = 0; c < summa::circuit::NUM_PERM; c++) std::memcpy(sigma_out + 32 * n * c, sigma[c].data(), 32 * n);
    if (rows_used_out) *rows_used_out = fp.rows_used;
  } catch (const std::exception& ex) {
    return fail(SG_ERR_INVALID, (std::string("sg_mst_inclusion_keygen_columns: ") + ex.what()).c_str());
  }
  return SG_OK;
}

// ------------------------------------------------------------------ witness side (Merkle sum tree)
int sg_mst_leaves_dev(const void* d_usernames, const void* d_balances, size_t n, uint32_t n_currencies,
                      void* d_hashes, void* stream) {
  if (n && (!d_usernames || !d_balances || !d_hashes)) return fail(SG_ERR_INVALID, "sg_mst_leaves: null argument");
  if (const char* problem = shape_problem(n_currencies, 0, n < (1ull << 32))) return refuse("sg_mst_leaves", problem);
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  hipError_t e = g_ctx->witness.init(g_ctx->stream);
  if (e == hipSuccess)
    e = g_ctx->witness.leaves(nullptr, static_cast<const fp_words*>(d_usernames), static_cast<const fp_words*>(d_balances), n,
                              n_currencies, static_cast<fp_words*>(d_hashes), nullptr, nullptr, s);
  if (e != hipSuccess) return hip_fail("mst leaves", e);
  return SG_OK;
}
int sg_mst_level_dev(const void* d_child_hashes, const void* d_child_balances, size_t n_parents, uint32_t n_currencies,
                     void* d_hashes, void* d_balances, void* stream) {
  if (n_parents && (!d_child_hashes || !d_child_balances || !d_hashes || !d_balances))
    return fail(SG_ERR_INVALID, "sg_mst_level: null argument");
  if (const char* problem = shape_problem(n_currencies, 0, n_parents < (1ull << 31))) return refuse("sg_mst_level", problem);
  LOCKED_CTX();
  hipError_t e = g_ctx->witness.init(g_ctx->stream);
  if (e == hipSuccess)
    e = g_ctx->witness.level(nullptr, static_cast<const fp_words*>(d_child_hashes), static_cast<const fp_words*>(d_child_balances),
                             n_parents, n_currencies, static_cast<fp_words*>(d_hashes),
                             static_cast<fp_words*>(d_balances), pick_stream(stream));
  if (e != hipSuccess) return hip_fail("mst level", e);
  return SG_OK;
}
// whole tree: node arrays are level-major (2^depth leaves, then 2^(depth-1) parents, ..., the root)
int sg_mst_build_dev(const void* d_usernames, const void* d_leaf_balances, uint32_t depth, uint32_t n_currencies,
                     void* d_node_hashes, void* d_node_balances, void* stream) {
  if (!d_usernames || !d_leaf_balances || !d_node_hashes || !d_node_balances || depth > kMaxDepth)
    return fail(SG_ERR_INVALID, "sg_mst_build: bad argument");
  const size_t n = (size_t)1 << depth, nc = n_currencies;
  uint8_t* h = static_cast<uint8_t*>(d_node_hashes);
  uint8_t* b = static_cast<uint8_t*>(d_node_balances);
  TRY(sg_mst_leaves_dev(d_usernames, d_leaf_balances, n, n_currencies, h, stream));
  {
    LOCKED_CTX();
    CHECK_HIP(hipMemcpyAsync(b, d_leaf_balances, n * nc * 32, hipMemcpyDeviceToDevice, pick_stream(stream)), "mst balances");
  }
  for (uint32_t l = 1; l <= depth; l++) {
    const size_t child = mst_level_first(l - 1, depth), parent = mst_level_first(l, depth);
    TRY(sg_mst_level_dev(h + 32 * child, b + 32 * child * nc, n >> l, n_currencies, h + 32 * parent, b + 32 * parent * nc, stream));
  }
  return SG_OK;
}
// Entry::new for a whole snapshot (mst_entries.hip).  Everything that can be wrong with the host buffers is found here, before
// the device is touched: the kernels trust their offsets.  The four buffers travel in one work space of the caller's stream
// (names, digits, then the two offset arrays from an 8-byte boundary on), so calls on one stream reuse it in stream order.
int sg_mst_entries_dev(const uint8_t* name_bytes, const uint64_t* name_off, const uint8_t* digit_bytes, const uint64_t* digit_off,
                       size_t n, size_t rows, uint32_t n_currencies, void* d_usernames, void* d_balances, void* stream) {
  if (!name_bytes || !name_off || !digit_bytes || !digit_off || !d_usernames || !d_balances)
    return fail(SG_ERR_INVALID, "sg_mst_entries: null argument");
  const bool sizes_ok = n != 0 && rows >= n && rows < (1ull << 32);
  if (const char* problem = shape_problem(n_currencies, 0, sizes_ok)) return refuse("sg_mst_entries", problem);
  const std::string problem = mst_entries_problem(name_off, digit_bytes, digit_off, n, n_currencies);
  if (!problem.empty()) return fail(SG_ERR_INVALID, ("sg_mst_entries: " + problem).c_str());
  const size_t fields = n * (size_t)n_currencies;
  const size_t name_len = name_off[n], digit_len = digit_off[fields];
  const size_t at_digits = name_len, at_name_off = (name_len + digit_len + 7) & ~(size_t)7, at_digit_off = at_name_off + 8 * (n + 1);
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  uint8_t* d = nullptr;
  CHECK_HIP(scratch_for(s, 11, at_digit_off + 8 * (fields + 1), &d), "sg_mst_entries: work space");
  if (name_len) CHECK_HIP(hipMemcpyAsync(d, name_bytes, name_len, hipMemcpyHostToDevice, s), "sg_mst_entries: names");
  CHECK_HIP(hipMemcpyAsync(d + at_digits, digit_bytes, digit_len, hipMemcpyHostToDevice, s), "sg_mst_entries: digits");
  CHECK_HIP(hipMemcpyAsync(d + at_name_off, name_off, 8 * (n + 1), hipMemcpyHostToDevice, s), "sg_mst_entries: name offsets");
  CHECK_HIP(hipMemcpyAsync(d + at_digit_off, digit_off, 8 * (fields + 1), hipMemcpyHostToDevice, s), "sg_mst_entries: digit offsets");
  CHECK_HIP(mst_entries_launch(d, reinterpret_cast<const uint64_t*>(d + at_name_off), d + at_digits,
                               reinterpret_cast<const uint64_t*>(d + at_digit_off), n, rows, n_currencies, d_usernames, d_balances, s),
            "sg_mst_entries");
  return SG_OK;
}
// The same two arrays from the text of a snapshot CSV that already lies on the device (mst_csv.h has the rules and the passes,
// mst_entries.hip the kernels).  Two calls, because the host sizes the outputs by the row count: the scan ends in one small
// copy and a wait, and so does the split, whose problem word the host reads before anything is hashed.  What is wrong with
// the arguments is refused before the device is touched; what is unusual about the text is reported, never refused.
void sg_mst_csv_geometry(uint32_t* tile_bytes, uint32_t* row_cap) {
  if (tile_bytes) *tile_bytes = MST_CSV_TILE;
  if (row_cap) *row_cap = MST_CSV_ROW_CAP;
}
int sg_mst_csv_scan_dev(const void* d_bytes, uint64_t len, uint64_t body_off, void* d_tile_scratch, uint64_t* n_rows_out,
                        uint32_t* flags_out, void* stream) {
  if (!d_bytes || !d_tile_scratch || !n_rows_out || !flags_out) return fail(SG_ERR_INVALID, "sg_mst_csv_scan: null argument");
  if (body_off > len || len - body_off >= (1ull << 32) || ((uintptr_t)d_tile_scratch & 3)) return refuse("sg_mst_csv_scan", "bad size");
  const uint64_t body_len = len - body_off, n_tiles = mst_csv_tiles(body_len);
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  uint32_t* tiles = static_cast<uint32_t*>(d_tile_scratch);
  CHECK_HIP(mst_csv_scan_launch(static_cast<const uint8_t*>(d_bytes) + body_off, body_len, tiles, s), "sg_mst_csv_scan");
  uint32_t result[2];
  TRY(download(reinterpret_cast<uint8_t*>(result), tiles + n_tiles, sizeof result, s));
  *n_rows_out = result[0];
  *flags_out = result[1];
  return SG_OK;
}
int sg_mst_csv_entries_dev(const void* d_bytes, uint64_t len, uint64_t body_off, const void* d_tile_scratch, uint32_t delimiter,
                           uint32_t n_currencies, uint64_t n_rows, uint64_t rows, void* d_span_scratch, void* d_usernames,
                           void* d_balances, uint64_t* problem_out, void* stream) {
  if (!d_bytes || !d_tile_scratch || !d_span_scratch || !d_usernames || !d_balances || !problem_out)
    return fail(SG_ERR_INVALID, "sg_mst_csv_entries: null argument");
  const bool delimiter_ok = delimiter < 256 && delimiter != '\n' && delimiter != '\r' && !(delimiter >= '0' && delimiter <= '9') && !mst_csv_forbidden((uint8_t)delimiter);
  // a row takes a byte of the body at least (its newline, or the last row's text)
  const bool sizes_ok = body_off < len && len - body_off < (1ull << 32) && n_rows != 0 && n_rows <= len - body_off && rows >= n_rows &&
                        rows < (1ull << 32) && !((uintptr_t)d_tile_scratch & 3) && !((uintptr_t)d_span_scratch & 7) && delimiter_ok;
  if (const char* problem = shape_problem(n_currencies, 0, sizes_ok)) return refuse("sg_mst_csv_entries", problem);
  const uint64_t body_len = len - body_off;
  const uint8_t* body = static_cast<const uint8_t*>(d_bytes) + body_off;
  uint64_t* words = static_cast<uint64_t*>(d_span_scratch);
  uint64_t* d_problem = words + mst_csv_span_words(n_rows, n_currencies);
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  CHECK_HIP(mst_csv_split_launch(body, body_len, static_cast<const uint32_t*>(d_tile_scratch), (uint8_t)delimiter, n_currencies, n_rows, words,
                                 d_problem, s),
            "sg_mst_csv_entries: split");
  uint64_t problem = 0;
  TRY(download(reinterpret_cast<uint8_t*>(&problem), d_problem, sizeof problem, s));
  *problem_out = problem == MST_CSV_NO_PROBLEM ? 0 : problem;
  if (*problem_out) return SG_OK;                            // the outputs stay unwritten
  CHECK_HIP(mst_csv_entries_launch(body, words, n_rows, rows, n_currencies, d_usernames, d_balances, s), "sg_mst_csv_entries");
  return SG_OK;
}
// The sorted flavour (include/summa_snapshot.h; mst_sort.h has the rules and the work space, mst_sort.cuh the kernels): the split
// as above with its problem word in the sort's work space, where the lengths step puts the longest name beside it -- one copy
// and one wait for both, and the host launches as many passes as that name has bytes.  The name spans are zeroed before the
// split, so that a row it reports without writing them has an empty name for the lengths step.  The spans in leaf order go
// into a second block of the span scratch, laid out as the first, and the hashing kernels run over it as they stand.
void ss_mst_sort_geometry(uint32_t* name_cap, uint32_t* tile_rows) {
  if (name_cap) *name_cap = MST_SORT_NAME_CAP;
  if (tile_rows) *tile_rows = MST_SORT_TILE;
}
int ss_mst_sort_scratch(uint64_t n_rows, uint64_t* bytes_out) {
  if (!bytes_out) return fail(SG_ERR_INVALID, "ss_mst_sort_scratch: null argument");
  if (n_rows == 0 || n_rows >= (1ull << 32)) return refuse("ss_mst_sort_scratch", "bad size");
  *bytes_out = 4 * mst_sort_work_words(n_rows);
  return SG_OK;
}
int ss_mst_csv_entries_sorted_dev(const void* d_bytes, uint64_t len, uint64_t body_off, const void* d_tile_scratch, uint32_t delimiter,
                                  uint32_t n_currencies, uint64_t n_rows, uint64_t rows, void* d_span_scratch, void* d_sort_scratch,
                                  void* d_order, void* d_name_spans, void* d_usernames, void* d_balances, uint64_t* problem_out,
                                  void* stream) {
  if (!d_bytes || !d_tile_scratch || !d_span_scratch || !d_sort_scratch || !d_order || !d_name_spans || !d_usernames || !d_balances ||
      !problem_out)
    return fail(SG_ERR_INVALID, "ss_mst_csv_entries_sorted: null argument");
  const bool delimiter_ok = delimiter < 256 && delimiter != '\n' && delimiter != '\r' && !(delimiter >= '0' && delimiter <= '9') && !mst_csv_forbidden((uint8_t)delimiter);
  const bool sizes_ok = body_off < len && len - body_off < (1ull << 32) && n_rows != 0 && n_rows <= len - body_off && rows >= n_rows &&
                        rows < (1ull << 32) && !((uintptr_t)d_tile_scratch & 3) && !((uintptr_t)d_span_scratch & 7) && delimiter_ok &&
                        !((uintptr_t)d_sort_scratch & 15) && !((uintptr_t)d_order & 3) && !((uintptr_t)d_name_spans & 3);
  if (const char* problem = shape_problem(n_currencies, 0, sizes_ok)) return refuse("ss_mst_csv_entries_sorted", problem);
  const uint64_t body_len = len - body_off;
  const uint8_t* body = static_cast<const uint8_t*>(d_bytes) + body_off;
  uint64_t* words = static_cast<uint64_t*>(d_span_scratch);
  uint64_t* sorted_words = words + mst_csv_span_words(n_rows, n_currencies);
  uint32_t* work = static_cast<uint32_t*>(d_sort_scratch);
  const MstCsvSpans spans = mst_csv_spans(words, n_rows, n_currencies);
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  CHECK_HIP(hipMemsetAsync(work, 0, 4 * MST_SORT_FRONT_WORDS, s), "ss_mst_csv_entries_sorted: work space");
  CHECK_HIP(hipMemsetAsync(spans.name_begin, 0, 16 * n_rows, s), "ss_mst_csv_entries_sorted: name spans");   // name_end follows
  CHECK_HIP(mst_csv_split_launch(body, body_len, static_cast<const uint32_t*>(d_tile_scratch), (uint8_t)delimiter, n_currencies, n_rows, words,
                                 reinterpret_cast<uint64_t*>(work + MST_SORT_AT_PROBLEM), s),
            "ss_mst_csv_entries_sorted: split");
  CHECK_HIP(mst_sort_lengths_launch(words, n_rows, n_currencies, work, s), "ss_mst_csv_entries_sorted: lengths");
  uint64_t result[2] = {0, 0};                               // the problem word, then the longest name in the low half
  TRY(download(reinterpret_cast<uint8_t*>(result), work, sizeof result, s));
  *problem_out = result[0] == MST_CSV_NO_PROBLEM ? 0 : result[0];
  if (*problem_out) return SG_OK;                            // the outputs stay unwritten
  CHECK_HIP(mst_sort_launch(body, words, n_rows, n_currencies, (uint32_t)result[1], work, static_cast<uint32_t*>(d_order),
                            static_cast<uint32_t*>(d_name_spans), sorted_words, s),
            "ss_mst_csv_entries_sorted: sort");
  CHECK_HIP(mst_csv_entries_launch(body, sorted_words, n_rows, rows, n_currencies, d_usernames, d_balances, s), "ss_mst_csv_entries_sorted");
  return SG_OK;
}
int ss_mst_find_names(const void* d_bytes, uint64_t len, uint64_t body_off, const void* d_name_spans, uint64_t n_rows,
                      const uint8_t* name_bytes, const uint64_t* name_off, size_t m, uint32_t* index_out, void* stream) {
  if (!d_bytes || !d_name_spans || !name_bytes || !name_off || !index_out) return fail(SG_ERR_INVALID, "ss_mst_find_names: null argument");
  return find_names("ss_mst_find_names", d_bytes, len, body_off, d_name_spans, nullptr, n_rows, name_bytes, name_off, m, index_out, stream);
}
// The names beside a tree whose leaves stay in file order (include/summa_snapshot.h; mst_names.h has the rules, mst_names.cuh the
// kernels).  The index is the sorted constructor up to the hashing: the split again -- sg_mst_csv_entries_dev declares its span
// scratch the library's own, so nothing here depends on what that call left there --, the lengths, one copy and one wait for the
// problem word and the longest name, the sort, and the split's name spans narrowed into d_leaf_name_spans.
int ss_mst_csv_name_index_dev(const void* d_bytes, uint64_t len, uint64_t body_off, const void* d_tile_scratch, uint32_t delimiter,
                              uint32_t n_currencies, uint64_t n_rows, void* d_span_scratch, void* d_sort_scratch, void* d_order,
                              void* d_name_spans, void* d_leaf_name_spans, uint64_t* problem_out, void* stream) {
  if (!d_bytes || !d_tile_scratch || !d_span_scratch || !d_sort_scratch || !d_order || !d_name_spans || !d_leaf_name_spans || !problem_out)
    return fail(SG_ERR_INVALID, "ss_mst_csv_name_index: null argument");
  const bool delimiter_ok = delimiter < 256 && delimiter != '\n' && delimiter != '\r' && !(delimiter >= '0' && delimiter <= '9') && !mst_csv_forbidden((uint8_t)delimiter);
  const bool sizes_ok = body_off < len && len - body_off < (1ull << 32) && n_rows != 0 && n_rows <= len - body_off &&
                        !((uintptr_t)d_tile_scratch & 3) && !((uintptr_t)d_span_scratch & 7) && delimiter_ok && !((uintptr_t)d_sort_scratch & 15) &&
                        !((uintptr_t)d_order & 3) && !((uintptr_t)d_name_spans & 3) && !((uintptr_t)d_leaf_name_spans & 3);
  if (const char* problem = shape_problem(n_currencies, 0, sizes_ok)) return refuse("ss_mst_csv_name_index", problem);
  const uint64_t body_len = len - body_off;
  const uint8_t* body = static_cast<const uint8_t*>(d_bytes) + body_off;
  uint64_t* words = static_cast<uint64_t*>(d_span_scratch);
  uint64_t* sorted_words = words + mst_csv_span_words(n_rows, n_currencies);
  uint32_t* work = static_cast<uint32_t*>(d_sort_scratch);
  const MstCsvSpans spans = mst_csv_spans(words, n_rows, n_currencies);
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  CHECK_HIP(hipMemsetAsync(work, 0, 4 * MST_SORT_FRONT_WORDS, s), "ss_mst_csv_name_index: work space");
  CHECK_HIP(hipMemsetAsync(spans.name_begin, 0, 16 * n_rows, s), "ss_mst_csv_name_index: name spans");   // name_end follows
  CHECK_HIP(mst_csv_split_launch(body, body_len, static_cast<const uint32_t*>(d_tile_scratch), (uint8_t)delimiter, n_currencies, n_rows, words,
                                 reinterpret_cast<uint64_t*>(work + MST_SORT_AT_PROBLEM), s),
            "ss_mst_csv_name_index: split");
  CHECK_HIP(mst_sort_lengths_launch(words, n_rows, n_currencies, work, s), "ss_mst_csv_name_index: lengths");
  uint64_t result[2] = {0, 0};                               // the problem word, then the longest name in the low half
  TRY(download(reinterpret_cast<uint8_t*>(result), work, sizeof result, s));
  *problem_out = result[0] == MST_CSV_NO_PROBLEM ? 0 : result[0];
  if (*problem_out) return SG_OK;                            // the outputs stay unwritten
  CHECK_HIP(mst_sort_launch(body, words, n_rows, n_currencies, (uint32_t)result[1], work, static_cast<uint32_t*>(d_order),
                            static_cast<uint32_t*>(d_name_spans), sorted_words, s),
            "ss_mst_csv_name_index: sort");
  CHECK_HIP(mst_names_leaf_spans_launch(words, n_rows, n_currencies, static_cast<uint32_t*>(d_leaf_name_spans), s),
            "ss_mst_csv_name_index: leaf spans");
  return SG_OK;
}
int ss_mst_find_leaves(const void* d_bytes, uint64_t len, uint64_t body_off, const void* d_name_spans, const void* d_order, uint64_t n_rows,
                       const uint8_t* name_bytes, const uint64_t* name_off, size_t m, uint32_t* index_out, void* stream) {
  if (!d_bytes || !d_name_spans || !d_order || !name_bytes || !name_off || !index_out)
    return fail(SG_ERR_INVALID, "ss_mst_find_leaves: null argument");
  return find_names("ss_mst_find_leaves", d_bytes, len, body_off, d_name_spans, d_order, n_rows, name_bytes, name_off, m, index_out, stream);
}
// The report of the names that occur more than once: three launches behind one small memset, then one 16-byte copy and the
// call's only wait.
int ss_mst_duplicate_names_scratch(uint64_t n_rows, uint64_t* bytes_out) {
  if (!bytes_out) return fail(SG_ERR_INVALID, "ss_mst_duplicate_names_scratch: null argument");
  if (n_rows == 0 || n_rows >= (1ull << 32)) return refuse("ss_mst_duplicate_names_scratch", "bad size");
  *bytes_out = mst_names_scratch_bytes(n_rows);
  return SG_OK;
}
int ss_mst_duplicate_names_dev(const void* d_bytes, uint64_t len, uint64_t body_off, const void* d_name_spans, const void* d_order,
                               uint64_t n_rows, void* d_shadowed, void* d_first, uint64_t cap, void* d_scratch, uint64_t* summary_out,
                               void* stream) {
  const std::string problem = mst_names_problem(d_bytes, len, body_off, d_name_spans, d_order, n_rows, d_shadowed, d_first, cap, d_scratch,
                                                summary_out);
  if (!problem.empty()) return refuse("ss_mst_duplicate_names", problem.c_str());
  uint32_t* work = static_cast<uint32_t*>(d_scratch);
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  CHECK_HIP(hipMemsetAsync(work, 0, 4 * MST_NAMES_FRONT_WORDS, s), "ss_mst_duplicate_names: work space");
  CHECK_HIP(mst_names_launch(static_cast<const uint8_t*>(d_bytes) + body_off, len - body_off, static_cast<const uint32_t*>(d_name_spans),
                             static_cast<const uint32_t*>(d_order), n_rows, static_cast<uint32_t*>(d_shadowed),
                             static_cast<uint32_t*>(d_first), cap, work, s),
            "ss_mst_duplicate_names");
  uint32_t result[MST_NAMES_FRONT_WORDS];
  TRY(download(reinterpret_cast<uint8_t*>(result), work, sizeof result, s));   // waits for the stream
  summary_out[0] = result[MST_NAMES_AT_REPEATED];
  summary_out[1] = result[MST_NAMES_AT_SHADOWED];
  summary_out[2] = summary_out[1] < cap ? summary_out[1] : cap;
  return SG_OK;
}
// The range audit of a built tree (include/summa_snapshot.h; mst_audit.h has the rules and the work space, mst_audit.cuh the
// kernels): four launches behind one small memset, then one 16-byte copy and the call's only wait.
int ss_mst_range_audit_scratch(uint32_t depth, uint64_t* bytes_out) {
  if (!bytes_out) return fail(SG_ERR_INVALID, "ss_mst_range_audit_scratch: null argument");
  if (depth > MST_AUDIT_MAX_DEPTH) return refuse("ss_mst_range_audit_scratch", "depth above 30");
  *bytes_out = mst_audit_scratch_bytes(depth);
  return SG_OK;
}
int ss_mst_range_audit_dev(const void* d_node_balances, uint32_t depth, uint32_t n_currencies, uint32_t n_bytes, void* d_node_flags,
                           void* d_leaf_reasons, void* d_bad_leaves, uint64_t bad_cap, void* d_scratch, uint64_t* summary_out,
                           void* stream) {
  const std::string problem = mst_audit_problem(d_node_balances, depth, n_currencies, n_bytes, d_node_flags, d_leaf_reasons, d_bad_leaves,
                                                bad_cap, d_scratch, summary_out);
  if (!problem.empty()) return refuse("ss_mst_range_audit", problem.c_str());
  uint32_t* work = static_cast<uint32_t*>(d_scratch);
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  CHECK_HIP(hipMemsetAsync(work, 0, 4 * MST_AUDIT_FRONT_WORDS, s), "ss_mst_range_audit: work space");
  CHECK_HIP(mst_audit_launch(d_node_balances, depth, n_currencies, n_bytes, static_cast<uint8_t*>(d_node_flags),
                             static_cast<uint32_t*>(d_leaf_reasons), static_cast<uint32_t*>(d_bad_leaves), bad_cap, work, s),
            "ss_mst_range_audit");
  uint32_t result[MST_AUDIT_FRONT_WORDS];
  TRY(download(reinterpret_cast<uint8_t*>(result), work, sizeof result, s));   // waits for the stream
  summary_out[0] = result[MST_AUDIT_AT_BAD_NODES];
  summary_out[1] = result[MST_AUDIT_AT_UNPROVABLE];
  summary_out[2] = summary_out[1] < bad_cap ? summary_out[1] : bad_cap;
  summary_out[3] = result[MST_AUDIT_AT_ROOT];
  return SG_OK;
}
// New balances for m leaves of a built tree, in place (mst.rs:169-204 for many leaves at once; witness.hip has the kernels).
// As above everything that can be wrong is found on the host first.  The geometry is the host's too (mst_update_plan.h): the
// parents to redo on every level, one launch per level, stream order the only barrier between levels.  One work space of the
// caller's stream holds the new balances as field elements (made from the digits by mst_balances_kernel), the digit offsets,
// the leaf indices followed by the plan's lists, then the digits.
int sg_mst_update_dev(const uint32_t* leaf_indices, const uint8_t* digit_bytes, const uint64_t* digit_off, size_t m, uint32_t depth,
                      uint32_t n_currencies, const void* d_usernames, void* d_leaf_balances, void* d_node_hashes, void* d_node_balances,
                      void* stream) {
  if (!leaf_indices || !digit_bytes || !digit_off || !d_usernames || !d_leaf_balances || !d_node_hashes || !d_node_balances)
    return fail(SG_ERR_INVALID, "sg_mst_update: null argument");
  if (const char* problem = shape_problem(n_currencies, depth)) return refuse("sg_mst_update", problem);
  const uint32_t nc = n_currencies;
  const size_t leaves = (size_t)1 << depth;
  {
    // the leaves' balances live twice, in their own array and as level 0 of the nodes': two allocations
    const uintptr_t lo_a = (uintptr_t)d_leaf_balances, hi_a = lo_a + 32 * leaves * nc;
    const uintptr_t lo_b = (uintptr_t)d_node_balances, hi_b = lo_b + 32 * (2 * leaves - 1) * nc;
    if (lo_a < hi_b && lo_b < hi_a) return fail(SG_ERR_INVALID, "sg_mst_update: d_leaf_balances overlaps d_node_balances");
  }
  const std::string problem = mst_update_problem(leaf_indices, digit_bytes, digit_off, m, depth, nc);
  if (!problem.empty()) return fail(SG_ERR_INVALID, ("sg_mst_update: " + problem).c_str());
  const MstUpdatePlan plan = mst_update_plan(leaf_indices, m, depth);
  std::vector<uint32_t> lists(leaf_indices, leaf_indices + m);   // the indices, then list 1 .. list depth: one copy
  lists.insert(lists.end(), plan.nodes.begin(), plan.nodes.end());
  const size_t fields = m * (size_t)nc, digit_len = digit_off[fields];
  const size_t at_digit_off = 32 * fields, at_lists = at_digit_off + 8 * (fields + 1), at_digits = at_lists + 4 * lists.size();
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  CHECK_HIP(g_ctx->witness.init(g_ctx->stream), "sg_mst_update: Poseidon table");
  uint8_t* d = nullptr;
  CHECK_HIP(scratch_for(s, 12, at_digits + digit_len, &d), "sg_mst_update: work space");
  CHECK_HIP(hipMemcpyAsync(d + at_digit_off, digit_off, 8 * (fields + 1), hipMemcpyHostToDevice, s), "sg_mst_update: digit offsets");
  CHECK_HIP(hipMemcpyAsync(d + at_lists, lists.data(), 4 * lists.size(), hipMemcpyHostToDevice, s), "sg_mst_update: lists");
  CHECK_HIP(hipMemcpyAsync(d + at_digits, digit_bytes, digit_len, hipMemcpyHostToDevice, s), "sg_mst_update: digits");
  fp_words* new_bal = reinterpret_cast<fp_words*>(d);
  const uint32_t* d_lists = reinterpret_cast<const uint32_t*>(d + at_lists);
  CHECK_HIP(mst_balances_launch(d + at_digits, reinterpret_cast<const uint64_t*>(d + at_digit_off), fields, new_bal, s),
            "sg_mst_update: balances");
  fp_words* h = static_cast<fp_words*>(d_node_hashes);
  fp_words* b = static_cast<fp_words*>(d_node_balances);
  CHECK_HIP(g_ctx->witness.leaves(d_lists, static_cast<const fp_words*>(d_usernames), new_bal, m, nc, h,
                                  static_cast<fp_words*>(d_leaf_balances), b, s),
            "sg_mst_update: leaves");
  for (uint32_t l = 1; l <= depth; l++) {
    const size_t child = mst_level_first(l - 1, depth), parent = mst_level_first(l, depth);
    CHECK_HIP(g_ctx->witness.level(d_lists + m + plan.offset[l - 1], h + child, b + child * nc, plan.count(l), nc, h + parent,
                                   b + parent * nc, s),
              "sg_mst_update: level");
  }
  return SG_OK;
}

// Circuit::synthesize on the device for users of a device-resident tree (witness.hip: the program is the floor plan)
int sg_mst_inclusion_witness_dev(const void* d_program, uint32_t n_items, uint32_t n_absorbs, const void* d_usernames,
                                 const void* d_node_hashes, const void* d_node_balances, uint32_t depth, uint32_t n_currencies,
                                 const void* d_user_indices, uint32_t n_users, void* d_advice, uint64_t rows, void* stream) {
  if (!d_program || !d_usernames || !d_node_hashes || !d_node_balances || !d_user_indices || !d_advice)
    return fail(SG_ERR_INVALID, "sg_mst_inclusion_witness: null argument");
  const bool sizes_ok = rows != 0 && rows <= (1ull << 28) && n_items <= (1u << 24) && n_users <= 65535;
  if (const char* problem = shape_problem(n_currencies, depth, sizes_ok)) return refuse("sg_mst_inclusion_witness", problem);
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  hipError_t e = g_ctx->witness.init(g_ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_advice, 0, (size_t)n_users * 3 * rows * 32, s);
  if (e == hipSuccess)
    e = g_ctx->witness.inclusion_witness(static_cast<const uint32_t*>(d_program), n_items, n_absorbs,
                                         static_cast<const fp_words*>(d_usernames), static_cast<const fp_words*>(d_node_hashes),
                                         static_cast<const fp_words*>(d_node_balances), depth, n_currencies,
                                         static_cast<const uint32_t*>(d_user_indices), n_users, static_cast<fp_words*>(d_advice),
                                         (size_t)rows, s);
  if (e != hipSuccess) return hip_fail("mst inclusion witness", e);
  return SG_OK;
}

}  // extern "C"
