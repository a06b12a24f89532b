// C ABI, a round settled in full on a tree in HBM (include/summa_admit.h): the measure of the names the NEW rows of a diff add, and
// the settle that admits them into the tree's padding, extends the name index, zeroes the GONE leaves and re-hashes the union of
// CHANGED, GONE and admitted leaves in one run (mst_admit.h has the rules, the work space and the host mirror, mst_admit.cuh the
// kernels).
#include "abi_internal.h"
#include "../../include/summa_admit.h"
#include "mst_admit.h"
#include "mst_update_plan.h"

using namespace sg;
namespace {
int refuse(const char* who, const std::string& problem) { return fail(SG_ERR_INVALID, (std::string(who) + ": " + problem).c_str()); }
}  // namespace

extern "C" {

int sa_mst_admit_scratch(uint64_t n_rows, uint32_t n_currencies, uint64_t n_new, uint64_t* bytes_out) {
  if (!bytes_out) return fail(SG_ERR_INVALID, "sa_mst_admit_scratch: null argument");
  if (n_rows == 0 || n_rows >= (1ull << 32)) return refuse("sa_mst_admit_scratch", "n_rows outside 1..2^32-1");
  if (n_currencies == 0 || n_currencies > 64) return refuse("sa_mst_admit_scratch", "n_currencies outside 1..64");
  if (n_new == 0 || n_new > n_rows) return refuse("sa_mst_admit_scratch", "n_new outside 1..n_rows");
  *bytes_out = mst_admit_scratch_bytes(n_rows, n_currencies, n_new);
  return SG_OK;
}

// Two small memsets and four launches (the sort's lengths, the admitted names' lengths, the audit's groups, the export's offsets),
// one 32-byte copy and the call's only wait; then, without a problem, the sort's passes and the three launches of the sorted NEW
// list are enqueued and the call returns.
int sa_mst_admit_measure_dev(const void* d_bytes, uint64_t len, uint64_t body_off, const void* d_span_scratch, uint64_t n_rows,
                             uint32_t n_currencies, const void* d_row_state, const void* d_new_rows, uint64_t n_new, uint64_t n_tree,
                             uint32_t depth, void* d_scratch, uint64_t* name_bytes_out, uint64_t* problem_out, void* stream) {
  const std::string problem = mst_admit_measure_problem(d_bytes, len, body_off, d_span_scratch, n_rows, n_currencies, d_row_state, d_new_rows,
                                                        n_new, n_tree, depth, d_scratch, name_bytes_out, problem_out);
  if (!problem.empty()) return refuse("sa_mst_admit_measure", problem);
  const uint64_t body_len = len - body_off;
  const uint8_t* body = static_cast<const uint8_t*>(d_bytes) + body_off;
  const uint64_t* words = static_cast<const uint64_t*>(d_span_scratch);
  uint32_t* work = static_cast<uint32_t*>(d_scratch);
  uint32_t* sort_work = work + mst_admit_at_sort();
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  CHECK_HIP(hipMemsetAsync(work, 0, 4 * (MST_ADMIT_FRONT_WORDS + MST_SORT_FRONT_WORDS), s), "sa_mst_admit_measure: work space");
  CHECK_HIP(hipMemsetAsync(sort_work + MST_SORT_AT_PROBLEM, 0xff, 8, s), "sa_mst_admit_measure: problem word");   // MST_CSV_NO_PROBLEM
  CHECK_HIP(mst_sort_lengths_launch(words, n_rows, n_currencies, sort_work, s), "sa_mst_admit_measure: lengths");
  CHECK_HIP(mst_admit_measure_launch(words, n_rows, n_currencies, body_len, static_cast<const uint32_t*>(d_new_rows), n_new, work, s),
            "sa_mst_admit_measure: names");
  uint32_t result[MST_ADMIT_RESULT_WORDS];
  TRY(download(reinterpret_cast<uint8_t*>(result), work, sizeof result, s));       // waits for the stream
  const uint32_t* front = result + MST_ADMIT_FRONT_WORDS;
  const uint64_t found = (uint64_t)front[MST_SORT_AT_PROBLEM] | (uint64_t)front[MST_SORT_AT_PROBLEM + 1] << 32;
  *problem_out = found == MST_CSV_NO_PROBLEM ? 0 : found;
  *name_bytes_out = (uint64_t)result[MST_ADMIT_AT_TOTAL] | (uint64_t)result[MST_ADMIT_AT_TOTAL + 1] << 32;
  if (*problem_out) return SG_OK;                            // nothing more is enqueued
  CHECK_HIP(mst_sort_launch(body, words, n_rows, n_currencies, front[MST_SORT_AT_LONGEST], sort_work, work + mst_admit_at_order(n_rows),
                            work + mst_admit_at_spans(n_rows), reinterpret_cast<uint64_t*>(work + mst_admit_at_sorted_words(n_rows, n_new)), s),
            "sa_mst_admit_measure: sort");
  CHECK_HIP(mst_admit_list_launch(static_cast<const uint8_t*>(d_row_state), n_rows, n_new, work, s), "sa_mst_admit_measure: list");
  return SG_OK;
}

// One work space of the caller's stream holds the union's balances as field elements (made from the file's text by the pack
// kernel), then the union and the plan's lists.
int sa_mst_settle_dev(const void* d_bytes, uint64_t len, uint64_t body_off, const void* d_span_scratch, uint64_t n_rows, uint32_t n_currencies,
                      const void* d_owner, const void* d_leaf_state, const void* d_changed, uint64_t n_changed, const void* d_gone,
                      uint64_t n_gone, const void* d_new_rows, uint64_t n_new, const void* d_scratch, const void* d_tree_bytes,
                      uint64_t tree_len, uint64_t tree_body_off, const void* d_name_spans, const void* d_order, const void* d_leaf_name_spans,
                      uint64_t n_tree, uint32_t depth, void* d_tree_bytes_out, uint64_t name_bytes, void* d_name_spans_out, void* d_order_out,
                      void* d_leaf_name_spans_out, void* d_usernames, void* d_leaf_balances, void* d_node_hashes, void* d_node_balances,
                      void* stream) {
  MstSettleArgs a;
  a.b_bytes = d_bytes, a.b_spans = d_span_scratch, a.owner = d_owner, a.leaf_state = d_leaf_state, a.changed = d_changed, a.gone = d_gone;
  a.new_rows = d_new_rows, a.scratch = d_scratch, a.t_bytes = d_tree_bytes, a.t_name_spans = d_name_spans, a.t_order = d_order;
  a.t_leaf_name_spans = d_leaf_name_spans, a.out_bytes = d_tree_bytes_out, a.out_name_spans = d_name_spans_out, a.out_order = d_order_out;
  a.out_leaf_name_spans = d_leaf_name_spans_out, a.usernames = d_usernames, a.leaf_balances = d_leaf_balances, a.node_hashes = d_node_hashes;
  a.node_balances = d_node_balances, a.b_len = len, a.b_body_off = body_off, a.n_rows = n_rows, a.n_changed = n_changed, a.n_gone = n_gone;
  a.n_new = n_new, a.t_len = tree_len, a.t_body_off = tree_body_off, a.n_tree = n_tree, a.name_bytes = name_bytes, a.nc = n_currencies;
  a.depth = depth;
  const std::string problem = mst_settle_problem(a);
  if (!problem.empty()) return refuse("sa_mst_settle", problem);
  const uint32_t nc = n_currencies;
  const size_t leaves = (size_t)1 << depth;
  {
    // the leaves' balances live twice, in their own array and as level 0 of the nodes': two allocations
    const uintptr_t lo_a = (uintptr_t)d_leaf_balances, hi_a = lo_a + 32 * leaves * nc;
    const uintptr_t lo_b = (uintptr_t)d_node_balances, hi_b = lo_b + 32 * (2 * leaves - 1) * nc;
    if (lo_a < hi_b && lo_b < hi_a) return fail(SG_ERR_INVALID, "sa_mst_settle: d_leaf_balances overlaps d_node_balances");
  }
  const size_t m = (size_t)(n_changed + n_gone + n_new);
  if (m == 0) return SG_OK;
  const uint64_t body_len = len - body_off;
  const uint8_t* body = static_cast<const uint8_t*>(d_bytes) + body_off;
  const uint64_t* words = static_cast<const uint64_t*>(d_span_scratch);
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  std::vector<uint32_t> changed(n_changed), gone(n_gone), lists;
  if (n_changed) TRY(download(reinterpret_cast<uint8_t*>(changed.data()), d_changed, 4 * n_changed, s));   // waits for the stream
  if (n_gone) TRY(download(reinterpret_cast<uint8_t*>(gone.data()), d_gone, 4 * n_gone, s));
  const std::string bad = mst_admit_union(changed.data(), n_changed, gone.data(), n_gone, n_tree, n_new, &lists);
  if (!bad.empty()) return refuse("sa_mst_settle", bad);       // nothing is written
  const MstUpdatePlan plan = mst_update_plan(lists.data(), m, depth);
  lists.insert(lists.end(), plan.nodes.begin(), plan.nodes.end());   // the union, then list 1 .. list depth: one copy
  const size_t fields = m * (size_t)nc, at_lists = 32 * fields;
  CHECK_HIP(g_ctx->witness.init(g_ctx->stream), "sa_mst_settle: Poseidon table");
  uint8_t* d = nullptr;
  CHECK_HIP(scratch_for(s, 16, at_lists + 4 * lists.size(), &d), "sa_mst_settle: work space");
  CHECK_HIP(hipMemcpyAsync(d + at_lists, lists.data(), 4 * lists.size(), hipMemcpyHostToDevice, s), "sa_mst_settle: lists");
  if (n_new) {
    const uint64_t body_t_len = tree_len - tree_body_off;
    uint8_t* out = static_cast<uint8_t*>(d_tree_bytes_out);
    CHECK_HIP(hipMemcpyAsync(out, d_tree_bytes, tree_len, hipMemcpyDeviceToDevice, s), "sa_mst_settle: text");
    CHECK_HIP(hipMemcpyAsync(d_leaf_name_spans_out, d_leaf_name_spans, 8 * n_tree, hipMemcpyDeviceToDevice, s), "sa_mst_settle: leaf spans");
    CHECK_HIP(mst_admit_merge_launch(body, body_len, words, n_rows, nc, static_cast<const uint32_t*>(d_new_rows), n_new,
                                     static_cast<const uint32_t*>(d_scratch), static_cast<const uint8_t*>(d_tree_bytes) + tree_body_off,
                                     body_t_len, static_cast<const uint32_t*>(d_name_spans), static_cast<const uint32_t*>(d_order), n_tree, depth,
                                     out + tree_body_off, name_bytes, static_cast<uint32_t*>(d_name_spans_out),
                                     static_cast<uint32_t*>(d_order_out), static_cast<uint32_t*>(d_leaf_name_spans_out), d_usernames, s),
              "sa_mst_settle: merge");
  }
  fp_words* new_bal = reinterpret_cast<fp_words*>(d);
  const uint32_t* d_lists = reinterpret_cast<const uint32_t*>(d + at_lists);
  CHECK_HIP(mst_admit_pack_launch(body, body_len, words, n_rows, nc, static_cast<const uint32_t*>(d_owner),
                                  static_cast<const uint8_t*>(d_leaf_state), static_cast<const uint32_t*>(d_new_rows), n_new, n_tree, d_lists, m,
                                  depth, new_bal, s),
            "sa_mst_settle: pack");
  fp_words* h = static_cast<fp_words*>(d_node_hashes);
  fp_words* b = static_cast<fp_words*>(d_node_balances);
  CHECK_HIP(g_ctx->witness.leaves(d_lists, static_cast<const fp_words*>(d_usernames), new_bal, m, nc, h,
                                  static_cast<fp_words*>(d_leaf_balances), b, s),
            "sa_mst_settle: leaves");
  for (uint32_t l = 1; l <= depth; l++) {
    const size_t child = mst_level_first(l - 1, depth), parent = mst_level_first(l, depth);
    CHECK_HIP(g_ctx->witness.level(d_lists + m + plan.offset[l - 1], h + child, b + child * nc, plan.count(l), nc, h + parent, b + parent * nc, s),
              "sa_mst_settle: level");
  }
  return SG_OK;
}

}  // extern "C"
