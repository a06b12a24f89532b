// C ABI, one round of snapshots against the next (include/summa_rounds.h): the diff of a new file with a tree in HBM and the
// apply of its changed balances (mst_diff.h has the rules, the work space and the host mirror, mst_diff.cuh the kernels).
#include "abi_internal.h"
#include "../../include/summa_rounds.h"
#include "mst_diff.h"
#include "mst_update_plan.h"

using namespace sg;
namespace {
int refuse(const char* who, const std::string& problem) { return fail(SG_ERR_INVALID, (std::string(who) + ": " + problem).c_str()); }
}  // namespace

extern "C" {

int sr_mst_diff_scratch(uint64_t n_rows, uint32_t depth, uint64_t* bytes_out) {
  if (!bytes_out) return fail(SG_ERR_INVALID, "sr_mst_diff_scratch: null argument");
  if (n_rows == 0 || n_rows >= (1ull << 32)) return refuse("sr_mst_diff_scratch", "n_rows outside 1..2^32-1");
  if (depth > MST_AUDIT_MAX_DEPTH) return refuse("sr_mst_diff_scratch", "depth above 30");
  *bytes_out = mst_diff_scratch_bytes(n_rows, depth);
  return SG_OK;
}

// The split as sg_mst_csv_entries_dev does it, its problem word behind the spans: one 8-byte copy and the first wait.  Then the
// three memsets and twelve launches of mst_diff_launch, one 32-byte copy and the second wait.
int sr_mst_csv_diff_dev(const void* d_bytes, uint64_t len, uint64_t body_off, const void* d_tile_scratch, uint32_t delimiter,
                        uint32_t n_currencies, uint64_t n_rows, void* d_span_scratch, const void* d_tree_bytes, uint64_t tree_len,
                        uint64_t tree_body_off, const void* d_name_spans, const void* d_order, uint64_t n_tree, uint32_t depth,
                        const void* d_leaf_balances, void* d_row_leaf, void* d_row_state, void* d_leaf_state, void* d_owner, void* d_changed,
                        void* d_new_rows, void* d_gone, uint64_t cap, void* d_scratch, uint64_t* problem_out, uint64_t* summary_out,
                        void* stream) {
  MstDiffArgs a;
  a.b_bytes = d_bytes, a.b_tiles = d_tile_scratch, a.b_spans = d_span_scratch, a.t_bytes = d_tree_bytes, a.t_name_spans = d_name_spans;
  a.t_order = d_order, a.leaf_balances = d_leaf_balances, a.row_leaf = d_row_leaf, a.row_state = d_row_state, a.leaf_state = d_leaf_state;
  a.owner = d_owner, a.changed = d_changed, a.new_rows = d_new_rows, a.gone = d_gone, a.scratch = d_scratch, a.problem_out = problem_out;
  a.summary_out = summary_out, a.b_len = len, a.b_body_off = body_off, a.n_rows = n_rows, a.t_len = tree_len, a.t_body_off = tree_body_off;
  a.n_tree = n_tree, a.cap = cap, a.delimiter = delimiter, a.nc = n_currencies, a.depth = depth;
  const std::string problem = mst_diff_problem(a);
  if (!problem.empty()) return refuse("sr_mst_csv_diff", problem);
  const uint64_t body_len = len - body_off;
  const uint8_t* body = static_cast<const uint8_t*>(d_bytes) + body_off;
  uint64_t* words = static_cast<uint64_t*>(d_span_scratch);
  uint64_t* d_problem = words + mst_csv_span_words(n_rows, n_currencies);
  uint32_t* work = static_cast<uint32_t*>(d_scratch);
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  CHECK_HIP(mst_csv_split_launch(body, body_len, static_cast<const uint32_t*>(d_tile_scratch), (uint8_t)delimiter, n_currencies, n_rows, words,
                                 d_problem, s),
            "sr_mst_csv_diff: split");
  uint64_t found = 0;
  TRY(download(reinterpret_cast<uint8_t*>(&found), d_problem, sizeof found, s));   // waits for the stream
  *problem_out = found == MST_CSV_NO_PROBLEM ? 0 : found;
  if (*problem_out) return SG_OK;                            // the outputs stay unwritten
  CHECK_HIP(mst_diff_launch(body, body_len, words, n_rows, n_currencies, static_cast<const uint8_t*>(d_tree_bytes) + tree_body_off,
                            tree_len - tree_body_off, static_cast<const uint32_t*>(d_name_spans), static_cast<const uint32_t*>(d_order), n_tree,
                            depth, d_leaf_balances, static_cast<uint32_t*>(d_row_leaf), static_cast<uint8_t*>(d_row_state),
                            static_cast<uint8_t*>(d_leaf_state), static_cast<uint32_t*>(d_owner), static_cast<uint32_t*>(d_changed),
                            static_cast<uint32_t*>(d_new_rows), static_cast<uint32_t*>(d_gone), cap, work, s),
            "sr_mst_csv_diff");
  uint32_t result[MST_DIFF_FRONT_WORDS];
  TRY(download(reinterpret_cast<uint8_t*>(result), work, sizeof result, s));       // waits for the stream
  for (uint32_t k = 0; k <= MST_DIFF_SUM_UNREACHABLE; k++) summary_out[k] = result[k];
  summary_out[MST_DIFF_SUM_NEW_LISTED] = summary_out[MST_DIFF_SUM_NEW] < cap ? summary_out[MST_DIFF_SUM_NEW] : cap;
  summary_out[MST_DIFF_SUM_GONE_LISTED] = summary_out[MST_DIFF_SUM_GONE] < cap ? summary_out[MST_DIFF_SUM_GONE] : cap;
  return SG_OK;
}

// One work space of the caller's stream holds the new balances as field elements (made from the file's text by the pack kernel),
// then the plan's lists; the changed leaves themselves are read where the diff left them.
int sr_mst_apply_diff_dev(const void* d_bytes, uint64_t len, uint64_t body_off, const void* d_span_scratch, uint64_t n_rows,
                          const void* d_owner, const void* d_changed, uint64_t n_changed, uint32_t depth, uint32_t n_currencies,
                          const void* d_usernames, void* d_leaf_balances, void* d_node_hashes, void* d_node_balances, void* stream) {
  const std::string problem = mst_diff_apply_problem(d_bytes, len, body_off, d_span_scratch, n_rows, d_owner, d_changed, n_changed, depth,
                                                     n_currencies, d_usernames, d_leaf_balances, d_node_hashes, d_node_balances);
  if (!problem.empty()) return refuse("sr_mst_apply_diff", problem);
  const uint32_t nc = n_currencies;
  const size_t leaves = (size_t)1 << depth, m = (size_t)n_changed;
  {
    // the leaves' balances live twice, in their own array and as level 0 of the nodes': two allocations
    const uintptr_t lo_a = (uintptr_t)d_leaf_balances, hi_a = lo_a + 32 * leaves * nc;
    const uintptr_t lo_b = (uintptr_t)d_node_balances, hi_b = lo_b + 32 * (2 * leaves - 1) * nc;
    if (lo_a < hi_b && lo_b < hi_a) return fail(SG_ERR_INVALID, "sr_mst_apply_diff: d_leaf_balances overlaps d_node_balances");
  }
  if (m == 0) return SG_OK;
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  std::vector<uint32_t> changed(m);
  TRY(download(reinterpret_cast<uint8_t*>(changed.data()), d_changed, 4 * m, s));   // waits for the stream
  for (size_t j = 0; j < m; j++) {
    if (changed[j] >= leaves) return refuse("sr_mst_apply_diff", "changed leaf at position " + std::to_string(j) + " is out of range");
    if (j && changed[j] <= changed[j - 1]) return refuse("sr_mst_apply_diff", "changed leaves do not strictly increase at position " + std::to_string(j));
  }
  const MstUpdatePlan plan = mst_update_plan(changed.data(), m, depth);
  const size_t fields = m * (size_t)nc, at_lists = 32 * fields;
  CHECK_HIP(g_ctx->witness.init(g_ctx->stream), "sr_mst_apply_diff: Poseidon table");
  uint8_t* d = nullptr;
  CHECK_HIP(scratch_for(s, 15, at_lists + 4 * plan.nodes.size() + 4, &d), "sr_mst_apply_diff: work space");
  if (!plan.nodes.empty())
    CHECK_HIP(hipMemcpyAsync(d + at_lists, plan.nodes.data(), 4 * plan.nodes.size(), hipMemcpyHostToDevice, s), "sr_mst_apply_diff: lists");
  fp_words* new_bal = reinterpret_cast<fp_words*>(d);
  const uint32_t* d_lists = reinterpret_cast<const uint32_t*>(d + at_lists);
  CHECK_HIP(mst_diff_pack_launch(static_cast<const uint8_t*>(d_bytes) + body_off, len - body_off, static_cast<const uint64_t*>(d_span_scratch),
                                 n_rows, nc, static_cast<const uint32_t*>(d_owner), static_cast<const uint32_t*>(d_changed), m, depth, new_bal, s),
            "sr_mst_apply_diff: pack");
  fp_words* h = static_cast<fp_words*>(d_node_hashes);
  fp_words* b = static_cast<fp_words*>(d_node_balances);
  CHECK_HIP(g_ctx->witness.leaves(static_cast<const uint32_t*>(d_changed), static_cast<const fp_words*>(d_usernames), new_bal, m, nc, h,
                                  static_cast<fp_words*>(d_leaf_balances), b, s),
            "sr_mst_apply_diff: leaves");
  for (uint32_t l = 1; l <= depth; l++) {
    const size_t child = mst_level_first(l - 1, depth), parent = mst_level_first(l, depth);
    CHECK_HIP(g_ctx->witness.level(d_lists + plan.offset[l - 1], h + child, b + child * nc, plan.count(l), nc, h + parent, b + parent * nc, s),
              "sr_mst_apply_diff: level");
  }
  return SG_OK;
}

}  // extern "C"
