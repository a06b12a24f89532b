// C ABI, a tree in HBM written back out as its snapshot CSV (include/summa_export.h): the rows' lengths and positions, then the
// bytes (mst_export.h has the rules, the work space and the host mirror, mst_export.cuh the kernels).
#include "abi_internal.h"
#include "../../include/summa_export.h"
#include "mst_export.h"

using namespace sg;
namespace {
int refuse(const char* who, const std::string& problem) { return fail(SG_ERR_INVALID, (std::string(who) + ": " + problem).c_str()); }
}  // namespace

extern "C" {

int sx_mst_csv_scratch(uint64_t n_rows, uint64_t* bytes_out) {
  if (!bytes_out) return fail(SG_ERR_INVALID, "sx_mst_csv_scratch: null argument");
  if (n_rows == 0 || n_rows >= (1ull << 32)) return refuse("sx_mst_csv_scratch", "n_rows outside 1..2^32-1");
  *bytes_out = mst_export_scratch_bytes(n_rows);
  return SG_OK;
}

// Three launches, one 8-byte copy and the only wait.
int sx_mst_csv_measure_dev(const void* d_tree_bytes, uint64_t tree_len, uint64_t tree_body_off, const void* d_leaf_name_spans, uint64_t n_rows,
                           uint32_t n_currencies, const void* d_leaf_balances, void* d_row_off, void* d_scratch, uint64_t* body_bytes_out,
                           void* stream) {
  const std::string problem = mst_export_measure_problem(d_tree_bytes, tree_len, tree_body_off, d_leaf_name_spans, n_rows, n_currencies,
                                                         d_leaf_balances, d_row_off, d_scratch, body_bytes_out);
  if (!problem.empty()) return refuse("sx_mst_csv_measure", problem);
  uint32_t* work = static_cast<uint32_t*>(d_scratch);
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  CHECK_HIP(mst_export_measure_launch(static_cast<const uint8_t*>(d_tree_bytes) + tree_body_off, tree_len - tree_body_off,
                                      static_cast<const uint32_t*>(d_leaf_name_spans), n_rows, n_currencies, d_leaf_balances,
                                      static_cast<uint32_t*>(d_row_off), work, s),
            "sx_mst_csv_measure");
  uint32_t total[2] = {0, 0};
  TRY(download(reinterpret_cast<uint8_t*>(total), work + MST_EXPORT_AT_TOTAL, sizeof total, s));   // waits for the stream
  *body_bytes_out = (uint64_t)total[0] | ((uint64_t)total[1] << 32);
  return SG_OK;
}

// One launch, no wait.
int sx_mst_csv_write_dev(const void* d_tree_bytes, uint64_t tree_len, uint64_t tree_body_off, const void* d_leaf_name_spans, uint64_t n_rows,
                         uint32_t n_currencies, const void* d_leaf_balances, uint32_t delimiter, const void* d_row_off, uint64_t body_bytes,
                         void* d_out, void* stream) {
  const std::string problem = mst_export_write_problem(d_tree_bytes, tree_len, tree_body_off, d_leaf_name_spans, n_rows, n_currencies,
                                                       d_leaf_balances, delimiter, d_row_off, body_bytes, d_out);
  if (!problem.empty()) return refuse("sx_mst_csv_write", problem);
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  CHECK_HIP(mst_export_write_launch(static_cast<const uint8_t*>(d_tree_bytes) + tree_body_off, tree_len - tree_body_off,
                                    static_cast<const uint32_t*>(d_leaf_name_spans), n_rows, n_currencies, d_leaf_balances, (uint8_t)delimiter,
                                    static_cast<const uint32_t*>(d_row_off), body_bytes, static_cast<uint8_t*>(d_out), s),
            "sx_mst_csv_write");
  return SG_OK;
}

}  // extern "C"
