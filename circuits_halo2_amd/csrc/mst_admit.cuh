// A round settled in full on a tree in HBM (included once by mst_entries.hip, behind the export: mst_admit.h has the rules, the
// work space and the host mirror).  The file's text, its spans, the diff's arrays and the tree's old text and index are read
// only.  The kernels that count by ballot or scan a wave's lengths keep all their lanes to the end, every load is guarded by the
// sizes the kernel is given, every span is cut to its text and every store is guarded by its buffer's length.  The two merges
// are a binary search per thread through two gathers a step, as the diff's match: a thread per name and as many waves in flight
// as the device takes.
#pragma once
#include "mst_admit.h"
#include "mst_export.cuh"   // mst_audit_groups_kernel behind it: the scan of the tile words

namespace sg {

static_assert(MST_ADMIT_TILE == 64, "a tile is a wave: its count is one ballot, its sum one reduction over the lanes");
static_assert(MST_ADMIT_TILE == MST_AUDIT_TILE && MST_ADMIT_GROUP == MST_AUDIT_GROUP && MST_ADMIT_THREADS == MST_AUDIT_THREADS,
              "the groups step is the audit's kernel");

// lengths, an admitted leaf per thread (the j-th NEW row in file order): its name's cut length into place[j], the wave's sum into
// tile_sum[tile], and j into the rank of its row
__global__ void __launch_bounds__(MST_ADMIT_THREADS) mst_admit_lengths_kernel(const uint64_t* __restrict__ name_begin,
                                                                            const uint64_t* __restrict__ name_end, uint32_t n_rows,
                                                                            uint64_t body_b_len, const uint32_t* __restrict__ new_rows,
                                                                            uint32_t m, uint32_t* __restrict__ place,
                                                                            uint32_t* __restrict__ rank, uint32_t* __restrict__ tile_sum) {
  side_kernel_prio();
  const uint64_t at = (uint64_t)blockIdx.x * MST_ADMIT_THREADS + threadIdx.x;
  uint32_t len = 0;
  if (at < m) {
    const uint32_t row = new_rows[at];
    uint64_t b, e;
    mst_admit_row_name(name_begin, name_end, n_rows, row, body_b_len, &b, &e);
    len = (uint32_t)(e - b);
    place[at] = len;
    if (row < n_rows) rank[row] = (uint32_t)at;
  }
  uint32_t sum = len;
#pragma unroll
  for (uint32_t off = 32; off; off >>= 1) sum += __shfl_xor(sum, off);
  const uint64_t tile = at / MST_ADMIT_TILE;
  if ((threadIdx.x & 63) == 0 && tile < mst_diff_tiles(m)) tile_sum[tile] = sum;
}

// marks, a sorted position of B per thread: tile_count[tile] = the wave's positions whose row is NEW
__global__ void __launch_bounds__(MST_ADMIT_THREADS) mst_admit_marks_kernel(const uint8_t* __restrict__ row_state,
                                                                          const uint32_t* __restrict__ order, uint32_t n_rows,
                                                                          uint32_t* __restrict__ tile_count) {
  side_kernel_prio();
  const uint64_t at = (uint64_t)blockIdx.x * MST_ADMIT_THREADS + threadIdx.x;
  bool hit = false;
  if (at < n_rows) {
    const uint32_t row = order[at];
    hit = row < n_rows && row_state[row] == MST_DIFF_ROW_NEW;
  }
  const uint32_t count = (uint32_t)__popcll(__ballot(hit));
  const uint64_t tile = at / MST_ADMIT_TILE;
  if ((threadIdx.x & 63) == 0 && tile < mst_diff_tiles(n_rows)) tile_count[tile] = count;
}

// scatter, a sorted position of B per thread: the row of a marked position goes to its place in the sorted NEW list -- the totals
// of the groups before its own, its tile's prefix and the lanes below it in the wave's ballot, data alone
__global__ void __launch_bounds__(MST_ADMIT_THREADS) mst_admit_scatter_kernel(const uint8_t* __restrict__ row_state,
                                                                            const uint32_t* __restrict__ order, uint32_t n_rows,
                                                                            const uint32_t* __restrict__ tile_count,
                                                                            const uint32_t* __restrict__ group_total,
                                                                            uint32_t* __restrict__ list, uint32_t m) {
  side_kernel_prio();
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t at = (uint64_t)blockIdx.x * MST_ADMIT_THREADS + threadIdx.x;
  const uint32_t tile = (uint32_t)(at / MST_ADMIT_TILE), groups = mst_diff_groups(n_rows);
  const uint32_t group = tile / MST_ADMIT_GROUP;
  uint32_t row = MST_DIFF_ABSENT;
  if (at < n_rows) row = order[at];
  const bool listed = row < n_rows && row_state[row] == MST_DIFF_ROW_NEW;
  const uint64_t peers = __ballot(listed);
  const uint32_t upto = group < groups ? group : groups;
  uint32_t before = 0;
  for (uint32_t g = lane; g < upto; g += 64) before += group_total[g];
#pragma unroll
  for (uint32_t off = 32; off; off >>= 1) before += __shfl_xor(before, off);
  if (listed) {                                                // at < n_rows: tile < tiles
    const uint64_t to = (uint64_t)before + tile_count[tile] + (uint32_t)__popcll(peers & (((uint64_t)1 << lane) - 1));
    if (to < m) list[to] = row;
  }
}

// merge, the sorted NEW list: the k-th name goes to position k + (old sorted names below it); its leaf is n_tree + the rank of its
// row, its span the place of its copy behind the old text
__global__ void __launch_bounds__(MST_ADMIT_THREADS) mst_admit_merge_new_kernel(const uint8_t* __restrict__ body_b, uint64_t body_b_len,
                                                                              const uint64_t* __restrict__ name_begin,
                                                                              const uint64_t* __restrict__ name_end, uint32_t n_rows,
                                                                              const uint32_t* __restrict__ list,
                                                                              const uint32_t* __restrict__ rank,
                                                                              const uint32_t* __restrict__ place, uint32_t m,
                                                                              const uint8_t* __restrict__ body_t, uint64_t body_t_len,
                                                                              const uint32_t* __restrict__ name_spans, uint32_t n_tree,
                                                                              uint32_t* __restrict__ order_out,
                                                                              uint32_t* __restrict__ name_spans_out) {
  side_kernel_prio();
  const uint64_t k = (uint64_t)blockIdx.x * MST_ADMIT_THREADS + threadIdx.x;
  if (k >= m) return;
  const uint32_t row = list[k];
  if (row >= n_rows) return;
  const uint32_t j = rank[row];
  if (j >= m) return;
  uint64_t b, e;
  mst_admit_row_name(name_begin, name_end, n_rows, row, body_b_len, &b, &e);
  const uint64_t to = k + mst_admit_tree_below(body_t, body_t_len, name_spans, n_tree, body_b + b, e - b);
  if (to >= (uint64_t)n_tree + m) return;
  const uint64_t begin = body_t_len + place[j];
  order_out[to] = n_tree + j;
  name_spans_out[2 * to] = (uint32_t)begin;
  name_spans_out[2 * to + 1] = (uint32_t)(begin + (e - b));
}

// merge, the tree's sorted names: position i goes to i + (sorted NEW names below its name), with its leaf and its span
__global__ void __launch_bounds__(MST_ADMIT_THREADS) mst_admit_merge_old_kernel(const uint8_t* __restrict__ body_b, uint64_t body_b_len,
                                                                              const uint64_t* __restrict__ name_begin,
                                                                              const uint64_t* __restrict__ name_end, uint32_t n_rows,
                                                                              const uint32_t* __restrict__ list, uint32_t m,
                                                                              const uint8_t* __restrict__ body_t, uint64_t body_t_len,
                                                                              const uint32_t* __restrict__ name_spans,
                                                                              const uint32_t* __restrict__ order, uint32_t n_tree,
                                                                              uint32_t* __restrict__ order_out,
                                                                              uint32_t* __restrict__ name_spans_out) {
  side_kernel_prio();
  const uint64_t i = (uint64_t)blockIdx.x * MST_ADMIT_THREADS + threadIdx.x;
  if (i >= n_tree) return;
  uint64_t b, e;
  mst_names_span(name_spans, body_t_len, (uint32_t)i, &b, &e);
  const uint64_t to = i + mst_admit_list_below(body_b, body_b_len, name_begin, name_end, n_rows, list, m, body_t + b, e - b);
  if (to >= (uint64_t)n_tree + m) return;
  order_out[to] = order[i];
  name_spans_out[2 * to] = name_spans[2 * i];
  name_spans_out[2 * to + 1] = name_spans[2 * i + 1];
}

// names, an admitted leaf per thread: its name's bytes behind the old text, its leaf span, and its username as the reader's
// mst_usernames_kernel makes it (keccak256 of the name, folded into the field)
__global__ void __launch_bounds__(MST_ENTRIES_BLOCK) mst_admit_names_kernel(const uint8_t* __restrict__ body_b, uint64_t body_b_len,
                                                                          const uint64_t* __restrict__ name_begin,
                                                                          const uint64_t* __restrict__ name_end, uint32_t n_rows,
                                                                          const uint32_t* __restrict__ new_rows,
                                                                          const uint32_t* __restrict__ place, uint32_t m, uint32_t n_tree,
                                                                          uint32_t leaves, uint64_t body_t_len, uint64_t body_out_len,
                                                                          uint8_t* __restrict__ body_out,
                                                                          uint32_t* __restrict__ leaf_name_spans_out,
                                                                          fp_words* __restrict__ users) {
  side_kernel_prio();
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m || n_tree + j >= leaves) return;
  uint64_t b, e;
  mst_admit_row_name(name_begin, name_end, n_rows, new_rows[j], body_b_len, &b, &e);
  const uint64_t to = body_t_len + place[j];
  for (uint64_t k = b; k < e; k++)
    if (to + (k - b) < body_out_len) body_out[to + (k - b)] = body_b[k];
  leaf_name_spans_out[2 * (n_tree + j)] = (uint32_t)to;
  leaf_name_spans_out[2 * (n_tree + j) + 1] = (uint32_t)(to + (e - b));
  uint64_t digest[4];
  keccak256_lanes(body_b + b, (size_t)(e - b), digest);
  uint32_t w[8];
  mst_username_words(digest, w);
  fp_words_store(users + n_tree + j, w);
}

// pack, a leaf of the union and a currency per thread: the source row's balance text folded into the field element the update
// takes, or zero
__global__ void __launch_bounds__(MST_ADMIT_THREADS) mst_admit_pack_kernel(const uint8_t* __restrict__ body_b, uint64_t body_b_len,
                                                                         const uint64_t* __restrict__ bal_begin,
                                                                         const uint64_t* __restrict__ bal_end, uint32_t n_rows, uint32_t nc,
                                                                         const uint32_t* __restrict__ owner,
                                                                         const uint8_t* __restrict__ leaf_state,
                                                                         const uint32_t* __restrict__ new_rows, uint32_t n_new,
                                                                         uint32_t n_tree, const uint32_t* __restrict__ leaves,
                                                                         uint64_t fields, uint32_t depth, fp_words* __restrict__ packed) {
  side_kernel_prio();
  const uint64_t t = (uint64_t)blockIdx.x * MST_ADMIT_THREADS + threadIdx.x;
  if (t >= fields) return;
  const uint32_t leaf = leaves[t / nc], c = (uint32_t)(t % nc);
  uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const uint32_t row = mst_admit_source_row(leaf, depth, n_tree, n_new, new_rows, leaf_state, owner, n_rows);
  if (row != MST_DIFF_ABSENT) {
    uint64_t b, e;
    mst_diff_span(bal_begin, bal_end, (uint64_t)row * nc + c, body_b_len, &b, &e);
    mst_decimal_words(body_b + b, (size_t)(e - b), w);
  }
  fp_words_store(packed + t, w);
}

static unsigned admit_blocks(uint64_t threads) { return (unsigned)((threads + MST_ADMIT_THREADS - 1) / MST_ADMIT_THREADS); }

hipError_t mst_admit_measure_launch(const uint64_t* d_words, uint64_t n_rows, uint32_t nc, uint64_t body_b_len, const uint32_t* d_new_rows,
                                    uint64_t n_new, uint32_t* d_work, hipStream_t stream) {
  if (n_rows == 0 || n_rows >= (1ull << 32) || nc == 0 || nc > 64 || n_new == 0 || n_new > n_rows) return hipErrorInvalidValue;
  const MstCsvSpans s = mst_csv_spans(const_cast<uint64_t*>(d_words), n_rows, nc);
  const uint32_t m = (uint32_t)n_new;
  uint32_t *place = d_work + mst_admit_at_places(n_rows, n_new), *rank = d_work + mst_admit_at_rank(n_rows);
  uint32_t *tile_sum = d_work + mst_admit_at_text_scan(n_rows, n_new), *group_total = tile_sum + mst_diff_tiles(n_new);
  mst_admit_lengths_kernel<<<admit_blocks(n_new), MST_ADMIT_THREADS, 0, stream>>>(s.name_begin, s.name_end, (uint32_t)n_rows, body_b_len,
                                                                              d_new_rows, m, place, rank, tile_sum);
  mst_audit_groups_kernel<<<mst_diff_groups(n_new), MST_AUDIT_THREADS, 0, stream>>>(tile_sum, mst_diff_tiles(n_new), group_total);
  // the export's offsets over the same geometry: a length becomes a place, the first wave leaves the total
  mst_export_offsets_kernel<<<admit_blocks(n_new), MST_EXPORT_THREADS, 0, stream>>>(place, m, tile_sum, group_total, d_work + MST_ADMIT_AT_TOTAL);
  return hipGetLastError();
}

hipError_t mst_admit_list_launch(const uint8_t* d_row_state, uint64_t n_rows, uint64_t n_new, uint32_t* d_work, hipStream_t stream) {
  if (n_rows == 0 || n_rows >= (1ull << 32) || n_new == 0 || n_new > n_rows) return hipErrorInvalidValue;
  const uint32_t* order = d_work + mst_admit_at_order(n_rows);
  uint32_t *tile_count = d_work + mst_admit_at_list_scan(n_rows, n_new), *group_total = tile_count + mst_diff_tiles(n_rows);
  uint32_t* list = d_work + mst_admit_at_list(n_rows);
  mst_admit_marks_kernel<<<admit_blocks(n_rows), MST_ADMIT_THREADS, 0, stream>>>(d_row_state, order, (uint32_t)n_rows, tile_count);
  mst_audit_groups_kernel<<<mst_diff_groups(n_rows), MST_AUDIT_THREADS, 0, stream>>>(tile_count, mst_diff_tiles(n_rows), group_total);
  mst_admit_scatter_kernel<<<admit_blocks(n_rows), MST_ADMIT_THREADS, 0, stream>>>(d_row_state, order, (uint32_t)n_rows, tile_count, group_total,
                                                                               list, (uint32_t)n_new);
  return hipGetLastError();
}

hipError_t mst_admit_merge_launch(const uint8_t* d_body_b, uint64_t body_b_len, const uint64_t* d_words, uint64_t n_rows, uint32_t nc,
                                  const uint32_t* d_new_rows, uint64_t n_new, const uint32_t* d_work, const uint8_t* d_body_t,
                                  uint64_t body_t_len, const uint32_t* d_name_spans, const uint32_t* d_order, uint64_t n_tree, uint32_t depth,
                                  uint8_t* d_body_out, uint64_t name_bytes, uint32_t* d_name_spans_out, uint32_t* d_order_out,
                                  uint32_t* d_leaf_name_spans_out, void* d_users, hipStream_t stream) {
  if (n_rows == 0 || n_rows >= (1ull << 32) || nc == 0 || nc > 64 || n_new == 0 || n_new > n_rows || depth > MST_AUDIT_MAX_DEPTH ||
      n_tree == 0 || n_tree + n_new > ((uint64_t)1 << depth) || body_t_len + name_bytes >= (1ull << 32))
    return hipErrorInvalidValue;
  const MstCsvSpans s = mst_csv_spans(const_cast<uint64_t*>(d_words), n_rows, nc);
  const uint32_t n = (uint32_t)n_rows, m = (uint32_t)n_new, nt = (uint32_t)n_tree;
  const uint32_t *list = d_work + mst_admit_at_list(n_rows), *rank = d_work + mst_admit_at_rank(n_rows);
  const uint32_t* place = d_work + mst_admit_at_places(n_rows, n_new);
  mst_admit_merge_new_kernel<<<admit_blocks(n_new), MST_ADMIT_THREADS, 0, stream>>>(d_body_b, body_b_len, s.name_begin, s.name_end, n, list, rank,
                                                                                place, m, d_body_t, body_t_len, d_name_spans, nt, d_order_out,
                                                                                d_name_spans_out);
  mst_admit_merge_old_kernel<<<admit_blocks(n_tree), MST_ADMIT_THREADS, 0, stream>>>(d_body_b, body_b_len, s.name_begin, s.name_end, n, list, m,
                                                                                 d_body_t, body_t_len, d_name_spans, d_order, nt, d_order_out,
                                                                                 d_name_spans_out);
  mst_admit_names_kernel<<<(unsigned)((n_new + MST_ENTRIES_BLOCK - 1) / MST_ENTRIES_BLOCK), MST_ENTRIES_BLOCK, 0, stream>>>(
      d_body_b, body_b_len, s.name_begin, s.name_end, n, d_new_rows, place, m, nt, (uint32_t)1 << depth, body_t_len, body_t_len + name_bytes,
      d_body_out, d_leaf_name_spans_out, static_cast<fp_words*>(d_users));
  return hipGetLastError();
}

hipError_t mst_admit_pack_launch(const uint8_t* d_body_b, uint64_t body_b_len, const uint64_t* d_words, uint64_t n_rows, uint32_t nc,
                                 const uint32_t* d_owner, const uint8_t* d_leaf_state, const uint32_t* d_new_rows, uint64_t n_new,
                                 uint64_t n_tree, const uint32_t* d_leaves, uint64_t n_leaves, uint32_t depth, void* d_packed,
                                 hipStream_t stream) {
  if (n_rows == 0 || n_rows >= (1ull << 32) || depth > MST_AUDIT_MAX_DEPTH || nc == 0 || nc > 64 || n_new > n_rows ||
      n_tree + n_new > ((uint64_t)1 << depth))
    return hipErrorInvalidValue;
  if (!n_leaves) return hipSuccess;
  const MstCsvSpans s = mst_csv_spans(const_cast<uint64_t*>(d_words), n_rows, nc);
  const uint64_t fields = n_leaves * nc;
  mst_admit_pack_kernel<<<admit_blocks(fields), MST_ADMIT_THREADS, 0, stream>>>(d_body_b, body_b_len, s.bal_begin, s.bal_end, (uint32_t)n_rows, nc,
                                                                            d_owner, d_leaf_state, d_new_rows, (uint32_t)n_new, (uint32_t)n_tree,
                                                                            d_leaves, fields, depth, static_cast<fp_words*>(d_packed));
  return hipGetLastError();
}

}  // namespace sg
