// The next round's snapshot against a tree in HBM (included once by mst_entries.hip, behind the names: mst_diff.h has the rules,
// the work space and the host mirror).  Both texts, the tree's spans, order and balances are read only.  The kernels that count by
// ballot keep all their lanes to the end, and every access is guarded by the sizes the kernel is given.  The lookup is one
// binary search per row through two gathers a step (a span, then name bytes): divergent and bound by latency, so a row per thread
// and as many waves in flight as the device takes is all there is to it.
#pragma once
#include "mst_diff.h"
#include "mst_names.cuh"   // mst_audit_groups_kernel: the scan of the tile counts

namespace sg {

static_assert(MST_DIFF_TILE == 64, "a tile is a wave: its count is one ballot");
static_assert(MST_DIFF_TILE == MST_AUDIT_TILE && MST_DIFF_GROUP == MST_AUDIT_GROUP && MST_DIFF_THREADS == MST_AUDIT_THREADS,
              "the groups step is the audit's kernel");

// match, a row of B per thread: its name where B's text has it is the query of the lower-bound search over T's sorted names; the
// leaf goes into row_leaf and the row into the leaf's owner by an atomic minimum -- the lowest row wins whatever the arrival order
__global__ void __launch_bounds__(MST_DIFF_THREADS) mst_diff_match_kernel(const uint8_t* __restrict__ body_b, uint64_t body_b_len,
                                                                         const uint64_t* __restrict__ name_begin,
                                                                         const uint64_t* __restrict__ name_end, uint32_t n,
                                                                         const uint8_t* __restrict__ body_t, uint64_t body_t_len,
                                                                         const uint32_t* __restrict__ name_spans,
                                                                         const uint32_t* __restrict__ order, uint32_t n_tree, uint32_t depth,
                                                                         uint32_t* __restrict__ row_leaf, uint32_t* __restrict__ owner) {
  side_kernel_prio();
  const uint64_t at = (uint64_t)blockIdx.x * MST_DIFF_THREADS + threadIdx.x;
  if (at >= n) return;
  uint64_t b, e;
  mst_diff_span(name_begin, name_end, at, body_b_len, &b, &e);
  const uint32_t leaf = mst_diff_lookup(body_t, body_t_len, name_spans, order, n_tree, depth, body_b + b, e - b);
  row_leaf[at] = leaf;
  if (leaf != MST_DIFF_ABSENT) atomicMin(owner + leaf, (uint32_t)at);   // leaf < 2^depth
}

// judge, a row of B per thread: its state, and for the owner of a leaf the compare of its nc balance texts, folded in the field,
// with the leaf's balances, and the leaf's state.  The wave's rows of each state by ballot, one atomic add per wave and state.
__global__ void __launch_bounds__(MST_DIFF_THREADS) mst_diff_judge_kernel(const uint8_t* __restrict__ body_b, uint64_t body_b_len,
                                                                         const uint64_t* __restrict__ bal_begin,
                                                                         const uint64_t* __restrict__ bal_end, uint32_t n, uint32_t nc,
                                                                         uint32_t depth, const fp_words* __restrict__ leaf_bal,
                                                                         const uint32_t* __restrict__ row_leaf,
                                                                         const uint32_t* __restrict__ owner, uint8_t* __restrict__ row_state,
                                                                         uint8_t* __restrict__ leaf_state, uint32_t* __restrict__ counts) {
  side_kernel_prio();
  const uint64_t at = (uint64_t)blockIdx.x * MST_DIFF_THREADS + threadIdx.x;
  uint8_t state = 0;
  if (at < n) {
    const uint32_t row = (uint32_t)at, leaf = row_leaf[at];
    state = MST_DIFF_ROW_NEW;
    if (leaf != MST_DIFF_ABSENT && leaf < ((uint32_t)1 << depth)) {
      state = MST_DIFF_ROW_SHADOWED;
      if (owner[leaf] == row) {
        bool differs = false;
        for (uint32_t c = 0; c < nc && !differs; c++) {
          uint64_t b, e;
          mst_diff_span(bal_begin, bal_end, (uint64_t)row * nc + c, body_b_len, &b, &e);
          uint32_t w[8];
          fp_words_load(leaf_bal + (size_t)leaf * nc + c, w);
          differs = !mst_diff_balance_equal(body_b, b, e, w);
        }
        state = differs ? MST_DIFF_ROW_CHANGED : MST_DIFF_ROW_SAME;
        leaf_state[leaf] = differs ? MST_DIFF_LEAF_CHANGED : MST_DIFF_LEAF_SAME;
      }
    }
    row_state[at] = state;
  }
  const uint32_t fresh = (uint32_t)__popcll(__ballot(state == MST_DIFF_ROW_NEW));
  const uint32_t shadowed = (uint32_t)__popcll(__ballot(state == MST_DIFF_ROW_SHADOWED));
  const uint32_t changed = (uint32_t)__popcll(__ballot(state == MST_DIFF_ROW_CHANGED));
  const uint32_t same = (uint32_t)__popcll(__ballot(state == MST_DIFF_ROW_SAME));
  if ((threadIdx.x & 63) == 0) {
    if (fresh) atomicAdd(counts + MST_DIFF_SUM_NEW, fresh);
    if (shadowed) atomicAdd(counts + MST_DIFF_SUM_SHADOWED, shadowed);
    if (changed) atomicAdd(counts + MST_DIFF_SUM_CHANGED, changed);
    if (same) atomicAdd(counts + MST_DIFF_SUM_SAME, same);
  }
}

// tree, a sorted position of T per thread: a position whose name is the name before it is a leaf no lookup reaches; the head of
// a run that no row owns is gone.  The owned heads have their state from judge.  Counts by ballot as above.
__global__ void __launch_bounds__(MST_DIFF_THREADS) mst_diff_tree_kernel(const uint8_t* __restrict__ body_t, uint64_t body_t_len,
                                                                        const uint32_t* __restrict__ name_spans,
                                                                        const uint32_t* __restrict__ order, uint32_t n_tree, uint32_t depth,
                                                                        const uint32_t* __restrict__ owner, uint8_t* __restrict__ leaf_state,
                                                                        uint32_t* __restrict__ counts) {
  side_kernel_prio();
  const uint64_t at = (uint64_t)blockIdx.x * MST_DIFF_THREADS + threadIdx.x;
  uint8_t code = 0;
  if (at < n_tree) {
    const uint32_t i = (uint32_t)at, leaf = order ? order[i] : i;
    if (leaf < ((uint32_t)1 << depth)) {
      if (mst_names_shadowed(body_t, body_t_len, name_spans, i)) code = MST_DIFF_LEAF_UNREACHABLE;
      else if (owner[leaf] == MST_DIFF_ABSENT) code = MST_DIFF_LEAF_GONE;
      if (code) leaf_state[leaf] = code;
    }
  }
  const uint32_t gone = (uint32_t)__popcll(__ballot(code == MST_DIFF_LEAF_GONE));
  const uint32_t unreachable = (uint32_t)__popcll(__ballot(code == MST_DIFF_LEAF_UNREACHABLE));
  if ((threadIdx.x & 63) == 0) {
    if (gone) atomicAdd(counts + MST_DIFF_SUM_GONE, gone);
    if (unreachable) atomicAdd(counts + MST_DIFF_SUM_UNREACHABLE, unreachable);
  }
}

// marks, an item per thread: tile_count[tile] = the wave's items whose state is `code`
__global__ void __launch_bounds__(MST_DIFF_THREADS) mst_diff_marks_kernel(const uint8_t* __restrict__ state, uint64_t n, uint8_t code,
                                                                         uint32_t* __restrict__ tile_count) {
  side_kernel_prio();
  const uint64_t at = (uint64_t)blockIdx.x * MST_DIFF_THREADS + threadIdx.x;
  const bool hit = at < n && state[at] == code;
  const uint32_t count = (uint32_t)__popcll(__ballot(hit));
  const uint64_t tile = at / MST_DIFF_TILE;
  if ((threadIdx.x & 63) == 0 && tile < mst_diff_tiles(n)) tile_count[tile] = count;
}

// scatter, an item per thread: where an item whose state is `code` stands in the list is the totals of the groups before its own,
// its tile's prefix and the lanes below it in the wave's ballot -- data alone.  With cap == 0 nothing is listed.
__global__ void __launch_bounds__(MST_DIFF_THREADS) mst_diff_scatter_kernel(const uint8_t* __restrict__ state, uint64_t n, uint8_t code,
                                                                           const uint32_t* __restrict__ tile_count,
                                                                           const uint32_t* __restrict__ group_total,
                                                                           uint32_t* __restrict__ out, uint64_t cap) {
  side_kernel_prio();
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t at = (uint64_t)blockIdx.x * MST_DIFF_THREADS + threadIdx.x;
  const uint32_t tile = (uint32_t)(at / MST_DIFF_TILE), groups = mst_diff_groups(n);
  const uint32_t group = tile / MST_DIFF_GROUP;
  const bool listed = cap != 0 && at < n && state[at] == code;
  const uint64_t peers = __ballot(listed);
  const uint32_t upto = group < groups ? group : groups;
  uint32_t before = 0;
  for (uint32_t g = lane; g < upto; g += 64) before += group_total[g];
#pragma unroll
  for (uint32_t off = 32; off; off >>= 1) before += __shfl_xor(before, off);
  if (listed) {                                              // at < n: tile < tiles
    const uint64_t place = (uint64_t)before + tile_count[tile] + (uint32_t)__popcll(peers & (((uint64_t)1 << lane) - 1));
    if (place < cap) out[place] = (uint32_t)at;
  }
}

// pack, a changed leaf and a currency per thread: the owner row's balance text folded into the field element the update takes
__global__ void __launch_bounds__(MST_DIFF_THREADS) mst_diff_pack_kernel(const uint8_t* __restrict__ body_b, uint64_t body_b_len,
                                                                        const uint64_t* __restrict__ bal_begin,
                                                                        const uint64_t* __restrict__ bal_end, uint32_t n_rows, uint32_t nc,
                                                                        const uint32_t* __restrict__ owner,
                                                                        const uint32_t* __restrict__ changed, uint64_t fields, uint32_t depth,
                                                                        fp_words* __restrict__ packed) {
  side_kernel_prio();
  const uint64_t t = (uint64_t)blockIdx.x * MST_DIFF_THREADS + threadIdx.x;
  if (t >= fields) return;
  const uint32_t leaf = changed[t / nc], c = (uint32_t)(t % nc);
  uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (leaf < ((uint32_t)1 << depth)) {
    const uint32_t row = owner[leaf];
    if (row < n_rows) {
      uint64_t b, e;
      mst_diff_span(bal_begin, bal_end, (uint64_t)row * nc + c, body_b_len, &b, &e);
      mst_decimal_words(body_b + b, (size_t)(e - b), w);
    }
  }
  fp_words_store(packed + t, w);
}

static unsigned diff_blocks(uint64_t threads) { return (unsigned)((threads + MST_DIFF_THREADS - 1) / MST_DIFF_THREADS); }

// the ordered list of the items of `state` whose value is `code`: marks, the audit's groups, scatter
static hipError_t diff_compact(const uint8_t* state, uint64_t n, uint8_t code, uint32_t* work, uint32_t* out, uint64_t cap, hipStream_t stream) {
  uint32_t *tile_count = work, *group_total = work + mst_diff_tiles(n);
  mst_diff_marks_kernel<<<diff_blocks(n), MST_DIFF_THREADS, 0, stream>>>(state, n, code, tile_count);
  mst_audit_groups_kernel<<<mst_diff_groups(n), MST_AUDIT_THREADS, 0, stream>>>(tile_count, mst_diff_tiles(n), group_total);
  mst_diff_scatter_kernel<<<diff_blocks(n), MST_DIFF_THREADS, 0, stream>>>(state, n, code, tile_count, group_total, out, cap);
  return hipGetLastError();
}

hipError_t mst_diff_launch(const uint8_t* d_body_b, uint64_t body_b_len, const uint64_t* d_words, uint64_t n_rows, uint32_t nc,
                           const uint8_t* d_body_t, uint64_t body_t_len, const uint32_t* d_name_spans, const uint32_t* d_order, uint64_t n_tree,
                           uint32_t depth, const void* d_leaf_balances, uint32_t* d_row_leaf, uint8_t* d_row_state, uint8_t* d_leaf_state,
                           uint32_t* d_owner, uint32_t* d_changed, uint32_t* d_new_rows, uint32_t* d_gone, uint64_t cap, uint32_t* d_work,
                           hipStream_t stream) {
  if (n_rows == 0 || n_rows >= (1ull << 32) || depth > MST_AUDIT_MAX_DEPTH || n_tree == 0 || n_tree > ((uint64_t)1 << depth) || nc == 0 ||
      nc > 64 || (cap && (!d_new_rows || !d_gone)))
    return hipErrorInvalidValue;
  const uint64_t leaves = (uint64_t)1 << depth;
  const uint32_t n = (uint32_t)n_rows, nt = (uint32_t)n_tree;
  const MstCsvSpans s = mst_csv_spans(const_cast<uint64_t*>(d_words), n_rows, nc);
  hipError_t e = hipMemsetAsync(d_work, 0, 4 * MST_DIFF_FRONT_WORDS, stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_owner, 0xff, 4 * leaves, stream);          // MST_DIFF_ABSENT
  if (e == hipSuccess) e = hipMemsetAsync(d_leaf_state, 0, leaves, stream);            // MST_DIFF_LEAF_PADDING
  if (e != hipSuccess) return e;
  mst_diff_match_kernel<<<diff_blocks(n_rows), MST_DIFF_THREADS, 0, stream>>>(d_body_b, body_b_len, s.name_begin, s.name_end, n, d_body_t,
                                                                           body_t_len, d_name_spans, d_order, nt, depth, d_row_leaf, d_owner);
  mst_diff_judge_kernel<<<diff_blocks(n_rows), MST_DIFF_THREADS, 0, stream>>>(d_body_b, body_b_len, s.bal_begin, s.bal_end, n, nc, depth,
                                                                           static_cast<const fp_words*>(d_leaf_balances), d_row_leaf, d_owner,
                                                                           d_row_state, d_leaf_state, d_work);
  mst_diff_tree_kernel<<<diff_blocks(n_tree), MST_DIFF_THREADS, 0, stream>>>(d_body_t, body_t_len, d_name_spans, d_order, nt, depth, d_owner,
                                                                          d_leaf_state, d_work);
  e = hipGetLastError();
  if (e == hipSuccess) e = diff_compact(d_leaf_state, leaves, MST_DIFF_LEAF_CHANGED, d_work + mst_diff_at_changed(), d_changed, ~0ull, stream);
  if (e == hipSuccess) e = diff_compact(d_leaf_state, leaves, MST_DIFF_LEAF_GONE, d_work + mst_diff_at_gone(depth), d_gone, cap, stream);
  if (e == hipSuccess) e = diff_compact(d_row_state, n_rows, MST_DIFF_ROW_NEW, d_work + mst_diff_at_new(depth), d_new_rows, cap, stream);
  return e;
}

hipError_t mst_diff_pack_launch(const uint8_t* d_body_b, uint64_t body_b_len, const uint64_t* d_words, uint64_t n_rows, uint32_t nc,
                                const uint32_t* d_owner, const uint32_t* d_changed, uint64_t n_changed, uint32_t depth, void* d_packed,
                                hipStream_t stream) {
  if (n_rows == 0 || n_rows >= (1ull << 32) || depth > MST_AUDIT_MAX_DEPTH || nc == 0 || nc > 64) return hipErrorInvalidValue;
  if (!n_changed) return hipSuccess;
  const MstCsvSpans s = mst_csv_spans(const_cast<uint64_t*>(d_words), n_rows, nc);
  const uint64_t fields = n_changed * nc;
  mst_diff_pack_kernel<<<diff_blocks(fields), MST_DIFF_THREADS, 0, stream>>>(d_body_b, body_b_len, s.bal_begin, s.bal_end, (uint32_t)n_rows, nc,
                                                                          d_owner, d_changed, fields, depth, static_cast<fp_words*>(d_packed));
  return hipGetLastError();
}

}  // namespace sg
