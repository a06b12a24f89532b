// The duplicate-username report and the index's spans in file order (included once by mst_entries.hip, behind the audit:
// mst_names.h has the rules, the work space and the host mirror).  The text, the spans and the order are read only.  Every kernel
// keeps all its lanes to the end -- the ballots count them -- and guards each access by the sizes it is given.  Span loads are
// coalesced (a position per lane, 8 bytes each); name bytes are gathers through the spans, as in the find kernel.
#pragma once
#include "mst_names.h"
#include "mst_audit.cuh"   // mst_audit_groups_kernel: the scan of the tile counts

namespace sg {

static_assert(MST_NAMES_TILE == 64, "a tile is a wave: its count is one ballot");
static_assert(MST_NAMES_TILE == MST_AUDIT_TILE && MST_NAMES_GROUP == MST_AUDIT_GROUP && MST_NAMES_THREADS == MST_AUDIT_THREADS,
              "the groups step is the audit's kernel");

// marks, a sorted position per thread: is its name the name before it?  tile_count[tile] = the wave's shadowed positions; a
// repeated name is a shadowed position behind one that is not -- the lane below in the ballot, for lane 0 one more compare --
// and the wave's number of them goes into the count by one atomic add.
__global__ void __launch_bounds__(MST_NAMES_THREADS) mst_names_marks_kernel(const uint8_t* __restrict__ body, uint64_t body_len,
                                                                           const uint32_t* __restrict__ name_spans, uint32_t n,
                                                                           uint32_t* __restrict__ tile_count,
                                                                           uint32_t* __restrict__ repeated) {
  side_kernel_prio();
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t at = (uint64_t)blockIdx.x * MST_NAMES_THREADS + threadIdx.x;
  const uint32_t i = (uint32_t)at;
  const bool mark = at < n && mst_names_shadowed(body, body_len, name_spans, i);
  const uint64_t marks = __ballot(mark);
  bool before = lane != 0 && ((marks >> (lane - 1)) & 1);
  if (lane == 0 && mark) before = mst_names_shadowed(body, body_len, name_spans, i - 1);   // mark: i >= 1
  const uint32_t heads = (uint32_t)__popcll(__ballot(mark && !before));
  const uint64_t tile = at / MST_NAMES_TILE;
  if (lane == 0 && tile < mst_names_tiles(n)) tile_count[tile] = (uint32_t)__popcll(marks);
  if (lane == 0 && heads) atomicAdd(repeated, heads);
}

// scatter, a sorted position per thread: where a shadowed position stands in the list is the totals of the groups before its
// own, its tile's prefix and the lanes below it in the wave's ballot -- data alone.  A listed position then finds the head of
// its run by the lower-bound search over all positions with its own name as the query, and both leaves go through the order
// where there is one.  The first wave also leaves what the host reads: the number of shadowed positions.  With cap == 0 nothing
// is listed and no name is compared.
__global__ void __launch_bounds__(MST_NAMES_THREADS) mst_names_scatter_kernel(const uint8_t* __restrict__ body, uint64_t body_len,
                                                                             const uint32_t* __restrict__ name_spans,
                                                                             const uint32_t* __restrict__ order, uint32_t n,
                                                                             const uint32_t* __restrict__ tile_count,
                                                                             const uint32_t* __restrict__ group_total,
                                                                             uint32_t* __restrict__ shadowed, uint32_t* __restrict__ first,
                                                                             uint64_t cap, uint32_t* __restrict__ result) {
  side_kernel_prio();
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t at = (uint64_t)blockIdx.x * MST_NAMES_THREADS + threadIdx.x;
  const uint32_t i = (uint32_t)at;
  const uint32_t tile = (uint32_t)(at / MST_NAMES_TILE), groups = mst_names_groups(n);
  const uint32_t group = tile / MST_NAMES_GROUP;
  const bool listed = cap != 0 && at < n && mst_names_shadowed(body, body_len, name_spans, i);
  const uint64_t peers = __ballot(listed);
  const uint32_t upto = at < MST_NAMES_TILE ? groups : group < groups ? group : groups;   // the first wave sums every group
  uint32_t before = 0, all = 0;
  for (uint32_t g = lane; g < upto; g += 64) {
    const uint32_t x = group_total[g];
    all += x;
    if (g < group) before += x;
  }
#pragma unroll
  for (uint32_t off = 32; off; off >>= 1) {
    before += __shfl_xor(before, off);
    all += __shfl_xor(all, off);
  }
  if (at == 0) result[MST_NAMES_AT_SHADOWED] = all;
  if (listed) {                                              // at < n: tile < tiles
    const uint64_t place = (uint64_t)before + tile_count[tile] + (uint32_t)__popcll(peers & (((uint64_t)1 << lane) - 1));
    if (place < cap) {
      const uint32_t head = mst_names_head(body, body_len, name_spans, n, i);   // head < n
      shadowed[place] = order ? order[i] : i;
      first[place] = order ? order[head] : head;
    }
  }
}

// the span copy, a file row per thread: the split's 64-bit name span as two 32-bit words (a body is under 4 GiB)
__global__ void __launch_bounds__(MST_NAMES_THREADS) mst_names_leaf_spans_kernel(const uint64_t* __restrict__ name_begin,
                                                                                const uint64_t* __restrict__ name_end, uint64_t n,
                                                                                uint32_t* __restrict__ leaf_name_spans) {
  side_kernel_prio();
  const uint64_t row = (uint64_t)blockIdx.x * MST_NAMES_THREADS + threadIdx.x;
  if (row < n) {
    leaf_name_spans[2 * row] = (uint32_t)name_begin[row];
    leaf_name_spans[2 * row + 1] = (uint32_t)name_end[row];
  }
}

hipError_t mst_names_leaf_spans_launch(const uint64_t* d_words, uint64_t n_rows, uint32_t nc, uint32_t* d_leaf_name_spans, hipStream_t stream) {
  if (n_rows == 0 || n_rows >= (1ull << 32)) return hipErrorInvalidValue;
  const MstCsvSpans s = mst_csv_spans(const_cast<uint64_t*>(d_words), n_rows, nc);
  mst_names_leaf_spans_kernel<<<(unsigned)((n_rows + MST_NAMES_THREADS - 1) / MST_NAMES_THREADS), MST_NAMES_THREADS, 0, stream>>>(
      s.name_begin, s.name_end, n_rows, d_leaf_name_spans);
  return hipGetLastError();
}

hipError_t mst_names_launch(const uint8_t* d_body, uint64_t body_len, const uint32_t* d_name_spans, const uint32_t* d_order, uint64_t n_rows,
                            uint32_t* d_shadowed, uint32_t* d_first, uint64_t cap, uint32_t* d_work, hipStream_t stream) {
  if (n_rows == 0 || n_rows >= (1ull << 32) || (cap && (!d_shadowed || !d_first))) return hipErrorInvalidValue;
  const uint32_t n = (uint32_t)n_rows, tiles = mst_names_tiles(n_rows), groups = mst_names_groups(n_rows);
  uint32_t *tile_count = d_work + mst_names_at_tiles(), *group_total = d_work + mst_names_at_groups(n_rows);
  const unsigned blocks = (unsigned)((n_rows + MST_NAMES_THREADS - 1) / MST_NAMES_THREADS);
  mst_names_marks_kernel<<<blocks, MST_NAMES_THREADS, 0, stream>>>(d_body, body_len, d_name_spans, n, tile_count,
                                                                   d_work + MST_NAMES_AT_REPEATED);
  mst_audit_groups_kernel<<<groups, MST_AUDIT_THREADS, 0, stream>>>(tile_count, tiles, group_total);
  mst_names_scatter_kernel<<<blocks, MST_NAMES_THREADS, 0, stream>>>(d_body, body_len, d_name_spans, d_order, n, tile_count, group_total,
                                                                     d_shadowed, d_first, cap, d_work);
  return hipGetLastError();
}

}  // namespace sg
