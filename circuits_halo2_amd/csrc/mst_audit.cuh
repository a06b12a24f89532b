// The range audit of a built tree (included once by mst_entries.hip, behind the sort: mst_audit.h has the rules, the work space
// and the host mirror).  The tree's arrays are read only.  Every kernel keeps all its lanes to the end -- the ballots count them --
// and guards each access by the sizes it is given.
#pragma once
#include "mst_audit.h"
#include "mst_sort.cuh"   // sort_block_scan

namespace sg {

static constexpr uint32_t MST_AUDIT_WAVES = MST_AUDIT_THREADS / 64;
static_assert(MST_AUDIT_TILE == 64, "a tile is a wave: its count is one ballot");
static_assert(MST_AUDIT_GROUP == MST_AUDIT_THREADS, "the groups step scans a count per thread");

// flags.  A workgroup owns MST_AUDIT_THREADS nodes and their nc * MST_AUDIT_THREADS balances, which lie in a row: in round j
// thread t takes balance j * THREADS + t of them, so a wave loads 2 KB in a row whatever nc is.  The balance leaves Montgomery
// form by one product (x 2^256 * 2^5 * 2^-261 = x, as msm_tiny_scalar's: the canonical integer the witness kernel's range-check
// items get by two), the header's predicate answers, and the wave's ballot is one word of the workgroup's bit string.  Then
// thread t is node t: its nc bits from the string, the flag byte, and the wave's bad nodes into the count by one atomic add.
__global__ void __launch_bounds__(MST_AUDIT_THREADS) mst_audit_flags_kernel(const fp_words* __restrict__ balances, uint32_t nodes,
                                                                           uint32_t nc, uint32_t n_bytes, uint8_t* __restrict__ flags,
                                                                           uint32_t* __restrict__ bad_nodes) {
  side_kernel_prio();
  __shared__ uint64_t s_bits[MST_AUDIT_MAX_CURRENCIES * MST_AUDIT_WAVES + 1];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t first = (uint64_t)blockIdx.x * MST_AUDIT_THREADS * nc, total = (uint64_t)nodes * nc;
  if (tid == 0) s_bits[nc * MST_AUDIT_WAVES] = 0;
  for (uint32_t j = 0; j < nc; j++) {
    const uint64_t at = first + j * MST_AUDIT_THREADS + tid;
    bool out = false;
    if (at < total) {
      f29 k = f29_zero();
      k.l[0] = 32;
      uint32_t w[8];
      f29_to_words(f29_cond_sub_p<Fr29>(f29_mul<Fr29>(f29_load_r256<Fr29>(balances + at), k)), w);
      out = !mst_audit_in_range(w, n_bytes);
    }
    const uint64_t word = __ballot(out);
    if (lane == 0) s_bits[j * MST_AUDIT_WAVES + wave] = word;
  }
  __syncthreads();
  const uint32_t node = blockIdx.x * MST_AUDIT_THREADS + tid;
  const uint32_t p = tid * nc, q = p >> 6, sh = p & 63;      // the node's bits: p .. p + nc of the string
  uint64_t bits = s_bits[q] >> sh;
  if (sh) bits |= s_bits[q + 1] << (64 - sh);
  if (nc < 64) bits &= ((uint64_t)1 << nc) - 1;
  const uint8_t flag = node < nodes ? mst_audit_flag(bits) : 0;
  if (node < nodes) flags[node] = flag;
  const uint32_t bad = (uint32_t)__popcll(__ballot(flag != 0));
  if (lane == 0 && bad) atomicAdd(bad_nodes, bad);
}

// masks, a leaf per thread; tile_count[tile] = the wave's leaves with a non-zero mask
__global__ void __launch_bounds__(MST_AUDIT_THREADS) mst_audit_masks_kernel(const uint8_t* __restrict__ flags, uint32_t depth,
                                                                           uint32_t* __restrict__ masks,
                                                                           uint32_t* __restrict__ tile_count) {
  side_kernel_prio();
  const uint32_t i = blockIdx.x * MST_AUDIT_THREADS + threadIdx.x, leaves = (uint32_t)1 << depth;
  uint32_t mask = 0;
  if (i < leaves) {
    mask = mst_audit_mask(flags, i, depth);
    masks[i] = mask;
  }
  const uint32_t count = (uint32_t)__popcll(__ballot(mask != 0));
  const uint32_t tile = i / MST_AUDIT_TILE;
  if ((threadIdx.x & 63) == 0 && tile < mst_audit_tiles(depth)) tile_count[tile] = count;
}

// groups, a tile count per thread: the exclusive prefix within the group in place, the group's total aside
__global__ void __launch_bounds__(MST_AUDIT_THREADS) mst_audit_groups_kernel(uint32_t* __restrict__ tile_count, uint32_t tiles,
                                                                            uint32_t* __restrict__ group_total) {
  side_kernel_prio();
  __shared__ uint32_t s_w[MST_AUDIT_WAVES];
  const uint32_t t = blockIdx.x * MST_AUDIT_GROUP + threadIdx.x;
  const uint32_t count = t < tiles ? tile_count[t] : 0u;
  uint32_t total;
  const uint32_t before = sort_block_scan<MST_AUDIT_THREADS>(count, s_w, &total);
  if (t < tiles) tile_count[t] = before;
  if (threadIdx.x == 0) group_total[blockIdx.x] = total;
}

// scatter, a leaf per thread: where a leaf with a non-zero mask stands in the list is the totals of the groups before its own,
// its tile's prefix and the lanes below it in the wave's ballot -- data alone.  The first wave also leaves what the host reads:
// the number of such leaves and the root's flag.
__global__ void __launch_bounds__(MST_AUDIT_THREADS) mst_audit_scatter_kernel(const uint32_t* __restrict__ masks, uint32_t depth,
                                                                             const uint8_t* __restrict__ flags,
                                                                             const uint32_t* __restrict__ tile_count,
                                                                             const uint32_t* __restrict__ group_total,
                                                                             uint32_t* __restrict__ bad, uint64_t bad_cap,
                                                                             uint32_t* __restrict__ result) {
  side_kernel_prio();
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t i = blockIdx.x * MST_AUDIT_THREADS + threadIdx.x, leaves = (uint32_t)1 << depth;
  const uint32_t tile = i / MST_AUDIT_TILE, groups = mst_audit_groups(depth);
  const uint32_t group = tile / MST_AUDIT_GROUP;
  const bool listed = i < leaves && masks[i] != 0;
  const uint64_t peers = __ballot(listed);
  const uint32_t upto = i < MST_AUDIT_TILE ? groups : group < groups ? group : groups;   // the first wave sums every group
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
  if (i == 0) {
    result[MST_AUDIT_AT_UNPROVABLE] = all;
    result[MST_AUDIT_AT_ROOT] = flags[mst_audit_nodes(depth) - 1];
  }
  if (listed) {
    const uint64_t at = (uint64_t)before + tile_count[tile] + (uint32_t)__popcll(peers & (((uint64_t)1 << lane) - 1));
    if (at < bad_cap) bad[at] = i;
  }
}

hipError_t mst_audit_launch(const void* d_node_balances, uint32_t depth, uint32_t nc, uint32_t n_bytes, uint8_t* d_flags, uint32_t* d_masks,
                            uint32_t* d_bad, uint64_t bad_cap, uint32_t* d_work, hipStream_t stream) {
  if (depth > MST_AUDIT_MAX_DEPTH || nc == 0 || nc > MST_AUDIT_MAX_CURRENCIES || n_bytes == 0 || n_bytes > MST_AUDIT_MAX_BYTES)
    return hipErrorInvalidValue;
  const uint32_t nodes = mst_audit_nodes(depth), leaves = (uint32_t)1 << depth, tiles = mst_audit_tiles(depth);
  uint32_t *tile_count = d_work + mst_audit_at_tiles(), *group_total = d_work + mst_audit_at_groups(depth);
  const unsigned leaf_blocks = (leaves + MST_AUDIT_THREADS - 1) / MST_AUDIT_THREADS;
  mst_audit_flags_kernel<<<(nodes + MST_AUDIT_THREADS - 1) / MST_AUDIT_THREADS, MST_AUDIT_THREADS, 0, stream>>>(
      static_cast<const fp_words*>(d_node_balances), nodes, nc, n_bytes, d_flags, d_work + MST_AUDIT_AT_BAD_NODES);
  mst_audit_masks_kernel<<<leaf_blocks, MST_AUDIT_THREADS, 0, stream>>>(d_flags, depth, d_masks, tile_count);
  mst_audit_groups_kernel<<<mst_audit_groups(depth), MST_AUDIT_THREADS, 0, stream>>>(tile_count, tiles, group_total);
  mst_audit_scatter_kernel<<<leaf_blocks, MST_AUDIT_THREADS, 0, stream>>>(d_masks, depth, d_flags, tile_count, group_total, d_bad, bad_cap,
                                                                        d_work);
  return hipGetLastError();
}

}  // namespace sg
