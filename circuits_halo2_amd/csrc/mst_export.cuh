// A tree in HBM written back out as its snapshot CSV (included once by mst_entries.hip, behind the diff: mst_export.h has the rules,
// the work space and the host mirror).  The text, the spans and the balances are read only.  The kernels that add up or scan a
// wave's lengths keep all their lanes to the end, every load is guarded by the sizes the kernel is given and every store of the
// writer by the body's length.
#pragma once
#include "mst_export.h"
#include "mst_audit.cuh"   // mst_audit_groups_kernel: the scan of the tile sums

namespace sg {

static_assert(MST_EXPORT_TILE == 64, "a tile is a wave: its sum is one reduction over the lanes");
static_assert(MST_EXPORT_TILE == MST_AUDIT_TILE && MST_EXPORT_GROUP == MST_AUDIT_GROUP && MST_EXPORT_THREADS == MST_AUDIT_THREADS,
              "the groups step is the audit's kernel");
static_assert(MST_EXPORT_STAGE % 16 == 0 && (MST_EXPORT_THREADS / 64) * MST_EXPORT_STAGE <= 64 * 1024, "the stage of a workgroup's waves");

// measure, a row per thread: the name's cut length, nc delimiters, the digits of its nc balances, the line end -> row_off[row];
// tile_sum[tile] = the wave's sum (a row is at most MST_EXPORT_MAX_ROW bytes: 32 bits hold 64 of them)
__global__ void __launch_bounds__(MST_EXPORT_THREADS) mst_export_measure_kernel(uint64_t body_len, const uint32_t* __restrict__ leaf_name_spans,
                                                                             uint32_t n, uint32_t nc, const fp_words* __restrict__ leaf_bal,
                                                                             uint32_t* __restrict__ row_off, uint32_t* __restrict__ tile_sum) {
  side_kernel_prio();
  const uint64_t at = (uint64_t)blockIdx.x * MST_EXPORT_THREADS + threadIdx.x;
  uint32_t len = 0;
  if (at < n) {
    const uint32_t i = (uint32_t)at;
    uint64_t b, e;
    mst_export_name(leaf_name_spans, body_len, i, &b, &e);
    uint32_t digits = 0;
    for (uint32_t c = 0; c < nc; c++) {
      uint32_t m[8];
      fp_words_load(leaf_bal + (size_t)i * nc + c, m);
      digits += mst_export_balance_digits(m);
    }
    len = mst_export_row_bytes((uint32_t)(e - b), nc, digits);
    row_off[at] = len;
  }
  uint32_t sum = len;
#pragma unroll
  for (uint32_t off = 32; off; off >>= 1) sum += __shfl_xor(sum, off);
  const uint64_t tile = at / MST_EXPORT_TILE;
  if ((threadIdx.x & 63) == 0 && tile < mst_export_tiles(n)) tile_sum[tile] = sum;
}

// offsets, a row per thread: its length, left in row_off by measure, becomes its start: the totals of the groups before its own,
// its tile's prefix and the lengths of the lanes below it -- data alone.  The first wave also leaves what the host reads: the sum
// of every group's total in 64 bits, low word first.
__global__ void __launch_bounds__(MST_EXPORT_THREADS) mst_export_offsets_kernel(uint32_t* __restrict__ row_off, uint32_t n,
                                                                             const uint32_t* __restrict__ tile_sum,
                                                                             const uint32_t* __restrict__ group_total,
                                                                             uint32_t* __restrict__ result) {
  side_kernel_prio();
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t at = (uint64_t)blockIdx.x * MST_EXPORT_THREADS + threadIdx.x;
  const uint32_t tile = (uint32_t)(at / MST_EXPORT_TILE), groups = mst_export_groups(n);
  const uint32_t group = tile / MST_EXPORT_GROUP;
  const uint32_t len = at < n ? row_off[at] : 0u;
  uint32_t below = len;                                        // inclusive scan over the lanes, then less the lane's own
#pragma unroll
  for (uint32_t off = 1; off < 64; off <<= 1) {
    const uint32_t x = __shfl_up(below, off);
    if (lane >= off) below += x;
  }
  below -= len;
  const uint32_t upto = at < MST_EXPORT_TILE ? groups : group < groups ? group : groups;   // the first wave sums every group
  uint32_t before = 0;
  unsigned long long all = 0;
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
  if (at == 0) {
    result[MST_EXPORT_AT_TOTAL] = (uint32_t)all;
    result[MST_EXPORT_AT_TOTAL + 1] = (uint32_t)(all >> 32);
  }
  if (at < n) row_off[at] = before + tile_sum[tile] + below;   // at < n: tile < tiles
}

// a row's bytes at out[at ..), every store guarded by limit: mst_export_put_row with the balances loaded 16 bytes at a time
__device__ __forceinline__ void export_put_row(const uint8_t* __restrict__ body, uint64_t body_len, const uint32_t* __restrict__ leaf_name_spans,
                                               uint32_t i, uint32_t nc, const fp_words* __restrict__ leaf_bal, uint8_t delim, uint8_t* out,
                                               uint64_t limit, uint64_t at) {
  uint64_t b, e;
  mst_export_name(leaf_name_spans, body_len, i, &b, &e);
  uint64_t p = at + mst_export_put_name(body, b, e, out, limit, at);
  for (uint32_t c = 0; c < nc; c++) {
    uint32_t m[8];
    fp_words_load(leaf_bal + (size_t)i * nc + c, m);
    p += mst_export_put_balance(m, delim, out, limit, p);
  }
  mst_export_put(out, limit, p, (uint8_t)'\n');
}

// write, a wave per tile: the tile's output is one run of bytes, from its first row's start to the next tile's (the body's end
// behind the last tile).  Every lane formats its row into the wave's stage in LDS, displaced so that a 16-byte piece of the stage
// is a 16-byte aligned piece of the output; then the wave stores the run, 16 bytes a lane where a piece lies inside it and byte
// by byte at its two ends.  A tile whose run does not fit the stage (long names, many currencies), or one of whose rows does not
// start inside the run (positions the library did not make), is written a row per thread with byte stores instead.
__global__ void __launch_bounds__(MST_EXPORT_THREADS) mst_export_write_tiles_kernel(const uint8_t* __restrict__ body, uint64_t body_len,
                                                                                 const uint32_t* __restrict__ leaf_name_spans, uint32_t n,
                                                                                 uint32_t nc, const fp_words* __restrict__ leaf_bal,
                                                                                 uint8_t delim, const uint32_t* __restrict__ row_off,
                                                                                 uint64_t body_bytes, uint8_t* __restrict__ out) {
  side_kernel_prio();
  __shared__ uint4 s_stage[(MST_EXPORT_THREADS / 64) * (MST_EXPORT_STAGE / 16)];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t at = (uint64_t)blockIdx.x * MST_EXPORT_THREADS + threadIdx.x;
  const uint64_t first = at - lane, next = first + MST_EXPORT_TILE;          // the tile's rows: first .. next
  uint8_t* stage = reinterpret_cast<uint8_t*>(s_stage + wave * (MST_EXPORT_STAGE / 16));
  const uint64_t run_begin = first < n ? row_off[first] : body_bytes;
  const uint64_t run_end = next < n ? row_off[next] : body_bytes;
  const uint32_t shift = (uint32_t)((uintptr_t)(out + run_begin) & 15);
  const uint64_t mine = at < n ? row_off[at] : run_begin;
  const bool staged = run_begin <= run_end && run_end <= body_bytes && run_end - run_begin + shift <= MST_EXPORT_STAGE &&
                      __all(mine >= run_begin && mine <= run_end);                  // the wave's
  if (at < n) {
    if (staged)
      export_put_row(body, body_len, leaf_name_spans, (uint32_t)at, nc, leaf_bal, delim, stage, MST_EXPORT_STAGE, mine - run_begin + shift);
    else
      export_put_row(body, body_len, leaf_name_spans, (uint32_t)at, nc, leaf_bal, delim, out, body_bytes, mine);
  }
  __syncthreads();
  if (!staged) return;
  // stage byte s is output byte run_begin - shift + s: piece k, stage bytes 16 k .. 16 k + 16, lies on a 16-byte boundary of both
  const uint32_t bytes = (uint32_t)(run_end - run_begin) + shift;
  for (uint32_t k = lane; 16 * k < bytes; k += 64) {
    const uint32_t lo = 16 * k, hi = lo + 16;
    uint8_t* to = out + run_begin - shift + lo;
    if (lo >= shift && hi <= bytes) {
      *reinterpret_cast<uint4*>(to) = s_stage[wave * (MST_EXPORT_STAGE / 16) + k];
    } else {
      for (uint32_t s = lo < shift ? shift : lo; s < hi && s < bytes; s++) to[s - lo] = stage[s];
    }
  }
}

static unsigned export_blocks(uint64_t threads) { return (unsigned)((threads + MST_EXPORT_THREADS - 1) / MST_EXPORT_THREADS); }

hipError_t mst_export_measure_launch(const uint8_t* d_body, uint64_t body_len, const uint32_t* d_leaf_name_spans, uint64_t n_rows, uint32_t nc,
                                     const void* d_leaf_balances, uint32_t* d_row_off, uint32_t* d_work, hipStream_t stream) {
  (void)d_body;
  if (n_rows == 0 || n_rows >= (1ull << 32) || nc == 0 || nc > MST_AUDIT_MAX_CURRENCIES || body_len >= (1ull << 32)) return hipErrorInvalidValue;
  const uint32_t n = (uint32_t)n_rows, tiles = mst_export_tiles(n_rows), groups = mst_export_groups(n_rows);
  uint32_t *tile_sum = d_work + mst_export_at_tiles(), *group_total = d_work + mst_export_at_groups(n_rows);
  mst_export_measure_kernel<<<export_blocks(n_rows), MST_EXPORT_THREADS, 0, stream>>>(body_len, d_leaf_name_spans, n, nc,
                                                                                static_cast<const fp_words*>(d_leaf_balances), d_row_off,
                                                                                tile_sum);
  mst_audit_groups_kernel<<<groups, MST_AUDIT_THREADS, 0, stream>>>(tile_sum, tiles, group_total);
  mst_export_offsets_kernel<<<export_blocks(n_rows), MST_EXPORT_THREADS, 0, stream>>>(d_row_off, n, tile_sum, group_total, d_work);
  return hipGetLastError();
}

hipError_t mst_export_write_launch(const uint8_t* d_body, uint64_t body_len, const uint32_t* d_leaf_name_spans, uint64_t n_rows, uint32_t nc,
                                   const void* d_leaf_balances, uint8_t delim, const uint32_t* d_row_off, uint64_t body_bytes, uint8_t* d_out,
                                   hipStream_t stream) {
  if (n_rows == 0 || n_rows >= (1ull << 32) || nc == 0 || nc > MST_AUDIT_MAX_CURRENCIES || body_len >= (1ull << 32) || body_bytes == 0 ||
      body_bytes >= (1ull << 32))
    return hipErrorInvalidValue;
  mst_export_write_tiles_kernel<<<export_blocks(n_rows), MST_EXPORT_THREADS, 0, stream>>>(
      d_body, body_len, d_leaf_name_spans, (uint32_t)n_rows, nc, static_cast<const fp_words*>(d_leaf_balances), delim, d_row_off, body_bytes, d_out);
  return hipGetLastError();
}

}  // namespace sg
