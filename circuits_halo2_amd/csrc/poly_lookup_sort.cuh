// Polynomial helpers, part 2b (included once by poly.hip, after poly_lookup_permute.cuh): the lookup argument's permuted columns
// for ANY table -- full-width field elements, as every theta-compressed multi-column lookup and every table of hashes has.
//
// Both columns become canonical 8 x u32 keys, are sorted as integers, and the table is placed by the rule of the range-table
// kernels and of the compiled host prover: a first occurrence in A' takes the first table row of its value, the table values
// left over go in increasing integer order into the repeated rows in increasing row order.
//
// The sort is a stable LSD radix sort, 8 bits per pass (LS_DIGIT_BITS).  Why 8: the scatter ranks a key among its wave's keys
// of the same digit with one ballot per digit bit and keeps one LDS counter per wave and digit -- 8 ballots per key and 4 KiB
// of counters; 11 bits would save 9 of 32 passes but costs 32 KiB of counters per workgroup and a [2048][tile] table whose scan
// outweighs the tile's keys.  A pass whose digit is the same in every key of a column does nothing for that column (the keys
// launch reduces the OR of all keys and the OR of their complements: a bit varies when both have it): a range table costs one
// or two passes, a column of equal values none.  The host cannot know this without a wait, so all LS_PASSES passes are
// launched and a constant one returns at its first instruction; each column finds its ping-pong side from the same words.
//
// Ordering between the steps is by kernel boundaries alone: no spin waits, no last-workgroup hand-offs, no flags read inside
// the launch that sets them.
#pragma once
#include "poly.h"
#include "side_prio.cuh"

namespace sg {

// bits of word w (0 = lowest) that differ between two keys of column `col`
__device__ __forceinline__ uint32_t ls_varying_word(const uint32_t* __restrict__ head, uint32_t col, uint32_t w) {
  return head[col * 16 + w] & head[col * 16 + 8 + w];
}
__device__ __forceinline__ bool ls_pass_runs(const uint32_t* __restrict__ head, uint32_t col, uint32_t pass) {
  return ((ls_varying_word(head, col, pass >> 2) >> ((pass & 3) * 8)) & 0xffu) != 0;
}
// which of the column's two key arrays holds its keys before pass `pass` (LS_PASSES: after the last): every pass that runs swaps
__device__ __forceinline__ uint32_t ls_side(const uint32_t* __restrict__ head, uint32_t col, uint32_t pass) {
  uint32_t ran = 0;
  for (uint32_t w = 0; w < 8; w++) {
    const uint32_t v = ls_varying_word(head, col, w);
    for (uint32_t b = 0; b < 4; b++)
      if (4 * w + b < pass && ((v >> (8 * b)) & 0xffu)) ran++;
  }
  return ran & 1u;
}
__device__ __forceinline__ const fp_words* ls_keys(const fp_words* keys, uint32_t rows, uint32_t col, uint32_t side) {
  return keys + ((size_t)col * 2 + side) * rows;
}
__device__ __forceinline__ uint32_t ls_digit(const uint4& lo, const uint4& hi, uint32_t pass) {
  const uint4 q = (pass & 16) ? hi : lo;
  const uint32_t sel = (pass >> 2) & 3;
  const uint32_t w = sel == 0 ? q.x : sel == 1 ? q.y : sel == 2 ? q.z : q.w;
  return (w >> ((pass & 3) * 8)) & 0xffu;
}
// 254-bit compares from the top word down
__device__ __forceinline__ int ls_cmp4(const uint4& a, const uint4& b) {
  if (a.w != b.w) return a.w < b.w ? -1 : 1;
  if (a.z != b.z) return a.z < b.z ? -1 : 1;
  if (a.y != b.y) return a.y < b.y ? -1 : 1;
  if (a.x != b.x) return a.x < b.x ? -1 : 1;
  return 0;
}
__device__ __forceinline__ bool ls_same(const uint4& a, const uint4& b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }

// exclusive prefix of v over the workgroup's THREADS threads and the sum of all; s_w: THREADS / 64 words
template <uint32_t THREADS>
__device__ __forceinline__ uint32_t ls_block_scan(uint32_t v, uint32_t* s_w, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (uint32_t off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(inc, off);
    if (lane >= off) inc += t;
  }
  __syncthreads();   // s_w may still be read from the call before
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < THREADS / 64; w++) {
    const uint32_t x = s_w[w];
    if (w < wave) before += x;
    all += x;
  }
  *total = all;
  return before + inc - v;
}

// ------------------------------------------------------------------ keys
// grid (rows / 256, 2): column y's Montgomery words -> canonical integers (keys[y][0]); head[16 y ..]: OR of the keys, OR of their
// complements (one wave reduction, one LDS reduction, one atomic per workgroup and word); the table's blocks clear used[]
__global__ void __launch_bounds__(256) lookup_sort_keys(const fp_words* __restrict__ input, const fp_words* __restrict__ table,
                                                        uint32_t rows, fp_words* __restrict__ keys, uint32_t* __restrict__ head,
                                                        uint32_t* __restrict__ used) {
  side_kernel_prio();
  __shared__ uint32_t s_red[4][16];
  const uint32_t col = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t i = blockIdx.x * 256 + tid;
  uint32_t r[16];
#pragma unroll
  for (int k = 0; k < 16; k++) r[k] = 0;
  if (i < rows) {
    f29 k32 = f29_zero();
    k32.l[0] = 32;   // canonical = x~ * 2^5 * 2^-261 (any 256-bit word value: the residue's representative below r)
    uint32_t w[8];
    f29_to_words(f29_cond_sub_p<P>(f29_mul<P>(f29_load_r256<P>((col ? table : input) + i), k32)), w);
    fp_words_store(keys + (size_t)col * 2 * rows + i, w);
#pragma unroll
    for (int k = 0; k < 8; k++) {
      r[k] = w[k];
      r[8 + k] = ~w[k];
    }
    if (col) used[i] = 0;
  }
#pragma unroll
  for (int k = 0; k < 16; k++)
#pragma unroll
    for (uint32_t off = 32; off; off >>= 1) r[k] |= __shfl_xor(r[k], off);
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < 16; k++) s_red[wave][k] = r[k];
  __syncthreads();
  if (tid < 16) {
    const uint32_t v = s_red[0][tid] | s_red[1][tid] | s_red[2][tid] | s_red[3][tid];
    if (v) atomicOr(&head[col * 16 + tid], v);
  }
}

// ------------------------------------------------------------------ one pass: histogram, scan, scatter
// grid (tiles, 2): hist[y][digit][tile] = how many of the tile's keys hold `digit` at this pass
__global__ void __launch_bounds__(LS_THREADS) lookup_sort_hist(const fp_words* __restrict__ keys, uint32_t rows,
                                                               const uint32_t* __restrict__ head, uint32_t* __restrict__ hist,
                                                               uint32_t pass) {
  side_kernel_prio();
  const uint32_t col = blockIdx.y, tid = threadIdx.x;
  if (!ls_pass_runs(head, col, pass)) return;
  const fp_words* src = ls_keys(keys, rows, col, ls_side(head, col, pass));
  __shared__ uint32_t s_h[LS_BINS];
  s_h[tid] = 0;
  __syncthreads();
#pragma unroll
  for (uint32_t j = 0; j < LS_ITEMS; j++) {
    const uint32_t i = blockIdx.x * LS_TILE + j * LS_THREADS + tid;
    if (i < rows) {
      const uint4 q = src[i].q[pass >> 4];   // the 16-byte half that holds the digit
      atomicAdd(&s_h[ls_digit(q, q, pass)], 1u);
    }
  }
  __syncthreads();
  hist[((size_t)col * LS_BINS + tid) * gridDim.x + blockIdx.x] = s_h[tid];
}
// grid (1, 2): exclusive prefix sums over data[y * stride .. + len), in place; len's allocation is rounded up to 4 words.  The
// sort's table in [digit][tile] order (pass < LS_PASSES: nothing to do where the pass does not run), and the placement's tile sums
__global__ void __launch_bounds__(1024) lookup_sort_scan(uint32_t* __restrict__ data, uint32_t len, size_t stride,
                                                         const uint32_t* __restrict__ head, uint32_t pass) {
  side_kernel_prio();
  const uint32_t col = blockIdx.y, tid = threadIdx.x;
  if (pass < LS_PASSES && !ls_pass_runs(head, col, pass)) return;
  __shared__ uint32_t s_w[16];
  uint32_t* d = data + (size_t)col * stride;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < len; base += 4096) {
    const uint32_t idx = base + tid * 4;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (idx < len) {
      v = *reinterpret_cast<const uint4*>(d + idx);
      if (idx + 1 >= len) v.y = 0;
      if (idx + 2 >= len) v.z = 0;
      if (idx + 3 >= len) v.w = 0;
    }
    uint32_t total;
    const uint32_t at = carry + ls_block_scan<1024>(v.x + v.y + v.z + v.w, s_w, &total);
    if (idx < len) *reinterpret_cast<uint4*>(d + idx) = make_uint4(at, at + v.x, at + v.x + v.y, at + v.x + v.y + v.z);
    carry += total;
  }
}
// grid (tiles, 2): the tile's keys go to hist[y][digit][tile] (scanned: where the tile's first key of that digit belongs) plus
// their rank among the tile's keys of the same digit.  Tile order is (wave, round, lane); a key's rank is what its wave's counter
// of the digit held before the round plus the lanes below it with the same digit -- stable.
__global__ void __launch_bounds__(LS_THREADS) lookup_sort_scatter(fp_words* __restrict__ keys, uint32_t rows,
                                                                  const uint32_t* __restrict__ head,
                                                                  const uint32_t* __restrict__ hist, uint32_t pass) {
  side_kernel_prio();
  const uint32_t col = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (!ls_pass_runs(head, col, pass)) return;
  const uint32_t side = ls_side(head, col, pass);
  const fp_words* src = ls_keys(keys, rows, col, side);
  fp_words* dst = keys + ((size_t)col * 2 + (side ^ 1u)) * rows;
  __shared__ uint32_t s_cnt[LS_THREADS / 64][LS_BINS];
#pragma unroll
  for (uint32_t w = 0; w < LS_THREADS / 64; w++) s_cnt[w][tid] = 0;
  __syncthreads();
  uint4 lo[LS_ITEMS], hi[LS_ITEMS];
  uint32_t digit[LS_ITEMS], rank[LS_ITEMS];
  const uint64_t below = ((uint64_t)1 << lane) - 1;
#pragma unroll
  for (uint32_t j = 0; j < LS_ITEMS; j++) {
    const uint32_t i = blockIdx.x * LS_TILE + wave * (64 * LS_ITEMS) + j * 64 + lane;
    const bool valid = i < rows;
    lo[j] = hi[j] = make_uint4(0, 0, 0, 0);
    if (valid) {
      lo[j] = src[i].q[0];
      hi[j] = src[i].q[1];
    }
    digit[j] = ls_digit(lo[j], hi[j], pass);
    uint64_t peers = __ballot(valid);   // the wave's keys of this round with my digit
#pragma unroll
    for (uint32_t b = 0; b < LS_DIGIT_BITS; b++) {
      const bool bit = (digit[j] >> b) & 1u;
      const uint64_t set = __ballot(valid && bit);
      peers &= bit ? set : ~set;
    }
    const uint32_t leader = valid ? (uint32_t)__ffsll((unsigned long long)peers) - 1 : lane;
    uint32_t prior = 0;
    if (valid && lane == leader) prior = atomicAdd(&s_cnt[wave][digit[j]], (uint32_t)__popcll(peers));
    prior = __shfl(prior, leader);
    rank[j] = prior + (uint32_t)__popcll(peers & below);
  }
  __syncthreads();
  {   // counters -> where the wave's first key of digit `tid` goes
    uint32_t at = hist[((size_t)col * LS_BINS + tid) * gridDim.x + blockIdx.x];
#pragma unroll
    for (uint32_t w = 0; w < LS_THREADS / 64; w++) {
      const uint32_t c = s_cnt[w][tid];
      s_cnt[w][tid] = at;
      at += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t j = 0; j < LS_ITEMS; j++) {
    const uint32_t i = blockIdx.x * LS_TILE + wave * (64 * LS_ITEMS) + j * 64 + lane;
    const uint32_t to = s_cnt[wave][digit[j]] + rank[j];
    if (i < rows && to < rows) {
      dst[to].q[0] = lo[j];
      dst[to].q[1] = hi[j];
    }
  }
}

// ------------------------------------------------------------------ placement
// row i of the sorted input: repeat[i] = (A'[i] == A'[i-1]); a first row looks its value up in the sorted table (lower bound: the
// first table row of that value) and marks that row used, or raises the verdict.  Distinct values hit distinct rows: plain stores.
__global__ void __launch_bounds__(256) lookup_sort_mark(const fp_words* __restrict__ keys, uint32_t rows, uint32_t* __restrict__ head,
                                                        uint32_t* __restrict__ used, uint32_t* __restrict__ repeat) {
  side_kernel_prio();
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows) return;
  const fp_words* a = ls_keys(keys, rows, 0, ls_side(head, 0, LS_PASSES));
  const fp_words* t = ls_keys(keys, rows, 1, ls_side(head, 1, LS_PASSES));
  const uint4 lo = a[i].q[0], hi = a[i].q[1];
  const bool rep = i > 0 && ls_same(a[i - 1].q[1], hi) && ls_same(a[i - 1].q[0], lo);
  repeat[i] = rep ? 1u : 0u;
  if (rep) return;
  uint32_t first = 0, end = rows;   // first table row whose key is not below mine
  while (first < end) {
    const uint32_t mid = (first + end) >> 1;
    int c = ls_cmp4(t[mid].q[1], hi);
    if (c == 0) c = ls_cmp4(t[mid].q[0], lo);
    if (c < 0) first = mid + 1; else end = mid;
  }
  if (first < rows && ls_same(t[first].q[1], hi) && ls_same(t[first].q[0], lo)) used[first] = 1u;
  else atomicMax(&head[LS_FLAG], 1u);
}
// grid (tiles, 2) over the flags repeat[] (y = 0) and !used[] (y = 1), LS_ITEMS consecutive rows per thread.  write = 0:
// sums[y][tile] = the tile's count.  write = 1 (sums scanned): rank[i] = repeated rows before input row i; left[n] = the n-th
// table row that no first row took.
__global__ void __launch_bounds__(LS_THREADS) lookup_sort_flags(uint32_t rows, const uint32_t* __restrict__ used,
                                                                const uint32_t* __restrict__ repeat, uint32_t* __restrict__ sums,
                                                                size_t sums_stride, uint32_t* __restrict__ rank,
                                                                uint32_t* __restrict__ left, uint32_t write) {
  side_kernel_prio();
  __shared__ uint32_t s_w[LS_THREADS / 64];
  const uint32_t y = blockIdx.y, i0 = blockIdx.x * LS_TILE + threadIdx.x * LS_ITEMS;
  uint32_t f[LS_ITEMS], mine = 0;
#pragma unroll
  for (uint32_t k = 0; k < LS_ITEMS; k++) {
    f[k] = 0;
    if (i0 + k < rows) f[k] = y ? 1u - used[i0 + k] : repeat[i0 + k];
    mine += f[k];
  }
  uint32_t total;
  uint32_t at = ls_block_scan<LS_THREADS>(mine, s_w, &total);
  uint32_t* tile_sum = sums + y * sums_stride + blockIdx.x;
  if (!write) {
    if (threadIdx.x == 0) *tile_sum = total;
    return;
  }
  at += *tile_sum;
#pragma unroll
  for (uint32_t k = 0; k < LS_ITEMS; k++) {
    if (i0 + k < rows) {
      if (!y) rank[i0 + k] = at;
      else if (f[k] && at < rows) left[at] = i0 + k;
    }
    at += f[k];
  }
}
// the verdict goes to *status (optional; e.g. mapped host memory); under verdict 0 both columns are written as Montgomery words:
// a first row takes its own value, repeated row i the leftover table value number rank[i]
__global__ void __launch_bounds__(256) lookup_sort_write(const fp_words* __restrict__ keys, uint32_t rows, const uint32_t* __restrict__ head,
                                                         const uint32_t* __restrict__ repeat, const uint32_t* __restrict__ rank,
                                                         const uint32_t* __restrict__ left, fp_words* __restrict__ out_a,
                                                         fp_words* __restrict__ out_s, uint32_t* status) {
  side_kernel_prio();
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const uint32_t verdict = head[LS_FLAG];
  if (status && i == 0) {
    *reinterpret_cast<volatile uint32_t*>(status) = verdict;
    __threadfence_system();
  }
  if (i >= rows || verdict) return;   // flagged inputs: the caller discards the outputs
  const fp_words* a = ls_keys(keys, rows, 0, ls_side(head, 0, LS_PASSES));
  const fp_words* t = ls_keys(keys, rows, 1, ls_side(head, 1, LS_PASSES));
  uint32_t wa[8], ws[8];
  fp_words_load(a + i, wa);
  uint32_t from = rows;
  if (repeat[i] && rank[i] < rows) from = left[rank[i]];
  if (from < rows) {
    fp_words_load(t + from, ws);
  } else {
#pragma unroll
    for (int k = 0; k < 8; k++) ws[k] = wa[k];
  }
  const f29 k = f29_const<P>(P::r517);   // v * 2^256 mod r: what fr_montgomery(.., to_mont) makes of the canonical words
  f29_store_canonical<P>(out_a + i, f29_mul<P>(f29_from_words<0>(wa), k));
  f29_store_canonical<P>(out_s + i, f29_mul<P>(f29_from_words<0>(ws), k));
}

hipError_t poly_lookup_permute(const fp_words* d_input, const fp_words* d_table, size_t rows, uint32_t* d_work,
                               fp_words* d_permuted_input, fp_words* d_permuted_table, uint32_t* d_status, hipStream_t stream) {
  if (!rows) return hipSuccess;
  if (rows > LS_MAX_ROWS) return hipErrorInvalidValue;
  const LookupSortLayout l = lookup_sort_layout(rows);
  const uint32_t n = (uint32_t)rows, tiles = (uint32_t)lookup_sort_tiles(rows), blocks = (n + 255) / 256;
  uint32_t* head = d_work;
  fp_words* keys = reinterpret_cast<fp_words*>(d_work + l.keys);
  uint32_t *hist = d_work + l.hist, *used = d_work + l.used, *repeat = d_work + l.repeat, *rank = d_work + l.rank, *left = d_work + l.left,
           *sums = d_work + l.sums;
  hipError_t e = hipMemsetAsync(head, 0, LS_HEAD_WORDS * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  lookup_sort_keys<<<dim3(blocks, 2), 256, 0, stream>>>(d_input, d_table, n, keys, head, used);
  for (uint32_t pass = 0; pass < LS_PASSES; pass++) {
    lookup_sort_hist<<<dim3(tiles, 2), LS_THREADS, 0, stream>>>(keys, n, head, hist, pass);
    lookup_sort_scan<<<dim3(1, 2), 1024, 0, stream>>>(hist, LS_BINS * tiles, (size_t)LS_BINS * tiles, head, pass);
    lookup_sort_scatter<<<dim3(tiles, 2), LS_THREADS, 0, stream>>>(keys, n, head, hist, pass);
  }
  lookup_sort_mark<<<blocks, 256, 0, stream>>>(keys, n, head, used, repeat);
  lookup_sort_flags<<<dim3(tiles, 2), LS_THREADS, 0, stream>>>(n, used, repeat, sums, l.sums_stride, rank, left, 0u);
  lookup_sort_scan<<<dim3(1, 2), 1024, 0, stream>>>(sums, tiles, l.sums_stride, head, LS_PASSES);
  lookup_sort_flags<<<dim3(tiles, 2), LS_THREADS, 0, stream>>>(n, used, repeat, sums, l.sums_stride, rank, left, 1u);
  lookup_sort_write<<<blocks, 256, 0, stream>>>(keys, n, head, repeat, rank, left, d_permuted_input, d_permuted_table, d_status);
  return hipGetLastError();
}

}  // namespace sg
