// The leaves' inputs, part 2 (included once by mst_entries.hip, behind the CSV reader's passes): a snapshot's usernames sorted
// where the file's text lies, and looked up there (mst_sort.h has the rules, the work space and the host mirror).  A sibling of
// the lookup sort's 8-bit pass (poly_lookup_sort.cuh), which moves 256-bit keys: here the row index alone moves, and a row's
// digit is read from the text through its span.  The kernels trust the spans: the CSV reader's split made them and the caller
// read its problem word before any of these is launched.
#pragma once
#include "mst_sort.h"
#include "side_prio.cuh"

namespace sg {

static constexpr uint32_t MST_SORT_WAVES = MST_SORT_THREADS / 64;
static_assert(MST_SORT_SCAN_ITEMS == 4, "a thread of the scan loads and stores one uint4 a step");

// lengths, a row per thread: a name over the cap reports (row, 7) -- a row the split reported keeps its lower code under the
// minimum, and one whose name span it left unwritten has the zeros the caller put there -- else the longest name grows
__global__ void __launch_bounds__(MST_SORT_THREADS) mst_sort_lengths_kernel(const uint64_t* __restrict__ name_begin,
                                                                           const uint64_t* __restrict__ name_end, uint64_t n,
                                                                           uint32_t* __restrict__ result) {
  side_kernel_prio();
  const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t len = 0;
  if (row < n) {
    const uint64_t l = name_end[row] - name_begin[row];
    if (mst_sort_name_too_long(l))
      atomicMin(reinterpret_cast<unsigned long long*>(result + MST_SORT_AT_PROBLEM),
                (unsigned long long)mst_csv_problem_word(row, MST_SORT_NAME_TOO_LONG));
    else
      len = (uint32_t)l;
  }
#pragma unroll
  for (uint32_t off = 32; off; off >>= 1) {
    const uint32_t other = __shfl_xor(len, off);
    len = other > len ? other : len;
  }
  if ((threadIdx.x & 63) == 0 && len) atomicMax(result + MST_SORT_AT_LONGEST, len);
}

// head, a row per thread: its padded name as MST_SORT_KEY_WORDS words into the OR of all keys and the OR of their complements
// (one wave reduction, one LDS reduction, one atomic per workgroup and word); order[0][row] = row
__global__ void __launch_bounds__(MST_SORT_THREADS) mst_sort_head_kernel(const uint8_t* __restrict__ body,
                                                                        const uint64_t* __restrict__ name_begin,
                                                                        const uint64_t* __restrict__ name_end, uint32_t n,
                                                                        uint32_t* __restrict__ head, uint32_t* __restrict__ order) {
  side_kernel_prio();
  __shared__ uint32_t s_red[MST_SORT_WAVES][2 * MST_SORT_KEY_WORDS];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t row = blockIdx.x * MST_SORT_THREADS + tid;
  uint32_t key[MST_SORT_KEY_WORDS], inv[MST_SORT_KEY_WORDS];
#pragma unroll
  for (uint32_t w = 0; w < MST_SORT_KEY_WORDS; w++) key[w] = inv[w] = 0;
  if (row < n) {
    const uint64_t begin = name_begin[row], end = name_end[row];
#pragma unroll
    for (uint32_t w = 0; w < MST_SORT_KEY_WORDS; w++) {
      if (begin + 4 * w < end) {                             // (the words behind the name stay 0)
#pragma unroll
        for (uint32_t b = 0; b < 4; b++) key[w] |= mst_sort_digit(body, begin, end, 4 * w + b) << (8 * b);
      }
      inv[w] = ~key[w];
    }
    order[row] = row;
  }
#pragma unroll
  for (uint32_t w = 0; w < MST_SORT_KEY_WORDS; w++)
#pragma unroll
    for (uint32_t off = 32; off; off >>= 1) {
      key[w] |= __shfl_xor(key[w], off);
      inv[w] |= __shfl_xor(inv[w], off);
    }
  if (lane == 0)
#pragma unroll
    for (uint32_t w = 0; w < MST_SORT_KEY_WORDS; w++) {
      s_red[wave][w] = key[w];
      s_red[wave][MST_SORT_KEY_WORDS + w] = inv[w];
    }
  __syncthreads();
  if (tid < 2 * MST_SORT_KEY_WORDS) {
    uint32_t v = 0;
#pragma unroll
    for (uint32_t w = 0; w < MST_SORT_WAVES; w++) v |= s_red[w][tid];
    if (v) atomicOr(&head[tid], v);
  }
}

// the digit of the row at place i of the order's side `src`, position pos
__device__ __forceinline__ uint32_t sort_digit_at(const uint8_t* __restrict__ body, const uint64_t* __restrict__ name_begin,
                                                  const uint64_t* __restrict__ name_end, uint32_t n, uint32_t row, uint32_t pos) {
  return row < n ? mst_sort_digit(body, name_begin[row], name_end[row], pos) : 0u;
}

// one workgroup per tile: hist[digit][tile] = how many of the tile's rows hold `digit` at position pos
__global__ void __launch_bounds__(MST_SORT_THREADS) mst_sort_hist_kernel(const uint8_t* __restrict__ body,
                                                                        const uint64_t* __restrict__ name_begin,
                                                                        const uint64_t* __restrict__ name_end, uint32_t n,
                                                                        const uint32_t* __restrict__ head,
                                                                        const uint32_t* __restrict__ order, uint32_t side_words,
                                                                        uint32_t* __restrict__ hist, uint32_t pos) {
  side_kernel_prio();
  if (!mst_sort_varies(head, pos)) return;
  const uint32_t tid = threadIdx.x;
  const uint32_t* src = order + (size_t)mst_sort_side(head, pos) * side_words;
  __shared__ uint32_t s_h[MST_SORT_BINS];
  s_h[tid] = 0;
  __syncthreads();
#pragma unroll
  for (uint32_t j = 0; j < MST_SORT_ITEMS; j++) {
    const uint32_t i = blockIdx.x * MST_SORT_TILE + j * MST_SORT_THREADS + tid;
    if (i < n) atomicAdd(&s_h[sort_digit_at(body, name_begin, name_end, n, src[i], pos)], 1u);
  }
  __syncthreads();
  hist[(size_t)tid * gridDim.x + blockIdx.x] = s_h[tid];
}

// exclusive prefix of v over the workgroup's THREADS threads and the sum of all; s_w: THREADS / 64 words
template <uint32_t THREADS>
__device__ __forceinline__ uint32_t sort_block_scan(uint32_t v, uint32_t* s_w, uint32_t* total) {
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
// one workgroup: exclusive prefix sums over hist[0 .. len), in place; len is a multiple of 4 and hist lies on a 16-byte boundary
__global__ void __launch_bounds__(MST_SORT_SCAN_BLOCK) mst_sort_scan_kernel(uint32_t* __restrict__ hist, uint32_t len,
                                                                           const uint32_t* __restrict__ head, uint32_t pos) {
  side_kernel_prio();
  if (!mst_sort_varies(head, pos)) return;
  __shared__ uint32_t s_w[MST_SORT_SCAN_BLOCK / 64];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < len; base += MST_SORT_SCAN_ITEMS * MST_SORT_SCAN_BLOCK) {
    const uint32_t idx = base + threadIdx.x * MST_SORT_SCAN_ITEMS;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (idx < len) v = *reinterpret_cast<const uint4*>(hist + idx);
    uint32_t total;
    const uint32_t at = carry + sort_block_scan<MST_SORT_SCAN_BLOCK>(v.x + v.y + v.z + v.w, s_w, &total);
    if (idx < len) *reinterpret_cast<uint4*>(hist + idx) = make_uint4(at, at + v.x, at + v.x + v.y, at + v.x + v.y + v.z);
    carry += total;
  }
}

// One workgroup per tile: a row goes to hist[digit][tile] (scanned: where the tile's first row of that digit belongs) plus its
// rank among the tile's rows of the same digit.  Tile order is (wave, round, lane), which is the order of the places; a row's
// rank is what its wave's counter of the digit held before the round plus the lanes below it with the same digit -- stable.
__global__ void __launch_bounds__(MST_SORT_THREADS) mst_sort_scatter_kernel(const uint8_t* __restrict__ body,
                                                                           const uint64_t* __restrict__ name_begin,
                                                                           const uint64_t* __restrict__ name_end, uint32_t n,
                                                                           const uint32_t* __restrict__ head,
                                                                           uint32_t* __restrict__ order, uint32_t side_words,
                                                                           const uint32_t* __restrict__ hist, uint32_t pos) {
  side_kernel_prio();
  if (!mst_sort_varies(head, pos)) return;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t side = mst_sort_side(head, pos);
  const uint32_t* src = order + (size_t)side * side_words;
  uint32_t* dst = order + (size_t)(side ^ 1u) * side_words;
  __shared__ uint32_t s_cnt[MST_SORT_WAVES][MST_SORT_BINS];
#pragma unroll
  for (uint32_t w = 0; w < MST_SORT_WAVES; w++) s_cnt[w][tid] = 0;
  __syncthreads();
  uint32_t row[MST_SORT_ITEMS], digit[MST_SORT_ITEMS], rank[MST_SORT_ITEMS];
  const uint64_t below = ((uint64_t)1 << lane) - 1;
#pragma unroll
  for (uint32_t j = 0; j < MST_SORT_ITEMS; j++) {
    const uint32_t i = blockIdx.x * MST_SORT_TILE + wave * (64 * MST_SORT_ITEMS) + j * 64 + lane;
    const bool valid = i < n;
    row[j] = valid ? src[i] : n;
    digit[j] = sort_digit_at(body, name_begin, name_end, n, row[j], pos);
    uint64_t peers = __ballot(valid);   // the wave's rows of this round with my digit
#pragma unroll
    for (uint32_t b = 0; b < 8; b++) {
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
  {   // counters -> where the wave's first row of digit `tid` goes
    uint32_t at = hist[(size_t)tid * gridDim.x + blockIdx.x];
#pragma unroll
    for (uint32_t w = 0; w < MST_SORT_WAVES; w++) {
      const uint32_t c = s_cnt[w][tid];
      s_cnt[w][tid] = at;
      at += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t j = 0; j < MST_SORT_ITEMS; j++) {
    const uint32_t i = blockIdx.x * MST_SORT_TILE + wave * (64 * MST_SORT_ITEMS) + j * 64 + lane;
    const uint32_t to = s_cnt[wave][digit[j]] + rank[j];
    if (i < n && to < n) dst[to] = row[j];
  }
}

// gather, a field per thread: field f of leaf i is field f of file row order[i] (0 the name, 1 + c balance c), written into the
// second block of spans; the name's thread also writes order_out[i] and the name's span as two 32-bit words
__global__ void __launch_bounds__(MST_SORT_THREADS) mst_sort_gather_kernel(const uint32_t* __restrict__ head,
                                                                          const uint32_t* __restrict__ order, uint32_t side_words,
                                                                          MstCsvSpans from, MstCsvSpans to, uint32_t n, uint32_t nc,
                                                                          uint32_t* __restrict__ order_out,
                                                                          uint32_t* __restrict__ name_spans) {
  side_kernel_prio();
  const uint64_t at = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t fields = nc + 1;
  const uint64_t i = at / fields;
  const uint32_t f = (uint32_t)(at % fields);
  if (i >= n) return;
  const uint32_t row = order[(size_t)mst_sort_final_side(head) * side_words + i];
  if (row >= n) return;
  if (f == 0) {
    const uint64_t b = from.name_begin[row], e = from.name_end[row];
    to.name_begin[i] = b;
    to.name_end[i] = e;
    order_out[i] = row;
    name_spans[2 * i] = (uint32_t)b;
    name_spans[2 * i + 1] = (uint32_t)e;
  } else {
    to.bal_begin[i * nc + f - 1] = from.bal_begin[(uint64_t)row * nc + f - 1];
    to.bal_end[i * nc + f - 1] = from.bal_end[(uint64_t)row * nc + f - 1];
  }
}

// find, a query per thread; with an order the position found answers as the file row that stands there
__global__ void __launch_bounds__(MST_SORT_THREADS) mst_find_names_kernel(const uint8_t* __restrict__ body, uint64_t body_len,
                                                                         const uint32_t* __restrict__ name_spans,
                                                                         const uint32_t* __restrict__ order, uint32_t n,
                                                                         const uint8_t* __restrict__ query,
                                                                         const uint64_t* __restrict__ query_off, uint64_t m,
                                                                         uint32_t* __restrict__ out) {
  side_kernel_prio();
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const uint64_t lo = query_off[j], hi = query_off[j + 1];
  const uint32_t at = mst_find_name(body, body_len, name_spans, n, query + lo, hi - lo);
  out[j] = order && at != MST_FIND_ABSENT ? order[at] : at;   // at < n where it is not MST_FIND_ABSENT
}

static unsigned blocks_for(uint64_t threads) { return (unsigned)((threads + MST_SORT_THREADS - 1) / MST_SORT_THREADS); }

hipError_t mst_sort_lengths_launch(const uint64_t* d_words, uint64_t n_rows, uint32_t nc, uint32_t* d_result, hipStream_t stream) {
  const MstCsvSpans s = mst_csv_spans(const_cast<uint64_t*>(d_words), n_rows, nc);
  mst_sort_lengths_kernel<<<blocks_for(n_rows), MST_SORT_THREADS, 0, stream>>>(s.name_begin, s.name_end, n_rows, d_result);
  return hipGetLastError();
}

hipError_t mst_sort_launch(const uint8_t* d_body, const uint64_t* d_words, uint64_t n_rows, uint32_t nc, uint32_t longest,
                           uint32_t* d_work, uint32_t* d_order, uint32_t* d_name_spans, uint64_t* d_sorted_words, hipStream_t stream) {
  if (n_rows == 0 || n_rows >= (1ull << 32) || longest > MST_SORT_NAME_CAP) return hipErrorInvalidValue;
  const uint32_t n = (uint32_t)n_rows, tiles = (uint32_t)mst_sort_tiles(n_rows), side_words = (uint32_t)mst_sort_side_words(n_rows);
  const MstCsvSpans from = mst_csv_spans(const_cast<uint64_t*>(d_words), n_rows, nc);
  const MstCsvSpans to = mst_csv_spans(d_sorted_words, n_rows, nc);
  uint32_t *head = d_work + MST_SORT_AT_HEAD, *order = d_work + mst_sort_at_order(n_rows, 0), *hist = d_work + mst_sort_at_hist(n_rows);
  mst_sort_head_kernel<<<blocks_for(n_rows), MST_SORT_THREADS, 0, stream>>>(d_body, from.name_begin, from.name_end, n, head, order);
  hipError_t e = hipGetLastError();
  for (uint32_t pos = longest; e == hipSuccess && pos-- != 0;) {
    mst_sort_hist_kernel<<<tiles, MST_SORT_THREADS, 0, stream>>>(d_body, from.name_begin, from.name_end, n, head, order, side_words, hist, pos);
    mst_sort_scan_kernel<<<1, MST_SORT_SCAN_BLOCK, 0, stream>>>(hist, MST_SORT_BINS * tiles, head, pos);
    mst_sort_scatter_kernel<<<tiles, MST_SORT_THREADS, 0, stream>>>(d_body, from.name_begin, from.name_end, n, head, order, side_words, hist, pos);
    e = hipGetLastError();
  }
  if (e != hipSuccess) return e;
  mst_sort_gather_kernel<<<blocks_for(n_rows * (nc + 1ull)), MST_SORT_THREADS, 0, stream>>>(head, order, side_words, from, to, n, nc, d_order,
                                                                                           d_name_spans);
  return hipGetLastError();
}

hipError_t mst_find_names_launch(const uint8_t* d_body, uint64_t body_len, const uint32_t* d_name_spans, const uint32_t* d_order,
                                 uint32_t n_rows, const uint8_t* d_query, const uint64_t* d_query_off, size_t m, uint32_t* d_out,
                                 hipStream_t stream) {
  mst_find_names_kernel<<<blocks_for(m), MST_SORT_THREADS, 0, stream>>>(d_body, body_len, d_name_spans, d_order, n_rows, d_query, d_query_off,
                                                                        m, d_out);
  return hipGetLastError();
}

}  // namespace sg
