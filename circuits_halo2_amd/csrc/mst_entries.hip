// The leaves' inputs of a Merkle sum tree from what an exchange has -- usernames and decimal balances -- on the device: the
// GPU counterpart of `Entry::new` over a whole snapshot (mst_entries.h has the arithmetic and the references).  Both
// kernels trust their offsets: sg_mst_entries_dev (abi_mst.hip) validates them on the host before it launches, and the
// CSV reader's passes below (mst_csv.h has their rules) validate the spans they make before anything is hashed.  The sort of
// those spans by name and the lookup by name are mst_sort.cuh, included at the end.
#include "mst_entries.h"
#include "mst_csv.h"

#include "bn254_curve29.cuh"
#include "side_prio.cuh"

namespace sg {
SG_DEFINE_SIDE_PRIO_SETTER(mst_entries_set_side_prio)

static constexpr uint32_t MST_ENTRIES_BLOCK = 128;

__device__ __forceinline__ void store_zero(fp_words* p) {
  const uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  fp_words_store(p, z);
}

// Both kernels read item i from bytes[lo .. hi) in one of two forms chosen at compile time.  Back to back (sg_mst_entries_dev,
// sg_mst_update_dev): lo = begin[i], hi = begin[i + 1], n + 1 offsets.  Pairs (the CSV reader, whose fields lie where the file
// has them): hi = end[i].
template <bool PAIRS>
__device__ __forceinline__ uint64_t item_end(const uint64_t* __restrict__ begin, const uint64_t* __restrict__ end, uint64_t i) {
  return PAIRS ? end[i] : begin[i + 1];
}
// one thread per row: rows below n hash their name, the others are the zero entry's username, the field element 0
template <bool PAIRS>
__global__ void __launch_bounds__(MST_ENTRIES_BLOCK) mst_usernames_kernel(const uint8_t* __restrict__ bytes,
                                                                         const uint64_t* __restrict__ begin,
                                                                         const uint64_t* __restrict__ end, uint32_t n, uint32_t rows,
                                                                         fp_words* __restrict__ users) {
  side_kernel_prio();
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  if (i >= n) {
    store_zero(users + i);
    return;
  }
  const uint64_t lo = begin[i], hi = item_end<PAIRS>(begin, end, i);
  uint64_t digest[4];
  keccak256_lanes(bytes + lo, (size_t)(hi - lo), digest);
  uint32_t w[8];
  mst_username_words(digest, w);
  fp_words_store(users + i, w);
}

// one thread per balance field: fields below `fields` = n * nc fold their digits, the others are 0
template <bool PAIRS>
__global__ void __launch_bounds__(MST_ENTRIES_BLOCK) mst_balances_kernel(const uint8_t* __restrict__ bytes,
                                                                        const uint64_t* __restrict__ begin,
                                                                        const uint64_t* __restrict__ end, uint64_t fields,
                                                                        uint64_t total, fp_words* __restrict__ balances) {
  side_kernel_prio();
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= total) return;
  if (j >= fields) {
    store_zero(balances + j);
    return;
  }
  const uint64_t lo = begin[j], hi = item_end<PAIRS>(begin, end, j);
  uint32_t w[8];
  mst_decimal_words(bytes + lo, (size_t)(hi - lo), w);
  fp_words_store(balances + j, w);
}

template <bool PAIRS>
static hipError_t entries_launch(const uint8_t* d_name_bytes, const uint64_t* d_name_begin, const uint64_t* d_name_end,
                                 const uint8_t* d_digit_bytes, const uint64_t* d_digit_begin, const uint64_t* d_digit_end, size_t n,
                                 size_t rows, uint32_t nc, void* d_users, void* d_balances, hipStream_t stream) {
  const uint64_t total = (uint64_t)rows * nc;                // rows < 2^32, nc <= 64: at most 2^31 blocks
  mst_usernames_kernel<PAIRS><<<(unsigned)((rows + MST_ENTRIES_BLOCK - 1) / MST_ENTRIES_BLOCK), MST_ENTRIES_BLOCK, 0, stream>>>(
      d_name_bytes, d_name_begin, d_name_end, (uint32_t)n, (uint32_t)rows, static_cast<fp_words*>(d_users));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  mst_balances_kernel<PAIRS><<<(unsigned)((total + MST_ENTRIES_BLOCK - 1) / MST_ENTRIES_BLOCK), MST_ENTRIES_BLOCK, 0, stream>>>(
      d_digit_bytes, d_digit_begin, d_digit_end, (uint64_t)n * nc, total, static_cast<fp_words*>(d_balances));
  return hipGetLastError();
}
hipError_t mst_entries_launch(const uint8_t* d_name_bytes, const uint64_t* d_name_off, const uint8_t* d_digit_bytes,
                              const uint64_t* d_digit_off, size_t n, size_t rows, uint32_t nc, void* d_users, void* d_balances,
                              hipStream_t stream) {
  return entries_launch<false>(d_name_bytes, d_name_off, nullptr, d_digit_bytes, d_digit_off, nullptr, n, rows, nc, d_users, d_balances,
                               stream);
}
hipError_t mst_balances_launch(const uint8_t* d_digit_bytes, const uint64_t* d_digit_off, size_t fields, void* d_balances,
                               hipStream_t stream) {
  if (!fields) return hipSuccess;
  mst_balances_kernel<false><<<(unsigned)((fields + MST_ENTRIES_BLOCK - 1) / MST_ENTRIES_BLOCK), MST_ENTRIES_BLOCK, 0, stream>>>(
      d_digit_bytes, d_digit_off, nullptr, (uint64_t)fields, (uint64_t)fields, static_cast<fp_words*>(d_balances));
  return hipGetLastError();
}
hipError_t mst_csv_entries_launch(const uint8_t* d_body, const uint64_t* d_words, size_t n, size_t rows, uint32_t nc, void* d_users,
                                  void* d_balances, hipStream_t stream) {
  const MstCsvSpans s = mst_csv_spans(const_cast<uint64_t*>(d_words), n, nc);
  return entries_launch<true>(d_body, s.name_begin, s.name_end, d_body, s.bal_begin, s.bal_end, n, rows, nc, d_users, d_balances, stream);
}

// ------------------------------------------------------------------ the CSV reader's four passes (mst_csv.h)
static constexpr uint32_t MST_CSV_BLOCK = MST_CSV_TILE / 16;    // a lane takes 16 bytes of the tile
static_assert(MST_CSV_BLOCK == 256, "the passes' LDS arrays and wave counts are written for 256 lanes");

// What a lane sees of its 16 bytes at body[pos ..): bit j of `newline`, `forbidden` and `bare_cr` is byte j's.  Bytes behind the
// body's end are in no class.  One 16-byte load where the address allows it (the caller places the body on a 16-byte
// boundary), byte loads otherwise and in the body's last lane; the byte behind the 16 is read for the '\r' before it alone.
struct CsvLaneMasks {
  uint32_t newline, forbidden, bare_cr;
};
__device__ __forceinline__ CsvLaneMasks csv_lane_masks(const uint8_t* __restrict__ body, uint64_t len, uint64_t pos) {
  CsvLaneMasks m = {0, 0, 0};
  if (pos >= len) return m;
  const uint32_t valid = len - pos < 16 ? (uint32_t)(len - pos) : 16;
  uint8_t b[16];
  if (valid == 16 && (reinterpret_cast<uintptr_t>(body + pos) & 15) == 0) {
    const uint4 v = *reinterpret_cast<const uint4*>(body + pos);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) b[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
  } else {
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) b[j] = j < valid ? body[pos + j] : (uint8_t)'x';
  }
#pragma unroll
  for (uint32_t j = 0; j < 16; j++) {
    if (j >= valid) break;
    if (b[j] == '\n') m.newline |= 1u << j;
    if (mst_csv_forbidden(b[j])) m.forbidden |= 1u << j;
    if (b[j] == '\r') {
      const uint8_t next = j < 15 ? b[j + 1] : pos + 16 < len ? body[pos + 16] : (uint8_t)0;
      if (mst_csv_bare_cr(pos + j, len, next)) m.bare_cr |= 1u << j;
    }
  }
  return m;
}

// pass 1: tiles[tile] = the tile's newlines | its flags.  A wave counts byte slot j of its 64 lanes with one ballot.
__global__ void __launch_bounds__(MST_CSV_BLOCK) mst_csv_count_kernel(const uint8_t* __restrict__ body, uint64_t len,
                                                                     uint32_t* __restrict__ tiles) {
  side_kernel_prio();
  __shared__ uint32_t wave_word[MST_CSV_BLOCK / 64];
  const uint64_t pos = (uint64_t)blockIdx.x * MST_CSV_TILE + 16 * threadIdx.x;
  const CsvLaneMasks m = csv_lane_masks(body, len, pos);
  uint32_t word = 0;
#pragma unroll
  for (uint32_t j = 0; j < 16; j++) word += (uint32_t)__popcll(__ballot((m.newline >> j) & 1));
  if (__ballot(m.forbidden != 0)) word |= MST_CSV_FLAG_BYTE;
  if (__ballot(m.bare_cr != 0)) word |= MST_CSV_FLAG_BARE_CR;
  if ((threadIdx.x & 63) == 0) wave_word[threadIdx.x >> 6] = word;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t count = 0, flags = 0;
    for (uint32_t w = 0; w < MST_CSV_BLOCK / 64; w++) {
      count += wave_word[w] & MST_CSV_COUNT_MASK;
      flags |= wave_word[w] & ~MST_CSV_COUNT_MASK;
    }
    tiles[blockIdx.x] = count | flags;
  }
}

// inclusive prefix sums of one value per thread over the block, in `lds` (blockDim.x words); every thread calls it
__device__ __forceinline__ uint32_t block_inclusive_sum(uint32_t* lds, uint32_t v) {
  const uint32_t t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < blockDim.x; d <<= 1) {
    const uint32_t below = t >= d ? lds[t - d] : 0;
    __syncthreads();
    lds[t] += below;
    __syncthreads();
  }
  return lds[t];
}

// pass 2, one workgroup: tiles[t] becomes the number of newlines before tile t; tiles[n_tiles] the row count (a last row
// without a newline counts), tiles[n_tiles + 1] the flags of all tiles
__global__ void __launch_bounds__(MST_CSV_SCAN_BLOCK) mst_csv_scan_kernel(const uint8_t* __restrict__ body, uint64_t len,
                                                                         uint64_t n_tiles, uint32_t* __restrict__ tiles) {
  side_kernel_prio();
  __shared__ uint32_t lds[MST_CSV_SCAN_BLOCK];
  const uint32_t t = threadIdx.x;
  uint32_t before = 0, flags = 0;
  for (uint64_t first = 0; first < n_tiles; first += MST_CSV_SCAN_BLOCK) {
    const uint64_t i = first + t;
    const uint32_t word = i < n_tiles ? tiles[i] : 0;
    const uint32_t count = word & MST_CSV_COUNT_MASK;
    flags |= word & ~MST_CSV_COUNT_MASK;
    const uint32_t upto = block_inclusive_sum(lds, count);
    if (i < n_tiles) tiles[i] = before + upto - count;
    before += lds[MST_CSV_SCAN_BLOCK - 1];
    __syncthreads();                                         // the next round overwrites lds
  }
  lds[t] = flags;
  __syncthreads();
  for (uint32_t d = MST_CSV_SCAN_BLOCK / 2; d != 0; d >>= 1) {
    if (t < d) lds[t] |= lds[t + d];
    __syncthreads();
  }
  if (t == 0) {
    tiles[n_tiles] = (uint32_t)mst_csv_rows(body, len, before);
    tiles[n_tiles + 1] = lds[0];
  }
}

// pass 3: the newlines of a tile again, ranked by a prefix over the lanes' counts: row_start[before + rank + 1] = position + 1.
// n_rows is the caller's: nothing is written behind row_start[n_rows], whatever it is.
__global__ void __launch_bounds__(MST_CSV_BLOCK) mst_csv_row_starts_kernel(const uint8_t* __restrict__ body, uint64_t len,
                                                                          const uint32_t* __restrict__ tiles, uint64_t n_rows,
                                                                          uint64_t* __restrict__ row_start) {
  side_kernel_prio();
  __shared__ uint32_t lds[MST_CSV_BLOCK];
  const uint64_t pos = (uint64_t)blockIdx.x * MST_CSV_TILE + 16 * threadIdx.x;
  uint32_t newline = csv_lane_masks(body, len, pos).newline;
  const uint32_t count = (uint32_t)__popc(newline);
  uint64_t at = (uint64_t)tiles[blockIdx.x] + block_inclusive_sum(lds, count) - count + 1;
  while (newline) {
    const uint32_t j = (uint32_t)__ffs(newline) - 1;
    newline &= newline - 1;
    if (at <= n_rows) row_start[at] = pos + j + 1;
    at++;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    row_start[0] = 0;
    if (body[len - 1] != '\n') row_start[n_rows] = len + 1;   // the last row ends as if a newline stood behind the body
  }
}

// pass 4, a row per thread: its spans, or its problem into *problem, where the lowest (row, code) stays
__global__ void __launch_bounds__(MST_ENTRIES_BLOCK) mst_csv_split_kernel(const uint8_t* __restrict__ body, uint64_t len, uint8_t delim,
                                                                         uint32_t nc, uint64_t n_rows, uint64_t* __restrict__ words,
                                                                         unsigned long long* __restrict__ problem) {
  side_kernel_prio();
  const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_rows) return;
  uint64_t lo, hi;
  uint32_t code = MST_CSV_ROW_START;
  if (mst_csv_row_bounds(words, row, len, &lo, &hi)) code = mst_csv_split_row(body, lo, hi, delim, nc, row, mst_csv_spans(words, n_rows, nc));
  if (code != MST_CSV_OK) atomicMin(problem, (unsigned long long)mst_csv_problem_word(row, code));
}

hipError_t mst_csv_scan_launch(const uint8_t* d_body, uint64_t body_len, uint32_t* d_tiles, hipStream_t stream) {
  const uint64_t n_tiles = mst_csv_tiles(body_len);           // body_len < 2^32: at most 2^20 blocks
  if (n_tiles) {
    mst_csv_count_kernel<<<(unsigned)n_tiles, MST_CSV_BLOCK, 0, stream>>>(d_body, body_len, d_tiles);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  mst_csv_scan_kernel<<<1, MST_CSV_SCAN_BLOCK, 0, stream>>>(d_body, body_len, n_tiles, d_tiles);
  return hipGetLastError();
}
hipError_t mst_csv_split_launch(const uint8_t* d_body, uint64_t body_len, const uint32_t* d_tiles, uint8_t delim, uint32_t nc,
                                uint64_t n_rows, uint64_t* d_words, uint64_t* d_problem, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(d_problem, 0xff, 8, stream);   // MST_CSV_NO_PROBLEM
  if (e != hipSuccess) return e;
  mst_csv_row_starts_kernel<<<(unsigned)mst_csv_tiles(body_len), MST_CSV_BLOCK, 0, stream>>>(d_body, body_len, d_tiles, n_rows, d_words);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  mst_csv_split_kernel<<<(unsigned)((n_rows + MST_ENTRIES_BLOCK - 1) / MST_ENTRIES_BLOCK), MST_ENTRIES_BLOCK, 0, stream>>>(
      d_body, body_len, delim, nc, n_rows, d_words, reinterpret_cast<unsigned long long*>(d_problem));
  return hipGetLastError();
}

}  // namespace sg

#include "mst_sort.cuh"   // the sorted flavour: the names' order, the spans in leaf order, lookup by name
#include "mst_audit.cuh"  // the range audit of a built tree: flags, reason masks, the ordered list
#include "mst_names.cuh"  // the names beside a tree in file order: the spans in file order, the report of repeated names
#include "mst_diff.cuh"   // the next round's file against the tree: the join by name, the report, the changed balances packed
#include "mst_export.cuh" // the tree written back out as its snapshot CSV: the rows' lengths and positions, the bytes
#include "mst_admit.cuh"  // a round settled in full: new users into the padding, the index extended, the gone zeroed, one run
