// Polynomial helpers, part 2 of 3 (included once by poly.hip, after poly_scan.cuh): the lookup
// argument's permuted columns for range tables.
#pragma once
#include "poly.h"
#include "side_prio.cuh"

namespace sg {

// ------------------------------------------------------------------ lookup permutation for range tables
// work layout (u32): hist_a[B] | hist_t[B] | pre_a[B] | pre_rep[B] | pre_left[B] | left[B]
__device__ __forceinline__ bool small_canonical(const fp_words* p, uint32_t* v) {
  f29 k = f29_zero();
  k.l[0] = 32;  // canonical = x~ * 2^5 * 2^-261
  uint32_t w[8];
  f29_to_words(f29_cond_sub_p<Fr29>(f29_mul<Fr29>(f29_load_r256<Fr29>(p), k)), w);
  *v = w[0];
  return !(w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) && w[0] < LOOKUP_BINS;
}
// Round 5: values below LOOKUP_LDS_BINS (every value of an 8-bit range table) are counted in the workgroup's LDS first and reach
// the global bins with one atomic per value the workgroup has seen -- most rows of a range check hold the same value (unused
// rows: 0), and 2 048 waves adding to ONE global word, even with one atomic per wave, were 44 us at 4 % VALU busy
// (profiles/r05z_proof_budget.json)
static constexpr uint32_t LOOKUP_LDS_BINS = 256;
__global__ void __launch_bounds__(256) lookup_permute_hist(const fp_words* __restrict__ input, const fp_words* __restrict__ table,
                                                           size_t rows, uint32_t* __restrict__ work, uint32_t* __restrict__ flag) {
  side_kernel_prio();
  __shared__ uint32_t s_a[LOOKUP_LDS_BINS], s_t[LOOKUP_LDS_BINS], s_max;
  s_a[threadIdx.x] = 0;
  s_t[threadIdx.x] = 0;
  if (threadIdx.x == 0) s_max = 0;
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < rows) {
    uint32_t a, t;
    if (!small_canonical(table + i, &t)) {
      atomicMax(flag, 2u);
    } else {
      if (t < LOOKUP_LDS_BINS) atomicAdd(&s_t[t], 1u);
      else atomicAdd(&work[LOOKUP_BINS + t], 1u);
      atomicMax(&s_max, t);   // highest table value: bounds the scans and searches below (a range table uses 256 of the 65536 bins)
      if (!small_canonical(input + i, &a)) {
        atomicMax(flag, 1u);
      } else {
        if (a < LOOKUP_LDS_BINS) atomicAdd(&s_a[a], 1u);
        else atomicAdd(&work[a], 1u);
      }
    }
  }
  __syncthreads();
  if (s_a[threadIdx.x]) atomicAdd(&work[threadIdx.x], s_a[threadIdx.x]);
  if (s_t[threadIdx.x]) atomicAdd(&work[LOOKUP_BINS + threadIdx.x], s_t[threadIdx.x]);
  if (threadIdx.x == 0 && s_max > *reinterpret_cast<volatile uint32_t*>(flag + 1)) atomicMax(flag + 1, s_max);
}
// one workgroup: three exclusive prefix sums over the bins (input counts, repeated rows, leftover table values)
__global__ void __launch_bounds__(1024) lookup_permute_scan(uint32_t* __restrict__ work, uint32_t* __restrict__ flag, uint32_t rows) {
  side_kernel_prio();
  __shared__ uint32_t s_sum[3][1024];
  const uint32_t bound = min(flag[1] + 1, LOOKUP_BINS), PER = (bound + 1023) / 1024;
  const uint32_t tid = threadIdx.x;
  uint32_t* hist_a = work;
  uint32_t* hist_t = work + LOOKUP_BINS;
  uint32_t* pre[3] = {work + 2 * LOOKUP_BINS, work + 3 * LOOKUP_BINS, work + 4 * LOOKUP_BINS};
  uint32_t* left = work + 5 * LOOKUP_BINS;
  uint32_t tot[3] = {0, 0, 0};
  bool missing = false;
  for (uint32_t j = 0; j < PER; j++) {
    const uint32_t v = tid * PER + j;
    if (v >= bound) break;
    const uint32_t ca = hist_a[v], ct = hist_t[v];
    const uint32_t used = ca ? 1u : 0u;
    missing = missing || ct < used;
    tot[0] += ca;
    tot[1] += ca - used;
    tot[2] += ct - min(ct, used);
  }
  if (missing) atomicMax(flag, 1u);
  for (int q = 0; q < 3; q++) s_sum[q][tid] = tot[q];
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {
    uint32_t add[3] = {0, 0, 0};
    if (tid >= d)
      for (int q = 0; q < 3; q++) add[q] = s_sum[q][tid - d];
    __syncthreads();
    for (int q = 0; q < 3; q++) s_sum[q][tid] += add[q];
    __syncthreads();
  }
  // an input above the table's maximum sits in a bin that was not scanned: the counts do not add up
  if (tid == 1023 && s_sum[0][1023] != rows) atomicMax(flag, 1u);
  uint32_t run[3];
  for (int q = 0; q < 3; q++) run[q] = s_sum[q][tid] - tot[q];
  for (uint32_t j = 0; j < PER; j++) {
    const uint32_t v = tid * PER + j;
    if (v >= bound) break;
    const uint32_t ca = hist_a[v], ct = hist_t[v];
    const uint32_t used = ca ? 1u : 0u, lf = ct - min(ct, used);
    pre[0][v] = run[0];
    pre[1][v] = run[1];
    pre[2][v] = run[2];
    left[v] = lf;
    run[0] += ca;
    run[1] += ca - used;
    run[2] += lf;
  }
}
// largest v with pre[v] <= x among the bins that own at least one element (count[v] > 0 and pre[v] <= x < pre[v] + count[v])
__device__ __forceinline__ uint32_t bin_of(const uint32_t* __restrict__ pre, const uint32_t* __restrict__ count, uint32_t x,
                                           uint32_t bound) {
  uint32_t lo = 0, hi = bound - 1;
  while (lo < hi) {   // last v with pre[v] <= x
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (pre[mid] <= x) lo = mid; else hi = mid - 1;
  }
  while (count[lo] == 0 && lo > 0) lo--;   // empty bins share their prefix with the owner before them
  return lo;
}
// opts (all optional): `clean` = the work space of the NEXT call on this stream, whose histograms and flag words this launch
// zeroes (2 * LOOKUP_BINS + 2 words at `clean`, the flag words first in clean_flag): no memset launches; `status` = where the
// call's verdict goes (0 ok, 1 an input not in the table, 2 table not a range table), e.g. mapped host memory; mont: the
// outputs in Montgomery form (otherwise canonical small integers, which the caller converts)
struct LookupWriteOpts {
  uint32_t* clean;
  uint32_t* clean_flag;
  uint32_t* status;
  uint32_t mont;
};
__global__ void __launch_bounds__(256) lookup_permute_write(size_t rows, const uint32_t* __restrict__ work,
                                                            const uint32_t* __restrict__ flag, fp_words* __restrict__ out_a,
                                                            fp_words* __restrict__ out_s, LookupWriteOpts o) {
  side_kernel_prio();
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o.clean) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t j = i; j < 2 * (size_t)LOOKUP_BINS; j += step) o.clean[j] = 0u;
    if (i < 2) o.clean_flag[i] = 0u;
  }
  const uint32_t verdict = flag[0];
  if (o.status && i == 0) {
    *reinterpret_cast<volatile uint32_t*>(o.status) = verdict;
    __threadfence_system();
  }
  if (i >= rows || verdict) return;   // flagged inputs: the caller discards the outputs
  const uint32_t bound = min(flag[1] + 1, LOOKUP_BINS);
  const uint32_t* hist_a = work;
  const uint32_t *pre_a = work + 2 * LOOKUP_BINS, *pre_rep = work + 3 * LOOKUP_BINS, *pre_left = work + 4 * LOOKUP_BINS,
                 *left = work + 5 * LOOKUP_BINS;
  const uint32_t v = bin_of(pre_a, hist_a, (uint32_t)i, bound);
  uint32_t s = v;
  const uint32_t within = (uint32_t)i - pre_a[v];
  if (within) s = bin_of(pre_left, left, pre_rep[v] + within - 1, bound);
  if (o.mont) {   // v * 2^256 mod r: what fr_montgomery(.., to_mont) makes of the canonical words
    f29 a = f29_zero(), b = f29_zero();
    a.l[0] = v;   // v, s < 2^16: one limb
    b.l[0] = s;
    const f29 k = f29_const<P>(P::r517);
    f29_store_canonical<P>(out_a + i, f29_mul<P>(a, k));
    f29_store_canonical<P>(out_s + i, f29_mul<P>(b, k));
    return;
  }
  fp_words w;   // canonical small integers; the caller converts both columns to Montgomery form
  w.q[0] = make_uint4(v, 0, 0, 0);
  w.q[1] = make_uint4(0, 0, 0, 0);
  out_a[i] = w;
  w.q[0].x = s;
  out_s[i] = w;
}
hipError_t poly_lookup_permute_small(const fp_words* d_input, const fp_words* d_table, size_t rows, uint32_t* d_work,
                                     fp_words* d_permuted_input, fp_words* d_permuted_table, uint32_t* d_flag,
                                     hipStream_t stream) {
  if (!rows) return hipSuccess;
  if (rows >= ((size_t)1 << 31)) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(d_work, 0, 2 * (size_t)LOOKUP_BINS * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(d_flag, 0, 2 * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  const unsigned blocks = (unsigned)((rows + 255) / 256);
  lookup_permute_hist<<<blocks, 256, 0, stream>>>(d_input, d_table, rows, d_work, d_flag);
  lookup_permute_scan<<<1, 1024, 0, stream>>>(d_work, d_flag, (uint32_t)rows);
  lookup_permute_write<<<blocks, 256, 0, stream>>>(rows, d_work, d_flag, d_permuted_input, d_permuted_table, LookupWriteOpts{nullptr, nullptr, nullptr, 0u});
  return hipGetLastError();
}
// the same without memsets, conversions or a copy back: d_work / d_flag must arrive zeroed (the previous call's write pass did it,
// or the allocation), d_next_work / d_next_flag are zeroed for the next call, *d_status receives the verdict, the outputs are
// Montgomery words
hipError_t poly_lookup_permute_small_chained(const fp_words* d_input, const fp_words* d_table, size_t rows, uint32_t* d_work,
                                             uint32_t* d_flag, uint32_t* d_next_work, uint32_t* d_next_flag, fp_words* d_permuted_input,
                                             fp_words* d_permuted_table, uint32_t* d_status, hipStream_t stream) {
  if (!rows) return hipSuccess;
  if (rows >= ((size_t)1 << 31)) return hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((rows + 255) / 256);
  lookup_permute_hist<<<blocks, 256, 0, stream>>>(d_input, d_table, rows, d_work, d_flag);
  lookup_permute_scan<<<1, 1024, 0, stream>>>(d_work, d_flag, (uint32_t)rows);
  lookup_permute_write<<<blocks, 256, 0, stream>>>(rows, d_work, d_flag, d_permuted_input, d_permuted_table,
                                                   LookupWriteOpts{d_next_work, d_next_flag, d_status, 1u});
  return hipGetLastError();
}

}  // namespace sg
