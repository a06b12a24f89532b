// Device-resident polynomial helpers around the MSM/NTT hot path (the
// first "next" row that needs no circuit knowledge): halo2's `eval_polynomial` (the 35
// evaluations of create_proof step 11), `BatchInvert::batch_invert` and the exclusive prefix
// product the permutation / lookup grand products are built from (steps 5-6).  With these the
// vectors that feed the commitments never leave HBM between an NTT and an MSM.
//
// All vectors: n x 32 B Fr, Montgomery-2^256 words (halo2curves layout); arithmetic on
// 9 x 29-bit limbs (bn254_f29.cuh) in the 2^261 domain.
//
// This file: evaluation, batch inversion, the element-wise product, the canonical-range check and the linear combinations, each
// launch function under its kernels.  poly_scan.cuh: the shared device helpers, prefix product, grand products, Kate division;
// poly_lookup_permute.cuh (range tables), poly_lookup_sort.cuh (any table); poly_random.cuh.  The host geometry of all of them is in poly_plan.h.
#include "poly.h"
#include "side_prio.cuh"

#include "poly_scan.cuh"
#include "poly_lookup_permute.cuh"
#include "poly_lookup_sort.cuh"
#include "poly_random.cuh"

namespace sg {
SG_DEFINE_SIDE_PRIO_SETTER(poly_set_side_prio)

// ---- eval_polynomial: sum_i c[i] x^i ------------------------------------------------------
// thread: Horner over CH consecutive coefficients; workgroup: pairwise fold with x^(CH*2^l);
// one partial per workgroup, folded again by the same kernel until one value is left.
// Coefficients and the running value stay in the memory (2^256) domain, only x is in the 2^261 domain: acc~ * x^ * 2^-261 =
// (acc x)~, so no coefficient is converted.  16 coefficients per thread in the batched path (32 workgroups per 2^17-term
// polynomial: the 40 evaluations of a proof fill the chip); longer polynomials (> 2^24 terms, where two levels of 2^12 no longer
// reach) and the single-polynomial path take 32 per thread.
template <uint32_t EV_CH>
__device__ __forceinline__ void eval_poly_block(const fp_words* __restrict__ c, uint32_t n, const words8& xw,
                                                uint32_t log_stride, fp_words* __restrict__ out,
                                                uint32_t (*sh)[9]) {
  // element i of this level has weight x^(i << log_stride)
  const uint32_t tid = threadIdx.x;
  f29 x = f29_words_to_r261<P>(xw.l);
  for (uint32_t k = 0; k < log_stride; k++) x = f29_sqr<P>(x);   // x^(2^log_stride)
  // Round 5: a workgroup's EV_CH * 256 coefficients are read COALESCED -- thread t takes the elements t, t + 256, t + 512, ...
  // of the block and runs Horner in y = x^256 over them; the fold below then pairs neighbours with x, x^2, x^4, ... x^128.
  // (Sixteen CONSECUTIVE coefficients per thread made every load instruction touch 64 different 512-byte-strided sectors: 42 % VALU
  // busy at a fifth of the memory rate, profiles/r05a_proof_budget.json.)  The powers x^(2^l), l = 0 .. 8, come from nine lanes.
  __shared__ uint32_t s_xp[9][9];
  if (tid < 9) {
    f29 xp = x;
    for (uint32_t l = 0; l < tid; l++) xp = f29_sqr<P>(xp);
    limbs_store(s_xp[tid], xp);
  }
  __syncthreads();
  const f29 y = limbs_load(s_xp[8]);
  const uint32_t base = blockIdx.x * EV_THREADS * EV_CH + tid;
  f29 acc = f29_zero();
  if (base < n) {
    // the highest element of this thread's column that exists, then down in steps of 256
    uint32_t j = min(EV_CH - 1, (n - 1 - base) / EV_THREADS);
    acc = f29_load_r256<P>(c + base + j * EV_THREADS);               // any 256-bit word value: bound < 6
    while (j-- > 0) acc = f29_mul_add<P>(acc, y, f29_load_r256<P>(c + base + j * EV_THREADS));   // acc y + c_i in one chain: < 8 * 2 / 170 + 1 + 6 < 8
  }
  limbs_store(sh[tid], acc);
  __syncthreads();
  // pairwise fold with x^(2^l) at level l; the sums stay lazy: the bound grows by 2 per level (< 8 + 16 after eight), well inside
  // what the next product takes, so only the last value is reduced.
  uint32_t level = 0;
  for (uint32_t s = 1; s < EV_THREADS; s <<= 1, level++) {
    if ((tid & (2 * s - 1)) == 0) {
      // lo + hi x^(..): bound + 2 per level; hi's bound (< 24) * 2 stays below 170
      limbs_store(sh[tid], f29_mul_add<P>(limbs_load(sh[tid + s]), limbs_load(s_xp[level]), limbs_load(sh[tid])));
    }
    __syncthreads();
  }
  if (tid == 0) f29_store_canonical<P>(out + blockIdx.x, f29_reduce_small<P>(limbs_load(sh[0])));   // the lazy sums back below 2p
}
__global__ void __launch_bounds__(256) eval_poly_kernel(const fp_words* __restrict__ c, uint32_t n, words8 xw,
                                                        uint32_t log_stride, fp_words* __restrict__ out) {
  side_kernel_prio();
  __shared__ uint32_t sh[EV_THREADS][9];
  eval_poly_block<EV_CH>(c, n, xw, log_stride, out, sh);
}
// m polynomials of one length, each at its own point: grid (blocks, m); level 0 reads the polynomials, level
// 1 folds the per-block partials (partials[j * stride ..]) into out[j]
struct EvalBatchArgs {
  const fp_words* polys[EVAL_BATCH_MAX];
  words8 x[EVAL_BATCH_MAX];
};
template <uint32_t CH>
__global__ void __launch_bounds__(256) eval_poly_batch_kernel(EvalBatchArgs a, uint32_t n, uint32_t level,
                                                              uint32_t stride, fp_words* __restrict__ partial,
                                                              fp_words* __restrict__ out) {
  side_kernel_prio();
  __shared__ uint32_t sh[EV_THREADS][9];
  const uint32_t j = blockIdx.y;
  constexpr uint32_t LOG = CH == 16 ? 12 : 13;   // log2(CH * EV_THREADS)
  if (level == 0) eval_poly_block<CH>(a.polys[j], n, a.x[j], 0, partial + (size_t)j * stride, sh);
  else eval_poly_block<CH>(partial + (size_t)j * stride, n, a.x[j], LOG, out + j, sh);
}
hipError_t poly_eval(const fp_words* d_coeffs, size_t n, const words8& x, fp_words* d_tmp_a, fp_words* d_tmp_b,
                     fp_words* d_out, hipStream_t stream) {
  // level sizes shrink by EV_CH * EV_THREADS per launch; weights: element i of level l is x^(i * stride_l)
  const fp_words* cur = d_coeffs;
  size_t m = n;
  uint32_t log_stride = 0;
  fp_words* bufs[2] = {d_tmp_a, d_tmp_b};
  int which = 0;
  while (true) {
    const uint32_t blocks = eval_blocks(m);
    fp_words* dst = blocks == 1 ? d_out : bufs[which];
    eval_poly_kernel<<<blocks, EV_THREADS, 0, stream>>>(cur, (uint32_t)m, x, log_stride, dst);
    if (blocks == 1) break;
    cur = dst;
    m = blocks;
    log_stride += EV_LOG;
    which ^= 1;
  }
  return hipGetLastError();
}
hipError_t poly_eval_batch(const fp_words* const* d_polys, const words8* xs, uint32_t m, size_t n, fp_words* d_partial,
                           fp_words* d_out, hipStream_t stream) {
  if (m == 0 || m > EVAL_BATCH_MAX) return hipErrorInvalidValue;
  const uint32_t blocks = eval_batch_plan_blocks(n);
  if (blocks == POLY_NO_PLAN) return hipErrorInvalidValue;
  EvalBatchArgs a;
  for (uint32_t j = 0; j < m; j++) {
    a.polys[j] = d_polys[j];
    a.x[j] = xs[j];
  }
  if (eval_batch_ch(n) == 16) {
    eval_poly_batch_kernel<16><<<dim3(blocks, m), EV_THREADS, 0, stream>>>(a, (uint32_t)n, 0, blocks, d_partial, d_out);
    eval_poly_batch_kernel<16><<<dim3(1, m), EV_THREADS, 0, stream>>>(a, blocks, 1, blocks, d_partial, d_out);
  } else {
    eval_poly_batch_kernel<32><<<dim3(blocks, m), EV_THREADS, 0, stream>>>(a, (uint32_t)n, 0, blocks, d_partial, d_out);
    eval_poly_batch_kernel<32><<<dim3(1, m), EV_THREADS, 0, stream>>>(a, blocks, 1, blocks, d_partial, d_out);
  }
  return hipGetLastError();
}

// ---- batch inversion (zeros stay zero, like ff::BatchInvert) --------------------------------
__global__ void __launch_bounds__(256) batch_invert_kernel(fp_words* __restrict__ a, uint32_t n) {
  side_kernel_prio();
  const uint32_t first = (blockIdx.x * blockDim.x + threadIdx.x) * BI_CH;
  if (first >= n) return;
  const uint32_t cnt = min(BI_CH, n - first);
  // straight-line (selects, no branches around the products) and small enough for the compiler to unroll both loops
  // in full, so pre[] stays in registers; a zero or out-of-range element leaves the running product as it is.  The
  // elements are read again on the way back (L2) rather than held: 8 more field elements per thread would halve the
  // occupancy.
  f29 pre[BI_CH];           // prefix products over the non-zero elements
  uint32_t live = 0;        // bit i: element i is in range and non-zero
  f29 acc = f29_one<P>();
#pragma unroll
  for (int i = 0; i < (int)BI_CH; i++) {
    pre[i] = acc;
    const f29 v = load_hat(a + min(first + i, n - 1));
    const bool on = (uint32_t)i < cnt && !f29_is_zero_mod_p<P>(v);
    live |= (uint32_t)on << i;
    const f29 next = f29_mul<P>(acc, v);
#pragma unroll
    for (int q = 0; q < 9; q++) acc.l[q] = on ? next.l[q] : acc.l[q];
  }
  f29 inv = f29_inv<P>(acc);
  // two loops of 4: one loop of 8 x (2 products + the store's domain change) is past the compiler's size limit for
  // "#pragma unroll" (-pragma-unroll-threshold) and would be unrolled by 4 only -- pre[] indexed at run time, in scratch
  auto back = [&](const int i) {
    const bool on = (live >> i) & 1;
    const f29 v = load_hat(a + min(first + i, n - 1));
    const f29 out = f29_mul<P>(inv, pre[i]);
    const f29 next = f29_mul<P>(inv, v);
    if (on) store_hat(a + first + i, out);
#pragma unroll
    for (int q = 0; q < 9; q++) inv.l[q] = on ? next.l[q] : inv.l[q];
  };
#pragma unroll
  for (int k = 0; k < 4; k++) back(7 - k);
#pragma unroll
  for (int k = 0; k < 4; k++) back(3 - k);
  static_assert(BI_CH == 8, "");
}
hipError_t poly_batch_invert(fp_words* d_a, size_t n, hipStream_t stream) {
  if (!n) return hipSuccess;
  const size_t threads = (n + BI_CH - 1) / BI_CH;
  batch_invert_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, stream>>>(d_a, (uint32_t)n);
  return hipGetLastError();
}

// ---- element-wise: out = a * b ------------------------------------------------------------------
__global__ void mul_elementwise_kernel(const fp_words* __restrict__ a, const fp_words* __restrict__ b, uint32_t n,
                                       fp_words* __restrict__ out) {
  side_kernel_prio();
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // a~ * b^ * 2^-261 = (ab)~
  f29_store_canonical<P>(out + i, f29_mul<P>(f29_load_r256<P>(a + i), load_hat(b + i)));
}
hipError_t poly_mul_elementwise(const fp_words* d_a, const fp_words* d_b, size_t n, fp_words* d_out,
                                hipStream_t stream) {
  if (!n) return hipSuccess;
  mul_elementwise_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(d_a, d_b, (uint32_t)n, d_out);
  return hipGetLastError();
}

// ---- canonical-range check of caller-supplied columns (halo2curves' Fr::from_repr refuses words >= r; the gate
// interpreter's lazy bounds assume them) -- a streaming pass, one 32-byte load per element
struct CanonCols {
  const fp_words* col[16];
};
__global__ void __launch_bounds__(256) count_noncanonical_kernel(CanonCols cols, uint32_t n, uint32_t* __restrict__ count, uint32_t flag_only) {
  side_kernel_prio();
  // r as 8 LE words
  const uint32_t R[8] = {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4* src = reinterpret_cast<const uint4*>(cols.col[blockIdx.y] + i);
  const uint4 lo = src[0], hi = src[1];
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  bool ge = true;   // w >= r, decided from the most significant word that differs
#pragma unroll
  for (int k = 0; k < 8; k++) {
    if (w[k] != R[k]) ge = w[k] > R[k];
  }
  if (ge) {
    if (flag_only) {   // a plain store of the same value from every finder: no atomic, so the word may live in mapped host memory
      *reinterpret_cast<volatile uint32_t*>(count) = 1u;
      __threadfence_system();
    } else {
      atomicAdd(count, 1u);
    }
  }
}
static hipError_t noncanonical_launch(const fp_words* const* d_cols, uint32_t m, size_t n, uint32_t* d_word, uint32_t flag_only,
                                      hipStream_t stream) {
  if (!m || !n) return hipSuccess;
  CanonCols cols{};
  for (uint32_t j = 0; j < m; j++) cols.col[j] = d_cols[j];
  count_noncanonical_kernel<<<dim3((unsigned)((n + 255) / 256), m), 256, 0, stream>>>(cols, (uint32_t)n, d_word, flag_only);
  return hipGetLastError();
}
hipError_t poly_flag_noncanonical(const fp_words* const* d_cols, uint32_t m, size_t n, uint32_t* d_flag, hipStream_t stream) {
  return noncanonical_launch(d_cols, m, n, d_flag, 1u, stream);
}
hipError_t poly_count_noncanonical(const fp_words* const* d_cols, uint32_t m, size_t n, uint32_t* d_count, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(d_count, 0, sizeof(uint32_t), stream);
  return e != hipSuccess ? e : noncanonical_launch(d_cols, m, n, d_count, 0u, stream);
}

// ---- out[i] = sum_j c_j * p_j[i] ------------------------------------------------------------------
// one body: the m coefficients into LDS, pairs of terms, the reduction on the way, the low addend
__device__ __forceinline__ void lincomb_rows(const fp_words* const* polys, const words8* coeff, uint32_t m, uint32_t n,
                                             const words8* low, uint32_t n_low, fp_words* __restrict__ out) {
  __shared__ uint32_t s_c[LINCOMB_MAX][9];
  if (threadIdx.x < m) limbs_store(s_c[threadIdx.x], f29_words_to_r261<P>(coeff[threadIdx.x].l));
  __syncthreads();
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  f29 acc = f29_zero();
  for (uint32_t j = 0; j < m; j += 2) {                       // two terms per reduction
    f29 c1 = f29_zero(), p1 = f29_zero();
    const f29 c0 = limbs_load(s_c[j]);
    const f29 p0 = f29_load_r256<P>(polys[j] + i);             // p~ * c^ = (pc)~
    if (j + 1 < m) {
      c1 = limbs_load(s_c[j + 1]);
      p1 = f29_load_r256<P>(polys[j + 1] + i);
    }
    acc = f29_add(acc, f29_mul2<P>(p0, c0, p1, c1));          // bound grows by 2 per pair
    if (lincomb_reduces_after(j)) acc = f29_mul<P>(acc, f29_one<P>());   // keep the lazy sum far below 170 p... (tilde stays tilde)
  }
  if (i < n_low) acc = f29_add(acc, f29_from_words<0>(low[i].l));   // the low-degree addend: a few rows only
  f29_store_canonical<P>(out + i, f29_mul<P>(acc, f29_one<P>()));
}
// (the two argument blocks differ in size on purpose: a single combination's is the smaller kernel argument)
struct LinCombArgs {
  const fp_words* polys[LINCOMB_MAX];
  words8 coeff[LINCOMB_MAX];
  words8 low[LINCOMB_LOW_MAX];   // a polynomial of n_low coefficients added to the combination (memory-domain words)
  uint32_t n_low;
};
__global__ void __launch_bounds__(256) lincomb_kernel(LinCombArgs a, uint32_t m, uint32_t n, fp_words* __restrict__ out) {
  side_kernel_prio();
  lincomb_rows(a.polys, a.coeff, m, n, a.low, a.n_low, out);
}
hipError_t poly_lincomb(const fp_words* const* d_polys, const words8* coeffs, uint32_t m, size_t n, fp_words* d_out,
                        hipStream_t stream, const words8* low, uint32_t n_low) {
  if (m > LINCOMB_MAX || n_low > LINCOMB_LOW_MAX || n_low > n) return hipErrorInvalidValue;   // m = 0: the low polynomial alone
  if (n == 0) return hipSuccess;
  LinCombArgs a;
  for (uint32_t j = 0; j < m; j++) {
    a.polys[j] = d_polys[j];
    a.coeff[j] = coeffs[j];
  }
  a.n_low = n_low;
  for (uint32_t t = 0; t < n_low; t++) a.low[t] = low[t];
  lincomb_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(a, m, (uint32_t)n, d_out);
  return hipGetLastError();
}

struct LinCombSetsArgs {
  const fp_words* polys[LINCOMB_SETS_POLYS];
  words8 coeff[LINCOMB_SETS_POLYS];
  words8 low[LINCOMB_SETS_MAX][LINCOMB_SETS_LOW];
  fp_words* out[LINCOMB_SETS_MAX];
  uint32_t first[LINCOMB_SETS_MAX + 1];
  uint32_t n_low[LINCOMB_SETS_MAX];
};
__global__ void __launch_bounds__(256) lincomb_sets_kernel(LinCombSetsArgs a, uint32_t n) {
  side_kernel_prio();
  const uint32_t set = blockIdx.y, j0 = a.first[set], m = a.first[set + 1] - j0;
  lincomb_rows(a.polys + j0, a.coeff + j0, m, n, a.low[set], a.n_low[set], a.out[set]);
}
hipError_t poly_lincomb_sets(const fp_words* const* d_polys, const words8* coeffs, const uint32_t* first, uint32_t n_sets, size_t n,
                             const words8* low, const uint32_t* n_low, fp_words* const* d_out, hipStream_t stream) {
  if (n_sets == 0 || n_sets > LINCOMB_SETS_MAX || first[0] != 0 || first[n_sets] > LINCOMB_SETS_POLYS) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  LinCombSetsArgs a{};
  for (uint32_t s = 0; s < n_sets; s++) {
    if (first[s + 1] < first[s] || first[s + 1] - first[s] > LINCOMB_MAX || n_low[s] > LINCOMB_SETS_LOW || n_low[s] > n) return hipErrorInvalidValue;
    a.first[s] = first[s];
    a.n_low[s] = n_low[s];
    a.out[s] = d_out[s];
    for (uint32_t t = 0; t < n_low[s]; t++) a.low[s][t] = low[s * LINCOMB_SETS_LOW + t];
  }
  a.first[n_sets] = first[n_sets];
  for (uint32_t j = 0; j < first[n_sets]; j++) {
    a.polys[j] = d_polys[j];
    a.coeff[j] = coeffs[j];
  }
  lincomb_sets_kernel<<<dim3((unsigned)((n + 255) / 256), n_sets), 256, 0, stream>>>(a, (uint32_t)n);
  return hipGetLastError();
}

}  // namespace sg
