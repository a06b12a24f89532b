// Polynomial helpers, part 1 of 3 (included once by poly.hip): the device helpers all parts share, and the helpers built on
// a workgroup scan -- the exclusive prefix product, the grand products of a proof and the Kate division.  Every step has one
// body; the single and the batched form (blockIdx.y = product / division) differ in where pointers and weights come from.
#pragma once
#include "poly.h"
#include "side_prio.cuh"

namespace sg {

typedef Fr29 P;
__device__ __forceinline__ f29 load_hat(const fp_words* p) {  // x~ words -> x^ (< 2p)
  uint32_t w[8];
  fp_words_load(p, w);
  return f29_words_to_r261<P>(w);
}
__device__ __forceinline__ void store_hat(fp_words* p, const f29& x_hat) {  // x^ -> canonical x~ words
  uint32_t w[8];
  f29_to_words(f29_reduce_with<P>(x_hat, P::r256), w);
  fp_words_store(p, w);
}
// the nine limbs of a field element to a row of LDS and back
__device__ __forceinline__ void limbs_store(uint32_t* row, const f29& v) {
#pragma unroll
  for (int q = 0; q < 9; q++) row[q] = v.l[q];
}
__device__ __forceinline__ f29 limbs_load(const uint32_t* row) {
  f29 v;
#pragma unroll
  for (int q = 0; q < 9; q++) v.l[q] = row[q];
  return v;
}

// ---- exclusive prefix product: out[0] = 1, out[i] = a[0] * ... * a[i-1] ------------------------
// three launches: per-block products, scan of the block products (one workgroup), final pass
__device__ __forceinline__ f29 block_exclusive_scan_mul(f29 mine, uint32_t (*sh)[9], uint32_t tid, uint32_t nthr,
                                                        f29* total) {
  // Hillis-Steele inclusive scan with multiplication, then shift
  limbs_store(sh[tid], mine);
  __syncthreads();
  f29 v = mine;
  for (uint32_t d = 1; d < nthr; d <<= 1) {
    f29 o = f29_one<P>();
    if (tid >= d) o = limbs_load(sh[tid - d]);
    __syncthreads();
    v = f29_mul<P>(v, o);
    limbs_store(sh[tid], v);
    __syncthreads();
  }
  if (total) *total = limbs_load(sh[nthr - 1]);
  f29 ex = f29_one<P>();
  if (tid) ex = limbs_load(sh[tid - 1]);
  __syncthreads();
  return ex;
}
// blockIdx.y = product: n elements and nblk block products each (a single product is a batch of one)
__global__ void __launch_bounds__(256) prefix_product_blocks_batch(const fp_words* __restrict__ a, uint32_t n, uint32_t nblk,
                                                                   fp_words* __restrict__ bprod) {
  side_kernel_prio();
  __shared__ uint32_t sh[PP_THREADS][9];
  a += (size_t)blockIdx.y * n;
  const uint32_t tid = threadIdx.x, first = (blockIdx.x * PP_THREADS + tid) * PP_CH;
  f29 acc = f29_one<P>();
  for (uint32_t i = 0; i < PP_CH; i++)
    if (first + i < n) acc = f29_mul<P>(acc, load_hat(a + first + i));
  f29 total;
  block_exclusive_scan_mul(acc, sh, tid, PP_THREADS, &total);
  if (tid == 0) store_hat(bprod + (size_t)blockIdx.y * nblk + blockIdx.x, total);
}
__global__ void __launch_bounds__(1024) prefix_product_scan_blocks_batch(fp_words* __restrict__ bprod, uint32_t nblk) {
  side_kernel_prio();
  __shared__ uint32_t sh[1024][9];
  bprod += (size_t)blockIdx.y * nblk;
  const uint32_t tid = threadIdx.x;
  f29 mine = tid < nblk ? load_hat(bprod + tid) : f29_one<P>();
  f29 ex = block_exclusive_scan_mul(mine, sh, tid, 1024, nullptr);
  if (tid < nblk) store_hat(bprod + tid, ex);
}
// the final pass over one block.  bprod: this block's scanned product; has_init: `init` multiplies every output; closing
// (optional): closing[slot] <- the output of closing_row
__device__ __forceinline__ void prefix_product_write_block(const fp_words* __restrict__ a, uint32_t n, const fp_words* __restrict__ bprod,
                                                           const words8& init, uint32_t has_init, uint32_t count_out,
                                                           fp_words* __restrict__ out, fp_words* closing, uint32_t slot,
                                                           uint32_t closing_row) {
  __shared__ uint32_t sh[PP_THREADS][9];
  const uint32_t tid = threadIdx.x, first = (blockIdx.x * PP_THREADS + tid) * PP_CH;
  f29 v[PP_CH];
  f29 acc = f29_one<P>();
#pragma unroll
  for (uint32_t i = 0; i < PP_CH; i++) {
    v[i] = (first + i < n) ? load_hat(a + first + i) : f29_one<P>();
    acc = f29_mul<P>(acc, v[i]);
  }
  f29 run = f29_mul<P>(block_exclusive_scan_mul(acc, sh, tid, PP_THREADS, nullptr), load_hat(bprod));
  if (has_init) run = f29_mul<P>(run, f29_words_to_r261<P>(init.l));
#pragma unroll
  for (uint32_t i = 0; i < PP_CH; i++) {
    if (first + i < count_out) store_hat(out + first + i, run);
    if (closing && first + i == closing_row) store_hat(closing + slot, run);
    run = f29_mul<P>(run, v[i]);
  }
}
__global__ void __launch_bounds__(256) prefix_product_write(const fp_words* __restrict__ a, uint32_t n,
                                                            const fp_words* __restrict__ bprod, words8 init,
                                                            uint32_t has_init, uint32_t count_out,
                                                            fp_words* __restrict__ out) {
  side_kernel_prio();
  prefix_product_write_block(a, n, bprod + blockIdx.x, init, has_init, count_out, out, nullptr, 0, 0);
}
__global__ void __launch_bounds__(256) prefix_product_write_batch(const fp_words* __restrict__ a, uint32_t n, uint32_t nblk,
                                                                  const fp_words* __restrict__ bprod, uint32_t count_out,
                                                                  GrandOut outs) {
  side_kernel_prio();
  prefix_product_write_block(a + (size_t)blockIdx.y * n, n, bprod + (size_t)blockIdx.y * nblk + blockIdx.x, words8{}, 0u, count_out,
                             outs.z[blockIdx.y], outs.closing, blockIdx.y, outs.closing_row);
}
hipError_t poly_prefix_product(const fp_words* d_a, size_t n, fp_words* d_tmp, fp_words* d_out, size_t count_out,
                               const words8* init, hipStream_t stream) {
  const uint32_t nblk = prefix_blocks(n, count_out);
  if (nblk == POLY_NO_PLAN) return hipErrorInvalidValue;
  if (nblk == 0) return hipSuccess;
  prefix_product_blocks_batch<<<dim3(nblk, 1), PP_THREADS, 0, stream>>>(d_a, (uint32_t)n, nblk, d_tmp);
  prefix_product_scan_blocks_batch<<<dim3(1, 1), 1024, 0, stream>>>(d_tmp, nblk);
  words8 one{};
  prefix_product_write<<<nblk, PP_THREADS, 0, stream>>>(d_a, (uint32_t)n, d_tmp, init ? *init : one, init ? 1u : 0u,
                                                        (uint32_t)count_out, d_out);
  return hipGetLastError();
}

// ---- grand-product fractions (halo2 permutation::prover::commit / lookup::prover::commit_product)
// permutation chunk: den[i] = prod_c (beta * sigma_c[i] + gamma + v_c[i])
//                    num[i] = prod_c (delta^(j0+c) * omega^i * beta + gamma + v_c[i])
// pow_tab: omega^i for i < n as 2^261-domain words (NttEngine::local_twiddles(omega, k + 1), cached per domain): one product
// instead of an exponentiation per row; read by the numerators only
__device__ __forceinline__ void perm_fraction_row(const PermCols& cols, uint32_t ncols, const f29& beta, const f29& gamma,
                                                  const words8& dstart_w, const words8& delta_w, uint32_t numer,
                                                  const fp_words* __restrict__ pow_tab, fp_words* __restrict__ io, uint32_t i) {
  f29 acc = numer ? load_hat(io + i) : f29_one<P>();          // numerators multiply the inverted denominators
  f29 dw = f29_one<P>();
  if (numer) dw = f29_mul<P>(f29_words_to_r261<P>(dstart_w.l), f29_load_r256<P>(pow_tab + i));   // hat * hat * 2^-261 = hat
  const f29 delta = f29_words_to_r261<P>(delta_w.l);
  for (uint32_t c = 0; c < ncols; c++) {
    f29 v = load_hat(cols.values[c] + i);                      // < 2
    f29 t = numer ? f29_mul<P>(dw, beta) : f29_mul<P>(load_hat(cols.sigma[c] + i), beta);
    t = f29_add(f29_add(t, gamma), v);                         // < 6
    acc = f29_mul<P>(acc, t);                                  // 12
    if (numer) dw = f29_mul<P>(dw, delta);
  }
  store_hat(io + i, acc);
}
// lookup: den[i] = (a'[i] + beta)(s'[i] + gamma);  num[i] = (a[i] + beta)(s[i] + gamma)
__device__ __forceinline__ void lookup_fraction_row(const fp_words* __restrict__ x, const fp_words* __restrict__ y, const f29& beta,
                                                    const f29& gamma, uint32_t numer, fp_words* __restrict__ io, uint32_t i) {
  f29 t = f29_mul<P>(f29_add(load_hat(x + i), beta), f29_add(load_hat(y + i), gamma));   // 4 * 4
  if (numer) t = f29_mul<P>(t, load_hat(io + i));
  store_hat(io + i, t);
}
__global__ void __launch_bounds__(256) perm_fraction_kernel(PermCols cols, uint32_t ncols, words8 beta_w, words8 gamma_w, words8 dstart_w,
                                                            words8 delta_w, uint32_t n, uint32_t numer,
                                                            const fp_words* __restrict__ pow_tab, fp_words* __restrict__ io) {
  side_kernel_prio();
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const f29 beta = f29_words_to_r261<P>(beta_w.l), gamma = f29_words_to_r261<P>(gamma_w.l);
  perm_fraction_row(cols, ncols, beta, gamma, dstart_w, delta_w, numer, pow_tab, io, i);
}
__global__ void lookup_fraction_kernel(const fp_words* __restrict__ x, const fp_words* __restrict__ y, words8 beta_w,
                                       words8 gamma_w, uint32_t n, uint32_t numer, fp_words* __restrict__ io) {
  side_kernel_prio();
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const f29 beta = f29_words_to_r261<P>(beta_w.l), gamma = f29_words_to_r261<P>(gamma_w.l);
  lookup_fraction_row(x, y, beta, gamma, numer, io, i);
}
hipError_t poly_perm_fraction(const PermCols& cols, uint32_t ncols, const words8& beta, const words8& gamma,
                              const words8& delta_start, const words8& delta, size_t n, int numer, fp_words* d_io,
                              hipStream_t stream, const fp_words* d_pow_tab) {
  if (numer && !d_pow_tab) return hipErrorInvalidValue;
  perm_fraction_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(cols, ncols, beta, gamma, delta_start, delta, (uint32_t)n,
                                                                        (uint32_t)numer, d_pow_tab, d_io);
  return hipGetLastError();
}
hipError_t poly_lookup_fraction(const fp_words* d_x, const fp_words* d_y, const words8& beta, const words8& gamma,
                                size_t n, int numer, fp_words* d_io, hipStream_t stream) {
  lookup_fraction_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(d_x, d_y, beta, gamma, (uint32_t)n,
                                                                          (uint32_t)numer, d_io);
  return hipGetLastError();
}
// ---- all grand products of a proof in batched launches ------------------------------------------------------
// halo2 builds the permutation argument's z per chunk and each lookup's z one after the other; every one of them is
// "denominators -> batch inversion -> numerators -> running product", and the inversion is ONE division-step chain per
// lane (~65 us) whatever the size.  Here the P products of a proof share the launches: blockIdx.y = product, one
// inversion pass over P * n elements, one three-launch running product with grid.y = P; a chunk's z continues from the
// previous chunk's last usable value through a device-side scalar (no host round trip).
__global__ void __launch_bounds__(256) grand_fraction_kernel(GrandProducts g, words8 beta_w, words8 gamma_w, words8 delta_w,
                                                             uint32_t n, uint32_t numer, const fp_words* __restrict__ pow_tab,
                                                             fp_words* __restrict__ io) {
  side_kernel_prio();
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (i >= n) return;
  io += (size_t)y * n;
  const f29 beta = f29_words_to_r261<P>(beta_w.l), gamma = f29_words_to_r261<P>(gamma_w.l);
  if (y < g.n_perm) {
    perm_fraction_row(g.perm[y], g.ncols[y], beta, gamma, g.delta_start[y], delta_w, numer, pow_tab, io, i);
  } else {
    const uint32_t l = y - g.n_perm;
    lookup_fraction_row(g.lookup[l][numer ? 0 : 2], g.lookup[l][numer ? 1 : 3], beta, gamma, numer, io, i);
  }
}
// z[i] *= *scalar (a value another kernel of the stream has just written: the previous chunk's z at its last usable row)
__global__ void __launch_bounds__(256) scale_by_device_scalar_kernel(fp_words* __restrict__ z, uint32_t n, const fp_words* __restrict__ scalar,
                                                                     fp_words* __restrict__ closing, uint32_t closing_row) {
  side_kernel_prio();
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const f29 v = f29_mul<P>(load_hat(z + i), load_hat(scalar));
  store_hat(z + i, v);
  if (closing && i == closing_row) store_hat(closing, v);   // (the unscaled value prefix_product_write_batch left there is replaced)
}
__global__ void __launch_bounds__(256) batch_invert_kernel(fp_words* __restrict__ a, uint32_t n);   // poly.hip
hipError_t poly_grand_products(const GrandProducts& g, const words8& beta, const words8& gamma, const words8& delta, size_t n,
                               size_t usable, const fp_words* d_pow_tab, fp_words* d_mod, fp_words* d_tmp, const GrandOut& outs,
                               hipStream_t stream) {
  const uint32_t Pn = g.n_perm + g.n_lookup;
  if (Pn == 0) return hipSuccess;
  if (Pn > GRAND_MAX || n == 0 || usable >= n || (g.n_perm && !d_pow_tab)) return hipErrorInvalidValue;
  const uint32_t nblk = grand_blocks(n);
  if (nblk == POLY_NO_PLAN) return hipErrorInvalidValue;
  const dim3 rows((unsigned)((n + 255) / 256), Pn);
  grand_fraction_kernel<<<rows, 256, 0, stream>>>(g, beta, gamma, delta, (uint32_t)n, 0u, d_pow_tab, d_mod);
  batch_invert_kernel<<<(unsigned)(((size_t)Pn * n / BI_CH + 255) / 256 + 1), 256, 0, stream>>>(d_mod, (uint32_t)(Pn * n));
  grand_fraction_kernel<<<rows, 256, 0, stream>>>(g, beta, gamma, delta, (uint32_t)n, 1u, d_pow_tab, d_mod);
  prefix_product_blocks_batch<<<dim3(nblk, Pn), PP_THREADS, 0, stream>>>(d_mod, (uint32_t)n, nblk, d_tmp);
  prefix_product_scan_blocks_batch<<<dim3(1, Pn), 1024, 0, stream>>>(d_tmp, nblk);
  prefix_product_write_batch<<<dim3(nblk, Pn), PP_THREADS, 0, stream>>>(d_mod, (uint32_t)n, nblk, d_tmp, (uint32_t)n, outs);
  // chunk j of the permutation argument starts where chunk j - 1 ended: z_j = z_{j-1}[usable] * (its own running product)
  for (uint32_t j = 1; j < g.n_perm; j++)
    scale_by_device_scalar_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(outs.z[j], (uint32_t)n, outs.z[j - 1] + usable,
                                                                                   outs.closing ? outs.closing + j : nullptr, outs.closing_row);
  return hipGetLastError();
}

// ---- Kate division: a(X) = q(X) (X - b) + a(b) -------------------------------------------------
// s_i = a_i + b s_{i+1} (s_n = 0), q_{i-1} = s_i, remainder s_0: a suffix scan whose combine step is
// "multiply by a power of b and add".  Three launches like the prefix product: block values, scan of
// the block values (one workgroup, <= 1024 blocks), final pass with the carries.
// S_t = sum_{u >= t} mine_u w^(u - t) over the nthr threads of a workgroup (w_pow[j] = w^(2^j), hat)
__device__ __forceinline__ f29 block_suffix_geometric(f29 mine, const f29* w_pow, uint32_t (*sh)[9], uint32_t tid,
                                                      uint32_t nthr) {
  limbs_store(sh[tid], mine);
  __syncthreads();
  f29 v = mine;                                              // lazy between steps: `mine` may come with a bound up to 8
  uint32_t j = 0;
  for (uint32_t d = 1; d < nthr; d <<= 1, j++) {
    f29 o = f29_zero();
    if (tid + d < nthr) o = limbs_load(sh[tid + d]);
    __syncthreads();
    v = f29_mul_add<P>(o, w_pow[j], v);                      // v + w^d * o: the bound grows by < 2 per step (< 2 + 16 after eight)
    limbs_store(sh[tid], v);
    __syncthreads();
  }
  return v;
}
__device__ __forceinline__ f29 kd_local(const fp_words* __restrict__ a, uint32_t n, uint32_t first, const f29& b_hat,
                                        f29* vals) {
  f29 acc = f29_zero();                                      // Horner from the top of the chunk down
#pragma unroll
  for (uint32_t k = KD_CH; k-- > 0;) {
    vals[k] = (first + k < n) ? load_hat(a + first + k) : f29_zero();
    acc = f29_mul_add<P>(acc, b_hat, vals[k]);               // acc * b + a_k: < 4 * 2 / 170 + 1 + 2 < 4
  }
  return acc;
}
// the scan weights b^(KD_CH * 2^j) (within a block) and b^(KD_BLOCK * 2^j) (across blocks), hat form: 21 dependent
// squarings that every thread of every launch used to repeat (they were a third of a division's latency); computed
// once on the host with the same limb code and passed as a kernel argument (a single division) or uploaded, one per
// division, and brought into LDS by every workgroup (a batch)
struct KatePowers {
  f29 b_hat;
  f29 chunk[8];   // b^(8 * 2^j)
  f29 block[10];  // b^(2048 * 2^j)
};
static_assert(sizeof(KatePowers) == KATE_POWERS_BYTES, "poly_plan.h sizes the batch's tables");
static KatePowers kate_powers(const words8& b) {
  KatePowers pw;
  pw.b_hat = f29_mul<P>(f29_from_words<0>(b.l), f29_const<P>(P::r266));   // = f29_words_to_r261
  f29 t = pw.b_hat;
  for (int i = 0; i < 3; i++) t = f29_sqr<P>(t);
  for (int j = 0; j < 8; j++) {
    pw.chunk[j] = t;
    t = f29_sqr<P>(t);
  }
  for (int j = 0; j < 10; j++) {   // t = b^(8 * 2^8) = b^2048 here
    pw.block[j] = t;
    t = f29_sqr<P>(t);
  }
  return pw;
}
__device__ __forceinline__ void kate_powers_to_lds(KatePowers* pw, const KatePowers* __restrict__ src) {
  for (uint32_t i = threadIdx.x; i < sizeof(KatePowers) / 4; i += blockDim.x)
    reinterpret_cast<uint32_t*>(pw)[i] = reinterpret_cast<const uint32_t*>(src)[i];
  __syncthreads();
}
// bval: this division's block values
__device__ __forceinline__ void kate_blocks_step(const fp_words* __restrict__ a, uint32_t n, const KatePowers& pw,
                                                 fp_words* __restrict__ bval) {
  __shared__ uint32_t sh[KD_THREADS][9];
  const uint32_t tid = threadIdx.x, first = (blockIdx.x * KD_THREADS + tid) * KD_CH;
  f29 vals[KD_CH];
  f29 local = kd_local(a, n, first, pw.b_hat, vals);
  f29 s = block_suffix_geometric(local, pw.chunk, sh, tid, KD_THREADS);
  if (tid == 0) store_hat(bval + blockIdx.x, s);
}
// carry[k] = sum_{u > k} bval[u] * (b^KD_BLOCK)^(u - k - 1): the value of s just above block k
__device__ __forceinline__ void kate_scan_blocks_step(fp_words* __restrict__ bval, uint32_t nblk, const KatePowers& pw) {
  __shared__ uint32_t sh[1024][9];
  const uint32_t tid = threadIdx.x, nthr = blockDim.x;        // nthr = power of two >= nblk: log2(nthr) scan steps
  f29 mine = tid < nblk ? load_hat(bval + tid) : f29_zero();
  block_suffix_geometric(mine, pw.block, sh, tid, nthr);      // sh[t] = inclusive suffix value
  f29 carry = f29_zero();
  if (tid + 1 < nthr) carry = limbs_load(sh[tid + 1]);
  __syncthreads();
  if (tid < nblk) store_hat(bval + tid, carry);
}
// carry: this division's carries (nullptr: a single-block division has none); rem_out (optional): s_0 = a(b)
__device__ __forceinline__ void kate_write_step(const fp_words* __restrict__ a, uint32_t n, const KatePowers& pw,
                                                const fp_words* __restrict__ carry, fp_words* __restrict__ q_out,
                                                fp_words* __restrict__ rem_out) {
  __shared__ uint32_t sh[KD_THREADS][9];
  const uint32_t tid = threadIdx.x, first = (blockIdx.x * KD_THREADS + tid) * KD_CH;
  f29 vals[KD_CH];
  const f29& b_hat = pw.b_hat;
  const f29* w = pw.chunk;
  f29 local = kd_local(a, n, first, b_hat, vals);
  // the top thread's chunk sees the block carry: s(lo) = local + b^KD_CH * carry
  if (carry && tid == KD_THREADS - 1) local = f29_mul_add<P>(load_hat(carry + blockIdx.x), w[0], local);
  block_suffix_geometric(local, w, sh, tid, KD_THREADS);      // sh[t] = s at the bottom of thread t's chunk
  f29 run = f29_zero();                                        // s just above this thread's chunk
  if (tid + 1 < KD_THREADS) run = limbs_load(sh[tid + 1]);
  else if (carry) run = load_hat(carry + blockIdx.x);
#pragma unroll
  for (uint32_t k = KD_CH; k-- > 0;) {
    const uint32_t i = first + k;
    run = f29_mul_add<P>(run, b_hat, vals[k]);                 // s_i = s_(i+1) b + a_i: < 20 * 2 / 170 + 1 + 2
    if (i < n) {
      if (i >= 1) store_hat(q_out + i - 1, run);
      else if (rem_out) store_hat(rem_out, run);
    }
  }
  if (first <= n - 1 && n - 1 < first + KD_CH) store_hat(q_out + n - 1, f29_zero());   // padding slot
}
__global__ void __launch_bounds__(256) kate_blocks(const fp_words* __restrict__ a, uint32_t n, KatePowers pw,
                                                   fp_words* __restrict__ bval) {
  side_kernel_prio();
  kate_blocks_step(a, n, pw, bval);
}
__global__ void __launch_bounds__(1024) kate_scan_blocks(fp_words* __restrict__ bval, uint32_t nblk, KatePowers pw) {
  side_kernel_prio();
  kate_scan_blocks_step(bval, nblk, pw);
}
__global__ void __launch_bounds__(256) kate_write(const fp_words* __restrict__ a, uint32_t n, KatePowers pw,
                                                  const fp_words* __restrict__ carry, fp_words* __restrict__ q_out,
                                                  fp_words* __restrict__ rem_out) {
  side_kernel_prio();
  kate_write_step(a, n, pw, carry, q_out, rem_out);
}
hipError_t poly_kate_division(const fp_words* d_a, size_t n, const words8& b, fp_words* d_tmp, fp_words* d_q,
                              fp_words* d_rem, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const uint32_t nblk = kate_blocks(n);
  if (nblk == POLY_NO_PLAN) return hipErrorInvalidValue;
  const KatePowers pw = kate_powers(b);
  if (nblk == 1) {  // n <= 2048: the block's suffix scan is the whole division, one launch instead of three
    kate_write<<<1, KD_THREADS, 0, stream>>>(d_a, (uint32_t)n, pw, nullptr, d_q, d_rem);
    return hipGetLastError();
  }
  kate_blocks<<<nblk, KD_THREADS, 0, stream>>>(d_a, (uint32_t)n, pw, d_tmp);
  kate_scan_blocks<<<1, kate_scan_threads(nblk), 0, stream>>>(d_tmp, nblk, pw);
  kate_write<<<nblk, KD_THREADS, 0, stream>>>(d_a, (uint32_t)n, pw, d_tmp, d_q, d_rem);
  return hipGetLastError();
}

// ---- several Kate divisions in one launch per step (grid.y = division): the quotients of SHPLONK's rotation sets.  By
// partial fractions 1 / prod_j (X - p_j) = sum_j c_j / (X - p_j), so the |S| divisions of a set are independent divisions
// of ONE polynomial (it vanishes on the whole set) instead of a chain; all sets' divisions go in one batch.  The scan
// weights live in device memory (one KatePowers per division, uploaded by the caller).
struct KateBatch {
  const fp_words* a[KATE_BATCH_MAX];
  fp_words* q[KATE_BATCH_MAX];
};
__global__ void __launch_bounds__(256) kate_blocks_batch(KateBatch bt, uint32_t n, const KatePowers* __restrict__ pws,
                                                         fp_words* __restrict__ bval, uint32_t nblk) {
  side_kernel_prio();
  __shared__ KatePowers pw;
  kate_powers_to_lds(&pw, pws + blockIdx.y);
  kate_blocks_step(bt.a[blockIdx.y], n, pw, bval + (size_t)blockIdx.y * nblk);
}
__global__ void __launch_bounds__(1024) kate_scan_blocks_batch(fp_words* __restrict__ bval, uint32_t nblk,
                                                               const KatePowers* __restrict__ pws) {
  side_kernel_prio();
  __shared__ KatePowers pw;
  kate_powers_to_lds(&pw, pws + blockIdx.y);
  kate_scan_blocks_step(bval + (size_t)blockIdx.y * nblk, nblk, pw);
}
// the remainder s_0 = a(b) is dropped (exact divisions)
__global__ void __launch_bounds__(256) kate_write_batch(KateBatch bt, uint32_t n, const KatePowers* __restrict__ pws,
                                                        const fp_words* __restrict__ carry_all, uint32_t nblk) {
  side_kernel_prio();
  __shared__ KatePowers pw;
  kate_powers_to_lds(&pw, pws + blockIdx.y);
  kate_write_step(bt.a[blockIdx.y], n, pw, nblk > 1 ? carry_all + (size_t)blockIdx.y * nblk : nullptr, bt.q[blockIdx.y], nullptr);
}
// q[j] = a[j] / (X - b[j]) for m <= 16 polynomials of n coefficients (n written per quotient, the last one 0); h_pw: m
// KatePowers on the host (scratch), d_pw / d_tmp: device scratch (kate_batch_powers_bytes / kate_batch_tmp_elems)
hipError_t poly_kate_division_batch(const fp_words* const* d_a, size_t n, const words8* b, uint32_t m, fp_words* const* d_q,
                                    uint8_t* h_pw, uint8_t* d_pw, fp_words* d_tmp, hipStream_t stream) {
  if (m == 0 || n == 0) return hipSuccess;
  if (m > KATE_BATCH_MAX) return hipErrorInvalidValue;
  const uint32_t nblk = kate_blocks(n);
  if (nblk == POLY_NO_PLAN) return hipErrorInvalidValue;
  KatePowers* hp = reinterpret_cast<KatePowers*>(h_pw);
  KateBatch bt{};
  for (uint32_t j = 0; j < m; j++) {
    hp[j] = kate_powers(b[j]);
    bt.a[j] = d_a[j];
    bt.q[j] = d_q[j];
  }
  hipError_t e = hipMemcpyAsync(d_pw, h_pw, kate_batch_powers_bytes(m), hipMemcpyHostToDevice, stream);
  if (e != hipSuccess) return e;
  const KatePowers* dp = reinterpret_cast<const KatePowers*>(d_pw);
  if (nblk > 1) {
    kate_blocks_batch<<<dim3(nblk, m), KD_THREADS, 0, stream>>>(bt, (uint32_t)n, dp, d_tmp, nblk);
    kate_scan_blocks_batch<<<dim3(1, m), kate_scan_threads(nblk), 0, stream>>>(d_tmp, nblk, dp);
  }
  kate_write_batch<<<dim3(nblk, m), KD_THREADS, 0, stream>>>(bt, (uint32_t)n, dp, d_tmp, nblk);
  return hipGetLastError();
}

}  // namespace sg
