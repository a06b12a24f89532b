// Set-up time operations on G1 points that are not part of the MSM engine: fixed-base products, the FFT over G1, prefix
// sums of a basis, the window table of fixed-base MSMs and the on-curve check (see g1_ops.h).
#include "g1_ops.h"
#include "host_wait.h"

#include <vector>

namespace sg {

// out[i] = scalars[i] * G  (ParamsKZG::setup's fixed-base products; also used to build
// synthetic bases for benchmarks).  One thread per scalar, double-and-add in XYZZ, result
// normalised on the device.
__global__ void __launch_bounds__(256) g1_fixed_base_mul(const fp_words* __restrict__ scalars, uint32_t n,
                                                         g1_affine_mem* __restrict__ out) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  typedef Fq29 P;
  words8 s;
  {
    f29 k = f29_zero();
    k.l[0] = 32;
    f29_to_words(f29_cond_sub_p<Fr29>(f29_mul<Fr29>(f29_load_r256<Fr29>(scalars + i), k)), s.l);
  }
  affine29 gen;
  {
    // G = (1, 2): Montgomery-2^256 words of 1 and 2, then the usual shifted load
    uint32_t w[16];
    f29 one256 = f29_const<P>(P::r256);             // limbs of 2^256 mod q == words of 1~
    f29_to_words(one256, w);
    f29 two = f29_cond_sub_p<P>(f29_normalize(f29_add(one256, one256)));
    f29_to_words(two, w + 8);
    gen = affine29_from_words(w);
  }
  xyzz29 acc = xyzz29_identity();
  for (int limb = 7; limb >= 0; limb--) {
    uint32_t w = s.l[7];
#pragma unroll
    for (int k = 7; k > 0; k--) s.l[k] = s.l[k - 1];
    s.l[0] = 0;
    for (int bit = 31; bit >= 0; bit--) {
      acc = xyzz29_double(acc);
      if ((w >> bit) & 1) xyzz29_madd(acc, gen);
    }
  }
  uint32_t ow[16];
  if (xyzz29_is_identity(acc)) {
    for (int k = 0; k < 16; k++) ow[k] = 0;
  } else {
    f29 iz = f29_inv<P>(acc.zzz);                            // 1/ZZZ
    f29 t = f29_mul<P>(acc.zz, iz);                          // ZZ/ZZZ = 1/Z
    f29 ax = f29_mul<P>(acc.x, f29_sqr<P>(t));               // X/ZZ
    f29 ay = f29_mul<P>(acc.y, iz);                          // Y/ZZZ
    f29_to_words(f29_reduce_with<P>(ax, P::r256), ow);
    f29_to_words(f29_reduce_with<P>(ay, P::r256), ow + 8);
  }
#pragma unroll
  for (int k = 0; k < 4; k++) out[i].q[k] = make_uint4(ow[4 * k], ow[4 * k + 1], ow[4 * k + 2], ow[4 * k + 3]);
}

hipError_t fixed_base_mul(const fp_words* d_scalars, size_t n, g1_affine_mem* d_out, hipStream_t stream) {
  if (!n) return hipSuccess;
  g1_fixed_base_mul<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(d_scalars, (uint32_t)n, d_out);
  return hipGetLastError();
}

// ------------------------------------------------------------------ N5: FFT over G1
// ParamsKZG::downsize / g_to_lagrange: the same radix-2 butterfly as
// best_fft with group elements: a' = a + w*b, b' = a - w*b, w*b a 254-bit scalar
// multiplication.  Set-up time only (once per SRS), so: one thread per butterfly per stage,
// points in XYZZ limb form in global memory, twiddles computed on the fly.
__device__ inline xyzz29 xyzz29_scalar_mul(const xyzz29& p, const uint32_t k[8]) {
  xyzz29 acc = xyzz29_identity();
  for (int limb = 7; limb >= 0; limb--) {
    const uint32_t w = k[limb];
    for (int bit = 31; bit >= 0; bit--) {
      acc = xyzz29_double(acc);
      if ((w >> bit) & 1) xyzz29_add(acc, p);
    }
  }
  return acc;
}
// canonical integer words of x^ (2^261-domain Fr)
__device__ __forceinline__ void fr29_to_integer_words(const f29& x, uint32_t w[8]) {
  f29 one = f29_zero();
  one.l[0] = 1;
  f29_to_words(f29_cond_sub_p<Fr29>(f29_mul<Fr29>(x, one)), w);
}
__global__ void g1fft_load(const g1_affine_mem* __restrict__ in, uint32_t log_n, xyzz29_mem* __restrict__ out) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >> log_n) return;
  g1_affine_mem raw = in[i];
  affine29 q = affine29_load(&raw);
  xyzz29 p = xyzz29_identity();
  xyzz29_madd(p, q);  // identity + q: reduces the lazy coordinates, sets ZZ = ZZZ = 1
  uint32_t r = log_n ? (__brev(i) >> (32 - log_n)) : 0;
  xyzz29_store(out + r, p);
}
__global__ void __launch_bounds__(128) g1fft_stage(xyzz29_mem* __restrict__ a, uint32_t log_n, uint32_t s, words8 omega) {
  uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >> (log_n - 1)) return;
  const uint32_t h = 1u << s, j = q & (h - 1), blk = q >> s;
  const uint32_t i0 = (blk << (s + 1)) + j, i1 = i0 + h;
  xyzz29 u = xyzz29_load(a + i0), v = xyzz29_load(a + i1);
  if (j) {
    uint32_t k[8];
    fr29_to_integer_words(f29_pow_u64<Fr29>(f29_words_to_r261<Fr29>(omega.l), (uint64_t)j << (log_n - s - 1)), k);
    v = xyzz29_scalar_mul(v, k);
  }
  xyzz29 sum = u;
  xyzz29_add(sum, v);
  if (!xyzz29_is_identity(v)) v.y = f29_sub<Fq29, 1>(f29_zero(), v.y);  // -v: Y < 4 -> 4p - Y
  xyzz29_add(u, v);
  xyzz29_store(a + i0, sum);
  xyzz29_store(a + i1, u);
}
// out[i] = scale * a[i], affine
__global__ void __launch_bounds__(128) g1fft_store(const xyzz29_mem* __restrict__ a, uint32_t log_n, words8 scale,
                                                   uint32_t has_scale, g1_affine_mem* __restrict__ out) {
  typedef Fq29 P;
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >> log_n) return;
  xyzz29 p = xyzz29_load(a + i);
  if (has_scale) {
    uint32_t k[8];
    fr29_to_integer_words(f29_words_to_r261<Fr29>(scale.l), k);
    p = xyzz29_scalar_mul(p, k);
  }
  uint32_t ow[16];
  if (xyzz29_is_identity(p)) {
    for (int k = 0; k < 16; k++) ow[k] = 0;
  } else {
    f29 iz = f29_inv<P>(p.zzz);
    f29 t = f29_mul<P>(p.zz, iz);
    f29_to_words(f29_reduce_with<P>(f29_mul<P>(p.x, f29_sqr<P>(t)), P::r256), ow);
    f29_to_words(f29_reduce_with<P>(f29_mul<P>(p.y, iz), P::r256), ow + 8);
  }
#pragma unroll
  for (int k = 0; k < 4; k++) out[i].q[k] = make_uint4(ow[4 * k], ow[4 * k + 1], ow[4 * k + 2], ow[4 * k + 3]);
}

hipError_t g1_fft(const g1_affine_mem* d_in, g1_affine_mem* d_out, uint32_t log_n, const words8& omega,
                  const words8* scale, xyzz29_mem* d_work, hipStream_t stream) {
  const uint32_t n = 1u << log_n;
  g1fft_load<<<(n + 127) / 128, 128, 0, stream>>>(d_in, log_n, d_work);
  for (uint32_t s = 0; s < log_n; s++)
    g1fft_stage<<<(n / 2 + 127) / 128, 128, 0, stream>>>(d_work, log_n, s, omega);
  words8 sc = scale ? *scale : omega;
  g1fft_store<<<(n + 127) / 128, 128, 0, stream>>>(d_work, log_n, sc, scale ? 1u : 0u, d_out);
  return hipGetLastError();
}

// ------------------------------------------------------------------ prefix sums of a basis (difference-form commits)
// Blocked scan over points: every thread runs through PFX_CHUNK consecutive elements (inclusive running sums in place,
// chunk total to the next level), the totals are scanned the same way recursively, then the offsets are added on the
// way down; the last step also normalises to affine.  Once per SRS.
static constexpr uint32_t PFX_CHUNK = 32;
template <bool AFFINE>
__global__ void __launch_bounds__(128) g1_prefix_chunks(const g1_affine_mem* __restrict__ in, xyzz29_mem* __restrict__ run, uint32_t n,
                                                       xyzz29_mem* __restrict__ totals) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t first = t * PFX_CHUNK;
  if (first >= n) return;
  const uint32_t last = min(n, first + PFX_CHUNK);
  xyzz29 acc = xyzz29_identity();
  for (uint32_t i = first; i < last; i++) {
    if (AFFINE) {
      g1_affine_mem raw = in[i];
      xyzz29_madd(acc, affine29_load(&raw));
    } else {
      xyzz29_add(acc, xyzz29_load(run + i));
    }
    xyzz29_store(run + i, acc);
  }
  if (totals) xyzz29_store(totals + t, acc);
}
// run[i] += upper[i / PFX_CHUNK - 1]  (upper = inclusive prefix sums of the chunk totals)
__global__ void __launch_bounds__(128) g1_prefix_apply(xyzz29_mem* __restrict__ run, uint32_t n, const xyzz29_mem* __restrict__ upper) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || i < PFX_CHUNK) return;
  xyzz29 v = xyzz29_load(run + i);
  xyzz29_add(v, xyzz29_load(upper + i / PFX_CHUNK - 1));
  xyzz29_store(run + i, v);
}
__global__ void __launch_bounds__(128) g1_prefix_store(const xyzz29_mem* __restrict__ run, uint32_t n, const xyzz29_mem* __restrict__ upper,
                                                      g1_affine_mem* __restrict__ out) {
  typedef Fq29 P;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  xyzz29 p = xyzz29_load(run + i);
  if (upper && i >= PFX_CHUNK) xyzz29_add(p, xyzz29_load(upper + i / PFX_CHUNK - 1));
  uint32_t ow[16];
  if (xyzz29_is_identity(p)) {
    for (int k = 0; k < 16; k++) ow[k] = 0;
  } else {
    f29 iz = f29_inv<P>(p.zzz);
    f29 t = f29_mul<P>(p.zz, iz);
    f29_to_words(f29_reduce_with<P>(f29_mul<P>(p.x, f29_sqr<P>(t)), P::r256), ow);
    f29_to_words(f29_reduce_with<P>(f29_mul<P>(p.y, iz), P::r256), ow + 8);
  }
#pragma unroll
  for (int k = 0; k < 4; k++) out[i].q[k] = make_uint4(ow[4 * k], ow[4 * k + 1], ow[4 * k + 2], ow[4 * k + 3]);
}
hipError_t g1_prefix_sums(const g1_affine_mem* d_in, size_t n, g1_affine_mem* d_out, hipStream_t stream) {
  if (!n) return hipSuccess;
  if (n >= (1ull << 31) || d_in == d_out) return hipErrorInvalidValue;
  // level sizes: n, ceil(n / 32), ... down to one chunk
  std::vector<size_t> size{n};
  while (size.back() > PFX_CHUNK) size.push_back((size.back() + PFX_CHUNK - 1) / PFX_CHUNK);
  size_t total = 0;
  for (size_t v : size) total += v;
  xyzz29_mem* work = nullptr;
  hipError_t e = hipMalloc(&work, total * sizeof(xyzz29_mem));
  if (e != hipSuccess) return e;
  std::vector<xyzz29_mem*> lvl(size.size());
  lvl[0] = work;
  for (size_t l = 1; l < size.size(); l++) lvl[l] = lvl[l - 1] + size[l - 1];
  auto grid = [](size_t threads) { return (unsigned)((threads + 127) / 128); };
  for (size_t l = 0; l < size.size(); l++) {   // up: running sums per chunk, totals to the next level
    const size_t chunks = (size[l] + PFX_CHUNK - 1) / PFX_CHUNK;
    xyzz29_mem* totals = l + 1 < size.size() ? lvl[l + 1] : nullptr;
    if (l == 0) g1_prefix_chunks<true><<<grid(chunks), 128, 0, stream>>>(d_in, lvl[0], (uint32_t)size[0], totals);
    else g1_prefix_chunks<false><<<grid(chunks), 128, 0, stream>>>(nullptr, lvl[l], (uint32_t)size[l], totals);
  }
  for (size_t l = size.size() - 1; l-- > 1;)   // down: levels size-2 .. 1 become global prefix sums
    g1_prefix_apply<<<grid(size[l]), 128, 0, stream>>>(lvl[l], (uint32_t)size[l], lvl[l + 1]);
  g1_prefix_store<<<grid(n), 128, 0, stream>>>(lvl[0], (uint32_t)n, size.size() > 1 ? lvl[1] : nullptr, d_out);
  e = hipGetLastError();
  if (e == hipSuccess) e = host_wait_stream(stream);
  (void)hipFree(work);
  return e;
}

// ------------------------------------------------------------------ fixed-base window table
// next[i] = 2^doublings * prev[i], affine (one inversion per point: this runs once per SRS)
__global__ void __launch_bounds__(128) msm_table_step(const g1_affine_mem* __restrict__ prev, uint32_t n,
                                                      uint32_t doublings, g1_affine_mem* __restrict__ next) {
  typedef Fq29 P;
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  g1_affine_mem raw = prev[i];
  uint32_t ow[16];
  bool ident = true;
#pragma unroll
  for (int k = 0; k < 4; k++) ident = ident && !(raw.q[k].x | raw.q[k].y | raw.q[k].z | raw.q[k].w);
  if (ident || doublings == 0) {
    next[i] = raw;
    return;
  }
  affine29 q = affine29_load(&raw);
  xyzz29 acc = xyzz29_double_affine(q);
  for (uint32_t d = 1; d < doublings; d++) acc = xyzz29_double(acc);
  if (xyzz29_is_identity(acc)) {
    for (int k = 0; k < 16; k++) ow[k] = 0;
  } else {
    f29 iz = f29_inv<P>(acc.zzz);
    f29 t = f29_mul<P>(acc.zz, iz);
    f29_to_words(f29_reduce_with<P>(f29_mul<P>(acc.x, f29_sqr<P>(t)), P::r256), ow);
    f29_to_words(f29_reduce_with<P>(f29_mul<P>(acc.y, iz), P::r256), ow + 8);
  }
#pragma unroll
  for (int k = 0; k < 4; k++) next[i].q[k] = make_uint4(ow[4 * k], ow[4 * k + 1], ow[4 * k + 2], ow[4 * k + 3]);
}

// table rows: row w = 2^(offset of window w) * bases, W x n affine points
hipError_t build_window_table(const g1_affine_mem* d_bases, size_t n, uint32_t c, FixedTable* out, hipStream_t stream) {
  if (n == 0 || n >= (1ull << 31) || c < 4 || c > 16) return hipErrorInvalidValue;
  FixedTable t;
  t.c = c;
  t.n = n;
  t.wp = make_window_plan(c);
  if ((size_t)t.wp.W * n >= (1ull << 31)) return hipErrorInvalidValue;
  hipError_t e = hipMalloc(&t.table, sizeof(g1_affine_mem) * n * t.wp.W);
  if (e != hipSuccess) return e;
  e = hipMemcpyAsync(t.table, d_bases, sizeof(g1_affine_mem) * n, hipMemcpyDeviceToDevice, stream);
  for (uint32_t w = 1; w < t.wp.W && e == hipSuccess; w++) {
    msm_table_step<<<(unsigned)((n + 127) / 128), 128, 0, stream>>>(t.table + (size_t)(w - 1) * n, (uint32_t)n,
                                                                    t.wp.width[w - 1], t.table + (size_t)w * n);
    e = hipGetLastError();
  }
  if (e != hipSuccess) {
    (void)hipFree(t.table);
    return e;
  }
  *out = t;
  return hipSuccess;
}

// is the 256-bit value of 8 LE words below the modulus?  (borrow chain of w - p over exactly normalised limbs)
template <class P>
__device__ __forceinline__ bool words_below_p(const uint32_t w[8]) {
  const f29 a = f29_from_words<0>(w);
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) borrow = (a.l[i] - P::p[i] - borrow) >> 31;
  return borrow != 0;
}
// points[i] on y^2 = x^3 + 3 (or the identity, 64 zero bytes)?  *bad counts the points that are not.  A coordinate whose
// words are not below q is bad whatever its residue (halo2curves' from_raw_bytes refuses it, and so does sg_pairing_check)
__global__ void __launch_bounds__(256) g1_on_curve_kernel(const g1_affine_mem* __restrict__ points, uint32_t n, uint32_t* bad) {
  typedef Fq29 P;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[16];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint4 v = points[i].q[k];
    w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
  }
  const affine29 p = affine29_from_words(w);
  if (p.inf) return;
  if (!words_below_p<P>(w) || !words_below_p<P>(w + 8)) {
    atomicAdd(bad, 1u);
    return;
  }
  const f29 one = f29_one<P>();
  const f29 x = f29_mul<P>(p.x, one), y = f29_mul<P>(p.y, one);       // bound 32 -> < 2
  const f29 x3 = f29_mul<P>(f29_sqr<P>(x), x), y2 = f29_sqr<P>(y);
  const f29 three = f29_add(f29_add(one, one), one);
  const f29 d = f29_sub<P, 1>(f29_sub<P, 0>(y2, x3), three);          // y^2 - x^3 - 3 (+ multiples of q)
  if (!f29_is_zero_mod_p<P>(d)) atomicAdd(bad, 1u);
}
hipError_t g1_on_curve(const g1_affine_mem* d_points, size_t n, uint32_t* d_bad, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(d_bad, 0, sizeof(uint32_t), stream);
  if (e != hipSuccess || !n) return e;
  g1_on_curve_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(d_points, (uint32_t)n, d_bad);
  return hipGetLastError();
}

}  // namespace sg
