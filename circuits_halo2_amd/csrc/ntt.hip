// Radix-2 NTT / iNTT over BN254 Fr for gfx950 -- the GPU side of halo2's `best_fft`
// and `EvaluationDomain::{ifft, coeff_to_extended, extended_to_coeff}` (SURVEY.md §8a N1-N4;
// reference call sites zk_prover/src/circuits/utils.rs:75,76,94-101).
//
// Layout: natural order in, natural order out, elements are 32-byte Montgomery Fr exactly
// as halo2curves stores them.  A transform of n = 2^L points is factored into 1-3 passes
// (four-step / six-step Cooley-Tukey).  Every pass is one launch of `ntt_pass`: a workgroup
// stages a tile of T contiguous columns x R strided rows in LDS, runs log2(R) radix-2 DIT
// stages there (one butterfly per thread per stage, twiddles = powers of omega_R from an LDS
// tile), multiplies by the inter-pass twiddle (table in the pass's output order, fully
// coalesced) and writes the tile back.  The first pass of a multi-pass plan writes each
// column as a contiguous run ("transposing" store) so that no bit-reversal or separate
// transpose pass ever touches HBM.
//
// HBM traffic per pass: 32 B read + 32 B write per element (+32 B twiddle on twiddled
// passes).  Arithmetic: (n/2) log2 n Montgomery products + one per element per twiddled pass.
#include "ntt.h"
#include "host_wait.h"
#include "side_prio.cuh"

#include <algorithm>
#include <cstring>

namespace sg {
SG_DEFINE_SIDE_PRIO_SETTER(ntt_set_side_prio)

// ------------------------------------------------------------------ device kernels
// Arithmetic: 9 x 29-bit limbs (bn254_f29.cuh).  Data stays in the Montgomery-2^256 domain it
// is stored in; twiddle tables hold w^ = w * 2^261 mod r (as canonical 8 x u32 words), so
// f29_mul(x~, w^) = (x w)~.  Inside a pass additions are lazy (bound grows by 2 per stage,
// <= 25 after 10 stages); every pass ends with one product per element (inter-pass twiddle,
// post-scale, or 1^) which brings the value below 2r, then a conditional subtraction makes it
// canonical for the 32-byte store.
struct PassArgs {
  const fp_words* tw_local;  // w_R^k in the 2^261 domain, k < R/2
  const fp_words* tw_pass;   // per-element twiddle in output order (nullptr: none)
  uint32_t log_r;            // log2 R  (DFT length of this pass)
  uint32_t log_t;            // log2 T  (contiguous columns per tile)
  uint32_t log_b;            // log2 B  (contiguous inner extent)
  uint32_t kind;             // 0: in-place-like (Y), 1: transposing first pass (X)
  uint32_t sig_lo;           // X only: b = lo + 2^sig_lo * hi  ->  b' = hi + 2^sig_hi * lo
  uint32_t sig_hi;
  uint32_t in_len;           // elements present in `in`; beyond that the input reads as zero
  uint32_t pre3;             // multiply input i by pre[i % 3]   (coeff_to_extended)
  uint32_t post3;            // multiply output j by post[j % 3] (extended_to_coeff / plain scale)
  uint32_t fold29;           // the data of this (last) pass carries a factor 2^29 (the plan's last twiddle table holds
                             // it): close with one Montgomery limb step instead of a product by 1^; post[] absorbs 2^-29
  uint32_t skip;             // leading DIT stages whose second operand is zero (zero-padded first pass): not executed
  uint32_t radix4;           // two DIT stages per sweep over the tile (four elements per thread)
  uint32_t pre[3][8];        // Montgomery-2^256 words, converted once per workgroup
  uint32_t post[3][8];
  // blockIdx.y selects the vector (a lone transform is vector 0 of a launch with grid.y = 1); same plan for all (small
  // transforms are a chain of launches at their ~5 us floor: the 9 iNTTs of a proof become 3 launches instead of 27)
  const fp_words* in_b[NTT_BATCH_MAX];
  fp_words* out_b[NTT_BATCH_MAX];
  // first pass: input element gi of vector y is multiplied by pre_tab_b[y][gi] (2^261-domain words) on load
  uint32_t pre_tab;
  const fp_words* pre_tab_b[NTT_BATCH_MAX];
};

struct LdsTile {
  uint4* lo;
  uint4* hi;
  uint32_t* top;
};
__device__ __forceinline__ void lds_put(const LdsTile& t, uint32_t i, const f29& v) {
  t.lo[i] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  t.hi[i] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
  t.top[i] = v.l[8];
}
__device__ __forceinline__ f29 lds_get(const LdsTile& t, uint32_t i) {
  uint4 a = t.lo[i], b = t.hi[i];
  f29 r;
  r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
  r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
  r.l[8] = t.top[i];
  return r;
}

// One pass.  grid.x = number of tiles = (2^log_b / T) * A  where A = n / (B*R).
// Dynamic LDS: (T*R + R/2 + 8) * 36 bytes.
__global__ void __launch_bounds__(1024) ntt_pass(PassArgs p) {
#define SG_NTT_R4 0
#include "ntt_pass_body.inc"
#undef SG_NTT_R4
}
// the same pass with two DIT stages per sweep (four elements per thread: more registers, half the threads)
__global__ void __launch_bounds__(512) ntt_pass_r4(PassArgs p) {
#define SG_NTT_R4 1
#include "ntt_pass_body.inc"
#undef SG_NTT_R4
}

// tw[k] = (w^k)^ for k < count; w given as Montgomery-2^256 words
__global__ void fill_powers(fp_words* tw, words8 w, uint32_t count) {
  side_kernel_prio();
  typedef Fr29 P;
  uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < count) f29_store_canonical<P>(tw + k, f29_pow_u64<P>(f29_words_to_r261<P>(w.l), k));
}

// inter-pass twiddle tables, in the output order of the pass they are applied in
//  mode 0 (2-pass, pass X):   idx = j2 + n2*i1            -> w^(i1*j2) * scale
//  mode 1 (3-pass, pass A):   idx = j3 + n3*(i2 + n2*i1)  -> w^(n1*i2*j3) * scale
//  mode 2 (3-pass, pass B):   idx = j3 + n3*j2 + n2n3*i1  -> w^(i1*(j3 + n3*j2))
//  times29: the table additionally carries the factor 2^29 that the last pass removes with f29_mont_step
__global__ void fill_pass_twiddles(fp_words* tw, words8 w, words8 scale, uint32_t has_scale, uint32_t mode,
                                   uint32_t l1, uint32_t l2, uint32_t l3, uint32_t log_n, uint32_t times29) {
  side_kernel_prio();
  typedef Fr29 P;
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >> log_n) return;
  uint64_t e;
  if (mode == 0) {
    uint64_t j2 = idx & ((1ull << l2) - 1), i1 = idx >> l2;
    e = i1 * j2;
  } else if (mode == 1) {
    uint64_t j3 = idx & ((1ull << l3) - 1), i2 = (idx >> l3) & ((1ull << l2) - 1);
    e = (i2 * j3) << l1;
  } else {
    uint64_t jj = idx & ((1ull << (l2 + l3)) - 1), i1 = idx >> (l2 + l3);
    e = i1 * jj;
  }
  e &= (1ull << log_n) - 1;
  f29 v = f29_pow_u64<P>(f29_words_to_r261<P>(w.l), e);
  if (has_scale) v = f29_mul<P>(v, f29_words_to_r261<P>(scale.l));
  if (times29) {   // v * (2^29 * 2^261) * 2^-261: the integer 2^290 mod r as limbs = (2^261 mod r) doubled 29 times
    f29 k = f29_one<P>();
    for (int i = 0; i < 29; i++) k = f29_cond_sub_p<P>(f29_normalize(f29_dbl(k)));
    v = f29_mul<P>(v, k);
  }
  f29_store_canonical<P>(tw + idx, v);
}
// out = w^e as Montgomery-2^256 words (host-visible domain constants)
__global__ void pow_single(fp_words* out, words8 w, uint64_t e) {
  side_kernel_prio();
  typedef Fr29 P;
  f29 v = f29_pow_u64<P>(f29_words_to_r261<P>(w.l), e);
  uint32_t o[8];
  f29_to_words(f29_reduce_with<P>(v, P::r256), o);
  fp_words_store(out, o);
}

__global__ void scale_kernel(fp_words* a, words8 s, size_t n) {
  side_kernel_prio();
  typedef Fr29 P;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) f29_store_canonical<P>(a + i, f29_mul<P>(f29_load_r256<P>(a + i), f29_words_to_r261<P>(s.l)));
}
// a[i] *= tab[i & (period-1)]   (divide_by_vanishing_poly; period = 2^(ext_k-k)); tab in the
// 2^256 domain like the data
__global__ void scale_periodic_kernel(fp_words* a, const fp_words* tab, uint32_t period, size_t n) {
  side_kernel_prio();
  typedef Fr29 P;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    uint32_t t[8];
    fp_words_load(tab + (i & (period - 1)), t);
    f29_store_canonical<P>(a + i, f29_mul<P>(f29_load_r256<P>(a + i), f29_words_to_r261<P>(t)));
  }
}
// dir = 1: canonical integers -> Montgomery-2^256 (x * 2^517 * 2^-261); dir = 0: the inverse
// (x~ * 2^5 * 2^-261)
__global__ void to_mont_kernel(const fp_words* in, fp_words* out, size_t n, int dir) {
  side_kernel_prio();
  typedef Fr29 P;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    f29 k = f29_zero();
    k.l[0] = 32;
    if (dir) k = f29_const<P>(P::r517);
    f29_store_canonical<P>(out + i, f29_mul<P>(f29_load_r256<P>(in + i), k));
  }
}

// ------------------------------------------------------------------ host side
static bool fp_host_eq(const words8& a, const words8& b) { return std::memcmp(&a, &b, sizeof(words8)) == 0; }

NttEngine::~NttEngine() { clear(); }

void NttEngine::clear() {
  for (auto& pl : plans_) {
    for (int i = 0; i < 3; i++) {
      if (pl.tw_pass[i]) (void)hipFree(pl.tw_pass[i]);
    }
  }
  plans_.clear();
  for (auto& kv : local_tw_) (void)hipFree(kv.tw);
  local_tw_.clear();
}

hipError_t NttEngine::local_twiddles(const words8& omega_r, uint32_t log_r, hipStream_t stream, fp_words** out) {
  for (auto& e : local_tw_) {
    if (e.log_r == log_r && fp_host_eq(e.omega_r, omega_r)) {
      *out = e.tw;
      return hipSuccess;
    }
  }
  uint32_t count = log_r ? (1u << (log_r - 1)) : 1;
  fp_words* d = nullptr;
  hipError_t err = hipMalloc(&d, sizeof(fp_words) * count);
  if (err != hipSuccess) return err;
  fill_powers<<<(count + 255) / 256, 256, 0, stream>>>(d, omega_r, count);
  err = hipGetLastError();
  if (err == hipSuccess) err = host_wait_stream(stream);  // complete before any other stream may use the cached table
  if (err != hipSuccess) {
    retire_device_memory(d);
    return err;
  }
  local_tw_.push_back({log_r, omega_r, d});
  *out = d;
  return hipSuccess;
}

hipError_t NttEngine::get_plan(uint32_t log_n, const words8& omega, const words8* scale, hipStream_t stream,
                               const NttPlan** out) {
  for (auto& pl : plans_) {
    if (pl.log_n == log_n && fp_host_eq(pl.omega, omega) && pl.has_scale == (scale != nullptr) &&
        (!scale || fp_host_eq(pl.scale, *scale))) {
      *out = &pl;
      return hipSuccess;
    }
  }
  NttPlan pl{};
  pl.log_n = log_n;
  pl.omega = omega;
  pl.has_scale = scale != nullptr;
  if (scale) pl.scale = *scale;
  const NttFactors f = ntt_factor(cfg_, log_n);
  pl.npass = f.npass;
  std::copy(f.l, f.l + 3, pl.l);
  const size_t n = (size_t)1 << log_n;
  hipError_t err;
  // omega_R for a length-R sub-transform is omega^(n/R): square omega (log_n - log_r) times
  // on the device via fill_powers' pow (host has no field arithmetic on purpose)
  auto omega_pow2 = [&](uint32_t times, words8* res) -> hipError_t {
    fp_words* d = nullptr;
    hipError_t e = hipMalloc(&d, sizeof(fp_words) * 2);
    if (e != hipSuccess) return e;
    // fill_powers computes w^k; k = 2^times fits 32 bits (times <= 28)
    pow_single<<<1, 1, 0, stream>>>(d, omega, 1ull << times);
    e = hipMemcpyAsync(res, d, sizeof(fp_words), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = host_wait_stream(stream);
    retire_device_memory(d);   // a few bytes per plan; hipFree would wait for every other stream of the device
    return e;
  };
  for (int i = 0; i < pl.npass; i++) {
    words8 wr;
    err = omega_pow2(log_n - pl.l[i], &wr);
    if (err != hipSuccess) return err;
    err = local_twiddles(wr, pl.l[i], stream, &pl.tw_local[i]);   // (cached by the engine: nothing of the plan's to give back)
    if (err != hipSuccess) return err;
  }
  // one inter-pass table per pass but the last (fill_pass_twiddles: mode 0; modes 1 and 2): the first holds the scale, the last
  // the factor 2^29.  A step that fails gives back the tables allocated so far.
  auto give_back = [&](hipError_t e) {
    for (fp_words* t : pl.tw_pass) retire_device_memory(t);
    return e;
  };
  const words8 one_or_scale = scale ? *scale : omega;  // placeholder when unused
  for (int t = 0; t < pl.npass - 1; t++) {
    err = hipMalloc(&pl.tw_pass[t], sizeof(fp_words) * n);
    if (err != hipSuccess) return give_back(err);
    fill_pass_twiddles<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(pl.tw_pass[t], omega, one_or_scale, scale && t == 0 ? 1 : 0,
                                                                         pl.npass == 2 ? 0 : 1 + t, pl.l[0], pl.l[1], pl.l[2], log_n,
                                                                         t == pl.npass - 2 ? 1 : 0);
  }
  err = hipGetLastError();
  // tables must be complete before any other stream may use the cached plan
  if (err == hipSuccess) err = host_wait_stream(stream);
  if (err != hipSuccess) return give_back(err);
  plans_.push_back(pl);
  *out = &plans_.back();
  return hipSuccess;
}

// The passes of one job, one launch each: geometry, tile and workgroup of pass `i`, and what rides on it, from ntt_plan.h.
hipError_t NttEngine::run(const Job& j, uint32_t log_n, const words8& omega, hipStream_t stream) {
  const NttFactors f = ntt_factor(cfg_, log_n);
  const NttPlan* pl;
  hipError_t err = get_plan(log_n, omega, ntt_scale_in_table(f, j.scale, j.post3) ? j.scale : nullptr, stream, &pl);
  if (err != hipSuccess) return err;
  const size_t n = (size_t)1 << log_n;
  PassArgs p{};
  for (int i = 0; i < f.npass; i++) {
    const NttPassRide r = ntt_pass_ride(f, i, j.src_len, j.scale, j.pre3, j.post3, j.pre_tab);
    for (uint32_t v = 0; v < j.count; v++) {
      fp_words* mid = j.src ? j.data[v] : j.scratch + (size_t)v * n;
      p.in_b[v] = r.in == NTT_MID ? mid : j.src ? j.src[v] : j.data[v];
      p.out_b[v] = r.out == NTT_MID ? mid : j.data[v];
      if (r.pre_tab) p.pre_tab_b[v] = j.pre_tab[v];
    }
    p.in_len = r.in_len;
    p.pre3 = r.pre3;
    p.pre_tab = r.pre_tab;
    p.post3 = r.post != NTT_POST_NONE;
    if (r.pre3) std::memcpy(p.pre, j.pre3, sizeof p.pre);
    for (int t = 0; t < 3 && p.post3; t++) std::memcpy(p.post[t], r.post == NTT_POST_CALLER ? j.post3[t].l : j.scale->l, 32);
    const NttPassGeom g = ntt_pass_geom(f, i);
    p.tw_local = pl->tw_local[g.tw_local];
    p.tw_pass = g.tw_pass < 0 ? nullptr : pl->tw_pass[g.tw_pass];
    p.log_r = g.log_r; p.log_b = g.log_b; p.kind = g.kind; p.sig_lo = g.sig_lo; p.sig_hi = g.sig_hi; p.fold29 = g.fold29;
    const NttPassShape s = ntt_pass_shape(cfg_, g, log_n, p.in_len, j.nbatch);
    if (s.lds_bytes > NTT_LDS_BUDGET || s.threads > (s.radix4 ? NTT_MAX_THREADS_R4 : NTT_MAX_THREADS)) return hipErrorInvalidConfiguration;
    p.skip = s.skip;
    p.log_t = s.log_t;
    p.radix4 = s.radix4;
    if (s.radix4) hipLaunchKernelGGL(ntt_pass_r4, dim3(s.grid_x, s.grid_y), dim3(s.threads), s.lds_bytes, stream, p);
    else hipLaunchKernelGGL(ntt_pass, dim3(s.grid_x, s.grid_y), dim3(s.threads), s.lds_bytes, stream, p);
    err = hipGetLastError();
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}

hipError_t NttEngine::transform_batch(fp_words* const* a, uint32_t count, fp_words* scratch, uint32_t log_n,
                                      const words8& omega, const words8* scale, hipStream_t stream,
                                      const fp_words* const* src, size_t src_len, const words8* pre3, const fp_words* const* pre_tab) {
  const size_t n = (size_t)1 << log_n;
  if (count == 0) return hipSuccess;
  if (pre_tab && (!src || src_len < n)) return hipErrorInvalidValue;   // (the zero-padded load path does not take a table)
  if (count > NTT_BATCH_MAX || log_n == 0) return hipErrorInvalidValue;
  return run(Job{a, count, count, src, src ? src_len : n, scratch, scale, pre3, nullptr, pre_tab}, log_n, omega, stream);
}

hipError_t NttEngine::init() {
  // allow the large dynamic-LDS tiles (up to the full 160 KiB of a CU)
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ntt_pass), hipFuncAttributeMaxDynamicSharedMemorySize, (int)NTT_LDS_BUDGET);
  if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(ntt_pass_r4), hipFuncAttributeMaxDynamicSharedMemorySize, (int)NTT_LDS_BUDGET);
  return e;
}

hipError_t NttEngine::transform(const fp_words* in, size_t in_len, fp_words* out, fp_words* scratch, uint32_t log_n,
                                const words8& omega, const words8* scale, const words8* pre3, const words8* post3,
                                hipStream_t stream) {
  if (log_n == 0) {   // one element: itself, times the plain scale
    hipError_t err = in != out ? hipMemcpyAsync(out, in, sizeof(fp_words), hipMemcpyDeviceToDevice, stream) : hipSuccess;
    if (err == hipSuccess && scale && !post3) scale_kernel<<<1, 64, 0, stream>>>(out, *scale, 1);
    return err;
  }
  // nbatch = 0: a lone transform keeps the latency shape whatever ntt.batch_min says
  return run(Job{&out, 1, 0, in == out ? nullptr : &in, in_len, scratch, scale, pre3, post3, nullptr}, log_n, omega, stream);
}

hipError_t ntt_scale(fp_words* a, const words8& s, size_t n, hipStream_t stream) {
  scale_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(a, s, n);
  return hipGetLastError();
}
hipError_t ntt_scale_periodic(fp_words* a, const fp_words* tab, uint32_t period, size_t n, hipStream_t stream) {
  scale_periodic_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(a, tab, period, n);
  return hipGetLastError();
}
hipError_t fr_montgomery(const fp_words* in, fp_words* out, size_t n, int to_mont, hipStream_t stream) {
  if (!n) return hipSuccess;
  to_mont_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(in, out, n, to_mont);
  return hipGetLastError();
}

}  // namespace sg
