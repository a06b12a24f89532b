// C ABI, polynomial family: sg_fr_*, grand products, Kate division, linear combinations, the lookup permutation, the KZG
// setup and the G1 / G2 / pairing / keccak helpers (summa_gpu.hip holds the core).
#include "abi_internal.h"

using namespace sg;

extern "C" {

// ------------------------------------------------------------------ misc
int sg_g1_fixed_base_mul_dev(const void* d_scalars, size_t n, void* d_out_affine, void* stream) {
  if (n && (!d_scalars || !d_out_affine)) return fail(SG_ERR_INVALID, "sg_g1_fixed_base_mul: null argument");
  LOCKED_CTX();
  hipError_t e = fixed_base_mul(static_cast<const fp_words*>(d_scalars), n, static_cast<g1_affine_mem*>(d_out_affine),
                                pick_stream(stream));
  if (e != hipSuccess) return hip_fail("fixed_base_mul", e);
  return SG_OK;
}
int sg_g1_fixed_base_mul(const uint8_t* scalars, size_t n, uint8_t* out_affine) {
  if (n && (!scalars || !out_affine)) return fail(SG_ERR_INVALID, "sg_g1_fixed_base_mul: null argument");
  LOCKED_CTX();
  TRY(upload(g_ctx->stage_a, scalars, n * 32, g_ctx->stream));
  hipError_t e = g_ctx->stage_b.reserve(n * 64 + 64);
  if (e != hipSuccess) return hip_fail("staging buffer", e);
  TRY(sg_g1_fixed_base_mul_dev(g_ctx->stage_a.p, n, g_ctx->stage_b.p, g_ctx->stream));
  if (!n) return SG_OK;
  return download(out_affine, g_ctx->stage_b.p, n * 64, g_ctx->stream);
}
// Verifier side of ParamsKZG::setup: scalar * (G2 generator) on the host (g2 = 1 * G2, s_g2 = tau * G2)
int sg_g2_generator_mul(const uint8_t scalar[32], uint8_t out[128]) {
  if (!scalar || !out) return fail(SG_ERR_INVALID, "sg_g2_generator_mul: null argument");
  sg::host::g2_generator_mul(scalar, out);
  return SG_OK;
}
// The verifier's last step (halo2 `SingleStrategy` -> multi_miller_loop + final_exponentiation; the EVM's precompile
// 0x08): *ok = (prod_i e(g1[i], g2[i]) == 1).  Host code (host_pairing.h); the slopes of a G2 point are computed once
// and cached by its bytes (the two G2 points of a KZG check are fixed per SRS).
static int pairing_check_impl(const uint8_t* g1_points, const uint8_t* g2_points, size_t n, int* ok, bool plain_check) {
  if (!ok || (n && (!g1_points || !g2_points))) return fail(SG_ERR_INVALID, "sg_pairing_check: null argument");
  if (n > 64) return fail(SG_ERR_INVALID, "sg_pairing_check: at most 64 pairs");
  using namespace sg::host;
  static std::mutex cache_mu;
  static std::map<std::string, PreparedG2> cache;
  std::vector<Affine> ps;
  std::vector<const PreparedG2*> qs;
  const Fq three = fq_from_u64(3);
  for (size_t i = 0; i < n; i++) {
    Affine p;
    std::memcpy(p.x.v, g1_points + 64 * i, 32);
    std::memcpy(p.y.v, g1_points + 64 * i + 32, 32);
    const bool p_inf = p.x.is_zero() && p.y.is_zero();
    if (Fq::geq_p(p.x.v) || Fq::geq_p(p.y.v)) return fail(SG_ERR_INVALID, "sg_pairing_check: G1 coordinate not reduced");
    if (!p_inf && !(p.y.sqr() == p.x.sqr() * p.x + three)) return fail(SG_ERR_INVALID, "sg_pairing_check: G1 point not on the curve");
    const uint8_t* qb = g2_points + 128 * i;
    G2AffinePt q;
    std::memcpy(q.x.c0.v, qb, 32); std::memcpy(q.x.c1.v, qb + 32, 32);
    std::memcpy(q.y.c0.v, qb + 64, 32); std::memcpy(q.y.c1.v, qb + 96, 32);
    q.inf = q.x.is_zero() && q.y.is_zero();
    if (Fq::geq_p(q.x.c0.v) || Fq::geq_p(q.x.c1.v) || Fq::geq_p(q.y.c0.v) || Fq::geq_p(q.y.c1.v))
      return fail(SG_ERR_INVALID, "sg_pairing_check: G2 coordinate not reduced");
    if (!g2_on_curve(q)) return fail(SG_ERR_INVALID, "sg_pairing_check: G2 point not on the twist");
    if (p_inf || q.inf) continue;  // e(O, Q) = e(P, O) = 1
    const PreparedG2* prep;
    {
      std::lock_guard<std::mutex> lk(cache_mu);
      std::string key(reinterpret_cast<const char*>(qb), 128);
      auto it = cache.find(key);
      if (it == cache.end()) {
        if (cache.size() >= 64) cache.clear();
        it = cache.emplace(key, prepare_g2(q)).first;
      }
      prep = &it->second;   // std::map nodes are stable; entries are only dropped by the clear() above
      ps.push_back(p);
      qs.push_back(new PreparedG2(*prep));
    }
  }
  const Fq12 ml = multi_miller_loop(ps, qs);
  for (const PreparedG2* q : qs) delete q;
  const bool one = final_exponentiation(ml).is_one();
  if (plain_check && final_exponentiation_plain(ml).is_one() != one) return fail(SG_ERR_HIP, "sg_pairing_check: the two final exponentiations disagree");
  *ok = one ? 1 : 0;
  return SG_OK;
}
int sg_pairing_check(const uint8_t* g1_points, const uint8_t* g2_points, size_t n, int* ok) {
  return pairing_check_impl(g1_points, g2_points, n, ok, false);
}
// the same with the final exponentiation cross-checked against its definition (tests)
int sg_pairing_check_slow(const uint8_t* g1_points, const uint8_t* g2_points, size_t n, int* ok) {
  return pairing_check_impl(g1_points, g2_points, n, ok, true);
}
// Keccak-256 as Ethereum uses it (`ethers::utils::keccak256`, zk_prover/src/merkle_sum_tree/entry.rs:21; the EVM
// transcript's hash, contracts/src/InclusionVerifier.sol:85-110): host utility for the host-language bindings
int sg_keccak256(const uint8_t* data, size_t len, uint8_t out[32]) {
  if (!out || (len && !data)) return fail(SG_ERR_INVALID, "sg_keccak256: null argument");
  const auto h = summa::prover::keccak256(data, len);
  std::memcpy(out, h.data(), 32);
  return SG_OK;
}
// ParamsKZG::<Bn256>::setup(k, rng) with tau supplied by the caller's RNG (zk_prover/src/circuits/
// utils.rs:70): g[i] = tau^i G, g_lagrange[i] = L_i(tau) G.  (g2 / s_g2 are verifier-side, not built.)
int sg_kzg_setup_dev(uint32_t k, const uint8_t tau[32], void* d_g, void* d_g_lagrange, void* stream) {
  if (!tau || !d_g || !d_g_lagrange || k > 28) return fail(SG_ERR_INVALID, "sg_kzg_setup: bad argument");
  LOCKED_CTX();
  const size_t n = (size_t)1 << k;
  hipError_t e = g_ctx->stage_a.reserve(n * 32);
  if (e == hipSuccess) e = g_ctx->stage_b.reserve(n * 32);
  if (e != hipSuccess) return hip_fail("staging buffer", e);
  hipStream_t s = pick_stream(stream);
  const words8 t = load32(tau);
  fp_words* pw = reinterpret_cast<fp_words*>(g_ctx->stage_a.p);
  fp_words* lg = reinterpret_cast<fp_words*>(g_ctx->stage_b.p);
  kzg_setup_scalars_launch(k, t, pw, lg, s);
  e = fixed_base_mul(pw, n, static_cast<g1_affine_mem*>(d_g), s);
  if (e == hipSuccess) e = fixed_base_mul(lg, n, static_cast<g1_affine_mem*>(d_g_lagrange), s);
  if (e == hipSuccess) e = host_wait_stream(s);  // staging buffers are reused by later calls
  if (e != hipSuccess) return hip_fail("kzg_setup", e);
  return SG_OK;
}
int sg_kzg_setup(uint32_t k, const uint8_t tau[32], uint8_t* g, uint8_t* g_lagrange) {
  if (!tau || !g || !g_lagrange || k > 28) return fail(SG_ERR_INVALID, "sg_kzg_setup: bad argument");
  const size_t bytes = (size_t)64 << k;
  void *dg = nullptr, *dl = nullptr;
  {
    LOCKED_CTX();
    CHECK_HIP(hipMalloc(&dg, bytes), "sg_kzg_setup");
    if (hipMalloc(&dl, bytes) != hipSuccess) {
      (void)hipFree(dg);
      return fail(SG_ERR_NOMEM, "sg_kzg_setup: out of device memory");
    }
  }
  int rc = sg_kzg_setup_dev(k, tau, dg, dl, nullptr);
  if (rc == SG_OK) {
    hipError_t e = hipMemcpy(g, dg, bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(g_lagrange, dl, bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = hip_fail("sg_kzg_setup", e);
  }
  (void)hipFree(dg);
  (void)hipFree(dl);
  return rc;
}

// N5: best_fft over G1 (FftGroup = G1) as used by ParamsKZG::downsize / g_to_lagrange:
// out[j] = sum_i omega^(ij) * in[i], optionally times `scale`; affine in, affine out.
int sg_g1_fft_dev(const void* d_in, void* d_out, const uint8_t omega[32], const uint8_t* scale, uint32_t log_n,
                  void* stream) {
  if (!d_in || !d_out || !omega || log_n > 28) return fail(SG_ERR_INVALID, "sg_g1_fft: bad argument");
  LOCKED_CTX();
  hipError_t e = g_ctx->scratch.reserve((size_t)144 << log_n);
  if (e != hipSuccess) return hip_fail("g1 fft work space", e);
  const words8 w = load32(omega), sc = scale ? load32(scale) : words8{};
  e = g1_fft(static_cast<const g1_affine_mem*>(d_in), static_cast<g1_affine_mem*>(d_out), log_n, w,
             scale ? &sc : nullptr, reinterpret_cast<xyzz29_mem*>(g_ctx->scratch.p), pick_stream(stream));
  if (e == hipSuccess) e = host_wait_stream(pick_stream(stream));  // scratch is shared with the NTT engine
  if (e != hipSuccess) return hip_fail("g1 fft", e);
  return SG_OK;
}
// ParamsKZG::downsize's recomputation of g_lagrange from g[0..2^k): iFFT over G1 (omega^-1, n^-1)
int sg_g1_to_lagrange(const uint8_t* g, uint32_t k, uint8_t* g_lagrange) {
  if (!g || !g_lagrange || k > 28) return fail(SG_ERR_INVALID, "sg_g1_to_lagrange: bad argument");
  const size_t bytes = (size_t)64 << k;
  words8 wi, ni;
  LOCKED_CTX();   // one lane for staging, transform and read-back
  {
    const DomainConsts* dc;
    TRY(get_consts(k, &dc));
    wi = dc->omega_inv;
    ni = dc->n_inv;
    TRY(upload(g_ctx->stage_a, g, bytes, g_ctx->stream));
    hipError_t e = g_ctx->stage_b.reserve(bytes);
    if (e != hipSuccess) return hip_fail("staging buffer", e);
    CHECK_HIP(host_wait_stream(g_ctx->stream), "stream sync");
  }
  int rc = sg_g1_fft_dev(g_ctx->stage_a.p, g_ctx->stage_b.p, reinterpret_cast<const uint8_t*>(&wi),
                         reinterpret_cast<const uint8_t*>(&ni), k, g_ctx->stream);
  if (rc != SG_OK) return rc;
  return download(g_lagrange, g_ctx->stage_b.p, bytes, g_ctx->stream);
}

int sg_fr_to_montgomery_dev(const void* d_in, void* d_out, size_t n, void* stream) {
  if (n && (!d_in || !d_out)) return fail(SG_ERR_INVALID, "null argument");
  LOCKED_CTX();
  hipError_t e = fr_montgomery(static_cast<const fp_words*>(d_in), static_cast<fp_words*>(d_out), n, 1, pick_stream(stream));
  if (e != hipSuccess) return hip_fail("fr_to_montgomery", e);
  return SG_OK;
}
int sg_lookup_permute_small_dev(const void* d_input, const void* d_table, size_t rows, void* d_permuted_input,
                                void* d_permuted_table, void* stream) {
  if (rows && (!d_input || !d_table || !d_permuted_input || !d_permuted_table)) return fail(SG_ERR_INVALID, "sg_lookup_permute: null argument");
  if (rows == 0) return SG_OK;
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  uint8_t* wb = nullptr;
  hipError_t e = scratch_for(s, 4, (LOOKUP_PERMUTE_WORK + 16) * sizeof(uint32_t), &wb);
  if (e != hipSuccess) return hip_fail("lookup permutation work space", e);
  uint32_t* work = reinterpret_cast<uint32_t*>(wb);
  uint32_t* flag = work + LOOKUP_PERMUTE_WORK;
  fp_words *pa = static_cast<fp_words*>(d_permuted_input), *ps = static_cast<fp_words*>(d_permuted_table);
  e = poly_lookup_permute_small(static_cast<const fp_words*>(d_input), static_cast<const fp_words*>(d_table), rows, work, pa, ps, flag, s);
  if (e == hipSuccess) e = fr_montgomery(pa, pa, rows, 1, s);
  if (e == hipSuccess) e = fr_montgomery(ps, ps, rows, 1, s);
  uint32_t h_flag = 0;
  if (e == hipSuccess) e = host_copy_d2h(&h_flag, flag, sizeof h_flag, s);
  if (e != hipSuccess) return hip_fail("lookup permutation", e);
  if (h_flag == 2) return fail(SG_ERR_UNSUPPORTED, "sg_lookup_permute_small: a table value is not below 2^16 (use the general path)");
  if (h_flag == 1) return fail(SG_ERR_WITNESS, "sg_lookup_permute_small: an input value is not in the table");
  return SG_OK;
}
int sg_lookup_permute_small_async_dev(const void* d_input, const void* d_table, size_t rows, void* d_permuted_input,
                                      void* d_permuted_table, void* d_status, void* stream) {
  if (!d_status || (rows && (!d_input || !d_table || !d_permuted_input || !d_permuted_table)))
    return fail(SG_ERR_INVALID, "sg_lookup_permute_small_async: null argument");
  if (rows == 0) return SG_OK;
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  Context::LookupWork& lw = g_ctx->lookup_work[s];
  constexpr size_t ONE = LOOKUP_PERMUTE_WORK + 16;   // words per work space, the two flag words behind the tables
  if (!lw.buf.p) {
    hipError_t e = lw.buf.reserve(2 * ONE);
    if (e == hipSuccess) e = hipMemsetAsync(lw.buf.p, 0, lw.buf.cap * sizeof(uint32_t), s);   // once per stream; afterwards every call cleans for the next
    if (e != hipSuccess) return hip_fail("lookup permutation work space", e);
    lw.next = 0;
  }
  uint32_t* work = lw.buf.p + lw.next * ONE;
  uint32_t* other = lw.buf.p + (lw.next ^ 1u) * ONE;
  lw.next ^= 1u;
  hipError_t e = poly_lookup_permute_small_chained(static_cast<const fp_words*>(d_input), static_cast<const fp_words*>(d_table), rows, work,
                                                   work + LOOKUP_PERMUTE_WORK, other, other + LOOKUP_PERMUTE_WORK,
                                                   static_cast<fp_words*>(d_permuted_input), static_cast<fp_words*>(d_permuted_table),
                                                   static_cast<uint32_t*>(d_status), s);
  if (e != hipSuccess) return hip_fail("lookup permutation", e);
  return SG_OK;
}
// The general path: one launch sequence for both forms.  The work space is the stream's own (scratch_for, slot 9): calls on one
// stream are ordered, so each may reuse what the one before it used, and a larger `rows` grows the buffer by DevBuf::reserve's rule
// -- the outgrown block is retired, not freed (devmem.h), so launches already queued on the stream keep reading valid memory.  A
// call with the same or fewer rows allocates nothing.
static int lookup_permute_launch(const char* who, const void* d_input, const void* d_table, size_t rows, void* d_permuted_input,
                                 void* d_permuted_table, void* d_status, hipStream_t s, uint32_t** work_out) {
  if (rows > LS_MAX_ROWS) return fail(SG_ERR_INVALID, "sg_lookup_permute: at most 2^31 - 1 rows");
  uint8_t* wb = nullptr;
  hipError_t e = scratch_for(s, 9, lookup_sort_work_bytes(rows), &wb);
  if (e != hipSuccess) return hip_fail("lookup permutation work space", e);
  uint32_t* work = reinterpret_cast<uint32_t*>(wb);
  e = poly_lookup_permute(static_cast<const fp_words*>(d_input), static_cast<const fp_words*>(d_table), rows, work,
                          static_cast<fp_words*>(d_permuted_input), static_cast<fp_words*>(d_permuted_table),
                          static_cast<uint32_t*>(d_status), s);
  if (e != hipSuccess) return hip_fail(who, e);
  *work_out = work;
  return SG_OK;
}
int sg_lookup_permute_dev(const void* d_input, const void* d_table, size_t rows, void* d_permuted_input, void* d_permuted_table,
                          void* stream) {
  if (rows && (!d_input || !d_table || !d_permuted_input || !d_permuted_table)) return fail(SG_ERR_INVALID, "sg_lookup_permute: null argument");
  if (rows == 0) return SG_OK;
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  uint32_t* work = nullptr;
  TRY(lookup_permute_launch("sg_lookup_permute", d_input, d_table, rows, d_permuted_input, d_permuted_table, nullptr, s, &work));
  uint32_t h_flag = 0;
  hipError_t e = host_copy_d2h(&h_flag, work + LS_FLAG, sizeof h_flag, s);
  if (e != hipSuccess) return hip_fail("lookup permutation", e);
  if (h_flag) return fail(SG_ERR_WITNESS, "sg_lookup_permute: an input value is not in the table");
  return SG_OK;
}
int sg_lookup_permute_async_dev(const void* d_input, const void* d_table, size_t rows, void* d_permuted_input, void* d_permuted_table,
                                void* d_status, void* stream) {
  if (!d_status || (rows && (!d_input || !d_table || !d_permuted_input || !d_permuted_table)))
    return fail(SG_ERR_INVALID, "sg_lookup_permute_async: null argument");
  if (rows == 0) return SG_OK;
  LOCKED_CTX();
  uint32_t* work = nullptr;
  return lookup_permute_launch("sg_lookup_permute_async", d_input, d_table, rows, d_permuted_input, d_permuted_table, d_status,
                               pick_stream(stream), &work);
}
int sg_fr_flag_noncanonical_dev(const void* const* d_cols, uint32_t m, size_t n, void* d_flag, void* stream) {
  if (!d_flag || (m && !d_cols) || m > 16) return fail(SG_ERR_INVALID, "sg_fr_flag_noncanonical: bad argument");
  for (uint32_t j = 0; j < m; j++)
    if (n && !d_cols[j]) return fail(SG_ERR_INVALID, "sg_fr_flag_noncanonical: null column");
  if (n >= (1ull << 32)) return fail(SG_ERR_INVALID, "sg_fr_flag_noncanonical: column too long");
  LOCKED_CTX();
  hipError_t e = poly_flag_noncanonical(reinterpret_cast<const fp_words* const*>(d_cols), m, n, static_cast<uint32_t*>(d_flag), pick_stream(stream));
  if (e != hipSuccess) return hip_fail("flag_noncanonical", e);
  return SG_OK;
}
int sg_fr_random_dev(const uint8_t key[32], uint64_t stream_id, void* d_out, size_t n, void* stream) {
  if (!key || (n && !d_out)) return fail(SG_ERR_INVALID, "sg_fr_random: null argument");
  LOCKED_CTX();
  uint32_t k[8];
  std::memcpy(k, key, 32);
  hipError_t e = poly_random(k, stream_id, n, static_cast<fp_words*>(d_out), pick_stream(stream));
  if (e != hipSuccess) return hip_fail("fr_random", e);
  return SG_OK;
}
int sg_fr_random_batch_dev(const uint8_t key[32], uint64_t first_stream_id, void* const* d_out, const size_t* n, uint32_t m, void* stream) {
  if (!key || (m && (!d_out || !n)) || m > RANDOM_BATCH_MAX) return fail(SG_ERR_INVALID, "sg_fr_random_batch: bad argument");
  for (uint32_t d = 0; d < m; d++)
    if (n[d] && !d_out[d]) return fail(SG_ERR_INVALID, "sg_fr_random_batch: null output");
  LOCKED_CTX();
  uint32_t k[8];
  std::memcpy(k, key, 32);
  hipError_t e = poly_random_batch(k, first_stream_id, m, reinterpret_cast<fp_words* const*>(d_out), n, pick_stream(stream));
  if (e != hipSuccess) return hip_fail("fr_random", e);
  return SG_OK;
}
int sg_fr_from_montgomery_dev(const void* d_in, void* d_out, size_t n, void* stream) {
  if (n && (!d_in || !d_out)) return fail(SG_ERR_INVALID, "null argument");
  LOCKED_CTX();
  hipError_t e = fr_montgomery(static_cast<const fp_words*>(d_in), static_cast<fp_words*>(d_out), n, 0, pick_stream(stream));
  if (e != hipSuccess) return hip_fail("fr_from_montgomery", e);
  return SG_OK;
}

// ------------------------------------------------------------------ polynomial helpers
int sg_fr_eval_poly_dev(const void* d_coeffs, size_t n, const uint8_t x[32], void* stream, uint8_t out[32]) {
  if (!x || !out || (n && !d_coeffs)) return fail(SG_ERR_INVALID, "sg_fr_eval_poly: null argument");
  if (n >= (1ull << 32)) return fail(SG_ERR_INVALID, "sg_fr_eval_poly: polynomial too long");
  if (n == 0) {
    std::memset(out, 0, 32);
    return SG_OK;
  }
  LOCKED_CTX();
  const size_t t = poly_eval_tmp_elems(n);
  hipError_t e = g_ctx->scratch.reserve((2 * t + 1) * 32);
  if (e != hipSuccess) return hip_fail("eval_poly work space", e);
  fp_words* tmp = reinterpret_cast<fp_words*>(g_ctx->scratch.p);
  const words8 xw = load32(x);
  hipStream_t s = pick_stream(stream);
  e = poly_eval(static_cast<const fp_words*>(d_coeffs), n, xw, tmp, tmp + t, tmp + 2 * t, s);
  if (e != hipSuccess) return hip_fail("eval_poly", e);
  return download(out, tmp + 2 * t, 32, s);
}
// The evaluation phase of a proof (35 eval_polynomial calls for MstInclusion) as batches: every polynomial
// at its own point, two launches and one read-back per batch of 40
int sg_fr_eval_poly_batch_dev(const void* const* d_polys, size_t n, const uint8_t* points, uint32_t m, void* stream,
                              uint8_t* out) {
  if (m && (!d_polys || !points || !out)) return fail(SG_ERR_INVALID, "sg_fr_eval_poly_batch: null argument");
  if (n > EVAL_BATCH_MAX_N) return fail(SG_ERR_INVALID, "sg_fr_eval_poly_batch: polynomial too long");
  if (m == 0) return SG_OK;
  if (n == 0) {
    std::memset(out, 0, 32 * (size_t)m);
    return SG_OK;
  }
  for (uint32_t j = 0; j < m; j++)
    if (!d_polys[j]) return fail(SG_ERR_INVALID, "sg_fr_eval_poly_batch: null polynomial");
  LOCKED_CTX();
  hipError_t e = g_ctx->scratch.reserve(eval_batch_tmp_elems(n) * 32);
  if (e != hipSuccess) return hip_fail("eval_poly work space", e);
  fp_words* partial = reinterpret_cast<fp_words*>(g_ctx->scratch.p);
  // the values land in page-locked host memory the last kernel writes directly: the host waits for the stream once and reads them
  uint8_t *h_mail = nullptr, *d_mail = nullptr;
  e = mailbox(&h_mail, &d_mail);
  if (e != hipSuccess) return hip_fail("eval_poly mailbox", e);
  static_assert(EVAL_BATCH_MAX * 32 <= Context::MAIL_BYTES, "the mailbox holds one batch of evaluations");
  hipStream_t s = pick_stream(stream);
  for (uint32_t first = 0; first < m; first += EVAL_BATCH_MAX) {
    const uint32_t cnt = eval_batch_count(m, first);
    words8 xs[EVAL_BATCH_MAX];
    std::memcpy(xs, points + 32 * (size_t)first, 32 * (size_t)cnt);
    e = poly_eval_batch(reinterpret_cast<const fp_words* const*>(d_polys + first), xs, cnt, n, partial, reinterpret_cast<fp_words*>(d_mail), s);
    if (e == hipSuccess) e = host_wait_stream(s);   // synchronises: scratch and mailbox are reused
    if (e != hipSuccess) return hip_fail("eval_poly_batch", e);
    std::memcpy(out + 32 * (size_t)first, h_mail, 32 * (size_t)cnt);
  }
  return SG_OK;
}
int sg_fr_eval_poly(const uint8_t* coeffs, size_t n, const uint8_t x[32], uint8_t out[32]) {
  if (!x || !out || (n && !coeffs)) return fail(SG_ERR_INVALID, "sg_fr_eval_poly: null argument");
  LOCKED_CTX();   // the staging buffer is this lane's until the evaluation has read it
  TRY(upload(g_ctx->stage_a, coeffs, n * 32, g_ctx->stream));
  return sg_fr_eval_poly_dev(g_ctx->stage_a.p, n, x, g_ctx->stream, out);
}
int sg_fr_batch_invert_dev(void* d_a, size_t n, void* stream) {
  if (n && !d_a) return fail(SG_ERR_INVALID, "sg_fr_batch_invert: null argument");
  if (n >= (1ull << 32)) return fail(SG_ERR_INVALID, "sg_fr_batch_invert: vector too long");
  LOCKED_CTX();
  hipError_t e = poly_batch_invert(static_cast<fp_words*>(d_a), n, pick_stream(stream));
  if (e != hipSuccess) return hip_fail("batch_invert", e);
  return SG_OK;
}
int sg_fr_prefix_product_dev(const void* d_a, size_t n, void* d_out, void* stream) {
  if (!d_out || (n && !d_a)) return fail(SG_ERR_INVALID, "sg_fr_prefix_product: null argument");
  if (n > PREFIX_MAX_SPAN - 1) return fail(SG_ERR_INVALID, "sg_fr_prefix_product: at most 2^21 - 1 elements");
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  uint8_t* tmp = nullptr;
  hipError_t e = scratch_for(s, 0, prefix_product_tmp_elems(n + 1) * 32 + 64, &tmp);
  if (e != hipSuccess) return hip_fail("prefix_product work space", e);
  e = poly_prefix_product(static_cast<const fp_words*>(d_a), n, reinterpret_cast<fp_words*>(tmp),
                          static_cast<fp_words*>(d_out), n + 1, nullptr, s);
  if (e != hipSuccess) return hip_fail("prefix_product", e);
  return SG_OK;
}
static int grand_product_tail(fp_words* d_mod, size_t n, const uint8_t* z0, void* d_z, hipStream_t s) {
  // z[0] = z0 (or 1), z[i] = z[i-1] * mod[i-1], n values
  uint8_t* tmp = nullptr;
  hipError_t e = scratch_for(s, 0, prefix_product_tmp_elems(n + 1) * 32 + 64, &tmp);
  if (e != hipSuccess) return hip_fail("grand product work space", e);
  const words8 init = z0 ? load32(z0) : words8{};
  e = poly_prefix_product(d_mod, n, reinterpret_cast<fp_words*>(tmp), static_cast<fp_words*>(d_z), n,
                          z0 ? &init : nullptr, s);
  if (e != hipSuccess) return hip_fail("grand product", e);
  return SG_OK;  // asynchronous: ordered on the caller's stream
}
int sg_permutation_product_dev(const void* const* d_values, const void* const* d_sigma, uint32_t ncols,
                               const uint8_t beta[32], const uint8_t gamma[32], const uint8_t delta_start[32],
                               uint32_t k, const uint8_t* z0, void* d_z, void* stream) {
  if (!d_values || !d_sigma || !beta || !gamma || !delta_start || !d_z || ncols == 0 || ncols > PERM_MAX_COLS ||
      k > GRAND_MAX_K)
    return fail(SG_ERR_INVALID, "sg_permutation_product: bad argument");
  LOCKED_CTX();
  const size_t n = (size_t)1 << k;
  const DomainConsts* dc;
  TRY(get_consts(k, &dc));
  PermCols cols{};
  for (uint32_t c = 0; c < ncols; c++) {
    if (!d_values[c] || !d_sigma[c]) return fail(SG_ERR_INVALID, "sg_permutation_product: null column");
    cols.values[c] = static_cast<const fp_words*>(d_values[c]);
    cols.sigma[c] = static_cast<const fp_words*>(d_sigma[c]);
  }
  hipStream_t s = pick_stream(stream);
  uint8_t* modb = nullptr;
  hipError_t e = scratch_for(s, 1, n * 32 + 64, &modb);
  if (e != hipSuccess) return hip_fail("grand product work space", e);
  fp_words* mod = reinterpret_cast<fp_words*>(modb);
  const words8 b = load32(beta), g = load32(gamma), ds = load32(delta_start), &dl = DELTA_M;
  e = poly_perm_fraction(cols, ncols, b, g, ds, dl, n, 0, mod, s);
  if (e == hipSuccess) e = poly_batch_invert(mod, n, s);
  fp_words* pw = nullptr;   // omega^i, i < n (cached per domain): one product instead of one exponentiation per row
  if (e == hipSuccess) e = g_ctx->ntt.local_twiddles(dc->omega, k + 1, s, &pw);
  if (e == hipSuccess) e = poly_perm_fraction(cols, ncols, b, g, ds, dl, n, 1, mod, s, pw);
  if (e != hipSuccess) return hip_fail("permutation product", e);
  return grand_product_tail(mod, n, z0, d_z, s);
}
int sg_lookup_product_dev(const void* d_input, const void* d_table, const void* d_permuted_input,
                          const void* d_permuted_table, const uint8_t beta[32], const uint8_t gamma[32], size_t n,
                          void* d_z, void* stream) {
  if (!d_input || !d_table || !d_permuted_input || !d_permuted_table || !beta || !gamma || !d_z || n == 0 ||
      n > PREFIX_MAX_SPAN - 1)
    return fail(SG_ERR_INVALID, "sg_lookup_product: bad argument");
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  uint8_t* modb = nullptr;
  hipError_t e = scratch_for(s, 1, n * 32 + 64, &modb);
  if (e != hipSuccess) return hip_fail("grand product work space", e);
  fp_words* mod = reinterpret_cast<fp_words*>(modb);
  const words8 b = load32(beta), g = load32(gamma);
  e = poly_lookup_fraction(static_cast<const fp_words*>(d_permuted_input), static_cast<const fp_words*>(d_permuted_table),
                           b, g, n, 0, mod, s);
  if (e == hipSuccess) e = poly_batch_invert(mod, n, s);
  if (e == hipSuccess)
    e = poly_lookup_fraction(static_cast<const fp_words*>(d_input), static_cast<const fp_words*>(d_table), b, g, n, 1,
                             mod, s);
  if (e != hipSuccess) return hip_fail("lookup product", e);
  return grand_product_tail(mod, n, nullptr, d_z, s);
}

int sg_grand_products_dev(const void* const* d_values, const void* const* d_sigma, const uint32_t* chunk_cols, uint32_t n_chunks,
                          const void* const* d_lookup_cols, uint32_t n_lookups, const uint8_t beta[32], const uint8_t gamma[32],
                          uint32_t k, size_t usable_rows, void* const* d_z, void* stream) {
  return sg_grand_products_closing_dev(d_values, d_sigma, chunk_cols, n_chunks, d_lookup_cols, n_lookups, beta, gamma, k, usable_rows, d_z,
                                       nullptr, stream);
}
int sg_grand_products_closing_dev(const void* const* d_values, const void* const* d_sigma, const uint32_t* chunk_cols, uint32_t n_chunks,
                                  const void* const* d_lookup_cols, uint32_t n_lookups, const uint8_t beta[32], const uint8_t gamma[32],
                                  uint32_t k, size_t usable_rows, void* const* d_z, void* d_closing, void* stream) {
  if (!beta || !gamma || !d_z || (n_chunks && (!d_values || !d_sigma || !chunk_cols)) || (n_lookups && !d_lookup_cols))
    return fail(SG_ERR_INVALID, "sg_grand_products: null argument");
  if (n_chunks + n_lookups == 0) return SG_OK;
  if (n_chunks + n_lookups > GRAND_MAX) return fail(SG_ERR_INVALID, "sg_grand_products: at most 8 products per call");
  if (k == 0 || k > GRAND_MAX_K) return fail(SG_ERR_INVALID, "sg_grand_products: 1 <= k <= 21");
  const size_t n = (size_t)1 << k;
  if (usable_rows >= n) return fail(SG_ERR_INVALID, "sg_grand_products: usable_rows must be below 2^k");
  LOCKED_CTX();
  const DomainConsts* dc;
  TRY(get_consts(k, &dc));
  GrandProducts g{};
  GrandOut outs{};
  g.n_perm = n_chunks;
  g.n_lookup = n_lookups;
  // delta^(index of the chunk's first column), on the host: a handful of products in the memory domain
  summa::prover::Fr dpow = summa::prover::Fr::one(), dlt;
  std::memcpy(dlt.l, &DELTA_M, 32);
  uint32_t col = 0;
  for (uint32_t j = 0; j < n_chunks; j++) {
    if (chunk_cols[j] == 0 || chunk_cols[j] > PERM_MAX_COLS) return fail(SG_ERR_INVALID, "sg_grand_products: 1 .. 8 columns per chunk");
    g.ncols[j] = chunk_cols[j];
    std::memcpy(g.delta_start[j].l, dpow.l, 32);
    for (uint32_t c = 0; c < chunk_cols[j]; c++, col++) {
      if (!d_values[col] || !d_sigma[col]) return fail(SG_ERR_INVALID, "sg_grand_products: null column");
      g.perm[j].values[c] = static_cast<const fp_words*>(d_values[col]);
      g.perm[j].sigma[c] = static_cast<const fp_words*>(d_sigma[col]);
      dpow = dpow * dlt;
    }
  }
  for (uint32_t l = 0; l < n_lookups; l++)
    for (int q = 0; q < 4; q++) {
      if (!d_lookup_cols[4 * l + q]) return fail(SG_ERR_INVALID, "sg_grand_products: null lookup column");
      g.lookup[l][q] = static_cast<const fp_words*>(d_lookup_cols[4 * l + q]);
    }
  for (uint32_t p = 0; p < n_chunks + n_lookups; p++) {
    if (!d_z[p]) return fail(SG_ERR_INVALID, "sg_grand_products: null output");
    outs.z[p] = static_cast<fp_words*>(d_z[p]);
  }
  outs.closing = static_cast<fp_words*>(d_closing);
  outs.closing_row = (uint32_t)usable_rows;
  hipStream_t s = pick_stream(stream);
  uint8_t *modb = nullptr, *tmpb = nullptr;
  hipError_t e = scratch_for(s, 1, grand_products_mod_elems(n, n_chunks + n_lookups) * 32 + 64, &modb);
  if (e == hipSuccess) e = scratch_for(s, 0, grand_products_tmp_elems(n, n_chunks + n_lookups) * 32 + 64, &tmpb);
  if (e != hipSuccess) return hip_fail("grand products work space", e);
  fp_words* pw = nullptr;   // omega^i, i < n (cached per domain)
  if (n_chunks) {
    e = g_ctx->ntt.local_twiddles(dc->omega, k + 1, s, &pw);
    if (e != hipSuccess) return hip_fail("grand products: power table", e);
  }
  e = poly_grand_products(g, load32(beta), load32(gamma), DELTA_M, n, usable_rows, pw, reinterpret_cast<fp_words*>(modb), reinterpret_cast<fp_words*>(tmpb), outs, s);
  if (e != hipSuccess) return hip_fail("grand products", e);
  return SG_OK;   // asynchronous: ordered on the caller's stream
}

int sg_fr_mul_dev(const void* d_a, const void* d_b, size_t n, void* d_out, void* stream) {
  if (n && (!d_a || !d_b || !d_out)) return fail(SG_ERR_INVALID, "sg_fr_mul: null argument");
  if (n >= (1ull << 32)) return fail(SG_ERR_INVALID, "sg_fr_mul: vector too long");
  LOCKED_CTX();
  hipError_t e = poly_mul_elementwise(static_cast<const fp_words*>(d_a), static_cast<const fp_words*>(d_b), n,
                                      static_cast<fp_words*>(d_out), pick_stream(stream));
  if (e != hipSuccess) return hip_fail("fr_mul", e);
  return SG_OK;
}

// halo2's kate_division(a, b) (arithmetic.rs): the quotient of a(X) by (X - b), as SHPLONK's multi-open
// applies it once per opening point; remainder = a(b) comes for free
int sg_fr_kate_division_dev(const void* d_a, size_t n, const uint8_t b[32], void* d_q, uint8_t* remainder_out,
                            void* stream) {
  if (!b || (n && (!d_a || !d_q))) return fail(SG_ERR_INVALID, "sg_fr_kate_division: null argument");
  if (n > KATE_MAX_N) return fail(SG_ERR_INVALID, "sg_fr_kate_division: at most 2^21 coefficients");
  if (d_a == d_q && n) return fail(SG_ERR_INVALID, "sg_fr_kate_division: the quotient must not alias the input");
  if (n == 0) {
    if (remainder_out) std::memset(remainder_out, 0, 32);
    return SG_OK;
  }
  LOCKED_CTX();
  const words8 bw = load32(b);
  hipStream_t s = pick_stream(stream);
  uint8_t* tb = nullptr;
  hipError_t e = scratch_for(s, 0, kate_tmp_elems() * 32 + 64, &tb);
  if (e != hipSuccess) return hip_fail("kate_division work space", e);
  fp_words* tmp = reinterpret_cast<fp_words*>(tb);
  uint8_t *h_mail = nullptr, *d_mail = nullptr;
  if (remainder_out) {
    e = mailbox(&h_mail, &d_mail);
    if (e != hipSuccess) return hip_fail("kate_division mailbox", e);
  }
  e = poly_kate_division(static_cast<const fp_words*>(d_a), n, bw, tmp, static_cast<fp_words*>(d_q),
                         remainder_out ? reinterpret_cast<fp_words*>(d_mail) : nullptr, s);
  // asynchronous unless the caller wants the remainder on the host (written by the kernel into mapped host memory)
  if (e == hipSuccess && remainder_out) {
    e = host_wait_stream(s);
    if (e == hipSuccess) std::memcpy(remainder_out, h_mail, 32);
  }
  if (e != hipSuccess) return hip_fail("kate_division", e);
  return SG_OK;
}
int sg_fr_kate_division_rem_dev(const void* d_a, size_t n, const uint8_t b[32], void* d_q, void* d_remainder, void* stream) {
  if (!b || !d_remainder || (n && (!d_a || !d_q))) return fail(SG_ERR_INVALID, "sg_fr_kate_division_rem: null argument");
  if (n == 0 || n > KATE_MAX_N) return fail(SG_ERR_INVALID, "sg_fr_kate_division_rem: between 1 and 2^21 coefficients");
  if (d_a == d_q) return fail(SG_ERR_INVALID, "sg_fr_kate_division_rem: the quotient must not alias the input");
  LOCKED_CTX();
  const words8 bw = load32(b);
  hipStream_t s = pick_stream(stream);
  uint8_t* tb = nullptr;
  hipError_t e = scratch_for(s, 0, kate_tmp_elems() * 32 + 64, &tb);
  if (e != hipSuccess) return hip_fail("kate_division work space", e);
  e = poly_kate_division(static_cast<const fp_words*>(d_a), n, bw, reinterpret_cast<fp_words*>(tb), static_cast<fp_words*>(d_q),
                         static_cast<fp_words*>(d_remainder), s);
  if (e != hipSuccess) return hip_fail("kate_division", e);
  return SG_OK;
}
// m <= 16 exact divisions q_j = a_j / (X - b_j) in one launch per scan step (a_j may repeat: by partial fractions the
// divisions of one rotation set are independent divisions of the same polynomial).  Asynchronous on `stream`.
// how many elements of the given columns are not canonical (word value >= r)?  Asynchronous: *d_count (a u32 in device
// memory) holds the number once the stream reaches this point.
int sg_fr_count_noncanonical_dev(const void* const* d_cols, uint32_t m, size_t n, void* d_count, void* stream) {
  if (!d_count || (m && !d_cols)) return fail(SG_ERR_INVALID, "sg_fr_count_noncanonical: null argument");
  if (m > 16) return fail(SG_ERR_INVALID, "sg_fr_count_noncanonical: at most 16 columns per call");
  if (n > 0xffffffffull) return fail(SG_ERR_INVALID, "sg_fr_count_noncanonical: too many rows");
  for (uint32_t j = 0; j < m; j++)
    if (n && !d_cols[j]) return fail(SG_ERR_INVALID, "sg_fr_count_noncanonical: null column");
  LOCKED_CTX();
  hipError_t e = poly_count_noncanonical(reinterpret_cast<const fp_words* const*>(d_cols), m, n, reinterpret_cast<uint32_t*>(d_count),
                                         reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail("count_noncanonical", e);
  return SG_OK;
}
int sg_fr_kate_division_batch_dev(const void* const* d_a, size_t n, const uint8_t* points, uint32_t m, void* const* d_q,
                                  void* stream) {
  if (m && (!d_a || !points || !d_q)) return fail(SG_ERR_INVALID, "sg_fr_kate_division_batch: null argument");
  if (m > KATE_BATCH_MAX) return fail(SG_ERR_INVALID, "sg_fr_kate_division_batch: at most 16 divisions per call");
  if (n > KATE_MAX_N) return fail(SG_ERR_INVALID, "sg_fr_kate_division_batch: at most 2^21 coefficients");
  for (uint32_t j = 0; j < m; j++)
    if (n && (!d_a[j] || !d_q[j] || d_a[j] == d_q[j])) return fail(SG_ERR_INVALID, "sg_fr_kate_division_batch: bad vector");
  if (m == 0 || n == 0) return SG_OK;
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  uint8_t* d_tmp = nullptr;
  hipError_t e = scratch_for(s, 6, kate_batch_tmp_elems(n, KATE_BATCH_MAX) * 32 + 64, &d_tmp);
  if (e != hipSuccess) return hip_fail("kate_division_batch work space", e);
  std::vector<words8> b(m);
  std::memcpy(b.data(), points, 32 * (size_t)m);
  // the power tables are computed on the host into page-locked memory of a ring slot and copied from there: asynchronous (the
  // call used to wait for the whole stream so that a local staging buffer could die -- 0.16 ms of a proof with the device idle
  // behind it); a slot is reused once the kernels that read it have run (an event; normally long complete)
  Context::BlobSlot* slot_p = nullptr;
  e = ring_slot(g_ctx->kate_ring, kate_batch_powers_bytes(KATE_BATCH_MAX), kate_batch_powers_bytes(KATE_BATCH_MAX), &slot_p);
  Context::BlobSlot& slot = *slot_p;
  if (e == hipSuccess)
    e = poly_kate_division_batch(reinterpret_cast<const fp_words* const*>(d_a), n, b.data(), m, reinterpret_cast<fp_words* const*>(d_q),
                                 slot.host, slot.dev, reinterpret_cast<fp_words*>(d_tmp), s);
  if (e == hipSuccess) e = hipEventRecord(slot.ev, s);
  if (e != hipSuccess) return hip_fail("kate_division_batch", e);
  return SG_OK;
}
// out[i] = sum_j coeffs[j] * polys[j][i]: the random linear combinations of SHPLONK / multi-open
int sg_fr_lincomb_dev(const void* const* d_polys, const uint8_t* coeffs, uint32_t m, size_t n, void* d_out, void* stream) {
  if (!d_polys || !coeffs || (n && !d_out)) return fail(SG_ERR_INVALID, "sg_fr_lincomb: null argument");
  if (m == 0 || m > LINCOMB_MAX) return fail(SG_ERR_INVALID, "sg_fr_lincomb: between 1 and 32 polynomials");
  if (n >= (1ull << 32)) return fail(SG_ERR_INVALID, "sg_fr_lincomb: vector too long");
  for (uint32_t j = 0; j < m; j++)
    if (n && !d_polys[j]) return fail(SG_ERR_INVALID, "sg_fr_lincomb: null polynomial");
  LOCKED_CTX();
  words8 cw[LINCOMB_MAX];
  std::memcpy(cw, coeffs, 32 * (size_t)m);
  hipError_t e = poly_lincomb(reinterpret_cast<const fp_words* const*>(d_polys), cw, m, n, static_cast<fp_words*>(d_out),
                              pick_stream(stream));
  if (e != hipSuccess) return hip_fail("lincomb", e);
  return SG_OK;
}

int sg_fr_lincomb_low_dev(const void* const* d_polys, const uint8_t* coeffs, uint32_t m, size_t n, const uint8_t* low, uint32_t n_low,
                          void* d_out, void* stream) {
  if ((m && (!d_polys || !coeffs)) || (n && !d_out) || (n_low && !low)) return fail(SG_ERR_INVALID, "sg_fr_lincomb_low: null argument");
  if (m > LINCOMB_MAX) return fail(SG_ERR_INVALID, "sg_fr_lincomb_low: at most 32 polynomials");
  if (n >= (1ull << 32) || n_low > LINCOMB_LOW_MAX || n_low > n) return fail(SG_ERR_INVALID, "sg_fr_lincomb_low: bad length");
  for (uint32_t j = 0; j < m; j++)
    if (n && !d_polys[j]) return fail(SG_ERR_INVALID, "sg_fr_lincomb_low: null polynomial");
  LOCKED_CTX();
  words8 cw[LINCOMB_MAX], lw[LINCOMB_LOW_MAX];
  if (m) std::memcpy(cw, coeffs, 32 * (size_t)m);
  if (n_low) std::memcpy(lw, low, 32 * (size_t)n_low);
  hipError_t e = poly_lincomb(reinterpret_cast<const fp_words* const*>(d_polys), cw, m, n, static_cast<fp_words*>(d_out),
                              pick_stream(stream), lw, n_low);
  if (e != hipSuccess) return hip_fail("lincomb", e);
  return SG_OK;
}

int sg_fr_lincomb_sets_dev(const void* const* d_polys, const uint8_t* coeffs, const uint32_t* set_sizes, uint32_t n_sets, size_t n,
                           const uint8_t* lows, const uint32_t* n_lows, void* const* d_outs, void* stream) {
  if (!d_polys || !coeffs || !set_sizes || !d_outs || n_sets == 0 || n_sets > LINCOMB_SETS_MAX) return fail(SG_ERR_INVALID, "sg_fr_lincomb_sets: bad argument");
  if (n >= (1ull << 32)) return fail(SG_ERR_INVALID, "sg_fr_lincomb_sets: vector too long");
  uint32_t first[LINCOMB_SETS_MAX + 1] = {0}, nl[LINCOMB_SETS_MAX] = {0};
  for (uint32_t s = 0; s < n_sets; s++) {
    if (set_sizes[s] > LINCOMB_MAX) return fail(SG_ERR_INVALID, "sg_fr_lincomb_sets: at most 32 polynomials per combination");
    first[s + 1] = first[s] + set_sizes[s];
    nl[s] = n_lows ? n_lows[s] : 0;
    if (nl[s] > LINCOMB_SETS_LOW || nl[s] > n || (nl[s] && !lows)) return fail(SG_ERR_INVALID, "sg_fr_lincomb_sets: at most 4 low coefficients per combination");
    if (n && !d_outs[s]) return fail(SG_ERR_INVALID, "sg_fr_lincomb_sets: null output");
  }
  if (first[n_sets] > LINCOMB_SETS_POLYS) return fail(SG_ERR_INVALID, "sg_fr_lincomb_sets: at most 48 polynomials in all");
  for (uint32_t j = 0; j < first[n_sets]; j++)
    if (n && !d_polys[j]) return fail(SG_ERR_INVALID, "sg_fr_lincomb_sets: null polynomial");
  LOCKED_CTX();
  words8 cw[LINCOMB_SETS_POLYS], lw[LINCOMB_SETS_MAX * LINCOMB_SETS_LOW];
  std::memcpy(cw, coeffs, 32 * (size_t)first[n_sets]);
  std::memset(lw, 0, sizeof lw);
  if (lows) std::memcpy(lw, lows, 32 * (size_t)n_sets * LINCOMB_SETS_LOW);
  hipError_t e = poly_lincomb_sets(reinterpret_cast<const fp_words* const*>(d_polys), cw, first, n_sets, n, lw, nl,
                                   reinterpret_cast<fp_words* const*>(d_outs), pick_stream(stream));
  if (e != hipSuccess) return hip_fail("lincomb sets", e);
  return SG_OK;
}

}  // extern "C"
