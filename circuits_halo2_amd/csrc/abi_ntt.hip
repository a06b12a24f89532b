// C ABI, transform family: NTTs, the extended domain, the cosets of the quotient, the vanishing polynomial (summa_gpu.hip
// holds the core).
#include "abi_internal.h"
#include "coset_plan.h"

using namespace sg;
namespace {

// `count` transforms of one size on `s`: batched while ntt_batched(log_n) holds, NTT_BATCH_MAX of them per launch, otherwise one
// after the other (pre_tab: batched sizes only).  ins == nullptr: in place, and multi-pass plans then need a scratch vector per
// transform -- slot 3 of the stream, reserved once, for the largest chunk, before the first launch (growing it frees the old
// buffer, which waits for the device).
int transforms(fp_words* const* outs, const fp_words* const* ins, size_t in_len, size_t count, uint32_t log_n,
               const words8& omega, const words8* divisor, const words8* pre3, const fp_words* const* pre_tab,
               hipStream_t s, const char* what) {
  if (!ntt_batched(log_n)) {
    if (pre_tab) return fail(SG_ERR_INVALID, what);
    for (size_t i = 0; i < count; i++)
      TRY(ntt_dev(ins ? ins[i] : outs[i], ins ? in_len : (size_t)1 << log_n, outs[i], log_n, omega, divisor, pre3, nullptr, s));
    return SG_OK;
  }
  uint8_t* scr = nullptr;
  if (count && ntt_needs_scratch(g_ctx->ntt.config(), log_n, !ins)) {
    hipError_t e = scratch_for(s, 3, std::min<size_t>(count, NTT_BATCH_MAX) * ((size_t)32 << log_n), &scr);
    if (e != hipSuccess) return hip_fail("ntt scratch", e);
  }
  for (size_t first = 0; first < count; first += NTT_BATCH_MAX) {
    const uint32_t cnt = (uint32_t)std::min<size_t>(NTT_BATCH_MAX, count - first);
    hipError_t e = g_ctx->ntt.transform_batch(outs + first, cnt, reinterpret_cast<fp_words*>(scr), log_n, omega, divisor, s,
                                              ins ? ins + first : nullptr, in_len, pre3, pre_tab ? pre_tab + first : nullptr);
    if (e != hipSuccess) return hip_fail(what, e);
  }
  return SG_OK;
}

// the host-pointer form of an in-place `_dev` call: through the lane's staging buffer, on the lane's own stream (the lane
// lock is re-entrant, and the `_dev` form has nothing to order against on that stream)
template <class DevCall>
int staged_in_place(uint8_t* host, size_t bytes, DevCall dev_call) {
  LOCKED_CTX();
  TRY(upload(g_ctx->stage_a, host, bytes, g_ctx->stream));
  TRY(dev_call(g_ctx->stage_a.p, g_ctx->stream));
  return download(host, g_ctx->stage_a.p, bytes, g_ctx->stream);
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------ NTT family
int sg_ntt_fr_dev(void* d_a, const uint8_t omega[32], uint32_t log_n, void* stream) {
  if (!d_a || !omega) return fail(SG_ERR_INVALID, "sg_ntt_fr: null argument");
  LOCKED_CTX();
  fp_words* a = static_cast<fp_words*>(d_a);
  return ntt_dev(a, (size_t)1 << log_n, a, log_n, load32(omega), nullptr, nullptr, nullptr, pick_stream(stream));
}
int sg_ntt_fr(uint8_t* a, const uint8_t omega[32], uint32_t log_n) {
  if (!a || !omega || log_n > 28) return fail(SG_ERR_INVALID, "sg_ntt_fr: bad argument");
  return staged_in_place(a, (size_t)32 << log_n, [&](void* d, void* s) { return sg_ntt_fr_dev(d, omega, log_n, s); });
}
// A batch of independent in-place transforms of one size (the 9 lagrange_to_coeff / 9
// coeff_to_extended calls of a proof): batched launches on the caller's stream while the size allows, above that round-robin
// over the two batch streams so that one transform's tail overlaps the next one's head.  divisor == NULL: plain best_fft.
int sg_ntt_fr_batch_dev(void* const* d_a, size_t count, const uint8_t omega[32], const uint8_t* divisor,
                        uint32_t log_n, void* stream) {
  if ((count && !d_a) || !omega || log_n > 28) return fail(SG_ERR_INVALID, "sg_ntt_fr_batch: bad argument");
  LOCKED_CTX();
  for (size_t i = 0; i < count; i++)   // before anything is enqueued, on either path
    if (!d_a[i]) return fail(SG_ERR_INVALID, "sg_ntt_fr_batch: null vector");
  Context& c = *g_ctx;
  const words8 w = load32(omega), dv = divisor ? load32(divisor) : words8{};
  const size_t n = (size_t)1 << log_n;
  const bool need_scratch = ntt_needs_scratch(c.ntt.config(), log_n, true);
  if (ntt_batched(log_n))   // asynchronous on the caller's stream, scratch per stream
    return transforms(reinterpret_cast<fp_words* const*>(d_a), nullptr, 0, count, log_n, w, divisor ? &dv : nullptr, nullptr, nullptr,
                      pick_stream(stream), "ntt batch");
  // larger ones: round robin over the two batch streams, one scratch area per stream, and the host waits for both
  if (need_scratch) {
    hipError_t e = c.scratch.reserve(2 * n * 32);
    if (e != hipSuccess) return hip_fail("ntt scratch", e);
  }
  CHECK_HIP(hipEventRecord(c.ev_in, pick_stream(stream)), "event");
  for (auto& bs : c.bstream) CHECK_HIP(hipStreamWaitEvent(bs, c.ev_in, 0), "stream wait");
  for (size_t i = 0; i < count; i++) {
    const int k = (int)(i & 1);
    fp_words* a = static_cast<fp_words*>(d_a[i]);
    fp_words* scratch = need_scratch ? reinterpret_cast<fp_words*>(c.scratch.p) + (size_t)k * n : nullptr;
    hipError_t e = c.ntt.transform(a, n, a, scratch, log_n, w, divisor ? &dv : nullptr, nullptr, nullptr, c.bstream[k]);
    if (e != hipSuccess) return hip_fail("ntt batch", e);
  }
  for (auto& bs : c.bstream) CHECK_HIP(host_wait_stream(bs), "stream sync");
  return SG_OK;
}

// the same out of place (d_out[i] = transform of d_in[i]; the inputs stay): what `lagrange_to_coeff` of a column that is
// still needed in Lagrange form costs without a device-to-device copy in front of it
int sg_ntt_fr_batch_oop_dev(const void* const* d_in, void* const* d_out, size_t count, const uint8_t omega[32], const uint8_t* divisor,
                            uint32_t log_n, void* stream) {
  if ((count && (!d_in || !d_out)) || !omega || log_n > 28) return fail(SG_ERR_INVALID, "sg_ntt_fr_batch_oop: bad argument");
  const size_t n = (size_t)1 << log_n;
  {
    // the vectors of a launch are transformed side by side: an output that overlaps ANY input, or another output, would be
    // read or written by two workgroups at once -- refused here ("the inputs untouched" is the call's promise)
    auto overlap = [&](const void* a, const void* b) {
      const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
      return x < y + 32 * n && y < x + 32 * n;
    };
    for (size_t i = 0; i < count; i++) {
      if (!d_in[i] || !d_out[i]) return fail(SG_ERR_INVALID, "sg_ntt_fr_batch_oop: null vector");
      for (size_t j = 0; j < count; j++) {
        if (overlap(d_out[i], d_in[j])) return fail(SG_ERR_INVALID, "sg_ntt_fr_batch_oop: an output overlaps an input");
        if (j != i && overlap(d_out[i], d_out[j])) return fail(SG_ERR_INVALID, "sg_ntt_fr_batch_oop: two outputs overlap");
      }
    }
  }
  if (!ntt_batched(log_n)) {   // copy, then in place over the two batch streams
    for (size_t i = 0; i < count; i++)
      CHECK_HIP(hipMemcpyAsync(d_out[i], d_in[i], n * 32, hipMemcpyDeviceToDevice, pick_stream(stream)), "D2D copy");
    return sg_ntt_fr_batch_dev(d_out, count, omega, divisor, log_n, stream);
  }
  LOCKED_CTX();
  const words8 w = load32(omega), dv = divisor ? load32(divisor) : words8{};
  return transforms(reinterpret_cast<fp_words* const*>(d_out), reinterpret_cast<const fp_words* const*>(d_in), n, count, log_n, w,
                    divisor ? &dv : nullptr, nullptr, nullptr, pick_stream(stream), "ntt batch");
}

int sg_intt_fr_dev(void* d_a, const uint8_t omega_inv[32], const uint8_t divisor[32], uint32_t log_n, void* stream) {
  if (!d_a || !omega_inv || !divisor) return fail(SG_ERR_INVALID, "sg_intt_fr: null argument");
  LOCKED_CTX();
  const words8 d = load32(divisor);
  fp_words* a = static_cast<fp_words*>(d_a);
  return ntt_dev(a, (size_t)1 << log_n, a, log_n, load32(omega_inv), &d, nullptr, nullptr, pick_stream(stream));
}
int sg_intt_fr(uint8_t* a, const uint8_t omega_inv[32], const uint8_t divisor[32], uint32_t log_n) {
  if (!a || !omega_inv || !divisor || log_n > 28) return fail(SG_ERR_INVALID, "sg_intt_fr: bad argument");
  return staged_in_place(a, (size_t)32 << log_n, [&](void* d, void* s) { return sg_intt_fr_dev(d, omega_inv, divisor, log_n, s); });
}
int sg_lagrange_to_coeff_dev(void* d_a, uint32_t k, void* stream) {
  if (!d_a || k > 28) return fail(SG_ERR_INVALID, "sg_lagrange_to_coeff: bad argument");
  LOCKED_CTX();
  const DomainConsts* dc;
  TRY(get_consts(k, &dc));
  TRY(sync_own_stream_into(pick_stream(stream)));
  fp_words* a = static_cast<fp_words*>(d_a);
  return ntt_dev(a, (size_t)1 << k, a, k, dc->omega_inv, &dc->n_inv, nullptr, nullptr, pick_stream(stream));
}
int sg_lagrange_to_coeff(uint8_t* a, uint32_t k) {
  if (!a || k > 28) return fail(SG_ERR_INVALID, "sg_lagrange_to_coeff: bad argument");
  return staged_in_place(a, (size_t)32 << k, [&](void* d, void* s) { return sg_lagrange_to_coeff_dev(d, k, s); });
}

int sg_coeff_to_extended_dev(const void* d_coeffs, uint32_t k, uint32_t ext_k, void* d_out, void* stream) {
  if (!d_coeffs || !d_out || ext_k > 28 || k > ext_k || d_coeffs == d_out)
    return fail(SG_ERR_INVALID, "sg_coeff_to_extended: bad argument");
  LOCKED_CTX();
  const DomainConsts* dc;
  TRY(get_consts(ext_k, &dc));
  TRY(sync_own_stream_into(pick_stream(stream)));
  words8 pre[3] = {dc->one, dc->zeta, dc->zeta2};
  return ntt_dev(static_cast<const fp_words*>(d_coeffs), (size_t)1 << k, static_cast<fp_words*>(d_out), ext_k, dc->omega,
                 nullptr, pre, nullptr, pick_stream(stream));
}
// several columns at once
int sg_coeff_to_extended_batch_dev(const void* const* d_coeffs, void* const* d_out, size_t count, uint32_t k, uint32_t ext_k,
                                   void* stream) {
  if ((count && (!d_coeffs || !d_out)) || ext_k > 28 || k > ext_k) return fail(SG_ERR_INVALID, "sg_coeff_to_extended_batch: bad argument");
  for (size_t i = 0; i < count; i++)
    if (!d_coeffs[i] || !d_out[i] || d_coeffs[i] == d_out[i]) return fail(SG_ERR_INVALID, "sg_coeff_to_extended_batch: bad vector");
  LOCKED_CTX();
  const DomainConsts* dc;
  TRY(get_consts(ext_k, &dc));
  hipStream_t s = pick_stream(stream);
  TRY(sync_own_stream_into(s));
  words8 pre[3] = {dc->one, dc->zeta, dc->zeta2};
  return transforms(reinterpret_cast<fp_words* const*>(d_out), reinterpret_cast<const fp_words* const*>(d_coeffs), (size_t)1 << k, count,
                    ext_k, dc->omega, nullptr, pre, nullptr, s, "coeff_to_extended batch");
}
int sg_coeff_to_extended(const uint8_t* coeffs, uint32_t k, uint32_t ext_k, uint8_t* out) {
  if (!coeffs || !out || ext_k > 28 || k > ext_k) return fail(SG_ERR_INVALID, "sg_coeff_to_extended: bad argument");
  LOCKED_CTX();
  TRY(upload(g_ctx->stage_a, coeffs, (size_t)32 << k, g_ctx->stream));
  hipError_t e = g_ctx->stage_b.reserve((size_t)32 << ext_k);
  if (e != hipSuccess) return hip_fail("staging buffer", e);
  TRY(sg_coeff_to_extended_dev(g_ctx->stage_a.p, k, ext_k, g_ctx->stage_b.p, g_ctx->stream));
  return download(out, g_ctx->stage_b.p, (size_t)32 << ext_k, g_ctx->stream);
}
int sg_extended_to_coeff_dev(void* d_ext, uint32_t k, uint32_t ext_k, void* stream) {
  if (!d_ext || ext_k > 28 || k > ext_k) return fail(SG_ERR_INVALID, "sg_extended_to_coeff: bad argument");
  LOCKED_CTX();
  const DomainConsts* dc;
  TRY(get_consts(ext_k, &dc));
  TRY(sync_own_stream_into(pick_stream(stream)));
  // undo the coset: a[i] *= zeta^-(i mod 3) = {1, zeta^2, zeta}; the 2^-ext_k divisor rides along
  words8 post[3] = {dc->n_inv, dc->ninv_zeta2, dc->ninv_zeta};
  fp_words* a = static_cast<fp_words*>(d_ext);
  return ntt_dev(a, (size_t)1 << ext_k, a, ext_k, dc->omega_inv, nullptr, nullptr, post, pick_stream(stream));
}
int sg_extended_to_coeff(uint8_t* ext, uint32_t k, uint32_t ext_k) {
  if (!ext || ext_k > 28 || k > ext_k) return fail(SG_ERR_INVALID, "sg_extended_to_coeff: bad argument");
  return staged_in_place(ext, (size_t)32 << ext_k, [&](void* d, void* s) { return sg_extended_to_coeff_dev(d, k, ext_k, s); });
}

}  // extern "C"

namespace sg {

// ------------------------------------------------------------------ the quotient on d cosets (quotient.h)
int coset_tables_for(uint32_t k, uint32_t ext_k, uint32_t nc, const Context::CosetTables** out) {
  using summa::prover::Fr;
  Context& c = *g_ctx;
  const auto key = std::make_tuple(k, ext_k, nc);
  auto it = c.coset_tables.find(key);
  if (it == c.coset_tables.end()) {
    const DomainConsts *dk, *de;
    TRY(get_consts(k, &dk));
    TRY(get_consts(ext_k, &de));
    Fr zeta, w_ext;
    std::memcpy(zeta.l, &dk->zeta, 32);
    std::memcpy(w_ext.l, &de->omega, 32);
    CosetPlan plan;
    const CosetPlanStatus st = coset_plan(k, nc, zeta, w_ext, &plan);
    if (st == CosetPlanStatus::singular) return fail(SG_ERR_INVALID, "cosets: singular Vandermonde matrix");
    if (st == CosetPlanStatus::inside_domain) return fail(SG_ERR_INVALID, "cosets: a coset inside the domain");
    Context::CosetTables t{};
    words8 inv_shift[MAX_COSETS];
    for (uint32_t b = 0; b < nc; b++) {
      std::memcpy(&t.shift[b], plan.shift[b].l, 32);
      std::memcpy(&inv_shift[b], plan.inv_shift[b].l, 32);
      for (uint32_t tt = 0; tt < nc; tt++) std::memcpy(t.m[tt * MAX_COSETS + b], plan.m[tt * nc + b].l, 32);
    }
    const size_t n = (size_t)1 << k;
    hipError_t e = hipMalloc(&t.fwd, sizeof(fp_words) * n * nc);
    if (e == hipSuccess) e = hipMalloc(&t.inv, sizeof(fp_words) * n * nc);
    if (e == hipSuccess) e = coset_fill_powers(t.fwd, t.shift, nc, k, c.stream);
    if (e == hipSuccess) e = coset_fill_powers(t.inv, inv_shift, nc, k, c.stream);
    if (e == hipSuccess) e = host_wait_stream(c.stream);
    if (e != hipSuccess) {   // (retired, not freed: a fill may still be running)
      retire_device_memory(t.fwd);
      retire_device_memory(t.inv);
      return hip_fail("coset tables", e);
    }
    it = c.coset_tables.emplace(key, t).first;
  }
  *out = &it->second;
  return SG_OK;
}
bool coset_shape_ok(uint32_t k, uint32_t ext_k, uint32_t nc) {
  return k >= 1 && ext_k > k && ext_k <= 28 && nc >= 1 && nc <= MAX_COSETS && nc <= (1u << (ext_k - k));
}

}  // namespace sg

extern "C" {

// size-2^k transforms of `count` vectors in place (forward: omega, no scale; inverse: omega^-1, 2^-k)
static int coset_ntts(fp_words* const* ptrs, size_t count, uint32_t k, bool inverse, hipStream_t s) {
  const DomainConsts* dk;
  TRY(get_consts(k, &dk));
  return transforms(ptrs, nullptr, 0, count, k, inverse ? dk->omega_inv : dk->omega, inverse ? &dk->n_inv : nullptr, nullptr, nullptr, s,
                    "coset ntt batch");
}
int sg_coeff_to_cosets_batch_dev(const void* const* d_coeffs, void* const* d_out, size_t count, uint32_t k, uint32_t ext_k,
                                 uint32_t n_cosets, void* stream) {
  if ((count && (!d_coeffs || !d_out)) || !coset_shape_ok(k, ext_k, n_cosets)) return fail(SG_ERR_INVALID, "sg_coeff_to_cosets_batch: bad argument");
  for (size_t i = 0; i < count; i++)
    if (!d_coeffs[i] || !d_out[i] || d_coeffs[i] == d_out[i]) return fail(SG_ERR_INVALID, "sg_coeff_to_cosets_batch: bad vector");
  LOCKED_CTX();
  const Context::CosetTables* t;
  TRY(coset_tables_for(k, ext_k, n_cosets, &t));
  hipStream_t s = pick_stream(stream);
  TRY(sync_own_stream_into(s));
  const size_t n = (size_t)1 << k;
  if (ntt_batched(k) && !g_sh.param[kRowCosetScalePass].load()) {
    // the coset shift c_b^i rides on the load of the first NTT pass (a table of 2^261-domain words per coset, indexed like the
    // input): no pass over HBM of its own, and every block of every column is a vector of ONE batched launch per pass
    const DomainConsts* dk;
    TRY(get_consts(k, &dk));
    std::vector<fp_words*> blocks;
    std::vector<const fp_words*> srcs, tabs;
    for (size_t j = 0; j < count; j++)
      for (uint32_t b = 0; b < n_cosets; b++) {
        blocks.push_back(static_cast<fp_words*>(d_out[j]) + b * n);
        srcs.push_back(static_cast<const fp_words*>(d_coeffs[j]));
        tabs.push_back(t->fwd + b * n);
      }
    return transforms(blocks.data(), srcs.data(), n, blocks.size(), k, dk->omega, nullptr, nullptr, tabs.data(), s, "coset ntt batch");
  }
  std::vector<fp_words*> blocks;
  for (size_t first = 0; first < count; first += COSET_BATCH_MAX) {
    const uint32_t cnt = (uint32_t)std::min<size_t>(COSET_BATCH_MAX, count - first);
    CosetScaleArgs a{};
    for (uint32_t j = 0; j < cnt; j++) {
      a.in[j] = static_cast<const fp_words*>(d_coeffs[first + j]);
      a.out[j] = static_cast<fp_words*>(d_out[first + j]);
      for (uint32_t b = 0; b < n_cosets; b++) blocks.push_back(a.out[j] + b * n);
    }
    a.table = t->fwd;
    a.log_n = k;
    a.nc = n_cosets;
    hipError_t e = coset_scale(a, cnt, s);
    if (e != hipSuccess) return hip_fail("coset scale", e);
  }
  return coset_ntts(blocks.data(), blocks.size(), k, false, s);
}
int sg_cosets_to_pieces_dev(void* d_values, void* const* d_pieces, uint32_t k, uint32_t ext_k, uint32_t n_cosets, void* stream) {
  if (!d_values || !d_pieces || !coset_shape_ok(k, ext_k, n_cosets)) return fail(SG_ERR_INVALID, "sg_cosets_to_pieces: bad argument");
  for (uint32_t t = 0; t < n_cosets; t++)
    if (!d_pieces[t]) return fail(SG_ERR_INVALID, "sg_cosets_to_pieces: null piece");
  // (refused before the inverse transforms below run in place: a refused call writes nothing)
  const size_t n = (size_t)1 << k;
  for (uint32_t i = 0; i < n_cosets; i++) {
    const uint8_t* lo = static_cast<const uint8_t*>(d_pieces[i]);
    const uint8_t* vb = static_cast<const uint8_t*>(d_values);
    if (lo < vb + 32 * n * n_cosets && vb < lo + 32 * n) return fail(SG_ERR_INVALID, "sg_cosets_to_pieces: the pieces may not overlap the values");
  }
  LOCKED_CTX();
  const Context::CosetTables* t;
  TRY(coset_tables_for(k, ext_k, n_cosets, &t));
  hipStream_t s = pick_stream(stream);
  TRY(sync_own_stream_into(s));
  fp_words* v = static_cast<fp_words*>(d_values);
  std::vector<fp_words*> blocks;
  for (uint32_t b = 0; b < n_cosets; b++) blocks.push_back(v + b * n);
  TRY(coset_ntts(blocks.data(), blocks.size(), k, true, s));
  CosetCombineArgs a{};
  a.raw = v;
  for (uint32_t i = 0; i < n_cosets; i++) a.pieces[i] = static_cast<fp_words*>(d_pieces[i]);
  a.table_inv = t->inv;
  a.log_n = k;
  a.nc = n_cosets;
  std::memcpy(a.m, t->m, sizeof(a.m));
  hipError_t e = coset_combine(a, s);
  if (e != hipSuccess) return hip_fail("coset combine", e);
  return SG_OK;
}

static int t_eval_table(uint32_t k, uint32_t ext_k, const fp_words** out) {
  Context& c = *g_ctx;
  uint64_t key = ((uint64_t)k << 32) | ext_k;
  auto it = c.t_evals.find(key);
  if (it == c.t_evals.end()) {
    const DomainConsts* dc;
    TRY(get_consts(ext_k, &dc));
    uint32_t cnt = 1u << (ext_k - k);
    fp_words* d = nullptr;
    CHECK_HIP(hipMalloc(&d, sizeof(fp_words) * cnt), "t_evaluations");
    t_eval_launch(k, ext_k, dc->omega, d, c.stream);
    CHECK_HIP(host_wait_stream(c.stream), "t_evaluations");
    it = c.t_evals.emplace(key, d).first;
  }
  *out = it->second;
  return SG_OK;
}
int sg_divide_by_vanishing_poly_dev(void* d_ext, uint32_t k, uint32_t ext_k, void* stream) {
  if (!d_ext || ext_k > 28 || k > ext_k) return fail(SG_ERR_INVALID, "sg_divide_by_vanishing_poly: bad argument");
  LOCKED_CTX();
  const fp_words* tab;
  TRY(t_eval_table(k, ext_k, &tab));
  hipError_t e = ntt_scale_periodic(static_cast<fp_words*>(d_ext), tab, 1u << (ext_k - k), (size_t)1 << ext_k,
                                    pick_stream(stream));
  if (e != hipSuccess) return hip_fail("divide_by_vanishing_poly", e);
  return SG_OK;
}
int sg_divide_by_vanishing_poly(uint8_t* ext, uint32_t k, uint32_t ext_k) {
  if (!ext || ext_k > 28 || k > ext_k) return fail(SG_ERR_INVALID, "sg_divide_by_vanishing_poly: bad argument");
  return staged_in_place(ext, (size_t)32 << ext_k, [&](void* d, void* s) { return sg_divide_by_vanishing_poly_dev(d, k, ext_k, s); });
}

int sg_domain_constant(uint32_t k, int which, uint8_t out[32]) {
  if (!out || k > 28 || which < 0 || which > 3) return fail(SG_ERR_INVALID, "sg_domain_constant: bad argument");
  LOCKED_CTX();
  const DomainConsts* dc;
  TRY(get_consts(k, &dc));
  const words8* src = which == 0 ? &dc->omega : which == 1 ? &dc->omega_inv : which == 2 ? &dc->n_inv : &dc->zeta;
  std::memcpy(out, src, 32);
  return SG_OK;
}

int sg_time_ntt_dev(void* d_a, uint32_t log_n, int reps, float* ms_out) {
  if (!d_a || !ms_out || reps < 1 || log_n > 28) return fail(SG_ERR_INVALID, "sg_time_ntt_dev: bad argument");
  LOCKED_CTX();
  const DomainConsts* dc;
  TRY(get_consts(log_n, &dc));
  fp_words* a = static_cast<fp_words*>(d_a);
  hipStream_t s = g_ctx->stream;
  TRY(ntt_dev(a, (size_t)1 << log_n, a, log_n, dc->omega, nullptr, nullptr, nullptr, s));  // warm plan + caches
  hipEvent_t e0, e1;
  CHECK_HIP(hipEventCreate(&e0), "event");
  CHECK_HIP(hipEventCreate(&e1), "event");
  CHECK_HIP(hipEventRecord(e0, s), "event");
  for (int r = 0; r < reps; r++) TRY(ntt_dev(a, (size_t)1 << log_n, a, log_n, dc->omega, nullptr, nullptr, nullptr, s));
  CHECK_HIP(hipEventRecord(e1, s), "event");
  CHECK_HIP(host_wait_event(e1), "event");
  float ms = 0;
  CHECK_HIP(hipEventElapsedTime(&ms, e0, e1), "event");
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *ms_out = ms / reps;
  return SG_OK;
}

}  // extern "C"
