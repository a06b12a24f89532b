// C ABI, quotient family: sg_quotient_*, the gate-program cache and sg_gates_program_* (summa_gpu.hip holds the core; the
// circuit's keygen and witness entry points are abi_mst.hip's).
#include "abi_internal.h"

using namespace sg;
namespace {

bool any_null(const void* const* p, size_t n) { return std::find(p, p + n, nullptr) != p + n; }
const fp_words* words(const void* p) { return static_cast<const fp_words*>(p); }
// the permutation argument's shape: `ncols` columns in `nsets` chunks of `chunk_len` (the last one may be short)
bool perm_shape_ok(uint32_t nsets, uint32_t ncols, uint32_t chunk_len, uint32_t k, uint32_t last_rotation_abs) {
  return nsets != 0 && nsets <= QUOT_MAX_SETS && ncols != 0 && ncols <= QUOT_MAX_COLS && chunk_len != 0 && chunk_len <= 11 &&
         (ncols + chunk_len - 1) / chunk_len == nsets && last_rotation_abs < (1u << k);
}
// Everything of a permutation block but `values` (the caller has zeroed `a` and checked shape and pointers).  cosets = 0: rows
// of the extended domain; cosets = c: every block is the 2^k domain shifted by c_b = zeta omega_ext^b.
int fill_perm_args(QuotPermArgs& a, const void* const* d_z, uint32_t nsets, const void* const* d_cols, const void* const* d_sigma,
                   uint32_t ncols, uint32_t chunk_len, const void* d_l0, const void* d_l_last, const void* d_l_active,
                   const uint8_t beta[32], const uint8_t gamma[32], const uint8_t y[32], uint32_t k, uint32_t ext_k,
                   uint32_t last_rotation_abs, uint32_t cosets, hipStream_t s) {
  for (uint32_t i = 0; i < nsets; i++) a.z[i] = words(d_z[i]);
  for (uint32_t i = 0; i < ncols; i++) {
    a.cols[i] = words(d_cols[i]);
    a.sigma[i] = words(d_sigma[i]);
  }
  a.l0 = words(d_l0); a.l_last = words(d_l_last); a.l_active = words(d_l_active);
  a.nsets = nsets; a.ncols = ncols; a.chunk_len = chunk_len; a.k = k; a.ext_k = cosets ? k : ext_k;
  a.cosets = cosets;
  a.last_rot_abs = last_rotation_abs;
  const DomainConsts *dk, *dw;   // dw: the domain whose omega takes a row to the next
  TRY(get_consts(k, &dk));
  TRY(get_consts(cosets ? k : ext_k, &dw));
  std::memcpy(a.beta, beta, 32); std::memcpy(a.gamma, gamma, 32); std::memcpy(a.y, y, 32);
  std::memcpy(a.delta, &DELTA_M, 32); std::memcpy(a.zeta, &dk->zeta, 32); std::memcpy(a.omega_ext, &dw->omega, 32);
  if (cosets) {
    const Context::CosetTables* t;
    TRY(coset_tables_for(k, ext_k, cosets, &t));
    for (uint32_t b = 0; b < cosets; b++) std::memcpy(a.shift[b], &t->shift[b], 32);
  }
  fp_words* pw = nullptr;
  hipError_t e = g_ctx->ntt.local_twiddles(dw->omega, 9, s, &pw);   // omega^t, t < 256
  if (e != hipSuccess) return hip_fail("quotient twiddles", e);
  a.pow_lo = pw;
  return SG_OK;
}
// the same of a lookup block (d_input: the input expression's values, or NULL where the kernel evaluates it on the way)
void fill_lookup_args(QuotLookupArgs& a, const void* d_z, const void* d_permuted_input, const void* d_permuted_table, const void* d_input,
                      const void* d_table, const void* d_l0, const void* d_l_last, const void* d_l_active, const uint8_t beta[32],
                      const uint8_t gamma[32], const uint8_t y[32], uint32_t k, uint32_t ext_k, uint32_t cosets) {
  a.z = words(d_z); a.permuted_input = words(d_permuted_input); a.permuted_table = words(d_permuted_table);
  a.input = words(d_input); a.table = words(d_table);
  a.l0 = words(d_l0); a.l_last = words(d_l_last); a.l_active = words(d_l_active);
  a.k = k; a.ext_k = cosets ? k : ext_k;
  a.cosets = cosets;
  std::memcpy(a.beta, beta, 32); std::memcpy(a.gamma, gamma, 32); std::memcpy(a.y, y, 32);
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------ quotient numerator (evaluate_h, generic parts)
// cosets = 0: the whole extended domain (row i = zeta omega_ext^i); cosets = c: coset-major arrays, block b = the 2^k rows
// of the coset zeta omega_ext^b H
static int quotient_permutation_impl(void* d_values, const void* const* d_z, uint32_t nsets, const void* const* d_cols,
                                     const void* const* d_sigma, uint32_t ncols, uint32_t chunk_len, const void* d_l0,
                                     const void* d_l_last, const void* d_l_active, const uint8_t beta[32],
                                     const uint8_t gamma[32], const uint8_t y[32], uint32_t k, uint32_t ext_k,
                                     uint32_t last_rotation_abs, uint32_t cosets, void* stream) {
  if (!d_values || !d_z || !d_cols || !d_sigma || !d_l0 || !d_l_last || !d_l_active || !beta || !gamma || !y)
    return fail(SG_ERR_INVALID, "sg_quotient_permutation: null argument");
  if (k == 0 || ext_k < k || ext_k > 28 || !perm_shape_ok(nsets, ncols, chunk_len, k, last_rotation_abs))
    return fail(SG_ERR_INVALID, "sg_quotient_permutation: bad shape");
  LOCKED_CTX();
  if (any_null(d_z, nsets)) return fail(SG_ERR_INVALID, "sg_quotient_permutation: null z");
  if (any_null(d_cols, ncols) || any_null(d_sigma, ncols)) return fail(SG_ERR_INVALID, "sg_quotient_permutation: null column");
  QuotPermArgs a;
  std::memset(&a, 0, sizeof(a));
  a.values = static_cast<fp_words*>(d_values);
  hipStream_t s = pick_stream(stream);
  TRY(fill_perm_args(a, d_z, nsets, d_cols, d_sigma, ncols, chunk_len, d_l0, d_l_last, d_l_active, beta, gamma, y, k, ext_k,
                     last_rotation_abs, cosets, s));
  hipError_t e = quotient_permutation(a, s);
  if (e != hipSuccess) return hip_fail("quotient_permutation", e);
  return SG_OK;
}
int sg_quotient_permutation_dev(void* d_values, const void* const* d_z, uint32_t nsets, const void* const* d_cols,
                                const void* const* d_sigma, uint32_t ncols, uint32_t chunk_len, const void* d_l0,
                                const void* d_l_last, const void* d_l_active, const uint8_t beta[32],
                                const uint8_t gamma[32], const uint8_t y[32], uint32_t k, uint32_t ext_k,
                                uint32_t last_rotation_abs, void* stream) {
  return quotient_permutation_impl(d_values, d_z, nsets, d_cols, d_sigma, ncols, chunk_len, d_l0, d_l_last, d_l_active, beta, gamma, y, k,
                                   ext_k, last_rotation_abs, 0, stream);
}
int sg_quotient_permutation_cosets_dev(void* d_values, const void* const* d_z, uint32_t nsets, const void* const* d_cols,
                                       const void* const* d_sigma, uint32_t ncols, uint32_t chunk_len, const void* d_l0,
                                       const void* d_l_last, const void* d_l_active, const uint8_t beta[32],
                                       const uint8_t gamma[32], const uint8_t y[32], uint32_t k, uint32_t ext_k,
                                       uint32_t n_cosets, uint32_t last_rotation_abs, void* stream) {
  if (!coset_shape_ok(k, ext_k, n_cosets)) return fail(SG_ERR_INVALID, "sg_quotient_permutation_cosets: bad shape");
  return quotient_permutation_impl(d_values, d_z, nsets, d_cols, d_sigma, ncols, chunk_len, d_l0, d_l_last, d_l_active, beta, gamma, y, k,
                                   ext_k, last_rotation_abs, n_cosets, stream);
}
static int quotient_lookup_impl(void* d_values, const void* d_z, const void* d_permuted_input, const void* d_permuted_table,
                                const void* d_input, const void* d_table, const void* d_l0, const void* d_l_last,
                                const void* d_l_active, const uint8_t beta[32], const uint8_t gamma[32], const uint8_t y[32],
                                uint32_t k, uint32_t ext_k, uint32_t cosets, void* stream) {
  if (!d_values || !d_z || !d_permuted_input || !d_permuted_table || !d_input || !d_table || !d_l0 || !d_l_last ||
      !d_l_active || !beta || !gamma || !y)
    return fail(SG_ERR_INVALID, "sg_quotient_lookup: null argument");
  if (k == 0 || ext_k < k || ext_k > 28) return fail(SG_ERR_INVALID, "sg_quotient_lookup: bad shape");
  LOCKED_CTX();
  QuotLookupArgs a;
  a.values = static_cast<fp_words*>(d_values);
  fill_lookup_args(a, d_z, d_permuted_input, d_permuted_table, d_input, d_table, d_l0, d_l_last, d_l_active, beta, gamma, y, k, ext_k, cosets);
  hipError_t e = quotient_lookup(a, pick_stream(stream));
  if (e != hipSuccess) return hip_fail("quotient_lookup", e);
  return SG_OK;
}
int sg_quotient_lookup_dev(void* d_values, const void* d_z, const void* d_permuted_input, const void* d_permuted_table,
                           const void* d_input, const void* d_table, const void* d_l0, const void* d_l_last,
                           const void* d_l_active, const uint8_t beta[32], const uint8_t gamma[32], const uint8_t y[32],
                           uint32_t k, uint32_t ext_k, void* stream) {
  return quotient_lookup_impl(d_values, d_z, d_permuted_input, d_permuted_table, d_input, d_table, d_l0, d_l_last, d_l_active, beta, gamma,
                              y, k, ext_k, 0, stream);
}
int sg_quotient_lookup_cosets_dev(void* d_values, const void* d_z, const void* d_permuted_input, const void* d_permuted_table,
                                  const void* d_input, const void* d_table, const void* d_l0, const void* d_l_last,
                                  const void* d_l_active, const uint8_t beta[32], const uint8_t gamma[32], const uint8_t y[32],
                                  uint32_t k, uint32_t n_cosets, void* stream) {
  if (n_cosets == 0 || n_cosets > QUOT_MAX_COSETS) return fail(SG_ERR_INVALID, "sg_quotient_lookup_cosets: bad shape");
  return quotient_lookup_impl(d_values, d_z, d_permuted_input, d_permuted_table, d_input, d_table, d_l0, d_l_last, d_l_active, beta, gamma,
                              y, k, k, n_cosets, stream);
}

// the lowered program of a graph, from the lane's cache (compiled on first sight), with its constant table refreshed for this
// call.  The caller holds the lane.
static int gate_program_for(const sg_graph* graph, uint32_t n_fixed, uint32_t n_advice, uint32_t n_instance, const uint8_t* challenges,
                            uint32_t n_challenges, const uint8_t beta[32], const uint8_t gamma[32], const uint8_t theta[32],
                            const uint8_t y[32], GateProgram** out) {
  const std::string err = g_ctx->gate_programs.lookup_or_compile(*graph, n_fixed, n_advice, n_instance, n_challenges, gates_env().lowering, out);
  if (!err.empty()) return fail(SG_ERR_INVALID, ("sg_quotient_gates: " + err).c_str());
  if ((graph->n_constants && !graph->constants)) return fail(SG_ERR_INVALID, "sg_quotient_gates: null constants");
  gate_const_table(*graph, challenges, n_challenges, beta, gamma, theta, y, &(*out)->const_words);
  return SG_OK;
}
static int quotient_gates_impl(void* d_values, const sg_graph* graph, const void* const* d_fixed, uint32_t n_fixed,
                               const void* const* d_advice, uint32_t n_advice, const void* const* d_instance,
                               uint32_t n_instance, const uint8_t* challenges, uint32_t n_challenges,
                               const uint8_t beta[32], const uint8_t gamma[32], const uint8_t theta[32], const uint8_t y[32],
                               uint32_t k, uint32_t ext_k, uint32_t cosets, void* stream) {
  if (!d_values || !graph || !beta || !gamma || !theta || !y || (n_fixed && !d_fixed) || (n_advice && !d_advice) ||
      (n_instance && !d_instance) || (n_challenges && !challenges))
    return fail(SG_ERR_INVALID, "sg_quotient_gates: null argument");
  if (k == 0 || ext_k < k || ext_k > 28) return fail(SG_ERR_INVALID, "sg_quotient_gates: bad shape");
  LOCKED_CTX();
  GateProgram* prog_p = nullptr;
  TRY(gate_program_for(graph, n_fixed, n_advice, n_instance, challenges, n_challenges, beta, gamma, theta, y, &prog_p));
  GateProgram& prog = *prog_p;
  static_assert(GATES_MAX_SLOTS == 64, "the message below names the limit");
  if (prog.n_slots > GATES_MAX_SLOTS) return fail(SG_ERR_INVALID, "sg_quotient_gates: more than 64 simultaneously live values");
  std::vector<const void*> cols;
  for (uint32_t i = 0; i < n_fixed; i++) cols.push_back(d_fixed[i]);
  for (uint32_t i = 0; i < n_advice; i++) cols.push_back(d_advice[i]);
  for (uint32_t i = 0; i < n_instance; i++) cols.push_back(d_instance[i]);
  if (any_null(cols.data(), cols.size())) return fail(SG_ERR_INVALID, "sg_quotient_gates: null column");
  hipStream_t s = pick_stream(stream);
  {
    hipError_t ev = hipSuccess;
    if (gates_run_by_value(prog, cols.data(), static_cast<fp_words*>(d_values), k, ext_k, s, cosets, &ev)) {
      if (ev != hipSuccess) return hip_fail("quotient_gates", ev);
      return SG_OK;
    }
  }
  // program + column pointers + constants travel as one small blob.  Ring of page-locked host / device buffer pairs, each
  // guarded by an event recorded after the kernel that reads it: the call is asynchronous (no host wait unless the ring
  // has wrapped onto a launch that is still running)
  const size_t bytes = gates_blob(prog, cols.data(), &g_ctx->gate_blob_host);
  // (never small: the ring rotates, and a slot sized by a small program would be re-allocated -- two allocations, 0.25 ms
  // with the device idle -- the first time the big program of the same prover comes round to it)
  Context::BlobSlot* slot_p = nullptr;
  hipError_t e = ring_slot(g_ctx->blob_ring, bytes, std::max<size_t>(bytes + bytes / 2 + 256, (size_t)256 << 10), &slot_p);
  Context::BlobSlot& slot = *slot_p;
  if (e == hipSuccess) {
    std::memcpy(slot.host, g_ctx->gate_blob_host.data(), bytes);
    e = hipMemcpyAsync(slot.dev, slot.host, bytes, hipMemcpyHostToDevice, s);
  }
  if (e == hipSuccess) e = gates_run(prog, slot.dev, static_cast<fp_words*>(d_values), k, ext_k, s, cosets);
  if (e == hipSuccess) e = hipEventRecord(slot.ev, s);
  if (e != hipSuccess) return hip_fail("quotient_gates", e);
  return SG_OK;
}
int sg_quotient_gates_dev(void* d_values, const sg_graph* graph, const void* const* d_fixed, uint32_t n_fixed,
                          const void* const* d_advice, uint32_t n_advice, const void* const* d_instance,
                          uint32_t n_instance, const uint8_t* challenges, uint32_t n_challenges,
                          const uint8_t beta[32], const uint8_t gamma[32], const uint8_t theta[32], const uint8_t y[32],
                          uint32_t k, uint32_t ext_k, void* stream) {
  return quotient_gates_impl(d_values, graph, d_fixed, n_fixed, d_advice, n_advice, d_instance, n_instance, challenges, n_challenges, beta,
                             gamma, theta, y, k, ext_k, 0, stream);
}
int sg_quotient_gates_cosets_dev(void* d_values, const sg_graph* graph, const void* const* d_fixed, uint32_t n_fixed,
                                 const void* const* d_advice, uint32_t n_advice, const void* const* d_instance,
                                 uint32_t n_instance, const uint8_t* challenges, uint32_t n_challenges,
                                 const uint8_t beta[32], const uint8_t gamma[32], const uint8_t theta[32], const uint8_t y[32],
                                 uint32_t k, uint32_t n_cosets, void* stream) {
  if (n_cosets == 0 || n_cosets > QUOT_MAX_COSETS) return fail(SG_ERR_INVALID, "sg_quotient_gates_cosets: bad shape");
  return quotient_gates_impl(d_values, graph, d_fixed, n_fixed, d_advice, n_advice, d_instance, n_instance, challenges, n_challenges, beta,
                             gamma, theta, y, k, k, n_cosets, stream);
}
// halo2's evaluate_h in one call: values <- gates, then the permutation argument, then the lookup argument (input expression
// evaluated on the way).  One fused kernel when the two programs are known ahead of time (csrc/numerator.hip), otherwise the
// separate kernels one after the other -- the same words either way.
int sg_quotient_numerator_cosets_dev(void* d_values, const sg_graph* gates, const sg_graph* lookup_input, const void* const* d_fixed,
                                     uint32_t n_fixed, const void* const* d_advice, uint32_t n_advice, const void* const* d_instance,
                                     uint32_t n_instance, const uint8_t* challenges, uint32_t n_challenges, const void* const* d_z,
                                     uint32_t nsets, const void* const* d_perm_cols, const void* const* d_sigma, uint32_t ncols,
                                     uint32_t chunk_len, const void* d_l0, const void* d_l_last, const void* d_l_active,
                                     const void* d_lookup_z, const void* d_permuted_input, const void* d_permuted_table,
                                     const void* d_table, void* d_input_work, const uint8_t beta[32], const uint8_t gamma[32],
                                     const uint8_t theta[32], const uint8_t y[32], uint32_t k, uint32_t ext_k, uint32_t n_cosets,
                                     uint32_t last_rotation_abs, void* stream) {
  if (!d_values || !gates || !lookup_input || !d_z || !d_perm_cols || !d_sigma || !d_l0 || !d_l_last || !d_l_active || !d_lookup_z ||
      !d_permuted_input || !d_permuted_table || !d_table || !beta || !gamma || !theta || !y || (n_fixed && !d_fixed) ||
      (n_advice && !d_advice) || (n_instance && !d_instance) || (n_challenges && !challenges))
    return fail(SG_ERR_INVALID, "sg_quotient_numerator_cosets: null argument");
  if (!coset_shape_ok(k, ext_k, n_cosets) || n_cosets > QUOT_MAX_COSETS) return fail(SG_ERR_INVALID, "sg_quotient_numerator_cosets: bad shape");
  // every precondition of either path is checked here, before one is chosen: a call both paths would refuse is refused
  // the same way, and nothing is launched for it
  if (!perm_shape_ok(nsets, ncols, chunk_len, k, last_rotation_abs))
    return fail(SG_ERR_INVALID, "sg_quotient_numerator_cosets: bad permutation shape");
  if (any_null(d_fixed, n_fixed) || any_null(d_advice, n_advice) || any_null(d_instance, n_instance))
    return fail(SG_ERR_INVALID, "sg_quotient_numerator_cosets: null column");
  if (any_null(d_z, nsets)) return fail(SG_ERR_INVALID, "sg_quotient_numerator_cosets: null z");
  if (any_null(d_perm_cols, ncols) || any_null(d_sigma, ncols))
    return fail(SG_ERR_INVALID, "sg_quotient_numerator_cosets: null permutation column");
  bool fused = false;
  if (g_sh.param[kRowFusedNumerator].load() && n_fixed + n_advice + n_instance <= NUM_MAX_COLS) {
    LOCKED_CTX();
    g_ctx->gate_programs.reserve(2);   // neither look-up below may evict the other's program
    GateProgram *pg = nullptr, *pi = nullptr;
    const uint8_t none[32] = {0};
    TRY(gate_program_for(gates, n_fixed, n_advice, n_instance, challenges, n_challenges, beta, gamma, theta, y, &pg));
    TRY(gate_program_for(lookup_input, n_fixed, n_advice, n_instance, none, 0, beta, gamma, theta, y, &pi));
    // (two structurally identical programs are one cache entry: its constant table holds the second call's constants only)
    if (pg != pi && numerator_fused_available(*pg, *pi)) {
      NumeratorArgs a;
      std::memset(&a, 0, sizeof a);
      a.values = static_cast<fp_words*>(d_values);
      uint32_t c = 0;
      for (uint32_t i = 0; i < n_fixed; i++) a.cols[c++] = static_cast<const fp_words*>(d_fixed[i]);
      for (uint32_t i = 0; i < n_advice; i++) a.cols[c++] = static_cast<const fp_words*>(d_advice[i]);
      for (uint32_t i = 0; i < n_instance; i++) a.cols[c++] = static_cast<const fp_words*>(d_instance[i]);
      hipStream_t s = pick_stream(stream);
      TRY(fill_perm_args(a.perm, d_z, nsets, d_perm_cols, d_sigma, ncols, chunk_len, d_l0, d_l_last, d_l_active, beta, gamma, y, k, ext_k,
                         last_rotation_abs, n_cosets, s));
      fill_lookup_args(a.look, d_lookup_z, d_permuted_input, d_permuted_table, nullptr, d_table, d_l0, d_l_last, d_l_active, beta, gamma, y, k,
                       ext_k, n_cosets);
      hipError_t e = numerator_fused(*pg, *pi, a, s);
      if (e != hipSuccess) return hip_fail("quotient numerator", e);
      fused = true;
    }
  }
  if (fused) return SG_OK;
  // any other pair of programs: the blocks one after the other over `values` (zeroed: a fresh numerator)
  const size_t rows = (size_t)n_cosets << k;
  void* input_work = d_input_work;
  if (!input_work) {
    LOCKED_CTX();
    uint8_t* w = nullptr;
    hipError_t e = scratch_for(pick_stream(stream), 8, rows * 32, &w);
    if (e != hipSuccess) return hip_fail("numerator work space", e);
    input_work = w;
  }
  {
    LOCKED_CTX();
    CHECK_HIP(hipMemsetAsync(d_values, 0, rows * 32, pick_stream(stream)), "memset");
  }
  const uint8_t none[32] = {0};
  TRY(sg_quotient_gates_cosets_dev(d_values, gates, d_fixed, n_fixed, d_advice, n_advice, d_instance, n_instance, challenges, n_challenges, beta,
                                   gamma, theta, y, k, n_cosets, stream));
  TRY(sg_quotient_permutation_cosets_dev(d_values, d_z, nsets, d_perm_cols, d_sigma, ncols, chunk_len, d_l0, d_l_last, d_l_active, beta, gamma, y,
                                         k, ext_k, n_cosets, last_rotation_abs, stream));
  TRY(sg_quotient_gates_cosets_dev(input_work, lookup_input, d_fixed, n_fixed, d_advice, n_advice, d_instance, n_instance, none, 0, beta, gamma,
                                   theta, y, k, n_cosets, stream));
  return sg_quotient_lookup_cosets_dev(d_values, d_lookup_z, d_permuted_input, d_permuted_table, input_work, d_table, d_l0, d_l_last, d_l_active,
                                       beta, gamma, y, k, n_cosets, stream);
}

// the lowered program itself, for tooling (tools/gen_gates_programs.py writes the ahead-of-time instantiations of the reference
// circuit's programs from it) and tests.  Host-only: no device is touched, no cache either.
static int lowered_program(const char* who, const sg_graph* graph, uint32_t n_fixed, uint32_t n_advice, uint32_t n_instance,
                           uint32_t n_challenges, GateProgram* prog) {
  const std::string err = compile_gates(*graph, n_fixed, n_advice, n_instance, n_challenges, gates_env().lowering, prog);
  if (!err.empty()) return fail(SG_ERR_INVALID, (std::string(who) + ": " + err).c_str());
  return SG_OK;
}
// how the interpreter would run a program: instructions and simultaneously live values (LDS slots per row; 8 or fewer keep
// two workgroups of 256 rows per CU)
int sg_gates_program_info(const sg_graph* graph, uint32_t n_fixed, uint32_t n_advice, uint32_t n_instance, uint32_t n_challenges,
                          uint32_t* n_ops_out, uint32_t* n_slots_out) {
  if (!graph || !n_ops_out || !n_slots_out) return fail(SG_ERR_INVALID, "sg_gates_program_info: null argument");
  GateProgram prog;
  TRY(lowered_program("sg_gates_program_info", graph, n_fixed, n_advice, n_instance, n_challenges, &prog));
  *n_ops_out = (uint32_t)prog.ops.size();
  *n_slots_out = prog.n_slots;
  return SG_OK;
}
// words_out = [n_slots, result_kind, result_index, n_ops, then (w0, dst, a, b) per instruction].  *n_words_out is the size
// needed; nothing is written beyond cap_words.
int sg_gates_program_words(const sg_graph* graph, uint32_t n_fixed, uint32_t n_advice, uint32_t n_instance, uint32_t n_challenges,
                           uint32_t* words_out, uint32_t cap_words, uint32_t* n_words_out) {
  if (!graph || !n_words_out || (cap_words && !words_out)) return fail(SG_ERR_INVALID, "sg_gates_program_words: null argument");
  GateProgram prog;
  TRY(lowered_program("sg_gates_program_words", graph, n_fixed, n_advice, n_instance, n_challenges, &prog));
  std::vector<uint32_t> w = {prog.n_slots, prog.result_kind, prog.result_index, (uint32_t)prog.ops.size()};
  for (const GateOp& o : prog.ops) { w.push_back(o.w0); w.push_back(o.dst); w.push_back(o.a); w.push_back(o.b); }
  *n_words_out = (uint32_t)w.size();
  if (cap_words >= w.size()) std::memcpy(words_out, w.data(), 4 * w.size());
  return SG_OK;
}

}  // extern "C"
