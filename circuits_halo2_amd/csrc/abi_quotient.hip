// C ABI, quotient family: sg_quotient_*, the gate-program cache, sg_gates_program_*, and the circuit's keygen and witness
// entry points (summa_gpu.hip holds the core).
#include "abi_internal.h"
#include "mst_entries.h"
#include "mst_update_plan.h"

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

// ------------------------------------------------------------------ keygen's circuit side
// What `keygen_vk` / `keygen_pk` need of `MstInclusionCircuit::synthesize` over 2^k rows [REF zk_prover/src/circuits/
// merkle_sum_tree.rs:228-520 replayed over halo2's SimpleFloorPlanner: include/summa_circuit.hpp]: the 11 fixed columns (round
// constants, range table, compressed selectors, constants) and the 6 permutation columns sigma_c[row] = the label delta^c' omega^row'
// of the cell (c, row) is copy-constrained to.  Host only (no device needed); Montgomery words, column-major.
int sg_mst_inclusion_keygen_columns(uint32_t k, uint32_t levels, uint32_t n_currencies, uint32_t n_bytes, uint8_t* fixed_out,
                                    uint8_t* sigma_out, uint32_t* rows_used_out) {
  if (!fixed_out || !sigma_out || k < 4 || k > 25 || levels == 0 || levels > 48 || n_currencies == 0 || n_currencies > 16 || n_bytes == 0 ||
      n_bytes > 31)
    return fail(SG_ERR_INVALID, "sg_mst_inclusion_keygen_columns: bad argument");
  try {
    using summa::prover::Fr;
    const summa::circuit::FloorPlan fp(k, levels, n_currencies, n_bytes);
    const size_t n = (size_t)1 << k;
    if (fp.rows_used + summa::circuit::BLINDING_FACTORS + 1 > n) return fail(SG_ERR_INVALID, "sg_mst_inclusion_keygen_columns: not enough rows");
    static const uint8_t root_2_28[32] = {0x03, 0xdd, 0xb9, 0xf5, 0x16, 0x6d, 0x18, 0xb7, 0x98, 0x86, 0x5e, 0xa9, 0x3d, 0xd3, 0x1f, 0x74,
                                          0x32, 0x15, 0xcf, 0x6d, 0xd3, 0x93, 0x29, 0xc8, 0xd3, 0x4f, 0x1e, 0xd9, 0x60, 0xc3, 0x7c, 0x9c};
    Fr omega = Fr::from_be_bytes_reduced(root_2_28);
    for (uint32_t i = k; i < 28; i++) omega = omega * omega;
    for (uint32_t c = 0; c < summa::circuit::NUM_FIXED; c++) std::memcpy(fixed_out + 32 * n * c, fp.fixed[c].data(), 32 * n);
    const auto sigma = fp.sigma(omega);
    for (uint32_t c = 0; c < summa::circuit::NUM_PERM; c++) std::memcpy(sigma_out + 32 * n * c, sigma[c].data(), 32 * n);
    if (rows_used_out) *rows_used_out = fp.rows_used;
  } catch (const std::exception& ex) {
    return fail(SG_ERR_INVALID, (std::string("sg_mst_inclusion_keygen_columns: ") + ex.what()).c_str());
  }
  return SG_OK;
}

// ------------------------------------------------------------------ witness side (Merkle sum tree)
int sg_mst_leaves_dev(const void* d_usernames, const void* d_balances, size_t n, uint32_t n_currencies,
                      void* d_hashes, void* stream) {
  if (n && (!d_usernames || !d_balances || !d_hashes)) return fail(SG_ERR_INVALID, "sg_mst_leaves: null argument");
  if (n_currencies == 0 || n_currencies > 64 || n >= (1ull << 32)) return fail(SG_ERR_INVALID, "sg_mst_leaves: bad size");
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  hipError_t e = g_ctx->witness.init(g_ctx->stream);
  if (e == hipSuccess)
    e = g_ctx->witness.leaves(static_cast<const fp_words*>(d_usernames), static_cast<const fp_words*>(d_balances), n,
                              n_currencies, static_cast<fp_words*>(d_hashes), s);
  if (e != hipSuccess) return hip_fail("mst leaves", e);
  return SG_OK;
}
int sg_mst_level_dev(const void* d_child_hashes, const void* d_child_balances, size_t n_parents, uint32_t n_currencies,
                     void* d_hashes, void* d_balances, void* stream) {
  if (n_parents && (!d_child_hashes || !d_child_balances || !d_hashes || !d_balances))
    return fail(SG_ERR_INVALID, "sg_mst_level: null argument");
  if (n_currencies == 0 || n_currencies > 64 || n_parents >= (1ull << 31)) return fail(SG_ERR_INVALID, "sg_mst_level: bad size");
  LOCKED_CTX();
  hipError_t e = g_ctx->witness.init(g_ctx->stream);
  if (e == hipSuccess)
    e = g_ctx->witness.level(static_cast<const fp_words*>(d_child_hashes), static_cast<const fp_words*>(d_child_balances),
                             n_parents, n_currencies, static_cast<fp_words*>(d_hashes),
                             static_cast<fp_words*>(d_balances), pick_stream(stream));
  if (e != hipSuccess) return hip_fail("mst level", e);
  return SG_OK;
}
// whole tree: node arrays are level-major (2^depth leaves, then 2^(depth-1) parents, ..., the root)
int sg_mst_build_dev(const void* d_usernames, const void* d_leaf_balances, uint32_t depth, uint32_t n_currencies,
                     void* d_node_hashes, void* d_node_balances, void* stream) {
  if (!d_usernames || !d_leaf_balances || !d_node_hashes || !d_node_balances || depth > 30)
    return fail(SG_ERR_INVALID, "sg_mst_build: bad argument");
  const size_t n = (size_t)1 << depth;
  uint8_t* h = static_cast<uint8_t*>(d_node_hashes);
  uint8_t* b = static_cast<uint8_t*>(d_node_balances);
  int rc = sg_mst_leaves_dev(d_usernames, d_leaf_balances, n, n_currencies, h, stream);
  if (rc != SG_OK) return rc;
  {
    LOCKED_CTX();
    CHECK_HIP(hipMemcpyAsync(b, d_leaf_balances, n * n_currencies * 32, hipMemcpyDeviceToDevice, pick_stream(stream)),
              "mst balances");
  }
  size_t off = 0;
  for (size_t m = n >> 1; m >= 1; m >>= 1) {
    const size_t child = off, parent = off + 2 * m;
    rc = sg_mst_level_dev(h + 32 * child, b + 32 * child * n_currencies, m, n_currencies, h + 32 * parent,
                          b + 32 * parent * n_currencies, stream);
    if (rc != SG_OK) return rc;
    off = parent;
  }
  return SG_OK;
}
// Entry::new for a whole snapshot (mst_entries.hip).  Everything that can be wrong with the host buffers is found here, before
// the device is touched: the kernels trust their offsets.  The four buffers travel in one work space of the caller's stream
// (names, digits, then the two offset arrays from an 8-byte boundary on), so calls on one stream reuse it in stream order.
int sg_mst_entries_dev(const uint8_t* name_bytes, const uint64_t* name_off, const uint8_t* digit_bytes, const uint64_t* digit_off,
                       size_t n, size_t rows, uint32_t n_currencies, void* d_usernames, void* d_balances, void* stream) {
  if (!name_bytes || !name_off || !digit_bytes || !digit_off || !d_usernames || !d_balances)
    return fail(SG_ERR_INVALID, "sg_mst_entries: null argument");
  if (n == 0 || rows < n || rows >= (1ull << 32) || n_currencies == 0 || n_currencies > 64)
    return fail(SG_ERR_INVALID, "sg_mst_entries: bad size");
  const std::string problem = mst_entries_problem(name_off, digit_bytes, digit_off, n, n_currencies);
  if (!problem.empty()) return fail(SG_ERR_INVALID, ("sg_mst_entries: " + problem).c_str());
  const size_t fields = n * (size_t)n_currencies;
  const size_t name_len = name_off[n], digit_len = digit_off[fields];
  const size_t at_digits = name_len, at_name_off = (name_len + digit_len + 7) & ~(size_t)7, at_digit_off = at_name_off + 8 * (n + 1);
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  uint8_t* d = nullptr;
  CHECK_HIP(scratch_for(s, 11, at_digit_off + 8 * (fields + 1), &d), "sg_mst_entries: work space");
  if (name_len) CHECK_HIP(hipMemcpyAsync(d, name_bytes, name_len, hipMemcpyHostToDevice, s), "sg_mst_entries: names");
  CHECK_HIP(hipMemcpyAsync(d + at_digits, digit_bytes, digit_len, hipMemcpyHostToDevice, s), "sg_mst_entries: digits");
  CHECK_HIP(hipMemcpyAsync(d + at_name_off, name_off, 8 * (n + 1), hipMemcpyHostToDevice, s), "sg_mst_entries: name offsets");
  CHECK_HIP(hipMemcpyAsync(d + at_digit_off, digit_off, 8 * (fields + 1), hipMemcpyHostToDevice, s), "sg_mst_entries: digit offsets");
  CHECK_HIP(mst_entries_launch(d, reinterpret_cast<const uint64_t*>(d + at_name_off), d + at_digits,
                               reinterpret_cast<const uint64_t*>(d + at_digit_off), n, rows, n_currencies, d_usernames, d_balances, s),
            "sg_mst_entries");
  return SG_OK;
}
// New balances for m leaves of a built tree, in place (mst.rs:169-204 for many leaves at once; witness.hip has the kernels).
// As above everything that can be wrong is found on the host first.  The geometry is the host's too (mst_update_plan.h): the
// parents to redo on every level, one launch per level, stream order the only barrier between levels.  One work space of the
// caller's stream holds the new balances as field elements (made from the digits by mst_balances_kernel), the digit offsets,
// the leaf indices followed by the plan's lists, then the digits.
int sg_mst_update_dev(const uint32_t* leaf_indices, const uint8_t* digit_bytes, const uint64_t* digit_off, size_t m, uint32_t depth,
                      uint32_t n_currencies, const void* d_usernames, void* d_leaf_balances, void* d_node_hashes, void* d_node_balances,
                      void* stream) {
  if (!leaf_indices || !digit_bytes || !digit_off || !d_usernames || !d_leaf_balances || !d_node_hashes || !d_node_balances)
    return fail(SG_ERR_INVALID, "sg_mst_update: null argument");
  if (depth > 30 || n_currencies == 0 || n_currencies > 64) return fail(SG_ERR_INVALID, "sg_mst_update: bad size");
  const uint32_t nc = n_currencies;
  const size_t leaves = (size_t)1 << depth;
  {
    // the leaves' balances live twice, in their own array and as level 0 of the nodes': two allocations
    const uintptr_t lo_a = (uintptr_t)d_leaf_balances, hi_a = lo_a + 32 * leaves * nc;
    const uintptr_t lo_b = (uintptr_t)d_node_balances, hi_b = lo_b + 32 * (2 * leaves - 1) * nc;
    if (lo_a < hi_b && lo_b < hi_a) return fail(SG_ERR_INVALID, "sg_mst_update: d_leaf_balances overlaps d_node_balances");
  }
  const std::string problem = mst_update_problem(leaf_indices, digit_bytes, digit_off, m, depth, nc);
  if (!problem.empty()) return fail(SG_ERR_INVALID, ("sg_mst_update: " + problem).c_str());
  const MstUpdatePlan plan = mst_update_plan(leaf_indices, m, depth);
  std::vector<uint32_t> lists(leaf_indices, leaf_indices + m);   // the indices, then list 1 .. list depth: one copy
  lists.insert(lists.end(), plan.nodes.begin(), plan.nodes.end());
  const size_t fields = m * (size_t)nc, digit_len = digit_off[fields];
  const size_t at_digit_off = 32 * fields, at_lists = at_digit_off + 8 * (fields + 1), at_digits = at_lists + 4 * lists.size();
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  CHECK_HIP(g_ctx->witness.init(g_ctx->stream), "sg_mst_update: Poseidon table");
  uint8_t* d = nullptr;
  CHECK_HIP(scratch_for(s, 12, at_digits + digit_len, &d), "sg_mst_update: work space");
  CHECK_HIP(hipMemcpyAsync(d + at_digit_off, digit_off, 8 * (fields + 1), hipMemcpyHostToDevice, s), "sg_mst_update: digit offsets");
  CHECK_HIP(hipMemcpyAsync(d + at_lists, lists.data(), 4 * lists.size(), hipMemcpyHostToDevice, s), "sg_mst_update: lists");
  CHECK_HIP(hipMemcpyAsync(d + at_digits, digit_bytes, digit_len, hipMemcpyHostToDevice, s), "sg_mst_update: digits");
  fp_words* new_bal = reinterpret_cast<fp_words*>(d);
  const uint32_t* d_lists = reinterpret_cast<const uint32_t*>(d + at_lists);
  CHECK_HIP(mst_balances_launch(d + at_digits, reinterpret_cast<const uint64_t*>(d + at_digit_off), fields, new_bal, s),
            "sg_mst_update: balances");
  fp_words* h = static_cast<fp_words*>(d_node_hashes);
  fp_words* b = static_cast<fp_words*>(d_node_balances);
  CHECK_HIP(g_ctx->witness.update_leaves(d_lists, new_bal, m, nc, static_cast<const fp_words*>(d_usernames),
                                         static_cast<fp_words*>(d_leaf_balances), h, b, s),
            "sg_mst_update: leaves");
  size_t child = 0;                                            // first node of level l - 1 in the level-major arrays
  for (uint32_t l = 1; l <= depth; l++) {
    const size_t parent = child + (leaves >> (l - 1));
    CHECK_HIP(g_ctx->witness.update_level(d_lists + m + plan.offset[l - 1], plan.count(l), h + child, b + child * nc, nc, h + parent,
                                          b + parent * nc, s),
              "sg_mst_update: level");
    child = parent;
  }
  return SG_OK;
}

// Circuit::synthesize on the device for users of a device-resident tree (witness.hip: the program is the floor plan)
int sg_mst_inclusion_witness_dev(const void* d_program, uint32_t n_items, uint32_t n_absorbs, const void* d_usernames,
                                 const void* d_node_hashes, const void* d_node_balances, uint32_t depth, uint32_t n_currencies,
                                 const void* d_user_indices, uint32_t n_users, void* d_advice, uint64_t rows, void* stream) {
  if (!d_program || !d_usernames || !d_node_hashes || !d_node_balances || !d_user_indices || !d_advice)
    return fail(SG_ERR_INVALID, "sg_mst_inclusion_witness: null argument");
  if (depth > 30 || n_currencies == 0 || n_currencies > 64 || rows == 0 || rows > (1ull << 28) || n_items > (1u << 24) || n_users > 65535)
    return fail(SG_ERR_INVALID, "sg_mst_inclusion_witness: bad size");
  LOCKED_CTX();
  hipStream_t s = pick_stream(stream);
  hipError_t e = g_ctx->witness.init(g_ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_advice, 0, (size_t)n_users * 3 * rows * 32, s);
  if (e == hipSuccess)
    e = g_ctx->witness.inclusion_witness(static_cast<const uint32_t*>(d_program), n_items, n_absorbs,
                                         static_cast<const fp_words*>(d_usernames), static_cast<const fp_words*>(d_node_hashes),
                                         static_cast<const fp_words*>(d_node_balances), depth, n_currencies,
                                         static_cast<const uint32_t*>(d_user_indices), n_users, static_cast<fp_words*>(d_advice),
                                         (size_t)rows, s);
  if (e != hipSuccess) return hip_fail("mst inclusion witness", e);
  return SG_OK;
}

}  // extern "C"
