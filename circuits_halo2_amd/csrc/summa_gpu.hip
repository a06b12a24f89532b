// C ABI of the MI355X back-end (include/summa_gpu.h).  Thin: argument checks, staging of
// host buffers, per-device context (stream, workspaces, twiddle / SRS caches), dispatch to
// the NTT and MSM engines.  No CPU implementation of the path exists in this library: if
// HIP is unusable every entry point fails with SG_ERR_NO_DEVICE / SG_ERR_HIP.
#include "abi_internal.h"

using namespace sg;
namespace sg {
SG_DEFINE_SIDE_PRIO_SETTER(abi_set_side_prio)

thread_local char g_err[512] = "";

int fail(int code, const char* what, hipError_t e) {
  if (e != hipSuccess) std::snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e));
  else std::snprintf(g_err, sizeof g_err, "%s", what);
  return code;
}
int hip_fail(const char* what, hipError_t e) {
  return fail(e == hipErrorOutOfMemory ? SG_ERR_NOMEM : SG_ERR_HIP, what, e);
}
// both MSM engines of a context hold one config
void msm_set(Context& c, uint32_t MsmConfig::*field, int v) { c.msm.config().*field = c.msm_b.config().*field = (uint32_t)v; }
}  // namespace sg

namespace {

__device__ void put_words(words8* dst, const f29& v_r261) {
  f29_to_words(f29_reduce_with<Fr29>(v_r261, Fr29::r256), dst->l);
}
// EvaluationDomain::new constants for 2^k (computed in the 2^261 domain, exported as words)
__global__ void domain_kernel(uint32_t k, DomainConsts* out) {
  side_kernel_prio();
  typedef Fr29 P;
  uint32_t rw[8], zw[8];
  for (int i = 0; i < 8; i++) { rw[i] = ROOT_OF_UNITY_M[i]; zw[i] = ZETA_M[i]; }
  f29 w = f29_words_to_r261<P>(rw), z = f29_words_to_r261<P>(zw);
  for (uint32_t i = k; i < 28; i++) w = f29_sqr<P>(w);
  // 2^k in the 2^261 domain: canonical integer times 2^522 * 2^-261; build it by doubling 1^
  f29 n = f29_one<P>();
  for (uint32_t i = 0; i < k; i++) n = f29_cond_sub_p<P>(f29_normalize(f29_dbl(n)));
  f29 ninv = f29_inv<P>(n);
  f29 z2 = f29_sqr<P>(z);
  put_words(&out->omega, w);
  put_words(&out->omega_inv, f29_inv<P>(w));
  put_words(&out->n_inv, ninv);
  put_words(&out->zeta, z);
  put_words(&out->zeta2, z2);
  put_words(&out->ninv_zeta2, f29_mul<P>(ninv, z2));
  put_words(&out->ninv_zeta, f29_mul<P>(ninv, z));
  put_words(&out->one, f29_one<P>());
}
// t_evaluations[i] = 1 / ((zeta * omega_ext^i)^(2^k) - 1), i < 2^(ext_k - k)
__global__ void t_eval_kernel(uint32_t k, uint32_t ext_k, words8 omega_ext, fp_words* out) {
  side_kernel_prio();
  typedef Fr29 P;
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >> (ext_k - k)) return;
  uint32_t zw[8];
  for (int j = 0; j < 8; j++) zw[j] = ZETA_M[j];
  f29 x = f29_mul<P>(f29_words_to_r261<P>(zw), f29_pow_u64<P>(f29_words_to_r261<P>(omega_ext.l), i));
  for (uint32_t s = 0; s < k; s++) x = f29_sqr<P>(x);
  x = f29_sub<P, 0>(x, f29_one<P>());
  uint32_t o[8];
  f29_to_words(f29_reduce_with<P>(f29_inv<P>(f29_mul<P>(x, f29_one<P>())), P::r256), o);
  fp_words_store(out + i, o);
}

// ParamsKZG::setup scalars: pw[i] = tau^i, lg[i] = L_i(tau) = omega^i (tau^n - 1) / (n (tau - omega^i))
// (Montgomery-2^256 words); the group part is g1_fixed_base_mul over them.
__global__ void kzg_setup_scalars(uint32_t k, words8 tau_w, fp_words* pw, fp_words* lg) {
  side_kernel_prio();
  typedef Fr29 P;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >> k) return;
  uint32_t rw[8];
  for (int q = 0; q < 8; q++) rw[q] = ROOT_OF_UNITY_M[q];
  f29 omega = f29_words_to_r261<P>(rw);
  for (uint32_t q = k; q < 28; q++) omega = f29_sqr<P>(omega);
  const f29 tau = f29_words_to_r261<P>(tau_w.l);
  uint32_t o[8];
  f29_to_words(f29_reduce_with<P>(f29_pow_u64<P>(tau, i), P::r256), o);
  fp_words_store(pw + i, o);
  f29 tn = tau;
  for (uint32_t q = 0; q < k; q++) tn = f29_sqr<P>(tn);
  f29 num = f29_sub<P, 0>(tn, f29_one<P>());                   // tau^n - 1
  f29 n = f29_one<P>();
  for (uint32_t q = 0; q < k; q++) n = f29_cond_sub_p<P>(f29_normalize(f29_dbl(n)));
  const f29 wi = f29_pow_u64<P>(omega, i);
  const f29 diff = f29_sub<P, 0>(tau, wi);
  f29 den = f29_mul<P>(n, diff);                               // n (tau - omega^i)
  f29 l = f29_mul<P>(f29_mul<P>(wi, num), f29_inv<P>(den));
  // tau is the domain point omega^i: 0 / 0 above (the inverse of 0 is 0), and L_i(omega^i) = 1 by definition; num is zero
  // for the whole domain then, so every other row is 0 already
  if (f29_is_zero_mod_p<P>(diff)) l = f29_one<P>();
  f29_to_words(f29_reduce_with<P>(l, P::r256), o);
  fp_words_store(lg + i, o);
}

static constexpr int kLanes = 8;          // upper bound; "lanes" of them are handed out (the concurrency model, below)

// ---- runtime parameters (sg_set_param / sg_get_param, one line each in include/summa_gpu.h).  kParams is the only list of
// them: a row holds a name, its scope, its default, what an incoming value becomes and how it takes effect.  The values in
// effect live in Shared::param; the library reads its configs and those atomics as before -- nothing here is looked up by
// name on a launch path.
enum class Scope {
  process,   // Shared::param is what the library reads (to_process: a copy elsewhere that needs the value too)
  lane,      // to_lane writes one context's configs: every existing lane when the value is set, every new one when it is made
  device,    // side_prio: to_process writes the device's copy -- when set while a device is bound, and when a context is made
};
struct ParamRow {
  const char* name;
  Scope scope;
  int def;                          // what sg_get_param reports until the parameter is set
  int (*clamp)(int);                // the value in effect for a requested one (>= 0), or -1: rejected
  void (*to_lane)(Context&, int);
  int (*to_process)(int);
};
template <int lo, int hi>
constexpr int in_range(int v) { return std::min(hi, std::max(lo, v)); }
constexpr int kNoLimit = 0x7fffffff;
// side_prio is device-wide, not per lane: wave priority 3 for every kernel but msm_accumulate (side_prio.cuh)
int set_side_prio(int on) {
  hipError_t e = msm_set_side_prio(on);
  if (e == hipSuccess) e = msm_tiny_set_side_prio(on);
  if (e == hipSuccess) e = msm_many_set_side_prio(on);
  if (e == hipSuccess) e = ntt_set_side_prio(on);
  if (e == hipSuccess) e = poly_set_side_prio(on);
  if (e == hipSuccess) e = quotient_set_side_prio(on);
  if (e == hipSuccess) e = gates_set_side_prio(on);
  if (e == hipSuccess) e = numerator_set_side_prio(on);
  if (e == hipSuccess) e = witness_set_side_prio(on);
  if (e == hipSuccess) e = mst_entries_set_side_prio(on);
  if (e == hipSuccess) e = abi_set_side_prio(on);
  if (e != hipSuccess) return hip_fail("side_prio", e);
  return SG_OK;
}
// a lane row named after its config field, whose default is what the config struct holds
#define MSM_ROW(field, clamp) \
  { "msm." #field, Scope::lane, (int)MsmConfig{}.field, clamp, [](Context& c, int v) { msm_set(c, &MsmConfig::field, v); }, nullptr }
#define NTT_ROW(field, clamp) \
  { "ntt." #field, Scope::lane, (int)NttConfig{}.field, clamp, [](Context& c, int v) { c.ntt.config().field = (uint32_t)v; }, nullptr }
constexpr ParamRow kParams[] = {
    {"lanes", Scope::process, 4, [](int v) { return v >= 1 && v <= kLanes ? v : -1; }, nullptr, nullptr},
    {"commit.combine_wait_us", Scope::process, 300, in_range<0, 100000>, nullptr, nullptr},
    {"commit.combine_target", Scope::process, 4, in_range<1, 32>, nullptr, nullptr},
    {"commit.combine_runners", Scope::process, 1, in_range<1, 4>, nullptr, nullptr},
    {"host.wait_sleep_us", Scope::process, 0, in_range<0, 1000>, nullptr, [](int v) -> int { host_wait_sleep_us().store(v); return SG_OK; }},
    {"msm.host_chunks", Scope::process, 0, in_range<0, 8>, nullptr, nullptr},
    {"msm.tiny_max", Scope::process, (int)MSM_TINY_MAX, in_range<0, (int)MSM_TINY_MAX>, nullptr, nullptr},
    // setting 1 clears the launch log, so that set(get) is not a no-op here while the log is on
    {"msm.acc_log", Scope::process, 0, in_range<0, 1>, nullptr, [](int v) -> int { msm_acc_log_enable(v != 0); return SG_OK; }},
    {"ntt.coset_scale_pass", Scope::process, 0, in_range<0, 1>, nullptr, nullptr},
    {"quotient.fused_numerator", Scope::process, 1, in_range<0, 1>, nullptr, nullptr},
    {"debug.fail_next_fused_job", Scope::process, 0, in_range<0, 1>, nullptr, nullptr},   // the combiner takes it back to 0
    {"side_prio", Scope::device, 1, in_range<0, 1>, nullptr, set_side_prio},
    MSM_ROW(window_bits, (in_range<0, kNoLimit>)),
    MSM_ROW(log_seg, (in_range<0, 12>)),
    // 0: the built-in sizes of each kind (2^25 generic, 2^27 fixed-base); anything else applies to both
    {"msm.log_fuse_entries", Scope::lane, 0, [](int v) { return v ? in_range<16, 30>(v) : 0; },
     [](Context& c, int v) {
       msm_set(c, &MsmConfig::log_fuse_entries, v ? v : (int)MSM_LOG_FUSE_ENTRIES_GENERIC);
       msm_set(c, &MsmConfig::log_fuse_entries_fixed, v ? v : (int)MSM_LOG_FUSE_ENTRIES_FIXED);
     }, nullptr},
    {"msm.red_threads", Scope::lane, 256, [](int v) { return v <= 64 ? 64 : v <= 128 ? 128 : 256; },
     [](Context& c, int v) { msm_set(c, &MsmConfig::red_threads, v); }, nullptr},
    {"msm.acc_threads", Scope::lane, 0, [](int v) { return v == 64 || v == 128 || v == 256 ? v : 0; },
     [](Context& c, int v) { msm_set(c, &MsmConfig::acc_threads, v); }, nullptr},
    MSM_ROW(log_scatter_rounds, (in_range<0, 6>)),
    MSM_ROW(two_pass, (in_range<0, 2>)),
    MSM_ROW(fused_frontend, (in_range<0, 2>)),
    MSM_ROW(acc_trace, (in_range<0, 1>)),
    MSM_ROW(acc_chain, (in_range<0, 1>)),
    MSM_ROW(red_lean, (in_range<0, 2>)),
    MSM_ROW(acc_waves_fixed, (in_range<0, 8>)),
    MSM_ROW(acc_waves, (in_range<0, 8>)),
    MSM_ROW(merge_quad_tasks, (in_range<0, kNoLimit>)),
    MSM_ROW(red2d_max_sets, (in_range<0, 32>)),
    MSM_ROW(red2d_fold, (in_range<1, 256>)),
    MSM_ROW(red2d_prefold, (in_range<0, 1>)),
    MSM_ROW(prefold_quad_buckets, (in_range<0, kNoLimit>)),
    MSM_ROW(red2d, (in_range<0, 2>)),
    MSM_ROW(quad, (in_range<0, 2>)),
    MSM_ROW(log_red_chunk, (in_range<0, 8>)),
    NTT_ROW(tile_log, (in_range<6, 12>)),
    NTT_ROW(threads, (in_range<64, 1024>)),
    NTT_ROW(big_tile_log, ([](int v) { return v ? in_range<6, 12>(v) : 0; })),   // 0: one shape for all
    NTT_ROW(big_threads, (in_range<64, 1024>)),
    NTT_ROW(batch_min, (in_range<1, kNoLimit>)),
    NTT_ROW(big_log, (in_range<1, kNoLimit>)),
    // 0: by size, 1: always, 2: never (NttConfig::radix4 counts the other way round: 1, 2, 0)
    {"ntt.radix4", Scope::lane, 0, [](int v) { return v == 1 || v == 2 ? v : 0; },
     [](Context& c, int v) { c.ntt.config().radix4 = v == 1 ? 2u : v == 2 ? 0u : 1u; }, nullptr},
    // the plans are cut by these two: the cached ones go.  No pass longer than 2^NTT_MAX_PASS_LOG points: its tile would not fit the LDS
    {"ntt.max_single_log", Scope::lane, (int)NttConfig{}.max_single_log, in_range<1, (int)NTT_MAX_PASS_LOG>,
     [](Context& c, int v) { c.ntt.config().max_single_log = (uint32_t)v; c.ntt.clear(); }, nullptr},
    {"ntt.max_multi_log", Scope::lane, (int)NttConfig{}.max_multi_log, in_range<4, (int)NTT_MAX_PASS_LOG>,
     [](Context& c, int v) { c.ntt.config().max_multi_log = (uint32_t)v; c.ntt.clear(); }, nullptr},
};
#undef MSM_ROW
#undef NTT_ROW
constexpr size_t kNumParams = sizeof kParams / sizeof kParams[0];
constexpr bool same_name(const char* a, const char* b) {
  while (*a && *a == *b) a++, b++;
  return *a == *b;
}
constexpr size_t param_index(const char* name) {   // kNumParams: no such parameter
  size_t i = 0;
  while (i < kNumParams && !same_name(kParams[i].name, name)) i++;
  return i;
}
constexpr bool params_sound() {   // every default is a value its own row keeps; every name is unique; every row takes effect
  for (size_t i = 0; i < kNumParams; i++) {
    const ParamRow& r = kParams[i];
    if (r.def < 0 || r.clamp(r.def) != r.def || param_index(r.name) != i) return false;
    if ((r.scope == Scope::lane) != (r.to_lane != nullptr) || (r.scope == Scope::device && !r.to_process)) return false;
  }
  return true;
}
static_assert(params_sound(), "kParams");

}  // namespace

namespace sg {

// the process rows the library reads in Shared::param
constexpr size_t kRowLanes = param_index("lanes"), kRowCombineWaitUs = param_index("commit.combine_wait_us"),
                 kRowCombineTarget = param_index("commit.combine_target"), kRowCombineRunners = param_index("commit.combine_runners"),
                 kRowHostChunks = param_index("msm.host_chunks"), kRowTinyMax = param_index("msm.tiny_max"),
                 kRowCosetScalePass = param_index("ntt.coset_scale_pass"), kRowFusedNumerator = param_index("quotient.fused_numerator"),
                 kRowFailNextFusedJob = param_index("debug.fail_next_fused_job");
static_assert(std::max({kRowLanes, kRowCombineWaitUs, kRowCombineTarget, kRowCombineRunners, kRowHostChunks, kRowTinyMax,
                        kRowCosetScalePass, kRowFusedNumerator, kRowFailNextFusedJob}) < kNumParams, "kParams");
static_assert(kNumParams <= kMaxParams, "kParams");

Shared::Shared() {
  for (size_t i = 0; i < kNumParams; i++) param[i].store(kParams[i].def);
}

// Concurrency model.  The library keeps "lanes" (default 4, at most kLanes) independent contexts ("lanes"), each with its own streams, MSM
// engines, NTT plans, staging and scratch buffers.  A call takes ONE lane for its whole duration (lane 0 when it is
// free, so a single-threaded caller always works in the same warm work space) and touches nothing of the others:
// calls from different host threads -- halo2 reaches best_multiexp / best_fft from rayon iterators; the batch driver
// keeps several proofs in flight -- run side by side on the device, host tails included.  Asynchronous `_dev` calls
// leave work behind only in buffers keyed by the caller's stream, so a lane can be handed to the next caller as soon
// as the call returns.  The lock is per lane and re-entrant for the owning thread (entry points that stage host
// buffers and then call their `_dev` form keep the lane in between).
Shared g_sh;
thread_local Context* g_ctx = nullptr;   // the lane this thread holds (valid inside LOCKED_CTX scopes only)
thread_local int g_depth = 0;

}  // namespace sg

namespace {

struct Lane {
  std::mutex mu;
  Context* ctx = nullptr;
};
Lane g_lanes[kLanes];
std::atomic<unsigned> g_rr{0};
thread_local Lane* g_held = nullptr;

// a new context takes every lane and device value in effect
void apply_params(Context& c) {
  for (size_t i = 0; i < kNumParams; i++) {
    if (kParams[i].scope == Scope::lane) kParams[i].to_lane(c, g_sh.param[i].load());
    else if (kParams[i].scope == Scope::device) (void)kParams[i].to_process(g_sh.param[i].load());
  }
}

// The main streams of the lanes in use are created together, before any of the library's other streams, so that they land
// on different hardware queues: two streams on ONE queue run their kernels one after the other whatever the priorities,
// and the next MSM's sort then sits behind the current accumulation instead of under it
// (profiles/r03_sweeps/persistent_accumulate.txt).  No more of them than lanes: every stream is a queue the firmware has
// to schedule, and idle ones cost too (a k = 17 proof: 5.83 ms with four, 6.27 ms with eight; raising HIP's number of
// hardware queues, GPU_MAX_HW_QUEUES = 8 / 16, takes a batch of sixteen proofs in flight from 237 to 140 / 52 proofs/s).
hipStream_t g_lane_main[kLanes] = {};   // guarded by g_sh.mu
hipError_t make_lane_streams(int count) {
  for (int i = 0; i < count && i < kLanes; i++) {
    if (g_lane_main[i]) continue;
    hipError_t e = hipStreamCreateWithFlags(&g_lane_main[i], hipStreamNonBlocking);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
int make_context(int device, int lane_index, Context** out) {
  Context* c = new Context();
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) {
    std::lock_guard<std::mutex> lk(g_sh.mu);
    e = make_lane_streams(std::max(g_sh.param[kRowLanes].load(), lane_index + 1));
    if (e == hipSuccess) c->stream = g_lane_main[lane_index];
  }
  if (e == hipSuccess) e = c->ntt.init();
  if (e == hipSuccess) e = c->msm.init();
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->bstream[0], hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->bstream[1], hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming);
  if (e == hipSuccess) e = hipMalloc(&c->d_consts, sizeof(DomainConsts));
  if (e != hipSuccess) {
    delete c;
    return hip_fail("sg_init", e);
  }
  c->device = device;
  *out = c;
  return SG_OK;
}

void destroy_context(Context* c) {
  for (auto& kv : c->t_evals) (void)hipFree(kv.second);
  for (auto& kv : c->coset_tables) {
    (void)hipFree(kv.second.fwd);
    (void)hipFree(kv.second.inv);
  }
  for (auto* ring : {&c->blob_ring, &c->kate_ring})
    for (auto& slot : ring->slot) {
      if (slot.ev) (void)hipEventDestroy(slot.ev);
      if (slot.host) (void)hipHostFree(slot.host);
      if (slot.dev) (void)hipFree(slot.dev);
    }
  c->ntt.clear();
  c->msm.release();
  c->msm_b.release();
  c->witness.release();
  for (auto& bs : c->bstream) {
    if (bs) (void)hipStreamDestroy(bs);
  }
  for (auto& ts : c->tstream) {
    if (ts) (void)hipStreamDestroy(ts);
  }
  if (c->ev_in) (void)hipEventDestroy(c->ev_in);
  c->stage_a.release();
  c->stage_b.release();
  c->scratch.release();
  for (auto& kv : c->stream_scratch) kv.second.release();
  for (auto& kv : c->lookup_work) kv.second.buf.release();
  if (c->h_mail) (void)hipHostFree(c->h_mail);
  if (c->h_many) (void)hipHostFree(c->h_many);
  if (c->d_consts) (void)hipFree(c->d_consts);
  c->stream = nullptr;   // one of g_lane_main: destroyed with the others at sg_shutdown
  delete c;
}

// take a lane for the calling thread (g_ctx / g_held): lane 0 if free, else the first free one, else wait
int acquire_lane() {
  int device;
  {
    std::lock_guard<std::mutex> lk(g_sh.mu);
    if (g_sh.device < 0) {
      // lazy default initialisation on device 0 keeps the seam a pure function call, like best_multiexp / best_fft
      int n = 0;
      if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(SG_ERR_NO_DEVICE, "no HIP device visible");
      g_sh.device = 0;
    }
    device = g_sh.device;
  }
  Lane* lane = nullptr;
  const int lanes = g_sh.param[kRowLanes].load();
  for (int i = 0; i < lanes && !lane; i++)
    if (g_lanes[i].mu.try_lock()) lane = &g_lanes[i];
  if (!lane) {   // more concurrent callers than lanes: wait for one (round-robin), for the whole of its current call
    lane = &g_lanes[g_rr.fetch_add(1) % (unsigned)lanes];
    lane->mu.lock();
  }
  if (!lane->ctx) {
    int rc = make_context(device, (int)(lane - g_lanes), &lane->ctx);
    if (rc != SG_OK) {
      lane->mu.unlock();
      return rc;
    }
    apply_params(*lane->ctx);
  }
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) {
    lane->mu.unlock();
    return hip_fail("hipSetDevice", e);
  }
  g_held = lane;
  g_ctx = lane->ctx;
  return SG_OK;
}

}  // namespace

namespace sg {

// The kernels of the family files live here, beside domain_kernel: every translation unit with a kernel holds a copy of the
// side_prio switch (side_prio.cuh) that sg_set_param has to write, and one copy is enough for these three.
void t_eval_launch(uint32_t k, uint32_t ext_k, const words8& omega_ext, fp_words* out, hipStream_t s) {
  const uint32_t cnt = 1u << (ext_k - k);
  t_eval_kernel<<<(cnt + 63) / 64, 64, 0, s>>>(k, ext_k, omega_ext, out);
}
void kzg_setup_scalars_launch(uint32_t k, const words8& tau, fp_words* pw, fp_words* lg, hipStream_t s) {
  kzg_setup_scalars<<<(unsigned)((((size_t)1 << k) + 127) / 128), 128, 0, s>>>(k, tau, pw, lg);
}

LaneHold::LaneHold() {
  if (g_depth > 0) {
    g_depth++;
    return;
  }
  rc = acquire_lane();
  if (rc == SG_OK) g_depth = 1;
}
LaneHold::~LaneHold() {
  if (rc != SG_OK) return;
  if (--g_depth == 0) {
    Lane* l = g_held;
    g_held = nullptr;
    g_ctx = nullptr;
    l->mu.unlock();
  }
}

// the SRS behind a handle: a COPY of the entry (device pointers, window tables' descriptors), taken under the lock, so
// that a concurrent sg_srs_precompute / sg_srs_free on another lane never changes it under a reader.  The device
// memory it names stays valid while the handle does (retired tables are kept until sg_collect_retired / sg_shutdown).
bool find_srs(uint64_t handle, Srs* out) {
  std::lock_guard<std::mutex> lk(g_sh.mu);
  auto it = g_sh.srs.find(handle);
  if (it == g_sh.srs.end()) return false;
  *out = it->second;
  return true;
}

int get_consts(uint32_t k, const DomainConsts** out) {
  Context& c = *g_ctx;
  auto it = c.consts.find(k);
  if (it == c.consts.end()) {
    domain_kernel<<<1, 1, 0, c.stream>>>(k, c.d_consts);
    DomainConsts h;
    CHECK_HIP(hipMemcpyAsync(&h, c.d_consts, sizeof h, hipMemcpyDeviceToHost, c.stream), "domain constants");
    CHECK_HIP(host_wait_stream(c.stream), "domain constants");
    it = c.consts.emplace(k, h).first;
  }
  *out = &it->second;
  return SG_OK;
}

// _dev entry points run on exactly the stream they are given (NULL = HIP's default stream,
// which is what torch.cuda.current_stream() is unless the caller switched streams)
hipStream_t pick_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// order the library's own stream work (plan/twiddle generation) before a caller stream
int sync_own_stream_into(hipStream_t s) {
  if (s == g_ctx->stream) return SG_OK;
  CHECK_HIP(host_wait_stream(g_ctx->stream), "stream sync");
  return SG_OK;
}

int ntt_dev(const fp_words* in, size_t in_len, fp_words* out, uint32_t log_n, const words8& omega,
            const words8* scale, const words8* pre3, const words8* post3, hipStream_t s) {
  Context& c = *g_ctx;
  if (log_n > 28) return fail(SG_ERR_INVALID, "log_n exceeds the 2-adicity (28) of BN254 Fr");
  // the scratch vector of a lone transform is the stream's own (slot 13: the batched transforms' slot 3 keeps its size), so
  // that transforms enqueued on a side stream never share it with work in flight on another stream
  uint8_t* scratch = nullptr;
  if (ntt_needs_scratch(c.ntt.config(), log_n, in == out)) {
    hipError_t e = scratch_for(s, 13, (size_t)32 << log_n, &scratch);
    if (e != hipSuccess) return hip_fail("ntt scratch", e);
  }
  // plans are generated on the same stream the transform runs on
  hipError_t e = c.ntt.transform(in, in_len, out, reinterpret_cast<fp_words*>(scratch), log_n, omega, scale, pre3, post3, s);
  if (e != hipSuccess) return hip_fail("ntt", e);
  return SG_OK;
}

hipError_t mailbox(uint8_t** host, uint8_t** dev) {
  Context& c = *g_ctx;
  if (!c.h_mail) {
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&c.h_mail), Context::MAIL_BYTES, hipHostMallocMapped | hipHostMallocCoherent);
    if (e != hipSuccess) return e;
    e = hipHostGetDevicePointer(reinterpret_cast<void**>(&c.d_mail), c.h_mail, 0);
    if (e != hipSuccess) return e;
  }
  *host = c.h_mail;
  *dev = c.d_mail;
  return hipSuccess;
}

hipError_t ring_slot(Context::BlobRing& ring, size_t bytes, size_t grow_to, Context::BlobSlot** out) {
  Context::BlobSlot& slot = ring.slot[ring.next++ % ring.size];
  *out = &slot;
  hipError_t e = hipSuccess;
  if (!slot.ev) e = hipEventCreateWithFlags(&slot.ev, hipEventDisableTiming);
  else if (hipEventQuery(slot.ev) != hipSuccess) e = host_wait_event(slot.ev);   // (a query first: waiting on an event that
                                                                                     // has long completed still costs a wake-up, 0.3 ms)
  if (e == hipSuccess && slot.cap < bytes) {
    if (slot.host) (void)hipHostFree(slot.host);
    retire_device_memory(slot.dev);
    slot.host = nullptr;
    slot.dev = nullptr;
    slot.cap = 0;
    e = hipHostMalloc(reinterpret_cast<void**>(&slot.host), grow_to, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&slot.dev), grow_to);
    if (e == hipSuccess) slot.cap = grow_to;
  }
  return e;
}

hipError_t scratch_for(hipStream_t s, int slot, size_t bytes, uint8_t** out) {
  DevBuf<uint8_t>& buf = g_ctx->stream_scratch[std::make_pair(s, slot)];
  hipError_t e = buf.reserve(bytes);  // growing frees the old buffer, which waits for the device: safe
  *out = buf.p;
  return e;
}

int upload(DevBuf<uint8_t>& buf, const uint8_t* host, size_t bytes, hipStream_t s) {
  hipError_t e = buf.reserve(bytes ? bytes : 1);
  if (e != hipSuccess) return hip_fail("staging buffer", e);
  if (bytes) CHECK_HIP(hipMemcpyAsync(buf.p, host, bytes, hipMemcpyHostToDevice, s), "H2D copy");
  return SG_OK;
}
int download(uint8_t* host, const void* dev, size_t bytes, hipStream_t s) {
  CHECK_HIP(host_copy_d2h(host, dev, bytes, s), "D2H copy");
  return SG_OK;
}

}  // namespace sg

extern "C" {

int sg_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}
const char* sg_version(void) { return "summa_gpu 0.1.0 gfx950"; }
int sg_device(void) {
  std::lock_guard<std::mutex> lk(g_sh.mu);
  return g_sh.device;
}
int sg_bind_thread(void) {
  const int device = sg_device();
  if (device < 0) return SG_OK;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return hip_fail("sg_bind_thread", e);
  return SG_OK;
}
const char* sg_last_error(void) { return g_err; }

int sg_init(int device) {
  {
    std::lock_guard<std::mutex> lk(g_sh.mu);
    if (g_sh.device == device) return SG_OK;
    if (g_sh.device >= 0) return fail(SG_ERR_INVALID, "sg_init: already bound to another device (one process per GPU)");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(SG_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n) return fail(SG_ERR_INVALID, "sg_init: device index out of range");
    g_sh.device = device;
  }
  LOCKED_CTX();   // creates lane 0: streams, plans' home, MSM engine attributes
  return SG_OK;
}

// host ranges page-locked for the library (sg_host_register, below)
struct HostRange {
  uintptr_t base;
  size_t bytes;
};
static std::mutex g_host_mu;
static std::vector<HostRange> g_host_ranges;
void sg_shutdown(void) {
  if (g_depth > 0) return;   // never from inside a call
  for (auto& l : g_lanes) l.mu.lock();
  int device;
  {
    std::lock_guard<std::mutex> lk(g_sh.mu);
    device = g_sh.device;
  }
  if (device >= 0) {
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();
    for (auto& l : g_lanes) {
      if (l.ctx) destroy_context(l.ctx);
      l.ctx = nullptr;
    }
    {
      std::lock_guard<std::mutex> lk(g_sh.mu);
      for (auto& st : g_lane_main) {
        if (st) (void)hipStreamDestroy(st);
        st = nullptr;
      }
    }
    {
      std::lock_guard<std::mutex> lk(g_host_mu);
      for (const HostRange& r : g_host_ranges) (void)hipHostUnregister(reinterpret_cast<void*>(r.base));
      g_host_ranges.clear();
    }
    std::lock_guard<std::mutex> lk(g_sh.mu);
    for (auto& kv : g_sh.srs) {
      (void)hipFree(kv.second.g);
      (void)hipFree(kv.second.g_lagrange);
      if (kv.second.lagrange_prefix) (void)hipFree(kv.second.lagrange_prefix);
      for (auto& t : kv.second.tab)
        if (t.table) (void)hipFree(t.table);
    }
    g_sh.srs.clear();
    for (auto& kv : g_sh.many) (void)hipFree(kv.second.S);
    g_sh.many.clear();
    g_sh.device = -1;
    retired_device_memory_collect();
    summa::prover::release_orphans();   // what the prover sessions of ended threads left behind
  }
  for (auto& l : g_lanes) l.mu.unlock();
}

// Returns the device memory the library has outgrown since it started (work spaces that were reallocated larger, window
// tables replaced by sg_srs_precompute).  It waits for the device: call it when no other call is in flight.
// ---- host memory the caller has page-locked for the library (sg_host_register): the host-pointer entry points move such
// ranges by direct DMA at link speed, asynchronously; anything else goes through the runtime's pageable path
[[maybe_unused]] static bool host_registered(const void* p, size_t bytes) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  std::lock_guard<std::mutex> lk(g_host_mu);
  for (const HostRange& r : g_host_ranges)
    if (a >= r.base && a + bytes <= r.base + r.bytes) return true;
  return false;
}
int sg_host_register(void* host, size_t bytes) {
  if (!host || !bytes) return fail(SG_ERR_INVALID, "sg_host_register: null or empty range");
  {
    LOCKED_CTX();   // a device is bound (the registration is made for it)
    const uintptr_t a = reinterpret_cast<uintptr_t>(host);
    {
      std::lock_guard<std::mutex> lk(g_host_mu);
      for (const HostRange& r : g_host_ranges)
        if (a < r.base + r.bytes && r.base < a + bytes) return fail(SG_ERR_INVALID, "sg_host_register: overlaps a registered range");
    }
    CHECK_HIP(hipHostRegister(host, bytes, hipHostRegisterDefault), "hipHostRegister");
    std::lock_guard<std::mutex> lk(g_host_mu);
    g_host_ranges.push_back({a, bytes});
  }
  return SG_OK;
}
int sg_host_unregister(void* host) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(host);
  {
    std::lock_guard<std::mutex> lk(g_host_mu);
    auto it = std::find_if(g_host_ranges.begin(), g_host_ranges.end(), [&](const HostRange& r) { return r.base == a; });
    if (it == g_host_ranges.end()) return fail(SG_ERR_INVALID, "sg_host_unregister: not the start of a registered range");
    g_host_ranges.erase(it);
  }
  CHECK_HIP(hipHostUnregister(host), "hipHostUnregister");
  return SG_OK;
}

int sg_stream_wait(void* stream) {
  const hipError_t e = host_wait_stream(static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail("sg_stream_wait", e);
  return SG_OK;
}

int sg_collect_retired(void) {
  if (g_depth > 0) return fail(SG_ERR_INVALID, "sg_collect_retired: not from inside a call");
  int device;
  {
    std::lock_guard<std::mutex> lk(g_sh.mu);
    device = g_sh.device;
  }
  if (device < 0) return SG_OK;
  for (auto& l : g_lanes) l.mu.lock();       // index order, no lane of our own held: no call is in flight meanwhile
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) {
    retired_device_memory_collect();
    summa::prover::release_orphans();
    // the lanes' own work spaces too (MSM buckets and sort buffers, NTT plans and twiddle tables, staging, scratch): which
    // lane met the largest job of the last workload is a matter of timing, so "what the library holds" would otherwise
    // creep up to lanes x the largest work space over a long-lived process.  They are rebuilt by the next call that
    // needs them (milliseconds); the lanes' main streams, the SRS cache and the proving keys stay.
    for (auto& l : g_lanes) {
      if (l.ctx) destroy_context(l.ctx);
      l.ctx = nullptr;
    }
  }
  for (auto& l : g_lanes) l.mu.unlock();
  if (e != hipSuccess) return hip_fail("sg_collect_retired", e);
  return SG_OK;
}

int sg_set_param(const char* name, int value) {
  if (!name || value < 0) return fail(SG_ERR_INVALID, "sg_set_param: bad argument");
  if (g_depth > 0) return fail(SG_ERR_INVALID, "sg_set_param: not from inside a call");
  const size_t i = param_index(name);
  if (i == kNumParams) return fail(SG_ERR_INVALID, "sg_set_param: unknown parameter");
  const ParamRow& row = kParams[i];
  const int v = row.clamp(value);
  if (v < 0) return fail(SG_ERR_INVALID, "sg_set_param: value out of range (lanes: 1..8)");
  int device;
  {
    std::lock_guard<std::mutex> lk(g_sh.mu);
    g_sh.param[i].store(v);
    device = g_sh.device;
    if (row.scope == Scope::process && row.to_process) return row.to_process(v);
  }
  if (row.scope == Scope::device && device >= 0) {   // with no device bound yet, the first context applies it
    CHECK_HIP(hipSetDevice(device), "sg_set_param");
    return row.to_process(v);
  }
  if (row.scope == Scope::lane) {
    // the lanes that exist already, one at a time and with none held (two threads setting parameters at once cannot
    // wait for each other's lane): each when it is idle, with the value in effect then
    for (auto& l : g_lanes) {
      std::lock_guard<std::mutex> lk(l.mu);
      if (l.ctx) row.to_lane(*l.ctx, g_sh.param[i].load());
    }
  }
  return SG_OK;
}

int sg_get_param(const char* name, int* value) {
  if (!name || !value) return fail(SG_ERR_INVALID, "sg_get_param: bad argument");
  const size_t i = param_index(name);
  if (i == kNumParams) return fail(SG_ERR_INVALID, "sg_get_param: unknown parameter");
  *value = g_sh.param[i].load();
  return SG_OK;
}

int sg_abi_version(void) { return SG_ABI_VERSION; }

}  // extern "C"
