// C ABI, MSM family: sg_msm_*, the SRS cache, sg_commit* and the commit combiner's entry points (summa_gpu.hip holds the core).
// Glue: what a commitment decides on the host is commit_plan.h's, the combiner's logic commit_combiner.h's (both HIP-free).
#include "abi_internal.h"
#include "commit_combiner.h"
#include "commit_plan.h"

using namespace sg;
namespace {

void report_timings(sg_msm_timings* timings, const MsmTimings& tm) {
  if (!timings) return;
  timings->digits_ms = tm.digits_ms; timings->sort_ms = tm.sort_ms; timings->accumulate_ms = tm.accumulate_ms;
  timings->reduce_ms = tm.reduce_ms; timings->total_ms = tm.total_ms; timings->window_bits = tm.window_bits;
  timings->windows = tm.windows; timings->tasks = tm.tasks; timings->max_bucket = tm.max_bucket;
  timings->accumulate_threads = tm.accumulate_threads;
  timings->order_ms = tm.order_ms;
}
// the SRS a commitment of n scalars runs against (a copy: find_srs)
int srs_for_commit(uint64_t handle, size_t n, Srs* out) {
  if (!find_srs(handle, out)) return fail(SG_ERR_INVALID, "unknown SRS handle");
  if (n > ((size_t)1 << out->k)) return fail(SG_ERR_INVALID, "sg_commit: polynomial longer than the SRS");
  return SG_OK;
}
// what commit_plan.h's rules ask of an SRS
SrsTables tables_of(const Srs& s) {
  SrsTables t;
  t.k = s.k;
  for (int b = 0; b < 3; b++) t.tab[b] = {s.tab[b].table != nullptr, s.tab[b].c, s.tab[b].n};
  return t;
}
// the jobs behind a handle of sg_msm_g1_many_begin (a copy, as find_srs); take: the handle ends here
bool find_many(uint64_t handle, ManyJobs* out, bool take = false) {
  std::lock_guard<std::mutex> lk(g_sh.mu);
  auto it = g_sh.many.find(handle);
  if (it == g_sh.many.end()) return false;
  *out = it->second;
  if (take) g_sh.many.erase(it);
  return true;
}
// 2^k points of g and of g_lagrange into device memory of the cache's own, under a new handle: from host memory, or (from_device)
// by device-to-device copies on `st` (e.g. out of the receive buffers of an RCCL broadcast)
int srs_upload(uint32_t k, const void* g, const void* g_lagrange, bool from_device, hipStream_t st, uint64_t* handle_out, const char* what) {
  const size_t bytes = (size_t)64 << k;
  Srs s{k, nullptr, nullptr, {}};
  hipError_t e = hipMalloc(&s.g, bytes);
  if (e == hipSuccess) e = hipMalloc(&s.g_lagrange, bytes);
  if (e == hipSuccess) e = from_device ? hipMemcpyAsync(s.g, g, bytes, hipMemcpyDeviceToDevice, st) : hipMemcpy(s.g, g, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = from_device ? hipMemcpyAsync(s.g_lagrange, g_lagrange, bytes, hipMemcpyDeviceToDevice, st)
                    : hipMemcpy(s.g_lagrange, g_lagrange, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess && from_device) e = host_wait_stream(st);   // the bases are read from other streams afterwards
  if (e != hipSuccess) {
    if (s.g) (void)hipFree(s.g);
    if (s.g_lagrange) (void)hipFree(s.g_lagrange);
    return hip_fail(what, e);
  }
  std::lock_guard<std::mutex> lk(g_sh.mu);
  const uint64_t h = g_sh.next_handle++;
  g_sh.srs[h] = s;
  *handle_out = h;
  return SG_OK;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------ MSM
int sg_msm_g1_dev_timed(const void* d_scalars, const void* d_bases, size_t n, void* stream, uint8_t out_affine[64],
                        sg_msm_timings* timings) {
  if (!out_affine || (n && (!d_scalars || !d_bases))) return fail(SG_ERR_INVALID, "sg_msm_g1: null argument");
  LOCKED_CTX();
  MsmTimings tm;
  // on the lane's own stream, after everything the caller has enqueued on his: the call returns the point, so nothing of
  // it is left on any stream afterwards, and the lanes' streams sit on different hardware queues (make_lane_streams) --
  // which the streams of callers on different threads may or may not
  hipStream_t st = pick_stream(stream);
  if (st != g_ctx->stream) {
    // (an idle caller stream needs no edge -- and a marker on it would queue behind whatever shares ITS hardware queue,
    // another lane's accumulation for instance)
    if (hipStreamQuery(st) != hipSuccess) {
      CHECK_HIP(hipEventRecord(g_ctx->ev_in, st), "event");
      CHECK_HIP(hipStreamWaitEvent(g_ctx->stream, g_ctx->ev_in, 0), "wait");
    }
    st = g_ctx->stream;
  }
  hipError_t e = g_ctx->msm.run(static_cast<const fp_words*>(d_scalars), static_cast<const g1_affine_mem*>(d_bases), n,
                                st, out_affine, timings ? &tm : nullptr);
  if (e != hipSuccess) return hip_fail("msm", e);
  report_timings(timings, tm);
  return SG_OK;
}
int sg_msm_g1_dev(const void* d_scalars, const void* d_bases, size_t n, void* stream, uint8_t out_affine[64]) {
  return sg_msm_g1_dev_timed(d_scalars, d_bases, n, stream, out_affine, nullptr);
}
// The host-pointer MSM entry points (sg_msm_g1: scalars and bases in host memory; sg_commit: scalars in host memory, bases
// resident) pay the link -- 96 or 32 bytes per pair at the 56 GB/s this platform reaches from pageable memory just as from
// page-locked memory -- before the last addition can run, and a lone MSM is a third latency chains (sort front end, bucket
// reduction, host tail) besides.  Large inputs are therefore cut into K chunks that run as K jobs on the lane's two
// engines (two streams) while a third stream carries the copies: chunk i's job runs while chunk i + 1 is still travelling,
// and one job's latency chains run under the other's accumulation.  The K partial points are added on the host.
//   [S0 B0] front(0) { back(i) [S i+1 B i+1] finish(i-1) front(i+1) } ... finish, sum
// -- chunk i + 1 crosses the link while chunk i's accumulation runs.  The order and what a failure leaves of it:
// run_chunk_pipeline (commit_plan.h), which also holds K's rule (host_chunk_count) and the chunks' bounds.
static int msm_host_chunked(const uint8_t* scalars, const uint8_t* bases_host, const g1_affine_mem* d_bases_resident, size_t n,
                            uint8_t out_affine[64]) {
  Context& c = *g_ctx;
  const uint32_t K = host_chunk_count(g_sh.param[kRowHostChunks].load(), n);
  if (K == 1) {
    TRY(upload(c.stage_a, scalars, n * 32, c.stream));
    if (bases_host) TRY(upload(c.stage_b, bases_host, n * 64, c.stream));
    const hipError_t e = c.msm.run(reinterpret_cast<const fp_words*>(c.stage_a.p),
                                   bases_host ? reinterpret_cast<const g1_affine_mem*>(c.stage_b.p) : d_bases_resident, n, c.stream, out_affine, nullptr);
    if (e != hipSuccess) return hip_fail("msm", e);
    return SG_OK;
  }
  hipError_t e = c.stage_a.reserve(n * 32);
  if (e == hipSuccess && bases_host) e = c.stage_b.reserve(n * 64);
  if (e != hipSuccess) return hip_fail("staging buffer", e);
  std::vector<uint8_t> part(64 * (size_t)K, 0);
  std::vector<hipEvent_t> ev_s(K, nullptr), ev_b(K, nullptr);
  struct Events {
    std::vector<hipEvent_t>&a, &b;
    ~Events() {
      for (auto v : {&a, &b})
        for (hipEvent_t x : *v)
          if (x) (void)hipEventDestroy(x);
    }
  } events_guard{ev_s, ev_b};
  for (uint32_t i = 0; i < K; i++) {
    CHECK_HIP(hipEventCreateWithFlags(&ev_s[i], hipEventDisableTiming), "event");
    if (bases_host) CHECK_HIP(hipEventCreateWithFlags(&ev_b[i], hipEventDisableTiming), "event");
  }
  struct Ops {
    Context& c;
    const uint8_t *scalars, *bases_host;
    const fp_words* d_s;
    const g1_affine_mem* d_b;
    std::vector<size_t> lo;
    std::vector<hipEvent_t>&ev_s, &ev_b;
    uint8_t* part;
    MsmEngine* eng[2];
    hipStream_t st[2], copy;
    size_t len(uint32_t i) const { return lo[i + 1] - lo[i]; }
    hipError_t copy_scalars(uint32_t i) {
      const hipError_t e = hipMemcpyAsync(c.stage_a.p + lo[i] * 32, scalars + lo[i] * 32, len(i) * 32, hipMemcpyHostToDevice, copy);
      return e == hipSuccess ? hipEventRecord(ev_s[i], copy) : e;
    }
    hipError_t copy_bases(uint32_t i) {
      if (!bases_host) return hipSuccess;
      const hipError_t e = hipMemcpyAsync(c.stage_b.p + lo[i] * 64, bases_host + lo[i] * 64, len(i) * 64, hipMemcpyHostToDevice, copy);
      return e == hipSuccess ? hipEventRecord(ev_b[i], copy) : e;
    }
    hipError_t front(uint32_t i) {
      const hipError_t e = hipStreamWaitEvent(st[i & 1], ev_s[i], 0);
      return e == hipSuccess ? eng[i & 1]->enqueue_front(d_s + lo[i], d_b + lo[i], len(i), st[i & 1], part + 64 * i, nullptr) : e;
    }
    hipError_t back(uint32_t i) {
      const hipError_t e2 = bases_host ? hipStreamWaitEvent(st[i & 1], ev_b[i], 0) : hipSuccess;
      const hipError_t e3 = eng[i & 1]->enqueue_back();    // (always: an engine left with an open job would poison the lane's next call)
      // (the wait failed but the job went out: closed here, for the driver finishes no job whose back reports a failure)
      if (e2 != hipSuccess && e3 == hipSuccess) (void)eng[i & 1]->finish();
      return e2 != hipSuccess ? e2 : e3;
    }
    hipError_t finish(uint32_t i) { return eng[i & 1]->finish(); }
  } ops{c, scalars, bases_host, reinterpret_cast<const fp_words*>(c.stage_a.p),
        bases_host ? reinterpret_cast<const g1_affine_mem*>(c.stage_b.p) : d_bases_resident, host_chunk_bounds(n, K), ev_s, ev_b, part.data(),
        {&c.msm, &c.msm_b}, {c.stream, c.bstream[0]}, c.bstream[1]};
  // the staging buffers may still be read by earlier work of the lane's stream: the other two streams start behind it
  CHECK_HIP(hipEventRecord(c.ev_in, c.stream), "event");
  CHECK_HIP(hipStreamWaitEvent(ops.st[1], c.ev_in, 0), "stream wait");
  CHECK_HIP(hipStreamWaitEvent(ops.copy, c.ev_in, 0), "stream wait");
  // every job of the call is "one of several in flight" from the start: a first accumulation launched at three waves per SIMD
  // (a job that believes it has the device to itself) would leave the second job's front end no registers to run in
  struct InFlight {
    InFlight() { msm_hold_in_flight(true); }
    ~InFlight() { msm_hold_in_flight(false); }
  } in_flight_guard;
  e = run_chunk_pipeline(K, ops);
  if (e != hipSuccess) return hip_fail("msm (host chunks)", e);
  return sg_g1_sum_affine(part.data(), K, out_affine);
}

int sg_msm_g1(const uint8_t* scalars, const uint8_t* bases, size_t n, uint8_t out_affine[64]) {
  if (!out_affine || (n && (!scalars || !bases))) return fail(SG_ERR_INVALID, "sg_msm_g1: null argument");
  LOCKED_CTX();
  if (n && n <= (size_t)g_sh.param[kRowTinyMax].load()) {   // a handful of points (the verifier's 37): one launch, no staging (MsmEngine::run_tiny)
    const hipError_t e = g_ctx->msm.run_tiny(scalars, bases, n, g_ctx->stream, out_affine);
    if (e != hipSuccess) return hip_fail("msm (one launch)", e);
    return SG_OK;
  }
  return msm_host_chunked(scalars, bases, nullptr, n, out_affine);
}

// A batch of independent MSMs (the commitments of one prover phase): two engines on two
// streams, so that MSM i's latency-bound bucket reduction overlaps MSM i+1's sort/accumulate.
// batch driver shared by sg_msm_g1_batch_dev (d_bases given) and sg_commit_batch_dev (tab given: every
// MSM runs over the precomputed window table); caller holds the context lock
static int msm_batch_locked(const void* const* d_scalars, const void* const* d_bases, const FixedTable* tab,
                            const size_t* n, size_t count, void* stream, uint8_t* out_affine, const uint8_t* diff = nullptr) {
  Context& c = *g_ctx;
  MsmEngine* eng[2] = {&c.msm, &c.msm_b};
  for (int k = 0; k < 2; k++) {
    if (!c.tstream[k]) {
      int lo = 0, hi = 0;
      (void)hipDeviceGetStreamPriorityRange(&lo, &hi);  // hi = numerically lowest = highest priority
      CHECK_HIP(hipStreamCreateWithPriority(&c.tstream[k], hipStreamNonBlocking, hi), "priority stream");
    }
    eng[k]->set_tail_stream(c.tstream[k]);
  }
  struct Restore {
    MsmEngine** e;
    ~Restore() { e[0]->set_tail_stream(nullptr); e[1]->set_tail_stream(nullptr); }
  } restore{eng};
  // inputs are ordered on the caller's stream
  CHECK_HIP(hipEventRecord(c.ev_in, pick_stream(stream)), "event");
  for (auto& bs : c.bstream) CHECK_HIP(hipStreamWaitEvent(bs, c.ev_in, 0), "stream wait");
  // consecutive MSMs of equal length are fused into one job; groups alternate between the two engines
  const std::vector<FusedGroup> groups =
      fused_groups(n, count, [&](size_t len) { return tab ? eng[0]->max_fused_fixed(*tab, len) : eng[0]->max_fused(len); });
  hipError_t e = hipSuccess;
  for (size_t gi = 0; gi < groups.size() && e == hipSuccess; gi++) {
    const int k = (int)(gi & 1);
    if (gi >= 2) {
      e = eng[k]->finish();
      if (e != hipSuccess) break;
    }
    const FusedGroup& g = groups[gi];
    if (tab) {  // d_bases then holds one window table per MSM (all with tab's plan)
      uint64_t diff_mask = 0;
      for (size_t m = 0; diff && m < g.count; m++) diff_mask |= (uint64_t)(diff[g.first + m] ? 1 : 0) << m;
      e = eng[k]->enqueue_front_fixed(reinterpret_cast<const fp_words* const*>(d_scalars + g.first), *tab, g.count,
                                      n[g.first], c.bstream[k], out_affine + 64 * g.first, nullptr,
                                      reinterpret_cast<const g1_affine_mem* const*>(d_bases + g.first), diff_mask);
    }
    else
      e = eng[k]->enqueue_front_fused(reinterpret_cast<const fp_words* const*>(d_scalars + g.first),
                                      reinterpret_cast<const g1_affine_mem* const*>(d_bases + g.first), g.count,
                                      n[g.first], c.bstream[k], out_affine + 64 * g.first, nullptr);
    if (e == hipSuccess) e = eng[k]->enqueue_back();
  }
  for (size_t gi = (groups.size() >= 2 ? groups.size() - 2 : 0); gi < groups.size() && e == hipSuccess; gi++)
    e = eng[gi & 1]->finish();
  if (e != hipSuccess) {
    (void)hipDeviceSynchronize();
    return hip_fail("msm batch", e);
  }
  return SG_OK;
}
int sg_msm_g1_batch_dev(const void* const* d_scalars, const void* const* d_bases, const size_t* n, size_t count,
                        void* stream, uint8_t* out_affine) {
  if (count && (!d_scalars || !d_bases || !n || !out_affine)) return fail(SG_ERR_INVALID, "sg_msm_g1_batch: null argument");
  for (size_t i = 0; i < count; i++) {
    if (n[i] && (!d_scalars[i] || !d_bases[i])) return fail(SG_ERR_INVALID, "sg_msm_g1_batch: null argument");
  }
  LOCKED_CTX();
  return msm_batch_locked(d_scalars, d_bases, nullptr, n, count, stream, out_affine);
}
int sg_msm_g1_batch(const uint8_t* const* scalars, const uint8_t* const* bases, const size_t* n, size_t count,
                    uint8_t* out_affine) {
  if (count && (!scalars || !bases || !n || !out_affine)) return fail(SG_ERR_INVALID, "sg_msm_g1_batch: null argument");
  std::vector<const void*> ds(count), db(count);
  LOCKED_CTX();   // held across staging AND the batch: the staging buffers are this lane's
  {
    size_t tot_s = 0, tot_b = 0;
    for (size_t i = 0; i < count; i++) { tot_s += n[i] * 32; tot_b += n[i] * 64; }
    hipError_t e = g_ctx->stage_a.reserve(tot_s + 64);
    if (e == hipSuccess) e = g_ctx->stage_b.reserve(tot_b + 64);
    if (e != hipSuccess) return hip_fail("staging buffer", e);
    size_t os = 0, ob = 0;
    for (size_t i = 0; i < count; i++) {
      if (n[i] && (!scalars[i] || !bases[i])) return fail(SG_ERR_INVALID, "sg_msm_g1_batch: null argument");
      if (n[i]) {
        CHECK_HIP(hipMemcpyAsync(g_ctx->stage_a.p + os, scalars[i], n[i] * 32, hipMemcpyHostToDevice, g_ctx->stream), "H2D copy");
        CHECK_HIP(hipMemcpyAsync(g_ctx->stage_b.p + ob, bases[i], n[i] * 64, hipMemcpyHostToDevice, g_ctx->stream), "H2D copy");
      }
      ds[i] = g_ctx->stage_a.p + os;
      db[i] = g_ctx->stage_b.p + ob;
      os += n[i] * 32;
      ob += n[i] * 64;
    }
  }
  return sg_msm_g1_batch_dev(ds.data(), db.data(), n, count, g_ctx->stream, out_affine);
}

// Sum of a handful of affine points on the host (combining the per-GPU partial results of a
// point-sharded MSM after the all_gather): a few Jacobian additions + one normalisation.
int sg_g1_sum_affine(const uint8_t* points, size_t n, uint8_t out_affine[64]) {
  if (!out_affine || (n && !points)) return fail(SG_ERR_INVALID, "sg_g1_sum_affine: null argument");
  if (n > 4096) return fail(SG_ERR_INVALID, "sg_g1_sum_affine: meant for a handful of points; use sg_msm_g1");
  using namespace sg::host;
  Jac acc = Jac::identity();
  for (size_t i = 0; i < n; i++) {
    Fq x, y;
    std::memcpy(x.v, points + 64 * i, 32);
    std::memcpy(y.v, points + 64 * i + 32, 32);
    if (x.is_zero() && y.is_zero()) continue;
    acc = jac_add(acc, Jac{x, y, Fq::one()});
  }
  jac_to_affine_bytes(acc, out_affine);
  return SG_OK;
}

int sg_srs_upload(uint32_t k, const uint8_t* g, const uint8_t* g_lagrange, uint64_t* handle_out) {
  if (!g || !g_lagrange || !handle_out || k > 28) return fail(SG_ERR_INVALID, "sg_srs_upload: bad argument");
  LOCKED_CTX();
  return srs_upload(k, g, g_lagrange, false, nullptr, handle_out, "sg_srs_upload");
}
// the same from device memory (e.g. the receive buffers of an RCCL broadcast): device-to-device copies on `stream`
int sg_srs_upload_dev(uint32_t k, const void* d_g, const void* d_g_lagrange, void* stream, uint64_t* handle_out) {
  if (!d_g || !d_g_lagrange || !handle_out || k > 28) return fail(SG_ERR_INVALID, "sg_srs_upload_dev: bad argument");
  LOCKED_CTX();
  return srs_upload(k, d_g, d_g_lagrange, true, pick_stream(stream), handle_out, "sg_srs_upload_dev");
}
// copies of the resident bases into caller-owned device buffers (2^k x 64 B each; either may be NULL)
int sg_srs_copy_dev(uint64_t handle, void* d_g_out, void* d_g_lagrange_out, void* stream) {
  LOCKED_CTX();
  Srs srs_v;
  if (!find_srs(handle, &srs_v)) return fail(SG_ERR_INVALID, "unknown SRS handle");
  const size_t bytes = (size_t)64 << srs_v.k;
  hipStream_t st = pick_stream(stream);
  if (d_g_out) CHECK_HIP(hipMemcpyAsync(d_g_out, srs_v.g, bytes, hipMemcpyDeviceToDevice, st), "sg_srs_copy_dev");
  if (d_g_lagrange_out) CHECK_HIP(hipMemcpyAsync(d_g_lagrange_out, srs_v.g_lagrange, bytes, hipMemcpyDeviceToDevice, st), "sg_srs_copy_dev");
  return SG_OK;
}
// `SerdeFormat::RawBytes` validation of ParamsKZG::read (halo2: from_raw_bytes rejects points off the curve; the
// `RawBytesUnchecked` format skips this): *bad_out = number of points of the resident SRS that fail y^2 = x^3 + 3
int sg_srs_check(uint64_t handle, uint64_t* bad_out) {
  if (!bad_out) return fail(SG_ERR_INVALID, "sg_srs_check: null argument");
  LOCKED_CTX();
  Srs srs;
  if (!find_srs(handle, &srs)) return fail(SG_ERR_INVALID, "unknown SRS handle");
  uint8_t* cnt = nullptr;
  hipStream_t s = g_ctx->stream;
  hipError_t e = scratch_for(s, 7, 64, &cnt);
  uint32_t h[2] = {0, 0};
  const size_t n = (size_t)1 << srs.k;
  for (int b = 0; b < 2 && e == hipSuccess; b++) {
    e = g1_on_curve(b ? srs.g_lagrange : srs.g, n, reinterpret_cast<uint32_t*>(cnt), s);
    if (e == hipSuccess) e = host_copy_d2h(&h[b], cnt, 4, s);
  }
  if (e != hipSuccess) return hip_fail("sg_srs_check", e);
  *bad_out = (uint64_t)h[0] + h[1];
  return SG_OK;
}
int sg_srs_free(uint64_t handle) {
  LOCKED_CTX();
  Srs gone;
  {
    std::lock_guard<std::mutex> lk(g_sh.mu);
    auto it = g_sh.srs.find(handle);
    if (it == g_sh.srs.end()) return fail(SG_ERR_INVALID, "sg_srs_free: unknown handle");
    gone = it->second;
    g_sh.srs.erase(it);
  }
  (void)hipFree(gone.g);          // hipFree waits for the device: work in flight on these bases completes first
  (void)hipFree(gone.g_lagrange);
  if (gone.lagrange_prefix) (void)hipFree(gone.lagrange_prefix);
  for (auto& t : gone.tab)
    if (t.table) (void)hipFree(t.table);
  return SG_OK;
}
// Precompute the fixed-base window table of one basis: W x 2^k points, row w = 2^(offset_w) * basis.
// Later sg_commit* calls on this basis take the fixed-base path (same result bits).
int sg_srs_precompute(uint64_t handle, int basis, uint32_t window_bits) {
  if (basis < 0 || basis > 2) return fail(SG_ERR_INVALID, "sg_srs_precompute: bad basis");
  if (window_bits && (window_bits < 4 || window_bits > 16)) return fail(SG_ERR_INVALID, "sg_srs_precompute: window_bits in [4, 16]");
  LOCKED_CTX();
  Srs s;   // a copy: the entry itself is updated under the lock once the table exists
  if (!find_srs(handle, &s)) return fail(SG_ERR_INVALID, "unknown SRS handle");
  const size_t n = (size_t)1 << s.k;
  const uint32_t c = window_bits ? window_bits : fixed_window_bits_for(n);
  hipError_t e = hipSuccess;
  g1_affine_mem* new_prefix = nullptr;
  if (basis == 2 && !s.lagrange_prefix) {   // Q_i = L_0 + ... + L_i, once per SRS
    g1_affine_mem* q = nullptr;
    e = hipMalloc(&q, n * sizeof(g1_affine_mem));
    if (e == hipSuccess) e = g1_prefix_sums(s.g_lagrange, n, q, g_ctx->stream);
    if (e != hipSuccess) {
      if (q) (void)hipFree(q);
      return hip_fail("sg_srs_precompute: prefix sums", e);
    }
    s.lagrange_prefix = new_prefix = q;
  }
  FixedTable t;
  e = build_window_table(basis == 2 ? s.lagrange_prefix : basis ? s.g_lagrange : s.g, n, c, &t, g_ctx->stream);
  if (e == hipSuccess) e = host_wait_stream(g_ctx->stream);
  if (e != hipSuccess) {
    if (new_prefix) (void)hipFree(new_prefix);
    return hip_fail("sg_srs_precompute", e);
  }
  {
    std::lock_guard<std::mutex> lk(g_sh.mu);
    auto it = g_sh.srs.find(handle);
    if (it == g_sh.srs.end()) {   // freed by another thread meanwhile
      retire_device_memory(t.table);
      retire_device_memory(new_prefix);
      return fail(SG_ERR_INVALID, "sg_srs_precompute: the handle was freed during the call");
    }
    if (new_prefix) {
      if (it->second.lagrange_prefix) retire_device_memory(new_prefix);   // two concurrent precomputes: keep the first
      else it->second.lagrange_prefix = new_prefix;
    }
    retire_device_memory(it->second.tab[basis].table);   // commitments of other lanes may still be reading the old table
    it->second.tab[basis] = t;
  }
  return SG_OK;
}
int sg_srs_device_ptrs(uint64_t handle, const void** d_g, const void** d_g_lagrange, uint32_t* k) {
  LOCKED_CTX();
  Srs srs;
  if (!find_srs(handle, &srs)) return fail(SG_ERR_INVALID, "unknown SRS handle");
  if (d_g) *d_g = srs.g;
  if (d_g_lagrange) *d_g_lagrange = srs.g_lagrange;
  if (k) *k = srs.k;
  return SG_OK;
}
// one commitment against the basis and table resolve_basis (commit_plan.h) names
static hipError_t commit_run(const Srs& s, int basis, const fp_words* d_scalars, size_t n, hipStream_t stream,
                             uint8_t out_affine[64], MsmTimings* tm = nullptr) {
  MsmEngine& eng = g_ctx->msm;
  const BasisChoice ch = resolve_basis(tables_of(s), basis, n);
  if (ch.fixed && n) {
    const fp_words* sc[1] = {d_scalars};
    hipError_t e = eng.enqueue_front_fixed(sc, s.tab[ch.table], 1, n, stream, out_affine, tm, nullptr, ch.diff ? 1u : 0u);
    if (e == hipSuccess) e = eng.enqueue_back();
    if (e == hipSuccess) e = eng.finish();
    return e;
  }
  return eng.run(d_scalars, ch.basis ? s.g_lagrange : s.g, n, stream, out_affine, tm);
}
int sg_commit_dev_timed(uint64_t srs_handle, int basis, const void* d_scalars, size_t n, void* stream,
                        uint8_t out_affine[64], sg_msm_timings* timings) {
  if (!out_affine || (n && !d_scalars) || basis < 0 || basis > 2) return fail(SG_ERR_INVALID, "sg_commit: bad argument");
  LOCKED_CTX();
  Srs s;
  TRY(srs_for_commit(srs_handle, n, &s));
  MsmTimings tm;
  hipError_t e = commit_run(s, basis, static_cast<const fp_words*>(d_scalars), n, pick_stream(stream), out_affine,
                            timings ? &tm : nullptr);
  if (e != hipSuccess) return hip_fail("msm", e);
  report_timings(timings, tm);
  return SG_OK;
}
int sg_commit_dev(uint64_t srs_handle, int basis, const void* d_scalars, size_t n, void* stream,
                  uint8_t out_affine[64]) {
  return sg_commit_dev_timed(srs_handle, basis, d_scalars, n, stream, out_affine, nullptr);
}
// `count` commitments of equal length against one basis as fused jobs (the advice / quotient-piece
// commitments of one proof phase); takes the fixed-base path when the table exists
int sg_commit_batch_dev(uint64_t srs_handle, int basis, const void* const* d_scalars, size_t count, size_t n,
                        void* stream, uint8_t* out_affine) {
  if ((count && (!d_scalars || !out_affine)) || basis < 0 || basis > 2) return fail(SG_ERR_INVALID, "sg_commit_batch: bad argument");
  for (size_t i = 0; i < count; i++)
    if (n && !d_scalars[i]) return fail(SG_ERR_INVALID, "sg_commit_batch: null argument");
  LOCKED_CTX();
  Srs s;
  TRY(srs_for_commit(srs_handle, n, &s));
  std::vector<size_t> ns(count, n);
  const BasisChoice ch = resolve_basis(tables_of(s), basis, n);
  std::vector<const void*> bases(count, ch.fixed ? (const void*)s.tab[ch.table].table : (const void*)(ch.basis ? s.g_lagrange : s.g));
  std::vector<uint8_t> flags(count, ch.diff ? 1 : 0);
  return msm_batch_locked(d_scalars, bases.data(), ch.fixed ? &s.tab[ch.table] : nullptr, ns.data(), count, stream, out_affine, flags.data());
}
// ---- commit combiner (commit_combiner.h): what it needs of the device and of this library
Combiner g_comb;
thread_local bool t_combine = false;
thread_local hipEvent_t t_ready = nullptr;

static int commit_batch_mixed_core(uint64_t srs_handle, const int* basis, const void* const* d_scalars, size_t count, size_t n,
                                   void* stream, uint8_t* out_affine);

// the members of `job` as one job on a lane of its own, whose stream waits for every member's inputs
static int combiner_run_job(const CommitJob& job, char err[sizeof(CommitReq::err)]) {
  int rc;
  {
    LaneHold hold;
    rc = hold.rc;
    for (size_t m = 0; m < job.n_members && rc == SG_OK; m++) {
      const hipError_t e = hipStreamWaitEvent(g_ctx->stream, static_cast<hipEvent_t>(job.members[m]->ready), 0);
      if (e != hipSuccess) rc = hip_fail("commit combiner: stream wait", e);
    }
    if (rc == SG_OK) rc = commit_batch_mixed_core(job.srs, job.basis, job.scalars, job.polys, job.n, g_ctx->stream, job.out);
  }
  if (rc != SG_OK) std::snprintf(err, sizeof(CommitReq::err), "%s", g_err);
  return rc;
}
static int commit_combined(uint64_t srs_handle, const int* basis, const void* const* d_scalars, size_t count, size_t n,
                           void* stream, uint8_t* out_affine) {
  if (!t_ready) CHECK_HIP(hipEventCreateWithFlags(&t_ready, hipEventDisableTiming), "event");
  CHECK_HIP(hipEventRecord(t_ready, pick_stream(stream)), "event");
  CommitReq req{srs_handle, n, count, basis, d_scalars, out_affine, t_ready};
  const int rc = g_comb.submit(
      req, combiner_run_job,
      [](CombinerKnob k) {
        return g_sh.param[k == CombinerKnob::runners ? kRowCombineRunners : k == CombinerKnob::wait_us ? kRowCombineWaitUs : kRowCombineTarget].load();
      },
      [] { return g_sh.param[kRowFailNextFusedJob].exchange(0) != 0; });
  if (rc != SG_OK) std::snprintf(g_err, sizeof g_err, "%s", req.err);
  return rc;
}

int sg_commit_combine_begin(void) {
  if (t_combine) return SG_OK;
  t_combine = true;
  g_comb.join();
  return SG_OK;
}
int sg_commit_combine_end(void) {
  if (!t_combine) return SG_OK;
  t_combine = false;
  g_comb.leave();
  if (t_ready) {                     // this thread's requests have all returned: nothing waits on the event any more
    (void)hipEventDestroy(t_ready);
    t_ready = nullptr;
  }
  return SG_OK;
}
int sg_commit_combining(void) { return t_combine ? 1 : 0; }
int sg_commit_combine_stats(uint64_t* jobs, uint64_t* requests) {
  if (jobs) *jobs = g_comb.jobs.load();
  if (requests) *requests = g_comb.requests.load();
  return SG_OK;
}

// sg_commit_batch_dev with one basis per polynomial (0 = g, 1 = g_lagrange): e.g. the grand-product commitments (Lagrange)
// and the random polynomial (coefficients) of one prover phase as ONE fused job
int sg_commit_batch_mixed_dev(uint64_t srs_handle, const int* basis, const void* const* d_scalars, size_t count, size_t n,
                              void* stream, uint8_t* out_affine) {
  if (count && (!d_scalars || !out_affine || !basis)) return fail(SG_ERR_INVALID, "sg_commit_batch_mixed: bad argument");
  for (size_t i = 0; i < count; i++)
    if ((n && !d_scalars[i]) || basis[i] < 0 || (basis[i] & ~SG_BASIS_SPARSE) > 2) return fail(SG_ERR_INVALID, "sg_commit_batch_mixed: bad argument");
  if (t_combine && count && n && count <= MAX_FUSED && g_depth == 0)
    return commit_combined(srs_handle, basis, d_scalars, count, n, stream, out_affine);
  return commit_batch_mixed_core(srs_handle, basis, d_scalars, count, n, stream, out_affine);
}
static int commit_batch_mixed_core(uint64_t srs_handle, const int* basis, const void* const* d_scalars, size_t count, size_t n,
                                   void* stream, uint8_t* out_affine) {
  LOCKED_CTX();
  Srs s;
  TRY(srs_for_commit(srs_handle, n, &s));
  const MixedChoice m = resolve_mixed(tables_of(s), basis, count, n);
  std::vector<size_t> ns(count, n);
  std::vector<const void*> bases(count);
  for (size_t i = 0; i < count; i++) bases[i] = m.fixed ? (const void*)s.tab[m.b[i]].table : (const void*)(m.b[i] ? s.g_lagrange : s.g);
  // the task length of a small all-sparse job (sparse_hint_applies), for this job only
  struct SegRestore {
    Context& c;
    uint32_t seg;
    ~SegRestore() { msm_set(c, &MsmConfig::log_seg, (int)seg); }
  } seg_restore{*g_ctx, g_ctx->msm.config().log_seg};
  if (sparse_hint_applies(m.all_sparse, m.fixed, count, g_ctx->msm.config().log_seg, n)) msm_set(*g_ctx, &MsmConfig::log_seg, 3);
  return msm_batch_locked(d_scalars, bases.data(), m.fixed ? &s.tab[0] : nullptr, ns.data(), count, stream, out_affine, m.flags.data());
}
int sg_commit(uint64_t srs_handle, int basis, const uint8_t* scalars, size_t n, uint8_t out_affine[64]) {
  if (!out_affine || (n && !scalars) || basis < 0 || basis > 2) return fail(SG_ERR_INVALID, "sg_commit: bad argument");
  LOCKED_CTX();
  Srs sr;
  TRY(srs_for_commit(srs_handle, n, &sr));
  const SrsTables t = tables_of(sr);
  if (commit_goes_in_chunks(t, basis, n))
    return msm_host_chunked(scalars, nullptr, resolve_basis(t, basis, n).basis ? sr.g_lagrange : sr.g, n, out_affine);
  TRY(upload(g_ctx->stage_a, scalars, n * 32, g_ctx->stream));
  hipError_t e = commit_run(sr, basis, reinterpret_cast<const fp_words*>(g_ctx->stage_a.p), n, g_ctx->stream, out_affine);
  if (e != hipSuccess) return hip_fail("msm", e);
  return SG_OK;
}

// ------------------------------------------------------------------ many small MSMs in one launch, sums over ranges of them
int sg_msm_g1_many_begin(const uint8_t* scalars, const uint8_t* bases, const uint32_t* first, uint32_t jobs, uint64_t* handle) {
  if (!first || !handle) return fail(SG_ERR_INVALID, "sg_msm_g1_many_begin: null argument");
  if (jobs > MSM_MANY_MAX_JOBS) return fail(SG_ERR_INVALID, "sg_msm_g1_many_begin: more than 2^14 jobs");
  for (uint32_t i = 0; i < jobs; i++) {
    if (first[i + 1] < first[i]) return fail(SG_ERR_INVALID, "sg_msm_g1_many_begin: `first` decreases");
    if (first[i + 1] - first[i] > MSM_TINY_MAX) return fail(SG_ERR_INVALID, "sg_msm_g1_many_begin: a job of more than 64 points");
  }
  const size_t n = first[jobs];   // the jobs index scalars / bases from their start
  if (n > first[0] && (!scalars || !bases)) return fail(SG_ERR_INVALID, "sg_msm_g1_many_begin: null argument");
  LOCKED_CTX();
  Context& c = *g_ctx;
  TRY(upload(c.stage_a, scalars, n > first[0] ? n * 32 : 0, c.stream));
  TRY(upload(c.stage_b, bases, n > first[0] ? n * 64 : 0, c.stream));
  uint8_t* d_first = nullptr;
  CHECK_HIP(scratch_for(c.stream, 10, ((size_t)jobs + 1) * sizeof(uint32_t), &d_first), "sg_msm_g1_many_begin: scratch");
  CHECK_HIP(hipMemcpyAsync(d_first, first, ((size_t)jobs + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream), "H2D copy");
  ManyJobs m{jobs, nullptr};
  const size_t bytes = std::max<size_t>(jobs, 1) * MSM_MANY_JOB_WORDS * sizeof(uint32_t);
  hipError_t e = hipMalloc(&m.S, bytes);
  if (e != hipSuccess) {   // out of memory: give the retired blocks back and try once more (DevBuf::reserve)
    retired_device_memory_collect();
    e = hipMalloc(&m.S, bytes);
  }
  if (e != hipSuccess) return hip_fail("sg_msm_g1_many_begin: window sums", e);
  e = msm_many_launch(reinterpret_cast<const fp_words*>(c.stage_a.p), reinterpret_cast<const g1_affine_mem*>(c.stage_b.p),
                      reinterpret_cast<const uint32_t*>(d_first), jobs, m.S, c.stream);
  // the sums may be asked for from any lane: S is complete (and the staging buffers free again) on return
  if (e == hipSuccess) e = host_wait_stream(c.stream);
  if (e != hipSuccess) {
    (void)hipFree(m.S);
    return hip_fail("sg_msm_g1_many_begin", e);
  }
  std::lock_guard<std::mutex> lk(g_sh.mu);
  *handle = g_sh.next_handle++;
  g_sh.many[*handle] = m;
  return SG_OK;
}
int sg_msm_g1_many_sums(uint64_t handle, const uint32_t* ranges, uint32_t count, uint8_t* out_affine) {
  if (count > MSM_MANY_MAX_RANGES) return fail(SG_ERR_INVALID, "sg_msm_g1_many_sums: more than 8 ranges");
  if (count && (!ranges || !out_affine)) return fail(SG_ERR_INVALID, "sg_msm_g1_many_sums: null argument");
  for (uint32_t r = 0; r < count; r++)
    if (ranges[2 * r] > ranges[2 * r + 1]) return fail(SG_ERR_INVALID, "sg_msm_g1_many_sums: a range that ends before it starts");
  LOCKED_CTX();
  ManyJobs m;
  if (!find_many(handle, &m)) return fail(SG_ERR_INVALID, "sg_msm_g1_many_sums: unknown handle");
  ManyRanges rg{};
  for (uint32_t r = 0; r < count; r++) {
    if (ranges[2 * r + 1] > m.jobs) return fail(SG_ERR_INVALID, "sg_msm_g1_many_sums: a range beyond the last job");
    rg.v[2 * r] = ranges[2 * r];
    rg.v[2 * r + 1] = ranges[2 * r + 1];
  }
  if (count == 0) return SG_OK;
  Context& c = *g_ctx;
  if (!c.h_many) {
    CHECK_HIP(hipHostMalloc(reinterpret_cast<void**>(&c.h_many), MSM_MANY_MAX_RANGES * MSM_MANY_JOB_WORDS * sizeof(uint32_t),
                            hipHostMallocMapped | hipHostMallocCoherent), "sg_msm_g1_many_sums: mapped host memory");
    CHECK_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&c.d_many), c.h_many, 0), "sg_msm_g1_many_sums: mapped host memory");
  }
  // (the buffer is this lane's, and the previous call waited for its kernel: nothing reads it now)
  CHECK_HIP(msm_many_sum_launch(m.S, rg, count, c.d_many, c.stream), "sg_msm_g1_many_sums");
  CHECK_HIP(host_wait_stream(c.stream), "sg_msm_g1_many_sums");
  const WindowPlan wp = make_window_plan(4);
  for (uint32_t r = 0; r < count; r++) msm_window_sums_to_affine(wp, c.h_many + r * MSM_MANY_JOB_WORDS, out_affine + 64 * (size_t)r);
  return SG_OK;
}
int sg_msm_g1_many_end(uint64_t handle) {
  LOCKED_CTX();
  ManyJobs gone;
  if (!find_many(handle, &gone, true)) return fail(SG_ERR_INVALID, "sg_msm_g1_many_end: unknown handle");
  // freed, not retired (as sg_srs_free does): a verifier that runs for days would otherwise pile up 16 KB per proof; begin and every
  // sums call waited for their kernels, so nothing reads S now
  (void)hipFree(gone.S);
  return SG_OK;
}

int sg_msm_launch_log(uint32_t* out_words, size_t cap_records, size_t* n_records) {
  if (!n_records || (cap_records && !out_words)) return fail(SG_ERR_INVALID, "sg_msm_launch_log: bad argument");
  static_assert(sizeof(AccLaunchRecord) == 8 * sizeof(uint32_t), "record layout is part of the ABI");
  *n_records = msm_acc_log_read(reinterpret_cast<AccLaunchRecord*>(out_words), cap_records);
  return SG_OK;
}

}  // extern "C"
