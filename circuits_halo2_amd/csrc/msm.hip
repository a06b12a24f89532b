// Pippenger bucket MSM over BN254 G1 for gfx950 -- the GPU side of halo2's `best_multiexp`
// (reached through ParamsKZG::commit / commit_lagrange from the reference's
// zk_prover/src/circuits/utils.rs:75,76,94-101,171-178).
//
//   result = sum_i s_i * P_i,  s_i: 32-B Montgomery Fr, P_i: 64-B affine Montgomery points.
//
// Pipeline (all on one stream; one host read-back of three counters to size the launches):
//   1 msm_digits      scalars -> canonical -> W signed c-bit digits (int16 rows, one per window)
//   2 msm_hist        LDS-staged window buckets: workgroup (chunk p, window j) histograms its
//                     chunk's digits in LDS (2^(c-1) counters, up to 128 KiB); zero digits are
//                     skipped, as in halo2
//     msm_hist_prefix per-bucket prefix over chunks -> bucket counts
//   3 msm_scan_*      exclusive scans: bucket offsets and task offsets (a task = <= L
//                     consecutive entries of one bucket, so heavy buckets are split)
//     msm_scatter     counting sort of the point indices by (window, bucket); slots are handed
//                     out by LDS atomics on per-workgroup cursors (no global atomics in the sort)
//   4 msm_accumulate  one lane per task: XYZZ accumulator += affine points (8M+2S each); persistent waves that
//                     take tickets of 64 tasks from one global counter
//     msm_merge       (only when a bucket had > L entries) same over partial sums
//   5 msm_reduce_*    sum_b b*B_b per window: per-thread running sums over G buckets, then a
//                     workgroup-wide suffix scan + tree reduction in LDS; repeated per level
//   6 host            Horner over the W window sums (c doublings each) + affine normalisation
//
// Signed digits halve the bucket count: digit d in [-2^(c-1), 2^(c-1)], bucket |d|, the point
// is negated on the fly when d < 0.  The group law is commutative, so the order in which a
// bucket's points are added (LDS atomics make it non-deterministic) never changes the result bits.
//
// This file is the host engine: plan (msm_plan.h), reserve, launch.  The kernels are in msm_sort.cuh, msm_accumulate.cuh and
// msm_reduce.cuh, included below into this one translation unit.
#include "msm.h"
#include "side_prio.cuh"
#include "host_wait.h"

#include <algorithm>
#include <atomic>
#include <functional>
#include <mutex>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_curve.h"

#include "msm_sort.cuh"
#include "msm_accumulate.cuh"
#include "msm_reduce.cuh"

namespace sg {
SG_DEFINE_SIDE_PRIO_SETTER(msm_set_side_prio)

// ------------------------------------------------------------------ host driver
MsmEngine::~MsmEngine() { release(); }

// Accumulations of different jobs never share the device: each one alone keeps the vector ALUs busy, and two polite ones
// side by side fill the register file that politeness leaves to the other kernels.  Every accumulation launch waits for
// the event recorded after the previous one (whichever engine / stream launched it).
// (process-wide state: the library serves ONE device per process -- sg_init binds it, one process per GPU -- so "of the
// process" is "of the device")
static std::mutex g_acc_chain_mu;
static std::atomic<int> g_jobs_in_flight{0};   // jobs of this process between their first kernel and the end of their host tail
static hipEvent_t g_acc_chain_last = nullptr;   // recorded after the most recent accumulation launch of the process
// wait for the previous accumulation, launch, record -- under ONE hold of the mutex: taken separately around the launch, two
// lanes could both wait on the same predecessor and then run their accumulations side by side, which is what the chain is for
// Launch log (parameter "msm.acc_log", profiling only): one record per msm_accumulate launch, appended under the chain's mutex,
// i.e. in the order in which the chained launches run on the device -- the i-th msm_accumulate of a kernel trace ordered by
// start time IS the i-th record, so a profile attributes every launch to its job exactly (tools/proof_budget.py)
static std::atomic<int> g_acc_log_on{0};
static std::vector<AccLaunchRecord> g_acc_log;
void msm_acc_log_enable(bool on) {
  std::lock_guard<std::mutex> lk(g_acc_chain_mu);
  g_acc_log_on.store(on ? 1 : 0);
  if (on) g_acc_log.clear();
}
size_t msm_acc_log_read(AccLaunchRecord* out, size_t cap) {
  std::lock_guard<std::mutex> lk(g_acc_chain_mu);
  const size_t m = std::min(cap, g_acc_log.size());
  if (out && m) std::memcpy(out, g_acc_log.data(), m * sizeof(AccLaunchRecord));
  return g_acc_log.size();
}
hipError_t MsmEngine::chained_accumulate(hipStream_t stream, hipEvent_t after_wait, const std::function<void()>& launch) {
  std::unique_lock<std::mutex> lk(g_acc_chain_mu, std::defer_lock);
  if (cfg_.acc_chain || g_acc_log_on.load()) lk.lock();
  if (cfg_.acc_chain) {
    if (g_acc_chain_last) SG_TRY(hipStreamWaitEvent(stream, g_acc_chain_last, 0));
  }
  if (g_acc_log_on.load()) {
    const Job& j = job_;
    g_acc_log.push_back(AccLaunchRecord{(uint64_t)j.f.entries, (uint32_t)j.f.n, j.f.M, j.a.total_threads(), j.f.fixed ? 1u : 0u,
                                        (uint32_t)g_jobs_in_flight.load(), 1u << j.f.log_L});
  }
  if (after_wait) SG_TRY(hipEventRecord(after_wait, stream));   // timing mode: the accumulation's own start, behind the chain wait
  launch();
  SG_TRY(hipGetLastError());
  if (cfg_.acc_chain) {
    // two events per engine, alternating: the previous record of this engine may still be the one another stream waits on
    chain_slot_ ^= 1;
    if (!ev_chain_[chain_slot_]) SG_TRY(hipEventCreateWithFlags(&ev_chain_[chain_slot_], hipEventDisableTiming));
    SG_TRY(hipEventRecord(ev_chain_[chain_slot_], stream));
    g_acc_chain_last = ev_chain_[chain_slot_];
  }
  return hipSuccess;
}
void MsmEngine::release() {
  mark_in_flight(false);
  {
    std::lock_guard<std::mutex> lk(g_acc_chain_mu);
    for (auto& e : ev_chain_) {
      if (e && g_acc_chain_last == e) g_acc_chain_last = nullptr;
      if (e) (void)hipEventDestroy(e);
      e = nullptr;
    }
  }
  for (DevBuf<uint32_t>* b : {&fe_, &tbase_, &part_entry_, &ccnt_, &coff_, &thist_, &sorted_, &counts_, &off_, &hist_, &bsum_, &meta_,
                              &ntask_[0], &ntask_[1], &toff_[0], &toff_[1]})
    b->release();
  for (DevBuf<xyzz29_mem>* b : {&partial_[0], &partial_[1], &red_a_[0], &red_a_[1], &red_s_[0], &red_s_[1], &red_r_[0], &red_r_[1]})
    b->release();
  trace_.release();
  part_fine_.release();
  dig_.release();
  order_.release();
  for (hipEvent_t* e : {&ev_acc_, &ev_meta_, &ev_done_, &ev_tiny_}) {
    if (*e) (void)hipEventDestroy(*e);
    *e = nullptr;
  }
  if (h_meta_) (void)hipHostFree(h_meta_);
  if (h_win_) (void)hipHostFree(h_win_);
  if (h_tiny_) (void)hipHostFree(h_tiny_);
  h_meta_ = nullptr;
  h_win_ = nullptr;
  h_tiny_ = d_tiny_ = nullptr;
}

uint32_t MsmEngine::window_bits_for(size_t n, bool fused) const { return sg::window_bits_for(cfg_, n, fused); }
size_t MsmEngine::max_fused(size_t n) const { return sg::max_fused(cfg_, n); }
size_t MsmEngine::max_fused_fixed(const FixedTable& tab, size_t n) const { return sg::max_fused_fixed(cfg_, tab.c, tab.wp.W, n); }

hipError_t MsmEngine::init() {
  {
    int dev = 0, cus = 0;
    SG_TRY(hipGetDevice(&dev));
    SG_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    cus_ = cus > 0 ? (uint32_t)cus : 256u;
  }
  SG_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(msm_reduce_buckets<1>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024));
  SG_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(msm_reduce_buckets_lean<1>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024));
  SG_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(msm_reduce_items<1>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, 112 * 1024));
  SG_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(msm_hist), hipFuncAttributeMaxDynamicSharedMemorySize,
                             128 * 1024));
  SG_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(msm_scatter), hipFuncAttributeMaxDynamicSharedMemorySize,
                             128 * 1024));
  SG_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(msm_partition), hipFuncAttributeMaxDynamicSharedMemorySize,
                             96 * 1024));
  SG_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(msm_fine_sort), hipFuncAttributeMaxDynamicSharedMemorySize,
                             128 * 1024));
  SG_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(msm_fine_sort_fused), hipFuncAttributeMaxDynamicSharedMemorySize,
                             128 * 1024));
  return hipSuccess;
}

// ---- phase 1: everything up to the counting sort; ends with an async copy of the counters
hipError_t MsmEngine::enqueue_front_fixed(const fp_words* const* d_scalars, const FixedTable& tab, size_t M, size_t n,
                                          hipStream_t stream, uint8_t* out_affine, MsmTimings* tm,
                                          const g1_affine_mem* const* tables, uint64_t diff_mask) {
  if (n > tab.n || !tab.table) return hipErrorInvalidValue;
  if (diff_mask && n != tab.n) return hipErrorInvalidValue;   // s[n] = 0 closes the telescoping sum only at full length
  const g1_affine_mem* bs[MAX_FUSED];
  // `tables` (optional): one window table per MSM, all built with tab's plan (same c and n), e.g. g and g_lagrange
  for (size_t m = 0; m < M && m < MAX_FUSED; m++) bs[m] = tables ? tables[m] : tab.table;
  return enqueue_front_job(d_scalars, bs, M, n, stream, out_affine, tm, &tab, diff_mask);
}

hipError_t MsmEngine::enqueue_front(const fp_words* d_scalars, const g1_affine_mem* d_bases, size_t n,
                                    hipStream_t stream, uint8_t* out_affine, MsmTimings* tm) {
  const fp_words* sc[1] = {d_scalars};
  const g1_affine_mem* bs[1] = {d_bases};
  return enqueue_front_fused(sc, bs, 1, n, stream, out_affine, tm);
}

// M independent MSMs of the same length n as ONE job: every kernel covers M*W windows, so the
// latency-bound phases (scans, bucket reduction, host round trips) are paid once per batch
hipError_t MsmEngine::enqueue_front_fused(const fp_words* const* d_scalars, const g1_affine_mem* const* d_bases,
                                          size_t M, size_t n, hipStream_t stream, uint8_t* out_affine,
                                          MsmTimings* tm) {
  return enqueue_front_job(d_scalars, d_bases, M, n, stream, out_affine, tm, nullptr, 0);
}
hipError_t MsmEngine::enqueue_front_job(const fp_words* const* d_scalars, const g1_affine_mem* const* d_bases, size_t M,
                                        size_t n, hipStream_t stream, uint8_t* out_affine, MsmTimings* tm,
                                        const FixedTable* fixed, uint64_t diff_mask) {
  // in flight from its first kernel on: an accumulation launched while ANOTHER job is still sorting must already leave
  // room for that sort (counted from the accumulation launch only, the first accumulation after a pause took the whole
  // register file and the other callers' front-ends waited a millisecond behind it)
  mark_in_flight(true);
  const hipError_t e = enqueue_front_impl(d_scalars, d_bases, M, n, stream, out_affine, tm, fixed, diff_mask);
  if (e != hipSuccess) mark_in_flight(false);
  return e;
}
hipError_t MsmEngine::enqueue_front_impl(const fp_words* const* d_scalars, const g1_affine_mem* const* d_bases, size_t M,
                                         size_t n, hipStream_t stream, uint8_t* out_affine, MsmTimings* tm,
                                         const FixedTable* fixed, uint64_t diff_mask) {
  Job& j = job_;
  j = Job{};
  j.stream = stream; j.out = out_affine; j.tm = tm;
  if (tm) *tm = MsmTimings{};
  const FrontPlan& f = j.f = plan_front(cfg_, M, n, fixed ? &fixed->wp : nullptr, fixed ? fixed->c : 0u, fixed ? fixed->n : (size_t)0,
                                        others_in_flight());
  if (!f.valid) return hipErrorInvalidValue;
  if (f.trivial) return hipSuccess;
  for (size_t m = 0; m < M; m++) {
    j.bp.scalars[m] = d_scalars[m];
    j.bp.bases[m] = d_bases[m];
  }
  j.bp.diff_mask = diff_mask;
  SG_TRY(reserve_front(f, stream));
  if (tm) {
    for (auto& e : j.ev) SG_TRY(hipEventCreate(&e));
    SG_TRY(hipEventRecord(j.ev[0], stream));
  }
  msm_digits<<<dim3((unsigned)((n + 255) / 256), (unsigned)M), 256, 0, stream>>>(j.bp, (uint32_t)n, f.wp, dig_.p);
  if (tm) SG_TRY(hipEventRecord(j.ev[1], stream));
  SG_TRY(f.two_pass ? launch_sort_two_pass(j) : launch_sort_single(j));
  if (tm) SG_TRY(hipEventRecord(j.ev[2], stream));
  return hipGetLastError();
}

// workspace (grown on demand, kept across calls), host words and events of the front end
hipError_t MsmEngine::reserve_front(const FrontPlan& f, hipStream_t stream) {
  SG_TRY(dig_.reserve(f.entries));
  SG_TRY(sorted_.reserve(f.entries));
  SG_TRY(hist_.reserve((size_t)f.W * f.P * (f.two_pass ? f.B : f.nbw)));
  if (f.two_pass) {
    SG_TRY(part_entry_.reserve(f.entries));
    SG_TRY(part_fine_.reserve(f.entries));
    SG_TRY(ccnt_.reserve((size_t)f.sets * f.B + 1));
    SG_TRY(coff_.reserve((size_t)f.sets * f.B + 1));
  }
  SG_TRY(bsum_.reserve(3 * 1024));
  SG_TRY(counts_.reserve((size_t)f.NB + 1));
  SG_TRY(off_.reserve((size_t)f.NB + 1));
  for (int i = 0; i < 2; i++) {
    SG_TRY(ntask_[i].reserve((size_t)f.NB + 1));
    SG_TRY(toff_[i].reserve((size_t)f.NB + 1));
  }
  {
    const uint32_t* before = meta_.p;
    SG_TRY(meta_.reserve(META_WORDS));
    if (meta_.p != before) SG_TRY(hipMemsetAsync(meta_.p, 0, META_WORDS * sizeof(uint32_t), stream));   // SCAN_DONE starts at zero (msm_scan_sums keeps it there)
  }
  if (f.fe) {
    const uint32_t* before = fe_.p;
    SG_TRY(fe_.reserve(FE_WORDS));
    if (fe_.p != before) SG_TRY(hipMemsetAsync(fe_.p, 0, fe_.cap * sizeof(uint32_t), stream));   // counters and histogram start at zero; every job leaves them there
    SG_TRY(tbase_.reserve((size_t)f.NBc + 1));
  }
  // the counters and the window sums reach the host through page-locked memory the kernels write directly (mapped,
  // coherent): no copy kernels between the producing kernel and the event the host waits for
  if (!h_meta_) {
    SG_TRY(hipHostMalloc(&h_meta_, META_WORDS * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent));
    SG_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_hmeta_), h_meta_, 0));
  }
  if (h_win_cap_ < f.hwin_words) {
    if (h_win_) (void)hipHostFree(h_win_);   // (the previous job has finished: finish() waited for its event)
    h_win_ = nullptr;
    SG_TRY(hipHostMalloc(&h_win_, f.hwin_words * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent));
    SG_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_hwin_), h_win_, 0));
    h_win_cap_ = f.hwin_words;
  }
  if (!ev_meta_) SG_TRY(hipEventCreateWithFlags(&ev_meta_, hipEventDisableTiming));
  if (!ev_done_) SG_TRY(hipEventCreateWithFlags(&ev_done_, hipEventDisableTiming));
  return hipSuccess;
}

hipError_t MsmEngine::launch_sort_two_pass(Job& j) {
  const FrontPlan& f = j.f;
  hipStream_t stream = j.stream;
  const uint32_t n = (uint32_t)f.n, B = f.B, NBc = f.NBc, collapse_W = f.fixed ? f.W1 : 0u;
  FrontEndScan fe_scan{nullptr, nullptr, nullptr, 0u, 0u};
  if (f.fe) fe_scan = FrontEndScan{fe_.p + FE_HP_DONE, coff_.p, tbase_.p, 1u << f.shift, f.log_L};
  msm_hist<<<dim3(f.W, f.P), 1024, B * sizeof(uint32_t), stream>>>(dig_.p, n, f.chunk, B, f.shift, hist_.p);
  msm_hist_prefix<<<(NBc + HP_BUCKETS - 1) / HP_BUCKETS, HP_BUCKETS * HP_GROUPS, 0, stream>>>(
      hist_.p, f.fixed ? f.W1 * f.P : f.P, B, NBc, ccnt_.p, fe_scan);
  // bin offsets (the task outputs of this scan are scratch)
  if (!f.fe) SG_TRY(launch_scan(ccnt_.p, NBc, f.log_L, coff_.p, ntask_[1].p, toff_[1].p, bsum_.p, meta_.p, stream));
  msm_partition<<<dim3(f.W, f.P), 1024, (3 * B + SORT_TILE) * sizeof(uint32_t) + SORT_TILE * sizeof(uint16_t), stream>>>(
      dig_.p, n, f.chunk, B, f.shift, hist_.p, coff_.p, collapse_W, f.n_tab, part_entry_.p, part_fine_.p);
  const uint32_t F = 1u << f.shift, fs_threads = 512;
  if (f.fe) {
    fe_parity_ ^= 1u;
    j.fe_parity = fe_parity_;
    msm_fine_sort_fused<<<NBc, fs_threads, (2 * F + 2 * fs_threads + SORT_TILE) * sizeof(uint32_t), stream>>>(
        part_entry_.p, part_fine_.p, coff_.p, ccnt_.p, B, f.shift, f.nbw, counts_.p, sorted_.p,
        FrontEndOut{off_.p, ntask_[0].p, toff_[0].p, tbase_.p, fe_.p, f.log_L, j.fe_parity});
    return hipSuccess;   // (the totals come with the task order, enqueue_back)
  }
  msm_fine_sort<<<NBc, fs_threads, (2 * F + fs_threads + SORT_TILE) * sizeof(uint32_t), stream>>>(
      part_entry_.p, part_fine_.p, coff_.p, ccnt_.p, B, f.shift, f.nbw, counts_.p, sorted_.p);
  SG_TRY(launch_scan(counts_.p, f.NB, f.log_L, off_.p, ntask_[0].p, toff_[0].p, bsum_.p, meta_.p, stream, d_hmeta_));
  return hipEventRecord(ev_meta_, stream);
}

hipError_t MsmEngine::launch_sort_single(Job& j) {
  const FrontPlan& f = j.f;
  hipStream_t stream = j.stream;
  const uint32_t n = (uint32_t)f.n, nbw = f.nbw;
  msm_hist<<<dim3(f.W, f.P), 1024, nbw * sizeof(uint32_t), stream>>>(dig_.p, n, f.chunk, nbw, 0, hist_.p);
  msm_hist_prefix<<<(f.NB + HP_BUCKETS - 1) / HP_BUCKETS, HP_BUCKETS * HP_GROUPS, 0, stream>>>(
      hist_.p, f.fixed ? f.W1 * f.P : f.P, nbw, f.NB, counts_.p, FrontEndScan{nullptr, nullptr, nullptr, 0u, 0u});
  SG_TRY(launch_scan(counts_.p, f.NB, f.log_L, off_.p, ntask_[0].p, toff_[0].p, bsum_.p, meta_.p, stream, d_hmeta_));
  SG_TRY(hipEventRecord(ev_meta_, stream));
  msm_scatter<<<dim3(f.W, f.P, 1u << f.log_R), 1024, (nbw >> f.log_R) * sizeof(uint32_t), stream>>>(
      dig_.p, n, f.chunk, nbw, hist_.p, off_.p, f.fixed ? f.W1 : 0u, f.n_tab, sorted_.p);
  return hipSuccess;
}

// ---- phase 2: needs the task count on the host; enqueues accumulate .. export + result copy
// jobs of this process between their first kernel and the end of their host tail (all engines, all lanes)
// (g_jobs_in_flight is defined with the accumulation chain, above)
// a caller that is about to run several jobs side by side on its own engines (the chunked host-pointer MSM) declares them
// "in flight" for the length of the call, so that the first of them already launches politely
void msm_hold_in_flight(bool on) { g_jobs_in_flight.fetch_add(on ? 1 : -1); }
void MsmEngine::mark_in_flight(bool on) {
  if (on == counted_) return;
  counted_ = on;
  g_jobs_in_flight.fetch_add(on ? 1 : -1);
}
bool MsmEngine::others_in_flight() const { return g_jobs_in_flight.load() > (counted_ ? 1 : 0); }
hipError_t MsmEngine::enqueue_back() {
  mark_in_flight(true);
  const hipError_t e = enqueue_back_impl();
  if (e != hipSuccess) mark_in_flight(false);
  return e;
}
hipError_t MsmEngine::finish() {
  const hipError_t e = finish_impl();
  mark_in_flight(false);
  return e;
}
hipError_t MsmEngine::enqueue_back_impl() {
  Job& j = job_;
  if (j.f.trivial) return hipSuccess;
  {
    const bool others = others_in_flight();   // ONE sample for every decision of this phase
    j.a = plan_accumulate(j.f, cfg_, cus_, others);
    j.r = plan_reduce(j.f, cfg_, others);
  }
  if (!j.r.valid) return hipErrorInvalidValue;
  SG_TRY(reserve_back(j));
  SG_TRY(launch_task_order(j));
  SG_TRY(launch_accumulate(j));
  SG_TRY(host_wait_event(ev_meta_));
  const volatile uint32_t* hm = h_meta_;   // written by the device (msm_scan_sums / msm_scan_small), complete with the event
  j.ntasks = hm[1];
  j.max_cnt = hm[2];
  if (!j.ntasks) {  // every digit was zero (the launches above found nothing to do)
    j.all_zero = true;
    return hipSuccess;
  }
  Partials ps{partial_[0].p, 0, 0};
  SG_TRY(launch_merge_rounds(j, ps));
  hipStream_t stream = j.stream;
  if (j.tm) SG_TRY(hipEventRecord(j.ev[3], stream));
  if (tail_stream_) {
    // the latency-bound tail runs on a high-priority stream so that its few workgroups are
    // dispatched ahead of the next MSM's accumulation (batches ping-pong between two engines)
    if (!ev_acc_) SG_TRY(hipEventCreateWithFlags(&ev_acc_, hipEventDisableTiming));
    SG_TRY(hipEventRecord(ev_acc_, stream));
    SG_TRY(hipStreamWaitEvent(tail_stream_, ev_acc_, 0));
    stream = tail_stream_;
  }
  return j.r.red2d ? launch_reduce_2d(j, ps, stream) : launch_reduce_scan(j, ps, stream);
}

// everything of the back end whose size the plans know (the merge rounds size theirs from the device's counters)
hipError_t MsmEngine::reserve_back(const Job& j) {
  const FrontPlan& f = j.f;
  const AccPlan& a = j.a;
  const ReducePlan& r = j.r;
  SG_TRY(partial_[0].reserve(a.partial_slots));
  SG_TRY(order_.reserve(a.ntasks_ub));
  if (!f.fe) SG_TRY(thist_.reserve((size_t)TASK_BINS * a.task_blocks));
  if (cfg_.acc_trace) SG_TRY(trace_.reserve((size_t)2 * a.total_threads() / 64));
  if (r.red2d) {
    const uint32_t rows = 1u << r.log_rows, cols = 1u << r.log_cols;
    SG_TRY(red_a_[0].reserve((size_t)f.sets * (rows + cols)));
    SG_TRY(red_a_[1].reserve((size_t)f.sets * (r.bits + 1)));
    if (r.prefold) SG_TRY(red_r_[0].reserve(f.NB));
    if (r.combine) SG_TRY(red_s_[0].reserve(f.sets));
    return hipSuccess;
  }
  for (int i = 0; i < 2; i++) {
    SG_TRY(red_a_[i].reserve((size_t)f.sets * r.blocks));
    SG_TRY(red_s_[i].reserve((size_t)f.sets * r.blocks));
    SG_TRY(red_r_[i].reserve((size_t)f.sets * r.blocks));
  }
  return hipSuccess;
}

// order_[pos] = (bucket, segment) of the task that runs as thread `pos`, longest tasks first
hipError_t MsmEngine::launch_task_order(const Job& j) {
  const FrontPlan& f = j.f;
  const AccPlan& a = j.a;
  if (f.fe) {
    msm_task_scatter_reserve<<<a.task_blocks, 256, 0, j.stream>>>(
        counts_.p, f.NB, f.log_L, a.task_block,
        FrontEndTotals{fe_.p, coff_.p, tbase_.p, off_.p, toff_[0].p, meta_.p, d_hmeta_, f.NBc, j.fe_parity, ACC_TICKET}, order_.p);
    return hipEventRecord(ev_meta_, j.stream);
  }
  msm_task_hist<<<a.task_blocks, 256, 0, j.stream>>>(counts_.p, f.NB, f.log_L, a.task_block, thist_.p);
  msm_task_scan<<<1, 256, 0, j.stream>>>(thist_.p, a.task_blocks, a.nbins, meta_.p + ACC_TICKET);
  msm_task_scatter<<<a.task_blocks, 256, 0, j.stream>>>(counts_.p, f.NB, f.log_L, a.task_block, thist_.p, order_.p);
  return hipSuccess;
}

hipError_t MsmEngine::launch_accumulate(const Job& j) {
  const FrontPlan& f = j.f;
  hipStream_t stream = j.stream;
  return chained_accumulate(stream, j.tm ? j.ev[5] : nullptr, [&]() {
    msm_accumulate<<<j.a.grid, j.a.threads, 0, stream>>>(sorted_.p, j.bp, f.NB / f.M, off_.p, counts_.p, toff_[0].p, order_.p,
                                                         f.log_L, meta_.p, meta_.p + ACC_TICKET, partial_[0].p,
                                                         cfg_.acc_trace ? trace_.p : nullptr);
  });
}

// heavy buckets: fold their partial sums until every bucket owns at most `fold`
hipError_t MsmEngine::launch_merge_rounds(const Job& j, Partials& ps) {
  const FrontPlan& f = j.f;
  hipStream_t stream = j.stream;
  for (MergeRound m = merge_rounds(f, j.ntasks, j.max_cnt); merge_round_next(f, j.r, m);) {
    const int nxt = 1 - ps.lvl;
    SG_TRY(launch_scan(ntask_[ps.lvl].p, f.NB, f.log_L, nullptr, ntask_[nxt].p, toff_[nxt].p, bsum_.p, meta_.p, stream));
    const uint32_t nt2 = m.items_ub;
    SG_TRY(partial_[1 - ps.pbuf].reserve(nt2));
    if (m.quad)
      msm_merge<4><<<(nt2 + 63) / 64, 256, 0, stream>>>(ps.cur, toff_[ps.lvl].p, ntask_[ps.lvl].p, toff_[nxt].p, f.NB, f.log_L,
                                                        meta_.p, partial_[1 - ps.pbuf].p);
    else
      msm_merge<1><<<(nt2 + 255) / 256, 256, 0, stream>>>(ps.cur, toff_[ps.lvl].p, ntask_[ps.lvl].p, toff_[nxt].p, f.NB, f.log_L,
                                                          meta_.p, partial_[1 - ps.pbuf].p);
    ps.pbuf = 1 - ps.pbuf;
    ps.cur = partial_[ps.pbuf].p;
    ps.lvl = nxt;
  }
  return hipSuccess;
}

// 2-D reduction (rows / columns / bits): plain sums only, ~9 dependent additions per launch instead of a chain
// of ~40.  Few sets: quad-cooperative additions and the powers of two on the host (bits + 1 points per set);
// many sets: one lane per addition and a third launch that applies the powers of two (one point per set).
hipError_t MsmEngine::launch_reduce_2d(const Job& j, const Partials& ps, hipStream_t stream) {
  const ReducePlan& r = j.r;
  const uint32_t NB = j.f.NB, sets = j.f.sets, bits = r.bits;
  const uint32_t* toff = toff_[ps.lvl].p;
  const uint32_t* ntask = ntask_[ps.lvl].p;
  Reduce2dShape sh{r.log_cols, r.log_rows};
  const dim3 lines((1u << r.log_rows) + (1u << r.log_cols), sets);
  if (r.prefold) {
    // partial sums -> one value per bucket (once), then line sums over plain arrays
    if (r.fold_quad) msm_fold_buckets<4><<<(NB + 63) / 64, 256, 0, stream>>>(ps.cur, toff, ntask, NB, red_r_[0].p);
    else msm_fold_buckets<1><<<(NB + 255) / 256, 256, 0, stream>>>(ps.cur, toff, ntask, NB, red_r_[0].p);
    if (r.quad) msm_reduce2d_lines_folded<4><<<lines, 256, 0, stream>>>(red_r_[0].p, sh, red_a_[0].p);
    else msm_reduce2d_lines_folded<1><<<lines, 256, 0, stream>>>(red_r_[0].p, sh, red_a_[0].p);
  } else if (r.quad) {
    msm_reduce2d_lines<4><<<lines, 256, 0, stream>>>(ps.cur, toff, ntask, sh, red_a_[0].p);
  } else {
    msm_reduce2d_lines<1><<<lines, 256, 0, stream>>>(ps.cur, toff, ntask, sh, red_a_[0].p);
  }
  if (r.quad) msm_reduce2d_bits<4><<<dim3(bits + 1, sets), 256, 0, stream>>>(red_a_[0].p, sh, red_a_[1].p);
  else msm_reduce2d_bits<1><<<dim3(bits + 1, sets), 256, 0, stream>>>(red_a_[0].p, sh, red_a_[1].p);
  const xyzz29_mem* fin = red_a_[1].p;
  if (r.combine) {
    msm_reduce2d_combine<<<sets, 32, 0, stream>>>(red_a_[1].p, bits, red_s_[0].p);
    fin = red_s_[0].p;
  }
  const uint32_t count = r.export_count(sets);
  if (j.tm) SG_TRY(hipEventRecord(j.ev[4], stream));
  msm_export_points<<<(count + 63) / 64, 64, 0, stream>>>(fin, count, d_hwin_);
  SG_TRY(hipEventRecord(ev_done_, stream));
  return hipGetLastError();
}

// scan-based reduction: level 0 over the buckets, level 1 over the workgroup items (see plan_reduce)
hipError_t MsmEngine::launch_reduce_scan(const Job& j, const Partials& ps, hipStream_t stream) {
  const ReducePlan& r = j.r;
  const uint32_t W = j.f.sets, nbw = j.f.nbw, threads = r.threads, blocks = r.blocks, T1 = r.T1;
  const uint32_t* toff = toff_[ps.lvl].p;
  const uint32_t* ntask = ntask_[ps.lvl].p;
  const size_t lds0 = (size_t)threads * 2 * sizeof(xyzz29_mem);
  ReduceOut lvl0{red_a_[0].p, red_s_[0].p, red_r_[0].p}, lvl1{red_a_[1].p, red_s_[1].p, red_r_[1].p};
  if (r.quad)
    msm_reduce_buckets<4><<<dim3(blocks, W), threads * 4, lds0, stream>>>(ps.cur, toff, ntask, nbw, r.log_G, lvl0);
  else if (r.lean)
    msm_reduce_buckets_lean<1><<<dim3(blocks, W), threads, lds0, stream>>>(ps.cur, toff, ntask, nbw, r.log_G, lvl0);
  else
    msm_reduce_buckets<1><<<dim3(blocks, W), threads, lds0, stream>>>(ps.cur, toff, ntask, nbw, r.log_G, lvl0);
  ReduceOut fin = lvl0;
  if (blocks > 1) {
    if (r.items_quad)
      msm_reduce_items<4><<<dim3(1, W), 3 * T1 * 4, (size_t)3 * T1 * sizeof(xyzz29_mem), stream>>>(lvl0, blocks, T1, lvl1);
    else
      msm_reduce_items<1><<<dim3(1, W), 3 * T1, (size_t)3 * T1 * sizeof(xyzz29_mem), stream>>>(lvl0, blocks, T1, lvl1);
    fin = lvl1;
  }
  if (j.tm) SG_TRY(hipEventRecord(j.ev[4], stream));
  msm_export_windows<<<(3 * W + 63) / 64, 64, 0, stream>>>(fin, W, blocks > 1 ? 1u : 0u, d_hwin_);
  SG_TRY(hipEventRecord(ev_done_, stream));
  return hipGetLastError();
}

// ---- phase 3: wait for the window sums; host tail
using host::Fq;
using host::Jac;
static Jac point_at(const uint32_t* h_win, uint32_t q) {
  using namespace host;
  Fq x, y, zz, zzz;
  std::memcpy(x.v, h_win + 32 * q, 32);
  std::memcpy(y.v, h_win + 32 * q + 8, 32);
  std::memcpy(zz.v, h_win + 32 * q + 16, 32);
  std::memcpy(zzz.v, h_win + 32 * q + 24, 32);
  return jac_from_xyzz(x, y, zz, zzz);
}
// window_w = A + 2^log_G (S + 2^log_N T) and result = sum_w 2^(offset_w) window_w: all 3W terms
// are placed at their bit offsets and folded by ONE double-and-add sweep from the top bit
// (254 + log_G + log_N doublings instead of W * (width + log_G + log_N))
// terms per window: legacy (A, S, T) at offsets (0, log_G, log_G + log_N); 2-D with host weights: term t < bits
// at offset t and the total at 0; 2-D with device weights: one term at 0
static Jac msm_total(const FrontPlan& f, const ReducePlan& r, const uint32_t* h_win, uint32_t m) {
  using namespace host;
  constexpr uint32_t MAXBIT = 254 + 16 + 16;
  const uint32_t Wm = f.fixed ? 1u : f.wp.W;  // fixed-base: the table rows already carry the window offsets
  const uint32_t per_win = r.per_win;
  int head[MAXBIT + 1];
  int next[3 * 64];
  for (auto& h : head) h = -1;
  uint32_t top = 0, off = 0;
  for (uint32_t w = 0; w < Wm; w++) {
    for (uint32_t which = 0; which < per_win; which++) {
      uint32_t rel;
      if (r.red2d == 1) rel = which < r.bits ? which : 0u;
      else if (r.red2d == 2) rel = 0;
      else rel = (which >= 1 ? r.log_G : 0) + (which == 2 ? r.log_N : 0);
      const uint32_t bit = off + rel;
      const int id = (int)(per_win * w + which);
      next[id] = head[bit];
      head[bit] = id;
      top = std::max(top, bit);
    }
    off += f.wp.width[w];
  }
  Jac total = Jac::identity();
  for (int bit = (int)top; bit >= 0; bit--) {
    total = jac_double(total);
    for (int id = head[bit]; id >= 0; id = next[id]) total = jac_add(total, point_at(h_win, per_win * m * Wm + (uint32_t)id));
  }
  return total;
}
// affine normalisation of the M results with ONE field inversion (Montgomery's trick): an inversion
// is ~13 us on the host, as much as the rest of a fixed-base tail
static void store_affine(const Jac* totals, uint32_t M, uint8_t* out_affine) {
  Fq prefix[MAX_FUSED];
  Fq run = Fq::one();
  for (uint32_t m = 0; m < M; m++) {
    prefix[m] = run;
    if (!totals[m].is_identity()) run = run * totals[m].z;
  }
  Fq inv = run.inv();
  for (uint32_t m = M; m-- > 0;) {
    uint8_t* out = out_affine + 64 * m;
    if (totals[m].is_identity()) {
      std::memset(out, 0, 64);
      continue;
    }
    const Fq zi = inv * prefix[m];
    inv = inv * totals[m].z;
    const Fq zi2 = zi.sqr();
    const Fq ax = totals[m].x * zi2, ay = totals[m].y * zi2 * zi;
    std::memcpy(out, ax.v, 32);
    std::memcpy(out + 32, ay.v, 32);
  }
}

hipError_t MsmEngine::finish_impl() {
  Job& j = job_;
  auto drop_events = [&]() {
    if (j.tm) {
      for (auto& e : j.ev) (void)hipEventDestroy(e);
    }
  };
  if (j.f.trivial) {
    std::memset(j.out, 0, 64 * std::max<size_t>(1, j.f.M));
    return hipSuccess;
  }
  if (j.all_zero) {
    std::memset(j.out, 0, 64 * (size_t)j.f.M);
    drop_events();
    return hipSuccess;
  }
  SG_TRY(host_wait_event(ev_done_));
  Jac totals[MAX_FUSED];
  for (uint32_t m = 0; m < j.f.M; m++) totals[m] = msm_total(j.f, j.r, h_win_, m);
  store_affine(totals, j.f.M, j.out);
  if (cfg_.acc_trace && j.a.total_threads()) print_acc_trace();
  if (j.tm) {
    report_timings();
    drop_events();
  }
  return hipSuccess;
}

// debug: when the waves of the accumulation left, as a share of the launch's span (first start .. last exit)
void MsmEngine::print_acc_trace() const {
  const size_t waves = job_.a.total_threads() / 64;
  std::vector<uint64_t> t(2 * waves);
  if (hipMemcpy(t.data(), trace_.p, t.size() * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return;
  uint64_t t0 = ~0ull, t1 = 0;
  for (size_t w = 0; w < waves; w++) { t0 = std::min(t0, t[2 * w]); t1 = std::max(t1, t[2 * w + 1]); }
  std::vector<double> ends(waves);
  size_t late = 0;
  const double span = (double)(t1 - t0) / 100.0;
  for (size_t w = 0; w < waves; w++) {
    ends[w] = (double)(t[2 * w + 1] - t0) / span;
    late += (double)(t[2 * w] - t0) / span > 5.0 ? 1 : 0;
  }
  std::sort(ends.begin(), ends.end());
  auto pct = [&](double q) { return ends[std::min(waves - 1, (size_t)(q * (double)waves))]; };
  std::fprintf(stderr, "[acc_trace] waves %zu (%zu started after 5 %% of the span), span %.0f ticks; 1 %% of the waves had left by %.1f %% of it, 10 %% by %.1f, 25 %% by %.1f, 50 %% by %.1f, 75 %% by %.1f, 90 %% by %.1f, 99 %% by %.1f\n",
               waves, late, span * 100.0, pct(0.01), pct(0.10), pct(0.25), pct(0.50), pct(0.75), pct(0.90), pct(0.99));
}

void MsmEngine::report_timings() {
  const Job& j = job_;
  MsmTimings* tm = j.tm;
  float ms;
  (void)hipEventElapsedTime(&ms, j.ev[0], j.ev[1]); tm->digits_ms = ms;
  (void)hipEventElapsedTime(&ms, j.ev[1], j.ev[2]); tm->sort_ms = ms;
  (void)hipEventElapsedTime(&ms, j.ev[5], j.ev[3]); tm->accumulate_ms = ms;   // the accumulation (and merge rounds) alone
  (void)hipEventElapsedTime(&ms, j.ev[2], j.ev[5]); tm->order_ms = ms;        // task ordering + time queued behind other jobs' accumulations
  (void)hipEventElapsedTime(&ms, j.ev[3], j.ev[4]); tm->reduce_ms = ms;
  (void)hipEventElapsedTime(&ms, j.ev[0], j.ev[4]); tm->total_ms = ms;
  tm->window_bits = j.f.c;
  tm->windows = j.f.wp.W;
  tm->tasks = j.ntasks;
  tm->max_bucket = j.max_cnt;
  tm->accumulate_threads = j.a.total_threads();
}

hipError_t MsmEngine::run(const fp_words* d_scalars, const g1_affine_mem* d_bases, size_t n, hipStream_t stream,
                          uint8_t out_affine[64], MsmTimings* tm) {
  SG_TRY(enqueue_front(d_scalars, d_bases, n, stream, out_affine, tm));
  SG_TRY(enqueue_back());
  return finish();
}

}  // namespace sg
