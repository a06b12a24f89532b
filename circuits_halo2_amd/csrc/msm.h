// Host-side interface of the MSM engine (msm.hip; its decisions: msm_plan.h; its kernels: msm_sort.cuh, msm_accumulate.cuh,
// msm_reduce.cuh).  The one-launch tiny MSM is in msm_tiny.hip, many of them in one launch in msm_many.hip, the set-up time G1
// operations in g1_ops.h.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>

#include "bn254_curve29.cuh"
#include "devmem.h"
#include "g1_ops.h"
#include "msm_plan.h"

#define SG_TRY(x)                      \
  do {                                 \
    hipError_t _e = (x);               \
    if (_e != hipSuccess) return _e;   \
  } while (0)

namespace sg {

static constexpr uint32_t MSM_TINY_MAX = 64;   // MSMs of at most this many points run as ONE launch (MsmEngine::run_tiny)

// many MSMs of at most MSM_TINY_MAX points in one launch (msm_many.hip): S holds 64 window sums of 32 words per job
static constexpr uint32_t MSM_MANY_WINDOWS = 64, MSM_MANY_MAX_JOBS = 1u << 14, MSM_MANY_MAX_RANGES = 8;
static constexpr size_t MSM_MANY_JOB_WORDS = (size_t)MSM_MANY_WINDOWS * 32;
struct ManyRanges {   // [v[2 r], v[2 r + 1]): the jobs of range r (kernel argument)
  uint32_t v[2 * MSM_MANY_MAX_RANGES];
};

struct MsmTimings {
  float digits_ms = 0, sort_ms = 0, accumulate_ms = 0, reduce_ms = 0, total_ms = 0;
  uint32_t window_bits = 0, windows = 0, tasks = 0, max_bucket = 0, accumulate_threads = 0;
  float order_ms = 0;   // between the sort and the accumulation: task ordering, and the wait behind other jobs' accumulations
};

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t need) {
    if (p && need <= cap) return hipSuccess;
    const size_t want = need + need / 4 + 64;
    T* q = nullptr;
    hipError_t e = hipMalloc(&q, want * sizeof(T));
    if (e != hipSuccess) {   // out of memory: give the retired blocks back and try once more
      retired_device_memory_collect();
      e = hipMalloc(&q, want * sizeof(T));
      if (e != hipSuccess) return e;
    }
    retire_device_memory(p);   // kernels enqueued earlier may still be reading the old block
    p = q;
    cap = want;
    return hipSuccess;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

struct BatchPtrs {  // inputs of a fused batch (kernel argument)
  const fp_words* scalars[MAX_FUSED];
  const g1_affine_mem* bases[MAX_FUSED];
  uint64_t diff_mask;  // bit m: MSM m is taken in difference form -- its digits are those of s[i] - s[i+1] (s[n] = 0) and
                       // its bases the inclusive prefix sums of the basis (see g1_prefix_sums)
};

class MsmEngine {
 public:
  ~MsmEngine();
  hipError_t init();
  void release();
  MsmConfig& config() { return cfg_; }
  void set_tail_stream(hipStream_t s) { tail_stream_ = s; }
  uint32_t window_bits_for(size_t n, bool fused = false) const;
  // d_scalars: n x 32 B Montgomery Fr, d_bases: n x 64 B affine; result: 64 B affine on the host
  hipError_t run(const fp_words* d_scalars, const g1_affine_mem* d_bases, size_t n, hipStream_t stream, uint8_t out_affine[64],
                 MsmTimings* tm);
  // n <= MSM_TINY_MAX points from HOST memory (the verifier's 37): one launch, no staging copy, result on return (msm_tiny.hip)
  hipError_t run_tiny(const uint8_t* h_scalars, const uint8_t* h_bases, size_t n, hipStream_t stream, uint8_t out_affine[64]);
  // the same in three phases, so that two engines on two streams can overlap one MSM's
  // latency-bound tail with the next MSM's sort/accumulate (sg_msm_g1_batch):
  //   enqueue_front: digits .. counting sort (+ async copy of the task counters)
  //   enqueue_back:  waits for the counters, enqueues accumulate .. reduction + result copy
  //   finish:        waits for the result copy, host tail (Horner + normalisation)
  hipError_t enqueue_front(const fp_words* d_scalars, const g1_affine_mem* d_bases, size_t n, hipStream_t stream,
                           uint8_t* out_affine, MsmTimings* tm);
  // M same-length MSMs fused into one job (out_affine: M x 64 bytes); M <= max_fused(n)
  hipError_t enqueue_front_fused(const fp_words* const* d_scalars, const g1_affine_mem* const* d_bases, size_t M,
                                 size_t n, hipStream_t stream, uint8_t* out_affine, MsmTimings* tm);
  size_t max_fused(size_t n) const;
  // the same over a precomputed window table (n <= tab.n): all M MSMs use the table's bases
  hipError_t enqueue_front_fixed(const fp_words* const* d_scalars, const FixedTable& tab, size_t M, size_t n,
                                 hipStream_t stream, uint8_t* out_affine, MsmTimings* tm,
                                 const g1_affine_mem* const* tables = nullptr, uint64_t diff_mask = 0);
  size_t max_fused_fixed(const FixedTable& tab, size_t n) const;
  hipError_t enqueue_back();
  hipError_t finish();

 private:
  struct Job {
    FrontPlan f{};       // the three plans: everything the launches below and the host tail read
    AccPlan a{};
    ReducePlan r{};
    BatchPtrs bp{};
    hipStream_t stream = nullptr;
    uint8_t* out = nullptr;
    MsmTimings* tm = nullptr;
    bool all_zero = false;
    uint32_t fe_parity = 0;   // fused front end: which replica set of fe_ this job uses
    uint32_t ntasks = 0, max_cnt = 0;   // read back from the device
    hipEvent_t ev[6];
  };
  struct Partials {   // where the partial sums of the buckets are: partial_[pbuf], indexed by toff_[lvl] / ntask_[lvl]
    const xyzz29_mem* cur = nullptr;
    int lvl = 0, pbuf = 0;
  };
  // `fixed`: the window table of a fixed-base job (nullptr: generic); diff_mask: see BatchPtrs
  hipError_t enqueue_front_job(const fp_words* const* d_scalars, const g1_affine_mem* const* d_bases, size_t M, size_t n,
                               hipStream_t stream, uint8_t* out_affine, MsmTimings* tm, const FixedTable* fixed, uint64_t diff_mask);
  hipError_t enqueue_front_impl(const fp_words* const* d_scalars, const g1_affine_mem* const* d_bases, size_t M, size_t n,
                                hipStream_t stream, uint8_t* out_affine, MsmTimings* tm, const FixedTable* fixed, uint64_t diff_mask);
  hipError_t enqueue_back_impl();
  hipError_t finish_impl();
  // the steps of the two enqueue phases, in the order they run
  hipError_t reserve_front(const FrontPlan& f, hipStream_t stream);
  hipError_t launch_sort_two_pass(Job& j);
  hipError_t launch_sort_single(Job& j);
  hipError_t reserve_back(const Job& j);
  hipError_t launch_task_order(const Job& j);
  hipError_t launch_accumulate(const Job& j);
  hipError_t launch_merge_rounds(const Job& j, Partials& ps);
  hipError_t launch_reduce_2d(const Job& j, const Partials& ps, hipStream_t stream);
  hipError_t launch_reduce_scan(const Job& j, const Partials& ps, hipStream_t stream);
  void print_acc_trace() const;
  void report_timings();
  void mark_in_flight(bool on);
  bool others_in_flight() const;   // another engine of this process has a job between its first kernel and its host tail
  bool counted_ = false;
  hipError_t chained_accumulate(hipStream_t stream, hipEvent_t after_wait, const std::function<void()>& launch);
  hipEvent_t ev_chain_[2] = {nullptr, nullptr};
  int chain_slot_ = 0;
  uint32_t cus_ = 256;
  Job job_;
  uint32_t fe_parity_ = 0;             // fused front end: replica set of the most recent job (alternates)
  hipEvent_t ev_meta_ = nullptr, ev_done_ = nullptr, ev_acc_ = nullptr, ev_tiny_ = nullptr;
  hipStream_t tail_stream_ = nullptr;  // optional high-priority stream for reduce + export
  MsmConfig cfg_;
  DevBuf<int16_t> dig_;
  DevBuf<uint2> order_;
  DevBuf<uint32_t> thist_;
  DevBuf<uint32_t> sorted_, counts_, off_, ntask_[2], toff_[2], hist_, bsum_, meta_;
  DevBuf<xyzz29_mem> partial_[2], red_a_[2], red_s_[2], red_r_[2];
  DevBuf<uint32_t> fe_, tbase_;
  DevBuf<uint64_t> trace_;
  DevBuf<uint32_t> part_entry_, ccnt_, coff_;  // two-pass sort: partitioned entries, coarse-bin counts / offsets
  DevBuf<uint16_t> part_fine_;
  uint32_t* h_meta_ = nullptr;   // page-locked, written by the scan kernels through d_hmeta_ (its device address)
  uint32_t* d_hmeta_ = nullptr;
  size_t h_win_cap_ = 0;
  uint32_t* h_win_ = nullptr;    // W x 3 x 32 words: canonical XYZZ of (A, S, T) per window; written by the export kernels through d_hwin_
  uint32_t* d_hwin_ = nullptr;
  uint8_t* h_tiny_ = nullptr;    // run_tiny: scalars, points (read by the kernel) and the window sums (written by it), mapped
  uint8_t* d_tiny_ = nullptr;
};

// the host tail of the one-launch kernels: W window sums (32 canonical words each) -> the affine point (msm_tiny.hip)
void msm_window_sums_to_affine(const WindowPlan& wp, const uint32_t* h_sums, uint8_t out_affine[64]);
// msm_many.hip.  d_first: jobs + 1 offsets into d_scalars / d_bases, no job above MSM_TINY_MAX points; d_S: jobs x
// MSM_MANY_JOB_WORDS words.  The sums of `count` ranges of jobs go to d_out (count x MSM_MANY_JOB_WORDS words; the device address of
// mapped host memory), one host tail each.
hipError_t msm_many_launch(const fp_words* d_scalars, const g1_affine_mem* d_bases, const uint32_t* d_first, uint32_t jobs,
                           uint32_t* d_S, hipStream_t stream);
hipError_t msm_many_sum_launch(const uint32_t* d_S, const ManyRanges& ranges, uint32_t count, uint32_t* d_out, hipStream_t stream);

// one msm_accumulate launch as the engine issued it (parameter "msm.acc_log"; sg_msm_launch_log)
struct AccLaunchRecord {
  uint64_t entries;       // (digit, point) pairs the launch accumulates
  uint32_t n, M;          // the job: M polynomials / MSMs of n scalars each
  uint32_t threads;       // grid of the launch
  uint32_t fixed;         // 1: fixed-base job (a commitment), 0: generic
  uint32_t jobs_in_flight;  // jobs of the process in flight when it was issued (this one included)
  uint32_t task_len;      // L: entries per accumulation task
};
void msm_acc_log_enable(bool on);
size_t msm_acc_log_read(AccLaunchRecord* out, size_t cap);   // returns the number of records held
// +1 / -1 on the count of jobs in flight (MsmEngine::others_in_flight), for callers that run several jobs side by side
void msm_hold_in_flight(bool on);

}  // namespace sg
