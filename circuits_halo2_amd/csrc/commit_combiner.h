// The commit combiner.  Proofs in flight on several host threads (circuits_halo2_amd/batch.py) each issue five commitment
// jobs; alone, every job pays its own sort front-end, bucket reduction and host tail, and the jobs of different threads
// compete for the chip.  A thread that has declared itself (sg_commit_combine_begin) hands its sg_commit_batch*_dev calls
// to the combiner instead: the first caller to find no job running becomes the runner, waits a bounded time for the
// other declared threads to arrive (they do: after one fused job all of them get their points at the same moment and
// reach their next commitment together), takes EVERYTHING pending with the same SRS and length and runs it as ONE
// fused job on a lane of its own; callers that arrive while a job runs form the next one.  No caller ever waits for a
// thread that might not come -- only for a deadline -- so a failed or finished proof cannot block the others.
//
// No HIP in here: the device is reached through the `run` callable of submit() alone (abi_msm.hip supplies it), and
// tests/cpp/commit_combiner_check.cpp drives the same code from threads with a stand-in for it.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <exception>
#include <mutex>
#include <vector>

#include "../../include/summa_gpu.h"
#include "msm_plan.h"

// the clock of the runner's deadline (a build under the thread sanitizer names std::chrono::system_clock here: that runtime
// does not know the call a steady_clock wait_until makes)
#ifndef SG_COMBINER_CLOCK
#define SG_COMBINER_CLOCK std::chrono::steady_clock
#endif

namespace sg {

using CombinerClock = SG_COMBINER_CLOCK;

struct CommitReq {
  uint64_t srs;
  size_t n, count;
  const int* basis;
  const void* const* scalars;
  uint8_t* out;
  void* ready;           // the caller's event, recorded on its stream after its inputs were enqueued
  int rc = SG_OK;
  bool done = false;
  char err[256] = "";
};
// what `run` gets: `polys` commitments of length n against one SRS, for `n_members` requests
struct CommitJob {
  uint64_t srs;
  size_t n, polys;
  const int* basis;
  const void* const* scalars;
  uint8_t* out;
  CommitReq* const* members;
  size_t n_members;
};
enum class CombinerKnob { runners, wait_us, target };

struct Combiner {
  std::mutex mu;
  std::condition_variable cv;
  std::deque<CommitReq*> pending;
  int runners = 0;                       // fused jobs running now
  int busy = 0;                          // requests inside those jobs
  int members = 0;                       // threads between join and leave
  std::atomic<uint64_t> jobs{0}, requests{0};   // statistics: fused jobs run, requests served
  std::atomic<uint64_t> isolated{0};     // members re-run alone after their fused job failed as a whole

  void join() {
    std::lock_guard<std::mutex> lk(mu);
    members++;
  }
  void leave() {
    std::lock_guard<std::mutex> lk(mu);
    members--;
    cv.notify_all();          // a runner waiting for this thread stops counting it
  }

  // Hands `req` in and returns its code once a job has served it (req.err holds the text of a failure); the calling thread
  // may run that job, and others', itself.
  //   run(const CommitJob&, char err[256]) -> int   runs the job's members as one job on a lane of its own, whose stream waits
  //                                                 for every member's `ready`; on failure the text goes to err
  //   knob(CombinerKnob) -> int                     the value in effect now (read anew at every use: a change during a wait counts)
  //   fail_next() -> bool                           debug hook, asked (and so consumed) only for jobs of more than one member
  template <class Run, class Knob, class FailNext>
  int submit(CommitReq& req, Run&& run, Knob&& knob, FailNext&& fail_next) {
    std::unique_lock<std::mutex> lk(mu);
    pending.push_back(&req);
    cv.notify_all();                         // a runner waiting for stragglers counts again
    while (!req.done) {
      const bool mine_pending = std::find(pending.begin(), pending.end(), &req) != pending.end();
      if (!mine_pending || runners >= knob(CombinerKnob::runners)) {   // my request is inside a running job, or no runner slot is free
        cv.wait(lk);
        continue;
      }
      runners++;                             // this thread runs the next job
      // the bounded wait shrinks with the company that can still come: a thread is a member for the whole of its proof, not
      // only around its commitments, so at the tail of a batch the few proofs left would otherwise sit out the full wait
      // (5 ms in batch.prove_batch) at every one of their five jobs for members that are busy elsewhere
      const int may_come = std::max(1, members - busy - (int)pending.size());
      const int wait_us = std::min(knob(CombinerKnob::wait_us), 400 * may_come);
      const auto deadline = CombinerClock::now() + std::chrono::microseconds(wait_us);
      // wait for company: until `target` requests are pending, or every declared thread that is not inside a running job
      // has arrived, or the deadline
      while ((int)pending.size() < std::min(knob(CombinerKnob::target), members - busy))
        if (cv.wait_until(lk, deadline) == std::cv_status::timeout) break;
      if (pending.empty()) {   // another runner took everything meanwhile (this thread's request included)
        runners--;
        cv.notify_all();
        continue;
      }
      // everything pending with the first request's SRS and length, up to MAX_FUSED polynomials
      std::vector<CommitReq*> batch;
      size_t polys = 0;
      CommitReq* first = pending.front();
      for (auto it = pending.begin(); it != pending.end();) {
        CommitReq* r = *it;
        if (r->srs == first->srs && r->n == first->n && polys + r->count <= MAX_FUSED) {
          batch.push_back(r);
          polys += r->count;
          it = pending.erase(it);
        } else {
          ++it;
        }
      }
      busy += (int)batch.size();
      lk.unlock();
      run_batch(batch, run, fail_next);
      lk.lock();
      for (CommitReq* r : batch) r->done = true;
      busy -= (int)batch.size();
      runners--;
      cv.notify_all();
    }
    return req.rc;
  }

 private:
  // on the runner's thread: one fused job for all requests of `batch` (same SRS, same n)
  template <class Run, class FailNext>
  void run_batch(const std::vector<CommitReq*>& batch, Run& run, FailNext& fail_next) {
    try {
      run_batch_unguarded(batch, run, fail_next);
    } catch (const std::exception& e) {   // (allocation failures of the host vectors: every member learns of it)
      for (CommitReq* r : batch) {
        r->rc = SG_ERR_NOMEM;
        std::snprintf(r->err, sizeof r->err, "commit combiner: %s", e.what());
      }
    }
  }
  template <class Run, class FailNext>
  void run_batch_unguarded(const std::vector<CommitReq*>& batch, Run& run, FailNext& fail_next) {
    std::vector<int> basis;
    std::vector<const void*> scalars;
    size_t total = 0;
    for (CommitReq* r : batch) total += r->count;
    basis.reserve(total);
    scalars.reserve(total);
    for (CommitReq* r : batch)
      for (size_t i = 0; i < r->count; i++) {
        basis.push_back(r->basis[i]);
        scalars.push_back(r->scalars[i]);
      }
    std::vector<uint8_t> out(64 * total);
    char err[sizeof batch[0]->err] = "";
    int rc;
    if (batch.size() > 1 && fail_next()) {
      rc = SG_ERR_NOMEM;
      std::snprintf(err, sizeof err, "commit combiner: injected failure of a fused job");
    } else {
      rc = run(CommitJob{batch[0]->srs, batch[0]->n, total, basis.data(), scalars.data(), out.data(), batch.data(), batch.size()}, err);
    }
    size_t at = 0;
    for (CommitReq* r : batch) {
      r->rc = rc;
      if (rc == SG_OK) std::memcpy(r->out, out.data() + 64 * at, 64 * r->count);
      else std::snprintf(r->err, sizeof r->err, "%s", err);
      at += r->count;
    }
    if (rc != SG_OK && batch.size() > 1) {
      // The fused job failed AS A WHOLE -- out of device memory at this size, one member's bad pointer or stale handle.  One
      // member's fault must not cost the others their proofs: every member gets a job of its own (same lane discipline:
      // the job's stream waits for that member's inputs) and its own return value and message.
      for (CommitReq* r : batch) {
        CommitReq* const alone[1] = {r};
        r->rc = run(CommitJob{r->srs, r->n, r->count, r->basis, r->scalars, r->out, alone, 1}, r->err);
        if (r->rc == SG_OK) r->err[0] = 0;
        isolated.fetch_add(1);
      }
    }
    jobs.fetch_add(1);
    requests.fetch_add(batch.size());
  }
};

}  // namespace sg
