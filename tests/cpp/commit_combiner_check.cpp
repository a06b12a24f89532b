// The commit combiner (csrc/commit_combiner.h) driven from threads on the CPU, with a stand-in for the device: `run` writes,
// per polynomial, 64 bytes made of that polynomial's scalar pointer and basis, records the job, and fails with a message
// when it meets a null scalar pointer.  One scenario per invocation (argv[1]); every check is independent of timing:
// where a scenario needs requests to be pending TOGETHER, the `runners` knob stays 0 (nobody may run a job) until they
// are, which is also what a parameter changed during a wait looks like.  Prints "fail: ..." lines and exits 1 if a check
// does not hold; otherwise the figures tests/test_commit_plan_cpu.py reads, and "ok".
//   load RUNNERS | bad_member | injected | absent | oversized
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>

#include "commit_combiner.h"

using namespace sg;

static std::atomic<int> g_failed{0};
#define CHECK(cond, ...)                                     \
  do {                                                       \
    if (!(cond)) {                                           \
      std::printf("fail: line %d: %s: ", __LINE__, #cond);   \
      std::printf(__VA_ARGS__);                              \
      std::printf("\n");                                     \
      g_failed = 1;                                          \
    }                                                        \
  } while (0)

struct JobRecord {
  uint64_t srs;
  size_t n, polys;
  std::vector<CommitReq> members;   // copies, taken while the job ran: the requests live on their callers' stacks
  int rc;
};
static void expected_point(const void* scalars, int basis, uint8_t out[64]) {
  for (int w = 0; w < 4; w++) {
    std::memcpy(out + 16 * w, &scalars, sizeof scalars);
    std::memcpy(out + 16 * w + 8, &basis, sizeof basis);
    std::memcpy(out + 16 * w + 12, &w, sizeof w);
  }
}

struct World {
  Combiner comb;
  std::atomic<int> runners{1}, wait_us{100000}, target{4}, fail_flag{0};
  std::mutex mu;   // of the records below
  std::vector<JobRecord> jobs;
  int running = 0, max_running = 0;

  int run(const CommitJob& j, char* err) {
    {
      std::lock_guard<std::mutex> lk(mu);
      max_running = std::max(max_running, ++running);
    }
    int rc = SG_OK;
    for (size_t i = 0; i < j.polys && rc == SG_OK; i++)
      if (!j.scalars[i]) {
        rc = SG_ERR_INVALID;
        std::snprintf(err, sizeof(CommitReq::err), "stand-in: null scalars at polynomial %zu of a job of %zu member(s)", i, j.n_members);
      }
    for (size_t i = 0; i < j.polys && rc == SG_OK; i++) expected_point(j.scalars[i], j.basis[i], j.out + 64 * i);
    std::this_thread::yield();
    std::lock_guard<std::mutex> lk(mu);
    jobs.push_back({j.srs, j.n, j.polys, {}, rc});
    for (size_t m = 0; m < j.n_members; m++) jobs.back().members.push_back(*j.members[m]);
    running--;
    return rc;
  }
  int submit(CommitReq& req) {
    return comb.submit(
        req, [this](const CommitJob& j, char* err) { return run(j, err); },
        [this](CombinerKnob k) { return (k == CombinerKnob::runners ? runners : k == CombinerKnob::wait_us ? wait_us : target).load(); },
        [this] { return fail_flag.exchange(0) != 0; });
  }
  // with runners == 0: returns once `count` requests are pending together, then lets one runner go
  void release_when_pending(size_t count) {
    for (;;) {
      {
        std::lock_guard<std::mutex> lk(comb.mu);
        if (comb.pending.size() == count) break;
      }
      std::this_thread::yield();
    }
    runners = 1;
    std::lock_guard<std::mutex> lk(comb.mu);
    comb.cv.notify_all();
  }
  // not_run: members of fused jobs that the hook failed before `run` saw them
  void check_quiet(uint64_t want_requests, uint64_t not_run = 0) {
    std::lock_guard<std::mutex> lk(comb.mu);
    CHECK(comb.pending.empty() && comb.runners == 0 && comb.busy == 0 && comb.members == 0, "pending %zu runners %d busy %d members %d",
          comb.pending.size(), comb.runners, comb.busy, comb.members);
    CHECK(comb.requests.load() == want_requests, "requests %" PRIu64, comb.requests.load());
    size_t served = 0;
    for (const JobRecord& j : jobs) {
      served += j.members.size();
      size_t polys = 0;
      for (const CommitReq& r : j.members) {
        polys += r.count;
        CHECK(r.srs == j.srs && r.n == j.n, "a job of srs %" PRIu64 " n %zu holds a request of srs %" PRIu64 " n %zu", j.srs, j.n, r.srs, r.n);
      }
      CHECK(polys == j.polys && polys <= MAX_FUSED, "a job of %zu polynomials, its members' %zu", j.polys, polys);
    }
    CHECK(served + not_run == want_requests + comb.isolated.load(), "served %zu, requests %" PRIu64 " + isolated %" PRIu64, served, want_requests, comb.isolated.load());
    std::printf("jobs=%zu requests=%" PRIu64 " isolated=%" PRIu64 " max_running=%d\n", jobs.size(), comb.requests.load(), comb.isolated.load(), max_running);
  }
};

// one request of `count` polynomials whose scalar pointers are its own; poisoned: one of them is null
struct Request {
  std::vector<char> own;
  std::vector<int> basis;
  std::vector<const void*> scalars;
  std::vector<uint8_t> out;
  CommitReq req;
  bool poisoned;
  Request(uint64_t srs, size_t n, size_t count, bool poisoned_)
      : own(count), basis(count), scalars(count), out(64 * count, 0xee), req{srs, n, count, nullptr, nullptr, nullptr, nullptr}, poisoned(poisoned_) {
    for (size_t i = 0; i < count; i++) {
      basis[i] = (int)(i % 3);
      scalars[i] = &own[i];
    }
    if (poisoned) scalars[count / 2] = nullptr;
    req.basis = basis.data();
    req.scalars = scalars.data();
    req.out = out.data();
  }
  // the return value, the message and the outputs are this request's own
  void check(int rc) const {
    CHECK(rc == req.rc && req.done, "rc %d, req.rc %d", rc, req.rc);
    if (poisoned) {
      CHECK(rc == SG_ERR_INVALID, "rc %d", rc);
      const std::string want = "stand-in: null scalars at polynomial " + std::to_string(req.count / 2) + " of a job of 1 member(s)";
      CHECK(want == req.err, "message '%s'", req.err);
      return;
    }
    CHECK(rc == SG_OK && req.err[0] == 0, "rc %d, message '%s'", rc, req.err);
    for (size_t i = 0; i < req.count; i++) {
      uint8_t want[64];
      expected_point(scalars[i], basis[i], want);
      CHECK(std::memcmp(want, out.data() + 64 * i, 64) == 0, "polynomial %zu of a request", i);
    }
  }
};

static void load(int runners) {
  World w;
  w.runners = runners;
  const int threads = 8, each = 50;
  std::vector<std::thread> ts;
  for (int t = 0; t < threads; t++)
    ts.emplace_back([&w, t] {
      w.comb.join();
      for (int i = 0; i < each; i++) {
        Request r(1 + ((t + i) & 1), i % 3 == 0 ? 1024 : 2048, 3, false);
        r.check(w.submit(r.req));
      }
      w.comb.leave();
    });
  for (auto& t : ts) t.join();
  w.check_quiet((uint64_t)threads * each);
  CHECK(w.max_running <= runners, "%d jobs at once with %d runners", w.max_running, runners);
  CHECK(w.comb.isolated.load() == 0, "isolated %" PRIu64, w.comb.isolated.load());
}

// `count` requests of `polys` polynomials from as many member threads, pending together before the first job starts
static void together(World& w, size_t count, size_t polys, int poisoned_one) {
  w.runners = 0;
  w.target = (int)count;
  std::vector<std::thread> ts;
  for (size_t t = 0; t < count; t++)
    ts.emplace_back([&w, t, polys, poisoned_one] {
      w.comb.join();
      Request r(7, 4096, polys, (int)t == poisoned_one);
      r.check(w.submit(r.req));
      w.comb.leave();
    });
  w.release_when_pending(count);
  for (auto& t : ts) t.join();
}

static void bad_member() {
  World w;
  together(w, 4, 3, 2);
  w.check_quiet(4);
  CHECK(w.jobs.size() == 5 && w.jobs[0].members.size() == 4 && w.jobs[0].rc == SG_ERR_INVALID, "%zu jobs", w.jobs.size());
  CHECK(w.comb.isolated.load() == 4 && w.comb.jobs.load() == 1, "isolated %" PRIu64, w.comb.isolated.load());
}

static void injected() {
  World w;
  w.fail_flag = 1;
  together(w, 4, 3, -1);
  CHECK(w.fail_flag.load() == 0, "the fused job did not take the flag");
  CHECK(w.jobs.size() == 4 && w.comb.isolated.load() == 4, "%zu jobs run, isolated %" PRIu64, w.jobs.size(), w.comb.isolated.load());
  for (const JobRecord& j : w.jobs) CHECK(j.members.size() == 1 && j.rc == SG_OK, "a re-run of %zu members, rc %d", j.members.size(), j.rc);
  // a job of one member does not ask the hook: the flag stays for the next fused job
  w.fail_flag = 1;
  w.comb.join();
  Request r(7, 4096, 3, false);
  r.check(w.submit(r.req));
  w.comb.leave();
  CHECK(w.fail_flag.load() == 1, "a single-member job consumed the flag");
  w.check_quiet(5, 4);
  CHECK(w.comb.isolated.load() == 4 && w.jobs.size() == 5, "isolated %" PRIu64 ", %zu jobs", w.comb.isolated.load(), w.jobs.size());
}

static void absent() {
  World w;
  w.target = 2;
  w.comb.join();   // a member that never submits
  std::thread t([&w] {
    w.comb.join();
    Request r(7, 4096, 3, false);
    r.check(w.submit(r.req));
    w.comb.leave();
  });
  t.join();
  w.comb.leave();
  w.check_quiet(1);
  CHECK(w.jobs.size() == 1, "%zu jobs", w.jobs.size());
}

static void oversized() {
  World w;
  together(w, 2, 40, -1);
  w.check_quiet(2);
  CHECK(w.jobs.size() == 2 && w.jobs[0].polys == 40 && w.jobs[1].polys == 40, "%zu jobs", w.jobs.size());
  CHECK(w.comb.isolated.load() == 0 && w.comb.jobs.load() == 2, "jobs %" PRIu64, w.comb.jobs.load());
}

int main(int argc, char** argv) {
  const std::string what = argc > 1 ? argv[1] : "";
  if (what == "load" && argc > 2) load(std::atoi(argv[2]));
  else if (what == "bad_member") bad_member();
  else if (what == "injected") injected();
  else if (what == "absent") absent();
  else if (what == "oversized") oversized();
  else {
    std::fprintf(stderr, "usage: commit_combiner_check load RUNNERS | bad_member | injected | absent | oversized\n");
    return 2;
  }
  if (g_failed) return 1;
  std::printf("ok\n");
  return 0;
}
