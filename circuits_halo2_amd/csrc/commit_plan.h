// What a commitment decides on the host before the MSM engine sees it: which basis and window table it runs against, how a
// batch is cut into fused jobs, how a host-pointer call is cut into chunks, and the order in which those chunks cross the link
// and run.  Pure functions and one driver template over the caller's device operations; abi_msm.hip fills the inputs from
// the SRS cache and makes the HIP calls.  Standard headers only: tests/cpp/commit_plan_check.cpp runs all of it without a GPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/summa_gpu.h"
#include "msm_plan.h"

namespace sg {

// ------------------------------------------------------------------ which basis, which table
// the window tables of an SRS (sg_srs_precompute): [0] g, [1] g_lagrange, [2] the prefix sums of g_lagrange
struct SrsTables {
  uint32_t k = 0;
  struct Table {
    bool present = false;
    uint32_t c = 0;
    size_t n = 0;
  } tab[3];
  bool same_plan(int a, int b) const { return tab[a].c == tab[b].c && tab[a].n == tab[b].n; }
};

struct BasisChoice {
  int basis;    // the basis that runs: 0 g, 1 g_lagrange, 2 the prefix sums
  bool diff;    // the scalars are taken in difference form (basis == 2)
  bool fixed;   // the window table of `basis` exists: the fixed-base path ...
  int table;    // ... over tab[table]; -1 for the generic MSM over the resident bases
};
// basis 2 = a Lagrange column taken in difference form (same commitment as basis 1): possible when the prefix-sum table
// exists and the column has the full 2^k rows; otherwise such a column is an ordinary Lagrange one
inline BasisChoice resolve_basis(const SrsTables& s, int basis, size_t n) {
  const bool diff = basis == 2 && s.tab[2].present && n == ((size_t)1 << s.k);
  const int b = basis == 2 && !diff ? 1 : basis;
  const bool fixed = s.tab[b].present;
  return BasisChoice{b, diff, fixed, fixed ? b : -1};
}

// one basis per column (sg_commit_batch_mixed_dev): all columns of the job run on one path
struct MixedChoice {
  bool fixed = false;        // fixed-base only when both tables exist with one plan; otherwise the generic fused path over g / g_lagrange
  bool diff_ok = false;      // difference form (basis 2) needs the prefix-sum table on the same plan; otherwise such a column is an ordinary Lagrange one
  bool all_sparse = false;   // every column carries SG_BASIS_SPARSE (and there is one)
  std::vector<uint8_t> b;      // per column: the basis that runs
  std::vector<uint8_t> flags;  // per column: 1 = difference form
};
inline MixedChoice resolve_mixed(const SrsTables& s, const int* basis, size_t count, size_t n) {
  MixedChoice m;
  m.fixed = s.tab[0].present && s.tab[1].present && s.same_plan(0, 1);
  m.diff_ok = m.fixed && s.tab[2].present && n == ((size_t)1 << s.k) && s.same_plan(2, 0);
  m.all_sparse = count > 0;
  m.b.resize(count);
  m.flags.resize(count);
  for (size_t i = 0; i < count; i++) {
    const int want = basis[i] & ~SG_BASIS_SPARSE;
    m.all_sparse = m.all_sparse && (basis[i] & SG_BASIS_SPARSE);
    m.b[i] = (uint8_t)(want == 2 ? (m.diff_ok ? 2 : 1) : want);
    m.flags[i] = m.b[i] == 2;
  }
  return m;
}
// A job whose columns are all witness-like (mostly zeros and small values: few entries, some of them in heavy buckets) is a
// latency chain of one task length whatever its size: tasks of 8 instead of 16 halve it (a proof's first commitment job
// 1.07 -> 1.00 ms) where dense jobs lose by them (profiles/r04_sweeps/task_length_by_phase.txt).  A hint, never semantics.
// (only for jobs small enough for the 2-D reduction, which adds up to eight partial sums per bucket itself: a fused job of many
// proofs' columns goes through merge rounds, and shorter tasks would add one)
inline bool sparse_hint_applies(bool all_sparse, bool fixed, size_t count, uint32_t log_seg, size_t n) {
  return all_sparse && fixed && count <= 5 && log_seg == 0 && n >= ((size_t)1 << 14);
}

// ------------------------------------------------------------------ a batch as fused jobs
// consecutive MSMs of equal length are fused into one job (all kernels span the whole group), at most limit(length) of them
struct FusedGroup {
  size_t first, count;
};
template <class Limit>
std::vector<FusedGroup> fused_groups(const size_t* n, size_t count, Limit&& limit) {
  std::vector<FusedGroup> groups;
  for (size_t i = 0; i < count;) {
    const size_t lim = limit(n[i]);
    size_t g = 1;
    while (i + g < count && n[i + g] == n[i] && g < lim) g++;
    groups.push_back({i, g});
    i += g;
  }
  return groups;
}

// ------------------------------------------------------------------ a host-pointer call as chunks
// K: "msm.host_chunks" (0 = by size: 2 from 2^18 pairs; more chunks lose: every job brings its own latency chains, and small
// kernels beside an accumulation run slowly)
static constexpr size_t MSM_HOST_SPLIT_MIN = (size_t)1 << 18;
static constexpr uint32_t MSM_HOST_CHUNKS_MAX = 8;
inline uint32_t host_chunk_count(int param, size_t n) {
  uint32_t K = (uint32_t)param;
  if (K == 0) K = n < MSM_HOST_SPLIT_MIN ? 1u : 2u;   // measured at 2^20 (profiles/r04_sweeps/host_chunks.txt): 2 is the best for both entry points
  K = std::min<uint32_t>(K, MSM_HOST_CHUNKS_MAX);
  if (n < 2 * (size_t)K) K = 1;
  return K;
}
// chunk i is [lo[i], lo[i + 1])
inline std::vector<size_t> host_chunk_bounds(size_t n, uint32_t K) {
  std::vector<size_t> lo(K + 1);
  for (uint32_t i = 0; i <= K; i++) lo[i] = n * i / K;
  return lo;
}
// sg_commit: no window table for this basis (sg_srs_precompute not called): the generic MSM over the resident bases, in chunks,
// so that the scalars' upload and one job's latency chains run under another job's accumulation
inline bool commit_goes_in_chunks(const SrsTables& s, int basis, size_t n) {
  return !resolve_basis(s, basis, n).fixed && n >= MSM_HOST_SPLIT_MIN;
}

// The order of a chunked call.  Chunk i's job runs on engine i & 1 while chunk i + 1 is still travelling, and one job's latency
// chains run under the other's accumulation:
//   [S0 B0] front(0) { back(i) [S i+1 B i+1] finish(i-1) front(i+1) } ... finish
// ops: copy_scalars(i), copy_bases(i) (the chunk's copies and their events), front(i) (sort front end), back(i) (accumulation
// and reduction), finish(i) (host tail), each returning an error code whose value-initialised form means success.  Returns the
// first failure.  After it nothing new is started, but from the first front on every open job is still closed in order: back
// for every chunk whose front succeeded (an engine left with an open job would poison the lane's next call), finish for every
// chunk whose back succeeded.
template <class Ops>
auto run_chunk_pipeline(uint32_t K, Ops& ops) -> decltype(ops.front(0u)) {
  using Err = decltype(ops.front(0u));
  const Err ok = Err();
  Err err = ok;
  enum State : uint8_t { NOTHING, FRONT_ENQUEUED, BACK_ENQUEUED, CLOSED };
  std::vector<uint8_t> state(K, NOTHING);
  auto copy_scalars = [&](uint32_t i) {
    if (err == ok) err = ops.copy_scalars(i);
  };
  auto copy_bases = [&](uint32_t i) {
    if (err == ok) err = ops.copy_bases(i);
  };
  auto front = [&](uint32_t i) {
    if (err != ok) return;
    err = ops.front(i);
    if (err == ok) state[i] = FRONT_ENQUEUED;
  };
  auto back = [&](uint32_t i) {
    if (state[i] != FRONT_ENQUEUED) return;
    const Err e = ops.back(i);
    state[i] = e == ok ? BACK_ENQUEUED : CLOSED;
    if (err == ok) err = e;
  };
  auto finish = [&](uint32_t i) {
    if (state[i] != BACK_ENQUEUED) return;
    const Err e = ops.finish(i);
    state[i] = CLOSED;
    if (err == ok) err = e;
  };
  copy_scalars(0);
  copy_bases(0);
  front(0);
  for (uint32_t i = 0; i < K; i++) {
    back(i);                              // (waits for chunk i's sort; then its accumulation is on the device ...)
    if (i + 1 < K) {
      copy_scalars(i + 1);                // ... and runs while the next chunk crosses the link (a copy from pageable memory blocks the host)
      copy_bases(i + 1);
      if (i >= 1) finish(i - 1);          // the engine chunk i + 1 runs on
      front(i + 1);
    }
  }
  for (uint32_t i = 0; i < K; i++) {       // whatever is still open (the last two jobs; everything after a failure)
    back(i);
    finish(i);
  }
  return err;
}

}  // namespace sg
