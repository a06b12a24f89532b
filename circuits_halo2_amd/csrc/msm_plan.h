// What an MSM job decides on the host before it launches anything: window widths, task length, which sort, which grids,
// which reduction.  Three plans, each filled by one pure function of the configuration, the job's shape and ONE sample of
// "are other jobs in flight" per phase; the engine (msm.hip) reserves and launches from their fields and takes no decision
// of its own.  Standard headers only: tests/cpp/msm_plan_check.cpp runs these rules without a GPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace sg {

static constexpr uint32_t MSM_LOG_FUSE_ENTRIES_GENERIC = 25, MSM_LOG_FUSE_ENTRIES_FIXED = 27;
struct MsmConfig {
  uint32_t window_bits = 0;    // 0: choose from n (log2 n - 2 single / - 4 fused, clamped to [4, 16])
  uint32_t log_seg = 0;        // L = 2^log_seg entries per accumulation task; 0: choose from n
  // fused batches hold at most 2^x (window, scalar) entries.  Fixed-base jobs (commitments): 27 = 64 polynomials of 2^17 rows over a
  // 16-window table in ONE job (round 5: with 25 a fused commitment job of a proof batch was cut into jobs of 16 polynomials, each
  // with a sort front end, reduction and host tail of its own: 269-272 -> 287-299 proofs/s at 64 proofs in flight,
  // profiles/r05_sweeps/batch_knobs.txt).  Generic jobs (sg_msm_g1_batch*) stay at 25: their groups alternate between two engines,
  // and eight MSMs of 2^20 run 6 % faster as four groups of two than as two of four (bench.py "batched": 1.45 against 1.54 ms per MSM)
  uint32_t log_fuse_entries = MSM_LOG_FUSE_ENTRIES_GENERIC;
  uint32_t log_fuse_entries_fixed = MSM_LOG_FUSE_ENTRIES_FIXED;
  uint32_t red_threads = 256;      // workgroup size of the level-0 bucket reduction (64, 128 or 256)
  uint32_t log_red_chunk = 0;  // G = 2^x buckets per thread in the bucket reduction; 0: auto
  uint32_t two_pass = 1;            // two-pass (coarse bin, in-LDS fine) sort: 0 never, 1 auto (>= 2^19 entries), 2 always
  uint32_t log_scatter_rounds = 0;  // the counting sort's scatter runs in 2^x bucket-range rounds
  uint32_t acc_threads = 0;    // workgroup size of msm_accumulate (0: 128)
  uint32_t acc_waves = 0;      // waves per SIMD of the persistent msm_accumulate launch: 0 = 3 (a full register file); >= 8: grid = tasks, one ticket per wave
  uint32_t acc_waves_fixed = 0; // ... of fixed-base jobs (the commitments of a proof, which run beside that proof's transforms on other streams): 0 = 2
  uint32_t merge_quad_tasks = 0x7fffffffu;  // merge rounds with more tasks than this use one lane per addition even when `quad` holds (default: no limit, the largest value sg_set_param takes)
  uint32_t red2d_max_sets = 6; // ... host-weights variant up to this many bucket sets (measured: tools/sweep_red2d.sh; 6 since the partial sums are folded first)
  uint32_t red2d = 1;          // 2-D (row / column / bit) bucket reduction: 0 never, 1 jobs of <= 4 bucket sets, 2 always
  uint32_t red2d_fold = 8;     // ... whose line sums add up to this many partial sums per bucket themselves (no merge round below that)
  uint32_t red2d_prefold = 1;  // ... after a pass that adds every bucket's partial sums once (msm_fold_buckets); 0: the line sums add them on the way (twice)
  uint32_t prefold_quad_buckets = 1u << 15;  // ... with a quad per bucket up to this many buckets in the job, one lane per bucket beyond
  uint32_t acc_chain = 1;      // accumulations of different jobs run one after the other (each waits for the previous launch's event)
  uint32_t red_lean = 1;       // level-0 bucket reduction within 168 registers (fits beside a polite accumulation): 0 never, 1 when other jobs are in flight, 2 always
  uint32_t fused_frontend = 1; // two-pass sort: scans and task histogram inside the sort's own kernels (msm_fine_sort_fused): 0 never (the launches of rounds 1-4), 1 when no other job is in flight, 2 always
  uint32_t acc_trace = 0;      // debug: msm_accumulate records when each wave starts and leaves; finish() prints the percentiles to stderr
  uint32_t quad = 1;           // quad-cooperative point additions in merge / reduction: 0 never, 1 auto, 2 always
};

// ------------------------------------------------------------------ limits the rules share with the kernels
static constexpr size_t MAX_FUSED = 64;             // MSMs in one fused job (BatchPtrs)
static constexpr uint32_t SORT_TILE = 8192;         // entries per LDS tile (both passes of the two-pass sort)
static constexpr uint32_t FE_MAX_BINS = 4096;       // coarse bins the last workgroup of msm_hist_prefix scans (fused front end)
static constexpr uint32_t TASK_BINS = 257;          // task length clamped to 256
static constexpr uint32_t SCAN_ITEMS = 8, SCAN_THREADS = 256, SCAN_BLOCK = SCAN_ITEMS * SCAN_THREADS;
static constexpr uint32_t SCAN_SMALL_PER = 4;       // x 1024 threads = 4 Ki buckets (beyond that the strided stores cost more than the launches saved)
static constexpr uint32_t MSM_MAX_BUCKETS = 1024 * SCAN_BLOCK;        // the scans handle 2^21 buckets (1024 blocks x 2048)
static constexpr size_t MSM_MAX_ENTRIES = (size_t)1 << 32;            // bucket offsets are 32-bit (n <= 2^27 at c = 16)
static_assert(MSM_MAX_BUCKETS == (1u << 21), "1024 scan blocks of 2048 buckets");

// ------------------------------------------------------------------ windows
struct WindowPlan {  // per-window digit widths (see msm_digits)
  uint32_t W;
  uint8_t width[64];
};

// window widths: W-1 signed windows + an unsigned top window, 254 bits in total
inline WindowPlan make_window_plan(uint32_t c) {
  WindowPlan wp{};
  const uint32_t W1 = wp.W = (255 + c - 1) / c;  // W*c >= 255: the top window never carries out
  for (uint32_t q = 0; q + 1 < W1; q++) wp.width[q] = (uint8_t)c;
  wp.width[W1 - 1] = (uint8_t)(c - 1);
  for (uint32_t k = 0, slack = W1 * c - 255; k < slack; k++) wp.width[W1 - 2 - k] -= 1;
  return wp;
}

inline uint32_t fixed_window_bits_for(size_t n) {
  uint32_t lg = 0;
  while (((size_t)1 << (lg + 1)) <= n) lg++;
  return std::min<uint32_t>(16, std::max<uint32_t>(4, lg));  // measured: tools/sweep_fixed_c.py (k = 11 .. 17)
}

// Window size, from the measured sweeps (profiles/r01_sweeps/sweep_c2.txt): a single MSM is
// partly latency-bound (few, deep tasks) and prefers larger windows (log2 n - 2); a fused batch
// is throughput-bound and prefers the work-optimal log2 n - 4.
inline uint32_t window_bits_for(const MsmConfig& cfg, size_t n, bool fused) {
  if (cfg.window_bits) return std::min<uint32_t>(16, std::max<uint32_t>(4, cfg.window_bits));
  uint32_t lg = 0;
  while (((size_t)1 << (lg + 1)) <= n) lg++;
  int c = (int)lg - (fused ? 4 : 2);
  return (uint32_t)std::min(16, std::max(4, c));
}

// how many same-length MSMs one fused job takes
inline size_t max_fused(const MsmConfig& cfg, size_t n) {
  if (n == 0) return MAX_FUSED;
  const uint32_t c = window_bits_for(cfg, n, true);
  const uint32_t W = (255 + c - 1) / c;
  const size_t nb = (size_t)W << (c - 1);
  // the scans handle 2^21 buckets (1024 blocks x 2048); cap the fused work space (cfg: log_fuse_entries)
  const size_t by_buckets = ((size_t)1 << 21) / nb;
  const size_t by_entries = ((size_t)1 << cfg.log_fuse_entries) / std::max<size_t>(1, (size_t)W * n);
  return std::max<size_t>(1, std::min<size_t>(std::min(by_buckets, by_entries), MAX_FUSED));
}
// ... over a window table of width c with W windows
inline size_t max_fused_fixed(const MsmConfig& cfg, uint32_t c, uint32_t W, size_t n) {
  if (n == 0) return MAX_FUSED;
  const size_t by_buckets = ((size_t)1 << 21) >> (c - 1);
  const size_t by_entries = ((size_t)1 << cfg.log_fuse_entries_fixed) / std::max<size_t>(1, (size_t)W * n);
  return std::max<size_t>(1, std::min<size_t>(std::min(by_buckets, by_entries), MAX_FUSED));
}

// ------------------------------------------------------------------ front plan: digits and sort
struct FrontPlan {
  bool valid = false;      // false: the engine answers hipErrorInvalidValue
  bool trivial = false;    // no points or no MSMs: nothing is launched, every result is the identity
  bool fixed = false;      // fixed-base mode: the job's windows all land in one bucket set per MSM (see msm_scatter)
  uint32_t M = 1, n_tab = 0;
  size_t n = 0, entries = 0;
  uint32_t c = 0, W1 = 0, W = 0, sets = 0, nbw = 0, NB = 0;   // W: digit rows of the whole fused job; sets: its bucket sets
  WindowPlan wp{};
  uint32_t log_L = 0;      // tasks of L = 2^log_L entries
  bool two_pass = false;   // msm_partition / msm_fine_sort instead of msm_scatter
  bool fe = false;         // ... with the scans and the task histogram inside the sort's own kernels
  uint32_t B = 1, shift = 0, NBc = 0;   // coarse bins per bucket set, bucket >> shift = bin, bins of the job
  uint32_t P = 1, chunk = 0;            // chunking of the scalars: W * P workgroups
  uint32_t log_R = 0;                   // single-pass sort: scatter rounds
  size_t hwin_words = 0;                // host words of the window sums, whichever reduction runs
};

// task length: deep enough to amortise, shallow enough that the longest dependent chain of
// additions stays a small multiple of the per-lane share of the work
inline uint32_t auto_log_L(size_t entries, uint32_t NB) {
  uint32_t log_L = 0;
  const size_t share = 2 * entries / (256 * 4 * 64 * 4);  // entries per resident lane, x2
  // small jobs are pure latency chains: shorter tasks (more lanes, more merging) win -- measured at k = 11 .. 17
  // (tools/sweep_seg_batch.sh, time_fixed_phases.py: below ~12 M entries the chip is not full and long tasks only
  // lengthen the chain: 6.3 M entries, L = 64 -> 16: 1.25 -> 1.02 ms)
  const size_t depth = entries / NB;  // mean entries per bucket
  if (entries < ((size_t)1 << 16)) log_L = 2;
  else if (entries < ((size_t)1 << 19)) log_L = 3;
  else if (depth < 40 && entries >= ((size_t)1 << 20)) {
    // large jobs with shallow buckets (arbitrary bases: ~n / 2^(c-1) per bucket): a task is a whole bucket, and L
    // only has to exceed the largest bucket so that no merge round is needed (k = 18: L = 16 -> 64: 0.99 -> 0.88 ms)
    // (uniform scalars: the largest of NB Poisson(depth) buckets is ~ depth + 6 sqrt(depth), 66 at depth 32)
    size_t need = depth + 8;
    for (size_t r = 1; r * r <= 64 * depth; r++) need = depth + 8 + r;  // + 8 sqrt(depth)
    log_L = 6;
    while (log_L < 8 && (((size_t)1 << log_L) < share || ((size_t)1 << log_L) < need)) log_L++;
  }
  else if (entries <= (size_t)7 << 20) log_L = 4;
  else if (entries <= (size_t)12 << 20) log_L = 5;
  else {
    log_L = 4;
    while (log_L < 8 && ((size_t)1 << log_L) < share) log_L++;
  }
  return log_L;
}

// fixed_wp: the window plan of the job's table (with its width fixed_c and row length n_tab), nullptr for a generic job
inline FrontPlan plan_front(const MsmConfig& cfg, size_t M, size_t n, const WindowPlan* fixed_wp, uint32_t fixed_c,
                            size_t n_tab, bool others_in_flight) {
  FrontPlan f;
  f.M = (uint32_t)M; f.n = n;
  if (n == 0 || M == 0) {
    f.valid = f.trivial = true;
    return f;
  }
  if (n >= (1ull << 31) || M > MAX_FUSED) return f;
  f.fixed = fixed_wp != nullptr;
  f.n_tab = f.fixed ? (uint32_t)n_tab : 0;
  const uint32_t c = f.c = f.fixed ? fixed_c : window_bits_for(cfg, n, M > 1);
  f.wp = f.fixed ? *fixed_wp : make_window_plan(c);
  const uint32_t W1 = f.W1 = f.wp.W;
  const uint32_t W = f.W = W1 * (uint32_t)M;             // digit rows of the whole fused job
  const uint32_t nbw = f.nbw = 1u << (c - 1);
  const uint32_t NB = f.NB = (f.fixed ? (uint32_t)M : W) * nbw;
  if (NB > MSM_MAX_BUCKETS) return f;
  const size_t entries = f.entries = (size_t)W * n;
  if (entries >= MSM_MAX_ENTRIES) return f;
  f.log_L = cfg.log_seg;
  if (!f.log_L) f.log_L = auto_log_L(entries, NB);
  // two-pass sort (msm_partition / msm_fine_sort) for everything but small jobs: B coarse bins per
  // bucket set, sized for ~4 Ki entries per bin (half an LDS tile, so Poisson tails still fit)
  const uint32_t sets = f.sets = f.fixed ? (uint32_t)M : W;
  const size_t set_entries = entries / sets;
  const bool two_pass = f.two_pass = cfg.two_pass == 2 || (cfg.two_pass == 1 && entries >= ((size_t)1 << 19));  // measured crossover
  uint32_t B = 1, shift = c - 1;
  if (two_pass) {
    while (B < 1024 && B < nbw && (set_entries / B > 4096 || (nbw / B) > 8192)) B <<= 1;
    shift = 0;
    while ((nbw >> shift) > B) shift++;
  }
  f.B = B; f.shift = shift;
  // chunking of the scalars for the LDS-staged counting sort: W * P workgroups
  const uint32_t target_wgs = two_pass ? 1024 : (nbw * 4 > 64 * 1024) ? 256 : 512;
  uint32_t P = std::max<uint32_t>(1, target_wgs / W);
  const uint32_t chunk = f.chunk = (uint32_t)std::max<size_t>(two_pass ? SORT_TILE : 1024, (n + P - 1) / P);
  f.P = (uint32_t)((n + chunk - 1) / chunk);
  f.NBc = two_pass ? sets * B : 0;
  // round 5: the scans and the task-length histogram ride on the sort's own kernels (msm_hist_prefix's and
  // msm_fine_sort_fused's last workgroups): five launches fewer per job
  // ... for a job that has the device to itself (a blocking MSM 1.73 -> 1.70 ms, a proof's commitment jobs 26 launches
  // fewer); with other jobs in flight the separate small kernels slip in beside the running accumulation more easily than one
  // heavier sort pass does (three MSMs in flight: 770 -> 745 M points/s with the fused form, profiles/r05_sweeps/frontend.txt):
  // 1 = by that rule, 2 = always, 0 = never
  f.fe = two_pass && f.NBc <= FE_MAX_BINS && (cfg.fused_frontend == 2 || (cfg.fused_frontend == 1 && !others_in_flight));
  f.log_R = std::min<uint32_t>(cfg.log_scatter_rounds, c - 1);
  f.hwin_words = std::max<size_t>((size_t)W * 96, (size_t)W * 32 * 17);   // (A, S, T) per window, or bits + 1 points per set
  f.valid = true;
  return f;
}

// ------------------------------------------------------------------ accumulate plan: task ordering and msm_accumulate
// buckets per workgroup in the ordering passes: ~128 workgroups, 256 .. 8192 buckets each
inline uint32_t task_block_for(uint32_t NB, uint32_t nbins) {
  const uint32_t max_blk = std::min<uint32_t>(128, (32 * 1024) / nbins);  // msm_task_scan: nbins * nblk <= 32 Ki
  uint32_t tb = 256;
  while ((NB + tb - 1) / tb > max_blk) tb <<= 1;
  return tb;
}

struct AccPlan {
  uint32_t ntasks_ub = 0;       // upper bound of the task count (the exact one is on the device when the launch runs)
  size_t partial_slots = 0;     // partial sums the accumulation may write
  uint32_t nbins = 0, task_block = 0, task_blocks = 0;   // task ordering: lengths 0 .. L, buckets per workgroup, workgroups
  uint32_t threads = 0, waves = 0, grid = 0;             // msm_accumulate: workgroup size, waves per SIMD, workgroups
  uint32_t total_threads() const { return grid * threads; }
};

inline AccPlan plan_accumulate(const FrontPlan& f, const MsmConfig& cfg, uint32_t cus, bool others_in_flight) {
  AccPlan a;
  const uint32_t NB = f.NB, log_L = f.log_L;
  // tasks: sum_b ceil(cnt_b / L) <= (#non-empty buckets) + entries / L -- enough to size the task tables and the
  // accumulation launch without the counters; the host reads them (for the merge rounds) while that launch runs
  const uint32_t ntasks_ub = a.ntasks_ub = (uint32_t)(std::min<size_t>(NB, f.entries) + (f.entries >> log_L));
  // bucket b owns cur[toff_[lvl][b] .. +ntask_[lvl][b])
  // (fused front end: a bucket's task slots start at its coarse bin's base, with gaps at the end of every bin)
  a.partial_slots = f.fe ? (size_t)NB + (f.entries >> log_L) + 1 : (size_t)ntasks_ub;
  a.nbins = std::min<uint32_t>(1u << log_L, TASK_BINS - 1) + 1;  // task lengths 0 .. L
  // (fused front end: no scan over bins x workgroups to keep small any more: more, smaller workgroups -- the pass is latency, not work)
  a.task_block = f.fe ? (NB >= (1u << 16) ? 512u : 256u) : task_block_for(NB, a.nbins);
  a.task_blocks = (NB + a.task_block - 1) / a.task_block;
  const uint32_t at = a.threads = cfg.acc_threads ? cfg.acc_threads : 128;  // measured: 128 beats 256 by 5 % at 2^20 (finer-grained tail), 64 loses in fixed mode
  // persistent launch: `waves` per SIMD on every CU (3 fill the register file)
  // ... three fill the register file (a job that has the device to itself); two leave a third of it to the kernels of other
  // streams, which run at wave priority 3 (side_kernel_prio): the other jobs in flight, a proof's transforms under its commitments
  // Round 5, fixed-base jobs: three waves when the job is several ROUNDS of tasks on a two-wave launch (the five dense quotient
  // pieces of a proof: 330 K tasks on 131 072 lanes) -- the counters show the two-wave launch issuing 61 % of the time where
  // three waves issue 87 %, and nothing runs beside that job (the evaluations wait for its challenge); a job of ONE round
  // (a single polynomial: W, W') keeps two: its time is the length of one task, which a third wave per SIMD only stretches
  // (k = 17 proof, phase 4 2.03 -> 1.90 ms, phase 6 1.20 -> 1.26 with three waves everywhere; profiles/r05_sweeps/accumulate_waves_fixed.txt)
  const uint32_t lanes2 = cus * 4u * 64u * 2u;
  const uint32_t waves_fixed_auto = ntasks_ub >= 3u * lanes2 ? 3u : 2u;
  const uint32_t waves = a.waves = f.fixed ? (cfg.acc_waves_fixed ? cfg.acc_waves_fixed : waves_fixed_auto)
                                           : (cfg.acc_waves ? cfg.acc_waves : (others_in_flight ? 2 : 3));
  const uint32_t wg_all = (ntasks_ub + at - 1) / at;
  a.grid = waves >= 8 ? wg_all : std::min<uint32_t>(wg_all, cus * (waves * 4 * 64 / at));
  return a;
}

// ------------------------------------------------------------------ reduce plan: merge rounds and bucket reduction
struct ReducePlan {
  bool valid = false;          // false: the scan reduction cannot cover the window (hipErrorInvalidValue)
  bool quad = false;           // quad-cooperative point additions
  uint32_t red2d = 0;          // 0: scan-based reduction, 1: 2-D with host weights, 2: 2-D with device weights
  uint32_t fold = 1;           // partial sums per bucket the reduction adds itself (no merge round below that)
  uint32_t merge_quad_tasks = 0;   // merge rounds of more tasks than this run one lane per addition
  // 2-D: nbw = 2^(log_rows + log_cols) buckets per set, bits + 1 terms per set
  uint32_t log_rows = 0, log_cols = 0, bits = 0;
  bool prefold = false, fold_quad = false, combine = false;   // msm_fold_buckets first (with a quad per bucket); powers of two on the device
  // scan: level 0 of `blocks` workgroups of `threads` logical threads, G = 2^log_G buckets each; level 1 of T1 items (0: none)
  uint32_t log_G = 0, log_N = 0, threads = 0, blocks = 0, T1 = 0;
  bool lean = false, items_quad = false;   // msm_reduce_buckets_lean; level 1 quad-cooperative
  uint32_t per_win = 3;        // terms per window the host tail receives
  uint32_t export_count(uint32_t sets) const { return combine ? sets : sets * (bits + 1); }   // 2-D: points for the host
};

inline ReducePlan plan_reduce(const FrontPlan& f, const MsmConfig& cfg, bool others_in_flight) {
  ReducePlan r;
  const uint32_t Wm = f.fixed ? 1u : f.wp.W;  // bucket sets ("windows") per MSM
  const uint32_t NB = f.NB, W = Wm * f.M, nbw = f.nbw;
  // quad-cooperative additions pay off while the reduction is a latency chain (few buckets in total);
  // with many windows it is throughput-bound and one lane per addition is the efficient shape
  const bool quad = r.quad = cfg.quad == 2 || (cfg.quad == 1 && NB <= (1u << 18));  // measured crossover: tools/small_batches2.sh
  r.merge_quad_tasks = cfg.merge_quad_tasks;
  // 2-D reduction or the scan-based one?  Decided before the merge rounds because the 2-D line sums can add a bucket's few
  // partial sums themselves: up to `fold` of them per bucket need no merge round (its launches -- three scans and the merge --
  // cost more than the extra additions inside a launch that runs anyway)
  // Measured (profiles/r01_sweeps): a clear win for up to 4 sets (k = 17 single commit: reduction 190 -> 90 us); with
  // many sets the tree sums waste lanes and the scan-based path below is faster, so the device-weights variant only
  // runs when forced (msm.red2d = 2).
  r.red2d = (cfg.red2d && f.c >= 5) ? ((W <= cfg.red2d_max_sets && Wm <= 4) ? 1u : (cfg.red2d >= 2 ? 2u : 0u)) : 0u;
  r.fold = r.red2d ? cfg.red2d_fold : 1u;
  // terms per window: legacy (A, S, T) at offsets (0, log_G, log_G + log_N); 2-D with host weights: term t < bits
  // at offset t and the total at 0; 2-D with device weights: one term at 0
  r.bits = f.c - 1;
  r.per_win = r.red2d == 1 ? r.bits + 1 : r.red2d == 2 ? 1u : 3u;
  if (r.red2d) {
    r.log_cols = (r.bits + 1) / 2;
    r.log_rows = r.bits / 2;
    r.prefold = cfg.red2d_prefold != 0;
    r.fold_quad = quad && NB <= cfg.prefold_quad_buckets;
    r.combine = r.red2d == 2;
    r.valid = true;
    return r;
  }
  // bucket reduction: level 0 over the buckets, level 1 over the workgroup items.  Both are chains of
  // dependent point additions with most of the chip idle, so by default a point addition is spread
  // over the 4 lanes of a quad (cfg.quad; see `quad` above): 64 logical threads per workgroup.
  const uint32_t max_threads = quad ? 64u : cfg.red_threads;       // logical threads per workgroup
  const uint32_t max_blocks = quad ? 64u : 256u;                    // level 1 holds 3 * T1 * Q <= 768 lanes
  // G buckets per logical thread: 8 for the largest windows, 4 below (depth vs. work, measured)
  // ... and 16 when other jobs are in flight: the reduction then runs under another job's accumulation, where what counts is
  // the instructions it issues (running sums are 2 additions per bucket, the scan and tree steps come per thread: 88 instead
  // of 116 wave-additions per 2048 buckets), not the length of its own chain (alone: 0.29 -> 0.39 ms; three MSMs in
  // flight: +0.7 % points/s, profiles/r04_sweeps/reduce_chunk_pipelined.txt)
  const uint32_t auto_log_G = nbw >= (1u << 14) ? ((!quad && others_in_flight) ? 4u : 3u) : 2u;
  r.log_G = std::min<uint32_t>(cfg.log_red_chunk ? cfg.log_red_chunk : auto_log_G, f.c - 1);
  while ((nbw >> r.log_G) > max_threads * max_blocks) r.log_G++;
  const uint32_t items = nbw >> r.log_G;  // chunks per window at level 0 (a power of two)
  const uint32_t threads = r.threads = std::min<uint32_t>(max_threads, std::max<uint32_t>(16, items));
  const uint32_t blocks = r.blocks = (items + threads - 1) / threads;
  if (blocks > max_blocks) return r;
  r.log_N = 0;
  while ((1u << r.log_N) < threads) r.log_N++;
  r.lean = !quad && (cfg.red_lean == 2 || (cfg.red_lean == 1 && others_in_flight));
  if (blocks > 1) {
    r.T1 = 16;
    while (r.T1 < blocks) r.T1 <<= 1;
    // level 1 is a handful of items per window whatever the job: always a latency chain, so its additions are
    // quad-cooperative whenever the workgroup fits (3 * T1 * 4 lanes)
    r.items_quad = quad || r.T1 <= 64;
  }
  r.valid = true;
  return r;
}

// heavy buckets: their partial sums are folded, L at a time, until every bucket owns at most `fold`.  The launch loop is
//   for (MergeRound m = merge_rounds(f, ntasks, max_cnt); merge_round_next(f, r, m);) launch over m.items_ub tasks
struct MergeRound {
  uint32_t max_items;   // partial sums of the heaviest bucket before the round
  uint32_t items_ub;    // upper bound of the partial sums alive after the round = tasks of the round
  bool quad;            // the round's additions are quad-cooperative
};
inline MergeRound merge_rounds(const FrontPlan& f, uint32_t ntasks, uint32_t max_cnt) {
  return MergeRound{(max_cnt + (1u << f.log_L) - 1) >> f.log_L, ntasks, false};
}
inline bool merge_round_next(const FrontPlan& f, const ReducePlan& r, MergeRound& m) {
  if (!(m.max_items > r.fold)) return false;
  // no host round trip: sum_b ceil(t_b / L) <= (#non-empty buckets) + items / L
  const uint32_t nt2 = std::min(f.NB, m.items_ub) + (m.items_ub >> f.log_L);
  m.items_ub = nt2;
  m.quad = r.quad && nt2 <= r.merge_quad_tasks;
  m.max_items = (m.max_items + (1u << f.log_L) - 1) >> f.log_L;
  return true;
}

}  // namespace sg
