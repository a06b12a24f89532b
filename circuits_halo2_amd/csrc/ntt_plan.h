// What a transform decides on the host before it launches anything: how many passes and of which lengths, what each pass is
// (which index it transforms, where it writes, which scale rides on it), which leading stages a zero-padded first pass leaves
// out, and the workgroup of every launch -- tile, kernel, threads, grid, dynamic LDS.  Pure functions of the configuration and
// the job's shape; the engine (ntt.hip) launches what they return and takes no decision of its own.  Standard headers only:
// tests/cpp/ntt_plan_check.cpp runs these rules without a GPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace sg {

struct NttConfig {
  // measured on MI355X (profiles/r01_sweeps/ntt_sweep*.txt): small tiles (several workgroups per CU
  // hide the barrier and load latency) beat fewer, longer passes: the kernel is product-bound
  uint32_t max_single_log = 11;  // largest transform done in one LDS-resident pass
  uint32_t max_multi_log = 9;    // largest per-pass DFT length in multi-pass plans (2^17 = 2^9 x 2^8: two passes)
  uint32_t tile_log = 9;         // log2(elements per workgroup tile)  (2^9 * 36 B = 18 KiB LDS)
  uint32_t threads = 256;        // one butterfly per thread per stage at tile_log = 9
  // throughput shape, for launches that fill the chip anyway (batches of >= batch_min vectors, transforms of >= 2^big_log):
  // re-swept in round 3 with the round-2 closings in place (profiles/r03_sweeps/ntt_plans.txt) -- a lone 2^17 transform is
  // three or two launches at their latency floor and wants many small workgroups; 16 of them, or 2^22 points, want
  // wider tiles (two columns per 2^9-point DFT, coalesced 64-byte runs) on 512 threads
  uint32_t big_tile_log = 10;
  uint32_t big_threads = 512;
  uint32_t batch_min = 4;
  uint32_t big_log = 20;
  uint32_t radix4 = 1;           // two DIT stages per sweep over the LDS tile ("ntt.radix4"; same words): 0 never, 1 the throughput shapes (batches of >= batch_min vectors, transforms of >= 2^big_log points), 2 always
};

// ------------------------------------------------------------------ limits the rules share with the kernels
static constexpr uint32_t NTT_BATCH_MAX = 32;   // vectors per batched launch (the 25 coset blocks of a proof phase: one launch per pass)
static constexpr size_t NTT_LDS_BUDGET = 160 * 1024;   // dynamic LDS NttEngine::init allows both pass kernels: all of a CU's
// a pass of 2^11 points is the longest whose one-column tile fits that budget (2^12: 221,536 bytes): the parameter table keeps
// NttConfig::max_single_log and max_multi_log at or below it, and three-pass plans stay below it by themselves (log_n <= 28:
// ceil(28 / 3) = 10)
static constexpr uint32_t NTT_MAX_PASS_LOG = 11;
static constexpr uint32_t NTT_MAX_THREADS = 1024, NTT_MAX_THREADS_R4 = 512;   // __launch_bounds__ of ntt_pass / ntt_pass_r4

// ------------------------------------------------------------------ the pass factorisation of a 2^log_n transform
struct NttFactors {
  int npass;
  uint32_t l[3];   // log2 of the per-pass DFT lengths n1, n2, n3 (n = n1*n2*n3); the passes run in the order n3, n2, n1
};
inline NttFactors ntt_factor(const NttConfig& cfg, uint32_t log_n) {
  NttFactors f{1, {0, 0, 0}};
  if (log_n <= cfg.max_single_log) {
    f.l[0] = log_n;
  } else if (log_n <= 2 * cfg.max_multi_log) {
    f.npass = 2;
    f.l[0] = (log_n + 1) / 2;  // n1 (second pass DFT length)
    f.l[1] = log_n - f.l[0];   // n2 (first pass DFT length)
  } else {
    f.npass = 3;
    f.l[0] = (log_n + 2) / 3;
    f.l[1] = (log_n - f.l[0] + 1) / 2;
    f.l[2] = log_n - f.l[0] - f.l[1];
  }
  return f;
}
// a plain scale is folded into the first inter-pass twiddle table when there is one; a single pass applies it on its store
// (as does every plan when the caller brings three post factors of its own)
inline bool ntt_scale_in_table(const NttFactors& f, bool has_scale, bool has_post3) { return has_scale && !has_post3 && f.npass > 1; }

// `count` transforms of 2^log_n points each go through the batched launches (one launch per pass for up to NTT_BATCH_MAX vectors)
// up to this size: below it every launch of a lone transform sits at its ~5 us latency floor, and a 2^20 transform fills the
// chip on its own, so from 2^19 on the transforms run one after the other
static constexpr uint32_t NTT_BATCHED_MAX_LOG = 18;
inline bool ntt_batched(uint32_t log_n) { return log_n >= 1 && log_n <= NTT_BATCHED_MAX_LOG; }
// an in-place transform of several passes needs a scratch vector of 2^log_n elements: its first pass writes the intermediate
inline bool ntt_needs_scratch(const NttConfig& cfg, uint32_t log_n, bool in_place) { return in_place && ntt_factor(cfg, log_n).npass > 1; }

// pass `i` (0 = first launched) of a plan: the DFT over one index of the factorisation
struct NttPassGeom {
  uint32_t log_r;            // log2 R  (DFT length of this pass)
  uint32_t log_b;            // log2 B  (contiguous inner extent)
  uint32_t kind;             // 0: in-place-like (Y), 1: transposing first pass (X)
  uint32_t sig_lo, sig_hi;   // X only: b = lo + 2^sig_lo * hi  ->  b' = hi + 2^sig_hi * lo
  uint32_t fold29;           // last pass of a multi-pass plan: the data carries the factor 2^29 of the plan's last twiddle table
  int tw_local;              // which of the plan's local twiddle tables (index into l[])
  int tw_pass;               // which inter-pass twiddle table the store multiplies by; -1: none
  bool first, last;
};
inline NttPassGeom ntt_pass_geom(const NttFactors& f, int i) {
  const uint32_t l1 = f.l[0], l2 = f.l[1], l3 = f.l[2];
  NttPassGeom g{};
  g.first = i == 0;
  g.last = i == f.npass - 1;
  g.tw_pass = -1;
  if (f.npass == 1) {
    g.log_r = l1; g.log_b = 0; g.kind = 0; g.tw_local = 0;
  } else if (f.npass == 2) {
    if (i == 0) {   // pass X: DFT over i2 (length n2, stride n1), columns i1 contiguous
      g.log_r = l2; g.log_b = l1; g.kind = 1; g.sig_lo = l1; g.sig_hi = 0; g.tw_local = 1; g.tw_pass = 0;
    } else {        // pass Y: DFT over i1 (length n1, stride n2), columns j2 contiguous
      g.log_r = l1; g.log_b = l2; g.kind = 0; g.fold29 = 1; g.tw_local = 0;
    }
  } else {
    if (i == 0) {          // pass A: DFT over i3 (length n3, stride n1 n2); writes j3 + n3*(i2 + n2*i1)
      g.log_r = l3; g.log_b = l1 + l2; g.kind = 1; g.sig_lo = l1; g.sig_hi = l2; g.tw_local = 2; g.tw_pass = 0;
    } else if (i == 1) {   // pass B: DFT over i2 (length n2, stride n3) for each i1, in place
      g.log_r = l2; g.log_b = l3; g.kind = 0; g.tw_local = 1; g.tw_pass = 1;
    } else {               // pass C: DFT over i1 (length n1, stride n2 n3)
      g.log_r = l1; g.log_b = l2 + l3; g.kind = 0; g.fold29 = 1; g.tw_local = 0;
    }
  }
  return g;
}

// what rides on pass `i` of a job: the first pass reads the caller's source (the data itself for an in-place job; `in_len`
// elements, zero beyond) with the pre factors and the load table, a middle pass works in place in the intermediate (the
// scratch vector of an in-place job, else the data), the last pass writes the data and its store takes the caller's three
// post factors, or the plain scale when no table holds it
enum NttBuf : uint32_t { NTT_SOURCE, NTT_DATA, NTT_MID };
enum NttPost : uint32_t { NTT_POST_NONE, NTT_POST_CALLER, NTT_POST_SCALE };
struct NttPassRide {
  uint32_t in_len;
  bool pre3, pre_tab;
  NttPost post;
  NttBuf in, out;
};
inline NttPassRide ntt_pass_ride(const NttFactors& f, int i, size_t in_len, bool has_scale, bool has_pre3, bool has_post3, bool has_pre_tab) {
  const NttPassGeom g = ntt_pass_geom(f, i);
  const bool first = g.first, last = g.last;
  const size_t n = (size_t)1 << (f.l[0] + f.l[1] + f.l[2]);
  NttPassRide r{};
  r.in_len = (uint32_t)(first ? std::min(in_len, n) : n);
  r.pre3 = first && has_pre3;
  r.pre_tab = first && has_pre_tab;
  r.post = !last ? NTT_POST_NONE : has_post3 ? NTT_POST_CALLER : has_scale && !ntt_scale_in_table(f, has_scale, has_post3) ? NTT_POST_SCALE : NTT_POST_NONE;
  r.in = first ? NTT_SOURCE : NTT_MID;
  r.out = last ? NTT_DATA : NTT_MID;
  return r;
}

// leading stages of a zero-padded FIRST pass that can be skipped: rows r >= in_len >> log_b are zero
inline uint32_t ntt_skippable_stages(const NttPassGeom& g, uint32_t in_len, uint32_t log_n) {
  if (g.kind != 1 || in_len == 0 || (in_len & (in_len - 1)) || in_len >= (1u << log_n)) return 0;
  const uint32_t rows = in_len >> g.log_b;   // nonzero rows of every column (in_len is a power of two)
  if (rows == 0 || rows >= (1u << g.log_r)) return 0;
  uint32_t z = 0;
  while ((1u << z) < rows) z++;
  return g.log_r - z;
}

// ------------------------------------------------------------------ the workgroup of one launch
struct NttPassShape {
  bool big;            // the throughput shape (big_tile_log / big_threads) applies
  uint32_t skip;       // leading DIT stages not executed
  uint32_t log_t;      // log2 T  (contiguous columns per tile)
  uint32_t radix4;     // ntt_pass_r4 runs
  uint32_t threads, grid_x, grid_y;
  size_t elems;        // E = T * R elements per tile
  size_t lds_bytes;    // dynamic LDS of the launch
};
// dynamic LDS of a tile of 2^(log_r + log_t) elements: 36 bytes per element, the R/2 local twiddles and 8 constant slots
// likewise, 64 bytes of slack for the alignment of the word planes
inline size_t ntt_lds_bytes(uint32_t log_r, uint32_t log_t) {
  return (((size_t)1 << (log_r + log_t)) + ((size_t)1 << log_r) / 2 + 8) * 36 + 64;
}
inline NttPassShape ntt_pass_shape(const NttConfig& cfg, const NttPassGeom& g, uint32_t log_n, uint32_t in_len, uint32_t nbatch) {
  NttPassShape s{};
  s.skip = ntt_skippable_stages(g, in_len, log_n);
  // tile width: as many contiguous columns as the tile setting and the LDS budget allow
  s.big = (nbatch >= cfg.batch_min || log_n >= cfg.big_log) && cfg.big_tile_log;
  const uint32_t tile_log = s.big ? cfg.big_tile_log : cfg.tile_log, max_threads = s.big ? cfg.big_threads : cfg.threads;
  uint32_t log_e = std::min<uint32_t>(tile_log, log_n);
  if (log_e < g.log_r) log_e = g.log_r;
  s.log_t = std::min<uint32_t>(log_e - g.log_r, g.log_b);
  // (tiles of 2^12 elements fit beside the twiddles of a pass of up to 2^9 points only)
  while (s.log_t && ntt_lds_bytes(g.log_r, s.log_t) > NTT_LDS_BUDGET) s.log_t--;
  s.elems = (size_t)1 << (g.log_r + s.log_t);
  s.lds_bytes = ntt_lds_bytes(g.log_r, s.log_t);
  // two stages per sweep: measured (profiles/r05_sweeps/ntt_radix4.txt) 3-6 % faster for the throughput shapes -- lone transforms
  // of 2^20 points and more, the batched launches of a proof (25 coset blocks: 323 -> 310 us) --, 25 % slower for a lone 2^17
  // transform (two launches at their latency floor, which want many threads)
  const bool want_r4 = cfg.radix4 == 2 || (cfg.radix4 == 1 && s.big);
  s.radix4 = want_r4 && g.log_r - s.skip >= 2 ? 1u : 0u;
  // one butterfly (radix-4 sweeps: one group of four elements) per thread per sweep
  s.threads = (uint32_t)std::min<size_t>(s.radix4 ? std::min<uint32_t>(max_threads, NTT_MAX_THREADS_R4) : std::min<uint32_t>(max_threads, NTT_MAX_THREADS),
                                         std::max<size_t>(64, s.elems / (s.radix4 ? 4 : 2)));
  s.grid_x = 1u << (log_n - g.log_r - s.log_t);
  s.grid_y = nbatch ? nbatch : 1;
  return s;
}

}  // namespace sg
