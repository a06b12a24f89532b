// MSM engine, the front end (included once by msm.hip): signed digits, the counting sort in its single-pass and two-pass
// forms, the scans that close it, and the ordering of the accumulation tasks.  The limits these kernels share with the host's
// planning (SORT_TILE, FE_MAX_BINS, TASK_BINS, SCAN_BLOCK, SCAN_SMALL_PER) are defined in msm_plan.h.
#pragma once
#include <type_traits>
#include "msm.h"
#include "side_prio.cuh"

namespace sg {

// ------------------------------------------------------------------ the engine's two small device tables, word by word
// meta_ (META_WORDS, zero when allocated): [0] entries, [1] tasks, [2] largest bucket count of the job (write_job_totals; the
// same three go to the host's mapped copy), [ACC_TICKET] msm_accumulate's task counter, [SCAN_DONE] the finished workgroups of
// msm_scan_sums (zero between launches).
static constexpr uint32_t ACC_TICKET = 8, SCAN_DONE = 12, META_WORDS = 16;
// fe_ (FE_WORDS, zero when allocated; the fused front end): [FE_HP_DONE] the finished workgroups of msm_hist_prefix (zero
// between launches), [FE_CURSOR + k] the task scatter's running position inside the tasks of length k (zero at its start), and
// two SETS of replicas, used by alternate jobs of the engine (a job's sort zeroes the other set for the next job): per replica
// r of set p at FE_SET + p * FE_SET_WORDS + r * FE_ROW: [0] tasks, [1] largest count, [2 + k] tasks of (clamped) length k
static constexpr uint32_t FE_HP_DONE = 3, FE_REPL = 64;
static constexpr uint32_t FE_CURSOR = 8, FE_ROW = TASK_BINS + 2, FE_SET_WORDS = FE_REPL * FE_ROW, FE_SET = FE_CURSOR + TASK_BINS,
                          FE_WORDS = FE_SET + 2 * FE_SET_WORDS;

// ------------------------------------------------------------------ shared bodies
// digit d != 0 lands in bucket |d| - 1 (d == 0 wraps to a huge value: msm_scatter's range test drops it) ...
__device__ __forceinline__ uint32_t digit_bucket(int32_t d) { return (uint32_t)(d < 0 ? -d : d) - 1u; }
// ... as the entry (row of the bases or of the window table, sign of the digit)
__device__ __forceinline__ uint32_t entry_word(uint32_t index, int32_t d) { return index | (d < 0 ? 0x80000000u : 0u); }

// Inclusive Hillis-Steele scan over the first n threads' words of NV separate LDS arrays (sums; MAX_LAST: the last array is a
// running maximum).  Every thread of the workgroup calls it, having stored its own words: one barrier, then two per step.
// `live` = false keeps a thread beyond the scanned range (msm_partition: B of 1024) out of the arrays but in the barriers.
template <uint32_t NV, bool MAX_LAST = false, typename T>
__device__ __forceinline__ void block_scan(uint32_t tid, uint32_t n, bool live, T* s0, T* s1 = nullptr, T* s2 = nullptr) {
  static_assert(NV >= 1 && NV <= 3, "one to three arrays");
  T* const s[3] = {s0, s1, s2};
  __syncthreads();
  for (uint32_t d = 1; d < n; d <<= 1) {
    T x[NV] = {};
    if (live && tid >= d) {
#pragma unroll
      for (uint32_t k = 0; k < NV; k++) x[k] = s[k][tid - d];
    }
    __syncthreads();
    if (live) {
#pragma unroll
      for (uint32_t k = 0; k < NV; k++) s[k][tid] = (MAX_LAST && k == NV - 1) ? max(s[k][tid], x[k]) : s[k][tid] + x[k];
    }
    __syncthreads();
  }
}

// The job's totals, by ONE thread: into off[NB] (optional), toff[NB], meta[0..2] and, when `host_meta` is given, straight into
// page-locked host memory the device can write (the host reads them after an event, no copy kernel in between).  `task_slots`
// is `tasks` but in the fused front end, whose task index space has gaps.
__device__ __forceinline__ void write_job_totals(uint32_t* off, uint32_t* toff, uint32_t NB, uint32_t* meta,
                                                 volatile uint32_t* host_meta, uint32_t entries, uint32_t task_slots,
                                                 uint32_t tasks, uint32_t largest) {
  if (off) off[NB] = entries;
  toff[NB] = task_slots;
  meta[0] = entries;
  meta[1] = tasks;
  meta[2] = largest;
  if (host_meta) {
    host_meta[0] = entries;
    host_meta[1] = tasks;
    host_meta[2] = largest;
    __threadfence_system();
  }
}

// A bucket of cv entries is nfull tasks of exactly L = 2^log_L entries plus at most one shorter task of rem; task lengths are
// histogrammed clamped to TASK_BINS - 1.
__device__ __forceinline__ uint32_t task_full_bin(uint32_t log_L) { return min(1u << log_L, TASK_BINS - 1); }
struct BucketTasks {
  uint32_t nfull, rem, full_bin, rem_bin;
};
__device__ __forceinline__ BucketTasks bucket_tasks(uint32_t cv, uint32_t log_L) {
  const uint32_t nfull = cv >> log_L, rem = cv - (nfull << log_L);
  return BucketTasks{nfull, rem, task_full_bin(log_L), min(rem, TASK_BINS - 1)};
}
// s_h[length] += the tasks of one bucket
__device__ __forceinline__ void count_bucket_tasks(uint32_t* s_h, uint32_t cv, uint32_t log_L) {
  const BucketTasks bt = bucket_tasks(cv, log_L);
  if (bt.nfull) atomicAdd(&s_h[bt.full_bin], bt.nfull);
  if (bt.rem) atomicAdd(&s_h[bt.rem_bin], 1u);
}
// ... of the task_block buckets of this workgroup
__device__ __forceinline__ void count_block_tasks(uint32_t* s_h, const uint32_t* __restrict__ cnt, uint32_t NB, uint32_t log_L,
                                                  uint32_t task_block) {
  for (uint32_t q = threadIdx.x; q < task_block; q += blockDim.x) {
    const uint32_t b = blockIdx.x * task_block + q;
    if (b < NB) count_bucket_tasks(s_h, cnt[b], log_L);
  }
}
// order[pos] = (bucket, segment) for every task of this workgroup's buckets, s_c[length] being the next free position among the
// tasks of that length
__device__ __forceinline__ void place_bucket_tasks(uint32_t* s_c, const uint32_t* __restrict__ cnt, uint32_t NB, uint32_t log_L,
                                                   uint32_t task_block, uint2* __restrict__ order) {
  for (uint32_t q = threadIdx.x; q < task_block; q += blockDim.x) {
    const uint32_t b = blockIdx.x * task_block + q;
    if (b < NB) {
      const BucketTasks bt = bucket_tasks(cnt[b], log_L);
      if (bt.nfull) {
        const uint32_t pos = atomicAdd(&s_c[bt.full_bin], bt.nfull);
        for (uint32_t seg = 0; seg < bt.nfull; seg++) order[pos + seg] = make_uint2(b, seg);
      }
      if (bt.rem) {
        const uint32_t pos = atomicAdd(&s_c[bt.rem_bin], 1u);
        order[pos] = make_uint2(b, bt.nfull);
      }
    }
  }
}

// ------------------------------------------------------------------ 1: signed digits
// Windows have individual widths (WindowPlan): W-1 signed windows of c or c-1 bits and an
// unsigned top window of at most c-1 bits, widths summing to exactly 254, so every window
// spreads its points over (almost) the same number of buckets -- a leftover-bits top window
// would put n / 2^t points in each of its 2^t buckets.
// dig[j*n + i] = digit j of scalar i as int16.  Adding K = sum_{j<W-1} 2^(o_j + w_j - 1)
// once makes every window's digit independent of its neighbours:
//   d_j = (((s + K) >> o_j) & (2^w_j - 1)) - 2^(w_j - 1)   in [-2^(w_j-1), 2^(w_j-1)).
// blockIdx.y = m selects the scalar vector of a fused batch (BatchPtrs); its digit rows are
// dig[(m*W + j)*n + i].
__global__ void msm_digits(BatchPtrs bp, uint32_t n, WindowPlan wp, int16_t* __restrict__ dig) {
  side_kernel_prio();
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const fp_words* __restrict__ scalars = bp.scalars[blockIdx.y];
  dig += (size_t)blockIdx.y * wp.W * n;
  words8 s;
  {
    // canonical scalar = s~ * 2^-256 = s~ * 2^5 * 2^-261
    f29 k = f29_zero();
    k.l[0] = 32;
    f29 v = f29_load_r256<Fr29>(scalars + i);                  // any 256-bit word value: bound < 6
    if ((bp.diff_mask >> blockIdx.y) & 1ull) {
      // difference form: the scalar of row i is s[i] - s[i+1] (s[n] = 0), against the prefix-summed basis
      if (i + 1 < n) v = f29_sub<Fr29, 2>(v, f29_load_r256<Fr29>(scalars + i + 1));   // + 8r: bound < 14
    }
    f29_to_words(f29_cond_sub_p<Fr29>(f29_mul<Fr29>(v, k)), s.l);
  }
  const uint32_t W = wp.W;
  // s += K (K < 2^254, s < 2^254: no overflow out of 256 bits)
  {
    uint32_t k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t o = 0;
    for (uint32_t j = 0; j + 1 < W; j++) {
      uint32_t bit = o + wp.width[j] - 1;
      uint32_t m = 1u << (bit & 31);
      uint32_t q = bit >> 5;
#pragma unroll
      for (int t = 0; t < 8; t++) k[t] |= (q == (uint32_t)t) ? m : 0u;
      o += wp.width[j];
    }
    uint32_t carry = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) {
      uint64_t t = (uint64_t)s.l[q] + k[q] + carry;
      s.l[q] = (uint32_t)t;
      carry = (uint32_t)(t >> 32);
    }
  }
  for (uint32_t j = 0; j < W; j++) {
    const uint32_t w = wp.width[j];
    uint32_t v = s.l[0] & ((1u << w) - 1);
#pragma unroll
    for (int q = 0; q < 7; q++) s.l[q] = (s.l[q] >> w) | (s.l[q + 1] << (32 - w));
    s.l[7] >>= w;
    int32_t d = (j + 1 < W) ? (int32_t)v - (int32_t)(1u << (w - 1)) : (int32_t)v;
    dig[(size_t)j * n + i] = (int16_t)d;
  }
}

// ------------------------------------------------------------------ 2: LDS-staged histogram
// grid (W, P): workgroup (j, p) counts the digits of scalar chunk p for window j in an LDS
// histogram of 2^(c-1) buckets, then stores it to hist[(j*P + p)*nbw + b].  The window is the
// fast grid index so that (workgroups being dealt round-robin to the 8 XCDs) the chunks of a
// window share an XCD's L2; measured neutral for msm_scatter's 4-byte scattered stores
// (WRITE_SIZE stays ~8x the useful bytes), kept because it costs nothing.
// `shift` > 0 histograms coarse bins (bucket >> shift) for the two-pass sort; nbw = bins per row.
__global__ void __launch_bounds__(1024) msm_hist(const int16_t* __restrict__ dig, uint32_t n, uint32_t chunk,
                                                 uint32_t nbw, uint32_t shift, uint32_t* __restrict__ hist) {
  side_kernel_prio();
  extern __shared__ uint32_t s_cnt[];
  const uint32_t j = blockIdx.x, p = blockIdx.y, P = gridDim.y;
  for (uint32_t b = threadIdx.x; b < nbw; b += blockDim.x) s_cnt[b] = 0;
  __syncthreads();
  const uint32_t lo = p * chunk, hi = min(n, lo + chunk);
  const int16_t* row = dig + (size_t)j * n;
  for (uint32_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    int32_t d = row[i];
    if (d) atomicAdd(&s_cnt[digit_bucket(d) >> shift], 1u);
  }
  __syncthreads();
  uint32_t* out = hist + ((size_t)j * P + p) * nbw;
  for (uint32_t b = threadIdx.x; b < nbw; b += blockDim.x) out[b] = s_cnt[b];
}
// per bucket: exclusive prefix over the P chunks (in place) and the bucket total.  Block of
// 32 buckets x 8 chunk groups: every thread sums its group's share of the column, the group
// bases come from LDS, then a second sweep writes the prefixes (a column is P strided loads;
// one thread per bucket made this the slowest kernel of a small MSM).
static constexpr uint32_t HP_BUCKETS = 32, HP_GROUPS = 8;
// Fused front end (`fe.done` != nullptr, coarse bins of the two-pass sort, NB <= FE_MAX_BINS): the workgroup that finishes LAST
// (a counter in device memory, as msm_scan_sums does for its block sums) also scans the bin totals -- coff[g] = entries before
// bin g and tbase[g] = task slots before bin g, a bin of F buckets and E entries owning F + (E >> log_L) slots (an upper bound
// of its sum_f ceil(c_f / L) tasks) -- in place of a launch of its own (msm_scan_small / msm_scan_sums + msm_scan_write).
struct FrontEndScan {
  uint32_t* done;    // counter of finished workgroups (zero between launches), nullptr: no scan here
  uint32_t* coff;    // [NB + 1]
  uint32_t* tbase;   // [NB + 1]
  uint32_t F, log_L;
};
__global__ void __launch_bounds__(256) msm_hist_prefix(uint32_t* __restrict__ hist, uint32_t P, uint32_t nbw, uint32_t NB,
                                                       uint32_t* __restrict__ counts, FrontEndScan fe) {
  side_kernel_prio();
  __shared__ uint32_t s_sum[HP_GROUPS][HP_BUCKETS];
  __shared__ uint32_t s_last;
  const uint32_t bx = threadIdx.x % HP_BUCKETS, gy = threadIdx.x / HP_BUCKETS;
  const uint32_t g = blockIdx.x * HP_BUCKETS + bx;  // global bucket id = j*nbw + b
  const bool live = g < NB;
  const uint32_t j = live ? g / nbw : 0, b = live ? g - j * nbw : 0;
  uint32_t* col = hist + (size_t)j * P * nbw + b;
  const uint32_t per = (P + HP_GROUPS - 1) / HP_GROUPS;
  const uint32_t lo = min(gy * per, P), hi = min(lo + per, P);
  uint32_t sum = 0;
  if (live)
    for (uint32_t p = lo; p < hi; p++) sum += col[(size_t)p * nbw];
  s_sum[gy][bx] = sum;
  __syncthreads();
  uint32_t run = 0;
  for (uint32_t q = 0; q < gy; q++) run += s_sum[q][bx];
  if (live) {
    for (uint32_t p = lo; p < hi; p++) {
      uint32_t v = col[(size_t)p * nbw];
      col[(size_t)p * nbw] = run;
      run += v;
    }
    if (gy == HP_GROUPS - 1) {
      if (fe.done) {   // a returning exchange: performed at the memory side once the value is back (no release fence needed below)
        const uint32_t was = atomicExch(&counts[g], run);
        asm volatile("" ::"v"(was));
      } else {
        counts[g] = run;
      }
    }
  }
  if (!fe.done) return;
  __syncthreads();                       // (every thread of the workgroup reaches this: the early return above is gone)
  if (threadIdx.x == 0) s_last = atomicAdd(fe.done, 1u) == gridDim.x - 1 ? 1u : 0u;
  __syncthreads();
  if (!s_last) return;
  // the last workgroup: exclusive scans over the NB <= 4096 bin totals, 16 per thread (atomic reads of what the other
  // workgroups' exchanges left)
  __shared__ uint32_t s_a[256], s_t[256];
  const uint32_t tid = threadIdx.x, per_t = (NB + 255) / 256, b0 = min(tid * per_t, NB), b1 = min(b0 + per_t, NB);
  uint32_t vals[FE_MAX_BINS / 256];
  uint32_t a = 0, t = 0;
#pragma unroll
  for (uint32_t q = 0; q < FE_MAX_BINS / 256; q++) vals[q] = (b0 + q < b1) ? atomicAdd(&counts[b0 + q], 0u) : 0u;   // all in flight together
#pragma unroll
  for (uint32_t q = 0; q < FE_MAX_BINS / 256; q++) {
    if (b0 + q < b1) {
      a += vals[q];
      t += fe.F + (vals[q] >> fe.log_L);
    }
  }
  s_a[tid] = a; s_t[tid] = t;
  block_scan<2>(tid, 256, true, s_a, s_t);
  uint32_t ra = s_a[tid] - a, rt = s_t[tid] - t;
#pragma unroll
  for (uint32_t q = 0; q < FE_MAX_BINS / 256; q++) {
    if (b0 + q < b1) {
      fe.coff[b0 + q] = ra;
      fe.tbase[b0 + q] = rt;
      ra += vals[q];
      rt += fe.F + (vals[q] >> fe.log_L);
    }
  }
  if (tid == 255) {
    fe.coff[NB] = s_a[255];
    fe.tbase[NB] = s_t[255];
    atomicExch(fe.done, 0u);             // ready for the next launch on this stream
  }
}

// ------------------------------------------------------------------ 3: scans over the buckets (multi-block)
// cnt[NB] -> off[NB+1] (exclusive scan, optional), ntask[b] = ceil(cnt[b]/L), toff[NB+1]
// (exclusive scan of ntask), meta = {sum cnt, sum ntask, max cnt}.  2048 buckets per block.

// The scan of the (<= 1024) block sums is done by whichever workgroup of this launch finishes LAST (a counter in device
// memory, zero between launches: the last arrival resets it; no workgroup ever waits for another): one ~5.5 us launch less per
// scan than with a one-workgroup launch of its own, two scans per MSM job.  The totals: write_job_totals.
__global__ void __launch_bounds__(256) msm_scan_sums(const uint32_t* __restrict__ cnt, uint32_t NB, uint32_t log_L,
                                                     uint32_t* __restrict__ bsum, uint32_t* __restrict__ meta,
                                                     uint32_t* __restrict__ off, uint32_t* __restrict__ toff,
                                                     volatile uint32_t* host_meta) {
  side_kernel_prio();
  __shared__ uint32_t s_a[SCAN_THREADS], s_t[SCAN_THREADS], s_m[SCAN_THREADS];
  __shared__ uint32_t s_last;
  const uint32_t Lm1 = (1u << log_L) - 1;
  uint32_t base = blockIdx.x * SCAN_BLOCK + threadIdx.x * SCAN_ITEMS;
  uint32_t a = 0, t = 0, m = 0;
#pragma unroll
  for (uint32_t k = 0; k < SCAN_ITEMS; k++) {
    uint32_t v = (base + k < NB) ? cnt[base + k] : 0;
    a += v;
    t += (v + Lm1) >> log_L;
    m = max(m, v);
  }
  s_a[threadIdx.x] = a; s_t[threadIdx.x] = t; s_m[threadIdx.x] = m;
  __syncthreads();
  for (uint32_t s = SCAN_THREADS / 2; s >= 1; s >>= 1) {
    if (threadIdx.x < s) {
      s_a[threadIdx.x] += s_a[threadIdx.x + s];
      s_t[threadIdx.x] += s_t[threadIdx.x + s];
      s_m[threadIdx.x] = max(s_m[threadIdx.x], s_m[threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    bsum[3 * blockIdx.x] = s_a[0];
    bsum[3 * blockIdx.x + 1] = s_t[0];
    bsum[3 * blockIdx.x + 2] = s_m[0];   // the largest count of the block
    __threadfence();                     // the sums above are visible device-wide before this workgroup counts as done
    s_last = atomicAdd(meta + SCAN_DONE, 1u) == gridDim.x - 1 ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  // the last workgroup: exclusive scan of the nblk <= 1024 block sums (4 per thread), totals out
  const uint32_t nblk = gridDim.x, tid = threadIdx.x;
  volatile uint32_t* vb = bsum;          // written by other workgroups of this launch: not through a cached non-coherent load
  uint32_t va[4], vt[4], vm = 0;
  a = 0; t = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) {
    const uint32_t b = 4 * tid + k;
    va[k] = b < nblk ? vb[3 * b] : 0u;
    vt[k] = b < nblk ? vb[3 * b + 1] : 0u;
    vm = max(vm, b < nblk ? vb[3 * b + 2] : 0u);
    a += va[k];
    t += vt[k];
  }
  __syncthreads();
  s_a[tid] = a; s_t[tid] = t; s_m[tid] = vm;
  block_scan<3, true>(tid, SCAN_THREADS, true, s_a, s_t, s_m);
  uint32_t ra = s_a[tid] - a, rt = s_t[tid] - t;
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) {
    const uint32_t b = 4 * tid + k;
    if (b < nblk) {
      bsum[3 * b] = ra;
      bsum[3 * b + 1] = rt;
    }
    ra += va[k];
    rt += vt[k];
  }
  if (tid == SCAN_THREADS - 1) {
    meta[SCAN_DONE] = 0;                 // ready for the next launch on this stream
    write_job_totals(off, toff, NB, meta, host_meta, s_a[tid], s_t[tid], s_t[tid], s_m[tid]);
  }
}
__global__ void __launch_bounds__(256) msm_scan_write(const uint32_t* __restrict__ cnt, uint32_t NB, uint32_t log_L,
                                                      const uint32_t* __restrict__ bsum, uint32_t* __restrict__ off,
                                                      uint32_t* __restrict__ ntask, uint32_t* __restrict__ toff) {
  side_kernel_prio();
  __shared__ uint32_t s_a[SCAN_THREADS], s_t[SCAN_THREADS];
  const uint32_t Lm1 = (1u << log_L) - 1, tid = threadIdx.x;
  uint32_t base = blockIdx.x * SCAN_BLOCK + tid * SCAN_ITEMS;
  uint32_t v[SCAN_ITEMS];
  uint32_t a = 0, t = 0;
#pragma unroll
  for (uint32_t k = 0; k < SCAN_ITEMS; k++) {
    v[k] = (base + k < NB) ? cnt[base + k] : 0;
    a += v[k];
    t += (v[k] + Lm1) >> log_L;
  }
  s_a[tid] = a; s_t[tid] = t;
  block_scan<2>(tid, SCAN_THREADS, true, s_a, s_t);
  uint32_t ra = bsum[3 * blockIdx.x] + s_a[tid] - a, rt = bsum[3 * blockIdx.x + 1] + s_t[tid] - t;
#pragma unroll
  for (uint32_t k = 0; k < SCAN_ITEMS; k++) {
    if (base + k < NB) {
      uint32_t nt = (v[k] + Lm1) >> log_L;
      if (off) off[base + k] = ra;
      ntask[base + k] = nt;
      toff[base + k] = rt;
      ra += v[k];
      rt += nt;
    }
  }
}

// ------------------------------------------------------------------ 4: single-pass sort, LDS-cursor scatter
// workgroup (p, j): cursors = bucket offset + this chunk's prefix, kept in LDS; every point
// of the chunk takes the next slot of its bucket with an LDS atomic.
__global__ void __launch_bounds__(1024) msm_scatter(const int16_t* __restrict__ dig, uint32_t n, uint32_t chunk,
                                                    uint32_t nbw, const uint32_t* __restrict__ hist,
                                                    const uint32_t* __restrict__ off, uint32_t collapse_W,
                                                    uint32_t n_tab, uint32_t* __restrict__ sorted) {
  side_kernel_prio();
  extern __shared__ uint32_t s_cur[];
  const uint32_t j = blockIdx.x, p = blockIdx.y, P = gridDim.y;
  // blockIdx.z = round r of R: only the buckets [r, r+1) * nbw / R are placed.  Every round re-reads
  // the (2-byte, coalesced) digits, but the 4-byte scattered stores of the workgroups in flight stay
  // inside 1/R of the output, so sectors fill up in L2 before they are written back.
  const uint32_t span = nbw / gridDim.z, b_lo = blockIdx.z * span;
  const uint32_t* pre = hist + ((size_t)j * P + p) * nbw + b_lo;
  // fixed-base mode (collapse_W = windows per MSM): the W windows of an MSM share ONE bucket set and an
  // entry names row (window, i) of the precomputed table  2^offset_w * P_i
  const uint32_t* ob = off + (size_t)(collapse_W ? j / collapse_W : j) * nbw + b_lo;
  const uint32_t base_idx = collapse_W ? (j % collapse_W) * n_tab : 0u;
  for (uint32_t b = threadIdx.x; b < span; b += blockDim.x) s_cur[b] = ob[b] + pre[b];
  __syncthreads();
  const uint32_t lo = p * chunk, hi = min(n, lo + chunk);
  const int16_t* row = dig + (size_t)j * n;
  for (uint32_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    int32_t d = row[i];
    uint32_t b = digit_bucket(d) - b_lo;   // d == 0 wraps to a huge value
    if (b < span) {
      uint32_t pos = atomicAdd(&s_cur[b], 1u);
      sorted[pos] = entry_word(base_idx + i, d);
    }
  }
}

// ------------------------------------------------------------------ 5: two-pass sort
// msm_scatter's 4-byte stores land all over the output (a workgroup holds chunk / nbw entries per
// bucket), and every one of them costs a 32-byte write to HBM.  The two-pass sort only ever writes
// runs: pass 1 partitions the digits into B coarse bins per bucket set (bin = bucket >> shift) through
// an LDS tile sort, so that a wave stores consecutive addresses; pass 2 gives each coarse bin to
// one workgroup, which counts its 2^shift buckets in LDS, emits the bucket counts and writes the
// bin's entries in bucket order, again from LDS.

// pass 1: grid (rows, P); row j / chunk p as in msm_hist.  chist holds the per-chunk exclusive
// prefixes (msm_hist_prefix), coff the bin offsets.  Output: (entry, bucket) pairs grouped by bin.
__global__ void __launch_bounds__(1024) msm_partition(const int16_t* __restrict__ dig, uint32_t n, uint32_t chunk,
                                                      uint32_t B, uint32_t shift, const uint32_t* __restrict__ chist,
                                                      const uint32_t* __restrict__ coff, uint32_t collapse_W,
                                                      uint32_t n_tab, uint32_t* __restrict__ part_entry,
                                                      uint16_t* __restrict__ part_fine) {
  side_kernel_prio();
  extern __shared__ uint32_t s_mem[];
  uint32_t* s_cnt = s_mem;                 // [B] tile counts, then tile bases
  uint32_t* s_base = s_cnt + B;            // [B]
  uint32_t* s_gcur = s_base + B;           // [B] global cursors of this (row, chunk)
  uint32_t* s_entry = s_gcur + B;          // [SORT_TILE]
  uint16_t* s_fine = reinterpret_cast<uint16_t*>(s_entry + SORT_TILE);  // [SORT_TILE]
  const uint32_t j = blockIdx.x, p = blockIdx.y, P = gridDim.y, tid = threadIdx.x;
  const uint32_t set = collapse_W ? j / collapse_W : j;
  const uint32_t base_idx = collapse_W ? (j % collapse_W) * n_tab : 0u;
  for (uint32_t b = tid; b < B; b += blockDim.x) s_gcur[b] = coff[(size_t)set * B + b] + chist[((size_t)j * P + p) * B + b];
  const uint32_t lo = p * chunk, hi = min(n, lo + chunk);
  const int16_t* row = dig + (size_t)j * n;
  constexpr uint32_t PER = SORT_TILE / 1024;
  for (uint32_t t0 = lo; t0 < hi; t0 += SORT_TILE) {
    for (uint32_t b = tid; b < B; b += blockDim.x) s_cnt[b] = 0;
    __syncthreads();
    int32_t d[PER];
    uint32_t rank[PER];
#pragma unroll
    for (uint32_t k = 0; k < PER; k++) {
      const uint32_t i = t0 + k * 1024 + tid;
      d[k] = i < hi ? (int32_t)row[i] : 0;
      if (d[k]) rank[k] = atomicAdd(&s_cnt[digit_bucket(d[k]) >> shift], 1u);
    }
    __syncthreads();
    // exclusive scan of the B tile counts (B <= 1024): s_base
    {
      uint32_t v = tid < B ? s_cnt[tid] : 0;
      if (tid < B) s_base[tid] = v;
      block_scan<1>(tid, B, tid < B, s_base);
      if (tid < B) s_base[tid] -= v;
      __syncthreads();
    }
#pragma unroll
    for (uint32_t k = 0; k < PER; k++) {
      if (d[k]) {
        const uint32_t fine = digit_bucket(d[k]);
        const uint32_t slot = s_base[fine >> shift] + rank[k];
        s_entry[slot] = entry_word(base_idx + t0 + k * 1024 + tid, d[k]);
        s_fine[slot] = (uint16_t)fine;
      }
    }
    __syncthreads();
    const uint32_t total = s_base[B - 1] + s_cnt[B - 1];
    for (uint32_t slot = tid; slot < total; slot += blockDim.x) {
      const uint32_t fine = s_fine[slot], bin = fine >> shift;
      const uint32_t g = s_gcur[bin] + (slot - s_base[bin]);
      part_entry[g] = s_entry[slot];
      part_fine[g] = (uint16_t)fine;
    }
    __syncthreads();
    for (uint32_t b = tid; b < B; b += blockDim.x) s_gcur[b] += s_cnt[b];
    __syncthreads();
  }
}

// pass 2: one workgroup per (set, coarse bin): F = 2^shift buckets.  counts[set*nbw + bin*F + f] and
// the bin's slice of `sorted` in bucket order.
//
// FE, the pass that also closes the front end (msm_fine_sort_fused).  A workgroup owns a coarse bin whose entry offset (coff)
// and task-slot base (tbase) are known from the coarse scan, so everything the bucket-level scans produce is local to it:
// off[b] = start + exclusive count prefix, ntask[b] = ceil(c / L), toff[b] = tbase + exclusive task prefix (the task index space
// has gaps at the end of every bin: consumers only ever index partial[toff[b] + seg]).  What is global -- the number of tasks,
// the largest bucket, the histogram of task lengths that orders the tasks longest first -- leaves the workgroup as
// fire-and-forget atomics into one of FE_REPL replicas (thousands of workgroups adding to ONE word per length cost a millisecond
// of serialised atomics) and is summed by the NEXT kernel of the job (msm_task_scatter_reserve), where the kernel boundary has
// made it complete: no workgroup waits for a return value or for another workgroup, and there is no release fence -- in this
// kernel a fence writes back an L2 that has just been filled with sorted entries, once per workgroup: a millisecond
// (profiles/r05_sweeps/frontend.txt has all three measurements).  msm_scan_sums, msm_scan_write, msm_task_hist and msm_task_scan
// are not in that job's chain.
struct FrontEndOut {
  uint32_t* off;
  uint32_t* ntask;
  uint32_t* toff;
  const uint32_t* tbase;
  uint32_t* fe;
  uint32_t log_L, parity;
};
// dynamic LDS: (2F + nthr + SORT_TILE) words, FE (2F + 2 nthr + SORT_TILE); s_th [TASK_BINS] and s_red [2] (tasks of the bin,
// largest count) are the fused kernel's own static LDS
template <bool FE>
__device__ __forceinline__ void fine_sort_body(const uint32_t* __restrict__ part_entry, const uint16_t* __restrict__ part_fine,
                                               const uint32_t* __restrict__ coff, const uint32_t* __restrict__ ccnt, uint32_t B,
                                               uint32_t shift, uint32_t nbw, uint32_t* __restrict__ counts,
                                               uint32_t* __restrict__ sorted, const FrontEndOut& o, uint32_t* s_th,
                                               uint32_t* s_red) {
  extern __shared__ uint32_t s_mem[];
  const uint32_t F = 1u << shift, tid = threadIdx.x, nthr = blockDim.x;
  uint32_t* s_cnt = s_mem;        // [F] counts, then cursors
  uint32_t* s_ofs = s_cnt + F;    // [F] exclusive offsets
  uint32_t* s_part = s_ofs + F;   // [nthr] scan scratch (FE: 64-bit words, over the start of s_out, which is not in use yet)
  uint32_t* s_out = s_part + nthr;  // [SORT_TILE]
  const uint32_t start = coff[blockIdx.x], E = ccnt[blockIdx.x];
  const uint32_t set = blockIdx.x / B, bin = blockIdx.x - set * B;
  if constexpr (FE) {
    // housekeeping for the jobs to come: the other replica set and the scatter's cursors back to zero (whoever used them last
    // has finished: same stream)
    uint32_t* other = o.fe + FE_SET + (o.parity ^ 1u) * FE_SET_WORDS;
    for (uint32_t row = blockIdx.x; row < FE_REPL; row += gridDim.x)
      for (uint32_t k = tid; k < FE_ROW; k += nthr) other[row * FE_ROW + k] = 0;
    if (blockIdx.x == 0)
      for (uint32_t k = tid; k < TASK_BINS; k += nthr) o.fe[FE_CURSOR + k] = 0;
  }
  for (uint32_t f = tid; f < F; f += nthr) s_cnt[f] = 0;
  if constexpr (FE) {
    for (uint32_t k = tid; k < TASK_BINS; k += nthr) s_th[k] = 0;
    if (tid < 2) s_red[tid] = 0;
  }
  __syncthreads();
  for (uint32_t i = tid; i < E; i += nthr) atomicAdd(&s_cnt[part_fine[start + i] & (F - 1)], 1u);
  __syncthreads();
  // exclusive scan over F (FE: of entries and tasks, the two sums packed in a 64-bit word): contiguous share per thread + ONE
  // Hillis-Steele over the shares
  const uint32_t per = (F + nthr - 1) / nthr, f0 = min(tid * per, F), f1 = min(f0 + per, F);
  const uint32_t Lm1 = (1u << o.log_L) - 1;
  uint32_t a = 0, t = 0, mx = 0;
  for (uint32_t f = f0; f < f1; f++) {
    const uint32_t c = s_cnt[f];
    a += c;
    if constexpr (FE) {
      t += (c + Lm1) >> o.log_L;
      mx = max(mx, c);
      count_bucket_tasks(s_th, c, o.log_L);
    }
  }
  using scan_t = std::conditional_t<FE, uint64_t, uint32_t>;
  scan_t* s_scan = reinterpret_cast<scan_t*>(s_part);
  if constexpr (FE) s_scan[tid] = ((uint64_t)t << 32) | a;
  else s_scan[tid] = a;
  block_scan<1>(tid, nthr, true, s_scan);
  uint32_t run = (uint32_t)s_scan[tid] - a, trun = 0;
  const size_t b_first = (size_t)set * nbw + (size_t)bin * F;
  if constexpr (FE) {
    trun = o.tbase[blockIdx.x] + (uint32_t)(s_scan[tid] >> 32) - t;
    if (t) atomicAdd(&s_red[0], t);
    if (mx) atomicMax(&s_red[1], mx);
  }
  uint32_t* cout = counts + b_first;
  for (uint32_t f = f0; f < f1; f++) {
    const uint32_t c = s_cnt[f];
    cout[f] = c;
    s_ofs[f] = run;
    if constexpr (FE) {
      const uint32_t nt = (c + Lm1) >> o.log_L;
      o.off[b_first + f] = start + run;
      o.ntask[b_first + f] = nt;
      o.toff[b_first + f] = trun;
      trun += nt;
    }
    run += c;
  }
  __syncthreads();
  if constexpr (FE) {
    // the bin's share of the global figures: fire and forget
    uint32_t* mine = o.fe + FE_SET + o.parity * FE_SET_WORDS + (blockIdx.x % FE_REPL) * FE_ROW;
    for (uint32_t k = tid; k <= task_full_bin(o.log_L); k += nthr)
      if (s_th[k]) atomicAdd(mine + 2 + k, s_th[k]);
    if (tid == 0) {
      if (s_red[0]) atomicAdd(mine, s_red[0]);
      if (s_red[1]) atomicMax(mine + 1, s_red[1]);
    }
  }
  for (uint32_t f = tid; f < F; f += nthr) s_cnt[f] = s_ofs[f];   // cursors
  __syncthreads();
  if (E <= SORT_TILE) {
    for (uint32_t i = tid; i < E; i += nthr) {
      const uint32_t pos = atomicAdd(&s_cnt[part_fine[start + i] & (F - 1)], 1u);
      s_out[pos] = part_entry[start + i];
    }
    __syncthreads();
    for (uint32_t i = tid; i < E; i += nthr) sorted[start + i] = s_out[i];
  } else {  // oversized bin (skewed scalars): place directly; the region belongs to this workgroup alone
    for (uint32_t i = tid; i < E; i += nthr) {
      const uint32_t pos = atomicAdd(&s_cnt[part_fine[start + i] & (F - 1)], 1u);
      sorted[start + pos] = part_entry[start + i];
    }
  }
}
__global__ void __launch_bounds__(512) msm_fine_sort(const uint32_t* __restrict__ part_entry,
                                                     const uint16_t* __restrict__ part_fine,
                                                     const uint32_t* __restrict__ coff,
                                                     const uint32_t* __restrict__ ccnt, uint32_t B, uint32_t shift,
                                                     uint32_t nbw, uint32_t* __restrict__ counts,
                                                     uint32_t* __restrict__ sorted) {
  side_kernel_prio();
  fine_sort_body<false>(part_entry, part_fine, coff, ccnt, B, shift, nbw, counts, sorted, FrontEndOut{}, nullptr, nullptr);
}
__global__ void __launch_bounds__(512) msm_fine_sort_fused(const uint32_t* __restrict__ part_entry,
                                                           const uint16_t* __restrict__ part_fine,
                                                           const uint32_t* __restrict__ coff,
                                                           const uint32_t* __restrict__ ccnt, uint32_t B, uint32_t shift,
                                                           uint32_t nbw, uint32_t* __restrict__ counts,
                                                           uint32_t* __restrict__ sorted, FrontEndOut o) {
  side_kernel_prio();
  __shared__ uint32_t s_th[TASK_BINS];
  __shared__ uint32_t s_red[2];
  fine_sort_body<true>(part_entry, part_fine, coff, ccnt, B, shift, nbw, counts, sorted, o, s_th, s_red);
}

// ------------------------------------------------------------------ 6: task ordering
// Longest tasks first, equal lengths side by side, so the 64 lanes of a wave run the same number of additions (bucket sizes
// are Poisson-distributed: without this a wave waits for its largest bucket, ~30 % of the lanes' time idle).

// thist[bin * nblk + blk] = number of tasks of (clamped) length `bin` in block blk
__global__ void __launch_bounds__(256) msm_task_hist(const uint32_t* __restrict__ cnt, uint32_t NB,
                                                     uint32_t log_L, uint32_t task_block,
                                                     uint32_t* __restrict__ thist) {
  side_kernel_prio();
  __shared__ uint32_t s_h[TASK_BINS];
  for (uint32_t k = threadIdx.x; k < TASK_BINS; k += blockDim.x) s_h[k] = 0;
  __syncthreads();
  count_block_tasks(s_h, cnt, NB, log_L, task_block);
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < TASK_BINS; k += blockDim.x) thist[k * gridDim.x + blockIdx.x] = s_h[k];
}
// one workgroup: exclusive scan of thist in DESCENDING bin order (bin-major, block-minor) over the nbins = L + 1 bins in
// use; total = nbins * nblk <= 32 Ki entries.  256 lanes with a handful of registers, two passes over the entries (the
// second one hits L2): the former 1024 lanes x 98 registers needed a whole CU's register file at once and, beside a
// running accumulation, waited for that accumulation to END -- a millisecond on the path of the next job.
__global__ void __launch_bounds__(256) msm_task_scan(uint32_t* __restrict__ thist, uint32_t nblk, uint32_t nbins,
                                                     uint32_t* __restrict__ ticket) {
  side_kernel_prio();
  __shared__ uint32_t s_sum[256];
  if (threadIdx.x == 0) *ticket = 0;   // msm_accumulate's task counter (next launch on this stream)
  const uint32_t total = nbins * nblk, tid = threadIdx.x;
  const uint32_t per = (total + 255) / 256;
  const uint32_t lo = min(tid * per, total), hi = min(lo + per, total);
  // position q in scan order <-> entry (nbins-1 - q / nblk) * nblk + q % nblk
  const uint32_t row0 = lo / nblk, col0 = lo - row0 * nblk;
  uint32_t a = 0;
  {
    uint32_t row = row0, col = col0;
#pragma unroll 8
    for (uint32_t q = lo; q < hi; q++) {
      a += thist[(nbins - 1 - row) * nblk + col];
      if (++col == nblk) { col = 0; row++; }
    }
  }
  s_sum[tid] = a;
  block_scan<1>(tid, 256, true, s_sum);
  uint32_t run = s_sum[tid] - a;
  {
    uint32_t row = row0, col = col0;
    for (uint32_t q = lo; q < hi; q++) {
      const uint32_t idx = (nbins - 1 - row) * nblk + col;
      const uint32_t v = thist[idx];
      thist[idx] = run;
      run += v;
      if (++col == nblk) { col = 0; row++; }
    }
  }
}
// order[pos] = (bucket, segment) of the task that runs as thread `pos`
__global__ void __launch_bounds__(256) msm_task_scatter(const uint32_t* __restrict__ cnt, uint32_t NB,
                                                        uint32_t log_L, uint32_t task_block,
                                                        const uint32_t* __restrict__ thist,
                                                        uint2* __restrict__ order) {
  side_kernel_prio();
  __shared__ uint32_t s_c[TASK_BINS];
  for (uint32_t k = threadIdx.x; k < TASK_BINS; k += blockDim.x) s_c[k] = thist[k * gridDim.x + blockIdx.x];
  __syncthreads();
  place_bucket_tasks(s_c, cnt, NB, log_L, task_block, order);
}

// the same after msm_fine_sort_fused: every workgroup first sums the replicas of the task-length histogram the sort left (the
// kernel boundary made them complete) into the positions at which each length starts in `order` (descending lengths), counts
// its own tasks per length, reserves their positions with one atomic per length on the running cursors, and places them --
// msm_task_hist and msm_task_scan are not needed.  Workgroup 0 also hands the job's totals to the accumulation and to the host.
// (Tasks of one length come in the order the reservations happen to be served: which lane runs which task is free, the sums
// are the same.)
struct FrontEndTotals {
  uint32_t* fe;
  const uint32_t* coff;           // [NBc]: entries of the job
  const uint32_t* tbase;          // [NBc]: task slots of the job
  uint32_t* off;                  // off[NB] <- entries
  uint32_t* toff;                 // toff[NB] <- task slots
  uint32_t* meta;                 // [0] entries, [1] tasks, [2] largest count; [ticket_word] <- 0
  volatile uint32_t* host_meta;   // the same three for the host (mapped page-locked memory)
  uint32_t NBc, parity, ticket_word;
};
__global__ void __launch_bounds__(256) msm_task_scatter_reserve(const uint32_t* __restrict__ cnt, uint32_t NB,
                                                                uint32_t log_L, uint32_t task_block, FrontEndTotals ft,
                                                                uint2* __restrict__ order) {
  side_kernel_prio();
  __shared__ uint32_t s_c[TASK_BINS], s_tot[TASK_BINS], s_red[2];
  const uint32_t tid = threadIdx.x;
  const uint32_t nbins = task_full_bin(log_L) + 1;
  const uint32_t* set = ft.fe + FE_SET + ft.parity * FE_SET_WORDS;
  for (uint32_t k = tid; k < TASK_BINS; k += blockDim.x) { s_c[k] = 0; s_tot[k] = 0; }
  if (tid < 2) s_red[tid] = 0;
  __syncthreads();
  for (uint32_t idx = tid; idx < nbins * FE_REPL; idx += blockDim.x) {
    const uint32_t k = idx % nbins, r = idx / nbins;
    const uint32_t v = set[r * FE_ROW + 2 + k];
    if (v) atomicAdd(&s_tot[k], v);
  }
  if (blockIdx.x == 0 && tid < FE_REPL) {
    const uint32_t tk = set[tid * FE_ROW], mxr = set[tid * FE_ROW + 1];
    if (tk) atomicAdd(&s_red[0], tk);
    if (mxr) atomicMax(&s_red[1], mxr);
  }
  count_block_tasks(s_c, cnt, NB, log_L, task_block);
  __syncthreads();
  if (blockIdx.x == 0 && tid == 0) {
    ft.meta[ft.ticket_word] = 0;          // msm_accumulate's task counter (the next launch on this stream)
    write_job_totals(ft.off, ft.toff, NB, ft.meta, ft.host_meta, ft.coff[ft.NBc], ft.tbase[ft.NBc], s_red[0], s_red[1]);
  }
  // position of this workgroup's tasks of length k: every longer task first, then what other workgroups reserved before
  for (uint32_t k = tid; k < nbins; k += blockDim.x) {
    uint32_t base = 0;
    for (uint32_t k2 = k + 1; k2 < nbins; k2++) base += s_tot[k2];
    const uint32_t mine = s_c[k];
    s_c[k] = base + (mine ? atomicAdd(ft.fe + FE_CURSOR + k, mine) : 0u);
  }
  __syncthreads();
  place_bucket_tasks(s_c, cnt, NB, log_L, task_block, order);
}

// the same three scans for NB <= 4 Ki buckets in ONE workgroup (a small MSM is a chain of ~25 launches with
// a ~5 us floor each; this replaces four of them -- memset + three kernels -- per scan): thread t owns
// buckets [t*per, (t+1)*per)
__global__ void __launch_bounds__(1024) msm_scan_small(const uint32_t* __restrict__ cnt, uint32_t NB, uint32_t log_L,
                                                       uint32_t* __restrict__ off, uint32_t* __restrict__ ntask,
                                                       uint32_t* __restrict__ toff, uint32_t* __restrict__ meta,
                                                       volatile uint32_t* host_meta) {
  side_kernel_prio();
  __shared__ uint32_t s_a[1024], s_t[1024], s_m[1024];
  const uint32_t Lm1 = (1u << log_L) - 1, tid = threadIdx.x;
  const uint32_t per = (NB + 1023) / 1024, lo = min(tid * per, NB);
  uint32_t v[SCAN_SMALL_PER];                      // all loads of a thread in flight together
#pragma unroll
  for (uint32_t k = 0; k < SCAN_SMALL_PER; k++) v[k] = (k < per && lo + k < NB) ? cnt[lo + k] : 0u;
  uint32_t a = 0, t = 0, m = 0;
#pragma unroll
  for (uint32_t k = 0; k < SCAN_SMALL_PER; k++) {
    a += v[k];
    t += (v[k] + Lm1) >> log_L;
    m = max(m, v[k]);
  }
  s_a[tid] = a; s_t[tid] = t; s_m[tid] = m;
  block_scan<3, true>(tid, 1024, true, s_a, s_t, s_m);
  uint32_t ra = s_a[tid] - a, rt = s_t[tid] - t;
#pragma unroll
  for (uint32_t k = 0; k < SCAN_SMALL_PER; k++) {
    if (k < per && lo + k < NB) {
      const uint32_t nt = (v[k] + Lm1) >> log_L;
      if (off) off[lo + k] = ra;
      ntask[lo + k] = nt;
      toff[lo + k] = rt;
      ra += v[k];
      rt += nt;
    }
  }
  if (tid == 1023) write_job_totals(off, toff, NB, meta, host_meta, s_a[tid], s_t[tid], s_t[tid], s_m[tid]);
}

// exclusive scans over NB buckets (one launch for small NB, else two); host_meta: see write_job_totals
static hipError_t launch_scan(const uint32_t* cnt, uint32_t NB, uint32_t log_L, uint32_t* off, uint32_t* ntask,
                              uint32_t* toff, uint32_t* bsum, uint32_t* meta, hipStream_t stream, uint32_t* host_meta = nullptr) {
  if (NB <= SCAN_SMALL_PER * 1024) {
    msm_scan_small<<<1, 1024, 0, stream>>>(cnt, NB, log_L, off, ntask, toff, meta, host_meta);
    return hipGetLastError();
  }
  const uint32_t nblk = (NB + SCAN_BLOCK - 1) / SCAN_BLOCK;
  if (nblk > 1024) return hipErrorInvalidValue;
  msm_scan_sums<<<nblk, SCAN_THREADS, 0, stream>>>(cnt, NB, log_L, bsum, meta, off, toff, host_meta);   // + the scan of the block sums
  msm_scan_write<<<nblk, SCAN_THREADS, 0, stream>>>(cnt, NB, log_L, bsum, off, ntask, toff);
  return hipGetLastError();
}

}  // namespace sg
