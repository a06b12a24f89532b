// MSM engine, part 3 of 3 (included once by msm.hip): the bucket reductions (scan-based and 2-D) and the export kernels.
#pragma once
#include "msm.h"
#include "side_prio.cuh"

namespace sg {

// ------------------------------------------------------------------ 5: bucket reduction
// Window sum = sum_b (b+1) * B_b.  No doublings run on the GPU: every level only adds, and
// the power-of-two weights are applied by the host tail, where a dependent chain of point
// doublings costs a fraction of a microsecond per step instead of several on one GPU lane.
//
// level 0: thread t of window j owns G = 2^log_G consecutive buckets: run_t = sum B,
//          acc_t = sum (k+1) B_{first+k} (running sums).  A workgroup w of N threads emits
//             A_w = sum_t acc_t,  S_w = sum_t t * run_t (= sum_{t>=1} Suf_t),  R_w = sum_t run_t
//          so that  window = sum_w [ A_w + G * S_w + G * N * w * R_w ].
// level 1: one workgroup per window:  A = sum A_w,  S = sum S_w,  T = sum_w w * R_w.
// host:    window = A + 2^log_G * (S + 2^log_N * T).
struct ReduceOut {
  xyzz29_mem* a;
  xyzz29_mem* s;
  xyzz29_mem* r;
};
// tree-sum of arr[0..len) (len a power of two) by logical threads li = 0..len/2-1 of a group;
// every thread of the workgroup must call it (barriers inside)
template <int Q>
__device__ __forceinline__ void tree_sum(xyzz29_mem* arr, uint32_t len, uint32_t li, uint32_t role, bool member) {
  for (uint32_t s = len >> 1; s >= 1; s >>= 1) {
    if (member && li < s) {
      xyzz29 a = xyzz29_load(&arr[li]);
      add_q<Q>(a, xyzz29_load(&arr[li + s]), role);
      if (role == 0) xyzz29_store(&arr[li], a);
    }
    __syncthreads();
  }
}
// in-place suffix scan of arr[0..N) by N logical threads (Hillis-Steele)
template <int Q>
__device__ __forceinline__ xyzz29 suffix_scan(xyzz29_mem* arr, xyzz29 mine, uint32_t N, uint32_t lt, uint32_t role) {
  if (role == 0) xyzz29_store(&arr[lt], mine);
  __syncthreads();
  for (uint32_t d = 1; d < N; d <<= 1) {
    xyzz29 other = xyzz29_identity();
    if (lt + d < N) other = xyzz29_load(&arr[lt + d]);
    __syncthreads();
    add_q<Q>(mine, other, role);
    if (role == 0) xyzz29_store(&arr[lt], mine);
    __syncthreads();
  }
  return mine;
}

// level 0: grid (blocks, W), N = blockDim.x / Q logical threads (power of two >= 16)
template <int Q>
__device__ __forceinline__ void reduce_buckets_body(const xyzz29_mem* __restrict__ partial, const uint32_t* __restrict__ toff,
                                                    const uint32_t* __restrict__ ntask, uint32_t nbw, uint32_t log_G,
                                                    ReduceOut out) {
  side_kernel_prio();
  extern __shared__ uint4 smem[];
  const uint32_t N = blockDim.x / Q, lt = threadIdx.x / Q, role = threadIdx.x % Q;
  xyzz29_mem* sA = reinterpret_cast<xyzz29_mem*>(smem);
  xyzz29_mem* sR = sA + N;
  const uint32_t chunk = blockIdx.x * N + lt;
  const uint32_t G = 1u << log_G;
  xyzz29 acc = xyzz29_identity(), run = xyzz29_identity();
  const uint32_t first = chunk << log_G;
  if (first < nbw) {
    const uint32_t wbase = blockIdx.y * nbw;
    auto fetch = [&](uint32_t k) {
      const uint32_t b = first + k;
      xyzz29 v = xyzz29_identity();   // (not "c ? load : identity": two temporaries behind a pointer phi stay in scratch)
      if (b < nbw && ntask[wbase + b]) v = xyzz29_load(partial + toff[wbase + b]);
      return v;
    };
    xyzz29 nxt = fetch(G - 1);
    for (uint32_t k = G; k-- > 0;) {
      const xyzz29 cur = nxt;
      if (k) nxt = fetch(k - 1);  // in flight while the two additions below run
      add_q<Q>(run, cur, role);
      add_q<Q>(acc, run, role);
    }
  }
  const uint32_t o = blockIdx.y * gridDim.x + blockIdx.x;
  if (role == 0) xyzz29_store(&sA[lt], acc);
  suffix_scan<Q>(sR, run, N, lt, role);            // sR[t] = Suf_t
  if (threadIdx.x == 0) {
    xyzz29_store(out.r + o, xyzz29_load(&sR[0]));
    xyzz29_store(&sR[0], xyzz29_identity());  // S sums t >= 1 only
  }
  __syncthreads();
  // two tree sums side by side: lower half of the logical threads folds sA, upper half sR
  const uint32_t halfN = N >> 1;
  xyzz29_mem* arr = (lt < halfN) ? sA : sR;
  tree_sum<Q>(arr, N, (lt < halfN) ? lt : lt - halfN, role, true);
  if (threadIdx.x == 0) xyzz29_store(out.a + o, xyzz29_load(&sA[0]));
  if (lt == halfN && role == 0) xyzz29_store(out.s + o, xyzz29_load(&sR[0]));
}
template <int Q>
__global__ void __launch_bounds__(256) msm_reduce_buckets(const xyzz29_mem* __restrict__ partial,
                                                          const uint32_t* __restrict__ toff,
                                                          const uint32_t* __restrict__ ntask, uint32_t nbw,
                                                          uint32_t log_G, ReduceOut out) {
  reduce_buckets_body<Q>(partial, toff, ntask, nbw, log_G, out);
}
// the same within 168 registers (60 values live in scratch, +5 %): a wave of it fits beside two waves of msm_accumulate on
// a SIMD, so the reduction of one job runs under the accumulation of the next instead of after it
template <int Q>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3)))
msm_reduce_buckets_lean(const xyzz29_mem* __restrict__ partial, const uint32_t* __restrict__ toff,
                        const uint32_t* __restrict__ ntask, uint32_t nbw, uint32_t log_G, ReduceOut out) {
  reduce_buckets_body<Q>(partial, toff, ntask, nbw, log_G, out);
}
// level 1: grid (1, W), blockDim = 3 * T1 * Q (T1 a power of two >= count): group 0 scans/folds
// the R items, group 1 folds A, group 2 folds S
template <int Q>
__global__ void __launch_bounds__(768) msm_reduce_items(ReduceOut in, uint32_t count, uint32_t T1, ReduceOut out) {
  side_kernel_prio();
  extern __shared__ uint4 smem[];
  xyzz29_mem* sR = reinterpret_cast<xyzz29_mem*>(smem);
  xyzz29_mem* sA = sR + T1;
  xyzz29_mem* sS = sA + T1;
  const uint32_t lt = threadIdx.x / Q, role = threadIdx.x % Q;
  const uint32_t g = lt / T1, li = lt - g * T1;
  const uint32_t base = blockIdx.y * count;
  xyzz29 v = xyzz29_identity();
  if (li < count) v = xyzz29_load((g == 0 ? in.r : g == 1 ? in.a : in.s) + base + li);
  if (role == 0) {
    if (g == 1) xyzz29_store(&sA[li], v);
    if (g == 2) xyzz29_store(&sS[li], v);
    // suffix scan of R (group 0 works, everyone keeps the barriers)
    if (g == 0) xyzz29_store(&sR[li], v);
  }
  __syncthreads();
  for (uint32_t d = 1; d < T1; d <<= 1) {
    xyzz29 other = xyzz29_identity();
    if (g == 0 && li + d < T1) other = xyzz29_load(&sR[li + d]);
    __syncthreads();
    if (g == 0) {
      add_q<Q>(v, other, role);
      if (role == 0) xyzz29_store(&sR[li], v);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) xyzz29_store(&sR[0], xyzz29_identity());  // T sums w >= 1 only
  __syncthreads();
  xyzz29_mem* arr = g == 0 ? sR : g == 1 ? sA : sS;
  tree_sum<Q>(arr, T1, li, role, true);
  if (li == 0 && role == 0) xyzz29_store((g == 0 ? out.r : g == 1 ? out.a : out.s) + blockIdx.y, xyzz29_load(&arr[0]));
}
// ------------------------------------------------------------------ 5b: 2-D bucket reduction (few bucket sets)
// The scan-based reduction above is a chain of ~40 dependent additions whatever the size.  With the bucket index
// split as b = hi * C + lo (C = 2^ceil(bits/2) columns, Rr = nbw / C rows),
//     sum_b (b + 1) B_b = C * sum_hi hi * R_hi + sum_lo lo * C_lo + U,   R_hi / C_lo row / column sums, U the total,
// and each small weighted sum by bits,  sum_x x * V_x = sum_j 2^j * (sum of the V_x with bit j of x set),
// everything on the device is a PLAIN sum: lines (rows and columns) first, then one masked sum per bit --
// two launches of ~9 dependent quad-cooperative additions each.  The powers of two are applied by the host tail,
// which already places terms at bit offsets; it receives bits + 1 points per bucket set, so this path is for
// jobs with few sets (fixed-base commits of up to 4 polynomials).
struct Reduce2dShape {
  uint32_t log_cols, log_rows;  // nbw = 2^(log_rows + log_cols)
};
// sum of up to 256 XYZZ values by one workgroup of 256 lanes: Q = 4: 64 quads (quad-cooperative additions, for
// few sets: latency), Q = 1: 256 lanes, one addition each (many sets: throughput); `get(e)` yields element e
template <int Q, typename F>
__device__ __forceinline__ xyzz29 wg_sum(uint32_t n, F get, xyzz29_mem* lds) {
  constexpr uint32_t NL = 256 / Q;  // logical threads
  const uint32_t lt = threadIdx.x / Q, role = threadIdx.x % Q;
  xyzz29 acc = xyzz29_identity();
  // (round 5: loading the next element while the addition runs was measured and is slower -- 366 -> 406 us of line sums per proof:
  // 185 registers instead of 149, and the loads of a quad's two to four elements are back to back anyway)
  for (uint32_t e = lt; e < n; e += NL) add_q<Q>(acc, get(e), role);
  if (role == 0) xyzz29_store(&lds[lt], acc);
  __syncthreads();
  tree_sum<Q>(lds, NL, lt, role, true);
  return xyzz29_load(&lds[0]);
}
// the same with `get(e, acc, role)` adding element e -- possibly several terms -- into the running sum itself
template <int Q, typename F>
__device__ __forceinline__ xyzz29 wg_sum_into(uint32_t n, F get, xyzz29_mem* lds) {
  constexpr uint32_t NL = 256 / Q;  // logical threads
  const uint32_t lt = threadIdx.x / Q, role = threadIdx.x % Q;
  xyzz29 acc = xyzz29_identity();
  for (uint32_t e = lt; e < n; e += NL) get(e, acc, role);
  if (role == 0) xyzz29_store(&lds[lt], acc);
  __syncthreads();
  tree_sum<Q>(lds, NL, lt, role, true);
  return xyzz29_load(&lds[0]);
}
// A bucket of a fixed-base job owns several partial sums (one per accumulation task: ~64 entries in tasks of 16).  The
// line sums below used to add them on the way -- twice, once in the row pass and once in the column pass, and with
// quad-cooperative additions (2.5 lanes' worth of issue slots each): 2 x 4.5 quad-additions per bucket where the sums
// themselves need 2.  This pass adds them ONCE, one logical thread per bucket, and leaves one value per bucket in
// bucket order, so the line sums read plain coalesced arrays.  Q = 4 (a quad per bucket) while the job is small enough
// for every bucket to get its quad at once (one bucket set: 2^15 quads), Q = 1 beyond.  grid: NB logical threads.
template <int Q>
__global__ void __launch_bounds__(256) msm_fold_buckets(const xyzz29_mem* __restrict__ partial, const uint32_t* __restrict__ toff,
                                                        const uint32_t* __restrict__ ntask, uint32_t NB,
                                                        xyzz29_mem* __restrict__ folded) {
  side_kernel_prio();
  const uint32_t b = (blockIdx.x * blockDim.x + threadIdx.x) / Q, role = threadIdx.x % Q;
  if (b >= NB) return;
  const uint32_t nt = ntask[b], t0 = toff[b];
  xyzz29 acc = xyzz29_identity();
  if (nt) {
    acc = xyzz29_load(partial + t0);
    xyzz29 nxt = acc;
    if (nt > 1) nxt = xyzz29_load(partial + t0 + 1);
    for (uint32_t t = 1; t < nt; t++) {
      const xyzz29 cur = nxt;
      if (t + 1 < nt) nxt = xyzz29_load(partial + t0 + t + 1);   // in flight while the addition below runs
      add_q<Q>(acc, cur, role);
    }
  }
  if (role == 0) xyzz29_store(folded + b, acc);
}
// grid (rows + cols, sets): line sums over folded buckets (one value per bucket, bucket order).  lines[set * (rows + cols) + L]
template <int Q>
__global__ void __launch_bounds__(256) msm_reduce2d_lines_folded(const xyzz29_mem* __restrict__ folded, Reduce2dShape sh,
                                                                 xyzz29_mem* __restrict__ lines) {
  side_kernel_prio();
  __shared__ xyzz29_mem lds[256 / Q];
  const uint32_t rows = 1u << sh.log_rows, cols = 1u << sh.log_cols, L = blockIdx.x, set = blockIdx.y;
  const xyzz29_mem* src = folded + ((size_t)set << (sh.log_rows + sh.log_cols));
  const bool is_row = L < rows;
  const uint32_t n = is_row ? cols : rows;
  xyzz29 sum = wg_sum<Q>(n, [&](uint32_t e) {
    return xyzz29_load(src + (is_row ? (L << sh.log_cols) + e : (e << sh.log_cols) + (L - rows)));
  }, lds);
  if (threadIdx.x == 0) xyzz29_store(lines + (size_t)set * (rows + cols) + L, sum);
}
// (the one-launch form: line sums that add a bucket's partial sums themselves; msm.red2d_prefold = 0)
// grid (rows + cols, sets): line sums.  lines[set * (rows + cols) + L]
template <int Q>
__global__ void __launch_bounds__(256) msm_reduce2d_lines(const xyzz29_mem* __restrict__ partial,
                                                          const uint32_t* __restrict__ toff,
                                                          const uint32_t* __restrict__ ntask, Reduce2dShape sh,
                                                          xyzz29_mem* __restrict__ lines) {
  side_kernel_prio();
  __shared__ xyzz29_mem lds[256 / Q];
  const uint32_t rows = 1u << sh.log_rows, cols = 1u << sh.log_cols, L = blockIdx.x, set = blockIdx.y;
  const uint32_t base = set << (sh.log_rows + sh.log_cols);
  const bool is_row = L < rows;
  const uint32_t n = is_row ? cols : rows;
  // a bucket owns ntask[b] partial sums (one per accumulation task; several when the heavy-bucket merge was folded in
  // here: the line sums add them on the way, which costs the few extra additions of a merge round without its launches)
  auto get = [&](uint32_t e, xyzz29& acc, uint32_t role) {
    const uint32_t b = base + (is_row ? (L << sh.log_cols) + e : (e << sh.log_cols) + (L - rows));
    const uint32_t nt = ntask[b], t0 = toff[b];
    for (uint32_t t = 0; t < nt; t++) add_q<Q>(acc, xyzz29_load(partial + t0 + t), role);
  };
  xyzz29 sum = wg_sum_into<Q>(n, get, lds);
  if (threadIdx.x == 0) xyzz29_store(lines + (size_t)set * (rows + cols) + L, sum);
}
// grid (log_rows + log_cols + 1, sets): WG j < log_cols: columns with bit j of lo set; next log_rows: rows with
// bit j' of hi set; last: all columns (= the total).  out[set * (bits + 1) + j]
template <int Q>
__global__ void __launch_bounds__(256) msm_reduce2d_bits(const xyzz29_mem* __restrict__ lines, Reduce2dShape sh,
                                                         xyzz29_mem* __restrict__ out) {
  side_kernel_prio();
  __shared__ xyzz29_mem lds[256 / Q];
  const uint32_t rows = 1u << sh.log_rows, cols = 1u << sh.log_cols, j = blockIdx.x, set = blockIdx.y;
  const uint32_t bits = sh.log_rows + sh.log_cols;
  const xyzz29_mem* ln = lines + (size_t)set * (rows + cols);
  xyzz29 sum;
  if (j < sh.log_cols) {
    sum = wg_sum<Q>(cols, [&](uint32_t e) {
      xyzz29 v = xyzz29_identity();
      if ((e >> j) & 1) v = xyzz29_load(ln + rows + e);
      return v;
    }, lds);
  } else if (j < bits) {
    const uint32_t jr = j - sh.log_cols;
    sum = wg_sum<Q>(rows, [&](uint32_t e) {
      xyzz29 v = xyzz29_identity();
      if ((e >> jr) & 1) v = xyzz29_load(ln + e);
      return v;
    }, lds);
  } else {
    sum = wg_sum<Q>(cols, [&](uint32_t e) { return xyzz29_load(ln + rows + e); }, lds);
  }
  if (threadIdx.x == 0) xyzz29_store(out + (size_t)set * (bits + 1) + j, sum);
}
// many sets: the powers of two on the device as well -- thread t doubles term t t times (<= 14 doublings), then
// a tree sum: one point per set.  grid (sets), 32 threads
__global__ void __launch_bounds__(32) msm_reduce2d_combine(const xyzz29_mem* __restrict__ terms, uint32_t bits,
                                                           xyzz29_mem* __restrict__ out) {
  side_kernel_prio();
  __shared__ xyzz29_mem lds[32];
  const uint32_t t = threadIdx.x, set = blockIdx.x;
  xyzz29 p = xyzz29_identity();
  if (t <= bits) {
    p = xyzz29_load(terms + (size_t)set * (bits + 1) + t);
    if (t < bits)
      for (uint32_t i = 0; i < t; i++) p = xyzz29_double(p);   // term t < bits has weight 2^t; term `bits` (the total) 1
  }
  xyzz29_store(&lds[t], p);
  __syncthreads();
  tree_sum<1>(lds, 32, t, 0, true);
  if (t == 0) xyzz29_store(out + set, xyzz29_load(&lds[0]));
}
// canonical words of `count` XYZZ points for the host tail (32 words each)
// (`out` is page-locked host memory mapped into the device: the words land where the host tail reads them)
__global__ void msm_export_points(const xyzz29_mem* __restrict__ in, uint32_t count, uint32_t* __restrict__ out) {
  side_kernel_prio();
  uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= count) return;
  uint32_t w[32];
  xyzz29_to_words(xyzz29_load(in + q), w);
  uint4* o = reinterpret_cast<uint4*>(out + 32 * q);
  for (int i = 0; i < 8; i++) o[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
  __threadfence_system();
}

// per-window (A, S, T) -> canonical 8 x u32 Montgomery-2^256 words (X, Y, ZZ, ZZZ each) for the
// host tail; out[(3*j + which)*32 ..]
__global__ void msm_export_windows(ReduceOut in, uint32_t W, uint32_t has_t, uint32_t* __restrict__ out) {
  side_kernel_prio();
  uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= 3 * W) return;
  uint32_t j = q / 3, which = q - 3 * j;
  uint32_t w[32];
  if (which == 2 && !has_t) {
    for (int i = 0; i < 32; i++) w[i] = 0;
  } else {
    xyzz29_to_words(xyzz29_load((which == 0 ? in.a : which == 1 ? in.s : in.r) + j), w);
  }
  uint4* o = reinterpret_cast<uint4*>(out + 32 * q);
  for (int i = 0; i < 8; i++) o[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
  __threadfence_system();
}

}  // namespace sg
