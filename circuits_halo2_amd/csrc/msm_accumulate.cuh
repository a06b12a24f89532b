// MSM engine, part 2 of 3 (included once by msm.hip): bucket accumulation and the merge rounds of heavy buckets.
#pragma once
#include "msm.h"
#include "side_prio.cuh"

namespace sg {

// ------------------------------------------------------------------ 4: accumulate / merge
__device__ __forceinline__ uint32_t find_owner(const uint32_t* __restrict__ toff, uint32_t NB, uint32_t t) {
  uint32_t lo = 0, hi = NB;  // invariant: toff[lo] <= t < toff[hi]
  while (hi - lo > 1) {
    uint32_t mid = (lo + hi) >> 1;
    if (toff[mid] <= t) lo = mid; else hi = mid;
  }
  return lo;
}

// Persistent: the grid is a fixed number of waves per SIMD (MsmConfig::acc_waves; three fill the register file at 161
// registers), and every wave takes tickets of 64 consecutive tasks from a counter until the task list (longest first, so
// the 64 lanes of a ticket have equal work) is used up: the end of the launch is balanced by construction instead of by
// the order in which the hardware happens to retire workgroups (2^20: 1.16 -> 1.12 ms; profiles/r03_sweeps/persistent_accumulate.txt).
// Sizing the launch to leave room for the kernels of other streams (two waves per SIMD) was measured too and does not pay:
// the kernels beside it still crawl (same file), and the accumulation alone loses 4 %.
__global__ void __launch_bounds__(256) msm_accumulate(const uint32_t* __restrict__ sorted, BatchPtrs bp,
                                                      uint32_t buckets_per_msm,
                                                      const uint32_t* __restrict__ off,
                                                      const uint32_t* __restrict__ cnt,
                                                      const uint32_t* __restrict__ toff,
                                                      const uint2* __restrict__ order, uint32_t log_L,
                                                      const uint32_t* __restrict__ meta, uint32_t* __restrict__ ticket,
                                                      xyzz29_mem* __restrict__ partial, uint64_t* __restrict__ trace) {
  // launched before the host has read the counters back (the read overlaps this kernel); the exact task count is meta[1]
  const uint32_t ntasks = meta[1], lane = threadIdx.x & 63u;
  // debug (msm.acc_trace): when every wave starts and leaves (wall_clock64 ticks)
  const uint32_t wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (trace && lane == 0) trace[2 * wave_id] = wall_clock64();
  for (;;) {
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(ticket, 64u);
    base = __builtin_amdgcn_readfirstlane(base);
    if (base >= ntasks) break;          // every wave gets here: the counter only grows
    const uint32_t t = base + lane;
    if (t < ntasks) {
      const uint2 o = order[t];
      const uint32_t b = o.x, seg = o.y;
      const g1_affine_mem* __restrict__ bases = bp.bases[b / buckets_per_msm];
      uint32_t start = off[b] + (seg << log_L);
      uint32_t end = min(off[b] + cnt[b], start + (1u << log_L));
      xyzz29 acc = xyzz29_identity();
      uint32_t e = sorted[start];
      g1_affine_mem raw = bases[e & 0x7fffffffu];
      for (uint32_t k = start; k < end; k++) {
        uint32_t e_next = 0;
        g1_affine_mem raw_next = raw;
        if (k + 1 < end) {  // prefetch the next point while this one is being added
          e_next = sorted[k + 1];
          raw_next = bases[e_next & 0x7fffffffu];
        }
        affine29 p = affine29_load(&raw);
        if (e >> 31) affine29_negate(p);
        xyzz29_madd(acc, p);
        e = e_next;
        raw = raw_next;
      }
      xyzz29_store(partial + toff[b] + seg, acc);
    }
  }
  if (trace && lane == 0) trace[2 * wave_id + 1] = wall_clock64();
}

// Every kernel below is written for LOGICAL threads of Q lanes: Q = 1 is one lane per point
// operation, Q = 4 the quad-cooperative addition (xyzz29_add_quad; all 4 lanes hold the same
// values).  lt = logical thread, role = lane within the quad.
template <int Q>
__device__ __forceinline__ void add_q(xyzz29& acc, const xyzz29& q, uint32_t role) {
  if (Q == 4) xyzz29_add_quad(acc, q, role);
  else xyzz29_add(acc, q);   // (inlined at every call site: one out-of-line copy per kernel was measured and is slower, docs/history.md section 4.11)
}
template <int Q>
__global__ void __launch_bounds__(256) msm_merge(const xyzz29_mem* __restrict__ in, const uint32_t* __restrict__ off,
                                                 const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ toff,
                                                 uint32_t NB, uint32_t log_L, const uint32_t* __restrict__ meta,
                                                 xyzz29_mem* __restrict__ out) {
  side_kernel_prio();
  // the grid covers a host-side upper bound; the exact task count of this level is meta[1]
  const uint32_t t = (blockIdx.x * blockDim.x + threadIdx.x) / Q, role = threadIdx.x % Q;
  if (t >= meta[1]) return;
  uint32_t b = find_owner(toff, NB, t);
  uint32_t seg = t - toff[b];
  uint32_t start = off[b] + (seg << log_L);
  uint32_t end = min(off[b] + cnt[b], start + (1u << log_L));
  xyzz29 acc = xyzz29_identity();
  for (uint32_t k = start; k < end; k++) add_q<Q>(acc, xyzz29_load(in + k), role);
  if (role == 0) xyzz29_store(out + t, acc);
}

}  // namespace sg
