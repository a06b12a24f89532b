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

// A prefetched point out of its buffer, in limbs -- and pinned there, so that the loads that refill the buffer, issued
// behind this, land in the buffer's own registers instead of a second buffer that is copied back at the end of the trip
// (2 x 8 v_mov_b64 per addition).  A point at infinity raises `redo`.
__device__ __forceinline__ affine29 affine29_take(const g1_affine_mem& raw, bool& redo) {
  affine29 p = affine29_load(&raw);
  uint32_t inf = p.inf;
#pragma unroll
  for (int i = 0; i < 9; i++) asm volatile("" : "+v"(p.x.l[i]), "+v"(p.y.l[i]));
  asm volatile("" : "+v"(inf) : : "memory");
  redo |= inf != 0;
  return p;
}

// Persistent: the grid is a fixed number of waves per SIMD (MsmConfig::acc_waves; three fit the register file at 138
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
      // Task head: the first point alone, or the sum of the first two by the affine + affine addition, without the products
      // that an accumulator of ZZ = ZZZ = 1 does not need.  Whatever is not the ordinary case of an addition -- a point at
      // infinity, P = +-Q, an empty task -- only raises `redo`: the lane goes on with a meaningless accumulator, and the
      // task is added again below by the additions that decide every case.  Reads past the end of the task fetch its last
      // entry again and are not used.
      const uint32_t last = max(end, start + 1) - 1;
      uint32_t e = sorted[start], e1 = sorted[min(start + 1, last)];
      g1_affine_mem raw = bases[e & 0x7fffffffu], raw1 = bases[e1 & 0x7fffffffu];
      bool redo = end <= start;
      affine29 p0 = affine29_take(raw, redo);
      if (e >> 31) affine29_negate(p0);
      xyzz29 acc;
      uint32_t k = start + 2;
      if (end - start == 1) {
        acc = xyzz29_from_affine(p0);
      } else {
        affine29 p1 = affine29_take(raw1, redo);
        if (e1 >> 31) affine29_negate(p1);
        e = sorted[min(k, last)];
        raw = bases[e & 0x7fffffffu];
        redo |= xyzz29_mmadd_ordinary(acc, p0, p1) != 0;
      }
      // Steady state: the ordinary addition, in place, is the only definition of the accumulator that the loop carries, and
      // the prefetch buffer is refilled where it stands as soon as its point is in limbs (affine29_take)
      for (; k < end; k++) {
        const affine29 p = affine29_take(raw, redo);
        const bool neg = e >> 31;
        e = sorted[min(k + 1, last)];
        raw = bases[e & 0x7fffffffu];
        redo |= xyzz29_madd_ordinary(acc, p, neg) != 0;
      }
      if (redo) {  // cold: the whole task by the additions that decide every case
        acc = xyzz29_identity();
        for (uint32_t i = start; i < end; i++) {
          const uint32_t ei = sorted[i];
          const g1_affine_mem q = bases[ei & 0x7fffffffu];
          xyzz29_madd(acc, affine29_load(&q), ei >> 31);
        }
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
