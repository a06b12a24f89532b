// What the one-launch MSM kernels share (msm_tiny.hip: one job, workgroup = window; msm_many.hip: many jobs, workgroup = eight
// windows of one job): a thread's scalar with every window's digit made independent, one digit of it, a point into LDS.
#pragma once
#include "msm.h"

namespace sg {

// canonical scalar + K, K = sum_{j < W-1} 2^(o_j + w_j - 1): every window's digit becomes independent of its neighbours
__device__ __forceinline__ words8 msm_tiny_scalar(const fp_words* scalar, const WindowPlan& wp) {
  words8 s;
  {
    f29 k = f29_zero();   // canonical scalar = s~ * 2^5 * 2^-261 (msm_digits)
    k.l[0] = 32;
    f29_to_words(f29_cond_sub_p<Fr29>(f29_mul<Fr29>(f29_load_r256<Fr29>(scalar), k)), s.l);
  }
  uint32_t kk[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t o = 0;
  for (uint32_t j = 0; j + 1 < wp.W; j++) {
    const uint32_t bit = o + wp.width[j] - 1;
    const uint32_t m = 1u << (bit & 31), q = bit >> 5;
#pragma unroll
    for (int i = 0; i < 8; i++) kk[i] |= (q == (uint32_t)i) ? m : 0u;
    o += wp.width[j];
  }
  uint32_t carry = 0;
#pragma unroll
  for (int q = 0; q < 8; q++) {
    const uint64_t v = (uint64_t)s.l[q] + kk[q] + carry;
    s.l[q] = (uint32_t)v;
    carry = (uint32_t)(v >> 32);
  }
  return s;
}

// the digit of window w (at bit offset off) of s = msm_tiny_scalar(..): signed, the top window unsigned
__device__ __forceinline__ int msm_tiny_digit(const words8& s, uint32_t w, uint32_t off, const WindowPlan& wp) {
  const uint32_t width = wp.width[w], q = off >> 5, r = off & 31;
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    lo = (q == (uint32_t)i) ? s.l[i] : lo;
    hi = (q + 1 == (uint32_t)i) ? s.l[i] : hi;
  }
  const uint32_t v = (uint32_t)((((uint64_t)hi << 32) | lo) >> r) & ((1u << width) - 1);
  return (w + 1 < wp.W) ? (int)v - (int)(1u << (width - 1)) : (int)v;
}

__device__ __forceinline__ void msm_tiny_point_to_lds(const g1_affine_mem* base, uint32_t dst[16]) {
  const uint4* src = base->q;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint4 x = src[i];
    dst[4 * i] = x.x; dst[4 * i + 1] = x.y; dst[4 * i + 2] = x.z; dst[4 * i + 3] = x.w;
  }
}

}  // namespace sg
