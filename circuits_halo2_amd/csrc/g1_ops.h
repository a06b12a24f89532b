// Set-up time operations on G1 points (g1_ops.hip): none of them is part of the MSM engine's hot path.
#pragma once
#include <hip/hip_runtime.h>

#include "bn254_curve29.cuh"
#include "msm_plan.h"

namespace sg {

#ifndef SG_WORDS8
#define SG_WORDS8
struct words8 {  // one field element as 8 LE u32 words (Montgomery-2^256), host side
  uint32_t l[8];
};
#endif

// Fixed-base mode (resident SRS): row w of `table` holds 2^(bit offset of window w) * P_i, so the W
// digits of a scalar are W independent (digit, point) pairs of ONE bucket set: W - 1 of the W
// bucket reductions disappear and the window can be as wide as the sort allows.
struct FixedTable {
  g1_affine_mem* table = nullptr;  // W x n affine points, row major
  size_t n = 0;
  uint32_t c = 0;
  WindowPlan wp{};
};
hipError_t build_window_table(const g1_affine_mem* d_bases, size_t n, uint32_t c, FixedTable* out, hipStream_t stream);

// FFT over G1 (N5): out = DFT_omega(in) [* scale], natural order; d_work: 2^log_n xyzz29_mem
hipError_t g1_fft(const g1_affine_mem* d_in, g1_affine_mem* d_out, uint32_t log_n, const words8& omega,
                  const words8* scale, xyzz29_mem* d_work, hipStream_t stream);
hipError_t fixed_base_mul(const fp_words* d_scalars, size_t n, g1_affine_mem* d_out, hipStream_t stream);
// out[i] = in[0] + ... + in[i], affine (the basis of difference-form commitments: sum_i s_i P_i = sum_i (s_i - s_{i+1}) Q_i with
// Q the inclusive prefix sums and s_n = 0 -- a column that is constant over long runs becomes a sparse MSM).  Set-up
// time only; allocates and frees its own work space.  d_out may not alias d_in.
hipError_t g1_prefix_sums(const g1_affine_mem* d_in, size_t n, g1_affine_mem* d_out, hipStream_t stream);
// *d_bad = number of points that are neither on y^2 = x^3 + 3 nor the identity
hipError_t g1_on_curve(const g1_affine_mem* d_points, size_t n, uint32_t* d_bad, hipStream_t stream);

}  // namespace sg
