#include "msm.h"
#include "side_prio.cuh"

#include "msm_tiny.cuh"

namespace sg {
SG_DEFINE_SIDE_PRIO_SETTER(msm_many_set_side_prio)

// ------------------------------------------------------------------ many handfuls of points: ONE launch, results kept on the device
// The batch verifier folds N proofs into one pairing check (csrc/verifier_abi.hip: sv_verify_batch): 2 N MSMs of at most
// MSM_TINY_MAX points each, of which only sums over ranges of jobs are ever wanted.  msm_tiny_kernel is shaped for the latency of one
// job -- one wave per window with 8 lanes adding, one host tail per job.  Here the shape is throughput: a workgroup (one wave) takes
// eight consecutive windows of one job, lane (j, b) = (t >> 3, t & 7) gathers bucket b + 1 of window 8 g + j, so all 64 lanes add;
// the weighted sum sum_b (b + 1) B_b is the tiny kernel's suffix scan and tree sum inside each group of eight lanes.  Same window plan
// and digit rule (c = 4: 64 windows of 8 buckets, signed digits, unsigned top window), same output format: lane (j, 0) stores the
// window's sum as 32 canonical words into S[job][window], in device memory.  A job's points are [first[job], first[job + 1]).
__global__ void __launch_bounds__(64) msm_many_kernel(const fp_words* __restrict__ scalars, const g1_affine_mem* __restrict__ bases,
                                                      const uint32_t* __restrict__ first, WindowPlan wp, uint32_t* __restrict__ S) {
  side_kernel_prio();
  __shared__ int s_dig[8][MSM_TINY_MAX];
  __shared__ uint32_t s_pt[MSM_TINY_MAX][16];
  __shared__ xyzz29_mem s_x[64];
  const uint32_t job = blockIdx.y, t = threadIdx.x, w0 = 8 * blockIdx.x;
  const uint32_t lo = first[job], n = first[job + 1] - lo;   // n <= MSM_TINY_MAX (checked by the caller)
  if (t < n) {
    const words8 s = msm_tiny_scalar(scalars + lo + t, wp);
    uint32_t off = 0;
    for (uint32_t j = 0; j < w0; j++) off += wp.width[j];
    for (uint32_t j = 0; j < 8; j++) {
      s_dig[j][t] = msm_tiny_digit(s, w0 + j, off, wp);
      off += wp.width[w0 + j];
    }
    msm_tiny_point_to_lds(bases + lo + t, s_pt[t]);
  }
  __syncthreads();
  const uint32_t j = t >> 3, b = t & 7;
  xyzz29 acc = xyzz29_identity();
  for (uint32_t i = 0; i < n; i++) {
    const int d = s_dig[j][i];
    if ((d < 0 ? -d : d) != (int)b + 1) continue;
    affine29 p = affine29_from_words(s_pt[i]);
    if (d < 0) affine29_negate(p);
    xyzz29_madd(acc, p);
  }
  // per group of eight lanes: R_b = sum_{b' >= b} B_b' (three steps), then sum_b R_b = sum_b (b + 1) B_b (three steps)
  for (uint32_t step = 1; step < 8; step <<= 1) {
    xyzz29_store(s_x + t, acc);
    __syncthreads();
    if (b + step < 8) xyzz29_add(acc, xyzz29_load(s_x + t + step));
    __syncthreads();
  }
  for (uint32_t step = 4; step >= 1; step >>= 1) {
    xyzz29_store(s_x + t, acc);
    __syncthreads();
    if (b < step) xyzz29_add(acc, xyzz29_load(s_x + t + step));
    __syncthreads();
  }
  if (b == 0) {
    uint32_t wd[32];
    xyzz29_to_words(acc, wd);
    uint4* dst = reinterpret_cast<uint4*>(S + ((size_t)job * 64 + w0 + j) * 32);
#pragma unroll
    for (int i = 0; i < 8; i++) dst[i] = make_uint4(wd[4 * i], wd[4 * i + 1], wd[4 * i + 2], wd[4 * i + 3]);
  }
}

// a window sum as the kernel above stored it -> registers (coordinates below 2p; an identity stays one: ZZ = 0)
static __device__ __forceinline__ xyzz29 xyzz29_from_canonical_words(const uint32_t* src) {
  uint32_t w[32];
  const uint4* q = reinterpret_cast<const uint4*>(src);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint4 v = q[i];
    w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
  }
  xyzz29 r;
  r.x = f29_reduce_small<Fq29>(f29_from_words<5>(w));          // 32 -> < 2
  r.y = f29_reduce_small<Fq29>(f29_from_words<5>(w + 8));
  r.zz = f29_reduce_small<Fq29>(f29_from_words<5>(w + 16));
  r.zzz = f29_reduce_small<Fq29>(f29_from_words<5>(w + 24));
  return r;
}

// Sums over ranges of jobs, window by window: workgroup (w, r) adds S[a_r .. b_r)[w] -- thread t takes jobs a + t, a + t + 256, ..,
// then a tree sum over the 256 partial sums through LDS -- and thread 0 writes the window's sum (same format) into mapped host
// memory at out[r][w].  An identity among the operands is ordinary data (xyzz29_add decides every case); an empty range gives 64
// identities.  The host then runs the tail once per range (msm_window_sums_to_affine).
__global__ void __launch_bounds__(256) msm_many_sum_kernel(const uint32_t* __restrict__ S, ManyRanges ranges, uint32_t* __restrict__ out) {
  side_kernel_prio();
  __shared__ xyzz29_mem s_x[128];
  const uint32_t w = blockIdx.x, r = blockIdx.y, t = threadIdx.x;
  const uint32_t a = ranges.v[2 * r], b = ranges.v[2 * r + 1];
  xyzz29 acc = xyzz29_identity();
  for (uint32_t i = a + t; i < b; i += 256) xyzz29_add(acc, xyzz29_from_canonical_words(S + ((size_t)i * 64 + w) * 32));
  for (uint32_t step = 128; step >= 1; step >>= 1) {
    if (t >= step && t < 2 * step) xyzz29_store(s_x + (t - step), acc);
    __syncthreads();
    if (t < step) xyzz29_add(acc, xyzz29_load(s_x + t));
    __syncthreads();
  }
  if (t == 0) {
    uint32_t wd[32];
    xyzz29_to_words(acc, wd);
#pragma unroll
    for (int i = 0; i < 32; i++) out[((size_t)r * 64 + w) * 32 + i] = wd[i];
  }
}

hipError_t msm_many_launch(const fp_words* d_scalars, const g1_affine_mem* d_bases, const uint32_t* d_first, uint32_t jobs,
                           uint32_t* d_S, hipStream_t stream) {
  if (jobs == 0) return hipSuccess;
  if (jobs > MSM_MANY_MAX_JOBS) return hipErrorInvalidValue;
  const WindowPlan wp = make_window_plan(4);
  if (wp.W != MSM_MANY_WINDOWS) return hipErrorInvalidValue;   // S's layout: 64 windows per job, eight groups of eight
  msm_many_kernel<<<dim3(MSM_MANY_WINDOWS / 8, jobs), 64, 0, stream>>>(d_scalars, d_bases, d_first, wp, d_S);
  return hipGetLastError();
}

hipError_t msm_many_sum_launch(const uint32_t* d_S, const ManyRanges& ranges, uint32_t count, uint32_t* d_out, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  if (count > MSM_MANY_MAX_RANGES) return hipErrorInvalidValue;
  msm_many_sum_kernel<<<dim3(MSM_MANY_WINDOWS, count), 256, 0, stream>>>(d_S, ranges, d_out);
  return hipGetLastError();
}

}  // namespace sg
