// The leaves' inputs of a Merkle sum tree from what an exchange has -- usernames and decimal balances -- on the device: the
// GPU counterpart of `Entry::new` over a whole snapshot (mst_entries.h has the arithmetic and the references).  Both
// kernels trust their offsets: sg_mst_entries_dev (abi_mst.hip) validates them on the host before it launches.
#include "mst_entries.h"

#include "bn254_curve29.cuh"
#include "side_prio.cuh"

namespace sg {
SG_DEFINE_SIDE_PRIO_SETTER(mst_entries_set_side_prio)

static constexpr uint32_t MST_ENTRIES_BLOCK = 128;

__device__ __forceinline__ void store_zero(fp_words* p) {
  const uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  fp_words_store(p, z);
}

// one thread per row: rows below n hash their name, the others are the zero entry's username, the field element 0
__global__ void __launch_bounds__(MST_ENTRIES_BLOCK) mst_usernames_kernel(const uint8_t* __restrict__ bytes,
                                                                         const uint64_t* __restrict__ off, uint32_t n,
                                                                         uint32_t rows, fp_words* __restrict__ users) {
  side_kernel_prio();
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  if (i >= n) {
    store_zero(users + i);
    return;
  }
  const uint64_t lo = off[i], hi = off[i + 1];
  uint64_t digest[4];
  keccak256_lanes(bytes + lo, (size_t)(hi - lo), digest);
  uint32_t w[8];
  mst_username_words(digest, w);
  fp_words_store(users + i, w);
}

// one thread per balance field: fields below `fields` = n * nc fold their digits, the others are 0
__global__ void __launch_bounds__(MST_ENTRIES_BLOCK) mst_balances_kernel(const uint8_t* __restrict__ bytes,
                                                                        const uint64_t* __restrict__ off, uint64_t fields,
                                                                        uint64_t total, fp_words* __restrict__ balances) {
  side_kernel_prio();
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= total) return;
  if (j >= fields) {
    store_zero(balances + j);
    return;
  }
  const uint64_t lo = off[j], hi = off[j + 1];
  uint32_t w[8];
  mst_decimal_words(bytes + lo, (size_t)(hi - lo), w);
  fp_words_store(balances + j, w);
}

hipError_t mst_entries_launch(const uint8_t* d_name_bytes, const uint64_t* d_name_off, const uint8_t* d_digit_bytes,
                              const uint64_t* d_digit_off, size_t n, size_t rows, uint32_t nc, void* d_users, void* d_balances,
                              hipStream_t stream) {
  const uint64_t total = (uint64_t)rows * nc;                // rows < 2^32, nc <= 64: at most 2^31 blocks
  mst_usernames_kernel<<<(unsigned)((rows + MST_ENTRIES_BLOCK - 1) / MST_ENTRIES_BLOCK), MST_ENTRIES_BLOCK, 0, stream>>>(
      d_name_bytes, d_name_off, (uint32_t)n, (uint32_t)rows, static_cast<fp_words*>(d_users));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  mst_balances_kernel<<<(unsigned)((total + MST_ENTRIES_BLOCK - 1) / MST_ENTRIES_BLOCK), MST_ENTRIES_BLOCK, 0, stream>>>(
      d_digit_bytes, d_digit_off, (uint64_t)n * nc, total, static_cast<fp_words*>(d_balances));
  return hipGetLastError();
}
hipError_t mst_balances_launch(const uint8_t* d_digit_bytes, const uint64_t* d_digit_off, size_t fields, void* d_balances,
                               hipStream_t stream) {
  if (!fields) return hipSuccess;
  mst_balances_kernel<<<(unsigned)((fields + MST_ENTRIES_BLOCK - 1) / MST_ENTRIES_BLOCK), MST_ENTRIES_BLOCK, 0, stream>>>(
      d_digit_bytes, d_digit_off, (uint64_t)fields, (uint64_t)fields, static_cast<fp_words*>(d_balances));
  return hipGetLastError();
}

}  // namespace sg
