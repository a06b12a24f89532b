// `Entry::new` for a whole snapshot (zk_prover/src/merkle_sum_tree/entry.rs:15-27): a username's field element is
// keccak256(username) read as a big-endian integer mod r (utils/operation_helpers.rs:5-8), a balance's is its decimal string
// folded digit by digit in the field (`Fp::from_str_vartime` behind big_uint_to_fp, :10-12).  The arithmetic below is plain
// C++ over bn254_f29.cuh and keccak_f1600.h, so it compiles without HIP (tests/cpp/mst_entries_check.cpp); the kernels that
// call it, one thread per name and one per balance, are in mst_entries.hip, and so is the launcher declared at the end.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "bn254_f29.cuh"
#include "keccak_f1600.h"

namespace sg {

// a Keccak-256 digest (four little-endian lanes, keccak256_lanes) as a big-endian integer mod r -> Montgomery words, the
// memory form of halo2curves.  The integer is below 2^256 < 6 r: one product with 2^517 (2^256 * 2^261) reduces and converts.
SG_HD void mst_username_words(const uint64_t digest[4], uint32_t out[8]) {
  uint32_t w[8];
#pragma unroll
  for (int m = 0; m < 4; m++) {
    // the least significant 8 bytes of the integer are the digest's last lane, byte-reversed
    const uint64_t v = digest[3 - m];
    const uint64_t s = ((v & 0x00000000000000ffULL) << 56) | ((v & 0x000000000000ff00ULL) << 40) | ((v & 0x0000000000ff0000ULL) << 24) |
                       ((v & 0x00000000ff000000ULL) << 8) | ((v & 0x000000ff00000000ULL) >> 8) | ((v & 0x0000ff0000000000ULL) >> 24) |
                       ((v & 0x00ff000000000000ULL) >> 40) | ((v & 0xff00000000000000ULL) >> 56);
    w[2 * m] = (uint32_t)s;
    w[2 * m + 1] = (uint32_t)(s >> 32);
  }
  f29_to_words(f29_reduce_with<Fr29>(f29_from_words<0>(w), Fr29::r517), out);
}

// ASCII decimal digits p[0 .. len) -> the number mod r as Montgomery words.  The accumulator holds the plain residue (below
// 2 r): a step is acc * (10 * 2^261) * 2^-261 + digit -- the digit joins the product's high columns (f29_mul_add), and with
// bounds 2 and 10 the result is below (20 / 170 + 1) r + 9 < 2 r again.  Any length; leading zeros change nothing.
SG_HD void mst_decimal_words(const uint8_t* p, size_t len, uint32_t out[8]) {
  const f29 one = f29_one<Fr29>();
  const f29 two = f29_dbl(one), eight = f29_dbl(f29_dbl(two));
  const f29 ten = f29_add(eight, two);                       // 10 * 2^261, lazily: below 10 r
  f29 acc = f29_zero(), digit = f29_zero();
  for (size_t i = 0; i < len; i++) {
    digit.l[0] = (uint32_t)(p[i] - (uint8_t)'0');
    acc = f29_mul_add<Fr29>(acc, ten, digit);
  }
  f29_to_words(f29_reduce_with<Fr29>(acc, Fr29::r517), out);
}

// "" if digit_bytes / digit_off describe `fields` decimal balance fields, else what is wrong with them (the lowest offending
// field by its index).  On its own for sg_mst_update_dev, which takes balances without names (mst_update_plan.h).
inline std::string mst_digit_fields_problem(const uint8_t* digit_bytes, const uint64_t* digit_off, size_t fields) {
  if (digit_off[0] != 0) return "digit_off[0] is not 0";
  for (size_t j = 0; j < fields; j++) {
    if (digit_off[j + 1] < digit_off[j]) return "digit_off decreases at field " + std::to_string(j);
  }
  for (size_t j = 0; j < fields; j++) {
    if (digit_off[j + 1] == digit_off[j]) return "balance field " + std::to_string(j) + " is empty";
    for (uint64_t t = digit_off[j]; t < digit_off[j + 1]; t++) {
      if (digit_bytes[t] < '0' || digit_bytes[t] > '9') return "balance field " + std::to_string(j) + " is not a decimal number";
    }
  }
  return "";
}
// What sg_mst_entries_dev refuses before it touches the device: "" if the four host buffers describe n names and n * nc
// balance fields, else what is wrong with them.
inline std::string mst_entries_problem(const uint64_t* name_off, const uint8_t* digit_bytes, const uint64_t* digit_off, size_t n,
                                       uint32_t nc) {
  if (name_off[0] != 0) return "name_off[0] is not 0";
  for (size_t i = 0; i < n; i++) {
    if (name_off[i + 1] < name_off[i]) return "name_off decreases at entry " + std::to_string(i);
  }
  return mst_digit_fields_problem(digit_bytes, digit_off, n * (size_t)nc);
}

#if defined(__HIPCC__)
// d_users[i] = Entry::new's username of name i, d_balances[i * nc + c] its balances, i < n; rows n .. rows of both are the
// zero entry (username 0, balances 0: entry.rs:30-38).  All six pointers are device memory; offsets as in sg_mst_entries_dev.
hipError_t mst_entries_launch(const uint8_t* d_name_bytes, const uint64_t* d_name_off, const uint8_t* d_digit_bytes,
                              const uint64_t* d_digit_off, size_t n, size_t rows, uint32_t nc, void* d_users, void* d_balances,
                              hipStream_t stream);
// the balances alone, no padding rows: d_balances[j] = field j, j < fields (sg_mst_update_dev's new balances)
hipError_t mst_balances_launch(const uint8_t* d_digit_bytes, const uint64_t* d_digit_off, size_t fields, void* d_balances,
                               hipStream_t stream);
#endif

}  // namespace sg
