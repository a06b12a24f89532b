// Keccak-f[1600] and Ethereum's Keccak-256 (rate 136, padding 0x01 .. 0x80) of a byte string that starts at any address.
// No HIP, no library: the same text is the device code of mst_usernames_kernel (mst_entries.hip) and a host function
// (tests/cpp/mst_entries_check.cpp runs it against known digests).
//
// The 25 lanes are 25 named-by-constant array elements: every loop below has a compile-time trip count and is unrolled,
// rho / pi is written out lane by lane, so no index depends on run-time data and the state stays in registers (50 VGPRs) --
// a state indexed at run time would live in scratch memory.  Message bytes are read one by one: a name starts wherever the
// one before it ended, and a 64-bit load from such an address is undefined on the host and slow or trapping on a device.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KECCAK_HD __host__ __device__ __forceinline__
#else
#define KECCAK_HD inline
#endif

namespace sg {

static constexpr size_t KECCAK256_RATE = 136;   // bytes per block: lanes 0..16

KECCAK_HD uint64_t keccak_rotl(uint64_t v, int r) { return (v << r) | (v >> (64 - r)); }

// one round with round constant rc; lanes indexed x + 5 y
KECCAK_HD void keccak_round(uint64_t (&a)[25], uint64_t rc) {
  uint64_t c[5], d[5], b[25];
#pragma unroll
  for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
  for (int x = 0; x < 5; x++) d[x] = c[(x + 4) % 5] ^ keccak_rotl(c[(x + 1) % 5], 1);
#pragma unroll
  for (int i = 0; i < 25; i++) a[i] ^= d[i % 5];
  // rho and pi: b[y + 5 ((2 x + 3 y) % 5)] = rotl(a[x + 5 y], offset[x + 5 y])
  b[0] = a[0];
  b[10] = keccak_rotl(a[1], 1);
  b[20] = keccak_rotl(a[2], 62);
  b[5] = keccak_rotl(a[3], 28);
  b[15] = keccak_rotl(a[4], 27);
  b[16] = keccak_rotl(a[5], 36);
  b[1] = keccak_rotl(a[6], 44);
  b[11] = keccak_rotl(a[7], 6);
  b[21] = keccak_rotl(a[8], 55);
  b[6] = keccak_rotl(a[9], 20);
  b[7] = keccak_rotl(a[10], 3);
  b[17] = keccak_rotl(a[11], 10);
  b[2] = keccak_rotl(a[12], 43);
  b[12] = keccak_rotl(a[13], 25);
  b[22] = keccak_rotl(a[14], 39);
  b[23] = keccak_rotl(a[15], 41);
  b[8] = keccak_rotl(a[16], 45);
  b[18] = keccak_rotl(a[17], 15);
  b[3] = keccak_rotl(a[18], 21);
  b[13] = keccak_rotl(a[19], 8);
  b[14] = keccak_rotl(a[20], 18);
  b[24] = keccak_rotl(a[21], 2);
  b[9] = keccak_rotl(a[22], 61);
  b[19] = keccak_rotl(a[23], 56);
  b[4] = keccak_rotl(a[24], 14);
#pragma unroll
  for (int y = 0; y < 25; y += 5) {
#pragma unroll
    for (int x = 0; x < 5; x++) a[y + x] = b[y + x] ^ (~b[y + (x + 1) % 5] & b[y + (x + 2) % 5]);
  }
  a[0] ^= rc;
}

KECCAK_HD void keccak_f1600(uint64_t (&a)[25]) {
  constexpr uint64_t RC[24] = {
      0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL, 0x000000000000808bULL,
      0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL, 0x000000000000008aULL, 0x0000000000000088ULL,
      0x0000000080008009ULL, 0x000000008000000aULL, 0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL,
      0x8000000000008003ULL, 0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800aULL, 0x800000008000000aULL,
      0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
#pragma unroll
  for (int r = 0; r < 24; r++) keccak_round(a, RC[r]);
}

// bytes p[0 .. 8) as a little-endian word
KECCAK_HD uint64_t keccak_load8(const uint8_t* p) {
  uint64_t w = 0;
#pragma unroll
  for (int b = 0; b < 8; b++) w |= (uint64_t)p[b] << (8 * b);
  return w;
}

// out[0 .. 4) = the digest's 32 bytes as four little-endian lanes (byte j of the digest = byte j % 8 of out[j / 8])
KECCAK_HD void keccak256_lanes(const uint8_t* p, size_t len, uint64_t out[4]) {
  uint64_t a[25];
#pragma unroll
  for (int i = 0; i < 25; i++) a[i] = 0;
  // One block per turn, the permutation in one place.  A block with 136 bytes left or more takes whole lanes only; the last
  // one has len < 136 message bytes, 0x01 behind them and 0x80 on byte 135 (the same byte when len = 135).
  for (;;) {
    const bool last = len < KECCAK256_RATE;
#pragma unroll
    for (int i = 0; i < 17; i++) {
      const size_t base = 8 * (size_t)i;
      uint64_t w = 0;
      if (base + 8 <= len) {
        w = keccak_load8(p + base);
      } else if (base <= len) {      // only in the last block: the lane the message ends in
#pragma unroll
        for (int b = 0; b < 8; b++) {
          if (base + b < len) w |= (uint64_t)p[base + b] << (8 * b);
        }
        w |= (uint64_t)0x01 << (8 * (len - base));
      }
      a[i] ^= w;
    }
    if (last) a[16] ^= 0x8000000000000000ULL;
    keccak_f1600(a);
    if (last) break;
    p += KECCAK256_RATE;
    len -= KECCAK256_RATE;
  }
#pragma unroll
  for (int i = 0; i < 4; i++) out[i] = a[i];
}

}  // namespace sg
