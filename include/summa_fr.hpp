// The two BN254 prime fields on the host, 4 x 64-bit Montgomery words: Fr (the scalars of the proof: transcript, challenges,
// the multi-open's arithmetic) and Fq (only ever converted: a commitment's coordinates, as the C ABI returns them, into the
// bytes the proof and the transcripts hold).  One body for both, templated on the modulus constants.
// Plain C++17, no GPU runtime: tests/cpp/proof_host_check.cpp builds it with a host compiler alone.
#pragma once
#include <array>
#include <cstdint>
#include <cstring>

namespace summa {
namespace prover {

// M: P[4] (the modulus), INV (-p^-1 mod 2^64), R1[4] (2^256 mod p: Montgomery one), R2[4] (2^512 mod p)
template <class M>
struct Mont {
  uint64_t l[4];
  static constexpr const uint64_t* P = M::P;
  static constexpr uint64_t INV = M::INV;
  static constexpr const uint64_t* R1 = M::R1;
  static constexpr const uint64_t* R2 = M::R2;
  static Mont zero() { return Mont{{0, 0, 0, 0}}; }
  static Mont one() { return Mont{{R1[0], R1[1], R1[2], R1[3]}}; }
  static bool geq_p(const uint64_t a[4]) {
    for (int i = 3; i >= 0; i--) {
      if (a[i] != P[i]) return a[i] > P[i];
    }
    return true;
  }
  static void sub_p(uint64_t a[4]) {
    unsigned __int128 borrow = 0;
    for (int i = 0; i < 4; i++) {
      unsigned __int128 t = (unsigned __int128)a[i] - P[i] - (uint64_t)borrow;
      a[i] = (uint64_t)t;
      borrow = (t >> 64) & 1;
    }
  }
  Mont operator+(const Mont& o) const {
    Mont r;
    unsigned __int128 c = 0;
    for (int i = 0; i < 4; i++) {
      c += (unsigned __int128)l[i] + o.l[i];
      r.l[i] = (uint64_t)c;
      c >>= 64;
    }
    if (c || geq_p(r.l)) sub_p(r.l);
    return r;
  }
  Mont operator-(const Mont& o) const {
    Mont r;
    unsigned __int128 borrow = 0;
    for (int i = 0; i < 4; i++) {
      unsigned __int128 t = (unsigned __int128)l[i] - o.l[i] - (uint64_t)borrow;
      r.l[i] = (uint64_t)t;
      borrow = (t >> 64) & 1;
    }
    if (borrow) {
      unsigned __int128 c = 0;
      for (int i = 0; i < 4; i++) {
        c += (unsigned __int128)r.l[i] + P[i];
        r.l[i] = (uint64_t)c;
        c >>= 64;
      }
    }
    return r;
  }
  Mont operator-() const { return zero() - *this; }
  Mont operator*(const Mont& o) const {  // CIOS Montgomery product
    uint64_t t[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
      unsigned __int128 c = 0;
      for (int j = 0; j < 4; j++) {
        c += (unsigned __int128)l[j] * o.l[i] + t[j];
        t[j] = (uint64_t)c;
        c >>= 64;
      }
      c += t[4];
      t[4] = (uint64_t)c;
      t[5] = (uint64_t)(c >> 64);
      const uint64_t m = t[0] * INV;
      c = (unsigned __int128)m * P[0] + t[0];
      c >>= 64;
      for (int j = 1; j < 4; j++) {
        c += (unsigned __int128)m * P[j] + t[j];
        t[j - 1] = (uint64_t)c;
        c >>= 64;
      }
      c += t[4];
      t[3] = (uint64_t)c;
      t[4] = t[5] + (uint64_t)(c >> 64);
    }
    Mont r{{t[0], t[1], t[2], t[3]}};
    if (t[4] || geq_p(r.l)) sub_p(r.l);
    return r;
  }
  bool operator==(const Mont& o) const { return !std::memcmp(l, o.l, 32); }
  bool operator!=(const Mont& o) const { return !(*this == o); }
  bool is_zero() const { return !(l[0] | l[1] | l[2] | l[3]); }
  Mont pow(const uint64_t e[4]) const {
    int top = 255;   // square-and-multiply from the highest set bit (most exponents here are rotations and small powers)
    while (top >= 0 && !((e[top / 64] >> (top % 64)) & 1)) top--;
    Mont r = one();
    for (int i = top; i >= 0; i--) {
      r = r * r;
      if ((e[i / 64] >> (i % 64)) & 1) r = r * *this;
    }
    return r;
  }
  Mont pow(uint64_t e) const {
    const uint64_t ee[4] = {e, 0, 0, 0};
    return pow(ee);
  }
  Mont inv() const {
    const uint64_t e[4] = {P[0] - 2, P[1], P[2], P[3]};
    return pow(e);
  }
  static Mont from_u64(uint64_t v) { return from_canonical_limbs(std::array<uint64_t, 4>{v, 0, 0, 0}.data()); }
  static Mont from_canonical_limbs(const uint64_t c[4]) {  // c < p
    Mont a{{c[0], c[1], c[2], c[3]}}, r2{{R2[0], R2[1], R2[2], R2[3]}};
    return a * r2;
  }
  // any 256-bit big-endian integer, reduced mod p (challenges: keccak output)
  static Mont from_be_bytes_reduced(const uint8_t b[32]) {
    uint64_t c[4];
    for (int i = 0; i < 4; i++) {
      uint64_t w = 0;
      for (int j = 0; j < 8; j++) w = (w << 8) | b[8 * (3 - i) + j];
      c[i] = w;
    }
    while (geq_p(c)) sub_p(c);
    return from_canonical_limbs(c);
  }
  void to_canonical_limbs(uint64_t out[4]) const {
    Mont o{{1, 0, 0, 0}};
    Mont c = *this * o;
    std::memcpy(out, c.l, 32);
  }
  void to_be_bytes(uint8_t out[32]) const {
    uint64_t c[4];
    to_canonical_limbs(c);
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 8; j++) out[8 * (3 - i) + j] = (uint8_t)(c[i] >> (8 * (7 - j)));
  }
  const uint8_t* bytes() const { return reinterpret_cast<const uint8_t*>(l); }  // Montgomery, as the ABI takes it
};

struct FrModulus {
  static constexpr uint64_t P[4] = {0x43e1f593f0000001ULL, 0x2833e84879b97091ULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL};
  static constexpr uint64_t INV = 0xc2e1f593efffffffULL;
  static constexpr uint64_t R1[4] = {0xac96341c4ffffffbULL, 0x36fc76959f60cd29ULL, 0x666ea36f7879462eULL, 0x0e0a77c19a07df2fULL};
  static constexpr uint64_t R2[4] = {0x1bb8e645ae216da7ULL, 0x53fe3ab1e35c59e3ULL, 0x8c49833d53bb8085ULL, 0x0216d0b17f4e44a5ULL};
};
struct FqModulus {
  static constexpr uint64_t P[4] = {0x3c208c16d87cfd47ULL, 0x97816a916871ca8dULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL};
  static constexpr uint64_t INV = 0x87d20782e4866389ULL;
  static constexpr uint64_t R1[4] = {0xd35d438dc58f0d9dULL, 0x0a78eb28f5c70b3dULL, 0x666ea36f7879462cULL, 0x0e0a77c19a07df2fULL};
  static constexpr uint64_t R2[4] = {0xf32cfc5b538afa89ULL, 0xb5e71911d44501fbULL, 0x47ab1eff0a417ff6ULL, 0x06d89f71cab8351fULL};
};
using Fr = Mont<FrModulus>;   // BN254 Fr on the host (Montgomery, 4 x 64)

// Fq only appears as bytes to convert: Montgomery little-endian (ABI) -> canonical big-endian (proof / transcript)
inline void fq_mont_to_be(const uint8_t in[32], uint8_t out[32]) {
  Mont<FqModulus> a;
  std::memcpy(a.l, in, 32);
  a.to_be_bytes(out);
}

}  // namespace prover
}  // namespace summa
