// Keccak-256, Blake2b and the two transcripts of the reference's provers, over the host field of summa_fr.hpp.
// Plain C++17, no GPU runtime.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "summa_fr.hpp"

namespace summa {
namespace prover {

// ------------------------------------------------------------------ Keccak-256 (Ethereum's) and the EVM transcript
inline void keccak_f(uint64_t s[25]) {
  static constexpr uint64_t RC[24] = {
      0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL, 0x000000000000808bULL,
      0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL, 0x000000000000008aULL, 0x0000000000000088ULL,
      0x0000000080008009ULL, 0x000000008000000aULL, 0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL,
      0x8000000000008003ULL, 0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800aULL, 0x800000008000000aULL,
      0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
  static constexpr int ROT[24] = {1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 2, 14, 27, 41, 56, 8, 25, 43, 62, 18, 39, 61, 20, 44};
  static constexpr int PIL[24] = {10, 7, 11, 17, 18, 3, 5, 16, 8, 21, 24, 4, 15, 23, 19, 13, 12, 2, 20, 14, 22, 9, 6, 1};
  for (int round = 0; round < 24; round++) {
    uint64_t bc[5];
    for (int i = 0; i < 5; i++) bc[i] = s[i] ^ s[i + 5] ^ s[i + 10] ^ s[i + 15] ^ s[i + 20];
    for (int i = 0; i < 5; i++) {
      const uint64_t t = bc[(i + 4) % 5] ^ ((bc[(i + 1) % 5] << 1) | (bc[(i + 1) % 5] >> 63));
      for (int j = 0; j < 25; j += 5) s[j + i] ^= t;
    }
    uint64_t t = s[1];
    for (int i = 0; i < 24; i++) {
      const int j = PIL[i];
      const uint64_t b = s[j];
      s[j] = (t << ROT[i]) | (t >> (64 - ROT[i]));
      t = b;
    }
    for (int j = 0; j < 25; j += 5) {
      for (int i = 0; i < 5; i++) bc[i] = s[j + i];
      for (int i = 0; i < 5; i++) s[j + i] ^= (~bc[(i + 1) % 5]) & bc[(i + 2) % 5];
    }
    s[0] ^= RC[round];
  }
}
inline std::array<uint8_t, 32> keccak256(const uint8_t* data, size_t len) {
  uint64_t s[25] = {0};
  constexpr size_t rate = 136;
  std::vector<uint8_t> buf(data, data + len);
  buf.push_back(0x01);
  while (buf.size() % rate) buf.push_back(0);
  buf.back() |= 0x80;
  for (size_t off = 0; off < buf.size(); off += rate) {
    for (size_t i = 0; i < rate / 8; i++) {
      uint64_t w;
      std::memcpy(&w, buf.data() + off + 8 * i, 8);
      s[i] ^= w;
    }
    keccak_f(s);
  }
  std::array<uint8_t, 32> out;
  std::memcpy(out.data(), s, 32);
  return out;
}

// Both transcripts of the reference [REF zk_prover/src/circuits/utils.rs:93 (Blake2bWrite / Challenge255, `full_prover`),
// :170 (Keccak256Transcript, `gen_proof_solidity_calldata`)]: absorb the verifying key's digest first (`vk.hash_into`),
// then the instances, commitments and evaluations as create_proof produces them.
struct EvmTranscript {
  std::vector<uint8_t> buf, proof;
  bool squeezed = false;
  void common_scalar(const Fr& v) {
    uint8_t b[32];
    v.to_be_bytes(b);
    buf.insert(buf.end(), b, b + 32);
    squeezed = false;
  }
  void write_scalar(const Fr& v) {
    common_scalar(v);
    proof.insert(proof.end(), buf.end() - 32, buf.end());
  }
  void write_point(const uint8_t affine_mont[64]) {  // as the ABI returns commitments
    uint8_t b[64];
    fq_mont_to_be(affine_mont, b);
    fq_mont_to_be(affine_mont + 32, b + 32);
    buf.insert(buf.end(), b, b + 64);
    proof.insert(proof.end(), b, b + 64);
    squeezed = false;
  }
  Fr squeeze() {   // keccak(buffer) mod r, the hash becomes the buffer; right after a squeeze: keccak(hash || 0x01)
    if (squeezed) {
      buf.resize(32);
      buf.push_back(0x01);
    }
    auto h = keccak256(buf.data(), buf.size());
    buf.assign(h.begin(), h.end());
    squeezed = true;
    return Fr::from_be_bytes_reduced(h.data());
  }
  Fr squeeze_again() { return squeeze(); }
};

// Blake2b (RFC 7693), unkeyed, with personalisation; `finalize` works on a copy, as the transcript needs it
struct Blake2b {
  uint64_t h[8];
  uint8_t buf[128];
  size_t buflen = 0;
  uint64_t t0 = 0, t1 = 0;
  static constexpr uint64_t IV[8] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
                                     0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL, 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
  Blake2b(size_t outlen, const char* personal16) {
    uint8_t param[64] = {0};
    param[0] = (uint8_t)outlen;
    param[2] = 1;
    param[3] = 1;
    if (personal16) std::memcpy(param + 48, personal16, std::min<size_t>(16, std::strlen(personal16)));
    for (int i = 0; i < 8; i++) {
      uint64_t w;
      std::memcpy(&w, param + 8 * i, 8);
      h[i] = IV[i] ^ w;
    }
  }
  static uint64_t rotr(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }
  void compress(const uint8_t block[128], bool last) {
    static constexpr uint8_t SIGMA[12][16] = {
        {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
        {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
        {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
        {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
        {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0},
        {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}};
    uint64_t m[16], v[16];
    std::memcpy(m, block, 128);
    for (int i = 0; i < 8; i++) {
      v[i] = h[i];
      v[i + 8] = IV[i];
    }
    v[12] ^= t0;
    v[13] ^= t1;
    if (last) v[14] = ~v[14];
    auto g = [&](int a, int b, int c, int d, uint64_t x, uint64_t y) {
      v[a] = v[a] + v[b] + x; v[d] = rotr(v[d] ^ v[a], 32);
      v[c] = v[c] + v[d]; v[b] = rotr(v[b] ^ v[c], 24);
      v[a] = v[a] + v[b] + y; v[d] = rotr(v[d] ^ v[a], 16);
      v[c] = v[c] + v[d]; v[b] = rotr(v[b] ^ v[c], 63);
    };
    for (int r = 0; r < 12; r++) {
      const uint8_t* sg = SIGMA[r];
      g(0, 4, 8, 12, m[sg[0]], m[sg[1]]); g(1, 5, 9, 13, m[sg[2]], m[sg[3]]);
      g(2, 6, 10, 14, m[sg[4]], m[sg[5]]); g(3, 7, 11, 15, m[sg[6]], m[sg[7]]);
      g(0, 5, 10, 15, m[sg[8]], m[sg[9]]); g(1, 6, 11, 12, m[sg[10]], m[sg[11]]);
      g(2, 7, 8, 13, m[sg[12]], m[sg[13]]); g(3, 4, 9, 14, m[sg[14]], m[sg[15]]);
    }
    for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[i + 8];
  }
  void update(const uint8_t* data, size_t len) {
    while (len) {
      if (buflen == 128) {   // a full buffer is only compressed once more input follows (the last block is special)
        t0 += 128;
        if (t0 < 128) t1++;
        compress(buf, false);
        buflen = 0;
      }
      const size_t take = std::min(len, 128 - buflen);
      std::memcpy(buf + buflen, data, take);
      buflen += take;
      data += take;
      len -= take;
    }
  }
  void finalize(uint8_t* out, size_t outlen) const {   // on a copy: the state keeps absorbing afterwards
    Blake2b c = *this;
    c.t0 += c.buflen;
    if (c.t0 < c.buflen) c.t1++;
    std::memset(c.buf + c.buflen, 0, 128 - c.buflen);
    c.compress(c.buf, true);
    std::memcpy(out, c.h, outlen);
  }
};
struct Blake2bTranscript {   // Blake2bWrite<_, G1Affine, Challenge255<_>> (halo2_proofs transcript.rs)
  Blake2b state{64, "Halo2-Transcript"};
  std::vector<uint8_t> proof;
  static void reverse32(uint8_t b[32]) { std::reverse(b, b + 32); }
  std::array<uint8_t, 32> common_scalar(const Fr& v) {   // returns the canonical little-endian bytes it absorbed
    uint8_t b[33];
    b[0] = 2;
    v.to_be_bytes(b + 1);
    reverse32(b + 1);
    state.update(b, 33);
    std::array<uint8_t, 32> le;
    std::memcpy(le.data(), b + 1, 32);
    return le;
  }
  void write_scalar(const Fr& v) {
    const auto le = common_scalar(v);
    proof.insert(proof.end(), le.begin(), le.end());
  }
  void write_point(const uint8_t affine_mont[64]) {
    uint8_t b[65];
    b[0] = 1;
    fq_mont_to_be(affine_mont, b + 1);
    fq_mont_to_be(affine_mont + 32, b + 33);
    reverse32(b + 1);
    reverse32(b + 33);
    bool inf = true;
    for (int i = 0; i < 64; i++) inf = inf && !affine_mont[i];
    if (inf) throw std::runtime_error("cannot write points at infinity to the transcript");
    state.update(b, 65);
    uint8_t c[32];
    std::memcpy(c, b + 1, 32);                    // x little-endian, bit 6 of the last byte = parity of y
    c[31] |= (uint8_t)((b[33] & 1) << 6);
    proof.insert(proof.end(), c, c + 32);
  }
  Fr squeeze() {   // prefix 0, digest of a clone, 64 bytes as a little-endian integer mod r (from_uniform_bytes)
    const uint8_t zero = 0;
    state.update(&zero, 1);
    uint8_t d[64];
    state.finalize(d, 64);
    Fr lo, hi, r2;
    std::memcpy(lo.l, d, 32);
    std::memcpy(hi.l, d + 32, 32);
    std::memcpy(r2.l, Fr::R2, 32);
    return lo * r2 + (hi * r2) * r2;              // lo R + hi R^2: Montgomery form of lo + hi 2^256
  }
  Fr squeeze_again() { return squeeze(); }
};

}  // namespace prover
}  // namespace summa
