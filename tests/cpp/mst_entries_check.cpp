// The HIP-free arithmetic behind sg_mst_entries_dev (csrc/keccak_f1600.h, csrc/mst_entries.h) on the host: the text the
// kernels compile, built by a host compiler alone.  tests/test_mst_entries_cpu.py feeds commands on stdin and compares what
// is printed with the oracle; the reduction of a digest is also compared here with summa_fr.hpp's.
//   k LEN       Keccak-256 of LEN bytes, byte j = (7 j + LEN) & 0xff, read from an odd address
//   m HEX       Keccak-256 of the given bytes ("-" = none), read from an odd address
//   b HEX64     32 bytes as a big-endian integer mod r
//   d DIGITS    a decimal string mod r
// Answers: "digest HEX" and "username HEX fr_same=0|1" for k / m, "reduced HEX fr_same=0|1" for b, "decimal HEX" for d;
// field elements as their 32 bytes in memory (Montgomery, little-endian).
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "keccak_f1600.h"
#include "mst_entries.h"
#include "summa_fr.hpp"

static std::string hex(const uint8_t* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; i++) {
    s.push_back(d[p[i] >> 4]);
    s.push_back(d[p[i] & 15]);
  }
  return s;
}
static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> v;
  if (s == "-") return v;
  for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
  return v;
}
// the digest's lanes -> field element, printed beside summa_fr.hpp's reduction of the same 32 bytes
static void print_reduced(const char* tag, const uint64_t lanes[4]) {
  uint8_t digest[32];
  std::memcpy(digest, lanes, 32);   // (little-endian host: lane i is bytes 8 i .. 8 i + 8)
  uint32_t w[8];
  sg::mst_username_words(lanes, w);
  const summa::prover::Fr want = summa::prover::Fr::from_be_bytes_reduced(digest);
  std::printf("%s %s fr_same=%d\n", tag, hex(reinterpret_cast<const uint8_t*>(w), 32).c_str(), std::memcmp(w, want.l, 32) == 0);
}
static void hash(const std::vector<uint8_t>& msg) {
  std::vector<uint8_t> buf(msg.size() + 1);   // the message starts at an odd address
  if (!msg.empty()) std::memcpy(buf.data() + 1, msg.data(), msg.size());
  uint64_t lanes[4];
  sg::keccak256_lanes(buf.data() + 1, msg.size(), lanes);
  std::printf("digest %s\n", hex(reinterpret_cast<const uint8_t*>(lanes), 32).c_str());
  print_reduced("username", lanes);
}

int main() {
  std::string cmd, arg;
  while (std::cin >> cmd >> arg) {
    if (cmd == "k") {
      const size_t len = std::stoul(arg);
      std::vector<uint8_t> msg(len);
      for (size_t j = 0; j < len; j++) msg[j] = (uint8_t)((7 * j + len) & 0xff);
      hash(msg);
    } else if (cmd == "m") {
      hash(unhex(arg));
    } else if (cmd == "b") {
      const std::vector<uint8_t> b = unhex(arg);
      if (b.size() != 32) return 2;
      uint64_t lanes[4];
      std::memcpy(lanes, b.data(), 32);
      print_reduced("reduced", lanes);
    } else if (cmd == "d") {
      uint32_t w[8];
      sg::mst_decimal_words(reinterpret_cast<const uint8_t*>(arg.data()), arg.size(), w);
      std::printf("decimal %s\n", hex(reinterpret_cast<const uint8_t*>(w), 32).c_str());
    } else {
      return 2;
    }
  }
  return 0;
}
