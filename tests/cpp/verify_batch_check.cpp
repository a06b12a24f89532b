// The batch verifier's decisions (csrc/verify_batch_plan.h) run on the CPU: reads one case per line from stdin,
//   mult <vk digest hex> <entropy hex | -> <proof hex | -> <instances hex | -> [<proof hex | -> <instances hex | -> ...]
//     prints the seed and then r_i for every proof, 16 bytes little-endian, as hex
//   bisect <honest | liar> <n_proofs> <dead: i,i,.. | -> <bad: i,i,.. | ->
//     runs the bisection over the proofs that are not `dead` (rejected by the host part) with a simulated `accepts`: honest -- a
//     range is accepted iff it holds no bad proof; liar -- the whole batch is rejected and every other range accepted.  Prints the
//     verdicts as a string of 0 / 1, the checks counted, the calls made and the most ranges one call carried.
// tests/test_verify_batch_cpu.py builds it with plain g++ and compares it with a restatement in Python.
#include <cstdio>
#include <iostream>
#include <set>
#include <sstream>
#include <string>

#include "verify_batch_plan.h"

namespace vb = sg::verify_batch;

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
  return out;
}
template <class T>
static std::string hex(const T& bytes) {
  std::string out;
  char b[3];
  for (uint8_t v : bytes) {
    std::snprintf(b, sizeof b, "%02x", v);
    out += b;
  }
  return out;
}
static std::set<uint32_t> index_set(const std::string& s) {
  std::set<uint32_t> out;
  if (s == "-") return out;
  std::istringstream in(s);
  std::string item;
  while (std::getline(in, item, ',')) out.insert((uint32_t)std::stoul(item));
  return out;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "mult") {
      std::string digest, entropy, a, b;
      in >> digest >> entropy;
      const std::vector<uint8_t> d = unhex(digest), e = unhex(entropy);
      std::vector<std::vector<uint8_t>> proofs, insts;
      while (in >> a >> b) {
        proofs.push_back(unhex(a));
        insts.push_back(unhex(b));
      }
      if (d.size() != 32 || (!e.empty() && e.size() != 32)) return 2;
      std::vector<vb::ProofView> views;
      for (size_t i = 0; i < proofs.size(); i++) {
        if (insts[i].size() % 32) return 2;
        views.push_back({proofs[i].data(), proofs[i].size(), insts[i].data(), (uint32_t)(insts[i].size() / 32)});
      }
      const vb::Digest s = vb::seed(d.data(), views.data(), (uint32_t)views.size(), e.empty() ? nullptr : e.data());
      std::printf("%s", hex(s).c_str());
      for (uint32_t i = 0; i < views.size(); i++) std::printf(" %s", hex(vb::multiplier(s, i)).c_str());
      std::printf("\n");
    } else if (what == "bisect") {
      std::string mode, dead_s, bad_s;
      uint32_t n = 0;
      in >> mode >> n >> dead_s >> bad_s;
      if ((mode != "honest" && mode != "liar") || n == 0 || n > vb::MAX_PROOFS) return 2;
      const std::set<uint32_t> dead = index_set(dead_s), bad = index_set(bad_s);
      std::vector<uint32_t> live;
      for (uint32_t i = 0; i < n; i++)
        if (!dead.count(i)) live.push_back(i);
      uint32_t calls = 0, most = 0;
      bool bad_call = false;
      auto accepts = [&](const std::vector<vb::Range>& ranges) {
        calls++;
        most = std::max<uint32_t>(most, (uint32_t)ranges.size());
        std::vector<uint8_t> v;
        for (const vb::Range& r : ranges) {
          if (r.a >= r.b || r.b > n) bad_call = true;
          if (mode == "liar") {
            v.push_back(calls == 1 ? 0 : 1);
            continue;
          }
          bool ok = true;
          for (uint32_t i = r.a; i < r.b; i++) ok = ok && !(bad.count(i) && !dead.count(i));   // a dead proof's jobs are empty
          v.push_back(ok ? 1 : 0);
        }
        return v;
      };
      const vb::Verdicts out = vb::bisect(live, n, accepts);
      if (bad_call || out.accepted.size() != n) return 3;
      std::string verdicts;
      for (uint8_t a : out.accepted) verdicts += a ? '1' : '0';
      std::printf("%s %u %u %u\n", verdicts.c_str(), out.checks, calls, most);
    } else {
      std::fprintf(stderr, "bad case: %s\n", line.c_str());
      return 2;
    }
  }
  return 0;
}
