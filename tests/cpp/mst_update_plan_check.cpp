// The HIP-free planning behind sg_mst_update_dev (csrc/mst_update_plan.h) on the host, built by a host compiler alone.
// tests/test_mst_update_cpu.py feeds commands on stdin and compares what is printed with sets of Python integers.
//   o DEPTH                                             mst_level_first of every level 0 .. DEPTH ("first F_0 .. F_DEPTH")
//   p DEPTH M I_0 .. I_{M-1}                            the plan of M leaf indices
//   v DEPTH NC M I_0 .. I_{M-1} K O_0 .. O_{K-1} HEX    mst_update_problem of the indices, K digit offsets and the digit bytes
//                                                       ("-" = none)
// Answers: for p a line "offsets O_0 .. O_DEPTH" and then, for every level l = 1 .. DEPTH, "list l N_0 N_1 .."; for v a line
// "problem TEXT" (TEXT empty: no problem).
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "mst_update_plan.h"

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> v;
  if (s == "-") return v;
  for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
  return v;
}
static bool read_indices(size_t m, std::vector<uint32_t>* out) {
  out->assign(m + 1, 0);   // (one more: a pointer to point at when m = 0)
  for (size_t j = 0; j < m; j++) {
    if (!(std::cin >> (*out)[j])) return false;
  }
  return true;
}

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    uint32_t depth = 0;
    size_t m = 0;
    std::vector<uint32_t> index;
    if (cmd == "p") {
      if (!(std::cin >> depth >> m) || !read_indices(m, &index)) return 2;
      const sg::MstUpdatePlan plan = sg::mst_update_plan(index.data(), m, depth);
      if (plan.offset.size() != (size_t)depth + 1 || plan.nodes.size() != plan.offset[depth]) return 3;
      std::printf("offsets");
      for (uint32_t o : plan.offset) std::printf(" %u", o);
      std::printf("\n");
      for (uint32_t l = 1; l <= depth; l++) {
        std::printf("list %u", l);
        for (uint32_t t = 0; t < plan.count(l); t++) std::printf(" %u", plan.list(l)[t]);
        std::printf("\n");
      }
    } else if (cmd == "o") {
      if (!(std::cin >> depth)) return 2;
      std::printf("first");
      for (uint32_t l = 0; l <= depth; l++) std::printf(" %llu", (unsigned long long)sg::mst_level_first(l, depth));
      std::printf("\n");
    } else if (cmd == "v") {
      uint32_t nc = 0;
      size_t k = 0;
      if (!(std::cin >> depth >> nc >> m) || !read_indices(m, &index) || !(std::cin >> k) || k == 0) return 2;
      std::vector<uint64_t> off(k);
      for (size_t i = 0; i < k; i++) {
        if (!(std::cin >> off[i])) return 2;
      }
      std::string hex;
      if (!(std::cin >> hex)) return 2;
      std::vector<uint8_t> bytes = unhex(hex);
      bytes.push_back(0);
      std::printf("problem %s\n", sg::mst_update_problem(index.data(), bytes.data(), off.data(), m, depth, nc).c_str());
    } else {
      return 2;
    }
  }
  return 0;
}
