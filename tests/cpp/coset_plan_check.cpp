// The host arithmetic of the quotient's cosets (csrc/coset_plan.h) run on the CPU: reads one shape per line from stdin,
//   k ext nc ZETA OMEGA_EXT
// (nc cosets of an extended domain of 2^(k + ext) rows; the two constants as the 64 hex digits of their 32 bytes in memory:
// Montgomery, little-endian, as sg_domain_constant returns them), and prints one line per shape,
//   ok shift=HEX,.. inv_shift=HEX,.. m=HEX,..          (m row-major [t][b], nc * nc entries; the same 32-byte form)
// or the refusal: "singular" (two cosets coincide) or "inside_domain" (a coset on which X^n - 1 vanishes).
// tests/test_coset_cases_cpu.py builds it with plain g++ and compares it with the Python integers of tests/coset_cases.py.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "coset_plan.h"

using summa::prover::Fr;

static bool unhex(const std::string& s, Fr* out) {
  if (s.size() != 64 || s.find_first_not_of("0123456789abcdef") != std::string::npos) return false;
  uint8_t b[32];
  for (size_t i = 0; i < 32; i++) b[i] = (uint8_t)std::stoul(s.substr(2 * i, 2), nullptr, 16);
  std::memcpy(out->l, b, 32);
  return true;
}
static void print_list(const char* name, const std::vector<Fr>& v) {
  std::printf(" %s=", name);
  for (size_t i = 0; i < v.size(); i++) {
    if (i) std::printf(",");
    for (size_t j = 0; j < 32; j++) std::printf("%02x", v[i].bytes()[j]);
  }
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    uint32_t k = 0, ext = 0, nc = 0;
    std::string zeta_hex, omega_hex;
    Fr zeta, omega_ext;
    if (!(in >> k >> ext >> nc >> zeta_hex >> omega_hex) || k < 1 || ext < 1 || k + ext > 28 || nc < 1 || nc > 8 || nc > (1u << ext) ||
        !unhex(zeta_hex, &zeta) || !unhex(omega_hex, &omega_ext)) {
      std::fprintf(stderr, "bad case: %s\n", line.c_str());
      return 2;
    }
    sg::CosetPlan plan;
    const sg::CosetPlanStatus st = sg::coset_plan(k, nc, zeta, omega_ext, &plan);
    if (st != sg::CosetPlanStatus::ok) {
      std::printf("%s\n", st == sg::CosetPlanStatus::singular ? "singular" : "inside_domain");
      continue;
    }
    std::printf("ok");
    print_list("shift", plan.shift);
    print_list("inv_shift", plan.inv_shift);
    print_list("m", plan.m);
    std::printf("\n");
  }
  return 0;
}
