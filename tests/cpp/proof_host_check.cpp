// Prints what the HIP-free headers of the compiled prover compute, for tests/test_proof_host_cpu.py to compare with Python
// integers: the shape tables, the gate challenges, h(x), and every scalar of the SHPLONK multi-open.  Includes only the three
// headers and builds with a host compiler alone, no ROCm include path -- which is itself the check that they are HIP-free:
//   g++ -std=c++17 -Wall -Wextra -Werror -fsanitize=address,undefined -Iinclude tests/cpp/proof_host_check.cpp
// stdin (whitespace-separated; field elements as 64 hex digits, big-endian, canonical):
//   k omega x y zeta nu mu, the evaluations in eval_order(), the QUOTIENT_PIECES evaluations h_i(x),
//   the number of gate-challenge cases, per case the number of groups, per group its length and exponents,
//   the number of Fq conversions, per conversion 64 hex digits (the 32 Montgomery bytes as the C ABI returns them)
// stdout: one line per result, `name values...`
#include <cstdio>
#include <iostream>
#include <string>

#include "summa_fr.hpp"
#include "summa_proof_host.hpp"
#include "summa_transcript.hpp"

using namespace summa::prover;

static void bytes_from_hex(const std::string& h, uint8_t out[32]) {
  if (h.size() != 64) throw std::runtime_error("64 hex digits expected");
  for (int i = 0; i < 32; i++) out[i] = (uint8_t)std::stoul(h.substr(2 * i, 2), nullptr, 16);
}
static Fr read_fr() {
  std::string h;
  std::cin >> h;
  uint8_t b[32];
  bytes_from_hex(h, b);
  return Fr::from_be_bytes_reduced(b);
}
static void put_hex(const uint8_t* b, size_t len) {
  std::printf(" ");
  for (size_t i = 0; i < len; i++) std::printf("%02x", b[i]);
}
static void put(const Fr& v) {
  uint8_t b[32];
  v.to_be_bytes(b);
  put_hex(b, 32);
}
static void line(const char* name, const std::vector<Fr>& vs) {
  std::printf("%s", name);
  for (const Fr& v : vs) put(v);
  std::printf("\n");
}
static const char* KIND[] = {"a", "f", "sigma", "z", "lz", "pin", "ptab", "random", "h"};

int main() {
  try {
    // the shape tables, as circuits_halo2_amd/prover.py spells them
    const auto order = eval_order();
    const auto sets = rotation_sets();
    for (const Query& q : order) std::printf("eval_order %s %u %d\n", KIND[q.key.kind], q.key.index, q.rot);
    for (const RotationSet& s : sets) {
      std::printf("rotation_set");
      for (int r : s.rots) std::printf(" %d", r);
      std::printf(" |");
      for (const Key& key : s.polys) std::printf(" %s:%u", KIND[key.kind], key.index);
      std::printf("\n");
    }
    for (uint32_t c = 0; c < NUM_SIGMA; c++) std::printf("perm %u %u\n", perm_kind[c], perm_idx[c]);

    uint32_t k;
    std::cin >> k;
    const size_t n = (size_t)1 << k;
    const Fr omega = read_fr(), x = read_fr(), y = read_fr(), zeta = read_fr(), nu = read_fr(), mu = read_fr();
    const RotationPoints point{x, omega, omega.pow((uint64_t)(n - 1))};
    Evaluations evals;
    for (const Query& q : order) evals.at[{q.key, q.rot}] = read_fr();
    std::vector<Fr> piece_evals;
    for (uint32_t i = 0; i < QUOTIENT_PIECES; i++) piece_evals.push_back(read_fr());

    const Fr x_n = x.pow((uint64_t)n);
    line("xn_pow", xn_powers(x_n));
    evals.h = h_at_x(piece_evals.data(), x_n);
    line("h_eval", {evals.h});
    for (int r : {ROT_LAST, -1, 0, 1}) {
      std::printf("point %d", r);
      put(point(r));
      std::printf("\n");
    }
    const auto denom_inv = lagrange_denominators_inv(sets, point);
    const auto zps = zeta_powers(sets, zeta);
    std::vector<std::vector<Fr>> rs;
    for (size_t si = 0; si < sets.size(); si++) {
      line("denom_inv", denom_inv[si]);
      rs.push_back(remainder_coefficients(sets[si], zps[si], denom_inv[si], point, evals));
      line("r", rs[si]);
    }
    const Divisions div = division_weights(sets, denom_inv, point, nu);
    line("div_points", div.points);
    line("div_weights", div.weights);
    const OutsideProducts op = outside_products(sets, point, mu);
    for (auto& kv : op.mu_minus) {
      std::printf("mu_minus %d", kv.first);
      put(kv.second);
      std::printf("\n");
    }
    line("outside", op.outside);
    line("z_s0", {op.z_s0});
    const Linearisation lin = linearisation(sets, rs, point, nu, mu);
    line("lin_coeffs", lin.coeffs);
    line("lin_low", lin.low);
    {   // a rotation set of five points is refused
      RotationSet five{{-2, -1, 0, 1, 2}, {{A_, 0}}};
      Evaluations e5;
      for (int r : five.rots) e5.at[{five.polys[0], r}] = Fr::one();
      bool refused = false;
      try {
        remainder_coefficients(five, {Fr::one()}, std::vector<Fr>(5, Fr::one()), point, e5);
      } catch (const std::runtime_error&) {
        refused = true;
      }
      std::printf("five_points_refused %d\n", (int)refused);
    }

    size_t cases;
    std::cin >> cases;
    for (size_t c = 0; c < cases; c++) {
      size_t groups;
      std::cin >> groups;
      std::vector<std::vector<uint32_t>> exps(groups);
      for (auto& g : exps) {
        size_t len;
        std::cin >> len;
        g.resize(len);
        for (auto& e : g) std::cin >> e;
      }
      line("gate_challenges", gate_challenges(exps, y));
    }

    // the Fq byte conversion (through the same Montgomery code as Fr) and the constants it rests on
    using Fq = Mont<FqModulus>;
    std::printf("fq_constants %d\n", (int)(Fq::one() * Fq::one() == Fq::one() && Fq::from_u64(1) == Fq::one() && Fr::from_u64(1) == Fr::one()));
    size_t conversions;
    std::cin >> conversions;
    for (size_t c = 0; c < conversions; c++) {
      std::string h;
      std::cin >> h;
      uint8_t in[32], out[32];
      bytes_from_hex(h, in);
      fq_mont_to_be(in, out);
      std::printf("fq_be");
      put_hex(out, 32);
      std::printf("\n");
    }

    // both transcripts: write_scalar(x), common_scalar(y), squeeze, squeeze
    {
      EvmTranscript tr;
      tr.write_scalar(x);
      tr.common_scalar(y);
      const Fr c1 = tr.squeeze(), c2 = tr.squeeze_again();
      line("evm_squeeze", {c1, c2});
      std::printf("evm_proof");
      put_hex(tr.proof.data(), tr.proof.size());
      std::printf("\n");
    }
    {
      Blake2bTranscript tr;
      tr.write_scalar(x);
      tr.common_scalar(y);
      const Fr c1 = tr.squeeze(), c2 = tr.squeeze_again();
      line("blake2b_squeeze", {c1, c2});
      std::printf("blake2b_proof");
      put_hex(tr.proof.data(), tr.proof.size());
      std::printf("\n");
    }
    if (!std::cin) throw std::runtime_error("short input");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "proof_host_check: %s\n", e.what());
    return 1;
  }
  return 0;
}
