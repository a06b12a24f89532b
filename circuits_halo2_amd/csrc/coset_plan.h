// The host arithmetic behind the quotient's cosets (quotient.h): for the first nc cosets c_b H of the 2^k domain H, c_b = zeta
// omega_ext^b, the shifts, their inverses, and M = V^-1 diag(1 / (g_b - 1)) with g_b = c_b^n and V[b][t] = g_b^t, which takes
// the blocks' inverse transforms to the quotient's pieces.  Host Fr only, no HIP: tests/cpp/coset_plan_check.cpp runs it
// without a GPU.
#pragma once
#include <utility>
#include <vector>

#include "../../include/summa_fr.hpp"

namespace sg {

enum class CosetPlanStatus { ok, singular, inside_domain };   // singular: two cosets coincide; inside_domain: some g_b = 1
struct CosetPlan {
  std::vector<summa::prover::Fr> shift, inv_shift;   // [nc]
  std::vector<summa::prover::Fr> m;                  // [nc][nc], row-major [t][b]
};
inline CosetPlanStatus coset_plan(uint32_t k, uint32_t nc, const summa::prover::Fr& zeta, const summa::prover::Fr& omega_ext, CosetPlan* out) {
  using summa::prover::Fr;
  std::vector<Fr> gamma(nc);
  out->shift.resize(nc);
  out->inv_shift.resize(nc);
  for (uint32_t b = 0; b < nc; b++) {
    out->shift[b] = zeta * omega_ext.pow((uint64_t)b);
    out->inv_shift[b] = out->shift[b].inv();
    gamma[b] = out->shift[b].pow((uint64_t)1 << k);
  }
  // inverse of V by Gauss-Jordan on [V | I]
  std::vector<std::vector<Fr>> a(nc, std::vector<Fr>(2 * nc, Fr::zero()));
  for (uint32_t b = 0; b < nc; b++) {
    Fr pw = Fr::one();
    for (uint32_t t = 0; t < nc; t++) {
      a[b][t] = pw;
      pw = pw * gamma[b];
    }
    a[b][nc + b] = Fr::one();
  }
  for (uint32_t col = 0; col < nc; col++) {
    uint32_t piv = col;
    while (piv < nc && a[piv][col].is_zero()) piv++;
    if (piv == nc) return CosetPlanStatus::singular;
    std::swap(a[piv], a[col]);
    const Fr inv = a[col][col].inv();
    for (auto& v : a[col]) v = v * inv;
    for (uint32_t r = 0; r < nc; r++) {
      if (r == col || a[r][col].is_zero()) continue;
      const Fr f = a[r][col];
      for (uint32_t q = 0; q < 2 * nc; q++) a[r][q] = a[r][q] - f * a[col][q];
    }
  }
  out->m.resize((size_t)nc * nc);
  for (uint32_t b = 0; b < nc; b++) {
    const Fr d = gamma[b] - Fr::one();
    if (d.is_zero()) return CosetPlanStatus::inside_domain;
    const Fr di = d.inv();
    for (uint32_t t = 0; t < nc; t++) out->m[(size_t)t * nc + b] = a[t][nc + b] * di;
  }
  return CosetPlanStatus::ok;
}

}  // namespace sg
