// What the proof of MstInclusionCircuit's constraint system needs of pure host arithmetic: the shape tables (evaluation order,
// rotation sets, permutation columns), halo2's `permute_expression_pair`, and the scalar steps of phases 4-6 of create_proof
// (gate challenges, h(x), SHPLONK's denominators, remainders, weights and linearisation) as plain functions over Fr.
// Shared by the prover (summa_prover.hpp) and the verifier (csrc/verifier_abi.hip).  omega comes from the library
// (sg_domain_constant), so every function takes the points it works on as arguments.
// Plain C++17, no GPU runtime: tests/cpp/proof_host_check.cpp pins these functions against Python integers.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <map>
#include <stdexcept>
#include <utility>
#include <vector>

#include "summa_fr.hpp"

namespace summa {
namespace prover {

// constraint-system constants of MstInclusionCircuit (circuits_halo2_amd/mst_inclusion.py)
constexpr uint32_t NUM_ADVICE = 3, NUM_FIXED = 11, NUM_SIGMA = 6, BLINDING = 5, CHUNK = 4, QUOTIENT_PIECES = 5;
constexpr int ROT_LAST = -(int)(BLINDING + 1);
enum Kind { A_, F_, SIGMA_, Z_, LZ_, PIN_, PTAB_, RANDOM_, H_ };
struct Key {
  Kind kind;
  uint32_t index;
  bool operator<(const Key& o) const { return kind != o.kind ? kind < o.kind : index < o.index; }
};
struct Query { Key key; int rot; };

inline std::vector<Query> eval_order() {  // [REF InclusionVerifier.sol:500-1000, calldata slots 0x03e4 ..]
  std::vector<Query> q = {{{A_, 0}, 0}, {{A_, 1}, 0}, {{A_, 0}, 1}, {{A_, 1}, 1}, {{A_, 2}, 0}, {{A_, 1}, -1}, {{A_, 0}, -1},
                          {{F_, 2}, 0}, {{F_, 3}, 0}, {{F_, 0}, 0}, {{F_, 1}, 0}};
  for (uint32_t j = 4; j < 11; j++) q.push_back({{F_, j}, 0});
  q.push_back({{RANDOM_, 0}, 0});
  for (uint32_t j = 0; j < 6; j++) q.push_back({{SIGMA_, j}, 0});
  for (Query x : std::vector<Query>{{{Z_, 0}, 0}, {{Z_, 0}, 1}, {{Z_, 0}, ROT_LAST}, {{Z_, 1}, 0}, {{Z_, 1}, 1}, {{LZ_, 0}, 0},
                                    {{LZ_, 0}, 1}, {{PIN_, 0}, 0}, {{PIN_, 0}, -1}, {{PTAB_, 0}, 0}})
    q.push_back(x);
  return q;
}
struct RotationSet { std::vector<int> rots; std::vector<Key> polys; };
inline std::vector<RotationSet> rotation_sets() {  // nu order; polynomials in increasing power of zeta [REF :1159-1340]
  std::vector<RotationSet> s(5);
  s[0] = {{-1, 0, 1}, {{A_, 0}, {A_, 1}}};
  s[1].rots = {0};
  s[1].polys = {{A_, 2}, {PTAB_, 0}, {F_, 2}, {F_, 3}, {F_, 0}, {F_, 1}};
  for (uint32_t j = 4; j < 11; j++) s[1].polys.push_back({F_, j});
  for (uint32_t j = 0; j < 6; j++) s[1].polys.push_back({SIGMA_, j});
  s[1].polys.push_back({H_, 0});
  s[1].polys.push_back({RANDOM_, 0});
  s[2] = {{ROT_LAST, 0, 1}, {{Z_, 0}}};
  s[3] = {{0, 1}, {{Z_, 1}, {LZ_, 0}}};
  s[4] = {{-1, 0}, {{PIN_, 0}}};
  return s;
}

// the permutation argument's columns in sigma order: (f2, a0, a1, f3, a2, instance), in chunks of CHUNK.  The kinds carry the
// values of the C ABI's SG_VS_FIXED / _ADVICE / _INSTANCE (summa_gpu.h; asserted where that header is in sight)
constexpr uint32_t COL_FIXED = 2, COL_ADVICE = 3, COL_INSTANCE = 4;
constexpr uint32_t perm_kind[NUM_SIGMA] = {COL_FIXED, COL_ADVICE, COL_ADVICE, COL_FIXED, COL_ADVICE, COL_INSTANCE};
constexpr uint32_t perm_idx[NUM_SIGMA] = {2, 0, 1, 3, 2, 0};

// halo2 `permute_expression_pair` on the usable rows (canonical limbs, rows of 4): A' sorted; S' such that every row
// has A'[i] == S'[i] or A'[i] == A'[i-1].  One-limb tables (range checks) sort by the low limb only.
inline void permute_expression_pair(const uint64_t* inp, const uint64_t* table, size_t rows, uint64_t* a_out, uint64_t* s_out) {
  using Row = std::array<uint64_t, 4>;
  auto less = [](const Row& x, const Row& y) {
    for (int i = 3; i >= 0; i--)
      if (x[i] != y[i]) return x[i] < y[i];
    return false;
  };
  std::vector<Row> a(rows), t(rows);
  std::memcpy(a.data(), inp, 32 * rows);
  std::memcpy(t.data(), table, 32 * rows);
  bool small = true;
  for (auto& r : t) small = small && !(r[1] | r[2] | r[3]);
  if (small) {  // sort 8-byte keys instead of 32-byte rows
    std::vector<uint64_t> ka(rows), kt(rows);
    for (size_t i = 0; i < rows; i++) {
      if (a[i][1] | a[i][2] | a[i][3]) throw std::runtime_error("lookup input value not in the table");
      ka[i] = a[i][0];
      kt[i] = t[i][0];
    }
    const uint64_t top = *std::max_element(kt.begin(), kt.end());
    if (top < (1u << 20)) {  // range tables: counting sort
      std::vector<uint32_t> ca(top + 1, 0), ct(top + 1, 0);
      for (size_t i = 0; i < rows; i++) {
        if (ka[i] > top) throw std::runtime_error("lookup input value not in the table");
        ca[ka[i]]++;
        ct[kt[i]]++;
      }
      size_t ia = 0, it = 0;
      for (uint64_t v = 0; v <= top; v++) {
        for (uint32_t c = 0; c < ca[v]; c++) ka[ia++] = v;
        for (uint32_t c = 0; c < ct[v]; c++) kt[it++] = v;
      }
    } else {
      std::sort(ka.begin(), ka.end());
      std::sort(kt.begin(), kt.end());
    }
    for (size_t i = 0; i < rows; i++) {
      a[i] = Row{ka[i], 0, 0, 0};
      t[i] = Row{kt[i], 0, 0, 0};
    }
  } else {
    std::sort(a.begin(), a.end(), less);
    std::sort(t.begin(), t.end(), less);
  }
  std::vector<Row> s(rows);
  std::vector<size_t> repeated;
  std::vector<bool> used(rows, false);
  size_t ti = 0;
  for (size_t i = 0; i < rows; i++) {
    if (i && a[i] == a[i - 1]) {
      repeated.push_back(i);
      continue;
    }
    while (ti < rows && less(t[ti], a[i])) ti++;   // both sorted: one forward sweep
    if (ti == rows || t[ti] != a[i]) throw std::runtime_error("lookup input value not in the table");
    used[ti] = true;
    s[i] = t[ti++];
  }
  size_t ri = 0;
  for (size_t j = 0; j < rows; j++)
    if (!used[j]) s[repeated[ri++]] = t[j];
  std::memcpy(a_out, a.data(), 32 * rows);
  std::memcpy(s_out, s.data(), 32 * rows);
}

// ------------------------------------------------------------------ phase 4: the gate program's challenges
// challenge i = sum over e in exps[i] of y^e (ProvingKey::gate_challenge_exps); never empty: the kernel takes a pointer
inline std::vector<Fr> gate_challenges(const std::vector<std::vector<uint32_t>>& exps, const Fr& y) {
  uint32_t top = 0;
  for (auto& group : exps)
    for (uint32_t e : group) top = std::max(top, e);
  std::vector<Fr> pw;   // y^0 .. y^top by one product each (an exponentiation per term was 60 us of host time with the device idle)
  if (top < (1u << 16)) {
    pw.resize((size_t)top + 1);
    pw[0] = Fr::one();
    for (uint32_t e = 1; e <= top; e++) pw[e] = pw[e - 1] * y;
  }
  std::vector<Fr> out;
  for (auto& group : exps) {
    Fr v = Fr::zero();
    for (uint32_t e : group) v = v + (pw.empty() ? y.pow((uint64_t)e) : pw[e]);
    out.push_back(v);
  }
  if (out.empty()) out.push_back(Fr::zero());
  return out;
}

// ------------------------------------------------------------------ phase 5: h(x) from the pieces
// h(X) = sum_i x^(n i) h_i(X) is never formed: its one use -- a term of rotation set 1's combination -- takes the five
// pieces themselves with the weights zeta^j x^(n i)
inline std::vector<Fr> xn_powers(const Fr& x_n) {
  std::vector<Fr> p(QUOTIENT_PIECES);
  p[0] = Fr::one();
  for (uint32_t i = 1; i < QUOTIENT_PIECES; i++) p[i] = p[i - 1] * x_n;
  return p;
}
inline Fr h_at_x(const Fr* piece_evals, const Fr& x_n) {   // QUOTIENT_PIECES values h_i(x)
  Fr h = Fr::zero();
  for (uint32_t i = QUOTIENT_PIECES; i-- > 0;) h = h * x_n + piece_evals[i];
  return h;
}

// ------------------------------------------------------------------ phase 6: SHPLONK's scalars
struct RotationPoints {   // x omega^rot
  Fr x, omega, omega_inv;
  Fr operator()(int rot) const { return rot >= 0 ? x * omega.pow((uint64_t)rot) : x * omega_inv.pow((uint64_t)(-rot)); }
};
struct Evaluations {   // the claimed values the multi-open is about
  std::map<std::pair<Key, int>, Fr> at;   // (polynomial, rotation) -> value, the proof's evaluations
  Fr h;                                   // h(x)
  Fr of(const Key& key, int rot) const { return key.kind == H_ ? h : at.at({key, rot}); }
};

// c_j = 1 / prod_{t != j} (p_j - p_t) for the points of every set: they depend only on x, so one host inversion serves all
// of them (Montgomery's trick) instead of one 254-step exponentiation each
inline std::vector<std::vector<Fr>> lagrange_denominators_inv(const std::vector<RotationSet>& sets, const RotationPoints& point) {
  std::vector<std::vector<Fr>> denom_inv(sets.size());
  std::vector<Fr*> slots;
  for (size_t si = 0; si < sets.size(); si++) {
    const auto& rots = sets[si].rots;
    denom_inv[si].assign(rots.size(), Fr::one());
    for (size_t i = 0; i < rots.size(); i++) {
      for (size_t j = 0; j < rots.size(); j++)
        if (j != i) denom_inv[si][i] = denom_inv[si][i] * (point(rots[i]) - point(rots[j]));
      slots.push_back(&denom_inv[si][i]);
    }
  }
  std::vector<Fr> prefix(slots.size());
  Fr run = Fr::one();
  for (size_t t = 0; t < slots.size(); t++) {
    prefix[t] = run;
    run = run * *slots[t];
  }
  Fr inv = run.inv();
  for (size_t t = slots.size(); t-- > 0;) {
    const Fr v = *slots[t];
    *slots[t] = inv * prefix[t];
    inv = inv * v;
  }
  return denom_inv;
}
// zeta^j for the polynomials of every set
inline std::vector<std::vector<Fr>> zeta_powers(const std::vector<RotationSet>& sets, const Fr& zeta) {
  std::vector<std::vector<Fr>> zps(sets.size());
  for (size_t si = 0; si < sets.size(); si++) {
    zps[si].resize(sets[si].polys.size());
    for (size_t j = 0; j < zps[si].size(); j++) zps[si][j] = j ? zps[si][j - 1] * zeta : Fr::one();
  }
  return zps;
}
// r_i(X) through the set's (points, values), the values being the zeta-combination of the set's polynomials there: host
// arithmetic on the evaluations alone.  At most four coefficients: r_i enters the kernels by value, never as a column
inline std::vector<Fr> remainder_coefficients(const RotationSet& set, const std::vector<Fr>& zp, const std::vector<Fr>& denom_inv,
                                              const RotationPoints& point, const Evaluations& evals) {
  std::vector<Fr> pts, vals;
  for (int r : set.rots) {
    pts.push_back(point(r));
    Fr v = Fr::zero();
    for (size_t j = 0; j < set.polys.size(); j++) v = v + zp[j] * evals.of(set.polys[j], r);
    vals.push_back(v);
  }
  if (pts.size() > 4) throw std::runtime_error("rotation set of more than four points");
  std::vector<Fr> rc(pts.size(), Fr::zero());
  for (size_t i = 0; i < pts.size(); i++) {
    std::vector<Fr> basis = {Fr::one()};
    for (size_t j = 0; j < pts.size(); j++) {
      if (j == i) continue;
      std::vector<Fr> nb(basis.size() + 1, Fr::zero());
      for (size_t t = 0; t < basis.size(); t++) {
        nb[t + 1] = nb[t + 1] + basis[t];
        nb[t] = nb[t] - pts[j] * basis[t];
      }
      basis = nb;
    }
    const Fr scale = vals[i] * denom_inv[i];
    for (size_t t = 0; t < basis.size(); t++) rc[t] = rc[t] + scale * basis[t];
  }
  return rc;
}
// f_i / Z_{S_i}: q_i - r_i vanishes on the whole set, and 1 / prod_j (X - p_j) = sum_j c_j / (X - p_j).  So every division of
// every set is an independent exact Kate division at one point, and f = sum_i nu^i f_i / Z_{S_i} is one linear combination
// of the quotients: the points (eleven, set by set) and the weights nu^i c_j
struct Divisions { std::vector<Fr> points, weights; };
inline Divisions division_weights(const std::vector<RotationSet>& sets, const std::vector<std::vector<Fr>>& denom_inv,
                                  const RotationPoints& point, const Fr& nu) {
  Divisions d;
  Fr nu_pow = Fr::one();
  for (size_t si = 0; si < sets.size(); si++) {
    for (size_t j = 0; j < sets[si].rots.size(); j++) {
      d.points.push_back(point(sets[si].rots[j]));
      d.weights.push_back(nu_pow * denom_inv[si][j]);
    }
    nu_pow = nu_pow * nu;
  }
  return d;
}
// mu - point(r) for every rotation of the sets, per set the product of those OUTSIDE the set (Z_{T \ S_i}(mu)), and
// Z_{S_0}(mu).  Nothing is inverted here: the verifier rejects a zero, the prover does not meet one
struct OutsideProducts {
  std::map<int, Fr> mu_minus;
  std::vector<Fr> outside;
  Fr z_s0;
};
inline OutsideProducts outside_products(const std::vector<RotationSet>& sets, const RotationPoints& point, const Fr& mu) {
  OutsideProducts o;
  for (const RotationSet& s : sets)
    for (int r : s.rots)
      if (!o.mu_minus.count(r)) o.mu_minus[r] = mu - point(r);
  for (const RotationSet& s : sets) {
    Fr d = Fr::one();
    for (auto& kv : o.mu_minus)
      if (std::find(s.rots.begin(), s.rots.end(), kv.first) == s.rots.end()) d = d * kv.second;
    o.outside.push_back(d);
  }
  o.z_s0 = Fr::one();
  for (int r : sets[0].rots) o.z_s0 = o.z_s0 * o.mu_minus.at(r);
  return o;
}
// L(X) = sum_i scale_i (q_i(X) - r_i(mu)) - Z_{S_0}(mu) f(X), with q_i = f_i + r_i and scale_i = nu^i Z_{T \ S_i}(mu) / Z_{T \ S_0}(mu):
//      = sum_i scale_i f_i(X) - Z_{S_0}(mu) f(X) + [ sum_i scale_i (r_i(X) - r_i(mu)) ]      (the bracket: at most four coefficients)
// coeffs: the scales of f_0 .. f_4, then -Z_{S_0}(mu) for f; low: the bracket
struct Linearisation { std::vector<Fr> coeffs, low; };
inline Linearisation linearisation(const std::vector<RotationSet>& sets, const std::vector<std::vector<Fr>>& rs,
                                   const RotationPoints& point, const Fr& nu, const Fr& mu) {
  const OutsideProducts o = outside_products(sets, point, mu);
  const Fr d0_inv = o.outside[0].inv();
  Linearisation l;
  l.low.assign(4, Fr::zero());
  Fr nu_pow = Fr::one();
  for (size_t i = 0; i < sets.size(); i++) {
    const Fr scale = nu_pow * o.outside[i] * d0_inv;
    l.coeffs.push_back(scale);
    Fr r_at_mu = Fr::zero();
    for (size_t t = rs[i].size(); t-- > 0;) r_at_mu = r_at_mu * mu + rs[i][t];
    for (size_t t = 0; t < rs[i].size(); t++) l.low[t] = l.low[t] + scale * rs[i][t];
    l.low[0] = l.low[0] - scale * r_at_mu;
    nu_pow = nu_pow * nu;
  }
  l.coeffs.push_back(-o.z_s0);
  return l;
}

}  // namespace prover
}  // namespace summa
