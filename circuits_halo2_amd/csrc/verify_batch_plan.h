// The decisions of the batch verifier (sv_verify_batch in verifier_abi.hip), apart from the device and the pairing: the random
// multipliers that fold N proofs into one check, and the bisection that finds the bad proofs of a rejected batch.  No HIP, no
// library call: tests/cpp/verify_batch_check.cpp runs both on the host.
#pragma once
#include <array>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/summa_transcript.hpp"

namespace sg {
namespace verify_batch {

static constexpr uint32_t MAX_PROOFS = 8192;   // two jobs per proof, 2^14 jobs per launch (msm_many.hip)

// ------------------------------------------------------------------ multipliers
// Every commitment enters a proof's final check linearly, so N checks L_i + (-W'_i paired with [s]_2) fold into one with
// multipliers r_i the prover could not predict: they are derived from everything the batch holds --
//   seed = Keccak256(vk_digest || N || for each proof: len || proof || n_instances || instances || entropy)
// (N and n_instances as 4 little-endian bytes, len as 8, instances as the 32-byte words the caller passed, entropy: 32 bytes of
// the caller's, zeros if none) -- and r_i = the low 128 bits of Keccak256(seed || i), i as 4 little-endian bytes; 0 becomes 1.
struct ProofView {
  const uint8_t* proof;
  size_t len;
  const uint8_t* instances;   // n_instances x 32 B
  uint32_t n_instances;
};
using Digest = std::array<uint8_t, 32>;

inline Digest seed(const uint8_t vk_digest[32], const ProofView* proofs, uint32_t n, const uint8_t* entropy /* 32 B or null */) {
  std::vector<uint8_t> buf(vk_digest, vk_digest + 32);
  auto le = [&](uint64_t v, int bytes) {
    for (int i = 0; i < bytes; i++) buf.push_back((uint8_t)(v >> (8 * i)));
  };
  le(n, 4);
  for (uint32_t i = 0; i < n; i++) {
    const ProofView& p = proofs[i];
    le(p.len, 8);
    buf.insert(buf.end(), p.proof, p.proof + p.len);
    le(p.n_instances, 4);
    buf.insert(buf.end(), p.instances, p.instances + 32 * (size_t)p.n_instances);
  }
  if (entropy) buf.insert(buf.end(), entropy, entropy + 32);
  else buf.insert(buf.end(), 32, 0);
  return summa::prover::keccak256(buf.data(), buf.size());
}

// r_i as 16 little-endian bytes, never zero
inline std::array<uint8_t, 16> multiplier(const Digest& s, uint32_t i) {
  uint8_t buf[36];
  std::memcpy(buf, s.data(), 32);
  for (int b = 0; b < 4; b++) buf[32 + b] = (uint8_t)(i >> (8 * b));
  const Digest h = summa::prover::keccak256(buf, sizeof buf);
  std::array<uint8_t, 16> r;
  std::memcpy(r.data(), h.data(), 16);   // the digest read as a little-endian integer: its low 128 bits
  bool zero = true;
  for (uint8_t b : r) zero = zero && b == 0;
  if (zero) r[0] = 1;
  return r;
}

// ------------------------------------------------------------------ bisection
struct Range {   // proofs [a, b)
  uint32_t a, b;
};
struct Verdicts {
  std::vector<uint8_t> accepted;   // per proof, 0 / 1
  uint32_t checks = 0;             // pairing checks made
};

// `live`: the proofs that passed the host part, ascending (the others are rejected already and hold empty jobs, so a range of
// proofs may span them).  `accepts(ranges)` answers, per range, whether the folded check over its proofs holds.  It is called with
// ONE range (the whole batch; a single proof) or with the TWO halves of a rejected range, which its sums can then serve in one
// launch: it decides the first half, and the second only if the first was rejected -- a rejected range whose first half is accepted
// has its fault in the second, which is rejected without a check of its own (its verdict is not read) but still descended.  A
// single proof that was only ever rejected by such an inference is decided by its own check at the leaf: since r_i != 0 that is the
// individual check, so a proof is never rejected on the word of a range.  Every call works on a strictly smaller range: the
// function ends whatever `accepts` answers.
template <class Accepts>
Verdicts bisect(const std::vector<uint32_t>& live, uint32_t n_proofs, Accepts&& accepts) {
  Verdicts out;
  out.accepted.assign(n_proofs, 0);
  if (live.empty()) return out;
  auto range = [&](size_t lo, size_t hi) { return Range{live[lo], live[hi - 1] + 1}; };
  auto accept_all = [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) out.accepted[live[i]] = 1;
  };
  struct Node {
    size_t lo, hi;
    bool checked;   // rejected by a check of its own (false: by inference)
  };
  out.checks = 1;
  if (accepts(std::vector<Range>{range(0, live.size())})[0]) {
    accept_all(0, live.size());
    return out;
  }
  std::vector<Node> rejected{{0, live.size(), true}};
  while (!rejected.empty()) {
    const Node nd = rejected.back();
    rejected.pop_back();
    if (nd.hi - nd.lo == 1) {
      if (!nd.checked) {
        out.checks++;
        if (accepts(std::vector<Range>{range(nd.lo, nd.hi)})[0]) accept_all(nd.lo, nd.hi);
      }
      continue;
    }
    const size_t mid = nd.lo + (nd.hi - nd.lo) / 2;
    const std::vector<uint8_t> v = accepts(std::vector<Range>{range(nd.lo, mid), range(mid, nd.hi)});
    out.checks++;
    if (v[0]) {
      accept_all(nd.lo, mid);
      rejected.push_back({mid, nd.hi, false});
      continue;
    }
    rejected.push_back({nd.lo, mid, true});
    out.checks++;
    if (v[1]) accept_all(mid, nd.hi);
    else rejected.push_back({mid, nd.hi, true});
  }
  return out;
}

}  // namespace verify_batch
}  // namespace sg
