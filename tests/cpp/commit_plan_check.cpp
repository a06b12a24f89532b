// The host decisions of a commitment (csrc/commit_plan.h) run on the CPU: reads one case per line from stdin and prints the
// rule's answer, one line per case.  tests/test_commit_plan_cpu.py builds it with plain g++ and restates each rule.
//   s K BASIS N  P0 C0 N0  P1 C1 N1  P2 C2 N2           -> basis diff fixed table chunks       (resolve_basis, commit_goes_in_chunks)
//   m K N  P0 C0 N0  P1 C1 N1  P2 C2 N2  COUNT B..      -> fixed diff_ok all_sparse | b.. | flags..             (resolve_mixed)
//   h ALL_SPARSE FIXED COUNT LOG_SEG N                  -> 0 or 1                                       (sparse_hint_applies)
//   g LIMIT COUNT N..                                   -> first:count ..                   (fused_groups; limit(0) = MAX_FUSED)
//   c PARAM N                                           -> K lo[0] .. lo[K]                (host_chunk_count, host_chunk_bounds)
//   p K OP I                                            -> the calls in order, then ret=CODE               (run_chunk_pipeline)
// (Pj Cj Nj: table j exists, its window width, its row length.)  `p` drives the pipeline with operations that only record
// themselves -- S copy_scalars, B copy_bases, F front, b back, f finish, each followed by the chunk -- and of which the one
// named by OP and I fails with a code of its own (marked `!` in the record); OP `-` fails nothing.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "commit_plan.h"

static bool read_tables(std::istream& in, sg::SrsTables* t) {
  for (auto& tab : t->tab) {
    int present = 0;
    if (!(in >> present >> tab.c >> tab.n)) return false;
    tab.present = present != 0;
  }
  return true;
}

struct Recorder {
  char fail_op;
  uint32_t fail_i;
  std::string record;
  int call(char op, uint32_t i) {
    const bool fails = op == fail_op && i == fail_i;
    record += std::string(record.empty() ? "" : " ") + op + std::to_string(i) + (fails ? "!" : "");
    return fails ? 1000 + 10 * (int)op + (int)i : 0;
  }
  int copy_scalars(uint32_t i) { return call('S', i); }
  int copy_bases(uint32_t i) { return call('B', i); }
  int front(uint32_t i) { return call('F', i); }
  int back(uint32_t i) { return call('b', i); }
  int finish(uint32_t i) { return call('f', i); }
};

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    char cmd = 0;
    in >> cmd;
    bool ok = true;
    if (cmd == 's') {
      sg::SrsTables t;
      int basis = 0;
      size_t n = 0;
      ok = (in >> t.k >> basis >> n) && read_tables(in, &t) && basis >= 0 && basis <= 2;
      if (ok) {
        const sg::BasisChoice ch = sg::resolve_basis(t, basis, n);
        std::printf("%d %d %d %d %d\n", ch.basis, (int)ch.diff, (int)ch.fixed, ch.table, (int)sg::commit_goes_in_chunks(t, basis, n));
      }
    } else if (cmd == 'm') {
      sg::SrsTables t;
      size_t n = 0, count = 0;
      ok = (in >> t.k >> n) && read_tables(in, &t) && (in >> count) && count <= 1024;
      std::vector<int> basis(count);
      for (size_t i = 0; ok && i < count; i++) ok = (in >> basis[i]) && basis[i] >= 0 && (basis[i] & ~SG_BASIS_SPARSE) <= 2;
      if (ok) {
        const sg::MixedChoice m = sg::resolve_mixed(t, basis.data(), count, n);
        std::printf("%d %d %d |", (int)m.fixed, (int)m.diff_ok, (int)m.all_sparse);
        for (uint8_t b : m.b) std::printf(" %d", (int)b);
        std::printf(" |");
        for (uint8_t f : m.flags) std::printf(" %d", (int)f);
        std::printf("\n");
      }
    } else if (cmd == 'h') {
      int all_sparse = 0, fixed = 0;
      size_t count = 0, n = 0;
      uint32_t log_seg = 0;
      ok = (bool)(in >> all_sparse >> fixed >> count >> log_seg >> n);
      if (ok) std::printf("%d\n", (int)sg::sparse_hint_applies(all_sparse != 0, fixed != 0, count, log_seg, n));
    } else if (cmd == 'g') {
      size_t limit = 0, count = 0;
      ok = (in >> limit >> count) && limit >= 1 && count <= 1024;
      std::vector<size_t> n(count);
      for (size_t i = 0; ok && i < count; i++) ok = (bool)(in >> n[i]);
      if (ok) {
        const auto groups = sg::fused_groups(n.data(), count, [&](size_t len) { return len ? limit : sg::MAX_FUSED; });
        for (size_t i = 0; i < groups.size(); i++) std::printf("%s%zu:%zu", i ? " " : "", groups[i].first, groups[i].count);
        std::printf("\n");
      }
    } else if (cmd == 'c') {
      int param = 0;
      size_t n = 0;
      ok = (bool)(in >> param >> n);
      if (ok) {
        const uint32_t K = sg::host_chunk_count(param, n);
        std::printf("%u", K);
        for (size_t lo : sg::host_chunk_bounds(n, K)) std::printf(" %zu", lo);
        std::printf("\n");
      }
    } else if (cmd == 'p') {
      uint32_t K = 0;
      Recorder rec{};
      ok = (in >> K >> rec.fail_op >> rec.fail_i) && K >= 1 && K <= sg::MSM_HOST_CHUNKS_MAX;
      if (ok) {
        const int ret = sg::run_chunk_pipeline(K, rec);
        std::printf("%s ret=%d\n", rec.record.c_str(), ret);
      }
    } else {
      ok = false;
    }
    if (!ok) {
      std::fprintf(stderr, "bad case: %s\n", line.c_str());
      return 2;
    }
  }
  return 0;
}
