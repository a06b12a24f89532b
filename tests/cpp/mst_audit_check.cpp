// Runs the serial steps of csrc/mst_audit.h -- the text the kernels of mst_audit.cuh compile -- for tests/test_mst_audit_cpu.py.
// Commands on stdin, one per line, values as hexadecimal canonical integers:
//   geometry                                 -> "geometry <threads> <tile> <group>"
//   scratch <depth>                          -> "scratch <bytes> <tiles> <groups>"
//   pred <n_bytes> <value>                   -> "pred <0|1>"
//   audit <depth> <nc> <n_bytes> <bad_cap> <(2^(depth+1) - 1) * nc values, level-major>
//                                            -> "flags ..", "masks ..", "bad ..", "summary <4 words>"
//   problem <balances> <depth> <nc> <n_bytes> <flags> <reasons> <bad> <bad_cap> <scratch> <summary>   (pointers as integers)
//                                            -> "problem <text>"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "mst_audit.h"

using namespace sg;

static void words_of(const std::string& hex, uint32_t w[8]) {
  for (int k = 0; k < 8; k++) w[k] = 0;
  if (hex.size() > 64) {
    std::fprintf(stderr, "a value of more than 256 bits\n");
    std::exit(2);
  }
  for (size_t d = 0; d < hex.size(); d++) {
    const char ch = hex[hex.size() - 1 - d];
    const uint32_t v = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : 99;
    if (v == 99) {
      std::fprintf(stderr, "not a hexadecimal digit\n");
      std::exit(2);
    }
    w[d / 8] |= v << (4 * (d % 8));
  }
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    if (cmd == "geometry") {
      std::printf("geometry %u %u %u\n", MST_AUDIT_THREADS, MST_AUDIT_TILE, MST_AUDIT_GROUP);
    } else if (cmd == "scratch") {
      uint32_t depth;
      in >> depth;
      std::printf("scratch %llu %u %u\n", (unsigned long long)mst_audit_scratch_bytes(depth), mst_audit_tiles(depth), mst_audit_groups(depth));
    } else if (cmd == "pred") {
      uint32_t n_bytes, w[8];
      std::string hex;
      in >> n_bytes >> hex;
      words_of(hex, w);
      std::printf("pred %d\n", mst_audit_in_range(w, n_bytes) ? 1 : 0);
    } else if (cmd == "audit") {
      uint32_t depth, nc, n_bytes;
      uint64_t bad_cap;
      in >> depth >> nc >> n_bytes >> bad_cap;
      const size_t count = (size_t)mst_audit_nodes(depth) * nc;
      std::vector<uint32_t> canon(8 * count);
      std::string hex;
      for (size_t i = 0; i < count; i++) {
        if (!(in >> hex)) {
          std::fprintf(stderr, "audit: %zu values expected\n", count);
          return 2;
        }
        words_of(hex, canon.data() + 8 * i);
      }
      for (uint32_t level = 0; level <= depth; level++)       // the 32-bit node numbers are mst_update_plan.h's
        if (mst_audit_node(level, 0, depth) != mst_level_first(level, depth)) {
          std::fprintf(stderr, "mst_audit_node disagrees with mst_level_first\n");
          return 3;
        }
      const MstAuditHost r = mst_audit_host(canon.data(), depth, nc, n_bytes, bad_cap);
      std::printf("flags");
      for (uint8_t f : r.flags) std::printf(" %u", f);
      std::printf("\nmasks");
      for (uint32_t m : r.masks) std::printf(" %u", m);
      std::printf("\nbad");
      for (uint32_t b : r.bad) std::printf(" %u", b);
      std::printf("\nsummary %llu %llu %llu %llu\n", (unsigned long long)r.summary[0], (unsigned long long)r.summary[1],
                  (unsigned long long)r.summary[2], (unsigned long long)r.summary[3]);
    } else if (cmd == "problem") {
      uint64_t bal, flags, reasons, bad, bad_cap, scratch, summary;
      uint32_t depth, nc, n_bytes;
      in >> bal >> depth >> nc >> n_bytes >> flags >> reasons >> bad >> bad_cap >> scratch >> summary;
      auto p = [](uint64_t v) { return reinterpret_cast<const void*>((uintptr_t)v); };
      std::printf("problem %s\n", mst_audit_problem(p(bal), depth, nc, n_bytes, p(flags), p(reasons), p(bad), bad_cap, p(scratch), p(summary)).c_str());
    } else {
      std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
