// The names beside a tree in file order and the report of repeated names (csrc/mst_names.h) on the host: the CSV reader's four
// passes (mst_csv_host), the sort's steps (mst_sort_host), then mst_names_host over the tiles and groups the kernels take.
// tests/test_mst_names_cpu.py feeds command lines on stdin:
//   geometry                      -> geometry THREADS TILE GROUP
//   scratch N_ROWS                -> scratch BYTES TILES GROUPS
//   problem D_BYTES LEN BODY_OFF D_NAME_SPANS D_ORDER N_ROWS D_SHADOWED D_FIRST CAP D_SCRATCH SUMMARY_OUT (pointers as integers)
//                                 -> problem WORDS...      (mst_names_problem: nothing behind the word for a good call)
//   file PATH N_CURRENCIES CAP... -> (header line and delimiter as in mst_csv_check.cpp)
//     sort N_ROWS FLAGS(hex) PROBLEM_ROW PROBLEM_CODE
//     order ROW ...               (the file row at every sorted position, when nothing is wrong)
//     spans BEGIN END ...         (the name at every sorted position, offsets into the body)
//     leafspans BEGIN END ...     (the name of every file row: the split's spans, narrowed)
//     find ROW ...                (every file row's own name through the order: the lowest row that holds it; then two absent names)
//     and per CAP, with the order (leaves in file order) and without (leaf i is sorted position i):
//     dups CAP ORDERED(1|0) REPEATED SHADOWED LISTED / shadowed LEAF ... / first LEAF ...
//     end
#include <cstdio>
#include <fstream>
#include <iostream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "mst_names.h"

static void list(const char* what, const std::vector<uint32_t>& v) {
  std::printf("%s", what);
  for (uint32_t x : v) std::printf(" %u", x);
  std::printf("\n");
}

static int file(const std::string& path, uint32_t nc, const std::vector<uint64_t>& caps) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return 2;
  // an exact-size heap copy: a read past the body's end is the sanitizer's to find
  const std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  const size_t eol = text.find('\n');
  if (eol == std::string::npos) return 3;
  const uint8_t delim = text.substr(0, eol).find(';') != std::string::npos ? ';' : ',';
  std::vector<uint8_t> body(text.begin() + eol + 1, text.end());
  const sg::MstCsvHost csv = sg::mst_csv_host(body.data(), body.size(), delim, nc);
  if (csv.flags || !csv.n_rows) {
    std::printf("sort %llu %x 0 0\nend\n", (unsigned long long)csv.n_rows, csv.flags);
    return 0;
  }
  const sg::MstSortHost r = sg::mst_sort_host(body.data(), csv, nc);
  std::printf("sort %llu %x %llu %u\n", (unsigned long long)csv.n_rows, csv.flags, (unsigned long long)(r.problem >> 8),
              (unsigned)(r.problem & 0xff));
  if (r.problem) {
    std::printf("end\n");
    return 0;
  }
  const uint32_t n = (uint32_t)csv.n_rows;
  list("order", r.order);
  list("spans", r.name_spans);
  std::vector<uint64_t> words = csv.words;
  const sg::MstCsvSpans s = sg::mst_csv_spans(words.data(), n, nc);
  std::vector<uint32_t> leaf_spans, found;
  for (uint32_t row = 0; row < n; row++) {
    leaf_spans.push_back((uint32_t)s.name_begin[row]);
    leaf_spans.push_back((uint32_t)s.name_end[row]);
  }
  list("leafspans", leaf_spans);
  auto find = [&](const std::vector<uint8_t>& q) {            // ss_mst_find_leaves: the position found, through the order
    const uint32_t at = sg::mst_find_name(body.data(), body.size(), r.name_spans.data(), n, q.data(), q.size());
    return at == sg::MST_FIND_ABSENT ? at : r.order[at];
  };
  for (uint32_t row = 0; row < n; row++)
    found.push_back(find(std::vector<uint8_t>(body.begin() + leaf_spans[2 * row], body.begin() + leaf_spans[2 * row + 1])));
  found.push_back(find(std::vector<uint8_t>(sg::MST_SORT_NAME_CAP + 1, 0x7f)));   // above every name of the subset
  found.push_back(find(std::vector<uint8_t>(1, 0x00)));                          // below every non-empty one
  list("find", found);
  for (uint64_t cap : caps)
    for (int ordered = 1; ordered >= 0; ordered--) {
      const sg::MstNamesHost d =
          sg::mst_names_host(body.data(), body.size(), r.name_spans.data(), ordered ? r.order.data() : nullptr, n, cap);
      std::printf("dups %llu %d %llu %llu %llu\n", (unsigned long long)cap, ordered, (unsigned long long)d.summary[0],
                  (unsigned long long)d.summary[1], (unsigned long long)d.summary[2]);
      list("shadowed", d.shadowed);
      list("first", d.first);
    }
  std::printf("end\n");
  return 0;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "geometry") {
      std::printf("geometry %u %u %u\n", sg::MST_NAMES_THREADS, sg::MST_NAMES_TILE, sg::MST_NAMES_GROUP);
    } else if (cmd == "scratch") {
      uint64_t n = 0;
      in >> n;
      std::printf("scratch %llu %u %u\n", (unsigned long long)sg::mst_names_scratch_bytes(n), sg::mst_names_tiles(n), sg::mst_names_groups(n));
    } else if (cmd == "problem") {
      uint64_t a[11] = {};
      for (uint64_t& x : a) in >> x;
      auto p = [&](int k) { return reinterpret_cast<const void*>((uintptr_t)a[k]); };
      std::printf("problem %s\n", sg::mst_names_problem(p(0), a[1], a[2], p(3), p(4), a[5], p(6), p(7), a[8], p(9), p(10)).c_str());
    } else if (cmd == "file") {
      std::string path;
      uint32_t nc = 0;
      std::vector<uint64_t> caps;
      in >> path >> nc;
      for (uint64_t cap; in >> cap;) caps.push_back(cap);
      if (const int rc = file(path, nc, caps)) return rc;
    } else if (!cmd.empty()) {
      return 4;
    }
  }
  return 0;
}
