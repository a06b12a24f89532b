// The device sort of a snapshot's usernames (csrc/mst_sort.h) on the host: the CSV reader's four passes (mst_csv_host), then the
// sort's steps one after the other over the tiles the kernels take -- lengths, head, one pass per byte position from the last
// to the first, gather.  tests/test_mst_sort_cpu.py writes files and feeds "PATH N_CURRENCIES" lines on stdin; header line and
// delimiter as in mst_csv_check.cpp.  Answers, per file:
//   body OFFSET DELIMITER(decimal) TILE_ROWS NAME_CAP
//   geom SCAN_BLOCK SCAN_ITEMS BINS TILES SCAN_STEPS   (the scan's width, the rows' tiles and the steps of a pass's scan)
//   sort N_ROWS FLAGS(hex) PROBLEM_ROW PROBLEM_CODE LONGEST PASSES_RUN
//   order ROW ...                    (the file row of every leaf, when nothing is wrong)
//   spans BEGIN END ...              (every leaf's name, offsets into the body)
//   find INDEX ...                   (mst_find_name of every row's own name, then of two names that are absent)
//   end
// With arguments it reads no file: every argument is a row count, answered by its "geom" line alone.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>

#include "mst_sort.h"

static void geom(uint64_t n_rows) {
  std::printf("geom %u %u %u %llu %llu\n", sg::MST_SORT_SCAN_BLOCK, sg::MST_SORT_SCAN_ITEMS, sg::MST_SORT_BINS,
              (unsigned long long)sg::mst_sort_tiles(n_rows), (unsigned long long)sg::mst_sort_scan_steps(n_rows));
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; i++) geom(std::stoull(argv[i]));
  if (argc > 1) return 0;
  std::string path;
  uint32_t nc;
  while (std::cin >> path >> nc) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return 2;
    // an exact-size heap copy: a read past the body's end is the sanitizer's to find
    const std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const size_t eol = text.find('\n');
    if (eol == std::string::npos) return 3;
    const size_t body_off = eol + 1;
    const uint8_t delim = text.substr(0, eol).find(';') != std::string::npos ? ';' : ',';
    std::vector<uint8_t> body(text.begin() + body_off, text.end());
    const sg::MstCsvHost csv = sg::mst_csv_host(body.data(), body.size(), delim, nc);
    std::printf("body %zu %u %u %u\n", body_off, delim, sg::MST_SORT_TILE, sg::MST_SORT_NAME_CAP);
    geom(csv.n_rows);
    if (csv.flags || !csv.n_rows) {
      std::printf("sort %llu %x 0 0 0 0\nend\n", (unsigned long long)csv.n_rows, csv.flags);
      continue;
    }
    const sg::MstSortHost r = sg::mst_sort_host(body.data(), csv, nc);
    std::printf("sort %llu %x %llu %u %u %u\n", (unsigned long long)csv.n_rows, csv.flags, (unsigned long long)(r.problem >> 8),
                (unsigned)(r.problem & 0xff), r.longest, r.passes_run);
    if (!r.problem) {
      std::printf("order");
      for (uint32_t row : r.order) std::printf(" %u", row);
      std::printf("\nspans");
      for (uint32_t at : r.name_spans) std::printf(" %u", at);
      std::printf("\nfind");
      const uint32_t n = (uint32_t)csv.n_rows;
      for (uint32_t i = 0; i < n; i++) {                     // leaf i's own name: the lowest leaf that holds it
        const uint32_t b = r.name_spans[2 * i], e = r.name_spans[2 * i + 1];
        std::vector<uint8_t> q(body.begin() + b, body.begin() + e);   // an exact-size copy again
        std::printf(" %u", sg::mst_find_name(body.data(), body.size(), r.name_spans.data(), n, q.data(), q.size()));
      }
      const std::vector<uint8_t> high(sg::MST_SORT_NAME_CAP + 1, 0x7f), low(1, 0x00);   // above every name of the subset, and below every non-empty one
      std::printf(" %u", sg::mst_find_name(body.data(), body.size(), r.name_spans.data(), n, high.data(), high.size()));
      std::printf(" %u\n", sg::mst_find_name(body.data(), body.size(), r.name_spans.data(), n, low.data(), low.size()));
    }
    std::printf("end\n");
  }
  return 0;
}
