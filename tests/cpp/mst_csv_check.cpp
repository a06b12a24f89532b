// The CSV reader's four passes (csrc/mst_csv.h) on the host, one after the other over the tiles the kernels take: the text the
// kernels compile for the byte classes and the row splitter, the same tile edges.  tests/test_mst_csv_cpu.py writes files and
// feeds "PATH N_CURRENCIES" lines on stdin.  The header is line 1 up to its '\n'; the delimiter is ';' if line 1 holds one,
// else ','.  Answers, per file:
//   body OFFSET DELIMITER(decimal) TILE ROW_CAP
//   geom SCAN_BLOCK TILES SCAN_ROUNDS                     (pass 2's width, the body's tiles and the rounds of its scan)
//   scan N_ROWS FLAGS(hex) PROBLEM_ROW PROBLEM_CODE       (the problem 0 0 where there is none, or where passes 3-4 did not run)
//   span ROW NAME_BEGIN NAME_END BEGIN END ...            (one per row when nothing is wrong; offsets into the body)
//   end
// With arguments it reads no file: every argument is a body length, answered by its "geom" line alone.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>

#include "mst_csv.h"

static void geom(uint64_t body_len) {
  std::printf("geom %u %llu %llu\n", sg::MST_CSV_SCAN_BLOCK, (unsigned long long)sg::mst_csv_tiles(body_len),
              (unsigned long long)sg::mst_csv_scan_rounds(body_len));
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
    const sg::MstCsvHost r = sg::mst_csv_host(body.data(), body.size(), delim, nc);
    std::printf("body %zu %u %u %u\n", body_off, delim, sg::MST_CSV_TILE, sg::MST_CSV_ROW_CAP);
    geom(body.size());
    std::printf("scan %llu %x %llu %u\n", (unsigned long long)r.n_rows, r.flags, (unsigned long long)(r.problem >> 8),
                (unsigned)(r.problem & 0xff));
    if (!r.flags && !r.problem && r.n_rows) {
      std::vector<uint64_t> words = r.words;
      const sg::MstCsvSpans s = sg::mst_csv_spans(words.data(), r.n_rows, nc);
      for (uint64_t i = 0; i < r.n_rows; i++) {
        std::printf("span %llu %llu %llu", (unsigned long long)i, (unsigned long long)s.name_begin[i], (unsigned long long)s.name_end[i]);
        for (uint32_t c = 0; c < nc; c++)
          std::printf(" %llu %llu", (unsigned long long)s.bal_begin[i * nc + c], (unsigned long long)s.bal_end[i * nc + c]);
        std::printf("\n");
      }
    }
    std::printf("end\n");
  }
  return 0;
}
