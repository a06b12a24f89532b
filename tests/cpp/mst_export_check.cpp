// A tree written back out as its snapshot CSV (csrc/mst_export.h) on the host: the CSV reader's four passes over the file
// (mst_csv_host), the sort's steps for a sorted tree (mst_sort_host), the balances folded as the device folds them, then
// mst_export_host over the tiles and groups the kernels take.  tests/test_mst_export_cpu.py feeds command lines on stdin:
//   geometry                  -> geometry THREADS TILE GROUP NAME_CAP MAX_ROW STAGE
//   scratch N_ROWS            -> scratch BYTES TILES GROUPS
//   measure_problem (10 integers, in the order of sx_mst_csv_measure_dev's arguments, pointers as integers)
//                             -> measure_problem WORDS...     (nothing behind the word for a good call)
//   write_problem (11 integers, in the order of sx_mst_csv_write_dev's arguments)   -> write_problem WORDS...
//   digits DECIMAL            -> digits TEXT COUNT BACK(1: mst_decimal_words of TEXT gives the Montgomery words of DECIMAL back)
//   export PATH N_CURRENCIES SORTED(1|0) DELIMITER(byte value) OUT_BODY OUT_OFFSETS
//                             -> export N_ROWS TOTAL, the body in OUT_BODY and n_rows x uint32 in OUT_OFFSETS,
//                                or refused WHICH when the reader or the sort does not take the file
//   clipped                   -> clipped TOTAL TEXT (| for a line feed): three rows whose spans reach behind the text, lie behind it
//                                and hold more than 64 bytes
#include <cstdio>
#include <fstream>
#include <iostream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "mst_export.h"

static int export_file(const std::string& path, uint32_t nc, bool sorted_tree, uint8_t out_delim, const std::string& out_body,
                       const std::string& out_offsets) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return 2;
  // an exact-size heap copy: a read past the body's end is the sanitizer's to find
  const std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  const size_t eol = text.find('\n');
  if (eol == std::string::npos) return 2;
  const uint8_t delim = text.substr(0, eol).find(';') != std::string::npos ? ';' : ',';
  const std::vector<uint8_t> body(text.begin() + eol + 1, text.end());
  const sg::MstCsvHost csv = sg::mst_csv_host(body.data(), body.size(), delim, nc);
  if (csv.flags || !csv.n_rows || csv.problem) return std::printf("refused file\n"), 0;
  const uint32_t n = (uint32_t)csv.n_rows;
  std::vector<uint64_t> words = csv.words;
  const sg::MstCsvSpans s = sg::mst_csv_spans(words.data(), n, nc);
  std::vector<uint32_t> order(n), spans(2 * (size_t)n);
  for (uint32_t i = 0; i < n; i++) {
    order[i] = i;
    spans[2 * (size_t)i] = (uint32_t)s.name_begin[i];
    spans[2 * (size_t)i + 1] = (uint32_t)s.name_end[i];
  }
  if (sorted_tree) {
    const sg::MstSortHost sorted = sg::mst_sort_host(body.data(), csv, nc);
    if (sorted.problem) return std::printf("refused sort\n"), 0;
    order = sorted.order;
    spans = sorted.name_spans;
  }
  // the leaves' balances as the device holds them: the file's texts folded, in leaf order
  std::vector<uint32_t> leaf_bal((size_t)8 * nc * n);
  for (uint32_t leaf = 0; leaf < n; leaf++)
    for (uint32_t c = 0; c < nc; c++) {
      const uint64_t at = (uint64_t)order[leaf] * nc + c;
      sg::mst_decimal_words(body.data() + s.bal_begin[at], (size_t)(s.bal_end[at] - s.bal_begin[at]), leaf_bal.data() + 8 * ((size_t)leaf * nc + c));
    }
  const sg::MstExportHost r = sg::mst_export_host(body.data(), body.size(), spans.data(), n, nc, leaf_bal.data(), out_delim);
  std::ofstream(out_body, std::ios::binary).write(reinterpret_cast<const char*>(r.out.data()), (std::streamsize)r.out.size());
  std::ofstream(out_offsets, std::ios::binary).write(reinterpret_cast<const char*>(r.row_off.data()), (std::streamsize)(4 * r.row_off.size()));
  std::printf("export %u %llu\n", n, (unsigned long long)r.total);
  return 0;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    auto p = [](uint64_t x) { return reinterpret_cast<const void*>((uintptr_t)x); };
    if (cmd == "geometry") {
      std::printf("geometry %u %u %u %u %u %u\n", sg::MST_EXPORT_THREADS, sg::MST_EXPORT_TILE, sg::MST_EXPORT_GROUP, sg::MST_EXPORT_NAME_CAP,
                  sg::MST_EXPORT_MAX_ROW, sg::MST_EXPORT_STAGE);
    } else if (cmd == "scratch") {
      uint64_t n = 0;
      in >> n;
      std::printf("scratch %llu %u %u\n", (unsigned long long)sg::mst_export_scratch_bytes(n), sg::mst_export_tiles(n), sg::mst_export_groups(n));
    } else if (cmd == "measure_problem") {
      uint64_t a[10] = {};
      for (uint64_t& x : a) in >> x;
      std::printf("measure_problem %s\n",
                  sg::mst_export_measure_problem(p(a[0]), a[1], a[2], p(a[3]), a[4], (uint32_t)a[5], p(a[6]), p(a[7]), p(a[8]), p(a[9])).c_str());
    } else if (cmd == "write_problem") {
      uint64_t a[11] = {};
      for (uint64_t& x : a) in >> x;
      std::printf("write_problem %s\n", sg::mst_export_write_problem(p(a[0]), a[1], a[2], p(a[3]), a[4], (uint32_t)a[5], p(a[6]), (uint32_t)a[7],
                                                                     p(a[8]), a[9], p(a[10]))
                                            .c_str());
    } else if (cmd == "digits") {
      std::string decimal;
      in >> decimal;
      uint32_t mont[8], w[8], back[8];
      sg::mst_decimal_words(reinterpret_cast<const uint8_t*>(decimal.data()), decimal.size(), mont);
      sg::mst_export_canonical(mont, w);
      std::vector<uint8_t> out(sg::mst_export_digit_count(w));      // exact size: a digit too many is the sanitizer's to find
      const uint32_t put = sg::mst_export_put_digits(w, out.data(), out.size(), 0);
      sg::mst_decimal_words(out.data(), out.size(), back);
      bool same = put == out.size() && put == sg::mst_export_balance_digits(mont);
      for (int k = 0; k < 8; k++) same = same && back[k] == mont[k];
      std::printf("digits %s %u %d\n", std::string(out.begin(), out.end()).c_str(), put, same ? 1 : 0);
    } else if (cmd == "export") {
      std::string path, out_body, out_offsets;
      uint32_t nc = 0, delim = 0;
      int sorted_tree = 0;
      in >> path >> nc >> sorted_tree >> delim >> out_body >> out_offsets;
      if (const int rc = export_file(path, nc, sorted_tree != 0, (uint8_t)delim, out_body, out_offsets)) return rc;
    } else if (cmd == "clipped") {
      // spans the reader did not make: behind the text, backwards, longer than the cap.  Nothing outside the text is read, and the
      // writer stays inside a buffer of the measured size.
      const std::string text = "abc," + std::string(80, 'z');
      const std::vector<uint8_t> body(text.begin(), text.end());
      const uint32_t spans[6] = {2, 1000, 90, 95, 4, 84};
      std::vector<uint32_t> bal(3 * 8, 0);
      const sg::MstExportHost r = sg::mst_export_host(body.data(), body.size(), spans, 3, 1, bal.data(), ',');
      std::string shown(r.out.begin(), r.out.end());
      for (char& ch : shown) ch = ch == '\n' ? '|' : ch;         // one line of output
      std::printf("clipped %llu %s\n", (unsigned long long)r.total, shown.c_str());
    } else if (!cmd.empty()) {
      return 4;
    }
  }
  return 0;
}
