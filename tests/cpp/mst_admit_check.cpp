// A round settled in full on a tree (csrc/mst_admit.h) on the host: the CSV reader's four passes over both files (mst_csv_host), the
// sort's steps over both (mst_sort_host), the diff (mst_diff_host), then mst_admit_host over the tiles and groups the kernels take.
// tests/test_mst_admit_cpu.py feeds command lines on stdin:
//   geometry                          -> geometry THREADS TILE GROUP NAME_CAP
//   scratch N_ROWS NC N_NEW           -> scratch BYTES AT_SORT AT_ORDER AT_SORTED_WORDS(in 32-bit words)
//   measure_problem (14 integers, in the order of sa_mst_admit_measure_dev's arguments, pointers as integers)  -> measure_problem WORDS...
//   settle_problem (32 integers, in the order of sa_mst_settle_dev's arguments)                                 -> settle_problem WORDS...
//   settle PATH_A PATH_B N_CURRENCIES ADMIT(1|0) ZERO(1|0) CAP     (header line and delimiter as in mst_csv_check.cpp)
//     tree N_TREE DEPTH / file N_ROWS, or refused WHICH when the reader or the sort does not take a file
//     then refused WORDS... | problem WORD | the result:
//     bytes NAME_BYTES / order LEAF... / sorted NAME... / leafnames NAME... (names in hex through the spans into the new text, - for the
//     empty name) / sortednew ROW... / union LEAF... / packed (8 words a field element)
//     end
#include <cstdio>
#include <fstream>
#include <iostream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "mst_admit.h"

template <class T>
static void list(const char* what, const std::vector<T>& v) {
  std::printf("%s", what);
  for (T x : v) std::printf(" %u", (unsigned)x);
  std::printf("\n");
}

struct Text {
  std::vector<uint8_t> body;
  uint8_t delim = ',';
  bool ok = false;
};
static Text read(const std::string& path) {
  Text t;
  std::ifstream f(path, std::ios::binary);
  if (!f) return t;
  // an exact-size heap copy: a read past the body's end is the sanitizer's to find
  const std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  const size_t eol = text.find('\n');
  if (eol == std::string::npos) return t;
  t.delim = text.substr(0, eol).find(';') != std::string::npos ? ';' : ',';
  t.body.assign(text.begin() + eol + 1, text.end());
  t.ok = true;
  return t;
}

// the names behind `spans` in `text`, every span cut to it as the kernels cut it
static void names(const char* what, const std::vector<uint8_t>& text, const std::vector<uint32_t>& spans) {
  std::printf("%s", what);
  for (size_t i = 0; 2 * i < spans.size(); i++) {
    uint64_t b, e;
    sg::mst_names_span(spans.data(), text.size(), (uint32_t)i, &b, &e);
    std::fputs(b == e ? " -" : " ", stdout);
    for (uint64_t k = b; k < e; k++) std::printf("%02x", text[k]);
  }
  std::printf("\n");
}

static int settle(const std::string& path_a, const std::string& path_b, uint32_t nc, bool admit, bool zero, uint64_t cap) {
  const Text ta = read(path_a), tb = read(path_b);
  if (!ta.ok || !tb.ok) return 2;
  const sg::MstCsvHost csv_a = sg::mst_csv_host(ta.body.data(), ta.body.size(), ta.delim, nc);
  const sg::MstCsvHost csv_b = sg::mst_csv_host(tb.body.data(), tb.body.size(), tb.delim, nc);
  if (csv_a.flags || !csv_a.n_rows || csv_a.problem) return std::printf("refused tree\nend\n"), 0;
  if (csv_b.flags || !csv_b.n_rows || csv_b.problem) return std::printf("refused file\nend\n"), 0;
  const sg::MstSortHost sorted_a = sg::mst_sort_host(ta.body.data(), csv_a, nc);
  if (sorted_a.problem) return std::printf("refused sort\nend\n"), 0;
  const sg::MstSortHost sorted_b = sg::mst_sort_host(tb.body.data(), csv_b, nc);
  const uint32_t n_tree = (uint32_t)csv_a.n_rows;
  uint32_t depth = 0;
  while (((uint64_t)1 << depth) < n_tree) depth++;
  // the tree in file order as the device holds it: the leaves' balances folded from the text, the names' spans in leaf order
  std::vector<uint64_t> words_a = csv_a.words;
  const sg::MstCsvSpans sa = sg::mst_csv_spans(words_a.data(), n_tree, nc);
  std::vector<uint32_t> leaf_bal((size_t)8 * nc << depth, 0), leaf_spans;
  for (uint32_t leaf = 0; leaf < n_tree; leaf++) {
    leaf_spans.push_back((uint32_t)sa.name_begin[leaf]);
    leaf_spans.push_back((uint32_t)sa.name_end[leaf]);
    for (uint32_t c = 0; c < nc; c++) {
      const uint64_t at = (uint64_t)leaf * nc + c;
      sg::mst_decimal_words(ta.body.data() + sa.bal_begin[at], (size_t)(sa.bal_end[at] - sa.bal_begin[at]), leaf_bal.data() + 8 * ((size_t)leaf * nc + c));
    }
  }
  std::printf("tree %u %u\nfile %llu\n", n_tree, depth, (unsigned long long)csv_b.n_rows);
  const sg::MstDiffHost diff = sg::mst_diff_host(tb.body.data(), tb.body.size(), csv_b.words.data(), csv_b.n_rows, nc, ta.body.data(),
                                                 ta.body.size(), sorted_a.name_spans.data(), sorted_a.order.data(), n_tree, depth,
                                                 leaf_bal.data(), cap);
  const sg::MstAdmitHost r = sg::mst_admit_host(tb.body.data(), tb.body.size(), csv_b.words.data(), csv_b.n_rows, nc, diff, sorted_b,
                                                ta.body.data(), ta.body.size(), sorted_a.name_spans.data(), sorted_a.order.data(),
                                                leaf_spans.data(), n_tree, depth, admit, zero);
  if (!r.refused.empty()) return std::printf("refused %s\nend\n", r.refused.c_str()), 0;
  if (r.problem) return std::printf("problem %llu\nend\n", (unsigned long long)r.problem), 0;
  std::printf("bytes %llu\n", (unsigned long long)r.name_bytes);
  list("order", r.order);
  names("sorted", r.text, r.name_spans);
  names("leafnames", r.text, r.leaf_name_spans);
  list("sortednew", r.sorted_new);
  list("union", r.leaves);
  list("packed", r.packed);
  std::printf("end\n");
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
      std::printf("geometry %u %u %u %u\n", sg::MST_ADMIT_THREADS, sg::MST_ADMIT_TILE, sg::MST_ADMIT_GROUP, sg::MST_ADMIT_NAME_CAP);
    } else if (cmd == "scratch") {
      uint64_t n = 0, m = 0;
      uint32_t nc = 0;
      in >> n >> nc >> m;
      std::printf("scratch %llu %llu %llu %llu\n", (unsigned long long)sg::mst_admit_scratch_bytes(n, nc, m),
                  (unsigned long long)sg::mst_admit_at_sort(), (unsigned long long)sg::mst_admit_at_order(n),
                  (unsigned long long)sg::mst_admit_at_sorted_words(n, m));
    } else if (cmd == "measure_problem") {
      uint64_t a[14] = {};
      for (uint64_t& x : a) in >> x;
      std::printf("measure_problem %s\n", sg::mst_admit_measure_problem(p(a[0]), a[1], a[2], p(a[3]), a[4], (uint32_t)a[5], p(a[6]), p(a[7]), a[8],
                                                                        a[9], (uint32_t)a[10], p(a[11]), p(a[12]), p(a[13]))
                                              .c_str());
    } else if (cmd == "settle_problem") {
      uint64_t a[32] = {};
      for (uint64_t& x : a) in >> x;
      sg::MstSettleArgs g;
      g.b_bytes = p(a[0]), g.b_len = a[1], g.b_body_off = a[2], g.b_spans = p(a[3]), g.n_rows = a[4], g.nc = (uint32_t)a[5], g.owner = p(a[6]);
      g.leaf_state = p(a[7]), g.changed = p(a[8]), g.n_changed = a[9], g.gone = p(a[10]), g.n_gone = a[11], g.new_rows = p(a[12]), g.n_new = a[13];
      g.scratch = p(a[14]), g.t_bytes = p(a[15]), g.t_len = a[16], g.t_body_off = a[17], g.t_name_spans = p(a[18]), g.t_order = p(a[19]);
      g.t_leaf_name_spans = p(a[20]), g.n_tree = a[21], g.depth = (uint32_t)a[22], g.out_bytes = p(a[23]), g.name_bytes = a[24];
      g.out_name_spans = p(a[25]), g.out_order = p(a[26]), g.out_leaf_name_spans = p(a[27]), g.usernames = p(a[28]), g.leaf_balances = p(a[29]);
      g.node_hashes = p(a[30]), g.node_balances = p(a[31]);
      std::printf("settle_problem %s\n", sg::mst_settle_problem(g).c_str());
    } else if (cmd == "settle") {
      std::string path_a, path_b;
      uint32_t nc = 0;
      int admit = 0, zero = 0;
      uint64_t cap = 0;
      in >> path_a >> path_b >> nc >> admit >> zero >> cap;
      if (const int rc = settle(path_a, path_b, nc, admit != 0, zero != 0, cap)) return rc;
    } else if (!cmd.empty()) {
      return 4;
    }
  }
  return 0;
}
