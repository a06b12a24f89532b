// The diff of a new round's file against a tree (csrc/mst_diff.h) on the host: the CSV reader's four passes over both files
// (mst_csv_host), the sort's steps over the tree's (mst_sort_host), then mst_diff_host over the tiles and groups the kernels take.
// tests/test_mst_diff_cpu.py feeds command lines on stdin:
//   geometry                        -> geometry THREADS TILE GROUP
//   scratch N_ROWS DEPTH            -> scratch BYTES LEAF_TILES LEAF_GROUPS ROW_TILES ROW_GROUPS
//   problem (27 integers, MstDiffArgs in the order of sr_mst_csv_diff_dev's arguments, pointers as integers)
//                                   -> problem WORDS...      (mst_diff_problem: nothing behind the word for a good call)
//   apply_problem (14 integers, in the order of sr_mst_apply_diff_dev's arguments)   -> apply_problem WORDS...
//   diff PATH_A PATH_B N_CURRENCIES SORTED(1|0) CAP...    (header line and delimiter as in mst_csv_check.cpp)
//     tree N_TREE DEPTH / file N_ROWS, or refused WHICH when the reader or the sort does not take a file
//     rowleaf, rowstate, leafstate, owner, changed, packed (8 words a field element)   -- of the first CAP's run
//     and per CAP: report CAP SUMMARY[8] STABLE(1: the arrays above came out the same) / new ROW ... / gone LEAF ...
//     end
#include <cstdio>
#include <fstream>
#include <iostream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "mst_diff.h"

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

static int diff(const std::string& path_a, const std::string& path_b, uint32_t nc, bool sorted_tree, const std::vector<uint64_t>& caps) {
  const Text ta = read(path_a), tb = read(path_b);
  if (!ta.ok || !tb.ok) return 2;
  const sg::MstCsvHost csv_a = sg::mst_csv_host(ta.body.data(), ta.body.size(), ta.delim, nc);
  const sg::MstCsvHost csv_b = sg::mst_csv_host(tb.body.data(), tb.body.size(), tb.delim, nc);
  if (csv_a.flags || !csv_a.n_rows || csv_a.problem) return std::printf("refused tree\nend\n"), 0;
  if (csv_b.flags || !csv_b.n_rows || csv_b.problem) return std::printf("refused file\nend\n"), 0;
  const sg::MstSortHost sorted = sg::mst_sort_host(ta.body.data(), csv_a, nc);
  if (sorted.problem) return std::printf("refused sort\nend\n"), 0;
  const uint32_t n_tree = (uint32_t)csv_a.n_rows;
  uint32_t depth = 0;
  while (((uint64_t)1 << depth) < n_tree) depth++;
  // the tree's leaf balances as the device holds them: the file's texts folded, in leaf order, zeros behind
  std::vector<uint64_t> words_a = csv_a.words;
  const sg::MstCsvSpans sa = sg::mst_csv_spans(words_a.data(), n_tree, nc);
  std::vector<uint32_t> leaf_bal((size_t)8 * nc << depth, 0);
  for (uint32_t leaf = 0; leaf < n_tree; leaf++) {
    const uint32_t row = sorted_tree ? sorted.order[leaf] : leaf;
    for (uint32_t c = 0; c < nc; c++) {
      const uint64_t at = (uint64_t)row * nc + c;
      sg::mst_decimal_words(ta.body.data() + sa.bal_begin[at], (size_t)(sa.bal_end[at] - sa.bal_begin[at]), leaf_bal.data() + 8 * ((size_t)leaf * nc + c));
    }
  }
  std::printf("tree %u %u\nfile %llu\n", n_tree, depth, (unsigned long long)csv_b.n_rows);
  sg::MstDiffHost head;
  for (size_t k = 0; k < caps.size(); k++) {
    const sg::MstDiffHost r =
        sg::mst_diff_host(tb.body.data(), tb.body.size(), csv_b.words.data(), csv_b.n_rows, nc, ta.body.data(), ta.body.size(),
                          sorted.name_spans.data(), sorted_tree ? nullptr : sorted.order.data(), n_tree, depth, leaf_bal.data(), caps[k]);
    if (k == 0) {
      head = r;
      list("rowleaf", r.row_leaf);
      list("rowstate", r.row_state);
      list("leafstate", r.leaf_state);
      list("owner", r.owner);
      list("changed", r.changed);
      list("packed", r.packed);
    }
    const bool stable = r.row_leaf == head.row_leaf && r.row_state == head.row_state && r.leaf_state == head.leaf_state && r.owner == head.owner &&
                        r.changed == head.changed && r.packed == head.packed;
    std::printf("report %llu", (unsigned long long)caps[k]);
    for (uint64_t x : r.summary) std::printf(" %llu", (unsigned long long)x);
    std::printf(" %d\n", stable ? 1 : 0);
    list("new", r.new_rows);
    list("gone", r.gone);
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
    auto p = [](uint64_t x) { return reinterpret_cast<const void*>((uintptr_t)x); };
    if (cmd == "geometry") {
      std::printf("geometry %u %u %u\n", sg::MST_DIFF_THREADS, sg::MST_DIFF_TILE, sg::MST_DIFF_GROUP);
    } else if (cmd == "scratch") {
      uint64_t n = 0;
      uint32_t depth = 0;
      in >> n >> depth;
      const uint64_t leaves = (uint64_t)1 << depth;
      std::printf("scratch %llu %u %u %u %u\n", (unsigned long long)sg::mst_diff_scratch_bytes(n, depth), sg::mst_diff_tiles(leaves),
                  sg::mst_diff_groups(leaves), sg::mst_diff_tiles(n), sg::mst_diff_groups(n));
    } else if (cmd == "problem") {
      uint64_t a[27] = {};
      for (uint64_t& x : a) in >> x;
      sg::MstDiffArgs g;
      g.b_bytes = p(a[0]), g.b_len = a[1], g.b_body_off = a[2], g.b_tiles = p(a[3]), g.delimiter = (uint32_t)a[4], g.nc = (uint32_t)a[5];
      g.n_rows = a[6], g.b_spans = p(a[7]), g.t_bytes = p(a[8]), g.t_len = a[9], g.t_body_off = a[10], g.t_name_spans = p(a[11]);
      g.t_order = p(a[12]), g.n_tree = a[13], g.depth = (uint32_t)a[14], g.leaf_balances = p(a[15]), g.row_leaf = p(a[16]);
      g.row_state = p(a[17]), g.leaf_state = p(a[18]), g.owner = p(a[19]), g.changed = p(a[20]), g.new_rows = p(a[21]), g.gone = p(a[22]);
      g.cap = a[23], g.scratch = p(a[24]), g.problem_out = p(a[25]), g.summary_out = p(a[26]);
      std::printf("problem %s\n", sg::mst_diff_problem(g).c_str());
    } else if (cmd == "apply_problem") {
      uint64_t a[14] = {};
      for (uint64_t& x : a) in >> x;
      std::printf("apply_problem %s\n", sg::mst_diff_apply_problem(p(a[0]), a[1], a[2], p(a[3]), a[4], p(a[5]), p(a[6]), a[7], (uint32_t)a[8],
                                                                   (uint32_t)a[9], p(a[10]), p(a[11]), p(a[12]), p(a[13]))
                                         .c_str());
    } else if (cmd == "diff") {
      std::string path_a, path_b;
      uint32_t nc = 0;
      int sorted_tree = 0;
      std::vector<uint64_t> caps;
      in >> path_a >> path_b >> nc >> sorted_tree;
      for (uint64_t cap; in >> cap;) caps.push_back(cap);
      if (const int rc = diff(path_a, path_b, nc, sorted_tree != 0, caps)) return rc;
    } else if (!cmd.empty()) {
      return 4;
    }
  }
  return 0;
}
