// Prints what csrc/poly_plan.h decides for the general lookup permutation (no HIP): the constants, then for every row count given
// as an argument its tiles, the word offset of every part of the work space and lookup_sort_work_bytes.
// tests/test_lookup_permute_cpu.py compares the lines with the rules restated in Python.
#include <cstdio>
#include <cstdlib>

#include "poly_plan.h"

int main(int argc, char** argv) {
  using namespace sg;
  std::printf("digit_bits=%u bins=%u passes=%u threads=%u items=%u tile=%u head=%u flag=%u launches=%u max_rows=%zu\n", LS_DIGIT_BITS, LS_BINS,
              LS_PASSES, LS_THREADS, LS_ITEMS, LS_TILE, LS_HEAD_WORDS, LS_FLAG, LS_LAUNCHES, LS_MAX_ROWS);
  for (int i = 1; i < argc; i++) {
    const size_t rows = std::strtoull(argv[i], nullptr, 10);
    const LookupSortLayout l = lookup_sort_layout(rows);
    std::printf("rows=%zu tiles=%zu keys=%zu hist=%zu used=%zu repeat=%zu rank=%zu left=%zu sums=%zu stride=%zu words=%zu bytes=%zu\n", rows,
                lookup_sort_tiles(rows), l.keys, l.hist, l.used, l.repeat, l.rank, l.left, l.sums, l.sums_stride, l.words,
                lookup_sort_work_bytes(rows));
  }
  return 0;
}
