// The host geometry of the polynomial helpers (csrc/poly_plan.h) run on the CPU.  Prints the constants on the first line; then
// reads one request per line from stdin (or takes them from the arguments, one request each) and prints what every rule returns:
//   size n m     the block counts, scan width, evaluation levels, batched-evaluation plan and work-space sizes of n elements
//                (m: polynomials of the batched evaluation, products of the grand products, divisions of the Kate batch)
//   prefix n c   the blocks of a prefix product of n elements that writes c outputs
//   lincomb m    the terms after which a linear combination of m terms reduces its lazy sum on the way
// "none": the helper refuses the size.  tests/test_poly_cases_cpu.py builds it with plain g++ and compares it with the restatement
// in tests/poly_cases.py.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "poly_plan.h"

using namespace sg;

static std::string blocks(uint32_t b) { return b == POLY_NO_PLAN ? "none" : std::to_string(b); }

static bool answer(const std::string& line) {
  std::istringstream in(line);
  std::string what;
  unsigned long long n = 0, m = 0;
  if (!(in >> what >> n)) return false;
  if (what == "lincomb") {
    std::string at;
    for (uint32_t j = 0; j < n; j += 2)
      if (lincomb_reduces_after(j)) at += (at.empty() ? "" : ",") + std::to_string(j + 1);
    std::printf("lincomb m=%llu mid=%s\n", n, at.empty() ? "-" : at.c_str());
    return true;
  }
  if (!(in >> m)) return false;
  if (what == "prefix") {
    std::printf("prefix n=%llu count_out=%llu blocks=%s\n", n, m, blocks(prefix_blocks(n, m)).c_str());
    return true;
  }
  if (what != "size") return false;
  const uint32_t kb = kate_blocks(n);
  std::string levels, launches;
  for (size_t cur = n; cur;) {   // the loop of poly_eval: a level per launch, until one workgroup is left
    levels += (levels.empty() ? "" : ",") + std::to_string(cur);
    const uint32_t b = eval_blocks(cur);
    if (b == 1) break;
    cur = b;
  }
  for (uint32_t first = 0; first < m; first += EVAL_BATCH_MAX) launches += (first ? "," : "") + std::to_string(eval_batch_count((uint32_t)m, first));
  const uint32_t bb = eval_batch_plan_blocks(n);
  std::printf("size n=%llu m=%llu prefix=%s prefix_rows=%s prefix_tmp=%zu grand=%s grand_mod=%zu grand_tmp=%zu kate=%s kate_scan=%s "
              "kate_tmp=%zu kate_batch_tmp=%zu kate_batch_powers=%zu eval_levels=%s eval_tmp=%zu batch_ch=%s batch_blocks=%s "
              "batch_partials=%zu batch_tmp=%zu batch_launches=%s\n",
              n, m, blocks(prefix_blocks(n, n + 1)).c_str(), blocks(prefix_blocks(n, n)).c_str(), prefix_product_tmp_elems(n + 1),
              blocks(grand_blocks(n)).c_str(), grand_products_mod_elems(n, (uint32_t)m), grand_products_tmp_elems(n, (uint32_t)m),
              blocks(kb).c_str(), kb == POLY_NO_PLAN || kb < 2 ? "-" : std::to_string(kate_scan_threads(kb)).c_str(), kate_tmp_elems(),
              kate_batch_tmp_elems(n, (uint32_t)m), kate_batch_powers_bytes((uint32_t)m), levels.empty() ? "-" : levels.c_str(),
              poly_eval_tmp_elems(n), bb == POLY_NO_PLAN ? "-" : std::to_string(eval_batch_ch(n)).c_str(), blocks(bb).c_str(),
              poly_eval_batch_blocks(n), eval_batch_tmp_elems(n), launches.empty() ? "-" : launches.c_str());
  return true;
}

int main(int argc, char** argv) {
  std::printf("PP_CH=%u PP_THREADS=%u PP_BLOCK=%u KD_CH=%u KD_THREADS=%u KD_BLOCK=%u BI_CH=%u EV_THREADS=%u EV_CH=%u EV_LOG=%u "
              "EVAL_BATCH_MAX=%u EVAL_BATCH_SMALL_MAX=%zu EVAL_BATCH_MAX_N=%zu POLY_SCAN_MAX=%u PREFIX_MAX_SPAN=%zu KATE_MAX_N=%zu "
              "KATE_BATCH_MAX=%u KATE_POWERS_BYTES=%zu GRAND_MAX=%u GRAND_MAX_K=%u LINCOMB_MAX=%u LINCOMB_LOW_MAX=%u LINCOMB_SETS_MAX=%u "
              "LINCOMB_SETS_POLYS=%u LINCOMB_SETS_LOW=%u\n",
              PP_CH, PP_THREADS, PP_BLOCK, KD_CH, KD_THREADS, KD_BLOCK, BI_CH, EV_THREADS, EV_CH, EV_LOG, EVAL_BATCH_MAX,
              EVAL_BATCH_SMALL_MAX, EVAL_BATCH_MAX_N, POLY_SCAN_MAX, PREFIX_MAX_SPAN, KATE_MAX_N, KATE_BATCH_MAX, KATE_POWERS_BYTES,
              GRAND_MAX, GRAND_MAX_K, LINCOMB_MAX, LINCOMB_LOW_MAX, LINCOMB_SETS_MAX, LINCOMB_SETS_POLYS, LINCOMB_SETS_LOW);
  std::string line;
  if (argc > 1) {
    for (int i = 1; i < argc; i++)
      if (!answer(argv[i])) return std::fprintf(stderr, "bad request: %s\n", argv[i]), 2;
    return 0;
  }
  while (std::getline(std::cin, line))
    if (!line.empty() && !answer(line)) return std::fprintf(stderr, "bad request: %s\n", line.c_str()), 2;
  return 0;
}
