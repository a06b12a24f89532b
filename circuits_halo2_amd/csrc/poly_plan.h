// What the polynomial helpers (poly.hip) decide on the host before they launch anything: chunk and workgroup sizes, block
// counts, the width of the Kate scan, the levels of either evaluation path, work-space sizes and what is refused.  Pure
// functions of the job's shape; the launch functions and the C ABI (abi_poly.hip) take their numbers from here.  Standard
// headers only: tests/cpp/poly_plan_check.cpp runs these rules without a GPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace sg {

static constexpr uint32_t POLY_NO_PLAN = 0xffffffffu;   // what a block count says of a size the helper refuses
static constexpr uint32_t POLY_SCAN_MAX = 1024;         // one workgroup scans the per-block values

// ---- eval_polynomial: 16 coefficients per thread in the batched path (32 workgroups per 2^17-term polynomial: the 40
// evaluations of a proof fill the chip); longer polynomials (> 2^24 terms, where two levels of 2^12 no longer reach) and the
// single-polynomial path take 32 per thread.
static constexpr uint32_t EV_THREADS = 256;
static constexpr uint32_t EV_CH = 32, EV_LOG = 13;   // the single-polynomial path (any length): log2(EV_CH * EV_THREADS)
static constexpr uint32_t EVAL_BATCH_MAX = 40;
static constexpr size_t EVAL_BATCH_SMALL_MAX = (size_t)1 << 24, EVAL_BATCH_MAX_N = (size_t)1 << 26;
// level sizes shrink by EV_CH * EV_THREADS per launch, until one workgroup is left
inline uint32_t eval_blocks(size_t m) { return (uint32_t)((m + (size_t)EV_CH * EV_THREADS - 1) / ((size_t)EV_CH * EV_THREADS)); }
inline size_t poly_eval_tmp_elems(size_t n) { return (n + (size_t)EV_CH * EV_THREADS - 1) / ((size_t)EV_CH * EV_THREADS) + 1; }
inline uint32_t eval_batch_ch(size_t n) { return n <= EVAL_BATCH_SMALL_MAX ? 16 : 32; }   // coefficients per thread
inline size_t poly_eval_batch_blocks(size_t n) {   // partials per polynomial (what d_partial holds m times)
  const size_t per = (size_t)eval_batch_ch(n) * EV_THREADS;
  return (n + per - 1) / per;
}
// two launches: the second level is one workgroup, so it folds at most ch * EV_THREADS partials (n <= 2^26)
inline uint32_t eval_batch_plan_blocks(size_t n) {
  const size_t blocks = poly_eval_batch_blocks(n);
  if (n == 0 || blocks > eval_batch_ch(n) * EV_THREADS) return POLY_NO_PLAN;
  return (uint32_t)blocks;
}
inline size_t eval_batch_tmp_elems(size_t n) { return EVAL_BATCH_MAX * (poly_eval_batch_blocks(n) + 1); }
// more than EVAL_BATCH_MAX polynomials: the launch that starts at polynomial `first` of m takes this many
inline uint32_t eval_batch_count(uint32_t m, uint32_t first) { return std::min<uint32_t>(EVAL_BATCH_MAX, m - first); }
static_assert((size_t)32 * EV_THREADS * 32 * EV_THREADS == EVAL_BATCH_MAX_N && (1u << EV_LOG) == EV_CH * EV_THREADS, "");

// ---- batch inversion
static constexpr uint32_t BI_CH = 8;

// ---- exclusive prefix product, grand products: per-block products, scan of the block products (one workgroup), final pass
static constexpr uint32_t PP_CH = 8, PP_THREADS = 256, PP_BLOCK = PP_CH * PP_THREADS;
static constexpr size_t PREFIX_MAX_SPAN = (size_t)POLY_SCAN_MAX * PP_BLOCK;   // 2^21
static constexpr uint32_t GRAND_MAX = 8, GRAND_MAX_K = 21;
static_assert(((size_t)1 << GRAND_MAX_K) == PREFIX_MAX_SPAN, "");
// the blocks kernel covers a[0..n), the write kernel out[0..count_out): n + 1 outputs <= 2^21, or n <= 2^21 with count_out <= n
inline uint32_t prefix_blocks(size_t n, size_t count_out) {
  const size_t span = std::max(n, count_out);
  if (span > PREFIX_MAX_SPAN || count_out > n + 1) return POLY_NO_PLAN;
  return (uint32_t)((span + PP_BLOCK - 1) / PP_BLOCK);
}
inline size_t prefix_product_tmp_elems(size_t n) { return (n + PP_BLOCK - 1) / PP_BLOCK + 1; }
inline uint32_t grand_blocks(size_t n) {   // n rows are read and n written: z[0..n), n <= 2^21
  return n > PREFIX_MAX_SPAN ? POLY_NO_PLAN : (uint32_t)((n + PP_BLOCK - 1) / PP_BLOCK);
}
inline size_t grand_products_mod_elems(size_t n, uint32_t products) { return (size_t)products * n; }
inline size_t grand_products_tmp_elems(size_t n, uint32_t products) { return (size_t)products * ((n + 1 + PP_BLOCK - 1) / PP_BLOCK) + 1; }

// ---- Kate division: block values, scan of the block values (one workgroup, <= 1024 blocks), final pass with the carries
static constexpr uint32_t KD_CH = 8, KD_THREADS = 256, KD_BLOCK = KD_CH * KD_THREADS;
static constexpr size_t KATE_MAX_N = (size_t)POLY_SCAN_MAX * KD_BLOCK;   // 2^21
static constexpr uint32_t KATE_BATCH_MAX = 16;
static constexpr size_t KATE_POWERS_BYTES = (1 + 8 + 10) * 9 * sizeof(uint32_t);   // sizeof(KatePowers)
inline uint32_t kate_blocks(size_t n) { return n > KATE_MAX_N ? POLY_NO_PLAN : (uint32_t)((n + KD_BLOCK - 1) / KD_BLOCK); }
// the scan's workgroup: the power of two >= nblk, at least a wave (one block: no scan launch at all)
inline uint32_t kate_scan_threads(uint32_t nblk) {
  uint32_t scan_threads = 64;
  while (scan_threads < nblk) scan_threads <<= 1;
  return scan_threads;
}
inline size_t kate_tmp_elems() { return POLY_SCAN_MAX + 1; }
inline size_t kate_batch_powers_bytes(uint32_t m) { return (size_t)m * KATE_POWERS_BYTES; }
inline size_t kate_batch_tmp_elems(size_t n, uint32_t m) { return (size_t)m * ((n + KD_BLOCK - 1) / KD_BLOCK) + 1; }

// ---- lookup permutation for any table (poly_lookup_sort.cuh): LSD radix sort of both columns' 254-bit keys, LS_DIGIT_BITS per
// pass, a workgroup per LS_TILE keys in the histogram and scatter launches and in the two flag scans of the placement
static constexpr uint32_t LS_DIGIT_BITS = 8, LS_BINS = 1u << LS_DIGIT_BITS, LS_PASSES = 256 / LS_DIGIT_BITS;
static constexpr uint32_t LS_THREADS = 256, LS_ITEMS = 4, LS_TILE = LS_THREADS * LS_ITEMS;
static constexpr uint32_t LS_HEAD_WORDS = 64;   // per column the OR of all keys and the OR of their complements (8 + 8 words), then the verdict
static constexpr uint32_t LS_FLAG = 32;         // the verdict's word in the head
static constexpr size_t LS_MAX_ROWS = ((size_t)1 << 31) - 1;
inline size_t lookup_sort_tiles(size_t rows) { return (rows + LS_TILE - 1) / LS_TILE; }
// work space in u32 words: head | keys[column][ping-pong][rows][8] | hist[column][digit][tile] | used[rows] | repeat[rows] |
// rank[rows] | left[rows] | sums[2][tiles rounded up to 4] -- every part but repeat / rank / left starts on a 16-byte boundary
struct LookupSortLayout {
  size_t keys, hist, used, repeat, rank, left, sums, sums_stride, words;
};
inline LookupSortLayout lookup_sort_layout(size_t rows) {
  const size_t tiles = lookup_sort_tiles(rows);
  LookupSortLayout l;
  l.keys = LS_HEAD_WORDS;
  l.hist = l.keys + 4 * 8 * rows;
  l.used = l.hist + 2 * (size_t)LS_BINS * tiles;
  l.repeat = l.used + rows;
  l.rank = l.repeat + rows;
  l.left = l.rank + rows;
  l.sums = l.left + rows;
  l.sums_stride = (tiles + 3) & ~(size_t)3;
  l.words = l.sums + 2 * l.sums_stride;
  return l;
}
inline size_t lookup_sort_work_bytes(size_t rows) { return lookup_sort_layout(rows).words * sizeof(uint32_t); }
// launches of one call whatever the keys hold (a pass over a digit on which a column is constant returns at once): the head's
// memset, the keys, three per pass, then mark, tile sums, their scan, compaction, write
static constexpr uint32_t LS_LAUNCHES = 2 + 3 * LS_PASSES + 5;

// ---- linear combinations
static constexpr uint32_t LINCOMB_MAX = 32;
static constexpr uint32_t LINCOMB_LOW_MAX = 8;
static constexpr uint32_t LINCOMB_SETS_MAX = 8, LINCOMB_SETS_POLYS = 48, LINCOMB_SETS_LOW = 4;
// the lazy sum of the pairs of terms is reduced on the way after the pair that starts at term j (every sixteenth pair)
constexpr bool lincomb_reduces_after(uint32_t j) { return (j & 31) == 30; }

}  // namespace sg
