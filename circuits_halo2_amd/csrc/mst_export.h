// A tree in HBM written back out as the snapshot CSV it now commits to (mst_export.cuh has the kernels, sx_mst_csv_measure_dev and
// sx_mst_csv_write_dev in abi_export.hip launch them): the inverse of the reader of mst_csv.h.  The names come from the text the
// tree keeps, through the span of every leaf's name; the balances from the leaves' field elements as they are now.
//
// The text, by definition (the header line is the host's):
//   body     one row per named leaf i in 0 .. n_rows - 1, in leaf order; padding leaves are not written
//   row      the name's bytes as they stand in the tree's text, then for each of the nc currencies the delimiter and the balance,
//            then '\n' -- the last row too, whatever the source file did, and "\r\n" comes out as "\n"
//   balance  the canonical integer in [0, r) of the leaf's field element in decimal: no leading zeros, "0" for zero.  So a source
//            007 comes out as 7, and a source integer >= r as its residue
//   name     the leaf's span cut to the body as mst_names_span cuts it, and to MST_EXPORT_NAME_CAP bytes behind its begin (no
//            index holds a longer name: mst_sort.h): whatever the spans hold, nothing outside the tree's text is read, and the
//            measured length is the cut one
// A row is at most 64 + 64 * (1 + 77) + 1 = 5057 bytes, so the sum of a tile's or a group's rows fits 32 bits; the body's length is
// formed in 64 bits, and row positions are 32 bits: a body of 2^32 bytes or more is measured and not written.
//
// Decimal digits: the eight Montgomery words leave Montgomery form by one field product (x 2^256 * 2^5 * 2^-261 = x, as the range
// audit's flags do it), the canonical integer is peeled into base-10^9 chunks by dividing its 32-bit words by the constant 10^9,
// the top chunk is printed without padding and every lower chunk as exactly nine digits.  A value whose words 2..7 are zero --
// every balance a circuit of n_bytes = 8 accepts -- takes a short path over one 64-bit integer.
//
// Steps, stream order the only barrier between them; the positions come from prefix sums over the data, never from the order in
// which workgroups finish (the geometry of mst_audit.h: MST_EXPORT_TILE rows a wave, MST_EXPORT_GROUP tile sums a workgroup):
//   measure   a row per thread: its length into row_off; the wave's sum is tile_sum[tile]
//   groups    mst_audit_groups_kernel as it stands: the exclusive prefix of the tile sums within a group in place, the total aside
//   offsets   a row per thread: row_off = the totals of the groups before + the tile's prefix + the lengths of the lanes below;
//             the first wave also leaves what the host reads, the sum of all group totals in 64 bits
//   write     every row's bytes at its position: a wave stages its tile's run of the output in LDS and stores it 16 bytes a lane;
//             every store is guarded by the body's length.  With positions the measure made, the rows cover the body exactly.
//             With others the bytes stay inside the buffer and are otherwise undefined
// Plain C++ below, so that the rules and the tile and group edges are tested without a GPU (tests/cpp/mst_export_check.cpp runs
// mst_export_host behind mst_csv_host and mst_sort_host).
#pragma once
#include <string>
#include <vector>

#include "mst_entries.h"   // bn254_f29.cuh, mst_decimal_words (the inverse, for the tests)
#include "mst_names.h"     // mst_names_span, the tile and group geometry

namespace sg {

static constexpr uint32_t MST_EXPORT_THREADS = MST_AUDIT_THREADS;
static constexpr uint32_t MST_EXPORT_TILE = MST_AUDIT_TILE;     // rows whose lengths add up to one word of the scan: a wave's
static constexpr uint32_t MST_EXPORT_GROUP = MST_AUDIT_GROUP;   // tile sums a workgroup of the groups step scans
static constexpr uint32_t MST_EXPORT_NAME_CAP = MST_SORT_NAME_CAP;
static constexpr uint32_t MST_EXPORT_MAX_DIGITS = 77;           // r has 77 digits
static constexpr uint32_t MST_EXPORT_CHUNKS = 9;                // base-10^9 chunks of a value below 2^256 < 10^81
static constexpr uint32_t MST_EXPORT_MAX_ROW = MST_EXPORT_NAME_CAP + MST_AUDIT_MAX_CURRENCIES * (1 + MST_EXPORT_MAX_DIGITS) + 1;
// the writer stages a tile's contiguous output in this many bytes of LDS a wave, up to 15 of them the slack in front of its first
// piece; a tile with more output (long names, many currencies) is written a row per thread
static constexpr uint32_t MST_EXPORT_STAGE = 8192;

// The work space in 32-bit words: what the host reads (the body's length, low and high word; two spares), the tiles' sums, the
// groups' totals.
static constexpr uint32_t MST_EXPORT_AT_TOTAL = 0, MST_EXPORT_FRONT_WORDS = 4;
SG_HD uint32_t mst_export_tiles(uint64_t n_rows) { return (uint32_t)((n_rows + MST_EXPORT_TILE - 1) / MST_EXPORT_TILE); }
SG_HD uint32_t mst_export_groups(uint64_t n_rows) { return (mst_export_tiles(n_rows) + MST_EXPORT_GROUP - 1) / MST_EXPORT_GROUP; }
SG_HD uint32_t mst_export_at_tiles() { return MST_EXPORT_FRONT_WORDS; }
SG_HD uint32_t mst_export_at_groups(uint64_t n_rows) { return mst_export_at_tiles() + mst_export_tiles(n_rows); }
// the size of d_scratch in bytes: 4 * (4 + tiles + groups), tiles = ceil(n_rows / 64), groups = ceil(tiles / 256); n_rows < 2^32
SG_HD uint64_t mst_export_scratch_bytes(uint64_t n_rows) { return 4ull * (mst_export_at_groups(n_rows) + mst_export_groups(n_rows)); }

// the eight Montgomery words of a field element -> the canonical integer in [0, r), eight little-endian words: one product
SG_HD void mst_export_canonical(const uint32_t mont[8], uint32_t w[8]) {
  f29 k = f29_zero();
  k.l[0] = 32;
  f29_to_words(f29_cond_sub_p<Fr29>(f29_mul<Fr29>(f29_from_words<0>(mont), k)), w);
}

// the base-10^9 chunks of the integer w, the least significant first; returns how many there are, 1 at least (zero is one chunk
// of 0).  chunk[k] for k at or above the count is 0.
struct MstExportChunks {
  uint32_t chunk[MST_EXPORT_CHUNKS];
};
SG_HD uint32_t mst_export_chunks(const uint32_t w[8], MstExportChunks* out) {
  constexpr uint32_t BASE = 1000000000u;
#pragma unroll
  for (uint32_t j = 0; j < MST_EXPORT_CHUNKS; j++) out->chunk[j] = 0;
  if ((w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) == 0) {        // below 2^64 < 10^27: three chunks at the most
    uint64_t v = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
    out->chunk[0] = (uint32_t)(v % BASE);
    v /= BASE;
    out->chunk[1] = (uint32_t)(v % BASE);
    out->chunk[2] = (uint32_t)(v / BASE);
    return out->chunk[2] ? 3u : out->chunk[1] ? 2u : 1u;
  }
  uint32_t q[8];
#pragma unroll
  for (uint32_t k = 0; k < 8; k++) q[k] = w[k];
  uint32_t count = 1;
  // peel j leaves a quotient below 2^256 / 10^(9 (j + 1)): the words that can still be non-zero before it are 8, 8, 7, 6, .. 1
#pragma unroll
  for (uint32_t j = 0; j < MST_EXPORT_CHUNKS; j++) {
    const uint32_t words = j < 2 ? 8u : 9u - j;
    uint64_t rem = 0;
#pragma unroll
    for (int k = 7; k >= 0; k--) {
      if ((uint32_t)k < words) {
        const uint64_t cur = (rem << 32) | q[k];               // rem < 10^9: below 2^62
        q[k] = (uint32_t)(cur / BASE);
        rem = cur % BASE;
      }
    }
    out->chunk[j] = (uint32_t)rem;
    if (rem) count = j + 1;
  }
  return count;
}
// the decimal digits of a chunk without padding: 1 for 0 .. 9, up to 9
SG_HD uint32_t mst_export_chunk_digits(uint32_t c) {
  uint32_t d = 1;
  if (c >= 10u) d = 2;
  if (c >= 100u) d = 3;
  if (c >= 1000u) d = 4;
  if (c >= 10000u) d = 5;
  if (c >= 100000u) d = 6;
  if (c >= 1000000u) d = 7;
  if (c >= 10000000u) d = 8;
  if (c >= 100000000u) d = 9;
  return d;
}
SG_HD uint32_t mst_export_top_chunk(const MstExportChunks& c, uint32_t count) {
  uint32_t top = 0;
#pragma unroll
  for (uint32_t j = 0; j < MST_EXPORT_CHUNKS; j++)
    if (j + 1 == count) top = c.chunk[j];
  return top;
}
// the digit count of the canonical integer w: 1 for zero, up to 77
SG_HD uint32_t mst_export_digit_count(const uint32_t w[8]) {
  MstExportChunks c;
  const uint32_t count = mst_export_chunks(w, &c);
  return 9 * (count - 1) + mst_export_chunk_digits(mst_export_top_chunk(c, count));
}
// a byte of the output at position `at` of `out`: every store is guarded by `limit`, the bytes `out` has
SG_HD void mst_export_put(uint8_t* out, uint64_t limit, uint64_t at, uint8_t byte) {
  if (at < limit) out[at] = byte;
}
// the decimal digits of the canonical integer w at out[at ..); returns how many (mst_export_digit_count of w)
SG_HD uint32_t mst_export_put_digits(const uint32_t w[8], uint8_t* out, uint64_t limit, uint64_t at) {
  MstExportChunks c;
  const uint32_t count = mst_export_chunks(w, &c);
  uint32_t top = mst_export_top_chunk(c, count);
  const uint32_t lead = mst_export_chunk_digits(top);
  for (uint32_t d = lead; d-- > 0;) {                          // the top chunk without padding
    mst_export_put(out, limit, at + d, (uint8_t)('0' + top % 10u));
    top /= 10u;
  }
  uint64_t p = at + lead;
#pragma unroll
  for (int j = (int)MST_EXPORT_CHUNKS - 2; j >= 0; j--) {      // every lower chunk as exactly nine digits
    if ((uint32_t)j + 1 < count) {
      uint32_t v = c.chunk[j];
#pragma unroll
      for (int d = 8; d >= 0; d--) {
        mst_export_put(out, limit, p + (uint32_t)d, (uint8_t)('0' + v % 10u));
        v /= 10u;
      }
      p += 9;
    }
  }
  return (uint32_t)(p - at);
}

// the name of leaf i: its span cut to the body and to MST_EXPORT_NAME_CAP bytes
SG_HD void mst_export_name(const uint32_t* leaf_name_spans, uint64_t body_len, uint32_t i, uint64_t* begin, uint64_t* end) {
  mst_names_span(leaf_name_spans, body_len, i, begin, end);
  if (*end - *begin > MST_EXPORT_NAME_CAP) *end = *begin + MST_EXPORT_NAME_CAP;
}
// the length of a row from its name's length and its balances' digit counts
SG_HD uint32_t mst_export_row_bytes(uint32_t name_len, uint32_t nc, uint32_t digits) { return name_len + nc + digits + 1; }
// the digits a balance given as Montgomery words takes
SG_HD uint32_t mst_export_balance_digits(const uint32_t mont[8]) {
  uint32_t w[8];
  mst_export_canonical(mont, w);
  return mst_export_digit_count(w);
}
// the delimiter and the balance at out[at ..); returns 1 + the digits
SG_HD uint32_t mst_export_put_balance(const uint32_t mont[8], uint8_t delim, uint8_t* out, uint64_t limit, uint64_t at) {
  uint32_t w[8];
  mst_export_canonical(mont, w);
  mst_export_put(out, limit, at, delim);
  return 1 + mst_export_put_digits(w, out, limit, at + 1);
}
// the name body[b .. e) at out[at ..); returns its length
SG_HD uint32_t mst_export_put_name(const uint8_t* body, uint64_t b, uint64_t e, uint8_t* out, uint64_t limit, uint64_t at) {
  for (uint64_t k = b; k < e; k++) mst_export_put(out, limit, at + (k - b), body[k]);
  return (uint32_t)(e - b);
}
// row i's length; leaf_bal: nc x 8 Montgomery words a leaf
inline uint32_t mst_export_measure_row(uint64_t body_len, const uint32_t* leaf_name_spans, uint32_t i, uint32_t nc, const uint32_t* leaf_bal) {
  uint64_t b, e;
  mst_export_name(leaf_name_spans, body_len, i, &b, &e);
  uint32_t digits = 0;
  for (uint32_t c = 0; c < nc; c++) digits += mst_export_balance_digits(leaf_bal + 8 * ((size_t)i * nc + c));
  return mst_export_row_bytes((uint32_t)(e - b), nc, digits);
}
// row i's bytes at out[at ..), every store guarded by limit; returns the row's length
inline uint32_t mst_export_put_row(const uint8_t* body, uint64_t body_len, const uint32_t* leaf_name_spans, uint32_t i, uint32_t nc,
                                   const uint32_t* leaf_bal, uint8_t delim, uint8_t* out, uint64_t limit, uint64_t at) {
  uint64_t b, e;
  mst_export_name(leaf_name_spans, body_len, i, &b, &e);
  uint64_t p = at + mst_export_put_name(body, b, e, out, limit, at);
  for (uint32_t c = 0; c < nc; c++) p += mst_export_put_balance(leaf_bal + 8 * ((size_t)i * nc + c), delim, out, limit, p);
  mst_export_put(out, limit, p++, (uint8_t)'\n');
  return (uint32_t)(p - at);
}

// the delimiter rule of the reader (mst_diff_problem's)
inline bool mst_export_delimiter_ok(uint32_t d) {
  return !(d >= 256 || d == '\n' || d == '\r' || (d >= '0' && d <= '9') || mst_csv_forbidden((uint8_t)d));
}
// What sx_mst_csv_measure_dev refuses before it touches a device: "" or what is wrong with the call.
inline std::string mst_export_measure_problem(const void* d_tree_bytes, uint64_t tree_len, uint64_t tree_body_off, const void* d_leaf_name_spans,
                                              uint64_t n_rows, uint32_t nc, const void* d_leaf_balances, const void* d_row_off,
                                              const void* d_scratch, const void* body_bytes_out) {
  if (!d_tree_bytes || !d_leaf_name_spans || !d_leaf_balances || !d_row_off || !d_scratch || !body_bytes_out) return "null argument";
  if (nc == 0 || nc > MST_AUDIT_MAX_CURRENCIES) return "n_currencies outside 1..64";
  if (n_rows == 0 || n_rows >= (1ull << 32)) return "n_rows outside 1..2^32-1";
  if (tree_body_off > tree_len || tree_len - tree_body_off >= (1ull << 32)) return "the tree's body_off behind len, or a body of 2^32 bytes or more";
  if ((uintptr_t)d_leaf_name_spans & 3) return "d_leaf_name_spans is not 4-byte aligned";
  if ((uintptr_t)d_leaf_balances & 15) return "d_leaf_balances is not 16-byte aligned";
  if ((uintptr_t)d_row_off & 3) return "d_row_off is not 4-byte aligned";
  if ((uintptr_t)d_scratch & 3) return "d_scratch is not 4-byte aligned";
  return "";
}
// What sx_mst_csv_write_dev refuses before it touches a device
inline std::string mst_export_write_problem(const void* d_tree_bytes, uint64_t tree_len, uint64_t tree_body_off, const void* d_leaf_name_spans,
                                            uint64_t n_rows, uint32_t nc, const void* d_leaf_balances, uint32_t delimiter, const void* d_row_off,
                                            uint64_t body_bytes, const void* d_out) {
  if (!d_tree_bytes || !d_leaf_name_spans || !d_leaf_balances || !d_row_off || !d_out) return "null argument";
  if (nc == 0 || nc > MST_AUDIT_MAX_CURRENCIES) return "n_currencies outside 1..64";
  if (n_rows == 0 || n_rows >= (1ull << 32)) return "n_rows outside 1..2^32-1";
  if (tree_body_off > tree_len || tree_len - tree_body_off >= (1ull << 32)) return "the tree's body_off behind len, or a body of 2^32 bytes or more";
  if (!mst_export_delimiter_ok(delimiter)) return "a delimiter the reader does not take";
  if (body_bytes == 0 || body_bytes >= (1ull << 32)) return "body_bytes outside 1..2^32-1";
  if ((uintptr_t)d_leaf_name_spans & 3) return "d_leaf_name_spans is not 4-byte aligned";
  if ((uintptr_t)d_leaf_balances & 15) return "d_leaf_balances is not 16-byte aligned";
  if ((uintptr_t)d_row_off & 3) return "d_row_off is not 4-byte aligned";
  return "";
}

// ------------------------------------------------------------------ the steps on the host, one after the other
struct MstExportHost {
  std::vector<uint32_t> row_off;    // n_rows: every row's start in the body (undefined when total >= 2^32)
  uint64_t total = 0;               // the body's length
  std::vector<uint8_t> out;         // the body, total bytes (empty when total >= 2^32)
};
// leaf_name_spans: begin and end of every leaf's name in `body`; leaf_bal: n_rows x nc x 8 Montgomery words.  Over the same tiles
// and groups as the kernels; the writer fills a buffer of exactly `total` bytes, behind its own guard.
inline MstExportHost mst_export_host(const uint8_t* body, uint64_t body_len, const uint32_t* leaf_name_spans, uint64_t n_rows, uint32_t nc,
                                     const uint32_t* leaf_bal, uint8_t delim) {
  MstExportHost r;
  const uint32_t n = (uint32_t)n_rows, tiles = mst_export_tiles(n_rows), groups = mst_export_groups(n_rows);
  std::vector<uint32_t> work(mst_export_scratch_bytes(n_rows) / 4, 0);
  uint32_t *tile_sum = work.data() + mst_export_at_tiles(), *group_total = work.data() + mst_export_at_groups(n_rows);
  r.row_off.assign(n, 0);
  for (uint32_t i = 0; i < n; i++) {                           // measure
    r.row_off[i] = mst_export_measure_row(body_len, leaf_name_spans, i, nc, leaf_bal);
    tile_sum[i / MST_EXPORT_TILE] += r.row_off[i];
  }
  for (uint32_t g = 0; g < groups; g++) {                      // groups: exclusive in place, the total aside
    uint32_t before = 0;
    for (uint32_t t = g * MST_EXPORT_GROUP; t < tiles && t < (g + 1) * MST_EXPORT_GROUP; t++) {
      const uint32_t sum = tile_sum[t];
      tile_sum[t] = before;
      before += sum;
    }
    group_total[g] = before;
  }
  uint32_t below = 0;                                          // offsets
  for (uint32_t i = 0; i < n; i++) {
    if (i % MST_EXPORT_TILE == 0) below = 0;
    const uint32_t tile = i / MST_EXPORT_TILE, group = tile / MST_EXPORT_GROUP, len = r.row_off[i];
    uint32_t before = 0;
    for (uint32_t g = 0; g < group; g++) before += group_total[g];
    r.row_off[i] = before + tile_sum[tile] + below;
    below += len;
  }
  for (uint32_t g = 0; g < groups; g++) r.total += group_total[g];
  if (r.total >= (1ull << 32)) return r;
  r.out.assign((size_t)r.total, 0);
  for (uint32_t i = 0; i < n; i++)                             // write
    mst_export_put_row(body, body_len, leaf_name_spans, i, nc, leaf_bal, delim, r.out.data(), r.total, r.row_off[i]);
  return r;
}

#if defined(__HIPCC__)
// measure, groups, offsets on `stream`: d_row_off[i] = row i's start, and the body's length as two words at
// d_work[MST_EXPORT_AT_TOTAL]; d_work: mst_export_scratch_bytes(n_rows)
hipError_t mst_export_measure_launch(const uint8_t* d_body, uint64_t body_len, const uint32_t* d_leaf_name_spans, uint64_t n_rows, uint32_t nc,
                                     const void* d_leaf_balances, uint32_t* d_row_off, uint32_t* d_work, hipStream_t stream);
// write on `stream`: exactly d_out[0 .. body_bytes), body_bytes < 2^32
hipError_t mst_export_write_launch(const uint8_t* d_body, uint64_t body_len, const uint32_t* d_leaf_name_spans, uint64_t n_rows, uint32_t nc,
                                   const void* d_leaf_balances, uint8_t delim, const uint32_t* d_row_off, uint64_t body_bytes, uint8_t* d_out,
                                   hipStream_t stream);
#endif

}  // namespace sg
