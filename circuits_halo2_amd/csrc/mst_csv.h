// A snapshot CSV read on the device (mst_entries.hip has the kernels, sg_mst_csv_scan_dev / sg_mst_csv_entries_dev in abi_mst.hip
// launch them): from the body of the file -- everything behind the header line -- to one (begin, end) pair per username and per
// balance field, which mst_usernames_kernel and mst_balances_kernel then hash and fold where the text lies.
//
// The reader takes a strict subset of CSV text and says when a file is outside it; it never judges the data itself.  The caller
// gives such a file to its host parser, which accepts or refuses it as it always did.  Inside the subset a row is what lies
// between two '\n' (one '\r' in front of the '\n' stripped; a last row without '\n' counts, mst_csv_rows), has exactly nc delimiters, and
// every field behind the first is one or more of '0'..'9'.  Outside it: a byte '"', 0 or >= 0x80 (quoting, what Python's csv
// refuses, what decodes in more than one way), a '\r' that no '\n' follows (csv ends a line there), an empty row (csv skips
// it), another count of delimiters, an empty or non-decimal balance, a row of more than MST_CSV_ROW_CAP bytes.
//
// Four passes, stream order the only barrier between them, no workgroup waits for another:
//   1 classify + count   a tile of MST_CSV_TILE bytes per workgroup -> its number of '\n' | the two byte flags
//   2 scan               one workgroup: the tiles' words -> how many '\n' lie before each tile; the row count n and the flags
//   3 row starts         a tile again: row_start[newlines before it + rank in the tile + 1] = position + 1
//   4 split + validate   a row per thread: the spans of its fields, or (row, code) into the problem word, the lowest row winning
// Plain C++ below, so that the byte classes, the row splitter and the tile edges are tested without a GPU
// (tests/cpp/mst_csv_check.cpp runs mst_csv_host, the four passes one after the other over the same tiles).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#if !defined(SG_HD)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SG_HD __host__ __device__ __forceinline__
#else
#define SG_HD inline
#endif
#endif

namespace sg {

static constexpr uint32_t MST_CSV_TILE = 4096;       // bytes of a workgroup's tile: 256 lanes x 16 bytes
static constexpr uint32_t MST_CSV_ROW_CAP = 131072;  // csv.field_size_limit()'s default: a longer row may hold a longer field
// a tile's word: its '\n' count (at most MST_CSV_TILE) and two flags; the scan's flag word has the same two bits
static constexpr uint32_t MST_CSV_FLAG_BYTE = 1u << 30;     // a byte '"', 0x00 or >= 0x80
static constexpr uint32_t MST_CSV_FLAG_BARE_CR = 1u << 31;  // a '\r' not followed by '\n' (the body's last byte included)
static constexpr uint32_t MST_CSV_COUNT_MASK = MST_CSV_FLAG_BYTE - 1;
// what pass 4 finds in a row; where a row has several, the lowest code is its problem
enum : uint32_t {
  MST_CSV_OK = 0,
  MST_CSV_ROW_TOO_LONG = 1,   // more than MST_CSV_ROW_CAP bytes between two newlines
  MST_CSV_EMPTY_ROW = 2,
  MST_CSV_DELIMITERS = 3,     // not exactly nc delimiters: a field short or a field long
  MST_CSV_EMPTY_BALANCE = 4,
  MST_CSV_NOT_DECIMAL = 5,    // a balance byte outside '0'..'9'
  MST_CSV_ROW_START = 6,      // row starts that do not increase within the body: only a caller's wrong n_rows makes them
};
static constexpr uint64_t MST_CSV_NO_PROBLEM = ~0ull;   // the problem word before any row reported: every (row, code) is below
SG_HD uint64_t mst_csv_problem_word(uint64_t row, uint32_t code) { return row << 8 | code; }

SG_HD bool mst_csv_forbidden(uint8_t b) { return b == '"' || b == 0 || b >= 0x80; }
// body[p] is '\r': does anything but '\n' follow?  `next` is body[p + 1], read only when p + 1 < len.
SG_HD bool mst_csv_bare_cr(uint64_t p, uint64_t len, uint8_t next) { return p + 1 >= len || next != '\n'; }
// The rows of a body with `newlines` '\n': a last line without one counts, and a blank last line -- the body ends in two line
// ends, as tests/golden/entry_17.csv does -- is no row: csv yields nothing for it, and nothing can follow it.  (A blank line
// anywhere else stays a row, an empty one, which pass 4 reports.)
SG_HD uint64_t mst_csv_rows(const uint8_t* body, uint64_t len, uint64_t newlines) {
  if (len == 0) return 0;
  if (body[len - 1] != '\n') return newlines + 1;
  uint64_t e = len - 1;                                      // where the last line end starts
  if (e != 0 && body[e - 1] == '\r') e--;
  return e == 0 || body[e - 1] == '\n' ? newlines - 1 : newlines;
}
SG_HD uint64_t mst_csv_tiles(uint64_t body_len) { return (body_len + MST_CSV_TILE - 1) / MST_CSV_TILE; }
// pass 2 is one workgroup of MST_CSV_SCAN_BLOCK lanes, a tile's word per lane and round: its rounds over a body
static constexpr uint32_t MST_CSV_SCAN_BLOCK = 1024;
SG_HD uint64_t mst_csv_scan_rounds(uint64_t body_len) { return (mst_csv_tiles(body_len) + MST_CSV_SCAN_BLOCK - 1) / MST_CSV_SCAN_BLOCK; }
// the caller's work spaces: the tiles' words followed by the row count and the flags; row starts, then the spans (uint64 each)
SG_HD uint64_t mst_csv_tile_words(uint64_t body_len) { return mst_csv_tiles(body_len) + 2; }
SG_HD uint64_t mst_csv_span_words(uint64_t n_rows, uint32_t nc) { return n_rows + 1 + 2 * n_rows * (1 + (uint64_t)nc); }

// The spans of n rows of nc balances, each an offset into the body: name i is [name_begin[i], name_end[i]), balance field
// j = i * nc + c is [bal_begin[j], bal_end[j]).  One block of uint64 behind the n + 1 row starts.
struct MstCsvSpans {
  uint64_t *name_begin, *name_end, *bal_begin, *bal_end;
};
SG_HD MstCsvSpans mst_csv_spans(uint64_t* row_start, uint64_t n_rows, uint32_t nc) {
  uint64_t* p = row_start + n_rows + 1;
  return {p, p + n_rows, p + 2 * n_rows, p + 2 * n_rows + n_rows * nc};
}

// Pass 4 for row `row`, which is body[lo .. hi) without its '\n': strips one '\r', writes the row's spans and returns its
// problem code.  Spans are written for the fields found, at most 1 + nc of them; a row with a problem leaves some unwritten.
// At most MST_CSV_ROW_CAP + 1 bytes are read.
SG_HD uint32_t mst_csv_split_row(const uint8_t* body, uint64_t lo, uint64_t hi, uint8_t delim, uint32_t nc, uint64_t row,
                                 const MstCsvSpans& s) {
  if (hi > lo && body[hi - 1] == '\r') hi--;
  if (hi - lo > MST_CSV_ROW_CAP) return MST_CSV_ROW_TOO_LONG;
  if (hi == lo) return MST_CSV_EMPTY_ROW;
  uint32_t field = 0;            // 0 the name, 1 + c balance c
  uint64_t begin = lo;
  bool empty_balance = false, not_decimal = false;
  for (uint64_t p = lo; p <= hi; p++) {
    const bool at_end = p == hi;
    const uint8_t b = at_end ? delim : body[p];
    if (b == delim) {
      if (field == 0) {
        s.name_begin[row] = begin;
        s.name_end[row] = p;
      } else {
        s.bal_begin[row * nc + field - 1] = begin;
        s.bal_end[row * nc + field - 1] = p;
        if (p == begin) empty_balance = true;
      }
      if (at_end) break;
      if (field == nc) return MST_CSV_DELIMITERS;    // a field too many
      field++;
      begin = p + 1;
    } else if (field != 0 && (b < '0' || b > '9')) {
      not_decimal = true;
    }
  }
  if (field != nc) return MST_CSV_DELIMITERS;
  return empty_balance ? MST_CSV_EMPTY_BALANCE : not_decimal ? MST_CSV_NOT_DECIMAL : MST_CSV_OK;
}
// pass 4's bounds on a row before it is read: its start and the position of its newline, from two row starts
SG_HD bool mst_csv_row_bounds(const uint64_t* row_start, uint64_t row, uint64_t body_len, uint64_t* lo, uint64_t* hi) {
  *lo = row_start[row];
  *hi = row_start[row + 1] - 1;
  return *lo <= *hi && *hi <= body_len;   // (a row start of 0 makes hi 2^64 - 1)
}

// ------------------------------------------------------------------ the four passes on the host, tile by tile
struct MstCsvHost {
  uint64_t n_rows = 0;
  uint32_t flags = 0;
  uint64_t problem = 0;                 // 0, or mst_csv_problem_word of the lowest offending row
  std::vector<uint64_t> words;          // row starts and spans, laid out as on the device (mst_csv_span_words of them)
};
// pass 1 for one tile
inline uint32_t mst_csv_tile_word(const uint8_t* body, uint64_t body_len, uint64_t tile) {
  const uint64_t lo = tile * MST_CSV_TILE, hi = lo + MST_CSV_TILE < body_len ? lo + MST_CSV_TILE : body_len;
  uint32_t word = 0;
  for (uint64_t p = lo; p < hi; p++) {
    const uint8_t b = body[p];
    if (b == '\n') word++;
    if (mst_csv_forbidden(b)) word |= MST_CSV_FLAG_BYTE;
    if (b == '\r' && mst_csv_bare_cr(p, body_len, p + 1 < body_len ? body[p + 1] : 0)) word |= MST_CSV_FLAG_BARE_CR;   // one past the tile
  }
  return word;
}
// Passes 1 and 2, then -- as the caller of the two entry points does -- 3 and 4 only where no flag is up and there is a row.
inline MstCsvHost mst_csv_host(const uint8_t* body, uint64_t body_len, uint8_t delim, uint32_t nc) {
  MstCsvHost r;
  const uint64_t tiles = mst_csv_tiles(body_len);
  std::vector<uint32_t> tile(tiles + 2);
  for (uint64_t t = 0; t < tiles; t++) tile[t] = mst_csv_tile_word(body, body_len, t);
  uint64_t before = 0;
  for (uint64_t t = 0; t < tiles; t++) {           // pass 2: in place, as the kernel does
    r.flags |= tile[t] & ~MST_CSV_COUNT_MASK;
    const uint32_t count = tile[t] & MST_CSV_COUNT_MASK;
    tile[t] = (uint32_t)before;
    before += count;
  }
  const bool open_end = body_len != 0 && body[body_len - 1] != '\n';
  r.n_rows = mst_csv_rows(body, body_len, before);
  if (r.flags || r.n_rows == 0) return r;
  r.words.assign(mst_csv_span_words(r.n_rows, nc), ~0ull);
  uint64_t* row_start = r.words.data();
  row_start[0] = 0;                                 // pass 3
  if (open_end) row_start[r.n_rows] = body_len + 1;
  for (uint64_t t = 0; t < tiles; t++) {
    uint64_t rank = 0;
    const uint64_t lo = t * MST_CSV_TILE, hi = lo + MST_CSV_TILE < body_len ? lo + MST_CSV_TILE : body_len;
    for (uint64_t p = lo; p < hi; p++) {
      if (body[p] != '\n') continue;
      const uint64_t at = tile[t] + rank++ + 1;
      if (at <= r.n_rows) row_start[at] = p + 1;     // (the newline of a blank last line starts no row)
    }
  }
  const MstCsvSpans spans = mst_csv_spans(row_start, r.n_rows, nc);
  uint64_t problem = MST_CSV_NO_PROBLEM;
  for (uint64_t row = 0; row < r.n_rows; row++) {   // pass 4
    uint64_t lo, hi;
    const uint32_t code = mst_csv_row_bounds(row_start, row, body_len, &lo, &hi) ? mst_csv_split_row(body, lo, hi, delim, nc, row, spans)
                                                                                  : (uint32_t)MST_CSV_ROW_START;
    const uint64_t word = mst_csv_problem_word(row, code);
    if (code != MST_CSV_OK && word < problem) problem = word;
  }
  r.problem = problem == MST_CSV_NO_PROBLEM ? 0 : problem;
  return r;
}

#if defined(__HIPCC__)
// passes 1 and 2 over d_body[0 .. body_len): d_tiles (mst_csv_tile_words u32) ends in the row count and the flag word
hipError_t mst_csv_scan_launch(const uint8_t* d_body, uint64_t body_len, uint32_t* d_tiles, hipStream_t stream);
// passes 3 and 4: d_words (mst_csv_span_words u64) gets the row starts and the spans, *d_problem the problem word
hipError_t mst_csv_split_launch(const uint8_t* d_body, uint64_t body_len, const uint32_t* d_tiles, uint8_t delim, uint32_t nc,
                                uint64_t n_rows, uint64_t* d_words, uint64_t* d_problem, hipStream_t stream);
// mst_entries_launch over spans: names and digits both lie in d_body
hipError_t mst_csv_entries_launch(const uint8_t* d_body, const uint64_t* d_words, size_t n, size_t rows, uint32_t nc, void* d_users,
                                  void* d_balances, hipStream_t stream);
#endif

}  // namespace sg
