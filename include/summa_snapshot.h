/* summa_snapshot.h -- C ABI of a snapshot sorted and looked up by username on the device, of the names' order beside a tree in
 * file order with the report of the usernames that occur more than once, and of the range audit of a built tree, exported by
 * the same shared library as include/summa_gpu.h.
 *
 * The reference's sorted constructor (zk_prover/src/merkle_sum_tree/mst.rs:89-100) orders its leaves by the usernames' bytes so
 * that index_of_username is a binary search (mst.rs:207-223).  sg_mst_csv_scan_dev / sg_mst_csv_entries_dev (summa_gpu.h) read a
 * snapshot CSV where its text lies, in file order; the two calls below do the same with the leaves in sorted order and answer
 * "which leaf is this user's" from the text, so that a sorted snapshot is built, looked up by name and updated by name without
 * the host reading a row.
 *
 * Order: names compare byte by byte, a proper prefix first; equal names keep file order (a stable sort, as Rust's sort_by and
 * Python's list.sort).  The device sorts names of at most name_cap = 64 bytes (a UUID has 36, a hex SHA-256 64): a longer one
 * is REPORTED as row problem SS_MST_CSV_ROW_NAME_TOO_LONG, behind the six of summa_gpu.h, so that the caller can hand such a
 * file to a host sort; the lookup takes queries of any length.
 *
 * Names beside a tree in file order: sg_mst_csv_entries_dev builds its leaves in file order, the reference's from_csv
 * (mst.rs:74-87) and the only order whose root equals a commitment made from the same file.  The sort moves row indices alone,
 * so ss_mst_csv_name_index_dev gives such a tree the sorted order of its names without touching a leaf, and ss_mst_find_leaves
 * answers "which leaf is this user's" through it: a name that occurs several times yields its first row in file order, the
 * reference's position() (mst.rs:207-223), because the sort is stable and the search a lower bound.  The reference accepts a file
 * with a username twice silently (mst.rs:103-134), and every later row of that name is a leaf no lookup can reach while its
 * balances sit in the committed sums: ss_mst_duplicate_names_dev reports those rows, for either kind of tree.
 *
 * Audit: the reference builds its tree from any balances (mst.rs:103-134 checks no range); the inclusion circuit range-checks,
 * against 2^(8 n_bytes), the user's own leaf balances, the sibling leaf's and the sibling middle node's at every level above
 * (circuits/merkle_sum_tree.rs:348-369, 424-438).  ss_mst_range_audit_dev answers, from the node balances where they lie, which
 * nodes hold such a balance and which users' circuits fail for it, before a proof is spent on finding out.
 *
 * Conventions as in summa_gpu.h: 0 or a negative sg_status; sg_last_error() (thread-local) explains a failure; `stream` is the
 * caller's hipStream_t (NULL: the default stream), and device work is ordered on it. */
#ifndef SUMMA_SNAPSHOT_H
#define SUMMA_SNAPSHOT_H

#include <stddef.h>
#include <stdint.h>

#include "summa_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SS_MST_CSV_ROW_NAME_TOO_LONG 7 /* a username of more than name_cap bytes */
#define SS_MST_FIND_ABSENT 0xFFFFFFFFu

/* ss_mst_sort_geometry: name_cap, the longest name the device sorts (64), and tile_rows, the rows a workgroup ranks in one pass
 * of the sort (2048).  Either pointer may be NULL.
 * ss_mst_sort_scratch: *bytes_out = the size of d_sort_scratch for n_rows rows.  SG_ERR_INVALID: a null pointer, n_rows == 0 or
 * n_rows >= 2^32.  Neither touches a device. */
void ss_mst_sort_geometry(uint32_t* name_cap, uint32_t* tile_rows);
int ss_mst_sort_scratch(uint64_t n_rows, uint64_t* bytes_out);

/* sg_mst_csv_entries_dev with the leaves in sorted order: after sg_mst_csv_scan_dev without flags and with its n_rows >= 1, with
 * the d_tile_scratch it filled.  DEVICE inputs and the preconditions on the text are that call's (summa_gpu.h).
 *   d_span_scratch  16 * (n_rows + 1 + 2 * n_rows * (1 + n_currencies)) bytes, 8-byte aligned: the spans in file order, then in
 *                   leaf order (twice what sg_mst_csv_entries_dev asks for its one block; the contents are the library's own)
 *   d_sort_scratch  ss_mst_sort_scratch(n_rows) bytes, 16-byte aligned (the contents are the library's own)
 * It finds every row's fields and the longest name, waits for the stream (one 16-byte copy) and sets *problem_out: 0, or
 * row << 8 | code of the lowest row outside what the device takes, SG_MST_CSV_ROW_* or SS_MST_CSV_ROW_NAME_TOO_LONG (of several
 * problems in that row the lowest code), and then writes nothing more.  With *problem_out == 0 it launches as many passes of the
 * sort as the longest name has bytes, and three outputs are filled in stream order:
 *   d_order       n_rows x uint32, 4-byte aligned: the file row (from 0 behind the header) of leaf i
 *   d_name_spans  n_rows x 2 x uint32, 4-byte aligned: begin and end of leaf i's name as offsets into the body (under 4 GiB)
 *   d_usernames (rows x 32 B), d_balances (rows x n_currencies x 32 B): exactly what sg_mst_entries_dev fills from the same
 *                 entries sorted stably by the names' bytes; rows >= n_rows, rows n_rows.. are zeroed
 * SG_ERR_INVALID, before the device is touched: what sg_mst_csv_entries_dev refuses, and a null or misaligned d_sort_scratch,
 * d_order or d_name_spans. */
int ss_mst_csv_entries_sorted_dev(const void* d_bytes, uint64_t len, uint64_t body_off, const void* d_tile_scratch, uint32_t delimiter,
                                  uint32_t n_currencies, uint64_t n_rows, uint64_t rows, void* d_span_scratch, void* d_sort_scratch,
                                  void* d_order, void* d_name_spans, void* d_usernames, void* d_balances, uint64_t* problem_out,
                                  void* stream);

/* index_of_username for m names at once, over the text and the d_name_spans of ss_mst_csv_entries_sorted_dev (DEVICE: d_bytes,
 * len, body_off, d_name_spans and n_rows as given to it and filled by it).  HOST inputs, laid out as the names of
 * sg_mst_entries_dev: query j is name_bytes[name_off[j] .. name_off[j+1]), name_off: m + 1 x uint64, name_off[0] = 0; any
 * length, 0 included -- a query longer than name_cap is simply not found.  HOST output: index_out[j] = the lowest leaf whose
 * name equals query j, or SS_MST_FIND_ABSENT (one thread per query: a lower-bound binary search that compares bytes in the
 * text).  The text and the spans are read in stream order -- the call sees work enqueued earlier on `stream` -- and the call
 * waits for the stream before it returns; the host buffers have been read by then.
 * SG_ERR_INVALID, before the device is touched: a null pointer; m == 0; n_rows == 0 or >= 2^32; body_off > len or a body of 2^32
 * bytes or more; a misaligned d_name_spans; offsets that do not start at 0 or that decrease. */
int ss_mst_find_names(const void* d_bytes, uint64_t len, uint64_t body_off, const void* d_name_spans, uint64_t n_rows,
                      const uint8_t* name_bytes, const uint64_t* name_off, size_t m, uint32_t* index_out, void* stream);

/* The sorted order of the names WITHOUT leaves: ss_mst_csv_entries_sorted_dev up to the hashing.  Called after
 * sg_mst_csv_scan_dev as that call is, usually behind sg_mst_csv_entries_dev, whose tree in file order it leaves alone.  DEVICE
 * inputs, the preconditions on the text, d_tile_scratch and d_sort_scratch are the sorted call's;
 *   d_span_scratch  16 * (n_rows + 1 + 2 * n_rows * (1 + n_currencies)) bytes, 8-byte aligned, as the sorted call's (the contents
 *                   are the library's own: the rows are split again here, nothing depends on what another call left there)
 * It finds every row's fields and the longest name, waits for the stream (one 16-byte copy) and sets *problem_out as the sorted
 * call does, SS_MST_CSV_ROW_NAME_TOO_LONG included, and with a problem writes nothing more.  With *problem_out == 0 three outputs
 * are filled in stream order:
 *   d_order            n_rows x uint32, 4-byte aligned: the file row (from 0 behind the header) at sorted position i
 *   d_name_spans       n_rows x 2 x uint32, 4-byte aligned: begin and end of the name at sorted position i, offsets into the body
 *                      -- what ss_mst_find_names, ss_mst_find_leaves and ss_mst_duplicate_names_dev read
 *   d_leaf_name_spans  n_rows x 2 x uint32, 4-byte aligned: begin and end of the name of file row r, the leaf r of a tree in file
 *                      order (d_leaf_name_spans[2 d_order[i] ..] = d_name_spans[2 i ..])
 * SG_ERR_INVALID, before the device is touched and with *problem_out as it was: a null pointer; n_currencies 0 or above 64; a
 * delimiter the reader does not take; body_off >= len or a body of 2^32 bytes or more; n_rows == 0 or above the body's bytes; a
 * misaligned d_tile_scratch (4), d_span_scratch (8), d_sort_scratch (16), d_order, d_name_spans or d_leaf_name_spans (4). */
int ss_mst_csv_name_index_dev(const void* d_bytes, uint64_t len, uint64_t body_off, const void* d_tile_scratch, uint32_t delimiter,
                              uint32_t n_currencies, uint64_t n_rows, void* d_span_scratch, void* d_sort_scratch, void* d_order,
                              void* d_name_spans, void* d_leaf_name_spans, uint64_t* problem_out, void* stream);

/* ss_mst_find_names for a tree whose leaves are in file order: the same search over d_name_spans, and the position found goes
 * through d_order (DEVICE, n_rows x uint32, 4-byte aligned, as ss_mst_csv_name_index_dev filled it) in the same kernel:
 * index_out[j] = d_order[position], or SS_MST_FIND_ABSENT.  The sort is stable and the search a lower bound, so a name that
 * occurs several times yields its lowest file row: the reference's position(), the first match in file order (mst.rs:207-223).
 * Inputs, stream order, the wait and SG_ERR_INVALID as for ss_mst_find_names, and a null or misaligned d_order. */
int ss_mst_find_leaves(const void* d_bytes, uint64_t len, uint64_t body_off, const void* d_name_spans, const void* d_order, uint64_t n_rows,
                       const uint8_t* name_bytes, const uint64_t* name_off, size_t m, uint32_t* index_out, void* stream);

/* ss_mst_duplicate_names_scratch: *bytes_out = the size of d_scratch for n_rows rows, 4 * (4 + tiles + groups) with
 * tiles = ceil(n_rows / 64) and groups = ceil(tiles / 256).  SG_ERR_INVALID: a null pointer, n_rows == 0 or n_rows >= 2^32.
 * Touches no device. */
int ss_mst_duplicate_names_scratch(uint64_t n_rows, uint64_t* bytes_out);

/* The names that occur more than once, from the sorted order of the names.  DEVICE inputs, read only: the text (d_bytes, len,
 * body_off) and d_name_spans as ss_mst_csv_entries_sorted_dev or ss_mst_csv_name_index_dev filled them for n_rows rows, and
 * d_order, n_rows x uint32 of the index call -- or NULL: leaf i is sorted position i, a sorted tree.  Sorted position i >= 1 is
 * SHADOWED iff its name equals the name at position i - 1, equal length and equal bytes (every span is cut to the body, so
 * whatever the spans hold nothing outside the body is read): a lookup by name finds the first row of a run of equal names
 * and never the rows behind it, whose balances still sit in the tree's sums.  DEVICE outputs:
 *   d_shadowed  cap x uint32, 4-byte aligned, NULL iff cap == 0: the leaves at the shadowed positions in sorted-position order --
 *               by name, and within a name by file row --, the first cap of them (their places come from prefix sums over the
 *               data, never from the order in which workgroups finish); entries behind the listed ones stay unwritten
 *   d_first     cap x uint32, 4-byte aligned, NULL iff cap == 0: beside each listed leaf the leaf that a lookup of its name finds,
 *               the head of its run (found by the lower-bound search, never by walking the run: n_rows equal names are fine)
 *   d_scratch   ss_mst_duplicate_names_scratch(n_rows) bytes, 4-byte aligned (the contents are the library's own)
 * HOST output: summary_out[0] = the names that occur more than once (the shadowed positions whose predecessor is not shadowed);
 * [1] = the shadowed rows; [2] = the rows listed, min([1], cap).
 * The inputs are read in stream order -- the call sees work enqueued earlier on `stream` --, the device outputs are written in
 * stream order, and the call waits for the stream once (one 16-byte copy) before it returns with the summary.
 * SG_ERR_INVALID, before the device is touched and with summary_out as it was: a null d_bytes, d_name_spans, d_scratch or
 * summary_out; a null d_shadowed or d_first with cap != 0; n_rows == 0 or >= 2^32; body_off > len or a body of 2^32 bytes or
 * more; d_name_spans, d_order, d_shadowed, d_first or d_scratch not 4-byte aligned. */
int ss_mst_duplicate_names_dev(const void* d_bytes, uint64_t len, uint64_t body_off, const void* d_name_spans, const void* d_order,
                               uint64_t n_rows, void* d_shadowed, void* d_first, uint64_t cap, void* d_scratch, uint64_t* summary_out,
                               void* stream);

/* ss_mst_range_audit_scratch: *bytes_out = the size of d_scratch for a tree of 2^depth leaves, 4 * (4 + tiles + groups) with
 * tiles = ceil(2^depth / 64) and groups = ceil(tiles / 256).  SG_ERR_INVALID: a null pointer, depth > 30.  Touches no device. */
int ss_mst_range_audit_scratch(uint32_t depth, uint64_t* bytes_out);

/* The range audit of a built tree with top = 2^(8 n_bytes).  DEVICE input: d_node_balances, the level-major node balances of
 * sg_mst_build_dev (2^(depth + 1) - 1 nodes x n_currencies x 32 B, Montgomery words), read only.  DEVICE outputs:
 *   d_node_flags    2^(depth + 1) - 1 bytes, level-major as the nodes: 0 if every balance of the node is below top, else 1 + the
 *                   lowest currency whose balance is not
 *   d_leaf_reasons  2^depth x uint32, 4-byte aligned: bit 0 of leaf i's word iff its own flag is non-zero, bit l + 1 (0 <= l < depth)
 *                   iff the flag of node (i >> l) ^ 1 of level l is -- the range checks of leaf i's circuit in the order of
 *                   synthesize; 0: all of them pass.  The sums on the leaf's own path above it are not in the mask: the circuit does
 *                   not check them, so a user below an overflowing middle node whose siblings are all in range is provable
 *   d_bad_leaves    bad_cap x uint32, 4-byte aligned, NULL iff bad_cap == 0: the leaves with a non-zero word in increasing order,
 *                   the first bad_cap of them (their places come from prefix sums over the data, never from the order in which
 *                   workgroups finish); entries behind the listed ones stay unwritten
 *   d_scratch       ss_mst_range_audit_scratch(depth) bytes, 4-byte aligned (the contents are the library's own)
 * HOST output: summary_out[0] = the nodes with a non-zero flag, the root included; [1] = the leaves with a non-zero word;
 * [2] = the leaves listed, min([1], bad_cap); [3] = the root's flag byte (the circuit leaves the root's sums to verification).
 * d_node_balances is read in stream order -- the call sees work enqueued earlier on `stream` --, the device outputs are written
 * in stream order, and the call waits for the stream once (one 16-byte copy) before it returns with the summary.
 * SG_ERR_INVALID, before the device is touched and with summary_out as it was: a null pointer (d_bad_leaves: with bad_cap != 0);
 * depth > 30; n_currencies 0 or above 64; n_bytes 0 or above 31; d_leaf_reasons, d_bad_leaves or d_scratch not 4-byte aligned;
 * d_node_balances not 16-byte aligned. */
int ss_mst_range_audit_dev(const void* d_node_balances, uint32_t depth, uint32_t n_currencies, uint32_t n_bytes, void* d_node_flags,
                           void* d_leaf_reasons, void* d_bad_leaves, uint64_t bad_cap, void* d_scratch, uint64_t* summary_out,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif
