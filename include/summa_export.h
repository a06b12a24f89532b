/* summa_export.h -- C ABI of a Merkle sum tree that sits in HBM written back out as the snapshot CSV it now commits to: the inverse
 * of the reader (sg_mst_csv_scan_dev / sg_mst_csv_entries_dev, summa_gpu.h).  The names come from the text the tree keeps in HBM,
 * the balances from the leaves' field elements as they are now -- after any sg_mst_update_dev or sr_mst_apply_diff_dev --, and
 * neither visits the host except as the finished bytes.  Exported by the same shared library as include/summa_gpu.h,
 * include/summa_snapshot.h and include/summa_rounds.h.
 *
 * The tree T has n_rows named leaves, the text they were read from and the span of every LEAF's name in it, as
 * ss_mst_csv_entries_sorted_dev (a sorted tree: d_name_spans is in leaf order) or ss_mst_csv_name_index_dev (a tree in file order:
 * d_leaf_name_spans) leave them (summa_snapshot.h).
 *
 * THE TEXT, by definition.  The header line is the caller's: `username`, then for every currency the delimiter and
 * balance_<name>_<chain>, then \n.  The BODY is one ROW per named leaf i in 0 .. n_rows - 1, in leaf order: a sorted tree is
 * written sorted, a tree in file order in file order; padding leaves are not written.
 *   row      the name's bytes exactly as they stand in the tree's text, then for each of the n_currencies balances the delimiter and
 *            the balance, then \n.  The last row ends in \n too, whatever the source file did, and a source \r\n comes out as \n.
 *   balance  the canonical integer in [0, r) of the leaf's field element, in decimal, with no leading zeros, and 0 for zero.  A
 *            source 007 comes out as 7, and a source integer >= r as its residue.
 *   name     the leaf's span is cut to the text's body, and to 64 bytes behind its begin (no index holds a longer name): whatever
 *            the spans hold, nothing outside the tree's text is read, and the measured length is the cut one.
 * A row is at most 64 + 64 * 78 + 1 bytes.  Duplicate names are written as they stand, every row of them.  So: a file the reader
 * takes comes back byte for byte when it is canonical (\n line ends, a final newline, no leading zeros, values below r) and the
 * tree is in file order and not updated; and the reader builds from any output a tree with the same root -- provided that no
 * padding leaf was given non-zero balances by leaf number, for such a leaf has no name and is not written.
 *
 * Row positions come from prefix sums over the data (a sum per 64 rows, a scan per 256 sums, the groups' totals), never from the
 * order in which workgroups finish: two runs give the same bytes.
 *
 * Conventions as in summa_gpu.h: 0 or a negative sg_status; sg_last_error() (thread-local) explains a failure; `stream` is the
 * caller's hipStream_t (NULL: the default stream), and device work is ordered on it. */
#ifndef SUMMA_EXPORT_H
#define SUMMA_EXPORT_H

#include <stddef.h>
#include <stdint.h>

#include "summa_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sx_mst_csv_scratch: *bytes_out = the size of d_scratch for n_rows rows, 4 * (4 + tiles + groups) with tiles = ceil(n_rows / 64)
 * and groups = ceil(tiles / 256).  SG_ERR_INVALID: a null pointer, n_rows == 0 or >= 2^32.  Touches no device. */
int sx_mst_csv_scratch(uint64_t n_rows, uint64_t* bytes_out);

/* The measure.  DEVICE inputs, read only:
 *   d_tree_bytes, tree_len, tree_body_off   the tree's text, as the call that built the tree took it
 *   d_leaf_name_spans  2 * n_rows x uint32, 4-byte aligned: begin and end of leaf i's name relative to the body
 *   n_rows, n_currencies
 *   d_leaf_balances    the tree's leaf balances (n_rows x n_currencies x 32 B at least, Montgomery words, 16-byte aligned)
 * DEVICE outputs, filled in stream order:
 *   d_row_off   n_rows x uint32, 4-byte aligned: every row's start in the body
 *   d_scratch   sx_mst_csv_scratch(n_rows) bytes, 4-byte aligned (the contents are the library's own)
 * HOST output: *body_bytes_out = the body's true length, formed in 64 bits.  The call waits for the stream once, for one 8-byte copy,
 * before it returns.  If the length is 2^32 or more, d_row_off is undefined and the caller must not write.
 * SG_ERR_INVALID, before the device is touched and with *body_bytes_out as it was: a null pointer; n_currencies 0 or above 64;
 * n_rows == 0 or >= 2^32; tree_body_off > tree_len or a text body of 2^32 bytes or more; a misaligned pointer. */
int sx_mst_csv_measure_dev(const void* d_tree_bytes, uint64_t tree_len, uint64_t tree_body_off, const void* d_leaf_name_spans, uint64_t n_rows,
                           uint32_t n_currencies, const void* d_leaf_balances, void* d_row_off, void* d_scratch, uint64_t* body_bytes_out,
                           void* stream);

/* The write.  The same DEVICE inputs, and: delimiter, one the reader takes (, or ; in practice); d_row_off and body_bytes as the
 * measure left them for the same inputs.  DEVICE output: d_out, body_bytes bytes, any alignment.  Exactly those bytes are written, in
 * stream order, nothing before or behind them -- every store is guarded by body_bytes, whatever d_row_off holds --, and the call
 * does not wait.
 * SG_ERR_INVALID, before the device is touched: a null pointer; n_currencies 0 or above 64; n_rows == 0 or >= 2^32; tree_body_off >
 * tree_len or a text body of 2^32 bytes or more; a delimiter the reader does not take; body_bytes == 0 or >= 2^32; a misaligned
 * pointer. */
int sx_mst_csv_write_dev(const void* d_tree_bytes, uint64_t tree_len, uint64_t tree_body_off, const void* d_leaf_name_spans, uint64_t n_rows,
                         uint32_t n_currencies, const void* d_leaf_balances, uint32_t delimiter, const void* d_row_off, uint64_t body_bytes,
                         void* d_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
