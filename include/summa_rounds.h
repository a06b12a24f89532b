/* summa_rounds.h -- C ABI of one round of a custodian's snapshots against the next: the new round's CSV joined by username with
 * a tree that sits in HBM, the report of who changed, who is new and who is gone, and the changed balances written into the tree
 * in place.  Exported by the same shared library as include/summa_gpu.h and include/summa_snapshot.h.
 *
 * The tree T has n_tree named leaves and the sorted order of their names in HBM, as ss_mst_csv_entries_sorted_dev (a sorted tree)
 * or ss_mst_csv_name_index_dev (a tree in file order) leave it (summa_snapshot.h).  The new file B is read where its text lies, as
 * sg_mst_csv_scan_dev / sg_mst_csv_entries_dev read a file (summa_gpu.h), with the same number of currencies.
 *
 * LOOKUP of a name in T is index_of_username: the first leaf of that name, the head of its run in the sorted order (mst.rs:207-223).
 * Every ROW r of B gets row_leaf[r], the lookup of its name or SR_MST_ABSENT, and one state:
 *   SR_MST_ROW_NEW       row_leaf[r] is SR_MST_ABSENT; a name of more than 64 bytes, or the empty name where T has none, is simply
 *                        not found
 *   SR_MST_ROW_SHADOWED  a lower row of B has the same row_leaf: the first row in file order wins; owner[leaf] is the minimum of the
 *                        rows that found the leaf
 *   SR_MST_ROW_CHANGED   the owner row, and at least one of its n_currencies balances differs from the leaf's
 *   SR_MST_ROW_SAME      the owner row, and all balances are equal
 * Balances compare AS FIELD ELEMENTS: the row's decimal text folded as the reader folds it (Fp::from_str_vartime) against the
 * Montgomery words of the leaf's balance.  So 007 equals 7, and an integer >= r equals its residue.
 * Every LEAF of T, all 2^depth of them, gets one state:
 *   SR_MST_LEAF_PADDING 0      no name, index >= n_tree
 *   SR_MST_LEAF_SAME 1         owned by a row, balances equal
 *   SR_MST_LEAF_CHANGED 2      owned by a row, a balance differs
 *   SR_MST_LEAF_GONE 3         a run's head that no row of B found
 *   SR_MST_LEAF_UNREACHABLE 4  a shadowed leaf of T (ss_mst_duplicate_names_dev): no lookup reaches it, so no row can own it; it is
 *                              neither changed nor gone
 * New users are NOT inserted and gone users are NOT zeroed by the apply: a leaf's username is fixed in a built tree.  The report is
 * what tells the caller that a rebuild is due.
 *
 * The plan of the apply -- which nodes of every level lie above a changed leaf -- is made on the HOST from the list of changed
 * leaves, 4 bytes a changed leaf; the balances never visit the host, neither as digits nor as field elements.
 *
 * Conventions as in summa_gpu.h: 0 or a negative sg_status; sg_last_error() (thread-local) explains a failure; `stream` is the
 * caller's hipStream_t (NULL: the default stream), and device work is ordered on it. */
#ifndef SUMMA_ROUNDS_H
#define SUMMA_ROUNDS_H

#include <stddef.h>
#include <stdint.h>

#include "summa_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SR_MST_ABSENT 0xFFFFFFFFu
#define SR_MST_LEAF_PADDING 0
#define SR_MST_LEAF_SAME 1
#define SR_MST_LEAF_CHANGED 2
#define SR_MST_LEAF_GONE 3
#define SR_MST_LEAF_UNREACHABLE 4
#define SR_MST_ROW_SAME 1
#define SR_MST_ROW_CHANGED 2
#define SR_MST_ROW_NEW 3
#define SR_MST_ROW_SHADOWED 4

/* sr_mst_diff_scratch: *bytes_out = the size of d_scratch for a file of n_rows rows against a tree of 2^depth leaves,
 * 4 * (8 + 2 * (leaf tiles + leaf groups) + row tiles + row groups) with tiles = ceil(items / 64) and groups = ceil(tiles / 256).
 * SG_ERR_INVALID: a null pointer, n_rows == 0 or >= 2^32, depth > 30.  Touches no device. */
int sr_mst_diff_scratch(uint64_t n_rows, uint32_t depth, uint64_t* bytes_out);

/* The diff.  DEVICE inputs, read only.  The new file: d_bytes, len, body_off, d_tile_scratch, delimiter, n_currencies and n_rows as
 * for sg_mst_csv_entries_dev, after sg_mst_csv_scan_dev without flags and with its n_rows >= 1;
 *   d_span_scratch  8 * (n_rows + 2 + 2 * n_rows * (1 + n_currencies)) bytes, 8-byte aligned: the rows are split here, and the
 *                   spans stay for sr_mst_apply_diff_dev (otherwise the contents are the library's own)
 * The tree: d_tree_bytes, tree_len, tree_body_off, d_name_spans and n_tree as the sorted or the index call of summa_snapshot.h took
 * and filled them; d_order of the index call, or NULL for a sorted tree (leaf i is sorted position i); depth; d_leaf_balances, the
 * tree's leaf balances (2^depth x n_currencies x 32 B, Montgomery words, 16-byte aligned).
 * It splits the file's rows, waits for the stream (one 8-byte copy) and sets *problem_out as sg_mst_csv_entries_dev does: 0, or
 * row << 8 | code of the lowest row outside what the device takes, and with a problem writes nothing more.  With *problem_out == 0
 * the DEVICE outputs are filled in stream order:
 *   d_row_leaf    n_rows x uint32, 4-byte aligned
 *   d_row_state   n_rows bytes, SR_MST_ROW_*
 *   d_leaf_state  2^depth bytes, SR_MST_LEAF_*
 *   d_owner       2^depth x uint32, 4-byte aligned: the lowest row that found the leaf, or SR_MST_ABSENT
 *   d_changed     min(n_rows, 2^depth) x uint32, 4-byte aligned: the CHANGED leaves in increasing order, all of them
 *   d_new_rows    cap x uint32, 4-byte aligned, NULL iff cap == 0: the NEW rows in increasing order, the first cap of them
 *   d_gone        cap x uint32, 4-byte aligned, NULL iff cap == 0: the GONE leaves in increasing order, the first cap of them
 *   d_scratch     sr_mst_diff_scratch(n_rows, depth) bytes, 4-byte aligned (the contents are the library's own)
 * Every list's places come from prefix sums over the data, never from the order in which workgroups finish; entries behind the
 * listed ones stay unwritten.  HOST output: summary_out[0..8) = the NEW, SHADOWED, CHANGED and SAME rows; the GONE and the
 * UNREACHABLE leaves; the new rows listed, min([0], cap); the gone leaves listed, min([4], cap).  The call waits for the stream once
 * more (one 32-byte copy) before it returns with the summary.
 * SG_ERR_INVALID, before the device is touched and with *problem_out and summary_out as they were: a null pointer (d_order may be
 * NULL; d_new_rows and d_gone with cap == 0); n_currencies 0 or above 64; depth > 30; a delimiter the reader does not take;
 * body_off >= len or a body of 2^32 bytes or more; n_rows == 0 or above the body's bytes; tree_body_off > tree_len or a tree body
 * of 2^32 bytes or more; n_tree == 0 or above 2^depth; a misaligned pointer. */
int sr_mst_csv_diff_dev(const void* d_bytes, uint64_t len, uint64_t body_off, const void* d_tile_scratch, uint32_t delimiter,
                        uint32_t n_currencies, uint64_t n_rows, void* d_span_scratch, const void* d_tree_bytes, uint64_t tree_len,
                        uint64_t tree_body_off, const void* d_name_spans, const void* d_order, uint64_t n_tree, uint32_t depth,
                        const void* d_leaf_balances, void* d_row_leaf, void* d_row_state, void* d_leaf_state, void* d_owner, void* d_changed,
                        void* d_new_rows, void* d_gone, uint64_t cap, void* d_scratch, uint64_t* problem_out, uint64_t* summary_out,
                        void* stream);

/* The apply: for the j-th of the n_changed leaves of d_changed the n_currencies balances of row d_owner[leaf] of the file are folded
 * once more where the text lies, and go through the listed leaf kernel and the listed level kernels exactly as sg_mst_update_dev
 * drives them.  DEVICE inputs as the diff took and left them: d_bytes, len, body_off, d_span_scratch, n_rows; d_owner; d_changed and
 * n_changed = summary_out[2].  The tree's four arrays as sg_mst_update_dev takes them, all written in place.  The list of changed
 * leaves is copied to the host in stream order (4 bytes a leaf, one wait) for the plan of the levels and checked there: leaf numbers
 * below 2^depth that strictly increase.  Everything else is enqueued on `stream`.  n_changed == 0 launches nothing and succeeds.
 * SG_ERR_INVALID, before the device is touched: a null pointer; n_currencies 0 or above 64; depth > 30; body_off >= len or a body of
 * 2^32 bytes or more; n_rows == 0 or above the body's bytes; n_changed above n_rows or 2^depth; a misaligned pointer;
 * d_leaf_balances overlapping d_node_balances.  SG_ERR_INVALID with nothing written: a list that is not as described. */
int sr_mst_apply_diff_dev(const void* d_bytes, uint64_t len, uint64_t body_off, const void* d_span_scratch, uint64_t n_rows,
                          const void* d_owner, const void* d_changed, uint64_t n_changed, uint32_t depth, uint32_t n_currencies,
                          const void* d_usernames, void* d_leaf_balances, void* d_node_hashes, void* d_node_balances, void* stream);

#ifdef __cplusplus
}
#endif
#endif
