/* summa_admit.h -- C ABI of a round settled IN FULL on a Merkle sum tree that sits in HBM: behind the diff of include/summa_rounds.h
 * the new users of the next round's file are admitted into the tree's padding leaves, the name index is extended by them, the gone
 * users' balances are zeroed, and the changed, gone and admitted leaves are re-hashed in ONE run of the update's kernels.  Exported
 * by the same shared library as include/summa_gpu.h, include/summa_snapshot.h, include/summa_rounds.h and include/summa_export.h.
 *
 * The tree T is in FILE order with its name index in HBM, as ss_mst_csv_name_index_dev leaves it (summa_snapshot.h): n_tree named
 * leaves, its text, d_name_spans, d_order and d_leaf_name_spans.  2^depth - n_tree padding leaves lie behind the named ones.  The
 * file B and the arrays of the diff are as sr_mst_csv_diff_dev took and left them, with a cap that left the lists complete.
 *
 * ZERO.  Every GONE leaf of the list gets n_currencies zero balances.  Its username, its place and its entry in the name index
 * stay: a lookup still finds it, sx_mst_csv_write_dev writes it as name,0,0, and a later diff of the same file still calls it GONE.
 * UNREACHABLE leaves are not touched.  The liabilities leave the committed sums; the row stays until a rebuild drops it.
 * ADMIT.  The j-th NEW row of B in file order becomes leaf n_tree + j: its username is the row's name hashed as Entry::new hashes
 * it, its balances are the row's, folded where the text lies.  A name that occurs twice among the NEW rows gets two leaves, the
 * later one shadowed, exactly as the reader treats a file with a repeated name.  The empty name is admitted as the empty name.
 * Whatever the padding leaf held before is overwritten.
 * AFTERWARDS the tree's text is the old text followed by the admitted names, one after the other in leaf order, without separators
 * (names are only ever read through spans; old spans keep their values), and the index holds n_tree + n_new entries: the sorted
 * order is the stable order by the names' bytes over all named leaves, equal names in leaf order -- bit for bit what
 * ss_mst_csv_name_index_dev makes of a file that holds those names in leaf order.
 *
 * Every position comes from prefix sums and lower bounds over the data, never from an atomic or the order in which workgroups
 * finish.  The plan of the levels is made on the HOST from the lists of changed and gone leaves, 4 bytes a leaf; the admitted
 * leaves are a range; the balances never visit the host.
 *
 * Conventions as in summa_gpu.h: 0 or a negative sg_status; sg_last_error() (thread-local) explains a failure; `stream` is the
 * caller's hipStream_t (NULL: the default stream), and device work is ordered on it. */
#ifndef SUMMA_ADMIT_H
#define SUMMA_ADMIT_H

#include <stddef.h>
#include <stdint.h>

#include "summa_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sa_mst_admit_scratch: *bytes_out = the size of d_scratch for n_new rows to admit from a file of n_rows rows: the sort's work
 * space (ss_mst_sort_scratch), 16 bytes a row of order, spans and ranks, 8 bytes a new row, the tiles and groups of two scans and
 * a second block of spans, 8 * (n_rows + 1 + 2 * n_rows * (1 + n_currencies)).
 * SG_ERR_INVALID: a null pointer, n_rows == 0 or >= 2^32, n_currencies 0 or above 64, n_new == 0 or above n_rows.  Touches no device. */
int sa_mst_admit_scratch(uint64_t n_rows, uint32_t n_currencies, uint64_t n_new, uint64_t* bytes_out);

/* The measure, for n_new >= 1.  DEVICE inputs, read only, as the diff took and left them: d_bytes, len, body_off, d_span_scratch
 * (8-byte aligned), n_rows, n_currencies; d_row_state (n_rows bytes); d_new_rows (n_new x uint32, 4-byte aligned: ALL the NEW rows,
 * n_new = summary_out[0] = summary_out[6]).  n_tree and depth are the tree's.
 *   d_scratch   sa_mst_admit_scratch(n_rows, n_currencies, n_new) bytes, 16-byte aligned; it stays for sa_mst_settle_dev
 *               (otherwise the contents are the library's own)
 * It measures the names of all rows and the admitted names' places, waits for the stream ONCE (one 32-byte copy) and sets
 *   *problem_out     0, or row << 8 | 7 of the lowest row of B whose name has more than 64 bytes (such a row is NEW by the diff's
 *                    rule); with a problem nothing more is enqueued
 *   *name_bytes_out  the bytes the admitted names add to the tree's text
 * and, without a problem, enqueues the sort of B's names and the sorted list of the NEW rows and returns without another wait.
 * SG_ERR_INVALID, before the device is touched and with both outputs as they were: a null pointer; n_currencies 0 or above 64;
 * depth > 30; body_off >= len or a body of 2^32 bytes or more; n_rows == 0 or above the body's bytes; n_new == 0 or above n_rows;
 * n_tree == 0 or above 2^depth; n_tree + n_new above 2^depth (the depth has to grow: a rebuild is due); a misaligned pointer. */
int sa_mst_admit_measure_dev(const void* d_bytes, uint64_t len, uint64_t body_off, const void* d_span_scratch, uint64_t n_rows,
                             uint32_t n_currencies, const void* d_row_state, const void* d_new_rows, uint64_t n_new, uint64_t n_tree,
                             uint32_t depth, void* d_scratch, uint64_t* name_bytes_out, uint64_t* problem_out, void* stream);

/* The settle.  DEVICE inputs, read only: the file and d_span_scratch as above; of the diff d_owner (2^depth x uint32) and
 * d_leaf_state (2^depth bytes); d_changed and n_changed = summary_out[2]; d_gone and n_gone = summary_out[4] to zero the gone
 * leaves, or n_gone = 0 (d_gone may be NULL) to leave them; d_new_rows, n_new and d_scratch as the measure took and left them
 * without a problem, or n_new = 0 to admit nobody -- then d_new_rows, d_scratch, the tree's text and index and the four outputs
 * below may be NULL and are not touched.  The tree's text and index: d_tree_bytes, tree_len, tree_body_off, d_name_spans
 * (2 n_tree x uint32), d_order (n_tree x uint32), d_leaf_name_spans (2 n_tree x uint32), n_tree, depth.
 * DEVICE outputs for n_new >= 1, none of them overlapping an input:
 *   d_tree_bytes_out        tree_len + name_bytes bytes: the old text, then the admitted names; name_bytes as the measure set it
 *   d_name_spans_out        2 (n_tree + n_new) x uint32, 4-byte aligned
 *   d_order_out             n_tree + n_new x uint32, 4-byte aligned
 *   d_leaf_name_spans_out   2 (n_tree + n_new) x uint32, 4-byte aligned
 * The tree's four arrays as sg_mst_update_dev takes them (16-byte aligned), all written in place: d_usernames at the admitted
 * leaves, the other three at the union of the changed, gone and admitted leaves and above it.
 * The lists of changed and gone leaves are copied to the host in stream order (4 bytes a leaf, the call's only waits) for the plan
 * of the levels and checked there; everything else is enqueued on `stream` and the call returns without waiting.  Nothing to do
 * (no list has a leaf) launches nothing and succeeds.
 * SG_ERR_INVALID, before the device is touched: a null pointer that is needed; n_currencies 0 or above 64; depth > 30; body_off >=
 * len or a body of 2^32 bytes or more; n_rows == 0 or above the body's bytes; n_changed above n_rows or 2^depth; n_new above
 * n_rows; n_tree == 0 or above 2^depth; n_tree + n_new above 2^depth; n_changed + n_gone above n_tree; name_bytes above 64 n_new;
 * a tree body that would reach 2^32 bytes with the names appended; a misaligned pointer; d_leaf_balances overlapping
 * d_node_balances.  SG_ERR_INVALID with nothing written: a changed or a gone list that does not strictly increase, names a leaf at
 * or above n_tree, or shares a leaf with the other. */
int sa_mst_settle_dev(const void* d_bytes, uint64_t len, uint64_t body_off, const void* d_span_scratch, uint64_t n_rows, uint32_t n_currencies,
                      const void* d_owner, const void* d_leaf_state, const void* d_changed, uint64_t n_changed, const void* d_gone,
                      uint64_t n_gone, const void* d_new_rows, uint64_t n_new, const void* d_scratch, const void* d_tree_bytes,
                      uint64_t tree_len, uint64_t tree_body_off, const void* d_name_spans, const void* d_order, const void* d_leaf_name_spans,
                      uint64_t n_tree, uint32_t depth, void* d_tree_bytes_out, uint64_t name_bytes, void* d_name_spans_out, void* d_order_out,
                      void* d_leaf_name_spans_out, void* d_usernames, void* d_leaf_balances, void* d_node_hashes, void* d_node_balances,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif
