/* peahip_eval.h -- C ABI of the all-item evaluation with several held-out positives per user (libpeahip.so, gfx950), next to
 * include/peahip.h, whose conventions hold here too: every entry point returns PEA_OK or a negative PEA_ERR_* code (peahip.h)
 * with the text at pea_last_error(), pointers are device pointers, `stream` is a hipStream_t passed as void *.
 */
#ifndef PEAHIP_EVAL_H_
#define PEAHIP_EVAL_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * pea_rank_full_multi (csrc/topk.hip, the fc1 / fc2 scorer of pea_rank_full) and pea_dot_rank_full_multi (csrc/dot_score.hip,
 * the inner product of pea_dot_rank_full): pea_rank_full for users that hold any number of positives, in ONE catalogue scan.
 *   unids [U]; positives as a CSR: pos_rowptr int64 [U + 1] (pos_rowptr[0] = 0, ascending, pos_rowptr[U] = Q), pos_items
 *   int64 [Q], every row strictly ascending node ids, any length, 0 included; the catalogue is the node ids
 *   [item_lo, item_lo + n_items); excl_rowptr [U + 1] / excl_items as pea_rank_full takes them (rows strictly ascending), or
 *   both NULL.
 *   The negatives N_q of user q are the catalogue items that are neither in q's exclusion row nor in q's positive row.  A
 *   positive outside the catalogue or inside the exclusion row is still scored and ranked; exclusion entries outside the
 *   catalogue are ignored.  With s the scorer, for flat positive j of user q (the order of pos_items):
 *     above [Q] int32      number of n in N_q with s(q, n) > s(q, pos_items[j]), strictly
 *     below [Q] int32      number of n in N_q with s(q, n) < s(q, pos_items[j]), strictly
 *     pos_score [Q] float  s(q, pos_items[j])
 *     n_neg [U] int32      the size of N_q
 *   These are the integers of the single-positive entry point: pea_rank_full([u_q], [pos_items[j]], exclusion = the sorted
 *   union of q's exclusion row and q's positive row) gives rank == above[j], auc == (float)below[j] / (float)n_neg[q] and the
 *   same pos_score, because a pair's score has the same bits in every entry point of its scorer.
 *   (pea_dot_rank_full IS pea_dot_rank_full_multi with one positive per user: it runs the same launches without a row
 *   pointer.  pea_rank_full keeps a scan of its own.)
 * How: a user's positives are cut into chunks of 8 thresholds; one (user, chunk) row rides in the scan where one user rides
 *   in a top-K scan, and every catalogue score is compared against the row's thresholds; a user with P positives
 *   costs ceil(P / 8) passes of scoring work.  The rows of a call are bounded by U + Q / 8 from the arguments alone, which
 *   sizes the launch and the workspace; per item range partial counts are added in range order (no atomics on counts, no
 *   float atomics: bitwise reproducible).  The finish scores every excluded item and every in-catalogue positive of a user
 *   once and takes it out of all of the user's counters (an item that is both is taken out once).
 * The order inside the rows of pos_items and of the exclusion is a precondition and is not checked; a pos_rowptr that
 *   breaks its own is clamped to [0, Q] and reads nothing out of bounds.
 * A user id or positive id outside [0, num_nodes) reads nothing out of range, leaves unspecified numbers in that user's
 *   (that positive's) outputs, everyone else's are right, and the call returns PEA_ERR_RANGE after the stream
 *   synchronisation that reads the flag, as pea_rank_full.
 * R: a multiple of 4, <= 64; D: a multiple of 4 in 4..256; n_items < 2^31 - 1.  Argument errors (PEA_ERR_ARG; a catalogue
 *   outside [0, num_nodes): PEA_ERR_RANGE; a short workspace: PEA_ERR_NOMEM) return before anything is launched.  U == 0
 *   returns PEA_OK; Q == 0 writes n_neg only.  No pointer may be NULL but the two of the exclusion (hand a Q == 0 call any
 *   valid address for pos_items, above, below and pos_score).
 * workspace: pea_rank_multi_workspace_bytes(U, Q, n_items, R) / pea_dot_rank_multi_workspace_bytes(U, Q, n_items, D), functions
 *   of their arguments alone; 0 for arguments the call would refuse.
 * ---------------------------------------------------------------------------------------------- */
size_t pea_rank_multi_workspace_bytes(int64_t U, int64_t Q, int64_t n_items, int R);
size_t pea_dot_rank_multi_workspace_bytes(int64_t U, int64_t Q, int64_t n_items, int D);
int pea_rank_full_multi(int64_t U, int R, int64_t num_nodes, const float *repr, const int64_t *unids, const int64_t *pos_rowptr,
                        const int64_t *pos_items, int64_t Q, int64_t item_lo, int64_t n_items, const int64_t *excl_rowptr,
                        const int64_t *excl_items, const float *fc1_w, const float *fc1_b, const float *fc2_w,
                        const float *fc2_b, int32_t *above, int32_t *below, float *pos_score, int32_t *n_neg, void *workspace,
                        size_t workspace_bytes, void *stream);
int pea_dot_rank_full_multi(int64_t U, int D, int64_t num_nodes, const float *repr, const int64_t *unids,
                            const int64_t *pos_rowptr, const int64_t *pos_items, int64_t Q, int64_t item_lo, int64_t n_items,
                            const int64_t *excl_rowptr, const int64_t *excl_items, int32_t *above, int32_t *below,
                            float *pos_score, int32_t *n_neg, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PEAHIP_EVAL_H_ */
