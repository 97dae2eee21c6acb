/* peahip_fm_eval.h -- C ABI of the full-catalogue evaluation of the factorisation-machine models of libpeahip.so (gfx950):
 * top-K recommendation, the all-item rank and the all-item rank with several positives per user, over the NFM fold, in
 * one pass over the catalogue (csrc/nfm_scan.hip); the [users, items] logit matrix is never written.  Next to
 * include/peahip_fm.h, whose conventions hold here too: every entry point returns PEA_OK or a negative PEA_ERR_* code
 * (peahip.h) with the text at pea_last_error(), pointers are device pointers, `stream` is a hipStream_t passed as void *,
 * nothing synchronises.
 *
 * The fold (E, H, num_users, num_items, emb, ld_emb, lin, w_fold, b_fold, w2, bias_fold) is passed as pea_nfm_score takes it
 * and a pair's logit has the bits pea_nfm_score gives it: both kernels call the tile body of csrc/nfm_tile.h.
 * Ids: uids [n_users] are LOCAL user ids in [0, num_users).  The catalogue is the LOCAL items [item_lo, item_lo + n_items),
 *   checked on the host against num_items (PEA_ERR_RANGE).  item_node0 is the node id of local item 0; excl_items, pos_items
 *   and out_items are NODE ids (item_node0 + local), so a model's exclusion lists go in as they are.
 *   excl_rowptr [n_users + 1] / excl_items: per requested user a strictly ascending row of items to leave out (entries outside
 *   the catalogue are ignored); both NULL for none.
 * A user id outside [0, num_users) sets *err_flag (an int32 the caller zeroed) to 1; nothing is read through it and its
 *   outputs are an all-(-1, -inf) list, or zero counters, a zero pos_score and n_neg 0.  A positive that is no item of the
 *   table sets the flag too and takes threshold 0.
 * Argument errors return PEA_ERR_ARG / PEA_ERR_RANGE (a short workspace PEA_ERR_NOMEM) before anything is launched; the
 *   scalars are checked before the pointers.  No float atomics; grids and splits are functions of the arguments alone;
 *   identical calls give identical bytes.
 *
 * pea_nfm_scan_supported(E, H, K): pure.  1 when the scan takes the widths and K (K = 0 asks for the rank forms, else K in
 *   1..128): what pea_nfm_supported takes, with the scan's LDS in a CU's 160 KB.
 * pea_nfm_scan_splits(n_users, n_items, K): pure.  The S item ranges a call cuts the catalogue into (K = 0: the rank forms);
 *   S K <= 2048, the entries the merge folds per user.  0 for arguments no call takes.
 * pea_nfm_scan_workspace_bytes(n_users, Q, n_excl, n_items, K, E, H): pure; 0 for a refused shape.  One size serves the
 *   three calls: pass K = 0 for the rank forms, Q = the positives (n_users for pea_nfm_rank_full, 0 for the top-K),
 *   n_excl = the exclusion entries.  Non-decreasing in every argument.
 * pea_nfm_recommend_topk: the contract of pea_dot_recommend_topk.  out_items / out_scores [n_users, K]: the K best eligible
 *   items in (logit descending, node id ascending) order, a (-1, -inf) tail where fewer are eligible.  K in 1..128.
 * pea_nfm_rank_full: the contract of pea_dot_rank_full.  pos_items [n_users]; over the catalogue items that are neither
 *   excluded nor the positive: rank = those whose logit is strictly higher than the positive's, auc = (float)(those strictly
 *   lower) / (float)(their number), 0 without any; pos_score = the positive's logit.  The positive may lie outside the
 *   catalogue.
 * pea_nfm_rank_full_multi: the contract of pea_dot_rank_full_multi (include/peahip_eval.h).  pos_rowptr [n_users + 1] /
 *   pos_items [Q], every row strictly ascending; in the flat order of pos_items above / below [Q] = the negatives (catalogue
 *   items in neither the user's exclusion row nor its positive row) scoring strictly higher / lower, pos_score [Q];
 *   n_neg [n_users] = the number of negatives.
 */
#ifndef PEAHIP_FM_EVAL_H_
#define PEAHIP_FM_EVAL_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PEA_NFM_SCAN_USERS 8 /* users of one workgroup: they share every staged tile of 64 item rows */
int pea_nfm_scan_supported(int E, int H, int K);
int pea_nfm_scan_splits(int64_t n_users, int64_t n_items, int K);
size_t pea_nfm_scan_workspace_bytes(int64_t n_users, int64_t Q, int64_t n_excl, int64_t n_items, int K, int E, int H);
int pea_nfm_recommend_topk(int E, int H, int64_t num_users, int64_t num_items, const float *emb, int64_t ld_emb, const float *lin,
                           const float *w_fold, const float *b_fold, const float *w2, const float *bias_fold, const int64_t *uids,
                           int64_t n_users, int K, int64_t item_lo, int64_t n_items, int64_t item_node0,
                           const int64_t *excl_rowptr, const int64_t *excl_items, int64_t *out_items, float *out_scores,
                           int *err_flag, void *workspace, size_t workspace_bytes, void *stream);
int pea_nfm_rank_full(int E, int H, int64_t num_users, int64_t num_items, const float *emb, int64_t ld_emb, const float *lin,
                      const float *w_fold, const float *b_fold, const float *w2, const float *bias_fold, const int64_t *uids,
                      int64_t n_users, const int64_t *pos_items, int64_t item_lo, int64_t n_items, int64_t item_node0,
                      const int64_t *excl_rowptr, const int64_t *excl_items, int32_t *rank, float *auc, float *pos_score,
                      int *err_flag, void *workspace, size_t workspace_bytes, void *stream);
int pea_nfm_rank_full_multi(int E, int H, int64_t num_users, int64_t num_items, const float *emb, int64_t ld_emb, const float *lin,
                            const float *w_fold, const float *b_fold, const float *w2, const float *bias_fold, const int64_t *uids,
                            int64_t n_users, const int64_t *pos_rowptr, const int64_t *pos_items, int64_t Q, int64_t item_lo,
                            int64_t n_items, int64_t item_node0, const int64_t *excl_rowptr, const int64_t *excl_items,
                            int32_t *above, int32_t *below, float *pos_score, int32_t *n_neg, int *err_flag, void *workspace,
                            size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PEAHIP_FM_EVAL_H_ */
