/* peahip_fm.h -- C ABI of the factorisation-machine models of libpeahip.so (gfx950), next to include/peahip.h, whose
 * conventions hold here too: every entry point returns PEA_OK or a negative PEA_ERR_* code (peahip.h) with the text at
 * pea_last_error(), pointers are device pointers unless their name ends in _host, `stream` is a hipStream_t passed as
 * void *, and nothing synchronises unless it says so.
 */
#ifndef PEAHIP_FM_H_
#define PEAHIP_FM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * NFM (csrc/nfm.hip): reference models/nfm.py, which wraps torchfm's NeuralFactorizationMachineModel.  The reference's own
 * file fixes the id concatenation, the MSE-on-sigmoid loss and the parameter names; the arithmetic inside torchfm is
 * [recalled] from pytorch-fm 0.7 (torchfm.model.nfm, torchfm.layer) and restated in tests/nfm_ref.py:
 *     U = num_users, I = num_items, E = emb_dim, H = hidden_size; ids are LOCAL: u in [0, U), i in [0, I)
 *     emb [U + I, E] (row stride ld_emb), lin [U + I] ; the rows of a pair are u and U + i
 *     c    = 0.5 ((e_u + e_i)^2 - (e_u^2 + e_i^2))                      [B, E]   (written as torchfm writes it)
 *     a    = keep1 s (((c - mean1) / sqrt(var1 + eps)) bn1_w + bn1_b)   batch mean and BIASED variance over the B rows
 *     h    = a W1^T + b1                                                W1 [H, E] (torch Linear layout)
 *     r    = keep2 s relu(((h - mean2) / sqrt(var2 + eps)) bn2_w + bn2_b)
 *     y    = ((lin[u] + lin[U + i]) + bias0) + (r . w2 + b2),   pred = sigmoid(y),   *out_loss = sum_b (pred_b - label_b)^2 / B
 * pea_nfm_supported(E, H): pure, needs no device.  E and H multiples of 4 in 4..128 (csrc/nfm.hip says why).
 * pea_nfm_train: the whole training step of B rows (uids, iids int64 [B], labels float32 [B]), 2 <= B <= 8192, as a chain of
 *   launches whose only dependencies are kernel boundaries; no float atomics, grids = f(B), bitwise reproducible.
 *   Dropout: keep1 [B, E] / keep2 [B, H] are byte masks (non-zero = kept) scaled by keep_scale = 1 / (1 - p), both given or
 *   both NULL (no dropout); nothing is drawn here.
 *   batch_stats [2 E + 2 H] = [mean1 | var1 | mean2 | var2] is always written.  update_running != 0: the four running buffers
 *   become (1 - momentum) old + momentum new, the variance entering UNBIASED (B / (B - 1)), as torch's BatchNorm1d does in
 *   training mode (the caller counts num_batches_tracked).
 *   d_dense and grad_rows are both given, or both NULL (forward only: same *out_loss, pred, batch_stats and running buffers):
 *     d_dense [H E + 2 H + 4 + 2 E + 2 H] = [dW1 (H E) | db1 (H) | dw2 (H) | db2, dbias0, 0, 0 | dbn1_w (E) | dbn1_b (E) |
 *                                            dbn2_w (H) | dbn2_b (H)]
 *     grad_rows [2 B, E + 4]: row b = [d loss / d e_u of pair b | d loss / d lin[u], 0, 0, 0], row B + b the item's: the caller
 *       scatters them by the 2 B positions (u_b, then U + i_b) into a zero-filled [U + I, E + 4] buffer with ONE
 *       pea_rows_scatter_sum (P = 1, R = E + 4): columns 0..E-1 are emb's gradient, column E is lin's.
 *     pos_ids [2 B] (optional, only with grad_rows): those positions as the scatter takes them, u_b at b and U + i_b at B + b,
 *       -1 (skipped by the scatter) for both positions of a pair with an id out of range.
 *   Stays asynchronous: a row with u outside [0, U) or i outside [0, I) sets the int at workspace[0] to 1; nothing is read or
 *   written through it and its two gradient rows are zero.  Batch normalisation couples all rows, so the other numbers of
 *   such a call are unspecified, but finite.
 *   Argument errors return PEA_ERR_ARG (a short workspace PEA_ERR_NOMEM) before anything is launched.
 *   workspace: pea_nfm_train_workspace_bytes(B, E, H) (0 = unsupported shape or B outside 2..8192).
 * pea_nfm_fold: the eval-mode MLP as one affine map and a relu, from the parameters and the RUNNING statistics:
 *     s1 = bn1_w / sqrt(bn1_var + eps), t1 = bn1_b - bn1_mean s1, s2 and t2 likewise;
 *     w_fold [H, E] = (s2[o] W1[o][e]) s1[e],  b_fold [H] = s2 (W1 t1 + b1) + t2,  bias_fold [1] = bias0 + b2.
 * pea_nfm_score: y = ((lin[u] + lin[U + i]) + bias_fold) + relu(w_fold (e_u (.) e_i) + b_fold) . w2 over the folded weights,
 *   the product on MFMA.  One kernel body, three addressing forms (mode):
 *     PEA_NFM_PAIRS  n_users pairs (uids[k], iids[k]);                         outputs [n_users]
 *     PEA_NFM_ROWS   uids [n_users] x candidate rows iids [n_users, C];        outputs [n_users, C]
 *     PEA_NFM_RANGE  uids [n_users] x the items item_lo .. item_lo + C - 1;    outputs [n_users, C] (iids unused)
 *   logits and / or pred = sigmoid(logits) are written (at least one is given).  PEA_NFM_ROWS with rank [n_users] (int32) and
 *   auc [n_users] (both or neither; needs logits): rank = the columns 1.. whose logit is strictly higher than column 0's,
 *   auc = the share of them strictly lower (0 for C = 1): the contract of pea_dot_rank_eval.
 *   A pair with an id out of range sets *err_flag (an int32 the caller zeroed) to 1, reads nothing and scores logit 0.
 * ---------------------------------------------------------------------------------------------- */
#define PEA_NFM_PAIRS 0
#define PEA_NFM_ROWS 1
#define PEA_NFM_RANGE 2
#define PEA_NFM_MAX_BATCH 8192
int pea_nfm_supported(int E, int H);
size_t pea_nfm_train_workspace_bytes(int64_t B, int E, int H);
int pea_nfm_train(int64_t B, int E, int H, int64_t num_users, int64_t num_items, const float *emb, int64_t ld_emb,
                  const float *lin, const float *bias0, const float *bn1_w, const float *bn1_b, float *bn1_mean,
                  float *bn1_var, const float *w1, const float *b1, const float *bn2_w, const float *bn2_b,
                  float *bn2_mean, float *bn2_var, const float *w2, const float *b2, float eps, float momentum,
                  int update_running, const int64_t *uids, const int64_t *iids, const float *labels,
                  const unsigned char *keep1, const unsigned char *keep2, float keep_scale, float *out_loss, float *pred,
                  float *batch_stats, float *d_dense, float *grad_rows, int64_t *pos_ids, void *workspace,
                  size_t workspace_bytes, void *stream);
int pea_nfm_fold(int E, int H, const float *w1, const float *b1, const float *bn1_w, const float *bn1_b, const float *bn1_mean,
                 const float *bn1_var, const float *bn2_w, const float *bn2_b, const float *bn2_mean, const float *bn2_var,
                 const float *bias0, const float *b2, float eps, float *w_fold, float *b_fold, float *bias_fold, void *stream);
int pea_nfm_score(int mode, int64_t n_users, int64_t C, int64_t item_lo, int E, int H, int64_t num_users, int64_t num_items,
                  const float *emb, int64_t ld_emb, const float *lin, const float *w_fold, const float *b_fold,
                  const float *w2, const float *bias_fold, const int64_t *uids, const int64_t *iids, float *logits,
                  float *pred, int *rank, float *auc, int *err_flag, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PEAHIP_FM_H_ */
