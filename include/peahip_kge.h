/* peahip_kge.h -- C ABI of the knowledge-graph-embedding models of libpeahip.so (gfx950), next to include/peahip.h, whose
 * conventions hold here too: every entry point returns PEA_OK or a negative PEA_ERR_* code (peahip.h) with the text at
 * pea_last_error(), pointers are device pointers unless their name ends in _host, `stream` is a hipStream_t passed as
 * void *, and nothing synchronises unless it says so.
 */
#ifndef PEAHIP_KGE_H_
#define PEAHIP_KGE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * CFKG (csrc/cfkg.hip): reference models/cfkg.py with the kg_loss of experiments/cfkg_solver_bpr.py:95-106 over B quadruples
 * (int64 rows (h, t+, t-, rel), row stride quad_stride >= 4) and its whole gradient, in one launch + a fixed-order reduction.
 * x [num_nodes, emb] (row stride ldx), r [num_rel, emb] (row stride ldr):
 *     hr = x[h] + r[rel]  (fp32, formed first),  pos = <hr, x[t+]>,  neg = <hr, x[t-]>
 *         (a group of L lanes per quadruple, L the smallest power of two with 4 L >= emb: one fma chain over a lane's four
 *          columns in ascending order, then a butterfly sum over the L lanes),
 *     *out_loss = -(sum_b log sigmoid(pos_b) + sum_b log sigmoid(-neg_b))   (sigmoid then log in fp32, as the reference),
 *   and with a = sigmoid(pos) - 1, b = sigmoid(neg), GH = a x[t+] + b x[t-]:
 *     grad_rows [3B, emb] (rows 3b, 3b + 1, 3b + 2 = h, t+, t-): GH, a hr, b hr,
 *     grad_r [num_rel, emb] = sum over the quadruples of relation rel of GH: every row written, zeros for a relation the
 *     batch does not name.  It is summed inside the launch (one [num_rel, emb] partial per workgroup in LDS, the tile's rows
 *     added in row order; the partials added in workgroup order): no scatter over relation ids is needed.
 *   The caller scatters grad_rows into a zero-filled [num_nodes, emb] gradient with pea_rows_scatter_sum (P = 1, R = emb;
 *   3B <= 16384).
 * pea_cfkg_supported(emb, num_rel): emb a multiple of 4 in 4..128, 1 <= num_rel <= PEA_CFKG_MAX_REL (the partial is at most
 *   32 KB of LDS); pure, needs no device.
 * pos_pred / neg_pred [B] are optional: both given or both NULL.  grad_rows and grad_r are both given, or both NULL: forward
 * only, no backward work is done and *out_loss has the same bits.  x may be a column block of a wider buffer: ldx and ldr are
 * multiples of 4 and at least emb; x, r, grad_rows and grad_r start on 16-byte boundaries.
 * The grid is a function of B alone; the loss is one sum per workgroup added in index order: no float atomics, bitwise
 * reproducible, 64-bit row indexing.
 * Stays asynchronous: a quadruple with a node id outside [0, num_nodes) or a relation id outside [0, num_rel) contributes
 *   nothing (three zero gradient rows, pos = neg = 0), reads nothing out of range and sets the int at workspace[0] to 1.
 * Argument errors return PEA_ERR_ARG (a short workspace PEA_ERR_NOMEM) before anything is launched.
 * workspace: pea_cfkg_train_workspace_bytes(B, emb, num_rel) (0 = unsupported or B < 0).
 * ---------------------------------------------------------------------------------------------- */
#define PEA_CFKG_MAX_REL 64
int pea_cfkg_supported(int emb, int num_rel);
size_t pea_cfkg_train_workspace_bytes(int64_t B, int emb, int num_rel);
int pea_cfkg_train(int64_t B, int emb, const float *x, int64_t ldx, int64_t num_nodes, const float *r, int64_t ldr,
                   int64_t num_rel, const int64_t *quads, int64_t quad_stride, float *out_loss, float *pos_pred,
                   float *neg_pred, float *grad_rows, float *grad_r, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PEAHIP_KGE_H_ */
