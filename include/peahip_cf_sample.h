/* peahip_cf_sample.h -- C ABI of the on-device CF epoch sampler of libpeahip.so (gfx950), next to include/peahip.h, whose
 * conventions hold here too: the entry point returns PEA_OK or a negative PEA_ERR_* code (peahip.h) with the text at
 * pea_last_error(), pointers are device pointers, `stream` is a hipStream_t passed as void *, and nothing synchronises.
 */
#ifndef PEAHIP_CF_SAMPLE_H_
#define PEAHIP_CF_SAMPLE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * pea_cf_sample: the whole CF training table of an epoch from one launch (csrc/cf_sampler.hip; tests/cf_sampler_ref.py restates
 * its streams in numpy), one thread per output row.
 *
 * Rows, r the row index before the shuffle, from the positives pos_u, pos_i [n_pos] (the user2item pairs in dataset order) and
 * k negatives per positive:
 *   mode 0 (BPR), no entity tables   n_pos * k rows (u, i+, i-), row r from positive r / k: the layout of pea_sample_negatives
 *   mode 0 (BPR), entity tables      the same rows, nine columns (u, i+, i-, e+, e-, mask_i, f+, f-, mask_u): the columns
 *                                    pea_entity_reg reads
 *   mode 1 (BCE)                     n_pos * (1 + k) rows of three columns: rows 0 .. n_pos - 1 are (u, i+, 1), row n_pos + j is
 *                                    (u of positive j / k, sampled item, 0).  Entity tables are refused.
 *
 * The streams.  Every draw is a word of Philox4x32-10 with key = (seed low word, seed high word) and counter (c0, c1, c2, c3);
 * c2 carries a tag from bit 8 up, c3 = offset.
 *   negative item of negative number j (mode 0: j = r; mode 1: j = r - n_pos), attempt a = 0..63, tag 0:
 *       w = philox(j lo32, j hi32, a, offset).x,   i- = item_lo + ((w * num_items) >> 32).
 *     With a key table (keys_sorted non-null: ascending, distinct) the draw is rejected while u * num_items + (i- - item_lo)
 *     is in it; after 64 rejections the last draw is kept and *exhausted counts the row.  Word for word the stream of
 *     pea_sample_negatives: columns 0..2 of an unshuffled mode-0 table are its output for the same seed and offset.
 *   entity columns of row r, tag 3: ONE call  E = philox(r lo32, r hi32, 3 << 8, offset),  all four words used.
 *       [a, b) = item_ent_ptr[i+ - item_lo], item_ent_ptr[i+ - item_lo + 1],  L = b - a.
 *       L == 0:  (e+, e-, mask_i) = (0, 0, 0).
 *       else     e+ = item_ent[a + ((E.x * L) >> 32)];  B the last block with block_lo[B] <= e+ (the first when there is none);
 *                e- = block_lo[B] + ((E.y * block_n[B]) >> 32);  mask_i = 1.   e- may equal e+.
 *     (f+, f-, mask_u) the same from E.z, E.w, user_ent_ptr[u - user_lo ..] and user_ent.
 *   shuffle == 1: row r is stored at out row perm(r), perm the bijection of [0, n_rows) that peahip_sample.h states (tag 2),
 *     unchanged: a shuffled table is pea_permute_rows of the unshuffled one with the same seed and offset.
 *
 * Tables.  keys_sorted [n_keys], keyed as pea_sample_negatives keys it.  item_ent_ptr [num_items + 1] / item_ent [nnz_i] and
 * user_ent_ptr [num_users + 1] / user_ent [nnz_u]: CSR of the entity node ids of every item and user; all four are null (no
 * entity columns) or none is.  With them, block_lo, block_n [n_blocks] are the node-type blocks (block_lo ascending, 1 <=
 * block_n < 2^32, the caller's to keep), staged in LDS, which is why n_blocks <= PEA_CF_MAX_BLOCKS; without them n_blocks,
 * block_lo, block_n, nnz_i and nnz_u are not looked at.
 *
 * No load is addressed by an unchecked id.  A row is BAD when an id it carries from pos_u / pos_i lies outside
 * [user_lo, user_lo + num_users) / [item_lo, item_lo + num_items), or when a CSR range read for it is not 0 <= a <= b <= nnz: it
 * keeps its ids as given, takes item_lo as its negative without a draw and (0, 0, 0) for each triple of entity columns, is
 * counted in *bad_rows (never in *exhausted) and reads nothing out of range.  Drawn ids and entity ids are only written.
 *
 * out [n_rows, ld_out] int64, ld_out >= the row width (3 or 9); columns beyond the width and the words between rows are
 * untouched.  *exhausted and *bad_rows (int) are cleared, then counted into: one integer add per workgroup each.
 * Argument errors (a null pointer with n_pos > 0, k < 1, a mode other than 0 or 1, a shuffle other than 0 or 1, ld_out below
 * the row width, item_lo or user_lo below 0, num_items or num_users outside [1, 2^32), n_keys < 0 or n_keys > 0 without a table,
 * a key table with (user_lo + num_users) * num_items >= 2^63, some but not all of the four entity tables, entity tables
 * with mode 1, entity tables with n_blocks outside 1..PEA_CF_MAX_BLOCKS, without block_lo / block_n or with nnz outside [0, 2^32),
 * more rows than the grid holds) return PEA_ERR_ARG before anything is launched.  n_pos == 0 returns PEA_OK and launches
 * nothing.  Integers only, no scratch, 64-bit row indexing.  Bitwise reproducible.
 * ---------------------------------------------------------------------------------------------- */
#define PEA_CF_MAX_BLOCKS 64
#define PEA_CF_BPR 0
#define PEA_CF_BCE 1
int pea_cf_sample(int64_t n_pos, int k, int mode, const int64_t *pos_u, const int64_t *pos_i, int64_t item_lo, int64_t num_items,
                  int64_t user_lo, int64_t num_users, const int64_t *keys_sorted, int64_t n_keys, const int64_t *item_ent_ptr,
                  const int64_t *item_ent, int64_t nnz_i, const int64_t *user_ent_ptr, const int64_t *user_ent, int64_t nnz_u,
                  int n_blocks, const int64_t *block_lo, const int64_t *block_n, uint64_t seed, uint32_t offset, int shuffle,
                  int64_t *out, int64_t ld_out, int *exhausted, int *bad_rows, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PEAHIP_CF_SAMPLE_H_ */
