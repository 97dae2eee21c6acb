/* peahip_sample.h -- C ABI of the on-device KG triple sampler and row shuffle of libpeahip.so (gfx950), next to
 * include/peahip.h, whose conventions hold here too: every entry point returns PEA_OK or a negative PEA_ERR_* code (peahip.h)
 * with the text at pea_last_error(), pointers are device pointers, `stream` is a hipStream_t passed as void *, and nothing
 * synchronises.
 */
#ifndef PEAHIP_SAMPLE_H_
#define PEAHIP_SAMPLE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * The streams (csrc/kg_sampler.hip; tests/kg_sampler_ref.py restates them in numpy).  Every draw is the first output word of
 * Philox4x32-10 with key = (seed low word, seed high word) and counter (c0, c1, c2, c3); c2 carries a tag from bit 8 up (the BPR
 * sampler pea_sample_negatives draws with tag 0), c3 = offset.
 *   negative tail of store row e, attempt a = 0..63:   w = philox(e lo32, e hi32, a | 1 << 8, offset),
 *       t- = seg_lo[s] + ((w * seg_n[s]) >> 32),  s the segment of row e.
 *     With a key table (n_keys > 0) a draw is redrawn when t- == t+ or when ((s * num_nodes) + h) * num_nodes + t- is in
 *     keys_sorted (ascending, distinct); after 64 rejected attempts the last draw is kept and *exhausted counts the row.
 *   perm(e), a bijection of [0, n):  b = max(bit_length(n - 1), 1), hb = (b + 1) / 2, m = 2^hb - 1; one pass maps x to y by
 *       L = x >> hb, R = x & m;  for j = 0..3: F = philox(R, j, 2 << 8, offset) & m, (L, R) = (R, L ^ F);  y = (L << hb) | R
 *     and is applied again while y >= n.
 *
 * pea_kg_sample: out row (h, t+, t-, relation id) of every triple of a store laid out relation by relation.
 *   heads, tails [n_triples]; segment s holds rows seg_ptr[s] .. seg_ptr[s + 1] - 1 (seg_ptr [n_seg + 1], non-decreasing from 0
 *   to n_triples; an empty segment is legal), has relation id seg_rel[s] and draws its negatives from seg_n[s] nodes starting
 *   at seg_lo[s] (all int64 [n_seg], 1 <= seg_n[s] < 2^32).  The four tables are staged in LDS once per workgroup, which is why
 *   n_seg <= PEA_KG_MAX_SEGMENTS.  They live on the device: the caller, who built them, answers for seg_ptr being monotone
 *   and ending at n_triples and for seg_n being in range (a bad table gives wrong ids, never an access out of bounds: no load
 *   or store is addressed by a drawn id).
 *   shuffle: 0 writes row e at out row e; 1 writes it at out row perm(e) (the store is read in order, each 32-byte row is
 *   stored at its shuffled place).
 *   out [n_triples, ld_out] int64, ld_out >= 4, columns 4.. untouched; *exhausted (int) is cleared, then counted into.
 * pea_permute_rows: out[perm(i)] = in[i] for a table of n rows of `width` int64 words (1..PEA_PERMUTE_MAX_WIDTH), row strides
 *   ld_in, ld_out >= width; words between the rows of out are untouched.  in and out must not overlap.
 * Argument errors (null pointers with n > 0, ld_out < 4, n_seg outside 1..PEA_KG_MAX_SEGMENTS, num_nodes outside [1, 2^32),
 * n_keys > 0 without a table, n_seg * num_nodes^2 >= 2^63 with a table, a shuffle other than 0 or 1, width outside
 * 1..PEA_PERMUTE_MAX_WIDTH, a row stride below the width, overlapping tables) return PEA_ERR_ARG before anything is launched.
 * n == 0 returns PEA_OK and launches nothing.  One thread per row, 64-bit row indexing, integers only; the only atomic is
 * one integer add per workgroup into *exhausted.  Bitwise reproducible.
 * ---------------------------------------------------------------------------------------------- */
#define PEA_KG_MAX_SEGMENTS 1024
#define PEA_PERMUTE_MAX_WIDTH 16
int pea_kg_sample(int64_t n_triples, const int64_t *heads, const int64_t *tails, int n_seg, const int64_t *seg_ptr,
                  const int64_t *seg_rel, const int64_t *seg_lo, const int64_t *seg_n, int64_t num_nodes,
                  const int64_t *keys_sorted, int64_t n_keys, uint64_t seed, uint32_t offset, int shuffle, int64_t *out,
                  int64_t ld_out, int *exhausted, void *stream);
int pea_permute_rows(int64_t n, int width, const int64_t *in, int64_t ld_in, int64_t *out, int64_t ld_out, uint64_t seed,
                     uint32_t offset, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PEAHIP_SAMPLE_H_ */
