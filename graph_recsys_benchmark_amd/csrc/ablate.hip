// Metapath ablation sweep in one pass (reference: the --metapath_test loop of graph_recsys_benchmark/solvers.py:224-241,
// model.eval(metapath_idx) -> models/base.py:191-195 -> metrics() once per metapath).  The conv stack does not depend on
// the masked channel; only the fusion does.  So:
//   fuse_ablate_kernel  one pass over the stack, every row's P channel vectors read once, all P + 1 fused variants written
//   rank_multi_kernel   the batched evaluator of fuse_score.hip over all variants in one launch
// Variant v of either kernel is bitwise what fuse_kernel(masked = v - 1) / rank_kernel(tables[v]) give: same operations in
// the same order per variant, nothing shared between variants but loads and the per-row logits.  No float atomics.
#include <algorithm>

#include "model.h"
#include "score_common.h"

namespace pea {
namespace {

// One online-softmax step of fuse_kernel (channel order; the same expressions, so the same bits).
__device__ __forceinline__ void softmax_step(float sc, const float4 &x, float &m, float &s, float4 &acc) {
    const float mn = fmaxf(m, sc);
    const float f = expf(m - mn), w = expf(sc - mn);
    s = s * f + w;
    acc.x = acc.x * f + w * x.x;
    acc.y = acc.y * f + w * x.y;
    acc.z = acc.z * f + w * x.z;
    acc.w = acc.w * f + w * x.w;
    m = mn;
}

// the channel logit x_p . att_p of fuse_kernel: per-lane partial, then the G-lane butterfly
template <int G>
__device__ __forceinline__ float chan_logit(const float4 &x, const float4 &a, bool in_row) {
    float sc = in_row ? (x.x * a.x + x.y * a.y) + (x.z * a.z + x.w * a.w) : 0.f;
#pragma unroll
    for (int off = 1; off < G; off <<= 1) sc += __shfl_xor(sc, off);
    return sc;
}

// Lane layout of fuse_kernel: G lanes x float4 cover the R columns of one node, 256 / G nodes per workgroup.
// PREG > 0: P <= PREG, the row's channel vectors and logits stay in registers across the P + 1 variants (every loop over
// channels is unrolled to PREG with a uniform p < P guard, so nothing is indexed at run time).  PREG == 0: any P <=
// kMaxChannels; the variants re-read the row (it was just fetched: L1 / L2 hits) and recompute the logits.
// out [P + 1, N, R]: variant 0 unmasked, variant 1 + p with channel p zeroed (it stays in the softmax with logit 0 / in the
// mean's divisor, as in the reference).  out_att [N, P] (optional): softmax weights of variant 0, 1 / P under 'mean'.
template <int G, int PREG>
__global__ __launch_bounds__(256) void fuse_ablate_kernel(int64_t N, int P, int R, const float *__restrict__ stack,
                                                          int64_t ld, const ChanCols col_of_channel,
                                                          const float *__restrict__ att, int mode,
                                                          float *__restrict__ out, float *__restrict__ out_att) {
    const int64_t item = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    const int sl = threadIdx.x % G;
    const bool valid = item < N;
    const int64_t n = valid ? item : 0;
    const bool in_row = sl * 4 < R;
    const bool active = valid && in_row;
    const int c4 = in_row ? sl * 4 : 0;
    const float *row = stack + n * ld + c4;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool mean = mode == PEA_FUSE_MEAN;
    float *dst = out + n * R + c4;
    const int64_t variant_stride = N * (int64_t)R;

    if constexpr (PREG > 0) {
        float4 x[PREG];
        float lg[PREG];
#pragma unroll
        for (int p = 0; p < PREG; ++p) {
            x[p] = zero;
            lg[p] = 0.f;
            if (p < P) {
                x[p] = ld4(row + col_of_channel.c[p]);
                if (!mean) lg[p] = chan_logit<G>(x[p], ld4(att + p * R + c4), in_row);
            }
        }
        for (int v = 0; v <= P; ++v) {
            const int masked = v - 1;
            float m = -3.0e38f, s = 0.f;
            float4 acc = zero;
#pragma unroll
            for (int p = 0; p < PREG; ++p) {
                if (p < P) {
                    const bool off = p == masked;
                    const float4 xv = off ? zero : x[p];
                    if (mean) {
                        acc.x += xv.x; acc.y += xv.y; acc.z += xv.z; acc.w += xv.w;
                    } else {
                        softmax_step(off ? 0.f : lg[p], xv, m, s, acc);
                    }
                }
            }
            const float inv = mean ? 1.0f / (float)P : 1.0f / s;
            if (active)
                *reinterpret_cast<float4 *>(dst + (int64_t)v * variant_stride) =
                    make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
            if (v == 0 && out_att && valid) {
#pragma unroll
                for (int p = 0; p < PREG; ++p)
                    if (p < P && p % G == sl) out_att[n * P + p] = mean ? inv : expf(lg[p] - m) * inv;
            }
        }
    } else {
        for (int v = 0; v <= P; ++v) {
            const int masked = v - 1;
            float m = -3.0e38f, s = 0.f;
            float4 acc = zero;
            for (int p = 0; p < P; ++p) {
                float4 xv = ld4(row + col_of_channel.c[p]);
                if (p == masked) xv = zero;
                if (mean) {
                    acc.x += xv.x; acc.y += xv.y; acc.z += xv.z; acc.w += xv.w;
                    continue;
                }
                softmax_step(chan_logit<G>(xv, ld4(att + p * R + c4), in_row), xv, m, s, acc);
            }
            const float inv = mean ? 1.0f / (float)P : 1.0f / s;
            if (active)
                *reinterpret_cast<float4 *>(dst + (int64_t)v * variant_stride) =
                    make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
            if (v == 0 && out_att) {
                for (int p = 0; p < P; ++p) {      // uniform trip count: the butterfly inside needs every lane
                    float w = inv;
                    if (!mean) w = expf(chan_logit<G>(ld4(row + col_of_channel.c[p]), ld4(att + p * R + c4), in_row) - m) * inv;
                    if (valid && p % G == sl) out_att[n * P + p] = w;
                }
            }
        }
    }
}

// rank_kernel (fuse_score.hip) over V tables: one wave per user, and the wave walks the variants.  The staged fc1 / fc2
// weights are loaded once per workgroup; with a shared candidate block (cand_stride == 0) the ids of the first two wave
// passes (C <= 128 covers the reference's 1 + 99) are loaded once and kept in registers.  Per variant the scoring and the
// wave reductions are rank_kernel's, statement for statement.
__global__ __launch_bounds__(256) void rank_multi_kernel(int V, int64_t U, int C, int R, int64_t N,
                                                         const float *__restrict__ tables,
                                                         const int64_t *__restrict__ unids,
                                                         const int64_t *__restrict__ cand, int64_t cand_stride,
                                                         const float *fc1_w, const float *fc1_b, const float *fc2_w,
                                                         const float *fc2_b, float *scores, int32_t *rank, float *auc,
                                                         float *loss, int *err) {
    stage_mlp(R, fc1_w, fc1_b, fc2_w);
    const float *w1 = smem, *b1 = smem + 2 * R * R, *w2 = b1 + R;
    const int lane = threadIdx.x % kWave;
    const int64_t uidx = (int64_t)blockIdx.x * (256 / kWave) + threadIdx.x / kWave;
    if (uidx >= U) return;
    const int64_t u = unids[uidx];
    if (u < 0 || u >= N) {
        if (lane == 0) atomicOr(err, 1);
        return;
    }
    const bool shared = cand_stride == 0;
    int64_t keep0 = -1, keep1 = -1;
    if (shared) {
        if (lane < C) keep0 = cand[uidx * C + lane];
        if (kWave + lane < C) keep1 = cand[uidx * C + kWave + lane];
    }
    const float b2 = fc2_b[0];
    for (int v = 0; v < V; ++v) {
        const float *repr = tables + (int64_t)v * N * R;
        const int64_t *cv = cand + (int64_t)v * cand_stride + uidx * C;
        const int64_t orow = (int64_t)v * U + uidx;
        float pos = 0.f;
        int higher = 0, gt = 0;
        float lsum = 0.f;
        float4 ur[4];
        if (R == 16) load_row<4>(repr + u * R, ur);
        for (int base = 0; base < C; base += kWave) {
            const int c = base + lane;
            float sc = 0.f;
            bool ok = c < C;
            if (ok) {
                const int64_t i = shared && base == 0 ? keep0 : shared && base == kWave ? keep1 : cv[c];
                if (i < 0 || i >= N) {
                    atomicOr(err, 1);
                    ok = false;
                } else {
                    if (R == 16) {
                        float4 ir[4];
                        load_row<4>(repr + i * R, ir);
                        sc = mlp_score_reg<4>(ur, ir, w1, b1, w2, b2);
                    } else {
                        sc = mlp_score(repr + u * R, repr + i * R, R, w1, b1, w2, b2);
                    }
                    if (scores) scores[orow * C + c] = sc;
                }
            }
            if (base == 0) pos = __shfl(sc, 0);
            if (ok && c > 0) {
                higher += sc > pos ? 1 : 0;
                gt += pos > sc ? 1 : 0;
                lsum += log_sigmoid_ref(pos - sc);
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            higher += __shfl_xor(higher, off);
            gt += __shfl_xor(gt, off);
            lsum += __shfl_xor(lsum, off);
        }
        if (lane == 0) {
            if (rank) rank[orow] = higher;
            if (auc) auc[orow] = (float)gt / (float)(C - 1);
            if (loss) loss[orow] = -lsum;
        }
    }
}

constexpr int kRegSmall = 4, kRegChannels = 16;   // register-resident paths: P <= 4, P <= 16; above: re-read the row

template <int G>
int launch_fuse_ablate_g(int64_t N, int P, int R, const float *stack, int64_t ld, const ChanCols &cols, const float *att,
                         int mode, float *out, float *out_att, hipStream_t stream) {
    const unsigned blocks = (unsigned)((N + (256 / G) - 1) / (256 / G));
    if (P <= kRegSmall)
        PEA_LAUNCH((fuse_ablate_kernel<G, kRegSmall>), dim3(blocks), dim3(256), 0, stream, N, P, R, stack, ld, cols, att, mode,
                   out, out_att);
    else if (P <= kRegChannels)
        PEA_LAUNCH((fuse_ablate_kernel<G, kRegChannels>), dim3(blocks), dim3(256), 0, stream, N, P, R, stack, ld, cols, att,
                   mode, out, out_att);
    else
        PEA_LAUNCH((fuse_ablate_kernel<G, 0>), dim3(blocks), dim3(256), 0, stream, N, P, R, stack, ld, cols, att, mode, out,
                   out_att);
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}

}  // namespace

int launch_fuse_ablate(int64_t N, int P, int R, const float *stack, int64_t ld, const ChanCols &col_of_channel,
                       const float *att, int mode, float *out_tables, float *out_att, hipStream_t stream) {
    PEA_REQUIRE(N > 0 && stack && out_tables, PEA_ERR_ARG, "fuse_ablate: null argument");
    PEA_REQUIRE(P > 0 && P <= kMaxChannels && R > 0 && R % 4 == 0 && R <= 256, PEA_ERR_ARG,
                "fuse_ablate: P=%d R=%d (P <= 64, R a multiple of 4 and <= 256)", P, R);
    PEA_REQUIRE(mode == PEA_FUSE_ATT || mode == PEA_FUSE_MEAN, PEA_ERR_ARG, "fuse_ablate: mode %d", mode);
    PEA_REQUIRE(mode == PEA_FUSE_MEAN || att != nullptr, PEA_ERR_ARG, "fuse_ablate: att is required for 'att' fusion");
    PEA_REQUIRE(ld % 4 == 0, PEA_ERR_ARG, "fuse_ablate: stack row stride must be a multiple of 4");
    // bytes: the stack once, P + 1 tables out
    ProfScope ps("fuse_ablate", stream, 4.0 * (double)N * R * (2.0 * P + 1.0));
    switch (lanes_for_r(R)) {
        case 1: return launch_fuse_ablate_g<1>(N, P, R, stack, ld, col_of_channel, att, mode, out_tables, out_att, stream);
        case 2: return launch_fuse_ablate_g<2>(N, P, R, stack, ld, col_of_channel, att, mode, out_tables, out_att, stream);
        case 4: return launch_fuse_ablate_g<4>(N, P, R, stack, ld, col_of_channel, att, mode, out_tables, out_att, stream);
        case 8: return launch_fuse_ablate_g<8>(N, P, R, stack, ld, col_of_channel, att, mode, out_tables, out_att, stream);
        case 16: return launch_fuse_ablate_g<16>(N, P, R, stack, ld, col_of_channel, att, mode, out_tables, out_att, stream);
        case 32: return launch_fuse_ablate_g<32>(N, P, R, stack, ld, col_of_channel, att, mode, out_tables, out_att, stream);
        default: return launch_fuse_ablate_g<64>(N, P, R, stack, ld, col_of_channel, att, mode, out_tables, out_att, stream);
    }
}

}  // namespace pea

// ---------------------------------------------------------------------------------------------- C ABI
using namespace pea;

extern "C" int pea_fuse_ablate(int64_t num_nodes, int P, int R, const float *stack, int64_t ld_stack,
                               const int *col_of_channel_host, const float *att, int fuse_mode, float *out_tables,
                               float *out_att, void *stream) {
    PEA_REQUIRE(num_nodes > 0 && stack && out_tables && col_of_channel_host, PEA_ERR_ARG, "fuse_ablate: null argument");
    PEA_REQUIRE(P > 0 && P <= kMaxChannels, PEA_ERR_ARG, "fuse_ablate: P=%d (1..%d)", P, kMaxChannels);
    ChanCols cols{};
    for (int p = 0; p < P; ++p) {
        PEA_REQUIRE(col_of_channel_host[p] >= 0 && col_of_channel_host[p] % 4 == 0 && col_of_channel_host[p] + R <= ld_stack,
                    PEA_ERR_ARG, "fuse_ablate: channel %d column %d outside the stack row", p, col_of_channel_host[p]);
        cols.c[p] = col_of_channel_host[p];
    }
    return launch_fuse_ablate(num_nodes, P, R, stack, ld_stack, cols, att, fuse_mode, out_tables, out_att, (hipStream_t)stream);
}

extern "C" int pea_model_forward_ablate(pea_model *model, const float *const *params_host, const float *x, const float *att,
                                        void *workspace, size_t workspace_bytes, float *out_tables, float *out_att,
                                        void *stream) {
    PEA_REQUIRE(out_tables, PEA_ERR_ARG, "forward_ablate: null argument");
    PEA_REQUIRE(!model || model->plan->shard_world == 1, PEA_ERR_ARG, "forward_ablate: single GPU only (the plan is sharded)");
    PEA_TRY(check_forward_args("forward_ablate", model, params_host, x, workspace, workspace_bytes, -1, nullptr));
    PEA_REQUIRE(model->d.fuse_mode == PEA_FUSE_MEAN || att, PEA_ERR_ARG, "forward_ablate: att is required for 'att' fusion");
    const AblateOut abl{out_tables, out_att};
    ForwardCall c;
    c.model = model;
    c.params = params_host;
    c.x = x;
    c.ldx = model->d.emb_dim;
    c.att = att;
    c.wsf = aligned_ws(workspace);
    c.stream = (hipStream_t)stream;
    c.abl = &abl;
    return model_forward(c);
}

extern "C" int pea_rank_eval_multi(int V, int64_t U, int C, int R, int64_t num_nodes, const float *tables,
                                   const int64_t *unids, const int64_t *cand, int64_t cand_variant_stride,
                                   const float *fc1_w, const float *fc1_b, const float *fc2_w, const float *fc2_b,
                                   float *scores, int32_t *rank, float *auc, float *loss, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    PEA_REQUIRE(R > 0 && R % 4 == 0 && R <= 64, PEA_ERR_ARG, "repr_dim %d must be a multiple of 4, <= 64", R);
    PEA_REQUIRE(V >= 1 && U >= 0 && C >= 2 && num_nodes > 0 && tables && unids && cand && fc1_w && fc1_b && fc2_w && fc2_b,
                PEA_ERR_ARG, "rank_eval_multi: bad argument");
    PEA_REQUIRE(cand_variant_stride == 0 || cand_variant_stride == U * (int64_t)C, PEA_ERR_ARG,
                "rank_eval_multi: cand_variant_stride %lld (0 = one shared [U, C] block, else U * C)",
                (long long)cand_variant_stride);
    if (U == 0) return PEA_OK;
    int *err = err_flag_for_current_device();
    PEA_REQUIRE(err != nullptr, PEA_ERR_HIP, "rank_eval_multi: no error-flag buffer on this device");
    PEA_MEMSET_ASYNC(err, 0, sizeof(int), stream);
    const size_t sh = (size_t)(2 * R * R + 2 * R) * sizeof(float);
    {
        ProfScope ps("rank_eval_multi", stream, (double)V * U * C * (4.0 * R + 12.0));
        PEA_LAUNCH(rank_multi_kernel, dim3((unsigned)((U + 3) / 4)), dim3(256), sh, stream, V, U, C, R, num_nodes, tables, unids,
                   cand, cand_variant_stride, fc1_w, fc1_b, fc2_w, fc2_b, scores, rank, auc, loss, err);
    }
    int rc = hipGetLastError() == hipSuccess ? PEA_OK : PEA_ERR_HIP;
    if (rc == PEA_OK) rc = read_err_flag(err, stream, "rank_eval_multi");
    return rc;
}
