// Metapath ablation sweep in one pass (reference: the --metapath_test loop of graph_recsys_benchmark/solvers.py:224-241,
// model.eval(metapath_idx) -> models/base.py:191-195 -> metrics() once per metapath).  The conv stack does not depend on
// the masked channel; only the fusion does.  So:
//   fuse_ablate_kernel  one pass over the stack, every row's P channel vectors read once, all P + 1 fused variants written
//   rank_multi_kernel   (fuse_score.hip) the batched evaluator over all variants in one launch
// Variant v of fuse_ablate_kernel is bitwise what fuse_kernel(masked = v - 1) gives: the fusion step and the channel logit
// are the one definition of score_common.h, and nothing is shared between variants but loads and the per-row logits.  No
// float atomics.
#include <algorithm>

#include "model.h"
#include "score_common.h"

namespace pea {
namespace {

// Lane layout of fuse_kernel (fuse_score.hip): G lanes x float4 cover the R columns of one node, 256 / G nodes per workgroup.
// PREG > 0: P <= PREG, the row's channel vectors and logits stay in registers across the P + 1 variants (every loop over
// channels is unrolled to PREG with a uniform p < P guard, so nothing is indexed at run time).  PREG == 0: any P <=
// kMaxChannels; the variants re-read the row (it was just fetched: L1 / L2 hits) and recompute the logits.
// out [P + 1, N, R]: variant 0 unmasked, variant 1 + p with channel p zeroed (it stays in the softmax with logit 0 / in the
// mean's divisor, as in the reference).  out_att [N, P] (optional): softmax weights of variant 0, 1 / P under 'mean'.
template <int G, int PREG>
__global__ __launch_bounds__(256) void fuse_ablate_kernel(int64_t N, int P, int R, const float *__restrict__ stack,
                                                          int64_t ld, const ChanCols col_of_channel, const ChanCopy copy,
                                                          const float *__restrict__ att, int mode,
                                                          float *__restrict__ out, float *__restrict__ out_att) {
    const int64_t item = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    const int sl = threadIdx.x % G;
    const bool valid = item < N;
    const int64_t n = valid ? item : 0;
    const bool in_row = sl * 4 < R;
    const bool active = valid && in_row;
    const int c4 = in_row ? sl * 4 : 0;
    const float *row0 = stack + n * ld;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool mean = mode == PEA_FUSE_MEAN;
    float *dst = out + n * R + c4;
    const int64_t variant_stride = N * (int64_t)R;
    const unsigned long long lone = copy_row_bits(copy, P, n);
    stage_copy_rows(copy, P, R, smem);

    if constexpr (PREG > 0) {
        float4 x[PREG];
        float lg[PREG];
#pragma unroll
        for (int p = 0; p < PREG; ++p) {
            x[p] = zero;
            lg[p] = 0.f;
            if (p < P) {
                x[p] = chan_value(row0 + col_of_channel.c[p], copy.c[p], copy, smem + 3 * p * R, R, (lone >> p) & 1, n, c4, sl);
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
                float4 xv = chan_value(row0 + col_of_channel.c[p], copy.c[p], copy, smem + 3 * p * R, R, (lone >> p) & 1, n, c4, sl);
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
                    if (!mean) w = expf(chan_logit<G>(chan_value(row0 + col_of_channel.c[p], copy.c[p], copy, smem + 3 * p * R, R, (lone >> p) & 1, n, c4, sl), ld4(att + p * R + c4), in_row) - m) * inv;
                    if (valid && p % G == sl) out_att[n * P + p] = w;
                }
            }
        }
    }
}

constexpr int kRegSmall = 4, kRegChannels = 16;   // register-resident paths: P <= 4, P <= 16; above: re-read the row

template <int G>
int launch_fuse_ablate_g(int64_t N, int P, int R, const float *stack, int64_t ld, const ChanCols &cols, const ChanCopy &copy, const float *att,
                         int mode, float *out, float *out_att, hipStream_t stream) {
    const unsigned blocks = (unsigned)((N + (256 / G) - 1) / (256 / G));
    if (P <= kRegSmall)
        PEA_LAUNCH((fuse_ablate_kernel<G, kRegSmall>), dim3(blocks), dim3(256), copy_lds_bytes(copy, P, R), stream, N, P, R, stack, ld, cols, copy, att,
                   mode, out, out_att);
    else if (P <= kRegChannels)
        PEA_LAUNCH((fuse_ablate_kernel<G, kRegChannels>), dim3(blocks), dim3(256), copy_lds_bytes(copy, P, R), stream, N, P, R, stack, ld, cols, copy, att,
                   mode, out, out_att);
    else
        PEA_LAUNCH((fuse_ablate_kernel<G, 0>), dim3(blocks), dim3(256), copy_lds_bytes(copy, P, R), stream, N, P, R, stack, ld, cols, copy, att, mode,
                   out, out_att);
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}

}  // namespace

int launch_fuse_ablate(int64_t N, int P, int R, const float *stack, int64_t ld, const ChanCols &col_of_channel,
                       const ChanCopy &copy, const float *att, int mode, float *out_tables, float *out_att, hipStream_t stream) {
    PEA_REQUIRE(N > 0 && stack && out_tables, PEA_ERR_ARG, "fuse_ablate: null argument");
    PEA_REQUIRE(P > 0 && P <= kMaxChannels && R > 0 && R % 4 == 0 && R <= 256, PEA_ERR_ARG,
                "fuse_ablate: P=%d R=%d (P <= 64, R a multiple of 4 and <= 256)", P, R);
    PEA_REQUIRE(mode == PEA_FUSE_ATT || mode == PEA_FUSE_MEAN, PEA_ERR_ARG, "fuse_ablate: mode %d", mode);
    PEA_REQUIRE(mode == PEA_FUSE_MEAN || att != nullptr, PEA_ERR_ARG, "fuse_ablate: att is required for 'att' fusion");
    PEA_REQUIRE(ld % 4 == 0, PEA_ERR_ARG, "fuse_ablate: stack row stride must be a multiple of 4");
    PEA_REQUIRE(copy_lds_bytes(copy, P, R) <= kCopyLdsMax, PEA_ERR_ARG, "fuse_ablate: copy rows of a %d x %d stack", P, R);
    // bytes: the stack once, P + 1 tables out
    ProfScope ps("fuse_ablate", stream, 4.0 * (double)N * R * (2.0 * P + 1.0));
    switch (lanes_for_r(R)) {
        case 1: return launch_fuse_ablate_g<1>(N, P, R, stack, ld, col_of_channel, copy, att, mode, out_tables, out_att, stream);
        case 2: return launch_fuse_ablate_g<2>(N, P, R, stack, ld, col_of_channel, copy, att, mode, out_tables, out_att, stream);
        case 4: return launch_fuse_ablate_g<4>(N, P, R, stack, ld, col_of_channel, copy, att, mode, out_tables, out_att, stream);
        case 8: return launch_fuse_ablate_g<8>(N, P, R, stack, ld, col_of_channel, copy, att, mode, out_tables, out_att, stream);
        case 16: return launch_fuse_ablate_g<16>(N, P, R, stack, ld, col_of_channel, copy, att, mode, out_tables, out_att, stream);
        case 32: return launch_fuse_ablate_g<32>(N, P, R, stack, ld, col_of_channel, copy, att, mode, out_tables, out_att, stream);
        default: return launch_fuse_ablate_g<64>(N, P, R, stack, ld, col_of_channel, copy, att, mode, out_tables, out_att, stream);
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
    return launch_fuse_ablate(num_nodes, P, R, stack, ld_stack, cols, ChanCopy{}, att, fuse_mode, out_tables, out_att, (hipStream_t)stream);
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
