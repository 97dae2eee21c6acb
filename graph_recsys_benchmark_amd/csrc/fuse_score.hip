// Channel fusion, BPR scoring and the batched evaluator for gfx950.
//   fuse_kernel   graph_recsys_benchmark/models/base.py:193-203  (stack, ablation mask, 'att'/'mean')
//   bpr kernels   models/base.py:208-214 (predict) + models/base.py:46-48 (-sum log sigmoid(pos-neg))
//   rank kernel   solvers.py:85-96 (score 1 + C-1 candidates, rank of the positive, auc, eval loss), over V tables at once
// All reductions have a fixed order (no float atomics): results are bitwise reproducible.
#include <algorithm>
#include <mutex>

#include "score_common.h"

namespace pea {
namespace {

// G lanes x float4 cover the R columns of one node; 64/G nodes per wave.  Softmax over the P channels
// is taken online in channel order.
// Sharded ranks: workgroups past the `fuse_blocks` that cover the rank's own rows fuse the rows a BPR batch names
// (FuseSelect): the same arithmetic on the same stack row as the table entry, written to sel.out[k] when this rank owns the
// node, zeros otherwise (the loss all-reduce sums these; round 2 ran a separate select launch over the finished table).
template <int G>
__global__ __launch_bounds__(256) void fuse_kernel(int64_t n_rows, const int *__restrict__ rows, int P, int R,
                                                   const float *__restrict__ stack, int64_t ld,
                                                   const ChanCols col_of_channel, const ChanCopy copy,
                                                   const float *__restrict__ att, int masked, int mode,
                                                   float *__restrict__ out, float *__restrict__ out_stack,
                                                   unsigned fuse_blocks, const FuseSelect sel, int64_t N) {
    const bool pick = blockIdx.x >= fuse_blocks;
    const int64_t item = (int64_t)(pick ? blockIdx.x - fuse_blocks : blockIdx.x) * (256 / G) + threadIdx.x / G;
    const int sl = threadIdx.x % G;
    bool valid = item < (pick ? sel.n : n_rows);
    int64_t n = 0;
    if (pick) {
        const int64_t id = valid ? sel.ids[item * sel.id_stride] : 0;
        const bool in_range = id >= 0 && id < N;
        if (valid && !in_range && sl == 0) atomicOr(sel.err, 1);
        const bool mine = in_range && (id / sel.tile) % sel.world == sel.rank;
        if (valid && !mine && sl * 4 < R) *reinterpret_cast<float4 *>(sel.out + item * R + sl * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        valid = valid && mine;
        n = valid ? id : 0;
        out_stack = nullptr;
    } else {
        n = valid ? (rows ? rows[item] : item) : 0;
    }
    float *dst_row = pick ? sel.out + item * R : (out ? out + n * R : nullptr);
    const bool active = valid && sl * 4 < R;
    const int c4 = sl * 4 < R ? sl * 4 : 0;
    float m = -3.0e38f, s = 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const unsigned long long lone = copy_row_bits(copy, P, n);
    stage_copy_rows(copy, P, R, smem);
    for (int p = 0; p < P; ++p) {
        float4 x = chan_value(stack + n * ld + col_of_channel.c[p], copy.c[p], copy, smem + 3 * p * R, R, (lone >> p) & 1, n, c4, sl);
        if (p == masked) x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (out_stack && active) *reinterpret_cast<float4 *>(out_stack + (n * P + p) * R + c4) = x;
        if (mode == PEA_FUSE_MEAN) {
            acc.x += x.x; acc.y += x.y; acc.z += x.z; acc.w += x.w;
            continue;
        }
        softmax_step(chan_logit<G>(x, ld4(att + p * R + c4), sl * 4 < R), x, m, s, acc);
    }
    if (!active || !dst_row) return;
    const float inv = mode == PEA_FUSE_MEAN ? 1.0f / (float)P : 1.0f / s;
    *reinterpret_cast<float4 *>(dst_row + c4) = make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
}

__global__ __launch_bounds__(256) void bpr_kernel(int64_t B, int R, int64_t N, const float *__restrict__ repr,
                                                  const int64_t *__restrict__ triples, int64_t stride,
                                                  const float *fc1_w, const float *fc1_b, const float *fc2_w,
                                                  const float *fc2_b, float *pos, float *neg, float *block_sums,
                                                  int *err) {
    stage_mlp(R, fc1_w, fc1_b, fc2_w);
    const float *w1 = smem, *b1 = smem + 2 * R * R, *w2 = b1 + R;
    __shared__ float red[256];
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float term = 0.f;
    if (b < B) {
        const int64_t u = triples[b * stride], ip = triples[b * stride + 1], in = triples[b * stride + 2];
        if (u < 0 || u >= N || ip < 0 || ip >= N || in < 0 || in >= N) {
            atomicOr(err, 1);
        } else {
            float sp, sn;
            if (R == 16) {  // the reference's repr_dim: all three rows fetched once, up front
                float4 ur[4], pr[4], nr[4];
                load_row<4>(repr + u * R, ur);
                load_row<4>(repr + ip * R, pr);
                load_row<4>(repr + in * R, nr);
                sp = mlp_score_reg<4>(ur, pr, w1, b1, w2, fc2_b[0]);
                sn = mlp_score_reg<4>(ur, nr, w1, b1, w2, fc2_b[0]);
            } else {
                sp = mlp_score(repr + u * R, repr + ip * R, R, w1, b1, w2, fc2_b[0]);
                sn = mlp_score(repr + u * R, repr + in * R, R, w1, b1, w2, fc2_b[0]);
            }
            if (pos) pos[b] = sp;
            if (neg) neg[b] = sn;
            term = log_sigmoid_ref(sp - sn);
        }
    }
    red[threadIdx.x] = term;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) block_sums[blockIdx.x] = red[0];
}

// An out-of-range triple contributed nothing to its block sum: the loss would be silently too small, so it is poisoned
// with NaN instead (the reference raises at cached_repr[unids]; the host mirror raises IndexError when it next reads the
// flag, see engine.check_pending_errors).
__global__ __launch_bounds__(256) void bpr_final_kernel(int n_blocks, const float *block_sums, const int *err, float *loss) {
    __shared__ float red[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < n_blocks; i += 256) s += block_sums[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = err[0] ? __int_as_float(0x7fc00000) : -red[0];
}

__global__ __launch_bounds__(256) void predict_kernel(int64_t B, int R, int64_t N, const float *__restrict__ repr,
                                                      const int64_t *__restrict__ unids,
                                                      const int64_t *__restrict__ inids, const float *fc1_w,
                                                      const float *fc1_b, const float *fc2_w, const float *fc2_b,
                                                      float *pred, int *err) {
    stage_mlp(R, fc1_w, fc1_b, fc2_w);
    const float *w1 = smem, *b1 = smem + 2 * R * R, *w2 = b1 + R;
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int64_t u = unids[b], i = inids[b];
    if (u < 0 || u >= N || i < 0 || i >= N) {
        atomicOr(err, 1);
        return;
    }
    if (R == 16) {
        float4 ur[4], ir[4];
        load_row<4>(repr + u * R, ur);
        load_row<4>(repr + i * R, ir);
        pred[b] = mlp_score_reg<4>(ur, ir, w1, b1, w2, fc2_b[0]);
    } else {
        pred[b] = mlp_score(repr + u * R, repr + i * R, R, w1, b1, w2, fc2_b[0]);
    }
}

// The batched evaluator (solvers.py:85-96) over V tables: one wave per user, and the wave walks the variants; V = 1 is
// pea_rank_eval.  The staged fc1 / fc2 weights are loaded once per workgroup; with a shared candidate block
// (cand_stride == 0) the ids of the first two wave passes (C <= 128 covers the reference's 1 + 99) are loaded once and kept
// in registers.  Per variant the ranking is rank_one_user of score_common.h.
__global__ __launch_bounds__(256) void rank_multi_kernel(int V, int64_t U, int C, int R, int64_t N,
                                                         const float *__restrict__ tables,
                                                         const int64_t *__restrict__ unids,
                                                         const int64_t *__restrict__ cand, int64_t cand_stride,
                                                         const float *fc1_w, const float *fc1_b, const float *fc2_w,
                                                         const float *fc2_b, float *scores, int32_t *rank, float *auc,
                                                         float *loss, int *err) {
    stage_mlp(R, fc1_w, fc1_b, fc2_w);
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
        const int64_t *cv = cand + (int64_t)v * cand_stride + uidx * C;
        const MlpScorer score(tables + (int64_t)v * N * R, u, R, b2);
        rank_one_user(score, [&](int base, int c) { return shared && base == 0 ? keep0 : shared && base == kWave ? keep1 : cv[c]; },
                      C, N, lane, (int64_t)v * U + uidx, scores, rank, auc, loss, err);
    }
}

}  // namespace

int launch_fuse(int64_t N, int P, int R, const float *stack, int64_t ld, const ChanCols &col_of_channel, const ChanCopy &copy,
                const float *att, int masked, int mode, const int *rows, int64_t n_rows, float *out,
                float *out_stack, hipStream_t stream, const FuseSelect *sel_in) {
    PEA_REQUIRE(P > 0 && P <= kMaxChannels && R > 0 && R % 4 == 0 && R <= 256, PEA_ERR_ARG,
                "fuse: P=%d R=%d (P <= 64, R a multiple of 4 and <= 256)", P, R);
    PEA_REQUIRE(masked < P, PEA_ERR_ARG, "fuse: masked channel %d out of range (P=%d)", masked, P);
    PEA_REQUIRE(mode == PEA_FUSE_MEAN || att != nullptr, PEA_ERR_ARG, "fuse: att is required for 'att' fusion");
    PEA_REQUIRE(ld % 4 == 0, PEA_ERR_ARG, "fuse: stack row stride must be a multiple of 4");
    if (!rows) n_rows = N;
    FuseSelect sel;
    if (sel_in && sel_in->n > 0) {
        sel = *sel_in;
        PEA_REQUIRE(sel.ids && sel.out && sel.err && sel.world >= 1 && sel.tile >= 1 && out != nullptr, PEA_ERR_ARG,
                    "fuse: batch-row selection needs ids, an output, an error flag and the fused table");
    }
    if (n_rows <= 0 && sel.n <= 0) return PEA_OK;
    const int G = lanes_for_r(R);
    const size_t lds = copy_lds_bytes(copy, P, R);
    PEA_REQUIRE(lds <= kCopyLdsMax, PEA_ERR_ARG, "fuse: copy rows of a %d x %d stack", P, R);
    ProfScope ps("fuse", stream, 4.0 * (double)(n_rows + sel.n) * R * (P + 1));
    const unsigned fuse_blocks = (unsigned)((std::max<int64_t>(n_rows, 0) + (256 / G) - 1) / (256 / G));
    const unsigned blocks = fuse_blocks + (unsigned)((sel.n + (256 / G) - 1) / (256 / G));
#define PEA_FUSE_CASE(g)                                                                                       \
    case g:                                                                                                    \
        PEA_LAUNCH(fuse_kernel<g>, dim3(blocks), dim3(256), lds, stream, n_rows, rows, P, R, stack, ld, \
                           col_of_channel, copy, att, masked, mode, out, out_stack, fuse_blocks, sel, N);            \
        break;
    switch (G) {
        PEA_FUSE_CASE(1)
        PEA_FUSE_CASE(2)
        PEA_FUSE_CASE(4)
        PEA_FUSE_CASE(8)
        PEA_FUSE_CASE(16)
        PEA_FUSE_CASE(32)
        default:
            PEA_LAUNCH(fuse_kernel<64>, dim3(blocks), dim3(256), lds, stream, n_rows, rows, P, R, stack, ld,
                               col_of_channel, copy, att, masked, mode, out, out_stack, fuse_blocks, sel, N);
    }
#undef PEA_FUSE_CASE
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}

}  // namespace pea

// ---------------------------------------------------------------------------------------------- C ABI
using pea::set_error;
using pea::err_flag_for_current_device;
using pea::read_err_flag;

extern "C" size_t pea_bpr_workspace_bytes(int64_t B) {
    const int64_t blocks = (B + 255) / 256;
    return (size_t)(blocks + 1) * sizeof(float) + 16;
}

static int check_r(int R) {
    PEA_REQUIRE(R > 0 && R % 4 == 0 && R <= 64, PEA_ERR_ARG, "repr_dim %d must be a multiple of 4, <= 64", R);
    return PEA_OK;
}

// One 4-byte error flag per device, allocated on first use and kept for the life of the process (pea_predict /
// pea_rank_eval used to hipMalloc + hipFree one per call).  The callers are the reference's single Python thread; two
// host threads scoring at once on one device would share the flag (an error is then reported to at least one of them).
int *pea::err_flag_for_current_device() {
    static std::mutex mu;
    static int *flags[64] = {nullptr};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (!flags[dev] && hipMalloc(&flags[dev], 256) != hipSuccess) flags[dev] = nullptr;
    return flags[dev];
}

int pea::read_err_flag(int *err_dev, hipStream_t stream, const char *what) {
    int h = 0;
    PEA_HIP(hipMemcpyAsync(&h, err_dev, sizeof(int), hipMemcpyDeviceToHost, stream));
    PEA_HIP(hipStreamSynchronize(stream));
    PEA_REQUIRE(h == 0, PEA_ERR_RANGE, "%s: node id outside [0, num_nodes)", what);
    return PEA_OK;
}

extern "C" int pea_bpr_score(int64_t B, int R, int64_t num_nodes, const float *repr, const int64_t *triples,
                             int64_t triple_stride, const float *fc1_w, const float *fc1_b, const float *fc2_w,
                             const float *fc2_b, float *pos, float *neg, float *loss, void *workspace,
                             size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    PEA_TRY(check_r(R));
    PEA_REQUIRE(B >= 0 && triple_stride >= 3, PEA_ERR_ARG, "bpr: B=%lld stride=%lld", (long long)B, (long long)triple_stride);
    PEA_REQUIRE(repr && triples && fc1_w && fc1_b && fc2_w && fc2_b && loss && workspace, PEA_ERR_ARG, "bpr: null pointer");
    PEA_REQUIRE(workspace_bytes >= pea_bpr_workspace_bytes(B), PEA_ERR_NOMEM, "bpr: workspace too small");
    const int blocks = (int)((B + 255) / 256);
    int *err = (int *)workspace;
    float *sums = (float *)workspace + 4;
    PEA_MEMSET_ASYNC(err, 0, sizeof(int), stream);
    const size_t sh = (size_t)(2 * R * R + 2 * R) * sizeof(float);
    pea::ProfScope ps("bpr_score", stream, (double)B * (12.0 + 12.0 * R + 4.0));
    if (blocks > 0) {
        PEA_LAUNCH(pea::bpr_kernel, dim3(blocks), dim3(256), sh, stream, B, R, num_nodes, repr, triples,
                           triple_stride, fc1_w, fc1_b, fc2_w, fc2_b, pos, neg, sums, err);
        PEA_HIP(hipGetLastError());
    }
    PEA_LAUNCH(pea::bpr_final_kernel, dim3(1), dim3(256), 0, stream, blocks, sums, err, loss);
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}

extern "C" int pea_predict(int64_t B, int R, int64_t num_nodes, const float *repr, const int64_t *unids,
                           const int64_t *inids, const float *fc1_w, const float *fc1_b, const float *fc2_w,
                           const float *fc2_b, float *pred, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    PEA_TRY(check_r(R));
    PEA_REQUIRE(B >= 0 && repr && unids && inids && fc1_w && fc1_b && fc2_w && fc2_b && pred, PEA_ERR_ARG, "predict: bad argument");
    if (B == 0) return PEA_OK;
    int *err = err_flag_for_current_device();
    PEA_REQUIRE(err != nullptr, PEA_ERR_HIP, "predict: no error-flag buffer on this device");
    PEA_MEMSET_ASYNC(err, 0, sizeof(int), stream);
    const size_t sh = (size_t)(2 * R * R + 2 * R) * sizeof(float);
    PEA_LAUNCH(pea::predict_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), sh, stream, B, R, num_nodes,
                       repr, unids, inids, fc1_w, fc1_b, fc2_w, fc2_b, pred, err);
    int rc = hipGetLastError() == hipSuccess ? PEA_OK : PEA_ERR_HIP;
    if (rc == PEA_OK) rc = read_err_flag(err, stream, "predict");
    return rc;
}

extern "C" int pea_rank_eval(int64_t U, int C, int R, int64_t num_nodes, const float *repr, const int64_t *unids,
                             const int64_t *cand, const float *fc1_w, const float *fc1_b, const float *fc2_w,
                             const float *fc2_b, float *scores, int32_t *rank, float *auc, float *loss,
                             void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    PEA_TRY(check_r(R));
    PEA_REQUIRE(U >= 0 && C >= 2 && repr && unids && cand && fc1_w && fc1_b && fc2_w && fc2_b, PEA_ERR_ARG, "rank_eval: bad argument");
    if (U == 0) return PEA_OK;
    int *err = err_flag_for_current_device();
    PEA_REQUIRE(err != nullptr, PEA_ERR_HIP, "rank_eval: no error-flag buffer on this device");
    PEA_MEMSET_ASYNC(err, 0, sizeof(int), stream);
    const size_t sh = (size_t)(2 * R * R + 2 * R) * sizeof(float);
    // the V = 1 case of the multi-table evaluator, the candidates read per table (stride U * C: nothing register-cached)
    PEA_LAUNCH(pea::rank_multi_kernel, dim3((unsigned)((U + 3) / 4)), dim3(256), sh, stream, 1, U, C, R, num_nodes, repr,
               unids, cand, U * (int64_t)C, fc1_w, fc1_b, fc2_w, fc2_b, scores, rank, auc, loss, err);
    int rc = hipGetLastError() == hipSuccess ? PEA_OK : PEA_ERR_HIP;
    if (rc == PEA_OK) rc = read_err_flag(err, stream, "rank_eval");
    return rc;
}

extern "C" int pea_rank_eval_multi(int V, int64_t U, int C, int R, int64_t num_nodes, const float *tables,
                                   const int64_t *unids, const int64_t *cand, int64_t cand_variant_stride,
                                   const float *fc1_w, const float *fc1_b, const float *fc2_w, const float *fc2_b,
                                   float *scores, int32_t *rank, float *auc, float *loss, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    PEA_TRY(check_r(R));
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
        pea::ProfScope ps("rank_eval_multi", stream, (double)V * U * C * (4.0 * R + 12.0));
        PEA_LAUNCH(pea::rank_multi_kernel, dim3((unsigned)((U + 3) / 4)), dim3(256), sh, stream, V, U, C, R, num_nodes, tables, unids,
                   cand, cand_variant_stride, fc1_w, fc1_b, fc2_w, fc2_b, scores, rank, auc, loss, err);
    }
    int rc = hipGetLastError() == hipSuccess ? PEA_OK : PEA_ERR_HIP;
    if (rc == PEA_OK) rc = read_err_flag(err, stream, "rank_eval_multi");
    return rc;
}

extern "C" int pea_fuse(int64_t num_nodes, int P, int R, const float *stack, int64_t ld_stack,
                        const int *col_of_channel_host, const float *att, int masked_channel, int fuse_mode, float *out,
                        void *stream) {
    PEA_REQUIRE(num_nodes > 0 && stack && out && col_of_channel_host, PEA_ERR_ARG, "fuse: null argument");
    PEA_REQUIRE(P > 0 && P <= pea::kMaxChannels, PEA_ERR_ARG, "fuse: P=%d (1..%d)", P, pea::kMaxChannels);
    PEA_REQUIRE(fuse_mode == PEA_FUSE_ATT || fuse_mode == PEA_FUSE_MEAN, PEA_ERR_ARG, "fuse: mode %d", fuse_mode);
    PEA_REQUIRE(masked_channel >= -1, PEA_ERR_ARG, "fuse: masked channel %d", masked_channel);
    pea::ChanCols cols{};
    for (int p = 0; p < P; ++p) {
        PEA_REQUIRE(col_of_channel_host[p] >= 0 && col_of_channel_host[p] % 4 == 0 && col_of_channel_host[p] + R <= ld_stack,
                    PEA_ERR_ARG, "fuse: channel %d column %d outside the stack row", p, col_of_channel_host[p]);
        cols.c[p] = col_of_channel_host[p];
    }
    return pea::launch_fuse(num_nodes, P, R, stack, ld_stack, cols, pea::ChanCopy{}, att, masked_channel, fuse_mode, nullptr, num_nodes, out,
                            nullptr, (hipStream_t)stream);
}
