// Training head of the inner-product scorer (KGAT / KGCN / NGCF), forward AND backward in one launch.  The table of those
// models is cat_k normalize(X_k) over the conv outputs X_k (models/kgat.py:45-51); here the un-normalised X_k arrive as
// column blocks and the normalised table is never formed.  Per triple (u, i, j):
//   n_k(r) = X_k[r] / max(||X_k[r]||_2, 1e-12)                                    F.normalize, per block
//   pos = sum_k n_k(u) . n_k(i),  neg = sum_k n_k(u) . n_k(j),  loss = -sum_b log sigmoid(pos_b - neg_b)
//   grad_rows [3B, D]: d loss / d X_k[r] for r = u, i, j (rows 3b, 3b + 1, 3b + 2), THROUGH the normalisation:
//     inv (dn - n (n . dn)) with inv = 1 / ||X||, and dn / 1e-12 where the norm is below 1e-12 (the clamp's branch)
// One thread owns a triple: three passes over its rows (norms, dots, gradients); the rows come from the cache after the
// first.  The loss tail is train_common.h's: bpr_term, the block sum in thread order and the blocks in index order: no
// atomics on floats.  The host scatters grad_rows into the per-block gradient tables with pea_rows_scatter_sum
// (rows_scatter.hip).
#include "train_common.h"

namespace pea {
namespace {

constexpr int kTB = 64;          // triples per workgroup
constexpr int kMaxBlocks = 4;
constexpr float kNormEps = 1e-12f;

struct DotBlocks {
    const float *x[kMaxBlocks];
    int64_t ld[kMaxBlocks];
    int w[kMaxBlocks];
    int n;
};

__global__ __launch_bounds__(kTB) void dot_bpr_train_kernel(int64_t B, const DotBlocks blk, int D, int64_t N,
                                                            const int64_t *__restrict__ triples, int64_t stride,
                                                            float *__restrict__ grad_rows, float *block_sums, int *err) {
    const int64_t b = (int64_t)blockIdx.x * kTB + threadIdx.x;
    float term = 0.f;
    if (b < B) {
        int64_t id[3];
        bool ok = true;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            id[j] = triples[b * stride + j];
            ok = ok && id[j] >= 0 && id[j] < N;
        }
        float *grow = grad_rows + 3 * b * D;
        if (!ok) {
            atomicOr(err, 1);
            for (int c = 0; c < 3 * D; c += 4) *reinterpret_cast<float4 *>(grow + c) = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            float den[kMaxBlocks][3], pk[kMaxBlocks], nk[kMaxBlocks];
            float pos = 0.f, neg = 0.f;
#pragma unroll
            for (int k = 0; k < kMaxBlocks; ++k) {
                if (k >= blk.n) break;
                const int w = blk.w[k];
                const float *r0 = blk.x[k] + id[0] * blk.ld[k], *r1 = blk.x[k] + id[1] * blk.ld[k], *r2 = blk.x[k] + id[2] * blk.ld[k];
                float q0 = 0.f, q1 = 0.f, q2 = 0.f;
                for (int c = 0; c < w; c += 4) {
                    const float4 a = ld4(r0 + c), p = ld4(r1 + c), q = ld4(r2 + c);
                    q0 = fmaf(a.x, a.x, q0); q0 = fmaf(a.y, a.y, q0); q0 = fmaf(a.z, a.z, q0); q0 = fmaf(a.w, a.w, q0);
                    q1 = fmaf(p.x, p.x, q1); q1 = fmaf(p.y, p.y, q1); q1 = fmaf(p.z, p.z, q1); q1 = fmaf(p.w, p.w, q1);
                    q2 = fmaf(q.x, q.x, q2); q2 = fmaf(q.y, q.y, q2); q2 = fmaf(q.z, q.z, q2); q2 = fmaf(q.w, q.w, q2);
                }
                den[k][0] = fmaxf(sqrtf(q0), kNormEps);
                den[k][1] = fmaxf(sqrtf(q1), kNormEps);
                den[k][2] = fmaxf(sqrtf(q2), kNormEps);
                float dp = 0.f, dn = 0.f;
                for (int c = 0; c < w; c += 4) {
                    const float4 a = ld4(r0 + c), p = ld4(r1 + c), q = ld4(r2 + c);
                    const float ax = a.x / den[k][0], ay = a.y / den[k][0], az = a.z / den[k][0], aw = a.w / den[k][0];
                    dp = fmaf(ax, p.x / den[k][1], dp); dp = fmaf(ay, p.y / den[k][1], dp);
                    dp = fmaf(az, p.z / den[k][1], dp); dp = fmaf(aw, p.w / den[k][1], dp);
                    dn = fmaf(ax, q.x / den[k][2], dn); dn = fmaf(ay, q.y / den[k][2], dn);
                    dn = fmaf(az, q.z / den[k][2], dn); dn = fmaf(aw, q.w / den[k][2], dn);
                }
                pk[k] = dp;
                nk[k] = dn;
                pos += dp;
                neg += dn;
            }
            const float d = pos - neg;
            float gp;      // d loss / d pos;  d loss / d neg = -gp
            bpr_term(d, term, gp);
            int col = 0;
#pragma unroll
            for (int k = 0; k < kMaxBlocks; ++k) {
                if (k >= blk.n) break;
                const int w = blk.w[k];
                const float *r0 = blk.x[k] + id[0] * blk.ld[k], *r1 = blk.x[k] + id[1] * blk.ld[k], *r2 = blk.x[k] + id[2] * blk.ld[k];
                const float d0 = den[k][0], d1 = den[k][1], d2 = den[k][2];
                // n . dn per row: u: gp (pos_k - neg_k), i: gp pos_k, j: -gp neg_k; a clamped row takes dn / eps
                const float t0 = d0 > kNormEps ? gp * (pk[k] - nk[k]) : 0.f;
                const float t1 = d1 > kNormEps ? gp * pk[k] : 0.f;
                const float t2 = d2 > kNormEps ? -gp * nk[k] : 0.f;
                for (int c = 0; c < w; c += 4) {
                    const float4 a = ld4(r0 + c), p = ld4(r1 + c), q = ld4(r2 + c);
                    const float av[4] = {a.x, a.y, a.z, a.w}, pv[4] = {p.x, p.y, p.z, p.w}, qv[4] = {q.x, q.y, q.z, q.w};
                    float g0[4], g1[4], g2[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float n0 = av[e] / d0, n1 = pv[e] / d1, n2 = qv[e] / d2;
                        g0[e] = (gp * (n1 - n2) - n0 * t0) / d0;
                        g1[e] = (gp * n0 - n1 * t1) / d1;
                        g2[e] = (-gp * n0 - n2 * t2) / d2;
                    }
                    *reinterpret_cast<float4 *>(grow + col + c) = make_float4(g0[0], g0[1], g0[2], g0[3]);
                    *reinterpret_cast<float4 *>(grow + D + col + c) = make_float4(g1[0], g1[1], g1[2], g1[3]);
                    *reinterpret_cast<float4 *>(grow + 2 * D + col + c) = make_float4(g2[0], g2[1], g2[2], g2[3]);
                }
                col += w;
            }
        }
    }
    block_sum_in_order<kTB>(term, block_sums + blockIdx.x);      // triple order inside the block
}

__global__ __launch_bounds__(64) void dot_bpr_final_kernel(int n_blocks, const float *block_sums, float *loss) {
    if (threadIdx.x == 0) store_loss(block_sums, n_blocks, loss);      // blocks in index order
}

}  // namespace
}  // namespace pea

using namespace pea;

extern "C" size_t pea_dot_bpr_train_workspace_bytes(int64_t B) {
    return B < 0 ? 0 : kWsSumsOffset + (size_t)((B + kTB - 1) / kTB + 4) * sizeof(float);
}

extern "C" int pea_dot_bpr_train(int64_t B, int n_blocks, const float *const *blocks_host, const int64_t *ld_host,
                                 const int *widths_host, int64_t num_nodes, const int64_t *triples, int64_t triple_stride,
                                 float *out_loss, float *grad_rows, void *workspace, size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    PEA_REQUIRE(B >= 0 && n_blocks >= 1 && n_blocks <= kMaxBlocks && blocks_host && ld_host && widths_host, PEA_ERR_ARG,
                "dot_bpr_train: B=%lld, %d blocks (1..%d)", (long long)B, n_blocks, kMaxBlocks);
    DotBlocks blk = {};
    blk.n = n_blocks;
    int D = 0;
    for (int k = 0; k < n_blocks; ++k) {
        const int w = widths_host[k];
        PEA_REQUIRE(w >= 4 && w % 4 == 0 && w <= 256, PEA_ERR_ARG, "dot_bpr_train: block %d width %d (a multiple of 4)", k, w);
        PEA_REQUIRE(blocks_host[k] && aligned16(blocks_host[k]) && ld_host[k] >= w && ld_host[k] % 4 == 0,
                    PEA_ERR_ARG, "dot_bpr_train: block %d pointer / stride %lld", k, (long long)ld_host[k]);
        blk.x[k] = blocks_host[k];
        blk.ld[k] = ld_host[k];
        blk.w[k] = w;
        D += w;
    }
    PEA_REQUIRE(D <= 256, PEA_ERR_ARG, "dot_bpr_train: total width %d (<= 256)", D);
    PEA_REQUIRE(num_nodes > 0 && triples && triple_stride >= 3 && out_loss && grad_rows && workspace, PEA_ERR_ARG,
                "dot_bpr_train: bad argument");
    PEA_REQUIRE(workspace_bytes >= pea_dot_bpr_train_workspace_bytes(B), PEA_ERR_NOMEM, "dot_bpr_train: workspace too small");
    int *err = ws_err_flag(workspace);
    float *sums = ws_sums(workspace);
    PEA_MEMSET_ASYNC(err, 0, sizeof(int), stream);
    const int blocks = (int)((B + kTB - 1) / kTB);
    ProfScope ps("dot_bpr_train", stream, (double)B * 3.0 * D * 8.0);
    if (blocks > 0) {
        PEA_LAUNCH(dot_bpr_train_kernel, dim3(blocks), dim3(kTB), 0, stream, B, blk, D, num_nodes, triples, triple_stride,
                   grad_rows, sums, err);
        PEA_HIP(hipGetLastError());
    }
    PEA_LAUNCH(dot_bpr_final_kernel, dim3(1), dim3(64), 0, stream, blocks, (const float *)sums, out_loss);
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}
