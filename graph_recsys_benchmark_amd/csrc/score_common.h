// Device helpers shared by the scoring kernels of fuse_score.hip, ablate.hip and dot_score.hip, each defined ONCE so that
// every kernel that uses one gives the same bits: the fc2(relu(fc1([u || i]))) scorer of graph_recsys_benchmark/models/
// base.py:208-214, the online-softmax step and channel logit of the fusion, the ranking of one user by one wave
// (solvers.py:85-96), and the per-device error flag the id-range checks report through.
#ifndef PEA_SCORE_COMMON_H_
#define PEA_SCORE_COMMON_H_

#include "agg_common.h"

namespace pea {

// One 4-byte error flag per device, allocated on first use and kept for the life of the process (fuse_score.hip).
int *err_flag_for_current_device();
// copies the flag back (one stream synchronisation); PEA_ERR_RANGE when a kernel set it
int read_err_flag(int *err_dev, hipStream_t stream, const char *what);

// lanes (x float4) that cover the R columns of one node in fuse_kernel and fuse_ablate_kernel: both must cut a row alike
inline int lanes_for_r(int R) {
    int g = 1;
    while (g * 4 < R) g <<= 1;
    return g;
}

namespace {

// fc2(relu(fc1([u || i])))  with fc1_w [R, 2R] staged in LDS by the caller
__device__ __forceinline__ float mlp_score(const float *__restrict__ ur, const float *__restrict__ ir, int R,
                                           const float *w1, const float *b1, const float *w2, float b2) {
    float o = 0.f;
    for (int k = 0; k < R; ++k) {
        const float *w = w1 + k * 2 * R;
        float a = 0.f;
        for (int c = 0; c < R; c += 4) {
            const float4 u = ld4(ur + c), wu = ld4(w + c);
            a += (u.x * wu.x + u.y * wu.y) + (u.z * wu.z + u.w * wu.w);
        }
        for (int c = 0; c < R; c += 4) {
            const float4 v = ld4(ir + c), wi = ld4(w + R + c);
            a += (v.x * wi.x + v.y * wi.y) + (v.z * wi.z + v.w * wi.w);
        }
        a += b1[k];
        o = fmaf(fmaxf(a, 0.f), w2[k], o);
    }
    return o + b2;
}

// same arithmetic with both rows held in registers (R = 4*R4 known at compile time)
template <int R4>
__device__ __forceinline__ float mlp_score_reg(const float4 (&u)[R4], const float4 (&v)[R4], const float *w1, const float *b1,
                                               const float *w2, float b2) {
    constexpr int R = 4 * R4;
    float o = 0.f;
    for (int k = 0; k < R; ++k) {
        const float *w = w1 + k * 2 * R;
        float a = 0.f;
#pragma unroll
        for (int c = 0; c < R4; ++c) {
            const float4 wu = ld4(w + 4 * c);
            a += (u[c].x * wu.x + u[c].y * wu.y) + (u[c].z * wu.z + u[c].w * wu.w);
        }
#pragma unroll
        for (int c = 0; c < R4; ++c) {
            const float4 wi = ld4(w + R + 4 * c);
            a += (v[c].x * wi.x + v[c].y * wi.y) + (v[c].z * wi.z + v[c].w * wi.w);
        }
        a += b1[k];
        o = fmaf(fmaxf(a, 0.f), w2[k], o);
    }
    return o + b2;
}

template <int R4>
__device__ __forceinline__ void load_row(const float *p, float4 (&r)[R4]) {
#pragma unroll
    for (int c = 0; c < R4; ++c) r[c] = ld4(p + 4 * c);
}

extern __shared__ float smem[];

__device__ __forceinline__ void stage_mlp(int R, const float *fc1_w, const float *fc1_b, const float *fc2_w) {
    for (int i = threadIdx.x; i < 2 * R * R; i += blockDim.x) smem[i] = fc1_w[i];
    for (int i = threadIdx.x; i < R; i += blockDim.x) {
        smem[2 * R * R + i] = fc1_b[i];
        smem[2 * R * R + R + i] = fc2_w[i];
    }
    __syncthreads();
}

// bit p: node n is a copy row of channel p.  All flags are fetched before the channel loop of a fusion kernel, several loads
// in flight, so that no row load of the loop waits for its flag first.
__device__ __forceinline__ unsigned long long copy_row_bits(const ChanCopy &cc, int P, int64_t n) {
    unsigned long long bits = 0;
    if (!cc.on) return bits;
#pragma unroll 8
    for (int p = 0; p < P; ++p) {
        const unsigned char *flag = cc.c[p].deg0;
        bits |= (unsigned long long)(flag != nullptr && flag[n] != 0) << p;
    }
    return bits;
}

// The packed rows the copy-row branch of chan_value reads, staged once per workgroup: [P][bias | att_j | att_i][R] floats of
// dynamic LDS (copy_lds_bytes; att rows zero for GCN), so that the branch, which starts when the row's own load has
// arrived, does not wait for a second memory latency.  (What the branch costs the fusion launch on the 25m-shaped graph,
// 0.044 -> 0.061 ms, is its arithmetic: the measured gain of the staging is within noise)
__device__ __forceinline__ void stage_copy_rows(const ChanCopy &cc, int P, int R, float *lds) {
    if (!cc.on) return;
    for (int i = threadIdx.x; i < 3 * P * R; i += blockDim.x) {
        const int c = i % R, k = (i / R) % 3;
        const CopyRows &S = cc.c[i / (3 * R)];
        float v = 0.f;
        if (S.deg0 && (k == 0 || S.att_src_at)) v = S.bias[(k == 0 ? 0 : k == 1 ? S.att_src_at : S.att_dst_at) + c];
        lds[i] = v;
    }
    __syncthreads();
}

// Channel value of node n at columns c4 .. c4 + 3, as every fusion kernel reads it (sl: the lane's place among the lanes of
// the node, 4 columns each; c4 = 4 sl, or 0 past the row's end): the stack entry (`row` = the node's stack row at the
// channel's column), or, where the last layer's aggregation left the row out (CopyRows), what short_rows + finish_row of
// agg.hip give a row whose only message is its self loop, operation for operation, so that the bits do not depend on who
// finishes the row.  GCN: fmaf(di * di, h, 0) + b.  GAT: (p h) (1 / (p + 1e-16)) + b with p = 2^(e log2(e) - round(e log2(e)))
// of the self-loop logit e.  p is 1 only for |e| < ~0.2, else 1 +- an ulp or two, so h + b would differ from the visit's
// value by up to 2 ulp OF h, which the bias can cancel down to any number of ulp of the sum.  Then the destination's relu.
// The lanes of a node take the branch together (head_sum is cross-lane).  The unwritten stack entry is never loaded.
// lone: bit p of copy_row_bits; rows: the channel's [bias | att_j | att_i][R] block of stage_copy_rows.
__device__ __forceinline__ float4 chan_value(const float *row, const CopyRows &S, const ChanCopy &cc, const float *rows, int R,
                                             bool lone, int64_t n, int c4, int sl) {
    float4 v = ld4(lone ? S.t + n * S.ld + c4 : row + c4);
    if (lone) {
        if (S.dinv) {
            const float di = S.dinv[n];
            v = fma4(di * di, v, make_float4(0.f, 0.f, 0.f, 0.f));
        } else if (S.att_src_at) {
            const int lane = (int)threadIdx.x % kWave, F4 = S.F / 4, pos = sl % F4;
            const bool pow2 = (F4 & (F4 - 1)) == 0;
            const float a_d = head_sum<0>(dot4(v, ld4(rows + 2 * R + c4)), lane, pos, F4, pow2);
            const float a = head_sum<0>(dot4(v, ld4(rows + R + c4)), lane, pos, F4, pow2);
            Soft st;
            st.init();
            st.push(leaky(a + a_d, cc.neg_slope), v);
            v = scale4(st.acc, 1.0f / (st.s + 1e-16f));
        }
        v = add4(v, ld4(rows + c4));
        if (cc.relu) v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
    }
    return v;
}

__device__ __forceinline__ float log_sigmoid_ref(float d) {
    // the reference takes sigmoid then log in fp32 with no clamp (may give -inf); keep that
    return logf(1.0f / (1.0f + expf(-d)));
}

// The MLP scorer of one user for rank_one_user: stage_mlp's weights in LDS and, at the reference's repr_dim R == 16, the
// user's row in registers (same arithmetic, same order as mlp_score).
struct MlpScorer {
    const float *repr, *w1, *b1, *w2;
    float b2;
    int R;
    int64_t u;
    float4 ur[4];
    __device__ __forceinline__ MlpScorer(const float *repr_, int64_t u_, int R_, float b2_)
        : repr(repr_), w1(smem), b1(smem + 2 * R_ * R_), w2(smem + 2 * R_ * R_ + R_), b2(b2_), R(R_), u(u_) {
        if (R == 16) load_row<4>(repr + u * R, ur);
    }
    __device__ __forceinline__ float operator()(int64_t i) const {
        if (R == 16) {
            float4 ir[4];
            load_row<4>(repr + i * R, ir);
            return mlp_score_reg<4>(ur, ir, w1, b1, w2, b2);
        }
        return mlp_score(repr + u * R, repr + i * R, R, w1, b1, w2, b2);
    }
};

// One wave ranks one user: lanes score the C candidates 64 per pass (candidate 0 is the positive), then rank / auc / loss
// by wave reductions in a fixed order.  score(i) is the user's score of node i; ids(base, c) is the id of candidate c in
// the pass that starts at `base`; `orow` is the user's row in the outputs (each optional).
template <class Scorer, class Ids>
__device__ __forceinline__ void rank_one_user(const Scorer &score, const Ids &ids, int C, int64_t N, int lane, int64_t orow,
                                              float *scores, int32_t *rank, float *auc, float *loss, int *err) {
    float pos = 0.f;
    int higher = 0, gt = 0;
    float lsum = 0.f;
    for (int base = 0; base < C; base += kWave) {
        const int c = base + lane;
        float sc = 0.f;
        bool ok = c < C;
        if (ok) {
            const int64_t i = ids(base, c);
            if (i < 0 || i >= N) {
                atomicOr(err, 1);
                ok = false;
            } else {
                sc = score(i);
                if (scores) scores[orow * C + c] = sc;
            }
        }
        if (base == 0) pos = __shfl(sc, 0);
        if (ok && c > 0) {
            // torch.sort(descending) places a negative ahead of the positive only if it scores strictly
            // higher (stable order keeps index 0 first among ties)
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

// One online-softmax step of the channel fusion (channel order).
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

// the channel logit x_p . att_p of the fusion: per-lane partial, then the G-lane butterfly
template <int G>
__device__ __forceinline__ float chan_logit(const float4 &x, const float4 &a, bool in_row) {
    float sc = in_row ? (x.x * a.x + x.y * a.y) + (x.z * a.z + x.w * a.w) : 0.f;
#pragma unroll
    for (int off = 1; off < G; off <<= 1) sc += __shfl_xor(sc, off);
    return sc;
}

}  // namespace
}  // namespace pea
#endif  // PEA_SCORE_COMMON_H_
