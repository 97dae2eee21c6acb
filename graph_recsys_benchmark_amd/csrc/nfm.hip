// NFM (reference models/nfm.py over torchfm's NeuralFactorizationMachineModel; the torchfm arithmetic is [recalled], see
// include/peahip_fm.h) for gfx950: the training step of a batch of labelled pairs, the eval-mode fold of the two batch
// normalisations into the first linear layer, and the eval-mode pair scorer.
//   c = 0.5 ((e_u + e_i)^2 - (e_u^2 + e_i^2))   a = keep1 s BN1(c)   h = a W1^T + b1   r = keep2 s relu(BN2(h))
//   y = (lin[u] + lin[U + i] + bias0) + (r . w2 + b2)   pred = sigmoid(y)   loss = mean((pred - label)^2)
// Both batch normalisations need column statistics of the WHOLE batch, forward and backward, so the step is a chain of
// launches and every dependency between workgroups is a kernel boundary (no cooperative launch, no flag, no spin):
//   1 nfm_c_kernel      gather, c -> workspace, per-workgroup (mean, M2, n) of c's columns
//   . nfm_stats_kernel  batch mean / biased variance of BN1 from the partials, running buffers updated
//   2 nfm_h_kernel      a -> LDS, h = a W1^T + b1 on MFMA (rows_times_wt on the RAW [H, E] image, as herec.hip multiplies)
//                       -> workspace, per-workgroup (mean, M2, n) of h's columns
//   . nfm_stats_kernel  the same for BN2
//   3 nfm_out_kernel    BN2, relu, mask, y, pred, the loss terms, gy = d loss / d y; partial dw2, dgamma2, dbeta2
//   . nfm_head_final    loss, dw2, db2, dbias0, dgamma2, dbeta2 (the last two ARE the two column sums BN2's backward needs)
//   4 nfm_bwd_kernel    dh (BN2 backward), dW1 on accumulator-resident tiles (dw_store), db1, da = dh W1 on MFMA, masked
//                       -> workspace, partial dgamma1, dbeta1 (the two sums of BN1's backward)
//   . nfm_w_final       dW1, db1, dgamma1, dbeta1
//   5 nfm_rows_kernel   dc (BN1 backward), the position rows [dc (.) e_i | gy 0 0 0] and [dc (.) e_u | gy 0 0 0]
// Variance: a workgroup takes the mean of each 16-row tile first and the squared deviations from it second (the tile is in
// LDS), merges its tiles by Chan's update, and the finals merge the workgroups' (n, mean, M2) the same way: no E[x^2] -
// E[x]^2 anywhere, so a column whose mean is large against its spread keeps its digits.
// Every partial set is added in workgroup order (ordered_sum or a loop in index order), tiles in the workgroup's fixed
// order (blockIdx.x, + gridDim.x, ...), rows of a tile in row order: no float atomics, grids = f(B), bitwise reproducible,
// 64-bit row indexing.  A pair with u outside [0, U) or i outside [0, I) sets the error flag; nothing is read or written
// through it (its c row is zero, its lin terms are zero, its position rows are zero).  BN couples all rows, so the other
// numbers of such a call are unspecified, but finite.
//
// What is supported (supported() below), and why the rest is not:
//   * E and H multiples of 4 in 4..128: 16-byte row accesses; one statistics thread per column of a 256-thread workgroup
//     takes E + H <= 256; dW1 is ceil16(H) / 16 x ceil16(E) / 16 <= 64 tiles = 16 accumulator tiles per wave (64 registers);
//   * the raw W1 image [ceil16(H)][ceil16(E) + 4] and the tile's rows resident in kLdsBudget: (128, 128) takes 93,184 bytes
//     in nfm_bwd_kernel and 103,680 in nfm_score_kernel (64 staged pairs), the largest; the bound is checked all the same;
//   * 2 <= B <= 8192: torch's BatchNorm refuses one row in training mode, and the 2 B positions go back through
//     pea_rows_scatter_sum (16384 keys sorted in LDS).
#include <algorithm>

#include "../../include/peahip_fm.h"
#include "nfm_tile.h"
#include "tile16.h"
#include "train_common.h"

namespace pea {
namespace {

constexpr int kMaxWg = 128;                   // partials per set: what a final adds in order
constexpr int kScoreMaxWg = 1024;
constexpr int64_t kMaxBatch = 8192;

size_t bwd_lds_bytes(int E, int H) {
    const int ep = ceil16(E), hp = ceil16(H);
    return sizeof(float) * ((size_t)hp * (ep + 4) + 2 * (size_t)kTR * (ep + 4) + (size_t)kTR * (hp + 4) + 64);
}

// the scorer: the folded image, 64 staged pairs, the waves' partial dots, the pairs' ids
size_t score_lds_bytes(int E, int H) {
    const int ep = ceil16(E), hp = ceil16(H);
    return sizeof(float) * ((size_t)hp * (ep + 4) + (size_t)64 * (ep + 4) + 4 * 64) + 2 * 64 * 8 + 64 * 4;
}

bool supported(int E, int H) {
    if (E < 4 || E > 128 || E % 4 != 0 || H < 4 || H > 128 || H % 4 != 0) return false;
    if (tiles_per_wave((ceil16(E) / 16) * (ceil16(H) / 16)) > 16) return false;
    return bwd_lds_bytes(E, H) <= kLdsBudget && score_lds_bytes(E, H) <= kLdsBudget;
}

struct NfArgs {
    int64_t B, U, I, ld_emb;
    int E, H, EP, HP, LDE, LDH;
    float scale, eps, inv_b;
    const float *emb, *lin, *bias0, *g1, *be1, *w1, *b1, *g2, *be2, *w2, *b2;
    const int64_t *uid, *iid;
    const float *label;
    const unsigned char *keep1, *keep2;       // [B, E], [B, H] or null
    float *mean1, *var1, *mean2, *var2;       // the batch statistics (outputs, read back by the later launches)
    float *pred;
    float *dg1, *dbe1, *dg2, *dbe2;           // outputs, read back by the backward launches
    float *rows;                              // [2B, E + 4]
    int64_t *pos;                             // [2B] or null: the table rows of the 2B positions, -1 for a bad pair
    float *cbuf, *hbuf, *dabuf, *gybuf;       // [B, E], [B, H], [B, E], [B]
    float *p1, *p2, *p3, *p4, *pw;            // the partial sets
    int *err;
};

extern __shared__ __attribute__((aligned(16))) float nf_smem[];

__device__ __forceinline__ int tile_rows(int64_t T, int64_t B) { return B - T * kTR < kTR ? (int)(B - T * kTR) : kTR; }

// one column of a tile of k rows into the running (n, mean, M2): the tile's mean first, its squared deviations second
__device__ __forceinline__ void tile_stats(const float *col, int ld, int k, float &n, float &mean, float &m2) {
    if (k <= 0) return;
    float s = 0.f;
    for (int rr = 0; rr < k; ++rr) s += col[rr * ld];
    const float mt = s / (float)k;
    float q = 0.f;
    for (int rr = 0; rr < k; ++rr) {
        const float d = col[rr * ld] - mt;
        q += d * d;
    }
    const float nn = n + (float)k, delta = mt - mean;
    mean += delta * ((float)k / nn);
    m2 += q + (delta * delta) * (n * (float)k / nn);
    n = nn;
}

// <p, q> over D columns: eight fma chains (column c in chain c % 8), added pairwise (herec.hip's dot8)
__device__ __forceinline__ float dot8(const float *p, const float *q, int D) {
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < D; c += 8) {
        const float4 x = ld4(p + c), y = ld4(q + c);
        a[0] = fmaf(x.x, y.x, a[0]); a[1] = fmaf(x.y, y.y, a[1]); a[2] = fmaf(x.z, y.z, a[2]); a[3] = fmaf(x.w, y.w, a[3]);
        if (c + 4 < D) {
            const float4 z = ld4(p + c + 4), w = ld4(q + c + 4);
            a[4] = fmaf(z.x, w.x, a[4]); a[5] = fmaf(z.y, w.y, a[5]); a[6] = fmaf(z.z, w.z, a[6]); a[7] = fmaf(z.w, w.w, a[7]);
        }
    }
    return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}

__device__ __forceinline__ float4 keep4(const unsigned char *keep, int64_t at, float scale) {
    if (!keep) return make_float4(1.f, 1.f, 1.f, 1.f);
    const unsigned char *k = keep + at;
    return make_float4(k[0] ? scale : 0.f, k[1] ? scale : 0.f, k[2] ? scale : 0.f, k[3] ? scale : 0.f);
}

__device__ __forceinline__ float rstd_of(float var, float eps) { return 1.0f / sqrtf(var + eps); }

// c of one pair, four columns: torchfm's FactorizationMachine(reduce_sum=False) as it writes it
__device__ __forceinline__ float4 fm_cross(float4 u, float4 i) {
    auto f = [](float a, float b) { return 0.5f * ((a + b) * (a + b) - (a * a + b * b)); };
    return make_float4(f(u.x, i.x), f(u.y, i.y), f(u.z, i.z), f(u.w, i.w));
}

// a = keep1 s (((c - mean1) rstd1) gamma1 + beta1) of row p, columns c .. c + 3; xh: (c - mean1) rstd1
__device__ __forceinline__ float4 bn1_row(const NfArgs &a, int64_t p, int c, float4 *xh) {
    const float4 x = ld4(a.cbuf + p * a.E + c), m = ld4(a.mean1 + c), v = ld4(a.var1 + c), g = ld4(a.g1 + c), b = ld4(a.be1 + c);
    const float4 k = keep4(a.keep1, p * a.E + c, a.scale);
    const float4 h = make_float4((x.x - m.x) * rstd_of(v.x, a.eps), (x.y - m.y) * rstd_of(v.y, a.eps), (x.z - m.z) * rstd_of(v.z, a.eps),
                                 (x.w - m.w) * rstd_of(v.w, a.eps));
    if (xh) *xh = h;
    return make_float4((h.x * g.x + b.x) * k.x, (h.y * g.y + b.y) * k.y, (h.z * g.z + b.z) * k.z, (h.w * g.w + b.w) * k.w);
}

// BN2, relu and mask of row p, columns c .. c + 3: r, and hn = (h - mean2) rstd2
__device__ __forceinline__ float4 bn2_row(const NfArgs &a, int64_t p, int c, float4 *hn) {
    const float4 x = ld4(a.hbuf + p * a.H + c), m = ld4(a.mean2 + c), v = ld4(a.var2 + c), g = ld4(a.g2 + c), b = ld4(a.be2 + c);
    const float4 k = keep4(a.keep2, p * a.H + c, a.scale);
    const float4 h = make_float4((x.x - m.x) * rstd_of(v.x, a.eps), (x.y - m.y) * rstd_of(v.y, a.eps), (x.z - m.z) * rstd_of(v.z, a.eps),
                                 (x.w - m.w) * rstd_of(v.w, a.eps));
    *hn = h;
    return make_float4(fmaxf(h.x * g.x + b.x, 0.f) * k.x, fmaxf(h.y * g.y + b.y, 0.f) * k.y, fmaxf(h.z * g.z + b.z, 0.f) * k.z,
                       fmaxf(h.w * g.w + b.w, 0.f) * k.w);
}

// ---------------------------------------------------------------------------------------------- 1: c and its statistics
__global__ __launch_bounds__(kThreads) void nfm_c_kernel(const NfArgs a) {
    const int LD = a.LDE, E = a.E, e4 = E / 4;
    float *Ct = nf_smem;                                         // [16][LD]
    int64_t *ids = reinterpret_cast<int64_t *>(Ct + kTR * LD);   // [2][16]: the emb rows u and U + i
    int *valid = reinterpret_cast<int *>(ids + 2 * kTR);
    const int64_t n_tiles = (a.B + kTR - 1) / kTR;
    float n = 0.f, mean = 0.f, m2 = 0.f;
    for (int64_t T = blockIdx.x; T < n_tiles; T += gridDim.x) {
        __syncthreads();
        if (threadIdx.x < kTR) {
            const int64_t p = T * kTR + threadIdx.x;
            int64_t u = 0, it = 0;
            bool ok = p < a.B;
            if (ok) {
                u = a.uid[p];
                it = a.iid[p];
                ok = u >= 0 && u < a.U && it >= 0 && it < a.I;
                if (!ok) atomicOr(a.err, 1);
            }
            valid[threadIdx.x] = ok ? 1 : 0;
            ids[threadIdx.x] = ok ? u : 0;
            ids[kTR + threadIdx.x] = ok ? a.U + it : 0;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < kTR * e4; i += kThreads) {
            const int rr = i / e4, c = 4 * (i - rr * e4);
            const int64_t p = T * kTR + rr;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid[rr]) v = fm_cross(ld4(a.emb + ids[rr] * a.ld_emb + c), ld4(a.emb + ids[kTR + rr] * a.ld_emb + c));
            st4(Ct + rr * LD + c, v);
            if (p < a.B) st4(a.cbuf + p * E + c, v);
        }
        __syncthreads();
        if (threadIdx.x < E) tile_stats(Ct + threadIdx.x, LD, tile_rows(T, a.B), n, mean, m2);
    }
    if (threadIdx.x < E) {
        a.p1[(size_t)blockIdx.x * 3 * E + threadIdx.x] = mean;
        a.p1[(size_t)blockIdx.x * 3 * E + E + threadIdx.x] = m2;
        a.p1[(size_t)blockIdx.x * 3 * E + 2 * E + threadIdx.x] = n;
    }
}

// batch mean and biased variance of C columns from the workgroups' (mean, M2, n) in workgroup order (Chan's merge against the
// batch mean); the running buffers take mean and the unbiased variance with `momentum` when given
__global__ __launch_bounds__(128) void nfm_stats_kernel(int n_wg, int64_t B, int C, const float *__restrict__ part, float *bmean,
                                                        float *bvar, float *run_mean, float *run_var, float momentum) {
    const int col = blockIdx.x * 128 + threadIdx.x;
    if (col >= C) return;
    const float *pm = part + col, *pq = part + C + col, *pn = part + 2 * C + col;
    const size_t stride = 3 * (size_t)C;
    float s = 0.f;
#pragma unroll 8
    for (int w = 0; w < n_wg; ++w) s += pn[w * stride] * pm[w * stride];
    const float mean = s / (float)B;
    float q = 0.f;
#pragma unroll 8
    for (int w = 0; w < n_wg; ++w) {
        const float d = pm[w * stride] - mean;
        q += pq[w * stride] + pn[w * stride] * (d * d);
    }
    const float var = q / (float)B;
    bmean[col] = mean;
    bvar[col] = var;
    if (run_mean) {
        run_mean[col] = (1.0f - momentum) * run_mean[col] + momentum * mean;
        run_var[col] = (1.0f - momentum) * run_var[col] + momentum * (q / (float)(B - 1));
    }
}

// ---------------------------------------------------------------------------------------------- 2: a, h and its statistics
__global__ __launch_bounds__(kThreads) void nfm_h_kernel(const NfArgs a) {
    const int LDE = a.LDE, LDH = a.LDH, E = a.E, H = a.H, e4 = E / 4;
    float *Ws = nf_smem;                          // [HP][LDE] raw W1: row = output, column = input
    float *At = Ws + (size_t)a.HP * LDE;          // [16][LDE]
    float *Ht = At + kTR * LDE;                   // [16][LDH]
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, n = lane & 15, g = lane >> 4;
    const int64_t n_tiles = (a.B + kTR - 1) / kTR;
    const int HT = a.HP / 16;
    for (int i = threadIdx.x; i < kTR * LDE; i += kThreads) At[i] = 0.f;      // the pad columns stay zero
    for (int i = threadIdx.x; i < kTR * LDH; i += kThreads) Ht[i] = 0.f;
    stage_weight<4>(a.w1, H, E, 0, Ws, a.HP, a.EP, LDE);
    float cn = 0.f, mean = 0.f, m2 = 0.f;
    for (int64_t T = blockIdx.x; T < n_tiles; T += gridDim.x) {
        __syncthreads();
        for (int i = threadIdx.x; i < kTR * e4; i += kThreads) {
            const int rr = i / e4, c = 4 * (i - rr * e4);
            const int64_t p = T * kTR + rr;
            st4(At + rr * LDE + c, p < a.B ? bn1_row(a, p, c, nullptr) : make_float4(0.f, 0.f, 0.f, 0.f));
        }
        __syncthreads();
        for (int v = wave; v < HT; v += kWaves) {
            f32x4 z[1] = {};
            rows_times_wt<1, 1>(Ws, a.HP, LDE, At, LDE, e4, v, n, g, z);
            const int col = 16 * v + 4 * g;
            if (col >= H) continue;
            const float4 bv = ld4(a.b1 + col);
            const float4 h = make_float4(z[0][0] + bv.x, z[0][1] + bv.y, z[0][2] + bv.z, z[0][3] + bv.w);
            const int64_t p = T * kTR + n;
            st4(Ht + n * LDH + col, h);
            if (p < a.B) st4(a.hbuf + p * H + col, h);
        }
        __syncthreads();
        if (threadIdx.x < H) tile_stats(Ht + threadIdx.x, LDH, tile_rows(T, a.B), cn, mean, m2);
    }
    if (threadIdx.x < H) {
        a.p2[(size_t)blockIdx.x * 3 * H + threadIdx.x] = mean;
        a.p2[(size_t)blockIdx.x * 3 * H + H + threadIdx.x] = m2;
        a.p2[(size_t)blockIdx.x * 3 * H + 2 * H + threadIdx.x] = cn;
    }
}

// ---------------------------------------------------------------------------------------------- 3: the head
template <bool BWD>
__global__ __launch_bounds__(kThreads) void nfm_out_kernel(const NfArgs a) {
    const int LDH = a.LDH, H = a.H, h4 = H / 4;
    float *Rt = nf_smem;                          // [16][LDH] r
    float *Hn = Rt + kTR * LDH;                   // [16][LDH] (h - mean2) rstd2
    float *gyl = Hn + kTR * LDH, *term = gyl + kTR;
    const int64_t n_tiles = (a.B + kTR - 1) / kTR;
    float dw2 = 0.f, dg = 0.f, db = 0.f, wg_loss = 0.f, wg_gy = 0.f;
    for (int64_t T = blockIdx.x; T < n_tiles; T += gridDim.x) {
        __syncthreads();
        for (int i = threadIdx.x; i < kTR * h4; i += kThreads) {
            const int rr = i / h4, c = 4 * (i - rr * h4);
            const int64_t p = T * kTR + rr;
            float4 r = make_float4(0.f, 0.f, 0.f, 0.f), hn = r;
            if (p < a.B) r = bn2_row(a, p, c, &hn);
            st4(Rt + rr * LDH + c, r);
            st4(Hn + rr * LDH + c, hn);
        }
        __syncthreads();
        if (threadIdx.x < kTR) {
            const int64_t p = T * kTR + threadIdx.x;
            float t = 0.f, gy = 0.f;
            if (p < a.B) {
                const int64_t u = a.uid[p], it = a.iid[p];
                const bool ok = u >= 0 && u < a.U && it >= 0 && it < a.I;
                const float lu = ok ? a.lin[u] : 0.f, li = ok ? a.lin[a.U + it] : 0.f;
                const float y = ((lu + li) + a.bias0[0]) + (dot8(Rt + threadIdx.x * LDH, a.w2, H) + a.b2[0]);
                const float pr = 1.0f / (1.0f + expf(-y));
                const float d = pr - a.label[p];
                t = d * d;
                gy = (2.0f * d * a.inv_b) * (pr * (1.0f - pr));
                a.pred[p] = pr;
                if (BWD) a.gybuf[p] = gy;
            }
            term[threadIdx.x] = t;
            gyl[threadIdx.x] = gy;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            float s = 0.f, q = 0.f;
            for (int k = 0; k < kTR; ++k) {
                s += term[k];
                q += gyl[k];
            }
            wg_loss += s;
            wg_gy += q;
        }
        if (BWD && threadIdx.x < H) {
            const float w = a.w2[threadIdx.x];
            const int k = tile_rows(T, a.B);
            for (int rr = 0; rr < k; ++rr) {
                const float r = Rt[rr * LDH + threadIdx.x];
                const float keep = a.keep2 ? (a.keep2[(T * kTR + rr) * H + threadIdx.x] ? a.scale : 0.f) : 1.f;
                const float dz = r > 0.f ? (gyl[rr] * w) * keep : 0.f;
                dw2 += gyl[rr] * r;
                db += dz;
                dg += dz * Hn[rr * LDH + threadIdx.x];
            }
        }
    }
    float *out = a.p3 + (size_t)blockIdx.x * (3 * H + 2);
    if (threadIdx.x == 0) {
        out[3 * H] = wg_loss;
        out[3 * H + 1] = wg_gy;
    }
    if (BWD && threadIdx.x < H) {
        out[threadIdx.x] = dw2;
        out[H + threadIdx.x] = dg;
        out[2 * H + threadIdx.x] = db;
    }
}

__global__ __launch_bounds__(128) void nfm_head_final(int n_wg, int64_t B, int H, const float *__restrict__ part, float *loss, float *dw2,
                                                      float *dg2, float *dbe2, float *db2, float *dbias0) {
    const int e = blockIdx.x * 128 + threadIdx.x;
    const size_t stride = 3 * H + 2;
    if (e == 3 * H) loss[0] = ordered_sum(part + e, stride, n_wg) / (float)B;
    if (!dw2 || e > 3 * H + 1) return;
    if (e == 3 * H + 1) {
        const float s = ordered_sum(part + e, stride, n_wg);
        db2[0] = s;
        dbias0[0] = s;
        dbias0[1] = dbias0[2] = 0.f;      // the two pad floats of d_dense behind them
    } else if (e < 3 * H) {
        const float s = ordered_sum(part + e, stride, n_wg);
        if (e < H) dw2[e] = s;
        else if (e < 2 * H) dg2[e - H] = s;
        else dbe2[e - 2 * H] = s;
    }
}

// ---------------------------------------------------------------------------------------------- 4: dh, dW1, db1, da
template <int NT>
__global__ __launch_bounds__(kThreads) void nfm_bwd_kernel(const NfArgs a) {
    const int LDE = a.LDE, LDH = a.LDH, E = a.E, H = a.H, e4 = E / 4, h4 = H / 4;
    float *Ws = nf_smem;                          // [HP][LDE] raw W1
    float *At = Ws + (size_t)a.HP * LDE;          // [16][LDE] a: the B operand of dW1
    float *Da = At + kTR * LDE;                   // [16][LDE] the masked da
    float *Dh = Da + kTR * LDE;                   // [16][LDH] dh: the A operand of dW1
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, n = lane & 15, g = lane >> 4;
    const int64_t n_tiles = (a.B + kTR - 1) / kTR;
    const int HT = a.HP / 16, ET = a.EP / 16;
    for (int i = threadIdx.x; i < 2 * kTR * LDE + kTR * LDH; i += kThreads) At[i] = 0.f;      // the pad columns stay zero
    stage_weight<4>(a.w1, H, E, 0, Ws, a.HP, a.EP, LDE);
    f32x4 dw[1][NT] = {};
    float db1 = 0.f, dg1 = 0.f, dbe1 = 0.f;
    for (int64_t T = blockIdx.x; T < n_tiles; T += gridDim.x) {
        __syncthreads();
        for (int i = threadIdx.x; i < kTR * e4; i += kThreads) {
            const int rr = i / e4, c = 4 * (i - rr * e4);
            const int64_t p = T * kTR + rr;
            st4(At + rr * LDE + c, p < a.B ? bn1_row(a, p, c, nullptr) : make_float4(0.f, 0.f, 0.f, 0.f));
        }
        // dh = ((dz - dbeta2 / B) - hn (dgamma2 / B)) rstd2 gamma2, dz = the masked relu gradient of gy w2
        for (int i = threadIdx.x; i < kTR * h4; i += kThreads) {
            const int rr = i / h4, c = 4 * (i - rr * h4);
            const int64_t p = T * kTR + rr;
            float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p < a.B) {
                float4 hn;
                const float4 r = bn2_row(a, p, c, &hn);
                const float4 k = keep4(a.keep2, p * H + c, a.scale), w = ld4(a.w2 + c), sg = ld4(a.dg2 + c), sb = ld4(a.dbe2 + c);
                const float4 v = ld4(a.var2 + c), gm = ld4(a.g2 + c);
                const float gy = a.gybuf[p];
                auto f = [&](float r_, float k_, float w_, float hn_, float sg_, float sb_, float v_, float gm_) {
                    const float dz = r_ > 0.f ? (gy * w_) * k_ : 0.f;
                    return (((dz - sb_ * a.inv_b) - hn_ * (sg_ * a.inv_b)) * rstd_of(v_, a.eps)) * gm_;
                };
                d = make_float4(f(r.x, k.x, w.x, hn.x, sg.x, sb.x, v.x, gm.x), f(r.y, k.y, w.y, hn.y, sg.y, sb.y, v.y, gm.y),
                                f(r.z, k.z, w.z, hn.z, sg.z, sb.z, v.z, gm.z), f(r.w, k.w, w.w, hn.w, sg.w, sb.w, v.w, gm.w));
            }
            st4(Dh + rr * LDH + c, d);
        }
        __syncthreads();
        if (threadIdx.x < H) {
            for (int rr = 0; rr < kTR; ++rr) db1 += Dh[rr * LDH + threadIdx.x];
        }
        // dW1 += dh^T a over the tile's 16 rows (4 k-steps): register r of lane (n, g) = dW1[16 v + 4 g + r][16 u + n]
#pragma unroll
        for (int q = 0; q < NT; ++q) {
            const int id = wave + kWaves * q;
            if (id >= HT * ET) continue;
            const int v = id / ET, u = id - v * ET;
            const int zo = g * LDH + 16 * v + n, xo = g * LDE + 16 * u + n;
#pragma unroll
            for (int t = 0; t < kTR / 4; ++t)
                dw[0][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(Dh[zo + 4 * t * LDH], At[xo + 4 * t * LDE], dw[0][q], 0, 0, 0);
        }
        // da = dh W1 (k = the image's rows), masked like a
        for (int u = wave; u < ET; u += kWaves) {
            f32x4 z[1] = {};
            rows_times_w<1, 1>(Ws, a.HP, LDE, Dh, LDH, h4, u, n, g, z);
            const int col = 16 * u + 4 * g;
            const int64_t p = T * kTR + n;
            if (col >= E) continue;
            float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p < a.B) {
                const float4 k = keep4(a.keep1, p * E + col, a.scale);
                d = make_float4(z[0][0] * k.x, z[0][1] * k.y, z[0][2] * k.z, z[0][3] * k.w);
                st4(a.dabuf + p * E + col, d);
            }
            st4(Da + n * LDE + col, d);
        }
        __syncthreads();
        if (threadIdx.x < E) {
            const int k = tile_rows(T, a.B);
            const float m = a.mean1[threadIdx.x], rs = rstd_of(a.var1[threadIdx.x], a.eps);
            for (int rr = 0; rr < k; ++rr) {
                const float d = Da[rr * LDE + threadIdx.x];
                dbe1 += d;
                dg1 += d * ((a.cbuf[(T * kTR + rr) * E + threadIdx.x] - m) * rs);
            }
        }
    }
    float *out = a.p4 + (size_t)blockIdx.x * (H + 2 * E);
    if (threadIdx.x < H) out[threadIdx.x] = db1;
    if (threadIdx.x < E) {
        out[H + threadIdx.x] = dg1;
        out[H + E + threadIdx.x] = dbe1;
    }
    dw_store<NT, 1>(dw, a.pw + (size_t)blockIdx.x * H * E, (size_t)H * E, H, E, 0, HT, ET, wave, n, g);
}

__global__ __launch_bounds__(256) void nfm_w_final(int n_wg, int E, int H, const float *__restrict__ pw, const float *__restrict__ p4,
                                                   float *dw1, float *db1, float *dg1, float *dbe1) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, wsz = (size_t)H * E, vsz = (size_t)H + 2 * E;
    if (e < wsz) {
        dw1[e] = ordered_sum(pw + e, wsz, n_wg);
    } else if (e < wsz + vsz) {
        const size_t k = e - wsz;
        const float s = ordered_sum(p4 + k, vsz, n_wg);
        if (k < (size_t)H) db1[k] = s;
        else if (k < (size_t)H + E) dg1[k - H] = s;
        else dbe1[k - H - E] = s;
    }
}

// ---------------------------------------------------------------------------------------------- 5: dc and the position rows
__global__ __launch_bounds__(kThreads) void nfm_rows_kernel(const NfArgs a) {
    const int E = a.E, e4 = E / 4, W = E + 4;
    const int64_t T = blockIdx.x;
    for (int i = threadIdx.x; i < kTR * (e4 + 1); i += kThreads) {
        const int rr = i / (e4 + 1), j = i - rr * (e4 + 1), c = 4 * j;
        const int64_t p = T * kTR + rr;
        if (p >= a.B) continue;
        const int64_t u = a.uid[p], it = a.iid[p];
        const bool ok = u >= 0 && u < a.U && it >= 0 && it < a.I;
        float4 ru = make_float4(0.f, 0.f, 0.f, 0.f), ri = ru;
        if (j == e4 && a.pos) {
            a.pos[p] = ok ? u : -1;
            a.pos[a.B + p] = ok ? a.U + it : -1;
        }
        if (ok && j == e4) {
            ru = ri = make_float4(a.gybuf[p], 0.f, 0.f, 0.f);
        } else if (ok) {
            const float4 x = ld4(a.cbuf + p * E + c), m = ld4(a.mean1 + c), v = ld4(a.var1 + c), gm = ld4(a.g1 + c);
            const float4 d = ld4(a.dabuf + p * E + c), sg = ld4(a.dg1 + c), sb = ld4(a.dbe1 + c);
            const float4 eu = ld4(a.emb + u * a.ld_emb + c), ei = ld4(a.emb + (a.U + it) * a.ld_emb + c);
            auto f = [&](float x_, float m_, float v_, float gm_, float d_, float sg_, float sb_) {
                const float rs = rstd_of(v_, a.eps);
                return (((d_ - sb_ * a.inv_b) - ((x_ - m_) * rs) * (sg_ * a.inv_b)) * rs) * gm_;
            };
            const float4 dc = make_float4(f(x.x, m.x, v.x, gm.x, d.x, sg.x, sb.x), f(x.y, m.y, v.y, gm.y, d.y, sg.y, sb.y),
                                          f(x.z, m.z, v.z, gm.z, d.z, sg.z, sb.z), f(x.w, m.w, v.w, gm.w, d.w, sg.w, sb.w));
            ru = make_float4(dc.x * ei.x, dc.y * ei.y, dc.z * ei.z, dc.w * ei.w);
            ri = make_float4(dc.x * eu.x, dc.y * eu.y, dc.z * eu.z, dc.w * eu.w);
        }
        st4(a.rows + p * W + c, ru);
        st4(a.rows + (a.B + p) * W + c, ri);
    }
}

// ---------------------------------------------------------------------------------------------- the eval-mode fold
// W'[o][e] = (s2[o] W1[o][e]) s1[e], b'[o] = s2[o] (sum_e W1[o][e] t1[e] + b1[o]) + t2[o] (e ascending), bias = bias0 + b2
__global__ __launch_bounds__(128) void nfm_fold_kernel(int E, int H, float eps, const float *__restrict__ w1, const float *__restrict__ b1,
                                                       const float *__restrict__ g1, const float *__restrict__ be1,
                                                       const float *__restrict__ rm1, const float *__restrict__ rv1,
                                                       const float *__restrict__ g2, const float *__restrict__ be2,
                                                       const float *__restrict__ rm2, const float *__restrict__ rv2,
                                                       const float *__restrict__ bias0, const float *__restrict__ b2, float *wf, float *bf,
                                                       float *bias) {
    const int o = blockIdx.x * 128 + threadIdx.x;
    if (o == 0) bias[0] = bias0[0] + b2[0];
    if (o >= H) return;
    const float s2 = g2[o] / sqrtf(rv2[o] + eps), t2 = be2[o] - rm2[o] * s2;
    float acc = 0.f;
    for (int e = 0; e < E; ++e) {
        const float s1 = g1[e] / sqrtf(rv1[e] + eps), t1 = be1[e] - rm1[e] * s1, w = w1[(size_t)o * E + e];
        wf[(size_t)o * E + e] = (s2 * w) * s1;
        acc += w * t1;
    }
    bf[o] = s2 * (acc + b1[o]) + t2;
}

// ---------------------------------------------------------------------------------------------- the eval-mode scorer
struct NsArgs {
    int64_t n_pairs, U, I, ld_emb, C, lo;
    int mode, E, H, EP, HP, LD;
    const float *emb, *lin, *wf, *bf, *w2, *bias;
    const int64_t *uid, *iid;
    float *logit, *pred;
    int *err;
};

// pair k of the three addressing forms: flat pairs, [U', C] candidate rows, [U'] x the item range [lo, lo + C)
__device__ __forceinline__ void pair_of(const NsArgs &a, int64_t k, int64_t &u, int64_t &it) {
    if (a.mode == PEA_NFM_PAIRS) {
        u = a.uid[k];
        it = a.iid[k];
    } else if (a.mode == PEA_NFM_ROWS) {
        u = a.uid[k / a.C];
        it = a.iid[k];
    } else {
        u = a.uid[k / a.C];
        it = a.lo + k % a.C;
    }
}

// One workgroup walks tiles of kSP = 64 pairs; the tile's arithmetic is nfm_tile.h's (nfm_x4, nfm_tile_dots, nfm_logit), which
// the catalogue scan of nfm_scan.hip calls too.

__global__ __launch_bounds__(kThreads) void nfm_score_kernel(const NsArgs a) {
    const int LD = a.LD, E = a.E, H = a.H, e4 = E / 4;
    float *Ws = nf_smem;                                          // [HP][LD] W'
    float *Xt = Ws + (size_t)a.HP * LD;                           // [64][LD]
    float *part = Xt + kSP * LD;                                  // [4 waves][64]
    int64_t *ids = reinterpret_cast<int64_t *>(part + kWaves * kSP);
    int *valid = reinterpret_cast<int *>(ids + 2 * kSP);
    const int64_t n_tiles = (a.n_pairs + kSP - 1) / kSP;
    for (int i = threadIdx.x; i < kSP * LD; i += kThreads) Xt[i] = 0.f;
    stage_weight<4>(a.wf, H, E, 0, Ws, a.HP, a.EP, LD);
    for (int64_t T = blockIdx.x; T < n_tiles; T += gridDim.x) {
        __syncthreads();
        if (threadIdx.x < kSP) {
            const int64_t k = T * kSP + threadIdx.x;
            int64_t u = 0, it = 0;
            bool ok = k < a.n_pairs;
            if (ok) {
                pair_of(a, k, u, it);
                ok = u >= 0 && u < a.U && it >= 0 && it < a.I;
                if (!ok) atomicOr(a.err, 1);
            }
            valid[threadIdx.x] = ok ? 1 : 0;
            ids[threadIdx.x] = ok ? u : 0;
            ids[kSP + threadIdx.x] = ok ? a.U + it : 0;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < kSP * e4; i += kThreads) {
            const int rr = i / e4, c = 4 * (i - rr * e4);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid[rr]) v = nfm_x4(ld4(a.emb + ids[rr] * a.ld_emb + c), ld4(a.emb + ids[kSP + rr] * a.ld_emb + c));
            st4(Xt + rr * LD + c, v);
        }
        __syncthreads();
        const float d = nfm_tile_dots(Ws, Xt, part, a.bf, a.w2, H, a.HP, LD, e4);
        if (threadIdx.x < kSP) {
            const int64_t k = T * kSP + threadIdx.x;
            if (k < a.n_pairs) {
                float y = 0.f;
                if (valid[threadIdx.x]) y = nfm_logit(a.lin[ids[threadIdx.x]], a.lin[ids[kSP + threadIdx.x]], a.bias[0], d);
                if (a.logit) a.logit[k] = y;
                if (a.pred) a.pred[k] = 1.0f / (1.0f + expf(-y));
            }
        }
    }
}

// rank [U'] = negatives of the row scoring strictly higher than column 0, auc = the share scoring strictly lower (0 without
// negatives): one wave per row, integer counts
__global__ __launch_bounds__(256) void nfm_rank_kernel(int64_t n_rows, int64_t C, const float *__restrict__ score, int *rank, float *auc) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const float pos = score[row * C];
    int above = 0, below = 0;
    for (int64_t j = 1 + lane; j < C; j += 64) {
        const float s = score[row * C + j];
        above += s > pos;
        below += s < pos;
    }
    for (int off = 32; off > 0; off >>= 1) {
        above += __shfl_xor(above, off);
        below += __shfl_xor(below, off);
    }
    if (lane == 0) {
        rank[row] = above;
        auc[row] = C > 1 ? (float)below / (float)(C - 1) : 0.f;
    }
}

int n_workgroups(int64_t B) { return (int)std::min<int64_t>((B + kTR - 1) / kTR, kMaxWg); }

// workspace: [flag | c | h | da | gy | p1 | p2 | p3 | p4 | pw], each part on a 256-byte boundary
struct WsLayout {
    size_t c, h, da, gy, p1, p2, p3, p4, pw, total;
};
WsLayout ws_layout(int64_t B, int E, int H) {
    const size_t g = (size_t)n_workgroups(B), f = sizeof(float);
    WsLayout l;
    size_t at = 256;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += align256(bytes);
        return here;
    };
    l.c = take((size_t)B * E * f);
    l.h = take((size_t)B * H * f);
    l.da = take((size_t)B * E * f);
    l.gy = take((size_t)B * f);
    l.p1 = take(g * 3 * E * f);
    l.p2 = take(g * 3 * H * f);
    l.p3 = take(g * (3 * H + 2) * f);
    l.p4 = take(g * (H + 2 * E) * f);
    l.pw = take(g * (size_t)H * E * f);
    l.total = at;
    return l;
}

template <int NT>
int launch_bwd(const NfArgs &a, int n_wg, size_t lds, hipStream_t stream) {
    PEA_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(&nfm_bwd_kernel<NT>), lds_limit(lds)));
    PEA_LAUNCH((nfm_bwd_kernel<NT>), dim3(n_wg), dim3(kThreads), lds, stream, a);
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}

}  // namespace
}  // namespace pea

using namespace pea;

extern "C" int pea_nfm_supported(int E, int H) { return supported(E, H) ? 1 : 0; }

extern "C" size_t pea_nfm_train_workspace_bytes(int64_t B, int E, int H) {
    if (!supported(E, H) || B < 2 || B > kMaxBatch) return 0;
    return ws_layout(B, E, H).total;
}

extern "C" int pea_nfm_train(int64_t B, int E, int H, int64_t num_users, int64_t num_items, const float *emb, int64_t ld_emb,
                             const float *lin, const float *bias0, const float *bn1_w, const float *bn1_b, float *bn1_mean,
                             float *bn1_var, const float *w1, const float *b1, const float *bn2_w, const float *bn2_b,
                             float *bn2_mean, float *bn2_var, const float *w2, const float *b2, float eps, float momentum,
                             int update_running, const int64_t *uids, const int64_t *iids, const float *labels,
                             const unsigned char *keep1, const unsigned char *keep2, float keep_scale, float *out_loss, float *pred,
                             float *batch_stats, float *d_dense, float *grad_rows, int64_t *pos_ids, void *workspace,
                             size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    PEA_REQUIRE(supported(E, H), PEA_ERR_ARG, "nfm_train: emb_dim %d with hidden_size %d is not supported (pea_nfm_supported)", E, H);
    PEA_REQUIRE(B >= 2 && B <= kMaxBatch, PEA_ERR_ARG,
                "nfm_train: %lld rows (batch normalisation needs 2 at least; the 2 B positions are scattered back: B <= %lld)",
                (long long)B, (long long)kMaxBatch);
    PEA_REQUIRE(num_users > 0 && num_items > 0, PEA_ERR_ARG, "nfm_train: %lld users and %lld items", (long long)num_users,
                (long long)num_items);
    PEA_REQUIRE(emb && lin && bias0 && bn1_w && bn1_b && w1 && b1 && bn2_w && bn2_b && w2 && b2 && uids && iids && labels && out_loss &&
                    pred && batch_stats && workspace,
                PEA_ERR_ARG, "nfm_train: null pointer");
    PEA_REQUIRE(ld_emb >= E && ld_emb % 4 == 0, PEA_ERR_ARG, "nfm_train: row stride %lld of emb (a multiple of 4, at least %d)",
                (long long)ld_emb, E);
    PEA_REQUIRE(aligned16(emb) && aligned16(bn1_w) && aligned16(bn1_b) && aligned16(w1) && aligned16(b1) && aligned16(bn2_w) &&
                    aligned16(bn2_b) && aligned16(w2) && aligned16(batch_stats) && aligned16(workspace),
                PEA_ERR_ARG, "nfm_train: emb, the dense parameters, batch_stats and the workspace must start on 16-byte boundaries");
    PEA_REQUIRE((keep1 != nullptr) == (keep2 != nullptr), PEA_ERR_ARG, "nfm_train: keep1 and keep2 are both given or both NULL");
    PEA_REQUIRE(!keep1 || (keep_scale > 0.f && keep_scale < 1e30f), PEA_ERR_ARG, "nfm_train: keep_scale %g", (double)keep_scale);
    PEA_REQUIRE(!update_running || (bn1_mean && bn1_var && bn2_mean && bn2_var), PEA_ERR_ARG,
                "nfm_train: update_running needs the four running buffers");
    const bool bwd = d_dense != nullptr;
    PEA_REQUIRE((grad_rows != nullptr) == bwd, PEA_ERR_ARG, "nfm_train: d_dense and grad_rows are both given or both NULL");
    PEA_REQUIRE(bwd || !pos_ids, PEA_ERR_ARG, "nfm_train: pos_ids comes with grad_rows");
    PEA_REQUIRE(!bwd || (aligned16(d_dense) && aligned16(grad_rows)), PEA_ERR_ARG,
                "nfm_train: d_dense and grad_rows must start on 16-byte boundaries");
    PEA_REQUIRE(workspace_bytes >= pea_nfm_train_workspace_bytes(B, E, H), PEA_ERR_NOMEM, "nfm_train: workspace too small");
    const WsLayout l = ws_layout(B, E, H);
    char *ws = (char *)workspace;
    NfArgs a = {};
    a.B = B; a.U = num_users; a.I = num_items; a.ld_emb = ld_emb;
    a.E = E; a.H = H; a.EP = ceil16(E); a.HP = ceil16(H); a.LDE = a.EP + 4; a.LDH = a.HP + 4;
    a.scale = keep1 ? keep_scale : 1.0f; a.eps = eps; a.inv_b = 1.0f / (float)B;
    a.emb = emb; a.lin = lin; a.bias0 = bias0; a.g1 = bn1_w; a.be1 = bn1_b; a.w1 = w1; a.b1 = b1; a.g2 = bn2_w; a.be2 = bn2_b;
    a.w2 = w2; a.b2 = b2; a.uid = uids; a.iid = iids; a.label = labels; a.keep1 = keep1; a.keep2 = keep2;
    a.mean1 = batch_stats; a.var1 = batch_stats + E; a.mean2 = batch_stats + 2 * E; a.var2 = batch_stats + 2 * E + H;
    a.pred = pred;
    // d_dense: [dW1 (H E) | db1 (H) | dw2 (H) | db2 | dbias0 | 0 0 | dgamma1 (E) | dbeta1 (E) | dgamma2 (H) | dbeta2 (H)]
    float *d_w1 = d_dense, *d_b1 = nullptr, *d_w2 = nullptr, *d_b2 = nullptr, *d_bias0 = nullptr;
    if (bwd) {
        d_b1 = d_w1 + (size_t)H * E; d_w2 = d_b1 + H; d_b2 = d_w2 + H; d_bias0 = d_b2 + 1;
        a.dg1 = d_b2 + 4; a.dbe1 = a.dg1 + E; a.dg2 = a.dbe1 + E; a.dbe2 = a.dg2 + H;
    }
    a.rows = grad_rows;
    a.pos = pos_ids;
    a.cbuf = (float *)(ws + l.c); a.hbuf = (float *)(ws + l.h); a.dabuf = (float *)(ws + l.da); a.gybuf = (float *)(ws + l.gy);
    a.p1 = (float *)(ws + l.p1); a.p2 = (float *)(ws + l.p2); a.p3 = (float *)(ws + l.p3); a.p4 = (float *)(ws + l.p4);
    a.pw = (float *)(ws + l.pw);
    a.err = ws_err_flag(workspace);
    PEA_MEMSET_ASYNC(a.err, 0, sizeof(int), stream);
    const int n_wg = n_workgroups(B);
    const size_t f = sizeof(float);
    {
        ProfScope ps("nfm_c", stream, (double)B * E * 4.0 * 3.0);
        PEA_LAUNCH(nfm_c_kernel, dim3(n_wg), dim3(kThreads), (size_t)kTR * a.LDE * f + 2 * kTR * 8 + kTR * 4, stream, a);
        PEA_HIP(hipGetLastError());
        PEA_LAUNCH(nfm_stats_kernel, dim3((E + 127) / 128), dim3(128), 0, stream, n_wg, B, E, (const float *)a.p1, a.mean1, a.var1,
                   update_running ? bn1_mean : (float *)nullptr, update_running ? bn1_var : (float *)nullptr, momentum);
        PEA_HIP(hipGetLastError());
    }
    {
        const size_t lds = f * ((size_t)a.HP * a.LDE + (size_t)kTR * a.LDE + (size_t)kTR * a.LDH);
        PEA_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(&nfm_h_kernel), lds_limit(lds)));
        ProfScope ps("nfm_h", stream, (double)B * (E + H) * 4.0);
        PEA_LAUNCH(nfm_h_kernel, dim3(n_wg), dim3(kThreads), lds, stream, a);
        PEA_HIP(hipGetLastError());
        PEA_LAUNCH(nfm_stats_kernel, dim3((H + 127) / 128), dim3(128), 0, stream, n_wg, B, H, (const float *)a.p2, a.mean2, a.var2,
                   update_running ? bn2_mean : (float *)nullptr, update_running ? bn2_var : (float *)nullptr, momentum);
        PEA_HIP(hipGetLastError());
    }
    {
        const size_t lds = f * (2 * (size_t)kTR * a.LDH + 2 * kTR);
        ProfScope ps("nfm_out", stream, (double)B * H * 4.0);
        if (bwd) PEA_LAUNCH(nfm_out_kernel<true>, dim3(n_wg), dim3(kThreads), lds, stream, a);
        else PEA_LAUNCH(nfm_out_kernel<false>, dim3(n_wg), dim3(kThreads), lds, stream, a);
        PEA_HIP(hipGetLastError());
        PEA_LAUNCH(nfm_head_final, dim3((3 * H + 2 + 127) / 128), dim3(128), 0, stream, n_wg, B, H, (const float *)a.p3, out_loss, d_w2,
                   a.dg2, a.dbe2, d_b2, d_bias0);
        PEA_HIP(hipGetLastError());
    }
    if (!bwd) return PEA_OK;
    {
        const size_t lds = bwd_lds_bytes(E, H);
        ProfScope ps("nfm_bwd", stream, (double)B * (2 * E + H) * 4.0);
        switch (tiles_per_wave((a.HP / 16) * (a.EP / 16))) {
            case 1: PEA_TRY(launch_bwd<1>(a, n_wg, lds, stream)); break;
            case 2: PEA_TRY(launch_bwd<2>(a, n_wg, lds, stream)); break;
            case 4: PEA_TRY(launch_bwd<4>(a, n_wg, lds, stream)); break;
            case 8: PEA_TRY(launch_bwd<8>(a, n_wg, lds, stream)); break;
            default: PEA_TRY(launch_bwd<16>(a, n_wg, lds, stream)); break;
        }
        const size_t total = (size_t)H * E + H + 2 * E;
        PEA_LAUNCH(nfm_w_final, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, n_wg, E, H, (const float *)a.pw,
                   (const float *)a.p4, d_w1, d_b1, a.dg1, a.dbe1);
        PEA_HIP(hipGetLastError());
    }
    {
        ProfScope ps("nfm_rows", stream, (double)B * E * 4.0 * 6.0);
        PEA_LAUNCH(nfm_rows_kernel, dim3((unsigned)((B + kTR - 1) / kTR)), dim3(kThreads), 0, stream, a);
        PEA_HIP(hipGetLastError());
    }
    return PEA_OK;
}

extern "C" int pea_nfm_fold(int E, int H, const float *w1, const float *b1, const float *bn1_w, const float *bn1_b, const float *bn1_mean,
                            const float *bn1_var, const float *bn2_w, const float *bn2_b, const float *bn2_mean, const float *bn2_var,
                            const float *bias0, const float *b2, float eps, float *w_fold, float *b_fold, float *bias_fold, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    PEA_REQUIRE(supported(E, H), PEA_ERR_ARG, "nfm_fold: emb_dim %d with hidden_size %d is not supported (pea_nfm_supported)", E, H);
    PEA_REQUIRE(w1 && b1 && bn1_w && bn1_b && bn1_mean && bn1_var && bn2_w && bn2_b && bn2_mean && bn2_var && bias0 && b2 && w_fold &&
                    b_fold && bias_fold,
                PEA_ERR_ARG, "nfm_fold: null pointer");
    ProfScope ps("nfm_fold", stream, (double)H * E * 8.0);
    PEA_LAUNCH(nfm_fold_kernel, dim3((H + 127) / 128), dim3(128), 0, stream, E, H, eps, w1, b1, bn1_w, bn1_b, bn1_mean, bn1_var, bn2_w,
               bn2_b, bn2_mean, bn2_var, bias0, b2, w_fold, b_fold, bias_fold);
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}

extern "C" int pea_nfm_score(int mode, int64_t n_users, int64_t C, int64_t item_lo, int E, int H, int64_t num_users, int64_t num_items,
                             const float *emb, int64_t ld_emb, const float *lin, const float *w_fold, const float *b_fold,
                             const float *w2, const float *bias_fold, const int64_t *uids, const int64_t *iids, float *logits,
                             float *pred, int *rank, float *auc, int *err_flag, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    PEA_REQUIRE(supported(E, H), PEA_ERR_ARG, "nfm_score: emb_dim %d with hidden_size %d is not supported (pea_nfm_supported)", E, H);
    PEA_REQUIRE(mode == PEA_NFM_PAIRS || mode == PEA_NFM_ROWS || mode == PEA_NFM_RANGE, PEA_ERR_ARG, "nfm_score: mode %d", mode);
    PEA_REQUIRE(n_users >= 0 && num_users > 0 && num_items > 0, PEA_ERR_ARG, "nfm_score: negative count or empty table");
    PEA_REQUIRE(emb && lin && w_fold && b_fold && w2 && bias_fold && uids && err_flag && (logits || pred), PEA_ERR_ARG,
                "nfm_score: null pointer (logits or pred must be given)");
    PEA_REQUIRE(mode == PEA_NFM_RANGE || iids, PEA_ERR_ARG, "nfm_score: iids is null");
    PEA_REQUIRE(mode == PEA_NFM_PAIRS || C >= 1, PEA_ERR_ARG, "nfm_score: %lld columns", (long long)C);
    PEA_REQUIRE(mode != PEA_NFM_RANGE || (item_lo >= 0 && item_lo + C <= num_items), PEA_ERR_ARG,
                "nfm_score: item range [%lld, +%lld) is not inside the %lld items", (long long)item_lo, (long long)C, (long long)num_items);
    PEA_REQUIRE((rank != nullptr) == (auc != nullptr) && (!rank || (mode == PEA_NFM_ROWS && logits)), PEA_ERR_ARG,
                "nfm_score: rank and auc come together, in the candidate-row form, from the logits");
    PEA_REQUIRE(ld_emb >= E && ld_emb % 4 == 0 && aligned16(emb) && aligned16(w_fold) && aligned16(b_fold) && aligned16(w2), PEA_ERR_ARG,
                "nfm_score: emb (row stride a multiple of 4, at least the width), w_fold, b_fold and w2 on 16-byte boundaries");
    NsArgs a = {};
    a.n_pairs = mode == PEA_NFM_PAIRS ? n_users : n_users * C;
    a.U = num_users; a.I = num_items; a.ld_emb = ld_emb; a.C = mode == PEA_NFM_PAIRS ? 1 : C; a.lo = item_lo;
    a.mode = mode; a.E = E; a.H = H; a.EP = ceil16(E); a.HP = ceil16(H); a.LD = a.EP + 4;
    a.emb = emb; a.lin = lin; a.wf = w_fold; a.bf = b_fold; a.w2 = w2; a.bias = bias_fold; a.uid = uids; a.iid = iids;
    a.logit = logits; a.pred = pred; a.err = err_flag;
    if (a.n_pairs == 0) return PEA_OK;
    const int64_t n_tiles = (a.n_pairs + kSP - 1) / kSP;
    const size_t lds = sizeof(float) * ((size_t)a.HP * a.LD + (size_t)kSP * a.LD + kWaves * kSP) + 2 * kSP * 8 + kSP * 4;
    PEA_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(&nfm_score_kernel), lds_limit(lds)));
    {
        ProfScope ps("nfm_score", stream, (double)a.n_pairs * 2.0 * E * H, (double)a.n_pairs * 8.0 * E);
        PEA_LAUNCH(nfm_score_kernel, dim3((unsigned)std::min<int64_t>(n_tiles, kScoreMaxWg)), dim3(kThreads), lds, stream, a);
        PEA_HIP(hipGetLastError());
    }
    if (rank) {
        PEA_LAUNCH(nfm_rank_kernel, dim3((unsigned)((n_users + 3) / 4)), dim3(256), 0, stream, n_users, C, (const float *)logits, rank, auc);
        PEA_HIP(hipGetLastError());
    }
    return PEA_OK;
}
