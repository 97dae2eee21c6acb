// Dense update of the reference's three baseline convs (nn/kgat_conv.py:46-54, nn/kgcn_conv.py:39-44,
// nn/ngcf_conv.py:46-48), forward and backward, for gfx950.  s = the weighted neighbour sum of x (pea_weighted_aggregate) is
// an INPUT; A1 = x + s, A2 = x * s, weights [in, out]:
//   PEA_KGU_KGAT   y = lrelu(A1 W1) + lrelu(A2 W2) + bias
//   PEA_KGU_KGCN   y = relu(A1 W1 + bias)
//   PEA_KGU_NGCF   y = lrelu(A1 W1 + A2 W2)       the reference writes x W_1 + s W_1 + (x * s) W_2; the first two products
//                                                 are merged here (one GEMM over x + s), which changes the rounding only
//   out = y * keep * keep_scale                   keep: optional [N, out] byte mask of the dropout that follows the conv
// Built from the tile toolkit of tile16.h: one workgroup = 4 waves walks its 16-row tiles in a fixed order (tile blockIdx.x,
// + gridDim.x, ...).  The weights sit in LDS once per workgroup (stage_weight); the tile's A1 / A2 rows are staged in LDS
// with 16-byte loads.  Every product runs from a zero accumulator with k ascending, in the TRANSPOSED orientation of
// mlp2.hip: the weights are the A operand and the data rows the B operand (rows_times_w), so lane (n, g) ends up with
// columns 16 u + 4 g .. + 3 of ROW n: one float4 per lane for bias, mask, output gradient and store.
// Backward: recomputes the pre-activations with the forward's code (nothing is saved between the calls), then
//   dZ = g * (z > 0 ? 1 : slope)  (0 for relu; z == 0 takes the slope, torch's rule),   g = g_out * keep * keep_scale
//   dA1 = dZ1 W1^T, dA2 = dZ2 W2^T,  dx = dA1 + dA2 * s,  ds = dA1 + dA2 * x
//   dW1 = A1^T dZ1, dW2 = A2^T dZ2,  dbias = column sum of g (KGAT) / of dZ1 (KGCN)
// dZ goes through LDS once (it is the B operand of dA with the row on the lane, rows_times_wt, and of dW with the row as
// k).  The dW tiles are dealt out to the four waves and stay in their accumulators over all tiles of the
// workgroup: one partial per workgroup (dw_store), added in workgroup order by kg_update_dw_kernel (ordered_sum).  No float
// atomics, grid = f(N), bitwise reproducible.
// Shapes whose two weight images and tiles exceed the CU's LDS (both widths > 112 with two weights) are cut into output
// column chunks: masks, dW and dbias are per output column, dA is the sum of the chunks' parts added in chunk order.
#include <algorithm>

#include "tile16.h"
#include "train_common.h"

namespace pea {
namespace {

constexpr int kMaxWg = 512;                   // partials of the backward: two workgroups per CU

struct Cfg {
    int IP = 0, OC = 0, LDA = 0, LDW = 0, LDZ = 0, nw = 1, nz = 0, NT = 1;
    size_t lds = 0;
};

bool supported(int kind, int in, int out) {
    return kind >= PEA_KGU_KGAT && kind <= PEA_KGU_NGCF && in >= 4 && in <= 128 && in % 4 == 0 && out >= 4 && out <= 128 &&
           out % 4 == 0;
}

Cfg make_cfg(int kind, int in, int out, bool bwd) {
    Cfg c;
    c.IP = ceil16(in);
    c.LDA = c.IP + 4;
    c.nw = kind == PEA_KGU_KGCN ? 1 : 2;
    c.nz = bwd ? c.nw + (kind == PEA_KGU_KGAT ? 1 : 0) : 0;
    const int outp = ceil16(out);
    for (int chunks = 1;; ++chunks) {
        c.OC = ceil16((outp + chunks - 1) / chunks);
        c.LDW = c.LDZ = c.OC + 4;
        c.lds = sizeof(float) * ((size_t)c.nw * c.IP * c.LDW + (size_t)c.nw * kTR * c.LDA + (size_t)c.nz * kTR * c.LDZ);
        // the backward also keeps its dW tiles in registers: at most 8 per wave and weight with two weights, 16 with one
        c.NT = tiles_per_wave((c.IP / 16) * (c.OC / 16));
        if ((c.lds <= kLdsBudget && (!bwd || c.NT <= (c.nw == 2 ? 8 : 16))) || c.OC == 16) break;
    }
    return c;
}

struct KguArgs {
    int64_t N;
    int kind, in, out;
    const float *x, *s, *w1, *w2, *bias;
    int64_t ldx, lds;
    float slope;
    const unsigned char *keep;
    float keep_scale;
    float *o;
    int64_t ldo;
    // backward
    const float *g;
    int64_t ldg;
    float *dx, *dsum;
    int64_t lddx, ldds;
    float *part;
    int want_dbias;
    int IP, OC, LDA, LDW, LDZ;
};

extern __shared__ __attribute__((aligned(16))) float kgu_smem[];

// A1 = x + s (and A2 = x * s) of the tile's 16 rows into LDS; rows >= N are zero rows
template <bool TWO>
__device__ __forceinline__ void stage_rows(const KguArgs &a, int64_t row0, float *A1t, float *A2t) {
    const int in4 = a.in / 4;
    for (int i = threadIdx.x; i < kTR * in4; i += kThreads) {
        const int r = i / in4, c = 4 * (i - r * in4);
        const int64_t row = row0 + r;
        float4 xv = make_float4(0.f, 0.f, 0.f, 0.f), sv = xv;
        if (row < a.N) {
            xv = ld4(a.x + row * a.ldx + c);
            sv = ld4(a.s + row * a.lds + c);
        }
        st4(A1t + r * a.LDA + c, make_float4(xv.x + sv.x, xv.y + sv.y, xv.z + sv.z, xv.w + sv.w));
        if (TWO) st4(A2t + r * a.LDA + c, make_float4(xv.x * sv.x, xv.y * sv.y, xv.z * sv.z, xv.w * sv.w));
    }
}

__device__ __forceinline__ float lrelu(float z, float slope) { return z > 0.f ? z : z * slope; }

// keep[row, col .. col + 3] * keep_scale as multipliers (1 without a mask)
__device__ __forceinline__ void keep4(const KguArgs &a, int64_t row, int col, float (&k)[4], float &scale) {
    scale = 1.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) k[r] = 1.f;
    if (a.keep) {
        const unsigned char *kp = a.keep + row * a.out + col;
#pragma unroll
        for (int r = 0; r < 4; ++r) k[r] = kp[r] ? 1.f : 0.f;
        scale = a.keep_scale;
    }
}

template <bool TWO>
__global__ __launch_bounds__(kThreads) void kg_update_fwd_kernel(const KguArgs a) {
    float *W1s = kgu_smem;
    float *W2s = W1s + (TWO ? a.IP * a.LDW : 0);
    float *A1t = W2s + a.IP * a.LDW;
    float *A2t = A1t + (TWO ? kTR * a.LDA : 0);
    constexpr int NC = TWO ? 2 : 1;      // weights = MFMA chains per product; without the second (KGCN) z2 / e2 are never read
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, n = lane & 15, g = lane >> 4;
    const int64_t n_tiles = (a.N + kTR - 1) / kTR;
    for (int i = threadIdx.x; i < (TWO ? 2 : 1) * kTR * a.LDA; i += kThreads) A1t[i] = 0.f;      // the pad columns stay zero
    for (int c0 = 0; c0 < a.out; c0 += a.OC) {
        __syncthreads();
        stage_weight<1>(a.w1, a.in, a.out, c0, W1s, a.IP, a.OC, a.LDW);      // one float at a time: the weights need no alignment
        if (TWO) stage_weight<1>(a.w2, a.in, a.out, c0, W2s, a.IP, a.OC, a.LDW);
        const int oc = a.out - c0 < a.OC ? a.out - c0 : a.OC;
        const int n_ut = (oc + 15) / 16;
        for (int64_t T = blockIdx.x; T < n_tiles; T += gridDim.x) {
            __syncthreads();
            stage_rows<TWO>(a, T * kTR, A1t, A2t);
            __syncthreads();
            const int64_t row = T * kTR + n;
            for (int u = wave; u < n_ut; u += kWaves) {
                f32x4 z[NC] = {};
                rows_times_w<NC, NC>(W1s, a.IP, a.LDW, A1t, a.LDA, a.in / 4, u, n, g, z);
                const f32x4 &z1 = z[0], &z2 = z[NC - 1];
                const int col = c0 + 16 * u + 4 * g;
                if (row >= a.N || col >= a.out) continue;
                float b[4] = {0.f, 0.f, 0.f, 0.f}, k[4], scale, y[4];
                if (a.bias) {
                    const float4 bv = ld4(a.bias + col);
                    b[0] = bv.x; b[1] = bv.y; b[2] = bv.z; b[3] = bv.w;
                }
                keep4(a, row, col, k, scale);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (a.kind == PEA_KGU_KGAT)
                        y[r] = (lrelu(z1[r], a.slope) + lrelu(z2[r], a.slope)) + b[r];
                    else if (a.kind == PEA_KGU_KGCN)
                        y[r] = fmaxf(z1[r] + b[r], 0.f);
                    else
                        y[r] = lrelu(z1[r] + z2[r], a.slope);
                    if (a.keep) y[r] = y[r] * k[r] * scale;
                }
                st4(a.o + row * a.ldo + col, make_float4(y[0], y[1], y[2], y[3]));
            }
        }
    }
}

// NT: dW tiles per wave and weight (tile id = wave + 4 q -> input tile id / n_ut, output tile id % n_ut)
template <int NT, bool TWO>
__global__ __launch_bounds__(kThreads) void kg_update_bwd_kernel(const KguArgs a) {
    float *W1s = kgu_smem;
    float *W2s = W1s + (TWO ? a.IP * a.LDW : 0);
    float *A1t = W2s + a.IP * a.LDW;
    float *A2t = A1t + (TWO ? kTR * a.LDA : 0);
    float *Z1t = A2t + kTR * a.LDA;
    float *Z2t = Z1t + (TWO ? kTR * a.LDZ : 0);
    float *Gt = Z2t + kTR * a.LDZ;                 // KGAT only: g itself, for dbias
    constexpr int NC = TWO ? 2 : 1;      // weights = MFMA chains per product; without the second (KGCN) z2 / e2 are never read
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, n = lane & 15, g = lane >> 4;
    const int64_t n_tiles = (a.N + kTR - 1) / kTR;
    const int IT = a.IP / 16;
    const size_t wsz = (size_t)a.in * a.out;
    float *part = a.part + (size_t)blockIdx.x * (2 * wsz + a.out);
    const float *Bt = a.kind == PEA_KGU_KGAT ? Gt : Z1t;      // what dbias sums
    for (int i = threadIdx.x; i < (TWO ? 2 : 1) * kTR * a.LDA; i += kThreads) A1t[i] = 0.f;
    for (int c0 = 0; c0 < a.out; c0 += a.OC) {
        __syncthreads();
        stage_weight<1>(a.w1, a.in, a.out, c0, W1s, a.IP, a.OC, a.LDW);      // one float at a time: the weights need no alignment
        if (TWO) stage_weight<1>(a.w2, a.in, a.out, c0, W2s, a.IP, a.OC, a.LDW);
        const int oc = a.out - c0 < a.OC ? a.out - c0 : a.OC;
        const int n_ut = (oc + 15) / 16;
        f32x4 dw[NC][NT] = {};
        float db = 0.f;
        for (int64_t T = blockIdx.x; T < n_tiles; T += gridDim.x) {
            __syncthreads();
            stage_rows<TWO>(a, T * kTR, A1t, A2t);
            __syncthreads();
            const int64_t row = T * kTR + n;
            // ---- pre-activations -> dZ tiles in LDS (zero for rows >= N and columns >= out)
            for (int u = wave; u < n_ut; u += kWaves) {
                f32x4 z[NC] = {};
                rows_times_w<NC, NC>(W1s, a.IP, a.LDW, A1t, a.LDA, a.in / 4, u, n, g, z);
                const f32x4 &z1 = z[0], &z2 = z[NC - 1];
                const int lc = 16 * u + 4 * g, col = c0 + lc;
                float gv[4] = {0.f, 0.f, 0.f, 0.f}, d1[4], d2[4];
                float b[4] = {0.f, 0.f, 0.f, 0.f};
                if (row < a.N && col < a.out) {
                    const float4 t = ld4(a.g + row * a.ldg + col);
                    float k[4], scale;
                    keep4(a, row, col, k, scale);
                    gv[0] = t.x; gv[1] = t.y; gv[2] = t.z; gv[3] = t.w;
                    if (a.keep) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) gv[r] = gv[r] * k[r] * scale;
                    }
                    if (a.bias) {
                        const float4 bv = ld4(a.bias + col);
                        b[0] = bv.x; b[1] = bv.y; b[2] = bv.z; b[3] = bv.w;
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (a.kind == PEA_KGU_KGAT) {
                        d1[r] = gv[r] * (z1[r] > 0.f ? 1.f : a.slope);
                        d2[r] = gv[r] * (z2[r] > 0.f ? 1.f : a.slope);
                    } else if (a.kind == PEA_KGU_KGCN) {
                        d1[r] = (z1[r] + b[r]) > 0.f ? gv[r] : 0.f;
                        d2[r] = 0.f;
                    } else {
                        d1[r] = d2[r] = gv[r] * ((z1[r] + z2[r]) > 0.f ? 1.f : a.slope);
                    }
                }
                st4(Z1t + n * a.LDZ + lc, make_float4(d1[0], d1[1], d1[2], d1[3]));
                if (TWO) st4(Z2t + n * a.LDZ + lc, make_float4(d2[0], d2[1], d2[2], d2[3]));
                if (a.kind == PEA_KGU_KGAT) st4(Gt + n * a.LDZ + lc, make_float4(gv[0], gv[1], gv[2], gv[3]));
            }
            __syncthreads();
            // ---- dA^T = W dZ^T per input tile v: register r of lane (n, g) = dA[row n][input 16 v + 4 g + r]
            for (int v = wave; v < IT; v += kWaves) {
                f32x4 e[NC] = {};
                rows_times_wt<NC, NC>(W1s, a.IP, a.LDW, Z1t, a.LDZ, oc / 4, v, n, g, e);
                const f32x4 &e1 = e[0], &e2 = e[NC - 1];
                const int col = 16 * v + 4 * g;
                if (row >= a.N || col >= a.in) continue;
                float4 rx = make_float4(e1[0], e1[1], e1[2], e1[3]), rs = rx;
                if (TWO) {
                    const float4 xv = ld4(a.x + row * a.ldx + col), sv = ld4(a.s + row * a.lds + col);
                    rx = make_float4(e1[0] + e2[0] * sv.x, e1[1] + e2[1] * sv.y, e1[2] + e2[2] * sv.z, e1[3] + e2[3] * sv.w);
                    rs = make_float4(e1[0] + e2[0] * xv.x, e1[1] + e2[1] * xv.y, e1[2] + e2[2] * xv.z, e1[3] + e2[3] * xv.w);
                }
                float *px = a.dx + row * a.lddx + col, *ps = a.dsum + row * a.ldds + col;
                if (c0 > 0) {      // a later output-column chunk adds its part to what the earlier ones left
                    const float4 ox = ld4(px), os = ld4(ps);
                    rx = make_float4(ox.x + rx.x, ox.y + rx.y, ox.z + rx.z, ox.w + rx.w);
                    rs = make_float4(os.x + rs.x, os.y + rs.y, os.z + rs.z, os.w + rs.w);
                }
                st4(px, rx);
                st4(ps, rs);
            }
            // ---- dW += A^T dZ over the tile's 16 rows (4 k-steps): register r of lane (n, g) = dW[16 v + 4 g + r][16 u + n]
            //      (written out here and in transr_train.hip, tile16.h says why)
#pragma unroll
            for (int q = 0; q < NT; ++q) {
                const int id = wave + kWaves * q;
                if (id >= IT * n_ut) continue;
                const int v = id / n_ut, u = id - v * n_ut;
                const int ao = g * a.LDA + 16 * v + n, zo = g * a.LDZ + 16 * u + n;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    dw[0][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(A1t[ao + 4 * t * a.LDA], Z1t[zo + 4 * t * a.LDZ], dw[0][q], 0, 0, 0);
                    if (TWO)
                        dw[NC - 1][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(A2t[ao + 4 * t * a.LDA], Z2t[zo + 4 * t * a.LDZ], dw[NC - 1][q], 0, 0, 0);
                }
            }
            if (a.want_dbias && (int)threadIdx.x < oc) {
                for (int r = 0; r < kTR; ++r) db += Bt[r * a.LDZ + threadIdx.x];
            }
        }
        // ---- this workgroup's partial of the chunk's columns
        dw_store<NT, NC>(dw, part, wsz, a.in, a.out, c0, IT, n_ut, wave, n, g);
        if (a.want_dbias && (int)threadIdx.x < oc) part[2 * wsz + c0 + threadIdx.x] = db;
    }
}

// element e of [dW1 | dW2 | dbias] = the workgroups' partials added in workgroup order
__global__ __launch_bounds__(256) void kg_update_dw_kernel(int n_wg, int in, int out, const float *__restrict__ part, float *dw1,
                                                          float *dw2, float *dbias) {
    const size_t wsz = (size_t)in * out, stride = 2 * wsz + out;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= stride) return;
    float *dst = e < wsz ? (dw1 ? dw1 + e : nullptr) : e < 2 * wsz ? (dw2 ? dw2 + (e - wsz) : nullptr) : (dbias ? dbias + (e - 2 * wsz) : nullptr);
    if (!dst) return;
    *dst = ordered_sum(part + e, stride, n_wg);
}

int check_args(const char *who, int64_t N, int kind, int in, int out, const float *x, int64_t ldx, const float *s, int64_t lds,
               const float *w1, const float *w2, const float *bias, const float *o, int64_t ldo) {
    PEA_REQUIRE(supported(kind, in, out), PEA_ERR_ARG, "%s: kind %d, widths %d -> %d (multiples of 4 in 4..128)", who, kind, in, out);
    PEA_REQUIRE(N >= 0 && x && s && w1 && o, PEA_ERR_ARG, "%s: null pointer or N < 0", who);
    PEA_REQUIRE(kind == PEA_KGU_KGCN ? w2 == nullptr : w2 != nullptr, PEA_ERR_ARG,
                "%s: w2 is required for KGAT / NGCF and must be NULL for KGCN", who);
    PEA_REQUIRE(kind != PEA_KGU_NGCF || bias == nullptr, PEA_ERR_ARG, "%s: NGCF has no bias", who);
    PEA_REQUIRE(ldx >= in && ldx % 4 == 0 && lds >= in && lds % 4 == 0 && ldo >= out && ldo % 4 == 0, PEA_ERR_ARG,
                "%s: row strides %lld / %lld / %lld (multiples of 4, at least the width)", who, (long long)ldx, (long long)lds,
                (long long)ldo);
    PEA_REQUIRE(aligned16(x) && aligned16(s) && aligned16(o) && aligned16(bias), PEA_ERR_ARG, "%s: x, s, out and bias must start on 16-byte boundaries", who);
    return PEA_OK;
}

}  // namespace
}  // namespace pea

using namespace pea;

extern "C" int pea_kg_update_supported(int kind, int in_width, int out_width) { return supported(kind, in_width, out_width) ? 1 : 0; }

extern "C" int pea_kg_update_forward(int64_t N, int kind, int in_width, int out_width, const float *x, int64_t ldx, const float *s,
                                     int64_t lds, const float *w1, const float *w2, const float *bias, float negative_slope,
                                     const unsigned char *keep, float keep_scale, float *out, int64_t ldo, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    PEA_TRY(check_args("kg_update_forward", N, kind, in_width, out_width, x, ldx, s, lds, w1, w2, bias, out, ldo));
    if (N == 0) return PEA_OK;
    const Cfg c = make_cfg(kind, in_width, out_width, false);
    KguArgs a = {};
    a.N = N; a.kind = kind; a.in = in_width; a.out = out_width;
    a.x = x; a.s = s; a.w1 = w1; a.w2 = w2; a.bias = bias; a.ldx = ldx; a.lds = lds;
    a.slope = negative_slope; a.keep = keep; a.keep_scale = keep_scale; a.o = out; a.ldo = ldo;
    a.IP = c.IP; a.OC = c.OC; a.LDA = c.LDA; a.LDW = c.LDW; a.LDZ = c.LDZ;
    const int64_t tiles = (N + kTR - 1) / kTR;
    const dim3 grid((unsigned)std::min<int64_t>(tiles, 1024));
    const double flop_bytes = (double)N * 4.0 * (2.0 * in_width + out_width) + (keep ? (double)N * out_width : 0.0);
    ProfScope ps("kg_update_fwd", stream, flop_bytes);
    if (c.nw == 2) {
        PEA_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(&kg_update_fwd_kernel<true>), lds_limit(c.lds)));
        PEA_LAUNCH(kg_update_fwd_kernel<true>, grid, dim3(kThreads), c.lds, stream, a);
    } else {
        PEA_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(&kg_update_fwd_kernel<false>), lds_limit(c.lds)));
        PEA_LAUNCH(kg_update_fwd_kernel<false>, grid, dim3(kThreads), c.lds, stream, a);
    }
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}

extern "C" size_t pea_kg_update_backward_workspace_bytes(int kind, int in_width, int out_width) {
    if (!supported(kind, in_width, out_width)) return 0;
    return (size_t)kMaxWg * (2 * (size_t)in_width * out_width + out_width) * sizeof(float) + 256;
}

namespace pea {
namespace {
template <int NT>
int launch_bwd(const Cfg &c, const KguArgs &a, dim3 grid, hipStream_t stream) {
    if (c.nw == 2) {
        constexpr int NT2 = NT > 8 ? 8 : NT;      // make_cfg never asks for more with two weights
        PEA_REQUIRE(c.NT <= 8, PEA_ERR_ARG, "kg_update_backward: %d dW tiles per wave", c.NT);
        PEA_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(&kg_update_bwd_kernel<NT2, true>), lds_limit(c.lds)));
        PEA_LAUNCH((kg_update_bwd_kernel<NT2, true>), grid, dim3(kThreads), c.lds, stream, a);
    } else {
        PEA_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(&kg_update_bwd_kernel<NT, false>), lds_limit(c.lds)));
        PEA_LAUNCH((kg_update_bwd_kernel<NT, false>), grid, dim3(kThreads), c.lds, stream, a);
    }
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}
}  // namespace
}  // namespace pea

extern "C" int pea_kg_update_backward(int64_t N, int kind, int in_width, int out_width, const float *x, int64_t ldx, const float *s,
                                      int64_t lds, const float *w1, const float *w2, const float *bias, float negative_slope,
                                      const unsigned char *keep, float keep_scale, const float *g_out, int64_t ldg, float *dx,
                                      int64_t lddx, float *ds, int64_t ldds, float *dw1, float *dw2, float *dbias, void *workspace,
                                      size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    PEA_TRY(check_args("kg_update_backward", N, kind, in_width, out_width, x, ldx, s, lds, w1, w2, bias, g_out, ldg));
    PEA_REQUIRE(dx && ds && dw1 && workspace, PEA_ERR_ARG, "kg_update_backward: null pointer");
    PEA_REQUIRE(kind == PEA_KGU_KGCN || dw2 != nullptr, PEA_ERR_ARG, "kg_update_backward: dw2 is required for KGAT / NGCF");
    PEA_REQUIRE(lddx >= in_width && lddx % 4 == 0 && ldds >= in_width && ldds % 4 == 0 && aligned16(dx) && aligned16(ds), PEA_ERR_ARG,
                "kg_update_backward: dx / ds strides %lld / %lld (multiples of 4, at least the width, 16-byte aligned)",
                (long long)lddx, (long long)ldds);
    PEA_REQUIRE(workspace_bytes >= pea_kg_update_backward_workspace_bytes(kind, in_width, out_width), PEA_ERR_NOMEM,
                "kg_update_backward: workspace too small");
    const size_t wsz = (size_t)in_width * out_width;
    if (kind == PEA_KGU_NGCF) dbias = nullptr;
    if (kind == PEA_KGU_KGCN) dw2 = nullptr;
    if (N == 0) {
        PEA_MEMSET_ASYNC(dw1, 0, wsz * sizeof(float), stream);
        if (dw2) PEA_MEMSET_ASYNC(dw2, 0, wsz * sizeof(float), stream);
        if (dbias) PEA_MEMSET_ASYNC(dbias, 0, (size_t)out_width * sizeof(float), stream);
        return PEA_OK;
    }
    const Cfg c = make_cfg(kind, in_width, out_width, true);
    KguArgs a = {};
    a.N = N; a.kind = kind; a.in = in_width; a.out = out_width;
    a.x = x; a.s = s; a.w1 = w1; a.w2 = w2; a.bias = bias; a.ldx = ldx; a.lds = lds;
    a.slope = negative_slope; a.keep = keep; a.keep_scale = keep_scale;
    a.g = g_out; a.ldg = ldg; a.dx = dx; a.dsum = ds; a.lddx = lddx; a.ldds = ldds;
    a.part = aligned_ws(workspace);
    a.want_dbias = dbias ? 1 : 0;
    a.IP = c.IP; a.OC = c.OC; a.LDA = c.LDA; a.LDW = c.LDW; a.LDZ = c.LDZ;
    const int64_t tiles = (N + kTR - 1) / kTR;
    const int n_wg = (int)std::min<int64_t>(tiles, kMaxWg);
    {
        ProfScope ps("kg_update_bwd", stream, (double)N * 4.0 * (4.0 * in_width + out_width) + (keep ? (double)N * out_width : 0.0));
        switch (c.NT) {
            case 1: PEA_TRY(launch_bwd<1>(c, a, dim3(n_wg), stream)); break;
            case 2: PEA_TRY(launch_bwd<2>(c, a, dim3(n_wg), stream)); break;
            case 4: PEA_TRY(launch_bwd<4>(c, a, dim3(n_wg), stream)); break;
            case 8: PEA_TRY(launch_bwd<8>(c, a, dim3(n_wg), stream)); break;
            default: PEA_TRY(launch_bwd<16>(c, a, dim3(n_wg), stream)); break;
        }
    }
    {
        const size_t total = 2 * wsz + out_width;
        ProfScope ps("kg_update_dw", stream, (double)n_wg * total * 4.0);
        PEA_LAUNCH(kg_update_dw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, n_wg, in_width, out_width,
                   (const float *)a.part, dw1, dw2, dbias);
        PEA_HIP(hipGetLastError());
    }
    return PEA_OK;
}
