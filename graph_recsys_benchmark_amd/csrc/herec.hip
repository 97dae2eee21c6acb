// HeRec (reference models/herec.py:36-46, experiments/herec_solver_bpr.py:108-121) for gfx950: the training step of a batch
// of labelled pairs in one launch, and the width-(D + 4) catalogue table that turns its scores into plain row dots.
//   S(n)       = sum_m sigmoid(E_m[n] W_m^T + b_m)        E_m [N, D] frozen tables, W_m [D, D] out x in (torch Linear)
//   pred(u, i) = <ue[u'], ie[i']> + <S(u), urk[u']> + <S(i), irk[i']>,   u' = u - acc_uids, i' = i - acc_iids
//   loss       = sum_b (pred_b - label_b)^2 / B,   g_b = 2 (pred_b - label_b) / B
//   dZ_m = dS (.) s_m (1 - s_m),  dS(u) = g urk[u'],  dS(i) = g irk[i'],  dW_m = dZ_m^T E_m[rows],  db_m = colsum dZ_m
//   g_user [B, 2D] = [g ie[i'], g S(u)],  g_item [B, 2D] = [g ue[u'], g S(i)]     (the caller scatters them by u' / i')
// Built from tile16.h like transr_train.hip: one workgroup = 4 waves walks tiles of 16 pairs = 32 gathered rows per table
// (block 0 the users, block 1 the items) in a fixed order (tile blockIdx.x, + gridDim.x, ...).  The M weights sit in LDS
// once per workgroup, RAW (image row = output o, column = input i), so Z = E W^T is the toolkit's transposed product
// (rows_times_wt: k = the image's columns, exactly D / 4 steps) and no transposed copy exists.  The tile keeps the gathered
// rows [M][32] (the B operand of dW) and s_m [M][32] (overwritten by dZ_m, the A operand of dW) in LDS; the four embedding
// tables are read from global memory where they are used (their rows are elementwise operands only).  pred is three dot
// products per pair (lanes 0..47 of wave 0: one term each), each eight fma chains in ascending column order (column c in
// chain c % 8) added pairwise, as transr_train.hip sums its squares.  dZ and db belong to one thread per (table, column)
// walking the tile's 32 rows in order: db stays in that thread's register over the workgroup's tiles.  dW_m [out, in] is
// dealt out to the waves as 16x16 tiles (id = wave + 4 q -> output tile id / IT, input tile id % IT, the same for every m:
// M chains per q) and stays in the accumulators over all tiles of the workgroup: one partial per workgroup (dw_store),
// added with the db partials and the loss sums in workgroup order by herec_final_kernel (ordered_sum).
// No float atomics, grid = f(B), bitwise reproducible, 64-bit row indexing.  A pair with an id out of range is staged as
// zero rows (nothing is read through it: its ids are replaced by the blocks' first rows and its g is 0), contributes
// nothing, gets zero gradient rows and sets the error flag; the mean still divides by B.
//
// What is supported (herec_supported below), and why the rest is not:
//   * D a multiple of 4 in 4..128: 16-byte row accesses, and dW tiles of a wave <= 16 (64 accumulator registers);
//   * 1 <= M <= PEA_HEREC_MAX_TABLES, M D <= 256 (one db thread per (table, column));
//   * M * tiles_per_wave(IT^2) <= 16 accumulator tiles per wave, IT = ceil16(D) / 16: M <= 4 up to D = 64, M <= 2 up
//     to D = 80, M = 1 beyond;
//   * all M images and the tile's rows resident in kLdsBudget (159,744 bytes): (64, 4) takes 148,416, (128, 1) 118,720,
//     (80, 2) 107,968.  (128, 2) would need 220,096 and is refused: there is no second code path that streams the images.
#include <algorithm>

#include "tile16.h"
#include "train_common.h"

namespace pea {
namespace {

constexpr int kMaxWg = 256;                   // partials of dW: one workgroup per CU
constexpr int kTblMaxWg = 512;                // workgroups of the table build (two to three fit a CU at M = 2, D = 64)
constexpr int kMaxT = PEA_HEREC_MAX_TABLES;
constexpr int kRows = 2 * kTR;                // gathered rows per table and tile

// floats behind the tiles: g, the loss term, pred parts and the validity per pair, the pair's two local ids (as int64)
constexpr int kSmallFloats = 16 + 16 + 16 + 2 * 2 * kTR;

size_t train_lds_bytes(int D, int M) {
    const int ip = ceil16(D), ld = ip + 4;
    return sizeof(float) * ((size_t)M * ip * ld + (size_t)(2 * M + 1) * kRows * ld + kSmallFloats);
}

size_t table_lds_bytes(int D, int M) {
    const int ip = ceil16(D), ld = ip + 4;
    return sizeof(float) * ((size_t)M * ip * ld + (size_t)(M + 2) * kRows * ld);
}

bool supported(int D, int M) {
    if (D < 4 || D > 128 || D % 4 != 0 || M < 1 || M > kMaxT || M * D > kThreads) return false;
    const int it = ceil16(D) / 16;
    if (M * tiles_per_wave(it * it) > 16) return false;
    return train_lds_bytes(D, M) <= kLdsBudget;
}

struct HrTables {
    const float *e[kMaxT];
    int64_t ld[kMaxT];
};

struct HrArgs {
    int64_t B, N, acc_u, num_u, acc_i, num_i;
    int D, M, IP, LD;
    HrTables t;
    const float *w, *b;                       // [M, D, D], [M, D]
    const float *ue, *ie, *urk, *irk;         // [num_u, D], [num_i, D], contiguous
    const int64_t *unids, *inids;
    const float *labels;
    float *pred;
    float *g_user, *g_item;                   // [B, 2 D]
    float *part, *dbp, *sums;
    int *err;
};

extern __shared__ __attribute__((aligned(16))) float hr_smem[];

// <p, q> over D columns: eight fma chains (column c in chain c % 8), added pairwise
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

// S of the tile's 32 staged rows per table: output tile v of every table on this wave, s_m = sigmoid(z + b_m) to St (when
// asked: the backward's operand; columns >= D as zeros) and their sum over m, in table order, to Ss
template <bool KEEP>
__device__ __forceinline__ void sigmoid_sum(const float *Ws, const float *Xt, float *St, float *Ss, const float *bias, int M, int D,
                                            int IP, int LD, int wave, int n, int g) {
    const int IT = IP / 16, in4 = D / 4;
    for (int v = wave; v < IT; v += kWaves) {
        const int col = 16 * v + 4 * g;
        f32x4 S[2] = {};
        for (int m = 0; m < M; ++m) {
            f32x4 z[2] = {};
            rows_times_wt<1, 2>(Ws + (size_t)m * IP * LD, IP, LD, Xt + (size_t)m * kRows * LD, LD, in4, v, n, g, z);
            float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (col < D) bv = ld4(bias + m * D + col);
            const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                float s[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s[r] = col < D ? 1.0f / (1.0f + expf(-(z[c][r] + bb[r]))) : 0.f;
                    S[c][r] += s[r];
                }
                if (KEEP) st4(St + ((size_t)m * kRows + c * kTR + n) * LD + col, make_float4(s[0], s[1], s[2], s[3]));
            }
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) st4(Ss + (c * kTR + n) * LD + col, make_float4(S[c][0], S[c][1], S[c][2], S[c][3]));
    }
}

// NT: dW tiles per wave and table; MT: tables (BWD only; the forward reads a.M); BWD = false: forward only
template <int NT, int MT, bool BWD>
__global__ __launch_bounds__(kThreads) void herec_train_kernel(const HrArgs a) {
    const int LD = a.LD, D = a.D, M = a.M;
    float *Ws = hr_smem;                                // [M][IP][LD] raw weights
    float *Xt = Ws + (size_t)M * a.IP * LD;             // [M][32][LD] gathered rows: users, then items
    float *St = Xt + (size_t)M * kRows * LD;            // [M][32][LD] s_m, then dZ_m
    float *Ss = St + (size_t)M * kRows * LD;            // [32][LD] S
    float *sm = Ss + kRows * LD;
    float *gco = sm, *term = sm + 16;
    int *valid = reinterpret_cast<int *>(sm + 32);
    int64_t *ids = reinterpret_cast<int64_t *>(sm + 48);        // [2][16]: u', i' of the tile's pairs
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, n = lane & 15, g = lane >> 4;
    const int64_t n_tiles = (a.B + kTR - 1) / kTR;
    const int IT = a.IP / 16, in4 = D / 4;
    for (int i = threadIdx.x; i < M * kRows * LD; i += kThreads) Xt[i] = 0.f;      // the pad columns stay zero
    for (int m = 0; m < M; ++m) stage_weight<4>(a.w + (size_t)m * D * D, D, D, 0, Ws + (size_t)m * a.IP * LD, a.IP, a.IP, LD);
    f32x4 dw[MT][NT] = {};
    float db = 0.f, wg_loss = 0.f;
    const float inv_b2 = 2.0f / (float)a.B;
    for (int64_t T = blockIdx.x; T < n_tiles; T += gridDim.x) {
        __syncthreads();
        // ---- the tile's ids: a pair beyond B or with an id out of range is a zero row everywhere below
        if (threadIdx.x < kTR) {
            const int64_t p = T * kTR + threadIdx.x;
            int64_t u = 0, it = 0;
            bool ok = p < a.B;
            if (ok) {
                u = a.unids[p];
                it = a.inids[p];
                ok = u >= 0 && u < a.N && u >= a.acc_u && u - a.acc_u < a.num_u && it >= 0 && it < a.N && it >= a.acc_i &&
                     it - a.acc_i < a.num_i;
                if (!ok) atomicOr(a.err, 1);
            }
            valid[threadIdx.x] = ok ? 1 : 0;
            ids[threadIdx.x] = ok ? u - a.acc_u : 0;
            ids[kTR + threadIdx.x] = ok ? it - a.acc_i : 0;
        }
        __syncthreads();
        {   // a thread's loads go out together (at most kPreX float4s: M D <= 256), then into LDS
            constexpr int kPreX = kThreads / kRows;
            float4 px[kPreX];
#pragma unroll
            for (int j = 0; j < kPreX; ++j) {
                const int i = threadIdx.x + j * kThreads, mr = i / in4, c = 4 * (i - mr * in4), m = mr / kRows, rr = mr - m * kRows;
                px[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (i < M * kRows * in4 && valid[rr & 15])
                    px[j] = ld4(a.t.e[m] + (ids[rr] + (rr < kTR ? a.acc_u : a.acc_i)) * a.t.ld[m] + c);
            }
#pragma unroll
            for (int j = 0; j < kPreX; ++j) {
                const int i = threadIdx.x + j * kThreads, mr = i / in4, c = 4 * (i - mr * in4);
                if (i < M * kRows * in4) st4(Xt + (size_t)mr * LD + c, px[j]);
            }
        }
        __syncthreads();
        sigmoid_sum<BWD>(Ws, Xt, St, Ss, a.b, M, D, a.IP, LD, wave, n, g);
        __syncthreads();
        // ---- pred: lane 16 k + n of wave 0 has term k of pair n; then the loss term and g
        if (wave == 0) {
            float s = 0.f;
            const int64_t ur = ids[n] * D, ir = ids[kTR + n] * D;
            if (g == 0) s = dot8(a.ue + ur, a.ie + ir, D);
            else if (g == 1) s = dot8(Ss + n * LD, a.urk + ur, D);
            else if (g == 2) s = dot8(Ss + (kTR + n) * LD, a.irk + ir, D);
            const float s1 = __shfl(s, (lane + kTR) & (kWave - 1)), s2 = __shfl(s, (lane + 2 * kTR) & (kWave - 1));
            if (lane < kTR) {
                const bool ok = valid[lane] != 0;
                const int64_t p = T * kTR + lane;
                const float pred = ok ? (s + s1) + s2 : 0.f;
                const float d = ok ? pred - a.labels[p] : 0.f;
                term[lane] = d * d;
                gco[lane] = d * inv_b2;
                if (a.pred && p < a.B) a.pred[p] = pred;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            float s = 0.f;
            for (int k = 0; k < kTR; ++k) s += term[k];      // pair order inside the tile, tiles in the workgroup's order
            wg_loss += s;
        }
        if (!BWD) continue;
        // ---- dZ_m over s_m in place and db: thread (m, c) walks the 32 rows in order
        if (threadIdx.x < M * D) {
            const int m = threadIdx.x / D, c = threadIdx.x - m * D;
            float *col = St + (size_t)m * kRows * LD + c;
#pragma unroll 4
            for (int rr = 0; rr < kRows; ++rr) {
                const float rk = rr < kTR ? a.urk[ids[rr] * D + c] : a.irk[ids[rr] * D + c];
                const float s = col[rr * LD];
                const float dz = (gco[rr & 15] * rk) * ((1.0f - s) * s);
                col[rr * LD] = dz;
                db += dz;
            }
        }
        // ---- the pairs' gradient rows: [g ie, g S(u)] and [g ue, g S(i)]
        for (int i = threadIdx.x; i < 4 * kTR * in4; i += kThreads) {
            const int sr = i / in4, c = 4 * (i - sr * in4), seg = sr / kTR, rr = sr - seg * kTR;
            const int64_t p = T * kTR + rr;
            if (p >= a.B) continue;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid[rr]) {
                const float gg = gco[rr];
                const float4 x = seg == 0   ? ld4(a.ie + ids[kTR + rr] * D + c)
                                 : seg == 1 ? ld4(Ss + rr * LD + c)
                                 : seg == 2 ? ld4(a.ue + ids[rr] * D + c)
                                            : ld4(Ss + (kTR + rr) * LD + c);
                v = make_float4(gg * x.x, gg * x.y, gg * x.z, gg * x.w);
            }
            st4((seg < 2 ? a.g_user : a.g_item) + p * 2 * D + (seg & 1) * D + c, v);
        }
        __syncthreads();
        // ---- dW_m += dZ_m^T E_m[rows] over the tile's 32 rows (8 k-steps): register r of lane (n, g) =
        //      dW_m[16 v + 4 g + r][16 u + n]  (written out here as in transr_train.hip, tile16.h says why)
#pragma unroll
        for (int q = 0; q < NT; ++q) {
            const int id = wave + kWaves * q;
            if (id >= IT * IT) continue;
            const int v = id / IT, u = id - v * IT;
            const int zo = g * LD + 16 * v + n, xo = g * LD + 16 * u + n;
#pragma unroll
            for (int t = 0; t < kRows / 4; ++t) {
#pragma unroll
                for (int m = 0; m < MT; ++m)
                    dw[m][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(St[m * kRows * LD + zo + 4 * t * LD], Xt[m * kRows * LD + xo + 4 * t * LD],
                                                                    dw[m][q], 0, 0, 0);
            }
        }
    }
    if (threadIdx.x == 0) a.sums[blockIdx.x] = wg_loss;
    if (!BWD) return;
    if (threadIdx.x < M * D) a.dbp[(size_t)blockIdx.x * M * D + threadIdx.x] = db;
    dw_store<NT, MT>(dw, a.part + (size_t)blockIdx.x * M * D * D, (size_t)D * D, D, D, 0, IT, IT, wave, n, g);
}

// element e of [dW | db] = the workgroups' partials added in workgroup order; the loss = the workgroups' sums in index
// order, divided by B
__global__ __launch_bounds__(256) void herec_final_kernel(int n_wg, int64_t B, size_t wsz, size_t bsz, const float *__restrict__ part,
                                                         const float *__restrict__ dbp, const float *__restrict__ sums, float *dw,
                                                         float *dbias, float *loss) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (dw && e < wsz) dw[e] = ordered_sum(part + e, wsz, n_wg);
    else if (dw && e < wsz + bsz) dbias[e - wsz] = ordered_sum(dbp + (e - wsz), bsz, n_wg);
    if (e == 0) loss[0] = ordered_sum(sums, 1, n_wg) / (float)B;
}

int n_workgroups(int64_t B) { return (int)std::min<int64_t>((B + kTR - 1) / kTR, kMaxWg); }

size_t dbp_offset() { return kWsSumsOffset + align256((size_t)kMaxWg * sizeof(float)); }
size_t part_offset(int64_t B, int D, int M) { return dbp_offset() + align256((size_t)n_workgroups(B) * M * D * sizeof(float)); }

template <int NT, int MT, bool BWD>
int launch_train(const HrArgs &a, int n_wg, hipStream_t stream) {
    const size_t lds = train_lds_bytes(a.D, a.M);
    PEA_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(&herec_train_kernel<NT, MT, BWD>), lds_limit(lds)));
    PEA_LAUNCH((herec_train_kernel<NT, MT, BWD>), dim3(n_wg), dim3(kThreads), lds, stream, a);
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}

template <int NT>
int launch_train_m(const HrArgs &a, int n_wg, hipStream_t stream) {
    if (a.M == 1) return launch_train<NT, 1, true>(a, n_wg, stream);      // supported(): M * NT <= 16
    if constexpr (NT <= 8) {
        if (a.M == 2) return launch_train<NT, 2, true>(a, n_wg, stream);
    }
    if constexpr (NT <= 4) {
        if (a.M == 3) return launch_train<NT, 3, true>(a, n_wg, stream);
        if (a.M == 4) return launch_train<NT, 4, true>(a, n_wg, stream);
    }
    set_error("herec_train: %d tables at %d accumulator tiles per wave", a.M, NT);
    return PEA_ERR_ARG;
}

// ---------------------------------------------------------------------------------------------- the catalogue table
struct HtArgs {
    int64_t N, acc_u, num_u, acc_i, num_i;
    int64_t u_tiles, n_tiles;                 // tiles of 32 rows: the users' first, then the items'
    int64_t seg_lo[3], seg_hi[3];             // the rows of other nodes
    int D, M, IP, LD;
    HrTables t;
    const float *w, *b;
    const float *ue, *ie, *urk, *irk;
    float *out;                               // [N, D + 4]
};

// user row [ue, 1, c_u, 0, 0], item row [ie, beta_i, 1, 0, 0], c_u = <S(u), urk[u']>, beta_i = <S(i), irk[i']> as one fma
// chain per row in ascending column order; rows of other nodes are zero-filled
__global__ __launch_bounds__(kThreads) void herec_table_kernel(const HtArgs a) {
    const int LD = a.LD, D = a.D, M = a.M, W = D + 4;
    float *Ws = hr_smem;
    float *Xt = Ws + (size_t)M * a.IP * LD;             // [M][32][LD]
    float *Ss = Xt + (size_t)M * kRows * LD;            // [32][LD]
    float *Rk = Ss + kRows * LD;                        // [32][LD] the rows' rk bias
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, n = lane & 15, g = lane >> 4;
    const int in4 = D / 4, w4 = W / 4;
    for (int s = 0; s < 3; ++s) {
        const int64_t lo = a.seg_lo[s] * w4, hi = a.seg_hi[s] * w4;
        for (int64_t i = lo + (int64_t)blockIdx.x * kThreads + threadIdx.x; i < hi; i += (int64_t)gridDim.x * kThreads)
            st4(a.out + 4 * i, make_float4(0.f, 0.f, 0.f, 0.f));
    }
    if ((int64_t)blockIdx.x >= a.n_tiles) return;
    for (int i = threadIdx.x; i < M * kRows * LD; i += kThreads) Xt[i] = 0.f;
    for (int m = 0; m < M; ++m) stage_weight<4>(a.w + (size_t)m * D * D, D, D, 0, Ws + (size_t)m * a.IP * LD, a.IP, a.IP, LD);
    // A tile's rows travel through registers: all of a thread's loads go out together (kPreX + 2 kPreE float4s, M D <= 256
    // and D <= 128 bound them), and the NEXT tile's are in flight while this one is multiplied
    constexpr int kPreX = kThreads / kRows, kPreE = kRows * (128 / 4) / kThreads;
    float4 px[kPreX], pk[kPreE], pe[kPreE];
    const int n_x = M * kRows * in4, n_e = kRows * in4;
    auto tile_of = [&](int64_t T, bool &user, int64_t &r0, int64_t &num, int64_t &acc) {
        user = T < a.u_tiles;
        r0 = (user ? T : T - a.u_tiles) * kRows;
        num = user ? a.num_u : a.num_i;
        acc = user ? a.acc_u : a.acc_i;
    };
    auto fetch = [&](int64_t T) {
        bool user;
        int64_t r0, num, acc;
        tile_of(T, user, r0, num, acc);
        const float *emb = user ? a.ue : a.ie, *rk = user ? a.urk : a.irk;
#pragma unroll
        for (int j = 0; j < kPreX; ++j) {
            const int i = threadIdx.x + j * kThreads, mr = i / in4, c = 4 * (i - mr * in4), m = mr / kRows, rr = mr - m * kRows;
            px[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < n_x && r0 + rr < num) px[j] = ld4(a.t.e[m] + (acc + r0 + rr) * a.t.ld[m] + c);
        }
#pragma unroll
        for (int j = 0; j < kPreE; ++j) {
            const int i = threadIdx.x + j * kThreads, rr = i / in4, c = 4 * (i - rr * in4);
            pk[j] = pe[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < n_e && r0 + rr < num) {
                pk[j] = ld4(rk + (r0 + rr) * D + c);
                pe[j] = ld4(emb + (r0 + rr) * D + c);
            }
        }
    };
    fetch(blockIdx.x);
    for (int64_t T = blockIdx.x; T < a.n_tiles; T += gridDim.x) {
        bool user;
        int64_t r0, num, acc;
        tile_of(T, user, r0, num, acc);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kPreX; ++j) {
            const int i = threadIdx.x + j * kThreads, mr = i / in4, c = 4 * (i - mr * in4);
            if (i < n_x) st4(Xt + (size_t)mr * LD + c, px[j]);
        }
#pragma unroll
        for (int j = 0; j < kPreE; ++j) {
            const int i = threadIdx.x + j * kThreads, rr = i / in4, c = 4 * (i - rr * in4);
            if (i >= n_e || r0 + rr >= num) continue;
            st4(Rk + rr * LD + c, pk[j]);
            st4(a.out + (acc + r0 + rr) * W + c, pe[j]);
        }
        if (T + gridDim.x < a.n_tiles) fetch(T + gridDim.x);
        __syncthreads();
        sigmoid_sum<false>(Ws, Xt, nullptr, Ss, a.b, M, D, a.IP, LD, wave, n, g);
        __syncthreads();
        if (threadIdx.x < kRows && r0 + threadIdx.x < num) {
            const float *s = Ss + threadIdx.x * LD, *k = Rk + threadIdx.x * LD;
            float c = 0.f;
            for (int j = 0; j < D; j += 4) {
                const float4 x = ld4(s + j), y = ld4(k + j);
                c = fmaf(x.x, y.x, c); c = fmaf(x.y, y.y, c); c = fmaf(x.z, y.z, c); c = fmaf(x.w, y.w, c);
            }
            st4(a.out + (acc + r0 + threadIdx.x) * W + D, user ? make_float4(1.f, c, 0.f, 0.f) : make_float4(c, 1.f, 0.f, 0.f));
        }
    }
}

int check_common(const char *who, int D, int M, const float *const *tables_host, const int64_t *ld_host, const float *w, const float *b,
                 const float *ue, const float *ie, const float *urk, const float *irk, int64_t acc_u, int64_t num_u, int64_t acc_i,
                 int64_t num_i, int64_t N, HrTables *t) {
    PEA_REQUIRE(supported(D, M), PEA_ERR_ARG, "%s: width %d with %d tables is not supported (pea_herec_supported)", who, D, M);
    PEA_REQUIRE(tables_host && ld_host && w && b && ue && ie && urk && irk, PEA_ERR_ARG, "%s: null pointer", who);
    PEA_REQUIRE(aligned16(w) && aligned16(b) && aligned16(ue) && aligned16(ie) && aligned16(urk) && aligned16(irk), PEA_ERR_ARG,
                "%s: the weights and the embedding tables must start on 16-byte boundaries", who);
    PEA_REQUIRE(N > 0 && num_u > 0 && num_i > 0 && acc_u >= 0 && acc_i >= 0 && acc_u + num_u <= N && acc_i + num_i <= N, PEA_ERR_ARG,
                "%s: user block [%lld, +%lld) and item block [%lld, +%lld) must be non-empty and lie in the %lld nodes", who,
                (long long)acc_u, (long long)num_u, (long long)acc_i, (long long)num_i, (long long)N);
    for (int m = 0; m < M; ++m) {
        PEA_REQUIRE(tables_host[m] && aligned16(tables_host[m]) && ld_host[m] >= D && ld_host[m] % 4 == 0, PEA_ERR_ARG,
                    "%s: table %d: null, not 16-byte aligned, or row stride %lld (a multiple of 4, at least the width)", who, m,
                    (long long)ld_host[m]);
        t->e[m] = tables_host[m];
        t->ld[m] = ld_host[m];
    }
    return PEA_OK;
}

}  // namespace
}  // namespace pea

using namespace pea;

extern "C" int pea_herec_supported(int D, int M) { return supported(D, M) ? 1 : 0; }

extern "C" size_t pea_herec_train_workspace_bytes(int64_t B, int D, int M) {
    if (!supported(D, M) || B < 0) return 0;
    return part_offset(B, D, M) + (size_t)n_workgroups(B) * M * D * D * sizeof(float);
}

extern "C" int pea_herec_train(int64_t B, int D, int M, const float *const *tables_host, const int64_t *ld_host, const float *w,
                               const float *b, const float *user_emb, const float *item_emb, const float *user_rk_bias,
                               const float *item_rk_bias, int64_t acc_uids, int64_t num_uids, int64_t acc_iids, int64_t num_iids,
                               int64_t num_nodes, const int64_t *unids, const int64_t *inids, const float *labels, float *out_loss,
                               float *pred, float *dw, float *db, float *g_user, float *g_item, void *workspace,
                               size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    HrArgs a = {};
    PEA_TRY(check_common("herec_train", D, M, tables_host, ld_host, w, b, user_emb, item_emb, user_rk_bias, item_rk_bias, acc_uids,
                         num_uids, acc_iids, num_iids, num_nodes, &a.t));
    PEA_REQUIRE(B >= 0 && unids && inids && labels && out_loss && workspace, PEA_ERR_ARG, "herec_train: null pointer or B < 0");
    const bool bwd = dw != nullptr;
    PEA_REQUIRE((db != nullptr) == bwd && (g_user != nullptr) == bwd && (g_item != nullptr) == bwd, PEA_ERR_ARG,
                "herec_train: dw, db, g_user and g_item are all given or all NULL");
    PEA_REQUIRE(!bwd || (aligned16(g_user) && aligned16(g_item)), PEA_ERR_ARG, "herec_train: g_user and g_item must start on 16-byte boundaries");
    PEA_REQUIRE(workspace_bytes >= pea_herec_train_workspace_bytes(B, D, M), PEA_ERR_NOMEM, "herec_train: workspace too small");
    a.B = B; a.N = num_nodes; a.acc_u = acc_uids; a.num_u = num_uids; a.acc_i = acc_iids; a.num_i = num_iids;
    a.D = D; a.M = M; a.IP = ceil16(D); a.LD = a.IP + 4;
    a.w = w; a.b = b; a.ue = user_emb; a.ie = item_emb; a.urk = user_rk_bias; a.irk = item_rk_bias;
    a.unids = unids; a.inids = inids; a.labels = labels; a.pred = pred; a.g_user = g_user; a.g_item = g_item;
    a.err = ws_err_flag(workspace);
    a.sums = ws_sums(workspace);
    a.dbp = (float *)((char *)workspace + dbp_offset());
    a.part = (float *)((char *)workspace + part_offset(B, D, M));
    PEA_MEMSET_ASYNC(a.err, 0, sizeof(int), stream);
    const int n_wg = n_workgroups(B);
    if (n_wg > 0) {
        const double work = (double)B * 2.0 * M * 4.0 * D * (bwd ? 2.0 : 1.0);
        ProfScope ps("herec_train", stream, work);
        if (!bwd) {
            PEA_TRY((launch_train<1, 1, false>(a, n_wg, stream)));
        } else {
            switch (tiles_per_wave((a.IP / 16) * (a.IP / 16))) {      // dW tiles per wave and table
                case 1: PEA_TRY(launch_train_m<1>(a, n_wg, stream)); break;
                case 4: PEA_TRY(launch_train_m<4>(a, n_wg, stream)); break;
                case 8: PEA_TRY(launch_train_m<8>(a, n_wg, stream)); break;
                default: PEA_TRY(launch_train_m<16>(a, n_wg, stream)); break;
            }
        }
    }
    {
        const size_t wsz = (size_t)M * D * D, bsz = (size_t)M * D, total = bwd ? wsz + bsz : 1;
        ProfScope ps("herec_final", stream, (double)n_wg * total * 4.0);
        PEA_LAUNCH(herec_final_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, n_wg, B, wsz, bsz, (const float *)a.part,
                   (const float *)a.dbp, (const float *)a.sums, dw, db, out_loss);
        PEA_HIP(hipGetLastError());
    }
    return PEA_OK;
}

extern "C" int pea_herec_table(int D, int M, const float *const *tables_host, const int64_t *ld_host, const float *w, const float *b,
                               const float *user_emb, const float *item_emb, const float *user_rk_bias, const float *item_rk_bias,
                               int64_t acc_uids, int64_t num_uids, int64_t acc_iids, int64_t num_iids, int64_t num_nodes, float *out,
                               void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    HtArgs a = {};
    PEA_TRY(check_common("herec_table", D, M, tables_host, ld_host, w, b, user_emb, item_emb, user_rk_bias, item_rk_bias, acc_uids,
                         num_uids, acc_iids, num_iids, num_nodes, &a.t));
    PEA_REQUIRE(out && aligned16(out), PEA_ERR_ARG, "herec_table: out is null or not 16-byte aligned");
    PEA_REQUIRE(acc_uids + num_uids <= acc_iids || acc_iids + num_iids <= acc_uids, PEA_ERR_ARG,
                "herec_table: the user and the item block overlap");
    a.N = num_nodes; a.acc_u = acc_uids; a.num_u = num_uids; a.acc_i = acc_iids; a.num_i = num_iids;
    a.u_tiles = (num_uids + kRows - 1) / kRows;
    a.n_tiles = a.u_tiles + (num_iids + kRows - 1) / kRows;
    const bool user_first = acc_uids < acc_iids;
    const int64_t lo0 = user_first ? acc_uids : acc_iids, hi0 = lo0 + (user_first ? num_uids : num_iids);
    const int64_t lo1 = user_first ? acc_iids : acc_uids, hi1 = lo1 + (user_first ? num_iids : num_uids);
    a.seg_lo[0] = 0; a.seg_hi[0] = lo0;
    a.seg_lo[1] = hi0; a.seg_hi[1] = lo1;
    a.seg_lo[2] = hi1; a.seg_hi[2] = num_nodes;
    a.D = D; a.M = M; a.IP = ceil16(D); a.LD = a.IP + 4;
    a.w = w; a.b = b; a.ue = user_emb; a.ie = item_emb; a.urk = user_rk_bias; a.irk = item_rk_bias;
    a.out = out;
    const size_t lds = table_lds_bytes(D, M);
    const int n_wg = (int)std::min<int64_t>(a.n_tiles, kTblMaxWg);
    PEA_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(&herec_table_kernel), lds_limit(lds)));
    ProfScope ps("herec_table", stream, (double)(num_uids + num_iids) * 4.0 * D * (M + 3), (double)(num_uids + num_iids) * 4.0 * D * M,
                 (double)num_nodes * 4.0 * D * M);
    PEA_LAUNCH(herec_table_kernel, dim3(n_wg), dim3(kThreads), lds, stream, a);
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}
