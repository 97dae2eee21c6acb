// KG phase of KGAT / KGCN: the TransR-style loss of experiments/kgat_solver_bpr.py:110-124 (kg_loss) and its whole backward in
// one launch, for gfx950.  Per quadruple (h, t+, t-, rel) with x [N, E], P = proj_mat [E, E], r [R, E]:
//   hp = x[h] P + r[rel],  dpos = hp - x[t+] P,  dneg = hp - x[t-] P,  pos = sum_c dpos_c^2,  neg = sum_c dneg_c^2
//   loss = -sum_b log sigmoid(pos_b - neg_b)                       (sign and form as the reference has them)
//   g = -(1 - sigmoid(pos - neg)),  G+ = 2 g dpos,  G- = -2 g dneg,  GH = G+ + G-
//   d x[h] = GH P^T,  d x[t+] = -(G+) P^T,  d x[t-] = -(G-) P^T,  d r[rel] = GH,  dP = x[h]^T GH - x[t+]^T G+ - x[t-]^T G-
// Built from the tile toolkit of tile16.h: one workgroup = 4 waves walks its tiles of 16 quadruples in a fixed order (tile
// blockIdx.x, + gridDim.x, ...).  P sits in LDS once per workgroup (stage_weight: zero rows / columns up to ceil16(E)); the
// tile's three operands [H; T+; T-] are staged in LDS with 16-byte loads.  Every product runs from a zero accumulator with k
// ascending, in the transposed orientation (P is the A operand, the data rows the B operand, rows_times_w): lane (n, g) ends
// up with columns 16 u + 4 g .. + 3 of ROW n.  The three forward products stay separate, as the reference has them (three
// chains in one k-loop).  dpos / dneg go through LDS; pos and neg are fma chains in ascending column order, eight of
// them (column c in chain c % 8, added pairwise at the end): one chain over 128 squares that sum to ~16 leaves an error of
// ~8e-6 in pos - neg, four times that of torch's tree sum, and g = d loss / d pos carries it into every gradient (dP at
// E = 128 then misses the fp32 criterion of the tests); with eight the error is torch's.  The loss term and g are
// bpr_term (train_common.h).  Backward: [GH; G+; G-] pass through LDS once: they are the B operand of the three row
// products with P^T (rows_times_wt) and of dP = [H; T+; T-]^T [GH; -G+; -G-] (the tile's 48 rows as k; the sign rides on
// the A operand).  The dP tiles are dealt out to the four waves and stay in their accumulators over all
// tiles of the workgroup: one partial per workgroup (dw_store), added in workgroup order by transr_final_kernel
// (ordered_sum), which also adds the workgroups' loss sums in index order (store_loss).
// No float atomics, grid = f(B), bitwise reproducible, 64-bit row indexing.  A quadruple with an id out of range is staged
// as zero rows (nothing is read through it), contributes nothing, gets zero gradient rows and sets the error flag.
#include <algorithm>

#include "tile16.h"
#include "train_common.h"

namespace pea {
namespace {

constexpr int kMaxWg = 256;                   // partials of dP: one workgroup per CU

bool supported(int emb) { return emb >= 4 && emb <= 128 && emb % 4 == 0; }

// floats behind the tiles: g and the loss term per row, the row's validity, its four ids (as int64)
constexpr int kSmallFloats = 16 + 16 + 16 + 2 * 4 * kTR;

size_t lds_bytes(int emb, bool bwd) {
    const int ip = ceil16(emb), ld = ip + 4;
    return sizeof(float) * ((size_t)ip * ld + (size_t)(3 + 2 + (bwd ? 3 : 0)) * kTR * ld + kSmallFloats);
}

struct TrArgs {
    int64_t B, N, R;
    int E, IP, LD;
    const float *x, *proj, *r;
    int64_t ldx, ldr;
    const int64_t *quads;
    int64_t qs;
    float *pos, *neg;
    float *grad_rows, *grad_rel;
    float *part, *sums;
    int *err;
};

extern __shared__ __attribute__((aligned(16))) float trs_smem[];

// NT: dP tiles per wave (tile id = wave + 4 q -> input tile id / IT, output tile id % IT); BWD = false: forward only
template <int NT, bool BWD>
__global__ __launch_bounds__(kThreads) void transr_train_kernel(const TrArgs a) {
    const int LD = a.LD;
    float *Ps = trs_smem;
    float *Xt = Ps + a.IP * LD;                   // [H; T+; T-], 48 rows
    float *Dt = Xt + 3 * kTR * LD;                // [dpos; dneg], 32 rows
    float *Gt = Dt + 2 * kTR * LD;                // [GH; G+; G-], 48 rows (backward only)
    float *sm = Gt + (BWD ? 3 * kTR * LD : 0);
    float *gco = sm, *term = sm + 16;
    int *valid = reinterpret_cast<int *>(sm + 32);
    int64_t *ids = reinterpret_cast<int64_t *>(sm + 48);      // [4][16]: h, t+, t-, rel of the tile's rows
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, n = lane & 15, g = lane >> 4;
    const int64_t n_tiles = (a.B + kTR - 1) / kTR;
    const int IT = a.IP / 16, in4 = a.E / 4, ip4 = a.IP / 4;
    for (int i = threadIdx.x; i < 3 * kTR * LD; i += kThreads) Xt[i] = 0.f;      // the pad columns stay zero
    stage_weight<4>(a.proj, a.E, a.E, 0, Ps, a.IP, a.IP, LD);
    f32x4 dp[1][NT] = {};
    float wg_loss = 0.f;
    for (int64_t T = blockIdx.x; T < n_tiles; T += gridDim.x) {
        __syncthreads();
        // ---- the tile's ids: a row beyond B or with an id out of range is a zero row everywhere below
        if (threadIdx.x < kTR) {
            const int64_t b = T * kTR + threadIdx.x;
            int64_t q[4] = {0, 0, 0, 0};
            bool ok = b < a.B;
            if (ok) {
#pragma unroll
                for (int j = 0; j < 4; ++j) q[j] = a.quads[b * a.qs + j];
                ok = q[0] >= 0 && q[0] < a.N && q[1] >= 0 && q[1] < a.N && q[2] >= 0 && q[2] < a.N && q[3] >= 0 && q[3] < a.R;
                if (!ok) atomicOr(a.err, 1);
            }
            valid[threadIdx.x] = ok ? 1 : 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) ids[j * kTR + threadIdx.x] = ok ? q[j] : 0;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < 3 * kTR * in4; i += kThreads) {
            const int rr = i / in4, c = 4 * (i - rr * in4);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid[rr & 15]) v = ld4(a.x + ids[rr] * a.ldx + c);
            st4(Xt + rr * LD + c, v);
        }
        __syncthreads();
        // ---- x[.] P per output tile u: register r of lane (n, g) = row n, column 16 u + 4 g + r; then dpos / dneg
        for (int u = wave; u < IT; u += kWaves) {
            f32x4 z[3] = {};
            rows_times_w<1, 3>(Ps, a.IP, LD, Xt, LD, in4, u, n, g, z);
            const f32x4 &zh = z[0], &zp = z[1], &zn = z[2];
            const int lc = 16 * u + 4 * g;
            float4 rv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid[n] && lc < a.E) rv = ld4(a.r + ids[3 * kTR + n] * a.ldr + lc);
            const float hp[4] = {zh[0] + rv.x, zh[1] + rv.y, zh[2] + rv.z, zh[3] + rv.w};
            st4(Dt + n * LD + lc, make_float4(hp[0] - zp[0], hp[1] - zp[1], hp[2] - zp[2], hp[3] - zp[3]));
            st4(Dt + (kTR + n) * LD + lc, make_float4(hp[0] - zn[0], hp[1] - zn[1], hp[2] - zn[2], hp[3] - zn[3]));
        }
        __syncthreads();
        // ---- pos (lanes 0..15) and neg (lanes 16..31) of wave 0: eight fma chains over the columns, then the loss term and g
        if (wave == 0) {
            float s = 0.f;
            if (lane < 2 * kTR) {
                const float *d = Dt + lane * LD;
                float q[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // column c goes to chain c % 8
                for (int c = 0; c < a.E; c += 8) {
                    const float4 v = ld4(d + c);
                    q[0] = fmaf(v.x, v.x, q[0]); q[1] = fmaf(v.y, v.y, q[1]); q[2] = fmaf(v.z, v.z, q[2]); q[3] = fmaf(v.w, v.w, q[3]);
                    if (c + 4 < a.E) {
                        const float4 w = ld4(d + c + 4);
                        q[4] = fmaf(w.x, w.x, q[4]); q[5] = fmaf(w.y, w.y, q[5]); q[6] = fmaf(w.z, w.z, q[6]); q[7] = fmaf(w.w, w.w, q[7]);
                    }
                }
                s = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
            }
            const float other = __shfl(s, (lane + kTR) & (kWave - 1));
            if (lane < kTR) {
                const bool ok = valid[lane] != 0;
                const float pos = ok ? s : 0.f, neg = ok ? other : 0.f, d = pos - neg;
                bpr_term(d, term[lane], gco[lane]);      // gco: d loss / d pos;  d loss / d neg = -g
                if (!ok) term[lane] = gco[lane] = 0.f;
                const int64_t b = T * kTR + lane;
                if (a.pos && b < a.B) {
                    a.pos[b] = pos;
                    a.neg[b] = neg;
                }
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            float s = 0.f;
            for (int k = 0; k < kTR; ++k) s += term[k];      // row order inside the tile, tiles in the workgroup's order
            wg_loss += s;
        }
        if (!BWD) continue;
        // ---- [GH; G+; G-] into LDS (zero for rows that do not count and columns >= E); GH is d r[rel] of the row
        for (int i = threadIdx.x; i < kTR * ip4; i += kThreads) {
            const int rr = i / ip4, c = 4 * (i - rr * ip4);
            const float4 dv = ld4(Dt + rr * LD + c), ev = ld4(Dt + (kTR + rr) * LD + c);
            const float g2 = 2.0f * gco[rr];
            const float4 gp = make_float4(g2 * dv.x, g2 * dv.y, g2 * dv.z, g2 * dv.w);
            const float4 gn = make_float4(-g2 * ev.x, -g2 * ev.y, -g2 * ev.z, -g2 * ev.w);
            float4 gh = make_float4(gp.x + gn.x, gp.y + gn.y, gp.z + gn.z, gp.w + gn.w);
            st4(Gt + rr * LD + c, gh);
            st4(Gt + (kTR + rr) * LD + c, gp);
            st4(Gt + (2 * kTR + rr) * LD + c, gn);
            const int64_t b = T * kTR + rr;
            if (b < a.B && c < a.E) {
                if (!valid[rr]) gh = make_float4(0.f, 0.f, 0.f, 0.f);
                st4(a.grad_rel + b * a.E + c, gh);
            }
        }
        __syncthreads();
        // ---- G P^T per input tile v: register r of lane (n, g) = row n, input 16 v + 4 g + r
        for (int v = wave; v < IT; v += kWaves) {
            f32x4 e[3] = {};
            rows_times_wt<1, 3>(Ps, a.IP, LD, Gt, LD, in4, v, n, g, e);
            const f32x4 &e0 = e[0], &e1 = e[1], &e2 = e[2];
            const int col = 16 * v + 4 * g;
            const int64_t b = T * kTR + n;
            if (b >= a.B || col >= a.E) continue;
            float4 r0 = make_float4(e0[0], e0[1], e0[2], e0[3]), r1 = make_float4(-e1[0], -e1[1], -e1[2], -e1[3]),
                   r2 = make_float4(-e2[0], -e2[1], -e2[2], -e2[3]);
            if (!valid[n]) r0 = r1 = r2 = make_float4(0.f, 0.f, 0.f, 0.f);
            float *gr = a.grad_rows + 3 * b * a.E + col;
            st4(gr, r0);
            st4(gr + a.E, r1);
            st4(gr + 2 * a.E, r2);
        }
        // ---- dP += [H; T+; T-]^T [GH; -G+; -G-] over the tile's 48 rows (12 k-steps): register r of lane (n, g) =
        //      dP[16 v + 4 g + r][16 u + n]  (written out here and in kg_update.hip, tile16.h says why)
#pragma unroll
        for (int q = 0; q < NT; ++q) {
            const int id = wave + kWaves * q;
            if (id >= IT * IT) continue;
            const int v = id / IT, u = id - v * IT;
            const int ao = g * LD + 16 * v + n, zo = g * LD + 16 * u + n;
#pragma unroll
            for (int t = 0; t < 12; ++t) {
                const float xv = Xt[ao + 4 * t * LD];
                dp[0][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(t < 4 ? xv : -xv, Gt[zo + 4 * t * LD], dp[0][q], 0, 0, 0);
            }
        }
    }
    if (threadIdx.x == 0) a.sums[blockIdx.x] = wg_loss;
    if (!BWD) return;
    dw_store<NT, 1>(dp, a.part + (size_t)blockIdx.x * a.E * a.E, 0, a.E, a.E, 0, IT, IT, wave, n, g);
}

// element e of dP = the workgroups' partials added in workgroup order; the loss = minus the workgroups' sums in index order
__global__ __launch_bounds__(256) void transr_final_kernel(int n_wg, int emb, const float *__restrict__ part,
                                                          const float *__restrict__ sums, float *dproj, float *loss) {
    const size_t wsz = (size_t)emb * emb, e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (dproj && e < wsz) dproj[e] = ordered_sum(part + e, wsz, n_wg);
    if (e == 0) store_loss(sums, n_wg, loss);
}

int n_workgroups(int64_t B) { return (int)std::min<int64_t>((B + kTR - 1) / kTR, kMaxWg); }

size_t part_offset() { return kWsSumsOffset + align256((size_t)kMaxWg * sizeof(float)); }

template <int NT, bool BWD>
int launch_main(const TrArgs &a, int n_wg, hipStream_t stream) {
    const size_t lds = lds_bytes(a.E, BWD);
    PEA_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(&transr_train_kernel<NT, BWD>), lds_limit(lds)));
    PEA_LAUNCH((transr_train_kernel<NT, BWD>), dim3(n_wg), dim3(kThreads), lds, stream, a);
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}

}  // namespace
}  // namespace pea

using namespace pea;

extern "C" int pea_transr_supported(int emb) { return supported(emb) ? 1 : 0; }

extern "C" size_t pea_transr_train_workspace_bytes(int64_t B, int emb) {
    if (!supported(emb) || B < 0) return 0;
    return part_offset() + (size_t)n_workgroups(B) * emb * emb * sizeof(float);
}

extern "C" int pea_transr_train(int64_t B, int emb, const float *x, int64_t ldx, int64_t num_nodes, const float *proj,
                                const float *r, int64_t ldr, int64_t num_rel, const int64_t *quads, int64_t quad_stride,
                                float *out_loss, float *pos_pred, float *neg_pred, float *grad_rows, float *grad_rel_rows,
                                float *dproj, void *workspace, size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    PEA_REQUIRE(supported(emb), PEA_ERR_ARG, "transr_train: width %d (a multiple of 4 in 4..128)", emb);
    PEA_REQUIRE(B >= 0 && x && proj && r && quads && out_loss && workspace, PEA_ERR_ARG, "transr_train: null pointer or B < 0");
    PEA_REQUIRE(aligned16(x) && aligned16(proj) && aligned16(r), PEA_ERR_ARG, "transr_train: x, proj and r must start on 16-byte boundaries");
    PEA_REQUIRE(ldx >= emb && ldx % 4 == 0 && ldr >= emb && ldr % 4 == 0, PEA_ERR_ARG,
                "transr_train: row strides %lld / %lld (multiples of 4, at least the width)", (long long)ldx, (long long)ldr);
    PEA_REQUIRE(num_nodes > 0 && num_rel > 0 && quad_stride >= 4, PEA_ERR_ARG, "transr_train: %lld nodes, %lld relations, quadruple stride %lld (>= 4)",
                (long long)num_nodes, (long long)num_rel, (long long)quad_stride);
    PEA_REQUIRE((pos_pred == nullptr) == (neg_pred == nullptr), PEA_ERR_ARG, "transr_train: pos_pred and neg_pred go together");
    const bool bwd = grad_rows != nullptr;
    PEA_REQUIRE((grad_rel_rows != nullptr) == bwd && (dproj != nullptr) == bwd, PEA_ERR_ARG,
                "transr_train: grad_rows, grad_rel_rows and dproj are all given or all NULL");
    PEA_REQUIRE(!bwd || (aligned16(grad_rows) && aligned16(grad_rel_rows)), PEA_ERR_ARG,
                "transr_train: grad_rows and grad_rel_rows must start on 16-byte boundaries");
    PEA_REQUIRE(workspace_bytes >= pea_transr_train_workspace_bytes(B, emb), PEA_ERR_NOMEM, "transr_train: workspace too small");
    TrArgs a = {};
    a.B = B; a.N = num_nodes; a.R = num_rel; a.E = emb; a.IP = ceil16(emb); a.LD = a.IP + 4;
    a.x = x; a.proj = proj; a.r = r; a.ldx = ldx; a.ldr = ldr; a.quads = quads; a.qs = quad_stride;
    a.pos = pos_pred; a.neg = neg_pred; a.grad_rows = grad_rows; a.grad_rel = grad_rel_rows;
    a.err = ws_err_flag(workspace);
    a.sums = ws_sums(workspace);
    a.part = (float *)((char *)workspace + part_offset());
    PEA_MEMSET_ASYNC(a.err, 0, sizeof(int), stream);
    const int n_wg = n_workgroups(B);
    if (n_wg > 0) {
        const double work = (double)B * 4.0 * emb * (bwd ? 8.0 : 4.0);
        ProfScope ps("transr_train", stream, work);
        if (!bwd) {
            PEA_TRY((launch_main<1, false>(a, n_wg, stream)));
        } else {
            switch (tiles_per_wave((a.IP / 16) * (a.IP / 16))) {      // dP tiles per wave: 1, 4, 8 or 16 for the widths taken
                case 1: PEA_TRY((launch_main<1, true>(a, n_wg, stream))); break;
                case 4: PEA_TRY((launch_main<4, true>(a, n_wg, stream))); break;
                case 8: PEA_TRY((launch_main<8, true>(a, n_wg, stream))); break;
                default: PEA_TRY((launch_main<16, true>(a, n_wg, stream))); break;
            }
        }
    }
    {
        const size_t total = bwd ? (size_t)emb * emb : 1;
        ProfScope ps("transr_final", stream, (double)n_wg * total * 4.0);
        PEA_LAUNCH(transr_final_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, n_wg, emb, (const float *)a.part,
                   (const float *)a.sums, dproj, out_loss);
        PEA_HIP(hipGetLastError());
    }
    return PEA_OK;
}
