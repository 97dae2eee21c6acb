// CFKG (reference models/cfkg.py): the kg_loss of experiments/cfkg_solver_bpr.py:95-106 and its whole backward in one launch,
// for gfx950.  Per quadruple (h, t+, t-, rel) with x [N, E] and r [R, E]:
//   hr = x[h] + r[rel],  pos = <hr, x[t+]>,  neg = <hr, x[t-]>
//   loss = -(sum_b log sigmoid(pos_b) + sum_b log sigmoid(-neg_b))
//   a = sigmoid(pos) - 1,  b = sigmoid(neg),  GH = a x[t+] + b x[t-]
//   d x[t+] = a hr,  d x[t-] = b hr,  d x[h] = GH,  d r[rel] = GH
// No product of matrices anywhere, so no MFMA: the launch is a gather of 4 B rows of E floats and a store of 3 B rows, and
// what it can save is latency and bytes.  A group of L lanes owns one quadruple (L the smallest power of two with
// 4 L >= E, 1..32): each lane holds one float4 of the four rows (zeros beyond E), forms hr in fp32 first as the reference
// does, runs the two dots as lane-local fma chains and adds them over the group with __shfl_xor.  Both halves of the
// loss term and a, b are bpr_term (train_common.h): bpr_term(pos) gives log sigmoid(pos) and a, bpr_term(-neg) gives
// log sigmoid(-neg) and -b.  A workgroup is 16 quadruples x L lanes (at least one wave) and walks its tiles of 16
// quadruples in a fixed order (tile blockIdx.x, + gridDim.x, ...); the grid is a function of B alone.
// The relation gradient is summed INSIDE the launch: R is small (the KG of the catalogue has 9 relations and one of
// them holds 98 % of the triples, which is the worst case of an LDS sort of equal ids), so every workgroup keeps one
// [R, E] partial in LDS.  The tile's GH rows are staged in LDS; thread c < E then walks the tile's 16 quadruples in
// row order and adds column c of each into row rel of the partial (the running row stays in a register while rel does
// not change: the same additions in the same order as a read-modify-write per quadruple).  The order of the additions
// is fixed by B, E and R and by which rows name which relation, never by timing.  Each workgroup writes its partial and
// its loss sum to the workspace; cfkg_final_kernel adds the partials in workgroup order (ordered_sum) and the loss sums in
// index order (store_loss).  No float atomics, bitwise reproducible, 64-bit row indexing.  A quadruple with an id out of
// range reads nothing through it, contributes nothing, gets three zero gradient rows and sets the error flag.
#include <algorithm>

#include "../../include/peahip_kge.h"
#include "train_common.h"

namespace pea {
namespace {

constexpr int kTQ = 16;       // quadruples of a tile
// workgroups = partials of d r: the final adds them one after the other, eight loads at a time, so its time grows with
// their number: with 128 a workgroup has one tile up to 2048 quadruples and three at the largest batch the node scatter takes
constexpr int kMaxWg = 128;

bool supported(int emb, int64_t num_rel) {
    return emb >= 4 && emb <= 128 && emb % 4 == 0 && num_rel >= 1 && num_rel <= PEA_CFKG_MAX_REL;
}

int lanes_of(int emb) {
    int l = 1;
    while (4 * l < emb) l *= 2;
    return l;
}

constexpr int block_threads(int L) { return kTQ * L < kWave ? kWave : kTQ * L; }

size_t lds_bytes(int emb, int num_rel, bool bwd) {
    const size_t small = 2 * kTQ;      // the loss terms and the relation ids of the tile
    return sizeof(float) * (small + (bwd ? (size_t)num_rel * emb + (size_t)kTQ * 4 * lanes_of(emb) : 0));
}

struct CfArgs {
    int64_t B, N;
    int R, E;
    const float *x, *r;
    int64_t ldx, ldr;
    const int64_t *quads;
    int64_t qs;
    float *pos, *neg;
    float *grad_rows;
    float *part, *sums;
    int *err;
};

extern __shared__ __attribute__((aligned(16))) float cf_smem[];

// L: lanes per quadruple; BWD = false: forward only (the same loss bits)
template <int L, bool BWD>
__global__ __launch_bounds__(block_threads(L)) void cfkg_train_kernel(const CfArgs a) {
    constexpr int W = 4 * L;                                        // floats of a staged GH row
    const int RE = a.R * a.E;
    float *part = cf_smem;                                          // [R][E]
    float *gh = part + (BWD ? RE : 0);                              // [kTQ][W]
    float *term = gh + (BWD ? kTQ * W : 0);                         // [kTQ]
    int *rel = reinterpret_cast<int *>(term + kTQ);                 // [kTQ], -1 = the row does not count
    const int q = threadIdx.x / L, l = threadIdx.x % L, c = 4 * l;
    const bool lane_on = q < kTQ, col_on = c < a.E;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    if (BWD)
        for (int i = 4 * threadIdx.x; i < RE; i += 4 * blockDim.x) st4(part + i, zero);
    const int64_t n_tiles = (a.B + kTQ - 1) / kTQ;
    float wg_loss = 0.f;
    for (int64_t T = blockIdx.x; T < n_tiles; T += gridDim.x) {
        __syncthreads();
        // ---- the quadruple's ids: a row beyond B or with an id out of range loads nothing and counts as zeros below
        const int64_t b = T * kTQ + q;
        const bool in = lane_on && b < a.B;
        int64_t id[4] = {0, 0, 0, 0};
        bool ok = in;
        if (in) {
#pragma unroll
            for (int j = 0; j < 4; ++j) id[j] = a.quads[b * a.qs + j];
            ok = id[0] >= 0 && id[0] < a.N && id[1] >= 0 && id[1] < a.N && id[2] >= 0 && id[2] < a.N && id[3] >= 0 && id[3] < a.R;
            if (!ok && l == 0) atomicOr(a.err, 1);
        }
        float4 h = zero, rv = zero, tp = zero, tn = zero;
        if (ok && col_on) {
            h = ld4(a.x + id[0] * a.ldx + c);
            rv = ld4(a.r + id[3] * a.ldr + c);
            tp = ld4(a.x + id[1] * a.ldx + c);
            tn = ld4(a.x + id[2] * a.ldx + c);
        }
        const float4 hr = make_float4(h.x + rv.x, h.y + rv.y, h.z + rv.z, h.w + rv.w);
        float pos = fmaf(hr.w, tp.w, fmaf(hr.z, tp.z, fmaf(hr.y, tp.y, fmaf(hr.x, tp.x, 0.f))));
        float neg = fmaf(hr.w, tn.w, fmaf(hr.z, tn.z, fmaf(hr.y, tn.y, fmaf(hr.x, tn.x, 0.f))));
#pragma unroll
        for (int off = L / 2; off > 0; off >>= 1) {      // every lane of the group ends with the whole sum
            pos += __shfl_xor(pos, off);
            neg += __shfl_xor(neg, off);
        }
        float t_pos, t_neg, ga, gb;
        bpr_term(pos, t_pos, ga);           // ga = sigmoid(pos) - 1 = a
        bpr_term(-neg, t_neg, gb);          // gb = sigmoid(-neg) - 1 = -b
        gb = -gb;
        if (lane_on && l == 0) {
            term[q] = ok ? t_pos + t_neg : 0.f;
            rel[q] = ok ? (int)id[3] : -1;
            if (a.pos && in) {
                a.pos[b] = ok ? pos : 0.f;
                a.neg[b] = ok ? neg : 0.f;
            }
        }
        if (BWD) {
            float4 g = zero, gp = zero, gn = zero;
            if (ok) {
                g = make_float4(ga * tp.x + gb * tn.x, ga * tp.y + gb * tn.y, ga * tp.z + gb * tn.z, ga * tp.w + gb * tn.w);
                gp = make_float4(ga * hr.x, ga * hr.y, ga * hr.z, ga * hr.w);
                gn = make_float4(gb * hr.x, gb * hr.y, gb * hr.z, gb * hr.w);
            }
            if (lane_on) st4(gh + q * W + c, g);
            if (in && col_on) {
                float *gr = a.grad_rows + 3 * b * a.E + c;      // rows 3b, 3b + 1, 3b + 2: h, t+, t-
                st4(gr, g);
                st4(gr + a.E, gp);
                st4(gr + 2 * a.E, gn);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            float s = 0.f;
            for (int k = 0; k < kTQ; ++k) s += term[k];      // row order inside the tile, tiles in the workgroup's order
            wg_loss += s;
        }
        // ---- d r: column threadIdx.x of the tile's GH rows into the rows of the partial, in row order
        if (BWD && threadIdx.x < a.E) {
            const int col = threadIdx.x;
            int cur = -1;
            float acc = 0.f;
            for (int k = 0; k < kTQ; ++k) {
                const int rk = rel[k];
                if (rk < 0) continue;
                if (rk != cur) {
                    if (cur >= 0) part[cur * a.E + col] = acc;
                    cur = rk;
                    acc = part[rk * a.E + col];
                }
                acc += gh[k * W + col];
            }
            if (cur >= 0) part[cur * a.E + col] = acc;
        }
    }
    if (threadIdx.x == 0) a.sums[blockIdx.x] = wg_loss;
    if (!BWD) return;
    __syncthreads();
    float *out = a.part + (size_t)blockIdx.x * RE;
    for (int i = 4 * threadIdx.x; i < RE; i += 4 * blockDim.x) st4(out + i, ld4(part + i));
}

// element e of d r = the workgroups' partials added in workgroup order; the loss = minus the workgroups' sums in index order
__global__ __launch_bounds__(256) void cfkg_final_kernel(int n_wg, int total, const float *__restrict__ part,
                                                        const float *__restrict__ sums, float *grad_r, float *loss) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (grad_r && e < total) grad_r[e] = ordered_sum(part + e, (size_t)total, n_wg);
    if (e == 0) store_loss(sums, n_wg, loss);
}

int n_workgroups(int64_t B) { return (int)std::min<int64_t>((B + kTQ - 1) / kTQ, kMaxWg); }

size_t part_offset() { return kWsSumsOffset + align256((size_t)kMaxWg * sizeof(float)); }

template <int L, bool BWD>
int launch_main(const CfArgs &a, int n_wg, hipStream_t stream) {
    PEA_LAUNCH((cfkg_train_kernel<L, BWD>), dim3(n_wg), dim3(block_threads(L)), lds_bytes(a.E, a.R, BWD), stream, a);
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}

template <bool BWD>
int launch_by_width(const CfArgs &a, int n_wg, hipStream_t stream) {
    switch (lanes_of(a.E)) {
        case 1: return launch_main<1, BWD>(a, n_wg, stream);
        case 2: return launch_main<2, BWD>(a, n_wg, stream);
        case 4: return launch_main<4, BWD>(a, n_wg, stream);
        case 8: return launch_main<8, BWD>(a, n_wg, stream);
        case 16: return launch_main<16, BWD>(a, n_wg, stream);
        default: return launch_main<32, BWD>(a, n_wg, stream);
    }
}

}  // namespace
}  // namespace pea

using namespace pea;

extern "C" int pea_cfkg_supported(int emb, int num_rel) { return supported(emb, num_rel) ? 1 : 0; }

extern "C" size_t pea_cfkg_train_workspace_bytes(int64_t B, int emb, int num_rel) {
    if (!supported(emb, num_rel) || B < 0) return 0;
    return part_offset() + (size_t)n_workgroups(B) * num_rel * emb * sizeof(float);
}

extern "C" int pea_cfkg_train(int64_t B, int emb, const float *x, int64_t ldx, int64_t num_nodes, const float *r, int64_t ldr,
                              int64_t num_rel, const int64_t *quads, int64_t quad_stride, float *out_loss, float *pos_pred,
                              float *neg_pred, float *grad_rows, float *grad_r, void *workspace, size_t workspace_bytes,
                              void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    PEA_REQUIRE(supported(emb, num_rel), PEA_ERR_ARG, "cfkg_train: width %d (a multiple of 4 in 4..128) with %lld relations (1..%d)", emb,
                (long long)num_rel, PEA_CFKG_MAX_REL);
    PEA_REQUIRE(B >= 0 && x && r && quads && out_loss && workspace, PEA_ERR_ARG, "cfkg_train: null pointer or B < 0");
    PEA_REQUIRE(aligned16(x) && aligned16(r), PEA_ERR_ARG, "cfkg_train: x and r must start on 16-byte boundaries");
    PEA_REQUIRE(ldx >= emb && ldx % 4 == 0 && ldr >= emb && ldr % 4 == 0, PEA_ERR_ARG,
                "cfkg_train: row strides %lld / %lld (multiples of 4, at least the width)", (long long)ldx, (long long)ldr);
    PEA_REQUIRE(num_nodes > 0 && quad_stride >= 4, PEA_ERR_ARG, "cfkg_train: %lld nodes, quadruple stride %lld (>= 4)",
                (long long)num_nodes, (long long)quad_stride);
    PEA_REQUIRE((pos_pred == nullptr) == (neg_pred == nullptr), PEA_ERR_ARG, "cfkg_train: pos_pred and neg_pred go together");
    const bool bwd = grad_rows != nullptr;
    PEA_REQUIRE((grad_r != nullptr) == bwd, PEA_ERR_ARG, "cfkg_train: grad_rows and grad_r are both given or both NULL");
    PEA_REQUIRE(!bwd || (aligned16(grad_rows) && aligned16(grad_r)), PEA_ERR_ARG,
                "cfkg_train: grad_rows and grad_r must start on 16-byte boundaries");
    PEA_REQUIRE(workspace_bytes >= pea_cfkg_train_workspace_bytes(B, emb, (int)num_rel), PEA_ERR_NOMEM,
                "cfkg_train: workspace too small");
    CfArgs a = {};
    a.B = B; a.N = num_nodes; a.R = (int)num_rel; a.E = emb;
    a.x = x; a.r = r; a.ldx = ldx; a.ldr = ldr; a.quads = quads; a.qs = quad_stride;
    a.pos = pos_pred; a.neg = neg_pred; a.grad_rows = grad_rows;
    a.err = ws_err_flag(workspace);
    a.sums = ws_sums(workspace);
    a.part = (float *)((char *)workspace + part_offset());
    PEA_MEMSET_ASYNC(a.err, 0, sizeof(int), stream);
    const int n_wg = n_workgroups(B);
    const int total = bwd ? a.R * emb : 1;
    if (n_wg > 0) {
        const double bytes = (double)B * emb * 4.0 * (bwd ? 7.0 : 4.0) + (bwd ? (double)n_wg * total * 4.0 : 0.0);
        ProfScope ps("cfkg_train", stream, bytes);
        if (bwd) {
            PEA_TRY(launch_by_width<true>(a, n_wg, stream));
        } else {
            PEA_TRY(launch_by_width<false>(a, n_wg, stream));
        }
    }
    {
        ProfScope ps("cfkg_final", stream, (double)n_wg * total * 4.0);
        PEA_LAUNCH(cfkg_final_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, n_wg, total, (const float *)a.part,
                   (const float *)a.sums, grad_r, out_loss);
        PEA_HIP(hipGetLastError());
    }
    return PEA_OK;
}
