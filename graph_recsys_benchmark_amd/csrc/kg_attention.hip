// Edge softmax and the KGAT / KGCN attention maps over destination-sorted CSR for gfx950 (wave64).
//
// Replaces the reference's attention-map update of its two KG baselines (graph_recsys_benchmark/experiments/
// kgat_solver_bpr.py:313-320, kgcn_solver_bpr.py:313-319) and the torch_geometric.utils.softmax (PyG 1.5.0) they call:
//   KGAT  alpha_e = sum_d xp[i,d] * tanh(xp[j,d] + s_e r[|t_e|, d])      xp = x @ proj_mat
//   KGCN  alpha_e = sum_d x[i,d] * s_e r[|t_e|, d]
//   att_e = exp(alpha_e - max_{e' -> i} alpha_e') / (sum_{e' -> i} exp(alpha_e' - max) + 1e-16)
// for every edge e = (j -> i) of type t_e, s_e = -1 where t_e < 0, else +1 (a reversed type-0 edge keeps +r[0]).
// No [E, emb] temporaries and no float atomics: the score of an edge is computed, used for its row's online (max, sum)
// and parked (LDS, or a slot-order scratch for hub chunks) for the normalising write, all in a fixed order, so results
// are bitwise reproducible run to run.
//
// Work layout (the plan's degree classes, csrc/plan.hip):
//   short rows : one G-lane subgroup per destination row (a lane per row for the scalar modes), edges in sequence
//   long rows  : one wave per row; NSG = 64 / G subgroups take the edges round-robin, U edges in flight each
//   hub rows   : one wave per <= 512-edge chunk writes an (m, s) record; es_merge folds the records in chunk order,
//                es_finish writes the chunk's edges
// G lanes x float4 hold one row of `emb` columns (emb a multiple of 4, <= 256): the destination row is loaded once per
// CSR row, the source row xp[j] and r[|t|] (a table of a few dozen rows) once per edge.
#include <algorithm>

#include "agg_common.h"

namespace pea {
namespace {

enum EsMode { ES_SOFTMAX = 0, ES_BWD = 1, ES_KGAT = 2, ES_KGCN = 3 };
constexpr int kShortCap = 32;       // LDS score slots per short-row subgroup (kShortDeg)
constexpr int kLdsFloats = 2048;    // 4 waves x kChunk long-item slots = (256 / 4 lanes) x kShortCap short-row slots

struct EsArgs {
    const int *rowptr, *col, *eid, *short_rows;
    const LongItem *long_items;
    const int *hub_first, *hub_count;
    int n_short, n_long, n_hub, n_long_blocks;
    const float *src;      // SOFTMAX: scores, BWD: forward output y (COO order)
    const float *grad;     // BWD: output gradient (COO order)
    const float *xd;       // KG: destination-side rows (KGAT: xp, KGCN: x), stride ld
    const float *xs;       // KGAT: source rows (xp), stride ld
    const float *rel;      // KG: r [num_types, emb] (row stride emb)
    const int *types;      // KG: signed edge type per CSR slot (pea_kg_edge_types)
    int emb, ld;
    float *out;            // [E] COO order
    float2 *rec;           // [n_slots] per hub chunk: (m, s) / (partial dot, 0)
    float2 *fin;           // [n_slots] the chunk's row state after the merge
    float *scratch;        // [e_kept] KG: scores in CSR slot order (hub chunks, oversized items)
};

// tanh from one v_exp_f32 and one v_rcp_f32: tanh|x| = (1 - 2^(-2 log2(e) |x|)) / (1 + 2^(...)).  Absolute error a few
// 1e-8 (relative error grows for |x| < 1e-3, where the product with xp[i,d] makes it irrelevant); DESIGN.md section 9.
__device__ __forceinline__ float tanh_fast(float x) {
    const float t = __builtin_amdgcn_exp2f(-2.0f * kLog2e * fabsf(x));
    return copysignf((1.0f - t) * __builtin_amdgcn_rcpf(1.0f + t), x);
}

// Scores of U edges (e[u] valid where ok[u]); every lane of the G-lane subgroup ends with the same values.
template <int MODE, int G, int U>
__device__ __forceinline__ void scores(const EsArgs &A, const int (&e)[U], const bool (&ok)[U], float4 xi, int c4,
                                       float (&a)[U]) {
    if (MODE == ES_SOFTMAX) {
#pragma unroll
        for (int u = 0; u < U; ++u) a[u] = ok[u] ? A.src[A.eid[e[u]]] : 0.f;
        return;
    }
    if (MODE == ES_BWD) {   // y_e g_e (terms of the row's segmented dot)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int id = ok[u] ? A.eid[e[u]] : 0;
            a[u] = ok[u] ? A.src[id] * A.grad[id] : 0.f;
        }
        return;
    }
    int t[U], j[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        t[u] = ok[u] ? A.types[e[u]] : 0;
        if (MODE == ES_KGAT) j[u] = ok[u] ? A.col[e[u]] : 0;
    }
    float4 r[U], h[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        r[u] = ld4(A.rel + (size_t)(t[u] < 0 ? -t[u] : t[u]) * A.emb + c4);
        if (MODE == ES_KGAT) h[u] = ld4(row_at(A.xs, j[u], A.ld) + c4);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const float s = t[u] < 0 ? -1.f : 1.f;
        const float4 sr = make_float4(s * r[u].x, s * r[u].y, s * r[u].z, s * r[u].w);   // trans_vec (exact)
        float d;
        if (MODE == ES_KGAT) {
            const float4 th = make_float4(tanh_fast(h[u].x + sr.x), tanh_fast(h[u].y + sr.y), tanh_fast(h[u].z + sr.z),
                                          tanh_fast(h[u].w + sr.w));
            d = dot4(xi, th);
        } else {
            d = dot4(xi, sr);
        }
        a[u] = G > 1 ? head_sum<G>(d, 0, 0, G, true) : d;
    }
}

// Online row state: forward (m in the log2 domain, s = sum 2^(a log2 e - m)) as in agg_common.h's Soft; backward: the
// segmented dot in s (m unused).
template <int MODE>
__device__ __forceinline__ void state_push(float &m, float &s, const float *a, const bool *ok, int n) {
    if (MODE == ES_BWD) {
        for (int u = 0; u < n; ++u) s += a[u];
        return;
    }
    float mx = -INFINITY;
    for (int u = 0; u < n; ++u) mx = fmaxf(mx, ok[u] ? a[u] : -INFINITY);
    const float mn = fmaxf(m, mx * kLog2e);
    s *= __builtin_amdgcn_exp2f(m - mn);
    m = mn;
    for (int u = 0; u < n; ++u) s += ok[u] ? __builtin_amdgcn_exp2f(fmaf(a[u], kLog2e, -mn)) : 0.f;
}

template <int MODE>
__device__ __forceinline__ void state_merge(float &m, float &s, float m2, float s2) {
    if (MODE == ES_BWD) {
        s += s2;
        return;
    }
    const float mn = fmaxf(m, m2);
    s = s * __builtin_amdgcn_exp2f(m - mn) + s2 * __builtin_amdgcn_exp2f(m2 - mn);
    m = mn;
}

// The normalised value of one edge from its row's final state (m, inv = 1 / (s + 1e-16); BWD: m = sum_e' y g).
template <int MODE>
__device__ __forceinline__ void finish_edge(const EsArgs &A, int e, float a, float m, float inv) {
    const int id = A.eid[e];
    if (MODE == ES_BWD) {
        A.out[id] = A.src[id] * (A.grad[id] - m);
        return;
    }
    if (MODE == ES_SOFTMAX) a = A.src[id];
    A.out[id] = __builtin_amdgcn_exp2f(fmaf(a, kLog2e, -m)) * inv;
}

// One CSR item (a whole row, or a hub chunk when slot >= 0) worked by `nsub` G-lane subgroups (this lane's subgroup is
// `sub`, its column slot `sl`); `len_loop` >= end - beg is the trip count every lane of the wave runs (cross-lane sums).
// buf: where the KG scores of a direct item are parked (LDS, or the slot-order scratch when the item is longer than
// `cap`); hub chunks always park them in the scratch for es_finish.
template <int MODE, int G, int U>
__device__ __forceinline__ void do_item(const EsArgs &A, int row, int beg, int end, int slot, int sub, int nsub, int sl,
                                        int tl, int len_loop, float *lds, int cap) {
    constexpr bool KG = MODE == ES_KGAT || MODE == ES_KGCN;
    const bool active = sl * 4 < A.emb;
    const int c4 = active ? sl * 4 : 0;
    float4 xi = make_float4(0.f, 0.f, 0.f, 0.f);
    if (KG && active && end > beg) xi = ld4(row_at(A.xd, row, A.ld) + c4);
    float *buf = (slot >= 0 || end - beg > cap) ? A.scratch + beg : lds;
    float m = kNegBig, s = 0.f;
    for (int b = 0; b < len_loop; b += nsub * U) {
        int e[U];
        bool ok[U];
        float a[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = b + u * nsub + sub;
            ok[u] = beg + k < end;
            e[u] = ok[u] ? beg + k : beg;
        }
        scores<MODE, G, U>(A, e, ok, xi, c4, a);
        state_push<MODE>(m, s, a, ok, U);
        if (KG && sl == 0) {
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (ok[u]) buf[e[u] - beg] = a[u];
        }
    }
    // fold the subgroups of the team (fixed xor butterfly: every lane ends with the same state)
    for (int off = G; off < nsub * G; off <<= 1) state_merge<MODE>(m, s, __shfl_xor(m, off), __shfl_xor(s, off));
    if (slot >= 0) {
        if (tl == 0) A.rec[slot] = make_float2(m, s);
        return;
    }
    if (end <= beg) return;
    if (KG) {   // the parked scores were written by other lanes of this wave
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    const float inv = MODE == ES_BWD ? 0.f : 1.0f / (s + 1e-16f);
    const float mm = MODE == ES_BWD ? s : m;
    for (int e = beg + tl; e < end; e += nsub * G) finish_edge<MODE>(A, e, KG ? buf[e - beg] : 0.f, mm, inv);
}

// workgroups [0, n_long_blocks): long rows and hub chunks, one wave per item (4 per workgroup, the plan's order);
// the rest: short rows, one G-lane subgroup per row
template <int MODE, int G>
__global__ __launch_bounds__(kBlock) void es_rows_kernel(const EsArgs A) {
    constexpr bool KG = MODE == ES_KGAT || MODE == ES_KGCN;
    __shared__ float lds[KG ? kLdsFloats : 1];
    const int lane = (int)threadIdx.x % kWave, wave = (int)threadIdx.x / kWave;
    if ((int)blockIdx.x < A.n_long_blocks) {
        const int item = (int)blockIdx.x * (kBlock / kWave) + wave;
        if (item >= A.n_long) return;  // wave-uniform
        const LongItem it = A.long_items[item];
        if (it.slot == -2) return;      // padding of the XCD-affine item layout
        do_item<MODE, G, 4>(A, it.row, it.beg, it.end, it.slot, lane / G, kWave / G, lane % G, lane, it.end - it.beg,
                            lds + wave * kChunk, kChunk);
        return;
    }
    const int q = ((int)blockIdx.x - A.n_long_blocks) * (kBlock / G) + (int)threadIdx.x / G;
    const int row = q < A.n_short ? A.short_rows[q] : 0;
    const int beg = q < A.n_short ? A.rowptr[row] : 0;
    const int end = q < A.n_short ? A.rowptr[row + 1] : 0;
    int len = end - beg;
    if (G > 1)
        for (int off = G; off < kWave; off <<= 1) len = max(len, __shfl_xor(len, off));
    do_item<MODE, G, 1>(A, row, beg, end, -1, 0, 1, lane % G, lane % G, len, lds + ((int)threadIdx.x / G) * kShortCap,
                        KG ? kShortCap : 0);
}

// hub rows: one wave per row folds its chunk records in chunk order and hands the row state to every chunk
template <int MODE>
__global__ __launch_bounds__(kBlock) void es_merge_kernel(const EsArgs A) {
    const int h = (int)blockIdx.x * (kBlock / kWave) + (int)threadIdx.x / kWave;
    const int lane = (int)threadIdx.x % kWave;
    if (h >= A.n_hub) return;
    const int first = A.hub_first[h], count = A.hub_count[h];
    float m = kNegBig, s = 0.f;
    for (int c = lane; c < count; c += kWave) {
        const float2 r = A.rec[first + c];
        state_merge<MODE>(m, s, r.x, r.y);
    }
    for (int off = 1; off < kWave; off <<= 1) state_merge<MODE>(m, s, __shfl_xor(m, off), __shfl_xor(s, off));
    for (int c = lane; c < count; c += kWave) A.fin[first + c] = make_float2(m, s);
}

// hub chunks: the normalising writes (one wave per chunk)
template <int MODE>
__global__ __launch_bounds__(kBlock) void es_finish_kernel(const EsArgs A) {
    constexpr bool KG = MODE == ES_KGAT || MODE == ES_KGCN;
    const int item = (int)blockIdx.x * (kBlock / kWave) + (int)threadIdx.x / kWave;
    const int lane = (int)threadIdx.x % kWave;
    if (item >= A.n_long) return;
    const LongItem it = A.long_items[item];
    if (it.slot < 0) return;
    const float2 st = A.fin[it.slot];
    const float inv = MODE == ES_BWD ? 0.f : 1.0f / (st.y + 1e-16f);
    const float mm = MODE == ES_BWD ? st.y : st.x;
    for (int e = it.beg + lane; e < it.end; e += kWave) finish_edge<MODE>(A, e, KG ? A.scratch[e] : 0.f, mm, inv);
}

__global__ void kg_types_kernel(int64_t E, const int *__restrict__ eid, const int64_t *__restrict__ type, int64_t stride,
                                int num_types, int *__restrict__ out, int *err) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int64_t t = type[(int64_t)eid[e] * stride];
    const bool bad = t <= -(int64_t)num_types || t >= (int64_t)num_types;
    if (bad) *err = 1;
    out[e] = bad ? 0 : (int)t;
}

const char *es_name(int mode, int which) {
    static const char *names[4][3] = {{"es_rows_softmax", "es_merge_softmax", "es_finish_softmax"},
                                      {"es_rows_bwd", "es_merge_bwd", "es_finish_bwd"},
                                      {"es_rows_kgat", "es_merge_kgat", "es_finish_kgat"},
                                      {"es_rows_kgcn", "es_merge_kgcn", "es_finish_kgcn"}};
    return names[mode][which];
}

template <int MODE, int G>
int es_launch(EsArgs A, const Relation &R, double gathered, double table, hipStream_t stream) {
    A.rowptr = R.rowptr;
    A.col = R.col;
    A.eid = R.eid;
    A.short_rows = R.short_rows;
    A.long_items = R.long_items;
    A.hub_first = R.hub_first;
    A.hub_count = R.hub_count;
    A.n_short = R.n_short;
    A.n_long = R.n_long;
    A.n_hub = R.n_hub;
    A.n_long_blocks = (R.n_long + 3) / 4;
    const int blocks = A.n_long_blocks + (R.n_short + kBlock / G - 1) / (kBlock / G);
    if (blocks > 0) {
        ProfScope ps(es_name(MODE, 0), stream, gathered, gathered, table);
        PEA_LAUNCH((es_rows_kernel<MODE, G>), dim3(blocks), dim3(kBlock), 0, stream, A);
        PEA_HIP(hipGetLastError());
    }
    if (R.n_hub > 0) {
        {
            ProfScope ps(es_name(MODE, 1), stream, 0.0);
            PEA_LAUNCH((es_merge_kernel<MODE>), dim3((R.n_hub + 3) / 4), dim3(kBlock), 0, stream, A);
            PEA_HIP(hipGetLastError());
        }
        ProfScope ps(es_name(MODE, 2), stream, 0.0);
        PEA_LAUNCH((es_finish_kernel<MODE>), dim3((R.n_long + 3) / 4), dim3(kBlock), 0, stream, A);
        PEA_HIP(hipGetLastError());
    }
    return PEA_OK;
}

template <int MODE>
int es_launch_g(const EsArgs &A, const Relation &R, double gathered, double table, hipStream_t stream) {
    switch (lanes_for(A.emb)) {
        case 4: return es_launch<MODE, 4>(A, R, gathered, table, stream);
        case 8: return es_launch<MODE, 8>(A, R, gathered, table, stream);
        case 16: return es_launch<MODE, 16>(A, R, gathered, table, stream);
        case 32: return es_launch<MODE, 32>(A, R, gathered, table, stream);
        default: return es_launch<MODE, 64>(A, R, gathered, table, stream);
    }
}

// workspace: [rec | fin] (n_slots float2 each) then the KG extras: scratch [e_kept], xp [N, emb] (KGAT)
size_t ws_state_bytes(const Relation &R) { return align256((size_t)R.n_slots * 2 * sizeof(float2)); }
size_t ws_scratch_bytes(const Relation &R) { return align256((size_t)R.e_kept * sizeof(float)); }

int check_plan(const pea_plan *plan, int relation, const char *who) {
    PEA_REQUIRE(plan && relation >= 0 && relation < (int)plan->rels.size(), PEA_ERR_ARG, "%s: bad relation", who);
    const Relation &R = plan->rels[(size_t)relation];
    PEA_REQUIRE(R.eid != nullptr || R.e_kept == 0, PEA_ERR_ARG, "%s: the plan was created without PEA_PLAN_EDGE_IDS", who);
    PEA_REQUIRE(!(plan->flags & PEA_PLAN_SELF_LOOPS), PEA_ERR_ARG,
                "%s: the plan must not carry PEA_PLAN_SELF_LOOPS (every edge of the caller's COO takes part)", who);
    return PEA_OK;
}

}  // namespace
}  // namespace pea

using namespace pea;

extern "C" size_t pea_edge_softmax_workspace_bytes(const pea_plan *plan, int relation) {
    if (!plan || relation < 0 || relation >= (int)plan->rels.size()) return 0;
    return ws_state_bytes(plan->rels[(size_t)relation]) + 256;
}

extern "C" int pea_edge_softmax(const pea_plan *plan, int relation, const float *src, float *out, void *workspace,
                                size_t workspace_bytes, void *stream) {
    PEA_TRY(check_plan(plan, relation, "edge_softmax"));
    const Relation &R = plan->rels[(size_t)relation];
    if (R.e_kept == 0) return PEA_OK;
    PEA_REQUIRE(src && out && workspace, PEA_ERR_ARG, "edge_softmax: null argument");
    PEA_REQUIRE(workspace_bytes >= pea_edge_softmax_workspace_bytes(plan, relation), PEA_ERR_NOMEM,
                "edge_softmax: workspace too small");
    EsArgs A{};
    A.src = src;
    A.out = out;
    A.emb = 4;
    A.rec = reinterpret_cast<float2 *>(aligned_ws(workspace));
    A.fin = A.rec + R.n_slots;
    return es_launch<ES_SOFTMAX, 1>(A, R, 12.0 * (double)R.e_kept, 0.0, (hipStream_t)stream);
}

extern "C" int pea_edge_softmax_backward(const pea_plan *plan, int relation, const float *y, const float *grad,
                                         float *grad_src, void *workspace, size_t workspace_bytes, void *stream) {
    PEA_TRY(check_plan(plan, relation, "edge_softmax_backward"));
    const Relation &R = plan->rels[(size_t)relation];
    if (R.e_kept == 0) return PEA_OK;
    PEA_REQUIRE(y && grad && grad_src && workspace, PEA_ERR_ARG, "edge_softmax_backward: null argument");
    PEA_REQUIRE(workspace_bytes >= pea_edge_softmax_workspace_bytes(plan, relation), PEA_ERR_NOMEM,
                "edge_softmax_backward: workspace too small");
    EsArgs A{};
    A.src = y;
    A.grad = grad;
    A.out = grad_src;
    A.emb = 4;
    A.rec = reinterpret_cast<float2 *>(aligned_ws(workspace));
    A.fin = A.rec + R.n_slots;
    return es_launch<ES_BWD, 1>(A, R, 16.0 * (double)R.e_kept, 0.0, (hipStream_t)stream);
}

extern "C" int pea_kg_edge_types(const pea_plan *plan, int relation, const int64_t *edge_type, int64_t stride, int num_types,
                                 int32_t *types_slot, void *stream) {
    PEA_TRY(check_plan(plan, relation, "kg_edge_types"));
    const Relation &R = plan->rels[(size_t)relation];
    PEA_REQUIRE(num_types > 0 && stride >= 1, PEA_ERR_ARG, "kg_edge_types: num_types %d, stride %lld", num_types,
                (long long)stride);
    if (R.e_kept == 0) return PEA_OK;
    PEA_REQUIRE(edge_type && types_slot, PEA_ERR_ARG, "kg_edge_types: null argument");
    hipStream_t st = (hipStream_t)stream;
    int *err = nullptr, herr = 0;
    PEA_HIP(hipMalloc((void **)&err, sizeof(int)));
    hipError_t e0 = hipMemsetAsync(err, 0, sizeof(int), st);
    if (e0 == hipSuccess) {
        hipLaunchKernelGGL(kg_types_kernel, dim3((unsigned)((R.e_kept + 255) / 256)), dim3(256), 0, st, R.e_kept, R.eid,
                           edge_type, stride, num_types, types_slot, err);
        e0 = hipGetLastError();
    }
    if (e0 == hipSuccess) e0 = hipMemcpyAsync(&herr, err, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e0 == hipSuccess) e0 = hipStreamSynchronize(st);
    (void)hipFree(err);
    PEA_HIP(e0);
    PEA_REQUIRE(herr == 0, PEA_ERR_RANGE, "kg_edge_types: an edge type outside (-%d, %d)", num_types, num_types);
    return PEA_OK;
}

extern "C" size_t pea_kg_attention_workspace_bytes(const pea_plan *plan, int relation, int mode, int emb) {
    if (!plan || relation < 0 || relation >= (int)plan->rels.size() || emb <= 0) return 0;
    const Relation &R = plan->rels[(size_t)relation];
    size_t b = ws_state_bytes(R) + ws_scratch_bytes(R) + 256;
    if (mode == PEA_KG_KGAT) b += (size_t)plan->N * (size_t)emb * sizeof(float);
    return b;
}

extern "C" int pea_kg_attention(const pea_plan *plan, int relation, int mode, int emb, const float *x, int64_t ldx,
                                const float *proj, const float *r, const int32_t *types_slot, float *att_map,
                                void *workspace, size_t workspace_bytes, void *stream) {
    PEA_TRY(check_plan(plan, relation, "kg_attention"));
    PEA_REQUIRE(mode == PEA_KG_KGAT || mode == PEA_KG_KGCN, PEA_ERR_ARG, "kg_attention: mode %d", mode);
    PEA_REQUIRE(emb > 0 && emb % 4 == 0 && emb <= 256, PEA_ERR_ARG,
                "kg_attention: emb %d must be a multiple of 4 in (0, 256]", emb);
    PEA_REQUIRE(ldx >= emb && ldx % 4 == 0, PEA_ERR_ARG, "kg_attention: row stride %lld must be a multiple of 4 >= emb",
                (long long)ldx);
    const Relation &R = plan->rels[(size_t)relation];
    if (R.e_kept == 0) return PEA_OK;
    PEA_REQUIRE(x && r && types_slot && att_map && workspace && (mode == PEA_KG_KGCN || proj), PEA_ERR_ARG,
                "kg_attention: null argument");
    PEA_REQUIRE(workspace_bytes >= pea_kg_attention_workspace_bytes(plan, relation, mode, emb), PEA_ERR_NOMEM,
                "kg_attention: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    EsArgs A{};
    A.rec = reinterpret_cast<float2 *>(aligned_ws(workspace));
    A.fin = A.rec + R.n_slots;
    A.scratch = reinterpret_cast<float *>(reinterpret_cast<char *>(A.rec) + ws_state_bytes(R));
    A.rel = r;
    A.types = types_slot;
    A.emb = emb;
    A.out = att_map;
    // per edge: the source row (KGAT) + eid, col, type and the output value
    const double per_edge = (mode == PEA_KG_KGAT ? 4.0 * emb : 0.0) + 16.0;
    if (mode == PEA_KG_KGCN) {
        A.xd = x;
        A.ld = (int)ldx;
        return es_launch_g<ES_KGCN>(A, R, per_edge * (double)R.e_kept, 0.0, st);
    }
    float *xp = reinterpret_cast<float *>(reinterpret_cast<char *>(A.scratch) + ws_scratch_bytes(R));
    pea_dense_job J{};
    J.a = x;
    J.lda = ldx;
    J.k = emb;
    J.w = proj;
    J.ldw = emb;
    J.n_out = emb;
    J.out = xp;
    J.ldo = emb;
    PEA_TRY(pea_dense_batch(plan->N, 1, &J, stream));
    A.xd = A.xs = xp;
    A.ld = emb;
    return es_launch_g<ES_KGAT>(A, R, per_edge * (double)R.e_kept, 4.0 * (double)R.src_span * emb, st);
}
