// Device helpers shared by the forward (agg.hip) and backward (agg_bwd.hip) aggregation kernels.
#pragma once
#include <type_traits>

#include "common.h"

namespace pea {
namespace {

constexpr int kBlock = 256;
constexpr float kNegBig = -3.0e38f;  // finite "minus infinity" for the running max (no inf-inf NaNs)
constexpr float kLog2e = 1.44269504088896340736f;

struct AggLaunch {
    int n_groups;
    int blk_start[kMaxAggGroups + 1];
    // agg_rows_kernel: workgroups [0, n_long_blocks) walk blk_start (long items), the rest blk_short (short rows)
    int n_long_blocks;
    int blk_short[kMaxAggGroups + 1];
    AggGroup g[kMaxAggGroups];
};

__device__ __forceinline__ float4 fma4(float w, float4 h, float4 a) {
    return make_float4(fmaf(w, h.x, a.x), fmaf(w, h.y, a.y), fmaf(w, h.z, a.z), fmaf(w, h.w, a.w));
}
__device__ __forceinline__ float4 scale4(float4 a, float f) { return make_float4(a.x * f, a.y * f, a.z * f, a.w * f); }
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 shfl_xor4(float4 v, int m) {
    return make_float4(__shfl_xor(v.x, m), __shfl_xor(v.y, m), __shfl_xor(v.z, m), __shfl_xor(v.w, m));
}

// Running softmax-weighted sum for one attention group over V4 float4 chunks per lane: value = acc / s with weights
// exp(e - m).  One chunk (Soft) keeps `acc` a plain float4; chunk(v) reads either form.
template <int V4>
struct SoftV {
    float m, s;
    typename std::conditional<V4 == 1, float4, float4[V4]>::type acc;
    __device__ __forceinline__ float4 &chunk(int v) {
        if constexpr (V4 == 1) return acc; else return acc[v];
    }
    __device__ __forceinline__ void init() {
        m = kNegBig;
        s = 0.f;
#pragma unroll
        for (int v = 0; v < V4; ++v) chunk(v) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // The running max m lives in the log2 domain, the logits e in NATURAL units exactly as the reference forms them
    // (leaky_relu(x_i . att_i + x_j . att_j), reference GATConv.message): a weight is 2^(e * log2(e) - m), one v_fma_f32 (the
    // product exact inside it) + one v_exp_f32.  Every weight of a state is relative to the same m, whatever m is, so the
    // rounding of m itself cancels in acc / s; only the small difference e * log2(e) - m is rounded.  (Round 2 folded
    // log2(e) into the packed attention vectors instead: one more rounding per vector component, and the exponent inherited
    // the rounding of the scaled logit -- up to 4x the sequential oracle's error on deep multi-head stacks.)
    __device__ __forceinline__ void push(float e, const float4 (&h)[V4]) {
        const float mn = fmaxf(m, e * kLog2e);
        const float fs = __builtin_amdgcn_exp2f(m - mn);                    // factor on the old state (1 when the max stays)
        const float p = __builtin_amdgcn_exp2f(fmaf(e, kLog2e, -mn));       // weight of the new edge
        m = mn;
        s = fmaf(s, fs, p);
#pragma unroll
        for (int v = 0; v < V4; ++v) {
            float4 &a = chunk(v);
            a.x = fmaf(a.x, fs, p * h[v].x);
            a.y = fmaf(a.y, fs, p * h[v].y);
            a.z = fmaf(a.z, fs, p * h[v].z);
            a.w = fmaf(a.w, fs, p * h[v].w);
        }
    }
    __device__ __forceinline__ void push(float e, float4 h) {  // one chunk, handed over as the float4 it is
        const float4 one[1] = {h};
        push(e, one);
    }
    __device__ __forceinline__ void merge(float m2, float s2, const float4 (&a2)[V4]) {
        const float mn = fmaxf(m, m2);
        const float f1 = __builtin_amdgcn_exp2f(m - mn), f2 = __builtin_amdgcn_exp2f(m2 - mn);
        s = s * f1 + s2 * f2;
#pragma unroll
        for (int v = 0; v < V4; ++v) chunk(v) = add4(scale4(chunk(v), f1), scale4(a2[v], f2));
        m = mn;
    }
    // One update for 4 edges with already-masked logits e (natural units; -inf = no edge, weight 2^(-inf) = 0): shared new
    // max, one rescale, four weights in slot order.  The batch size is part of the arithmetic: it stays 4 whatever the
    // caller keeps in flight, so every variant of the gather produces the same bits.
    __device__ __forceinline__ void batch4(const float (&e)[4], const float4 (&h)[4][V4]) {
        float mx = -INFINITY;                                                // largest logit of the batch, natural units
#pragma unroll
        for (int u = 0; u < 4; ++u) mx = fmaxf(mx, e[u]);
        const float mn = fmaxf(m, mx * kLog2e);                              // running max, log2 domain (finite)
        const float fs = __builtin_amdgcn_exp2f(m - mn);
        m = mn;
        s *= fs;
#pragma unroll
        for (int v = 0; v < V4; ++v) chunk(v) = scale4(chunk(v), fs);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float p = __builtin_amdgcn_exp2f(fmaf(e[u], kLog2e, -mn));  // 0 for the masked slots
            s += p;
#pragma unroll
            for (int v = 0; v < V4; ++v) chunk(v) = fma4(p, h[u][v], chunk(v));
        }
    }
    // fold the kWave / G subgroup states of a wave (xor butterfly: every lane ends with the same value)
    template <int G>
    __device__ __forceinline__ void fold() {
#pragma unroll
        for (int off = G; off < kWave; off <<= 1) {
            const float m2 = __shfl_xor(m, off), s2 = __shfl_xor(s, off);
            float4 a2[V4];
#pragma unroll
            for (int v = 0; v < V4; ++v) a2[v] = shfl_xor4(chunk(v), off);
            merge(m2, s2, a2);
        }
    }
};
using Soft = SoftV<1>;

// slope in [0, 1] (checked on the host): leaky_relu(a) = max(a, slope * a)
__device__ __forceinline__ float leaky(float a, float slope) { return fmaxf(a, a * slope); }

// row j of a [rows, ld] fp32 matrix: one 32x32->64 multiply-add, no sign extension
__device__ __forceinline__ const float *row_at(const float *base, int j, int ld) {
    return base + (unsigned long long)(unsigned)j * (unsigned)ld;
}

__device__ __forceinline__ float dot4(float4 a, float4 b) { return fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, a.w * b.w))); }

// Sum of v over the F4 = F/4 consecutive lanes that hold one attention head's columns (every lane of the
// head gets the total).  The logit (x_i.att_i).sum(-1) + (x_j.att_j).sum(-1) of GATConv.message is thus
// computed from the gathered row itself: no per-node attention scalars are stored or gathered.
// F4T > 0: head width known at compile time (a power of two): constant-offset xor shuffles (DPP / swizzle).
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {  // v from the lane the DPP control selects (all rows, all banks)
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}

template <int F4T>
__device__ __forceinline__ float head_sum(float v, int lane, int pos, int F4, bool pow2) {
    if (F4T > 0) {  // all-reduce inside aligned power-of-two lane groups with data-parallel primitives (no LDS crossbar)
        if (F4T >= 2) v += dpp_f<0xB1>(v);    // quad_perm [1,0,3,2]
        if (F4T >= 4) v += dpp_f<0x4E>(v);    // quad_perm [2,3,0,1]
        if (F4T >= 8) v += dpp_f<0x141>(v);   // row_half_mirror: the other quad of the 8-lane half
        if (F4T >= 16) v += dpp_f<0x140>(v);  // row_mirror: the other half of the 16-lane row
        if (F4T >= 32) v += __shfl_xor(v, 16);
        if (F4T >= 64) v += __shfl_xor(v, 32);
        return v;
    }
    if (pow2) {
        for (int off = 1; off < F4; off <<= 1) v += __shfl_xor(v, off);
        return v;
    }
    for (int off = 1; off < F4; off <<= 1) {
        const float o = __shfl_down(v, off);
        if (pos + off < F4) v += o;
    }
    return __shfl(v, lane - pos);
}

__device__ __forceinline__ int find_group(const AggLaunch &L) {
    int g = 0;
    while (g + 1 < L.n_groups && (int)blockIdx.x >= L.blk_start[g + 1]) ++g;
    return g;
}

// Long item `item` of a group.  slot == -2 means no work: the padding of the XCD-affine item layout (plan.hip), and here
// also an index past the group's items.  Wave-uniform.  By value: the four fields arrive in one 16-byte load.
__device__ __forceinline__ LongItem item_at(const AggGroup &P, int item) {
    if (item >= P.n_long) return LongItem{0, 0, 0, -2};
    return P.long_items[item];
}

// ------------------------------------------------------------------------------------------------ host: launch planning
inline int lanes_for(int W) {
    int g = 4;
    while (g * 4 < W) g <<= 1;
    return g;
}

// the gather footprint of a group (a launch reports the largest among its groups)
inline double table_bytes(const AggGroup &g) { return g.table_rows * 4.0 * g.W; }

// Appends g to L with n_long of its long items (4 per workgroup): a group starts on a multiple of 8 workgroups, so that
// item -> workgroup -> XCD (round-robin) is the plan's placement in the thin and in the fat kernel alike, forward and backward.
inline AggGroup &add_group(AggLaunch &L, const AggGroup &g, int n_long, int &blocks) {
    L.blk_start[L.n_groups] = blocks;
    AggGroup &c = L.g[L.n_groups++];
    c = g;
    c.n_long = n_long;
    blocks += ((n_long + 3) / 4 + 7) / 8 * 8;
    return c;
}

}  // namespace
}  // namespace pea
