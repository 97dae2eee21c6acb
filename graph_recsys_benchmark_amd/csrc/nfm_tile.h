// The NFM pair tile, defined ONCE: nfm_score_kernel (nfm.hip) and the catalogue scan and its threshold pass (nfm_scan.hip)
// call the same three functions, so a pair's logit has the same bits wherever it is computed.  One workgroup = kThreads
// threads = 4 waves scores kSP = 64 pairs, four MFMA row blocks:
//   x = e_u (.) e_i (nfm_x4) sits in LDS as Xt [64][LD];
//   nfm_tile_dots: z = x W'^T over the staged image of W' [HP][LD] as four chains that share each weight value
//     (rows_times_wt<1, 4>; wave w the output tiles w, w + 4, ..), relu(z + b') w2 added per lane over its tiles in tile
//     order, over the lane's four column groups by two xor shuffles, over the waves in wave order;
//   nfm_logit: ((lin[u] + lin[U + i]) + bias) + d, the linear terms first, as the training step adds them.
// Nothing here depends on where a pair sits in its tile.  The build has -ffp-contract=off.
#pragma once
#include "tile16.h"

namespace pea {
namespace {

constexpr int kSB = 4, kSP = kSB * kTR;       // row blocks and pairs of one tile

// four columns of x of one pair
__device__ __forceinline__ float4 nfm_x4(float4 u, float4 i) { return make_float4(u.x * i.x, u.y * i.y, u.z * i.z, u.w * i.w); }

// d of the tile's 64 pairs: thread k < kSP returns pair k's, the others 0.  Called by all kThreads threads once Xt is
// complete (a barrier lies behind the caller's writes); holds ONE barrier, between the waves' partials and their sum, and
// leaves `part` [kWaves][kSP] readable until the caller's next barrier.
__device__ __forceinline__ float nfm_tile_dots(const float *Ws, const float *Xt, float *part, const float *__restrict__ bf,
                                               const float *__restrict__ w2, int H, int HP, int LD, int e4) {
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, n = lane & 15, g = lane >> 4;
    const int HT = HP / 16;
    float s[kSB] = {0.f, 0.f, 0.f, 0.f};
    for (int v = wave; v < HT; v += kWaves) {
        f32x4 z[kSB] = {};
        rows_times_wt<1, kSB>(Ws, HP, LD, Xt, LD, e4, v, n, g, z);
        const int col = 16 * v + 4 * g;
        if (col >= H) continue;
        const float4 b = ld4(bf + col), w = ld4(w2 + col);
#pragma unroll
        for (int c = 0; c < kSB; ++c)
            s[c] += ((fmaxf(z[c][0] + b.x, 0.f) * w.x + fmaxf(z[c][1] + b.y, 0.f) * w.y) +
                     (fmaxf(z[c][2] + b.z, 0.f) * w.z + fmaxf(z[c][3] + b.w, 0.f) * w.w));
    }
#pragma unroll
    for (int c = 0; c < kSB; ++c) {
        s[c] += __shfl_xor(s[c], 16);
        s[c] += __shfl_xor(s[c], 32);
        if (g == 0) part[wave * kSP + c * kTR + n] = s[c];
    }
    __syncthreads();
    const int k = threadIdx.x;
    return k < kSP ? (part[k] + part[kSP + k]) + (part[2 * kSP + k] + part[3 * kSP + k]) : 0.f;
}

__device__ __forceinline__ float nfm_logit(float lin_u, float lin_i, float bias, float d) { return ((lin_u + lin_i) + bias) + d; }

}  // namespace
}  // namespace pea
