// The 16-row MFMA tile toolkit of the training kernels kg_update.hip and transr_train.hip, each piece defined ONCE so that
// both kernels cut, multiply and reduce their tiles alike.  One workgroup = kThreads threads = 4 waves walks tiles of kTR
// rows; every product runs on v_mfma_f32_16x16x4_f32 from a zero accumulator with k ascending, lane (n, g) =
// (lane & 15, lane >> 4) holding k = 4 t + g in step t.  A weight [in, out] sits in LDS as a zero-padded image [ceil16(in)][width + 4]; the operands of a
// tile are blocks of kTR rows, one behind the other (block c at base + c * kTR * ld), so a product over several operands
// runs its chains interleaved inside one k-loop: independent accumulators, each weight value loaded once per step.
// dW-style gradients (rows as k) are dealt out to the waves as 16x16 tiles (tile id = wave + kWaves q -> input tile
// id / n_ut, output tile id % n_ut), stay in the accumulators over all row tiles of the workgroup and leave as one
// partial per workgroup (dw_store; train_common.h: ordered_sum adds them in workgroup order).  The accumulate step itself
// is NOT here: each kernel writes its q / k-step loop out.  With the loop in a function the compiler allocates the kernels
// differently: 256 VGPRs + 256 AGPRs + scratch for transr_train_kernel<16, true> and one to two waves of occupancy less for
// kg_update_bwd_kernel<.., false>; with one tile per call it moves as far the other way.  Neither is the measured code
// (profiles/r09/train_refactor.md).
#pragma once
#include "common.h"

namespace pea {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kTR = 16;                       // rows of one tile: one MFMA operand
constexpr size_t kLdsBudget = 156 * 1024;     // of the CU's 160 KB

inline int ceil16(int v) { return (v + 15) / 16 * 16; }

// `tiles` accumulator tiles dealt to the waves: tiles per wave, rounded up to a power of two (the kernels' NT)
inline int tiles_per_wave(int tiles) {
    const int per_wave = (tiles + kWaves - 1) / kWaves;
    int nt = 1;
    while (nt < per_wave) nt <<= 1;
    return nt;
}

// what a kernel's dynamic-LDS limit is raised to: once, to the most any configuration asks for
inline size_t lds_limit(size_t lds) { return lds > 64 * 1024 ? kLdsBudget : 0; }

// columns [c0, c0 + OC) of a [in, out] weight into its LDS image [IP][LDW]; rows >= in and columns >= out are zero.
// V floats per access: 4 = 16-byte loads (c0 and out multiples of 4, w 16-byte aligned), 1 = a weight of any alignment
template <int V>
__device__ __forceinline__ void stage_weight(const float *w, int in, int out, int c0, float *img, int IP, int OC, int LDW) {
    for (int i = threadIdx.x; i < IP * (OC / V); i += kThreads) {
        const int k = i / (OC / V), c = V * (i - k * (OC / V));
        const bool inside = k < in && c0 + c < out;
        if (V == 4) st4(img + k * LDW + c, inside ? ld4(w + (size_t)k * out + c0 + c) : make_float4(0.f, 0.f, 0.f, 0.f));
        else img[k * LDW + c] = inside ? w[(size_t)k * out + c0 + c] : 0.f;
    }
}

// NC chains over `steps` k-steps, added to acc (the caller's zeros): chain c multiplies weight image c (one image for all chains when
// NW == 1) at W[wo + t * wstep] by operand block c at B[bo + 4 t].  All chains share ONE k-loop.
template <int NW, int NC>
__device__ __forceinline__ void mfma_chains(const float *W, int wimg, int wo, int wstep, const float *B, int bblk, int bo, int steps,
                                            f32x4 (&acc)[NC]) {
    static_assert(NW == 1 || NW == NC, "one weight for all chains or one per chain");
    for (int t = 0; t < steps; ++t) {
        float w[NW];
#pragma unroll
        for (int c = 0; c < NW; ++c) w[c] = W[c * wimg + wo + t * wstep];
#pragma unroll
        for (int c = 0; c < NC; ++c)
            acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[NW == 1 ? 0 : c], B[c * bblk + bo + 4 * t], acc[c], 0, 0, 0);
    }
}

// the product with the row on the lane, Z = A W for output tile u (k = the weight's rows, k4 steps): register r of lane
// (n, g) = Z[row n][column 16 u + 4 g + r].  The image is the A operand, the staged rows [kTR][LDA] the B operand
template <int NW, int NC>
__device__ __forceinline__ void rows_times_w(const float *W, int IP, int LDW, const float *A, int LDA, int k4, int u, int n, int g,
                                             f32x4 (&acc)[NC]) {
    mfma_chains<NW, NC>(W, IP * LDW, g * LDW + 16 * u + n, 4 * LDW, A, kTR * LDA, n * LDA + g, k4, acc);
}

// the transposed product dA = dZ W^T for input tile v (k = the weight's columns, k4 steps): register r of lane (n, g) =
// dA[row n][input 16 v + 4 g + r]
template <int NW, int NC>
__device__ __forceinline__ void rows_times_wt(const float *W, int IP, int LDW, const float *Z, int LDZ, int k4, int v, int n, int g,
                                              f32x4 (&acc)[NC]) {
    mfma_chains<NW, NC>(W, IP * LDW, (16 * v + n) * LDW + g, 4, Z, kTR * LDZ, n * LDZ + g, k4, acc);
}

// this workgroup's partial: the wave's tiles into columns c0 + .. of part [NC][in, out] (matrix c at part + c * wsz)
template <int NT, int NC>
__device__ __forceinline__ void dw_store(const f32x4 (&dw)[NC][NT], float *part, size_t wsz, int in, int out, int c0, int IT, int n_ut,
                                         int wave, int n, int g) {
#pragma unroll
    for (int q = 0; q < NT; ++q) {
        const int id = wave + kWaves * q;
        if (id >= IT * n_ut) continue;
        const int v = id / n_ut, u = id - v * n_ut;
        const int col = c0 + 16 * u + n;
        if (col >= out) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 16 * v + 4 * g + r;
            if (i >= in) continue;
#pragma unroll
            for (int c = 0; c < NC; ++c) part[c * wsz + (size_t)i * out + col] = dw[c][q][r];
        }
    }
}

}  // namespace
}  // namespace pea
