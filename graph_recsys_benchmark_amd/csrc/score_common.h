// Device helpers shared by the scoring kernels of fuse_score.hip and ablate.hip: the fc2(relu(fc1([u || i]))) scorer of
// graph_recsys_benchmark/models/base.py:208-214 in ONE order of operations, so that every kernel that scores a pair gives
// the same bits for it, and the per-device error flag the id-range checks report through.
#ifndef PEA_SCORE_COMMON_H_
#define PEA_SCORE_COMMON_H_

#include "common.h"

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

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }

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

__device__ __forceinline__ float log_sigmoid_ref(float d) {
    // the reference takes sigmoid then log in fp32 with no clamp (may give -inf); keep that
    return logf(1.0f / (1.0f + expf(-d)));
}

}  // namespace
}  // namespace pea
#endif  // PEA_SCORE_COMMON_H_
