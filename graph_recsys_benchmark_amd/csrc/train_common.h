// What the training kernels (bpr_train.hip, dot_train.hip, transr_train.hip, kg_update.hip) share besides their tiles,
// each piece defined ONCE: the BPR loss term with its derivative, the thread-order block sum, the fixed-order reduction of
// per-workgroup partials, and where the error flag and the partial sums sit in a loss kernel's workspace.  No float
// atomics anywhere: the same additions in the same order on every run.
#pragma once
#include "score_common.h"

namespace pea {

// workspace of a loss entry point that checks ids: the int32 error flag at byte 0, the workgroups' float sums at byte 256
constexpr size_t kWsSumsOffset = 256;
inline int *ws_err_flag(void *workspace) { return (int *)workspace; }
inline float *ws_sums(void *workspace) { return (float *)((char *)workspace + kWsSumsOffset); }

namespace {

// d = pos - neg  ->  the loss term log sigmoid(d) (the reference's formula, log_sigmoid_ref) and g = d loss / d pos =
// -(1 - sigmoid(d));  d loss / d neg = -g
__device__ __forceinline__ void bpr_term(float d, float &term, float &g) {
    term = log_sigmoid_ref(d);
    g = -(1.0f - 1.0f / (1.0f + expf(-d)));
}

// the workgroup's TB terms added by thread 0 in thread order
template <int TB>
__device__ __forceinline__ void block_sum_in_order(float term, float *out) {
    __shared__ float red[TB];
    red[threadIdx.x] = term;
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.f;
        for (int k = 0; k < TB; ++k) a += red[k];
        *out = a;
    }
}

// p[0] + p[stride] + ... (n terms) added in index order; the loads go out eight at a time, the order of the additions stays
__device__ __forceinline__ float ordered_sum(const float *__restrict__ p, size_t stride, int n) {
    float acc = 0.f;
    int w = 0;
    for (; w + 8 <= n; w += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = p[(size_t)(w + j) * stride];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += v[j];
    }
    for (; w < n; ++w) acc += p[(size_t)w * stride];
    return acc;
}

// the ordered final of a loss: minus the workgroups' sums in index order (one thread calls this)
__device__ __forceinline__ void store_loss(const float *__restrict__ sums, int n, float *loss) { loss[0] = -ordered_sum(sums, 1, n); }

}  // namespace
}  // namespace pea
