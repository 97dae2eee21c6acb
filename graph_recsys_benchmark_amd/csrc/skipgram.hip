// pea_skipgram_train: the skip-gram loss of metapath2vec over whole walks and its whole backward (reference
// models/metapath2vec.py:117-121 cuts every walk of T ids into T - C + 1 windows, :147-172 gathers [windows, C - 1, D] rows of
// the table per side and leaves the backward to torch's index backward over every duplicated id).  Here a walk's table rows
// are read ONCE, by the workgroup that owns the walk:
//   1 sg_keys    one thread per walk position: the (id, position) sort key, the valid pairs counted per side (integers only)
//   2 sg_walk    one workgroup per walk: its T rows staged in LDS, the (T - C + 1)(C - 1) pair dots -> loss terms and pair
//                coefficients d loss / d out (already scaled by 1 / n_valid of the side), then every position's gradient row
//                formed from its <= 2 (C - 1) window partners and written once: posgrad [rows * T, D]
//   3 sg_sort    rocprim::radix_sort_keys over the bits in use: the positions of a node become one run, in position order
//   4 sg_runs    the run-summing idea of rows_scatter.hip for runs of any length: a run is cut at every kPiece-th sorted slot;
//                a lane group per piece adds its rows in slot order; a piece that is a whole run writes the node's row,
//                the others a partial record of their slot chunk (first piece of a chunk: "head", a run's first piece that
//                leaves its chunk: "tail")
//   5 sg_merge   a lane group per run that left its chunk: tail + the heads of the following chunks, in chunk order
//   6 sg_touched rocprim::select of the run starts: the ascending unique ids;   7 sg_final: the loss sums in index order
// No float atomics; every sum has a fixed order: identical calls give identical bytes.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "common.h"

namespace pea {
namespace {

typedef unsigned long long u64;

constexpr int kPiece = 256;          // sorted slots per chunk: no lane group adds more than this many rows
constexpr int kRunBatch = 8;         // rows a lane group keeps in flight
constexpr int kWalkThreads = 256;
constexpr int kPad = 4;              // LDS row stride D + 4 floats: consecutive rows start 4 banks apart (D = 64 alone: all on bank 0)
constexpr float kEps = 1e-15f;

extern __shared__ float sg_lds[] __attribute__((aligned(16)));

struct SgWalks {
    const long long *pos, *neg;
    long long n_pos, n_neg, pos_stride, neg_stride, num_nodes;
    int T, C, D;
};

__device__ __forceinline__ const long long *walk_row(const SgWalks &a, long long row) {
    return row < a.n_pos ? a.pos + row * a.pos_stride : a.neg + (row - a.n_pos) * a.neg_stride;
}

constexpr int kKeysPerThread = 4;    // sg_keys: 1024 positions per workgroup, so the two counters take one add per workgroup

__global__ __launch_bounds__(256) void sg_keys_kernel(const SgWalks a, long long n, int pos_bits, u64 *__restrict__ keys,
                                                      u64 *__restrict__ n_valid, int *__restrict__ flag) {
    __shared__ unsigned wave_cnt[2][4];
    unsigned cnt_pos = 0, cnt_neg = 0;
    for (int u = 0; u < kKeysPerThread; ++u) {
        const long long i = ((long long)blockIdx.x * kKeysPerThread + u) * 256 + threadIdx.x;
        if (i >= n) break;
        const long long row = i / a.T;
        const int t = (int)(i - row * a.T);
        const long long *ids = walk_row(a, row);
        const long long id = ids[t];
        const bool valid = id >= 0 && id < a.num_nodes;
        if (id >= a.num_nodes) atomicOr(flag, 1);
        keys[i] = ((u64)(valid ? id : a.num_nodes) << pos_bits) | (u64)i;
        if (valid && t <= a.T - a.C) {
            unsigned c = 0;
            for (int k = 1; k < a.C; ++k) {
                const long long v = ids[t + k];
                c += (v >= 0 && v < a.num_nodes) ? 1u : 0u;
            }
            if (row < a.n_pos) cnt_pos += c;
            else cnt_neg += c;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        cnt_pos += __shfl_xor(cnt_pos, off);
        cnt_neg += __shfl_xor(cnt_neg, off);
    }
    if ((threadIdx.x & 63) == 0) {
        wave_cnt[0][threadIdx.x >> 6] = cnt_pos;
        wave_cnt[1][threadIdx.x >> 6] = cnt_neg;
    }
    __syncthreads();
    if (threadIdx.x < 2) {       // integer atomics: the counts do not depend on the order
        const unsigned c = wave_cnt[threadIdx.x][0] + wave_cnt[threadIdx.x][1] + wave_cnt[threadIdx.x][2] + wave_cnt[threadIdx.x][3];
        if (c) atomicAdd(n_valid + threadIdx.x, (u64)c);
    }
}

// LDS: e [T][D + kPad] the walk's rows (zeros for a skipped id) | coef [(T - C + 1)(C - 1)] | sid [T] (id, or -1)
__global__ __launch_bounds__(kWalkThreads) void sg_walk_kernel(const SgWalks a, int g_shift, const float *__restrict__ table,
                                                               long long ld, const u64 *__restrict__ n_valid,
                                                               float *__restrict__ posgrad, float *__restrict__ walk_loss) {
    const int T = a.T, C = a.C, D = a.D, S = D + kPad, W = T - C + 1, npairs = W * (C - 1);
    float *e = sg_lds;
    float *coef = e + T * S;
    int *sid = reinterpret_cast<int *>(coef + npairs);
    __shared__ float wave_sum[kWalkThreads / 64];
    const long long row = blockIdx.x;
    const bool positive = row < a.n_pos;
    const long long *ids = walk_row(a, row);
    const int G = 1 << g_shift, grp = (int)threadIdx.x >> g_shift, n_grp = kWalkThreads >> g_shift;
    const int c4 = 4 * ((int)threadIdx.x & (G - 1));
    for (int t = grp; t < T; t += n_grp) {
        const long long id = ids[t];
        const bool valid = id >= 0 && id < a.num_nodes;
        if (c4 < D) st4(e + t * S + c4, valid ? ld4(table + id * ld + c4) : make_float4(0.f, 0.f, 0.f, 0.f));
        if (c4 == 0) sid[t] = valid ? (int)id : -1;
    }
    __syncthreads();
    const u64 nv = n_valid[positive ? 0 : 1];
    const float inv = nv > 0 ? 1.f / (float)nv : 0.f;
    float lsum = 0.f;
    for (int q = threadIdx.x; q < npairs; q += kWalkThreads) {
        const int j = q / (C - 1), k = q - j * (C - 1) + 1;
        float c = 0.f;
        if (sid[j] >= 0 && sid[j + k] >= 0) {
            const float *x = e + j * S, *y = e + (j + k) * S;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int d = 0; d < D; d += 4) {
                const float4 u = ld4(x + d), v = ld4(y + d);
                acc = make_float4(fmaf(u.x, v.x, acc.x), fmaf(u.y, v.y, acc.y), fmaf(u.z, v.z, acc.z), fmaf(u.w, v.w, acc.w));
            }
            const float out = (acc.x + acc.y) + (acc.z + acc.w);
            const float s = 1.f / (1.f + expf(-out)), oms = 1.f / (1.f + expf(out));     // sigmoid(out), 1 - sigmoid(out)
            if (positive) {
                lsum -= logf(s + kEps);
                c = -(s * oms) / (s + kEps) * inv;
            } else {
                lsum -= logf(oms + kEps);
                c = (s * oms) / (oms + kEps) * inv;
            }
        }
        coef[q] = c;
    }
    for (int off = 32; off > 0; off >>= 1) lsum += __shfl_xor(lsum, off);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = lsum;
    __syncthreads();
    if (threadIdx.x == 0) walk_loss[row] = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
    if (c4 >= D) return;
    for (int p = grp; p < T; p += n_grp) {
        if (sid[p] < 0) continue;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p < W) {                                   // p starts a window: its C - 1 partners to the right
            for (int k = 1; k < C; ++k) {
                const float c = coef[p * (C - 1) + k - 1];
                const float4 v = ld4(e + (p + k) * S + c4);
                acc = make_float4(fmaf(c, v.x, acc.x), fmaf(c, v.y, acc.y), fmaf(c, v.z, acc.z), fmaf(c, v.w, acc.w));
            }
        }
        for (int k = 1; k < C; ++k) {                  // p is partner k of the window that starts at p - k
            const int j = p - k;
            if (j < 0 || j >= W) continue;
            const float c = coef[j * (C - 1) + k - 1];
            const float4 v = ld4(e + j * S + c4);
            acc = make_float4(fmaf(c, v.x, acc.x), fmaf(c, v.y, acc.y), fmaf(c, v.z, acc.z), fmaf(c, v.w, acc.w));
        }
        st4(posgrad + ((size_t)row * T + p) * D + c4, acc);
    }
}

__device__ __forceinline__ float4 add4(float4 x, float4 y) { return make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w); }

__global__ __launch_bounds__(256) void sg_runs_kernel(long long n, const u64 *__restrict__ sorted, int pos_bits, u64 num_nodes,
                                                      const float *__restrict__ posgrad, int D, int g_shift,
                                                      float *__restrict__ grad, float *__restrict__ partial,
                                                      unsigned char *__restrict__ flags) {
    const long long slot = ((long long)blockIdx.x * 256 + threadIdx.x) >> g_shift;
    const int c4 = 4 * ((int)threadIdx.x & ((1 << g_shift) - 1));
    if (slot >= n) return;
    const u64 id = sorted[slot] >> pos_bits;
    const bool run_start = slot == 0 || (sorted[slot - 1] >> pos_bits) != id;
    const bool valid = id < num_nodes;
    if (c4 == 0) flags[slot] = (run_start && valid) ? 1 : 0;
    if (!valid || c4 >= D || !(run_start || slot % kPiece == 0)) return;
    const long long chunk = slot / kPiece;
    const long long lim = (chunk + 1) * kPiece < n ? (chunk + 1) * kPiece : n;
    const u64 pos_mask = ((u64)1 << pos_bits) - 1;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    long long i = slot;
    while (i < lim) {
        float4 t[kRunBatch];
        int cnt = 0;
#pragma unroll
        for (int u = 0; u < kRunBatch; ++u) {
            const u64 key = i + u < lim ? sorted[i + u] : ~(u64)0;
            const bool same = cnt == u && (key >> pos_bits) == id;
            cnt += same ? 1 : 0;
            t[u] = same ? ld4(posgrad + (size_t)(key & pos_mask) * D + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < kRunBatch; ++u)
            if (u < cnt) acc = add4(acc, t[u]);
        i += cnt;
        if (cnt < kRunBatch) break;
    }
    const bool run_end = i == n || (sorted[i] >> pos_bits) != id;
    float *dst = (run_start && run_end) ? grad + (size_t)id * D : partial + (size_t)(2 * chunk + (run_start ? 1 : 0)) * D;
    st4(dst + c4, acc);
}

__global__ __launch_bounds__(256) void sg_merge_kernel(long long n, long long n_chunks, const u64 *__restrict__ sorted, int pos_bits,
                                                       u64 num_nodes, int D, int g_shift, const float *__restrict__ partial,
                                                       float *__restrict__ grad) {
    const long long c = ((long long)blockIdx.x * 256 + threadIdx.x) >> g_shift;
    const int c4 = 4 * ((int)threadIdx.x & ((1 << g_shift) - 1));
    if (c >= n_chunks - 1 || c4 >= D) return;                   // the last chunk's runs end inside it
    const long long last = (c + 1) * kPiece - 1;                // < n: chunk c + 1 exists
    const u64 id = sorted[last] >> pos_bits;
    if (id >= num_nodes || (sorted[last + 1] >> pos_bits) != id) return;
    if (c > 0 && (sorted[c * kPiece - 1] >> pos_bits) == id) return;   // the run began before this chunk: its piece here is a head
    float4 acc = ld4(partial + (size_t)(2 * c + 1) * D + c4);
    for (long long k = c + 1; k < n_chunks && (sorted[k * kPiece] >> pos_bits) == id; ++k)
        acc = add4(acc, ld4(partial + (size_t)(2 * k) * D + c4));
    st4(grad + (size_t)id * D + c4, acc);
}

__global__ __launch_bounds__(1024) void sg_final_kernel(long long n_pos, long long n_neg, const float *__restrict__ walk_loss,
                                                        const u64 *__restrict__ n_valid, float *__restrict__ loss) {
    __shared__ float part[2][1024];
    for (int side = 0; side < 2; ++side) {
        const float *src = walk_loss + (side ? n_pos : 0);
        const long long m = side ? n_neg : n_pos;
        float s = 0.f;
        for (long long i = threadIdx.x; i < m; i += 1024) s += src[i];
        part[side][threadIdx.x] = s;
    }
    __syncthreads();
    for (int half = 512; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) {
            part[0][threadIdx.x] += part[0][threadIdx.x + half];
            part[1][threadIdx.x] += part[1][threadIdx.x + half];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float p = n_valid[0] > 0 ? part[0][0] / (float)n_valid[0] : 0.f;
        const float q = n_valid[1] > 0 ? part[1][0] / (float)n_valid[1] : 0.f;
        loss[0] = p + q;
        loss[1] = p;
        loss[2] = q;
    }
}

struct KeyToId {
    int pos_bits;
    __host__ __device__ int operator()(const u64 &key) const { return (int)(key >> pos_bits); }
};

int bits_for(u64 v) {      // bits needed to hold the value v
    int b = 1;
    while (b < 64 && (v >> b) != 0) ++b;
    return b;
}

int group_shift(int D) {   // lanes per row: the power of two >= D / 4
    int s = 0;
    while ((4 << s) < D) ++s;
    return s;
}

struct SgLayout {
    size_t keys, sorted, flags, walk_loss, partial, posgrad, temp, temp_bytes, total;
};

bool sg_layout(long long n_pos, long long n_neg, int T, int C, int D, SgLayout *L) {
    const long long rows = n_pos + n_neg, n = rows * T;
    const long long chunks = (n + kPiece - 1) / kPiece;
    size_t sort_bytes = 0, sel_bytes = 0;
    if (n > 0) {
        if (rocprim::radix_sort_keys(nullptr, sort_bytes, (const u64 *)nullptr, (u64 *)nullptr, (size_t)n, 0u, 64u, (hipStream_t)0) != hipSuccess) return false;
        if (rocprim::select(nullptr, sel_bytes, rocprim::make_transform_iterator((const u64 *)nullptr, KeyToId{0}),
                            (const unsigned char *)nullptr, (int *)nullptr, (int *)nullptr, (size_t)n, (hipStream_t)0) != hipSuccess)
            return false;
    }
    size_t at = 0;
    L->keys = at;        at += align256((size_t)n * 8);
    L->sorted = at;      at += align256((size_t)n * 8);
    L->flags = at;       at += align256((size_t)n);
    L->walk_loss = at;   at += align256((size_t)rows * 4);
    L->partial = at;     at += align256((size_t)chunks * 2 * D * 4);
    L->posgrad = at;     at += align256((size_t)n * D * 4);
    L->temp = at;
    L->temp_bytes = sort_bytes > sel_bytes ? sort_bytes : sel_bytes;
    at += align256(L->temp_bytes);
    L->total = at + 256;                                      // aligned_ws may move the start by up to 255 bytes
    return true;
}

}  // namespace
}  // namespace pea

using namespace pea;

extern "C" int pea_skipgram_supported(int D, int T, int C) {
    return (D >= 4 && D <= 128 && D % 4 == 0 && C >= 2 && C <= 16 && T >= C && T <= 128) ? 1 : 0;
}

extern "C" size_t pea_skipgram_workspace_bytes(int64_t n_pos, int64_t n_neg, int T, int C, int D) {
    if (!pea_skipgram_supported(D, T, C) || n_pos < 0 || n_neg < 0 || (n_pos + n_neg) * (int64_t)T >= ((int64_t)1 << 31)) return 0;
    SgLayout L;
    return sg_layout(n_pos, n_neg, T, C, D, &L) ? L.total : 0;
}

extern "C" int pea_skipgram_train(int64_t n_pos, int64_t n_neg, int T, int C, int D, const float *table, int64_t ld,
                                  int64_t num_nodes, const int64_t *pos_walks, int64_t pos_stride, const int64_t *neg_walks,
                                  int64_t neg_stride, float *loss, int64_t *n_valid, float *grad, int32_t *touched,
                                  int32_t *touched_count, int32_t *err_flag, void *workspace, size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    PEA_REQUIRE(!tape_active(), PEA_ERR_ARG, "skipgram_train: not recordable on a launch tape (it sorts with rocprim)");
    PEA_REQUIRE(pea_skipgram_supported(D, T, C), PEA_ERR_ARG,
                "skipgram_train: D=%d T=%d C=%d not supported (D a multiple of 4 in 4..128, 2 <= C <= 16, C <= T <= 128)", D, T, C);
    PEA_REQUIRE(n_pos >= 0 && n_neg >= 0 && (n_pos + n_neg) * (int64_t)T < ((int64_t)1 << 31), PEA_ERR_ARG,
                "skipgram_train: %lld + %lld walks of %d ids ((n_pos + n_neg) * T < 2^31)", (long long)n_pos, (long long)n_neg, T);
    PEA_REQUIRE(num_nodes > 0 && num_nodes < ((int64_t)1 << 31) && table && ld >= D && ld % 4 == 0 && aligned16(table), PEA_ERR_ARG,
                "skipgram_train: table [num_nodes, D] with a row stride that is a multiple of 4 and a 16-byte aligned start expected");
    PEA_REQUIRE((pos_walks || n_pos == 0) && (neg_walks || n_neg == 0) && pos_stride >= T && neg_stride >= T, PEA_ERR_ARG,
                "skipgram_train: walks missing or walk stride below T");
    PEA_REQUIRE(loss && n_valid && grad && aligned16(grad) && touched && touched_count && err_flag, PEA_ERR_ARG, "skipgram_train: null output");
    SgLayout L;
    PEA_REQUIRE(sg_layout(n_pos, n_neg, T, C, D, &L), PEA_ERR_HIP, "skipgram_train: rocprim size query failed");
    PEA_REQUIRE(workspace && workspace_bytes >= L.total, PEA_ERR_NOMEM, "skipgram_train: workspace too small (%zu < %zu bytes)",
                workspace_bytes, L.total);
    char *ws = reinterpret_cast<char *>(aligned_ws(workspace));
    int *flag = err_flag;
    u64 *keys = reinterpret_cast<u64 *>(ws + L.keys), *sorted = reinterpret_cast<u64 *>(ws + L.sorted);
    unsigned char *flags = reinterpret_cast<unsigned char *>(ws + L.flags);
    float *walk_loss = reinterpret_cast<float *>(ws + L.walk_loss), *partial = reinterpret_cast<float *>(ws + L.partial);
    float *posgrad = reinterpret_cast<float *>(ws + L.posgrad);
    u64 *nv = reinterpret_cast<u64 *>(n_valid);
    const long long rows = n_pos + n_neg, n = rows * T, n_chunks = (n + kPiece - 1) / kPiece;
    const int pos_bits = bits_for((u64)(n > 0 ? n - 1 : 0)), id_bits = bits_for((u64)num_nodes), g_shift = group_shift(D);
    SgWalks a{reinterpret_cast<const long long *>(pos_walks), reinterpret_cast<const long long *>(neg_walks), (long long)n_pos,
              (long long)n_neg, (long long)pos_stride, (long long)neg_stride, (long long)num_nodes, T, C, D};

    PEA_HIP(hipMemsetAsync(flag, 0, sizeof(int), stream));
    PEA_HIP(hipMemsetAsync(n_valid, 0, 2 * sizeof(int64_t), stream));
    PEA_HIP(hipMemsetAsync(touched_count, 0, sizeof(int32_t), stream));
    {
        ProfScope ps("sg_grad_zero", stream, (double)num_nodes * D * 4.0);
        PEA_HIP(hipMemsetAsync(grad, 0, (size_t)num_nodes * D * sizeof(float), stream));
    }
    if (n > 0) {
        {
            ProfScope ps("sg_keys", stream, (double)n * 16.0);
            PEA_LAUNCH(sg_keys_kernel, dim3((unsigned)((n + 256 * kKeysPerThread - 1) / (256 * kKeysPerThread))), dim3(256), 0, stream, a, n, pos_bits, keys, nv, flag);
            PEA_HIP(hipGetLastError());
        }
        {
            const size_t lds = ((size_t)T * (D + kPad) + (size_t)(T - C + 1) * (C - 1) + T) * 4;
            PEA_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(&sg_walk_kernel), (size_t)(128 * (128 + kPad) + 113 * 15 + 128) * 4));
            ProfScope ps("sg_walk", stream, (double)n * D * 8.0 + (double)n * 8.0);     // rows read once, gradient rows written once
            PEA_LAUNCH(sg_walk_kernel, dim3((unsigned)rows), dim3(kWalkThreads), lds, stream, a, g_shift, table, (long long)ld,
                       (const u64 *)nv, posgrad, walk_loss);
            PEA_HIP(hipGetLastError());
        }
        {
            ProfScope ps("sg_sort", stream, (double)n * 16.0);
            size_t temp = L.temp_bytes;
            PEA_HIP(rocprim::radix_sort_keys(ws + L.temp, temp, (const u64 *)keys, sorted, (size_t)n, 0u, (unsigned)(pos_bits + id_bits), stream));
        }
        {
            ProfScope ps("sg_runs", stream, (double)n * D * 4.0 + (double)n * 9.0);
            const long long threads = n << g_shift;
            PEA_LAUNCH(sg_runs_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, n, (const u64 *)sorted, pos_bits,
                       (u64)num_nodes, (const float *)posgrad, D, g_shift, grad, partial, flags);
            PEA_HIP(hipGetLastError());
        }
        if (n_chunks > 1) {
            ProfScope ps("sg_merge", stream, (double)n_chunks * 16.0);
            const long long threads = (n_chunks - 1) << g_shift;
            PEA_LAUNCH(sg_merge_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, n, n_chunks, (const u64 *)sorted,
                       pos_bits, (u64)num_nodes, D, g_shift, (const float *)partial, grad);
            PEA_HIP(hipGetLastError());
        }
        {
            ProfScope ps("sg_touched", stream, (double)n * 9.0);
            size_t temp = L.temp_bytes;
            PEA_HIP(rocprim::select(ws + L.temp, temp, rocprim::make_transform_iterator((const u64 *)sorted, KeyToId{pos_bits}),
                                    (const unsigned char *)flags, touched, touched_count, (size_t)n, stream));
        }
    }
    ProfScope ps("sg_final", stream, (double)rows * 4.0);
    PEA_LAUNCH(sg_final_kernel, dim3(1), dim3(1024), 0, stream, (long long)n_pos, (long long)n_neg, (const float *)walk_loss,
               (const u64 *)nv, loss);
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}
