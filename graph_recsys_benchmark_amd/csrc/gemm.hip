// Dense per-layer transforms of the PEA path for gfx950: h = x.W^T (GAT), x.W (GCN),
// lin_rel(mean) + lin_root(x) (SAGE) -- the torch.nn.Linear / matmul calls inside the PyG convs
// (reference call site graph_recsys_benchmark/models/base.py:138-139, SURVEY.md 2.1 "dense transform").
//
// The weights of every layer are re-packed each forward (they change every optimizer step) into
// k-major blocks  B[k][col]  so one GEMM job can serve several channels that share the same input
// (all P first-layer channels read the same x, models/base.py:192-193).
//
// f32-input MFMA (exact fp32 products, fp32 accumulation).  Five kernels; a body reads: row tile, load A, walk B, store.
// The k order of one MFMA step is what makes two kernels round differently (host side: plan_gemm_launches picks the kernel).
//   gemm_persist_kernel        (k <= 128): persistent workgroups keep the whole k-major B (+ bias row) in LDS; one wave owns
//                              a 32-row tile, its A fragment in registers, and walks 32-column tiles: 16 LDS reads ahead, 32
//                              v_mfma_f32_32x32x2_f32, 16 stores with no memory wait anywhere in the column loop.
//                              k order: a step takes k and k + 4 (lane (r, h) holds float4 chunks 2q + h of row r).
//   gemm_skinny_kernel         (<= 16 output columns): 64 rows per wave, 4 independent v_mfma_f32_16x16x4_f32 chains, float4
//                              stores.  k order: a step takes k, k + 4, k + 8, k + 12 (lane (j, q): float4 chunks 4i + q).
//   gemm_mfma_kernel           (k > 128, staged fallback): (column tile, 128-deep k chunk) stages through a double-buffered
//                              LDS image.  k order: chunks in order, a step takes k and k + 64.
//   gemm_deep_kernel           (k > 128): one stage per 128-deep k chunk for all column tiles.  k order: as gemm_mfma_kernel.
//   gemm_deep_resident_kernel  (k > 128, B fits the LDS): no barrier after the copy.  k order: 64-deep chunks in order, a
//                              step takes k and k + 4.
// Shared: job_rows / source_row / RowTile (which rows a wave owns), a_row / a_src / a_bias / a_fix (one input row with the
// edge-less-row substitution; every kernel loads A through them), find_out (where a column goes; every kernel), store_tile
// (the 16 stores of a 32x32 tile).  gemm_persist_kernel shares load_a, find_out and load_orow only: its row preamble, segment
// preload, gate chain and store epilogue stay written out in its body (see the comment on it).
// Measured (profiles/tools/gemm_bench.cpp, mfma_peak.cpp, mfma_lds.cpp): the fp32 matrix pipe sustains 154 TFLOP/s on this
// part; the [N,64]x[64,576] first-layer transform runs at 66-75 TFLOP/s because fp32 MFMA chains and an HBM store stream
// are additive here (profiles/tools/overlap_probe.cpp: two kernels on two streams, or specialised waves of one kernel,
// dword or float4 stores: t(both) = t(MFMA) + t(stores) within 3 %): 0.17 ms of MFMA chains + 0.09 ms for 630 MB of
// output = 0.26 ms, measured 0.27 ms (rocBLAS: 0.35 ms).
#include <algorithm>
#include <cstdlib>

#include "common.h"

namespace pea {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kMaxBatch = 12;
struct GemmBatch {
    int n;
    GemmJob j[kMaxBatch];
};

// ---------------------------------------------------------------------------------------------- row tile
// The rows a job covers: its own row list where it has one, else the launch's (null list = rows 0 .. n - 1).  LISTED =
// false: the launch has no list anywhere, known at compile time.
struct RowSet {
    const int *rows;
    int64_t n;
};
template <bool LISTED = true>
__device__ __forceinline__ RowSet job_rows(const GemmJob &J, const int *rows, int64_t n_rows) {
    if (!LISTED) return RowSet{nullptr, n_rows};
    return J.rows ? RowSet{J.rows, J.n_rows} : RowSet{rows, n_rows};
}
// row g of the set: whether it exists, and the table row it names (0 when it does not, so that every address stays valid)
__device__ __forceinline__ int64_t source_row(const RowSet &R, int64_t g, bool &rv) {
    rv = g < R.n;
    return rv ? (R.rows ? (int64_t)R.rows[g] : g) : 0;
}

// A wave's 32-row tile.  Lane (r, h) reads input row row0 + r (rv, srow) and stores accumulator rows (reg & 3) + 8 *
// (reg >> 2) + 4 * h: orow holds their ids (row-list jobs; loaded once per tile), valid the bit mask of those inside the
// job.  The constructor resolves the input row; load_ids, a step of its own so that a kernel can issue its A loads first,
// fills orow and valid.  (gemm_persist_kernel keeps its own preamble, see the comment on it; it calls load_orow directly
// and, unlisted, skips it for a full tile.)
struct RowTile {
    RowSet R;
    int64_t row0, srow;
    bool rv, listed;
    int orow[16];
    unsigned valid;
    __device__ __forceinline__ RowTile(const RowSet &R_, int64_t row0_, int lane)
        : R(R_), row0(row0_), listed(R_.rows != nullptr), valid(0xffffu) {
        srow = source_row(R, row0 + (lane & 31), rv);
    }
    // Row ids of the lane's 16 accumulator rows and the bit mask of those inside the job; consuming the loads here keeps
    // memory waits out of the epilogue.  (A function of its own that returns the mask: written into `valid` in place, the
    // same statements cost the persistent kernel two more spilled registers.)
    static __device__ __forceinline__ unsigned load_orow(const int *rows, int64_t row0, int h, int64_t n_rows, int (&orow)[16]) {
        unsigned valid = 0;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int64_t g = row0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
            orow[reg] = g < n_rows ? (rows ? rows[g] : (int)g) : 0;
            valid |= (g < n_rows ? 1u : 0u) << reg;
        }
        if (rows) {
            int probe = 0;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) probe |= orow[reg];
            if (probe < 0) valid = 0;  // never true (ids are non-negative): makes the loads complete here
        }
        return valid;
    }
    __device__ __forceinline__ void load_ids(int h) { valid = load_orow(R.rows, row0, h, R.n, orow); }
};

// ---------------------------------------------------------------------------------------------- A operand
// One input row as a lane reads it: block pointers, and the edge-less-row substitution where the row is flagged.
// PLAIN (the backward's products): one input block, no substitution -- nothing but p1 and rv is formed.
struct ARow {
    const float *p1, *p2;
    bool rv, alt;
    float sc;
};
template <bool PLAIN = false>
__device__ __forceinline__ ARow a_row(const GemmJob &J, int64_t srow, bool rv) {
    if (PLAIN) return ARow{J.A1 + srow * J.lda1, nullptr, rv, false, 1.f};
    const bool alt = J.a1_mask != nullptr && rv && J.a1_mask[srow] != 0;
    float sc = 1.f;
    if (J.a1_scale) {
        const float di = J.a1_scale[srow];
        sc = alt ? di * di : 1.f;
    }
    const float *p1 = alt ? J.a1_alt + srow * J.lda_alt : J.A1 + srow * J.lda1;
    const float *p2 = J.K2 > 0 ? J.A2 + srow * J.lda2 : p1;
    return ARow{p1, p2, rv, alt, sc};
}
// address of float4 chunk k of the row: first block, second block, or (k past the end) a valid address to be zeroed later
template <bool PLAIN = false>
__device__ __forceinline__ const float *a_src(const GemmJob &J, const ARow &R, int k) {
    if (PLAIN) return R.p1 + (k < J.K1 ? k : 0);
    const bool ok = k < J.K1 + J.K2;
    return (k < J.K1 || !ok) ? R.p1 + (ok ? k : 0) : R.p2 + (k - J.K1);
}
// chunk k of the substitution's bias (the same for every row)
__device__ __forceinline__ float4 a_bias(const GemmJob &J, int k) {
    return (J.a1_mask != nullptr && J.a1_bias != nullptr && k < J.K1) ? ld4(J.a1_bias + k) : make_float4(0.f, 0.f, 0.f, 0.f);
}
// a loaded chunk as the MFMA takes it: substituted (sub: the row is flagged and k lies in the first block), zero unless keep
// (the row exists and k < K).  The callers form the two predicates: with the job and the row passed in and `k < K1 + K2`
// formed here, gemm_persist_kernel came out as another instruction stream, and a slower one.
__device__ __forceinline__ float4 a_fix(bool sub, float sc, bool keep, float4 t, float4 bv) {
    if (sub) {  // same roundings as the aggregation kernel's finish_row: product, + bias, relu
        t = make_float4(fmaxf(sc * t.x + bv.x, 0.f), fmaxf(sc * t.y + bv.y, 0.f), fmaxf(sc * t.z + bv.z, 0.f),
                        fmaxf(sc * t.w + bv.w, 0.f));
    }
    return make_float4(keep ? t.x : 0.f, keep ? t.y : 0.f, keep ? t.z : 0.f, keep ? t.w : 0.f);
}

// Branch-free A fragment load: every lane issues all its float4 loads back to back (invalid rows / k-ranges are
// clamped to a valid address and zeroed afterwards), then the edge-less-row transform is applied with selects.
template <int KH, bool IL = false>
__device__ __forceinline__ void load_a(const GemmJob &J, int64_t srow, bool rv, int kbase, float (&a)[KH]) {
    // IL: the two k-halves of a row interleave by float4 (kbase = chunk start + 4h, chunks 8 floats apart): one load
    // instruction then reads 32 contiguous bytes per row instead of two 16-byte pieces 128+ bytes apart
    const int K = J.K1 + J.K2;
    const ARow R = a_row(J, srow, rv);
    float4 v[KH / 4], bv[KH / 4];
#pragma unroll
    for (int q = 0; q < KH / 4; ++q) {
        const int k = IL ? kbase + q * 8 : kbase + q * 4;
        v[q] = ld4(a_src(J, R, k));
        bv[q] = a_bias(J, k);
    }
#pragma unroll
    for (int q = 0; q < KH / 4; ++q) {
        const int k = IL ? kbase + q * 8 : kbase + q * 4;
        const float4 t = a_fix(R.alt && k < J.K1, R.sc, rv && k < K, v[q], bv[q]);
        a[q * 4 + 0] = t.x;
        a[q * 4 + 1] = t.y;
        a[q * 4 + 2] = t.z;
        a[q * 4 + 3] = t.w;
    }
}
// The plain, interleaved form for the resident kernel, whose 128-register budget has no room for the loaded chunks
// beside the fragment: each chunk is fixed up as it is loaded (the loads still go out together; the compiler moves them).
template <int KH>
__device__ __forceinline__ void load_a_plain(const GemmJob &J, int64_t srow, bool rv, int kbase, float (&a)[KH]) {
    const ARow R = a_row<true>(J, srow, rv);
#pragma unroll
    for (int q = 0; q < KH / 4; ++q) {
        const int k = kbase + q * 8;
        const float4 t = a_fix(false, 1.f, rv && k < J.K1, ld4(a_src<true>(J, R, k)), make_float4(0.f, 0.f, 0.f, 0.f));
        a[q * 4 + 0] = t.x;
        a[q * 4 + 1] = t.y;
        a[q * 4 + 2] = t.z;
        a[q * 4 + 3] = t.w;
    }
}

// ---------------------------------------------------------------------------------------------- epilogue
// Segments of a job in registers, the unused entries emptied: a loop that reads them has no scalar-memory wait.
__device__ __forceinline__ void load_segments(const GemmJob &J, GemmSegment (&S)[kMaxSegments]) {
    const int n_seg = J.n_seg;
#pragma unroll
    for (int sg = 0; sg < kMaxSegments; ++sg) {
        S[sg] = J.seg[sg < n_seg ? sg : 0];
        if (sg >= n_seg) S[sg].c1 = S[sg].c0;
    }
}

// Where column c of a job's output goes.  The job is wave-uniform, so the segment table is read with scalar loads (or
// sits in registers: load_segments) and the per-lane answer is a chain of selects (no memory wait in the epilogue).
struct OutCol {
    float *dst;
    int ld, relu;
};
__device__ __forceinline__ OutCol find_out(const GemmSegment *seg, int n_seg, int n_out, int c) {
    OutCol o{nullptr, 0, 0};
    for (int sg = 0; sg < n_seg; ++sg) {
        const bool in = c >= seg[sg].c0 && c < seg[sg].c1;
        o.dst = in ? seg[sg].dst + (c - seg[sg].c0) : o.dst;
        o.ld = in ? seg[sg].ld : o.ld;
        o.relu = in ? seg[sg].relu : o.relu;
    }
    if (c >= n_out) o.dst = nullptr;
    return o;
}

// Accumulator rows of a lane: (reg & 3) + 8 * (reg >> 2) + 4 * h.  All 16 stores are issued back to back: nothing in
// here may wait on memory (a wait between two stores serialises them on the store acknowledgements, which is what
// bounded the first version of this epilogue).  T.orow: row ids of a row-list job, loaded once per tile; null-list jobs
// address arithmetically.
__device__ __forceinline__ void store_tile(const f32x16 &acc, const OutCol o, float bias, const RowTile &T, int h) {
    if (!o.dst) return;
    float v[16];  // every value first, in straight-line code: the predicated stores below then touch no loaded register
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const float t = acc[reg] + bias;
        v[reg] = o.relu ? fmaxf(t, 0.f) : t;
    }
    if (T.listed) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg)
            if ((T.valid >> reg) & 1u) o.dst[(int64_t)T.orow[reg] * o.ld] = v[reg];
        return;
    }
    float *p = o.dst + (T.row0 + 4 * h) * o.ld;
    if (T.valid == 0xffffu) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) p[(int64_t)((reg & 3) + 8 * (reg >> 2)) * o.ld] = v[reg];
    } else {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg)
            if ((T.valid >> reg) & 1u) p[(int64_t)((reg & 3) + 8 * (reg >> 2)) * o.ld] = v[reg];
    }
}

// ---------------------------------------------------------------------------------------------- staged B
// One stage of a double-buffered B image, 256 threads: rows [k0, k0 + 256 * NLD / (W / 4)) x columns [col0, col0 + W) of
// the job's k-major B, fetched into registers while the previous stage's MFMAs run, stashed after them.
template <int W, int NLD>
__device__ __forceinline__ void fetch_b(const GemmJob &J, int k0, int col0, int tid, float4 (&pre)[NLD]) {
    const int K = J.K1 + J.K2;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int idx = tid + i * 256;
        const int k = k0 + idx / (W / 4), c = col0 + (idx % (W / 4)) * 4;
        pre[i] = (k < K && c < J.b_cols) ? ld4(J.B + (size_t)k * J.ldb + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
template <int W, int NLD>
__device__ __forceinline__ void stash_b(float *img, int tid, const float4 (&pre)[NLD]) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int idx = tid + i * 256;
        *reinterpret_cast<float4 *>(img + (idx / (W / 4)) * W + (idx % (W / 4)) * 4) = pre[i];
    }
}

// 4 waves = 4 row tiles per block share each 32-column B tile through a double-buffered LDS image
// (one barrier per stage; the next tile's global loads are in flight during the MFMAs).
template <int KH>
__global__ __launch_bounds__(256) void gemm_mfma_kernel(const GemmBatch Bt, const int *__restrict__ rows, int64_t n_rows) {
    __shared__ float Bs[2][2 * KH][32];
    constexpr int NLD = (2 * KH * 32 / 4) / 256;  // float4 loads per thread per B tile
    const GemmJob &J = Bt.j[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    RowTile T(job_rows(J, rows, n_rows), ((int64_t)blockIdx.x * 4 + (tid >> 6)) * 32, lane);
    const int K = J.K1 + J.K2;
    const int nkc = (K + 2 * KH - 1) / (2 * KH), nct = (J.n_out + 31) / 32;
    const int n_stage = nkc * nct;
    float a[KH];
    if (nkc == 1) load_a<KH>(J, T.srow, T.rv, h * KH, a);
    T.load_ids(h);

    float4 pre[NLD];
    auto fetch = [&](int stage) { fetch_b<32>(J, (stage % nkc) * 2 * KH, (stage / nkc) * 32, tid, pre); };
    fetch(0);
    stash_b<32>(&Bs[0][0][0], tid, pre);
    f32x16 acc;
    for (int s = 0; s < n_stage; ++s) {
        __syncthreads();
        const int col0 = (s / nkc) * 32, kci = s % nkc;
        if (s + 1 < n_stage) fetch(s + 1);
        if (kci == 0) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        }
        if (nkc > 1) load_a<KH>(J, T.srow, T.rv, kci * 2 * KH + h * KH, a);
        const float *bs = &Bs[s & 1][h * KH][r];
#pragma unroll
        for (int kk = 0; kk < KH; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], bs[kk * 32], acc, 0, 0, 0);
        if (kci == nkc - 1) {
            // epilogue: this lane owns column c of rows (reg&3) + 8*(reg>>2) + 4*h
            const int c = col0 + r;
            const OutCol o = find_out(J.seg, J.n_seg, J.n_out, c);
            const float bias = (J.bias && c < J.n_out) ? J.bias[c] : 0.f;
            store_tile(acc, o, bias, T, h);
        }
        if (s + 1 < n_stage) stash_b<32>(&Bs[(s + 1) & 1][0][0], tid, pre);
    }
}

extern __shared__ float g_lds[];

// Deep k (K > 128: the first layer's input gradient dx = dT_0 W_cat, K = sum of the channels' hidden widths), outputs up
// to 32 * NCT columns: the staged kernel above walks (column tile, k chunk) stages and so reads every A chunk once per
// column tile and takes a barrier per stage; here a stage is one 128-deep k chunk for ALL column tiles (NCT accumulator
// tiles per wave): A is read once, half the barriers, and the next chunk's A fragment and B tile are in flight during the
// MFMAs.  Same k order per output as the staged kernel (chunks in order, within a chunk kk = 0..63 with the two k-halves
// on the two lane halves).
template <int NCT>
__global__ __launch_bounds__(256) void gemm_deep_kernel(const GemmBatch Bt, const int *__restrict__ rows, int64_t n_rows) {
    constexpr int KH = 64, W = 32 * NCT, NLD = 32 * W / 256;   // float4 loads per thread per B stage (128 x W floats)
    const GemmJob &J = Bt.j[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    RowTile T(job_rows(J, rows, n_rows), ((int64_t)blockIdx.x * 4 + (tid >> 6)) * 32, lane);
    T.load_ids(h);
    const int K = J.K1 + J.K2;
    const int nkc = (K + 2 * KH - 1) / (2 * KH);
    float4 pre[NLD];
    float a[KH], a2[KH];
    f32x16 acc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[ct][i] = 0.f;
    fetch_b<W>(J, 0, 0, tid, pre);
    stash_b<W>(g_lds, tid, pre);
    load_a<KH>(J, T.srow, T.rv, h * KH, a);
    for (int kc = 0; kc < nkc; ++kc) {
        __syncthreads();
        const bool more = kc + 1 < nkc;
        if (more) {
            fetch_b<W>(J, (kc + 1) * 2 * KH, 0, tid, pre);
            load_a<KH>(J, T.srow, T.rv, (kc + 1) * 2 * KH + h * KH, a2);
        }
        const float *bs = g_lds + ((size_t)(kc & 1) * 2 * KH + h * KH) * W + r;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int kk = 0; kk < KH; ++kk) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], bs[kk * W + 32 * ct], acc[ct], 0, 0, 0);
        if (more) {
            stash_b<W>(g_lds + (size_t)((kc + 1) & 1) * 2 * KH * W, tid, pre);
#pragma unroll
            for (int kk = 0; kk < KH; ++kk) a[kk] = a2[kk];
        }
    }
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        const int c = 32 * ct + r;
        const OutCol o = find_out(J.seg, J.n_seg, J.n_out, c);
        const float bias = (J.bias && c < J.n_out) ? J.bias[c] : 0.f;
        store_tile(acc[ct], o, bias, T, h);
    }
}

// Deep k with a B that fits the LDS whole (K x 32 NCT floats <= 150 KB: the 25m model's dx = dT_0 W_cat is 576 x 64 =
// 147 KB): every workgroup copies B once, then its 16 waves walk 32-row tiles with NO barrier, like the persistent kernel
// below, but over k chunks of 64.  NOT the k order of gemm_deep_kernel: one MFMA step here takes k and k + 4 (the lane
// halves interleave by float4, as in the persistent kernel), there k and k + 64, so the two round differently and a
// product is bit-identical only against the same kernel (which one runs follows from the batch's largest k and n_out).
// Its jobs have one input block and no edge-less-row substitution (the backward's products): load_a_plain.
template <int NCT>
__global__ __launch_bounds__(1024) void gemm_deep_resident_kernel(const GemmBatch Bt, const int *__restrict__ rows, int64_t n_rows) {
    constexpr int KH = 32, W = 32 * NCT, NW = 16;   // 64-deep k chunks: 112 registers per lane, 16 waves per CU
    const GemmJob &J = Bt.j[blockIdx.y];
    const RowSet R = job_rows(J, rows, n_rows);
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5, wave = tid >> 6;
    const int K = J.K1 + J.K2;
    const int nkc = (K + 2 * KH - 1) / (2 * KH);
    for (int idx = tid; idx < K * (W / 4); idx += 1024) {   // the whole k-major B: K rows (a partial last chunk re-reads row K - 1
        const int k = idx / (W / 4), c = (idx % (W / 4)) * 4;   // against A values that are zero there)
        *reinterpret_cast<float4 *>(g_lds + (size_t)k * W + c) = c < J.b_cols ? ld4(J.B + (size_t)k * J.ldb + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    const int64_t n_tiles = (R.n + 31) / 32;
    for (int64_t tile = (int64_t)blockIdx.x * NW + wave; tile < n_tiles; tile += (int64_t)gridDim.x * NW) {
        RowTile T(R, tile * 32, lane);
        T.load_ids(h);
        float a[KH];   // no second fragment buffer: 16 waves per CU cover the load latency, a 128-register budget does not fit one
        f32x16 acc[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[ct][i] = 0.f;
        for (int kc = 0; kc < nkc; ++kc) {
            load_a_plain<KH>(J, T.srow, T.rv, kc * 2 * KH + 4 * h, a);   // a[4q + e] = k  kc * 64 + 4 (2q + h) + e
            const float *bs = g_lds + ((size_t)kc * 2 * KH + 4 * h) * W + r;   // image row of a[kl]: + 8 (kl / 4) + kl % 4
            const bool last_partial = (kc + 1) * 2 * KH > K;            // wave-uniform
            const int kbase = kc * 2 * KH + 4 * h;                      // image row of a[0] of this lane half
            // B operands in batches of 8 LDS reads per column tile, fenced: left alone, the scheduler hoists all 64 * NCT
            // reads of the chunk ahead of the MFMAs and spills
#pragma unroll
            for (int g = 0; g < KH / 8; ++g) {
                float bb[NCT][8];
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int kl = 8 * g + u;   // row kc * 128 + h * 64 + kl of the image, clamped in a partial last chunk
                        const int ko = 8 * (kl / 4) + kl % 4;   // interleaved k order of the fragment
                        bb[ct][u] = last_partial ? g_lds[(size_t)min(kbase + ko, K - 1) * W + r + 32 * ct] : bs[ko * W + 32 * ct];
                    }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                    for (int u = 0; u < 8; ++u) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[8 * g + u], bb[ct][u], acc[ct], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            const int c = 32 * ct + r;
            const OutCol o = find_out(J.seg, J.n_seg, J.n_out, c);
            const float bias = (J.bias && c < J.n_out) ? J.bias[c] : 0.f;
            store_tile(acc[ct], o, bias, T, h);
        }
    }
}

// Persistent variant (the default): every workgroup first copies the WHOLE k-major B of all its jobs into LDS
// (the 9 first-layer transforms of the MovieLens model are one 64 x 596 block = 149 KiB of the CU's 160 KiB), then its
// 16 waves walk (job, 32-row tile, column group) items with no barrier at all: A fragment from global, B fragment
// from LDS, 32 MFMAs per 32x32 output tile, stores straight from the accumulators.
// Its body shares load_a, find_out and RowTile::load_orow with the other kernels and keeps the rest written out: built on
// RowTile, load_segments and store_tile (the gate an operand of it) its listed launches measured 5 - 7 % slower, and its
// instruction stream follows every statement of the body (profiles/gemm_kernels_refactor.md, sections 1 and 3).  So the row
// override, the segment preload, a gate-only select chain and the relu / gate / store triple exist here a second time.
constexpr int kColGroup = 5;      // 32-column tiles per item
struct PersistArgs {
    int n_items;                   // all jobs
    int col_group;                 // 32-column tiles per item
    int item_start[kMaxBatch + 1]; // first item of job j
    int lds_off[kMaxBatch];        // float offset of job j's B image, row stride lds_ld[j]
    int lds_ld[kMaxBatch];
    int n_tiles[kMaxBatch];        // 32-row tiles of job j (jobs may carry their own row lists)
};

template <int KH, bool LISTED>
__global__ __launch_bounds__(KH > 32 ? 512 : 1024) void gemm_persist_kernel(const GemmBatch Bt, const PersistArgs Pa, const int *__restrict__ rows,
                                                            int64_t n_rows) {
    constexpr int NT = KH > 32 ? 512 : 1024, NW = NT / 64;  // deeper k needs more registers per lane
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    // B images, 8 float4 loads in flight per thread
    for (int j = 0; j < Bt.n; ++j) {
        const GemmJob &J = Bt.j[j];
        const int K = J.K1 + J.K2, ld = Pa.lds_ld[j], q4 = ld / 4, total = 2 * KH * q4;
        const float inv_q4 = 1.0f / (float)q4;
        float4 *dst = reinterpret_cast<float4 *>(g_lds + Pa.lds_off[j]);
        constexpr int U = 8;
        for (int base = 0; base < total; base += NT * U) {
            float4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int idx = base + u * NT + tid;
                const int k = (int)(((float)idx + 0.5f) * inv_q4), c = (idx - k * q4) * 4;
                v[u] = (idx < total && k < K && c < J.b_cols) ? ld4(J.B + (size_t)k * J.ldb + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int idx = base + u * NT + tid;
                if (idx < total) dst[idx] = v[u];
            }
        }
        // row 2*KH of the image: the bias, so the column loop below issues no global load at all (a load there
        // makes every tile wait for the previous tile's stores to be acknowledged)
        for (int c = tid; c < ld; c += NT) g_lds[Pa.lds_off[j] + 2 * KH * ld + c] = (J.bias && c < J.n_out) ? J.bias[c] : 0.f;
    }
    __syncthreads();
    const int stride = gridDim.x * NW;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // item, job and tile are wave-uniform: scalar registers
    for (int item = blockIdx.x * NW + wave; item < Pa.n_items; item += stride) {
        int j = 0;
        while (j + 1 < Bt.n && item >= Pa.item_start[j + 1]) ++j;
        const GemmJob &J = Bt.j[j];
        const int *jrows = LISTED ? (J.rows ? J.rows : rows) : nullptr;
        const int64_t jn = (LISTED && J.rows) ? J.n_rows : n_rows;
        const int local = item - Pa.item_start[j];
        const int n_tiles = Pa.n_tiles[j];
        const int tile = local % n_tiles, grp = local / n_tiles;  // consecutive waves -> consecutive row tiles
        const int64_t row0 = (int64_t)tile * 32, grow = row0 + r;
        const bool rv = grow < jn;
        const int64_t srow = rv ? ((LISTED && jrows) ? (int64_t)jrows[grow] : grow) : 0;
        // everything the column loop needs from the job, read once per item (scalar registers): the loop itself
        // then has no scalar-memory wait, which shares its counter with the LDS reads
        const int n_out = J.n_out, n_seg = J.n_seg;
        GemmSegment S[kMaxSegments];
#pragma unroll
        for (int sg = 0; sg < kMaxSegments; ++sg) {
            S[sg] = J.seg[sg < n_seg ? sg : 0];
            if (sg >= n_seg) S[sg].c1 = S[sg].c0;
        }
        float a[KH];
        load_a<KH, true>(J, srow, rv, 4 * h, a);
        int orow[16];
        unsigned valid = 0xffffu;
        if (LISTED || row0 + 32 > jn) valid = RowTile::load_orow(jrows, row0, h, jn, orow);
        const int ld = Pa.lds_ld[j];
        // k order of a lane: float4 chunks 2q + h of the row (the two halves of a row interleave by 16 bytes, so one
        // load instruction reads 32 contiguous bytes per row); the B image is read with the same permutation
        const float *bimg = g_lds + Pa.lds_off[j] + (4 * h) * ld + r;
        const float *bias_img = g_lds + Pa.lds_off[j] + 2 * KH * ld + r;
        const int nct = (n_out + 31) / 32;
        const int ct_end = min(nct, (grp + 1) * Pa.col_group);
        // gated jobs (col_group <= 2 for them): the gate values of this lane's 16 rows x 2 column tiles are fetched here,
        // before the column loop, which must not issue a global load (see the bias row of the image)
        float gv[2][16];
        const bool gated = S[0].gate != nullptr;   // wave-uniform; a gated job has the gate on every segment
        if (gated) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int c = (grp * Pa.col_group + t) * 32 + r;
                const float *gp = nullptr;
                int ldg = 0;
#pragma unroll
                for (int sg = 0; sg < kMaxSegments; ++sg) {
                    const bool in = c >= S[sg].c0 && c < S[sg].c1;
                    gp = in ? S[sg].gate + (c - S[sg].c0) : gp;
                    ldg = in ? S[sg].ld_gate : ldg;
                }
                const bool col_ok = gp != nullptr && c < n_out && grp * Pa.col_group + t < ct_end;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int64_t rr = (LISTED || row0 + 32 > jn) ? (int64_t)orow[reg] : row0 + 4 * h + (reg & 3) + 8 * (reg >> 2);
                    const bool ok = col_ok && ((valid >> reg) & 1u);
                    gv[t][reg] = ok ? gp[(ok ? rr : 0) * ldg] : 1.f;
                }
            }
        }
        for (int ct = grp * Pa.col_group; ct < ct_end; ++ct) {
            const int col0 = ct * 32, c = col0 + r;
            const float bias = bias_img[col0];
            f32x16 acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
            // B fragment in batches of 8 LDS reads, the next batch issued before this batch's MFMAs
            float bb[2][8];
#pragma unroll
            for (int u = 0; u < 8; ++u) bb[0][u] = bimg[(8 * (u / 4) + u % 4) * ld + col0];
#pragma unroll
            for (int g = 0; g < KH / 8; ++g) {
                if (g + 1 < KH / 8) {
#pragma unroll
                    for (int u = 0; u < 8; ++u) bb[(g + 1) & 1][u] = bimg[(16 * (g + 1) + 8 * (u / 4) + u % 4) * ld + col0];
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[8 * g + u], bb[g & 1][u], acc, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            // epilogue: lane (r, h) owns column c of rows (reg & 3) + 8 * (reg >> 2) + 4h.  Nothing in here waits on
            // memory, so the 16 stores go out back to back.
            const OutCol o = find_out(S, kMaxSegments, n_out, c);
            if (!o.dst) continue;
            float *dst = o.dst;
            const int ldo = o.ld, relu = o.relu;
            float v[16];
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const float t = acc[reg] + bias;
                v[reg] = relu ? fmaxf(t, 0.f) : t;
            }
            if (gated) {
                const int t = ct - grp * Pa.col_group;   // 0 or 1
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) v[reg] = (t == 0 ? gv[0][reg] : gv[1][reg]) > 0.f ? v[reg] : 0.f;
            }
            if (LISTED) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg)
                    if ((valid >> reg) & 1u) dst[(int64_t)orow[reg] * ldo] = v[reg];
            } else {
                float *p = dst + (row0 + 4 * h) * ldo;
                if (valid == 0xffffu) {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) p[(int64_t)((reg & 3) + 8 * (reg >> 2)) * ldo] = v[reg];
                } else {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg)
                        if ((valid >> reg) & 1u) p[(int64_t)((reg & 3) + 8 * (reg >> 2)) * ldo] = v[reg];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- narrow outputs
// Transforms with at most 16 output columns (the last layer of every PEA channel: hidden -> repr_dim = 16) are bound
// by how fast the [rows, K] input streams in, not by the matrix pipe, and a 32x32 tile would waste half of it.  One
// wave owns 64 rows: 4 independent v_mfma_f32_16x16x4_f32 chains (one per 16-row group) with the WEIGHTS as the row
// operand, so lane (j = lane % 16, q = lane / 16) ends up with row j's columns 4q..4q+3 -- one float4 store -- and its
// 16 float4 input loads (all four groups) are issued before anything waits on them: twice the bytes in flight per
// wave of the 32-row kernel.  k order per lane: float4 chunks 4i + q of the row (the four lanes of a row read 64
// contiguous bytes per instruction); the weight image in LDS is read with the same permutation.

struct SkinnyArgs {
    // > 0: every job has this many 64-row tiles and item i is (tile i / n_jobs, job i % n_jobs): the jobs of a level read
    // adjacent column blocks of the SAME rows (one 256-byte piece each out of a 2304-byte row), so waves that run together
    // then sweep whole rows instead of nine strided passes over the table (PEA_SKINNY_JOBMAJOR=1: the old job-major order)
    int tiles_per_job;
    int n_items;
    int item_start[kMaxBatch + 1];  // first item (64-row tile) of job j
    int lds_off[kMaxBatch];         // float offset of job j's image: [KQ*16][16] weights + [16] bias
};

template <int KQ, bool LISTED>  // KQ float4 chunks per lane and 16-row group: K <= 16 * KQ
__global__ __launch_bounds__(512) void gemm_skinny_kernel(const GemmBatch Bt, const SkinnyArgs Sa, const int *__restrict__ rows,
                                                          int64_t n_rows) {
    constexpr int KP = 16 * KQ, G = 4;
    const int tid = threadIdx.x, lane = tid & 63, jr = lane & 15, q = lane >> 4;
    for (int j = 0; j < Bt.n; ++j) {
        const GemmJob &J = Bt.j[j];
        const int K = J.K1 + J.K2;
        float *img = g_lds + Sa.lds_off[j];
        for (int idx = tid; idx < KP * 16; idx += 512) {
            const int k = idx >> 4, c = idx & 15;
            img[idx] = (k < K && c < J.n_out) ? J.B[(size_t)k * J.ldb + c] : 0.f;
        }
        if (tid < 16) img[KP * 16 + tid] = (J.bias && tid < J.n_out) ? J.bias[tid] : 0.f;
    }
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int stride = gridDim.x * 8;
    for (int item = blockIdx.x * 8 + wave; item < Sa.n_items; item += stride) {
        int j = 0, tile;
        if (Sa.tiles_per_job > 0) {
            tile = item / Bt.n;
            j = item - tile * Bt.n;
        } else {
            while (j + 1 < Bt.n && item >= Sa.item_start[j + 1]) ++j;
            tile = item - Sa.item_start[j];
        }
        const GemmJob &J = Bt.j[j];
        const RowSet R = job_rows<LISTED>(J, rows, n_rows);
        const int64_t row0 = (int64_t)tile * (16 * G);
        const int K = J.K1 + J.K2, K1 = J.K1, n_out = J.n_out;
        GemmSegment S[kMaxSegments];
        load_segments(J, S);
        // ---- input rows: all G * KQ float4 loads of the lane go out before the first use
        int64_t srow[G];
        bool rv[G];
#pragma unroll
        for (int g = 0; g < G; ++g) srow[g] = source_row(R, row0 + 16 * g + jr, rv[g]);
        ARow ar[G];
#pragma unroll
        for (int g = 0; g < G; ++g) ar[g] = a_row(J, srow[g], rv[g]);
        float4 xa[G][KQ];
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int i = 0; i < KQ; ++i) xa[g][i] = ld4(a_src(J, ar[g], 16 * i + 4 * q));
        float4 ab[KQ];  // bias of the edge-less-row transform (same for every row)
#pragma unroll
        for (int i = 0; i < KQ; ++i) ab[i] = a_bias(J, 16 * i + 4 * q);
        // ---- weights of this job: lane (col = jr, q) holds W[16i + 4q + e][jr]
        const float *img = g_lds + Sa.lds_off[j];
        float w[KQ][4];
#pragma unroll
        for (int i = 0; i < KQ; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) w[i][e] = img[(16 * i + 4 * q + e) * 16 + jr];
        const float4 bias = *reinterpret_cast<const float4 *>(img + KP * 16 + 4 * q);
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int i = 0; i < KQ; ++i) {
                const int k = 16 * i + 4 * q;
                xa[g][i] = a_fix(ar[g].alt && k < K1, ar[g].sc, rv[g] && k < K, xa[g][i], ab[i]);
            }
        f32x4 acc[G];
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < KQ; ++i) {
#pragma unroll
            for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i][0], xa[g][i].x, acc[g], 0, 0, 0);
#pragma unroll
            for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i][1], xa[g][i].y, acc[g], 0, 0, 0);
#pragma unroll
            for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i][2], xa[g][i].z, acc[g], 0, 0, 0);
#pragma unroll
            for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i][3], xa[g][i].w, acc[g], 0, 0, 0);
        }
        // ---- epilogue: columns c .. c+3 of row srow[g]
        const OutCol o = find_out(S, kMaxSegments, n_out, 4 * q);
        if (!o.dst) continue;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float4 v = make_float4(acc[g][0] + bias.x, acc[g][1] + bias.y, acc[g][2] + bias.z, acc[g][3] + bias.w);
            if (o.relu) v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
            if (rv[g]) *reinterpret_cast<float4 *>(o.dst + srow[g] * o.ld) = v;
        }
    }
}


constexpr int kMaxPack = 24;   // layers per pack launch (the launch record travels as a kernel argument)
struct PackLaunch {
    int n;
    PackJob j[kMaxPack];
};

// one block per layer: writes the k-major weight block (and the folded attention columns)
__global__ __launch_bounds__(256) void pack_kernel(const PackLaunch L) {
    const PackJob &J = L.j[blockIdx.x];
    const int tid = threadIdx.x;
    int krows = J.in;
    if (J.kind == PEA_KIND_GAT) {
        for (int idx = tid; idx < J.HF * J.in; idx += 256) {
            const int o = idx / J.in, k = idx % J.in;
            J.B[(size_t)k * J.ldb + o] = J.w0[idx];
        }
        for (int o = tid; o < J.HF; o += 256) {
            // log2(e) folded in: the aggregation kernels keep logits in the log2 domain (leaky_relu commutes with a
            // positive scale), so every softmax weight is a single v_exp_f32
            J.att_dst[o] = J.w1[o];  // att_i multiplies the TARGET row (natural units: the exponent takes log2(e), agg_common.h)
            J.att_src[o] = J.w2[o];  // att_j multiplies the SOURCE row
        }
    } else if (J.kind == PEA_KIND_GCN) {
        for (int idx = tid; idx < J.in * J.HF; idx += 256) {
            const int k = idx / J.HF, o = idx % J.HF;
            J.B[(size_t)k * J.ldb + o] = J.w0[idx];
        }
    } else if (J.kind == PEA_PACK_SAGE2) {  // two k-major blocks: lin_rel^T (the gather source's transform), lin_root^T
        for (int idx = tid; idx < J.HF * J.in; idx += 256) {
            const int o = idx / J.in, k = idx % J.in;
            J.B[(size_t)k * J.ldb + o] = J.w0[idx];
            J.B2[(size_t)k * J.ldb2 + o] = J.w1[idx];
        }
        for (int idx = tid; idx < J.in * (J.ldb2 - J.HF); idx += 256) {
            const int k = idx / (J.ldb2 - J.HF), c = idx % (J.ldb2 - J.HF);
            J.B2[(size_t)k * J.ldb2 + J.HF + c] = 0.f;
        }
    } else {
        krows = 2 * J.in;
        for (int idx = tid; idx < J.HF * J.in; idx += 256) {
            const int o = idx / J.in, k = idx % J.in;
            J.B[(size_t)k * J.ldb + o] = J.w0[idx];
            J.B[(size_t)(J.in + k) * J.ldb + o] = J.w1[idx];
        }
    }
    for (int idx = tid; idx < krows * J.zero_n; idx += 256) {
        const int k = idx / J.zero_n, c = idx % J.zero_n;
        J.B[(size_t)k * J.ldb + J.zero_col + c] = 0.f;
    }
    for (int o = tid; o < J.HF; o += 256) J.bias[o] = J.w3 ? J.w3[o] : 0.f;
}

}  // namespace

// ---------------------------------------------------------------- host side: plan, then launch
// plan_gemm_launches decides what launch_gemm_batch issues, with no device and no environment (pea_dense_route shows the same
// decision where no GPU is).  The kernels differ in k summation order, so the rules are bit-relevant; DESIGN.md section 4 has
// them as a table.  In this order: the gate check; narrow jobs (skinny_ok) to the skinny kernel, one launch per k class (k <=
// 32 / 64 / 128: KH = 16 / 32 / 64, KQ = KH / 8); of the others, those with k <= 128 to the persistent kernel per k class,
// cut into column chunks where the B image exceeds the LDS budget, a launch closing when the next image would not fit; then
// k > 128, the deep kernel chosen per launch (close_deep).  At most kMaxBatch jobs per launch; jobs are checked (check_job) as
// they are reached and dropped when they have no rows.
constexpr size_t kLdsBudget = 160 * 1024 - 1024;  // dynamic LDS a workgroup may claim (one workgroup per CU)
static_assert(kMaxBatch == PEA_ROUTE_MAX_JOBS, "pea_dense_route_entry holds one index per batch entry");

struct GemmEnv {   // the A/B switches, read once per call by the caller of the planner
    bool deep_staged;      // PEA_DEEP_STAGED=1: every deep launch on the per-column-tile staged kernel
    bool skinny_jobmajor;  // PEA_SKINNY_JOBMAJOR=1: the skinny kernel's old job-major item order
};
static GemmEnv gemm_env() {
    const char *deep = getenv("PEA_DEEP_STAGED"), *major = getenv("PEA_SKINNY_JOBMAJOR");
    return GemmEnv{deep && atoi(deep) != 0, major && atoi(major) != 0};
}

struct GemmLaunch {
    GemmLaunch() {}        // filled in place by the planner: nothing of its ~4 KB is cleared first
    int family, variant;   // PEA_ROUTE_*; KQ (skinny), KH (persist), NCT (deep resident / chunk), 64 (staged)
    bool listed;           // some job reads a row list
    GemmBatch Bt;          // chunk rewrites and b_cols applied
    int src[kMaxBatch];    // index of each batch entry's job in the caller's list
    PersistArgs Pa;        // PEA_ROUTE_PERSIST
    SkinnyArgs Sa;         // PEA_ROUTE_SKINNY
    size_t lds;            // dynamic LDS bytes
    const char *name;      // profile name
    double bytes;          // attributed to the launch
    int per_cu;            // grid = (per_cu ? min(per_cu * CUs, blocks) : blocks, deep kernels: one grid row per job)
    int64_t blocks;
};
struct GemmPiece {   // columns [c0, c1) of job src (all of them unless the job was cut), on their way into a launch
    int src, c0, c1;
    int family, KH;  // PEA_ROUTE_SKINNY, _PERSIST or _DEEP_STAGED (k > 128: the launch picks the deep kernel); k class
};

static int check_job(const GemmJob &job) {
    PEA_REQUIRE(job.K1 > 0 && job.K1 % 4 == 0 && job.K2 % 4 == 0, PEA_ERR_ARG,
                "gemm: input widths (%d, %d) must be multiples of 4", job.K1, job.K2);
    PEA_REQUIRE(job.n_out > 0 && job.ldb >= job.n_out, PEA_ERR_ARG, "gemm: output width %d / ldb %d", job.n_out, job.ldb);
    PEA_REQUIRE(job.lda1 % 4 == 0 && (job.K2 == 0 || job.lda2 % 4 == 0), PEA_ERR_ARG,
                "gemm: input row strides must be multiples of 4 floats");
    PEA_REQUIRE(job.n_seg > 0 && job.n_seg <= kMaxSegments, PEA_ERR_ARG, "gemm: %d segments", job.n_seg);
    return PEA_OK;
}

// a job qualifies when its output is at most 16 columns wide, k fits 128 and every segment can take float4 stores
static bool skinny_ok(const GemmJob &J) {
    if (J.no_narrow || J.seg[0].gate || J.n_out > 16 || J.K1 + J.K2 > 128 || J.ldb < J.n_out) return false;
    for (int sg = 0; sg < J.n_seg; ++sg) {
        const GemmSegment &S = J.seg[sg];
        if (S.c0 % 4 || S.c1 % 4 || S.ld % 4 || (reinterpret_cast<uintptr_t>(S.dst) & 15)) return false;
    }
    return true;
}

static int k_class(int K) { return K <= 32 ? 16 : K <= 64 ? 32 : 64; }   // KH of the persistent kernel; KQ = KH / 8

static void close_skinny(GemmLaunch &L, int KQ, int64_t n_rows, const GemmEnv &env) {
    SkinnyArgs &Sa = L.Sa;
    int off = 0, items = 0;
    for (int j = 0; j < L.Bt.n; ++j) {
        Sa.lds_off[j] = off;
        off += (16 * KQ + 1) * 16;
        Sa.item_start[j] = items;
        items += (int)(((L.Bt.j[j].rows ? L.Bt.j[j].n_rows : n_rows) + 63) / 64);
    }
    Sa.item_start[L.Bt.n] = items;
    Sa.n_items = items;
    bool same = L.Bt.n > 1;
    for (int j = 1; j < L.Bt.n; ++j) same = same && (Sa.item_start[j + 1] - Sa.item_start[j]) == Sa.item_start[1];
    Sa.tiles_per_job = same && !env.skinny_jobmajor ? Sa.item_start[1] : 0;
    L.family = PEA_ROUTE_SKINNY;
    L.variant = KQ;
    L.name = "gemm_mfma_narrow";
    L.lds = (size_t)off * sizeof(float);
    L.per_cu = 2;
    L.blocks = (items + 7) / 8;
}

static void close_persist(GemmLaunch &L, int KH, int64_t n_rows) {
    PersistArgs &Pa = L.Pa;
    Pa.col_group = kColGroup;
    for (int j = 0; j < L.Bt.n; ++j)
        if (L.Bt.j[j].seg[0].gate) Pa.col_group = 2;   // gated epilogues hold the gate values of two column tiles
    int off = 0, items = 0;
    for (int j = 0; j < L.Bt.n; ++j) {
        const int nct = (L.Bt.j[j].n_out + 31) / 32;
        const int n_tiles = (int)(((L.Bt.j[j].rows ? L.Bt.j[j].n_rows : n_rows) + 31) / 32);
        Pa.n_tiles[j] = n_tiles;
        Pa.lds_ld[j] = nct * 32;
        Pa.lds_off[j] = off;
        off += (2 * KH + 1) * Pa.lds_ld[j];
        Pa.item_start[j] = items;
        items += n_tiles * ((nct + Pa.col_group - 1) / Pa.col_group);
    }
    Pa.item_start[L.Bt.n] = items;
    Pa.n_items = items;
    const int waves = (KH > 32 ? 512 : 1024) / 64;
    L.family = PEA_ROUTE_PERSIST;
    L.variant = KH;
    L.name = L.Bt.n == 1 ? "gemm_mfma_shared" : "gemm_mfma_batch";
    L.lds = (size_t)off * sizeof(float);
    L.per_cu = L.lds * 2 <= kLdsBudget ? 2 : 1;  // two workgroups share a CU when their B images both fit
    L.blocks = (items + waves - 1) / waves;
}

static void close_deep(GemmLaunch &L, int64_t n_rows, const GemmEnv &env) {
    int64_t max_rows = n_rows;
    int max_out = 0, max_k = 0;
    bool plain = true;   // one input block, no edge-less-row substitution: what the resident kernel's loader takes
    for (int q = 0; q < L.Bt.n; ++q) {
        const GemmJob &J = L.Bt.j[q];
        max_rows = std::max<int64_t>(max_rows, J.rows ? J.n_rows : 0);
        max_out = std::max(max_out, J.n_out);
        max_k = std::max(max_k, J.K1 + J.K2);
        plain = plain && J.K2 == 0 && J.a1_mask == nullptr;
    }
    const int nct = max_out <= 32 ? 1 : max_out <= 64 ? 2 : 4;
    const size_t lds_res = (size_t)max_k * 32 * nct * sizeof(float);
    L.name = "gemm_mfma_deep";
    L.variant = nct;
    L.per_cu = 0;
    L.blocks = (max_rows + 127) / 128;
    if (plain && max_out <= 64 && lds_res <= kLdsBudget && !env.deep_staged) {   // (4 column tiles would spill)
        L.family = PEA_ROUTE_DEEP_RESIDENT;   // B resident in LDS, no barriers: persistent workgroups
        L.lds = lds_res;
        L.per_cu = 1;
        L.blocks = std::max<int64_t>(1, ((max_rows + 31) / 32 + 15) / 16);
    } else if (max_out <= 128 && !env.deep_staged) {
        L.family = PEA_ROUTE_DEEP_CHUNK;
        L.lds = (size_t)2 * 128 * 32 * nct * sizeof(float);
    } else {
        L.family = PEA_ROUTE_DEEP_STAGED;
        L.variant = 64;
        L.lds = 0;
    }
}

// The batch entry of a piece: the job itself (b_cols filled in, except for the skinny kernel, which does not read it), or its
// column chunk: B, bias, the segments and their gates move with the columns.
static void place_piece(GemmJob &C, const GemmJob &J, const GemmPiece &P) {
    C = J;
    if (P.family == PEA_ROUTE_SKINNY) return;
    C.b_cols = std::min(J.ldb - P.c0, (P.c1 - P.c0 + 3) / 4 * 4);   // the piece's own columns (GemmJob::b_cols); the image's pad past c1 is not loaded
    if (P.c1 - P.c0 == J.n_out) return;
    C.B = J.B + P.c0;
    C.n_out = P.c1 - P.c0;
    C.bias = J.bias ? J.bias + P.c0 : nullptr;
    C.n_seg = 0;
    for (int sg = 0; sg < J.n_seg; ++sg) {
        const int a0 = std::max(J.seg[sg].c0, P.c0), a1 = std::min(J.seg[sg].c1, P.c1);
        if (a1 <= a0) continue;
        GemmSegment S = J.seg[sg];
        S.dst = J.seg[sg].dst + (a0 - J.seg[sg].c0);
        if (S.gate) S.gate = J.seg[sg].gate + (a0 - J.seg[sg].c0);
        S.c0 = a0 - P.c0;
        S.c1 = a1 - P.c0;
        C.seg[C.n_seg++] = S;
    }
}

// what the batch in L.Bt needs beside its jobs
static void close_launch(GemmLaunch &L, int family, int KH, bool rows_given, int64_t n_rows, const GemmEnv &env) {
    L.listed = rows_given;
    L.bytes = 0.0;
    for (int q = 0; q < L.Bt.n; ++q) {
        const GemmJob &J = L.Bt.j[q];
        L.listed = L.listed || J.rows != nullptr;
        L.bytes += 4.0 * (double)(J.rows ? J.n_rows : n_rows) * (J.K1 + J.K2 + J.n_out);
    }
    if (family == PEA_ROUTE_SKINNY) close_skinny(L, KH / 8, n_rows, env);
    else if (family == PEA_ROUTE_PERSIST) close_persist(L, KH, n_rows);
    else close_deep(L, n_rows, env);
}

// The launches of one launch_gemm_batch call, in issue order.  Pure: no HIP call, no getenv, and of the pointers inside the
// jobs only the segments' dst addresses are looked at (their alignment, skinny_ok); none is dereferenced.
static int plan_gemm_launches(const GemmJob *jobs_in, int n_jobs_in, bool rows_given, int64_t n_rows, const GemmEnv &env,
                              std::vector<GemmLaunch> *out) {
    for (int i = 0; i < n_jobs_in; ++i) {   // a gated epilogue exists in the persistent kernel only (k <= 128)
        bool any = false, all = true;
        for (int sg = 0; sg < jobs_in[i].n_seg; ++sg) {
            any = any || jobs_in[i].seg[sg].gate != nullptr;
            all = all && jobs_in[i].seg[sg].gate != nullptr;
        }
        PEA_REQUIRE(!any || (all && jobs_in[i].K1 + jobs_in[i].K2 <= 128), PEA_ERR_ARG,
                    "gemm: a gated job needs the gate on every segment and k <= 128");
    }
    std::vector<GemmPiece> pieces;
    pieces.reserve((size_t)n_jobs_in);
    for (int KH : {16, 32, 64})   // narrow outputs first, by k class
        for (int i = 0; i < n_jobs_in; ++i) {
            const GemmJob &J = jobs_in[i];
            if (!skinny_ok(J) || k_class(J.K1 + J.K2) != KH) continue;
            PEA_TRY(check_job(J));
            if ((J.rows ? J.n_rows : n_rows) > 0) pieces.push_back({i, 0, J.n_out, PEA_ROUTE_SKINNY, KH});
        }
    for (int i = 0; i < n_jobs_in; ++i) {
        if (skinny_ok(jobs_in[i])) continue;
        PEA_TRY(check_job(jobs_in[i]));
        const GemmJob &J = jobs_in[i];
        if ((J.rows ? J.n_rows : n_rows) <= 0) continue;
        const int K = J.K1 + J.K2, KH = k_class(K);
        const int max_cols = (int)(kLdsBudget / sizeof(float) / (size_t)(2 * KH + 1)) / 32 * 32;
        if (K > 128 || J.n_out <= max_cols) {
            pieces.push_back({i, 0, J.n_out, K > 128 ? PEA_ROUTE_DEEP_STAGED : PEA_ROUTE_PERSIST, KH});
            continue;
        }
        for (int c0 = 0; c0 < J.n_out; c0 += max_cols) {  // column chunks of an oversize job; one that no segment stores is dropped
            const int c1 = std::min(J.n_out, c0 + max_cols);
            bool stored = false;
            for (int sg = 0; sg < J.n_seg; ++sg) stored = stored || std::min(J.seg[sg].c1, c1) > std::max(J.seg[sg].c0, c0);
            if (stored) pieces.push_back({i, c0, c1, PEA_ROUTE_PERSIST, KH});
        }
    }
    out->reserve(pieces.size());   // no launch record is ever moved
    for (int family : {PEA_ROUTE_SKINNY, PEA_ROUTE_PERSIST, PEA_ROUTE_DEEP_STAGED})
        for (int KH : {16, 32, 64}) {
            GemmLaunch *L = nullptr;   // the open launch of this pass
            size_t lds = 0;
            for (const GemmPiece &P : pieces) {
                if (P.family != family || P.KH != KH) continue;
                const size_t need =   // the piece's B image in the persistent kernel's LDS
                    family != PEA_ROUTE_PERSIST ? 0 : (size_t)(2 * KH + 1) * ((P.c1 - P.c0 + 31) / 32 * 32) * sizeof(float);
                if (L && (L->Bt.n == kMaxBatch || lds + need > kLdsBudget)) {
                    close_launch(*L, family, KH, rows_given, n_rows, env);
                    L = nullptr;
                }
                if (!L) {
                    out->emplace_back();
                    L = &out->back();
                    L->Bt.n = 0;
                    lds = 0;
                }
                L->src[L->Bt.n] = P.src;
                place_piece(L->Bt.j[L->Bt.n++], jobs_in[P.src], P);
                lds += need;
            }
            if (L) close_launch(*L, family, KH, rows_given, n_rows, env);
        }
    return PEA_OK;
}

// tables: the PersistArgs / SkinnyArgs of the launch.  PEA_LAUNCH captures the batch and the tables by value (tape replay).
template <auto Kernel, class... Tables>
static int issue(const GemmLaunch &L, dim3 grid, int threads, int lds_limit, const int *rows, int64_t n_rows, hipStream_t stream,
                 const Tables &...tables) {
    PEA_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(Kernel), (size_t)lds_limit));
    const GemmBatch &Bt = L.Bt;
    const size_t lds = L.lds;
    ProfScope ps(L.name, stream, L.bytes);
    PEA_LAUNCH(Kernel, grid, dim3(threads), lds, stream, Bt, tables..., rows, n_rows);
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}

constexpr int route_key(int family, int variant, bool listed) { return family * 1000 + variant * 2 + (listed ? 1 : 0); }

static int issue_gemm(const GemmLaunch &L, const int *rows, int64_t n_rows, hipStream_t stream) {
    int n_cu = 0;
    if (L.per_cu) PEA_TRY(device_cu_count(&n_cu));
    const dim3 grid((unsigned)(L.per_cu ? std::min<int64_t>((int64_t)L.per_cu * n_cu, L.blocks) : L.blocks),
                    (unsigned)(L.family >= PEA_ROUTE_DEEP_RESIDENT ? L.Bt.n : 1));
    constexpr int kAll = (int)kLdsBudget;
    const int own = (int)L.lds;   // the 128-chunk kernels: 64 KiB (NCT = 2) and 128 KiB (NCT = 4); NCT = 1 fits the default limit
    // only the skinny and the persistent kernel have a variant for row lists
    switch (route_key(L.family, L.variant, L.listed && L.family <= PEA_ROUTE_PERSIST)) {
        case route_key(PEA_ROUTE_SKINNY, 2, true): return issue<gemm_skinny_kernel<2, true>>(L, grid, 512, kAll, rows, n_rows, stream, L.Sa);
        case route_key(PEA_ROUTE_SKINNY, 2, false): return issue<gemm_skinny_kernel<2, false>>(L, grid, 512, kAll, rows, n_rows, stream, L.Sa);
        case route_key(PEA_ROUTE_SKINNY, 4, true): return issue<gemm_skinny_kernel<4, true>>(L, grid, 512, kAll, rows, n_rows, stream, L.Sa);
        case route_key(PEA_ROUTE_SKINNY, 4, false): return issue<gemm_skinny_kernel<4, false>>(L, grid, 512, kAll, rows, n_rows, stream, L.Sa);
        case route_key(PEA_ROUTE_SKINNY, 8, true): return issue<gemm_skinny_kernel<8, true>>(L, grid, 512, kAll, rows, n_rows, stream, L.Sa);
        case route_key(PEA_ROUTE_SKINNY, 8, false): return issue<gemm_skinny_kernel<8, false>>(L, grid, 512, kAll, rows, n_rows, stream, L.Sa);
        case route_key(PEA_ROUTE_PERSIST, 16, true): return issue<gemm_persist_kernel<16, true>>(L, grid, 1024, kAll, rows, n_rows, stream, L.Pa);
        case route_key(PEA_ROUTE_PERSIST, 16, false): return issue<gemm_persist_kernel<16, false>>(L, grid, 1024, kAll, rows, n_rows, stream, L.Pa);
        case route_key(PEA_ROUTE_PERSIST, 32, true): return issue<gemm_persist_kernel<32, true>>(L, grid, 1024, kAll, rows, n_rows, stream, L.Pa);
        case route_key(PEA_ROUTE_PERSIST, 32, false): return issue<gemm_persist_kernel<32, false>>(L, grid, 1024, kAll, rows, n_rows, stream, L.Pa);
        case route_key(PEA_ROUTE_PERSIST, 64, true): return issue<gemm_persist_kernel<64, true>>(L, grid, 512, kAll, rows, n_rows, stream, L.Pa);
        case route_key(PEA_ROUTE_PERSIST, 64, false): return issue<gemm_persist_kernel<64, false>>(L, grid, 512, kAll, rows, n_rows, stream, L.Pa);
        case route_key(PEA_ROUTE_DEEP_RESIDENT, 1, false): return issue<gemm_deep_resident_kernel<1>>(L, grid, 1024, kAll, rows, n_rows, stream);
        case route_key(PEA_ROUTE_DEEP_RESIDENT, 2, false): return issue<gemm_deep_resident_kernel<2>>(L, grid, 1024, kAll, rows, n_rows, stream);
        case route_key(PEA_ROUTE_DEEP_CHUNK, 2, false): return issue<gemm_deep_kernel<2>>(L, grid, 256, own, rows, n_rows, stream);
        case route_key(PEA_ROUTE_DEEP_CHUNK, 4, false): return issue<gemm_deep_kernel<4>>(L, grid, 256, own, rows, n_rows, stream);
        case route_key(PEA_ROUTE_DEEP_CHUNK, 1, false): return issue<gemm_deep_kernel<1>>(L, grid, 256, 0, rows, n_rows, stream);
        case route_key(PEA_ROUTE_DEEP_STAGED, 64, false): return issue<gemm_mfma_kernel<64>>(L, grid, 256, 0, rows, n_rows, stream);
    }
    set_error("gemm: no kernel for route (%d, %d)", L.family, L.variant);
    return PEA_ERR_ARG;
}

int launch_gemm_batch(const GemmJob *jobs, int n_jobs, const int *rows, int64_t n_rows, hipStream_t stream) {
    std::vector<GemmLaunch> plan;
    PEA_TRY(plan_gemm_launches(jobs, n_jobs, rows != nullptr, n_rows, gemm_env(), &plan));
    for (const GemmLaunch &L : plan) PEA_TRY(issue_gemm(L, rows, n_rows, stream));
    return PEA_OK;
}

int launch_gemm(const GemmJob &job, const int *rows, int64_t n_rows, hipStream_t stream) {
    return launch_gemm_batch(&job, 1, rows, n_rows, stream);
}

int gemm_route(const GemmJob *jobs, int n_jobs, bool rows_given, int64_t n_rows, int cap, pea_dense_route_entry *entries, int *count) {
    std::vector<GemmLaunch> plan;
    PEA_TRY(plan_gemm_launches(jobs, n_jobs, rows_given, n_rows, gemm_env(), &plan));
    *count = (int)plan.size();
    for (int i = 0; i < *count && i < cap; ++i) {
        const GemmLaunch &L = plan[(size_t)i];
        pea_dense_route_entry &E = entries[i];
        snprintf(E.name, sizeof(E.name), "%s", L.name);
        E.family = L.family;
        E.variant = L.variant;
        E.listed = L.listed ? 1 : 0;
        E.col_group = L.family == PEA_ROUTE_PERSIST ? L.Pa.col_group : 0;
        E.lds_bytes = (int64_t)L.lds;
        E.n_jobs = L.Bt.n;
        for (int q = 0; q < L.Bt.n; ++q) {   // differences of addresses only: nothing is read through them
            const GemmJob &C = L.Bt.j[q], &J = jobs[L.src[q]];
            E.job[q] = L.src[q];
            E.col0[q] = (int)(C.B - J.B);
            E.n_out[q] = C.n_out;
            E.gate_col0[q] = C.seg[0].gate ? (int)(C.seg[0].gate - J.seg[0].gate) : -1;
        }
    }
    return PEA_OK;
}

int launch_pack(const PackJob *jobs, int n_jobs, hipStream_t stream) {
    for (int base = 0; base < n_jobs; base += kMaxPack) {
        PackLaunch L;
        L.n = n_jobs - base < kMaxPack ? n_jobs - base : kMaxPack;
        for (int i = 0; i < L.n; ++i) L.j[i] = jobs[base + i];
        ProfScope ps("pack_weights", stream);
        PEA_LAUNCH(pack_kernel, dim3(L.n), dim3(256), 0, stream, L);
        PEA_HIP(hipGetLastError());
    }
    return PEA_OK;
}

}  // namespace pea
