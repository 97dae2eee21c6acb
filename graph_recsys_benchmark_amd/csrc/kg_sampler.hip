// Device-side KG triple sampler for gfx950 with the epoch shuffle inside the launch (include/peahip_sample.h).  An ADDITION
// to the bit-exact host path (utils/sampling.py: kg_negative_sampling restates reference datasets/movielens.py:861-877 id
// for id): the same rows (h, t+, t-, relation id), its own counter-based stream.  tests/kg_sampler_ref.py restates every
// line below in numpy over oracle/philox.py.
//   draw     w = philox((e lo, e hi, attempt | 1 << 8, offset)).x,  t- = lo_s + floor(w n_s / 2^32); (lo_s, n_s) of the
//            triple's segment: (0, num_nodes) is the reference's distribution, a node-type block the typed one.  With a key
//            table a draw equal to t+ or completing a known triple ((s N + h) N + t-) is redrawn, up to 64 attempts.
//   shuffle  store row e goes to output row perm(e): a 4-round Feistel network over [0, 2^(2 hb)) whose round function is
//            philox((R, round, 2 << 8, offset)).x & (2^hb - 1), walked until it lands below n (a bijection of [0, n)).
// The third counter word carries a tag from bit 8 up: the BPR sampler (sampler.hip) draws with tag 0, so one seed serves both.
// The store is read in order and each 32-byte row stored at perm(e) (the scatter form; the gather form, which inverts perm
// per output row and stores in order, measured no faster and was not kept: DESIGN.md section 20).  Integers only; no scratch.
#include "common.h"
#include "philox.h"
#include "sample_common.h"
#include "../../include/peahip_sample.h"

namespace pea {
namespace {

constexpr int kBlock = 256;
// thread e: store row e, written at output row perm(e) (shuffle) or e
__global__ __launch_bounds__(kBlock) void kg_sample_kernel(long long n, const long long *__restrict__ heads,
                                                           const long long *__restrict__ tails, int n_seg,
                                                           const long long *__restrict__ seg_ptr, const long long *__restrict__ seg_rel,
                                                           const long long *__restrict__ seg_lo, const long long *__restrict__ seg_n,
                                                           long long num_nodes, const long long *__restrict__ keys, long long n_keys,
                                                           Stream st, int shuffle, int hb, long long *__restrict__ out,
                                                           long long ld_out, int *__restrict__ exhausted) {
    __shared__ long long s_ptr[PEA_KG_MAX_SEGMENTS + 1], s_rel[PEA_KG_MAX_SEGMENTS], s_lo[PEA_KG_MAX_SEGMENTS];
    __shared__ unsigned s_n[PEA_KG_MAX_SEGMENTS];
    __shared__ int s_fail[kBlock / kWave];
    for (int k = threadIdx.x; k < n_seg; k += kBlock) {
        s_ptr[k] = seg_ptr[k];
        s_rel[k] = seg_rel[k];
        s_lo[k] = seg_lo[k];
        s_n[k] = (unsigned)seg_n[k];
    }
    if (threadIdx.x == 0) s_ptr[n_seg] = seg_ptr[n_seg];
    __syncthreads();
    const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
    bool failed = false;
    if (e < n) {
        const long long dst = shuffle ? (long long)perm_of((unsigned long long)e, (unsigned long long)n, hb, st) : e;
        // the last segment that starts at or before e: an empty segment shares its start with the next one and is passed over
        int lo = 0, hi = n_seg - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (s_ptr[mid] <= e) lo = mid;
            else hi = mid - 1;
        }
        const int s = lo;
        const long long h = heads[e], t = tails[e];
        const long long base = s_lo[s];
        const unsigned long long span = s_n[s];
        // below 2^63 whenever a key table is given (checked on the host); unsigned, so that it wraps quietly when none is
        const long long key0 = (long long)(((unsigned long long)s * (unsigned long long)num_nodes + (unsigned long long)h) *
                                           (unsigned long long)num_nodes);
        long long neg = base;
        bool ok = false;
        for (int attempt = 0; attempt < kMaxAttempts && !ok; ++attempt) {
            const U4 w = philox4x32_10(U4{(unsigned)e, (unsigned)((unsigned long long)e >> 32), (unsigned)attempt | kTagDraw, st.offset},
                                       st.k0, st.k1);
            neg = base + (long long)(((unsigned long long)w.x * span) >> 32);
            ok = n_keys == 0 || (neg != t && !contains(keys, n_keys, key0 + neg));
        }
        failed = !ok;
        long long *o = out + dst * ld_out;
        o[0] = h;
        o[1] = t;
        o[2] = neg;
        o[3] = s_rel[s];
    }
    // rows whose attempts ran out: one ballot per wave, one atomic per workgroup
    const unsigned long long votes = __ballot(failed);
    if ((threadIdx.x & (kWave - 1)) == 0) s_fail[threadIdx.x / kWave] = __popcll(votes);
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < kBlock / kWave; ++w) total += s_fail[w];
        if (total) atomicAdd(exhausted, total);
    }
}

// out[perm(i)] = in[i], rows of `width` words
__global__ __launch_bounds__(kBlock) void permute_rows_kernel(long long n, int width, const long long *__restrict__ in,
                                                              long long ld_in, long long *__restrict__ out, long long ld_out,
                                                              Stream st, int hb) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const long long dst = (long long)perm_of((unsigned long long)i, (unsigned long long)n, hb, st);
    const long long *src = in + i * ld_in;
    long long *o = out + dst * ld_out;
    for (int c = 0; c < width; ++c) o[c] = src[c];
}

}  // namespace
}  // namespace pea

using namespace pea;

extern "C" int pea_kg_sample(int64_t n_triples, const int64_t *heads, const int64_t *tails, int n_seg, const int64_t *seg_ptr,
                             const int64_t *seg_rel, const int64_t *seg_lo, const int64_t *seg_n, int64_t num_nodes,
                             const int64_t *keys_sorted, int64_t n_keys, uint64_t seed, uint32_t offset, int shuffle,
                             int64_t *out, int64_t ld_out, int *exhausted, void *stream) {
    PEA_REQUIRE(n_triples >= 0 && ld_out >= 4, PEA_ERR_ARG, "kg_sample: bad sizes (n_triples %lld, ld_out %lld)",
                (long long)n_triples, (long long)ld_out);
    PEA_REQUIRE(n_seg >= 1 && n_seg <= PEA_KG_MAX_SEGMENTS, PEA_ERR_ARG, "kg_sample: %d segments (1..%d)", n_seg, PEA_KG_MAX_SEGMENTS);
    PEA_REQUIRE(num_nodes >= 1 && num_nodes < (1ll << 32), PEA_ERR_ARG, "kg_sample: num_nodes %lld outside [1, 2^32)",
                (long long)num_nodes);
    PEA_REQUIRE(shuffle == 0 || shuffle == 1, PEA_ERR_ARG, "kg_sample: shuffle %d (0 or 1)", shuffle);
    PEA_REQUIRE(n_keys >= 0 && (keys_sorted || n_keys == 0), PEA_ERR_ARG, "kg_sample: key table missing");
    // ((s N + h) N + t) < n_seg N^2 must fit an int64
    PEA_REQUIRE(n_keys == 0 || (unsigned __int128)n_seg * (unsigned __int128)num_nodes * (unsigned __int128)num_nodes <
                                   ((unsigned __int128)1 << 63),
                PEA_ERR_ARG, "kg_sample: %d segments of %lld nodes overflow the 63-bit triple key", n_seg, (long long)num_nodes);
    PEA_REQUIRE((heads && tails && seg_ptr && seg_rel && seg_lo && seg_n && out && exhausted) || n_triples == 0, PEA_ERR_ARG,
                "kg_sample: null argument");
    if (n_triples == 0) return PEA_OK;
    hipStream_t st = (hipStream_t)stream;
    const Stream rs{(unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), (unsigned)offset};
    const int hb = half_bits(n_triples);
    const dim3 grid((unsigned)((n_triples + kBlock - 1) / kBlock));
    PEA_REQUIRE((n_triples + kBlock - 1) / kBlock < (1ll << 31), PEA_ERR_ARG, "kg_sample: %lld triples exceed the grid",
                (long long)n_triples);
    PEA_MEMSET_ASYNC(exhausted, 0, sizeof(int), st);
    ProfScope ps("kg_sample", st, 48.0 * (double)n_triples);
    const long long *h = reinterpret_cast<const long long *>(heads), *t = reinterpret_cast<const long long *>(tails);
    const long long *sp = reinterpret_cast<const long long *>(seg_ptr), *sr = reinterpret_cast<const long long *>(seg_rel);
    const long long *sl = reinterpret_cast<const long long *>(seg_lo), *sn = reinterpret_cast<const long long *>(seg_n);
    const long long *keys = reinterpret_cast<const long long *>(keys_sorted);
    long long *o = reinterpret_cast<long long *>(out);
    PEA_LAUNCH(kg_sample_kernel, grid, dim3(kBlock), 0, st, (long long)n_triples, h, t, n_seg, sp, sr, sl, sn, (long long)num_nodes,
               keys, (long long)n_keys, rs, shuffle, hb, o, (long long)ld_out, exhausted);
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}

extern "C" int pea_permute_rows(int64_t n, int width, const int64_t *in, int64_t ld_in, int64_t *out, int64_t ld_out,
                                uint64_t seed, uint32_t offset, void *stream) {
    PEA_REQUIRE(n >= 0 && width >= 1 && width <= PEA_PERMUTE_MAX_WIDTH, PEA_ERR_ARG, "permute_rows: bad sizes (n %lld, width %d)",
                (long long)n, width);
    PEA_REQUIRE(ld_in >= width && ld_out >= width, PEA_ERR_ARG, "permute_rows: row strides %lld, %lld below the width %d",
                (long long)ld_in, (long long)ld_out, width);
    PEA_REQUIRE((in && out) || n == 0, PEA_ERR_ARG, "permute_rows: null argument");
    if (n == 0) return PEA_OK;
    PEA_REQUIRE((n + kBlock - 1) / kBlock < (1ll << 31), PEA_ERR_ARG, "permute_rows: %lld rows exceed the grid", (long long)n);
    // in and out must not overlap: every row is read and written once, in no order
    const uintptr_t in0 = reinterpret_cast<uintptr_t>(in), out0 = reinterpret_cast<uintptr_t>(out);
    const uintptr_t in1 = in0 + (uintptr_t)((n - 1) * ld_in + width) * 8, out1 = out0 + (uintptr_t)((n - 1) * ld_out + width) * 8;
    PEA_REQUIRE(in1 <= out0 || out1 <= in0, PEA_ERR_ARG, "permute_rows: in and out overlap");
    hipStream_t st = (hipStream_t)stream;
    const Stream rs{(unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), (unsigned)offset};
    ProfScope ps("permute_rows", st, 16.0 * (double)n * width);
    PEA_LAUNCH(permute_rows_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, (long long)n, width,
               reinterpret_cast<const long long *>(in), (long long)ld_in, reinterpret_cast<long long *>(out), (long long)ld_out, rs,
               half_bits(n));
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}
