// Device-side CF epoch sampler for gfx950 (include/peahip_cf_sample.h): the whole training table of an epoch from one launch,
// one thread per output row.  An ADDITION to the bit-exact host path (utils/sampling.py: cf_negative_sampling and
// entity_aware_row restate reference datasets/movielens.py:879-997 and :1147-1181 id for id): the same rows, its own
// counter-based streams.  tests/cf_sampler_ref.py restates every line below in numpy over oracle/philox.py.
//   BPR      (u, i+, i-), row r from positive r / k; the negative is the draw of sampler.hip, word for word (tag 0, counter r)
//   BPR + e  the same row and the six entity columns entity.hip reads: ONE Philox call per row under tag 3 gives the four
//            words that pick e+ from the item's list, e- from e+'s node-type block, f+ and f- the same for the user
//   BCE      n_pos rows (u, i+, 1), then n_pos k rows (u, i-, 0); negative j draws with counter j
//   shuffle  row r goes to output row perm(r), the bijection of sample_common.h
// The node-type blocks are staged in LDS once per workgroup.  Loads are addressed by checked ids only: a row whose u or i+ lies
// outside its block, or whose CSR range is not inside its list, draws nothing and is counted in *bad_rows.  Integers only; no
// scratch; one integer add per workgroup into each of the two counters.
#include "common.h"
#include "philox.h"
#include "sample_common.h"
#include "../../include/peahip_cf_sample.h"

namespace pea {
namespace {

constexpr int kBlock = 256;

struct CfArgs {
    long long n_pos, n_rows;
    int k, mode, n_blocks, shuffle, hb;
    const long long *pos_u, *pos_i;
    long long item_lo, num_items, user_lo, num_users;
    const long long *keys;
    long long n_keys;
    const long long *item_ptr, *item_ent, *user_ptr, *user_ent;   // all null: three columns
    long long nnz_i, nnz_u;
    const long long *block_lo, *block_n;
    Stream st;
    long long *out;
    long long ld_out;
    int *exhausted, *bad_rows;
};

// the list [a, b) of `id` in a CSR over `n` owners and `nnz` entries; false when it does not lie inside the entries
__device__ __forceinline__ bool list_of(const long long *__restrict__ ptr, long long id, long long nnz, long long &a, long long &b) {
    a = ptr[id];
    b = ptr[id + 1];
    return a >= 0 && a <= b && b <= nnz;
}

// (e+, e-, mask) of one list from two words: e+ a member of the list, e- uniform over the block of e+
__device__ __forceinline__ void entity_pair(const long long *__restrict__ ent, long long a, long long b, unsigned w_pos, unsigned w_neg,
                                            int n_blocks, const long long *s_lo, const unsigned *s_n, long long *o) {
    const unsigned long long len = (unsigned long long)(b - a);
    if (len == 0) {
        o[0] = o[1] = o[2] = 0;
        return;
    }
    const long long e = ent[a + (long long)(((unsigned long long)w_pos * len) >> 32)];
    int lo = 0, hi = n_blocks - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (s_lo[mid] <= e) lo = mid;
        else hi = mid - 1;
    }
    o[0] = e;
    o[1] = s_lo[lo] + (long long)(((unsigned long long)w_neg * (unsigned long long)s_n[lo]) >> 32);
    o[2] = 1;
}

// one workgroup's count into a counter: one ballot per wave, one atomic per workgroup
__device__ __forceinline__ void count_into(int *counter, bool flag, int *s_cnt) {
    const unsigned long long votes = __ballot(flag);
    if ((threadIdx.x & (kWave - 1)) == 0) s_cnt[threadIdx.x / kWave] = __popcll(votes);
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < kBlock / kWave; ++w) total += s_cnt[w];
        if (total) atomicAdd(counter, total);
    }
}

// thread r: row r, written at output row perm(r) (shuffle) or r
__global__ __launch_bounds__(kBlock) void cf_sample_kernel(CfArgs p) {
    __shared__ long long s_lo[PEA_CF_MAX_BLOCKS];
    __shared__ unsigned s_n[PEA_CF_MAX_BLOCKS];
    __shared__ int s_fail[kBlock / kWave], s_bad[kBlock / kWave];
    const bool ent = p.item_ptr != nullptr;
    if (ent) {
        for (int b = threadIdx.x; b < p.n_blocks; b += kBlock) {
            s_lo[b] = p.block_lo[b];
            s_n[b] = (unsigned)p.block_n[b];
        }
        __syncthreads();
    }
    const long long r = (long long)blockIdx.x * kBlock + threadIdx.x;
    bool failed = false, bad = false;
    if (r < p.n_rows) {
        const bool positive = p.mode == PEA_CF_BCE && r < p.n_pos;       // a (u, i+, 1) row: no draw
        const bool carries_item = p.mode == PEA_CF_BPR || positive;
        const long long j = p.mode == PEA_CF_BCE ? r - p.n_pos : r;      // the negative's number
        const long long src = positive ? r : j / p.k;
        const long long u = p.pos_u[src];
        const long long ip = carries_item ? p.pos_i[src] : p.item_lo;
        const long long uo = u - p.user_lo, io = ip - p.item_lo;
        bad = uo < 0 || uo >= p.num_users || io < 0 || io >= p.num_items;
        long long ia = 0, ib = 0, ua = 0, ub = 0;
        if (ent && !bad) bad = !list_of(p.item_ptr, io, p.nnz_i, ia, ib) || !list_of(p.user_ptr, uo, p.nnz_u, ua, ub);
        long long neg = p.item_lo;
        if (!positive && !bad) {
            bool ok = false;
            for (int attempt = 0; attempt < kMaxAttempts && !ok; ++attempt) {
                const U4 w = philox4x32_10(U4{(unsigned)j, (unsigned)((unsigned long long)j >> 32), (unsigned)attempt, p.st.offset},
                                           p.st.k0, p.st.k1);
                const long long d = (long long)(((unsigned long long)w.x * (unsigned long long)p.num_items) >> 32);
                neg = p.item_lo + d;
                ok = p.keys == nullptr || !contains(p.keys, p.n_keys, u * p.num_items + d);
            }
            failed = !ok;
        }
        const long long dst = p.shuffle ? (long long)perm_of((unsigned long long)r, (unsigned long long)p.n_rows, p.hb, p.st) : r;
        long long *o = p.out + dst * p.ld_out;
        if (p.mode == PEA_CF_BCE) {
            o[0] = u;
            o[1] = positive ? ip : neg;
            o[2] = positive ? 1 : 0;
        } else {
            o[0] = u;
            o[1] = ip;
            o[2] = neg;
            if (ent) {
                long long e[6] = {0, 0, 0, 0, 0, 0};
                if (!bad) {
                    const U4 w = philox4x32_10(U4{(unsigned)r, (unsigned)((unsigned long long)r >> 32), kTagEntity, p.st.offset},
                                               p.st.k0, p.st.k1);
                    entity_pair(p.item_ent, ia, ib, w.x, w.y, p.n_blocks, s_lo, s_n, e);
                    entity_pair(p.user_ent, ua, ub, w.z, w.w, p.n_blocks, s_lo, s_n, e + 3);
                }
#pragma unroll
                for (int c = 0; c < 6; ++c) o[3 + c] = e[c];
            }
        }
    }
    count_into(p.exhausted, failed, s_fail);
    count_into(p.bad_rows, bad, s_bad);
}

}  // namespace
}  // namespace pea

using namespace pea;

extern "C" int pea_cf_sample(int64_t n_pos, int k, int mode, const int64_t *pos_u, const int64_t *pos_i, int64_t item_lo,
                             int64_t num_items, int64_t user_lo, int64_t num_users, const int64_t *keys_sorted, int64_t n_keys,
                             const int64_t *item_ent_ptr, const int64_t *item_ent, int64_t nnz_i, const int64_t *user_ent_ptr,
                             const int64_t *user_ent, int64_t nnz_u, int n_blocks, const int64_t *block_lo, const int64_t *block_n,
                             uint64_t seed, uint32_t offset, int shuffle, int64_t *out, int64_t ld_out, int *exhausted,
                             int *bad_rows, void *stream) {
    PEA_REQUIRE(n_pos >= 0 && k >= 1, PEA_ERR_ARG, "cf_sample: bad sizes (n_pos %lld, k %d)", (long long)n_pos, k);
    PEA_REQUIRE(mode == PEA_CF_BPR || mode == PEA_CF_BCE, PEA_ERR_ARG, "cf_sample: mode %d (0 = BPR, 1 = BCE)", mode);
    PEA_REQUIRE(shuffle == 0 || shuffle == 1, PEA_ERR_ARG, "cf_sample: shuffle %d (0 or 1)", shuffle);
    PEA_REQUIRE(num_items >= 1 && num_items < (1ll << 32) && num_users >= 1 && num_users < (1ll << 32), PEA_ERR_ARG,
                "cf_sample: num_items %lld or num_users %lld outside [1, 2^32)", (long long)num_items, (long long)num_users);
    PEA_REQUIRE(item_lo >= 0 && user_lo >= 0, PEA_ERR_ARG, "cf_sample: item_lo %lld or user_lo %lld below 0", (long long)item_lo,
                (long long)user_lo);
    PEA_REQUIRE(n_keys >= 0 && (keys_sorted || n_keys == 0), PEA_ERR_ARG, "cf_sample: key table missing");
    // u * num_items + item offset < (user_lo + num_users) * num_items must fit an int64
    PEA_REQUIRE(!keys_sorted || ((unsigned __int128)user_lo + (unsigned __int128)num_users) * (unsigned __int128)num_items <
                                    ((unsigned __int128)1 << 63),
                PEA_ERR_ARG, "cf_sample: users up to %lld times %lld items overflow the 63-bit pair key",
                (long long)user_lo + (long long)num_users, (long long)num_items);
    const int n_ent = (item_ent_ptr != nullptr) + (item_ent != nullptr) + (user_ent_ptr != nullptr) + (user_ent != nullptr);
    PEA_REQUIRE(n_ent == 0 || n_ent == 4, PEA_ERR_ARG, "cf_sample: %d of the four entity tables given (all or none)", n_ent);
    const bool ent = n_ent == 4;
    PEA_REQUIRE(!(ent && mode == PEA_CF_BCE), PEA_ERR_ARG, "cf_sample: entity tables with the BCE rows (BPR only)");
    if (ent) {
        PEA_REQUIRE(n_blocks >= 1 && n_blocks <= PEA_CF_MAX_BLOCKS, PEA_ERR_ARG, "cf_sample: %d node-type blocks (1..%d)", n_blocks,
                    PEA_CF_MAX_BLOCKS);
        PEA_REQUIRE(block_lo && block_n, PEA_ERR_ARG, "cf_sample: entity tables without the node-type blocks");
        PEA_REQUIRE(nnz_i >= 0 && nnz_i < (1ll << 32) && nnz_u >= 0 && nnz_u < (1ll << 32), PEA_ERR_ARG,
                    "cf_sample: nnz_i %lld or nnz_u %lld outside [0, 2^32)", (long long)nnz_i, (long long)nnz_u);
    }
    const int width = ent ? 9 : 3;
    PEA_REQUIRE(ld_out >= width, PEA_ERR_ARG, "cf_sample: ld_out %lld below the row width %d", (long long)ld_out, width);
    PEA_REQUIRE((pos_u && pos_i && out && exhausted && bad_rows) || n_pos == 0, PEA_ERR_ARG, "cf_sample: null argument");
    if (n_pos == 0) return PEA_OK;
    const unsigned __int128 total = (unsigned __int128)n_pos * (unsigned __int128)(mode == PEA_CF_BCE ? (long long)k + 1 : (long long)k);
    PEA_REQUIRE(total + (kBlock - 1) < ((unsigned __int128)kBlock << 31), PEA_ERR_ARG, "cf_sample: %lld positives times %d exceed the grid",
                (long long)n_pos, k);
    hipStream_t st = (hipStream_t)stream;
    CfArgs a;
    a.n_pos = n_pos;
    a.n_rows = (long long)total;
    a.k = k;
    a.mode = mode;
    a.n_blocks = ent ? n_blocks : 0;
    a.shuffle = shuffle;
    a.hb = half_bits(a.n_rows);
    a.pos_u = reinterpret_cast<const long long *>(pos_u);
    a.pos_i = reinterpret_cast<const long long *>(pos_i);
    a.item_lo = item_lo;
    a.num_items = num_items;
    a.user_lo = user_lo;
    a.num_users = num_users;
    a.keys = reinterpret_cast<const long long *>(keys_sorted);
    a.n_keys = n_keys;
    a.item_ptr = reinterpret_cast<const long long *>(item_ent_ptr);
    a.item_ent = reinterpret_cast<const long long *>(item_ent);
    a.user_ptr = reinterpret_cast<const long long *>(user_ent_ptr);
    a.user_ent = reinterpret_cast<const long long *>(user_ent);
    a.nnz_i = ent ? nnz_i : 0;
    a.nnz_u = ent ? nnz_u : 0;
    a.block_lo = reinterpret_cast<const long long *>(block_lo);
    a.block_n = reinterpret_cast<const long long *>(block_n);
    a.st = Stream{(unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), (unsigned)offset};
    a.out = reinterpret_cast<long long *>(out);
    a.ld_out = ld_out;
    a.exhausted = exhausted;
    a.bad_rows = bad_rows;
    PEA_MEMSET_ASYNC(exhausted, 0, sizeof(int), st);
    PEA_MEMSET_ASYNC(bad_rows, 0, sizeof(int), st);
    ProfScope ps("cf_sample", st, (8.0 * width + 16.0) * (double)a.n_rows);
    PEA_LAUNCH(cf_sample_kernel, dim3((unsigned)((a.n_rows + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a);
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}
