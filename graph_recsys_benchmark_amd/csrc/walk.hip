// Random walks of metapath2vec on the device (reference models/metapath2vec.py:101-140, where the positive walks are drawn on
// the CPU, one torch_sparse adj.sample per step, and the negative ones with one torch.randint per step).
//   pea_metapath_walks: walks over the plan's destination-sorted CSR, one relation per step, the relations cycling
//   pea_uniform_walks:  the "negative walks": every step uniform over the node-id block of the step's target type
// One walk per thread: the steps of a walk depend on one another, the parallelism is across walks.  Stream: Philox4x32-10,
// key = seed, counter = (walk row lo, hi, step t, offset); the first output word w picks slot floor(w * deg / 2^32).
// tests/walk_ref.py restates both in numpy on top of oracle/philox.py.
#include "common.h"
#include "philox.h"

namespace pea {
namespace {

constexpr int kMaxCycle = 16;

struct WalkCycle {     // by value in the kernel arguments
    const int *rowptr[kMaxCycle];
    const int *col[kMaxCycle];
    int len;
};

struct BlockCycle {
    long long lo[kMaxCycle];
    unsigned n[kMaxCycle];
    int len;
};

__device__ __forceinline__ unsigned draw(long long row, int t, unsigned offset, unsigned seed_lo, unsigned seed_hi) {
    return philox4x32_10(U4{(unsigned)row, (unsigned)((unsigned long long)row >> 32), (unsigned)t, offset}, seed_lo, seed_hi).x;
}

__global__ __launch_bounds__(256) void metapath_walk_kernel(long long n_walks, int L, long long num_nodes, const WalkCycle cyc,
                                                            const long long *__restrict__ starts, unsigned seed_lo,
                                                            unsigned seed_hi, unsigned offset, long long *__restrict__ walks,
                                                            long long ld, int *__restrict__ status) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_walks) return;
    long long *out = walks + r * ld;
    long long cur = starts[r];
    if (cur < 0 || cur >= num_nodes) {
        for (int t = 0; t <= L; ++t) out[t] = -1;
        atomicAdd(status + 1, 1);
        return;
    }
    out[0] = cur;
    int step = 0;                                          // (t - 1) % cycle length
    for (int t = 1; t <= L; ++t) {
        const int *rowptr = cyc.rowptr[step];
        const int beg = rowptr[cur];
        const unsigned deg = (unsigned)(rowptr[cur + 1] - beg);
        if (deg == 0) {                                    // dead end: this column and every later one
            for (int q = t; q <= L; ++q) out[q] = -1;
            atomicAdd(status, 1);
            return;
        }
        const unsigned w = draw(r, t, offset, seed_lo, seed_hi);
        cur = cyc.col[step][beg + (int)(((unsigned long long)w * deg) >> 32)];
        out[t] = cur;
        step = step + 1 == cyc.len ? 0 : step + 1;
    }
}

__global__ __launch_bounds__(256) void uniform_walk_kernel(long long n_walks, int L, const BlockCycle cyc,
                                                           const long long *__restrict__ starts, unsigned seed_lo,
                                                           unsigned seed_hi, unsigned offset, long long *__restrict__ walks,
                                                           long long ld) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_walks) return;
    long long *out = walks + r * ld;
    out[0] = starts[r];
    int step = 0;
    for (int t = 1; t <= L; ++t) {
        const unsigned w = draw(r, t, offset, seed_lo, seed_hi);
        out[t] = cyc.lo[step] + (long long)(((unsigned long long)w * cyc.n[step]) >> 32);
        step = step + 1 == cyc.len ? 0 : step + 1;
    }
}

}  // namespace
}  // namespace pea

using namespace pea;

extern "C" int pea_metapath_walks(const pea_plan *plan, int cycle_len, const int *relation_of_step_host, int walk_length,
                                  int64_t n_walks, const int64_t *starts, uint64_t seed, uint32_t offset, int64_t *walks,
                                  int64_t ld, int32_t *status, void *stream) {
    PEA_REQUIRE(plan && relation_of_step_host && cycle_len > 0 && cycle_len <= kMaxCycle, PEA_ERR_ARG,
                "metapath_walks: a plan and a cycle of 1..%d relations expected (got %d)", kMaxCycle, cycle_len);
    PEA_REQUIRE(!(plan->flags & PEA_PLAN_SELF_LOOPS), PEA_ERR_ARG,
                "metapath_walks: the plan was built with PEA_PLAN_SELF_LOOPS (its CSR has the i -> i edges removed)");
    PEA_REQUIRE(plan->shard_world == 1, PEA_ERR_ARG, "metapath_walks: the plan is sharded");
    PEA_REQUIRE(walk_length >= 0 && n_walks >= 0 && ld >= (int64_t)walk_length + 1, PEA_ERR_ARG,
                "metapath_walks: bad sizes (walk_length %d, n_walks %lld, ld %lld)", walk_length, (long long)n_walks, (long long)ld);
    PEA_REQUIRE(status && ((starts && walks) || n_walks == 0), PEA_ERR_ARG, "metapath_walks: null argument");
    WalkCycle cyc;
    cyc.len = cycle_len;
    for (int s = 0; s < cycle_len; ++s) {
        const int rel = relation_of_step_host[s];
        PEA_REQUIRE(rel >= 0 && rel < (int)plan->rels.size(), PEA_ERR_ARG, "metapath_walks: relation %d of step %d is not in the plan (%d relations)",
                    rel, s, (int)plan->rels.size());
        cyc.rowptr[s] = plan->rels[(size_t)rel].rowptr;
        cyc.col[s] = plan->rels[(size_t)rel].col;
    }
    hipStream_t st = (hipStream_t)stream;
    PEA_MEMSET_ASYNC(status, 0, 2 * sizeof(int), st);
    if (n_walks == 0) return PEA_OK;
    ProfScope ps("metapath_walks", st, (double)n_walks * (walk_length + 1) * 8.0);
    PEA_LAUNCH(metapath_walk_kernel, dim3((unsigned)((n_walks + 255) / 256)), dim3(256), 0, st, (long long)n_walks, walk_length,
               (long long)plan->N, cyc, reinterpret_cast<const long long *>(starts), (unsigned)(seed & 0xffffffffu),
               (unsigned)(seed >> 32), (unsigned)offset, reinterpret_cast<long long *>(walks), (long long)ld, status);
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}

extern "C" int pea_uniform_walks(int cycle_len, const int64_t *block_lo_host, const int64_t *block_n_host, int walk_length,
                                 int64_t n_walks, const int64_t *starts, uint64_t seed, uint32_t offset, int64_t *walks,
                                 int64_t ld, void *stream) {
    PEA_REQUIRE(block_lo_host && block_n_host && cycle_len > 0 && cycle_len <= kMaxCycle, PEA_ERR_ARG,
                "uniform_walks: a cycle of 1..%d node blocks expected (got %d)", kMaxCycle, cycle_len);
    PEA_REQUIRE(walk_length >= 0 && n_walks >= 0 && ld >= (int64_t)walk_length + 1, PEA_ERR_ARG,
                "uniform_walks: bad sizes (walk_length %d, n_walks %lld, ld %lld)", walk_length, (long long)n_walks, (long long)ld);
    PEA_REQUIRE((starts && walks) || n_walks == 0, PEA_ERR_ARG, "uniform_walks: null argument");
    BlockCycle cyc;
    cyc.len = cycle_len;
    for (int s = 0; s < cycle_len; ++s) {
        PEA_REQUIRE(block_n_host[s] > 0 && block_n_host[s] < ((int64_t)1 << 32), PEA_ERR_ARG,
                    "uniform_walks: block %d holds %lld nodes (0 < n < 2^32)", s, (long long)block_n_host[s]);
        cyc.lo[s] = block_lo_host[s];
        cyc.n[s] = (unsigned)block_n_host[s];
    }
    if (n_walks == 0) return PEA_OK;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps("uniform_walks", st, (double)n_walks * (walk_length + 1) * 8.0);
    PEA_LAUNCH(uniform_walk_kernel, dim3((unsigned)((n_walks + 255) / 256)), dim3(256), 0, st, (long long)n_walks, walk_length, cyc,
               reinterpret_cast<const long long *>(starts), (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32),
               (unsigned)offset, reinterpret_cast<long long *>(walks), (long long)ld);
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}
