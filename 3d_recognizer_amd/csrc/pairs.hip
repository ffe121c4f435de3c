// Pair counts of two integer id arrays (utils/instance_metrics.py: pair_counts; InstanceEvaluator, Model.evaluate_instances):
// the sparse contingency table of a (M) against b (M) - every pair (a_i, b_i) that occurs, once, in ascending order of (a, b)
// with -1 first, and how many points carry it.  The numpy twin is pair_counts_host; everything here is integer work, so the
// result equals the twin's exactly and is a pure function of the input (no atomics outside the sort's LDS histograms, whose
// sums do not depend on the order of arrival).
//
//   rl_pairs_sort    keys         per chunk of consecutive positions: key = (a + 1) * (B + 1) + (b + 1) with a value below -1
//                                 read as -1; a value >= A (>= B) is out of range: its key is formed from -1 and the chunk's
//                                 slot of `bad` is raised (every chunk writes its slot: nothing has to be cleared first)
//                    per 8-bit digit of the key, lowest first, only the digits (A + 1) * (B + 1) - 1 needs (rl_radix.h):
//                      hist, scan, scatter
//                    head_count   per chunk the number of positions whose key differs from the one before (rl_cells.h)
//                    head_scan    one workgroup: exclusive prefix of those counts, P = their sum; the chunks' `bad` slots
//                                 folded into one flag; head_out = {P, flag}; start[P] = M
//   rl_pairs_write   head_write   runs numbered by wavefront ballots in position order; at a run's first position j:
//                                 start[run] = j, pa[run] = key / (B + 1) - 1, pb[run] = key % (B + 1) - 1
//                    counts       count[run] = start[run + 1] - start[run]: the distance to the next head
// No workgroup waits for another one: every scan over the whole array is split over launches.  The host reads back head_out
// once, between the two calls.
#include "rl_cells.h"

namespace {

struct PairsLayout {
    RadixLayout sort;
    size_t off_cnt, off_bad, off_start, bytes;
};

PairsLayout pairs_layout(long M) {
    PairsLayout L;
    RlCarve c;
    L.sort = radix_layout(c, M);
    L.off_cnt = c.take((size_t)L.sort.chunks * sizeof(uint32_t));
    L.off_bad = c.take((size_t)L.sort.chunks * sizeof(uint32_t));
    L.off_start = c.take((size_t)(M + 1) * sizeof(uint32_t));
    L.bytes = c.at;
    return L;
}

__device__ __forceinline__ int64_t pr_load(const void* __restrict__ p, int is64, long i) {
    return is64 ? ((const int64_t*)p)[i] : (int64_t)((const int32_t*)p)[i];
}

// one workgroup per chunk
__global__ __launch_bounds__(GR_THREADS) void pr_keys(const void* __restrict__ a, int a64, const void* __restrict__ b, int b64,
                                                       long M, int64_t A, int64_t B, long chunk,
                                                       uint64_t* __restrict__ keys, uint32_t* __restrict__ bad) {
    const long i0 = (long)blockIdx.x * chunk;
    const long i1 = min(M, i0 + chunk);
    int out = 0;
    for (long i = i0 + threadIdx.x; i < i1; i += GR_THREADS) {
        int64_t va = pr_load(a, a64, i), vb = pr_load(b, b64, i);
        if (va >= A) va = -1, out = 1;
        if (vb >= B) vb = -1, out = 1;
        va = va < -1 ? -1 : va;
        vb = vb < -1 ? -1 : vb;
        keys[i] = (uint64_t)((va + 1) * (B + 1) + (vb + 1));
    }
    out = __syncthreads_or(out);
    if (threadIdx.x == 0) bad[blockIdx.x] = out ? 1u : 0u;
}

// one workgroup: the heads before every chunk, P, and the flag of the keys
__global__ __launch_bounds__(GR_THREADS) void pr_head_scan(uint32_t* __restrict__ cnt, const uint32_t* __restrict__ bad,
                                                            int chunks, long M, int64_t* __restrict__ head_out,
                                                            uint32_t* __restrict__ start) {
    int out = 0;
    for (int j = threadIdx.x; j < chunks; j += GR_THREADS) out |= bad[j] != 0u;
    out = __syncthreads_or(out);
    const uint32_t P = block_exclusive_scan(cnt, chunks);
    if (threadIdx.x == 0) {
        head_out[0] = (int64_t)P;
        head_out[1] = out ? 1 : 0;
        start[P] = (uint32_t)M;          // P <= M: start holds M + 1 entries
    }
}

// one wavefront per chunk
__global__ __launch_bounds__(64) void pr_head_write(const uint64_t* __restrict__ keys, long M, long chunk, int64_t B, long P,
                                                     const uint32_t* __restrict__ cnt, uint32_t* __restrict__ start,
                                                     int32_t* __restrict__ pa, int32_t* __restrict__ pb) {
    const int lane = threadIdx.x;
    const unsigned long long upto = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull;
    const long i0 = (long)blockIdx.x * chunk;
    const long i1 = min(M, i0 + chunk);
    uint32_t run = cnt[blockIdx.x];       // heads before this chunk
    for (long t0 = i0; t0 < i1; t0 += 64) {
        const long j = t0 + lane;
        const bool head = j < i1 && is_head(keys, j);
        const unsigned long long m = __ballot(head);
        if (head) {
            const long seg = (long)run + __popcll(m & upto) - 1;
            if (seg < P) {                // (always: P counted these heads)
                const uint64_t k = keys[j];
                start[seg] = (uint32_t)j;
                pa[seg] = (int32_t)((int64_t)(k / (uint64_t)(B + 1)) - 1);
                pb[seg] = (int32_t)((int64_t)(k % (uint64_t)(B + 1)) - 1);
            }
        }
        run += (uint32_t)__popcll(m);
    }
}

__global__ __launch_bounds__(GR_THREADS) void pr_counts(const uint32_t* __restrict__ start, long P, long M,
                                                         int64_t* __restrict__ count) {
    const long s = (long)blockIdx.x * GR_THREADS + threadIdx.x;
    if (s >= P) return;
    count[s] = (int64_t)start[s + 1] - (int64_t)start[s];       // s + 1 <= P <= M: inside start
}

int pairs_check(const char* who, int64_t M, int64_t A, int64_t B, const void* ws, int64_t ws_bytes) {
    RL_REQUIRE(M > 0 && M < 0x7fffffffLL, RL_ERR_ARGS, "%s: M=%lld outside 1 .. 2^31-2", who, (long long)M);
    RL_REQUIRE(A >= 1 && A <= 0x7fffffffLL && B >= 1 && B <= 0x7fffffffLL, RL_ERR_ARGS, "%s: A=%lld, B=%lld outside 1 .. 2^31-1",
               who, (long long)A, (long long)B);
    return rl_ws_check(who, ws, ws_bytes, rl_pairs_workspace_bytes(M));
}

}  // namespace

extern "C" int64_t rl_pairs_workspace_bytes(int64_t M) {
    if (M <= 0 || M >= 0x7fffffffLL) return 0;
    return (int64_t)pairs_layout(M).bytes;
}

extern "C" int rl_pairs_sort(const void* a, int a_bytes, const void* b, int b_bytes, int64_t M, int64_t A, int64_t B,
                             int64_t* head_out, void* ws, int64_t ws_bytes, void* stream) {
    RL_REQUIRE((a_bytes == 4 || a_bytes == 8) && (b_bytes == 4 || b_bytes == 8), RL_ERR_ARGS,
               "rl_pairs_sort: ids of %d and %d bytes, int32 or int64 expected", a_bytes, b_bytes);
    int rc = pairs_check("rl_pairs_sort", M, A, B, ws, ws_bytes);
    if (rc) return rc;
    RL_REQUIRE(a && b && head_out, RL_ERR_ARGS, "rl_pairs_sort: null pointer");
    hipStream_t sm = (hipStream_t)stream;
    const PairsLayout L = pairs_layout(M);
    const RadixBufs sort = radix_bufs(ws, L.sort);
    uint32_t* cnt = rl_at<uint32_t>(ws, L.off_cnt);
    uint32_t* bad = rl_at<uint32_t>(ws, L.off_bad);
    const int passes = grid_passes(rl_bits_of((A + 1) * (B + 1) - 1));       // < 2^62: A, B < 2^31
    hipLaunchKernelGGL(pr_keys, dim3(sort.chunks), dim3(GR_THREADS), 0, sm, a, a_bytes == 8, b, b_bytes == 8, (long)M, A, B,
                       sort.chunk, sort.keys[passes & 1], bad);
    RL_LAUNCH_CHECK("rl_pairs_sort (keys)");
    rc = radix_sort("rl_pairs_sort", sort, (long)M, passes, sm);
    if (rc) return rc;
    hipLaunchKernelGGL(grid_head_count, dim3(sort.chunks), dim3(64), 0, sm, sort.keys[0], (long)M, sort.chunk, cnt);
    RL_LAUNCH_CHECK("rl_pairs_sort (head count)");
    hipLaunchKernelGGL(pr_head_scan, dim3(1), dim3(GR_THREADS), 0, sm, cnt, bad, sort.chunks, (long)M, head_out,
                       rl_at<uint32_t>(ws, L.off_start));
    rl_note_kernel("pr_head_scan");
    RL_LAUNCH_CHECK("rl_pairs_sort (head scan)");
    return RL_OK;
}

extern "C" int rl_pairs_write(int64_t M, int64_t A, int64_t B, int64_t P, int32_t* pa, int32_t* pb, int64_t* count, void* ws,
                              int64_t ws_bytes, void* stream) {
    int rc = pairs_check("rl_pairs_write", M, A, B, ws, ws_bytes);
    if (rc) return rc;
    RL_REQUIRE(P > 0 && P <= M, RL_ERR_ARGS, "rl_pairs_write: P=%lld pairs of M=%lld points", (long long)P, (long long)M);
    RL_REQUIRE(pa && pb && count, RL_ERR_ARGS, "rl_pairs_write: null pointer");
    hipStream_t sm = (hipStream_t)stream;
    const PairsLayout L = pairs_layout(M);
    uint32_t* start = rl_at<uint32_t>(ws, L.off_start);
    hipLaunchKernelGGL(pr_head_write, dim3(L.sort.chunks), dim3(64), 0, sm, rl_at<const uint64_t>(ws, L.sort.off_keys[0]), (long)M,
                       L.sort.chunk, B, (long)P, rl_at<const uint32_t>(ws, L.off_cnt), start, pa, pb);
    RL_LAUNCH_CHECK("rl_pairs_write (head write)");
    hipLaunchKernelGGL(pr_counts, dim3(rl_cdiv(P, GR_THREADS)), dim3(GR_THREADS), 0, sm, start, (long)P, (long)M, count);
    rl_note_kernel("pr_counts");
    RL_LAUNCH_CHECK("rl_pairs_write (counts)");
    return RL_OK;
}
