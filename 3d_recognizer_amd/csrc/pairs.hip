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
    long chunk;      // positions per chunk
    int chunks;
    size_t off_tot, off_cnt, off_bad, off_hist, off_keys0, off_keys1, off_idx0, off_idx1, off_start, bytes;
};

PairsLayout pairs_layout(long M) {
    PairsLayout L;
    grid_chunks(M, &L.chunk, &L.chunks);
    L.off_tot = 0;
    L.off_cnt = L.off_tot + al256(GR_BINS * sizeof(uint32_t));
    L.off_bad = L.off_cnt + al256((size_t)L.chunks * sizeof(uint32_t));
    L.off_hist = L.off_bad + al256((size_t)L.chunks * sizeof(uint32_t));
    L.off_keys0 = L.off_hist + al256((size_t)GR_BINS * L.chunks * sizeof(uint32_t));
    L.off_keys1 = L.off_keys0 + al256((size_t)M * sizeof(uint64_t));
    L.off_idx0 = L.off_keys1 + al256((size_t)M * sizeof(uint64_t));
    L.off_idx1 = L.off_idx0 + al256((size_t)M * sizeof(uint32_t));
    L.off_start = L.off_idx1 + al256((size_t)M * sizeof(uint32_t));
    L.bytes = L.off_start + al256((size_t)(M + 1) * sizeof(uint32_t));
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
    RL_REQUIRE(ws_bytes >= rl_pairs_workspace_bytes(M), RL_ERR_ARGS, "%s: workspace of %lld bytes, %lld needed", who,
               (long long)ws_bytes, (long long)rl_pairs_workspace_bytes(M));
    RL_REQUIRE(ws, RL_ERR_ARGS, "%s: null pointer", who);
    RL_REQUIRE(((uintptr_t)ws & 255) == 0, RL_ERR_ARGS, "%s: workspace not 256-byte aligned", who);
    return RL_OK;
}

int pairs_key_bits(int64_t A, int64_t B) {
    int64_t x = (A + 1) * (B + 1) - 1;       // < 2^62: A, B < 2^31
    int b = 0;
    while (x > 0) ++b, x >>= 1;
    return b < 1 ? 1 : b;
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
    char* base = (char*)ws;
    uint32_t* tot = (uint32_t*)(base + L.off_tot);
    uint32_t* cnt = (uint32_t*)(base + L.off_cnt);
    uint32_t* bad = (uint32_t*)(base + L.off_bad);
    uint32_t* hist = (uint32_t*)(base + L.off_hist);
    uint64_t* keys[2] = {(uint64_t*)(base + L.off_keys0), (uint64_t*)(base + L.off_keys1)};
    uint32_t* idx[2] = {(uint32_t*)(base + L.off_idx0), (uint32_t*)(base + L.off_idx1)};
    uint32_t* start = (uint32_t*)(base + L.off_start);
    const int passes = grid_passes(pairs_key_bits(A, B));
    hipLaunchKernelGGL(pr_keys, dim3(L.chunks), dim3(GR_THREADS), 0, sm, a, a_bytes == 8, b, b_bytes == 8, (long)M, A, B,
                       L.chunk, keys[passes & 1], bad);
    RL_LAUNCH_CHECK("rl_pairs_sort (keys)");
    rc = grid_radix_sort("rl_pairs_sort", keys, idx, (long)M, passes, L.chunk, L.chunks, hist, tot, sm);
    if (rc) return rc;
    hipLaunchKernelGGL(grid_head_count, dim3(L.chunks), dim3(64), 0, sm, keys[0], (long)M, L.chunk, cnt);
    RL_LAUNCH_CHECK("rl_pairs_sort (head count)");
    hipLaunchKernelGGL(pr_head_scan, dim3(1), dim3(GR_THREADS), 0, sm, cnt, bad, L.chunks, (long)M, head_out, start);
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
    char* base = (char*)ws;
    const uint32_t* cnt = (const uint32_t*)(base + L.off_cnt);
    const uint64_t* keys = (const uint64_t*)(base + L.off_keys0);
    uint32_t* start = (uint32_t*)(base + L.off_start);
    hipLaunchKernelGGL(pr_head_write, dim3(L.chunks), dim3(64), 0, sm, keys, (long)M, L.chunk, B, (long)P, cnt, start, pa, pb);
    RL_LAUNCH_CHECK("rl_pairs_write (head write)");
    hipLaunchKernelGGL(pr_counts, dim3(rl_cdiv(P, GR_THREADS)), dim3(GR_THREADS), 0, sm, start, (long)P, (long)M, count);
    rl_note_kernel("pr_counts");
    RL_LAUNCH_CHECK("rl_pairs_write (counts)");
    return RL_OK;
}
