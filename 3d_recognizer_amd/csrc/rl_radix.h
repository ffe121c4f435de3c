// The stable LSD radix sort of (64-bit key, 32-bit payload) pairs behind every sort-and-segment feature - grid.hip, cluster.hip,
// pairs.hip, boxes.hip and lovasz.hip: per 8-bit digit of the key, lowest first, three launches - hist, scan, scatter (see
// grid.hip's header comment).  Equal digits keep their order, so equal keys stay in ascending initial position; integer work
// only, and no workgroup waits for another one.  Below the kernels: where the sort's buffers lie in a client's workspace
// (radix_layout), their typed pointers (radix_bufs) and the host loop over the digits (radix_sort).
#pragma once
#include "rl_common.h"

namespace {

constexpr int GR_THREADS = 256;
constexpr int GR_BINS = 256;             // 8-bit digits
constexpr long GR_MIN_CHUNK = 2048;      // positions per chunk (a multiple of 64), at most GR_MAX_CHUNKS chunks
constexpr long GR_MAX_CHUNKS = 8192;

__global__ __launch_bounds__(GR_THREADS) void grid_hist(const uint64_t* __restrict__ keys, long M, int shift, long chunk,
                                                         int chunks, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[GR_BINS];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const long i0 = (long)blockIdx.x * chunk;
    const long i1 = min(M, i0 + chunk);
    for (long i = i0 + threadIdx.x; i < i1; i += GR_THREADS) atomicAdd(&h[(keys[i] >> shift) & (GR_BINS - 1)], 1u);
    __syncthreads();
    hist[(long)threadIdx.x * chunks + blockIdx.x] = h[threadIdx.x];      // bin-major, chunk-minor
}

// the exclusive prefix of x[0 .. n) in place by one workgroup (a thread owns consecutive entries); returns the total
__device__ uint32_t block_exclusive_scan(uint32_t* __restrict__ x, int n) {
    __shared__ uint32_t part[GR_THREADS];
    const int t = threadIdx.x;
    const int per = (n + GR_THREADS - 1) / GR_THREADS;
    const int j0 = min(n, t * per), j1 = min(n, j0 + per);
    uint32_t s = 0;
    for (int j = j0; j < j1; ++j) s += x[j];
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < GR_THREADS; o <<= 1) {
        const uint32_t u = t >= o ? part[t - o] : 0u;
        __syncthreads();
        part[t] += u;
        __syncthreads();
    }
    uint32_t run = part[t] - s;
    for (int j = j0; j < j1; ++j) {
        const uint32_t v = x[j];
        x[j] = run;
        run += v;
    }
    return part[GR_THREADS - 1];
}

// workgroup b: bin b's counts over the chunks -> offsets inside the bin, and the bin's total
__global__ __launch_bounds__(GR_THREADS) void grid_scan(uint32_t* __restrict__ hist, int chunks, uint32_t* __restrict__ tot) {
    const uint32_t total = block_exclusive_scan(hist + (long)blockIdx.x * chunks, chunks);
    if (threadIdx.x == 0) tot[blockIdx.x] = total;
}

// one wavefront per chunk.  idx_in == nullptr: the first pass, the point of position i is i
__global__ __launch_bounds__(64) void grid_scatter(const uint64_t* __restrict__ keys_in, const uint32_t* __restrict__ idx_in,
                                                    uint64_t* __restrict__ keys_out, uint32_t* __restrict__ idx_out, long M,
                                                    int shift, long chunk, int chunks, const uint32_t* __restrict__ hist,
                                                    const uint32_t* __restrict__ tot) {
    __shared__ uint32_t cur[GR_BINS];
    const int lane = threadIdx.x;
    {   // where bin b starts = the totals of the bins below it; this chunk's share of bin b starts hist[b][chunk] further
        uint32_t t4[4], s = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { t4[k] = tot[lane * 4 + k]; s += t4[k]; }
        uint32_t incl = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(incl, o, 64);
            if (lane >= o) incl += u;
        }
        uint32_t run = incl - s;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            cur[lane * 4 + k] = run + hist[(long)(lane * 4 + k) * chunks + blockIdx.x];
            run += t4[k];
        }
    }
    __syncthreads();
    const long i0 = (long)blockIdx.x * chunk;
    const long i1 = min(M, i0 + chunk);
    constexpr int U = 4;       // groups of 64 requested together: the groups are a dependent chain through the LDS cursors
    for (long t0 = i0; t0 < i1; t0 += 64 * U) {
        uint64_t kv[U];
        uint32_t pv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long i = t0 + u * 64 + lane;
            kv[u] = i < i1 ? keys_in[i] : 0ull;
            pv[u] = i < i1 ? (idx_in ? idx_in[i] : (uint32_t)i) : 0u;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (t0 + u * 64 >= i1) break;                              // wavefront-uniform
            const bool live = t0 + u * 64 + lane < i1;
            const uint32_t d = (uint32_t)(kv[u] >> shift) & (GR_BINS - 1);
            unsigned long long same = __ballot(live);                  // lanes of this group with the same digit
#pragma unroll
            for (int bit = 0; bit < 8; ++bit) {
                const unsigned long long m = __ballot((d >> bit) & 1u);
                same &= ((d >> bit) & 1u) ? m : ~m;
            }
            if (live) {
                const unsigned long long below = same & ((1ull << lane) - 1ull);
                const long pos = (long)cur[d] + __popcll(below);
                if (pos < M) {                                         // (always: the histograms counted these keys)
                    keys_out[pos] = kv[u];
                    idx_out[pos] = pv[u];
                }
                if (below == 0ull) cur[d] += (uint32_t)__popcll(same); // the first lane of the match advances the cursor
            }
            __syncthreads();
        }
    }
}

// positions per chunk and chunks of the sort (and of a client's scans over the sorted array) for M positions
inline void grid_chunks(long M, long* chunk, int* chunks) {
    long c = (M + GR_MAX_CHUNKS - 1) / GR_MAX_CHUNKS;
    c = (c + 63) / 64 * 64;
    *chunk = c < GR_MIN_CHUNK ? GR_MIN_CHUNK : c;
    *chunks = (int)((M + *chunk - 1) / *chunk);
}

// the sorted (key, point) pairs end in buffer 0 whatever the number of passes: an odd number starts from buffer 1
inline int grid_passes(int key_bits) { return (key_bits + 7) / 8; }

// The sort's pieces of a workspace: tot (GR_BINS counters), hist (GR_BINS * cap), two key and two payload buffers of M.
// cap is the capacity of the per-chunk arrays: `chunks`, or (cap > 0) a client's own bound on it.
struct RadixLayout {
    long chunk;      // positions per chunk
    int chunks;
    size_t off_tot, off_hist, off_keys[2], off_idx[2];
};

inline RadixLayout radix_layout(RlCarve& c, long M, long cap = 0) {
    RadixLayout L;
    grid_chunks(M, &L.chunk, &L.chunks);
    if (cap <= 0) cap = L.chunks;
    L.off_tot = c.take(GR_BINS * sizeof(uint32_t));
    L.off_hist = c.take((size_t)GR_BINS * cap * sizeof(uint32_t));
    for (int k = 0; k < 2; ++k) L.off_keys[k] = c.take((size_t)M * sizeof(uint64_t));
    for (int k = 0; k < 2; ++k) L.off_idx[k] = c.take((size_t)M * sizeof(uint32_t));
    return L;
}

struct RadixBufs {
    long chunk;
    int chunks;
    uint32_t *tot, *hist;
    uint64_t* keys[2];
    uint32_t* idx[2];
};

inline RadixBufs radix_bufs(const void* ws, const RadixLayout& L) {
    return {L.chunk, L.chunks, rl_at<uint32_t>(ws, L.off_tot), rl_at<uint32_t>(ws, L.off_hist),
            {rl_at<uint64_t>(ws, L.off_keys[0]), rl_at<uint64_t>(ws, L.off_keys[1])},
            {rl_at<uint32_t>(ws, L.off_idx[0]), rl_at<uint32_t>(ws, L.off_idx[1])}};
}

// The LSD radix sort of (keys, position) over `passes` 8-bit digits: the caller writes its keys to keys[passes & 1] (the first
// pass takes position i as the payload of key i), the sorted pairs end in keys[0], idx[0].
inline int radix_sort(const char* who, const RadixBufs& b, long M, int passes, hipStream_t sm) {
    char name[96];
    int cur = passes & 1;
    for (int p = 0; p < passes; ++p, cur ^= 1) {
        hipLaunchKernelGGL(grid_hist, dim3(b.chunks), dim3(GR_THREADS), 0, sm, b.keys[cur], M, 8 * p, b.chunk, b.chunks, b.hist);
        snprintf(name, sizeof(name), "%s (hist)", who);
        RL_LAUNCH_CHECK(name);
        hipLaunchKernelGGL(grid_scan, dim3(GR_BINS), dim3(GR_THREADS), 0, sm, b.hist, b.chunks, b.tot);
        snprintf(name, sizeof(name), "%s (scan)", who);
        RL_LAUNCH_CHECK(name);
        hipLaunchKernelGGL(grid_scatter, dim3(b.chunks), dim3(64), 0, sm, b.keys[cur], p == 0 ? nullptr : b.idx[cur],
                           b.keys[cur ^ 1], b.idx[cur ^ 1], M, 8 * p, b.chunk, b.chunks, b.hist, b.tot);
        snprintf(name, sizeof(name), "%s (scatter)", who);
        RL_LAUNCH_CHECK(name);
    }
    return RL_OK;          // (cur == 0 here: the sorted pairs are in buffer 0)
}

}  // namespace
