// Statistical outlier removal (rl_outliers_*; the numpy twin and the contract are randlanet/utils/outliers.py): PCL's
// StatisticalOutlierRemoval / Open3D's remove_statistical_outlier.  m_i = the mean fp64 distance of point i to its k nearest
// neighbours; mu and sigma of m over the cloud by two fixed-order fp64 sums (rl_fixedsum.h: the order of boxes.hip for one id
// whose members are points 0 .. M-1); a point with m_i > mu + std_ratio * sigma is removed, the others are numbered in
// ascending index.  -ffp-contract=off keeps every operation a correctly rounded one, so the result equals the twin's bit
// for bit.
//
//   rl_outliers_mean_distance  ol_mean     one lane per query: the k + 1 squared distances rl_knn_f32 just wrote for it, sqrt in
//                                          fp64, added in rank order, divided by k
//   rl_outliers_filter = rl_outliers_threshold, then rl_outliers_compact (exported on their own for tools/time_outliers.py)
//   rl_outliers_threshold      ol_partial  one WAVEFRONT per chunk of 1024 points: 16 coalesced turns per lane, six shuffles
//                              ol_total    one wavefront: lane l adds the chunk sums l, l + 64, .. in turn, six shuffles; lane 0
//                                          makes mu = S1 / M
//                              ol_partial, ol_total again for (m - mu) * (m - mu); lane 0 makes sigma and the threshold
//   rl_outliers_compact        ol_count    one wavefront per chunk: kept points by ballot and popcount
//                              ol_scan     one workgroup: the exclusive prefix of those counts, and M'
//                              ol_write    one wavefront per chunk: keep, slot and kept by ballots in index order
// No atomics at all, and no workgroup waits for another one.
//
// Mapping and why.  ol_mean's work per point is k + 1 loads, square roots and dependent adds, sequential inside a point, so a
// point is a lane; what can be shared is the load: the wavefront's 64 rows are one contiguous run of 64 * (k + 1) floats,
// staged into LDS with all lanes busy whatever k is and read back rank-major - (rank j, query q) at j * 64 + q - so the 64
// lanes of one read hit 64 different banks.  (k + 1) * 256 bytes of LDS: 4.25 KiB at k = 16.  The sums follow boxes.hip: a
// chunk's wavefront reads 16 runs of 512 contiguous bytes, all in flight before the first add (selects, not branches), and the
// second level of a 10^7-point cloud is 153 coalesced turns of one wavefront.  The compaction is rl_cells.h's heads pattern
// over the same chunks.  In all m is read four times (32 bytes per point) and 5 to 13 bytes per point are written.
#include "rl_fixedsum.h"
#include "rl_radix.h"

#include <math.h>

namespace {

constexpr int OL_LANES = 64;
constexpr int OL_WAVES = GR_THREADS / 64;

// what the kernels of rl_outliers_filter hand each other: mu, sigma, the threshold and M' (as a double: exact below 2^53)
struct OlStats {
    double v[4];
};

struct OlLayout {
    long chunks;         // ceil(M / FS_CHUNK)
    size_t off_part, off_cnt, bytes;
};

OlLayout outliers_layout(long M) {
    OlLayout L;
    RlCarve c;
    L.chunks = (M + FS_CHUNK - 1) / FS_CHUNK;
    c.take(sizeof(OlStats));
    L.off_part = c.take((size_t)L.chunks * sizeof(double));
    L.off_cnt = c.take((size_t)L.chunks * sizeof(uint32_t));
    L.bytes = c.at;
    return L;
}

// one wavefront = one workgroup = 64 consecutive queries, one lane per query
__global__ __launch_bounds__(OL_LANES) void ol_mean(const float* __restrict__ d2, long first, long Q, int k,
                                                    double* __restrict__ mean_out) {
    extern __shared__ float tile[];                    // [k + 1][64]
    const int lane = threadIdx.x;
    const int k1 = k + 1;
    const long q0 = (long)blockIdx.x * OL_LANES;       // this wavefront's first query, counted from `first`
    const int nq = (int)min((long)OL_LANES, Q - q0);
    const float* run = d2 + q0 * k1;
    const int entries = nq * k1;
    for (int e = lane; e < entries; e += OL_LANES) {   // entry e of the run is (query e / k1, rank e % k1)
        const int qq = e / k1, r = e - qq * k1;
        tile[r * OL_LANES + qq] = run[e];
    }
    __syncthreads();
    if (lane >= nq) return;
    double s = 0.0;
    for (int j = 0; j < k1; ++j) s = s + sqrt((double)tile[j * OL_LANES + lane]);
    mean_out[first + q0 + lane] = s / (double)k;
}

// one wavefront per chunk.  kDev: the squared differences from mu (st->v[0]); otherwise the values themselves
template <bool kDev>
__global__ __launch_bounds__(GR_THREADS) void ol_partial(const double* __restrict__ mean, long M, long chunks,
                                                          const OlStats* __restrict__ st, double* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const long c = (long)blockIdx.x * OL_WAVES + (threadIdx.x >> 6);
    if (c >= chunks) return;                           // wavefront-uniform
    const long j0 = c * FS_CHUNK;
    double m[FS_TURNS];
#pragma unroll
    for (int t = 0; t < FS_TURNS; ++t) {
        const long j = j0 + t * 64 + lane;
        m[t] = mean[j < M ? j : j0];
    }
    const double mu = kDev ? st->v[0] : 0.0;
    double acc = 0.0;
#pragma unroll
    for (int t = 0; t < FS_TURNS; ++t) {
        const bool live = j0 + t * 64 + lane < M;      // selects, not branches: the loads above stay in flight together
        const double d = m[t] - mu;
        const double v = kDev ? d * d : m[t];
        acc = live ? acc + v : acc;
    }
    const double s = fs_fold64(acc);
    if (lane == 0) part[c] = s;
}

// one wavefront: the chunk sums by the same rule.  kDev: S2 -> sigma and the threshold; otherwise S1 -> mu
template <bool kDev>
__global__ __launch_bounds__(OL_LANES) void ol_total(const double* __restrict__ part, long chunks, long M, double std_ratio,
                                                     OlStats* __restrict__ st, double* __restrict__ stats_out) {
    const int lane = threadIdx.x;
    double acc = 0.0;
    for (long c = lane; c < chunks; c += 64) acc = acc + part[c];
    const double s = fs_fold64(acc);
    if (lane != 0) return;
    if (!kDev) {
        st->v[0] = s / (double)M;
        return;
    }
    const double mu = st->v[0];
    const double sigma = sqrt(s / (double)(M - 1));
    const double thr = mu + std_ratio * sigma;
    st->v[1] = sigma;
    st->v[2] = thr;
    stats_out[0] = mu;
    stats_out[1] = sigma;
    stats_out[2] = thr;
}

// one wavefront per chunk: how many of its points are kept
__global__ __launch_bounds__(OL_LANES) void ol_count(const double* __restrict__ mean, long M, const OlStats* __restrict__ st,
                                                     uint32_t* __restrict__ cnt) {
    const int lane = threadIdx.x;
    const long j0 = (long)blockIdx.x * FS_CHUNK;
    const double thr = st->v[2];
    uint32_t n = 0;
#pragma unroll
    for (int t = 0; t < FS_TURNS; ++t) {
        const long j = j0 + t * 64 + lane;
        const double m = mean[j < M ? j : j0];
        n += (uint32_t)__popcll(__ballot(j < M && m <= thr));
    }
    if (lane == 0) cnt[blockIdx.x] = n;
}

__global__ __launch_bounds__(GR_THREADS) void ol_scan(uint32_t* __restrict__ cnt, int chunks, OlStats* __restrict__ st,
                                                      double* __restrict__ stats_out) {
    const uint32_t kept = block_exclusive_scan(cnt, chunks);
    if (threadIdx.x == 0) {
        st->v[3] = (double)kept;
        stats_out[3] = (double)kept;
    }
}

__global__ __launch_bounds__(OL_LANES) void ol_write(const double* __restrict__ mean, long M, const OlStats* __restrict__ st,
                                                     const uint32_t* __restrict__ cnt, uint8_t* __restrict__ keep_out,
                                                     int32_t* __restrict__ slot_out, int64_t* __restrict__ kept_out) {
    const int lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    const long j0 = (long)blockIdx.x * FS_CHUNK;
    const double thr = st->v[2];
    uint32_t run = cnt[blockIdx.x];                    // kept points before this chunk
    for (int t = 0; t < FS_TURNS; ++t) {
        if (j0 + t * 64 >= M) break;                   // wavefront-uniform
        const long j = j0 + t * 64 + lane;
        const bool live = j < M;
        const bool keep = live && mean[live ? j : j0] <= thr;
        const unsigned long long b = __ballot(keep);
        if (live) {
            const long s = (long)run + __popcll(b & below);
            keep_out[j] = keep ? 1 : 0;
            slot_out[j] = keep ? (int32_t)s : -1;
            if (keep && s < M) kept_out[s] = (int64_t)j;           // (always: s counts kept points below j)
        }
        run += (uint32_t)__popcll(b);
    }
}

}  // namespace

extern "C" int64_t rl_outliers_workspace_bytes(int64_t M) {
    if (M < 2 || M >= 0x7fffffffLL) return 0;
    return (int64_t)outliers_layout(M).bytes;
}

extern "C" int rl_outliers_mean_distance(const float* d2, int64_t M, int64_t first, int64_t Q, int k, double* mean_out,
                                         void* stream) {
    RL_REQUIRE(k >= 1 && k < RL_KNN_MAX_K, RL_ERR_ARGS, "rl_outliers_mean_distance: k=%d outside 1 .. %d", k, RL_KNN_MAX_K - 1);
    RL_REQUIRE(M > k && M < 0x7fffffffLL, RL_ERR_ARGS, "rl_outliers_mean_distance: M=%lld outside k+1=%d .. 2^31-2",
               (long long)M, k + 1);
    RL_REQUIRE(first >= 0 && Q > 0 && first <= M - Q, RL_ERR_ARGS,
               "rl_outliers_mean_distance: queries %lld .. %lld of M=%lld points", (long long)first,
               (long long)first + (long long)Q - 1, (long long)M);
    RL_REQUIRE(d2 && mean_out, RL_ERR_ARGS, "rl_outliers_mean_distance: null pointer");
    const size_t lds = (size_t)(k + 1) * OL_LANES * sizeof(float);
    hipLaunchKernelGGL(ol_mean, dim3(rl_cdiv(Q, OL_LANES)), dim3(OL_LANES), lds, (hipStream_t)stream, d2, (long)first, (long)Q,
                       k, mean_out);
    rl_note_kernel("ol_mean");
    RL_LAUNCH_CHECK("rl_outliers_mean_distance");
    return RL_OK;
}

namespace {

int outliers_check(const char* who, int64_t M, const void* ws, int64_t ws_bytes) {
    RL_REQUIRE(M >= 2 && M < 0x7fffffffLL, RL_ERR_ARGS, "%s: M=%lld outside 2 .. 2^31-2", who, (long long)M);
    return rl_ws_check(who, ws, ws_bytes, rl_outliers_workspace_bytes(M));
}

}  // namespace

extern "C" int rl_outliers_threshold(const double* mean, int64_t M, double std_ratio, double* stats_out, void* ws,
                                     int64_t ws_bytes, void* stream) {
    RL_REQUIRE(std_ratio >= 0.0 && std_ratio <= 1.7976931348623157e308, RL_ERR_ARGS,
               "rl_outliers_threshold: std_ratio=%g is not a finite number >= 0", std_ratio);
    int rc = outliers_check("rl_outliers_threshold", M, ws, ws_bytes);
    if (rc) return rc;
    RL_REQUIRE(mean && stats_out, RL_ERR_ARGS, "rl_outliers_threshold: null pointer");
    hipStream_t sm = (hipStream_t)stream;
    const OlLayout L = outliers_layout(M);
    OlStats* st = (OlStats*)ws;
    double* part = rl_at<double>(ws, L.off_part);
    const dim3 block(GR_THREADS), wave(OL_LANES), per_chunk(rl_cdiv(L.chunks, OL_WAVES));
    hipLaunchKernelGGL(ol_partial<false>, per_chunk, block, 0, sm, mean, (long)M, L.chunks, (const OlStats*)st, part);
    RL_LAUNCH_CHECK("rl_outliers_threshold (mean partial)");
    hipLaunchKernelGGL(ol_total<false>, dim3(1), wave, 0, sm, (const double*)part, L.chunks, (long)M, std_ratio, st, stats_out);
    RL_LAUNCH_CHECK("rl_outliers_threshold (mean)");
    hipLaunchKernelGGL(ol_partial<true>, per_chunk, block, 0, sm, mean, (long)M, L.chunks, (const OlStats*)st, part);
    RL_LAUNCH_CHECK("rl_outliers_threshold (deviation partial)");
    hipLaunchKernelGGL(ol_total<true>, dim3(1), wave, 0, sm, (const double*)part, L.chunks, (long)M, std_ratio, st, stats_out);
    rl_note_kernel("ol_total");
    RL_LAUNCH_CHECK("rl_outliers_threshold (threshold)");
    return RL_OK;
}

extern "C" int rl_outliers_compact(const double* mean, int64_t M, uint8_t* keep_out, int32_t* slot_out, int64_t* kept_out,
                                   double* stats_out, void* ws, int64_t ws_bytes, void* stream) {
    int rc = outliers_check("rl_outliers_compact", M, ws, ws_bytes);
    if (rc) return rc;
    RL_REQUIRE(mean && keep_out && slot_out && kept_out && stats_out, RL_ERR_ARGS, "rl_outliers_compact: null pointer");
    hipStream_t sm = (hipStream_t)stream;
    const OlLayout L = outliers_layout(M);
    OlStats* st = (OlStats*)ws;
    uint32_t* cnt = rl_at<uint32_t>(ws, L.off_cnt);
    const dim3 block(GR_THREADS), wave(OL_LANES);
    hipLaunchKernelGGL(ol_count, dim3((unsigned)L.chunks), wave, 0, sm, mean, (long)M, (const OlStats*)st, cnt);
    RL_LAUNCH_CHECK("rl_outliers_compact (count)");
    hipLaunchKernelGGL(ol_scan, dim3(1), block, 0, sm, cnt, (int)L.chunks, st, stats_out);
    RL_LAUNCH_CHECK("rl_outliers_compact (scan)");
    hipLaunchKernelGGL(ol_write, dim3((unsigned)L.chunks), wave, 0, sm, mean, (long)M, (const OlStats*)st,
                       (const uint32_t*)cnt, keep_out, slot_out, kept_out);
    rl_note_kernel("ol_write");
    RL_LAUNCH_CHECK("rl_outliers_compact (write)");
    return RL_OK;
}

// the two halves in order, every refusal of both before the first launch
extern "C" int rl_outliers_filter(const double* mean, int64_t M, double std_ratio, uint8_t* keep_out, int32_t* slot_out,
                                  int64_t* kept_out, double* stats_out, void* ws, int64_t ws_bytes, void* stream) {
    RL_REQUIRE(std_ratio >= 0.0 && std_ratio <= 1.7976931348623157e308, RL_ERR_ARGS,
               "rl_outliers_filter: std_ratio=%g is not a finite number >= 0", std_ratio);
    int rc = outliers_check("rl_outliers_filter", M, ws, ws_bytes);
    if (rc) return rc;
    RL_REQUIRE(mean && keep_out && slot_out && kept_out && stats_out, RL_ERR_ARGS, "rl_outliers_filter: null pointer");
    rc = rl_outliers_threshold(mean, M, std_ratio, stats_out, ws, ws_bytes, stream);
    if (rc) return rc;
    return rl_outliers_compact(mean, M, keep_out, slot_out, kept_out, stats_out, ws, ws_bytes, stream);
}
