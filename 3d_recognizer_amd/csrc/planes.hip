// RANSAC plane segmentation (rl_planes_*; the numpy twin and the contract are randlanet/utils/planes.py): PCL's SACSegmentation
// with SACMODEL_PLANE / Open3D's segment_plane.  T planes through three points each, every one scored by the number of points
// within `threshold` of it, s = ((nx*x + ny*y) + nz*z) + d and |s| <= threshold; the first maximum wins.  Every operation is
// one correctly rounded fp32 one (-ffp-contract=off; packed v_pk_* halves round on their own) and the scores are integers, so
// the result equals the twin's bit for bit whatever the order of the work.
//
//   rl_planes_hypotheses  pl_hyp         ONE workgroup, one lane per hypothesis and turn: gathers three rows, writes the plane
//                                        or four NaNs, and ORs the "index outside [0, M)" flag over the workgroup
//   rl_planes_count       pl_count       the hot path, T * M tests: one wavefront per (128 hypotheses, chunk of points); a lane
//                                        holds two hypotheses' coefficients in registers, the points are wave-uniform (scalar
//                                        loads), the counts stay in the lane's registers: no ballot, no shuffle, no atomic.
//                                        Writes its row piece of the table [chunks][T], coalesced
//                         pl_sum         one workgroup per 64 hypotheses, 16 wavefronts: wavefront w adds the chunks w, w + 16,
//                                        .., LDS, wavefront 0 adds the 16 partial counts (integers: any order)
//                         pl_best        one workgroup: the first maximum of counts and its index, -1 when it is 0
//   rl_planes_split       pl_count_mask  one wavefront per chunk of 1024 points: the points NOT on the plane by ballot
//                         pl_scan        one workgroup: the exclusive prefix of those counts, and M'
//                         pl_write       one wavefront per chunk: inlier, slot and kept by ballots in index order
// No atomics at all, and no workgroup waits for another one.
//
// Mapping and why.  The test is six fp32 operations, a compare and an integer add; nothing in it can be shared between two
// hypotheses or two points but the operands.  With a hypothesis per lane the four coefficients are loaded once per chunk and
// the point's three coordinates come from the scalar cache as SGPR operands, so the inner loop is VALU work only, and the
// count needs no cross-lane step.  The alternative - points in registers, the hypothesis uniform, ballot and a scalar
// popcount per test - is as exact but adds a ballot and scalar work to every test and cannot use the packed operations, so
// it was not built (has the instruction counts and the measured times).  The chunk is sized so that the table stays at 2^20 entries (4 MiB) or 8 chunks, whichever is larger: at most 1024
// chunks, at least 256 points each.
#include "rl_fixedsum.h"
#include "rl_radix.h"

#include <math.h>

namespace {

constexpr int PL_LANES = 64;
constexpr int PL_H = 2;                          // hypotheses a lane of pl_count owns
constexpr int PL_GROUP = PL_LANES * PL_H;        // hypotheses of one wavefront
constexpr int PL_HYP_THREADS = 1024;
constexpr int PL_SUM_WAVES = 16;
constexpr long PL_MIN_CHUNK = 256;               // points per chunk of pl_count, a multiple of 64
constexpr long PL_MAX_CHUNKS = 1024;
constexpr long PL_TABLE = 1L << 20;              // table entries aimed at
constexpr long PL_FEW_CHUNKS = 8;                // .. but never fewer chunks than this allowed
constexpr int PL_UNROLL = 8;

struct PlLayout {
    long chunk;          // points per chunk of pl_count
    long chunks;
    long split_chunks;   // ceil(M / FS_CHUNK): the chunks of the compaction
    size_t off_cnt, off_table, bytes;
};

// the compaction's counts come first: their place depends on M alone, so rl_planes_split needs no T
PlLayout planes_layout(long M, long T) {
    PlLayout L;
    RlCarve c;
    long cap = PL_TABLE / T;
    cap = cap < PL_FEW_CHUNKS ? PL_FEW_CHUNKS : cap > PL_MAX_CHUNKS ? PL_MAX_CHUNKS : cap;
    L.chunk = ((M + cap - 1) / cap + 63) / 64 * 64;
    if (L.chunk < PL_MIN_CHUNK) L.chunk = PL_MIN_CHUNK;
    L.chunks = (M + L.chunk - 1) / L.chunk;
    L.split_chunks = (M + FS_CHUNK - 1) / FS_CHUNK;
    L.off_cnt = c.take((size_t)L.split_chunks * sizeof(uint32_t));
    L.off_table = c.take((size_t)L.chunks * (size_t)T * sizeof(uint32_t));
    L.bytes = c.at;
    return L;
}

struct PlAxis {
    float x, y, z, cos_min;
    int on;
};

__global__ __launch_bounds__(PL_HYP_THREADS) void pl_hyp(const float* __restrict__ xyz, long M, const int64_t* __restrict__ tri,
                                                         int T, PlAxis ax, float* __restrict__ planes,
                                                         int32_t* __restrict__ bad_out) {
    int bad = 0;
    const float nan = __int_as_float(0x7fc00000);
    for (int t = threadIdx.x; t < T; t += PL_HYP_THREADS) {
        const int64_t i0 = tri[3 * (long)t], i1 = tri[3 * (long)t + 1], i2 = tri[3 * (long)t + 2];
        const bool inside = i0 >= 0 && i0 < M && i1 >= 0 && i1 < M && i2 >= 0 && i2 < M;
        float nx = nan, ny = nan, nz = nan, d = nan;
        if (inside) {
            const float ax0 = xyz[3 * i0], ay0 = xyz[3 * i0 + 1], az0 = xyz[3 * i0 + 2];
            const float e1x = xyz[3 * i1] - ax0, e1y = xyz[3 * i1 + 1] - ay0, e1z = xyz[3 * i1 + 2] - az0;
            const float e2x = xyz[3 * i2] - ax0, e2y = xyz[3 * i2 + 1] - ay0, e2z = xyz[3 * i2 + 2] - az0;
            const float cx = e1y * e2z - e1z * e2y;
            const float cy = e1z * e2x - e1x * e2z;
            const float cz = e1x * e2y - e1y * e2x;
            const float l2 = (cx * cx + cy * cy) + cz * cz;
            // the correctly rounded fp32 root: the fp64 one (correctly rounded, as in outliers.hip) rounded once more is it,
            // since 53 >= 2 * 24 + 2 bits; __fsqrt_rn compiles to a bare v_sqrt_f32 here, one ulp off now and then
            const float r = (float)sqrt((double)l2);
            const float hx = __fdiv_rn(cx, r), hy = __fdiv_rn(cy, r), hz = __fdiv_rn(cz, r);
            bool valid = l2 > 0.0f && l2 <= 3.4028234663852886e38f;
            if (ax.on) valid = valid && fabsf((hx * ax.x + hy * ax.y) + hz * ax.z) >= ax.cos_min;
            if (valid) {
                nx = hx, ny = hy, nz = hz;
                d = -((hx * ax0 + hy * ay0) + hz * az0);
            }
        } else {
            bad = 1;
        }
        float4* out = (float4*)planes;           // (hipMalloc'ed and offset by whole rows: 16-byte aligned is asked for)
        out[t] = make_float4(nx, ny, nz, d);
    }
    const int any = __syncthreads_or(bad);
    if (threadIdx.x == 0) bad_out[0] = any ? 1 : 0;
}

typedef float pl_f2 __attribute__((ext_vector_type(2)));

// one point against the lane's two hypotheses, side by side in the halves of a packed operation (each half is rounded on
// its own); x, y, z are wave-uniform
__device__ __forceinline__ void pl_test(pl_f2 nx, pl_f2 ny, pl_f2 nz, pl_f2 d, float x, float y, float z, float thr,
                                        uint32_t& n0, uint32_t& n1) {
    const pl_f2 s = ((nx * x + ny * y) + nz * z) + d;
    n0 += fabsf(s.x) <= thr ? 1u : 0u;
    n1 += fabsf(s.y) <= thr ? 1u : 0u;
}

// grid (hypothesis groups, chunks), one wavefront each
__global__ __launch_bounds__(PL_LANES) void pl_count(const float* __restrict__ xyz, long M, const float* __restrict__ planes,
                                                     int T, float thr, long chunk, uint32_t* __restrict__ table) {
    static_assert(PL_H == 2, "a lane holds its hypotheses in the two halves of packed registers");
    const int lane = threadIdx.x;
    const int t0 = blockIdx.x * PL_GROUP + lane;             // the lane's hypotheses: t0 and t0 + 64
    const int t1 = t0 + PL_LANES;
    const float nan = __int_as_float(0x7fc00000);
    const float4 a = t0 < T ? ((const float4*)planes)[t0] : make_float4(nan, nan, nan, nan);
    const float4 b = t1 < T ? ((const float4*)planes)[t1] : make_float4(nan, nan, nan, nan);
    const pl_f2 nx = {a.x, b.x}, ny = {a.y, b.y}, nz = {a.z, b.z}, d = {a.w, b.w};
    uint32_t n0 = 0u, n1 = 0u;
    const long j0 = (long)blockIdx.y * chunk;
    const long j1 = min(M, j0 + chunk);
    const float* __restrict__ p = xyz + 3 * j0;
    long j = j0;
    for (; j + PL_UNROLL <= j1; j += PL_UNROLL, p += 3 * PL_UNROLL) {
        float q[3 * PL_UNROLL];
#pragma unroll
        for (int u = 0; u < 3 * PL_UNROLL; ++u) q[u] = p[u];
#pragma unroll
        for (int u = 0; u < PL_UNROLL; ++u) pl_test(nx, ny, nz, d, q[3 * u], q[3 * u + 1], q[3 * u + 2], thr, n0, n1);
    }
    for (; j < j1; ++j, p += 3) pl_test(nx, ny, nz, d, p[0], p[1], p[2], thr, n0, n1);
    uint32_t* row = table + (long)blockIdx.y * T;
    if (t0 < T) row[t0] = n0;
    if (t1 < T) row[t1] = n1;
}

// one workgroup per 64 hypotheses
__global__ __launch_bounds__(PL_LANES * PL_SUM_WAVES) void pl_sum(const uint32_t* __restrict__ table, int chunks, int T,
                                                                  int32_t* __restrict__ counts) {
    __shared__ uint32_t part[PL_SUM_WAVES][PL_LANES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int t = blockIdx.x * PL_LANES + lane;
    uint32_t s = 0;
    if (t < T)
        for (int c = w; c < chunks; c += PL_SUM_WAVES) s += table[(long)c * T + t];
    part[w][lane] = s;
    __syncthreads();
    if (w != 0 || t >= T) return;
    s = 0;
#pragma unroll
    for (int k = 0; k < PL_SUM_WAVES; ++k) s += part[k][lane];
    counts[t] = (int32_t)s;
}

// one workgroup: the first maximum.  key = count * 2^32 + (2^32 - 1 - t): the largest key is the largest count at the lowest t
__global__ __launch_bounds__(GR_THREADS) void pl_best(const int32_t* __restrict__ counts, int T, int32_t* __restrict__ best) {
    __shared__ unsigned long long key[GR_THREADS];
    unsigned long long k = 0ull;
    for (int t = threadIdx.x; t < T; t += GR_THREADS) {
        const unsigned long long v = ((unsigned long long)(uint32_t)counts[t] << 32) | (0xffffffffu - (uint32_t)t);
        k = v > k ? v : k;
    }
    key[threadIdx.x] = k;
    __syncthreads();
    for (int o = GR_THREADS / 2; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) key[threadIdx.x] = max(key[threadIdx.x], key[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const uint32_t n = (uint32_t)(key[0] >> 32);
        best[0] = n ? (int32_t)(0xffffffffu - (uint32_t)key[0]) : -1;
        best[1] = (int32_t)n;
    }
}

// the plane of the split: row best[0] of `planes` (four NaNs when no plane was found), or `planes` itself without `best`
__device__ __forceinline__ float4 pl_plane(const float* __restrict__ planes, const int32_t* __restrict__ best) {
    const float nan = __int_as_float(0x7fc00000);
    if (!best) return ((const float4*)planes)[0];
    const int b = best[0];
    return b < 0 ? make_float4(nan, nan, nan, nan) : ((const float4*)planes)[b];
}

__device__ __forceinline__ bool pl_inlier(const float4 pl, const float* __restrict__ xyz, long j, float thr) {
    const float s = ((pl.x * xyz[3 * j] + pl.y * xyz[3 * j + 1]) + pl.z * xyz[3 * j + 2]) + pl.w;
    return fabsf(s) <= thr;
}

// one wavefront per chunk: how many of its points are NOT on the plane
__global__ __launch_bounds__(PL_LANES) void pl_count_mask(const float* __restrict__ xyz, long M, const float* __restrict__ planes,
                                                          const int32_t* __restrict__ best, float thr,
                                                          uint32_t* __restrict__ cnt) {
    const int lane = threadIdx.x;
    const long j0 = (long)blockIdx.x * FS_CHUNK;
    const float4 pl = pl_plane(planes, best);
    uint32_t n = 0;
#pragma unroll 4
    for (int t = 0; t < FS_TURNS; ++t) {
        const long j = j0 + t * 64 + lane;
        const bool live = j < M;
        n += (uint32_t)__popcll(__ballot(live && !pl_inlier(pl, xyz, live ? j : j0, thr)));
    }
    if (lane == 0) cnt[blockIdx.x] = n;
}

__global__ __launch_bounds__(GR_THREADS) void pl_scan(uint32_t* __restrict__ cnt, int chunks, int64_t* __restrict__ n_out) {
    const uint32_t kept = block_exclusive_scan(cnt, chunks);
    if (threadIdx.x == 0) n_out[0] = (int64_t)kept;
}

__global__ __launch_bounds__(PL_LANES) void pl_write(const float* __restrict__ xyz, long M, const float* __restrict__ planes,
                                                     const int32_t* __restrict__ best, float thr,
                                                     const uint32_t* __restrict__ cnt, uint8_t* __restrict__ inlier_out,
                                                     int32_t* __restrict__ slot_out, int64_t* __restrict__ kept_out) {
    const int lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    const long j0 = (long)blockIdx.x * FS_CHUNK;
    const float4 pl = pl_plane(planes, best);
    uint32_t run = cnt[blockIdx.x];                    // kept points before this chunk
    for (int t = 0; t < FS_TURNS; ++t) {
        if (j0 + t * 64 >= M) break;                   // wavefront-uniform
        const long j = j0 + t * 64 + lane;
        const bool live = j < M;
        const bool keep = live && !pl_inlier(pl, xyz, live ? j : j0, thr);
        const unsigned long long b = __ballot(keep);
        if (live) {
            const long s = (long)run + __popcll(b & below);
            inlier_out[j] = keep ? 0 : 1;
            slot_out[j] = keep ? (int32_t)s : -1;
            if (keep && s < M) kept_out[s] = (int64_t)j;           // (always: s counts kept points below j)
        }
        run += (uint32_t)__popcll(b);
    }
}

bool pl_size_ok(int64_t M) { return M >= 3 && M < 0x7fffffffLL; }
bool pl_threshold_ok(float thr) { return thr > 0.0f && thr <= 3.4028234663852886e38f; }

}  // namespace

extern "C" int64_t rl_planes_workspace_bytes(int64_t M, int64_t T) {
    if (!pl_size_ok(M) || T < 1 || T > RL_PLANES_MAX_HYPOTHESES) return 0;
    return (int64_t)planes_layout(M, T).bytes;
}

extern "C" int rl_planes_hypotheses(const float* xyz, int64_t M, const int64_t* triples, int64_t T, const float* axis,
                                    float cos_min, float* planes_out, int32_t* bad_out, void* stream) {
    RL_REQUIRE(pl_size_ok(M), RL_ERR_ARGS, "rl_planes_hypotheses: M=%lld outside 3 .. 2^31-2", (long long)M);
    RL_REQUIRE(T >= 1 && T <= RL_PLANES_MAX_HYPOTHESES, RL_ERR_ARGS, "rl_planes_hypotheses: T=%lld outside 1 .. %d",
               (long long)T, RL_PLANES_MAX_HYPOTHESES);
    RL_REQUIRE(xyz && triples && planes_out && bad_out, RL_ERR_ARGS, "rl_planes_hypotheses: null pointer");
    RL_REQUIRE(((uintptr_t)planes_out & 15) == 0, RL_ERR_ARGS, "rl_planes_hypotheses: planes_out not 16-byte aligned");
    PlAxis ax = {0.0f, 0.0f, 0.0f, 0.0f, 0};
    if (axis) {
        ax = {axis[0], axis[1], axis[2], cos_min, 1};
        RL_REQUIRE(isfinite(ax.x) && isfinite(ax.y) && isfinite(ax.z) && cos_min >= 0.0f && cos_min <= 1.0f, RL_ERR_ARGS,
                   "rl_planes_hypotheses: axis (%g, %g, %g) not finite or cos_min=%g outside 0 .. 1", ax.x, ax.y, ax.z, cos_min);
    }
    hipLaunchKernelGGL(pl_hyp, dim3(1), dim3(PL_HYP_THREADS), 0, (hipStream_t)stream, xyz, (long)M, triples, (int)T, ax,
                       planes_out, bad_out);
    rl_note_kernel("pl_hyp");
    RL_LAUNCH_CHECK("rl_planes_hypotheses");
    return RL_OK;
}

extern "C" int rl_planes_count(const float* xyz, int64_t M, const float* planes, int64_t T, float threshold,
                               int32_t* counts_out, int32_t* best_out, void* ws, int64_t ws_bytes, void* stream) {
    RL_REQUIRE(pl_size_ok(M), RL_ERR_ARGS, "rl_planes_count: M=%lld outside 3 .. 2^31-2", (long long)M);
    RL_REQUIRE(T >= 1 && T <= RL_PLANES_MAX_HYPOTHESES, RL_ERR_ARGS, "rl_planes_count: T=%lld outside 1 .. %d", (long long)T,
               RL_PLANES_MAX_HYPOTHESES);
    RL_REQUIRE(pl_threshold_ok(threshold), RL_ERR_ARGS, "rl_planes_count: threshold=%g is not a finite number > 0",
               (double)threshold);
    int rc = rl_ws_check("rl_planes_count", ws, ws_bytes, rl_planes_workspace_bytes(M, T));
    if (rc) return rc;
    RL_REQUIRE(xyz && planes && counts_out && best_out, RL_ERR_ARGS, "rl_planes_count: null pointer");
    RL_REQUIRE(((uintptr_t)planes & 15) == 0, RL_ERR_ARGS, "rl_planes_count: planes not 16-byte aligned");
    hipStream_t sm = (hipStream_t)stream;
    const PlLayout L = planes_layout(M, T);
    uint32_t* table = rl_at<uint32_t>(ws, L.off_table);
    hipLaunchKernelGGL(pl_count, dim3(rl_cdiv(T, PL_GROUP), (unsigned)L.chunks), dim3(PL_LANES), 0, sm, xyz, (long)M, planes,
                       (int)T, threshold, L.chunk, table);
    RL_LAUNCH_CHECK("rl_planes_count (count)");
    hipLaunchKernelGGL(pl_sum, dim3(rl_cdiv(T, PL_LANES)), dim3(PL_LANES * PL_SUM_WAVES), 0, sm, (const uint32_t*)table,
                       (int)L.chunks, (int)T, counts_out);
    RL_LAUNCH_CHECK("rl_planes_count (sum)");
    hipLaunchKernelGGL(pl_best, dim3(1), dim3(GR_THREADS), 0, sm, (const int32_t*)counts_out, (int)T, best_out);
    rl_note_kernel("pl_best");
    RL_LAUNCH_CHECK("rl_planes_count (best)");
    return RL_OK;
}

extern "C" int rl_planes_split(const float* xyz, int64_t M, const float* plane, const int32_t* best, float threshold,
                               uint8_t* inlier_out, int32_t* slot_out, int64_t* kept_out, int64_t* n_out, void* ws,
                               int64_t ws_bytes, void* stream) {
    RL_REQUIRE(pl_size_ok(M), RL_ERR_ARGS, "rl_planes_split: M=%lld outside 3 .. 2^31-2", (long long)M);
    RL_REQUIRE(pl_threshold_ok(threshold), RL_ERR_ARGS, "rl_planes_split: threshold=%g is not a finite number > 0",
               (double)threshold);
    int rc = rl_ws_check("rl_planes_split", ws, ws_bytes, rl_planes_workspace_bytes(M, 1));
    if (rc) return rc;
    RL_REQUIRE(xyz && plane && inlier_out && slot_out && kept_out && n_out, RL_ERR_ARGS, "rl_planes_split: null pointer");
    RL_REQUIRE(((uintptr_t)plane & 15) == 0, RL_ERR_ARGS, "rl_planes_split: plane not 16-byte aligned");
    hipStream_t sm = (hipStream_t)stream;
    const PlLayout L = planes_layout(M, 1);
    uint32_t* cnt = rl_at<uint32_t>(ws, L.off_cnt);
    const dim3 wave(PL_LANES), per_chunk((unsigned)L.split_chunks);
    hipLaunchKernelGGL(pl_count_mask, per_chunk, wave, 0, sm, xyz, (long)M, plane, best, threshold, cnt);
    RL_LAUNCH_CHECK("rl_planes_split (count)");
    hipLaunchKernelGGL(pl_scan, dim3(1), dim3(GR_THREADS), 0, sm, cnt, (int)L.split_chunks, n_out);
    RL_LAUNCH_CHECK("rl_planes_split (scan)");
    hipLaunchKernelGGL(pl_write, per_chunk, wave, 0, sm, xyz, (long)M, plane, best, threshold, (const uint32_t*)cnt, inlier_out,
                       slot_out, kept_out);
    rl_note_kernel("pl_write");
    RL_LAUNCH_CHECK("rl_planes_split (write)");
    return RL_OK;
}
