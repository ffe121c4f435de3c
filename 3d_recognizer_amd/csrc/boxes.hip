// Oriented boxes of point sets given by integer ids (utils/boxes.py: instance_boxes; Model.predict_instances(oriented_boxes=
// True), Model.evaluate_instances(boxes=True)): per id count, axis-aligned box, and the box along the principal axes of its
// points - fp64 mean and covariance, 6 cyclic Jacobi sweeps (rl_jacobi.h, shared with normals.hip), projection min / max.
// The numpy twin and the contract are randlanet/utils/boxes.py; every fp64 sum runs in the twin's fixed order and
// -ffp-contract=off keeps every operation a correctly rounded one, so the result equals the twin's bit for bit.
//
//   rl_boxes_sort     keys        key = id for 0 <= id < I, the sentinel I for every other point (sorted to the end)
//                     sort        the stable radix sort of (key, point index) (rl_radix.h): the members of an id follow each
//                                 other in ascending point index
//                     starts      one lane per id: start[k] = the first sorted position whose key is >= k (binary search), so
//                                 an id without members is an empty run and start[I] ends the last one
//                     counts      chunks of id k = ceil(n_k / BX_CHUNK)
//                     scan        one workgroup: the exclusive prefix of those = the first chunk of every id; their sum NC
//   rl_boxes_moments  partial     one WAVEFRONT per chunk (below): lane sums over its turns, folded in halves -> 3 sums
//                     fold        one wavefront per id: lane l adds the chunk sums l, l + 64, .. in turn, folded in halves;
//                                 mean = sum / n_k
//                     partial, fold again for the six products of the differences from the mean -> covariance
//   rl_boxes_fit      axes        one lane per id: Jacobi, eigenvalues in descending order, the two leading columns made
//                                 orthonormal, signs, the normalised cross product
//                     project     one wavefront per chunk: t_a = (dx*a0 + dy*a1) + dz*a2 per member and axis, min / max of t
//                                 and of the coordinates over the chunk (min and max do not depend on the order)
//                     final       one wavefront per id: min / max over its chunks, extent, center, the one rounding to fp32
// No atomics at all, no LDS outside the sort, and no workgroup waits for another one.
//
// Mapping and why.  The sums must have ONE order that is a function of n_k alone, that a wavefront can follow at full memory
// width, and that spreads a wall of 10^6 points over many wavefronts (cluster.hip's cl_reduce, one wavefront per instance
// adding member after member, does neither).  A chunk is BX_CHUNK = 64 * BX_TURNS = 1024 consecutive members of one id,
// counted from the id's first member - not 1024 sorted positions - so the order cannot depend on where an id lies among the
// others.  Lane l of the chunk's wavefront takes members l, l + 64, ..: one load instruction reads 64 consecutive entries
// of the sorted index (256 contiguous bytes) and gathers 64 rows of 12 bytes that ascend in memory; the BX_TURNS loads of
// a lane are independent and the adds that follow are selects, not branches, so all 16 are in flight before the first add.
// The 64 lane sums are folded in halves by six xor-shuffles (no LDS allocation, no bank conflicts) - a sequential pass over
// the lanes would cost 64 dependent fp64 adds per value, four times the 16 turns themselves.  BX_TURNS = 16: the 48
// coordinate registers of a lane bring the mean pass to 70 VGPRs, the covariance pass to 115 and the projection - nine axis
// components and twelve running extremes in fp64 on top - to 190, all without scratch; a 5 * 10^6-point id becomes 4883
// wavefronts (19 per CU of 256), and the fixed cost per chunk - a binary search for the id, six shuffles per value, one
// 48-byte store - is spread over 1024 members.  The chunk sums of an id are added by the same rule (lane l takes chunks l,
// l + 64, ..), so the second level of a 10^7-point id is 153 coalesced turns of one wavefront, not 9766 dependent adds of
// one lane.  Measured on 10^7 points: 1.08 ms with 10^4 even ids, 0.82 ms with one id holding half of them.
#include "rl_cells.h"
#include "rl_fixedsum.h"
#include "rl_jacobi.h"

namespace {

constexpr int BX_TURNS = FS_TURNS;
constexpr int BX_CHUNK = FS_CHUNK;           // members per chunk (CHUNK of utils/boxes.py)
constexpr int BX_WAVES = GR_THREADS / 64;

struct BoxState {
    int64_t NC;          // chunks of all ids
    int64_t pad[3];
};

struct BoxLayout {
    RadixLayout sort;
    long parts;          // upper bound of NC: M / BX_CHUNK + min(I, M)
    size_t off_start, off_cb, off_mean, off_cov, off_axes, off_lam, off_part, off_box, bytes;
};

BoxLayout boxes_layout(long M, long I) {
    BoxLayout L;
    RlCarve c;
    L.parts = M / BX_CHUNK + (I < M ? I : M);
    c.take(sizeof(BoxState));
    L.sort = radix_layout(c, M);
    L.off_start = c.take((size_t)(I + 1) * sizeof(uint32_t));
    L.off_cb = c.take((size_t)(I + 1) * sizeof(uint32_t));
    L.off_mean = c.take((size_t)I * 3 * sizeof(double));
    L.off_cov = c.take((size_t)I * 6 * sizeof(double));
    L.off_axes = c.take((size_t)I * 9 * sizeof(double));
    L.off_lam = c.take((size_t)I * 3 * sizeof(double));
    L.off_part = c.take((size_t)L.parts * 6 * sizeof(double));
    L.off_box = c.take((size_t)L.parts * 6 * sizeof(float));
    L.bytes = c.at;
    return L;
}

__global__ __launch_bounds__(GR_THREADS) void bx_keys(const void* __restrict__ ids, int is64, long M, long I,
                                                       uint64_t* __restrict__ keys) {
    const long i = (long)blockIdx.x * GR_THREADS + threadIdx.x;
    if (i >= M) return;
    const int64_t v = is64 ? ((const int64_t*)ids)[i] : (int64_t)((const int32_t*)ids)[i];
    keys[i] = v >= 0 && v < I ? (uint64_t)v : (uint64_t)I;
}

// one lane per k in [0, I]: the first position whose key is >= k
__global__ __launch_bounds__(GR_THREADS) void bx_starts(const uint64_t* __restrict__ keys, long M, long I,
                                                         uint32_t* __restrict__ start) {
    const long k = (long)blockIdx.x * GR_THREADS + threadIdx.x;
    if (k > I) return;
    long a = 0, b = M;
    while (a < b) {
        const long m = a + ((b - a) >> 1);
        if (keys[m] < (uint64_t)k) a = m + 1;
        else b = m;
    }
    start[k] = (uint32_t)a;
}

__global__ __launch_bounds__(GR_THREADS) void bx_counts(const uint32_t* __restrict__ start, long I, uint32_t* __restrict__ cb) {
    const long k = (long)blockIdx.x * GR_THREADS + threadIdx.x;
    if (k >= I) return;
    const uint32_t s0 = start[k], s1 = start[k + 1];
    const uint32_t n = s1 > s0 ? s1 - s0 : 0u;
    cb[k] = (n + (uint32_t)(BX_CHUNK - 1)) / (uint32_t)BX_CHUNK;
}

__global__ __launch_bounds__(GR_THREADS) void bx_scan(uint32_t* __restrict__ cb, long I, BoxState* __restrict__ st) {
    const uint32_t total = block_exclusive_scan(cb, (int)I);
    if (threadIdx.x == 0) {
        cb[I] = total;
        st->NC = (int64_t)total;
    }
}

// What a wavefront needs to know about chunk c: its id k and its members' sorted positions j0 .. j1-1.  Wavefront-uniform.
struct BoxChunk {
    long k, j0, j1;
};

__device__ __forceinline__ bool bx_chunk(long c, long M, long I, long parts, const uint32_t* __restrict__ start,
                                         const uint32_t* __restrict__ cb, const BoxState* __restrict__ st, BoxChunk* out) {
    if (c >= parts || c >= st->NC) return false;
    long a = 0, b = I;                       // cb[a] <= c < cb[b]: cb[0] = 0 and cb[I] = NC
    while (b - a > 1) {
        const long m = a + ((b - a) >> 1);
        if ((long)cb[m] <= c) a = m;
        else b = m;
    }
    long s1 = start[a + 1];
    s1 = s1 > M ? M : s1;
    const long j0 = (long)start[a] + (c - (long)cb[a]) * BX_CHUNK;
    const long j1 = j0 + BX_CHUNK < s1 ? j0 + BX_CHUNK : s1;
    out->k = a;
    out->j0 = j0;
    out->j1 = j1;
    return j0 < j1;                          // (always: the id has ceil(n / BX_CHUNK) chunks)
}

// the coordinates of this lane's BX_TURNS members of the chunk; `live` turns first
__device__ __forceinline__ void bx_load(const float* __restrict__ xyz, long M, const uint32_t* __restrict__ idx,
                                        const BoxChunk& ch, int lane, float (&p)[BX_TURNS][3]) {
    long i[BX_TURNS];
#pragma unroll
    for (int t = 0; t < BX_TURNS; ++t) {
        const long j = ch.j0 + t * 64 + lane;
        const long v = idx[j < ch.j1 ? j : ch.j0];
        i[t] = v < M ? v : 0;                // (never: idx is a permutation)
    }
#pragma unroll
    for (int t = 0; t < BX_TURNS; ++t) {
        const float* q = xyz + i[t] * 3;
        p[t][0] = q[0]; p[t][1] = q[1]; p[t][2] = q[2];
    }
}

// one wavefront per chunk.  kCov: the six products of the differences from the id's mean; otherwise the three coordinates
template <bool kCov>
__global__ __launch_bounds__(GR_THREADS) void bx_partial(const float* __restrict__ xyz, long M, long I, long parts,
                                                          const uint32_t* __restrict__ idx,
                                                          const uint32_t* __restrict__ start,
                                                          const uint32_t* __restrict__ cb, const BoxState* __restrict__ st,
                                                          const double* __restrict__ mean, double* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const long c = (long)blockIdx.x * BX_WAVES + (threadIdx.x >> 6);
    BoxChunk ch;
    if (!bx_chunk(c, M, I, parts, start, cb, st, &ch)) return;
    float p[BX_TURNS][3];
    bx_load(xyz, M, idx, ch, lane, p);
    constexpr int E = kCov ? 6 : 3;
    double acc[E];
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.0;
    double mx = 0.0, my = 0.0, mz = 0.0;
    if (kCov) { mx = mean[ch.k * 3]; my = mean[ch.k * 3 + 1]; mz = mean[ch.k * 3 + 2]; }
#pragma unroll
    for (int t = 0; t < BX_TURNS; ++t) {
        const bool live = ch.j0 + t * 64 + lane < ch.j1;       // selects, not branches: the loads above stay in flight together
        double v[E];
        if (kCov) {
            const double dx = (double)p[t][0] - mx, dy = (double)p[t][1] - my, dz = (double)p[t][2] - mz;
            v[0] = dx * dx; v[1] = dx * dy; v[2] = dx * dz;
            v[3 % E] = dy * dy; v[4 % E] = dy * dz; v[5 % E] = dz * dz;
        } else {
            v[0] = (double)p[t][0]; v[1] = (double)p[t][1]; v[2] = (double)p[t][2];
        }
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] = live ? acc[e] + v[e] : acc[e];
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const double s = fs_fold64(acc[e]);
        if (lane == 0) part[c * 6 + e] = s;
    }
}

// one wavefront per id: its chunk sums by the same rule, divided by the count
template <bool kCov>
__global__ __launch_bounds__(GR_THREADS) void bx_fold(long I, long parts, const uint32_t* __restrict__ start,
                                                       const uint32_t* __restrict__ cb, const double* __restrict__ part,
                                                       double* __restrict__ out, double* __restrict__ copy) {
    constexpr int E = kCov ? 6 : 3;
    const int lane = threadIdx.x & 63;
    const long k = (long)blockIdx.x * BX_WAVES + (threadIdx.x >> 6);
    if (k >= I) return;                      // wavefront-uniform
    const long c0 = cb[k];
    long c1 = cb[k + 1];
    c1 = c1 > parts ? parts : c1;
    const uint32_t s0 = start[k], s1 = start[k + 1];
    const double n = s1 > s0 ? (double)(s1 - s0) : 1.0;
    double acc[E];
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.0;
    for (long c = c0 + lane; c < c1; c += 64)
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] += part[c * 6 + e];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const double s = fs_fold64(acc[e]) / n;
        if (lane == 0) {
            out[k * E + e] = s;
            if (copy) copy[k * E + e] = s;
        }
    }
}

__device__ __forceinline__ void bx_unit(double (&v)[3]) {
    const double n = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    v[0] = v[0] / n; v[1] = v[1] / n; v[2] = v[2] / n;
}

// the component of largest magnitude, ties to the lowest index, is made positive
__device__ __forceinline__ void bx_positive(double (&v)[3]) {
    double big = v[0];
    if (fabs(v[1]) > fabs(big)) big = v[1];
    if (fabs(v[2]) > fabs(big)) big = v[2];
    const bool neg = big < 0.0;
    v[0] = neg ? -v[0] : v[0]; v[1] = neg ? -v[1] : v[1]; v[2] = neg ? -v[2] : v[2];
}

// one lane per id
__global__ __launch_bounds__(GR_THREADS) void bx_axes(long I, const double* __restrict__ cov, double* __restrict__ axes,
                                                       double* __restrict__ lam_out) {
    const long k = (long)blockIdx.x * GR_THREADS + threadIdx.x;
    if (k >= I) return;
    const double* c = cov + k * 6;
    double a00 = c[0], a01 = c[1], a02 = c[2], a11 = c[3], a12 = c[4], a22 = c[5];
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
    for (int sweep = 0; sweep < 6; ++sweep) {
        nr_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);      // (0, 1), r = 2
        nr_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);      // (0, 2), r = 1
        nr_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);      // (1, 2), r = 0
    }
    // the place of every eigenvalue in descending order, ties to the lower index
    const double lam[3] = {a00, a11, a22};
    const double col[3][3] = {{v00, v10, v20}, {v01, v11, v21}, {v02, v12, v22}};
    const int place[3] = {(a11 > a00) + (a22 > a00), (a00 >= a11) + (a22 > a11), (a00 >= a22) + (a11 >= a22)};
    double ax[3][3] = {}, ls[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (place[i] == a) { ax[a][0] = col[i][0]; ax[a][1] = col[i][1]; ax[a][2] = col[i][2]; ls[a] = lam[i]; }
    // orthonormal once more (the rotations leave V so to a few ulps only): unit, Gram-Schmidt, unit, cross, unit
    bx_unit(ax[0]);
    bx_positive(ax[0]);
    const double s = (ax[0][0] * ax[1][0] + ax[0][1] * ax[1][1]) + ax[0][2] * ax[1][2];
#pragma unroll
    for (int x = 0; x < 3; ++x) ax[1][x] = ax[1][x] - s * ax[0][x];
    bx_unit(ax[1]);
    bx_positive(ax[1]);
    ax[2][0] = ax[0][1] * ax[1][2] - ax[0][2] * ax[1][1];
    ax[2][1] = ax[0][2] * ax[1][0] - ax[0][0] * ax[1][2];
    ax[2][2] = ax[0][0] * ax[1][1] - ax[0][1] * ax[1][0];
    bx_unit(ax[2]);
    double* o = axes + k * 9;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        o[a * 3] = ax[a][0]; o[a * 3 + 1] = ax[a][1]; o[a * 3 + 2] = ax[a][2];
        lam_out[k * 3 + a] = ls[a];
    }
}

// one wavefront per chunk: min / max of the three projections (fp64, into part) and of the coordinates (fp32, into box)
__global__ __launch_bounds__(GR_THREADS) void bx_project(const float* __restrict__ xyz, long M, long I, long parts,
                                                          const uint32_t* __restrict__ idx,
                                                          const uint32_t* __restrict__ start,
                                                          const uint32_t* __restrict__ cb, const BoxState* __restrict__ st,
                                                          const double* __restrict__ mean, const double* __restrict__ axes,
                                                          double* __restrict__ part, float* __restrict__ box) {
    const int lane = threadIdx.x & 63;
    const long c = (long)blockIdx.x * BX_WAVES + (threadIdx.x >> 6);
    BoxChunk ch;
    if (!bx_chunk(c, M, I, parts, start, cb, st, &ch)) return;
    float p[BX_TURNS][3];
    bx_load(xyz, M, idx, ch, lane, p);
    const double mx = mean[ch.k * 3], my = mean[ch.k * 3 + 1], mz = mean[ch.k * 3 + 2];
    double ax[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) ax[e] = axes[ch.k * 9 + e];
    double tlo[3] = {INFINITY, INFINITY, INFINITY}, thi[3] = {-INFINITY, -INFINITY, -INFINITY};
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int t = 0; t < BX_TURNS; ++t) {
        const bool live = ch.j0 + t * 64 + lane < ch.j1;
        const double dx = (double)p[t][0] - mx, dy = (double)p[t][1] - my, dz = (double)p[t][2] - mz;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double v = (dx * ax[a * 3] + dy * ax[a * 3 + 1]) + dz * ax[a * 3 + 2];
            tlo[a] = live ? fmin(tlo[a], v) : tlo[a]; thi[a] = live ? fmax(thi[a], v) : thi[a];
            lo[a] = live ? fminf(lo[a], p[t][a]) : lo[a]; hi[a] = live ? fmaxf(hi[a], p[t][a]) : hi[a];
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        for (int h = 32; h >= 1; h >>= 1) {
            tlo[a] = fmin(tlo[a], __shfl_xor(tlo[a], h, 64)); thi[a] = fmax(thi[a], __shfl_xor(thi[a], h, 64));
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], h, 64)); hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], h, 64));
        }
        if (lane == 0) {
            part[c * 6 + a] = tlo[a]; part[c * 6 + 3 + a] = thi[a];
            box[c * 6 + a] = lo[a]; box[c * 6 + 3 + a] = hi[a];
        }
    }
}

// one wavefront per id
__global__ __launch_bounds__(GR_THREADS) void bx_final(long I, long parts, const uint32_t* __restrict__ start,
                                                        const uint32_t* __restrict__ cb, const double* __restrict__ mean,
                                                        const double* __restrict__ axes, const double* __restrict__ lam,
                                                        const double* __restrict__ part, const float* __restrict__ box,
                                                        int32_t* __restrict__ count_out, float* __restrict__ lo_out,
                                                        float* __restrict__ hi_out, float* __restrict__ center_out,
                                                        float* __restrict__ axes_out, float* __restrict__ extent_out,
                                                        float* __restrict__ lam_out) {
    const int lane = threadIdx.x & 63;
    const long k = (long)blockIdx.x * BX_WAVES + (threadIdx.x >> 6);
    if (k >= I) return;                      // wavefront-uniform
    const long c0 = cb[k];
    long c1 = cb[k + 1];
    c1 = c1 > parts ? parts : c1;
    const uint32_t s0 = start[k], s1 = start[k + 1];
    const uint32_t n = s1 > s0 ? s1 - s0 : 0u;
    double tlo[3] = {INFINITY, INFINITY, INFINITY}, thi[3] = {-INFINITY, -INFINITY, -INFINITY};
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long c = c0 + lane; c < c1; c += 64)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            tlo[a] = fmin(tlo[a], part[c * 6 + a]); thi[a] = fmax(thi[a], part[c * 6 + 3 + a]);
            lo[a] = fminf(lo[a], box[c * 6 + a]); hi[a] = fmaxf(hi[a], box[c * 6 + 3 + a]);
        }
#pragma unroll
    for (int a = 0; a < 3; ++a)
        for (int h = 32; h >= 1; h >>= 1) {
            tlo[a] = fmin(tlo[a], __shfl_xor(tlo[a], h, 64)); thi[a] = fmax(thi[a], __shfl_xor(thi[a], h, 64));
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], h, 64)); hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], h, 64));
        }
    if (lane != 0) return;
    count_out[k] = (int32_t)n;
    double ext[3], half[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (n == 0u) tlo[a] = 0.0, thi[a] = 0.0;     // an id without members: extent and center 0, lo / hi stay +-inf
        ext[a] = thi[a] - tlo[a];
        half[a] = (tlo[a] + thi[a]) * 0.5;
        lo_out[k * 3 + a] = lo[a];
        hi_out[k * 3 + a] = hi[a];
        extent_out[k * 3 + a] = (float)ext[a];
        lam_out[k * 3 + a] = (float)lam[k * 3 + a];
    }
    const double* ax = axes + k * 9;
#pragma unroll
    for (int x = 0; x < 3; ++x)
        center_out[k * 3 + x] = (float)(((mean[k * 3 + x] + ax[x] * half[0]) + ax[3 + x] * half[1]) + ax[6 + x] * half[2]);
#pragma unroll
    for (int e = 0; e < 9; ++e) axes_out[k * 9 + e] = (float)ax[e];
}

int boxes_check(const char* who, int64_t M, int64_t I, const void* ws, int64_t ws_bytes) {
    RL_REQUIRE(M > 0 && M < 0x7fffffffLL, RL_ERR_ARGS, "%s: M=%lld outside 1 .. 2^31-2", who, (long long)M);
    RL_REQUIRE(I > 0 && I < 0x7fffffffLL, RL_ERR_ARGS, "%s: I=%lld ids, outside 1 .. 2^31-2", who, (long long)I);
    return rl_ws_check(who, ws, ws_bytes, rl_boxes_workspace_bytes(M, I));
}

}  // namespace

extern "C" int64_t rl_boxes_workspace_bytes(int64_t M, int64_t I) {
    if (M <= 0 || M >= 0x7fffffffLL || I <= 0 || I >= 0x7fffffffLL) return 0;
    return (int64_t)boxes_layout(M, I).bytes;
}

extern "C" int rl_boxes_sort(const void* ids, int id_bytes, int64_t M, int64_t I, void* ws, int64_t ws_bytes, void* stream) {
    RL_REQUIRE(id_bytes == 4 || id_bytes == 8, RL_ERR_ARGS, "rl_boxes_sort: ids of %d bytes, int32 or int64 expected", id_bytes);
    int rc = boxes_check("rl_boxes_sort", M, I, ws, ws_bytes);
    if (rc) return rc;
    RL_REQUIRE(ids, RL_ERR_ARGS, "rl_boxes_sort: null pointer");
    hipStream_t sm = (hipStream_t)stream;
    const BoxLayout L = boxes_layout(M, I);
    const RadixBufs sort = radix_bufs(ws, L.sort);
    uint32_t* start = rl_at<uint32_t>(ws, L.off_start);
    uint32_t* cb = rl_at<uint32_t>(ws, L.off_cb);
    const int passes = grid_passes(rl_bits_of(I));
    hipLaunchKernelGGL(bx_keys, dim3(rl_cdiv(M, GR_THREADS)), dim3(GR_THREADS), 0, sm, ids, id_bytes == 8, (long)M, (long)I,
                       sort.keys[passes & 1]);
    RL_LAUNCH_CHECK("rl_boxes_sort (keys)");
    rc = radix_sort("rl_boxes_sort", sort, (long)M, passes, sm);
    if (rc) return rc;
    hipLaunchKernelGGL(bx_starts, dim3(rl_cdiv(I + 1, GR_THREADS)), dim3(GR_THREADS), 0, sm, sort.keys[0], (long)M, (long)I, start);
    RL_LAUNCH_CHECK("rl_boxes_sort (starts)");
    hipLaunchKernelGGL(bx_counts, dim3(rl_cdiv(I, GR_THREADS)), dim3(GR_THREADS), 0, sm, start, (long)I, cb);
    RL_LAUNCH_CHECK("rl_boxes_sort (counts)");
    hipLaunchKernelGGL(bx_scan, dim3(1), dim3(GR_THREADS), 0, sm, cb, (long)I, (BoxState*)ws);
    rl_note_kernel("bx_scan");
    RL_LAUNCH_CHECK("rl_boxes_sort (scan)");
    return RL_OK;
}

extern "C" int rl_boxes_moments(const float* xyz, int64_t M, int64_t I, double* mean_out, double* cov_out, void* ws,
                                int64_t ws_bytes, void* stream) {
    int rc = boxes_check("rl_boxes_moments", M, I, ws, ws_bytes);
    if (rc) return rc;
    RL_REQUIRE(xyz, RL_ERR_ARGS, "rl_boxes_moments: null pointer");
    hipStream_t sm = (hipStream_t)stream;
    const BoxLayout L = boxes_layout(M, I);
    const BoxState* st = (const BoxState*)ws;
    const uint32_t* idx = rl_at<const uint32_t>(ws, L.sort.off_idx[0]);
    const uint32_t* start = rl_at<const uint32_t>(ws, L.off_start);
    const uint32_t* cb = rl_at<const uint32_t>(ws, L.off_cb);
    double* mean = rl_at<double>(ws, L.off_mean);
    double* cov = rl_at<double>(ws, L.off_cov);
    double* part = rl_at<double>(ws, L.off_part);
    const dim3 block(GR_THREADS), per_chunk(rl_cdiv(L.parts, BX_WAVES)), per_id(rl_cdiv(I, BX_WAVES));
    hipLaunchKernelGGL(bx_partial<false>, per_chunk, block, 0, sm, xyz, (long)M, (long)I, L.parts, idx, start, cb, st,
                       (const double*)nullptr, part);
    RL_LAUNCH_CHECK("rl_boxes_moments (mean partial)");
    hipLaunchKernelGGL(bx_fold<false>, per_id, block, 0, sm, (long)I, L.parts, start, cb, (const double*)part, mean, mean_out);
    RL_LAUNCH_CHECK("rl_boxes_moments (mean)");
    hipLaunchKernelGGL(bx_partial<true>, per_chunk, block, 0, sm, xyz, (long)M, (long)I, L.parts, idx, start, cb, st,
                       (const double*)mean, part);
    RL_LAUNCH_CHECK("rl_boxes_moments (covariance partial)");
    hipLaunchKernelGGL(bx_fold<true>, per_id, block, 0, sm, (long)I, L.parts, start, cb, (const double*)part, cov, cov_out);
    rl_note_kernel("bx_fold");
    RL_LAUNCH_CHECK("rl_boxes_moments (covariance)");
    return RL_OK;
}

extern "C" int rl_boxes_fit(const float* xyz, int64_t M, int64_t I, int32_t* count_out, float* lo_out, float* hi_out,
                            float* center_out, float* axes_out, float* extent_out, float* eigenvalues_out, void* ws,
                            int64_t ws_bytes, void* stream) {
    int rc = boxes_check("rl_boxes_fit", M, I, ws, ws_bytes);
    if (rc) return rc;
    RL_REQUIRE(xyz && count_out && lo_out && hi_out && center_out && axes_out && extent_out && eigenvalues_out, RL_ERR_ARGS,
               "rl_boxes_fit: null pointer");
    hipStream_t sm = (hipStream_t)stream;
    const BoxLayout L = boxes_layout(M, I);
    const BoxState* st = (const BoxState*)ws;
    const uint32_t* idx = rl_at<const uint32_t>(ws, L.sort.off_idx[0]);
    const uint32_t* start = rl_at<const uint32_t>(ws, L.off_start);
    const uint32_t* cb = rl_at<const uint32_t>(ws, L.off_cb);
    const double* mean = rl_at<const double>(ws, L.off_mean);
    const double* cov = rl_at<const double>(ws, L.off_cov);
    double* axes = rl_at<double>(ws, L.off_axes);
    double* lam = rl_at<double>(ws, L.off_lam);
    double* part = rl_at<double>(ws, L.off_part);
    float* box = rl_at<float>(ws, L.off_box);
    const dim3 block(GR_THREADS);
    hipLaunchKernelGGL(bx_axes, dim3(rl_cdiv(I, GR_THREADS)), block, 0, sm, (long)I, cov, axes, lam);
    RL_LAUNCH_CHECK("rl_boxes_fit (axes)");
    hipLaunchKernelGGL(bx_project, dim3(rl_cdiv(L.parts, BX_WAVES)), block, 0, sm, xyz, (long)M, (long)I, L.parts, idx, start,
                       cb, st, mean, (const double*)axes, part, box);
    RL_LAUNCH_CHECK("rl_boxes_fit (project)");
    hipLaunchKernelGGL(bx_final, dim3(rl_cdiv(I, BX_WAVES)), block, 0, sm, (long)I, L.parts, start, cb, mean,
                       (const double*)axes, (const double*)lam, (const double*)part, (const float*)box, count_out, lo_out,
                       hi_out, center_out, axes_out, extent_out, eigenvalues_out);
    rl_note_kernel("bx_final");
    RL_LAUNCH_CHECK("rl_boxes_fit (final)");
    return RL_OK;
}
