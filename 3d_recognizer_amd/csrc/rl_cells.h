// What the clients of rl_radix.h's sort share on top of it.  grid.hip, cluster.hip and keypoints.hip: the box of a cloud and the cell grid over
// it (origin, dims, the key of a point - the fixed fp32 expressions of randlanet/utils/grid.py), the front of their workspaces
// (cells_layout) and the heads of a sorted key array (runs of equal keys -> segment numbers and segment starts, grid_heads).
// pairs.hip: is_head and head_count.  boxes.hip: the sort alone.  See grid.hip's header comment for the launches.  Integer work
// and fixed fp32 expressions only; no workgroup waits for another one.
#pragma once
#include "rl_common.h"
#include "rl_radix.h"

#include <math.h>

namespace {

constexpr int GR_WAVES = GR_THREADS / 64;
constexpr int GR_PARTS = 1024;           // workgroups of box_partial
constexpr float GR_DIM_CAP = 4.0e18f;    // dims are clamped here before the conversion to int64 (the caller refuses >= 2^21)

struct GridState {
    float origin[3];
    float cell;
    int64_t dims[3];
    int64_t V;
    int64_t M;
    int64_t pad[2];
};

__global__ __launch_bounds__(GR_THREADS) void grid_box_partial(const float* __restrict__ cloud, long M, int dim,
                                                                float* __restrict__ box) {
    __shared__ float red[6][GR_WAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long i = (long)blockIdx.x * GR_THREADS + t; i < M; i += (long)gridDim.x * GR_THREADS) {
        const float* q = cloud + i * dim;
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], q[a]); hi[a] = fmaxf(hi[a], q[a]); }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        for (int o = 32; o >= 1; o >>= 1) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], o, 64));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o, 64));
        }
        if (lane == 0) { red[a][wave] = lo[a]; red[3 + a][wave] = hi[a]; }
    }
    __syncthreads();
    if (t < 6) {
        float v = red[t][0];
        for (int w = 1; w < GR_WAVES; ++w) v = t < 3 ? fminf(v, red[t][w]) : fmaxf(v, red[t][w]);
        box[(long)blockIdx.x * 6 + t] = v;
    }
}

// one workgroup: the box from the partial boxes (min / max: any order gives the same bits), then origin and dims
__global__ __launch_bounds__(GR_THREADS) void grid_box_final(const float* __restrict__ box, int parts, float cell, long M,
                                                              GridState* __restrict__ st, int64_t* __restrict__ dims_out) {
    __shared__ float red[6][GR_THREADS];
    const int t = threadIdx.x;
    float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int j = t; j < parts; j += GR_THREADS)
#pragma unroll
        for (int a = 0; a < 6; ++a) v[a] = a < 3 ? fminf(v[a], box[j * 6 + a]) : fmaxf(v[a], box[j * 6 + a]);
#pragma unroll
    for (int a = 0; a < 6; ++a) red[a][t] = v[a];
    __syncthreads();
    if (t < 3) {
        float lo = red[t][0], hi = red[3 + t][0];
        for (int j = 1; j < GR_THREADS; ++j) { lo = fminf(lo, red[t][j]); hi = fmaxf(hi, red[3 + t][j]); }
        const float o = __fmul_rn(floorf(__fdiv_rn(lo, cell)), cell);
        float d = __fadd_rn(floorf(__fdiv_rn(__fsub_rn(hi, o), cell)), 1.f);
        d = fminf(fmaxf(d, 1.f), GR_DIM_CAP);           // (o can round to just above min: the cell index is clamped at 0)
        st->origin[t] = o;
        st->dims[t] = (int64_t)d;
        dims_out[t] = (int64_t)d;
        if (t == 0) st->cell = cell, st->M = M, st->V = 0;
    }
}

// the two launches of the box: parts partial boxes into box (GR_PARTS * 6 floats), then origin and dims into st and dims_out
inline long grid_box_parts(long M) {
    const long parts = (M + 8 * GR_THREADS - 1) / (8 * GR_THREADS);
    return parts > GR_PARTS ? GR_PARTS : parts;
}

// the cell of point p per axis: v = max(floor((p - o) / c), 0) in fp32 with a correctly rounded division, below dims
__device__ __forceinline__ void grid_cell_of(const float* __restrict__ p, const GridState* __restrict__ st, int64_t v[3]) {
    const float c = st->cell;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float f = floorf(__fdiv_rn(__fsub_rn(p[a], st->origin[a]), c));
        const int64_t d = st->dims[a];
        int64_t q = (int64_t)fminf(fmaxf(f, 0.f), GR_DIM_CAP);
        v[a] = q < d ? q : d - 1;                        // (never taken: floor((p - o) / c) is monotone in p and p <= max)
    }
}

__device__ __forceinline__ uint64_t grid_cell_key(const float* __restrict__ p, const GridState* __restrict__ st) {
    int64_t v[3];
    grid_cell_of(p, st, v);
    return (uint64_t)((v[2] * st->dims[1] + v[1]) * st->dims[0] + v[0]);
}

__device__ __forceinline__ bool is_head(const uint64_t* __restrict__ keys, long j) {
    return j == 0 || keys[j] != keys[j - 1];
}

// the first position of the sorted keys whose key is >= k (cluster.hip and keypoints.hip find a row of cells by it)
__device__ __forceinline__ long grid_lower_bound(const uint64_t* __restrict__ keys, long M, uint64_t k) {
    long a = 0, b = M;
    while (a < b) {
        const long m = a + ((b - a) >> 1);
        if (keys[m] < k) a = m + 1;
        else b = m;
    }
    return a;
}

// The 27 cells around the cell of `key` as rows of contiguous keys, in ascending key order: row(klo, khi) per row that lies
// inside the grid, until one returns false (keypoints.hip and cluster.hip's density rule walk them: the rows after the own
// one too, which the union never scans).
template <class Row>
__device__ __forceinline__ void grid_rows(uint64_t key, const GridState* __restrict__ st, Row&& row) {
    const int64_t dx = st->dims[0], dy = st->dims[1], dz = st->dims[2];
    const int64_t vx = (int64_t)(key % (uint64_t)dx), t = (int64_t)(key / (uint64_t)dx), vy = t % dy, vz = t / dy;
    const int64_t x0 = vx > 0 ? vx - 1 : 0, x1 = vx + 1 < dx ? vx + 1 : dx - 1;
    for (int64_t z = vz - 1; z <= vz + 1; ++z) {
        if (z < 0 || z >= dz) continue;
        for (int64_t y = vy - 1; y <= vy + 1; ++y) {
            if (y < 0 || y >= dy) continue;
            const uint64_t base = (uint64_t)((z * dy + y) * dx);
            if (!row(base + (uint64_t)x0, base + (uint64_t)x1)) return;
        }
    }
}

// v of a wavefront-uniform lane (v_readlane_b32: no trip through the LDS crossbar)
__device__ __forceinline__ float grid_lane(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// one wavefront per chunk
__global__ __launch_bounds__(64) void grid_head_count(const uint64_t* __restrict__ keys, long M, long chunk,
                                                       uint32_t* __restrict__ cnt) {
    const int lane = threadIdx.x;
    const long i0 = (long)blockIdx.x * chunk;
    const long i1 = min(M, i0 + chunk);
    uint32_t n = 0;
    for (long t0 = i0; t0 < i1; t0 += 64) {
        const long j = t0 + lane;
        n += (uint32_t)__popcll(__ballot(j < i1 && is_head(keys, j)));
    }
    if (lane == 0) cnt[blockIdx.x] = n;
}

__global__ __launch_bounds__(GR_THREADS) void grid_head_scan(uint32_t* __restrict__ cnt, int chunks, long M,
                                                              GridState* __restrict__ st, int64_t* __restrict__ V_out,
                                                              uint32_t* __restrict__ start) {
    const uint32_t V = block_exclusive_scan(cnt, chunks);
    if (threadIdx.x == 0) {
        st->V = (int64_t)V;
        V_out[0] = (int64_t)V;
        start[V] = (uint32_t)M;          // V <= M: start holds M + 1 entries
    }
}

__global__ __launch_bounds__(64) void grid_head_write(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx,
                                                       long M, long chunk, const uint32_t* __restrict__ cnt,
                                                       int32_t* __restrict__ inverse, uint32_t* __restrict__ start) {
    const int lane = threadIdx.x;
    const unsigned long long upto = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull;
    const long i0 = (long)blockIdx.x * chunk;
    const long i1 = min(M, i0 + chunk);
    uint32_t run = cnt[blockIdx.x];       // heads before this chunk
    for (long t0 = i0; t0 < i1; t0 += 64) {
        const long j = t0 + lane;
        const bool live = j < i1;
        const bool head = live && is_head(keys, j);
        const unsigned long long b = __ballot(head);
        if (live) {
            const uint32_t seg = run + (uint32_t)__popcll(b & upto) - 1u;     // (position 0 is a head: never below 0)
            const uint32_t i = idx[j];
            if ((long)i < M) inverse[i] = (int32_t)seg;
            if (head) start[seg] = (uint32_t)j;
        }
        run += (uint32_t)__popcll(b);
    }
}

// The front of grid.hip's and cluster.hip's workspaces: the GridState at offset 0, the partial boxes, the sort, and the heads'
// cnt (heads per chunk, then their prefix) and start (M + 1 entries); `bytes` is where this front ends - grid.hip's workspace
struct CellsLayout {
    RadixLayout sort;
    size_t off_box, off_cnt, off_start, bytes;
};

inline CellsLayout cells_layout(RlCarve& c, long M) {
    CellsLayout L;
    c.take(sizeof(GridState));
    L.off_box = c.take((size_t)GR_PARTS * 6 * sizeof(float));
    L.sort = radix_layout(c, M);
    L.off_cnt = c.take((size_t)L.sort.chunks * sizeof(uint32_t));
    L.off_start = c.take((size_t)(M + 1) * sizeof(uint32_t));
    L.bytes = c.at;
    return L;
}

// the heads of the sorted keys in buffer 0: their number into st->V and V_out, the segment of every point into inverse
inline int grid_heads(const char* who, const RadixBufs& b, long M, GridState* st, int64_t* V_out, int32_t* inverse,
                      uint32_t* cnt, uint32_t* start, hipStream_t sm) {
    char name[96];
    hipLaunchKernelGGL(grid_head_count, dim3(b.chunks), dim3(64), 0, sm, b.keys[0], M, b.chunk, cnt);
    snprintf(name, sizeof(name), "%s (head count)", who);
    RL_LAUNCH_CHECK(name);
    hipLaunchKernelGGL(grid_head_scan, dim3(1), dim3(GR_THREADS), 0, sm, cnt, b.chunks, M, st, V_out, start);
    snprintf(name, sizeof(name), "%s (head scan)", who);
    RL_LAUNCH_CHECK(name);
    hipLaunchKernelGGL(grid_head_write, dim3(b.chunks), dim3(64), 0, sm, b.keys[0], b.idx[0], M, b.chunk, cnt, inverse, start);
    snprintf(name, sizeof(name), "%s (head write)", who);
    RL_LAUNCH_CHECK(name);
    return RL_OK;
}

}  // namespace
