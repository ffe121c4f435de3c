// TSDF fusion of depth frames (rl_tsdf_*; the numpy twin and the contract are randlanet/utils/tsdf.py): a dense truncated signed
// distance volume of nx * ny * nz voxels, x fastest, as two fp32 arrays - tsdf and weight.  A frame is integrated by projecting
// every voxel centre into it (projective distance along the camera's z axis, the nearest pixel, a running mean with a capped
// weight); the surface is read out as the zero crossings on the edges between neighbouring voxels, in ascending edge order.
// -ffp-contract=off keeps every operation a correctly rounded fp32 one, in the order of the twin, so the results equal the
// twin's bit for bit.
//
//   rl_tsdf_integrate  ts_integrate  one launch: a lane per run of 4 voxels, no workspace
//   rl_tsdf_count      ts_count      one wavefront per chunk of 1024 voxels: the emitting edges of its voxels (0 .. 3 each)
//                      ts_scan       one workgroup: the exclusive prefix of those counts, and M
//   rl_tsdf_points     ts_write      one wavefront per chunk: the edges again, and their points in order
// No atomics at all, and no workgroup waits for another one.
//
// Mapping and why.  The volume is 8 bytes in per voxel and 8 bytes out per updated voxel, against about 60 fp32 operations and
// one gathered 2-byte pixel: a stream, so the accesses are made wide.  A lane takes a run of 4 consecutive voxels of the linear
// array - one 16-byte load per array where the run is aligned and inside the volume, element by element otherwise (the tail, an
// array that is only 4-byte aligned) - and consecutive lanes consecutive runs, which lie along x: neighbouring voxels project
// to neighbouring pixels, so a wavefront's gathers fall into a few lines of the frame.  (i, j, k) of a run's first voxel come
// from two divisions, the others by carrying.  A run is stored only when one of its voxels changed, so a frame that sees a
// tenth of the volume writes a tenth of it.
// The extraction is depth.hip's count / scan / write compaction over edges instead of pixels: the order inside a turn of 256
// voxels comes from the lanes' popcounts (12 edges a lane) and one wavefront prefix.  The neighbours' values (+1, +nx, +nx*ny)
// are loaded only by the lanes that hold a voxel of enough weight - in a volume that is mostly unseen, few - and hit lines that
// the next lanes or chunks read anyway.
#include "rl_radix.h"

#include <math.h>

namespace {

constexpr int TS_LANES = 64;
constexpr int TS_RUN = 4;                          // voxels of a lane per turn: 16 bytes per array
constexpr int TS_TURN = TS_LANES * TS_RUN;
constexpr int TS_TURNS = 4;
constexpr long TS_CHUNK = (long)TS_TURN * TS_TURNS;
constexpr int TS_THREADS = 256;                    // ts_integrate: runs per workgroup

struct TsVolume {
    long V;                  // voxels
    uint32_t nx, ny, nz;
    float ox, oy, oz, voxel;
};

struct TsFrame {
    const uint16_t* depth;
    int W, H;
    float Wf, Hf;
    float fx, fy, ppx, ppy, scale;
    float z_lo, z_hi;
    float trunc, neg_trunc, max_weight;
    float r[9], t[3];        // world to camera
};

inline long ts_chunks(long V) { return (V + TS_CHUNK - 1) / TS_CHUNK; }

// p[i0 .. i0 + 3]; an entry at or beyond V reads as entry V - 1 (its value is never used).  One 16-byte load where the run lies
// inside and is aligned
__device__ __forceinline__ void ts_read4(const float* __restrict__ p, long i0, long V, float v[TS_RUN]) {
    if (i0 + TS_RUN <= V && ((uintptr_t)(p + i0) & 15) == 0) {
        const float4 w = *reinterpret_cast<const float4*>(p + i0);
        v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
        return;
    }
#pragma unroll
    for (int e = 0; e < TS_RUN; ++e) {
        const long i = i0 + e;
        v[e] = p[i < V ? i : V - 1];
    }
}

// the entries of the run whose bit in `mask` is set are written; where the run lies inside and is aligned the whole run is,
// by one 16-byte store (the other entries hold what was loaded)
__device__ __forceinline__ void ts_write4(float* __restrict__ p, long i0, long V, const float v[TS_RUN], uint32_t mask) {
    if (i0 + TS_RUN <= V && ((uintptr_t)(p + i0) & 15) == 0) {
        *reinterpret_cast<float4*>(p + i0) = make_float4(v[0], v[1], v[2], v[3]);
        return;
    }
#pragma unroll
    for (int e = 0; e < TS_RUN; ++e) {
        const long i = i0 + e;
        if (((mask >> e) & 1u) && i < V) p[i] = v[e];
    }
}

// (i, j, k) of voxel n, and the step to voxel n + 1
struct TsCell {
    uint32_t i, j, k;
};
__device__ __forceinline__ TsCell ts_cell(uint32_t n, const TsVolume& g) {
    const uint32_t row = n / g.nx;
    TsCell c;
    c.i = n - row * g.nx;
    c.k = row / g.ny;
    c.j = row - c.k * g.ny;
    return c;
}
__device__ __forceinline__ void ts_next(TsCell& c, const TsVolume& g) {
    if (++c.i == g.nx) {
        c.i = 0u;
        if (++c.j == g.ny) c.j = 0u, ++c.k;
    }
}
__device__ __forceinline__ float ts_centre(uint32_t i, float o, float voxel) { return o + ((float)i + 0.5f) * voxel; }

// one voxel against the frame: true when it is updated, t and w then hold the new values
__device__ __forceinline__ bool ts_update(const TsFrame& f, float cx, float cy, float cz, float& t, float& w) {
    const float qz = ((f.r[6] * cx + f.r[7] * cy) + f.r[8] * cz) + f.t[2];
    if (!(qz > 0.f)) return false;
    const float qx = ((f.r[0] * cx + f.r[1] * cy) + f.r[2] * cz) + f.t[0];
    const float qy = ((f.r[3] * cx + f.r[4] * cy) + f.r[5] * cz) + f.t[1];
    const float uf = (__fdiv_rn(qx, qz) * f.fx + f.ppx) + 0.5f;
    const float vf = (__fdiv_rn(qy, qz) * f.fy + f.ppy) + 0.5f;
    if (!(uf >= 0.f && uf < f.Wf && vf >= 0.f && vf < f.Hf)) return false;       // (a NaN or an infinity fails it)
    const int u = (int)uf, v = (int)vf;                                          // 0 <= u < W, 0 <= v < H by the test above
    const uint32_t d = f.depth[(long)v * f.W + u];
    if (d == 0u) return false;
    const float z = (float)d * f.scale;
    if (!(f.z_lo < z && z < f.z_hi)) return false;
    const float sdf = z - qz;
    if (sdf < f.neg_trunc) return false;
    float s = __fdiv_rn(sdf, f.trunc);
    s = s > 1.f ? 1.f : s;
    const float w1 = w + 1.f;
    t = __fdiv_rn(t * w + s, w1);
    w = w1 > f.max_weight ? f.max_weight : w1;
    return true;
}

__global__ __launch_bounds__(TS_THREADS) void ts_integrate(const TsVolume g, const TsFrame f, float* __restrict__ tsdf,
                                                           float* __restrict__ weight) {
    const long i0 = ((long)blockIdx.x * TS_THREADS + threadIdx.x) * TS_RUN;
    if (i0 >= g.V) return;
    float t[TS_RUN], w[TS_RUN];
    ts_read4(tsdf, i0, g.V, t);
    ts_read4(weight, i0, g.V, w);
    TsCell c = ts_cell((uint32_t)i0, g);
    uint32_t changed = 0u;
#pragma unroll
    for (int e = 0; e < TS_RUN; ++e) {
        if (i0 + e < g.V) {
            const float cx = ts_centre(c.i, g.ox, g.voxel), cy = ts_centre(c.j, g.oy, g.voxel), cz = ts_centre(c.k, g.oz, g.voxel);
            changed |= ts_update(f, cx, cy, cz, t[e], w[e]) ? 1u << e : 0u;
        }
        ts_next(c, g);
    }
    if (changed == 0u) return;
    ts_write4(tsdf, i0, g.V, t, changed);
    ts_write4(weight, i0, g.V, w, changed);
}

struct TsSurface {
    const float* tsdf;
    const float* weight;
    float min_weight;
};

// the emitting edges of the run i0 .. i0 + 3: bit 3 * e + a for voxel i0 + e and axis a, which is the order of the output.
// t holds the run's tsdf values and tb[a][e] those of the neighbours where a bit is set
__device__ __forceinline__ uint32_t ts_edges(const TsVolume& g, const TsSurface& s, long i0, float t[TS_RUN],
                                             float tb[3][TS_RUN]) {
    float w[TS_RUN];
    ts_read4(s.weight, i0, g.V, w);
    uint32_t heavy = 0u;
#pragma unroll
    for (int e = 0; e < TS_RUN; ++e) heavy |= (i0 + e < g.V && w[e] >= s.min_weight) ? 1u << e : 0u;
    if (heavy == 0u) return 0u;
    ts_read4(s.tsdf, i0, g.V, t);
    const long step[3] = {1, (long)g.nx, (long)g.nx * g.ny};
    float wb[3][TS_RUN];
    {   // along x the neighbours are the run itself, one further, and one more voxel
        const long last = i0 + TS_RUN < g.V ? i0 + TS_RUN : g.V - 1;
#pragma unroll
        for (int e = 0; e + 1 < TS_RUN; ++e) tb[0][e] = t[e + 1], wb[0][e] = w[e + 1];
        tb[0][TS_RUN - 1] = s.tsdf[last], wb[0][TS_RUN - 1] = s.weight[last];
    }
#pragma unroll
    for (int a = 1; a < 3; ++a) {
        const long b0 = i0 + step[a];
        if (b0 < g.V) {
            ts_read4(s.tsdf, b0, g.V, tb[a]);
            ts_read4(s.weight, b0, g.V, wb[a]);
        } else {
#pragma unroll
            for (int e = 0; e < TS_RUN; ++e) tb[a][e] = 0.f, wb[a][e] = 0.f;     // (no neighbour: never read below)
        }
    }
    TsCell c = ts_cell((uint32_t)i0, g);
    uint32_t mask = 0u;
#pragma unroll
    for (int e = 0; e < TS_RUN; ++e) {
        if ((heavy >> e) & 1u) {
            const bool has[3] = {c.i + 1u < g.nx, c.j + 1u < g.ny, c.k + 1u < g.nz};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const bool emit = has[a] && wb[a][e] >= s.min_weight && ((t[e] < 0.f) != (tb[a][e] < 0.f));
                mask |= emit ? 1u << (3 * e + a) : 0u;
            }
        }
        ts_next(c, g);
    }
    return mask;
}

__device__ __forceinline__ uint32_t ts_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one wavefront per chunk: how many of its edges emit a point
__global__ __launch_bounds__(TS_LANES) void ts_count(const TsVolume g, const TsSurface s, uint32_t* __restrict__ cnt) {
    const int lane = threadIdx.x;
    uint32_t n = 0;
#pragma unroll
    for (int turn = 0; turn < TS_TURNS; ++turn) {
        const long i0 = (long)blockIdx.x * TS_CHUNK + turn * TS_TURN + lane * TS_RUN;
        float t[TS_RUN], tb[3][TS_RUN];
        if (i0 < g.V) n += (uint32_t)__popc(ts_edges(g, s, i0, t, tb));
    }
    n = ts_wave_sum(n);
    if (lane == 0) cnt[blockIdx.x] = n;
}

// one workgroup: M as a 64-bit sum (3 * V may pass 2^32; the 32-bit prefix below is exact whenever M < 2^32, and the caller
// refuses a larger M), then the exclusive prefix of the counts
__global__ __launch_bounds__(GR_THREADS) void ts_scan(uint32_t* __restrict__ cnt, int chunks, int64_t* __restrict__ count_out) {
    __shared__ unsigned long long part[GR_THREADS / 64];
    unsigned long long sum = 0ull;
    for (int j = threadIdx.x; j < chunks; j += GR_THREADS) sum += cnt[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = 0ull;
        for (int k = 0; k < GR_THREADS / 64; ++k) total += part[k];
        count_out[0] = (int64_t)total;
    }
    __syncthreads();
    block_exclusive_scan(cnt, chunks);
}

// one wavefront per chunk: the points of its emitting edges at the rows the prefix gives them
__global__ __launch_bounds__(TS_LANES) void ts_write(const TsVolume g, const TsSurface s, const uint32_t* __restrict__ cnt,
                                                     float* __restrict__ xyz_out, int64_t* __restrict__ edge_out, long capacity) {
    const int lane = threadIdx.x;
    uint32_t run = cnt[blockIdx.x];                     // emitting edges before this chunk
    for (int turn = 0; turn < TS_TURNS; ++turn) {
        const long t0 = (long)blockIdx.x * TS_CHUNK + turn * TS_TURN;
        if (t0 >= g.V) break;                           // wavefront-uniform
        const long i0 = t0 + lane * TS_RUN;
        float t[TS_RUN], tb[3][TS_RUN];
        const uint32_t mask = i0 < g.V ? ts_edges(g, s, i0, t, tb) : 0u;
        const uint32_t mine = (uint32_t)__popc(mask);
        uint32_t incl = mine;                           // emitting edges of the lanes up to this one
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        long row = (long)run + (incl - mine);
        run += __shfl(incl, 63, 64);
        if (mask == 0u) continue;                       // (no shuffle below this line)
        TsCell c = ts_cell((uint32_t)i0, g);
#pragma unroll
        for (int e = 0; e < TS_RUN; ++e) {
            if ((mask >> (3 * e)) & 7u) {
                const float ctr[3] = {ts_centre(c.i, g.ox, g.voxel), ts_centre(c.j, g.oy, g.voxel), ts_centre(c.k, g.oz, g.voxel)};
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    if (!((mask >> (3 * e + a)) & 1u)) continue;
                    const float frac = __fdiv_rn(t[e], t[e] - tb[a][e]);
                    const float moved = ctr[a] + frac * g.voxel;
                    if (row < capacity) {
                        xyz_out[3 * row + 0] = a == 0 ? moved : ctr[0];
                        xyz_out[3 * row + 1] = a == 1 ? moved : ctr[1];
                        xyz_out[3 * row + 2] = a == 2 ? moved : ctr[2];
                        edge_out[row] = 3 * (int64_t)(i0 + e) + a;
                    }
                    ++row;
                }
            }
            ts_next(c, g);
        }
    }
}

inline bool ts_finite(float x) { return x >= -3.402823466e38f && x <= 3.402823466e38f; }

// the refusals every entry shares, and the volume's record
inline int ts_volume(const char* who, const float* tsdf, const float* weight, int nx, int ny, int nz, const float* origin,
                     float voxel, TsVolume* g) {
    RL_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1 && (int64_t)nx * ny < 0x80000000LL && (int64_t)nx * ny * nz < 0x80000000LL,
               RL_ERR_ARGS, "%s: a volume of %d x %d x %d voxels, outside 1 .. 2^31 - 1", who, nx, ny, nz);
    RL_REQUIRE(tsdf && weight && origin, RL_ERR_ARGS, "%s: null pointer", who);
    RL_REQUIRE((((uintptr_t)tsdf | (uintptr_t)weight) & 3) == 0, RL_ERR_ARGS, "%s: a volume that is not 4-byte aligned", who);
    RL_REQUIRE(ts_finite(voxel) && voxel > 0.f, RL_ERR_ARGS, "%s: voxel=%g must be finite and greater than 0", who, voxel);
    RL_REQUIRE(ts_finite(origin[0]) && ts_finite(origin[1]) && ts_finite(origin[2]), RL_ERR_ARGS,
               "%s: origin=(%g, %g, %g) must be finite", who, origin[0], origin[1], origin[2]);
    g->V = (long)nx * ny * nz;
    g->nx = (uint32_t)nx, g->ny = (uint32_t)ny, g->nz = (uint32_t)nz;
    g->ox = origin[0], g->oy = origin[1], g->oz = origin[2], g->voxel = voxel;
    return RL_OK;
}

inline int ts_surface(const char* who, const float* tsdf, const float* weight, int min_weight, TsSurface* s) {
    RL_REQUIRE(min_weight >= 1 && min_weight <= 65535, RL_ERR_ARGS, "%s: min_weight=%d outside 1 .. 65535", who, min_weight);
    s->tsdf = tsdf, s->weight = weight, s->min_weight = (float)min_weight;
    return RL_OK;
}

}  // namespace

extern "C" int64_t rl_tsdf_workspace_bytes(int64_t voxels) {
    if (voxels < 1 || voxels >= 0x80000000LL) return 0;
    RlCarve c;
    c.take((size_t)ts_chunks((long)voxels) * sizeof(uint32_t));
    return (int64_t)c.at;
}

extern "C" int rl_tsdf_integrate(float* tsdf, float* weight, int nx, int ny, int nz, const float* origin, float voxel, float trunc,
                                 int max_weight, const uint16_t* depth, int W, int H, float fx, float fy, float ppx, float ppy,
                                 float depth_scale, float z_lo, float z_hi, const float* world_to_camera, void* stream) {
    const char* who = "rl_tsdf_integrate";
    TsVolume g;
    int rc = ts_volume(who, tsdf, weight, nx, ny, nz, origin, voxel, &g);
    if (rc) return rc;
    RL_REQUIRE(ts_finite(trunc) && trunc > 0.f, RL_ERR_ARGS, "%s: trunc=%g must be finite and greater than 0", who, trunc);
    RL_REQUIRE(max_weight >= 1 && max_weight <= 65535, RL_ERR_ARGS, "%s: max_weight=%d outside 1 .. 65535", who, max_weight);
    RL_REQUIRE(W >= 1 && H >= 1 && W < (1 << 24) && H < (1 << 24) && (int64_t)W * H < 0x80000000LL, RL_ERR_ARGS,
               "%s: a frame of %d x %d pixels, a side outside 1 .. 2^24 - 1 or 2^31 pixels or more", who, H, W);
    RL_REQUIRE(ts_finite(fx) && fx > 0.f && ts_finite(fy) && fy > 0.f && ts_finite(depth_scale) && depth_scale > 0.f,
               RL_ERR_ARGS, "%s: fx=%g, fy=%g, depth_scale=%g must be finite and greater than 0", who, fx, fy, depth_scale);
    RL_REQUIRE(ts_finite(ppx) && ts_finite(ppy), RL_ERR_ARGS, "%s: ppx=%g, ppy=%g must be finite", who, ppx, ppy);
    RL_REQUIRE(z_lo < z_hi, RL_ERR_ARGS, "%s: z_lo=%g is not below z_hi=%g", who, z_lo, z_hi);
    RL_REQUIRE(depth && world_to_camera, RL_ERR_ARGS, "%s: null pointer", who);
    RL_REQUIRE(((uintptr_t)depth & 1) == 0, RL_ERR_ARGS, "%s: a frame that is not 2-byte aligned", who);
    for (int j = 0; j < 12; ++j)
        RL_REQUIRE(ts_finite(world_to_camera[j]), RL_ERR_ARGS, "%s: world_to_camera[%d]=%g is not finite", who, j,
                   world_to_camera[j]);
    TsFrame f;
    f.depth = depth, f.W = W, f.H = H, f.Wf = (float)W, f.Hf = (float)H;
    f.fx = fx, f.fy = fy, f.ppx = ppx, f.ppy = ppy, f.scale = depth_scale;
    f.z_lo = z_lo, f.z_hi = z_hi;
    f.trunc = trunc, f.neg_trunc = -trunc, f.max_weight = (float)max_weight;
    for (int j = 0; j < 9; ++j) f.r[j] = world_to_camera[j];
    for (int j = 0; j < 3; ++j) f.t[j] = world_to_camera[9 + j];
    const long runs = (g.V + TS_RUN - 1) / TS_RUN;
    hipLaunchKernelGGL(ts_integrate, dim3((unsigned)((runs + TS_THREADS - 1) / TS_THREADS)), dim3(TS_THREADS), 0,
                       (hipStream_t)stream, g, f, tsdf, weight);
    rl_note_kernel("ts_integrate");
    RL_LAUNCH_CHECK("rl_tsdf_integrate");
    return RL_OK;
}

extern "C" int rl_tsdf_count(const float* tsdf, const float* weight, int nx, int ny, int nz, const float* origin, float voxel,
                             int min_weight, int64_t* count_out, void* ws, int64_t ws_bytes, void* stream) {
    const char* who = "rl_tsdf_count";
    TsVolume g;
    TsSurface s;
    int rc = ts_volume(who, tsdf, weight, nx, ny, nz, origin, voxel, &g);
    if (rc) return rc;
    if ((rc = ts_surface(who, tsdf, weight, min_weight, &s))) return rc;
    RL_REQUIRE(count_out, RL_ERR_ARGS, "%s: null pointer", who);
    if ((rc = rl_ws_check(who, ws, ws_bytes, rl_tsdf_workspace_bytes(g.V)))) return rc;
    hipStream_t sm = (hipStream_t)stream;
    const long chunks = ts_chunks(g.V);
    uint32_t* cnt = rl_at<uint32_t>(ws, 0);
    hipLaunchKernelGGL(ts_count, dim3((unsigned)chunks), dim3(TS_LANES), 0, sm, g, s, cnt);
    RL_LAUNCH_CHECK("rl_tsdf_count (count)");
    hipLaunchKernelGGL(ts_scan, dim3(1), dim3(GR_THREADS), 0, sm, cnt, (int)chunks, count_out);
    rl_note_kernel("ts_scan");
    RL_LAUNCH_CHECK("rl_tsdf_count (scan)");
    return RL_OK;
}

extern "C" int rl_tsdf_points(const float* tsdf, const float* weight, int nx, int ny, int nz, const float* origin, float voxel,
                              int min_weight, int64_t count, float* xyz_out, int64_t* edge_out, int64_t capacity, void* ws,
                              int64_t ws_bytes, void* stream) {
    const char* who = "rl_tsdf_points";
    TsVolume g;
    TsSurface s;
    int rc = ts_volume(who, tsdf, weight, nx, ny, nz, origin, voxel, &g);
    if (rc) return rc;
    if ((rc = ts_surface(who, tsdf, weight, min_weight, &s))) return rc;
    RL_REQUIRE(count >= 1 && count < 0x100000000LL && count <= 3 * (int64_t)g.V, RL_ERR_ARGS,
               "%s: count=%lld outside 1 .. min(2^32 - 1, 3 * voxels)", who, (long long)count);
    RL_REQUIRE(capacity >= count, RL_ERR_ARGS, "%s: outputs of %lld rows for %lld points", who, (long long)capacity,
               (long long)count);
    RL_REQUIRE(xyz_out && edge_out, RL_ERR_ARGS, "%s: null pointer", who);
    RL_REQUIRE(((uintptr_t)xyz_out & 3) == 0 && ((uintptr_t)edge_out & 7) == 0, RL_ERR_ARGS, "%s: misaligned outputs", who);
    if ((rc = rl_ws_check(who, ws, ws_bytes, rl_tsdf_workspace_bytes(g.V)))) return rc;
    hipLaunchKernelGGL(ts_write, dim3((unsigned)ts_chunks(g.V)), dim3(TS_LANES), 0, (hipStream_t)stream, g, s,
                       (const uint32_t*)rl_at<uint32_t>(ws, 0), xyz_out, edge_out, (long)capacity);
    rl_note_kernel("ts_write");
    RL_LAUNCH_CHECK("rl_tsdf_points");
    return RL_OK;
}
