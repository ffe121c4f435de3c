// Depth frames to points (rl_depth_*; the numpy twin and the contract are randlanet/utils/depth.py): the stage between a depth
// camera's raw z16 frame and the cloud every other entry starts from.  Per pixel: the temporal filter (librealsense's rule with
// persistence off, restated in utils/depth.py) against a resident uint16 state, z = d * depth_scale, the pinhole ray - with the
// inverse Brown-Conrady model when coefficients are given - and the point (x * z, y * z, z); the pixels with d != 0 and
// z_lo < z < z_hi are written in row-major pixel order, with their pixel index.  -ffp-contract=off keeps every operation a
// correctly rounded fp32 one, in the order of the twin, so the result equals the twin's bit for bit.
//
//   rl_depth_points  dp_count  one wavefront per chunk of 1024 pixels: the kept pixels of the chunk (the filtered value is
//                              recomputed from the old state, nothing is stored)
//                    dp_scan   one workgroup: the exclusive prefix of those counts, and M
//                    dp_write  one wavefront per chunk: state and filtered frame (the ONE update of the state per frame), and the
//                              kept points in pixel order
//   without outputs for the points (the filter alone): dp_write only.
// No atomics at all, and no workgroup waits for another one.
//
// Mapping and why.  A pixel is 2 bytes in (with the filter 2 more in and 2 out) and a kept point 16 bytes out, so one pixel per
// lane would issue 2-byte loads.  A lane takes a run of 8 consecutive pixels - one 16-byte load per array - and a wavefront a
// turn of 512, two turns per chunk; the order inside a turn comes from the lanes' popcounts and one wavefront prefix (six
// shuffles), not from a ballot per pixel.  The runs are laid from the 16-byte boundary at or below `depth`, so every run that
// lies inside the frame is aligned whatever the frame's own alignment is (frame i of a (B, H, W) tensor with odd H * W is only
// 2-byte aligned); the runs that straddle the frame's ends, and the runs of a state or filtered frame that is aligned
// differently from `depth`, go element by element.  The ray of a pixel is recomputed (a subtraction and a division per axis): a
// table of rays would cost 8 bytes of traffic per pixel to save them in a kernel that is bound by its launches, not its ALU.
#include "rl_radix.h"

#include <math.h>

namespace {

constexpr int DP_LANES = 64;
constexpr int DP_RUN = 8;                          // pixels of a lane per turn: 16 bytes
constexpr int DP_TURN = DP_LANES * DP_RUN;
constexpr int DP_TURNS = 2;
constexpr long DP_CHUNK = (long)DP_TURN * DP_TURNS;

struct DpArgs {
    const uint16_t* depth;
    uint16_t* state;         // null: no temporal filter
    uint16_t* filtered;      // null: not wanted
    long P;                  // pixels
    int W, stride;
    int head;                // uint16 elements between the 16-byte boundary at or below depth and depth: 0 .. 7
    float fx, fy, ppx, ppy, scale;
    int distort;
    float k1, k2, p1, p2, k3;
    float alpha, one_minus_alpha;
    int delta;
    float z_lo, z_hi;
};

// chunks of a frame of P pixels whose first pixel lies `head` elements into its first run
inline long dp_chunks(long P, int head) { return (P + head + DP_CHUNK - 1) / DP_CHUNK; }

// p[i0 .. i0 + 7]; an entry outside [0, P) reads as 0.  One 16-byte load where the run lies inside and is aligned
__device__ __forceinline__ void dp_load8(const uint16_t* __restrict__ p, long i0, long P, uint32_t v[DP_RUN]) {
    if (i0 >= 0 && i0 + DP_RUN <= P && ((uintptr_t)(p + i0) & 15) == 0) {
        const uint4 w = *reinterpret_cast<const uint4*>(p + i0);
        v[0] = w.x & 0xffffu; v[1] = w.x >> 16;
        v[2] = w.y & 0xffffu; v[3] = w.y >> 16;
        v[4] = w.z & 0xffffu; v[5] = w.z >> 16;
        v[6] = w.w & 0xffffu; v[7] = w.w >> 16;
        return;
    }
#pragma unroll
    for (int j = 0; j < DP_RUN; ++j) {
        const long i = i0 + j;
        const uint32_t x = p[i < 0 ? 0 : (i < P ? i : P - 1)];
        v[j] = i >= 0 && i < P ? x : 0u;
    }
}

// the same run written; entries outside [0, P) are not
__device__ __forceinline__ void dp_store8(uint16_t* __restrict__ p, long i0, long P, const uint32_t v[DP_RUN]) {
    if (i0 >= 0 && i0 + DP_RUN <= P && ((uintptr_t)(p + i0) & 15) == 0) {
        uint4 w;
        w.x = v[0] | (v[1] << 16);
        w.y = v[2] | (v[3] << 16);
        w.z = v[4] | (v[5] << 16);
        w.w = v[6] | (v[7] << 16);
        *reinterpret_cast<uint4*>(p + i0) = w;
        return;
    }
#pragma unroll
    for (int j = 0; j < DP_RUN; ++j) {
        const long i = i0 + j;
        if (i >= 0 && i < P) p[i] = (uint16_t)v[j];
    }
}

// the temporal filter of one pixel: current value c, state s -> the output, and the new state
__device__ __forceinline__ uint32_t dp_filter(uint32_t c, uint32_t s, const DpArgs& a, uint32_t* s_new) {
    if (c == 0u) {
        *s_new = s;
        return 0u;
    }
    uint32_t o = c;
    const int diff = (int)c - (int)s;
    if (s != 0u && (diff < 0 ? -diff : diff) < a.delta) {
        const float f = (a.alpha * (float)c + a.one_minus_alpha * (float)s) + 0.5f;
        const int t = (int)f;
        o = (uint32_t)(t > 65535 ? 65535 : t);
    }
    *s_new = o;
    return o;
}

// the run i0 .. i0 + 7 of this lane: the values the deprojection reads into d (the filtered ones with a state) and the new
// state into s_new; returns the mask of the kept pixels and leaves their z in z
__device__ __forceinline__ uint32_t dp_run(const DpArgs& a, long i0, uint32_t d[DP_RUN], uint32_t s_new[DP_RUN],
                                           float z[DP_RUN]) {
    dp_load8(a.depth, i0, a.P, d);
    if (a.state) {
        uint32_t s[DP_RUN];
        dp_load8(a.state, i0, a.P, s);
#pragma unroll
        for (int j = 0; j < DP_RUN; ++j) d[j] = dp_filter(d[j], s[j], a, &s_new[j]);
    }
    const uint32_t first = (uint32_t)(i0 < 0 ? 0 : i0);     // (below P < 2^31 wherever a value is not 0)
    const uint32_t v0 = first / (uint32_t)a.W, u0 = first - v0 * (uint32_t)a.W;
    uint32_t mask = 0u;
#pragma unroll
    for (int j = 0; j < DP_RUN; ++j) {
        z[j] = (float)d[j] * a.scale;
        bool keep = d[j] != 0u && a.z_lo < z[j] && z[j] < a.z_hi;       // (d is 0 outside the frame)
        if (a.stride > 1 && keep) {
            const uint32_t i = (uint32_t)(i0 + j);
            const uint32_t v = v0 + (u0 + (i - first)) / (uint32_t)a.W, u = i - v * (uint32_t)a.W;
            keep = u % (uint32_t)a.stride == 0u && v % (uint32_t)a.stride == 0u;
        }
        mask |= keep ? 1u << j : 0u;
    }
    return mask;
}

__device__ __forceinline__ uint32_t dp_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one wavefront per chunk: how many of its pixels are kept
__global__ __launch_bounds__(DP_LANES) void dp_count(const DpArgs a, uint32_t* __restrict__ cnt) {
    const int lane = threadIdx.x;
    uint32_t n = 0;
#pragma unroll
    for (int t = 0; t < DP_TURNS; ++t) {
        const long i0 = (long)blockIdx.x * DP_CHUNK + t * DP_TURN + lane * DP_RUN - a.head;
        uint32_t d[DP_RUN], s_new[DP_RUN];
        float z[DP_RUN];
        if (i0 < a.P) n += (uint32_t)__popc(dp_run(a, i0, d, s_new, z));
    }
    n = dp_wave_sum(n);
    if (lane == 0) cnt[blockIdx.x] = n;
}

__global__ __launch_bounds__(GR_THREADS) void dp_scan(uint32_t* __restrict__ cnt, int chunks, int64_t* __restrict__ count_out) {
    const uint32_t kept = block_exclusive_scan(cnt, chunks);
    if (threadIdx.x == 0) count_out[0] = (int64_t)kept;
}

// one wavefront per chunk.  xyz_out == nullptr: the filter alone
__global__ __launch_bounds__(DP_LANES) void dp_write(const DpArgs a, const uint32_t* __restrict__ cnt,
                                                     float* __restrict__ xyz_out, int32_t* __restrict__ pixel_out) {
    const int lane = threadIdx.x;
    uint32_t run = xyz_out ? cnt[blockIdx.x] : 0u;      // kept pixels before this chunk
    for (int t = 0; t < DP_TURNS; ++t) {
        const long t0 = (long)blockIdx.x * DP_CHUNK + t * DP_TURN - a.head;
        if (t0 >= a.P) break;                           // wavefront-uniform
        const long i0 = t0 + lane * DP_RUN;
        uint32_t d[DP_RUN], s_new[DP_RUN], mask = 0u;
        float z[DP_RUN];
        if (i0 < a.P) {
            mask = dp_run(a, i0, d, s_new, z);
            if (a.state) dp_store8(a.state, i0, a.P, s_new);
            if (a.filtered) dp_store8(a.filtered, i0, a.P, d);
        }
        if (!xyz_out) continue;                         // wavefront-uniform
        const uint32_t mine = (uint32_t)__popc(mask);
        uint32_t incl = mine;                           // kept pixels of the lanes up to this one
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        long s = (long)run + (incl - mine);
        run += __shfl(incl, 63, 64);
        if (mask == 0u) continue;                       // (no shuffle below this line)
        const uint32_t first = (uint32_t)(i0 < 0 ? 0 : i0);
        const uint32_t v0 = first / (uint32_t)a.W, u0 = first - v0 * (uint32_t)a.W;
#pragma unroll
        for (int j = 0; j < DP_RUN; ++j) {
            if (!((mask >> j) & 1u)) continue;
            const uint32_t i = (uint32_t)(i0 + j);
            const uint32_t v = v0 + (u0 + (i - first)) / (uint32_t)a.W, u = i - v * (uint32_t)a.W;
            float x = __fdiv_rn((float)u - a.ppx, a.fx);
            float y = __fdiv_rn((float)v - a.ppy, a.fy);
            if (a.distort) {
                const float r2 = x * x + y * y;
                const float f = 1.f + r2 * (a.k1 + r2 * (a.k2 + r2 * a.k3));
                const float xd = x * f + ((2.f * a.p1) * (x * y) + a.p2 * (r2 + 2.f * (x * x)));
                const float yd = y * f + ((2.f * a.p2) * (x * y) + a.p1 * (r2 + 2.f * (y * y)));
                x = xd;
                y = yd;
            }
            if (s < a.P) {                              // (always: s counts kept pixels before i)
                xyz_out[3 * s + 0] = x * z[j];
                xyz_out[3 * s + 1] = y * z[j];
                xyz_out[3 * s + 2] = z[j];
                pixel_out[s] = (int32_t)i;
            }
            ++s;
        }
    }
}

inline bool dp_finite(float x) { return x >= -3.402823466e38f && x <= 3.402823466e38f; }

}  // namespace

extern "C" int64_t rl_depth_workspace_bytes(int64_t pixels) {
    if (pixels < 1 || pixels >= 0x80000000LL) return 0;
    RlCarve c;
    c.take((size_t)dp_chunks((long)pixels, DP_RUN - 1) * sizeof(uint32_t));      // (whatever the frame's alignment is)
    return (int64_t)c.at;
}

extern "C" int rl_depth_points(const uint16_t* depth, uint16_t* state, uint16_t* filtered_out, int W, int H, int stride,
                               float fx, float fy, float ppx, float ppy, float depth_scale, const float* coeffs, float alpha,
                               float one_minus_alpha, int delta, float z_lo, float z_hi, float* xyz_out, int32_t* pixel_out,
                               int64_t* count_out, void* ws, int64_t ws_bytes, void* stream) {
    RL_REQUIRE(W >= 1 && H >= 1 && (int64_t)W * H < 0x80000000LL, RL_ERR_ARGS,
               "rl_depth_points: a frame of %d x %d pixels, outside 1 .. 2^31 - 1", H, W);
    RL_REQUIRE(stride >= 1, RL_ERR_ARGS, "rl_depth_points: stride=%d below 1", stride);
    RL_REQUIRE(dp_finite(fx) && fx > 0.f && dp_finite(fy) && fy > 0.f && dp_finite(depth_scale) && depth_scale > 0.f,
               RL_ERR_ARGS, "rl_depth_points: fx=%g, fy=%g, depth_scale=%g must be finite and greater than 0", fx, fy,
               depth_scale);
    RL_REQUIRE(dp_finite(ppx) && dp_finite(ppy), RL_ERR_ARGS, "rl_depth_points: ppx=%g, ppy=%g must be finite", ppx, ppy);
    RL_REQUIRE(z_lo < z_hi, RL_ERR_ARGS, "rl_depth_points: z_lo=%g is not below z_hi=%g", z_lo, z_hi);
    if (coeffs)
        for (int j = 0; j < 5; ++j)
            RL_REQUIRE(dp_finite(coeffs[j]), RL_ERR_ARGS, "rl_depth_points: coeffs[%d]=%g is not finite", j, coeffs[j]);
    if (state) {
        RL_REQUIRE(alpha > 0.f && alpha <= 1.f, RL_ERR_ARGS, "rl_depth_points: alpha=%g outside (0, 1]", alpha);
        RL_REQUIRE(one_minus_alpha >= 0.f && one_minus_alpha < 1.f, RL_ERR_ARGS,
                   "rl_depth_points: one_minus_alpha=%g outside [0, 1)", one_minus_alpha);
        RL_REQUIRE(delta >= 1 && delta <= 65535, RL_ERR_ARGS, "rl_depth_points: delta=%d outside 1 .. 65535", delta);
    }
    const bool points = xyz_out || pixel_out || count_out;
    RL_REQUIRE(!points || (xyz_out && pixel_out && count_out), RL_ERR_ARGS, "rl_depth_points: null pointer");
    RL_REQUIRE(points || state, RL_ERR_ARGS, "rl_depth_points: neither a state to filter nor outputs for the points");
    RL_REQUIRE(depth, RL_ERR_ARGS, "rl_depth_points: null pointer");
    RL_REQUIRE((((uintptr_t)depth | (uintptr_t)state | (uintptr_t)filtered_out) & 1) == 0, RL_ERR_ARGS,
               "rl_depth_points: a frame that is not 2-byte aligned");
    const long P = (long)W * H;
    if (points) {
        int rc = rl_ws_check("rl_depth_points", ws, ws_bytes, rl_depth_workspace_bytes(P));
        if (rc) return rc;
    }
    DpArgs a;
    a.depth = depth, a.state = state, a.filtered = filtered_out;
    a.P = P, a.W = W, a.stride = stride;
    a.head = (int)(((uintptr_t)depth & 15) / sizeof(uint16_t));
    a.fx = fx, a.fy = fy, a.ppx = ppx, a.ppy = ppy, a.scale = depth_scale;
    a.distort = coeffs != nullptr;
    a.k1 = coeffs ? coeffs[0] : 0.f, a.k2 = coeffs ? coeffs[1] : 0.f, a.p1 = coeffs ? coeffs[2] : 0.f;
    a.p2 = coeffs ? coeffs[3] : 0.f, a.k3 = coeffs ? coeffs[4] : 0.f;
    a.alpha = alpha, a.one_minus_alpha = one_minus_alpha, a.delta = delta;
    a.z_lo = z_lo, a.z_hi = z_hi;
    hipStream_t sm = (hipStream_t)stream;
    const long chunks = dp_chunks(P, a.head);
    uint32_t* cnt = points ? rl_at<uint32_t>(ws, 0) : nullptr;
    if (points) {
        hipLaunchKernelGGL(dp_count, dim3((unsigned)chunks), dim3(DP_LANES), 0, sm, a, cnt);
        RL_LAUNCH_CHECK("rl_depth_points (count)");
        hipLaunchKernelGGL(dp_scan, dim3(1), dim3(GR_THREADS), 0, sm, cnt, (int)chunks, count_out);
        RL_LAUNCH_CHECK("rl_depth_points (scan)");
    }
    hipLaunchKernelGGL(dp_write, dim3((unsigned)chunks), dim3(DP_LANES), 0, sm, a, (const uint32_t*)cnt, xyz_out, pixel_out);
    rl_note_kernel("dp_write");
    RL_LAUNCH_CHECK("rl_depth_points (write)");
    return RL_OK;
}
