// Fast point feature histograms (rl_fpfh_*; the numpy twin and the contract are randlanet/utils/features.py): PCL's
// FPFHEstimation / Open3D's compute_fpfh_feature, with the third angle replaced by its diamond pseudo-angle so that no libm
// function is involved.  The inputs are the cloud, its normals and the k + 1 rows of rl_knn_f32 of the cloud in itself.  Every
// operation is one correctly rounded fp32 one (-ffp-contract=off, true division, the root through fp64), the histograms are
// integers, and the weighted sums run in rank order inside one lane, so the result equals the twin's bit for bit.
//
//   rl_fpfh_spfh  fp_spfh  one WAVEFRONT per point, lane r - 1 owns the neighbour of rank r (k <= 63): two gathered rows, the
//                          Darboux frame, three bins; a bin's count is the popcount of a ballot, which lane `bin` keeps:
//                          33 ballots per point, no LDS, no atomic.  Writes the point's 33 bytes
//   rl_fpfh_fpfh  fp_fpfh  one wavefront per point, lane b owns bin b (33 of 64 lanes): the index and the weight of a rank are
//                          wave-uniform, the neighbour's 33 SPFH bytes one coalesced read; the sub-histogram's sum in bin
//                          order by eleven shuffles; scales, quantises, writes 33 floats and 36 bytes
// Mapping and why.  A lane per POINT would need 33 counters indexed by a run-time bin per lane - scratch memory or an LDS
// histogram with read-modify-write per pair - and its gathers (the neighbour's row and normal) would be 64 unrelated rows per
// instruction either way.  With the neighbourhood in the lanes the per-pair arithmetic (about 90 operations with three
// divisions and three roots) is spread over k lanes, the histogram is 33 scalar popcounts, and in the second kernel the bins in
// the lanes make the k SPFH rows coalesced 33-byte reads and the rank order a plain loop.  What is left idle is 64 - k lanes
// in the first kernel and 31 in the second; both kernels are bound by the latency of their gathers, not by the VALU, and four
// wavefronts per workgroup with up to eight workgroups per CU hide it.
#include "rl_common.h"

#include <math.h>

namespace {

constexpr int FP_BINS = 11;
constexpr int FP_DIM = 33;
constexpr int FP_CODE = 36;
constexpr int FP_WAVES = 4;           // points per workgroup

__device__ __forceinline__ float fp_sqrt(float x) { return (float)sqrt((double)x); }      // correctly rounded (see planes.hip)

// bin(t) of the contract: top when t >= top, trunc(t) when 0 < t < top, 0 otherwise (a NaN fails both compares)
__device__ __forceinline__ int fp_bin(float t, int top) { return t >= (float)top ? top : (t > 0.0f ? (int)t : 0); }

__device__ __forceinline__ float fp_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

__global__ __launch_bounds__(64 * FP_WAVES) void fp_spfh(const float* __restrict__ xyz, const float* __restrict__ normals, long M,
                                                          const int64_t* __restrict__ idx, const float* __restrict__ d2,
                                                          long first, long Q, int k, uint8_t* __restrict__ spfh) {
    const int lane = threadIdx.x & 63;
    const long qi = (long)blockIdx.x * FP_WAVES + (threadIdx.x >> 6);      // wave-uniform
    if (qi >= Q) return;
    const long i = first + qi;
    const int k1 = k + 1;
    const bool has = lane < k;                                            // the lane's rank is lane + 1
    const long jj = has ? idx[qi * k1 + lane + 1] : i;
    const bool inside = jj >= 0 && jj < M;                                // (always, from rl_knn_f32: nothing is read outside)
    const long j = inside ? jj : i;
    const float dd = has ? d2[qi * k1 + lane + 1] : 0.0f;
    const float px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
    const float ux = normals[3 * i], uy = normals[3 * i + 1], uz = normals[3 * i + 2];
    const float nx = normals[3 * j], ny = normals[3 * j + 1], nz = normals[3 * j + 2];
    const float dist = fp_sqrt(dd);
    const float dx = __fdiv_rn(xyz[3 * j] - px, dist), dy = __fdiv_rn(xyz[3 * j + 1] - py, dist),
                dz = __fdiv_rn(xyz[3 * j + 2] - pz, dist);
    float vx = dy * uz - dz * uy, vy = dz * ux - dx * uz, vz = dx * uy - dy * ux;
    const float lv2 = (vx * vx + vy * vy) + vz * vz;
    const float lv = fp_sqrt(lv2);
    vx = __fdiv_rn(vx, lv), vy = __fdiv_rn(vy, lv), vz = __fdiv_rn(vz, lv);
    const float wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;
    const float f1 = fp_dot(vx, vy, vz, nx, ny, nz);
    const float f2 = fp_dot(ux, uy, uz, dx, dy, dz);
    const float x = fp_dot(ux, uy, uz, nx, ny, nz);
    const float y = fp_dot(wx, wy, wz, nx, ny, nz);
    const bool counted = has && inside && dd != 0.0f && lv2 > 0.0f && lv2 <= 3.4028234663852886e38f &&
                         (ux != 0.0f || uy != 0.0f || uz != 0.0f) && (nx != 0.0f || ny != 0.0f || nz != 0.0f);
    const int b1 = fp_bin((f1 + 1.0f) * 5.5f, FP_BINS - 1);
    const int b2 = fp_bin((f2 + 1.0f) * 5.5f, FP_BINS - 1);
    const float s = fabsf(x) + fabsf(y);
    const float r = __fdiv_rn(y, s);
    float a = x > 0.0f ? 2.0f + r : (y >= 0.0f ? 4.0f - r : 0.0f - r);
    a = s > 0.0f ? a : 0.0f;
    const int b3 = fp_bin(a * 2.75f, FP_BINS - 1);
    uint32_t mine = 0;
#pragma unroll
    for (int b = 0; b < FP_BINS; ++b) {
        const uint32_t c1 = (uint32_t)__popcll(__ballot(counted && b1 == b));
        const uint32_t c2 = (uint32_t)__popcll(__ballot(counted && b2 == b));
        const uint32_t c3 = (uint32_t)__popcll(__ballot(counted && b3 == b));
        mine = lane == b ? c1 : lane == FP_BINS + b ? c2 : lane == 2 * FP_BINS + b ? c3 : mine;
    }
    if (lane < FP_DIM) spfh[i * FP_DIM + lane] = (uint8_t)mine;
}

__global__ __launch_bounds__(64 * FP_WAVES) void fp_fpfh(const uint8_t* __restrict__ spfh, long M, const int64_t* __restrict__ idx,
                                                          const float* __restrict__ d2, long first, long Q, int k,
                                                          float* __restrict__ desc, uint8_t* __restrict__ code) {
    const int lane = threadIdx.x & 63;
    const long qi = (long)blockIdx.x * FP_WAVES + (threadIdx.x >> 6);      // wave-uniform
    if (qi >= Q) return;
    const long i = first + qi;
    const int k1 = k + 1;
    const int bin = lane < FP_DIM ? lane : 0;                             // (the idle lanes follow bin 0 and write nothing)
    float acc = 0.0f;
    for (int r = 1; r <= k; ++r) {
        const long jj = idx[qi * k1 + r];
        const float dd = d2[qi * k1 + r];
        const float w = __fdiv_rn(1.0f, dd);
        const bool use = jj >= 0 && jj < M && dd != 0.0f && fabsf(w) <= 3.4028234663852886e38f;      // wave-uniform
        if (use) acc = acc + (float)spfh[jj * FP_DIM + bin] * w;
    }
    const int base = (bin / FP_BINS) * FP_BINS;
    float S = 0.0f;
#pragma unroll
    for (int b = 0; b < FP_BINS; ++b) S = S + __shfl(acc, base + b, 64);
    const bool ok = S > 0.0f && S <= 3.4028234663852886e38f;
    const float scale = __fdiv_rn(100.0f, S);
    const float F = ok ? acc * scale : 0.0f;
    const float t = F * 2.55f + 0.5f;
    const int c = t >= 255.0f ? 255 : (t > 0.0f ? (int)t : 0);
    if (lane < FP_DIM) desc[i * FP_DIM + lane] = F;
    if (lane < FP_CODE) code[i * FP_CODE + lane] = lane < FP_DIM ? (uint8_t)c : (uint8_t)0;
}

bool fp_size_ok(int64_t M, int k) { return k >= 2 && k <= RL_KNN_MAX_K - 1 && M >= k + 1 && M < 0x7fffffffLL; }

int fp_check(const char* who, int64_t M, int64_t first, int64_t Q, int k) {
    RL_REQUIRE(k >= 2 && k <= RL_KNN_MAX_K - 1, RL_ERR_ARGS, "%s: k=%d outside 2 .. %d", who, k, RL_KNN_MAX_K - 1);
    RL_REQUIRE(fp_size_ok(M, k), RL_ERR_ARGS, "%s: M=%lld outside k + 1 = %d .. 2^31-2", who, (long long)M, k + 1);
    RL_REQUIRE(first >= 0 && Q > 0 && first <= M - Q, RL_ERR_ARGS, "%s: rows %lld .. %lld of M=%lld points", who, (long long)first,
               (long long)first + (long long)Q - 1, (long long)M);
    return RL_OK;
}

}  // namespace

extern "C" int rl_fpfh_spfh(const float* xyz, const float* normals, int64_t M, const int64_t* idx, const float* d2, int64_t first,
                            int64_t Q, int k, uint8_t* spfh_out, void* stream) {
    int rc = fp_check("rl_fpfh_spfh", M, first, Q, k);
    if (rc) return rc;
    RL_REQUIRE(xyz && normals && idx && d2 && spfh_out, RL_ERR_ARGS, "rl_fpfh_spfh: null pointer");
    hipLaunchKernelGGL(fp_spfh, dim3(rl_cdiv(Q, FP_WAVES)), dim3(64 * FP_WAVES), 0, (hipStream_t)stream, xyz, normals, (long)M, idx,
                       d2, (long)first, (long)Q, k, spfh_out);
    rl_note_kernel("fp_spfh");
    RL_LAUNCH_CHECK("rl_fpfh_spfh");
    return RL_OK;
}

extern "C" int rl_fpfh_fpfh(const uint8_t* spfh, int64_t M, const int64_t* idx, const float* d2, int64_t first, int64_t Q, int k,
                            float* desc_out, uint8_t* code_out, void* stream) {
    int rc = fp_check("rl_fpfh_fpfh", M, first, Q, k);
    if (rc) return rc;
    RL_REQUIRE(spfh && idx && d2 && desc_out && code_out, RL_ERR_ARGS, "rl_fpfh_fpfh: null pointer");
    hipLaunchKernelGGL(fp_fpfh, dim3(rl_cdiv(Q, FP_WAVES)), dim3(64 * FP_WAVES), 0, (hipStream_t)stream, spfh, (long)M, idx, d2,
                       (long)first, (long)Q, k, desc_out, code_out);
    rl_note_kernel("fp_fpfh");
    RL_LAUNCH_CHECK("rl_fpfh_fpfh");
    return RL_OK;
}
