// Rigid registration by iterative closest point (rl_icp_*; the numpy twin and the contract are randlanet/utils/registration.py):
// PCL's IterativeClosestPoint / Open3D's registration_icp.  One evaluation of a transform T is: the source moved by T in fp32,
// its exact 1-NN in the target (rl_knn_f32, not here), and per valid pair the 29 fp64 terms of the linearised point-to-plane
// (or point-to-point) problem, summed over the source in the fixed order of rl_fixedsum.h (one id whose members are source
// points 0 .. Ms-1).  The 6x6 solve and the update of T are the host's.  -ffp-contract=off keeps every operation a correctly
// rounded one, so the sums equal the twin's bit for bit.
//
//   rl_icp_transform  icp_transform  one lane per point: q = ((R0*x + R1*y) + R2*z) + t per row, fp32
//   rl_icp_sums       icp_sums       one WAVEFRONT per chunk of 1024 source points, 16 turns per lane: the pair's index and d2
//                                    (coalesced), q (coalesced), the target row and its normal (gathered, 24 bytes), the 29
//                                    terms in fp64, added per lane from 0.0; six shuffles per column; the chunk's sums and its
//                                    ballot-popcount count to the workspace, the correspondence of the rows to corr_out
//   rl_icp_fold       icp_fold       one wavefront per column: lane l adds the chunk sums l, l + 64, .. in turn, six shuffles;
//                                    a thirtieth wavefront adds the counts as integers
// No atomics, and no workgroup waits for another one.
//
// Mapping and why.  The summation order fixes the shape: a chunk is a wavefront and a lane owns 16 members, so Ms = 10^6 is 977
// wavefronts - fewer than the chip's 1024 SIMDs.  Occupancy therefore never limits icp_sums (its 138 / 148 VGPRs, no scratch, would allow 3
// wavefronts per SIMD; it gets one); what bounds it is the latency of one wavefront's dependent chain - index, then the
// gathered rows, then ~100 (plane) or ~300 (point) fp64 operations per pair - which is why the turns are unrolled by four: the
// loads of four pairs are in flight before the first term is formed.  The point metric evaluates the plane rule for the three
// unit axes as the contract says; the products by 0.0 and 1.0 are not removed by hand.
#include "rl_common.h"
#include "rl_fixedsum.h"

namespace {

constexpr int ICP_COLS = 29;          // 21 J_u*J_v (u <= v), 6 J_u*r, r*r, d2
constexpr int ICP_THREADS = 256;      // icp_transform

struct IcpRt {
    float r[9];
    float t[3];
};

struct IcpLayout {
    long chunks;         // ceil(Ms / FS_CHUNK)
    size_t off_part, off_cnt, bytes;
};

IcpLayout icp_layout(long Ms) {
    IcpLayout L;
    RlCarve c;
    L.chunks = (Ms + FS_CHUNK - 1) / FS_CHUNK;
    L.off_part = c.take((size_t)L.chunks * ICP_COLS * sizeof(double));      // column-major: [column][chunk]
    L.off_cnt = c.take((size_t)L.chunks * sizeof(uint32_t));
    L.bytes = c.at;
    return L;
}

__global__ __launch_bounds__(ICP_THREADS) void icp_transform(const float* __restrict__ src, long first, long Q, IcpRt m,
                                                             float* __restrict__ q_out) {
    const long i = (long)blockIdx.x * ICP_THREADS + threadIdx.x;
    if (i >= Q) return;
    const float* p = src + (first + i) * 3;
    const float x = p[0], y = p[1], z = p[2];
    float* o = q_out + (first + i) * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) o[a] = ((m.r[3 * a] * x + m.r[3 * a + 1] * y) + m.r[3 * a + 2] * z) + m.t[a];
}

// the 28 terms of one pair that depend on the normal: p the moved source point, d = p - y, n the normal
__device__ __forceinline__ void icp_terms(const double p[3], const double d[3], const double n[3], double c[ICP_COLS - 1]) {
    const double r = (d[0] * n[0] + d[1] * n[1]) + d[2] * n[2];
    const double J[6] = {p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0], n[0], n[1], n[2]};
    int e = 0;
#pragma unroll
    for (int u = 0; u < 6; ++u)
#pragma unroll
        for (int v = u; v < 6; ++v) c[e++] = J[u] * J[v];
#pragma unroll
    for (int u = 0; u < 6; ++u) c[21 + u] = J[u] * r;
    c[27] = r * r;
}

// one wavefront = one workgroup = chunk first / FS_CHUNK + blockIdx.x.  kPlane: the target's normals; otherwise the unit axes
template <bool kPlane>
__global__ __launch_bounds__(64) void icp_sums(const float* __restrict__ q, const float* __restrict__ normals,
                                               const float* __restrict__ target, long Mt, const int64_t* __restrict__ idx,
                                               const float* __restrict__ d2, long Ms, long first, float gate2,
                                               int64_t* __restrict__ corr_out, long chunks, double* __restrict__ part,
                                               uint32_t* __restrict__ cnt) {
    const int lane = threadIdx.x;
    const long c = first / FS_CHUNK + blockIdx.x;
    const long j0 = c * FS_CHUNK;
    double acc[ICP_COLS];
#pragma unroll
    for (int e = 0; e < ICP_COLS; ++e) acc[e] = 0.0;
    uint32_t pairs = 0;
#pragma unroll 4
    for (int t = 0; t < FS_TURNS; ++t) {
        const long i = j0 + t * 64 + lane;
        const bool live = i < Ms;
        const long ii = live ? i : j0;                     // (a dead lane reads the chunk's first row and adds +0.0)
        const long jj = idx[ii - first];
        const float dd = d2[ii - first];
        const bool inside = jj >= 0 && jj < Mt;            // (always, from rl_knn_f32: nothing is read outside the target)
        const bool valid = live && inside && dd <= gate2;
        const long j = inside ? jj : 0;
        const double p[3] = {(double)q[ii * 3], (double)q[ii * 3 + 1], (double)q[ii * 3 + 2]};
        const double d[3] = {p[0] - (double)target[j * 3], p[1] - (double)target[j * 3 + 1], p[2] - (double)target[j * 3 + 2]};
        double s[ICP_COLS];
        if constexpr (kPlane) {
            const double n[3] = {(double)normals[j * 3], (double)normals[j * 3 + 1], (double)normals[j * 3 + 2]};
            icp_terms(p, d, n, s);
        } else {
            double w[ICP_COLS - 1];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double n[3] = {a == 0 ? 1.0 : 0.0, a == 1 ? 1.0 : 0.0, a == 2 ? 1.0 : 0.0};
                icp_terms(p, d, n, w);
#pragma unroll
                for (int e = 0; e < ICP_COLS - 1; ++e) s[e] = a == 0 ? w[e] : s[e] + w[e];      // (c^0 + c^1) + c^2
            }
        }
        s[ICP_COLS - 1] = (double)dd;
#pragma unroll
        for (int e = 0; e < ICP_COLS; ++e) acc[e] = acc[e] + (valid ? s[e] : 0.0);
        pairs += (uint32_t)__popcll(__ballot(valid));
        if (live) corr_out[i] = valid ? (int64_t)jj : (int64_t)-1;
    }
#pragma unroll
    for (int e = 0; e < ICP_COLS; ++e) {
        const double s = fs_fold64(acc[e]);
        if (lane == 0) part[(long)e * chunks + c] = s;
    }
    if (lane == 0) cnt[c] = pairs;
}

// wavefront b < 29: column b's chunk sums by the same rule; wavefront 29: the counts
__global__ __launch_bounds__(64) void icp_fold(const double* __restrict__ part, const uint32_t* __restrict__ cnt, long chunks,
                                               double* __restrict__ out) {
    const int lane = threadIdx.x;
    const int b = blockIdx.x;
    if (b < ICP_COLS) {
        const double* col = part + (long)b * chunks;
        double acc = 0.0;
        for (long c = lane; c < chunks; c += 64) acc = acc + col[c];
        const double s = fs_fold64(acc);
        if (lane == 0) out[1 + b] = s;
        return;
    }
    long long n = 0;
    for (long c = lane; c < chunks; c += 64) n += (long long)cnt[c];
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) n += __shfl_xor(n, h, 64);
    if (lane == 0) out[0] = (double)n;                     // (at most Ms < 2^31: exact)
}

bool icp_size_ok(int64_t M) { return M >= 1 && M < 0x7fffffffLL; }

}  // namespace

extern "C" int64_t rl_icp_workspace_bytes(int64_t Ms) {
    if (!icp_size_ok(Ms)) return 0;
    return (int64_t)icp_layout(Ms).bytes;
}

extern "C" int rl_icp_transform(const float* src, int64_t Ms, int64_t first, int64_t Q, const float* rt, float* q_out,
                                void* stream) {
    RL_REQUIRE(icp_size_ok(Ms), RL_ERR_ARGS, "rl_icp_transform: Ms=%lld outside 1 .. 2^31-2", (long long)Ms);
    RL_REQUIRE(first >= 0 && Q > 0 && first <= Ms - Q, RL_ERR_ARGS, "rl_icp_transform: rows %lld .. %lld of Ms=%lld points",
               (long long)first, (long long)first + (long long)Q - 1, (long long)Ms);
    RL_REQUIRE(src && rt && q_out, RL_ERR_ARGS, "rl_icp_transform: null pointer");
    IcpRt m;
    for (int a = 0; a < 9; ++a) m.r[a] = rt[a];
    for (int a = 0; a < 3; ++a) m.t[a] = rt[9 + a];
    hipLaunchKernelGGL(icp_transform, dim3(rl_cdiv(Q, ICP_THREADS)), dim3(ICP_THREADS), 0, (hipStream_t)stream, src, (long)first,
                       (long)Q, m, q_out);
    rl_note_kernel("icp_transform");
    RL_LAUNCH_CHECK("rl_icp_transform");
    return RL_OK;
}

extern "C" int rl_icp_sums(const float* q, const float* normals, const float* target, int64_t Mt, const int64_t* idx,
                           const float* d2, int64_t Ms, int64_t first, int64_t Q, float gate2, int metric, int64_t* corr_out,
                           void* ws, int64_t ws_bytes, void* stream) {
    RL_REQUIRE(icp_size_ok(Ms), RL_ERR_ARGS, "rl_icp_sums: Ms=%lld outside 1 .. 2^31-2", (long long)Ms);
    RL_REQUIRE(icp_size_ok(Mt), RL_ERR_ARGS, "rl_icp_sums: Mt=%lld outside 1 .. 2^31-2", (long long)Mt);
    RL_REQUIRE(first >= 0 && Q > 0 && first <= Ms - Q, RL_ERR_ARGS, "rl_icp_sums: rows %lld .. %lld of Ms=%lld points",
               (long long)first, (long long)first + (long long)Q - 1, (long long)Ms);
    // a chunk's sum is made by one wavefront of one call: the rows start at a chunk and end at one, or at the cloud's end
    RL_REQUIRE(first % FS_CHUNK == 0 && (Q % FS_CHUNK == 0 || first + Q == Ms), RL_ERR_ARGS,
               "rl_icp_sums: rows %lld .. %lld do not start and end at chunks of %d", (long long)first,
               (long long)first + (long long)Q - 1, FS_CHUNK);
    RL_REQUIRE(gate2 > 0.f && gate2 <= 3.4028234663852886e38f, RL_ERR_ARGS, "rl_icp_sums: gate2=%g is not a finite number > 0",
               (double)gate2);
    RL_REQUIRE(metric == 0 || metric == 1, RL_ERR_ARGS, "rl_icp_sums: metric=%d is neither 0 (plane) nor 1 (point)", metric);
    int rc = rl_ws_check("rl_icp_sums", ws, ws_bytes, rl_icp_workspace_bytes(Ms));
    if (rc) return rc;
    RL_REQUIRE(q && target && idx && d2 && corr_out && (normals || metric == 1), RL_ERR_ARGS, "rl_icp_sums: null pointer");
    const IcpLayout L = icp_layout(Ms);
    double* part = rl_at<double>(ws, L.off_part);
    uint32_t* cnt = rl_at<uint32_t>(ws, L.off_cnt);
    const dim3 grid((unsigned)rl_cdiv(Q, FS_CHUNK)), wave(64);
    if (metric == 0)
        hipLaunchKernelGGL(icp_sums<true>, grid, wave, 0, (hipStream_t)stream, q, normals, target, (long)Mt, idx, d2, (long)Ms,
                           (long)first, gate2, corr_out, L.chunks, part, cnt);
    else
        hipLaunchKernelGGL(icp_sums<false>, grid, wave, 0, (hipStream_t)stream, q, normals, target, (long)Mt, idx, d2, (long)Ms,
                           (long)first, gate2, corr_out, L.chunks, part, cnt);
    rl_note_kernel("icp_sums");
    RL_LAUNCH_CHECK("rl_icp_sums");
    return RL_OK;
}

extern "C" int rl_icp_fold(int64_t Ms, double* out, void* ws, int64_t ws_bytes, void* stream) {
    RL_REQUIRE(icp_size_ok(Ms), RL_ERR_ARGS, "rl_icp_fold: Ms=%lld outside 1 .. 2^31-2", (long long)Ms);
    int rc = rl_ws_check("rl_icp_fold", ws, ws_bytes, rl_icp_workspace_bytes(Ms));
    if (rc) return rc;
    RL_REQUIRE(out, RL_ERR_ARGS, "rl_icp_fold: null pointer");
    const IcpLayout L = icp_layout(Ms);
    hipLaunchKernelGGL(icp_fold, dim3(ICP_COLS + 1), dim3(64), 0, (hipStream_t)stream, (const double*)rl_at<double>(ws, L.off_part),
                       (const uint32_t*)rl_at<uint32_t>(ws, L.off_cnt), L.chunks, out);
    rl_note_kernel("icp_fold");
    RL_LAUNCH_CHECK("rl_icp_fold");
    return RL_OK;
}
