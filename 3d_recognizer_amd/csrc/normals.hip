// Normals and curvature of a point cloud from every point's k nearest neighbours (rl_normals; the numpy twin and the
// contract are randlanet/utils/normals.py): the fp64 covariance of the k neighbour rows, 6 cyclic Jacobi sweeps, the
// eigenvector of the smallest eigenvalue turned towards a viewpoint or upward.  Every sum runs in the twin's order - the
// K-NN's rank order - and -ffp-contract=off keeps every operation a correctly rounded fp64 one, so the result equals the
// twin's bit for bit.
//
// Mapping: one wavefront = one workgroup = 64 consecutive queries, one lane per query.  The work per point is k gathered
// 12-byte rows, ~9k fp64 multiply-adds and 18 rotations, all of it sequential inside a point, so a point cannot be
// split over lanes without changing the order of its sums; the gathers are what can be shared.  The wavefront reads its
// 64*k neighbour indices as one contiguous run of nbr_idx (coalesced 8-byte loads, 64 in flight per instruction) and
// gathers the rows into LDS with all 64 lanes busy, whatever k is; then every lane walks its own k rows twice (centroid,
// covariance) out of LDS.  The LDS tile is rank-major - row (rank j, query q) at (j*64 + q)*3 floats - so the 64 lanes of
// one read are 3 dwords apart: no bank conflicts on the reads that run 2k times; the staging writes, which run once,
// take the conflicts.  64*k*12 bytes of LDS: 12 KiB at k = 16 (13 workgroups per CU), 48 KiB at k = 64.
#include "rl_common.h"
#include "rl_jacobi.h"

namespace {

constexpr int NR_LANES = 64;

__global__ __launch_bounds__(NR_LANES) void normals_kernel(const float* __restrict__ xyz, long M,
                                                           const int64_t* __restrict__ nbr, long first, long Q, int k,
                                                           const float* __restrict__ viewpoint,
                                                           float* __restrict__ normals_out, float* __restrict__ curv_out,
                                                           double* __restrict__ cov_out) {
    extern __shared__ float rows[];                    // [k][64][3]
    const int lane = threadIdx.x;
    const long q0 = (long)blockIdx.x * NR_LANES;       // this wavefront's first query, counted from `first`
    const int nq = (int)min((long)NR_LANES, Q - q0);
    // stage: entry e of this wavefront's run of nbr_idx is (query e / k, rank e % k)
    const int64_t* run = nbr + q0 * k;
    const int entries = nq * k;
    for (int e = lane; e < entries; e += NR_LANES) {
        long j = run[e];
        j = j < 0 ? 0 : (j >= M ? M - 1 : j);          // (the K-NN never leaves [0, M): a guard against a foreign buffer)
        const float* s = xyz + 3 * j;
        const int qq = e / k, r = e - qq * k;
        float* d = rows + (r * NR_LANES + qq) * 3;
        d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
    }
    __syncthreads();
    if (lane >= nq) return;
    const float* mine = rows + lane * 3;
    const double kk = (double)k;
    double mx = 0.0, my = 0.0, mz = 0.0;
    for (int j = 0; j < k; ++j) {
        const float* p = mine + j * (NR_LANES * 3);
        mx += (double)p[0]; my += (double)p[1]; mz += (double)p[2];
    }
    mx /= kk; my /= kk; mz /= kk;
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
    for (int j = 0; j < k; ++j) {
        const float* p = mine + j * (NR_LANES * 3);
        const double dx = (double)p[0] - mx, dy = (double)p[1] - my, dz = (double)p[2] - mz;
        a00 += dx * dx; a01 += dx * dy; a02 += dx * dz;
        a11 += dy * dy; a12 += dy * dz; a22 += dz * dz;
    }
    a00 /= kk; a01 /= kk; a02 /= kk; a11 /= kk; a12 /= kk; a22 /= kk;
    const long i = first + q0 + lane;                  // this lane's point
    if (cov_out) {
        double* c = cov_out + (q0 + lane) * 6;
        c[0] = a00; c[1] = a01; c[2] = a02; c[3] = a11; c[4] = a12; c[5] = a22;
    }
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
    for (int sweep = 0; sweep < 6; ++sweep) {
        nr_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);      // (0, 1), r = 2
        nr_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);      // (0, 2), r = 1
        nr_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);      // (1, 2), r = 0
    }
    // the smallest eigenvalue, ties to the lowest index, and its column of V
    const bool one = a11 < a00;
    double lam = one ? a11 : a00, n0 = one ? v01 : v00, n1 = one ? v11 : v10, n2 = one ? v21 : v20;
    const bool two = a22 < lam;
    lam = two ? a22 : lam; n0 = two ? v02 : n0; n1 = two ? v12 : n1; n2 = two ? v22 : n2;
    const double tr = (a00 + a11) + a22;
    float curv = 0.f;
    if (tr > 0.0) {
        curv = (float)(fmax(lam, 0.0) / tr);
    } else {
        n0 = 0.0; n1 = 0.0; n2 = 0.0;
    }
    bool neg = n2 != 0.0 ? n2 < 0.0 : (n1 != 0.0 ? n1 < 0.0 : n0 < 0.0);      // upward
    if (viewpoint) {
        const float* p = xyz + 3 * i;
        const double w0 = (double)viewpoint[0] - (double)p[0], w1 = (double)viewpoint[1] - (double)p[1],
                     w2 = (double)viewpoint[2] - (double)p[2];
        const double s = (n0 * w0 + n1 * w1) + n2 * w2;
        neg = s == 0.0 ? neg : s < 0.0;
    }
    float* o = normals_out + 3 * i;
    o[0] = (float)(neg ? -n0 : n0);
    o[1] = (float)(neg ? -n1 : n1);
    o[2] = (float)(neg ? -n2 : n2);
    curv_out[i] = curv;
}

}  // namespace

extern "C" int rl_normals(const float* xyz, int64_t M, const int64_t* nbr_idx, int64_t first, int64_t Q, int k,
                          const float* viewpoint, float* normals_out, float* curvature_out, double* cov_out, void* stream) {
    RL_REQUIRE(k >= 3 && k <= RL_KNN_MAX_K, RL_ERR_ARGS, "rl_normals: k=%d outside 3 .. %d", k, RL_KNN_MAX_K);
    RL_REQUIRE(M >= k && M < 0x7fffffffLL, RL_ERR_ARGS, "rl_normals: M=%lld outside k=%d .. 2^31-2", (long long)M, k);
    RL_REQUIRE(first >= 0 && Q > 0 && first <= M - Q, RL_ERR_ARGS, "rl_normals: queries %lld .. %lld of M=%lld points",
               (long long)first, (long long)first + (long long)Q - 1, (long long)M);
    RL_REQUIRE(xyz && nbr_idx && normals_out && curvature_out, RL_ERR_ARGS, "rl_normals: null pointer");
    const size_t lds = (size_t)k * NR_LANES * 3 * sizeof(float);
    hipLaunchKernelGGL(normals_kernel, dim3(rl_cdiv(Q, NR_LANES)), dim3(NR_LANES), lds, (hipStream_t)stream, xyz, (long)M,
                       nbr_idx, (long)first, (long)Q, k, viewpoint, normals_out, curvature_out, cov_out);
    rl_note_kernel("normals_kernel");
    RL_LAUNCH_CHECK("rl_normals");
    return RL_OK;
}
