// RANSAC over feature correspondences (rl_global_*; the numpy twin and the contract are randlanet/utils/registration.py:
// global_registration): PCL's SampleConsensusPrerejective / Open3D's registration_ransac_based_on_feature_matching.  T rigid
// transforms from three correspondences each, pre-rejected by the similarity of the triangles' edges, every one scored by the
// number of correspondences it brings within the gate; the host takes the first maximum.  Every operation is one correctly
// rounded fp32 one (-ffp-contract=off; packed v_pk_* halves round on their own) and the scores are integers; the sixteen sums
// of the refinement are fp64 in the fixed order of rl_fixedsum.h.  So everything equals the twin's bit for bit.
//
//   rl_global_hypotheses  gl_hyp     one lane per hypothesis: gathers six rows, the edge test, two triangle frames,
//                                    R = F_b F_a^T and t; writes twelve floats or twelve NaNs, and ORs the "index outside
//                                    [0, C) or [0, Mt)" flag per workgroup
//   rl_global_count       gl_pairs   one lane per correspondence: the row [a_c | b_c] (six floats) the count reads uniformly
//                         gl_count   the hot path, T * C tests, built on pl_count of planes.hip: one wavefront per (128
//                                    hypotheses, chunk of correspondences); a lane holds two hypotheses' twelve coefficients
//                                    in the halves of packed registers, the correspondence's six floats are wave-uniform
//                                    (scalar loads), the counts stay in the lane's registers.  Writes its piece of [chunks][T]
//                         gl_sum     one workgroup per 64 hypotheses: the table's column sums (integers: any order)
//   rl_global_sums        gl_sums    built on icp_sums of icp.hip: one WAVEFRONT per chunk of 1024 correspondences, 16 turns
//                                    per lane: the transform, the gate, the inlier byte, sixteen fp64 terms added per lane
//                                    from 0.0, six shuffles per column
//                         gl_fold    one wavefront per column: the chunk sums by the same rule
// No atomics, and no workgroup waits for another one.
//
// Mapping and why.  A test is 29 fp32 operations (18 for q, 3 for e, 5 for e2), a compare and an integer add; as in pl_count
// nothing but the operands can be shared, so the hypotheses sit in the lanes - 24 registers for two of them - and the
// correspondences come through the scalar cache.  gl_pairs resolves b_c = target[j_c] once, so the count's operand stream is
// one contiguous array of 24 bytes per test row instead of a dependent gather per test.
#include "rl_common.h"
#include "rl_fixedsum.h"

#include <math.h>

namespace {

constexpr int GL_LANES = 64;
constexpr int GL_GROUP = 128;                    // hypotheses of one wavefront of gl_count: two per lane
constexpr int GL_THREADS = 256;                  // gl_hyp, gl_pairs
constexpr int GL_SUM_WAVES = 16;
constexpr long GL_MIN_CHUNK = 256;               // correspondences per chunk of gl_count
constexpr long GL_MAX_CHUNKS = 1024;
constexpr long GL_TABLE = 1L << 20;              // table entries aimed at
constexpr long GL_FEW_CHUNKS = 8;                // .. but never fewer chunks than this allowed
constexpr int GL_UNROLL = 4;
constexpr int GL_COLS = 16;                      // 1, a (3), b (3), a_u * b_v (9)
constexpr float GL_FLT_MAX = 3.4028234663852886e38f;

struct GlLayout {
    long chunk, chunks;          // of gl_count
    long sum_chunks;             // ceil(C / FS_CHUNK)
    size_t off_part, off_pairs, off_table, bytes;
};

// the pieces of rl_global_sums come first and depend on C alone, so it needs no T
GlLayout global_layout(long C, long T) {
    GlLayout L;
    RlCarve c;
    long cap = GL_TABLE / T;
    cap = cap < GL_FEW_CHUNKS ? GL_FEW_CHUNKS : cap > GL_MAX_CHUNKS ? GL_MAX_CHUNKS : cap;
    L.chunk = ((C + cap - 1) / cap + 63) / 64 * 64;
    if (L.chunk < GL_MIN_CHUNK) L.chunk = GL_MIN_CHUNK;
    L.chunks = (C + L.chunk - 1) / L.chunk;
    L.sum_chunks = (C + FS_CHUNK - 1) / FS_CHUNK;
    L.off_part = c.take((size_t)L.sum_chunks * GL_COLS * sizeof(double));      // column-major: [column][chunk]
    L.off_pairs = c.take((size_t)C * 6 * sizeof(float));
    L.off_table = c.take((size_t)L.chunks * (size_t)T * sizeof(uint32_t));
    L.bytes = c.at;
    return L;
}

__device__ __forceinline__ float gl_sqrt(float x) { return (float)sqrt((double)x); }      // correctly rounded (see planes.hip)

struct GlTri {
    float l[3];                  // squared lengths of p1 - p0, p2 - p0, p2 - p1
    float u[3], v[3], w[3];
};

__device__ __forceinline__ GlTri gl_triangle(const float* __restrict__ xyz, long i0, long i1, long i2) {
    GlTri t;
    float p0[3], e1[3], e2[3], e3[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        p0[a] = xyz[3 * i0 + a];
        const float p1 = xyz[3 * i1 + a], p2 = xyz[3 * i2 + a];
        e1[a] = p1 - p0[a], e2[a] = p2 - p0[a], e3[a] = p2 - p1;
    }
    t.l[0] = (e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2];
    t.l[1] = (e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2];
    t.l[2] = (e3[0] * e3[0] + e3[1] * e3[1]) + e3[2] * e3[2];
    const float r = gl_sqrt(t.l[0]);
#pragma unroll
    for (int a = 0; a < 3; ++a) t.u[a] = __fdiv_rn(e1[a], r);
    const float c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const float rc = gl_sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a) t.w[a] = __fdiv_rn(c[a], rc);
    t.v[0] = t.w[1] * t.u[2] - t.w[2] * t.u[1];
    t.v[1] = t.w[2] * t.u[0] - t.w[0] * t.u[2];
    t.v[2] = t.w[0] * t.u[1] - t.w[1] * t.u[0];
    return t;
}

__global__ __launch_bounds__(GL_THREADS) void gl_hyp(const float* __restrict__ src, long C, const float* __restrict__ tgt, long Mt,
                                                     const int64_t* __restrict__ corr, const int64_t* __restrict__ tri, long T,
                                                     float s2, float* __restrict__ hyp, int32_t* __restrict__ bad_out) {
    const long t = (long)blockIdx.x * GL_THREADS + threadIdx.x;
    int bad = 0;
    if (t < T) {
        const float nan = __int_as_float(0x7fc00000);
        float out[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) out[e] = nan;
        const int64_t a0 = tri[3 * t], a1 = tri[3 * t + 1], a2 = tri[3 * t + 2];
        bool inside = a0 >= 0 && a0 < C && a1 >= 0 && a1 < C && a2 >= 0 && a2 < C;
        int64_t b0 = 0, b1 = 0, b2 = 0;
        if (inside) {
            b0 = corr[a0], b1 = corr[a1], b2 = corr[a2];
            inside = b0 >= 0 && b0 < Mt && b1 >= 0 && b1 < Mt && b2 >= 0 && b2 < Mt;
        }
        if (inside) {
            const GlTri A = gl_triangle(src, a0, a1, a2);
            const GlTri B = gl_triangle(tgt, b0, b1, b2);
            bool valid = true;
#pragma unroll
            for (int e = 0; e < 3; ++e)
                valid = valid && A.l[e] > 0.0f && B.l[e] > 0.0f && A.l[e] >= s2 * B.l[e] && B.l[e] >= s2 * A.l[e];
            float m[12];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int s = 0; s < 3; ++s) m[3 * r + s] = (B.u[r] * A.u[s] + B.v[r] * A.v[s]) + B.w[r] * A.w[s];
#pragma unroll
            for (int r = 0; r < 3; ++r)
                m[9 + r] = tgt[3 * b0 + r] - ((m[3 * r] * src[3 * a0] + m[3 * r + 1] * src[3 * a0 + 1]) + m[3 * r + 2] * src[3 * a0 + 2]);
#pragma unroll
            for (int e = 0; e < 12; ++e) valid = valid && fabsf(m[e]) <= GL_FLT_MAX;
            if (valid) {
#pragma unroll
                for (int e = 0; e < 12; ++e) out[e] = m[e];
            }
        } else {
            bad = 1;
        }
#pragma unroll
        for (int e = 0; e < 12; ++e) hyp[12 * t + e] = out[e];
    }
    const int any = __syncthreads_or(bad);
    if (threadIdx.x == 0) bad_out[blockIdx.x] = any ? 1 : 0;
}

// one workgroup: ORs the per-workgroup flags of gl_hyp into flag[0]
__global__ __launch_bounds__(GL_THREADS) void gl_flag(const int32_t* __restrict__ part, int n, int32_t* __restrict__ flag) {
    int bad = 0;
    for (int i = threadIdx.x; i < n; i += GL_THREADS) bad |= part[i];
    const int any = __syncthreads_or(bad);
    if (threadIdx.x == 0) flag[0] = any ? 1 : 0;
}

__global__ __launch_bounds__(GL_THREADS) void gl_pairs(const float* __restrict__ src, long C, const float* __restrict__ tgt, long Mt,
                                                       const int64_t* __restrict__ corr, float* __restrict__ pairs) {
    const long c = (long)blockIdx.x * GL_THREADS + threadIdx.x;
    if (c >= C) return;
    const int64_t jj = corr[c];
    const bool inside = jj >= 0 && jj < Mt;                  // (the caller's flag says so: nothing is read outside the target)
    const float nan = __int_as_float(0x7fc00000);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        pairs[6 * c + a] = src[3 * c + a];
        pairs[6 * c + 3 + a] = inside ? tgt[3 * jj + a] : nan;
    }
}

typedef float gl_f2 __attribute__((ext_vector_type(2)));

// one correspondence [a | b] (wave-uniform) against the lane's two hypotheses, side by side in the halves of packed operations
__device__ __forceinline__ void gl_test(const gl_f2 (&m)[12], const float* p, float g2, uint32_t& n0, uint32_t& n1) {
    const float x = p[0], y = p[1], z = p[2];
    const gl_f2 ex = (((m[0] * x + m[1] * y) + m[2] * z) + m[9]) - p[3];
    const gl_f2 ey = (((m[3] * x + m[4] * y) + m[5] * z) + m[10]) - p[4];
    const gl_f2 ez = (((m[6] * x + m[7] * y) + m[8] * z) + m[11]) - p[5];
    const gl_f2 e2 = (ex * ex + ey * ey) + ez * ez;
    n0 += e2.x <= g2 ? 1u : 0u;
    n1 += e2.y <= g2 ? 1u : 0u;
}

// grid (hypothesis groups, chunks), one wavefront each
__global__ __launch_bounds__(GL_LANES) void gl_count(const float* __restrict__ pairs, long C, const float* __restrict__ hyp, long T,
                                                     float g2, long chunk, uint32_t* __restrict__ table) {
    const int lane = threadIdx.x;
    const long t0 = (long)blockIdx.x * GL_GROUP + lane;       // the lane's hypotheses: t0 and t0 + 64
    const long t1 = t0 + GL_LANES;
    const float nan = __int_as_float(0x7fc00000);
    gl_f2 m[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        m[e].x = t0 < T ? hyp[12 * t0 + e] : nan;
        m[e].y = t1 < T ? hyp[12 * t1 + e] : nan;
    }
    uint32_t n0 = 0u, n1 = 0u;
    const long j0 = (long)blockIdx.y * chunk;
    const long j1 = min(C, j0 + chunk);
    const float* __restrict__ p = pairs + 6 * j0;
    long j = j0;
    for (; j + GL_UNROLL <= j1; j += GL_UNROLL, p += 6 * GL_UNROLL) {
        float q[6 * GL_UNROLL];
#pragma unroll
        for (int u = 0; u < 6 * GL_UNROLL; ++u) q[u] = p[u];
#pragma unroll
        for (int u = 0; u < GL_UNROLL; ++u) gl_test(m, q + 6 * u, g2, n0, n1);
    }
    for (; j < j1; ++j, p += 6) gl_test(m, p, g2, n0, n1);
    uint32_t* row = table + (long)blockIdx.y * T;
    if (t0 < T) row[t0] = n0;
    if (t1 < T) row[t1] = n1;
}

// one workgroup per 64 hypotheses
__global__ __launch_bounds__(GL_LANES * GL_SUM_WAVES) void gl_sum(const uint32_t* __restrict__ table, int chunks, long T,
                                                                  int32_t* __restrict__ counts) {
    __shared__ uint32_t part[GL_SUM_WAVES][GL_LANES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long t = (long)blockIdx.x * GL_LANES + lane;
    uint32_t s = 0;
    if (t < T)
        for (int c = w; c < chunks; c += GL_SUM_WAVES) s += table[(long)c * T + t];
    part[w][lane] = s;
    __syncthreads();
    if (w != 0 || t >= T) return;
    s = 0;
#pragma unroll
    for (int k = 0; k < GL_SUM_WAVES; ++k) s += part[k][lane];
    counts[t] = (int32_t)s;
}

struct GlRt {
    float m[12];
};

// one wavefront = one workgroup = chunk blockIdx.x of 1024 correspondences
__global__ __launch_bounds__(64) void gl_sums(const float* __restrict__ src, long C, const float* __restrict__ tgt, long Mt,
                                              const int64_t* __restrict__ corr, GlRt rt, float g2, uint8_t* __restrict__ inlier_out,
                                              long chunks, double* __restrict__ part) {
    const int lane = threadIdx.x;
    const long c = blockIdx.x;
    const long j0 = c * FS_CHUNK;
    double acc[GL_COLS];
#pragma unroll
    for (int e = 0; e < GL_COLS; ++e) acc[e] = 0.0;
#pragma unroll 2
    for (int t = 0; t < FS_TURNS; ++t) {
        const long i = j0 + t * 64 + lane;
        const bool live = i < C;
        const long ii = live ? i : j0;                     // (a dead lane reads the chunk's first row and adds +0.0)
        const long jj = corr[ii];
        const bool inside = jj >= 0 && jj < Mt;            // (the caller's flag says so: nothing is read outside the target)
        const long j = inside ? jj : 0;
        const float a[3] = {src[3 * ii], src[3 * ii + 1], src[3 * ii + 2]};
        const float b[3] = {tgt[3 * j], tgt[3 * j + 1], tgt[3 * j + 2]};
        float e[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            e[r] = (((rt.m[3 * r] * a[0] + rt.m[3 * r + 1] * a[1]) + rt.m[3 * r + 2] * a[2]) + rt.m[9 + r]) - b[r];
        const float e2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
        const bool in = live && inside && e2 <= g2;
        double s[GL_COLS];
        s[0] = 1.0;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            s[1 + u] = (double)a[u];
            s[4 + u] = (double)b[u];
#pragma unroll
            for (int v = 0; v < 3; ++v) s[7 + 3 * u + v] = (double)a[u] * (double)b[v];
        }
#pragma unroll
        for (int k = 0; k < GL_COLS; ++k) acc[k] = acc[k] + (in ? s[k] : 0.0);
        if (live) inlier_out[i] = in ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < GL_COLS; ++k) {
        const double s = fs_fold64(acc[k]);
        if (lane == 0) part[(long)k * chunks + c] = s;
    }
}

// wavefront b: column b's chunk sums by the same rule
__global__ __launch_bounds__(64) void gl_fold(const double* __restrict__ part, long chunks, double* __restrict__ out) {
    const int lane = threadIdx.x;
    const double* col = part + (long)blockIdx.x * chunks;
    double acc = 0.0;
    for (long c = lane; c < chunks; c += 64) acc = acc + col[c];
    const double s = fs_fold64(acc);
    if (lane == 0) out[blockIdx.x] = s;
}

bool gl_size_ok(int64_t C) { return C >= 3 && C < 0x7fffffffLL; }
bool gl_target_ok(int64_t Mt) { return Mt >= 1 && Mt < 0x7fffffffLL; }
bool gl_gate_ok(float g2) { return g2 > 0.0f && g2 <= GL_FLT_MAX; }

}  // namespace

extern "C" int64_t rl_global_workspace_bytes(int64_t C, int64_t T) {
    if (!gl_size_ok(C) || T < 1 || T > RL_GLOBAL_MAX_HYPOTHESES) return 0;
    return (int64_t)global_layout(C, T).bytes;
}

extern "C" int rl_global_hypotheses(const float* source, int64_t C, const float* target, int64_t Mt, const int64_t* corr,
                                    const int64_t* triples, int64_t T, float s2, float* hyp_out, int32_t* bad_out, void* ws,
                                    int64_t ws_bytes, void* stream) {
    RL_REQUIRE(gl_size_ok(C), RL_ERR_ARGS, "rl_global_hypotheses: C=%lld outside 3 .. 2^31-2", (long long)C);
    RL_REQUIRE(gl_target_ok(Mt), RL_ERR_ARGS, "rl_global_hypotheses: Mt=%lld outside 1 .. 2^31-2", (long long)Mt);
    RL_REQUIRE(T >= 1 && T <= RL_GLOBAL_MAX_HYPOTHESES, RL_ERR_ARGS, "rl_global_hypotheses: T=%lld outside 1 .. %d", (long long)T,
               RL_GLOBAL_MAX_HYPOTHESES);
    RL_REQUIRE(s2 >= 0.0f && s2 <= 1.0f, RL_ERR_ARGS, "rl_global_hypotheses: s2=%g outside 0 .. 1", (double)s2);
    int rc = rl_ws_check("rl_global_hypotheses", ws, ws_bytes, rl_global_workspace_bytes(C, T));
    if (rc) return rc;
    RL_REQUIRE(source && target && corr && triples && hyp_out && bad_out, RL_ERR_ARGS, "rl_global_hypotheses: null pointer");
    hipStream_t sm = (hipStream_t)stream;
    const GlLayout L = global_layout(C, T);
    int32_t* flags = rl_at<int32_t>(ws, L.off_table);        // (the table is not in use yet: T / 256 <= chunks * T words)
    const int blocks = rl_cdiv(T, GL_THREADS);
    hipLaunchKernelGGL(gl_hyp, dim3(blocks), dim3(GL_THREADS), 0, sm, source, (long)C, target, (long)Mt, corr, triples, (long)T, s2,
                       hyp_out, flags);
    RL_LAUNCH_CHECK("rl_global_hypotheses (hypotheses)");
    hipLaunchKernelGGL(gl_flag, dim3(1), dim3(GL_THREADS), 0, sm, (const int32_t*)flags, blocks, bad_out);
    rl_note_kernel("gl_hyp");
    RL_LAUNCH_CHECK("rl_global_hypotheses (flag)");
    return RL_OK;
}

extern "C" int rl_global_count(const float* source, int64_t C, const float* target, int64_t Mt, const int64_t* corr,
                               const float* hyp, int64_t T, float gate2, int32_t* counts_out, void* ws, int64_t ws_bytes,
                               void* stream) {
    RL_REQUIRE(gl_size_ok(C), RL_ERR_ARGS, "rl_global_count: C=%lld outside 3 .. 2^31-2", (long long)C);
    RL_REQUIRE(gl_target_ok(Mt), RL_ERR_ARGS, "rl_global_count: Mt=%lld outside 1 .. 2^31-2", (long long)Mt);
    RL_REQUIRE(T >= 1 && T <= RL_GLOBAL_MAX_HYPOTHESES, RL_ERR_ARGS, "rl_global_count: T=%lld outside 1 .. %d", (long long)T,
               RL_GLOBAL_MAX_HYPOTHESES);
    RL_REQUIRE(gl_gate_ok(gate2), RL_ERR_ARGS, "rl_global_count: gate2=%g is not a finite number > 0", (double)gate2);
    int rc = rl_ws_check("rl_global_count", ws, ws_bytes, rl_global_workspace_bytes(C, T));
    if (rc) return rc;
    RL_REQUIRE(source && target && corr && hyp && counts_out, RL_ERR_ARGS, "rl_global_count: null pointer");
    hipStream_t sm = (hipStream_t)stream;
    const GlLayout L = global_layout(C, T);
    float* pairs = rl_at<float>(ws, L.off_pairs);
    uint32_t* table = rl_at<uint32_t>(ws, L.off_table);
    hipLaunchKernelGGL(gl_pairs, dim3(rl_cdiv(C, GL_THREADS)), dim3(GL_THREADS), 0, sm, source, (long)C, target, (long)Mt, corr, pairs);
    RL_LAUNCH_CHECK("rl_global_count (pairs)");
    hipLaunchKernelGGL(gl_count, dim3(rl_cdiv(T, GL_GROUP), (unsigned)L.chunks), dim3(GL_LANES), 0, sm, (const float*)pairs, (long)C,
                       hyp, (long)T, gate2, L.chunk, table);
    RL_LAUNCH_CHECK("rl_global_count (count)");
    hipLaunchKernelGGL(gl_sum, dim3(rl_cdiv(T, GL_LANES)), dim3(GL_LANES * GL_SUM_WAVES), 0, sm, (const uint32_t*)table, (int)L.chunks,
                       (long)T, counts_out);
    rl_note_kernel("gl_count");
    RL_LAUNCH_CHECK("rl_global_count (sum)");
    return RL_OK;
}

extern "C" int rl_global_sums(const float* source, int64_t C, const float* target, int64_t Mt, const int64_t* corr, const float* rt,
                              float gate2, uint8_t* inlier_out, double* out, void* ws, int64_t ws_bytes, void* stream) {
    RL_REQUIRE(gl_size_ok(C), RL_ERR_ARGS, "rl_global_sums: C=%lld outside 3 .. 2^31-2", (long long)C);
    RL_REQUIRE(gl_target_ok(Mt), RL_ERR_ARGS, "rl_global_sums: Mt=%lld outside 1 .. 2^31-2", (long long)Mt);
    RL_REQUIRE(gl_gate_ok(gate2), RL_ERR_ARGS, "rl_global_sums: gate2=%g is not a finite number > 0", (double)gate2);
    int rc = rl_ws_check("rl_global_sums", ws, ws_bytes, rl_global_workspace_bytes(C, 1));
    if (rc) return rc;
    RL_REQUIRE(source && target && corr && rt && inlier_out && out, RL_ERR_ARGS, "rl_global_sums: null pointer");
    hipStream_t sm = (hipStream_t)stream;
    const GlLayout L = global_layout(C, 1);
    double* part = rl_at<double>(ws, L.off_part);
    GlRt m;
    for (int e = 0; e < 12; ++e) m.m[e] = rt[e];
    hipLaunchKernelGGL(gl_sums, dim3((unsigned)L.sum_chunks), dim3(64), 0, sm, source, (long)C, target, (long)Mt, corr, m, gate2,
                       inlier_out, L.sum_chunks, part);
    RL_LAUNCH_CHECK("rl_global_sums (sums)");
    hipLaunchKernelGGL(gl_fold, dim3(GL_COLS), dim3(64), 0, sm, (const double*)part, L.sum_chunks, out);
    rl_note_kernel("gl_sums");
    RL_LAUNCH_CHECK("rl_global_sums (fold)");
    return RL_OK;
}
