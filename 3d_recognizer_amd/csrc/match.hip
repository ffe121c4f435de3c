// Brute-force nearest neighbour in descriptor space (rl_match_u8; the numpy twin and the contract are
// randlanet/utils/features.py: match_features): for every source code row (36 bytes) the target row of the smallest
// sum_b (cs_b - ct_b)^2, ties to the lowest target index.  Everything is integer arithmetic - the distance is at most
// 33 * 255^2 < 2^22 -, so the result does not depend on any order of the work.
//
//   mt_norms    one lane per target row: nt_j = sum_b ct_b^2, nine packed dot products
//   mt_match    the hot path, Ms * Mt * 9 packed dot products: one wavefront per (64 source rows, slice of the targets).  A
//               lane holds its source row in nine registers; the target rows are wave-uniform (scalar loads, as planes.hip
//               feeds its points), so the inner loop is VALU work only: nine v_dot4_u32_u8 into one accumulator, then
//               key = nt_j - 2 * dot - the lane's own norm is the same for every j and is added at the end -, one compare and
//               two selects.  A strict < over ascending j keeps the lowest index.  Writes (key, j) of the slice
//   mt_combine  one lane per source row: the lexicographic minimum of (key, j) over the slices in ascending order - the slices
//               are ascending index ranges, so a strict < again keeps the lowest index -, plus the row's own norm
// No atomics, no workgroup waits for another one; the slices make the grid large enough for the chip when Ms is small and do
// not change the result.
#include "rl_common.h"

namespace {

constexpr int MT_WORDS = 9;                 // 36 bytes of a code row
constexpr int MT_THREADS = 256;             // mt_norms, mt_combine
constexpr int MT_UNROLL = 4;
constexpr long MT_MIN_SLICE = 256;          // target rows of a slice at least (but for the last)
constexpr long MT_MAX_SLICES = 64;
constexpr long MT_WAVES = 4096;             // wavefronts aimed at: four per SIMD

struct MtLayout {
    long slices, slice;                     // number of slices, target rows per slice
    size_t off_norm, off_key, off_idx, bytes;
};

MtLayout match_layout(long Ms, long Mt) {
    MtLayout L;
    RlCarve c;
    const long groups = (Ms + 63) / 64;
    long want = (MT_WAVES + groups - 1) / groups;
    const long most = (Mt + MT_MIN_SLICE - 1) / MT_MIN_SLICE;
    want = want > MT_MAX_SLICES ? MT_MAX_SLICES : want;
    want = want > most ? most : want;
    want = want < 1 ? 1 : want;
    L.slice = (Mt + want - 1) / want;
    L.slices = (Mt + L.slice - 1) / L.slice;
    L.off_norm = c.take((size_t)Mt * sizeof(int32_t));
    L.off_key = c.take((size_t)L.slices * (size_t)Ms * sizeof(int32_t));
    L.off_idx = c.take((size_t)L.slices * (size_t)Ms * sizeof(int32_t));
    L.bytes = c.at;
    return L;
}

__device__ __forceinline__ uint32_t mt_dot(uint32_t a, uint32_t b, uint32_t c) {
#if __has_builtin(__builtin_amdgcn_udot4)
    return __builtin_amdgcn_udot4(a, b, c, false);
#else
    return c + (a & 255u) * (b & 255u) + ((a >> 8) & 255u) * ((b >> 8) & 255u) + ((a >> 16) & 255u) * ((b >> 16) & 255u) +
           (a >> 24) * (b >> 24);
#endif
}

__global__ __launch_bounds__(MT_THREADS) void mt_norms(const uint32_t* __restrict__ code, long M, int32_t* __restrict__ norm) {
    const long j = (long)blockIdx.x * MT_THREADS + threadIdx.x;
    if (j >= M) return;
    uint32_t n = 0;
#pragma unroll
    for (int w = 0; w < MT_WORDS; ++w) {
        const uint32_t v = code[j * MT_WORDS + w];
        n = mt_dot(v, v, n);
    }
    norm[j] = (int32_t)n;
}

// one target row (wave-uniform words t[0..8], norm nt) against the lane's source row
__device__ __forceinline__ void mt_test(const uint32_t (&s)[MT_WORDS], const uint32_t* t, int32_t nt, int32_t j, int32_t& best,
                                        int32_t& at) {
    uint32_t dot = 0;
#pragma unroll
    for (int w = 0; w < MT_WORDS; ++w) dot = mt_dot(s[w], t[w], dot);
    const int32_t key = nt - 2 * (int32_t)dot;              // (|key| < 2^23)
    const bool less = key < best;
    best = less ? key : best;
    at = less ? j : at;
}

// grid (source groups, slices), one wavefront each
__global__ __launch_bounds__(64) void mt_match(const uint32_t* __restrict__ src, long Ms, const uint32_t* __restrict__ tgt, long Mt,
                                               const int32_t* __restrict__ norm, long slice, int32_t* __restrict__ key_out,
                                               int32_t* __restrict__ idx_out) {
    const long i = (long)blockIdx.x * 64 + threadIdx.x;
    const long ii = i < Ms ? i : Ms - 1;                     // (a dead lane follows the last row and writes nothing)
    uint32_t s[MT_WORDS];
#pragma unroll
    for (int w = 0; w < MT_WORDS; ++w) s[w] = src[ii * MT_WORDS + w];
    const long j0 = (long)blockIdx.y * slice;
    const long j1 = min(Mt, j0 + slice);
    int32_t best = 0x7fffffff, at = (int32_t)j0;
    const uint32_t* __restrict__ p = tgt + j0 * MT_WORDS;
    long j = j0;
    for (; j + MT_UNROLL <= j1; j += MT_UNROLL, p += MT_UNROLL * MT_WORDS) {
        uint32_t t[MT_UNROLL * MT_WORDS];
        int32_t nt[MT_UNROLL];
#pragma unroll
        for (int u = 0; u < MT_UNROLL * MT_WORDS; ++u) t[u] = p[u];
#pragma unroll
        for (int u = 0; u < MT_UNROLL; ++u) nt[u] = norm[j + u];
#pragma unroll
        for (int u = 0; u < MT_UNROLL; ++u) mt_test(s, t + u * MT_WORDS, nt[u], (int32_t)(j + u), best, at);
    }
    for (; j < j1; ++j, p += MT_WORDS) mt_test(s, p, norm[j], (int32_t)j, best, at);
    if (i < Ms) {
        key_out[(long)blockIdx.y * Ms + i] = best;
        idx_out[(long)blockIdx.y * Ms + i] = at;
    }
}

__global__ __launch_bounds__(MT_THREADS) void mt_combine(const uint32_t* __restrict__ src, long Ms, const int32_t* __restrict__ key,
                                                         const int32_t* __restrict__ idx, int slices, int64_t* __restrict__ idx_out,
                                                         int32_t* __restrict__ dist_out) {
    const long i = (long)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i >= Ms) return;
    int32_t best = key[i], at = idx[i];
    for (int c = 1; c < slices; ++c) {
        const int32_t k = key[(long)c * Ms + i];
        const bool less = k < best;                          // (slice c holds larger indices than the slices before it)
        at = less ? idx[(long)c * Ms + i] : at;
        best = less ? k : best;
    }
    uint32_t n = 0;
#pragma unroll
    for (int w = 0; w < MT_WORDS; ++w) {
        const uint32_t v = src[i * MT_WORDS + w];
        n = mt_dot(v, v, n);
    }
    idx_out[i] = (int64_t)at;
    dist_out[i] = (int32_t)n + best;
}

bool mt_size_ok(int64_t M) { return M >= 1 && M < 0x7fffffffLL; }

}  // namespace

extern "C" int64_t rl_match_workspace_bytes(int64_t Ms, int64_t Mt) {
    if (!mt_size_ok(Ms) || !mt_size_ok(Mt)) return 0;
    return (int64_t)match_layout(Ms, Mt).bytes;
}

extern "C" int rl_match_u8(const uint8_t* code_source, int64_t Ms, const uint8_t* code_target, int64_t Mt, int64_t* idx_out,
                           int32_t* dist_out, void* ws, int64_t ws_bytes, void* stream) {
    RL_REQUIRE(mt_size_ok(Ms), RL_ERR_ARGS, "rl_match_u8: Ms=%lld outside 1 .. 2^31-2", (long long)Ms);
    RL_REQUIRE(mt_size_ok(Mt), RL_ERR_ARGS, "rl_match_u8: Mt=%lld outside 1 .. 2^31-2", (long long)Mt);
    int rc = rl_ws_check("rl_match_u8", ws, ws_bytes, rl_match_workspace_bytes(Ms, Mt));
    if (rc) return rc;
    RL_REQUIRE(code_source && code_target && idx_out && dist_out, RL_ERR_ARGS, "rl_match_u8: null pointer");
    RL_REQUIRE(((uintptr_t)code_source & 3) == 0 && ((uintptr_t)code_target & 3) == 0, RL_ERR_ARGS,
               "rl_match_u8: codes not 4-byte aligned");
    hipStream_t sm = (hipStream_t)stream;
    const MtLayout L = match_layout(Ms, Mt);
    int32_t* norm = rl_at<int32_t>(ws, L.off_norm);
    int32_t* key = rl_at<int32_t>(ws, L.off_key);
    int32_t* idx = rl_at<int32_t>(ws, L.off_idx);
    const uint32_t* src = (const uint32_t*)code_source;
    const uint32_t* tgt = (const uint32_t*)code_target;
    hipLaunchKernelGGL(mt_norms, dim3(rl_cdiv(Mt, MT_THREADS)), dim3(MT_THREADS), 0, sm, tgt, (long)Mt, norm);
    RL_LAUNCH_CHECK("rl_match_u8 (norms)");
    hipLaunchKernelGGL(mt_match, dim3(rl_cdiv(Ms, 64), (unsigned)L.slices), dim3(64), 0, sm, src, (long)Ms, tgt, (long)Mt,
                       (const int32_t*)norm, L.slice, key, idx);
    RL_LAUNCH_CHECK("rl_match_u8 (match)");
    hipLaunchKernelGGL(mt_combine, dim3(rl_cdiv(Ms, MT_THREADS)), dim3(MT_THREADS), 0, sm, src, (long)Ms, (const int32_t*)key,
                       (const int32_t*)idx, (int)L.slices, idx_out, dist_out);
    rl_note_kernel("mt_match");
    RL_LAUNCH_CHECK("rl_match_u8 (combine)");
    return RL_OK;
}
