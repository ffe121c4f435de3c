// Voted-crop inference over a whole scene (Model.predict_scene): the per-crop pick / select / gather / update and the
// per-crop probability blend of RandLA-Net's test protocol (Hu et al., CVPR 2020; the authors' S3DIS / Semantic3D
// testers), kept on the device between forwards.  The numpy twin of every step is randlanet/utils/scene.py.
//
// One crop (rl_scene_crop), M points, n = crop size, six launches, no host synchronisation:
//   pick_partial   per-workgroup min of the 64-bit key (ordered bits(possibility) << 32 | index) -> ties go to the
//                  lowest index; workgroup 0 also clears the three radix histograms of this crop
//   d2_hist        every workgroup folds the partial keys to the centre c, computes d2_i = ((dx*dx)+(dy*dy))+(dz*dz)
//                  (the KNN's expression, no FMA), stores bits(d2_i) (non-negative fp32 bits are monotone as uint32)
//                  and histograms the top 11 bits (LDS histogram per workgroup, integer atomics into the global one)
//   radix_hist x2  resolve the previous digit (the bin the n-th smallest key falls in, and its rank inside the bin),
//                  histogram the next 11 / 10 bits of the keys that share the resolved prefix
//   count          resolve the last digit: T = the n-th smallest d2 bits, k_eq = how many keys == T are taken;
//                  count keys < T and == T per workgroup (contiguous chunks of the index range)
//   write          the crop = every key < T plus the k_eq lowest-indexed keys == T, written in ascending index order
//                  (exclusive prefix over the workgroups' counts, then wave ballots inside a chunk); the same launch
//                  gathers cloud row i into rows_out[pos] and adds (1 - d2_i / d2max)^2 to possibility[i], d2max = T
//                  (the largest d2 of the crop; T == 0 -> every selected point is at the centre: delta 1)
// Everything is integer or a fixed fp32 expression, so the crop sequence is bit-identical to the twin's.
//
// Padded crops (rl_scene_crop_padded, rl_scenes_crop_padded): a scene of M < n points.  The same six launches select
// min(n, M) = M keys, so T is the largest d2 of the scene, every point is written to slot i and raised once; the slots
// j >= M then hold row j mod M (cyclic repeats), each a function of (base, M, j) alone, written by a grid-stride loop of
// the write launch - no workgroup waits for another.  With M >= n the launches are the unpadded ones.
#include <algorithm>

#include "rl_common.h"
#include "rl_fixed.h"

namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_WAVES = SC_THREADS / 64;
constexpr int SC_BINS = 2048;           // 11-bit digits (the last one has 10 bits: 1024 bins used)
constexpr int SC_MAX_PICK = 1024;       // workgroups of pick_partial
constexpr int SC_MAX_GROUPS = 2048;     // workgroups of the select passes (contiguous chunks)
constexpr int SC_MAX_MIN = 1024;        // workgroups of the min-count reduction

struct SceneState {
    uint32_t centre;
    uint32_t b0, k0;      // digit 0 (bits 31..21) of the n-th key and the rank left inside its bin
    uint32_t b1, k1;      // digit 1 (bits 20..10)
    uint32_t T, k_eq;     // the n-th key, and how many keys equal to it the crop takes
    uint32_t pad[9];
};

// the workspace of one scene: the SceneState at offset 0; only the keys depend on M, and they come last
struct SceneWs { size_t off_pick, off_hist, off_cnt, off_min, off_keys, bytes; };

SceneWs scene_ws(long M) {
    SceneWs W;
    RlCarve c;
    c.take(sizeof(SceneState));
    W.off_pick = c.take(SC_MAX_PICK * sizeof(uint64_t));
    W.off_hist = c.take(3 * SC_BINS * sizeof(uint32_t));
    W.off_cnt = c.take(2 * SC_MAX_GROUPS * sizeof(uint32_t));
    W.off_min = c.take(SC_MAX_MIN * sizeof(int32_t));
    W.off_keys = c.take((size_t)M * sizeof(uint32_t));
    W.bytes = c.at;
    return W;
}

struct Layout {
    int groups;   // select-pass workgroups
    long chunk;   // points per workgroup (multiple of SC_THREADS)
    int pick;     // pick_partial workgroups
};

__host__ __device__ Layout layout(long M) {
    Layout L;
    long g = (M + 4 * SC_THREADS - 1) / (4 * SC_THREADS);
    if (g > SC_MAX_GROUPS) g = SC_MAX_GROUPS;
    if (g < 1) g = 1;
    L.chunk = ((M + g - 1) / g + SC_THREADS - 1) / SC_THREADS * SC_THREADS;
    L.groups = (int)((M + L.chunk - 1) / L.chunk);
    long p = (M + 8 * SC_THREADS - 1) / (8 * SC_THREADS);
    L.pick = (int)(p > SC_MAX_PICK ? SC_MAX_PICK : (p < 1 ? 1 : p));
    return L;
}

// total order of fp32 values as uint32 (negative values included; the possibilities are non-negative in practice)
__device__ __forceinline__ uint32_t ordered_bits(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}

__device__ uint64_t block_min_u64(uint64_t v) {
    __shared__ uint64_t part[SC_WAVES];
    v = wave_min_u64(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) part[w] = v;
    __syncthreads();
    uint64_t r = part[0];
#pragma unroll
    for (int i = 1; i < SC_WAVES; ++i) r = part[i] < r ? part[i] : r;
    return r;
}

__device__ uint32_t block_sum_u32(uint32_t v) {
    __shared__ uint32_t part[SC_WAVES];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) part[w] = v;
    __syncthreads();
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < SC_WAVES; ++i) r += part[i];
    return r;
}

// The bin of hist[0..nbins) that holds the k-th smallest key (1-based), and k minus the keys in the bins below it.
// Every thread returns the same pair.
__device__ void resolve_digit(const uint32_t* __restrict__ hist, int nbins, uint32_t k, uint32_t& bin, uint32_t& rank) {
    __shared__ uint32_t scan[SC_THREADS];
    __shared__ uint32_t res[2];
    const int per = nbins / SC_THREADS;            // 8 or 4 bins per thread
    const int t = threadIdx.x;
    uint32_t s = 0;
    for (int j = 0; j < per; ++j) s += hist[t * per + j];
    __syncthreads();
    scan[t] = s;
    __syncthreads();
    for (int o = 1; o < SC_THREADS; o <<= 1) {     // inclusive Hillis-Steele scan
        const uint32_t add = t >= o ? scan[t - o] : 0u;
        __syncthreads();
        scan[t] += add;
        __syncthreads();
    }
    if (t == 0) res[0] = 0, res[1] = 1;
    __syncthreads();
    uint32_t below = scan[t] - s;
    if (below < k && k <= scan[t]) {               // exactly one thread: the counts add up to at least k
        for (int j = 0; j < per; ++j) {
            const uint32_t h = hist[t * per + j];
            if (k <= below + h) {
                res[0] = (uint32_t)(t * per + j);
                res[1] = k - below;
                break;
            }
            below += h;
        }
    }
    __syncthreads();
    bin = res[0];
    rank = res[1];
}

__global__ __launch_bounds__(SC_THREADS) void scene_pick_partial(const float* __restrict__ poss, long M,
                                                                  uint64_t* __restrict__ partial, uint32_t* __restrict__ hist) {
    uint64_t best = ~0ull;
    for (long i = (long)blockIdx.x * SC_THREADS + threadIdx.x; i < M; i += (long)gridDim.x * SC_THREADS) {
        const uint64_t key = ((uint64_t)ordered_bits(poss[i]) << 32) | (uint32_t)i;
        best = key < best ? key : best;
    }
    best = block_min_u64(best);
    if (threadIdx.x == 0) partial[blockIdx.x] = best;
    if (blockIdx.x == 0)
        for (int j = threadIdx.x; j < 3 * SC_BINS; j += SC_THREADS) hist[j] = 0u;
}

// d2 of the points [i0, i1) of `cloud` (rows `dim` floats apart) to (cx, cy, cz), their bits into keys, the top 11 bits
// histogrammed into hist[0]
__device__ void d2_hist_body(const float* __restrict__ cloud, long i0, long i1, int dim, float cx, float cy, float cz,
                             uint32_t* __restrict__ keys, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[SC_BINS];
    for (int j = threadIdx.x; j < SC_BINS; j += SC_THREADS) h[j] = 0u;
    __syncthreads();
    for (long i = i0 + threadIdx.x; i < i1; i += SC_THREADS) {
        const float* p = cloud + i * dim;
        const float dx = __fsub_rn(cx, p[0]), dy = __fsub_rn(cy, p[1]), dz = __fsub_rn(cz, p[2]);
        const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
        const uint32_t key = __float_as_uint(d2);
        keys[i] = key;
        atomicAdd(&h[key >> 21], 1u);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < SC_BINS; j += SC_THREADS)
        if (h[j]) atomicAdd(&hist[j], h[j]);
}

__global__ __launch_bounds__(SC_THREADS) void scene_d2_hist(const float* __restrict__ cloud, long M, int dim,
                                                             const uint64_t* __restrict__ partial, int npick,
                                                             uint32_t* __restrict__ keys, uint32_t* __restrict__ hist,
                                                             SceneState* __restrict__ st, long chunk) {
    uint64_t best = ~0ull;
    for (int j = threadIdx.x; j < npick; j += SC_THREADS) best = partial[j] < best ? partial[j] : best;
    best = block_min_u64(best);
    const long c = (long)(uint32_t)(best & 0xffffffffull);
    if (blockIdx.x == 0 && threadIdx.x == 0) st->centre = (uint32_t)c;
    const long i0 = (long)blockIdx.x * chunk;
    d2_hist_body(cloud, i0, min(M, i0 + chunk), dim, cloud[c * dim + 0], cloud[c * dim + 1], cloud[c * dim + 2], keys,
                 hist);
}

// level 1: resolve digit 0 from hist[0], histogram bits 20..10 of the keys in that bin into hist[1]
// level 2: resolve digit 1 from hist[1] (digit 0 from st), histogram bits 9..0 of the keys in that bin into hist[2]
__device__ void radix_hist_body(const uint32_t* __restrict__ keys, long M, int level, uint32_t n,
                                uint32_t* __restrict__ hist, SceneState* __restrict__ st, long chunk) {
    __shared__ uint32_t h[SC_BINS];
    for (int j = threadIdx.x; j < SC_BINS; j += SC_THREADS) h[j] = 0u;
    uint32_t bin, rank, prefix;
    int shift, mask;
    if (level == 1) {
        resolve_digit(hist, SC_BINS, n, bin, rank);
        if (blockIdx.x == 0 && threadIdx.x == 0) st->b0 = bin, st->k0 = rank;
        prefix = bin;                 // keys >> 21
        shift = 21;
        mask = SC_BINS - 1;
    } else {
        const uint32_t b0 = st->b0, k0 = st->k0;
        resolve_digit(hist + SC_BINS, SC_BINS, k0, bin, rank);
        if (blockIdx.x == 0 && threadIdx.x == 0) st->b1 = bin, st->k1 = rank;
        prefix = (b0 << 11) | bin;    // keys >> 10
        shift = 10;
        mask = 1023;
    }
    uint32_t* out = hist + level * SC_BINS;
    const int lo_shift = level == 1 ? 10 : 0;
    const long i0 = (long)blockIdx.x * chunk;
    const long i1 = min(M, i0 + chunk);
    for (long i = i0 + threadIdx.x; i < i1; i += SC_THREADS) {
        const uint32_t key = keys[i];
        if ((key >> shift) == prefix) atomicAdd(&h[(key >> lo_shift) & mask], 1u);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < SC_BINS; j += SC_THREADS)
        if (h[j]) atomicAdd(&out[j], h[j]);
}

__global__ __launch_bounds__(SC_THREADS) void scene_radix_hist(const uint32_t* __restrict__ keys, long M, int level,
                                                                uint32_t n, uint32_t* __restrict__ hist,
                                                                SceneState* __restrict__ st, long chunk) {
    radix_hist_body(keys, M, level, n, hist, st, chunk);
}

__device__ void count_body(const uint32_t* __restrict__ keys, long M, const uint32_t* __restrict__ hist,
                           SceneState* __restrict__ st, uint32_t* __restrict__ cnt, int groups, long chunk) {
    uint32_t b2, k_eq;
    resolve_digit(hist + 2 * SC_BINS, 1024, st->k1, b2, k_eq);
    const uint32_t T = (st->b0 << 21) | (st->b1 << 10) | b2;
    if (blockIdx.x == 0 && threadIdx.x == 0) st->T = T, st->k_eq = k_eq;
    uint32_t lt = 0, eq = 0;
    const long i0 = (long)blockIdx.x * chunk;
    const long i1 = min(M, i0 + chunk);
    for (long i = i0 + threadIdx.x; i < i1; i += SC_THREADS) {
        const uint32_t key = keys[i];
        lt += key < T;
        eq += key == T;
    }
    lt = block_sum_u32(lt);
    eq = block_sum_u32(eq);
    if (threadIdx.x == 0) cnt[blockIdx.x] = lt, cnt[groups + blockIdx.x] = eq;
}

__global__ __launch_bounds__(SC_THREADS) void scene_count(const uint32_t* __restrict__ keys, long M,
                                                           const uint32_t* __restrict__ hist, SceneState* __restrict__ st,
                                                           uint32_t* __restrict__ cnt, int groups, long chunk) {
    count_body(keys, M, hist, st, cnt, groups, chunk);
}

// The crop's points of this workgroup's chunk in ascending index order: emit(pos, i) for each, and the possibility update.
// Returns this thread's smallest (ordered bits(possibility after the update), base + i) over the whole chunk when
// kRefresh (the per-scene minimum of rl_scenes_crop), ~0 otherwise.
template <bool kRefresh, class Emit>
__device__ uint64_t write_body(long M, const uint32_t* __restrict__ keys, const SceneState* __restrict__ st,
                               const uint32_t* __restrict__ cnt, int groups, long chunk, float* __restrict__ poss, int n,
                               long base, Emit emit) {
    __shared__ uint32_t wl[SC_WAVES], we[SC_WAVES];
    const uint32_t T = st->T, k_eq = st->k_eq;
    const float dmax = __uint_as_float(T);
    // exclusive prefix of the counts of the workgroups before this one
    uint32_t lt = 0, eq = 0;
    for (int g = threadIdx.x; g < (int)blockIdx.x; g += SC_THREADS) lt += cnt[g], eq += cnt[groups + g];
    uint32_t run_lt = block_sum_u32(lt), run_eq = block_sum_u32(eq);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
    uint64_t best = ~0ull;
    const long i0 = (long)blockIdx.x * chunk;
    const long i1 = min(M, i0 + chunk);
    for (long t0 = i0; t0 < i1; t0 += SC_THREADS) {           // tiles of 256 points in index order
        const long i = t0 + threadIdx.x;
        const uint32_t key = i < i1 ? keys[i] : 0xffffffffu;
        const bool is_lt = i < i1 && key < T, is_eq = i < i1 && key == T;
        const uint64_t blt = __ballot(is_lt), beq = __ballot(is_eq);
        if (lane == 0) wl[w] = (uint32_t)__popcll(blt), we[w] = (uint32_t)__popcll(beq);
        __syncthreads();
        uint32_t lt_before = run_lt + (uint32_t)__popcll(blt & below);
        uint32_t eq_before = run_eq + (uint32_t)__popcll(beq & below);
        uint32_t tl = 0, te = 0;
#pragma unroll
        for (int v = 0; v < SC_WAVES; ++v) {
            if (v < w) lt_before += wl[v], eq_before += we[v];
            tl += wl[v];
            te += we[v];
        }
        __syncthreads();
        run_lt += tl;
        run_eq += te;
        const long pos = (long)lt_before + (long)min(eq_before, k_eq);
        if ((is_lt || (is_eq && eq_before < k_eq)) && pos < n) {      // (pos < n always: the histograms count n)
            emit(pos, i);
            const float r = T == 0u ? 0.f : __fdiv_rn(__uint_as_float(key), dmax);
            const float one_m = __fsub_rn(1.f, r);
            const float p = __fadd_rn(poss[i], __fmul_rn(one_m, one_m));
            poss[i] = p;
            if (kRefresh) {
                const uint64_t k = ((uint64_t)ordered_bits(p) << 32) | (uint32_t)(base + i);
                best = k < best ? k : best;
            }
        } else if (kRefresh && i < i1) {
            const uint64_t k = ((uint64_t)ordered_bits(poss[i]) << 32) | (uint32_t)(base + i);
            best = k < best ? k : best;
        }
    }
    return best;
}

__global__ __launch_bounds__(SC_THREADS) void scene_write(const float* __restrict__ cloud, long M, int dim,
                                                           const uint32_t* __restrict__ keys,
                                                           const SceneState* __restrict__ st,
                                                           const uint32_t* __restrict__ cnt, int groups, long chunk,
                                                           float* __restrict__ poss, float* __restrict__ rows,
                                                           long row_stride, int32_t* __restrict__ idx_out, int n) {
    auto emit = [&](long pos, long i) {
        idx_out[pos] = (int32_t)i;
        const float* src = cloud + i * dim;
        float* dst = rows + pos * row_stride;
        for (int c = 0; c < dim; ++c) dst[c] = src[c];
    };
    // the repeats of a padded crop (M < n: the select took every point, slot i = row i): slot j = row j mod M
    for (long j = M + (long)blockIdx.x * SC_THREADS + threadIdx.x; j < n; j += (long)gridDim.x * SC_THREADS)
        emit(j, (long)((uint32_t)j % (uint32_t)M));
    if ((int)blockIdx.x >= groups) return;         // (the workgroups a padded crop launches for its repeats only)
    write_body<false>(M, keys, st, cnt, groups, chunk, poss, n, 0, emit);
}

// exp_fixed (rl_fixed.h): e^x for x <= 0 as a fixed sequence of fp32 operations, the bits of utils/scene.py: exp_fixed

// one thread per crop point: softmax over the C classes of the first n columns of logits (C, ld), then the blend.
// FIXED false (rl_scene_accumulate): rl_softmax_cf's expression, the library's expf.  FIXED true
// (rl_scene_accumulate_first): exp_fixed, the twin's bits.
template <bool FIXED>
__global__ __launch_bounds__(SC_THREADS) void scene_accumulate(const float* __restrict__ logits, int C, int n, long ld,
                                                                const int32_t* __restrict__ idx, float oms, float s,
                                                                float* __restrict__ prob, int32_t* __restrict__ count,
                                                                long M) {
    const int j = blockIdx.x * SC_THREADS + threadIdx.x;
    if (j >= n) return;
    const long i = idx[j];
    if (i < 0 || i >= M) return;
    const float* z = logits + j;
    auto ex = [](float x) { return FIXED ? exp_fixed(x) : expf(x); };
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, z[(long)c * ld]);
    float den = 0.f;
    for (int c = 0; c < C; ++c) den = __fadd_rn(den, ex(__fsub_rn(z[(long)c * ld], m)));
    float* p = prob + i * C;
    for (int c = 0; c < C; ++c) {
        const float sm = __fdiv_rn(ex(__fsub_rn(z[(long)c * ld], m)), den);
        p[c] = __fadd_rn(__fmul_rn(s, p[c]), __fmul_rn(oms, sm));
    }
    count[i] += 1;
}

__global__ __launch_bounds__(SC_THREADS) void scene_min_partial(const int32_t* __restrict__ count, long M,
                                                                 int32_t* __restrict__ part) {
    int32_t v = 0x7fffffff;
    for (long i = (long)blockIdx.x * SC_THREADS + threadIdx.x; i < M; i += (long)gridDim.x * SC_THREADS)
        v = min(v, count[i]);
    // int32 counts are >= 0: the unsigned key order is the signed order
    const uint64_t r = block_min_u64((uint64_t)(uint32_t)v);
    if (threadIdx.x == 0) part[blockIdx.x] = (int32_t)r;
}

__global__ __launch_bounds__(SC_THREADS) void scene_min_final(const int32_t* __restrict__ part, int nparts,
                                                               int32_t* __restrict__ out) {
    int32_t v = 0x7fffffff;
    for (int j = threadIdx.x; j < nparts; j += SC_THREADS) v = min(v, part[j]);
    const uint64_t r = block_min_u64((uint64_t)(uint32_t)v);
    if (threadIdx.x == 0) out[0] = (int32_t)r;
}


// ---- many scenes (rl_scenes_*, the training crops of Model.train_scenes) -----------------------------------------------------
// The scenes are concatenated: scene s owns rows [off[s], off[s+1]) of xyz.  The picked scene's range lives in the workspace,
// so every select pass is launched for the largest scene and the workgroups past the picked scene's extent exit; the passes
// touch the picked scene only.  One 64-bit key per scene, (ordered bits(possibility) << 32) | global row, is the minimum of
// that scene: the pick folds the S keys, and the crop's write pass refreshes the key of the scene it changed.

struct ScenesState {
    SceneState sel;          // the select passes' state (centre = the picked global row)
    float cx, cy, cz;        // the crop centre: xyz[g] + noise
    int32_t s;               // the picked scene
    int64_t base, M;         // its rows [base, base + M)
    int64_t chunk;
    int32_t groups;
    int32_t S;
    int64_t max_points;
    uint32_t n_sel;          // how many keys the select passes take: n, or min(n, M) for a padded crop
};

// the workspace of many scenes: the ScenesState at offset 0
struct ScenesWs { size_t off_scene_min, off_offsets, off_hist, off_cnt, off_keys, bytes; };

ScenesWs scenes_ws(int S, long max_points) {
    ScenesWs W;
    RlCarve c;
    c.take(sizeof(ScenesState));
    W.off_scene_min = c.take((size_t)S * sizeof(uint64_t));
    W.off_offsets = c.take((size_t)(S + 1) * sizeof(int64_t));
    W.off_hist = c.take(3 * SC_BINS * sizeof(uint32_t));
    W.off_cnt = c.take(2 * SC_MAX_GROUPS * sizeof(uint32_t));
    W.off_keys = c.take((size_t)max_points * sizeof(uint32_t));
    W.bytes = c.at;
    return W;
}

constexpr int SS_INIT_PARTS = 64;    // workgroups per scene of the initial minima

// the offsets into the workspace, every scene's key to ~0
__global__ __launch_bounds__(SC_THREADS) void scenes_init_state(const int64_t* __restrict__ off, int S, int64_t max_points,
                                                                 ScenesState* __restrict__ st, int64_t* __restrict__ off_ws,
                                                                 uint64_t* __restrict__ scene_min) {
    for (int j = blockIdx.x * SC_THREADS + threadIdx.x; j <= S; j += gridDim.x * SC_THREADS) {
        off_ws[j] = off[j];
        if (j < S) scene_min[j] = ~0ull;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) st->S = S, st->max_points = max_points;
}

// grid (SS_INIT_PARTS, S): the minimum key of every scene
__global__ __launch_bounds__(SC_THREADS) void scenes_init_min(const float* __restrict__ poss,
                                                               const int64_t* __restrict__ off_ws,
                                                               uint64_t* __restrict__ scene_min) {
    const int s = blockIdx.y;
    const long b = off_ws[s], e = off_ws[s + 1];
    uint64_t best = ~0ull;
    for (long i = b + (long)blockIdx.x * SC_THREADS + threadIdx.x; i < e; i += (long)gridDim.x * SC_THREADS) {
        const uint64_t key = ((uint64_t)ordered_bits(poss[i]) << 32) | (uint32_t)i;
        best = key < best ? key : best;
    }
    best = block_min_u64(best);
    if (threadIdx.x == 0 && best != ~0ull) atomicMin((unsigned long long*)&scene_min[s], (unsigned long long)best);
}

// one workgroup: g = the least key over the scenes, s = its scene; the crop's centre, range and layout; the three radix
// histograms cleared; scene s's key cleared for the write pass to refresh
__global__ __launch_bounds__(SC_THREADS) void scenes_pick(const float* __restrict__ xyz, int stride,
                                                           const float* __restrict__ noise, ScenesState* __restrict__ st,
                                                           uint64_t* __restrict__ scene_min, const int64_t* __restrict__ off,
                                                           uint32_t* __restrict__ hist, int64_t* __restrict__ scene_out,
                                                           int n, int pad) {
    __shared__ int picked;
    const int S = st->S;
    uint64_t best = ~0ull;
    for (int j = threadIdx.x; j < S; j += SC_THREADS) best = scene_min[j] < best ? scene_min[j] : best;
    best = block_min_u64(best);
    if (threadIdx.x == 0) picked = 0;
    for (int j = threadIdx.x; j < 3 * SC_BINS; j += SC_THREADS) hist[j] = 0u;
    __syncthreads();
    for (int j = threadIdx.x; j < S; j += SC_THREADS)
        if (scene_min[j] == best) picked = j;          // keys of different scenes differ in their row: one writer
    __syncthreads();
    if (threadIdx.x == 0) {
        const int s = picked;
        const long base = off[s];
        long M = off[s + 1] - base;
        M = M < 0 ? 0 : (M > st->max_points ? st->max_points : M);     // (keys hold max_points: never past them)
        long g = (long)(uint32_t)(best & 0xffffffffull);
        if (best == ~0ull || g < base || g >= base + M) g = base;        // (a workspace rl_scenes_init never saw)
        const Layout L = layout(M > 0 ? M : 1);
        st->s = s;
        st->base = base;
        st->M = M;
        st->chunk = L.chunk;
        st->groups = M > 0 ? L.groups : 0;
        st->n_sel = (uint32_t)(pad && M < n ? M : n);
        st->sel.centre = (uint32_t)g;
        const float* p = xyz + g * (long)stride;
        st->cx = noise ? __fadd_rn(p[0], noise[0]) : p[0];
        st->cy = noise ? __fadd_rn(p[1], noise[1]) : p[1];
        st->cz = noise ? __fadd_rn(p[2], noise[2]) : p[2];
        scene_min[s] = ~0ull;
        scene_out[0] = s;
    }
}

__global__ __launch_bounds__(SC_THREADS) void scenes_d2_hist(const float* __restrict__ xyz, int stride,
                                                              ScenesState* __restrict__ st, uint32_t* __restrict__ keys,
                                                              uint32_t* __restrict__ hist) {
    if ((int)blockIdx.x >= st->groups) return;
    const long i0 = (long)blockIdx.x * st->chunk;
    d2_hist_body(xyz + st->base * stride, i0, min((long)st->M, i0 + (long)st->chunk), stride, st->cx, st->cy, st->cz, keys,
                 hist);
}

__global__ __launch_bounds__(SC_THREADS) void scenes_radix_hist(const uint32_t* __restrict__ keys, int level,
                                                                 uint32_t* __restrict__ hist, ScenesState* __restrict__ st) {
    if ((int)blockIdx.x >= st->groups) return;
    radix_hist_body(keys, st->M, level, st->n_sel, hist, &st->sel, st->chunk);
}

__global__ __launch_bounds__(SC_THREADS) void scenes_count(const uint32_t* __restrict__ keys,
                                                            const uint32_t* __restrict__ hist, ScenesState* __restrict__ st,
                                                            uint32_t* __restrict__ cnt) {
    if ((int)blockIdx.x >= st->groups) return;
    count_body(keys, st->M, hist, &st->sel, cnt, st->groups, st->chunk);
}

// the crop's global rows into idx_out (n) int64 in ascending order, the possibility update, scene s's key refreshed
__global__ __launch_bounds__(SC_THREADS) void scenes_write(const uint32_t* __restrict__ keys,
                                                            const ScenesState* __restrict__ st,
                                                            const uint32_t* __restrict__ cnt, float* __restrict__ poss,
                                                            int64_t* __restrict__ idx_out, int n,
                                                            uint64_t* __restrict__ scene_min) {
    const long base = st->base;
    // the repeats of a padded crop (n_sel = M < n: the select took every point, slot i = row base + i): slot j = row
    // base + j mod M, by every workgroup of the launch; n_sel == n otherwise
    const uint32_t n_sel = st->n_sel;
    if (n_sel > 0u)
        for (long j = (long)n_sel + (long)blockIdx.x * SC_THREADS + threadIdx.x; j < n; j += (long)gridDim.x * SC_THREADS)
            idx_out[j] = base + (long)((uint32_t)j % n_sel);
    if ((int)blockIdx.x >= st->groups) return;
    uint64_t best = write_body<true>(st->M, keys, &st->sel, cnt, st->groups, st->chunk, poss + base, n, base,
                                     [&](long pos, long i) { idx_out[pos] = base + i; });
    best = block_min_u64(best);
    if (threadIdx.x == 0) atomicMin((unsigned long long*)&scene_min[st->s], (unsigned long long)best);
}


// ---- voted crops over many scenes (rl_scenes_vote_*, Model.predict_scenes) ------------------------------------------------------
// The sampler above, competing for coverage instead of for ever: count (T) holds how many crops a point was in, low (S) the
// minimum of every scene's counts, and a scene takes part in the pick while low[s] < votes ("open").  The count rises with
// the possibility, in the crop's write launch, so the next crop of the same pass already sees a covered scene closed (a
// padded scene's farthest point gains no possibility: by possibility alone it would be picked again at once).  A crop that
// finds no open scene is idle: n_sel = groups = 0, and every later launch of that crop exits without writing.  The twin is
// utils/scene.py: scenes_vote_crop.

// scenes_pick among the open scenes; low[s] to INT32_MAX for the write launch to refresh; first_out = the duplicate-free slots
__global__ __launch_bounds__(SC_THREADS) void scenes_vote_pick(const float* __restrict__ cloud, int dim,
                                                                ScenesState* __restrict__ st,
                                                                uint64_t* __restrict__ scene_min,
                                                                const int64_t* __restrict__ off, uint32_t* __restrict__ hist,
                                                                int32_t* __restrict__ low, int votes,
                                                                int64_t* __restrict__ scene_out,
                                                                int32_t* __restrict__ first_out, int n, int pad) {
    __shared__ int picked;
    const int S = st->S;
    uint64_t best = ~0ull;
    for (int j = threadIdx.x; j < S; j += SC_THREADS)
        if (low[j] < votes) best = scene_min[j] < best ? scene_min[j] : best;
    best = block_min_u64(best);
    if (threadIdx.x == 0) picked = -1;
    for (int j = threadIdx.x; j < 3 * SC_BINS; j += SC_THREADS) hist[j] = 0u;
    __syncthreads();
    if (best != ~0ull)
        for (int j = threadIdx.x; j < S; j += SC_THREADS)
            if (low[j] < votes && scene_min[j] == best) picked = j;      // keys of different scenes differ in their row
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int s = picked;
    long base = 0, M = 0, g = 0;
    if (s >= 0) {
        base = off[s];
        M = off[s + 1] - base;
        M = M < 0 ? 0 : (M > st->max_points ? st->max_points : M);         // (keys hold max_points: never past them)
        g = (long)(uint32_t)(best & 0xffffffffull);
    }
    if (s < 0 || M <= 0 || g < base || g >= base + M) {                    // no open scene (or a workspace rl_scenes_init
        st->s = -1;                                                        // never saw): the slot is idle
        st->base = 0;
        st->M = 0;
        st->chunk = SC_THREADS;
        st->groups = 0;
        st->n_sel = 0u;
        scene_out[0] = -1;
        first_out[0] = 0;
        return;
    }
    const Layout L = layout(M);
    const uint32_t n_sel = (uint32_t)(pad && M < n ? M : n);
    st->s = s;
    st->base = base;
    st->M = M;
    st->chunk = L.chunk;
    st->groups = L.groups;
    st->n_sel = n_sel;
    st->sel.centre = (uint32_t)g;
    const float* p = cloud + g * (long)dim;
    st->cx = p[0];
    st->cy = p[1];
    st->cz = p[2];
    scene_min[s] = ~0ull;
    low[s] = 0x7fffffff;
    scene_out[0] = s;
    first_out[0] = (int32_t)n_sel;
}

// scenes_write, and: count += 1 beside the possibility update, low[s] = the scene's least count (integer atomicMin over the
// workgroups, as the scene key), cloud row i gathered into rows + pos*row_stride (the repeats of a padded crop too)
__global__ __launch_bounds__(SC_THREADS) void scenes_vote_write(const float* __restrict__ cloud, int dim,
                                                                 const uint32_t* __restrict__ keys,
                                                                 const ScenesState* __restrict__ st,
                                                                 const uint32_t* __restrict__ cnt, float* __restrict__ poss,
                                                                 int32_t* __restrict__ count, int32_t* __restrict__ low,
                                                                 float* __restrict__ rows, long row_stride,
                                                                 int64_t* __restrict__ idx_out, int n,
                                                                 uint64_t* __restrict__ scene_min) {
    const uint32_t n_sel = st->n_sel;
    if (n_sel == 0u) return;                       // an idle slot: idx_out and rows keep what they hold
    const long base = st->base;
    auto place = [&](long pos, long i) {           // slot pos <- global row base + i
        idx_out[pos] = base + i;
        const float* src = cloud + (base + i) * dim;
        float* dst = rows + pos * row_stride;
        for (int c = 0; c < dim; ++c) dst[c] = src[c];
    };
    for (long j = (long)n_sel + (long)blockIdx.x * SC_THREADS + threadIdx.x; j < n; j += (long)gridDim.x * SC_THREADS)
        place(j, (long)((uint32_t)j % n_sel));
    if ((int)blockIdx.x >= st->groups) return;
    const long M = st->M, chunk = st->chunk;
    int32_t* cs = count + base;
    uint64_t best = write_body<true>(M, keys, &st->sel, cnt, st->groups, chunk, poss + base, n, base, [&](long pos, long i) {
        place(pos, i);
        cs[i] += 1;                                // once per point: a crop's points are distinct
    });
    // the least count of this chunk after the update; thread t reads the points it alone may have raised (i = t mod 256)
    int32_t least = 0x7fffffff;
    const long i0 = (long)blockIdx.x * chunk;
    const long i1 = min(M, i0 + chunk);
    for (long i = i0 + threadIdx.x; i < i1; i += SC_THREADS) least = min(least, cs[i]);
    best = block_min_u64(best);
    // int32 counts are >= 0: the unsigned key order is the signed order
    const uint64_t lo = block_min_u64((uint64_t)(uint32_t)least);
    if (threadIdx.x == 0) {
        atomicMin((unsigned long long*)&scene_min[st->s], (unsigned long long)best);
        atomicMin(&low[st->s], (int32_t)lo);
    }
}

// one workgroup: how many scenes are open
__global__ __launch_bounds__(SC_THREADS) void scenes_vote_open(const ScenesState* __restrict__ st,
                                                                const int32_t* __restrict__ low, int votes,
                                                                int32_t* __restrict__ open_out) {
    const int S = st->S;
    uint32_t open = 0;
    for (int j = threadIdx.x; j < S; j += SC_THREADS) open += low[j] < votes;
    open = block_sum_u32(open);
    if (threadIdx.x == 0) open_out[0] = (int32_t)open;
}

// scene_accumulate<true> on global int64 rows over the first first[0] slots (read on the device: 0 for an idle slot); no count
__global__ __launch_bounds__(SC_THREADS) void scenes_vote_accumulate(const float* __restrict__ logits, int C, int n, long ld,
                                                                      const int64_t* __restrict__ idx,
                                                                      const int32_t* __restrict__ first, float oms, float s,
                                                                      float* __restrict__ prob, long T) {
    const int j = blockIdx.x * SC_THREADS + threadIdx.x;
    if (j >= n || j >= first[0]) return;
    const long i = idx[j];
    if (i < 0 || i >= T) return;
    const float* z = logits + j;
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, z[(long)c * ld]);
    float den = 0.f;
    for (int c = 0; c < C; ++c) den = __fadd_rn(den, exp_fixed(__fsub_rn(z[(long)c * ld], m)));
    float* p = prob + i * C;
    for (int c = 0; c < C; ++c) {
        const float sm = __fdiv_rn(exp_fixed(__fsub_rn(z[(long)c * ld], m)), den);
        p[c] = __fadd_rn(__fmul_rn(s, p[c]), __fmul_rn(oms, sm));
    }
}

}  // namespace

extern "C" int64_t rl_scene_workspace_bytes(int64_t M, int n) {
    (void)n;
    if (M <= 0) return 0;
    return (int64_t)scene_ws(M).bytes;
}

namespace {

// rl_scene_crop (pad = false) and rl_scene_crop_padded: the same six launches; a padded crop of M < n points selects M keys
// and its write launch has workgroups for the n - M repeats as well
int scene_crop_impl(const char* fn, bool pad, const float* cloud, int64_t M, int dim, float* possibility, int n,
                    float* rows_out, int64_t row_stride, int32_t* idx_out, void* ws, int64_t ws_bytes, void* stream) {
    RL_REQUIRE(M > 0 && M < 0x7fffffffLL, RL_ERR_ARGS, "%s: M=%lld outside 1 .. 2^31-2", fn, (long long)M);
    RL_REQUIRE(dim >= 3, RL_ERR_ARGS, "%s: dim=%d, the rows need x, y, z", fn, dim);
    RL_REQUIRE(n > 0 && (pad || n <= M), RL_ERR_ARGS, "%s: crop of n=%d points out of M=%lld", fn, n, (long long)M);
    RL_REQUIRE(row_stride >= dim, RL_ERR_ARGS, "%s: row_stride=%lld < dim=%d", fn, (long long)row_stride, dim);
    RL_REQUIRE(cloud && possibility && rows_out && idx_out, RL_ERR_ARGS, "%s: null pointer", fn);
    int rc = rl_ws_check(fn, ws, ws_bytes, rl_scene_workspace_bytes(M, n));
    if (rc) return rc;
    hipStream_t sm = (hipStream_t)stream;
    const SceneWs W = scene_ws(M);
    SceneState* state = (SceneState*)ws;
    uint64_t* pick = rl_at<uint64_t>(ws, W.off_pick);
    uint32_t* hist = rl_at<uint32_t>(ws, W.off_hist);
    uint32_t* cnt = rl_at<uint32_t>(ws, W.off_cnt);
    uint32_t* keys = rl_at<uint32_t>(ws, W.off_keys);
    const Layout L = layout(M);
    const uint32_t n_sel = (uint32_t)(n < M ? n : M);              // the keys the select takes
    long wg = L.groups;                                            // the write launch: the chunks, and the repeats
    if (n > M) wg = std::max(wg, std::min<long>(((long)n - M + 4 * SC_THREADS - 1) / (4 * SC_THREADS), SC_MAX_GROUPS));
    hipLaunchKernelGGL(scene_pick_partial, dim3(L.pick), dim3(SC_THREADS), 0, sm, possibility, (long)M, pick, hist);
    RL_LAUNCH_CHECK(fn);
    hipLaunchKernelGGL(scene_d2_hist, dim3(L.groups), dim3(SC_THREADS), 0, sm, cloud, (long)M, dim, pick, L.pick, keys,
                       hist, state, L.chunk);
    RL_LAUNCH_CHECK(fn);
    for (int level = 1; level <= 2; ++level) {
        hipLaunchKernelGGL(scene_radix_hist, dim3(L.groups), dim3(SC_THREADS), 0, sm, keys, (long)M, level, n_sel, hist,
                           state, L.chunk);
        RL_LAUNCH_CHECK(fn);
    }
    hipLaunchKernelGGL(scene_count, dim3(L.groups), dim3(SC_THREADS), 0, sm, keys, (long)M, hist, state, cnt, L.groups,
                       L.chunk);
    RL_LAUNCH_CHECK(fn);
    hipLaunchKernelGGL(scene_write, dim3((int)wg), dim3(SC_THREADS), 0, sm, cloud, (long)M, dim, keys, state, cnt,
                       L.groups, L.chunk, possibility, rows_out, (long)row_stride, idx_out, n);
    rl_note_kernel("scene_write");
    RL_LAUNCH_CHECK(fn);
    return RL_OK;
}

// rl_scene_accumulate (ld = n, first = n, the library's expf) and rl_scene_accumulate_first (fixed: exp_fixed)
int scene_accumulate_impl(const char* fn, bool fixed, const float* logits, int C, int n, int64_t ld, int first,
                          const int32_t* idx, float one_minus_s, float s, float* prob, int32_t* count, int64_t M,
                          void* stream) {
    RL_REQUIRE(C > 0 && n > 0 && M > 0 && first > 0 && first <= n && n <= ld && first <= M, RL_ERR_ARGS,
               "%s: bad sizes C=%d n=%d M=%lld ld=%lld first=%d", fn, C, n, (long long)M, (long long)ld, first);
    RL_REQUIRE(logits && idx && prob && count, RL_ERR_ARGS, "%s: null pointer", fn);
    auto kernel = fixed ? scene_accumulate<true> : scene_accumulate<false>;
    hipLaunchKernelGGL(kernel, dim3(rl_cdiv(first, SC_THREADS)), dim3(SC_THREADS), 0, (hipStream_t)stream, logits, C, first,
                       (long)ld, idx, one_minus_s, s, prob, count, (long)M);
    rl_note_kernel("scene_accumulate");
    RL_LAUNCH_CHECK(fn);
    return RL_OK;
}

}  // namespace

extern "C" int rl_scene_crop(const float* cloud, int64_t M, int dim, float* possibility, int n, float* rows_out,
                             int64_t row_stride, int32_t* idx_out, void* ws, int64_t ws_bytes, void* stream) {
    return scene_crop_impl("rl_scene_crop", false, cloud, M, dim, possibility, n, rows_out, row_stride, idx_out, ws,
                           ws_bytes, stream);
}

extern "C" int rl_scene_crop_padded(const float* cloud, int64_t M, int dim, float* possibility, int n, float* rows_out,
                                    int64_t row_stride, int32_t* idx_out, void* ws, int64_t ws_bytes, void* stream) {
    return scene_crop_impl("rl_scene_crop_padded", true, cloud, M, dim, possibility, n, rows_out, row_stride, idx_out, ws,
                           ws_bytes, stream);
}

extern "C" int rl_scene_accumulate(const float* logits, int C, int n, const int32_t* idx, float one_minus_s, float s,
                                   float* prob, int32_t* count, int64_t M, void* stream) {
    RL_REQUIRE(C > 0 && n > 0 && M > 0 && n <= M, RL_ERR_ARGS, "rl_scene_accumulate: bad sizes C=%d n=%d M=%lld", C, n,
               (long long)M);
    return scene_accumulate_impl("rl_scene_accumulate", false, logits, C, n, n, n, idx, one_minus_s, s, prob, count, M, stream);
}

extern "C" int rl_scene_accumulate_first(const float* logits, int C, int n, const int32_t* idx, float one_minus_s, float s,
                                         float* prob, int32_t* count, int64_t M, int64_t ld, int first, void* stream) {
    return scene_accumulate_impl("rl_scene_accumulate_first", true, logits, C, n, ld, first, idx, one_minus_s, s, prob, count, M,
                                 stream);
}

extern "C" int rl_scene_min_count(const int32_t* count, int64_t M, int32_t* out, void* ws, void* stream) {
    RL_REQUIRE(M > 0, RL_ERR_ARGS, "rl_scene_min_count: M=%lld", (long long)M);
    RL_REQUIRE(count && out && ws, RL_ERR_ARGS, "rl_scene_min_count: null pointer");
    hipStream_t sm = (hipStream_t)stream;
    int32_t* part = rl_at<int32_t>(ws, scene_ws(M).off_min);
    long g = (M + 8 * SC_THREADS - 1) / (8 * SC_THREADS);
    if (g > SC_MAX_MIN) g = SC_MAX_MIN;
    hipLaunchKernelGGL(scene_min_partial, dim3((int)g), dim3(SC_THREADS), 0, sm, count, (long)M, part);
    RL_LAUNCH_CHECK("rl_scene_min_count");
    hipLaunchKernelGGL(scene_min_final, dim3(1), dim3(SC_THREADS), 0, sm, part, (int)g, out);
    rl_note_kernel("scene_min_final");
    RL_LAUNCH_CHECK("rl_scene_min_count");
    return RL_OK;
}

extern "C" int64_t rl_scenes_workspace_bytes(int S, int64_t max_points, int n) {
    (void)n;
    if (S <= 0 || max_points <= 0) return 0;
    return (int64_t)scenes_ws(S, max_points).bytes;
}

extern "C" int rl_scenes_init(const int64_t* off, int S, int64_t max_points, const float* possibility, void* ws,
                              int64_t ws_bytes, void* stream) {
    RL_REQUIRE(S > 0, RL_ERR_ARGS, "rl_scenes_init: S=%d scenes", S);
    RL_REQUIRE(max_points > 0 && max_points < 0x7fffffffLL, RL_ERR_ARGS, "rl_scenes_init: max_points=%lld outside 1 .. 2^31-2",
               (long long)max_points);
    RL_REQUIRE(off && possibility, RL_ERR_ARGS, "rl_scenes_init: null pointer");
    int rc = rl_ws_check("rl_scenes_init", ws, ws_bytes, rl_scenes_workspace_bytes(S, max_points, 1));
    if (rc) return rc;
    hipStream_t sm = (hipStream_t)stream;
    const ScenesWs W = scenes_ws(S, max_points);
    ScenesState* st = (ScenesState*)ws;
    uint64_t* scene_min = rl_at<uint64_t>(ws, W.off_scene_min);
    int64_t* off_ws = rl_at<int64_t>(ws, W.off_offsets);
    hipLaunchKernelGGL(scenes_init_state, dim3(rl_cdiv(S + 1, SC_THREADS)), dim3(SC_THREADS), 0, sm, off, S, max_points, st,
                       off_ws, scene_min);
    RL_LAUNCH_CHECK("rl_scenes_init (state)");
    hipLaunchKernelGGL(scenes_init_min, dim3(SS_INIT_PARTS, S), dim3(SC_THREADS), 0, sm, possibility, off_ws, scene_min);
    rl_note_kernel("scenes_init_min");
    RL_LAUNCH_CHECK("rl_scenes_init (min)");
    return RL_OK;
}

namespace {

// What rl_scenes_crop, rl_scenes_crop_padded and rl_scenes_vote_crop share (the callers have checked their own arguments): the
// requirements on the scenes and the workspace, its pieces, and B crops in order - each crop sees what the previous ones
// raised.  A crop is pick(b, W) - one workgroup that picks the scene and the centre and writes how many keys the select takes
// (n, or min(n, M_s) when padded) into the state - the four select launches over the largest scene, and write(b, W, GW).
struct ScenesBufs { ScenesState* st; uint64_t* scene_min; const int64_t* off; uint32_t *hist, *cnt, *keys; };

template <class Pick, class Write>
int scenes_crop_loop(const char* fn, bool pad, const float* xyz, int stride, int S, int64_t max_points, int n, int B, void* ws,
                     int64_t ws_bytes, hipStream_t sm, Pick pick, Write write) {
    RL_REQUIRE(max_points > 0 && max_points < 0x7fffffffLL, RL_ERR_ARGS, "%s: max_points=%lld outside 1 .. 2^31-2", fn,
               (long long)max_points);
    RL_REQUIRE(n > 0 && (pad || n <= max_points), RL_ERR_ARGS, "%s: crop of n=%d points, largest scene %lld", fn, n,
               (long long)max_points);
    int rc = rl_ws_check(fn, ws, ws_bytes, rl_scenes_workspace_bytes(S, max_points, n));
    if (rc) return rc;
    const ScenesWs L = scenes_ws(S, max_points);
    const ScenesBufs W = {(ScenesState*)ws, rl_at<uint64_t>(ws, L.off_scene_min), rl_at<const int64_t>(ws, L.off_offsets),
                          rl_at<uint32_t>(ws, L.off_hist), rl_at<uint32_t>(ws, L.off_cnt), rl_at<uint32_t>(ws, L.off_keys)};
    long G = (max_points + 4 * SC_THREADS - 1) / (4 * SC_THREADS);     // layout()'s group bound for the largest scene
    G = G > SC_MAX_GROUPS ? SC_MAX_GROUPS : G;
    long GW = G;                           // the write launch of a padded crop also covers the repeats of a small scene
    if (pad) GW = std::max(G, std::min<long>(((long)n + 4 * SC_THREADS - 1) / (4 * SC_THREADS), SC_MAX_GROUPS));
    for (int b = 0; b < B; ++b) {
        pick(b, W);
        RL_LAUNCH_CHECK(fn);
        hipLaunchKernelGGL(scenes_d2_hist, dim3((int)G), dim3(SC_THREADS), 0, sm, xyz, stride, W.st, W.keys, W.hist);
        RL_LAUNCH_CHECK(fn);
        for (int level = 1; level <= 2; ++level) {
            hipLaunchKernelGGL(scenes_radix_hist, dim3((int)G), dim3(SC_THREADS), 0, sm, W.keys, level, W.hist, W.st);
            RL_LAUNCH_CHECK(fn);
        }
        hipLaunchKernelGGL(scenes_count, dim3((int)G), dim3(SC_THREADS), 0, sm, W.keys, W.hist, W.st, W.cnt);
        RL_LAUNCH_CHECK(fn);
        write(b, W, (int)GW);
        RL_LAUNCH_CHECK(fn);
    }
    return RL_OK;
}

// rl_scenes_crop (pad = false) and rl_scenes_crop_padded
int scenes_crop_impl(const char* fn, bool pad, const float* xyz, int stride, int S, int64_t max_points, float* possibility,
                     int n, int B, const float* noise, int64_t* idx_out, int64_t* scene_out, void* ws, int64_t ws_bytes,
                     void* stream) {
    RL_REQUIRE(S > 0 && B > 0, RL_ERR_ARGS, "%s: S=%d scenes, B=%d crops", fn, S, B);
    RL_REQUIRE(stride >= 3, RL_ERR_ARGS, "%s: stride=%d, the rows need x, y, z", fn, stride);
    RL_REQUIRE(xyz && possibility && idx_out && scene_out, RL_ERR_ARGS, "%s: null pointer", fn);
    hipStream_t sm = (hipStream_t)stream;
    int rc = scenes_crop_loop(
        fn, pad, xyz, stride, S, max_points, n, B, ws, ws_bytes, sm,
        [&](int b, const ScenesBufs& W) {
            hipLaunchKernelGGL(scenes_pick, dim3(1), dim3(SC_THREADS), 0, sm, xyz, stride, noise ? noise + 3 * b : nullptr, W.st,
                               W.scene_min, W.off, W.hist, scene_out + b, n, pad ? 1 : 0);
        },
        [&](int b, const ScenesBufs& W, int GW) {
            hipLaunchKernelGGL(scenes_write, dim3(GW), dim3(SC_THREADS), 0, sm, W.keys, W.st, W.cnt, possibility,
                               idx_out + (long)b * n, n, W.scene_min);
        });
    if (rc) return rc;
    rl_note_kernel("scenes_write");
    return RL_OK;
}

}  // namespace

extern "C" int rl_scenes_crop(const float* xyz, int stride, int S, int64_t max_points, float* possibility, int n, int B,
                              const float* noise, int64_t* idx_out, int64_t* scene_out, void* ws, int64_t ws_bytes,
                              void* stream) {
    return scenes_crop_impl("rl_scenes_crop", false, xyz, stride, S, max_points, possibility, n, B, noise, idx_out,
                            scene_out, ws, ws_bytes, stream);
}

extern "C" int rl_scenes_crop_padded(const float* xyz, int stride, int S, int64_t max_points, float* possibility, int n,
                                     int B, const float* noise, int64_t* idx_out, int64_t* scene_out, void* ws,
                                     int64_t ws_bytes, void* stream) {
    return scenes_crop_impl("rl_scenes_crop_padded", true, xyz, stride, S, max_points, possibility, n, B, noise, idx_out,
                            scene_out, ws, ws_bytes, stream);
}

extern "C" int rl_scenes_vote_crop(const float* cloud, int dim, int S, int64_t max_points, float* possibility, int32_t* count,
                                   int32_t* low, int votes, int n, int B, int pad, float* rows_out, int64_t slot_stride,
                                   int64_t row_stride, int64_t* idx_out, int64_t* scene_out, int32_t* first_out,
                                   int32_t* open_out, void* ws, int64_t ws_bytes, void* stream) {
    const char* fn = "rl_scenes_vote_crop";
    RL_REQUIRE(S > 0 && B > 0 && votes > 0, RL_ERR_ARGS, "%s: S=%d scenes, B=%d crops, votes=%d", fn, S, B, votes);
    RL_REQUIRE(dim >= 3, RL_ERR_ARGS, "%s: dim=%d, the rows need x, y, z", fn, dim);
    RL_REQUIRE(row_stride >= dim, RL_ERR_ARGS, "%s: row_stride=%lld < dim=%d", fn, (long long)row_stride, dim);
    RL_REQUIRE(B == 1 || slot_stride >= (int64_t)n * row_stride, RL_ERR_ARGS, "%s: slot_stride=%lld < n*row_stride=%lld", fn,
               (long long)slot_stride, (long long)((int64_t)n * row_stride));
    RL_REQUIRE(cloud && possibility && count && low && rows_out && idx_out && scene_out && first_out && open_out, RL_ERR_ARGS,
               "%s: null pointer", fn);
    hipStream_t sm = (hipStream_t)stream;
    int rc = scenes_crop_loop(
        fn, pad != 0, cloud, dim, S, max_points, n, B, ws, ws_bytes, sm,
        [&](int b, const ScenesBufs& W) {
            hipLaunchKernelGGL(scenes_vote_pick, dim3(1), dim3(SC_THREADS), 0, sm, cloud, dim, W.st, W.scene_min, W.off, W.hist,
                               low, votes, scene_out + b, first_out + b, n, pad ? 1 : 0);
        },
        [&](int b, const ScenesBufs& W, int GW) {
            hipLaunchKernelGGL(scenes_vote_write, dim3(GW), dim3(SC_THREADS), 0, sm, cloud, dim, W.keys, W.st, W.cnt,
                               possibility, count, low, rows_out + (long)b * slot_stride, (long)row_stride,
                               idx_out + (long)b * n, n, W.scene_min);
        });
    if (rc) return rc;
    hipLaunchKernelGGL(scenes_vote_open, dim3(1), dim3(SC_THREADS), 0, sm, (const ScenesState*)ws, low, votes, open_out);
    rl_note_kernel("scenes_vote_open");
    RL_LAUNCH_CHECK(fn);
    return RL_OK;
}

extern "C" int rl_scenes_vote_accumulate(const float* logits, int C, int n, int64_t ld, int64_t slot_stride, int B,
                                         const int64_t* idx, const int32_t* first, float one_minus_s, float s, float* prob,
                                         int64_t T, void* stream) {
    const char* fn = "rl_scenes_vote_accumulate";
    RL_REQUIRE(C > 0 && n > 0 && B > 0 && T > 0 && n <= ld, RL_ERR_ARGS, "%s: bad sizes C=%d n=%d B=%d T=%lld ld=%lld", fn, C,
               n, B, (long long)T, (long long)ld);
    RL_REQUIRE(B == 1 || slot_stride >= (int64_t)(C - 1) * ld + n, RL_ERR_ARGS, "%s: slot_stride=%lld, the slots overlap", fn,
               (long long)slot_stride);
    RL_REQUIRE(logits && idx && first && prob, RL_ERR_ARGS, "%s: null pointer", fn);
    for (int b = 0; b < B; ++b) {          // in order: the crops of a pass overlap
        hipLaunchKernelGGL(scenes_vote_accumulate, dim3(rl_cdiv(n, SC_THREADS)), dim3(SC_THREADS), 0, (hipStream_t)stream,
                           logits + (long)b * slot_stride, C, n, (long)ld, idx + (long)b * n, first + b, one_minus_s, s, prob,
                           (long)T);
        RL_LAUNCH_CHECK(fn);
    }
    rl_note_kernel("scenes_vote_accumulate");
    return RL_OK;
}
