// Keypoints of labelled, scored points (Model.predict_keypoints, utils/keypoints.py: confidence_peaks): the local maxima of
// the score over a radius among the points of one label, each refined to the score-weighted mean of the neighbourhood it rules
// over.  The numpy twin is randlanet/utils/keypoints.py; every decision is a fixed fp32 expression of the input and every sum
// runs in a fixed order, so the result equals the twin's bit for bit whatever the scheduling.
//
//   part(i)     label >= 0, not ignored, score >= min_score          near(i, j)  same label, d2 <= r2 (the clustering's edge)
//   support(i)  the j with part(j) and near(i, j), i included        live(i)     part(i) and support(i) >= min_points
//   beats(j, i) score_j > score_i, or equal scores and j < i         peak(i)     live(i), no live j != i near it that beats it
//
//   rl_keypoints_cells    box_partial, box_final (rl_cells.h) over ALL points with the clustering's cell edge c = r * 1.0625f:
//                         origin and dims into the workspace, dims to the caller (who refuses 2^16 cells or more on an axis)
//   rl_keypoints_sort     keys     the cell key of a point that takes part, the sentinel dims_x*dims_y*dims_z for every other
//                         sort     the stable radix sort of (key, point index) (rl_radix.h)
//                         pack     (x, y, z, score) of every sorted position as one float4, the low 32 bits of its label beside it
//   rl_keypoints_support  one lane per sorted position: ALL 27 cells around its own as 9 rows of up to 3 contiguous cells, each
//                         row found by a binary search over the sorted keys - the rows after the own one too, which the
//                         clustering never scans, because support and suppression are not symmetric work that one of the two
//                         points can do for both; the lane counts the near() points: support[j]
//   rl_keypoints_peaks    peak     the same walk over the live candidates only, left at the first one that beats the point;
//                                  peakpos[i] = sorted position + 1 of a peak, 0 of every other point
//                         count, total, write   the peaks compacted in ascending point index by a scan over chunks of peakpos
//                                  (a wavefront per chunk counts, one workgroup scans the counts, a wavefront per chunk writes):
//                                  the sorted arrays stay as they are for the refinement; K to the caller
//   rl_keypoints_refine   one WAVEFRONT per keypoint: the same 9 rows, 64 candidates loaded at a time in sorted-position order;
//                         the members - live and near the peak - are then added one by one in that order in fp64 (lane 0 owns
//                         the chain of W = sum score, lanes 1 .. 3 those of S_a = sum score * (x_a - peak_a), every product
//                         rounded before it is added); position = peak + S / W rounded once to fp32
//
// Candidates whose labels agree in their low 32 bits are told apart by the full label of the point, read only for a candidate
// that passed every other test.  Plain loads and vector stores; no atomics at all; no workgroup waits for another one.
#include "rl_cells.h"

namespace {

constexpr int KP_MAX_DIM_BITS = 16;      // the caller refuses a grid of 2^16 cells or more on an axis

// the front is the clustering's (GridState, boxes, sort, cnt, start); start holds the sorted positions of the K peaks
struct KeypointLayout {
    CellsLayout cells;
    size_t off_pts, off_lab, off_support, off_peakpos, bytes;
};

KeypointLayout keypoint_layout(long M) {
    KeypointLayout L;
    RlCarve c;
    L.cells = cells_layout(c, M);
    L.off_pts = c.take((size_t)M * sizeof(float4));
    L.off_lab = c.take((size_t)M * sizeof(uint32_t));
    L.off_support = c.take((size_t)M * sizeof(int32_t));
    L.off_peakpos = c.take((size_t)M * sizeof(uint32_t));
    L.bytes = c.at;
    return L;
}

__global__ __launch_bounds__(GR_THREADS) void kp_keys(const float* __restrict__ xyz, const int64_t* __restrict__ labels,
                                                       const float* __restrict__ scores, long M, float min_score,
                                                       const int64_t* __restrict__ ignore, int n_ignore,
                                                       const GridState* __restrict__ st, uint64_t* __restrict__ keys) {
    const long i = (long)blockIdx.x * GR_THREADS + threadIdx.x;
    if (i >= M) return;
    const int64_t label = labels[i];
    bool part = label >= 0 && scores[i] >= min_score;
    for (int k = 0; k < n_ignore; ++k)
        if (ignore[k] == label) part = false;
    keys[i] = part ? grid_cell_key(xyz + i * 3, st) : (uint64_t)(st->dims[0] * st->dims[1] * st->dims[2]);
}

__global__ __launch_bounds__(GR_THREADS) void kp_pack(const float* __restrict__ xyz, const int64_t* __restrict__ labels,
                                                       const float* __restrict__ scores, const uint32_t* __restrict__ idx,
                                                       long M, float4* __restrict__ pts, uint32_t* __restrict__ lab) {
    const long j = (long)blockIdx.x * GR_THREADS + threadIdx.x;
    if (j >= M) return;
    const long i = idx[j];
    if (i >= M) return;                       // (never: idx is a permutation)
    const float* p = xyz + i * 3;
    pts[j] = make_float4(p[0], p[1], p[2], scores[i]);
    lab[j] = (uint32_t)(uint64_t)labels[i];
}

// the clustering's edge rule, un-fused fp32
__device__ __forceinline__ bool kp_within(const float4 a, const float4 b, float r2) {
    const float dx = __fsub_rn(a.x, b.x), dy = __fsub_rn(a.y, b.y), dz = __fsub_rn(a.z, b.z);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)) <= r2;
}

__global__ __launch_bounds__(GR_THREADS) void kp_support(const int64_t* __restrict__ labels, long M,
                                                          const GridState* __restrict__ st, const uint64_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ idx, const float4* __restrict__ pts,
                                                          const uint32_t* __restrict__ lab, float r2,
                                                          int32_t* __restrict__ support) {
    const long j = (long)blockIdx.x * GR_THREADS + threadIdx.x;
    if (j >= M) return;
    const uint64_t key = keys[j];
    int32_t n = 0;
    if (key < (uint64_t)(st->dims[0] * st->dims[1] * st->dims[2]) && idx[j] < M) {
        const float4 me = pts[j];
        const uint32_t mylab32 = lab[j];
        const int64_t mylab = labels[idx[j]];
        grid_rows(key, st, [&](uint64_t klo, uint64_t khi) {
            for (long jj = grid_lower_bound(keys, M, klo); jj < M && keys[jj] <= khi; ++jj)
                if (lab[jj] == mylab32 && kp_within(me, pts[jj], r2) && labels[idx[jj]] == mylab) ++n;
            return true;
        });
    }
    support[j] = n;                           // 0 for a point that takes no part: never live
}

__global__ __launch_bounds__(GR_THREADS) void kp_peak(const int64_t* __restrict__ labels, long M,
                                                       const GridState* __restrict__ st, const uint64_t* __restrict__ keys,
                                                       const uint32_t* __restrict__ idx, const float4* __restrict__ pts,
                                                       const uint32_t* __restrict__ lab, const int32_t* __restrict__ support,
                                                       float r2, int min_pts, uint32_t* __restrict__ peakpos) {
    const long j = (long)blockIdx.x * GR_THREADS + threadIdx.x;
    if (j >= M) return;
    const uint32_t i = idx[j];
    if (i >= M) return;                       // (never)
    bool peak = support[j] >= min_pts;        // live (support is 0 where the key is the sentinel)
    if (peak) {
        const float4 me = pts[j];
        const uint32_t mylab32 = lab[j];
        const int64_t mylab = labels[i];
        grid_rows(keys[j], st, [&](uint64_t klo, uint64_t khi) {
            for (long jj = grid_lower_bound(keys, M, klo); jj < M && keys[jj] <= khi; ++jj) {
                if (support[jj] < min_pts || lab[jj] != mylab32) continue;
                const float4 q = pts[jj];
                if (!(q.w > me.w || (q.w == me.w && idx[jj] < i))) continue;         // (jj == j beats nobody)
                if (kp_within(me, q, r2) && labels[idx[jj]] == mylab) {
                    peak = false;
                    return false;
                }
            }
            return true;
        });
    }
    peakpos[i] = peak ? (uint32_t)j + 1u : 0u;           // every point is some position's: all of peakpos is written
}

// one wavefront per chunk of points: the peaks among them
__global__ __launch_bounds__(64) void kp_count(const uint32_t* __restrict__ peakpos, long M, long chunk,
                                                uint32_t* __restrict__ cnt) {
    const int lane = threadIdx.x;
    const long i0 = (long)blockIdx.x * chunk;
    const long i1 = min(M, i0 + chunk);
    uint32_t n = 0;
    for (long t0 = i0; t0 < i1; t0 += 64) {
        const long i = t0 + lane;
        n += (uint32_t)__popcll(__ballot(i < i1 && peakpos[i] != 0u));
    }
    if (lane == 0) cnt[blockIdx.x] = n;
}

__global__ __launch_bounds__(GR_THREADS) void kp_total(uint32_t* __restrict__ cnt, int chunks, GridState* __restrict__ st,
                                                        int64_t* __restrict__ K_out) {
    const uint32_t K = block_exclusive_scan(cnt, chunks);
    if (threadIdx.x == 0) {
        st->pad[1] = (int64_t)K;
        K_out[0] = (int64_t)K;
    }
}

// one wavefront per chunk: list[k] = the sorted position of the k-th peak in ascending point index (list holds M + 1 entries)
__global__ __launch_bounds__(64) void kp_write(const uint32_t* __restrict__ peakpos, long M, long chunk,
                                                const uint32_t* __restrict__ cnt, uint32_t* __restrict__ list) {
    const int lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    const long i0 = (long)blockIdx.x * chunk;
    const long i1 = min(M, i0 + chunk);
    uint32_t run = cnt[blockIdx.x];           // peaks before this chunk
    for (long t0 = i0; t0 < i1; t0 += 64) {
        const long i = t0 + lane;
        const uint32_t p = i < i1 ? peakpos[i] : 0u;
        const unsigned long long b = __ballot(p != 0u);
        const long k = (long)run + __popcll(b & below);
        if (p != 0u && k < M) list[k] = p - 1u;
        run += (uint32_t)__popcll(b);
    }
}

// one wavefront per keypoint
__global__ __launch_bounds__(GR_THREADS) void kp_refine(const int64_t* __restrict__ labels, long M, long K,
                                                         const GridState* __restrict__ st, const uint64_t* __restrict__ keys,
                                                         const uint32_t* __restrict__ idx, const float4* __restrict__ pts,
                                                         const uint32_t* __restrict__ lab, const int32_t* __restrict__ support,
                                                         const uint32_t* __restrict__ list, float r2, int min_pts,
                                                         int64_t* __restrict__ index_out, int64_t* __restrict__ classes_out,
                                                         float* __restrict__ position_out, float* __restrict__ score_out,
                                                         float* __restrict__ mean_out, int32_t* __restrict__ count_out) {
    const int lane = threadIdx.x & 63;
    const long k = (long)blockIdx.x * GR_WAVES + (threadIdx.x >> 6);
    if (k >= K || k >= st->pad[1]) return;                   // wavefront-uniform
    const long p = list[k];
    if (p >= M || idx[p] >= M) return;                       // (never)
    const long i = idx[p];
    const float4 me = pts[p];
    const uint32_t mylab32 = lab[p];
    const int64_t mylab = labels[i];
    const float mine = lane == 1 ? me.x : lane == 2 ? me.y : me.z;
    double acc = 0.0;                                        // lane 0: W, lanes 1 .. 3: S_x, S_y, S_z
    long count = 0;
    grid_rows(keys[p], st, [&](uint64_t klo, uint64_t khi) {
        const long j0 = grid_lower_bound(keys, M, klo), j1 = grid_lower_bound(keys, M, khi + 1);     // wavefront-uniform
        for (long base = j0; base < j1; base += 64) {
            const long j = base + lane;
            const bool in = j < j1;
            const float4 q = pts[in ? j : p];
            bool member = in && support[j] >= min_pts && lab[j] == mylab32 && kp_within(me, q, r2);
            if (member) member = labels[idx[j]] == mylab;
            unsigned long long todo = __ballot(member);
            count += __popcll(todo);
            while (todo) {                                   // member after member: the fixed order of the contract
                const int t = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
                todo &= todo - 1ull;
                const float s = grid_lane(q.w, t), x = grid_lane(q.x, t), y = grid_lane(q.y, t), z = grid_lane(q.z, t);
                const double d = __dsub_rn((double)(lane == 1 ? x : lane == 2 ? y : z), (double)mine);
                acc = __dadd_rn(acc, lane == 0 ? (double)s : __dmul_rn((double)s, d));
            }
        }
        return true;
    });
    const double W = __shfl(acc, 0, 64);
    if (lane >= 1 && lane <= 3) position_out[k * 3 + lane - 1] = W == 0.0 ? mine : (float)__dadd_rn((double)mine, acc / W);
    if (lane == 0) {
        index_out[k] = i;
        classes_out[k] = mylab;
        score_out[k] = me.w;
        mean_out[k] = (float)(W / (double)count);
        count_out[k] = (int32_t)count;
    }
}

int keypoints_check(const char* who, int64_t M, const void* ws, int64_t ws_bytes) {
    RL_REQUIRE(M > 0 && M < 0x7fffffffLL, RL_ERR_ARGS, "%s: M=%lld outside 1 .. 2^31-2", who, (long long)M);
    return rl_ws_check(who, ws, ws_bytes, rl_keypoints_workspace_bytes(M));
}

int keypoints_radius(const char* who, float radius) {
    RL_REQUIRE(radius > 0.f && isfinite(radius) && isfinite(radius * radius) && isfinite(radius * 1.0625f), RL_ERR_ARGS,
               "%s: radius=%g must be positive and finite", who, (double)radius);
    return RL_OK;
}

struct KeypointBufs {
    GridState* st;
    RadixBufs sort;
    float4* pts;
    uint32_t *lab, *peakpos, *cnt, *list;
    int32_t* support;
};

KeypointBufs keypoint_bufs(void* ws, long M) {
    const KeypointLayout L = keypoint_layout(M);
    return {(GridState*)ws, radix_bufs(ws, L.cells.sort), rl_at<float4>(ws, L.off_pts), rl_at<uint32_t>(ws, L.off_lab),
            rl_at<uint32_t>(ws, L.off_peakpos), rl_at<uint32_t>(ws, L.cells.off_cnt), rl_at<uint32_t>(ws, L.cells.off_start),
            rl_at<int32_t>(ws, L.off_support)};
}

}  // namespace

extern "C" int64_t rl_keypoints_workspace_bytes(int64_t M) {
    if (M <= 0 || M >= 0x7fffffffLL) return 0;
    return (int64_t)keypoint_layout(M).bytes;
}

extern "C" int rl_keypoints_cells(const float* xyz, int64_t M, float radius, int64_t* dims_out, void* ws, int64_t ws_bytes,
                                  void* stream) {
    int rc = keypoints_radius("rl_keypoints_cells", radius);
    if (rc) return rc;
    rc = keypoints_check("rl_keypoints_cells", M, ws, ws_bytes);
    if (rc) return rc;
    RL_REQUIRE(xyz && dims_out, RL_ERR_ARGS, "rl_keypoints_cells: null pointer");
    hipStream_t sm = (hipStream_t)stream;
    float* box = rl_at<float>(ws, keypoint_layout(M).cells.off_box);
    const long parts = grid_box_parts(M);
    hipLaunchKernelGGL(grid_box_partial, dim3((int)parts), dim3(GR_THREADS), 0, sm, xyz, (long)M, 3, box);
    RL_LAUNCH_CHECK("rl_keypoints_cells (partial)");
    hipLaunchKernelGGL(grid_box_final, dim3(1), dim3(GR_THREADS), 0, sm, box, (int)parts, radius * 1.0625f, (long)M,
                       (GridState*)ws, dims_out);
    rl_note_kernel("grid_box_final");
    RL_LAUNCH_CHECK("rl_keypoints_cells (final)");
    return RL_OK;
}

extern "C" int rl_keypoints_sort(const float* xyz, const int64_t* labels, const float* scores, int64_t M, float min_score,
                                 const int64_t* ignore, int n_ignore, int key_bits, void* ws, int64_t ws_bytes, void* stream) {
    RL_REQUIRE(!(min_score != min_score), RL_ERR_ARGS, "rl_keypoints_sort: min_score is not a number");
    RL_REQUIRE(key_bits >= 1 && key_bits <= 3 * KP_MAX_DIM_BITS + 1, RL_ERR_ARGS, "rl_keypoints_sort: key_bits=%d outside 1 .. %d",
               key_bits, 3 * KP_MAX_DIM_BITS + 1);
    RL_REQUIRE(n_ignore >= 0 && (n_ignore == 0 || ignore), RL_ERR_ARGS, "rl_keypoints_sort: %d ignored classes without a list",
               n_ignore);
    int rc = keypoints_check("rl_keypoints_sort", M, ws, ws_bytes);
    if (rc) return rc;
    RL_REQUIRE(xyz && labels && scores, RL_ERR_ARGS, "rl_keypoints_sort: null pointer");
    hipStream_t sm = (hipStream_t)stream;
    const KeypointBufs b = keypoint_bufs(ws, (long)M);
    const dim3 grid(rl_cdiv(M, GR_THREADS)), block(GR_THREADS);
    const int passes = grid_passes(key_bits);
    hipLaunchKernelGGL(kp_keys, grid, block, 0, sm, xyz, labels, scores, (long)M, min_score, ignore, n_ignore, b.st,
                       b.sort.keys[passes & 1]);
    RL_LAUNCH_CHECK("rl_keypoints_sort (keys)");
    rc = radix_sort("rl_keypoints_sort", b.sort, (long)M, passes, sm);
    if (rc) return rc;
    hipLaunchKernelGGL(kp_pack, grid, block, 0, sm, xyz, labels, scores, b.sort.idx[0], (long)M, b.pts, b.lab);
    rl_note_kernel("kp_pack");
    RL_LAUNCH_CHECK("rl_keypoints_sort (pack)");
    return RL_OK;
}

extern "C" int rl_keypoints_support(const int64_t* labels, int64_t M, float radius, void* ws, int64_t ws_bytes, void* stream) {
    int rc = keypoints_radius("rl_keypoints_support", radius);
    if (rc) return rc;
    rc = keypoints_check("rl_keypoints_support", M, ws, ws_bytes);
    if (rc) return rc;
    RL_REQUIRE(labels, RL_ERR_ARGS, "rl_keypoints_support: null pointer");
    const KeypointBufs b = keypoint_bufs(ws, (long)M);
    hipLaunchKernelGGL(kp_support, dim3(rl_cdiv(M, GR_THREADS)), dim3(GR_THREADS), 0, (hipStream_t)stream, labels, (long)M, b.st,
                       b.sort.keys[0], b.sort.idx[0], b.pts, b.lab, radius * radius, b.support);
    rl_note_kernel("kp_support");
    RL_LAUNCH_CHECK("rl_keypoints_support");
    return RL_OK;
}

extern "C" int rl_keypoints_peaks(const int64_t* labels, int64_t M, float radius, int64_t min_points, int64_t* K_out, void* ws,
                                  int64_t ws_bytes, void* stream) {
    int rc = keypoints_radius("rl_keypoints_peaks", radius);
    if (rc) return rc;
    RL_REQUIRE(min_points >= 1, RL_ERR_ARGS, "rl_keypoints_peaks: min_points=%lld", (long long)min_points);
    rc = keypoints_check("rl_keypoints_peaks", M, ws, ws_bytes);
    if (rc) return rc;
    RL_REQUIRE(labels && K_out, RL_ERR_ARGS, "rl_keypoints_peaks: null pointer");
    hipStream_t sm = (hipStream_t)stream;
    const KeypointBufs b = keypoint_bufs(ws, (long)M);
    const int min_pts = (int)(min_points > M ? M + 1 : min_points);
    hipLaunchKernelGGL(kp_peak, dim3(rl_cdiv(M, GR_THREADS)), dim3(GR_THREADS), 0, sm, labels, (long)M, b.st, b.sort.keys[0],
                       b.sort.idx[0], b.pts, b.lab, b.support, radius * radius, min_pts, b.peakpos);
    RL_LAUNCH_CHECK("rl_keypoints_peaks (peak)");
    hipLaunchKernelGGL(kp_count, dim3(b.sort.chunks), dim3(64), 0, sm, b.peakpos, (long)M, b.sort.chunk, b.cnt);
    RL_LAUNCH_CHECK("rl_keypoints_peaks (count)");
    hipLaunchKernelGGL(kp_total, dim3(1), dim3(GR_THREADS), 0, sm, b.cnt, b.sort.chunks, b.st, K_out);
    RL_LAUNCH_CHECK("rl_keypoints_peaks (total)");
    hipLaunchKernelGGL(kp_write, dim3(b.sort.chunks), dim3(64), 0, sm, b.peakpos, (long)M, b.sort.chunk, b.cnt, b.list);
    rl_note_kernel("kp_write");
    RL_LAUNCH_CHECK("rl_keypoints_peaks (write)");
    return RL_OK;
}

extern "C" int rl_keypoints_refine(const int64_t* labels, int64_t M, int64_t K, float radius, int64_t min_points,
                                   int64_t* index_out, int64_t* classes_out, float* position_out, float* score_out,
                                   float* mean_score_out, int32_t* count_out, void* ws, int64_t ws_bytes, void* stream) {
    int rc = keypoints_radius("rl_keypoints_refine", radius);
    if (rc) return rc;
    RL_REQUIRE(min_points >= 1, RL_ERR_ARGS, "rl_keypoints_refine: min_points=%lld", (long long)min_points);
    rc = keypoints_check("rl_keypoints_refine", M, ws, ws_bytes);
    if (rc) return rc;
    RL_REQUIRE(K > 0 && K <= M, RL_ERR_ARGS, "rl_keypoints_refine: K=%lld keypoints of M=%lld points", (long long)K, (long long)M);
    RL_REQUIRE(labels && index_out && classes_out && position_out && score_out && mean_score_out && count_out, RL_ERR_ARGS,
               "rl_keypoints_refine: null pointer");
    const KeypointBufs b = keypoint_bufs(ws, (long)M);
    const int min_pts = (int)(min_points > M ? M + 1 : min_points);
    hipLaunchKernelGGL(kp_refine, dim3(rl_cdiv(K, GR_WAVES)), dim3(GR_THREADS), 0, (hipStream_t)stream, labels, (long)M, (long)K,
                       b.st, b.sort.keys[0], b.sort.idx[0], b.pts, b.lab, b.support, b.list, radius * radius, min_pts, index_out,
                       classes_out, position_out, score_out, mean_score_out, count_out);
    rl_note_kernel("kp_refine");
    RL_LAUNCH_CHECK("rl_keypoints_refine");
    return RL_OK;
}
