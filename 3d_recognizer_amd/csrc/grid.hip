// Grid subsampling of a raw scene (the front of RandLA-Net's large-scene protocol: the authors' grid_subsampling) and the
// confusion matrix of a voted scene (its back): one representative per occupied voxel - barycentre, mean features, majority
// label - and the scoring of every raw point through the representative of its own cell.  The numpy twin of every step is
// randlanet/utils/grid.py; everything here is integer work or a fixed fp32 / fp64 expression, so the result equals the twin's
// bit for bit and is a pure function of the input (no floating-point atomics, no arrival order anywhere).
//
//   rl_grid_bounds   box_partial   per-workgroup min / max of x, y, z
//                    box_final     one workgroup folds them; origin o = floor(min / c) * c and dims = floor((max - o) / c) + 1
//                                  (each operation rounded to fp32) into the workspace, dims also to the caller
//   rl_grid_sort     keys          v = floor((p - o) / c) per axis (correctly rounded division), key = (vz*dy + vy)*dx + vx
//                    per 8-bit digit of the key, lowest first (LSD radix sort of (key, point index), only the digits dims need;
//                    the pass kernels and their host loop live in rl_radix.h, which every sorting feature shares; the box, the
//                    key and the heads live in rl_cells.h, which cluster.hip shares):
//                      hist        per chunk of consecutive positions a 256-bin histogram (LDS), stored bin-major
//                      scan        per bin the exclusive prefix over the chunks, and the bin's total
//                      scatter     one wavefront per chunk: bin bases from the totals, then 64 positions at a time in position
//                                  order, equal digits ranked by lane through ballots -> STABLE: a cell's points stay in
//                                  ascending point index
//   rl_grid_heads    head_count    per chunk the number of positions whose key differs from the one before
//                    head_scan     one workgroup: exclusive prefix of those counts, V = their sum (int64, to the caller too)
//                    head_write    segment of every sorted position (ballots in position order): inverse[perm[j]] = segment,
//                                  start[segment] = j at its first position
//   rl_grid_reduce   reduce        one lane per cell: its points in sorted (= ascending index) order summed in fp64 column by
//                                  column, mean = sum / count in fp64 rounded once to fp32; labels by integer counts per
//                                  class, the most frequent one, ties to the lowest class; a label outside [0, n_classes)
//                                  falls through the counting, and a cell without a vote gets -1 (unlabelled)
//   rl_scene_confusion             argmax of prob row inverse[i] (or i), ties to the lowest class, (label, argmax) counted in an
//                                  LDS table per workgroup and added to the (C, C) int64 table by integer atomics
// No workgroup waits for another one: every scan over the whole array is split over launches.
#include "rl_cells.h"

namespace {

constexpr int GR_COLS = 8;               // columns a lane of the reduction sums together
constexpr int GR_CONF_LDS_C = 64;        // classes up to which the confusion table of a workgroup lives in LDS

CellsLayout grid_layout(long M) {
    RlCarve c;
    return cells_layout(c, M);
}

__global__ __launch_bounds__(GR_THREADS) void grid_keys(const float* __restrict__ cloud, long M, int dim,
                                                         const GridState* __restrict__ st, uint64_t* __restrict__ keys) {
    const long i = (long)blockIdx.x * GR_THREADS + threadIdx.x;
    if (i >= M) return;
    keys[i] = grid_cell_key(cloud + i * dim, st);
}

// one lane per cell; the segment in sorted order = ascending point index
__global__ __launch_bounds__(GR_THREADS) void grid_reduce(const float* __restrict__ cloud, long M, int dim,
                                                           const uint32_t* __restrict__ idx,
                                                           const uint32_t* __restrict__ start,
                                                           const GridState* __restrict__ st,
                                                           const int64_t* __restrict__ labels, int n_classes, long V,
                                                           float* __restrict__ rows_out, int64_t* __restrict__ labels_out,
                                                           int32_t* __restrict__ count_out) {
    const long v = (long)blockIdx.x * GR_THREADS + threadIdx.x;
    if (v >= V || v >= st->V) return;
    long j0 = start[v], j1 = start[v + 1];
    j1 = j1 > M ? M : j1;
    j0 = j0 > j1 ? j1 : j0;
    const double n = (double)(j1 - j0);
    count_out[v] = (int32_t)(j1 - j0);
    for (int c0 = 0; c0 < dim; c0 += GR_COLS) {
        double s[GR_COLS];
#pragma unroll
        for (int k = 0; k < GR_COLS; ++k) s[k] = 0.0;
        for (long j = j0; j < j1; ++j) {
            const float* p = cloud + (long)idx[j] * dim + c0;
#pragma unroll
            for (int k = 0; k < GR_COLS; ++k)
                if (c0 + k < dim) s[k] += (double)p[k];
        }
#pragma unroll
        for (int k = 0; k < GR_COLS; ++k)
            if (c0 + k < dim) rows_out[v * dim + c0 + k] = (float)(s[k] / n);
    }
    if (labels) {
        int best = 0;
        long best_n = -1;
        if (j1 - j0 >= n_classes) {                     // a crowded cell: one count per class
            for (int c = 0; c < n_classes; ++c) {
                long m = 0;
                for (long j = j0; j < j1; ++j) m += labels[idx[j]] == c;
                if (m > best_n) best_n = m, best = c;   // strictly more: ties stay with the lowest class
            }
        } else {
            // one count per LABEL the cell holds (a cell of n points costs at most n * n whatever n_classes is): a label that is
            // the best so far was counted already; among equal counts the lowest class wins, as above
            for (long j = j0; j < j1; ++j) {
                const int64_t l = labels[idx[j]];
                if (l < 0 || l >= n_classes || (best_n > 0 && l == best)) continue;
                long m = 0;
                for (long k = j0; k < j1; ++k) m += labels[idx[k]] == l;
                if (m > best_n || (m == best_n && l < best)) best_n = m, best = (int)l;
            }
        }
        labels_out[v] = best_n > 0 ? best : -1;         // no vote (every label of the cell outside [0, n_classes)): unlabelled
    }
}

template <bool kLds>
__global__ __launch_bounds__(GR_THREADS) void scene_confusion(const float* __restrict__ prob, long V, int C,
                                                               const int64_t* __restrict__ labels, long M,
                                                               const int32_t* __restrict__ inverse,
                                                               unsigned long long* __restrict__ table) {
    __shared__ uint32_t h[kLds ? GR_CONF_LDS_C * GR_CONF_LDS_C : 1];
    if (kLds) {
        for (int j = threadIdx.x; j < C * C; j += GR_THREADS) h[j] = 0u;
        __syncthreads();
    }
    for (long i = (long)blockIdx.x * GR_THREADS + threadIdx.x; i < M; i += (long)gridDim.x * GR_THREADS) {
        const int64_t l = labels[i];
        if (l < 0 || l >= C) continue;                  // unlabelled
        const long r = inverse ? (long)inverse[i] : i;
        if (r < 0 || r >= V) continue;
        const float* p = prob + r * C;
        int best = 0;
        float pb = p[0];
        for (int c = 1; c < C; ++c)
            if (p[c] > pb) pb = p[c], best = c;         // strictly greater: ties stay with the lowest class
        if (kLds) atomicAdd(&h[(int)l * C + best], 1u);
        else atomicAdd(&table[l * C + best], 1ull);
    }
    if (kLds) {
        __syncthreads();
        for (int j = threadIdx.x; j < C * C; j += GR_THREADS)
            if (h[j]) atomicAdd(&table[j], (unsigned long long)h[j]);
    }
}

int grid_check(const char* who, int64_t M, int dim, const void* ws, int64_t ws_bytes) {
    RL_REQUIRE(M > 0 && M < 0x7fffffffLL, RL_ERR_ARGS, "%s: M=%lld outside 1 .. 2^31-2", who, (long long)M);
    RL_REQUIRE(dim >= 3, RL_ERR_ARGS, "%s: dim=%d, the rows need x, y, z", who, dim);
    return rl_ws_check(who, ws, ws_bytes, rl_grid_workspace_bytes(M, dim));
}

}  // namespace

extern "C" int64_t rl_grid_workspace_bytes(int64_t M, int dim) {
    (void)dim;
    if (M <= 0 || M >= 0x7fffffffLL) return 0;
    return (int64_t)grid_layout(M).bytes;
}

extern "C" int rl_grid_bounds(const float* cloud, int64_t M, int dim, float cell, int64_t* dims_out, void* ws,
                              int64_t ws_bytes, void* stream) {
    RL_REQUIRE(cell > 0.f && isfinite(cell), RL_ERR_ARGS, "rl_grid_bounds: cell=%g must be positive and finite", (double)cell);
    int rc = grid_check("rl_grid_bounds", M, dim, ws, ws_bytes);
    if (rc) return rc;
    RL_REQUIRE(cloud && dims_out, RL_ERR_ARGS, "rl_grid_bounds: null pointer");
    hipStream_t sm = (hipStream_t)stream;
    float* box = rl_at<float>(ws, grid_layout(M).off_box);
    const long parts = grid_box_parts(M);
    hipLaunchKernelGGL(grid_box_partial, dim3((int)parts), dim3(GR_THREADS), 0, sm, cloud, (long)M, dim, box);
    RL_LAUNCH_CHECK("rl_grid_bounds (partial)");
    hipLaunchKernelGGL(grid_box_final, dim3(1), dim3(GR_THREADS), 0, sm, box, (int)parts, cell, (long)M, (GridState*)ws,
                       dims_out);
    rl_note_kernel("grid_box_final");
    RL_LAUNCH_CHECK("rl_grid_bounds (final)");
    return RL_OK;
}

extern "C" int rl_grid_sort(const float* cloud, int64_t M, int dim, int key_bits, void* ws, int64_t ws_bytes, void* stream) {
    RL_REQUIRE(key_bits >= 1 && key_bits <= 63, RL_ERR_ARGS, "rl_grid_sort: key_bits=%d outside 1 .. 63", key_bits);
    int rc = grid_check("rl_grid_sort", M, dim, ws, ws_bytes);
    if (rc) return rc;
    RL_REQUIRE(cloud, RL_ERR_ARGS, "rl_grid_sort: null pointer");
    hipStream_t sm = (hipStream_t)stream;
    const RadixBufs sort = radix_bufs(ws, grid_layout(M).sort);
    const int passes = grid_passes(key_bits);
    hipLaunchKernelGGL(grid_keys, dim3(rl_cdiv(M, GR_THREADS)), dim3(GR_THREADS), 0, sm, cloud, (long)M, dim,
                       (const GridState*)ws, sort.keys[passes & 1]);
    RL_LAUNCH_CHECK("rl_grid_sort (keys)");
    rc = radix_sort("rl_grid_sort", sort, (long)M, passes, sm);
    if (rc) return rc;
    rl_note_kernel("grid_scatter");      // (the sorted pairs are in buffer 0)
    return RL_OK;
}

extern "C" int rl_grid_heads(int64_t M, int dim, int64_t* V_out, int32_t* inverse, void* ws, int64_t ws_bytes, void* stream) {
    int rc = grid_check("rl_grid_heads", M, dim, ws, ws_bytes);
    if (rc) return rc;
    RL_REQUIRE(V_out && inverse, RL_ERR_ARGS, "rl_grid_heads: null pointer");
    hipStream_t sm = (hipStream_t)stream;
    const CellsLayout L = grid_layout(M);
    rc = grid_heads("rl_grid_heads", radix_bufs(ws, L.sort), (long)M, (GridState*)ws, V_out, inverse,
                    rl_at<uint32_t>(ws, L.off_cnt), rl_at<uint32_t>(ws, L.off_start), sm);
    rl_note_kernel("grid_head_write");
    return rc;
}

extern "C" int rl_grid_reduce(const float* cloud, int64_t M, int dim, const int64_t* labels, int n_classes, int64_t V,
                              float* rows_out, int64_t* labels_out, int32_t* count_out, void* ws, int64_t ws_bytes,
                              void* stream) {
    int rc = grid_check("rl_grid_reduce", M, dim, ws, ws_bytes);
    if (rc) return rc;
    RL_REQUIRE(V > 0 && V <= M, RL_ERR_ARGS, "rl_grid_reduce: V=%lld cells of M=%lld points", (long long)V, (long long)M);
    RL_REQUIRE(cloud && rows_out && count_out, RL_ERR_ARGS, "rl_grid_reduce: null pointer");
    RL_REQUIRE(!labels || (n_classes > 0 && labels_out), RL_ERR_ARGS,
               "rl_grid_reduce: labels need n_classes=%d > 0 and labels_out", n_classes);
    const CellsLayout L = grid_layout(M);
    hipLaunchKernelGGL(grid_reduce, dim3(rl_cdiv(V, GR_THREADS)), dim3(GR_THREADS), 0, (hipStream_t)stream, cloud, (long)M,
                       dim, rl_at<const uint32_t>(ws, L.sort.off_idx[0]), rl_at<const uint32_t>(ws, L.off_start),
                       (const GridState*)ws, labels, n_classes, (long)V, rows_out, labels_out, count_out);
    rl_note_kernel("grid_reduce");
    RL_LAUNCH_CHECK("rl_grid_reduce");
    return RL_OK;
}

extern "C" int rl_scene_confusion(const float* prob, int64_t V, int C, const int64_t* labels, int64_t M,
                                  const int32_t* inverse, int64_t* table, void* stream) {
    RL_REQUIRE(V > 0 && M > 0 && M < 0x7fffffffLL, RL_ERR_ARGS, "rl_scene_confusion: bad sizes V=%lld M=%lld", (long long)V,
               (long long)M);
    RL_REQUIRE(C > 0 && C <= 32768, RL_ERR_ARGS, "rl_scene_confusion: C=%d classes", C);
    RL_REQUIRE(inverse || V == M, RL_ERR_ARGS, "rl_scene_confusion: without inverse prob needs M=%lld rows, has V=%lld",
               (long long)M, (long long)V);
    RL_REQUIRE(prob && labels && table, RL_ERR_ARGS, "rl_scene_confusion: null pointer");
    long g = (M + 16 * GR_THREADS - 1) / (16 * GR_THREADS);
    g = g > 1024 ? 1024 : g;
    if (C <= GR_CONF_LDS_C)
        hipLaunchKernelGGL(scene_confusion<true>, dim3((int)g), dim3(GR_THREADS), 0, (hipStream_t)stream, prob, (long)V, C,
                           labels, (long)M, inverse, (unsigned long long*)table);
    else
        hipLaunchKernelGGL(scene_confusion<false>, dim3((int)g), dim3(GR_THREADS), 0, (hipStream_t)stream, prob, (long)V, C,
                           labels, (long)M, inverse, (unsigned long long*)table);
    rl_note_kernel("scene_confusion");
    RL_LAUNCH_CHECK("rl_scene_confusion");
    return RL_OK;
}
