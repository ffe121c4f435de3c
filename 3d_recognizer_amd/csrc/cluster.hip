// Euclidean clustering of labelled points (Model.predict_instances, utils/cluster.py: euclidean_clusters): the connected
// components of the graph that joins two participating points of the same label when d2 <= r2, numbered by their smallest
// point index, with count, class, centroid, bounding box and mean score per kept component.  The numpy twin is
// randlanet/utils/cluster.py; the components are a pure function of the input (the edge rule is a fixed fp32 expression, the
// numbering a property of the component), so the result equals the twin's bit for bit whatever the scheduling.
//
//   rl_cluster_cells   box_partial, box_final (rl_cells.h) over ALL points with the cell edge c = r * 1.0625f: origin and
//                      dims into the workspace, dims to the caller (who refuses 2^16 cells or more on an axis)
//   rl_cluster_union   keys       the cell key of a participating point, the sentinel dims_x*dims_y*dims_z for every other
//                                 point (sorted to the end); parent[i] = i, size[i] = 0
//                      sort       the stable radix sort of (key, point index) (rl_radix.h)
//                      pack       (x, y, z, low 32 bits of the label) of every sorted position: the scan reads neighbours
//                                 contiguously instead of gathering them
//                      union      one lane per sorted position j: the cells that precede its own in key order among the 27
//                                 around it - 4 rows of 3 cells found by a binary search over the sorted keys, and its own row
//                                 backwards from j - so that every joined pair is met exactly once, by the later of the two;
//                                 label equality and d2 <= r2, then hook (below)
//                      flatten    root[i] = find(i) (-1 for a point that takes no part); size[root] += 1 by integer atomics,
//                                 one per run of equal roots in a wavefront
//                      rootkeys   key = root when size[root] >= min_points, the sentinel M otherwise
//                      sort       (key, point index) again: segments are kept components in ascending root = ascending
//                                 smallest member, members in ascending index; everything dropped is the last segment
//                      heads      head_count, head_scan, head_write (rl_cells.h): segment of every point, segment starts
//                      finish     instance[i] = its segment or -1; I = segments without the sentinel's
//   rl_cluster_union_smooth   the smoothness-constrained rule (utils/cluster.py, "smooth edge"): the same launches with the
//                      kernels' SMOOTH = true instantiations.  keys and flatten: a point whose curvature lies above the maximum
//                      takes no part; pack: a second float4 per sorted position, (nx, ny, nz, 0), behind the plain workspace;
//                      union: a pair that passed the low-32-bit label test and d2 <= r2 - most candidates of the 14 cells fail
//                      on distance - then reads the other point's normal and needs abs((nx_i*nx_j + ny_i*ny_j) + nz_i*nz_j) >=
//                      cos_angle, un-fused fp32, before the hook.  The test is symmetric (fp32 multiplication commutes) and
//                      a pure function of the pair, so the components are again a pure function of the input.  The SMOOTH =
//                      false instantiations are the kernels of rl_cluster_union and hold nothing of the smooth rule; sorts,
//                      union-find, heads, finish and reduce are shared
//   rl_cluster_union_dense    the density rule (utils/cluster.py, "density": DBSCAN's min_samples): the same launches with the
//                      kernels' DENSE = true instantiations and two more between pack and union.
//                      support    one lane per sorted position: ALL 27 cells around its own as 9 rows of up to 3 contiguous
//                                 cells (grid_rows, rl_cells.h) - the rows after the own one too, because support is not
//                                 symmetric work that one of the two points can do for both -, counting near() under the
//                                 PLAIN rule, also when normals are given, and leaving at min_samples: support is only ever
//                                 compared with it.  core = support >= min_samples
//                      union      a pair is skipped unless both ends are core
//                      attach     one lane per sorted position: a core point gets itself; a participating point that is not
//                                 core walks the same 9 rows for the core points it has an edge to (the smooth edge with
//                                 normals) and keeps the minimum of (d2, point index): attach[i] = that core point, or -1
//                                 for noise and for a point that takes no part.  Runs after union only because nothing it
//                                 reads is written there; its result is a pure function of the input
//                      flatten    root[i] = find(attach[i]) where attach[i] >= 0, -1 otherwise: a core point its own root, a
//                                 border point the root of the core point it joined; size counts both.  Only core points were
//                                 hooked, so a root is its component's smallest CORE index, and the second sort numbers by it
//                      support (M) int32 by sorted position and attach (M) int32 by point index lie behind the workspace of
//                      the rule they extend.  The DENSE = false instantiations are the kernels of rl_cluster_union and
//                      rl_cluster_union_smooth and hold nothing of the density rule.  No atomics in support and attach: plain
//                      loads and vector stores
//   rl_cluster_reduce  one WAVEFRONT per instance: 64 members loaded at a time, then added one by one in member order in fp64
//                      (lanes 0 .. 3 own the chains of x, y, z, score); box by min / max; class and count
//   rl_scene_labels    one lane per row: argmax (ties to the lowest class), confidence = p[argmax] / (fp64 sum in class order)
//
// The union-find (after ECL-CC, Jaiganesh and Burtscher, HPDC 2018) is lock-free: no lane ever waits for another one.
//   invariant   parent[x] <= x always, and parent[x] is in x's component.  Only two writes exist: a successful compare-and-
//               swap parent[hi]: hi -> lo with lo < hi (hook), and parent[x] = g with g read as parent[parent[x]] <= parent[x]
//               < x (path halving; x is no root then and never becomes one again, so the store cannot undo a hook: hooks only
//               change roots).  A stale value read for parent[x] is a former ancestor: still below x, still in the component.
//   find        every step moves to a strictly smaller index or returns: at most x steps.
//   hook        the compare-and-swap fails only when parent[hi] != hi, i.e. another lane put hi under something smaller; the
//               retry starts from find(that value) < hi and find(lo) <= lo < hi, so max(ra, rb) falls strictly with every
//               failed attempt: at most hi attempts, whatever the other lanes do.
//   result      the larger root always goes under the smaller one, so every tree's root is its smallest index; once every
//               edge was hooked the trees are the components, and root = the component's smallest point index.
// parent is read and written by relaxed agent-scope atomics only (never hoisted, never served from a stale L1 line).
#include "rl_cells.h"

namespace {

constexpr int CL_MAX_DIM_BITS = 16;      // the caller refuses a grid of 2^16 cells or more on an axis
constexpr int CL_ROWS = 5;               // rows of cells a lane scans: 4 whole rows below its own, and its own

// the smooth rule's workspace is the plain one, then the normals of the sorted positions (rl_cluster_cells and
// rl_cluster_reduce never look at them and serve both rules); the density rule's is that of the rule it extends ([0] plain,
// [1] smooth), then support and attach
struct ClusterLayout {
    CellsLayout cells;
    size_t off_pts, off_parent, off_root, off_size, off_comp, bytes, off_nrm, smooth_bytes;
    size_t off_support[2], off_attach[2], dense_bytes[2];
};

ClusterLayout cluster_layout(long M) {
    ClusterLayout L;
    RlCarve c;
    L.cells = cells_layout(c, M);
    L.off_pts = c.take((size_t)M * sizeof(float4));
    L.off_parent = c.take((size_t)M * sizeof(int32_t));
    L.off_root = c.take((size_t)M * sizeof(int32_t));
    L.off_size = c.take((size_t)M * sizeof(int32_t));
    L.off_comp = c.take((size_t)M * sizeof(int32_t));
    L.bytes = c.at;
    L.off_nrm = c.take((size_t)M * sizeof(float4));
    L.smooth_bytes = c.at;
    for (int smooth = 0; smooth < 2; ++smooth) {
        RlCarve d;
        d.at = smooth ? L.smooth_bytes : L.bytes;
        L.off_support[smooth] = d.take((size_t)M * sizeof(int32_t));
        L.off_attach[smooth] = d.take((size_t)M * sizeof(int32_t));
        L.dense_bytes[smooth] = d.at;
    }
    return L;
}

__device__ __forceinline__ bool cl_takes_part(int64_t label, const int64_t* __restrict__ ignore, int n_ignore) {
    if (label < 0) return false;
    for (int k = 0; k < n_ignore; ++k)
        if (ignore[k] == label) return false;
    return true;
}

// the smooth rule's addition: a point whose curvature lies above the maximum takes no part (curvature NULL: no maximum)
template <bool SMOOTH>
__device__ __forceinline__ bool cl_takes_part(long i, int64_t label, const int64_t* __restrict__ ignore, int n_ignore,
                                              const float* __restrict__ curvature, float max_curvature) {
    if (!cl_takes_part(label, ignore, n_ignore)) return false;
    if constexpr (SMOOTH) {
        if (curvature && curvature[i] > max_curvature) return false;
    }
    return true;
}

__device__ __forceinline__ int cl_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cl_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x's tree, halving the path on the way.  Terminates: x falls strictly with every turn.
__device__ __forceinline__ int cl_find(int* __restrict__ parent, int x) {
    for (;;) {
        const int p = cl_load(parent + x);
        if (p >= x) return x;                 // a root (parent[x] > x does not exist)
        const int g = cl_load(parent + p);
        if (g >= p) return p;
        cl_store(parent + x, g);              // x is no root: this cannot collide with a hook, which only swaps roots
        x = g;
    }
}

// joins the trees of a and b, the larger root under the smaller one.  Terminates: a failed swap means parent[hi] fell below
// hi, and both new roots lie below hi, so max(ra, rb) falls strictly with every turn.
__device__ __forceinline__ void cl_hook(int* __restrict__ parent, int a, int b) {
    int ra = cl_find(parent, a), rb = cl_find(parent, b);
    while (ra != rb) {
        const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        int seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return;
        ra = cl_find(parent, seen);           // seen = parent[hi] < hi
        rb = cl_find(parent, lo);
    }
}

// SMOOTH = false is the Euclidean rule: curvature, max_curvature (keys, flatten), normals, nrm (pack) and nrm, cos_t (union,
// try) are never read, and the instantiation holds no instruction of the smooth rule.
template <bool SMOOTH>
__global__ __launch_bounds__(GR_THREADS) void cl_keys(const float* __restrict__ xyz, const int64_t* __restrict__ labels,
                                                       long M, const int64_t* __restrict__ ignore, int n_ignore,
                                                       const GridState* __restrict__ st, uint64_t* __restrict__ keys,
                                                       int* __restrict__ parent, int* __restrict__ size,
                                                       const float* __restrict__ curvature, float max_curvature) {
    const long i = (long)blockIdx.x * GR_THREADS + threadIdx.x;
    if (i >= M) return;
    const uint64_t sentinel = (uint64_t)(st->dims[0] * st->dims[1] * st->dims[2]);
    keys[i] = cl_takes_part<SMOOTH>(i, labels[i], ignore, n_ignore, curvature, max_curvature) ? grid_cell_key(xyz + i * 3, st)
                                                                                              : sentinel;
    parent[i] = (int)i;
    size[i] = 0;
}

template <bool SMOOTH>
__global__ __launch_bounds__(GR_THREADS) void cl_pack(const float* __restrict__ xyz, const int64_t* __restrict__ labels,
                                                       const uint32_t* __restrict__ idx, long M, float4* __restrict__ pts,
                                                       const float* __restrict__ normals, float4* __restrict__ nrm) {
    const long j = (long)blockIdx.x * GR_THREADS + threadIdx.x;
    if (j >= M) return;
    const long i = idx[j];
    if (i >= M) return;                       // (never: idx is a permutation)
    const float* p = xyz + i * 3;
    pts[j] = make_float4(p[0], p[1], p[2], __int_as_float((int)(uint32_t)(uint64_t)labels[i]));
    if constexpr (SMOOTH) {
        const float* n = normals + i * 3;
        nrm[j] = make_float4(n[0], n[1], n[2], 0.f);
    }
}

// the plain edge's distance part, un-fused fp32: d2 <= r2 (d2 to the caller)
__device__ __forceinline__ bool cl_within(const float4 a, const float4 b, float r2, float& d2) {
    const float dx = __fsub_rn(a.x, b.x), dy = __fsub_rn(a.y, b.y), dz = __fsub_rn(a.z, b.z);
    d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    return d2 <= r2;
}

// the smooth edge's addition: unsigned, whichever way a normal was turned; a zero normal joins nobody
__device__ __forceinline__ bool cl_agree(const float4 a, const float4 b, float cos_t) {
    const float dot = __fadd_rn(__fadd_rn(__fmul_rn(a.x, b.x), __fmul_rn(a.y, b.y)), __fmul_rn(a.z, b.z));
    return fabsf(dot) >= cos_t;
}

// DENSE = false is the rule without min_samples: support and min_s (union, try) and attach (flatten) are never read, and the
// instantiation holds no instruction of the density rule.
template <bool SMOOTH, bool DENSE>
__device__ __forceinline__ void cl_try(const float4 me, int i, int64_t mylab, long jj, const float4* __restrict__ pts,
                                       const uint32_t* __restrict__ idx, const int64_t* __restrict__ labels, float r2,
                                       int* __restrict__ parent, const float4 mynrm, const float4* __restrict__ nrm,
                                       float cos_t, const int32_t* __restrict__ support, int min_s) {
    const float4 q = pts[jj];
    if (__float_as_int(q.w) != __float_as_int(me.w)) return;
    const float dx = __fsub_rn(me.x, q.x), dy = __fsub_rn(me.y, q.y), dz = __fsub_rn(me.z, q.z);
    const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    if (!(d2 <= r2)) return;
    if constexpr (DENSE) {                    // only two core points are joined
        if (support[jj] < min_s) return;
    }
    if constexpr (SMOOTH) {                   // the normal is read for the pairs that are close only, not for every candidate
        const float4 n = nrm[jj];
        const float dot = __fadd_rn(__fadd_rn(__fmul_rn(mynrm.x, n.x), __fmul_rn(mynrm.y, n.y)), __fmul_rn(mynrm.z, n.z));
        if (!(fabsf(dot) >= cos_t)) return;   // unsigned: whichever way a normal was turned; a zero normal joins nobody
    }
    const int k = (int)idx[jj];
    if (labels[k] != mylab) return;           // (labels that differ above bit 31 only)
    cl_hook(parent, i, k);
}

template <bool SMOOTH, bool DENSE>
__global__ __launch_bounds__(GR_THREADS) void cl_union(const int64_t* __restrict__ labels, long M,
                                                        const GridState* __restrict__ st, const uint64_t* __restrict__ keys,
                                                        const uint32_t* __restrict__ idx, const float4* __restrict__ pts,
                                                        float r2, int* __restrict__ parent, const float4* __restrict__ nrm,
                                                        float cos_t, const int32_t* __restrict__ support, int min_s) {
    const long j = (long)blockIdx.x * GR_THREADS + threadIdx.x;
    if (j >= M) return;
    const int64_t dx = st->dims[0], dy = st->dims[1], dz = st->dims[2];
    const uint64_t key = keys[j];
    if (key >= (uint64_t)(dx * dy * dz)) return;             // takes no part
    if constexpr (DENSE) {
        if (support[j] < min_s) return;                      // no core point: joins nobody here (attach places it)
    }
    const int i = (int)idx[j];
    if (i < 0 || i >= M) return;                             // (never)
    const float4 me = pts[j];
    float4 mynrm = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (SMOOTH) mynrm = nrm[j];
    const int64_t mylab = labels[i];
    const int64_t vx = (int64_t)(key % (uint64_t)dx), t = (int64_t)(key / (uint64_t)dx), vy = t % dy, vz = t / dy;
    const int64_t x0 = vx > 0 ? vx - 1 : 0, x1 = vx + 1 < dx ? vx + 1 : dx - 1;
    // the rows below the own one in key order: (z-1, y-1), (z-1, y), (z-1, y+1), (z, y-1), cells x0 .. x1
    for (int r = 0; r < CL_ROWS - 1; ++r) {
        const int64_t z = r < 3 ? vz - 1 : vz, y = r < 3 ? vy - 1 + r : vy - 1;
        if (z < 0 || y < 0 || y >= dy) continue;
        const uint64_t klo = (uint64_t)((z * dy + y) * dx + x0), khi = (uint64_t)((z * dy + y) * dx + x1);
        for (long jj = grid_lower_bound(keys, M, klo); jj < M && keys[jj] <= khi; ++jj)
            cl_try<SMOOTH, DENSE>(me, i, mylab, jj, pts, idx, labels, r2, parent, mynrm, nrm, cos_t, support, min_s);
    }
    // the own row: the cell before and the own cell up to the own position
    const uint64_t klo = key - (uint64_t)(vx - x0);
    for (long jj = j - 1; jj >= 0 && keys[jj] >= klo; --jj)
        cl_try<SMOOTH, DENSE>(me, i, mylab, jj, pts, idx, labels, r2, parent, mynrm, nrm, cos_t, support, min_s);
}

// support[j] = min(support of the point at sorted position j, min_s) under the plain rule, 0 for a point that takes no part (its
// key is the sentinel, and no row reaches the sentinel: such points are never counted either)
__global__ __launch_bounds__(GR_THREADS) void cl_support(const int64_t* __restrict__ labels, long M,
                                                          const GridState* __restrict__ st, const uint64_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ idx, const float4* __restrict__ pts,
                                                          float r2, int min_s, int32_t* __restrict__ support) {
    const long j = (long)blockIdx.x * GR_THREADS + threadIdx.x;
    if (j >= M) return;
    const uint64_t key = keys[j];
    int32_t n = 0;
    if (key < (uint64_t)(st->dims[0] * st->dims[1] * st->dims[2]) && idx[j] < M) {
        const float4 me = pts[j];
        const int64_t mylab = labels[idx[j]];
        grid_rows(key, st, [&](uint64_t klo, uint64_t khi) {
            for (long jj = grid_lower_bound(keys, M, klo); jj < M && keys[jj] <= khi; ++jj) {
                const float4 q = pts[jj];
                float d2;
                if (__float_as_int(q.w) != __float_as_int(me.w) || !cl_within(me, q, r2, d2)) continue;
                if (labels[idx[jj]] != mylab) continue;      // (labels that differ above bit 31 only)
                if (++n >= min_s) return false;              // core: nothing more to learn
            }
            return true;
        });
    }
    support[j] = n;
}

// attach[i] of the point i at sorted position j: i for a core point, the core point it joins for a border point, -1 otherwise
template <bool SMOOTH>
__global__ __launch_bounds__(GR_THREADS) void cl_attach(const int64_t* __restrict__ labels, long M,
                                                         const GridState* __restrict__ st, const uint64_t* __restrict__ keys,
                                                         const uint32_t* __restrict__ idx, const float4* __restrict__ pts,
                                                         float r2, const int32_t* __restrict__ support, int min_s,
                                                         const float4* __restrict__ nrm, float cos_t,
                                                         int32_t* __restrict__ attach) {
    const long j = (long)blockIdx.x * GR_THREADS + threadIdx.x;
    if (j >= M) return;
    const uint32_t i = idx[j];
    if (i >= M) return;                       // (never: idx is a permutation, so all of attach is written)
    const uint64_t key = keys[j];
    int a = -1;
    if (key < (uint64_t)(st->dims[0] * st->dims[1] * st->dims[2])) {
        if (support[j] >= min_s) {
            a = (int)i;
        } else {
            const float4 me = pts[j];
            float4 mynrm = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (SMOOTH) mynrm = nrm[j];
            const int64_t mylab = labels[i];
            float best = 0.f;
            grid_rows(key, st, [&](uint64_t klo, uint64_t khi) {
                for (long jj = grid_lower_bound(keys, M, klo); jj < M && keys[jj] <= khi; ++jj) {
                    if (support[jj] < min_s) continue;       // (jj == j is no core point)
                    const float4 q = pts[jj];
                    float d2;
                    if (__float_as_int(q.w) != __float_as_int(me.w) || !cl_within(me, q, r2, d2)) continue;
                    const int k = (int)idx[jj];
                    if (!(a < 0 || d2 < best || (d2 == best && k < a))) continue;    // the minimum of (d2, point index)
                    if constexpr (SMOOTH) {
                        if (!cl_agree(mynrm, nrm[jj], cos_t)) continue;
                    }
                    if (k < 0 || k >= M || labels[k] != mylab) continue;
                    best = d2;
                    a = k;
                }
                return true;
            });
        }
    }
    attach[i] = a;
}

template <bool SMOOTH, bool DENSE>
__global__ __launch_bounds__(GR_THREADS) void cl_flatten(const int64_t* __restrict__ labels, long M,
                                                          const int64_t* __restrict__ ignore, int n_ignore,
                                                          int* __restrict__ parent, int* __restrict__ root,
                                                          int* __restrict__ size, const float* __restrict__ curvature,
                                                          float max_curvature, const int32_t* __restrict__ attach) {
    const long i = (long)blockIdx.x * GR_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int r = -1;
    if constexpr (DENSE) {                    // a core point: itself; a border point: the core point it joined
        const int a = i < M ? attach[i] : -1;
        if (a >= 0 && a < M) r = cl_find(parent, a);
    } else {
        if (i < M && cl_takes_part<SMOOTH>(i, labels[i], ignore, n_ignore, curvature, max_curvature))
            r = cl_find(parent, (int)i);
    }
    if (i < M) root[i] = r;
    // one integer atomic per run of equal roots in the wavefront (a component's points often follow each other)
    const int before = __shfl_up(r, 1, 64);
    const bool head = lane == 0 || before != r;
    const unsigned long long heads = __ballot(head);
    if (head && r >= 0) {
        const unsigned long long above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
        const int next = above ? __ffsll((long long)above) - 1 : 64;
        atomicAdd(size + r, next - lane);
    }
}

__global__ __launch_bounds__(GR_THREADS) void cl_rootkeys(const int* __restrict__ root, const int* __restrict__ size, long M,
                                                           int min_points, uint64_t* __restrict__ keys) {
    const long i = (long)blockIdx.x * GR_THREADS + threadIdx.x;
    if (i >= M) return;
    const int r = root[i];
    keys[i] = r >= 0 && r < M && size[r] >= min_points ? (uint64_t)r : (uint64_t)M;
}

__global__ __launch_bounds__(GR_THREADS) void cl_finish(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx,
                                                         const int32_t* __restrict__ comp, long M,
                                                         GridState* __restrict__ st, int32_t* __restrict__ instance,
                                                         int64_t* __restrict__ I_out) {
    const long j = (long)blockIdx.x * GR_THREADS + threadIdx.x;
    if (j >= M) return;
    const long i = idx[j];
    if (i < M) instance[i] = keys[j] < (uint64_t)M ? comp[i] : -1;
    if (j == M - 1) {
        const int64_t I = st->V - (keys[j] < (uint64_t)M ? 0 : 1);       // the dropped points are the last segment
        st->pad[1] = I;
        I_out[0] = I;
    }
}

// one wavefront per instance; the segment in sorted order = ascending point index
__global__ __launch_bounds__(GR_THREADS) void cl_reduce(const float* __restrict__ xyz, const int64_t* __restrict__ labels,
                                                         const float* __restrict__ scores, long M, long I,
                                                         const uint32_t* __restrict__ idx, const uint32_t* __restrict__ start,
                                                         const GridState* __restrict__ st, int64_t* __restrict__ classes_out,
                                                         int32_t* __restrict__ count_out, float* __restrict__ centroid_out,
                                                         float* __restrict__ lo_out, float* __restrict__ hi_out,
                                                         float* __restrict__ score_out) {
    const int lane = threadIdx.x & 63;
    const long k = (long)blockIdx.x * GR_WAVES + (threadIdx.x >> 6);
    if (k >= I || k >= st->pad[1]) return;                   // wavefront-uniform
    long j0 = start[k], j1 = start[k + 1];
    j1 = j1 > M ? M : j1;
    if (j0 >= j1) return;                                    // (never: a segment holds a point)
    double acc = 0.0;                                        // lane 0: x, 1: y, 2: z, 3: score
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long base = j0; base < j1; base += 64) {
        const long j = base + lane;
        const bool live = j < j1;
        long i = idx[live ? j : j0];
        i = i < M ? i : 0;                                   // (never)
        const float* p = xyz + i * 3;
        const float v0 = p[0], v1 = p[1], v2 = p[2], v3 = scores ? scores[i] : 0.f;
        if (live) {
            lo[0] = fminf(lo[0], v0); lo[1] = fminf(lo[1], v1); lo[2] = fminf(lo[2], v2);
            hi[0] = fmaxf(hi[0], v0); hi[1] = fmaxf(hi[1], v1); hi[2] = fmaxf(hi[2], v2);
        }
        const int n = (int)(j1 - base < 64 ? j1 - base : 64);
        for (int t = 0; t < n; ++t) {                        // member after member: the fixed order of the contract
            // (t is wavefront-uniform: four v_readlane_b32, no trip through the LDS crossbar)
            const float a0 = grid_lane(v0, t), a1 = grid_lane(v1, t), a2 = grid_lane(v2, t), a3 = grid_lane(v3, t);
            acc += (double)(lane == 0 ? a0 : lane == 1 ? a1 : lane == 2 ? a2 : a3);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
        for (int o = 32; o >= 1; o >>= 1) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], o, 64));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o, 64));
        }
    const double n = (double)(j1 - j0);
    if (lane < 3) centroid_out[k * 3 + lane] = (float)(acc / n);
    if (lane == 3 && score_out) score_out[k] = (float)(acc / n);
    if (lane == 0) {
        count_out[k] = (int32_t)(j1 - j0);
        classes_out[k] = labels[idx[j0] < M ? idx[j0] : 0];
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo_out[k * 3 + a] = lo[a]; hi_out[k * 3 + a] = hi[a]; }
    }
}

__global__ __launch_bounds__(GR_THREADS) void scene_labels(const float* __restrict__ prob, long V, int C, float min_confidence,
                                                            int64_t* __restrict__ labels_out, float* __restrict__ conf_out) {
    const long v = (long)blockIdx.x * GR_THREADS + threadIdx.x;
    if (v >= V) return;
    const float* p = prob + v * C;
    int best = 0;
    float pb = p[0];
    double s = (double)p[0];
    for (int c = 1; c < C; ++c) {
        if (p[c] > pb) pb = p[c], best = c;                  // strictly greater: ties stay with the lowest class
        s += (double)p[c];
    }
    const float conf = (float)((double)pb / s);
    conf_out[v] = conf;
    labels_out[v] = conf < min_confidence ? -1 : best;
}

int cluster_check(const char* who, int64_t M, const void* ws, int64_t ws_bytes, bool smooth = false, bool dense = false) {
    RL_REQUIRE(M > 0 && M < 0x7fffffffLL, RL_ERR_ARGS, "%s: M=%lld outside 1 .. 2^31-2", who, (long long)M);
    return rl_ws_check(who, ws, ws_bytes,
                       dense    ? rl_cluster_dense_workspace_bytes(M, smooth)
                       : smooth ? rl_cluster_smooth_workspace_bytes(M)
                                : rl_cluster_workspace_bytes(M));
}

}  // namespace

extern "C" int64_t rl_cluster_workspace_bytes(int64_t M) {
    if (M <= 0 || M >= 0x7fffffffLL) return 0;
    return (int64_t)cluster_layout(M).bytes;
}

extern "C" int64_t rl_cluster_smooth_workspace_bytes(int64_t M) {
    if (M <= 0 || M >= 0x7fffffffLL) return 0;
    return (int64_t)cluster_layout(M).smooth_bytes;
}

extern "C" int64_t rl_cluster_dense_workspace_bytes(int64_t M, int smooth) {
    if (M <= 0 || M >= 0x7fffffffLL) return 0;
    return (int64_t)cluster_layout(M).dense_bytes[smooth ? 1 : 0];
}

extern "C" int rl_cluster_cells(const float* xyz, int64_t M, float radius, int64_t* dims_out, void* ws, int64_t ws_bytes,
                                void* stream) {
    RL_REQUIRE(radius > 0.f && isfinite(radius), RL_ERR_ARGS, "rl_cluster_cells: radius=%g must be positive and finite",
               (double)radius);
    int rc = cluster_check("rl_cluster_cells", M, ws, ws_bytes);
    if (rc) return rc;
    RL_REQUIRE(xyz && dims_out, RL_ERR_ARGS, "rl_cluster_cells: null pointer");
    const float cell = radius * 1.0625f;
    RL_REQUIRE(isfinite(cell), RL_ERR_ARGS, "rl_cluster_cells: radius=%g is too large", (double)radius);
    hipStream_t sm = (hipStream_t)stream;
    float* box = rl_at<float>(ws, cluster_layout(M).cells.off_box);
    const long parts = grid_box_parts(M);
    hipLaunchKernelGGL(grid_box_partial, dim3((int)parts), dim3(GR_THREADS), 0, sm, xyz, (long)M, 3, box);
    RL_LAUNCH_CHECK("rl_cluster_cells (partial)");
    hipLaunchKernelGGL(grid_box_final, dim3(1), dim3(GR_THREADS), 0, sm, box, (int)parts, cell, (long)M, (GridState*)ws,
                       dims_out);
    rl_note_kernel("grid_box_final");
    RL_LAUNCH_CHECK("rl_cluster_cells (final)");
    return RL_OK;
}

// rl_cluster_union (SMOOTH = false: normals, curvature, cos_angle and max_curvature are not looked at),
// rl_cluster_union_smooth and rl_cluster_union_dense (DENSE = true; otherwise min_samples is not looked at)
template <bool SMOOTH, bool DENSE>
static int cluster_union(const char* who, const float* xyz, const int64_t* labels, int64_t M, float radius, const int64_t* ignore,
                  int n_ignore, int key_bits, int64_t min_points, const float* normals, const float* curvature, float cos_angle,
                  float max_curvature, int64_t min_samples, int32_t* instance_out, int64_t* I_out, void* ws, int64_t ws_bytes,
                  void* stream) {
    RL_REQUIRE(radius > 0.f && isfinite(radius) && isfinite(radius * radius), RL_ERR_ARGS,
               "%s: radius=%g must be positive and finite", who, (double)radius);
    RL_REQUIRE(key_bits >= 1 && key_bits <= 3 * CL_MAX_DIM_BITS + 1, RL_ERR_ARGS, "%s: key_bits=%d outside 1 .. %d", who,
               key_bits, 3 * CL_MAX_DIM_BITS + 1);
    RL_REQUIRE(min_points >= 1, RL_ERR_ARGS, "%s: min_points=%lld", who, (long long)min_points);
    RL_REQUIRE(n_ignore >= 0 && (n_ignore == 0 || ignore), RL_ERR_ARGS, "%s: %d ignored classes without a list", who,
               n_ignore);
    if (SMOOTH) {
        RL_REQUIRE(cos_angle > 0.f && cos_angle <= 1.f, RL_ERR_ARGS, "%s: cos_angle=%g outside (0, 1]", who, (double)cos_angle);
        RL_REQUIRE(!curvature || !(max_curvature != max_curvature), RL_ERR_ARGS, "%s: max_curvature is not a number", who);
    }
    if (DENSE) RL_REQUIRE(min_samples >= 1, RL_ERR_ARGS, "%s: min_samples=%lld", who, (long long)min_samples);
    int rc = cluster_check(who, M, ws, ws_bytes, SMOOTH, DENSE);
    if (rc) return rc;
    RL_REQUIRE(xyz && labels && instance_out && I_out && (!SMOOTH || normals), RL_ERR_ARGS, "%s: null pointer", who);
    hipStream_t sm = (hipStream_t)stream;
    const ClusterLayout L = cluster_layout(M);
    GridState* st = (GridState*)ws;
    const RadixBufs sort = radix_bufs(ws, L.cells.sort);
    uint64_t* const* keys = sort.keys;
    uint32_t* const* idx = sort.idx;
    float4* pts = rl_at<float4>(ws, L.off_pts);
    float4* nrm = SMOOTH ? rl_at<float4>(ws, L.off_nrm) : nullptr;
    int* parent = rl_at<int>(ws, L.off_parent);
    int* root = rl_at<int>(ws, L.off_root);
    int* size = rl_at<int>(ws, L.off_size);
    int32_t* comp = rl_at<int32_t>(ws, L.off_comp);
    int32_t* support = DENSE ? rl_at<int32_t>(ws, L.off_support[SMOOTH]) : nullptr;
    int32_t* attach = DENSE ? rl_at<int32_t>(ws, L.off_attach[SMOOTH]) : nullptr;
    const int min_s = DENSE ? (int)(min_samples > M ? M + 1 : min_samples) : 1;
    const dim3 grid(rl_cdiv(M, GR_THREADS)), block(GR_THREADS);
    const float r2 = radius * radius;
    const int min_pts = (int)(min_points > M ? M + 1 : min_points);

    int passes = grid_passes(key_bits);
    hipLaunchKernelGGL(cl_keys<SMOOTH>, grid, block, 0, sm, xyz, labels, (long)M, ignore, n_ignore, st, keys[passes & 1], parent,
                       size, curvature, max_curvature);
    RL_LAUNCH_CHECK("rl_cluster_union (keys)");
    rc = radix_sort("rl_cluster_union (cells)", sort, (long)M, passes, sm);
    if (rc) return rc;
    hipLaunchKernelGGL(cl_pack<SMOOTH>, grid, block, 0, sm, xyz, labels, idx[0], (long)M, pts, normals, nrm);
    RL_LAUNCH_CHECK("rl_cluster_union (pack)");
    if (DENSE) {
        hipLaunchKernelGGL(cl_support, grid, block, 0, sm, labels, (long)M, st, keys[0], idx[0], pts, r2, min_s, support);
        rl_note_kernel("cl_support");
        RL_LAUNCH_CHECK("rl_cluster_union_dense (support)");
    }
    hipLaunchKernelGGL((cl_union<SMOOTH, DENSE>), grid, block, 0, sm, labels, (long)M, st, keys[0], idx[0], pts, r2, parent, nrm,
                       cos_angle, support, min_s);
    RL_LAUNCH_CHECK("rl_cluster_union (union)");
    if (DENSE) {
        hipLaunchKernelGGL(cl_attach<SMOOTH>, grid, block, 0, sm, labels, (long)M, st, keys[0], idx[0], pts, r2, support, min_s,
                           nrm, cos_angle, attach);
        rl_note_kernel("cl_attach");
        RL_LAUNCH_CHECK("rl_cluster_union_dense (attach)");
    }
    hipLaunchKernelGGL((cl_flatten<SMOOTH, DENSE>), grid, block, 0, sm, labels, (long)M, ignore, n_ignore, parent, root, size,
                       curvature, max_curvature, attach);
    RL_LAUNCH_CHECK("rl_cluster_union (flatten)");
    passes = grid_passes(rl_bits_of(M));
    hipLaunchKernelGGL(cl_rootkeys, grid, block, 0, sm, root, size, (long)M, min_pts, keys[passes & 1]);
    RL_LAUNCH_CHECK("rl_cluster_union (rootkeys)");
    rc = radix_sort("rl_cluster_union (roots)", sort, (long)M, passes, sm);
    if (rc) return rc;
    rc = grid_heads("rl_cluster_union", sort, (long)M, st, &st->pad[0], comp, rl_at<uint32_t>(ws, L.cells.off_cnt),
                    rl_at<uint32_t>(ws, L.cells.off_start), sm);
    if (rc) return rc;
    hipLaunchKernelGGL(cl_finish, grid, block, 0, sm, keys[0], idx[0], comp, (long)M, st, instance_out, I_out);
    rl_note_kernel("cl_finish");
    RL_LAUNCH_CHECK("rl_cluster_union (finish)");
    return RL_OK;
}

extern "C" int rl_cluster_union(const float* xyz, const int64_t* labels, int64_t M, float radius, const int64_t* ignore,
                                int n_ignore, int key_bits, int64_t min_points, int32_t* instance_out, int64_t* I_out, void* ws,
                                int64_t ws_bytes, void* stream) {
    return cluster_union<false, false>("rl_cluster_union", xyz, labels, M, radius, ignore, n_ignore, key_bits, min_points,
                                       nullptr, nullptr, 0.f, 0.f, 1, instance_out, I_out, ws, ws_bytes, stream);
}

extern "C" int rl_cluster_union_smooth(const float* xyz, const int64_t* labels, int64_t M, float radius, const int64_t* ignore,
                                       int n_ignore, int key_bits, int64_t min_points, const float* normals,
                                       const float* curvature, float cos_angle, float max_curvature, int32_t* instance_out,
                                       int64_t* I_out, void* ws, int64_t ws_bytes, void* stream) {
    return cluster_union<true, false>("rl_cluster_union_smooth", xyz, labels, M, radius, ignore, n_ignore, key_bits, min_points,
                                      normals, curvature, cos_angle, max_curvature, 1, instance_out, I_out, ws, ws_bytes, stream);
}

extern "C" int rl_cluster_union_dense(const float* xyz, const int64_t* labels, int64_t M, float radius, const int64_t* ignore,
                                      int n_ignore, int key_bits, int64_t min_points, const float* normals,
                                      const float* curvature, float cos_angle, float max_curvature, int64_t min_samples,
                                      int32_t* instance_out, int64_t* I_out, void* ws, int64_t ws_bytes, void* stream) {
    const char* who = "rl_cluster_union_dense";
    if (normals)
        return cluster_union<true, true>(who, xyz, labels, M, radius, ignore, n_ignore, key_bits, min_points, normals, curvature,
                                         cos_angle, max_curvature, min_samples, instance_out, I_out, ws, ws_bytes, stream);
    RL_REQUIRE(!curvature, RL_ERR_ARGS, "%s: curvature without normals", who);
    return cluster_union<false, true>(who, xyz, labels, M, radius, ignore, n_ignore, key_bits, min_points, nullptr, nullptr, 0.f,
                                      0.f, min_samples, instance_out, I_out, ws, ws_bytes, stream);
}

extern "C" int rl_cluster_reduce(const float* xyz, const int64_t* labels, const float* scores, int64_t M, int64_t I,
                                 int64_t* classes_out, int32_t* count_out, float* centroid_out, float* lo_out, float* hi_out,
                                 float* score_out, void* ws, int64_t ws_bytes, void* stream) {
    int rc = cluster_check("rl_cluster_reduce", M, ws, ws_bytes);
    if (rc) return rc;
    RL_REQUIRE(I > 0 && I <= M, RL_ERR_ARGS, "rl_cluster_reduce: I=%lld instances of M=%lld points", (long long)I, (long long)M);
    RL_REQUIRE(xyz && labels && classes_out && count_out && centroid_out && lo_out && hi_out, RL_ERR_ARGS,
               "rl_cluster_reduce: null pointer");
    RL_REQUIRE(!scores == !score_out, RL_ERR_ARGS, "rl_cluster_reduce: scores and score_out go together");
    const CellsLayout L = cluster_layout(M).cells;
    hipLaunchKernelGGL(cl_reduce, dim3(rl_cdiv(I, GR_WAVES)), dim3(GR_THREADS), 0, (hipStream_t)stream, xyz, labels, scores,
                       (long)M, (long)I, rl_at<const uint32_t>(ws, L.sort.off_idx[0]), rl_at<const uint32_t>(ws, L.off_start),
                       (const GridState*)ws, classes_out, count_out, centroid_out, lo_out, hi_out, score_out);
    rl_note_kernel("cl_reduce");
    RL_LAUNCH_CHECK("rl_cluster_reduce");
    return RL_OK;
}

extern "C" int rl_scene_labels(const float* prob, int64_t V, int C, float min_confidence, int64_t* labels_out, float* conf_out,
                               void* stream) {
    RL_REQUIRE(V > 0 && V < 0x7fffffffLL, RL_ERR_ARGS, "rl_scene_labels: V=%lld outside 1 .. 2^31-2", (long long)V);
    RL_REQUIRE(C > 0 && C <= 32768, RL_ERR_ARGS, "rl_scene_labels: C=%d classes", C);
    RL_REQUIRE(!(min_confidence != min_confidence), RL_ERR_ARGS, "rl_scene_labels: min_confidence is not a number");
    RL_REQUIRE(prob && labels_out && conf_out, RL_ERR_ARGS, "rl_scene_labels: null pointer");
    hipLaunchKernelGGL(scene_labels, dim3(rl_cdiv(V, GR_THREADS)), dim3(GR_THREADS), 0, (hipStream_t)stream, prob, (long)V, C,
                       min_confidence, labels_out, conf_out);
    rl_note_kernel("scene_labels");
    RL_LAUNCH_CHECK("rl_scene_labels");
    return RL_OK;
}
