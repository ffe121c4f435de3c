// The Lovasz-Softmax loss (Berman et al., CVPR 2018) on (B, C, N) logits, alone or summed with the masked cross entropy: the
// mIoU surrogate of the un-fused head path.  The numpy twin of every step is randlanet/utils/lovasz.py, which is the
// specification: the softmax is exp_fixed's (rl_fixed.h), so every error e = |[y = c] - p_c| is the twin's float32 bit for bit,
// the order of a class' errors is an integer sort, and every coefficient is one fixed fp64 expression of exact integers - the
// (C, B*N) table `coef` equals the twin's bit for bit and is a pure function of the input (no floating-point atomics, no arrival
// order anywhere, no host read-back: the number of labelled points P and the class counts G_c are device state).
//
//   rl_lovasz_forward   rl_loss_forward_masked (kind 0, masked) on its own region of the workspace: the record's counts, the cross
//                       entropy, and in its totals record G_c (label counts) for everything below
//                       keys     one thread per point: softmax, then per class key = fg << 63 | class << 32 | ~bits(e) at position
//                                class * B*N + point; an unlabelled point's keys carry class C and sort to the tail
//                       sort     rl_radix.h's radix_sort: hist / scan / scatter per 8-bit digit over the 32 + bitlength(C) low bits: class
//                                ascending, e descending, ties in ascending point index (stable); bit 63 rides along
//                       count    per chunk of sorted positions the number of foreground keys
//                       prefix   one workgroup: P, the prefix of G_c over the classes, W = sum of w_c over the present classes,
//                                and the exclusive prefix of the chunk counts.  Class c owns positions [c*P, (c+1)*P), and all
//                                foreground keys of the classes below c lie below c*P: cum_r = (foreground keys up to the
//                                position) - (G of the classes below) - no segmented scan
//                       coef     one wavefront per chunk, 64 positions at a time, foreground ranked by ballots:
//                                J_r = 1 - (G - cum_r) / (G + r - cum_r), g_r = J_r - J_(r-1) in fp64, coef[class][point] =
//                                (float)g_r (0 for absent classes and unlabelled points: every entry is written), and the chunk's
//                                fp64 sum of e * g_r * w_c in a fixed order
//                       finalize one workgroup: the chunk sums in index order / W -> out[0] (+ the cross entropy with with_ce)
//   rl_lovasz_backward  (with_ce: rl_loss_backward_masked first) one thread per point: p again, d_c = sign(p_c - fg) coef w_c / W,
//                       dz_k = p_k (d_k - sum_c d_c p_c) * grad_scale, written or added to the cross entropy's gradient
// No workgroup waits for another one: every scan over the whole array is split over launches.
#include "rl_common.h"
#include "rl_fixed.h"
#include "rl_radix.h"

#include <math.h>

namespace {

constexpr int LV_THREADS = 256;
constexpr uint64_t LV_FG = 1ull << 63;       // foreground flag of a key: above every digit the sort looks at
constexpr uint32_t LV_CLASS_MASK = 0x1ffu;   // class field of a key, bits 32 .. 40: 0 .. RL_MAX_CLASSES (= unlabelled at C = 256)

struct LvState {
    int64_t P;                               // labelled points
    double W;                                // sum of w_c over the present classes
    int64_t pad[2];
    int64_t gpre[RL_MAX_CLASSES + 1];        // labelled points of the classes below c; gpre[C] = P
};

struct LvLayout {
    long M, T;       // points, keys
    RadixLayout sort;
    size_t off_loss, off_cnt, off_part, off_coef, bytes;
};

bool lv_supported(int B, int C, int N) {
    return B > 0 && N > 0 && C >= 1 && C <= RL_MAX_CLASSES && (int64_t)B * N * C < (1ll << 31);
}

LvLayout lv_layout(int B, int C, int N) {
    LvLayout L;
    RlCarve c;
    L.M = (long)B * N;
    L.T = L.M * C;
    // the per-chunk arrays are sized by a bound on `chunks` that never falls when T rises (the chunk size steps up with T)
    long cap = (L.T + GR_MIN_CHUNK - 1) / GR_MIN_CHUNK;
    cap = cap > GR_MAX_CHUNKS ? GR_MAX_CHUNKS : cap;
    c.take(sizeof(LvState));
    L.off_loss = c.take((size_t)rl_loss_work_doubles(L.M, C) * sizeof(double));
    L.sort = radix_layout(c, L.T, cap);
    L.off_cnt = c.take((size_t)cap * sizeof(uint32_t));
    L.off_part = c.take((size_t)cap * sizeof(double));
    L.off_coef = c.take((size_t)L.T * sizeof(float));       // the last piece: rl_lovasz_coef_offset
    L.bytes = c.at;
    return L;
}

int lv_key_bits(int C) {
    int bits = 0;
    for (int v = C; v > 0; v >>= 1) ++bits;      // the class field holds 0 .. C
    return 32 + bits;
}

// softmax_fixed of one point (utils/scene.py): the maximum, then the denominator summed in class order
__device__ __forceinline__ void lv_softmax_head(const float* __restrict__ z, long N, int C, float& m, float& den) {
    m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, z[(long)c * N]);
    den = 0.f;
    for (int c = 0; c < C; ++c) den = __fadd_rn(den, exp_fixed(__fsub_rn(z[(long)c * N], m)));
}

__global__ __launch_bounds__(LV_THREADS) void lv_keys(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                       int B, int C, int N, uint64_t* __restrict__ keys) {
    const long M = (long)B * N;
    const long e = (long)blockIdx.x * LV_THREADS + threadIdx.x;
    if (e >= M) return;
    const long b = e / N;
    const long i = e - b * N;
    const float* z = logits + (b * C) * (long)N + i;
    const int64_t l = labels[e];
    const bool lin = l >= 0 && l < C;
    float m, den;
    lv_softmax_head(z, N, C, m, den);
    for (int c = 0; c < C; ++c) {
        const float p = __fdiv_rn(exp_fixed(__fsub_rn(z[(long)c * N], m)), den);
        const bool fg = lin && l == c;
        const float err = fabsf(__fsub_rn(fg ? 1.f : 0.f, p));
        keys[(long)c * M + e] = (fg ? LV_FG : 0ull) | ((uint64_t)(lin ? c : C) << 32) | (uint64_t)(~__float_as_uint(err));
    }
}

// one wavefront per chunk
__global__ __launch_bounds__(64) void lv_count(const uint64_t* __restrict__ keys, long T, long chunk,
                                                uint32_t* __restrict__ cnt) {
    const int lane = threadIdx.x;
    const long i0 = (long)blockIdx.x * chunk;
    const long i1 = min(T, i0 + chunk);
    uint32_t n = 0;
    for (long t0 = i0; t0 < i1; t0 += 64) {
        const long j = t0 + lane;
        n += (uint32_t)__popcll(__ballot(j < i1 && (keys[j] & LV_FG) != 0ull));
    }
    if (lane == 0) cnt[blockIdx.x] = n;
}

// one workgroup.  totals: the totals record of the masked cross entropy's forward; its label counts are G_c
__global__ __launch_bounds__(GR_THREADS) void lv_prefix(const double* __restrict__ totals, const float* __restrict__ cwt, int C,
                                                         uint32_t* __restrict__ cnt, int chunks, LvState* __restrict__ st) {
    if (threadIdx.x == 0) {
        int64_t run = 0;
        double W = 0.0;
        for (int c = 0; c < C; ++c) {
            const int64_t G = (int64_t)totals[3 * C + c];
            st->gpre[c] = run;
            run += G;
            if (G > 0) W += cwt ? (double)cwt[c] : 1.0;
        }
        st->gpre[C] = run;
        st->P = run;
        st->W = W;
    }
    block_exclusive_scan(cnt, chunks);
}

// one wavefront per chunk
__global__ __launch_bounds__(64) void lv_coef(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx, long T,
                                               long chunk, const uint32_t* __restrict__ cnt, const LvState* __restrict__ st,
                                               const float* __restrict__ cwt, int C, float* __restrict__ coef,
                                               double* __restrict__ part) {
    const int lane = threadIdx.x;
    const unsigned long long upto = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull;
    const long P = st->P;
    const long i0 = (long)blockIdx.x * chunk;
    const long i1 = min(T, i0 + chunk);
    long run = cnt[blockIdx.x];              // foreground keys before this chunk
    double acc = 0.0;
    for (long t0 = i0; t0 < i1; t0 += 64) {
        const long j = t0 + lane;
        const bool live = j < i1;
        const uint64_t key = live ? keys[j] : 0ull;
        const bool fgb = live && (key & LV_FG) != 0ull;
        const unsigned long long bal = __ballot(fgb);
        if (live) {
            float cf = 0.f;
            const int c = (int)((uint32_t)(key >> 32) & LV_CLASS_MASK);
            if (c < C) {                      // a (class, labelled point) pair; class C is the unlabelled tail
                const long G = st->gpre[c + 1] - st->gpre[c];
                const long r = j - (long)c * P + 1;
                if (G > 0 && r >= 1 && r <= P) {
                    const long cum = run + __popcll(bal & upto) - st->gpre[c];
                    const long cum0 = cum - (fgb ? 1 : 0);
                    const double Jr = 1.0 - (double)(G - cum) / (double)(G + r - cum);
                    const double Jp = r > 1 ? 1.0 - (double)(G - cum0) / (double)(G + (r - 1) - cum0) : 0.0;
                    const double g = Jr - Jp;
                    cf = (float)g;
                    const float err = __uint_as_float(~(uint32_t)key);
                    acc += ((double)err * g) * (cwt ? (double)cwt[c] : 1.0);
                }
            }
            const uint32_t src = idx[j];
            if ((long)src < T) coef[src] = cf;      // (always: the payload is the key's initial position)
        }
        run += __popcll(bal);
    }
    acc = rl_wave_sum(acc);
    if (lane == 0) part[blockIdx.x] = acc;
}

// one workgroup: the chunk sums in index order (a thread owns consecutive chunks, thread 0 adds the threads in order)
__global__ __launch_bounds__(GR_THREADS) void lv_finalize(const double* __restrict__ part, int chunks,
                                                           const LvState* __restrict__ st, int with_ce,
                                                           double* __restrict__ out) {
    __shared__ double red[GR_THREADS];
    const int t = threadIdx.x;
    const int per = (chunks + GR_THREADS - 1) / GR_THREADS;
    const int j0 = min(chunks, t * per), j1 = min(chunks, j0 + per);
    double s = 0.0;
    for (int j = j0; j < j1; ++j) s += part[j];
    red[t] = s;
    __syncthreads();
    if (t == 0) {
        double tot = 0.0;
        for (int k = 0; k < GR_THREADS; ++k) tot += red[k];
        const double W = st->W;
        const double loss = W > 0.0 ? tot / W : 0.0;
        out[0] = with_ce ? out[0] + loss : loss;     // (out[0] holds the cross entropy of the launch before)
    }
}

__global__ __launch_bounds__(LV_THREADS) void lv_bwd(const float* __restrict__ logits, const int64_t* __restrict__ labels, int B,
                                                      int C, int N, const float* __restrict__ coef,
                                                      const LvState* __restrict__ st, const float* __restrict__ cwt,
                                                      float grad_scale, int accumulate, float* __restrict__ dlogits) {
    __shared__ float sc[RL_MAX_CLASSES];     // w_c / W of the present classes, 0 otherwise
    for (int c = threadIdx.x; c < C; c += LV_THREADS) {
        const double W = st->W;
        const long G = st->gpre[c + 1] - st->gpre[c];
        sc[c] = (W > 0.0 && G > 0) ? (float)((cwt ? (double)cwt[c] : 1.0) / W) : 0.f;
    }
    __syncthreads();
    const long M = (long)B * N;
    for (long e = (long)blockIdx.x * LV_THREADS + threadIdx.x; e < M; e += (long)gridDim.x * LV_THREADS) {
        const long b = e / N;
        const long i = e - b * N;
        const float* z = logits + (b * C) * (long)N + i;
        float* dz = dlogits + (b * C) * (long)N + i;
        const int64_t l = labels[e];
        if (!(l >= 0 && l < C)) {           // unlabelled: exact zeros, written (the cross entropy's gradient is 0 there too)
            for (int c = 0; c < C; ++c) dz[(long)c * N] = 0.f;
            continue;
        }
        float m, den;
        lv_softmax_head(z, N, C, m, den);
        float dot = 0.f;
        for (int c = 0; c < C; ++c) {
            const float p = __fdiv_rn(exp_fixed(__fsub_rn(z[(long)c * N], m)), den);
            const float fg = l == c ? 1.f : 0.f;
            const float sg = p > fg ? 1.f : (p < fg ? -1.f : 0.f);
            dot += (sg * coef[(long)c * M + e] * sc[c]) * p;
        }
        for (int c = 0; c < C; ++c) {
            const float p = __fdiv_rn(exp_fixed(__fsub_rn(z[(long)c * N], m)), den);
            const float fg = l == c ? 1.f : 0.f;
            const float sg = p > fg ? 1.f : (p < fg ? -1.f : 0.f);
            const float v = p * (sg * coef[(long)c * M + e] * sc[c] - dot) * grad_scale;
            dz[(long)c * N] = accumulate ? dz[(long)c * N] + v : v;
        }
    }
}

int lv_check(const char* who, const void* logits, const void* labels, int B, int C, int N, const void* ws, int64_t ws_bytes) {
    RL_REQUIRE(B > 0 && N > 0 && C > 0, RL_ERR_ARGS, "%s: bad sizes B=%d C=%d N=%d", who, B, C, N);
    RL_REQUIRE(C <= RL_MAX_CLASSES, RL_ERR_UNSUPPORTED, "%s: C=%d exceeds %d classes", who, C, RL_MAX_CLASSES);
    RL_REQUIRE((int64_t)B * N * C < (1ll << 31), RL_ERR_UNSUPPORTED, "%s: B*N*C=%lld keys, the sort takes fewer than 2^31", who,
               (long long)((int64_t)B * N * C));
    RL_REQUIRE(logits && labels, RL_ERR_ARGS, "%s: null pointer", who);
    return rl_ws_check(who, ws, ws_bytes, rl_lovasz_workspace_bytes(B, C, N));
}

}  // namespace

extern "C" int64_t rl_lovasz_workspace_bytes(int B, int C, int N) {
    if (!lv_supported(B, C, N)) return -1;
    return (int64_t)lv_layout(B, C, N).bytes;
}

extern "C" int64_t rl_lovasz_coef_offset(int B, int C, int N) {
    if (!lv_supported(B, C, N)) return -1;
    return (int64_t)lv_layout(B, C, N).off_coef;
}

extern "C" int rl_lovasz_forward(const float* logits, const int64_t* labels, int B, int C, int N, int with_ce,
                                 const float* class_weight, void* ws, int64_t ws_bytes, double* out, void* stream) {
    const char* who = "rl_lovasz_forward";
    int rc = lv_check(who, logits, labels, B, C, N, ws, ws_bytes);
    if (rc) return rc;
    RL_REQUIRE(out, RL_ERR_ARGS, "%s: null out", who);
    hipStream_t sm = (hipStream_t)stream;
    const LvLayout L = lv_layout(B, C, N);
    LvState* st = (LvState*)ws;
    double* lossw = rl_at<double>(ws, L.off_loss);
    const RadixBufs sort = radix_bufs(ws, L.sort);
    uint32_t* cnt = rl_at<uint32_t>(ws, L.off_cnt);
    double* part = rl_at<double>(ws, L.off_part);
    // the record's counts, the cross entropy in out[0], and G_c in the totals record
    rc = rl_loss_forward_masked(logits, labels, B, C, N, 0, 0.f, 0.f, 0, class_weight, 1, lossw, out, stream);
    if (rc) return rc;
    const int passes = grid_passes(lv_key_bits(C));
    hipLaunchKernelGGL(lv_keys, dim3(rl_cdiv(L.M, LV_THREADS)), dim3(LV_THREADS), 0, sm, logits, labels, B, C, N,
                       sort.keys[passes & 1]);
    RL_LAUNCH_CHECK("rl_lovasz_forward (keys)");
    rc = radix_sort(who, sort, L.T, passes, sm);
    if (rc) return rc;
    hipLaunchKernelGGL(lv_count, dim3(sort.chunks), dim3(64), 0, sm, sort.keys[0], L.T, sort.chunk, cnt);
    RL_LAUNCH_CHECK("rl_lovasz_forward (count)");
    hipLaunchKernelGGL(lv_prefix, dim3(1), dim3(GR_THREADS), 0, sm, lossw + rl_loss_totals_offset(C), class_weight, C, cnt,
                       sort.chunks, st);
    RL_LAUNCH_CHECK("rl_lovasz_forward (prefix)");
    hipLaunchKernelGGL(lv_coef, dim3(sort.chunks), dim3(64), 0, sm, sort.keys[0], sort.idx[0], L.T, sort.chunk, cnt, st,
                       class_weight, C, rl_at<float>(ws, L.off_coef), part);
    RL_LAUNCH_CHECK("rl_lovasz_forward (coef)");
    hipLaunchKernelGGL(lv_finalize, dim3(1), dim3(GR_THREADS), 0, sm, part, sort.chunks, st, with_ce, out);
    rl_note_kernel("lv_coef");
    RL_LAUNCH_CHECK("rl_lovasz_forward (finalize)");
    return RL_OK;
}

extern "C" int rl_lovasz_backward(const float* logits, const int64_t* labels, int B, int C, int N, int with_ce,
                                  const float* class_weight, const void* ws, int64_t ws_bytes, float grad_scale,
                                  float* dlogits, void* stream) {
    const char* who = "rl_lovasz_backward";
    int rc = lv_check(who, logits, labels, B, C, N, ws, ws_bytes);
    if (rc) return rc;
    RL_REQUIRE(dlogits, RL_ERR_ARGS, "%s: null dlogits", who);
    const LvLayout L = lv_layout(B, C, N);
    if (with_ce) {
        rc = rl_loss_backward_masked(logits, labels, B, C, N, 0, 0.f, 0.f, 0, rl_at<const double>(ws, L.off_loss), grad_scale,
                                     class_weight, 1, dlogits, stream);
        if (rc) return rc;
    }
    long g = (L.M + LV_THREADS - 1) / LV_THREADS;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(lv_bwd, dim3((int)g), dim3(LV_THREADS), 0, (hipStream_t)stream, logits, labels, B, C, N,
                       rl_at<const float>(ws, L.off_coef), (const LvState*)ws, class_weight, grad_scale, with_ce ? 1 : 0,
                       dlogits);
    rl_note_kernel("lv_bwd");
    RL_LAUNCH_CHECK("rl_lovasz_backward");
    return RL_OK;
}
