/*
 * rl_randlanet.h - C ABI of librandla_hip.so: the MI355X (gfx950) kernels of the RandLA-Net
 * segmentation hot path, a drop-in for the compiled / ATen pieces of
 * matthiasverstraete/3d_recognizer's `randlanet` package.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; every pointer is a DEVICE pointer owned by the
 *     caller unless said otherwise; nothing is allocated, freed or synchronised inside.
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous on it and is
 *     capturable into a hipGraph (no host synchronisation, no allocation).
 *   - return 0 on success, a negative RL_ERR_* otherwise; rl_last_error() gives the text.
 *     Nothing throws across the boundary.
 *   - activations are POINT-MAJOR / CHANNEL-LAST fp32: a (B, n, C) tensor is B*n rows of C
 *     floats.  A "batch-strided" operand addresses row (b, i) at base + (b*bstride + i)*ld,
 *     which lets a kernel read the first n rows of every cloud of a larger (B, n_parent, C)
 *     tensor - the reference's "random sampling" prefix slice (modules.py:587-589).
 *   - a "lazy" operand is a raw pre-BatchNorm tensor plus per-channel scale/shift and an
 *     activation: value = act(raw*scale[c] + shift[c]).  Consumers apply it while loading, so
 *     BatchNorm+activation never costs a pass over memory (SharedMLP.forward, modules.py:93-104).
 *
 * Reference interfaces replaced (paths relative to the reference repository):
 *   rl_knn_f32            knn_tpk.knn(support, querry, k)   randlanet/utils/src/bindings.cpp:5-7,
 *                         knn.cpp:43-61; also knn_naive / knn_approximate, utils/knn.py:7-117
 *   rl_gemm / rl_wgrad    SharedMLP conv / conv-transpose 1x1 (modules.py:82-84,99), fc_start
 *                         Linear (modules.py:494), AttentivePooling score Linear (modules.py:235),
 *                         with RelativePositionEncoding (modules.py:173-186) as an A-operand source
 *   rl_bn_*               BatchNorm2d(eps 1e-6, momentum 0.99) (modules.py:85-89, 496-499)
 *   rl_copy_rows / rl_scatter_add_rows
 *                         PointFeatureAugmentation gather+concat (modules.py:213-221), permutation /
 *                         prefix slicing (modules.py:571-573, 608), nearest-neighbour interpolation
 *                         gather + skip concat (modules.py:359-364, 600-602) and their backward
 *   rl_csr_build / rl_segment_sum_rows
 *                         the backward of those gathers (torch's scatter_add_) in a fixed summation order
 *   rl_pool_fwd/_bwd      PointFeatureAugmentation + AttentivePooling fused (modules.py:213-253)
 *   rl_attpool_*          AttentivePooling softmax over K + weighted sum (modules.py:246-253)
 *   rl_add_act_*          LocalFeatureAggregation residual + LeakyReLU (modules.py:325)
 *   rl_resid_bn_bwd_*     its backward fused with the two BatchNorm backwards behind it
 *   rl_rpe_build          RelativePositionEncoding (modules.py:173-186), materialised
 *   rl_scale_mask         Dropout of fc_end (modules.py:528)
 *   rl_batch_assemble     PointCloudPreprocessor.preprocess + augmentation + collation (dataset.py:61-131)
 *   rl_upsample_cf        UpSampler nni / nna / idw / isdw (modules.py:343-456)
 *   rl_logits_*           un-permute + (B,C,N) layout of the logits (modules.py:608-611)
 *   rl_loss_*             FocalTverskyLoss / FocalLoss / cross entropy (utils/losses.py:17-87,
 *                         trainer.py:244-269) and accuracy / iou (utils/metrics.py:8-59)
 *   rl_adam_step          torch.optim.Adam step of Trainer.train (utils/trainer.py:78,119)
 *   rl_scene_*            no counterpart: voted-crop scene inference (RandLA-Net's test protocol, Model.predict_scene)
 *   rl_scenes_*           no counterpart: training crops over many scenes (RandLA-Net's training sampler, Model.train_scenes)
 *   rl_scenes_vote_*      no counterpart: voted crops over many scenes at once (Model.predict_scenes)
 *   rl_grid_*             no counterpart: grid subsampling of a raw scene (the authors' grid_subsampling; utils/grid.py)
 *   rl_scene_confusion    no counterpart: the confusion matrix of a voted scene over its raw points (Model.evaluate_scenes)
 *   rl_cluster_*          no counterpart: Euclidean clustering of labelled points into instances (utils/cluster.py)
 *   rl_keypoints_*        no counterpart: confidence peaks of labelled, scored points (utils/keypoints.py)
 *   rl_scene_labels       no counterpart: label and confidence of every voted point (Model.predict_instances)
 *   rl_normals            no counterpart: normals and curvature of a bare cloud as input features (utils/normals.py)
 *   rl_pairs_*            no counterpart: pair counts of two id arrays, the table behind instance AP (utils/instance_metrics.py)
 *   rl_boxes_*            no counterpart: oriented boxes of the point sets that integer ids name (utils/boxes.py)
 *   rl_lovasz_*           no counterpart: the Lovasz-Softmax loss, alone or summed with cross entropy (utils/lovasz.py)
 *   rl_outliers_*         no counterpart: statistical outlier removal of a scan before anything looks at it (utils/outliers.py)
 *   rl_depth_*            temporal filter, deprojection and range filter of a depth frame (camera/realsense_camera.py:90-125;
 *                         utils/depth.py)
 *   rl_planes_*           no counterpart: RANSAC plane segmentation, the desk or the ground taken out of a scan (utils/planes.py)
 *   rl_icp_*              no counterpart: rigid registration of overlapping scans by iterative closest point
 *   rl_fpfh_*, rl_match_* no counterpart: FPFH descriptors of a cloud and their brute-force matching
 *   rl_global_*           no counterpart: RANSAC over feature correspondences, the initial pose of rl_icp_*
 *                         (utils/registration.py)
 *   rl_tsdf_*             no counterpart: TSDF fusion of a stream of depth frames and its surface as points (utils/tsdf.py)
 */
#ifndef RL_RANDLANET_H
#define RL_RANDLANET_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* (the plan queries rl_gemm_plan and rl_wgrad_plan2 are appended under the same rule)
 * (round 9 appends rl_gemm_desc.a2_first, rl_wgrad_desc.a2_first and rl_set / rl_get_decoder_cat under the same rule)
 * (round 8 appends rl_gemm_desc.a2_*, rl_gemm_concat_supported, rl_attpool_src with rl_attpool_cat_supported / _fwd_cat / _bwd_cat and rl_set / rl_get_pool256_x
 * under the same rule as round 7)
 * (round 7 appends rl_wgrad_desc.a2_*, rl_pool_desc.x_optional, rl_wgrad_plan and rl_set / rl_get_pool128_x: zero-filled new
 * fields mean what the library did before and no existing field moves, so the number - which callers pin - stays 110) */
#define RL_VERSION 110     /* round 6: rl_gemm_stat_slots (64-row tiles of the wide GEMM), rl_bn_finalize pivot vector; round 5: shifted BatchNorm statistics (stats_pivot_* fields, rl_bn_finalize pivoted), rl_head_*; round 4: rl_launch_count */

#define RL_OK 0
#define RL_ERR_ARGS (-1)         /* bad shape / null pointer / unsupported size            */
#define RL_ERR_FEW_SUPPORT (-2)  /* knn: support has fewer than k points (knn.cpp:15-17)   */
#define RL_ERR_LAUNCH (-3)       /* hip launch error                                        */
#define RL_ERR_UNSUPPORTED (-4)  /* valid in the reference, not implemented by this build   */

#define RL_MAX_SLOTS 1024        /* partial-statistics slots written by row-streaming kernels */
#define RL_KNN_MAX_K 64
#define RL_MAX_CLASSES 256       /* classes every rl_loss_* entry takes (training and the on-device evaluation); inference has no such bound */

const char* rl_last_error(void);
/* name of the main kernel function the last entry point dispatched to on this thread (profiling aid:
 * matches the kernel names of a rocprofv3 trace) */
const char* rl_last_kernel(void);
int rl_version(void);
/* kernel launches issued by this library in the calling process so far (every entry point counts the kernels it launches;
 * a measurement aid: the difference around an eager step = the kernels a rocprofv3 trace shows for it) */
int64_t rl_launch_count(void);
/* measurement aid: one idle wavefront that occupies `stream` for `us` microseconds (<= 20000) - stands in for a collective of
 * known length when a schedule around it is timed on a single GPU (tools/allreduce_standin.py); touches no memory */
int rl_spin_us(int us, void* stream);

/* Number of partial-statistics slots a row-streaming kernel writes for `rows` rows:
 * rl_gemm uses rows_per_tile = 128, rl_loss 256; rl_bn_bwd_reduce has its own rl_bn_bwd_slots. */
int rl_row_blocks(int64_t rows, int rows_per_tile);

/* ------------------------------------------------------------------------------------------
 * Exact K nearest neighbours.  d2 = ((dx*dx)+(dy*dy))+(dz*dz) in IEEE fp32 without FMA
 * (nanoflann.hpp:488-497), rows ascending by (d2, index).  support (B,Ns,3), query (B,Nq,3)
 * contiguous fp32; idx_out (B,Nq,k) int64, d2_out (B,Nq,k) fp32.  k <= RL_KNN_MAX_K.
 * Replaces knn_tpk.knn (bindings.cpp:5-7).
 * workspace: device scratch of rl_knn_workspace_bytes(B,Ns,Nq,k) bytes, 256-byte aligned; with it
 * supports of >= 512 points are searched through a uniform grid (same answer, ~100x fewer
 * distance evaluations); NULL selects the tiled brute-force scan.                           */
int64_t rl_knn_workspace_bytes(int B, int Ns, int Nq, int k);
int rl_knn_f32(const float* support, const float* query, int B, int Ns, int Nq, int k,
               int64_t* idx_out, float* d2_out, void* workspace, int64_t workspace_bytes,
               void* stream);

/* Host twin: the same search on the calling host, HOST pointers, no GPU involved, synchronous (queries are split over
 * the hardware threads).  Same contract and error codes; backs the package's CPU device (reference model.py:38-40
 * falls back to the CPU when there is no GPU: config P, predict.py on a GPU-less box).                         */
int rl_knn_f32_cpu(const float* support, const float* query, int B, int Ns, int Nq, int k,
                   int64_t* idx_out, float* d2_out);

/* Same search with int32 indices and batch strides (in points), used inside the network:
 * cloud b of the support starts at support + b*support_bstride*3.                          */
int rl_knn_i32(const float* support, int64_t support_bstride, const float* query,
               int64_t query_bstride, int B, int Ns, int Nq, int k, int32_t* idx_out,
               float* d2_out, void* workspace, int64_t workspace_bytes, void* stream);

/* Several searches over the same B clouds in one launch set (a forward pass needs eight that depend
 * only on the coordinates: encoder K-NN on every level, decoder 1-NN between levels).  Each task is
 * one rl_knn_i32 call; the small ones run beside the large one instead of after it.  At most 8 tasks. */
typedef struct rl_knn_task {
    const float* support;
    int64_t support_bstride;
    const float* query;
    int64_t query_bstride;
    int32_t Ns, Nq, k;
    int32_t* idx_out;
    float* d2_out;
} rl_knn_task;

int64_t rl_knn_multi_workspace_bytes(const rl_knn_task* tasks, int ntasks, int B);
int rl_knn_multi(const rl_knn_task* tasks, int ntasks, int B, void* workspace, int64_t workspace_bytes,
                 void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-point linear layer (1x1 conv / conv-transpose / Linear):   Y = A' . W (+ bias)
 *   A' [M x K] : A-operand, M = B*n rows.
 *       a_mode 0: row (b,i) = A + (b*a_bstride + i)*lda, lazily transformed by in_* if
 *                 in_scale != NULL.
 *       a_mode 1: relative position encoding rows built on the fly (modules.py:173-186):
 *                 M = B*n*nbr_k, row (b,i,j) = [xyz_i, xyz_nb, xyz_i - xyz_nb, sqrt(d2)],
 *                 K must be 10; xyz cloud b starts at xyz + b*xyz_bstride*3; nbr_idx/nbr_d2 are
 *                 (B,n,nbr_k) contiguous.
 *   W element (k, c) = W[k*w_ks + c*w_ns]   (Conv2d/Linear weight (N,K): w_ks=1, w_ns=K;
 *                                           ConvTranspose2d weight (K,N): w_ks=N, w_ns=1)
 *   Y row (b,i) = Y + (b*y_bstride + i)*ldy ; accumulate != 0 adds into Y.
 *   stats != NULL: per-block column sums of Y and Y*Y are written as doubles to
 *       stats[slot][0][c], stats[slot][1][c] for slot < rl_gemm_stat_slots(M,N,K) (BatchNorm batch
 *       statistics, finished by rl_bn_finalize with that slot count).                        */
typedef struct rl_gemm_desc {
    const float* A;
    int64_t lda, a_bstride;
    int32_t a_mode;
    int32_t in_act;
    float in_slope;
    const float* in_scale;
    const float* in_shift;
    const float* xyz;
    int64_t xyz_bstride;
    const int32_t* nbr_idx;
    const float* nbr_d2;
    int32_t nbr_k;
    int32_t B, n, N, K;
    const float* W;
    int64_t w_ks, w_ns;
    const float* bias;
    float* Y;
    int64_t ldy, y_bstride;
    int32_t accumulate;
    double* stats;
    /* optional scratch of rl_gemm_kslab_floats(M,N,K) floats: lets a wide layer with few rows split K
     * over workgroups (deterministic two-pass reduction); NULL or too small = single pass */
    float* kslab;
    int64_t kslab_floats;
    /* optional "split-scatter" epilogue (the dX of PointFeatureAugmentation's concat, modules.py:213-221):
     *   addend  != NULL : v += addend[R*N + c] before anything else (row stride N, row R = global row)
     *   out2    != NULL : columns c >= split_col are not stored to Y.  With out2_index == NULL they are stored to
     *                     out2[R*(N - split_col) + c - split_col] (a dense (M, N - split_col) tensor: the gradient of
     *                     every gathered row, summed per destination afterwards by rl_segment_sum_rows in a fixed
     *                     order - the deterministic path the network uses).  With out2_index they are atomically
     *                     added to out2[(b*out2_bstride + out2_index[R])*(N - split_col) + c - split_col], b = R / rows
     *                     per cloud (order-dependent in the last bits; out2 zeroed by the caller).
     *                     Columns c < split_col go to Y as usual (ldy, y_bstride, accumulate apply to them only).
     * Needs the LDS-tiled kernel (K or N > 64, 16-byte aligned operands) and no statistics; else RL_ERR_UNSUPPORTED.
     * (round 9) K, N <= 64: the streaming kernel stores a DENSE split - out2 alone (no addend, no out2_index), split_col % 16 == 0,
     * plain fp32 rows in 16-byte pieces: a 16-column tile goes to Y (which may accumulate) or to out2 (plain stores). */
    const float* addend;
    float* out2;
    const int32_t* out2_index;
    int64_t out2_bstride;
    int32_t split_col;
    /* optional, wide layers in the bf16 arithmetic modes: the weight already split into bf16 head / tail planes in the
     * orientation THIS product reads it - plane[n*K + k] = W(k, n), tails N*K elements after the heads (rl_split_weights;
     * 16-byte aligned, K % 8 == 0).  Selects the 8-wavefront kernel: no conversion of the weight per tile, four
     * wavefronts per SIMD instead of two.  Same arithmetic, same results as without it. */
    const void* W_split;
    /* optional, with stats: SHIFTED statistics.  The partial sums are those of (y - pivot) and (y - pivot)^2 with
     * pivot[c] = stats_pivot_mean[c] - (stats_pivot_bias ? stats_pivot_bias[c] : 0) - the layer's running mean (what torch's
     * BatchNorm2d keeps, modules.py:85-89), minus the conv bias this product leaves out (rl_bn_finalize folded_bias) -
     * subtracted per element BEFORE squaring, so that a channel whose spread is a few 1e-4 of its mean keeps its variance
     * (the reference's ATen BatchNorm is two-pass; E[y^2] - E[y]^2 on fp32 partial sums is not).  rl_bn_finalize must then be
     * told `pivoted`.  NULL = plain sums (pivot 0). */
    const float* stats_pivot_mean;
    const float* stats_pivot_bias;
    /* optional (round 6), streaming kernel only (K, N <= 64: rl_gemm_streams(d) == 1): this product is the gradient G w.r.t. the
     * ACTIVATED output of a BatchNorm layer - the input gradient of the layer behind it - and `stats` receives, instead of the
     * forward sums, what rl_bn_bwd_reduce would leave for that layer: sum g' and sum g' xhat per column, g' = G act'(Yl scale +
     * shift), xhat = (Yl - mean) invstd, with Yl = bnb_Y the layer's raw output (same rows and row layout as Y), bnb_scale /
     * bnb_shift its folded BatchNorm, bnb_mean / bnb_invstd its saved batch statistics, bnb_act / bnb_slope its activation.
     * rl_gemm_stat_slots(M, N, K) slots; then rl_bn_bwd_finalize + rl_bn_bwd_apply - no reduce sweep over G and Yl.
     * Y must be complete after this call (the only or the last accumulating writer).  No pivot. */
    const float* bnb_Y;
    const float* bnb_scale;
    const float* bnb_shift;
    const float* bnb_mean;
    const float* bnb_invstd;
    int32_t bnb_act;
    float bnb_slope;
    /* "Concat-gather" A operand (round 8; a2_split > 0), the fields and the meaning of rl_wgrad_desc.a2_*: A' is the concatenation
     * of two sources that is never stored -
     *   k-columns [0, a2_split)  : source 1 = A, lda, a_bstride with the fold in_scale / in_shift / in_act / in_slope;
     *   k-columns [a2_split, K)  : source 2, row (b, a2_idx[R]) at A2 + (b*a2_bstride + a2_idx[R])*lda2 for the row R of cloud b
     *                              (one int32 per row of A', trusted to lie inside the cloud), with its own fold a2_scale /
     *                              a2_shift (both or neither) / a2_act / a2_slope.
     * Every value is act(v*scale + shift) as rl_copy_rows stores it (max(z, z*e): a clipped ReLU input is -0), so with A = U,
     * A2 = G, a2_idx = idx the product is bitwise that over the stored concatenation.  (A source WITHOUT a fold goes through the
     * same expression with scale 1, shift 0, where the stored copy keeps the raw value: a raw -0 enters as +0.  The operand then
     * differs from the stored one in the sign of that zero only and the product does not: an accumulator that starts at +0 is the
     * same after adding +0 or -0.)  The A loaders of the LDS-DMA wide kernel
     * fetch each 32-column chunk from the source it lies in; the 8 indices of an 8-row piece come over the scalar unit, a tile
     * ahead.  Supported where that kernel takes the product of the stored operand in one pass - bf16x3 / bf16 arithmetic with
     * W_split, "dma" staging, no K split - and K == 2*a2_split <= 1024, a2_split % 32 == 0, n % 16 == 0 (so that a piece lies in
     * one cloud and M % 16 == 0); anything else is RL_ERR_UNSUPPORTED and launches nothing (ask rl_gemm_concat_supported).
     * A2 16-byte aligned, lda2 % 4 == 0, lda >= a2_split, lda2 >= K - a2_split.  Zero-filled: an ordinary operand.
     * Measured (profiles/r08_pool256_x_in_place.md, 81920 x 256 x 256 on an MI355X): 57 us from the two sources against 52 us
     * from the stored concatenation, which costs a 27 us copy and 84 MB to build - the step gains 0.9 % with its other readers. */
    int32_t a2_split;
    int32_t a2_act;
    const float* A2;
    int64_t lda2, a2_bstride;
    const int32_t* a2_idx;
    const float* a2_scale;
    const float* a2_shift;
    float a2_slope;
    /* (round 9) != 0: the column order is [gathered | direct] - the decoder's [interpolated | skip]: source 2 (A2, a2_idx, its
     * fold) holds the k-columns [0, a2_split) and source 1 (A, its fold) the columns [a2_split, K); then lda >= K - a2_split and
     * lda2 >= a2_split.  0: the order above, the same bits as before the field existed.  The same conditions either way. */
    int32_t a2_first;
} rl_gemm_desc;

/* TWO products over one A' in ONE launch of the LDS-DMA wide GEMM (round 6): Y1 = A'.W1, Y2 = A'.W2 - mlp1 and shortcut of an
 * encoder level (modules.py:314, 325), which both read the level's input: the rows are fetched once and the narrow product's
 * few tiles ride along with the wide one's.  Both descriptors must name the same A' (pointer, strides, lazy transform; a_mode 0,
 * K % 32 == 0, K <= 1024) and carry W_split (bf16 arithmetic modes); neither product narrow enough for the exact-fp32 streaming
 * kernel (K <= 64 and N <= 64: its arithmetic would change); dense outputs (ldy == N, y_bstride == n);
 * statistics (with their pivots) for both or for none - each into its own buffer, rl_row_blocks(M, 128) slots; no bias, no
 * accumulate, no split epilogue.  Bitwise the results of two rl_gemm calls on 128 x 128 tiles.
 * rl_gemm_pair_supported: 1 if the pair can go out as one launch, else the caller issues two rl_gemm calls. */
int rl_gemm_streams(const rl_gemm_desc* d);
/* What rl_gemm's validation and plan answer for d under the process settings as they stand, without a launch: RL_OK,
 * RL_ERR_ARGS or RL_ERR_UNSUPPORTED.  The question a caller asks before it decides not to store a concatenation (a2_split > 0). */
int rl_gemm_concat_supported(const rl_gemm_desc* d);
/* What rl_gemm would launch for d, without launching it (the counterpart of rl_wgrad_plan): rl_gemm's return code (a refusal
 * included), and on RL_OK the grid (3 ints), the workgroup size, the output tile of the LDS-DMA wide kernel (bm, bn; 0, 0 on
 * every other kernel), the K ranges of the launch (1: no split), the column block of the split-K reducer (0: none, else 16
 * or 64), the kernel's name (the one rl_last_kernel reports) and its instantiation by name, e.g. "sgemm_kernel<2,4,bnb>",
 * "wgemm2_kernel<bf16x3,stats,64x128>".  Any output may be NULL. */
int rl_gemm_plan(const rl_gemm_desc* d, int32_t* grid_xyz, int32_t* threads, int32_t* tile_bm_bn, int32_t* ksplit,
                 int32_t* reduce_cols, const char** kernel, const char** variant);
int rl_gemm_pair_supported(const rl_gemm_desc* a, const rl_gemm_desc* b);
int rl_gemm_pair(const rl_gemm_desc* a, const rl_gemm_desc* b, void* stream);

/* Splits weights for rl_gemm_desc.W_split: out (2*N*K bf16) <- heads, then tails, of W(k, n) = W[k*w_ks + n*w_ns].
 * One launch for all items (every wide layer of a step, in both orientations: forward and dgrad). */
typedef struct rl_wsplit_item {
    const float* W;
    int64_t w_ks, w_ns;
    int32_t K, N;
    void* out;
} rl_wsplit_item;

int rl_split_weights(const rl_wsplit_item* items, int count, void* stream);

int64_t rl_gemm_kslab_floats(int64_t M, int N, int K);
/* slots of `stats` an (M, N, K) product fills (<= RL_MAX_SLOTS): those of rl_gemm's launch plan for an aligned, pre-split
 * product with statistics of that shape - one per 64-row block where that plan runs the wide GEMM on 64-row output tiles
 * (few rows), else one per 128-row block.  rl_gemm hands this count to whichever kernel its own plan launches, and every
 * kernel zero-fills the slots it does not use, so this is the count to hand to rl_bn_finalize.  The count depends on the
 * arithmetic mode (rl_set_wide_gemm), the rl_set_wgemm_* settings and the device: call it under the same ones as the rl_gemm /
 * rl_bn_finalize it sizes - a count that disagrees with the launch's grid gives wrong BatchNorm statistics. */
int64_t rl_gemm_stat_slots(int64_t M, int N, int K);

/* Arithmetic of the wide kernels (K or N > 64: rl_gemm's LDS-tiled kernel, rl_wgrad's 128x128 kernel):
 *   "bf16x3" (default)  every fp32 operand is split into a bf16 head and tail on its way into LDS and a product is
 *                       a_hi*w_hi + a_hi*w_lo + a_lo*w_hi on v_mfma_f32_16x16x32_bf16, fp32 accumulate: ~2^-16
 *                       relative product error; network logits within 2.5e-6 of the fp32 CPU forward
 *   "fp32"              v_mfma_f32_16x16x4_f32, bitwise an fp32 FMA chain
 *   "bf16"              heads only: plain bf16 operands, fp32 accumulate (does NOT meet the 1e-3 logits bound)
 * The environment variable RL_WIDE_GEMM sets the initial mode.  Storage, accumulation, statistics and the
 * narrow (streaming) kernels are fp32 in every mode.  Not thread-safe against concurrent launches.           */
int rl_set_wide_gemm(const char* mode);
const char* rl_get_wide_gemm(void);
/* How the wide forward / input-gradient GEMM of the bf16 modes stages its operands:
 *   "dma" (default)  wgemm2_kernel: one persistent 12-wavefront workgroup per CU; four loader wavefronts bring the raw fp32
 *                    rows and the pre-split weight planes into LDS rings by LDS-DMA (global_load_lds_dwordx4), four chunks
 *                    deep and across the workgroup's tiles; eight compute wavefronts convert on the fragment
 *   "registers"      wgemm_kernel: global loads converted on their way into LDS, one chunk ahead, two workgroups per CU
 * Same products in the same order: Y is bitwise the same (the BatchNorm partial sums are grouped differently).
 * K % 32 != 0 or K > 1024 always takes "registers".                                                                   */
int rl_set_wgemm_staging(const char* how);
/* Output tile of the "dma" kernel: "auto" (default) = 128 x 128, or 64 x 128 / 64 x 64 where 128 x 128 tiles would leave
 * at most half / a quarter of the CUs with a tile (the deep levels: few rows) - more workgroups in one pass, mostly no K split;
 * "128" = always 128 x 128 (round 5).  Y is bitwise the same; the BatchNorm partial sums are grouped per 64 rows
 * (rl_gemm_stat_slots).  "128" also keeps the narrow (16 < N <= 64) products off the "dma" kernel.                     */
int rl_set_wgemm_tile(const char* how);
/* Diagnostics: enable = 0 switches the K split of wide products with few output tiles off (one summation order whatever the
 * kernel and its tile: what the bitwise kernel-against-kernel tests compare on); 1 (default) restores it.               */
int rl_set_gemm_ksplit(int enable);
/* Diagnostics: the streaming GEMM (K, N <= 64) on 1/div of its workgroups (1 = default).  Y is bitwise the same; the rows a
 * lane adds into its BatchNorm partial sums change - the regression knob for "a re-grouping of the statistics must not move
 * a gradient" (tests/test_net_gpu.py; round 4 met 0.5 - 3 % before the sums were shifted).                              */
int rl_set_sgemm_grid_div(int div);
int rl_gemm(const rl_gemm_desc* d, void* stream);

/* Weight / bias gradient of the same layer:  dW(k,c) = sum_r A'[r][k] * dY[r][c],
 * db[c] = sum_r dY[r][c].  The A-operand fields have the meaning they have in rl_gemm_desc.
 * dY row (b,i) = dY + (b*dy_bstride + i)*lddy.  dW is written with the strides (w_ks, w_ns) of
 * the weight it belongs to.  Deterministic: per-block partial slabs in `slab` (at least
 * rl_wgrad_slab_floats() floats) are summed in a fixed order by a second kernel.            */
typedef struct rl_wgrad_desc {
    const float* A;
    int64_t lda, a_bstride;
    int32_t a_mode;
    int32_t in_act;
    float in_slope;
    const float* in_scale;
    const float* in_shift;
    const float* xyz;
    int64_t xyz_bstride;
    const int32_t* nbr_idx;
    const float* nbr_d2;
    int32_t nbr_k;
    int32_t B, n, N, K;
    const float* dY;
    int64_t lddy, dy_bstride;
    float* dW;
    int64_t w_ks, w_ns;
    float* dbias; /* nullable */
    float* slab;
    int64_t slab_floats;
    /* != 0: only the partial slabs are written; the caller sums them later with
     * rl_wgrad_reduce_batch (one launch for all layers of a backward pass), so `slab` must be
     * private to this layer until then */
    int32_t defer_reduce;
    /* bf16-storage mode: A and dY are bf16 rows (lda / lddy count elements).  Wide layers only (a 128 x 128 tile of dW,
     * i.e. N or K > 64), plain A operand, outside the fp32 arithmetic mode; the products are then exact bf16 x bf16. */
    int32_t rows_bf16;
    /* "Concat-gather" A operand (a2_split > 0): A' is the concatenation of two sources that is never stored -
     *   k-columns [0, a2_split)  : source 1 = A, lda, a_bstride with the fold in_scale / in_shift / in_act / in_slope;
     *   k-columns [a2_split, K)  : source 2, row (b, a2_idx[R]) at A2 + (b*a2_bstride + a2_idx[R])*lda2 for the row R of cloud b
     *                              (a2_idx holds one int32 per row of A', trusted to lie inside the cloud), with its own fold
     *                              a2_scale / a2_shift (both or neither) / a2_act / a2_slope.
     * Every value is act(v*scale + shift) exactly as rl_pool_bwd forms its X tile, so with A = U, A2 = G, a2_idx = idx the result
     * is bitwise that of the X_out it would have stored (rl_pool_desc.x_optional).  Supported: the wide (128 x 128 tile) kernel
     * in the bf16x3 / bf16 arithmetic modes, fp32 rows, K == 2*a2_split, a2_split % 16 == 0 - anything else is
     * RL_ERR_UNSUPPORTED and launches nothing.  A2 16-byte aligned, lda2 % 4 == 0, lda >= a2_split, lda2 >= K - a2_split. */
    int32_t a2_split;
    int32_t a2_act;
    const float* A2;
    int64_t lda2, a2_bstride;
    const int32_t* a2_idx;
    const float* a2_scale;
    const float* a2_shift;
    float a2_slope;
    /* (round 9) != 0: [gathered | direct] - source 2 holds the k-columns [0, a2_split), source 1 those from a2_split on; see
     * rl_gemm_desc.a2_first.  A grouped launch (rl_wgrad_batch) carries up to eight concat-gather layers, of either order. */
    int32_t a2_first;
} rl_wgrad_desc;

int64_t rl_wgrad_slab_floats(int64_t M, int N, int K);
int rl_wgrad(const rl_wgrad_desc* d, void* stream);
/* What rl_wgrad would launch for d, without launching it: the return code rl_wgrad's validation and plan give (RL_OK,
 * RL_ERR_ARGS, RL_ERR_UNSUPPORTED), and on RL_OK the grid (3 ints), the workgroup size and the kernel's name (the one
 * rl_last_kernel reports).  Any output may be NULL. */
int rl_wgrad_plan(const rl_wgrad_desc* d, int32_t* grid_xyz, int32_t* threads, const char** kernel);
/* The same answer and the rest of the plan: the number of partial slabs, the rows each workgroup row sums, the kind of grouped
 * launch the layer may join (rl_wgrad_batchable) and the kernel instantiation by name, e.g. "swgrad_kernel<2,4>",
 * "pwgrad128w_kernel<bf16x3>" (for tests that pin which instantiation a shape gets).  Any output may be NULL. */
int rl_wgrad_plan2(const rl_wgrad_desc* d, int32_t* grid_xyz, int32_t* threads, const char** kernel, int32_t* nsplit,
                   int64_t* rows_per_block, int32_t* batch, const char** variant);

/* Deferred second pass of rl_wgrad for `count` layers in one launch per 48 items: item i sums
 * the nsplit = slab_floats_used / (N*K + N) partial slabs of its layer in the same fixed order
 * as the per-layer reducer and writes dW (strides w_ks, w_ns) and dbias (nullable).
 * `items` is a HOST array (copied into the kernel arguments).                                 */
typedef struct rl_wgrad_reduce_item {
    const float* slab;
    float* dW;
    float* dbias;
    int64_t w_ks, w_ns;
    int32_t nsplit, N, K;
    int32_t reserved;
} rl_wgrad_reduce_item;

int rl_wgrad_nsplit(int64_t M, int N, int K);
/* Several layers' weight gradients in ONE launch: the layers of a backward pass are independent of each other and mostly
 * small (the wide ones 80 - 216 workgroups each on a chip that holds 512, the narrow ones 5 - 46 us each), so one by one
 * they leave most CUs idle and pay a launch each.  rl_wgrad_batchable: 0 = must go through rl_wgrad, 1 = joins the grouped
 * launch of the wide (128 x 128-tile) kernel (fp32 rows, bf16x3 / bf16 arithmetic), 2 = joins the grouped launch of the
 * narrow (streaming) kernel (K, N <= 64, fp32 rows, tensor operand).  rl_wgrad_batch takes a queue of either or both kinds
 * (one launch per kind and per 24 layers); every descriptor must have defer_reduce set; the partial slabs are exactly
 * those of rl_wgrad (same split, same per-workgroup arithmetic: bitwise equal results) and are summed by
 * rl_wgrad_reduce_batch as before.                                                                                    */
int rl_wgrad_batchable(const rl_wgrad_desc* d);
int rl_wgrad_batch(const rl_wgrad_desc* descs, int count, void* stream);
int rl_wgrad_reduce_batch(const rl_wgrad_reduce_item* items, int count, void* stream);

/* ------------------------------------------------------------------------------------------
 * BatchNorm2d(eps, momentum) folded into per-channel (scale, shift).
 * training != 0: mean/var from the `nslots` partial sums written by a producer over `count`
 *   rows; running stats updated as torch does (running = (1-m)*running + m*batch, unbiased
 *   variance; num_batches_tracked += 1 when nbt != NULL); saves mean and invstd for backward.
 * training == 0: scale/shift from the running statistics; stats may be NULL.
 * folded_bias (C floats or NULL): the bias of the layer in front (SharedMLP's conv bias, modules.py:93-104), when the
 *   producer left it OUT of the tensor - it cancels in (y - mean), so the GEMM epilogue need not add it.  The statistics
 *   and the saved mean are then those of (y - bias), (scale, shift) apply to that tensor, and the running mean is kept
 *   as the reference keeps it: that of y (mean + bias); in eval mode the running mean is read as (running_mean - bias).
 * pivoted != 0 (training): the partial sums are SHIFTED - those of (t - p) and (t - p)^2 of the stored tensor t,
 *   p[c] = m[c] - folded_bias[c] with m = `pivot` when given, else running_mean (either as it stands BEFORE this call's
 *   update): mean = p + S/n, var = Q/n - (S/n)^2.  The producer must have been given the same two vectors
 *   (rl_gemm_desc.stats_pivot_*, rl_pool_desc.pivot_mean*).
 * pivot (C floats or NULL; training): the caller's pivot vector of this layer (round 6).  After the fold it holds THIS
 *   batch's mean of y (mean + folded bias) - the next step's pivot: always within the batch-to-batch drift of the mean,
 *   wherever a loaded checkpoint's running mean sits (a pivot ten standard deviations off costs the variance two digits);
 *   zero it for a fresh / freshly loaded model (pivot 0 = plain sums for one step). */
int rl_bn_finalize(const double* stats, int nslots, int64_t count, int C, const float* gamma,
                   const float* beta, float* running_mean, float* running_var, int64_t* nbt,
                   float momentum, float eps, int training, float* scale, float* shift,
                   float* save_mean, float* save_invstd, const float* folded_bias, int pivoted, float* pivot, void* stream);

/* Several independent layers' folds in one launch (same arithmetic per layer as rl_bn_finalize: same results).  The folds of
 * the layers at one dependency depth of an encoder level - mlp1 / shortcut / mlp_rpe1, then pool1.mlp / mlp_rpe2 - are wanted
 * at the same moment, and a fold is a launch that costs ten times its work.                                              */
typedef struct rl_bn_finalize_item {
    const double* stats;
    int64_t count;
    const float* gamma;
    const float* beta;
    float* running_mean;
    float* running_var;
    int64_t* num_batches_tracked;
    float* scale;
    float* shift;
    float* save_mean;
    float* save_invstd;
    const float* folded_bias;
    int32_t nslots, C, training;
    float momentum, eps;
    int32_t pivoted;
    float* pivot;
} rl_bn_finalize_item;
int rl_bn_finalize_batch(const rl_bn_finalize_item* items, int count, void* stream);

/* BatchNorm + activation backward for a lazy tensor Y (rows x C, row (b,i) at (b*bstride+i)*ld)
 * whose activated value received gradient G (same addressing):
 *   g = G * act'(Y*scale+shift);  xhat = (Y-mean)*invstd
 *   rl_bn_bwd_reduce : partial sums of g and g*xhat -> stats[slot][0|1][c], slot < rl_bn_bwd_slots(M)
 *   rl_bn_bwd_finalize: dgamma = sum g*xhat, dbeta = sum g, coef[0][c] = mean g, coef[1][c] = mean g*xhat
 *   rl_bn_bwd_apply  : G <- scale * (g - coef0 - xhat*coef1)      (training)
 *                      G <- scale * g                              (coef == NULL: eval / no BN)  */
typedef struct rl_bn_bwd_desc {
    float* G;
    const float* Y;
    int64_t ld, bstride;
    int32_t B, n, C;
    int32_t act;
    float slope;
    const float* scale;
    const float* shift;
    const float* mean;
    const float* invstd;
    double* stats;      /* reduce: out */
    const float* coef;  /* apply: in, 2*C floats, or NULL */
} rl_bn_bwd_desc;

/* (nslots, 2, C) per-workgroup partials -> (2, C) totals in slot order.  SyncBN / equivalence mode: the caller
 * all-reduces the totals over the ranks and passes them on as ONE slot with the global row count
 * (rl_bn_finalize / rl_bn_bwd_finalize with nslots = 1).                                             */
int rl_bn_reduce_slots(const double* stats, int nslots, int C, double* out, void* stream);
int rl_bn_bwd_slots(int64_t rows);
int rl_bn_bwd_reduce(const rl_bn_bwd_desc* d, void* stream);
int rl_bn_bwd_finalize(const double* stats, int nslots, int64_t count, int C, float* dgamma,
                       float* dbeta, float* coef, void* stream);
/* rl_bn_bwd_finalize for the two BatchNorms behind a residual junction (same row and channel counts) in one launch. */
int rl_bn_bwd_finalize_pair(const double* stats0, const double* stats1, int nslots, int64_t count, int C, float* dgamma0,
                            float* dbeta0, float* coef0, float* dgamma1, float* dbeta1, float* coef1, void* stream);
/* rl_bn_bwd_finalize for up to 8 unrelated layers in one launch (round 6): e.g. a virtual rpe stage (sums left by its pooling
 * kernel) together with the per-point layer whose reduce sweep ran right behind it.  Same arithmetic per layer. */
typedef struct rl_bn_bwd_finalize_item {
    const double* stats;
    int64_t count;
    float* dgamma;
    float* dbeta;
    float* coef;
    int32_t nslots, C;
} rl_bn_bwd_finalize_item;
int rl_bn_bwd_finalize_batch(const rl_bn_bwd_finalize_item* items, int count, void* stream);
int rl_bn_bwd_apply(const rl_bn_bwd_desc* d, void* stream);
/* The three steps in ONE launch for a small tensor (rows <= 2048, C % 4 == 0, ld % 4 == 0, 16-byte aligned; ask
 * rl_bn_bwd_fused_supported): a workgroup owns a channel quad and all its rows, so the batch sums never leave it.  G becomes
 * the gradient w.r.t. Y in place, dgamma / dbeta (and, when coef_out != NULL, the 2*C means rl_bn_bwd_finalize would
 * leave) are written.  Same expressions per element; the sums are grouped per wavefront (another fixed order).
 * Replaces the same reference lines as the three (BatchNorm2d backward of modules.py:85-89).                          */
int rl_bn_bwd_fused_supported(int64_t rows, int C, int64_t ld);
int rl_bn_bwd_fused(const rl_bn_bwd_desc* d, int64_t count, float* dgamma, float* dbeta, float* coef_out, void* stream);

/* Backward of the residual junction of LocalFeatureAggregation (modules.py:325):
 *     O = LeakyReLU_slope( BN1(Y1) + BN2(Y2) ),   Y1 = mlp2 output, Y2 = shortcut output, no activation of their own.
 * Both branches receive the same g = G * (O > 0 ? 1 : slope); one sweep reduces both BatchNorms' sums
 * (rl_resid_bn_bwd_reduce fills stats1 / stats2 in the slot layout of rl_bn_bwd_reduce, to be finished by
 * rl_bn_bwd_finalize each) and one sweep writes both results (rl_resid_bn_bwd_apply):
 *     G  <- scale1 * (g - coef1[0] - xhat1 * coef1[1]),   G2 <- scale2 * (g - coef2[0] - xhat2 * coef2[1]).
 * All tensors are dense rows x C (C % 4 == 0, C/4 a power of two <= 256, 16-byte aligned); this replaces
 * rl_add_act_bwd + a copy + two rl_bn_bwd_reduce + two rl_bn_bwd_apply (15 passes over the tensor -> 10).       */
typedef struct rl_resid_bn_bwd_desc {
    float* G;                /* in: dL/dO;  apply: out, gradient w.r.t. Y1 */
    float* G2;               /* apply: out, gradient w.r.t. Y2 */
    const float* O;
    float slope;
    int64_t rows;
    int32_t C;
    const float* Y1; const float* scale1; const float* mean1; const float* invstd1;
    const float* Y2; const float* scale2; const float* mean2; const float* invstd2;
    double* stats1; double* stats2;          /* reduce: out */
    const float* coef1; const float* coef2;  /* apply: in (2*C floats each) */
} rl_resid_bn_bwd_desc;

int rl_resid_bn_bwd_supported(int64_t rows, int C);
int rl_resid_bn_bwd_reduce(const rl_resid_bn_bwd_desc* d, void* stream);
int rl_resid_bn_bwd_apply(const rl_resid_bn_bwd_desc* d, void* stream);
/* ... and the junction's two sweeps + rl_bn_bwd_finalize_pair as ONE launch for rows <= 2048 (stats / coef fields unused). */
int rl_resid_bn_bwd_fused_supported(int64_t rows, int C);
int rl_resid_bn_bwd_fused(const rl_resid_bn_bwd_desc* d, float* dgamma1, float* dbeta1, float* dgamma2, float* dbeta2, void* stream);

/* ------------------------------------------------------------------------------------------
 * Row movement.  dst row r of `rows` rows (r = b*rows_per_batch + i) receives `C` channels:
 *   src row = b*src_bstride + (index ? (index_shared ? index[i] : index[r]) : i)
 *   dst[r*ldd + c] (=|+=) lazy(src[src_row*lds + c]),  c < C
 * index may be int32 (index32) or int64 (index64); at most one is non-NULL.
 * Covers: input permutation, PointFeatureAugmentation gather+concat, decoder interpolation
 * gather + skip concat, gradient splits.                                                    */
typedef struct rl_rows_desc {
    const float* src;
    int64_t lds, src_bstride;
    float* dst;
    int64_t ldd;
    int64_t rows, rows_per_batch;
    int32_t C;
    const int32_t* index32;
    const int64_t* index64;
    int32_t index_shared;
    int32_t accumulate;
    int32_t act;
    float slope;
    const float* scale;
    const float* shift;
} rl_rows_desc;

int rl_copy_rows(const rl_rows_desc* d, void* stream);
/* Two independent copies (e.g. the two halves of a concat, modules.py:183 / 362) in one launch; same results as two calls. */
int rl_copy_rows_pair(const rl_rows_desc* d0, const rl_rows_desc* d1, void* stream);

/* Transposed movement (gather backward): dst[(b*src_bstride + index[r])*ldd + c] += src[r*lds + c]
 * (src_bstride names the batch stride of the INDEXED tensor, here dst) with fp32 atomics.  NON-DETERMINISTIC (the order of
 * the adds is not fixed; dst must be zeroed by the caller) and NOT used by the network's schedule, whose gather backward is
 * rl_csr_build + rl_segment_sum_rows: refused with RL_ERR_UNSUPPORTED unless RL_ALLOW_FLOAT_ATOMICS=1 is in the environment
 * (the same holds for rl_gemm's out2_index).                                                                          */
int rl_scatter_add_rows(const rl_rows_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * Deterministic gather backward.  The reference's backward of `torch.gather(features, idx)`
 * (PointFeatureAugmentation, modules.py:213-221; nearest_neighbor_interpolation, modules.py:359-364)
 * is a scatter_add_ whose summation order is undefined.  Here the neighbour graph is transposed once
 * per step and every destination row adds its contributions in ascending source-row order.
 *
 * rl_csr_build: for each task (a graph idx (B, n_src, k) int32 with values in [0, n_dst)) writes
 *   offsets (B, n_dst + 1): segment bounds of destination j of cloud b, local to the cloud
 *   entries (B, n_src*k)  : local source rows r = i*k + kk with idx[b][i][kk] == j, ascending per segment
 * All tasks (<= 8, same B) run in one launch set; workspace of rl_csr_workspace_bytes bytes, 256-byte
 * aligned.  Out-of-range indices are ignored.                                                   */
typedef struct rl_csr_task {
    const int32_t* idx;
    int32_t n_src, k, n_dst;
    int32_t* offsets;
    int32_t* entries;
} rl_csr_task;

int64_t rl_csr_workspace_bytes(const rl_csr_task* tasks, int ntasks, int B);
int rl_csr_build(const rl_csr_task* tasks, int ntasks, int B, void* workspace, int64_t workspace_bytes,
                 void* stream);

/* dst[(b*dst_bstride + j)*ldd + c] (=|+=) sum over e in [offsets[b][j], offsets[b][j+1]) of
 * src[(b*src_bstride + entries[b][e])*lds + c],  c < C, added in the order of the segment.
 * `src` may point at a column offset inside wider rows (lds is the row stride).                 */
typedef struct rl_segsum_desc {
    const float* src;
    int64_t lds, src_bstride;
    float* dst;
    int64_t ldd, dst_bstride;
    const int32_t* offsets;
    const int32_t* entries;
    int64_t entries_per_cloud;
    int32_t B, n_dst, C;
    int32_t accumulate;
    int32_t src_bf16;       /* bf16-storage mode: the source rows are bf16 (lds counts elements); sums and dst stay fp32 */
} rl_segsum_desc;

int rl_segment_sum_rows(const rl_segsum_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * Attentive pooling core (modules.py:246-253) on X, S of shape (P*K) x C (K consecutive rows
 * per point): A = softmax over the K rows of S, per channel;  Pout[p][c] = sum_k A*X.
 * Backward: dS = A * dP * (X - Pout);  dXa = dP * A  (the direct path of X).               */
int rl_attpool_fwd(const float* X, const float* S, int64_t P, int K, int C, float* Pout,
                   void* stream);
int rl_attpool_bwd(const float* X, const float* S, const float* Pout, const float* dP, int64_t P,
                   int K, int C, float* dS, float* dXa, void* stream);

/* The same on an X = [act(bn(U)) | act(bn(G[idx]))] that is not stored (round 8): channels below h of row pt*16 + k come from
 * U[(pt*16 + k)*ldu + c], the others from G[(b*g_bstride + idx[pt*16 + k])*ldg + c - h] with b = pt / n, each through its half's
 * fold (scale / shift both or neither; the value rl_copy_rows would have stored, bit for bit) - same arithmetic behind the load,
 * the same Pout / dS / dXa bits.  K == 16, C == 2*h, h % 64 == 0, fewer than 2^32 elements; else RL_ERR_UNSUPPORTED. */
typedef struct rl_attpool_src {
    const float* U;
    int64_t ldu;
    const float* u_scale;
    const float* u_shift;
    int32_t u_act;
    float u_slope;
    const float* G;
    int64_t ldg, g_bstride;
    const float* g_scale;
    const float* g_shift;
    int32_t g_act;
    float g_slope;
    const int32_t* idx;      /* one int32 per row of X, inside the cloud */
    int32_t n;               /* points per cloud */
    int32_t h;               /* columns per half */
} rl_attpool_src;
int rl_attpool_cat_supported(const rl_attpool_src* x, int64_t P, int K, int C);   /* the entries' own validation, no launch */
int rl_attpool_fwd_cat(const rl_attpool_src* x, const float* S, int64_t P, int K, int C, float* Pout, void* stream);
int rl_attpool_bwd_cat(const rl_attpool_src* x, const float* S, const float* Pout, const float* dP, int64_t P, int K, int C,
                       float* dS, float* dXa, void* stream);
/* How a caller that has the choice hands the d = 256 block's X (the un-fused pooling path) to the score product, the attentive
 * pooling and the weight gradient: "in_place" (X is never stored: rl_gemm_desc.a2_*, rl_attpool_*_cat, rl_wgrad_desc.a2_*) or
 * "stored" (rl_copy_rows_pair builds it).  Same results bit for bit.  The library only keeps the setting; a process setting
 * rather than an environment variable so that both paths can run in one process. */
int rl_set_pool256_x(const char* mode);
const char* rl_get_pool256_x(void);
/* (round 9) The same choice for a decoder step's concat [act(bn(x))[nn] | skip] (modules.py:362): "in_place" (never stored: the
 * step's product and weight gradient take rl_gemm_desc.a2_* / rl_wgrad_desc.a2_* with a2_first = 1, and the input gradient of a
 * narrow step leaves in two pieces through the streaming kernel's dense split store) or "stored" (rl_copy_rows_pair builds it).
 * Same results bit for bit; the library only keeps the setting. */
int rl_set_decoder_cat(const char* mode);
const char* rl_get_decoder_cat(void);

/* Fused attentive pooling (d = 16 / 32 / 64, and 128 in the bf16x3 / bf16 arithmetic modes; 16 neighbours): gather + concat
 * (modules.py:213-221), score Linear + softmax over K + weighted sum (modules.py:246-253) without
 * materialising the (points*K) x d tensors.
 *   U   (points*16) x d/2 lazy rpe-branch features;  G  lazy per-point features, row (b,i) at
 *   (b*g_bstride + i)*(d/2), gathered through idx (points,16) int32;  W (d,d) score weight.
 * rl_pool_fwd : Pout (points, d).
 * rl_pool_bwd : given dP (points, d) recomputes the block and produces GU (gradient w.r.t. the
 *   activated U, stored or accumulated), DG ((points*16) x d/2, plain stores: the gradient w.r.t. the
 *   activated gathered row of every neighbourhood slot - rl_segment_sum_rows then sums it per gathered
 *   point in a fixed order) and dW (d,d) through per-workgroup slabs (rl_pool_slab_floats floats).  */
typedef struct rl_pool_desc {
    const float* U;
    const float* u_scale;
    const float* u_shift;
    int32_t u_act;
    float u_slope;
    const float* G;
    int64_t g_bstride;
    const float* g_scale;
    const float* g_shift;
    int32_t g_act;
    float g_slope;
    const int32_t* idx;
    const float* W;
    int64_t points;
    int32_t n, d, nbr_k;
    float* Pout;
    const float* dP;
    float* GU;
    int32_t gu_accumulate;
    float* DG;
    float* dW;
    float* slab;
    int64_t slab_floats;
    /* d = 128 (supported outside the fp32 arithmetic mode): rl_pool_bwd does not produce dW; it writes the block's
     * X = [rpe, gathered] and dS, (points*16) x 128 floats each, and the caller computes dW = dS^T.X with rl_wgrad
     * (dY = dS_out, A = X_out).  dW / slab are ignored then. */
    float* X_out;
    float* dS_out;
    /* u_source 1 / 2 (d = 16 / 32 / 64): the rpe-branch half of X is not read from U but RECOMPUTED per point from the
     * coordinates - the outputs of mlp_rpe1 / mlp_rpe2 (modules.py:287-291, 313-320) never exist in memory:
     *   1: relu(bn1(rpe . W1^T + b1))                          rpe = [x_i, x_nbr, x_i - x_nbr, sqrt(d2)] (modules.py:173-186)
     *   2: relu(bn2(relu(bn1(rpe . W1^T + b1)) . W2^T + b2))
     * xyz (B, xyz_bstride, xyz_width) with xyz_width 3 (0 means 3) or 4 (x, y, z and one unused float per point,
     * 16-byte aligned: one gather per neighbour instead of three); nbr_d2 (points,16); W1 (d/2, 10), W2 (d/2, d/2)
     * reference conv layouts [out][in];
     * scale / shift = the folded BatchNorms (rl_bn_finalize on rl_rpe_stats' partials), mean / invstd = their saved
     * batch statistics (backward entry points only).  U is ignored.                                         */
    int32_t u_source;
    const float* xyz;
    int64_t xyz_bstride;
    const float* nbr_d2;
    const float* W1;
    const float* b1;
    const float* scale1;
    const float* shift1;
    const float* W2;
    const float* b2;
    const float* scale2;
    const float* shift2;
    const float* mean1;
    const float* invstd1;
    const float* mean2;
    const float* invstd2;
    int32_t xyz_width;
    /* rl_pool_bwd with a virtual stage, optional: when this launch COMPLETES the gradient of the stage's activated
     * output (GU after it holds the total), it also leaves the batch-statistics partials of that stage's BatchNorm
     * backward - what rl_rpe_bn_reduce would compute from GU - in bn_bwd_stats[slot][2][d/2], slot <
     * rl_pool_bwd_slots(points, d), saving that pass. */
    double* bn_bwd_stats;
    /* rl_pool_fwd with u_source 1, optional: the batch statistics of the NEXT stage's raw output (mlp_rpe2 applied to the
     * tile this launch has in registers) - what rl_rpe_stats with u_source 2 would compute - as partials
     * bn_fwd_stats2[slot][2][d/2], slot < rl_pool_fwd_slots(points, d).  Needs W2 / b2. */
    double* bn_fwd_stats2;
    /* bf16-storage mode (backward entry points): the (points*16)-row gradient tensors this block WRITES are bf16 (2 bytes
     * per element, round to nearest even) instead of fp32: DG, X_out and dS_out always; GU - and the G / GU1 arguments
     * of rl_rpe_bn_reduce / rl_rpe_wgrad - when the rpe branch is virtual (u_source > 0).  With a real U tensor GU stays
     * fp32 (it continues into the fp32 GEMM chain).  Needs the bf16x3 arithmetic mode.  0: everything fp32.        */
    int32_t rows_bf16;
    /* SHIFTED BatchNorm statistics (see rl_gemm_desc.stats_pivot_*): the running mean of mlp_rpe1's / mlp_rpe2's BatchNorm
     * (modules.py:288-291).  With pivot_mean1, rl_rpe_stats (u_source 1) leaves the sums of (y - pivot_mean1) and its square,
     * y = raw + b1; with pivot_mean2 so do rl_rpe_stats (u_source 2) and rl_pool_fwd's bn_fwd_stats2 for the second stage.
     * rl_bn_finalize must then be called with `pivoted` (and no folded bias: these sums are those of y).  NULL: plain sums. */
    const float* pivot_mean1;
    const float* pivot_mean2;
    /* rl_pool_bwd at d = 128, != 0: X_out may be NULL, and the kernel then does not store X at all (a third of its stores) -
     * the caller's weight gradient reads X's halves in place (rl_wgrad_desc.a2_*: A = U, A2 = G, a2_idx = idx).  fp32 rows
     * only.  0: a d = 128 call without X_out is refused as before. */
    int32_t x_optional;
} rl_pool_desc;

int rl_pool_supported(int d, int nbr_k);
int64_t rl_pool_slab_floats(int64_t points, int d);
int rl_pool_bwd_slots(int64_t points, int d);   /* workgroups (= partial slots) of an rl_pool_bwd launch with a virtual stage */
/* workgroups of an rl_pool_bwd launch = partial dW slabs it leaves.  With rl_pool_desc.dW == NULL the call does not sum them: the
 * caller queues (slab, nsplit = this, N = K = d, stride d*d + d) for rl_wgrad_reduce_batch.  rl_pool_slab_floats covers both. */
int rl_pool_bwd_grid(int64_t points, int d, int virtual_stage);
int rl_pool_fwd_slots(int64_t points, int d);   /* workgroups (= partial slots) of an rl_pool_fwd launch */
int rl_pool_fwd(const rl_pool_desc* d, void* stream);
int rl_pool_bwd(const rl_pool_desc* d, void* stream);
/* How a caller that has the choice hands the d = 128 block's X to its weight gradient: "stored" (rl_pool_bwd writes X_out, the
 * weight gradient reads it back) or "in_place" (x_optional + the concat-gather operand).  Same results bit for bit.  The
 * library only keeps the setting (rl_pool_bwd and rl_wgrad do what their descriptors say): it is a process setting rather
 * than an environment variable so that both paths can run in one process. */
int rl_set_pool128_x(const char* mode);
const char* rl_get_pool128_x(void);

/* BatchNorm batch statistics of the RAW output of stage u_source (1: mlp_rpe1, 2: mlp_rpe2) of the virtual rpe branch
 * described by d (xyz, idx, nbr_d2, W1, b1 [, scale1, shift1, W2, b2]): per-workgroup partials (sum, sum of squares;
 * doubles) stats[slot][2][d/2], slot < rl_rpe_stats_slots(points) - what the GEMM epilogue of that layer would have left
 * for rl_bn_finalize, without the (points*16) x d/2 tensor.                                                    */
int rl_rpe_stats_slots(int64_t points);
int rl_rpe_stats(const rl_pool_desc* d, double* stats, void* stream);

/* Backward of virtual stage u_source (BatchNorm + ReLU + the stage's Linear).  G (points*16, d/2) is the gradient w.r.t.
 * the ACTIVATED stage output, as rl_pool_bwd writes it to GU; the raw tile is recomputed (scale / shift / mean / invstd
 * of the stage's BatchNorm - and of stage 1 for stage 2 - must be set in d).
 *   rl_rpe_bn_reduce : partials of sum g and sum g*xhat, g = G*[output > 0]: stats[slot][2][d/2], slot <
 *                      rl_rpe_stats_slots(points), for rl_bn_bwd_finalize (-> dgamma, dbeta, coef).
 *   rl_rpe_wgrad     : dY = scale*(g - coef[c] - xhat*coef[d/2 + c]); per-workgroup partial slabs [slot][h*Kin + h]
 *                      (dW[n][k], then db[n]; Kin = 10 for stage 1, d/2 for stage 2), nsplit = rl_rpe_stats_slots(points),
 *                      to be summed by rl_wgrad_reduce_batch; stage 2 also writes GU1 (points*16, d/2) = dY . W2, the
 *                      gradient w.r.t. the activated stage-1 output.                                                  */
int rl_rpe_bn_reduce(const rl_pool_desc* d, const float* G, double* stats, void* stream);
int64_t rl_rpe_wgrad_slab_floats(int64_t points, int d, int stage);
int rl_rpe_wgrad(const rl_pool_desc* d, const float* G, const float* coef, float* slab, int64_t slab_floats,
                 float* GU1, void* stream);

/* Residual sum of two lazy tensors + LeakyReLU (modules.py:325):
 *   O = lrelu(Y1*s1+b1 + Y2*s2+b2);  backward (in place): G <- G * (O > 0 ? 1 : slope)       */
int rl_add_act_fwd(const float* Y1, const float* s1, const float* b1, const float* Y2,
                   const float* s2, const float* b2, int64_t rows, int C, float slope, float* O,
                   void* stream);
int rl_add_act_bwd(float* G, const float* O, int64_t rows, int C, float slope, void* stream);

/* RelativePositionEncoding (modules.py:173-186) written out once per level: row (b, i, j) of out, 12 floats
 * apart, holds [x_i, x_nbr, x_i - x_nbr, sqrt(d2)] (10 channels) and two zeros of padding, so that the row
 * is 16-byte aligned and the tensor can be the A operand of rl_gemm / rl_wgrad with K = 10, lda = 12.
 * The a_mode-1 operand source computes the same values inside the kernels; this tensor is the faster choice
 * when it is read more than once (forward + weight gradient).  xyz (B, xyz_bstride, 3), idx/d2 (B,n,k).   */
int rl_rpe_build(const float* xyz, int64_t xyz_bstride, const int32_t* nbr_idx, const float* nbr_d2, int B,
                 int n, int k, float* out, void* stream);
/* the same with the DISTANCES given (RelativePositionEncoding.forward's own signature, modules.py:159-186) */
int rl_rpe_build_dist(const float* xyz, int64_t xyz_bstride, const int32_t* nbr_idx, const float* nbr_dist, int B,
                      int n, int k, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Input pipeline on the device: PointCloudPreprocessor.preprocess
 * (randlanet/utils/dataset.py:61-97) + perturbate_point_cloud (randlanet/utils/augmentation.py:147-167)
 * + the DataLoader collation, for a batch of clouds that are resident in HBM.  The caller draws the
 * random numbers (sample indices, jitter noise, scale, rotation matrix, shift draws), this call applies
 * them in the reference's order with float64 arithmetic and rounds to float32 at the end, exactly
 * where the reference does (dataset.py:51).  One rl_cloud_job per cloud, array in DEVICE memory.
 *   indices (B,n) int64: rows of the source cloud to take (preprocessing.sample_points, :35-62)
 *   noise   (B,n,3) float64 standard-normal draws for the jitter, or NULL (no jitter)
 *   scratch rl_batch_assemble_scratch_doubles(B, n) float64 of work space ((B,n,3) coordinates + the records / arrival
 *           counters of the cloud-wide sums; any content - the call resets what it needs; one scratch per concurrent call)
 * Up to 16 workgroups share a cloud and meet at an arrival-counter barrier per cloud-wide sum; their number is sized so that
 * a launch fits the device at once (occupancy calculator, per device), and the wait is BOUNDED: a workgroup whose peers do not
 * arrive within ~1 s (a CU mask or partition mode the attribute does not show) gives up, sets the cloud's error word in
 * `scratch` (32-bit word rl_batch_assemble_flag_u32(B, n, b): 0 = fine) and writes the finite coordinates it has - never NaN -
 * instead of hanging the GPU; the caller reads the B words back (asynchronously) and treats a non-zero one as a failed
 * launch.
 *   out_input (B,n,3+F) float32 = [xyz, features], out_labels (B,n) int64
 * normal_col (0 = none): 1 + the first of three consecutive feature columns that hold a DIRECTION (a surface normal).  With
 * augment != 0 such a triple turns with the cloud: n'_r = float(((n_x*R[3r] + n_y*R[3r+1]) + n_z*R[3r+2])) in float64, the
 * product the centred coordinates go through; jitter, scale and shift do not act on directions, and every other column and
 * every coordinate is computed exactly as with normal_col = 0.  A triple that does not fit - normal_col < 0 or
 * 3 + normal_col - 1 > F - is refused with RL_ERR_ARGS before any launch where the host can read the records (pinned host
 * memory, which the device reads in place: no copy, no synchronisation); records in plain device memory are checked by the kernel instead, which
 * copies such a cloud's features as they are and sets bit 1 (value 2) of its error word.                               */
typedef struct rl_cloud_job {
    const void* xyz;          /* (n_points,3) float32, or float64 when xyz_f64 != 0 */
    const float* features;    /* (n_points,F) */
    const int64_t* labels;    /* (n_points,) */
    int64_t n_points;
    int32_t xyz_f64;
    int32_t normalization;    /* 0 none, 1 "mean", 2 "max", 3 "stdev", 4 any other string (centre only) */
    int32_t augment;          /* 0: the fields below are ignored */
    int32_t normal_col;       /* 0 none; c + 1: feature columns c, c+1, c+2 are a direction and are rotated by R */
    double jitter_variance, jitter_limit;
    double scale;             /* np.random.uniform(1 - scale_limit, 1 + scale_limit) */
    double R[9];              /* Rz.Ry.Rx, row-major */
    double shift[3];          /* np.random.uniform(-shift_limit, shift_limit, 3), before the radius factor */
} rl_cloud_job;

int64_t rl_batch_assemble_scratch_doubles(int B, int n);
int64_t rl_batch_assemble_flag_u32(int B, int n, int b);
int rl_batch_assemble(const rl_cloud_job* jobs_dev, int B, int n, int F, const int64_t* indices,
                      const double* noise, double* scratch, float* out_input, int64_t* out_labels,
                      void* stream);
/* The random draws rl_batch_assemble consumes, made on the device in ONE launch (the device loader's fast mode; the
 * reference draws them from numpy's global stream - preprocessing.py:35-62 np.random.choice, augmentation.py:147 np.random.randn -
 * which is the loader's "numpy" mode): indices (B,n) = n rows of each cloud without replacement (a keyed permutation of
 * [0, n_points), no sort; with replacement past n_points), noise (B,n,3) = standard-normal float64; either may be NULL.  Pure
 * functions of (seed, cloud, position). */
int rl_batch_draw(const rl_cloud_job* jobs_dev, int B, int n, uint64_t seed, int64_t* indices, double* noise, void* stream);

/* ------------------------------------------------------------------------------------------
 * The head of the network, fused for the training step (round 5): Dropout(p) -> fc_end.3 (Conv2d 32 -> C without BatchNorm,
 * modules.py:525-530) -> un-permute (modules.py:608) -> loss + metric counts (losses.py:17-87, metrics.py:8-59) as ONE kernel,
 * and its whole backward - loss derivative, permute, input gradient of fc_end.3, Dropout backward - as ONE more, which also
 * leaves the BatchNorm-backward sums of fc_end.1 and fc_end.3's weight / bias gradient slabs.  The step's logits are never stored.
 *   X (B*N, 32): raw output of fc_end.1 in PERMUTED row order, with its folded BatchNorm (scale, shift, act, slope) applied on
 *     load; perm (N) int64: row r of cloud b is point perm[r] (its label: labels[b][perm[r]]); W (C, 32), bias (C): fc_end.3.
 *   Dropout: the mask of rl_dropout_fwd (Philox on (element quad, *drop_key | drop_seed), rows offset by drop_first_row);
 *     drop_p == 0: none.
 *   work: rl_loss_work_doubles(B*N, C) doubles; rl_head_fwd fills the slots and the totals record and writes `out`
 *     (1 + 4*C doubles) exactly as rl_loss_forward does; rl_head_bwd reads the totals record.
 *   rl_head_bwd: G (B*N, 32) = gradient w.r.t. fc_end.1's ACTIVATED output (input of rl_bn_bwd_apply / rl_bn_backward);
 *     bn_bwd_stats (optional): [rl_head_grid(rows)][2][32] doubles, the partials rl_bn_bwd_reduce would leave for fc_end.1
 *     (needs mean / invstd); slab: rl_head_grid(rows) partial records of C*32 + C floats (dW[C][32], then db[C]) for
 *     rl_wgrad_reduce_batch (nsplit = rl_head_grid(rows), N = C, K = 32).
 * rl_head_supported(C, K): 1 for K == 32 and 1 <= C <= 32 (up to 8 classes: a class' weights and sums in registers; 9 .. 32,
 * round 6: the three 32-row products of a trip on exact-fp32 MFMA with their operands in LDS); otherwise the caller runs the
 * separate entry points.  The fused head takes 1 .. 32 classes only: from 33 classes on (up to RL_MAX_CLASSES) the caller runs
 * rl_dropout_fwd, rl_gemm, rl_logits_unpermute and rl_loss_forward, and the (B,C,N) logits of the step are stored. */
typedef struct rl_head_desc {
    const float* X;
    const float* scale;
    const float* shift;
    int32_t act;
    float slope;
    const float* mean;
    const float* invstd;
    const float* W;
    const float* bias;
    const int64_t* perm;
    const int64_t* labels;
    int32_t B, N, C;
    int32_t loss_kind;
    float alpha, gamma;
    int32_t neglect_background;
    float drop_p;
    const int64_t* drop_key;
    uint64_t drop_seed;
    int64_t drop_first_row;
    double* work;
    float* G;
    double* bn_bwd_stats;
    float* slab;
    int64_t slab_floats;
    float grad_scale;
    int32_t reserved;
    /* optional (drop_p > 0): B*N uint32 - the forward stores each row's 32 keep bits, the backward reads them instead of running
     * the generator a second time (a Philox call is ~40 quarter-rate integer multiplies: the dominant cost of both kernels) */
    void* drop_mask;
    int64_t perm_bstride;           /* 0: one permutation for every cloud; N: cloud b reads perm + b * N (rl_band_sort) */
    /* the masked mode of the loss (see rl_loss_forward_masked): C class weights on the device or NULL, and the flag; weights
     * imply the flag; NULL and 0: the default mode */
    const float* class_weight;
    int32_t masked;
} rl_head_desc;
int rl_head_supported(int C, int K);
int rl_head_grid(int64_t rows);
int rl_head_fwd(const rl_head_desc* d, double* out, void* stream);
int rl_head_bwd(const rl_head_desc* d, void* stream);

/* Dropout (fc_end, modules.py:528) with a keep-mask drawn by the caller (uint8, 1 = keep):
 * x[i] = mask[i] ? x[i]*scale : 0, in place; the same call is its own backward.             */
int rl_scale_mask(float* x, const uint8_t* mask, float scale, int64_t count, void* stream);

/* Dropout (fc_end's nn.Dropout, modules.py:528) with a counter-based generator (Philox4x32-10): element e of the
 * (rows, C) tensor is kept iff philox(seed, key[0], e) >= p*2^32; kept values are scaled by 1/(1-p).  `key` is a
 * device scalar, so a captured graph draws a fresh mask per replay: rl_dropout_tick does counter[0] += 1 and copies
 * the new value to key_out[0]; forward and backward of one pass read the same key and regenerate the same mask (no
 * mask tensor).  rl_dropout_fwd also applies the producer's lazy BatchNorm + activation; dense rows (ld = C), C % 4 == 0.
 * `first_row`: index of row 0 in the tensor of the WHOLE batch - e = (first_row + r) * C + c - so that ranks holding
 * shards of one batch draw the slices of ONE mask (0 for a single process). */
int rl_dropout_tick(int64_t* counter, int64_t* key_out, void* stream);
int rl_dropout_fwd(const float* src, const float* scale, const float* shift, int act, float slope, float* dst,
                   int64_t rows, int64_t first_row, int C, const int64_t* key, uint64_t seed, float p, void* stream);
int rl_dropout_bwd(float* G, int64_t rows, int64_t first_row, int C, const int64_t* key, uint64_t seed, float p, void* stream);

/* UpSampler (modules.py:343-456) on channel-first features feat (B,F,N1) with neighbours
 * idx/d2 (B,N2,k) from rl_knn_i32: power 0 = nearest-neighbour interpolation (k = 1),
 * power 1 / 2 = inverse (squared) distance weighting, w = (1+1e-7)/(dist^power + 1e-7)
 * normalised over the k neighbours.  out (B,F,N2).                                          */
int rl_upsample_cf(const float* feat, const int32_t* idx, const float* d2, int B, int F, int N1,
                   int N2, int k, int power, float* out, void* stream);

/* logits (B,N,C) channel-last in permuted order  <->  (B,C,N) in original order
 * (modules.py:608-611): out[b][c][perm[i]] = in[b][i][c]; backward is the gather.           */
int rl_logits_unpermute(const float* in, const int64_t* perm, int B, int N, int C, float* out,
                        void* stream);
int rl_logits_permute_grad(const float* dout, const int64_t* perm, int B, int N, int C,
                           float* din, void* stream);
/* the same with one permutation PER CLOUD: cloud b reads perm + b * perm_bstride (0: the shared permutation above) */
int rl_logits_unpermute_b(const float* in, const int64_t* perm, int64_t perm_bstride, int B, int N, int C, float* out,
                          void* stream);
int rl_logits_permute_grad_b(const float* dout, const int64_t* perm, int64_t perm_bstride, int B, int N, int C,
                             float* din, void* stream);

/* A spatial order INSIDE the sampling bands of the forward's permutation (modules.py:571, 587-598).  The reference sub-samples
 * by prefixes of ONE random permutation, so only the band [edges[k], edges[k+1]) a point falls in matters (edges = 0, N/dec^L,
 * ..., N/dec, N); inside a band the order is free, and the kernels run faster when it follows space.  perm_out[b] (N) holds, band
 * by band, the entries of `perm` in that band ordered by (4096-cell Morton code of cloud b's point, position) - a stable counting
 * sort, deterministic.  rows: (B, N, row_stride) fp32 with x, y, z first.  workspace: rl_band_sort_workspace_bytes(...) bytes,
 * 256-byte aligned.  Four launches, no memset, no global atomics.                                                              */
int64_t rl_band_sort_workspace_bytes(int B, int N, const int* edges, int nbands);
int rl_band_sort(const float* rows, int64_t row_stride, const int64_t* perm, int B, int N, const int* edges, int nbands,
                 int64_t* perm_out, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Loss + metrics on logits (B,C,N) fp32 and labels (B,N) int64, 1 <= C <= RL_MAX_CLASSES (256): every rl_loss_* entry below
 * returns RL_ERR_UNSUPPORTED above it and launches nothing.  1 .. 32 classes and 33 .. 256 classes run different kernels
 *  behind the same entries, records and formulas; rl_loss_max_classes() returns the bound of the build.
 * kind: 0 cross_entropy, 1 focal(gamma), 2 focal Tversky(alpha, gamma, neglect background)
 * (trainer.py:244-269 maps dice -> (0.5, 1), tversky -> (0.7, 1), focal_tversky -> (0.7, 4/3)).
 * rl_loss_forward fills out[0] = loss and the metric counts
 *   out[1 + 0*C + c] = #(pred==c & label==c), out[1 + 1*C + c] = #(label==c),
 *   out[1 + 2*C + c] = #(pred==c),            out[1 + 3*C + c] = sum_n softmax_c (diagnostic)
 * (accuracy / iou of metrics.py:8-59 are ratios of these counts), all as doubles, and keeps
 * what rl_loss_backward needs in `work` (rl_loss_work_doubles(B*N, C) doubles).
 * rl_loss_backward writes dlogits (B,C,N) = dloss/dlogits * grad_scale.                      */
int rl_loss_max_classes(void);
int64_t rl_loss_work_doubles(int64_t points, int C);
/* 1 <= C <= RL_MAX_CLASSES */
int rl_loss_forward(const float* logits, const int64_t* labels, int B, int C, int N, int kind,
                    float alpha, float gamma, int neglect_background, double* work, double* out,
                    void* stream);
/* 1 <= C <= RL_MAX_CLASSES */
int rl_loss_backward(const float* logits, const int64_t* labels, int B, int C, int N, int kind,
                     float alpha, float gamma, int neglect_background, const double* work,
                     float grad_scale, float* dlogits, void* stream);

/* The MASKED mode of the same loss, for partly labelled and class-imbalanced scenes.  A point is labelled when
 * 0 <= label < C; with masked != 0 an unlabelled point adds nothing to the loss or to any count (inter, label count,
 * prediction count, sum of softmax - `out` and `work` keep their layouts) and its gradient is exactly 0 at every class.
 * class_weight: C floats on the device (finite, >= 0, positive sum - and a positive sum over the classes the Tversky family
 * averages; the caller checks) or NULL for all ones; weights imply masked.  With w = class_weight and
 * W = sum over the labelled points of w[label]:
 *   cross entropy / focal: sum over the labelled points of w[label] * term / W (torch's cross_entropy(weight=, ignore_index=));
 *   Tversky family: tp, sum p, sum y over the labelled points, loss = sum_c w_c (1 - TI_c)^gamma / sum_c w_c over the
 *   classes it averages (from 1 with neglect_background).
 * W is formed on the device from the label counts of the totals record, by the forward's finalize and by the backward: it is
 * never a launch argument, so a captured step follows its batch.  No labelled point: loss 0, gradient 0.  Without weights and
 * without unlabelled points the results equal the default mode's bit for bit; class_weight NULL and masked 0 IS the default
 * mode (the same kernels as rl_loss_forward / rl_loss_backward).  1 <= C <= RL_MAX_CLASSES for both.               */
int rl_loss_forward_masked(const float* logits, const int64_t* labels, int B, int C, int N, int kind, float alpha,
                           float gamma, int neglect_background, const float* class_weight, int masked, double* work,
                           double* out, void* stream);
int rl_loss_backward_masked(const float* logits, const int64_t* labels, int B, int C, int N, int kind, float alpha,
                            float gamma, int neglect_background, const double* work, float grad_scale,
                            const float* class_weight, int masked, float* dlogits, void* stream);

/* The same loss in two steps, for the data-parallel EQUIVALENCE mode (the dice ratio of the global
 * batch is not the mean of per-rank dice ratios): rl_loss_partials runs the pass over the logits and leaves this
 * rank's sums in the totals record, 5*C+1 doubles at work + rl_loss_totals_offset(C); the caller all-reduces that
 * record (SUM) over the ranks; rl_loss_from_totals forms the loss and the metric counts from it with the GLOBAL
 * point count; rl_loss_backward_global is rl_loss_backward normalised by the global point count.
 * 1 <= C <= RL_MAX_CLASSES for all four.                                                                      */
int rl_loss_partials(const float* logits, const int64_t* labels, int B, int C, int N, int kind, float gamma,
                     double* work, void* stream);
int64_t rl_loss_totals_offset(int C);
int rl_loss_from_totals(int64_t points_total, int C, int kind, float alpha, float gamma, int neglect_background,
                        double* work, double* out, void* stream);
int rl_loss_backward_global(const float* logits, const int64_t* labels, int B, int C, int N, int kind, float alpha,
                            float gamma, int neglect_background, const double* work, float grad_scale,
                            int64_t points_total, float* dlogits, void* stream);

/* The Lovasz-Softmax loss (Berman et al., CVPR 2018), the sorted mIoU surrogate, alone or summed with the masked cross entropy
 * (with_ce != 0): loss kinds 3 and 4 of the Python layers.  randlanet/utils/lovasz.py is its specification (a numpy twin); in short
 *   p = softmax per point by exp_fixed (rl_scene_accumulate_first's bits); a point is labelled when 0 <= label < C, and the
 *   Lovasz term always skips the others; P labelled points, G_c of them of class c, class c "present" when G_c > 0;
 *   per present class: e_i = |[y_i = c] - p_ci| in fp32, sorted descending, ties by ascending point index b*N + i;
 *   J_r = 1 - (G_c - cum_r) / (G_c + r - cum_r) (cum_r: foreground among the first r), g_r = J_r - J_(r-1) in fp64, J_0 = 0;
 *   loss = sum_c w_c sum_r e_(r) g_r / sum of w_c over the present classes (w = class_weight or ones; 0 when that sum is 0);
 *   dloss/dp_ci = sign(p_ci - [y_i = c]) g_rank(i) w_c / sum w, g constant; dlogits by the softmax' backward, exact zeros
 *   at unlabelled points.
 * ws: rl_lovasz_workspace_bytes(B, C, N) bytes, 256-byte aligned (-1: unsupported sizes); the forward leaves in it what the
 *   backward reads, among it the table coef (C, B*N) fp32 = (float)g_rank(i), 0 at absent classes and unlabelled points, at
 *   byte offset rl_lovasz_coef_offset(B, C, N): equal to the twin's bit for bit.
 * out: rl_loss_forward's record of 1 + 4*C doubles; out[1:] is exactly what rl_loss_forward_masked(kind 0, masked = 1) writes,
 *   out[0] the Lovasz loss, plus that cross entropy (same class_weight) with with_ce.
 * 1 <= C <= RL_MAX_CLASSES and B*N*C < 2^31, else RL_ERR_UNSUPPORTED and nothing is launched; null pointers or a small workspace
 * -> RL_ERR_ARGS before any launch.  The sort is the stable radix sort of rl_grid_sort; P, G_c and the present set are device
 * state (no host read-back: a captured step follows its batch); no floating-point atomics, no workgroup waits for another one,
 * results are a pure function of the input.                                                                          */
int64_t rl_lovasz_workspace_bytes(int B, int C, int N);
int64_t rl_lovasz_coef_offset(int B, int C, int N);
int rl_lovasz_forward(const float* logits, const int64_t* labels, int B, int C, int N, int with_ce,
                      const float* class_weight, void* ws, int64_t ws_bytes, double* out, void* stream);
int rl_lovasz_backward(const float* logits, const int64_t* labels, int B, int C, int N, int with_ce,
                       const float* class_weight, const void* ws, int64_t ws_bytes, float grad_scale, float* dlogits,
                       void* stream);

/* Softmax over the class axis of (B,C,N) logits -> confidences (model.py:137, 229).         */
int rl_softmax_cf(const float* logits, int B, int C, int N, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Adam over a flat parameter buffer (torch.optim.Adam defaults, trainer.py:78): step[0] is
 * incremented on the device, lr is read from device memory, grads are multiplied by
 * grad_scale first (1/world_size after a gradient all-reduce).                              */
int rl_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                 const float* lr, float beta1, float beta2, float eps, float grad_scale,
                 int64_t* step, void* stream);

/* ------------------------------------------------------------------------------------------
 * Voted-crop inference over a whole scene (Model.predict_scene; no counterpart in the reference).  Restates the test
 * protocol of RandLA-Net (Hu et al., CVPR 2020; the authors' S3DIS / Semantic3D testers) - one "possibility" value per
 * point, crops of the n nearest neighbours of the least covered point, softmax blended per point - with the arithmetic
 * of the numpy twin randlanet/utils/scene.py, bit for bit where it says so.
 *   cloud (M, dim) row-major fp32, dim = 3 + F, x y z first; possibility (M) fp32; indices int32 (M < 2^31 - 1).
 * rl_scene_crop, one crop on the device, the centre never leaves it:
 *   pick     c = argmin possibility, ties to the lowest index;
 *   select   d2_i = ((dx*dx)+(dy*dy))+(dz*dz) without FMA (the expression of rl_knn_*), the crop = the n smallest keys
 *            (d2_i, i): every d2 < T plus the lowest-indexed points with d2 == T, T the n-th smallest d2 (radix select
 *            over the fp32 bits, 11/11/10-bit digits); idx_out (n) int32 in ASCENDING POINT INDEX order;
 *   gather   rows_out + j*row_stride = cloud row idx_out[j] (the raw frame), row_stride >= dim floats;
 *   update   possibility[idx_out[j]] += t*t, t = 1 - d2_j / d2max (correctly rounded division), d2max = T the largest
 *            d2 of the crop (d2max == 0: t = 1) - bit-identical to the same float32 expressions in numpy.
 *   ws: rl_scene_workspace_bytes(M, n) bytes, 256-byte aligned (also serves rl_scene_min_count).  n > M, dim < 3,
 *   row_stride < dim or a small workspace -> RL_ERR_ARGS before any launch.  Six launches, no host synchronisation.
 * rl_scene_accumulate, one crop's logits (C, n) (class stride n; row b of an eval forward's (B, C, n) output):
 *   sm = softmax over C (rl_softmax_cf's expression); prob[idx[j]*C + c] = s*prob[..] + one_minus_s*sm_c (prob (M, C),
 *   one_minus_s rounded to fp32 once by the caller); count[idx[j]] += 1 (int32 (M)).  idx must be duplicate-free (a crop
 *   is); crops that overlap are blended by one call each, in order, on one stream.
 * rl_scene_min_count: out[0] = min over count (M), one int32 in device memory; ws as for rl_scene_crop.
 * rl_scene_crop_padded, rl_scene_crop's arguments, any n > 0 (Model.predict_scene(pad_small_scenes=True)):
 *   M >= n   rl_scene_crop's crop, bit for bit (the same launches);
 *   M <  n   the select takes every point: T = the largest d2 of the scene, every possibility rises ONCE by
 *            (1 - d2_i / T)^2 (T == 0: by 1), slot j of idx_out (n) and rows_out (n rows) holds cloud row j mod M - rows
 *            0 .. M-1 ascending, then repeated cyclically (numpy: np.resize(arange(M), n)).  The authors' generator fills
 *            a small cloud up with np.random.choice; cyclic repeats are a deliberate deviation: every point weighs the same
 *            within one repeat, and no random stream enters the crop sequence.
 *   The workspace is rl_scene_crop's (its size does not depend on n).  Six launches; no workgroup waits for another.
 * rl_scene_accumulate_first, rl_scene_accumulate over the first `first` slots of a crop whose logits are (C, ld) (class
 *   stride ld >= n >= first, first <= M): slots first .. n-1 (the repeats of a padded crop) leave prob and count untouched,
 *   so a point is voted once per crop.  The blend is rl_scene_accumulate's; the softmax takes its exp by a fixed sequence
 *   of fp32 operations (k = rint(x*log2(e)), r = x - k*ln2 in two steps, Cephes' degree-5 polynomial by Horner in separate
 *   multiplies and adds, times 2^k; 0 below -87) instead of the library's expf, so a host restatement of those operations
 *   (utils/scene.py: exp_fixed) gives the same bits.  Against rl_scene_accumulate at ld = first = n the probabilities
 *   differ by a few 1e-7 relative.                                                                                      */
int64_t rl_scene_workspace_bytes(int64_t M, int n);
int rl_scene_crop(const float* cloud, int64_t M, int dim, float* possibility, int n, float* rows_out, int64_t row_stride,
                  int32_t* idx_out, void* ws, int64_t ws_bytes, void* stream);
int rl_scene_accumulate(const float* logits, int C, int n, const int32_t* idx, float one_minus_s, float s, float* prob,
                        int32_t* count, int64_t M, void* stream);
int rl_scene_min_count(const int32_t* count, int64_t M, int32_t* out, void* ws, void* stream);
int rl_scene_crop_padded(const float* cloud, int64_t M, int dim, float* possibility, int n, float* rows_out,
                         int64_t row_stride, int32_t* idx_out, void* ws, int64_t ws_bytes, void* stream);
int rl_scene_accumulate_first(const float* logits, int C, int n, const int32_t* idx, float one_minus_s, float s, float* prob,
                              int32_t* count, int64_t M, int64_t ld, int first, void* stream);

/* Training crops over many scenes (Model.train_scenes; no counterpart in the reference): RandLA-Net's training sampler
 * (the authors' spatially_regular_gen) on the device, the crop of rl_scene_crop generalised to S concatenated scenes.
 *   xyz (T, stride floats) fp32, x y z first; scene s owns rows [off[s], off[s+1]) (off (S+1) int64 in DEVICE memory,
 *   off[0] = 0, every scene n .. max_points rows, T < 2^31 - 1); possibility (T) fp32.  The row counts live in device
 *   memory and are not checked: a scene of fewer than n rows leaves part of its crop's idx_out row unwritten (callers
 *   validate the sizes on the host, as utils/scene_loader.py does).
 * rl_scenes_init: copies off into ws and keeps one key per scene, min over the scene of (ordered bits(possibility), row).
 *   Call it again after the possibilities were rewritten.  Every rl_scenes_crop on that workspace must pass the same S and
 *   max_points as the rl_scenes_init call that prepared it (the workspace layout depends on both).
 * rl_scenes_crop, B crops in order, each one:
 *   pick     g = argmin (possibility, row) over all scenes (the least of the S keys), s = the scene of g;
 *            scene_out[b] = s (int64);
 *   centre   p = xyz[g] + noise[b] (one fp32 add per component; noise (B, 3) fp32 in device memory, or NULL: p = xyz[g]);
 *   select   over scene s only, rl_scene_crop's d2 and key order: idx_out[b*n .. b*n+n) = the n smallest keys (d2_i, i) as
 *            GLOBAL rows (int64), ascending; T_s = the largest d2 of the crop;
 *   update   possibility[i] += (1 - d2_i / T_s)^2 as in rl_scene_crop; the key of scene s is refreshed.
 *   Every launch is sized for max_points; the range of the picked scene comes from ws, so a crop reads and writes
 *   O(M_s + S) bytes.  With S = 1 and no noise the crops are rl_scene_crop's, bit for bit.  No host synchronisation.
 *   ws: rl_scenes_workspace_bytes(S, max_points, n) bytes, 256-byte aligned, prepared by rl_scenes_init.  Bad sizes,
 *   null pointers or a small workspace -> RL_ERR_ARGS before any launch.
 * rl_scenes_crop_padded, rl_scenes_crop's arguments, scenes of 1 .. max_points rows, any n > 0 (also above max_points;
 *   Model.train_scenes(pad_small_scenes=True)): the pick kernel writes min(n, M_s) into ws, the number of keys the select
 *   passes take.  A picked scene of M_s >= n rows gives rl_scenes_crop's crop, bit for bit; one of M_s < n rows is taken
 *   whole as in rl_scene_crop_padded - T_s = its largest d2, every possibility raised once, idx_out[b*n + j] = off[s] +
 *   j mod M_s - the repeats written by every workgroup of the write launch, none waiting for another.  The workspace is
 *   rl_scenes_crop's (its size does not depend on n).                                                                 */
int64_t rl_scenes_workspace_bytes(int S, int64_t max_points, int n);
int rl_scenes_init(const int64_t* off, int S, int64_t max_points, const float* possibility, void* ws, int64_t ws_bytes,
                   void* stream);
int rl_scenes_crop(const float* xyz, int stride, int S, int64_t max_points, float* possibility, int n, int B,
                   const float* noise, int64_t* idx_out, int64_t* scene_out, void* ws, int64_t ws_bytes, void* stream);
int rl_scenes_crop_padded(const float* xyz, int stride, int S, int64_t max_points, float* possibility, int n, int B,
                          const float* noise, int64_t* idx_out, int64_t* scene_out, void* ws, int64_t ws_bytes,
                          void* stream);

/* Voted crops over many scenes (Model.predict_scenes, evaluate_scenes(together=True); no counterpart in the reference):
 * rl_scenes_crop_padded's sampler competing for coverage.  All scenes of a group stay resident; every slot of a pass goes
 * to the least covered point among the scenes that still need votes, and a scene leaves the moment it is covered.  The
 * numpy twin is randlanet/utils/scene.py: scenes_vote_crop / scenes_vote_accumulate, bit for bit.
 *   cloud (T, dim) row-major fp32, dim = 3 + F, x y z first, scene s owning rows [off[s], off[s+1]) as above; possibility
 *   (T) fp32; count (T) int32 and low (S) int32, both ZEROED by the caller before the first call: count[i] = the crops
 *   point i was in, low[s] = min of count over scene s.  Scene s is OPEN while low[s] < votes.  ws prepared by
 *   rl_scenes_init (same S and max_points).
 * rl_scenes_vote_crop, B crops in order, each one:
 *   pick     the least of the S scene keys among the open scenes.  No open scene: the slot is IDLE - scene_out[b] = -1,
 *            first_out[b] = 0, and every later launch of this crop exits without writing (idx_out / rows_out of the slot
 *            keep what they hold).  Otherwise as rl_scenes_crop(_padded when pad != 0) without noise: scene_out[b] = s,
 *            first_out[b] = min(n, M_s) = the leading duplicate-free slots (n without pad), low[s] = INT32_MAX;
 *   select   rl_scenes_crop's three select launches, unchanged;
 *   write    rl_scenes_crop(_padded)'s idx_out[b*n + j] (GLOBAL rows, int64) and possibility update, and beside it
 *            count[i] += 1 once per selected point (the cyclic repeats of a padded crop do not count); every workgroup
 *            folds the least count of its chunk after the update into low[s] by an integer atomicMin (the mechanism of the
 *            scene key); cloud row idx_out[b*n + j] is gathered into rows_out + b*slot_stride + j*row_stride (dim floats;
 *            row_stride >= dim, slot_stride >= n*row_stride), the repeats of a padded crop too;
 *   then one launch writes the number of open scenes to open_out[0] (int32, DEVICE memory).
 *   The count rises at crop time, not at blend time: the next crop of the same pass already sees a covered scene closed
 *   (a padded scene's farthest point gains 0 possibility - by possibility alone it would be picked again at once).  The
 *   crops taken from scene s are therefore a prefix of the sequence rl_scene_crop(_padded) takes on s alone from the same
 *   possibilities, ending at the first crop after which every point of s has `votes`.  6*B + 1 launches, no host
 *   synchronisation, no floating-point atomics, no workgroup waits for another.  Bad sizes, null pointers or a small
 *   workspace -> RL_ERR_ARGS before any launch.
 * rl_scenes_vote_accumulate, B launches in order (the crops of a pass overlap), slot b: logits + b*slot_stride is (C, ld)
 *   (class stride ld >= n), idx + b*n its GLOBAL rows (int64), first[b] (int32, read ON THE DEVICE: rl_scenes_vote_crop's
 *   first_out) the leading slots that are blended - slots j >= first[b] leave prob untouched, so an idle slot is a no-op
 *   and a point is voted once per crop.  prob (T, C): rl_scene_accumulate_first's softmax (the fixed exp) and blend.  No
 *   count is touched.  Bad sizes or null pointers -> RL_ERR_ARGS before any launch.                                        */
int rl_scenes_vote_crop(const float* cloud, int dim, int S, int64_t max_points, float* possibility, int32_t* count,
                        int32_t* low, int votes, int n, int B, int pad, float* rows_out, int64_t slot_stride,
                        int64_t row_stride, int64_t* idx_out, int64_t* scene_out, int32_t* first_out, int32_t* open_out,
                        void* ws, int64_t ws_bytes, void* stream);
int rl_scenes_vote_accumulate(const float* logits, int C, int n, int64_t ld, int64_t slot_stride, int B, const int64_t* idx,
                              const int32_t* first, float one_minus_s, float s, float* prob, int64_t T, void* stream);

/* Grid subsampling (randlanet/utils/grid.py: grid_subsample; Model.predict_scene / evaluate_scenes / train_scenes with
 * grid=; no counterpart in the reference): one representative per occupied voxel of edge `cell` - the barycentre, the mean
 * of every feature column, the majority label - with the arithmetic of the numpy twin grid_subsample_host, bit for bit.
 *   cloud (M, dim) row-major fp32, dim = 3 + F, x y z first, every coordinate finite (the caller checks); M < 2^31 - 1.
 * The four calls share one workspace and run in this order on one stream; the host reads back dims (to refuse a grid
 * dimension >= 2^21 and to count the key's bits) and V (to size the outputs), nothing else.
 * rl_grid_bounds:
 *   origin   o = floor(min / c) * c per axis, c = cell, every operation rounded to fp32;
 *   dims     floor((max - o) / c) + 1 per axis, at least 1; dims_out (3) int64 in DEVICE memory: x, y, z (clamped at 4e18).
 * rl_grid_sort, key_bits = the bits of dims_x * dims_y * dims_z - 1 (at least 1):
 *   key      v = max(floor((p - o) / c), 0) per axis in fp32 with a correctly rounded division, key = (vz*dims_y + vy)*dims_x
 *            + vx as int64;
 *   sort     (key, point index) by key, STABLE: an LSD radix sort over ceil(key_bits / 8) 8-bit digits, each pass a histogram
 *            per chunk of positions, a prefix over (digit, chunk), and a scatter whose ranks inside a chunk come from
 *            wavefront ballots in position order - the points of a cell stay in ascending index.
 * rl_grid_heads: the cells are the runs of equal keys of the sorted pairs, numbered in ascending key order: V_out[0] = their
 *   number (int64, DEVICE memory), inverse[i] = the cell of point i (int32 (M)); per-chunk head counts, their prefix by one
 *   workgroup, then the numbers by wavefront ballots in position order.
 * rl_grid_reduce, V as read back from V_out (cells past the V of the workspace are not written):
 *   rows_out (V, dim) fp32: every column summed over the cell's points in ascending point index in fp64, divided by the
 *            count in fp64, rounded once to fp32; count_out (V) int32;
 *   labels   (M) int64 in [0, n_classes) (the caller checks) or NULL; labels_out (V) int64: the most frequent class of the
 *            cell, ties to the lowest class.  One lane owns a cell: no atomics, a fixed order of every sum.
 *   ws: rl_grid_workspace_bytes(M, dim) bytes, 256-byte aligned.  Bad sizes, a cell that is not positive and finite, null
 *   pointers or a small workspace -> RL_ERR_ARGS before any launch.  No workgroup waits for another one.
 * rl_scene_confusion: table[label_i * C + argmax_c prob[r_i * C + c]] += 1 for every point i of (M) whose label is inside
 *   [0, C) (others are skipped: unlabelled), r_i = inverse[i] (int32, rows of prob (V, C) fp32; rows outside [0, V) are
 *   skipped) or i when inverse is NULL (then V == M); argmax ties go to the lowest class.  table (C, C) int64 in device
 *   memory is ADDED to by integer atomics (per-workgroup LDS tables up to 64 classes): the caller zeroes it and may
 *   accumulate several scenes.                                                                                          */
int64_t rl_grid_workspace_bytes(int64_t M, int dim);
int rl_grid_bounds(const float* cloud, int64_t M, int dim, float cell, int64_t* dims_out, void* ws, int64_t ws_bytes,
                   void* stream);
int rl_grid_sort(const float* cloud, int64_t M, int dim, int key_bits, void* ws, int64_t ws_bytes, void* stream);
int rl_grid_heads(int64_t M, int dim, int64_t* V_out, int32_t* inverse, void* ws, int64_t ws_bytes, void* stream);
int rl_grid_reduce(const float* cloud, int64_t M, int dim, const int64_t* labels, int n_classes, int64_t V, float* rows_out,
                   int64_t* labels_out, int32_t* count_out, void* ws, int64_t ws_bytes, void* stream);
int rl_scene_confusion(const float* prob, int64_t V, int C, const int64_t* labels, int64_t M, const int32_t* inverse,
                       int64_t* table, void* stream);

/* Euclidean clustering (randlanet/utils/cluster.py: euclidean_clusters; Model.predict_instances; no counterpart in the
 * reference): the connected components of the points that take part - label >= 0 and not in ignore - under the edge rule
 * "same label and d2 <= r2", r2 = radius * radius rounded to fp32, d2 = (dx*dx + dy*dy) + dz*dz with every operation rounded
 * to fp32; components of fewer than min_points points are dropped; the kept ones are numbered 0 .. I-1 in ascending order of
 * their smallest point index.  The numpy twin is euclidean_clusters_host; the result is a pure function of the input and
 * equals the twin's bit for bit.
 *   xyz (M, 3) row-major fp32, every coordinate finite (the caller checks); labels (M) int64; M < 2^31 - 1.
 * The three calls share one workspace and run in this order on one stream; the host reads back dims (to refuse a grid of
 * 2^16 cells or more on an axis and to count the key's bits) and I (to size the outputs), nothing else.
 * rl_cluster_cells: the box of ALL points and the grid of cell edge c = radius * 1.0625f over it, origin and dims as
 *   rl_grid_bounds computes them; dims_out (3) int64 in DEVICE memory.  With fewer than 2^16 cells on an axis every pair
 *   within radius lies at most one cell apart on every axis (DESIGN.md section 5 has the argument).
 * rl_cluster_union, key_bits = the bits of dims_x * dims_y * dims_z (at least 1; that product is the key of the points that
 *   take no part): cell keys, the stable radix sort of rl_grid_sort, then one lane per point scans the cells around its own
 *   and joins by a lock-free union-find over int32 parents (32-bit integer compare-and-swap, the larger root under the
 *   smaller one, path halving; relaxed agent-scope atomic loads and stores; no lane waits for another, no floating-point
 *   atomics); roots, component sizes by integer atomics, a second sort by root, heads.  ignore: n_ignore int64 classes in
 *   DEVICE memory (NULL with n_ignore = 0).  instance_out (M) int32: the number of the point's component, -1 for a point
 *   that takes no part or whose component was dropped; I_out[0] (int64, DEVICE memory) = I.
 * rl_cluster_reduce, I as read back from I_out (I >= 1): per instance classes_out (I) int64, count_out (I) int32,
 *   centroid_out (I, 3) fp32 - every column summed in fp64 over the members in ascending point index, divided by the count in
 *   fp64, rounded once -, lo_out / hi_out (I, 3) fp32 the bounding box, and with scores (M) fp32 score_out (I) fp32, the
 *   same fixed-order mean (both NULL otherwise).  One wavefront owns an instance: no atomics, a fixed order of every sum.
 *   ws: rl_cluster_workspace_bytes(M) bytes, 256-byte aligned.  Bad sizes, a radius that is not positive and finite,
 *   min_points < 1, null pointers or a small workspace -> RL_ERR_ARGS before any launch.
 * rl_scene_labels: per row of prob (V, C) fp32 the argmax (ties to the lowest class, as rl_scene_confusion), conf_out[v] =
 *   that entry divided by the row's sum - fp64, classes in order - rounded once to fp32, labels_out[v] = the argmax, or -1
 *   when the confidence is below min_confidence.                                                                        */
int64_t rl_cluster_workspace_bytes(int64_t M);
int rl_cluster_cells(const float* xyz, int64_t M, float radius, int64_t* dims_out, void* ws, int64_t ws_bytes, void* stream);
int rl_cluster_union(const float* xyz, const int64_t* labels, int64_t M, float radius, const int64_t* ignore, int n_ignore,
                     int key_bits, int64_t min_points, int32_t* instance_out, int64_t* I_out, void* ws, int64_t ws_bytes,
                     void* stream);
int rl_cluster_reduce(const float* xyz, const int64_t* labels, const float* scores, int64_t M, int64_t I, int64_t* classes_out,
                      int32_t* count_out, float* centroid_out, float* lo_out, float* hi_out, float* score_out, void* ws,
                      int64_t ws_bytes, void* stream);
int rl_scene_labels(const float* prob, int64_t V, int C, float min_confidence, int64_t* labels_out, float* conf_out,
                    void* stream);

/* Smoothness-constrained clustering (randlanet/utils/cluster.py: euclidean_clusters(normals=, normal_angle=); Model.
 * predict_instances(normal_angle=); no counterpart in the reference): the components of rl_cluster_union under one more
 * condition on an edge, abs((nx_i*nx_j + ny_i*ny_j) + nz_i*nz_j) >= cos_angle with every operation rounded to fp32 and nothing
 * fused - the normals of two joined points agree, whichever way each one was turned; a zero normal joins nobody - and, with
 * curvature, one more on taking part: a point with curvature[i] > max_curvature takes none and gets -1.  The transitive closure,
 * min_points, the numbering and the cells are those of rl_cluster_union, and the result equals the twin's bit for bit.
 *   normals (M, 3) row-major fp32, finite (the caller checks), used as given; curvature (M) fp32, finite, or NULL for no
 *   maximum (max_curvature is then not looked at); cos_angle in (0, 1], the caller's float32(cos(angle)); max_curvature no NaN.
 * rl_cluster_union_smooth takes the place of rl_cluster_union between rl_cluster_cells and rl_cluster_reduce, which serve both
 * rules.  ws: rl_cluster_smooth_workspace_bytes(M) bytes, 256-byte aligned: the workspace of rl_cluster_workspace_bytes(M), then
 * (nx, ny, nz, 0) of every sorted position, which the scan reads only for a pair that passed the label and the distance
 * test.  Everything else, the errors included, as rl_cluster_union.                                                        */
int64_t rl_cluster_smooth_workspace_bytes(int64_t M);
int rl_cluster_union_smooth(const float* xyz, const int64_t* labels, int64_t M, float radius, const int64_t* ignore,
                            int n_ignore, int key_bits, int64_t min_points, const float* normals, const float* curvature,
                            float cos_angle, float max_curvature, int32_t* instance_out, int64_t* I_out, void* ws,
                            int64_t ws_bytes, void* stream);

/* Density-based clustering (randlanet/utils/cluster.py: euclidean_clusters(min_samples=); Model.predict_instances(min_samples=);
 * no counterpart in the reference): DBSCAN's density condition (Ester et al., KDD 1996) on top of either rule above.
 *   near(i, j)   the plain edge of rl_cluster_union: both points take part, the same label over all 64 bits, d2 <= r2.
 *   support(i)   the number of j with near(i, j), i itself included - always the plain rule, also with normals; a point that
 *                takes no part (label < 0, ignored, curvature above max_curvature) is not counted.
 *   core(i)      i takes part and support(i) >= min_samples (the support kernel stops counting there).
 *   components   the transitive closure of the edges between two core points: the smooth edge with normals, else the plain one.
 *   border       a point that takes part, is not core and has an edge (same rule) to a core point joins the component of
 *                exactly one: the smallest d2, among equal d2 the lowest point index.  It transmits nothing: two components
 *                that share only border points stay two.  Every other point that takes part is noise and gets -1.
 *   min_points applies to a component with its border points; the kept components are numbered in ascending order of their
 *   smallest CORE point index; rl_cluster_reduce's statistics run over all members.  The result is a pure function of the
 *   input and equals the twin's bit for bit.  min_samples = 1 makes every participating point core: rl_cluster_union's result.
 * rl_cluster_union_dense takes the place of rl_cluster_union between rl_cluster_cells and rl_cluster_reduce.  Its arguments
 * are those of rl_cluster_union_smooth - normals == NULL selects the plain rule (curvature must then be NULL too; cos_angle and
 * max_curvature are not looked at) - and min_samples >= 1.  Two launches more than the rule it extends: support before the
 * union, attach (the border rule) after it; one lane per sorted position walks all 27 cells around its own; plain loads and
 * vector stores, no atomics in either.  ws: rl_cluster_dense_workspace_bytes(M, smooth) bytes, smooth = normals != NULL,
 * 256-byte aligned: the workspace of the rule it extends, then support (M) int32 by sorted position and attach (M) int32 by
 * point index.  min_samples < 1 -> RL_ERR_ARGS before any launch; everything else, the errors included, as
 * rl_cluster_union_smooth.                                                                                                */
int64_t rl_cluster_dense_workspace_bytes(int64_t M, int smooth);
int rl_cluster_union_dense(const float* xyz, const int64_t* labels, int64_t M, float radius, const int64_t* ignore,
                           int n_ignore, int key_bits, int64_t min_points, const float* normals, const float* curvature,
                           float cos_angle, float max_curvature, int64_t min_samples, int32_t* instance_out, int64_t* I_out,
                           void* ws, int64_t ws_bytes, void* stream);

/* Keypoints (randlanet/utils/keypoints.py: confidence_peaks; Model.predict_keypoints; no counterpart in the reference): the
 * local maxima of a per-point score over a radius inside a label, each refined to the score-weighted mean of its neighbourhood.
 * A point takes part when its label is >= 0 and not in ignore and its score is >= min_score; near(i, j) is rl_cluster_union's
 * edge rule (same label over all 64 bits, d2 <= r2, un-fused fp32); support(i) counts the participating j near i, i included;
 * a point is live when it takes part with support >= min_points; j beats i when score_j > score_i, or the scores are equal and
 * j < i; a peak is a live point that no other live point near it beats.  Keypoints are numbered in ascending peak index.  The
 * numpy twin is confidence_peaks_host; the result is a pure function of the input and equals the twin's bit for bit.
 *   xyz (M, 3) row-major fp32, every coordinate finite; labels (M) int64; scores (M) fp32, finite and >= 0 (the caller
 *   checks); M < 2^31 - 1.
 * The five calls share one workspace and run in this order on one stream; the host reads back dims (to refuse a grid of 2^16
 * cells or more on an axis and to count the key's bits) and K (to size the outputs), nothing else.
 * rl_keypoints_cells: as rl_cluster_cells - the box of ALL points, the grid of cell edge radius * 1.0625f; dims_out (3) int64
 *   in DEVICE memory.
 * rl_keypoints_sort, key_bits as for rl_cluster_union: cell keys (the sentinel dims_x * dims_y * dims_z for a point that takes
 *   no part), the stable radix sort, then (x, y, z, score) and the low 32 label bits of every sorted position.  ignore:
 *   n_ignore int64 classes in DEVICE memory (NULL with n_ignore = 0); min_score no NaN.
 * rl_keypoints_support: one lane per sorted position walks all 27 cells around its own - 9 rows of contiguous keys, each found
 *   by a binary search - and counts the points near it.
 * rl_keypoints_peaks: the same walk over live candidates, left at the first one that beats the point; the peaks compacted in
 *   ascending point index by a scan; K_out[0] (int64, DEVICE memory) = K.
 * rl_keypoints_refine, K as read back from K_out (K >= 1), radius and min_points as before: one wavefront per keypoint adds its
 *   members - the live points near the peak - one by one in ascending (cell key, point index) in fp64, every product rounded
 *   before it is added: W = sum score_j, S_a = sum score_j * (x_j,a - x_p,a).  index_out (K) int64 the peak's point, classes_out
 *   (K) int64, position_out (K, 3) fp32 = x_p + S / W rounded once (x_p when W == 0), score_out (K) fp32 the peak's score,
 *   mean_score_out (K) fp32 = W / count, count_out (K) int32 the members.  No atomics; no workgroup waits for another one.
 *   ws: rl_keypoints_workspace_bytes(M) bytes (0 for a refused M), 256-byte aligned.  Bad sizes, a radius that is not positive
 *   and finite, min_points < 1, null pointers or a small workspace -> RL_ERR_ARGS before any launch.                        */
int64_t rl_keypoints_workspace_bytes(int64_t M);
int rl_keypoints_cells(const float* xyz, int64_t M, float radius, int64_t* dims_out, void* ws, int64_t ws_bytes, void* stream);
int rl_keypoints_sort(const float* xyz, const int64_t* labels, const float* scores, int64_t M, float min_score,
                      const int64_t* ignore, int n_ignore, int key_bits, void* ws, int64_t ws_bytes, void* stream);
int rl_keypoints_support(const int64_t* labels, int64_t M, float radius, void* ws, int64_t ws_bytes, void* stream);
int rl_keypoints_peaks(const int64_t* labels, int64_t M, float radius, int64_t min_points, int64_t* K_out, void* ws,
                       int64_t ws_bytes, void* stream);
int rl_keypoints_refine(const int64_t* labels, int64_t M, int64_t K, float radius, int64_t min_points, int64_t* index_out,
                        int64_t* classes_out, float* position_out, float* score_out, float* mean_score_out, int32_t* count_out,
                        void* ws, int64_t ws_bytes, void* stream);

/* Normals and curvature (randlanet/utils/normals.py: estimate_normals; Model.predict_scene(normals=k); no counterpart in the
 * reference): per query point the fp64 covariance of its k nearest neighbours, its eigenvector of the smallest eigenvalue and
 * that eigenvalue's share of the trace.  The numpy twin is estimate_normals_host; the result is a pure function of the input
 * and equals the twin's bit for bit.
 *   xyz (M, 3) row-major fp32, every coordinate finite (the caller checks); 3 <= k <= RL_KNN_MAX_K, k <= M < 2^31 - 1.
 *   nbr_idx (Q, k) int64: the idx_out of rl_knn_f32 (B = 1, support = the cloud) for the queries first .. first+Q-1 of the
 *   cloud - ascending by (d2, index), the point itself among them.  Rank order is the order of every sum.
 * Per query, fp64 and nothing fused: mu = (sum of the k rows) / k; C_ab = (sum of (p_j,a - mu_a) * (p_j,b - mu_b)) / k for
 * (00, 01, 02, 11, 12, 22); 6 cyclic Jacobi sweeps over the pairs (0,1), (0,2), (1,2) with A = C, V = I, a pair with A_pq == 0
 * skipped, theta = (A_qq - A_pp) / (2 A_pq), t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c;
 * n = the column of V of the smallest diagonal entry lam (ties to the lowest index), curvature = max(lam, 0) / tr with
 * tr = (A_00 + A_11) + A_22, rounded once to fp32; tr <= 0 (the neighbours coincide) gives n = 0 and curvature = 0.
 * n is negated when s = (n_0 w_0 + n_1 w_1) + n_2 w_2 < 0 with w = viewpoint - p in fp64; without a viewpoint (NULL), or when
 * s == 0, when the first non-zero of (n_2, n_1, n_0) is negative; then rounded to fp32.
 *   viewpoint: 3 floats in DEVICE memory, or NULL.  normals_out (M, 3) and curvature_out (M) fp32: the WHOLE cloud's arrays,
 *   of which this call writes the rows first .. first+Q-1.  cov_out (Q, 6) fp64 or NULL (tests only): C of every query.
 * One launch, one wavefront per 64 queries, one lane per query; k * 768 bytes of LDS; no atomics, a fixed order of every sum.
 * Bad sizes or null pointers -> RL_ERR_ARGS before any launch.                                                       */
int rl_normals(const float* xyz, int64_t M, const int64_t* nbr_idx, int64_t first, int64_t Q, int k, const float* viewpoint,
               float* normals_out, float* curvature_out, double* cov_out, void* stream);

/* Pair counts (randlanet/utils/instance_metrics.py: pair_counts; InstanceEvaluator, Model.evaluate_instances; no counterpart
 * in the reference): the sparse contingency table of two integer id arrays - every pair (a_i, b_i) that occurs, once, in
 * ascending order of (a, b) with -1 first, and how many of the M points carry it.  The numpy twin is pair_counts_host; integer
 * work only, no workgroup waits for another one, the result is a pure function of the input and equals the twin's exactly.
 *   a, b (M) in DEVICE memory, int32 or int64 each (a_bytes, b_bytes = 4 or 8); 1 <= M < 2^31 - 1; 1 <= A, B <= 2^31 - 1.
 *   A value below -1 counts as -1.  A value >= A (>= B) is out of range: it raises the flag and counts as -1.
 * The two calls share one workspace and run in this order on one stream; the host reads back head_out between them - P to
 * size the outputs, the flag to refuse - and nothing else.
 * rl_pairs_sort: one launch forms key = (a + 1) * (B + 1) + (b + 1) as 64 bits and one flag slot per chunk of positions; the
 *   stable radix sort of rl_grid_sort over ceil(bits / 8) digits, bits = the bit length of (A + 1) * (B + 1) - 1 (at least 1);
 *   the heads of the runs of equal keys counted per chunk and prefixed by one workgroup, which also folds the flag slots.
 *   head_out (2) int64 in DEVICE memory: head_out[0] = P, the number of distinct pairs; head_out[1] = 1 when a value was out
 *   of range (the table is then not to be used), else 0.
 * rl_pairs_write, P as read back from head_out[0] (1 <= P <= M): the runs numbered by wavefront ballots in position order;
 *   pa (P), pb (P) int32 the pair of run s, count (P) int64 the distance from its head to the next one (M after the last):
 *   no atomics.  count sums to M.
 *   ws: rl_pairs_workspace_bytes(M) bytes (0 for a refused M), 256-byte aligned.  Bad sizes, id widths other than 4 or 8,
 *   null pointers, a misaligned or small workspace -> RL_ERR_ARGS before any launch.                                   */
int64_t rl_pairs_workspace_bytes(int64_t M);
int rl_pairs_sort(const void* a, int a_bytes, const void* b, int b_bytes, int64_t M, int64_t A, int64_t B, int64_t* head_out,
                  void* ws, int64_t ws_bytes, void* stream);
int rl_pairs_write(int64_t M, int64_t A, int64_t B, int64_t P, int32_t* pa, int32_t* pb, int64_t* count, void* ws,
                   int64_t ws_bytes, void* stream);

/* Oriented boxes (randlanet/utils/boxes.py: instance_boxes; Model.predict_instances(oriented_boxes=True),
 * Model.evaluate_instances(boxes=True); no counterpart in the reference): per id k in [0, I) of an integer id array the count,
 * the axis-aligned box, and center, axes, extent and eigenvalues of the box along the principal axes of the id's points.  The
 * numpy twin is instance_boxes_host; the result is a pure function of the input and equals the twin's bit for bit.
 *   xyz (M, 3) row-major fp32, every coordinate finite (the caller checks); ids (M) in DEVICE memory, int32 or int64
 *   (id_bytes = 4 or 8); 1 <= M < 2^31 - 1; 1 <= I < 2^31 - 1.  An id outside [0, I) belongs to no box.
 * The members of an id are its points in ascending point index.  Every fp64 sum over them runs in one fixed order, a function
 * of their number alone: chunks of 1024 consecutive members; inside a chunk lane l (of 64) adds members l, l + 64, .. in turn
 * from 0.0; the 64 lane sums are folded in halves (s_l += s_(l + h), h = 32 .. 1); the chunk sums of an id are added by the
 * same rule (lane l takes chunks l, l + 64, .., then the fold).  Nothing is fused.
 * The three calls share one workspace and run in this order on one stream; the host reads nothing back.
 * rl_boxes_sort: key = id, or I for an id outside [0, I); the stable radix sort of rl_grid_sort over the bits of I; per id the
 *   first sorted position (a binary search: an id without members is an empty run), its chunks, and their prefix by one
 *   workgroup.
 * rl_boxes_moments: mean = (fixed sum of the coordinates) / n, then C_ab = (fixed sum of (p_a - mean_a) * (p_b - mean_b)) / n
 *   for (00, 01, 02, 11, 12, 22); one wavefront per chunk, then one per id.  mean_out (I, 3) and cov_out (I, 6) fp64, or NULL
 *   (tests only).  An id without members has mean and covariance 0.
 * rl_boxes_fit: the 6 cyclic Jacobi sweeps of rl_normals on C; the eigenvalues in descending order, ties to the lower index;
 *   u, w the columns of the two largest; axis 0 = unit(u), axis 1 = unit(w - dot(axis 0, w) * axis 0), each then negated when
 *   its component of largest magnitude (ties to the lowest index) is negative; axis 2 = unit(axis 0 x axis 1), all in fp64
 *   with unit(a) = a / sqrt(dot(a, a)) by true divisions.  t_a = (dx * axis_a,x + dy * axis_a,y) + dz * axis_a,z with d = p - mean; extent_a = max t_a - min t_a;
 *   center = ((mean + axis_0 * h_0) + axis_1 * h_1) + axis_2 * h_2 with h_a = (min t_a + max t_a) * 0.5; rounded once to fp32.
 *   count_out (I) int32; lo_out, hi_out, center_out, extent_out, eigenvalues_out (I, 3) fp32; axes_out (I, 3, 3) fp32, row a =
 *   axis a.  An id without members: count 0, lo = +inf, hi = -inf, center, extent and eigenvalues 0, the axes the identity.
 *   No atomics anywhere: min and max go through per-chunk partials and a second small reduce.
 *   ws: rl_boxes_workspace_bytes(M, I) bytes (0 for a refused M or I), 256-byte aligned.  Bad sizes, an id width other than 4
 *   or 8, null pointers, a misaligned or small workspace -> RL_ERR_ARGS before any launch.                               */
int64_t rl_boxes_workspace_bytes(int64_t M, int64_t I);
int rl_boxes_sort(const void* ids, int id_bytes, int64_t M, int64_t I, void* ws, int64_t ws_bytes, void* stream);
int rl_boxes_moments(const float* xyz, int64_t M, int64_t I, double* mean_out, double* cov_out, void* ws, int64_t ws_bytes,
                     void* stream);
int rl_boxes_fit(const float* xyz, int64_t M, int64_t I, int32_t* count_out, float* lo_out, float* hi_out, float* center_out,
                 float* axes_out, float* extent_out, float* eigenvalues_out, void* ws, int64_t ws_bytes, void* stream);

/* Statistical outlier removal (randlanet/utils/outliers.py: statistical_outliers; Model.predict_scene(outliers=(k, std_ratio));
 * no counterpart in the reference): PCL's StatisticalOutlierRemoval, Open3D's remove_statistical_outlier.  A point whose mean
 * distance to its k nearest neighbours lies more than std_ratio standard deviations above the cloud's mean of that quantity is
 * removed; the kept points are numbered in ascending index.  The numpy twin is statistical_outliers_host; the result is a pure
 * function of the input and equals the twin's bit for bit.
 *   1 <= k <= RL_KNN_MAX_K - 1 (the search is for k + 1 rows); k + 1 <= M < 2^31 - 1.
 * rl_outliers_mean_distance: d2 (Q, k + 1) fp32 in DEVICE memory, the d2_out of rl_knn_f32 (B = 1, support = the cloud, k + 1
 *   neighbours) for the queries first .. first+Q-1 of the cloud - ascending, the point's own 0 among them.  Per query, fp64 and
 *   nothing fused: m = (sum over ranks 0 .. k of sqrt(d2_j), from 0.0, one by one in rank order) / k - PCL's convention: the
 *   zero is searched for and skipped.  mean_out (M) fp64: the WHOLE cloud's array, of which this call writes the rows
 *   first .. first+Q-1.  One launch, one wavefront per 64 queries, one lane per query; (k + 1) * 256 bytes of LDS.
 * rl_outliers_filter, once mean (M) fp64 is complete: mu = S1 / M with S1 the fixed sum of m, sigma = sqrt(S2 / (M - 1)) with
 *   S2 the fixed sum of (m - mu) * (m - mu), t = mu + std_ratio * sigma (product, then sum); keep_i = (m_i <= t).  "Fixed sum" is
 *   the order of rl_boxes_moments for one id whose members are points 0 .. M-1: chunks of 1024, lane l adds members l, l + 64,
 *   .. from 0.0, the 64 lane sums folded in halves, the chunk sums by the same rule.  std_ratio: finite, >= 0.
 *   keep_out (M) uint8 0 / 1; slot_out (M) int32, the position of a kept point among the kept ones, -1 for a removed one;
 *   kept_out (M) int64, of which the first M' entries are written: the kept points in ascending index; stats_out (4) fp64 in
 *   DEVICE memory: mu, sigma, t and M' (as a double).  Seven launches: per sum one wavefront per chunk and one wavefront over
 *   the chunk sums, then counts per chunk by ballot, their prefix by one workgroup, and the write.  No atomics, no workgroup
 *   waits for another one.
 *   ws: rl_outliers_workspace_bytes(M) bytes (0 for a refused M: below 2 or above 2^31 - 2), 256-byte aligned.
 * Bad sizes, a std_ratio that is negative or not finite, null pointers, a misaligned or small workspace -> RL_ERR_ARGS before
 * any launch.                                                                                                           */
int64_t rl_outliers_workspace_bytes(int64_t M);
int rl_outliers_mean_distance(const float* d2, int64_t M, int64_t first, int64_t Q, int k, double* mean_out, void* stream);
int rl_outliers_filter(const double* mean, int64_t M, double std_ratio, uint8_t* keep_out, int32_t* slot_out, int64_t* kept_out,
                       double* stats_out, void* ws, int64_t ws_bytes, void* stream);
/* The two halves of rl_outliers_filter on their own, for a caller that times them or wants the threshold alone; the same
 * arguments, workspace and refusals.  rl_outliers_threshold: the four launches of the two sums; writes stats_out[0 .. 2] and
 * keeps them in ws.  rl_outliers_compact, after it on the same stream and workspace: the three launches of the mask and the
 * compaction; writes keep_out, slot_out, kept_out and stats_out[3].                                                    */
int rl_outliers_threshold(const double* mean, int64_t M, double std_ratio, double* stats_out, void* ws, int64_t ws_bytes,
                          void* stream);
int rl_outliers_compact(const double* mean, int64_t M, uint8_t* keep_out, int32_t* slot_out, int64_t* kept_out,
                        double* stats_out, void* ws, int64_t ws_bytes, void* stream);

/* Depth frames to points (randlanet/utils/depth.py: deproject, TemporalFilter, depth_points; Model.predict_depth; the
 * reference does this stage on the host, camera/realsense_camera.py:90-125): the arithmetic between a depth camera's raw z16
 * frame and the cloud.  The numpy twins are deproject_host and TemporalFilter's host path; the result is a pure function of
 * the inputs and equals the twins' bit for bit - every operation below is one correctly rounded fp32 operation.
 *   depth (H, W) uint16 in DEVICE memory, row-major, 2-byte aligned (a frame of a batch need not be 16-byte aligned);
 *   1 <= W, H and W * H < 2^31; stride >= 1; fx, fy, depth_scale finite and > 0; ppx, ppy finite; z_lo < z_hi.
 *   state: null, or the (H, W) uint16 state of the temporal filter in DEVICE memory (all 0 before the first frame), updated
 *   in place, exactly once.  Per pixel with current value c and state p: c == 0 -> output 0, state unchanged; p == 0 -> output
 *   c, state c; |c - p| < delta -> f = (alpha * c + one_minus_alpha * p) + 0.5, output min(65535, trunc(f)), state that;
 *   otherwise output c, state c.  0 < alpha <= 1, 0 <= one_minus_alpha < 1 (the caller's fp32 1 - alpha; not recomputed),
 *   1 <= delta <= 65535; all three are ignored without a state.  filtered_out: null, or (H, W) uint16 for the outputs.
 *   Pixel (v, u) with output d takes part when v % stride == 0 and u % stride == 0: z = d * depth_scale,
 *   x = (u - ppx) / fx, y = (v - ppy) / fy; with coeffs - five floats in HOST memory (k1, k2, p1, p2, k3), the inverse
 *   Brown-Conrady model; null: pinhole - r2 = x*x + y*y, f = 1 + r2*(k1 + r2*(k2 + r2*k3)),
 *   xd = x*f + ((2*p1)*(x*y) + p2*(r2 + 2*(x*x))), yd = y*f + ((2*p2)*(x*y) + p1*(r2 + 2*(y*y))) replace x and y; the point
 *   is (x*z, y*z, z), kept when d != 0 and z_lo < z and z < z_hi.
 *   xyz_out (W*H, 3) fp32 and pixel_out (W*H) int32, of which the first M rows are written: the kept points in row-major
 *   pixel order and their v * W + u; count_out (1) int64 in DEVICE memory: M.  All three null: the filter alone (a state is
 *   then required), one launch.  Otherwise three launches: counts per chunk of 1024 pixels (the filtered value is recomputed,
 *   the state is not written), their prefix by one workgroup, and the write (state, filtered frame, points).  No atomics, no
 *   workgroup waits for another one.
 *   ws: rl_depth_workspace_bytes(W * H) bytes (0 for a refused size), 256-byte aligned; not read for the filter alone.
 * Bad sizes or parameters, null or odd pointers, a misaligned or small workspace -> RL_ERR_ARGS before any launch.        */
int64_t rl_depth_workspace_bytes(int64_t pixels);
int rl_depth_points(const uint16_t* depth, uint16_t* state, uint16_t* filtered_out, int W, int H, int stride, float fx, float fy,
                    float ppx, float ppy, float depth_scale, const float* coeffs, float alpha, float one_minus_alpha, int delta,
                    float z_lo, float z_hi, float* xyz_out, int32_t* pixel_out, int64_t* count_out, void* ws, int64_t ws_bytes,
                    void* stream);

/* RANSAC plane segmentation (randlanet/utils/planes.py: fit_plane, segment_planes; Model.predict_scene(remove_planes=...); no
 * counterpart in the reference): PCL's SACSegmentation with SACMODEL_PLANE, Open3D's segment_plane.  T planes through three
 * points each are scored by the number of points within `threshold` of them, and the first maximum wins.  The numpy twin is
 * fit_plane_host; every result is a pure function of the inputs and equals the twin's bit for bit - every operation below is
 * one correctly rounded fp32 operation, nothing fused, and the scores are integers.
 *   3 <= M < 2^31 - 1; 1 <= T <= RL_PLANES_MAX_HYPOTHESES; threshold finite and > 0.  xyz (M, 3) fp32 in DEVICE memory.
 * rl_planes_hypotheses: triples (T, 3) int64 in DEVICE memory.  Hypothesis t from the rows p0, p1, p2 of its triple:
 *   e1 = p1 - p0, e2 = p2 - p0, c = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x), l2 = (cx*cx + cy*cy) + cz*cz,
 *   n = c / sqrt(l2) (a correctly rounded root, a true division per component), d = -((nx*p0x + ny*p0y) + nz*p0z).  It is valid
 *   iff l2 > 0 and l2 is finite, and - with axis: three floats in HOST memory, a unit vector; null: no such rule -
 *   |(nx*ax + ny*ay) + nz*az| >= cos_min (0 <= cos_min <= 1; ignored without an axis).  planes_out (T, 4) fp32, 16-byte
 *   aligned: [nx, ny, nz, d], four NaNs for an invalid hypothesis.  A triple with an index outside [0, M) reads nothing, is
 *   invalid, and sets bad_out (1) int32 in DEVICE memory to 1 (0 otherwise): the caller reads it with the result and raises.
 *   One launch of one workgroup.
 * rl_planes_count: planes (T, 4) fp32 as above.  Point i is an inlier of a plane iff |((nx*x_i + ny*y_i) + nz*z_i) + d|
 *   <= threshold (a NaN compares false).  counts_out (T) int32: the inliers of every plane; best_out (2) int32 in DEVICE
 *   memory: the index of the first maximum of counts and that maximum, or -1 and 0 when no plane has an inlier.  Three
 *   launches: the T * M tests - one wavefront per 128 planes and chunk of points, the counts per chunk into a table in ws -,
 *   the table's column sums, and the maximum by one workgroup.
 * rl_planes_split: the points NOT on one plane, numbered in ascending index.  plane: with best null, four floats [nx, ny, nz,
 *   d]; with best (the best_out above) row best[0] of the (T, 4) array `plane`, four NaNs - no inlier - when best[0] < 0.
 *   inlier_out (M) uint8 0 / 1; slot_out (M) int32, the position of a kept point among the kept ones, -1 for a plane point;
 *   kept_out (M) int64, of which the first M' entries are written; n_out (1) int64 in DEVICE memory: M'.  Three launches:
 *   counts per chunk of 1024 points by ballot, their prefix by one workgroup, and the write.
 *   ws: rl_planes_workspace_bytes(M, T) bytes (0 for a refused M or T), 256-byte aligned, at most 4 * max(2^20, 8 * T) + 4 *
 *   ceil(M / 1024) + 512 bytes; rl_planes_split needs those of T = 1 only, which every larger T includes.
 * No atomics, no workgroup waits for another one.  Bad sizes, a threshold that is not finite or <= 0, null or misaligned
 * pointers, a misaligned or small workspace -> RL_ERR_ARGS before any launch.                                            */
#define RL_PLANES_MAX_HYPOTHESES 65536
int64_t rl_planes_workspace_bytes(int64_t M, int64_t T);
int rl_planes_hypotheses(const float* xyz, int64_t M, const int64_t* triples, int64_t T, const float* axis, float cos_min,
                         float* planes_out, int32_t* bad_out, void* stream);
int rl_planes_count(const float* xyz, int64_t M, const float* planes, int64_t T, float threshold, int32_t* counts_out,
                    int32_t* best_out, void* ws, int64_t ws_bytes, void* stream);
int rl_planes_split(const float* xyz, int64_t M, const float* plane, const int32_t* best, float threshold,
                    uint8_t* inlier_out, int32_t* slot_out, int64_t* kept_out, int64_t* n_out, void* ws, int64_t ws_bytes,
                    void* stream);

/* Rigid registration by iterative closest point (randlanet/utils/registration.py: icp, evaluate_registration;
 * Model.predict_views; no counterpart in the reference): PCL's IterativeClosestPoint, Open3D's registration_icp.  One
 * evaluation of a transform T = [R | t] moves the source by it, pairs every moved point with its exact nearest neighbour in the
 * target (rl_knn_f32 with B = 1, k = 1), and sums the 29 fp64 terms of the linearised problem over the pairs inside the gate;
 * the 6x6 solve and the update of T are the host's.  The numpy twin is icp_host; every result is a pure function of the inputs
 * and equals the twin's bit for bit - nothing is fused.
 *   1 <= Ms < 2^31 - 1 source points, 1 <= Mt < 2^31 - 1 target points; src (Ms, 3), target (Mt, 3), normals (Mt, 3) row-major
 *   fp32 in DEVICE memory.
 * rl_icp_transform: rt, twelve floats in HOST memory: R row-major, then t.  q = ((R_a0*x + R_a1*y) + R_a2*z) + t_a per row a,
 *   one correctly rounded fp32 operation at a time.  q_out (Ms, 3) fp32: the WHOLE cloud's array, of which this call writes the
 *   rows first .. first+Q-1.  One launch, one lane per point.
 * rl_icp_sums: q as above; idx (Q, 1) int64 and d2 (Q, 1) fp32, the outputs of rl_knn_f32 for the queries q[first .. first+Q-1]
 *   in the target.  The rows start at a multiple of 1024 and end at one or at Ms.  Pair i is VALID iff d2_i <= gate2 (finite,
 *   > 0).  In fp64, every product rounded before it is added: p = q_i, y = target[idx_i], n = normals[idx_i], d = p - y,
 *   r = (d0*n0 + d1*n1) + d2*n2, J = (p1*n2 - p2*n1, p2*n0 - p0*n2, p0*n1 - p1*n0, n0, n1, n2); the 29 columns are the 21
 *   products J_u*J_v (u <= v, row-major upper triangle), the 6 products J_u*r, r*r, and d2_i.  metric 0 (point to plane): as
 *   written.  metric 1 (point to point; normals may be NULL): the same rule for n = e_0, e_1, e_2, the three results added per
 *   column as (c^0 + c^1) + c^2, d2_i once.  An invalid pair adds +0.0 to every column, so the order of every sum is a function
 *   of Ms alone: the fixed sum of rl_boxes_moments for one id whose members are source points 0 .. Ms-1 - chunks of 1024, lane l
 *   adds members l, l + 64, .. from 0.0, the 64 lane sums folded in halves.  One launch, one wavefront per chunk: the chunk's
 *   29 sums and its number of valid pairs go to ws; corr_out (Ms) int64, the WHOLE cloud's array, receives idx_i or -1 (an
 *   invalid pair) for the rows of this call.  An idx outside [0, Mt) reads row 0 and is invalid.
 * rl_icp_fold, once every chunk's rl_icp_sums ran on the same stream and workspace: the chunk sums by the same rule (lane l
 *   takes chunks l, l + 64, .., then the fold), one wavefront per column in one launch; the counts as an integer sum.  out (30)
 *   fp64 in DEVICE memory: the number of valid pairs (as a double: exact), then the 29 sums.
 *   ws: rl_icp_workspace_bytes(Ms) bytes (0 for a refused Ms), 256-byte aligned: 236 bytes per chunk.
 * No atomics, no workgroup waits for another one.  Bad sizes, a gate that is not finite and positive, a metric other than 0 or
 * 1, null pointers (normals with metric 1 excepted), misaligned rows, a misaligned or small workspace -> RL_ERR_ARGS before any
 * launch.                                                                                                               */
int64_t rl_icp_workspace_bytes(int64_t Ms);
int rl_icp_transform(const float* src, int64_t Ms, int64_t first, int64_t Q, const float* rt, float* q_out, void* stream);
int rl_icp_sums(const float* q, const float* normals, const float* target, int64_t Mt, const int64_t* idx, const float* d2,
                int64_t Ms, int64_t first, int64_t Q, float gate2, int metric, int64_t* corr_out, void* ws, int64_t ws_bytes,
                void* stream);
int rl_icp_fold(int64_t Ms, double* out, void* ws, int64_t ws_bytes, void* stream);

/* Fast point feature histograms and their matching (randlanet/utils/features.py: fpfh, match_features; no counterpart in the
 * reference): PCL's FPFHEstimation, Open3D's compute_fpfh_feature, with the third angle replaced by its diamond pseudo-angle.
 * The numpy twins are fpfh_host and match_features_host, whose module docstring is the contract: fp32, one correctly rounded
 * operation at a time, nothing fused, true division and square root, no libm; every result equals the twin's bit for bit.
 *   2 <= k <= RL_KNN_MAX_K - 1; k + 1 <= M < 2^31 - 1.  xyz, normals (M, 3) fp32; idx (Q, k + 1) int64 and d2 (Q, k + 1) fp32:
 *   the outputs of rl_knn_f32 for the queries first .. first+Q-1 of the cloud in itself (B = 1, k + 1 rows).  All in DEVICE
 *   memory.  An idx outside [0, M) is skipped and nothing is read for it.
 * rl_fpfh_spfh: spfh_out (M, 33) uint8, the WHOLE cloud's array, of which this call writes the rows first .. first+Q-1: the
 *   counts of the three pair features over the ranks 1 .. k, 11 bins each.  One launch, one wavefront per point.
 * rl_fpfh_fpfh, once rl_fpfh_spfh wrote every row: desc_out (M, 33) fp32 and code_out (M, 36) uint8, the WHOLE cloud's arrays,
 *   rows first .. first+Q-1: the 1 / d2-weighted sums of the neighbours' SPFH rows in rank order, each sub-histogram scaled to
 *   100, and its quantisation min(255, trunc(F * 2.55 + 0.5)) with three zero bytes behind.  One launch, one wavefront per point.
 * rl_match_u8: code_source (Ms, 36) and code_target (Mt, 36) uint8, 4-byte aligned; 1 <= Ms, Mt < 2^31 - 1.  idx_out (Ms) int64
 *   and dist_out (Ms) int32: the target row of the smallest sum of squared byte differences and that sum, ties to the lowest
 *   index.  Three launches: the targets' norms, Ms * Mt * 9 packed byte dot products over (64 sources, slice of targets) per
 *   wavefront, and the lexicographic minimum over the slices.  ws: rl_match_workspace_bytes(Ms, Mt) bytes (0 for refused
 *   sizes), 256-byte aligned: 4 * Mt + 8 * Ms * slices + 768 at most, slices <= 64.
 * No atomics, no workgroup waits for another one.  Bad sizes, null or misaligned pointers, a misaligned or small workspace
 * -> RL_ERR_ARGS before any launch.                                                                                       */
int rl_fpfh_spfh(const float* xyz, const float* normals, int64_t M, const int64_t* idx, const float* d2, int64_t first, int64_t Q,
                 int k, uint8_t* spfh_out, void* stream);
int rl_fpfh_fpfh(const uint8_t* spfh, int64_t M, const int64_t* idx, const float* d2, int64_t first, int64_t Q, int k,
                 float* desc_out, uint8_t* code_out, void* stream);
int64_t rl_match_workspace_bytes(int64_t Ms, int64_t Mt);
int rl_match_u8(const uint8_t* code_source, int64_t Ms, const uint8_t* code_target, int64_t Mt, int64_t* idx_out,
                int32_t* dist_out, void* ws, int64_t ws_bytes, void* stream);

/* RANSAC over correspondences (randlanet/utils/registration.py: global_registration; Model.predict_views(global_init=...); no
 * counterpart in the reference): PCL's SampleConsensusPrerejective, Open3D's registration_ransac_based_on_feature_matching.
 * The numpy twin is global_registration_host, whose module docstring is the contract; every result equals it bit for bit.
 *   3 <= C < 2^31 - 1 correspondences (c, corr[c]): source (C, 3) and target (Mt, 3) fp32, corr (C) int64 in [0, Mt);
 *   1 <= T <= RL_GLOBAL_MAX_HYPOTHESES.  All arrays in DEVICE memory unless said otherwise.
 * rl_global_hypotheses: triples (T, 3) int64 in [0, C); s2 in [0, 1], the squared edge similarity.  hyp_out (T, 12) fp32: R
 *   row-major, then t, of the transform that maps the triangle of the three source points onto that of their target points,
 *   or twelve NaNs for a hypothesis that fails the edge test or has a non-finite entry.  An index outside its range reads
 *   nothing, gives NaNs and sets bad_out (1) int32 to 1 (0 otherwise).  Two launches: one lane per hypothesis, and the flag.
 * rl_global_count: hyp (T, 12) as above; correspondence c is an inlier of a hypothesis iff |R a_c + t - b_c|^2 <= gate2
 *   (finite, > 0; fp32, un-fused).  counts_out (T) int32.  Three launches: the rows [a_c | b_c], the T * C tests - one
 *   wavefront per 128 hypotheses and chunk of correspondences, the counts per chunk into a table in ws -, the column sums.
 * rl_global_sums: rt, twelve floats in HOST memory as above.  inlier_out (C) uint8 0 / 1 by the same rule; out (16) fp64: the
 *   fixed sums (rl_icp_sums' order: chunks of 1024) over the inliers of 1, a (3), b (3), a_u * b_v (9, u-major) in fp64.  Two
 *   launches: one wavefront per chunk, one per column.
 *   ws: rl_global_workspace_bytes(C, T) bytes (0 for refused sizes), 256-byte aligned; rl_global_sums needs those of T = 1.
 * No atomics, no workgroup waits for another one.  Bad sizes, a bad gate or s2, null pointers, a misaligned or small
 * workspace -> RL_ERR_ARGS before any launch.                                                                             */
#define RL_GLOBAL_MAX_HYPOTHESES 1048576
int64_t rl_global_workspace_bytes(int64_t C, int64_t T);
int rl_global_hypotheses(const float* source, int64_t C, const float* target, int64_t Mt, const int64_t* corr,
                         const int64_t* triples, int64_t T, float s2, float* hyp_out, int32_t* bad_out, void* ws,
                         int64_t ws_bytes, void* stream);
int rl_global_count(const float* source, int64_t C, const float* target, int64_t Mt, const int64_t* corr, const float* hyp,
                    int64_t T, float gate2, int32_t* counts_out, void* ws, int64_t ws_bytes, void* stream);
int rl_global_sums(const float* source, int64_t C, const float* target, int64_t Mt, const int64_t* corr, const float* rt,
                   float gate2, uint8_t* inlier_out, double* out, void* ws, int64_t ws_bytes, void* stream);

/* TSDF fusion of depth frames (randlanet/utils/tsdf.py: TsdfVolume, DepthFusion; no counterpart in the reference, whose camera
 * loop predicts on single frames): KinectFusion's volume, Open3D's TSDFVolume.  A dense volume of nx * ny * nz voxels of edge
 * `voxel` whose minimum corner is `origin`: two fp32 arrays tsdf and weight of shape (nz, ny, nx), x fastest, in DEVICE memory,
 * 4-byte aligned (16-byte aligned arrays are read and written 16 bytes at a time); all 1.0 and all 0.0 at the start.  Voxel
 * (i, j, k) has the linear index n = (k*ny + j)*nx + i and the centre c_x = ox + ((float)i + 0.5) * voxel, likewise c_y, c_z.
 * The numpy twin is utils/tsdf.py, whose module docstring is the contract; every result is a pure function of the inputs and
 * equals the twin's bit for bit - every operation below is one correctly rounded fp32 operation, nothing fused, true division.
 *   1 <= nx, ny, nz and nx * ny * nz < 2^31; origin: three floats in HOST memory, finite; voxel finite and > 0.
 * rl_tsdf_integrate: one depth frame into the volume.  depth (H, W) uint16 in DEVICE memory, row-major, 2-byte aligned;
 *   1 <= W, H < 2^24 and W * H < 2^31; fx, fy, depth_scale finite and > 0; ppx, ppy finite; z_lo < z_hi; trunc finite and > 0;
 *   1 <= max_weight <= 65535; world_to_camera: twelve finite floats in HOST memory, R' row-major, then t' (rl_icp_transform's
 *   layout).  Per voxel: q_a = ((R'_a0*c_x + R'_a1*c_y) + R'_a2*c_z) + t'_a; skipped unless q_z > 0; uf = ((q_x / q_z) * fx +
 *   ppx) + 0.5, vf = ((q_y / q_z) * fy + ppy) + 0.5; skipped unless 0 <= uf < W and 0 <= vf < H (a NaN or an infinity is
 *   skipped); d = depth[(int)vf, (int)uf]; skipped if d == 0; z = d * depth_scale; skipped unless z_lo < z and z < z_hi;
 *   sdf = z - q_z; skipped if sdf < -trunc; s = min(1, sdf / trunc); with the voxel's weight w: tsdf = (tsdf * w + s) / (w + 1),
 *   weight = min(w + 1, max_weight).  A skipped voxel is not written.  One launch, a lane per run of 4 voxels, no workspace.
 * rl_tsdf_count: the edge 3n + a joins voxel n and its neighbour b one step up along axis a (0, 1, 2 = x, y, z) where that lies
 *   inside the volume; it EMITS a point iff weight[n] >= min_weight and weight[b] >= min_weight and (tsdf[n] < 0) != (tsdf[b] <
 *   0); 1 <= min_weight <= 65535.  count_out (1) int64 in DEVICE memory: M, the number of emitting edges.  Two launches: the
 *   counts per chunk of 1024 voxels, one wavefront each, and their exclusive prefix by one workgroup, both kept in ws.
 * rl_tsdf_points, after rl_tsdf_count on the same stream, workspace, volume and min_weight: count, the M read back, 1 <= count <
 *   2^32 (M = 0 needs no call); xyz_out (capacity, 3) fp32 and edge_out (capacity) int64 with capacity >= count, of which the
 *   first M rows are written, in ascending edge order: f = tsdf[n] / (tsdf[n] - tsdf[b]), the point is the centre of n with
 *   coordinate a replaced by c_a + f * voxel, and edge = 3n + a.  No row at or beyond capacity is written whatever ws holds.
 *   One launch, one wavefront per chunk.
 *   ws: rl_tsdf_workspace_bytes(nx * ny * nz) bytes (0 for a refused size), 256-byte aligned: 4 bytes per chunk.
 * No atomics, no workgroup waits for another one.  Bad sizes or parameters, null or misaligned pointers, a misaligned or small
 * workspace -> RL_ERR_ARGS before any launch.                                                                             */
int64_t rl_tsdf_workspace_bytes(int64_t voxels);
int rl_tsdf_integrate(float* tsdf, float* weight, int nx, int ny, int nz, const float* origin, float voxel, float trunc,
                      int max_weight, const uint16_t* depth, int W, int H, float fx, float fy, float ppx, float ppy,
                      float depth_scale, float z_lo, float z_hi, const float* world_to_camera, void* stream);
int rl_tsdf_count(const float* tsdf, const float* weight, int nx, int ny, int nz, const float* origin, float voxel,
                  int min_weight, int64_t* count_out, void* ws, int64_t ws_bytes, void* stream);
int rl_tsdf_points(const float* tsdf, const float* weight, int nx, int ny, int nz, const float* origin, float voxel,
                   int min_weight, int64_t count, float* xyz_out, int64_t* edge_out, int64_t capacity, void* ws,
                   int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RL_RANDLANET_H */
