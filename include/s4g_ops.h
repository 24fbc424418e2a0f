/*
 * s4g_ops.h -- C ABI of libs4g_hip.so, the MI355X (gfx950) replacement for the
 * reference's pybind11 extension `pn2_ext`.
 *
 * Reference interface replaced (paths relative to
 * /root/reference/inference/grasp_proposal/network_models/models/pointnet2_utils/):
 *   csrc/main.cpp:6-14 registers seven at::Tensor functions; each entry point
 *   below cites the prototype it replaces.  The reference's Python wrappers
 *   (functions.py:42,72,99,105,127,163,170) are the only callers.
 *
 * Conventions (all entry points):
 *   - extern "C", plain device pointers and int64 sizes, no torch types.
 *   - return 0 on success, <0 = S4G_E* argument error (nothing launched),
 *     >0 = hipError_t from the launch.  No exceptions, no allocation, no
 *     host synchronisation, no global state; re-entrant.
 *   - the caller owns every buffer (outputs and workspace) and passes the HIP
 *     stream to launch on (hipStream_t as void*; NULL = default stream) --
 *     the reference launches on the legacy default stream with no guard.
 *   - clouds are channel-first fp32 exactly as the Python API hands them over,
 *     (B,3,N) contiguous; the reference's internal (B,N,3) transposed copies
 *     (sampling_kernel.cu:141, ball_query_kernel.cu:105-106,
 *     interpolate_kernel.cu:111-112) are not made.
 *   - indices are int64 as in the reference (AT kLong outputs).
 *   - `flags`: bit 0 (S4G_FLAG_FMAD) selects the distance arithmetic.
 *       0: every fp32 op rounded separately, d = ((dx*dx)+(dy*dy))+(dz*dz)
 *          (canonical; what the oracle and all parity tests use)
 *       1: emulate nvcc's default -fmad contraction,
 *          d = fma(dz,dz, fma(dy,dy, dx*dx)).
 */
#ifndef S4G_OPS_H_
#define S4G_OPS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1: operators; 2: f16x2 contraction fields, crop / voxel / outlier / grid 3-NN / _ws entry points;
 * 3: fused layer chains (W2 / W3 fields), GATHER_ADD / INTERP_ADD loaders, s4g_interp_add_cl_f32,
 *    s4g_group_points_ws_f32, device-side cell choice of s4g_three_nn_grid_f32 (cell < 0).
 * 4: per-scene activation maxima (rows_per_scene), bf16 chains, s4g_heads_chain_f32.
 * 5: s4g_group_rel_xyz_i32 and the rel_xyz4 field of s4g_gemm_desc_t.
 * 6: pre_* members of s4g_heads_desc_t (the last FP level's tail in front of the heads).
 * 7: s4g_fps_gather_ex_i32, s4g_fps_prefix_check_f32, s4g_fps_prepass_f32 (no layout change).
 * 8: s4g_group_rel_xyz_unique_i32 and the seg4 / seg_rows fields of s4g_gemm_desc_t (the first SA level
 *    contracts a centroid's distinct rows only); out2 / ldc2 / split_n / out_amax2 (two layers that read the
 *    same tensor as one launch); the operators in double (*_f64); s4g_build_variants.
 * 9: s4g_heads_desc_t.out_batch_stride (the four heads written as channel slices of one packed
 *    (B, 21, N) tensor: the all-gather payload of the multi-GPU path without a packing copy).
 * 10: s4g_group_points_backward_det_f32 / s4g_three_interpolate_backward_det_f32 / s4g_scatter_det_workspace_bytes
 *    (the backward scatters in a fixed order: run-to-run bit-identical, equal to the oracle's sequential sum).
 * 11: s4g_heads_desc_t.head_mask (a launch may evaluate a subset of the four heads).
 * 12: s4g_test_knobs_enabled (the A/B knobs below are ignored without S4G_TEST_KNOBS=1; no layout change),
 *     s4g_collision_counts_n_f32 (collision counts over padded best-first pose lists with device-side counts),
 *     s4g_sort_pairs_u32 / s4g_exclusive_scan_i32 (the library's own stable radix sort and scan).
 * 13: s4g_contact_heads_f32 (output tail of the contact network, MODEL.TYPE "PN2"), s4g_decode_poses_abs_f32
 *     (pose decode for an absolute translation head); no layout change.
 * 14: S4G_GEMM_LOAD_CHANNEL_FIRST, S4G_GEMM_EPI_MAX_CHANNEL_FIRST and s4g_gemm_desc_t.a_L (any SharedMLP / SA max-pool
 *     on its own (B, C, L) tensors: s4g_release_amd.accelerate), s4g_amax_per_scene_f32.
 *     s4g_gemm_desc_t.cbias (a per-centroid bias of the GATHER_ADD loader: the edge levels of MODEL.TYPE "EDGEPN2D";
 *     NULL behaves as before the member existed; it sits in front of a_L, whose offset grew by 8).
 *     Added under 14 with no layout change: s4g_eval_frames_f32 / s4g_eval_frames_workspace_bytes (batched antipodal
 *     and collision grading of grasp frames against a labelled scene cloud with normals); s4g_local_search_f32 /
 *     s4g_local_search_workspace_bytes (the data generator's per-frame local grasp search); s4g_darboux_frames_f32 /
 *     s4g_darboux_frames_workspace_bytes (the Darboux frames that search starts from); s4g_match_normals_f32 /
 *     s4g_match_normals_workspace_bytes (the scene normals a view's points take over in front of those frames);
 *     s4g_contact_search_f32 / s4g_contact_search_workspace_bytes (the contact model's grading of every scene frame),
 *     s4g_match_nearest_f32 (the nearest scene point of every view point) and s4g_contact_select_f32 (the contact
 *     model's per-view-point normal and best frame); s4g_best_placement_f32 (the best placement of that search per
 *     frame and its global -> local matrix), s4g_close_region_f32 / s4g_close_region_workspace_bytes (the packed
 *     close-region point sets and 12-channel projection maps the GPD and PointNetGPD baselines read);
 *     s4g_gpd_pack_f32 / s4g_gpd_pack_bytes / s4g_gpd_forward_f32 / s4g_gpd_workspace_bytes (the GPD baseline's
 *     classifier on those maps: two 5x5 convolutions with max-pools on the matrix cores and two linear layers);
 *     s4g_pngpd_pack_f32 / s4g_pngpd_pack_bytes / s4g_pngpd_forward_f32 / s4g_pngpd_workspace_bytes (the PointNetGPD
 *     baseline's classifier on the packed close-region point sets, or on dense (G, 3, n) sets: two per-point trunks
 *     with a segment maximum and the per-set layers on the matrix cores); s4g_estimate_normals_f32 /
 *     s4g_estimate_normals_workspace_bytes (PCA normals of a cloud that has none: the input of all of the above for a
 *     sensor cloud); s4g_contact_pairs_f32 / s4g_contact_pairs_workspace_bytes (the antipodal point pairs of an
 *     object cloud) and s4g_contact_pair_grade_f32 / s4g_contact_pair_grade_workspace_bytes (their rolled frames
 *     graded over that cloud, the kept frames and the object point of each: the per-object data the contact model's
 *     scenes are composed from); s4g_darboux_object_frames_f32 / s4g_darboux_object_frames_workspace_bytes (every
 *     object point's Darboux frame and opposite frame) and s4g_darboux_object_grade_f32 /
 *     s4g_darboux_object_grade_workspace_bytes (both graded over the object's own cloud: the per-object data the
 *     curvature model's scenes are composed from); s4g_precomputed_select_f32 (every view point's frame, scores and
 *     recommended placements looked up at its nearest point of such a scene) and s4g_precomputed_search_f32 /
 *     s4g_precomputed_search_workspace_bytes (the collision check of the recommended placements against the dense
 *     scene: the view stage of the curvature model's fast label pipeline);
 *     s4g_precomputed_baseline_search_f32 / s4g_precomputed_baseline_search_workspace_bytes (the same collision check
 *     without the label gate and the best-placement fold: the fast baseline labels GPD and PointNetGPD are trained on);
 *     s4g_process_views_f32 / s4g_process_views_workspace_bytes (crop, voxel trace and radius-outlier removal of B
 *     rendered views: the processed cloud and the reference index every view-stage call above starts from);
 *     s4g_eval_view_search_f32 / s4g_eval_view_search_workspace_bytes (the first collision-free placement of every
 *     frame of a view against the view itself) and s4g_eval_scene_grade_f32 / s4g_eval_scene_grade_workspace_bytes
 *     (its ground truth against the dense labelled scene: the data GPD and PointNetGPD are evaluated on);
 *     s4g_contact_refine_f32 / s4g_contact_refine_workspace_bytes (the per-object frames of s4g_contact_pair_grade_f32
 *     re-graded over the object's cloud under shifted placements, and the kept rows), s4g_match_knn_f32 (the nearest
 *     points of every point of a cloud, the indices alone) and s4g_contact_reduce_i32 (the per-point cap of those
 *     frames with the surplus handed to neighbouring points: the refine and reduce stages between the per-object data
 *     and the contact model's scenes); s4g_render_views_f32 / s4g_render_views_workspace_bytes (the rendered views
 *     themselves: pinhole range images of posed triangle meshes and the noise-free and noisy clouds
 *     s4g_process_views_f32 and its trace start from). */
#define S4G_ABI_VERSION 14

/* ---------------------------------------------------------------------------
 * Environment variables.
 *
 * PRODUCTION SURFACE -- the only variables the shipped library and its Python host read on their own (7):
 *   S4G_TEST_KNOBS=1               master switch for everything in the second list (library and host side)
 *   S4G_HIP_LIB=path               load another build of this library (warns; tools/ab_libs.sh)
 *   S4G_GEMM_MODE=f16x2|bf16x3|fp32|bf16   default contraction arithmetic of FusedPointNet2 (constructor argument wins)
 *   S4G_DIST_MODE=fmad             distance arithmetic contract (S4G_FLAG_FMAD) instead of strict
 *   S4G_BACKWARD=atomic            group_points / three_interpolate backward through the atomicAdd kernels (the
 *                                  reference's scheme, order undefined) instead of the deterministic sorted-segment sums
 *   S4G_GEO_STREAMS=n, S4G_DENSE_STREAMS=n   geometry / contraction streams of the pipeline (2 / 1)
 *  (bench.py reads S4G_BENCH_FORCE_DIST, S4G_BENCH_TIMER_EVERY, NCCL_MAX_NCHANNELS, and for tests/test_bench_world.py
 *   S4G_BENCH_BACKEND=gloo; the oracle reads S4G_ORACLE_LIB / S4G_ORACLE_F64 -- test infrastructure, not the product.)
 *
 * A/B AND TEST KNOBS -- IGNORED unless the process sets S4G_TEST_KNOBS=1 (tests/conftest.py does; tools that set one set
 * it too; s4g_test_knobs_enabled() says whether they are honoured).  Round 6: a stray
 * variable in a launcher's environment can no longer change which kernel a production rank runs.  Every alternative is
 * exact (same results; the defaults are the measured-fastest paths), so the switch can change speed, never values.
 *  library side (s4g::knob in csrc/s4g_common.h; per call unless noted):
 *   S4G_FPS_MODE=dense|pruned      FPS kernel for N <= 25 600: full scan | group-pruned (default: pruned
 *                                  above 10 240 points, and above 5 120 when M >= 2 048).  =dense also turns the L2-resident pruned kernel
 *                                  off for 25 600 < N <= 65 535 (the streaming kernel runs instead)
 *   S4G_BQ_MODE=scan|grid          ball query path (default: grid from 8 192 points)
 *   S4G_NN_SPLIT=0                 3-NN: never the split scan for 24 <= N2 <= 2 048
 *   S4G_INTERP_MODE=lane           three_interpolate: lane-per-point kernel instead of the LDS tile
 *   S4G_GEMM_SINGLE_CHAIN=0|1      plain single layers never / wherever supported on mlp_chain_kernel's first-layer
 *                                  form (default: where it measured faster: Cout >= 1024 or K >= 1024)
 *   S4G_MLP1_MFMA=0                first SA level's 3 -> C layer on the vector ALU (the chain kernel's loader) instead of
 *                                  one MFMA step inside the chain kernel (f16x2 form with rel_xyz4 records)
 *  host side (_cabi.knob; read when a FusedPointNet2 is built / an operator is called):
 *   S4G_SA_UNIQUE=0                first SA level contracts all K rows, padding copies included
 *   S4G_REL_XYZ=0                  first SA level's loader follows the indices itself
 *   S4G_SA_LINEAR_FIRST=0, S4G_FP_LINEAR_FIRST=0   no linear-layer-before-grouping / -interpolation
 *   S4G_FP_CHAIN_NEXT=0            the next FP level's linear-first layer as a launch of its own
 *   S4G_GEMM_FUSE2=0               layer chains as separate launches
 *   S4G_MERGE_SHARED=0             sa{l}.0f and fp{f}.0d (same input tensor) as two launches instead of one
 *   S4G_HEADS_PRE=0                FP tail outside the heads launch
 *   S4G_FPS_PREFIX=0               always sample SA levels 2 and 3 (no prefix proof)
 *   S4G_NN_MODE=scan               3-NN: never the cell-grid search
 *   S4G_PACKED_OUT=0               FusedPointNet2 returns four head tensors of their own instead of channel slices of one
 *                                  packed (B, 21, N) tensor
 * ------------------------------------------------------------------------- */

#define S4G_OK 0
#define S4G_EINVAL (-1)     /* bad size / null pointer */
#define S4G_EWORKSPACE (-2) /* workspace too small */
#define S4G_EUNSUPPORTED (-3)

#define S4G_FLAG_FMAD 1

typedef void *s4g_stream_t; /* hipStream_t */

/* operator ids for s4g_workspace_bytes */
#define S4G_OP_FPS 1
#define S4G_OP_BALL_QUERY 2
#define S4G_OP_THREE_NN 3

int s4g_abi_version(void);
/* ABI >= 8.  Always 0: the library carries no kernel variants; kept because the symbol is part of the ABI. */
int s4g_build_variants(void);
/* 1 when the A/B / test knobs listed above are honoured in this process (S4G_TEST_KNOBS=1 in the environment);
 * 0: the library ignores every one of them. */
int s4g_test_knobs_enabled(void);
const char *s4g_error_string(int code);

/* Bytes of device scratch an operator needs for the given problem
 * (0 if none).  dims: FPS (B,N,M,0); BALL_QUERY (B,N,M,K); THREE_NN (B,N1,N2,0). */
size_t s4g_workspace_bytes(int op, int64_t B, int64_t d0, int64_t d1, int64_t d2);

/* FarthestPointSample(points (B,3,N), num_centroids) -> index (B,M) int64
 * replaces csrc/sampling.h:7-9, csrc/sampling_kernel.cu:128-172.
 * Requires M > 0, N >= M (sampling_kernel.cu:137-139).  idx[b,0] = 0. */
int s4g_fps_f32(const float *xyz_b3n, int64_t B, int64_t N, int64_t M,
                int64_t *idx_bm, void *ws, size_t ws_bytes, int flags,
                s4g_stream_t stream);

/* BallQuery(points (B,3,N), centroids (B,3,M), radius, K)
 *   -> index (B,M,K) int64, count (B,M) int64
 * replaces csrc/ball_query.h:7-11, csrc/ball_query_kernel.cu:89-133.
 * Outputs are fully written (rows without any hit are zero, as the
 * reference's at::zeros leaves them). */
int s4g_ball_query_f32(const float *xyz_b3n, const float *ctr_b3m, int64_t B,
                       int64_t N, int64_t M, float radius, int64_t K,
                       int64_t *idx_bmk, int64_t *cnt_bm, void *ws,
                       size_t ws_bytes, int flags, s4g_stream_t stream);

/* GroupPointsForward(input (B,C,N), index (B,M,K)) -> (B,C,M,K)
 * replaces csrc/grouping.h:7-9, csrc/grouping_kernel.cu:32-54. */
int s4g_group_points_f32(const float *in_bcn, const int64_t *idx_bmk, int64_t B,
                         int64_t C, int64_t N, int64_t M, int64_t K,
                         float *out_bcmk, s4g_stream_t stream);

/* GroupPointsBackward(grad_output (B,C,M,K), index, N) -> grad_input (B,C,N)
 * replaces csrc/grouping.h:11-14, csrc/grouping_kernel.cu:106-152.
 * grad_in is zeroed by the call, then scatter-added (fp32 atomics). */
/* group_points for C == 3 (the xyz grouping of QueryGrouper, modules.py:42) through an
 * index-ordered (x, y, z, 0) copy in `ws` (B * N * 16 bytes): one 16-byte gather per
 * neighbour.  Same output as s4g_group_points_f32(C = 3); without a (large enough,
 * 16-byte aligned) workspace or with M*K % 4 != 0 it IS that call. */
int s4g_group_points_xyz_f32(const float *xyz_b3n, const int64_t *idx_bmk, int64_t B, int64_t N,
                             int64_t M, int64_t K, float *out_b3mk, void *ws, size_t ws_bytes,
                             s4g_stream_t stream);
/* s4g_group_points_f32 through a channels-last copy of the features in `ws` (B * N * C
 * floats): 64 channels of a neighbour are one 256-byte read and the channel-first rows
 * leave as 16-byte stores.  Bit-identical output; without a (large enough, 16-byte
 * aligned) workspace or with C % 4 != 0 it IS that call. */
int s4g_group_points_ws_f32(const float *feat_bcn, const int64_t *idx_bmk, int64_t B, int64_t C,
                            int64_t N, int64_t M, int64_t K, float *out_bcmk, void *ws,
                            size_t ws_bytes, s4g_stream_t stream);
int s4g_group_points_backward_f32(const float *gout_bcmk,
                                  const int64_t *idx_bmk, int64_t B, int64_t C,
                                  int64_t N, int64_t M, int64_t K,
                                  float *gin_bcn, s4g_stream_t stream);

/* gather_points(points (B,C,N), index (B,M)) -> (B,C,M)
 * replaces the torch.gather in functions.py:10-25. */
int s4g_gather_points_f32(const float *in_bcn, const int64_t *idx_bm, int64_t B,
                          int64_t C, int64_t N, int64_t M, float *out_bcm,
                          s4g_stream_t stream);

/* PointSearch(query (B,3,N1), key (B,3,N2), 3)
 *   -> index (B,N1,3) int64, SQUARED distance (B,N1,3) fp32
 * replaces csrc/interpolate.h:8-11, csrc/interpolate_kernel.cu:92-132.
 * Requires N2 >= 3 (interpolate_kernel.cu:106).
 * Out of contract, but contained: a query with a NaN / inf coordinate (or squared distances that all overflow) enters no
 * key at all; the reference then leaves its initialisers -- index -1, distance +inf in slot 0 -- and its consumers read
 * row -1.  Every 3-NN entry point of this library (this one, _i32, _grid, _weights*, _f64) writes index 0 for such a
 * slot and keeps the distance: the interpolation weight of that slot is 0 either way, and nothing downstream can be
 * driven out of bounds by a bad depth pixel (a GPU memory fault takes the process down). */
int s4g_three_nn_f32(const float *q_b3n1, const float *k_b3n2, int64_t B,
                     int64_t N1, int64_t N2, int64_t *idx_bn3, float *d2_bn3,
                     void *ws, size_t ws_bytes, int flags, s4g_stream_t stream);

/* InterpolateForward(input (B,C,N2), index (B,N1,3), weight (B,N1,3))
 *   -> (B,C,N1)
 * replaces csrc/interpolate.h:13-16, csrc/interpolate_kernel.cu:191-236. */
int s4g_three_interpolate_f32(const float *feat_bcn2, const int64_t *idx_bn3,
                              const float *w_bn3, int64_t B, int64_t C,
                              int64_t N2, int64_t N1, float *out_bcn1,
                              int flags, s4g_stream_t stream);

/* InterpolateBackward(grad_output (B,C,N1), index, weight, N2) -> (B,C,N2)
 * replaces csrc/interpolate.h:18-22, csrc/interpolate_kernel.cu:296-341. */
/* s4g_three_interpolate_f32 through a channels-last copy of the sparse features in `ws`
 * (B * N2 * C floats): a quad of channels is one 16-byte gather.  Bit-identical output;
 * without a (large enough, 16-byte aligned) workspace or with C % 4 != 0 it IS that call. */
int s4g_three_interpolate_ws_f32(const float *feat_bcn2, const int64_t *idx_bn3, const float *w_bn3,
                                 int64_t B, int64_t C, int64_t N2, int64_t N1, float *out_bcn1,
                                 void *ws, size_t ws_bytes, int flags, s4g_stream_t stream);
/* Fast path, FP levels: the first shared-MLP layer is linear, so it is applied to the sparse
 * features BEFORE the interpolation (and to the skip features separately); this call then
 * forms out[p][c] = act(y[p][c] + bias[c] + sum_k nw[p][k] * sparse[b*N2 + nidx[p][k]][c]) on
 * channels-last tensors (y may be NULL; C % 4 == 0, C <= 1024) and leaves max|out| in
 * out_amax64 (B rows of 64 uint32 slots, one row per scene, zeroed by the caller; may be NULL).  No reference counterpart:
 * modules.py:122-128 interpolates first; the two orders agree to fp32 round-off. */
int s4g_interp_add_cl_f32(const float *y_pc, const float *sparse_rc, const int32_t *nidx_p3,
                          const float *nw_p3, const float *bias_c, int64_t B, int64_t N1, int64_t N2,
                          int64_t C, int relu, float *out_pc, float *out_amax64, s4g_stream_t stream);
int s4g_three_interpolate_backward_f32(const float *gout_bcn1,
                                       const int64_t *idx_bn3,
                                       const float *w_bn3, int64_t B, int64_t C,
                                       int64_t N2, int64_t N1, float *gin_bcn2,
                                       s4g_stream_t stream);

/* ABI >= 10.  The two backward scatters DETERMINISTICALLY: same signatures plus a workspace of
 * s4g_scatter_det_workspace_bytes(B, N, T) bytes (256-byte aligned; T = M K for group_points, 3 N1 for
 * three_interpolate; 0 = the sizes are not supported: B T and B N must stay below 2^31).  The contributions are
 * ordered by a stable radix sort on (scene, target point) and every target is summed by one thread in ascending
 * position order -- the sum a sequential loop over the positions forms: run-to-run bit-identical and equal to
 * the CPU oracle bit for bit, where the reference's atomicAdd scatter (grouping_kernel.cu:94,
 * interpolate_kernel.cu:283; s4g_*_backward_f32 above) leaves the order to the hardware.  An index outside
 * [0, N) contributes nothing. */
size_t s4g_scatter_det_workspace_bytes(int64_t B, int64_t N, int64_t T);
/* ... plus room for a channels-last copy of the gradients (C >= 32; weighted = 0: group_points, T = M K; 1:
 * three_interpolate, T = 3 N1): given that much, the two entry points below sum a target from 256-byte rows instead of
 * 4-byte gathers (measured ~3 x faster on the feature tensors; bit-identical results).  Given only the size above they
 * take the gather form. */
size_t s4g_scatter_det_workspace_bytes_c(int64_t B, int64_t C, int64_t N, int64_t T, int weighted);
int s4g_group_points_backward_det_f32(const float *gout_bcmk, const int64_t *idx_bmk, int64_t B, int64_t C,
                                      int64_t N, int64_t M, int64_t K, float *gin_bcn, void *ws,
                                      size_t ws_bytes, s4g_stream_t stream);
int s4g_three_interpolate_backward_det_f32(const float *gout_bcn1, const int64_t *idx_bn3, const float *w_bn3,
                                           int64_t B, int64_t C, int64_t N2, int64_t N1, float *gin_bcn2,
                                           void *ws, size_t ws_bytes, s4g_stream_t stream);

/* Inverse-distance weights of FeatureInterpolator.forward
 * (modules.py:118-120): w = (1/max(d2,eps)) / sum_k (1/max(d2,eps)). */
int s4g_interp_weights_f32(const float *d2_bn3, int64_t B, int64_t N1,
                           float eps, float *w_bn3, s4g_stream_t stream);


/* ---------------------------------------------------------------------------
 * Inference fast path: the shared-MLP contraction on the fp32 matrix cores.
 *
 * One launch computes, for `groups` independent problems (blockIdx.y),
 *     Y[p][n] = act( sum_k A[p][k] * W[n][k] + bias[n] ),  p < P, n < Cout
 * with BatchNorm already folded into W / bias by the caller and every
 * activation stored channels-last ([position][channel], fp32).  It replaces
 * the per-layer Conv{1,2}d(k=1) -> BatchNorm -> ReLU of
 * network_models/nn_utils/conv.py:28-34,68-74 together with the tensor
 * plumbing around it in pointnet2_utils/modules.py (group + concat :42-50,
 * max over neighbours :242-243, interpolate + concat :118-127).
 *
 * loader  S4G_GEMM_LOAD_PLAIN   A row p = A + p*lda + a_coff + g*a_gcol
 *         S4G_GEMM_LOAD_GATHER  A row p = [ feat[b*N + gidx[p]][0..Cf) |
 *                                xyz[b,:,gidx[p]] - ctr[b,:,m] | 0.. ]
 *                                (K order [feat, xyz]; W permuted to match)
 *         S4G_GEMM_LOAD_INTERP  A row p = [ sum_k nw[p,k]*sparse[b*N2+nidx[p,k]] |
 *                                dense[p][0..C1) ]
 *         S4G_GEMM_LOAD_GATHER_MLP1  first xyz-only SA layer folded into the loader:
 *                                A row p = relu(W1 . (xyz[b,:,gidx[p]] - ctr[b,:,m]) + b1),
 *                                mlp1_w = Cin x (wx, wy, wz, bias) fp32
 *         S4G_GEMM_LOAD_GATHER_ADD  first SA layer of a level WITH features, applied to the
 *                                features before the grouping (it is linear; feat = F =
 *                                W_feat . features, (B*N, Cf = Cin) channels-last):
 *                                A row p = relu(F[b*N + gidx[p]] + W_xyz . (xyz - ctr) + b1),
 *                                mlp1_w = Cin x (wx, wy, wz, bias); a_amax bounds |F| and
 *                                a_amax_floor the xyz + bias part (the two are ADDED); with `cbias` the
 *                                bias is a row per centroid (see the member)
 *         S4G_GEMM_LOAD_CHANNEL_FIRST  (ABI >= 14) A is a (B, Cin, a_L) fp32 tensor, channels first:
 *                                A row p = b*a_L + l = A[b][0..Cin)[l]; any Cin >= 1 and any a_L >= 1
 *                                (P % a_L == 0), columns past Cin read as zero.  Lanes walk positions,
 *                                so a wave reads contiguous runs of one channel; the transpose to
 *                                [position][channel] happens on the way into LDS.  FP32 / F16X2 only
 *         S4G_GEMM_LOAD_INTERP_ADD  first FP layer applied before the interpolation (linear):
 *                                A row p = relu(dense[p] + loader_bias + sum_k nw[p,k] *
 *                                sparse[b*N2 + nidx[p,k]]), sparse = W_a . sparse features and
 *                                dense = W_b . skip features (or NULL), both (rows, C2 = Cin);
 *                                a_amax / a_amax2 / a_amax_floor bound the three terms (ADDED)
 * epilogue S4G_GEMM_EPI_STORE   out[p*ldc + c_coff + g*c_gcol + n]
 *          S4G_GEMM_EPI_MAX     out[(p/K)*ldc + c_coff + n] = max over the K
 *                               consecutive rows of a group (K in 16,32,64)
 *          S4G_GEMM_EPI_CHANNEL_FIRST  (B,C,N) tensors cf_ptr[h], channel
 *                               ranges cf_start[h]..cf_start[h+1], sigmoid on
 *                               channels >= cf_sigmoid_from
 *          S4G_GEMM_EPI_MAX_CHANNEL_FIRST  (ABI >= 14) out (B, Cout, M) channels first:
 *                               out[b][n][m] = relu(bias[n] + max over the K consecutive rows of
 *                               group b*M + m), any K >= 1 and M >= 1 (P % (M*K) == 0; groups may
 *                               straddle row tiles).  relu must be 1 (else S4G_EINVAL); `out` must be
 *                               zero-filled by the caller: a tile reduces its rows first and merges
 *                               each (group, channel) it holds with ONE unsigned atomicMax on the bits
 *                               of the non-negative result (order-independent: deterministic).
 *                               FP32 / F16X2 only
 * W is [groups][Cout][Kpad] with Kpad % 8 == 0 (zero padded), bias
 * [groups][Cout].  Cf, C2, lda, a_coff, C1 must be multiples of 4.
 * ------------------------------------------------------------------------- */
#define S4G_GEMM_LOAD_PLAIN 0
#define S4G_GEMM_LOAD_GATHER 1
#define S4G_GEMM_LOAD_INTERP 2
#define S4G_GEMM_LOAD_GATHER_MLP1 3
#define S4G_GEMM_LOAD_GATHER_ADD 4
#define S4G_GEMM_LOAD_INTERP_ADD 5
#define S4G_GEMM_LOAD_CHANNEL_FIRST 6
#define S4G_GEMM_EPI_STORE 0
#define S4G_GEMM_EPI_MAX 1
#define S4G_GEMM_EPI_CHANNEL_FIRST 2
#define S4G_GEMM_EPI_MAX_CHANNEL_FIRST 3
#define S4G_GEMM_FP32 0
#define S4G_GEMM_BF16X3 1
#define S4G_GEMM_BF16 2 /* reduced precision: one bf16 product, fp32 accumulate */
#define S4G_GEMM_F16X2 3 /* fp32-class: two fp16 planes per operand, three products */

typedef struct s4g_gemm_desc {
  int32_t loader, epilogue, groups, relu;
  int32_t P, Cin, Kpad, Cout;
  const float *W;
  const float *bias;
  int32_t w_gstride, b_gstride; /* elements between groups */
  /* PLAIN */
  const float *A;
  int32_t lda, a_coff, a_gcol;
  /* GATHER */
  const int32_t *gidx; /* (B*M*K) neighbour index inside its scene */
  const float *feat;   /* (B*N, Cf) channels-last or NULL when Cf == 0 */
  const float *xyz;    /* (B,3,N) */
  const float *ctr;    /* (B,3,M) */
  int32_t Cf, N, M, K;
  /* INTERP */
  const int32_t *nidx; /* (B*N1, 3) */
  const float *nw;     /* (B*N1, 3) */
  const float *sparse; /* (B*N2, C2) */
  const float *dense;  /* (B*N1, C1) or NULL when C1 == 0 */
  int32_t C2, C1, N2, N1;
  /* output */
  float *out;
  int32_t ldc, c_coff, c_gcol;
  float *cf_ptr[4];
  int32_t cf_start[5];
  int32_t cf_sigmoid_from, cf_N;
  /* arithmetic: S4G_GEMM_FP32 = v_mfma_f32_32x32x2_f32 on W (exact fp32 fma
   * chain); S4G_GEMM_BF16X3 = each fp32 operand split exactly into three bf16
   * numbers, six v_mfma_f32_32x32x16_bf16 per step, fp32 accumulate (drops
   * only terms below 2^-24 |a||b|); S4G_GEMM_BF16 = the hi planes only (plain
   * bf16 inputs, fp32 accumulate: reduced precision, NOT within the 1e-4 bar,
   * for the bf16 roofline configuration).  W_bf16x3 is [3][groups][Cout][Kpad16]
   * bf16 (hi, mid, lo planes of W), Kpad16 % 16 == 0. */
  int32_t precision, Kpad16;
  const void *W_bf16x3;
  const float *mlp1_w; /* GATHER_MLP1: (Cin, 4) = wx, wy, wz, bias */
  /* S4G_GEMM_F16X2 (ABI >= 2): every fp32 operand x is scaled by a power of two
   * s into fp16's range and split x*s = x1 + x2 (two fp16, round-to-nearest:
   * 22 significand bits); three v_mfma_f32_32x32x16_f16 per step evaluate
   * a1*w1 + (a1*w2 + a2*w1) with fp32 accumulation -- the error of a plain
   * fp32 dot product, at half the MFMA count of BF16X3.
   *   W_f16x2      [2][groups][Cout][Kpad16] fp16 planes of W[n][:] / w_inv_scale[n]
   *   w_inv_scale  [groups][Cout] power-of-two 1/s per output channel
   *   a_amax(2)    NULL or 64 floats whose maximum bounds |A| (two pointers: the
   *                INTERP loader reads two tensors); a_amax_floor >= 0 is a host
   *                side bound joined with them (ball radius for the GATHER xyz
   *                columns, the MLP1 bound) -- at least one must be positive
   *   out_amax     NULL or 64 uint32 slots (zeroed by the caller before the
   *                launch): receives atomicMax(bits of max |out|), the a_amax of
   *                the next layer. */
  const void *W_f16x2;
  const float *w_inv_scale;
  const float *a_amax, *a_amax2;
  float a_amax_floor;
  float *out_amax;
  /* optional: the same two fp16 planes in MFMA-fragment order,
   * [groups][Cout/32][Kpad16/16][2 planes][64 lanes][8 halves] with lane = 32*(k/8 % 2) + n % 32
   * (needs Cout % 32 == 0).  When given, launches with Kpad16 % 64 == 0,
   * Cout % 128 == 0 and a short contraction (the A panel of 64 or 128 positions
   * fits LDS) use the resident-A kernel, which streams W fragments straight into
   * the matrix-core operand registers. */
  const void *W_f16x2_frag;
  /* ABI >= 4: with precision S4G_GEMM_BF16 the three *_f16x2_frag pointers hold ONE bf16 plane
   * each in the same fragment order ([groups][Cout/32][Kpad16/16][64 lanes][8 bf16]) and select the
   * single-product form of the fused chains below (no scales: w*_inv_scale, a_amax*, out_amax are
   * ignored) -- the reduced-precision roofline configuration.
   * ABI >= 3, optional: a SECOND layer fused behind this one (S4G_GEMM_F16X2, loader PLAIN
   * GATHER_MLP1, GATHER_ADD or INTERP_ADD, Kpad16 == Cout == C with C = 128, 256 or 512 -- for the plain
   * loader + STORE at C == 256 also Kpad16 == 2 C or 4 C: the first layer then runs through two or four
   * panel loads --, Cout2 % 64 == 0; epilogue MAX
   * with K == 64 and groups == 1, or STORE with any group count -- W2 / w2_inv_scale / bias2
   * then hold `groups` blocks like their first-layer counterparts): the launch computes
   *   out = epilogue(relu2(bias2 + W2 . relu(bias + W . A)))
   * with the C-channel intermediate kept in LDS (split with a per-tile power-of-two scale).
   * W2_f16x2_frag / w2_inv_scale / bias2 describe W2 (Cout2 x C) like W_f16x2_frag /
   * w_inv_scale / bias describe W; out, ldc, c_coff, out_amax refer to the final output.
   * S4G_GEMM_BF16 chains with epilogue MAX need a ReLU behind the LAST layer (relu2, or relu3 of a three-layer
   * chain): the single-plane form only has the max of activated values and answers S4G_EUNSUPPORTED
   * otherwise.  The F16X2 form takes MAX with or without it.  s4g_gemm_chain_supported answers for exactly
   * the (loader, epilogue, C, Kpad16) combinations this paragraph accepts. */
  const void *W2_f16x2_frag;
  const float *w2_inv_scale;
  const float *bias2;
  int32_t Cout2, relu2;
  /* optional THIRD layer (then Cout2 == C: layer 2's output stays in LDS as well and the
   * epilogue / out / ldc / out_amax describe layer 3, Cout3 % 64 == 0). */
  const void *W3_f16x2_frag;
  const float *w3_inv_scale;
  const float *bias3;
  int32_t Cout3, relu3;
  const float *loader_bias; /* S4G_GEMM_LOAD_INTERP_ADD: Cin floats */
  /* ABI >= 4: activation maxima PER SCENE.  rows_per_scene > 0: a_amax / a_amax2 / out_amax are
   * [P / rows_per_scene][64] slot rows and loader row p reads / feeds row p / rows_per_scene, so a
   * scene's power-of-two scales -- and its results -- do not depend on the other scenes of the
   * batch (a tile that straddles scenes joins their rows); 0: one 64-slot row for all rows. */
  int32_t rows_per_scene;
  /* ABI >= 5, optional, S4G_GEMM_LOAD_GATHER_MLP1: (P, 4) fp32 rows (xyz[b,:,gidx[p]] - ctr[b,:,m], 0)
   * as s4g_group_rel_xyz_i32 writes them.  The loader then reads one coalesced 16-byte record per
   * row instead of following gidx into the cloud (two dependent round trips at the head of every
   * workgroup); gidx / xyz / ctr are not read.  Same values, same results. */
  const float *rel_xyz4;
  /* ABI >= 8, optional, both or neither; only S4G_GEMM_LOAD_GATHER_MLP1 + rel_xyz4 + a fused second
   * layer (W2_f16x2_frag) + S4G_GEMM_EPI_MAX with K == 64 and relu2: the DISTINCT-row form.  rel_xyz4 then
   * holds what s4g_group_rel_xyz_unique_i32 wrote -- per centroid only the rows ball_query did not pad
   * (ball_query_kernel.cu:64-67 repeats the first hit; modules.py:243's max over the neighbours cannot
   * see the copies) -- scene b's rows at b * rows_per_scene .. + seg_rows[b] (a multiple of 256, the
   * tallest tile; rows_per_scene % 256 == 0), seg4[row / 4] the OUTPUT row (b M + m) of every group of
   * four rows, -1 for filler.  `out` must be zero-filled by the caller: a centroid's pieces are merged
   * with an unsigned atomicMax on the post-ReLU values.  Same maxima as the 64-row form; the hidden
   * layer's per-tile power-of-two scales see other rows, so outputs agree to fp32 round-off, not bitwise. */
  const int32_t *seg4;
  const int32_t *seg_rows;
  /* ABI >= 8, optional: a SECOND output tensor for a plain single layer (loader PLAIN, epilogue STORE, groups 1,
   * no fused layers; f16x2 / bf16 precision): two layers that read the same input run as one launch with W, bias
   * and scales concatenated along Cout -- output channels [0, split_n) go to `out` (row stride ldc, c_coff 0),
   * channels [split_n, Cout) to `out2` (row stride ldc2, column n - split_n) and their per-scene maxima to
   * out_amax2.  split_n and Cout multiples of 256.  (The network's first SA layer on features and the first FP
   * layer on the skip features read the same level: modules.py:242 / :505.) */
  float *out2;
  int32_t ldc2, split_n;
  float *out_amax2;
  /* ABI >= 14, optional, S4G_GEMM_LOAD_GATHER_ADD only (S4G_EINVAL with any other loader): a bias PER CENTROID,
   * (nscenes * M, Cin) fp32 channels-last, 16-byte aligned.  When non-NULL the row of centroid (b, m) uses
   * cbias[(b*M + m)*Cin + k] in place of mlp1_w[k].w (mlp1_w[k].xyz as before):
   *   A row p = relu(F[b*N + gidx[p]] + W_xyz . (xyz - ctr) + cbias[b*M + m])
   * -- the edge levels of MODEL.TYPE "EDGEPN2D", whose first layer W . [rel | f_j | f_j - f_c] + b splits into
   * W_xyz . rel (this loader), (W_a + W_b) . f_j per point (F) and b - W_b . f_c(m) per centroid (cbias).
   * F16X2: the three terms are ADDED, so a_amax bounds |F|, a_amax2 |cbias| (the out_amax of the launch that
   * wrote it) and a_amax_floor the xyz term alone.  NULL: everything as without the member.  The ctypes mirror's
   * last member is pinned to a_L, so this one sits in front of it. */
  const float *cbias;
  /* ABI >= 14: S4G_GEMM_LOAD_CHANNEL_FIRST: positions per scene of the (B, Cin, a_L) input (N of a (B, C, N)
   * tensor, M*K of a (B, C, M, K) one).  rows_per_scene = a_L gives per-scene scales. */
  int32_t a_L;
} s4g_gemm_desc_t;

int s4g_mlp_gemm_f32(const s4g_gemm_desc_t *desc, s4g_stream_t stream);

/* ---------------------------------------------------------------------------
 * The four per-point heads as ONE launch (ABI >= 4).  Replaces, for inference,
 * PointNet2_tcls.py:126-140: mlp_seg / mlp_R / mlp_t / mlp_movable (four SharedMLP stacks
 * C -> H0 -> H1 -> H2 -> H3 over the SAME (B, C, N) input, definitions :83-95) and their
 * Conv1d logit layers (+ Sigmoid on movable_logit), BatchNorm folded by the caller.  A workgroup
 * keeps the 64 x C input panel and every hidden activation in LDS; only X and the four
 * (B, c_h, N) outputs touch HBM.  Shipped widths only: C = 256, H = (512, 256, 256, 128).
 *   precision    S4G_GEMM_F16X2 (fp32-class) or S4G_GEMM_BF16 (one bf16 plane, reduced precision)
 *   W_frag[l]    layer l's planes in MFMA-fragment order ([Cout/32][K/16][planes][64][8]):
 *                l = 0: the four first layers stacked (4 H0 x C); l = 1..3: (4, H_l, H_{l-1});
 *                l = 4: the logit layers zero-padded to (4, 32, H3)
 *   bias[l], w_inv_scale[l]  per output channel, same stacking (w_inv_scale: F16X2 only)
 *   out[h], channels[h]      head h's (B, channels[h], N) fp32 tensor; sigmoid_head = index of the
 *                head whose logits pass through a sigmoid (-1: none)
 *   a_amax / a_amax_floor / rows_per_scene   bound |X| per scene (F16X2), as in s4g_gemm_desc_t
 * ------------------------------------------------------------------------- */
typedef struct s4g_heads_desc {
  int32_t precision, P, N, ldx;
  int32_t C, H0, H1, H2, H3;
  const float *X; /* (P, ldx >= C) channels-last */
  const void *W_frag[5];
  const float *bias[5];
  const float *w_inv_scale[5];
  float *out[4];
  int32_t channels[4];
  int32_t sigmoid_head;
  const float *a_amax;
  float a_amax_floor;
  int32_t rows_per_scene;
  /* ABI >= 6, optional (pre_W_frag[0] != NULL): the tail of the LAST feature-propagation level in
   * front of the heads, in the same launch -- PointnetFPModule.forward (pointnet2_utils/modules.py:
   * 498-507) of fp_modules[2] with its first layer already applied to the sparse features
   * (S4G_GEMM_LOAD_INTERP_ADD's algebra): the workgroup's input panel is formed as
   *     X0[p] = relu(sum_k pre_nw[p][k] * pre_sparse[b N2 + pre_nidx[p][k]] (+ pre_dense[p]) + pre_lbias)
   * and two C -> C layers (pre_W_frag / pre_bias / pre_w_inv_scale [0..1], ReLU each) run on it
   * inside LDS before the heads read it; X / ldx are then unused and a_amax / pre_a_amax2 bound
   * |pre_sparse| / |pre_dense| per scene (a_amax_floor: the bias bound, summed with them).  The
   * (P, C) feature tensor between fp_modules[2] and the heads never exists in HBM. */
  const void *pre_W_frag[2];
  const float *pre_bias[2];
  const float *pre_w_inv_scale[2];
  const int32_t *pre_nidx;   /* (P, 3) */
  const float *pre_nw;       /* (P, 3) */
  const float *pre_sparse;   /* (B N2, C) channels-last */
  const float *pre_dense;    /* (P, C) or NULL */
  const float *pre_lbias;    /* C */
  const float *pre_a_amax2;  /* per-scene maxima of pre_dense or NULL */
  int32_t pre_N2;
  /* ABI >= 9, optional: floats between two consecutive scenes' blocks of EVERY out[h].  0 = each out[h] is
   * its own contiguous (B, channels[h], N) tensor.  Non-zero (>= channels[h] N): the four heads are channel
   * slices of ONE packed (B, C_total, N) tensor -- out[h] = packed + first_channel_h * N, out_batch_stride =
   * C_total * N -- which is what the multi-GPU path all-gathers (dist.py), so no copy packs the outputs. */
  int64_t out_batch_stride;
  /* ABI >= 11, optional: bit h set = evaluate head h; 0 = all four.  Heads that are not evaluated leave their out[h]
   * untouched (it may be NULL).  A serving path that only decodes the best-scoring points runs the score head (bit 0) on
   * every point and the pose heads (bits 1..3) on the points it keeps: FusedPointNet2(..., topk=). */
  int32_t head_mask;
} s4g_heads_desc_t;

int s4g_heads_chain_f32(const s4g_heads_desc_t *desc, s4g_stream_t stream);

/* ABI >= 14.  Per-scene bound of |x| for f16x2 inputs that no launch of this library produced: x is B scenes of
 * n_per_scene fp32 values each; slot row b of out_slots ((B, 64) uint32, ZEROED by the caller) receives atomicMax
 * of the bits of max |x| over scene b -- the layout s4g_gemm_desc_t.a_amax reads with rows_per_scene > 0. */
int s4g_amax_per_scene_f32(const float *x, int64_t B, int64_t n_per_scene, float *out_slots, s4g_stream_t stream);

/* 1 when s4g_mlp_gemm_f32 has a fused-chain form (W2_f16x2_frag set) for this first-layer
 * loader, final epilogue, chain width C (= Cout = Cout2 of a three-layer chain) and first-layer
 * depth Kpad16; callers decide with it which layers to hand over as one launch. */
int s4g_gemm_chain_supported(int loader, int epilogue, int C, int Kpad16);

/* int32-index variants used by the fast path (same kernels and semantics as
 * s4g_ball_query_f32 / s4g_three_nn_f32; the int64 API tensors are an
 * interface requirement of the reference, not of the hardware).
 * s4g_three_nn_weights_i32 also applies the inverse-distance weights of
 * modules.py:118-120 and does not write the distances. */
int s4g_ball_query_i32(const float *xyz_b3n, const float *ctr_b3m, int64_t B,
                       int64_t N, int64_t M, float radius, int64_t K,
                       int32_t *idx_bmk, int32_t *cnt_bm, void *ws,
                       size_t ws_bytes, int flags, s4g_stream_t stream);
int s4g_three_nn_weights_i32(const float *q_b3n1, const float *k_b3n2, int64_t B,
                             int64_t N1, int64_t N2, float eps, int32_t *idx_bn3,
                             float *w_bn3, void *ws, size_t ws_bytes, int flags,
                             s4g_stream_t stream);
/* Grid-accelerated variant of s4g_three_nn_weights_i32 for the fast path: keys are
 * binned into cells of edge `cell` (use the set-abstraction radius of the level
 * the keys came from), the queries are binned into the same cells by the same launch
 * and walked in cell order (a wave's 64 queries share their key rows), each searches
 * 27 cells, unanswered queries fall back to the index-order scan in the same call --
 * identical results for every input.  cell < 0 (round 4, what the fast path passes): the edge is chosen on
 * the device, 1.75 x the median distance from a key to its third-nearest other key over 64 sample keys (one
 * wave each) -- the SA radius is the right edge on surface-like clouds only.
 * Workspace: s4g_three_nn_grid_workspace_bytes(B, N1, N2) (keys' grid + fail list +
 * the binned queries: ~128 bytes per query + 0.6 MB per scene); N2 <= 65536. */
size_t s4g_three_nn_grid_workspace_bytes(int64_t B, int64_t N1, int64_t N2);
/* Diagnostic (ABI >= 8): byte offset, inside that workspace, of the fail list's header of int32 words -- word 0:
 * the queries the 27 cells could not answer in the last call (they took the all-keys scan), words 4 / 5: the
 * device-chosen 1 / edge and acceptance bound (floats) when cell < 0. */
size_t s4g_three_nn_grid_header_offset(int64_t B, int64_t N2);
int s4g_three_nn_weights_grid_i32(const float *q_b3n1, const float *k_b3n2, int64_t B,
                                  int64_t N1, int64_t N2, float eps, float cell,
                                  int32_t *idx_bn3, float *w_bn3, void *ws,
                                  size_t ws_bytes, int flags, s4g_stream_t stream);

/* s4g_three_nn_f32's outputs (int64 indices, squared distances) through the same grid:
 * for operator-API callers.  cell > 0: the caller names the cell edge; cell < 0: the call
 * derives one on the device (1.75 x the median third-neighbour distance of 64 sample keys,
 * no host read).  Same workspace; identical results for any cell. */
int s4g_three_nn_grid_f32(const float *q_b3n1, const float *k_b3n2, int64_t B, int64_t N1,
                          int64_t N2, float cell, int64_t *idx_bn3, float *d2_bn3, void *ws,
                          size_t ws_bytes, int flags, s4g_stream_t stream);

/* QueryGrouper's operator pair in one pass (modules.py:39-42):
 * ball_query + group_points(xyz, index).  Same outputs as calling
 * s4g_ball_query_f32 then s4g_group_points_f32 with C = 3: index (B,M,K) int64,
 * count (B,M) int64, grouped (B,3,M,K) fp32 (NOT centroid-subtracted). */
int s4g_query_group_f32(const float *xyz_b3n, const float *ctr_b3m, int64_t B,
                        int64_t N, int64_t M, float radius, int64_t K,
                        int64_t *idx_bmk, int64_t *cnt_bm, float *grouped_b3mk,
                        void *ws, size_t ws_bytes, int flags, s4g_stream_t stream);

/* group_points(xyz, index) - centroid as one 16-byte record per neighbour (modules.py:42-44:
 * group_xyz = group_points(xyz, index); group_xyz -= new_xyz.unsqueeze(-1)), for the first SA
 * layer's loader (s4g_gemm_desc_t.rel_xyz4): out (B*M*K, 4) = (x - cx, y - cy, z - cz, 0), each
 * difference one rounded fp32 subtraction. */
int s4g_group_rel_xyz_i32(const float *xyz_b3n, const float *ctr_b3m, const int32_t *idx_bmk,
                          int64_t B, int64_t N, int64_t M, int64_t K, float *rel_pk4,
                          s4g_stream_t stream);

/* The same records without ball_query's padding copies (ABI >= 8; see s4g_gemm_desc_t.seg4).
 * cnt_bm = ball_query's count output (int32).  Centroid m of scene b contributes
 * c4 = round_up(max(cnt, 1), 4) rows (slots cnt .. c4-1 are copies of slot 0, so they are valid
 * padding; an empty ball keeps its K copies of point 0 as 4 rows), centroids back to back from
 * row b M K:
 *   rel_pk4       (B M K, 4) capacity, rows as above; rows between a scene's last centroid and
 *                 rows_b[b] are zero records
 *   seg4          (B M K / 4) int32: b M + m per group of 4 rows, -1 for the filler rows
 *   row_start_bm  (B, M) int32: first row of every centroid relative to its scene's base
 *   rows_b        (B) int32: rows of scene b, rounded up to 256
 * A scene whose rows would exceed 7/8 of M K keeps the PLAIN layout instead (centroid m at row m K, all K
 * slots, rows_b[b] == M K): the segmented epilogue would cost more than the few copies save; the
 * contraction takes its 64-row epilogue for such a scene.  The choice depends on the scene alone.
 * K % 4 == 0 and (M K) % 256 == 0, else S4G_EUNSUPPORTED. */
int s4g_group_rel_xyz_unique_i32(const float *xyz_b3n, const float *ctr_b3m, const int32_t *idx_bmk,
                                 const int32_t *cnt_bm, int64_t B, int64_t N, int64_t M, int64_t K,
                                 float *rel_pk4, int32_t *seg4, int32_t *row_start_bm, int32_t *rows_b,
                                 s4g_stream_t stream);

/* FPS + centroid gather in one call: idx (B,M) int32 and ctr (B,3,M) planar. */
int s4g_fps_gather_i32(const float *xyz_b3n, int64_t B, int64_t N, int64_t M,
                       int32_t *idx_bm, float *ctr_b3m, void *ws, size_t ws_bytes,
                       int flags, s4g_stream_t stream);

/* FPS of the NEXT set-abstraction level without running it (round 3).
 *
 * modules.py:80-83 samples each level from the previous level's centroids, which are the picks of
 * the previous FPS in pick order.  FPS over such a set, started at its element 0 (sampling_kernel.cu:
 * 66-68), re-picks the set's own prefix: element k was the farthest point of the WHOLE cloud from
 * {0..k-1}, the set contains it, so it is also the farthest point of the set -- as long as no other
 * element ties with it, which is the only case in which the tie rule of sampling_kernel.cu:87-105
 * matters.  s4g_fps_gather_ex_i32 = s4g_fps_gather_i32 with two optional extras:
 *   dist_bm (B,M): the min-distance every pick had when it was taken (+inf for pick 0);
 *                  S4G_EUNSUPPORTED (nothing launched) if this size's kernel cannot report it;
 *   run_b (B):     run_b[b] == 0 = "scene b's result is the identity prefix": idx = 0..M-1, ctr =
 *                  the first M input points, nothing sampled (only honoured by the kernels for
 *                  N <= 10 240; larger inputs are sampled regardless).
 * s4g_fps_prefix_check_f32 proves or refutes the prefix property per scene: ctr_b3m (B,3,M1) and
 * dist_bm (B,M1) from the previous level's call; run_b[b] = 0 iff, at every step k < M2, no element
 * other than k reaches element k's distance (same fp32 arithmetic as the sampler; FMAD flag as
 * usual).  A scene with run_b[b] = 1 is then sampled for real, so the indices are the reference's
 * in every case.  One check over M2 steps also covers deeper levels that sample a prefix of this
 * one (fewer steps over fewer elements).  5 120 -> 1 024: 20 us instead of 0.87 ms. */
int s4g_fps_gather_ex_i32(const float *xyz_b3n, int64_t B, int64_t N, int64_t M, int32_t *idx_bm,
                          float *ctr_b3m, float *dist_bm, const int32_t *run_b, void *ws,
                          size_t ws_bytes, int flags, s4g_stream_t stream);
int s4g_fps_prefix_check_f32(const float *ctr_b3m, const float *dist_bm, int64_t B, int64_t M1,
                             int64_t M2, int32_t *run_b, int flags, s4g_stream_t stream);

/* Diagnostic entry (tests): the pruned FPS kernels' pre-pass on its own -- ONE launch, one
 * workgroup per scene: bounding box, a 15-bit cell key per point (2-D Hilbert curve over the two
 * long axes for thin clouds, extent-dealt Morton bits otherwise), LDS counting sort.  Outputs
 * perm (B,N): a permutation of 0..N-1 per scene (cell order; the order INSIDE a cell is not
 * reproducible), and gbox (B,G,6): (min x,y,z, max x,y,z) of every run of 64 consecutive perm
 * entries; G >= ceil(N / 64) groups are written (groups past the end hold NaN).  N <= 65 535.
 * The FPS result never depends on the permutation (sampling_kernel.cu:49-119 has no such step);
 * it only decides how many groups a pick has to revisit. */
int s4g_fps_prepass_f32(const float *xyz_b3n, int64_t B, int64_t N, int64_t G, int32_t *perm_bn,
                        float *gbox_bg6, s4g_stream_t stream);

/* ---------------------------------------------------------------------------
 * Next row: pose decode right after the network.
 * s4g_expected_score_f32: softmax over the C score classes of (B,C,N) logits,
 *   score = sum_c values[c] * softmax[c]   (utils/file_logger_cls.py:34-36,66-68;
 *   grasp_detector.py:145-149 with its own `values`).
 * s4g_decode_poses_f32: for the selected point indices sel (B,K): row-major
 *   R from frame_R (B,9,N), tau = sum_c t_bins[c]*softmax(frame_t)[c],
 *   t = -tau*R[:,0] + p, Gram-Schmidt -> H (B,K,4,4) row-major
 *   (utils/file_logger_cls.py:38-47,203-218; grasp_detector.py:124-135,176-180).
 * ------------------------------------------------------------------------- */
int s4g_expected_score_f32(const float *logits_bcn, int64_t B, int64_t C, int64_t N,
                           const float *values_c, float *score_bn, s4g_stream_t stream);
int s4g_decode_poses_f32(const float *xyz_b3n, const float *frame_R_b9n,
                         const float *frame_t_btn, const int64_t *sel_bk, int64_t B,
                         int64_t N, int64_t K, int64_t TC, const float *t_bins,
                         float *H_bk44, s4g_stream_t stream);

/* ABI 13: the contact network (MODEL.TYPE "PN2", reference network_models/models/PointNet2.py).
 * s4g_contact_heads_f32: raw head logits (B, 17, M) in the order score 3 | R 6 | t 3 | movable 5 (what
 *   s4g_heads_chain_f32 with out_batch_stride = 17 M, or the channel-first epilogue with the four heads as one
 *   17-channel head, writes) -> the network's outputs (B, 20, M): score 3 (copied) | frame_R 9 | frame_t 3 |
 *   movable 5 (copied).  frame_R = toRotMatrix of the 6-D logits (functions/functions.py:179-190: b1 = a1/|a1|,
 *   b2 = a2 - (a2.b1) b1 normalised, b3 = b1 x b2, channel 3i + j = b_j[i]); frame_t = p + t with p the point's
 *   coordinates in xyz (B, 3, N): point m, or point index_bm[b, m] (int64, may be NULL when M == N) for a
 *   forward over a scene's kept points.  Zero or parallel a1 / a2 give NaN in that point's frame_R only.
 *   raw and out must not overlap.
 * s4g_decode_poses_abs_f32: like s4g_decode_poses_f32 for an ABSOLUTE translation frame_t (B, 3, N):
 *   H = [Gram-Schmidt(R) | frame_t[:, sel]] (B, K, 4, 4) row-major. */
int s4g_contact_heads_f32(const float *raw_b17m, const float *xyz_b3n, const int64_t *index_bm, int64_t B,
                          int64_t N, int64_t M, float *out_b20m, s4g_stream_t stream);
int s4g_decode_poses_abs_f32(const float *frame_R_b9n, const float *frame_t_b3n, const int64_t *sel_bk,
                             int64_t B, int64_t N, int64_t K, float *H_bk44, s4g_stream_t stream);

/* Next row f2: batched gripper-vs-cloud collision counts, replaces the per-pose
 * loop over CloudCollisionChecker.view_non_collision
 * (cloud_processor/view_collision_checker.py:37-65, grasp_detector.py:216-234).
 * g2l = global->gripper 4x4 row-major per pose; gripper6 (HOST pointer) =
 * {FINGER_LENGTH, BOTTOM_LENGTH, HALF_HAND_THICKNESS, HALF_BOTTOM_WIDTH,
 *  HALF_BOTTOM_SPACE, BACK_COLLISION_MARGIN} (configs/gripper_config.py:10-21,
 * processing_config.py:39); counts (B,K,2) int32 = {behind the palm, inside
 * the finger volumes}. */
int s4g_collision_counts_f32(const float *xyz_b3n, const float *g2l_bk44, int64_t B,
                             int64_t N, int64_t K, const float *gripper6,
                             int32_t *counts_bk2, s4g_stream_t stream);
/* ABI 12: the same over best-first pose lists padded to K rows: only the first pose_count_b[b] (DEVICE int64, (B,); NULL =
 * all K) rows of scene b are poses -- the rest get zero counts without scanning the cloud (detector.GraspDetector: K =
 * 2 048 rows, a few dozen to a few hundred of them poses; the counts never visit the host) -- a workgroup walks several
 * poses, so the launch stays small.  invert_se3 = 1: the matrices are the POSES themselves (gripper -> global) and the
 * kernel forms their analytic SE(3) inverse [R^T | -R^T t] in fp32, the form grasp_detector.py:219 feeds the check
 * (torch_batch_transformation_inv, utils/math_utils.py:26-40), instead of the caller. */
int s4g_collision_counts_n_f32(const float *xyz_b3n, const float *g2l_bk44, int64_t B, int64_t N,
                               int64_t K, const float *gripper6, const int64_t *pose_count_b,
                               int invert_se3, int32_t *counts_bk2, s4g_stream_t stream);

/* Grading of grasp frames against the dense, labelled scene cloud (csrc/eval_frames.hip): EvalExpCloud.eval_frame
 * (eval_experiment/eval_point_cloud.py:39-113) for every pose of every scene, without host synchronisation.
 * xyz, normals (B, 3, N) fp32 (the normals are rotated by g2l[:3, :3] and NOT re-normalised), labels (B, N) int32,
 * g2l (B, K, 4, 4), pose_count_b and invert_se3 as in s4g_collision_counts_n_f32.  params10 (HOST pointer) = the six
 * values of gripper6, then {BACK_COLLISION_THRESHOLD, FINGER_COLLISION_THRESHOLD, CLOSE_REGION_MIN_POINTS,
 * NEIGHBOR_DEPTH} (eval_experiment/config.py:39-48).  Every inequality is strict, all arithmetic fp32.
 * Outputs, per pose row:
 *   ints_bk8   int32 (B, K, 8) = {back, finger, close, multi_objects, n_left, n_right, collision, 0}: back / finger are
 *              the two integers of s4g_collision_counts_n_f32 bit for bit; close = points of the close region (:95-97);
 *              multi_objects = more than one distinct label among them; collision = back > params[6] or finger >
 *              params[7]; n_left / n_right = populations of the two bands of _antipodal_score (:56-57)
 *   floats_bk5 fp32 (B, K, 5) = {left_y, right_y, mean_left, mean_right, score}: left_y / right_y = maximum / minimum
 *              of local y over the close region (0 when it is empty); mean_* = mean |n_local.y| over the band;
 *              score = mean_left * mean_right.
 *   n_left, n_right, mean_left, mean_right and score are 0 unless the pose reaches the score: close >= params[8],
 *   no collision, one label (:107-111).  Rows at or past pose_count_b[b] are not scanned and read 0 everywhere.
 * Run-to-run bit-identical: integers and extrema by integer atomics, the band sums in a fixed order (per-chunk
 * partials in the workspace, summed pairwise in chunk order), no floating-point atomics.
 * N < 2^30 (S4G_EINVAL otherwise).
 * Workspace: s4g_eval_frames_workspace_bytes(B, N, K) bytes, 256-byte aligned; contents need not be initialised. */
size_t s4g_eval_frames_workspace_bytes(int64_t B, int64_t N, int64_t K);
int s4g_eval_frames_f32(const float *xyz_b3n, const float *normals_b3n, const int32_t *labels_bn,
                        const float *g2l_bk44, int64_t B, int64_t N, int64_t K, const float *params10,
                        const int64_t *pose_count_b, int invert_se3, int32_t *ints_bk8, float *floats_bk5,
                        void *workspace, size_t workspace_bytes, s4g_stream_t stream);

/* Local grasp search of the data generator (csrc/local_search.hip): TorchSingleViewPointCloud.finger_hand with
 * _table_collision_check and _antipodal_score (data_gen/pcd_classes/torch_single_view_point_cloud.py:152-180,224-358)
 * for every frame of every scene, without host synchronisation.  Per frame, L approach depths x T rolls about the
 * frame's x axis = L * T placements, each graded against the scene cloud.
 * points (B, F, 3) frame origins, frames (B, F, 3, 3) with the x, y, z axes as COLUMNS, xyz / normals (B, 3, N) fp32,
 * labels (B, N) int32.  frame_count_b (device, may be NULL): only the first frame_count_b[b] rows of scene b are
 * frames; the others are not scanned and read as invalid.  1 <= L <= 8, 1 <= T <= 16 (S4G_EINVAL otherwise).
 * params13 (HOST pointer) = {FINGER_LENGTH, BOTTOM_LENGTH, HALF_HAND_THICKNESS, HALF_BOTTOM_WIDTH, HALF_BOTTOM_SPACE,
 *   BACK_COLLISION_MARGIN, BACK_COLLISION_THRESHOLD, FINGER_COLLISION_THRESHOLD, CLOSE_REGION_MIN_POINTS,
 *   NEIGHBOR_DEPTH, TABLE_HEIGHT, TABLE_HEIGHT + TABLE_COLLISION_OFFSET, NUM_POINTS_THRESHOLD}
 *   (data_gen/configs/config.py:17-56,89); no_label = the label of a placement without one (len(NAME_LIST)).
 * tables_3l2t (DEVICE pointer, 3 L + 2 T floats) = {depth dl[L], slab lower bound dl - BOTTOM_LENGTH [L], slab upper
 *   bound dl + FINGER_LENGTH [L], cos[T], sin[T]} (config.py:34,44,75-82).
 * A frame with mean |frame| < 1e-6 or p.z + frame[2][0] * FINGER_LENGTH < TABLE_HEIGHT fails its gate (:257,259): not
 * scanned, everything reads as for a padding row.  Every inequality is strict, all arithmetic fp32.
 * Outputs (P = L * T, placement index = depth * T + roll):
 *   ints_bfp6      int32 (B, F, P, 6) = {search_score, objects_label, back, finger, close, table_collision}: back /
 *                  finger / close = the points of the depth slab behind the palm / in the fingers / in the close region
 *                  (:294-321), counted for every placement of a frame that passed its gate and that does not collide with
 *                  the table (the others are skipped before anything is counted, :288, and read 0); table_collision = a corner
 *                  of the gripper's box below params[11] (:224-241); search_score = close and objects_label = the
 *                  region's label where the placement reaches the score -- no table collision, at least params[12]
 *                  points in the slab, back <= params[6], finger <= params[7], close >= params[8], one label
 *                  (:273-330) -- else 0 and no_label
 *   scores_bfp     fp32 (B, F, P): the antipodal score (:167-176) where the placement reaches it, else 0; NaN where a
 *                  band is empty, as in s4g_eval_frames_f32
 *   slab_bfl       int32 (B, F, L): points of each depth slab (:270-273)
 *   valid_bf       int32 (B, F): 1 where the maximum of the frame's scores is not below 1e-4 (:348)
 *   valid_index_bf int32 (B, F): the valid frames of the scene in ascending order, then -1;  count_b int64 (B): how many
 * Every frame's row holds its own results only (the reference leaves a rejected frame's entries in the slot the next
 * frame reuses).  Run-to-run bit-identical and batch invariant: integers and extrema by integer atomics, the band sums
 * as integers of scale 2^-30 (each |n.y| clamped to 4), no floating-point atomics.  N < 2^30, B and F <= 65 535.
 * Workspace: s4g_local_search_workspace_bytes(B, N, F, L, T) bytes, 256-byte aligned; contents need not be
 * initialised. */
size_t s4g_local_search_workspace_bytes(int64_t B, int64_t N, int64_t F, int64_t L, int64_t T);
int s4g_local_search_f32(const float *points_bf3, const float *frames_bf33, const float *xyz_b3n,
                         const float *normals_b3n, const int32_t *labels_bn, int64_t B, int64_t N, int64_t F,
                         int64_t L, int64_t T, const float *params13, int32_t no_label, const float *tables_3l2t,
                         const int64_t *frame_count_b, int32_t *ints_bfp6, float *scores_bfp, int32_t *slab_bfl,
                         int32_t *valid_bf, int32_t *valid_index_bf, int64_t *count_b, void *workspace,
                         size_t workspace_bytes, s4g_stream_t stream);

/* Baseline inputs (csrc/close_region.hip): TorchBaseLineSingleViewPointCloud.finger_hand's best placement and crop
 * (data_gen/pcd_classes/torch_baseline_single_view_point_cloud.py:220-331), close_region_projection (:334-393) and the
 * crop of torch_precomputed_baseline.py:350-383 (the search of that class is s4g_precomputed_baseline_search_f32
 * below), without host synchronisation.
 *
 * s4g_best_placement_f32: points (B, F, 3), frames (B, F, 3, 3) (axes as COLUMNS), scores (B, F, L * T) and tables_3l2t
 * as s4g_local_search_f32 reads and writes them.  Per frame, over the L * T placements in flattened order, the first
 * one whose score is > 0 and > every earlier score (a NaN is never taken, :308-312); the frame is valid unless that
 * score is < 1e-4 (:323).
 *   index_bf       int32 (B, F): the placement, -1 where the frame is invalid;  score_bf fp32 (B, F): its score (0 where
 *                  no placement was taken)
 *   g2l_bf44       fp32 (B, F, 4, 4) = LOCAL_TO_LOCAL_SEARCH[index] @ [R^T | -R^T p] (`baseline_frame`, :320-322), formed
 *                  directly in fp32; all 0 where the frame is invalid
 *   valid_index_bf int32 (B, F): the valid frames in ascending order, then -1;  count_b int64 (B): how many
 * B, F <= 65 535, 1 <= L <= 8, 1 <= T <= 16.
 *
 * s4g_close_region_f32: g2l (B, F, 4, 4) global -> local matrices (rows 0..2 are read), xyz / normals (B, 3, N) fp32.
 * live_bf (device int32 (B, F), may be NULL): rows with 0 are not scanned; frame_count_b (device, may be NULL): rows at
 * or past frame_count_b[b] are not scanned.  Such rows read count 0, flags 0 and zero maps.
 * params13 (HOST pointer) = {x_lo, x_hi, HALF_BOTTOM_SPACE, HALF_HAND_THICKNESS, unit x, y, z, h0 x, y, z, hstep x, y, z}.
 * A point is a member of a frame's close region iff x_lo < lx < x_hi, |ly| < params[2] and |lz| < params[3] for
 * l = G[0..2] . (x, y, z, 1) in fp32, each operation rounded on its own; every inequality strict.
 *   count_bf     int32 (B, F): the members; exact whatever the capacity
 *   offset_bf1   int64 (B, F + 1): the exclusive scan of count in frame order
 *   points_b3c / normals_b3c fp32 (B, 3, capacity), index_bc int32 (B, capacity): frame f's set is the slice
 *                offset[f] : offset[f + 1], in ASCENDING SCENE-POINT INDEX (the order of the reference's boolean
 *                indexing): (lx, ly + params[2], lz + params[3]) (:314-315), the rotation of G applied to the normal, and
 *                the source point index.  Storage past the last stored frame is left untouched.
 *   flags_bf     int32 (B, F): bit 0 = the set does not fit (offset[f + 1] > capacity): nothing is stored for the frame;
 *                bit 1 = a kept point or normal is not finite.  Either bit: the frame's maps are 0.
 *   maps_bf12rr  fp32 (B, F, 12, R, R), 2 <= R <= 64.  Voxel per axis a = floor(c / unit[a]), an fp32 division; a point
 *                counts iff all three indices are in [0, R).  Per voxel: the mean normal (sum / count) and occupancy
 *                (count > 0).  For the axis orders i = 0, 1, 2 = (x, y, z), (y, z, x), (z, x, y) the map is indexed by the
 *                first two axes and summed along the third: channel 4 i = the mean of h0 + k * hstep over the occupied
 *                voxels k of the line (torch.linspace(unit / 2, dim - unit / 2, R)[k], :379-381), channels 4 i + 1 ..
 *                4 i + 3 = the sum of the voxel means over the line divided by the number of occupied voxels; a pixel
 *                without an occupied voxel is 0 (:377-391).
 * Run-to-run bit-identical and batch invariant: counts are integers, the per-voxel normal sums are integers of scale
 * 2^-30 (each component clamped to [-4, 4]) added with integer atomics, everything after them runs in a fixed order.
 * B, F <= 65 535, N < 2^31 - 2048, capacity < 2^31.  Workspace: s4g_close_region_workspace_bytes(B, N, F, capacity)
 * bytes, 256-byte aligned; contents need not be initialised. */
int s4g_best_placement_f32(const float *points_bf3, const float *frames_bf33, const float *scores_bfp,
                           const float *tables_3l2t, int64_t B, int64_t F, int64_t L, int64_t T, int32_t *index_bf,
                           float *score_bf, float *g2l_bf44, int32_t *valid_index_bf, int64_t *count_b,
                           s4g_stream_t stream);
size_t s4g_close_region_workspace_bytes(int64_t B, int64_t N, int64_t F, int64_t capacity);
int s4g_close_region_f32(const float *g2l_bf44, const float *xyz_b3n, const float *normals_b3n,
                         const int32_t *live_bf, const int64_t *frame_count_b, int64_t B, int64_t N, int64_t F,
                         int64_t capacity, int64_t R, const float *params13, int32_t *count_bf, int64_t *offset_bf1,
                         float *points_b3c, float *normals_b3c, int32_t *index_bc, float *maps_bf12rr,
                         int32_t *flags_bf, void *workspace, size_t workspace_bytes, s4g_stream_t stream);

/* GPDClassifier on the 60 x 60 close-region maps (csrc/gpd.hip; added under ABI 14):
 * inference/grasp_proposal/network_models/models/GPD.py in eval mode, without host synchronisation.  Per image x (Cin, 60, 60):
 *   p1 = maxpool2x2(conv1(x) + b1)   conv1 Cin -> 20, 5x5, valid, stride 1, cross-correlation   (20, 28, 28)   no ReLU
 *   p2 = maxpool2x2(conv2(p1) + b2)  conv2 20 -> 50, 5x5                                         (50, 12, 12)   no ReLU
 *   h  = relu(fc1(flatten(p2)) + c1) flatten order (c, y, x), 7200 -> 500
 *   logits = fc2(h) + c2             500 -> classes
 * Pool windows start at even rows and columns.  1 <= Cin <= 12, 1 <= classes <= 16.
 *
 * s4g_gpd_pack_f32: the eight parameter tensors (DEVICE pointers, fp32, contiguous, torch's shapes: conv1_w (20, Cin, 5, 5),
 * conv2_w (50, 20, 5, 5), fc1_w (500, 7200), fc2_w (classes, 500)) -> `packed` (device, s4g_gpd_pack_bytes(Cin, classes)
 * bytes, 16-byte aligned): the conv and fc1 weights as two power-of-two scaled fp16 planes in MFMA fragment order, the
 * biases and fc2 in fp32, and the constants the activation scales are formed from.  Pack again when a parameter changes.
 *
 * s4g_gpd_forward_f32: maps = image g at maps + g * image_stride + c * channel_stride (in floats), the (60, 60) plane
 * contiguous; channels 0 .. Cin - 1 are read.  index (device int32 (G), may be NULL = 0 .. G - 1): row g scores image
 * index[g] of the num_images images; a negative index, or one >= num_images, reads nothing and writes a ZERO row.  With
 * index NULL, G > num_images is S4G_EINVAL.  The convolutions and fc1 run on v_mfma_f32_32x32x16_f16 in the f16x2 split
 * (three products per MAC, fp32 accumulate) with power-of-two activation scales PER IMAGE (from the image's own largest
 * magnitude and bounds formed from it and the weights); fc2 in fp32 FMAs.  Every row is therefore independent of the
 * other rows, of G, of `chunk` and of the run: batch invariant and bit-reproducible.  An image that holds a NaN or an
 * infinity in a channel that is read gets NaN in every output row of its own; the other rows do not change.
 *   logits (G, classes); pool1 (G, 20, 28, 28), pool2 (G, 50, 12, 12), hidden (G, 500): fp32 copies of the levels,
 *   written only where the pointer is not NULL.
 * The images are processed `chunk` at a time (0: 1 024; at most 32 768); the workspace is
 * s4g_gpd_workspace_bytes(min(chunk, G), Cin, classes) bytes (0 stands for 1 024 there too), 16-byte aligned, contents
 * need not be initialised.  G, num_images < 2^31. */
size_t s4g_gpd_pack_bytes(int Cin, int classes);
int s4g_gpd_pack_f32(const float *conv1_w, const float *conv1_b, const float *conv2_w, const float *conv2_b,
                     const float *fc1_w, const float *fc1_b, const float *fc2_w, const float *fc2_b, int Cin, int classes,
                     void *packed, s4g_stream_t stream);
size_t s4g_gpd_workspace_bytes(int64_t chunk, int Cin, int classes);
int s4g_gpd_forward_f32(const float *maps, int64_t image_stride, int64_t channel_stride, const int32_t *index, int64_t G,
                        int64_t num_images, const void *packed, int Cin, int classes, int64_t chunk, float *pool1,
                        float *pool2, float *hidden, float *logits, void *workspace, size_t workspace_bytes,
                        s4g_stream_t stream);

/* PointNetClassifier on variable-length point sets (csrc/pointnet_gpd.hip; added under ABI 14):
 * inference/grasp_proposal/network_models/models/PointNetGPD.py in eval mode with every BatchNorm folded into its layer by
 * the caller, without host synchronisation, every launch on `stream`.  Per set x (3, n), n >= 1:
 *   stn_global = max_j relu(W3 relu(W2 relu(W1 x_j + b1) + b2) + b3)      feat.stn.conv1..3: 3 -> 64 -> 128 -> 1024
 *   trans      = fc3(relu(fc2(relu(fc1(stn_global))))) + I                feat.stn.fc1..3: 1024 -> 512 -> 256 -> 9, (3, 3)
 *   global     = max_j (V3 relu(V2 relu(V1 trans^T x_j + c1) + c2) + c3)  feat.conv1..3, NO ReLU after the last layer
 *   hidden     = relu(fc2(relu(fc1(global))))                             fc1, fc2: 1024 -> 512 -> 256
 *   logits     = fc3(hidden)                                              256 -> classes, 1 <= classes <= 16
 *
 * s4g_pngpd_pack_f32: weights12 / biases12 are HOST arrays of twelve DEVICE pointers (fp32, contiguous, torch's
 * (out, in) shapes, kernel-size-1 convolutions as (out, in)) in the order feat.stn.conv1, conv2, conv3, fc1, fc2, fc3,
 * feat.conv1, conv2, conv3, fc1, fc2, fc3 -> `packed` (device, s4g_pngpd_pack_bytes(classes) bytes, 16-byte aligned):
 * the 64 -> 128, 128 -> 1024, 1024 -> 512 and 512 -> 256 weights as two power-of-two scaled fp16 planes in MFMA fragment
 * order, the rest in fp32, and the constants the activation scales are formed from.  Pack again when a parameter changes.
 *
 * s4g_pngpd_forward_f32: point j, coordinate c of source set s lies at points + base[s] + c * channel_stride + j (floats):
 *   dense  (offset == NULL): base[s] = s * set_stride, every set holds n_points points; num_sets sets;
 *   packed (offset != NULL): s = b * F + f, base[s] = b * set_stride + offset[b * (F + 1) + f], count[s] points
 *          (offset int64 (B, F + 1), count int32 (B, F), flags int32 (B, F) or NULL: the fields of s4g_close_region_f32),
 *          num_sets = B * F, capacity = the points per scene the buffer holds.
 * index (device int32 (G), may be NULL = 0 .. G - 1): row g scores source set index[g].  With index NULL, G > num_sets is
 * S4G_EINVAL.  status (G) int32, may be NULL:
 *   0  scored;
 *   1  the set holds a NaN or an infinity: every output row of it is NaN, nothing of it is staged, no other row changes;
 *   2  not scored: index negative or >= num_sets, no points, flags bit 0, or a slice that leaves [0, capacity): ZERO rows
 *      (the reference raises on an empty set; the zero row is this library's decision).
 * The four matrix layers named above and both trunks' 64 -> 128 and 128 -> 1024 layers run on v_mfma_f32_32x32x16_f16 in
 * the f16x2 split (three products per MAC, fp32 accumulate); the 3 -> 64 and 256 -> 9 / classes layers in fp32 FMAs in a
 * fixed order.  The transform is folded into a per-set first layer V1 trans^T; the 64- and 128-wide per-point
 * intermediates stay in LDS.  A tile is 128 points of one set; the tile list is scanned on the device from the counts;
 * the segment maximum merges tiles with integer atomicMax on an order-preserving key: exact and order independent.
 * Power-of-two scales PER SET.  Every row is independent of the other rows, of G, of `chunk`, of the input form and of
 * the run: batch invariant and bit-reproducible.
 *   logits (G, classes); stn_global (G, 1024), trans (G, 3, 3), global_feat (G, 1024), hidden (G, 256): fp32 copies of
 *   the levels, written only where the pointer is not NULL.
 * The sets are processed `chunk` at a time (0: 1 024; at most 32 768); the workspace is
 * s4g_pngpd_workspace_bytes(min(chunk, G), classes) bytes (0 stands for 1 024 there too), 16-byte aligned, contents
 * need not be initialised.  G, num_sets, n_points, capacity < 2^31. */
size_t s4g_pngpd_pack_bytes(int classes);
int s4g_pngpd_pack_f32(const float *const *weights12, const float *const *biases12, int classes, void *packed,
                       s4g_stream_t stream);
size_t s4g_pngpd_workspace_bytes(int64_t chunk, int classes);
int s4g_pngpd_forward_f32(const float *points, int64_t set_stride, int64_t channel_stride, int64_t n_points,
                          const int64_t *offset, const int32_t *count, const int32_t *flags, int64_t F, int64_t capacity,
                          const int32_t *index, int64_t G, int64_t num_sets, const void *packed, int classes,
                          int64_t chunk, float *stn_global, float *trans, float *global_feat, float *hidden,
                          int32_t *status, float *logits, void *workspace, size_t workspace_bytes, s4g_stream_t stream);

/* Darboux frames of the data generator's label search (csrc/darboux.hip): TorchSingleViewPointCloud._estimate_frame
 * (data_gen/pcd_classes/torch_single_view_point_cloud.py:107-133) for every frame row of every scene, without host
 * synchronisation.  xyz / normals (B, 3, N) fp32, the normals used as given (not re-normalised); frame_index (B, F)
 * int32 indices into the cloud.  A row is PADDING where its index is negative or >= N, or where frame_count_b (device,
 * may be NULL) is given and f >= frame_count_b[b]: frame and point 0, count 0, flags 0.
 * Per frame row, i = frame_index[b][f], n = normals[:, i]:
 *   neighbours = every point j of scene b with squared distance < radius * radius (fp32 product; the subtraction,
 *     squares and sum in fp32, each op rounded on its own; strict), i itself included; any number of them;
 *   c = (I - n n^T) mean_j(n_j), cov = sum_j (n_j - c)(n_j - c)^T (:122-125: the mean is projected, the n_j are not),
 *     both accumulated in double in an order fixed by the scene, cov rounded to fp32 once (scaled by its trace);
 *   v0 = the eigenvector of cov's smallest eigenvalue (cyclic Jacobi in fp32), minor = normalise(v0 - (v0 . n) n),
 *     principal = minor x n, the frame's COLUMNS = [-n, -principal, minor] (:126-133), formed in double, rounded once.
 * Eigenvector sign (the reference leaves it to LAPACK): of the unnormalised minor axis v0 - (v0 . n) n the component
 *   with the largest magnitude is positive, the lowest index winning a tie.  The other sign flips columns y and z
 *   together: a half turn about the approach axis.
 * count < min_neighbours: the identity frame, as the reference leaves it (:118-120), flags 0.
 * Degenerate rows: the unnormalised minor axis has squared norm below 1e-12 (v0 parallel to n), or the point, its
 *   normal or a neighbour's normal is not finite (the reference gives NaN): the ZERO frame, which
 *   s4g_local_search_f32's gate rejects, and flags bit 1.  The point is written as given.
 * Outputs: frames_bf33 fp32 (B, F, 3, 3) row-major, axes as columns; points_bf3 fp32 (B, F, 3) = xyz[:, i];
 *   count_bf int32 (B, F) = the neighbour count k; flags_bf int32 (B, F): bit 0 = a frame was estimated, bit 1 =
 *   degenerate.
 * Run-to-run bit-identical and batch invariant: no atomics touch a sum, every cell of the neighbour grid is read in
 * ascending point index.  A scene outside the grid's exactness range (a coordinate further than about 4 000 radii
 * from the scene's first point, or not finite) or with N > 65 536 is scanned in index order: the same neighbour sets;
 * the sums run in another order, so the last bits may differ from the grid's.
 * Cost: a frame reads the points of its 27 cells twice, and the ordering pass ranks every point against the points
 * of its own cell, so both grow with the square of a cell's population: linear in N for a view sampled at about the
 * radius (tens of points per cell), and of the order of N * N point reads where a whole scene falls into one cell
 * (4e9 for 65 536 points inside one radius -- the same order as the F * k reads the frames themselves then need).
 * radius in (0, 1e18), min_neighbours >= 1, N and F < 2^30, B <= 65 535 (S4G_EINVAL otherwise).
 * Workspace: s4g_darboux_frames_workspace_bytes(B, N, F) bytes (0 for N > 65 536), 256-byte aligned; contents need
 * not be initialised. */
size_t s4g_darboux_frames_workspace_bytes(int64_t B, int64_t N, int64_t F);
int s4g_darboux_frames_f32(const float *xyz_b3n, const float *normals_b3n, const int32_t *frame_index_bf,
                           const int64_t *frame_count_b, int64_t B, int64_t N, int64_t F, float radius,
                           int32_t min_neighbours, float *frames_bf33, float *points_bf3, int32_t *count_bf,
                           int32_t *flags_bf, void *workspace, size_t workspace_bytes, s4g_stream_t stream);

/* Scene-normal transfer of the data generator's label pipeline (csrc/match_normals.hip):
 * TorchSingleViewPointCloud._find_normal (data_gen/pcd_classes/torch_single_view_point_cloud.py:135-150) for every
 * view point of every scene, without host synchronisation.  query (B, 3, N) fp32 the view; scene / scene_normals
 * (B, 3, M) fp32 the dense scene, the normals used as given; camera (B, 3) fp32 the camera LOCATION, or NULL: no
 * orientation.  Per view point q of scene b:
 *   neighbours = every scene point j with squared distance < radius * radius (fp32 product; the subtraction, squares
 *     and sum in fp32, each op rounded on its own; strict), as for s4g_darboux_frames_f32;
 *   cap: where more than max_nn qualify, the max_nn smallest by (fp32 squared distance, index) are kept: open3d's
 *     search_hybrid_vector_3d(radius, max_nn) with its unspecified tie order replaced by "the lower index wins";
 *   m = the mean of the kept normals, in double: a fixed butterfly over the kept normals in (distance, index) rank
 *     order, no atomics;
 *   n = m / |m| (open3d's normalize_normals: a zero vector stays zero);
 *   orient (camera given; orient_normals_towards_camera_location), ref = camera - q in double: |n| == 0 -> n =
 *     ref / |ref|, or (0, 0, 1) where ref is zero; else n . ref < 0 -> n = -n; n . ref == 0 leaves n.  A ref that
 *     is not finite (the query or the camera is not) gives no direction: n stays as it is;
 *   n is rounded to fp32 once.
 * Decisions.  (1) No neighbour: the mean of nothing is NaN, which normalize_normals turns into (0, 0, 1); that is then
 *   oriented; flags bit 1.  (2) The kept normals cancel to exactly zero: the unit vector towards the camera (the zero
 *   vector without a camera); flags bit 2.  (3) A query that is not finite: nothing compares as near, so (1), and
 *   flags bit 3; it is not oriented.  (4) A scene point that is not finite is never a neighbour.  (5) A kept normal
 *   that is not finite: the output is (NaN, NaN, NaN) and flags bit 3 (the reference gives NaN in the components
 *   concerned, or (0, 0, 1) where the first one is); s4g_darboux_frames_f32 marks such a row degenerate.
 * Outputs: normals_b3n fp32 (B, 3, N); count_bn int32 (B, N) = the number of normals averaged, at most max_nn;
 *   flags_bn int32 (B, N): bit 0 = capped (more than max_nn points inside the radius), bit 1 = empty, bit 2 =
 *   cancelled, bit 3 = not finite.
 * Neighbour grid: 64^3 toroidal cells of edge just above the radius about the scene's first point, built with the
 * library's stable radix sort on (scene, cell) keys: NO limit on M.  A scene with a coordinate further than about
 * 4 000 radii from its first point, or not finite, and a query that far from it, are scanned in index order: the same
 * neighbour sets, the same ranks, the same bits.  No scene is scanned for its size.
 * Run-to-run bit-identical and batch invariant (the kept set is a function of the candidate SET, the sum runs in rank
 * order).  Batches above 256 scenes (fewer where 256 * M >= 2^31) are served in chunks on one workspace.
 * Cost: the candidates of a query are the population of its 27 cells, read 64 at a time by one wave; each batch that
 * holds a candidate nearer than the current max_nn-th costs a list insertion, and every 64 insertions one ranking
 * pass of 128 LDS reads.  A whole scene inside one radius costs M reads per query, as the scan does.
 * radius in (0, 1e18), max_nn in [1, 64], N and M < 2^30, M >= 1, B <= 65 535 (S4G_EINVAL otherwise).
 * Workspace: s4g_match_normals_workspace_bytes(B, N, M) bytes (about 36 bytes per scene point and 2 MiB per scene of
 * a chunk), 256-byte aligned; contents need not be initialised. */
size_t s4g_match_normals_workspace_bytes(int64_t B, int64_t N, int64_t M);
int s4g_match_normals_f32(const float *query_b3n, const float *scene_b3m, const float *scene_normals_b3m,
                          const float *camera_b3 /* may be NULL */, int64_t B, int64_t N, int64_t M, float radius,
                          int32_t max_nn, float *normals_b3n, int32_t *count_bn, int32_t *flags_bn,
                          void *workspace, size_t workspace_bytes, s4g_stream_t stream);

/* Normal estimation (csrc/match_normals.hip): PointCloud.estimate_normals of the reference
 * (data_gen/pcd_classes/pointcloud.py:48-60; the same method in cloud_processor.py:44-52, eval_experiment/pointcloud.py
 * and data_gen/eval/pointcloud.py) -- open3d's estimate_normals(KDTreeSearchParamHybrid(radius, max_nn),
 * fast_normal_computation=False), normalize_normals and orient_normals_towards_camera_location -- for every point of
 * every cloud, without host synchronisation.  cloud (B, 3, N) fp32; camera (B, 3) fp32 the camera LOCATION, or NULL;
 * live_b (B,) int32 on the device, or NULL: the rows of cloud b at or past live_b[b] (clamped to [0, N]) are padding.
 * Every live point is a query, and the live finite points are the keys.  Per query p:
 *   neighbours = every key with squared distance < radius * radius, the rule of s4g_match_normals_f32 (fp32, each op
 *     rounded on its own, strict); where more than max_nn qualify the max_nn smallest by (fp32 squared distance, index)
 *     are kept.  The query is its own neighbour at distance 0; its copies at a lower index rank before it;
 *   d_j = key_j - p in double; S1 = sum d_j, S2 = sum d_j d_j^T in double by a fixed butterfly over the kept keys in
 *     rank order (no atomics); cov = S2 / k - (S1 / k)(S1 / k)^T, k the number kept;
 *   n = the unit eigenvector of cov's smallest eigenvalue (cyclic Jacobi in double on cov scaled by its largest entry;
 *     the lowest column where two eigenvalues are equal);
 *   sign: with a camera, ref = camera - p in double, n . ref < 0 -> n = -n.  Without a camera, where n . ref is
 *     exactly 0 and where ref is not finite: the component of n of largest magnitude is positive, the lowest axis
 *     winning a tie (the rule of s4g_darboux_frames_f32);
 *   n is rounded to fp32 once.
 * Decisions (open3d cannot be run where this library is tested; these define the result).  (1) Fewer than 3 kept
 *   neighbours: (0, 0, 1), then given its sign as above; flags bit 1 (open3d leaves the point's previous normal, (0, 0,
 *   1) in a cloud that had none).  (2) Every kept point identical, or a solve that gives a zero or non-finite vector:
 *   (0, 0, 1), given its sign; flags bit 2 (open3d's solver returns the zero vector, which it replaces by (0, 0, 1)).
 *   Collinear neighbours are not flagged: they get a unit vector perpendicular to their line.  (3) A query that is not
 *   finite: (0, 0, 1) as it stands, count 0, flags bit 3 alone; a point that is not finite is never a neighbour.
 *   (4) More than max_nn points inside the radius: flags bit 0.  (5) Padding rows: the zero vector, count 0, flags bit 4
 *   alone; they are neither queries nor keys.
 * Outputs: normals_b3n fp32 (B, 3, N); count_bn int32 (B, N) the number of kept neighbours; flags_bn int32 (B, N).
 * Neighbour grid: that of s4g_match_normals_f32 about the cloud's first live finite point.  A point that is not finite
 * or is padding is held by no cell and sends no scene to the index-order scan; a finite live point further than about
 * 4 000 radii from the origin does: the same neighbour sets, ranks and bits either way.  Run-to-run bit-identical and
 * batch invariant; batches above 256 scenes (fewer where 256 * N >= 2^31) are served in chunks on one workspace.
 * radius in (0, 1e18), max_nn in [1, 64], N < 2^30, B <= 65 535 (S4G_EINVAL otherwise).
 * Workspace: s4g_estimate_normals_workspace_bytes(B, N) bytes (S4G_EWORKSPACE below that), 256-byte aligned; contents
 * need not be initialised. */
size_t s4g_estimate_normals_workspace_bytes(int64_t B, int64_t N);
int s4g_estimate_normals_f32(const float *cloud_b3n, const float *camera_b3 /* may be NULL */,
                             const int32_t *live_b /* may be NULL: all N */, int64_t B, int64_t N, float radius,
                             int32_t max_nn, float *normals_b3n, int32_t *count_bn, int32_t *flags_bn,
                             void *workspace, size_t workspace_bytes, s4g_stream_t stream);

/* The nearest scene point of every view point (csrc/match_normals.hip): the max_nn = 1 search of
 * TorchPrecomputedSingleViewPointCloud._find_match (data_gen/pcd_classes/torch_contact_single_view_point_cloud.py:
 * 142-150), returning the index.  The same grid, fp32 distance rule, strict radius, "(distance, then lower index)
 * wins" and index-order fallback as s4g_match_normals_f32, whose build and query code it shares: the same bits from
 * the grid and from the fallback.  nearest_bn int32 (B, N): the scene index, or -1 where no scene point is inside the
 * radius or the query is not finite.  A scene point that is not finite is never a neighbour.
 * radius in (0, 1e18), N and M < 2^30, M >= 1, B <= 65 535 (S4G_EINVAL otherwise).
 * Workspace: what s4g_match_normals_workspace_bytes gives for (B, N, M); contents need not be initialised. */
int s4g_match_nearest_f32(const float *query_b3n, const float *scene_b3m, int64_t B, int64_t N, int64_t M,
                          float radius, int32_t *nearest_bn, void *workspace, size_t workspace_bytes,
                          s4g_stream_t stream);

/* Grading of the contact model's labels (csrc/contact_search.hip): TorchPrecomputedSingleViewPointCloud.finger_hand
 * with _table_collision_check (data_gen/pcd_classes/torch_contact_single_view_point_cloud.py:236-294) for every scene
 * frame of every scene, without host synchronisation.  The reference grades a frame from global_to_local and the
 * scene alone and repeats that for every view point that picked the frame; here a scene frame is graded once.
 * g2l (B, F, 4, 4) fp32 row-major, the scene's global_to_local; xyz (B, 3, M) fp32; labels (B, M) int32.
 * frame_count_b (device, may be NULL): rows at or past frame_count_b[b] are not scanned and read invalid, label
 * no_label and 0 everywhere else.
 * nz, ny, nx in [1, 4]: the lengths of HEIGHT_SEARCH, WIDTH_SEARCH, LENGTH_SEARCH (S4G_EINVAL otherwise); P = nz * ny *
 * nx placements, index (iz * ny + iy) * nx + ix: the reference's loops (:270-279), dz outer, dx inner.
 * params10 (HOST pointer) = {FINGER_LENGTH, BOTTOM_LENGTH, HALF_HAND_THICKNESS, HALF_BOTTOM_WIDTH, HALF_BOTTOM_SPACE,
 *   BACK_COLLISION_MARGIN, TABLE_HEIGHT + TABLE_COLLISION_OFFSET, max |dx|, max |dy|, max |dz|} (the last three size
 *   the bounding cull only); no_label = the label of a frame without one (len(NAME_LIST)).
 * tables_2z3y2x (DEVICE pointer, 2 nz + 3 ny + 2 nx floats) = {-HHT + dz [nz], HHT + dz [nz], -HBS + dy [ny],
 *   HBS + dy [ny], dy [ny], -BOTTOM_LENGTH + dx [nx], FINGER_LENGTH + dx [nx]}: every bound formed in double and
 *   rounded to fp32 once, as torch compares an fp32 tensor with a Python scalar.
 * Per frame, local = g2l @ [p; 1] in fp32 as s4g_eval_frames_f32 forms it, once per scene point; per placement, with
 * every inequality strict (:271-286):
 *   z_bool = z < HHT + dz and z > -HHT + dz;  y_bool = y < HBS + dy and y > -HBS + dy;  abs_y = |y + dy| (one fp32
 *   add; the sign of dy in y_bool and in abs_y is the reference's);  y_collision = abs_y > HBS and abs_y < HBW;
 *   x_bool = x > -BOTTOM_LENGTH + dx and x < FINGER_LENGTH + dx;
 *   finger = count(z & x & y_collision);  close = count(x & z & y_bool);  behind = count of close points with x <
 *   BACK_COLLISION_MARGIN (the reference's min() < margin wherever the region is not empty);  multi_label = the
 *   close region holds more than one label.  A point that is not finite is in no region.
 * A frame is valid when no corner of the CENTRED gripper box (local_to_global @ GRIPPER_BOUND) is below params10[6]
 * and every placement has finger == 0, close > 0, behind == 0 and one label.  The reference returns at the first
 * failing placement; validity is the AND over the placements, so all are counted in one pass.
 * Decisions.  (1) An empty close region makes the reference raise (min() of an empty tensor): here the frame is
 *   invalid and fail bit 4 is set.  (2) local_to_global is the rigid inverse [R^T | -R^T t] formed in the kernel from
 *   g2l, not torch.inverse; g2l must be rigid and is not checked.  (3) A g2l entry that is not finite: the frame is
 *   not scanned, invalid, counts 0, fail = bit 5 alone.  (4) The table verdict covers the centred box only:
 *   LOCAL_SEARCH_TO_LOCAL (:18-28) is written element by element into an expand()ed tensor, the writes alias and all
 *   nine matrices end as the identity, so _table_collision_check never sees a shifted box.
 * Outputs:
 *   ints_bfp4  int32 (B, F, P, 4) = {finger, close, behind, multi_label}, counted whatever the table verdict
 *   table_bf   int32 (B, F): 1 where the centred box collides with the table
 *   valid_bf   int32 (B, F);  label_bf int32 (B, F): the close region's label of the LAST placement (dz = dy = dx = 0
 *              as shipped, :293) where the frame is valid, else no_label
 *   fail_bf    int32 (B, F), over all placements: bit 0 = table, bit 1 = finger, bit 2 = behind, bit 3 = several
 *              labels, bit 4 = empty close region, bit 5 = a g2l entry that is not finite; valid = (fail == 0)
 * Run-to-run bit-identical and batch invariant: counts and label extrema by integer atomics, no floating-point
 * atomics.  M < 2^30, F < 2^30 (the frame loop runs inside the kernel), B <= 65 535.
 * Cost: every scene point is transformed for every frame, M * F * 18 flops; a point inside the widened box's
 * circumsphere then costs the region tests.  There is no spatial index over the scene.
 * Workspace: s4g_contact_search_workspace_bytes(B, M, F, P) bytes (20 per placement), 256-byte aligned; contents
 * need not be initialised; every launch of the call is a kernel. */
size_t s4g_contact_search_workspace_bytes(int64_t B, int64_t M, int64_t F, int64_t P);
int s4g_contact_search_f32(const float *g2l_bf44, const float *xyz_b3m, const int32_t *labels_bm, int64_t B, int64_t M,
                           int64_t F, int64_t nz, int64_t ny, int64_t nx, const float *params10, int32_t no_label,
                           const float *tables_2z3y2x, const int64_t *frame_count_b, int32_t *ints_bfp4,
                           int32_t *table_bf, int32_t *valid_bf, int32_t *label_bf, int32_t *fail_bf, void *workspace,
                           size_t workspace_bytes, s4g_stream_t stream);

/* The contact model's label per view point (csrc/contact_search.hip): the rest of _find_match (:146-173) and of
 * run_score (:189-208) of torch_contact_single_view_point_cloud.py, one thread per view point, without host
 * synchronisation.  nearest (B, N) int32 from s4g_match_nearest_f32 (run on the noise-free reference cloud); cloud
 * (B, 3, N) the noisy view; scene_normals (B, 3, M); camera (B, 3) the camera location; offsets (B, M + 1) and order
 * (B, F) int32: a CSR whose row i lists the scene frames of scene point i in ascending frame index (the order of
 * np.nonzero(frame_point_index == i), :152), any number of them; valid (B, F) int32 from s4g_contact_search_f32;
 * search, antipodal (B, F) fp32 the scene's scores.  Per view point, i = nearest:
 *   n = scene_normals[:, i], or (0, 0, 1) where i is -1 (:146-151); n / |n| in double, a zero normal giving NaN as
 *     numpy does (:166); turned towards the camera by the rule of s4g_match_normals_f32 (ref = camera - cloud point,
 *     not the reference-cloud point); rounded to fp32 once;
 *   score of a frame = min(log(search) / 6.5, 1) * antipodal in fp32, a NaN kept as torch.min keeps it (:189-193);
 *   the fold (:200-206): best = 0; for each valid frame of i in ascending frame index: best > s skips it, else best = s
 *     and arg = frame -- an equal score picks the later frame, a NaN propagates as in the reference;
 *   the point is valid when best > 0 (:208).
 * Outputs: normals_b3n fp32 (B, 3, N); best_frame_bn int32 (B, N) the scene frame of a valid point, else -1;
 * point_score_bn fp32 (B, N) = best; valid_index_bn int32 (B, N) the valid view points in ascending order, then -1;
 * count_b int64 (B).  N, M, F < 2^30, M >= 1, B <= 65 535 (S4G_EINVAL otherwise).  No workspace. */
int s4g_contact_select_f32(const int32_t *nearest_bn, const float *cloud_b3n, const float *scene_normals_b3m,
                           const float *camera_b3, const int32_t *offsets_bm1, const int32_t *order_bf,
                           const int32_t *valid_bf, const float *search_bf, const float *antipodal_bf, int64_t B,
                           int64_t N, int64_t M, int64_t F, float *normals_b3n, int32_t *best_frame_bn,
                           float *point_score_bn, int32_t *valid_index_bn, int64_t *count_b, s4g_stream_t stream);

/* The refine stage of the contact-object pipeline (csrc/contact_refine.hip; added under ABI 14 with no layout change):
 * check_single_collision of data_gen/utils/refine_contact_object.py:45-114 for every frame of every object, over the
 * object's own cloud, without host synchronisation.
 * g2l (B, F, 4, 4) fp32 row-major; xyz (B, 3, M) fp32; search (B, F) fp32 the frames' search_score.  count_b (device,
 * may be NULL): the points of object b are its first count_b[b]; frame_count_b (device, may be NULL) likewise for rows.
 * A row is LIVE when it lies below frame_count_b[b] and search > min_search_score (:46; a NaN is not); other rows are
 * never scanned and get fail = bit 4 alone.  A live row with a g2l entry that is not finite is never scanned either:
 * fail = bit 3 alone.
 * nz, ny, nx in [1, 4], P = nz * ny * nx placements, index (iz * ny + iy) * nx + ix (dz outer, dx inner, :74-83);
 * params8 (HOST) = {FINGER_LENGTH, BOTTOM_LENGTH, HALF_HAND_THICKNESS, HALF_BOTTOM_WIDTH, HALF_BOTTOM_SPACE, max |dx|,
 * max |dy|, max |dz|}; tables_2z3y2x (DEVICE) as for s4g_contact_search_f32, and the same inequalities on the same
 * fp32 local coordinates (:75-85), the sign of dy in y_bool and in |y + dy| the script's:
 *   finger = count(z & x & y_collision) (:86);  close = count(x & z & y_bool) (:89-90);  behind = count of close points
 *   with x < 0 (:93).
 * A frame is kept when every placement has finger <= collision_threshold, close >= min_search_score and behind == 0;
 * its score is the minimum close count over the placements (:95) as an exact fp32.  1 <= min_search_score < 2^24 and
 * collision_threshold >= 0 (S4G_EINVAL otherwise): with a minimum of 1 the count gate precedes the min() of an empty
 * region, where the script raises.  The script returns at the first failing placement; all are counted here.
 * Outputs: counts_bfp3 int32 (B, F, P, 3) = {finger, close, behind}, zero on rows that are not scanned; kept_bf int32
 *   (B, F); score_bf fp32 (B, F), 0 where not kept; fail_bf int32 (B, F): bit 0 = finger, bit 1 = too few close
 *   points, bit 2 = behind, bit 3 = not finite, bit 4 = not live; kept = (fail == 0); kept_index_bf int32 (B, F) the
 *   kept rows in ascending order, then -1; kept_count_b int64 (B).
 * Run-to-run bit-identical and batch invariant: integer atomics only.  M, F < 2^30, M >= 1, B <= 65 535.
 * Workspace: s4g_contact_refine_workspace_bytes(B, M, F, P) bytes (12 per placement); contents need not be
 * initialised; every launch of the call is a kernel. */
size_t s4g_contact_refine_workspace_bytes(int64_t B, int64_t M, int64_t F, int64_t P);
int s4g_contact_refine_f32(const float *g2l_bf44, const float *xyz_b3m, const float *search_bf, int64_t B, int64_t M,
                           int64_t F, int64_t nz, int64_t ny, int64_t nx, const float *params8,
                           int32_t min_search_score, int32_t collision_threshold, const float *tables_2z3y2x,
                           const int64_t *count_b, const int64_t *frame_count_b, int32_t *counts_bfp3,
                           int32_t *kept_bf, float *score_bf, int32_t *fail_bf, int32_t *kept_index_bf,
                           int64_t *kept_count_b, void *workspace, size_t workspace_bytes, s4g_stream_t stream);

/* The neighbours of every point of a cloud (csrc/match_normals.hip; added under ABI 14): open3d's
 * search_hybrid_vector_3d(radius, max_nn) of a cloud's own points as s4g_estimate_normals_f32 runs it -- the live finite
 * points with fp32 squared distance < radius^2 (strict), of them the max_nn smallest by (squared distance, index), the
 * point itself included; a lower-index copy of a point therefore ranks before the point -- the indices alone.
 * cloud (B, 3, N) fp32; live_b int32 (B) or NULL as for s4g_estimate_normals_f32; 1 <= max_nn <= 64.
 * knn_bnk int32 (B, N, max_nn): the kept indices in rank order, -1 beyond their count; all -1 for a padding row and for
 * a point that is not finite.  Workspace: what s4g_estimate_normals_workspace_bytes gives for (B, N). */
int s4g_match_knn_f32(const float *cloud_b3n, const int32_t *live_b, int64_t B, int64_t N, float radius,
                      int32_t max_nn, int32_t *knn_bnk, void *workspace, size_t workspace_bytes, s4g_stream_t stream);

/* The reduce stage of the contact-object pipeline (csrc/contact_refine.hip; added under ABI 14): the fold of
 * data_gen/utils/smooth_contact_object.py:61-89, one wave per object.  frame_point_index (B, F) int32; offsets
 * (B, N + 1) and order (B, F) int32: a CSR whose row i lists, in ascending frame index, the frames that passed the
 * filter (:37) and whose point is i (:62); knn (B, N, max_nn) from s4g_match_knn_f32; count_b (device, may be NULL) the
 * points of object b.  Points are visited in ascending index with running counts num[]:
 *   more than frame_per_point frames: the first frame_per_point - num[i] are appended for i (:64); if more than
 *     min_rest frames remain beyond the first frame_per_point (:70-71), neighbour n of rank r takes frame rest[r] when
 *     n < i and num[n] < frame_per_point, or n > i and num[n] < max_neighbor_frame (:75-81); i itself takes nothing;
 *   1 .. frame_per_point frames: the first min(frame_per_point - num[i], len) are appended (:84).
 * Outputs in the script's append order: source_frame_bc, point_index_bc int32 (B, cap) -- the frame's row and the point
 * it now belongs to, the NEIGHBOUR for a spread frame -- then -1; count_out_b int64 (B) stays exact when it exceeds
 * cap, and flags_b int32 (B) bit 0 says so.  A row of the CSR whose point is outside [0, count) counts for nobody.
 * 1 <= frame_per_point <= 255, 0 <= max_neighbor_frame <= frame_per_point, 1 <= max_nn <= 8, min_rest >= max_nn - 1
 * (rest[r] then exists for every rank), 1 <= N <= 65 536 (the running counts are N bytes of LDS), B <= 65 535
 * (S4G_EINVAL otherwise).  No atomics, no workspace. */
int s4g_contact_reduce_i32(const int32_t *frame_point_index_bf, const int32_t *offsets_bn1, const int32_t *order_bf,
                           const int32_t *knn_bnk, const int64_t *count_b, int64_t B, int64_t N, int64_t F,
                           int32_t frame_per_point, int32_t max_neighbor_frame, int32_t min_rest, int32_t max_nn,
                           int64_t cap, int32_t *source_frame_bc, int32_t *point_index_bc, int64_t *count_out_b,
                           int32_t *flags_b, s4g_stream_t stream);

/* The view stage of the curvature model's fast label pipeline (csrc/precomputed_view.hip; added under ABI 14 with no
 * layout change): TorchPrecomputedSingleViewPointCloud.run_score
 * (data_gen/pcd_classes/torch_precomputed_single_view_point_cloud.py), without host synchronisation.  Both entry points
 * are run-to-run bit-identical and batch invariant: integer atomics and ballots only, no floating-point atomics.
 * P = L * T placements per point, index = depth * T + roll; 1 <= L <= 8, 1 <= T <= 16 (S4G_EINVAL otherwise).
 *
 * s4g_precomputed_select_f32 = _find_match (:130-178) with magic_formula (:180-185), one thread per view point.
 * nearest (B, N) int32 from s4g_match_nearest_f32 (run on the noise-free reference cloud); cloud (B, 3, N) the noisy
 * view; scene_normals (B, 3, M); camera (B, 3) the camera location; scene_frames (B, M, 3, 3) with the axes as COLUMNS;
 * search, inv_search (B, M, P) int32 and antipodal, inv_antipodal (B, M, P) fp32 the scene's scores.  Per view point,
 * i = nearest, or -1 where the noisy point is not finite:
 *   n = the normal of i by the rule of s4g_contact_select_f32: the scene normal, or (0, 0, 1) without one, n / |n| in
 *     double, turned towards the camera seen from the NOISY point; normals_b3n holds it rounded to fp32 once;
 *   flipped = n . frame[:, 0] > 0 (:163), formed in double from the unrounded n and the fp32 frame column;
 *   frames = the scene frame of i, columns 0 and 1 negated where flipped (:166); the scene's inv_frame is not read;
 *   pre_search / pre_antipodal = the scene's scores of i, the inv_* arrays where flipped (:167-170);
 *   mask = (double)pre_search > search_threshold and (double)pre_antipodal > antipodal_threshold (:181-183: numpy
 *     compares in float64, so the fp32 value 0.300000012 passes > 0.3);
 *   candidate = i >= 0, some mask bit set, and the noisy z > sample_region in fp32 (:172-174).
 *   i < 0: normal (0, 0, 1) turned towards the camera, the identity frame, scores 0, mask 0, no candidate.
 * Outputs: normals_b3n fp32 (B, 3, N); flipped_bn int32 (B, N); frames_bn33 fp32 (B, N, 3, 3); pre_search_bnp int32 and
 * pre_antipodal_bnp fp32 (B, N, P); mask_bnp bytes 0 / 1 (B, N, P); candidate_bn int32 (B, N); frame_index_bn int32
 * (B, N) the candidates in ascending order, then -1; frame_count_b int64 (B).  N, M < 2^30, M >= 1, B <= 65 535.
 * No workspace.
 *
 * s4g_precomputed_search_f32 = finger_hand (:277-396) with _table_collision_check (:258-275) for F candidate rows per
 * scene.  points (B, F, 3) the noisy view points, frames (B, F, 3, 3) (axes as COLUMNS), mask bytes, pre_search int32
 * and pre_antipodal fp32 (B, F, P) as the select call writes them; xyz (B, 3, M) fp32 and labels (B, M) int32 the dense
 * scene, a NaN point of which is in no region and in no slab; frame_count_b (device, may be NULL): only the first
 * frame_count_b[b] rows of scene b are frames.
 * params13 (HOST pointer) = {FINGER_LENGTH, BOTTOM_LENGTH, HALF_HAND_THICKNESS, HALF_BOTTOM_WIDTH, HALF_BOTTOM_SPACE,
 *   BACK_COLLISION_MARGIN, BACK_COLLISION_THRESHOLD, FINGER_COLLISION_THRESHOLD, CLOSE_REGION_MIN_POINTS,
 *   TABLE_HEIGHT + TABLE_COLLISION_OFFSET, NUM_POINTS_THRESHOLD, valid_search_min (1, :384), valid_antipodal_min
 *   (0.1, :385)}; tables_3l2t (DEVICE pointer) as for s4g_local_search_f32.
 * The only frame gate is mean |frame| < 1e-6 (:295): the reach gate of s4g_local_search_f32 does not exist in this
 * class.  [R^T | -R^T p], the table verdicts, the roll and every region test are those of s4g_local_search_f32, the
 * same operations in the same order: with an all-true mask the counts are its counts bit for bit.
 * A depth without a mask bit is skipped before its slab is counted (:305): slab 0.  A placement is graded when its
 * mask bit is set and its table verdict is clear (:327); its gates in the reference's order, every inequality strict:
 * slab >= params[10] (:312), back <= params[6] (:342), finger <= params[7] (:353), close >= params[8] (:363), one
 * label (:369).  A placement that passes takes search_score = pre_search, antipodal = pre_antipodal, objects_label =
 * the region's label; every other one 0 / 0 / no_label.
 * Outputs: ints_bfp6 int32 (B, F, P, 6) = {search_score, objects_label, back, finger, close, table_collision}, the
 *   counts 0 for a placement that was not graded; scores_bfp fp32 (B, F, P); slab_bfl int32 (B, F, L);
 *   valid_bf int32 (B, F): 0 where max(search_score) < params[11] or max(antipodal) < params[12] (:384), or the gate
 *   failed; valid_index_bf int32 (B, F) ascending, then -1; count_b int64 (B).
 * Every frame's row holds its own results only (the reference does not clear slot valid_grasp after a rejected frame).
 * M < 2^30, B and F <= 65 535.  Cost: every scene point is transformed for every frame with a mask bit, M * F * 18
 * flops; one sweep of the cloud, no second scan.
 * Workspace: s4g_precomputed_search_workspace_bytes(B, M, F, L, T) bytes, 256-byte aligned; contents need not be
 * initialised; every launch of the call is a kernel. */
int s4g_precomputed_select_f32(const int32_t *nearest_bn, const float *cloud_b3n, const float *scene_normals_b3m,
                               const float *camera_b3, const float *scene_frames_bm33, const int32_t *search_bmp,
                               const int32_t *inv_search_bmp, const float *antipodal_bmp,
                               const float *inv_antipodal_bmp, int64_t B, int64_t N, int64_t M, int64_t L, int64_t T,
                               double search_threshold, double antipodal_threshold, float sample_region,
                               float *normals_b3n, int32_t *flipped_bn, float *frames_bn33, int32_t *pre_search_bnp,
                               float *pre_antipodal_bnp, uint8_t *mask_bnp, int32_t *candidate_bn,
                               int32_t *frame_index_bn, int64_t *frame_count_b, s4g_stream_t stream);
size_t s4g_precomputed_search_workspace_bytes(int64_t B, int64_t M, int64_t F, int64_t L, int64_t T);
int s4g_precomputed_search_f32(const float *points_bf3, const float *frames_bf33, const uint8_t *mask_bfp,
                               const int32_t *pre_search_bfp, const float *pre_antipodal_bfp, const float *xyz_b3m,
                               const int32_t *labels_bm, int64_t B, int64_t M, int64_t F, int64_t L, int64_t T,
                               const float *params13, int32_t no_label, const float *tables_3l2t,
                               const int64_t *frame_count_b, int32_t *ints_bfp6, float *scores_bfp, int32_t *slab_bfl,
                               int32_t *valid_bf, int32_t *valid_index_bf, int64_t *count_b, void *workspace,
                               size_t workspace_bytes, s4g_stream_t stream);

/* The fast BASELINE labels (csrc/precomputed_view.hip; added under ABI 14 with no layout change):
 * TorchPrecomputedBaselinePointCloud.finger_hand with _table_collision_check
 * (data_gen/pcd_classes/torch_precomputed_baseline.py:227-348, 381-382) for F candidate rows per scene, without host
 * synchronisation.  Run-to-run bit-identical and batch invariant: integer atomics only, no memset, every launch of the
 * call is a kernel; graph-capturable.
 *
 * Inputs as for s4g_precomputed_search_f32, without pre_search and without labels: points (B, F, 3), frames
 * (B, F, 3, 3) (axes as COLUMNS), mask bytes (B, F, P) (`all_frame_bool`: pre_antipodal > 0.3 alone, :177-180),
 * pre_antipodal fp32 (B, F, P), xyz (B, 3, M) fp32, frame_count_b (device, may be NULL).
 * params11 (HOST pointer) = the first eleven of s4g_precomputed_search_f32's params13; tables_3l2t (DEVICE pointer).
 * The frame gate, [R^T | -R^T p], the table verdicts, the slab counters, the roll and every region test are those of
 * s4g_precomputed_search_f32 -- one sweep body compiled twice, here with three accumulator words per placement, no
 * label read and no atomicMin / atomicMax: back / finger / close / slab are its integers bit for bit.
 * Gates of a placement in the reference's order: depth without a mask bit (:275), slab >= params[10] (:282), table
 * verdict clear and mask bit set (:297), back <= params[6] (:312), finger <= params[7] (:323), close >= params[8]
 * (:333; as written: with params[8] <= 0 an empty close region passes, where s4g_precomputed_search_f32 needs a point
 * for its label).  There is NO label gate.  A placement that passes reads scores = pre_antipodal, every other one 0.
 * The fold (:337-348): over the L * T placements in flattened order, depths outer and rolls inner, the first one whose
 * score is > 0 and > every earlier taken one; a NaN is never taken.  The frame is valid when one was taken (:350);
 * there is no 1e-4 line as in s4g_best_placement_f32 (with a mask threshold >= 1e-4 the two agree).
 * Outputs: ints_bfp4 int32 (B, F, P, 4) = {back, finger, close, table_collision}; scores_bfp fp32 (B, F, P);
 *   slab_bfl int32 (B, F, L); index_bf int32 (B, F) the placement taken or -1; score_bf fp32 (B, F) its score or 0;
 *   g2l_bf44 fp32 (B, F, 4, 4) = LOCAL_TO_LOCAL_SEARCH[index] @ [R^T | -R^T p] (:381-382), the same fp32 operations as
 *   s4g_best_placement_f32, all 0 where invalid; valid_index_bf int32 (B, F) ascending, then -1; count_b int64 (B).
 * Every frame's row holds its own results only (no stale slots).  Limits: those of s4g_precomputed_search_f32.
 * Workspace: s4g_precomputed_baseline_search_workspace_bytes(B, M, F, L, T) bytes, 256-byte aligned; contents need
 * not be initialised. */
size_t s4g_precomputed_baseline_search_workspace_bytes(int64_t B, int64_t M, int64_t F, int64_t L, int64_t T);
int s4g_precomputed_baseline_search_f32(const float *points_bf3, const float *frames_bf33, const uint8_t *mask_bfp,
                                        const float *pre_antipodal_bfp, const float *xyz_b3m, int64_t B, int64_t M,
                                        int64_t F, int64_t L, int64_t T, const float *params11,
                                        const float *tables_3l2t, const int64_t *frame_count_b, int32_t *ints_bfp4,
                                        float *scores_bfp, int32_t *slab_bfl, int32_t *index_bf, float *score_bf,
                                        float *g2l_bf44, int32_t *valid_index_bf, int64_t *count_b, void *workspace,
                                        size_t workspace_bytes, s4g_stream_t stream);

/* The baselines' EVALUATION data (csrc/eval_data.hip; added under ABI 14 with no layout change):
 * EvalDataGenerator.run_collision (data_gen/eval/evaluation_data_generator.py) -- the candidate grasps found on a
 * rendered view alone, and the ground truth of each against the dense labelled scene -- without host synchronisation.
 * Both entry points are run-to-run bit-identical and batch invariant (integer atomics and fixed-order sums only),
 * graph-capturable, with no memset and no host read: every launch of a call is a kernel.
 *
 * s4g_eval_view_search_f32 = finger_hand_view (:228-330) with _table_collision_check (:209-226) for F frames of each of
 * B views.  points (B, F, 3), frames (B, F, 3, 3) (axes as COLUMNS), xyz (B, 3, N) fp32 the VIEW cloud itself,
 * frame_count_b (device, may be NULL), live_bf (device int32, may be NULL; 0 = the row is not scanned).
 * params12 (HOST pointer) = the eleven of s4g_precomputed_baseline_search_f32, then TABLE_HEIGHT;
 * tables_3l2t (DEVICE pointer) as for s4g_local_search_f32.
 * Per frame: the frame gate mean |frame| < 1e-6 (:242), the reach gate p.z + frame[2, 0] * FINGER_LENGTH < TABLE_HEIGHT
 * in fp32 (:244, the one s4g_local_search_f32 has and the precomputed classes lack), [R^T | -R^T p] and the table
 * verdicts as s4g_precomputed_baseline_search_f32 forms them.  The cloud sweep is that entry point's three-word sweep
 * body compiled again (csrc/pv_sweep.h) with every placement open: there is no mask and no looked-up score, and with
 * an all-true mask there back / finger / close / slab are the same integers bit for bit.
 * Gates of a placement, depths outer and rolls inner: slab >= params[10] (:258, a depth below it is skipped whole),
 * table verdict clear (:273), back <= params[6] (:287), finger <= params[7] (:298), close >= params[8] (:306).  The
 * FIRST placement that passes is taken (:322-330); there is no score, no label gate and no fold.
 * Outputs: ints_bfp4 int32 (B, F, P, 4) = {back, finger, close, table_collision}; slab_bfl int32 (B, F, L); index_bf
 *   int32 (B, F) the placement taken or -1; g2l_bf44 fp32 (B, F, 4, 4) = LOCAL_TO_LOCAL_SEARCH[index] @ [R^T | -R^T p]
 *   (:322-324) by the fp32 operations of s4g_best_placement_f32, all 0 where invalid; flags_bf int32 (B, F): 1 = not
 *   scanned (past frame_count_b or live == 0), 2 = the frame or its origin is not finite, 4 = frame gate, 8 = reach
 *   gate, 0 = searched; valid_index_bf int32 (B, F) ascending, then -1; count_b int64 (B).
 * A row that is not searched reads 0 / -1 everywhere.  A cloud point that is not finite is in no region.
 * Limits: those of s4g_precomputed_baseline_search_f32.  F == 0 sets count_b to 0 (by a kernel).
 * Workspace: s4g_eval_view_search_workspace_bytes(B, N, F, L, T), 256-byte aligned; contents need not be initialised.
 *
 * s4g_eval_scene_grade_f32 = finger_hand_scene (:332-391) with _antipodal_score (:161-186) for K poses of each of B
 * scenes.  g2l (B, K, 4, 4) fp32 global -> gripper (`baseline_frame`), xyz, normals (B, 3, M) fp32, labels (B, M)
 * int32, pose_count_b (device, may be NULL), live_bk (device int32, may be NULL; 0 = the row is not scanned).
 * params11 (HOST pointer) = the ten of s4g_eval_frames_f32, then NUM_POINTS_THRESHOLD.
 * local = g2l @ [p; 1], the region tests, the label test (minimum != maximum), the y extrema, the band rule and the
 * fixed-order band sums are those of s4g_eval_frames_f32 -- one body compiled twice (csrc/eval_sweep.h): back, finger,
 * close, the multi-label flag, the bands and the score are its bits wherever both reach the score.  Added: slab =
 * count(-BOTTOM_LENGTH < lx < FINGER_LENGTH), and this class's order of returns, reported as `stage`:
 *   1 slab < params[10] (:346); 2 back > params[6] (:360); 3 finger > params[7] (:371); 4 more than one distinct label
 *   in the close region (:381); 5 close < params[8] (:388); 0 scored (:391).
 *   non_collision = 0 at stages 1..3, else 1; single_label = 1 at stages 5 and 0, else 0 -- so an EMPTY close region has
 *   a single label, as written; the score is 0 unless stage is 0 (an empty region never reaches the score).
 * Outputs: ints_bk8 int32 (B, K, 8) = {slab, back, finger, close, distinct labels > 1, n_left, n_right, stage}, the four
 *   counts whatever the stage; non_collision_bk, single_label_bk uint8 (B, K); score_bk fp32 (B, K), NaN where a band is
 *   empty, as s4g_eval_frames_f32; floats_bk4 fp32 (B, K, 4) = {left_y, right_y, mean_left, mean_right}.
 * A row that is not scanned reads 0 everywhere.  A pose that is not finite is in no region: both booleans 0 and 16 is
 * added to its stage word.  Limits: those of s4g_eval_frames_f32.
 * Workspace: s4g_eval_scene_grade_workspace_bytes(B, M, K), 256-byte aligned; contents need not be initialised.
 *
 * Decisions of the pair (INTEGRATION.md has them at length).  (1) No stale slots.  (2) `frame` of the reference's dump
 * is the rigid inverse formed directly by the caller, not torch.inverse.  (3) A frame below the neighbour minimum is
 * not a candidate: this class's zero frame, which the caller expresses with live_bf.  (4) The eigenvector sign is that
 * of s4g_darboux_frames_f32.  (5) An empty close region has a single label.  (6) The crop of the view's close region
 * (s4g_close_region_f32) tests the composed g2l where the reference tests the unshifted slab. */
size_t s4g_eval_view_search_workspace_bytes(int64_t B, int64_t N, int64_t F, int64_t L, int64_t T);
int s4g_eval_view_search_f32(const float *points_bf3, const float *frames_bf33, const float *xyz_b3n, int64_t B,
                             int64_t N, int64_t F, int64_t L, int64_t T, const float *params12,
                             const float *tables_3l2t, const int64_t *frame_count_b, const int32_t *live_bf,
                             int32_t *ints_bfp4, int32_t *slab_bfl, int32_t *index_bf, float *g2l_bf44,
                             int32_t *flags_bf, int32_t *valid_index_bf, int64_t *count_b, void *workspace,
                             size_t workspace_bytes, s4g_stream_t stream);
size_t s4g_eval_scene_grade_workspace_bytes(int64_t B, int64_t M, int64_t K);
int s4g_eval_scene_grade_f32(const float *g2l_bk44, const float *xyz_b3m, const float *normals_b3m,
                             const int32_t *labels_bm, int64_t B, int64_t M, int64_t K, const float *params11,
                             const int64_t *pose_count_b, const int32_t *live_bk, int32_t *ints_bk8,
                             uint8_t *non_collision_bk, uint8_t *single_label_bk, float *score_bk, float *floats_bk4,
                             void *workspace, size_t workspace_bytes, s4g_stream_t stream);

/* The contact model's per-object frames (csrc/contact_pairs.hip): GenerateContactObjectData of
 * data_gen/data_generator/data_object_contact_point_generator.py for every object of a batch, without host
 * synchronisation.  Both entry points are run-to-run bit-identical and batch invariant: integer atomics and ballots
 * only, no floating-point atomics.
 *
 * s4g_contact_pairs_f32 = cache_contact_pair (:103-123).  xyz, normals (B, 3, N) fp32, the normals of unit length;
 * count_b (device, may be NULL): only the first count_b[b] points of object b are points.  Per i < j, in double from the
 * fp32 inputs and in the reference's operation order:
 *   d = |p_j - p_i|;  u = (p_j - p_i) / clip(d, 1e-4, 1);  c_ij = u . n_i;  c_ji = -u . n_j;  score = |c_ij * c_ji|;
 *   the pair is kept when d < max_distance (2 * HALF_BOTTOM_SPACE) and score > cos_threshold (0.95), both strict, both
 *   thresholds formed by the caller in double.  A point that is not finite, or at or past count_b[b], pairs with nothing.
 * Outputs: pairs_bp2 int32 (B, max_pairs, 2) in the order of np.nonzero(np.triu(...)): ascending i, then ascending j;
 *   pair_score_bp fp32 (B, max_pairs), the double rounded once; rows past the count are -1 / 0;
 *   pair_count_b int64 (B): the exact count, also when the list does not fit; flags_b int32 (B): bit 0 = more than
 *   max_pairs pairs (the first max_pairs are written, nothing past the end).
 * Two passes over the same predicate (count per row, the library's scan, write by ballot rank): the order does not
 * depend on arrival.  Cost: N * (N - 1) / 2 tests in double per object.
 * Limits: 1 <= N <= 2^20, B * N * (N - 1) / 2 < 2^31 (the scan is int32), max_pairs < 2^24, B <= 65 535 (S4G_EINVAL).
 * Workspace: s4g_contact_pairs_workspace_bytes(B, N); contents need not be initialised.
 *
 * s4g_contact_pair_grade_f32 = _estimate_grasp_quality with check_collision (:125-221) and get_frame_neighbor
 * (:79-86) over pairs_bp2 (B, P, 2), of which the first pair_count_b[b] (device, may be NULL: all P) are graded.
 * T rolls (theta_search, at most 16), W shifts (width_shift, at most 4).
 *   params5 (HOST) = {HALF_BOTTOM_WIDTH, HALF_BOTTOM_SPACE, BACK_COLLISION_MARGIN, BOTTOM_LENGTH, FINGER_LENGTH}, each
 *     formed in double and rounded to fp32 once;  gates3 (HOST, double) = {min_points, back_threshold, finger_threshold};
 *   tables_12t2w (DEVICE, 12 T + 2 W floats) = rows 0..2 of torch.inverse(local_search_to_local)[theta] (:29-40), then
 *     -HALF_HAND_THICKNESS + dw [W], HALF_HAND_THICKNESS + dw [W] rounded once.
 * Per pair, once, in double and rounded to fp32 once: y = (p_j - p_i) / |.|, x = e_y - (e_y . y) y normalised,
 * z = x cross y, c the midpoint, T = [R^T | -R^T c] (:139-152).  Per object point local = T p in fp32 as
 * s4g_eval_frames_f32 forms it; a point with |ly| >= HBW contributes nothing; close_plane = |ly| < HBS, finger plane =
 * HBS < |ly| < HBW; per roll s = L2LS[theta] local in fp32 in the same operation order; per roll and shift, with every
 * inequality strict: back = count(sx < margin & sx > -BOTTOM_LENGTH & z), finger = count(sx > margin & sx <
 * FINGER_LENGTH & z & finger plane), close = the same in the close plane, z = sz < HHT + dw & sz > -HHT + dw.
 * Gates, in the reference's order: a pair with close_plane < min_points has no frame.  Per roll, shifts in the given
 * order: skip one with back > back_threshold, then one with finger > finger_threshold, then one with close <
 * min_points, else acc += close / 3 (an fp32 division, an fp32 add).  `last` is the LAST shift's value (:194-214): 0
 * where that shift was skipped by a collision, its close count where it failed min_points alone.  The frame is valid
 * when acc >= min_points and last >= min_points; its score is min(acc, last), an exact fp32 function of integers.
 * Decisions.  (1) The frame is formed in double and its rigid inverse analytically, not by torch.inverse in fp32.
 *   (2) A pair whose frame is not finite (y parallel to e_y, coincident points, a point that is not finite) gets no
 *   frame and fail bit 0; the reference would propagate NaN.  (3) pair_score and antipodal_score are fp32, the double
 *   rounded once; the reference keeps float64.  (4) Thresholds and search lists are configuration with the reference's
 *   values as defaults, bounded by the small maxima above.
 * Dense outputs: counts_bptw3 int32 (B, P, T, W, 3) = {back, finger, close}, counted whatever the gates say;
 *   close_plane_bp int32 (B, P); score_bpt fp32, valid_bpt int32 (B, P, T); fail_bp int32 (B, P): bit 0 = the frame is
 *   not finite, bit 1 = close_plane < min_points, bit 2 = an index outside the object.  Rows at or past
 *   pair_count_b[b] read 0 everywhere.
 * Frames out (max_frames rows per object): the valid (pair, roll) in ascending pair * T + roll, the reference's append
 *   order: g2l_bf44 fp32 = L2LS[theta] @ T (:218); search_score_bf; antipodal_score_bf = pair_score_bp of the pair (0
 *   where that is NULL); frame_source_bf int32 = pair * T + roll; frame_point_index_bf int32: the object point nearest
 *   to the frame's centre, the translation of the rigid inverse of g2l, by fp32 squared distance in global coordinates
 *   (the arithmetic of s4g_match_nearest_f32, no radius), the lower index winning a tie.  Rows past the count are 0 /
 *   -1.  frame_count_b int64 (B): the exact count; flags_b int32 (B): bit 1 = more than max_frames frames.
 * Cost: every object point is transformed for every pair, N * P * 18 flops; a point inside the gripper's width then
 *   costs 14 flops per roll.  Limits: 1 <= N <= 2^20, P < 2^24, P * T < 2^30, max_frames < 2^30, B <= 65 535.
 * Workspace: s4g_contact_pair_grade_workspace_bytes(B, N, P, T, W); contents need not be initialised; every launch of
 * the call is a kernel. */
size_t s4g_contact_pairs_workspace_bytes(int64_t B, int64_t N);
int s4g_contact_pairs_f32(const float *xyz_b3n, const float *normals_b3n, const int64_t *count_b, int64_t B, int64_t N,
                          int64_t max_pairs, double max_distance, double cos_threshold, int32_t *pairs_bp2,
                          float *pair_score_bp, int64_t *pair_count_b, int32_t *flags_b, void *workspace,
                          size_t workspace_bytes, s4g_stream_t stream);
size_t s4g_contact_pair_grade_workspace_bytes(int64_t B, int64_t N, int64_t P, int64_t T, int64_t W);
int s4g_contact_pair_grade_f32(const float *xyz_b3n, const int64_t *count_b, const int32_t *pairs_bp2,
                               const float *pair_score_bp, const int64_t *pair_count_b, int64_t B, int64_t N, int64_t P,
                               int64_t T, int64_t W, const float *params5, const double *gates3,
                               const float *tables_12t2w, int64_t max_frames, int32_t *counts_bptw3,
                               int32_t *close_plane_bp, float *score_bpt, int32_t *valid_bpt, int32_t *fail_bp,
                               float *g2l_bf44, float *search_score_bf, float *antipodal_score_bf,
                               int32_t *frame_source_bf, int32_t *frame_point_index_bf, int64_t *frame_count_b,
                               int32_t *flags_b, void *workspace, size_t workspace_bytes, s4g_stream_t stream);

/* The curvature (Darboux) model's per-object data (csrc/darboux.hip, csrc/darboux_object.hip): GenerateDarbouxObjectData
 * of data_gen/data_generator/data_object_darboux_generator.py for every object of a batch, without host
 * synchronisation.  Both entry points are run-to-run bit-identical and batch invariant: fixed summation order, integer
 * atomics and ballots only, no floating-point atomics.  xyz, normals (B, 3, N) fp32; count_b (device, may be NULL): only
 * the first count_b[b] points of object b are points.
 *
 * s4g_darboux_object_frames_f32 = _estimate_frame (:62-92) for every point.  Neighbours: squared distance < radius^2 in
 * fp32, the point itself included, over the ordered cell grid of s4g_darboux_frames_f32 (a cell's records are read in
 * ascending point index; points at or past count_b[b] are binned but never neighbours, so they should be finite: an
 * object with a point that is not finite is scanned in index order -- the same sets, sums in another order).  In double:
 * n = the neighbours' mean normal, normalised (:73-74); centroid = M mean with M = I - (n.n), the SCALAR n.n taken off
 * every entry of the identity as the reference's 1-D `normal.T @ normal` does (:80-81), i.e. centroid_i = mean_i -
 * (n.n) (mean_x + mean_y + mean_z); cov = sum of (normal - centroid)(normal - centroid)^T (:82-83), rounded to fp32
 * once scaled by its trace; its smallest eigenvector by cyclic Jacobi in fp32 as s4g_darboux_frames_f32 runs it;
 * minor = e - (e.n) n normalised with that entry point's sign rule; principal = minor x n.  frames_bn33 = columns
 * [-n, -principal, minor], inv_frames_bn33 = [n, principal, minor], each rounded to fp32 once.  neighbours_bn int32 the
 * neighbour count; flags_bn int32: 1 = estimated, 2 = degenerate or not finite, 4 = fewer than min_neighbours; with 2
 * and 4, and for rows at or past count_b[b] (flags 0), both frames are ZERO (:75-78; not the identity of the view class).
 * Limits: 1 <= N <= 65 536 (the grid's bitmap; S4G_EINVAL beyond), B <= 65 535.
 * Workspace: s4g_darboux_object_frames_workspace_bytes(B, N); contents need not be initialised.
 *
 * s4g_darboux_object_grade_f32 = _estimate_grasp_quality with finger_hand_view and _antipodal_score (:94-247).  F frames
 * per object at the points frame_index_bf (device, int32, may be NULL: frame f sits at point f; an index outside
 * [0, count_b[b]) fails the row), each in two directions: frames_bf33 and inv_frames_bf33 (B, F, 3, 3), axes as columns.
 * L depths, T rolls, S shifts of the hand along its thickness in the reference's loop order (at most 8, 16, 4).
 *   params9 (HOST) = {HALF_BOTTOM_WIDTH, HALF_BOTTOM_SPACE, BACK_COLLISION_MARGIN, BACK_COLLISION_THRESHOLD,
 *     FINGER_COLLISION_THRESHOLD, CLOSE_REGION_MIN_POINTS, NEIGHBOR_DEPTH, NUM_POINTS_THRESHOLD, HALF_HAND_THICKNESS +
 *     max |dz|};  tables_3l2t2s (DEVICE) = dl [L], dl - BOTTOM_LENGTH [L], dl + FINGER_LENGTH [L], cos [T], sin [T] as
 *     for s4g_local_search_f32, then -HALF_HAND_THICKNESS + dz [S], HALF_HAND_THICKNESS + dz [S] rounded once.
 * Per (frame, direction): global -> local is [R^T | -R^T p] formed as s4g_local_search_f32 forms it (no fp32
 * torch.inverse); a frame with mean |entry| < 1e-6 (:136) or that is not finite gets zero scores and fail = 1 (the
 * reference raises).  Per depth: slab = count(lx < dl + FL & lx > dl - BL); below NUM_POINTS_THRESHOLD its T placements
 * stay 0 (:153).  Per placement and shift, every inequality strict, on the rolled slab points: z = zz < HHT + dz & zz >
 * -HHT + dz; back = z & |yy| < HBW & lx - dl < -margin; finger = z & HBS < |yy| < HBW; close = z & |yy| < HBS.  Shifts in
 * order: skip on back > threshold, then on finger > threshold; close_num = close; skip on close_num < min points; else
 * single = mean |n.y| left band * mean right band (:223-247; empty band: NaN), temp_antipodal += single / 3, temp_search
 * += close_num / 3 (fp32 divisions and adds).  search = int(min(temp_search, close_num)) by truncation, antipodal =
 * min(temp_antipodal, single) with NaN propagating: close_num and single are those of the LAST shift that got that far
 * (:200,211,215-218).  There is no table gate and no label gate.
 * Outputs: search_bf2lt int32, antipodal_bf2lt fp32 (B, F, 2, L, T); counts_bf2lts3 int32 (B, F, 2, L, T, S, 3) = {back,
 * finger, close}, counted whatever the gates say; slab_bf2l int32 (B, F, 2, L); fail_bf2 int32 (B, F, 2).  A failed row
 * reads 0 everywhere else.
 * Cost: every object point is transformed for every row, N * 2 F * 18 flops; a point inside the cull costs 6 flops per
 * roll.  Limits: N < 2^30, B * F * 2 * L * T * S <= 2^27, B <= 65 535 (S4G_EINVAL).
 * Workspace: s4g_darboux_object_grade_workspace_bytes(B, N, F, L, T, S) (0 for lists beyond the maxima); contents need
 * not be initialised; every launch of the call is a kernel. */
size_t s4g_darboux_object_frames_workspace_bytes(int64_t B, int64_t N);
int s4g_darboux_object_frames_f32(const float *xyz_b3n, const float *normals_b3n, const int64_t *count_b, int64_t B,
                                  int64_t N, float radius, int32_t min_neighbours, float *frames_bn33,
                                  float *inv_frames_bn33, int32_t *neighbours_bn, int32_t *flags_bn, void *workspace,
                                  size_t workspace_bytes, s4g_stream_t stream);
size_t s4g_darboux_object_grade_workspace_bytes(int64_t B, int64_t N, int64_t F, int64_t L, int64_t T, int64_t S);
int s4g_darboux_object_grade_f32(const float *xyz_b3n, const float *normals_b3n, const int64_t *count_b,
                                 const float *frames_bf33, const float *inv_frames_bf33, const int32_t *frame_index_bf,
                                 int64_t B, int64_t N, int64_t F, int64_t L, int64_t T, int64_t S, const float *params9,
                                 const float *tables_3l2t2s, int32_t *search_bf2lt, float *antipodal_bf2lt,
                                 int32_t *counts_bf2lts3, int32_t *slab_bf2l, int32_t *fail_bf2, void *workspace,
                                 size_t workspace_bytes, s4g_stream_t stream);

/* ---- next row f3: cloud pre-processing on device -------------------------
 * Single-scene passes in front of the network (reference
 * grasp_proposal/cloud_processor/cloud_processor.py:12-42, constants
 * configs/processing_config.py:17-23, caller grasp_detector.py:94-105).  The
 * reference delegates voxelisation and outlier removal to open3d (>= 0.12,
 * absent here) and discards their results; the semantics below restate open3d's
 * published algorithms (oracle/preprocess.py; parity unpinned).
 *
 * s4g_crop_indices_f32: CloudPreProcessor.filter_work_space (:12-29).
 *   workspace6 = {lo_x, hi_x, lo_y, hi_y, lo_z, hi_z} (HOST pointer); index_n
 *   receives the ascending indices of the points strictly inside the box,
 *   *count (device) their number.
 * s4g_voxel_down_sample_f32: CloudPreProcessor.voxelize (:38-41) = open3d
 *   VoxelDownSample.  origin3 / dims3 are HOST pointers: origin = min(points) -
 *   voxel/2, dims = cells per axis (product < 2^32); a NaN or infinite origin
 *   (the bound of a cloud with such a coordinate: crop first) is S4G_EINVAL, as
 *   are voxel <= 0 and dims <= 0.  out_3n is (3, N) with row
 *   stride N: the first *count columns hold the cell means (double sum in point
 *   order, rounded once), cells in ascending (iz, iy, ix) order.
 * s4g_radius_outlier_mask_f32: CloudPreProcessor.remove_outliers (:31-36) = open3d
 *   RemoveRadiusOutliers.  keep_n[j] = 1 iff more than nb_points points (j itself
 *   included) lie at squared distance < radius^2 (canonical fp32 arithmetic).
 *   Workspace: s4g_radius_outlier_workspace_bytes(N) (0 for N > 65536: scan). */
/* ABI 12: the library's own device primitives behind the deterministic scatters and the voxel down-sample (round 6:
 * csrc/radix_sort.hip replaces rocPRIM's): a STABLE least-significant-digit radix sort of n (uint32 key, uint32 value)
 * pairs on the low `bits` key bits (8 bits per pass; equal keys keep their input order) -- result in keys_out / vals_out,
 * keys_in / vals_in are clobbered -- and an int32 exclusive scan (out must not alias in).  No counterpart in the
 * reference (which leaves order to atomicAdd / open3d's hash map). */
size_t s4g_sort_pairs_workspace_bytes(int64_t n);
int s4g_sort_pairs_u32(uint32_t *keys_in, uint32_t *vals_in, int64_t n, int bits, uint32_t *keys_out,
                       uint32_t *vals_out, void *ws, size_t ws_bytes, s4g_stream_t stream);
size_t s4g_exclusive_scan_workspace_bytes(int64_t n);
int s4g_exclusive_scan_i32(const int32_t *in, int32_t *out, int64_t n, void *ws, size_t ws_bytes,
                           s4g_stream_t stream);

int s4g_crop_indices_f32(const float *xyz_3n, int64_t N, const float *workspace6,
                         int32_t *index_n, int32_t *count, s4g_stream_t stream);
size_t s4g_voxel_down_sample_workspace_bytes(int64_t N);
int s4g_voxel_down_sample_f32(const float *xyz_3n, int64_t N, float voxel,
                              const float *origin3, const int32_t *dims3, float *out_3n,
                              int32_t *count, void *ws, size_t ws_bytes, s4g_stream_t stream);
size_t s4g_radius_outlier_workspace_bytes(int64_t N);
int s4g_radius_outlier_mask_f32(const float *xyz_3n, int64_t N, float radius,
                                int32_t nb_points, uint8_t *keep_n, void *ws, size_t ws_bytes,
                                int flags, s4g_stream_t stream);

/* The view stage's first step for B views in one call (csrc/process_views.hip; added under ABI 14 with no layout
 * change): `processing_and_trace` of the data generator (data_gen/pcd_classes/
 * torch_precomputed_single_view_point_cloud.py:64-97) -- workspace crop, open3d's voxel_down_sample_and_trace over the
 * caller's bounds, remove_radius_outlier, and per kept row its index in the cloud that came in.  No host read; a
 * captured call is a plain chain of kernel nodes.
 *   xyz_b3n (B, 3, N) fp32; count_b (B,) int32 on the device or NULL: rows at or past count_b[b] (clamped to [0, N]) do
 *   not exist.  workspace6 / origin3 / dims3 are HOST pointers as in the three entries above: origin = min_bound -
 *   voxel / 2, dims = floor((max_bound - origin) / voxel) + 1.  The grid must contain the crop box (the cells of both
 *   faces of every axis lie in [0, dims - 1]; S4G_EINVAL otherwise): no kept point is clamped.
 *   Per scene the result equals s4g_crop_indices_f32 -> s4g_voxel_down_sample_f32 (same origin3 / dims3) ->
 *   s4g_radius_outlier_mask_f32 (same flags) bit for bit:
 *   points_out_b3n (B, 3, N): the kept voxel means in ascending (iz, iy, ix) cell order, NaN from column count on;
 *   index_out_bn (B, N) int32: per kept mean the HIGHEST original index among its voxel's points (open3d's trace
 *   matrix holds the last index added per octant; np.max(trace, axis=1) is the highest of the voxel), -1 from count on;
 *   counts_out_b3 (B, 3) int32: rows after the crop, voxels, kept means.
 * Limits: B <= 65 535, B * N < 2^31, cells < 2^32, 0 < radius < 1e18 (S4G_EINVAL).  Workspace:
 * s4g_process_views_workspace_bytes(B, N) bytes (S4G_EWORKSPACE below that), 256-byte aligned; contents undefined
 * between calls.  Every refusal happens before the first launch. */
size_t s4g_process_views_workspace_bytes(int64_t B, int64_t N);
int s4g_process_views_f32(const float *xyz_b3n, const int32_t *count_b /* may be NULL */, int64_t B, int64_t N,
                          const float *workspace6, float voxel, const float *origin3, const int32_t *dims3,
                          float radius, int32_t nb_points, float *points_out_b3n, int32_t *index_out_bn,
                          int32_t *counts_out_b3, void *ws, size_t ws_bytes, int flags, s4g_stream_t stream);

/* The rendered views the view stage starts from (csrc/render_views.hip; added under ABI 14 with no layout change):
 * data_gen/render/cycles_render.py:25-36, 118-153 without Blender -- a pinhole image of RAY LENGTHS per scene and
 * camera, unprojected along the unit rays of K^-1, cut at a planar depth, z negated and moved to the world frame; the
 * noisy cloud is the same from range * multiplier on the index set of the noise-free one.  The renderer is pinned by
 * this restatement alone (Cycles itself cannot be run against it).  B scenes x V cameras in one call; no host read; a
 * captured call is a plain chain of kernel nodes; run-to-run bit-identical; a scene's result does not depend on the
 * batch around it.
 *   tri_bt9 (B, T, 9) fp32 world-space triangles (three vertices, xyz each); tri_count_b (B,) int32 on the device or
 *   NULL: rows at or past tri_count_b[b] (clamped to [0, T]) do not exist and may hold anything.  cam_bv12 (B, V, 12)
 *   DOUBLE on the device: the camera-to-world rotation R row-major, then the camera centre c; the camera looks down its
 *   -z, +x is right, +y is up.  fx, fy, cx, cy: the pinhole; pixel i = row * W + col has x = col + 0.5, y = row + 0.5,
 *   row 0 is the LOWEST row.  noise_bvp (B, V, H * W) double multipliers of the range, or NULL.
 * Arithmetic, all in double from the fp32 inputs, each operation rounded once, sums left to right, no FMA:
 *   camera-frame vertex v = R^T (p - c) (v_i = R_0i d_0 + R_1i d_1 + R_2i d_2); e1 = v1 - v0, e2 = v2 - v0;
 *   ray r = ((x - cx) / fx, (y - cy) / fy, -1) from the origin, not normalised;
 *   P = r x e2, det = e1 . P, U = -(v0 . P), Q = -(v0 x e1), V = r . Q, Tn = e2 . Q;
 *   det > 0: hit iff U >= 0, V >= 0, U + V <= det, Tn > 0; det < 0: the four signs mirrored; det == 0 or a non-finite
 *   det, U, V or Tn never hits; both faces hit.  Planar depth t = Tn / det; the hit with the smallest t is taken, the
 *   lowest triangle index among equal t.  nor = sqrt(rx^2 + ry^2 + 1), range32 = (float)(t * nor), dir = (rx / nor,
 *   ry / nor, 1 / nor).  A pixel is kept iff it was hit and (double)range32 * (1 / nor) < max_depth.  Camera-frame
 *   point (range32 * dir.x, range32 * dir.y, -(range32 * dir.z)), world point R p + c (row i: R_i0 x + R_i1 y + R_i2 z
 *   + c_i) rounded to fp32 once; the noisy point the same from (double)range32 * noise.
 * Dense outputs: range_bvp (B, V, H * W) fp32, +inf on a miss; tri_bvp int32, -1 on a miss.  Compact outputs, the kept
 * pixels in ascending i: points_bv3p and noisy_bv3p (B, V, 3, H * W) fp32 (noisy_bv3p is not touched when noise_bvp is
 * NULL), pixel_bvp (B, V, H * W) int32, count_bv (B, V) int32; from count on NaN in the point arrays and -1 in
 * pixel_bvp (the conventions of s4g_process_views_f32's input and output).
 * Limits: B * V <= 65 535, 0 < H * W <= 2^22, T < 2^24, fx, fy > 0, all four pinhole values finite (S4G_EINVAL).
 * Workspace: s4g_render_views_workspace_bytes(B, V, T, H, W) bytes (0 outside the limits; S4G_EWORKSPACE below that),
 * 256-byte aligned; contents undefined between calls.  Every refusal happens before the first launch. */
size_t s4g_render_views_workspace_bytes(int64_t B, int64_t V, int64_t T, int64_t H, int64_t W);
int s4g_render_views_f32(const float *tri_bt9, const int32_t *tri_count_b /* may be NULL */, const double *cam_bv12,
                         int64_t B, int64_t V, int64_t T, double fx, double fy, double cx, double cy, double max_depth,
                         int64_t H, int64_t W, const double *noise_bvp /* may be NULL */, float *range_bvp,
                         int32_t *tri_bvp, float *points_bv3p, float *noisy_bv3p, int32_t *pixel_bvp, int32_t *count_bv,
                         void *ws, size_t ws_bytes, s4g_stream_t stream);

/* The training objective and metric of the three networks, fused (csrc/loss.hip; added under ABI 14 with no layout
 * change): PointNet2Loss / PointNet2Metric of the reference's network_models/models/PointNet2_tcls.py:156-267
 * (variant 0, the curvature model) and PointNet2.py:156-258 (variant 1, the contact and edge models), with
 * smooth_cross_entropy of nn_utils/functional.py:91-114.  One descriptor drives both entries; every tensor is
 * contiguous and on the device, predictions and gradients fp32.
 *   s4g_grasp_loss_f32: losses[4] = cls, R, t, mov, and the UNIT gradient of each loss with respect to its own
 *   prediction tensor (g_score / g_R / g_t / g_movable, in the tensors' shapes; a NULL pointer skips that store).
 *     cls, label_smoothing == 0: torch's weighted mean, sum_i w[y_i] nll_i / sum_i w[y_i]; label -100 is in neither sum.
 *     cls, label_smoothing > 0: s_c = [c == y](1 - ls) + ls / C, per point -sum_c s_c w_c logp_c (the weight by class),
 *       plain mean over B N.
 *     mov: mean |p - y| over B D N; gradient sign(p - y) / (B D N), sign(0) = 0.
 *     R: over the first F points, L1 = mean_9 (p - g)^2, L2 the same with channels 1, 2, 4, 5, 7, 8 of g negated,
 *       mean_{B F}(min(L1, L2) scene_score) 5; a tie takes L1; the gradient is zero from point F on.
 *     t: variant 0, cross entropy of frame_t[:, :, :F] against int64 labels (B, F), unweighted, -100 ignored, times 0.2;
 *       variant 1, mean_{B F}(sum_3 (p - g)^2 scene_score) 20 against fp32 labels (B, 3, F).
 *   A class label outside its range that is not -100 contributes nothing, gets a zero gradient and sets bit 0 of
 *   status[0] (bit 1 for best_frame_t); status[0] is written by every call.  F == 0, or every label ignored, gives NaN
 *   losses and zero gradients, as torch.  Non-finite predictions propagate through their own point only.
 *   s4g_grasp_metric_f32: cls_acc (B N) and mov_acc (B D N) floats of 0 / 1 (argmax with the lowest index on a tie;
 *   (p > 0.5) against int(label)), metrics[0] = R_err = mean_{B F}(scene_score min(angle, angle_inv)) with
 *   angle = acos(clamp((sum_9 g p - 1) / 2, -1, 1)), and t_acc (B F) for variant 0 or metrics[1] = t_err =
 *   mean sqrt(sum_3 (g - p)^2) for variant 1.
 * The result is a function of the inputs alone: per-point terms in fp32, one double partial per loss and fixed tile of
 * 1 024 points, the partials summed in tile order by one workgroup and rounded to fp32 once; no float atomics.
 * Limits: 1 <= B <= 65 535, N >= 1, B N < 2^31, 0 <= F <= N, 2 <= C <= 8, 1 <= D <= 8, 2 <= Ct <= 8 (variant 0) or
 * Ct == 3 (variant 1), scene_score_stride >= F, 0 <= label_smoothing < 1 (S4G_EINVAL).  Workspace:
 * s4g_grasp_loss_workspace_bytes(B, N, F) bytes (0 outside the limits; S4G_EWORKSPACE below that), 256-byte aligned;
 * contents undefined between calls.  Every refusal happens before the first launch; no host read. */
typedef struct s4g_loss_desc {
  int32_t variant;                /* 0 curvature, 1 contact */
  int32_t B, N, F, C, D, Ct;
  int32_t scene_score_stride;     /* floats between the rows of scene_score */
  float label_smoothing;
  float w[8];                     /* class weights of the score loss, w[0 .. C) */
  const float *score_logits;      /* (B, C, N) */
  const float *movable;           /* (B, D, N), after the sigmoid */
  const float *frame_R;           /* (B, 9, N) */
  const float *frame_t;           /* (B, Ct, N) */
  const int64_t *score_labels;    /* (B, N) */
  const float *movable_labels;    /* (B, D, N) */
  const float *best_frame_R;      /* (B, 9, F) */
  const void *best_frame_t;       /* variant 0: int64 (B, F); variant 1: fp32 (B, 3, F) */
  const float *scene_score;       /* (B, >= F): row b starts at b * scene_score_stride */
  float *losses;                  /* loss entry: 4 */
  float *g_score, *g_movable, *g_R, *g_t; /* loss entry: may be NULL */
  int32_t *status;                /* loss entry: 1 */
  float *cls_acc, *mov_acc, *t_acc;       /* metric entry: (B N), (B D N), (B F; variant 0) */
  float *metrics;                 /* metric entry: 2 = R_err, t_err (0 for variant 0) */
  void *ws;
  size_t ws_bytes;
} s4g_loss_desc_t;
size_t s4g_grasp_loss_workspace_bytes(int64_t B, int64_t N, int64_t F);
int s4g_grasp_loss_f32(const s4g_loss_desc_t *desc, s4g_stream_t stream);
int s4g_grasp_metric_f32(const s4g_loss_desc_t *desc, s4g_stream_t stream);

/* ---------------------------------------------------------------------------
 * The operators in DOUBLE (ABI >= 8).  The reference's extension dispatches every kernel over float and
 * double (AT_DISPATCH_FLOATING_TYPES: sampling_kernel.cu:148-167, ball_query_kernel.cu:116-128,
 * grouping_kernel.cu:48-51,136-150, interpolate_kernel.cu:114-126,212-232,317-338).  Same layouts, index
 * types, tie rules and padding as the *_f32 entry points; plain kernels (S4G never uses double).
 *   s4g_fps_f64: ws = (B, N) doubles (the reference's `temp`), ws_bytes >= 8 B N.
 *   s4g_ball_query_f64: `radius` is a C float as in ball_query.h and is cast to double before squaring.
 *   s4g_three_nn_f64: the reference's initial distance 1e40 is FINITE in double: a slot no key entered reports it
 *     (not +inf), a key 1e20 or more away enters nowhere, and the initialiser -1 can sit in any of the three slots
 *     (one or two keys nearer than 1e20): each reports index 0, as every 3-NN entry point does (s4g_three_nn_f32).
 *   The two backwards refuse a NULL argument before gin is zero-filled.
 *   gather_points = group_points with K == 1.  Inverse-distance weights: torch ops in the caller.
 * ------------------------------------------------------------------------- */
int s4g_fps_f64(const double *xyz_b3n, int64_t B, int64_t N, int64_t M, int64_t *idx_bm, void *ws,
                size_t ws_bytes, int flags, s4g_stream_t stream);
int s4g_ball_query_f64(const double *xyz_b3n, const double *ctr_b3m, int64_t B, int64_t N, int64_t M,
                       float radius, int64_t K, int64_t *idx_bmk, int64_t *cnt_bm, int flags,
                       s4g_stream_t stream);
int s4g_three_nn_f64(const double *query_b3n1, const double *key_b3n2, int64_t B, int64_t N1, int64_t N2,
                     int64_t *idx_bn3, double *d2_bn3, int flags, s4g_stream_t stream);
int s4g_group_points_f64(const double *in_bcn, const int64_t *idx_bmk, int64_t B, int64_t C, int64_t N,
                         int64_t M, int64_t K, double *out_bcmk, s4g_stream_t stream);
int s4g_group_points_backward_f64(const double *gout_bcmk, const int64_t *idx_bmk, int64_t B, int64_t C,
                                  int64_t N, int64_t M, int64_t K, double *gin_bcn, s4g_stream_t stream);
int s4g_three_interpolate_f64(const double *feat_bcn2, const int64_t *idx_bn3, const double *w_bn3,
                              int64_t B, int64_t C, int64_t N2, int64_t N1, double *out_bcn1, int flags,
                              s4g_stream_t stream);
int s4g_three_interpolate_backward_f64(const double *gout_bcn1, const int64_t *idx_bn3,
                                       const double *w_bn3, int64_t B, int64_t C, int64_t N2, int64_t N1,
                                       double *gin_bcn2, s4g_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* S4G_OPS_H_ */
