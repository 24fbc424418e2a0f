// The evaluation data of the baselines: EvalDataGenerator.run_collision (data_gen/eval/evaluation_data_generator.py),
// which the reference drives as two Python loops -- finger_hand_view per sampled frame against the view cloud, then
// finger_hand_scene per valid grasp against the dense labelled scene -- restated for every frame of every view and
// every pose of every scene.  Contract: include/s4g_ops.h (s4g_eval_view_search_f32, s4g_eval_scene_grade_f32).
//
// s4g_eval_view_search_f32 = finger_hand_view (:228-330) with _table_collision_check (:209-226).  Per frame the FIRST
// placement, depths outer and rolls inner, that passes every gate is taken (:322-330): there is no score, no label gate
// and no "best".
//   evd_setup_kernel    per frame: the frame gate (:242), the reach gate (:244), [R^T | -R^T p] and the L * T table
//                       verdicts exactly as pv_setup_kernel / ls_setup_kernel form them, per depth the open rolls = table
//                       clear (there is no mask: every depth's slab is counted), the accumulators' neutral values
//   evd_scan_kernel     ONE sweep of the view cloud: pv_scan (pv_sweep.h) in its three-word form, the body that
//                       s4g_precomputed_baseline_search_f32 compiles: back / finger / close / slab are its integers
//   evd_finish_kernel   the gates in the reference's order (:258,273,287,298,306), the first passing placement by one
//                       thread, the matrix LOCAL_TO_LOCAL_SEARCH[i] @ global_to_local (:322-324, best_placement_g2l)
//   compact_valid_kernel
//
// s4g_eval_scene_grade_f32 = finger_hand_scene (:332-391) with _antipodal_score (:161-186).
//   eval_init_kernel    (eval_sweep.h) the per-pose accumulators to their neutral values
//   evs_scan_kernel     eval_scan (eval_sweep.h) with the slab counter: the body of s4g_eval_frames_f32's first scan
//   evs_band_kernel     eval_band with THIS class's gate: only poses that reach :391 are swept a second time
//   evs_finish_kernel   the line at which the reference returned (`stage`), the two booleans, the score
//
// Decisions.  (1) No stale slots: every frame's row holds its own results.  (2) The rigid inverse of a taken matrix is
// the caller's, formed directly, not by torch.inverse (:95).  (3) A frame below the neighbour minimum keeps this
// class's ZERO frame (:63) and fails the frame gate; the caller passes live = 0 for it.  (4) The eigenvector sign is
// that of s4g_darboux_frames_f32.  (5) An empty close region has a single label, as written (:379-384).  (6) A frame,
// origin or pose that is not finite makes its row invalid and is flagged; a cloud point that is not finite is in no
// region.
//
// Limits: N, M < 2^30, B <= 65 535, F <= 65 535, B * F * L * T <= 2^26 (those of s4g_precomputed_baseline_search_f32);
// B * K <= 2^27 (that of s4g_eval_frames_f32).
#include "eval_sweep.h"
#include "pv_sweep.h"

namespace s4g {

// ---- the view search -------------------------------------------------------------------------------------------------
constexpr int EVD_GX = 32;           // workgroups that share a view's frame list (frame k belongs to workgroup k mod 32)
constexpr int EVD_U = 4;             // points per lane held in registers while the workgroup's frames pass over them
// frames per workgroup and pass: the three-word sweep of s4g_precomputed_baseline_search_f32 with its LDS budget
// (20 * 128 * 3 * 4 = 30 KiB, four workgroups per CU).  Taken over from there, not tuned here.
constexpr int EVD_SLOTS = 20;
constexpr int EVD_CHUNK_POINTS = 16384;  // point ranges per view: ceil(N / 16 384) within [4, 64]
constexpr int EVD_MIN_CHUNKS = 4;
constexpr int EVD_MAX_CHUNKS = 64;
constexpr int EVD_ACC = 3;           // per placement: back, finger, close

// flags_bf bits
constexpr int EVD_FLAG_NOT_SCANNED = 1;   // past frame_count_b or live == 0
constexpr int EVD_FLAG_NOT_FINITE = 2;    // the frame or its origin holds a NaN or an infinity
constexpr int EVD_FLAG_FRAME_GATE = 4;    // mean |frame| < 1e-6 (:242)
constexpr int EVD_FLAG_REACH_GATE = 8;    // p.z + frame[2, 0] * FINGER_LENGTH < TABLE_HEIGHT (:244)

// words (B, F, L, 2) unsigned as pv_scan reads them: [0] the rolls of the depth whose box clears the table, bit 31 set
// for every depth of a frame that is scanned; [1] the rolls whose box meets the table
__global__ __launch_bounds__(64) void evd_setup_kernel(
    const float* __restrict__ points, const float* __restrict__ frames, const float* __restrict__ tables, int F,
    PvParams p, float table_height, const int64_t* __restrict__ frame_count, const int* __restrict__ live,
    float* __restrict__ hdr, int* __restrict__ acc, int* __restrict__ slab, unsigned* __restrict__ words,
    int* __restrict__ flags) {
  __shared__ unsigned opn[PV_MAX_L], tbl[PV_MAX_L];
  const int b = blockIdx.y, f = blockIdx.x, lane = threadIdx.x;
  const size_t row = (size_t)b * F + f;
  float r[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) r[i] = frames[row * 9 + i];
  const float px = points[row * 3], py = points[row * 3 + 1], pz = points[row * 3 + 2];
  int flag = 0;
  if (!(f < frame_rows(frame_count, b, F)) || (live && live[row] == 0)) flag = EVD_FLAG_NOT_SCANNED;
  if (!flag) {
    bool fin = isfinite(px) && isfinite(py) && isfinite(pz);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      fin = fin && isfinite(r[i]);
      s = s + fabsf(r[i]);
    }
    if (!fin) flag = EVD_FLAG_NOT_FINITE;
    else if (__fdiv_rn(s, 9.0f) < 1e-6f) flag = EVD_FLAG_FRAME_GATE;                  // :242
    else if (__fadd_rn(pz, __fmul_rn(r[6], p.fl)) < table_height) flag = EVD_FLAG_REACH_GATE;   // :244
  }
  const bool ok = flag == 0;
  if (lane < PV_MAX_L) opn[lane] = tbl[lane] = 0u;
  __syncthreads();
  const int P = p.L * p.T;
  for (int pl = lane; pl < P; pl += 64) {
    const int d = pl / p.T, t = pl % p.T;
    const float dl = tables[d], c = tables[3 * p.L + t], sn = tables[3 * p.L + p.T + t];
    // row 2 of [R | p] @ LOCAL_SEARCH_TO_LOCAL[pl]: the inverse roll and the shift dl along the frame's x axis
    const float m0 = r[6], m1 = r[7] * c + r[8] * sn, m2 = r[7] * (-sn) + r[8] * c, m3 = r[6] * dl + pz;
    bool hit = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) {                                                    // GRIPPER_BOUND (config.py:58-64)
      const float cx = (k & 4) ? -p.bl : p.fl, cy = (k & 2) ? -p.hbw : p.hbw, cz = (k & 1) ? -p.hht : p.hht;
      hit = hit || (m0 * cx + m1 * cy + m2 * cz + m3 < p.table_limit);               // :225
    }
    if (ok && hit) atomicOr(&tbl[d], 1u << t);
    if (ok) atomicOr(&opn[d], (hit ? 0u : (1u << t)) | PV_DEPTH_MASKED);
    int* a = acc + (row * P + pl) * EVD_ACC;
#pragma unroll
    for (int w = 0; w < EVD_ACC; ++w) a[w] = acc_neutral(w);
  }
  __syncthreads();
  if (lane < p.L) {
    slab[row * p.L + lane] = 0;
    words[(row * p.L + lane) * 2] = opn[lane];
    words[(row * p.L + lane) * 2 + 1] = tbl[lane];
  }
  if (lane == 0) {
    float* h = hdr + row * PV_HDR;
#pragma unroll
    for (int i = 0; i < 3; ++i) {                                                    // row i of R^T = column i of R
      const float a = r[i], bb = r[3 + i], c = r[6 + i];
      h[4 * i] = a; h[4 * i + 1] = bb; h[4 * i + 2] = c;
      h[4 * i + 3] = -__fadd_rn(__fadd_rn(__fmul_rn(a, px), __fmul_rn(bb, py)), __fmul_rn(c, pz));
    }
    ((int*)h)[12] = ok ? 1 : 0;
    ((int*)h)[13] = ok ? 1 : 0;                        // every frame that passes its gates is scanned
    h[14] = h[15] = 0.f;
    flags[row] = flag;
  }
}

__global__ __launch_bounds__(256) void evd_scan_kernel(
    const float* __restrict__ xyz, const float* __restrict__ hdr, const unsigned* __restrict__ words,
    const float* __restrict__ tables, int N, int F, PvParams p, int* __restrict__ slab, int* __restrict__ acc,
    const int64_t* __restrict__ frame_count) {
  pv_scan<false, EVD_GX, EVD_U, EVD_SLOTS, EVD_ACC>(xyz, nullptr, hdr, words, tables, N, F, p, slab, acc, frame_count);
}

// one workgroup per frame, one thread per placement for the gates, every comparison as pvb_finish_kernel makes it; then
// ONE thread takes the first passing placement in flattened order, so the result does not depend on thread arrival
__global__ __launch_bounds__(PV_MAX_P) void evd_finish_kernel(
    const float* __restrict__ points, const float* __restrict__ frames, const float* __restrict__ tables,
    const float* __restrict__ hdr, const unsigned* __restrict__ words, const int* __restrict__ slab,
    const int* __restrict__ acc, int F, PvParams p, int* __restrict__ ints, int* __restrict__ slab_out,
    int* __restrict__ index, float* __restrict__ g2l) {
  __shared__ int ps[PV_MAX_P];
  const int b = blockIdx.y, f = blockIdx.x, pl = threadIdx.x;
  const int L = p.L, T = p.T, P = L * T;
  const size_t row = (size_t)b * F + f;
  const bool ok = ((const int*)(hdr + row * PV_HDR))[12] != 0;      // (0 for rows that are not scanned: evd_setup_kernel)
  if (pl < P) {
    int vi[4] = {0, 0, 0, 0};
    bool pass = false;
    if (ok) {
      const int d = pl / T, r = pl % T;
      const int* a = acc + (row * P + pl) * EVD_ACC;
      const bool open = (words[(row * L + d) * 2] >> r) & 1u;         // table verdict clear (:273)
      vi[0] = a[0]; vi[1] = a[1]; vi[2] = a[2];                      // (0 for a placement that was not graded)
      vi[3] = (words[(row * L + d) * 2 + 1] >> r) & 1u;
      pass = open && !((double)slab[row * L + d] < (double)p.slab_thr);               // :258
      pass = pass && !((double)a[0] > (double)p.back_thr);            // :287
      pass = pass && !((double)a[1] > (double)p.fing_thr);            // :298
      pass = pass && !((double)a[2] < (double)p.min_points);          // :306
    }
    int* oi = ints + (row * P + pl) * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) oi[c] = vi[c];
    ps[pl] = pass ? 1 : 0;
  }
  if (pl < L) slab_out[row * L + pl] = ok ? slab[row * L + pl] : 0;
  __syncthreads();
  if (pl != 0) return;
  int bi = -1;
  for (int i = 0; i < P; ++i)
    if (ps[i]) { bi = i; break; }                                     // :322-330: the first one returns
  index[row] = bi;
  float* o = g2l + row * 16;
  if (bi < 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = 0.f;
    return;
  }
  best_placement_g2l(frames + row * 9, points[row * 3], points[row * 3 + 1], points[row * 3 + 2], tables, L, T, bi, o);
}

// ---- the scene grade -------------------------------------------------------------------------------------------------
constexpr int EVS_GX = 16;           // workgroups that share a scene's pose list (pose k belongs to workgroup k mod 16)
constexpr int EVS_U = 4;             // points per lane held in registers while the workgroup's poses pass over them
constexpr int EVS_SLOTS = 32;        // poses per pass: the launch plan of s4g_eval_frames_f32, taken over, not tuned here
constexpr int EVS_MIN_CHUNKS = 8;    // point ranges per scene: ceil(M / 8 192) within [8, 64]
constexpr int EVS_MAX_CHUNKS = 64;
constexpr int EVS_CHUNK_POINTS = 8192;
constexpr int EVS_STAGE_NOT_FINITE = 16;  // in the stage word: the pose holds a NaN or an infinity

struct EvsParams {
  EvalParams e;
  float slab_thr;                    // NUM_POINTS_THRESHOLD
};

// the line at which finger_hand_scene returned, from a pose's accumulators: 0 scored (:391), 1 slab (:346), 2 back
// (:360), 3 finger (:371), 4 labels (:381), 5 few points (:388; an empty region never reaches _antipodal_score)
__device__ __forceinline__ int evs_stage(const int* __restrict__ a, const EvsParams& p) {
  if ((double)a[7] < (double)p.slab_thr) return 1;
  if ((double)a[0] > (double)p.e.back_threshold) return 2;
  if ((double)a[1] > (double)p.e.finger_threshold) return 3;
  if (a[2] > 0 && a[3] != a[4]) return 4;
  if ((double)a[2] < (double)p.e.min_points || a[2] <= 0) return 5;
  return 0;
}

struct EvsGate {
  EvsParams p;
  const int* live;
  __device__ __forceinline__ bool operator()(size_t row, const int* __restrict__ a) const {
    return (!live || live[row] != 0) && evs_stage(a, p) == 0;
  }
};

__global__ __launch_bounds__(256) void evs_scan_kernel(
    const float* __restrict__ xyz, const int* __restrict__ labels, const float* __restrict__ g2l, int M, int K,
    EvsParams p, int* __restrict__ acc, const int64_t* __restrict__ pose_count, const int* __restrict__ live) {
  eval_scan<true, EVS_GX, EVS_U, EVS_SLOTS>(xyz, labels, g2l, M, K, p.e.box, acc, pose_count, live, 0);
}

__global__ __launch_bounds__(256) void evs_band_kernel(
    const float* __restrict__ xyz, const float* __restrict__ normals, const float* __restrict__ g2l, int M, int K,
    EvsParams p, const int* __restrict__ acc, float* __restrict__ part, const int64_t* __restrict__ pose_count,
    const int* __restrict__ live) {
  eval_band<EVS_GX, EVS_U, EVS_SLOTS>(xyz, normals, g2l, M, K, p.e.box, p.e.neighbor_depth, EvsGate{p, live}, acc, part,
                                      pose_count, 0);
}

// one thread per pose row
__global__ __launch_bounds__(64) void evs_finish_kernel(
    const float* __restrict__ g2l, const int* __restrict__ acc, const float* __restrict__ part, int M, int K, int nchunk,
    EvsParams p, const int64_t* __restrict__ pose_count, const int* __restrict__ live, int* __restrict__ ints,
    unsigned char* __restrict__ non_collision, unsigned char* __restrict__ single_label, float* __restrict__ score,
    float* __restrict__ floats) {
  const int b = blockIdx.y;
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= K) return;
  const size_t row = (size_t)b * K + k;
  int vi[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float vf[4] = {0.f, 0.f, 0.f, 0.f};
  float sc = 0.f;
  int nc = 0, sl = 0;
  if (k < frame_rows(pose_count, b, K) && (!live || live[row] != 0)) {
    const int* a = acc + row * EV_ACC;
    bool fin = true;
#pragma unroll
    for (int c = 0; c < 12; ++c) fin = fin && isfinite(g2l[row * 16 + c]);
    const int stage = evs_stage(a, p);
    vi[0] = a[7]; vi[1] = a[0]; vi[2] = a[1]; vi[3] = a[2];
    vi[4] = (a[2] > 0 && a[3] != a[4]) ? 1 : 0;
    vi[7] = stage | (fin ? 0 : EVS_STAGE_NOT_FINITE);
    nc = (stage == 0 || stage >= 4) ? 1 : 0;                         // collision_bool starts at 1 (:202)
    sl = (stage == 0 || stage == 5) ? 1 : 0;                         // label_bool starts at 0 (:203), set at :384
    if (a[2] > 0) { vf[0] = ord2f(a[5]); vf[1] = ord2f(a[6]); }
    if (stage == 0) {
      const BandMeans m = eval_band_means(part + row * nchunk * 4, M, nchunk);
      vi[5] = m.n_left; vi[6] = m.n_right;
      vf[2] = m.mean_left; vf[3] = m.mean_right;
      sc = __fmul_rn(vf[2], vf[3]);                                  // :185; an empty band gives NaN there and here
    }
    if (!fin) { nc = 0; sl = 0; }                                   // (its counts are all 0: no comparison with a NaN holds)
  }
  int* oi = ints + row * 8;
#pragma unroll
  for (int c = 0; c < 8; ++c) oi[c] = vi[c];
#pragma unroll
  for (int c = 0; c < 4; ++c) floats[row * 4 + c] = vf[c];
  non_collision[row] = (unsigned char)nc;
  single_label[row] = (unsigned char)sl;
  score[row] = sc;
}

}  // namespace s4g

extern "C" size_t s4g_eval_view_search_workspace_bytes(int64_t B, int64_t N, int64_t F, int64_t L, int64_t T) {
  if (B <= 0 || N <= 0 || F <= 0 || L <= 0 || T <= 0 || L > s4g::PV_MAX_L || T > s4g::PV_MAX_T) return 0;
  return s4g::pv_layout((size_t)B, (size_t)F, (size_t)L, (size_t)T, s4g::EVD_ACC).total;
}

extern "C" int s4g_eval_view_search_f32(const float* points_bf3, const float* frames_bf33, const float* xyz_b3n,
                                        int64_t B, int64_t N, int64_t F, int64_t L, int64_t T, const float* params12,
                                        const float* tables_3l2t, const int64_t* frame_count_b, const int32_t* live_bf,
                                        int32_t* ints_bfp4, int32_t* slab_bfl, int32_t* index_bf, float* g2l_bf44,
                                        int32_t* flags_bf, int32_t* valid_index_bf, int64_t* count_b, void* workspace,
                                        size_t workspace_bytes, s4g_stream_t stream) {
  using namespace s4g;
  if (B < 0 || N <= 0 || F < 0 || B > 65535 || F > 65535 || N >= (1ll << 30)) return S4G_EINVAL;
  if (L <= 0 || T <= 0 || L > PV_MAX_L || T > PV_MAX_T) return S4G_EINVAL;
  if (B * F * L * T > (1ll << 26)) return S4G_EINVAL;       // (the limits of s4g_precomputed_baseline_search_f32)
  if (B == 0) return S4G_OK;
  if (!count_b) return S4G_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (F > 0) {
    if (!points_bf3 || !frames_bf33 || !xyz_b3n || !params12 || !tables_3l2t || !ints_bfp4 || !slab_bfl || !index_bf ||
        !g2l_bf44 || !flags_bf || !valid_index_bf)
      return S4G_EINVAL;
    if (!workspace || workspace_bytes < s4g_eval_view_search_workspace_bytes(B, N, F, L, T)) return S4G_EWORKSPACE;
    PvParams p;
    p.fl = params12[0]; p.bl = params12[1]; p.hht = params12[2]; p.hbw = params12[3]; p.hbs = params12[4];
    p.margin = params12[5]; p.back_thr = params12[6]; p.fing_thr = params12[7]; p.min_points = params12[8];
    p.table_limit = params12[9]; p.slab_thr = params12[10];
    p.valid_search_min = p.valid_antipodal_min = 0.f;         // (not read: this class has no validity line)
    p.r2lim = (p.hbw * p.hbw + p.hht * p.hht) * 1.0001f;      // as s4g_precomputed_search_f32
    p.L = (int)L; p.T = (int)T; p.no_label = 0;
    const PvLayout lay = pv_layout((size_t)B, (size_t)F, (size_t)L, (size_t)T, EVD_ACC);
    char* ws = (char*)workspace;
    float* hdr = (float*)(ws + lay.hdr);
    int* acc = (int*)(ws + lay.acc);
    int* slab = (int*)(ws + lay.slab);
    unsigned* words = (unsigned*)(ws + lay.words);
    const dim3 per_frame((unsigned)F, (unsigned)B);
    hipLaunchKernelGGL(evd_setup_kernel, per_frame, dim3(64), 0, st, points_bf3, frames_bf33, tables_3l2t, (int)F, p,
                       params12[11], frame_count_b, (const int*)live_bf, hdr, acc, slab, words, (int*)flags_bf);
    S4G_LAUNCH_CHECK();
    const dim3 grid(EVD_GX, (unsigned)sweep_chunks(N, EVD_CHUNK_POINTS, EVD_MIN_CHUNKS, EVD_MAX_CHUNKS), (unsigned)B);
    hipLaunchKernelGGL(evd_scan_kernel, grid, dim3(256), 0, st, xyz_b3n, (const float*)hdr, (const unsigned*)words,
                       tables_3l2t, (int)N, (int)F, p, slab, acc, frame_count_b);
    S4G_LAUNCH_CHECK();
    hipLaunchKernelGGL(evd_finish_kernel, per_frame, dim3(PV_MAX_P), 0, st, points_bf3, frames_bf33, tables_3l2t,
                       (const float*)hdr, (const unsigned*)words, (const int*)slab, (const int*)acc, (int)F, p,
                       (int*)ints_bfp4, (int*)slab_bfl, (int*)index_bf, g2l_bf44);
    S4G_LAUNCH_CHECK();
  }
  // (F == 0: the kernel reads and writes no row and sets the counts to 0 -- no memset node in a captured graph)
  hipLaunchKernelGGL(compact_valid_kernel<KeepNonNegative>, dim3((unsigned)B), dim3(256), 0, st, (const int*)index_bf,
                     (int)F, (int*)valid_index_bf, count_b);
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}

extern "C" size_t s4g_eval_scene_grade_workspace_bytes(int64_t B, int64_t M, int64_t K) {
  if (B <= 0 || M <= 0 || K <= 0) return 0;
  using namespace s4g;
  const size_t poses = (size_t)B * (size_t)K;
  const size_t nchunk = (size_t)sweep_chunks(M, EVS_CHUNK_POINTS, EVS_MIN_CHUNKS, EVS_MAX_CHUNKS);
  return align256(poses * EV_ACC * sizeof(int)) + poses * nchunk * 4 * sizeof(float);
}

extern "C" int s4g_eval_scene_grade_f32(const float* g2l_bk44, const float* xyz_b3m, const float* normals_b3m,
                                        const int32_t* labels_bm, int64_t B, int64_t M, int64_t K,
                                        const float* params11, const int64_t* pose_count_b, const int32_t* live_bk,
                                        int32_t* ints_bk8, uint8_t* non_collision_bk, uint8_t* single_label_bk,
                                        float* score_bk, float* floats_bk4, void* workspace, size_t workspace_bytes,
                                        s4g_stream_t stream) {
  using namespace s4g;
  if (B < 0 || M <= 0 || K < 0 || B > 65535 || M >= (1ll << 30) || K >= (1ll << 31)) return S4G_EINVAL;
  if (B * K > (1ll << 27)) return S4G_EINVAL;       // (the accumulator grid: 8 ints per pose row, 256 per workgroup)
  if (B == 0 || K == 0) return S4G_OK;
  if (!g2l_bk44 || !xyz_b3m || !normals_b3m || !labels_bm || !params11 || !ints_bk8 || !non_collision_bk ||
      !single_label_bk || !score_bk || !floats_bk4)
    return S4G_EINVAL;
  if (!workspace || workspace_bytes < s4g_eval_scene_grade_workspace_bytes(B, M, K)) return S4G_EWORKSPACE;
  EvsParams p = {{{params11[0], params11[1], params11[2], params11[3], params11[4], params11[5]},
                  params11[6], params11[7], params11[8], params11[9]},
                 params11[10]};
  hipStream_t st = (hipStream_t)stream;
  const int nchunk = sweep_chunks(M, EVS_CHUNK_POINTS, EVS_MIN_CHUNKS, EVS_MAX_CHUNKS);
  const int64_t poses = B * K;
  int* acc = (int*)workspace;
  float* part = (float*)((char*)workspace + align256((size_t)poses * EV_ACC * sizeof(int)));
  hipLaunchKernelGGL(eval_init_kernel, dim3((unsigned)((poses * EV_ACC + 255) / 256)), dim3(256), 0, st, acc, poses);
  S4G_LAUNCH_CHECK();
  const dim3 grid(EVS_GX, (unsigned)nchunk, (unsigned)B);
  hipLaunchKernelGGL(evs_scan_kernel, grid, dim3(256), 0, st, xyz_b3m, (const int*)labels_bm, g2l_bk44, (int)M, (int)K,
                     p, acc, pose_count_b, (const int*)live_bk);
  S4G_LAUNCH_CHECK();
  hipLaunchKernelGGL(evs_band_kernel, grid, dim3(256), 0, st, xyz_b3m, normals_b3m, g2l_bk44, (int)M, (int)K, p,
                     (const int*)acc, part, pose_count_b, (const int*)live_bk);
  S4G_LAUNCH_CHECK();
  hipLaunchKernelGGL(evs_finish_kernel, dim3((unsigned)((K + 63) / 64), (unsigned)B), dim3(64), 0, st, g2l_bk44,
                     (const int*)acc, (const float*)part, (int)M, (int)K, nchunk, p, pose_count_b,
                     (const int*)live_bk, (int*)ints_bk8, (unsigned char*)non_collision_bk,
                     (unsigned char*)single_label_bk, score_bk, floats_bk4);
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}
