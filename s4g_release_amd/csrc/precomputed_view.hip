// The view stage of the data generator's fast pipeline: TorchPrecomputedSingleViewPointCloud.run_score
// (data_gen/pcd_classes/torch_precomputed_single_view_point_cloud.py) restated for every view point of every scene.
// Contract: include/s4g_ops.h (s4g_precomputed_select_f32, s4g_precomputed_search_f32,
// s4g_precomputed_baseline_search_f32).
//
// s4g_precomputed_select_f32 = _find_match (:130-178) with magic_formula (:180-185) after the nearest-neighbour search
// (s4g_match_nearest_f32), one thread per view point: the scene normal of its nearest scene point turned towards the
// camera, the scene frame of that point (columns 0 and 1 negated where the normal points along column 0, :163-166), the
// scene's scores or, for a flipped point, its inv_* scores (:167-170), the placements that both thresholds recommend
// (:181-183, compared in double), and whether the point is a candidate: matched, a recommended placement, above the
// sample region (:172-174).
//   pv_select_kernel                      the above
//   compact_valid_kernel (frame_sweep.h)  frame_index: the candidates of a scene in ascending order, -1 padded, and their count
//
// s4g_precomputed_search_f32 = finger_hand (:277-396) with _table_collision_check (:258-275), which run_score (:232-235)
// drives as a Python loop over the candidate frames: only the recommended placements are collision-checked against the
// dense scene, and one that passes takes over the scene's scores.  No normals are read, no antipodal band is swept.
//   pv_setup_kernel    per frame: the gate (:295; there is NO reach gate in this class), [R^T | -R^T p] and the L*T table
//                      verdicts exactly as ls_setup_kernel forms them, per depth the open rolls = table clear AND mask,
//                      and the neutral values of the accumulators (no memset: every launch of the call is a kernel)
//   pv_scan_kernel     ONE cloud sweep (frame_sweep.h: points outer, frames inner): the slab counters of the depths
//                      that hold a mask bit (:305-312) and, per open placement, the counts behind the palm / in the
//                      fingers / in the close region and the label minimum / maximum -- five words, not the eight of
//                      local_search.hip: no y extrema, no band kernel; in LDS, then the workspace, integer atomics only
//   pv_finish_kernel   the gates in the reference's order (:327-371), the looked-up scores (:373-381), validity (:384)
//   compact_valid_kernel
//
// Decisions.  (1) No stale slots: every frame's row holds its own results (the reference does not clear slot valid_grasp
// after a rejected frame).  (2) local_to_global is formed directly by the caller, not by torch.inverse (:124).  (3) An
// unmatched or non-finite view point: normal (0, 0, 1) turned towards the camera, the identity frame, zero scores, never
// a candidate.  (4) The thresholds 50 and 0.3 are compared in double, as numpy compares them.  (5) Everything else stays
// as written; a view without candidates simply has frame_count 0.
// The slab counter of a depth runs when the depth holds a MASK bit (:305), whatever the table says about its rolls, as
// in the reference: with an all-true mask the slab counts are those of s4g_local_search_f32.
//
// s4g_precomputed_baseline_search_f32 = TorchPrecomputedBaselinePointCloud.finger_hand
// (data_gen/pcd_classes/torch_precomputed_baseline.py:246-348, 381-382), the baseline variant of the same lookup: the
// mask is the antipodal threshold alone (the caller's; stage A is s4g_precomputed_select_f32 with the search threshold
// at -inf), there is NO label gate, and a frame's result is the fold over its passing placements.
//   pv_setup_kernel<3>   as above, three neutral words per placement
//   pvb_scan_kernel      the same sweep body (pv_scan, compiled twice), three words: no label is read
//   pvb_finish_kernel    the gates (:275-333), the looked-up score, the fold (:337-348) by one thread, the matrix (:381)
//   compact_valid_kernel
// The crop and maps of the view (:350-380) are s4g_close_region_f32 with x in (0, FINGER_LENGTH).
//
// Limits: N, M < 2^30, B <= 65 535; for the searches F <= 65 535 as well (grid.x of the per-frame kernels).
#include "pv_sweep.h"

namespace s4g {

constexpr int PV_GX = 32;            // workgroups that share a scene's frame list (frame k belongs to workgroup k mod 32)
constexpr int PV_U = 4;              // points per lane held in registers while the workgroup's frames pass over them
// frames per workgroup and pass.  The accumulators are 5 words per placement where ls_scan_kernel keeps 8: 12 slots
// take 12 * 128 * 5 * 4 = 30 KiB of LDS, what 8 slots take there (32 KiB), so four workgroups still share a CU's
// 160 KiB while a pass covers 384 frames of a scene instead of 256 (a third fewer table loads, accumulator clears,
// flushes and cloud reads per frame).  16 slots (40 KiB) would drop a CU to three workgroups.
constexpr int PV_SLOTS = 12;
constexpr int PV_CHUNK_POINTS = 16384;   // point ranges per scene: ceil(M / 16 384) within [4, 64]
constexpr int PV_MIN_CHUNKS = 4;
constexpr int PV_MAX_CHUNKS = 64;
constexpr int PV_ACC = 5;            // per placement: back, finger, close, label min, label max (ACC_WORDS' prefix)
// The baseline class (s4g_precomputed_baseline_search_f32) has no label gate: its sweep keeps the three counts only.
// 20 * 128 * 3 * 4 = 30 KiB of LDS is what 12 five-word slots take, so four workgroups still share a CU and a pass
// covers 640 frames of a scene instead of 384.  20 is derived from that LDS budget alone: it is not a measured optimum,
// no other slot count has been timed.
constexpr int PVB_SLOTS = 20;
constexpr int PVB_ACC = 3;           // per placement: back, finger, close

// ---- stage A: one thread per view point ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pv_select_kernel(
    const int* __restrict__ nearest, const float* __restrict__ cloud, const float* __restrict__ scene_normals,
    const float* __restrict__ camera, const float* __restrict__ scene_frames, const int* __restrict__ search,
    const int* __restrict__ inv_search, const float* __restrict__ antipodal, const float* __restrict__ inv_antipodal,
    int N, int M, int P, double search_thr, double antipodal_thr, float sample_region, float* __restrict__ normals,
    int* __restrict__ flipped, float* __restrict__ frames, int* __restrict__ pre_search,
    float* __restrict__ pre_antipodal, unsigned char* __restrict__ mask, int* __restrict__ candidate) {
  const int b = blockIdx.y;
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= (size_t)N) return;
  const float* c0 = cloud + (size_t)b * 3 * N;
  const float vx = c0[q], vy = c0[(size_t)N + q], vz = c0[2 * (size_t)N + q];
  int i = nearest[(size_t)b * N + q];
  if (i >= M) i = -1;                                  // (cannot happen for s4g_match_nearest_f32's output)
  if (!(isfinite(vx) && isfinite(vy) && isfinite(vz))) i = -1;          // decision 3
  const Normal64 n = scene_normal_towards_camera(scene_normals + (size_t)b * 3 * M, M, i, c0, N, q,
                                                 camera + (size_t)b * 3);
  float* o = normals + (size_t)b * 3 * N;
  o[q] = (float)n.x;
  o[(size_t)N + q] = (float)n.y;
  o[2 * (size_t)N + q] = (float)n.z;
  const size_t row = (size_t)b * N + q;
  float r[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};           // :133
  bool flip = false;
  if (i >= 0) {
    const float* f = scene_frames + ((size_t)b * M + i) * 9;
#pragma unroll
    for (int c = 0; c < 9; ++c) r[c] = f[c];                             // :149
    // n . frame[:, 0] in double, from the unrounded normal (:163)
    flip = n.x * (double)r[0] + n.y * (double)r[3] + n.z * (double)r[6] > 0.0;
    if (flip) {                                                          // :166
      r[0] = -r[0]; r[3] = -r[3]; r[6] = -r[6];
      r[1] = -r[1]; r[4] = -r[4]; r[7] = -r[7];
    }
  }
#pragma unroll
  for (int c = 0; c < 9; ++c) frames[row * 9 + c] = r[c];
  flipped[row] = flip ? 1 : 0;
  bool any = false;
  if (i >= 0) {
    const size_t src = ((size_t)b * M + i) * P;
    const int* s = (flip ? inv_search : search) + src;                  // :167-170
    const float* a = (flip ? inv_antipodal : antipodal) + src;
    for (int pl = 0; pl < P; ++pl) {
      const int sv = s[pl];
      const float av = a[pl];
      const bool m = ((double)sv > search_thr) && ((double)av > antipodal_thr);    // :181-183
      pre_search[row * P + pl] = sv;
      pre_antipodal[row * P + pl] = av;
      mask[row * P + pl] = m ? 1 : 0;
      any = any || m;
    }
  } else {
    for (int pl = 0; pl < P; ++pl) {
      pre_search[row * P + pl] = 0;
      pre_antipodal[row * P + pl] = 0.f;
      mask[row * P + pl] = 0;
    }
  }
  candidate[row] = (any && vz > sample_region) ? 1 : 0;                  // :172-174 (i >= 0 is implied by `any`)
}

// ---- stage B ----------------------------------------------------------------------------------------------------------
// words (B, F, L, 2) unsigned: [0] the rolls of the depth that are graded (mask bit set, table verdict clear; bit 31:
// the depth holds a mask bit at all), [1] the rolls whose box meets the table
template <int ACC>
__global__ __launch_bounds__(64) void pv_setup_kernel(
    const float* __restrict__ points, const float* __restrict__ frames, const unsigned char* __restrict__ mask,
    const float* __restrict__ tables, int F, PvParams p, const int64_t* __restrict__ frame_count,
    float* __restrict__ hdr, int* __restrict__ acc, int* __restrict__ slab, unsigned* __restrict__ words) {
  __shared__ unsigned opn[PV_MAX_L], tbl[PV_MAX_L];
  const int b = blockIdx.y, f = blockIdx.x, lane = threadIdx.x;
  const size_t row = (size_t)b * F + f;
  float r[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) r[i] = frames[row * 9 + i];
  const float px = points[row * 3], py = points[row * 3 + 1], pz = points[row * 3 + 2];
  bool ok = f < frame_rows(frame_count, b, F);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 9; ++i) s = s + fabsf(r[i]);
  if (__fdiv_rn(s, 9.0f) < 1e-6f) ok = false;                                        // :295
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
      hit = hit || (m0 * cx + m1 * cy + m2 * cz + m3 < p.table_limit);               // :274
    }
    const bool mk = ok && mask[row * P + pl] != 0;
    if (ok && hit) atomicOr(&tbl[d], 1u << t);
    if (mk) atomicOr(&opn[d], (hit ? 0u : (1u << t)) | PV_DEPTH_MASKED);
    int* a = acc + (row * P + pl) * ACC;
#pragma unroll
    for (int w = 0; w < ACC; ++w) a[w] = acc_neutral(w);
  }
  __syncthreads();
  unsigned any = 0u;
  for (int d = 0; d < p.L; ++d) any |= opn[d];
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
    ((int*)h)[13] = (ok && any) ? 1 : 0;               // a frame without a mask bit is never scanned
    h[14] = h[15] = 0.f;
  }
}

// The sweep of both searches is pv_scan (pv_sweep.h, which s4g_eval_view_search_f32 compiles too): LABELS = true is the
// view stage's five-word form, LABELS = false the baseline's three-word form.
__global__ __launch_bounds__(256) void pv_scan_kernel(
    const float* __restrict__ xyz, const int* __restrict__ labels, const float* __restrict__ hdr,
    const unsigned* __restrict__ words, const float* __restrict__ tables, int N, int F, PvParams p,
    int* __restrict__ slab, int* __restrict__ acc, const int64_t* __restrict__ frame_count) {
  pv_scan<true, PV_GX, PV_U, PV_SLOTS, PV_ACC>(xyz, labels, hdr, words, tables, N, F, p, slab, acc, frame_count);
}

__global__ __launch_bounds__(256) void pvb_scan_kernel(
    const float* __restrict__ xyz, const float* __restrict__ hdr, const unsigned* __restrict__ words,
    const float* __restrict__ tables, int N, int F, PvParams p, int* __restrict__ slab, int* __restrict__ acc,
    const int64_t* __restrict__ frame_count) {
  pv_scan<false, PV_GX, PV_U, PVB_SLOTS, PVB_ACC>(xyz, nullptr, hdr, words, tables, N, F, p, slab, acc, frame_count);
}

// one workgroup per frame, one thread per placement
__global__ __launch_bounds__(PV_MAX_P) void pv_finish_kernel(
    const float* __restrict__ hdr, const unsigned* __restrict__ words, const int* __restrict__ slab,
    const int* __restrict__ acc, const int* __restrict__ pre_search, const float* __restrict__ pre_antipodal, int F,
    PvParams p, int* __restrict__ ints, float* __restrict__ scores, int* __restrict__ slab_out,
    int* __restrict__ valid) {
  const int b = blockIdx.y, f = blockIdx.x, pl = threadIdx.x;
  const int L = p.L, T = p.T, P = L * T;
  const size_t row = (size_t)b * F + f;
  const bool ok = ((const int*)(hdr + row * PV_HDR))[12] != 0;      // (0 for padding rows: pv_setup_kernel)
  int keep_s = 0, keep_a = 0;
  if (pl < P) {
    int vi[6] = {0, p.no_label, 0, 0, 0, 0};
    float score = 0.f;
    if (ok) {
      const int d = pl / T, r = pl % T;
      const int* a = acc + (row * P + pl) * PV_ACC;
      const bool open = (words[(row * L + d) * 2] >> r) & 1u;         // mask bit set and table verdict clear (:327)
      vi[2] = a[0]; vi[3] = a[1]; vi[4] = a[2];                      // (0 for a placement that was not graded)
      vi[5] = (words[(row * L + d) * 2 + 1] >> r) & 1u;
      bool pass = open && !((double)slab[row * L + d] < (double)p.slab_thr);          // :312
      pass = pass && !((double)a[0] > (double)p.back_thr);            // :342
      pass = pass && !((double)a[1] > (double)p.fing_thr);            // :353
      pass = pass && !((double)a[2] < (double)p.min_points) && a[2] > 0;               // :363
      pass = pass && a[3] == a[4];                                    // one label (:369)
      if (pass) {
        vi[0] = pre_search[row * P + pl];                             // :373-375
        vi[1] = a[3];                                                 // :376-378
        score = pre_antipodal[row * P + pl];                          // :379-381
      }
      // :384: the frame is rejected when max(search) < valid_search_min or max(antipodal) < valid_antipodal_min; a NaN
      // score is not below anything, as torch.max keeps it
      keep_s = !((double)vi[0] < (double)p.valid_search_min);
      keep_a = !(score < p.valid_antipodal_min);
    }
    int* oi = ints + (row * P + pl) * 6;
#pragma unroll
    for (int c = 0; c < 6; ++c) oi[c] = vi[c];
    scores[row * P + pl] = score;
  }
  if (pl < L) slab_out[row * L + pl] = ok ? slab[row * L + pl] : 0;
  const int any_s = __syncthreads_or(keep_s);
  const int any_a = __syncthreads_or(keep_a);
  if (pl == 0) valid[row] = (any_s && any_a) ? 1 : 0;
}

// The baseline class's finish (torch_precomputed_baseline.py:275-348): one workgroup per frame, one thread per
// placement for the gates, every comparison as pv_finish_kernel makes it, without the label gate; then ONE thread folds
// the L * T looked-up scores in flattened order (depths outer, rolls inner) exactly as cr_best_kernel folds them, so the
// result does not depend on thread arrival.  The frame is valid when a placement was taken (:350): the mask bit already
// says score > antipodal_threshold, there is no 1e-4 line in this class.
__global__ __launch_bounds__(PV_MAX_P) void pvb_finish_kernel(
    const float* __restrict__ points, const float* __restrict__ frames, const float* __restrict__ tables,
    const float* __restrict__ hdr, const unsigned* __restrict__ words, const int* __restrict__ slab,
    const int* __restrict__ acc, const float* __restrict__ pre_antipodal, int F, PvParams p, int* __restrict__ ints,
    float* __restrict__ scores, int* __restrict__ slab_out, int* __restrict__ index, float* __restrict__ best_score,
    float* __restrict__ g2l) {
  __shared__ float sc[PV_MAX_P];
  const int b = blockIdx.y, f = blockIdx.x, pl = threadIdx.x;
  const int L = p.L, T = p.T, P = L * T;
  const size_t row = (size_t)b * F + f;
  const bool ok = ((const int*)(hdr + row * PV_HDR))[12] != 0;      // (0 for padding rows: pv_setup_kernel)
  if (pl < P) {
    int vi[4] = {0, 0, 0, 0};
    float score = 0.f;
    if (ok) {
      const int d = pl / T, r = pl % T;
      const int* a = acc + (row * P + pl) * PVB_ACC;
      const bool open = (words[(row * L + d) * 2] >> r) & 1u;         // mask bit set and table verdict clear (:275, :297)
      vi[0] = a[0]; vi[1] = a[1]; vi[2] = a[2];                      // (0 for a placement that was not graded)
      vi[3] = (words[(row * L + d) * 2 + 1] >> r) & 1u;
      bool pass = open && !((double)slab[row * L + d] < (double)p.slab_thr);          // :282
      pass = pass && !((double)a[0] > (double)p.back_thr);            // :312
      pass = pass && !((double)a[1] > (double)p.fing_thr);            // :323
      pass = pass && !((double)a[2] < (double)p.min_points);          // :333
      if (pass) score = pre_antipodal[row * P + pl];                  // :337-338
    }
    int* oi = ints + (row * P + pl) * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) oi[c] = vi[c];
    scores[row * P + pl] = score;
    sc[pl] = score;
  }
  if (pl < L) slab_out[row * L + pl] = ok ? slab[row * L + pl] : 0;
  __syncthreads();
  if (pl != 0) return;
  float best = 0.f;                                                   // the zeroed slot (:119)
  int bi = -1;
  for (int i = 0; i < P; ++i) {
    const float v = sc[i];
    if (v > best) { best = v; bi = i; }                               // :339; false for a NaN
  }
  index[row] = bi;
  best_score[row] = best;
  float* o = g2l + row * 16;
  if (bi < 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = 0.f;
    return;
  }
  best_placement_g2l(frames + row * 9, points[row * 3], points[row * 3 + 1], points[row * 3 + 2], tables, L, T, bi, o);
}

}  // namespace s4g

extern "C" int s4g_precomputed_select_f32(const int32_t* nearest_bn, const float* cloud_b3n,
                                          const float* scene_normals_b3m, const float* camera_b3,
                                          const float* scene_frames_bm33, const int32_t* search_bmp,
                                          const int32_t* inv_search_bmp, const float* antipodal_bmp,
                                          const float* inv_antipodal_bmp, int64_t B, int64_t N, int64_t M, int64_t L,
                                          int64_t T, double search_threshold, double antipodal_threshold,
                                          float sample_region, float* normals_b3n, int32_t* flipped_bn,
                                          float* frames_bn33, int32_t* pre_search_bnp, float* pre_antipodal_bnp,
                                          uint8_t* mask_bnp, int32_t* candidate_bn, int32_t* frame_index_bn,
                                          int64_t* frame_count_b, s4g_stream_t stream) {
  using namespace s4g;
  if (B < 0 || B > 65535 || N < 0 || N >= (1ll << 30) || M < 1 || M >= (1ll << 30)) return S4G_EINVAL;
  if (L <= 0 || T <= 0 || L > PV_MAX_L || T > PV_MAX_T) return S4G_EINVAL;
  if (B == 0) return S4G_OK;
  if (!frame_count_b || !scene_normals_b3m || !camera_b3 || !scene_frames_bm33 || !search_bmp || !inv_search_bmp ||
      !antipodal_bmp || !inv_antipodal_bmp)
    return S4G_EINVAL;
  if (N > 0 && (!nearest_bn || !cloud_b3n || !normals_b3n || !flipped_bn || !frames_bn33 || !pre_search_bnp ||
                !pre_antipodal_bnp || !mask_bnp || !candidate_bn || !frame_index_bn))
    return S4G_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (N > 0) {
    hipLaunchKernelGGL(pv_select_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)B), dim3(256), 0, st,
                       (const int*)nearest_bn, cloud_b3n, scene_normals_b3m, camera_b3, scene_frames_bm33,
                       (const int*)search_bmp, (const int*)inv_search_bmp, antipodal_bmp, inv_antipodal_bmp, (int)N,
                       (int)M, (int)(L * T), search_threshold, antipodal_threshold, sample_region, normals_b3n,
                       (int*)flipped_bn, frames_bn33, (int*)pre_search_bnp, pre_antipodal_bnp,
                       (unsigned char*)mask_bnp, (int*)candidate_bn);
    S4G_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(compact_valid_kernel<KeepNonZero>, dim3((unsigned)B), dim3(256), 0, st, (const int*)candidate_bn,
                     (int)N, (int*)frame_index_bn, frame_count_b);
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}

extern "C" size_t s4g_precomputed_search_workspace_bytes(int64_t B, int64_t M, int64_t F, int64_t L, int64_t T) {
  if (B <= 0 || M <= 0 || F <= 0 || L <= 0 || T <= 0 || L > s4g::PV_MAX_L || T > s4g::PV_MAX_T) return 0;
  return s4g::pv_layout((size_t)B, (size_t)F, (size_t)L, (size_t)T, s4g::PV_ACC).total;
}

extern "C" int s4g_precomputed_search_f32(const float* points_bf3, const float* frames_bf33, const uint8_t* mask_bfp,
                                          const int32_t* pre_search_bfp, const float* pre_antipodal_bfp,
                                          const float* xyz_b3m, const int32_t* labels_bm, int64_t B, int64_t M,
                                          int64_t F, int64_t L, int64_t T, const float* params13, int32_t no_label,
                                          const float* tables_3l2t, const int64_t* frame_count_b, int32_t* ints_bfp6,
                                          float* scores_bfp, int32_t* slab_bfl, int32_t* valid_bf,
                                          int32_t* valid_index_bf, int64_t* count_b, void* workspace,
                                          size_t workspace_bytes, s4g_stream_t stream) {
  using namespace s4g;
  if (B < 0 || M <= 0 || F < 0 || B > 65535 || F > 65535 || M >= (1ll << 30)) return S4G_EINVAL;
  if (L <= 0 || T <= 0 || L > PV_MAX_L || T > PV_MAX_T) return S4G_EINVAL;
  if (B * F * L * T > (1ll << 26)) return S4G_EINVAL;       // (the accumulators: 5 ints per placement, indexed in size_t)
  if (B == 0) return S4G_OK;
  if (!count_b) return S4G_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (F == 0) {
    hipError_t e = hipMemsetAsync(count_b, 0, (size_t)B * sizeof(int64_t), st);
    return e == hipSuccess ? S4G_OK : (int)e;
  }
  if (!points_bf3 || !frames_bf33 || !mask_bfp || !pre_search_bfp || !pre_antipodal_bfp || !xyz_b3m || !labels_bm ||
      !params13 || !tables_3l2t || !ints_bfp6 || !scores_bfp || !slab_bfl || !valid_bf || !valid_index_bf)
    return S4G_EINVAL;
  if (!workspace || workspace_bytes < s4g_precomputed_search_workspace_bytes(B, M, F, L, T)) return S4G_EWORKSPACE;
  PvParams p;
  p.fl = params13[0]; p.bl = params13[1]; p.hht = params13[2]; p.hbw = params13[3]; p.hbs = params13[4];
  p.margin = params13[5]; p.back_thr = params13[6]; p.fing_thr = params13[7]; p.min_points = params13[8];
  p.table_limit = params13[9]; p.slab_thr = params13[10]; p.valid_search_min = params13[11];
  p.valid_antipodal_min = params13[12];
  // the roll's cos / sin are fp32 values of deg / 57.29578: c^2 + s^2 is 1 within 1e-6, the slack is 1e-4
  p.r2lim = (p.hbw * p.hbw + p.hht * p.hht) * 1.0001f;
  p.L = (int)L; p.T = (int)T; p.no_label = no_label;
  const PvLayout lay = pv_layout((size_t)B, (size_t)F, (size_t)L, (size_t)T, PV_ACC);
  char* ws = (char*)workspace;
  float* hdr = (float*)(ws + lay.hdr);
  int* acc = (int*)(ws + lay.acc);
  int* slab = (int*)(ws + lay.slab);
  unsigned* words = (unsigned*)(ws + lay.words);
  const dim3 per_frame((unsigned)F, (unsigned)B);
  hipLaunchKernelGGL(pv_setup_kernel<PV_ACC>, per_frame, dim3(64), 0, st, points_bf3, frames_bf33,
                     (const unsigned char*)mask_bfp, tables_3l2t, (int)F, p, frame_count_b, hdr, acc, slab, words);
  S4G_LAUNCH_CHECK();
  const dim3 grid(PV_GX, (unsigned)sweep_chunks(M, PV_CHUNK_POINTS, PV_MIN_CHUNKS, PV_MAX_CHUNKS), (unsigned)B);
  hipLaunchKernelGGL(pv_scan_kernel, grid, dim3(256), 0, st, xyz_b3m, (const int*)labels_bm, (const float*)hdr,
                     (const unsigned*)words, tables_3l2t, (int)M, (int)F, p, slab, acc, frame_count_b);
  S4G_LAUNCH_CHECK();
  hipLaunchKernelGGL(pv_finish_kernel, per_frame, dim3(PV_MAX_P), 0, st, (const float*)hdr, (const unsigned*)words,
                     (const int*)slab, (const int*)acc, (const int*)pre_search_bfp, pre_antipodal_bfp, (int)F, p,
                     (int*)ints_bfp6, scores_bfp, (int*)slab_bfl, (int*)valid_bf);
  S4G_LAUNCH_CHECK();
  hipLaunchKernelGGL(compact_valid_kernel<KeepNonZero>, dim3((unsigned)B), dim3(256), 0, st, (const int*)valid_bf,
                     (int)F, (int*)valid_index_bf, count_b);
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}

extern "C" size_t s4g_precomputed_baseline_search_workspace_bytes(int64_t B, int64_t M, int64_t F, int64_t L,
                                                                  int64_t T) {
  if (B <= 0 || M <= 0 || F <= 0 || L <= 0 || T <= 0 || L > s4g::PV_MAX_L || T > s4g::PV_MAX_T) return 0;
  return s4g::pv_layout((size_t)B, (size_t)F, (size_t)L, (size_t)T, s4g::PVB_ACC).total;
}

extern "C" int s4g_precomputed_baseline_search_f32(const float* points_bf3, const float* frames_bf33,
                                                   const uint8_t* mask_bfp, const float* pre_antipodal_bfp,
                                                   const float* xyz_b3m, int64_t B, int64_t M, int64_t F, int64_t L,
                                                   int64_t T, const float* params11, const float* tables_3l2t,
                                                   const int64_t* frame_count_b, int32_t* ints_bfp4, float* scores_bfp,
                                                   int32_t* slab_bfl, int32_t* index_bf, float* score_bf,
                                                   float* g2l_bf44, int32_t* valid_index_bf, int64_t* count_b,
                                                   void* workspace, size_t workspace_bytes, s4g_stream_t stream) {
  using namespace s4g;
  if (B < 0 || M <= 0 || F < 0 || B > 65535 || F > 65535 || M >= (1ll << 30)) return S4G_EINVAL;
  if (L <= 0 || T <= 0 || L > PV_MAX_L || T > PV_MAX_T) return S4G_EINVAL;
  if (B * F * L * T > (1ll << 26)) return S4G_EINVAL;       // (the limits of s4g_precomputed_search_f32)
  if (B == 0) return S4G_OK;
  if (!count_b) return S4G_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (F == 0) {
    hipError_t e = hipMemsetAsync(count_b, 0, (size_t)B * sizeof(int64_t), st);
    return e == hipSuccess ? S4G_OK : (int)e;
  }
  if (!points_bf3 || !frames_bf33 || !mask_bfp || !pre_antipodal_bfp || !xyz_b3m || !params11 || !tables_3l2t ||
      !ints_bfp4 || !scores_bfp || !slab_bfl || !index_bf || !score_bf || !g2l_bf44 || !valid_index_bf)
    return S4G_EINVAL;
  if (!workspace || workspace_bytes < s4g_precomputed_baseline_search_workspace_bytes(B, M, F, L, T))
    return S4G_EWORKSPACE;
  PvParams p;
  p.fl = params11[0]; p.bl = params11[1]; p.hht = params11[2]; p.hbw = params11[3]; p.hbs = params11[4];
  p.margin = params11[5]; p.back_thr = params11[6]; p.fing_thr = params11[7]; p.min_points = params11[8];
  p.table_limit = params11[9]; p.slab_thr = params11[10];
  p.valid_search_min = p.valid_antipodal_min = 0.f;         // (not read: this class has no validity line)
  p.r2lim = (p.hbw * p.hbw + p.hht * p.hht) * 1.0001f;      // as s4g_precomputed_search_f32
  p.L = (int)L; p.T = (int)T; p.no_label = 0;
  const PvLayout lay = pv_layout((size_t)B, (size_t)F, (size_t)L, (size_t)T, PVB_ACC);
  char* ws = (char*)workspace;
  float* hdr = (float*)(ws + lay.hdr);
  int* acc = (int*)(ws + lay.acc);
  int* slab = (int*)(ws + lay.slab);
  unsigned* words = (unsigned*)(ws + lay.words);
  const dim3 per_frame((unsigned)F, (unsigned)B);
  hipLaunchKernelGGL(pv_setup_kernel<PVB_ACC>, per_frame, dim3(64), 0, st, points_bf3, frames_bf33,
                     (const unsigned char*)mask_bfp, tables_3l2t, (int)F, p, frame_count_b, hdr, acc, slab, words);
  S4G_LAUNCH_CHECK();
  const dim3 grid(PV_GX, (unsigned)sweep_chunks(M, PV_CHUNK_POINTS, PV_MIN_CHUNKS, PV_MAX_CHUNKS), (unsigned)B);
  hipLaunchKernelGGL(pvb_scan_kernel, grid, dim3(256), 0, st, xyz_b3m, (const float*)hdr, (const unsigned*)words,
                     tables_3l2t, (int)M, (int)F, p, slab, acc, frame_count_b);
  S4G_LAUNCH_CHECK();
  hipLaunchKernelGGL(pvb_finish_kernel, per_frame, dim3(PV_MAX_P), 0, st, points_bf3, frames_bf33, tables_3l2t,
                     (const float*)hdr, (const unsigned*)words, (const int*)slab, (const int*)acc, pre_antipodal_bfp,
                     (int)F, p, (int*)ints_bfp4, scores_bfp, (int*)slab_bfl, (int*)index_bf, score_bf, g2l_bf44);
  S4G_LAUNCH_CHECK();
  hipLaunchKernelGGL(compact_valid_kernel<KeepNonNegative>, dim3((unsigned)B), dim3(256), 0, st, (const int*)index_bf,
                     (int)F, (int*)valid_index_bf, count_b);
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}
