// Batched grading of grasp frames against a dense, labelled scene cloud with normals: restates
// EvalExpCloud.eval_frame (eval_experiment/eval_point_cloud.py:39-113), which the reference calls once per pose -- a
// dozen boolean-mask compactions, a torch.unique and a .cpu() each -- as four launches over all poses of all scenes,
// with no host synchronisation.
//
//   eval_init_kernel     the per-pose accumulators (workspace) to their neutral values
//   eval_scan_kernel     first scan of the cloud: the counts behind the palm / in the fingers (frame_sweep.h `gripper_regions`,
//                        which collision_counts_kernel calls too: the two integers are equal bit for bit), the
//                        close-region count, its label minimum / maximum (more than one distinct label <=> min != max:
//                        no `unique`) and its y extrema (ordered-integer atomics: order independent)
//   eval_band_kernel     second scan, ONLY for poses that reached the score (enough close-region points, no collision,
//                        one label): the sums of |n_local.y| over the two bands under the finger pads, whose bounds
//                        depend on the extrema of the whole cloud.  No floating-point atomics: a wave tree-sums the
//                        1 024 points of a sweep, adds that to its own accumulator (at most 8 sweeps per chunk up to
//                        N = 524 288), the four waves of a workgroup are summed in a fixed order into one partial per
//                        (pose, chunk) in the workspace
//   eval_finish_kernel   flags, pairwise sum of the chunk partials in chunk order, means and score; padding rows read 0
//
// Both scans are cloud sweeps: frame_sweep.h has the skeleton and the full-wave bound their ballots rely on.
//
// The rejected alternative (compact the close region's (y, |n.y|) pairs into the workspace during the first scan and
// reduce those): profiles/r09_eval_frames.md.
#include "frame_sweep.h"

namespace s4g {

struct EvalParams {
  GripperBox box;                  // the collision counter's six values
  float back_threshold, finger_threshold, min_points, neighbor_depth;
};

constexpr int EV_GX = 16;          // workgroups that share a scene's pose list (pose k belongs to workgroup k mod 16)
constexpr int EV_U = 4;            // points per lane held in registers while the workgroup's poses pass over them
constexpr int EV_SLOTS = 32;       // poses per pass (their matrices and accumulators live in LDS)
constexpr int EV_MIN_CHUNKS = 8;   // point ranges per scene: ceil(N / 8 192) within [8, 64]
constexpr int EV_MAX_CHUNKS = 64;
constexpr int EV_CHUNK_POINTS = 8192;
constexpr int EV_ACC = 8;          // per-pose accumulator ints: back, finger, close, label min, label max, y max, y min, -

// the verdicts of :83-111 from a pose's accumulators; scored = the pose reaches _antipodal_score
__device__ __forceinline__ bool eval_gate(const int* __restrict__ a, const EvalParams& p, bool* collision, bool* multi) {
  *collision = ((double)a[0] > (double)p.back_threshold) || ((double)a[1] > (double)p.finger_threshold);   // :83,93
  *multi = a[2] > 0 && a[3] != a[4];                                                                      // :99-102
  return a[2] > 0 && !((double)a[2] < (double)p.min_points) && !*collision && !*multi;                    // :107-111
}

__global__ __launch_bounds__(256) void eval_init_kernel(int* __restrict__ acc, int64_t n_pose) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pose * EV_ACC) return;
  acc[i] = acc_neutral((int)(i % EV_ACC));
}

// The cloud sweep of frame_sweep.h, points outer, poses inner: a workgroup keeps 1 024 points in registers and runs all
// its poses over them.  Labels are read only where a wave has a close-region point (rare: the region is a few cm wide).
__global__ __launch_bounds__(256) void eval_scan_kernel(
    const float* __restrict__ xyz, const int* __restrict__ labels, const float* __restrict__ g2l, int N, int K,
    EvalParams p, int* __restrict__ acc, const int64_t* __restrict__ pose_count, int invert_se3) {
  __shared__ float gl[EV_SLOTS][12];
  __shared__ int cnt[EV_SLOTS][EV_ACC];
  const int b = blockIdx.z, t = threadIdx.x, lane = t & 63;
  const float* px = xyz + (size_t)b * 3 * N;
  const int* lab = labels + (size_t)b * N;
  const ChunkRange rg = chunk_range(N);
  if (rg.empty()) return;
  const int kmax = frame_rows(pose_count, b, K);
  for (int j0 = 0; blockIdx.x + EV_GX * j0 < kmax; j0 += EV_SLOTS) {
    __syncthreads();                                  // (the previous pass's tables have been read)
    if (t < EV_SLOTS) {
      const int k = blockIdx.x + EV_GX * (j0 + t);
#pragma unroll
      for (int w = 0; w < ACC_WORDS; ++w) cnt[t][w] = acc_neutral(w);
      if (k < kmax) load_g2l(g2l + ((size_t)b * K + k) * 16, invert_se3, gl[t]);
    }
    __syncthreads();
    const int nslot = pass_slots(kmax, EV_GX, j0, EV_SLOTS);
    for (int i0 = rg.lo + t; i0 < sweep_end<EV_U>(rg.hi); i0 += 256 * EV_U) {
      PointBlock<EV_U> pt;
      pt.load(px, N, i0, rg.hi);
      for (int sl = 0; sl < nslot; ++sl) {
        float g[12];
#pragma unroll
        for (int c = 0; c < 12; ++c) g[c] = gl[sl][c];
        int nback = 0, nfing = 0, nclose = 0;
        int lmin = INT_MAX, lmax = INT_MIN, ymx = INT_MIN, ymn = INT_MAX;
        bool hit = false;
#pragma unroll
        for (int u = 0; u < EV_U; ++u) {
          const GripperRegions r = gripper_regions(g, pt.x[u], pt.y[u], pt.z[u], p.box);
          const bool cr = pt.in[u] && r.closer;
          nback += __popcll(__ballot(pt.in[u] && r.back));      // wave-uniform
          nfing += __popcll(__ballot(pt.in[u] && r.fing));
          nclose += __popcll(__ballot(cr));
          if (cr) {
            const int l = lab[pt.idx[u]], o = f2ord(r.ly);
            lmin = min(lmin, l); lmax = max(lmax, l);
            ymx = max(ymx, o); ymn = min(ymn, o);
            hit = true;
          }
        }
        if (lane == 0) {
          if (nback) atomicAdd(&cnt[sl][0], nback);
          if (nfing) atomicAdd(&cnt[sl][1], nfing);
          if (nclose) atomicAdd(&cnt[sl][2], nclose);
        }
        if (hit) {
          atomicMin(&cnt[sl][3], lmin); atomicMax(&cnt[sl][4], lmax);
          atomicMax(&cnt[sl][5], ymx); atomicMin(&cnt[sl][6], ymn);
        }
      }
    }
    __syncthreads();
    if (t < nslot) {
      const int k = blockIdx.x + EV_GX * (j0 + t);
      int* a = acc + ((size_t)b * K + k) * EV_ACC;
      if (cnt[t][0]) atomicAdd(a + 0, cnt[t][0]);
      if (cnt[t][1]) atomicAdd(a + 1, cnt[t][1]);
      if (cnt[t][2]) {
        atomicAdd(a + 2, cnt[t][2]);
        atomicMin(a + 3, cnt[t][3]); atomicMax(a + 4, cnt[t][4]);
        atomicMax(a + 5, cnt[t][5]); atomicMin(a + 6, cnt[t][6]);
      }
    }
  }
}

// The second scan.  A workgroup keeps, per pass, only those of its 32 poses that reached the score (compacted in pose
// order), so a pass without one costs a table load and no cloud read.  part (B, K, chunks, 4) = {sum left, sum right,
// n left, n right (int bits)} is written for every (scored pose, non-empty chunk) and read for nothing else.
__global__ __launch_bounds__(256) void eval_band_kernel(
    const float* __restrict__ xyz, const float* __restrict__ normals, const float* __restrict__ g2l, int N, int K,
    EvalParams p, const int* __restrict__ acc, float* __restrict__ part, const int64_t* __restrict__ pose_count,
    int invert_se3) {
  __shared__ float gl[EV_SLOTS][12];
  __shared__ float thr[EV_SLOTS][2];
  __shared__ int kof[EV_SLOTS];
  __shared__ int nlive;
  __shared__ float wsum[EV_SLOTS][4][2];
  __shared__ int wcnt[EV_SLOTS][4][2];
  const int b = blockIdx.z, chunk = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const float* px = xyz + (size_t)b * 3 * N;
  const float* pn = normals + (size_t)b * 3 * N;
  const int nchunk = (int)gridDim.y;
  const ChunkRange rg = chunk_range(N);
  if (rg.empty()) return;                            // eval_finish_kernel does not read an empty chunk's partials
  const int kmax = frame_rows(pose_count, b, K);
  for (int j0 = 0; blockIdx.x + EV_GX * j0 < kmax; j0 += EV_SLOTS) {
    __syncthreads();
    if (t < EV_SLOTS) {                               // (the first 32 lanes of wave 0)
      const int k = blockIdx.x + EV_GX * (j0 + t);
      bool live = false;
      float lthr = 0.f, rthr = 0.f;
      if (k < kmax) {
        const int* a = acc + ((size_t)b * K + k) * EV_ACC;
        bool collision, multi;
        live = eval_gate(a, p, &collision, &multi);
        const float left_y = ord2f(a[5]), right_y = ord2f(a[6]);                             // :52-53
        const float depth = fminf(__fdiv_rn(__fsub_rn(left_y, right_y), 3.0f), p.neighbor_depth);   // :54
        lthr = __fsub_rn(left_y, depth);                                                     // :56
        rthr = __fadd_rn(right_y, depth);                                                    // :57
      }
      const uint64_t m = __ballot(live);
      if (live) {
        const int pos = mask_rank(m);
        load_g2l(g2l + ((size_t)b * K + k) * 16, invert_se3, gl[pos]);
        thr[pos][0] = lthr; thr[pos][1] = rthr;
        kof[pos] = k;
      }
      if (t == 0) nlive = __popcll(m);
    }
    ((float*)wsum)[t] = 0.f;                          // 32 x 4 x 2 = 256 entries each
    ((int*)wcnt)[t] = 0;
    __syncthreads();
    const int nslot = nlive;
    if (nslot == 0) continue;                         // workgroup-uniform
    for (int i0 = rg.lo + t; i0 < sweep_end<EV_U>(rg.hi); i0 += 256 * EV_U) {
      PointBlock<EV_U> pt;
      pt.load(px, N, i0, rg.hi);
      for (int sl = 0; sl < nslot; ++sl) {
        float g[12];
#pragma unroll
        for (int c = 0; c < 12; ++c) g[c] = gl[sl][c];
        const float lthr = thr[sl][0], rthr = thr[sl][1];
        int nl = 0, nr = 0;
        float sl_ = 0.f, sr_ = 0.f;                   // this lane's (at most 4, nearly always at most 1) band terms
#pragma unroll
        for (int u = 0; u < EV_U; ++u) {
          const GripperRegions r = gripper_regions(g, pt.x[u], pt.y[u], pt.z[u], p.box);
          const bool cr = pt.in[u] && r.closer;
          const bool il = cr && (r.ly > lthr), ir = cr && (r.ly < rthr);                     // :56-57
          nl += __popcll(__ballot(il));
          nr += __popcll(__ballot(ir));
          if (il || ir) {
            // n_local.y = row 1 of the rotation times the normal (:69), not re-normalised; |.| (:58-59)
            const float a = fabsf(g[4] * pn[pt.idx[u]] + g[5] * pn[(size_t)N + pt.idx[u]] + g[6] * pn[2 * (size_t)N + pt.idx[u]]);
            if (il) sl_ += a;
            if (ir) sr_ += a;
          }
        }
        if (nl + nr) {                                // wave-uniform, rare: a butterfly sum over the 64 lanes
#pragma unroll
          for (int off = 32; off; off >>= 1) {
            sl_ += __shfl_xor(sl_, off);
            sr_ += __shfl_xor(sr_, off);
          }
          if (lane == 0) {                            // this wave's own cells: sweeps add in sweep order
            wsum[sl][wave][0] += sl_; wsum[sl][wave][1] += sr_;
            wcnt[sl][wave][0] += nl; wcnt[sl][wave][1] += nr;
          }
        }
      }
    }
    __syncthreads();
    if (t < nslot) {
      float* o = part + (((size_t)b * K + kof[t]) * nchunk + chunk) * 4;
      o[0] = (wsum[t][0][0] + wsum[t][1][0]) + (wsum[t][2][0] + wsum[t][3][0]);
      o[1] = (wsum[t][0][1] + wsum[t][1][1]) + (wsum[t][2][1] + wsum[t][3][1]);
      o[2] = __int_as_float(wcnt[t][0][0] + wcnt[t][1][0] + wcnt[t][2][0] + wcnt[t][3][0]);
      o[3] = __int_as_float(wcnt[t][0][1] + wcnt[t][1][1] + wcnt[t][2][1] + wcnt[t][3][1]);
    }
  }
}

// one thread per pose row
__global__ __launch_bounds__(64) void eval_finish_kernel(
    const int* __restrict__ acc, const float* __restrict__ part, int N, int K, int nchunk, EvalParams p,
    const int64_t* __restrict__ pose_count, int* __restrict__ ints, float* __restrict__ floats) {
  const int b = blockIdx.y;
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= K) return;
  int* oi = ints + ((size_t)b * K + k) * 8;
  float* of = floats + ((size_t)b * K + k) * 5;
  int vi[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float vf[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (k < frame_rows(pose_count, b, K)) {
    const int* a = acc + ((size_t)b * K + k) * EV_ACC;
    bool collision, multi;
    const bool scored = eval_gate(a, p, &collision, &multi);
    vi[0] = a[0]; vi[1] = a[1]; vi[2] = a[2]; vi[3] = multi; vi[6] = collision;
    if (a[2] > 0) { vf[0] = ord2f(a[5]); vf[1] = ord2f(a[6]); }
    if (scored) {
      // pairwise sum of the chunk partials in chunk order (a binary counter of pending subtree sums)
      float stl[8], str[8];
      int nl = 0, nr = 0, j = 0;
      const int nc = (N + nchunk - 1) / nchunk;
      const float* q = part + ((size_t)b * K + k) * nchunk * 4;
      for (int c = 0; c < nchunk && c * (int64_t)nc < N; ++c, ++j) {
        float l = q[4 * c], r = q[4 * c + 1];
        nl += __float_as_int(q[4 * c + 2]);
        nr += __float_as_int(q[4 * c + 3]);
        int lvl = 0;
        for (int jj = j; jj & 1; jj >>= 1, ++lvl) { l = stl[lvl] + l; r = str[lvl] + r; }
        stl[lvl] = l; str[lvl] = r;
      }
      float sl_ = 0.f, sr_ = 0.f;
      bool have = false;
      for (int lvl = 0; lvl < 8; ++lvl)
        if ((j >> lvl) & 1) {
          sl_ = have ? stl[lvl] + sl_ : stl[lvl];
          sr_ = have ? str[lvl] + sr_ : str[lvl];
          have = true;
        }
      vi[4] = nl; vi[5] = nr;
      vf[2] = __fdiv_rn(sl_, (float)nl);              // torch.mean (:61); an empty band gives NaN there and here
      vf[3] = __fdiv_rn(sr_, (float)nr);
      vf[4] = __fmul_rn(vf[2], vf[3]);
    }
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) oi[c] = vi[c];
#pragma unroll
  for (int c = 0; c < 5; ++c) of[c] = vf[c];
}

}  // namespace s4g

extern "C" size_t s4g_eval_frames_workspace_bytes(int64_t B, int64_t N, int64_t K) {
  if (B <= 0 || N <= 0 || K <= 0) return 0;
  using namespace s4g;
  const size_t poses = (size_t)B * (size_t)K;
  const size_t nchunk = (size_t)sweep_chunks(N, EV_CHUNK_POINTS, EV_MIN_CHUNKS, EV_MAX_CHUNKS);
  return align256(poses * EV_ACC * sizeof(int)) + poses * nchunk * 4 * sizeof(float);
}

extern "C" int s4g_eval_frames_f32(const float* xyz_b3n, const float* normals_b3n, const int32_t* labels_bn,
                                   const float* g2l_bk44, int64_t B, int64_t N, int64_t K, const float* params10,
                                   const int64_t* pose_count_b, int invert_se3, int32_t* ints_bk8, float* floats_bk5,
                                   void* workspace, size_t workspace_bytes, s4g_stream_t stream) {
  using namespace s4g;
  if (B < 0 || N <= 0 || K < 0 || B > 65535 || N >= (1ll << 30) || K >= (1ll << 31) || (invert_se3 & ~1)) return S4G_EINVAL;
  if (B * K > (1ll << 27)) return S4G_EINVAL;       // (the accumulator grid: 8 ints per pose row, 256 per workgroup)
  if (B == 0 || K == 0) return S4G_OK;
  if (!xyz_b3n || !normals_b3n || !labels_bn || !g2l_bk44 || !params10 || !ints_bk8 || !floats_bk5) return S4G_EINVAL;
  if (!workspace || workspace_bytes < s4g_eval_frames_workspace_bytes(B, N, K)) return S4G_EWORKSPACE;
  EvalParams p = {{params10[0], params10[1], params10[2], params10[3], params10[4], params10[5]},
                  params10[6], params10[7], params10[8], params10[9]};
  hipStream_t st = (hipStream_t)stream;
  const int nchunk = sweep_chunks(N, EV_CHUNK_POINTS, EV_MIN_CHUNKS, EV_MAX_CHUNKS);
  const int64_t poses = B * K;
  int* acc = (int*)workspace;
  float* part = (float*)((char*)workspace + align256((size_t)poses * EV_ACC * sizeof(int)));
  hipLaunchKernelGGL(eval_init_kernel, dim3((unsigned)((poses * EV_ACC + 255) / 256)), dim3(256), 0, st, acc, poses);
  S4G_LAUNCH_CHECK();
  const dim3 grid(EV_GX, (unsigned)nchunk, (unsigned)B);
  hipLaunchKernelGGL(eval_scan_kernel, grid, dim3(256), 0, st, xyz_b3n, (const int*)labels_bn, g2l_bk44, (int)N, (int)K,
                     p, acc, pose_count_b, invert_se3);
  S4G_LAUNCH_CHECK();
  hipLaunchKernelGGL(eval_band_kernel, grid, dim3(256), 0, st, xyz_b3n, normals_b3n, g2l_bk44, (int)N, (int)K, p,
                     (const int*)acc, part, pose_count_b, invert_se3);
  S4G_LAUNCH_CHECK();
  hipLaunchKernelGGL(eval_finish_kernel, dim3((unsigned)((K + 63) / 64), (unsigned)B), dim3(64), 0, st,
                     (const int*)acc, (const float*)part, (int)N, (int)K, nchunk, p, pose_count_b, (int*)ints_bk8,
                     floats_bk5);
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}
