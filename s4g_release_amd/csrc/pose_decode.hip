// Pose decode on the device: the step right after the network in the
// reference's callers.
//
// Restates, per point / per selected grasp,
//   utils/file_logger_cls.py:34-47   softmax over score classes, frame_R as
//                                     row-major 3x3, softmax over the 4 t bins
//                                     times (0.08, 0.06, 0.04, 0.02),
//                                     t = -tau * R[:,0] + p
//   utils/file_logger_cls.py:66-68   expected score  sum_c value[c] * softmax[c]
//                                     (value = linspace(0,1,C+1)[:-1]; the
//                                     detector uses [1:], grasp_detector.py:146-148)
//   utils/file_logger_cls.py:203-218 Gram-Schmidt: x = R[:,0]/|.|,
//   grasp_detector.py:124-135        y = R[:,1] - (x.y) x, normalised, z = x cross y,
//                                     H = [x y z | t; 0 0 0 1]
// Two tiny HBM-bound kernels around a top-K selection, so only K poses per
// scene (K * 18 floats) instead of 21 channels x N points leave the GPU / go
// into the all-gather.
#include "frame_sweep.h"

namespace s4g {

// expected score per point; score logits are (B, C, N) channel-first, C <= 8
__global__ __launch_bounds__(256) void expected_score_kernel(
    const float* __restrict__ logits, int C, int N, const float* __restrict__ values,
    float* __restrict__ out) {
  const int b = blockIdx.y;
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const float* l = logits + (size_t)b * C * N + n;
  float mx = l[0];
  for (int c = 1; c < C; ++c) mx = fmaxf(mx, l[(size_t)c * N]);
  float den = 0.f, num = 0.f;
  for (int c = 0; c < C; ++c) {
    const float e = expf(l[(size_t)c * N] - mx);
    den += e;
    num += values[c] * e;
  }
  out[(size_t)b * N + n] = num / den;
}

// H = [x y z | t; 0 0 0 1] row-major from the row-major 3x3 r (R[i][j] = r[3i + j]): Gram-Schmidt on its first
// two columns
__device__ __forceinline__ void gram_schmidt_pose(const float* r, float tx, float ty, float tz, float* __restrict__ h) {
  float x0 = r[0], x1 = r[3], x2 = r[6];
  const float xn = sqrtf(x0 * x0 + x1 * x1 + x2 * x2);
  x0 /= xn; x1 /= xn; x2 /= xn;
  float y0 = r[1], y1 = r[4], y2 = r[7];
  const float d = x0 * y0 + x1 * y1 + x2 * y2;
  y0 -= d * x0; y1 -= d * x1; y2 -= d * x2;
  // second projection: for nearly parallel columns (angle a) the first leaves x.y ~ eps / sin(a) (3e-5 at a = 1e-2);
  // repeating it brings x.y back to rounding level
  const float d2 = x0 * y0 + x1 * y1 + x2 * y2;
  y0 -= d2 * x0; y1 -= d2 * x1; y2 -= d2 * x2;
  const float yn = sqrtf(y0 * y0 + y1 * y1 + y2 * y2);
  y0 /= yn; y1 /= yn; y2 /= yn;
  const float z0 = x1 * y2 - x2 * y1, z1 = x2 * y0 - x0 * y2, z2 = x0 * y1 - x1 * y0;
  h[0] = x0; h[1] = y0; h[2] = z0; h[3] = tx;
  h[4] = x1; h[5] = y1; h[6] = z1; h[7] = ty;
  h[8] = x2; h[9] = y2; h[10] = z2; h[11] = tz;
  h[12] = 0.f; h[13] = 0.f; h[14] = 0.f; h[15] = 1.f;
}

// one thread per selected grasp: 4x4 row-major pose
__global__ __launch_bounds__(64) void decode_pose_kernel(
    const float* __restrict__ xyz, const float* __restrict__ frame_R,
    const float* __restrict__ frame_t, const int64_t* __restrict__ sel, int N, int K,
    int TC, const float* __restrict__ t_bins, float* __restrict__ H) {
  const int b = blockIdx.y;
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= K) return;
  const int n = (int)sel[(size_t)b * K + k];
  const float* R = frame_R + (size_t)b * 9 * N + n;     // R[i][j] = channel 3i + j
  float r[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) r[c] = R[(size_t)c * N];
  const float* tl = frame_t + (size_t)b * TC * N + n;
  float mx = tl[0];
  for (int c = 1; c < TC; ++c) mx = fmaxf(mx, tl[(size_t)c * N]);
  float den = 0.f, num = 0.f;
  for (int c = 0; c < TC; ++c) {
    const float e = expf(tl[(size_t)c * N] - mx);
    den += e;
    num += t_bins[c] * e;
  }
  const float tau = num / den;
  const float* p = xyz + (size_t)b * 3 * N + n;
  const float tx = -tau * r[0] + p[0], ty = -tau * r[3] + p[N], tz = -tau * r[6] + p[2 * (size_t)N];
  gram_schmidt_pose(r, tx, ty, tz, H + ((size_t)b * K + k) * 16);
}


// the same for an ABSOLUTE translation (the contact network's frame_t = point + offset, (B, 3, N)): H = [Gram-Schmidt(R)
// | frame_t[:, sel]], no depth-bin softmax
__global__ __launch_bounds__(64) void decode_pose_abs_kernel(
    const float* __restrict__ frame_R, const float* __restrict__ frame_t, const int64_t* __restrict__ sel, int N, int K,
    float* __restrict__ H) {
  const int b = blockIdx.y;
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= K) return;
  const int n = (int)sel[(size_t)b * K + k];
  const float* R = frame_R + (size_t)b * 9 * N + n;     // R[i][j] = channel 3i + j
  float r[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) r[c] = R[(size_t)c * N];
  const float* t = frame_t + (size_t)b * 3 * N + n;
  gram_schmidt_pose(r, t[0], t[N], t[2 * (size_t)N], H + ((size_t)b * K + k) * 16);
}

}  // namespace s4g

extern "C" int s4g_expected_score_f32(const float* logits_bcn, int64_t B, int64_t C, int64_t N,
                                      const float* values_c, float* score_bn,
                                      s4g_stream_t stream) {
  if (B < 0 || C <= 0 || N < 0 || B > 65535 || N >= (1ll << 31)) return S4G_EINVAL;
  if (B == 0 || N == 0) return S4G_OK;
  if (!logits_bcn || !values_c || !score_bn) return S4G_EINVAL;
  hipLaunchKernelGGL(s4g::expected_score_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)B),
                     dim3(256), 0, (hipStream_t)stream, logits_bcn, (int)C, (int)N, values_c,
                     score_bn);
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}

extern "C" int s4g_decode_poses_f32(const float* xyz_b3n, const float* frame_R_b9n,
                                    const float* frame_t_btn, const int64_t* sel_bk, int64_t B,
                                    int64_t N, int64_t K, int64_t TC, const float* t_bins,
                                    float* H_bk44, s4g_stream_t stream) {
  if (B < 0 || N <= 0 || K < 0 || TC <= 0 || B > 65535 || N >= (1ll << 31)) return S4G_EINVAL;
  if (B == 0 || K == 0) return S4G_OK;
  if (!xyz_b3n || !frame_R_b9n || !frame_t_btn || !sel_bk || !t_bins || !H_bk44) return S4G_EINVAL;
  hipLaunchKernelGGL(s4g::decode_pose_kernel, dim3((unsigned)((K + 63) / 64), (unsigned)B), dim3(64),
                     0, (hipStream_t)stream, xyz_b3n, frame_R_b9n, frame_t_btn, sel_bk, (int)N,
                     (int)K, (int)TC, t_bins, H_bk44);
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}

extern "C" int s4g_decode_poses_abs_f32(const float* frame_R_b9n, const float* frame_t_b3n, const int64_t* sel_bk,
                                        int64_t B, int64_t N, int64_t K, float* H_bk44, s4g_stream_t stream) {
  if (B < 0 || N <= 0 || K < 0 || B > 65535 || N >= (1ll << 31)) return S4G_EINVAL;
  if (B == 0 || K == 0) return S4G_OK;
  if (!frame_R_b9n || !frame_t_b3n || !sel_bk || !H_bk44) return S4G_EINVAL;
  hipLaunchKernelGGL(s4g::decode_pose_abs_kernel, dim3((unsigned)((K + 63) / 64), (unsigned)B), dim3(64), 0,
                     (hipStream_t)stream, frame_R_b9n, frame_t_b3n, sel_bk, (int)N, (int)K, H_bk44);
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}

// ---------------------------------------------------------------------------
// Batched gripper-vs-cloud collision counts: restates
// CloudCollisionChecker.view_non_collision
// (cloud_processor/view_collision_checker.py:37-65), which the detector calls
// once per pose in a Python loop with a host sync each (grasp_detector.py:216-234).
// One workgroup per pose streams the cloud once (HBM/L2-bound, 12 B per point)
// and counts the points behind the palm and inside the two finger volumes.
// ---------------------------------------------------------------------------
namespace s4g {

constexpr int COLL_CHUNKS = 8;     // point ranges per scene (a workgroup scans one range)
constexpr int COLL_GX = 16;        // workgroups that share a scene's pose list (pose k belongs to workgroup k mod 16)
constexpr int COLL_U = 4;          // points per lane held in registers while the workgroup's poses pass over them
constexpr int COLL_SLOTS = 32;     // poses per pass (their matrices and counters live in LDS)

// The cloud sweep of frame_sweep.h, points outer, poses inner: a workgroup keeps 1 024 points in registers and runs ALL
// its poses over them before it loads the next 1 024 -- the cloud is read once per workgroup instead of once per pose.  (Round 6: with one workgroup
// per pose every candidate re-read the whole 48 902-point cloud from L2: ~500 candidates per scene x 16 scenes x 587 KB
// = 4.8 GB per call, 0.5 ms of a pipelined step.)
__global__ __launch_bounds__(256) void collision_counts_kernel(
    const float* __restrict__ xyz, const float* __restrict__ g2l, int N, int K, GripperBox g,
    int* __restrict__ counts, const int64_t* __restrict__ pose_count, int invert_se3) {
  __shared__ float gl[COLL_SLOTS][12];
  __shared__ int cnt[COLL_SLOTS][2];
  const int b = blockIdx.z, t = threadIdx.x, lane = t & 63;
  const float* px = xyz + (size_t)b * 3 * N;
  const ChunkRange rg = chunk_range(N);
  if (rg.empty()) return;                            // nothing to count: `counts` is pre-zeroed by the launcher
  const int kmax = frame_rows(pose_count, b, K);     // padding rows: never scanned (counts pre-zeroed)
  // this workgroup's poses: k = blockIdx.x + COLL_GX * j, j = 0, 1, ... ; COLL_SLOTS of them per pass
  for (int j0 = 0; blockIdx.x + COLL_GX * j0 < kmax; j0 += COLL_SLOTS) {
    __syncthreads();                                  // (the previous pass's tables have been read)
    if (t < COLL_SLOTS) {
      const int k = blockIdx.x + COLL_GX * (j0 + t);
      cnt[t][0] = cnt[t][1] = 0;
      if (k < kmax) load_g2l(g2l + ((size_t)b * K + k) * 16, invert_se3, gl[t]);   // row-major 4x4
    }
    __syncthreads();
    const int nslot = pass_slots(kmax, COLL_GX, j0, COLL_SLOTS);
    for (int i0 = rg.lo + t; i0 < sweep_end<COLL_U>(rg.hi); i0 += 256 * COLL_U) {
      PointBlock<COLL_U> pt;
      pt.load(px, N, i0, rg.hi);
      for (int sl = 0; sl < nslot; ++sl) {
        float gm[12];
#pragma unroll
        for (int c = 0; c < 12; ++c) gm[c] = gl[sl][c];
        int nback = 0, nfing = 0;
#pragma unroll
        for (int u = 0; u < COLL_U; ++u) {
          const GripperRegions r = gripper_regions(gm, pt.x[u], pt.y[u], pt.z[u], g);
          nback += __popcll(__ballot(pt.in[u] && r.back));      // wave-uniform
          nfing += __popcll(__ballot(pt.in[u] && r.fing));
        }
        if (lane == 0) {
          if (nback) atomicAdd(&cnt[sl][0], nback);
          if (nfing) atomicAdd(&cnt[sl][1], nfing);
        }
      }
    }
    __syncthreads();
    if (t < 2 * nslot) {
      const int sl = t >> 1, w = t & 1;
      const int k = blockIdx.x + COLL_GX * (j0 + sl);
      if (cnt[sl][w]) atomicAdd(counts + ((size_t)b * K + k) * 2 + w, cnt[sl][w]);
    }
  }
}

static int launch_collision(const float* xyz, const float* g2l, int64_t B, int64_t N, int64_t K, const float* gripper6,
                            const int64_t* pose_count, int invert_se3, int32_t* counts, hipStream_t st) {
  GripperBox g = {gripper6[0], gripper6[1], gripper6[2], gripper6[3], gripper6[4], gripper6[5]};
  hipError_t e = hipMemsetAsync(counts, 0, sizeof(int32_t) * 2 * (size_t)B * (size_t)K, st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(collision_counts_kernel, dim3(COLL_GX, COLL_CHUNKS, (unsigned)B), dim3(256), 0, st, xyz, g2l, (int)N, (int)K,
                     g, counts, pose_count, invert_se3);
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}

}  // namespace s4g

extern "C" int s4g_collision_counts_f32(const float* xyz_b3n, const float* g2l_bk44, int64_t B,
                                        int64_t N, int64_t K, const float* gripper6,
                                        int32_t* counts_bk2, s4g_stream_t stream) {
  if (B < 0 || N <= 0 || K < 0 || B > 65535 || N >= (1ll << 31)) return S4G_EINVAL;
  if (B == 0 || K == 0) return S4G_OK;
  if (!xyz_b3n || !g2l_bk44 || !gripper6 || !counts_bk2) return S4G_EINVAL;
  return s4g::launch_collision(xyz_b3n, g2l_bk44, B, N, K, gripper6, nullptr, 0, counts_bk2, (hipStream_t)stream);
}

// The same for best-first pose lists of which only the first pose_count_b[b] rows of scene b are poses (device counts:
// the caller never reads them on the host): the padding rows get zero counts and are never scanned.
// invert_se3 = 1: the matrices are the POSES (gripper -> global) and the kernel forms their analytic SE(3) inverse itself.
extern "C" int s4g_collision_counts_n_f32(const float* xyz_b3n, const float* g2l_bk44, int64_t B,
                                          int64_t N, int64_t K, const float* gripper6,
                                          const int64_t* pose_count_b, int invert_se3, int32_t* counts_bk2,
                                          s4g_stream_t stream) {
  if (B < 0 || N <= 0 || K < 0 || B > 65535 || N >= (1ll << 31) || (invert_se3 & ~1)) return S4G_EINVAL;
  if (B == 0 || K == 0) return S4G_OK;
  if (!xyz_b3n || !g2l_bk44 || !gripper6 || !counts_bk2) return S4G_EINVAL;   // (pose_count_b may be NULL: every row is a pose)
  return s4g::launch_collision(xyz_b3n, g2l_bk44, B, N, K, gripper6, pose_count_b, invert_se3, counts_bk2,
                               (hipStream_t)stream);
}
