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
// Both scans are cloud sweeps: frame_sweep.h has the skeleton and the full-wave bound their ballots rely on, eval_sweep.h
// the bodies of the two scans, which s4g_eval_scene_grade_f32 (eval_data.hip) compiles too.
//
// The rejected alternative (compact the close region's (y, |n.y|) pairs into the workspace during the first scan and
// reduce those): profiles/r09_eval_frames.md.
#include "eval_sweep.h"

namespace s4g {

constexpr int EV_GX = 16;          // workgroups that share a scene's pose list (pose k belongs to workgroup k mod 16)
constexpr int EV_U = 4;            // points per lane held in registers while the workgroup's poses pass over them
constexpr int EV_SLOTS = 32;       // poses per pass (their matrices and accumulators live in LDS)
constexpr int EV_MIN_CHUNKS = 8;   // point ranges per scene: ceil(N / 8 192) within [8, 64]
constexpr int EV_MAX_CHUNKS = 64;
constexpr int EV_CHUNK_POINTS = 8192;

// the verdicts of :83-111 from a pose's accumulators; scored = the pose reaches _antipodal_score
__device__ __forceinline__ bool eval_gate(const int* __restrict__ a, const EvalParams& p, bool* collision, bool* multi) {
  *collision = ((double)a[0] > (double)p.back_threshold) || ((double)a[1] > (double)p.finger_threshold);   // :83,93
  *multi = a[2] > 0 && a[3] != a[4];                                                                      // :99-102
  return a[2] > 0 && !((double)a[2] < (double)p.min_points) && !*collision && !*multi;                    // :107-111
}

__global__ __launch_bounds__(256) void eval_scan_kernel(
    const float* __restrict__ xyz, const int* __restrict__ labels, const float* __restrict__ g2l, int N, int K,
    EvalParams p, int* __restrict__ acc, const int64_t* __restrict__ pose_count, int invert_se3) {
  eval_scan<false, EV_GX, EV_U, EV_SLOTS>(xyz, labels, g2l, N, K, p.box, acc, pose_count, nullptr, invert_se3);
}

// which poses reach _antipodal_score: the gate of this class
struct EvalFramesGate {
  EvalParams p;
  __device__ __forceinline__ bool operator()(size_t, const int* __restrict__ a) const {
    bool collision, multi;
    return eval_gate(a, p, &collision, &multi);
  }
};

__global__ __launch_bounds__(256) void eval_band_kernel(
    const float* __restrict__ xyz, const float* __restrict__ normals, const float* __restrict__ g2l, int N, int K,
    EvalParams p, const int* __restrict__ acc, float* __restrict__ part, const int64_t* __restrict__ pose_count,
    int invert_se3) {
  eval_band<EV_GX, EV_U, EV_SLOTS>(xyz, normals, g2l, N, K, p.box, p.neighbor_depth, EvalFramesGate{p}, acc, part,
                                   pose_count, invert_se3);
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
      const BandMeans m = eval_band_means(part + ((size_t)b * K + k) * nchunk * 4, N, nchunk);
      vi[4] = m.n_left; vi[5] = m.n_right;
      vf[2] = m.mean_left;                            // torch.mean (:61); an empty band gives NaN there and here
      vf[3] = m.mean_right;
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
