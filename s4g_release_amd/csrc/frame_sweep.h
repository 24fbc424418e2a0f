// The cloud sweep: what the frame-grading kernels share.  collision_counts_kernel (pose_decode.hip), eval_scan_kernel /
// eval_band_kernel (eval_frames.hip), ls_scan_kernel / ls_band_kernel (local_search.hip) and cs_scan_kernel
// (contact_search.hip) all run many rigid frames of a scene over that scene's dense cloud:
//
//   grid (GX, chunks, B), 256 threads.  blockIdx.y owns the point range `chunk_range`; blockIdx.x owns the frames
//   k = blockIdx.x + GX * j of its scene, SLOTS of them per pass (`pass_slots`), their 3 x 4 matrices and counters in LDS.
//
//     for j0 (passes of SLOTS frames)          tables and counters of the pass to LDS, counters to `acc_neutral`
//       for i0 (sweeps of 256 * U points)      `PointBlock<U>::load`: U points per lane, in registers
//         for sl (the frames of the pass)      `local_point`, the kernel's own regions, LDS atomics / ballots
//       flush the counters to the workspace with integer atomics (order independent: results are bit-identical
//       from run to run)
//
// The loop nest stays written out in every kernel: they differ in what a point contributes.  Only what is identical is
// here, each piece once.  The tuning constants (EV_*, LS_*, CS_*, COLL_*) stay with their kernels.
//
// THE FULL-WAVE BOUND.  A sweep loop runs `for (i0 = range.lo + t; i0 < sweep_end<U>(range.hi); i0 += 256 * U)`, not
// `i0 < range.hi`: the lanes of one wave differ by less than 64 in i0, so with the wider bound a wave that still holds
// an in-range point is fully active.  The ballots and the 64-lane butterfly of the kernels rely on that; lanes past the
// range are masked by `in[u]` and hold the chunk's last point.  cs_scan_kernel has neither a ballot nor a shuffle --
// every contribution is a per-lane LDS atomic, so a partly active wave counts the same -- and keeps the narrow bound
// `i0 < range.hi`, its masked lanes holding the sweep's first point i0: it sits at 100 scalar registers, the most that
// 8 waves per SIMD allow, and the wide bound (104) or the chunk's last point (101) takes it to 7
// (profiles/r14_frame_sweep.md).
#pragma once
#include <limits.h>

#include "s4g_common.h"

namespace s4g {

// point ranges per scene: ceil(N / chunk_points) within [min_chunks, max_chunks] (grid.y of a sweep launch)
static inline int sweep_chunks(int64_t N, int chunk_points, int min_chunks, int max_chunks) {
  int64_t c = (N + chunk_points - 1) / chunk_points;
  if (c < min_chunks) c = min_chunks;
  if (c > max_chunks) c = max_chunks;
  return (int)c;
}

static inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// the rows of scene b that are frames: all K, or the first count[b] of a padded list (the others are never scanned)
__device__ __forceinline__ int frame_rows(const int64_t* __restrict__ count, int b, int K) {
  if (!count) return K;
  return (int)min((int64_t)K, max((int64_t)0, count[b]));
}

// the points [lo, hi) of chunk blockIdx.y of gridDim.y.  It is empty whenever (gridDim.y - 1) * ceil(N / gridDim.y) >= N
// (8 chunks: N = 1..7, 9..14, ..., 49): return then, before any barrier -- the test is workgroup-uniform.
struct ChunkRange {
  int lo, hi;
  __device__ __forceinline__ bool empty() const { return lo >= hi; }
};
__device__ __forceinline__ ChunkRange chunk_range(int N) {
  const int nc = (N + (int)gridDim.y - 1) / (int)gridDim.y;
  ChunkRange r;
  r.lo = (int)blockIdx.y * nc;
  r.hi = min(N, r.lo + nc);
  return r;
}

// the frames of this workgroup in the pass that starts at j0: k = blockIdx.x + GX * (j0 + slot) < kmax, at most SLOTS
__device__ __forceinline__ int pass_slots(int kmax, int GX, int j0, int SLOTS) {
  const int left = (kmax - 1 - (int)blockIdx.x) / GX + 1 - j0;        // frames of this workgroup from j0 on
  return left < SLOTS ? left : SLOTS;
}

// the end of a sweep loop: THE FULL-WAVE BOUND above
template <int U>
__device__ __forceinline__ int sweep_end(int i_hi) { return i_hi + 256 * (U - 1); }

// the points of a sweep: i0 + 256 * u, u < U, of the channel-first cloud px (3, N); a lane past i_hi is masked
// (`in[u]` false) and holds point `masked`: the chunk's last point (i_hi - 1, always a point of the cloud) unless the
// caller names another
template <int U>
struct PointBlock {
  float x[U], y[U], z[U];
  bool in[U];
  int idx[U];
  __device__ __forceinline__ void load(const float* __restrict__ px, int N, int i0, int i_hi, int masked) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + 256 * u;
      in[u] = i < i_hi;
      idx[u] = in[u] ? i : masked;
      x[u] = px[(size_t)idx[u]];
      y[u] = px[(size_t)N + idx[u]];
      z[u] = px[2 * (size_t)N + idx[u]];
    }
  }
  __device__ __forceinline__ void load(const float* __restrict__ px, int N, int i0, int i_hi) {
    load(px, N, i0, i_hi, i_hi - 1);
  }
};

// a point in a frame: g = rows 0..2 of global -> local, row-major 3 x 4.  fp32, each op rounded on its own in this
// order (these translation units are compiled with -ffp-contract=off): every kernel sees the same bits
struct LocalPoint {
  float x, y, z;
};
__device__ __forceinline__ LocalPoint local_point(const float* __restrict__ g, float x, float y, float z) {
  LocalPoint l;
  l.x = g[0] * x + g[1] * y + g[2] * z + g[3];
  l.y = g[4] * x + g[5] * y + g[6] * z + g[7];
  l.z = g[8] * x + g[9] * y + g[10] * z + g[11];
  return l;
}

// the roll of LOCAL_TO_LOCAL_SEARCH (configs/config.py:79-82): every scan of local_search.hip and of
// precomputed_view.hip calls this, so they see the same y bit for bit
__device__ __forceinline__ void ls_roll(float c, float s, float y, float z, float* yy, float* zz) {
  *yy = c * y + s * z;
  *zz = (-s) * y + c * z;
}

// LOCAL_TO_LOCAL_SEARCH[bi] @ [R^T | -R^T p] as 16 floats, row-major 4 x 4: the reference's `baseline_frame`
// (torch_baseline_single_view_point_cloud.py:320-322, torch_precomputed_baseline.py:381-382), formed directly in fp32.
// r = the frame (axes as columns, row-major 3 x 3), tables = dl[L], lo[L], hi[L], cos[T], sin[T].  cr_best_kernel
// (close_region.hip) and pvb_finish_kernel (precomputed_view.hip) both call this: the same bits
__device__ __forceinline__ void best_placement_g2l(const float* __restrict__ r, float px, float py, float pz,
                                                   const float* __restrict__ tables, int L, int T, int bi,
                                                   float* __restrict__ o) {
  float g[3][4];
#pragma unroll
  for (int i = 0; i < 3; ++i) {                                                      // [R^T | -R^T p] as ls_setup_kernel forms it
    const float a = r[i], bb = r[3 + i], c = r[6 + i];
    g[i][0] = a; g[i][1] = bb; g[i][2] = c;
    g[i][3] = -__fadd_rn(__fadd_rn(__fmul_rn(a, px), __fmul_rn(bb, py)), __fmul_rn(c, pz));
  }
  const int d = bi / T, t = bi % T;
  const float dl = tables[d], cs = tables[3 * L + t], sn = tables[3 * L + T + t];
  // LOCAL_TO_LOCAL_SEARCH[i] (config.py:79-89): x - dl, then the roll (y, z) -> (c y + s z, -s y + c z)
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    o[c] = c == 3 ? g[0][3] - dl : g[0][c];
    o[4 + c] = cs * g[1][c] + sn * g[2][c];
    o[8 + c] = (-sn) * g[1][c] + cs * g[2][c];
    o[12 + c] = c == 3 ? 1.f : 0.f;
  }
}

// a monotone map float -> int (and back: it is an involution) for every non-NaN value: atomicMax / atomicMin on it give
// the float maximum / minimum whatever the order of arrival
__device__ __forceinline__ int f2ord(float f) {
  const int i = __float_as_int(f);
  return i ^ ((i >> 31) & 0x7fffffff);
}
__device__ __forceinline__ float ord2f(int o) { return __int_as_float(o ^ ((o >> 31) & 0x7fffffff)); }

// the accumulator words of a frame or placement, in the workspace and in LDS: counts (words 0..2), label minimum (3),
// label maximum (4), ordered-integer y maximum (5), y minimum (6); a kernel that keeps fewer uses a prefix.  The value
// a word starts from:
constexpr int ACC_WORDS = 7;
__device__ __forceinline__ int acc_neutral(int w) {
  return (w == 3 || w == 6) ? INT_MAX : (w == 4 || w == 5) ? INT_MIN : 0;
}

// one workgroup per scene: the rows b * n + i whose flag satisfies `keep`, in ascending order, -1 padded, and their count
struct KeepNonZero {
  __device__ __forceinline__ bool operator()(int v) const { return v != 0; }
};
struct KeepNonNegative {
  __device__ __forceinline__ bool operator()(int v) const { return v >= 0; }
};
template <class Keep>
__global__ __launch_bounds__(256) void compact_valid_kernel(const int* __restrict__ flag, int n,
                                                            int* __restrict__ valid_index, int64_t* __restrict__ count) {
  __shared__ int wtot[4];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int base = 0;
  for (int f0 = 0; f0 < n; f0 += 256) {
    const int f = f0 + t;
    const bool v = f < n && Keep()(flag[(size_t)b * n + f]);
    const uint64_t m = __ballot(v);
    if (lane == 0) wtot[wave] = __popcll(m);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wave; ++w) off += wtot[w];
    if (v) valid_index[(size_t)b * n + off + mask_rank(m)] = f;
    base += wtot[0] + wtot[1] + wtot[2] + wtot[3];
    __syncthreads();
  }
  for (int f = base + t; f < n; f += 256) valid_index[(size_t)b * n + f] = -1;
  if (t == 0) count[b] = base;
}

// ---- the normal a view point takes over from its nearest scene point: the rule s4g_contact_select_f32 documents
// (include/s4g_ops.h), as a function.  scene_normals (3, M) and cloud (3, N) of one scene, i the scene point or < 0,
// q the view point, cam the camera location.  n = the scene normal of i, or (0, 0, 1) without one; n / |n| in double (a
// zero normal gives NaN, as numpy does); turned towards the camera as seen from cloud point q; NOT rounded: the caller
// rounds to fp32 once.  cs_select_kernel (contact_search.hip) holds the same statements inline --------------------------
struct Normal64 {
  double x, y, z;
};
__device__ __forceinline__ Normal64 scene_normal_towards_camera(const float* __restrict__ scene_normals, int M, int i,
                                                                const float* __restrict__ cloud, int N, size_t q,
                                                                const float* __restrict__ cam) {
  double nx = 0.0, ny = 0.0, nz = 1.0;                 // no neighbour: it must be table
  if (i >= 0) {
    const double ax = (double)scene_normals[i], ay = (double)scene_normals[(size_t)M + i],
                 az = (double)scene_normals[2 * (size_t)M + i];
    const double len = sqrt(ax * ax + ay * ay + az * az);
    nx = ax / len; ny = ay / len; nz = az / len;
  }
  const double rx = (double)cam[0] - (double)cloud[q], ry = (double)cam[1] - (double)cloud[(size_t)N + q],
               rz = (double)cam[2] - (double)cloud[2 * (size_t)N + q];
  if (finite(rx) && finite(ry) && finite(rz)) {       // no reference direction otherwise: n stays
    if (nx == 0.0 && ny == 0.0 && nz == 0.0) {
      const double rl = sqrt(rx * rx + ry * ry + rz * rz);
      if (rl > 0.0) {
        nx = rx / rl; ny = ry / rl; nz = rz / rl;
      } else {
        nz = 1.0;
      }
    } else if (nx * rx + ny * ry + nz * rz < 0.0) {
      nx = -nx; ny = -ny; nz = -nz;
    }
  }
  Normal64 n;
  n.x = nx; n.y = ny; n.z = nz;
  return n;
}

// ---- the gripper box against a cloud: shared by collision_counts_kernel and the frame grading of eval_frames.hip, so
// that the counts behind the palm / in the fingers are the same integers by construction --------------------------------
struct GripperBox {
  float finger_length, bottom_length, half_hand_thickness, half_bottom_width, half_bottom_space,
      back_margin;
};

// rows 0..2 of a pose row's global -> local matrix G (row-major 4x4) as 12 floats (row-major 3x4)
__device__ __forceinline__ void load_g2l(const float* __restrict__ G, int invert_se3, float* __restrict__ o) {
  float g00 = G[0], g01 = G[1], g02 = G[2], g03 = G[3];
  float g10 = G[4], g11 = G[5], g12 = G[6], g13 = G[7];
  float g20 = G[8], g21 = G[9], g22 = G[10], g23 = G[11];
  if (invert_se3) {
    // the matrix is the POSE (gripper -> global): its analytic SE(3) inverse [R^T | -R^T t] in fp32
    // (torch_batch_transformation_inv, utils/math_utils.py:26-40, as grasp_detector.py:219 calls it) -- formed
    // here instead of by a batched 3x3 library GEMM per call (0.26 ms for 16 x 2 048 poses)
    const float tx = g03, ty = g13, tz = g23;
    const float r01 = g01, r02 = g02, r12 = g12;
    g01 = g10; g02 = g20; g12 = g21;
    g10 = r01; g20 = r02; g21 = r12;
    g03 = -__fadd_rn(__fadd_rn(__fmul_rn(g00, tx), __fmul_rn(g01, ty)), __fmul_rn(g02, tz));
    g13 = -__fadd_rn(__fadd_rn(__fmul_rn(g10, tx), __fmul_rn(g11, ty)), __fmul_rn(g12, tz));
    g23 = -__fadd_rn(__fadd_rn(__fmul_rn(g20, tx), __fmul_rn(g21, ty)), __fmul_rn(g22, tz));
  }
  o[0] = g00; o[1] = g01; o[2] = g02; o[3] = g03;
  o[4] = g10; o[5] = g11; o[6] = g12; o[7] = g13;
  o[8] = g20; o[9] = g21; o[10] = g22; o[11] = g23;
}

// the regions of view_collision_checker.py:39-60 / eval_point_cloud.py:70-97 for one point; every inequality strict
struct GripperRegions {
  bool back, fing, closer, slab;     // slab: the depth slab alone, -bottom_length < lx < finger_length
  float ly;
};
__device__ __forceinline__ GripperRegions gripper_regions(const float* __restrict__ g, float x, float y, float z,
                                                          const GripperBox& p) {
  const LocalPoint l = local_point(g, x, y, z);
  const float lx = l.x, ly = l.y, lz = l.z;
  const bool close = (lx < p.finger_length) && (lx > -p.bottom_length);                    // :39-40 / :70-71
  const bool zin = (lz < p.half_hand_thickness) && (lz > -p.half_hand_thickness);          // :44-45 / :75-76
  GripperRegions r;
  r.back = close && zin && (ly < p.half_bottom_width) && (ly > -p.half_bottom_width) && (lx < -p.back_margin);   // :47-49
  const bool fl = (ly < p.half_bottom_width) && (ly > p.half_bottom_space);                // :54-55
  const bool fr = (ly > -p.half_bottom_width) && (ly < -p.half_bottom_space);              // :56-57
  r.fing = close && zin && (fl || fr);                                                      // :59-60
  r.closer = close && zin && (ly < p.half_bottom_space) && (ly > -p.half_bottom_space);    // eval_point_cloud.py:95-97
  r.slab = close;
  r.ly = ly;
  return r;
}

}  // namespace s4g
