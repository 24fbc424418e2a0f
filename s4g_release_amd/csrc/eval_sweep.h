// The two cloud scans behind the antipodal score of a pose against a dense labelled scene, written once:
// s4g_eval_frames_f32 (eval_frames.hip) and s4g_eval_scene_grade_f32 (eval_data.hip) both compile them, so the counts,
// the label test, the y extrema, the bands and the band sums of the two are the same bits by construction.  The two
// classes differ in their gates (which pose reaches the score) and in one counter: SCENE = true also counts the depth
// slab (-BOTTOM_LENGTH < lx < FINGER_LENGTH, word 7 of a pose's accumulators, which SCENE = false never touches) and
// skips the poses whose `live` entry is 0.  The tuning constants stay with their kernels and come in as template
// arguments; the init and finish kernels stay in their files.
#pragma once
#include "frame_sweep.h"

namespace s4g {

struct EvalParams {
  GripperBox box;                  // the collision counter's six values
  float back_threshold, finger_threshold, min_points, neighbor_depth;
};

constexpr int EV_ACC = 8;          // per-pose accumulator ints: back, finger, close, label min, label max, y max, y min, slab

// the per-pose accumulators (workspace) to their neutral values: no memset, every launch of a call is a kernel
static __global__ __launch_bounds__(256) void eval_init_kernel(int* __restrict__ acc, int64_t n_pose) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pose * EV_ACC) return;
  acc[i] = acc_neutral((int)(i % EV_ACC));
}

// The first scan, points outer, poses inner: a workgroup keeps 256 * U points in registers and runs all its poses over
// them.  Labels are read only where a wave has a close-region point (rare: the region is a few cm wide).
// grid (GX, chunks, B), 256 threads; SLOTS poses per workgroup and pass.
template <bool SCENE, int GX, int U, int SLOTS>
__device__ __forceinline__ void eval_scan(
    const float* __restrict__ xyz, const int* __restrict__ labels, const float* __restrict__ g2l, int N, int K,
    const GripperBox& box, int* __restrict__ acc, const int64_t* __restrict__ pose_count,
    const int* __restrict__ live, int invert_se3) {
  __shared__ float gl[SLOTS][12];
  __shared__ int cnt[SLOTS][EV_ACC];
  __shared__ int on[SCENE ? SLOTS : 1];             // SCENE: the pose is scanned
  const int b = blockIdx.z, t = threadIdx.x, lane = t & 63;
  const float* px = xyz + (size_t)b * 3 * N;
  const int* lab = labels + (size_t)b * N;
  const ChunkRange rg = chunk_range(N);
  if (rg.empty()) return;
  const int kmax = frame_rows(pose_count, b, K);
  for (int j0 = 0; blockIdx.x + GX * j0 < kmax; j0 += SLOTS) {
    __syncthreads();                                  // (the previous pass's tables have been read)
    if (t < SLOTS) {
      const int k = blockIdx.x + GX * (j0 + t);
#pragma unroll
      for (int w = 0; w < ACC_WORDS; ++w) cnt[t][w] = acc_neutral(w);
      if (k < kmax) load_g2l(g2l + ((size_t)b * K + k) * 16, invert_se3, gl[t]);
      if constexpr (SCENE) {
        cnt[t][7] = 0;
        on[t] = k < kmax && (!live || live[(size_t)b * K + k] != 0);
      }
    }
    __syncthreads();
    const int nslot = pass_slots(kmax, GX, j0, SLOTS);
    for (int i0 = rg.lo + t; i0 < sweep_end<U>(rg.hi); i0 += 256 * U) {
      PointBlock<U> pt;
      pt.load(px, N, i0, rg.hi);
      for (int sl = 0; sl < nslot; ++sl) {
        if constexpr (SCENE) {
          if (!on[sl]) continue;                      // (workgroup-uniform) a pose that is not scanned
        }
        float g[12];
#pragma unroll
        for (int c = 0; c < 12; ++c) g[c] = gl[sl][c];
        int nback = 0, nfing = 0, nclose = 0, nslab = 0;
        int lmin = INT_MAX, lmax = INT_MIN, ymx = INT_MIN, ymn = INT_MAX;
        bool hit = false;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const GripperRegions r = gripper_regions(g, pt.x[u], pt.y[u], pt.z[u], box);
          const bool cr = pt.in[u] && r.closer;
          nback += __popcll(__ballot(pt.in[u] && r.back));      // wave-uniform
          nfing += __popcll(__ballot(pt.in[u] && r.fing));
          nclose += __popcll(__ballot(cr));
          if constexpr (SCENE) nslab += __popcll(__ballot(pt.in[u] && r.slab));
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
          if constexpr (SCENE) {
            if (nslab) atomicAdd(&cnt[sl][7], nslab);
          }
        }
        if (hit) {
          atomicMin(&cnt[sl][3], lmin); atomicMax(&cnt[sl][4], lmax);
          atomicMax(&cnt[sl][5], ymx); atomicMin(&cnt[sl][6], ymn);
        }
      }
    }
    __syncthreads();
    if (t < nslot) {
      const int k = blockIdx.x + GX * (j0 + t);
      int* a = acc + ((size_t)b * K + k) * EV_ACC;
      if (cnt[t][0]) atomicAdd(a + 0, cnt[t][0]);
      if (cnt[t][1]) atomicAdd(a + 1, cnt[t][1]);
      if (cnt[t][2]) {
        atomicAdd(a + 2, cnt[t][2]);
        atomicMin(a + 3, cnt[t][3]); atomicMax(a + 4, cnt[t][4]);
        atomicMax(a + 5, cnt[t][5]); atomicMin(a + 6, cnt[t][6]);
      }
      if constexpr (SCENE) {
        if (cnt[t][7]) atomicAdd(a + 7, cnt[t][7]);
      }
    }
  }
}

// The second scan.  A workgroup keeps, per pass, only those of its SLOTS poses that reached the score -- Gate()(row,
// accumulators) says which -- compacted in pose order, so a pass without one costs a table load and no cloud read.
// part (B, K, chunks, 4) = {sum left, sum right, n left, n right (int bits)} is written for every (scored pose,
// non-empty chunk) and read for nothing else.  No floating-point atomics: a wave tree-sums the points of a sweep, adds
// that to its own accumulator, the four waves of a workgroup are summed in a fixed order.  SLOTS * 8 must be 256.
template <int GX, int U, int SLOTS, class Gate>
__device__ __forceinline__ void eval_band(
    const float* __restrict__ xyz, const float* __restrict__ normals, const float* __restrict__ g2l, int N, int K,
    const GripperBox& box, float neighbor_depth, const Gate& gate, const int* __restrict__ acc,
    float* __restrict__ part, const int64_t* __restrict__ pose_count, int invert_se3) {
  static_assert(SLOTS * 8 == 256, "one thread per (slot, wave, side) cell");
  __shared__ float gl[SLOTS][12];
  __shared__ float thr[SLOTS][2];
  __shared__ int kof[SLOTS];
  __shared__ int nlive;
  __shared__ float wsum[SLOTS][4][2];
  __shared__ int wcnt[SLOTS][4][2];
  const int b = blockIdx.z, chunk = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const float* px = xyz + (size_t)b * 3 * N;
  const float* pn = normals + (size_t)b * 3 * N;
  const int nchunk = (int)gridDim.y;
  const ChunkRange rg = chunk_range(N);
  if (rg.empty()) return;                            // the finish kernels do not read an empty chunk's partials
  const int kmax = frame_rows(pose_count, b, K);
  for (int j0 = 0; blockIdx.x + GX * j0 < kmax; j0 += SLOTS) {
    __syncthreads();
    if (t < SLOTS) {                                  // (the first 32 lanes of wave 0)
      const int k = blockIdx.x + GX * (j0 + t);
      bool live = false;
      float lthr = 0.f, rthr = 0.f;
      if (k < kmax) {
        const int* a = acc + ((size_t)b * K + k) * EV_ACC;
        live = gate((size_t)b * K + k, a);
        const float left_y = ord2f(a[5]), right_y = ord2f(a[6]);                             // :52-53
        const float depth = fminf(__fdiv_rn(__fsub_rn(left_y, right_y), 3.0f), neighbor_depth);   // :54
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
    ((float*)wsum)[t] = 0.f;                          // SLOTS x 4 x 2 = 256 entries each
    ((int*)wcnt)[t] = 0;
    __syncthreads();
    const int nslot = nlive;
    if (nslot == 0) continue;                         // workgroup-uniform
    for (int i0 = rg.lo + t; i0 < sweep_end<U>(rg.hi); i0 += 256 * U) {
      PointBlock<U> pt;
      pt.load(px, N, i0, rg.hi);
      for (int sl = 0; sl < nslot; ++sl) {
        float g[12];
#pragma unroll
        for (int c = 0; c < 12; ++c) g[c] = gl[sl][c];
        const float lthr = thr[sl][0], rthr = thr[sl][1];
        int nl = 0, nr = 0;
        float sl_ = 0.f, sr_ = 0.f;                   // this lane's (at most U, nearly always at most 1) band terms
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const GripperRegions r = gripper_regions(g, pt.x[u], pt.y[u], pt.z[u], box);
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

// a scored pose's band populations and means from its chunk partials q (nchunk, 4): the pairwise sum of the partials in
// chunk order (a binary counter of pending subtree sums), then torch.mean (:61); an empty band gives NaN there and here
struct BandMeans {
  int n_left, n_right;
  float mean_left, mean_right;
};
__device__ __forceinline__ BandMeans eval_band_means(const float* __restrict__ q, int N, int nchunk) {
  float stl[8], str[8];
  int nl = 0, nr = 0, j = 0;
  const int nc = (N + nchunk - 1) / nchunk;
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
  BandMeans m;
  m.n_left = nl; m.n_right = nr;
  m.mean_left = __fdiv_rn(sl_, (float)nl);
  m.mean_right = __fdiv_rn(sr_, (float)nr);
  return m;
}

}  // namespace s4g
