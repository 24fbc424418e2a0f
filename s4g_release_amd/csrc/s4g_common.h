// Device-side helpers shared by the gfx950 kernels of libs4g_hip.so.
// Wave = 64 lanes everywhere; this code targets CDNA4 only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/s4g_ops.h"

#define S4G_WAVE 64

#define S4G_LAUNCH_CHECK()                        \
  do {                                            \
    hipError_t e_ = hipGetLastError();            \
    if (e_ != hipSuccess) return (int)e_;         \
  } while (0)

#include <atomic>
#include <cstdlib>
#include <cstring>

namespace s4g {
// A/B and test knobs (include/s4g_ops.h lists them): read from the environment ONLY when the process also sets
// S4G_TEST_KNOBS=1.  A production process that does not set the master switch cannot have its kernel selection changed
// by a stray variable in some launcher's environment; every knob selects an exact path, so the switch changes speed,
// never results.  Not cached: tests flip it within one process.
inline bool test_knobs_enabled() {
  const char* m = getenv("S4G_TEST_KNOBS");
  return m && m[0] == '1' && m[1] == 0;
}
inline const char* knob(const char* name) { return test_knobs_enabled() ? getenv(name) : nullptr; }
}  // namespace s4g

namespace s4g {

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE setting: one slot per (call site,
// device), set on the first launch there and again whenever a launch needs more than the slot
// holds; a failure is returned to the caller and never memoised.
struct LdsAttrCache {
  std::atomic<int> bytes[64];
};
inline int allow_dynamic_lds(const void* func, size_t lds_bytes, LdsAttrCache& cache) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  const bool slot = dev >= 0 && dev < 64;
  if (slot && cache.bytes[dev].load(std::memory_order_relaxed) >= (int)lds_bytes) return 0;
  e = hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  if (e != hipSuccess) return (int)e;
  if (slot) cache.bytes[dev].store((int)lds_bytes, std::memory_order_relaxed);
  return 0;
}

// Squared distance with the arithmetic contract of include/s4g_ops.h.
// The translation units are compiled with -ffp-contract=off, and the
// __f*_rn intrinsics additionally pin each rounding.
template <bool FMAD>
__device__ __forceinline__ float dist2(float x1, float y1, float z1, float x2,
                                       float y2, float z2) {
  const float dx = __fsub_rn(x2, x1);
  const float dy = __fsub_rn(y2, y1);
  const float dz = __fsub_rn(z2, z1);
  if constexpr (FMAD) {
    float t = __fmul_rn(dx, dx);
    t = __fmaf_rn(dy, dy, t);
    t = __fmaf_rn(dz, dz, t);
    return t;
  } else {
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)),
                     __fmul_rn(dz, dz));
  }
}

// ---- DPP helpers (gfx9 encodings) ------------------------------------------
// quad_perm [1,0,3,2] = 0xB1, quad_perm [2,3,0,1] = 0x4E,
// row_half_mirror = 0x141, row_mirror = 0x140.
// (old = 0 with bound_ctrl: every lane of these permutations has a valid source, so the value is
// the same as with old = v -- but in this form the compiler folds the move into its consumer,
// `v_max_u32_dpp v, v, v quad_perm:...` = ONE instruction per reduction step instead of
// mov / nop / mov_dpp / max: half the instructions and half the dependent chain of every
// row16_* / wave_* reduction below)
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}

// After these four steps every lane holds the max of its row of 16 lanes.
__device__ __forceinline__ uint32_t row16_max_u32(uint32_t v) {
  v = max(v, dpp_u32<0xB1>(v));
  v = max(v, dpp_u32<0x4E>(v));
  v = max(v, dpp_u32<0x141>(v));
  v = max(v, dpp_u32<0x140>(v));
  return v;
}
__device__ __forceinline__ uint32_t row16_min_u32(uint32_t v) {
  v = min(v, dpp_u32<0xB1>(v));
  v = min(v, dpp_u32<0x4E>(v));
  v = min(v, dpp_u32<0x141>(v));
  v = min(v, dpp_u32<0x140>(v));
  return v;
}

// Wave-wide (64 lanes) reductions; the result is wave-uniform (SGPR).
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  v = row16_max_u32(v);
  const uint32_t a = __builtin_amdgcn_readlane(v, 0);
  const uint32_t b = __builtin_amdgcn_readlane(v, 16);
  const uint32_t c = __builtin_amdgcn_readlane(v, 32);
  const uint32_t d = __builtin_amdgcn_readlane(v, 48);
  return max(max(a, b), max(c, d));
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
  v = row16_min_u32(v);
  const uint32_t a = __builtin_amdgcn_readlane(v, 0);
  const uint32_t b = __builtin_amdgcn_readlane(v, 16);
  const uint32_t c = __builtin_amdgcn_readlane(v, 32);
  const uint32_t d = __builtin_amdgcn_readlane(v, 48);
  return min(min(a, b), min(c, d));
}

// Inclusive prefix sum over the 64 lanes: Hillis-Steele inside each row of 16
// (row_shr 1,2,4,8 with zero fill), then row_bcast15 / row_bcast31 carry the
// row totals across (6 DPP adds, no LDS crossbar traffic).
__device__ __forceinline__ uint32_t wave_inclusive_scan_u32(uint32_t v) {
#define S4G_DPP0(CTRL, RM) \
  (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, RM, 0xF, true)
  v += S4G_DPP0(0x111, 0xF);
  v += S4G_DPP0(0x112, 0xF);
  v += S4G_DPP0(0x114, 0xF);
  v += S4G_DPP0(0x118, 0xF);
  v += S4G_DPP0(0x142, 0xA);
  v += S4G_DPP0(0x143, 0xC);
#undef S4G_DPP0
  return v;
}

__device__ __forceinline__ int lane_id() {
  return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0));
}

// Number of set bits of `mask` strictly below this lane.
__device__ __forceinline__ int mask_rank(uint64_t mask) {
  return (int)__builtin_amdgcn_mbcnt_hi(
      (uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
}

// ---- gripper box against a cloud: shared by collision_counts_kernel (pose_decode.hip) and the frame grading
// (eval_frames.hip), so that the counts behind the palm / in the fingers are the same integers by construction ------
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

// the regions of view_collision_checker.py:39-60 / eval_point_cloud.py:70-97 for one point; every inequality strict,
// fp32, each op rounded on its own (these translation units are compiled with -ffp-contract=off)
struct GripperRegions {
  bool back, fing, closer;
  float ly;
};
__device__ __forceinline__ GripperRegions gripper_regions(const float* __restrict__ g, float x, float y, float z,
                                                          const GripperBox& p) {
  const float lx = g[0] * x + g[1] * y + g[2] * z + g[3];
  const float ly = g[4] * x + g[5] * y + g[6] * z + g[7];
  const float lz = g[8] * x + g[9] * y + g[10] * z + g[11];
  const bool close = (lx < p.finger_length) && (lx > -p.bottom_length);                    // :39-40 / :70-71
  const bool zin = (lz < p.half_hand_thickness) && (lz > -p.half_hand_thickness);          // :44-45 / :75-76
  GripperRegions r;
  r.back = close && zin && (ly < p.half_bottom_width) && (ly > -p.half_bottom_width) && (lx < -p.back_margin);   // :47-49
  const bool fl = (ly < p.half_bottom_width) && (ly > p.half_bottom_space);                // :54-55
  const bool fr = (ly > -p.half_bottom_width) && (ly < -p.half_bottom_space);              // :56-57
  r.fing = close && zin && (fl || fr);                                                      // :59-60
  r.closer = close && zin && (ly < p.half_bottom_space) && (ly > -p.half_bottom_space);    // eval_point_cloud.py:95-97
  r.ly = ly;
  return r;
}

}  // namespace s4g
