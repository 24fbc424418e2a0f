// Labels of the contact model (MODEL.TYPE "PN2"): the data generator's TorchPrecomputedSingleViewPointCloud
// (data_gen/pcd_classes/torch_contact_single_view_point_cloud.py) restated for every scene frame of every scene.
// Contract: include/s4g_ops.h (s4g_contact_search_f32, s4g_contact_select_f32).
//
// s4g_contact_search_f32 = finger_hand (:251-294) with _table_collision_check (:236-249), which run_score (:183-185)
// drives as a Python loop over every (view point, frame) pair: one 4 x M product, nine sets of boolean masks, a
// torch.unique and a host read each.  Grading reads global_to_local and the scene alone, so a scene frame is graded
// ONCE per scene here, whichever view points picked it.
//
// Per frame: nz heights x ny widths x nx lengths = P placements (3 x 3 x 1 as shipped), index (iz * ny + iy) * nx + ix:
// the reference's loops, dz outer, dx inner.  The placements share the frame, so a scene point is transformed ONCE per
// frame; they differ in the bounds of a device table only.  A point further from the frame's origin (in local
// coordinates) than the circumradius of the box widened by the largest shifts is in no region of any placement.
//
//   cs_setup_kernel   the neutral values of every accumulator (no memset: every launch of the call is a kernel)
//   cs_scan_kernel    a cloud sweep (frame_sweep.h: points outer, frames inner): per placement the counts in the fingers / in
//                     the close region / of close points behind the margin and the label minimum / maximum, in LDS,
//                     then the workspace; integer atomics only, so the result does not depend on their order
//   cs_finish_kernel  per frame: the table verdict of the centred box, the verdicts of the placements, the failure
//                     bits, validity and the label
//
// Decisions.  (1) An empty close region makes the reference raise (min() of an empty tensor, :286): here the frame is
// invalid, fail bit 4.  (2) local_to_global is the rigid inverse [R^T | -R^T t] formed here from g2l, not
// torch.inverse (:120); g2l must be rigid and is not checked.  (3) A g2l entry that is not finite: the frame is not
// scanned, invalid, fail bit 5.  (4) The table verdict covers the centred box only: LOCAL_SEARCH_TO_LOCAL (:18-28) is
// written element by element into an expand()ed tensor, the writes alias and all nine matrices end as the identity.
//
// s4g_contact_select_f32 = the rest of _find_match (:146-173) and of run_score (:189-208), one thread per view point:
// the scene normal of its nearest scene point, normalised in double and turned towards the camera, and the fold of
// the valid frames of that scene point in ascending frame index (:200-206).
//
// Limits: M < 2^30, F < 2^30 (the frame loops run inside the kernels or over grid.x), B <= 65 535 (grid.y / grid.z).
#include "frame_sweep.h"

namespace s4g {

constexpr int CS_MAX_LIST = 4;           // compiled maximum of each of the three shift lists
constexpr int CS_MAX_P = CS_MAX_LIST * CS_MAX_LIST * CS_MAX_LIST;
constexpr int CS_GX = 64;                // workgroups that share a scene's frame list (frame k belongs to workgroup k mod 64)
constexpr int CS_U = 4;                  // points per lane held in registers while the workgroup's frames pass over them
constexpr int CS_SLOTS = 8;              // frames per workgroup and pass: 512 per scene and pass
constexpr int CS_CHUNK_POINTS = 16384;   // point ranges per scene: ceil(M / 16 384) within [4, 64]
constexpr int CS_MIN_CHUNKS = 4;
constexpr int CS_MAX_CHUNKS = 64;
constexpr int CS_ACC = 5;                // per placement: finger, close, behind, label min, label max

struct CsParams {
  float fl, bl, hht, hbw, hbs, margin, table_limit;   // the gripper box, BACK_COLLISION_MARGIN, TABLE_HEIGHT + OFFSET
  float r2cull;                                       // the cull radius squared, with slack
  int nz, ny, nx, no_label;
};

// device table layout (floats): z lower[nz], z upper[nz], y lower[ny], y upper[ny], dy[ny], x lower[nx], x upper[nx]
struct CsTables {
  float zlo[CS_MAX_LIST], zhi[CS_MAX_LIST], ylo[CS_MAX_LIST], yhi[CS_MAX_LIST], dy[CS_MAX_LIST], xlo[CS_MAX_LIST],
      xhi[CS_MAX_LIST];
};

// one thread per accumulator set
__global__ __launch_bounds__(256) void cs_setup_kernel(int* __restrict__ acc, size_t sets) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= sets) return;
  int* a = acc + i * CS_ACC;
#pragma unroll
  for (int w = 0; w < CS_ACC; ++w) a[w] = acc_neutral(w);
}

__global__ __launch_bounds__(256) void cs_scan_kernel(
    const float* __restrict__ xyz, const int* __restrict__ labels, const float* __restrict__ g2l,
    const float* __restrict__ tables, int M, int F, CsParams p, int* __restrict__ acc,
    const int64_t* __restrict__ frame_count) {
  __shared__ float gl[CS_SLOTS][12];
  __shared__ int live[CS_SLOTS];
  __shared__ int cnt[CS_SLOTS][CS_MAX_P][CS_ACC];
  __shared__ CsTables tb;
  const int b = blockIdx.z, t = threadIdx.x;
  const int nz = p.nz, ny = p.ny, nx = p.nx, P = nz * ny * nx;
  const float* px = xyz + (size_t)b * 3 * M;
  const int* lab = labels + (size_t)b * M;
  const ChunkRange rg = chunk_range(M);
  if (rg.empty()) return;
  if (t < nz) { tb.zlo[t] = tables[t]; tb.zhi[t] = tables[nz + t]; }
  if (t < ny) { tb.ylo[t] = tables[2 * nz + t]; tb.yhi[t] = tables[2 * nz + ny + t]; tb.dy[t] = tables[2 * nz + 2 * ny + t]; }
  if (t < nx) { tb.xlo[t] = tables[2 * nz + 3 * ny + t]; tb.xhi[t] = tables[2 * nz + 3 * ny + nx + t]; }
  const int fmax = frame_rows(frame_count, b, F);
  for (int j0 = 0; (int)blockIdx.x + CS_GX * j0 < fmax; j0 += CS_SLOTS) {
    __syncthreads();                                  // (the previous pass's accumulators have been flushed)
    const int nslot = pass_slots(fmax, CS_GX, j0, CS_SLOTS);
    if (t < nslot) {
      const float* G = g2l + ((size_t)b * F + blockIdx.x + (size_t)CS_GX * (j0 + t)) * 16;
      bool ok = true;
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        const float v = G[c];
        ok = ok && finite(v);
        if (c < 12) gl[t][c] = v;
      }
      live[t] = ok ? 1 : 0;                           // a frame with an entry that is not finite is never scanned
    }
    for (int i = t; i < nslot * P * CS_ACC; i += 256) {
      ((int*)cnt[i / (P * CS_ACC)])[i % (P * CS_ACC)] = acc_neutral(i % CS_ACC);
    }
    __syncthreads();
    // (the narrow bound, not sweep_end, and masked lanes on point i0 < hi: no ballot or shuffle below, and this kernel
    //  has no scalar register to spare at 8 waves per SIMD: frame_sweep.h)
    for (int i0 = rg.lo + t; i0 < rg.hi; i0 += 256 * CS_U) {
      PointBlock<CS_U> pt;
      pt.load(px, M, i0, rg.hi, i0);
      for (int sl = 0; sl < nslot; ++sl) {
        if (!live[sl]) continue;                      // workgroup-uniform
        float g[12];
#pragma unroll
        for (int c = 0; c < 12; ++c) g[c] = gl[sl][c];
#pragma unroll
        for (int u = 0; u < CS_U; ++u) {
          const LocalPoint l = local_point(g, pt.x[u], pt.y[u], pt.z[u]);
          const float lx = l.x, ly = l.y, lz = l.z;
          // the cull; a point that is not finite gives NaN or inf here and is in no region
          if (!pt.in[u] || !(lx * lx + ly * ly + lz * lz < p.r2cull)) continue;
          unsigned zb = 0, xb = 0, yb = 0, yc = 0;
          for (int k = 0; k < nz; ++k) zb |= (((lz < tb.zhi[k]) && (lz > tb.zlo[k])) ? 1u : 0u) << k;       // :271-272
          if (!zb) continue;
          for (int k = 0; k < nx; ++k) xb |= (((lx > tb.xlo[k]) && (lx < tb.xhi[k])) ? 1u : 0u) << k;       // :280-281
          if (!xb) continue;
          for (int k = 0; k < ny; ++k) {
            yb |= (((ly < tb.yhi[k]) && (ly > tb.ylo[k])) ? 1u : 0u) << k;                                  // :274-275
            const float ay = fabsf(ly + tb.dy[k]);                                                          // :276
            yc |= (((ay > p.hbs) && (ay < p.hbw)) ? 1u : 0u) << k;                                          // :277
          }
          if (!(yb | yc)) continue;
          const bool behind = lx < p.margin;                                                                // :286
          const int lb = lab[i0 + 256 * u];       // (= pt.idx[u] of a point in range; four registers less)
          for (int kz = 0; kz < nz; ++kz) {
            if (!((zb >> kz) & 1u)) continue;
            for (int ky = 0; ky < ny; ++ky) {
              const bool closer = (yb >> ky) & 1u, fing = (yc >> ky) & 1u;
              if (!(closer || fing)) continue;
              for (int kx = 0; kx < nx; ++kx) {
                if (!((xb >> kx) & 1u)) continue;
                int* a = cnt[sl][(kz * ny + ky) * nx + kx];
                if (fing) atomicAdd(a + 0, 1);                                                              // :282
                if (closer) {                                                                               // :285
                  atomicAdd(a + 1, 1);
                  if (behind) atomicAdd(a + 2, 1);
                  atomicMin(a + 3, lb); atomicMax(a + 4, lb);                                               // :288
                }
              }
            }
          }
        }
      }
    }
    __syncthreads();
    for (int i = t; i < nslot * P; i += 256) {
      const int sl = i / P, pl = i % P;
      const int* c = cnt[sl][pl];
      int* a = acc + (((size_t)b * F + blockIdx.x + (size_t)CS_GX * (j0 + sl)) * P + pl) * CS_ACC;
      if (c[0]) atomicAdd(a + 0, c[0]);
      if (c[1]) {
        atomicAdd(a + 1, c[1]);
        if (c[2]) atomicAdd(a + 2, c[2]);
        atomicMin(a + 3, c[3]); atomicMax(a + 4, c[4]);
      }
    }
  }
}

// one thread per frame
__global__ __launch_bounds__(256) void cs_finish_kernel(
    const float* __restrict__ g2l, const int* __restrict__ acc, int F, CsParams p,
    const int64_t* __restrict__ frame_count, int* __restrict__ ints, int* __restrict__ table, int* __restrict__ valid,
    int* __restrict__ label, int* __restrict__ fail) {
  const int b = blockIdx.y;
  const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= (size_t)F) return;
  const size_t row = (size_t)b * F + f;
  const int P = p.nz * p.ny * p.nx;
  const bool row_in = f < (size_t)frame_rows(frame_count, b, F);
  float G[16];
  bool all_finite = true;
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    G[c] = g2l[row * 16 + c];
    all_finite = all_finite && finite(G[c]);
  }
  int* oi = ints + row * P * 4;
  int bits = 0, hit = 0, lbl = p.no_label;
  if (!row_in || !all_finite) {
    for (int i = 0; i < P * 4; ++i) oi[i] = 0;
    if (row_in) bits = 32;
  } else {
    // row 2 of local_to_global = [R^T | -R^T t]: column 2 of R and the z of -R^T t; the corners are GRIPPER_BOUND
    // (configs/config.py:58-64) under the identity search matrix (:244-248)
    const float m0 = G[2], m1 = G[6], m2 = G[10];
    const float m3 = -__fadd_rn(__fadd_rn(__fmul_rn(m0, G[3]), __fmul_rn(m1, G[7])), __fmul_rn(m2, G[11]));
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float cx = (k & 4) ? -p.bl : p.fl, cy = (k & 2) ? -p.hbw : p.hbw, cz = (k & 1) ? -p.hht : p.hht;
      hit |= (m0 * cx + m1 * cy + m2 * cz + m3 < p.table_limit) ? 1 : 0;             // :248
    }
    bits = hit;
    for (int pl = 0; pl < P; ++pl) {
      const int* a = acc + (row * P + pl) * CS_ACC;
      const int fing = a[0], close = a[1], behind = a[2];
      const int multi = (close > 0 && a[3] != a[4]) ? 1 : 0;
      oi[pl * 4] = fing; oi[pl * 4 + 1] = close; oi[pl * 4 + 2] = behind; oi[pl * 4 + 3] = multi;
      bits |= (fing > 0 ? 2 : 0) | (behind > 0 ? 4 : 0) | (multi ? 8 : 0) | (close == 0 ? 16 : 0);
    }
    if (bits == 0) lbl = acc[(row * P + P - 1) * CS_ACC + 3];                       // :293, the last placement's label
  }
  table[row] = hit;
  valid[row] = (row_in && all_finite && bits == 0) ? 1 : 0;
  label[row] = lbl;
  fail[row] = bits;
}

// one thread per view point
__global__ __launch_bounds__(256) void cs_select_kernel(
    const int* __restrict__ nearest, const float* __restrict__ cloud, const float* __restrict__ scene_normals,
    const float* __restrict__ camera, const int* __restrict__ offsets, const int* __restrict__ order,
    const int* __restrict__ valid, const float* __restrict__ search, const float* __restrict__ antipodal, int N, int M,
    int F, float* __restrict__ normals, int* __restrict__ best_frame, float* __restrict__ point_score) {
  const int b = blockIdx.y;
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= (size_t)N) return;
  int i = nearest[(size_t)b * N + q];
  if (i >= M) i = -1;                                  // (cannot happen for s4g_match_nearest_f32's output)
  double nx = 0.0, ny = 0.0, nz = 1.0;                 // no neighbour: it must be table (:146-148)
  if (i >= 0) {
    const float* n0 = scene_normals + (size_t)b * 3 * M;
    const double ax = (double)n0[i], ay = (double)n0[(size_t)M + i], az = (double)n0[2 * (size_t)M + i];
    const double len = sqrt(ax * ax + ay * ay + az * az);
    nx = ax / len; ny = ay / len; nz = az / len;       // a zero normal gives NaN, as numpy does (:166)
  }
  const float* c0 = cloud + (size_t)b * 3 * N;
  const float* cam = camera + (size_t)b * 3;
  const double rx = (double)cam[0] - (double)c0[q], ry = (double)cam[1] - (double)c0[(size_t)N + q],
               rz = (double)cam[2] - (double)c0[2 * (size_t)N + q];
  if (finite(rx) && finite(ry) && finite(rz)) {   // no reference direction otherwise: n stays
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
  float* o = normals + (size_t)b * 3 * N;
  o[q] = (float)nx;
  o[(size_t)N + q] = (float)ny;
  o[2 * (size_t)N + q] = (float)nz;
  float best = 0.f;
  int arg = -1;
  if (i >= 0) {
    const int* off = offsets + (size_t)b * ((size_t)M + 1);
    const int lo = max(0, off[i]), hi = min(F, off[i + 1]);
    for (int k = lo; k < hi; ++k) {                    // the frames of scene point i in ascending frame index (:152)
      const int f = order[(size_t)b * F + k];
      if (f < 0 || f >= F || !valid[(size_t)b * F + f]) continue;                  // :198
      const float s = __fdiv_rn(logf(search[(size_t)b * F + f]), 6.5f);            // :189
      const float m = (s != s) ? s : fminf(s, 1.0f);                               // :190-192, torch.min keeps a NaN
      const float sc = __fmul_rn(m, antipodal[(size_t)b * F + f]);                 // :193
      if (best > sc) continue;                                                     // :202-203
      best = sc;                                                                   // :205-206: an equal score picks the later frame
      arg = f;
    }
  }
  point_score[(size_t)b * N + q] = best;
  best_frame[(size_t)b * N + q] = (best > 0.f) ? arg : -1;                         // :208
}

}  // namespace s4g

extern "C" size_t s4g_contact_search_workspace_bytes(int64_t B, int64_t M, int64_t F, int64_t P) {
  (void)M;
  if (B <= 0 || F <= 0 || P <= 0 || P > s4g::CS_MAX_P) return 0;
  return s4g::align256((size_t)B * (size_t)F * (size_t)P * s4g::CS_ACC * sizeof(int));
}

extern "C" int s4g_contact_search_f32(const float* g2l_bf44, const float* xyz_b3m, const int32_t* labels_bm, int64_t B,
                                      int64_t M, int64_t F, int64_t nz, int64_t ny, int64_t nx, const float* params10,
                                      int32_t no_label, const float* tables_2z3y2x, const int64_t* frame_count_b,
                                      int32_t* ints_bfp4, int32_t* table_bf, int32_t* valid_bf, int32_t* label_bf,
                                      int32_t* fail_bf, void* workspace, size_t workspace_bytes, s4g_stream_t stream) {
  using namespace s4g;
  if (B < 0 || M <= 0 || F < 0 || B > 65535 || F >= (1ll << 30) || M >= (1ll << 30)) return S4G_EINVAL;
  if (nz <= 0 || ny <= 0 || nx <= 0 || nz > CS_MAX_LIST || ny > CS_MAX_LIST || nx > CS_MAX_LIST) return S4G_EINVAL;
  if (B == 0 || F == 0) return S4G_OK;
  if (!g2l_bf44 || !xyz_b3m || !labels_bm || !params10 || !tables_2z3y2x || !ints_bfp4 || !table_bf || !valid_bf ||
      !label_bf || !fail_bf)
    return S4G_EINVAL;
  const int64_t P = nz * ny * nx;
  const size_t sets = (size_t)B * (size_t)F * (size_t)P;
  if ((sets + 255) / 256 > 0x7fffffffull) return S4G_EINVAL;       // (cs_setup_kernel's grid)
  if (!workspace || workspace_bytes < s4g_contact_search_workspace_bytes(B, M, F, P)) return S4G_EWORKSPACE;
  CsParams p;
  p.fl = params10[0]; p.bl = params10[1]; p.hht = params10[2]; p.hbw = params10[3]; p.hbs = params10[4];
  p.margin = params10[5]; p.table_limit = params10[6];
  // the box widened by the largest shifts: |x| < max(fl, bl) + |dx|, |y| < hbw + |dy|, |z| < hht + |dz|; the fp32
  // sum of squares is within 1e-6 relative of the exact one, the slack is 1e-3
  const float ex = (p.fl > p.bl ? p.fl : p.bl) + fabsf(params10[7]), ey = p.hbw + fabsf(params10[8]),
              ez = p.hht + fabsf(params10[9]);
  p.r2cull = (ex * ex + ey * ey + ez * ez) * 1.001f;
  p.nz = (int)nz; p.ny = (int)ny; p.nx = (int)nx; p.no_label = no_label;
  hipStream_t st = (hipStream_t)stream;
  int* acc = (int*)workspace;
  hipLaunchKernelGGL(cs_setup_kernel, dim3((unsigned)((sets + 255) / 256)), dim3(256), 0, st, acc, sets);
  S4G_LAUNCH_CHECK();
  const dim3 grid(CS_GX, (unsigned)sweep_chunks(M, CS_CHUNK_POINTS, CS_MIN_CHUNKS, CS_MAX_CHUNKS), (unsigned)B);
  hipLaunchKernelGGL(cs_scan_kernel, grid, dim3(256), 0, st, xyz_b3m, (const int*)labels_bm, g2l_bf44, tables_2z3y2x,
                     (int)M, (int)F, p, acc, frame_count_b);
  S4G_LAUNCH_CHECK();
  hipLaunchKernelGGL(cs_finish_kernel, dim3((unsigned)((F + 255) / 256), (unsigned)B), dim3(256), 0, st, g2l_bf44,
                     (const int*)acc, (int)F, p, frame_count_b, (int*)ints_bfp4, (int*)table_bf, (int*)valid_bf,
                     (int*)label_bf, (int*)fail_bf);
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}

extern "C" int s4g_contact_select_f32(const int32_t* nearest_bn, const float* cloud_b3n, const float* scene_normals_b3m,
                                      const float* camera_b3, const int32_t* offsets_bm1, const int32_t* order_bf,
                                      const int32_t* valid_bf, const float* search_bf, const float* antipodal_bf,
                                      int64_t B, int64_t N, int64_t M, int64_t F, float* normals_b3n,
                                      int32_t* best_frame_bn, float* point_score_bn, int32_t* valid_index_bn,
                                      int64_t* count_b, s4g_stream_t stream) {
  using namespace s4g;
  if (B < 0 || B > 65535 || N < 0 || N >= (1ll << 30) || M < 1 || M >= (1ll << 30) || F < 0 || F >= (1ll << 30))
    return S4G_EINVAL;
  if (B == 0) return S4G_OK;
  if (!count_b || !offsets_bm1 || !scene_normals_b3m || !camera_b3) return S4G_EINVAL;
  if (N > 0 && (!nearest_bn || !cloud_b3n || !normals_b3n || !best_frame_bn || !point_score_bn || !valid_index_bn))
    return S4G_EINVAL;
  if (F > 0 && (!order_bf || !valid_bf || !search_bf || !antipodal_bf)) return S4G_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (N > 0) {
    hipLaunchKernelGGL(cs_select_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)B), dim3(256), 0, st,
                       (const int*)nearest_bn, cloud_b3n, scene_normals_b3m, camera_b3, (const int*)offsets_bm1,
                       (const int*)order_bf, (const int*)valid_bf, search_bf, antipodal_bf, (int)N, (int)M, (int)F,
                       normals_b3n, (int*)best_frame_bn, point_score_bn);
    S4G_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(compact_valid_kernel<KeepNonNegative>, dim3((unsigned)B), dim3(256), 0, st, (const int*)best_frame_bn, (int)N,
                     (int*)valid_index_bn, count_b);
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}
