// Batched local grasp search against a dense, labelled scene cloud with normals: restates the per-point label search of
// the reference's data generator -- TorchSingleViewPointCloud.finger_hand with _table_collision_check and
// _antipodal_score (data_gen/pcd_classes/torch_single_view_point_cloud.py:152-180,224-358), which run_score (:198-201)
// drives as a Python loop over frames with 48 inner iterations of boolean-mask compactions, a torch.unique and several
// host reads each -- as six launches over all frames of all scenes, with no host synchronisation.
//
// Per frame: L approach depths x T rolls about the frame's x axis = L*T placements (4 x 12 as shipped).  They share the
// local x axis, so a scene point is transformed ONCE per frame; the roll keeps y^2 + z^2, so a point outside the cylinder
// y^2 + z^2 < half_bottom_width^2 + half_hand_thickness^2 or outside every depth slab is outside every region of every
// placement and only counts for the per-depth slab counters.
//
//   ls_setup_kernel    per frame: the two gates (:257,259), [R^T | -R^T p] (:91-94), the L*T table verdicts (:224-241)
//                      and the neutral values of the frame's accumulators (no memset: every launch of the call is a kernel)
//   ls_scan_kernel     first scan, a cloud sweep (frame_sweep.h: points outer, frames inner): the slab counters (:270-273) and,
//                      for the points that pass the cull, per placement that the table verdict lets through the counts
//                      behind the palm / in the fingers /
//                      in the close region, the label minimum / maximum and the ordered-integer y extrema; in LDS, then
//                      the workspace
//   ls_band_kernel     second scan, only for placements that reached the score: sum |n.y| over the two bands (:167-176)
//                      in 2^-30 fixed point with INTEGER atomics -- order independent, so results are bit-identical from
//                      run to run and batch invariant without a fixed reduction tree (one partial per (frame, chunk), as
//                      the pose grading keeps, would make the workspace 48 times as large: 48 placements per frame)
//   ls_finish_kernel   the gates in the reference's order, search score, label, antipodal score, frame validity (:348)
//   compact_valid_kernel (frame_sweep.h)  valid_index: the valid frames of a scene in ascending order, -1 padded, and their count
#include "frame_sweep.h"

namespace s4g {

constexpr int LS_MAX_L = 8;          // compiled maxima of the depth and roll lists
constexpr int LS_MAX_T = 16;
constexpr int LS_MAX_P = LS_MAX_L * LS_MAX_T;
constexpr int LS_GX = 32;            // workgroups that share a scene's frame list (frame k belongs to workgroup k mod 32)
constexpr int LS_U = 4;              // points per lane held in registers while the workgroup's frames pass over them
constexpr int LS_SLOTS = 8;          // frames per workgroup and pass (matrices and accumulators in LDS): 256 per scene and pass
constexpr int LS_CHUNK_POINTS = 16384;   // point ranges per scene: ceil(N / 16 384) within [4, 64]
constexpr int LS_MIN_CHUNKS = 4;
constexpr int LS_MAX_CHUNKS = 64;
constexpr int LS_ACC = 8;            // per placement: back, finger, close, label min, label max, y max, y min, table verdict
constexpr int LS_HDR = 16;           // per frame: 12 floats of [R^T | -R^T p], the gate verdict, 3 unused
constexpr float LS_FIX = 1073741824.0f;  // 2^30: |n.y| terms are summed as integers of this scale, clamped to 4

struct LsParams {
  float fl, bl, hht, hbw, hbs, margin;                     // the gripper box (GripperBox order)
  float back_thr, fing_thr, min_points, nd;                // thresholds and NEIGHBOR_DEPTH
  float table_height, table_limit, slab_thr;               // TABLE_HEIGHT, TABLE_HEIGHT + TABLE_COLLISION_OFFSET, NUM_POINTS_THRESHOLD
  float r2lim;                                             // the cull radius squared, with slack for the fp32 roll
  int L, T, no_label;
};

// device table layout (floats): dl[L], slab lower bound[L], slab upper bound[L], cos[T], sin[T]
struct LsTables {
  float dl[LS_MAX_L], lo[LS_MAX_L], hi[LS_MAX_L], cs[LS_MAX_T], sn[LS_MAX_T];
};

__device__ __forceinline__ void ls_load_tables(const float* __restrict__ tables, int L, int T, LsTables* s, int t) {
  if (t < L) { s->dl[t] = tables[t]; s->lo[t] = tables[L + t]; s->hi[t] = tables[2 * L + t]; }
  if (t < T) { s->cs[t] = tables[3 * L + t]; s->sn[t] = tables[3 * L + T + t]; }
}

// does the placement reach the score?  the skips of :273,288,302,313,323,328 in the reference's order
__device__ __forceinline__ bool ls_gate(const int* __restrict__ a, int slab_n, const LsParams& p) {
  if (a[7]) return false;                                            // table (:288)
  if ((double)slab_n < (double)p.slab_thr) return false;             // too few points in the depth slab (:273)
  if ((double)a[0] > (double)p.back_thr) return false;               // :302
  if ((double)a[1] > (double)p.fing_thr) return false;               // :313
  if ((double)a[2] < (double)p.min_points || a[2] <= 0) return false;   // :323
  return a[3] == a[4];                                               // one label (:328)
}

__global__ __launch_bounds__(64) void ls_setup_kernel(
    const float* __restrict__ points, const float* __restrict__ frames, const float* __restrict__ tables, int F,
    LsParams p, const int64_t* __restrict__ frame_count, float* __restrict__ hdr, int* __restrict__ acc,
    int* __restrict__ slab, unsigned long long* __restrict__ bsum, int* __restrict__ bcnt) {
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
  if (__fdiv_rn(s, 9.0f) < 1e-6f) ok = false;                                        // :257
  if (__fadd_rn(pz, __fmul_rn(r[6], p.fl)) < p.table_height) ok = false;             // :259
  if (lane == 0) {
    float* h = hdr + row * LS_HDR;
#pragma unroll
    for (int i = 0; i < 3; ++i) {                                                    // row i of R^T = column i of R
      const float a = r[i], bb = r[3 + i], c = r[6 + i];
      h[4 * i] = a; h[4 * i + 1] = bb; h[4 * i + 2] = c;
      h[4 * i + 3] = -__fadd_rn(__fadd_rn(__fmul_rn(a, px), __fmul_rn(bb, py)), __fmul_rn(c, pz));
    }
    ((int*)h)[12] = ok ? 1 : 0;
    h[13] = h[14] = h[15] = 0.f;
  }
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
      hit = hit || (m0 * cx + m1 * cy + m2 * cz + m3 < p.table_limit);               // :240
    }
    int* a = acc + (row * P + pl) * LS_ACC;
#pragma unroll
    for (int w = 0; w < ACC_WORDS; ++w) a[w] = acc_neutral(w);
    a[7] = (ok && hit) ? 1 : 0;
    bsum[(row * P + pl) * 2] = bsum[(row * P + pl) * 2 + 1] = 0ull;
    bcnt[(row * P + pl) * 2] = bcnt[(row * P + pl) * 2 + 1] = 0;
  }
  if (lane < p.L) slab[row * p.L + lane] = 0;
}

__global__ __launch_bounds__(256) void ls_scan_kernel(
    const float* __restrict__ xyz, const int* __restrict__ labels, const float* __restrict__ hdr,
    const float* __restrict__ tables, int N, int F, LsParams p, int* __restrict__ slab, int* __restrict__ acc,
    const int64_t* __restrict__ frame_count) {
  __shared__ float gl[LS_SLOTS][12];
  __shared__ int live[LS_SLOTS];
  __shared__ int scnt[LS_SLOTS][LS_MAX_L];
  __shared__ unsigned opn[LS_SLOTS][LS_MAX_L];      // per depth, the rolls whose table verdict lets the placement through
  __shared__ int cnt[LS_SLOTS][LS_MAX_P][LS_ACC];
  __shared__ LsTables tb;
  const int b = blockIdx.z, t = threadIdx.x, lane = t & 63;
  const int L = p.L, T = p.T, P = L * T;
  const float* px = xyz + (size_t)b * 3 * N;
  const int* lab = labels + (size_t)b * N;
  const ChunkRange rg = chunk_range(N);
  if (rg.empty()) return;
  ls_load_tables(tables, L, T, &tb, t);
  const int fmax = frame_rows(frame_count, b, F);
  for (int j0 = 0; blockIdx.x + LS_GX * j0 < fmax; j0 += LS_SLOTS) {
    __syncthreads();                                  // (the previous pass's accumulators have been flushed)
    const int nslot = pass_slots(fmax, LS_GX, j0, LS_SLOTS);
    if (t < nslot) {
      const float* h = hdr + ((size_t)b * F + blockIdx.x + LS_GX * (j0 + t)) * LS_HDR;
#pragma unroll
      for (int c = 0; c < 12; ++c) gl[t][c] = h[c];
      live[t] = ((const int*)h)[12];
    }
    for (int i = t; i < nslot * LS_MAX_L; i += 256) ((int*)scnt)[i] = 0;
    if (t < nslot * L) {
      const int sl = t / L, d = t % L;
      const int* a = acc + (((size_t)b * F + blockIdx.x + LS_GX * (j0 + sl)) * P + d * T) * LS_ACC;
      unsigned mask = 0;
      for (int r = 0; r < T; ++r) mask |= (a[r * LS_ACC + 7] ? 0u : 1u) << r;      // (ls_setup_kernel wrote it; no scan changes it)
      opn[sl][d] = mask;
    }
    for (int i = t; i < nslot * P * LS_ACC; i += 256) {
      ((int*)cnt[i / (P * LS_ACC)])[i % (P * LS_ACC)] = acc_neutral(i & (LS_ACC - 1));
    }
    __syncthreads();
    for (int i0 = rg.lo + t; i0 < sweep_end<LS_U>(rg.hi); i0 += 256 * LS_U) {
      PointBlock<LS_U> pt;
      pt.load(px, N, i0, rg.hi);
      for (int sl = 0; sl < nslot; ++sl) {
        if (!live[sl]) continue;                      // a frame that failed a gate: never scanned (workgroup-uniform)
        float g[12];
#pragma unroll
        for (int c = 0; c < 12; ++c) g[c] = gl[sl][c];
        float lx[LS_U], ly[LS_U], lz[LS_U];
        unsigned m[LS_U];
#pragma unroll
        for (int u = 0; u < LS_U; ++u) {
          const LocalPoint l = local_point(g, pt.x[u], pt.y[u], pt.z[u]);
          lx[u] = l.x; ly[u] = l.y; lz[u] = l.z;
          m[u] = 0;
        }
        for (int d = 0; d < L; ++d) {                 // the depth slabs (:270-271): wave-uniform counts
          const float lo = tb.lo[d], hi = tb.hi[d];
          int n = 0;
#pragma unroll
          for (int u = 0; u < LS_U; ++u) {
            const bool s = pt.in[u] && (lx[u] < hi) && (lx[u] > lo);
            n += __popcll(__ballot(s));
            m[u] |= (s ? 1u : 0u) << d;
          }
          if (lane == 0 && n) atomicAdd(&scnt[sl][d], n);
        }
#pragma unroll
        for (int u = 0; u < LS_U; ++u) {
          if (!m[u] || !(ly[u] * ly[u] + lz[u] * lz[u] < p.r2lim)) continue;          // the cull
          // a placement that collides with the table is skipped before anything is counted (:288): its counts stay 0
          unsigned rolls = 0;
          for (int d = 0; d < L; ++d) rolls |= ((m[u] >> d) & 1u) ? opn[sl][d] : 0u;
          if (!rolls) continue;
          const int lb = lab[pt.idx[u]];
          for (int r = 0; r < T; ++r) {
            if (!((rolls >> r) & 1u)) continue;
            float yy, zz;
            ls_roll(tb.cs[r], tb.sn[r], ly[u], lz[u], &yy, &zz);
            if (!((zz < p.hht) && (zz > -p.hht))) continue;                            // :294-295
            if (!((yy < p.hbw) && (yy > -p.hbw))) continue;                            // outside back, fingers and close region
            const bool closer = (yy < p.hbs) && (yy > -p.hbs);                         // :317-319
            const bool fing = (yy > p.hbs) || (yy < -p.hbs);                           // :306-312
            const int o = f2ord(yy);
            for (int d = 0; d < L; ++d) {
              if (!((m[u] >> d) & 1u) || !((opn[sl][d] >> r) & 1u)) continue;
              int* a = cnt[sl][d * T + r];
              if (lx[u] - tb.dl[d] < -p.margin) atomicAdd(a + 0, 1);                   // :297-300
              if (fing) atomicAdd(a + 1, 1);
              if (closer) {
                atomicAdd(a + 2, 1);
                atomicMin(a + 3, lb); atomicMax(a + 4, lb);
                atomicMax(a + 5, o); atomicMin(a + 6, o);
              }
            }
          }
        }
      }
    }
    __syncthreads();
    for (int i = t; i < nslot * L; i += 256) {
      const int sl = i / L, d = i % L, n = scnt[sl][d];
      if (n) atomicAdd(slab + ((size_t)b * F + blockIdx.x + LS_GX * (j0 + sl)) * L + d, n);
    }
    for (int i = t; i < nslot * P; i += 256) {
      const int sl = i / P, pl = i % P;
      const int* c = cnt[sl][pl];
      int* a = acc + (((size_t)b * F + blockIdx.x + LS_GX * (j0 + sl)) * P + pl) * LS_ACC;
      if (c[0]) atomicAdd(a + 0, c[0]);
      if (c[1]) atomicAdd(a + 1, c[1]);
      if (c[2]) {
        atomicAdd(a + 2, c[2]);
        atomicMin(a + 3, c[3]); atomicMax(a + 4, c[4]);
        atomicMax(a + 5, c[5]); atomicMin(a + 6, c[6]);
      }
    }
  }
}

// The second scan.  bsum (B, F, P, 2) uint64 = fixed-point sums of |n.y| under the left / right pad, bcnt (B, F, P, 2)
// their populations; both zeroed by ls_setup_kernel.  A placement that does not reach the score gets bounds no y satisfies.
__global__ __launch_bounds__(256) void ls_band_kernel(
    const float* __restrict__ xyz, const float* __restrict__ normals, const float* __restrict__ hdr,
    const float* __restrict__ tables, int N, int F, LsParams p, const int* __restrict__ slab,
    const int* __restrict__ acc, unsigned long long* __restrict__ bsum, int* __restrict__ bcnt,
    const int64_t* __restrict__ frame_count) {
  __shared__ float gl[LS_SLOTS][12];
  __shared__ int live[LS_SLOTS];
  __shared__ int anylive;
  __shared__ unsigned lmask[LS_SLOTS][LS_MAX_L];    // per depth, the rolls whose placement reached the score
  __shared__ float thr[LS_SLOTS][LS_MAX_P][2];
  __shared__ unsigned long long bs[LS_SLOTS][LS_MAX_P][2];
  __shared__ int bc[LS_SLOTS][LS_MAX_P][2];
  __shared__ LsTables tb;
  const int b = blockIdx.z, t = threadIdx.x;
  const int L = p.L, T = p.T, P = L * T;
  const float* px = xyz + (size_t)b * 3 * N;
  const float* pn = normals + (size_t)b * 3 * N;
  const ChunkRange rg = chunk_range(N);
  if (rg.empty()) return;
  ls_load_tables(tables, L, T, &tb, t);
  const int fmax = frame_rows(frame_count, b, F);
  for (int j0 = 0; blockIdx.x + LS_GX * j0 < fmax; j0 += LS_SLOTS) {
    __syncthreads();
    const int nslot = pass_slots(fmax, LS_GX, j0, LS_SLOTS);
    if (t < nslot) {
      const float* h = hdr + ((size_t)b * F + blockIdx.x + LS_GX * (j0 + t)) * LS_HDR;
#pragma unroll
      for (int c = 0; c < 12; ++c) gl[t][c] = h[c];
      live[t] = 0;
    }
    if (t < LS_SLOTS * LS_MAX_L) ((unsigned*)lmask)[t] = 0u;
    if (t == 0) anylive = 0;
    __syncthreads();
    for (int i = t; i < nslot * P; i += 256) {
      const int sl = i / P, pl = i % P;
      const size_t row = (size_t)b * F + blockIdx.x + LS_GX * (j0 + sl);
      const int* a = acc + (row * P + pl) * LS_ACC;
      float lthr = __int_as_float(0x7f800000), rthr = __int_as_float(0xff800000);     // +inf, -inf: an empty band
      if (((const int*)(hdr + row * LS_HDR))[12] && ls_gate(a, slab[row * L + pl / T], p)) {
        const float left_y = ord2f(a[5]), right_y = ord2f(a[6]);                          // :167-168
        const float depth = fminf(__fdiv_rn(__fsub_rn(left_y, right_y), 3.0f), p.nd);           // :169
        lthr = __fsub_rn(left_y, depth);                                                        // :171
        rthr = __fadd_rn(right_y, depth);                                                       // :172
        live[sl] = 1;
        anylive = 1;
        atomicOr(&lmask[sl][pl / T], 1u << (pl % T));
      }
      thr[sl][pl][0] = lthr; thr[sl][pl][1] = rthr;
      bs[sl][pl][0] = bs[sl][pl][1] = 0ull;
      bc[sl][pl][0] = bc[sl][pl][1] = 0;
    }
    __syncthreads();
    if (!anylive) continue;                           // workgroup-uniform: no cloud read for this pass
    for (int i0 = rg.lo + t; i0 < sweep_end<LS_U>(rg.hi); i0 += 256 * LS_U) {
      PointBlock<LS_U> pt;
      pt.load(px, N, i0, rg.hi);
      for (int sl = 0; sl < nslot; ++sl) {
        if (!live[sl]) continue;
        float g[12];
#pragma unroll
        for (int c = 0; c < 12; ++c) g[c] = gl[sl][c];
#pragma unroll
        for (int u = 0; u < LS_U; ++u) {
          if (!pt.in[u]) continue;
          const LocalPoint l = local_point(g, pt.x[u], pt.y[u], pt.z[u]);
          const float lx = l.x, ly = l.y, lz = l.z;
          unsigned m = 0;
          for (int d = 0; d < L; ++d) m |= (((lx < tb.hi[d]) && (lx > tb.lo[d])) ? 1u : 0u) << d;
          if (!m || !(ly * ly + lz * lz < p.r2lim)) continue;
          unsigned rolls = 0;
          for (int d = 0; d < L; ++d) rolls |= ((m >> d) & 1u) ? lmask[sl][d] : 0u;
          if (!rolls) continue;                       // no placement of this point's slabs reached the score
          // the normal in the frame: rows 1 and 2 of R^T (:267); the roll below gives its y in the placement (:339-341)
          const float nx = pn[pt.idx[u]], ny = pn[(size_t)N + pt.idx[u]], nz = pn[2 * (size_t)N + pt.idx[u]];
          const float ny_l = g[4] * nx + g[5] * ny + g[6] * nz;
          const float nz_l = g[8] * nx + g[9] * ny + g[10] * nz;
          for (int r = 0; r < T; ++r) {
            if (!((rolls >> r) & 1u)) continue;
            float yy, zz;
            ls_roll(tb.cs[r], tb.sn[r], ly, lz, &yy, &zz);
            if (!((zz < p.hht) && (zz > -p.hht) && (yy < p.hbs) && (yy > -p.hbs))) continue;   // the close region
            // |n.y| as an integer of scale 2^30; fminf also turns a NaN into the clamp: no undefined conversion
            const unsigned long long q =
                (unsigned long long)__float2ll_rn(fminf(fabsf(tb.cs[r] * ny_l + tb.sn[r] * nz_l), 4.0f) * LS_FIX);
            for (int d = 0; d < L; ++d) {
              if (!((m >> d) & 1u)) continue;
              const int pl = d * T + r;
              if (yy > thr[sl][pl][0]) { atomicAdd(&bs[sl][pl][0], q); atomicAdd(&bc[sl][pl][0], 1); }   // :171
              if (yy < thr[sl][pl][1]) { atomicAdd(&bs[sl][pl][1], q); atomicAdd(&bc[sl][pl][1], 1); }   // :172
            }
          }
        }
      }
    }
    __syncthreads();
    for (int i = t; i < nslot * P * 2; i += 256) {
      const int sl = i / (2 * P), e = i % (2 * P);
      const int n = ((const int*)bc[sl])[e];
      if (n) {
        const size_t o = ((size_t)b * F + blockIdx.x + LS_GX * (j0 + sl)) * P * 2 + e;
        atomicAdd(bsum + o, ((const unsigned long long*)bs[sl])[e]);
        atomicAdd(bcnt + o, n);
      }
    }
  }
}

// one workgroup per frame, one thread per placement
__global__ __launch_bounds__(LS_MAX_P) void ls_finish_kernel(
    const float* __restrict__ hdr, const int* __restrict__ slab, const int* __restrict__ acc,
    const unsigned long long* __restrict__ bsum, const int* __restrict__ bcnt, int F, LsParams p,
    int* __restrict__ ints, float* __restrict__ scores, int* __restrict__ slab_out, int* __restrict__ valid) {
  const int b = blockIdx.y, f = blockIdx.x, pl = threadIdx.x;
  const int L = p.L, T = p.T, P = L * T;
  const size_t row = (size_t)b * F + f;
  const bool ok = ((const int*)(hdr + row * LS_HDR))[12] != 0;      // (0 for padding rows: ls_setup_kernel)
  int keep = 0;
  if (pl < P) {
    int vi[6] = {0, p.no_label, 0, 0, 0, 0};
    float score = 0.f;
    if (ok) {
      const int* a = acc + (row * P + pl) * LS_ACC;
      vi[2] = a[0]; vi[3] = a[1]; vi[4] = a[2]; vi[5] = a[7];
      if (ls_gate(a, slab[row * L + pl / T], p)) {
        vi[0] = a[2];                                                 // :332-333
        vi[1] = a[3];                                                 // :334-336
        const size_t o = (row * P + pl) * 2;
        // torch.mean (:176): an empty band gives NaN there, in the pose grading and here
        const float ml = (float)((double)bsum[o] * (1.0 / (double)LS_FIX) / (double)bcnt[o]);
        const float mr = (float)((double)bsum[o + 1] * (1.0 / (double)LS_FIX) / (double)bcnt[o + 1]);
        score = __fmul_rn(ml, mr);
      }
      keep = !(score < 1e-4f);                                        // :348: the maximum is not below 1e-4
    }
    int* oi = ints + (row * P + pl) * 6;
#pragma unroll
    for (int c = 0; c < 6; ++c) oi[c] = vi[c];
    scores[row * P + pl] = score;
  }
  if (pl < L) slab_out[row * L + pl] = ok ? slab[row * L + pl] : 0;
  const int any = __syncthreads_or(keep);
  if (pl == 0) valid[row] = any ? 1 : 0;
}

struct LsLayout {
  size_t hdr, acc, slab, bsum, bcnt, total;           // byte offsets
};
static inline LsLayout ls_layout(size_t B, size_t F, size_t L, size_t T) {
  const size_t rows = B * F, P = L * T;
  LsLayout o;
  o.hdr = 0;
  o.acc = align256(rows * LS_HDR * sizeof(float));
  o.bsum = o.acc + align256(rows * P * LS_ACC * sizeof(int));
  o.bcnt = o.bsum + align256(rows * P * 2 * sizeof(unsigned long long));
  o.slab = o.bcnt + align256(rows * P * 2 * sizeof(int));
  o.total = o.slab + align256(rows * L * sizeof(int));
  return o;
}

}  // namespace s4g

extern "C" size_t s4g_local_search_workspace_bytes(int64_t B, int64_t N, int64_t F, int64_t L, int64_t T) {
  if (B <= 0 || N <= 0 || F <= 0 || L <= 0 || T <= 0 || L > s4g::LS_MAX_L || T > s4g::LS_MAX_T) return 0;
  return s4g::ls_layout((size_t)B, (size_t)F, (size_t)L, (size_t)T).total;
}

extern "C" int s4g_local_search_f32(const float* points_bf3, const float* frames_bf33, const float* xyz_b3n,
                                    const float* normals_b3n, const int32_t* labels_bn, int64_t B, int64_t N,
                                    int64_t F, int64_t L, int64_t T, const float* params13, int32_t no_label,
                                    const float* tables_3l2t, const int64_t* frame_count_b, int32_t* ints_bfp6,
                                    float* scores_bfp, int32_t* slab_bfl, int32_t* valid_bf, int32_t* valid_index_bf,
                                    int64_t* count_b, void* workspace, size_t workspace_bytes, s4g_stream_t stream) {
  using namespace s4g;
  if (B < 0 || N <= 0 || F < 0 || B > 65535 || F > 65535 || N >= (1ll << 30)) return S4G_EINVAL;
  if (L <= 0 || T <= 0 || L > LS_MAX_L || T > LS_MAX_T) return S4G_EINVAL;
  if (B * F * L * T > (1ll << 26)) return S4G_EINVAL;       // (the accumulators: 8 ints per placement, indexed in size_t)
  if (B == 0) return S4G_OK;
  if (!count_b) return S4G_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (F == 0) {
    hipError_t e = hipMemsetAsync(count_b, 0, (size_t)B * sizeof(int64_t), st);
    return e == hipSuccess ? S4G_OK : (int)e;
  }
  if (!points_bf3 || !frames_bf33 || !xyz_b3n || !normals_b3n || !labels_bn || !params13 || !tables_3l2t ||
      !ints_bfp6 || !scores_bfp || !slab_bfl || !valid_bf || !valid_index_bf)
    return S4G_EINVAL;
  if (!workspace || workspace_bytes < s4g_local_search_workspace_bytes(B, N, F, L, T)) return S4G_EWORKSPACE;
  LsParams p;
  p.fl = params13[0]; p.bl = params13[1]; p.hht = params13[2]; p.hbw = params13[3]; p.hbs = params13[4];
  p.margin = params13[5]; p.back_thr = params13[6]; p.fing_thr = params13[7]; p.min_points = params13[8];
  p.nd = params13[9]; p.table_height = params13[10]; p.table_limit = params13[11]; p.slab_thr = params13[12];
  // the roll's cos / sin are fp32 values of deg / 57.29578: c^2 + s^2 is 1 within 1e-6, the slack is 1e-4
  p.r2lim = (p.hbw * p.hbw + p.hht * p.hht) * 1.0001f;
  p.L = (int)L; p.T = (int)T; p.no_label = no_label;
  const LsLayout lay = ls_layout((size_t)B, (size_t)F, (size_t)L, (size_t)T);
  char* ws = (char*)workspace;
  float* hdr = (float*)(ws + lay.hdr);
  int* acc = (int*)(ws + lay.acc);
  unsigned long long* bsum = (unsigned long long*)(ws + lay.bsum);
  int* bcnt = (int*)(ws + lay.bcnt);
  int* slab = (int*)(ws + lay.slab);
  const dim3 per_frame((unsigned)F, (unsigned)B);
  hipLaunchKernelGGL(ls_setup_kernel, per_frame, dim3(64), 0, st, points_bf3, frames_bf33, tables_3l2t, (int)F, p,
                     frame_count_b, hdr, acc, slab, bsum, bcnt);
  S4G_LAUNCH_CHECK();
  const dim3 grid(LS_GX, (unsigned)sweep_chunks(N, LS_CHUNK_POINTS, LS_MIN_CHUNKS, LS_MAX_CHUNKS), (unsigned)B);
  hipLaunchKernelGGL(ls_scan_kernel, grid, dim3(256), 0, st, xyz_b3n, (const int*)labels_bn, (const float*)hdr,
                     tables_3l2t, (int)N, (int)F, p, slab, acc, frame_count_b);
  S4G_LAUNCH_CHECK();
  hipLaunchKernelGGL(ls_band_kernel, grid, dim3(256), 0, st, xyz_b3n, normals_b3n, (const float*)hdr, tables_3l2t,
                     (int)N, (int)F, p, (const int*)slab, (const int*)acc, bsum, bcnt, frame_count_b);
  S4G_LAUNCH_CHECK();
  hipLaunchKernelGGL(ls_finish_kernel, per_frame, dim3(LS_MAX_P), 0, st, (const float*)hdr, (const int*)slab,
                     (const int*)acc, (const unsigned long long*)bsum, (const int*)bcnt, (int)F, p, (int*)ints_bfp6,
                     scores_bfp, (int*)slab_bfl, (int*)valid_bf);
  S4G_LAUNCH_CHECK();
  hipLaunchKernelGGL(compact_valid_kernel<KeepNonZero>, dim3((unsigned)B), dim3(256), 0, st, (const int*)valid_bf, (int)F,
                     (int*)valid_index_bf, count_b);
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}
