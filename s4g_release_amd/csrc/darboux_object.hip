// Per-object grading of Darboux frames: GenerateDarbouxObjectData._estimate_grasp_quality with finger_hand_view and
// _antipodal_score (data_gen/data_generator/data_object_darboux_generator.py:94-247), which grades every point's frame
// and its opposite frame against the object's own cloud in a Python loop -- L depths x T rolls x S shifts of the hand
// along its thickness per frame (4 x 12 x 3 as shipped) -- as four launches over all frames of all objects, with no
// host synchronisation.  Contract: include/s4g_ops.h (s4g_darboux_object_grade_f32).  The frames themselves come from
// darboux_object_frames_kernel (darboux.hip), which shares the ordered grid of the view frames.
//
// A ROW is one (frame, direction): row = 2 * f + dir, dir 0 = `frame`, dir 1 = `inv_frame`.  Both matrices are read as
// given, so the call also grades frames that are not each other's opposite.  The placements of a row share the local x
// axis, so an object point is transformed ONCE per row; the roll keeps y^2 + z^2, and the S shifts differ in the z
// window only, so a point outside the cylinder y^2 + z^2 < HBW^2 + (HHT + max|dz|)^2 or outside every depth slab is
// outside every region of every placement and shift and only counts for the slab counters; one rolled point feeds the
// accumulators of all shifts.
//
//   do_setup_kernel    per row: the frame gate (:136), [R^T | -R^T p] as ls_setup_kernel forms it, the neutral values of
//                      the row's accumulators (no memset: every launch of the call is a kernel)
//   do_scan_kernel     first scan, a cloud sweep (frame_sweep.h: points outer, rows inner): the slab counters (:150-153)
//                      and per (placement, shift) the counts behind the palm / in the fingers / in the close region and
//                      the ordered-integer y extrema of the close region; in LDS, then the workspace (integer atomics)
//   do_band_kernel     second scan, only for the (placement, shift) cells that passed their three gates: sum |n.y| over
//                      the two bands (:235-244) in 2^-30 fixed point with INTEGER atomics
//   do_finish_kernel   the gates per shift and the fold over the shifts in the reference's order (:179-218)
#include "frame_sweep.h"

namespace s4g {

constexpr int DO_MAX_L = 8;          // compiled maxima of the depth, roll and shift lists
constexpr int DO_MAX_T = 16;
constexpr int DO_MAX_S = 4;
constexpr int DO_MAX_P = DO_MAX_L * DO_MAX_T;
constexpr int DO_GX = 128;           // workgroups that share an object's rows (row k belongs to workgroup k mod 128): with 8
                                     // point ranges, 1 024 workgroups for one object (32 left three quarters of the CUs idle)
constexpr int DO_U = 4;              // points per lane held in registers while the workgroup's rows pass over them
constexpr int DO_SLOTS = 8;          // rows per workgroup and pass at most (fewer where the lists are long: do_slots)
constexpr int DO_CHUNK_POINTS = 1024;    // point ranges per object: ceil(N / 1 024) within [8, 64]
constexpr int DO_MIN_CHUNKS = 8;
constexpr int DO_MAX_CHUNKS = 64;
constexpr int DO_ACC = 5;            // per (placement, shift): back, finger, close, ordered y maximum, ordered y minimum
constexpr int DO_HDR = 16;           // per row: 12 floats of [R^T | -R^T p], the gate verdict, 3 unused
constexpr int DO_LDS_BYTES = 48 * 1024;  // dynamic LDS of a scan: a third of the 160 KB of a CU, three workgroups each
constexpr float DO_FIX = 1073741824.0f;  // 2^30: |n.y| terms are summed as integers of this scale, clamped to 4

struct DoParams {
  float hbw, hbs, margin;                                  // HALF_BOTTOM_WIDTH, HALF_BOTTOM_SPACE, BACK_COLLISION_MARGIN
  float back_thr, fing_thr, min_points, nd, slab_thr;      // thresholds and NEIGHBOR_DEPTH
  float r2lim;                                             // the cull radius squared, with slack for the fp32 roll
  int L, T, S, slots;
};

// device table layout (floats): dl[L], slab lower bound[L], slab upper bound[L], cos[T], sin[T], z lower[S], z upper[S]
struct DoTables {
  float dl[DO_MAX_L], lo[DO_MAX_L], hi[DO_MAX_L], cs[DO_MAX_T], sn[DO_MAX_T], zlo[DO_MAX_S], zhi[DO_MAX_S];
};

__device__ __forceinline__ void do_load_tables(const float* __restrict__ tables, int L, int T, int S, DoTables* s, int t) {
  if (t < L) { s->dl[t] = tables[t]; s->lo[t] = tables[L + t]; s->hi[t] = tables[2 * L + t]; }
  if (t < T) { s->cs[t] = tables[3 * L + t]; s->sn[t] = tables[3 * L + T + t]; }
  if (t < S) { s->zlo[t] = tables[3 * L + 2 * T + t]; s->zhi[t] = tables[3 * L + 2 * T + S + t]; }
}

__device__ __forceinline__ int do_acc_neutral(int w) { return w == 3 ? INT_MIN : w == 4 ? INT_MAX : 0; }

// does the shift reach the score?  the skips of :188,193,201 in the reference's order (the slab skip of :153 first)
__device__ __forceinline__ bool do_gate(const int* __restrict__ a, int slab_n, const DoParams& p) {
  if ((double)slab_n < (double)p.slab_thr) return false;
  if ((double)a[0] > (double)p.back_thr) return false;
  if ((double)a[1] > (double)p.fing_thr) return false;
  return !((double)a[2] < (double)p.min_points) && a[2] > 0;
}

// the roll of LOCAL_TO_LOCAL_SEARCH (configs/config.py:79-82): both scans call this, so they see the same y bit for bit
__device__ __forceinline__ void do_roll(float c, float s, float y, float z, float* yy, float* zz) {
  *yy = c * y + s * z;
  *zz = (-s) * y + c * z;
}

// the points of object b: the first count[b] of N
__device__ __forceinline__ int do_points(const int64_t* __restrict__ count, int b, int N) { return frame_rows(count, b, N); }

__global__ __launch_bounds__(64) void do_setup_kernel(
    const float* __restrict__ xyz, const float* __restrict__ frames, const float* __restrict__ inv_frames,
    const int32_t* __restrict__ frame_index, const int64_t* __restrict__ count, int N, int F, DoParams p,
    float* __restrict__ hdr, int* __restrict__ acc, int* __restrict__ slab, unsigned long long* __restrict__ bsum,
    int* __restrict__ bcnt) {
  const int b = blockIdx.y, k = blockIdx.x, f = k >> 1, dir = k & 1, lane = threadIdx.x;
  const size_t row = (size_t)b * 2 * F + k;
  const float* __restrict__ src = (dir ? inv_frames : frames) + ((size_t)b * F + f) * 9;
  float r[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) r[i] = src[i];
  const int nb = do_points(count, b, N);
  const int idx = frame_index ? frame_index[(size_t)b * F + f] : f;
  bool ok = idx >= 0 && idx < nb;
  const int ic = ok ? idx : 0;
  const float* __restrict__ p0 = xyz + (size_t)b * 3 * N;
  const float px = p0[ic], py = p0[(size_t)N + ic], pz = p0[2 * (size_t)N + ic];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 9; ++i) s = s + fabsf(r[i]);
  if (!(__fdiv_rn(s, 9.0f) >= 1e-6f) || !(s < 3.0e38f)) ok = false;                  // :136; not finite: decision 2
  if (!(fabsf(px) < 3.0e38f && fabsf(py) < 3.0e38f && fabsf(pz) < 3.0e38f)) ok = false;
  if (lane == 0) {
    float* h = hdr + row * DO_HDR;
#pragma unroll
    for (int i = 0; i < 3; ++i) {                                                    // row i of R^T = column i of R
      const float a = r[i], bb = r[3 + i], c = r[6 + i];
      h[4 * i] = a; h[4 * i + 1] = bb; h[4 * i + 2] = c;
      h[4 * i + 3] = -__fadd_rn(__fadd_rn(__fmul_rn(a, px), __fmul_rn(bb, py)), __fmul_rn(c, pz));
    }
    ((int*)h)[12] = ok ? 1 : 0;
    h[13] = h[14] = h[15] = 0.f;
  }
  const int C = p.L * p.T * p.S;
  for (int c = lane; c < C; c += 64) {
    int* a = acc + (row * C + c) * DO_ACC;
#pragma unroll
    for (int w = 0; w < DO_ACC; ++w) a[w] = do_acc_neutral(w);
    bsum[(row * C + c) * 2] = bsum[(row * C + c) * 2 + 1] = 0ull;
    bcnt[(row * C + c) * 2] = bcnt[(row * C + c) * 2 + 1] = 0;
  }
  if (lane < p.L) slab[row * p.L + lane] = 0;
}

// the rows of object b that can be live: all 2 F of an index list, else those of its points
__device__ __forceinline__ int do_rows(const int32_t* __restrict__ frame_index, const int64_t* __restrict__ count, int b,
                                       int N, int F) {
  return frame_index ? 2 * F : 2 * min(F, do_points(count, b, N));
}

__global__ __launch_bounds__(256) void do_scan_kernel(
    const float* __restrict__ xyz, const float* __restrict__ hdr, const float* __restrict__ tables, int N, int F,
    DoParams p, int* __restrict__ slab, int* __restrict__ acc, const int32_t* __restrict__ frame_index,
    const int64_t* __restrict__ count) {
  extern __shared__ int do_cnt[];                   // [slots][P][S][DO_ACC]
  __shared__ float gl[DO_SLOTS][12];
  __shared__ int live[DO_SLOTS];
  __shared__ int scnt[DO_SLOTS][DO_MAX_L];
  __shared__ DoTables tb;
  const int b = blockIdx.z, t = threadIdx.x, lane = t & 63;
  const int L = p.L, T = p.T, S = p.S, C = L * T * S;
  const float* px = xyz + (size_t)b * 3 * N;
  const ChunkRange rg = chunk_range(do_points(count, b, N));
  if (rg.empty()) return;
  do_load_tables(tables, L, T, S, &tb, t);
  const int kmax = do_rows(frame_index, count, b, N, F);
  for (int j0 = 0; blockIdx.x + DO_GX * j0 < kmax; j0 += p.slots) {
    __syncthreads();                                  // (the previous pass's accumulators have been flushed)
    const int nslot = pass_slots(kmax, DO_GX, j0, p.slots);
    if (t < nslot) {
      const float* h = hdr + ((size_t)b * 2 * F + blockIdx.x + DO_GX * (j0 + t)) * DO_HDR;
#pragma unroll
      for (int c = 0; c < 12; ++c) gl[t][c] = h[c];
      live[t] = ((const int*)h)[12];
    }
    for (int i = t; i < nslot * DO_MAX_L; i += 256) ((int*)scnt)[i] = 0;
    for (int i = t; i < nslot * C * DO_ACC; i += 256) do_cnt[i] = do_acc_neutral(i % DO_ACC);
    __syncthreads();
    for (int i0 = rg.lo + t; i0 < sweep_end<DO_U>(rg.hi); i0 += 256 * DO_U) {
      PointBlock<DO_U> pt;
      pt.load(px, N, i0, rg.hi);
      for (int sl = 0; sl < nslot; ++sl) {
        if (!live[sl]) continue;                      // a row that failed the gate: never scanned (workgroup-uniform)
        float g[12];
#pragma unroll
        for (int c = 0; c < 12; ++c) g[c] = gl[sl][c];
        float lx[DO_U], ly[DO_U], lz[DO_U];
        unsigned m[DO_U];
#pragma unroll
        for (int u = 0; u < DO_U; ++u) {
          const LocalPoint l = local_point(g, pt.x[u], pt.y[u], pt.z[u]);
          lx[u] = l.x; ly[u] = l.y; lz[u] = l.z;
          m[u] = 0;
        }
        for (int d = 0; d < L; ++d) {                 // the depth slabs (:150-151): wave-uniform counts
          const float lo = tb.lo[d], hi = tb.hi[d];
          int n = 0;
#pragma unroll
          for (int u = 0; u < DO_U; ++u) {
            const bool s = pt.in[u] && (lx[u] < hi) && (lx[u] > lo);
            n += __popcll(__ballot(s));
            m[u] |= (s ? 1u : 0u) << d;
          }
          if (lane == 0 && n) atomicAdd(&scnt[sl][d], n);
        }
        int* base = do_cnt + sl * C * DO_ACC;
#pragma unroll
        for (int u = 0; u < DO_U; ++u) {
          if (!m[u] || !(ly[u] * ly[u] + lz[u] * lz[u] < p.r2lim)) continue;          // the cull
          for (int r = 0; r < T; ++r) {
            float yy, zz;
            do_roll(tb.cs[r], tb.sn[r], ly[u], lz[u], &yy, &zz);
            if (!((yy < p.hbw) && (yy > -p.hbw))) continue;                            // outside back, fingers and close region
            unsigned zs = 0;
            for (int s = 0; s < S; ++s) zs |= (((zz < tb.zhi[s]) && (zz > tb.zlo[s])) ? 1u : 0u) << s;   // :183-184
            if (!zs) continue;
            const bool closer = (yy < p.hbs) && (yy > -p.hbs);                         // :196-198
            const bool fing = (yy > p.hbs) || (yy < -p.hbs);                           // :173-176
            const int o = f2ord(yy);
            for (int d = 0; d < L; ++d) {
              if (!((m[u] >> d) & 1u)) continue;
              const bool back = lx[u] - tb.dl[d] < -p.margin;                          // :169-171
              for (int s = 0; s < S; ++s) {
                if (!((zs >> s) & 1u)) continue;
                int* a = base + (((d * T + r) * S) + s) * DO_ACC;
                if (back) atomicAdd(a + 0, 1);
                if (fing) atomicAdd(a + 1, 1);
                if (closer) {
                  atomicAdd(a + 2, 1);
                  atomicMax(a + 3, o); atomicMin(a + 4, o);
                }
              }
            }
          }
        }
      }
    }
    __syncthreads();
    for (int i = t; i < nslot * L; i += 256) {
      const int sl = i / L, d = i % L, n = scnt[sl][d];
      if (n) atomicAdd(slab + ((size_t)b * 2 * F + blockIdx.x + DO_GX * (j0 + sl)) * L + d, n);
    }
    for (int i = t; i < nslot * C; i += 256) {
      const int sl = i / C, c = i % C;
      const int* s = do_cnt + (size_t)i * DO_ACC;
      int* a = acc + (((size_t)b * 2 * F + blockIdx.x + DO_GX * (j0 + sl)) * C + c) * DO_ACC;
      if (s[0]) atomicAdd(a + 0, s[0]);
      if (s[1]) atomicAdd(a + 1, s[1]);
      if (s[2]) {
        atomicAdd(a + 2, s[2]);
        atomicMax(a + 3, s[3]); atomicMin(a + 4, s[4]);
      }
    }
  }
}

// The second scan.  bsum (rows, C, 2) uint64 = fixed-point sums of |n.y| under the left / right pad, bcnt (rows, C, 2)
// their populations; both zeroed by do_setup_kernel.  A cell that does not reach the score gets bounds no y satisfies.
// Dynamic LDS per slot: C x 2 uint64 sums, then C x 2 float bounds, then C x 2 int populations.
__global__ __launch_bounds__(256) void do_band_kernel(
    const float* __restrict__ xyz, const float* __restrict__ normals, const float* __restrict__ hdr,
    const float* __restrict__ tables, int N, int F, DoParams p, const int* __restrict__ slab,
    const int* __restrict__ acc, unsigned long long* __restrict__ bsum, int* __restrict__ bcnt,
    const int32_t* __restrict__ frame_index, const int64_t* __restrict__ count) {
  extern __shared__ unsigned long long do_band[];
  __shared__ float gl[DO_SLOTS][12];
  __shared__ int live[DO_SLOTS];
  __shared__ int anylive;
  __shared__ unsigned lmask[DO_SLOTS][DO_MAX_L][DO_MAX_S];   // per depth and shift, the rolls whose cell reached the score
  __shared__ DoTables tb;
  const int b = blockIdx.z, t = threadIdx.x;
  const int L = p.L, T = p.T, S = p.S, C = L * T * S;
  unsigned long long* bs = do_band;                                   // [slots][C][2]
  float* thr = (float*)(do_band + (size_t)p.slots * C * 2);           // [slots][C][2]
  int* bc = (int*)(thr + (size_t)p.slots * C * 2);                    // [slots][C][2]
  const float* px = xyz + (size_t)b * 3 * N;
  const float* pn = normals + (size_t)b * 3 * N;
  const ChunkRange rg = chunk_range(do_points(count, b, N));
  if (rg.empty()) return;
  do_load_tables(tables, L, T, S, &tb, t);
  const int kmax = do_rows(frame_index, count, b, N, F);
  for (int j0 = 0; blockIdx.x + DO_GX * j0 < kmax; j0 += p.slots) {
    __syncthreads();
    const int nslot = pass_slots(kmax, DO_GX, j0, p.slots);
    if (t < nslot) {
      const float* h = hdr + ((size_t)b * 2 * F + blockIdx.x + DO_GX * (j0 + t)) * DO_HDR;
#pragma unroll
      for (int c = 0; c < 12; ++c) gl[t][c] = h[c];
      live[t] = 0;
    }
    for (int i = t; i < DO_SLOTS * DO_MAX_L * DO_MAX_S; i += 256) ((unsigned*)lmask)[i] = 0u;
    if (t == 0) anylive = 0;
    __syncthreads();
    for (int i = t; i < nslot * C; i += 256) {
      const int sl = i / C, c = i % C, pl = c / S, s = c % S;
      const size_t row = (size_t)b * 2 * F + blockIdx.x + DO_GX * (j0 + sl);
      const int* a = acc + (row * C + c) * DO_ACC;
      float lthr = __int_as_float(0x7f800000), rthr = __int_as_float(0xff800000);     // +inf, -inf: an empty band
      if (((const int*)(hdr + row * DO_HDR))[12] && do_gate(a, slab[row * L + pl / T], p)) {
        const float left_y = ord2f(a[3]), right_y = ord2f(a[4]);                          // :235-236
        const float depth = fminf(__fdiv_rn(__fsub_rn(left_y, right_y), 3.0f), p.nd);     // :237
        lthr = __fsub_rn(left_y, depth);                                                  // :239
        rthr = __fadd_rn(right_y, depth);                                                 // :240
        live[sl] = 1;
        anylive = 1;
        atomicOr(&lmask[sl][pl / T][s], 1u << (pl % T));
      }
      thr[2 * i] = lthr; thr[2 * i + 1] = rthr;
      bs[2 * i] = bs[2 * i + 1] = 0ull;
      bc[2 * i] = bc[2 * i + 1] = 0;
    }
    __syncthreads();
    if (!anylive) continue;                           // workgroup-uniform: no cloud read for this pass
    for (int i0 = rg.lo + t; i0 < sweep_end<DO_U>(rg.hi); i0 += 256 * DO_U) {
      PointBlock<DO_U> pt;
      pt.load(px, N, i0, rg.hi);
      for (int sl = 0; sl < nslot; ++sl) {
        if (!live[sl]) continue;
        float g[12];
#pragma unroll
        for (int c = 0; c < 12; ++c) g[c] = gl[sl][c];
#pragma unroll
        for (int u = 0; u < DO_U; ++u) {
          if (!pt.in[u]) continue;
          const LocalPoint l = local_point(g, pt.x[u], pt.y[u], pt.z[u]);
          const float lx = l.x, ly = l.y, lz = l.z;
          unsigned m = 0;
          for (int d = 0; d < L; ++d) m |= (((lx < tb.hi[d]) && (lx > tb.lo[d])) ? 1u : 0u) << d;
          if (!m || !(ly * ly + lz * lz < p.r2lim)) continue;
          unsigned rolls = 0;
          for (int d = 0; d < L; ++d) {
            if (!((m >> d) & 1u)) continue;
            for (int s = 0; s < S; ++s) rolls |= lmask[sl][d][s];
          }
          if (!rolls) continue;                       // no cell of this point's slabs reached the score
          // the normal in the frame: rows 1 and 2 of R^T (:146); the roll below gives its y in the placement (:205-207)
          const float nx = pn[pt.idx[u]], ny = pn[(size_t)N + pt.idx[u]], nz = pn[2 * (size_t)N + pt.idx[u]];
          const float ny_l = g[4] * nx + g[5] * ny + g[6] * nz;
          const float nz_l = g[8] * nx + g[9] * ny + g[10] * nz;
          for (int r = 0; r < T; ++r) {
            if (!((rolls >> r) & 1u)) continue;
            float yy, zz;
            do_roll(tb.cs[r], tb.sn[r], ly, lz, &yy, &zz);
            if (!((yy < p.hbs) && (yy > -p.hbs))) continue;                                     // the close region's y
            unsigned zs = 0;
            for (int s = 0; s < S; ++s) zs |= (((zz < tb.zhi[s]) && (zz > tb.zlo[s])) ? 1u : 0u) << s;
            if (!zs) continue;
            // |n.y| as an integer of scale 2^30; fminf also turns a NaN into the clamp: no undefined conversion
            const unsigned long long q =
                (unsigned long long)__float2ll_rn(fminf(fabsf(tb.cs[r] * ny_l + tb.sn[r] * nz_l), 4.0f) * DO_FIX);
            for (int d = 0; d < L; ++d) {
              if (!((m >> d) & 1u)) continue;
              for (int s = 0; s < S; ++s) {
                if (!((zs >> s) & 1u) || !((lmask[sl][d][s] >> r) & 1u)) continue;
                const int e = 2 * ((sl * L * T + d * T + r) * S + s);
                if (yy > thr[e]) { atomicAdd(&bs[e], q); atomicAdd(&bc[e], 1); }                   // :239
                if (yy < thr[e + 1]) { atomicAdd(&bs[e + 1], q); atomicAdd(&bc[e + 1], 1); }       // :240
              }
            }
          }
        }
      }
    }
    __syncthreads();
    for (int i = t; i < nslot * C * 2; i += 256) {
      const int sl = i / (2 * C), e = i % (2 * C);
      const int n = bc[i];
      if (n) {
        const size_t o = ((size_t)b * 2 * F + blockIdx.x + DO_GX * (j0 + sl)) * C * 2 + e;
        atomicAdd(bsum + o, bs[i]);
        atomicAdd(bcnt + o, n);
      }
    }
  }
}

// one workgroup per row, one thread per placement: the fold over the shifts (:179-218)
__global__ __launch_bounds__(DO_MAX_P) void do_finish_kernel(
    const float* __restrict__ hdr, const int* __restrict__ slab, const int* __restrict__ acc,
    const unsigned long long* __restrict__ bsum, const int* __restrict__ bcnt, int F, DoParams p,
    int* __restrict__ search, float* __restrict__ antipodal, int* __restrict__ counts, int* __restrict__ slab_out,
    int* __restrict__ fail) {
  const int b = blockIdx.y, k = blockIdx.x, pl = threadIdx.x;
  const int L = p.L, T = p.T, S = p.S, P = L * T, C = P * S;
  const size_t row = (size_t)b * 2 * F + k;
  const bool ok = ((const int*)(hdr + row * DO_HDR))[12] != 0;      // (0 for padding rows: do_setup_kernel)
  if (pl < P) {
    float temp_search = 0.f, temp_antipodal = 0.f, close_num = 0.f, single = 0.f;          // :179-180, decision 1
    const int slab_n = slab[row * L + pl / T];
    for (int s = 0; s < S; ++s) {
      const int* a = acc + (row * C + pl * S + s) * DO_ACC;
      int* c = counts + (row * C + pl * S + s) * 3;
      c[0] = ok ? a[0] : 0; c[1] = ok ? a[1] : 0; c[2] = ok ? a[2] : 0;
      if (!ok || (double)slab_n < (double)p.slab_thr) continue;                              // :136, :153
      if ((double)a[0] > (double)p.back_thr) continue;                                       // :188
      if ((double)a[1] > (double)p.fing_thr) continue;                                       // :193
      close_num = (float)a[2];                                                               // :200
      if (close_num < p.min_points || a[2] <= 0) continue;                                   // :201
      const size_t o = (row * C + pl * S + s) * 2;
      // torch.mean (:246): an empty band gives NaN there and here
      const float ml = (float)((double)bsum[o] * (1.0 / (double)DO_FIX) / (double)bcnt[o]);
      const float mr = (float)((double)bsum[o + 1] * (1.0 / (double)DO_FIX) / (double)bcnt[o + 1]);
      single = __fmul_rn(ml, mr);                                                            // :211
      temp_antipodal = __fadd_rn(temp_antipodal, __fdiv_rn(single, 3.0f));                   // :212
      temp_search = __fadd_rn(temp_search, __fdiv_rn(close_num, 3.0f));                      // :213
    }
    // torch.min (:215-218) propagates NaN; the int tensor of :104-105 truncates
    search[row * P + pl] = (int)fminf(temp_search, close_num);
    antipodal[row * P + pl] = (temp_antipodal != temp_antipodal || single != single) ? __int_as_float(0x7fc00000)
                                                                                      : fminf(temp_antipodal, single);
  }
  if (pl < L) slab_out[row * L + pl] = ok ? slab[row * L + pl] : 0;
  if (pl == 0) fail[row] = ok ? 0 : 1;
}

struct DoLayout {
  size_t hdr, acc, slab, bsum, bcnt, total;           // byte offsets
};
static inline DoLayout do_layout(size_t B, size_t F, size_t L, size_t T, size_t S) {
  const size_t rows = B * F * 2, C = L * T * S;
  DoLayout o;
  o.hdr = 0;
  o.bsum = align256(rows * DO_HDR * sizeof(float));
  o.acc = o.bsum + align256(rows * C * 2 * sizeof(unsigned long long));
  o.bcnt = o.acc + align256(rows * C * DO_ACC * sizeof(int));
  o.slab = o.bcnt + align256(rows * C * 2 * sizeof(int));
  o.total = o.slab + align256(rows * L * sizeof(int));
  return o;
}

// rows per workgroup and pass: what fits DO_LDS_BYTES of the larger of the two scans' per-row tables
static inline int do_slots(size_t L, size_t T, size_t S) {
  const size_t C = L * T * S;
  const size_t per_row = C * (2 * sizeof(unsigned long long) + 2 * sizeof(float) + 2 * sizeof(int));   // 32 C >= 20 C
  size_t s = DO_LDS_BYTES / per_row;
  return (int)(s < 1 ? 1 : s > DO_SLOTS ? DO_SLOTS : s);
}

}  // namespace s4g

extern "C" size_t s4g_darboux_object_grade_workspace_bytes(int64_t B, int64_t N, int64_t F, int64_t L, int64_t T,
                                                           int64_t S) {
  (void)N;
  if (B <= 0 || F <= 0 || L <= 0 || T <= 0 || S <= 0 || L > s4g::DO_MAX_L || T > s4g::DO_MAX_T || S > s4g::DO_MAX_S)
    return 0;
  return s4g::do_layout((size_t)B, (size_t)F, (size_t)L, (size_t)T, (size_t)S).total;
}

extern "C" int s4g_darboux_object_grade_f32(const float* xyz_b3n, const float* normals_b3n, const int64_t* count_b,
                                            const float* frames_bf33, const float* inv_frames_bf33,
                                            const int32_t* frame_index_bf, int64_t B, int64_t N, int64_t F, int64_t L,
                                            int64_t T, int64_t S, const float* params9, const float* tables_3l2t2s,
                                            int32_t* search_bf2lt, float* antipodal_bf2lt, int32_t* counts_bf2lts3,
                                            int32_t* slab_bf2l, int32_t* fail_bf2, void* workspace,
                                            size_t workspace_bytes, s4g_stream_t stream) {
  using namespace s4g;
  if (B < 0 || N <= 0 || F < 0 || B > 65535 || F >= (1ll << 30) || N >= (1ll << 30)) return S4G_EINVAL;
  if (L <= 0 || T <= 0 || S <= 0 || L > DO_MAX_L || T > DO_MAX_T || S > DO_MAX_S) return S4G_EINVAL;
  if (B * F * 2 * L * T * S > (1ll << 27)) return S4G_EINVAL;   // (the accumulators, indexed in size_t; 2 F fits a grid)
  if (B == 0 || F == 0) return S4G_OK;
  if (!xyz_b3n || !normals_b3n || !frames_bf33 || !inv_frames_bf33 || !params9 || !tables_3l2t2s || !search_bf2lt ||
      !antipodal_bf2lt || !counts_bf2lts3 || !slab_bf2l || !fail_bf2)
    return S4G_EINVAL;
  if (!workspace || workspace_bytes < s4g_darboux_object_grade_workspace_bytes(B, N, F, L, T, S)) return S4G_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  DoParams p;
  p.hbw = params9[0]; p.hbs = params9[1]; p.margin = params9[2]; p.back_thr = params9[3]; p.fing_thr = params9[4];
  p.min_points = params9[5]; p.nd = params9[6]; p.slab_thr = params9[7];
  // params9[8] = HALF_HAND_THICKNESS + max |dz|.  The roll's cos / sin are fp32 values of deg / 57.29578: c^2 + s^2 is
  // 1 within 1e-6, the slack is 1e-4
  p.r2lim = (p.hbw * p.hbw + params9[8] * params9[8]) * 1.0001f;
  p.L = (int)L; p.T = (int)T; p.S = (int)S; p.slots = do_slots((size_t)L, (size_t)T, (size_t)S);
  const DoLayout lay = do_layout((size_t)B, (size_t)F, (size_t)L, (size_t)T, (size_t)S);
  char* ws = (char*)workspace;
  float* hdr = (float*)(ws + lay.hdr);
  int* acc = (int*)(ws + lay.acc);
  unsigned long long* bsum = (unsigned long long*)(ws + lay.bsum);
  int* bcnt = (int*)(ws + lay.bcnt);
  int* slab = (int*)(ws + lay.slab);
  const size_t C = (size_t)(L * T * S);
  const dim3 per_row((unsigned)(2 * F), (unsigned)B);
  hipLaunchKernelGGL(do_setup_kernel, per_row, dim3(64), 0, st, xyz_b3n, frames_bf33, inv_frames_bf33, frame_index_bf,
                     count_b, (int)N, (int)F, p, hdr, acc, slab, bsum, bcnt);
  S4G_LAUNCH_CHECK();
  const dim3 grid(DO_GX, (unsigned)sweep_chunks(N, DO_CHUNK_POINTS, DO_MIN_CHUNKS, DO_MAX_CHUNKS), (unsigned)B);
  hipLaunchKernelGGL(do_scan_kernel, grid, dim3(256), (size_t)p.slots * C * DO_ACC * sizeof(int), st, xyz_b3n,
                     (const float*)hdr, tables_3l2t2s, (int)N, (int)F, p, slab, acc, frame_index_bf, count_b);
  S4G_LAUNCH_CHECK();
  hipLaunchKernelGGL(do_band_kernel, grid, dim3(256), (size_t)p.slots * C * 32, st, xyz_b3n, normals_b3n,
                     (const float*)hdr, tables_3l2t2s, (int)N, (int)F, p, (const int*)slab, (const int*)acc, bsum, bcnt,
                     frame_index_bf, count_b);
  S4G_LAUNCH_CHECK();
  hipLaunchKernelGGL(do_finish_kernel, per_row, dim3(DO_MAX_P), 0, st, (const float*)hdr, (const int*)slab,
                     (const int*)acc, (const unsigned long long*)bsum, (const int*)bcnt, (int)F, p, search_bf2lt,
                     antipodal_bf2lt, counts_bf2lts3, slab_bf2l, fail_bf2);
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}
