// The cloud sweep of the placement searches that keep plain counts per placement: s4g_precomputed_search_f32 and
// s4g_precomputed_baseline_search_f32 (precomputed_view.hip) and s4g_eval_view_search_f32 (eval_data.hip) all compile
// `pv_scan` below, so the counts behind the palm / in the fingers / in the close region and the slab counters of the
// three are the same integers by construction.  What is here is what those files share and nothing else: the compiled
// maxima, the per-frame header layout, the parameter block, the tables, the sweep body and the workspace layout.  The
// tuning constants (workgroups per scene, points per lane, frames per pass) stay with their kernels and come in as
// template arguments; the setup and finish kernels differ per class and stay in their files.
#pragma once
#include "frame_sweep.h"

namespace s4g {

constexpr int PV_MAX_L = 8;          // compiled maxima of the depth and roll lists (those of local_search.hip)
constexpr int PV_MAX_T = 16;
constexpr int PV_MAX_P = PV_MAX_L * PV_MAX_T;
constexpr int PV_HDR = 16;           // per frame: 12 floats of [R^T | -R^T p], the gate verdict, "holds a mask bit", 2 unused
constexpr unsigned PV_DEPTH_MASKED = 1u << 31;   // in a depth's word: the depth holds a mask bit; bits 0..15 the open rolls

struct PvParams {
  float fl, bl, hht, hbw, hbs, margin;                     // the gripper box (GripperBox order)
  float back_thr, fing_thr, min_points;                    // thresholds
  float table_limit, slab_thr;                             // TABLE_HEIGHT + TABLE_COLLISION_OFFSET, NUM_POINTS_THRESHOLD
  float valid_search_min, valid_antipodal_min;             // :384-385
  float r2lim;                                             // the cull radius squared, with slack for the fp32 roll
  int L, T, no_label;
};

// device table layout (floats), that of s4g_local_search_f32: dl[L], slab lower bound[L], slab upper bound[L], cos[T], sin[T]
struct PvTables {
  float dl[PV_MAX_L], lo[PV_MAX_L], hi[PV_MAX_L], cs[PV_MAX_T], sn[PV_MAX_T];
};

__device__ __forceinline__ void pv_load_tables(const float* __restrict__ tables, int L, int T, PvTables* s, int t) {
  if (t < L) { s->dl[t] = tables[t]; s->lo[t] = tables[L + t]; s->hi[t] = tables[2 * L + t]; }
  if (t < T) { s->cs[t] = tables[3 * L + t]; s->sn[t] = tables[3 * L + T + t]; }
}

// The sweep, written once: LABELS = true is the view stage's five-word form (ACC = 5), LABELS = false the three-word
// form of the baseline classes (ACC = 3), which reads no label and does no atomicMin / atomicMax.  Everything else --
// the slab counters, the cull, the roll, every comparison -- is the same statement in both, so the counts of the two are
// the same integers.  grid (GX, chunks, B), 256 threads; U points per lane; SLOTS frames per workgroup and pass.
// hdr (B, F, PV_HDR): [R^T | -R^T p], word 13 = the frame is scanned.  words (B, F, L, 2): [0] the rolls of the depth
// that are graded, bit 31 = the depth's slab is counted.  slab (B, F, L) and acc (B, F, L * T, ACC) hold their neutral
// values when the sweep starts.
template <bool LABELS, int GX, int U, int SLOTS, int ACC>
__device__ __forceinline__ void pv_scan(
    const float* __restrict__ xyz, const int* __restrict__ labels, const float* __restrict__ hdr,
    const unsigned* __restrict__ words, const float* __restrict__ tables, int N, int F, const PvParams& p,
    int* __restrict__ slab, int* __restrict__ acc, const int64_t* __restrict__ frame_count) {
  __shared__ float gl[SLOTS][12];
  __shared__ int live[SLOTS];
  __shared__ int anylive;
  __shared__ int scnt[SLOTS][PV_MAX_L];
  __shared__ unsigned opn[SLOTS][PV_MAX_L];         // per depth, the rolls that are graded; bit 31: the slab is counted
  __shared__ int cnt[SLOTS][PV_MAX_P][ACC];
  __shared__ PvTables tb;
  const int b = blockIdx.z, t = threadIdx.x, lane = t & 63;
  const int L = p.L, T = p.T, P = L * T;
  const float* px = xyz + (size_t)b * 3 * N;
  const int* lab = LABELS ? labels + (size_t)b * N : nullptr;
  const ChunkRange rg = chunk_range(N);
  if (rg.empty()) return;
  pv_load_tables(tables, L, T, &tb, t);
  const int fmax = frame_rows(frame_count, b, F);
  for (int j0 = 0; blockIdx.x + GX * j0 < fmax; j0 += SLOTS) {
    __syncthreads();                                  // (the previous pass's accumulators have been flushed)
    const int nslot = pass_slots(fmax, GX, j0, SLOTS);
    if (t == 0) anylive = 0;
    __syncthreads();
    if (t < nslot) {
      const float* h = hdr + ((size_t)b * F + blockIdx.x + GX * (j0 + t)) * PV_HDR;
#pragma unroll
      for (int c = 0; c < 12; ++c) gl[t][c] = h[c];
      live[t] = ((const int*)h)[13];
      if (live[t]) anylive = 1;
    }
    for (int i = t; i < nslot * PV_MAX_L; i += 256) ((int*)scnt)[i] = 0;
    for (int i = t; i < nslot * L; i += 256) {
      const int sl = i / L, d = i % L;
      opn[sl][d] = words[(((size_t)b * F + blockIdx.x + GX * (j0 + sl)) * L + d) * 2];
    }
    for (int i = t; i < nslot * P * ACC; i += 256) {
      ((int*)cnt[i / (P * ACC)])[i % (P * ACC)] = acc_neutral((i % (P * ACC)) % ACC);
    }
    __syncthreads();
    if (!anylive) continue;                           // workgroup-uniform: no cloud read, nothing to flush
    for (int i0 = rg.lo + t; i0 < sweep_end<U>(rg.hi); i0 += 256 * U) {
      PointBlock<U> pt;
      pt.load(px, N, i0, rg.hi);
      for (int sl = 0; sl < nslot; ++sl) {
        if (!live[sl]) continue;                      // a frame that failed its gate or has no mask bit: never scanned
        float g[12];
#pragma unroll
        for (int c = 0; c < 12; ++c) g[c] = gl[sl][c];
        float lx[U], ly[U], lz[U];
        unsigned m[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const LocalPoint l = local_point(g, pt.x[u], pt.y[u], pt.z[u]);
          lx[u] = l.x; ly[u] = l.y; lz[u] = l.z;
          m[u] = 0;
        }
        for (int d = 0; d < L; ++d) {                 // the depth slabs (:309-310) that hold a mask bit (:305)
          if (!(opn[sl][d] & PV_DEPTH_MASKED)) continue;                               // (workgroup-uniform)
          const float lo = tb.lo[d], hi = tb.hi[d];
          int n = 0;
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const bool s = pt.in[u] && (lx[u] < hi) && (lx[u] > lo);
            n += __popcll(__ballot(s));
            m[u] |= (s ? 1u : 0u) << d;
          }
          if (lane == 0 && n) atomicAdd(&scnt[sl][d], n);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (!m[u] || !(ly[u] * ly[u] + lz[u] * lz[u] < p.r2lim)) continue;          // the cull
          unsigned rolls = 0;
          for (int d = 0; d < L; ++d) rolls |= ((m[u] >> d) & 1u) ? (opn[sl][d] & 0xffffu) : 0u;
          if (!rolls) continue;
          int lb = 0;
          if constexpr (LABELS) lb = lab[pt.idx[u]];
          for (int r = 0; r < T; ++r) {
            if (!((rolls >> r) & 1u)) continue;
            float yy, zz;
            ls_roll(tb.cs[r], tb.sn[r], ly[u], lz[u], &yy, &zz);
            if (!((zz < p.hht) && (zz > -p.hht))) continue;                            // :334-335
            if (!((yy < p.hbw) && (yy > -p.hbw))) continue;                            // outside back, fingers and close region
            const bool closer = (yy < p.hbs) && (yy > -p.hbs);                         // :357-359
            const bool fing = (yy > p.hbs) || (yy < -p.hbs);                           // :346-352
            for (int d = 0; d < L; ++d) {
              if (!((m[u] >> d) & 1u) || !((opn[sl][d] >> r) & 1u)) continue;
              int* a = cnt[sl][d * T + r];
              if (lx[u] - tb.dl[d] < -p.margin) atomicAdd(a + 0, 1);                   // :337-340
              if (fing) atomicAdd(a + 1, 1);
              if (closer) {
                atomicAdd(a + 2, 1);
                if constexpr (LABELS) { atomicMin(a + 3, lb); atomicMax(a + 4, lb); }
              }
            }
          }
        }
      }
    }
    __syncthreads();
    for (int i = t; i < nslot * L; i += 256) {
      const int sl = i / L, d = i % L, n = scnt[sl][d];
      if (n) atomicAdd(slab + ((size_t)b * F + blockIdx.x + GX * (j0 + sl)) * L + d, n);
    }
    for (int i = t; i < nslot * P; i += 256) {
      const int sl = i / P, pl = i % P;
      const int* c = cnt[sl][pl];
      int* a = acc + (((size_t)b * F + blockIdx.x + GX * (j0 + sl)) * P + pl) * ACC;
      if (c[0]) atomicAdd(a + 0, c[0]);
      if (c[1]) atomicAdd(a + 1, c[1]);
      if (c[2]) {
        atomicAdd(a + 2, c[2]);
        if constexpr (LABELS) { atomicMin(a + 3, c[3]); atomicMax(a + 4, c[4]); }
      }
    }
  }
}

struct PvLayout {
  size_t hdr, acc, slab, words, total;                // byte offsets
};
static inline PvLayout pv_layout(size_t B, size_t F, size_t L, size_t T, size_t acc_words) {
  const size_t rows = B * F, P = L * T;
  PvLayout o;
  o.hdr = 0;
  o.acc = align256(rows * PV_HDR * sizeof(float));
  o.slab = o.acc + align256(rows * P * acc_words * sizeof(int));
  o.words = o.slab + align256(rows * L * sizeof(int));
  o.total = o.words + align256(rows * L * 2 * sizeof(unsigned));
  return o;
}

}  // namespace s4g
