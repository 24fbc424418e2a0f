// The refine and reduce stages of the contact-object pipeline: data_gen/utils/refine_contact_object.py:45-114 and
// data_gen/utils/smooth_contact_object.py:36-97, which stand between GenerateContactObjectData
// (contact_pairs.hip) and GenerateContactScene.  Contract: include/s4g_ops.h (s4g_contact_refine_f32,
// s4g_contact_reduce_i32).
//
// s4g_contact_refine_f32 = check_single_collision (:71-97) for every frame of every object, which the script runs as a
// Python loop with one 4 x M product and nine sets of boolean masks per frame, over the object's OWN cloud.
//
//   cr_setup_kernel    zeroes the accumulators (no memset: every launch of the call is a kernel)
//   cr_scan_kernel     the cloud sweep of frame_sweep.h as cs_scan_kernel (contact_search.hip) runs it, points outer,
//                      frames inner, a point transformed once per frame, with THREE words per placement -- in the
//                      fingers (:86), in the close region (:89-90), close points with x < 0 (:93) -- and neither a
//                      label nor an extremum: 13 frames per workgroup and pass in the LDS cs_scan_kernel's five-word
//                      slots need for 8.  A row the pre-filter (:46) drops, a row at or past frame_count and a row
//                      with an entry that is not finite is never scanned (workgroup-uniform), and a pass without a
//                      live row does not sweep at all.
//   cr_finish_kernel   per frame: the verdict over the placements, the minimum close count, the failure bits
//   compact_valid_kernel   the kept rows in ascending frame index
//
// Decisions.  (1) min_search_score >= 1: the count gate (:91) then precedes the min() of an empty close region (:93),
// where the script would raise, and `if search_result:` (:101) never drops a kept frame.  (2) The script returns at
// the first failing placement; kept is the AND over the placements, so all are counted.  (3) check_single_collision(j)
// reads the enclosing i (:73); the loop passes i, so both are the same frame.
//
// s4g_contact_reduce_i32 = the fold of smooth_contact_object.py:61-89, which is sequential over an object's points (a
// point's surplus goes to neighbours whose running counts earlier points have changed): one wave per object, objects in
// parallel.  It walks the CSR of the filtered frames by point (rows of points without frames are never visited); the
// running counts live in LDS as bytes; the neighbours of a step go to lanes and the append position is ranked by
// ballot, so the order is the script's whatever the arrival.
//
// Limits: M, F < 2^30, B <= 65 535; the fold N <= 65 536 (the counters' LDS), frame_per_point <= 255, max_nn <= 8.
#include "frame_sweep.h"

namespace s4g {

constexpr int CR_MAX_LIST = 4;           // compiled maximum of each of the three shift lists
constexpr int CR_MAX_P = CR_MAX_LIST * CR_MAX_LIST * CR_MAX_LIST;
constexpr int CR_GX = 64;                // workgroups that share an object's frame list (frame k belongs to workgroup k mod 64)
constexpr int CR_U = 4;                  // points per lane held in registers while the workgroup's frames pass over them
constexpr int CR_SLOTS = 13;             // frames per workgroup and pass: 832 per object and pass
constexpr int CR_CHUNK_POINTS = 16384;   // point ranges per object: ceil(M / 16 384) within [4, 64]
constexpr int CR_MIN_CHUNKS = 4;
constexpr int CR_MAX_CHUNKS = 64;
constexpr int CR_ACC = 3;                // per placement: finger, close, behind
constexpr int CR_FAIL_FINGER = 1, CR_FAIL_FEW = 2, CR_FAIL_BEHIND = 4, CR_FAIL_NONFINITE = 8, CR_FAIL_FILTERED = 16;
constexpr int CR_FOLD_MAX_POINTS = 65536;
constexpr int CR_FOLD_MAX_NN = 8;

struct CrParams {
  float hbw, hbs;                        // HALF_BOTTOM_WIDTH, HALF_BOTTOM_SPACE
  float r2cull;                          // the cull radius squared, with slack
  float min_score;                       // MIN_SEARCH_SCORE as fp32 (exact: below 2^24)
  int nz, ny, nx, min_count, threshold;
};

struct CrTables {
  float zlo[CR_MAX_LIST], zhi[CR_MAX_LIST], ylo[CR_MAX_LIST], yhi[CR_MAX_LIST], dy[CR_MAX_LIST], xlo[CR_MAX_LIST],
      xhi[CR_MAX_LIST];
};

__device__ __forceinline__ int cr_points(const int64_t* __restrict__ count, int b, int M) {
  if (!count) return M;
  return (int)min((int64_t)M, max((int64_t)0, count[b]));
}

__global__ __launch_bounds__(256) void cr_setup_kernel(int* __restrict__ acc, size_t words) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < words) acc[i] = 0;
}

__global__ __launch_bounds__(256) void cr_scan_kernel(
    const float* __restrict__ xyz, const float* __restrict__ g2l, const float* __restrict__ search,
    const float* __restrict__ tables, int M, int F, CrParams p, int* __restrict__ acc,
    const int64_t* __restrict__ count, const int64_t* __restrict__ frame_count) {
  __shared__ float gl[CR_SLOTS][12];
  __shared__ int live[CR_SLOTS];
  __shared__ int cnt[CR_SLOTS][CR_MAX_P][CR_ACC];
  __shared__ CrTables tb;
  const int b = blockIdx.z, t = threadIdx.x;
  const int nz = p.nz, ny = p.ny, nx = p.nx, P = nz * ny * nx;
  const float* px = xyz + (size_t)b * 3 * M;
  const ChunkRange rg = chunk_range(cr_points(count, b, M));
  if (rg.empty()) return;
  if (t < nz) { tb.zlo[t] = tables[t]; tb.zhi[t] = tables[nz + t]; }
  if (t < ny) { tb.ylo[t] = tables[2 * nz + t]; tb.yhi[t] = tables[2 * nz + ny + t]; tb.dy[t] = tables[2 * nz + 2 * ny + t]; }
  if (t < nx) { tb.xlo[t] = tables[2 * nz + 3 * ny + t]; tb.xhi[t] = tables[2 * nz + 3 * ny + nx + t]; }
  const int fmax = frame_rows(frame_count, b, F);
  for (int j0 = 0; (int)blockIdx.x + CR_GX * j0 < fmax; j0 += CR_SLOTS) {
    __syncthreads();                                  // (the previous pass's accumulators have been flushed)
    const int nslot = pass_slots(fmax, CR_GX, j0, CR_SLOTS);
    bool ok = false;
    if (t < nslot) {
      const size_t row = (size_t)b * F + blockIdx.x + (size_t)CR_GX * (j0 + t);
      const float* G = g2l + row * 16;
      ok = search[row] > p.min_score;                 // :46; a NaN score is dropped
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        const float v = G[c];
        ok = ok && finite(v);
        if (c < 12) gl[t][c] = v;
      }
      live[t] = ok ? 1 : 0;
    }
    for (int i = t; i < nslot * P * CR_ACC; i += 256) ((int*)cnt[i / (P * CR_ACC)])[i % (P * CR_ACC)] = 0;
    if (!__syncthreads_or(ok ? 1 : 0)) continue;      // no live row in this pass: nothing to sweep, nothing to flush
    // (the narrow bound, not sweep_end: no ballot or shuffle below, every contribution is a per-lane LDS atomic)
    for (int i0 = rg.lo + t; i0 < rg.hi; i0 += 256 * CR_U) {
      PointBlock<CR_U> pt;
      pt.load(px, M, i0, rg.hi, i0);
      for (int sl = 0; sl < nslot; ++sl) {
        if (!live[sl]) continue;                      // workgroup-uniform
        float g[12];
#pragma unroll
        for (int c = 0; c < 12; ++c) g[c] = gl[sl][c];
#pragma unroll
        for (int u = 0; u < CR_U; ++u) {
          const LocalPoint l = local_point(g, pt.x[u], pt.y[u], pt.z[u]);
          const float lx = l.x, ly = l.y, lz = l.z;
          // the cull; a point that is not finite gives NaN or inf here and is in no region
          if (!pt.in[u] || !(lx * lx + ly * ly + lz * lz < p.r2cull)) continue;
          unsigned zb = 0, xb = 0, yb = 0, yc = 0;
          for (int k = 0; k < nz; ++k) zb |= (((lz < tb.zhi[k]) && (lz > tb.zlo[k])) ? 1u : 0u) << k;       // :75-76
          if (!zb) continue;
          for (int k = 0; k < nx; ++k) xb |= (((lx > tb.xlo[k]) && (lx < tb.xhi[k])) ? 1u : 0u) << k;       // :84-85
          if (!xb) continue;
          for (int k = 0; k < ny; ++k) {
            yb |= (((ly < tb.yhi[k]) && (ly > tb.ylo[k])) ? 1u : 0u) << k;                                  // :78-79
            const float ay = fabsf(ly + tb.dy[k]);                                                          // :80
            yc |= (((ay > p.hbs) && (ay < p.hbw)) ? 1u : 0u) << k;                                          // :81
          }
          if (!(yb | yc)) continue;
          const bool behind = lx < 0.f;                                                                     // :93
          for (int kz = 0; kz < nz; ++kz) {
            if (!((zb >> kz) & 1u)) continue;
            for (int ky = 0; ky < ny; ++ky) {
              const bool closer = (yb >> ky) & 1u, fing = (yc >> ky) & 1u;
              if (!(closer || fing)) continue;
              for (int kx = 0; kx < nx; ++kx) {
                if (!((xb >> kx) & 1u)) continue;
                int* a = cnt[sl][(kz * ny + ky) * nx + kx];
                if (fing) atomicAdd(a + 0, 1);                                                              // :86
                if (closer) {                                                                               // :89
                  atomicAdd(a + 1, 1);
                  if (behind) atomicAdd(a + 2, 1);
                }
              }
            }
          }
        }
      }
    }
    __syncthreads();
    for (int i = t; i < nslot * P * CR_ACC; i += 256) {
      const int sl = i / (P * CR_ACC), w = i % (P * CR_ACC);
      const int c = ((const int*)cnt[sl])[w];
      if (c) atomicAdd(acc + ((size_t)b * F + blockIdx.x + (size_t)CR_GX * (j0 + sl)) * P * CR_ACC + w, c);
    }
  }
}

// one thread per frame
__global__ __launch_bounds__(256) void cr_finish_kernel(
    const float* __restrict__ g2l, const float* __restrict__ search, const int* __restrict__ acc, int F, CrParams p,
    const int64_t* __restrict__ frame_count, int* __restrict__ counts, int* __restrict__ kept,
    float* __restrict__ score, int* __restrict__ fail) {
  const int b = blockIdx.y;
  const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= (size_t)F) return;
  const size_t row = (size_t)b * F + f;
  const int P = p.nz * p.ny * p.nx;
  int bits = 0;
  if (!(f < (size_t)frame_rows(frame_count, b, F)) || !(search[row] > p.min_score)) {
    bits = CR_FAIL_FILTERED;
  } else {
    bool all_finite = true;
#pragma unroll
    for (int c = 0; c < 16; ++c) all_finite = all_finite && finite(g2l[row * 16 + c]);
    if (!all_finite) bits = CR_FAIL_NONFINITE;
  }
  int* oc = counts + row * P * CR_ACC;
  int lowest = INT_MAX;
  if (bits) {
    for (int i = 0; i < P * CR_ACC; ++i) oc[i] = 0;
  } else {
    const int* a = acc + row * P * CR_ACC;
    for (int pl = 0; pl < P; ++pl) {
      const int fing = a[pl * 3], close = a[pl * 3 + 1], behind = a[pl * 3 + 2];
      oc[pl * 3] = fing; oc[pl * 3 + 1] = close; oc[pl * 3 + 2] = behind;
      bits |= (fing > p.threshold ? CR_FAIL_FINGER : 0) | (close < p.min_count ? CR_FAIL_FEW : 0) |      // :87, :91
              (behind > 0 ? CR_FAIL_BEHIND : 0);                                                          // :93
      lowest = min(lowest, close);                                                                        // :95
    }
  }
  kept[row] = bits == 0 ? 1 : 0;
  score[row] = bits == 0 ? (float)lowest : 0.f;        // a count below 2^30: exact below 2^24, the cloud's size
  fail[row] = bits;
}

// One wave per object: the fold of smooth_contact_object.py:61-89 over the CSR (offsets, order) of the filtered frames
// by point.  pfn = point_frame_num as bytes in LDS.
__global__ __launch_bounds__(64) void cr_fold_kernel(
    const int32_t* __restrict__ fpi, const int32_t* __restrict__ offsets, const int32_t* __restrict__ order,
    const int32_t* __restrict__ knn, const int64_t* __restrict__ count, int N, int F, int fpp, int mnf, int min_rest,
    int max_nn, int cap, int32_t* __restrict__ source, int32_t* __restrict__ point, int64_t* __restrict__ out_count,
    int32_t* __restrict__ flags) {
  extern __shared__ unsigned char pfn_lds[];
  volatile unsigned char* pfn = pfn_lds;   // other lanes write it between two reads of a lane
  const int b = blockIdx.x, lane = threadIdx.x;
  const int Nb = cr_points(count, b, N);
  const int32_t* off = offsets + (size_t)b * ((size_t)N + 1);
  const int32_t* ord = order + (size_t)b * F;
  const int32_t* fp = fpi + (size_t)b * F;
  const int32_t* nb = knn + (size_t)b * N * max_nn;
  int32_t* src = source + (size_t)b * cap;
  int32_t* pnt = point + (size_t)b * cap;
  for (int i = lane; i < ((Nb + 3) & ~3); i += 64) pfn[i] = 0;
  __builtin_amdgcn_wave_barrier();
  const int total = min(F, max(0, off[N]));           // the frames that passed the filter and name a point
  int outpos = 0;
  int k = 0;
  while (k < total) {                                 // every step consumes at least one row: k grows
    const int f0 = ord[k];
    const int i = (f0 >= 0 && f0 < F) ? fp[f0] : -1;
    if (i < 0 || i >= Nb) { ++k; continue; }          // (not a CSR of this list: the row counts for nobody)
    int hi = min(total, off[i + 1]);
    if (hi <= k) hi = k + 1;
    const int len = hi - k;
    const int cur = pfn[i];
    const int room = max(0, fpp - cur);
    const int take = len > fpp ? room : min(room, len);                     // :64, :84
    for (int j = lane; j < take; j += 64) {
      if (outpos + j < cap) { src[outpos + j] = ord[k + j]; pnt[outpos + j] = i; }
    }
    outpos += take;
    if (lane == 0) pfn[i] = (unsigned char)(cur + take);
    __builtin_amdgcn_wave_barrier();
    if (len > fpp && len - fpp > min_rest) {                                // :63, :71
      int n = -1;
      if (lane < max_nn) n = nb[(size_t)i * max_nn + lane];
      bool give = false;
      if (n >= 0 && n < Nb && lane < len - fpp) {
        const int c = pfn[n];
        give = (n < i && c < fpp) || (n > i && c < mnf);                    // :75-76; the point itself takes nothing
      }
      const uint64_t m = __ballot(give);
      if (give) {
        const int pos = outpos + mask_rank(m);
        if (pos < cap) { src[pos] = ord[k + fpp + lane]; pnt[pos] = n; }    // :78-81: rest[r], the NEIGHBOUR's index
        pfn[n] = (unsigned char)(pfn[n] + 1);
      }
      outpos += __popcll(m);
      __builtin_amdgcn_wave_barrier();
    }
    k = hi;
  }
  for (int j = min(outpos, cap) + lane; j < cap; j += 64) { src[j] = -1; pnt[j] = -1; }
  if (lane == 0) {
    out_count[b] = outpos;
    flags[b] = outpos > cap ? 1 : 0;
  }
}

}  // namespace s4g

extern "C" size_t s4g_contact_refine_workspace_bytes(int64_t B, int64_t M, int64_t F, int64_t P) {
  (void)M;
  if (B <= 0 || F <= 0 || P <= 0 || P > s4g::CR_MAX_P) return 0;
  return s4g::align256((size_t)B * (size_t)F * (size_t)P * s4g::CR_ACC * sizeof(int));
}

extern "C" int s4g_contact_refine_f32(const float* g2l_bf44, const float* xyz_b3m, const float* search_bf, int64_t B,
                                      int64_t M, int64_t F, int64_t nz, int64_t ny, int64_t nx, const float* params8,
                                      int32_t min_search_score, int32_t collision_threshold,
                                      const float* tables_2z3y2x, const int64_t* count_b,
                                      const int64_t* frame_count_b, int32_t* counts_bfp3, int32_t* kept_bf,
                                      float* score_bf, int32_t* fail_bf, int32_t* kept_index_bf, int64_t* kept_count_b,
                                      void* workspace, size_t workspace_bytes, s4g_stream_t stream) {
  using namespace s4g;
  if (B < 0 || M <= 0 || F < 0 || B > 65535 || F >= (1ll << 30) || M >= (1ll << 30)) return S4G_EINVAL;
  if (nz <= 0 || ny <= 0 || nx <= 0 || nz > CR_MAX_LIST || ny > CR_MAX_LIST || nx > CR_MAX_LIST) return S4G_EINVAL;
  if (min_search_score < 1 || min_search_score >= (1 << 24) || collision_threshold < 0) return S4G_EINVAL;
  if (B == 0) return S4G_OK;
  if (!kept_count_b || !params8 || !tables_2z3y2x) return S4G_EINVAL;
  if (F > 0 && (!g2l_bf44 || !xyz_b3m || !search_bf || !counts_bfp3 || !kept_bf || !score_bf || !fail_bf ||
                !kept_index_bf))
    return S4G_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (F > 0) {
    const int64_t P = nz * ny * nx;
    const size_t words = (size_t)B * (size_t)F * (size_t)P * CR_ACC;
    if ((words + 255) / 256 > 0x7fffffffull) return S4G_EINVAL;     // (cr_setup_kernel's grid)
    if (!workspace || workspace_bytes < s4g_contact_refine_workspace_bytes(B, M, F, P)) return S4G_EWORKSPACE;
    CrParams p;
    const float fl = params8[0], bl = params8[1], hht = params8[2];
    p.hbw = params8[3]; p.hbs = params8[4];
    // the box widened by the largest shifts, as s4g_contact_search_f32 forms it
    const float ex = (fl > bl ? fl : bl) + fabsf(params8[5]), ey = p.hbw + fabsf(params8[6]),
                ez = hht + fabsf(params8[7]);
    p.r2cull = (ex * ex + ey * ey + ez * ez) * 1.001f;
    p.min_score = (float)min_search_score;
    p.nz = (int)nz; p.ny = (int)ny; p.nx = (int)nx; p.min_count = min_search_score; p.threshold = collision_threshold;
    int* acc = (int*)workspace;
    hipLaunchKernelGGL(cr_setup_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, acc, words);
    S4G_LAUNCH_CHECK();
    const dim3 grid(CR_GX, (unsigned)sweep_chunks(M, CR_CHUNK_POINTS, CR_MIN_CHUNKS, CR_MAX_CHUNKS), (unsigned)B);
    hipLaunchKernelGGL(cr_scan_kernel, grid, dim3(256), 0, st, xyz_b3m, g2l_bf44, search_bf, tables_2z3y2x, (int)M,
                       (int)F, p, acc, count_b, frame_count_b);
    S4G_LAUNCH_CHECK();
    hipLaunchKernelGGL(cr_finish_kernel, dim3((unsigned)((F + 255) / 256), (unsigned)B), dim3(256), 0, st, g2l_bf44,
                       search_bf, (const int*)acc, (int)F, p, frame_count_b, (int*)counts_bfp3, (int*)kept_bf, score_bf,
                       (int*)fail_bf);
    S4G_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(compact_valid_kernel<KeepNonZero>, dim3((unsigned)B), dim3(256), 0, st, (const int*)kept_bf,
                     (int)F, (int*)kept_index_bf, kept_count_b);
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}

extern "C" int s4g_contact_reduce_i32(const int32_t* frame_point_index_bf, const int32_t* offsets_bn1,
                                      const int32_t* order_bf, const int32_t* knn_bnk, const int64_t* count_b,
                                      int64_t B, int64_t N, int64_t F, int32_t frame_per_point,
                                      int32_t max_neighbor_frame, int32_t min_rest, int32_t max_nn, int64_t cap,
                                      int32_t* source_frame_bc, int32_t* point_index_bc, int64_t* count_out_b,
                                      int32_t* flags_b, s4g_stream_t stream) {
  using namespace s4g;
  if (B < 0 || B > 65535 || N < 1 || N > CR_FOLD_MAX_POINTS || F < 0 || F >= (1ll << 30) || cap < 0 ||
      cap >= (1ll << 30))
    return S4G_EINVAL;
  if (frame_per_point < 1 || frame_per_point > 255 || max_neighbor_frame < 0 || max_neighbor_frame > frame_per_point ||
      max_nn < 1 || max_nn > CR_FOLD_MAX_NN || min_rest < max_nn - 1)
    return S4G_EINVAL;
  if (B == 0) return S4G_OK;
  if (!offsets_bn1 || !knn_bnk || !count_out_b || !flags_b) return S4G_EINVAL;
  if (F > 0 && (!frame_point_index_bf || !order_bf)) return S4G_EINVAL;
  if (cap > 0 && (!source_frame_bc || !point_index_bc)) return S4G_EINVAL;
  const size_t lds = ((size_t)N + 3) & ~(size_t)3;
  hipLaunchKernelGGL(cr_fold_kernel, dim3((unsigned)B), dim3(64), lds, (hipStream_t)stream, frame_point_index_bf,
                     offsets_bn1, order_bf, knn_bnk, count_b, (int)N, (int)F, (int)frame_per_point,
                     (int)max_neighbor_frame, (int)min_rest, (int)max_nn, (int)cap, source_frame_bc, point_index_bc,
                     count_out_b, flags_b);
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}
