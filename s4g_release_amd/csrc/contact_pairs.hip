// The contact model's per-object frames: GenerateContactObjectData (data_gen/data_generator/
// data_object_contact_point_generator.py) restated for every object of a batch, without host synchronisation.
// Contract: include/s4g_ops.h (s4g_contact_pairs_f32, s4g_contact_pair_grade_f32).
//
// s4g_contact_pairs_f32 = cache_contact_pair (:103-123): the N x N antipodal test, evaluated in double from the fp32
// inputs in the reference's operation order, and the list of np.nonzero(np.triu(...)): ascending i, then ascending j.
// Order must not depend on arrival, so the predicate runs twice:
//
//   cp_pairs_kernel<false>  one wave per row i, columns j > i in 64-lane steps: the row's count (popcount of a ballot)
//   exclusive_scan_i32      the library's own scan (radix_sort.h): counts -> offsets, over all rows of all objects
//   cp_fill_kernel          -1 / 0 into every row of the padded list
//   cp_pairs_kernel<true>   the same walk; a kept column's place is the row's offset + the running count + its rank in
//                           the ballot.  Row 0's wave also writes the object's exact count and its overflow flag
//
// s4g_contact_pair_grade_f32 = _estimate_grasp_quality with check_collision (:125-221), the frames it appends and
// get_frame_neighbor (:79-86):
//
//   cp_frame_kernel    per pair, once, in double and rounded to fp32 once: y = (p_j - p_i) / |.|, x = e_y - (e_y . y) y
//                      normalised, z = x cross y, the midpoint c, T = [R^T | -R^T c] (:139-152)
//   cp_zero_kernel     the counters of the workspace (no memset: every launch of the call is a kernel)
//   cp_scan_kernel     a cloud sweep (frame_sweep.h: points outer, pairs inner): per (roll, shift) the counts behind the
//                      palm / in the fingers / in the close region, and the pair's close-plane count, in LDS, then the
//                      workspace; integer atomics only, so the result does not depend on their order
//   cp_finish_kernel   per (pair, roll): the reference's gates in the reference's order (:186-217), score and validity
//   compact_valid_kernel  the valid (pair, roll) in ascending pair * T + roll: the reference's append order
//   cp_emit_kernel     per kept frame: global_to_local = L2LS[roll] @ T (:218), its scores and its source
//   cp_nearest_kernel  one wave per kept frame: the object point nearest to the frame's centre (:82-85), a 64-bit
//                      (distance bits, index) key reduced by minimum
//
// Decisions.  (1) The frame is formed in double and its rigid inverse analytically, not by torch.inverse in fp32
// (:152).  (2) A pair whose frame is not finite (y parallel to e_y, coincident points, a point that is not finite)
// gets no frame and fail bit 0; the reference would propagate NaN.  (3) pair_score and antipodal_score are fp32, the
// double rounded once; the reference keeps float64.  (4) Thresholds and search lists are configuration with the
// reference's values as defaults, bounded by CP_MAX_THETA rolls and CP_MAX_SHIFT shifts.
//
// Limits: 1 <= N <= 2^20 and B * N * (N - 1) / 2 < 2^31 (the scan is int32), max_pairs and P < 2^24, P * T < 2^30,
// max_frames < 2^30, B <= 65 535 (grid.y / grid.z).
#include "frame_sweep.h"
#include "radix_sort.h"

namespace s4g {

constexpr int CP_MAX_THETA = 16;         // compiled maximum of theta_search (12 as shipped)
constexpr int CP_MAX_SHIFT = 4;          // compiled maximum of width_shift (3 as shipped)
constexpr int CP_KINDS = 3;              // back, finger, close
constexpr int CP_MAX_WORDS = CP_MAX_THETA * CP_MAX_SHIFT * CP_KINDS + 1;   // + the close-plane count; 109 as shipped
constexpr int CP_GX = 256;               // workgroups that share an object's pair list (pair k belongs to workgroup k mod 256)
constexpr int CP_U = 4;                  // points per lane held in registers while the workgroup's pairs pass over them
constexpr int CP_SLOTS = 16;             // pairs per workgroup and pass: 16 x 193 words = 12 KiB of LDS at the maxima, so
                                         // eight workgroups of a compute unit keep under its 160 KiB
constexpr int CP_CHUNK_POINTS = 1024;    // point ranges per object: ceil(N / 1 024) within [1, 64]: one sweep each
constexpr int CP_MIN_CHUNKS = 1;
constexpr int CP_MAX_CHUNKS = 64;

// ---- pair enumeration -------------------------------------------------------------------------------------------------

// the test of :104-114 for row i, column j, in double from the fp32 inputs; every NaN fails it
__device__ __forceinline__ bool cp_pair_test(double pix, double piy, double piz, double nix, double niy, double niz,
                                             const float* __restrict__ px, const float* __restrict__ pn, int N, int j,
                                             double max_distance, double cos_threshold, double* __restrict__ score) {
  const double vx = (double)px[j] - pix, vy = (double)px[(size_t)N + j] - piy, vz = (double)px[2 * (size_t)N + j] - piz;
  const double d = sqrt(vx * vx + vy * vy + vz * vz);
  const double dc = d < 1e-4 ? 1e-4 : (d > 1.0 ? 1.0 : d);                       // np.clip(norm, 0.0001, 1), :107
  const double ux = vx / dc, uy = vy / dc, uz = vz / dc;
  const double cij = ux * nix + uy * niy + uz * niz;                              // :109
  const double cji = (-ux) * (double)pn[j] + (-uy) * (double)pn[(size_t)N + j] + (-uz) * (double)pn[2 * (size_t)N + j];
  const double s = fabs(cij * cji);                                               // :111
  *score = s;
  return (d < max_distance) && (s > cos_threshold);                               // :105, :113
}

// one wave per row; WRITE = false: rowcnt[b * N + i]; WRITE = true: the row's pairs at off[b * N + i] - off[b * N]
template <bool WRITE>
__global__ __launch_bounds__(256) void cp_pairs_kernel(
    const float* __restrict__ xyz, const float* __restrict__ nrm, const int64_t* __restrict__ count, int B, int N,
    int max_pairs, double max_distance, double cos_threshold, int* __restrict__ rowcnt, const int* __restrict__ off,
    int* __restrict__ pairs, float* __restrict__ pair_score, int64_t* __restrict__ pair_count,
    int* __restrict__ flags) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int i = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (i >= N) return;                                  // wave-uniform
  const float* px = xyz + (size_t)b * 3 * N;
  const float* pn = nrm + (size_t)b * 3 * N;
  const int n = frame_rows(count, b, N);               // a point at or past count[b] pairs with nothing
  const size_t row = (size_t)b * N + i;
  int base = 0;
  if (WRITE) {
    const int start = off[(size_t)b * N];
    base = off[row] - start;
    if (i == 0 && lane == 0) {
      const int total = off[(size_t)(b + 1) * N] - start;
      pair_count[b] = total;
      flags[b] = total > max_pairs ? 1 : 0;
    }
  } else if (b == 0 && i == 0 && lane == 0) {
    rowcnt[(size_t)B * N] = 0;                         // (the scan's last element: its offset is the grand total)
  }
  int kept = 0;
  if (i < n) {
    const double pix = px[i], piy = px[(size_t)N + i], piz = px[2 * (size_t)N + i];
    const double nix = pn[i], niy = pn[(size_t)N + i], niz = pn[2 * (size_t)N + i];
    for (int j0 = i + 1; j0 < n; j0 += 64) {           // the diagonal can never pass: i < j
      const int j = j0 + lane;
      double s = 0.0;
      const bool ok = j < n && cp_pair_test(pix, piy, piz, nix, niy, niz, px, pn, N, j, max_distance, cos_threshold, &s);
      const uint64_t m = __ballot(ok);
      if (WRITE && ok) {
        const int at = base + kept + mask_rank(m);
        if (at < max_pairs) {
          pairs[((size_t)b * max_pairs + at) * 2] = i;
          pairs[((size_t)b * max_pairs + at) * 2 + 1] = j;
          pair_score[(size_t)b * max_pairs + at] = (float)s;
        }
      }
      kept += __popcll(m);
    }
  }
  if (!WRITE && lane == 0) rowcnt[row] = kept;
}

__global__ __launch_bounds__(256) void cp_fill_kernel(int* __restrict__ pairs, float* __restrict__ pair_score, size_t rows) {
  const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  pairs[2 * r] = -1;
  pairs[2 * r + 1] = -1;
  pair_score[r] = 0.f;
}

// ---- pair grading -----------------------------------------------------------------------------------------------------

struct CpParams {
  float hbw, hbs, margin, neg_bl, fl;    // HALF_BOTTOM_WIDTH, HALF_BOTTOM_SPACE, BACK_COLLISION_MARGIN, -BOTTOM_LENGTH, FINGER_LENGTH
  double min_points, back_threshold, finger_threshold;
  int T, W, words;                       // rolls, shifts, T * W * 3 + 1
};

// one thread per pair: rows 0..2 of T = [R^T | -R^T c] and whether the pair is scanned
__global__ __launch_bounds__(256) void cp_frame_kernel(
    const float* __restrict__ xyz, const int64_t* __restrict__ count, const int* __restrict__ pairs,
    const int64_t* __restrict__ pair_count, int N, int P, float* __restrict__ Tm, int* __restrict__ live,
    int* __restrict__ fail) {
  const int b = blockIdx.y;
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= (size_t)P) return;
  const size_t row = (size_t)b * P + k;
  const float* px = xyz + (size_t)b * 3 * N;
  float* o = Tm + row * 12;
  int bits = 0;
  bool ok = false;
  if (k < (size_t)frame_rows(pair_count, b, P)) {
    const int n = frame_rows(count, b, N);
    const int i = pairs[row * 2], j = pairs[row * 2 + 1];
    if (i < 0 || j < 0 || i >= n || j >= n) {
      bits = 4;
    } else {
      const double ax = px[i], ay = px[(size_t)N + i], az = px[2 * (size_t)N + i];
      const double bx = px[j], by = px[(size_t)N + j], bz = px[2 * (size_t)N + j];
      const double vx = bx - ax, vy = by - ay, vz = bz - az;
      const double len = sqrt(vx * vx + vy * vy + vz * vz);
      const double y0 = vx / len, y1 = vy / len, y2 = vz / len;                  // :139-140
      double x0 = 0.0 - y1 * y0, x1 = 1.0 - y1 * y1, x2 = 0.0 - y1 * y2;         // :142-143, e_y = (0, 1, 0)
      const double xl = sqrt(x0 * x0 + x1 * x1 + x2 * x2);
      x0 /= xl; x1 /= xl; x2 /= xl;                                              // :144
      const double z0 = x1 * y2 - x2 * y1, z1 = x2 * y0 - x0 * y2, z2 = x0 * y1 - x1 * y0;   // :145
      const double cx = (ax + bx) / 2, cy = (ay + by) / 2, cz = (az + bz) / 2;   // :150
      const double t[12] = {x0, x1, x2, -(x0 * cx + x1 * cy + x2 * cz), y0, y1, y2, -(y0 * cx + y1 * cy + y2 * cz),
                            z0, z1, z2, -(z0 * cx + z1 * cy + z2 * cz)};
      ok = true;
#pragma unroll
      for (int c = 0; c < 12; ++c) {
        o[c] = (float)t[c];
        ok = ok && finite(t[c]);
      }
      if (!ok) bits = 1;
    }
  }
  if (!ok) {
#pragma unroll
    for (int c = 0; c < 12; ++c) o[c] = 0.f;
  }
  live[row] = ok ? 1 : 0;
  fail[row] = bits;
}

__global__ __launch_bounds__(256) void cp_zero_kernel(int* __restrict__ acc, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) acc[i] = 0;
}

// device table layout (floats): rows 0..2 of L2LS[theta] (12 each, T of them), z lower[W], z upper[W]
__global__ __launch_bounds__(256) void cp_scan_kernel(
    const float* __restrict__ xyz, const int64_t* __restrict__ count, const float* __restrict__ Tm,
    const int* __restrict__ live_g, const float* __restrict__ tables, int N, int P, CpParams p,
    const int64_t* __restrict__ pair_count, int* __restrict__ acc) {
  __shared__ float gl[CP_SLOTS][12];
  __shared__ int live[CP_SLOTS];
  __shared__ int cnt[CP_SLOTS][CP_MAX_WORDS];
  __shared__ float rollx[CP_MAX_THETA][4], rollz[CP_MAX_THETA][4];     // rows 0 and 2 of L2LS: x and z of the roll
  __shared__ float zlo[CP_MAX_SHIFT], zhi[CP_MAX_SHIFT];
  const int b = blockIdx.z, t = threadIdx.x;
  const int T = p.T, W = p.W, words = p.words;
  const float* px = xyz + (size_t)b * 3 * N;
  const int n = frame_rows(count, b, N);
  const ChunkRange full = chunk_range(N);
  ChunkRange rg;
  rg.lo = full.lo;
  rg.hi = min(full.hi, n);                             // points at or past count[b] are not part of the object
  if (rg.empty()) return;
  if (t < T * 4) {
    rollx[t >> 2][t & 3] = tables[(t >> 2) * 12 + (t & 3)];
    rollz[t >> 2][t & 3] = tables[(t >> 2) * 12 + 8 + (t & 3)];
  }
  if (t < W) {
    zlo[t] = tables[T * 12 + t];
    zhi[t] = tables[T * 12 + W + t];
  }
  const int kmax = frame_rows(pair_count, b, P);
  for (int j0 = 0; (int)blockIdx.x + CP_GX * j0 < kmax; j0 += CP_SLOTS) {
    __syncthreads();                                   // (the previous pass's counters have been flushed)
    const int nslot = pass_slots(kmax, CP_GX, j0, CP_SLOTS);
    if (t < nslot * 12) {
      const size_t row = (size_t)b * P + blockIdx.x + (size_t)CP_GX * (j0 + t / 12);
      gl[t / 12][t % 12] = Tm[row * 12 + t % 12];
      if (t % 12 == 0) live[t / 12] = live_g[row];
    }
    for (int i = t; i < nslot * words; i += 256) cnt[i / words][i % words] = 0;
    __syncthreads();
    // (the narrow bound: every contribution is a per-lane LDS atomic, no ballot or shuffle: frame_sweep.h)
    for (int i0 = rg.lo + t; i0 < rg.hi; i0 += 256 * CP_U) {
      PointBlock<CP_U> pt;
      pt.load(px, N, i0, rg.hi, i0);
      for (int sl = 0; sl < nslot; ++sl) {
        if (!live[sl]) continue;                       // workgroup-uniform
        float g[12];
#pragma unroll
        for (int c = 0; c < 12; ++c) g[c] = gl[sl][c];
        int* c = cnt[sl];
#pragma unroll
        for (int u = 0; u < CP_U; ++u) {
          const LocalPoint l = local_point(g, pt.x[u], pt.y[u], pt.z[u]);
          const float ay = fabsf(l.y);
          // a point with |ly| >= hbw contributes nothing; one that is not finite gives NaN here
          if (!pt.in[u] || !(ay < p.hbw)) continue;
          const bool close = ay < p.hbs;                                          // :171-172
          const bool fing = ay > p.hbs;                                           // :176-180
          if (!(close || fing)) continue;                                         // (|ly| == hbs: in no plane, :182)
          if (close) atomicAdd(c + words - 1, 1);                                 // :173
          for (int th = 0; th < T; ++th) {
            const float sx = rollx[th][0] * l.x + rollx[th][1] * l.y + rollx[th][2] * l.z + rollx[th][3];   // :184
            const bool backx = (sx < p.margin) && (sx > p.neg_bl);                // :188-189
            const bool fingx = (sx > p.margin) && (sx < p.fl);                    // :190-191
            if (!(backx || fingx)) continue;
            const float sz = rollz[th][0] * l.x + rollz[th][1] * l.y + rollz[th][2] * l.z + rollz[th][3];
            const int kind = backx ? 0 : (fing ? 1 : 2);                          // :197, :202, :206
            for (int w = 0; w < W; ++w) {
              if ((sz < zhi[w]) && (sz > zlo[w])) atomicAdd(c + (th * W + w) * CP_KINDS + kind, 1);         // :195-196
            }
          }
        }
      }
    }
    __syncthreads();
    for (int i = t; i < nslot * words; i += 256) {
      const int sl = i / words, w = i % words;
      const int v = cnt[sl][w];
      if (v) atomicAdd(acc + ((size_t)b * P + blockIdx.x + (size_t)CP_GX * (j0 + sl)) * words + w, v);
    }
  }
}

// one thread per (pair, roll)
__global__ __launch_bounds__(256) void cp_finish_kernel(
    const int* __restrict__ acc, const int* __restrict__ live, int P, CpParams p, int* __restrict__ counts,
    int* __restrict__ close_plane, float* __restrict__ score, int* __restrict__ valid, int* __restrict__ fail) {
  const int b = blockIdx.y;
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int T = p.T, W = p.W;
  if (q >= (size_t)P * T) return;
  const size_t k = q / T;
  const int th = (int)(q % T);
  const size_t row = (size_t)b * P + k;
  const int* a = acc + row * p.words;
  const bool scanned = live[row] != 0;
  const int plane = scanned ? a[p.words - 1] : 0;
  int* oc = counts + ((size_t)row * T + th) * W * CP_KINDS;
  float accum = 0.f, last = 0.f;                                                  // :192, :194
  for (int w = 0; w < W; ++w) {
    const int back = scanned ? a[(th * W + w) * CP_KINDS] : 0, fing = scanned ? a[(th * W + w) * CP_KINDS + 1] : 0,
              close = scanned ? a[(th * W + w) * CP_KINDS + 2] : 0;
    oc[w * CP_KINDS] = back; oc[w * CP_KINDS + 1] = fing; oc[w * CP_KINDS + 2] = close;
    last = 0.f;                                                                   // :194: reset for every shift
    if ((double)back > p.back_threshold) continue;                                // :199
    if ((double)fing > p.finger_threshold) continue;                              // :203
    last = (float)close;                                                          // :207
    if ((double)last < p.min_points) continue;                                    // :209
    accum = __fadd_rn(accum, __fdiv_rn(last, 3.0f));                              // :212
  }
  const bool planes = scanned && !((double)plane < p.min_points);                 // :173
  const bool ok = planes && !((double)accum < p.min_points) && !((double)last < p.min_points);   // :214
  score[row * T + th] = ok ? fminf(accum, last) : 0.f;                            // :217
  valid[row * T + th] = ok ? 1 : 0;
  if (th == 0) {
    close_plane[row] = plane;
    if (scanned && !planes) fail[row] |= 2;
  }
}

// one thread per row of the frame list
__global__ __launch_bounds__(256) void cp_emit_kernel(
    const int* __restrict__ vindex, const int64_t* __restrict__ vcount, const float* __restrict__ Tm,
    const float* __restrict__ tables, const float* __restrict__ score, const float* __restrict__ pair_score, int P,
    int T, int max_frames, float* __restrict__ g2l, float* __restrict__ search, float* __restrict__ antipodal,
    int* __restrict__ source, int64_t* __restrict__ frame_count, int* __restrict__ flags) {
  const int b = blockIdx.y;
  const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = vcount[b];
  if (f == 0) {
    frame_count[b] = total;
    flags[b] = total > (int64_t)max_frames ? 2 : 0;
  }
  if (f >= (size_t)max_frames) return;
  const size_t orow = (size_t)b * max_frames + f;
  float* o = g2l + orow * 16;
  if ((int64_t)f >= total) {
#pragma unroll
    for (int c = 0; c < 16; ++c) o[c] = 0.f;
    search[orow] = 0.f;
    antipodal[orow] = 0.f;
    source[orow] = -1;
    return;
  }
  const int q = vindex[(size_t)b * P * T + f];
  const size_t row = (size_t)b * P + q / T;
  const float* m = tables + (size_t)(q % T) * 12;
  const float* tm = Tm + row * 12;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      // :218 in fp32; row 3 of T is (0, 0, 0, 1)
      float v = m[r * 4] * tm[c] + m[r * 4 + 1] * tm[4 + c] + m[r * 4 + 2] * tm[8 + c];
      if (c == 3) v = v + m[r * 4 + 3];
      o[r * 4 + c] = v;
    }
  }
  o[12] = 0.f; o[13] = 0.f; o[14] = 0.f; o[15] = 1.f;
  search[orow] = score[(size_t)b * P * T + q];
  antipodal[orow] = pair_score ? pair_score[row] : 0.f;
  source[orow] = q;
}

// one wave per row of the frame list
__global__ __launch_bounds__(256) void cp_nearest_kernel(
    const float* __restrict__ xyz, const int64_t* __restrict__ count, const float* __restrict__ g2l,
    const int* __restrict__ source, int N, int max_frames, int* __restrict__ nearest) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int f = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (f >= max_frames) return;                         // wave-uniform
  const size_t orow = (size_t)b * max_frames + f;
  if (source[orow] < 0) {                              // wave-uniform
    if (lane == 0) nearest[orow] = -1;
    return;
  }
  const float* G = g2l + orow * 16;
  // the translation of the rigid inverse [R^T | -R^T t]: the frame's centre in global coordinates (:82-83)
  const float cx = -__fadd_rn(__fadd_rn(__fmul_rn(G[0], G[3]), __fmul_rn(G[4], G[7])), __fmul_rn(G[8], G[11]));
  const float cy = -__fadd_rn(__fadd_rn(__fmul_rn(G[1], G[3]), __fmul_rn(G[5], G[7])), __fmul_rn(G[9], G[11]));
  const float cz = -__fadd_rn(__fadd_rn(__fmul_rn(G[2], G[3]), __fmul_rn(G[6], G[7])), __fmul_rn(G[10], G[11]));
  const float* px = xyz + (size_t)b * 3 * N;
  const int n = frame_rows(count, b, N);
  unsigned long long best = ~0ull;
  for (int i = lane; i < n; i += 64) {
    const float d2 = dist2<false>(cx, cy, cz, px[i], px[(size_t)N + i], px[2 * (size_t)N + i]);
    if (!finite(d2)) continue;
    // d2 >= 0: its bits order as the value does; the lower index wins a tie
    const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)i;
    best = key < best ? key : best;
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const unsigned long long o = __shfl_xor(best, s);
    best = o < best ? o : best;
  }
  if (lane == 0) nearest[orow] = best == ~0ull ? -1 : (int)(unsigned)(best & 0xffffffffull);
}

struct CpPairsWs {
  int* rowcnt;
  int* off;
  void* scan;
  size_t scan_bytes, total;
};
static CpPairsWs cp_pairs_ws(void* base, size_t B, size_t N) {
  const size_t rows = B * N + 1;
  CpPairsWs w;
  size_t at = 0;
  auto take = [&](size_t bytes) {
    void* ptr = base ? (char*)base + at : nullptr;
    at += align256(bytes);
    return ptr;
  };
  w.rowcnt = (int*)take(rows * sizeof(int));
  w.off = (int*)take(rows * sizeof(int));
  w.scan_bytes = scan_ws_bytes(rows);
  w.scan = take(w.scan_bytes);
  w.total = at;
  return w;
}

struct CpGradeWs {
  float* Tm;
  int* live;
  int* acc;
  int* vindex;
  int64_t* vcount;
  size_t total;
};
static CpGradeWs cp_grade_ws(void* base, size_t B, size_t P, size_t T, size_t W) {
  CpGradeWs w;
  size_t at = 0;
  auto take = [&](size_t bytes) {
    void* ptr = base ? (char*)base + at : nullptr;
    at += align256(bytes);
    return ptr;
  };
  w.Tm = (float*)take(B * P * 12 * sizeof(float));
  w.live = (int*)take(B * P * sizeof(int));
  w.acc = (int*)take(B * P * (T * W * CP_KINDS + 1) * sizeof(int));
  w.vindex = (int*)take(B * P * T * sizeof(int));
  w.vcount = (int64_t*)take(B * sizeof(int64_t));
  w.total = at;
  return w;
}

static bool cp_pairs_shape_ok(int64_t B, int64_t N) {
  if (B < 0 || B > 65535 || N < 1 || N > (1ll << 20)) return false;
  return B == 0 || N * (N - 1) / 2 < (1ll << 31) / B;
}

}  // namespace s4g

extern "C" size_t s4g_contact_pairs_workspace_bytes(int64_t B, int64_t N) {
  if (B <= 0 || !s4g::cp_pairs_shape_ok(B, N)) return 0;
  return s4g::cp_pairs_ws(nullptr, (size_t)B, (size_t)N).total;
}

extern "C" int s4g_contact_pairs_f32(const float* xyz_b3n, const float* normals_b3n, const int64_t* count_b, int64_t B,
                                     int64_t N, int64_t max_pairs, double max_distance, double cos_threshold,
                                     int32_t* pairs_bp2, float* pair_score_bp, int64_t* pair_count_b, int32_t* flags_b,
                                     void* workspace, size_t workspace_bytes, s4g_stream_t stream) {
  using namespace s4g;
  if (!cp_pairs_shape_ok(B, N) || max_pairs < 0 || max_pairs >= (1ll << 24)) return S4G_EINVAL;
  if (B == 0) return S4G_OK;
  if (!xyz_b3n || !normals_b3n || !pair_count_b || !flags_b || (max_pairs > 0 && (!pairs_bp2 || !pair_score_bp)))
    return S4G_EINVAL;
  if (!workspace || workspace_bytes < s4g_contact_pairs_workspace_bytes(B, N)) return S4G_EWORKSPACE;
  const CpPairsWs w = cp_pairs_ws(workspace, (size_t)B, (size_t)N);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((N + 3) / 4), (unsigned)B);
  hipLaunchKernelGGL(cp_pairs_kernel<false>, grid, dim3(256), 0, st, xyz_b3n, normals_b3n, count_b, (int)B, (int)N,
                     (int)max_pairs, max_distance, cos_threshold, w.rowcnt, (const int*)nullptr, (int*)nullptr,
                     (float*)nullptr, (int64_t*)nullptr, (int*)nullptr);
  S4G_LAUNCH_CHECK();
  const size_t rows = (size_t)B * (size_t)N + 1;
  if (int rc = exclusive_scan_i32(w.scan, w.scan_bytes, w.rowcnt, w.off, rows, st)) return rc;
  if (max_pairs > 0) {
    const size_t fill = (size_t)B * (size_t)max_pairs;
    hipLaunchKernelGGL(cp_fill_kernel, dim3((unsigned)((fill + 255) / 256)), dim3(256), 0, st, (int*)pairs_bp2,
                       pair_score_bp, fill);
    S4G_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(cp_pairs_kernel<true>, grid, dim3(256), 0, st, xyz_b3n, normals_b3n, count_b, (int)B, (int)N,
                     (int)max_pairs, max_distance, cos_threshold, (int*)nullptr, (const int*)w.off, (int*)pairs_bp2,
                     pair_score_bp, pair_count_b, (int*)flags_b);
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}

static bool cp_grade_shape_ok(int64_t B, int64_t N, int64_t P, int64_t T, int64_t W, int64_t max_frames) {
  return B >= 0 && B <= 65535 && N >= 1 && N <= (1ll << 20) && P >= 0 && P < (1ll << 24) && T >= 1 &&
         T <= s4g::CP_MAX_THETA && W >= 1 && W <= s4g::CP_MAX_SHIFT && P * T < (1ll << 30) && max_frames >= 0 &&
         max_frames < (1ll << 30);
}

extern "C" size_t s4g_contact_pair_grade_workspace_bytes(int64_t B, int64_t N, int64_t P, int64_t T, int64_t W) {
  if (B <= 0 || P <= 0 || !cp_grade_shape_ok(B, N, P, T, W, 0)) return 0;
  return s4g::cp_grade_ws(nullptr, (size_t)B, (size_t)P, (size_t)T, (size_t)W).total;
}

extern "C" int s4g_contact_pair_grade_f32(
    const float* xyz_b3n, const int64_t* count_b, const int32_t* pairs_bp2, const float* pair_score_bp,
    const int64_t* pair_count_b, int64_t B, int64_t N, int64_t P, int64_t T, int64_t W, const float* params5,
    const double* gates3, const float* tables_12t2w, int64_t max_frames, int32_t* counts_bptw3,
    int32_t* close_plane_bp, float* score_bpt, int32_t* valid_bpt, int32_t* fail_bp, float* g2l_bf44,
    float* search_score_bf, float* antipodal_score_bf, int32_t* frame_source_bf, int32_t* frame_point_index_bf,
    int64_t* frame_count_b, int32_t* flags_b, void* workspace, size_t workspace_bytes, s4g_stream_t stream) {
  using namespace s4g;
  if (!cp_grade_shape_ok(B, N, P, T, W, max_frames)) return S4G_EINVAL;
  if (B == 0) return S4G_OK;
  if (!frame_count_b || !flags_b) return S4G_EINVAL;
  if (P > 0 && (!xyz_b3n || !pairs_bp2 || !params5 || !gates3 || !tables_12t2w || !counts_bptw3 || !close_plane_bp ||
                !score_bpt || !valid_bpt || !fail_bp))
    return S4G_EINVAL;
  if (max_frames > 0 && (!xyz_b3n || !g2l_bf44 || !search_score_bf || !antipodal_score_bf || !frame_source_bf ||
                         !frame_point_index_bf))
    return S4G_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  CpGradeWs w;
  w.Tm = nullptr; w.live = nullptr; w.acc = nullptr; w.vindex = nullptr; w.vcount = frame_count_b; w.total = 0;
  if (P > 0) {
    if (!workspace || workspace_bytes < s4g_contact_pair_grade_workspace_bytes(B, N, P, T, W)) return S4G_EWORKSPACE;
    w = cp_grade_ws(workspace, (size_t)B, (size_t)P, (size_t)T, (size_t)W);
    CpParams p;
    p.hbw = params5[0]; p.hbs = params5[1]; p.margin = params5[2]; p.neg_bl = -params5[3]; p.fl = params5[4];
    p.min_points = gates3[0]; p.back_threshold = gates3[1]; p.finger_threshold = gates3[2];
    p.T = (int)T; p.W = (int)W; p.words = (int)(T * W * CP_KINDS + 1);
    const dim3 per_pair((unsigned)((P + 255) / 256), (unsigned)B);
    hipLaunchKernelGGL(cp_frame_kernel, per_pair, dim3(256), 0, st, xyz_b3n, count_b, (const int*)pairs_bp2,
                       pair_count_b, (int)N, (int)P, w.Tm, w.live, (int*)fail_bp);
    S4G_LAUNCH_CHECK();
    const size_t nacc = (size_t)B * (size_t)P * (size_t)p.words;
    if ((nacc + 255) / 256 > 0x7fffffffull) return S4G_EINVAL;
    hipLaunchKernelGGL(cp_zero_kernel, dim3((unsigned)((nacc + 255) / 256)), dim3(256), 0, st, w.acc, nacc);
    S4G_LAUNCH_CHECK();
    const dim3 grid(CP_GX, (unsigned)sweep_chunks(N, CP_CHUNK_POINTS, CP_MIN_CHUNKS, CP_MAX_CHUNKS), (unsigned)B);
    hipLaunchKernelGGL(cp_scan_kernel, grid, dim3(256), 0, st, xyz_b3n, count_b, (const float*)w.Tm,
                       (const int*)w.live, tables_12t2w, (int)N, (int)P, p, pair_count_b, w.acc);
    S4G_LAUNCH_CHECK();
    hipLaunchKernelGGL(cp_finish_kernel, dim3((unsigned)((P * T + 255) / 256), (unsigned)B), dim3(256), 0, st,
                       (const int*)w.acc, (const int*)w.live, (int)P, p, (int*)counts_bptw3, (int*)close_plane_bp,
                       score_bpt, (int*)valid_bpt, (int*)fail_bp);
    S4G_LAUNCH_CHECK();
    hipLaunchKernelGGL(compact_valid_kernel<KeepNonZero>, dim3((unsigned)B), dim3(256), 0, st, (const int*)valid_bpt,
                       (int)(P * T), w.vindex, w.vcount);
    S4G_LAUNCH_CHECK();
  } else {
    hipLaunchKernelGGL(cp_zero_kernel, dim3((unsigned)((2 * B + 255) / 256)), dim3(256), 0, st, (int*)frame_count_b,
                       (size_t)(2 * B));                  // (int64 zeros, two words each)
    S4G_LAUNCH_CHECK();
    w.vcount = frame_count_b;
  }
  const int64_t rows = max_frames > 0 ? max_frames : 1;   // (row 0's thread writes the count and the flag)
  hipLaunchKernelGGL(cp_emit_kernel, dim3((unsigned)((rows + 255) / 256), (unsigned)B), dim3(256), 0, st,
                     (const int*)w.vindex, (const int64_t*)w.vcount, (const float*)w.Tm, tables_12t2w,
                     (const float*)score_bpt, pair_score_bp, (int)P, (int)T, (int)max_frames, g2l_bf44,
                     search_score_bf, antipodal_score_bf, (int*)frame_source_bf, frame_count_b, (int*)flags_b);
  S4G_LAUNCH_CHECK();
  if (max_frames > 0) {
    hipLaunchKernelGGL(cp_nearest_kernel, dim3((unsigned)((max_frames + 3) / 4), (unsigned)B), dim3(256), 0, st,
                       xyz_b3n, count_b, (const float*)g2l_bf44, (const int*)frame_source_bf, (int)N,
                       (int)max_frames, (int*)frame_point_index_bf);
    S4G_LAUNCH_CHECK();
  }
  return S4G_OK;
}
