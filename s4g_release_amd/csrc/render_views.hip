// The step in front of the data generator's view pipeline: the views themselves.  data_gen/render/cycles_render.py
// renders every scene from four fixed cameras inside Blender and keeps, per view, a pinhole depth image of RAY LENGTHS
// (:118-153): unprojected along the unit rays of K^-1 (:25-36), cut at a planar depth of 5 m, z negated (the camera
// looks down -z, +x right, +y up), moved to the world frame.  Restated here as a primary-ray caster against a triangle
// soup; B scenes x V cameras in one sync-free call.  Contract and arithmetic: include/s4g_ops.h (s4g_render_views_f32).
//
//   setup    one thread per (view, triangle): camera-frame vertices R^T (p - c) in double, the edge vectors, the two
//            ray-independent Moeller-Trumbore terms (the ray origin is 0: Q = -v0 x e1 and Tn = e2 . Q), and a
//            conservative screen box in pixels (all three vertices at depth <= 0: none; any: the image; else the
//            projected extent widened by one pixel).  One workgroup = one chunk of RV_CHUNK triangles, whose boxes'
//            union is kept too (integer LDS atomics: a minimum does not depend on their order);
//   cast     one workgroup per RV_TILE x RV_TILE pixel tile.  Chunks whose union box misses the tile are skipped; of
//            the others every thread tests one triangle's box, and an ordered ballot compaction appends the survivors
//            to an LDS list (ascending triangle index), which every pixel thread walks when it fills and at the end.
//            The nearest hit is a per-thread (t, index) minimum with a strict <: the lowest index wins a tie, and no
//            result depends on an arrival order.  No per-tile list in global memory: no capacity, no overflow path;
//   compact  kept pixels in ascending pixel index: per-segment counts, one workgroup per view scans them, a second
//            ordered ballot writes the points, the pixel indices and the padding.
// A culled triangle could not have been hit (the box is wider than the rounding of the projection by a pixel), so the
// dense maps equal a scan of every triangle per pixel.
#include <limits.h>
#include <math.h>

#include <cmath>

#include "s4g_common.h"

namespace s4g {

constexpr int RV_TILE = 16;                      // pixels per tile edge
constexpr int RV_THREADS = RV_TILE * RV_TILE;    // one thread per pixel of the tile
constexpr int RV_CHUNK = 256;                    // triangles per box chunk: one per thread of a round
constexpr int RV_CAP = 384;                      // LDS survivor list; flushed when a further chunk might not fit (41 KB
                                                 // with the indices: three workgroups per CU)
constexpr int RV_REC = 13;                       // doubles per triangle record: v0, e1, e2, Q, Tn
constexpr int RV_SEG = 256;                      // pixels per compaction segment
constexpr int64_t RV_MAX_VIEWS = 65535;
constexpr int64_t RV_MAX_PIXELS = 1ll << 22;
constexpr int64_t RV_MAX_TRIANGLES = 1ll << 24;  // exclusive

static_assert(RV_CHUNK == RV_THREADS, "a round of the cast kernel tests one box per thread");
static_assert(RV_CAP >= RV_CHUNK, "an empty list takes a whole chunk");
static_assert(RV_SEG == 256 && RV_THREADS == 256, "four waves per workgroup");

struct RvWs {
  double* rec;      // [BV * T * RV_REC]
  int4* box;        // [BV * T] (x0, x1, y0, y1) inclusive pixel ranges; x0 > x1: culled
  int4* cbox;       // [BV * chunks] the union of a chunk's boxes
  int* seg_count;   // [BV * segs]
  int* seg_base;    // [BV * segs] kept pixels of the view in front of the segment
};

static size_t rv_align(size_t v) { return (v + 255) & ~(size_t)255; }

static size_t rv_ws(void* base, int64_t BV, int64_t T, int64_t P, RvWs* w) {
  char* p = (char*)base;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* r = p ? p + off : nullptr;
    off += rv_align(bytes);
    return r;
  };
  const size_t chunks = (size_t)((T + RV_CHUNK - 1) / RV_CHUNK), segs = (size_t)((P + RV_SEG - 1) / RV_SEG);
  RvWs t;
  t.rec = (double*)take((size_t)BV * (size_t)T * RV_REC * sizeof(double));
  t.box = (int4*)take((size_t)BV * (size_t)T * sizeof(int4));
  t.cbox = (int4*)take((size_t)BV * chunks * sizeof(int4));
  t.seg_count = (int*)take((size_t)BV * segs * sizeof(int));
  t.seg_base = (int*)take((size_t)BV * segs * sizeof(int));
  if (w) *w = t;
  return off + 256;   // never 0 for a shape inside the limits
}

static bool rv_shape_ok(int64_t B, int64_t V, int64_t T, int64_t H, int64_t W) {
  if (B < 0 || V < 0 || T < 0 || T >= RV_MAX_TRIANGLES) return false;
  if (B > RV_MAX_VIEWS || V > RV_MAX_VIEWS || B * V > RV_MAX_VIEWS) return false;
  if (H <= 0 || W <= 0 || H > RV_MAX_PIXELS || W > RV_MAX_PIXELS || H * W > RV_MAX_PIXELS) return false;
  return true;
}

// lowest / highest pixel index whose centre can lie in [lo, hi] (pixel coordinates), widened by one pixel and cut to
// [0, n - 1]; anything that does not compare (NaN) takes the whole axis
__device__ __forceinline__ void rv_extent(double lo, double hi, int n, int& i0, int& i1) {
  const double a = floor(lo) - 1.0, b = floor(hi) + 1.0;
  i0 = !(a >= 0.0) ? 0 : (a > (double)n ? n : (int)a);
  i1 = !(b <= (double)(n - 1)) ? n - 1 : (b < -1.0 ? -1 : (int)b);
}

__global__ __launch_bounds__(RV_CHUNK) void rv_setup_kernel(const float* __restrict__ tri_bt9,
                                                            const int32_t* __restrict__ tri_count_b,
                                                            const double* __restrict__ cam_bv12, int V, int T,
                                                            int chunks, double fx, double fy, double cx, double cy,
                                                            int H, int W, RvWs ws) {
  __shared__ int bb[4];
  const int bv = blockIdx.y, b = bv / V, chunk = blockIdx.x, t = threadIdx.x;
  if (t == 0) {
    bb[0] = INT_MAX;
    bb[1] = -1;
    bb[2] = INT_MAX;
    bb[3] = -1;
  }
  __syncthreads();
  int n = T;
  if (tri_count_b) {
    n = tri_count_b[b];
    n = n < 0 ? 0 : (n > T ? T : n);
  }
  const int k = chunk * RV_CHUNK + t;
  if (k < T) {
    int4 box = make_int4(INT_MAX, -1, INT_MAX, -1);
    if (k < n) {   // rows at or past the count are never read
      const double* __restrict__ cam = cam_bv12 + (size_t)bv * 12;
      const float* __restrict__ p = tri_bt9 + ((size_t)b * T + k) * 9;
      double v[3][3];
      bool ok = true;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double d0 = (double)p[3 * j] - cam[9], d1 = (double)p[3 * j + 1] - cam[10],
                     d2 = (double)p[3 * j + 2] - cam[11];
#pragma unroll
        for (int i = 0; i < 3; ++i) {   // R^T (p - c): column i of R
          v[j][i] = cam[i] * d0 + cam[3 + i] * d1 + cam[6 + i] * d2;
          ok = ok && finite(v[j][i]);
        }
      }
      if (ok) {
        const double z0 = -v[0][2], z1 = -v[1][2], z2 = -v[2][2];   // depths along the viewing direction
        const int behind = (z0 <= 0.0 ? 1 : 0) + (z1 <= 0.0 ? 1 : 0) + (z2 <= 0.0 ? 1 : 0);
        if (behind == 0) {
          const double x0 = cx + fx * (v[0][0] / z0), x1 = cx + fx * (v[1][0] / z1), x2 = cx + fx * (v[2][0] / z2);
          const double y0 = cy + fy * (v[0][1] / z0), y1 = cy + fy * (v[1][1] / z1), y2 = cy + fy * (v[2][1] / z2);
          rv_extent(fmin(x0, fmin(x1, x2)), fmax(x0, fmax(x1, x2)), W, box.x, box.y);
          rv_extent(fmin(y0, fmin(y1, y2)), fmax(y0, fmax(y1, y2)), H, box.z, box.w);
        } else if (behind < 3) {
          box = make_int4(0, W - 1, 0, H - 1);
        }
      }
      if (box.x <= box.y && box.z <= box.w) {
        double* __restrict__ r = ws.rec + ((size_t)bv * T + k) * RV_REC;
        const double ax = v[0][0], ay = v[0][1], az = v[0][2];
        const double e1x = v[1][0] - ax, e1y = v[1][1] - ay, e1z = v[1][2] - az;
        const double e2x = v[2][0] - ax, e2y = v[2][1] - ay, e2z = v[2][2] - az;
        // Q = (0 - v0) x e1
        const double qx = -(ay * e1z - az * e1y), qy = -(az * e1x - ax * e1z), qz = -(ax * e1y - ay * e1x);
        r[0] = ax, r[1] = ay, r[2] = az;
        r[3] = e1x, r[4] = e1y, r[5] = e1z;
        r[6] = e2x, r[7] = e2y, r[8] = e2z;
        r[9] = qx, r[10] = qy, r[11] = qz;
        r[12] = e2x * qx + e2y * qy + e2z * qz;
        atomicMin(&bb[0], box.x);
        atomicMax(&bb[1], box.y);
        atomicMin(&bb[2], box.z);
        atomicMax(&bb[3], box.w);
      } else {
        box = make_int4(INT_MAX, -1, INT_MAX, -1);
      }
    }
    ws.box[(size_t)bv * T + k] = box;
  }
  __syncthreads();
  if (t == 0) ws.cbox[(size_t)bv * chunks + chunk] = make_int4(bb[0], bb[1], bb[2], bb[3]);
}

// One triangle against the ray (rx, ry, -1) from the origin: Moeller-Trumbore scaled by the determinant, no division in
// a decision.  Both faces; det == 0 and non-finite terms never hit; a strict < keeps the earlier (lower) index on a tie.
__device__ __forceinline__ void rv_test(const double* __restrict__ q, int idx, double rx, double ry, double& best_t,
                                        int& best_i) {
  const double px = ry * q[8] + q[7];             // P = r x e2, r.z = -1
  const double py = -q[6] - rx * q[8];
  const double pz = rx * q[7] - ry * q[6];
  const double det = q[3] * px + q[4] * py + q[5] * pz;
  const double U = -(q[0] * px + q[1] * py + q[2] * pz);
  const double Vv = rx * q[9] + ry * q[10] - q[11];
  const double Tn = q[12];
  bool hit;
  if (det > 0.0)
    hit = U >= 0.0 && Vv >= 0.0 && U + Vv <= det && Tn > 0.0;
  else
    hit = det < 0.0 && U <= 0.0 && Vv <= 0.0 && U + Vv >= det && Tn < 0.0;
  if (hit && finite(det) && finite(U) && finite(Vv) && finite(Tn)) {
    const double t = Tn / det;
    if (t < best_t) {
      best_t = t;
      best_i = idx;
    }
  }
}

__global__ __launch_bounds__(RV_THREADS) void rv_cast_kernel(int T, int chunks, int tiles_x, double fx, double fy,
                                                             double cx, double cy, int H, int W, RvWs ws,
                                                             float* __restrict__ range_bvp,
                                                             int32_t* __restrict__ tri_bvp) {
  __shared__ double s_rec[RV_CAP * RV_REC];
  __shared__ int s_idx[RV_CAP];
  __shared__ int wave_cnt[RV_THREADS / 64];
  const int bv = blockIdx.y;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int t = threadIdx.x, wave = t >> 6;
  const int tx0 = tx * RV_TILE, tx1 = tx0 + RV_TILE - 1, ty0 = ty * RV_TILE, ty1 = ty0 + RV_TILE - 1;
  const int col = tx0 + (t & (RV_TILE - 1)), row = ty0 + t / RV_TILE;
  const bool active = col < W && row < H;
  const double rx = ((double)col + 0.5 - cx) / fx, ry = ((double)row + 0.5 - cy) / fy;
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  double best_t = inf;
  int best_i = -1;
  const int4* __restrict__ box = ws.box + (size_t)bv * T;
  const int4* __restrict__ cbox = ws.cbox + (size_t)bv * chunks;
  const double* __restrict__ rec = ws.rec + (size_t)bv * T * RV_REC;
  int n = 0;   // survivors in the list: the same value in every thread
  for (int c = 0; c < chunks; ++c) {
    const int4 cb = cbox[c];
    // the workgroup's own decision: one address, one value
    const int skip = __builtin_amdgcn_readfirstlane((cb.x > tx1 || cb.y < tx0 || cb.z > ty1 || cb.w < ty0) ? 1 : 0);
    if (skip) continue;
    const int k = c * RV_CHUNK + t;
    bool keep = false;
    if (k < T) {
      const int4 bx = box[k];
      keep = bx.x <= tx1 && bx.y >= tx0 && bx.z <= ty1 && bx.w >= ty0;
    }
    const uint64_t m = __ballot(keep);
    if ((t & 63) == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < RV_THREADS / 64; ++w) {
      const int cnt = wave_cnt[w];
      before += w < wave ? cnt : 0;
      total += cnt;
    }
    if (keep) {
      const int pos = n + before + mask_rank(m);   // < n + RV_CHUNK <= RV_CAP
      const double* __restrict__ src = rec + (size_t)k * RV_REC;
#pragma unroll
      for (int j = 0; j < RV_REC; ++j) s_rec[pos * RV_REC + j] = src[j];
      s_idx[pos] = k;
    }
    n = __builtin_amdgcn_readfirstlane(n + total);
    __syncthreads();
    if (n > RV_CAP - RV_CHUNK) {   // the next chunk might not fit
      if (active)
        for (int s = 0; s < n; ++s) rv_test(s_rec + s * RV_REC, s_idx[s], rx, ry, best_t, best_i);
      n = 0;
      __syncthreads();
    }
  }
  if (active) {
    for (int s = 0; s < n; ++s) rv_test(s_rec + s * RV_REC, s_idx[s], rx, ry, best_t, best_i);
    const size_t o = (size_t)bv * H * W + (size_t)row * W + col;
    const double nor = sqrt(rx * rx + ry * ry + 1.0);
    range_bvp[o] = best_i >= 0 ? (float)(best_t * nor) : __int_as_float(0x7f800000);
    tri_bvp[o] = best_i;
  }
}

// Pixel i of a view: whether it is kept, its stored range and the unit direction of its ray.
__device__ __forceinline__ bool rv_pixel(int i, int W, double fx, double fy, double cx, double cy, double max_depth,
                                         const float* __restrict__ range, const int32_t* __restrict__ tri, double& r,
                                         double& dx, double& dy, double& dz) {
  const int row = i / W, col = i - row * W;
  const double rx = ((double)col + 0.5 - cx) / fx, ry = ((double)row + 0.5 - cy) / fy;
  const double nor = sqrt(rx * rx + ry * ry + 1.0);
  dx = rx / nor;
  dy = ry / nor;
  dz = 1.0 / nor;
  r = (double)range[i];
  return tri[i] >= 0 && r * dz < max_depth;
}

__global__ __launch_bounds__(RV_SEG) void rv_count_kernel(int P, int segs, double fx, double fy, double cx, double cy,
                                                          double max_depth, int W, const float* __restrict__ range_bvp,
                                                          const int32_t* __restrict__ tri_bvp, RvWs ws) {
  __shared__ int wave_cnt[RV_SEG / 64];
  const int bv = blockIdx.y, i = blockIdx.x * RV_SEG + threadIdx.x;
  bool keep = false;
  if (i < P) {
    double r, dx, dy, dz;
    keep = rv_pixel(i, W, fx, fy, cx, cy, max_depth, range_bvp + (size_t)bv * P, tri_bvp + (size_t)bv * P, r, dx, dy,
                    dz);
  }
  const uint64_t m = __ballot(keep);
  if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0)
    ws.seg_count[(size_t)bv * segs + blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// One workgroup per view: exclusive scan of its segment counts (thread t owns a run of consecutive segments).
__global__ __launch_bounds__(RV_SEG) void rv_scan_kernel(int segs, RvWs ws, int32_t* __restrict__ count_bv) {
  __shared__ uint32_t wave_sum[RV_SEG / 64];
  const int bv = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int* __restrict__ cnt = ws.seg_count + (size_t)bv * segs;
  int* __restrict__ base = ws.seg_base + (size_t)bv * segs;
  const int per = (segs + RV_SEG - 1) / RV_SEG;
  const int lo = min(t * per, segs), hi = min(lo + per, segs);
  uint32_t own = 0;
  for (int s = lo; s < hi; ++s) own += (uint32_t)cnt[s];
  const uint32_t inc = wave_inclusive_scan_u32(own);
  if (lane == 63) wave_sum[wave] = inc;
  __syncthreads();
  uint32_t run = inc - own, total = 0;
#pragma unroll
  for (int w = 0; w < RV_SEG / 64; ++w) {
    run += w < wave ? wave_sum[w] : 0u;
    total += wave_sum[w];
  }
  for (int s = lo; s < hi; ++s) {
    base[s] = (int)run;
    run += (uint32_t)cnt[s];
  }
  if (t == 0) count_bv[bv] = (int)total;
}

__global__ __launch_bounds__(RV_SEG) void rv_write_kernel(int P, int segs, double fx, double fy, double cx, double cy,
                                                          double max_depth, int W,
                                                          const double* __restrict__ cam_bv12,
                                                          const double* __restrict__ noise_bvp,
                                                          const float* __restrict__ range_bvp,
                                                          const int32_t* __restrict__ tri_bvp, RvWs ws,
                                                          const int32_t* __restrict__ count_bv,
                                                          float* __restrict__ points_bv3p,
                                                          float* __restrict__ noisy_bv3p,
                                                          int32_t* __restrict__ pixel_bvp) {
  __shared__ int wave_cnt[RV_SEG / 64];
  const int bv = blockIdx.y, t = threadIdx.x, wave = t >> 6, i = blockIdx.x * RV_SEG + t;
  const double* __restrict__ cam = cam_bv12 + (size_t)bv * 12;
  bool keep = false;
  double r = 0.0, dx = 0.0, dy = 0.0, dz = 0.0;
  if (i < P)
    keep = rv_pixel(i, W, fx, fy, cx, cy, max_depth, range_bvp + (size_t)bv * P, tri_bvp + (size_t)bv * P, r, dx, dy,
                    dz);
  const uint64_t m = __ballot(keep);
  if ((t & 63) == 0) wave_cnt[wave] = __popcll(m);
  __syncthreads();
  int before = 0;
#pragma unroll
  for (int w = 0; w < RV_SEG / 64; ++w) before += w < wave ? wave_cnt[w] : 0;
  float* __restrict__ pts = points_bv3p + (size_t)bv * 3 * P;
  float* __restrict__ nsy = noisy_bv3p ? noisy_bv3p + (size_t)bv * 3 * P : nullptr;
  int32_t* __restrict__ pix = pixel_bvp + (size_t)bv * P;
  if (keep) {
    const int pos = ws.seg_base[(size_t)bv * segs + blockIdx.x] + before + mask_rank(m);   // <= i < P
    if (pos >= 0 && pos < P) {   // (cannot be otherwise: the counts are this call's own)
      const double x = r * dx, y = r * dy, z = -(r * dz);
      pts[pos] = (float)(cam[0] * x + cam[1] * y + cam[2] * z + cam[9]);
      pts[(size_t)P + pos] = (float)(cam[3] * x + cam[4] * y + cam[5] * z + cam[10]);
      pts[2 * (size_t)P + pos] = (float)(cam[6] * x + cam[7] * y + cam[8] * z + cam[11]);
      if (nsy) {
        const double rn = r * noise_bvp[(size_t)bv * P + i];
        const double xn = rn * dx, yn = rn * dy, zn = -(rn * dz);
        nsy[pos] = (float)(cam[0] * xn + cam[1] * yn + cam[2] * zn + cam[9]);
        nsy[(size_t)P + pos] = (float)(cam[3] * xn + cam[4] * yn + cam[5] * zn + cam[10]);
        nsy[2 * (size_t)P + pos] = (float)(cam[6] * xn + cam[7] * yn + cam[8] * zn + cam[11]);
      }
      pix[pos] = i;
    }
  }
  int kept = count_bv[bv];
  kept = kept < 0 ? 0 : kept;
  if (i < P && i >= kept) {   // the padding behind the view's kept pixels
    const float nan = __int_as_float(0x7fc00000);
    pts[i] = nan;
    pts[(size_t)P + i] = nan;
    pts[2 * (size_t)P + i] = nan;
    if (nsy) {
      nsy[i] = nan;
      nsy[(size_t)P + i] = nan;
      nsy[2 * (size_t)P + i] = nan;
    }
    pix[i] = -1;
  }
}

}  // namespace s4g

extern "C" size_t s4g_render_views_workspace_bytes(int64_t B, int64_t V, int64_t T, int64_t H, int64_t W) {
  if (!s4g::rv_shape_ok(B, V, T, H, W)) return 0;
  return s4g::rv_ws(nullptr, B * V, T, H * W, nullptr);
}

extern "C" int s4g_render_views_f32(const float* tri_bt9, const int32_t* tri_count_b, const double* cam_bv12, int64_t B,
                                    int64_t V, int64_t T, double fx, double fy, double cx, double cy, double max_depth,
                                    int64_t H, int64_t W, const double* noise_bvp, float* range_bvp, int32_t* tri_bvp,
                                    float* points_bv3p, float* noisy_bv3p, int32_t* pixel_bvp, int32_t* count_bv,
                                    void* ws, size_t ws_bytes, s4g_stream_t stream) {
  using namespace s4g;
  if (!rv_shape_ok(B, V, T, H, W)) return S4G_EINVAL;
  if (!(fx > 0.0) || !(fy > 0.0) || !std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) ||
      !std::isfinite(cy))
    return S4G_EINVAL;
  const int64_t BV = B * V, P = H * W;
  if (BV == 0) return S4G_OK;
  if (!cam_bv12 || !range_bvp || !tri_bvp || !points_bv3p || !pixel_bvp || !count_bv) return S4G_EINVAL;
  if (T > 0 && !tri_bt9) return S4G_EINVAL;
  if (noise_bvp && !noisy_bv3p) return S4G_EINVAL;
  if (!ws || ws_bytes < rv_ws(nullptr, BV, T, P, nullptr)) return S4G_EWORKSPACE;
  RvWs w;
  rv_ws(ws, BV, T, P, &w);
  hipStream_t st = (hipStream_t)stream;
  const int chunks = (int)((T + RV_CHUNK - 1) / RV_CHUNK), segs = (int)((P + RV_SEG - 1) / RV_SEG);
  const int tiles_x = (int)((W + RV_TILE - 1) / RV_TILE), tiles_y = (int)((H + RV_TILE - 1) / RV_TILE);
  if (chunks > 0) {
    hipLaunchKernelGGL(rv_setup_kernel, dim3((unsigned)chunks, (unsigned)BV), dim3(RV_CHUNK), 0, st, tri_bt9,
                       tri_count_b, cam_bv12, (int)V, (int)T, chunks, fx, fy, cx, cy, (int)H, (int)W, w);
    S4G_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(rv_cast_kernel, dim3((unsigned)tiles_x * (unsigned)tiles_y, (unsigned)BV), dim3(RV_THREADS), 0, st,
                     (int)T, chunks, tiles_x, fx, fy, cx, cy, (int)H, (int)W, w, range_bvp, tri_bvp);
  S4G_LAUNCH_CHECK();
  hipLaunchKernelGGL(rv_count_kernel, dim3((unsigned)segs, (unsigned)BV), dim3(RV_SEG), 0, st, (int)P, segs, fx, fy, cx,
                     cy, max_depth, (int)W, range_bvp, tri_bvp, w);
  S4G_LAUNCH_CHECK();
  hipLaunchKernelGGL(rv_scan_kernel, dim3((unsigned)BV), dim3(RV_SEG), 0, st, segs, w, count_bv);
  S4G_LAUNCH_CHECK();
  hipLaunchKernelGGL(rv_write_kernel, dim3((unsigned)segs, (unsigned)BV), dim3(RV_SEG), 0, st, (int)P, segs, fx, fy, cx,
                     cy, max_depth, (int)W, cam_bv12, noise_bvp, range_bvp, tri_bvp, w, count_bv, points_bv3p,
                     noise_bvp ? noisy_bv3p : nullptr, pixel_bvp);
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}
