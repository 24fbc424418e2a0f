// Darboux frames of the data generator's label search for every frame row of every scene:
// TorchSingleViewPointCloud._estimate_frame (data_gen/pcd_classes/torch_single_view_point_cloud.py:107-133), which
// estimate_frames (:98-105) loops over the sampled points with one kd-tree radius query and one eigh each.
// Contract: include/s4g_ops.h (s4g_darboux_frames_f32).
//
// Neighbourhood: the toroidal cell grid of grid.h with the cell edge just above the radius (as the ball query and
// the radius outlier filter build it), so a frame reads the 27 cells around its point.  The build places a cell's
// records by LDS atomics, in an order that changes from run to run; darboux_order_kernel rewrites every cell in
// ascending point index, with the record's normal next to it, into a compact copy.  Every sum below then runs in a
// fixed order that depends on the scene alone: run-to-run bit-identical and batch invariant without atomics.
// A scene outside the grid's exactness range (grid.h, flags[b]) or above GR_MAX_POINTS is scanned in index order:
// the same neighbour sets, sums in another order.
//
// Per frame, one thread, two passes over the neighbours (no list, no cap): count and normal sum, then the
// deviations' second moments.  Both are accumulated in double -- on a near-flat patch the two small eigenvalues are
// 1e-3 of the large one and the deviations are differences of nearly equal fp32 numbers -- and the covariance is
// rounded to fp32 once, scaled by its trace.  The eigen-solve is cyclic Jacobi in fp32 (DB_SWEEPS sweeps, the count
// fixed), the frame is formed from its eigenvector in double and rounded once.
#include "grid.h"

namespace s4g {

constexpr int DB_THREADS = 128;
constexpr int DB_SWEEPS = 6;
constexpr int DB_ORDER_THREADS = 256;

struct DarbouxWs {
  GridWs grid;
  float4* rec;   // [B][N] (x, y, z, index bits): cell after cell in the grid's record order, ascending index within a cell
  float4* nrm;   // [B][N] the records' normals (x, y, z, 0)
  int* shift;    // [B][GR_RANGES] record offset in the grid's `sorted` minus the offset in `rec`
};

static size_t db_align(size_t v) { return (v + 255) & ~(size_t)255; }

static size_t darboux_ws(void* base, int64_t B, int64_t N, DarbouxWs* w) {
  if (N > GR_MAX_POINTS || N <= 0) return 0;
  char* p = (char*)base;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* r = p ? p + off : nullptr;
    off += db_align(bytes);
    return r;
  };
  void* g = take(grid_ws_bytes(B, N));
  float4* rec = (float4*)take((size_t)B * N * sizeof(float4));
  float4* nrm = (float4*)take((size_t)B * N * sizeof(float4));
  int* shift = (int*)take((size_t)B * GR_RANGES * sizeof(int));
  if (w && p) {
    w->grid = grid_ws_carve(g, B, N);
    w->rec = rec;
    w->nrm = nrm;
    w->shift = shift;
  }
  return off;
}

// One thread per record of the grid: its place in the compact copy = the records of the stripes in front, the cells
// of its stripe in front, and the records of its own cell with a smaller point index.  The rank is a linear pass over
// the cell: quadratic in a cell's population, like the frames' own reads of that cell (include/s4g_ops.h, "Cost").
__global__ __launch_bounds__(DB_ORDER_THREADS) void darboux_order_kernel(
    const float* __restrict__ xyz, const float* __restrict__ normals, int N, float inv_h, DarbouxWs ws) {
  const int b = blockIdx.z, g = blockIdx.y;
  if (ws.grid.flags[b] != 0) return;  // out of the exactness range: the frames of this scene scan
  const int* __restrict__ st0 = ws.grid.starts + (size_t)b * GR_RANGES * GR_START_STRIDE;
  const int* __restrict__ st = st0 + g * GR_START_STRIDE;
  int base = 0;  // records of the stripes in front of g
  for (int r = 0; r < g; ++r) base += st0[r * GR_START_STRIDE + GR_RANGE_SLOTS] - r * N;
  if (blockIdx.x == 0 && threadIdx.x == 0) ws.shift[b * GR_RANGES + g] = g * N - base;
  const int q = blockIdx.x * DB_ORDER_THREADS + threadIdx.x;
  const int cnt = st[GR_RANGE_SLOTS] - g * N;
  if (q >= cnt) return;
  const float4* __restrict__ src = ws.grid.sorted + (size_t)b * GR_RANGES * N;
  const float4 me = src[g * N + q];
  const float* __restrict__ p0 = xyz + (size_t)b * 3 * N;
  const float ox = p0[0], oy = p0[N], oz = p0[2 * (size_t)N];
  const int slot = grid_slot(grid_coord(me.x, ox, inv_h), grid_coord(me.y, oy, inv_h),
                             grid_coord(me.z, oz, inv_h)) & (GR_RANGE_SLOTS - 1);
  const int lo = st[slot], hi = st[slot + 1];
  const int mine = __float_as_int(me.w);
  int rank = 0;
  for (int i = lo; i < hi; ++i) rank += __float_as_int(src[i].w) < mine ? 1 : 0;
  const int dst = base + (lo - g * N) + rank;
  if (dst < 0 || dst >= N || mine < 0 || mine >= N) return;  // (cannot happen: the slot is the build's own)
  const float* __restrict__ n0 = normals + (size_t)b * 3 * N;
  ws.rec[(size_t)b * N + dst] = me;
  ws.nrm[(size_t)b * N + dst] = make_float4(n0[mine], n0[N + mine], n0[2 * (size_t)N + mine], 0.f);
}

// One Jacobi rotation of the symmetric 3x3 matrix in the (p, q) plane; r is the third index.  v?p / v?q are the
// columns p and q of the eigenvector matrix.  An off-diagonal of 0 is left alone; theta overflowing gives t = 0.
__device__ __forceinline__ void jacobi_rotate(float& app, float& aqq, float& apq, float& arp, float& arq, float& v0p,
                                              float& v0q, float& v1p, float& v1q, float& v2p, float& v2q) {
  if (apq == 0.f) return;
  const float theta = (aqq - app) / (2.f * apq);
  float t = 1.f / (fabsf(theta) + sqrtf(theta * theta + 1.f));
  if (theta < 0.f) t = -t;
  const float c = 1.f / sqrtf(t * t + 1.f), s = t * c;
  app = app - t * apq;
  aqq = aqq + t * apq;
  apq = 0.f;
  const float rp = c * arp - s * arq, rq = s * arp + c * arq;
  arp = rp;
  arq = rq;
  float a = c * v0p - s * v0q, d = s * v0p + c * v0q;
  v0p = a; v0q = d;
  a = c * v1p - s * v1q; d = s * v1p + c * v1q;
  v1p = a; v1q = d;
  a = c * v2p - s * v2q; d = s * v2p + c * v2q;
  v2p = a; v2q = d;
}

// fn(normal x, y, z) for every point of scene b at squared distance < r2 of (x, y, z), in an order fixed by the scene.
// LIM (the per-object frames): only the points whose index is below nlim are points.
template <bool LIM = false, typename Fn>
__device__ __forceinline__ void darboux_neighbours(bool grid, const DarbouxWs& ws, const float* __restrict__ p0,
                                                   const float* __restrict__ n0, int b, int N, float x, float y, float z,
                                                   float ox, float oy, float oz, float r2, float inv_h, Fn fn,
                                                   int nlim = 0) {
  if (grid) {
    const int icx = grid_coord(x, ox, inv_h), icy = grid_coord(y, oy, inv_h), icz = grid_coord(z, oz, inv_h);
    const float4* __restrict__ rec = ws.rec + (size_t)b * N;
    const float4* __restrict__ nrm = ws.nrm + (size_t)b * N;
    const int* __restrict__ starts = ws.grid.starts + (size_t)b * GR_RANGES * GR_START_STRIDE;
    const int* __restrict__ shift = ws.shift + b * GR_RANGES;
    for (int dz = -1; dz <= 1; ++dz)
      for (int dy = -1; dy <= 1; ++dy) {
        const int zz = (icz + dz) & 31, yy = (icy + dy) & 31;
        const int range = grid_range(yy, zz);
        const int* __restrict__ st = starts + range * GR_START_STRIDE + grid_local_row(yy, zz);
        const int sh = shift[range];
        const int x0 = (icx - 1) & 31;
        int b0 = st[x0], e0, b1 = 0, e1 = 0;   // the row's three x cells: one run, or two where it wraps
        if (x0 <= GR_DIM - 3) {
          e0 = st[x0 + 3];
        } else {
          e0 = st[GR_DIM];
          b1 = st[0];
          e1 = st[(x0 + 3) & 31];
        }
        for (int i = b0 - sh; i < e0 - sh; ++i) {
          const float4 q = rec[i];
          if (dist2<false>(x, y, z, q.x, q.y, q.z) < r2 && (!LIM || __float_as_int(q.w) < nlim)) {
            const float4 m = nrm[i];
            fn(m.x, m.y, m.z);
          }
        }
        for (int i = b1 - sh; i < e1 - sh; ++i) {
          const float4 q = rec[i];
          if (dist2<false>(x, y, z, q.x, q.y, q.z) < r2 && (!LIM || __float_as_int(q.w) < nlim)) {
            const float4 m = nrm[i];
            fn(m.x, m.y, m.z);
          }
        }
      }
  } else {
    const int n = LIM ? nlim : N;
    for (int i = 0; i < n; ++i)
      if (dist2<false>(x, y, z, p0[i], p0[N + i], p0[2 * (size_t)N + i]) < r2) fn(n0[i], n0[N + i], n0[2 * (size_t)N + i]);
  }
}

__global__ __launch_bounds__(DB_THREADS) void darboux_frames_kernel(
    const float* __restrict__ xyz, const float* __restrict__ normals, const int32_t* __restrict__ frame_index,
    const int64_t* __restrict__ frame_count, int N, int F, float r2, float inv_h, int min_neighbours, int have_grid,
    DarbouxWs ws, float* __restrict__ frames, float* __restrict__ points, int32_t* __restrict__ count,
    int32_t* __restrict__ flags) {
  const int b = blockIdx.y;
  const int f = blockIdx.x * DB_THREADS + threadIdx.x;
  if (f >= F) return;
  const size_t row = (size_t)b * F + f;
  float* __restrict__ fr = frames + row * 9;
  float* __restrict__ pt = points + row * 3;
  const int i = frame_index[row];
  const bool live = i >= 0 && i < N && (!frame_count || (int64_t)f < frame_count[b]);
  float o[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float px = 0.f, py = 0.f, pz = 0.f;
  int k = 0, flag = 0;
  if (live) {
    const float* __restrict__ p0 = xyz + (size_t)b * 3 * N;
    const float* __restrict__ n0 = normals + (size_t)b * 3 * N;
    px = p0[i]; py = p0[N + i]; pz = p0[2 * (size_t)N + i];
    const float nxf = n0[i], nyf = n0[N + i], nzf = n0[2 * (size_t)N + i];
    // a point or normal that is not finite still counts its neighbours (none, for a point that is not finite)
    const bool own_bad = !(finite(px) && finite(py) && finite(pz) && finite(nxf) && finite(nyf) &&
                           finite(nzf));
    const float ox = p0[0], oy = p0[N], oz = p0[2 * (size_t)N];
    const bool grid = have_grid && ws.grid.flags[b] == 0 && grid_coord_ok(px, ox, inv_h) &&
                      grid_coord_ok(py, oy, inv_h) && grid_coord_ok(pz, oz, inv_h);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    darboux_neighbours(grid, ws, p0, n0, b, N, px, py, pz, ox, oy, oz, r2, inv_h, [&](float ax, float ay, float az) __attribute__((always_inline)) {
      ++k;
      sx += (double)ax;
      sy += (double)ay;
      sz += (double)az;
    });
    const double nx = (double)nxf, ny = (double)nyf, nz = (double)nzf;
    if (own_bad || !(fabs(sx) <= 1.7e308 && fabs(sy) <= 1.7e308 && fabs(sz) <= 1.7e308)) {
      flag = 2;                       // the point, its normal or a neighbour's normal is not finite
    } else if (k < min_neighbours) {
      o[0] = o[4] = o[8] = 1.f;       // :118-120, the frame stays the identity
    } else {
      // :122-124 -- the MEAN is projected off the normal, the neighbours' normals are not
      const double mx = sx / (double)k, my = sy / (double)k, mz = sz / (double)k;
      const double mn = mx * nx + my * ny + mz * nz;
      const double cx = mx - nx * mn, cy = my - ny * mn, cz = mz - nz * mn;
      double cxx = 0.0, cxy = 0.0, cxz = 0.0, cyy = 0.0, cyz = 0.0, czz = 0.0;
      darboux_neighbours(grid, ws, p0, n0, b, N, px, py, pz, ox, oy, oz, r2, inv_h, [&](float ax, float ay, float az) __attribute__((always_inline)) {
        const double dx = (double)ax - cx, dy = (double)ay - cy, dz = (double)az - cz;
        cxx += dx * dx; cxy += dx * dy; cxz += dx * dz;
        cyy += dy * dy; cyz += dy * dz; czz += dz * dz;
      });
      const double tr = cxx + cyy + czz;
      const double sc = tr > 0.0 ? 1.0 / tr : 0.0;   // the eigenvectors do not depend on the scale
      float a00 = (float)(cxx * sc), a01 = (float)(cxy * sc), a02 = (float)(cxz * sc);
      float a11 = (float)(cyy * sc), a12 = (float)(cyz * sc), a22 = (float)(czz * sc);
      float v00 = 1.f, v01 = 0.f, v02 = 0.f, v10 = 0.f, v11 = 1.f, v12 = 0.f, v20 = 0.f, v21 = 0.f, v22 = 1.f;
      for (int s = 0; s < DB_SWEEPS; ++s) {
        jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
        jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
        jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
      }
      // the eigenvector of the smallest eigenvalue; the lowest column wins a tie
      double ex = (double)v00, ey = (double)v10, ez = (double)v20;
      float small = a00;
      if (a11 < small) { small = a11; ex = (double)v01; ey = (double)v11; ez = (double)v21; }
      if (a22 < small) { small = a22; ex = (double)v02; ey = (double)v12; ez = (double)v22; }
      // :128-130
      const double en = ex * nx + ey * ny + ez * nz;
      double ux = ex - en * nx, uy = ey - en * ny, uz = ez - en * nz;
      const double uu = ux * ux + uy * uy + uz * uz;
      if (!(uu >= 1e-12 && uu <= 1.7e308 && fabs(tr) <= 1.7e308)) {
        flag = 2;                     // the eigenvector is parallel to the normal, or something overflowed
      } else {
        // sign: the largest component of the unnormalised minor axis is positive, the lowest index wins a tie
        double lead = ux;
        if (fabs(uy) > fabs(lead)) lead = uy;
        if (fabs(uz) > fabs(lead)) lead = uz;
        const double inv = (lead < 0.0 ? -1.0 : 1.0) / sqrt(uu);
        ux *= inv; uy *= inv; uz *= inv;
        const double qx = uy * nz - uz * ny, qy = uz * nx - ux * nz, qz = ux * ny - uy * nx;   // minor x normal
        o[0] = (float)-nx; o[1] = (float)-qx; o[2] = (float)ux;                                // :132, axes as columns
        o[3] = (float)-ny; o[4] = (float)-qy; o[5] = (float)uy;
        o[6] = (float)-nz; o[7] = (float)-qz; o[8] = (float)uz;
        flag = 1;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 9; ++j) fr[j] = o[j];
  pt[0] = px; pt[1] = py; pt[2] = pz;
  count[row] = k;
  flags[row] = flag;
}

// The per-object frames of GenerateDarbouxObjectData._estimate_frame (data_gen/data_generator/
// data_object_darboux_generator.py:62-92): one thread per point of every object, over the same ordered grid.  It
// differs from the view class in three places, all kept as written: the normal is the normalised MEAN of the
// neighbours' normals (:73-74); the centroid is M @ mean with M = I - (n.n), a SCALAR taken off every entry of the
// identity (:80, the 1-D `normal.T @ normal`), so centroid_i = mean_i - (n.n) (mean_x + mean_y + mean_z); and below
// min_neighbours both frames are ZERO (:75-78).  frame = [-n, -principal, minor], inv_frame = [n, principal, minor].
__global__ __launch_bounds__(DB_THREADS) void darboux_object_frames_kernel(
    const float* __restrict__ xyz, const float* __restrict__ normals, const int64_t* __restrict__ obj_count, int N,
    float r2, float inv_h, int min_neighbours, DarbouxWs ws, float* __restrict__ frames, float* __restrict__ inv_frames,
    int32_t* __restrict__ count, int32_t* __restrict__ flags) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * DB_THREADS + threadIdx.x;
  if (i >= N) return;
  const size_t row = (size_t)b * N + i;
  const int nlim = obj_count ? (int)min((int64_t)N, max((int64_t)0, obj_count[b])) : N;
  float o[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int k = 0, flag = 0;
  if (i < nlim) {
    const float* __restrict__ p0 = xyz + (size_t)b * 3 * N;
    const float* __restrict__ n0 = normals + (size_t)b * 3 * N;
    const float px = p0[i], py = p0[N + i], pz = p0[2 * (size_t)N + i];
    const bool own_bad = !(finite(px) && finite(py) && finite(pz));
    const float ox = p0[0], oy = p0[N], oz = p0[2 * (size_t)N];
    const bool grid = ws.grid.flags[b] == 0 && grid_coord_ok(px, ox, inv_h) && grid_coord_ok(py, oy, inv_h) &&
                      grid_coord_ok(pz, oz, inv_h);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    darboux_neighbours<true>(grid, ws, p0, n0, b, N, px, py, pz, ox, oy, oz, r2, inv_h, [&](float ax, float ay, float az) __attribute__((always_inline)) {
      ++k;
      sx += (double)ax;
      sy += (double)ay;
      sz += (double)az;
    }, nlim);
    const double ss = sx * sx + sy * sy + sz * sz;
    if (own_bad || !(ss <= 1.7e308)) {
      flag = 2;                       // the point or a neighbour's normal is not finite
    } else if (k < min_neighbours) {
      flag = 4;                       // :75-78, both frames stay zero
    } else if (!(ss >= 1e-24)) {
      flag = 2;                       // the mean normal vanishes: :74 divides by zero
    } else {
      const double mx = sx / (double)k, my = sy / (double)k, mz = sz / (double)k;     // :73
      const double inv_m = 1.0 / sqrt(mx * mx + my * my + mz * mz);
      const double nx = mx * inv_m, ny = my * inv_m, nz = mz * inv_m;                   // :74
      const double nn = nx * nx + ny * ny + nz * nz;                                    // :80, the scalar
      const double off = nn * (mx + my + mz);                                           // :81
      const double cx = mx - off, cy = my - off, cz = mz - off;
      double cxx = 0.0, cxy = 0.0, cxz = 0.0, cyy = 0.0, cyz = 0.0, czz = 0.0;
      darboux_neighbours<true>(grid, ws, p0, n0, b, N, px, py, pz, ox, oy, oz, r2, inv_h, [&](float ax, float ay, float az) __attribute__((always_inline)) {
        const double dx = (double)ax - cx, dy = (double)ay - cy, dz = (double)az - cz;  // :82-83
        cxx += dx * dx; cxy += dx * dy; cxz += dx * dz;
        cyy += dy * dy; cyz += dy * dz; czz += dz * dz;
      }, nlim);
      const double tr = cxx + cyy + czz;
      const double sc = tr > 0.0 ? 1.0 / tr : 0.0;
      float a00 = (float)(cxx * sc), a01 = (float)(cxy * sc), a02 = (float)(cxz * sc);
      float a11 = (float)(cyy * sc), a12 = (float)(cyz * sc), a22 = (float)(czz * sc);
      float v00 = 1.f, v01 = 0.f, v02 = 0.f, v10 = 0.f, v11 = 1.f, v12 = 0.f, v20 = 0.f, v21 = 0.f, v22 = 1.f;
      for (int s = 0; s < DB_SWEEPS; ++s) {
        jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
        jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
        jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
      }
      double ex = (double)v00, ey = (double)v10, ez = (double)v20;
      float small = a00;
      if (a11 < small) { small = a11; ex = (double)v01; ey = (double)v11; ez = (double)v21; }
      if (a22 < small) { small = a22; ex = (double)v02; ey = (double)v12; ez = (double)v22; }
      const double en = ex * nx + ey * ny + ez * nz;                                    // :86
      double ux = ex - en * nx, uy = ey - en * ny, uz = ez - en * nz;
      const double uu = ux * ux + uy * uy + uz * uz;
      if (!(uu >= 1e-12 && uu <= 1.7e308 && fabs(tr) <= 1.7e308)) {
        flag = 2;
      } else {
        double lead = ux;             // the sign rule of darboux_frames_kernel
        if (fabs(uy) > fabs(lead)) lead = uy;
        if (fabs(uz) > fabs(lead)) lead = uz;
        const double inv = (lead < 0.0 ? -1.0 : 1.0) / sqrt(uu);
        ux *= inv; uy *= inv; uz *= inv;                                                // :87
        const double qx = uy * nz - uz * ny, qy = uz * nx - ux * nz, qz = ux * ny - uy * nx;   // :88
        o[0] = (float)nx; o[1] = (float)qx; o[2] = (float)ux;                           // :91, axes as columns
        o[3] = (float)ny; o[4] = (float)qy; o[5] = (float)uy;
        o[6] = (float)nz; o[7] = (float)qz; o[8] = (float)uz;
        flag = 1;
      }
    }
  }
  float* __restrict__ fr = frames + row * 9;
  float* __restrict__ iv = inv_frames + row * 9;
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    iv[j] = o[j];
    fr[j] = (j % 3 == 2 || flag != 1) ? o[j] : -o[j];                                   // :90 (a zero frame stays +0)
  }
  count[row] = k;
  flags[row] = flag;
}

}  // namespace s4g

extern "C" size_t s4g_darboux_object_frames_workspace_bytes(int64_t B, int64_t N) {
  if (B <= 0) return 0;
  return s4g::darboux_ws(nullptr, B, N, nullptr);
}

extern "C" int s4g_darboux_object_frames_f32(const float* xyz_b3n, const float* normals_b3n, const int64_t* count_b,
                                             int64_t B, int64_t N, float radius, int32_t min_neighbours,
                                             float* frames_bn33, float* inv_frames_bn33, int32_t* neighbours_bn,
                                             int32_t* flags_bn, void* workspace, size_t workspace_bytes,
                                             s4g_stream_t stream) {
  using namespace s4g;
  if (B < 0 || B > 65535 || N < 1 || N > GR_MAX_POINTS) return S4G_EINVAL;
  if (!(radius > 0.f) || !(radius < 1e18f) || min_neighbours < 1) return S4G_EINVAL;
  if (B == 0) return S4G_OK;
  if (!xyz_b3n || !normals_b3n || !frames_bn33 || !inv_frames_bn33 || !neighbours_bn || !flags_bn) return S4G_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const float r2 = radius * radius;
  const float h = radius * (1.0f + 1.0f / 256.0f);
  const float inv_h = 1.0f / h;
  DarbouxWs w = {};
  const size_t need = darboux_ws(workspace, B, N, nullptr);
  if (!workspace || workspace_bytes < need) return S4G_EWORKSPACE;
  darboux_ws(workspace, B, N, &w);
  if (int rc = launch_grid_build(xyz_b3n, B, N, inv_h, w.grid, st, false)) return rc;
  hipLaunchKernelGGL(darboux_order_kernel,
                     dim3((unsigned)((N + DB_ORDER_THREADS - 1) / DB_ORDER_THREADS), GR_RANGES, (unsigned)B),
                     dim3(DB_ORDER_THREADS), 0, st, xyz_b3n, normals_b3n, (int)N, inv_h, w);
  S4G_LAUNCH_CHECK();
  hipLaunchKernelGGL(darboux_object_frames_kernel, dim3((unsigned)((N + DB_THREADS - 1) / DB_THREADS), (unsigned)B),
                     dim3(DB_THREADS), 0, st, xyz_b3n, normals_b3n, count_b, (int)N, r2, inv_h, (int)min_neighbours, w,
                     frames_bn33, inv_frames_bn33, neighbours_bn, flags_bn);
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}

extern "C" size_t s4g_darboux_frames_workspace_bytes(int64_t B, int64_t N, int64_t F) {
  (void)F;
  if (B <= 0) return 0;
  return s4g::darboux_ws(nullptr, B, N, nullptr);
}

extern "C" int s4g_darboux_frames_f32(const float* xyz_b3n, const float* normals_b3n, const int32_t* frame_index_bf,
                                      const int64_t* frame_count_b, int64_t B, int64_t N, int64_t F, float radius,
                                      int32_t min_neighbours, float* frames_bf33, float* points_bf3, int32_t* count_bf,
                                      int32_t* flags_bf, void* workspace, size_t workspace_bytes, s4g_stream_t stream) {
  using namespace s4g;
  if (B < 0 || B > 65535 || N < 0 || N >= (1ll << 30) || F < 0 || F >= (1ll << 30)) return S4G_EINVAL;
  if (!(radius > 0.f) || !(radius < 1e18f) || min_neighbours < 1) return S4G_EINVAL;
  if (B == 0 || F == 0) return S4G_OK;
  if (!frame_index_bf || !frames_bf33 || !points_bf3 || !count_bf || !flags_bf) return S4G_EINVAL;
  if (N > 0 && (!xyz_b3n || !normals_b3n)) return S4G_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const float r2 = radius * radius;   // fp32 product, as for the ball query
  // cell edge slightly above the radius, as for the ball query (grid.h)
  const float h = radius * (1.0f + 1.0f / 256.0f);
  const float inv_h = 1.0f / h;
  DarbouxWs w = {};
  const size_t need = darboux_ws(workspace, B, N, nullptr);
  const int have_grid = need != 0;
  if (have_grid) {
    if (!workspace || workspace_bytes < need) return S4G_EWORKSPACE;
    darboux_ws(workspace, B, N, &w);
    if (int rc = launch_grid_build(xyz_b3n, B, N, inv_h, w.grid, st, false)) return rc;
    hipLaunchKernelGGL(darboux_order_kernel,
                       dim3((unsigned)((N + DB_ORDER_THREADS - 1) / DB_ORDER_THREADS), GR_RANGES, (unsigned)B),
                       dim3(DB_ORDER_THREADS), 0, st, xyz_b3n, normals_b3n, (int)N, inv_h, w);
    S4G_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(darboux_frames_kernel, dim3((unsigned)((F + DB_THREADS - 1) / DB_THREADS), (unsigned)B),
                     dim3(DB_THREADS), 0, st, xyz_b3n, normals_b3n, frame_index_bf, frame_count_b, (int)N, (int)F, r2,
                     inv_h, (int)min_neighbours, have_grid, w, frames_bf33, points_bf3, count_bf, flags_bf);
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}
