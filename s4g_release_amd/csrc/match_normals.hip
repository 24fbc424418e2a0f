// Scene-normal transfer of the data generator's label pipeline for every view point of every scene:
// TorchSingleViewPointCloud._find_normal (data_gen/pcd_classes/torch_single_view_point_cloud.py:135-150), which loops
// over the view with one kd-tree search_hybrid_vector_3d(radius, max_nn) each, then normalises and orients the cloud.
// Contract: include/s4g_ops.h (s4g_match_normals_f32).  s4g_match_nearest_f32 -- the max_nn = 1 search of
// TorchPrecomputedSingleViewPointCloud._find_match (torch_contact_single_view_point_cloud.py:142-150), the index alone --
// runs the same build and the same query loop and stops before the normals.
//
// Neighbourhood: a toroidal 64^3 cell grid over the SCENE (the keys; the queries are another set) with the cell edge
// just above the radius and the cell coordinates of grid.h, built with the library's own stable radix sort instead of
// the LDS bitmaps of the 32^3 grid -- so there is no limit on the number of scene points.  One sort of
// (scene << 18 | cell, point index) pairs serves up to MN_CHUNK scenes; being stable it leaves every cell in ascending
// point index.  The cell starts are an exclusive scan of the cells' populations (integer atomics: the counts do not
// depend on their order).  A compact copy holds the records (x, y, z, index) in sorted order.  A batch above MN_CHUNK
// scenes is served chunk after chunk on the same workspace.
//
// Per view point, one wave: the candidates of the 27 cells (nine rows of three x-adjacent cells: one run of records
// each, two where the row wraps), 64 at a time; a candidate inside the radius is the 64-bit key (fp32 bits of d^2,
// scene index) -- non-negative floats order as their bit patterns, the index makes every key distinct.  The wave
// keeps a list of at most 128 keys in LDS and a threshold, the max_nn-th smallest key seen so far: a batch is
// filtered against it by ballot, the survivors are appended, and a full list is cut back to its max_nn smallest by
// ranking every key against the list.  The kept set depends on the candidates as a SET only, so the grid and the
// index-order scan (a scene or a query outside the grid's exactness range) give the same keys in the same rank order.
// The kept normals are then summed in double by a fixed butterfly over the ranks: no atomics touch a sum, the order
// depends on the scene and the query alone -- run-to-run bit-identical and batch invariant, and identical between
// the grid and the scan.
#include "grid.h"
#include "radix_sort.h"

namespace s4g {

constexpr int MN_DIM = 64;                                 // cells per axis (toroidal)
constexpr int MN_CELL_BITS = 18;
constexpr int MN_CELLS = MN_DIM * MN_DIM * MN_DIM;         // 262 144
constexpr int MN_CHUNK = 256;                              // scenes per sort: 8 more key bits
constexpr int MN_MAX_NN = 64;
constexpr int MN_LIST = 128;                               // keys a wave buffers between two cuts
constexpr int MN_THREADS = 256, MN_WAVES = MN_THREADS / 64;
constexpr int MN_BUILD_THREADS = 256;

struct MatchWs {
  uint32_t *keys_a, *keys_b, *vals_a, *vals_b;   // [Bc * M] sort ping-pong; keys_b / vals_b hold the result
  void* sort;                                    // radix_sort_ws_bytes(Bc * M)
  int* count;                                    // [Bc * MN_CELLS + 1] cell populations (the last entry stays 0) ...
  int* flags;                                    // ... then [Bc] 1 = scene out of the exactness range -> scan (cleared together)
  int* start;                                    // [Bc * MN_CELLS + 1] record offsets, scene after scene
  void* scan;                                    // scan_ws_bytes(Bc * MN_CELLS + 1)
  float4* rec;                                   // [Bc * M] (x, y, z, index bits) in sorted order
};

static size_t mn_align(size_t v) { return (v + 255) & ~(size_t)255; }

// scenes one pass serves: the sort's keys hold 32 bits and the scan's offsets 31
static int64_t mn_chunk(int64_t B, int64_t M) {
  int64_t c = ((1ll << 31) - 1) / (M > 0 ? M : 1);
  if (c > MN_CHUNK) c = MN_CHUNK;
  if (c > B) c = B;
  return c < 1 ? 1 : c;
}

// 16-byte words that hold the populations of Bc scenes, the closing entry and the scene flags
static size_t mn_clear_int4(int64_t Bc) { return ((size_t)Bc * MN_CELLS + 1 + (size_t)Bc + 3) / 4; }

static size_t match_ws(void* base, int64_t Bc, int64_t M, MatchWs* w) {
  char* p = (char*)base;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* r = p ? p + off : nullptr;
    off += mn_align(bytes);
    return r;
  };
  const size_t n = (size_t)Bc * (size_t)M, cells = (size_t)Bc * MN_CELLS + 1;
  uint32_t* ka = (uint32_t*)take(n * 4);
  uint32_t* kb = (uint32_t*)take(n * 4);
  uint32_t* va = (uint32_t*)take(n * 4);
  uint32_t* vb = (uint32_t*)take(n * 4);
  void* sort = take(radix_sort_ws_bytes(n));
  int* count = (int*)take(mn_clear_int4(Bc) * sizeof(int4));
  int* start = (int*)take(cells * 4);
  void* scan = take(scan_ws_bytes(cells));
  float4* rec = (float4*)take(n * sizeof(float4));
  if (w && p) {
    w->keys_a = ka; w->keys_b = kb; w->vals_a = va; w->vals_b = vb;
    w->sort = sort;
    w->count = count;
    w->flags = count + cells;
    w->start = start;
    w->scan = scan;
    w->rec = rec;
  }
  return off;
}

__device__ __forceinline__ int mn_cell(int cx, int cy, int cz) {
  return ((cz & (MN_DIM - 1)) << 12) | ((cy & (MN_DIM - 1)) << 6) | (cx & (MN_DIM - 1));
}

// Clears the cell populations and the scene flags (a kernel of the call's own, so that a captured graph holds a plain
// chain of kernel nodes).
__global__ __launch_bounds__(MN_BUILD_THREADS) void match_clear_kernel(int4* __restrict__ p, size_t n4) {
  const size_t i = (size_t)blockIdx.x * MN_BUILD_THREADS + threadIdx.x;
  if (i < n4) p[i] = make_int4(0, 0, 0, 0);
}

// One thread per scene point: its sort key and its cell's population.  A point outside the exactness range of
// grid.h (or not finite) sends its scene to the scan; it still gets a key (cell 0) so that the sort stays whole.
__global__ __launch_bounds__(MN_BUILD_THREADS) void match_keys_kernel(const float* __restrict__ scene, int M,
                                                                      float inv_h, MatchWs ws) {
  const int b = blockIdx.y;
  const int j = blockIdx.x * MN_BUILD_THREADS + threadIdx.x;
  if (j >= M) return;
  const float* __restrict__ p0 = scene + (size_t)b * 3 * M;
  const float ox = p0[0], oy = p0[M], oz = p0[2 * (size_t)M];
  const float x = p0[j], y = p0[M + j], z = p0[2 * (size_t)M + j];
  int cell = 0;
  if (grid_coord_ok(x, ox, inv_h) && grid_coord_ok(y, oy, inv_h) && grid_coord_ok(z, oz, inv_h))
    cell = mn_cell(grid_coord(x, ox, inv_h), grid_coord(y, oy, inv_h), grid_coord(z, oz, inv_h));
  else
    ws.flags[b] = 1;
  const size_t i = (size_t)b * M + j;
  ws.keys_a[i] = ((uint32_t)b << MN_CELL_BITS) | (uint32_t)cell;
  ws.vals_a[i] = (uint32_t)j;
  atomicAdd(&ws.count[(size_t)b * MN_CELLS + cell], 1);
}

// One thread per sorted record: the compact copy the queries read.
__global__ __launch_bounds__(MN_BUILD_THREADS) void match_order_kernel(const float* __restrict__ scene, int M,
                                                                       MatchWs ws) {
  const int b = blockIdx.y;
  const int q = blockIdx.x * MN_BUILD_THREADS + threadIdx.x;
  if (q >= M) return;
  const size_t i = (size_t)b * M + q;
  const uint32_t j = ws.vals_b[i];
  if (j >= (uint32_t)M) return;   // (cannot happen: the values are the build's own)
  const float* __restrict__ p0 = scene + (size_t)b * 3 * M;
  ws.rec[i] = make_float4(p0[j], p0[M + j], p0[2 * (size_t)M + j], __int_as_float((int)j));
}

// A wave's running selection: `list` holds n distinct keys, every one below `thr`; once max_nn keys have been seen
// thr is the max_nn-th smallest of them, so a key at or above it can never be kept.
struct MnSelect {
  volatile uint64_t* list;   // [MN_LIST] LDS, this wave's
  uint64_t thr;
  int n, inside, max_nn, lane;

  // cuts the list to its min(n, max_nn) smallest keys, in ascending order
  __device__ __forceinline__ void cut() {
    const uint64_t none = ~0ull;
    const uint64_t k0 = lane < n ? list[lane] : none, k1 = lane + 64 < n ? list[lane + 64] : none;
    int r0 = 0, r1 = 0;
    for (int i = 0; i < n; ++i) {
      const uint64_t v = list[i];
      r0 += v < k0 ? 1 : 0;
      r1 += v < k1 ? 1 : 0;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < n && r0 < max_nn) list[r0] = k0;
    if (lane + 64 < n && r1 < max_nn) list[r1] = k1;
    __builtin_amdgcn_wave_barrier();
    if (n >= max_nn) {
      n = max_nn;
      thr = list[max_nn - 1];
    }
  }

  // one candidate per lane (wave-uniform call)
  __device__ __forceinline__ void consider(bool valid, float d2, float r2, int index) {
    const bool in = valid && d2 < r2;
    inside += __popcll(__ballot(in));
    const uint64_t key = ((uint64_t)__float_as_uint(d2) << 32) | (uint32_t)index;
    const bool keep = in && key < thr;
    const uint64_t m = __ballot(keep);
    if (m == 0) return;
    const int cnt = __popcll(m);
    if (n + cnt > MN_LIST) cut();   // n <= 64 afterwards
    if (keep) list[n + mask_rank(m)] = key;
    n += cnt;
    __builtin_amdgcn_wave_barrier();
  }
};

__device__ __forceinline__ double mn_wave_sum(double v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);
  return v;
}

// NEAREST: the search alone with max_nn = 1 (s4g_match_nearest_f32): the kept key's index, or -1; no normal is read.
template <bool NEAREST>
__global__ __launch_bounds__(MN_THREADS) void match_query_kernel(
    const float* __restrict__ query, const float* __restrict__ scene, const float* __restrict__ scene_normals,
    const float* __restrict__ camera, int N, int M, float r2, float inv_h, int max_nn, MatchWs ws,
    float* __restrict__ normals, int32_t* __restrict__ count, int32_t* __restrict__ flags,
    int32_t* __restrict__ nearest) {
  __shared__ uint64_t lists[MN_WAVES][MN_LIST];
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x * MN_WAVES + wave;
  if (q >= N) return;   // the whole wave
  const float* __restrict__ q0 = query + (size_t)b * 3 * N;
  const float* __restrict__ p0 = scene + (size_t)b * 3 * M;
  const float* __restrict__ n0 = NEAREST ? nullptr : scene_normals + (size_t)b * 3 * M;
  const float x = q0[q], y = q0[N + q], z = q0[2 * (size_t)N + q];
  const bool q_ok = finite(x) && finite(y) && finite(z);
  MnSelect s;
  s.list = lists[wave];
  s.thr = ~0ull;
  s.n = 0;
  s.inside = 0;
  s.max_nn = max_nn;
  s.lane = lane;
  if (q_ok) {   // nothing is near a point that is not finite
    const float ox = p0[0], oy = p0[M], oz = p0[2 * (size_t)M];
    const bool grid = ws.flags[b] == 0 && grid_coord_ok(x, ox, inv_h) && grid_coord_ok(y, oy, inv_h) &&
                      grid_coord_ok(z, oz, inv_h);
    if (grid) {
      const int icx = grid_coord(x, ox, inv_h), icy = grid_coord(y, oy, inv_h), icz = grid_coord(z, oz, inv_h);
      const int* __restrict__ start = ws.start + (size_t)b * MN_CELLS;
      // lane r < 9 fetches row r's runs: the row's three x cells are one run of records, or two where it wraps
      int vb0 = 0, ve0 = 0, vb1 = 0, ve1 = 0;
      if (lane < 9) {
        const int dz = lane / 3 - 1, dy = lane % 3 - 1;
        const int row = mn_cell(0, icy + dy, icz + dz);
        const int x0 = (icx - 1) & (MN_DIM - 1);
        vb0 = start[row + x0];
        if (x0 <= MN_DIM - 3) {
          ve0 = start[row + x0 + 3];
        } else {
          ve0 = start[row + MN_DIM];
          vb1 = start[row];
          ve1 = start[row + ((x0 + 3) & (MN_DIM - 1))];
        }
      }
      const float4* __restrict__ rec = ws.rec;   // the starts are offsets into the whole chunk
      const int lo = b * M, hi = lo + M;         // (the runs of scene b lie inside its own records)
      for (int r = 0; r < 9; ++r) {
        for (int run = 0; run < 2; ++run) {
          int rb = __shfl(run ? vb1 : vb0, r), re = __shfl(run ? ve1 : ve0, r);
          rb = rb < lo ? lo : rb;
          re = re > hi ? hi : re;
          for (int base = rb; base < re; base += 64) {
            const int i = base + lane;
            const bool valid = i < re;
            float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid) c = rec[i];
            s.consider(valid, dist2<false>(x, y, z, c.x, c.y, c.z), r2, __float_as_int(c.w));
          }
        }
      }
    } else {
      for (int base = 0; base < M; base += 64) {
        const int j = base + lane;
        const bool valid = j < M;
        float cx = 0.f, cy = 0.f, cz = 0.f;
        if (valid) { cx = p0[j]; cy = p0[M + j]; cz = p0[2 * (size_t)M + j]; }
        s.consider(valid, dist2<false>(x, y, z, cx, cy, cz), r2, j);
      }
    }
  }
  s.cut();   // ascending, at most max_nn
  const int k = s.n < max_nn ? s.n : max_nn;
  if constexpr (NEAREST) {
    if (lane == 0) nearest[(size_t)b * N + q] = k > 0 ? (int32_t)(uint32_t)s.list[0] : -1;
    return;
  }
  // the kept normals, rank r in lane r, summed in double by a fixed butterfly
  double ax = 0.0, ay = 0.0, az = 0.0;
  bool bad = false;
  if (lane < k) {
    const uint32_t j = (uint32_t)s.list[lane];
    if (j < (uint32_t)M) {   // (cannot be otherwise: the index is the scene's own)
      const float fx = n0[j], fy = n0[M + j], fz = n0[2 * (size_t)M + j];
      bad = !(finite(fx) && finite(fy) && finite(fz));
      ax = (double)fx; ay = (double)fy; az = (double)fz;
    }
  }
  const bool any_bad = __ballot(bad) != 0;
  const double sx = mn_wave_sum(ax), sy = mn_wave_sum(ay), sz = mn_wave_sum(az);
  if (lane != 0) return;
  int flag = (s.inside > max_nn ? 1 : 0) | (k == 0 ? 2 : 0) | (!q_ok || any_bad ? 8 : 0);
  double nx = 0.0, ny = 0.0, nz = 1.0;   // the mean of nothing is NaN: normalize_normals makes it (0, 0, 1)
  bool orient = camera != nullptr;
  if (any_bad) {
    nx = ny = nz = __longlong_as_double(0x7ff8000000000000ll);
    orient = false;
  } else if (k > 0) {
    const double mx = sx / (double)k, my = sy / (double)k, mz = sz / (double)k;
    const double len = sqrt(mx * mx + my * my + mz * mz);
    if (len > 0.0) {
      nx = mx / len; ny = my / len; nz = mz / len;
    } else {
      nx = ny = nz = 0.0;   // the kept normals cancel
      flag |= 4;
    }
  }
  if (orient) {
    const float* __restrict__ c0 = camera + (size_t)b * 3;
    const double rx = (double)c0[0] - (double)x, ry = (double)c0[1] - (double)y, rz = (double)c0[2] - (double)z;
    if (finite(rx) && finite(ry) && finite(rz)) {   // no reference direction otherwise: n stays
      if (nx == 0.0 && ny == 0.0 && nz == 0.0) {
        const double rl = sqrt(rx * rx + ry * ry + rz * rz);   // differences of fp32 numbers: no overflow in double
        if (rl > 0.0) {
          nx = rx / rl; ny = ry / rl; nz = rz / rl;
        } else {
          nz = 1.0;
        }
      } else if (nx * rx + ny * ry + nz * rz < 0.0) {
        nx = -nx; ny = -ny; nz = -nz;
      }
    }
  }
  float* __restrict__ o = normals + (size_t)b * 3 * N;
  o[q] = (float)nx;
  o[N + q] = (float)ny;
  o[2 * (size_t)N + q] = (float)nz;
  count[(size_t)b * N + q] = k;
  flags[(size_t)b * N + q] = flag;
}

}  // namespace s4g

extern "C" size_t s4g_match_normals_workspace_bytes(int64_t B, int64_t N, int64_t M) {
  (void)N;
  if (B <= 0 || M <= 0 || M >= (1ll << 30)) return 0;
  return s4g::match_ws(nullptr, s4g::mn_chunk(B, M), M, nullptr);
}

namespace s4g {

// The build (clear, keys, sort, scan, order) and the query launch both entry points share; nearest_bn != NULL selects
// the index-only query.
static int match_run(const float* query_b3n, const float* scene_b3m, const float* scene_normals_b3m,
                     const float* camera_b3, int64_t B, int64_t N, int64_t M, float radius, int32_t max_nn,
                     float* normals_b3n, int32_t* count_bn, int32_t* flags_bn, int32_t* nearest_bn, void* workspace,
                     size_t workspace_bytes, s4g_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  const float r2 = radius * radius;   // fp32 product, as for the ball query
  // cell edge slightly above the radius, as for the ball query (grid.h)
  const float h = radius * (1.0f + 1.0f / 256.0f);
  const float inv_h = 1.0f / h;
  const int64_t chunk = mn_chunk(B, M);
  const size_t need = match_ws(nullptr, chunk, M, nullptr);
  if (!workspace || workspace_bytes < need) return S4G_EWORKSPACE;
  for (int64_t b0 = 0; b0 < B; b0 += chunk) {
    const int64_t Bc = B - b0 < chunk ? B - b0 : chunk;
    MatchWs w = {};
    match_ws(workspace, Bc, M, &w);
    const size_t n = (size_t)Bc * (size_t)M, cells = (size_t)Bc * MN_CELLS + 1;
    const float* sc = scene_b3m + (size_t)b0 * 3 * M;
    const size_t n4 = mn_clear_int4(Bc);
    hipLaunchKernelGGL(match_clear_kernel, dim3((unsigned)((n4 + MN_BUILD_THREADS - 1) / MN_BUILD_THREADS)),
                       dim3(MN_BUILD_THREADS), 0, st, (int4*)w.count, n4);
    S4G_LAUNCH_CHECK();
    const dim3 bgrid((unsigned)((M + MN_BUILD_THREADS - 1) / MN_BUILD_THREADS), (unsigned)Bc);
    hipLaunchKernelGGL(match_keys_kernel, bgrid, dim3(MN_BUILD_THREADS), 0, st, sc, (int)M, inv_h, w);
    S4G_LAUNCH_CHECK();
    unsigned bits = MN_CELL_BITS;
    while (bits < 32 && ((int64_t)1 << (bits - MN_CELL_BITS)) < Bc) ++bits;
    if (int rc = radix_sort_pairs(w.sort, radix_sort_ws_bytes(n), w.keys_a, w.keys_b, w.vals_a, w.vals_b, n, bits, st))
      return rc;
    if (int rc = exclusive_scan_i32(w.scan, scan_ws_bytes(cells), w.count, w.start, cells, st)) return rc;
    hipLaunchKernelGGL(match_order_kernel, bgrid, dim3(MN_BUILD_THREADS), 0, st, sc, (int)M, w);
    S4G_LAUNCH_CHECK();
    const dim3 qgrid((unsigned)((N + MN_WAVES - 1) / MN_WAVES), (unsigned)Bc);
    if (nearest_bn) {
      hipLaunchKernelGGL(match_query_kernel<true>, qgrid, dim3(MN_THREADS), 0, st, query_b3n + (size_t)b0 * 3 * N, sc,
                         (const float*)nullptr, (const float*)nullptr, (int)N, (int)M, r2, inv_h, 1, w,
                         (float*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, nearest_bn + (size_t)b0 * N);
    } else {
      hipLaunchKernelGGL(match_query_kernel<false>, qgrid, dim3(MN_THREADS), 0, st, query_b3n + (size_t)b0 * 3 * N, sc,
                         scene_normals_b3m + (size_t)b0 * 3 * M, camera_b3 ? camera_b3 + (size_t)b0 * 3 : nullptr,
                         (int)N, (int)M, r2, inv_h, (int)max_nn, w, normals_b3n + (size_t)b0 * 3 * N,
                         count_bn + (size_t)b0 * N, flags_bn + (size_t)b0 * N, (int32_t*)nullptr);
    }
    S4G_LAUNCH_CHECK();
  }
  return S4G_OK;
}

}  // namespace s4g

extern "C" int s4g_match_normals_f32(const float* query_b3n, const float* scene_b3m, const float* scene_normals_b3m,
                                     const float* camera_b3, int64_t B, int64_t N, int64_t M, float radius,
                                     int32_t max_nn, float* normals_b3n, int32_t* count_bn, int32_t* flags_bn,
                                     void* workspace, size_t workspace_bytes, s4g_stream_t stream) {
  using namespace s4g;
  if (B < 0 || B > 65535 || N < 0 || N >= (1ll << 30) || M < 1 || M >= (1ll << 30)) return S4G_EINVAL;
  if (!(radius > 0.f) || !(radius < 1e18f) || max_nn < 1 || max_nn > MN_MAX_NN) return S4G_EINVAL;
  if (B == 0 || N == 0) return S4G_OK;
  if (!query_b3n || !scene_b3m || !scene_normals_b3m || !normals_b3n || !count_bn || !flags_bn) return S4G_EINVAL;
  return match_run(query_b3n, scene_b3m, scene_normals_b3m, camera_b3, B, N, M, radius, max_nn, normals_b3n, count_bn,
                   flags_bn, nullptr, workspace, workspace_bytes, stream);
}

// The max_nn = 1 search of TorchPrecomputedSingleViewPointCloud._find_match
// (data_gen/pcd_classes/torch_contact_single_view_point_cloud.py:142-150): the index alone.
extern "C" int s4g_match_nearest_f32(const float* query_b3n, const float* scene_b3m, int64_t B, int64_t N, int64_t M,
                                     float radius, int32_t* nearest_bn, void* workspace, size_t workspace_bytes,
                                     s4g_stream_t stream) {
  using namespace s4g;
  if (B < 0 || B > 65535 || N < 0 || N >= (1ll << 30) || M < 1 || M >= (1ll << 30)) return S4G_EINVAL;
  if (!(radius > 0.f) || !(radius < 1e18f)) return S4G_EINVAL;
  if (B == 0 || N == 0) return S4G_OK;
  if (!query_b3n || !scene_b3m || !nearest_bn) return S4G_EINVAL;
  return match_run(query_b3n, scene_b3m, nullptr, nullptr, B, N, M, radius, 1, nullptr, nullptr, nullptr, nearest_bn,
                   workspace, workspace_bytes, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// Normal estimation (s4g_estimate_normals_f32): PointCloud.estimate_normals of the reference
// (data_gen/pcd_classes/pointcloud.py:48-60): open3d's hybrid search, the plane fit of the kept neighbours,
// normalize_normals and orient_normals_towards_camera_location.  The cloud is its own key set: the grid, the sort and
// MnSelect above serve it unchanged.  What differs from the matching:
//   - the grid's origin is the first LIVE FINITE point (normals_origin_kernel), and a point that is not finite or lies
//     at or past live[b] sends no scene to the scan: it is sorted behind every scene of the chunk (scene number Bc in
//     its key) and counted in no cell, so no query ever reads it;
//   - the kept points' differences to the query are formed in double, their first and second moments summed by the
//     butterfly above in rank order, cov = S2 / k - (S1 / k)(S1 / k)^T;
//   - the eigenvector of the smallest eigenvalue by cyclic Jacobi in double on the matrix scaled by its largest entry
//     (every lane of the wave holds the same sums and runs the same solve; lane 0 writes).
// ---------------------------------------------------------------------------------------------------------------
namespace s4g {

constexpr int EN_SWEEPS = 10;          // cyclic Jacobi in double: quadratic, leaves the loop after 5 to 7 sweeps
constexpr int EN_FEW = 3;              // fewer kept neighbours than this define no plane
constexpr int EN_CAPPED = 1, EN_FEWBIT = 2, EN_DEGENERATE = 4, EN_NONFINITE = 8, EN_PADDING = 16;

struct NormalsWs {
  MatchWs m;
  float4* origin;                      // [Bc] the first live finite point of every scene (zero where there is none)
};

static size_t normals_ws(void* base, int64_t Bc, int64_t N, NormalsWs* w) {
  const size_t off = match_ws(base, Bc, N, w ? &w->m : nullptr);
  if (w && base) w->origin = (float4*)((char*)base + off);
  return off + mn_align((size_t)Bc * sizeof(float4));
}

// scenes one pass serves: as mn_chunk, with one key value (scene number Bc) left for the points no cell holds
static int64_t normals_chunk(int64_t B, int64_t N) { return mn_chunk(B, N); }

__device__ __forceinline__ int normals_live(const int32_t* __restrict__ live, int b, int N) {
  if (!live) return N;
  const int n = live[b];
  return n < 0 ? 0 : (n > N ? N : n);
}

// One workgroup per scene: the first live finite point in index order, 256 points at a time.
__global__ __launch_bounds__(MN_BUILD_THREADS) void normals_origin_kernel(const float* __restrict__ cloud,
                                                                          const int32_t* __restrict__ live, int N,
                                                                          float4* __restrict__ origin) {
  __shared__ int first;
  const int b = blockIdx.x;
  const int n = normals_live(live, b, N);
  const float* __restrict__ p0 = cloud + (size_t)b * 3 * N;
  if (threadIdx.x == 0) first = 0x7fffffff;
  __syncthreads();
  for (int base = 0; base < n; base += MN_BUILD_THREADS) {   // n is the workgroup's: the loop is uniform
    const int j = base + (int)threadIdx.x;
    const bool ok = j < n && finite(p0[j]) && finite(p0[N + j]) && finite(p0[2 * (size_t)N + j]);
    if (__syncthreads_or(ok ? 1 : 0)) {
      if (ok) atomicMin(&first, j);
      break;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int j = first;
    origin[b] = j < n ? make_float4(p0[j], p0[N + j], p0[2 * (size_t)N + j], 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// One thread per point: its sort key and, where it is a key of the search, its cell's population.  A finite live
// point outside the exactness range sends its scene to the scan (cell 0, as above); a point that is not finite or not
// live takes scene number Bc and no cell.
__global__ __launch_bounds__(MN_BUILD_THREADS) void normals_keys_kernel(const float* __restrict__ cloud,
                                                                        const int32_t* __restrict__ live, int N, int Bc,
                                                                        float inv_h, NormalsWs ws) {
  const int b = blockIdx.y;
  const int j = blockIdx.x * MN_BUILD_THREADS + threadIdx.x;
  if (j >= N) return;
  const float* __restrict__ p0 = cloud + (size_t)b * 3 * N;
  const float4 o = ws.origin[b];
  const float x = p0[j], y = p0[N + j], z = p0[2 * (size_t)N + j];
  const size_t i = (size_t)b * N + j;
  uint32_t key = (uint32_t)Bc << MN_CELL_BITS;
  if (j < normals_live(live, b, N) && finite(x) && finite(y) && finite(z)) {
    int cell = 0;
    if (grid_coord_ok(x, o.x, inv_h) && grid_coord_ok(y, o.y, inv_h) && grid_coord_ok(z, o.z, inv_h))
      cell = mn_cell(grid_coord(x, o.x, inv_h), grid_coord(y, o.y, inv_h), grid_coord(z, o.z, inv_h));
    else
      ws.m.flags[b] = 1;
    key = ((uint32_t)b << MN_CELL_BITS) | (uint32_t)cell;
    atomicAdd(&ws.m.count[(size_t)b * MN_CELLS + cell], 1);
  }
  ws.m.keys_a[i] = key;
  ws.m.vals_a[i] = (uint32_t)j;
}

// One thread per sorted record: the compact copy the queries read.  The scene comes from the sorted key: the records of
// the points no cell holds lie behind the last scene's and are never read (they are filled all the same).
__global__ __launch_bounds__(MN_BUILD_THREADS) void normals_order_kernel(const float* __restrict__ cloud, int N, int Bc,
                                                                         NormalsWs ws) {
  const int q = blockIdx.x * MN_BUILD_THREADS + threadIdx.x;
  if (q >= N) return;
  const size_t i = (size_t)blockIdx.y * N + q;
  const uint32_t s = ws.m.keys_b[i] >> MN_CELL_BITS, j = ws.m.vals_b[i];
  const float nan = __int_as_float(0x7fc00000);
  float4 r = make_float4(nan, nan, nan, __int_as_float(0));
  if (s < (uint32_t)Bc && j < (uint32_t)N) {
    const float* __restrict__ p0 = cloud + (size_t)s * 3 * N;
    r = make_float4(p0[j], p0[N + j], p0[2 * (size_t)N + j], __int_as_float((int)j));
  }
  ws.m.rec[i] = r;
}

// One Jacobi rotation in double, as darboux.hip's in fp32: (p, q) the plane, r the third index, v?p / v?q the columns
// p and q of the eigenvector matrix.  An off-diagonal too small to turn anything is left alone.
__device__ __forceinline__ void normals_rotate(double& app, double& aqq, double& apq, double& arp, double& arq,
                                               double& v0p, double& v0q, double& v1p, double& v1q, double& v2p,
                                               double& v2q) {
  if (!(fabs(apq) > 1e-40)) return;
  const double theta = (aqq - app) / (2.0 * apq);
  double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
  if (theta < 0.0) t = -t;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app = app - t * apq;
  aqq = aqq + t * apq;
  apq = 0.0;
  const double rp = c * arp - s * arq, rq = s * arp + c * arq;
  arp = rp;
  arq = rq;
  double a = c * v0p - s * v0q, d = s * v0p + c * v0q;
  v0p = a; v0q = d;
  a = c * v1p - s * v1q; d = s * v1p + c * v1q;
  v1p = a; v1q = d;
  a = c * v2p - s * v2q; d = s * v2p + c * v2q;
  v2p = a; v2q = d;
}

__global__ __launch_bounds__(MN_THREADS) void normals_query_kernel(
    const float* __restrict__ cloud, const float* __restrict__ camera, const int32_t* __restrict__ live, int N,
    int total, float r2, float inv_h, int max_nn, NormalsWs ws, float* __restrict__ normals,
    int32_t* __restrict__ count, int32_t* __restrict__ flags) {
  __shared__ uint64_t lists[MN_WAVES][MN_LIST];
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x * MN_WAVES + wave;
  if (q >= N) return;   // the whole wave
  const int n_live = normals_live(live, b, N);
  const float* __restrict__ p0 = cloud + (size_t)b * 3 * N;
  float* __restrict__ o = normals + (size_t)b * 3 * N;
  if (q >= n_live) {    // padding: neither a query nor a key
    if (lane == 0) {
      o[q] = 0.f; o[N + q] = 0.f; o[2 * (size_t)N + q] = 0.f;
      count[(size_t)b * N + q] = 0;
      flags[(size_t)b * N + q] = EN_PADDING;
    }
    return;
  }
  const float x = p0[q], y = p0[N + q], z = p0[2 * (size_t)N + q];
  if (!(finite(x) && finite(y) && finite(z))) {   // no neighbourhood, no direction to turn to
    if (lane == 0) {
      o[q] = 0.f; o[N + q] = 0.f; o[2 * (size_t)N + q] = 1.f;
      count[(size_t)b * N + q] = 0;
      flags[(size_t)b * N + q] = EN_NONFINITE;
    }
    return;
  }
  MnSelect s;
  s.list = lists[wave];
  s.thr = ~0ull;
  s.n = 0;
  s.inside = 0;
  s.max_nn = max_nn;
  s.lane = lane;
  const float4 org = ws.origin[b];
  const bool grid = ws.m.flags[b] == 0 && grid_coord_ok(x, org.x, inv_h) && grid_coord_ok(y, org.y, inv_h) &&
                    grid_coord_ok(z, org.z, inv_h);
  if (grid) {
    const int icx = grid_coord(x, org.x, inv_h), icy = grid_coord(y, org.y, inv_h), icz = grid_coord(z, org.z, inv_h);
    const int* __restrict__ start = ws.m.start + (size_t)b * MN_CELLS;
    // lane r < 9 fetches row r's runs, as match_query_kernel does
    int vb0 = 0, ve0 = 0, vb1 = 0, ve1 = 0;
    if (lane < 9) {
      const int dz = lane / 3 - 1, dy = lane % 3 - 1;
      const int row = mn_cell(0, icy + dy, icz + dz);
      const int x0 = (icx - 1) & (MN_DIM - 1);
      vb0 = start[row + x0];
      if (x0 <= MN_DIM - 3) {
        ve0 = start[row + x0 + 3];
      } else {
        ve0 = start[row + MN_DIM];
        vb1 = start[row];
        ve1 = start[row + ((x0 + 3) & (MN_DIM - 1))];
      }
    }
    const float4* __restrict__ rec = ws.m.rec;   // the starts are offsets into the whole chunk
    for (int r = 0; r < 9; ++r) {
      for (int run = 0; run < 2; ++run) {
        int rb = __shfl(run ? vb1 : vb0, r), re = __shfl(run ? ve1 : ve0, r);
        rb = rb < 0 ? 0 : rb;
        re = re > total ? total : re;
        for (int base = rb; base < re; base += 64) {
          const int i = base + lane;
          const bool valid = i < re;
          float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
          if (valid) c = rec[i];
          s.consider(valid, dist2<false>(x, y, z, c.x, c.y, c.z), r2, __float_as_int(c.w));
        }
      }
    }
  } else {
    for (int base = 0; base < n_live; base += 64) {   // a point that is not finite fails the comparison by itself
      const int j = base + lane;
      const bool valid = j < n_live;
      float cx = 0.f, cy = 0.f, cz = 0.f;
      if (valid) { cx = p0[j]; cy = p0[N + j]; cz = p0[2 * (size_t)N + j]; }
      s.consider(valid, dist2<false>(x, y, z, cx, cy, cz), r2, j);
    }
  }
  s.cut();   // ascending, at most max_nn
  const int k = s.n < max_nn ? s.n : max_nn;
  // the kept points, rank r in lane r: differences to the query in double, moments by the fixed butterfly
  double dx = 0.0, dy = 0.0, dz = 0.0;
  if (lane < k) {
    const uint32_t j = (uint32_t)s.list[lane];
    if (j < (uint32_t)N) {   // (cannot be otherwise: the index is the cloud's own)
      dx = (double)p0[j] - (double)x;
      dy = (double)p0[N + j] - (double)y;
      dz = (double)p0[2 * (size_t)N + j] - (double)z;
    }
  }
  const double s1x = mn_wave_sum(dx), s1y = mn_wave_sum(dy), s1z = mn_wave_sum(dz);
  const double sxx = mn_wave_sum(dx * dx), syy = mn_wave_sum(dy * dy), szz = mn_wave_sum(dz * dz);
  const double sxy = mn_wave_sum(dx * dy), sxz = mn_wave_sum(dx * dz), syz = mn_wave_sum(dy * dz);
  int flag = s.inside > max_nn ? EN_CAPPED : 0;
  double nx = 0.0, ny = 0.0, nz = 1.0;
  if (k < EN_FEW) {
    flag |= EN_FEWBIT;
  } else if (sxx + syy + szz == 0.0) {   // every kept point is the query's copy (a square of a difference is 0 only there)
    flag |= EN_DEGENERATE;
  } else {
    const double ik = 1.0 / (double)k;
    const double mx = s1x * ik, my = s1y * ik, mz = s1z * ik;
    double a00 = sxx * ik - mx * mx, a11 = syy * ik - my * my, a22 = szz * ik - mz * mz;
    double a01 = sxy * ik - mx * my, a02 = sxz * ik - mx * mz, a12 = syz * ik - my * mz;
    const double big = fmax(fmax(fmax(fabs(a00), fabs(a11)), fabs(a22)), fmax(fmax(fabs(a01), fabs(a02)), fabs(a12)));
    bool solved = false;
    if (big > 0.0 && finite(big)) {
      const double sc = 1.0 / big;
      a00 *= sc; a11 *= sc; a22 *= sc; a01 *= sc; a02 *= sc; a12 *= sc;
      double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
      for (int sw = 0; sw < EN_SWEEPS; ++sw) {
        if (!(fabs(a01) + fabs(a02) + fabs(a12) > 1e-24)) break;
        normals_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
        normals_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
        normals_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
      }
      // the smallest eigenvalue, the lowest column on a tie
      double ex = v00, ey = v10, ez = v20, e = a00;
      if (a11 < e) { ex = v01; ey = v11; ez = v21; e = a11; }
      if (a22 < e) { ex = v02; ey = v12; ez = v22; e = a22; }
      const double len = sqrt(ex * ex + ey * ey + ez * ez);
      if (len > 0.0 && finite(len)) {
        nx = ex / len; ny = ey / len; nz = ez / len;
        solved = true;
      }
    }
    if (!solved) flag |= EN_DEGENERATE;
  }
  // sign: towards the camera; without a direction the component of largest magnitude is positive, the lowest axis on a
  // tie (the rule of s4g_darboux_frames_f32)
  double dot = 0.0;
  if (camera != nullptr) {
    const float* __restrict__ c0 = camera + (size_t)b * 3;
    const double rx = (double)c0[0] - (double)x, ry = (double)c0[1] - (double)y, rz = (double)c0[2] - (double)z;
    if (finite(rx) && finite(ry) && finite(rz)) dot = nx * rx + ny * ry + nz * rz;
  }
  bool flip = dot < 0.0;
  if (dot == 0.0) {
    double lead = nx;
    if (fabs(ny) > fabs(lead)) lead = ny;
    if (fabs(nz) > fabs(lead)) lead = nz;
    flip = lead < 0.0;
  }
  if (flip) { nx = -nx; ny = -ny; nz = -nz; }
  if (lane != 0) return;
  o[q] = (float)nx;
  o[N + q] = (float)ny;
  o[2 * (size_t)N + q] = (float)nz;
  count[(size_t)b * N + q] = k;
  flags[(size_t)b * N + q] = flag;
}

// The neighbour INDICES alone (s4g_match_knn_f32): normals_query_kernel's search over the same build, then the kept
// list's indices in rank order -- (fp32 squared distance, index) ascending, the query itself or a lower-index copy of
// it first -- and -1 beyond the count.  A padding row and a point that is not finite have no neighbours.
__global__ __launch_bounds__(MN_THREADS) void match_knn_kernel(
    const float* __restrict__ cloud, const int32_t* __restrict__ live, int N, int total, float r2, float inv_h,
    int max_nn, NormalsWs ws, int32_t* __restrict__ knn) {
  __shared__ uint64_t lists[MN_WAVES][MN_LIST];
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x * MN_WAVES + wave;
  if (q >= N) return;   // the whole wave
  const int n_live = normals_live(live, b, N);
  const float* __restrict__ p0 = cloud + (size_t)b * 3 * N;
  int32_t* __restrict__ o = knn + ((size_t)b * N + q) * max_nn;
  float x = 0.f, y = 0.f, z = 0.f;
  if (q < n_live) { x = p0[q]; y = p0[N + q]; z = p0[2 * (size_t)N + q]; }
  if (q >= n_live || !(finite(x) && finite(y) && finite(z))) {
    if (lane < max_nn) o[lane] = -1;
    return;
  }
  MnSelect s;
  s.list = lists[wave];
  s.thr = ~0ull;
  s.n = 0;
  s.inside = 0;
  s.max_nn = max_nn;
  s.lane = lane;
  const float4 org = ws.origin[b];
  const bool grid = ws.m.flags[b] == 0 && grid_coord_ok(x, org.x, inv_h) && grid_coord_ok(y, org.y, inv_h) &&
                    grid_coord_ok(z, org.z, inv_h);
  if (grid) {
    const int icx = grid_coord(x, org.x, inv_h), icy = grid_coord(y, org.y, inv_h), icz = grid_coord(z, org.z, inv_h);
    const int* __restrict__ start = ws.m.start + (size_t)b * MN_CELLS;
    // lane r < 9 fetches row r's runs, as match_query_kernel does
    int vb0 = 0, ve0 = 0, vb1 = 0, ve1 = 0;
    if (lane < 9) {
      const int dz = lane / 3 - 1, dy = lane % 3 - 1;
      const int row = mn_cell(0, icy + dy, icz + dz);
      const int x0 = (icx - 1) & (MN_DIM - 1);
      vb0 = start[row + x0];
      if (x0 <= MN_DIM - 3) {
        ve0 = start[row + x0 + 3];
      } else {
        ve0 = start[row + MN_DIM];
        vb1 = start[row];
        ve1 = start[row + ((x0 + 3) & (MN_DIM - 1))];
      }
    }
    const float4* __restrict__ rec = ws.m.rec;   // the starts are offsets into the whole chunk
    for (int r = 0; r < 9; ++r) {
      for (int run = 0; run < 2; ++run) {
        int rb = __shfl(run ? vb1 : vb0, r), re = __shfl(run ? ve1 : ve0, r);
        rb = rb < 0 ? 0 : rb;
        re = re > total ? total : re;
        for (int base = rb; base < re; base += 64) {
          const int i = base + lane;
          const bool valid = i < re;
          float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
          if (valid) c = rec[i];
          s.consider(valid, dist2<false>(x, y, z, c.x, c.y, c.z), r2, __float_as_int(c.w));
        }
      }
    }
  } else {
    for (int base = 0; base < n_live; base += 64) {   // a point that is not finite fails the comparison by itself
      const int j = base + lane;
      const bool valid = j < n_live;
      float cx = 0.f, cy = 0.f, cz = 0.f;
      if (valid) { cx = p0[j]; cy = p0[N + j]; cz = p0[2 * (size_t)N + j]; }
      s.consider(valid, dist2<false>(x, y, z, cx, cy, cz), r2, j);
    }
  }
  s.cut();   // ascending, at most max_nn
  const int k = s.n < max_nn ? s.n : max_nn;
  if (lane < max_nn) {
    int32_t j = -1;
    if (lane < k) {
      const uint32_t v = (uint32_t)s.list[lane];
      if (v < (uint32_t)N) j = (int32_t)v;   // (cannot be otherwise: the index is the cloud's own)
    }
    o[lane] = j;
  }
}

}  // namespace s4g

extern "C" size_t s4g_estimate_normals_workspace_bytes(int64_t B, int64_t N) {
  if (B <= 0 || N <= 0 || N >= (1ll << 30)) return 0;
  return s4g::normals_ws(nullptr, s4g::normals_chunk(B, N), N, nullptr);
}

namespace s4g {

// The build (clear, origin, keys, sort, scan, order) of scenes [b0, b0 + Bc) that s4g_estimate_normals_f32 and
// s4g_match_knn_f32 share; the caller launches its query kernel on w.
static int normals_build(const float* xyz, const int32_t* lv, int64_t Bc, int64_t N, float inv_h, void* workspace,
                         NormalsWs* w, hipStream_t st) {
  normals_ws(workspace, Bc, N, w);
  const size_t n = (size_t)Bc * (size_t)N, cells = (size_t)Bc * MN_CELLS + 1;
  const size_t n4 = mn_clear_int4(Bc);
  hipLaunchKernelGGL(match_clear_kernel, dim3((unsigned)((n4 + MN_BUILD_THREADS - 1) / MN_BUILD_THREADS)),
                     dim3(MN_BUILD_THREADS), 0, st, (int4*)w->m.count, n4);
  S4G_LAUNCH_CHECK();
  hipLaunchKernelGGL(normals_origin_kernel, dim3((unsigned)Bc), dim3(MN_BUILD_THREADS), 0, st, xyz, lv, (int)N,
                     w->origin);
  S4G_LAUNCH_CHECK();
  const dim3 bgrid((unsigned)((N + MN_BUILD_THREADS - 1) / MN_BUILD_THREADS), (unsigned)Bc);
  hipLaunchKernelGGL(normals_keys_kernel, bgrid, dim3(MN_BUILD_THREADS), 0, st, xyz, lv, (int)N, (int)Bc, inv_h, *w);
  S4G_LAUNCH_CHECK();
  unsigned bits = MN_CELL_BITS;   // scene numbers 0 .. Bc: Bc itself marks the points no cell holds
  while (bits < 32 && ((int64_t)1 << (bits - MN_CELL_BITS)) < Bc + 1) ++bits;
  if (int rc = radix_sort_pairs(w->m.sort, radix_sort_ws_bytes(n), w->m.keys_a, w->m.keys_b, w->m.vals_a, w->m.vals_b,
                                n, bits, st))
    return rc;
  if (int rc = exclusive_scan_i32(w->m.scan, scan_ws_bytes(cells), w->m.count, w->m.start, cells, st)) return rc;
  hipLaunchKernelGGL(normals_order_kernel, bgrid, dim3(MN_BUILD_THREADS), 0, st, xyz, (int)N, (int)Bc, *w);
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}

}  // namespace s4g

extern "C" int s4g_estimate_normals_f32(const float* cloud_b3n, const float* camera_b3, const int32_t* live_b, int64_t B,
                                        int64_t N, float radius, int32_t max_nn, float* normals_b3n, int32_t* count_bn,
                                        int32_t* flags_bn, void* workspace, size_t workspace_bytes,
                                        s4g_stream_t stream) {
  using namespace s4g;
  if (B < 0 || B > 65535 || N < 0 || N >= (1ll << 30)) return S4G_EINVAL;
  if (!(radius > 0.f) || !(radius < 1e18f) || max_nn < 1 || max_nn > MN_MAX_NN) return S4G_EINVAL;
  if (B == 0 || N == 0) return S4G_OK;
  if (!cloud_b3n || !normals_b3n || !count_bn || !flags_bn) return S4G_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const float r2 = radius * radius;                      // as match_run: the fp32 product,
  const float h = radius * (1.0f + 1.0f / 256.0f);       // the cell edge slightly above the radius
  const float inv_h = 1.0f / h;
  const int64_t chunk = normals_chunk(B, N);
  const size_t need = normals_ws(nullptr, chunk, N, nullptr);
  if (!workspace || workspace_bytes < need) return S4G_EWORKSPACE;
  for (int64_t b0 = 0; b0 < B; b0 += chunk) {
    const int64_t Bc = B - b0 < chunk ? B - b0 : chunk;
    NormalsWs w = {};
    const float* xyz = cloud_b3n + (size_t)b0 * 3 * N;
    const int32_t* lv = live_b ? live_b + b0 : nullptr;
    if (int rc = normals_build(xyz, lv, Bc, N, inv_h, workspace, &w, st)) return rc;
    const dim3 qgrid((unsigned)((N + MN_WAVES - 1) / MN_WAVES), (unsigned)Bc);
    hipLaunchKernelGGL(normals_query_kernel, qgrid, dim3(MN_THREADS), 0, st, xyz,
                       camera_b3 ? camera_b3 + (size_t)b0 * 3 : nullptr, lv, (int)N, (int)(Bc * N), r2, inv_h,
                       (int)max_nn, w, normals_b3n + (size_t)b0 * 3 * N, count_bn + (size_t)b0 * N,
                       flags_bn + (size_t)b0 * N);
    S4G_LAUNCH_CHECK();
  }
  return S4G_OK;
}

// The max_nn nearest points of every point of a cloud within the radius, the indices alone: the kd-tree search of
// smooth_contact_object.py:72.  Workspace: s4g_estimate_normals_workspace_bytes(B, N).
extern "C" int s4g_match_knn_f32(const float* cloud_b3n, const int32_t* live_b, int64_t B, int64_t N, float radius,
                                 int32_t max_nn, int32_t* knn_bnk, void* workspace, size_t workspace_bytes,
                                 s4g_stream_t stream) {
  using namespace s4g;
  if (B < 0 || B > 65535 || N < 0 || N >= (1ll << 30)) return S4G_EINVAL;
  if (!(radius > 0.f) || !(radius < 1e18f) || max_nn < 1 || max_nn > MN_MAX_NN) return S4G_EINVAL;
  if (B == 0 || N == 0) return S4G_OK;
  if (!cloud_b3n || !knn_bnk) return S4G_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const float r2 = radius * radius;
  const float h = radius * (1.0f + 1.0f / 256.0f);
  const float inv_h = 1.0f / h;
  const int64_t chunk = normals_chunk(B, N);
  const size_t need = normals_ws(nullptr, chunk, N, nullptr);
  if (!workspace || workspace_bytes < need) return S4G_EWORKSPACE;
  for (int64_t b0 = 0; b0 < B; b0 += chunk) {
    const int64_t Bc = B - b0 < chunk ? B - b0 : chunk;
    NormalsWs w = {};
    const float* xyz = cloud_b3n + (size_t)b0 * 3 * N;
    const int32_t* lv = live_b ? live_b + b0 : nullptr;
    if (int rc = normals_build(xyz, lv, Bc, N, inv_h, workspace, &w, st)) return rc;
    const dim3 qgrid((unsigned)((N + MN_WAVES - 1) / MN_WAVES), (unsigned)Bc);
    hipLaunchKernelGGL(match_knn_kernel, qgrid, dim3(MN_THREADS), 0, st, xyz, lv, (int)N, (int)(Bc * N), r2, inv_h,
                       (int)max_nn, w, knn_bnk + (size_t)b0 * N * max_nn);
    S4G_LAUNCH_CHECK();
  }
  return S4G_OK;
}
