// The first stage of the data generator's view pipeline for B views in one sync-free call: `processing_and_trace`
// (data_gen/pcd_classes/torch_precomputed_single_view_point_cloud.py:64-97, the same code in
// torch_contact_single_view_point_cloud.py:79-112 and torch_precomputed_baseline.py:76-109) -- workspace crop,
// open3d's voxel_down_sample_and_trace over the CALLER's bounds, remove_radius_outlier, and the index of every kept
// row in the cloud the call was given.  Contract: include/s4g_ops.h (s4g_process_views_f32).
//
// Per scene the result is what s4g_crop_indices_f32 -> s4g_voxel_down_sample_f32 (same origin3 / dims3) ->
// s4g_radius_outlier_mask_f32 give, bit for bit (preprocess.hip; the arithmetic below is theirs, unchanged), plus the
// trace: the highest original index among a voxel's points.  What differs is the shape of the work:
//   crop     one workgroup per scene, the ordered ballot compaction of crop_compact_kernel with a scene base;
//   voxel    ONE stable radix sort of (scene << cell_bits | cell, original index) pairs per chunk of scenes; a row the
//            crop dropped takes the all-ones key of the sort's width, which no live row can have (pv_plan), and so
//            sorts behind every scene.  The host refuses bounds that do not contain the crop box: no kept point is
//            clamped, and neither the grid nor the sort width depends on the data.  Heads, the library's exclusive scan,
//            one thread per scene (two binary searches in the sorted keys: the scene's first cell and its cell count) and
//            one thread per cell follow.  The sort is stable and the crop keeps the order, so a cell's records are in
//            ascending original index: the trace is the cell's last record;
//   radius   the toroidal 64^3 grid of match_normals.hip over the voxel means of every scene of the chunk (cell edge
//            just above the radius, origin = the scene's first mean, grid.h's cell coordinates and exactness range): keys,
//            a second sort, the cells' populations (integer atomics: a count does not depend on their order) and their
//            exclusive scan, a compact copy of the records in sorted order.  One thread per SORTED record counts its
//            27 cells and stops at cnt > nb, so the lanes of a wave walk the same runs; a scene with a mean outside
//            the exactness range scans its means in index order.  The count is a property of the candidate SET;
//   finish   one workgroup per scene: ordered ballot compaction of the kept means (no arrival order anywhere), the
//            trace, the final count, NaN / -1 behind it.
// Every device count is clamped to [0, N] where it is read.  A batch above the chunk is served chunk after chunk on
// the same workspace: the number of launches depends on the number of chunks alone.
#include <float.h>
#include <math.h>

#include "grid.h"
#include "radix_sort.h"
#include "s4g_common.h"

namespace s4g {

constexpr int PV_THREADS = 1024;                           // crop / finish: points per round
constexpr int PV_BLOCK = 256;
constexpr int PV_DIM = 64;                                 // radius grid: cells per axis (toroidal)
constexpr int PV_CELL_BITS = 18;
constexpr int PV_CELLS = PV_DIM * PV_DIM * PV_DIM;
constexpr int PV_CHUNK = 256;                              // scenes per pass at most (the radius grid's tables)

struct PvWs {
  int* crop;                                     // [Bc * N] ascending kept indices, scene after scene
  uint32_t *keys_a, *keys_b, *vals_a, *vals_b;   // [Bc * N] sort ping-pong; keys_b / vals_b hold the result
  void* sort;                                    // radix_sort_ws_bytes(Bc * N)
  int *head, *rank;                              // [Bc * N]
  int* vbase;                                    // [Bc] cells in front of the scene's first
  float4* vox;                                   // [Bc * N] (mean, trace bits), scene b's cells from b * N
  int* count;                                    // [Bc * PV_CELLS + 1] radius cell populations (the last entry stays 0) ...
  int* flags;                                    // ... then [Bc] 1 = scene out of the exactness range -> scan; set per pass
  int* start;                                    // [Bc * PV_CELLS + 1]
  void* scan;                                    // scan_ws_bytes of the longer of the two scans
  size_t scan_bytes;
  float4* rec;                                   // [Bc * N] (mean, cell number in the scene) in radius-sorted order
  uint8_t* keep;                                 // [Bc * N]
};

static size_t pv_align(size_t v) { return (v + 255) & ~(size_t)255; }

// scenes one pass serves at most, whatever the voxel grid: the rows' offsets hold 31 bits
static int64_t pv_chunk_max(int64_t B, int64_t N) {
  int64_t c = ((1ll << 31) - 1) / (N > 0 ? N : 1);
  if (c > PV_CHUNK) c = PV_CHUNK;
  if (c > B) c = B;
  return c < 1 ? 1 : c;
}

static size_t pv_clear_int4(int64_t Bc) { return ((size_t)Bc * PV_CELLS + 1 + (size_t)Bc + 3) / 4; }

static size_t pv_ws(void* base, int64_t Bc, int64_t N, PvWs* w) {
  char* p = (char*)base;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* r = p ? p + off : nullptr;
    off += pv_align(bytes);
    return r;
  };
  const size_t n = (size_t)Bc * (size_t)N, cells = (size_t)Bc * PV_CELLS + 1;
  const size_t s0 = scan_ws_bytes(n), s1 = scan_ws_bytes(cells);
  PvWs t;
  t.crop = (int*)take(n * 4);
  t.keys_a = (uint32_t*)take(n * 4);
  t.keys_b = (uint32_t*)take(n * 4);
  t.vals_a = (uint32_t*)take(n * 4);
  t.vals_b = (uint32_t*)take(n * 4);
  t.sort = take(radix_sort_ws_bytes(n));
  t.head = (int*)take(n * 4);
  t.rank = (int*)take(n * 4);
  t.vbase = (int*)take((size_t)Bc * 4);
  t.vox = (float4*)take(n * sizeof(float4));
  t.count = (int*)take(pv_clear_int4(Bc) * sizeof(int4));
  t.flags = nullptr;                             // behind the populations of the pass's own Bc scenes: the entry sets it
  t.start = (int*)take(cells * 4);
  t.scan_bytes = s0 > s1 ? s0 : s1;
  t.scan = take(t.scan_bytes);
  t.rec = (float4*)take(n * sizeof(float4));
  t.keep = (uint8_t*)take(n);
  if (w) *w = t;
  return off;
}

// What the voxel grid leaves of the 32 key bits.  cell_bits = ceil(log2(cells)); the dead key is all ones over the
// sort's width.  Its scene number is 2^scene_bits - 1 >= slots - 1: where the grid does not fill its bits (cells <
// 2^cell_bits) the all-ones cell is no cell and slots = scenes; where it does, one more scene number is set aside.
struct PvPlan {
  int64_t chunk;
  unsigned cell_bits, bits;
  uint32_t dead;
};

static PvPlan pv_plan(int64_t B, int64_t N, uint64_t cells) {
  PvPlan p;
  p.cell_bits = 1;
  while (p.cell_bits < 32 && (1ull << p.cell_bits) < cells) ++p.cell_bits;
  const bool full = (1ull << p.cell_bits) == cells;        // (never with 32 bits: cells < 2^32)
  int64_t cap = p.cell_bits >= 32 ? 1 : (1ll << (32 - p.cell_bits)) - (full ? 1 : 0);
  if (cap < 1) cap = 1;
  p.chunk = pv_chunk_max(B, N);
  if (p.chunk > cap) p.chunk = cap;
  const int64_t slots = p.chunk + (full ? 1 : 0);
  unsigned sb = 0;
  while (((int64_t)1 << sb) < slots) ++sb;
  p.bits = p.cell_bits + sb;                                // <= 32 by the cap
  p.dead = p.bits >= 32 ? 0xffffffffu : (1u << p.bits) - 1u;
  return p;
}

__device__ __forceinline__ int pv_clamp(int n, int N) { return n < 0 ? 0 : (n > N ? N : n); }

__global__ __launch_bounds__(PV_BLOCK) void pv_zero_counts_kernel(int32_t* __restrict__ counts, int n) {
  const int i = blockIdx.x * PV_BLOCK + threadIdx.x;
  if (i < n) counts[i] = 0;
}

// One workgroup per scene: crop_compact_kernel's loop over the scene's live rows.
__global__ __launch_bounds__(PV_THREADS) void pv_crop_kernel(
    const float* __restrict__ xyz, const int32_t* __restrict__ live, int N, float lox, float hix, float loy, float hiy,
    float loz, float hiz, int* __restrict__ index, int32_t* __restrict__ counts) {
  __shared__ int wave_cnt[PV_THREADS / 64];
  __shared__ int base_s;
  const int b = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n = live ? pv_clamp(live[b], N) : N;
  const float* px = xyz + (size_t)b * 3 * N;
  const float* py = px + N;
  const float* pz = px + 2 * (size_t)N;
  int* __restrict__ out = index + (size_t)b * N;
  if (t == 0) base_s = 0;
  __syncthreads();
  for (int j0 = 0; j0 < n; j0 += PV_THREADS) {   // n is the workgroup's: the loop is uniform
    const int j = j0 + t;
    bool keep = false;
    if (j < n) {
      const float x = px[j], y = py[j], z = pz[j];
      keep = x > lox && y > loy && z > loz && x < hix && y < hiy && z < hiz;
    }
    const uint64_t m = __ballot(keep);
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < PV_THREADS / 64; ++w) {
      const int c = wave_cnt[w];
      before += w < wave ? c : 0;
      total += c;
    }
    const int base = base_s;
    if (keep) out[base + before + mask_rank(m)] = j;   // < n <= N: one slot per kept row
    __syncthreads();
    if (t == 0) base_s = base + total;
  }
  __syncthreads();
  if (t == 0) counts[(size_t)b * 3] = base_s;
}

// One thread per row of the cropped list: voxel_key_kernel's cell under the scene's number, the value is the ORIGINAL
// index.  Rows past the scene's crop count take the dead key.
__global__ __launch_bounds__(PV_BLOCK) void pv_voxel_keys_kernel(
    const float* __restrict__ xyz, int N, float ox, float oy, float oz, float voxel, int dx, int dy, int dz,
    unsigned cell_bits, uint32_t dead, const int32_t* __restrict__ counts, PvWs ws) {
  const int b = blockIdx.y;
  const int k = blockIdx.x * PV_BLOCK + threadIdx.x;
  if (k >= N) return;
  const size_t i = (size_t)b * N + k;
  uint32_t key = dead, val = 0;
  if (k < pv_clamp(counts[(size_t)b * 3], N)) {
    const int j = ws.crop[i];
    if (j >= 0 && j < N) {   // (cannot be otherwise: the list is the crop's own)
      const float* __restrict__ p0 = xyz + (size_t)b * 3 * N;
      // floor((p - origin) / voxel), each operation rounded once (fp32)
      int ix = (int)floorf(__fdiv_rn(__fsub_rn(p0[j], ox), voxel));
      int iy = (int)floorf(__fdiv_rn(__fsub_rn(p0[N + j], oy), voxel));
      int iz = (int)floorf(__fdiv_rn(__fsub_rn(p0[2 * (size_t)N + j], oz), voxel));
      ix = min(max(ix, 0), dx - 1);
      iy = min(max(iy, 0), dy - 1);
      iz = min(max(iz, 0), dz - 1);
      const uint32_t cell = ((uint32_t)iz * (uint32_t)dy + (uint32_t)iy) * (uint32_t)dx + (uint32_t)ix;
      key = (uint32_t)(((uint64_t)b << cell_bits) | (uint64_t)cell);
      val = (uint32_t)j;
    }
  }
  ws.keys_a[i] = key;
  ws.vals_a[i] = val;
}

__global__ __launch_bounds__(PV_BLOCK) void pv_heads_kernel(const uint32_t* __restrict__ key, size_t n, uint32_t dead,
                                                            int* __restrict__ head) {
  const size_t i = (size_t)blockIdx.x * PV_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t k = key[i];
  head[i] = (k != dead && (i == 0 || k != key[i - 1])) ? 1 : 0;
}

// first sorted row whose key is at or above `target`
__device__ __forceinline__ size_t pv_lower_bound(const uint32_t* __restrict__ key, size_t n, uint64_t target) {
  size_t lo = 0, hi = n;
  while (lo < hi) {
    const size_t mid = lo + (hi - lo) / 2;
    if ((uint64_t)key[mid] < target) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// One thread per scene: the cells in front of its first (a scene's first row is a head, a dead row is none) and its
// cell count.
__global__ __launch_bounds__(PV_BLOCK) void pv_segments_kernel(const uint32_t* __restrict__ key, size_t n, int Bc, int N,
                                                               unsigned cell_bits, uint32_t dead,
                                                               const int* __restrict__ head,
                                                               const int* __restrict__ rank, int* __restrict__ vbase,
                                                               int32_t* __restrict__ counts) {
  const int b = blockIdx.x * PV_BLOCK + threadIdx.x;
  if (b >= Bc) return;
  const int total = rank[n - 1] + head[n - 1];
  const size_t lo = pv_lower_bound(key, n, (uint64_t)b << cell_bits);
  const size_t hi = b + 1 < Bc ? pv_lower_bound(key, n, (uint64_t)(b + 1) << cell_bits)
                               : pv_lower_bound(key, n, (uint64_t)dead);
  const int r0 = lo < n ? rank[lo] : total, r1 = hi < n ? rank[hi] : total;
  vbase[b] = r0;
  counts[(size_t)b * 3 + 1] = pv_clamp(r1 - r0, N);
}

// One thread per voxel: voxel_mean_kernel's walk (double sum in index order, one rounding), and the last record's
// index.
__global__ __launch_bounds__(PV_BLOCK) void pv_voxel_mean_kernel(const float* __restrict__ xyz, int N, size_t n, int Bc,
                                                                 unsigned cell_bits, PvWs ws) {
  const size_t i = (size_t)blockIdx.x * PV_BLOCK + threadIdx.x;
  if (i >= n) return;
  if (!ws.head[i]) return;
  const uint32_t k = ws.keys_b[i];
  const uint32_t b = (uint32_t)((uint64_t)k >> cell_bits);
  if (b >= (uint32_t)Bc) return;   // (cannot happen: a head is a live row)
  const int v = ws.rank[i] - ws.vbase[b];
  if (v < 0 || v >= N) return;     // (cannot happen: a scene has at most N rows)
  const float* __restrict__ p0 = xyz + (size_t)b * 3 * N;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  int cnt = 0;
  uint32_t last = 0;
  for (size_t r = i; r < n && ws.keys_b[r] == k; ++r) {
    const uint32_t p = ws.vals_b[r];
    if (p >= (uint32_t)N) continue;   // (cannot happen: the values are the build's own)
    sx += (double)p0[p];
    sy += (double)p0[N + p];
    sz += (double)p0[2 * (size_t)N + p];
    last = p;
    ++cnt;
  }
  ws.vox[(size_t)b * N + v] = make_float4((float)(sx / (double)cnt), (float)(sy / (double)cnt),
                                          (float)(sz / (double)cnt), __int_as_float((int)last));
}

__device__ __forceinline__ int pv_cell(int cx, int cy, int cz) {
  return ((cz & (PV_DIM - 1)) << 12) | ((cy & (PV_DIM - 1)) << 6) | (cx & (PV_DIM - 1));
}

__global__ __launch_bounds__(PV_BLOCK) void pv_clear_kernel(int4* __restrict__ p, size_t n4) {
  const size_t i = (size_t)blockIdx.x * PV_BLOCK + threadIdx.x;
  if (i < n4) p[i] = make_int4(0, 0, 0, 0);
}

// One thread per voxel slot: the mean's sort key and its cell's population.  A mean outside the exactness range of
// grid.h sends its scene to the scan; it still gets a key (cell 0) so that the sort stays whole.  Slots past the
// scene's voxel count take scene number Bc and no cell.
__global__ __launch_bounds__(PV_BLOCK) void pv_radius_keys_kernel(int N, int Bc, float inv_h,
                                                                  const int32_t* __restrict__ counts, PvWs ws) {
  const int b = blockIdx.y;
  const int v = blockIdx.x * PV_BLOCK + threadIdx.x;
  if (v >= N) return;
  const size_t i = (size_t)b * N + v;
  uint32_t key = (uint32_t)Bc << PV_CELL_BITS;
  if (v < pv_clamp(counts[(size_t)b * 3 + 1], N)) {
    const float4 o = ws.vox[(size_t)b * N], p = ws.vox[i];
    int cell = 0;
    if (grid_coord_ok(p.x, o.x, inv_h) && grid_coord_ok(p.y, o.y, inv_h) && grid_coord_ok(p.z, o.z, inv_h))
      cell = pv_cell(grid_coord(p.x, o.x, inv_h), grid_coord(p.y, o.y, inv_h), grid_coord(p.z, o.z, inv_h));
    else
      ws.flags[b] = 1;
    key = ((uint32_t)b << PV_CELL_BITS) | (uint32_t)cell;
    atomicAdd(&ws.count[(size_t)b * PV_CELLS + cell], 1);
  }
  ws.keys_a[i] = key;
  ws.vals_a[i] = (uint32_t)v;
}

// One thread per sorted record: the compact copy the counts read.  The records of the slots no cell holds lie behind
// the last scene's and are never read (they are filled all the same).
__global__ __launch_bounds__(PV_BLOCK) void pv_radius_order_kernel(int N, size_t n, int Bc, PvWs ws) {
  const size_t i = (size_t)blockIdx.x * PV_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = ws.keys_b[i] >> PV_CELL_BITS, v = ws.vals_b[i];
  const float nan = __int_as_float(0x7fc00000);
  float4 r = make_float4(nan, nan, nan, __int_as_float(0));
  if (s < (uint32_t)Bc && v < (uint32_t)N) {
    const float4 p = ws.vox[(size_t)s * N + v];
    r = make_float4(p.x, p.y, p.z, __int_as_float((int)v));
  }
  ws.rec[i] = r;
}

// One thread per sorted record: radius_count_kernel's count over the 27 cells (nine rows of three x-adjacent cells:
// one run of records each, two where the row wraps), or over the scene's means in index order.
template <bool FMAD>
__global__ __launch_bounds__(PV_BLOCK) void pv_radius_count_kernel(int N, size_t n, int Bc, float r2, float inv_h, int nb,
                                                                   const int32_t* __restrict__ counts, PvWs ws) {
  const size_t i = (size_t)blockIdx.x * PV_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t b = ws.keys_b[i] >> PV_CELL_BITS;
  if (b >= (uint32_t)Bc) return;   // a slot no cell holds
  const float4 q = ws.rec[i];
  const uint32_t v = (uint32_t)__float_as_int(q.w);
  if (v >= (uint32_t)N) return;    // (cannot happen: the values are the build's own)
  const float x = q.x, y = q.y, z = q.z;
  const float4* __restrict__ vox = ws.vox + (size_t)b * N;
  int cnt = 0;
  if (ws.flags[b] == 0) {          // every mean of the scene, this one included, is inside the exactness range
    const float4 o = vox[0];
    const int icx = grid_coord(x, o.x, inv_h), icy = grid_coord(y, o.y, inv_h), icz = grid_coord(z, o.z, inv_h);
    const int* __restrict__ start = ws.start + (size_t)b * PV_CELLS;   // offsets into the whole chunk's records
    const float4* __restrict__ rec = ws.rec;
    const int x0 = (icx - 1) & (PV_DIM - 1);
    // the query's own row first, then the four beside it, then the corners (3 (dz + 1) + dy + 1 = 4, 3, 5, 1, 7, 0,
    // 2, 6, 8): the count does not depend on the order, and the near records end it early
    for (int k = 0; k < 9 && cnt <= nb; ++k) {
      const int code = (int)((0x862071534ull >> (4 * k)) & 15);
      const int dz = code / 3 - 1, dy = code % 3 - 1;
      const int row = pv_cell(0, icy + dy, icz + dz);
      long long b0 = start[row + x0], e0, b1 = 0, e1 = 0;
      if (x0 <= PV_DIM - 3) {
        e0 = start[row + x0 + 3];
      } else {
        e0 = start[row + PV_DIM];
        b1 = start[row];
        e1 = start[row + ((x0 + 3) & (PV_DIM - 1))];
      }
      b0 = b0 < 0 ? 0 : b0;
      b1 = b1 < 0 ? 0 : b1;
      e0 = e0 > (long long)n ? (long long)n : e0;
      e1 = e1 > (long long)n ? (long long)n : e1;
      for (long long r = b0; r < e0 && cnt <= nb; ++r) {
        const float4 c = rec[r];
        cnt += dist2<FMAD>(x, y, z, c.x, c.y, c.z) < r2 ? 1 : 0;
      }
      for (long long r = b1; r < e1 && cnt <= nb; ++r) {
        const float4 c = rec[r];
        cnt += dist2<FMAD>(x, y, z, c.x, c.y, c.z) < r2 ? 1 : 0;
      }
    }
  } else {
    // toroidal aliasing is only ruled out inside the grid's exactness range: scan
    const int vc = pv_clamp(counts[(size_t)b * 3 + 1], N);
    for (int r = 0; r < vc && cnt <= nb; ++r) {
      const float4 c = vox[r];
      cnt += dist2<FMAD>(x, y, z, c.x, c.y, c.z) < r2 ? 1 : 0;
    }
  }
  ws.keep[(size_t)b * N + v] = cnt > nb ? 1 : 0;
}

// One workgroup per scene: the kept means in cell order, their trace, the count, and the padding behind them.
__global__ __launch_bounds__(PV_THREADS) void pv_finish_kernel(int N, PvWs ws, float* __restrict__ points,
                                                               int32_t* __restrict__ index,
                                                               int32_t* __restrict__ counts) {
  __shared__ int wave_cnt[PV_THREADS / 64];
  __shared__ int base_s;
  const int b = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int vc = pv_clamp(counts[(size_t)b * 3 + 1], N);
  const float4* __restrict__ vox = ws.vox + (size_t)b * N;
  const uint8_t* __restrict__ keep_b = ws.keep + (size_t)b * N;
  float* __restrict__ ox = points + (size_t)b * 3 * N;
  float* __restrict__ oy = ox + N;
  float* __restrict__ oz = ox + 2 * (size_t)N;
  int32_t* __restrict__ oi = index + (size_t)b * N;
  if (t == 0) base_s = 0;
  __syncthreads();
  for (int v0 = 0; v0 < vc; v0 += PV_THREADS) {   // vc is the workgroup's: the loop is uniform
    const int v = v0 + t;
    const bool keep = v < vc && keep_b[v] != 0;
    const uint64_t m = __ballot(keep);
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < PV_THREADS / 64; ++w) {
      const int c = wave_cnt[w];
      before += w < wave ? c : 0;
      total += c;
    }
    const int base = base_s;
    if (keep) {
      const float4 p = vox[v];
      const int pos = base + before + mask_rank(m);   // <= v < N
      ox[pos] = p.x;
      oy[pos] = p.y;
      oz[pos] = p.z;
      oi[pos] = __float_as_int(p.w);
    }
    __syncthreads();
    if (t == 0) base_s = base + total;
  }
  __syncthreads();
  const int kept = base_s;
  if (t == 0) counts[(size_t)b * 3 + 2] = kept;
  const float nan = __int_as_float(0x7fc00000);
  for (int k = kept + t; k < N; k += PV_THREADS) {
    ox[k] = nan;
    oy[k] = nan;
    oz[k] = nan;
    oi[k] = -1;
  }
}

}  // namespace s4g

extern "C" size_t s4g_process_views_workspace_bytes(int64_t B, int64_t N) {
  if (B <= 0 || N <= 0 || B > 65535 || B * N >= (1ll << 31)) return 0;
  return s4g::pv_ws(nullptr, s4g::pv_chunk_max(B, N), N, nullptr);
}

extern "C" int s4g_process_views_f32(const float* xyz_b3n, const int32_t* count_b, int64_t B, int64_t N,
                                     const float* workspace6, float voxel, const float* origin3, const int32_t* dims3,
                                     float radius, int32_t nb_points, float* points_out_b3n, int32_t* index_out_bn,
                                     int32_t* counts_out_b3, void* ws, size_t ws_bytes, int flags,
                                     s4g_stream_t stream) {
  using namespace s4g;
  if (B < 0 || B > 65535 || N < 0 || N >= (1ll << 31) || B * N >= (1ll << 31)) return S4G_EINVAL;
  if (!workspace6 || !origin3 || !dims3 || !(voxel > 0.f) || !(radius > 0.f) || !(radius < 1e18f) || nb_points < 0)
    return S4G_EINVAL;
  if (dims3[0] <= 0 || dims3[1] <= 0 || dims3[2] <= 0 ||
      (uint64_t)dims3[0] * (uint64_t)dims3[1] * (uint64_t)dims3[2] >= (1ull << 32))
    return S4G_EINVAL;
  for (int a = 0; a < 3; ++a) {
    if (!(fabsf(origin3[a]) <= FLT_MAX)) return S4G_EINVAL;
    // the grid must contain the crop box (the cell arithmetic is monotone: both faces inside, everything between
    // them inside); an empty or NaN box keeps nothing and asks nothing of the grid
    const float lo = workspace6[2 * a], hi = workspace6[2 * a + 1];
    if (lo < hi) {
      const float clo = floorf((float)(lo - origin3[a]) / voxel), chi = floorf((float)(hi - origin3[a]) / voxel);
      if (!(clo >= 0.f) || !(chi <= (float)(dims3[a] - 1))) return S4G_EINVAL;
    }
  }
  if (B == 0) return S4G_OK;
  if (!counts_out_b3) return S4G_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (N == 0) {
    hipLaunchKernelGGL(pv_zero_counts_kernel, dim3((unsigned)((3 * B + PV_BLOCK - 1) / PV_BLOCK)), dim3(PV_BLOCK), 0, st,
                       counts_out_b3, (int)(3 * B));
    S4G_LAUNCH_CHECK();
    return S4G_OK;
  }
  if (!xyz_b3n || !points_out_b3n || !index_out_bn) return S4G_EINVAL;
  const int64_t chunk_max = pv_chunk_max(B, N);
  if (!ws || ws_bytes < pv_ws(nullptr, chunk_max, N, nullptr)) return S4G_EWORKSPACE;
  const uint64_t cells = (uint64_t)dims3[0] * (uint64_t)dims3[1] * (uint64_t)dims3[2];
  const PvPlan plan = pv_plan(B, N, cells);
  PvWs w;
  pv_ws(ws, chunk_max, N, &w);
  const float r2 = radius * radius;                      // fp32 product, as for the ball query
  const float h = radius * (1.0f + 1.0f / 256.0f);       // cell edge slightly above the radius (grid.h)
  const float inv_h = 1.0f / h;
  const bool fmad = (flags & S4G_FLAG_FMAD) != 0;
  unsigned rbits = PV_CELL_BITS;                         // scene numbers 0 .. chunk: chunk itself marks the empty slots
  while (rbits < 32 && ((int64_t)1 << (rbits - PV_CELL_BITS)) < plan.chunk + 1) ++rbits;
  for (int64_t b0 = 0; b0 < B; b0 += plan.chunk) {
    const int64_t Bc = B - b0 < plan.chunk ? B - b0 : plan.chunk;
    const size_t n = (size_t)Bc * (size_t)N, gcells = (size_t)Bc * PV_CELLS + 1;
    const float* xyz = xyz_b3n + (size_t)b0 * 3 * N;
    int32_t* counts = counts_out_b3 + (size_t)b0 * 3;
    const unsigned nblocks = (unsigned)((n + PV_BLOCK - 1) / PV_BLOCK);
    const dim3 sgrid((unsigned)((N + PV_BLOCK - 1) / PV_BLOCK), (unsigned)Bc);
    hipLaunchKernelGGL(pv_crop_kernel, dim3((unsigned)Bc), dim3(PV_THREADS), 0, st, xyz,
                       count_b ? count_b + b0 : nullptr, (int)N, workspace6[0], workspace6[1], workspace6[2],
                       workspace6[3], workspace6[4], workspace6[5], w.crop, counts);
    S4G_LAUNCH_CHECK();
    hipLaunchKernelGGL(pv_voxel_keys_kernel, sgrid, dim3(PV_BLOCK), 0, st, xyz, (int)N, origin3[0], origin3[1],
                       origin3[2], voxel, dims3[0], dims3[1], dims3[2], plan.cell_bits, plan.dead, counts, w);
    S4G_LAUNCH_CHECK();
    if (int rc = radix_sort_pairs(w.sort, radix_sort_ws_bytes(n), w.keys_a, w.keys_b, w.vals_a, w.vals_b, n, plan.bits,
                                  st))
      return rc;
    hipLaunchKernelGGL(pv_heads_kernel, dim3(nblocks), dim3(PV_BLOCK), 0, st, w.keys_b, n, plan.dead, w.head);
    S4G_LAUNCH_CHECK();
    if (int rc = exclusive_scan_i32(w.scan, w.scan_bytes, w.head, w.rank, n, st)) return rc;
    hipLaunchKernelGGL(pv_segments_kernel, dim3((unsigned)((Bc + PV_BLOCK - 1) / PV_BLOCK)), dim3(PV_BLOCK), 0, st,
                       w.keys_b, n, (int)Bc, (int)N, plan.cell_bits, plan.dead, w.head, w.rank, w.vbase, counts);
    S4G_LAUNCH_CHECK();
    hipLaunchKernelGGL(pv_voxel_mean_kernel, dim3(nblocks), dim3(PV_BLOCK), 0, st, xyz, (int)N, n, (int)Bc,
                       plan.cell_bits, w);
    S4G_LAUNCH_CHECK();
    const size_t n4 = pv_clear_int4(Bc);
    hipLaunchKernelGGL(pv_clear_kernel, dim3((unsigned)((n4 + PV_BLOCK - 1) / PV_BLOCK)), dim3(PV_BLOCK), 0, st,
                       (int4*)w.count, n4);
    S4G_LAUNCH_CHECK();
    PvWs wr = w;
    wr.flags = w.count + gcells;   // cleared with the populations above
    hipLaunchKernelGGL(pv_radius_keys_kernel, sgrid, dim3(PV_BLOCK), 0, st, (int)N, (int)Bc, inv_h, counts, wr);
    S4G_LAUNCH_CHECK();
    if (int rc = radix_sort_pairs(w.sort, radix_sort_ws_bytes(n), w.keys_a, w.keys_b, w.vals_a, w.vals_b, n, rbits, st))
      return rc;
    if (int rc = exclusive_scan_i32(w.scan, w.scan_bytes, w.count, w.start, gcells, st)) return rc;
    hipLaunchKernelGGL(pv_radius_order_kernel, dim3(nblocks), dim3(PV_BLOCK), 0, st, (int)N, n, (int)Bc, wr);
    S4G_LAUNCH_CHECK();
    if (fmad)
      hipLaunchKernelGGL(pv_radius_count_kernel<true>, dim3(nblocks), dim3(PV_BLOCK), 0, st, (int)N, n, (int)Bc, r2,
                         inv_h, (int)nb_points, counts, wr);
    else
      hipLaunchKernelGGL(pv_radius_count_kernel<false>, dim3(nblocks), dim3(PV_BLOCK), 0, st, (int)N, n, (int)Bc, r2,
                         inv_h, (int)nb_points, counts, wr);
    S4G_LAUNCH_CHECK();
    hipLaunchKernelGGL(pv_finish_kernel, dim3((unsigned)Bc), dim3(PV_THREADS), 0, st, (int)N, wr,
                       points_out_b3n + (size_t)b0 * 3 * N, index_out_bn + (size_t)b0 * N, counts);
    S4G_LAUNCH_CHECK();
  }
  return S4G_OK;
}
