// The inputs of the two baselines the paper compares against (GPD's 12-channel projection maps, PointNetGPD's close-region
// point sets): restates TorchBaseLineSingleViewPointCloud.finger_hand's best-placement fold and crop
// (data_gen/pcd_classes/torch_baseline_single_view_point_cloud.py:220-331) and close_region_projection (:334-393), and
// the crop of torch_precomputed_baseline.py:350-383, for every frame of every scene without host synchronisation.
//
//   cr_best_kernel     per frame: the first of the L*T placements whose score is > 0 and > every earlier one (:308-312), the
//                      validity line (:323) and LOCAL_TO_LOCAL_SEARCH[i] @ [R^T | -R^T p] (:320-322), formed directly
//   compact_valid_kernel (frame_sweep.h)  valid_index and count per scene
//   cr_count_kernel    a cloud sweep (frame_sweep.h): per (frame, point chunk) the points of the close region and whether a
//                      kept point or normal is not finite
//   cr_scan_kernel     per scene, the exclusive scan in (frame, chunk) order: count, offset (int64), flags, and where in
//                      the packed buffers every chunk of a stored frame starts
//   cr_fill_kernel     the same sweep again: point, normal and source index of every member, in ascending point index.  A
//                      sweep holds the points i0 + 256 u + 64 wave + lane: the ballot rank inside a wave plus the
//                      prefix over (u, wave), kept in LDS, is the member's place
//   cr_maps_kernel     one workgroup per stored frame: voxels floor(c / unit), per voxel the count and the three normal
//                      sums, then the three projections.  The grid is walked in tiles of one x slab and 32 y rows
//                      (2 048 voxels in LDS: 60^3 voxels of four values do not fit); the set is binned by tile first so
//                      that a tile reads its own points only.  Rows of map 0 finish inside a tile, columns of map 2
//                      inside a slab, map 1 is kept in registers over the slabs in ascending x.
//
// Order independence: the counts are integers and the normal sums are integers of scale 2^-30 (each component clamped to
// [-4, 4], as the band sums of local_search.hip), added with integer atomics; everything after them runs in a fixed
// order.  No floating-point atomics: results are bit-identical from run to run and batch invariant.
#include "frame_sweep.h"

namespace s4g {

constexpr int CR_GX = 32;            // workgroups that share a scene's frame list
constexpr int CR_U = 4;              // points per lane and sweep: a sweep is 1 024 points
constexpr int CR_SLOTS = 8;          // frames per workgroup and pass: 256 per scene and pass
constexpr int CR_CHUNK_POINTS = 16384;   // point ranges per scene: ceil(N / 16 384) within [4, 64]
constexpr int CR_MIN_CHUNKS = 4;
constexpr int CR_MAX_CHUNKS = 64;
constexpr int CR_MAX_R = 64;         // compiled maximum of the projection resolution
constexpr int CR_TILE_Y = 32;        // y rows of a voxel tile
constexpr float CR_FIX = 1073741824.0f;  // 2^30

struct CrParams {
  float x_lo, x_hi, hbs, hht;        // the region: x_lo < x < x_hi, |y| < hbs, |z| < hht
  float unit[3], h0[3], hstep[3];    // voxel edge per axis; height of voxel k on an axis = h0 + k * hstep
  int R;
};

__device__ __forceinline__ bool cr_member(const LocalPoint& l, const CrParams& p) {
  return (l.x > p.x_lo) && (l.x < p.x_hi) && (fabsf(l.y) < p.hbs) && (fabsf(l.z) < p.hht);
}

// is row k of scene b a frame that is scanned?  (k is below the scene's frame count already)
__device__ __forceinline__ bool cr_live(const int* __restrict__ live, size_t row) { return !live || live[row] != 0; }

// the frame's rotation applied to a normal
__device__ __forceinline__ LocalPoint cr_normal(const float* __restrict__ g, float x, float y, float z) {
  LocalPoint l;
  l.x = g[0] * x + g[1] * y + g[2] * z;
  l.y = g[4] * x + g[5] * y + g[6] * z;
  l.z = g[8] * x + g[9] * y + g[10] * z;
  return l;
}

__global__ __launch_bounds__(256) void cr_best_kernel(
    const float* __restrict__ points, const float* __restrict__ frames, const float* __restrict__ scores,
    const float* __restrict__ tables, int rows, int L, int T, int* __restrict__ index, float* __restrict__ score,
    float* __restrict__ g2l) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  const int P = L * T;
  const float* s = scores + (size_t)row * P;
  float best = 0.f;                                                                  // the zeroed slot (:74)
  int bi = -1;
  for (int i = 0; i < P; ++i) {
    const float v = s[i];
    if (v > best) { best = v; bi = i; }                                              // :308-309; false for a NaN
  }
  const bool ok = bi >= 0 && !(best < 1e-4f);                                        // :323
  index[row] = ok ? bi : -1;
  score[row] = best;
  float* o = g2l + (size_t)row * 16;
  if (!ok) {
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = 0.f;
    return;
  }
  const float* r = frames + (size_t)row * 9;
  const float px = points[(size_t)row * 3], py = points[(size_t)row * 3 + 1], pz = points[(size_t)row * 3 + 2];
  best_placement_g2l(r, px, py, pz, tables, L, T, bi, o);         // (frame_sweep.h, as text)
}

// the tables of a pass: rows 0..2 of the frames' matrices
__device__ __forceinline__ void cr_load_frame(const float* __restrict__ g2l, size_t row, float* __restrict__ o) {
  const float* G = g2l + row * 16;
#pragma unroll
  for (int c = 0; c < 12; ++c) o[c] = G[c];
}

// cnt, nf (B, F, C): written for every row below the scene's frame count, by the one workgroup that owns (row, chunk)
__global__ __launch_bounds__(256) void cr_count_kernel(
    const float* __restrict__ g2l, const float* __restrict__ xyz, const float* __restrict__ normals,
    const int* __restrict__ live, const int64_t* __restrict__ frame_count, int N, int F, CrParams p,
    int* __restrict__ cnt, int* __restrict__ nf) {
  __shared__ float gl[CR_SLOTS][12];
  __shared__ int slive[CR_SLOTS], scnt[CR_SLOTS], snf[CR_SLOTS];
  const int b = blockIdx.z, t = threadIdx.x, lane = t & 63, C = gridDim.y;
  const float* px = xyz + (size_t)b * 3 * N;
  const float* pn = normals + (size_t)b * 3 * N;
  const ChunkRange rg = chunk_range(N);
  const int fmax = frame_rows(frame_count, b, F);
  for (int j0 = 0; blockIdx.x + CR_GX * j0 < fmax; j0 += CR_SLOTS) {
    __syncthreads();
    const int nslot = pass_slots(fmax, CR_GX, j0, CR_SLOTS);
    if (t < nslot) {
      const size_t row = (size_t)b * F + blockIdx.x + CR_GX * (j0 + t);
      cr_load_frame(g2l, row, gl[t]);
      slive[t] = cr_live(live, row) ? 1 : 0;
      scnt[t] = 0;
      snf[t] = 0;
    }
    __syncthreads();
    if (!rg.empty()) {
      for (int base0 = rg.lo; base0 < rg.hi; base0 += 256 * CR_U) {      // workgroup-uniform: every wave is fully active
        PointBlock<CR_U> pt;
        pt.load(px, N, base0 + t, rg.hi);
        for (int sl = 0; sl < nslot; ++sl) {
          if (!slive[sl]) continue;
          float g[12];
#pragma unroll
          for (int c = 0; c < 12; ++c) g[c] = gl[sl][c];
          int n = 0;
#pragma unroll
          for (int u = 0; u < CR_U; ++u) {
            const LocalPoint l = local_point(g, pt.x[u], pt.y[u], pt.z[u]);
            const bool in = pt.in[u] && cr_member(l, p);
            n += __popcll(__ballot(in));
            if (in) {
              const int i = pt.idx[u];
              const LocalPoint m = cr_normal(g, pn[i], pn[(size_t)N + i], pn[2 * (size_t)N + i]);
              const bool good = finite(l.x) && finite(l.y + p.hbs) && finite(l.z + p.hht) && finite(m.x) &&
                                finite(m.y) && finite(m.z);
              if (!good) atomicOr(&snf[sl], 1);
            }
          }
          if (lane == 0 && n) atomicAdd(&scnt[sl], n);
        }
      }
    }
    __syncthreads();
    if (t < nslot) {
      const size_t o = ((size_t)b * F + blockIdx.x + CR_GX * (j0 + t)) * C + blockIdx.y;
      cnt[o] = scnt[t];
      nf[o] = snf[t];
    }
  }
}

// one workgroup per scene.  base (B, F, C): where chunk c of frame f starts in the scene's packed buffers, -1 where the
// frame is not stored
__global__ __launch_bounds__(256) void cr_scan_kernel(
    const int* __restrict__ cnt, const int* __restrict__ nf, const int* __restrict__ live,
    const int64_t* __restrict__ frame_count, int F, int C, int64_t capacity, int* __restrict__ count,
    int64_t* __restrict__ offset, int* __restrict__ flags, int* __restrict__ base) {
  __shared__ long long st[256];
  __shared__ long long carry;
  const int b = blockIdx.x, t = threadIdx.x;
  const int fmax = frame_rows(frame_count, b, F);
  if (t == 0) carry = 0;
  __syncthreads();
  for (int f0 = 0; f0 < F; f0 += 256) {
    const int f = f0 + t;
    const size_t row = (size_t)b * F + f;
    const bool alive = f < fmax && cr_live(live, row);
    long long tot = 0;
    int bad = 0;
    if (alive) {
      for (int c = 0; c < C; ++c) {
        tot += cnt[row * C + c];
        bad |= nf[row * C + c];
      }
    }
    st[t] = tot;
    __syncthreads();
    long long pre = carry;
    for (int i = 0; i < t; ++i) pre += st[i];
    if (f < F) {
      const long long end = pre + tot;
      const bool fits = end <= (long long)capacity;
      count[row] = (int)tot;
      offset[(size_t)b * (F + 1) + f] = pre;
      flags[row] = alive ? ((fits ? 0 : 1) | (bad ? 2 : 0)) : 0;
      long long run = pre;
      for (int c = 0; c < C; ++c) {
        base[row * C + c] = (alive && fits) ? (int)run : -1;
        if (alive) run += cnt[row * C + c];
      }
    }
    __syncthreads();
    if (t == 255) carry = pre + tot;
    __syncthreads();
  }
  if (t == 0) offset[(size_t)b * (F + 1) + F] = carry;
}

__global__ __launch_bounds__(256) void cr_fill_kernel(
    const float* __restrict__ g2l, const float* __restrict__ xyz, const float* __restrict__ normals,
    const int* __restrict__ live, const int64_t* __restrict__ frame_count, int N, int F, CrParams p,
    const int* __restrict__ base, int64_t capacity, float* __restrict__ out_p, float* __restrict__ out_n,
    int* __restrict__ out_i) {
  __shared__ float gl[CR_SLOTS][12];
  __shared__ int slive[CR_SLOTS];
  __shared__ int pos[2][CR_SLOTS];
  __shared__ int wcnt[2][CR_SLOTS][CR_U * 4];       // members per (u, wave) of the sweep, in the order of the point index
  const int b = blockIdx.z, t = threadIdx.x, lane = t & 63, wave = t >> 6, C = gridDim.y;
  const float* px = xyz + (size_t)b * 3 * N;
  const float* pn = normals + (size_t)b * 3 * N;
  const size_t cap = (size_t)capacity;
  float* op = out_p + (size_t)b * 3 * cap;
  float* on = out_n + (size_t)b * 3 * cap;
  int* oi = out_i + (size_t)b * cap;
  const ChunkRange rg = chunk_range(N);
  if (rg.empty()) return;                             // workgroup-uniform, before any barrier
  const int fmax = frame_rows(frame_count, b, F);
  for (int j0 = 0; blockIdx.x + CR_GX * j0 < fmax; j0 += CR_SLOTS) {
    __syncthreads();
    const int nslot = pass_slots(fmax, CR_GX, j0, CR_SLOTS);
    if (t < nslot) {
      const size_t row = (size_t)b * F + blockIdx.x + CR_GX * (j0 + t);
      cr_load_frame(g2l, row, gl[t]);
      const int bs = cr_live(live, row) ? base[row * C + blockIdx.y] : -1;
      slive[t] = bs >= 0 ? 1 : 0;
      pos[0][t] = bs;
    }
    __syncthreads();
    int any = 0;
    for (int sl = 0; sl < nslot; ++sl) any |= slive[sl];
    if (!any) continue;                               // workgroup-uniform: no frame of the pass is stored
    int par = 0;
    for (int base0 = rg.lo; base0 < rg.hi; base0 += 256 * CR_U, par ^= 1) {
      PointBlock<CR_U> pt;
      pt.load(px, N, base0 + t, rg.hi);
      unsigned keep[CR_U];
#pragma unroll
      for (int u = 0; u < CR_U; ++u) keep[u] = 0u;
      for (int sl = 0; sl < nslot; ++sl) {
        if (!slive[sl]) continue;
        float g[12];
#pragma unroll
        for (int c = 0; c < 12; ++c) g[c] = gl[sl][c];
#pragma unroll
        for (int u = 0; u < CR_U; ++u) {
          const LocalPoint l = local_point(g, pt.x[u], pt.y[u], pt.z[u]);
          const bool in = pt.in[u] && cr_member(l, p);
          const uint64_t m = __ballot(in);
          keep[u] |= (in ? 1u : 0u) << sl;
          if (lane == 0) wcnt[par][sl][u * 4 + wave] = __popcll(m);
        }
      }
      __syncthreads();
      for (int sl = 0; sl < nslot; ++sl) {
        if (!slive[sl]) continue;
        const int* w = wcnt[par][sl];
#pragma unroll
        for (int u = 0; u < CR_U; ++u) {
          const bool in = (keep[u] >> sl) & 1u;
          const uint64_t m = __ballot(in);
          if (!m) continue;                           // wave-uniform
          if (in) {
            int o = pos[par][sl] + mask_rank(m);
            for (int e = 0; e < u * 4 + wave; ++e) o += w[e];
            float g[12];
#pragma unroll
            for (int c = 0; c < 12; ++c) g[c] = gl[sl][c];
            const LocalPoint l = local_point(g, pt.x[u], pt.y[u], pt.z[u]);      // the bits the ballot above was taken on
            const int i = pt.idx[u];
            const LocalPoint q = cr_normal(g, pn[i], pn[(size_t)N + i], pn[2 * (size_t)N + i]);
            if ((size_t)o < cap) {                    // (holds for every stored frame: the scan kernel checked the end)
              op[o] = l.x; op[cap + o] = l.y + p.hbs; op[2 * cap + o] = l.z + p.hht;     // :314-315
              on[o] = q.x; on[cap + o] = q.y; on[2 * cap + o] = q.z;
              oi[o] = i;
            }
          }
        }
        if (t == sl) {
          int n = pos[par][sl];
          for (int e = 0; e < CR_U * 4; ++e) n += w[e];
          pos[par ^ 1][sl] = n;
        }
      }
    }
  }
}

// one workgroup per frame.  vkey, vbin (B, capacity): the voxel of every stored point and the points sorted by tile
__global__ __launch_bounds__(256) void cr_maps_kernel(
    const int* __restrict__ count, const int64_t* __restrict__ offset, const int* __restrict__ flags,
    const float* __restrict__ pts, const float* __restrict__ nrm, int F, int64_t capacity, CrParams p,
    int* __restrict__ vkey, int* __restrict__ vbin, float* __restrict__ maps) {
  __shared__ int cnt[CR_TILE_Y][CR_MAX_R];
  __shared__ long long sm[3][CR_TILE_Y][CR_MAX_R];
  __shared__ int hist[2 * CR_MAX_R], start[2 * CR_MAX_R], cursor[2 * CR_MAX_R];
  __shared__ float partf[4][CR_MAX_R][3];
  __shared__ int parti[4][CR_MAX_R][2];
  const int f = blockIdx.x, b = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const size_t row = (size_t)b * F + f;
  const int R = p.R, RR = R * R;
  float* out = maps + row * 12 * (size_t)RR;
  for (int i = t; i < 12 * RR; i += 256) out[i] = 0.f;
  const int n = count[row];
  if (flags[row] != 0 || n <= 0) return;              // workgroup-uniform: not stored, not finite, empty or not a frame
  const size_t cap = (size_t)capacity;
  const size_t off = (size_t)offset[(size_t)b * (F + 1) + f];
  const float* P = pts + (size_t)b * 3 * cap + off;
  const float* Q = nrm + (size_t)b * 3 * cap + off;
  int* key = vkey + (size_t)b * cap + off;
  int* bin = vbin + (size_t)b * cap + off;
  if (t < 2 * CR_MAX_R) hist[t] = 0;
  for (int i = t; i < CR_TILE_Y * CR_MAX_R; i += 256) {
    ((int*)cnt)[i] = 0;
    ((long long*)sm)[i] = 0; ((long long*)sm)[CR_TILE_Y * CR_MAX_R + i] = 0; ((long long*)sm)[2 * CR_TILE_Y * CR_MAX_R + i] = 0;
  }
  __syncthreads();
  const float fR = (float)R;
  for (int j = t; j < n; j += 256) {
    // floor(c / unit): an fp32 division by the fp32 unit (what torch computes on the CPU, :343-349)
    const float qx = floorf(__fdiv_rn(P[j], p.unit[0]));
    const float qy = floorf(__fdiv_rn(P[cap + j], p.unit[1]));
    const float qz = floorf(__fdiv_rn(P[2 * cap + j], p.unit[2]));
    const bool ok = qx >= 0.f && qx < fR && qy >= 0.f && qy < fR && qz >= 0.f && qz < fR;     // :351-352
    int k = -1;
    if (ok) {
      const int ix = (int)qx, iy = (int)qy, iz = (int)qz;
      k = ix | (iy << 8) | (iz << 16);
      atomicAdd(&hist[2 * ix + iy / CR_TILE_Y], 1);
    }
    key[j] = k;
  }
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int i = 0; i < 2 * CR_MAX_R; ++i) { start[i] = cursor[i] = run; run += hist[i]; }
  }
  __syncthreads();
  for (int j = t; j < n; j += 256) {
    const int k = key[j];
    if (k >= 0) bin[atomicAdd(&cursor[2 * (k & 255) + ((k >> 8) & 255) / CR_TILE_Y], 1)] = j;   // any order: the sums are integers
  }
  __syncthreads();
  // map 1, pixel (y, z) summed along x: this thread owns z = lane and y = 4 j + wave
  int a1n[16];                                        // occupied voxels on the line (bits 0..7) and the sum of their x index
  float a1s[16][3];
#pragma unroll
  for (int j = 0; j < 16; ++j) { a1n[j] = 0; a1s[j][0] = a1s[j][1] = a1s[j][2] = 0.f; }
  for (int x = 0; x < R; ++x) {
    if (hist[2 * x] + hist[2 * x + 1] == 0) continue;  // workgroup-uniform
    int occ2 = 0, sumk2 = 0;                           // map 2, pixel (z, x) summed along y: this thread's rows of it
    float s2[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int ns = hist[2 * x + h];
      if (ns == 0) continue;                           // workgroup-uniform
      const int s0 = start[2 * x + h];
      for (int i = t; i < ns; i += 256) {
        const int j = bin[s0 + i];
        const int k = key[j];
        const int yl = ((k >> 8) & 255) % CR_TILE_Y, iz = k >> 16;
        atomicAdd(&cnt[yl][iz], 1);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float v = fminf(fmaxf(Q[c * cap + j], -4.0f), 4.0f);
          atomicAdd((unsigned long long*)&sm[c][yl][iz], (unsigned long long)__float2ll_rn(v * CR_FIX));
        }
      }
      __syncthreads();
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const int yl = 4 * jj + wave;
        const int v = cnt[yl][lane];
        if (!__ballot(v > 0)) continue;                // wave-uniform: an empty row
        const int occ = v > 0 ? 1 : 0;
        float mean[3] = {0.f, 0.f, 0.f};
        if (occ) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            mean[c] = (float)((double)sm[c][yl][lane] * (1.0 / (double)CR_FIX) / (double)v);     // :374
            sm[c][yl][lane] = 0;
          }
          cnt[yl][lane] = 0;                           // the tile is left clean for the next one
        }
        const int j = 8 * h + jj;
        a1n[j] += occ ? (1 | (x << 8)) : 0;
        occ2 += occ;
        sumk2 += occ ? CR_TILE_Y * h + yl : 0;
        int ro = occ, rk = occ ? lane : 0;
        float rs[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          a1s[j][c] = a1s[j][c] + mean[c];
          s2[c] = s2[c] + mean[c];
          rs[c] = mean[c];
        }
        // map 0, pixel (x, y) summed along z: the lanes of this wave, a fixed butterfly
        for (int d = 32; d >= 1; d >>= 1) {
          ro += __shfl_xor(ro, d);
          rk += __shfl_xor(rk, d);
#pragma unroll
          for (int c = 0; c < 3; ++c) rs[c] = rs[c] + __shfl_xor(rs[c], d);
        }
        if (lane == 0) {
          const size_t o = (size_t)x * R + CR_TILE_Y * h + yl;
          const float fo = (float)ro;
          out[o] = __fdiv_rn((float)ro * p.h0[2] + p.hstep[2] * (float)rk, fo);                   // :388
#pragma unroll
          for (int c = 0; c < 3; ++c) out[(size_t)(1 + c) * RR + o] = __fdiv_rn(rs[c], fo);     // :387
        }
      }
      __syncthreads();
    }
    parti[wave][lane][0] = occ2; parti[wave][lane][1] = sumk2;
#pragma unroll
    for (int c = 0; c < 3; ++c) partf[wave][lane][c] = s2[c];
    __syncthreads();
    if (t < R) {
      int ro = 0, rk = 0;
      float rs[3] = {0.f, 0.f, 0.f};
      for (int w = 0; w < 4; ++w) {
        ro += parti[w][t][0]; rk += parti[w][t][1];
#pragma unroll
        for (int c = 0; c < 3; ++c) rs[c] = rs[c] + partf[w][t][c];
      }
      if (ro > 0) {
        const size_t o = (size_t)8 * RR + (size_t)t * R + x;
        const float fo = (float)ro;
        out[o] = __fdiv_rn((float)ro * p.h0[1] + p.hstep[1] * (float)rk, fo);
#pragma unroll
        for (int c = 0; c < 3; ++c) out[(size_t)(1 + c) * RR + o] = __fdiv_rn(rs[c], fo);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int y = 4 * j + wave, ro = a1n[j] & 255, rk = a1n[j] >> 8;
    if (y < R && lane < R && ro > 0) {
      const size_t o = (size_t)4 * RR + (size_t)y * R + lane;
      const float fo = (float)ro;
      out[o] = __fdiv_rn((float)ro * p.h0[0] + p.hstep[0] * (float)rk, fo);
#pragma unroll
      for (int c = 0; c < 3; ++c) out[(size_t)(1 + c) * RR + o] = __fdiv_rn(a1s[j][c], fo);
    }
  }
}

struct CrLayout {
  size_t cnt, nf, base, vkey, vbin, total;            // byte offsets
};
static inline CrLayout cr_layout(size_t B, size_t F, size_t C, size_t capacity) {
  CrLayout o;
  const size_t per = align256(B * F * C * sizeof(int));
  o.cnt = 0;
  o.nf = per;
  o.base = 2 * per;
  o.vkey = 3 * per;
  o.vbin = o.vkey + align256(B * capacity * sizeof(int));
  o.total = o.vbin + align256(B * capacity * sizeof(int));
  return o;
}

static inline bool cr_sizes_ok(int64_t B, int64_t N, int64_t F, int64_t capacity) {
  return B >= 0 && F >= 0 && N > 0 && capacity >= 0 && B <= 65535 && F <= 65535 && N < (1ll << 31) - 2048 &&
         capacity < (1ll << 31);
}

}  // namespace s4g

extern "C" int s4g_best_placement_f32(const float* points_bf3, const float* frames_bf33, const float* scores_bfp,
                                      const float* tables_3l2t, int64_t B, int64_t F, int64_t L, int64_t T,
                                      int32_t* index_bf, float* score_bf, float* g2l_bf44, int32_t* valid_index_bf,
                                      int64_t* count_b, s4g_stream_t stream) {
  using namespace s4g;
  if (B < 0 || F < 0 || B > 65535 || F > 65535 || L <= 0 || T <= 0 || L > 8 || T > 16) return S4G_EINVAL;
  if (B == 0) return S4G_OK;
  if (!count_b) return S4G_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (F == 0) {
    hipError_t e = hipMemsetAsync(count_b, 0, (size_t)B * sizeof(int64_t), st);
    return e == hipSuccess ? S4G_OK : (int)e;
  }
  if (!points_bf3 || !frames_bf33 || !scores_bfp || !tables_3l2t || !index_bf || !score_bf || !g2l_bf44 ||
      !valid_index_bf)
    return S4G_EINVAL;
  const int rows = (int)(B * F);
  hipLaunchKernelGGL(cr_best_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, points_bf3, frames_bf33,
                     scores_bfp, tables_3l2t, rows, (int)L, (int)T, (int*)index_bf, score_bf, g2l_bf44);
  S4G_LAUNCH_CHECK();
  hipLaunchKernelGGL(compact_valid_kernel<KeepNonNegative>, dim3((unsigned)B), dim3(256), 0, st, (const int*)index_bf,
                     (int)F, (int*)valid_index_bf, count_b);
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}

extern "C" size_t s4g_close_region_workspace_bytes(int64_t B, int64_t N, int64_t F, int64_t capacity) {
  using namespace s4g;
  if (!cr_sizes_ok(B, N, F, capacity) || B == 0 || F == 0) return 0;
  const int C = sweep_chunks(N, CR_CHUNK_POINTS, CR_MIN_CHUNKS, CR_MAX_CHUNKS);
  return cr_layout((size_t)B, (size_t)F, (size_t)C, (size_t)capacity).total;
}

extern "C" int s4g_close_region_f32(const float* g2l_bf44, const float* xyz_b3n, const float* normals_b3n,
                                    const int32_t* live_bf, const int64_t* frame_count_b, int64_t B, int64_t N,
                                    int64_t F, int64_t capacity, int64_t R, const float* params13,
                                    int32_t* count_bf, int64_t* offset_bf1, float* points_b3c, float* normals_b3c,
                                    int32_t* index_bc, float* maps_bf12rr, int32_t* flags_bf, void* workspace,
                                    size_t workspace_bytes, s4g_stream_t stream) {
  using namespace s4g;
  if (!cr_sizes_ok(B, N, F, capacity) || R < 2 || R > CR_MAX_R || !params13) return S4G_EINVAL;
  if (B == 0) return S4G_OK;
  if (!offset_bf1) return S4G_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (F == 0) {
    hipError_t e = hipMemsetAsync(offset_bf1, 0, (size_t)B * sizeof(int64_t), st);
    return e == hipSuccess ? S4G_OK : (int)e;
  }
  if (!g2l_bf44 || !xyz_b3n || !normals_b3n || !count_bf || !maps_bf12rr || !flags_bf) return S4G_EINVAL;
  if (capacity > 0 && (!points_b3c || !normals_b3c || !index_bc)) return S4G_EINVAL;
  if (!workspace || workspace_bytes < s4g_close_region_workspace_bytes(B, N, F, capacity)) return S4G_EWORKSPACE;
  CrParams p;
  p.x_lo = params13[0]; p.x_hi = params13[1]; p.hbs = params13[2]; p.hht = params13[3];
  for (int a = 0; a < 3; ++a) {
    p.unit[a] = params13[4 + a]; p.h0[a] = params13[7 + a]; p.hstep[a] = params13[10 + a];
    if (!(p.unit[a] > 0.f)) return S4G_EINVAL;
  }
  p.R = (int)R;
  const int C = sweep_chunks(N, CR_CHUNK_POINTS, CR_MIN_CHUNKS, CR_MAX_CHUNKS);
  const CrLayout lay = cr_layout((size_t)B, (size_t)F, (size_t)C, (size_t)capacity);
  char* ws = (char*)workspace;
  int* cnt = (int*)(ws + lay.cnt);
  int* nf = (int*)(ws + lay.nf);
  int* base = (int*)(ws + lay.base);
  int* vkey = (int*)(ws + lay.vkey);
  int* vbin = (int*)(ws + lay.vbin);
  const dim3 grid(CR_GX, (unsigned)C, (unsigned)B);
  hipLaunchKernelGGL(cr_count_kernel, grid, dim3(256), 0, st, g2l_bf44, xyz_b3n, normals_b3n, (const int*)live_bf,
                     frame_count_b, (int)N, (int)F, p, cnt, nf);
  S4G_LAUNCH_CHECK();
  hipLaunchKernelGGL(cr_scan_kernel, dim3((unsigned)B), dim3(256), 0, st, (const int*)cnt, (const int*)nf,
                     (const int*)live_bf, frame_count_b, (int)F, C, capacity, (int*)count_bf, offset_bf1,
                     (int*)flags_bf, base);
  S4G_LAUNCH_CHECK();
  if (capacity > 0) {
    hipLaunchKernelGGL(cr_fill_kernel, grid, dim3(256), 0, st, g2l_bf44, xyz_b3n, normals_b3n, (const int*)live_bf,
                       frame_count_b, (int)N, (int)F, p, (const int*)base, capacity, points_b3c, normals_b3c,
                       (int*)index_bc);
    S4G_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(cr_maps_kernel, dim3((unsigned)F, (unsigned)B), dim3(256), 0, st, (const int*)count_bf,
                     (const int64_t*)offset_bf1, (const int*)flags_bf, (const float*)points_b3c,
                     (const float*)normals_b3c, (int)F, capacity, p, vkey, vbin, maps_bf12rr);
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}
