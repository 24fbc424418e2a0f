// PointNetClassifier (inference/grasp_proposal/network_models/models/PointNetGPD.py, eval mode, BatchNorm folded by
// the caller) on variable-length point sets that are read where they lie:
//   STN trunk     x (3, n) -> relu 64 -> relu 128 -> relu 1024 -> max over the set          "stn_global"
//   STN head      1024 -> relu 512 -> relu 256 -> 9, + I                                    "trans" (3, 3)
//   feature trunk x^T trans -> relu 64 -> relu 128 -> 1024 (NO ReLU) -> max over the set    "global"
//   head          1024 -> relu 512 -> relu 256 ("hidden") -> classes                        logits
//
// Point j, coordinate c of set g lies at points + base[g] + c * cstride + j; base and len are formed on the device
// (prep_kernel) from offset / count / flags / index, or trivially for the dense form.
//
// TILE LIST.  A tile is T = 128 consecutive points of ONE set; set g has ceil(len / T) tiles, none when it is not in
// state 0.  scan_kernel turns the counts into tile_start[0 .. n]; the trunk kernel runs a fixed grid whose workgroups
// stride over the tiles (surplus workgroups find none and exit) and find a tile's set by bisection.  Rows of a tile
// past the end of its set repeat the set's last point, which changes no maximum; 32-row blocks that hold only such
// rows are skipped.
//
// A trunk tile: the 3 -> 64 layer in fp32 FMAs (x, y, z order, then the bias) into an f16x2 LDS panel; 64 -> 128 on
// v_mfma_f32_32x32x16_f16 in the TRANSPOSED form (A = weights, B = points), so that a lane's four accumulators of a
// group are four consecutive channels of one point and go to the next panel as one 8-byte write per plane; 128 -> 1024
// in the normal form (A = points from LDS, B = weights held in registers, two channel tiles per A read), so that the
// maximum over the rows is a maximum over a lane's 16 accumulators and one exchange between the half waves.  The
// 64- and 128-wide intermediates never leave LDS.  One integer atomicMax per (tile, channel) on the order-preserving
// key of the fp32 bits (negative values: all bits flipped; others: sign bit set; 0 = "nothing yet") merges the tiles
// of a set: exact, order independent, deterministic.
//
// T = 128: W of the 128 -> 1024 layer (512 KB in two planes) is streamed once per 128 rows.  The panels take
// 2 * 128 * (144 + 272) B = 104 KiB, one workgroup of eight waves per CU; T = 256 does not fit the 160 KiB.
//
// The transform is never applied to the points: the STN tail writes the set's own first layer W1 trans^T (64 x 3).
//
// SCALES are powers of two and PER SET: from the set's largest coordinate magnitude and bounds (max |x| * max row sum
// |w| + max |b|, chained) formed from it and from constants of the weights computed at pack time -- for the feature
// trunk's first layer from the set's own folded weights; the per-set layers from the largest magnitude of the set's
// own 1024 maxima.  Nothing a set's kernels read depends on another set and every accumulation order is fixed by the
// code: rows are bit-identical alone, in any batch, at any position, for any chunk, dense or packed, run to run.
//
// Set states: 0 = normal; 1 = the set holds a NaN or an infinity (nothing of it is staged; every output row is NaN);
// 2 = not scored (index -1 or out of range, count 0, flags bit 0, or a slice that leaves the buffer): zero rows.
//
// No operand of an MFMA here comes straight out of inline asm: the asm-split halves go through LDS or memory first,
// so the `s_nop` the README asks for between such a block and an MFMA has no place in this file.
#include "mlp_common.h"

namespace s4g {
namespace pngpd {

constexpr int T = 128;       // rows (points) per tile of the trunk kernel
constexpr int R = 32;        // sets per workgroup of the per-set MFMA layers
constexpr int C1 = 64, C2 = 128, C3 = 1024, F1 = 512, F2 = 256, CLSP = 16;
constexpr int X1S = 9, X2S = 17;     // LDS row strides in 16-byte slots: odd, so 16 lanes' b128 reads hit 16 slots
constexpr int DEFAULT_CHUNK = 1024, MAX_CHUNK = 32768;
constexpr int TRUNK_GRID = 2048;

struct SetState {
  int64_t base;
  int32_t len, mode;
  float amax;
  int32_t pad[3];
};

// header words, per half (0 = STN, 1 = feature trunk + classifier head): hdr[16 * half + word]
enum { H_L1 = 0, H_B1, H_SW2, H_IW2, H_L2, H_B2, H_SW3, H_IW3, H_SWA, H_IWA, H_LA, H_BA, H_SWB, H_IWB, H_WORDS = 16 };

struct HalfLayout {
  size_t w1, b2, b3, bA, bB, wC, bC, w2, w3, wA, wB;
};
struct Layout {
  size_t hdr;
  HalfLayout h[2];
  size_t total;
};
inline Layout layout() {
  Layout L;
  size_t o = 256;
  L.hdr = 0;
  for (int t = 0; t < 2; ++t) {
    HalfLayout& H = L.h[t];
    H.w1 = o; o += C1 * 4 * 4;
    H.b2 = o; o += C2 * 4;
    H.b3 = o; o += C3 * 4;
    H.bA = o; o += F1 * 4;
    H.bB = o; o += F2 * 4;
    H.wC = o; o += (size_t)CLSP * F2 * 4;
    H.bC = o; o += 256;
    H.w2 = o; o += (size_t)C1 * C2 * 4;       // two fp16 planes
    H.w3 = o; o += (size_t)C2 * C3 * 4;
    H.wA = o; o += (size_t)C3 * F1 * 4;
    H.wB = o; o += (size_t)F1 * F2 * 4;
  }
  L.total = o;
  return L;
}

struct WsLayout {
  size_t st, tiles, gmax, l1, w1set, keys, gsplit, hsplit, hid, total;
};
inline WsLayout ws_layout(int64_t n) {
  WsLayout W;
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  size_t o = 0;
  W.st = o; o = up(o + (size_t)n * sizeof(SetState));
  W.tiles = o; o = up(o + (size_t)(n + 1) * 8);
  W.gmax = o; o = up(o + (size_t)n * 4);
  W.l1 = o; o = up(o + (size_t)n * 4);
  W.w1set = o; o = up(o + (size_t)n * C1 * 4 * 4);
  W.keys = o; o = up(o + (size_t)n * 2 * C3 * 4);
  W.gsplit = o; o = up(o + (size_t)n * C3 * 4);
  W.hsplit = o; o = up(o + (size_t)n * F1 * 4);
  W.hid = o; o = up(o + (size_t)n * F2 * 4);
  W.total = o;
  return W;
}

// s = 2^(14 - floor(log2 bound)) and its inverse: |v| <= bound gives |v s| < 2^15, inside fp16.  The exponent is clamped
// so that both stay normal numbers whatever the bound is (0, denormal, huge).
__device__ __forceinline__ void pow2_scale(float bound, float& s, float& inv) {
  int e = (int)((__float_as_uint(bound) >> 23) & 0xff);
  e = min(max(e, 27), 254);
  s = __uint_as_float((uint32_t)(268 - e) << 23);
  inv = __uint_as_float((uint32_t)(e - 14) << 23);
}

__device__ __forceinline__ void split1(float v, float s, _Float16& h, _Float16& l) {
  const float x = __builtin_amdgcn_fmed3f(v * s, -65504.f, 65504.f);
  h = (_Float16)x;
  l = (_Float16)(x - (float)h);
}
__device__ __forceinline__ uint16_t bits16(_Float16 v) { return __builtin_bit_cast(uint16_t, v); }

__device__ __forceinline__ float by_mode(float v, int mode) {
  return mode == 0 ? v : (mode == 1 ? __uint_as_float(0x7fc00000u) : 0.0f);
}

// order-preserving key of an fp32 value; 0 is below every key
__device__ __forceinline__ uint32_t max_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) {
  return k == 0 ? 0.0f : __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

__device__ __forceinline__ uint32_t block_max_u32(uint32_t v, uint32_t* sh, int nwaves) {
  v = wave_max_u32(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t m = 0;
  for (int w = 0; w < nwaves; ++w) m = max(m, sh[w]);
  return m;
}

// ------------------------------------------------------------------------------------------------ pack time
struct PackSrc {
  const float* w[12];
  const float* b[12];
};

__device__ float block_max_abs(const float* p, int n, uint32_t* sh) {
  uint32_t m = 0;
  for (int i = threadIdx.x; i < n; i += 256) m = max(m, __float_as_uint(p[i]) & 0x7fffffffu);
  return __uint_as_float(min(block_max_u32(m, sh, 4), 0x7f7fffffu));
}
__device__ float block_max_rowsum(const float* p, int rows, int cols, uint32_t* sh) {
  uint32_t m = 0;
  for (int r = threadIdx.x; r < rows; r += 256) {
    float s = 0.f;
    for (int k = 0; k < cols; ++k) s += fabsf(p[(size_t)r * cols + k]);
    m = max(m, __float_as_uint(s) & 0x7fffffffu);
  }
  return __uint_as_float(min(block_max_u32(m, sh, 4), 0x7f7fffffu));
}

// grid 2 (one block per half)
__global__ __launch_bounds__(256) void stats_kernel(const PackSrc src, float* __restrict__ hdr_all) {
  __shared__ uint32_t sh[4];
  const int half = blockIdx.x;
  const float* const* w = src.w + 6 * half;
  const float* const* b = src.b + 6 * half;
  float* hdr = hdr_all + H_WORDS * half;
  const float l1 = block_max_rowsum(w[0], C1, 3, sh), b1 = block_max_abs(b[0], C1, sh);
  const float m2 = block_max_abs(w[1], C2 * C1, sh), l2 = block_max_rowsum(w[1], C2, C1, sh);
  const float b2 = block_max_abs(b[1], C2, sh);
  const float m3 = block_max_abs(w[2], C3 * C2, sh);
  const float mA = block_max_abs(w[3], F1 * C3, sh), lA = block_max_rowsum(w[3], F1, C3, sh);
  const float bA = block_max_abs(b[3], F1, sh);
  const float mB = block_max_abs(w[4], F2 * F1, sh);
  if (threadIdx.x == 0) {
    hdr[H_L1] = l1 * 1.001f;   // the roundings of the row sums
    hdr[H_B1] = b1;
    hdr[H_L2] = l2 * 1.001f;
    hdr[H_B2] = b2;
    hdr[H_LA] = lA * 1.001f;
    hdr[H_BA] = bA;
    pow2_scale(m2, hdr[H_SW2], hdr[H_IW2]);
    pow2_scale(m3, hdr[H_SW3], hdr[H_IW3]);
    pow2_scale(mA, hdr[H_SWA], hdr[H_IWA]);
    pow2_scale(mB, hdr[H_SWB], hdr[H_IWB]);
  }
}

// grid (ceil(CLSP * F2 / 256), 2)
__global__ __launch_bounds__(256) void pack_small_kernel(const PackSrc src, int classes, char* __restrict__ P,
                                                         const Layout L) {
  const int half = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const HalfLayout& H = L.h[half];
  const float* const* w = src.w + 6 * half;
  const float* const* b = src.b + 6 * half;
  const int nout = half == 0 ? 9 : classes;
  if (i < C1 * 4) ((float*)(P + H.w1))[i] = (i & 3) < 3 ? w[0][(i >> 2) * 3 + (i & 3)] : b[0][i >> 2];
  if (i < C2) ((float*)(P + H.b2))[i] = b[1][i];
  if (i < C3) ((float*)(P + H.b3))[i] = b[2][i];
  if (i < F1) ((float*)(P + H.bA))[i] = b[3][i];
  if (i < F2) ((float*)(P + H.bB))[i] = b[4][i];
  if (i < CLSP) ((float*)(P + H.bC))[i] = i < nout ? b[5][i] : 0.f;
  if (i < CLSP * F2) ((float*)(P + H.wC))[i] = (i / F2) < nout ? w[5][i] : 0.f;
}

// w (N, K) row-major -> fragment order [step][tile][plane][lane] x 8 halves: lane (r = lane & 31, h = lane >> 5) holds
// w[32 tile + r][16 step + 8 h + j], which is the B operand of X W^T and the A operand of W X^T alike.
__global__ __launch_bounds__(256) void pack_frag_kernel(const float* __restrict__ w, int K, int NT,
                                                        const float* __restrict__ scale, uint4* __restrict__ out) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int nsteps = K / 16;
  if (idx >= nsteps * NT * 64) return;
  const int lane = idx & 63, nt = (idx >> 6) % NT, step = idx / (64 * NT);
  const int r = lane & 31, h = lane >> 5;
  const float* row = w + (size_t)(nt * 32 + r) * K + 16 * step + 8 * h;
  const float s = *scale;
  uint32_t Hh[4], Ll[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    _Float16 h0, l0, h1, l1;
    split1(row[2 * j], s, h0, l0);
    split1(row[2 * j + 1], s, h1, l1);
    Hh[j] = (uint32_t)bits16(h0) | ((uint32_t)bits16(h1) << 16);
    Ll[j] = (uint32_t)bits16(l0) | ((uint32_t)bits16(l1) << 16);
  }
  const size_t o = ((size_t)(step * NT + nt) * 2) * 64 + lane;
  out[o] = make_uint4(Hh[0], Hh[1], Hh[2], Hh[3]);
  out[o + 64] = make_uint4(Ll[0], Ll[1], Ll[2], Ll[3]);
}

// ------------------------------------------------------------------------------------------------ per set state
struct PrepArgs {
  const float* points;
  int64_t set_stride, cstride, npts;
  const int64_t* offset;     // NULL: the dense form
  const int32_t* count;
  const int32_t* flags;
  int64_t F, capacity;
  const int32_t* index;
  int64_t g0, num_sets;
  SetState* st;
  uint32_t* keys;            // (n, 2, 1024)
};

// grid n, 256 threads
__global__ __launch_bounds__(256) void prep_kernel(const PrepArgs a) {
  __shared__ uint32_t sh[4];
  const int t = threadIdx.x, i = blockIdx.x;
  const int64_t src = a.index ? (int64_t)a.index[a.g0 + i] : a.g0 + i;
  bool skip = src < 0 || src >= a.num_sets;
  int64_t base = 0, len = 0;
  if (!skip) {
    if (a.offset) {
      const int64_t b = src / a.F, f = src % a.F;
      const int64_t off = a.offset[b * (a.F + 1) + f];
      len = a.count[src];
      skip = len <= 0 || off < 0 || off + len > a.capacity || (a.flags && (a.flags[src] & 1));
      base = b * a.set_stride + off;
    } else {
      len = a.npts;
      skip = len <= 0;
      base = src * a.set_stride;
    }
  }
  uint32_t m = 0;
  if (!skip) {
    for (int c = 0; c < 3; ++c) {
      const float* p = a.points + base + c * a.cstride;
      for (int64_t k = t; k < len; k += 256) m = max(m, __float_as_uint(p[k]) & 0x7fffffffu);
    }
  }
  m = block_max_u32(m, sh, 4);
  for (int k = t; k < 2 * C3; k += 256) a.keys[(size_t)i * 2 * C3 + k] = 0u;
  if (t == 0) {
    SetState s;
    s.mode = skip ? 2 : (m > 0x7f7fffffu ? 1 : 0);
    s.base = s.mode == 0 ? base : 0;
    s.len = s.mode == 0 ? (int32_t)len : 0;
    s.amax = s.mode == 0 ? __uint_as_float(m) : 0.f;
    s.pad[0] = s.pad[1] = s.pad[2] = 0;
    a.st[i] = s;
  }
}

// one block of 1024 threads: tile_start[0 .. n] = the exclusive scan of ceil(len / T)
__global__ __launch_bounds__(1024) void scan_kernel(const SetState* __restrict__ st, int n,
                                                    int64_t* __restrict__ tile_start) {
  __shared__ int64_t part[1024];
  const int t = threadIdx.x, per = (n + 1023) / 1024;
  const int lo = min(t * per, n), hi = min(lo + per, n);
  int64_t s = 0;
  for (int i = lo; i < hi; ++i) s += ((int64_t)st[i].len + T - 1) / T;
  part[t] = s;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int64_t v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int64_t run = part[t] - s;
  for (int i = lo; i < hi; ++i) {
    tile_start[i] = run;
    run += ((int64_t)st[i].len + T - 1) / T;
  }
  if (t == 1023) tile_start[n] = part[1023];
}

// ------------------------------------------------------------------------------------------------ the trunks
struct TrunkArgs {
  const float* points;
  int64_t cstride;
  const SetState* st;
  const int64_t* tile_start;
  int n;
  const float* w1;       // (64, 4) = (w0, w1, w2, b): the STN's first layer
  const float* w1set;    // nullable (n, 64, 4): the set's own first layer (feature trunk)
  const float* l1set;    // with w1set: the set's max row sum of |w|
  const float* hdr;      // this half's header words
  const uint4* w2f;
  const float* b2;
  const uint4* w3f;
  const float* b3;
  uint32_t* keys;        // key of (set i, channel n) at keys[i * 2048 + n]
};

template <bool RELU3>
__global__ __launch_bounds__(512) void trunk_kernel(const TrunkArgs a) {
  __shared__ uint4 x1h[T * X1S], x1l[T * X1S], x2h[T * X2S], x2l[T * X2S];
  __shared__ __attribute__((aligned(16))) float w1s[C1 * 4];
  __shared__ float xyz[3][T];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, r = lane & 31, h = lane >> 5;
  const int64_t total = a.tile_start[a.n];
  const float iW2 = a.hdr[H_IW2], iW3 = a.hdr[H_IW3];

  for (int64_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
    int lo = 0, hi = a.n;          // the last set whose tile_start <= tile (a set without tiles repeats its start)
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (a.tile_start[mid] <= tile) lo = mid; else hi = mid;
    }
    const int s = lo;
    const SetState st = a.st[s];
    const int j0 = (int)(tile - a.tile_start[s]) * T;
    const int rows = min(T, st.len - j0), mtiles = (rows + 31) >> 5;
    float s1, i1, s2, i2;
    const float l1 = a.w1set ? a.l1set[s] : a.hdr[H_L1];
    const float bound1 = (st.amax * l1 + a.hdr[H_B1]) * 1.001f;   // 1.001: the fp32 roundings of the bound itself
    pow2_scale(bound1, s1, i1);
    const float bound2 = (bound1 * a.hdr[H_L2] + a.hdr[H_B2]) * 1.001f;
    pow2_scale(bound2, s2, i2);

    if (t < C1 * 4) w1s[t] = a.w1set ? a.w1set[(size_t)s * C1 * 4 + t] : a.w1[t];
    if (t < 3 * T) {
      const int c = t / T, p = t % T;
      xyz[c][p] = a.points[st.base + c * a.cstride + min(j0 + p, st.len - 1)];
    }
    __syncthreads();

    // 3 -> 64, ReLU: thread = (point, 16 channels)
    {
      const int p = t & (T - 1), q = t >> 7;
      if (p < mtiles * 32) {
        const float x = xyz[0][p], y = xyz[1][p], z = xyz[2][p];
#pragma unroll
        for (int o8 = 0; o8 < 2; ++o8) {
          float v[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float4 w = *(const float4*)&w1s[(16 * q + 8 * o8 + j) * 4];
            v[j] = fmaxf(fmaf(w.z, z, fmaf(w.y, y, fmaf(w.x, x, 0.f))) + w.w, 0.f);
          }
          uint2 h0, l0, h1, l1q;
          split2_h<false>(make_float4(v[0], v[1], v[2], v[3]), s1, h0, l0);
          split2_h<false>(make_float4(v[4], v[5], v[6], v[7]), s1, h1, l1q);
          x1h[p * X1S + 2 * q + o8] = make_uint4(h0.x, h0.y, h1.x, h1.y);
          x1l[p * X1S + 2 * q + o8] = make_uint4(l0.x, l0.y, l1q.x, l1q.y);
        }
      }
    }
    __syncthreads();

    // 64 -> 128, ReLU, transposed: wave = (channel tile, two point tiles)
    {
      const int ct = wave & 3;
      uint4 ah[4], al[4];
#pragma unroll
      for (int step = 0; step < 4; ++step) {
        ah[step] = a.w2f[(size_t)((step * 4 + ct) * 2) * 64 + lane];
        al[step] = a.w2f[(size_t)((step * 4 + ct) * 2 + 1) * 64 + lane];
      }
      float bias[4][4];
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i) bias[g][i] = a.b2[ct * 32 + 8 * g + 4 * h + i];
      const float deq = iW2 * i1;
      for (int pt = (wave >> 2) * 2; pt < min((wave >> 2) * 2 + 2, mtiles); ++pt) {
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
        for (int step = 0; step < 4; ++step) {
          const uint4 bh = x1h[(pt * 32 + r) * X1S + 2 * step + h], bl = x1l[(pt * 32 + r) * X1S + 2 * step + h];
          acc = chain_mfma<2>(al[step], bh, acc);
          acc = chain_mfma<2>(ah[step], bl, acc);
          acc = chain_mfma<2>(ah[step], bh, acc);
        }
        uint2* oh = (uint2*)&x2h[(pt * 32 + r) * X2S];
        uint2* ol = (uint2*)&x2l[(pt * 32 + r) * X2S];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float v[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = fmaxf(acc[4 * g + i] * deq + bias[g][i], 0.f);
          uint2 vh, vl;
          split2_h<false>(make_float4(v[0], v[1], v[2], v[3]), s2, vh, vl);
          const int c4 = (ct * 32 + 8 * g + 4 * h) >> 2;
          oh[c4] = vh;
          ol[c4] = vl;
        }
      }
    }
    __syncthreads();

    // 128 -> 1024 and the maximum over the rows: wave = two channel tiles at a time, W in registers
    {
      const float deq = iW3 * i2;
#pragma unroll 1
      for (int it = 0; it < 2; ++it) {
        const int np = wave + 8 * it;
        uint4 bh[8][2], bl[8][2];
#pragma unroll
        for (int step = 0; step < 8; ++step)
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            bh[step][q] = a.w3f[(size_t)((step * 32 + 2 * np + q) * 2) * 64 + lane];
            bl[step][q] = a.w3f[(size_t)((step * 32 + 2 * np + q) * 2 + 1) * 64 + lane];
          }
        float m0 = -INFINITY, m1 = -INFINITY;
#pragma unroll 1
        for (int mt = 0; mt < mtiles; ++mt) {
          f32x16 acc0, acc1;
#pragma unroll
          for (int e = 0; e < 16; ++e) acc0[e] = 0.f, acc1[e] = 0.f;
#pragma unroll
          for (int step = 0; step < 8; ++step) {
            const uint4 xh = x2h[(mt * 32 + r) * X2S + 2 * step + h], xl = x2l[(mt * 32 + r) * X2S + 2 * step + h];
            acc0 = chain_mfma<2>(xl, bh[step][0], acc0);
            acc1 = chain_mfma<2>(xl, bh[step][1], acc1);
            acc0 = chain_mfma<2>(xh, bl[step][0], acc0);
            acc1 = chain_mfma<2>(xh, bl[step][1], acc1);
            acc0 = chain_mfma<2>(xh, bh[step][0], acc0);
            acc1 = chain_mfma<2>(xh, bh[step][1], acc1);
          }
#pragma unroll
          for (int e = 0; e < 16; ++e) m0 = fmaxf(m0, acc0[e]), m1 = fmaxf(m1, acc1[e]);
        }
        m0 = fmaxf(m0, __shfl_xor(m0, 32, 64));
        m1 = fmaxf(m1, __shfl_xor(m1, 32, 64));
        // half wave 0 publishes the first channel tile, half wave 1 the second
        const int n = (2 * np + h) * 32 + r;
        float v = (h ? m1 : m0) * deq + a.b3[n];
        if (RELU3) v = fmaxf(v, 0.f);
        atomicMax(&a.keys[(size_t)s * 2 * C3 + n], max_key(v));
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ per set layers
// The 1024 maxima of a set: keys -> fp32, the set's largest magnitude, and the f16x2 row the next layer reads
// ([octet of channels][plane] x 8 halves).  grid n, 256 threads x 4 channels.
__global__ __launch_bounds__(256) void finalize_kernel(const uint32_t* __restrict__ keys, const SetState* __restrict__ st,
                                                       float* __restrict__ gmax, uint2* __restrict__ gsplit,
                                                       float* __restrict__ feat) {
  __shared__ uint32_t sh[4];
  const int t = threadIdx.x, i = blockIdx.x;
  const int mode = st[i].mode;
  const uint4 k = *(const uint4*)&keys[(size_t)i * 2 * C3 + 4 * t];
  float v[4] = {key_value(k.x), key_value(k.y), key_value(k.z), key_value(k.w)};
  uint32_t m = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (mode != 0) v[j] = 0.f;
    m = max(m, __float_as_uint(v[j]) & 0x7fffffffu);
  }
  m = min(block_max_u32(m, sh, 4), 0x7f7fffffu);
  float s, inv;
  pow2_scale(__uint_as_float(m), s, inv);
  uint2 vh, vl;
  split2_h<true>(make_float4(v[0], v[1], v[2], v[3]), s, vh, vl);
  uint2* row = gsplit + (size_t)i * (C3 / 2);
  row[((t >> 1) * 2) * 2 + (t & 1)] = vh;
  row[((t >> 1) * 2 + 1) * 2 + (t & 1)] = vl;
  if (t == 0) gmax[i] = __uint_as_float(m);
  if (feat)
    *(float4*)&feat[(size_t)i * C3 + 4 * t] =
        make_float4(by_mode(v[0], mode), by_mode(v[1], mode), by_mode(v[2], mode), by_mode(v[3], mode));
}

struct HeadScales {
  float sg, ig, sa, ia;
};
__device__ __forceinline__ HeadScales head_scales(float gmax, const float* __restrict__ hdr) {
  HeadScales S;
  pow2_scale(gmax, S.sg, S.ig);
  pow2_scale((gmax * hdr[H_LA] + hdr[H_BA]) * 1.001f, S.sa, S.ia);
  return S;
}

// relu(X W^T + b) for R = 32 sets per workgroup: grid (ceil(n / 32), N / 128), four waves x one 32-unit tile, A rows
// straight from the sets' split rows.  FIRST: 1024 -> 512, split output; else 512 -> 256, fp32 output.
template <int K, int N, bool FIRST>
__global__ __launch_bounds__(256) void fc_kernel(const uint4* __restrict__ in, const SetState* __restrict__ st,
                                                 const float* __restrict__ gmax, const uint4* __restrict__ wf,
                                                 const float* __restrict__ bias, const float* __restrict__ hdr, int n,
                                                 uint16_t* __restrict__ out_split, float* __restrict__ out,
                                                 float* __restrict__ feat) {
  constexpr int NT = N / 32, STEPS = K / 16;
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int m0 = blockIdx.x * R, nt = blockIdx.y * 4 + (threadIdx.x >> 6);
  const uint4* a0 = in + (size_t)min(m0 + r, n - 1) * (K / 4) + h * 2;
  const uint4* wq = wf + (size_t)nt * 128 + lane;
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll 4
  for (int s = 0; s < STEPS; ++s) {
    const uint4 ah = a0[s * 4], al = a0[s * 4 + 1];
    const uint4 bh = wq[(size_t)s * NT * 128], bl = wq[(size_t)s * NT * 128 + 64];
    acc = chain_mfma<2>(al, bh, acc);
    acc = chain_mfma<2>(ah, bl, acc);
    acc = chain_mfma<2>(ah, bh, acc);
  }
  const float inW = hdr[FIRST ? H_IWA : H_IWB];
  const int u = nt * 32 + r;
  const float b = bias[u];
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int i = m0 + (e & 3) + 8 * (e >> 2) + 4 * h;
    if (i >= n) continue;
    const int mode = st[i].mode;
    const HeadScales S = head_scales(gmax[i], hdr);
    const float v = fmaxf(acc[e] * inW * (FIRST ? S.ig : S.ia) + b, 0.f);
    if constexpr (FIRST) {
      _Float16 vh, vl;
      split1(mode == 0 ? v : 0.f, S.sa, vh, vl);
      const size_t o = (((size_t)i * (N / 8) + (u >> 3)) * 2) * 8 + (u & 7);
      out_split[o] = bits16(vh);
      out_split[o + 8] = bits16(vl);
    } else {
      out[(size_t)i * N + u] = mode == 0 ? v : 0.f;
      if (feat) feat[(size_t)i * N + u] = by_mode(v, mode);
    }
  }
}

// One wave per set, fp32 FMAs in a fixed order: lane l sums k = l, l + 64, ..., then a butterfly over the lanes.
__device__ __forceinline__ float wave_dot256(const float* __restrict__ x, const float* __restrict__ w, int lane) {
  float acc = 0.f;
  for (int k = lane; k < F2; k += 64) acc = fmaf(x[k], w[k], acc);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
  return acc;
}

// trans = fc3(hid) + I, and the set's own first feature layer W1 trans^T with its row-sum bound
__global__ __launch_bounds__(64) void stn_tail_kernel(const float* __restrict__ hid, const SetState* __restrict__ st,
                                                      const float* __restrict__ wC, const float* __restrict__ bC,
                                                      const float* __restrict__ w1feat, float* __restrict__ w1set,
                                                      float* __restrict__ l1set, float* __restrict__ trans) {
  const int lane = threadIdx.x, i = blockIdx.x;
  const int mode = st[i].mode;
  float tr[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const float v = wave_dot256(hid + (size_t)i * F2, wC + k * F2, lane) + bC[k] + (k % 4 == 0 ? 1.f : 0.f);
    tr[k] = mode == 0 ? v : 0.f;
    if (trans && lane == 0) trans[(size_t)i * 9 + k] = by_mode(v, mode);
  }
  // (x^T trans)_j = sum_i x_i trans[i][j]  =>  w'[o][i] = sum_j w[o][j] trans[i][j]
  const float4 w = *(const float4*)&w1feat[lane * 4];
  float4 o;
  o.x = fmaf(w.z, tr[2], fmaf(w.y, tr[1], w.x * tr[0]));
  o.y = fmaf(w.z, tr[5], fmaf(w.y, tr[4], w.x * tr[3]));
  o.z = fmaf(w.z, tr[8], fmaf(w.y, tr[7], w.x * tr[6]));
  o.w = w.w;
  *(float4*)&w1set[((size_t)i * C1 + lane) * 4] = o;
  const float rs = (fabsf(o.x) + fabsf(o.y) + fabsf(o.z)) * 1.001f;
  const uint32_t m = wave_max_u32(min(__float_as_uint(rs) & 0x7fffffffu, 0x7f7fffffu));
  if (lane == 0) l1set[i] = __uint_as_float(m);
}

__global__ __launch_bounds__(64) void cls_tail_kernel(const float* __restrict__ hid, const SetState* __restrict__ st,
                                                      const float* __restrict__ wC, const float* __restrict__ bC,
                                                      int classes, float* __restrict__ logits,
                                                      int32_t* __restrict__ status) {
  const int lane = threadIdx.x, i = blockIdx.x;
  const int mode = st[i].mode;
  for (int c = 0; c < classes; ++c) {
    const float v = wave_dot256(hid + (size_t)i * F2, wC + c * F2, lane) + bC[c];
    if (lane == 0) logits[(size_t)i * classes + c] = by_mode(v, mode);
  }
  if (status && lane == 0) status[i] = mode;
}

inline bool dims_ok(int classes) { return classes >= 1 && classes <= CLSP; }

}  // namespace pngpd
}  // namespace s4g

using namespace s4g;
using namespace s4g::pngpd;

extern "C" size_t s4g_pngpd_pack_bytes(int classes) {
  if (!dims_ok(classes)) return 0;
  return layout().total;
}

extern "C" int s4g_pngpd_pack_f32(const float* const* weights12, const float* const* biases12, int classes, void* packed,
                                  s4g_stream_t stream) {
  if (!dims_ok(classes) || !weights12 || !biases12 || !packed || ((uintptr_t)packed & 15)) return S4G_EINVAL;
  PackSrc src;
  for (int i = 0; i < 12; ++i) {
    if (!weights12[i] || !biases12[i]) return S4G_EINVAL;
    src.w[i] = weights12[i];
    src.b[i] = biases12[i];
  }
  hipStream_t st = (hipStream_t)stream;
  const Layout L = layout();
  char* P = (char*)packed;
  float* hdr = (float*)(P + L.hdr);
  stats_kernel<<<2, 256, 0, st>>>(src, hdr);
  S4G_LAUNCH_CHECK();
  pack_small_kernel<<<dim3((CLSP * F2 + 255) / 256, 2), 256, 0, st>>>(src, classes, P, L);
  S4G_LAUNCH_CHECK();
  for (int t = 0; t < 2; ++t) {
    const HalfLayout& H = L.h[t];
    const float* h = hdr + H_WORDS * t;
    const struct { const float* w; int K, N, word; size_t off; } jobs[4] = {
        {src.w[6 * t + 1], C1, C2, H_SW2, H.w2}, {src.w[6 * t + 2], C2, C3, H_SW3, H.w3},
        {src.w[6 * t + 3], C3, F1, H_SWA, H.wA}, {src.w[6 * t + 4], F1, F2, H_SWB, H.wB}};
    for (const auto& j : jobs) {
      const int items = (j.K / 16) * (j.N / 32) * 64;
      pack_frag_kernel<<<(items + 255) / 256, 256, 0, st>>>(j.w, j.K, j.N / 32, h + j.word, (uint4*)(P + j.off));
      S4G_LAUNCH_CHECK();
    }
  }
  return S4G_OK;
}

extern "C" size_t s4g_pngpd_workspace_bytes(int64_t chunk, int classes) {
  if (!dims_ok(classes) || chunk < 0 || chunk > MAX_CHUNK) return 0;
  return ws_layout(chunk > 0 ? chunk : DEFAULT_CHUNK).total;
}

extern "C" int s4g_pngpd_forward_f32(const float* points, int64_t set_stride, int64_t channel_stride, int64_t n_points,
                                     const int64_t* offset, const int32_t* count, const int32_t* flags, int64_t F,
                                     int64_t capacity, const int32_t* index, int64_t G, int64_t num_sets,
                                     const void* packed, int classes, int64_t chunk, float* stn_global, float* trans,
                                     float* global_feat, float* hidden, int32_t* status, float* logits, void* ws,
                                     size_t ws_bytes, s4g_stream_t stream) {
  if (!dims_ok(classes) || G < 0 || num_sets < 0 || chunk < 0 || chunk > MAX_CHUNK || !packed ||
      ((uintptr_t)packed & 15) || G > 0x7fffffff || num_sets > 0x7fffffff || set_stride < 0 || channel_stride < 0 ||
      n_points < 0 || n_points > 0x7fffffff || capacity < 0 || capacity > 0x7fffffff)
    return S4G_EINVAL;
  if (offset && (!count || F < 1 || num_sets % F != 0)) return S4G_EINVAL;
  if (G == 0) return S4G_OK;
  if (!logits || (!points && num_sets > 0) || (!index && G > num_sets)) return S4G_EINVAL;
  int64_t ch = chunk > 0 ? chunk : DEFAULT_CHUNK;
  if (ch > G) ch = G;
  const WsLayout W = ws_layout(ch);
  if (!ws || ((uintptr_t)ws & 15)) return S4G_EINVAL;
  if (ws_bytes < W.total) return S4G_EWORKSPACE;
  hipStream_t stq = (hipStream_t)stream;
  const Layout L = layout();
  const char* P = (const char*)packed;
  char* wsb = (char*)ws;
  SetState* st = (SetState*)(wsb + W.st);
  int64_t* tiles = (int64_t*)(wsb + W.tiles);
  float* gmax = (float*)(wsb + W.gmax);
  float* l1set = (float*)(wsb + W.l1);
  float* w1set = (float*)(wsb + W.w1set);
  uint32_t* keys = (uint32_t*)(wsb + W.keys);
  uint4* gsplit = (uint4*)(wsb + W.gsplit);
  uint4* hsplit = (uint4*)(wsb + W.hsplit);
  float* hid = (float*)(wsb + W.hid);
  const int64_t max_len = offset ? capacity : n_points;

  for (int64_t g0 = 0; g0 < G; g0 += ch) {
    const int n = (int)(G - g0 < ch ? G - g0 : ch);
    PrepArgs pa;
    pa.points = points; pa.set_stride = set_stride; pa.cstride = channel_stride; pa.npts = n_points;
    pa.offset = offset; pa.count = count; pa.flags = flags; pa.F = F; pa.capacity = capacity; pa.index = index;
    pa.g0 = g0; pa.num_sets = num_sets; pa.st = st; pa.keys = keys;
    prep_kernel<<<n, 256, 0, stq>>>(pa);
    S4G_LAUNCH_CHECK();
    scan_kernel<<<1, 1024, 0, stq>>>(st, n, tiles);
    S4G_LAUNCH_CHECK();
    const int64_t most = (int64_t)n * ((max_len + T - 1) / T);
    const int grid = (int)(most < 1 ? 1 : (most < TRUNK_GRID ? most : TRUNK_GRID));
    for (int t = 0; t < 2; ++t) {
      const HalfLayout& H = L.h[t];
      const float* hdr = (const float*)(P + L.hdr) + H_WORDS * t;
      TrunkArgs ta;
      ta.points = points; ta.cstride = channel_stride; ta.st = st; ta.tile_start = tiles; ta.n = n;
      ta.w1 = (const float*)(P + H.w1); ta.w1set = t ? w1set : nullptr; ta.l1set = l1set; ta.hdr = hdr;
      ta.w2f = (const uint4*)(P + H.w2); ta.b2 = (const float*)(P + H.b2);
      ta.w3f = (const uint4*)(P + H.w3); ta.b3 = (const float*)(P + H.b3);
      ta.keys = keys + (size_t)t * C3;
      if (t == 0)
        trunk_kernel<true><<<grid, 512, 0, stq>>>(ta);
      else
        trunk_kernel<false><<<grid, 512, 0, stq>>>(ta);
      S4G_LAUNCH_CHECK();
      float* gout = t ? global_feat : stn_global;
      finalize_kernel<<<n, 256, 0, stq>>>(keys + (size_t)t * C3, st, gmax, (uint2*)gsplit,
                                          gout ? gout + (size_t)g0 * C3 : nullptr);
      S4G_LAUNCH_CHECK();
      fc_kernel<C3, F1, true><<<dim3((n + R - 1) / R, F1 / 128), 256, 0, stq>>>(
          gsplit, st, gmax, (const uint4*)(P + H.wA), (const float*)(P + H.bA), hdr, n, (uint16_t*)hsplit, nullptr,
          nullptr);
      S4G_LAUNCH_CHECK();
      fc_kernel<F1, F2, false><<<dim3((n + R - 1) / R, F2 / 128), 256, 0, stq>>>(
          hsplit, st, gmax, (const uint4*)(P + H.wB), (const float*)(P + H.bB), hdr, n, nullptr, hid,
          (t && hidden) ? hidden + (size_t)g0 * F2 : nullptr);
      S4G_LAUNCH_CHECK();
      if (t == 0)
        stn_tail_kernel<<<n, 64, 0, stq>>>(hid, st, (const float*)(P + H.wC), (const float*)(P + H.bC),
                                           (const float*)(P + L.h[1].w1), w1set, l1set,
                                           trans ? trans + (size_t)g0 * 9 : nullptr);
      else
        cls_tail_kernel<<<n, 64, 0, stq>>>(hid, st, (const float*)(P + H.wC), (const float*)(P + H.bC), classes,
                                           logits + (size_t)g0 * classes, status ? status + g0 : nullptr);
      S4G_LAUNCH_CHECK();
    }
  }
  return S4G_OK;
}
