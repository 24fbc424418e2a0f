// GPDClassifier (inference/grasp_proposal/network_models/models/GPD.py, eval mode) on the 60 x 60 close-region maps:
//   p1 = maxpool2x2(conv1(x) + b1)   Cin -> 20, 5x5 valid      (20, 28, 28)   no ReLU
//   p2 = maxpool2x2(conv2(p1) + b2)  20 -> 50, 5x5 valid       (50, 12, 12)   no ReLU
//   h  = relu(fc1(flatten(p2)) + c1) 7200 -> 500, flatten order (c, y, x)
//   logits = fc2(h) + c2             500 -> classes
//
// The two convolutions are implicit GEMMs on v_mfma_f32_32x32x16_f16 in the f16x2 split of mlp_common.h (two scaled
// fp16 planes, three products per MAC, fp32 accumulate).  M = output positions, N = output channels, K = (ky, kx, c)
// with c in groups of 8, so that a lane's operand fragment is ONE 16-byte LDS read of a channels-last image.
//
// Tile: 32 positions = 4 conv rows x 8 conv columns = 2 x 4 pool windows, row m = 4 w + p with w the window and
// p = (dy, dx): a lane's registers 4 g .. 4 g + 3 hold rows 8 g + 4 (lane >> 5) + 0..3, which are the four positions of
// window 2 g + (lane >> 5), so the pool is a maximum of four accumulators of one lane and a window never straddles two
// tiles.  One wave owns a whole tile row (all tiles along x, all channel tiles): 7 accumulator tiles for conv1 (56 / 8 x
// one 32-channel tile), 6 for conv2 (24 / 8 x two).  A workgroup of WR waves stages the 4 WR + 4 input rows its WR
// tile rows read.
//
// Scales are powers of two and PER IMAGE: the input's from the image's own maximum, pool1's and pool2's from bounds
// (max |x| * max_co sum |w| + max |b|, chained) formed from that maximum and from constants of the weights computed at
// pack time.  Nothing an image's kernels read depends on another image, the accumulation order is fixed by the code:
// batch invariant and bit-reproducible.
//
// Image states: 0 = normal; 1 = the image holds a NaN or an infinity (nothing of it is staged; every output row of it is
// NaN); 2 = index -1 or out of range (never read; every output row of it is 0).
#include "mlp_common.h"

namespace s4g {
namespace gpd {

constexpr int IMG = 60, P1 = 28, P2 = 12, C1 = 20, C2 = 50, C1G = 3 /* pool1 channel groups of 8 */;
constexpr int FCK = 7200, HID = 500, HIDP = 512, CLSP = 16;
constexpr int FC_STEPS = FCK / 16, FC_NT = HIDP / 32, FC_ROWS = 32;
constexpr int DEFAULT_CHUNK = 1024, MAX_CHUNK = 32768;
constexpr size_t P1_U4 = (size_t)P1 * P1 * C1G * 2;   // uint4 per image of the split pool1 image
constexpr size_t P2_U4 = (size_t)(FCK / 8) * 2;       // uint4 per image of the split pool2 row

struct ImgState {
  int32_t src, mode;
  float amax;
  int32_t pad;
};

// header words of the packed parameters
enum { H_SW1 = 0, H_IW1, H_L1, H_B1, H_SW2, H_IW2, H_L2, H_B2, H_SW3, H_IW3 };

struct Layout {
  size_t hdr, b1, b2, c1, w4, c2, w1, w2, w3, total;
  int cg1, ns1, ns2;
};
inline Layout layout(int Cin) {
  Layout L;
  L.cg1 = Cin <= 8 ? 1 : 2;
  L.ns1 = (25 * L.cg1 + 1) / 2;
  L.ns2 = (25 * C1G + 1) / 2;
  L.hdr = 0;
  L.b1 = 256;
  L.b2 = L.b1 + 256;
  L.c1 = L.b2 + 256;
  L.w4 = L.c1 + HIDP * 4;
  L.c2 = L.w4 + (size_t)CLSP * HIDP * 4;
  L.w1 = L.c2 + 256;
  L.w2 = L.w1 + (size_t)L.ns1 * 2048;
  L.w3 = L.w2 + (size_t)L.ns2 * 2 * 2048;
  L.total = L.w3 + (size_t)FC_STEPS * FC_NT * 2048;
  return L;
}

struct WsLayout {
  size_t st, p1, p2, hid, total;
};
inline WsLayout ws_layout(int64_t chunk) {
  WsLayout W;
  W.st = 0;
  W.p1 = ((size_t)chunk * sizeof(ImgState) + 255) & ~(size_t)255;
  W.p2 = W.p1 + (size_t)chunk * P1_U4 * 16;
  W.hid = W.p2 + (size_t)chunk * P2_U4 * 16;
  W.total = W.hid + (size_t)chunk * HIDP * 4;
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

struct Scales {
  float sA, iA, s1, i1, s2, i2;
};
__device__ __forceinline__ Scales scales_of(float amax, const float* __restrict__ hdr) {
  Scales S;
  pow2_scale(amax, S.sA, S.iA);
  // 1.001: the fp32 roundings of the bound itself
  const float bound1 = (amax * hdr[H_L1] + hdr[H_B1]) * 1.001f;
  pow2_scale(bound1, S.s1, S.i1);
  const float bound2 = (bound1 * hdr[H_L2] + hdr[H_B2]) * 1.001f;
  pow2_scale(bound2, S.s2, S.i2);
  return S;
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

// ------------------------------------------------------------------------------------------------ pack time
__global__ __launch_bounds__(256) void stats_kernel(const float* __restrict__ w1, int k1, const float* __restrict__ b1,
                                                    const float* __restrict__ w2, const float* __restrict__ b2,
                                                    const float* __restrict__ w3, float* __restrict__ hdr) {
  __shared__ uint32_t sh[3][4];
  __shared__ float rows[128];
  const int t = threadIdx.x;
  uint32_t m1 = 0, m2 = 0, m3 = 0;
  for (int i = t; i < C1 * k1; i += 256) m1 = max(m1, __float_as_uint(w1[i]) & 0x7fffffffu);
  for (int i = t; i < C2 * C1 * 25; i += 256) m2 = max(m2, __float_as_uint(w2[i]) & 0x7fffffffu);
  for (int i = t; i < HID * FCK; i += 256) m3 = max(m3, __float_as_uint(w3[i]) & 0x7fffffffu);
  m1 = wave_max_u32(m1);
  m2 = wave_max_u32(m2);
  m3 = wave_max_u32(m3);
  if ((t & 63) == 0) {
    sh[0][t >> 6] = m1;
    sh[1][t >> 6] = m2;
    sh[2][t >> 6] = m3;
  }
  float rs = 0.f;
  if (t < C1) {
    for (int k = 0; k < k1; ++k) rs += fabsf(w1[t * k1 + k]);
  } else if (t >= 64 && t < 64 + C2) {
    for (int k = 0; k < C1 * 25; ++k) rs += fabsf(w2[(t - 64) * C1 * 25 + k]);
  }
  if (t < 128) rows[t] = rs;
  __syncthreads();
  if (t == 0) {
    float s, inv;
    for (int l = 0; l < 3; ++l) {
      const uint32_t m = max(max(sh[l][0], sh[l][1]), max(sh[l][2], sh[l][3]));
      pow2_scale(__uint_as_float(min(m, 0x7f7fffffu)), s, inv);
      hdr[l * 4 + 0] = s;
      hdr[l * 4 + 1] = inv;
    }
    float L1 = 0.f, L2 = 0.f, B1 = 0.f, B2 = 0.f;
    for (int i = 0; i < C1; ++i) L1 = fmaxf(L1, rows[i]), B1 = fmaxf(B1, fabsf(b1[i]));
    for (int i = 0; i < C2; ++i) L2 = fmaxf(L2, rows[64 + i]), B2 = fmaxf(B2, fabsf(b2[i]));
    hdr[H_L1] = L1 * 1.001f;   // the roundings of the row sums
    hdr[H_B1] = B1;
    hdr[H_L2] = L2 * 1.001f;
    hdr[H_B2] = B2;
  }
}

__global__ __launch_bounds__(256) void pack_small_kernel(const float* __restrict__ b1, const float* __restrict__ b2,
                                                         const float* __restrict__ c1, const float* __restrict__ w4,
                                                         const float* __restrict__ c2, int classes,
                                                         float* __restrict__ o_b1, float* __restrict__ o_b2,
                                                         float* __restrict__ o_c1, float* __restrict__ o_w4,
                                                         float* __restrict__ o_c2) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < 32) o_b1[i] = i < C1 ? b1[i] : 0.f;
  if (i < 64) o_b2[i] = i < C2 ? b2[i] : 0.f;
  if (i < HIDP) o_c1[i] = i < HID ? c1[i] : 0.f;
  if (i < CLSP) o_c2[i] = i < classes ? c2[i] : 0.f;
  if (i < CLSP * HIDP) {
    const int c = i / HIDP, k = i % HIDP;
    o_w4[i] = (c < classes && k < HID) ? w4[c * HID + k] : 0.f;
  }
}

// Weights in fragment order: [step][channel tile][plane][lane] x 8 halves; lane (r = lane & 31, h = lane >> 5) holds
// B[k = 16 step + 8 h + j][n = 32 tile + r].  CONV: k group 2 step + h = (ky * 5 + kx) * CG + cg, channel 8 cg + j.
template <bool CONV>
__global__ __launch_bounds__(256) void pack_frag_kernel(const float* __restrict__ w, int cin, int cout, int CG, int NT,
                                                        int nsteps, const float* __restrict__ hdr, int scale_word,
                                                        uint4* __restrict__ out) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= nsteps * NT * 64) return;
  const int lane = idx & 63, nt = (idx >> 6) % NT, step = idx / (64 * NT);
  const int r = lane & 31, h = lane >> 5, n = nt * 32 + r, gi = 2 * step + h;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    v[j] = 0.f;
    if constexpr (CONV) {
      if (gi < 25 * CG && n < cout) {
        const int tap = gi / CG, c = 8 * (gi % CG) + j;
        if (c < cin) v[j] = w[((size_t)n * cin + c) * 25 + tap];
      }
    } else {
      if (n < cout) v[j] = w[(size_t)n * FCK + 16 * step + 8 * h + j];
    }
  }
  const float s = hdr[scale_word];
  uint32_t H[4], L[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    _Float16 h0, l0, h1, l1;
    split1(v[2 * j], s, h0, l0);
    split1(v[2 * j + 1], s, h1, l1);
    H[j] = (uint32_t)bits16(h0) | ((uint32_t)bits16(h1) << 16);
    L[j] = (uint32_t)bits16(l0) | ((uint32_t)bits16(l1) << 16);
  }
  const size_t o = ((size_t)(step * NT + nt) * 2) * 64 + lane;
  out[o] = make_uint4(H[0], H[1], H[2], H[3]);
  out[o + 64] = make_uint4(L[0], L[1], L[2], L[3]);
}

// ------------------------------------------------------------------------------------------------ per image state
__global__ __launch_bounds__(256) void prep_kernel(const float* __restrict__ maps, int64_t istride, int64_t cstride,
                                                   const int32_t* __restrict__ index, int64_t g0, int64_t num_images,
                                                   int Cin, ImgState* __restrict__ st) {
  __shared__ uint32_t sh[4];
  const int t = threadIdx.x, i = blockIdx.x;
  const int64_t src = index ? (int64_t)index[g0 + i] : g0 + i;
  const bool skip = src < 0 || src >= num_images;
  uint32_t m = 0;
  if (!skip) {
    for (int c = 0; c < Cin; ++c) {
      const float* p = maps + src * istride + c * cstride;
      for (int k = t; k < IMG * IMG; k += 256) m = max(m, __float_as_uint(p[k]) & 0x7fffffffu);
    }
  }
  m = wave_max_u32(m);
  if ((t & 63) == 0) sh[t >> 6] = m;
  __syncthreads();
  if (t == 0) {
    m = max(max(sh[0], sh[1]), max(sh[2], sh[3]));
    ImgState s;
    s.mode = skip ? 2 : (m > 0x7f7fffffu ? 1 : 0);
    s.src = s.mode == 0 ? (int32_t)src : -1;
    s.amax = s.mode == 0 ? __uint_as_float(m) : 0.f;
    s.pad = 0;
    st[i] = s;
  }
}

// ------------------------------------------------------------------------------------------------ the convolutions
struct ConvArgs {
  const float* maps;       // FIRST: the caller's maps
  int64_t istride, cstride;
  int Cin;
  const uint4* in_split;   // !FIRST: the split pool1 images of the chunk
  const ImgState* st;
  const uint4* wfrag;
  const float* bias;       // padded to 32 NT
  const float* hdr;
  uint16_t* out_split;     // FIRST: split pool1 images; else split pool2 rows
  float* feat;             // nullable fp32 copy, at the chunk's first image
};

// 5x5 valid convolution + bias + 2x2/2 max-pool of an IW x IW image with 8 CG channels into COUT channels.
// grid (strips, images), WR waves.
template <int CG, int NT, int IW, int WR, int TX, int COUT, bool FIRST>
__global__ __launch_bounds__(WR * 64) void conv_pool_kernel(const ConvArgs a) {
  constexpr int ROWS = 4 * WR + 4, NG = 25 * CG, NSTEPS = (NG + 1) / 2, PW = (IW - 4) / 2, NTHR = WR * 64;
  static_assert(8 * TX + 4 == IW, "tile row covers the conv width");
  // LDS image in 16-byte slots: pixel stride PS, row stride RS.  A ds_read_b128 is served in groups of 16 lanes which,
  // with the row order above, hold 4 columns of two rows and the other 4 columns of the next two: the 16 slots
  // PS x + RS y (mod 16) of a group are distinct for PS odd and RS = 8 (mod 16), and for PS = 4 and RS odd.
  constexpr int PS = CG == 2 ? 4 : 2 * CG + 1;
  constexpr int RS = CG == 2 ? IW * PS + 1 : ((IW * PS + 7) / 16) * 16 + 8;
  static_assert(RS >= IW * PS && (CG == 2 ? RS % 2 == 1 : RS % 16 == 8), "conflict-free operand reads");
  __shared__ uint4 lds[ROWS * RS];
  __shared__ int goff[NG + 1];
  const int t = threadIdx.x, strip = blockIdx.x, i = blockIdx.y;
  const ImgState st = a.st[i];
  const Scales S = scales_of(st.amax, a.hdr);
  const int y0 = strip * 4 * WR;

  for (int g = t; g <= NG; g += NTHR) {
    const int gc = min(g, NG - 1), tap = gc / CG, cg = gc % CG;
    goff[g] = (tap / 5) * RS + (tap % 5) * PS + cg * 2;
  }
  if constexpr (FIRST) {
    const float* img = a.maps + (int64_t)(st.mode == 0 ? st.src : 0) * a.istride;
    // four (pixel, channel group) items per thread at a time: 32 loads in flight before the first split
    constexpr int TOTAL = ROWS * IW * CG, UNR = 4;
    for (int idx0 = t; idx0 < TOTAL; idx0 += NTHR * UNR) {
      float v[UNR][8];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int idx = idx0 + u * NTHR;
        const int x = idx % IW, q = idx / IW, cg = q % CG, y = q / CG;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int c = 8 * cg + j;
          v[u][j] = (st.mode == 0 && idx < TOTAL && c < a.Cin) ? img[(int64_t)c * a.cstride + (y0 + y) * IW + x] : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int idx = idx0 + u * NTHR;
        if (idx >= TOTAL) break;
        const int x = idx % IW, q = idx / IW, cg = q % CG, y = q / CG;
        uint2 h0, l0, h1, l1;
        split2_h<false>(make_float4(v[u][0], v[u][1], v[u][2], v[u][3]), S.sA, h0, l0);
        split2_h<false>(make_float4(v[u][4], v[u][5], v[u][6], v[u][7]), S.sA, h1, l1);
        const int o = y * RS + x * PS + cg * 2;
        lds[o] = make_uint4(h0.x, h0.y, h1.x, h1.y);
        lds[o + 1] = make_uint4(l0.x, l0.y, l1.x, l1.y);
      }
    }
  } else {
    const uint4* src = a.in_split + (size_t)i * (IW * IW * CG * 2) + (size_t)y0 * IW * CG * 2;
    for (int idx = t; idx < ROWS * IW * CG * 2; idx += NTHR) {
      const int e = idx % (CG * 2), px = idx / (CG * 2);
      lds[(px / IW) * RS + (px % IW) * PS + e] = src[idx];
    }
  }
  __syncthreads();

  const int wave = t >> 6, lane = t & 63, r = lane & 31, h = lane >> 5;
  const int w = r >> 2, p = r & 3;
  const int base = (4 * wave + 2 * (w >> 2) + (p >> 1)) * RS + (2 * (w & 3) + (p & 1)) * PS;
  f32x16 acc[TX][NT];
#pragma unroll
  for (int tx = 0; tx < TX; ++tx)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[tx][nt][e] = 0.f;

#pragma unroll 2
  for (int step = 0; step < NSTEPS; ++step) {
    uint4 bh[NT], bl[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      bh[nt] = a.wfrag[(size_t)((step * NT + nt) * 2) * 64 + lane];
      bl[nt] = a.wfrag[(size_t)((step * NT + nt) * 2 + 1) * 64 + lane];
    }
    const int off = base + goff[2 * step + h];
#pragma unroll
    for (int tx = 0; tx < TX; ++tx) {
      const uint4 ah = lds[off + tx * 8 * PS], al = lds[off + tx * 8 * PS + 1];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        acc[tx][nt] = chain_mfma<2>(al, bh[nt], acc[tx][nt]);
        acc[tx][nt] = chain_mfma<2>(ah, bl[nt], acc[tx][nt]);
        acc[tx][nt] = chain_mfma<2>(ah, bh[nt], acc[tx][nt]);
      }
    }
  }

  const float inW = a.hdr[FIRST ? H_IW1 : H_IW2], inA = FIRST ? S.iA : S.i1, sO = FIRST ? S.s1 : S.s2;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int n = nt * 32 + r;
    const float b = a.bias[n];
#pragma unroll
    for (int tx = 0; tx < TX; ++tx) {
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const f32x16& c = acc[tx][nt];
        const float m = fmaxf(fmaxf(c[4 * g4], c[4 * g4 + 1]), fmaxf(c[4 * g4 + 2], c[4 * g4 + 3]));
        const float v = m * inW * inA + b;
        const int wd = 2 * g4 + h;
        const int py = 2 * (strip * WR + wave) + (wd >> 2), px = 4 * tx + (wd & 3);
        if (n < COUT && a.feat) a.feat[(((size_t)i * COUT + n) * PW + py) * PW + px] = by_mode(v, st.mode);
        _Float16 vh, vl;
        split1(st.mode == 0 ? v : 0.f, sO, vh, vl);
        if constexpr (FIRST) {
          if (n < 8 * C1G) {
            const size_t o = ((((size_t)i * PW * PW + py * PW + px) * C1G + (n >> 3)) * 2) * 8 + (n & 7);
            a.out_split[o] = bits16(vh);
            a.out_split[o + 8] = bits16(vl);
          }
        } else {
          if (n < COUT) {
            const int k = n * (PW * PW) + py * PW + px;
            const size_t o = (((size_t)i * (FCK / 8) + (k >> 3)) * 2) * 8 + (k & 7);
            a.out_split[o] = bits16(vh);
            a.out_split[o + 8] = bits16(vl);
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ fc1 + ReLU
// grid (ceil(n / 32), 4), four waves: the workgroup's 32 images x one 32-unit tile per wave (tile 4 blockIdx.y + wave),
// K = 7200 in 450 steps straight from global fragments; the four waves read the same image rows.
__global__ __launch_bounds__(256) void fc1_kernel(const uint4* __restrict__ p2, const ImgState* __restrict__ st,
                                                  const uint4* __restrict__ w3, const float* __restrict__ c1,
                                                  const float* __restrict__ hdr, int n, float* __restrict__ hid,
                                                  float* __restrict__ feat) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int m0 = blockIdx.x * FC_ROWS, nt = blockIdx.y * 4 + (threadIdx.x >> 6);
  const uint4* a0 = p2 + (size_t)min(m0 + r, n - 1) * P2_U4 + h * 2;
  const uint4* wq = w3 + (size_t)nt * 128 + lane;
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll 4
  for (int s = 0; s < FC_STEPS; ++s) {
    const uint4 ah = a0[s * 4], al = a0[s * 4 + 1];
    const uint4 bh = wq[(size_t)s * FC_NT * 128], bl = wq[(size_t)s * FC_NT * 128 + 64];
    acc = chain_mfma<2>(al, bh, acc);
    acc = chain_mfma<2>(ah, bl, acc);
    acc = chain_mfma<2>(ah, bh, acc);
  }
  const float inW = hdr[H_IW3];
  const int u = nt * 32 + r;
  if (u >= HID) return;
  const float b = c1[u];
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int img = m0 + (e & 3) + 8 * (e >> 2) + 4 * h;
    if (img >= n) continue;
    const ImgState s = st[img];
    const Scales S = scales_of(s.amax, hdr);
    const float v = fmaxf(acc[e] * inW * S.i2 + b, 0.f);
    hid[(size_t)img * HIDP + u] = s.mode == 0 ? v : 0.f;
    if (feat) feat[(size_t)img * HID + u] = by_mode(v, s.mode);
  }
}

// ------------------------------------------------------------------------------------------------ fc2
// One wave per image, fp32 FMAs in a fixed order: lane l sums k = l, l + 64, ..., then a butterfly over the lanes.
__global__ __launch_bounds__(64) void fc2_kernel(const float* __restrict__ hid, const ImgState* __restrict__ st,
                                                 const float* __restrict__ w4, const float* __restrict__ c2, int classes,
                                                 float* __restrict__ logits) {
  const int lane = threadIdx.x, i = blockIdx.x;
  const int mode = st[i].mode;
  const float* hrow = hid + (size_t)i * HIDP;
  for (int c = 0; c < classes; ++c) {
    float acc = 0.f;
    for (int k = lane; k < HID; k += 64) acc = fmaf(hrow[k], w4[c * HIDP + k], acc);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if (lane == 0) logits[(size_t)i * classes + c] = by_mode(acc + c2[c], mode);
  }
}

inline bool dims_ok(int Cin, int classes) { return Cin >= 1 && Cin <= 12 && classes >= 1 && classes <= CLSP; }

}  // namespace gpd
}  // namespace s4g

using namespace s4g;
using namespace s4g::gpd;

extern "C" size_t s4g_gpd_pack_bytes(int Cin, int classes) {
  if (!dims_ok(Cin, classes)) return 0;
  return layout(Cin).total;
}

extern "C" int s4g_gpd_pack_f32(const float* conv1_w, const float* conv1_b, const float* conv2_w, const float* conv2_b,
                                const float* fc1_w, const float* fc1_b, const float* fc2_w, const float* fc2_b, int Cin,
                                int classes, void* packed, s4g_stream_t stream) {
  if (!dims_ok(Cin, classes) || !conv1_w || !conv1_b || !conv2_w || !conv2_b || !fc1_w || !fc1_b || !fc2_w || !fc2_b ||
      !packed || ((uintptr_t)packed & 15))
    return S4G_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const Layout L = layout(Cin);
  char* P = (char*)packed;
  float* hdr = (float*)(P + L.hdr);
  stats_kernel<<<1, 256, 0, st>>>(conv1_w, Cin * 25, conv1_b, conv2_w, conv2_b, fc1_w, hdr);
  S4G_LAUNCH_CHECK();
  pack_small_kernel<<<(CLSP * HIDP + 255) / 256, 256, 0, st>>>(conv1_b, conv2_b, fc1_b, fc2_w, fc2_b, classes,
                                                               (float*)(P + L.b1), (float*)(P + L.b2),
                                                               (float*)(P + L.c1), (float*)(P + L.w4),
                                                               (float*)(P + L.c2));
  S4G_LAUNCH_CHECK();
  pack_frag_kernel<true><<<(L.ns1 * 64 + 255) / 256, 256, 0, st>>>(conv1_w, Cin, C1, L.cg1, 1, L.ns1, hdr, H_SW1,
                                                                   (uint4*)(P + L.w1));
  S4G_LAUNCH_CHECK();
  pack_frag_kernel<true><<<(L.ns2 * 2 * 64 + 255) / 256, 256, 0, st>>>(conv2_w, C1, C2, C1G, 2, L.ns2, hdr, H_SW2,
                                                                       (uint4*)(P + L.w2));
  S4G_LAUNCH_CHECK();
  pack_frag_kernel<false><<<(FC_STEPS * FC_NT * 64 + 255) / 256, 256, 0, st>>>(fc1_w, FCK, HID, 0, FC_NT, FC_STEPS, hdr,
                                                                               H_SW3, (uint4*)(P + L.w3));
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}

static int64_t effective_chunk(int64_t chunk, int64_t G) {
  int64_t c = chunk > 0 ? chunk : DEFAULT_CHUNK;
  if (G > 0 && c > G) c = G;
  return c;
}

extern "C" size_t s4g_gpd_workspace_bytes(int64_t chunk, int Cin, int classes) {
  if (!dims_ok(Cin, classes) || chunk < 0 || chunk > MAX_CHUNK) return 0;
  return ws_layout(chunk > 0 ? chunk : DEFAULT_CHUNK).total;
}

extern "C" int s4g_gpd_forward_f32(const float* maps, int64_t image_stride, int64_t channel_stride, const int32_t* index,
                                   int64_t G, int64_t num_images, const void* packed, int Cin, int classes,
                                   int64_t chunk, float* pool1, float* pool2, float* hidden, float* logits, void* ws,
                                   size_t ws_bytes, s4g_stream_t stream) {
  if (!dims_ok(Cin, classes) || G < 0 || num_images < 0 || chunk < 0 || chunk > MAX_CHUNK || !packed ||
      ((uintptr_t)packed & 15) || G > 0x7fffffff || num_images > 0x7fffffff || image_stride < 0 || channel_stride < 0)
    return S4G_EINVAL;
  if (G == 0) return S4G_OK;
  if (!logits || (!maps && num_images > 0) || (!index && G > num_images)) return S4G_EINVAL;
  const int64_t ch = effective_chunk(chunk, G);
  const WsLayout W = ws_layout(ch);
  if (!ws || ((uintptr_t)ws & 15)) return S4G_EINVAL;
  if (ws_bytes < W.total) return S4G_EWORKSPACE;
  hipStream_t stq = (hipStream_t)stream;
  const Layout L = layout(Cin);
  const char* P = (const char*)packed;
  const float* hdr = (const float*)(P + L.hdr);
  char* wsb = (char*)ws;
  ImgState* st = (ImgState*)(wsb + W.st);
  uint4* p1s = (uint4*)(wsb + W.p1);
  uint4* p2s = (uint4*)(wsb + W.p2);
  float* hid = (float*)(wsb + W.hid);

  for (int64_t g0 = 0; g0 < G; g0 += ch) {
    const int n = (int)(G - g0 < ch ? G - g0 : ch);
    prep_kernel<<<n, 256, 0, stq>>>(maps, image_stride, channel_stride, index, g0, num_images, Cin, st);
    S4G_LAUNCH_CHECK();
    ConvArgs a1;
    a1.maps = maps; a1.istride = image_stride; a1.cstride = channel_stride; a1.Cin = Cin; a1.in_split = nullptr;
    a1.st = st; a1.wfrag = (const uint4*)(P + L.w1); a1.bias = (const float*)(P + L.b1); a1.hdr = hdr;
    a1.out_split = (uint16_t*)p1s; a1.feat = pool1 ? pool1 + (size_t)g0 * C1 * P1 * P1 : nullptr;
    if (L.cg1 == 1)
      conv_pool_kernel<1, 1, IMG, 2, 7, C1, true><<<dim3(7, n), 128, 0, stq>>>(a1);
    else
      conv_pool_kernel<2, 1, IMG, 2, 7, C1, true><<<dim3(7, n), 128, 0, stq>>>(a1);
    S4G_LAUNCH_CHECK();
    ConvArgs a2 = a1;
    a2.maps = nullptr; a2.in_split = p1s; a2.wfrag = (const uint4*)(P + L.w2); a2.bias = (const float*)(P + L.b2);
    a2.out_split = (uint16_t*)p2s; a2.feat = pool2 ? pool2 + (size_t)g0 * C2 * P2 * P2 : nullptr;
    conv_pool_kernel<C1G, 2, P1, 3, 3, C2, false><<<dim3(2, n), 192, 0, stq>>>(a2);
    S4G_LAUNCH_CHECK();
    fc1_kernel<<<dim3((n + FC_ROWS - 1) / FC_ROWS, FC_NT / 4), 256, 0, stq>>>(p2s, st, (const uint4*)(P + L.w3),
                                                                     (const float*)(P + L.c1), hdr, n, hid,
                                                                     hidden ? hidden + (size_t)g0 * HID : nullptr);
    S4G_LAUNCH_CHECK();
    fc2_kernel<<<n, 64, 0, stq>>>(hid, st, (const float*)(P + L.w4), (const float*)(P + L.c2), classes,
                                  logits + (size_t)g0 * classes);
    S4G_LAUNCH_CHECK();
  }
  return S4G_OK;
}
