// The training objective and metric of the three S4G networks, fused: reference network_models/models/
// PointNet2_tcls.py:156-267 (variant 0, the curvature model) and PointNet2.py:156-258 (variant 1, the contact and edge
// models), with smooth_cross_entropy of nn_utils/functional.py:91-114.  One call gives the four losses AND the unit
// gradient of each loss with respect to its own prediction tensor; include/s4g_ops.h states the semantics.
//
// Three launches, no float atomics, no host read:
//   1. loss_label_hist_kernel: the labels alone.  Per LOSS_HIST_TILE consecutive labels one row of integer counts (the
//      classes of the score labels; the non-ignored best_frame_t of variant 0; the labels outside their range).  The
//      denominators sum w[y_i] and count(best_frame_t != -100) follow from integers, so they do not depend on any order.
//   2. loss_main_kernel: one workgroup per fixed tile of LOSS_TILE points of one scene, LOSS_PTS points per thread, the
//      channels looped.  Every prediction is read once and its final gradient written once.  Per-point terms in fp32
//      (expf / logf on max-subtracted logits), accumulated in double: wave sums by shuffles over 64 lanes, then LDS, one
//      partial per loss and tile.  The tile is a constant, so the partials do not depend on the grid.
//   3. loss_finish_kernel: one workgroup sums the partials in tile order in double, divides once and rounds to fp32 once.
//
// Vector access: a channel row starts at (b C + c) N floats, 16-byte aligned only where N % 4 == 0 (and the tensor's
// base is).  Exactly then a thread takes its LOSS_PTS = 4 consecutive points with one float4 per channel; otherwise the
// scalar path (points tid + 256 j).  The label rows of length F are always read with scalar loads.
#include "s4g_common.h"

namespace s4g {

constexpr int LOSS_THREADS = 256;
constexpr int LOSS_PTS = 4;                          // points per thread
constexpr int LOSS_TILE = 1024;                      // points per workgroup = LOSS_THREADS * LOSS_PTS
constexpr int LOSS_HIST_TILE = 4096;                 // labels per histogram row
constexpr int LOSS_HIST_COLS = 16;                   // 0..7 class counts (t rows: 0 = valid labels), 8 = out of range
constexpr int LOSS_MAX_CH = 8;                       // C, D, Ct <= 8
constexpr int64_t LOSS_MAX_POINTS = (1ll << 31) - 1; // B * N
constexpr int64_t LOSS_MAX_B = 65535;
constexpr int64_t LOSS_IGNORE = -100;                // torch's default ignore_index
static_assert(LOSS_TILE == LOSS_THREADS * LOSS_PTS, "one tile = four points per thread");

struct LossWs {
  int32_t* hist;      // (rows_n + rows_f, LOSS_HIST_COLS)
  double* partial;    // (B * tiles, 4)
  int rows_n, rows_f, tiles;
};

__host__ __device__ inline int64_t loss_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

static size_t loss_ws_layout(int64_t B, int64_t N, int64_t F, void* ws, LossWs* out) {
  const int64_t rows_n = loss_ceil_div(B * N, LOSS_HIST_TILE), rows_f = loss_ceil_div(B * F, LOSS_HIST_TILE);
  const int64_t tiles = loss_ceil_div(N, LOSS_TILE);
  size_t hist_bytes = (size_t)(rows_n + rows_f) * LOSS_HIST_COLS * sizeof(int32_t);
  hist_bytes = (hist_bytes + 255) & ~(size_t)255;
  const size_t part_bytes = (size_t)(B * tiles) * 4 * sizeof(double);
  if (out) {
    out->hist = (int32_t*)ws;
    out->partial = (double*)((char*)ws + hist_bytes);
    out->rows_n = (int)rows_n;
    out->rows_f = (int)rows_f;
    out->tiles = (int)tiles;
  }
  return hist_bytes + part_bytes;
}

// ---------------------------------------------------------------------------------------------------- 1. label pre-pass
__global__ __launch_bounds__(LOSS_THREADS) void loss_label_hist_kernel(const int64_t* __restrict__ score_labels,
                                                                       const int64_t* __restrict__ t_labels, int64_t BN,
                                                                       int64_t BF, int C, int Ct, int rows_n,
                                                                       int32_t* __restrict__ hist) {
  __shared__ int h[LOSS_HIST_COLS];
  const int tid = threadIdx.x, r = blockIdx.x;
  if (tid < LOSS_HIST_COLS) h[tid] = 0;
  __syncthreads();
  const bool is_t = r >= rows_n;
  const int64_t* lab = is_t ? t_labels : score_labels;
  const int64_t count = is_t ? BF : BN, first = (int64_t)(is_t ? r - rows_n : r) * LOSS_HIST_TILE;
  const int K = is_t ? Ct : C;
  for (int k = 0; k < LOSS_HIST_TILE / LOSS_THREADS; ++k) {
    const int64_t i = first + tid + (int64_t)k * LOSS_THREADS;
    if (i >= count) break;
    const int64_t y = lab[i];
    if (y >= 0 && y < K) atomicAdd(&h[is_t ? 0 : (int)y], 1);          // integer LDS counts: no order to depend on
    else if (y != LOSS_IGNORE) atomicAdd(&h[8], 1);
  }
  __syncthreads();
  if (tid < LOSS_HIST_COLS) hist[(size_t)r * LOSS_HIST_COLS + tid] = h[tid];
}

// The column totals of the histogram rows: tot[0][c] over the score rows, tot[1][c] over the best_frame_t rows.
__device__ __forceinline__ void loss_hist_totals(const int32_t* __restrict__ hist, int rows_n, int rows_f,
                                                 unsigned long long (&tot)[2][LOSS_HIST_COLS]) {
  const int tid = threadIdx.x, col = tid & (LOSS_HIST_COLS - 1);
  if (tid < 2 * LOSS_HIST_COLS) tot[tid >> 4][col] = 0ull;
  __syncthreads();
  unsigned long long a = 0ull, b = 0ull;
  for (int r = tid >> 4; r < rows_n + rows_f; r += LOSS_THREADS / LOSS_HIST_COLS) {
    const unsigned long long v = (unsigned long long)hist[(size_t)r * LOSS_HIST_COLS + col];
    if (r < rows_n) a += v; else b += v;
  }
  if (a) atomicAdd(&tot[0][col], a);
  if (b) atomicAdd(&tot[1][col], b);
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------- tile access helpers
template <bool VEC>
__device__ __forceinline__ int loss_point(int base, int tid, int j) {
  return VEC ? base + LOSS_PTS * tid + j : base + tid + LOSS_THREADS * j;
}

// v[j] = row[point j] for the points below `lim` (0 elsewhere).  VEC: lim and the row start are multiples of 4 floats
// where a float4 is taken, or the four points are tested one by one (lim = F on a row of length N).
template <bool VEC>
__device__ __forceinline__ void loss_load4(const float* __restrict__ row, int base, int tid, int lim, float (&v)[LOSS_PTS]) {
  if constexpr (VEC) {
    const int n = base + LOSS_PTS * tid;
    if (n < lim) {                 // n + 3 < N: the row has a multiple of 4 entries and n is one
      const float4 t = *reinterpret_cast<const float4*>(row + n);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
      v[0] = v[1] = v[2] = v[3] = 0.f;
    }
  } else {
#pragma unroll
    for (int j = 0; j < LOSS_PTS; ++j) {
      const int n = base + tid + LOSS_THREADS * j;
      v[j] = n < lim ? row[n] : 0.f;
    }
  }
}

template <bool VEC>
__device__ __forceinline__ void loss_store4(float* __restrict__ row, int base, int tid, int N, const float (&v)[LOSS_PTS]) {
  if constexpr (VEC) {
    const int n = base + LOSS_PTS * tid;
    if (n < N) *reinterpret_cast<float4*>(row + n) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < LOSS_PTS; ++j) {
      const int n = base + tid + LOSS_THREADS * j;
      if (n < N) row[n] = v[j];
    }
  }
}

__device__ __forceinline__ double loss_wave_sum(double v) {
#pragma unroll
  for (int o = S4G_WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o, S4G_WAVE);
  return v;                                                            // lane 0 holds the wave's sum
}

// The workgroup's sums of acc[0..K), waves in order; valid in thread 0.
template <int K>
__device__ __forceinline__ void loss_block_sum(double (&acc)[K], double (*red)[4]) {
  const int tid = threadIdx.x, wave = tid / S4G_WAVE, lane = tid % S4G_WAVE;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double s = loss_wave_sum(acc[k]);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

// softmax and log-softmax of the K <= 8 channels of one point on max-subtracted logits (fp32, as torch's)
__device__ __forceinline__ void loss_softmax8(const float (&v)[LOSS_MAX_CH], int K, float (&sm)[LOSS_MAX_CH],
                                              float (&lp)[LOSS_MAX_CH]) {
  float m = v[0];
#pragma unroll
  for (int c = 1; c < LOSS_MAX_CH; ++c)
    if (c < K) m = fmaxf(m, v[c]);
  float e[LOSS_MAX_CH], s = 0.f;
#pragma unroll
  for (int c = 0; c < LOSS_MAX_CH; ++c)
    if (c < K) { e[c] = expf(v[c] - m); s += e[c]; }
  const float ls = logf(s);
#pragma unroll
  for (int c = 0; c < LOSS_MAX_CH; ++c) {
    sm[c] = c < K ? e[c] / s : 0.f;
    lp[c] = c < K ? (v[c] - m) - ls : 0.f;
  }
}

// the smaller of two values as torch.min takes it: the first on a tie, a NaN wins
__device__ __forceinline__ bool loss_second_wins(float a, float b) { return b < a || (b != b && a == a); }

struct LossArgs {
  s4g_loss_desc_t d;
  LossWs ws;
};

// --------------------------------------------------------------------------------------------------------- 2. main pass
template <bool VEC>
__global__ __launch_bounds__(LOSS_THREADS) void loss_main_kernel(const LossArgs a) {
  __shared__ unsigned long long tot[2][LOSS_HIST_COLS];
  __shared__ double red[4][4];
  const s4g_loss_desc_t& d = a.d;
  const int tid = threadIdx.x, b = blockIdx.y, base = blockIdx.x * LOSS_TILE;
  const int N = d.N, F = d.F, C = d.C, D = d.D, Ct = d.Ct;
  loss_hist_totals(a.ws.hist, a.ws.rows_n, a.ws.rows_f, tot);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};                               // cls, R, t, mov

  // ---- cls
  {
    const bool smooth = d.label_smoothing > 0.f;
    float scale;
    if (smooth) {
      scale = (float)(1.0 / ((double)d.B * (double)N));
    } else {
      double den = 0.0;
#pragma unroll
      for (int c = 0; c < LOSS_MAX_CH; ++c)
        if (c < C) den += (double)d.w[c] * (double)tot[0][c];
      scale = (float)(1.0 / den);
    }
    float v[LOSS_MAX_CH][LOSS_PTS], g[LOSS_MAX_CH][LOSS_PTS];
#pragma unroll
    for (int c = 0; c < LOSS_MAX_CH; ++c) {
      if (c < C) loss_load4<VEC>(d.score_logits + ((size_t)b * C + c) * N, base, tid, N, v[c]);
#pragma unroll
      for (int j = 0; j < LOSS_PTS; ++j) g[c][j] = 0.f;
    }
    const float ls = d.label_smoothing, off = ls / (float)C;
#pragma unroll
    for (int j = 0; j < LOSS_PTS; ++j) {
      const int n = loss_point<VEC>(base, tid, j);
      if (n >= N) continue;
      const int64_t y = d.score_labels[(size_t)b * N + n];
      if (y < 0 || y >= C) continue;                                   // -100 and out-of-range: nothing, zero gradient
      float x[LOSS_MAX_CH], sm[LOSS_MAX_CH], lp[LOSS_MAX_CH];
#pragma unroll
      for (int c = 0; c < LOSS_MAX_CH; ++c) x[c] = v[c][j];
      loss_softmax8(x, C, sm, lp);
      if (smooth) {                                                    // weight by class, plain mean over B N
        float term = 0.f, sw = 0.f;
#pragma unroll
        for (int c = 0; c < LOSS_MAX_CH; ++c)
          if (c < C) {
            const float s = (c == (int)y ? 1.f - ls : 0.f) + off;
            term += s * lp[c] * d.w[c];
            sw += s * d.w[c];
          }
        acc[0] += (double)(-term);
#pragma unroll
        for (int c = 0; c < LOSS_MAX_CH; ++c)
          if (c < C) {
            const float s = (c == (int)y ? 1.f - ls : 0.f) + off;
            g[c][j] = (sw * sm[c] - s * d.w[c]) * scale;
          }
      } else {                                                         // torch's weighted mean
        float wy = 0.f, lpy = 0.f;
#pragma unroll
        for (int c = 0; c < LOSS_MAX_CH; ++c)
          if (c == (int)y) { wy = d.w[c]; lpy = lp[c]; }
        acc[0] += (double)(-(wy * lpy));
#pragma unroll
        for (int c = 0; c < LOSS_MAX_CH; ++c)
          if (c < C) g[c][j] = wy * (sm[c] - (c == (int)y ? 1.f : 0.f)) * scale;
      }
    }
    if (d.g_score) {
#pragma unroll
      for (int c = 0; c < LOSS_MAX_CH; ++c)
        if (c < C) loss_store4<VEC>(d.g_score + ((size_t)b * C + c) * N, base, tid, N, g[c]);
    }
  }

  // ---- mov: L1, sign(0) = 0
  {
    const float scale = (float)(1.0 / ((double)d.B * (double)D * (double)N));
    for (int c = 0; c < D; ++c) {
      float p[LOSS_PTS], y[LOSS_PTS], g[LOSS_PTS];
      loss_load4<VEC>(d.movable + ((size_t)b * D + c) * N, base, tid, N, p);
      loss_load4<VEC>(d.movable_labels + ((size_t)b * D + c) * N, base, tid, N, y);
#pragma unroll
      for (int j = 0; j < LOSS_PTS; ++j) {
        const float diff = p[j] - y[j];                                // 0 for the points past N
        acc[3] += (double)fabsf(diff);
        g[j] = (float)((diff > 0.f) - (diff < 0.f)) * scale;
      }
      if (d.g_movable) loss_store4<VEC>(d.g_movable + ((size_t)b * D + c) * N, base, tid, N, g);
    }
  }

  const bool tile_has_frames = base < F;                               // uniform: the tile holds a point below F
  // ---- R: min over the two sign branches of the label frame, weighted by scene_score
  if (tile_has_frames) {
    const double kR = 10.0 / (9.0 * (double)d.B * (double)F);
    float p[9][LOSS_PTS], g[9][LOSS_PTS];
#pragma unroll
    for (int c = 0; c < 9; ++c) loss_load4<VEC>(d.frame_R + ((size_t)b * 9 + c) * N, base, tid, F, p[c]);
#pragma unroll
    for (int j = 0; j < LOSS_PTS; ++j) {
      const int n = loss_point<VEC>(base, tid, j);
      const bool in = n < F;
      float gt[9], s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int c = 0; c < 9; ++c) {
        gt[c] = in ? d.best_frame_R[((size_t)b * 9 + c) * F + n] : 0.f;
        const bool neg = c % 3 != 0;                                   // columns 1 and 2 of the row-major frame
        const float d1 = p[c][j] - gt[c], d2 = neg ? p[c][j] + gt[c] : d1;
        s1 += d1 * d1;
        s2 += d2 * d2;
      }
      const bool second = loss_second_wins(s1, s2);                    // a tie takes branch 1
      const float sc = in ? d.scene_score[(size_t)b * d.scene_score_stride + n] : 0.f;
      if (in) acc[1] += (double)(second ? s2 : s1) * (double)sc;
      const double k = (double)sc * kR;
#pragma unroll
      for (int c = 0; c < 9; ++c) {
        const float diff = (second && c % 3 != 0) ? p[c][j] + gt[c] : p[c][j] - gt[c];
        g[c][j] = in ? (float)((double)diff * k) : 0.f;
      }
    }
    if (d.g_R) {
#pragma unroll
      for (int c = 0; c < 9; ++c) loss_store4<VEC>(d.g_R + ((size_t)b * 9 + c) * N, base, tid, N, g[c]);
    }
  } else if (d.g_R) {
    const float z[LOSS_PTS] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 9; ++c) loss_store4<VEC>(d.g_R + ((size_t)b * 9 + c) * N, base, tid, N, z);
  }

  // ---- t
  if (tile_has_frames && d.variant == 0) {                             // unweighted cross entropy over the F points
    const float scale = (float)(0.2 / (double)tot[1][0]);
    const int64_t* tl = (const int64_t*)d.best_frame_t;
    float v[LOSS_MAX_CH][LOSS_PTS], g[LOSS_MAX_CH][LOSS_PTS];
#pragma unroll
    for (int c = 0; c < LOSS_MAX_CH; ++c) {
      if (c < Ct) loss_load4<VEC>(d.frame_t + ((size_t)b * Ct + c) * N, base, tid, F, v[c]);
#pragma unroll
      for (int j = 0; j < LOSS_PTS; ++j) g[c][j] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < LOSS_PTS; ++j) {
      const int n = loss_point<VEC>(base, tid, j);
      if (n >= F) continue;
      const int64_t y = tl[(size_t)b * F + n];
      if (y < 0 || y >= Ct) continue;
      float x[LOSS_MAX_CH], sm[LOSS_MAX_CH], lp[LOSS_MAX_CH];
#pragma unroll
      for (int c = 0; c < LOSS_MAX_CH; ++c) x[c] = v[c][j];
      loss_softmax8(x, Ct, sm, lp);
      float lpy = 0.f;
#pragma unroll
      for (int c = 0; c < LOSS_MAX_CH; ++c)
        if (c == (int)y) lpy = lp[c];
      acc[2] += (double)(-lpy);
#pragma unroll
      for (int c = 0; c < LOSS_MAX_CH; ++c)
        if (c < Ct) g[c][j] = (sm[c] - (c == (int)y ? 1.f : 0.f)) * scale;
    }
    if (d.g_t) {
#pragma unroll
      for (int c = 0; c < LOSS_MAX_CH; ++c)
        if (c < Ct) loss_store4<VEC>(d.g_t + ((size_t)b * Ct + c) * N, base, tid, N, g[c]);
    }
  } else if (tile_has_frames) {                                        // squared offset error weighted by scene_score
    const double kT = 40.0 / ((double)d.B * (double)F);
    const float* tl = (const float*)d.best_frame_t;
    float p[3][LOSS_PTS], g[3][LOSS_PTS];
#pragma unroll
    for (int c = 0; c < 3; ++c) loss_load4<VEC>(d.frame_t + ((size_t)b * 3 + c) * N, base, tid, F, p[c]);
#pragma unroll
    for (int j = 0; j < LOSS_PTS; ++j) {
      const int n = loss_point<VEC>(base, tid, j);
      const bool in = n < F;
      const float sc = in ? d.scene_score[(size_t)b * d.scene_score_stride + n] : 0.f;
      float diff[3], s = 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        diff[c] = p[c][j] - (in ? tl[((size_t)b * 3 + c) * F + n] : 0.f);
        s += diff[c] * diff[c];
      }
      if (in) acc[2] += (double)s * (double)sc;
      const double k = (double)sc * kT;
#pragma unroll
      for (int c = 0; c < 3; ++c) g[c][j] = in ? (float)((double)diff[c] * k) : 0.f;
    }
    if (d.g_t) {
#pragma unroll
      for (int c = 0; c < 3; ++c) loss_store4<VEC>(d.g_t + ((size_t)b * 3 + c) * N, base, tid, N, g[c]);
    }
  } else if (d.g_t) {
    const float z[LOSS_PTS] = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < Ct; ++c) loss_store4<VEC>(d.g_t + ((size_t)b * Ct + c) * N, base, tid, N, z);
  }

  loss_block_sum<4>(acc, red);
  if (tid == 0) {
    double* out = a.ws.partial + ((size_t)b * a.ws.tiles + blockIdx.x) * 4;
    out[0] = acc[0]; out[1] = acc[1]; out[2] = acc[2]; out[3] = acc[3];
  }
}

// The sums of K columns of `partial` (count rows of 4 doubles) in a fixed order: thread t takes rows t, t + 256, ... in
// ascending order, then a fixed tree over the threads.  Valid in thread 0.
template <int K>
__device__ __forceinline__ void loss_ordered_sum(const double* __restrict__ partial, int64_t count, double (&out)[K],
                                                 double (*tree)[LOSS_THREADS]) {
  const int tid = threadIdx.x;
  double s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = 0.0;
  for (int64_t r = tid; r < count; r += LOSS_THREADS) {
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] += partial[(size_t)r * 4 + k];
  }
#pragma unroll
  for (int k = 0; k < K; ++k) tree[k][tid] = s[k];
  __syncthreads();
  for (int w = LOSS_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) {
#pragma unroll
      for (int k = 0; k < K; ++k) tree[k][tid] += tree[k][tid + w];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < K; ++k) out[k] = tree[k][0];
}

// ------------------------------------------------------------------------------------------------------------ 3. finish
__global__ __launch_bounds__(LOSS_THREADS) void loss_finish_kernel(const LossArgs a) {
  __shared__ unsigned long long tot[2][LOSS_HIST_COLS];
  __shared__ double tree[4][LOSS_THREADS];
  const s4g_loss_desc_t& d = a.d;
  loss_hist_totals(a.ws.hist, a.ws.rows_n, a.ws.rows_f, tot);
  double sum[4];
  loss_ordered_sum<4>(a.ws.partial, (int64_t)d.B * a.ws.tiles, sum, tree);
  if (threadIdx.x != 0) return;
  const double BN = (double)d.B * (double)d.N, BF = (double)d.B * (double)d.F;
  double den_cls = BN;
  if (!(d.label_smoothing > 0.f)) {
    den_cls = 0.0;
    for (int c = 0; c < d.C; ++c) den_cls += (double)d.w[c] * (double)tot[0][c];
  }
  d.losses[0] = (float)(sum[0] / den_cls);                             // 0 / 0 = NaN where every label is ignored
  d.losses[1] = (float)(sum[1] * 5.0 / (9.0 * BF));                    // F == 0: NaN, as torch's mean of nothing
  d.losses[2] = d.variant == 0 ? (float)(sum[2] * 0.2 / (double)tot[1][0]) : (float)(sum[2] * 20.0 / BF);
  d.losses[3] = (float)(sum[3] / (BN * (double)d.D));
  d.status[0] = (tot[0][8] ? 1 : 0) | (tot[1][8] ? 2 : 0);
}

// ------------------------------------------------------------------------------------------------------------- metric
template <bool VEC>
__global__ __launch_bounds__(LOSS_THREADS) void metric_main_kernel(const LossArgs a) {
  __shared__ double red[4][4];
  const s4g_loss_desc_t& d = a.d;
  const int tid = threadIdx.x, b = blockIdx.y, base = blockIdx.x * LOSS_TILE;
  const int N = d.N, F = d.F, C = d.C, D = d.D, Ct = d.Ct;
  double acc[2] = {0.0, 0.0};                                          // R_err, t_err

  {                                                                    // cls_acc: the lowest index wins a tie
    float best[LOSS_PTS], v[LOSS_PTS];
    int arg[LOSS_PTS] = {0, 0, 0, 0};
    loss_load4<VEC>(d.score_logits + (size_t)b * C * N, base, tid, N, best);
    for (int c = 1; c < C; ++c) {
      loss_load4<VEC>(d.score_logits + ((size_t)b * C + c) * N, base, tid, N, v);
#pragma unroll
      for (int j = 0; j < LOSS_PTS; ++j)
        if (v[j] > best[j]) { best[j] = v[j]; arg[j] = c; }
    }
#pragma unroll
    for (int j = 0; j < LOSS_PTS; ++j) {
      const int n = loss_point<VEC>(base, tid, j);
      if (n < N) d.cls_acc[(size_t)b * N + n] = (int64_t)arg[j] == d.score_labels[(size_t)b * N + n] ? 1.f : 0.f;
    }
  }
  for (int c = 0; c < D; ++c) {                                        // mov_acc: (p > 0.5) against int(label)
    float p[LOSS_PTS], y[LOSS_PTS], r[LOSS_PTS];
    loss_load4<VEC>(d.movable + ((size_t)b * D + c) * N, base, tid, N, p);
    loss_load4<VEC>(d.movable_labels + ((size_t)b * D + c) * N, base, tid, N, y);
#pragma unroll
    for (int j = 0; j < LOSS_PTS; ++j) r[j] = (p[j] > 0.5f ? 1 : 0) == (int)y[j] ? 1.f : 0.f;
    loss_store4<VEC>(d.mov_acc + ((size_t)b * D + c) * N, base, tid, N, r);
  }
  if (base < F) {
    float p[9][LOSS_PTS];
#pragma unroll
    for (int c = 0; c < 9; ++c) loss_load4<VEC>(d.frame_R + ((size_t)b * 9 + c) * N, base, tid, F, p[c]);
#pragma unroll
    for (int j = 0; j < LOSS_PTS; ++j) {
      const int n = loss_point<VEC>(base, tid, j);
      if (n >= F) continue;
      float tr1 = 0.f, tr2 = 0.f;                                      // trace(G P^T) = sum_9 g p
#pragma unroll
      for (int c = 0; c < 9; ++c) {
        const float m = d.best_frame_R[((size_t)b * 9 + c) * F + n] * p[c][j];
        tr1 += m;
        tr2 += c % 3 != 0 ? -m : m;
      }
      float c1 = (tr1 - 1.f) / 2.f, c2 = (tr2 - 1.f) / 2.f;
      c1 = c1 < -1.f ? -1.f : (c1 > 1.f ? 1.f : c1);                   // NaN passes through, as torch.clamp
      c2 = c2 < -1.f ? -1.f : (c2 > 1.f ? 1.f : c2);
      const float a1 = acosf(c1), a2 = acosf(c2);
      const float m = loss_second_wins(a1, a2) ? a2 : a1;
      acc[0] += (double)(d.scene_score[(size_t)b * d.scene_score_stride + n] * m);
    }
    if (d.variant == 0) {                                              // t_acc
      const int64_t* tl = (const int64_t*)d.best_frame_t;
      float best[LOSS_PTS], v[LOSS_PTS];
      int arg[LOSS_PTS] = {0, 0, 0, 0};
      loss_load4<VEC>(d.frame_t + (size_t)b * Ct * N, base, tid, F, best);
      for (int c = 1; c < Ct; ++c) {
        loss_load4<VEC>(d.frame_t + ((size_t)b * Ct + c) * N, base, tid, F, v);
#pragma unroll
        for (int j = 0; j < LOSS_PTS; ++j)
          if (v[j] > best[j]) { best[j] = v[j]; arg[j] = c; }
      }
#pragma unroll
      for (int j = 0; j < LOSS_PTS; ++j) {
        const int n = loss_point<VEC>(base, tid, j);
        if (n < F) d.t_acc[(size_t)b * F + n] = (int64_t)arg[j] == tl[(size_t)b * F + n] ? 1.f : 0.f;
      }
    } else {                                                           // t_err
      const float* tl = (const float*)d.best_frame_t;
      float p3[3][LOSS_PTS];
#pragma unroll
      for (int c = 0; c < 3; ++c) loss_load4<VEC>(d.frame_t + ((size_t)b * 3 + c) * N, base, tid, F, p3[c]);
#pragma unroll
      for (int j = 0; j < LOSS_PTS; ++j) {
        const int n = loss_point<VEC>(base, tid, j);
        if (n >= F) continue;
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float diff = tl[((size_t)b * 3 + c) * F + n] - p3[c][j];
          s += diff * diff;
        }
        acc[1] += (double)sqrtf(s);
      }
    }
  }
  loss_block_sum<2>(acc, red);
  if (tid == 0) {
    double* out = a.ws.partial + ((size_t)b * a.ws.tiles + blockIdx.x) * 4;
    out[0] = acc[0]; out[1] = acc[1];
  }
}

__global__ __launch_bounds__(LOSS_THREADS) void metric_finish_kernel(const LossArgs a) {
  __shared__ double tree[2][LOSS_THREADS];
  const s4g_loss_desc_t& d = a.d;
  double sum[2];
  loss_ordered_sum<2>(a.ws.partial, (int64_t)d.B * a.ws.tiles, sum, tree);
  if (threadIdx.x != 0) return;
  const double BF = (double)d.B * (double)d.F;
  d.metrics[0] = (float)(sum[0] / BF);
  d.metrics[1] = d.variant == 0 ? 0.f : (float)(sum[1] / BF);
}

static bool loss_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Everything both entries refuse, before any launch.
static int loss_check(const s4g_loss_desc_t* d, LossWs* ws) {
  if (!d) return S4G_EINVAL;
  if (d->variant != 0 && d->variant != 1) return S4G_EINVAL;
  if (d->B < 1 || d->N < 1 || d->F < 0 || d->F > d->N) return S4G_EINVAL;
  if ((int64_t)d->B > LOSS_MAX_B || (int64_t)d->B * d->N > LOSS_MAX_POINTS) return S4G_EINVAL;
  if (d->C < 2 || d->C > LOSS_MAX_CH || d->D < 1 || d->D > LOSS_MAX_CH) return S4G_EINVAL;
  if (d->variant == 0 ? (d->Ct < 2 || d->Ct > LOSS_MAX_CH) : d->Ct != 3) return S4G_EINVAL;
  if (d->scene_score_stride < d->F) return S4G_EINVAL;
  if (!(d->label_smoothing >= 0.f && d->label_smoothing < 1.f)) return S4G_EINVAL;
  if (!d->score_logits || !d->movable || !d->frame_R || !d->frame_t || !d->score_labels || !d->movable_labels)
    return S4G_EINVAL;
  if (d->F > 0 && (!d->best_frame_R || !d->best_frame_t || !d->scene_score)) return S4G_EINVAL;
  if (!d->ws || ((uintptr_t)d->ws & 255)) return S4G_EWORKSPACE;
  if (d->ws_bytes < loss_ws_layout(d->B, d->N, d->F, d->ws, ws)) return S4G_EWORKSPACE;
  return S4G_OK;
}

}  // namespace s4g

extern "C" size_t s4g_grasp_loss_workspace_bytes(int64_t B, int64_t N, int64_t F) {
  if (B < 1 || N < 1 || F < 0 || F > N || B > s4g::LOSS_MAX_B || B * N > s4g::LOSS_MAX_POINTS) return 0;
  return s4g::loss_ws_layout(B, N, F, nullptr, nullptr);
}

extern "C" int s4g_grasp_loss_f32(const s4g_loss_desc_t* desc, s4g_stream_t stream) {
  using namespace s4g;
  LossArgs a;
  const int rc = loss_check(desc, &a.ws);
  if (rc != S4G_OK) return rc;
  a.d = *desc;
  if (!a.d.losses || !a.d.status) return S4G_EINVAL;
  if (a.d.variant == 1) a.ws.rows_f = 0;                               // float labels: no histogram of best_frame_t
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(loss_label_hist_kernel, dim3((unsigned)(a.ws.rows_n + a.ws.rows_f)), dim3(LOSS_THREADS), 0, st,
                     a.d.score_labels, (const int64_t*)a.d.best_frame_t, (int64_t)a.d.B * a.d.N,
                     (int64_t)a.d.B * a.d.F, a.d.C, a.d.Ct, a.ws.rows_n, a.ws.hist);
  S4G_LAUNCH_CHECK();
  const bool vec = a.d.N % 4 == 0 && loss_aligned16(a.d.score_logits) && loss_aligned16(a.d.movable) &&
                   loss_aligned16(a.d.frame_R) && loss_aligned16(a.d.frame_t) && loss_aligned16(a.d.movable_labels) &&
                   loss_aligned16(a.d.g_score) && loss_aligned16(a.d.g_movable) && loss_aligned16(a.d.g_R) &&
                   loss_aligned16(a.d.g_t);
  const dim3 grid((unsigned)a.ws.tiles, (unsigned)a.d.B);
  if (vec) hipLaunchKernelGGL(loss_main_kernel<true>, grid, dim3(LOSS_THREADS), 0, st, a);
  else hipLaunchKernelGGL(loss_main_kernel<false>, grid, dim3(LOSS_THREADS), 0, st, a);
  S4G_LAUNCH_CHECK();
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(LOSS_THREADS), 0, st, a);
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}

extern "C" int s4g_grasp_metric_f32(const s4g_loss_desc_t* desc, s4g_stream_t stream) {
  using namespace s4g;
  LossArgs a;
  const int rc = loss_check(desc, &a.ws);
  if (rc != S4G_OK) return rc;
  a.d = *desc;
  if (!a.d.cls_acc || !a.d.mov_acc || !a.d.metrics) return S4G_EINVAL;
  if (a.d.variant == 0 && a.d.F > 0 && !a.d.t_acc) return S4G_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = a.d.N % 4 == 0 && loss_aligned16(a.d.score_logits) && loss_aligned16(a.d.movable) &&
                   loss_aligned16(a.d.frame_R) && loss_aligned16(a.d.frame_t) && loss_aligned16(a.d.movable_labels) &&
                   loss_aligned16(a.d.mov_acc);
  const dim3 grid((unsigned)a.ws.tiles, (unsigned)a.d.B);
  if (vec) hipLaunchKernelGGL(metric_main_kernel<true>, grid, dim3(LOSS_THREADS), 0, st, a);
  else hipLaunchKernelGGL(metric_main_kernel<false>, grid, dim3(LOSS_THREADS), 0, st, a);
  S4G_LAUNCH_CHECK();
  hipLaunchKernelGGL(metric_finish_kernel, dim3(1), dim3(LOSS_THREADS), 0, st, a);
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}
