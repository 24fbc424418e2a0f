// Output tail of the contact network (`MODEL.TYPE: "PN2"`, reference network_models/models/PointNet2.py:125-147):
// the heads launch writes the raw logits, this one elementwise launch turns them into the network's outputs.
//
//   raw (B, 17, M):  score 3 | R 6 | t 3 | movable 5   (movable already through its sigmoid)
//   out (B, 20, M):  score 3 | frame_R 9 | frame_t 3 | movable 5
//
//   frame_R = toRotMatrix(R) (functions/functions.py:179-190): b1 = a1 / |a1|, b2 = a2 - (a2.b1) b1, b2 /= |b2|,
//             b3 = b1 x b2, stack([b1, b2, b3], dim=2) -> channel 3i + j = b_j[i]  (ONE projection, as torch's)
//   frame_t = points + t                               (PointNet2.py:137)
//
// One thread per point, channel-first loads and stores (consecutive lanes, consecutive points).  Plain sqrtf and
// division (the library is built with -ffp-contract=off and this file keeps NaN semantics): a zero a1 or an a2
// parallel to it gives NaN in that point's frame_R, as torch does, and nothing else.
#include "s4g_common.h"

namespace s4g {

constexpr int CONTACT_RAW_C = 17, CONTACT_OUT_C = 20;

__global__ __launch_bounds__(256) void contact_heads_kernel(const float* __restrict__ raw, const float* __restrict__ xyz,
                                                            const int64_t* __restrict__ index, int M, int N,
                                                            float* __restrict__ out) {
  const int b = blockIdx.y;
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const float* in = raw + (size_t)b * CONTACT_RAW_C * M + m;
  float* o = out + (size_t)b * CONTACT_OUT_C * M + m;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[(size_t)c * M] = in[(size_t)c * M];                 // score logits
#pragma unroll
  for (int c = 0; c < 5; ++c) o[(size_t)(15 + c) * M] = in[(size_t)(12 + c) * M];   // movable (sigmoid applied)
  // frame_R
  float x0 = in[(size_t)3 * M], x1 = in[(size_t)4 * M], x2 = in[(size_t)5 * M];
  float y0 = in[(size_t)6 * M], y1 = in[(size_t)7 * M], y2 = in[(size_t)8 * M];
  const float xn = sqrtf(x0 * x0 + x1 * x1 + x2 * x2);
  x0 /= xn; x1 /= xn; x2 /= xn;
  const float d = y0 * x0 + y1 * x1 + y2 * x2;
  y0 -= d * x0; y1 -= d * x1; y2 -= d * x2;
  const float yn = sqrtf(y0 * y0 + y1 * y1 + y2 * y2);
  y0 /= yn; y1 /= yn; y2 /= yn;
  const float z0 = x1 * y2 - x2 * y1, z1 = x2 * y0 - x0 * y2, z2 = x0 * y1 - x1 * y0;
  o[(size_t)3 * M] = x0;  o[(size_t)4 * M] = y0;  o[(size_t)5 * M] = z0;
  o[(size_t)6 * M] = x1;  o[(size_t)7 * M] = y1;  o[(size_t)8 * M] = z1;
  o[(size_t)9 * M] = x2;  o[(size_t)10 * M] = y2; o[(size_t)11 * M] = z2;
  // frame_t: the point's coordinates (of the scene's point index[b, m] for a top-K forward) + the offsets
  const int64_t n = index ? index[(size_t)b * M + m] : (int64_t)m;
  if (n >= 0 && n < N) {
    const float* p = xyz + (size_t)b * 3 * N + n;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[(size_t)(12 + c) * M] = p[(size_t)c * N] + in[(size_t)(9 + c) * M];
  } else {                                  // out of contract (index outside the scene): no read, a visible NaN
#pragma unroll
    for (int c = 0; c < 3; ++c) o[(size_t)(12 + c) * M] = __builtin_nanf("");
  }
}

}  // namespace s4g

extern "C" int s4g_contact_heads_f32(const float* raw_b17m, const float* xyz_b3n, const int64_t* index_bm, int64_t B,
                                     int64_t N, int64_t M, float* out_b20m, s4g_stream_t stream) {
  if (B < 0 || N < 0 || M < 0 || B > 65535 || N >= (1ll << 31) || M >= (1ll << 31)) return S4G_EINVAL;
  if (!index_bm && M != N) return S4G_EINVAL;          // without an index, point m is the scene's point m
  if (B == 0 || M == 0) return S4G_OK;
  if (N == 0 || !raw_b17m || !xyz_b3n || !out_b20m) return S4G_EINVAL;
  if (raw_b17m == out_b20m) return S4G_EINVAL;        // not in place: the channel layouts differ
  hipLaunchKernelGGL(s4g::contact_heads_kernel, dim3((unsigned)((M + 255) / 256), (unsigned)B), dim3(256), 0,
                     (hipStream_t)stream, raw_b17m, xyz_b3n, index_bm, (int)M, (int)N, out_b20m);
  S4G_LAUNCH_CHECK();
  return S4G_OK;
}
