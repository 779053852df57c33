// Similarity maps of the pretext model (the reference's MoCoDiffLossTwoFc.cam_visualize, moco/builder_diffspeed_diffloss.py:449-490)
// and the picture panels its visualization.py draws from them (:52-74, :92-111).
//
// rsp_cam_maps: with X = mean over the P positions of an NDHWC feature map F (B, P, C) and the two head weights (dim, C) of each
// encoder, per sample b (kr = k_row[b], the row of feat_k that pairs with b):
//   Ms_qA[b][p] = sum_c ((k_wA @ k_X[kr]) @ q_wA)[c] * q_F[b][p][c]       Ms_qM: the same with k_wM, q_wM
//   Ms_kA[b][p] = sum_c ((q_wA @ q_X[b]) @ k_wA)[c] * k_F[kr][p][c]       Ms_kM: the same with q_wM, k_wM
// No layout change, no atomics, fixed summation order: the same input gives the same bits.
//   cam_mean_kernel     one thread per (side, sample, channel): the P rows summed in row order (four running sums, combined in a
//                       fixed order), coalesced across the channels.  First read of the feature maps.
//   cam_vector_kernel   one workgroup per (sample, map): v = W_other @ X_other (one wave per output, butterfly sum), then
//                       u = v @ W_self (one thread per channel, serial over dim, coalesced rows of W_self).  The weights stay in L2.
//   cam_dot_kernel      one workgroup per (side, sample, 8 rows): the side's two channel vectors in LDS, one wave per (b, p) row,
//                       16-byte loads where the pitch allows, every row dotted with BOTH vectors.  Second and last read.
//
// rsp_cam_overlay: per panel, mean of the map over T', min-max normalisation over (H', W') (max == min: 0), bilinear resize with
// half-pixel centres, the analytic jet colour map on the continuous value, 0.6 * frame + 0.4 * colour, round to nearest, uint8 RGB.
#include "common.h"

#include <math.h>

namespace {

constexpr int CAM_THREADS = 256;
constexpr int CAM_WAVES = CAM_THREADS / 64;
constexpr int CAM_ROWS = 8;                      // (b, p) rows per workgroup of cam_dot_kernel: two per wave
constexpr int CAM_MAX_LDS_FLOATS = 12 * 1024;    // 48 KiB of dynamic LDS per workgroup
constexpr int OV_MAX_HW = 4096;                  // positions of one map held in LDS by the overlay kernel

// grid (ceil(C / 256), B, 2): side 0 = query, 1 = key.  mean: [2][B][C]
__global__ __launch_bounds__(CAM_THREADS) void cam_mean_kernel(const float* __restrict__ feat_q, long long ld_q,
                                                               const float* __restrict__ feat_k, long long ld_k, int P, int C,
                                                               float* __restrict__ mean) {
  const int c = blockIdx.x * CAM_THREADS + threadIdx.x, b = blockIdx.y, side = blockIdx.z, B = gridDim.y;
  if (c >= C) return;
  const long long ld = side ? ld_k : ld_q;
  const float* x = (side ? feat_k : feat_q) + (long long)b * P * ld + c;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int p = 0;
  for (; p + 4 <= P; p += 4) {
    s0 += x[(long long)p * ld];
    s1 += x[(long long)(p + 1) * ld];
    s2 += x[(long long)(p + 2) * ld];
    s3 += x[(long long)(p + 3) * ld];
  }
  for (; p < P; ++p) s0 += x[(long long)p * ld];
  mean[((long long)side * B + b) * C + c] = ((s0 + s1) + (s2 + s3)) / (float)P;
}

// grid (B, 4): map 0 = qA, 1 = qM, 2 = kA, 3 = kM.  u: [4][B][C].  Dynamic LDS: C + dim floats.
__global__ __launch_bounds__(CAM_THREADS) void cam_vector_kernel(const float* __restrict__ mean, const int* __restrict__ k_row,
                                                                 const float* __restrict__ w_qA, const float* __restrict__ w_qM,
                                                                 const float* __restrict__ w_kA, const float* __restrict__ w_kM,
                                                                 int B, int C, int dim_A, int dim_M, float* __restrict__ u) {
  extern __shared__ __attribute__((aligned(16))) float cam_lds[];
  const int b = blockIdx.x, map = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int side = map >> 1, head = map & 1;
  const int dim = head ? dim_M : dim_A;
  const float* w_self = side ? (head ? w_kM : w_kA) : (head ? w_qM : w_qA);
  const float* w_other = side ? (head ? w_qM : w_qA) : (head ? w_kM : w_kA);
  const int kr = k_row[b];
  const bool ok = kr >= 0 && kr < B;       // a bad pairing index poisons this sample's maps instead of reading out of bounds
  // the OTHER side's pooled feature: the key row kr for a query map, the query row b for a key map
  const float* x = mean + ((long long)(side ? 0 : 1) * B + (side ? b : (ok ? kr : 0))) * C;
  float* xs = cam_lds;
  float* v = cam_lds + C;
  for (int c = t; c < C; c += CAM_THREADS) xs[c] = x[c];
  __syncthreads();
  for (int n = wave; n < dim; n += CAM_WAVES) {
    const float* wr = w_other + (long long)n * C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += wr[c] * xs[c];
    s = rsp_wave_sum(s);
    if (lane == 0) v[n] = s;
  }
  __syncthreads();
  float* out = u + ((long long)map * B + b) * C;
  for (int c = t; c < C; c += CAM_THREADS) {
    float s = 0.f;
    for (int n = 0; n < dim; ++n) s += v[n] * w_self[(long long)n * C + c];
    out[c] = ok ? s : NAN;
  }
}

// grid (ceil(P / CAM_ROWS), B, 2).  Dynamic LDS: 2 * C floats (the side's A and M vectors).  out: [4][B][P]
template <bool VEC>
__global__ __launch_bounds__(CAM_THREADS) void cam_dot_kernel(const float* __restrict__ feat_q, long long ld_q,
                                                              const float* __restrict__ feat_k, long long ld_k,
                                                              const int* __restrict__ k_row, const float* __restrict__ u, int P, int C,
                                                              float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float cam_lds[];
  const int b = blockIdx.y, side = blockIdx.z, B = gridDim.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  float* uA = cam_lds;
  float* uM = cam_lds + C;
  const float* gA = u + ((long long)(side * 2) * B + b) * C;
  const float* gM = gA + (long long)B * C;
  for (int c = t; c < C; c += CAM_THREADS) {
    uA[c] = gA[c];
    uM[c] = gM[c];
  }
  __syncthreads();
  int row = b;
  if (side) {
    const int kr = k_row[b];
    row = (kr >= 0 && kr < B) ? kr : 0;      // (the vectors of a bad index are NaN already: so is every dot product)
  }
  const long long ld = side ? ld_k : ld_q;
  const float* base = (side ? feat_k : feat_q) + (long long)row * P * ld;
  const int p0 = blockIdx.x * CAM_ROWS;
  for (int p = p0 + wave; p < p0 + CAM_ROWS && p < P; p += CAM_WAVES) {
    const float* x = base + (long long)p * ld;
    float a = 0.f, m = 0.f;
    if (VEC) {
      const floatx4* x4 = reinterpret_cast<const floatx4*>(x);
      const floatx4* a4 = reinterpret_cast<const floatx4*>(uA);
      const floatx4* m4 = reinterpret_cast<const floatx4*>(uM);
      for (int i = lane; i < (C >> 2); i += 64) {
        const floatx4 f = x4[i], ua = a4[i], um = m4[i];
        a += (f.x * ua.x + f.y * ua.y) + (f.z * ua.z + f.w * ua.w);
        m += (f.x * um.x + f.y * um.y) + (f.z * um.z + f.w * um.w);
      }
    } else {
      for (int c = lane; c < C; c += 64) {
        const float f = x[c];
        a += f * uA[c];
        m += f * uM[c];
      }
    }
    a = rsp_wave_sum(a);
    m = rsp_wave_sum(m);
    if (lane == 0) {
      out[((long long)(side * 2) * B + b) * P + p] = a;
      out[((long long)(side * 2 + 1) * B + b) * P + p] = m;
    }
  }
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// half-pixel centres (align_corners = False): source coordinate of output pixel o, clamped below at 0; i1 clamped at n - 1
__device__ __forceinline__ void bilinear_tap(int o, float scale, int n, int& i0, int& i1, float& w1) {
  float s = scale * ((float)o + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = min((int)s, n - 1);
  i1 = min(i0 + 1, n - 1);
  w1 = s - (float)i0;
}

// grid (ceil(size * size / 256 / 4), N).  maps: [N][Tp][Hp][Wp]; panel n shows sample n % B of clip_a (n < N / 2 or no clip_b) or
// clip_b, frame t of a (B, 3, T, size, size) clip in [0, 1]; out: [N][size][size][3]
__global__ __launch_bounds__(CAM_THREADS) void cam_overlay_kernel(const float* __restrict__ maps, int N, int Tp, int Hp, int Wp,
                                                                  const float* __restrict__ clip_a, const float* __restrict__ clip_b,
                                                                  int B, int T, int t_frame, int size, uint8_t* __restrict__ out) {
  __shared__ float mp[OV_MAX_HW];
  __shared__ float red[2][CAM_WAVES];
  const int n = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int HW = Hp * Wp;
  const float* m = maps + (long long)n * Tp * HW;
  float lo = INFINITY, hi = -INFINITY;
  for (int i = t; i < HW; i += CAM_THREADS) {
    float s = 0.f;
    for (int j = 0; j < Tp; ++j) s += m[(long long)j * HW + i];      // frame order
    s = Tp == 1 ? s : s / (float)Tp;
    mp[i] = s;
    lo = fminf(lo, s);
    hi = fmaxf(hi, s);
  }
  lo = -rsp_wave_max(-lo);
  hi = rsp_wave_max(hi);
  if (lane == 0) {
    red[0][wave] = lo;
    red[1][wave] = hi;
  }
  __syncthreads();
  lo = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
  hi = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
  const float range = hi - lo;
  const bool flat = !(range > 0.f);
  const float sy = (float)Hp / (float)size, sx = (float)Wp / (float)size;
  const float* clip = (clip_b != nullptr && n >= N / 2) ? clip_b : clip_a;
  const long long plane = (long long)size * size;
  const float* frame = clip + ((long long)(n % B) * 3 * T + t_frame) * plane;
  const long long chan = (long long)T * plane;
  uint8_t* o = out + (long long)n * plane * 3;
  const int total = size * size;
  for (int px = blockIdx.x * CAM_THREADS + t; px < total; px += gridDim.x * CAM_THREADS) {
    const int y = px / size, x = px - y * size;
    int y0, y1, x0, x1;
    float wy, wx;
    bilinear_tap(y, sy, Hp, y0, y1, wy);
    bilinear_tap(x, sx, Wp, x0, x1, wx);
    float v = 0.f;
    if (!flat) {
      const float v00 = (mp[y0 * Wp + x0] - lo) / range, v01 = (mp[y0 * Wp + x1] - lo) / range;
      const float v10 = (mp[y1 * Wp + x0] - lo) / range, v11 = (mp[y1 * Wp + x1] - lo) / range;
      v = (1.f - wy) * ((1.f - wx) * v00 + wx * v01) + wy * ((1.f - wx) * v10 + wx * v11);
    }
    const float col[3] = {clamp01(1.5f - fabsf(4.f * v - 3.f)), clamp01(1.5f - fabsf(4.f * v - 2.f)),
                          clamp01(1.5f - fabsf(4.f * v - 1.f))};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float f = frame[c * chan + px] * 255.f;
      const float r = rintf(0.6f * f + 0.4f * (col[c] * 255.f));
      o[(long long)px * 3 + c] = (uint8_t)fminf(fmaxf(r, 0.f), 255.f);
    }
  }
}

}  // namespace

size_t rsp_cam_maps_workspace(int32_t B, int32_t C) {
  if (B <= 0 || C <= 0) return 0;
  return (size_t)6 * (size_t)B * (size_t)C * sizeof(float);      // [2][B][C] pooled means + [4][B][C] channel vectors
}

int rsp_cam_maps(const float* feat_q, int32_t ld_q, const float* feat_k, int32_t ld_k, const int32_t* k_row, int32_t B, int32_t P,
                 int32_t C, const float* w_qA, const float* w_qM, const float* w_kA, const float* w_kM, int32_t dim_A, int32_t dim_M,
                 float* out, void* workspace, size_t workspace_bytes, void* stream) {
  RSP_REQUIRE(feat_q && feat_k && k_row && w_qA && w_qM && w_kA && w_kM && out && workspace, "rsp_cam_maps: null pointer");
  RSP_REQUIRE(B >= 1 && B <= 65535 && P >= 1 && C >= 1 && dim_A >= 1 && dim_M >= 1 && ld_q >= C && ld_k >= C,
              "rsp_cam_maps: bad size (1 <= B <= 65535, P, C, dim >= 1, ld >= C)");
  RSP_REQUIRE((long long)C + (dim_A > dim_M ? dim_A : dim_M) <= CAM_MAX_LDS_FLOATS && 2ll * C <= CAM_MAX_LDS_FLOATS,
              "rsp_cam_maps: C + dim and 2 * C must fit 12288 floats of LDS");
  RSP_REQUIRE((long long)rsp_cdiv(P, CAM_ROWS) <= 0x7fffffffll, "rsp_cam_maps: P too large");
  if (workspace_bytes < rsp_cam_maps_workspace(B, C)) {
    rsp_set_error("rsp_cam_maps: workspace too small");
    return RSP_EWORKSPACE;
  }
  float* mean = reinterpret_cast<float*>(workspace);
  float* u = mean + (size_t)2 * B * C;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cam_mean_kernel, dim3(rsp_cdiv(C, CAM_THREADS), B, 2), dim3(CAM_THREADS), 0, s, feat_q, (long long)ld_q, feat_k,
                     (long long)ld_k, P, C, mean);
  int rc = rsp_check_launch("cam_mean_kernel");
  if (rc != RSP_OK) return rc;
  const int dim = dim_A > dim_M ? dim_A : dim_M;
  hipLaunchKernelGGL(cam_vector_kernel, dim3(B, 4), dim3(CAM_THREADS), (size_t)(C + dim) * sizeof(float), s, mean, k_row, w_qA, w_qM,
                     w_kA, w_kM, B, C, dim_A, dim_M, u);
  rc = rsp_check_launch("cam_vector_kernel");
  if (rc != RSP_OK) return rc;
  // 16-byte loads need whole float4s per row and rows that start on a 16-byte boundary (the workspace is carved in C-float steps)
  const bool vec = (C % 4 == 0) && (ld_q % 4 == 0) && (ld_k % 4 == 0) && rsp_aligned16(feat_q) && rsp_aligned16(feat_k) &&
                   rsp_aligned16(workspace);
  const dim3 grid(rsp_cdiv(P, CAM_ROWS), B, 2);
  const size_t lds = (size_t)2 * C * sizeof(float);
  if (vec)
    hipLaunchKernelGGL(cam_dot_kernel<true>, grid, dim3(CAM_THREADS), lds, s, feat_q, (long long)ld_q, feat_k, (long long)ld_k, k_row, u,
                       P, C, out);
  else
    hipLaunchKernelGGL(cam_dot_kernel<false>, grid, dim3(CAM_THREADS), lds, s, feat_q, (long long)ld_q, feat_k, (long long)ld_k, k_row,
                       u, P, C, out);
  return rsp_check_launch("cam_dot_kernel");
}

int rsp_cam_overlay(const float* maps, int32_t N, int32_t Tp, int32_t Hp, int32_t Wp, const float* clip_a, const float* clip_b,
                    int32_t B, int32_t T, int32_t t, int32_t size, uint8_t* out, void* stream) {
  RSP_REQUIRE(maps && clip_a && out, "rsp_cam_overlay: null pointer");
  RSP_REQUIRE(N >= 1 && N <= 65535 && Tp >= 1 && Hp >= 1 && Wp >= 1 && (long long)Hp * Wp <= OV_MAX_HW,
              "rsp_cam_overlay: bad map size (1 <= N <= 65535, H' * W' <= 4096)");
  RSP_REQUIRE(B >= 1 && T >= 1 && t >= 0 && t < T && size >= 1 && size <= 4096,
              "rsp_cam_overlay: bad clip size (0 <= t < T, 1 <= size <= 4096)");
  RSP_REQUIRE(clip_b ? (N == 2 * (N / 2) && (N / 2) % B == 0) : N % B == 0,
              "rsp_cam_overlay: the panels of each clip must be a multiple of its B samples");
  const int blocks = rsp_cdiv(rsp_cdiv((long long)size * size, CAM_THREADS), 4);
  hipLaunchKernelGGL(cam_overlay_kernel, dim3(blocks, N), dim3(CAM_THREADS), 0, (hipStream_t)stream, maps, N, Tp, Hp, Wp, clip_a, clip_b,
                     B, T, t, size, out);
  return rsp_check_launch("cam_overlay_kernel");
}
