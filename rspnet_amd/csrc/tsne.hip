// Embedding maps (rsp_tsne_affinities, rsp_tsne_fit): exact t-SNE of N stored feature rows.  The affinities are one call; every
// iteration of the descent is issued from one call, three launches each, nothing read back, nothing atomic.
// include/rspnet_hip.h states the rule; rspnet_amd/tsne.py restates it in numpy fp64 (tsne_reference).
//
// Kernels of the affinities:
//   inv_norm_kernel     the search's (rsp_inv_norms, cos_search.h): inv = 1 / sqrtf(ss) for a valid row (ss finite and > 0), 0 otherwise.
//   ts_compact_kernel   one block: the valid rows in ascending order as a list (rsp_compact_rows, cos_search.h), -1 behind
//                       it; invc[rank] = the inverse norm of the listed row; M, rows_valid and rows_bad.  Every later kernel walks the
//                       list by rank, so the result is, to the bit, the result on x without the invalid rows.
//   ts_dist_kernel      repr_pair_kernel's GEMM tile (64 x 128 ranks, 32-wide k chunks through double-buffered LDS, register prefetch,
//                       v_mfma_f32_32x32x2_f32, the same accumulator mapping) with the rows gathered through the list.  The dot product
//                       is symmetric by itself (the same k order on both sides of the diagonal); the two inverse norms are applied
//                       lower rank first, so d is symmetric to the bit.  Elements outside M x M (inside N x N) are written as 0.
//   ts_calib_kernel     one wave per rank: 64 bisection steps + one pass at the final beta, each a pass over its row of d (lane l: columns
//                       l, l + 64, ... in order, then the xor butterfly).  Leaves beta, the row minimum and S.
//   ts_joint_kernel     one block per rank i: p_ij from d_ij (= d_ji to the bit, so no transposed read is needed) and the two rows'
//                       (beta, min, S); the row's fp64 sums of p and p log p (thread t: columns t, t + 256, ...; the wave butterfly, the
//                       four waves in order).  Elements outside M x M are written as 0.
//   ts_info_kernel      one block: the row sums in a fixed order in fp64 into info.
// Kernels of one iteration of the fit:
//   ts_pair_kernel      block = 64 ranks i x one split of the ranks j.  A 64 x 64 tile of p and the 64 y_j go through LDS; thread
//                       (wave w, lane r) takes rank i0 + r and the tile's columns 16 w .. 16 w + 15 in order: w = 1 / (1 + r2), the four
//                       force sums, z and e in fp32.  The four waves are added in wave order; partials per split in the workspace.
//   ts_reduce_kernel    one thread per rank: the splits in split order (fp32); z and e of a block of 256 ranks in fp64 (butterfly, then
//                       the four waves in order).
//   ts_update_kernel    one thread per rank: Z and E from the block partials (lane l: blocks l, l + 64, ...; the butterfly) in fp64,
//                       the gradient and van der Maaten's update through the row list; kl_trace[t].
#include "cos_search.h"

namespace {

constexpr int TS_BQ = 64;              // ranks i per distance tile
constexpr int TS_BG = 128;             // ranks j per distance tile
constexpr int TS_KC = 32;              // k per LDS chunk
constexpr int TS_LD = TS_KC + 4;       // LDS row pitch (floats) of a chunk: the float4 reads along k stay conflict-free
constexpr int TS_BUF = (TS_BQ + TS_BG) * TS_LD;
constexpr size_t TS_LDS_BYTES = (size_t)2 * TS_BUF * sizeof(float);      // 55 296: two workgroups per CU

constexpr int TP_R = 64;               // ranks i per pair tile, ranks j per staged chunk
constexpr int TP_LD = TP_R + 1;        // LDS pitch of the staged p tile: lane r reads row r, conflict-free
constexpr int TP_TARGET_BLOCKS = 1024; // four workgroups per CU on 256 CUs
constexpr int TS_ROWS = 256;           // ranks per block of the reduce / update kernels
constexpr int TS_STEPS = 64;           // bisection steps of the calibration
constexpr int TS_PART = 8;             // floats per (split, rank) partial: attr x, y, rep x, y, z, e, two pad words

struct TsState {      // at the head of the affinities' workspace
  int m, pad;
};

// The number of column splits of the pair kernel for m listed rows: about TP_TARGET_BLOCKS blocks, a split at least one 64-column chunk.
// From m alone, so that the order of the sums does not depend on the invalid rows.
__host__ __device__ __forceinline__ int ts_splits(int m) {
  const int c = m > TP_R ? (m + TP_R - 1) / TP_R : 1;
  const int s = min(c, (TP_TARGET_BLOCKS + c - 1) / c);
  return s < 1 ? 1 : s;
}

__global__ __launch_bounds__(256) void ts_compact_kernel(const float* __restrict__ inv, int N, int* __restrict__ rows,
                                                         float* __restrict__ invc, TsState* __restrict__ st,
                                                         rsp_tsne_info* __restrict__ info) {
  const int t = threadIdx.x;
  const int base = rsp_compact_rows(0, N, [&](int i) { return inv[i] > 0.f; }, [&](int r, int i) {
    rows[r] = i;
    invc[r] = inv[i];
  });
  for (int r = base + t; r < N; r += 256) rows[r] = -1;
  if (t == 0) {
    st->m = base;
    st->pad = 0;
    info->rows_valid = base;
    info->rows_bad = N - base;
  }
}

__global__ __launch_bounds__(256) void ts_dist_kernel(const float* __restrict__ x, int ld, int N, int D, const int* __restrict__ rows,
                                                      const float* __restrict__ invc, const TsState* __restrict__ st,
                                                      float* __restrict__ dmat, int ldd) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l32 = lane & 31, h = lane >> 5;
  const int wq = wave >> 1, wg = wave & 1;
  const int M = st->m;
  const int i0 = blockIdx.x * TS_BQ, j0 = blockIdx.y * TS_BG;
  const int nch = (D + TS_KC - 1) / TS_KC;
  const bool outside = i0 >= M || j0 >= M;      // (the whole block: no barrier is reached)

  floatx16 acc0, acc1;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    acc0[e] = 0.f;
    acc1[e] = 0.f;
  }
  if (!outside) {
    int gq[4], gg[8];      // the rows of x this thread stages; -1: rank not listed
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int r = i0 + ((t + 256 * it) >> 4);
      gq[it] = r < M ? rows[r] : -1;
    }
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int r = j0 + ((t + 256 * it) >> 4);
      gg[it] = r < M ? rows[r] : -1;
    }
    float2 rq[4], rg[8];
    auto load = [&](int kc) {
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int k2 = kc + 2 * ((t + 256 * it) & 15);
        rq[it] = (gq[it] >= 0 && k2 < D) ? *reinterpret_cast<const float2*>(x + (long long)gq[it] * ld + k2) : make_float2(0.f, 0.f);
      }
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int k2 = kc + 2 * ((t + 256 * it) & 15);
        rg[it] = (gg[it] >= 0 && k2 < D) ? *reinterpret_cast<const float2*>(x + (long long)gg[it] * ld + k2) : make_float2(0.f, 0.f);
      }
    };
    auto store = [&](float* buf) {
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int e = t + 256 * it;
        *reinterpret_cast<float2*>(buf + (e >> 4) * TS_LD + 2 * (e & 15)) = rq[it];
      }
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int e = t + 256 * it;
        *reinterpret_cast<float2*>(buf + (TS_BQ + (e >> 4)) * TS_LD + 2 * (e & 15)) = rg[it];
      }
    };
    load(0);
    store(sm);
    __syncthreads();
    for (int ch = 0; ch < nch; ++ch) {
      const float* buf = sm + (ch & 1) * TS_BUF;
      if (ch + 1 < nch) load((ch + 1) * TS_KC);
      const float* qa = buf + (32 * wq + l32) * TS_LD + 4 * h;
      const float* gb0 = buf + (TS_BQ + 64 * wg + l32) * TS_LD + 4 * h;
      const float* gb1 = gb0 + 32 * TS_LD;
      // lane half h takes k = 8m + 4h + j at step j of group m, for A and B alike: every k of the chunk once, in ascending order
#pragma unroll
      for (int m = 0; m < TS_KC / 8; ++m) {
        const float4 a = *reinterpret_cast<const float4*>(qa + 8 * m);
        const float4 b0 = *reinterpret_cast<const float4*>(gb0 + 8 * m);
        const float4 b1 = *reinterpret_cast<const float4*>(gb1 + 8 * m);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0.x, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b1.x, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b0.y, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1.y, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b0.z, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b1.z, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b0.w, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b1.w, acc1, 0, 0, 0);
      }
      if (ch + 1 < nch) store(sm + ((ch + 1) & 1) * TS_BUF);
      __syncthreads();
    }
  }

  const int jc0 = j0 + 64 * wg + l32, jc1 = jc0 + 32;
  const float ig0 = jc0 < M ? invc[jc0] : 0.f;
  const float ig1 = jc1 < M ? invc[jc1] : 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int i = i0 + 32 * wq + (e >> 2) * 8 + h * 4 + (e & 3);
    if (i >= N) continue;
    const float iq = i < M ? invc[i] : 0.f;
    float* out = dmat + (long long)i * ldd;
    if (jc0 < N) {
      // the lower rank's inverse norm first: the search's expression above the diagonal, its mirror image below
      const float s = i < jc0 ? acc0[e] * iq * ig0 : acc0[e] * ig0 * iq;
      out[jc0] = (i < M && jc0 < M && i != jc0) ? fmaxf(2.f - 2.f * s, 0.f) : 0.f;
    }
    if (jc1 < N) {
      const float s = i < jc1 ? acc1[e] * iq * ig1 : acc1[e] * ig1 * iq;
      out[jc1] = (i < M && jc1 < M && i != jc1) ? fmaxf(2.f - 2.f * s, 0.f) : 0.f;
    }
  }
}

__global__ __launch_bounds__(256) void ts_calib_kernel(const float* __restrict__ dmat, int ldd, const TsState* __restrict__ st,
                                                       float logp, int N, float* __restrict__ beta, float* __restrict__ rmin,
                                                       float* __restrict__ rsum) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int M = st->m;
  if (i >= N) return;
  if (i >= M) {      // (the whole wave) not a rank: beta says so
    if (lane == 0) {
      beta[i] = NAN;
      rmin[i] = 0.f;
      rsum[i] = 1.f;
    }
    return;
  }
  const float* d = dmat + (long long)i * ldd;
  float mn = INFINITY;
  for (int j = lane; j < M; j += 64)
    if (j != i) mn = fminf(mn, d[j]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o));
  float b = 1.f, lo = 0.f, hi = INFINITY, S = 0.f;
  for (int step = 0; step <= TS_STEPS; ++step) {      // the last pass: S at the final beta
    float s = 0.f, a = 0.f;
    for (int j = lane; j < M; j += 64) {
      if (j != i) {
        const float dd = d[j] - mn;
        const float e = expf(-b * dd);
        s += e;
        a = fmaf(e, dd, a);
      }
    }
    s = rsp_wave_sum(s);
    a = rsp_wave_sum(a);
    S = s;
    if (step == TS_STEPS) break;
    const float H = logf(s) + b * a / s;
    if (H > logp) {
      lo = b;
      b = hi == INFINITY ? 2.f * b : (lo + hi) * 0.5f;
    } else {
      hi = b;
      b = (lo + hi) * 0.5f;
    }
  }
  if (lane == 0) {
    beta[i] = b;
    rmin[i] = mn;
    rsum[i] = S;
  }
}

__global__ __launch_bounds__(256) void ts_joint_kernel(const float* __restrict__ dmat, int ldd, const TsState* __restrict__ st, int N,
                                                       const float* __restrict__ beta, const float* __restrict__ rmin,
                                                       const float* __restrict__ rsum, float* __restrict__ pmat, int ldp,
                                                       double* __restrict__ rowpart) {
  __shared__ double red[4][2];
  const int i = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int M = st->m;
  float* out = pmat + (long long)i * ldp;
  double sp = 0.0, sl = 0.0;
  if (i >= M) {      // (the whole block)
    for (int j = t; j < N; j += 256) out[j] = 0.f;
  } else {
    const float* d = dmat + (long long)i * ldd;
    const float bi = beta[i], mi = rmin[i], si = rsum[i];
    const float scale = 1.f / (2.f * (float)M);
    for (int j = t; j < N; j += 256) {
      float p = 0.f;
      if (j < M && j != i) {
        const float dij = d[j];
        const float cij = expf(-bi * (dij - mi)) / si;
        const float cji = expf(-beta[j] * (dij - rmin[j])) / rsum[j];
        const float lo = i < j ? cij : cji, hi = i < j ? cji : cij;      // (a + b commutes; the order is fixed all the same)
        p = (lo + hi) * scale;
      }
      out[j] = p;
      sp += (double)p;
      if (p > 0.f) sl += (double)(p * logf(p));
    }
  }
  sp = rsp_wave_sum_d(sp);
  sl = rsp_wave_sum_d(sl);
  if (lane == 0) {
    red[wave][0] = sp;
    red[wave][1] = sl;
  }
  __syncthreads();
  if (t < 2) rowpart[2 * (long long)i + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

__global__ __launch_bounds__(1024) void ts_info_kernel(const double* __restrict__ rowpart, int N, rsp_tsne_info* __restrict__ info) {
  __shared__ double red[16][2];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  double sp = 0.0, sl = 0.0;
  for (int i = t; i < N; i += 1024) {
    sp += rowpart[2 * (long long)i];
    sl += rowpart[2 * (long long)i + 1];
  }
  sp = rsp_wave_sum_d(sp);
  sl = rsp_wave_sum_d(sl);
  if (lane == 0) {
    red[wave][0] = sp;
    red[wave][1] = sl;
  }
  __syncthreads();
  if (t == 0) {
    double a = 0.0, b = 0.0;
    for (int w = 0; w < 16; ++w) {
      a += red[w][0];
      b += red[w][1];
    }
    info->psum = a;
    info->plogp = b;
  }
}

// ---- the fit ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ts_pair_kernel(const float* __restrict__ pmat, int ldp, const int* __restrict__ rows,
                                                      const rsp_tsne_info* __restrict__ info, const float* __restrict__ y,
                                                      float* __restrict__ part, int N) {
  __shared__ float sp[TP_R * TP_LD];
  __shared__ float2 sy[TP_R];
  __shared__ float red[3][TP_R][6];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int M = (int)info->rows_valid;
  const int i0 = blockIdx.x * TP_R;
  const int splits = ts_splits(M), split = blockIdx.y;
  if (i0 >= M || split >= splits) return;      // (the whole block: the launch is sized by N)
  const int chunks = (M + TP_R - 1) / TP_R;
  const int c_lo = (int)((long long)split * chunks / splits), c_hi = (int)((long long)(split + 1) * chunks / splits);
  const int i = i0 + lane;
  const bool mine = i < M;
  float2 yi = make_float2(0.f, 0.f);
  if (mine) yi = *reinterpret_cast<const float2*>(y + 2 * (long long)rows[i]);
  float ax = 0.f, ay = 0.f, rx = 0.f, ry = 0.f, z = 0.f, e = 0.f;

  for (int ch = c_lo; ch < c_hi; ++ch) {
    const int j0 = ch * TP_R;
    // the 64 x 64 tile of p: thread t loads column t & 63 of rows t >> 6, + 4, ... (a wave: 256 consecutive bytes of one row)
#pragma unroll 4
    for (int r = wave; r < TP_R; r += 4) {
      const int ii = i0 + r, jj = j0 + lane;
      sp[r * TP_LD + lane] = (ii < M && jj < M) ? pmat[(long long)ii * ldp + jj] : 0.f;
    }
    if (t < TP_R) {
      const int jj = j0 + t;
      sy[t] = jj < M ? *reinterpret_cast<const float2*>(y + 2 * (long long)rows[jj]) : make_float2(0.f, 0.f);
    }
    __syncthreads();
    if (mine) {
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        const int cc = 16 * wave + c, j = j0 + cc;
        if (j < M && j != i) {
          const float2 yj = sy[cc];
          const float dx = yi.x - yj.x, dy = yi.y - yj.y;
          const float r2 = dx * dx + dy * dy;
          const float w = 1.f / (1.f + r2);
          const float p = sp[lane * TP_LD + cc];
          const float pw = p * w, ww = w * w;
          ax += pw * dx;
          ay += pw * dy;
          rx += ww * dx;
          ry += ww * dy;
          z += w;
          e += p * log1pf(r2);
        }
      }
    }
    __syncthreads();
  }
  if (wave > 0) {
    float* r = red[wave - 1][lane];
    r[0] = ax;
    r[1] = ay;
    r[2] = rx;
    r[3] = ry;
    r[4] = z;
    r[5] = e;
  }
  __syncthreads();
  if (wave == 0 && mine) {
    float v[6] = {ax, ay, rx, ry, z, e};
#pragma unroll
    for (int w = 0; w < 3; ++w)
#pragma unroll
      for (int q = 0; q < 6; ++q) v[q] += red[w][lane][q];
    float2* out = reinterpret_cast<float2*>(part + ((long long)split * N + i) * TS_PART);      // (the workspace promises 8 bytes)
    out[0] = make_float2(v[0], v[1]);
    out[1] = make_float2(v[2], v[3]);
    out[2] = make_float2(v[4], v[5]);
  }
}

__global__ __launch_bounds__(256) void ts_reduce_kernel(const float* __restrict__ part, const rsp_tsne_info* __restrict__ info, int N,
                                                        float* __restrict__ rowsum, double* __restrict__ bpart) {
  __shared__ double red[4][2];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int M = (int)info->rows_valid;
  if (blockIdx.x * TS_ROWS >= M) return;      // (the whole block)
  const int i = blockIdx.x * TS_ROWS + t, splits = ts_splits(M);
  double dz = 0.0, de = 0.0;
  if (i < M) {
    float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < splits; ++s) {
      const float2* in = reinterpret_cast<const float2*>(part + ((long long)s * N + i) * TS_PART);
      const float2 a = in[0], b = in[1], c = in[2];
      v[0] += a.x;
      v[1] += a.y;
      v[2] += b.x;
      v[3] += b.y;
      v[4] += c.x;
      v[5] += c.y;
    }
    float2* rs = reinterpret_cast<float2*>(rowsum + 4 * (long long)i);
    rs[0] = make_float2(v[0], v[1]);
    rs[1] = make_float2(v[2], v[3]);
    dz = (double)v[4];
    de = (double)v[5];
  }
  dz = rsp_wave_sum_d(dz);
  de = rsp_wave_sum_d(de);
  if (lane == 0) {
    red[wave][0] = dz;
    red[wave][1] = de;
  }
  __syncthreads();
  if (t < 2) bpart[2 * blockIdx.x + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

__global__ __launch_bounds__(256) void ts_update_kernel(const float* __restrict__ rowsum, const double* __restrict__ bpart,
                                                        const int* __restrict__ rows, const rsp_tsne_info* __restrict__ info,
                                                        const float2* __restrict__ sched, int it, int t_out, float* __restrict__ y,
                                                        float* __restrict__ inc, float* __restrict__ gains,
                                                        double* __restrict__ kl_trace) {
  const int t = threadIdx.x, lane = t & 63;
  const int M = (int)info->rows_valid;
  if (blockIdx.x * TS_ROWS >= M && blockIdx.x > 0) return;
  const int nb = (M + TS_ROWS - 1) / TS_ROWS;
  double Z = 0.0, E = 0.0;
  for (int b = lane; b < nb; b += 64) {
    Z += bpart[2 * b];
    E += bpart[2 * b + 1];
  }
  Z = rsp_wave_sum_d(Z);
  E = rsp_wave_sum_d(E);
  if (blockIdx.x == 0 && t == 0) kl_trace[t_out] = info->plogp + E + log(Z);
  const int i = blockIdx.x * TS_ROWS + t;
  if (i >= M) return;
  const float2 s0 = sched[2 * (long long)it], s1 = sched[2 * (long long)it + 1];      // lr, momentum | exaggeration, pad
  const float lr = s0.x, mom = s0.y, exag = s1.x;
  const float Zf = (float)Z;
  const float2* rs = reinterpret_cast<const float2*>(rowsum + 4 * (long long)i);
  const float2 fa = rs[0], fr = rs[1];
  const float g[2] = {4.f * (exag * fa.x - fr.x / Zf), 4.f * (exag * fa.y - fr.y / Zf)};
  const long long o = 2 * (long long)rows[i];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const float v = inc[o + c];
    float gn = gains[o + c];
    gn = ((g[c] > 0.f) != (v > 0.f)) ? gn + 0.2f : gn * 0.8f;
    gn = gn < 0.01f ? 0.01f : gn;      // (a NaN gain stays NaN)
    const float nv = mom * v - lr * gn * g[c];
    gains[o + c] = gn;
    inc[o + c] = nv;
    y[o + c] += nv;
  }
}

// ---- host: the carve-up of the workspaces -------------------------------------------------------------------------------------
struct AffPlan {
  size_t off_inv, off_invc, off_min, off_sum, off_rowpart, off_dmat, bytes;
};

AffPlan aff_plan(int N) {
  AffPlan p;
  const size_t v = rsp_align_up((size_t)N * sizeof(float), 256);
  p.off_inv = 256;
  p.off_invc = p.off_inv + v;
  p.off_min = p.off_invc + v;
  p.off_sum = p.off_min + v;
  p.off_rowpart = p.off_sum + v;
  p.off_dmat = p.off_rowpart + rsp_align_up((size_t)N * 2 * sizeof(double), 256);
  p.bytes = p.off_dmat + rsp_align_up((size_t)N * N * sizeof(float), 256);      // (used only without dmat; the query has no such argument)
  return p;
}

struct FitPlan {
  int max_splits;
  size_t off_rowsum, off_bpart, bytes;
};

FitPlan fit_plan(int N) {
  FitPlan p;
  p.max_splits = 1;
  for (int c = 1; c <= rsp_cdiv(N, TP_R); ++c) {      // ts_splits is not monotone in m: the launch and the partials take its maximum
    const int s = ts_splits(c * TP_R);
    if (s > p.max_splits) p.max_splits = s;
  }
  p.off_rowsum = rsp_align_up((size_t)p.max_splits * N * TS_PART * sizeof(float), 256);
  p.off_bpart = p.off_rowsum + rsp_align_up((size_t)N * 4 * sizeof(float), 256);
  p.bytes = p.off_bpart + rsp_align_up((size_t)rsp_cdiv(N, TS_ROWS) * 2 * sizeof(double), 256);
  return p;
}

bool n_ok(int N) { return N >= 2 && N <= 16384; }

int fail(const char* who, const char* what, int code) {
  char buf[200];
  snprintf(buf, sizeof buf, "%s: %s", who, what);
  rsp_set_error(buf);
  return code;
}

bool aligned(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

}  // namespace

size_t rsp_tsne_affinities_workspace(int32_t N, int32_t D) {
  return (n_ok(N) && D >= 2 && D <= 4096 && D % 2 == 0) ? aff_plan(N).bytes : 0;
}

int rsp_tsne_affinities(const float* x, int32_t ld, int32_t N, int32_t D, float perplexity, float* pmat, int32_t ldp, int32_t* rows,
                        float* beta, float* dmat, rsp_tsne_info* info, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "rsp_tsne_affinities";
  if (!x || !pmat || !rows || !beta || !info || !workspace) return fail(who, "null pointer", RSP_EINVAL);
  if (!(n_ok(N) && D >= 2 && D <= 4096 && D % 2 == 0 && ld >= D && ld % 2 == 0 && ldp >= N))
    return fail(who, "bad size (2 <= N <= 16384, 2 <= D <= 4096, D and ld even, ld >= D, ldp >= N)", RSP_EINVAL);
  if (!(isfinite(perplexity) && perplexity >= 1.f && perplexity <= 1024.f))
    return fail(who, "perplexity must be finite and in [1, 1024]", RSP_EINVAL);
  if (!aligned(x, 8) || !aligned(info, 8) || !aligned(workspace, 8))
    return fail(who, "x, info and the workspace must be 8-byte aligned", RSP_EINVAL);
  if (!aligned(pmat, 4) || !aligned(rows, 4) || !aligned(beta, 4) || !aligned(dmat, 4))
    return fail(who, "pmat, rows, beta and dmat must be 4-byte aligned", RSP_EINVAL);
  const AffPlan p = aff_plan(N);
  if (workspace_bytes < p.bytes) return fail(who, "workspace too small", RSP_EWORKSPACE);
  hipStream_t s = (hipStream_t)stream;
  char* ws = reinterpret_cast<char*>(workspace);
  TsState* st = reinterpret_cast<TsState*>(ws);
  float* inv = reinterpret_cast<float*>(ws + p.off_inv);
  float* invc = reinterpret_cast<float*>(ws + p.off_invc);
  float* rmin = reinterpret_cast<float*>(ws + p.off_min);
  float* rsum = reinterpret_cast<float*>(ws + p.off_sum);
  double* rowpart = reinterpret_cast<double*>(ws + p.off_rowpart);
  float* d = dmat ? dmat : reinterpret_cast<float*>(ws + p.off_dmat);
  const int ldd = dmat ? ldp : N;      // (dmat, when given, has pmat's pitch)

  int rc = rsp_inv_norms(x, ld, N, D, inv, nullptr, s);
  if (rc != RSP_OK) return rc;
  hipLaunchKernelGGL(ts_compact_kernel, dim3(1), dim3(256), 0, s, (const float*)inv, (int)N, (int*)rows, invc, st, info);
  rc = rsp_check_launch("ts_compact_kernel");
  if (rc != RSP_OK) return rc;
  rc = rsp_launch_lds<ts_dist_kernel>(dim3(rsp_cdiv(N, TS_BQ), rsp_cdiv(N, TS_BG)), TS_LDS_BYTES, TS_LDS_BYTES, s,
                                      std::make_tuple(x, (int)ld, (int)N, (int)D, (const int*)rows, (const float*)invc,
                                                      (const TsState*)st, d, ldd),
                                      "ts_dist_kernel");
  if (rc != RSP_OK) return rc;
  hipLaunchKernelGGL(ts_calib_kernel, dim3(rsp_cdiv(N, 4)), dim3(256), 0, s, (const float*)d, ldd, (const TsState*)st, logf(perplexity),
                     (int)N, beta, rmin, rsum);
  rc = rsp_check_launch("ts_calib_kernel");
  if (rc != RSP_OK) return rc;
  hipLaunchKernelGGL(ts_joint_kernel, dim3(N), dim3(256), 0, s, (const float*)d, ldd, (const TsState*)st, (int)N, (const float*)beta,
                     (const float*)rmin, (const float*)rsum, pmat, (int)ldp, rowpart);
  rc = rsp_check_launch("ts_joint_kernel");
  if (rc != RSP_OK) return rc;
  hipLaunchKernelGGL(ts_info_kernel, dim3(1), dim3(1024), 0, s, (const double*)rowpart, (int)N, info);
  return rsp_check_launch("ts_info_kernel");
}

size_t rsp_tsne_fit_workspace(int32_t N) { return n_ok(N) ? fit_plan(N).bytes : 0; }

int rsp_tsne_fit(const float* pmat, int32_t ldp, const int32_t* rows, const rsp_tsne_info* info, int32_t N, const float* sched_dev,
                 int32_t first_iter, int32_t iters, float* y, float* inc, float* gains, double* kl_trace, void* workspace,
                 size_t workspace_bytes, void* stream) {
  const char* who = "rsp_tsne_fit";
  if (!pmat || !rows || !info || !sched_dev || !y || !inc || !gains || !kl_trace || !workspace) return fail(who, "null pointer", RSP_EINVAL);
  if (!(n_ok(N) && ldp >= N)) return fail(who, "bad size (2 <= N <= 16384, ldp >= N)", RSP_EINVAL);
  if (!(iters >= 1 && iters <= 10000)) return fail(who, "iters must be in [1, 10000]", RSP_EINVAL);
  if (first_iter < 0) return fail(who, "first_iter must not be negative", RSP_EINVAL);
  if (!aligned(y, 8) || !aligned(inc, 8) || !aligned(gains, 8) || !aligned(kl_trace, 8) || !aligned(info, 8) || !aligned(workspace, 8) ||
      !aligned(sched_dev, 8))
    return fail(who, "y, inc, gains, kl_trace, info, sched and the workspace must be 8-byte aligned", RSP_EINVAL);
  if (!aligned(pmat, 4) || !aligned(rows, 4)) return fail(who, "pmat and rows must be 4-byte aligned", RSP_EINVAL);
  const FitPlan p = fit_plan(N);
  if (workspace_bytes < p.bytes) return fail(who, "workspace too small", RSP_EWORKSPACE);
  hipStream_t s = (hipStream_t)stream;
  char* ws = reinterpret_cast<char*>(workspace);
  float* part = reinterpret_cast<float*>(ws);
  float* rowsum = reinterpret_cast<float*>(ws + p.off_rowsum);
  double* bpart = reinterpret_cast<double*>(ws + p.off_bpart);
  const float2* sched = reinterpret_cast<const float2*>(sched_dev);
  const int nb = rsp_cdiv(N, TS_ROWS);

  for (int t = 0; t < iters; ++t) {
    hipLaunchKernelGGL(ts_pair_kernel, dim3(rsp_cdiv(N, TP_R), p.max_splits), dim3(256), 0, s, pmat, (int)ldp, (const int*)rows, info,
                       (const float*)y, part, (int)N);
    int rc = rsp_check_launch("ts_pair_kernel");
    if (rc != RSP_OK) return rc;
    hipLaunchKernelGGL(ts_reduce_kernel, dim3(nb), dim3(256), 0, s, (const float*)part, info, (int)N, rowsum, bpart);
    rc = rsp_check_launch("ts_reduce_kernel");
    if (rc != RSP_OK) return rc;
    hipLaunchKernelGGL(ts_update_kernel, dim3(nb), dim3(256), 0, s, (const float*)rowsum, (const double*)bpart, (const int*)rows, info,
                       sched, (int)(first_iter + t), t, y, inc, gains, kl_trace);
    rc = rsp_check_launch("ts_update_kernel");
    if (rc != RSP_OK) return rc;
  }
  return RSP_OK;
}
