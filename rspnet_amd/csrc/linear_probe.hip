// Linear probe on frozen features (rsp_linear_probe_fit, rsp_linear_probe_logits): a softmax classifier z = (x f) W^T + b fitted by
// SGD with momentum over contiguous row chunks, every step of the fit issued from one call, nothing read back, nothing atomic.
// include/rspnet_hip.h states the rule; rspnet_amd/linear_probe.py restates it in numpy fp64 (probe_reference).
//
// Kernels:
//   probe_rows_kernel        one wave per row: the fp32 sum of squares by inv_norm_kernel's own routine (rsp_row_sumsq, cos_search.h), the row factor
//                            f = scale / sqrtf(ss) (normalize) or scale, and the flag every later kernel selects by: ss valid and
//                            the label inside [0, C).
//   probe_compact_kernel    per chunk of `batch` rows: its valid rows in ascending order as a list of row indices, and their number m
//                            (integers; rsp_compact_rows, cos_search.h).  Every later kernel of a step walks that list, so an invalid row
//                            is not read again and the fit is, to the bit, the fit on x without it; also the counts of all of x.
//   probe_fwd_kernel<CT, F>  cos_topk_kernel's / repr_pair_kernel's GEMM tile (64 rows, 32-wide k chunks through double-buffered
//                            LDS, register prefetch, v_mfma_f32_32x32x2_f32, the same accumulator mapping) with the rows of x f as
//                            one operand and CT rows of W as the other; the four waves are 2 x 2, each 32 rows x CT / 2 classes.
//                            F = false: bias and a plain store of z (the logits call: NaN for an invalid row).  F = true (one block owns all classes
//                            of its rows): z + bias goes to an LDS tile that aliases the chunk buffers, then wave w takes rows
//                            16 w .. 16 w + 15 one after the other (probe_softmax_rows): G and the row's loss, the logits never
//                            written.  Fixed order of the row reductions: lane l holds classes l, l + 64, ... in ascending order,
//                            then the wave's xor butterfly (32, 16, 8, 4, 2, 1); the 64 row losses of a block are added by one
//                            thread in row order.
//   probe_softmax_kernel     the same rows routine over z in global memory, in place (general path).
//   probe_wgrad_kernel       repr_gram_kernel with two different operands: block = a 64 x 128 tile of dW (classes x D) x one split
//                            of the step's rows.  Chunks of 32 rows are staged once as [row][64 G-columns | 128 xh-columns] and both
//                            MFMA operands are read from it transposed (the 32 lanes of a half read 32 consecutive words: conflict
//                            free).  The block of D-tile 0 also adds db of its 64 classes from the same staged chunk (wave 0, fp32,
//                            row order).  fp32 partials per split in the workspace; the split count is probe_splits at the step's m.
//   probe_update_kernel      one thread per element of W and b: the split partials in split order, weight decay, the rsp_sgd_step
//                            rule with lr read from the device array; wave 0 of block 0 adds the step's loss partials (lane l:
//                            partials l, l + 64, ... in order, then the butterfly) and writes loss_trace[t].
#include "cos_search.h"

namespace {

constexpr int PF_BR = 64;              // rows per forward tile
constexpr int PF_KC = 32;              // k per LDS chunk
constexpr int PF_LD = PF_KC + 4;       // LDS row pitch (floats) of a chunk: the float4 reads along k stay conflict-free
constexpr int PF_CT_GENERAL = 128;     // class tile of the general instance
constexpr int PF_FUSED_MAX_C = 256;

constexpr int WG_BA = 64;              // classes per dW tile
constexpr int WG_BB = 128;             // feature columns per dW tile
constexpr int WG_KC = 32;              // rows per staged chunk
constexpr int WG_LD = WG_BA + WG_BB;   // floats per staged row
constexpr int WG_BUF = WG_KC * WG_LD;
constexpr size_t WG_LDS_BYTES = (size_t)2 * WG_BUF * sizeof(float);      // 49 152: three workgroups per CU
constexpr int WG_TARGET_BLOCKS = 1024;

template <int CT>
constexpr size_t pf_lds_bytes() {
  return (size_t)2 * (PF_BR + CT) * PF_LD * sizeof(float);      // 55 296 (CT 128), 92 160 (CT 256)
}

__global__ __launch_bounds__(256) void probe_rows_kernel(const float* __restrict__ x, int ld, int N, int D,
                                                         const long long* __restrict__ y, int C, int normalize, float scale,
                                                         float* __restrict__ fac, int* __restrict__ ok) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= N) return;
  const float s = rsp_row_sumsq(x + (long long)row * ld, D, lane);
  if (lane == 0) {
    bool good = s < INFINITY && (normalize ? s > 0.f : s >= 0.f);      // (a NaN fails every comparison)
    if (y) {
      const long long lab = y[row];
      good = good && lab >= 0 && lab < C;
    }
    fac[row] = normalize ? scale / sqrtf(s) : scale;
    ok[row] = good ? 1 : 0;
  }
}

// The effective split count of a weight-gradient launch over `rows` rows: about WG_TARGET_BLOCKS blocks (cap = that over the tile
// count), at least four 32-row chunks per split (repr_gram_kernel's formula).  Monotone in rows: the launch is sized by `batch`, the
// kernels use the value at the step's m.
__host__ __device__ __forceinline__ int probe_splits(int cap, int rows) {
  const int s = min(cap, ((rows + WG_KC - 1) / WG_KC) / 4);
  return s < 1 ? 1 : s;
}

// block c < nchunks: the valid rows of chunk c (rows [c batch, c batch + batch) of x) in ascending order into idx[c batch ..], their
// number into mcnt[c] (rsp_compact_rows: integers, order fixed); block nchunks: the valid rows of all of x, into counts.
__global__ __launch_bounds__(256) void probe_compact_kernel(const int* __restrict__ ok, int N, int batch, int nchunks,
                                                            int* __restrict__ idx, int* __restrict__ mcnt, int* __restrict__ counts) {
  const int t = threadIdx.x, c = blockIdx.x;
  const long long lo = c < nchunks ? (long long)c * batch : 0;
  const long long hi = c < nchunks ? (lo + batch < N ? lo + batch : N) : N;
  const int base = rsp_compact_rows(lo, hi, [&](long long i) { return ok[i] != 0; }, [&](int r, long long i) {
    if (c < nchunks) idx[lo + r] = (int)i;
  });
  if (t == 0) {
    if (c < nchunks) {
      mcnt[c] = base;
    } else {
      counts[0] = base;
      counts[1] = N - base;
    }
  }
}

// Rows 16 wave .. 16 wave + 15 of the 64-row tile at i0 of the step's n valid rows, one after the other by the whole wave: z (pitch
// zld) -> G = (softmax(z) - onehot(y)) / n into g (pitch C; may be the same memory as z: a lane writes only elements it alone has
// read), the row's loss into rl[row of the tile] (0 past n).  rows: the step's valid rows (indices into x and y).
__device__ __forceinline__ void probe_softmax_rows(const float* z, int zld, float* g, int C, int i0, int n, const int* __restrict__ rows,
                                                   const long long* __restrict__ y, float* rl, int wave, int lane) {
  const float mf = (float)n;
  for (int q = 0; q < 16; ++q) {
    const int i = 16 * wave + q, rr = i0 + i;
    float loss = 0.f;
    if (rr < n) {
      const float* zr = z + (long long)i * zld;
      float* gr = g + (long long)rr * C;
      const int lab = (int)y[rows[rr]];
      float mx = -INFINITY;
      for (int c = lane; c < C; c += 64) mx = fmaxf(mx, zr[c]);
      mx = rsp_wave_max(mx);
      float s = 0.f, zy = 0.f;
      for (int c = lane; c < C; c += 64) {
        const float v = zr[c];
        s += expf(v - mx);
        if (c == lab) zy = v;
      }
      s = rsp_wave_sum(s);
      zy = __shfl(zy, lab & 63);
      loss = (mx + logf(s)) - zy;
      for (int c = lane; c < C; c += 64) gr[c] = (expf(zr[c] - mx) / s - (c == lab ? 1.f : 0.f)) / mf;
    }
    if (lane == 0) rl[i] = loss;
  }
}

template <int CT, bool FUSED>
__global__ __launch_bounds__(256) void probe_fwd_kernel(const float* __restrict__ x, int ld, int nmax, int D,
                                                        const float* __restrict__ fac, const int* __restrict__ rows,
                                                        const int* __restrict__ ok,
                                                        const long long* __restrict__ y, const float* __restrict__ W,
                                                        const float* __restrict__ b, int C, const int* __restrict__ mptr,
                                                        float* __restrict__ out, int ldo, float* __restrict__ losspart) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int NB = CT / 64;                       // 32-wide accumulators per wave
  constexpr int NG = CT / 16;                       // float2 slots of W per thread and chunk
  constexpr int BUF = (PF_BR + CT) * PF_LD;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l32 = lane & 31, h = lane >> 5;
  const int wq = wave >> 1, wg = wave & 1;
  const int i0 = blockIdx.x * PF_BR, c0 = blockIdx.y * CT;
  const int nch = (D + PF_KC - 1) / PF_KC;
  // the fit: the step's m valid rows, listed in `rows`; the logits call: rows 0 .. nmax - 1 of x, the invalid ones flagged in `ok`
  const int n = mptr ? mptr[0] : nmax;
  if (i0 >= n) return;      // (the whole block, before any barrier: the launch is sized by the step's row count, not by m)

  bool okq[4], okc[NG];      // the rows this thread stages: inside the step and valid; inside W
  float fq[4];
  int gq[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int rr = i0 + ((t + 256 * it) >> 4);
    gq[it] = rr < n ? (rows ? rows[rr] : rr) : 0;
    okq[it] = rr < n && (rows || ok[gq[it]] != 0);
    fq[it] = okq[it] ? fac[gq[it]] : 0.f;
  }
#pragma unroll
  for (int it = 0; it < NG; ++it) okc[it] = c0 + ((t + 256 * it) >> 4) < C;
  float2 rq[4], rg[NG];
  auto load = [&](int kc) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int k2 = kc + 2 * ((t + 256 * it) & 15);
      // selected, never multiplied away: an invalid row is not read at all
      rq[it] = (okq[it] && k2 < D) ? *reinterpret_cast<const float2*>(x + (long long)gq[it] * ld + k2) : make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int it = 0; it < NG; ++it) {
      const int e = t + 256 * it, row = e >> 4, k2 = kc + 2 * (e & 15);
      rg[it] = (okc[it] && k2 < D) ? *reinterpret_cast<const float2*>(W + (long long)(c0 + row) * D + k2) : make_float2(0.f, 0.f);
    }
  };
  auto store = [&](float* buf) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int e = t + 256 * it;
      *reinterpret_cast<float2*>(buf + (e >> 4) * PF_LD + 2 * (e & 15)) = make_float2(rq[it].x * fq[it], rq[it].y * fq[it]);
    }
#pragma unroll
    for (int it = 0; it < NG; ++it) {
      const int e = t + 256 * it;
      *reinterpret_cast<float2*>(buf + (PF_BR + (e >> 4)) * PF_LD + 2 * (e & 15)) = rg[it];
    }
  };

  floatx16 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[nb][e] = 0.f;
  }
  load(0);
  store(sm);
  __syncthreads();
  for (int ch = 0; ch < nch; ++ch) {
    const float* buf = sm + (ch & 1) * BUF;
    if (ch + 1 < nch) load((ch + 1) * PF_KC);
    const float* qa = buf + (32 * wq + l32) * PF_LD + 4 * h;
    const float* gb = buf + (PF_BR + (CT / 2) * wg + l32) * PF_LD + 4 * h;
    // lane half h takes k = 8m + 4h + j at step j of group m, for A and B alike: every k of the chunk once
#pragma unroll
    for (int m = 0; m < PF_KC / 8; ++m) {
      const float4 a = *reinterpret_cast<const float4*>(qa + 8 * m);
      float4 bb[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) bb[nb] = *reinterpret_cast<const float4*>(gb + 32 * nb * PF_LD + 8 * m);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bb[nb].x, acc[nb], 0, 0, 0);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bb[nb].y, acc[nb], 0, 0, 0);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bb[nb].z, acc[nb], 0, 0, 0);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bb[nb].w, acc[nb], 0, 0, 0);
    }
    if (ch + 1 < nch) store(sm + ((ch + 1) & 1) * BUF);
    __syncthreads();      // (after the last chunk too: the fused epilogue's tile aliases the buffers)
  }

  if constexpr (!FUSED) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int col = c0 + (CT / 2) * wg + 32 * nb + l32;
      const float bias = col < C ? b[col] : 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int rr = i0 + 32 * wq + (e >> 2) * 8 + h * 4 + (e & 3);
        if (rr < n && col < C) out[(long long)rr * ldo + col] = (rows || ok[rr] != 0) ? acc[nb][e] + bias : NAN;
      }
    }
  } else {
    constexpr int ZLD = CT + 1;      // 64 rows of CT + 1 floats and the 64 row losses: inside the two chunk buffers
    static_assert(PF_BR * ZLD + PF_BR <= 2 * BUF, "the logit tile must fit the chunk buffers");
    float* zt = sm;
    float* rl = sm + PF_BR * ZLD;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int lc = (CT / 2) * wg + 32 * nb + l32;
      const float bias = lc < C ? b[lc] : 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = 32 * wq + (e >> 2) * 8 + h * 4 + (e & 3);
        zt[i * ZLD + lc] = acc[nb][e] + bias;
      }
    }
    __syncthreads();
    probe_softmax_rows(zt, ZLD, out, C, i0, n, rows, y, rl, wave, lane);
    __syncthreads();
    if (t == 0) {
      float s = 0.f;
      for (int i = 0; i < PF_BR; ++i) s += rl[i];
      losspart[blockIdx.x] = s;
    }
  }
}

__global__ __launch_bounds__(256) void probe_softmax_kernel(float* zg, int C, const int* __restrict__ rows,
                                                            const long long* __restrict__ y, const int* __restrict__ mptr,
                                                            float* __restrict__ losspart) {
  __shared__ float rl[PF_BR];
  const int t = threadIdx.x, i0 = blockIdx.x * PF_BR, n = mptr[0];
  if (i0 >= n) return;
  probe_softmax_rows(zg + (long long)i0 * C, C, zg, C, i0, n, rows, y, rl, t >> 6, t & 63);
  __syncthreads();
  if (t == 0) {
    float s = 0.f;
    for (int i = 0; i < PF_BR; ++i) s += rl[i];
    losspart[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(256) void probe_wgrad_kernel(const float* __restrict__ G, int C, const float* __restrict__ x, int ld,
                                                          const int* __restrict__ rows, const int* __restrict__ mptr, int D,
                                                          const float* __restrict__ fac, int tiles_b, int split_cap,
                                                          float* __restrict__ dwpart, float* __restrict__ dbpart) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l32 = lane & 31, h = lane >> 5;
  const int wa = wave >> 1, wb = wave & 1;
  const int ta = blockIdx.x / tiles_b, tb = blockIdx.x - ta * tiles_b;
  const int a0 = ta * WG_BA, b0 = tb * WG_BB;
  const int split = blockIdx.y;
  const int n = mptr[0], splits = probe_splits(split_cap, n);
  if (split >= splits) return;      // (the whole block: the launch is sized by the split count at `batch` rows)
  const int chunks = (n + WG_KC - 1) / WG_KC;
  const int c_lo = (int)((long long)split * chunks / splits), c_hi = (int)((long long)(split + 1) * chunks / splits);
  const bool sums_db = tb == 0 && wave == 0;

  // this thread's float2 slots of a chunk: 4 of G (slot e = t + 256 it: staged row e / 32, float2 column e % 32 of the 64 classes) and
  // 8 of x (staged row e / 64, float2 column e % 64 of the 128 feature columns)
  const int gcol = a0 + 2 * (t & 31), xcol = b0 + 2 * (t & 63);
  float2 rg[4], rx[8];
  float rf[8];
  auto load = [&](int chunk) {
    // the row flags and factors first, then the data in one batch; the product is formed at the store
    int gx[8];
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int rr = chunk * WG_KC + ((t + 256 * it) >> 6);
      gx[it] = rr < n ? rows[rr] : -1;
      rf[it] = gx[it] >= 0 ? fac[gx[it]] : 0.f;
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      // G's pitch C may be odd: two scalar loads; a row past n is not read
      const int rr = chunk * WG_KC + ((t + 256 * it) >> 5);
      const float* gp = G + (long long)rr * C + gcol;
      rg[it].x = (rr < n && gcol < C) ? gp[0] : 0.f;
      rg[it].y = (rr < n && gcol + 1 < C) ? gp[1] : 0.f;
    }
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      rx[it] = (gx[it] >= 0 && xcol < D) ? *reinterpret_cast<const float2*>(x + (long long)gx[it] * ld + xcol) : make_float2(0.f, 0.f);
    }
  };
  auto store = [&](float* buf) {
#pragma unroll
    for (int it = 0; it < 4; ++it) *reinterpret_cast<float2*>(buf + ((t + 256 * it) >> 5) * WG_LD + 2 * (t & 31)) = rg[it];
#pragma unroll
    for (int it = 0; it < 8; ++it)
      *reinterpret_cast<float2*>(buf + ((t + 256 * it) >> 6) * WG_LD + WG_BA + 2 * (t & 63)) = make_float2(rx[it].x * rf[it], rx[it].y * rf[it]);
  };

  floatx16 acc0, acc1;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    acc0[e] = 0.f;
    acc1[e] = 0.f;
  }
  float cs = 0.f;
  load(c_lo);      // (with n = 0 the one split is empty: it stages zeros and uses none of them)
  store(sm);
  __syncthreads();
  for (int ch = c_lo; ch < c_hi; ++ch) {
    const float* buf = sm + ((ch - c_lo) & 1) * WG_BUF;
    if (ch + 1 < c_hi) load(ch + 1);
    // step j: lane half h holds staged row 2 j + h, for A (its class) and B (its feature columns) alike
    const float* pa = buf + h * WG_LD + 32 * wa + l32;
    const float* pb = buf + h * WG_LD + WG_BA + 64 * wb + l32;
#pragma unroll
    for (int j = 0; j < WG_KC / 2; ++j) {
      const float a = pa[2 * j * WG_LD];
      const float b0v = pb[2 * j * WG_LD], b1v = pb[2 * j * WG_LD + 32];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0v, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1v, acc1, 0, 0, 0);
    }
    if (sums_db) {
#pragma unroll
      for (int k = 0; k < WG_KC; ++k) cs += buf[k * WG_LD + lane];
    }
    if (ch + 1 < c_hi) store(sm + ((ch + 1 - c_lo) & 1) * WG_BUF);
    __syncthreads();
  }

  const int bc0 = b0 + 64 * wb + l32, bc1 = bc0 + 32;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int a = a0 + 32 * wa + (e >> 2) * 8 + h * 4 + (e & 3);
    if (a < C) {
      float* row = dwpart + ((long long)split * C + a) * D;
      if (bc0 < D) row[bc0] = acc0[e];
      if (bc1 < D) row[bc1] = acc1[e];
    }
  }
  if (sums_db && a0 + lane < C) dbpart[(long long)split * C + a0 + lane] = cs;
}

__global__ __launch_bounds__(256) void probe_update_kernel(const float* __restrict__ dwpart, const float* __restrict__ dbpart,
                                                           int split_cap, int C, int D, float* __restrict__ W, float* __restrict__ b,
                                                           float* __restrict__ mom, const float* __restrict__ lr_dev, int step,
                                                           float mu, float wd, const float* __restrict__ losspart,
                                                           const int* __restrict__ mptr, float* __restrict__ loss_out) {
  const long long CD = (long long)C * D;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const float lr = lr_dev[step];
  const int m = mptr[0], splits = probe_splits(split_cap, m);
  if (i < CD + C) {
    const bool is_w = i < CD;
    const float* part = is_w ? dwpart + i : dbpart + (i - CD);
    const long long pitch = is_w ? CD : C;
    float* p = is_w ? W + i : b + (i - CD);
    float g = 0.f;
    for (int s = 0; s < splits; ++s) g += part[s * pitch];
    const float pv = *p;
    const float d = g + wd * pv;
    const float bv = step == 0 ? d : mom[i] * mu + d;
    mom[i] = bv;
    *p = pv - lr * bv;
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    const int nloss = (m + PF_BR - 1) / PF_BR;
    float s = 0.f;
    for (int k = threadIdx.x; k < nloss; k += 64) s += losspart[k];
    s = rsp_wave_sum(s);
    if (threadIdx.x == 0) loss_out[0] = m > 0 ? s / (float)m : 0.f;
  }
}

// ---- host: the carve-up of the workspace --------------------------------------------------------------------------------
struct Plan {
  int nchunks, tiles_a, tiles_b, split_cap, splits, nloss;
  size_t off_ok, off_idx, off_mcnt, off_g, off_loss, off_dw, off_db, bytes, rows_bytes;
};

Plan make_plan(int N, int D, int C, int batch) {
  Plan p;
  p.nchunks = rsp_cdiv(N, batch);
  p.tiles_a = rsp_cdiv(C, WG_BA);
  p.tiles_b = rsp_cdiv(D, WG_BB);
  p.split_cap = rsp_cdiv(WG_TARGET_BLOCKS, p.tiles_a * p.tiles_b);
  p.splits = probe_splits(p.split_cap, batch);
  p.nloss = rsp_cdiv(batch, PF_BR);
  p.off_ok = rsp_align_up((size_t)N * sizeof(float), 256);
  p.rows_bytes = p.off_ok + rsp_align_up((size_t)N * sizeof(int), 256);
  p.off_idx = p.rows_bytes;
  p.off_mcnt = p.off_idx + rsp_align_up((size_t)N * sizeof(int), 256);
  p.off_g = p.off_mcnt + rsp_align_up((size_t)p.nchunks * sizeof(int), 256);
  p.off_loss = p.off_g + rsp_align_up((size_t)batch * C * sizeof(float), 256);
  p.off_dw = p.off_loss + rsp_align_up((size_t)p.nloss * sizeof(float), 256);
  p.off_db = p.off_dw + rsp_align_up((size_t)p.splits * C * D * sizeof(float), 256);
  p.bytes = p.off_db + rsp_align_up((size_t)p.splits * C * sizeof(float), 256);
  return p;
}

bool sizes_ok(int N, int D, int C) { return N >= 1 && D >= 2 && D <= 4096 && D % 2 == 0 && C >= 1 && C <= 1024; }

int fail(const char* who, const char* what, int code) {
  char buf[200];
  snprintf(buf, sizeof buf, "%s: %s", who, what);
  rsp_set_error(buf);
  return code;
}

bool aligned(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

bool force_general() {
  const char* e = getenv("RSP_PROBE_GENERAL");      // A/B and test switch: the general instance at any C
  return e && *e && *e != '0';
}

int launch_rows(const float* x, int ld, int N, int D, const long long* y, int C, int normalize, float scale, float* fac, int* ok,
                hipStream_t s) {
  hipLaunchKernelGGL(probe_rows_kernel, dim3(rsp_cdiv(N, 4)), dim3(256), 0, s, x, ld, N, D, y, C, normalize, scale, fac, ok);
  return rsp_check_launch("probe_rows_kernel");
}

template <int CT, bool FUSED>
int launch_fwd(dim3 grid, hipStream_t s, const float* x, int ld, int nmax, int D, const float* fac, const int* rows, const int* ok,
               const long long* y, const float* W, const float* b, int C, const int* mptr, float* out, int ldo, float* losspart) {
  return launch_lds<probe_fwd_kernel<CT, FUSED>>("probe_fwd_kernel", grid, pf_lds_bytes<CT>(), s, x, ld, nmax, D, fac, rows, ok, y, W, b, C, mptr,
                                                 out, ldo, losspart);
}

}  // namespace

size_t rsp_linear_probe_workspace(int32_t N, int32_t D, int32_t C, int32_t batch) {
  return (sizes_ok(N, D, C) && batch >= 1 && batch <= N) ? make_plan(N, D, C, batch).bytes : 0;
}

int rsp_linear_probe_fit(const float* x, int32_t ld, int32_t N, int32_t D, const int64_t* y, int32_t C, int32_t batch,
                         int32_t first_step, int32_t steps, const float* lr_dev, float mu, float wd, int32_t normalize, float scale,
                         float* w, float* b, float* mom, float* loss_trace, int32_t* counts, void* workspace, size_t workspace_bytes,
                         void* stream) {
  const char* who = "rsp_linear_probe_fit";
  if (!x || !y || !lr_dev || !w || !b || !mom || !loss_trace || !counts || !workspace) return fail(who, "null pointer", RSP_EINVAL);
  if (!(sizes_ok(N, D, C) && ld >= D && ld % 2 == 0))
    return fail(who, "bad size (1 <= N, 2 <= D <= 4096, D and ld even, ld >= D, 1 <= C <= 1024)", RSP_EINVAL);
  if (!(batch >= 1 && batch <= N && steps >= 1 && first_step >= 0 && (long long)first_step + steps <= 0x7fffffffll))
    return fail(who, "bad step plan (1 <= batch <= N, 1 <= steps, 0 <= first_step)", RSP_EINVAL);
  if (!aligned(x, 8) || !aligned(y, 8) || !aligned(w, 8) || !aligned(workspace, 8))
    return fail(who, "x, y, w and the workspace must be 8-byte aligned", RSP_EINVAL);
  if (!aligned(lr_dev, 4) || !aligned(b, 4) || !aligned(mom, 4) || !aligned(loss_trace, 4) || !aligned(counts, 4))
    return fail(who, "lr, b, mom, loss_trace and counts must be 4-byte aligned", RSP_EINVAL);
  const Plan p = make_plan(N, D, C, batch);
  if (workspace_bytes < p.bytes) return fail(who, "workspace too small", RSP_EWORKSPACE);
  hipStream_t s = (hipStream_t)stream;
  char* ws = reinterpret_cast<char*>(workspace);
  float* fac = reinterpret_cast<float*>(ws);
  int* ok = reinterpret_cast<int*>(ws + p.off_ok);
  int* idx = reinterpret_cast<int*>(ws + p.off_idx);
  int* mcnt = reinterpret_cast<int*>(ws + p.off_mcnt);
  float* G = reinterpret_cast<float*>(ws + p.off_g);
  float* losspart = reinterpret_cast<float*>(ws + p.off_loss);
  float* dwpart = reinterpret_cast<float*>(ws + p.off_dw);
  float* dbpart = reinterpret_cast<float*>(ws + p.off_db);
  const long long* yl = reinterpret_cast<const long long*>(y);
  const bool fused = C <= PF_FUSED_MAX_C && !force_general();

  int rc = launch_rows(x, ld, N, D, yl, C, normalize, scale, fac, ok, s);
  if (rc != RSP_OK) return rc;
  hipLaunchKernelGGL(probe_compact_kernel, dim3(p.nchunks + 1), dim3(256), 0, s, (const int*)ok, (int)N, (int)batch, p.nchunks, idx,
                     mcnt, (int*)counts);
  rc = rsp_check_launch("probe_compact_kernel");
  if (rc != RSP_OK) return rc;

  const long long outs = (long long)C * D + C;
  for (int t = 0; t < steps; ++t) {
    const int chunk = t % p.nchunks;
    const int r0 = chunk * batch, n = (N - r0) < batch ? (N - r0) : batch;
    const int* mptr = mcnt + chunk;
    const int* rows = idx + r0;
    const int tiles = rsp_cdiv(n, PF_BR);
    const int* none = nullptr;
    if (fused && C <= 128) {
      rc = launch_fwd<128, true>(dim3(tiles), s, x, ld, n, D, fac, rows, none, yl, w, b, C, mptr, G, C, losspart);
    } else if (fused) {
      rc = launch_fwd<256, true>(dim3(tiles), s, x, ld, n, D, fac, rows, none, yl, w, b, C, mptr, G, C, losspart);
    } else {
      rc = launch_fwd<PF_CT_GENERAL, false>(dim3(tiles, rsp_cdiv(C, PF_CT_GENERAL)), s, x, ld, n, D, fac, rows, none, yl, w, b, C, mptr, G, C,
                                            losspart);
      if (rc != RSP_OK) return rc;
      hipLaunchKernelGGL(probe_softmax_kernel, dim3(tiles), dim3(256), 0, s, G, (int)C, rows, yl, mptr, losspart);
      rc = rsp_check_launch("probe_softmax_kernel");
    }
    if (rc != RSP_OK) return rc;
    rc = launch_lds<probe_wgrad_kernel>("probe_wgrad_kernel", dim3(p.tiles_a * p.tiles_b, p.splits), WG_LDS_BYTES, s, (const float*)G, (int)C,
                                        x, (int)ld, rows, mptr, (int)D, (const float*)fac, p.tiles_b, p.split_cap, dwpart, dbpart);
    if (rc != RSP_OK) return rc;
    hipLaunchKernelGGL(probe_update_kernel, dim3(rsp_cdiv(outs, 256)), dim3(256), 0, s, (const float*)dwpart, (const float*)dbpart,
                       p.split_cap, (int)C, (int)D, w, b, mom, lr_dev, (int)(first_step + t), mu, wd, (const float*)losspart, mptr,
                       loss_trace + t);
    rc = rsp_check_launch("probe_update_kernel");
    if (rc != RSP_OK) return rc;
  }
  return RSP_OK;
}

int rsp_linear_probe_logits(const float* x, int32_t ld, int32_t N, int32_t D, const float* w, const float* b, int32_t C,
                            int32_t normalize, float scale, float* logits, int32_t ld_out, void* workspace, size_t workspace_bytes,
                            void* stream) {
  const char* who = "rsp_linear_probe_logits";
  if (!x || !w || !b || !logits || !workspace) return fail(who, "null pointer", RSP_EINVAL);
  if (!(sizes_ok(N, D, C) && ld >= D && ld % 2 == 0 && ld_out >= C))
    return fail(who, "bad size (1 <= N, 2 <= D <= 4096, D and ld even, ld >= D, 1 <= C <= 1024, ld_out >= C)", RSP_EINVAL);
  if (!aligned(x, 8) || !aligned(w, 8) || !aligned(workspace, 8) || !aligned(b, 4) || !aligned(logits, 4))
    return fail(who, "x, w and the workspace must be 8-byte aligned, b and logits 4-byte", RSP_EINVAL);
  const Plan p = make_plan(N, D, C, N);
  if (workspace_bytes < p.rows_bytes) return fail(who, "workspace too small", RSP_EWORKSPACE);
  hipStream_t s = (hipStream_t)stream;
  char* ws = reinterpret_cast<char*>(workspace);
  float* fac = reinterpret_cast<float*>(ws);
  int* ok = reinterpret_cast<int*>(ws + p.off_ok);
  int rc = launch_rows(x, ld, N, D, nullptr, C, normalize, scale, fac, ok, s);
  if (rc != RSP_OK) return rc;
  return launch_fwd<PF_CT_GENERAL, false>(dim3(rsp_cdiv(N, PF_BR), rsp_cdiv(C, PF_CT_GENERAL)), s, x, ld, N, D, fac,
                                          (const int*)nullptr, (const int*)ok, (const long long*)nullptr, w, b, C, (const int*)nullptr, logits,
                                          ld_out, (float*)nullptr);
}
