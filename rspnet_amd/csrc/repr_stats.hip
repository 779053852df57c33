// Label-free representation statistics of N embedding rows (rsp_repr_stats): the sums over all valid pairs i < j of exp(c (s - 1)), s and
// s^2 of the cosine similarity s, the D x D Gram matrix of the unit rows and their column sums -- one call, the N x N matrix never
// stored, nothing atomic.  include/rspnet_hip.h states the rule; rspnet_amd/repr_stats.py restates it in numpy fp64.
//
// Kernels:
//   inv_norm_kernel      the search's (rsp_inv_norms, cos_search.h): inv = 1/sqrtf(ss) for a valid row (ss finite and > 0), 0 for an
//                        invalid one -- the flag every later kernel selects by.
//   repr_pair_kernel     cos_topk_kernel's GEMM tile (64 x 128 rows, 32-wide k chunks through double-buffered LDS, register prefetch,
//                        v_mfma_f32_32x32x2_f32, the same accumulator mapping) with both operands from x.  The tiles that hold some
//                        i < j are numbered column tile by column tile: column tile tj (rows 128 tj ..) meets row tiles 0 .. 2 tj + 1, so
//                        tile id = tj (tj + 1) + ti.  A block takes `per` consecutive ids; the epilogue masks element-wise (i < j, both
//                        rows valid), each thread adds its 32 elements of a tile in fp32, then into its fp64 sums; the block's fp64
//                        sums (wave butterfly, then the four waves in order) go to the workspace.
//   repr_gram_kernel     block = a 64 x 128 tile of the Gram matrix x one split of the row axis.  Chunks of 32 rows are staged once as
//                        [row][64 a-columns | 128 b-columns] of xh = x * inv (invalid rows and the out-of-range selected to 0); both
//                        MFMA operands are read from it transposed: lane l reads row k = 2 j + (l >> 5), column l & 31 -- the 32 lanes
//                        of a half read 32 consecutive words, which is conflict-free at any pitch.  A tile wholly below the diagonal
//                        (a0 >= b0 + 128) returns at once: its elements are the mirror images of computed ones.  The block of b-tile
//                        ta / 2 -- always computed -- also adds the column sums of its 64 a-columns (wave 0, fp32, row order).  fp32
//                        partials per split in the workspace.
//   repr_reduce_kernel   gram / colsum: the splits in split order in fp64, every element written; an element of a skipped tile is
//                        read from its mirror image, so the matrix is symmetric to the bit.
//   repr_final_kernel    one block: the pair partials in a fixed order in fp64, the valid / invalid row counts (integers).
#include "cos_search.h"

#include <math.h>

namespace {

constexpr int RP_BQ = 64;              // rows i per pair tile
constexpr int RP_BG = 128;             // rows j per pair tile
constexpr int RP_KC = 32;              // k per LDS chunk
constexpr int RP_LD = RP_KC + 4;       // LDS row pitch (floats) of a chunk: the float4 reads along k stay conflict-free
constexpr int RP_BUF = (RP_BQ + RP_BG) * RP_LD;
constexpr size_t RP_LDS_BYTES = (size_t)2 * RP_BUF * sizeof(float);      // 55 296: two workgroups per CU
constexpr int RP_MAX_BLOCKS = 1 << 15;

constexpr int GR_BA = 64;              // Gram rows (a) per tile
constexpr int GR_BB = 128;             // Gram columns (b) per tile
constexpr int GR_KC = 32;              // embedding rows per staged chunk
constexpr int GR_LD = GR_BA + GR_BB;   // floats per staged row
constexpr int GR_BUF = GR_KC * GR_LD;
constexpr size_t GR_LDS_BYTES = (size_t)2 * GR_BUF * sizeof(float);      // 49 152: three workgroups per CU
constexpr int GR_TARGET_BLOCKS = 1024;
constexpr int FIN_THREADS = 1024;

__global__ __launch_bounds__(256) void repr_pair_kernel(const float* __restrict__ x, int ld, int N, int D, float c,
                                                        const float* __restrict__ inv, int ntiles, int per, int nct,
                                                        double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  __shared__ double red[4][3];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l32 = lane & 31, h = lane >> 5;
  const int wq = wave >> 1, wg = wave & 1;
  const int nch = (D + RP_KC - 1) / RP_KC;
  const int id_lo = blockIdx.x * per, id_hi = min(id_lo + per, ntiles);
  const int last0 = (nct - 1) * nct;      // first id of the last column tile (it meets every row tile)
  double de = 0.0, ds = 0.0, d2 = 0.0;

  for (int id = id_lo; id < id_hi; ++id) {
    int tj;
    if (id >= last0) {
      tj = nct - 1;
    } else {
      tj = (int)((sqrtf(4.f * (float)id + 1.f) - 1.f) * 0.5f);
      while (tj * (tj + 1) > id) --tj;
      while ((tj + 1) * (tj + 2) <= id) ++tj;
    }
    const int i0 = (id - tj * (tj + 1)) * RP_BQ, j0 = tj * RP_BG;

    bool okq[4], okg[8];      // the rows this thread stages: inside x and valid
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int row = i0 + ((t + 256 * it) >> 4);
      okq[it] = row < N && inv[row] > 0.f;
    }
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int row = j0 + ((t + 256 * it) >> 4);
      okg[it] = row < N && inv[row] > 0.f;
    }
    float2 rq[4], rg[8];
    auto load = [&](int kc) {
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int e = t + 256 * it, row = e >> 4, k2 = kc + 2 * (e & 15);
        rq[it] = (okq[it] && k2 < D) ? *reinterpret_cast<const float2*>(x + (long long)(i0 + row) * ld + k2) : make_float2(0.f, 0.f);
      }
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int e = t + 256 * it, row = e >> 4, k2 = kc + 2 * (e & 15);
        rg[it] = (okg[it] && k2 < D) ? *reinterpret_cast<const float2*>(x + (long long)(j0 + row) * ld + k2) : make_float2(0.f, 0.f);
      }
    };
    auto store = [&](float* buf) {
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int e = t + 256 * it;
        *reinterpret_cast<float2*>(buf + (e >> 4) * RP_LD + 2 * (e & 15)) = rq[it];
      }
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int e = t + 256 * it;
        *reinterpret_cast<float2*>(buf + (RP_BQ + (e >> 4)) * RP_LD + 2 * (e & 15)) = rg[it];
      }
    };

    floatx16 acc0, acc1;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      acc0[e] = 0.f;
      acc1[e] = 0.f;
    }
    load(0);
    store(sm);
    __syncthreads();
    for (int ch = 0; ch < nch; ++ch) {
      const float* buf = sm + (ch & 1) * RP_BUF;
      if (ch + 1 < nch) load((ch + 1) * RP_KC);
      const float* qa = buf + (32 * wq + l32) * RP_LD + 4 * h;
      const float* gb0 = buf + (RP_BQ + 64 * wg + l32) * RP_LD + 4 * h;
      const float* gb1 = gb0 + 32 * RP_LD;
      // lane half h takes k = 8m + 4h + j at step j of group m, for A and B alike: every k of the chunk once
#pragma unroll
      for (int m = 0; m < RP_KC / 8; ++m) {
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
      if (ch + 1 < nch) store(sm + ((ch + 1) & 1) * RP_BUF);
      __syncthreads();      // (after the last chunk too: the next tile's first store overwrites buffer 0)
    }

    // the thread's 32 elements in a fixed order in fp32, then into its fp64 sums
    const int jc0 = j0 + 64 * wg + l32, jc1 = jc0 + 32;
    const float ig0 = jc0 < N ? inv[jc0] : 0.f;
    const float ig1 = jc1 < N ? inv[jc1] : 0.f;
    float fe = 0.f, fs = 0.f, f2 = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int i = i0 + 32 * wq + (e >> 2) * 8 + h * 4 + (e & 3);
      const float iq = i < N ? inv[i] : 0.f;
      const bool ok0 = iq > 0.f && ig0 > 0.f && i < jc0;      // (an inverse norm > 0: the row exists and is valid)
      const bool ok1 = iq > 0.f && ig1 > 0.f && i < jc1;
      const float s0 = ok0 ? acc0[e] * iq * ig0 : 0.f;
      const float s1 = ok1 ? acc1[e] * iq * ig1 : 0.f;
      fe += ok0 ? expf(c * (s0 - 1.f)) : 0.f;
      fs += s0;
      f2 += s0 * s0;
      fe += ok1 ? expf(c * (s1 - 1.f)) : 0.f;
      fs += s1;
      f2 += s1 * s1;
    }
    de += (double)fe;
    ds += (double)fs;
    d2 += (double)f2;
  }

  de = rsp_wave_sum_d(de);
  ds = rsp_wave_sum_d(ds);
  d2 = rsp_wave_sum_d(d2);
  if (lane == 0) {
    red[wave][0] = de;
    red[wave][1] = ds;
    red[wave][2] = d2;
  }
  __syncthreads();
  if (t < 3) part[(long long)blockIdx.x * 3 + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

__global__ __launch_bounds__(256) void repr_gram_kernel(const float* __restrict__ x, int ld, int N, int D, const float* __restrict__ inv,
                                                        int tiles_b, int splits, float* __restrict__ gpart, float* __restrict__ cpart) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l32 = lane & 31, h = lane >> 5;
  const int wa = wave >> 1, wb = wave & 1;
  const int ta = blockIdx.x / tiles_b, tb = blockIdx.x - ta * tiles_b;
  const int a0 = ta * GR_BA, b0 = tb * GR_BB;
  if (a0 >= b0 + GR_BB) return;      // wholly below the diagonal: repr_reduce_kernel mirrors (the whole block leaves, before any barrier)
  const int split = blockIdx.y;
  const int chunks = (N + GR_KC - 1) / GR_KC;
  const int c_lo = (int)((long long)split * chunks / splits), c_hi = (int)((long long)(split + 1) * chunks / splits);
  const bool sums_cols = tb == (ta >> 1) && wave == 0;      // (128 (ta / 2) <= a0: a computed tile for every ta)

  // this thread's 12 float2 slots of a chunk: slot e = t + 256 it is staged row e / 96, float2 column e % 96 (32 of a, then 64 of b)
  int srow[12], scol[12];
#pragma unroll
  for (int it = 0; it < 12; ++it) {
    const int e = t + 256 * it, c2 = e % (GR_LD / 2);
    srow[it] = e / (GR_LD / 2);
    scol[it] = c2 < GR_BA / 2 ? a0 + 2 * c2 : b0 + 2 * (c2 - GR_BA / 2);
  }
  // the inverse norms of a chunk's rows first, then the x loads in one batch (a load whose use sits inside its own branch would be
  // waited for there: twelve round trips in a row); the product is formed at the store
  float2 r[12];
  float riv[12];
  auto load = [&](int chunk) {
#pragma unroll
    for (int it = 0; it < 12; ++it) {
      const int n = chunk * GR_KC + srow[it];
      riv[it] = n < N ? inv[n] : 0.f;
    }
#pragma unroll
    for (int it = 0; it < 12; ++it) {
      const int n = chunk * GR_KC + srow[it];
      // selected, never multiplied away: an invalid row is not read at all
      r[it] = (riv[it] > 0.f && scol[it] < D) ? *reinterpret_cast<const float2*>(x + (long long)n * ld + scol[it]) : make_float2(0.f, 0.f);
    }
  };
  auto store = [&](float* buf) {
#pragma unroll
    for (int it = 0; it < 12; ++it)
      *reinterpret_cast<float2*>(buf + 2 * (t + 256 * it)) = make_float2(r[it].x * riv[it], r[it].y * riv[it]);
  };

  floatx16 acc0, acc1;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    acc0[e] = 0.f;
    acc1[e] = 0.f;
  }
  float cs = 0.f;
  load(c_lo);
  store(sm);
  __syncthreads();
  for (int ch = c_lo; ch < c_hi; ++ch) {
    const float* buf = sm + ((ch - c_lo) & 1) * GR_BUF;
    if (ch + 1 < c_hi) load(ch + 1);
    // step j: lane half h holds staged row 2 j + h, for A (its a-column) and B (its b-columns) alike
    const float* pa = buf + h * GR_LD + 32 * wa + l32;
    const float* pb = buf + h * GR_LD + GR_BA + 64 * wb + l32;
#pragma unroll
    for (int j = 0; j < GR_KC / 2; ++j) {
      const float a = pa[2 * j * GR_LD];
      const float b0v = pb[2 * j * GR_LD], b1v = pb[2 * j * GR_LD + 32];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0v, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1v, acc1, 0, 0, 0);
    }
    if (sums_cols) {
#pragma unroll
      for (int k = 0; k < GR_KC; ++k) cs += buf[k * GR_LD + lane];
    }
    if (ch + 1 < c_hi) store(sm + ((ch + 1 - c_lo) & 1) * GR_BUF);
    __syncthreads();
  }

  const int bc0 = b0 + 64 * wb + l32, bc1 = bc0 + 32;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int a = a0 + 32 * wa + (e >> 2) * 8 + h * 4 + (e & 3);
    if (a < D) {
      float* row = gpart + ((long long)split * D + a) * D;
      if (bc0 < D) row[bc0] = acc0[e];
      if (bc1 < D) row[bc1] = acc1[e];
    }
  }
  if (sums_cols && a0 + lane < D) cpart[(long long)split * D + a0 + lane] = cs;
}

__global__ __launch_bounds__(256) void repr_reduce_kernel(const float* __restrict__ gpart, const float* __restrict__ cpart, int D,
                                                          int splits, double* __restrict__ gram, double* __restrict__ colsum) {
  const long long DD = (long long)D * D;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < DD) {
    const int a = (int)(i / D), b = (int)(i - (long long)a * D);
    const bool computed = a / GR_BA * GR_BA < b / GR_BB * GR_BB + GR_BB;      // repr_gram_kernel's own test on the element's tile
    const long long src = computed ? i : (long long)b * D + a;
    double s = 0.0;
    for (int sp = 0; sp < splits; ++sp) s += (double)gpart[sp * DD + src];
    gram[i] = s;
  } else if (i < DD + D) {
    const int a = (int)(i - DD);
    double s = 0.0;
    for (int sp = 0; sp < splits; ++sp) s += (double)cpart[(long long)sp * D + a];
    colsum[a] = s;
  }
}

__global__ __launch_bounds__(FIN_THREADS) void repr_final_kernel(const double* __restrict__ part, int nblocks,
                                                                 const float* __restrict__ inv, int N, rsp_repr_sums* __restrict__ out) {
  __shared__ double red[FIN_THREADS / 64][3];
  __shared__ int cnt[FIN_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  double v[3] = {0.0, 0.0, 0.0};
  for (int b = t; b < nblocks; b += FIN_THREADS) {
#pragma unroll
    for (int q = 0; q < 3; ++q) v[q] += part[(long long)b * 3 + q];
  }
  int good = 0;
  for (int i = t; i < N; i += FIN_THREADS) good += inv[i] > 0.f ? 1 : 0;
#pragma unroll
  for (int q = 0; q < 3; ++q) v[q] = rsp_wave_sum_d(v[q]);
  good = rsp_wave_sum_i(good);
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < 3; ++q) red[wave][q] = v[q];
    cnt[wave] = good;
  }
  __syncthreads();
  if (t == 0) {
    double s[3] = {0.0, 0.0, 0.0};
    int g = 0;
    for (int w = 0; w < FIN_THREADS / 64; ++w) {
#pragma unroll
      for (int q = 0; q < 3; ++q) s[q] += red[w][q];
      g += cnt[w];
    }
    out->pair_exp = s[0];
    out->pair_cos = s[1];
    out->pair_cos2 = s[2];
    out->rows_valid = g;
    out->rows_bad = N - g;
  }
}

// ---- host: the tile walk and the carve-up of the workspace ------------------------------------------------------------------
struct Plan {
  int nct, ntiles, per, blocks;      // pair kernel
  int tiles_a, tiles_b, splits;      // Gram kernel
  size_t off_part, off_gpart, off_cpart, bytes;
};

Plan make_plan(int N, int D) {
  Plan p;
  p.nct = rsp_cdiv(N, RP_BG);
  p.ntiles = (p.nct - 1) * p.nct + rsp_cdiv(N, RP_BQ);
  p.per = rsp_cdiv(p.ntiles, RP_MAX_BLOCKS);
  p.blocks = rsp_cdiv(p.ntiles, p.per);
  p.tiles_a = rsp_cdiv(D, GR_BA);
  p.tiles_b = rsp_cdiv(D, GR_BB);
  // about GR_TARGET_BLOCKS blocks, at least four 32-row chunks per split
  const int chunks = rsp_cdiv(N, GR_KC);
  int s = rsp_cdiv(GR_TARGET_BLOCKS, p.tiles_a * p.tiles_b);
  if (s > chunks / 4) s = chunks / 4;
  p.splits = s < 1 ? 1 : s;
  p.off_part = rsp_align_up((size_t)N * sizeof(float), 256);
  // (sized by the bound, not by `blocks`: the query is monotone in N)
  p.off_gpart = p.off_part + rsp_align_up((size_t)(p.ntiles < RP_MAX_BLOCKS ? p.ntiles : RP_MAX_BLOCKS) * 3 * sizeof(double), 256);
  p.off_cpart = p.off_gpart + rsp_align_up((size_t)p.splits * D * D * sizeof(float), 256);
  p.bytes = p.off_cpart + rsp_align_up((size_t)p.splits * D * sizeof(float), 256);
  return p;
}

bool sizes_ok(int N, int D) { return N >= 1 && N <= 262144 && D >= 2 && D <= 4096 && D % 2 == 0; }

int fail(const char* what, int code) {
  char buf[160];
  snprintf(buf, sizeof buf, "rsp_repr_stats: %s", what);
  rsp_set_error(buf);
  return code;
}

bool aligned8(const void* p) { return (((uintptr_t)p) & 7) == 0; }

}  // namespace

size_t rsp_repr_stats_workspace(int32_t N, int32_t D) { return sizes_ok(N, D) ? make_plan(N, D).bytes : 0; }

int rsp_repr_stats(const float* x, int32_t ld, int32_t N, int32_t D, float c, rsp_repr_sums* sums, double* gram, double* colsum,
                   void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !sums || !workspace) return fail("null pointer", RSP_EINVAL);
  if (!(sizes_ok(N, D) && ld >= D && ld % 2 == 0))
    return fail("bad size (1 <= N <= 262144, 2 <= D <= 4096, D and ld even, ld >= D)", RSP_EINVAL);
  if (!(isfinite(c) && c > 0.f && c <= 64.f)) return fail("c must be finite and in (0, 64]", RSP_EINVAL);
  if ((gram == nullptr) != (colsum == nullptr)) return fail("gram and colsum go together", RSP_EINVAL);
  if (!aligned8(x) || !aligned8(sums) || !aligned8(gram) || !aligned8(colsum) || !aligned8(workspace))
    return fail("x, sums, gram, colsum and the workspace must be 8-byte aligned", RSP_EINVAL);
  const Plan p = make_plan(N, D);
  if (workspace_bytes < p.bytes) return fail("workspace too small", RSP_EWORKSPACE);
  hipStream_t s = (hipStream_t)stream;
  char* ws = reinterpret_cast<char*>(workspace);
  float* inv = reinterpret_cast<float*>(ws);
  double* part = reinterpret_cast<double*>(ws + p.off_part);
  float* gpart = reinterpret_cast<float*>(ws + p.off_gpart);
  float* cpart = reinterpret_cast<float*>(ws + p.off_cpart);

  int rc = rsp_inv_norms(x, ld, N, D, inv, nullptr, s);
  if (rc != RSP_OK) return rc;
  rc = launch_lds<repr_pair_kernel>("repr_pair_kernel", dim3(p.blocks), RP_LDS_BYTES, s, x, (int)ld, (int)N, (int)D, c, (const float*)inv,
                                    p.ntiles, p.per, p.nct, part);
  if (rc != RSP_OK) return rc;
  hipLaunchKernelGGL(repr_final_kernel, dim3(1), dim3(FIN_THREADS), 0, s, (const double*)part, p.blocks, (const float*)inv, N, sums);
  rc = rsp_check_launch("repr_final_kernel");
  if (rc != RSP_OK || !gram) return rc;
  rc = launch_lds<repr_gram_kernel>("repr_gram_kernel", dim3(p.tiles_a * p.tiles_b, p.splits), GR_LDS_BYTES, s, x, (int)ld, (int)N, (int)D,
                                    (const float*)inv, p.tiles_b, p.splits, gpart, cpart);
  if (rc != RSP_OK) return rc;
  const long long outs = (long long)D * D + D;
  hipLaunchKernelGGL(repr_reduce_kernel, dim3(rsp_cdiv(outs, 256)), dim3(256), 0, s, (const float*)gpart, (const float*)cpart, D,
                     p.splits, gram, colsum);
  return rsp_check_launch("repr_reduce_kernel");
}
