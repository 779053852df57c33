// Video retrieval search (the search half of the reference's retrieval.py:150-176): for every query row the k nearest gallery
// rows by cosine distance, without ever materialising the Nq x Ng distance matrix, and the top-k hit counts from the result.
//
// Ranking rule: similarity s = (q.g) * (1/|q|) * (1/|g|) in fp32 (a zero-norm row has inverse norm 0, so s = 0 and distance 1,
// as sklearn's normalize leaves such a row zero); rows are ranked by s descending, an exact tie goes to the LOWER gallery index.
// That is a total order, so the result is unique: every split of the gallery computes the same s for the same pair (same
// k order of the dot product) and the merge of the per-split lists by the same order gives the same list for any split count.
//
// Kernels:
//   inv_norm_kernel    one wave per row: 1/|x| (0 for a zero row) of the query and gallery rows, into the workspace.
//   cos_topk_kernel    block = 64 queries x one gallery split.  Per gallery tile of 128 rows the 4 waves (2 x 2, 32 x 64 each)
//                      accumulate the dot products on v_mfma_f32_32x32x2_f32 from LDS chunks of 32 k (register prefetch of the
//                      next chunk, double-buffered LDS), scale them to similarities into an LDS score tile (aliasing the chunk
//                      buffers), and each wave updates the running top-k of 16 queries: its list lives in registers, lane j
//                      = rank j; tile scores above the current k-th best are inserted in ascending gallery order (ballot +
//                      shift), which keeps the tie rule.  The split's list goes to the workspace.
//   cos_merge_kernel   one wave per query: merges the split lists in split order by the same insertion, writes indices and
//                      distances clip(1 - s, 0, 2); empty slots (Ng < k) get index -1 and distance +inf.
//   topk_hits_kernel   one block: per query the first rank whose gallery label equals the query's label, counted per k.
#include "common.h"

#include <math.h>

namespace {

constexpr int CT_BQ = 64;              // queries per block
constexpr int CT_BG = 128;             // gallery rows per tile
constexpr int CT_KC = 32;              // k per LDS chunk
constexpr int CT_LD = CT_KC + 4;       // LDS row pitch (floats) of a chunk
constexpr int CT_SLD = CT_BG + 4;      // LDS row pitch (floats) of the score tile
constexpr int CT_BUF = (CT_BQ + CT_BG) * CT_LD;      // floats per chunk buffer
constexpr int CT_MAXK = 64;
constexpr int CT_MAX_KS = 16;

static_assert(CT_BQ * CT_SLD <= 2 * CT_BUF, "score tile must fit in the chunk buffers it aliases");

__global__ __launch_bounds__(256) void inv_norm_kernel(const float* __restrict__ x, int ld, int n, int D, float* __restrict__ inv) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  const float* p = x + (long long)row * ld;
  float s = 0.f;
  for (int c = 2 * lane; c < D; c += 128) {
    const float2 v = *reinterpret_cast<const float2*>(p + c);
    s = fmaf(v.x, v.x, s);
    s = fmaf(v.y, v.y, s);
  }
  s = rsp_wave_sum(s);
  if (lane == 0) inv[row] = s > 0.f ? 1.f / sqrtf(s) : 0.f;
}

// Insert (s, i) into the wave's sorted list (lane j = rank j, j < k).  Entries already in the list that are >= s stay ahead:
// the caller inserts in ascending gallery index order, so on an exact tie the lower index stays first.
__device__ __forceinline__ bool list_insert(float& tv, int& ti, float s, int i, unsigned long long kmask, int lane) {
  const int pos = __popcll(__ballot(tv >= s) & kmask);
  if (pos >= __popcll(kmask)) return false;
  const float uv = __shfl_up(tv, 1);
  const int ui = __shfl_up(ti, 1);
  if (lane > pos) {
    tv = uv;
    ti = ui;
  } else if (lane == pos) {
    tv = s;
    ti = i;
  }
  return true;
}

__global__ __launch_bounds__(256) void cos_topk_kernel(const float* __restrict__ q, int ldq, int Nq, const float* __restrict__ g,
                                                       int ldg, int Ng, int D, int k, int splits, const float* __restrict__ invq,
                                                       const float* __restrict__ invg, float* __restrict__ part_val,
                                                       int* __restrict__ part_idx) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l32 = lane & 31, h = lane >> 5;
  const int wq = wave >> 1, wg = wave & 1;
  const int q0 = blockIdx.x * CT_BQ;
  const int split = blockIdx.y;
  const int gtiles = (Ng + CT_BG - 1) / CT_BG;
  const int tile_lo = (int)((long long)split * gtiles / splits), tile_hi = (int)((long long)(split + 1) * gtiles / splits);
  const int nch = (D + CT_KC - 1) / CT_KC;
  const unsigned long long kmask = k >= 64 ? ~0ull : ((1ull << k) - 1ull);

  // running top-k of the wave's 16 queries (rows 16 * wave + r of the block), lane j = rank j
  float tv[16];
  int ti[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    tv[r] = -INFINITY;
    ti[r] = -1;
  }

  for (int tile = tile_lo; tile < tile_hi; ++tile) {
    const int g0 = tile * CT_BG;
    float2 rq[4], rg[8];
    auto load = [&](int kc) {
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int e = t + 256 * it, row = e >> 4, k2 = kc + 2 * (e & 15);
        rq[it] = (q0 + row < Nq && k2 < D) ? *reinterpret_cast<const float2*>(q + (long long)(q0 + row) * ldq + k2)
                                           : make_float2(0.f, 0.f);
      }
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int e = t + 256 * it, row = e >> 4, k2 = kc + 2 * (e & 15);
        rg[it] = (g0 + row < Ng && k2 < D) ? *reinterpret_cast<const float2*>(g + (long long)(g0 + row) * ldg + k2)
                                           : make_float2(0.f, 0.f);
      }
    };
    auto store = [&](float* buf) {
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int e = t + 256 * it;
        *reinterpret_cast<float2*>(buf + (e >> 4) * CT_LD + 2 * (e & 15)) = rq[it];
      }
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int e = t + 256 * it;
        *reinterpret_cast<float2*>(buf + (CT_BQ + (e >> 4)) * CT_LD + 2 * (e & 15)) = rg[it];
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
    for (int c = 0; c < nch; ++c) {
      const float* buf = sm + (c & 1) * CT_BUF;
      if (c + 1 < nch) load((c + 1) * CT_KC);
      const float* qa = buf + (32 * wq + l32) * CT_LD + 4 * h;
      const float* gb0 = buf + (CT_BQ + 64 * wg + l32) * CT_LD + 4 * h;
      const float* gb1 = gb0 + 32 * CT_LD;
      // lane half h takes k = 8m + 4h + j at step j of group m, for A and B alike: every k of the chunk once
#pragma unroll
      for (int m = 0; m < CT_KC / 8; ++m) {
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
      if (c + 1 < nch) store(sm + ((c + 1) & 1) * CT_BUF);
      __syncthreads();
    }

    // similarities into the score tile (aliases the chunk buffers: every wave passed the last chunk's barrier)
    {
      const int col0 = 64 * wg + l32, col1 = col0 + 32;
      const float ig0 = g0 + col0 < Ng ? invg[g0 + col0] : 0.f;
      const float ig1 = g0 + col1 < Ng ? invg[g0 + col1] : 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = 32 * wq + (e >> 2) * 8 + h * 4 + (e & 3);
        const float iq = q0 + row < Nq ? invq[q0 + row] : 0.f;
        sm[row * CT_SLD + col0] = g0 + col0 < Ng ? acc0[e] * iq * ig0 : -INFINITY;
        sm[row * CT_SLD + col1] = g0 + col1 < Ng ? acc1[e] * iq * ig1 : -INFINITY;
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float* srow = sm + (16 * wave + r) * CT_SLD;
      const float thr = __shfl(tv[r], k - 1);
      unsigned long long m0 = __ballot(srow[lane] > thr), m1 = __ballot(srow[lane + 64] > thr);
      while (m0) {
        const int j = __ffsll((long long)m0) - 1;
        m0 &= m0 - 1;
        list_insert(tv[r], ti[r], srow[j], g0 + j, kmask, lane);
      }
      while (m1) {
        const int j = __ffsll((long long)m1) - 1;
        m1 &= m1 - 1;
        list_insert(tv[r], ti[r], srow[64 + j], g0 + 64 + j, kmask, lane);
      }
    }
    __syncthreads();      // the next tile's first chunk overwrites the score tile
  }

#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = q0 + 16 * wave + r;
    if (row < Nq && lane < k) {
      const long long o = ((long long)split * Nq + row) * k + lane;
      part_val[o] = tv[r];
      part_idx[o] = ti[r];
    }
  }
}

__global__ __launch_bounds__(256) void cos_merge_kernel(const float* __restrict__ part_val, const int* __restrict__ part_idx,
                                                        int Nq, int k, int splits, int* __restrict__ idx, float* __restrict__ dist) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= Nq) return;
  const unsigned long long kmask = k >= 64 ? ~0ull : ((1ull << k) - 1ull);
  float tv = -INFINITY;
  int ti = -1;
  for (int s = 0; s < splits; ++s) {      // ascending gallery ranges: a tie with an earlier split's entry stays behind it
    const long long o = ((long long)s * Nq + row) * k;
    const float pv = lane < k ? part_val[o + lane] : -INFINITY;
    const int pi = lane < k ? part_idx[o + lane] : -1;
    for (int j = 0; j < k; ++j) {
      const int cj = __shfl(pi, j);
      if (cj < 0) break;                                                   // the split's list ends here
      if (!list_insert(tv, ti, __shfl(pv, j), cj, kmask, lane)) break;      // sorted: the rest of this list loses too
    }
  }
  if (lane < k) {
    idx[(long long)row * k + lane] = ti;
    dist[(long long)row * k + lane] = ti < 0 ? INFINITY : fminf(fmaxf(1.f - tv, 0.f), 2.f);
  }
}

struct KsArg {
  int ks[CT_MAX_KS];
};

__global__ __launch_bounds__(256) void topk_hits_kernel(const int* __restrict__ idx, int Nq, int k, const long long* __restrict__ yq,
                                                        const long long* __restrict__ yg, int Ng, KsArg ks, int nks,
                                                        int* __restrict__ counts) {
  __shared__ int sc[CT_MAX_KS];
  if (threadIdx.x < CT_MAX_KS) sc[threadIdx.x] = 0;
  __syncthreads();
  int local[CT_MAX_KS];
#pragma unroll
  for (int i = 0; i < CT_MAX_KS; ++i) local[i] = 0;
  for (int row = threadIdx.x; row < Nq; row += blockDim.x) {
    const long long label = yq[row];
    int first = k;
    for (int j = 0; j < k; ++j) {
      const int gi = idx[(long long)row * k + j];
      if (gi >= 0 && gi < Ng && yg[gi] == label) {
        first = j;
        break;
      }
    }
#pragma unroll
    for (int i = 0; i < CT_MAX_KS; ++i) local[i] += (i < nks && first < ks.ks[i]) ? 1 : 0;
  }
#pragma unroll
  for (int i = 0; i < CT_MAX_KS; ++i)
    if (i < nks) atomicAdd(&sc[i], local[i]);      // integer sums: order-free
  __syncthreads();
  if (threadIdx.x < nks) counts[threadIdx.x] = sc[threadIdx.x];
}

size_t lds_bytes() { return (size_t)2 * CT_BUF * sizeof(float); }

}  // namespace

int32_t rsp_cosine_topk_splits(int32_t Nq, int32_t Ng, int32_t splits) {
  if (Nq <= 0 || Ng <= 0) return 1;
  const int qtiles = rsp_cdiv(Nq, CT_BQ), gtiles = rsp_cdiv(Ng, CT_BG);
  // default: about 2048 blocks (8 per CU) for an even last round, at least 8 gallery tiles per split
  int s = splits > 0 ? splits : rsp_cdiv(2048, qtiles);
  if (splits <= 0 && s > gtiles / 8) s = gtiles / 8;
  if (s > gtiles) s = gtiles;
  return s < 1 ? 1 : s;
}

size_t rsp_cosine_topk_workspace(int32_t Nq, int32_t Ng, int32_t D, int32_t k, int32_t splits) {
  (void)D;
  if (Nq <= 0 || Ng <= 0 || k <= 0) return 0;
  const int s = rsp_cosine_topk_splits(Nq, Ng, splits);
  return rsp_align_up((size_t)(Nq + Ng) * sizeof(float), 256) + (size_t)s * Nq * k * (sizeof(float) + sizeof(int32_t));
}

int rsp_cosine_topk(const float* q, int32_t ldq, int32_t Nq, const float* g, int32_t ldg, int32_t Ng, int32_t D, int32_t k,
                    int32_t splits, int32_t* idx, float* dist, void* workspace, size_t workspace_bytes, void* stream) {
  RSP_REQUIRE(q && g && idx && dist && workspace, "rsp_cosine_topk: null pointer");
  RSP_REQUIRE(Nq > 0 && Ng > 0 && D > 0 && D % 2 == 0 && ldq >= D && ldg >= D && ldq % 2 == 0 && ldg % 2 == 0,
              "rsp_cosine_topk: bad size (D and the leading dimensions must be even, ld >= D)");
  RSP_REQUIRE(k >= 1 && k <= CT_MAXK, "rsp_cosine_topk: k must be in [1, 64]");
  RSP_REQUIRE((((uintptr_t)q) & 7) == 0 && (((uintptr_t)g) & 7) == 0, "rsp_cosine_topk: q / g must be 8-byte aligned");
  if (workspace_bytes < rsp_cosine_topk_workspace(Nq, Ng, D, k, splits)) {
    rsp_set_error("rsp_cosine_topk: workspace too small");
    return RSP_EWORKSPACE;
  }
  const int S = rsp_cosine_topk_splits(Nq, Ng, splits);
  float* invq = reinterpret_cast<float*>(workspace);
  float* invg = invq + Nq;
  char* part = reinterpret_cast<char*>(workspace) + rsp_align_up((size_t)(Nq + Ng) * sizeof(float), 256);
  float* part_val = reinterpret_cast<float*>(part);
  int* part_idx = reinterpret_cast<int*>(part + (size_t)S * Nq * k * sizeof(float));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(inv_norm_kernel, dim3(rsp_cdiv(Nq, 4)), dim3(256), 0, s, q, ldq, Nq, D, invq);
  int rc = rsp_check_launch("inv_norm_kernel");
  if (rc != RSP_OK) return rc;
  hipLaunchKernelGGL(inv_norm_kernel, dim3(rsp_cdiv(Ng, 4)), dim3(256), 0, s, g, ldg, Ng, D, invg);
  rc = rsp_check_launch("inv_norm_kernel");
  if (rc != RSP_OK) return rc;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&cos_topk_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds_bytes());
    attr_set = true;
  }
  hipLaunchKernelGGL(cos_topk_kernel, dim3(rsp_cdiv(Nq, CT_BQ), S), dim3(256), lds_bytes(), s, q, ldq, Nq, g, ldg, Ng, D, k, S,
                     invq, invg, part_val, part_idx);
  rc = rsp_check_launch("cos_topk_kernel");
  if (rc != RSP_OK) return rc;
  hipLaunchKernelGGL(cos_merge_kernel, dim3(rsp_cdiv(Nq, 4)), dim3(256), 0, s, part_val, part_idx, Nq, k, S, idx, dist);
  return rsp_check_launch("cos_merge_kernel");
}

int rsp_topk_hits(const int32_t* idx, int32_t Nq, int32_t k, const int64_t* y_q, const int64_t* y_g, int32_t Ng,
                  const int32_t* ks_host, int32_t nks, int32_t* counts, void* stream) {
  RSP_REQUIRE(idx && y_q && y_g && ks_host && counts, "rsp_topk_hits: null pointer");
  RSP_REQUIRE(Nq > 0 && Ng > 0 && k >= 1 && nks >= 1 && nks <= CT_MAX_KS, "rsp_topk_hits: bad size (1 <= len(ks) <= 16)");
  KsArg ks = {};
  for (int i = 0; i < nks; ++i) {
    RSP_REQUIRE(ks_host[i] >= 1 && ks_host[i] <= k, "rsp_topk_hits: every k of ks must be in [1, columns of idx]");
    ks.ks[i] = ks_host[i];
  }
  hipLaunchKernelGGL(topk_hits_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, idx, Nq, k,
                     reinterpret_cast<const long long*>(y_q), reinterpret_cast<const long long*>(y_g), Ng, ks, nks, counts);
  return rsp_check_launch("topk_hits_kernel");
}
