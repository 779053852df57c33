// Cosine top-k search: for every query row the k (1..256) nearest gallery rows by cosine similarity, as per-split sorted lists in
// the workspace, without ever materialising the Nq x Ng matrix.  rsp_cosine_topk (retrieval.hip) and rsp_knn_classify (knn.hip) run
// it and merge the lists in a kernel of their own.
//
// Ranking rule: similarity s = (q.g) * (1/|q|) * (1/|g|) in fp32 (a zero-norm row has inverse norm 0, so s = 0 and distance 1,
// as sklearn's normalize leaves such a row zero); rows are ranked by s descending, an exact tie goes to the LOWER gallery index.
// That is a total order, so the result is unique: every split of the gallery computes the same s for the same pair (same
// k order of the dot product) and the merge of the per-split lists by the same order gives the same list for any split count.
//
// Kernels:
//   inv_norm_kernel      one wave per row: 1/|x| of the query and gallery rows, into the workspace; 0 for a row that is not valid (sum
//                        of squares finite and > 0) -- the flag rsp_repr_stats, rsp_kmeans_fit and rsp_tsne_affinities select by
//                        (rsp_inv_norms).
//   cos_topk_kernel<S, K1>   block = 64 queries x one gallery split.  Per gallery tile of 128 rows the 4 waves (2 x 2, 32 x 64 each)
//                        accumulate the dot products on v_mfma_f32_32x32x2_f32 from LDS chunks of 32 k (register prefetch of the
//                        next chunk, double-buffered LDS), scale them to similarities into an LDS score tile (aliasing the chunk
//                        buffers), and each wave updates the running top-k of 16 queries: its lists live in registers (16 x S x 2
//                        VGPRs, S = ceil(k / 64), cos_search.h); tile scores above the current k-th best are inserted in ascending
//                        gallery order (ballot + shift), which keeps the tie rule.  The split's list goes to the workspace.
//                        K1 (k = 1: the assignment step of rsp_kmeans_fit, and any search for one neighbour): the insertion is
//                        replaced by the wave's arg-max of the tile (lower index on a tie), the same entry at a fraction of the cost.
#include "cos_search.h"

namespace {

constexpr int CS_BQ = 64;              // queries per block
constexpr int CS_BG = 128;             // gallery rows per tile
constexpr int CS_KC = 32;              // k per LDS chunk
constexpr int CS_LD = CS_KC + 4;       // LDS row pitch (floats) of a chunk
constexpr int CS_SLD = CS_BG + 4;      // LDS row pitch (floats) of the score tile
constexpr int CS_BUF = (CS_BQ + CS_BG) * CS_LD;      // floats per chunk buffer
constexpr size_t CS_LDS_BYTES = (size_t)2 * CS_BUF * sizeof(float);

static_assert(CS_BQ * CS_SLD <= 2 * CS_BUF, "score tile must fit in the chunk buffers it aliases");

// stop (here and in cos_topk_kernel): nullptr, or a device flag that makes the whole launch return at once when it is not 0 (the
// iterations rsp_kmeans_fit issues past its device-side stop).
__global__ __launch_bounds__(256) void inv_norm_kernel(const float* __restrict__ x, int ld, int n, int D, float* __restrict__ inv,
                                                       const int* __restrict__ stop) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n || (stop && *stop)) return;
  const float s = rsp_row_sumsq(x + (long long)row * ld, D, lane);
  if (lane == 0) inv[row] = (s > 0.f && s < INFINITY) ? 1.f / sqrtf(s) : 0.f;      // (a NaN fails both comparisons)
}

template <int S, bool K1>
__global__ __launch_bounds__(256) void cos_topk_kernel(const float* __restrict__ q, int ldq, int Nq, const float* __restrict__ g,
                                                       int ldg, int Ng, int D, int k, int splits, const float* __restrict__ invq,
                                                       const float* __restrict__ invg, float* __restrict__ part_val,
                                                       int* __restrict__ part_idx, const int* __restrict__ stop) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  if (stop && *stop) return;      // (the whole block, before any barrier)
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l32 = lane & 31, h = lane >> 5;
  const int wq = wave >> 1, wg = wave & 1;
  const int q0 = blockIdx.x * CS_BQ;
  const int split = blockIdx.y;
  const int gtiles = (Ng + CS_BG - 1) / CS_BG;
  const int tile_lo = (int)((long long)split * gtiles / splits), tile_hi = (int)((long long)(split + 1) * gtiles / splits);
  const int nch = (D + CS_KC - 1) / CS_KC;
  const unsigned long long kmask = last_slot_mask(k, S);

  // running top-k of the wave's 16 queries (rows 16 * wave + r of the block)
  float tv[16][S];
  int ti[16][S];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
#pragma unroll
    for (int sl = 0; sl < S; ++sl) {
      tv[r][sl] = -INFINITY;
      ti[r][sl] = -1;
    }
  }

  for (int tile = tile_lo; tile < tile_hi; ++tile) {
    const int g0 = tile * CS_BG;
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
        *reinterpret_cast<float2*>(buf + (e >> 4) * CS_LD + 2 * (e & 15)) = rq[it];
      }
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int e = t + 256 * it;
        *reinterpret_cast<float2*>(buf + (CS_BQ + (e >> 4)) * CS_LD + 2 * (e & 15)) = rg[it];
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
      const float* buf = sm + (c & 1) * CS_BUF;
      if (c + 1 < nch) load((c + 1) * CS_KC);
      const float* qa = buf + (32 * wq + l32) * CS_LD + 4 * h;
      const float* gb0 = buf + (CS_BQ + 64 * wg + l32) * CS_LD + 4 * h;
      const float* gb1 = gb0 + 32 * CS_LD;
      // lane half h takes k = 8m + 4h + j at step j of group m, for A and B alike: every k of the chunk once
#pragma unroll
      for (int m = 0; m < CS_KC / 8; ++m) {
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
      if (c + 1 < nch) store(sm + ((c + 1) & 1) * CS_BUF);
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
        sm[row * CS_SLD + col0] = g0 + col0 < Ng ? acc0[e] * iq * ig0 : -INFINITY;
        sm[row * CS_SLD + col1] = g0 + col1 < Ng ? acc1[e] * iq * ig1 : -INFINITY;
      }
    }
    __syncthreads();
    if constexpr (K1) {
      // k = 1: the tile's maximum of each query by the whole wave -- the lower index on a tie, a NaN or -inf score is no candidate --
      // taken only when strictly greater than the running one: the entry the insertion below leaves in a one-entry list
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float* srow = sm + (16 * wave + r) * CS_SLD;
        const float v0 = srow[lane], v1 = srow[lane + 64];
        float bv = v0 == v0 ? v0 : -INFINITY;
        int bj = lane;
        if (v1 > bv) {
          bv = v1;
          bj = lane + 64;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const float ov = __shfl_xor(bv, o);
          const int oj = __shfl_xor(bj, o);
          if (ov > bv || (ov == bv && oj < bj)) {
            bv = ov;
            bj = oj;
          }
        }
        if (bv > tv[r][0]) {
          tv[r][0] = bv;
          ti[r][0] = g0 + bj;
        }
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float* srow = sm + (16 * wave + r) * CS_SLD;
        const float thr = __shfl(tv[r][S - 1], k - 1 - 64 * (S - 1));      // the current k-th best (a NaN score never passes)
        unsigned long long m0 = __ballot(srow[lane] > thr), m1 = __ballot(srow[lane + 64] > thr);
        while (m0) {
          const int j = __ffsll((long long)m0) - 1;
          m0 &= m0 - 1;
          list_insert<S>(tv[r], ti[r], srow[j], g0 + j, k, kmask, lane);
        }
        while (m1) {
          const int j = __ffsll((long long)m1) - 1;
          m1 &= m1 - 1;
          list_insert<S>(tv[r], ti[r], srow[64 + j], g0 + 64 + j, k, kmask, lane);
        }
      }
    }
    __syncthreads();      // the next tile's first chunk overwrites the score tile
  }

#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = q0 + 16 * wave + r;
#pragma unroll
    for (int sl = 0; sl < S; ++sl) {
      const int rk = 64 * sl + lane;
      if (row < Nq && rk < k) {
        const long long o = ((long long)split * Nq + row) * k + rk;
        part_val[o] = tv[r][sl];
        part_idx[o] = ti[r][sl];
      }
    }
  }
}

template <int S, bool K1 = false>
int launch_search(const float* q, int ldq, int Nq, const float* g, int ldg, int Ng, int D, int k, int splits, const float* invq,
                  const float* invg, float* part_val, int* part_idx, const int* stop, hipStream_t s) {
  static bool attr_set = false;      // the instance's own: its dynamic LDS exceeds the default limit
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&cos_topk_kernel<S, K1>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)CS_LDS_BYTES);
    attr_set = true;
  }
  hipLaunchKernelGGL((cos_topk_kernel<S, K1>), dim3(rsp_cdiv(Nq, CS_BQ), splits), dim3(256), CS_LDS_BYTES, s, q, ldq, Nq, g, ldg, Ng, D, k,
                     splits, invq, invg, part_val, part_idx, stop);
  return rsp_check_launch("cos_topk_kernel");
}

int fail(const char* who, const char* what, int code) {
  char buf[160];
  snprintf(buf, sizeof buf, "%s: %s", who, what);
  rsp_set_error(buf);
  return code;
}

}  // namespace

int32_t rsp_cosine_topk_splits(int32_t Nq, int32_t Ng, int32_t splits) {
  if (Nq <= 0 || Ng <= 0) return 1;
  const int qtiles = rsp_cdiv(Nq, CS_BQ), gtiles = rsp_cdiv(Ng, CS_BG);
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

int rsp_cos_search_check(const char* who, const float* q, int ldq, int Nq, const float* g, int ldg, int Ng, int D, int k, int kmax) {
  if (!(Nq > 0 && Ng > 0 && D > 0 && D % 2 == 0 && ldq >= D && ldg >= D && ldq % 2 == 0 && ldg % 2 == 0))
    return fail(who, "bad size (D and the leading dimensions must be even, ld >= D)", RSP_EINVAL);
  if (!(k >= 1 && k <= kmax)) {
    char what[48];
    snprintf(what, sizeof what, "k must be in [1, %d]", kmax);
    return fail(who, what, RSP_EINVAL);
  }
  if ((((uintptr_t)q) & 7) != 0 || (((uintptr_t)g) & 7) != 0) return fail(who, "q / g must be 8-byte aligned", RSP_EINVAL);
  return RSP_OK;
}

int rsp_inv_norms(const float* x, int ld, int n, int D, float* inv, const int* stop, hipStream_t s) {
  hipLaunchKernelGGL(inv_norm_kernel, dim3(rsp_cdiv(n, 4)), dim3(256), 0, s, x, ld, n, D, inv, stop);
  return rsp_check_launch("inv_norm_kernel");
}

int rsp_cos_search(const char* who, const float* q, int ldq, int Nq, const float* g, int ldg, int Ng, int D, int k, int splits,
                   void* workspace, size_t workspace_bytes, hipStream_t s, CosLists* lists) {
  return rsp_cos_search_gated(who, q, ldq, Nq, g, ldg, Ng, D, k, splits, workspace, workspace_bytes, s, lists, nullptr, true);
}

int rsp_cos_search_gated(const char* who, const float* q, int ldq, int Nq, const float* g, int ldg, int Ng, int D, int k, int splits,
                         void* workspace, size_t workspace_bytes, hipStream_t s, CosLists* lists, const int* stop, bool norm_q) {
  if (workspace_bytes < rsp_cosine_topk_workspace(Nq, Ng, D, k, splits)) return fail(who, "workspace too small", RSP_EWORKSPACE);
  splits = rsp_cosine_topk_splits(Nq, Ng, splits);
  float* invq = reinterpret_cast<float*>(workspace);
  float* invg = invq + Nq;
  char* part = reinterpret_cast<char*>(workspace) + rsp_align_up((size_t)(Nq + Ng) * sizeof(float), 256);
  lists->val = reinterpret_cast<float*>(part);
  lists->idx = reinterpret_cast<int*>(part + (size_t)splits * Nq * k * sizeof(float));
  lists->splits = splits;
  lists->inv_q = invq;
  lists->inv_g = invg;
  int rc = norm_q ? rsp_inv_norms(q, ldq, Nq, D, invq, stop, s) : RSP_OK;
  if (rc != RSP_OK) return rc;
  rc = rsp_inv_norms(g, ldg, Ng, D, invg, stop, s);
  if (rc != RSP_OK) return rc;
  if (k == 1) return launch_search<1, true>(q, ldq, Nq, g, ldg, Ng, D, k, splits, invq, invg, lists->val, lists->idx, stop, s);
  switch (rsp_cdiv(k, 64)) {
    case 1: return launch_search<1>(q, ldq, Nq, g, ldg, Ng, D, k, splits, invq, invg, lists->val, lists->idx, stop, s);
    case 2: return launch_search<2>(q, ldq, Nq, g, ldg, Ng, D, k, splits, invq, invg, lists->val, lists->idx, stop, s);
    case 3: return launch_search<3>(q, ldq, Nq, g, ldg, Ng, D, k, splits, invq, invg, lists->val, lists->idx, stop, s);
    default: return launch_search<4>(q, ldq, Nq, g, ldg, Ng, D, k, splits, invq, invg, lists->val, lists->idx, stop, s);
  }
}
