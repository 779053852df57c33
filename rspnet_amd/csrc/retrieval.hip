// Video retrieval search (the search half of the reference's retrieval.py:150-176): for every query row the k nearest gallery
// rows by cosine distance, without ever materialising the Nq x Ng distance matrix, and the top-k hit counts from the result.
//
// The search, its ranking rule (similarity in fp32 descending, an exact tie to the LOWER gallery index, the same list for any split
// count) and the sorted list of a wave are cos_search.hip's and cos_search.h's; rsp_cosine_topk runs it with one list slot per lane.
//
// Kernels:
//   cos_merge_kernel   one wave per query: merges the split lists in split order by the search's insertion, writes indices and
//                      distances clip(1 - s, 0, 2); empty slots (Ng < k) get index -1 and distance +inf.
//   topk_hits_kernel   one block: per query the first rank whose gallery label equals the query's label, counted per k.
#include "cos_search.h"

namespace {

constexpr int CT_MAXK = 64;
constexpr int CT_MAX_KS = 16;

__global__ __launch_bounds__(256) void cos_merge_kernel(const float* __restrict__ part_val, const int* __restrict__ part_idx,
                                                        int Nq, int k, int splits, int* __restrict__ idx, float* __restrict__ dist) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= Nq) return;
  float tv[1];
  int ti[1];
  merge_lists<1>(tv, ti, part_val, part_idx, Nq, row, k, splits, lane);
  store_list<1>(tv, ti, row, k, lane, idx, dist);
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

}  // namespace

int rsp_cosine_topk(const float* q, int32_t ldq, int32_t Nq, const float* g, int32_t ldg, int32_t Ng, int32_t D, int32_t k,
                    int32_t splits, int32_t* idx, float* dist, void* workspace, size_t workspace_bytes, void* stream) {
  RSP_REQUIRE(q && g && idx && dist && workspace, "rsp_cosine_topk: null pointer");
  int rc = rsp_cos_search_check("rsp_cosine_topk", q, ldq, Nq, g, ldg, Ng, D, k, CT_MAXK);
  if (rc != RSP_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  CosLists part;
  rc = rsp_cos_search("rsp_cosine_topk", q, ldq, Nq, g, ldg, Ng, D, k, splits, workspace, workspace_bytes, s, &part);
  if (rc != RSP_OK) return rc;
  hipLaunchKernelGGL(cos_merge_kernel, dim3(rsp_cdiv(Nq, 4)), dim3(256), 0, s, part.val, part.idx, Nq, k, part.splits, idx, dist);
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
