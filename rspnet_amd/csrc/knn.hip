// Weighted kNN classifier of instance discrimination (the monitor of a pretext run): for every query row the k (1..256) nearest
// gallery rows by cosine similarity, a per-class vote with weights exp((s - 1) / T), the predicted class, the rank of the
// query's own class and the top-1 / top-5 hit counts -- one call, the Nq x Ng matrix never stored.
//
// The neighbours are the search's (cos_search.hip, the one rsp_cosine_topk runs): s = (q.g) * (1/|q|) * (1/|g|) in fp32, descending,
// an exact tie to the LOWER gallery index, the same list for any split count; here with S = ceil(k / 64) list slots per lane.
//
// Kernels:
//   knn_vote_kernel<S>     one wave per query, four per block: merges the split lists in ascending gallery order by the search's
//                          insertion, writes idx / dist when asked, then votes.  Lane l owns classes l, l + 64, ... of the wave's
//                          num_classes floats of LDS; the neighbours are walked in rank order, label and weight broadcast from the
//                          lane that holds the rank, and the owner lane adds: fp32 sums in rank order, no atomics, every LDS word
//                          only ever touched by its owner lane.  Two wave reductions give pred and rank.
//   knn_hits_kernel        one block: hits[0] / hits[1] = rows i < valid with rank[i] < 1 / < 5 (integer adds).
#include "cos_search.h"

namespace {

constexpr int KN_MAXC = 1024;

template <int S>
__global__ __launch_bounds__(256) void knn_vote_kernel(const float* __restrict__ part_val, const int* __restrict__ part_idx, int Nq,
                                                       int Ng, int k, int splits, const long long* __restrict__ yg,
                                                       const long long* __restrict__ yq, float inv_T, int C, int* __restrict__ idx,
                                                       float* __restrict__ dist, float* __restrict__ votes, int* __restrict__ pred,
                                                       int* __restrict__ rank) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= Nq) return;      // a whole wave: no block-level barrier below
  float* v = sm + (threadIdx.x >> 6) * C;      // the wave's votes; word c only ever touched by lane c % 64
  float tv[S];
  int ti[S];
  merge_lists<S>(tv, ti, part_val, part_idx, Nq, row, k, splits, lane);
  if (idx) store_list<S>(tv, ti, row, k, lane, idx, dist);

  // label (-1: no vote) and weight of the ranks this lane holds
  int lab[S];
  float wt[S];
#pragma unroll
  for (int sl = 0; sl < S; ++sl) {
    const int rk = 64 * sl + lane;
    const bool has = rk < k && ti[sl] >= 0 && ti[sl] < Ng;
    const long long y = has ? yg[ti[sl]] : -1;
    lab[sl] = (y >= 0 && y < C) ? (int)y : -1;
    wt[sl] = has ? expf((tv[sl] - 1.f) * inv_T) : 0.f;
  }
  for (int c = lane; c < C; c += 64) v[c] = 0.f;
#pragma unroll
  for (int sl = 0; sl < S; ++sl) {
    const int n = min(64, k - 64 * sl);
    for (int j = 0; j < n; ++j) {      // rank order, rank 0 first
      const int l = __shfl(lab[sl], j);
      const float w = __shfl(wt[sl], j);
      if (l >= 0 && (l & 63) == lane) v[l] += w;
    }
  }

  // pred: the largest vote, an exact tie to the lower class
  float bv = -1.f;
  int bc = 0x7fffffff;
  for (int c = lane; c < C; c += 64) {
    const float x = v[c];
    if (x > bv) {
      bv = x;
      bc = c;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o);
    const int oc = __shfl_xor(bc, o);
    if (ov > bv || (ov == bv && oc < bc)) {
      bv = ov;
      bc = oc;
    }
  }
  if (lane == 0) pred[row] = bc;
  if (votes)
    for (int c = lane; c < C; c += 64) votes[(long long)row * C + c] = v[c];
  if (yq) {
    const long long t = yq[row];
    int r = C;      // a label outside [0, C): a miss
    if (t >= 0 && t < C) {
      const int tc = (int)t;
      const float vt = __shfl(lane == (tc & 63) ? v[tc] : 0.f, tc & 63);
      int n = 0;
      for (int c = lane; c < C; c += 64) {
        const float x = v[c];
        n += (x > vt || (x == vt && c < tc)) ? 1 : 0;
      }
      r = rsp_wave_sum_i(n);
    }
    if (lane == 0) rank[row] = r;
  }
}

__global__ __launch_bounds__(256) void knn_hits_kernel(const int* __restrict__ rank, int valid, int* __restrict__ hits) {
  __shared__ int sc[2];
  if (threadIdx.x < 2) sc[threadIdx.x] = 0;
  __syncthreads();
  int h1 = 0, h5 = 0;
  for (int i = threadIdx.x; i < valid; i += blockDim.x) {
    const int r = rank[i];
    h1 += r < 1 ? 1 : 0;
    h5 += r < 5 ? 1 : 0;
  }
  atomicAdd(&sc[0], h1);      // integer sums: order-free
  atomicAdd(&sc[1], h5);
  __syncthreads();
  if (threadIdx.x < 2) hits[threadIdx.x] = sc[threadIdx.x];
}

template <int S>
int launch_vote(const CosLists& part, int Nq, int Ng, int k, const int64_t* y_g, const int64_t* y_q, float inv_T, int C, int* idx,
                float* dist, float* votes, int* pred, int* rank, hipStream_t s) {
  hipLaunchKernelGGL(knn_vote_kernel<S>, dim3(rsp_cdiv(Nq, 4)), dim3(256), (size_t)4 * C * sizeof(float), s, part.val, part.idx, Nq, Ng,
                     k, part.splits, reinterpret_cast<const long long*>(y_g), reinterpret_cast<const long long*>(y_q), inv_T, C, idx,
                     dist, votes, pred, rank);
  return rsp_check_launch("knn_vote_kernel");
}

}  // namespace

size_t rsp_knn_classify_workspace(int32_t Nq, int32_t Ng, int32_t D, int32_t k, int32_t num_classes, int32_t splits) {
  (void)num_classes;      // the votes live in LDS
  return rsp_cosine_topk_workspace(Nq, Ng, D, k, splits);
}

int rsp_knn_classify(const float* q, int32_t ldq, int32_t Nq, const int64_t* y_q, const float* g, int32_t ldg, int32_t Ng,
                     const int64_t* y_g, int32_t D, int32_t k, float T, int32_t num_classes, int32_t splits, int32_t valid,
                     int32_t* idx, float* dist, float* votes, int32_t* pred, int32_t* rank, int32_t* hits, void* workspace,
                     size_t workspace_bytes, void* stream) {
  RSP_REQUIRE(q && g && y_g && pred && workspace, "rsp_knn_classify: null pointer");
  int rc = rsp_cos_search_check("rsp_knn_classify", q, ldq, Nq, g, ldg, Ng, D, k, COS_SEARCH_MAXK);
  if (rc != RSP_OK) return rc;
  RSP_REQUIRE(num_classes >= 1 && num_classes <= KN_MAXC, "rsp_knn_classify: num_classes must be in [1, 1024]");
  RSP_REQUIRE(isfinite(T) && T >= 0.01f, "rsp_knn_classify: T must be finite and >= 0.01");
  RSP_REQUIRE((idx == nullptr) == (dist == nullptr), "rsp_knn_classify: idx and dist go together");
  RSP_REQUIRE((rank != nullptr) == (y_q != nullptr), "rsp_knn_classify: rank is required with y_q and only with it");
  RSP_REQUIRE(!hits || y_q, "rsp_knn_classify: hits needs y_q");
  RSP_REQUIRE(valid >= 0 && valid <= Nq, "rsp_knn_classify: valid must be in [0, Nq]");
  hipStream_t s = (hipStream_t)stream;
  CosLists part;
  rc = rsp_cos_search("rsp_knn_classify", q, ldq, Nq, g, ldg, Ng, D, k, splits, workspace, workspace_bytes, s, &part);
  if (rc != RSP_OK) return rc;
  const float inv_T = 1.f / T;
  switch (rsp_cdiv(k, 64)) {
    case 1: rc = launch_vote<1>(part, Nq, Ng, k, y_g, y_q, inv_T, num_classes, idx, dist, votes, pred, rank, s); break;
    case 2: rc = launch_vote<2>(part, Nq, Ng, k, y_g, y_q, inv_T, num_classes, idx, dist, votes, pred, rank, s); break;
    case 3: rc = launch_vote<3>(part, Nq, Ng, k, y_g, y_q, inv_T, num_classes, idx, dist, votes, pred, rank, s); break;
    default: rc = launch_vote<4>(part, Nq, Ng, k, y_g, y_q, inv_T, num_classes, idx, dist, votes, pred, rank, s); break;
  }
  if (rc != RSP_OK || !hits) return rc;
  hipLaunchKernelGGL(knn_hits_kernel, dim3(1), dim3(256), 0, s, rank, valid, hits);
  return rsp_check_launch("knn_hits_kernel");
}
