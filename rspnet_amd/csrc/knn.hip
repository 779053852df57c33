// Weighted kNN classifier of instance discrimination (the monitor of a pretext run): for every query row the k (1..256) nearest
// gallery rows by cosine similarity, a per-class vote with weights exp((s - 1) / T), the predicted class, the rank of the
// query's own class and the top-1 / top-5 hit counts -- one call, the Nq x Ng matrix never stored.
//
// Similarity and ranking are rsp_cosine_topk's (retrieval.hip): s = (q.g) * (1/|q|) * (1/|g|) in fp32, descending, an exact tie
// to the LOWER gallery index; the same dot-product order in every split, so the list does not depend on the split count.  The
// search kernels here are copies of retrieval.hip's with the per-query list widened from one register slot per lane to S =
// ceil(k / 64): rank r lives in slot r / 64, lane r % 64.  S = 1 is retrieval.hip's code, statement for statement.
//
// Kernels:
//   knn_inv_norm_kernel    one wave per row: 1/|x| (0 for a zero row).
//   knn_topk_kernel<S>     block = 64 queries x one gallery split; fp32 MFMA on double-buffered LDS chunks, the score tile aliasing
//                          the chunk buffers, each wave keeps the running lists of 16 queries in registers (16 x S x 2 VGPRs).
//   knn_vote_kernel<S>     one wave per query, four per block: merges the split lists in ascending gallery order by the same
//                          insertion, writes idx / dist when asked, then votes.  Lane l owns classes l, l + 64, ... of the wave's
//                          num_classes floats of LDS; the neighbours are walked in rank order, label and weight broadcast from the
//                          lane that holds the rank, and the owner lane adds: fp32 sums in rank order, no atomics, every LDS word
//                          only ever touched by its owner lane.  Two wave reductions give pred and rank.
//   knn_hits_kernel        one block: hits[0] / hits[1] = rows i < valid with rank[i] < 1 / < 5 (integer adds).
#include "common.h"

#include <math.h>

namespace {

constexpr int KN_BQ = 64;              // queries per block
constexpr int KN_BG = 128;             // gallery rows per tile
constexpr int KN_KC = 32;              // k per LDS chunk
constexpr int KN_LD = KN_KC + 4;       // LDS row pitch (floats) of a chunk
constexpr int KN_SLD = KN_BG + 4;      // LDS row pitch (floats) of the score tile
constexpr int KN_BUF = (KN_BQ + KN_BG) * KN_LD;      // floats per chunk buffer
constexpr int KN_MAXK = 256;
constexpr int KN_MAXC = 1024;

static_assert(KN_BQ * KN_SLD <= 2 * KN_BUF, "score tile must fit in the chunk buffers it aliases");

__global__ __launch_bounds__(256) void knn_inv_norm_kernel(const float* __restrict__ x, int ld, int n, int D, float* __restrict__ inv) {
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

// Insert (s, i) into the wave's sorted list of k entries (rank r = slot r / 64, lane r % 64).  Entries already in the list that
// are >= s stay ahead: the caller inserts in ascending gallery index order, so on an exact tie the lower index stays first.
// kmask: the lanes of the LAST slot that belong to the list (the slots below it are full).
template <int S>
__device__ __forceinline__ bool list_insert(float (&tv)[S], int (&ti)[S], float s, int i, int k, unsigned long long kmask, int lane) {
  int pos = 0;
#pragma unroll
  for (int sl = 0; sl < S; ++sl) {
    const unsigned long long b = __ballot(tv[sl] >= s);
    pos += __popcll(sl == S - 1 ? (b & kmask) : b);
  }
  if (pos >= k) return false;
  float bv[S];      // lane 63 of the slot below, as it was before the shift
  int bi[S];
#pragma unroll
  for (int sl = 1; sl < S; ++sl) {
    bv[sl] = __shfl(tv[sl - 1], 63);
    bi[sl] = __shfl(ti[sl - 1], 63);
  }
#pragma unroll
  for (int sl = 0; sl < S; ++sl) {
    float uv = __shfl_up(tv[sl], 1);
    int ui = __shfl_up(ti[sl], 1);
    if (sl > 0 && lane == 0) {
      uv = bv[sl];
      ui = bi[sl];
    }
    const int r = 64 * sl + lane;
    if (r > pos) {
      tv[sl] = uv;
      ti[sl] = ui;
    } else if (r == pos) {
      tv[sl] = s;
      ti[sl] = i;
    }
  }
  return true;
}

__device__ __forceinline__ unsigned long long last_slot_mask(int k, int S) {
  const int n = k - 64 * (S - 1);
  return n >= 64 ? ~0ull : ((1ull << n) - 1ull);
}

template <int S>
__global__ __launch_bounds__(256) void knn_topk_kernel(const float* __restrict__ q, int ldq, int Nq, const float* __restrict__ g,
                                                       int ldg, int Ng, int D, int k, int splits, const float* __restrict__ invq,
                                                       const float* __restrict__ invg, float* __restrict__ part_val,
                                                       int* __restrict__ part_idx) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l32 = lane & 31, h = lane >> 5;
  const int wq = wave >> 1, wg = wave & 1;
  const int q0 = blockIdx.x * KN_BQ;
  const int split = blockIdx.y;
  const int gtiles = (Ng + KN_BG - 1) / KN_BG;
  const int tile_lo = (int)((long long)split * gtiles / splits), tile_hi = (int)((long long)(split + 1) * gtiles / splits);
  const int nch = (D + KN_KC - 1) / KN_KC;
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
    const int g0 = tile * KN_BG;
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
        *reinterpret_cast<float2*>(buf + (e >> 4) * KN_LD + 2 * (e & 15)) = rq[it];
      }
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int e = t + 256 * it;
        *reinterpret_cast<float2*>(buf + (KN_BQ + (e >> 4)) * KN_LD + 2 * (e & 15)) = rg[it];
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
      const float* buf = sm + (c & 1) * KN_BUF;
      if (c + 1 < nch) load((c + 1) * KN_KC);
      const float* qa = buf + (32 * wq + l32) * KN_LD + 4 * h;
      const float* gb0 = buf + (KN_BQ + 64 * wg + l32) * KN_LD + 4 * h;
      const float* gb1 = gb0 + 32 * KN_LD;
      // lane half h takes k = 8m + 4h + j at step j of group m, for A and B alike: every k of the chunk once
#pragma unroll
      for (int m = 0; m < KN_KC / 8; ++m) {
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
      if (c + 1 < nch) store(sm + ((c + 1) & 1) * KN_BUF);
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
        sm[row * KN_SLD + col0] = g0 + col0 < Ng ? acc0[e] * iq * ig0 : -INFINITY;
        sm[row * KN_SLD + col1] = g0 + col1 < Ng ? acc1[e] * iq * ig1 : -INFINITY;
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float* srow = sm + (16 * wave + r) * KN_SLD;
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

// One split's sorted list into the wave's list; false once an entry loses (sorted: the rest of that list loses too).
template <int S>
__device__ __forceinline__ void merge_split(float (&tv)[S], int (&ti)[S], const float* __restrict__ pv_, const int* __restrict__ pi_,
                                            int k, unsigned long long kmask, int lane) {
  float pv[S];
  int pi[S];
#pragma unroll
  for (int sl = 0; sl < S; ++sl) {
    const int rk = 64 * sl + lane;
    pv[sl] = rk < k ? pv_[rk] : -INFINITY;
    pi[sl] = rk < k ? pi_[rk] : -1;
  }
#pragma unroll
  for (int sl = 0; sl < S; ++sl) {
    const int n = min(64, k - 64 * sl);
    for (int j = 0; j < n; ++j) {
      const int cj = __shfl(pi[sl], j);
      if (cj < 0) return;                                                            // the split's list ends here
      if (!list_insert<S>(tv, ti, __shfl(pv[sl], j), cj, k, kmask, lane)) return;
    }
  }
}

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
  const unsigned long long kmask = last_slot_mask(k, S);
  float tv[S];
  int ti[S];
#pragma unroll
  for (int sl = 0; sl < S; ++sl) {
    tv[sl] = -INFINITY;
    ti[sl] = -1;
  }
  for (int s = 0; s < splits; ++s) {      // ascending gallery ranges: a tie with an earlier split's entry stays behind it
    const long long o = ((long long)s * Nq + row) * k;
    merge_split<S>(tv, ti, part_val + o, part_idx + o, k, kmask, lane);
  }
  if (idx) {
#pragma unroll
    for (int sl = 0; sl < S; ++sl) {
      const int rk = 64 * sl + lane;
      if (rk < k) {
        idx[(long long)row * k + rk] = ti[sl];
        dist[(long long)row * k + rk] = ti[sl] < 0 ? INFINITY : fminf(fmaxf(1.f - tv[sl], 0.f), 2.f);
      }
    }
  }

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
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
      r = n;
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

size_t topk_lds_bytes() { return (size_t)2 * KN_BUF * sizeof(float); }

struct Args {
  const float *q, *g;
  int ldq, Nq, ldg, Ng, D, k, splits, C;
  float inv_T;
  const long long *yq, *yg;
  float *invq, *invg, *part_val;
  int* part_idx;
  int* idx;
  float *dist, *votes;
  int *pred, *rank;
};

template <int S>
int launch_search_and_vote(const Args& a, hipStream_t s) {
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&knn_topk_kernel<S>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)topk_lds_bytes());
    attr_set = true;
  }
  hipLaunchKernelGGL(knn_topk_kernel<S>, dim3(rsp_cdiv(a.Nq, KN_BQ), a.splits), dim3(256), topk_lds_bytes(), s, a.q, a.ldq, a.Nq, a.g,
                     a.ldg, a.Ng, a.D, a.k, a.splits, a.invq, a.invg, a.part_val, a.part_idx);
  int rc = rsp_check_launch("knn_topk_kernel");
  if (rc != RSP_OK) return rc;
  hipLaunchKernelGGL(knn_vote_kernel<S>, dim3(rsp_cdiv(a.Nq, 4)), dim3(256), (size_t)4 * a.C * sizeof(float), s, a.part_val,
                     a.part_idx, a.Nq, a.Ng, a.k, a.splits, a.yg, a.yq, a.inv_T, a.C, a.idx, a.dist, a.votes, a.pred, a.rank);
  return rsp_check_launch("knn_vote_kernel");
}

}  // namespace

size_t rsp_knn_classify_workspace(int32_t Nq, int32_t Ng, int32_t D, int32_t k, int32_t num_classes, int32_t splits) {
  (void)D;
  (void)num_classes;
  if (Nq <= 0 || Ng <= 0 || k <= 0) return 0;
  const int s = rsp_cosine_topk_splits(Nq, Ng, splits);
  return rsp_align_up((size_t)(Nq + Ng) * sizeof(float), 256) + (size_t)s * Nq * k * (sizeof(float) + sizeof(int32_t));
}

int rsp_knn_classify(const float* q, int32_t ldq, int32_t Nq, const int64_t* y_q, const float* g, int32_t ldg, int32_t Ng,
                     const int64_t* y_g, int32_t D, int32_t k, float T, int32_t num_classes, int32_t splits, int32_t valid,
                     int32_t* idx, float* dist, float* votes, int32_t* pred, int32_t* rank, int32_t* hits, void* workspace,
                     size_t workspace_bytes, void* stream) {
  RSP_REQUIRE(q && g && y_g && pred && workspace, "rsp_knn_classify: null pointer");
  RSP_REQUIRE(Nq > 0 && Ng > 0 && D > 0 && D % 2 == 0 && ldq >= D && ldg >= D && ldq % 2 == 0 && ldg % 2 == 0,
              "rsp_knn_classify: bad size (D and the leading dimensions must be even, ld >= D)");
  RSP_REQUIRE(k >= 1 && k <= KN_MAXK, "rsp_knn_classify: k must be in [1, 256]");
  RSP_REQUIRE(num_classes >= 1 && num_classes <= KN_MAXC, "rsp_knn_classify: num_classes must be in [1, 1024]");
  RSP_REQUIRE(isfinite(T) && T >= 0.01f, "rsp_knn_classify: T must be finite and >= 0.01");
  RSP_REQUIRE((((uintptr_t)q) & 7) == 0 && (((uintptr_t)g) & 7) == 0, "rsp_knn_classify: q / g must be 8-byte aligned");
  RSP_REQUIRE((idx == nullptr) == (dist == nullptr), "rsp_knn_classify: idx and dist go together");
  RSP_REQUIRE((rank != nullptr) == (y_q != nullptr), "rsp_knn_classify: rank is required with y_q and only with it");
  RSP_REQUIRE(!hits || y_q, "rsp_knn_classify: hits needs y_q");
  RSP_REQUIRE(valid >= 0 && valid <= Nq, "rsp_knn_classify: valid must be in [0, Nq]");
  if (workspace_bytes < rsp_knn_classify_workspace(Nq, Ng, D, k, num_classes, splits)) {
    rsp_set_error("rsp_knn_classify: workspace too small");
    return RSP_EWORKSPACE;
  }
  Args a = {};
  a.q = q, a.g = g, a.ldq = ldq, a.Nq = Nq, a.ldg = ldg, a.Ng = Ng, a.D = D, a.k = k, a.C = num_classes;
  a.splits = rsp_cosine_topk_splits(Nq, Ng, splits);
  a.inv_T = 1.f / T;
  a.yq = reinterpret_cast<const long long*>(y_q), a.yg = reinterpret_cast<const long long*>(y_g);
  a.invq = reinterpret_cast<float*>(workspace);
  a.invg = a.invq + Nq;
  char* part = reinterpret_cast<char*>(workspace) + rsp_align_up((size_t)(Nq + Ng) * sizeof(float), 256);
  a.part_val = reinterpret_cast<float*>(part);
  a.part_idx = reinterpret_cast<int*>(part + (size_t)a.splits * Nq * k * sizeof(float));
  a.idx = idx, a.dist = dist, a.votes = votes, a.pred = pred, a.rank = rank;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(knn_inv_norm_kernel, dim3(rsp_cdiv(Nq, 4)), dim3(256), 0, s, q, ldq, Nq, D, a.invq);
  int rc = rsp_check_launch("knn_inv_norm_kernel");
  if (rc != RSP_OK) return rc;
  hipLaunchKernelGGL(knn_inv_norm_kernel, dim3(rsp_cdiv(Ng, 4)), dim3(256), 0, s, g, ldg, Ng, D, a.invg);
  rc = rsp_check_launch("knn_inv_norm_kernel");
  if (rc != RSP_OK) return rc;
  switch (rsp_cdiv(k, 64)) {
    case 1: rc = launch_search_and_vote<1>(a, s); break;
    case 2: rc = launch_search_and_vote<2>(a, s); break;
    case 3: rc = launch_search_and_vote<3>(a, s); break;
    default: rc = launch_search_and_vote<4>(a, s); break;
  }
  if (rc != RSP_OK || !hits) return rc;
  hipLaunchKernelGGL(knn_hits_kernel, dim3(1), dim3(256), 0, s, rank, valid, hits);
  return rsp_check_launch("knn_hits_kernel");
}
