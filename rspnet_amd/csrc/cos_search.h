// Internal interface of the cosine top-k search (cos_search.hip), used by rsp_cosine_topk (retrieval.hip) and rsp_knn_classify
// (knn.hip): the host launcher that leaves the per-split lists in the workspace, and the sorted list of a wave, which the search
// kernel and the two merge kernels (cos_merge_kernel, knn_vote_kernel) share.  Not part of the C ABI.
#pragma once
#include "common.h"

#include <math.h>

constexpr int COS_SEARCH_MAXK = 256;      // 4 list slots of 64 ranks

// The fp32 sum of squares of one row of D (even) floats by one wave, the same value in every lane: lane l takes its float2 columns
// 2 l, 2 l + 128, ... by fmaf, x then y; then the wave's xor butterfly.  inv_norm_kernel (cos_search.hip) and probe_rows_kernel
// (linear_probe.hip) both call it, so "the sum of squares as the search forms it" is one piece of code.
__device__ __forceinline__ float rsp_row_sumsq(const float* __restrict__ p, int D, int lane) {
  float s = 0.f;
  for (int c = 2 * lane; c < D; c += 128) {
    const float2 v = *reinterpret_cast<const float2*>(p + c);
    s = fmaf(v.x, v.x, s);
    s = fmaf(v.y, v.y, s);
  }
  return rsp_wave_sum(s);
}

// inv[row] = 1 / sqrtf(rsp_row_sumsq(row)) for the n rows of x, 0 for a row whose sum of squares is not finite and > 0 (one launch of
// inv_norm_kernel, cos_search.hip): the inverse norms of the search, and the validity flag of rsp_repr_stats, rsp_kmeans_fit and
// rsp_tsne_affinities.  stop: nullptr, or a device flag that turns the launch into a no-op while it is not 0.
int rsp_inv_norms(const float* x, int ld, int n, int D, float* inv, const int* stop, hipStream_t s);

// Stream compaction of the indices [lo, hi) by a block of 256 threads, in trips of 256: emit(rank, i) for every i with valid(i), rank
// counting the valid indices in ascending order from 0 (the wave's ballot, the four waves' counts through LDS, the trips' running
// total: integers, order fixed).  Returns the number of valid indices to every thread.  Holds barriers: all 256 threads call it.
// probe_compact_kernel (linear_probe.hip), km_compact_kernel (cluster.hip) and ts_compact_kernel (tsne.hip) are this plus a trailer.
template <class Index, class Valid, class Emit>
__device__ __forceinline__ int rsp_compact_rows(Index lo, Index hi, Valid valid, Emit emit) {
  __shared__ int wcnt[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int base = 0;
  for (Index start = lo; start < hi; start += 256) {
    const Index i = start + t;
    const bool v = i < hi && valid(i);
    const unsigned long long mask = __ballot(v);
    if (lane == 0) wcnt[wave] = __popcll(mask);
    __syncthreads();
    int woff = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      woff += w < wave ? wcnt[w] : 0;
      tot += wcnt[w];
    }
    if (v) emit(base + woff + __popcll(mask & ((1ull << lane) - 1ull)), i);
    base += tot;
    __syncthreads();
  }
  return base;
}

// The per-split lists the search left in the workspace: entry (split * Nq + row) * k + rank, sorted by rank; a list that is not
// full (fewer than k gallery rows in the split) ends in index -1.
struct CosLists {
  float* val;
  int* idx;
  int splits;
  const float* inv_q;      // the inverse norms the search left at the head of the workspace: [Nq], then inv_g [Ng]
  const float* inv_g;
};

// The size, k and alignment checks both entry points make on q and g; `who` is the entry point's name in the message.
int rsp_cos_search_check(const char* who, const float* q, int ldq, int Nq, const float* g, int ldg, int Ng, int D, int k, int kmax);
// Checks and carves the workspace (rsp_cosine_topk_workspace bytes), runs the inverse norms of q and g and then the search.
int rsp_cos_search(const char* who, const float* q, int ldq, int Nq, const float* g, int ldg, int Ng, int D, int k, int splits,
                   void* workspace, size_t workspace_bytes, hipStream_t s, CosLists* lists);
// The same search for a caller that issues it many times over one query matrix (rsp_kmeans_fit): stop, when not nullptr, is a device
// flag that turns every launch into a no-op while it is not 0; norm_q = false keeps the query norms of an earlier call on the same
// workspace.  rsp_cos_search is this with (nullptr, true).
int rsp_cos_search_gated(const char* who, const float* q, int ldq, int Nq, const float* g, int ldg, int Ng, int D, int k, int splits,
                         void* workspace, size_t workspace_bytes, hipStream_t s, CosLists* lists, const int* stop, bool norm_q);

// A wave's sorted list of k entries in S = ceil(k / 64) register slots per lane: rank r lives in slot r / 64, lane r % 64.
// kmask: the lanes of the LAST slot that belong to the list (the slots below it are full).
__device__ __forceinline__ unsigned long long last_slot_mask(int k, int S) {
  const int n = k - 64 * (S - 1);
  return n >= 64 ? ~0ull : ((1ull << n) - 1ull);
}

// Insert (s, i).  Entries already in the list that are >= s stay ahead: the caller inserts in ascending gallery index order, so on
// an exact tie the lower index stays first.  false: s is behind all k entries.
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

// One split's sorted list into the wave's list; stops once an entry loses (sorted: the rest of that list loses too).
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

// Query `row`'s list over the whole gallery: the split lists merged in split order, that is in ascending gallery ranges, so a
// tie with an earlier split's entry stays behind it.
template <int S>
__device__ __forceinline__ void merge_lists(float (&tv)[S], int (&ti)[S], const float* __restrict__ part_val,
                                            const int* __restrict__ part_idx, int Nq, int row, int k, int splits, int lane) {
  const unsigned long long kmask = last_slot_mask(k, S);
#pragma unroll
  for (int sl = 0; sl < S; ++sl) {
    tv[sl] = -INFINITY;
    ti[sl] = -1;
  }
  for (int s = 0; s < splits; ++s) {
    const long long o = ((long long)s * Nq + row) * k;
    merge_split<S>(tv, ti, part_val + o, part_idx + o, k, kmask, lane);
  }
}

// The list as row `row` of idx / dist: distance clip(1 - s, 0, 2); an empty entry (Ng < k) is index -1 at distance +inf.
template <int S>
__device__ __forceinline__ void store_list(const float (&tv)[S], const int (&ti)[S], int row, int k, int lane, int* __restrict__ idx,
                                           float* __restrict__ dist) {
#pragma unroll
  for (int sl = 0; sl < S; ++sl) {
    const int rk = 64 * sl + lane;
    if (rk < k) {
      idx[(long long)row * k + rk] = ti[sl];
      dist[(long long)row * k + rk] = ti[sl] < 0 ? INFINITY : fminf(fmaxf(1.f - tv[sl], 0.f), 2.f);
    }
  }
}
