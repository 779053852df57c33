// Step fingerprints: one 32-byte record per tensor of a list -- an exact position-dependent bit hash, sum of squares, sum of
// magnitudes, largest magnitude and the count of non-finite elements -- from one call.  The project's own: the
// reference has nothing like it.
//
// The record is a function of the VALUES only: the same words at another address, another alignment, on another stream or in
// another process give the same 32 bytes, the two doubles included.
//   hash       sum over i of fmix32(w_i + i * 0x9E3779B1) mod 2^64, w_i the i-th 32-bit word, fmix32 murmur3's finaliser (a bijection
//              of 32-bit words: a change of ONE word always changes the hash; several changes at once escape with probability
//              about 2^-32).  Integer sums are exact in any order.
//   nonfinite  words whose exponent field is all ones; they stay in the hash and are left out of the three float fields.
//   sumsq, sum_abs   fp64 (the square of an fp32 value is exact in fp64), in the fixed order below.
//   max_abs    exact fp32 maximum of |v| over the finite elements.
// kind 1 (raw words: int64 counters) forms the hash only.
//
// Kernels (no atomics, no fences, no memset / memcpy: capturable, and the float order is a function of `words` alone):
//   fingerprint_chunk_kernel   one workgroup of 256 per chunk of RSP_FP_CHUNK words; the chunk's job by binary search of chunk0.
//                              Element j of the chunk belongs to thread (j / 4) % 256 -- a 16-byte-aligned chunk loads float4, a
//                              misaligned one scalars under the SAME mapping -- and each thread accumulates in index order; wave
//                              butterfly, then the four waves in wave order through LDS; one 32-byte partial per chunk.
//   fingerprint_finish_kernel  one wave per job: lane l adds the partials of chunks l, l + 64, ... in order, butterfly, lane 0 stores
//                              the record (every field, zeros for an empty job).  The pattern of xent_finish_kernel (classify.hip).
#include "common.h"

namespace {

constexpr int FP_THREADS = 256;
constexpr int FP_GROUPS = RSP_FP_CHUNK / (4 * FP_THREADS);      // 4-word groups per thread and chunk: 8
constexpr int64_t FP_MAX_CHUNKS = 1ll << 23;                     // 2^36 words: the grid stays below 2^31 threads
static_assert(RSP_FP_CHUNK % (4 * FP_THREADS) == 0, "a chunk is a whole number of rounds of 4-word groups");
static_assert(sizeof(rsp_fingerprint_job) == 32 && sizeof(rsp_fingerprint_rec) == 32, "ABI: both structs are 32 bytes");

struct Acc {
  unsigned long long hash;
  double sumsq, sum_abs;
  float max_abs;
  unsigned nonfinite;
};

__device__ __forceinline__ unsigned fmix32(unsigned x) {
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

template <bool FLOATS>
__device__ __forceinline__ void take(Acc& a, unsigned w, unsigned i) {
  a.hash += fmix32(w + i * 0x9E3779B1u);
  if (FLOATS) {
    if ((w & 0x7F800000u) == 0x7F800000u) {
      ++a.nonfinite;
    } else {
      const float v = __uint_as_float(w & 0x7FFFFFFFu);
      const double d = (double)v;
      a.sumsq = fma(d, d, a.sumsq);      // d * d is exact: one rounding, that of the sum
      a.sum_abs += d;
      a.max_abs = fmaxf(a.max_abs, v);
    }
  }
}

__device__ __forceinline__ void combine(Acc& a, const Acc& b) {
  a.hash += b.hash;
  a.sumsq += b.sumsq;
  a.sum_abs += b.sum_abs;
  a.max_abs = fmaxf(a.max_abs, b.max_abs);
  a.nonfinite += b.nonfinite;
}

__device__ __forceinline__ Acc wave_butterfly(Acc a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Acc b;
    b.hash = __shfl_xor(a.hash, o);
    b.sumsq = __shfl_xor(a.sumsq, o);
    b.sum_abs = __shfl_xor(a.sum_abs, o);
    b.max_abs = __shfl_xor(a.max_abs, o);
    b.nonfinite = __shfl_xor(a.nonfinite, o);
    combine(a, b);
  }
  return a;
}

__device__ __forceinline__ void store_rec(rsp_fingerprint_rec* __restrict__ dst, const Acc& a) {
  dst->hash = a.hash;
  dst->sumsq = a.sumsq;
  dst->sum_abs = a.sum_abs;
  dst->max_abs = a.max_abs;
  dst->nonfinite = a.nonfinite;
}

// the words [0, n) of one chunk that starts at global word index i0; p: the chunk's first word
template <bool FLOATS>
__device__ __forceinline__ void chunk_words(Acc& a, const unsigned* __restrict__ p, int n, unsigned i0, int t) {
  if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
#pragma unroll
    for (int g = 0; g < FP_GROUPS; ++g) {
      const int j = (g * FP_THREADS + t) * 4;
      if (j + 4 <= n) {
        const uint4 q = *reinterpret_cast<const uint4*>(p + j);
        take<FLOATS>(a, q.x, i0 + j);
        take<FLOATS>(a, q.y, i0 + j + 1);
        take<FLOATS>(a, q.z, i0 + j + 2);
        take<FLOATS>(a, q.w, i0 + j + 3);
      } else {
        for (int k = j; k < n; ++k) take<FLOATS>(a, p[k], i0 + k);
      }
    }
  } else {
#pragma unroll
    for (int g = 0; g < FP_GROUPS; ++g) {
      const int j = (g * FP_THREADS + t) * 4;
      if (j + 4 <= n) {
        const unsigned w0 = p[j], w1 = p[j + 1], w2 = p[j + 2], w3 = p[j + 3];
        take<FLOATS>(a, w0, i0 + j);
        take<FLOATS>(a, w1, i0 + j + 1);
        take<FLOATS>(a, w2, i0 + j + 2);
        take<FLOATS>(a, w3, i0 + j + 3);
      } else {
        for (int k = j; k < n; ++k) take<FLOATS>(a, p[k], i0 + k);
      }
    }
  }
}

__global__ __launch_bounds__(FP_THREADS) void fingerprint_chunk_kernel(const rsp_fingerprint_job* __restrict__ jobs, int n_jobs,
                                                                       rsp_fingerprint_rec* __restrict__ partial) {
  __shared__ Acc sw[FP_THREADS / 64];
  const long long c = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  // the last job with chunk0 <= c: jobs without a chunk share their chunk0 with the job behind them and are never the last
  int lo = 0, hi = n_jobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].chunk0 <= c) lo = mid; else hi = mid - 1;
  }
  const rsp_fingerprint_job job = jobs[lo];
  const long long start = (c - job.chunk0) * (long long)RSP_FP_CHUNK;
  Acc a = {0ull, 0.0, 0.0, 0.f, 0u};
  if (start >= 0 && start < job.words) {      // (a table that does not describe this chunk leaves a zero partial, never a stray read)
    const long long left = job.words - start;
    const int n = left < RSP_FP_CHUNK ? (int)left : RSP_FP_CHUNK;
    const unsigned* p = reinterpret_cast<const unsigned*>(job.ptr) + start;
    if (job.kind == 0) chunk_words<true>(a, p, n, (unsigned)start, t);
    else chunk_words<false>(a, p, n, (unsigned)start, t);
  }
  a = wave_butterfly(a);
  if (lane == 0) sw[wave] = a;
  __syncthreads();
  if (t == 0) {
    Acc r = sw[0];
    combine(r, sw[1]);
    combine(r, sw[2]);
    combine(r, sw[3]);
    store_rec(partial + c, r);
  }
}

__global__ __launch_bounds__(64) void fingerprint_finish_kernel(const rsp_fingerprint_job* __restrict__ jobs, long long total_chunks,
                                                                const rsp_fingerprint_rec* __restrict__ partial,
                                                                rsp_fingerprint_rec* __restrict__ out) {
  const int lane = threadIdx.x;
  const rsp_fingerprint_job job = jobs[blockIdx.x];
  long long n = job.words > 0 ? (job.words + RSP_FP_CHUNK - 1) / RSP_FP_CHUNK : 0;
  if (job.chunk0 < 0 || job.chunk0 > total_chunks || n > total_chunks - job.chunk0) n = 0;      // never read past the workspace
  Acc a = {0ull, 0.0, 0.0, 0.f, 0u};
  for (long long k = lane; k < n; k += 64) {
    const rsp_fingerprint_rec r = partial[job.chunk0 + k];
    const Acc b = {r.hash, r.sumsq, r.sum_abs, r.max_abs, r.nonfinite};
    combine(a, b);
  }
  a = wave_butterfly(a);
  if (lane == 0) store_rec(out + blockIdx.x, a);
}

}  // namespace

size_t rsp_fingerprint_workspace(int64_t total_chunks) {
  if (total_chunks <= 0 || total_chunks > FP_MAX_CHUNKS) return 0;
  return (size_t)total_chunks * sizeof(rsp_fingerprint_rec);
}

int rsp_fingerprint(const rsp_fingerprint_job* jobs_dev, int32_t n_jobs, int64_t total_chunks, rsp_fingerprint_rec* out_dev,
                    void* workspace, size_t workspace_bytes, void* stream) {
  RSP_REQUIRE(n_jobs >= 0, "rsp_fingerprint: n_jobs must not be negative");
  if (n_jobs == 0) return RSP_OK;
  RSP_REQUIRE(jobs_dev && out_dev, "rsp_fingerprint: null pointer");
  RSP_REQUIRE(total_chunks >= 0 && total_chunks <= FP_MAX_CHUNKS, "rsp_fingerprint: bad size (0 <= total_chunks <= 2^23)");
  RSP_REQUIRE(((uintptr_t)jobs_dev & 7) == 0 && ((uintptr_t)out_dev & 7) == 0 && ((uintptr_t)workspace & 7) == 0,
              "rsp_fingerprint: the job table, the records and the workspace must be 8-byte aligned");
  if (total_chunks > 0 && (!workspace || workspace_bytes < rsp_fingerprint_workspace(total_chunks))) {
    rsp_set_error("rsp_fingerprint: workspace too small");
    return RSP_EWORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  rsp_fingerprint_rec* partial = reinterpret_cast<rsp_fingerprint_rec*>(workspace);
  if (total_chunks > 0) {
    hipLaunchKernelGGL(fingerprint_chunk_kernel, dim3((unsigned)total_chunks), dim3(FP_THREADS), 0, s, jobs_dev, n_jobs, partial);
    const int rc = rsp_check_launch("fingerprint_chunk_kernel");
    if (rc != RSP_OK) return rc;
  }
  hipLaunchKernelGGL(fingerprint_finish_kernel, dim3(n_jobs), dim3(64), 0, s, jobs_dev, (long long)total_chunks, partial, out_dev);
  return rsp_check_launch("fingerprint_finish_kernel");
}
