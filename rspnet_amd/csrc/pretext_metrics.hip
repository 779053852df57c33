// The per-step bookkeeping of the pretext loop (the reference's pretrain.py:167-195) as one call: accuracy(topk=(1, 5)) of both
// contrast logit matrices, the top-1 of the ranking pair (framework/metrics/classification.py:6-20) and the eight
// AverageMeter.update calls (framework/meters/average.py:22-26).
//
// labels_A is all zeros, so the positive is column 0 and the rank of a row is a COUNT: rank = #{c : v[c] > v[0]}.  A column equal
// to the positive does not count -- an exact tie goes to the lower index, the rule of rsp_xent_metrics -- and a NaN never compares
// greater.  A NaN positive is a miss.  Hit counts are integers and every accuracy is two fp32 operations: results are exact.
//
// Kernels (no atomics, fixed reduction order: the same input gives the same bits):
//   pretext_rank_kernel    one workgroup of 256 per row of each matrix (2 * B workgroups).  Rows start at r * K1 floats and the
//                          shipped K1 = 16385 is odd, so a row is 4-byte aligned only: scalar loads up to the first 16-byte
//                          boundary, 16-byte loads over the body, scalar loads over the tail.  Counts are summed per wave, then
//                          over the 4 waves through LDS; the row's rank goes to the workspace.
//   pretext_finish_kernel  one wave: hit counts over the B rows (lane-strided, then the butterfly), acc and the meter update
//                          by lane 0.
#include "common.h"

namespace {

constexpr int PM_THREADS = 256;
constexpr int PM_MISS = 0x7fffffff;

__global__ __launch_bounds__(PM_THREADS) void pretext_rank_kernel(const float* __restrict__ logits1,
                                                                  const float* __restrict__ logits2, int B, int K1,
                                                                  int* __restrict__ rank_out) {
  __shared__ int si[PM_THREADS / 64];
  const int r = blockIdx.x, t = threadIdx.x;
  const float* base = (r < B ? logits1 : logits2) + (long long)(r < B ? r : r - B) * K1;
  const float v0 = base[0];
  // floats in front of the first 16-byte boundary (the pointer is float-aligned), then whole float4s, then the rest
  const int head = min(K1, (int)(((16u - (unsigned)((uintptr_t)base & 15u)) & 15u) >> 2));
  const int nvec = (K1 - head) >> 2;
  const int tail0 = head + (nvec << 2);
  int n = 0;
  if (t < head) n += base[t] > v0 ? 1 : 0;
  const floatx4* body = reinterpret_cast<const floatx4*>(base + head);
  for (int i = t; i < nvec; i += PM_THREADS) {
    const floatx4 x = body[i];
    n += (x[0] > v0 ? 1 : 0) + (x[1] > v0 ? 1 : 0) + (x[2] > v0 ? 1 : 0) + (x[3] > v0 ? 1 : 0);
  }
  if (tail0 + t < K1) n += base[tail0 + t] > v0 ? 1 : 0;      // at most 3 columns
  n = rsp_wave_sum_i(n);
  if ((t & 63) == 0) si[t >> 6] = n;
  __syncthreads();
  if (t == 0) rank_out[r] = v0 == v0 ? si[0] + si[1] + si[2] + si[3] : PM_MISS;
}

__global__ __launch_bounds__(64) void pretext_finish_kernel(const int* __restrict__ rank, const float* __restrict__ lposM,
                                                            const float* __restrict__ lnegM, int B,
                                                            const float* __restrict__ losses, float* __restrict__ acc,
                                                            rsp_pretext_meters* __restrict__ meters) {
  const int lane = threadIdx.x;
  int h[5] = {0, 0, 0, 0, 0};
  for (int b = lane; b < B; b += 64) {
    const int r1 = rank[b], r2 = rank[B + b];
    h[0] += r1 == 0 ? 1 : 0;
    h[1] += r1 < 5 ? 1 : 0;
    h[2] += r2 == 0 ? 1 : 0;
    h[3] += r2 < 5 ? 1 : 0;
    h[4] += lposM[b] >= lnegM[b] ? 1 : 0;      // top-1 of cat(l_pos_M, l_neg_M) with the tie to column 0; a NaN is a miss
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) h[i] = rsp_wave_sum_i(h[i]);
  if (lane != 0) return;
  // correct_k * (100.0 / batch_size): the factor is rounded to fp32 first, as a Python scalar times a float tensor is
  const float per = (float)(100.0 / (double)B);
  float a[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    a[i] = __fmul_rn((float)h[i], per);
    acc[i] = a[i];
  }
  if (!meters) return;
  const float n = (float)B;
  const float val[8] = {losses[0], losses[1], a[0], a[1], a[2], a[3], losses[2], a[4]};
  for (int i = 0; i < 8; ++i) {
    meters->val[i] = val[i];
    meters->sum[i] = __fadd_rn(meters->sum[i], __fmul_rn(val[i], n));      // two roundings, as sum += val * n has
    meters->count[i] += B;
  }
}

}  // namespace

size_t rsp_pretext_metrics_workspace(int32_t B) {
  if (B <= 0) return 0;
  return (size_t)2 * (size_t)B * sizeof(int32_t);
}

int rsp_pretext_metrics(const float* logits1, const float* logits2, const float* lposM, const float* lnegM, int32_t B, int32_t K1,
                        const float* losses, float* acc, rsp_pretext_meters* meters, void* workspace, size_t workspace_bytes,
                        void* stream) {
  RSP_REQUIRE(B >= 1 && K1 >= 5, "rsp_pretext_metrics: bad size (B >= 1, K1 >= 5)");
  RSP_REQUIRE(logits1 && logits2 && lposM && lnegM && acc && workspace, "rsp_pretext_metrics: null pointer");
  RSP_REQUIRE(losses || !meters, "rsp_pretext_metrics: meters need the three losses");
  RSP_REQUIRE(((uintptr_t)logits1 & 3) == 0 && ((uintptr_t)logits2 & 3) == 0 && ((uintptr_t)workspace & 3) == 0,
              "rsp_pretext_metrics: misaligned pointer");
  RSP_REQUIRE(workspace_bytes >= rsp_pretext_metrics_workspace(B), "rsp_pretext_metrics: workspace too small");
  int* rank = reinterpret_cast<int*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pretext_rank_kernel, dim3(2 * B), dim3(PM_THREADS), 0, s, logits1, logits2, B, K1, rank);
  int rc = rsp_check_launch("pretext_rank_kernel");
  if (rc != RSP_OK) return rc;
  hipLaunchKernelGGL(pretext_finish_kernel, dim3(1), dim3(64), 0, s, rank, lposM, lnegM, B, losses, acc, meters);
  return rsp_check_launch("pretext_finish_kernel");
}
