// Everything the fine-tune loop does behind the classifier's logits (the reference's finetune.py:101-143), as one call:
// crop mean (:54-61), nn.CrossEntropyLoss forward and gradient (:105), accuracy(topk=(1, 5)) over the valid samples (:112-139,
// framework/metrics/classification.py:6-20) and the three AverageMeter.update calls (framework/meters/average.py:22-26).
//
// Rank rule: rank(s) = #{c : avg[s][c] > avg[s][t]} + #{c < t : avg[s][c] == avg[s][t]}, t = target[s]; top-1 needs rank 0, top-5
// rank < 5.  An exact tie therefore goes to the lower class index (torch.topk leaves ties unspecified: the one divergence).  A
// sample with a NaN (crop-mean) logit or a target outside [0, classes) is a miss, and the rows of a sample with a bad target get
// a NaN gradient: the batch loss is NaN then, and its gradient must not look usable.  Infinite logits are ranked by the comparison
// like any other value (torch.topk's accuracy): +inf at the target is a hit although the sample's loss is NaN.
//
// Kernels (no atomics, no fences, fixed reduction order: the same input gives the same bits):
//   xent_sample_kernel   one workgroup of 256 per sample, thread t owns classes t, t + 256, ... (at most 16: classes <= 4096) in
//                        registers: crop mean in crop order -> avg_logits; row max, sum of exp and rank by wave reductions
//                        combined over the 4 waves in wave order; softmax gradient to every crop row of the sample; the sample's
//                        loss and rank to the workspace.
//   xent_finish_kernel   one wave: mean of the per-sample losses (lane-strided serial sums, then the butterfly), hit counts over
//                        the first `valid` samples, loss / acc outputs and the meter update by lane 0.
#include "common.h"

#include <math.h>

namespace {

constexpr int XE_THREADS = 256;
constexpr int XE_PER = 16;                            // classes per thread
constexpr int XE_MAX_CLASSES = XE_THREADS * XE_PER;   // 4096
constexpr int XE_MAX_CROP = 32;
constexpr int XE_MISS = 0x7fffffff;

__device__ __forceinline__ float crop_mean(const float* __restrict__ base, int ld, int n_crop, int c) {
  float s = 0.f;
  for (int j = 0; j < n_crop; ++j) s += base[(long long)j * ld + c];      // crop order: the same bits wherever it is evaluated
  return n_crop == 1 ? s : s / (float)n_crop;
}

__global__ __launch_bounds__(XE_THREADS) void xent_sample_kernel(const float* __restrict__ logits, int classes, int ld, int n_crop,
                                                                 int S, const long long* __restrict__ target,
                                                                 float* __restrict__ avg_logits, float* __restrict__ dlogits,
                                                                 float* __restrict__ sample_loss, int* __restrict__ sample_rank) {
  __shared__ float sf[2][XE_THREADS / 64];
  __shared__ int si[2][XE_THREADS / 64];
  const int s = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const float* base = logits + (long long)s * n_crop * ld;
  const long long tg = target[s];
  const bool good = tg >= 0 && tg < classes;

  float v[XE_PER];
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < XE_PER; ++i) {
    const int c = t + XE_THREADS * i;
    v[i] = -INFINITY;
    if (c < classes) {
      v[i] = crop_mean(base, ld, n_crop, c);
      avg_logits[(long long)s * classes + c] = v[i];
      m = fmaxf(m, v[i]);
    }
  }
  m = rsp_wave_max(m);
  if (lane == 0) sf[0][wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(sf[0][0], sf[0][1]), fmaxf(sf[0][2], sf[0][3]));

  const float vt = good ? crop_mean(base, ld, n_crop, (int)tg) : 0.f;
  float e[XE_PER];
  float sum = 0.f;
  int rank = 0, nans = 0;
#pragma unroll
  for (int i = 0; i < XE_PER; ++i) {
    const int c = t + XE_THREADS * i;
    e[i] = 0.f;
    if (c < classes) {
      e[i] = expf(v[i] - m);
      sum += e[i];
      rank += (v[i] > vt || (v[i] == vt && c < (int)tg)) ? 1 : 0;
      nans += v[i] != v[i] ? 1 : 0;
    }
  }
  sum = rsp_wave_sum(sum);
  rank = rsp_wave_sum_i(rank);
  nans = rsp_wave_sum_i(nans);
  if (lane == 0) {
    sf[1][wave] = sum;
    si[0][wave] = rank;
    si[1][wave] = nans;
  }
  __syncthreads();
  sum = ((sf[1][0] + sf[1][1]) + sf[1][2]) + sf[1][3];
  rank = si[0][0] + si[0][1] + si[0][2] + si[0][3];
  nans = si[1][0] + si[1][1] + si[1][2] + si[1][3];

  const float loss = good ? (logf(sum) + m) - vt : NAN;
  if (t == 0) {
    sample_loss[s] = loss;
    // a NaN logit or a bad target is a miss; an infinite logit is ranked by comparison like any other value, as torch.topk ranks
    // it, though +inf anywhere in the row makes the loss NaN (inf - inf)
    sample_rank[s] = good && nans == 0 ? rank : XE_MISS;
  }
  if (dlogits) {
    const float denom = (float)S * (float)n_crop;
#pragma unroll
    for (int i = 0; i < XE_PER; ++i) {
      const int c = t + XE_THREADS * i;
      if (c < classes) {
        const float g = good ? (e[i] / sum - (c == (int)tg ? 1.f : 0.f)) / denom : NAN;
        for (int j = 0; j < n_crop; ++j) dlogits[((long long)s * n_crop + j) * classes + c] = g;
      }
    }
  }
}

__global__ __launch_bounds__(64) void xent_finish_kernel(const float* __restrict__ sample_loss, const int* __restrict__ sample_rank,
                                                         int S, int valid, int classes, float* __restrict__ loss,
                                                         float* __restrict__ acc, rsp_cls_meters* __restrict__ meters) {
  const int lane = threadIdx.x;
  float sum = 0.f;
  int h1 = 0, h5 = 0;
  for (int s = lane; s < S; s += 64) {
    sum += sample_loss[s];
    if (s < valid) {
      const int r = sample_rank[s];
      h1 += r == 0 ? 1 : 0;
      h5 += r < 5 ? 1 : 0;
    }
  }
  sum = rsp_wave_sum(sum);
  h1 = rsp_wave_sum_i(h1);
  h5 = rsp_wave_sum_i(h5);
  if (lane != 0) return;
  const float l = sum / (float)S;
  loss[0] = l;
  if (valid <= 0) return;
  // correct_k * (100.0 / batch_size): the factor is rounded to fp32 first, as a Python scalar times a float tensor is
  const float per = (float)(100.0 / (double)valid);
  const float a1 = __fmul_rn((float)h1, per), a5 = __fmul_rn((float)h5, per);
  const bool top5 = classes >= 5;
  acc[0] = a1;
  if (top5) acc[1] = a5;
  if (meters) {
    const float n = (float)valid;
    const float val[3] = {l, a1, a5};
    for (int i = 0; i < 3; ++i) {
      if (i == 2 && !top5) break;
      meters->val[i] = val[i];
      meters->sum[i] = __fadd_rn(meters->sum[i], __fmul_rn(val[i], n));      // two roundings, as sum += val * n has
      meters->count[i] += valid;
    }
  }
}

}  // namespace

size_t rsp_xent_metrics_workspace(int32_t rows, int32_t n_crop) {
  if (rows <= 0 || n_crop <= 0 || rows % n_crop) return 0;
  return (size_t)(rows / n_crop) * (sizeof(float) + sizeof(int32_t));
}

int rsp_xent_metrics(const float* logits, int32_t rows, int32_t classes, int32_t ld, int32_t n_crop, const int64_t* target,
                     int32_t valid, float* avg_logits, float* dlogits, float* loss, float* acc, rsp_cls_meters* meters,
                     void* workspace, size_t workspace_bytes, void* stream) {
  RSP_REQUIRE(logits && target && avg_logits && loss && acc && workspace, "rsp_xent_metrics: null pointer");
  RSP_REQUIRE(rows >= 1 && classes >= 1 && classes <= XE_MAX_CLASSES && ld >= classes,
              "rsp_xent_metrics: bad size (rows >= 1, 1 <= classes <= 4096, ld >= classes)");
  RSP_REQUIRE(n_crop >= 1 && n_crop <= XE_MAX_CROP && rows % n_crop == 0,
              "rsp_xent_metrics: n_crop must be in [1, 32] and divide rows");
  const int S = rows / n_crop;
  RSP_REQUIRE(valid >= 0 && valid <= S, "rsp_xent_metrics: valid must be in [0, rows / n_crop]");
  if (workspace_bytes < rsp_xent_metrics_workspace(rows, n_crop)) {
    rsp_set_error("rsp_xent_metrics: workspace too small");
    return RSP_EWORKSPACE;
  }
  float* sample_loss = reinterpret_cast<float*>(workspace);
  int* sample_rank = reinterpret_cast<int*>(sample_loss + S);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(xent_sample_kernel, dim3(S), dim3(XE_THREADS), 0, s, logits, classes, ld, n_crop, S,
                     reinterpret_cast<const long long*>(target), avg_logits, dlogits, sample_loss, sample_rank);
  int rc = rsp_check_launch("xent_sample_kernel");
  if (rc != RSP_OK) return rc;
  hipLaunchKernelGGL(xent_finish_kernel, dim3(1), dim3(64), 0, s, sample_loss, sample_rank, S, valid, classes, loss, acc, meters);
  return rsp_check_launch("xent_finish_kernel");
}
