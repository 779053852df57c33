// Clustering evaluation (rsp_kmeans_fit, rsp_kmeans_assign, rsp_contingency): spherical k-means on N stored feature rows, every
// iteration issued from one call, nothing read back, stopped on the device; and the cluster x label contingency table behind NMI / ARI /
// purity.  include/rspnet_hip.h states the rule; rspnet_amd/cluster.py restates it in numpy fp64 (kmeans_reference).
//
// The assignment step IS the cosine search (cos_search.hip) with the centroids as the gallery and k = 1: no second similarity
// expression lives here.  The search's inverse norms of x, left at the head of its workspace, also decide validity (1 / sqrtf(ss) is
// > 0 exactly when ss is finite and > 0) and form xh = x * inv when the update stages a row.
//
// Kernels (fit: six launches per iteration, every one of them returns at once while the stop flag of the state is set):
//   km_compact_kernel   once per call, one block: the valid rows of x in ascending order as a list of row indices and their number
//                       M (rsp_compact_rows, cos_search.h); assign = -1 for the invalid ones; the state reset.
//                       Every later kernel walks that list by rank, so the fit is, to the bit, the fit on x without the invalid rows.
//   km_assign_kernel    one thread per listed row: the search's k = 1 lists merged in split order (a later split's entry takes over
//                       only when strictly greater: the tie rule), the new assignment against the previous one; a block of 256 ranks
//                       leaves (changed, assigned, sum of sim in fp64: the wave's xor butterfly, then the four waves in order).
//   km_step_kernel      one wave: the block partials (lane l: l, l + 64, ... in order, then the butterfly) into changed_trace[t] and
//                       objective_trace[t]; the stop: t > 0 and nothing changed.
//   km_update_kernel    probe_wgrad_kernel with a one-hot first operand built on the fly: block = a 64 x 128 tile of cent (clusters x
//                       D) x one split of the listed rows.  Chunks of 32 rows are staged as their 32 cluster ids and [row][128 xh
//                       columns]; the MFMA's A operand is (id == cluster) ? 1 : 0, so an element of cent is the plain fp32 sum of its
//                       rows' xh in row order (1 * v and 0 * v are exact).  The block of D-tile 0 also counts its 64 clusters
//                       (integers).  fp32 partials per split in the workspace; the split count is km_splits at M.
//   km_reduce_kernel    block = one cluster x 256 columns: the cluster's count over the splits; with a count > 0 the split partials in
//                       split order into cent, else cent is left as it is.
//   km_finish_kernel    one block: info, the trace entries past iters_run (-1 / NaN), the empty clusters.
//   km_assign_rows_kernel   rsp_kmeans_assign: one thread per row of x, no list: the merged neighbour, -1 / NaN for an invalid row.
//   contingency_zero_kernel, contingency_count_kernel   the table zeroed by a kernel, then integer atomic adds (order-free, exact).
#include "cos_search.h"

namespace {

constexpr int KM_BA = 64;              // clusters per cent tile
constexpr int KM_BB = 128;             // feature columns per cent tile
constexpr int KM_KC = 32;              // rows per staged chunk
constexpr int KM_BUF = KM_KC * KM_BB;  // floats per staged chunk (16 KiB; two buffers and the ids: static LDS)
constexpr int KM_TARGET_BLOCKS = 1024;
constexpr int KM_ROWS = 256;           // ranks per block of km_assign_kernel

struct KmState {      // in the workspace; reset by km_compact_kernel
  int stop, iters_run, converged, unassigned, m, pad;
};
struct KmPartial {
  double obj;
  int changed, assigned;
};

// The split count of an update over `rows` listed rows: about KM_TARGET_BLOCKS blocks (cap = that over the tile count), at least four
// 32-row chunks per split (probe_splits' formula).  Monotone in rows: the launch is sized by N, the kernels use the value at M.
__host__ __device__ __forceinline__ int km_splits(int cap, int rows) {
  const int s = min(cap, ((rows + KM_KC - 1) / KM_KC) / 4);
  return s < 1 ? 1 : s;
}

__global__ __launch_bounds__(256) void km_compact_kernel(const float* __restrict__ inv, int N, int* __restrict__ rows,
                                                         int* __restrict__ assign, KmState* __restrict__ st) {
  const int t = threadIdx.x;
  const auto valid = [&](int i) { return inv[i] > 0.f; };      // (ss finite and > 0: rsp_inv_norms)
  const int base = rsp_compact_rows(0, N, valid, [&](int r, int i) { rows[r] = i; });
  for (int i = t; i < N; i += 256)
    if (!valid(i)) assign[i] = -1;
  if (t == 0) {
    st->stop = 0;
    st->iters_run = 0;
    st->converged = 0;
    st->unassigned = 0;
    st->m = base;
    st->pad = 0;
  }
}

// Row `row`'s single neighbour from the search's k = 1 lists: the splits in order, a later one only when strictly greater (what
// merge_lists does with one slot).  -1: no centroid is returnable.
__device__ __forceinline__ int km_best(const float* __restrict__ val, const int* __restrict__ idx, int splits, int N, int row,
                                       float* sim) {
  float bv = -INFINITY;
  int bi = -1;
  for (int s = 0; s < splits; ++s) {
    const long long o = (long long)s * N + row;
    const int i = idx[o];
    const float v = val[o];
    if (i >= 0 && v > bv) {
      bv = v;
      bi = i;
    }
  }
  *sim = bv;
  return bi;
}

__global__ __launch_bounds__(256) void km_assign_kernel(const float* __restrict__ val, const int* __restrict__ idx, int splits, int N,
                                                        const int* __restrict__ rows, const KmState* __restrict__ st, int t,
                                                        int* __restrict__ assign, KmPartial* __restrict__ part) {
  __shared__ double wobj[4];
  __shared__ int wchg[4], wasg[4];
  if (st->stop) return;
  const int m = st->m, j = blockIdx.x * KM_ROWS + threadIdx.x;
  if (blockIdx.x * KM_ROWS >= m) return;      // (the whole block: the launch is sized by N)
  int changed = 0, assigned = 0;
  double obj = 0.0;
  if (j < m) {
    const int row = rows[j];
    float sim;
    const int a = km_best(val, idx, splits, N, row, &sim);
    changed = t == 0 ? 1 : (assign[row] != a ? 1 : 0);      // (at t = 0 assign holds nothing yet and is not read)
    assign[row] = a;
    if (a >= 0) {
      assigned = 1;
      obj = (double)sim;
    }
  }
  obj = rsp_wave_sum_d(obj);
  changed = rsp_wave_sum_i(changed);
  assigned = rsp_wave_sum_i(assigned);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    wobj[wave] = obj;
    wchg[wave] = changed;
    wasg[wave] = assigned;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    KmPartial p;
    p.obj = ((wobj[0] + wobj[1]) + wobj[2]) + wobj[3];
    p.changed = wchg[0] + wchg[1] + wchg[2] + wchg[3];
    p.assigned = wasg[0] + wasg[1] + wasg[2] + wasg[3];
    part[blockIdx.x] = p;
  }
}

__global__ __launch_bounds__(64) void km_step_kernel(const KmPartial* __restrict__ part, KmState* __restrict__ st, int t,
                                                     int* __restrict__ changed_trace, double* __restrict__ objective_trace) {
  if (st->stop) return;
  const int lane = threadIdx.x, m = st->m, nb = (m + KM_ROWS - 1) / KM_ROWS;
  double obj = 0.0;
  int changed = 0, assigned = 0;
  for (int b = lane; b < nb; b += 64) {
    obj += part[b].obj;
    changed += part[b].changed;
    assigned += part[b].assigned;
  }
  obj = rsp_wave_sum_d(obj);
  changed = rsp_wave_sum_i(changed);
  assigned = rsp_wave_sum_i(assigned);
  if (lane == 0) {
    changed_trace[t] = changed;
    objective_trace[t] = assigned > 0 ? obj / (double)assigned : 0.0;
    st->iters_run = t + 1;
    st->unassigned = m - assigned;
    if (t > 0 && changed == 0) {
      st->converged = 1;
      st->stop = 1;
    }
  }
}

__global__ __launch_bounds__(256) void km_update_kernel(const float* __restrict__ x, int ld, int D, const float* __restrict__ inv,
                                                        const int* __restrict__ rows, const int* __restrict__ assign,
                                                        const KmState* __restrict__ st, int C, int tiles_b, int split_cap,
                                                        float* __restrict__ sumpart, int* __restrict__ cntpart) {
  __shared__ __attribute__((aligned(16))) float sm[2 * KM_BUF];
  __shared__ int ids[2][KM_KC];
  if (st->stop) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l32 = lane & 31, h = lane >> 5;
  const int wa = wave >> 1, wb = wave & 1;
  const int ta = blockIdx.x / tiles_b, tb = blockIdx.x - ta * tiles_b;
  const int a0 = ta * KM_BA, b0 = tb * KM_BB;
  const int split = blockIdx.y;
  const int n = st->m, splits = km_splits(split_cap, n);
  if (split >= splits) return;      // (the whole block: the launch is sized by the split count at N rows)
  const int chunks = (n + KM_KC - 1) / KM_KC;
  const int c_lo = (int)((long long)split * chunks / splits), c_hi = (int)((long long)(split + 1) * chunks / splits);
  const bool counts_too = tb == 0 && wave == 0;

  // this thread's 8 float2 slots of a chunk (slot e = t + 256 it: staged row e / 64, float2 column e % 64 of the 128 feature
  // columns); thread t < 32 also stages the cluster id of staged row t
  const int xcol = b0 + 2 * (t & 63);
  float2 rx[8];
  float rf[8];
  int rid = -1;
  auto load = [&](int chunk) {
    int gx[8];
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int rr = chunk * KM_KC + ((t + 256 * it) >> 6);
      gx[it] = rr < n ? rows[rr] : -1;
      rf[it] = gx[it] >= 0 ? inv[gx[it]] : 0.f;
    }
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      // selected, never multiplied away: a row that is not listed is not read at all
      rx[it] = (gx[it] >= 0 && xcol < D) ? *reinterpret_cast<const float2*>(x + (long long)gx[it] * ld + xcol) : make_float2(0.f, 0.f);
    }
    if (t < KM_KC) {
      const int rr = chunk * KM_KC + t;
      rid = rr < n ? assign[rows[rr]] : -1;
    }
  };
  auto store = [&](int b) {
    float* buf = sm + b * KM_BUF;
#pragma unroll
    for (int it = 0; it < 8; ++it)
      *reinterpret_cast<float2*>(buf + ((t + 256 * it) >> 6) * KM_BB + 2 * (t & 63)) = make_float2(rx[it].x * rf[it], rx[it].y * rf[it]);
    if (t < KM_KC) ids[b][t] = rid;
  };

  floatx16 acc0, acc1;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    acc0[e] = 0.f;
    acc1[e] = 0.f;
  }
  int cnt = 0;
  const int mine = a0 + 32 * wa + l32;      // the cluster of this lane's A rows
  load(c_lo);      // (with n = 0 the one split is empty: it stages zeros and uses none of them)
  store(0);
  __syncthreads();
  for (int ch = c_lo; ch < c_hi; ++ch) {
    const int b = (ch - c_lo) & 1;
    const float* buf = sm + b * KM_BUF;
    if (ch + 1 < c_hi) load(ch + 1);
    // step j: lane half h holds staged row 2 j + h, for A (its cluster's one-hot entry) and B (its feature columns) alike
    const float* pb = buf + h * KM_BB + 64 * wb + l32;
#pragma unroll
    for (int j = 0; j < KM_KC / 2; ++j) {
      const float a = ids[b][2 * j + h] == mine ? 1.f : 0.f;
      const float b0v = pb[2 * j * KM_BB], b1v = pb[2 * j * KM_BB + 32];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0v, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1v, acc1, 0, 0, 0);
    }
    if (counts_too) {
#pragma unroll
      for (int k = 0; k < KM_KC; ++k) cnt += ids[b][k] == a0 + lane ? 1 : 0;
    }
    if (ch + 1 < c_hi) store(b ^ 1);
    __syncthreads();
  }

  const int bc0 = b0 + 64 * wb + l32, bc1 = bc0 + 32;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int a = a0 + 32 * wa + (e >> 2) * 8 + h * 4 + (e & 3);
    if (a < C) {
      float* row = sumpart + ((long long)split * C + a) * D;
      if (bc0 < D) row[bc0] = acc0[e];
      if (bc1 < D) row[bc1] = acc1[e];
    }
  }
  if (counts_too && a0 + lane < C) cntpart[(long long)split * C + a0 + lane] = cnt;
}

__global__ __launch_bounds__(256) void km_reduce_kernel(const float* __restrict__ sumpart, const int* __restrict__ cntpart,
                                                        const KmState* __restrict__ st, int split_cap, int C, int D,
                                                        float* __restrict__ cent, int* __restrict__ counts) {
  __shared__ int total;
  if (st->stop) return;
  const int c = blockIdx.x, col = blockIdx.y * 256 + threadIdx.x;
  const int splits = km_splits(split_cap, st->m);
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  int local = 0;
  for (int s = threadIdx.x; s < splits; s += 256) local += cntpart[(long long)s * C + c];
  if (local) atomicAdd(&total, local);      // (integers in LDS: order-free)
  __syncthreads();
  const int n = total;
  if (blockIdx.y == 0 && threadIdx.x == 0) counts[c] = n;
  if (n > 0 && col < D) {
    // the splits in split order; eight loads in flight at a time (the order of the additions is what is fixed)
    const float* p = sumpart + (long long)c * D + col;
    const long long pitch = (long long)C * D;
    float g = 0.f;
    int s = 0;
    for (; s + 8 <= splits; s += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = p[(s + u) * pitch];
#pragma unroll
      for (int u = 0; u < 8; ++u) g += v[u];
    }
    for (; s < splits; ++s) g += p[s * pitch];
    cent[(long long)c * D + col] = g;
  }
}

__global__ __launch_bounds__(256) void km_finish_kernel(const KmState* __restrict__ st, int N, int C, int max_iters,
                                                        const int* __restrict__ counts, int* __restrict__ changed_trace,
                                                        double* __restrict__ objective_trace, rsp_kmeans_info* __restrict__ info) {
  __shared__ int empty;
  if (threadIdx.x == 0) empty = 0;
  __syncthreads();
  int local = 0;
  for (int c = threadIdx.x; c < C; c += 256) local += counts[c] == 0 ? 1 : 0;
  if (local) atomicAdd(&empty, local);
  for (int t = st->iters_run + threadIdx.x; t < max_iters; t += 256) {
    changed_trace[t] = -1;
    objective_trace[t] = (double)NAN;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    info->rows_valid = st->m;
    info->rows_bad = N - st->m;
    info->iters_run = st->iters_run;
    info->converged = st->converged;
    info->empty = empty;
    info->unassigned = st->unassigned;
  }
}

__global__ __launch_bounds__(256) void km_assign_rows_kernel(const float* __restrict__ val, const int* __restrict__ idx, int splits,
                                                             int N, const float* __restrict__ inv, int* __restrict__ assign,
                                                             float* __restrict__ sim) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= N) return;
  float s;
  int a = km_best(val, idx, splits, N, row, &s);
  if (!(inv[row] > 0.f)) a = -1;
  assign[row] = a;
  if (sim) sim[row] = a >= 0 ? s : NAN;
}

__global__ __launch_bounds__(256) void contingency_zero_kernel(long long total, unsigned long long* __restrict__ table,
                                                               unsigned long long* __restrict__ dropped) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) table[i] = 0ull;
  if (blockIdx.x == 0 && threadIdx.x == 0) dropped[0] = 0ull;
}

__global__ __launch_bounds__(256) void contingency_count_kernel(const int* __restrict__ assign, const long long* __restrict__ y, int N,
                                                                int C, int L, unsigned long long* __restrict__ table,
                                                                unsigned long long* __restrict__ dropped) {
  const int stride = gridDim.x * 256;
  int bad = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < N; i += stride) {
    const int a = assign[i];
    const long long l = y[i];
    if (a >= 0 && a < C && l >= 0 && l < L) {
      atomicAdd(&table[(long long)a * L + l], 1ull);      // (integers: order-free, exact)
    } else {
      ++bad;
    }
  }
  bad = rsp_wave_sum_i(bad);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(dropped, (unsigned long long)bad);
}

// ---- host: the carve-up of the workspace --------------------------------------------------------------------------------
struct Plan {
  int tiles_a, tiles_b, split_cap, splits, nblocks;
  size_t search_bytes, off_state, off_rows, off_part, off_sum, off_cnt, bytes;
};

Plan make_plan(int N, int D, int C) {
  Plan p;
  p.tiles_a = rsp_cdiv(C, KM_BA);
  p.tiles_b = rsp_cdiv(D, KM_BB);
  p.split_cap = rsp_cdiv(KM_TARGET_BLOCKS, p.tiles_a * p.tiles_b);
  p.splits = km_splits(p.split_cap, N);
  p.nblocks = rsp_cdiv(N, KM_ROWS);
  p.search_bytes = rsp_cosine_topk_workspace(N, C, D, 1, 0);
  p.off_state = rsp_align_up(p.search_bytes, 256);
  p.off_rows = p.off_state + 256;
  p.off_part = p.off_rows + rsp_align_up((size_t)N * sizeof(int), 256);
  p.off_sum = p.off_part + rsp_align_up((size_t)p.nblocks * sizeof(KmPartial), 256);
  p.off_cnt = p.off_sum + rsp_align_up((size_t)p.splits * C * D * sizeof(float), 256);
  p.bytes = p.off_cnt + rsp_align_up((size_t)p.splits * C * sizeof(int), 256);
  return p;
}

bool sizes_ok(int N, int D, int C) {
  return N >= 1 && N <= 262144 && D >= 2 && D <= 4096 && D % 2 == 0 && C >= 1 && C <= 1024;
}

int fail(const char* who, const char* what, int code) {
  char buf[200];
  snprintf(buf, sizeof buf, "%s: %s", who, what);
  rsp_set_error(buf);
  return code;
}

bool aligned(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

}  // namespace

size_t rsp_kmeans_workspace(int32_t N, int32_t D, int32_t C) { return sizes_ok(N, D, C) ? make_plan(N, D, C).bytes : 0; }

int rsp_kmeans_fit(const float* x, int32_t ld, int32_t N, int32_t D, float* cent, int32_t C, int32_t max_iters, int32_t* assign,
                   int32_t* counts, int32_t* changed_trace, double* objective_trace, rsp_kmeans_info* info, void* workspace,
                   size_t workspace_bytes, void* stream) {
  const char* who = "rsp_kmeans_fit";
  if (!x || !cent || !assign || !counts || !changed_trace || !objective_trace || !info || !workspace)
    return fail(who, "null pointer", RSP_EINVAL);
  if (!(sizes_ok(N, D, C) && ld >= D && ld % 2 == 0))
    return fail(who, "bad size (1 <= N <= 262144, 2 <= D <= 4096, D and ld even, ld >= D, 1 <= C <= 1024)", RSP_EINVAL);
  if (!(max_iters >= 1 && max_iters <= 1000)) return fail(who, "max_iters must be in [1, 1000]", RSP_EINVAL);
  if (!aligned(x, 8) || !aligned(cent, 8) || !aligned(objective_trace, 8) || !aligned(info, 8) || !aligned(workspace, 8))
    return fail(who, "x, cent, objective_trace, info and the workspace must be 8-byte aligned", RSP_EINVAL);
  if (!aligned(assign, 4) || !aligned(counts, 4) || !aligned(changed_trace, 4))
    return fail(who, "assign, counts and changed_trace must be 4-byte aligned", RSP_EINVAL);
  const Plan p = make_plan(N, D, C);
  if (workspace_bytes < p.bytes) return fail(who, "workspace too small", RSP_EWORKSPACE);
  hipStream_t s = (hipStream_t)stream;
  char* ws = reinterpret_cast<char*>(workspace);
  KmState* st = reinterpret_cast<KmState*>(ws + p.off_state);
  int* rows = reinterpret_cast<int*>(ws + p.off_rows);
  KmPartial* part = reinterpret_cast<KmPartial*>(ws + p.off_part);
  float* sumpart = reinterpret_cast<float*>(ws + p.off_sum);
  int* cntpart = reinterpret_cast<int*>(ws + p.off_cnt);

  for (int t = 0; t < max_iters; ++t) {
    // the first search runs ungated (the state is reset behind it) and leaves the inverse norms of x for all later ones
    CosLists lists;
    int rc = rsp_cos_search_gated(who, x, ld, N, cent, D, C, D, 1, 0, workspace, p.search_bytes, s, &lists, t ? &st->stop : nullptr, t == 0);
    if (rc != RSP_OK) return rc;
    if (t == 0) {
      hipLaunchKernelGGL(km_compact_kernel, dim3(1), dim3(256), 0, s, lists.inv_q, (int)N, rows, (int*)assign, st);
      rc = rsp_check_launch("km_compact_kernel");
      if (rc != RSP_OK) return rc;
    }
    hipLaunchKernelGGL(km_assign_kernel, dim3(p.nblocks), dim3(256), 0, s, (const float*)lists.val, (const int*)lists.idx, lists.splits,
                       (int)N, (const int*)rows, (const KmState*)st, t, (int*)assign, part);
    rc = rsp_check_launch("km_assign_kernel");
    if (rc != RSP_OK) return rc;
    hipLaunchKernelGGL(km_step_kernel, dim3(1), dim3(64), 0, s, (const KmPartial*)part, st, t, (int*)changed_trace, objective_trace);
    rc = rsp_check_launch("km_step_kernel");
    if (rc != RSP_OK) return rc;
    hipLaunchKernelGGL(km_update_kernel, dim3(p.tiles_a * p.tiles_b, p.splits), dim3(256), 0, s, x, (int)ld, (int)D, lists.inv_q,
                       (const int*)rows, (const int*)assign, (const KmState*)st, (int)C, p.tiles_b, p.split_cap, sumpart, cntpart);
    rc = rsp_check_launch("km_update_kernel");
    if (rc != RSP_OK) return rc;
    hipLaunchKernelGGL(km_reduce_kernel, dim3(C, rsp_cdiv(D, 256)), dim3(256), 0, s, (const float*)sumpart, (const int*)cntpart,
                       (const KmState*)st, p.split_cap, (int)C, (int)D, cent, (int*)counts);
    rc = rsp_check_launch("km_reduce_kernel");
    if (rc != RSP_OK) return rc;
  }
  hipLaunchKernelGGL(km_finish_kernel, dim3(1), dim3(256), 0, s, (const KmState*)st, (int)N, (int)C, (int)max_iters, (const int*)counts,
                     (int*)changed_trace, objective_trace, info);
  return rsp_check_launch("km_finish_kernel");
}

int rsp_kmeans_assign(const float* x, int32_t ld, int32_t N, int32_t D, const float* cent, int32_t C, int32_t* assign, float* sim,
                      void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "rsp_kmeans_assign";
  if (!x || !cent || !assign || !workspace) return fail(who, "null pointer", RSP_EINVAL);
  if (!(sizes_ok(N, D, C) && ld >= D && ld % 2 == 0))
    return fail(who, "bad size (1 <= N <= 262144, 2 <= D <= 4096, D and ld even, ld >= D, 1 <= C <= 1024)", RSP_EINVAL);
  if (!aligned(x, 8) || !aligned(cent, 8) || !aligned(workspace, 8) || !aligned(assign, 4) || !aligned(sim, 4))
    return fail(who, "x, cent and the workspace must be 8-byte aligned, assign and sim 4-byte", RSP_EINVAL);
  hipStream_t s = (hipStream_t)stream;
  CosLists lists;
  int rc = rsp_cos_search(who, x, ld, N, cent, D, C, D, 1, 0, workspace, workspace_bytes, s, &lists);
  if (rc != RSP_OK) return rc;
  hipLaunchKernelGGL(km_assign_rows_kernel, dim3(rsp_cdiv(N, 256)), dim3(256), 0, s, (const float*)lists.val, (const int*)lists.idx,
                     lists.splits, (int)N, lists.inv_q, (int*)assign, sim);
  return rsp_check_launch("km_assign_rows_kernel");
}

int rsp_contingency(const int32_t* assign, const int64_t* y, int32_t N, int32_t C, int32_t L, int64_t* table, int64_t* dropped,
                    void* stream) {
  const char* who = "rsp_contingency";
  if (!assign || !y || !table || !dropped) return fail(who, "null pointer", RSP_EINVAL);
  if (!(N >= 1 && N <= 262144 && C >= 1 && C <= 1024 && L >= 1 && L <= 1024))
    return fail(who, "bad size (1 <= N <= 262144, 1 <= C <= 1024, 1 <= L <= 1024)", RSP_EINVAL);
  if (!aligned(assign, 4) || !aligned(y, 8) || !aligned(table, 8) || !aligned(dropped, 8))
    return fail(who, "assign must be 4-byte aligned, y, table and dropped 8-byte", RSP_EINVAL);
  hipStream_t s = (hipStream_t)stream;
  const long long total = (long long)C * L;
  unsigned long long* tab = reinterpret_cast<unsigned long long*>(table);
  unsigned long long* drp = reinterpret_cast<unsigned long long*>(dropped);
  hipLaunchKernelGGL(contingency_zero_kernel, dim3(rsp_cdiv(total, 256) < 2048 ? rsp_cdiv(total, 256) : 2048), dim3(256), 0, s, total,
                     tab, drp);
  int rc = rsp_check_launch("contingency_zero_kernel");
  if (rc != RSP_OK) return rc;
  hipLaunchKernelGGL(contingency_count_kernel, dim3(rsp_cdiv(N, 256) < 2048 ? rsp_cdiv(N, 256) : 2048), dim3(256), 0, s, assign,
                     reinterpret_cast<const long long*>(y), (int)N, (int)C, (int)L, tab, drp);
  return rsp_check_launch("contingency_count_kernel");
}
