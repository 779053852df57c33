// Shared helpers for librspnet_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <tuple>

#include "rspnet_hip.h"

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

#define RSP_WAVE 64

void rsp_set_error(const char* msg);
void rsp_note_reset(void);                    // arm the per-call kernel-name note (errors.hip)
void rsp_note_kernel(const char* fmt, ...);    // first matrix kernel launched since the last reset

static inline int rsp_check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    char buf[256];
    snprintf(buf, sizeof buf, "%.*s: %s", (int)strcspn(what, "<"), what, hipGetErrorString(e));      // (a name, or a note format: up to its '<')
    rsp_set_error(buf);
    return RSP_ELAUNCH;
  }
  return RSP_OK;
}

// Planning options of the convolution launchers: the one table behind rsp_conv3d_set_option (conv_options.hip).  Columns: enum
// constant, option name, environment variable, flag (1: the variable counts as set when present, whatever its value) or integer
// (0: atoi), built-in default.  The planning functions look an option up by its constant: one relaxed atomic load + the cached
// environment value, no string comparison on the launch path.
#define RSP_CONV_OPTIONS(X)                                                             \
  X(OPT_NARROW_MAX_TILES, "narrow_max_tiles", "RSP_NARROW_MAX_TILES", 0, 512)           \
  X(OPT_NARROW32_MAX_UNITS, "narrow32_max_units", "RSP_NARROW32_MAX_UNITS", 0, 256)     \
  X(OPT_TALL_MIN_TILES, "tall_min_tiles", "RSP_TALL_MIN_TILES", 0, 0)                   \
  X(OPT_TWO_LEVEL_MIN_CHUNKS, "two_level_min_chunks", "RSP_TWO_LEVEL_MIN_CHUNKS", 0, 0) \
  X(OPT_DIRECT_MAX_TILES, "direct_max_tiles", "RSP_DIRECT_MAX_TILES", 0, 0)             \
  X(OPT_NO_PERSIST, "no_persist", "RSP_NO_PERSIST", 1, 0)                               \
  X(OPT_NO_HALF_BLOCK, "no_half_block", "RSP_NO_HALF_BLOCK", 1, 0)                      \
  X(OPT_NO_PAD_SKIP, "no_pad_skip", "RSP_NO_PAD_SKIP", 1, 0)                            \
  X(OPT_NO_DMAJOR, "no_dmajor", "RSP_NO_DMAJOR", 1, 0)                                  \
  X(OPT_NO_TM_SKIP, "no_tm_skip", "RSP_NO_TM_SKIP", 1, 0)                               \
  X(OPT_NO_MULTI_SPLIT, "no_multi_split", "RSP_NO_MULTI_SPLIT", 1, 0)
#define RSP_OPTION_ID(id, name, env, flag, dflt) id,
enum RspConvOption { RSP_CONV_OPTIONS(RSP_OPTION_ID) RSP_OPT_COUNT };
#undef RSP_OPTION_ID
int rsp_conv_option(RspConvOption id);      // the effective value: set_option's if >= 0, else the environment's, else the default

// Launch (256 threads) of a kernel instance whose dynamic LDS can exceed the default limit.  KERNEL is a template argument, so
// the "attribute raised" flag is the instance's own: hipFuncAttributeMaxDynamicSharedMemorySize goes to lds_max on its first launch.
// `args`: the kernel's arguments (std::tie); `fmt, note...`: how the instance is spelled (rsp_note_kernel).
template <auto KERNEL, class... Args, class... Note>
int rsp_launch_lds(dim3 grid, size_t lds, size_t lds_max, hipStream_t s, const std::tuple<Args...>& args, const char* fmt, Note... note) {
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max);
    attr_set = true;
  }
  rsp_note_kernel(fmt, note...);
  std::apply([&](const auto&... a) { hipLaunchKernelGGL(KERNEL, grid, dim3(256), lds, s, a...); }, args);
  return rsp_check_launch(fmt);
}

// The same launch without the note, for the kernels outside the convolution launchers (repr_stats.hip, linear_probe.hip: the note is
// what rsp_last_conv_kernel reads): the attribute goes to `lds` on the instance's first launch, so a capture comes after one eager call.
template <auto KERNEL, class... Args>
int launch_lds(const char* name, dim3 grid, size_t lds, hipStream_t s, Args... args) {
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr_set = true;
  }
  hipLaunchKernelGGL(KERNEL, grid, dim3(256), lds, s, args...);
  return rsp_check_launch(name);
}

#define RSP_REQUIRE(cond, msg)     \
  do {                             \
    if (!(cond)) {                 \
      rsp_set_error(msg);          \
      return RSP_EINVAL;           \
    }                              \
  } while (0)

static inline size_t rsp_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline int rsp_cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
static inline bool rsp_aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// Bijective XCD-aware block remap (cdna_hip_programming.md §5 "XCD swizzle must be bijective"):
// blocks b and b+8 share an XCD; give each XCD a contiguous chunk of tile ids so neighbouring tiles
// (which share input halos / weight panels) hit the same 4 MiB L2.
__device__ __forceinline__ int rsp_xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7;
  const int xcd = bid & 7;
  const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + (bid >> 3);
}

__device__ __forceinline__ float rsp_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ int rsp_wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double rsp_wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float rsp_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// Non-finite values propagate as in the reference's torch ops (no fast-math in the build: `v != v` is the NaN test).  For operands
// that are not NaN each helper computes what the expression it replaces computed, to the bit.
//   rsp_max_nan        IEEE 754-2019 maximum — one v_maximum3_f32 on gfx950: NaN if either operand is NaN, else fmaxf's result
//                      (-0 < +0 included).  The scan step of max_pool3d, `(v > best) || isnan(v)`, where only the value is kept.
//   rsp_relu           torch.relu: maximum(z, 0), NaN stays NaN (fmaxf(NaN, 0) is 0)
//   rsp_relu_blocks    ReLU's backward (threshold_backward): the gradient is dropped where the activation input is <= 0 — a NaN
//                      input passes it on (`!(z > 0)` would drop it)
//   rsp_max_takes      the same scan step for value and arg-max together: a NaN displaces whatever is held, a later NaN displaces
//                      an earlier one, nothing else displaces a NaN
//   rsp_max_displaced  input-centric form of the scan: whether window element `v`, scanned earlier / later than `mine`, takes the
//                      window from `mine` (first maximum in scan order; with NaNs in the window the last NaN holds it)
__device__ __forceinline__ float rsp_max_nan(float best, float v) { return __builtin_elementwise_maximum(best, v); }
__device__ __forceinline__ float rsp_relu(float z) { return __builtin_elementwise_maximum(z, 0.f); }
__device__ __forceinline__ bool rsp_relu_blocks(float z) { return z <= 0.f; }
__device__ __forceinline__ bool rsp_max_takes(float v, float best) { return v > best || v != v; }
__device__ __forceinline__ bool rsp_max_displaced(bool earlier, float v, float mine) {
  const bool vn = v != v, mn = mine != mine;
  return earlier ? (!mn && (vn || v >= mine)) : (vn || (!mn && v > mine));
}

// Division by a launch constant as multiply-high + shift (the prologue of every tile decodes 4 GEMM rows per thread into
// (n, d, h, w) and its k position into (tap, channel): with hardware-free integer division that was ~1000 instructions
// per wave).  Exact for 0 <= n < 2^31: mul = ceil(2^(31+s) / d), s = ceil(log2 d); q = umulhi(n, mul) >> (s - 1).
struct FastDiv {
  unsigned mul;   // 0: divisor 1
  unsigned shr;
  int d;
};

static inline FastDiv fastdiv_make(int d) {
  FastDiv f = {0u, 0u, d};
  if (d <= 1) return f;
  int s = 0;
  while ((1ll << s) < d) ++s;
  const unsigned long long pw = 1ull << (31 + s);
  f.mul = (unsigned)((pw + (unsigned long long)d - 1) / (unsigned long long)d);
  f.shr = (unsigned)(s - 1);
  return f;
}

__device__ __forceinline__ int fastdiv(int n, const FastDiv f) {
  return f.mul ? (int)(__umulhi((unsigned)n, f.mul) >> f.shr) : n;
}
