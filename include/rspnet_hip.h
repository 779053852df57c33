/*
 * rspnet_hip.h — C ABI of librspnet_hip.so: the MI355X (gfx950) kernels behind RSPNet's pretext hot path.
 *
 * The reference (PeihaoChen/RSPNet) has NO native interface: every op on the path is an ATen call made from
 * Python.  Each entry point below therefore cites the *reference call site* whose ATen op
 * it replaces; the Python binding a maintainer would add is the ctypes stub shown in INTEGRATION.md (our own
 * host side, rspnet_amd/_lib.py, is exactly that stub).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 unless its type says otherwise; tensors are dense NDHWC
 *     ("rows" = N*D*H*W positions, channels contiguous, row pitch given by an `ld` argument in floats);
 *   - weights cross the boundary in the reference's own layout (Cout,Cin,kT,kH,kW) (nn.Conv3d.weight,
 *     SURVEY.md §A.5) and are re-packed on device by rsp_conv3d_pack_*;
 *   - `stream` is a hipStream_t passed as void*; calls only enqueue work (no sync, no allocation: graph-capturable);
 *   - return value: 0 = ok, negative = RSP_E* (see rsp_strerror); nothing is written on a negative return.
 */
#ifndef RSPNET_HIP_H
#define RSPNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSP_OK 0
#define RSP_EINVAL (-1)      /* bad geometry / null pointer / misaligned pointer */
#define RSP_EWORKSPACE (-2)  /* workspace too small */
#define RSP_ELAUNCH (-3)     /* hipLaunch error (hipGetLastError text via rsp_last_error) */
#define RSP_EUNSUPPORTED (-4)

const char* rsp_strerror(int code);
const char* rsp_last_error(void);
/* Demangled template instance of the FIRST matrix kernel the calling thread's most recent rsp_conv3d_{fwd,dgrad,dgrad_packed,
 * wgrad} call launched (written by the launcher itself; "" if the call launched none).  Cross-checks rsp_conv3d_kernel_name. */
const char* rsp_last_conv_kernel(void);
/* ABI version.  130 folded every operation's suffixed variants (_v, _x, _t, _g, _gate_) into ONE entry point under the plain name
 * with the full argument list, and dropped the stand-alone per-channel statistics pass that no convolution on the path needed: a
 * binding written against 120 must be re-checked against the declarations below. */
int rsp_version(void);

/* ---------------------------------------------------------------------------------------------------------
 * 3-D convolution (nn.Conv3d, groups=1, dilation=1): models/c3d.py:21-52, models/resnet.py:20-28,131-138,
 * models/s3dg.py:19-20,48-51,60, models/r2plus1d_vcop.py:54-55,66-67.
 * x: [N,Di,Hi,Wi,(in_ld)]  y: [N,Do,Ho,Wo,(out_ld)]  with Do = (Di+2pT-kT)/sT+1 ...
 * ------------------------------------------------------------------------------------------------------- */
typedef struct rsp_conv3d_desc {
  int32_t N, Di, Hi, Wi, Cin;
  int32_t Do, Ho, Wo, Cout;
  int32_t kT, kH, kW;
  int32_t sT, sH, sW;
  int32_t pT, pH, pW;
  int32_t in_ld;   /* floats between consecutive positions of x (>= Cin; lets x be a channel slice) */
  int32_t out_ld;  /* same for y */
} rsp_conv3d_desc;

/* Number of floats of the packed forward weight.  The layout is private to the library and chosen per descriptor
 * ([Cout][taps][Cin] with K padded to a multiple of 4 for the implicit-GEMM kernel, [taps][64][4] for the 4-channel stem
 * kernel); pack and forward must be called with the same descriptor. */
size_t rsp_conv3d_packed_fwd_elems(const rsp_conv3d_desc* d);
/* (Cout,Cin,kT,kH,kW) -> forward-packed. */
int rsp_conv3d_pack_fwd(const rsp_conv3d_desc* d, const float* w_ref, float* w_packed, void* stream);

/* Number of stat tiles of the output grid (128-row tiles, or 8x16 output patches on the stem path): stat partials are
 * [tiles][Cout][2] (sum, sum of squares of the bias-free conv output) — consumed by rsp_bn_finalize.  */
int32_t rsp_conv3d_stat_tiles(const rsp_conv3d_desc* d);
size_t rsp_conv3d_fwd_workspace(const rsp_conv3d_desc* d);
/* y = conv(x, w) + bias.  bias and stat_partials may be NULL. */
int rsp_conv3d_fwd(const rsp_conv3d_desc* d, const float* x, const float* w_packed, const float* bias, float* y,
                   float* stat_partials, void* workspace, size_t workspace_bytes, void* stream);

/* Forward of a stem whose output is only ever read through BatchNorm -> ReLU -> MaxPool3d(1,2,2) by a pass that keeps nothing for
 * a backward (the key passes): instead of y, the kernel writes the maximum and the minimum of conv(x, w) + bias over each (1,2,2)
 * window, [N][Do][Ho/2][Wo/2][Cout] each (a NaN in the window makes both NaN); stat_partials are those of rsp_conv3d_fwd, bit for
 * bit.  BatchNorm apply and ReLU are monotone per channel, so rsp_bn_act_minmax_fwd on the pair gives what rsp_bn_act_pool_fwd gives
 * on y.  Covered (applicable != 0): descriptors on the resident 4-channel stem kernel with 8x16 patches, even Ho and Wo, Cout a
 * multiple of 4; w_packed is the forward-packed weight of the same descriptor. */
int rsp_conv3d_stem_pooled_applicable(const rsp_conv3d_desc* d);
int rsp_conv3d_stem_pooled_fwd(const rsp_conv3d_desc* d, const float* x, const float* w_packed, const float* bias, float* y_max,
                               float* y_min, float* stat_partials, void* stream);

/* dgrad: dx = conv_transpose(dy, w).  Replaces autograd's conv backward-input for every conv on the path
 * (loss.backward(), pretrain.py:164).  w_ref in reference layout; packs per stride-parity class into workspace. */
size_t rsp_conv3d_dgrad_workspace(const rsp_conv3d_desc* d);
int rsp_conv3d_dgrad(const rsp_conv3d_desc* d, const float* dy, const float* w_ref, float* dx, void* workspace,
                     size_t workspace_bytes, void* stream);

/* dgrad over weights already re-packed into the per-stride-class layouts (rsp_conv3d_pack_jobs(which = 1) + rsp_pack_run):
 * the workspace then only holds the K-split partials (rsp_conv3d_dgrad_workspace(d) is always enough).
 * rsp_conv3d_packed_dgrad_elems is an upper bound: the jobs write the sum of their O x Kld floats from w_packed on and the rest of
 * the buffer is neither written nor read (it may stay uninitialised; tests/test_pack_gpu.py keeps NaNs there). */
size_t rsp_conv3d_packed_dgrad_elems(const rsp_conv3d_desc* d);
int rsp_conv3d_dgrad_packed(const rsp_conv3d_desc* d, const float* dy, const float* w_packed, float* dx, void* workspace,
                            size_t workspace_bytes, void* stream);

/* Batched weight re-pack.  The weights change once per step (torch.optim.SGD step, pretrain.py:165; momentum update of the key
 * encoder, builder_diffspeed_diffloss.py:337-343), so every convolution's packed copy is rebuilt once per step: instead of one
 * small launch per convolution (and per dgrad stride class) the host describes the re-packs once — the weight and packed
 * buffers do not move — uploads the array, and replays it with ONE launch per step and encoder.
 *   rsp_conv3d_pack_jobs: fills (host memory) the jobs that re-pack w_ref (reference layout (Cout_src, Cin_src, kT, kH, kW)) into
 *     w_packed for descriptor d; d->Cout / d->Cin may exceed the source dims, the excess is zero (channel padding, e.g. the
 *     3 -> 4 channel stems; for those the library notes, per w_packed address, that the filters have three real input channels, and
 *     rsp_conv3d_fwd on that buffer skips the zero fourth channel's multiply-adds).  which = 0: forward layout (1 job,
 *     rsp_conv3d_packed_fwd_elems floats); which = 1: all dgrad
 *     stride-class layouts (<= sT*sH*sW jobs, rsp_conv3d_packed_dgrad_elems floats).  Returns the number of jobs or RSP_E*.
 *   rsp_pack_run: executes n_jobs jobs stored in DEVICE memory; max_blocks = the largest `blocks` field among them (grid.x).
 *   rsp_conv3d_pack_forget: the owner of a packed buffer calls this before releasing it: the library drops what it noted about
 *     that address (the three-channel mark of a stem), so that an unrelated buffer which later lands on the same address never
 *     inherits it (an unmarked stem buffer runs all four channel steps: always correct). */
typedef struct rsp_pack_job {
  const void* src;
  void* dst;
  int64_t total;
  int32_t kind, Cout_src, Cin_src, kT, kH, kW;
  int32_t transpose, O, C, Kld, nTd, nTh, nTw, k0d, k0h, k0w, kstepd, ksteph, kstepw, ntaps;
  int32_t blocks, reserved;   /* workgroups this job needs (one per packed row) */
} rsp_pack_job;
int32_t rsp_conv3d_pack_jobs(const rsp_conv3d_desc* d, int32_t which, int32_t Cout_src, int32_t Cin_src, const float* w_ref,
                             float* w_packed, rsp_pack_job* jobs, int32_t max_jobs);
int rsp_pack_run(const rsp_pack_job* jobs_device, int32_t n_jobs, int32_t max_blocks, void* stream);
void rsp_conv3d_pack_forget(const void* w_packed);

/* wgrad: dw (reference layout, overwritten) = sum over positions of dy ⊗ im2col(x); dbias (nullable) = sum dy.
 *   cout_valid, cin_valid: the parameter's own channel counts.  A convolution may run with its channels zero padded in the
 *     descriptor (d->Cout / d->Cin) but not in the parameter: dw_ref is (cout_valid, cin_valid, kT, kH, kW) and the gradients of the
 *     padding channels are dropped.  Unpadded: pass d->Cout and d->Cin.  dbias only with unpadded channels.
 *   rowgeom_table (nullable): the kernels stream a per-row geometry table (input byte offset + padding-validity bits of each output
 *     position: a function of the geometry alone).  With NULL it is computed in a pre-pass of the call, in the workspace; a caller
 *     that keeps one table per geometry (rsp_conv3d_rowgeom_bytes, rsp_conv3d_rowgeom: one launch, once) passes it here and saves
 *     that launch — 59 per S3D-G step.
 * workspace and table 16-byte aligned. */
size_t rsp_conv3d_wgrad_workspace(const rsp_conv3d_desc* d);
size_t rsp_conv3d_rowgeom_bytes(const rsp_conv3d_desc* d);
int rsp_conv3d_rowgeom(const rsp_conv3d_desc* d, void* table, void* stream);
int rsp_conv3d_wgrad(const rsp_conv3d_desc* d, const float* x, const float* dy, float* dw_ref, float* dbias, int32_t cout_valid,
                     int32_t cin_valid, const void* rowgeom_table, void* workspace, size_t workspace_bytes, void* stream);

/* Name of the kernel template instance the library launches for this descriptor (which: 0 forward, 1 dgrad, 2 wgrad;
 * 16-byte aligned tensors assumed) -- lets bench.py label its roofline block with the kernel that actually dominates a
 * backbone and match it to the rocprofv3 kernel-trace row.  Static string, never NULL. */
const char* rsp_conv3d_kernel_name(const rsp_conv3d_desc* d, int which);

/* Share (0..1] of the convolution's algorithmic multiply-adds — 2*MACs counted with the taps that read the zero padding, as
 * cuDNN / oneDNN under the reference's nn.Conv3d count them (models/c3d.py:21-52) — that the launched kernels actually execute:
 * the implicit-GEMM walks skip K chunks (forward / dgrad) and row chunks (wgrad) that are padding for a whole tile.  Host
 * arithmetic only (the kernels' own planning code), no GPU.  which: 0 forward, 1 dgrad, 2 wgrad (frame-granular estimate).
 * bench.py prices roofline.executed_frac with it next to the algorithmic rate. */
double rsp_conv3d_executed_fraction(const rsp_conv3d_desc* d, int which);

/* Planning options of the convolution launchers, settable at run time (process-wide; host arithmetic only: which kernel instance and
 * which K split a descriptor gets — every choice computes the same convolution, in another summation order).  One table (csrc/common.h
 * RSP_CONV_OPTIONS) holds each option's name, environment variable and default.  An option's value is what was stored here (>= 0),
 * else its environment variable (read once per process; an integer through atoi, a flag set when the variable is present at all),
 * else the default; a value < 0 goes back to the environment / the default.  Returns the previous EFFECTIVE value, or RSP_EINVAL
 * ("unknown option") for a name that is not in the table.
 *   "narrow_max_tiles"    launches of fewer than this many 128-wide tiles (and 97..128 or > 160 columns) run on the 64-wide tile
 *                         (default 512, environment RSP_NARROW_MAX_TILES; 0: never; < 0: back to the default).
 *   "narrow32_max_units"  launches of at most this many 128 x 64 tiles (more than 32 columns, K of at least 8 chunks) run on the
 *                         32-wide tile with the whole K per unit instead of a K split + reduce launch (default 256, environment
 *                         RSP_NARROW32_MAX_UNITS; 0: never; < 0: back to the default).
 *   "tall_min_tiles"      33..64-column launches of at least this many 256-row tiles run on the 256 x 64 instance of the persistent
 *                         kernel (default 0 = never: measured neutral-to-negative per step in round 6; environment
 *                         RSP_TALL_MIN_TILES; < 0: back to the default).
 *   "two_level_min_chunks" slice-major 128-wide launches of at least this many 32-deep K chunks sum K in panels of 512 products
 *                         (a second accumulator set, two waves per SIMD): the CPU convolution's error level on the long-K layers
 *                         (default 0 = never: priced in round 6; environment RSP_TWO_LEVEL_MIN_CHUNKS).
 *   "direct_max_tiles"    launches of at most this many 128 x 128 tiles with Cin % 16 == 0 run on igemm_direct_kernel (default 0 =
 *                         never: superseded by the 64-wide tiles; environment RSP_DIRECT_MAX_TILES).
 * Flags (default 0; 1 switches the fast path off, for A/B measurements):
 *   "no_persist"          RSP_NO_PERSIST       per-tile instead of persistent implicit-GEMM kernels
 *   "no_half_block"       RSP_NO_HALF_BLOCK    the 160-wide / 32-row instances instead of those with a 16-wide MFMA block
 *   "no_pad_skip"         RSP_NO_PAD_SKIP      no skipping of K chunks / row chunks that fall into the padding
 *   "no_dmajor"           RSP_NO_DMAJOR        no depth-major row order
 *   "no_tm_skip"          RSP_NO_TM_SKIP       no dead-tap skipping on the tap-major walk
 *   "no_multi_split"      RSP_NO_MULTI_SPLIT   few-tile strided input gradients: no common K split of the classes that share a launch
 * Used by the kernel tests (an instance at sizes the checker finishes in seconds) and by tools/geom_bench.py (A/B of a plan in one
 * process).  The whole-step parity tests run under the DEFAULT plan only. */
int rsp_conv3d_set_option(const char* name, int32_t value);

/* Host evaluation of the constant division the conv kernels use to decode GEMM rows and k positions (multiply-high by a
 * host-computed magic number + shift, exact for 0 <= n < 2^31): returns n / d computed that way.  No GPU needed; exists so
 * the CPU test suite can check the derivation over the full range. */
int rsp_fastdiv_check(int d, int n);

/* ---------------------------------------------------------------------------------------------------------
 * BatchNorm3d (train mode) fused with ReLU / residual add / MaxPool3d:
 * models/c3d.py:22-24 (bn+relu+pool), models/resnet.py:61-77, models/s3dg.py:23,28-33, r2plus1d_vcop.py:59-60,116-123.
 * ------------------------------------------------------------------------------------------------------- */
/* Reduce stat partials -> mean (incl. conv bias), invstd; update running stats
 * (running_var with the unbiased n/(n-1) estimate), as F.batch_norm(training=True) does.
 * count = number of positions per channel.  scale_shift out: [2][C] = (gamma*invstd, beta - mean*gamma*invstd).
 *   stat_ld (>= C) = channels per partial row: the C channels may be a slice of a wider convolution's partials (several
 *     BasicConv3d that share their input run as ONE GEMM over the concatenated filters, models/s3dg.py:80-88).
 *   c_valid: the parameter's own length.  A convolution may run with its output channels zero-padded from c_valid to C
 *     (models/r2plus1d_vcop.py:35-38: mid channel counts such as 83 / 230 / 921 run as 84 / 232 / 924 so that rows are 16 bytes
 *     aligned): conv_bias / gamma / beta / running_mean / running_var hold c_valid entries; channels [c_valid, C) get
 *     scale = shift = 0 and move no running statistic.  Unpadded: pass C.
 *   batch_stats_out (nullable): deferred running statistics.  When given, running_mean / running_var are NOT moved (both ignored)
 *     and this pass's batch moments are written instead — [2][c_valid]: mean (conv bias included), unbiased variance;
 *     rsp_bn_running_update later applies  r = (1 - momentum) r + momentum * moment  for a whole list of layers in one launch (jobs
 *     in device memory), the update nn.BatchNorm3d does inside forward.  The two key-encoder passes of a step
 *     (builder_diffspeed_diffloss.py:445,512) go through the SAME BatchNorm buffers; deferring the second pass's update lets the
 *     passes run side by side in a captured graph and still leaves the buffers as two consecutive forwards would. */
typedef struct rsp_bn_ema_job {
  float* running_mean;
  float* running_var;
  const float* batch_stats; /* [2][C] */
  int32_t C;
  float momentum;
} rsp_bn_ema_job;
size_t rsp_bn_finalize_workspace(int32_t tiles, int32_t C);
int rsp_bn_finalize(const float* stat_partials, int32_t tiles, int32_t C, int32_t c_valid, int32_t stat_ld, int64_t count,
                    const float* conv_bias, const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                    float* running_var, float* batch_stats_out, float* mean_invstd /*[2][C]*/, float* scale_shift /*[2][C]*/,
                    void* workspace, size_t workspace_bytes, void* stream);
int rsp_bn_running_update(const rsp_bn_ema_job* jobs_device, int32_t n_jobs, int32_t max_c, void* stream);

typedef struct rsp_pool3d_desc {
  int32_t N, Di, Hi, Wi, C;
  int32_t Do, Ho, Wo;
  int32_t kT, kH, kW, sT, sH, sW, pT, pH, pW; /* k=s=1,p=0: no pooling */
  int32_t in_ld, out_ld, res_ld;
} rsp_pool3d_desc;

/* out = maxpool(act(scale*y + shift (+ residual)) (* gate)) ; act = ReLU if relu!=0.  residual (nullable) has y's shape.
 *   gate (nullable): per-sample channel gates [N][C], multiplied in after the activation and before the max (see rsp_bn_gate_sums). */
int rsp_bn_act_pool_fwd(const rsp_pool3d_desc* d, const float* y, const float* scale_shift, const float* residual,
                        int relu, const float* gate, float* out, void* stream);

/* The ResNet stems' bn1 -> relu -> MaxPool3d(3, 2, 1) (models/resnet.py:139,203-207) — BatchNorm apply and an OVERLAPPING 3x3x3 or
 * 1x3x3 max-pool (any stride / padding) in one pass over the convolution output: out = maxpool(act(scale*y + shift) (* gate)); argmax
 * (nullable) as rsp_maxpool3d_fwd writes it (first maximum in scan order, linear input position per sample), so that
 * rsp_maxpool3d_bwd and then rsp_bn_act_pool_bwd (unit window) form its backward.  Bit-identical to rsp_bn_act_pool_fwd with a unit
 * window followed by rsp_maxpool3d_fwd; the activated tensor is neither written nor read.  rsp_bn_act_pool_fwd takes this path
 * itself for such windows (no residual).  Needs C, in_ld, out_ld multiples of 4 and 16-byte aligned pointers
 * (rsp_bn_act_maxpool_applicable).
 *   gate (nullable): S3D-G's per-sample channel gates [N][C], multiplied in between the activation and the pool
 *     (models/s3dg.py:105-108: the two front-end sep_conv units are followed by (1,3,3) / (1,2,2) max-pools): rsp_bn_gate_sums ->
 *     this, instead of rsp_bn_act_pool_fwd (unit window) -> rsp_maxpool3d_fwd; same bits. */
int rsp_bn_act_maxpool_applicable(const rsp_pool3d_desc* d);
int rsp_bn_act_maxpool_fwd(const rsp_pool3d_desc* d, const float* y, const float* scale_shift, int relu, const float* gate, float* out,
                           int32_t* argmax, void* stream);

/* Backward of the fused block, two launches:
 *  reduce: per-channel partial sums of dz and dz*xhat (dz = grad at the BN output after pool routing + ReLU mask)
 *  apply : dy = gamma*invstd*(dz - mean(dz) - xhat*mean(dz*xhat)); also d(residual) = dz (if dres != NULL),
 *          dgamma = sum(dz*xhat), dbeta = sum(dz).
 * The pooled activation is recomputed from y (saved conv output), never stored.
 *   c_valid: the parameter's own length, as in rsp_bn_finalize: gamma / dgamma / dbeta hold c_valid entries; the padding channels
 *     [c_valid, C) have gamma = 0.  Unpadded: pass d->C.
 *   gate, dmean (both or neither): the block sits behind an S3D-G self-gating unit whose forward kept no activation
 *     (rsp_bn_gate_sums, act == NULL): dout is the gradient of the GATED output; gate [N][C] from the forward, dmean [N][C] from
 *     rsp_gate_bwd_params.  Unit windows, no residual. */
size_t rsp_bn_bwd_workspace(const rsp_pool3d_desc* d);
int rsp_bn_act_pool_bwd(const rsp_pool3d_desc* d, const float* y, const float* residual, const float* dout,
                        const float* gamma, const float* mean_invstd, const float* scale_shift, int relu, float* dy,
                        float* dres, float* dgamma, float* dbeta, int32_t c_valid, const float* gate, const float* dmean,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Pooled units (disjoint windows of 4 or 8 positions, no residual, no gate; C, in_ld, out_ld multiples of 4 and 16-byte aligned
 * pointers: applicable != 0) whose forward is followed by a backward.  The forward also keeps y_sel [N][Do][Ho][Wo][C] (dense), the
 * raw y at the position of each window the backward's arg-max rule selects; `out` is rsp_bn_act_pool_fwd's, bit for bit.  The
 * backward's reduce pass then reads dout and y_sel instead of dout and all of y (its sums only involve the selected positions; the
 * others contribute exact zeros), with the same partial-sum partitioning: dy, dgamma, dbeta are rsp_bn_act_pool_bwd's bit for bit.
 * Workspace: rsp_bn_bwd_workspace(d). */
int rsp_bn_act_pool_sel_applicable(const rsp_pool3d_desc* d);
int rsp_bn_act_pool_sel_fwd(const rsp_pool3d_desc* d, const float* y, const float* scale_shift, int relu, float* out, float* y_sel,
                            void* stream);
int rsp_bn_act_pool_sel_bwd(const rsp_pool3d_desc* d, const float* y, const float* y_sel, const float* dout, const float* gamma,
                            const float* mean_invstd, const float* scale_shift, int relu, float* dy, float* dgamma, float* dbeta,
                            int32_t c_valid, void* workspace, size_t workspace_bytes, void* stream);

/* Second half of a stem unit after rsp_conv3d_stem_pooled_fwd: out = act(fma(scale, scale >= 0 ? y_max : y_min, shift)) per channel
 * over `positions` rows of C floats (out: pitch out_ld, so a channel slice of a wider tensor is a valid destination).  For scale == 0
 * both operands are evaluated and a NaN from either (0 * +-inf) is kept.  Equal to rsp_bn_act_pool_fwd on the full-size output under
 * ==, NaNs in the same places; the sign of a zero may differ.  Finite scales only. */
int rsp_bn_act_minmax_fwd(const float* y_max, const float* y_min, int64_t positions, int32_t C, int32_t out_ld,
                          const float* scale_shift, int relu, float* out, void* stream);

/* Eval-mode counterpart of rsp_bn_act_pool_bwd — BatchNorm on its running statistics — in ONE pass over y and dout:
 *   dz = gradient at the BatchNorm output after pool routing + ReLU mask, recomputed from y with the forward's tie rule
 *   dy = scale*dz (0 on the padding channels [c_valid, C)); d(residual) = dz (if dres != NULL)
 *   dgamma = sum(dz*xhat), dbeta = sum(dz), xhat = (y - mean')*invstd          (both nullable, c_valid entries)
 * scale_shift [2][C] is what the forward applied; mean_invstd [2][C] holds mean' = running_mean - conv_bias and
 * rsqrt(running_var + eps) and is read only when a parameter gradient is asked for.  With dgamma == dbeta == NULL no sums are
 * formed and neither mean_invstd nor the workspace is touched (frozen affine parameters).  Otherwise every workgroup writes its
 * partial sums to the workspace and one small launch adds them in a fixed order: no atomics, bit-identical run to run.  Same
 * geometry conventions as rsp_bn_act_pool_bwd (disjoint windows of any size, separate pitches for y / dout / residual). */
size_t rsp_bn_eval_bwd_workspace(const rsp_pool3d_desc* d);
int rsp_bn_eval_act_pool_bwd(const rsp_pool3d_desc* d, const float* y, const float* residual, const float* dout,
                             const float* mean_invstd, const float* scale_shift, int relu, float* dy, float* dres,
                             float* dgamma, float* dbeta, int32_t c_valid, void* workspace, size_t workspace_bytes,
                             void* stream);

/* Stand-alone MaxPool3d, any window/stride/padding (models/resnet.py:139, models/s3dg.py:90,107-119).
 * argmax (nullable in forward when no backward is needed): [N,Do,Ho,Wo,C] int32, linear input position per sample. */
int rsp_maxpool3d_fwd(const rsp_pool3d_desc* d, const float* x, float* out, int32_t* argmax, void* stream);
int rsp_maxpool3d_bwd(const rsp_pool3d_desc* d, const float* dout, const int32_t* argmax, float* dx, void* stream);

/* S3D-G self-gating (models/s3dg.py:63-72): out = x * sigmoid(W·mean_p(x) + b); x:[N][P][C] (pitch in_ld), W (C,C)
 * = excitation.weight viewed (C,C,1,1,1), b (C).  Saves mean [N][C] and gate [N][C] for backward. */
size_t rsp_gate_fwd_workspace(int32_t N, int32_t P, int32_t C);
int rsp_gate_fwd(const float* x, int32_t N, int32_t P, int32_t C, int32_t in_ld, const float* w, const float* b,
                 float* out, int32_t out_ld, float* mean, float* gate, void* workspace, size_t workspace_bytes,
                 void* stream);
/* The same unit with the gate's spatial mean taken by the kernel that applies the BatchNorm in front of it
 * (sep_conv = ... BasicConv3d -> excitation, models/s3dg.py:52-72): rsp_bn_gate_sums computes a = relu(y*scale + shift), its
 * per-(sample, channel) mean and the gate in one pass over y — storing a ([N][P][C], pitch act_ld) only when `act` is given (a
 * backward will read it) — and the gated output is then either rsp_gate_apply(a) or, without the stored activation,
 * rsp_bn_act_pool_fwd (with the gate) straight from y (optionally through the max-pool that follows the front-end units, s3dg.py:105-109).
 * Bit-identical to rsp_bn_act_pool_fwd + rsp_gate_fwd (+ rsp_maxpool3d_fwd).  Workspace: rsp_gate_fwd_workspace(N, P, C). */
int rsp_bn_gate_sums(const float* y, int32_t N, int32_t P, int32_t C, int32_t y_ld, const float* scale_shift, int relu,
                     float* act, int32_t act_ld, const float* w, const float* b, float* mean, float* gate, void* workspace,
                     size_t workspace_bytes, void* stream);
int rsp_gate_apply(const float* x, int32_t N, int32_t P, int32_t C, int32_t in_ld, const float* gate, float* out, int32_t out_ld,
                   void* stream);
/* Parameter half of the gating backward with the activation recomputed from y: dw (C,C), db (C) and dmean [N][C] (the data half
 * runs inside rsp_bn_act_pool_bwd).  Workspace: rsp_gate_bwd_workspace(N, P, C). */
int rsp_gate_bwd_params(const float* y, const float* scale_shift, int relu, const float* dout, int32_t N, int32_t P, int32_t C,
                        int32_t y_ld, int32_t dout_ld, const float* w, const float* mean, const float* gate, float* dw, float* db,
                        float* dmean, void* workspace, size_t workspace_bytes, void* stream);
size_t rsp_gate_bwd_workspace(int32_t N, int32_t P, int32_t C);
int rsp_gate_bwd(const float* x, const float* dout, int32_t N, int32_t P, int32_t C, int32_t x_ld, int32_t dout_ld,
                 const float* w, const float* mean, const float* gate, float* dx, int32_t dx_ld, float* dw, float* db,
                 void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Projection heads: AdaptiveAvgPool3d(1) -> Flatten -> Linear x2 -> F.normalize (moco/split_wrapper.py:138-152,163-169)
 * feat: [B][P][C] (ld = feat_ld).  w1,w2: (dim, C) row-major (nn.Linear.weight), b1,b2: (dim).
 * out: qa,qm [B][dim] unit-norm; saves pooled [B][C] and raw (pre-normalize) [2][B][dim] for backward.
 * ------------------------------------------------------------------------------------------------------- */
int rsp_head_fwd(const float* feat, int32_t B, int32_t P, int32_t C, int32_t feat_ld, const float* w1,
                 const float* b1, const float* w2, const float* b2, int32_t dim, float* out1, float* out2,
                 float* pooled, float* raw, void* stream);
size_t rsp_head_bwd_workspace(int32_t B, int32_t dim);
int rsp_head_bwd(const float* dout1, const float* dout2, const float* pooled, const float* raw, const float* w1,
                 const float* w2, int32_t B, int32_t P, int32_t C, int32_t feat_ld, int32_t dim, float* dw1,
                 float* db1, float* dw2, float* db2, float* dfeat, void* workspace, size_t workspace_bytes,
                 void* stream);

/* 'mlp' head variant (moco/split_wrapper.py:171-179: pool -> Linear(C,C) -> ReLU -> Linear(C,dim) -> F.normalize),
 * built from generic pieces.  x:[N][P][C] pitch ld; linear weights (Cout,Cin) row-major like nn.Linear.weight. */
int rsp_spatial_mean_fwd(const float* x, int32_t N, int32_t P, int32_t C, int32_t ld, float* mean, void* stream);
int rsp_spatial_mean_bwd(const float* dmean, int32_t N, int32_t P, int32_t C, int32_t ld, float* dx, void* stream);
int rsp_linear_fwd(const float* x, int32_t B, int32_t Cin, const float* w, const float* bias, int32_t Cout, int relu,
                   float* y, void* stream);
size_t rsp_linear_bwd_workspace(int32_t B, int32_t Cout);
/* y = forward output (for the ReLU mask); dx may be NULL. */
int rsp_linear_bwd(const float* x, const float* y, const float* dy, const float* w, int32_t B, int32_t Cin, int32_t Cout,
                   int relu, float* dx, float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream);
int rsp_l2norm_fwd(const float* x, int32_t B, int32_t dim, float* y, void* stream);
int rsp_l2norm_bwd(const float* x, const float* dy, int32_t B, int32_t dim, float* dx, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Contrastive block (moco/builder_diffspeed_diffloss.py:521-538) and Loss (:263-283).
 * logits1 = [qA.kA | qA@queue]/T, logits2 = [qA.knegA | qA@queue]/T  each [B][1+K];  lposM = qM.kM/T, lnegM = qM.knegM/T
 * queue: [dim][K] (register_buffer "queue", :329-330).  qA/kA/knegA are [B][dim]; qM/kM/knegM are [B][dim_m]
 * (dim_m == dim except for fc_type 'speednet', whose second head is 1-dimensional: moco/split_wrapper.py:124-126).
 * ------------------------------------------------------------------------------------------------------- */
int rsp_logits_fwd(const float* qA, const float* qM, const float* kA, const float* kM, const float* knegA,
                   const float* knegM, const float* queue, int32_t B, int32_t dim, int32_t dim_m, int32_t K, float inv_T,
                   float* logits1, float* logits2, float* lposM, float* lnegM, void* stream);
size_t rsp_logits_bwd_workspace(int32_t B, int32_t dim, int32_t K);
int rsp_logits_bwd(const float* dlogits1, const float* dlogits2, const float* dlposM, const float* dlnegM,
                   const float* kA, const float* kM, const float* knegA, const float* knegM, const float* queue,
                   int32_t B, int32_t dim, int32_t dim_m, int32_t K, float inv_T, float* dqA, float* dqM, void* workspace,
                   size_t workspace_bytes, void* stream);

/* losses[3] = (A*(ce1+ce2)+M*ranking, ce1+ce2, ranking); CE targets are class 0 (labels_A), ranking target +1.
 * Also writes the gradients for d(losses[0]) = 1: dlogits1/2 [B][1+K], dlpos/dlneg [B]. */
int rsp_loss_fwd_bwd(const float* logits1, const float* logits2, const float* lposM, const float* lnegM, int32_t B,
                     int32_t K1 /* = 1+K */, float margin, float A, float M, float* losses, float* dlogits1,
                     float* dlogits2, float* dlposM, float* dlnegM, float* row_scratch /*[2*B]*/, void* stream);

/* queue[:, ptr:ptr+n] = keys.T  (_dequeue_and_enqueue, :345-359); keys [n][dim]. */
int rsp_queue_enqueue(float* queue, int32_t dim, int32_t K, int32_t ptr, const float* keys, int32_t n, void* stream);
/* The same with the pointer in device memory: reads *ptr_dev (the module's int64 queue_ptr buffer, :332), writes the slab and
 * advances *ptr_dev by n modulo K (:356-359).  No host-side pointer: a step captured in a HIP graph replays correctly. */
int rsp_queue_enqueue_dev(float* queue, int32_t dim, int32_t K, int64_t* ptr_dev, const float* keys, int32_t n, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Step glue
 * ------------------------------------------------------------------------------------------------------- */
/* _diff_speed frame gather (:421-443) fused with the shuffle-BN sample permutation (:384-387) and the
 * NCDHW -> NDHWC layout change:  out[j] = im[src[j]][:, frames(step[j])], frames(s) = 0, s, 2s, ... (T_out of them).
 * im: (B_in, C, T_in, H, W) NCDHW as the reference's data loader hands it over; out: [B_out][T_out][H][W][C_out],
 * C_out >= C, extra channels zero (C_out = 4 lets a 3-channel stem convolution use 16-byte gathers). */
int rsp_clip_gather(const float* im, int32_t B_in, int32_t C, int32_t T_in, int32_t H, int32_t W, const int32_t* src,
                    const int32_t* step, int32_t B_out, int32_t T_out, int32_t C_out, float* out, void* stream);
/* The step's gathers in ONE launch: n_jobs (<= 4) gathers of identical geometry — the k_negative clips, the k clips (both in the
 * send order of their shuffle-BN exchange, :361-387) and the query clips (:421-447) — each with its own source batch, index and
 * speed vectors and output.  A launch that moves 0.5 GB streams at HBM rate; three launches of 0.18 GB each spend a fifth of their
 * 48 us on ramp-up and tail. */
int rsp_clip_gather_multi(int32_t n_jobs, const float* const* ims, const int32_t* const* srcs, const int32_t* const* steps,
                          float* const* outs, int32_t B_in, int32_t C, int32_t T_in, int32_t H, int32_t W, int32_t B_out, int32_t T_out,
                          int32_t C_out, void* stream);

/* _momentum_update_key_encoder (:337-343) on flat parameter buffers: k = k*m + q*(1-m). */
int rsp_momentum_update(float* k, const float* q, int64_t n, float m, void* stream);

/* torch.optim.SGD step (pretrain.py:65-72,165) on flat buffers: d = g*gscale + wd*p; buf = first ? d : mu*buf + d;
 * p -= lr*buf. */
int rsp_sgd_step(float* p, const float* g, float* buf, int64_t n, float lr, float mu, float wd, float gscale,
                 int first, void* stream);

/* Small element-wise ops on dense fp32 vectors (y may alias a or b):
 *   RSP_ELT_RELU_FWD     y = max(a, 0)              nn.ReLU between the two convs of ConvFc (moco/split_wrapper.py:31-34)
 *   RSP_ELT_RELU_BWD     y = a > 0 ? b : 0          its backward (a = forward output, b = incoming gradient)
 *   RSP_ELT_SIGMOID_FWD  y = 1 / (1 + exp(-a))      torch.sigmoid of the 'speednet' head (moco/split_wrapper.py:146-147)
 *   RSP_ELT_SIGMOID_BWD  y = b * a * (1 - a)        its backward (a = forward output)
 *   RSP_ELT_ADD          y = a + b                  autograd's gradient accumulation where a tensor has several consumers
 *                                                   (residual adds models/resnet.py:72-75, inception fan-out models/s3dg.py:93-99) */
#define RSP_ELT_RELU_FWD 0
#define RSP_ELT_RELU_BWD 1
#define RSP_ELT_SIGMOID_FWD 2
#define RSP_ELT_SIGMOID_BWD 3
#define RSP_ELT_ADD 4
int rsp_eltwise(int32_t op, const float* a, const float* b /* nullable for the *_FWD ops */, float* y, int64_t n, void* stream);

/* rows gather: out[j][:] = in[idx[j]][:]  (feature un-shuffle, :389-406). */
int rsp_rows_gather(const float* in, const int32_t* idx, int32_t n, int32_t width, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Per-clip GPU augmentation of the pretext data path, fused into one pass:
 *   ToTensorVideo -> Resize(size, bilinear, align_corners=False) -> RandomGrayScale -> ColorJitter (brightness, contrast,
 *   saturation, hue in a per-clip random order) -> RandomHorizontalFlipVideo -> NormalizeVideo
 * and the `moco.aug_plus` variant  ... -> RandomApply(ColorJitter) -> RandomGrayScale -> RandomApply(GaussianBlur 3x3) -> ...
 * (datasets/classification/__init__.py:189-218; transforms_spatial.py:16-25; transforms_tensor.py:12-34,52-143;
 *  functional_tensor.py:89-162,254-417; applied clip by clip in SequentialGPUCollateFn, transforms_tensor.py:207-233).
 * The random draws stay on the host (Python's `random`, same order as the reference); each clip is described by one
 * rsp_augment_clip_desc in DEVICE memory.  src is the uint8 (T,h,w,3) crop produced by RawVideoRandomCrop
 * (transforms_spatial.py:28-80), addressed through pitches so it may also point into a larger decoded frame.
 * out: float32 (n_clips, 3, T, size, size) -- the model's NCDHW input -- with `out_clip_stride` floats between clips.
 * ------------------------------------------------------------------------------------------------------- */
#define RSP_AUG_BRIGHTNESS 0
#define RSP_AUG_CONTRAST 1
#define RSP_AUG_SATURATION 2
#define RSP_AUG_HUE 3
typedef struct rsp_augment_clip_desc {
  const uint8_t* src;
  int64_t frame_pitch;   /* bytes between frames */
  int32_t row_pitch;     /* bytes between rows (pixels are 3 packed bytes) */
  int32_t h, w;          /* region height / width */
  int32_t gray, flip;    /* gray: 0 no, 1 RandomGrayScale hit BEFORE the colour ops (default chain), 2 AFTER them (aug_plus chain),
                            +4 GaussianBlur hit (aug_plus: 3x3 zero-padded blur of the intermediate image, before the flip);
                            flip: RandomHorizontalFlipVideo hit */
  int32_t n_ops;         /* 0..4 colour ops, applied in this order */
  int32_t op[4];         /* RSP_AUG_* */
  float factor[4];       /* (float)ratio, or the hue shift */
  float one_minus[4];    /* (float)(1.0 - ratio), evaluated in double as Python does (functional_tensor.py:103-106) */
} rsp_augment_clip_desc;
size_t rsp_augment_workspace(int32_t n_clips, int32_t T, int32_t size);
/* mean3 / std3 / blur9: HOST pointers to 3 / 3 / 9 floats (read during the call); blur9 = row-major 3x3 kernel of
 * transforms_tensor.py:GaussianBlur (:146-204), may be NULL when no descriptor has the blur bit. */
int rsp_augment_batch(const rsp_augment_clip_desc* descs, int32_t n_clips, int32_t T, int32_t size, const float* mean3,
                      const float* std3, const float* blur9, float* out, int64_t out_clip_stride, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Video retrieval search (cos_search.hip, retrieval.hip; the reference's retrieval.py:150-176).
 * q (Nq x D, row pitch ldq) and g (Ng x D, row pitch ldg): fp32 row-major, D and the pitches even, 8-byte aligned bases.
 * Writes for every query the k (1..64) nearest gallery rows by cosine distance d = clip(1 - q.g / (|q| |g|), 0, 2), best
 * first: idx (Nq x k, int32) and dist (Nq x k, fp32).  Ranking: fp32 similarity descending; an exact tie goes to the lower
 * gallery index.  A zero-norm row has similarity 0 (distance 1) to everything.  When Ng < k the tail slots hold index -1 and
 * distance +inf.  The Nq x Ng matrix is never stored.  splits: gallery ranges searched by separate workgroups and merged
 * (<= 0: chosen from the sizes; rsp_cosine_topk_splits tells the count used); the output does not depend on it, bit for bit.
 *
 * Non-finite rows (the same for rsp_knn_classify, any k, any split count).  The inverse norm of a row is 1 / sqrt(sum of squares) in
 * fp32 where that sum is positive and finite, and 0 otherwise: for a zero row, for a row holding a NaN or an Inf, and for a finite row
 * whose squares overflow fp32 (an element beyond about 1.8e19).  The similarity is (q.g) * (1/|q|) * (1/|g|) as always, so
 *   - a gallery row holding a NaN or an Inf has a NaN similarity to every query (NaN or +-inf times 0).  A NaN similarity never
 *     enters a list: such a row is never returned, and every other row is ranked exactly as if the gallery did not hold it -- the
 *     lists equal, bit for bit, those of a search without these rows (indices shifted).  With fewer than k rows left the tail is -1
 *     / +inf, as for Ng < k;
 *   - a query row holding a NaN or an Inf has a NaN similarity to every gallery row: index -1 and distance +inf in all k slots;
 *   - a finite row whose squares overflow behaves as a zero row -- similarity 0, distance 1 -- as long as its fp32 dot products stay
 *     finite; a dot product that overflows too gives NaN (inf * 0) and that pair is left out.  (torch.topk would rank a NaN first;
 *     sklearn's cosine_distances, which the reference calls, refuses non-finite input.)
 * ------------------------------------------------------------------------------------------------------------- */
int32_t rsp_cosine_topk_splits(int32_t Nq, int32_t Ng, int32_t splits);
size_t rsp_cosine_topk_workspace(int32_t Nq, int32_t Ng, int32_t D, int32_t k, int32_t splits);
int rsp_cosine_topk(const float* q, int32_t ldq, int32_t Nq, const float* g, int32_t ldg, int32_t Ng, int32_t D, int32_t k,
                    int32_t splits, int32_t* idx, float* dist, void* workspace, size_t workspace_bytes, void* stream);
/* counts[i] = number of queries whose label y_q[row] appears among the labels y_g[idx[row][0 .. ks[i])] (retrieval.py:169-
 * 176).  idx: the Nq x k output of rsp_cosine_topk (negative entries never hit); y_q / y_g: int64 device labels; ks_host: HOST
 * array of nks (1..16) values in [1, k], read during the call; counts: nks int32 on the device.  A query whose row held a NaN or an
 * Inf comes out of the search with -1 in every slot, so it is counted for no k (it stays in the denominator Nq the caller divides
 * by); a gallery row holding one is in no list and so hits for nobody. */
int rsp_topk_hits(const int32_t* idx, int32_t Nq, int32_t k, const int64_t* y_q, const int64_t* y_g, int32_t Ng,
                  const int32_t* ks_host, int32_t nks, int32_t* counts, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Weighted kNN classifier (cos_search.hip, knn.hip): the monitor of a pretext run -- the k nearest labelled gallery rows of every query vote for
 * their class with weight exp(s / T); top-1 / top-5 hits of the queries' own labels.  One call, the Nq x Ng matrix never stored.
 * q, g, ldq, ldg, D, splits: as for the search above (D and the pitches even, ld >= D, 8-byte aligned bases).  1 <= k <= 256,
 * 1 <= num_classes <= 1024, T finite and >= 0.01.  y_g: Ng int64 labels; y_q: Nq int64 labels or NULL.
 *   neighbours  the search's rule: s = (q.g) * (1/|q|) * (1/|g|) in fp32 (a zero-norm row: inverse norm 0), s descending, an exact
 *               tie to the lower gallery index, independent of `splits`; a NaN similarity never enters a list.  Ng < k: only Ng
 *               neighbours exist and vote.
 *   idx, dist   [Nq][k], both or neither (may be NULL): as the search writes them (-1 / +inf past Ng); for k <= 64 the search's
 *               output bit for bit.
 *   weights     w_j = expf((s_j - 1) * (1/T)), 1/T formed once on the host as a float: every class of a query is scaled by the
 *               same exp(-1/T), so the ranking is that of exp(s / T) and nothing overflows.
 *   votes       [Nq][num_classes] (may be NULL): votes[i][c] = sum of w_j over the neighbours j of query i with y_g[j] == c, in
 *               fp32 in neighbour-rank order, rank 0 first.  No floating-point atomics: the bits depend on the values only.  A
 *               gallery label outside [0, num_classes) casts no vote.
 *   pred        [Nq]: the class with the largest vote, an exact tie to the lower class index.
 *   rank        [Nq], required if and only if y_q is given: #{c : v[c] > v[t]} + #{c < t : v[c] == v[t]}, t = y_q[i] (the tie rule
 *               of rsp_xent_metrics); num_classes -- a miss -- for a y_q[i] outside [0, num_classes).
 *   hits        [2] (may be NULL; needs y_q): the number of i < valid with rank[i] < 1 and with rank[i] < 5 (also written when
 *               num_classes < 5).  0 <= valid <= Nq cuts the repeated tail of a wrapped last batch.
 *   non-finite  rows: the search's rule (above).  A gallery row holding a NaN or an Inf is nobody's neighbour and casts no vote; the
 *               other rows vote exactly as if the gallery did not hold it.  A query row holding one has no neighbours: idx -1 and
 *               dist +inf in every slot, every vote 0, pred 0 (all classes tie, the lower wins) and rank = y_q[i] (the classes
 *               below the label stand ahead of it in that tie), so hits[0] counts it only if its label is 0 and hits[1] only if its
 *               label is below 5 -- what a constant prediction of class 0 would score.  A finite row whose squares overflow votes
 *               and is voted for as a zero row: similarity 0, weight exp(-1 / T).
 * A bad argument is RSP_EINVAL, a workspace below rsp_knn_classify_workspace RSP_EWORKSPACE, before anything is launched.
 * Kernels only, all on `stream`.
 * ------------------------------------------------------------------------------------------------------------- */
size_t rsp_knn_classify_workspace(int32_t Nq, int32_t Ng, int32_t D, int32_t k, int32_t num_classes, int32_t splits);
int rsp_knn_classify(const float* q, int32_t ldq, int32_t Nq, const int64_t* y_q, const float* g, int32_t ldg, int32_t Ng,
                     const int64_t* y_g, int32_t D, int32_t k, float T, int32_t num_classes, int32_t splits, int32_t valid,
                     int32_t* idx, float* dist, float* votes, int32_t* pred, int32_t* rank, int32_t* hits, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Everything behind the classifier's logits in the fine-tune loop (classify.hip; the reference's finetune.py:101-143), one call:
 * EpochContext.average_logits (:54-61), nn.CrossEntropyLoss forward + gradient (:105, Engine.criterion :187), the tail cut
 * (:112-119), accuracy(output, target, topk=(1, 5)) (:132-139, framework/metrics/classification.py:6-20) and the three
 * AverageMeter.update calls (:135-141, framework/meters/average.py:22-26).
 * logits: rows x classes fp32, row pitch ld >= classes, the n_crop (1..32) crops of a sample adjacent; S = rows / n_crop samples
 * (rows % n_crop != 0: RSP_EINVAL); classes 1..4096; target: S int64 labels; 0 <= valid <= S.
 *   avg_logits [S][classes]  fp32 sum of a sample's crop rows in crop order, divided by n_crop (a copy when n_crop = 1).
 *   loss [1]                 mean over ALL S samples of logsumexp(avg[s]) - avg[s][target[s]] (row max subtracted first).
 *   dlogits [rows][classes]  (softmax(avg[s])[c] - [c == target[s]]) / (S * n_crop) in every crop row of sample s; may be NULL.
 *   acc [2]                  top-1 / top-5 hit rate in percent over the first `valid` samples: fp32(hits) * fp32(100.0 / valid).
 *                            rank(s) = #{c : avg[s][c] > avg[s][t]} + #{c < t : avg[s][c] == avg[s][t]}, t = target[s]; top-1:
 *                            rank 0, top-5: rank < 5 -- an exact tie goes to the lower class index (torch.topk leaves it open).
 *   meters                   device struct, may be NULL: val[i] = v_i, sum[i] += v_i * valid, count[i] += valid for (loss, acc1, acc5).
 * classes < 5: acc[1] and the acc5 meter are left untouched (:137-139).  valid == 0: only avg_logits, loss and dlogits are written
 * (:121-122).  A target outside [0, classes) or a NaN logit makes that sample's loss (and so `loss`) NaN and the sample a miss; the
 * gradient rows of a sample with a bad target are NaN.  Infinite logits follow nn.CrossEntropyLoss and torch.topk: -inf off the
 * target contributes nothing; -inf at the target gives that sample the loss +inf, a finite gradient and the last rank; +inf
 * anywhere in a row (or a row of -inf only) makes the sample's loss and its gradient rows NaN (inf - inf), while its rank is still
 * the count above -- +inf at the target is a hit, +inf elsewhere stands ahead of the target.  (n_crop > 1: the rule applies to the
 * crop mean, which is NaN when the crops hold +inf and -inf.)  No atomics: the same input gives the same bits.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct rsp_cls_meters {   /* order: loss, acc1, acc5 */
  float val[3];
  float sum[3];
  int32_t count[3];
} rsp_cls_meters;
size_t rsp_xent_metrics_workspace(int32_t rows, int32_t n_crop);
int rsp_xent_metrics(const float* logits, int32_t rows, int32_t classes, int32_t ld, int32_t n_crop, const int64_t* target,
                     int32_t valid, float* avg_logits, float* dlogits, float* loss, float* acc, rsp_cls_meters* meters,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The per-step bookkeeping of the pretext loop (pretext_metrics.hip; the reference's pretrain.py:167-195), one call: accuracy(topk=
 * (1, 5)) of both contrast logit matrices, the top-1 of the ranking pair (framework/metrics/classification.py:6-20) and the eight
 * AverageMeter.update calls (framework/meters/average.py:22-26).
 * logits1, logits2: dense [B][K1] fp32 as rsp_logits_fwd writes them (rows start at r * K1 floats: 4-byte alignment is enough);
 * the positive is column 0 (labels_A is all zeros).  lposM, lnegM: B fp32 each.  B >= 1, K1 >= 5.
 *   rank(row) = #{c : v[c] > v[0]}: a column EQUAL to the positive does not count -- an exact tie goes to the lower index, the rule
 *   of rsp_xent_metrics (torch.topk leaves it open) -- and a NaN column never counts.  A NaN positive is a miss.
 *   acc [5]   (acc1_A, acc5_A, acc1_A_n, acc5_A_n, acc1_M) in percent, fp32(hits) * fp32(100.0 / B).  The first four: rank == 0 and
 *             rank < 5 over logits1 / logits2; acc1_M counts rows with lposM >= lnegM (a NaN on either side is a miss).
 *   losses    the [3] (loss, loss_A, loss_M) rsp_loss_fwd_bwd wrote; read only for the meters (may be NULL when meters is).
 *   meters    device struct, may be NULL: val[i] = v_i, sum[i] += v_i * B (fp32), count[i] += B for the eight values in the struct's
 *             order (losses[0], losses[1], acc[0..3], losses[2], acc[4]).
 *   workspace 2 * B int32; after the call it holds the ranks, logits1's rows then logits2's (0x7fffffff for a NaN positive).
 * A bad size, a null pointer or a workspace below rsp_pretext_metrics_workspace(B) is RSP_EINVAL before anything is launched.  Two
 * kernel launches, no memset / memcpy, no atomics: capturable, and the same input gives the same bits.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct rsp_pretext_meters {  /* order: loss, loss_A, acc1_A, acc5_A, acc1_A_n, acc5_A_n, loss_M, acc1_M */
  float val[8];
  float sum[8];
  int32_t count[8];
} rsp_pretext_meters;
size_t rsp_pretext_metrics_workspace(int32_t B);
int rsp_pretext_metrics(const float* logits1, const float* logits2, const float* lposM, const float* lnegM, int32_t B, int32_t K1,
                        const float* losses, float* acc, rsp_pretext_meters* meters, void* workspace, size_t workspace_bytes,
                        void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Similarity maps of the pretext model and their picture panels (cam.hip): MoCoDiffLossTwoFc.cam_visualize
 * (moco/builder_diffspeed_diffloss.py:449-490) and what visualization.py:52-111 draws from its result.
 *
 * cam maps: all four maps from the two NDHWC feature maps, no layout change.
 *   feat_q, feat_k [B][P][C] fp32, row pitch ld_q / ld_k >= C floats (P = T' * H' * W');
 *   k_row [B] int32: the row of feat_k that pairs with sample b (identity: the reference's pairing of the shuffled key batch;
 *     the inverse shuffle: key maps in the caller's order).  A value outside [0, B) makes sample b's four maps NaN;
 *   w_qA, w_kA [dim_A][C], w_qM, w_kM [dim_M][C]: the head weights (fc1[2].weight, fc2[2].weight) of the two encoders;
 *   out [4][B][P], order qA, qM, kA, kM.  With X = mean over P of F and kr = k_row[b]:
 *     out[qA][b][p] = sum_c ((w_kA @ k_X[kr]) @ w_qA)[c] * feat_q[b][p][c]        qM: the same with w_kM, w_qM
 *     out[kA][b][p] = sum_c ((w_qA @ q_X[b]) @ w_kA)[c] * feat_k[kr][p][c]        kM: the same with w_qM, w_kM
 *   Each feature map is read twice (pooled mean; dot products).  fp32 accumulation in a fixed order, no atomics: the same input gives
 *   the same bits.  C + max(dim_A, dim_M) <= 12288 and 2 * C <= 12288 (LDS).  16-byte loads when C, ld_q, ld_k are multiples of 4 and
 *   the pointers 16-byte aligned; any C otherwise.
 * the workspace holds [2][B][C] pooled means + [4][B][C] channel vectors.
 *
 * cam overlay: N picture panels in one launch.  maps [N][T'][H'][W'] fp32; per panel: mean over T', v = (m - min) / (max - min) over
 *   (H', W') (max == min: v = 0), bilinear resize of v to size x size with half-pixel centres (align_corners = False, no
 *   antialiasing), colour r = clamp(1.5 - |4v - 3|), g = clamp(1.5 - |4v - 2|), b = clamp(1.5 - |4v - 1|) clamped to [0, 1],
 *   pixel = round_to_nearest(0.6 * 255 * frame + 0.4 * 255 * colour) clamped to [0, 255].
 *   clip_a, clip_b: (B, 3, T, size, size) fp32 clips in [0, 1] (NOT normalised); frame t of sample n % B is drawn under panel n, from
 *   clip_a for the first N / 2 panels and clip_b for the rest (clip_b NULL: clip_a for all).  H' * W' <= 4096.
 *   out [N][size][size][3] uint8 RGB.
 * ------------------------------------------------------------------------------------------------------------- */
size_t rsp_cam_maps_workspace(int32_t B, int32_t C);
int rsp_cam_maps(const float* feat_q, int32_t ld_q, const float* feat_k, int32_t ld_k, const int32_t* k_row, int32_t B, int32_t P,
                 int32_t C, const float* w_qA, const float* w_qM, const float* w_kA, const float* w_kM, int32_t dim_A, int32_t dim_M,
                 float* out, void* workspace, size_t workspace_bytes, void* stream);
int rsp_cam_overlay(const float* maps, int32_t N, int32_t Tp, int32_t Hp, int32_t Wp, const float* clip_a, const float* clip_b,
                    int32_t B, int32_t T, int32_t t, int32_t size, uint8_t* out, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Step fingerprints (fingerprint.hip; the project's own, no counterpart in the reference): one 32-byte record per tensor of a list
 * of device tensors, from one call.  Additive: the ABI version stays 130.
 *
 * jobs_dev: DEVICE table of n_jobs entries.
 *   ptr      the tensor's first word, 4-byte aligned (16-byte alignment is used when present and changes no result);
 *   words    its length in 32-bit words, 0 <= words < 2^31 (0: an all-zero record);
 *   chunk0   running sum of ceil(words / RSP_FP_CHUNK) over the preceding jobs; total_chunks is the sum over all jobs (<= 2^23);
 *   kind     0: fp32 data; 1: raw words (an int64 tensor passes 2 * numel): only `hash` is formed, the other fields are 0.
 * out_dev: n_jobs records.  With w_i the i-th word as uint32, i from 0, v_i the same word as fp32:
 *   hash       sum_i fmix32((w_i + i * 0x9E3779B1) mod 2^32) mod 2^64, fmix32 = murmur3's 32-bit finaliser (x ^= x >> 16;
 *              x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16).  A bijection per word: a change of any single word
 *              always changes the hash; several simultaneous changes escape with probability about 2^-32 per tensor.  Position
 *              dependent: a swap of two unequal elements is seen.
 *   nonfinite  number of words whose exponent field is all ones; those stay in the hash and are left out of the next three.
 *   sumsq, sum_abs   fp64 sums of v_i^2 (exact squares) and |v_i|;   max_abs   exact fp32 maximum of |v_i| (0 if none).
 * The record is a function of the values only: the same words at another address or alignment, on another stream or in another
 * process give the same 32 bytes, the doubles included (the summation order depends on `words` alone).
 * workspace: rsp_fingerprint_workspace(total_chunks) bytes (32 per chunk), 8-byte aligned; may be NULL when total_chunks is 0.
 * n_jobs == 0 returns 0 without a launch.  A negative count, a null or misaligned pointer or a bad total_chunks is RSP_EINVAL, a
 * workspace below the query RSP_EWORKSPACE, both before anything is launched.  Two kernel launches, no memset / memcpy, no
 * atomics: capturable.  The table itself is not checked (it is on the device): a chunk it does not describe contributes zeros.
 * ------------------------------------------------------------------------------------------------------------- */
#define RSP_FP_CHUNK 8192 /* 32-bit words per partial */
typedef struct rsp_fingerprint_job {
  const void* ptr;
  int64_t words;
  int64_t chunk0;
  int32_t kind;
  int32_t reserved;
} rsp_fingerprint_job; /* 32 bytes */
typedef struct rsp_fingerprint_rec {
  uint64_t hash;
  double sumsq;
  double sum_abs;
  float max_abs;
  uint32_t nonfinite;
} rsp_fingerprint_rec; /* 32 bytes */
size_t rsp_fingerprint_workspace(int64_t total_chunks);
int rsp_fingerprint(const rsp_fingerprint_job* jobs_dev, int32_t n_jobs, int64_t total_chunks, rsp_fingerprint_rec* out_dev,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Label-free representation statistics (repr_stats.hip; the project's own, no counterpart in the reference): whether N embedding
 * rows spread over the sphere or collapse, from ONE call -- the pair sums behind uniformity (Wang & Isola) and the mean pairwise cosine,
 * the Gram matrix behind the effective rank (RankMe) and the per-dimension spread.  The N x N matrix is never stored.  Additive: the
 * ABI version stays 130.
 * x: N x D fp32 row-major with row pitch ld; D and ld even, ld >= D, the base 8-byte aligned; 1 <= N <= 262144, 2 <= D <= 4096.
 * c = 2 t of the uniformity's exp(-t |xi - xj|^2) = exp(c (s - 1)): finite, in (0, 64].  gram [D][D] and colsum [D] (fp64): both or
 * both NULL.  sums, gram, colsum and the workspace (rsp_repr_stats_workspace bytes) are 8-byte aligned.
 *   validity    ss_i = the fp32 sum of squares of row i (each lane of a wave: its float2 columns 2 l, 2 l + 128, ... by fmaf, x then y;
 *               then the wave's xor butterfly -- the search's inverse-norm kernel).  Row i is valid iff ss_i is finite and > 0: a zero
 *               row and a row holding a NaN or an Inf are invalid.  An invalid row takes part in nothing and is counted in rows_bad;
 *               its elements are selected away when staged, never multiplied by zero.  M = rows_valid.
 *   similarity  s_ij = (x_i . x_j) * inv_i * inv_j in fp32, inv_i = 1 / sqrtf(ss_i): the search's expression.
 *   pair sums   over valid i < j, each pair exactly once: pair_exp = sum expf(c * (s - 1)) (the argument is <= about 0: nothing
 *               overflows), pair_cos = sum s, pair_cos2 = sum s * s.  Each thread adds its 32 elements of a 64 x 128 tile in fp32 in a
 *               fixed order; everything above that -- a thread's tiles, the workgroup, the partials in the workspace, the final
 *               reduce -- is added in fp64 in a fixed order: the same input and the same N give the same bits.
 *   gram        gram[a][b] = sum over valid i of xh_ia * xh_ib, colsum[a] = sum over valid i of xh_ia, xh = x * inv formed in fp32 when
 *               staged.  Products and the accumulation inside a split of the row axis run on the fp32 MFMA (colsum: fp32 adds in row
 *               order); the split count is chosen from N and D; the splits are added in fp64 in split order.  Every element of gram
 *               is written, both triangles; a 64 x 128 tile wholly below the diagonal is the mirror image of the computed elements
 *               above it, so gram is symmetric to the bit.
 * A bad argument is RSP_EINVAL, a workspace below the query RSP_EWORKSPACE, both before anything is launched.  Kernels only, all on
 * `stream`: no memset, no memcpy, no atomics; capturable after a first eager call.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct rsp_repr_sums {      /* device struct, 40 bytes */
  double pair_exp, pair_cos, pair_cos2;   /* sums over valid pairs i < j of exp(c*(s-1)), s, s*s */
  int64_t rows_valid, rows_bad;
} rsp_repr_sums;
size_t rsp_repr_stats_workspace(int32_t N, int32_t D);
int rsp_repr_stats(const float* x, int32_t ld, int32_t N, int32_t D, float c, rsp_repr_sums* sums, double* gram, double* colsum,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Linear probe on frozen features (linear_probe.hip; the reference configures it as finetune's `linear` overlay, only_train_fc, and
 * runs the frozen backbone again every epoch): a softmax classifier fitted by SGD with momentum on N stored feature rows, all
 * `steps` steps issued from ONE call, nothing read back.  Additive: the ABI version stays 130.
 * x: N x D fp32 row-major with row pitch ld; D and ld even, ld >= D, the base 8-byte aligned (the rule of the cosine search);
 * y [N] int64, 8-byte aligned.  1 <= C <= 1024, 1 <= N, 2 <= D <= 4096, 1 <= batch <= N, 1 <= steps, 0 <= first_step.
 * w [C][D] (nn.Linear.weight's layout, 8-byte aligned), b [C], mom [C*D + C] (w's buffer, then b's), lr_dev [>= first_step + steps]
 * on the device, loss_trace [steps], counts [2]: 4-byte aligned.  workspace: rsp_linear_probe_workspace bytes, 8-byte aligned.
 *   row factor  f_i = scale / sqrtf(ss_i), ss_i = the fp32 sum of squares of row i (each lane of a wave: its float2 columns 2 l,
 *               2 l + 128, ... by fmaf, x then y; then the wave's xor butterfly -- the search's inverse-norm kernel); f_i = scale with
 *               normalize = 0.
 *   valid rows  row i is valid iff ss_i is finite and > 0 (normalize = 0: finite) and 0 <= y_i < C.  An invalid row takes part in
 *               nothing: the valid rows of every chunk are listed once (in ascending order) and the steps walk that list, so its
 *               elements are selected away, never multiplied by zero, and with batch = N the fit equals, to the bit, the fit on x
 *               without those rows.  counts[0] = valid rows of x, counts[1] = invalid ones (integers, from a kernel).
 *   model       xh_i = x_i * f_i (fp32, when staged); z = xh W^T + b on the fp32 MFMA (a k-ordered fmaf chain), bias added last.
 *   step t      (t = 0 .. steps - 1) rows [r0, r0 + n), r0 = (t mod ceil(N / batch)) * batch, n = min(batch, N - r0); m = the valid
 *               rows among them.  loss_trace[t] = (sum over those rows of max_i + logf(sum_c expf(z_ic - max_i)) - z_i[y_i]) / m,
 *               0 with m = 0.  G_i = (expf(z_i - max_i) / sum_i - onehot(y_i)) / m for a valid row, zeros otherwise.
 *               dW = G^T xh + wd W, db = sum_i G_i + wd b; buf = (first_step + t == 0) ? d : mu * buf + d; p -= lr[first_step + t] *
 *               buf -- the rsp_sgd_step rule, weight decay on W and b alike (torch.optim.SGD over fc.parameters()).
 *   order       a row's max / sum: lane l of a wave takes classes l, l + 64, ... in ascending order, then the xor butterfly; a
 *               64-row tile's losses in row order, the tiles' partials lane l: l, l + 64, ... then the butterfly.  dW / db: the rows
 *               of a step are cut into `splits` ranges of 32-row chunks (splits from C, D and the step's m alone), a range runs on the MFMA
 *               in row order (db: fp32 adds in row order), the ranges are added in fp32 in range order.  No atomics: the same input
 *               gives the same bits, eagerly or replayed.
 *   non-finite  a NaN or Inf in w, b, lr or mom propagates as the arithmetic says; one in x, or a label outside [0, C), invalidates
 *               that row only.
 * C <= 256: three launches per step (logits, softmax, loss and G in one kernel -- the logits are never stored); four otherwise
 * (the environment variable RSP_PROBE_GENERAL=1 selects that path at any C: an A/B switch).  The two paths are each held to the rule
 * and need not agree to the bit.
 * rsp_linear_probe_logits: logits[i][c] = z_ic of the rule (row pitch ld_out >= C), NaN in every class of an invalid row (validity
 * without the label condition) -- rsp_xent_metrics then counts the row as a miss.  It needs the first 2 * align256(4 N) bytes of the
 * workspace: rsp_linear_probe_workspace(N, D, C, b) for any b is enough.
 * A bad argument is RSP_EINVAL, a workspace below the need RSP_EWORKSPACE, both before anything is launched.  Kernels only, all on
 * `stream`: no memset, no memcpy, no atomics; capturable after a first eager call.
 * workspace of fit: f, the flags and the row lists (3 x 4 N), the m of every chunk, G (batch x C), the loss partials (ceil(batch / 64)), the split
 * partials of dW and db (splits x (C D + C)), each rounded up to 256 bytes.
 * ------------------------------------------------------------------------------------------------------------- */
size_t rsp_linear_probe_workspace(int32_t N, int32_t D, int32_t C, int32_t batch);
int rsp_linear_probe_fit(const float* x, int32_t ld, int32_t N, int32_t D, const int64_t* y, int32_t C, int32_t batch,
                         int32_t first_step, int32_t steps, const float* lr_dev, float mu, float wd, int32_t normalize, float scale,
                         float* w, float* b, float* mom /* [C*D + C] */, float* loss_trace /* [steps] */, int32_t* counts /* [2] */,
                         void* workspace, size_t workspace_bytes, void* stream);
int rsp_linear_probe_logits(const float* x, int32_t ld, int32_t N, int32_t D, const float* w, const float* b, int32_t C,
                            int32_t normalize, float scale, float* logits, int32_t ld_out, void* workspace, size_t workspace_bytes,
                            void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Clustering evaluation (cluster.hip; the project's own, no counterpart in the reference): spherical k-means on N stored feature
 * rows, all max_iters iterations issued from ONE call, stopped on the device, nothing read back; and the cluster x label table behind
 * NMI, ARI and purity.  Additive: the ABI version stays 130.
 * x: N x D fp32 row-major with row pitch ld; D and ld even, ld >= D, the base 8-byte aligned (the rule of the cosine search).
 * cent [C][D] (pitch D, 8-byte aligned): in = the initial centroids, out = the final ones.  1 <= N <= 262144, 2 <= D <= 4096,
 * 1 <= C <= 1024, 1 <= L <= 1024, 1 <= max_iters <= 1000.  assign [N], counts [C], changed_trace [max_iters]: int32, 4-byte aligned;
 * objective_trace [max_iters] (fp64), info and the workspace (rsp_kmeans_workspace bytes): 8-byte aligned.
 *   validity    ss_i = the fp32 sum of squares of row i as the search forms it (rsp_row_sumsq: each lane of a wave its float2 columns
 *               2 l, 2 l + 128, ... by fmaf, x then y; then the wave's xor butterfly).  Row i is valid iff ss_i is finite and > 0.  An
 *               invalid row gets assign = -1, is counted in rows_bad and takes part in nothing: the valid rows are listed once, in
 *               ascending order, and every kernel walks that list by rank, so its elements are selected away, never multiplied by
 *               zero, and the fit equals, to the bit, the fit on x without those rows.
 *   assignment  assign[i] = the single neighbour rsp_cosine_topk(q = x, g = cent, k = 1) returns for row i, sim[i] its similarity
 *               s = (x_i . m_c) * inv_i * inv_c in fp32 -- the search itself runs, there is no second expression.  A zero centroid
 *               has inverse norm 0 (s = 0); a centroid holding a NaN or an Inf is never returned; an exact tie goes to the LOWER
 *               cluster index.  A valid row for which no centroid is returnable gets -1 (sim NaN) and is counted in `unassigned`.
 *   iteration   t = 0 .. max_iters - 1: assign from the current cent.  changed_trace[t] = the rows whose assignment differs from
 *               iteration t - 1 (t = 0: rows_valid).  objective_trace[t] = the sum of sim over the assigned rows / their number, 0
 *               with none: the fp32 values added in fp64 -- a block of 256 list ranks by the wave's xor butterfly and then its four
 *               waves in order, the blocks lane l: l, l + 64, ... in order and then the butterfly.  If t > 0 and changed_trace[t] ==
 *               0: converged = 1, iters_run = t + 1 and nothing is updated further.  Otherwise the update: for a cluster with
 *               counts[c] > 0, cent[c][a] = the sum over the rows with assign == c of xh_ia, xh = x * inv_i formed in fp32 when
 *               staged, left unnormalised (the search normalises); a cluster with counts[c] == 0 keeps its centroid.  The update
 *               also follows the last iteration of a fit that has not converged: the returned cent is always the sum over the
 *               returned assign, and counts its bincount.
 *   order       the update is onehot(assign)^T xh on the fp32 MFMA: the listed rows are cut into `splits` ranges of 32-row chunks
 *               (splits from C, D and rows_valid alone); inside a range an element of cent is the fp32 sum of its rows' xh in
 *               ascending row order (1 * v and 0 * v are exact, a k-ordered fmaf chain); the ranges are added in fp32 in range
 *               order.  No float atomics: the same input gives the same bits, eagerly or replayed.
 *   traces      entries t >= iters_run: changed_trace = -1, objective_trace = NaN.  Every element of cent (of a non-empty cluster),
 *               assign, counts, both traces and info is written on every call.
 *   info        rows_valid, rows_bad; iters_run (max_iters when not converged), converged; empty = the clusters with count 0 and
 *               unassigned = the valid rows with assign -1, both in the returned assignment.
 *   stop        the call issues the launches of all max_iters iterations (six each after the first); behind the stop they read a device
 *               flag and return at once.  No read-back, no synchronisation inside the call.
 * rsp_kmeans_assign: assign / sim (sim may be NULL) of the rule for the rows of x against given centroids, no update.  workspace:
 * rsp_cosine_topk_workspace(N, C, D, 1, 0) bytes (rsp_kmeans_workspace(N, D, C) is enough).
 * rsp_contingency: table[c][l] = the number of i with assign[i] == c and y[i] == l (y int64, 8-byte aligned, as table and dropped);
 * rows with assign outside [0, C) -- the -1 rows -- or y outside [0, L) are counted in dropped[0].  Exact integers (the table is
 * zeroed by a kernel, then integer atomic adds); every element of the table is written.
 * A bad argument is RSP_EINVAL with the entry point's name in rsp_last_error(), a workspace below the query RSP_EWORKSPACE, both
 * before anything is launched.  Kernels only, all on `stream`: no memset, no memcpy, no float atomics; capturable after a first eager call.
 * workspace of fit: the search's (inverse norms and k = 1 lists), the state, the row list (4 N), the block partials (16 per 256 rows),
 * the split partials of cent and counts (splits x (C D + C)), each rounded up to 256 bytes.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct rsp_kmeans_info {      /* device struct, 32 bytes */
  int64_t rows_valid, rows_bad;
  int32_t iters_run, converged, empty, unassigned;
} rsp_kmeans_info;
size_t rsp_kmeans_workspace(int32_t N, int32_t D, int32_t C);
int rsp_kmeans_fit(const float* x, int32_t ld, int32_t N, int32_t D, float* cent /* [C][D]: in = initial, out = final */, int32_t C,
                   int32_t max_iters, int32_t* assign /* [N] */, int32_t* counts /* [C] */, int32_t* changed_trace /* [max_iters] */,
                   double* objective_trace /* [max_iters] */, rsp_kmeans_info* info, void* workspace, size_t workspace_bytes,
                   void* stream);
int rsp_kmeans_assign(const float* x, int32_t ld, int32_t N, int32_t D, const float* cent, int32_t C, int32_t* assign /* [N] */,
                      float* sim /* [N], nullable */, void* workspace, size_t workspace_bytes, void* stream);
int rsp_contingency(const int32_t* assign, const int64_t* y, int32_t N, int32_t C, int32_t L, int64_t* table /* [C][L] */,
                    int64_t* dropped /* [1] */, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Embedding maps (tsne.hip; the project's own, no counterpart in the reference): exact t-SNE of N stored feature rows.  The
 * affinities are ONE call; all `iters` iterations of the descent are issued from ONE call, three launches each, nothing read back.
 * Additive: the ABI version stays 130.
 * x: N x D fp32 row-major with row pitch ld; D and ld even, ld >= D, the base 8-byte aligned (the rule of the cosine search).
 * 2 <= N <= 16384, 2 <= D <= 4096, perplexity finite and in [1, 1024], 1 <= iters <= 10000, 0 <= first_iter.
 * pmat [N][ldp], ldp >= N (its top-left M x M holds p over the listed rows, the rest of the N x N is written as 0), dmat (optional,
 * pmat's shape and pitch; without it the distances live in the workspace), rows [N] int32, beta [N]: 4-byte aligned.  y, inc, gains
 * [N][2] fp32 indexed by the ORIGINAL row, kl_trace [iters] fp64, sched [first_iter + iters][4] fp32, info and both workspaces:
 * 8-byte aligned.
 *   valid rows   row i is valid iff its fp32 sum of squares ss_i, formed by rsp_row_sumsq -- the search's routine: each lane of a wave
 *                its float2 columns 2 l, 2 l + 128, ... by fmaf, x then y; then the wave's xor butterfly --, is finite and > 0.  The
 *                valid rows are listed once, in ascending order: rows[r] for rank r < M, -1 behind; M = info.rows_valid.  Every later
 *                kernel walks that list, so an invalid row takes part in nothing, its y, inc and gains are never read or written, and
 *                the result equals, to the bit, the result on x without that row.
 *   distance     s_ij = (x_i . x_j) * inv_i * inv_j in fp32 on the fp32 MFMA (a k-ordered chain; inv = 1 / sqrtf(ss)), the inverse
 *                norm of the lower rank applied first: the search's expression above the diagonal, its mirror image below.
 *                d_ij = fmaxf(2 - 2 s_ij, 0); d_ii is not used (stored as 0); d is symmetric to the bit.
 *   calibration  per rank i over j != i: m_i = min_j d_ij; e_j(b) = expf(-b (d_ij - m_i)), S = sum e_j, A = sum e_j (d_ij - m_i) (fmaf),
 *                H = logf(S) + b A / S.  b = 1, lo = 0, hi = +inf, then exactly 64 steps: H > logf(perplexity): lo = b, b = isinf(hi) ?
 *                2 b : (lo + hi) / 2; otherwise hi = b, b = (lo + hi) / 2.  No early exit.  beta[r] = the final b, NaN for r >= M;
 *                c_ij = e_j(beta_i) / S_i with S_i formed at the final b.  Every row sum: lane l of one wave adds columns l, l + 64, ...
 *                in ascending order in fp32, then the xor butterfly.  No atomics.
 *   joint        p_ij = (c_ij + c_ji) * (1 / (2 M)) in fp32, the lower rank's term first; p_ii = 0; symmetric to the bit.  c_ji is
 *                recomputed from d_ij (= d_ji) and rank j's (beta, m, S), so it is the same float the calibration of j defines.
 *                info.psum = sum p, info.plogp = sum over p > 0 of p logf(p) (the fp32 product), added in fp64: thread t of rank i's
 *                block adds columns t, t + 256, ...; the wave butterfly, the four waves in order; then the ranks t, t + 1024, ... of
 *                one block, the butterfly, the sixteen waves in order.
 *   iteration t  over listed i != j: r2 = dx dx + dy dy with (dx, dy) = y_i - y_j, w = 1 / (1 + r2); attr_i = sum p_ij w (dx, dy),
 *                rep_i = sum w w (dx, dy), z_i = sum w, e_i = sum p_ij log1pf(r2); Z = sum z_i, E = sum e_i;
 *                g_i = 4 (exag_t attr_i - rep_i / (float)Z); kl_trace[t] = plogp + E + log(Z): the KL of the map BEFORE the update,
 *                with the un-exaggerated p.  Per coordinate: gains = ((g > 0) != (inc > 0)) ? gains + 0.2 : gains * 0.8, floored at
 *                0.01; inc = mom_t inc - lr_t gains g; y += inc.  No re-centring.  (lr_t, mom_t, exag_t, pad) = sched[first_iter + t].
 *   order        the ranks j are cut into 64-column chunks and the chunks into `splits` ranges (splits from M alone).  Thread (wave
 *                w, lane r) of a block takes rank i0 + r and columns 16 w .. 16 w + 15 of every chunk of the range in ascending order
 *                in fp32; the four waves are added in wave order, the ranges in range order (fp32).  Z and E: the z_i, e_i of 256
 *                ranks in fp64 by the butterfly and the four waves in order; those blocks lane l: l, l + 64, ..., then the butterfly.
 *                No atomics, no memset, no memcpy: the same input gives the same bits, eagerly or replayed.
 *   non-finite   a NaN or Inf in x invalidates that row only; one in y, inc, gains or sched propagates as the arithmetic says (Z goes
 *                NaN, then the whole map and kl_trace from that iteration on).
 * rsp_tsne_fit takes pmat, rows and info as rsp_tsne_affinities left them (N: the same N); it is resumable: a second call with
 * first_iter advanced continues the same trajectory.
 * A bad argument is RSP_EINVAL with the entry point's name in rsp_last_error(), a workspace below the query RSP_EWORKSPACE, both
 * before anything is launched.  Kernels only, all on `stream`; capturable after a first eager call.
 * workspaces: affinities -- the state, four vectors of N floats, 2 N doubles and the N x N distances; fit -- the split partials
 * (splits x N x 8 floats), 4 N floats and the block partials, each rounded up to 256 bytes.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct rsp_tsne_info {      /* device struct, 32 bytes */
  double plogp, psum;
  int64_t rows_valid, rows_bad;
} rsp_tsne_info;
size_t rsp_tsne_affinities_workspace(int32_t N, int32_t D);
int rsp_tsne_affinities(const float* x, int32_t ld, int32_t N, int32_t D, float perplexity, float* pmat, int32_t ldp,
                        int32_t* rows /* [N] */, float* beta /* [N] */, float* dmat /* nullable */, rsp_tsne_info* info,
                        void* workspace, size_t workspace_bytes, void* stream);
size_t rsp_tsne_fit_workspace(int32_t N);
int rsp_tsne_fit(const float* pmat, int32_t ldp, const int32_t* rows, const rsp_tsne_info* info, int32_t N, const float* sched_dev,
                 int32_t first_iter, int32_t iters, float* y, float* inc, float* gains, double* kl_trace /* [iters] */,
                 void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RSPNET_HIP_H */
