/*
 * ymi.h - C ABI of libyolo_mi355.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * YOLOv8-CBAM-Swin forward/backward hot path.
 *
 * The reference (mazouziwissem/improving_yolov8_CBAM_SwinBlock, a fork of Ultralytics 8.3.108) has no
 * native kernels: its operator modules call torch.nn.functional, i.e. ATen.  Each entry point below
 * therefore cites the reference *call site* whose ATen work it replaces (paths relative to the
 * reference's ultralytics/ directory).  The Python-side binding is
 * improving_yolov8_cbam_swinblock_amd/_lib.py (ctypes); INTEGRATION.md shows the stub a maintainer
 * of the reference would add.
 *
 * Conventions
 *  - plain pointers and sizes only; all pointers are DEVICE pointers unless named host_*;
 *  - activations are NHWC ("channels last"): element (n,h,w,c) of a ymi_tensor lives at
 *    data[((n*h_dim + h)*w_dim + w)*ld + c]; ld >= c lets a tensor be a channel slice of a wider
 *    buffer (this is how chunk/concat cost nothing);
 *  - dtype of activations: YMI_F32 (parity mode, exact-f32 MFMA) or YMI_BF16 (fast mode, bf16 MFMA
 *    with f32 accumulation); per-channel vectors (bias, BN affine, statistics) are always f32;
 *  - trainable weights cross the ABI in the reference's own layouts (conv OIHW f32, linear [out,in]
 *    f32); ymi_pack_* turn them into the kernels' K-contiguous operand layouts;
 *  - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*); nothing allocates,
 *    frees or synchronises, so calls are graph-capturable; workspaces are caller-provided;
 *  - return 0 on success, a negative YMI_E* otherwise; ymi_last_error() gives thread-local text.
 */
#ifndef YMI_H
#define YMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YMI_VERSION 1

enum { YMI_F32 = 0, YMI_BF16 = 1 };
enum { YMI_ACT_NONE = 0, YMI_ACT_SILU = 1, YMI_ACT_GELU = 2 };
enum { YMI_OK = 0, YMI_EINVAL = -1, YMI_EALIGN = -2, YMI_ELAUNCH = -3, YMI_EWORKSPACE = -4 };

typedef struct ymi_tensor {
    void* data;
    int64_t n, h, w, c;
    int64_t ld;    /* elements between consecutive pixels, >= c */
    int32_t dtype; /* YMI_F32 | YMI_BF16 */
    int32_t _pad;
} ymi_tensor;

int ymi_version(void);
const char* ymi_last_error(void);
/* Development options: named integers that select the "before" arm of a measured change, a grid size for an in-step sweep or a
 * forced code path for a test (csrc/common.h: YmiOpt lists them with their defaults; an environment variable YMI_<NAME> present at
 * process start sets the initial value).  The reference has no counterpart (its knobs are cfg/default.yaml keys); production code sets
 * none.  set: YMI_EINVAL for an unknown name; get: -1 for an unknown name. */
int ymi_set_option(const char* name, int64_t value);
int64_t ymi_get_option(const char* name);

/* Optional live timing of the MFMA GEMM kernels (HIP events on the launch stream) for bench.py's roofline
 * line.  begin(): pre-create events for `capacity` launches and start recording; end(): synchronise the
 * device and return per-family totals (family 0: implicit-GEMM conv forward / data-gradient / token GEMMs,
 * family 1: weight-gradient GEMM): elapsed ms, algorithmic FLOP (2*M*N*K of the launch), launch count. */
int ymi_profile_begin(int64_t capacity);
int ymi_profile_end(double* ms_by_family, double* flop_by_family, int64_t* launches_by_family);
/* as ymi_profile_end, plus per family: the algorithmic HBM bytes (operands read once, result written once) and the sum
 * over launches of each launch's own roofline time max(flop / MFMA peak of its dtype, bytes / 8 TB/s), in ms. */
int ymi_profile_end_ex(double* ms_by_family, double* flop_by_family, int64_t* launches_by_family, double* bytes_by_family,
                       double* bound_ms_by_family);

/* ---------------------------------------------------------------- layout / data movement ---- */

/* NCHW f32 image -> NHWC (dst.dtype), channels c..dst.c-1 zero-filled.  Replaces the implicit
 * layout of the first conv's input: nn/tasks.py:171 feeding nn/modules/conv.py:79. */
int ymi_nchw_to_nhwc(const float* src, int64_t n, int64_t c, int64_t h, int64_t w, const ymi_tensor* dst, void* stream);
/* NHWC (any dtype) -> NCHW f32.  API edge for callers that want the reference's memory format. */
int ymi_nhwc_to_nchw(const ymi_tensor* src, float* dst, void* stream);
/* dst[n,h,w,0:c] = src (dtype may differ: cast).  torch.cat of nn/modules/conv.py:683 and
 * nn/modules/block.py:226,304 when the producer could not write into the slice itself. */
int ymi_copy(const ymi_tensor* src, const ymi_tensor* dst, void* stream);
/* dst[n,2h+i,2w+j,:] = src[n,h,w,:] : nn.Upsample(None, 2, "nearest"), cfg yolov8.yaml:759,764. */
int ymi_upsample2x(const ymi_tensor* src, const ymi_tensor* dst, void* stream);
/* adjoint: dst[n,h,w,:] = sum of the 2x2 block of src. */
int ymi_upsample2x_bwd(const ymi_tensor* src, const ymi_tensor* dst, void* stream);
/* adjoint accumulated onto dst: dst[n,h,w,:] += sum of the 2x2 block of src (dst already holds the other consumers' gradient). */
int ymi_upsample2x_bwd_acc(const ymi_tensor* src, const ymi_tensor* dst, void* stream);
/* dst += src (f32 accumulate, elementwise over NHWC tensors of equal shape). */
int ymi_add_inplace(const ymi_tensor* src, const ymi_tensor* dst, void* stream);

/* ------------------------------------------------------------------------- weight packing ---- */

/* OIHW f32 -> [O][kh][kw][Ipad] in `dtype` (K contiguous): operand of ymi_conv2d_fwd.
 * Ipad >= I, a multiple of 8 (bf16) / 4 (f32); padded channels are zero. */
int ymi_pack_conv_weight_fwd(const float* w_oihw, int64_t o, int64_t i, int64_t kh, int64_t kw, int64_t ipad, int32_t dtype, void* dst, void* stream);
/* OIHW f32 -> operand of ymi_conv2d_bwd_data: for stride 1 one block [I][kh][kw][O] with taps
 * flipped; for stride 2 the four output-parity classes back to back (sizes from
 * ymi_conv_dgrad_pack_elems). */
int ymi_pack_conv_weight_dgrad(const float* w_oihw, int64_t o, int64_t i, int64_t kh, int64_t kw, int64_t stride, int32_t dtype, void* dst, void* stream);
/* same, with the K axis (dy channels) zero-padded from o_real to o_pad rows. */
int ymi_pack_conv_weight_dgrad_ex(const float* w_oihw, int64_t o_real, int64_t o_pad, int64_t i, int64_t kh, int64_t kw, int64_t stride, int32_t dtype, void* dst, void* stream);
int64_t ymi_conv_dgrad_pack_elems(int64_t o, int64_t i, int64_t kh, int64_t kw, int64_t stride);
/* All weights of a model in ONE launch.  descs_device: array of ymi_pack_desc in device memory; block_start_device:
 * int32[count+1] prefix sums of the workgroups per tensor = ceil(max(o, opad if dst_dgrad) / 32) * ceil(max(i, ipad if dst_fwd) / 32)
 * (a workgroup reads a 32 x 32 channel tile of the source once and writes both operands from LDS); either destination may be
 * NULL; kh * kw <= 9.
 * Same layouts as ymi_pack_conv_weight_fwd / _dgrad_ex (nn.Linear weights: kh = kw = 1). */
typedef struct ymi_pack_desc {
    const float* src;
    void* dst_fwd;
    void* dst_dgrad;
    int32_t o, i, kh, kw, ipad, opad, stride;
    int32_t ostride; /* row length of the data-gradient operand; 0 = opad.  With ostride > opad several weights fill one operand side by side: */
    int32_t o_off;   /* ... this weight's first column (the merged operand of Detect's sibling convolutions cv2[i][0] / cv3[i][0], head.py:71-72) */
    int32_t _pad;
} ymi_pack_desc;
int ymi_pack_conv_weights_batch(const void* descs_device, const int32_t* block_start_device, int32_t count, int32_t total_blocks,
                                int32_t dtype, void* stream);
/* [rows][cols] f32 -> `dtype`, optionally transposed ([cols][rows]): nn.Linear / in_proj weights. */
int ymi_pack_matrix(const float* src, int64_t rows, int64_t cols, int32_t transpose, int32_t dtype, void* dst, void* stream);

/* ------------------------------------------------------------ convolution (implicit GEMM) ---- */

/* y = act(scale[c] * conv(x, w) + bias[c]) + residual        (MFMA implicit GEMM, NHWC)
 *   w: packed by ymi_pack_conv_weight_fwd with ipad == x->c;  pad = k/2 ("autopad", conv.py:28-34).
 *   scale, bias, residual may be NULL.  If stat_partials != NULL the kernel also writes per-M-block
 *   partial sums [blocks][2][cout] (sum, sum of squares of the ROUNDED outputs) for train-mode BN;
 *   *host_stat_blocks receives `blocks`.  ymi_conv2d_stat_blocks() gives an upper bound for sizing.
 * Replaces F.conv2d at nn/modules/conv.py:79,91 (Conv), nn/modules/head.py:45-59 (Detect stacks),
 * nn/modules/cbam.py:24-26 is NOT routed here (tiny, fused in ymi_cbam_*).
 * With kh=kw=1 and n*h*w = rows it is the token GEMM of nn/modules/swin_block.py:31-35,51,53. */
int ymi_conv2d_fwd(const ymi_tensor* x, const void* w_packed, int64_t cout, int64_t kh, int64_t kw, int64_t stride,
                   const float* scale, const float* bias, int32_t act, const ymi_tensor* residual, const ymi_tensor* y,
                   float* stat_partials, int64_t* host_stat_blocks, void* stream);
int64_t ymi_conv2d_stat_blocks(int64_t m_rows, int64_t cout);
/* Several independent convolutions (any shapes; same dtype; statistics mode for all or none; input channels in whole K steps of the same
 * width class; with statistics: the same output-pixel count per BatchNorm group) in ONE launch, at most 8: the same stage of Detect's three levels (nn/modules/head.py:66-74 loops over them), whose small
 * levels cannot fill the chip alone.  Arguments per problem as ymi_conv2d_fwd; stat_blocks is written by the call. */
typedef struct ymi_conv_problem {
    const ymi_tensor* x;
    const void* w_packed;
    int64_t cout, kh, kw, stride;
    const float* scale;
    const float* bias;
    int32_t act, _pad;
    const ymi_tensor* residual;
    const ymi_tensor* y;
    float* stat_partials;
    int64_t stat_blocks;
    int64_t stat_stride, stat_offset; /* statistics rows [block][2][stat_stride] with this problem's channels at column stat_offset: the problems of
                                       * one BatchNorm group share a row array (all problems of a launch use the same row tile); 0: [2][cout] */
} ymi_conv_problem;
int ymi_conv2d_fwd_multi(const ymi_conv_problem* problems, int32_t n, void* stream);

/* Train-mode BatchNorm2d statistics from the partials above (nn/modules/conv.py:66,79 with
 * eps/momentum of utils/torch_utils.py:468-470): writes scale = gamma*invstd, shift = beta - mean*scale,
 * save_mean, save_invstd, and updates running_mean / running_var (unbiased) in place. */
int ymi_bn_finalize(const float* stat_partials, int64_t blocks, int64_t count, int64_t c, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, float momentum, float eps, float* scale, float* shift,
                    float* save_mean, float* save_invstd, void* stream);
/* the same for two BatchNorms whose channels lie side by side (channels >= split read gamma2 / beta2 and update running_*2): the
 * BatchNorms of two convolutions that ran as one, or side by side into one buffer (Detect's branches, head.py:44-59). */
int ymi_bn_finalize_pair(const float* stat_partials, int64_t blocks, int64_t count, int64_t c, int64_t split, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, const float* gamma2, const float* beta2, float* running_mean2, float* running_var2,
                         float momentum, float eps, float* scale, float* shift, float* save_mean, float* save_invstd, void* stream);
/* out = act(raw*scale[c] + shift[c]) + residual : BN-affine + SiLU (+ Bottleneck add, block.py:488). */
int ymi_scale_shift_act(const ymi_tensor* raw, const float* scale, const float* shift, int32_t act, const ymi_tensor* residual,
                        const ymi_tensor* out, void* stream);

/* Conv + train-mode BN + SiLU in one call: conv (raw, statistics) -> finalize -> affine+SiLU.
 * `raw` (saved for backward) and `out` have y's shape; workspace >= ymi_conv2d_stat_blocks*2*cout*4 B
 * + 2*cout*4 B.  Replaces Conv.forward, nn/modules/conv.py:69-79. */
int ymi_conv2d_bn_silu_fwd(const ymi_tensor* x, const void* w_packed, int64_t cout, int64_t kh, int64_t kw, int64_t stride,
                           const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum,
                           float eps, int32_t act, const ymi_tensor* residual, const ymi_tensor* raw, const ymi_tensor* out,
                           float* save_mean, float* save_invstd, void* workspace, size_t workspace_bytes, void* stream);

/* The same Conv block in TWO launches: the GEMM's statistics epilogue adds its per-block sums as 64-bit fixed-point atomics (exact, order-free:
 * the statistics stay bit-reproducible) into stat_acc = [4][2][cout] int64, ZERO on entry, and the affine + activation pass finalizes them in its
 * prologue (scale / shift per thread; saved mean / inverse deviation and the running statistics by its first workgroup) - no finalize launch.
 * `_acc_ok`: whether the affine pass takes these tensors in that form (cout a multiple of 4 up to 1024, 4-element-aligned rows); the per-channel
 * vectors must be 16-byte aligned.  Replaces Conv.forward, nn/modules/conv.py:69-79, as ymi_conv2d_bn_silu_fwd does. */
int ymi_conv2d_bn_silu_fwd_acc_ok(const ymi_tensor* raw, const ymi_tensor* out, const ymi_tensor* residual);
int ymi_conv2d_bn_silu_fwd_acc(const ymi_tensor* x, const void* w_packed, int64_t cout, int64_t kh, int64_t kw, int64_t stride,
                               const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum,
                               float eps, int32_t act, const ymi_tensor* residual, const ymi_tensor* raw, const ymi_tensor* out,
                               float* save_mean, float* save_invstd, void* stat_acc, void* stream);

/* Backward of act(BN_train(raw)) w.r.t. raw, two passes:
 *  reduce: partial sums of dz and dz*xhat per channel, dz = dout * act'(raw*scale+shift)
 *  apply : draw = gamma*invstd*(dz - mean(dz) - xhat*mean(dz*xhat)); also dgamma, dbeta. */
int ymi_bn_act_bwd(const ymi_tensor* dout, const ymi_tensor* raw, const float* gamma, const float* save_mean,
                   const float* save_invstd, const float* beta, int32_t act, const ymi_tensor* draw, float* dgamma, float* dbeta,
                   void* workspace, size_t workspace_bytes, void* stream);

/* Two Conv blocks that read the SAME input as ONE convolution - the first convolutions of Detect's two branches, cv2[i][0] and cv3[i][0]
 * (nn/modules/head.py:44-59,71-72): w_packed holds the first convolution's packed weights followed by the second's (output channels
 * [0, split) / [split, cout)); BatchNorm is per channel, so with each half reading its own gamma / beta and updating its own running
 * statistics the result equals the two separate blocks.  raw / out / save_mean / save_invstd cover all cout channels.  split % 4 == 0. */
int ymi_conv2d_bn_silu_fwd_pair(const ymi_tensor* x, const void* w_packed, int64_t cout, int64_t split, int64_t kh, int64_t kw, int64_t stride,
                                const float* gamma, const float* beta, float* running_mean, float* running_var, const float* gamma2,
                                const float* beta2, float* running_mean2, float* running_var2, float momentum, float eps, int32_t act,
                                const ymi_tensor* raw, const ymi_tensor* out, float* save_mean, float* save_invstd, void* workspace,
                                size_t workspace_bytes, void* stream);
/* ... and the backward of its BatchNorm + activation (as ymi_bn_act_bwd; dgamma / dbeta hold all channels, the first block's first). */
int ymi_bn_act_bwd_pair(const ymi_tensor* dout, const ymi_tensor* raw, const float* gamma, const float* beta, const float* gamma2,
                        const float* beta2, int64_t split, const float* save_mean, const float* save_invstd, int32_t act,
                        const ymi_tensor* draw, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream);
/* dx = conv_transpose(dy, w): operand packed by ymi_pack_conv_weight_dgrad.  Adjoint of conv.py:79. */
int ymi_conv2d_bwd_data(const ymi_tensor* dy, const void* w_dgrad_packed, int64_t cin, int64_t kh, int64_t kw, int64_t stride,
                        const ymi_tensor* dx, void* stream);
/* the same with up to two addends in the epilogue: dx = dgrad(dy) + add1 (+ add2).  An addend may BE dx (in-place
 * accumulation).  This is how the gradient sums of tensors with several consumers (Bottleneck shortcut block.py:488, the
 * two Detect branches head.py:72, neck skip connections yolov8.yaml:760-773, SwinBlock residuals swin_block.py:52-53) are
 * formed without separate add kernels.  kh = kw = 1 with stride 2: only the pixels on the stride grid receive a gradient; the others
 * are left as the caller prepared them (zeros) and addends must be NULL (EINVAL otherwise). */
int ymi_conv2d_bwd_data_add(const ymi_tensor* dy, const void* w_dgrad_packed, int64_t cin, int64_t kh, int64_t kw, int64_t stride,
                            const ymi_tensor* add1, const ymi_tensor* add2, const ymi_tensor* dx, void* stream);
/* ... and several independent STRIDE-1 data gradients in one launch (k x k kernel, k in {1, 3}; addends as above). */
typedef struct ymi_dgrad_problem {
    const ymi_tensor* dy;
    const void* w_dgrad_packed;
    int64_t cin, k;
    const ymi_tensor* add1;
    const ymi_tensor* add2;
    const ymi_tensor* dx;
} ymi_dgrad_problem;
int ymi_conv2d_bwd_data_multi(const ymi_dgrad_problem* problems, int32_t n, void* stream);
/* dw (OIHW f32 [cout_real][cin_real][kh][kw], overwritten) = sum over pixels dy (x) x ; optional
 * dbias = column sums of dy: a buffer of dy->c floats (the PADDED channel count), of which the first cout_real are the bias gradient.  x / dy may carry zero-padded channels (x->c >= cin_real,
 * dy->c >= cout_real).  Split-K MFMA GEMM + ordered slab reduce (deterministic); workspace from
 * ymi_conv2d_bwd_weight_workspace. */
int ymi_conv2d_bwd_weight(const ymi_tensor* x, const ymi_tensor* dy, int64_t cout_real, int64_t cin_real, int64_t kh, int64_t kw,
                          int64_t stride, float* dw_oihw, float* dbias, void* workspace, size_t workspace_bytes, void* stream);
size_t ymi_conv2d_bwd_weight_workspace(int64_t m_rows, int64_t cout, int64_t cin, int64_t kh, int64_t kw);
/* The same GEMM with the ordered slab sum DEFERRED: `pending` (host memory) receives what ymi_wgrad_reduce_batch needs.
 * The caller keeps `workspace` (the slabs) alive until that launch.  One reduce launch then serves every layer of a
 * backward pass (the 73 per-layer reduce launches of YOLOv8s were pure latency). */
typedef struct ymi_wgrad_pending {
    const void* slab;    /* [splits][elems], float32 or (slab_bf16) bfloat16 first-level partials */
    float* dw;           /* OIHW destination */
    int64_t elems;       /* padded Cout * (taps * padded Cin) */
    int32_t splits, ng, cin, cout_real, cin_real, ntaps;
    int32_t lanes;       /* interleaved split chains per output element (4, 8, 16 or 32) */
    int32_t first_block; /* set by ymi_wgrad_reduce_batch */
    int32_t blocks;      /* workgroups this record needs: ceil(elems / e / (256 / lanes)), e = 8 elements per lane for bfloat16 slabs, 4 for float32 */
    int32_t slab_bf16;   /* 1: the slabs hold bfloat16 (the bf16 path), 0: float32 (parity mode) */
    const float* bias_slab; /* optional: [splits][padded Cout] float32 column sums of dY per split (the bias gradient's partials, formed by the */
    float* dbias;           /* weight-gradient GEMM itself); their sum over the splits goes to dbias [padded Cout].  NULL: no bias */
} ymi_wgrad_pending;
int ymi_conv2d_bwd_weight_deferred(const ymi_tensor* x, const ymi_tensor* dy, int64_t cout_real, int64_t cin_real, int64_t kh, int64_t kw,
                                   int64_t stride, float* dw_oihw, float* dbias, void* workspace, size_t workspace_bytes,
                                   ymi_wgrad_pending* pending, void* stream);
/* Riders.  mode 1: a deferred weight-gradient launch (ymi_conv2d_bwd_weight_deferred) is HELD BACK - at most one - until the next BatchNorm
 * backward on the same stream (ymi_bn_act_bwd / _pair) has issued its reduce pass; it is then launched with that layer's final pass (the sum of
 * the partial rows, the apply pass's coefficients: a 1-16 workgroup kernel at a dependent-launch latency otherwise) as extra workgroups of its own
 * grid.  The next deferred call, ymi_wgrad_reduce_batch and mode 0 issue a held launch as it is; mode 2 forgets it (after a backward pass that
 * raised).  The caller keeps operands and workspace of a deferred launch alive until the batched slab sum in any case.  No reference counterpart. */
int ymi_wgrad_hold(int32_t mode);
/* host_records: the n records of the pending layers (HOST memory; first_block is filled in here); device_table: device
 * scratch for n records.  The records reach the device inside kernel arguments (no host staging: graph-capturable). */
int ymi_wgrad_reduce_batch(const ymi_wgrad_pending* host_records, int32_t n, ymi_wgrad_pending* device_table, void* stream);

/* Backward of a 1x1 stride-1 Conv block, act(BN_train(conv1x1(x))), as the reduce and final pass of ymi_bn_act_bwd followed by ONE kernel that
 * applies the BatchNorm backward on its operand path and forms both products: dx = draw W (+ add1 (+ add2), as ymi_conv2d_bwd_data_add; an addend
 * may be dx) and the weight-gradient slabs of draw^T x (slab sum as ymi_conv2d_bwd_weight / _deferred: pending == NULL sums before the call returns
 * control of the stream).  draw, the gradient of the raw convolution output, is never stored; its bfloat16 values are those ymi_bn_act_bwd writes.
 * Scope (`_ok` says whether these tensors are inside it): bfloat16; dout / raw with 64 or 128 channels; x / dx / addends of one shape with the
 * pixels of dout and a multiple of 8 up to 512 channels; every tensor may be a channel slice of a wider buffer (16-byte aligned rows).
 * w_dgrad_packed: ymi_pack_conv_weight_dgrad's operand [cin][cout].  dw_oihw: [cout][cin] float32.  workspace >= ymi_conv1x1_bn_act_bwd_workspace bytes;
 * with a pending record the caller keeps it alive until ymi_wgrad_reduce_batch.  The launch is never held for a rider (it produces dx); a held
 * launch rides with this call's final pass as with ymi_bn_act_bwd's.  No reference counterpart (Conv.forward's autograd, nn/modules/conv.py:69-79). */
int ymi_conv1x1_bn_act_bwd_ok(const ymi_tensor* dout, const ymi_tensor* raw, const ymi_tensor* x, const ymi_tensor* add1, const ymi_tensor* add2,
                              const ymi_tensor* dx);
size_t ymi_conv1x1_bn_act_bwd_workspace(int64_t m_rows, int64_t cout, int64_t cin);
int ymi_conv1x1_bn_act_bwd(const ymi_tensor* dout, const ymi_tensor* raw, const float* gamma, const float* save_mean, const float* save_invstd,
                           const float* beta, int32_t act, const ymi_tensor* x, const void* w_dgrad_packed, const ymi_tensor* add1,
                           const ymi_tensor* add2, const ymi_tensor* dx, float* dgamma, float* dbeta, float* dw_oihw, void* workspace,
                           size_t workspace_bytes, ymi_wgrad_pending* pending, void* stream);

/* The model's FIRST Conv block on the float32 NCHW image the caller hands over (cfg/models/v8/yolov8.yaml:738 `Conv [64, 3, 2]` through
 * nn/modules/conv.py:50-79): act(BatchNorm_train(conv 3x3, stride 2, pad 1)) as DIRECT kernels that never store the raw convolution output
 * (27 products per output: recomputing is cheaper than reading back; csrc/first_conv.hip).  c <= 4, cout in {16, 32, 48, 64}, h even,
 * w % 4 == 0, bfloat16 outputs.
 *   forward : statistics pass over the image, finalize (running statistics updated), apply pass -> out.  x4 receives the image as NHWC
 *             bfloat16 [n, 4, h, w] (dense) - all the backward pass needs of the input.
 *             workspace >= (2 * cout + (ymi_first_conv_stat_blocks(n, h, w) + 64) * 2 * cout) * 4 bytes.
 *   backward: dgamma, dbeta [cout] and the weight gradient dw_oihw [cout, c, 3, 3] (the image receives none).  pending == NULL: dw is summed
 *             before the call returns control of the stream; else the slab sum is left to ymi_wgrad_reduce_batch (record in *pending).
 *             workspace >= ymi_first_conv_bwd_workspace bytes. */
int64_t ymi_first_conv_stat_blocks(int64_t n, int64_t h, int64_t w);
int ymi_first_conv_bn_act_fwd(const float* img_nchw, int64_t n, int64_t c, int64_t h, int64_t w, const float* weight_oihw, int64_t cout,
                              const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                              int32_t act, const ymi_tensor* x4, const ymi_tensor* out, float* save_mean, float* save_invstd,
                              void* workspace, size_t workspace_bytes, void* stream);
int64_t ymi_first_conv_bwd_workspace(int64_t n, int64_t h, int64_t w, int64_t cout);
int ymi_first_conv_bn_act_bwd(const ymi_tensor* x4, const float* weight_oihw, int64_t c, int64_t cout, const float* gamma, const float* beta,
                              const float* save_mean, const float* save_invstd, int32_t act, const ymi_tensor* dout, float* dgamma, float* dbeta,
                              float* dw_oihw, void* workspace, size_t workspace_bytes, ymi_wgrad_pending* pending, void* stream);

/* ------------------------------------------------------------------ depthwise convolution ---- */
/* Pure depthwise convolutions (groups == cin == cout), csrc/dwconv.hip: square k in {3, 5}, stride in {1, 2}, pad k/2, dilation 1, NHWC;
 * channels in whole 16-byte chunks (C % 8 == 0 in YMI_BF16, C % 4 == 0 in YMI_F32); every tensor may be a channel slice of a wider buffer.
 * w is the module's own [C][1][k][k] float32 weight and enters the arithmetic as float32 (no packed copy); accumulation is float32; every
 * output is rounded once, on store.  Direct kernels on the vector ALUs (no reduction over channels: nothing for the matrix pipe).
 *
 * y = act(scale[c] * conv(x, w) + bias[c]) + residual; scale, bias, residual may be NULL.  With stat_partials != NULL (scale, bias, residual
 * NULL, act none) the raw output plus per-workgroup rows [blocks][2][C] - sum and sum of squares of the ROUNDED outputs, the contract of
 * ymi_conv2d_fwd, so ymi_bn_finalize reads them unchanged; *host_stat_blocks receives `blocks` <= ymi_dwconv2d_stat_blocks().
 * Replaces the grouped F.conv2d of nn/modules/conv.py:79,91 as DWConv (conv.py:194-209) and GhostConv.cv2 (conv.py:357-358,370-371) call it. */
int ymi_dwconv2d_fwd(const ymi_tensor* x, const float* w, int64_t k, int64_t stride, const float* scale, const float* bias, int32_t act,
                     const ymi_tensor* residual, const ymi_tensor* y, float* stat_partials, int64_t* host_stat_blocks, void* stream);
int64_t ymi_dwconv2d_stat_blocks(int64_t n, int64_t ho, int64_t wo, int64_t c);
/* The train-mode depthwise Conv block in one call: the kernel above (raw, statistics rows) -> ymi_bn_finalize -> ymi_scale_shift_act (with the
 * optional residual).  Arguments as ymi_conv2d_bn_silu_fwd; workspace >= (ymi_dwconv2d_stat_blocks * 2 * C + 2 * C) * 4 bytes.  raw, save_mean
 * and save_invstd are what ymi_bn_act_bwd takes.  Replaces Conv.forward, nn/modules/conv.py:69-79, for g == c1 == c2. */
int ymi_dwconv2d_bn_act_fwd(const ymi_tensor* x, const float* w, int64_t k, int64_t stride, const float* gamma, const float* beta,
                            float* running_mean, float* running_var, float momentum, float eps, int32_t act, const ymi_tensor* residual,
                            const ymi_tensor* raw, const ymi_tensor* out, float* save_mean, float* save_invstd, void* workspace,
                            size_t workspace_bytes, void* stream);
/* dx = conv_transpose(dy, w) (+ add); add may be NULL and may BE dx (in-place accumulation: a thread reads its addend before it stores).
 * Stride 1: the forward body with the taps rotated; stride 2: a gather over the taps of matching parity (no atomics).  Adjoint of conv.py:79
 * for g == c1 == c2; the addend forms the gradient sum of GhostConv's y (conv.py:370-371: y feeds the concat and cv2). */
int ymi_dwconv2d_bwd_data(const ymi_tensor* dy, const float* w, int64_t k, int64_t stride, const ymi_tensor* add, const ymi_tensor* dx, void* stream);
/* dw ([C][1][k][k] float32, overwritten) = sum over pixels of dy * x per tap and channel: every workgroup sums its pixels on chip and stores
 * one row [k*k][C] in `workspace`; a second launch adds the rows in a fixed order.  No float atomics: bit-identical from run to run.
 * workspace >= ymi_dwconv2d_bwd_weight_workspace(dy->n, dy->h, dy->w, C, k) bytes.  Weight gradient of conv.py:79 for g == c1 == c2. */
int ymi_dwconv2d_bwd_weight(const ymi_tensor* x, const ymi_tensor* dy, int64_t k, int64_t stride, float* dw, void* workspace,
                            size_t workspace_bytes, void* stream);
size_t ymi_dwconv2d_bwd_weight_workspace(int64_t n, int64_t ho, int64_t wo, int64_t c, int64_t k);

/* -------------------------------------------------------------------- SPPF pooling cascade ---- */

/* y1 = maxpool_k(y0), y2 = maxpool_k(y1), y3 = maxpool_k(y2), stride 1, pad k/2 (-inf):
 * nn/modules/block.py:220,225.  One LDS-staged kernel; y1..y3 are usually channel slices of the
 * concat buffer that SPPF.cv2 reads. */
int ymi_sppf_pool3_fwd(const ymi_tensor* y0, int64_t k, const ymi_tensor* y1, const ymi_tensor* y2, const ymi_tensor* y3, void* stream);
/* Adjoint of the cascade: dx = dy0 + route(dy1 + route(dy2 + route(dy3 | y2) | y1) | y0), a deterministic gather in which every
 * window's gradient goes to its first arg-max in row-major order (PyTorch's max_pool2d tie rule).  No input is modified; dx may
 * not alias them.  Maps that fit LDS whole (<= ~2100 pixels in bf16) run in one launch with the running gradient in f32 and need
 * no workspace; larger maps run stage by stage through `workspace` (ymi_sppf_pool3_bwd_workspace bytes, 16-byte aligned), the
 * intermediate gradients rounded to the tensor dtype like the reference's. */
int64_t ymi_sppf_pool3_bwd_workspace(int64_t n, int64_t h, int64_t w, int64_t c, int dtype);
int ymi_sppf_pool3_bwd(const ymi_tensor* y0, const ymi_tensor* y1, const ymi_tensor* y2, int64_t k, const ymi_tensor* dy0,
                       const ymi_tensor* dy1, const ymi_tensor* dy2, const ymi_tensor* dy3, const ymi_tensor* dx, void* workspace,
                       int64_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------------- CBAM ---- */

/* out = x * ca * sa with ca = sigmoid(MLP(avg) + MLP(max)) (nn/modules/cbam.py:29-38),
 * sa = sigmoid(conv7x7([mean_c(x*ca), max_c(x*ca)])) (cbam.py:48-53), composed as cbam.py:62-71.
 * w1: [hidden][C] f32, w2: [C][hidden] f32, wsa: [2][k][k] f32.  Saved for backward: ca [N][C] f32,
 * smap [N][H][W][2] f32 (mean,max of x*ca), sa [N][H][W] f32, and the arg-max indices.
 * x, out, dout, dx: c and ld multiples of 4 and the base on a 4-element boundary (YMI_EINVAL otherwise);
 * k = 3 or 7, 1 <= hidden <= 1024, and C <= 1024 in the backward. */
int ymi_cbam_fwd(const ymi_tensor* x, const float* w1, const float* w2, int64_t hidden, const float* wsa, int64_t ksa,
                 const ymi_tensor* out, float* ca, float* pooled /*[N][2][C]*/, int32_t* pool_argmax /*[N][C]*/, float* smap,
                 int32_t* smap_argmax /*[N][H][W]*/, float* sa, void* stream);
int ymi_cbam_bwd(const ymi_tensor* x, const ymi_tensor* dout, const float* w1, const float* w2, int64_t hidden, const float* wsa,
                 int64_t ksa, const float* ca, const float* pooled, const int32_t* pool_argmax, const float* smap,
                 const int32_t* smap_argmax, const float* sa, const ymi_tensor* dx, float* dw1, float* dw2, float* dwsa,
                 void* workspace, size_t workspace_bytes, void* stream);
size_t ymi_cbam_bwd_workspace(int64_t n, int64_t h, int64_t w, int64_t c, int64_t hidden);

/* ------------------------------------------------------------------------------ SwinBlock ---- */

/* Integer index maps of nn/modules/swin_block.py:8-20 (bit-exact requirement): for window-ordered
 * token t the flat padded-grid pixel index, tokens = n*hp*wp. */
int ymi_window_partition_index(int64_t n, int64_t hp, int64_t wp, int64_t ws, int32_t* index, void* stream);
/* tokens[t,:] = x[pixel(t),:] (zero where the pixel is padding) / inverse with crop. */
int ymi_window_partition(const ymi_tensor* x, int64_t ws, const ymi_tensor* tokens /*n=1,h=1,w=T*/, void* stream);
int ymi_window_reverse(const ymi_tensor* tokens, int64_t ws, const ymi_tensor* x, void* stream);
/* t = LayerNorm(gather(x)) : pad + 'b c h w -> b h w c' + window_partition + norm1 fused
 * (swin_block.py:41-50).  With ws == 0 no gather: plain row-wise LayerNorm (norm2, :53).
 * Saves mean / rstd per token for backward. */
int ymi_layernorm_fwd(const ymi_tensor* x, int64_t ws, const float* gamma, const float* beta, float eps, const ymi_tensor* out,
                      float* mean, float* rstd, void* stream);
/* dx = LayerNorm adjoint (written through the window map when ws != 0; pad tokens are dropped =
 * the crop of :58); accumulate != 0 adds into dx instead (LayerNorm input that also feeds a skip). */
int ymi_layernorm_bwd(const ymi_tensor* x, int64_t ws, const ymi_tensor* dout, const float* gamma, const float* mean,
                      const float* rstd, const ymi_tensor* dx, int32_t accumulate, float* dgamma, float* dbeta, void* workspace,
                      size_t workspace_bytes, void* stream);
/* the same with an addend: dx = LayerNorm gradient + add (the gradient the LN input receives from its other consumers,
 * e.g. the residual branch of swin_block.py:52-53); add may be dx itself. */
int ymi_layernorm_bwd_add(const ymi_tensor* x, int64_t ws, const ymi_tensor* dout, const float* gamma, const float* mean, const float* rstd,
                          const ymi_tensor* add, const ymi_tensor* dx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                          void* stream);
/* Window attention core of nn.MultiheadAttention as used at swin_block.py:29,51:
 * qkv [T][3C] (q pre-scaled is NOT assumed: the kernel scales by 1/sqrt(hd)); per (window, head)
 * P = softmax(q k^T / sqrt(hd)) over all `wlen` keys, o = P v; out [T][C].  lse [T][heads] saved.
 * Any window length; hd = C / heads a multiple of 4, at most 256 (wider: YMI_EINVAL, nothing is launched).  No atomics,
 * run-to-run identical.  (The PSA entry points below keep their own limit of 192.) */
int ymi_window_attention_fwd(const ymi_tensor* qkv, int64_t wlen, int64_t heads, const ymi_tensor* out, float* lse, void* stream);
int ymi_window_attention_bwd(const ymi_tensor* qkv, const ymi_tensor* out, const ymi_tensor* dout, const float* lse, int64_t wlen,
                             int64_t heads, const ymi_tensor* dqkv, void* stream);
/* Attention core of the reference's block.py Attention (C2PSA / PSABlock): full-map self-attention per image and head on
 * qkv [T][heads * (2 kd + hd)], packed per head as [q (kd) | k (kd) | v (hd)]; T is a whole number of images of `tokens`
 * tokens each (any positive count).  P = softmax(q k^T * kd^-0.5) over the image's tokens, o = P v; out [T][heads * hd];
 * v_out (may be null) receives V compacted to [T][heads * hd]; lse [T][heads] saved.  Flash-style tiles: no atomics,
 * run-to-run identical.  kd and hd: multiples of 4, at most 192. */
int ymi_psa_attention_fwd(const ymi_tensor* qkv, int64_t tokens, int64_t heads, int64_t kd, const ymi_tensor* out, const ymi_tensor* v_out,
                          float* lse, void* stream);
/* dqkv [T][heads * (2 kd + hd)]; dv_add [T][heads * hd] (may be null) is added into the V columns in float32, before the store. */
int ymi_psa_attention_bwd(const ymi_tensor* qkv, const ymi_tensor* out, const ymi_tensor* dout, const float* lse, const ymi_tensor* dv_add,
                          int64_t tokens, int64_t heads, int64_t kd, const ymi_tensor* dqkv, void* stream);
/* Generic token GEMM backward helpers (nn.Linear adjoint): column sums for bias gradients. */
int ymi_colsum(const ymi_tensor* x, float* out /*[c]*/, void* workspace, size_t workspace_bytes, void* stream);
/* dx = dy * gelu'(pre) (exact erf GELU, swin_block.py:33). */
int ymi_gelu_bwd(const ymi_tensor* pre, const ymi_tensor* dy, const ymi_tensor* dx, void* stream);

/* ---- v8 detection loss on the per-level Detect maps ----------------------------------------------------------
 * Replaces v8DetectionLoss.__call__ (utils/loss.py:201-255) with its helpers: preprocess (loss.py:176-191),
 * bbox_decode (loss.py:193-199), TaskAlignedAssigner.forward (utils/tal.py:45-104), BboxLoss / DFLoss
 * (loss.py:65-120) and bbox_iou(CIoU=True) (utils/metrics.py:74-134).  box_maps[l] is the NHWC map
 * [B,H_l,W_l,64] of Detect.cv2[l] (reg_max 16), cls_maps[l] the map [B,H_l,W_l,nc] of Detect.cv3[l]; anchors are
 * ordered level by level, row-major, as the reference's concat.  All arithmetic is f32; maps may be f32 or bf16. */

/* ragged label rows (image index, class, xywh normalised) -> dense out[batch, max_boxes, 5] = (class, xyxy in pixels);
 * rows keep their order inside an image, unused slots are zero, rows beyond max_boxes of an image are dropped. */
int ymi_detect_targets(const float* batch_idx, const float* cls, const float* bboxes_xywhn, int64_t n, int64_t batch, int64_t max_boxes,
                       float img_w, float img_h, float* out, void* stream);
/* bytes of the state (kept from forward to backward) and of the scratch workspace */
int ymi_detect_loss_sizes(int64_t batch, int64_t anchors, int64_t max_boxes, size_t* state_bytes, size_t* workspace_bytes);
/* raw[3] = (box, cls, dfl) sums divided by max(sum of target scores, 1), before the hyper-parameter gains.
 * out_scale == NULL: loss_out[3] = raw.  out_scale (device [6]): loss_out[6], loss_out[k] = raw[k] * out_scale[k] and
 * loss_out[3 + k] = raw[k] * out_scale[3 + k]: the criterion's two results (loss * gains * batch, loss * gains; reference
 * utils/loss.py:250-255) from this one launch.
 * strides: host array [nl]; targets: device [batch, max_boxes, 5] as written by ymi_detect_targets. */
int ymi_detect_loss_fwd(int32_t nl, const ymi_tensor* box_maps, const ymi_tensor* cls_maps, const float* strides, const float* targets,
                        int64_t max_boxes, int32_t topk, float alpha, float beta, const float* out_scale, float* loss_out, void* state,
                        size_t state_bytes, void* workspace, size_t workspace_bytes, void* stream);
/* gradients of sum_k grad_loss[k] * grad_scale[k] * raw[k] with respect to the maps (grad_loss: device [3]; grad_scale: device [3]
 * or NULL = 1: the out_scale[0..2] the forward multiplied its differentiable result by).  dcls_maps may be channel slices of
 * wider buffers (ld > c); they may also have MORE channels than the class maps (the same count on every level): the extra
 * channels are written as zeros (channel-padded gradient buffers need no separate fill). */
int ymi_detect_loss_bwd(int32_t nl, const ymi_tensor* box_maps, const ymi_tensor* cls_maps, const float* strides, const void* state,
                        size_t state_bytes, const float* grad_loss, const float* grad_scale, const ymi_tensor* dbox_maps,
                        const ymi_tensor* dcls_maps, void* stream);

/* Detect._inference (nn/modules/head.py:103-142, non-export branch; DFL nn/modules/block.py:58-77; make_anchors /
 * dist2bbox utils/tal.py:364-388): per level l a box map [B,H,W,64] and a class map [B,H,W,nc] (NHWC, channel slices of
 * the concatenated Detect output are fine) -> y [B][4+nc][A] float32: rows 0..3 = (cx, cy, w, h) in pixels, rows 4.. =
 * sigmoid(class logits); anchors in the reference's order (level, y, x), centre offset 0.5. */
int ymi_detect_decode(int32_t nl, const ymi_tensor* box_maps, const ymi_tensor* cls_maps, const float* strides, float* y, void* stream);

/* ------------------------------------------------------------------ instance segmentation ---- */

/* nn.ConvTranspose2d(c, c, 2, 2, 0) of Proto (nn/modules/block.py:80-100) is four 1x1 GEMMs, one per output sub-pixel: ymi_conv2d_fwd with the
 * weight viewed as [4c, c] gives src [N,H,W,4c], channel (2a + b) * c + k; this copy puts it at dst [N,2H,2W,c] (2y + a, 2x + b, k).
 * Channels and pixel strides in whole 16-byte chunks, both tensors of one dtype. */
int ymi_depth_to_space2(const ymi_tensor* src, const ymi_tensor* dst, void* stream);
/* the inverse: src [N,2H,2W,c] -> dst [N,H,W,4c] (the output gradient, for the data- and weight-gradient GEMMs) */
int ymi_space_to_depth2(const ymi_tensor* src, const ymi_tensor* dst, void* stream);
/* ymi_detect_loss_fwd that also hands the assignment over: gidx_out (device [batch, anchors] int32, or NULL) receives the gt index of every
 * anchor (-1: background), reference utils/tal.py target_gt_idx under fg_mask.  Everything else is computed as without it. */
int ymi_detect_loss_fwd_assign(int32_t nl, const ymi_tensor* box_maps, const ymi_tensor* cls_maps, const float* strides, const float* targets,
                               int64_t max_boxes, int32_t topk, float alpha, float beta, const float* out_scale, float* loss_out, void* state,
                               size_t state_bytes, void* workspace, size_t workspace_bytes, int32_t* gidx_out, void* stream);
/* Segment's eval output (nn/modules/head.py:186-208): ymi_detect_decode with the anchors' mask coefficients behind the classes,
 * y [B][4+nc+nm][A] float32; mc_maps[l]: [B,H_l,W_l,nm] of Segment.cv4[l]. */
int ymi_detect_decode_seg(int32_t nl, const ymi_tensor* box_maps, const ymi_tensor* cls_maps, const ymi_tensor* mc_maps, const float* strides,
                          float* y, void* stream);
/* ---- oriented boxes: the OBB head's angle, v8OBBLoss and the head's eval output ------------------------------------------------------
 * Reference: nn/modules/head.py:211-238 (OBB), utils/loss.py:607-720 (v8OBBLoss), loss.py:111-132 (RotatedBboxLoss), utils/tal.py:329-361
 * (RotatedTaskAlignedAssigner), tal.py:397-416 (dist2rbox), utils/metrics.py:178-239 (probiou).  A box is (x, y, w, h, r): centre, extents
 * along its own axes, angle in radians.  float32 arithmetic on bf16 or float32 maps; fixed summation order, no atomics, nothing read back,
 * every shape static given max_boxes. */

/* angle[B][A] (float32 radians) = (sigmoid(logit) - 0.25) * pi from the per-level one-channel logit maps [B,H_l,W_l,1] of OBB.cv4[l] (channel
 * slices of padded buffers: a pixel stride), anchors level by level, row-major, as the reference's view + cat (head.py:225-227). */
int ymi_obb_angle_fwd(int32_t nl, const ymi_tensor* logit_maps, float* angle, void* stream);
/* dlogit = dangle * pi * s * (1 - s), s = sigmoid(logit).  dlogit_maps[l] is shaped as logit_maps[l] but may have MORE channels (the same count
 * on every level): the channels behind the first are written as zeros. */
int ymi_obb_angle_bwd(int32_t nl, const ymi_tensor* logit_maps, const float* dangle, const ymi_tensor* dlogit_maps, void* stream);
/* ragged label rows (image index, class, xywhr with xywh normalised) -> dense out[batch, max_boxes, 6] = (class, xywh in pixels, angle), in
 * stable order within an image, unused slots zero.  The reference's filter comes first (loss.py:655-656): a row is dropped unless
 * w * img_h >= 2 and h * img_w >= 2 - the width against the image HEIGHT, as the reference multiplies them. */
int ymi_obb_targets(const float* batch_idx, const float* cls, const float* bboxes_xywhr, int64_t n, int64_t batch, int64_t max_boxes, float img_w,
                    float img_h, float* out, void* stream);
int ymi_obb_loss_sizes(int64_t batch, int64_t anchors, int64_t max_boxes, size_t* state_bytes, size_t* workspace_bytes);
/* v8OBBLoss.__call__ in the stages of ymi_detect_loss_fwd; box_maps, cls_maps, strides, out_scale and loss_out as there; angle: device
 * [batch, anchors] as ymi_obb_angle_fwd writes it; targets: device [batch, max_boxes, 6] as ymi_obb_targets writes them (a row is a label when
 * its five box values sum to more than 0).
 *   decode  : DFL expectation, dist2rbox -> [B, A, 5] in grid units
 *   metric  : inside test of the rotated rectangle (four dot products, an edge counts as inside), overlap = probiou(gt, pred * stride)
 *             clamped at 0, metric = score^alpha * overlap^beta
 *   top-k, claim by highest overlap, per-gt maxima: the detection loss's kernels
 *   finalize: target (xywh / stride, angle), weight, label per anchor
 *   sums    : (1 - probiou(pred, target)) * weight; DFL against the target's unrotated extents; BCE; the fixed-order final sums */
int ymi_obb_loss_fwd(int32_t nl, const ymi_tensor* box_maps, const ymi_tensor* cls_maps, const float* angle, const float* strides, const float* targets,
                     int64_t max_boxes, int32_t topk, float alpha, float beta, const float* out_scale, float* loss_out, void* state, size_t state_bytes,
                     void* workspace, size_t workspace_bytes, void* stream);
/* gradients as ymi_detect_loss_bwd, and dangle [batch, anchors] float32: through the covariance and through the centre's rotation about the
 * anchor.  probiou's clamps pass no gradient outside their range; background anchors get exact zeros in dbox_maps and dangle. */
int ymi_obb_loss_bwd(int32_t nl, const ymi_tensor* box_maps, const ymi_tensor* cls_maps, const float* angle, const float* strides, const void* state,
                     size_t state_bytes, const float* grad_loss, const float* grad_scale, const ymi_tensor* dbox_maps, const ymi_tensor* dcls_maps,
                     float* dangle, void* stream);
/* OBB's eval output (head.py:222-238): y [B][4+nc+1][A] float32, rows 0..3 = dist2rbox(DFL(box), angle, anchor) * stride as (x, y, w, h),
 * rows 4..4+nc-1 the class sigmoids, row 4+nc the angle.  ymi_detect_decode is untouched. */
int ymi_detect_decode_obb(int32_t nl, const ymi_tensor* box_maps, const ymi_tensor* cls_maps, const float* angle, const float* strides, float* y,
                          void* stream);

/* The mask term of v8SegmentationLoss (utils/loss.py:349-438; crop_mask utils/ops.py:661-677) with overlap-encoded masks, nm = 32.
 * mc_maps[l]: [B,H_l,W_l,32] coefficient maps, proto: [B,mh,mw,32] (both f32 or bf16, read as they are; sums in f32); masks: device
 * [B,masks_h,masks_w] uint8 (masks_f32 = 0) or float32, read with F.interpolate(mode="nearest")'s index rule when its size is not (mh, mw);
 * gidx: as ymi_detect_loss_fwd_assign writes it; targets: as ymi_detect_targets writes them; det_out6: the six results of the detection
 * loss; scale6: its out_scale.  out8[0..3] = (box, seg, cls, dfl) scaled for backward, out8[4..7] = scaled for logging; seg takes the box
 * gain.  Foreground anchors per image are bounded by min(anchors, topk * max_boxes): every grid is static, nothing is read back, no atomics
 * (fixed summation order).  state: ymi_mask_loss_sizes bytes, kept for the backward.
 * Precondition the library cannot check: gidx holds batch * A entries and targets batch * max_boxes * 5, with A = the sum of H_l * W_l over
 * mc_maps and the levels in the order of the box maps the assignment was made on (ops.mask_loss checks the shapes). */
int ymi_mask_loss_sizes(int64_t batch, int64_t anchors, int64_t max_boxes, int32_t topk, size_t* state_bytes);
int ymi_mask_loss_fwd(int32_t nl, const ymi_tensor* mc_maps, const ymi_tensor* proto, const void* masks, int32_t masks_f32, int64_t masks_h,
                      int64_t masks_w, const int32_t* gidx, const float* targets, int64_t max_boxes, int32_t topk, float img_w, float img_h,
                      const float* det_out6, const float* scale6, float* out8, void* state, size_t state_bytes, void* stream);
/* gradients of grad_out8[1] * out8[1] with respect to the coefficient maps (rows of foreground anchors only: the caller zero-fills dmc_maps)
 * and to the prototype map (every pixel written). */
int ymi_mask_loss_bwd(int32_t nl, const ymi_tensor* mc_maps, const ymi_tensor* proto, const void* masks, int32_t masks_f32, int64_t masks_h,
                      int64_t masks_w, int64_t max_boxes, int32_t topk, const void* state, size_t state_bytes, const float* grad_out8,
                      const float* scale6, const ymi_tensor* dmc_maps, const ymi_tensor* dproto, void* stream);

/* non_max_suppression (utils/ops.py:181-332, as models/yolo/detect/val.py:113-133 and the predictor call it) on y [B][4+nc][A] float32 as
 * ymi_detect_decode writes it -> det [B][max_det][6] float32, rows (x1, y1, x2, y2, conf, cls) in kept order and zero past the count, and
 * count [B] int32 (csrc/nms.hip: three launches of B workgroups, no host round trip, no data-dependent grid: graph-capturable).
 *   candidates : multi_label (and nc > 1): every (anchor, class) with score > conf_thres; else the anchor's best class (first maximum) if its
 *                score > conf_thres; host_classes (HOST array of n_classes class ids) keeps only those classes: NULL = no filter, non-NULL
 *                with n_classes 0 = a filter that keeps nothing (the reference's result for an empty list)
 *   order      : descending score; equal scores by ascending anchor, then ascending class (the reference leaves ties to argsort and
 *                torchvision: this rule is the library's own); the first max_nms of that order enter the suppression
 *   suppression: greedy, the arithmetic of torchvision.ops.nms in float32 on the boxes offset by cls * max_wh (agnostic != 0: no offset):
 *                iou = inter / (area_i + area_j - inter), one rounding per operation, suppressed when iou > iou_thres with the threshold
 *                taken in float32 too (as torchvision's GPU kernel takes it; its CPU kernel compares the float32 iou with a double
 *                threshold, which differs only for an iou equal to float32(iou_thres) when that lies above iou_thres, e.g. 0.6)
 *   result     : the first max_det kept candidates with their original boxes (x -+ w/2, y -+ h/2)
 * max_det <= 2048, max_nms <= 2^20, thresholds in [0, 1].  The reference's wall-clock time limit (ops.py:328-330) is not reproduced.
 * workspace (8-byte aligned) of ymi_detect_nms_sizes bytes: B * pow2ceil(min(max_nms, A * nc)) 8-byte keys + the candidate counts. */
int ymi_detect_nms_sizes(int64_t batch, int64_t anchors, int64_t nc, int64_t max_nms, int64_t max_det, size_t* workspace_bytes);
int ymi_detect_nms(const float* y, int64_t batch, int64_t nc, int64_t anchors, float conf_thres, float iou_thres, int32_t multi_label,
                   int32_t agnostic, const int32_t* host_classes, int32_t n_classes, int64_t max_det, int64_t max_nms, float max_wh, float* det,
                   int32_t* count, void* workspace, size_t workspace_bytes, void* stream);
/* The same on Segment's eval output y [B][4 + nc + nm][A] (ymi_detect_decode_seg): only rows 4 .. 4 + nc are scores; every decision, and so det
 * and count, are ymi_detect_nms's on y[:, :4 + nc], bit for bit.  coef [B][max_det][nm] float32 receives y[b][4 + nc + m][a] of the kept
 * anchors, zero past the count.  Any nm >= 1; the workspace is ymi_detect_nms_sizes's. */
int ymi_detect_nms_seg(const float* y, int64_t batch, int64_t nc, int64_t nm, int64_t anchors, float conf_thres, float iou_thres, int32_t multi_label,
                       int32_t agnostic, const int32_t* host_classes, int32_t n_classes, int64_t max_det, int64_t max_nms, float max_wh, float* det,
                       int32_t* count, float* coef, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------- mask decode ---- */
/* process_mask / crop_mask (utils/ops.py:661-710) and the counts of mask_iou (utils/metrics.py:137), csrc/maskdec.hip.  One launch each, grids
 * from shapes only, no workspace, nothing read back; the only atomics are integer adds.  proto: the prototype map [B][nm][mh][mw] as Proto's
 * eval output has it (logical NCHW, NHWC memory: n = B, h = mh, w = mw, c = nm = YMI_MASK_NM, 16-byte aligned pixels), bfloat16 or float32.
 * (ih, iw): the network input's size, the space the boxes are in.
 *   logit      : the float32 sum over m of coef[m] * proto[b][m][r][c], channel order, one fused multiply-add per term
 *   crop       : x1' = x1 * float32(mw / iw), x2' likewise, y1' = y1 * float32(mh / ih), y2' likewise (one rounded product each); pixel (r, c)
 *                is inside when c >= x1' && c < x2' && r >= y1' && r < y2'; the cropped logit is 0 outside
 * ymi_process_mask: box [n][4] float32, coef [n][nm] float32, img [n] int32 (the row's image; outside [0, B): a zero mask) ->
 *   mask [n][oh][ow] uint8 (0 / 1), area [n] int32 (the mask's sum).  upsample == 0: (oh, ow) = (mh, mw), mask = cropped logit > 0.
 *   upsample != 0: (oh, ow) = (ih, iw) >= (mh, mw): the cropped logits resampled as F.interpolate(mode="bilinear", align_corners=False) does
 *   (the index and weight rule of ymi_scale_image), then > 0.
 * ymi_mask_overlap: det [batch][max_det][6], count [batch] and coef [batch][max_det][nm] as ymi_detect_nms_seg leaves them, boxes in network-
 *   input pixels; masks [batch][masks_h][masks_w]: the overlap encoding (0 background, v the image's v-th object), uint8 or float32
 *   (masks_f32 != 0), of the prototype map's size (other sizes are refused: the reference would resample) ->
 *   inter [batch][max_det][n_bins], area_pred [batch][max_det], area_gt [batch][n_bins] int32, n_bins <= YMI_MASK_MAX_BINS: over the pixels inside
 *   detection d's crop with logit > 0, area_pred counts one and inter[.][v] counts one where the encoding is v < n_bins; area_gt[v] counts
 *   the image's pixels whose encoding is v.  Rows at or beyond count[b] are zero.  mask_iou(label j, detection d) is then
 *   inter[d][j + 1] / ((area_gt[j + 1] + area_pred[d]) - inter[d][j + 1] + 1e-7f), every operand an exact integer (ymi_val_match_masks). */
#define YMI_MASK_NM 32
#define YMI_MASK_MAX_BINS 256
int ymi_process_mask(const ymi_tensor* proto, const float* box, const float* coef, const int32_t* img, int64_t n, int64_t ih, int64_t iw,
                     int32_t upsample, uint8_t* mask, int32_t* area, void* stream);
int ymi_mask_overlap(const float* det, const float* coef, const int32_t* count, int64_t batch, int64_t max_det, const ymi_tensor* proto, int64_t ih,
                     int64_t iw, const void* masks, int32_t masks_f32, int64_t masks_h, int64_t masks_w, int64_t n_bins, int32_t* inter,
                     int32_t* area_pred, int32_t* area_gt, void* stream);

/* ------------------------------------------------------------------------ image rescaling ---- */
/* F.interpolate(mode="bilinear", align_corners=False) of an image batch with what the reference does around it, as one launch
 * (csrc/resize.hip): utils/torch_utils.py:475-495 (scale_img), models/yolo/detect/train.py:100-114 (preprocess_batch), nn/tasks.py:392.
 *   src   : `planes` = B * C planes [h][w], NCHW contiguous; uint8 (src_uint8 != 0) or float32
 *   dst   : float32 planes [hp][wp]; rows < hs and columns < ws hold the interpolation to (hs, ws), the rest pad_value
 *           (F.pad(img, [0, wp - ws, 0, hp - hs], value)); hs <= hp, ws <= wp
 *   normalize (uint8 sources only): every source value is divided by 255 first, rounded as img.float() / 255 rounds
 *   flip_lr / flip_ud: the source is read as x.flip(3) / x.flip(2)
 * Arithmetic, in float32, one rounding per operation: scale = in / out, s = max((dst + 0.5) * scale - 0.5, 0), i0 = floor(s),
 * i1 = min(i0 + 1, in - 1), l1 = s - i0, l0 = 1 - l1, out = l0y * (l0x * a + l1x * b) + l1y * (l0x * c + l1x * d).  hs == h and
 * ws == w copies the converted source exactly. */
int ymi_scale_image(const void* src, int32_t src_uint8, int64_t planes, int64_t h, int64_t w, float* dst, int64_t hp, int64_t wp, int64_t hs,
                    int64_t ws, float pad_value, int32_t normalize, int32_t flip_lr, int32_t flip_ud, void* stream);
/* _descale_pred + _clip_augmented + the final torch.cat of nn/tasks.py:394-439 as one launch: n <= 3 decoded Detect outputs
 * src[i] [batch][rows = 4 + nc][anchors[i]] float32 (HOST arrays of n entries each); source i contributes its anchors [lo[i], hi[i]) to
 * out [batch][rows][sum (hi - lo)], in source order.  Rows 0..3 are divided by scale[i]; then row 0 becomes img_w[i] - x for flip[i] == 3
 * and row 1 becomes img_h[i] - y for flip[i] == 2 (flip 0: neither); the class rows are copied. */
int ymi_tta_merge(int32_t n, const float* const* src, const int64_t* anchors, const int64_t* lo, const int64_t* hi, const float* scale,
                  const int32_t* flip, const int64_t* img_h, const int64_t* img_w, int64_t batch, int64_t rows, float* out, void* stream);

/* ------------------------------------------------------------- prediction on real images ---- */
/* LetterBox (data/augment.py:1479-1603) and the conversion of engine/predictor.py:144-162 (BGR HWC uint8 -> RGB NCHW float / 255) for a
 * ragged list of images (csrc/resize.hip).  The GEOMETRY is the caller's: r, int(round(w * r)), dw / 2, int(round(dh - 0.1)) and the auto /
 * scale_fill / scaleup / center branches are host arithmetic (ops.letterbox states them as the reference does); the library receives integers.
 *   images : HOST array of n entries; src: DEVICE pointer to a contiguous [h][w][3] uint8 image; (hs, ws): the interpolated size;
 *            (top, left): where it lies in the destination; top + hs <= H, left + ws <= W
 *   dst    : float32 [n][3][H][W]; every element is written exactly once
 * The table travels in the kernel arguments, YMI_LETTERBOX_MAX images per launch; a longer list takes further launches.
 * Per destination element (y, x) of image i, plane c, in this order:
 *   1. outside [top, top + hs) x [left, left + ws): level = pad_value (a grey level in [0, 255]; the reference pads with 114)
 *   2. hs == h and ws == w: level = src[y - top][x - left][cs], cs = 2 - c with bgr != 0, else c - the byte itself, no arithmetic
 *   3. else, in float32 with one rounding per operation (the rule of ymi_scale_image; the source coordinate is OpenCV INTER_LINEAR's):
 *      scale = in / out, s = max((dst + 0.5) * scale - 0.5, 0), i0 = floor(s), i1 = min(i0 + 1, in - 1), l1 = s - i0, l0 = 1 - l1,
 *      v = l0y * (l0x * a + l1x * b) + l1y * (l0x * c + l1x * d) on the BYTE VALUES a..d; level = floorf(v + 0.5f)
 *   4. normalize != 0: dst = level / 255 rounded as img.float() / 255 rounds; else dst = level.  Either way the output lies on the lattice of the
 *      reference's uint8 image.  (OpenCV interpolates with 11-bit fixed-point coefficients: its level may differ from step 3's by one.) */
#define YMI_LETTERBOX_MAX 32
typedef struct ymi_letterbox_image {
    const uint8_t* src;
    int32_t h, w, hs, ws, top, left;
} ymi_letterbox_image;
int ymi_letterbox_batch(const ymi_letterbox_image* images, int64_t n, float* dst, int64_t H, int64_t W, int32_t pad_value, int32_t normalize,
                        int32_t bgr, void* stream);
/* scale_boxes + clip_boxes (utils/ops.py:93-127, :335-354) as one launch on det [batch][max_det] rows of `cols` >= 4 float32 columns, row
 * stride det_ld, and count [batch] int32 as ymi_detect_nms leaves them (count == NULL: every row is live).
 *   params : DEVICE float32 [batch][5] = (gain, pad_x, pad_y, w0, h0) per image; gain and pad are the caller's (the `ratio_pad is None` branch
 *            of scale_boxes is host arithmetic, Python's round included)
 * Per live row, in float32, in this order:
 *   1. padding != 0: x1 = x1 - pad_x, y1 = y1 - pad_y and, unless xywh != 0, x2 = x2 - pad_x, y2 = y2 - pad_y
 *   2. all four are divided by gain: the IEEE float32 quotient x / float32(gain), which is what `tensor /= python_float` computes - neither
 *      a product with the reciprocal nor a double-precision division
 *   3. columns 0 and 2 are clamped to [0, w0], columns 1 and 3 to [0, h0] (min(max(v, 0), hi); xywh rows are clamped the same way, as the
 *      reference does); columns 4.. are copied
 * Rows at or beyond count[b] are written as zeros out of place and left as they are in place (out == det, out_ld == det_ld). */
int ymi_scale_boxes(const float* det, int64_t det_ld, const int32_t* count, const float* params, int64_t batch, int64_t max_det, int64_t cols,
                    int32_t padding, int32_t xywh, float* out, int64_t out_ld, void* stream);

/* ------------------------------------------------------------------- training augmentation ---- */
/* The reference's v8_transforms at perspective = 0 (data/augment.py): Mosaic._mosaic4 (:658-714), RandomPerspective (:1017-1078, :1185-1261),
 * RandomHSV (:1346-1382), RandomFlip (:1433-1476) and the conversion to the float32 NCHW batch, csrc/augment.hip.  Every random draw and all the
 * geometry are the caller's (data.augment draws, ops.mosaic_placement / ops.affine_matrix compute); the library receives a table row per image.
 *
 * DISCLOSURE.  The warp rule and the colour round trip below are OpenCV's warpAffine INTER_LINEAR fixed-point scheme and its 8-bit
 * BGR <-> HSV conversion AS RECALLED: no OpenCV was at hand when this was written, so neither is verified against OpenCV.  The rules written here
 * are the contract; the tests hold the kernels to them bit for bit.
 *
 * ymi_augment_batch: images.  One launch per YMI_AUGMENT_MAX images.
 *   table   : HOST array of n rows, validated here (sources lie within their images, placements within the canvas, coordinates below 2^30);
 *   table_d : the SAME n rows in DEVICE memory (the caller uploads them together with the images: one copy); the kernel reads these
 *   dst     : float32 [n][3][size][size]; every element is written exactly once
 * A row: n_src (1..4) sources, each a DEVICE pointer to a contiguous [h][w][3] uint8 image and its placement (x1a, y1a, x2a, y2a, x1b, y1b) as
 * _mosaic4 computes it: canvas pixel (cy, cx) with x1a <= cx < x2a, y1a <= cy < y2a is source pixel (cy - y1a + y1b, cx - x1a + x1b).
 * Placements do not overlap (the first that holds a pixel gives it).  The canvas (canvas_h x canvas_w; 2s x 2s for a mosaic, the image itself
 * for n_src = 1) is never materialised: a canvas pixel that no placement holds, and every pixel outside the canvas, is `border` (114).
 * Per destination element (y, x) of image i, plane c, in this order:
 *   1. flips: yw = flip_ud ? size - 1 - y : y, xw = flip_lr ? size - 1 - x : x (the reference flips after the warp: the flipped image's
 *      pixel (y, x) is the warped image's pixel (yw, xw))
 *   2. warp, with the inverse 2 x 3 matrix A in double (ops.affine_matrix inverts M as warpAffine does) and rn = round-half-even to int:
 *        X = (rn(A[0] * xw * 1024) + rn((A[1] * yw + A[2]) * 1024) + 16) >> 5      (every product and sum rounded on its own: no fma;
 *        Y = (rn(A[3] * xw * 1024) + rn((A[4] * yw + A[5]) * 1024) + 16) >> 5       >> is arithmetic)
 *        sx = X >> 5, fx = X & 31, sy = Y >> 5, fy = Y & 31
 *        level = ((32 - fx) * (32 - fy) * p00 + fx * (32 - fy) * p01 + (32 - fx) * fy * p10 + fx * fy * p11 + 512) >> 10
 *      with p00 = canvas(sy, sx), p01 = canvas(sy, sx + 1), p10 = canvas(sy + 1, sx), p11 = canvas(sy + 1, sx + 1) per BGR channel, each
 *      tap resolved by itself as above
 *   3. lut != NULL (RandomHSV; the reference skips the stage when all three gains are 0): (b, g, r) -> (h, s, v) in integers,
 *        v = max(b, g, r), d = v - min(b, g, r), sdiv[k] = rn((255 << 12) / (double)k), hdiv[k] = rn((180 << 12) / (6.0 * k)), sdiv[0] = hdiv[0] = 0
 *        s = (d * sdiv[v] + (1 << 11)) >> 12
 *        h = v == r ? g - b : v == g ? b - r + 2 * d : r - g + 4 * d;  h = (h * hdiv[d] + (1 << 11)) >> 12;  h < 0: h += 180
 *      then h = lut[h], s = lut[256 + s], v = lut[512 + v] (three 256-byte tables the caller builds as RandomHSV does; hue entries stay
 *      below 180, which is the caller's to see to: a larger one is read as hue 0), then back in
 *      float32, every operation rounded on its own: H = h * (6.0f / 180.0f), S = s * (1.0f / 255.0f), V = v * (1.0f / 255.0f);
 *        s == 0: b = g = r = V;  else k = floor(H), f = H - k,
 *        t0 = V, t1 = V * (1 - S), t2 = V * (1 - S * f), t3 = V * (1 - S * (1 - f)),
 *        (b, g, r) = (t1,t3,t0) (t1,t0,t2) (t3,t0,t1) (t0,t2,t1) (t0,t1,t3) (t2,t1,t0) for k = 0..5
 *      and each is rn(t * 255.0f) clamped to [0, 255]
 *   4. plane c takes channel 2 - c with bgr != 0 (BGR -> RGB), else channel c;  normalize != 0: dst = level / 255 rounded as
 *      img.float() / 255 rounds; else dst = level */
#define YMI_AUGMENT_MAX 32
#define YMI_AUGMENT_MAX_SRC 4
typedef struct ymi_augment_source {
    const uint8_t* src;
    int32_t h, w;
    int32_t x1a, y1a, x2a, y2a, x1b, y1b;
} ymi_augment_source;
typedef struct ymi_augment_image {
    ymi_augment_source s[YMI_AUGMENT_MAX_SRC];
    double A[6];
    const uint8_t* lut;
    int32_t n_src, canvas_h, canvas_w, flip_ud, flip_lr, _pad;
} ymi_augment_image;
int ymi_augment_batch(const ymi_augment_image* table, const ymi_augment_image* table_d, int64_t n, float* dst, int64_t size, int32_t border,
                      int32_t normalize, int32_t bgr, void* stream);
/* ymi_augment_boxes: the labels of the same batch, one launch, one workgroup (a batch has a few thousand rows at most).
 *   rows   : DEVICE float32 [n][7] = (image, source slot, cls, x, y, w, h), xywh normalised to the row's source image; image by image in
 *            ascending order (a row that lies outside its image's [row_start, row_end), or names no image or slot, is dropped)
 *   images : DEVICE array of `batch` ymi_augment_label_image
 *   out    : batch_idx [n], cls [n] and bboxes [n][4] float32 hold the kept rows compacted in their original order (elements at and beyond
 *            total are not written); keep [n] int32 is 1 for a kept row; count [batch] and total [1] int32.  The order is the rows': a
 *            prefix sum over keep, no atomically claimed slots.
 * Per row, in float32, every operation rounded on its own, in the reference's order (k: the row's slot):
 *   1. xywh2xyxy: x1 = x - w / 2, y1 = y - h / 2, x2 = x + w / 2, y2 = y + h / 2
 *   2. x *= src_w[k], y *= src_h[k] (denormalize); x *= ratio_w[k], y *= ratio_h[k] (LetterBox._update_labels; 1 in a mosaic);
 *      x += padw[k], y += padh[k] (Mosaic._update_labels :809-813 / LetterBox._update_labels :1629-1632)
 *   3. canvas > 0 (Mosaic._cat_labels :859-861): clip to [0, canvas]; a row with (x2 - x1) * (y2 - y1) <= 0 is dropped
 *   4. apply_bboxes (:1100-1112): the corners (x1,y1) (x2,y2) (x1,y2) (x2,y1) through X = M[0] * x + M[1] * y + M[2], Y = M[3] * x + M[4] * y
 *      + M[5], summed left to right (the reference's sum is a BLAS product whose order is not stated: agreement to a few ulp of the largest
 *      term, not bit for bit), then min / max; clip X to [0, size_w], Y to [0, size_h]
 *   5. box_candidates (:1297-1300) against the box of step 3 times `scale`: w1 = x2 * scale - x1 * scale, h1 likewise, w2, h2 of step 4;
 *      kept when w2 > 2 and h2 > 2 and w2 * h2 / (w1 * h1 + 1e-16f) > area_thr and max(w2 / (h2 + 1e-16f), h2 / (w2 + 1e-16f)) < 100
 *   6. xyxy2xywh: cx = (x1 + x2) / 2, cy = (y1 + y2) / 2, w2, h2; flip_ud: cy = size_h - cy; flip_lr: cx = size_w - cx
 *   7. Format (:2072-2074): cx / size_w, cy / size_h, w2 / size_w, h2 / size_h, IEEE float32 quotients */
typedef struct ymi_augment_label_image {
    float src_w[YMI_AUGMENT_MAX_SRC], src_h[YMI_AUGMENT_MAX_SRC], ratio_w[YMI_AUGMENT_MAX_SRC], ratio_h[YMI_AUGMENT_MAX_SRC];
    float padw[YMI_AUGMENT_MAX_SRC], padh[YMI_AUGMENT_MAX_SRC];
    float M[6];
    float scale, size_w, size_h, canvas;
    int32_t flip_ud, flip_lr, row_start, row_end;
} ymi_augment_label_image;
int ymi_augment_boxes(const float* rows, int64_t n, const ymi_augment_label_image* images, int64_t batch, float area_thr, float* batch_idx,
                      float* cls, float* bboxes, int32_t* keep, int32_t* count, int32_t* total, void* stream);

/* ------------------------------------------------------------------ validation statistics ---- */
/* What the validator does per image after NMS (models/yolo/detect/val.py:135-155, :174-216; utils/metrics.py box_iou and
 * ConfusionMatrix.process_batch :335-391; engine/validator.py match_predictions), csrc/valmatch.hip: ONE launch of `batch` workgroups, no
 * workspace, no allocation, no synchronisation; it only enqueues on `stream`.
 *   det, count : [batch][max_det][6] float32 rows (x1, y1, x2, y2, conf, cls) in ranked order and [batch] int32, as ymi_detect_nms /
 *                ymi_scale_boxes leave them; max_det <= 2048; rows at or beyond count[b] are ignored whatever they hold
 *   labels     : the batch's table of n_labels rows in the batch's own order: lab_img int32 (image of the row; rows of other values
 *                belong to nobody), lab_cls float32, lab_box [n_labels][4] float32 normalised (cx, cy, w, h).  An image's rows need not be
 *                contiguous; neither n_labels nor the rows per image are capped (the table is staged through LDS YMI_VALMATCH_CHUNK rows
 *                at a time).  "Table order" below is the order of an image's rows in this table.  n_labels may be 0.
 *   img_w, img_h : the network input's size;  native: DEVICE float32 [batch][5] = (gain, pad_x, pad_y, w0, h0), the table of
 *                ymi_scale_boxes, or NULL (labels stay in the network input's pixels)
 *   levels     : HOST array of n_levels <= YMI_VALMATCH_MAX_LEVELS float32 IoU levels; it travels in the kernel arguments
 *   single_cls : != 0: every detection and every label counts as class 0, in tp and in the matrix
 *   tp         : [batch][max_det][n_levels] uint8, every element written; zero at and beyond count[b]
 *   cm         : NULL (no matrix) or int32 [(nc + 1) * (nc + 1)], row = predicted class, column = labelled class, index nc = background;
 *                ADDED to with integer atomics (the caller zeroes it once per validation), so the result does not depend on any order
 * Every step is one rounded float32 operation, in this order (the host path's torch statements; no fused multiply-add):
 *   label box  : hw = w / 2, hh = h / 2; x1 = (cx - hw) * img_w, y1 = (cy - hh) * img_h, x2 = (cx + hw) * img_w, y2 = (cy + hh) * img_h;
 *                with native: v = (v - pad) / gain (pad_x for x, pad_y for y; the IEEE quotient, as in ymi_scale_boxes), then
 *                min(max(v, 0), w0) for x, min(max(v, 0), h0) for y
 *   iou        : box_iou(label, detection): iw = max(min(lx2, px2) - max(lx1, px1), 0), ih likewise, inter = iw * ih,
 *                area_l = (lx2 - lx1) * (ly2 - ly1), area_p likewise, iou = inter / (((area_l + area_p) - inter) + 1e-7f)
 *   tp         : overlap = iou * (1 if the class columns are equal as floats, else 0).  Detection d claims the label of largest overlap,
 *                the first maximum in table order (a detection that overlaps nothing claims the image's first row, as argmax does); s[d]
 *                is that overlap.  m[d] = the largest s[e] over e < d with the same claim (-inf if there is none).
 *                tp[d][t] = s[d] >= levels[t] and not (m[d] >= levels[t]).  An image without labels has tp = 0.
 *   cm         : only detections with conf > cm_conf take part; iou is taken regardless of class.  A detection claims the label of largest
 *                iou (first maximum in table order) if that iou > cm_iou (both thresholds compared in float32).  A claimed label goes to
 *                the claimant of largest iou.  Then: the holder of a label adds 1 to cm[det_cls][gt_cls]; every other participating
 *                detection - no claim, or its claim lost to a better one: it does not fall back to another label - adds 1 to
 *                cm[det_cls][nc]; every label nobody claims adds 1 to cm[nc][gt_cls] (an image without detections: all of its labels; an
 *                image without labels: all of its detections above cm_conf go to cm[det_cls][nc]).
 *                Equal ious: the reference leaves them to argsort; the library's own rule is the lower table row for a detection's claim,
 *                then the lower detection index for a label's holder.  Class ids are truncated to integers as .int() does; an update in
 *                which a class id lies outside [0, nc) is not counted (a label held by such a detection is not counted as missed either). */
#define YMI_VALMATCH_CHUNK 1024
#define YMI_VALMATCH_MAX_LEVELS 16
int ymi_val_match(const float* det, const int32_t* count, int64_t batch, int64_t max_det, const int32_t* lab_img, const float* lab_cls,
                  const float* lab_box, int64_t n_labels, float img_w, float img_h, const float* native, const float* levels, int32_t n_levels,
                  int32_t single_cls, uint8_t* tp, int32_t* cm, int64_t nc, float cm_conf, float cm_iou, void* stream);
/* The tp rule above with mask_iou in place of box_iou (models/yolo/segment/val.py:231-273 with overlap=True), the same kernel body: the overlap
 * of detection d with the image's j-th label in table order is, in float32, one rounding per operation,
 *   inter[b][d][j + 1] / (((area_gt[b][j + 1] + area_pred[b][d]) - inter[b][d][j + 1]) + 1e-7f)
 * on the counts ymi_mask_overlap leaves; labels with j + 1 >= n_bins overlap nothing.  Claims, ties, levels and single_cls as in ymi_val_match.
 * -> tp_m [batch][max_det][n_levels] uint8.  No confusion matrix: that stays box-based. */
int ymi_val_match_masks(const float* det, const int32_t* count, int64_t batch, int64_t max_det, const int32_t* lab_img, const float* lab_cls,
                        int64_t n_labels, const int32_t* inter, const int32_t* area_pred, const int32_t* area_gt, int64_t n_bins, const float* levels,
                        int32_t n_levels, int32_t single_cls, uint8_t* tp_m, void* stream);

/* ------------------------------------------------------------------------- optimizer step ---- */
/* The update either side of backward, reference engine/trainer.py:614-622 (optimizer_step: clip_grad_norm_(10.0),
 * SGD-nesterov step, EMA update), :788-849 (three parameter groups) and utils/torch_utils.py:657-673 (ModelEMA.update),
 * as multi-tensor launches over a DEVICE table of every tensor (built once: parameters, momentum and EMA buffers do not
 * move).  Gradient tensors move from step to step in eager mode, so their device addresses are passed as a HOST array
 * and travel in the kernel arguments (graph-capturable, no staging buffer).
 *   table      [n] ymi_opt_entry; group: 0 biases, 1 decayed weights, 2 norm weights (index into hyper's lr / wd);
 *              momentum / ema may be NULL (no momentum buffer: EMA-only entry; no ema: EMA not attached)
 *   chunk_map  [n_chunks][2] int32 (tensor index, chunk index): one workgroup per ymi_opt_chunk_elems() elements
 *   hyper      [20] float on the device: lr[3], weight_decay[3], momentum (Adam: beta1), max_norm (<= 0: no clipping), ema decay,
 *              ema tau, nesterov (0/1), gradient scale (1 / world size), beta2 (RMSprop: alpha), eps, rule (0 SGD-momentum - reference
 *              trainer.py:832-833; 1 AdamW, 2 Adam, 3 Adamax, 4 NAdam, 5 RAdam - trainer.py:829-830; 6 RMSprop - :831), 1 - beta2,
 *              1 - beta1 (differences taken in double on the host, as torch passes them), NAdam's momentum_decay, the float32 tails of beta1 and momentum_decay (NAdam)
 *   state      64 bytes on the device, zero before the first step: float clip, float total_norm, float ema_d, float 1-ema_d,
 *              int64 updates, int64 steps (Adam's t), float 1/(1-beta1^t), float sqrt(1-beta2^t), 4 floats of per-step scalars
 *              (NAdam's two weights and bias correction, RAdam's rectification), double mu_product (NAdam)
 * A launch covers tensors [first_tensor, first_tensor + n_tensors), n_tensors <= YMI_OPT_MAX_GRADS, whose chunks are the
 * n_chunks entries at chunk_map; host_grads[i] is the gradient of tensor first_tensor + i or NULL (no gradient this step). */
#define YMI_OPT_MAX_GRADS 448
typedef struct ymi_opt_entry {
    float* param;
    float* momentum; /* SGD / RMSprop: momentum buffer; Adam family: exp_avg */
    float* ema;
    int64_t numel;
    int32_t group;
    int32_t _pad;
    float* second;   /* Adam / AdamW / NAdam / RAdam: exp_avg_sq; Adamax: exp_inf; RMSprop: square_avg; NULL for SGD and EMA-only entries */
    float* acc;      /* the tensor's slice of the accumulation arena (ymi_opt_grad_accumulate); NULL until gradients are accumulated */
} ymi_opt_entry;
int64_t ymi_opt_chunk_elems(void);
/* partial sums of squares of (gradient * scale) into partials[partials_offset ..]; finalize != 0 (last launch of a step):
 * fixed-order sum of all partials_total partials -> state.total_norm, state.clip = min(1, max_norm / (norm + 1e-6)),
 * state.updates += 1, state.ema_d = decay * (1 - exp(-updates / tau)). */
int ymi_opt_grad_norm(const ymi_opt_entry* table, const int32_t* chunk_map, int32_t first_tensor, int32_t n_tensors, int64_t n_chunks,
                      const float* const* host_grads, const float* hyper, float* partials, int64_t partials_offset, int64_t partials_total,
                      void* state, int32_t finalize, void* stream);
/* rule 0: g = grad*scale*clip (+ wd*p); buf = momentum*buf + g; g = nesterov ? g + momentum*buf : buf; p -= lr*g;
 * rule 1 / 2 (torch.optim.AdamW / Adam): p *= 1 - lr*wd (Adam: g += wd*p); m = m + (g-m)(1-beta1); v = beta2 v + (1-beta2) g g;
 *   p -= lr/(1-beta1^t) * m / (sqrt(v)/sqrt(1-beta2^t) + eps);
 * rule 3 .. 6 (torch.optim.Adamax / NAdam / RAdam / RMSprop with momentum, torch's default hyper-parameters): the single-tensor
 *   update of each, weight decay added to the gradient;
 * then ema = d*ema + (1-d)*p.  `rule` must equal hyper[14] (it selects the compiled kernel; pass 2 reads hyper[14] for the bias corrections).  host_grads == NULL: EMA-only pass over the given tensors (buffers, frozen parameters). */
int ymi_opt_update(const ymi_opt_entry* table, const int32_t* chunk_map, int32_t first_tensor, int32_t n_tensors, int64_t n_chunks,
                   const float* const* host_grads, const float* hyper, const void* state, int32_t rule, void* stream);
/* gradient accumulation outside autograd (reference trainer.py:305,397): table[t].acc[i] += host_grads[t - first_tensor][i] in float32 for
 * every tensor of the launch, over the same table / chunk_map ranges as ymi_opt_grad_norm.  A tensor whose gradient pointer or acc is NULL
 * is skipped (its acc stays as it is).  One read of g and acc, one write of acc per element, 16-byte accesses where both addresses allow;
 * no atomics: sums form in call order, (g1 + g2) + g3, as AccumulateGrad forms them.  Only numel and acc of an entry are read. */
int ymi_opt_grad_accumulate(const ymi_opt_entry* table, const int32_t* chunk_map, int32_t first_tensor, int32_t n_tensors, int64_t n_chunks,
                            const float* const* host_grads, void* stream);

/* SwinBlock MLP: Linear(C,4C) -> exact GELU -> Linear(4C,C) (+ skip).  Reference: ultralytics/nn/modules/swin_block.py:33 (definition)
 * and :53 (`x = x + self.mlp(self.norm2(x))`).  Token matrices are ymi_tensors with n = h = 1, w = tokens.
 * fwd: pre = u W1^T + b1 and post = gelu(pre) are both written by fc1's epilogue; out = post W2^T + b2 (+ residual).
 * bwd_data: dpre = (dout W2) * gelu'(pre) from fc2's data-gradient epilogue; du = dpre W1 (+ add1 + add2); du may be NULL.
 * Weights are the ymi_pack_conv_weight_fwd / _dgrad images of the two nn.Linear weights viewed as 1x1 convolutions. */
int ymi_swin_mlp_fwd(const ymi_tensor* u, const void* w1_packed, const float* b1, int64_t hidden, const void* w2_packed, const float* b2,
                     const ymi_tensor* residual, const ymi_tensor* pre, const ymi_tensor* post, const ymi_tensor* out, void* stream);
int ymi_swin_mlp_bwd_data(const ymi_tensor* dout, const void* w2_dgrad_packed, const ymi_tensor* pre, const ymi_tensor* dpre,
                          const void* w1_dgrad_packed, const ymi_tensor* add1, const ymi_tensor* add2, const ymi_tensor* du, void* stream);

/* SwinBlock's second half as one kernel per direction: out = x + fc2(gelu(fc1(LayerNorm(x)))) - swin_block.py:53 with the modules of
 * swin_block.py:30-35 (norm2, mlp) - for bfloat16 tokens of 128, 256 or 384 channels, the SwinBlock widths of the model files (csrc/swin_mlp.hip;
 * `supported` says whether a shape takes this path, anything else keeps ymi_layernorm_fwd + ymi_swin_mlp_fwd).  The [T, hidden] activations
 * never reach HBM in the forward except, when training, the bf16 pre-activations once, in a private register-order layout of
 * ymi_swin_ln_mlp_pre_elems(T, hidden) elements.
 *   supported: dtype bfloat16, c in {128, 256, 384}, hidden a multiple of 32 that leaves the fc1 bias room in LDS beside the weight ring:
 *             hidden <= 8192 at c = 128 and 256, <= 4096 at c = 384
 *   pack    : w1 [hidden][c], w2 [c][hidden] (float32, nn.Linear layouts) -> `packed`, ymi_swin_ln_mlp_pack_elems = 4 c hidden bfloat16 elements:
 *             four images of c * hidden elements (fc1, fc2, fc2 transposed, fc1 transposed), each [hidden/32 chunks][32 c elements] with a chunk
 *             laid out as the MFMA A fragments the kernels read - rows form [c/16 k-steps][64 lanes][8] (images 0, 2), cols form
 *             [c/32 tiles][2 steps][64 lanes][8] (images 1, 3); a chunk image is 8 / 16 / 24 KB at c = 128 / 256 / 384
 *   pre     : private, [tile][hidden/32 chunks][wave][2][64 lanes][8] bfloat16 with tiles of 256 tokens and 8 waves at c = 128 and 256, of 128
 *             tokens and 4 waves at c = 384 (a wave = 32 tokens); pre_elems pads the token count to a multiple of 256, which both tiles divide
 *   fwd     : u / mean / rstd / pre non-null = training (u: LayerNorm output [T][c], saved for fc1's weight gradient and LayerNorm's backward)
 *   bwd_data: post = gelu(pre) and dpre = (dout W2) * gelu'(pre), both [T][hidden] row-major for the two weight-gradient GEMMs
 *             (ymi_conv2d_bwd_weight on (post, dout) and (u, dpre)); du = dpre W1 [T][c], LayerNorm's incoming gradient.  The kernel stores whole
 *             token tiles (256 or 128 rows, as above): post / dpre are dense (ld == hidden) views of the first T rows of buffers of ymi_swin_ln_mlp_pre_elems elements. */
int ymi_swin_ln_mlp_supported(int64_t c, int64_t hidden, int32_t dtype);
int64_t ymi_swin_ln_mlp_pack_elems(int64_t c, int64_t hidden);
int64_t ymi_swin_ln_mlp_pre_elems(int64_t tokens, int64_t hidden);
int ymi_swin_ln_mlp_pack(const float* w1, const float* w2, int64_t c, int64_t hidden, void* packed, void* stream);
int ymi_swin_ln_mlp_fwd(const ymi_tensor* x, const float* gamma, const float* beta, float eps, const void* packed, const float* b1, const float* b2,
                        int64_t hidden, const ymi_tensor* u, float* mean, float* rstd, void* pre, const ymi_tensor* out, void* stream);
int ymi_swin_ln_mlp_bwd_data(const ymi_tensor* dout, const void* packed, const void* pre, int64_t hidden, const ymi_tensor* post, const ymi_tensor* dpre,
                             const ymi_tensor* du, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* YMI_H */
