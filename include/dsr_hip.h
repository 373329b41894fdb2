/* dsr_hip.h -- C ABI of libdsr_hip.so, the MI355X (gfx950) kernel library behind the
 * nn.Module surface of LewisClifton/Deep-Super-Resolution.
 *
 * The reference has no FFI of its own: every device op is reached through
 * torch.nn modules.  This ABI is what those modules' forward/backward bind to in this build
 * (deep-super-resolution_amd/_lib.py, ctypes).  Conventions:
 *   - plain C: raw DEVICE pointers borrowed for the duration of the call, sizes as ints; no torch
 *     types.  The caller allocates every output and workspace.
 *   - every function only ENQUEUES work on `stream` and never synchronises, allocates or copies
 *     from the host: all of them are HIP-graph capturable.
 *   - return 0 on success, a negative code otherwise; dsr_last_error() gives the message.  The
 *     Python side turns that into RuntimeError (the reference raises on bad configs:
 *     utils/downsampler.py:12,38; models/DIP/utils.py:74,92).
 *   - activation tensors: NHWC, 16-bit (dtype 0 = bf16, 1 = f16), channel count padded up to a
 *     multiple of 8 ("Cp"); parameters, statistics, gradients of parameters: fp32 in the
 *     reference's own layouts (OIHW conv weights etc.).
 * Each entry cites the reference code whose device work it replaces.
 */
#ifndef DSR_HIP_H
#define DSR_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* dsr_stream_t; /* == hipStream_t */

#define DSR_BF16 0
#define DSR_F16 1

enum { DSR_OK = 0, DSR_E_ARG = -1, DSR_E_LAUNCH = -2, DSR_E_WORKSPACE = -3, DSR_E_UNSUPPORTED = -4 };

const char* dsr_last_error(void);
int dsr_abi_version(void);

/* ------------------------------------------------------------------ convolution
 * One descriptor for nn.Conv2d as the reference uses it:
 *   generator.py:7,11,52 (3x3 s1 p1), :30 (64->256), :47,62 (9x9 p4); discriminator.py:7,25 (3x3 s1|s2 p1);
 *   models/DIP/utils.py:83-105 (ReflectionPad2d + Conv2d k in {1,3}, stride 1|2, padding 0);
 *   utils/GAN.py:69-72 (VGG19 3x3 p1).
 * pad_mode: 0 zero, 1 reflect (the DIP padder folded into the tile loader), 2 replicate. */
typedef struct dsr_conv_desc {
  int dtype;
  int N, H, W;      /* input spatial size */
  int Cin, Cout;    /* real channel counts; tensors hold round_up(C, 8) channels */
  int KH, KW, stride, pad, pad_mode;
} dsr_conv_desc;

/* fused epilogue of the forward conv */
typedef struct dsr_epilogue {
  int act;                 /* 0 none, 1 leaky(slope), 2 prelu(*prelu), 3 relu, 4 tanh, 5 sigmoid, 6 elu(alpha=1) */
  float slope;
  const float* prelu;      /* 1-element device tensor (nn.PReLU(), generator.py:9,34,48) or NULL */
  const float* bias;       /* [Cout] or NULL */
  float* stats_partial;    /* [dsr_conv_stats_rows()][2][round_up(Cout,8)] sum / sum-of-squares rows for
                              a following train-mode BatchNorm (pre-activation values), or NULL */
  int pixel_shuffle;       /* 1: store through nn.PixelShuffle(2) (generator.py:32,38):
                              y is [N][2*OH][2*OW][round_up(Cout/4, 8)] */
  float* out_nchw_f32;     /* non-NULL: write fp32 NCHW [N][Cout][OH][OW] here instead of y (last layers) */
  /* inference-time folding of an eval-mode BatchNorm2d and a skip connection (generator.py:14-25 under gan_G.eval()):
   * y = act((conv + bias) * bn_scale[c] + bn_shift[c]) + residual.  All NULL for the plain epilogue.  Only layers for
   * which dsr_conv_fwd_affine_supported() is non-zero accept them; others return DSR_E_UNSUPPORTED. */
  const float* bn_scale;   /* [round_up(Cout,8)] */
  const float* bn_shift;   /* [round_up(Cout,8)] */
  const void* residual;    /* same layout as y */
} dsr_epilogue;

int dsr_conv_fwd_affine_supported(const dsr_conv_desc* d);

int dsr_conv_out_size(const dsr_conv_desc* d, int* OH, int* OW);
/* rows of the BatchNorm statistics partial buffer written by dsr_conv_fwd */
int dsr_conv_stats_rows(const dsr_conv_desc* d);
/* element counts (16-bit) of the two packed weight images */
size_t dsr_conv_packed_elems(const dsr_conv_desc* d, int dgrad);
/* w [Cout][Cin][KH][KW] fp32 -> w_fwd [KH*KW][round_up(Cout,8)][round_up(Cin,8)],
 *                               w_dgrad [KH*KW][round_up(Cin,8)][round_up(Cout,8)] (may be NULL) */
int dsr_conv_pack_weight(const dsr_conv_desc* d, const float* w, void* w_fwd, void* w_dgrad, dsr_stream_t s);
/* the same packing for `count` weights in one launch per 48 (HOST arrays of device pointers and of Cout / Cin / KH*KW,
 * read before the call returns): an optimiser refreshes the images of everything it just updated */
int dsr_conv_pack_weight_multi(int dtype, int count, const float* const* w, void* const* w_fwd, void* const* w_dgrad,
                               const int* cout, const int* cin, const int* taps, dsr_stream_t s);
/* y = epilogue(conv(x, w) ) */
int dsr_conv_fwd(const dsr_conv_desc* d, const void* x, const void* w_fwd, const dsr_epilogue* e, void* y,
                 dsr_stream_t s);
/* dx = conv_transpose(dy, w) : autograd of nn.Conv2d w.r.t. its input.
 * workspace: dsr_conv_dgrad_workspace(d) bytes (non-zero only for reflect padding: the fp32 gradient of the padded input,
 * folded onto dx with one rounding). */
size_t dsr_conv_dgrad_workspace(const dsr_conv_desc* d);
int dsr_conv_dgrad(const dsr_conv_desc* d, const void* dy, const void* w_dgrad, void* dx, void* workspace,
                   size_t ws_bytes, dsr_stream_t s);
/* dw [Cout][Cin][KH][KW] fp32 (overwritten) = autograd of nn.Conv2d w.r.t. its weight */
size_t dsr_conv_wgrad_workspace(const dsr_conv_desc* d);
int dsr_conv_wgrad(const dsr_conv_desc* d, const void* x, const void* dy, float* dw, void* workspace, size_t ws_bytes,
                   dsr_stream_t s);

/* Fused backward of a first layer whose input needs no gradient -- Conv2d(<=3 -> 64, 3x3, s1, p1) + LeakyReLU | ReLU |
 * nothing (discriminator.py:22,25-27): dw (OIHW fp32) and db (nullable) from x, the gradient dout w.r.t. the activation
 * output and that output y, in one pass (g = dout * act'(y) is never written).  _supported() says whether a descriptor
 * qualifies; callers otherwise use dsr_pw_act_bwd + dsr_conv_wgrad. */
int dsr_conv_first_bwd_supported(const dsr_conv_desc* d, int act);
size_t dsr_conv_first_bwd_workspace(const dsr_conv_desc* d);
int dsr_conv_first_bwd(const dsr_conv_desc* d, const void* x, const void* dout, const void* y, int act, float slope,
                       float* dw, float* db, void* workspace, size_t ws_bytes, dsr_stream_t s);
/* The same without y: the sign of the pre-activation is recomputed from x and the layer's own fp32 weights w (OIHW) and
 * bias (nullable) -- the 1.07 GB activation of discriminator.py:25 at 512x512, batch 32, is not read by this pass. */
int dsr_conv_first_bwd_recompute(const dsr_conv_desc* d, const void* x, const void* dout, const float* w, const float* bias,
                                 int act, float slope, float* dw, float* db, void* workspace, size_t ws_bytes, dsr_stream_t s);

/* dsr_conv_dgrad of the 9x9 64 -> 3 tail (generator.py:78) whose input is PReLU(PixelShuffle(2)(conv)) (generator.py:37-39), with
 * that activation's whole backward in the same launch: the gradient w.r.t. the tail's input is never written; what comes out is
 * dyu [N][H/2][W/2][256], the gradient of the shuffle conv's output (channel 4c + 2i + j <- pixel (2h+i, 2w+j), masked by the
 * PReLU derivative taken from the sign of act_out = the tail's own input), and dsr_conv_dgrad_ps_rows(d) partial rows of [2][256]:
 * the column sums of dyu (that conv's bias gradient) and the PReLU-weight gradient terms (column 0 of the second slice) --
 * exactly what dsr_pw_act_bwd(pixshuf = 1) produces from dx and act_out.  prelu: the (positive) PReLU weight on the device. */
int dsr_conv_dgrad_ps_supported(const dsr_conv_desc* d);
int dsr_conv_dgrad_ps_rows(const dsr_conv_desc* d);
int dsr_conv_dgrad_ps(const dsr_conv_desc* d, const void* dy, const void* w_dgrad, const void* act_out, const float* prelu,
                      void* dyu, float* partial, dsr_stream_t s);

/* dsr_conv_dgrad of a 3x3 stride-2 layer (discriminator.py:31,33,35) whose input is the output of BatchNorm + LeakyReLU
 * (:14-19), with the two per-channel sums the BatchNorm backward of that layer needs formed in the same launch: partial gets
 * dsr_conv_dgrad_bn_rows(d) rows of [3][r8(Cin)] = (sum g, sum g*y, 0) with g = dx * act'(scale*y + shift) -- what
 * dsr_pw_bn_act_bwd_reduce would write after reading dx and y (bn_y: that layer's raw conv output, same shape as dx) once more;
 * feed them to dsr_pw_bn_bwd_finalize.  act: LeakyReLU or none.  _supported(): H, W even, tiles of 256 gradient pixels that
 * are whole rows of one image, one 64-channel slice per block. */
int dsr_conv_dgrad_bn_supported(const dsr_conv_desc* d);
int dsr_conv_dgrad_bn_rows(const dsr_conv_desc* d);
int dsr_conv_dgrad_bn(const dsr_conv_desc* d, const void* dy, const void* w_dgrad, void* dx, const void* bn_y,
                      const float* bn_scale, const float* bn_shift, int act, float slope, float* partial, dsr_stream_t s);

/* The backward counterpart of dsr_conv_first2_fwd for a step that needs no image gradient (the discriminator's own update,
 * train_GAN.py:47-56): the input gradient of the stride-2 layer d1 (discriminator.py:29) and the whole backward of the image
 * layer d0 under it (:25-27: activation mask, bias gradient, weight gradient) in ONE launch.  The gradient of the 64-channel
 * activation between them (1.07 GB at 512x512, batch 32) is formed per tile in LDS and never written.  dy: gradient of d1's
 * conv output [N][H/2][W/2][64]; w1_dgrad: d1's packed input-gradient weights (dsr_conv_pack_weight); img: NHWC 16-bit image
 * with 8 channels; w0 (OIHW fp32) / b0 (nullable): d0's parameters as the forward used them; dw0 (OIHW fp32), db0 (nullable).
 * _supported(): 64 -> 64 channels, even H and W with (W/2) % 256 == 0, d0 as dsr_conv_first_bwd_supported. */
int dsr_conv_dgrad_first_bwd_supported(const dsr_conv_desc* d0, const dsr_conv_desc* d1, int act0);
size_t dsr_conv_dgrad_first_bwd_workspace(const dsr_conv_desc* d1);
int dsr_conv_dgrad_first_bwd(const dsr_conv_desc* d0, const dsr_conv_desc* d1, const void* dy, const void* w1_dgrad,
                             const void* img, const float* w0, const float* b0, int act0, float slope0, float* dw0, float* db0,
                             void* workspace, size_t ws_bytes, dsr_stream_t s);

/* The discriminator's first two convolutions (discriminator.py:25 Conv2d(3,64,3,1,1) + LeakyReLU; :29 Conv2d(64,64,3,2,1) in
 * front of its BatchNorm) as ONE forward launch: the first layer's 64-channel activation (1.07 GB at 512x512, batch 32) is
 * recomputed per tile in LDS and goes to HBM only if `a0` is given (training: the second layer's weight gradient reads it).
 * d0 / d1: the two layers' descriptors (same N, H, W); x: NHWC 16-bit image with 8 channels; w0 / w1: packed forward images;
 * y1: raw second-layer output [N][OH][OW][64]; stats (nullable): dsr_conv_first2_stats_rows(d0) rows of [2][64] partial sums. */
int dsr_conv_first2_supported(const dsr_conv_desc* d0, const dsr_conv_desc* d1);
int dsr_conv_first2_stats_rows(const dsr_conv_desc* d0);
int dsr_conv_first2_fwd(const dsr_conv_desc* d0, const dsr_conv_desc* d1, const void* x, const void* w0, const float* bias0,
                        float slope0, const void* w1, const float* bias1, void* a0, void* y1, float* stats, dsr_stream_t s);

/* Which kernel the dispatcher launches for this descriptor (measurement aid: bench.py labels its HIP-event timings
 * with it so they can be matched against rocprofv3's kernel names).  op: 0 forward, 1 dgrad, 2 wgrad.  `e` may be
 * NULL (no statistics, no pixel shuffle, NHWC output).  Returns a static string; never NULL. */
/* dx = dgrad(dy) * act'(x_act) in one launch: x_act = this conv's own input = the OUTPUT of the activation in front of it
 * (ReLU, or LeakyReLU with slope > 0); replaces the producing layer's separate activation-backward pass (the VGG19 trunk of
 * utils/GAN.py:19-57 is a chain of conv + ReLU pairs).  Bit-identical to dsr_conv_dgrad followed by dsr_pw_act_bwd. */
int dsr_conv_dgrad_masked_supported(const dsr_conv_desc* d);
int dsr_conv_dgrad_masked(const dsr_conv_desc* d, const void* dy, const void* w_dgrad, const void* x_act, int act, float slope,
                          void* dx, dsr_stream_t s);
/* dx = dgrad(dy) + addend in one launch (the gradient of a residual block's input: conv path + skip path,
 * generator.py:24); dsr_conv_dgrad_add_supported tells whether the shape is taken (64 -> 64 3x3 stride 1 zero pad). */
int dsr_conv_dgrad_add_supported(const dsr_conv_desc* d);
int dsr_conv_dgrad_add(const dsr_conv_desc* d, const void* dy, const void* w_dgrad, const void* addend, void* dx,
                       dsr_stream_t s);
/* Every 3x3 / stride-1 / pad-1 weight gradient of a backward pass in one contraction launch + one reduction launch
 * (replaces the per-layer weight-gradient kernels of loss.backward(), train_GAN.py:52,63).  Entries whose dws[i] are equal
 * must be adjacent and are summed into that one gradient (a weight applied to two batches).  All entries share one dtype.
 * dsr_conv_wgrad_batchable: 1 if the shape is taken; the workspace size depends on the whole table. */
int dsr_conv_wgrad_batchable(const dsr_conv_desc* d);
size_t dsr_conv_wgrad_batched_workspace(int count, const dsr_conv_desc* descs, float* const* dws);
int dsr_conv_wgrad_batched(int count, const dsr_conv_desc* descs, const void* const* xs, const void* const* dys,
                           float* const* dws, void* workspace, size_t ws_bytes, dsr_stream_t s);
const char* dsr_conv_kernel_name(const dsr_conv_desc* d, int op, const dsr_epilogue* e);

/* ------------------------------------------------------------------ pointwise / reductions (pointwise.hip)
 * nn.BatchNorm2d / PReLU / LeakyReLU / Tanh / Sigmoid / residual add / PixelShuffle backward / losses / Adam.
 * See the kernel comments in csrc/pointwise.hip for the reference lines each covers. */
int dsr_pw_nchw_to_nhwc(int dtype, const float* src, void* dst, int N, int C, int H, int W, int Cp, dsr_stream_t s);
int dsr_pw_nhwc_to_nchw(int dtype, const void* src, float* dst, int N, int C, int H, int W, int Cp, dsr_stream_t s);
int dsr_pw_pack_weight(int dtype, const float* w, void* wf, void* wd, int Cout, int Cin, int T, int NBo, int CinP,
                       int NBi, int CoutP, dsr_stream_t s);
/* Two-stage deterministic reductions: kernels write one partial ROW per block; the finalize entry points first
 * compact many rows in parallel into <= dsr_pw_scratch_rows() rows stored right behind the partial buffer, so EVERY
 * partial buffer handed to dsr_pw_bn_finalize / dsr_pw_bn_bwd_finalize / dsr_pw_sum_rows(compact=1) must have room
 * for `rows + dsr_pw_scratch_rows()` rows. */
int dsr_pw_scratch_rows(void);
/* out[c] (+)= scale * sum_r partial[r*row_stride + col_offset + c], c < C */
int dsr_pw_sum_rows(const float* partial, int rows, int row_stride, int col_offset, int C, float scale, float* out,
                    int accumulate, int compact, dsr_stream_t s);
int dsr_pw_bn_finalize(const float* partial, int tiles, int stride, int C, int Cp, float count, const float* gamma,
                       const float* beta, float* running_mean, float* running_var, long long* num_batches_tracked,
                       float momentum, float eps, int updates, float* scale, float* shift, float* mean, float* rstd,
                       dsr_stream_t s);
int dsr_pw_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                          float eps, int C, int Cp, float* scale, float* shift, float* mean, float* rstd,
                          dsr_stream_t s);
/* grid sizing shared by the two-stage reductions: returns #blocks, writes rows per block */
int dsr_pw_reduce_blocks(size_t P, int* rows_per_block);
int dsr_pw_channel_stats(int dtype, const void* x, size_t P, int Cp, int blocks, int rpb, float* partial,
                         dsr_stream_t s);
int dsr_pw_bn_act_fwd(int dtype, const void* y, const float* scale, const float* shift, const void* residual, void* out,
                      size_t P, int Cp, int act, float slope, const float* prelu, dsr_stream_t s);
int dsr_pw_bn_act_bwd_reduce(int dtype, const void* dout, const void* y, const float* scale, const float* shift,
                             const float* mean, const float* rstd, size_t P, int Cp, int blocks, int rpb, int act,
                             float slope, const float* prelu, float* partial, dsr_stream_t s);
int dsr_pw_bn_bwd_finalize(const float* partial, int blocks, int C, int Cp, float count, const float* mean,
                           const float* rstd, float* dgamma, float* dbeta, float* dprelu, float* c1, float* c2,
                           dsr_stream_t s);
int dsr_pw_bn_act_bwd_apply(int dtype, const void* dout, const void* y, const float* scale, const float* shift,
                            const float* mean, const float* rstd, const float* c1, const float* c2, void* dy, size_t P,
                            int Cp, int act, float slope, const float* prelu, int train, dsr_stream_t s);
int dsr_pw_act_bwd(int dtype, const void* dout, const void* out, void* dy, int N, int H, int W, int CyP, int CoP,
                   int pixshuf, int act, float slope, const float* prelu, int blocks, int rpb, float* partial,
                   dsr_stream_t s);
int dsr_pw_act_bwd_nchw(int dtype, const float* dout, const float* out, void* dy, int N, int C, int H, int W, int Cp,
                        int act, dsr_stream_t s);
int dsr_pw_colsum(int dtype, const void* x, size_t P, int Cp, int blocks, int rpb, float* partial, dsr_stream_t s);
int dsr_pw_add(int dtype, const void* a, const void* b, void* out, size_t nvec, dsr_stream_t s);
/* out[i] = (a * x[i] + b * y[i]) * g[0] over n fp32 elements; y nullable (-> 0), g nullable device scalar (-> 1).
 * The scalar arithmetic of the step recipes (utils/GAN.py:105,122 loss sums; loss-gradient scaling). */
int dsr_pw_axpby_f32(const float* x, const float* y, float a, float b, const float* g, float* out, size_t n,
                     dsr_stream_t s);
int dsr_pw_diff_loss(const float* pred, const float* tgt, float* grad, size_t n, int mode, float* partial, int blocks,
                     dsr_stream_t s);
int dsr_pw_bce_const(const float* p, int n, float target, float* loss, float* grad, int accumulate, dsr_stream_t s);
/* ---- Adam (torch.optim.Adam defaults, no weight decay): ONE argument block for the three launch shapes -- one tensor
 * (dsr_pw_adam), up to 64 small tensors per launch (dsr_pw_adam_multi) and the dense head's weight gradient + Adam in one
 * pass (dsr_linear_wgrad_adam, below).  The block says where the coefficients come from; the three device pointers are
 * independently nullable:
 *   all three NULL       lr and grad_scale from the host (1/S when a static loss scale S is in use).
 *   loss_scale           the gradient multiplier is 1 / loss_scale[0] (optim.DynamicLossScaler: exact, the scale is a power of
 *                        two) and grad_scale is NOT read.
 *   found_inf            found_inf[0] != 0: the launch writes nothing -- not p, m, v nor the shadow.
 *   hyper                lr = hyper[0], and the multiplier chosen above is multiplied ONCE by hyper[1], the clipping coefficient
 *                        (dsr_clip_finalize writes both): hyper[1] == 1 gives the bits of the same call without hyper.
 * With all three NULL the kernels that run hold no trace of the pointers; any other combination is resolved on the device.
 * Every entry point checks the same things before its first launch (DSR_E_ARG): args and args->step non-NULL and 4-byte
 * aligned, hyper / loss_scale / found_inf 4-byte aligned when set, every tensor non-NULL, aligned and of n > 0 elements,
 * count > 0.  Tensor alignment follows the accesses of each launch: dsr_pw_adam moves p, g, m and v as 16-byte vectors and
 * the shadow as 8-byte ones, so it wants them 16- and 8-byte aligned (as dsr_linear_wgrad_adam does) and refuses a view 4,
 * 8 or 12 bytes off such a boundary; dsr_pw_adam_multi's accesses are scalar and its tensors need 4 bytes only, which is
 * where optim.FusedAdam sends such a view.  An empty tensor is refused in every mode, on purpose: one rule instead of one per mode.
 * optim.FusedAdam leaves zero-element parameters out of its tables, so such a parameter is a no-op in every mode. */
typedef struct dsr_adam_args {
  const int*   step;        /* device step counter, already advanced for this step; required            */
  float        lr, b1, b2, eps;
  float        grad_scale;  /* host multiplier of g; unused when loss_scale != NULL                      */
  const float* hyper;       /* nullable: device {lr, clip coefficient}: lr = hyper[0], multiplier *= hyper[1] */
  const float* loss_scale;  /* nullable: multiplier = 1 / loss_scale[0]                                  */
  const float* found_inf;   /* nullable: found_inf[0] != 0 -> the launch writes nothing                  */
} dsr_adam_args;
/* shadow_bf16 (nullable): also write the bf16 image of the updated parameter (same layout) */
int dsr_pw_adam(float* p, const float* g, float* m, float* v, size_t n, void* shadow_bf16, const dsr_adam_args* args,
                dsr_stream_t s);
/* the same update for `count` tensors in as few launches as possible (64 tensors per launch); the four pointer
 * arrays and n[] are HOST arrays of device pointers / element counts, read before the call returns */
int dsr_pw_adam_multi(int count, float* const* p, const float* const* g, float* const* m, float* const* v,
                      const size_t* n, const dsr_adam_args* args, dsr_stream_t s);
/* step[0] += 1, unless found_inf (nullable) is set: the step counter of a step the loss scaler skips stays */
int dsr_pw_incr(int* step, const float* found_inf, dsr_stream_t s);

/* ------------------------------------------------------------------ dynamic loss scale (optim.DynamicLossScaler)
 * What torch.amp.GradScaler is to torch.optim, with nothing read on the host: the state is three device words, scale
 * (fp32, always a power of two, so that un-scaling is exact), growth_tracker (int32) and found_inf (fp32, 0 or 1), and the
 * skipped step is decided inside the kernels.  Order within a step: dsr_amp_check, dsr_pw_incr with found_inf, the Adam
 * launches with loss_scale and found_inf in their dsr_adam_args, dsr_amp_update.
 * dsr_amp_check: found_inf[0] = 1 if any element of the `count` fp32 tensors is Inf or NaN (HOST tables of device pointers
 * and element counts, read before the call returns; a NULL entry is a parameter without a gradient and is skipped; 64 tensors
 * per launch).  Never writes 0: dsr_amp_update clears the flag.
 * dsr_amp_update: torch's _amp_update_scale_ -- found_inf: scale *= backoff_factor, tracker = 0; otherwise tracker += 1 and,
 * when it reaches growth_interval, scale *= growth_factor (unless that is not finite) and tracker = 0 -- then found_inf = 0.
 * growth_factor = 2^k, backoff_factor = 2^-k, k >= 1; growth_interval >= 1.  stats (nullable): int32[2], steps taken and
 * steps skipped, incremented here. */
int dsr_amp_check(int count, const float* const* grads, const size_t* numel, float* found_inf, dsr_stream_t s);
int dsr_amp_update(float* scale, int* growth_tracker, float* found_inf, float growth_factor, float backoff_factor,
                   int growth_interval, int* stats, dsr_stream_t s);

/* ------------------------------------------------------------------ gradient-norm clipping and a device-resident learning rate
 * (optim.FusedAdam(lr=<tensor>, max_grad_norm=c)).  torch.nn.utils.clip_grad_norm_(params, c, norm_type=2) followed by
 * torch.optim.Adam, with nothing read on the host and no gradient rewritten: the coefficient is applied inside the Adam
 * kernels.  Order within a step: (dsr_amp_check,) dsr_pw_incr, dsr_clip_sumsq and / or dsr_linear_factor_gram,
 * dsr_clip_finalize, the Adam launches with dsr_adam_args.hyper set.
 * dsr_clip_sumsq: one fp32 partial sum of squares per block over `count` fp32 tensors (HOST tables as dsr_amp_check takes
 * them: a NULL entry is skipped, 64 tensors per launch, views 4 / 8 / 12 bytes off a 16-byte boundary are fine), written
 * with plain stores at partials[0 .. dsr_clip_sumsq_partials()): no atomics, bit-reproducible.
 * dsr_clip_finalize: sums partials (fp32) and gram_partials (fp64) in fp64 in a fixed order; norm = sqrt(sum) * |grad_scale|,
 * or sqrt(sum) / scale[0] when scale (the dynamic loss scaler's word) is non-NULL; coef = min(1, max_norm / (norm + 1e-6)),
 * torch's formula (max_norm <= 0: coef = 1, no clipping); writes grad_norm[0], clip_coef[0] (both nullable) and the hyper
 * block hyper[0] = lr (lr_dev[0] when lr_dev is non-NULL, else lr_host), hyper[1] = coef.  Either count may be 0. */
size_t dsr_clip_sumsq_partials(int count, const float* const* grads, const size_t* numel);
int dsr_clip_sumsq(int count, const float* const* grads, const size_t* numel, float* partials, size_t n_partials,
                   dsr_stream_t s);
int dsr_clip_finalize(const float* partials, int n_partials, const double* gram_partials, int n_gram, float grad_scale,
                      const float* scale, float max_norm, const float* lr_dev, float lr_host, float* grad_norm,
                      float* clip_coef, float* hyper, dsr_stream_t s);

/* ------------------------------------------------------------------ discriminator dense head (linear.hip)
 * models/GAN/discriminator.py:37-45,65-72: flatten(C,H,W) -> Linear(K,O) -> LeakyReLU(0.2) -> Linear(O,1) -> Sigmoid */
/* 16-bit shadow copy of an fp32 tensor (n % 8 == 0; src and dst 16-byte aligned: the kernel moves 16-byte vectors, a
 * misaligned pointer is DSR_E_ARG) */
int dsr_cast16(int dtype, const float* src, void* dst, size_t n, dsr_stream_t s);
/* mode 0: flat[b][c*HW+p] = act[b][p][c];  1: flatT[c*HW+p][b] (Bp columns, zero padded);  2: act <- flat */
int dsr_flatten(int dtype, const void* src, void* dst, int B, int HW, int C, int Cp, int Bp, int mode, dsr_stream_t s);
size_t dsr_linear_fwd_workspace(int B, size_t K, int O);
/* out[b][o] (fp32) = act(sum_k x[b][k] w16[o][k] + bias[o]) */
int dsr_linear_fwd(int dtype, const void* x, const void* w16, const float* bias, int act, float slope, float* out,
                   int B, size_t K, int O, void* workspace, size_t ws_bytes, dsr_stream_t s);
/* dx[b][k] (16-bit) = sum_o dy16[b][o] w16[o][k] */
int dsr_linear_dgrad(int dtype, const void* dy16, const void* w16, void* dx, int B, int O, size_t K, dsr_stream_t s);
/* dw[o][k] (fp32, overwritten) = sum_b dyT16[o][b] xT16[k][b];  Bp in {32, 64} */
int dsr_linear_wgrad(int dtype, const void* dyT16, const void* xT16, float* dw, int Bp, int O, size_t K,
                     dsr_stream_t s);
/* data-parallel form: dw = scale * sum over R gathered rank-local factor pairs, dyT16_all [R][O][Bp], xT16_all [R][K][Bp]
 * (all-gather the 67 MB + 128 KB factors instead of all-reducing the 2.1 GB gradient) */
int dsr_linear_wgrad_gathered(int dtype, const void* dyT16_all, const void* xT16_all, float* dw, int Bp, int O, size_t K,
                              int R, float scale, dsr_stream_t s);
/* the same contraction with torch.optim.Adam's update applied to p / m / v (and p's bf16 shadow) in the epilogue: the
 * gradient is never written (R = 1, scale = 1: bit-identical to dsr_linear_wgrad followed by dsr_pw_adam); K % 64 == 0.
 * p / m / v and the two factor tables are accessed 16 bytes at a time and the shadow 8: they must be aligned to that
 * (the words of dsr_adam_args to 4); a misaligned pointer is DSR_E_ARG.  args: as for dsr_pw_adam, every mode.
 * Replaces loss.backward() writing dense1.weight.grad + optimizer.step() reading it (train_GAN.py:52-53 on
 * discriminator.py:54). */
int dsr_linear_wgrad_adam(int dtype, const void* dyT16_all, const void* xT16_all, int Bp, int O, size_t K, int R, float scale,
                          float* p, float* m, float* v, void* shadow_bf16, const dsr_adam_args* args, dsr_stream_t s);
/* squared Frobenius norm of the factored gradient dW = scale * sum_{(r,b)} dyT[r][:,b] (x) xT[r][:,b] WITHOUT forming it:
 * |dW|^2 = scale^2 * sum_{i,j} Gx[i][j] Gdy[i][j] over the (R Bp)^2 Gram matrices of the two tables (same arguments as
 * dsr_linear_wgrad_adam).  The workspace (16-byte aligned, dsr_linear_factor_gram_workspace() bytes) starts with
 * dsr_linear_factor_gram_dots() fp64 partial sums -- what dsr_clip_finalize takes as gram_partials -- followed by the
 * per-block fp32 Gram partials they were combined from (in fp64).  R * Bp > 512: DSR_E_UNSUPPORTED (both queries answer 0). */
size_t dsr_linear_factor_gram_workspace(int Bp, int O, size_t K, int R);
int dsr_linear_factor_gram_dots(int Bp, int R);
int dsr_linear_factor_gram(int dtype, const void* dyT16_all, const void* xT16_all, int Bp, int O, size_t K, int R, float scale,
                           void* workspace, size_t ws_bytes, dsr_stream_t s);
/* out[b] = sigmoid(h[b][:] . w2 + b2[0]);  b2 is required (a one-element device tensor): NULL is DSR_E_ARG */
int dsr_dense2_fwd(const float* h, const float* w2, const float* b2, int B, int K1, float* out, dsr_stream_t s);
/* backward of the fp32 tail; also emits the 16-bit dy / dy^T operands of the two dense1 GEMMs */
int dsr_dense2_bwd(int dtype, const float* dout, const float* out, const float* h, const float* w2, int B, int K1,
                   int Bp, float slope, float* dw2, float* db2, float* db1, void* dy16, void* dyT16, dsr_stream_t s);

/* ------------------------------------------------------------------ resampling / data movement (resample.hip) */
/* nn.MaxPool2d(2,2) of the VGG19 trunk (utils/GAN.py:24,29,38,47) and of DIP's downsample_mode='max'.  torch's rule: the window is
 * scanned (0,0),(0,1),(1,0),(1,1) and the running maximum replaced when v > m or v is NaN -- a NaN propagates; the backward
 * routes dy to the last NaN of the window if it holds one, otherwise to the first maximum */
int dsr_maxpool2_fwd(int dtype, const void* x, void* y, int N, int H, int W, int Cp, dsr_stream_t s);
int dsr_maxpool2_bwd(int dtype, const void* x, const void* dy, void* dx, int N, int H, int W, int Cp, dsr_stream_t s);
/* the same with the backward of the ReLU that produced x folded in (conv + ReLU + MaxPool of the VGG trunk, utils/GAN.py:24-47):
 * dx = routed dy where the window maximum is > 0.  x must be a ReLU output: no NaN, nothing negative */
int dsr_maxpool2_relu_bwd(int dtype, const void* x, const void* dy, void* dx, int N, int H, int W, int Cp, dsr_stream_t s);
/* nn.AvgPool2d(2,2) after a stride-1 conv: downsample_mode='avg' of models/DIP/utils.py:86-94 (floor mode);
 * H, W are the INPUT size of the pool.  downsample_mode='max' uses dsr_maxpool2_* above. */
int dsr_avgpool2_fwd(int dtype, const void* x, void* y, int N, int H, int W, int Cp, dsr_stream_t s);
int dsr_avgpool2_bwd(int dtype, const void* dy, void* dx, int N, int H, int W, int Cp, dsr_stream_t s);
/* nn.Upsample(scale_factor=2, mode='nearest') (models/DIP/skip.py:77, the builder's default); H, W = INPUT size */
int dsr_nearest2x_fwd(int dtype, const void* x, void* y, int N, int H, int W, int Cp, dsr_stream_t s);
int dsr_nearest2x_bwd(int dtype, const void* dy, void* dx, int N, int H, int W, int Cp, dsr_stream_t s);
/* nn.Upsample(scale_factor=2, mode='bilinear') (models/DIP/skip.py:77); H, W are the INPUT size */
int dsr_bilinear2x_fwd(int dtype, const void* x, void* y, int N, int H, int W, int Cp, dsr_stream_t s);
int dsr_bilinear2x_bwd(int dtype, const void* dy, void* dx, int N, int H, int W, int Cp, dsr_stream_t s);
/* VGG19_Weights.IMAGENET1K_V1.transforms() (utils/GAN.py:82-83): separable antialiased resize + crop + normalise.
 * src fp32 NCHW [N][C<=3][H][W] -> dst NHWC 16-bit [N][OH][OW][8]; tables are host-built (utils/GAN.py mirror):
 * per output index start/count/weights[KT]; the backward takes the transposed tables. */
int dsr_resize_norm_fwd(int dtype, const float* src, void* dst, int N, int C, int H, int W, int OH, int OW,
                        const int* ys, const int* yc, const float* yw, const int* xs, const int* xc, const float* xw,
                        int KT, const float* mean3, const float* std3, dsr_stream_t s);
int dsr_resize_norm_bwd(int dtype, const void* dout, float* dsrc, int N, int C, int H, int W, int OH, int OW,
                        const int* ty_s, const int* ty_c, const float* ty_w, const int* tx_s, const int* tx_c,
                        const float* tx_w, int KT, const float* std3, dsr_stream_t s);
/* Concat with centre crop (models/DIP/utils.py:18-38) and its adjoint: 16-bit NHWC box copy
 * dst[n][dy0+y][dx0+x][cd0+c] = src[n][sy0+y][sx0+x][cs0+c], y<BH, x<BW, c<C */
int dsr_box_copy(const void* src, void* dst, int N, int BH, int BW, int C, int SH, int SW, int SCp, int sy0, int sx0,
                 int cs0, int DH, int DW, int DCp, int dy0, int dx0, int cd0, dsr_stream_t s);
/* Downsampler (utils/downsampler.py:44-71): depthwise k x k kernel, stride f, ReplicationPad2d(p); fp32 NCHW, NC = N*C */
int dsr_downsample_fwd(const float* x, const float* kern, float* y, int NC, int H, int W, int k, int f, int p,
                       dsr_stream_t s);
int dsr_downsample_bwd(const float* dy, const float* kern, float* dx, int NC, int H, int W, int k, int f, int p,
                       dsr_stream_t s);

/* Dense (learnable) Downsampler: ReplicationPad2d(p) + Conv2d(C, C, k, stride=f) + bias, every filter live -- what
 * get_params('down') optimises (utils/DIP.py:59-61).  fp32 NCHW, contiguous; w is OIHW [C][C][k][k]; 1 <= C <= 4
 * (more: DSR_E_UNSUPPORTED); OH = (H + 2p - k) / f + 1 (an empty output is DSR_E_ARG).  fp32 FMA throughout.
 *   fwd  : y[n][co][oy][ox] = b[co] + sum_ci sum_ij w[co][ci][i][j] x[n][ci][clamp(oy f + i - p)][clamp(ox f + j - p)];
 *          b may be NULL (no bias)
 *   dgrad: dx = the adjoint with respect to x, the replicate pad's included (border pixels collect what the pad copied
 *          from them); dx is written, not accumulated
 *   wgrad: dw[co][ci][i][j] = sum_{n,oy,ox} dy[n][co][oy][ox] x[n][ci][clamp(..)][clamp(..)], db[co] = sum dy (db may be
 *          NULL); both written, not accumulated.  Deterministic: per-slab partials in `workspace`
 *          (dsr_downsample_dense_wgrad_workspace bytes, a pure host query; too small: DSR_E_WORKSPACE) summed in index
 *          order by a second launch, no float atomics -- two calls on the same inputs give the same bits. */
int dsr_downsample_dense_fwd(const float* x, const float* w, const float* b, float* y, int N, int C, int H, int W, int k,
                             int f, int p, dsr_stream_t s);
int dsr_downsample_dense_dgrad(const float* dy, const float* w, float* dx, int N, int C, int H, int W, int k, int f, int p,
                               dsr_stream_t s);
size_t dsr_downsample_dense_wgrad_workspace(int N, int C, int H, int W, int k, int f, int p);
int dsr_downsample_dense_wgrad(const float* x, const float* dy, float* dw, float* db, void* workspace,
                               size_t workspace_bytes, int N, int C, int H, int W, int k, int f, int p, dsr_stream_t s);

/* SSIM as the reference's scripts measure it (torchmetrics StructuralSimilarityIndexMeasure at train_GAN.py:31,111,
 * eval_GAN.py:31,48): Gaussian 11x11 sigma 1.5 window, per plane, window positions inside the image; c1 = (k1 range)^2,
 * c2 = (k2 range)^2 (K1 0.01, K2 0.03 there), both > 0 and finite.  The metric modules of metrics.py and evaluate.ssim.
 * dsr_ssim_img_f32: fp32 NCHW img1, img2 [N][C][H][W] -> per_image[N] = mean SSIM over the image's C x (H-10) x (W-10) window
 * positions (nullable), total[0] (+= if accumulate; nullable) = total_scale * sum_n per_image[n]; partial: scratch of
 * dsr_ssim_img_blocks(N, C, H, W) floats.  Two launches (tiles, then a one-block fold in a fixed order).
 * dsr_ssim_bwd_f32: g[N] (device) = upstream gradient of each per-image value -> grad1 / grad2 (fp32 NCHW, either nullable, not
 * both) = g[n] d per_image[n] / d img, one launch; the moments are recomputed per tile.
 * dsr_psnr_stats_f32: preds, target fp32 [N][E] -> per block of dsr_psnr_blocks(N, E) (blocks of one image are consecutive):
 * partial_sse[b] = sum of squared errors, partial_keys[2b], [2b+1] = order-preserving keys of the target's min, max
 * (f >= 0: bits | 0x80000000, f < 0: ~bits).
 * dsr_psnr_finalize: log_scale = 10 / ln(base).  per_image != null: per_image[n] = log_scale (2 ln data_range - ln(SSE_n / E)),
 * value (nullable) = value_scale * sum_n per_image[n], state[0] += that sum, state[1] += N.  per_image == null: value = PSNR of the
 * whole batch with range = data_range, or (infer_range) max(target max, 0) - min(target min, 0); state (nullable, double[4]:
 * SSE, count, running min, running max) += the batch's SSE and N E, min / max folded in.
 * dsr_metric_accumulate: state[0] += sum_n per_image[n], state[1] += N (double[2]).
 * dsr_metric_compute: out[0] = state[0] (mode 0), state[0] / state[1] (mode 1), or the PSNR of a dsr_psnr_finalize batch state
 * (mode 2; range = data_range, or state[3] - state[2] with infer_range). */
int dsr_ssim_img_blocks(int N, int C, int H, int W);
int dsr_ssim_img_f32(const float* img1, const float* img2, int N, int C, int H, int W, float c1, float c2, float* partial,
                     float* per_image, float* total, float total_scale, int accumulate, dsr_stream_t s);
int dsr_ssim_bwd_f32(const float* img1, const float* img2, int N, int C, int H, int W, float c1, float c2, const float* g,
                     float* grad1, float* grad2, dsr_stream_t s);
int dsr_psnr_blocks(int N, int E);
int dsr_psnr_stats_f32(const float* preds, const float* target, int N, int E, float* partial_sse, unsigned* partial_keys,
                       dsr_stream_t s);
int dsr_psnr_finalize(const float* partial_sse, const unsigned* partial_keys, int N, int E, int infer_range, float data_range,
                      float log_scale, float* per_image, float* value, float value_scale, double* state, dsr_stream_t s);
int dsr_metric_accumulate(const float* per_image, int N, double* state, dsr_stream_t s);
int dsr_metric_compute(const double* state, int mode, int infer_range, float data_range, float log_scale, float* out,
                       dsr_stream_t s);

/* Multi-scale SSIM (torchmetrics MultiScaleStructuralSimilarityIndexMeasure restated; metrics.py).  Per scale s < L the pair
 * of images gives per-image means of SSIM and of its contrast-structure term cs = (2 cov + c2) / (var1 + var2 + c2) over the
 * same window positions as dsr_ssim_img_f32; between scales both images are halved by a 2x2 mean (floor: an odd last row or
 * column is dropped); out[n] = prod_s v_s[n]^betas[s] with v = (cs_0 .. cs_{L-2}, ssim_{L-1}) after `normalize`.
 * 1 <= L <= DSR_MSSSIM_MAX_SCALES, and H >> (L-1), W >> (L-1) >= 11: H, W >= dsr_msssim_min_size(L) = 11 << (L-1) (0: bad L).
 * dsr_ssim_cs_img_f32: sim[N], cs[N] (either nullable, not both) = the two per-image means; partial: 8-byte aligned scratch of
 * 2 * dsr_ssim_cs_img_blocks(N, C, H, W) floats.  Two launches (tiles, then a one-block fold in a fixed order).
 * dsr_avgpool2_pair_f32: in1, in2 [planes][H][W] -> out1, out2 [planes][H/2][W/2], one launch.
 * dsr_msssim_pyramid_floats: the floats of one image's levels 1 .. L-1, [N][C][H >> s][W >> s] each, level 1 first (0: bad sizes).
 * dsr_msssim_combine: raw [L][N] (device; row s = the cs means of scale s, row L-1 the SSIM means), betas[L] (HOST, positive
 * and finite), normalize 0 none / 1 relu (max(raw, 0)) / 2 simple ((raw + 1) / 2) -> vals [L][N] (nullable) the normalised
 * values, per_image[N] (nullable), total[0] (nullable) = total_scale * sum_n per_image[n], factors [L][N] (nullable) =
 * d per_image[n] / d raw[s][n] = betas[s] per_image[n] / vals[s][n] (halved under simple).  Under relu a clamped value gives
 * per_image[n] = 0 and all of that image's factors 0.  One launch.
 * dsr_msssim_bwd_f32: one scale of the backward.  g[N] = upstream of per_image; w_sim[N], w_cs[N] (either nullable, not both) =
 * this scale's factors for the SSIM / cs mean; coarse1 / coarse2 (nullable) [N][C][H/2][W/2] = the gradient that arrived at
 * the pooled images.  grad1 / grad2 (either nullable, not both; a coarse gradient needs its grad) =
 * g (w_sim d sim + w_cs d cs) / d img + 0.25 coarse[y/2][x/2] inside the pooled extent.  One launch of
 * dsr_msssim_bwd_blocks(N, C, H, W) blocks; calling it from scale L-1 down to 0 is the whole backward. */
#define DSR_MSSSIM_MAX_SCALES 8
int dsr_msssim_min_size(int L);
size_t dsr_msssim_pyramid_floats(int N, int C, int H, int W, int L);
int dsr_ssim_cs_img_blocks(int N, int C, int H, int W);
int dsr_ssim_cs_img_f32(const float* img1, const float* img2, int N, int C, int H, int W, float c1, float c2, float* partial,
                        float* sim, float* cs, dsr_stream_t s);
int dsr_avgpool2_pair_f32(const float* in1, const float* in2, float* out1, float* out2, int planes, int H, int W,
                          dsr_stream_t s);
int dsr_msssim_combine(const float* raw, int N, int L, const float* betas, int normalize, float* vals, float* per_image,
                       float* total, float total_scale, float* factors, dsr_stream_t s);
int dsr_msssim_bwd_blocks(int N, int C, int H, int W);
int dsr_msssim_bwd_f32(const float* img1, const float* img2, int N, int C, int H, int W, float c1, float c2, const float* g,
                       const float* w_sim, const float* w_cs, const float* coarse1, const float* coarse2, float* grad1,
                       float* grad2, dsr_stream_t s);

/* LPIPS with the AlexNet trunk (torchmetrics LearnedPerceptualImagePatchSimilarity(net_type='alex') at train_GAN.py:32,112,
 * eval_GAN.py:32,49, DIP.py:75,185; csrc/lpips.hip).  The five convolutions are dsr_conv_fwd calls; these are the rest.
 * dsr_lpips_tap_sizes: hw[2k], hw[2k+1] = height, width of tap k (relu1..relu5) for an H x W image; DSR_E_ARG if the trunk
 * would produce an empty map.
 * dsr_lpips_stem_prep: fp32 NCHW [N][3][H][W] img1, img2 -> out [2N][h1+2][w1+2][64] 16-bit NHWC (img1 first): optional
 * x -> 2x - 1 (normalize), the scaling layer, zero padding 2, then the 4x4 space-to-depth, channel (py*4 + px)*3 + c of block
 * (by, bx) = padded pixel (4by + py, 4bx + px) of channel c; channels 48..63 and pixels past the padded image are 0.  The stem
 * is then a 3x3 / stride-1 / pad-0 conv of 64 -> 64 channels.  range[2] (device, preset to 0xffffffff, 0) receives the
 * atomic min / max of the raw input values as order-preserving keys (f >= 0: bits | 0x80000000, f < 0: ~bits).
 * dsr_maxpool3s2_fwd: nn.MaxPool2d(3, 2) (floor mode, no padding) on NHWC 16-bit; H, W = INPUT size (>= 3).
 * dsr_lpips_distance: taps k < ntaps (HOST tables): feats[k] = [2N][hw[k]][cp[k]] 16-bit, lin_w[k] = [c[k]] fp32 device;
 * partial gets dsr_lpips_distance_blocks(ntaps, hw, N) block sums of sum_c w[c] (n1[c] - n2[c])^2, n = f / sqrt(1e-8 + |f|^2).
 * dsr_lpips_finalize: per_image[N] = sum_k (1/hw[k]) * (tap k's sums of image n); total[0] (+= if accumulate) =
 * total_scale * sum_n per_image[n]. */
int dsr_lpips_tap_sizes(int H, int W, int* hw);
int dsr_lpips_stem_prep(int dtype, const float* img1, const float* img2, int N, int H, int W, int normalize, void* out,
                        unsigned* range, dsr_stream_t s);
int dsr_maxpool3s2_fwd(int dtype, const void* x, void* y, int N, int H, int W, int Cp, dsr_stream_t s);
int dsr_lpips_distance_blocks(int ntaps, const int* hw, int N);
int dsr_lpips_distance(int dtype, int ntaps, const void* const* feats, const float* const* lin_w, const int* hw, const int* cp,
                       const int* c, int N, float* partial, dsr_stream_t s);
int dsr_lpips_finalize(int ntaps, const int* hw, int N, const float* partial, float* per_image, float* total, float total_scale,
                       int accumulate, dsr_stream_t s);

/* The backward of the same path (LPIPS as a training loss; the five input gradients are dsr_conv_dgrad /
 * dsr_conv_dgrad_masked calls).  All gradients are 16-bit NHWC and carry the caller's static loss `scale` (a power of two keeps
 * it exact), which dsr_lpips_stem_prep_bwd divides out again.
 * dsr_lpips_distance_bwd: tables as dsr_lpips_distance; g[N] (device fp32) = upstream gradient of each image's value.  With
 * s = sqrt(1e-8 + |f|^2), n = f / s, u[c] = 2 w[c] (n1[c] - n2[c]) g[image] scale / hw[k]:  d1[k] = (u - n1 <u, n1>) / s1 * (f1 > 0),
 * d2[k] = -(u - n2 <u, n2>) / s2 * (f2 > 0), each [N][hw[k]][cp[k]]: the gradient at the pre-activation of the tap's ReLU.  d1 or
 * d2 may be NULL (that half is not written), not both.
 * dsr_maxpool3s2_bwd: dx [N][H][W][Cp] = autograd of nn.MaxPool2d(3, 2) for dy [N][OH][OW][Cp] with the windows' arg-max
 * recomputed from x (torch's tie rule: row-major scan, first maximum), fp32 sum of the at most four dy a pixel wins; times
 * (x > 0) if relu_mask; plus addend (same shape as x, nullable); one rounding.
 * dsr_lpips_stem_prep_bwd: dx [N][h1+2][w1+2][64] (gradient of dsr_lpips_stem_prep's output, one image set) -> dimg fp32
 * [N][3][H][W] = dx gathered back, / scaling-layer scale[c], * 2 if normalize, / scale. */
int dsr_lpips_distance_bwd(int dtype, int ntaps, const void* const* feats, const float* const* lin_w, const int* hw, const int* cp,
                           const int* c, int N, const float* g, float scale, void* const* d1, void* const* d2, dsr_stream_t s);
int dsr_maxpool3s2_bwd(int dtype, const void* x, const void* dy, const void* addend, void* dx, int N, int H, int W, int Cp,
                       int relu_mask, dsr_stream_t s);
int dsr_lpips_stem_prep_bwd(int dtype, const void* dx, int N, int H, int W, int normalize, float scale, float* dimg,
                            dsr_stream_t s);

/* measurement aid: out16[2x] = shader-clock cycle counter (s_memtime) and out16[2x+1] = 100 MHz real-time counter
 * (s_memrealtime) of XCD x (8 pairs; zero-fill before), read when the stream reaches this launch; two samples give the average
 * shader clock of what ran between them (difference pairs of the same XCD only: the cycle counters are per XCD) */
int dsr_clock_sample(unsigned long long* out16, dsr_stream_t s);
/* ---- data-side byte kernels (dataset.py:9-62,121-159; utils/degradation.py:5-20) on device-resident
 * uint8 HWC images.  Integer / byte arithmetic, bit-identical to Pillow / numpy.
 * dsr_resample_u8: ONE pass of Pillow's 8-bit resampler along `axis` (1 = width, 0 = height); `bounds` [out_size][2] and `kk`
 * [out_size][ksize] are the 22-bit fixed-point tables of Pillow's precompute_coeffs + normalize_coeffs_8bpc (device int32,
 * built on the host by utils/degradation.py: resample_tables).  Image.resize(.., BICUBIC) = width pass, then height pass. */
int dsr_resample_u8(const unsigned char* src, unsigned char* dst, int H, int W, int C, int axis, int out_size, const int* bounds,
                    const int* kk, int ksize, dsr_stream_t s);
/* out = uint8(clip(img + noise, 0, 255)) (truncating cast); noise float64 (drawn by numpy, as the reference does) or float32 */
int dsr_noise_gaussian_u8(const unsigned char* img, const void* noise, int noise_is_f64, unsigned char* out, size_t n, dsr_stream_t s);
/* salt -> 255, then pepper -> 0, per pixel over all channels; salt / pepper: [H][W] bytes (non-zero = hit) */
int dsr_salt_pepper_u8(const unsigned char* img, const unsigned char* salt, const unsigned char* pepper, unsigned char* out, int H,
                       int W, int C, dsr_stream_t s);
/* B patches of ph x pw pixels, one from each of B RGB images (HOST tables of device pointers / sizes / corners), converted to an
 * fp32 [B][3][ph][pw] batch: ToTensor (/255) followed by the scaling `mode` selects */
enum { DSR_PATCH_UNIT = 0,      /* [0,1]: ToTensor only */
       DSR_PATCH_LR_REF = 1,    /* dataset.py:152: /255 a second time (the reference's LR scaling as written) */
       DSR_PATCH_HR_REF = 2,    /* dataset.py:155-157: /255 a second time, *2, -1 (as written) */
       DSR_PATCH_HR_UNIT = 3 }; /* *2 - 1: the [-1,1] its comments intend */
/* dataset.py:149-159 in place on an fp32 tensor ToTensor already put in [0,1]: mode DSR_PATCH_LR_REF: x /= 255;
 * DSR_PATCH_HR_REF: x = x / 255 * 2 - 1 (true divisions, as on the host) */
int dsr_scale_images_f32(float* x, size_t n, int mode, dsr_stream_t s);
#define DSR_PATCH_BATCH_MAX 64
int dsr_patch_batch_u8(int count, const unsigned char* const* images, const int* heights, const int* widths, const int* tops,
                       const int* lefts, int ph, int pw, int mode, float* out, dsr_stream_t s);

/* ------------------------------------------------------------------ flips and quarter turns (d4.hip)
 * The eight elements of the dihedral group D4 acting on [..., H, W] images.  Code k in 0..7, r = k % 4, m = k >= 4:
 *   T_k(x) = rot90(flip(x, W) if m else x, r)        (torch.rot90 / torch.flip; H x W for even r, W x H for odd r)
 * as a gather T_k(x)[i][j] = x[a][b]:  r = 0: (i, j)   1: (j, W-1-i)   2: (H-1-i, W-1-j)   3: (H-1-j, i);  if m, b = W-1-b
 * (H, W: the source's sizes).  Training augmentation (one code per patch) and geometric self-ensemble at inference. */
/* dsr_patch_batch_u8 with one code per patch (HOST table xforms[count]): patch b, scaled by `mode` as there, is stored as
 * T_{xforms[b]} of itself in out [count][3][ph][pw].  A code with odd r needs ph == pw. */
int dsr_patch_batch_u8_d4(int count, const unsigned char* const* images, const int* heights, const int* widths, const int* tops,
                          const int* lefts, const int* xforms, int ph, int pw, int mode, float* out, dsr_stream_t s);
/* src [planes][h][w] fp32 -> T_k(src) for every k set in the 8-bit mask, one launch: the codes with even r to dst_even
 * [n_even][planes][h][w], those with odd r to dst_odd [n_odd][planes][w][h], each in ascending k.  A destination may be NULL
 * only when the mask holds none of its codes. */
int dsr_d4_expand_f32(const float* src, int planes, int h, int w, int mask, float* dst_even, float* dst_odd, dsr_stream_t s);
/* The inverse and the mean, one launch: src_even [n_even][planes][H][W] and src_odd [n_odd][planes][W][H] laid out as
 * dsr_d4_expand_f32 writes them; dst [planes][H][W] = (sum over the k of mask, ASCENDING, of T_k^-1(src_k)) * (1.0f / count),
 * summed in fp32 in exactly that order (the first term is taken as it is): the result is defined bit for bit. */
int dsr_d4_mean_f32(const float* src_even, const float* src_odd, int planes, int H, int W, int mask, float* dst, dsr_stream_t s);

/* ------------------------------------------------------------------ blind degradation (degrade.hip)
 * LR = quant(clip((HR (*) k) sampled every `scale`-th pixel + sigma * z)) on uint8 [H][W][3] device images, a blur kernel and
 * a noise level per sample.  LR pixel (Y, X) of the LR grid, channel c, r = ks / 2, taps in row-major order:
 *   acc = 0;  for i, for j:  acc = fmaf(k[i][j], (float)HR[refl(s*Y + offset + i - r, H)][refl(s*X + offset + j - r, W)][c], acc)
 *   if noise:  acc = fmaf(noise_std[b], z[b][c][y][x], acc)        (z at the OUTPUT position, after the D4 code)
 *   acc = min(max(acc, 0), 255);  if quantise: acc = rintf(acc)    (half to even)
 *   v = acc / 255.0f, then the scaling `mode` selects, as dsr_patch_batch_u8
 * refl: reflection at the borders of the whole image without repeating the edge (-1 -> 1, H -> H - 2).  offset = 0 samples
 * blurred[0::s, 0::s].  Both entry points run the same code: a patch equals that region of the whole image bit for bit. */
/* dsr_patch_batch_u8_d4 cutting LR patches out of HR images: HOST tables as there, tops / lefts in LR pixels, xforms NULL for
 * no D4 codes; kernels: device fp32 [count][ks][ks], ks odd in 1..21 and ks / 2 < min(H, W); scale in 1..8, offset in
 * 0..scale-1; noise: device fp32 [count][3][ph][pw] standard-normal draws or NULL, noise_std: device fp32 [count] in 0..255
 * units (given exactly when noise is); out: fp32 [count][3][ph][pw].  The centre scale * (top + ph - 1) + offset of the last
 * row (column) of a patch has to lie inside its image. */
int dsr_degrade_batch_u8(int count, const unsigned char* const* images, const int* heights, const int* widths, const int* tops,
                         const int* lefts, const int* xforms, int ph, int pw, int scale, int offset, const float* kernels, int ks,
                         const float* noise, const float* noise_std, int quantise, int mode, float* out, dsr_stream_t s);
/* One image, one kernel [ks][ks]: out uint8 [h][w][3], h = (H - offset + scale - 1) / scale and w likewise, always clipped and
 * rounded; noise: device fp32 [3][h][w] or NULL, noise_std: device fp32 [1] */
int dsr_degrade_image_u8(const unsigned char* image, int H, int W, int scale, int offset, const float* kernel, int ks,
                         const float* noise, const float* noise_std, unsigned char* out, dsr_stream_t s);

/* ------------------------------------------------------------------ JPEG round trip (jpeg.hip)
 * Baseline JPEG compression and decompression of RGB images at a quality per sample, uint8 in, uint8 out, no bitstream (the
 * entropy coder is lossless): the last stage of the BSRGAN / Real-ESRGAN degradation.  With libjpeg's default "islow" DCT
 * the codec is integer arithmetic throughout, and this is its definition here (equal to Pillow's
 * save(..., 'JPEG', quality=q, subsampling=0|2) + open; tests/jpeg_ref.py restates it in numpy).  All values are integers,
 * >> is an arithmetic shift, DS(x, n) = (x + (1 << (n-1))) >> n, F(x) = int(x * 65536 + 0.5).
 *  1. Pad on the right and bottom by edge replication to multiples of 8 (4:4:4) or 16 (4:2:0).
 *  2. Y  = ( F(.299) R + F(.587) G + F(.114) B + 32768) >> 16
 *     Cb = (-F(.16874) R - F(.33126) G + F(.5) B + (128 << 16) + 32767) >> 16
 *     Cr = ( F(.5) R - F(.41869) G - F(.08131) B + (128 << 16) + 32767) >> 16
 *  3. 4:2:0 only: each chroma plane becomes (a + b + c + d + bias) >> 2 over the 2x2 cells of the padded plane, bias = 1 in
 *     even output columns and 2 in odd ones; then every chroma row at or below ceil(H/2) is replaced by row ceil(H/2) - 1
 *     (the bottom padding repeats the last DOWNSAMPLED row, not the last image row).
 *  4. s = 5000 / q for q < 50, else 200 - 2 q;  t = clip((base * s + 50) / 100, 1, 255) with the two Annex-K base tables
 *     (luminance for Y, chrominance for Cb and Cr); q in 1..100.
 *  5. Per 8x8 block, jfdctint on sample - 128: rows, then columns, CONST_BITS = 13, PASS1_BITS = 2, constants 2446, 3196,
 *     4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172; pass 1 descales by 11 with the DC and index-4
 *     terms << 2, pass 2 by 15 with those terms DS(., 2): 8 times the DCT.
 *  6. d = t << 3;  k = (|c| + (d >> 1)) / d with the sign of c;  dequantised: k * t.
 *  7. jidctint: columns (descale 11), then rows (descale 18); + 128, clipped to 0..255.
 *  8. 4:2:0 only: chroma is upsampled to 2 ceil(H/2) x 2 ceil(W/2) from the ceil(H/2) x ceil(W/2) real samples alone.
 *     ceil(W/2) > 2: libjpeg's triangle filter -- cs = 3 * this row + the nearer neighbour row (the row above for the upper
 *     output row, the row below for the lower one, replicated at the edges); out[2i] = (3 cs[i] + cs[i-1] + 8) >> 4,
 *     out[2i+1] = (3 cs[i] + cs[i+1] + 7) >> 4, the first column (4 cs[0] + 8) >> 4, the last (4 cs[last] + 7) >> 4.
 *     ceil(W/2) <= 2: every sample is repeated 2x2.
 *  9. cb = Cb - 128, cr = Cr - 128;  R = Y + ((F(1.402) cr + 32768) >> 16),  B = Y + ((F(1.772) cb + 32768) >> 16),
 *     G = Y + ((-F(.34414) cb + 32768 - F(.71414) cr) >> 16), each clipped to 0..255; cropped to H x W.
 * 32-bit integers hold every intermediate.  Nothing is allocated, read back or waited for: the calls can be captured into a
 * graph.  quality: DEVICE int32 [count], 1..100 (the kernels clamp a value outside; they derive the tables themselves);
 * subsampling: 0 (4:4:4, one launch) or 2 (4:2:0, two launches), Pillow's numbers; count in 1..65535, H and W in 1..65536. */
/* bytes of workspace of the two calls below: 0 for 4:4:4 (workspace may then be NULL) and for arguments they refuse; for
 * 4:2:0 the decoded Y, Cb and Cr planes of every image.  A pure host query. */
size_t dsr_jpeg_workspace(int count, int H, int W, int subsampling);
/* in, out: uint8 [count][H][W][3]; out must not be in; workspace: 16-byte aligned device memory of dsr_jpeg_workspace bytes */
int dsr_jpeg_u8(const unsigned char* in, unsigned char* out, int count, int H, int W, const int* quality, int subsampling,
                void* workspace, dsr_stream_t s);
/* The patch batches of the data path: in fp32 [count][3][h][w] in DSR_PATCH_UNIT scaling, read as the grey level
 * (int)rintf(min(max(255 * v, 0), 255)); out, same shape, not in: the decoded level as a float, / 255.0f, then the scaling
 * `mode` selects, as dsr_patch_batch_u8 */
int dsr_jpeg_batch_f32(const float* in, float* out, int count, int h, int w, const int* quality, int subsampling, int mode,
                       void* workspace, dsr_stream_t s);

/* ------------------------------------------------------------------ L-BFGS (lbfgs.hip)
 * torch.optim.LBFGS with line_search_fn=None (utils/DIP.py:24-31) in the vector-free form (Chen, Wang & Zhou, NIPS 2014):
 * the two-loop recursion runs on the Gram matrix of the basis {s_i, y_i, g} in fp64; the vectors are read by two streaming
 * passes.  A flat vector of n fp32 elements is split into `count` tensors (HOST tables of device pointers and element counts,
 * read before the call returns, summing to n).  history: 1 .. 1024 pairs.
 * ws: dsr_lbfgs_workspace(history, n, count) bytes, zero-filled before the first call (that is the fresh state); vecs:
 * dsr_lbfgs_vector_floats(history, n) floats, zero-filled.  The pair (ws, vecs) is the optimizer's whole state.
 * vecs, with m = history: 2 (m + 1) + 2 fp32 vectors of n_pad floats each, n_pad = n rounded up to a multiple of 4; the
 * n_pad - n padding floats of every vector stay 0.  Vector j (0 <= j <= m) is S slot j, vector m + 1 + j is Y slot j, vector
 * 2 (m + 1) + b is gradient buffer b (0 or 1; one holds the current flat gradient, the other the previous one, and they swap
 * on every pass that computes a direction).  The ring has m + 1 slots: at most m hold committed pairs, and one free slot
 * holds the pending pair (s = t d of the last direction, y = g - g_prev written by the gather pass) until the next scalar
 * pass commits it (ys > 1e-10: it becomes the newest pair, and a full ring frees its oldest slot) or drops it.  A pass
 * writes the current gradient buffer, Y of the free slot and, if it computes a direction, S of the slot that is free
 * afterwards; it writes no other float of vecs.
 * The first five ints of ws: [0] n_iter and [1] func_evals (state["n_iter"], state["func_evals"] of torch's optimizer, over
 * all step() calls), [2] iterations and [3] closure calls of the running step(), [4] live pairs: the committed pairs held
 * in the ring, 0 .. history, after the last scalar pass (a dropped pair does not count; it stays at history once the ring
 * wraps).  The rest of ws is private.
 * Per closure call: dsr_lbfgs_gather (the .grad tensors; NULL entries are zero gradients), dsr_lbfgs_dots, dsr_lbfgs_scalar
 * (loss: the closure's device scalar; first = 1 for the first closure of a step()), dsr_lbfgs_combine (the parameters).
 * The scalar pass writes stop[0] = 1 when torch would not call the closure again (every break of lbfgs.py). */
size_t dsr_lbfgs_workspace(int history, size_t n, int count);
size_t dsr_lbfgs_vector_floats(int history, size_t n);
int dsr_lbfgs_gather(int count, const float* const* grads, const size_t* numel, void* ws, size_t ws_bytes, float* vecs,
                     int history, size_t n, dsr_stream_t s);
int dsr_lbfgs_dots(void* ws, size_t ws_bytes, const float* vecs, int history, size_t n, int count, dsr_stream_t s);
int dsr_lbfgs_scalar(void* ws, size_t ws_bytes, int history, size_t n, int count, const float* loss, int first, int* stop,
                     double lr, int max_iter, int max_eval, double tolerance_grad, double tolerance_change, dsr_stream_t s);
int dsr_lbfgs_combine(int count, float* const* params, const size_t* numel, void* ws, size_t ws_bytes, float* vecs,
                      int history, size_t n, dsr_stream_t s);

/* ------------------------------------------------------------------ exponential moving average of a model's weights
 * (optim.WeightEMA).  torch.optim.swa_utils.AveragedModel with get_ema_multi_avg_fn, with nothing read on the host: the
 * count of averaged steps is a device word and "copy or lerp" is decided inside the kernel, so an update is the same launch
 * sequence on every call and replays from a HIP graph.  Order within a step: after the Adam launches, every
 * dsr_ema_update_multi launch, then ONE dsr_ema_tick; under a dynamic loss scale, before dsr_amp_update clears found_inf.
 * dsr_ema_update_multi: shadow[i] <- shadow[i] + w * (p[i] - shadow[i]) over `count` fp32 tensors (HOST tables of device
 * pointers and element counts, read before the call returns; 64 tensors per launch; an entry with n[i] == 0, or with both
 * pointers NULL, is skipped; views 4 / 8 / 12 bytes off a 16-byte boundary are fine).  w comes from n_averaged[0] (int32,
 * only read here):
 *   mode 0 (DSR_EMA_TORCH):  n_averaged == 0: shadow <- p, an exact copy; otherwise w = 1 - decay
 *   mode 1 (DSR_EMA_WARMUP): k = n_averaged + 1, w = 1 - min(decay, (1 + k) / (10 + k)); no copy step
 * copy (nullable HOST array): copy[i] != 0 -> tensor i is copied exactly whatever n_averaged is (buffers that follow the
 * model).  found_inf (nullable; the dynamic loss scaler's fp32 word): != 0 -> no write at all.  Plain vector stores, no
 * atomics: the same bits on every run.  0 <= decay <= 1.
 * dsr_ema_tick: n_averaged[0] += 1 unless found_inf[0] != 0 (one thread; the only writer of that word).
 * dsr_ema_swap_multi: a[i] <-> b[i], bit for bit, same tables (a[i] == b[i] is a no-op; other overlaps are undefined). */
#define DSR_EMA_TORCH 0
#define DSR_EMA_WARMUP 1
int dsr_ema_update_multi(int count, float* const* shadow, const float* const* p, const size_t* n, const unsigned char* copy,
                         float decay, int mode, const int* n_averaged, const float* found_inf, dsr_stream_t s);
int dsr_ema_tick(int* n_averaged, const float* found_inf, dsr_stream_t s);
int dsr_ema_swap_multi(int count, float* const* a, float* const* b, const size_t* n, dsr_stream_t s);

/* ------------------------------------------------------------------ Y-channel PSNR / SSIM with a border shave (luma.hip)
 * The evaluation protocol of the published super-resolution tables (metrics.LumaPeakSignalNoiseRatio,
 * metrics.LumaStructuralSimilarityIndexMeasure, metrics.rgb_to_y; PARITY UNPINNED: restated from the documented behaviour of
 * MATLAB's rgb2ycbcr and basicsr).  Images are [N][3][H][W] of dtype DSR_BF16, DSR_F16 or DSR_F32, read as they are and
 * computed in fp32:
 *   q(x) = rintf(fminf(fmaxf(x, 0), 1) * 255.0f) / 255 if quantize, else x;   Y = (16 + 65.481 r + 128.553 g + 24.966 b) / 255;
 *   region: rows [shave, H - shave), columns [shave, W - shave), h x w = (H - 2 shave) x (W - 2 shave) >= 1 x 1.
 * dsr_luma_blocks: the number of partial sums of one launch (N images, consecutive blocks per image; 0: bad sizes).
 * dsr_luma_sse_stats: partial_sse[dsr_luma_blocks()] = per-block sums of dY^2 over the region, dY = (65.481 dr + 128.553 dg +
 *   24.966 db) / 255 with d. = q(preds.) - q(target.) (the difference is taken per channel, before the weights).
 * dsr_luma_pair: y_preds, y_target [N][1][h][w] fp32 = Y of the region of both images in one launch (h, w >= 11: they feed
 *   dsr_ssim_img_f32 with C = 1), and, if partial_sse is not NULL, the same partial sums in the same pass.
 * dsr_rgb_to_y: y [N][1][h][w] fp32 of one tensor.
 * dsr_luma_psnr_finalize: per_image[n] = 10 log10(h w / SSE_n) (+inf for SSE_n == 0), the partials of an image folded in a
 *   fixed order in double; value[0] = value_scale * sum_n per_image[n]; state (dsr_metric_accumulate's float64 pair): state[0]
 *   += sum_n per_image[n], state[1] += N.  per_image, value, state: each nullable, not all three.  No atomics anywhere. */
#define DSR_F32 2
int dsr_luma_blocks(int N, int H, int W, int shave);
int dsr_luma_sse_stats(int dtype_preds, const void* preds, int dtype_target, const void* target, int N, int C, int H, int W,
                       int shave, int quantize, float* partial_sse, dsr_stream_t s);
int dsr_luma_pair(int dtype_preds, const void* preds, int dtype_target, const void* target, int N, int C, int H, int W, int shave,
                  int quantize, float* y_preds, float* y_target, float* partial_sse, dsr_stream_t s);
int dsr_rgb_to_y(int dtype, const void* x, int N, int C, int H, int W, int shave, int quantize, float* y, dsr_stream_t s);
int dsr_luma_psnr_finalize(const float* partial_sse, int N, int H, int W, int shave, float* per_image, float* value,
                           float value_scale, double* state, dsr_stream_t s);

/* ------------------------------------------------------------------ feature-space loss taps (featloss.hip)
 * The content term of SRGAN / ESRGAN / Real-ESRGAN (perceptual.VggFeatureLoss, functional.FeatureTap): a distance between two
 * feature maps of a frozen trunk, taken on the 16-bit NHWC maps where they live.  f (generated image) and t (target) are
 * [P][Cp], P = N H W pixels, Cp = round_up(C, 8) with zero pad channels in BOTH maps (they then contribute nothing), dtype
 * DSR_BF16 or DSR_F16, 16-byte aligned.  mode: DSR_FEAT_L1 or DSR_FEAT_MSE.
 * dsr_featloss_blocks: the number of fp32 partials of one tap (the grid of dsr_pw_reduce_blocks(P); 0 for P == 0).
 * dsr_featloss_tap_fwd: partial[b] = block b's sum of |f - t| (L1) or (f - t)^2 (MSE), accumulated in fp32 from the 16-bit
 *   values; relu_out (nullable, [P][Cp]): max(f, 0) written in the same pass -- a tap BEFORE the activation feeds the next
 *   layer without a second read of the map.  Plain stores, no atomics: two calls on the same inputs give the same bits.
 * dsr_featloss_fold: value[0] = (float)(sum of the partials, in a fixed order, in double) / count; count = N C H W, the number
 *   of REAL elements, gives the unweighted mean.
 * dsr_featloss_tap_bwd: one launch and one rounding per element,
 *     df = (dnext ? dnext * m : 0) + g[0] * coef * d,
 *   d = sign(f - t) with sign(0) = 0 (L1) or 2 (f - t) (MSE); m = (f > 0) if masked (the forward wrote relu_out: the ReLU's
 *   backward rides here) else 1; dnext: the nullable 16-bit gradient arriving from the next layer; g: the device fp32 upstream
 *   gradient of this tap's mean; coef: a host float, 1 / (N C H W) times any scale the caller folds in.
 * dsr_featloss_relu: out = max(x, 0) on a map (the target's trunk behind a pre-activation tap).
 * dsr_featloss_combine: out[0] = sum_k weights[k] * values[k][0] over n <= 32 one-element device scalars (HOST tables, read
 *   before the call returns); dsr_featloss_combine_bwd: gout[k] = g[0] * weights[k], k < n.
 * A null required pointer, Cp % 8 != 0, P == 0 or an unknown mode returns DSR_E_ARG before anything is launched. */
#define DSR_FEAT_L1 0
#define DSR_FEAT_MSE 1
int dsr_featloss_blocks(size_t P);
int dsr_featloss_tap_fwd(int dtype, const void* f, const void* t, void* relu_out, size_t P, int Cp, int mode, float* partial,
                         dsr_stream_t s);
int dsr_featloss_fold(const float* partial, int blocks, float count, float* value, dsr_stream_t s);
int dsr_featloss_tap_bwd(int dtype, const void* f, const void* t, const void* dnext, const float* g, float coef, int mode,
                         int masked, void* df, size_t P, int Cp, dsr_stream_t s);
int dsr_featloss_relu(int dtype, const void* x, void* out, size_t P, int Cp, dsr_stream_t s);
int dsr_featloss_combine(int n, const float* const* values, const float* weights, float* out, dsr_stream_t s);
int dsr_featloss_combine_bwd(int n, const float* weights, const float* g, float* gout, dsr_stream_t s);

/* ------------------------------------------------------------------ style (Gram-matrix) term of the feature loss (featstyle.hip)
 * The texture half of the perceptual loss (perceptual.VggFeatureLoss(style_weight=), functional.FeatureStyleTap).  f is a
 * tapped map [N][HW][Cp] (NHWC, HW pixels per image, Cp = round_up(C, 8) with zero pad channels), DSR_BF16 or DSR_F16, 16-byte
 * aligned.  Limits of every entry point: Cp % 8 == 0, 1 <= C <= Cp <= 512, HW >= 1, N >= 1, N HW < 2^31.
 * dsr_gram_chunks(HW): the number of pixel chunks of one image, ceil(HW / 1024).  The chunk size is a constant of the kernel,
 *   so the summation order depends on the shape alone.  dsr_gram_workspace(N, HW, Cp): the fp32 ELEMENTS of the workspace,
 *   N * chunks * Cp * Cp (0 for a shape outside the limits).
 * dsr_gram_fwd: gram[N][C][C] (fp32) = scale * sum_p f[n][p][i] f[n][p][j]: MFMA with fp32 accumulation over the tile pairs on or
 *   above the diagonal, one fp32 slab per pixel chunk in the workspace, then the slabs are summed in chunk order and entry
 *   (i, j) and its mirror are written from the same sum: gram[n] is bit-symmetric.  No atomics: two calls give equal bits.
 * dsr_gram_loss: value[0] = (float)(sum crit(gram_f - gram_t) / (N C C)), crit = |.| (DSR_FEAT_L1) or (.)^2 (DSR_FEAT_MSE),
 *   accumulated in double in a fixed order; partial: DSR_GRAM_LOSS_PARTIALS * N doubles of scratch (per-slice sums and maxima;
 *   N <= 65535).  It also writes the operand of the
 *   backward GEMM, s16[N][Cp][Cp] in the map's dtype (pad rows and columns zero): sign(G - Gt) with sign(0) = 0 for L1 and
 *   s_scale[n] = 1; (G - Gt) / s_scale[n] with s_scale[n] = max |G - Gt| of image n for MSE (an all-zero difference gives
 *   s16 = 0, s_scale[n] = 1).  The entries are of order one, so fp16 neither overflows nor underflows.  A NaN or an Inf in
 *   G - Gt makes value[0] non-finite, leaves a non-finite entry in s16 in both modes (L1 stores it as it is and does not take
 *   the sign of an Inf) and, for MSE, is s_scale[n]: dsr_featstyle_tap_bwd then writes non-finite values into df of image n,
 *   and of image n alone.
 * dsr_featstyle_tap_bwd: one launch and one rounding per element,
 *     df[n][p][c] = (dnext ? dnext * m : 0) + g_content[0] * coef_content * d
 *                   + g_style[0] * coef_style * s_scale[n] * sum_i f[n][p][i] * s16[n][i][c],
 *   m, d, mode, masked, dnext as in dsr_featloss_tap_bwd; t and g_content are both null for a style-only tap.  coef_style is a
 *   host float that carries every scalar factor of the style gradient -- 2 scale / (N C C) for the symmetric D + D^T, times 2
 *   for MSE, times any loss scale the caller folds in -- so none of them is ever rounded to 16 bits.
 * A null required pointer, a shape outside the limits or an unknown mode returns DSR_E_ARG before anything is launched. */
#define DSR_GRAM_LOSS_SLICES 32
#define DSR_GRAM_LOSS_PARTIALS (2 * DSR_GRAM_LOSS_SLICES)
int dsr_gram_chunks(int HW);
size_t dsr_gram_workspace(int N, int HW, int Cp);
int dsr_gram_fwd(int dtype, const void* f, int N, int HW, int C, int Cp, float scale, float* workspace, float* gram, dsr_stream_t s);
int dsr_gram_loss(int dtype, const float* gram_f, const float* gram_t, int N, int C, int Cp, int mode, double* partial, float* value,
                  void* s16, float* s_scale, dsr_stream_t s);
int dsr_featstyle_tap_bwd(int dtype, const void* f, const void* t, const void* dnext, const float* g_content, float coef_content,
                          int mode, int masked, const void* s16, const float* s_scale, const float* g_style, float coef_style,
                          void* df, int N, int HW, int Cp, dsr_stream_t s);

/* ------------------------------------------------------------------ MATLAB-style antialiased resampling (imresize.hip)
 * y = W_h . x . W_w^T per plane in ONE launch: the H pass runs from global memory into an LDS strip, the W pass out of it; the
 * intermediate stays fp32 and never reaches HBM.  Per axis the caller passes DEVICE tables built on the host (utils/imresize.py:
 * float64 arithmetic, one rounding to fp32): idx [out][taps] 0-based source indices, already mirrored, and w [out][taps] fp32;
 * a padding entry carries weight 0 and a valid index (indices are clamped to the axis before use).  Per output and pass: one
 * fmaf per tap, in tap order, from 0; no atomics: the result is defined bit for bit.  The backward pass is the same call on dy
 * with the transposed tables (H, W = dy's size, OH, OW = dx's).
 * dsr_imresize_f32: x [planes][H][W] -> y [planes][OH][OW], fp32.
 * dsr_imresize_u8:  x [H][W][C] -> y [OH][OW][C], uint8; computed in fp32 from the bytes with no rounding between the passes,
 *   stored as min(max(floorf(v + 0.5f), 0), 255).
 * A null pointer, a size < 1 or planes * max(H W, OH OW) >= 2^31 is DSR_E_ARG; taps_h or taps_w outside 1..64 is
 * DSR_E_UNSUPPORTED; both before anything is launched.  A tile whose strip does not fit the LDS is computed from global memory
 * with the same arithmetic (same bits), never truncated. */
int dsr_imresize_f32(const float* x, float* y, int planes, int H, int W, int OH, int OW, const int* idx_h, const float* w_h,
                     int taps_h, const int* idx_w, const float* w_w, int taps_w, dsr_stream_t s);
int dsr_imresize_u8(const unsigned char* x, unsigned char* y, int H, int W, int C, int OH, int OW, const int* idx_h,
                    const float* w_h, int taps_h, const int* idx_w, const float* w_w, int taps_w, dsr_stream_t s);

/* ------------------------------------------------------------------ residual dense block on a growth buffer (conv_rdb.hip)
 * One 3x3 / stride 1 / zero-pad 1 convolution whose input is the channel PREFIX [0, Cin) of an NHWC tensor with pixel stride
 * ldx >= Cin, and whose Cout in {32, 64} outputs land at channel offset y_off of a tensor with pixel stride ldy -- the same
 * tensor for conv1..4 of a dense block (the concatenation is then free), another one for conv5:
 *     v = sum_taps sum_ci x[n, y+dy, x+dx, ci] * w[c, ci, dy, dx] + bias[c]       fp32 accumulation
 *     v = act(v)                       act: DSR_ACT_NONE, or DSR_ACT_LEAKY with slope > 0 (v >= 0 ? v : v * slope)
 *     if res1: v = fmaf(v, beta1, res1[n, y, x, r1_off + c]);   if res2: v = fmaf(v, beta2, res2[n, y, x, r2_off + c])
 *     y[n, y, x, y_off + c] = r16(v)                                               one rounding, to nearest even
 * w is the packed forward image [9][Cout][Cin] of dsr_conv_pack_weight.  Cin, every stride and every offset are multiples of
 * 32 channels.  bias, res1 and res2 may be NULL.  Within a launch no byte is both read and written: DSR_E_ARG (before anything
 * is launched) for a NULL x / w / y, a bad dtype, size, stride or offset, y_off + Cout > ldy (the same for the residuals),
 * an output range that overlaps the input prefix (y == x and y_off < Cin) or a residual range of the same tensor, a tensor
 * of 2^31 bytes or more per image or 2^32 bytes or more in total.  max_blocks <= 0: one persistent block per CU; > 0 caps the
 * grid.  dsr_conv_rdb_supported: non-zero when the shape fields (pointers are not looked at) describe a launch this kernel
 * takes; 0 for a NULL argument.  (A shape measured slower than the composed form -- dsr_conv_fwd on a concatenated copy --
 * would be refused here; tools/microbench_rrdb.py found none.) */
typedef struct {
  int dtype;               /* DSR_BF16 | DSR_F16 */
  int N, H, W;
  int Cin, Cout;
  const void* x;           /* [N][H][W][ldx], channels [0, Cin) are read */
  int ldx;
  const void* w;           /* [9][Cout][Cin] */
  const float* bias;       /* [Cout] or NULL */
  int act;
  float slope;
  const void* res1;        /* [N][H][W][ldr1] or NULL, channels [r1_off, r1_off + Cout) */
  int ldr1, r1_off;
  float beta1;
  const void* res2;
  int ldr2, r2_off;
  float beta2;
  void* y;                 /* [N][H][W][ldy], channels [y_off, y_off + Cout) are written */
  int ldy, y_off;
  int max_blocks;
} dsr_rdb_conv;
int dsr_conv_rdb_supported(const dsr_rdb_conv* c);
int dsr_conv_rdb_fwd(const dsr_rdb_conv* c, dsr_stream_t s);

/* Backward of a dense block on its growth buffers (conv_rdb.hip, conv_rdb_bwd.hip).  B is the block's forward buffer
 * [N][H][W][192] (x in [0, 64), x_k in [64 + 32 (k - 1), 64 + 32 k)), G a gradient buffer of B's shape.
 *
 * dsr_conv_rdb_dgrad, one 3x3 / stride 1 / pad 1 input gradient: the K in {32, 64} channels [dy_off, dy_off + K) of dy are
 * correlated with the mirrored kernel (wd: the dgrad image [9][Cout][K] of dsr_conv_pack_weight for a [K][Cout][3][3] weight),
 * giving Cout (a multiple of 32) channels that land in channels [0, Cout) of dx:
 *     v = scale * sum_taps sum_k dy[n, y-dy, x-dx, dy_off + k] * w[k, c, dy, dx]    products of 16-bit operands, fp32 sums
 *     if accumulate: v = v + dx[n, y, x, c]                                        (the 16-bit value already there)
 *     if c < g_limit: v = fmaf(g[n, y, x, c], g_scale, v)
 *     if c >= mask_lo: v = v * (act_out[n, y, x, c] >= 0 ? 1 : slope)              LeakyReLU mask from the stored OUTPUT
 *     dx[n, y, x, c] = r16(v)                                                      one rounding, to nearest even
 * dy may be dx itself (in place) when the ranges are disjoint, dy_off >= Cout: a tile's output bytes are read and written
 * only by the one block that owns the tile, and halo reads touch only the other channel range.  g and act_out are other
 * tensors than dx.  DSR_E_ARG before anything is launched for a NULL dy / wd / dx (or g with g_limit > 0, act_out with
 * mask_lo < Cout), a bad dtype, size, stride, offset or limit, overlapping ranges, a tensor of 2^31 bytes or more per image or
 * 2^32 bytes or more in total.  dsr_conv_rdb_dgrad_supported looks at the shape fields only. */
typedef struct {
  int dtype;               /* DSR_BF16 | DSR_F16 */
  int N, H, W;
  int K, Cout;
  const void* dy;          /* [N][H][W][lddy], channels [dy_off, dy_off + K) are read */
  int lddy, dy_off;
  const void* wd;          /* [9][Cout][K] */
  float scale;
  void* dx;                /* [N][H][W][lddx], channels [0, Cout) are written */
  int lddx;
  int accumulate;
  const void* g;           /* [N][H][W][ldg] or NULL, channels [0, g_limit) */
  int ldg, g_limit;
  float g_scale;
  const void* act_out;     /* [N][H][W][ldact] or NULL: the forward buffer, read in channels [mask_lo, Cout) */
  int ldact, mask_lo;      /* mask_lo == Cout: no mask */
  float slope;
  int max_blocks;
} dsr_rdb_dgrad;
int dsr_conv_rdb_dgrad_supported(const dsr_rdb_dgrad* c);
int dsr_conv_rdb_dgrad(const dsr_rdb_dgrad* c, dsr_stream_t s);

/* dsr_conv_rdb_wgrad: the ten parameter gradients of one dense block (num_feat 64, num_grow_ch 32) once dgrad_2 has run, i.e.
 * when channels [64, 192) of dy hold the masked dY_1 .. dY_4:
 *     dw[k][co, ci, i, j] = sum_{n,y,x} x[n, y+i-1, x+j-1, ci] * dY_{k+1}[n, y, x, co],  zero outside the image, ci < 64 + 32 k
 *     db[k][co] = sum_{n,y,x} dY_{k+1}[n, y, x, co]                    dY_5 = gscale * g (the factor is applied to the sums)
 * fp32, PyTorch layouts; a NULL dw[k] / db[k] is not computed.  Products of 16-bit operands, fp32 sums, the pixel range cut
 * into dsr_conv_rdb_wgrad_chunks() chunks whose partial sums are added in chunk order: no atomics, two runs give equal
 * bits.  The bias gradients come from a column-sum pass of their own inside the call.  workspace: device memory, 16-byte
 * aligned, dsr_conv_rdb_wgrad_workspace() bytes (too small: DSR_E_WORKSPACE); the queries return 0 for a shape the call
 * refuses (DSR_E_ARG: ldx or lddy other than 192, ldg < 64, sizes as above). */
typedef struct {
  int dtype;
  int N, H, W;
  const void* x;           /* B  [N][H][W][ldx] */
  int ldx;
  const void* dy;          /* G  [N][H][W][lddy] */
  int lddy;
  const void* g;           /* dL/dout [N][H][W][ldg], channels [0, 64) */
  int ldg;
  float gscale;
  float* dw[5];
  float* db[5];
} dsr_rdb_wgrad;
int dsr_conv_rdb_wgrad_supported(const dsr_rdb_wgrad* c);
size_t dsr_conv_rdb_wgrad_workspace(const dsr_rdb_wgrad* c);
int dsr_conv_rdb_wgrad_chunks(const dsr_rdb_wgrad* c);
int dsr_conv_rdb_wgrad(const dsr_rdb_wgrad* c, void* workspace, size_t workspace_bytes, dsr_stream_t s);
/* out = r16(fmaf(a, beta, b)) on nvec 16-byte vectors of 16-bit values; b may be NULL (out = r16(a * beta)); out may be a or b */
int dsr_scale_add16(int dtype, const void* a, float beta, const void* b, void* out, size_t nvec, dsr_stream_t s);

/* ------------------------------------------------------------------ spectral normalisation (spectral_norm.hip)
 * torch.nn.utils.spectral_norm(conv) with n_power_iterations = 1 for up to 64 layers per call.  HOST tables of `count`
 * entries: w[i] the fp32 weight viewed as [cout[i]][k[i]] row-major (k = Cin KH KW), u[i] [cout[i]], v[i] [k[i]], w_sn[i] the
 * output of w[i]'s shape (another buffer than w[i]); sigma: DEVICE fp32 [count]; ws: DEVICE workspace, 16-byte aligned, of
 * dsr_spectral_norm_workspace() bytes (0 for a bad shape table).
 *   training != 0:  t = W^T u;  v = t / max(|t|, eps);  s = W v;  u = s / max(|s|, eps);  sigma = u . s;  u and v are rewritten
 *   training == 0:  sigma = u . (W v); u and v are only read
 *   W_sn = W / sigma (a true division per element).
 * Four launches (two in eval mode) for the whole group, no host read, no atomics, every sum in a fixed order: the same state
 * gives the same bits, and a captured call advances the iteration on every replay.
 * dsr_spectral_norm_bwd: dw[i] = (g[i] - <g[i], w_sn[i]> u[i] v[i]^T) / sigma[i] with u, v, sigma, w_sn as that forward left
 * them (torch treats u and v as constants); two launches; ws of dsr_spectral_norm_bwd_workspace() bytes.
 * count outside 1..64, a null table / entry / sigma / ws, a cout or k below 1, a layer of 2^31 elements or more, a pointer off
 * its alignment or a workspace that is too small return DSR_E_ARG before anything is launched. */
size_t dsr_spectral_norm_workspace(int count, const int* cout, const int* k);
size_t dsr_spectral_norm_bwd_workspace(int count, const int* cout, const int* k);
int dsr_spectral_norm_fwd(int count, const float* const* w, float* const* u, float* const* v, const int* cout, const int* k,
                          int training, float eps, float* sigma, float* const* w_sn, float* ws, size_t ws_bytes, dsr_stream_t s);
int dsr_spectral_norm_bwd(int count, const float* const* g, const float* const* w_sn, const float* const* u,
                          const float* const* v, const int* cout, const int* k, const float* sigma, float* const* dw, float* ws,
                          size_t ws_bytes, dsr_stream_t s);

/* ------------------------------------------------------------------ GAN loss on logits (pointwise.hip)
 * BasicSR's GANLoss against a constant label, mean over the n fp32 logits x:
 *   DSR_GAN_VANILLA  BCEWithLogits: softplus(z) = max(z, 0) + log1p(exp(-|z|)), z = -x (target_is_real) or x
 *   DSR_GAN_LSGAN    (x - t)^2, t = 1 or 0
 *   DSR_GAN_HINGE    is_disc: relu(1 + z); otherwise -x (the generator's form, whatever the label)
 * loss[0] = the mean (elements added in double, in a fixed order, one rounding to fp32); grad[i] = d loss / d x[i].
 * partial: dsr_gan_loss_blocks(n) doubles of scratch.  Two launches, no host read, no atomics. */
#define DSR_GAN_VANILLA 0
#define DSR_GAN_LSGAN 1
#define DSR_GAN_HINGE 2
int dsr_gan_loss_blocks(size_t n);
int dsr_gan_loss(const float* x, size_t n, int kind, int target_is_real, int is_disc, float* grad, double* partial, float* loss,
                 dsr_stream_t s);

/* ------------------------------------------------------------------ relativistic average GAN loss on logits (ragan.hip)
 * ESRGAN's RaGAN term (BasicSR ESRGANModel.optimize_parameters): each of the n fp32 logits x is judged against the mean of
 * the m fp32 logits of the opposite class.  n and m are independent.
 *   rel(x[n], other[m], kind, target_is_real, is_disc)
 *     mu    = (sum_j other[j]) / m        added in double in a fixed order, rounded to fp32 ONCE
 *     z_i   = x_i - mu                    one fp32 subtraction
 *     loss  = (sum_i l(z_i)) / n          l = the per-element term of dsr_gan_loss for (kind, target_is_real, is_disc),
 *                                         evaluated in fp32 exactly as there, added in double, one rounding
 *     grad_x[i]     = l'(z_i) / n                          (optional output: null = not written)
 *     grad_other[j] = -(sum_i l'(z_i)) / (n m)   for all j (optional output; the sum in double, one rounding)
 * Every sum is thread-strided, then folded over the wave, the block and the blocks in block order: no atomics, no host
 * read, the same input gives the same bits.  Three launches, with or without the gradients, all on `s`.  ws: DEVICE scratch, 8-byte
 * aligned, of dsr_rel_gan_loss_workspace(n, m) bytes (0 for n == 0 or m == 0).  A null x / other / ws / loss, n == 0 or
 * m == 0, an unknown kind, a tensor off its 4-byte or ws off its 8-byte alignment return DSR_E_ARG before any launch. */
size_t dsr_rel_gan_loss_workspace(size_t n, size_t m);
int dsr_rel_gan_loss(const float* x, size_t n, const float* other, size_t m, int kind, int target_is_real, int is_disc,
                     float* grad_x, float* grad_other, void* ws, float* loss, dsr_stream_t s);

/* ------------------------------------------------------------------ LDL artifact-map loss (ldl.hip)
 * "Details or Artifacts: A Locally Discriminative Learning Approach" (CVPR 2022) as BasicSR's ldl_opt computes it (PARITY
 * UNPINNED: restated, the float64 statement is tests/ldl_ref.py).  x (the generator's output, which carries the gradient), gt
 * and e (the EMA generator's output): fp32 [N][C][H][W], contiguous.  k: the odd window, p = (k - 1) / 2, K = k k, M = N C H W.
 *   r[n,y,x]  = sum_c |gt - x|,  re = sum_c |gt - e|         fp32, in channel order
 *   mu, v     = mean and unbiased variance (/ (K - 1)) of r over the k x k window of the reflect-padded plane (the edge is not
 *               repeated), in two passes:  mu = r_q + (sum (r - r_q)) / K,  v = (sum (r - mu)^2) / (K - 1)
 *   V_n       = unbiased variance of r[n] over its H W values, from double sums shifted by r[n,0,0];  g_n = V_n^(1/5), formed in
 *               double and rounded to fp32 once
 *   m         = 0 where r < re, otherwise 1 (a tie keeps the weight; a NaN compares false and stays in the loss)
 *   w         = g_n v m                                        the artifact map [N][1][H][W] (optional output `map`)
 *   loss[0]   = (sum_n g_n S_n) / M,  S_n = sum m r v          in double, one rounding  (= mean |w x - w gt|, as w >= 0)
 *   dx[n,c,q] = sign(x - gt) dr[n,q] upstream[0],  sign(0) = 0:
 *     detach_weight:  dr = w / M
 *     otherwise:      dr = [ w + (2 / (K - 1)) g_n sum_{u in pre(q)} sum_{q' in window(u)} (m r)[q'] (r[q] - mu[q'])
 *                            + S_n (1/5) V_n^(-4/5) 2 (r - rbar_n) / (H W - 1) ] / M
 *     pre(q): q and its mirror images in the pad, window(u): the part of u's window inside the image (the adjoint of
 *     reflect-pad + box sum); the mask is a constant of the gradient.
 *   V_n == 0 (r constant): that image adds 0 to the loss, and its map and gradient are 0 (torch: 0 * inf = NaN).
 * dsr_ldl_fwd: two launches (tile pass, finalize); it leaves what dsr_ldl_bwd (one launch) needs in ws.  No atomics, no host
 * read (upstream is a DEVICE scalar), per-image sums are double block partials folded in a fixed order: the same input gives
 * the same bits.  ws: DEVICE scratch, 8-byte aligned, of dsr_ldl_workspace(N, C, H, W, k) bytes (0 for a shape the entry points
 * refuse).  A null pointer, k not odd in 3..11, H or W <= p, N C H W >= 2^31 or a misaligned pointer return DSR_E_ARG before
 * anything is launched. */
size_t dsr_ldl_workspace(int N, int C, int H, int W, int k);
int dsr_ldl_fwd(const float* x, const float* gt, const float* e, int N, int C, int H, int W, int k, void* ws, float* loss,
                float* map, dsr_stream_t s);
int dsr_ldl_bwd(const float* x, const float* gt, const void* ws, const float* upstream, int N, int C, int H, int W, int k,
                int detach_weight, float* dx, dsr_stream_t s);

/* ------------------------------------------------------------------ second-order Real-ESRGAN degradation
 * fp32 [B][C][H][W] batches in [0, 1] scaling; every call only enqueues on `s` (no allocation, no sync, no host read).
 *
 * dsr_filter2d_f32 (filter2d.hip), BasicSR's filter2D: a correlation with a kernel per sample, reflected borders,
 *   acc = 0;  for i, for j:  acc = fmaf(k[b][i][j], x[b][c][refl(Y + i - r)][refl(X + j - r)], acc),  r = ks / 2
 * one fmaf per tap in row-major tap order (taps whose weight is 0 may be left out: they add exact zeros), no atomics: the
 * result is defined bit for bit and does not depend on the tiling.  kernels: fp32 [B][ks][ks], or [ks][ks] for every sample
 * when shared == 1.  ks odd in 1..21, H, W >= ks / 2 + 1, B C H W < 2^31, y must not overlap x: otherwise DSR_E_ARG.
 *
 * dsr_noise_gaussian_f32 / dsr_noise_poisson_f32 (degrade_noise.hip), C == 3.  z: fp32 [B][3][H][W] and zg: fp32 [B][H][W]
 * draws made by the caller; gray: uint8 [B], non-zero = the sample takes zg for all three channels; sigma (0..255 units),
 * vals, scale: fp32 [B]; all on the device.  y may be x.
 *   Gaussian: y = clamp(fmaf(sigma[b] / 255, gray[b] ? zg : z, x), 0, 1)
 *   Poisson:  q = rintf(clamp(255 x, 0, 255)) / 255;  colour n = z / vals[b] - q;  grey n = zg / vals[b] - (0.2989 q_r + 0.587 q_g
 *             + 0.114 q_b, as one product and two fmaf);  y = clamp(fmaf(scale[b], n, x), 0, 1)
 *
 * dsr_usm_mask / dsr_usm_combine (degrade_noise.hip), the pointwise steps of the unsharp mask on n < 2^31 elements:
 *   mask = |x - blur| * 255 > threshold ? 1 : 0
 *   res = x - blur;  sharp = clamp(fmaf(weight, res, x), 0, 1);  y = fmaf(soft, sharp - x, x)
 * A null pointer or a size out of range is DSR_E_ARG before anything is launched. */
int dsr_filter2d_f32(const float* x, float* y, const float* kernels, int B, int C, int H, int W, int ks, int shared,
                     dsr_stream_t s);
int dsr_noise_gaussian_f32(const float* x, const float* z, const float* zg, const float* sigma, const unsigned char* gray,
                           float* y, int B, int H, int W, dsr_stream_t s);
int dsr_noise_poisson_f32(const float* x, const float* z, const float* zg, const float* vals, const float* scale,
                          const unsigned char* gray, float* y, int B, int H, int W, dsr_stream_t s);
int dsr_usm_mask(const float* x, const float* blur, float threshold, float* mask, size_t n, dsr_stream_t s);
int dsr_usm_combine(const float* x, const float* blur, const float* soft, float weight, float* y, size_t n, dsr_stream_t s);

/* ------------------------------------------------------------------ NIQE, the no-reference quality score (niqe.hip)
 * Mittal, Soundararajan, Bovik 2013 as BasicSR's calculate_niqe computes it (metrics.NaturalnessImageQualityEvaluator,
 * metrics.niqe_features; PARITY UNPINNED: restated, the float64 statement is tests/niqe_ref.py).
 * dsr_niqe_plane: x [N][3][H][W] of dtype DSR_BF16, DSR_F16 or DSR_F32 -> plane [N][hc][wc] fp32, hc = (H - 2 shave) / 96 * 96,
 *   wc likewise: per pixel of rows [shave, shave + hc), columns [shave, shave + wc) the 8-bit codes c = rintf(fminf(fmaxf(x, 0),
 *   1) * 255.0f) and Y = 16 + round_half_even((65481 r + 128553 g + 24966 b) / 255000) in integer arithmetic.  Fewer than two
 *   96 x 96 blocks, or N hc wc >= 2^31, is DSR_E_ARG.
 * dsr_niqe_moments: plane [N][hc][wc] fp32 with hc, wc multiples of block (96: scale 1; 48: scale 2, on the half-size plane);
 *   window: DEVICE fp64 [7][7].  In fp64, borders replicated, one separately rounded multiply and add per tap in row-major
 *   window order:  mu = w (*) x,  sigma = sqrt(|w (*) x^2 - mu^2|),  v = (x - mu) / (sigma + 1)  ((*): convolution, the window
 *   flipped).  Per block (row-major grid, nb = (hc / block)(wc / block)) and map m in { v, v roll(v,(0,1)), v roll(v,(1,0)),
 *   v roll(v,(1,1)), v roll(v,(1,-1)) } -- numpy's circular roll inside the block -- out [N][nb][5][5] fp64 holds
 *   count(m < 0), count(m > 0), sum of m^2 over m < 0, over m > 0, sum |m|.  Fixed summation order, no atomics.
 * dsr_niqe_features: m1, m2 = the moments of scale 1 and 2 over the same block grid; tables: DEVICE fp64 [3][9801] over alpha =
 *   arange(0.2, 10.001, 0.001): Gamma(2/a)^2 / (Gamma(1/a) Gamma(3/a)) (strictly increasing), sqrt(Gamma(1/a) / Gamma(3/a)),
 *   Gamma(2/a) / Gamma(1/a).  feat [N][nb][36] fp64: per scale (1 first) [alpha, (beta_l + beta_r) / 2] of v and [alpha,
 *   (beta_r - beta_l) Gamma(2/alpha) / Gamma(1/alpha), beta_l, beta_r] of each product; alpha is written as 0.2 + 0.001 index,
 *   the index that of np.argmin((table - r_norm)^2), 0 when r_norm is not finite (a map with no negative or no positive value).
 * A null pointer or a size out of range is DSR_E_ARG before anything is launched. */
int dsr_niqe_plane(int dtype, const void* x, int N, int C, int H, int W, int shave, float* plane, dsr_stream_t s);
int dsr_niqe_moments(const float* plane, int N, int hc, int wc, int block, const double* window, double* out, dsr_stream_t s);
int dsr_niqe_features(const double* m1, const double* m2, int N, int nb, const double* tables, double* feat, dsr_stream_t s);

/* ------------------------------------------------------------------ SRVGGNetCompact (conv_compact.hip, pw_compact.hip)
 * BasicSR's compact generator (models/GAN/srvgg.py; PARITY UNPINNED, the float64 statement is tests/compact_ref.py).
 *
 * dsr_conv_prelu_c_fwd, a body layer: 3x3 / stride 1 / zero-pad 1 from x [N][H][W][64] (16-bit) to y [N][H][W][64] with a
 * per-channel PReLU, nn.PReLU(num_parameters=64).  w: the packed forward image [9][64][64] of dsr_conv_pack_weight; bias: fp32
 * [64] or NULL; slope: fp32 [64] ON THE DEVICE, read by every launch (a HIP-graph replay after an optimiser step uses the new
 * slopes), or NULL for no activation:
 *     v = sum_taps sum_ci x[n, y+dy, x+dx, ci] * w[c, ci, dy, dx] + bias[c]       fp32 accumulation
 *     v = v > 0 ? v : v * slope[c]                                                 any sign of slope
 *     y[n, y, x, c] = r16(v)                                                       one rounding, to nearest even
 * dsr_conv_shuffle_add_fwd, the tail: the same convolution to Q = C s^2 outputs (s, C in 1..4), stored through PixelShuffle(s)
 * with the fp32 image `base` [N][C][H][W] (or NULL) added per LR pixel; w: [9][r8(Q)][64], whose pad rows are never stored;
 * bias: fp32 [Q] or NULL; out: fp32 [N][C][s H][s W]:
 *     v = sum_taps sum_ci x * w[q] + bias[q];  v = v + base[n, c, y, x];  out[n, c, s y + i, s x + j] = v,  q = c s^2 + i s + j
 * in fp32 with no 16-bit rounding.
 * Both: DSR_E_ARG before anything is launched for a NULL x / w / y (out), a bad dtype, N, H or W < 1, an output range that
 * overlaps x (or base), a tensor of 2^31 bytes or more per image or 2^32 or more in total; s or C outside 1..4 is
 * DSR_E_UNSUPPORTED.  max_blocks <= 0: one persistent block per CU; > 0 caps the grid (same bits for every value).  The
 * _supported queries look at the shape fields only; 0 for a NULL argument. */
typedef struct {
  int dtype;               /* DSR_BF16 | DSR_F16 */
  int N, H, W;
  const void* x;           /* [N][H][W][64] */
  const void* w;           /* [9][64][64] */
  const float* bias;       /* [64] or NULL */
  const float* slope;      /* [64] or NULL */
  void* y;                 /* [N][H][W][64] */
  int max_blocks;
} dsr_compact_conv;
int dsr_conv_prelu_c_supported(const dsr_compact_conv* c);
int dsr_conv_prelu_c_fwd(const dsr_compact_conv* c, dsr_stream_t s);
typedef struct {
  int dtype;
  int N, H, W;
  int C, s;
  const void* x;           /* [N][H][W][64] */
  const void* w;           /* [9][r8(C s^2)][64] */
  const float* bias;       /* [C s^2] or NULL */
  const float* base;       /* [N][C][H][W] or NULL */
  float* out;              /* [N][C][s H][s W] */
  int max_blocks;
} dsr_compact_tail;
int dsr_conv_shuffle_add_supported(const dsr_compact_tail* c);
int dsr_conv_shuffle_add_fwd(const dsr_compact_tail* c, dsr_stream_t s);

/* Pointwise pieces of the composed (training) form.  z, y, dy, dz: 16-bit NHWC [P][Cp], Cp a multiple of 8; slope: fp32 [C],
 * C <= Cp (pad channels take slope 0).
 *     dsr_pw_prelu_c_fwd:  y = r16(z > 0 ? z : z * slope[c])
 *     dsr_pw_prelu_c_bwd:  dz = r16(dy * (z > 0 ? 1 : slope[c]));  dslope[c] = sum_p dy * z * [z <= 0]     (torch's rules at 0)
 * The mask comes from the stored pre-activation z, so every slope is exact.  partial: fp32 [dsr_pw_prelu_c_rows(P)][Cp]
 * scratch, row r the sum over one pixel range; dslope [C] adds the rows in a fixed order (dsr_pw_prelu_c_fold_width() rows
 * side by side): no atomics, two runs give equal bits.  partial and dslope are both NULL (no slope gradient) or both given.
 * dsr_shuffle_add_f32: out[n][c][s y + i][s x + j] = t[n][c s^2 + i s + j][y][x] + base[n][c][y][x] (base may be NULL), fp32.
 * dsr_shuffle_add_bwd_f32: dt = the un-shuffle of dout; dbase (or NULL) [n][c][y][x] = sum_{i, j} dout[...], i then j.
 * A NULL required pointer or a size out of range (s outside 1..4, 2^31 elements or more) is DSR_E_ARG before any launch. */
int dsr_pw_prelu_c_fwd(int dtype, const void* z, const float* slope, void* y, size_t P, int C, int Cp, dsr_stream_t s);
int dsr_pw_prelu_c_rows(size_t P);
int dsr_pw_prelu_c_fold_width(void);
int dsr_pw_prelu_c_bwd(int dtype, const void* dy, const void* z, const float* slope, void* dz, size_t P, int C, int Cp,
                       float* partial, float* dslope, dsr_stream_t s);
int dsr_shuffle_add_f32(const float* t, const float* base, float* out, int N, int C, int s, int H, int W, dsr_stream_t st);
int dsr_shuffle_add_bwd_f32(const float* dout, float* dt, float* dbase, int N, int C, int s, int H, int W, dsr_stream_t st);

#ifdef __cplusplus
}
#endif
#endif
