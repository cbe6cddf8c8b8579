/*
 * pwg_kernels.h -- C ABI of libpwgkernels.so, the MI355X (gfx950) kernel library
 * behind the ParallelWaveGAN-compatible Python surface in parallelwavegan_amd/.
 *
 * The reference (kan-bayashi/ParallelWaveGAN) has no native code: every FLOP of
 * its hot path is an ATen op called from Python.  Each entry
 * point below therefore replaces an ATen *call site* in the reference; the
 * file:line of that call site (relative to /root/reference/) is cited on every
 * declaration.  A maintainer binds these with ctypes.
 *
 * Conventions
 *   - plain C: raw device pointers (fp32, contiguous NCW), ints, floats; no
 *     torch types.  `stream` is a hipStream_t passed as void*.
 *   - the library allocates nothing; every buffer incl. packed weights and
 *     workspaces is owned by the caller.
 *   - every launch goes to `stream`; no implicit device synchronisation.
 *   - return value: PWG_OK (0) or a negative pwg_status; pwg_last_error()
 *     returns a thread-local human-readable message for the last failure.
 */
#ifndef PWG_KERNELS_H_
#define PWG_KERNELS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum pwg_status {
  PWG_OK = 0,
  PWG_ERR_BAD_SHAPE = -1,   /* inconsistent sizes in a descriptor            */
  PWG_ERR_UNSUPPORTED = -2, /* valid request this build has no kernel for     */
  PWG_ERR_LAUNCH = -3,      /* hipLaunchKernel / hipGetLastError failed        */
  PWG_ERR_NULL = -4,        /* required pointer is NULL                        */
  PWG_ERR_WORKSPACE = -5    /* workspace too small                             */
} pwg_status;

const char* pwg_last_error(void);
/* ABI version: bumped on any signature change. */
int pwg_abi_version(void);
/* Returns 950 (the only ISA this library is built for). */
int pwg_target_arch(void);

/* ------------------------------------------------------------------------- */
/* Per-launch timing (measurement support).  While enabled, every */
/* kernel launched through this ABI is bracketed by hipEvents recorded on the   */
/* stream it is launched on; totals are kept per kernel family together with     */
/* the ALGORITHMIC flops/bytes of the launches (not hardware counters).          */
/* pwg_prof_get/_num_kernels synchronise the recorded events.                     */
/* ------------------------------------------------------------------------- */
int pwg_prof_enable(int on);
int pwg_prof_reset(void);
int pwg_prof_num_kernels(void);
int pwg_prof_get(int32_t idx, char* name, size_t name_cap, double* total_ms, int64_t* launches,
                 double* flops, double* bytes);

/* Concurrency hint for the tile / split heuristics of the convolution kernels: the fraction of the chip ONE launch
 * should aim to fill (1.0 = it runs alone, the default; 0.5 = about two launches run concurrently, e.g. the parallel
 * sub-discriminator branches of a captured training step, so fewer but more efficient tiles win).  Process-wide;
 * values outside (0, 1] are ignored; returns the previous value.  Measured on the HiFi-GAN V1 step: +2.7 %.      */
float pwg_set_concurrency_hint(float fill_scale);

/* Debugging aid (tests): while on, every CU's LDS is filled with NaN bit patterns before each MFMA    */
/* kernel launched through this ABI, so that a result depending on LDS nobody wrote (0 * stale tile      */
/* element in a contraction) turns non-finite deterministically.  Same as the environment variable       */
/* PWG_POISON_LDS=1, switchable at run time; returns the previous setting.                                */
int pwg_debug_poison_lds(int on);

/* ------------------------------------------------------------------------- */
/* Activations / padding selectors                                            */
/* ------------------------------------------------------------------------- */
enum { PWG_ACT_NONE = 0, PWG_ACT_LEAKY_RELU = 1, PWG_ACT_TANH = 2, PWG_ACT_RELU = 3 };
enum { PWG_PAD_ZERO = 0, PWG_PAD_REFLECT = 1, PWG_PAD_REPLICATE = 2 };

/* ------------------------------------------------------------------------- */
/* 1-D convolution family                                                     */
/*                                                                            */
/* One descriptor covers every convolution on the hot path:                   */
/*   - torch.nn.Conv1d (dilated / strided / grouped), e.g.                    */
/*       layers/residual_block.py:190-196,213-220  (HiFi-GAN MRF)             */
/*       layers/residual_block.py:78-86             (PWG dilated gate conv)   */
/*       models/hifigan.py:75-81,143-149            (input / output conv)     */
/*       models/hifigan.py:516-568                  (MSD grouped strided)     */
/*       layers/residual_stack.py:47-55             (MelGAN stack, reflect)   */
/*   - torch.nn.ConvTranspose1d, computed polyphase (transposed = 1):         */
/*       models/hifigan.py:99-107, models/melgan.py:93-101                    */
/*   - torch.nn.Conv2d with (k,1) kernels on the period-folded view           */
/*       (width = period): models/hifigan.py:314-341                          */
/*                                                                            */
/* Fused around the contraction (all optional):                               */
/*   y = post_act( (conv(pre_act(pad(x)), w) + bias + add1 + add2) * out_mul  */
/*                  / out_div )                                               */
/* which is how `x = xt + x` (residual_block.py:257), the MRF `cs += ...;     */
/* c = cs / num_blocks` (hifigan.py:186-190) and the final Tanh               */
/* (hifigan.py:150) disappear into the producing kernel.                      */
/* ------------------------------------------------------------------------- */
typedef struct pwg_conv1d_desc {
  int32_t batch;
  int32_t c_in;       /* total input channels                                 */
  int32_t c_out;      /* total output channels                                */
  int32_t t_in;       /* input length  (rows H for the (k,1) Conv2d case)     */
  int32_t t_out;      /* output length (rows H_out)                           */
  int32_t width;      /* 1 for Conv1d; the period p for (k,1) Conv2d          */
  int32_t kernel;     /* taps                                                 */
  int32_t stride;
  int32_t dilation;
  int32_t pad_left;   /* implicit padding on the left (zeros/reflect/...)     */
  int32_t groups;
  int32_t transposed; /* 0: Conv1d semantics, 1: ConvTranspose1d semantics    */
                      /*    (stride = upsampling factor, pad_left = `padding`)*/
  int32_t pad_mode;   /* PWG_PAD_*  (reflect/replicate only for width==1)     */
  int32_t pre_act;    /* PWG_ACT_NONE | LEAKY_RELU | RELU applied to x        */
  float pre_slope;
  int32_t post_act;   /* PWG_ACT_* applied to the result                      */
  float post_slope;
  float out_mul;      /* 1.0f = off                                           */
  float out_div;      /* 1.0f = off  (true IEEE division, matches `cs / 3`)   */
} pwg_conv1d_desc;

/* Number of floats of the packed weight image for `d` (forward direction). */
size_t pwg_conv1d_packed_weight_floats(const pwg_conv1d_desc* d);

/* Re-layout a torch-format weight into the kernel's [group][tap][ci][M] image.
 *   transposed == 0: w is (c_out, c_in/groups, kernel)   [torch Conv1d]
 *   transposed == 1: w is (c_in, c_out/groups, kernel)   [torch ConvTranspose1d]
 * `scale` (optional, may be NULL) holds one multiplier per dim-0 slice of w,
 * i.e. g/||v|| of old-style weight_norm (see pwg_weight_norm_scale), so that
 * weight_norm + pack is one pass.                                             */
int pwg_conv1d_pack_weight(const pwg_conv1d_desc* d, const float* w, const float* scale,
                           float* w_packed, void* stream);

/* y = fused conv forward (see above).  bias/add1/add2 may be NULL; y must not alias any input.
 * x: (batch, c_in, t_in*width)  y/add1/add2: (batch, c_out, t_out*width).
 * workspace (optional, may be NULL/0): launches that cannot fill the chip but have a long
 * reduction (e.g. 1024 channels over 9..110 columns per item) are run as 2/4/8 reduction
 * slices of a bigger tile; each slice writes a y-shaped slab of `workspace` and a second kernel
 * sums the slabs in slice order and applies the fused terms (deterministic).  Query the size
 * (floats, 0 = not needed) first; without a workspace the launch runs unsplit.              */
size_t pwg_conv1d_forward_workspace_floats(const pwg_conv1d_desc* d);
int pwg_conv1d_forward(const pwg_conv1d_desc* d, const float* x, const float* w_packed,
                       const float* bias, const float* add1, const float* add2, float* y,
                       float* workspace, size_t workspace_floats, void* stream);

/* ---- backward (training; replaces ATen convolution_backward at the same call sites) ---- */
/* Weight image for the data-gradient direction (the dual convolution).          */
size_t pwg_conv1d_packed_weight_bwd_floats(const pwg_conv1d_desc* d);
int pwg_conv1d_pack_weight_bwd(const pwg_conv1d_desc* d, const float* w, const float* scale,
                               float* w_packed_bwd, void* stream);
/* ---- weight bank (round 4): the weight preparation of a whole model in two launches ----
 * Replaces the per-layer sequence pwg_weight_norm_scale + pwg_conv1d_pack_weight + pwg_conv1d_pack_weight_bwd
 * (i.e. the reference's per-layer weight-norm hook, torch/nn/utils/weight_norm.py `_weight_norm`, evaluated before
 * every F.conv1d call of the layers/ and models/ modules) by ONE row-scale launch and ONE packing launch over a device table.
 * pwg_weight_bank_build fills a HOST table (pwg_weight_bank_table_bytes(n) bytes) and `info[8]`; the caller copies
 * the table to the device once and passes that copy to pwg_weight_bank_prepare, whose launches have constant
 * arguments (hipGraph-capturable).  Results are bit-identical to the per-layer entry points.
 * item: w = weight / weight_v (torch layout), g = weight_g or NULL, scale = n0 floats (iff g), fwd / bwd = images of
 * pwg_conv1d_packed_weight_floats / _bwd_floats floats (NULL: not built), desc = any descriptor of the layer.   */
typedef struct pwg_bank_item {
  const float* w;
  const float* g;
  float* scale;
  float* fwd;
  float* bwd;
  pwg_conv1d_desc desc;
} pwg_bank_item;
size_t pwg_weight_bank_table_bytes(int32_t n_items);
int pwg_weight_bank_build(const pwg_bank_item* items, int32_t n_items, void* table_host, size_t table_bytes,
                          int32_t* info);
int pwg_weight_bank_prepare(const void* table_dev, const int32_t* info, int32_t with_bwd, void* stream);

/* dx = d(pre_act)/dx(x) * conv_data_grad(dy) + accum.  `d` is the FORWARD descriptor
 * (its post_act/out_mul/out_div are NOT differentiated here: the caller passes the gradient
 * w.r.t. the pre-post_act, pre-scale result).  x: forward input (may be NULL when
 * pre_act == NONE); accum: optional tensor added to the result (gradient accumulation);
 * it must NOT alias dx (the kernels treat outputs as restrict).  workspace: as for
 * pwg_conv1d_forward (split reduction), sized by the query below.                    */
size_t pwg_conv1d_backward_data_workspace_floats(const pwg_conv1d_desc* d);
int pwg_conv1d_backward_data(const pwg_conv1d_desc* d, const float* dy, const float* w_packed_bwd,
                             const float* x, const float* accum, float* dx, float* workspace,
                             size_t workspace_floats, void* stream);
/* dw (torch layout, same shape as the forward weight) = sum_{b,t} dy * pre_act(x) taps;
 * db[c] = sum dy.  The (batch, time) reduction is cut into slices that each write a private
 * slab of `workspace`; a second kernel sums the slabs (deterministic, no atomics).  For plain
 * convolutions the bias gradient is produced by the same launch (row sums of the dy tiles the
 * kernel stages anyway).  Query the workspace size (floats, may be 0) first.  Either of dw/db
 * may be NULL.                                                                      */
size_t pwg_conv1d_backward_weight_workspace_floats(const pwg_conv1d_desc* d);
int pwg_conv1d_backward_weight(const pwg_conv1d_desc* d, const float* x, const float* dy, float* dw,
                               float* db, float* workspace, size_t workspace_floats, void* stream);

/* Weight-normalised layers (old-style torch.nn.utils.weight_norm, dim 0: every conv of the generators and
 * discriminators): the same weight-gradient kernel, but the finishing kernel turns the reduction slabs
 * directly into dv and dg  (dg = <dw, v> / |v|,  dv = (g / |v|)(dw - v <dw, v> / |v|^2))  -- dw is never
 * materialised and the separate slab-reduction and weight-norm-backward launches disappear.  v / g: the
 * layer's weight_v (torch weight layout) and weight_g; db optional as above.  The workspace is mandatory. */
size_t pwg_conv1d_backward_weight_wn_workspace_floats(const pwg_conv1d_desc* d);
int pwg_conv1d_backward_weight_wn(const pwg_conv1d_desc* d, const float* x, const float* dy, const float* v,
                                  const float* g, float* dv, float* dg, float* db, float* workspace,
                                  size_t workspace_floats, void* stream);

/* Tuning / diagnostics: the same operation with an explicit tile configuration
 * (0 <= tile_config < pwg_conv1d_num_tile_configs()) and staging path (use_dma:
 * 1 = LDS-DMA double-buffered, 0 = register-staged).  tools/bench_conv.py sweeps
 * these to derive the heuristic inside pwg_conv1d_forward; results are identical
 * for every configuration up to fp32 summation order.                          */
int pwg_conv1d_num_tile_configs(void);
int pwg_conv1d_forward_cfg(const pwg_conv1d_desc* d, const float* x, const float* w_packed,
                           const float* bias, const float* add1, const float* add2, float* y,
                           int32_t tile_config, int32_t use_dma, void* stream);

/* ---- bf16-operand inference (opt-in; csrc/conv1d_bf16.hip) ----
 * The same fused convolution at the same call sites as pwg_conv1d_forward (layers/residual_block.py:190-196,213-220,
 * models/hifigan.py:75-81,99-107,143-149: F.conv1d / F.conv_transpose1d under torch.no_grad(), bin/decode.py:158-169),
 * with bf16 OPERANDS on the gfx950 bf16 MFMA instructions.  Numerical definition:
 *   1. pre_act is applied to the fp32 input in fp32;  2. the activated input is rounded to bf16 (nearest-even);
 *   3. the effective fp32 weight (w * scale) is rounded to bf16 once, by the packer;  4. products are accumulated in fp32;
 *   5. bias, add1, add2, out_mul, out_div, post_act and the stored result are fp32.
 * Tensors stay fp32 in memory.  Covered: groups == 1, width == 1, zero padding, and either stride-1 Conv1d (any kernel /
 * dilation whose window fits LDS) or ConvTranspose1d with kernel == 2 * stride; pwg_conv1d_bf16_supported is pure host
 * logic (no device needed; pwg_last_error names the reason for 0).  Deterministic (no split reduction, no atomics).
 * Inference only: there is no backward.  `scale` as for pwg_conv1d_pack_weight; the image is
 * pwg_conv1d_bf16_packed_weight_bytes bytes (0 = unsupported), 16-B aligned.  pwg_conv1d_bf16_forward takes the arguments
 * of pwg_conv1d_forward in the same order (the workspace is never used and may be NULL / 0).
 * pwg_conv1d_bf16_forward_cfg (tuning): mfma_shape 32 = 32x32x16, 16 = 16x16x32 at the same output tile.              */
int pwg_conv1d_bf16_supported(const pwg_conv1d_desc* d);
size_t pwg_conv1d_bf16_packed_weight_bytes(const pwg_conv1d_desc* d);
int pwg_conv1d_bf16_pack_weight(const pwg_conv1d_desc* d, const float* w, const float* scale, void* w_packed,
                                void* stream);
int pwg_conv1d_bf16_forward(const pwg_conv1d_desc* d, const float* x, const void* w_packed, const float* bias,
                            const float* add1, const float* add2, float* y, float* workspace, size_t workspace_floats,
                            void* stream);
int pwg_conv1d_bf16_forward_cfg(const pwg_conv1d_desc* d, const float* x, const void* w_packed, const float* bias,
                                const float* add1, const float* add2, float* y, int32_t mfma_shape, void* stream);

/* ---- split-operand inference (fp32-accurate on the bf16 matrix pipe; csrc/conv1d_split.hip) ----
 * The fused convolution of pwg_conv1d_forward for stride-1 Conv1d, groups == 1, width == 1, zero padding, forward only,
 * computed on the gfx950 bf16 MFMA instructions from operands split three ways.  Numerical definition:
 *   1. pre_act is applied to the fp32 input in fp32;
 *   2. an fp32 value v (activated input; effective weight w * scale, split once by the packer) is split exactly as
 *      hi = bf16_rne(v), r = v - float(hi), mid = bf16_rne(r), lo = bf16_rne(r - float(mid)), v == hi + mid + lo;
 *   3. per operand pair the six products lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi (weight part . input part) are
 *      accumulated in this order in fp32 by the MFMA; each dropped product is <= 2^-24 of the full product (about 2^-28 on average);
 *   4. bias, add1, add2, out_mul, out_div, post_act and the stored result are fp32.
 * Non-finite inputs give non-finite outputs (an inf may come out as NaN).  Deterministic (no split reduction, no
 * atomics; the accumulation order of an element does not depend on tile or grid).  pwg_conv1d_split_supported is pure
 * host logic (no device needed; pwg_last_error names the reason for 0).  The image is
 * pwg_conv1d_split_packed_weight_bytes bytes (0 = unsupported), 16-B aligned: three images of the bf16 layout.
 * pwg_conv1d_split_forward takes the arguments of pwg_conv1d_forward in the same order (the workspace is never used and
 * may be NULL / 0).  pwg_conv1d_split_forward_cfg (tuning / tests): mfma_shape 32 = 32x32x16, 16 = 16x16x32 at the same
 * output tile; tile_mode 0 = the small-grid rule decides, 1 = full-size tiles (where they fit LDS), 2 = half-size tiles
 * (same bits).                                                                                                       */
int pwg_conv1d_split_supported(const pwg_conv1d_desc* d);
size_t pwg_conv1d_split_packed_weight_bytes(const pwg_conv1d_desc* d);
int pwg_conv1d_split_pack_weight(const pwg_conv1d_desc* d, const float* w, const float* scale, void* w_packed,
                                 void* stream);
int pwg_conv1d_split_forward(const pwg_conv1d_desc* d, const float* x, const void* w_packed, const float* bias,
                             const float* add1, const float* add2, float* y, float* workspace, size_t workspace_floats,
                             void* stream);
int pwg_conv1d_split_forward_cfg(const pwg_conv1d_desc* d, const float* x, const void* w_packed, const float* bias,
                                 const float* add1, const float* add2, float* y, int32_t mfma_shape, int32_t tile_mode,
                                 void* stream);
/* The form of the kernel's reduction step (additive; pwg_abi_version() stays 15).  Resident: a step loads all its
 * weight fragments, then issues its MFMAs.  Streamed: the fragments are requested a row tile ahead of their MFMAs, across
 * taps and chunks.  Same products in the same order: same bits.  The launch plan chooses per class (input channels,
 * taps); pwg_conv1d_split_step_form answers that choice for a descriptor -- 1 resident, 2 streamed, 0 unsupported
 * (pwg_last_error names the reason) -- as pure host logic.  pwg_conv1d_split_forward_step (tests / A-B tools) is
 * pwg_conv1d_split_forward_cfg plus step_form: 0 = the plan decides, 1 = resident, 2 = streamed.                       */
int pwg_conv1d_split_step_form(const pwg_conv1d_desc* d);
int pwg_conv1d_split_forward_step(const pwg_conv1d_desc* d, const float* x, const void* w_packed, const float* bias,
                                  const float* add1, const float* add2, float* y, int32_t mfma_shape, int32_t tile_mode,
                                  int32_t step_form, void* stream);
/* The form of the kernel's window staging (additive; pwg_abi_version() stays 15): a second axis beside the step form.
 * Staged: a chunk's 16-B loads are issued, waited for, split and written to the LDS planes between the two barriers of the
 * chunk.  Prefetched: the raw fp32 window of chunk n + 1 is requested by LDS-DMA in front of the tap loop of chunk n, into
 * a region of LDS beside the planes, and split from there behind it (resident step, 16-B staging: t_in % 4 == 0, x 16-B
 * aligned).  Same values to the same plane addresses: same bits.  pwg_conv1d_split_window_form answers the launch plan's
 * choice for a descriptor -- 1 staged, 2 prefetched, 0 unsupported (pwg_last_error names the reason) -- as pure host
 * logic.  pwg_conv1d_split_forward_window (tests / A-B tools) is pwg_conv1d_split_forward_step plus window_form: 0 = the
 * plan decides, 1 = staged, 2 = prefetched; a 2 on a launch the form does not cover (no 16-B staging, the streamed step
 * named with it, LDS) is refused with a message and launches nothing.                                               */
int pwg_conv1d_split_window_form(const pwg_conv1d_desc* d);
int pwg_conv1d_split_forward_window(const pwg_conv1d_desc* d, const float* x, const void* w_packed, const float* bias,
                                    const float* add1, const float* add2, float* y, int32_t mfma_shape,
                                    int32_t tile_mode, int32_t step_form, int32_t window_form, void* stream);

/* ---- split-operand inference of the upsampling layers (csrc/conv1d_split.hip, convtr1d_split_mfma_kernel) ----
 * The fused transposed convolution of pwg_conv1d_forward at the ConvTranspose1d call site of the HiFi-GAN generator
 * (models/hifigan.py:184-185: `c = self.upsamples[i](c)`, LeakyReLU + ConvTranspose1d with kernel == 2 * stride,
 * under torch.no_grad(), bin/decode.py:158-169), computed under the numerical definition of the split-operand inference above, points 1 - 4 word for
 * word.  Covered: transposed descriptors with kernel == 2 * stride (any stride, odd ones included), groups == 1,
 * width == 1, zero padding, forward only; a stride-1 descriptor is refused (it belongs to pwg_conv1d_split_*), and
 * pwg_conv1d_split_supported keeps refusing transposed ones.  The contraction is the polyphase one of the bf16 kernel
 * (rows co * stride + phase, two taps); the image is three parts of the bf16 kernel's transposed image
 * (pwg_convtr1d_split_packed_weight_bytes == 3 x pwg_conv1d_bf16_packed_weight_bytes), `scale` per INPUT channel as
 * torch lays out a ConvTranspose1d weight.  Output samples are written 16 B at a time when stride % 4 == 0,
 * padding % 4 == 0, t_out % 4 == 0 and y / add1 / add2 are 16-B aligned, else 4 B at a time; samples outside
 * [0, t_out) are never written.  Deterministic; the accumulation order of an element is that of
 * pwg_conv1d_split_forward on the stride-1 twin of the layer (kernel 2, pad_left 1, rows co * stride + phase), so the
 * two agree bit for bit.  pwg_convtr1d_split_supported is pure host logic (pwg_last_error names the reason for 0).
 * pwg_convtr1d_split_forward takes the arguments of pwg_conv1d_forward (the workspace is never used);
 * pwg_convtr1d_split_forward_cfg (tuning / tests): mfma_shape and tile_mode as for pwg_conv1d_split_forward_cfg.     */
int pwg_convtr1d_split_supported(const pwg_conv1d_desc* d);
size_t pwg_convtr1d_split_packed_weight_bytes(const pwg_conv1d_desc* d);
int pwg_convtr1d_split_pack_weight(const pwg_conv1d_desc* d, const float* w, const float* scale, void* w_packed,
                                   void* stream);
int pwg_convtr1d_split_forward(const pwg_conv1d_desc* d, const float* x, const void* w_packed, const float* bias,
                               const float* add1, const float* add2, float* y, float* workspace,
                               size_t workspace_floats, void* stream);
int pwg_convtr1d_split_forward_cfg(const pwg_conv1d_desc* d, const float* x, const void* w_packed, const float* bias,
                                   const float* add1, const float* add2, float* y, int32_t mfma_shape,
                                   int32_t tile_mode, void* stream);

/* ---- stateful streaming form of the causal convolutions (fp32; csrc/conv1d_stream.hip; ABI v14) ----
 * The causal layers of the reference -- CausalConv1d.forward, layers/causal_conv.py:32-42 (`self.conv(self.pad(x))
 * [:, :, :x.size(2)]`), and CausalConvTranspose1d.forward, :68-78 (`self.deconv(self.pad(x))[:, :, self.stride :
 * -self.stride]`) -- evaluated on one CHUNK of a stream: x (batch, c_in, n) are the n new columns (d->t_in = n), the
 * columns before them come from hist_in (batch, c_in, H), H = (kernel - 1) * dilation (1 for the transposed form).  The
 * same launch writes y (batch, c_out, n), or n * stride for the transposed form (d->t_out), and hist_out (batch, c_in, H)
 * = the last H columns of concat(hist_in, x), also when n < H.  History is the RAW input: pre_act is applied while the
 * window is staged, to both sources alike.  hist_in == NULL: start of stream, the left context is what pad_mode gives
 * (zero / reflect, which needs n > H / replicate; the transposed form: replicated first column, or zero).  hist_in and
 * hist_out must be distinct buffers (ping-pong).  The fused epilogue is pwg_conv1d_forward's; w_packed is the SAME image
 * (pwg_conv1d_pack_weight).  Covered: groups == 1, width == 1, and either a stride-1 Conv1d with pad_left == (kernel - 1)
 * * dilation and t_out == t_in, or a ConvTranspose1d with kernel == 2 * stride, pad_left == stride, t_out == t_in *
 * stride; pwg_conv1d_stream_supported is pure host logic (no device needed; pwg_last_error names the reason for 0).
 * pwg_conv1d_stream_hist_floats = batch * c_in * H (0 = unsupported, or kernel 1).  Deterministic, and the sum order of
 * an output element depends neither on n, nor on the batch, nor on the chunk's position: any partition of a stream
 * gives the same bits -- provided every convolution of the push runs here, so a kernel-1 layer (H == 0; hist_in and
 * hist_out may be NULL) belongs on this entry point too: pwg_conv1d_forward picks its reduction split from n and batch. */
int pwg_conv1d_stream_supported(const pwg_conv1d_desc* d);
size_t pwg_conv1d_stream_hist_floats(const pwg_conv1d_desc* d);
int pwg_conv1d_stream_forward(const pwg_conv1d_desc* d, const float* x, const float* hist_in, float* hist_out,
                              const float* w_packed, const float* bias, const float* add1, const float* add2, float* y,
                              void* stream);

/* ---- the stream launch with bf16 operands (opt-in; csrc/conv1d_stream_bf16.hip) ----
 * pwg_conv1d_stream_forward under the numerical definition of the bf16-operand inference above: the window is
 * concat(hist_in, x) with RAW fp32 history; pre_act is applied in fp32 while the window is staged, to history, chunk
 * and start-of-stream padding alike; the activated value is rounded to bf16 (nearest-even); the weights are the bf16
 * image of pwg_conv1d_bf16_pack_weight -- packed through a descriptor of the layer's geometry with PWG_PAD_ZERO, since
 * the image does not depend on padding and the packer admits no other -- products accumulate in fp32 on
 * v_mfma_f32_16x16x32_bf16; the epilogue and the stored result are fp32.  hist_out is bit-identical to what
 * pwg_conv1d_stream_forward writes for the same inputs: the state tensors, their shapes and
 * pwg_conv1d_stream_hist_floats are shared, a stream's state does not depend on its precision.
 * pwg_conv1d_stream_bf16_supported answers exactly as pwg_conv1d_stream_supported for every descriptor (pure host
 * logic; pwg_last_error names the reason for 0).  Deterministic, and the sum order of an output element depends on the
 * layer alone (csrc/conv1d_stream_bf16.hip): any partition of a stream gives the same bits, kernel-1 layers (H == 0)
 * included.
 * These two symbols are purely additive -- no existing signature or behaviour changes -- so pwg_abi_version() stays 15. */
int pwg_conv1d_stream_bf16_supported(const pwg_conv1d_desc* d);
int pwg_conv1d_stream_bf16_forward(const pwg_conv1d_desc* d, const float* x, const float* hist_in, float* hist_out,
                                   const void* w_packed_bf16, const float* bias, const float* add1,
                                   const float* add2, float* y, void* stream);

/* ---- the stream launch with delayed addends and a valid window (fp32; csrc/conv1d_stream.hip) ----
 * For streaming a NON-causal network with a fixed look-ahead: every layer runs in its causal form on a shifted time
 * axis, so an addend of the epilogue (the residual input of a unit, the running sum of the MRF blocks) is older than
 * the launch's output by a fixed number of columns and is read through a delay line, and the columns that lie outside
 * the utterance on the shifted axis must be exact zeros, as the whole-utterance zero padding is.
 * d, x, hist_in, hist_out, w_packed, bias, y: as for pwg_conv1d_stream_forward, with d->pad_mode == PWG_PAD_ZERO.
 * For output column j (chunk-relative, 0 <= j < d->t_out):
 *   valid_lo <= j < valid_hi: the value pwg_conv1d_stream_forward computes, with add_i[j] replaced by
 *     concat(add_i_hist_in, add_i)[j] -- add_i_hist_in (batch, c_out, delay_i) holds the delay_i addend columns before
 *     this chunk, NULL = zeros (start of stream);
 *   every other column: 0.0f is STORED (not skipped), whatever bias, addends and post_act are.
 * add_i_hist_out (batch, c_out, delay_i) = the last delay_i columns of concat(add_i_hist_in, add_i), written by the
 * same launch, also when d->t_out < delay_i; it must be a buffer distinct from add_i_hist_in.  delay_i == 0: a plain
 * addend (or none: add_i NULL), both history pointers ignored.  delay_i > 0 needs add_i and add_i_hist_out.
 * Contraction, sum order ((p0 + p1) + p2) + p3 and tile rule are pwg_conv1d_stream_forward's: with delay_i == 0 and
 * the window [0, t_out) y and hist_out equal that entry's bit for bit; with delays they equal that entry given the
 * addends delayed on the host.  The addends are read from their two sources in the epilogue (no LDS).
 * pwg_conv1d_stream_delayed_supported: pure host logic (no device needed); 0 -- pwg_last_error names the reason -- for
 * whatever pwg_conv1d_stream_supported refuses, for a pad_mode other than PWG_PAD_ZERO, and for a delay that is
 * negative or above 144 columns (the cap of a history).
 * These two symbols are purely additive -- no existing signature or behaviour changes -- so pwg_abi_version() stays 15. */
int pwg_conv1d_stream_delayed_supported(const pwg_conv1d_desc* d, int32_t delay1, int32_t delay2);
int pwg_conv1d_stream_delayed_forward(const pwg_conv1d_desc* d, const float* x, const float* hist_in, float* hist_out,
                                      const float* w_packed, const float* bias, const float* add1,
                                      const float* add1_hist_in, float* add1_hist_out, int32_t delay1, const float* add2,
                                      const float* add2_hist_in, float* add2_hist_out, int32_t delay2, int32_t valid_lo,
                                      int32_t valid_hi, float* y, void* stream);

/* ---- the delayed stream launch with bf16 operands (opt-in; csrc/conv1d_stream_bf16.hip) ----
 * pwg_conv1d_stream_delayed_forward under the numerical definition of pwg_conv1d_stream_bf16_forward: the activated
 * window is rounded to bf16, w_packed_bf16 is the bf16 image of pwg_conv1d_bf16_pack_weight (16-B aligned), products
 * accumulate in fp32 on v_mfma_f32_16x16x32_bf16; bias, the delayed addends, out_mul / out_div, post_act, the stored
 * result, the history and the delay lines are fp32.  Every other parameter, the delay lines, the valid window and the
 * pointer rules (delay_i > 0 needs add_i and add_i_hist_out; every hist_in distinct from its hist_out) are those of
 * pwg_conv1d_stream_delayed_forward; a column outside [valid_lo, valid_hi) is stored as 0.0f, and bf16(act(0)) = 0, so
 * the next layer sees the whole-utterance zero padding.  hist_out and both add_i_hist_out are bit-identical to what
 * pwg_conv1d_stream_delayed_forward writes for the same inputs: a stream's state does not depend on its precision.
 * With delay_i == 0 and the window [0, t_out) y equals pwg_conv1d_stream_bf16_forward's bit for bit; with delays it
 * equals that entry given the addends delayed on the host.  Sum order and tile rule are that entry's: any partition of
 * a stream gives the same bits.
 * pwg_conv1d_stream_bf16_delayed_supported answers exactly as pwg_conv1d_stream_delayed_supported for every descriptor
 * and pair of delays, with the same pwg_last_error reason (pure host logic, no device needed).
 * These two symbols are purely additive -- no existing signature or behaviour changes -- so pwg_abi_version() stays 15. */
int pwg_conv1d_stream_bf16_delayed_supported(const pwg_conv1d_desc* d, int32_t delay1, int32_t delay2);
int pwg_conv1d_stream_bf16_delayed_forward(const pwg_conv1d_desc* d, const float* x, const float* hist_in,
                                           float* hist_out, const void* w_packed_bf16, const float* bias,
                                           const float* add1, const float* add1_hist_in, float* add1_hist_out,
                                           int32_t delay1, const float* add2, const float* add2_hist_in,
                                           float* add2_hist_out, int32_t delay2, int32_t valid_lo, int32_t valid_hi,
                                           float* y, void* stream);

/* ---- the delayed stream launch with a position per item: the slotted form (csrc/conv1d_stream.hip, _bf16.hip) ----
 * For a pool of streams whose utterances start and end independently (utils.StreamPool): the delayed
 * launch, its scalar window replaced by the launch's `rate` (output columns per frame), the output's `delay` (columns)
 * and `slots`, a DEVICE table of 4 int32 per item b (read by the kernel; 4-B aligned):
 *   slots[4b + 0]  frames that went before this push (>= 0; the caller may saturate it once before * rate >= delay).
 *                  0: the item is FRESH -- hist_in and both add_i_hist_in read as zeros for it, whatever they hold
 *   slots[4b + 1]  frames of the utterance from this push's first frame on (negative past its end), if bit 1 below
 *   slots[4b + 2]  bit 0: the item is PAUSED; bit 1: slots[4b + 1] is known
 *   slots[4b + 3]  not read by the kernel: the caller's own
 * A running item's valid window is [max(delay - before * rate, 0), delay + left * rate) clamped to [0, t_out] (the whole
 * of [.., t_out) while `left` is unknown), formed in 64 bits; its y, hist_out and add_i_hist_out are bit for bit what
 * the delayed entry writes for a batch-1 launch of this item with that window (hist_in NULL if fresh).
 * A paused item takes no frames: its hist_out / add_i_hist_out are its hist_in / add_i_hist_in copied through (zeros if
 * it is fresh), its y columns are stored as 0.0f, and its x and addend columns are not read.
 * Every other parameter and pointer rule is the delayed entry's, except that hist_in (where the layer has history) and
 * add_i_hist_in (where delay_i > 0) must be given: the start of a stream is an item's, not the launch's.  Coverage is
 * that of pwg_conv1d_stream_delayed_supported / pwg_conv1d_stream_bf16_delayed_supported.
 * These two symbols are purely additive -- no existing signature or behaviour changes -- so pwg_abi_version() stays 15. */
int pwg_conv1d_stream_slots_forward(const pwg_conv1d_desc* d, const float* x, const float* hist_in, float* hist_out,
                                    const float* w_packed, const float* bias, const float* add1,
                                    const float* add1_hist_in, float* add1_hist_out, int32_t delay1, const float* add2,
                                    const float* add2_hist_in, float* add2_hist_out, int32_t delay2, const int32_t* slots,
                                    int32_t rate, int32_t delay, float* y, void* stream);
int pwg_conv1d_stream_slots_forward_bf16(const pwg_conv1d_desc* d, const float* x, const float* hist_in, float* hist_out,
                                         const void* w_packed_bf16, const float* bias, const float* add1,
                                         const float* add1_hist_in, float* add1_hist_out, int32_t delay1,
                                         const float* add2, const float* add2_hist_in, float* add2_hist_out,
                                         int32_t delay2, const int32_t* slots, int32_t rate, int32_t delay, float* y,
                                         void* stream);

/* ---- the delayed stream launch of a REFLECT-padded layer: the mirrored form (fp32; csrc/conv1d_stream.hip) ----
 * For streaming the non-causal (multi-band) MelGAN with a fixed look-ahead.  Replaces, chunk by chunk, the
 * ReflectionPad1d + Conv1d pairs of the reference generator (models/melgan.py:70-73 the first k = 7 convolution,
 * :135-140 the last one; layers/residual_stack.py:49-52 the dilated k = 3 convolution of a stack) as the delayed entry
 * replaces the zero-padded layers.  The layer runs in its causal form on an axis shifted by its padding p = (k-1)*d/2:
 * output column q is produced once input column q + p has arrived, and by then the columns reflection reads have
 * arrived too (left edge: -1 .. q-p mirror to 1 .. p-q <= q+p; right edge: T-1+i mirrors to T-1-i inside the same
 * 2p+1 window).  History and chunk stay RAW -- they hold stored zeros (or a flush's dummy columns) outside the
 * utterance, never mirror images -- and the window mirrors on read.
 * d: the causal descriptor of the layer (stride 1, pad_left == (k-1)*d, t_out == t_in, groups == 1) with
 *   pad_mode == PWG_PAD_REFLECT and an even (k-1)*d <= 144; t_in = columns of this chunk.
 * x, hist_in (NULL: start of stream, zeros), hist_out, w_packed, bias, y: as for pwg_conv1d_stream_delayed_forward;
 *   hist_out = the last (k-1)*d raw columns of concat(hist_in, x).  There are no addends.
 * [in_lo, in_hi): the valid window of the INPUT in chunk-relative input columns, unclamped: in_lo < 0 means the
 *   utterance's first column lies in the history, in_hi = INT32_MAX that its length is not known yet.  Both are saturated
 *   on the host.  A window column t in [-(k-1)*d, t_in) reads column 2*in_lo - t if t < in_lo, 2*(in_hi-1) - t if
 *   t >= in_hi, else t; the mapped column is then taken from the history if negative, from the chunk otherwise, and
 *   reads as zero if it lies outside [-(k-1)*d, t_in) (no address is formed from it).
 * [valid_lo, valid_hi): the valid window of the output as for the delayed entry: other columns are STORED as 0.0f.  For a
 *   layer of a network, valid_lo = in_lo + p and valid_hi = in_hi + p; a valid column never depends on a column that
 *   read as zero, provided the utterance is longer than p (reflection's own precondition).
 * Contraction, sum order, tile rule, pre- and post-activation (tanh included) are pwg_conv1d_stream_forward's: any
 * partition of a stream gives the same bits.
 * pwg_conv1d_stream_mirrored_supported: pure host logic (no device needed); 0 -- pwg_last_error names the reason -- for a
 * transposed layer, a pad_mode other than PWG_PAD_REFLECT, an odd (k-1)*d, and whatever pwg_conv1d_stream_supported
 * refuses (stride, groups, a history above 144 columns).
 * These two symbols are purely additive -- no existing signature or behaviour changes -- so pwg_abi_version() stays 15. */
int pwg_conv1d_stream_mirrored_supported(const pwg_conv1d_desc* d);
int pwg_conv1d_stream_mirrored_forward(const pwg_conv1d_desc* d, const float* x, const float* hist_in, float* hist_out,
                                       const float* w_packed, const float* bias, float* y, int32_t in_lo, int32_t in_hi,
                                       int32_t valid_lo, int32_t valid_hi, void* stream);

/* ---- the mirrored launch with a position per item: the slotted-mirrored form (fp32; csrc/conv1d_stream.hip) ----
 * For a pool of look-ahead streams of the non-causal (multi-band) MelGAN whose utterances start and end independently
 * (utils.MelGANStreamPool).  Replaces, chunk by chunk and item by item, the same ReflectionPad1d +
 * Conv1d pairs of the reference generator as the mirrored entry (models/melgan.py:70-73 the first k = 7 convolution,
 * :135-140 the last one; layers/residual_stack.py:49-52 the dilated k = 3 convolution of a stack).
 * d, x, hist_out, w_packed, bias, y: as for pwg_conv1d_stream_mirrored_forward; there are no addends.  hist_in must be
 *   given where the layer has history: the start of a stream is an item's, not the launch's.
 * slots, rate, delay: the DEVICE table, the output columns per frame and the OUTPUT's delay of
 *   pwg_conv1d_stream_slots_forward (delay >= p = (k-1)*d/2: the input is delay - p columns late).
 * Per item b, from its row: in_lo = (delay - p) - before * rate, and in_hi = (delay - p) + left * rate if the length is
 *   known, else unbounded; both are formed in 64 bits and saturated to [-(k-1)*d, t_in + 64] on the device, by the
 *   statement the mirrored entry applies on the host.  A running item's y and hist_out are bit for bit what the mirrored
 *   entry writes for a batch-1 launch of this item with [in_lo, in_hi) and [valid_lo, valid_hi) = [in_lo + p, in_hi + p)
 *   (hist_in NULL if the item is FRESH).  A PAUSED item's hist_out is its hist_in copied through (zeros if it is fresh),
 *   its y columns are stored as 0.0f and its x columns are not read.
 * While an utterance's length is unknown its chunk's columns stop p short of its end, so no output that needs the
 * right-hand mirror is computed before the table knows the length.
 * Coverage is that of pwg_conv1d_stream_mirrored_supported (there is no query of its own); pwg_last_error names the
 * reason for a refusal: a NULL hist_in or slots, pad_mode != PWG_PAD_REFLECT, hist_in == hist_out, delay < p.
 * Purely additive -- no existing signature or behaviour changes -- so pwg_abi_version() stays 15. */
int pwg_conv1d_stream_slots_mirrored_forward(const pwg_conv1d_desc* d, const float* x, const float* hist_in,
                                             float* hist_out, const float* w_packed, const float* bias,
                                             const int32_t* slots, int32_t rate, int32_t delay, float* y, void* stream);

/* Diagnostics (host only, no launch, no device needed): the tile and grid a conv stream launch takes for `d` -- the
 * plain, delayed, slotted and mirrored entries, fp32 and bf16 alike: they share one tile rule, evaluated here by the
 * call the launches make.  out[5]:
 *   out[0] tile rows (16 or 32), out[1] tile columns (16, 32 or 64: chunks of up to 16 / 32 / more columns); 32 rows
 *          only with 64 columns and ceil(m / 32) * column tiles * batch >= 512 workgroups (m = c_out, or c_out * stride
 *          for the transposed form)
 *   out[2..4] grid: column tiles, row blocks, batch.
 * Refuses what pwg_conv1d_stream_supported refuses, with the same pwg_last_error reason, and a NULL out.
 * Purely additive -- no existing signature or behaviour changes -- so pwg_abi_version() stays 15. */
int pwg_conv1d_stream_plan(const pwg_conv1d_desc* d, int32_t* out);

/* Diagnostics (host only, no launch, no device needed): the plan pwg_conv1d_forward derives for a descriptor.
 * has_addends: 1 if add1 / add2 will be passed.  out[8]:
 *   out[0] kernel family: 0 = MFMA implicit-GEMM kernel, 1 = grouped 16x16x4 kernel, 2 = single-input-channel
 *          streaming kernel, 3 = few-output-channel streaming kernel (out[1..7] are 0 unless out[0] == 0)
 *   out[1] tile configuration, out[2] reduction slices (the workspace query is sized for them), out[3] 1 = LDS-DMA path
 *   out[4] logical tile order inside an XCD's run of workgroups: 0 = the row blocks of a column tile together (they
 *          share the x window in that XCD's L2; the default), 1 = the items of a (row block, reduction slice) together
 *          (they share the weight chunk; measured no faster, kept selectable: PWG_TILE_ORDER=1 forces it, =2 lets a
 *          bytes-per-XCD model choose per launch)
 *   out[5..7] grid (column tiles, row blocks x groups, items x slices).
 * pwg_debug_conv_tile_of_workgroup evaluates, on the host, the kernel's own dispatch-id -> logical-tile map
 * (out[3] = column tile, row block index, item * ksplit + slice): tests walk it to show it is a bijection.        */
int pwg_conv1d_plan(const pwg_conv1d_desc* d, int32_t has_addends, int32_t* out);
int pwg_debug_conv_tile_of_workgroup(int32_t grid_x, int32_t grid_y, int32_t grid_z, int32_t row_blocks,
                                     int32_t ksplit, int32_t item_major, int32_t workgroup, int32_t* out);

/* The sibling for the weight gradient (host only, no launch, no device needed; purely additive): what
 * pwg_conv1d_backward_weight (weight_norm = 0) or pwg_conv1d_backward_weight_wn (weight_norm = 1) launches for `d`,
 * decided by the functions the launcher itself calls, so it reflects this process's PWG_WG_* overrides and concurrency
 * hint.  has_bias: db will be requested.  out[20]:
 *   out[0]  kernel family: 0 = conv1d_wgrad_kernel (fp32 MFMA), 1 = grouped 16x16x4 kernel (gconv.hip), 2 = single-input-
 *           channel kernel, 3 = 1 x 1 kernel (wgrad_k1.hip); out[4..17] are 0 unless out[0] == 0
 *   out[1]  slab finisher: 0 = none (one slice: the kernel stores the gradients), 1 = reduce_slabs_kernel (family 1: its own
 *           reduction kernel), 2 = reduce_slabs_wide_kernel, 3 = slab reduction + pwg_weight_norm_backward, 4 / 5 = the fused
 *           weight-norm finisher, narrow / wide
 *   out[2], out[3]  workspace floats the entry point asks for, low 31 bits and the bits above: what the workspace query
 *           returns (the queries always reserve the fused bias row; with weight_norm = 0 and has_bias = 0 the row is left out)
 *   out[4]  1 = 32 x 32 tile, out[5] accumulators (taps) per wave TG, out[6] taps per workgroup, out[7] tap groups (grid z),
 *   out[8]  1 = per-tap windows, out[9] chunk columns TT, out[10] rows_half (> 0: row-aligned chunks), out[11] 1 = 16-byte
 *           row staging, out[12] MODE (0..4), out[13] 1 = an activating instantiation, out[14] compile-time stride of MODE 3
 *           (0 = run time), out[15] tiles (grid y), out[16] reduction slices (grid x), out[17] dynamic LDS bytes
 *   out[18] slabs the finisher sums (families 0, 2, 3), out[19] floats between the X tile's rows in LDS (family 0).
 * Refuses what the launcher refuses: bad groups, a pad mode, tensors above 4 GiB, a LeakyReLU slope outside [0, 1],
 * a transposed layer with dilation and stride, more than 160 KiB of LDS, a weight-norm row beyond the LDS row buffer. */
int pwg_conv1d_backward_weight_plan(const pwg_conv1d_desc* d, int32_t weight_norm, int32_t has_bias, int32_t* out);

/* ------------------------------------------------------------------------- */
/* One HiFi-GAN MRF residual unit as ONE launch (inference; channels 32 / 64)  */
/*                                                                            */
/*   y = ( x + conv_{k,1}(lrelu(conv_{k,d}(lrelu(x)) + b1)) + b2 [+ add2] ) [/ out_div]      (has_conv2 = 1)
 *   y = ( x + conv_{k,d}(lrelu(x)) + b1 [+ add2] ) [/ out_div]                                (has_conv2 = 0)
 * replaces one iteration of the loop at layers/residual_block.py:253-257 (`xt = convs1[idx](x);
 * xt = convs2[idx](xt); x = xt + x`), add2 / out_div additionally fold the MRF mean of
 * models/hifigan.py:186-190.  All input channels of a column tile stay resident in LDS, the
 * intermediate activation never reaches HBM (csrc/resunit.hip).  Both convolutions are
 * "same"-padded with zeros (padding = (k-1)/2*dilation), k odd, t % 4 == 0, 0 < slope < 1;
 * pwg_resunit_supported() tells whether a unit fits (otherwise use two pwg_conv1d_forward calls:
 * identical result up to fp32 summation order).  Weights: torch layout (C, C, k) re-laid by
 * pwg_resunit_pack_weight (`scale` = optional weight-norm row scale as in pwg_conv1d_pack_weight).
 * x / y / add2: (batch, channels, t), 16-B aligned, y must not alias x.                            */
typedef struct pwg_resunit_desc {
  int32_t batch;
  int32_t channels;
  int32_t t;
  int32_t kernel;
  int32_t dilation;   /* of the first convolution; the second one has dilation 1 */
  int32_t has_conv2;
  float slope1;       /* LeakyReLU in front of the first convolution  */
  float slope2;       /* LeakyReLU in front of the second convolution */
  float out_div;      /* 1.0f = off */
} pwg_resunit_desc;
int pwg_resunit_supported(const pwg_resunit_desc* d);
/* 1 when the one-launch unit is also the faster choice on MI355X (measured, see csrc/resunit.hip) */
int pwg_resunit_profitable(const pwg_resunit_desc* d);
size_t pwg_resunit_packed_weight_floats(int32_t channels, int32_t kernel);
int pwg_resunit_pack_weight(int32_t channels, int32_t kernel, const float* w, const float* scale,
                            float* w_packed, void* stream);
int pwg_resunit_forward(const pwg_resunit_desc* d, const float* x, const float* w1_packed, const float* b1,
                        const float* w2_packed, const float* b2, const float* add2, float* y, void* stream);

/* ---- split-operand residual unit (fp32-accurate on the bf16 matrix pipe; csrc/resunit_split.hip) ----
 * The unit of pwg_resunit_forward (same descriptor, same formula, both forms) under the numerical definition of the
 * split-operand inference above, applied twice:
 *   1. lrelu(x) is formed in fp32 and split three ways; the effective weights are split once by the packer;
 *   2. the six products lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi go into one fp32 accumulator set;
 *   3. h = lrelu(acc + b1) is formed in fp32 (v > 0 ? v : v * slope2), is zero outside [0, t) and is split three ways;
 *   4. the residual is the raw fp32 x; the epilogue is acc + bias + x + add2, then the true division by out_div.
 * The accumulation order of an output element is that of pwg_conv1d_split_forward (32-channel chunk, tap, reduction
 * step, product), so a unit is bit-identical to two chained pwg_conv1d_split_forward_cfg launches at the same
 * mfma_shape (conv1: pre_act = post_act = leaky, bias b1; conv2: bias b2, add1 = x, add2, out_div), and deterministic.
 * w1_split / w2_split are the images of pwg_conv1d_split_pack_weight for a channels -> channels convolution of this
 * kernel size (the image depends on neither dilation, padding nor length), 16-B aligned; w2_split is NULL exactly when
 * has_conv2 == 0.  Covered: channels 32 / 64, odd kernel, t % 4 == 0, 0 < slope < 1, a window whose three bf16 planes
 * fit 80 KB of LDS; x / y / add2 16-B aligned, y != x.  pwg_resunit_split_supported is pure host logic (no device
 * needed; pwg_last_error names the reason for 0); anything else is refused with a message and launches nothing.
 * pwg_resunit_split_forward_cfg (tuning / tests): mfma_shape 32 = 32x32x16, 16 = 16x16x32 (the default).
 * These symbols are purely additive, so pwg_abi_version() stays 15. */
int pwg_resunit_split_supported(const pwg_resunit_desc* d);
int pwg_resunit_split_forward(const pwg_resunit_desc* d, const float* x, const void* w1_split, const float* b1,
                              const void* w2_split, const float* b2, const float* add2, float* y, void* stream);
int pwg_resunit_split_forward_cfg(const pwg_resunit_desc* d, const float* x, const void* w1_split, const float* b1,
                                  const void* w2_split, const float* b2, const float* add2, float* y, int32_t mfma_shape,
                                  void* stream);
/* The ragged form: one launch over a batch whose items have their own lengths (the batched form of the decode loop of
 * bin/decode.py:214-243).  frames: device int32 (batch,), 0 <= frames[b]; item b ends at column
 * tv = min(frames[b] * rate, t), t stays the row stride.  x and add2 must be exactly zero at the columns >= tv of their
 * item (pwg_zero_tail establishes that); h is zero outside [0, tv); the columns < tv of y are bit for bit those of
 * pwg_resunit_split_forward_cfg on the item alone with t = tv at the same mfma_shape, the columns >= tv are stored as
 * 0.0f.  A workgroup whose tile lies at or beyond tv only stores zeros.  Nothing on the host depends on the table's
 * values: a captured launch serves every set of lengths.  pwg_resunit_split_ragged_supported is
 * pwg_resunit_split_supported plus rate % 4 == 0 (a value of four samples is stored whole or as zeros), pure host
 * logic with its reason in pwg_last_error.  A NULL or unaligned table, or such a rate, is refused with a message and
 * launches nothing.  Additive: pwg_abi_version() stays 15. */
int pwg_resunit_split_ragged_supported(const pwg_resunit_desc* d, int32_t rate);
int pwg_resunit_split_forward_ragged(const pwg_resunit_desc* d, const float* x, const void* w1_split, const float* b1,
                                     const void* w2_split, const float* b2, const float* add2, float* y,
                                     int32_t mfma_shape, const int32_t* frames, int32_t rate, void* stream);
/* The chained block: n_units <= 3 pair-form units (has_conv2 = 1) of one kernel size, unit u with dilation dilations[u]
 * and slopes slopes1[u] / slopes2[u], as ONE launch.  Bit for bit n_units chained pwg_resunit_split_forward_cfg launches
 * at the same mfma_shape: units 0 .. n_units - 2 with add2 = NULL and out_div = 1, the last with add2 and d->out_div;
 * d->dilation, d->slope1 and d->slope2 are not read.  Every phase of every unit computes the same frame of H columns
 * (256 at 32 channels, 128 at 64); with edge = sum over the units of (k - 1) / 2 * (dilation + 1), rounded up to a
 * multiple of 4, a frame starts at column t0 - edge and stores its central bn_out = H - 2 * edge columns.
 * pwg_resblock_split_supported is pure host logic (reason in pwg_last_error); it refuses bn_out < H / 2, a
 * single-convolution unit, n_units outside 1 .. 3 and whatever pwg_resunit_split_supported refuses for a unit; the
 * forward refuses y == x.  pwg_resblock_split_frame reports out[0..5] = H, bn_out, edge, margin rows of a plane, LDS
 * bytes, frames per row.  w1_split / b1 / w2_split / b2: host arrays of n_units device pointers (a bias may be NULL).
 * Additive: pwg_abi_version() stays 15. */
int pwg_resblock_split_supported(const pwg_resunit_desc* d, int32_t n_units, const int32_t* dilations);
int pwg_resblock_split_frame(const pwg_resunit_desc* d, int32_t n_units, const int32_t* dilations, int32_t* out);
int pwg_resblock_split_forward_cfg(const pwg_resunit_desc* d, int32_t n_units, const int32_t* dilations,
                                   const float* slopes1, const float* slopes2, const float* x,
                                   const void* const* w1_split, const float* const* b1, const void* const* w2_split,
                                   const float* const* b2, const float* add2, float* y, int32_t mfma_shape, void* stream);

/* ------------------------------------------------------------------------- */
/* One MelGAN residual stack as ONE launch (channels 48 / 96 / 192, kernel 3; csrc/resstack.hip)             */
/*                                                                            */
/*   h = conv_{3,dilation}(reflect_pad_dilation(lrelu(x))) + b1;   y = conv_{1x1}(lrelu(h)) + b2 + conv_{1x1}(x) + bs
 * replaces ResidualStack.forward (layers/residual_stack.py:75-85: `self.stack(c) + self.skip_layer(c)` with the
 * Sequential of :45-53 and the skip layer of :73).  All channels of a column tile stay resident in LDS; `h` (the
 * pre-activation output of the dilated convolution, what a backward pass needs) is written out only when the pointer
 * is given.  t % 4 == 0, t >= 64, 1 <= dilation <= 27, 0 < slope < 1; pwg_resstack_supported() tells whether a unit
 * fits (otherwise use three pwg_conv1d_forward calls: identical result up to fp32 summation order).  Weights: torch
 * layouts (C, C, 3), (C, C, 1), (C, C, 1) re-laid into ONE image by pwg_resstack_pack_weight (`scale*` = optional
 * weight-norm row scales as in pwg_conv1d_pack_weight).  x / y / h: (batch, channels, t), x 16-B aligned, y and h must
 * not alias x.                                                                                                   */
int pwg_resstack_supported(int32_t channels, int32_t t, int32_t dilation);
size_t pwg_resstack_packed_weight_floats(int32_t channels);
int pwg_resstack_pack_weight(int32_t channels, const float* w1, const float* scale1, const float* w2,
                             const float* scale2, const float* ws, const float* scale_s, float* w_packed, void* stream);
int pwg_resstack_forward(int32_t batch, int32_t channels, int32_t t, int32_t dilation, float slope, const float* x,
                         const float* w_packed, const float* b1, const float* b2, const float* bs, float* y, float* h,
                         void* stream);
/* The ragged form (inference; ResidualStack.forward of layers/residual_stack.py:75-85 inside the batched form of the
 * decode loop of bin/decode.py:214-243): frames device int32 (batch,), item b is the sequence [0, tb),
 * tb = min(frames[b] * rate, t), inside a row of stride t.  The reflection (ReflectionPad1d of
 * layers/residual_stack.py:49) mirrors at tb, nothing at or past tb is read (x may hold anything there, NaN included),
 * the columns >= tb of y are stored as 0.0f, and a workgroup whose tile lies at or past tb only stores zeros.  For
 * tb % 4 == 0, tb >= 64, tb > dilation the columns < tb of y are bit for bit pwg_resstack_forward on the item alone with
 * t = tb; with every item at t the output is the plain call's.  h is not written.  Nothing on the host reads the table:
 * a captured launch serves every set of lengths.  pwg_resstack_ragged_supported is pwg_resstack_supported plus
 * rate >= 4, rate % 4 == 0 (pure host logic).  A NULL or misaligned table, such a rate and everything the plain call
 * refuses are refused with a message before any launch.  Additive: pwg_abi_version() stays 15. */
int pwg_resstack_ragged_supported(int32_t channels, int32_t t, int32_t dilation, int32_t rate);
int pwg_resstack_forward_ragged(int32_t batch, int32_t channels, int32_t t, int32_t dilation, float slope, const float* x,
                                const float* w_packed, const float* b1, const float* b2, const float* bs, float* y,
                                const int32_t* frames, int32_t rate, void* stream);
/* Data gradient of the same unit in ONE launch (the backward of the three convolutions' data paths and of both
 * LeakyReLUs, layers/residual_stack.py:45-85 under autograd), in the padded domain of the dilated convolution:
 *   dh[t]  = lrelu'(h[t]) * (W2^T dy)[t]                                              (batch, channels, t)
 *   dxp[p] = lrelu'(xp[p]) * sum_tap (W1[tap]^T dh)[p - tap*dilation] + (Ws^T dy)[p - dilation]   (batch, channels, t + 2*dilation)
 * with xp = ReflectionPad1d(dilation)(x) and dy, dh zero outside [0, t): dx = pwg_pad1d_backward(dxp) (the
 * reflection's adjoint), dh is the dilated layer's weight-gradient operand.  `h` as written by pwg_resstack_forward;
 * weights re-laid (transposed) by pwg_resstack_pack_weight_bwd (same size as the forward image).                  */
int pwg_resstack_pack_weight_bwd(int32_t channels, const float* w1, const float* scale1, const float* w2,
                                 const float* scale2, const float* ws, const float* scale_s, float* w_packed,
                                 void* stream);
int pwg_resstack_backward_data(int32_t batch, int32_t channels, int32_t t, int32_t dilation, float slope,
                               const float* dy, const float* h, const float* x, const float* w_packed_bwd, float* dh,
                               float* dxp, void* stream);

/* One gated residual layer of the Parallel WaveGAN generator as ONE launch (csrc/wavenet.hip):
 *   z = conv_{k=3,dilation}(x) + b_dil + conv1x1_aux(c);  g = tanh(z[:64]) * sigmoid(z[64:]);
 *   skips_out = (conv1x1_skip(g) + b_skip + skips) * skip_mul;   x_out = (conv1x1_out(g) + b_out + x) * out_mul
 * replacing the five ATen calls of WaveNetResidualBlock.forward (layers/residual_block.py:102-140) plus the
 * running skip sum of the generator (models/parallel_wavegan.py:164-169).  Built for the PWG.v1 geometry
 * (64 residual / 128 gate / 64 skip / 80 aux channels, kernel 3, non-causal); pwg_wavenet_layer_supported says so.
 * x, skips, x_out, skips_out, g_out: (batch, 64, t); c: (batch, 80, t) (the upsampled mel); z_out: (batch, 128, t).
 * skips may be NULL (first layer); skips_out may alias skips; x_out must not alias x.  z_out / g_out (both or
 * neither; NULL in inference) receive the gate input and output for the backward pass.
 * `packed`: pwg_wavenet_pack_weights image of the four torch-layout weights w_dil (128, 64, 3), w_aux (128, 80, 1),
 * w_skip (64, 64, 1), w_out (64, 64, 1), each with an optional weight-norm row scale.                          */
typedef struct pwg_wavenet_desc {
  int32_t batch;
  int32_t t;
  int32_t residual_channels;
  int32_t gate_channels;
  int32_t skip_channels;
  int32_t aux_channels;
  int32_t kernel;
  int32_t dilation;
  int32_t causal;
  float out_mul;   /* sqrt(0.5) */
  float skip_mul;  /* 1, or sqrt(1 / layers) in the last layer */
} pwg_wavenet_desc;
int pwg_wavenet_layer_supported(const pwg_wavenet_desc* d);
size_t pwg_wavenet_packed_weight_floats(const pwg_wavenet_desc* d);
int pwg_wavenet_pack_weights(const pwg_wavenet_desc* d, const float* w_dil, const float* scale_dil, const float* w_aux,
                             const float* scale_aux, const float* w_skip, const float* scale_skip, const float* w_out,
                             const float* scale_out, float* packed, void* stream);
int pwg_wavenet_layer_forward(const pwg_wavenet_desc* d, const float* x, const float* c, const float* skips,
                              const float* packed, const float* b_dil, const float* b_skip, const float* b_out,
                              float* x_out, float* skips_out, float* z_out, float* g_out, void* stream);
/* ---- stateful streaming form of the CAUSAL layer (fp32; csrc/wavenet_stream.hip) ----
 * The layer formula above on the next d->t = n columns of a stream, d->causal = 1 (layers/residual_block.py:74-76,
 * 102-140: left-only padding (kernel-1)*dilation): the dilated taps read columns n - 2d, n - d, n of
 * X = concat(hist_in (batch, 64, H), x (batch, 64, n)), H = (kernel-1)*dilation = 2d; the residual is x.
 * hist_in == NULL is the start of a stream: zero left context.  The same launch writes hist_out = the last H raw
 * columns of X, also when n < H.  hist_in and hist_out must be distinct buffers; skips may be NULL (first layer);
 * skips_out may alias skips; x_out must not alias x.  c: (batch, 80, n).
 * Geometry: 64 residual / 128 gate / 64 skip / 80 aux channels, kernel 3, causal, any dilation >= 1, any n >= 1,
 * batch 1 .. 65535; pwg_wavenet_stream_supported is pure host logic (no device needed; pwg_last_error names the reason
 * for 0).  pwg_wavenet_stream_hist_floats = batch * 64 * (kernel-1) * dilation (0 = unsupported).
 * `packed`: the pwg_wavenet_pack_weights image, unchanged -- its row order (tap 0, 1, 2, aux) does not depend on
 * causality; the packer refuses a causal descriptor, so pack through a non-causal one of the same channels.
 * Deterministic, and the sum order of an output element depends on the layer alone (not on n, the batch or the chunk's
 * position): any partition of a stream gives bit-identical results.
 * These three symbols are purely additive -- no existing signature or behaviour changes.                         */
int pwg_wavenet_stream_supported(const pwg_wavenet_desc* d);
size_t pwg_wavenet_stream_hist_floats(const pwg_wavenet_desc* d);
int pwg_wavenet_stream_forward(const pwg_wavenet_desc* d, const float* x, const float* c, const float* skips,
                               const float* hist_in, float* hist_out, const float* packed, const float* b_dil,
                               const float* b_skip, const float* b_out, float* x_out, float* skips_out, void* stream);
/* ---- the delayed form: the NON-causal layer in a stream with a fixed look-ahead (fp32; csrc/wavenet_stream.hip) ----
 * d->causal = 0 (the layer's own descriptor).  The non-causal layer reads x at t - d, t, t + d; on a time axis shifted
 * by d these are the causal taps n - 2d, n - d, n of X = concat(hist_in, x), so the launch is the causal one -- same
 * kernel body, same image, same contraction -- whose output is d columns later than its input, with four differences:
 *   residual      the MIDDLE tap X[n - d] (the causal layer adds X[n]);
 *   conditioning  output column j reads C[j - c_delay], C = concat(c_line (batch, 80, c_cols), c (batch, 80, n)) indexed
 *                 from the chunk's first column (j - c_delay < 0: c_line[c_cols + j - c_delay]); c_line == NULL reads
 *                 as zeros (start of stream); 0 <= c_delay <= c_cols.  The line is the caller's (pwg_delay_line_forward
 *                 keeps it): one line serves every layer of a generator, each at its own c_delay;
 *   skip sum      output column j adds concat(skip_line_in (batch, 64, d), skips (batch, 64, n))[j] -- the running sum is
 *                 d columns older than this layer's output; skip_line_in == NULL: zeros.  The same launch writes
 *                 skip_line_out (batch, 64, d) = the last d columns of that concatenation, also when n < d.
 *                 skips == NULL (first layer): no addend, both line pointers ignored;
 *   valid window  x_out and skips_out columns outside [valid_lo, valid_hi) (chunk-relative) are STORED as 0.0f: the
 *                 zero padding the next layer sees.
 * hist_in / hist_out and skip_line_in / skip_line_out must be distinct buffers; x_out must not alias x and skips_out
 * must not alias skips (tiles read their neighbours' columns).
 * Geometry: that of pwg_wavenet_stream_supported with causal == 0; a causal descriptor and a negative c_delay are
 * refused, as is whatever takes a byte offset inside one item past 32 bits (pwg_last_error names the reason).
 * pwg_wavenet_stream_delayed_supported is pure host logic; pwg_wavenet_stream_delayed_hist_floats = batch * 64 *
 * (kernel-1) * dilation (0 = unsupported).  The sum order of an output element is the causal form's and depends on the
 * layer alone (not on n, the batch, c_delay, its alignment, or which staging path a window took): any partition of a
 * stream gives bit-identical results.
 * These three symbols are purely additive -- no existing signature or behaviour changes -- so pwg_abi_version() stays 15. */
int pwg_wavenet_stream_delayed_supported(const pwg_wavenet_desc* d, int32_t c_delay);
size_t pwg_wavenet_stream_delayed_hist_floats(const pwg_wavenet_desc* d);
int pwg_wavenet_stream_delayed_forward(const pwg_wavenet_desc* d, const float* x, const float* c, const float* c_line,
                                       int32_t c_cols, int32_t c_delay, const float* skips, const float* skip_line_in,
                                       float* skip_line_out, const float* hist_in, float* hist_out, const float* packed,
                                       const float* b_dil, const float* b_skip, const float* b_out, int32_t valid_lo,
                                       int32_t valid_hi, float* x_out, float* skips_out, void* stream);
/* ---- the delayed layer with a position per item: the slotted form (csrc/wavenet_stream.hip, _bf16.hip) ----
 * For a pool of Parallel WaveGAN look-ahead streams whose utterances start and end independently (utils.PWGStreamPool,
 * DESIGN.md s11.11).  Replaces pwg_wavenet_stream_delayed_forward / pwg_wavenet_stream_bf16_delayed_forward of a
 * lock-step batch: the scalar window gives way to `slots` -- the DEVICE table of pwg_conv1d_stream_slots_forward, 4 int32
 * per item, the same rows, flags and window rule -- with the launch's `rate` (columns per frame) and output `delay`.
 * A running item's x_out, skips_out, hist_out and skip_line_out are bit for bit what the delayed entry writes for a
 * batch-1 launch of this item with its window; a FRESH item (slots[4b] == 0) reads hist_in, c_line and skip_line_in as
 * NULL whatever they hold; a PAUSED item writes hist_out = hist_in and skip_line_out = skip_line_in (zeros if it is also
 * fresh), stores 0.0f to its x_out and skips_out columns and reads none of its x, c, skips.
 * Every other parameter and pointer rule is the delayed entry's, except that hist_in, c_line (where c_delay > 0) and,
 * with skips, skip_line_in must be given: the start of a stream is an item's, not the launch's.  Coverage is that of
 * pwg_wavenet_stream_delayed_supported / pwg_wavenet_stream_bf16_delayed_supported.  The bf16 entry has no z / g outputs.
 * These two symbols are purely additive -- no existing signature or behaviour changes -- so pwg_abi_version() stays 15. */
int pwg_wavenet_stream_slots_forward(const pwg_wavenet_desc* d, const float* x, const float* c, const float* c_line,
                                     int32_t c_cols, int32_t c_delay, const float* skips, const float* skip_line_in,
                                     float* skip_line_out, const float* hist_in, float* hist_out, const float* packed,
                                     const float* b_dil, const float* b_skip, const float* b_out, const int32_t* slots,
                                     int32_t rate, int32_t delay, float* x_out, float* skips_out, void* stream);
int pwg_wavenet_stream_slots_forward_bf16(const pwg_wavenet_desc* d, const float* x, const float* c, const float* c_line,
                                          int32_t c_cols, int32_t c_delay, const float* skips, const float* skip_line_in,
                                          float* skip_line_out, const float* hist_in, float* hist_out, const void* packed,
                                          const float* b_dil, const float* b_skip, const float* b_out,
                                          const int32_t* slots, int32_t rate, int32_t delay, float* x_out,
                                          float* skips_out, void* stream);
/* ---- bf16-operand inference form of the same layer (opt-in; csrc/wavenet_bf16.hip) ----
 * The definition of the bf16-operand convolution (pwg_conv1d_bf16_*, above) applied to each of the layer's four
 * convolutions, in ONE launch:
 *   z         = W_dil (*) bf16(x) + W_aux . bf16(c) + b_dil      (products accumulated in fp32 on the bf16 MFMA)
 *   g         = bf16(tanh(z[:64]) * sigmoid(z[64:]))              (gate in fp32, then rounded to nearest-even)
 *   skips_out = (W_skip . g + b_skip + skips) * skip_mul;   x_out = (W_out . g + b_out + x) * out_mul
 * where W_* are the effective weights (w * scale) rounded to bf16 once, by pwg_wavenet_bf16_pack_weights, and the bias,
 * the residual x (read in fp32, not from the rounded operand), the running skip sum and every tensor in memory are
 * fp32.  Geometry: that of pwg_wavenet_layer_supported (PWG.v1 channels, kernel 3, non-causal, any dilation, any t >= 1,
 * batch 1 .. 65535); pwg_wavenet_bf16_supported is pure host logic (no device needed; pwg_last_error names the reason
 * for 0).  The image is pwg_wavenet_bf16_packed_weight_bytes bytes (0 = unsupported), 16-B aligned.
 * pwg_wavenet_bf16_layer_forward takes the arguments of pwg_wavenet_layer_forward in the same order; z_out / g_out
 * (both or neither, NULL in normal use) receive the fp32 z and the bf16-rounded g (stored as fp32) for stage tests.
 * x, c 4-B aligned.  Deterministic (no split reduction, no atomics).  Inference only: there is no backward.
 * pwg_wavenet_bf16_layer_forward_cfg (tuning): mfma_shape 32 = 32x32x16, 16 = 16x16x32 at the same tiles.       */
int pwg_wavenet_bf16_supported(const pwg_wavenet_desc* d);
size_t pwg_wavenet_bf16_packed_weight_bytes(const pwg_wavenet_desc* d);
int pwg_wavenet_bf16_pack_weights(const pwg_wavenet_desc* d, const float* w_dil, const float* scale_dil,
                                  const float* w_aux, const float* scale_aux, const float* w_skip, const float* scale_skip,
                                  const float* w_out, const float* scale_out, void* packed, void* stream);
int pwg_wavenet_bf16_layer_forward(const pwg_wavenet_desc* d, const float* x, const float* c, const float* skips,
                                   const void* packed, const float* b_dil, const float* b_skip, const float* b_out,
                                   float* x_out, float* skips_out, float* z_out, float* g_out, void* stream);
int pwg_wavenet_bf16_layer_forward_cfg(const pwg_wavenet_desc* d, const float* x, const float* c, const float* skips,
                                       const void* packed, const float* b_dil, const float* b_skip, const float* b_out,
                                       float* x_out, float* skips_out, float* z_out, float* g_out, int32_t mfma_shape,
                                       void* stream);
/* ---- the ragged forms of the layer, fp32 and bf16 (inference; csrc/wavenet.hip, csrc/wavenet_bf16.hip) ----
 * One launch over a batch whose items have their own lengths (WaveNetResidualBlock.forward of
 * layers/residual_block.py:102-140 inside the batched form of the decode loop of bin/decode.py:214-243).  frames: device
 * int32 (batch,), 0 <= frames[b]; item b is the sequence [0, e), e = min(frames[b] * rate, t), inside a row of stride t.
 * Every read of x, c and skips at a column >= e is replaced by zero -- the three tap windows, the residual, the skip sum,
 * and the bf16 kernel's separate fp32 residual and skip loads -- so those columns may hold anything, NaN included; the
 * columns >= e of x_out and skips_out are NOT written (no zero-tail pass is needed between layers: the next layer does
 * not read them either).  A workgroup whose 64 columns lie at or past e returns before any load, so the cost follows
 * the lengths; an item of 0 frames does nothing.  The fast staging path is taken where a window lies inside [0, e).
 * The columns < e of both outputs are bit for bit those of pwg_wavenet_layer_forward (pwg_wavenet_bf16_layer_forward_cfg
 * at the same mfma_shape) on the item alone: contiguous x[b, :, :e], c[b, :, :e], skips[b, :, :e] with d->t = e; with
 * every item at t the outputs are the plain call's.  No z_out / g_out.  skips may be NULL; skips_out may alias skips;
 * x_out must not alias x.  Nothing on the host depends on the table's values: a captured launch serves every set of
 * lengths.  pwg_wavenet_layer_ragged_supported is pwg_wavenet_layer_supported plus rate >= 4, rate % 4 == 0 (an item
 * ends where a row of t % 4 == 0 may end: a value of four samples is stored whole or not at all), with the kernel's
 * limit on t (128 * t * 4 < 2^32: byte offsets into an item are 32-bit); pure host logic, no device needed, the reason
 * for 0 in pwg_last_error.  It answers for both precisions.  A NULL or misaligned (4 B) table, rate <= 0 or another rate
 * it refuses, a causal descriptor and everything the plain calls refuse are refused with a message, launching nothing.
 * mfma_shape of the bf16 form: 32, 16, or 0 = the default of pwg_wavenet_bf16_layer_forward.
 * These three symbols are purely additive, so pwg_abi_version() stays 15. */
int pwg_wavenet_layer_ragged_supported(const pwg_wavenet_desc* d, int32_t rate);
int pwg_wavenet_layer_forward_ragged(const pwg_wavenet_desc* d, const float* x, const float* c, const float* skips,
                                     const float* packed, const float* b_dil, const float* b_skip, const float* b_out,
                                     float* x_out, float* skips_out, const int32_t* frames, int32_t rate, void* stream);
int pwg_wavenet_bf16_layer_forward_ragged(const pwg_wavenet_desc* d, const float* x, const float* c, const float* skips,
                                          const void* packed, const float* b_dil, const float* b_skip,
                                          const float* b_out, float* x_out, float* skips_out, int32_t mfma_shape,
                                          const int32_t* frames, int32_t rate, void* stream);
/* ---- the two streaming forms of the layer with bf16 operands (opt-in; csrc/wavenet_stream_bf16.hip) ----
 * pwg_wavenet_stream_forward and pwg_wavenet_stream_delayed_forward computed the way pwg_wavenet_bf16_layer_forward
 * computes: the windows of x and c (history, conditioning line and chunk alike) are rounded to bf16 while they are
 * staged, `packed` is the pwg_wavenet_bf16_pack_weights image (its K order tap 0, 1, 2, aux does not depend on
 * causality; the packer refuses a causal descriptor, so pack through a non-causal one of the same channels), products
 * are accumulated in fp32 on the 32x32x16 bf16 MFMA, the gate is fp32 and rounded to bf16; biases, the residual (the
 * fp32 value re-read from memory: x[n], or concat(hist_in, x)[n - d] in the delayed form), the skip addend, scales,
 * tensors, history and lines are fp32.  hist_out and skip_line_out are the raw fp32 columns the fp32 launches write,
 * bit for bit, so the state of a stream does not depend on its precision.
 * Arguments: those of the fp32 entries in the same order, then z_out (batch, 128, n) / g_out (batch, 64, n) (both or
 * neither, NULL in normal use: the fp32 z and the bf16-rounded g, stored as fp32, for stage tests).  Geometry, pointer,
 * aliasing and 32-bit-offset rules are those of the fp32 forms, refused with the same words in pwg_last_error; the
 * *_supported entries are pure host logic; history sizes are pwg_wavenet_stream_hist_floats and
 * pwg_wavenet_stream_delayed_hist_floats.  The sum order of an output element is that of pwg_wavenet_bf16_layer_forward
 * and depends on the layer alone (not on n, the batch, the chunk's position, c_delay, its alignment, or which staging
 * path a window took): any partition of a stream gives bit-identical results, and the delayed launch over a whole
 * utterance gives the bits of pwg_wavenet_bf16_layer_forward.  Inference only.
 * These four symbols are purely additive -- no existing signature or behaviour changes -- so pwg_abi_version() stays 15. */
int pwg_wavenet_stream_bf16_supported(const pwg_wavenet_desc* d);
int pwg_wavenet_stream_bf16_forward(const pwg_wavenet_desc* d, const float* x, const float* c, const float* skips,
                                    const float* hist_in, float* hist_out, const void* packed, const float* b_dil,
                                    const float* b_skip, const float* b_out, float* x_out, float* skips_out, float* z_out,
                                    float* g_out, void* stream);
int pwg_wavenet_stream_bf16_delayed_supported(const pwg_wavenet_desc* d, int32_t c_delay);
int pwg_wavenet_stream_bf16_delayed_forward(const pwg_wavenet_desc* d, const float* x, const float* c, const float* c_line,
                                            int32_t c_cols, int32_t c_delay, const float* skips, const float* skip_line_in,
                                            float* skip_line_out, const float* hist_in, float* hist_out, const void* packed,
                                            const float* b_dil, const float* b_skip, const float* b_out, int32_t valid_lo,
                                            int32_t valid_hi, float* x_out, float* skips_out, float* z_out, float* g_out,
                                            void* stream);
/* Data path of the layer's backward pass in two launches (the weight gradients use pwg_conv1d_backward_weight*):
 *   gate_backward: dz (batch, 128, t) = d loss / d z from dx_out, ds_out (gradients w.r.t. x_out / skips_out; dx_out
 *     may be NULL) and the saved z -- the two 1x1 data gradients (K = 128), the out_mul / skip_mul scales and the
 *     tanh * sigmoid derivative; also writes go = out_mul * dx_out (the residual-path gradient and the out-conv
 *     weight-gradient operand; NULL with dx_out).
 *   data_backward: dx = dilated-conv data gradient of dz (+ go) and dc = aux 1x1 data gradient of dz (either may be NULL).
 * `packed_bwd`: pwg_wavenet_pack_weights_bwd image (depends on d->out_mul and d->skip_mul).                       */
size_t pwg_wavenet_packed_weight_bwd_floats(const pwg_wavenet_desc* d);
int pwg_wavenet_pack_weights_bwd(const pwg_wavenet_desc* d, const float* w_dil, const float* scale_dil, const float* w_aux,
                                 const float* scale_aux, const float* w_skip, const float* scale_skip, const float* w_out,
                                 const float* scale_out, float* packed, void* stream);
int pwg_wavenet_gate_backward(const pwg_wavenet_desc* d, const float* z, const float* dx_out, const float* ds_out,
                              const float* packed_bwd, float* dz, float* go, void* stream);
/* dc_accum (may be NULL, may alias dc): the gradient the LATER layers already accumulated for the shared aux features
 * c -- added in the epilogue, so the sum over the 30 layers needs no separate add launches.                          */
int pwg_wavenet_data_backward(const pwg_wavenet_desc* d, const float* dz, const float* go, const float* packed_bwd,
                              const float* dc_accum, float* dx, float* dc, void* stream);
/* The layer's parameter gradients in three launches: two contractions over time -- dz (128 rows) against the three
 * tap windows of x and c (272 rows), and [gs = skip_mul * ds_out ; go] (128 rows) against the saved gate output g (64
 * rows) -- into per-slice slabs, and one finish kernel that sums the slices in a fixed order and writes, per
 * convolution (grads[0..3] = dilated, aux, skip, out; torch weight layouts (rows, in, k)): the weight gradient (v NULL)
 * or, for a weight-normalised convolution w = g v / |v|, the gradients w.r.t. v and g; and the bias gradient.
 * go and grads[3].dw are NULL together (last layer); dg / db may be NULL.  Deterministic.                            */
typedef struct pwg_wavenet_param_grad {
  const float* v;  /* weight-norm direction tensor (shape of the weight), or NULL for a plain weight */
  const float* g;  /* weight-norm magnitudes (rows), NULL iff v is NULL */
  float* dw;       /* out: gradient w.r.t. the weight (v NULL) or w.r.t. v */
  float* dg;       /* out: gradient w.r.t. g, or NULL */
  float* db;       /* out: bias gradient, or NULL */
} pwg_wavenet_param_grad;
size_t pwg_wavenet_weight_backward_workspace_floats(const pwg_wavenet_desc* d);
int pwg_wavenet_weight_backward(const pwg_wavenet_desc* d, const float* dz, const float* x, const float* c, const float* gs,
                                const float* go, const float* g, const pwg_wavenet_param_grad* grads, float* workspace,
                                size_t workspace_floats, void* stream);
/* Diagnostics, host only: how the two contraction launches of `d` cut the flattened (item, 32-column chunk) range into
 * slices -- out[0..3] = {slices, chunks per slice} of the dil+aux launch, then of the skip+out launch -- by the rule the
 * launch and the workspace query use.  The workspace holds slices0 slabs of [128][273] floats, then slices1 slabs of
 * [128][65]: per slab row the contraction's columns ([tap0 x | tap1 x | tap2 x | c], or g) and the row sum of the
 * 128-row operand.  Launches nothing; an unsupported descriptor is refused as pwg_wavenet_weight_backward refuses it.
 * Purely additive -- no existing signature or behaviour changes -- so pwg_abi_version() stays 15. */
int pwg_wavenet_weight_backward_plan(const pwg_wavenet_desc* d, int32_t out[4]);

/* Old-style torch.nn.utils.weight_norm (dim=0) scale: scale[i] = g[i]/||v[i,...]||_2
 * replaces torch._weight_norm at every conv call site.
 * v: (n0, inner) flattened, g: (n0).                                          */
int pwg_weight_norm_scale(const float* v, const float* g, float* scale, int32_t n0,
                          int32_t inner, void* stream);
/* w = v * scale[dim0]  (materialises the torch-format weight, e.g. for
 * remove_weight_norm(): models/hifigan.py:209-219)                            */
int pwg_scale_rows(const float* v, const float* scale, float* w, int32_t n0, int32_t inner,
                   void* stream);

/* ------------------------------------------------------------------------- */
/* Activation / reparametrisation backward                                     */
/* ------------------------------------------------------------------------- */
/* dx = dy * scale * act'(.), act' written in terms of the activation OUTPUT y
 * (tanh: 1-y^2; leaky_relu: y>0 ? 1 : slope; relu: y>0).  Replaces the autograd
 * nodes of torch.nn.Tanh / LeakyReLU at models/hifigan.py:150, :329 etc.        */
int pwg_act_backward(const float* dy, const float* y, float* dx, int64_t n, int32_t act, float slope,
                     float scale, void* stream);
/* y = ((a + b) + c) / div (c may be NULL): the MRF combine `cs += block(c); c = cs / num_blocks`
 * (models/hifigan.py:186-190) when the residual blocks run as parallel graph branches.   */
int pwg_add3_div(const float* a, const float* b, const float* c, float* y, int64_t n, float div, void* stream);
/* Backward of old-style weight_norm (dim 0): given dw (torch layout) returns dv, dg. */
int pwg_weight_norm_backward(const float* dw, const float* v, const float* g, float* dv, float* dg,
                             int32_t n0, int32_t inner, void* stream);
/* torch.nn.utils.spectral_norm (dim 0, one power iteration, eps 1e-12) as used by the first
 * HiFi-GAN scale discriminator (models/hifigan.py:613-621,750-754).  w_orig viewed as
 * (rows, cols) = (c_out, c_in/groups * k).  do_iter != 0 updates u (rows) and v (cols) in
 * place (training-mode forward); sigma[0] = u^T W v; w = w_orig / sigma.
 * tmp: max(rows, 32 * cols) floats of workspace (row-sliced partial sums of W^T u). */
int pwg_spectral_norm_forward(const float* w_orig, float* u, float* v, float* sigma, float* w, float* tmp,
                              int32_t rows, int32_t cols, int32_t do_iter, float eps, void* stream);
/* The same, also leaving this forward's u / v in u_saved (rows) / v_saved (cols): the copies torch's hook takes for the
 * backward pass (torch/nn/utils/spectral_norm.py compute_weight: `u.clone()`, `v.clone()`), written by the iteration's own
 * kernels; fewer dependent launches (ABI v11).  u_saved == u / v_saved == v is allowed when do_iter == 0.  */
int pwg_spectral_norm_forward_saved(const float* w_orig, float* u, float* v, float* sigma, float* w, float* tmp,
                                    float* u_saved, float* v_saved, int32_t rows, int32_t cols, int32_t do_iter,
                                    float eps, void* stream);
/* dw_orig = dw / sigma - (<dw, w_orig> / sigma^2) u v^T ;  scratch: PWG_SPECTRAL_NORM_SCRATCH_FLOATS floats
 * (the dot product is summed through per-block shares in a fixed order: no atomics).  */
#define PWG_SPECTRAL_NORM_SCRATCH_FLOATS 257
int pwg_spectral_norm_backward(const float* dw, const float* w_orig, const float* u, const float* v,
                               const float* sigma, float* dw_orig, float* scratch, int32_t rows,
                               int32_t cols, void* stream);

/* ------------------------------------------------------------------------- */
/* Parallel WaveGAN specific element-wise stages                               */
/* ------------------------------------------------------------------------- */
/* WaveNet gate: out = tanh(z[:, :C]) * sigmoid(z[:, C:]); z (B, 2C, T), out (B, C, T)
 * (layers/residual_block.py:120-132).                                           */
int pwg_gate_forward(const float* z, float* out, int32_t batch, int32_t channels, int64_t t, void* stream);
int pwg_gate_backward(const float* z, const float* dout, float* dz, int32_t batch, int32_t channels,
                      int64_t t, void* stream);
/* One stage of the mel upsampler: F.interpolate(nearest, x scale) followed by the
 * (freq_kernel, 2*scale+1) single-channel Conv2d over (mel channel, time), fused
 * (layers/upsample.py:43-45,88-103,121-127):
 *   y[b][c][t] = sum_f sum_j w[f][j] * x[b][c + f - (F-1)/2][(t + j - pad_left) / scale],
 * rows = B * channels (zero padding on the channel axis; freq_kernel = 1 is the shipped recipes' case);
 * pad_left = scale (centred) or 2*scale (use_causal_conv: :96-99,121-125, output trimmed
 * to the stretched length).  `act` / `slope`: the optional nonlinearity after the stage (:105-110), applied in the
 * epilogue; its backward is pwg_act_backward on the stage output, then pwg_stretch_conv_backward.  The weight
 * gradient is summed through per-block shares in `workspace` in a fixed order (no atomics).           */
#define PWG_STRETCH_CONV_WGRAD_BLOCKS 512
int pwg_stretch_conv_forward(const float* x, const float* w, float* y, int64_t rows, int32_t t_in,
                             int32_t scale, int32_t kernel, int32_t pad_left, int32_t channels,
                             int32_t freq_kernel, int32_t act, float slope, void* stream);
/* The causal stage (kernel 2*scale+1, pad_left 2*scale, freq_kernel 1) on the next n input columns of a stream:
 *   y[r][t] = act(sum_j w[j] * X[r][floor((t + j - 2*scale) / scale)]),  t in [0, n*scale),
 *   X = concat(hist_in (rows, 2), x (rows, n)); hist_in == NULL: zeros (start of stream = the stage's zero padding).
 * One launch writes y (rows, n*scale) and hist_out (rows, 2) = the last 2 columns of X (also for n = 1).  hist_in and
 * hist_out must be distinct buffers.  Fixed j-ascending sum order: partitions of a stream agree bit for bit.
 * freq_kernel != 1 is refused (pwg_last_error names the reason).  Purely additive.                              */
int pwg_stretch_conv_stream(const float* x, const float* hist_in, float* hist_out, const float* w, float* y,
                            int64_t rows, int32_t n, int32_t scale, int32_t freq_kernel, int32_t act, float slope,
                            void* stream);
/* The NON-causal stage (pad_left = scale) in a stream with a fixed look-ahead: it is the causal stage above on a time
 * axis shifted by `scale` columns, same weights.  pwg_stretch_conv_stream plus a valid window: output columns outside
 * [valid_lo, valid_hi) (chunk-relative, of n*scale) are STORED as 0.0f -- the stage has no bias and act(0) = 0, yet the
 * `scale` columns around the utterance are not zero by themselves.  With the window [0, n*scale) y and hist_out are
 * pwg_stretch_conv_stream's bit for bit.
 * pwg_delay_line_forward: X = concat(line_in (rows, columns), x (rows, n)), line_in == NULL: zeros; line_out (rows,
 * columns) = the last `columns` columns of X, also when n < columns; delayed_out (rows, n), if not NULL, = the first n
 * columns of X (x, `columns` columns late).  line_in and line_out must be distinct buffers; delayed_out must not alias
 * x.  It only copies: exact.  (The noise line and the conditioning line of the Parallel WaveGAN look-ahead stream.)
 * These two symbols are purely additive -- no existing signature or behaviour changes -- so pwg_abi_version() stays 15. */
int pwg_stretch_conv_stream_delayed(const float* x, const float* hist_in, float* hist_out, const float* w, float* y,
                                    int64_t rows, int32_t n, int32_t scale, int32_t freq_kernel, int32_t act, float slope,
                                    int32_t valid_lo, int32_t valid_hi, void* stream);
int pwg_delay_line_forward(const float* x, const float* line_in, float* line_out, float* delayed_out, int64_t rows,
                           int32_t n, int32_t columns, void* stream);
/* The slotted forms of the two entries above (utils.PWGStreamPool): `items` items of `channels` rows
 * each stand where `rows` stood, and `slots` -- the DEVICE table of pwg_conv1d_stream_slots_forward, one row per item,
 * same flags and window rule -- stands where the window stood.
 * pwg_stretch_conv_stream_slots replaces pwg_stretch_conv_stream_delayed: a running item is that launch of its rows with
 * the window of (`rate` output columns per frame, output `delay`); a fresh item reads hist_in as zeros; a paused item's y
 * columns are 0.0f and its hist_out is its hist_in (zeros if fresh).
 * pwg_delay_line_slots_forward replaces pwg_delay_line_forward (which has no window, so this takes the table alone): a
 * fresh item's line reads as zeros; a paused item's line is copied through and its delayed_out columns are 0.0f.
 * pwg_slot_seed_history replaces the host-side replication of conv_in's first frame (ConvInUpsampleNetwork.
 * lookahead_forward): every item that is fresh and not paused gets column 0 of its x (items, channels, n) in all `columns`
 * columns of its hist (items, channels, columns); every other item's hist is left untouched.
 * hist_in / line_in must be given (the start of a stream is an item's); up to 65535 items.  Copies and the stage's own
 * fmaf chain: bit for bit the lock-step entries.
 * These three symbols are purely additive -- no existing signature or behaviour changes -- so pwg_abi_version() stays 15. */
int pwg_stretch_conv_stream_slots(const float* x, const float* hist_in, float* hist_out, const float* w, float* y,
                                  int64_t items, int32_t channels, int32_t n, int32_t scale, int32_t freq_kernel,
                                  int32_t act, float slope, const int32_t* slots, int32_t rate, int32_t delay, void* stream);
int pwg_delay_line_slots_forward(const float* x, const float* line_in, float* line_out, float* delayed_out, int64_t items,
                                 int32_t channels, int32_t n, int32_t columns, const int32_t* slots, void* stream);
int pwg_slot_seed_history(const float* x, float* hist, int64_t items, int32_t channels, int32_t n, int32_t columns,
                          const int32_t* slots, void* stream);
size_t pwg_stretch_conv_backward_workspace_floats(int32_t kernel, int32_t freq_kernel);
int pwg_stretch_conv_backward(const float* dy, const float* x, const float* w, float* dx, float* dw,
                              int64_t rows, int32_t t_in, int32_t scale, int32_t kernel, int32_t pad_left,
                              int32_t channels, int32_t freq_kernel, float* workspace, size_t workspace_floats,
                              void* stream);
/* Pseudo-QMF filterbank as polyphase kernels (layers/pqmf.py:120-149; csrc/pqmf.hip), 1 <= subbands <= 8:
 *   down:  y[b][k][i] = sum_j  h[k][j]               * x[b][i K + j - pad]     x (B, 1, t_in) -> y (B, K, n_out)
 *   up:    x[b][t]    = sum_k sum_i g[k][t + pad - i K] * y[b][k][i]           y (B, K, n_in) -> x (B, 1, t_out)
 * (zero outside the signals).  PQMF.analysis = down with h = analysis_filter, pad = taps / 2,
 * n_out = floor(T / K) for ANY T (the reference's stride-K pick after the full-rate FIR, pqmf.py:120-131);
 * PQMF.synthesis = up with g[k][m] = K * synthesis_filter[k][taps - m], t_out = K * n_in (pqmf.py:133-149).
 * Each is the adjoint of the other with the same filter, which is how the backward passes run.  */
int pwg_pqmf_down(const float* x, const float* h, float* y, int32_t batch, int64_t t_in, int64_t n_out,
                  int32_t subbands, int32_t len, int32_t pad, void* stream);
int pwg_pqmf_up(const float* y, const float* g, float* x, int32_t batch, int64_t n_in, int64_t t_out,
                int32_t subbands, int32_t len, int32_t pad, void* stream);

/* ---- stateful streaming form of PQMF.synthesis (csrc/pqmf.hip; ABI v15) ----
 * `up` with g[k][m] = K * synthesis_filter[k][taps - m] (layers/pqmf.py:133-149), evaluated WHILE the sub-band columns
 * arrive.  In groups ("positions") of K output samples, position q reads the columns q + d, d in [dlo, dhi] =
 * [ceil((pad - len + 1) / K), floor((K - 1 + pad) / K)], so a stream emits position q once column q + dhi is there:
 * a fixed delay of D = dhi columns (K * D samples; 8 columns = 32 samples for K = 4, taps = 62) and a history of
 * H = dhi - dlo raw columns per band (15).  pwg_pqmf_up_stream_geometry returns H and D (pure host logic).
 * One launch: the window is concat(hist_in (batch, K, H), y (batch, K, n)); hist_in == NULL is the start of a stream
 * (zero context, which is what `up` pads).  It writes x (batch, K * n_emit) = the last n_emit positions complete in the
 * window, i.e. the chunk positions [n - D - n_emit, n - D) -- n_emit == n in steady state, max(0, n - D) at the start
 * of a stream, 0 (x may be NULL) while a stream has no more than D columns; 0 <= n_emit <= n -- and hist_out
 * (batch, K, H) = the last H columns of the window, also when n < H.  hist_in and hist_out must be distinct buffers.
 * D zero columns pushed at the end flush the tail.  Every output is one fma chain from 0 over (k ascending, column
 * ascending), the chain of `up`: for finite input the emissions of any partition of a stream, batched or not,
 * concatenate to the bits of pwg_pqmf_up on the whole signal.  No workspace, no atomics.  1 <= subbands <= 8. */
int pwg_pqmf_up_stream_geometry(int32_t subbands, int32_t len, int32_t pad, int32_t* hist_columns,
                                int32_t* delay_columns);
int pwg_pqmf_up_stream(const float* y, const float* hist_in, float* hist_out, const float* g, float* x, int32_t batch,
                       int64_t n, int64_t n_emit, int32_t subbands, int32_t len, int32_t pad, void* stream);

/* pwg_pqmf_up_stream with a position per item, for a pool of multi-band MelGAN streams (utils.MelGANStreamPool,
 * DESIGN.md s11.12; the same synthesis of layers/pqmf.py:133-149).  `slots` is the DEVICE table of
 * pwg_conv1d_stream_slots_forward, one row per item; only "fresh" (slots[4b] == 0) and "paused" are read.  The launch
 * always emits n_emit = n positions, the chunk positions [-D, n - D) -- every column they read lies in [-H, n) -- into
 * x (batch, K * n).  A running item is pwg_pqmf_up_stream with n_emit = n on the item alone, bit for bit, with hist_in
 * NULL if the item is FRESH (whatever its buffer holds).  A PAUSED item's hist_out is its hist_in copied through (zeros
 * if it is fresh), its x columns are stored as 0.0f and its y columns are not read.  The generator stores exact zeros
 * around each utterance, which is the padding `up` applies, so the synthesis needs no window; the first D positions of a
 * fresh item lie before its stream and are the caller's to drop.  hist_in is required (where H > 0), hist_in and
 * hist_out must be distinct, slots must be given.  Additive: pwg_abi_version() stays 15. */
int pwg_pqmf_up_stream_slots(const float* y, const float* hist_in, float* hist_out, const float* g, float* x,
                             const int32_t* slots, int32_t batch, int64_t n, int32_t subbands, int32_t len, int32_t pad,
                             void* stream);

/* ---- StyleMelGAN pieces (layers/tade_res_block.py, models/style_melgan.py) ---- */
/* torch.nn.InstanceNorm1d(affine=False) over `rows` = B*C rows of t samples (tade_res_block.py:27,66):
 * y = (x - mean) / sqrt(var + eps) with the biased variance; mean / rstd (rows floats each) are kept
 * for the backward: dx = rstd * (dy - mean(dy) - y * mean(dy * y)).                              */
int pwg_instance_norm_forward(const float* x, float* y, float* mean, float* rstd, int64_t rows, int32_t t,
                              float eps, void* stream);
int pwg_instance_norm_backward(const float* dy, const float* y, const float* rstd, float* dx, int64_t rows,
                               int32_t t, void* stream);
/* torch.nn.Upsample(scale_factor, mode="nearest") along time (+ optional addend of the output shape,
 * the `upsample(residual) + x` of tade_res_block.py:161): y[r][t] = x[r][t / scale] (+ add[r][t]). */
int pwg_upsample_nearest_forward(const float* x, const float* add, float* y, int64_t rows, int32_t t_in,
                                 int32_t scale, void* stream);
int pwg_upsample_nearest_backward(const float* dy, float* dx, int64_t rows, int32_t t_in, int32_t scale,
                                  void* stream);
/* TADE modulation (tade_res_block.py:69-72): cg (B, 2C, t_in*scale), xn (B, C, t_in):
 * y[b][c][t] = cg[b][c][t] * xn[b][c][t / scale] + cg[b][C + c][t].                              */
int pwg_tade_modulate_forward(const float* xn, const float* cg, float* y, int32_t batch, int32_t channels,
                              int32_t t_in, int32_t scale, void* stream);
int pwg_tade_modulate_backward(const float* dy, const float* xn, const float* cg, float* dxn, float* dcg,
                               int32_t batch, int32_t channels, int32_t t_in, int32_t scale, void* stream);
/* Gated activation of TADEResBlock (tade_res_block.py:151-158): z (B, 2C, T) -> y (B, C, T),
 * y = softmax_over_channels(z[:, :C]) * tanh(z[:, C:])  (use_softmax != 0) or sigmoid(.) * tanh(.). */
int pwg_softmax_gate_forward(const float* z, float* y, int32_t batch, int32_t channels, int64_t t,
                             int32_t use_softmax, void* stream);
int pwg_softmax_gate_backward(const float* z, const float* dy, float* dz, int32_t batch, int32_t channels,
                              int64_t t, int32_t use_softmax, void* stream);
/* The ragged forms of the four forwards above (csrc/tade_ragged.hip): the TADE stages of tade_res_block.py over a batch
 * whose items have their own lengths, the batched form of the loop of bin/decode.py:214-243.  frames: device int32
 * (batch,); item b ends at column e = min(frames[b] * rate, t) of its rows (rate_out and t = t_in * scale for the two
 * that upsample: the table counts columns of the OUTPUT), t stays the row stride.  Nothing at or past e is read (NaN
 * may sit there), every column in [e, t) is stored as +0.0f, e == 0 stores an all-zero item, a workgroup whose columns
 * all lie at or past e only stores zeros, and the columns < e are bit for bit what the plain entry gives on the item
 * alone, a contiguous (1, channels, e) tensor; the instance norm's statistics run over [0, e) in the plain kernel's
 * order and it keeps no mean / rstd (forward only).  add may be NULL.  Nothing on the host depends on the table's
 * values: a captured launch serves every set of lengths.  Refused as pwg_zero_tail refuses (a message in
 * pwg_last_error, nothing launched): NULL or misaligned (4 B) pointers, rate <= 0, batch or channels outside
 * 1 .. 65535, rows of 2^31 columns or more.  Additive: pwg_abi_version() stays 15. */
int pwg_instance_norm_ragged(const float* x, float* y, const int32_t* frames, int32_t batch, int32_t channels,
                             int32_t t, int32_t rate, float eps, void* stream);
int pwg_upsample_nearest_ragged(const float* x, const float* add, float* y, const int32_t* frames, int32_t batch,
                                int32_t channels, int32_t t_in, int32_t scale, int32_t rate_out, void* stream);
int pwg_tade_modulate_ragged(const float* xn, const float* cg, float* y, const int32_t* frames, int32_t batch,
                             int32_t channels, int32_t t_in, int32_t scale, int32_t rate_out, void* stream);
int pwg_softmax_gate_ragged(const float* z, float* y, const int32_t* frames, int32_t batch, int32_t channels,
                            int64_t t, int32_t rate, int32_t use_softmax, void* stream);

/* ---- UHiFiGAN pieces (models/uhifigan.py) ---- */
/* One operand of torch.cat(dim=1) (uhifigan.py:286): y (batch, c_dst, t)[:, c_off : c_off + c_src] = x
 * (batch, c_src, t); reverse != 0 copies that slice of y back into x (the concatenation's backward). */
int pwg_copy_channels(float* x, float* y, int32_t batch, int32_t c_src, int32_t c_dst, int32_t c_off,
                      int64_t t, int32_t reverse, void* stream);
/* torch.nn.Dropout in training mode (uhifigan.py:86,130): y = x * keep / (1 - p) with a counter-based
 * mask hash(seed + *seed_dev, index) >= p * 2^32; calling it again with the same seeds on the output
 * gradient is the backward.  seed_dev (optional device scalar) lets a captured hipGraph draw a new mask
 * at every replay.  (Different random stream than torch's Philox: same distribution, other draws.)    */
int pwg_dropout(const float* x, float* y, int64_t n, float p, uint64_t seed, const uint64_t* seed_dev,
                void* stream);

/* ---- training input assembly (bin/train.py:646-896 Collater, mel -> waveform branch) ---- */
/* Random-crop batch from a device-resident corpus: audio / mel are the utterances concatenated
 * (mel row-major (frames, channels)), *_off their start offsets (elements / frames), audio_len the
 * waveform lengths.  For item b of utterance utt[b] and start frame start[b]:
 *   y (batch, 1, steps)                 = audio[start*hop : start*hop + steps]   (edge-padded)
 *   c (batch, channels, frames_ctx)     = mel[start - acw : start - acw + frames_ctx]^T
 * with frames_ctx = steps/hop + 2*acw.  The start frames are drawn by the caller.     */
int pwg_gather_crop(const float* audio, const int64_t* audio_off, const int64_t* audio_len, const float* mel,
                    const int64_t* mel_off, const int32_t* utt, const int32_t* start, float* y, float* c,
                    int32_t batch, int32_t steps, int32_t hop, int32_t frames_ctx, int32_t acw,
                    int32_t channels, void* stream);

/* ---- inference I/O helpers (around bin/decode.py:214-243) ---- */
/* pcm[i] = (int16) rint(clamp(x[i], -1, 1) * 32767): the PCM_16 conversion of the synthesised wave. */
int pwg_wave_to_pcm16(const float* x, int16_t* pcm, int64_t n, void* stream);
/* y (batch, channels, frames) = (x (batch, frames, channels) - mean[c]) / scale[c]: the
 * `normalize_before` step of `inference` (models/hifigan.py:262-266) fused with its transpose;
 * mean/scale may both be NULL (transpose only).                                       */
int pwg_normalize_transpose(const float* x, const float* mean, const float* scale, float* y,
                            int32_t batch, int32_t frames, int32_t channels, void* stream);
/* Ragged batches (utterances of different lengths in one forward; the batched form of the loop of
 * bin/decode.py:214-243): y (batch, channels, t), frames device int32 (batch,), rate = columns of y per frame.  Stores
 * 0.0f at the columns >= min(frames[b] * rate, t) of every row of item b; write-only (y may hold anything there, NaN
 * included), the columns below are not touched.  16-B stores where a row's tail allows (rows of odd t are not 16-B
 * aligned), scalar stores at the ragged head and end; a workgroup whose columns lie inside the item returns at once,
 * so the cost follows the padding.  Run behind any convolution launch it re-establishes the invariant of a ragged
 * forward: item b of a tensor at rate r is exactly zero at every column >= frames[b] * r.  Refused with a message,
 * launching nothing: NULL or misaligned (4 B) y / frames, rate <= 0, batch outside 1 .. 65535. */
int pwg_zero_tail(float* y, const int32_t* frames, int32_t batch, int32_t channels, int64_t t, int32_t rate,
                  void* stream);
/* pwg_zero_tail with the mirror the next reflect-padded consumer reads (the per-item ReflectionPad1d of
 * models/melgan.py:71,136 and layers/residual_stack.py:49 inside the batched form of the loop of
 * bin/decode.py:214-243): with e = min(frames[b] * rate, t), column e + j (0 <= j < pad, e + j < t) receives
 * y[b][c][e - 2 - j] and every column >= e + pad receives 0.0f; in place (sources lie below e, destinations at or
 * above it).  pad = 0 stores what pwg_zero_tail stores; e = 0 zeroes the item; a source index below 0 (e <= pad:
 * reflection is undefined) is clamped to 0 -- unspecified values, no access outside the tensor.  Refused as
 * pwg_zero_tail refuses, plus pad < 0.  Additive: pwg_abi_version() stays 15. */
int pwg_mirror_tail(float* y, const int32_t* frames, int32_t batch, int32_t channels, int64_t t, int32_t rate,
                    int32_t pad, void* stream);

/* ------------------------------------------------------------------------- */
/* Pooling / explicit padding                                                  */
/* ------------------------------------------------------------------------- */
/* torch.nn.AvgPool1d over `rows` rows (models/hifigan.py:773-775: k4 s2 p2,
 * count_include_pad=1; models/melgan.py:409-414: k4 s2 p1 count_include_pad=0).   */
int pwg_avg_pool1d_forward(const float* x, float* y, int64_t rows, int32_t t_in, int32_t t_out,
                           int32_t kernel, int32_t stride, int32_t pad, int32_t count_include_pad,
                           void* stream);
int pwg_avg_pool1d_backward(const float* dy, float* dx, int64_t rows, int32_t t_in, int32_t t_out,
                            int32_t kernel, int32_t stride, int32_t pad, int32_t count_include_pad,
                            void* stream);
/* F.pad(x, (pad_left, pad_right), mode) for mode = PWG_PAD_* (period discriminator tail,
 * models/hifigan.py:365-368; MelGAN ReflectionPad1d when training).                */
int pwg_pad1d_forward(const float* x, float* y, int64_t rows, int32_t t_in, int32_t pad_left,
                      int32_t pad_right, int32_t mode, void* stream);
int pwg_pad1d_backward(const float* dy, float* dx, int64_t rows, int32_t t_in, int32_t pad_left,
                       int32_t pad_right, int32_t mode, void* stream);

/* ------------------------------------------------------------------------- */
/* Spectral losses: torch.stft(center=True, reflect) is computed as            */
/*   frame_fold  (B,T) -> (B, hop, n_cols):  y[b][c][n] = reflect_pad(x)[n*hop+c] */
/*   conv1d      Cin = hop, Cout = 2*bins, k = ceil(win/hop)  (windowed DFT basis  */
/*               as the weight; runs on the MFMA conv kernel above)               */
/*   stft_mag    sqrt(max(re^2+im^2, eps))                                        */
/* replacing losses/stft_loss.py:16-40 and losses/mel_loss.py:95-110.             */
/* ------------------------------------------------------------------------- */
int pwg_frame_fold_forward(const float* x, float* y, int32_t batch, int32_t t, int32_t pad, int32_t hop,
                           int32_t n_cols, void* stream);
int pwg_frame_fold_backward(const float* dy, float* dx, int32_t batch, int32_t t, int32_t pad,
                            int32_t hop, int32_t n_cols, void* stream);
/* spec: (B, 2*bins, frames), rows [0,bins) real, [bins,2*bins) imaginary.         */
int pwg_stft_mag_forward(const float* spec, float* mag, int32_t batch, int32_t bins, int32_t frames,
                         float eps, void* stream);
int pwg_stft_mag_backward(const float* spec, const float* mag, const float* dmag, float* dspec,
                          int32_t batch, int32_t bins, int32_t frames, float eps, void* stream);
/* y = log(max(x, eps)) / log_div  (log_div = 1, ln2, ln10: losses/mel_loss.py:71-79,108-110) */
int pwg_log_clamp_forward(const float* x, float* y, int64_t n, float eps, float log_div, void* stream);
int pwg_log_clamp_backward(const float* x, const float* dy, float* dx, int64_t n, float eps, float log_div,
                           void* stream);

/* Fused single-resolution STFT loss of a (predicted, target) pair -- one launch instead of the
 * frame/conv/mag/log/reduce chain above, and no spectrum-shaped tensor in HBM:
 *   sums[0] = sum (|Y| - |X|)^2   sums[1] = sum |Y|^2   sums[2] = sum |log|Y| - log|X||
 * over the (B, bins, frames) magnitudes |.| = sqrt(max(re^2 + im^2, eps)), and the two losses themselves:
 *   sums[3] = SpectralConvergenceLoss = sqrt(sums[0]) / sqrt(sums[1])      (losses/stft_loss.py:61)
 *   sums[4] = LogSTFTMagnitudeLoss    = sums[2] / (B * bins * frames)      (:82)
 * (`sums`: 5 device floats); torch.stft + clamp + sqrt are :16-40.
 *   fx, fy : the two signals folded by pwg_frame_fold_forward, (B, hop, n_cols), n_cols >= frames + taps - 1
 *   basis  : windowed DFT image [tap][hop][m_pad], m_pad = 64 * ceil(bins / 32); each 64-row group holds
 *            32 cosine rows then the 32 matching -sine rows (rows of bins >= `bins` are zero)
 *   workspace: pwg_stft_loss_workspace_floats() floats.  Deterministic (fixed tiles, fixed sum order).
 * Backward: given the forward's `sums` and g2 = d loss / d (sums[3], sums[4]) (2 DEVICE floats) writes dspec
 * (B, 2*bins, frames) = [d re | d im]  (the gradient of sums[3] is 0 where sums[0] == 0, torch.norm's subgradient)
 * of the PREDICTED signal's spectrum (the target is a constant), i.e. the dy operand of
 * pwg_conv1d_backward_data on the DFT convolution; pwg_frame_fold_backward finishes the chain.        */
size_t pwg_stft_loss_workspace_floats(int32_t batch, int32_t bins, int32_t frames);
int pwg_stft_loss_forward(const float* fx, const float* fy, const float* basis, int32_t batch, int32_t hop,
                          int32_t n_cols, int32_t taps, int32_t bins, int32_t frames, float eps,
                          float* workspace, float* sums, void* stream);
int pwg_stft_loss_backward(const float* fx, const float* fy, const float* basis, int32_t batch, int32_t hop,
                           int32_t n_cols, int32_t taps, int32_t bins, int32_t frames, float eps,
                           const float* sums, const float* g2, float* dspec, void* stream);

/* ---- STFT loss through a radix-2 FFT in LDS (round 4; power-of-two n_fft in 256 .. 2048) ----
 * Same contract as pwg_stft_loss_forward / _backward (reference losses/stft_loss.py:16-40, :61, :82: torch.stft with
 * center=True / reflect padding / window zero-padded to n_fft, clamp 1e-7, sqrt, the two losses), computed from the raw
 * signals x (predicted), y (target), both (B, T): one complex FFT per frame carries both signals.  window: `win` floats;
 * twiddle: n_fft / 2 pairs (cos, -sin)(2 pi t / n_fft) (host float64 -> float32); sums: 5 floats [S_d, S_y, S_l, sc, mag].
 * Backward: g2 = upstream gradients of (sc, mag) on the device; dframes: scratch of B * (1 + T / hop) * win floats; dx (B, T). */
int pwg_stft_fft_supported(int32_t n_fft, int32_t win, int32_t hop);
size_t pwg_stft_fft_workspace_floats(int32_t batch, int32_t frames, int32_t n_fft);
int pwg_stft_fft_loss_forward(const float* x, const float* y, const float* window, const float* twiddle, int32_t batch,
                              int32_t t, int32_t n_fft, int32_t hop, int32_t win, float eps, float* workspace,
                              float* sums, void* stream);
int pwg_stft_fft_loss_backward(const float* x, const float* y, const float* window, const float* twiddle, int32_t batch,
                               int32_t t, int32_t n_fft, int32_t hop, int32_t win, float eps, const float* sums,
                               const float* g2, float* dframes, float* dx, void* stream);

/* Mel-spectrogram loss through the same FFT (reference losses/mel_loss.py:95-110, :150-165; eps = the module's 1e-10):
 * total[0] = sum_{b,j,f} | log(max(mel_x, eps)) - log(max(mel_y, eps)) | / log_div.  fb: filterbank [n_mels][bins_pad]
 * (bin fastest, bins_pad >= n_fft / 2 + 1); mel_range: per mel (first, last) bin of its non-zero support; bin_range: per
 * bin (first, last) mel covering it (int32 pairs).  workspace: pwg_stft_fft_workspace_floats() floats; dframes / dx as above. */
int pwg_mel_fft_loss_forward(const float* x, const float* y, const float* window, const float* twiddle, const float* fb,
                             const int32_t* mel_range, const int32_t* bin_range, int32_t batch, int32_t t, int32_t n_fft,
                             int32_t hop, int32_t win, int32_t n_mels, int32_t bins_pad, float eps, float log_div,
                             float* workspace, float* total, void* stream);
int pwg_mel_fft_loss_backward(const float* x, const float* y, const float* window, const float* twiddle, const float* fb,
                              const int32_t* mel_range, const int32_t* bin_range, int32_t batch, int32_t t, int32_t n_fft,
                              int32_t hop, int32_t win, int32_t n_mels, int32_t bins_pad, float eps, float log_div,
                              const float* gout, float* dframes, float* dx, void* stream);

/* Fused mel-spectrogram loss of a (predicted, target) pair (losses/mel_loss.py:95-110,150-165):
 *   sum[0] = sum_{b,j,f} | log(max(mel_x, eps)) - log(max(mel_y, eps)) | / log_div,
 *   mel = filterbank (n_mels x bins) applied to |STFT| = sqrt(max(re^2 + im^2, eps)); F.l1_loss is sum[0] / (B * n_mels * frames).
 * Same tiling and operands as pwg_stft_loss_*; the filterbank contraction runs on MFMA from the magnitude
 * registers.  mel_t: filterbank [32 * ceil(bins / 32)][mels_pad] (mel fastest, mels_pad = 32 * ceil(n_mels / 32),
 * zero padded); mel_b: the same matrix as [mels_pad][32 * ceil(bins / 32)] (bin fastest).  mel_x / mel_y
 * (B, n_mels, frames) receive the un-clamped mels (kept for the backward pass).  workspace:
 * pwg_mel_loss_workspace_floats() floats.  Backward writes dspec = [d re | d im] of the predicted signal.   */
size_t pwg_mel_loss_workspace_floats(int32_t batch, int32_t bins, int32_t frames, int32_t n_mels);
int pwg_mel_loss_forward(const float* fx, const float* fy, const float* basis, const float* mel_t, int32_t batch,
                         int32_t hop, int32_t n_cols, int32_t taps, int32_t bins, int32_t frames, int32_t n_mels,
                         float eps, float log_div, float* workspace, float* mel_x, float* mel_y, float* sum,
                         void* stream);
int pwg_mel_loss_backward(const float* fx, const float* basis, const float* mel_b, const float* mel_x,
                          const float* mel_y, int32_t batch, int32_t hop, int32_t n_cols, int32_t taps,
                          int32_t bins, int32_t frames, int32_t n_mels, float eps, float log_div,
                          const float* gout, float* dspec, void* stream);

/* ------------------------------------------------------------------------- */
/* Loss reductions (deterministic two-stage sums)                              */
/*   out[0] = scale * sum_i term_i ;  mode 0 |a-b| (F.l1_loss: feat_match_loss.py:44, */
/*   mel_loss.py:163, stft_loss.py:82), 1 (a-b)^2 and 2 a^2 (Frobenius norms,        */
/*   stft_loss.py:61), 3 (a-c)^2 (F.mse_loss against a constant: adversarial_loss.py */
/*   :54-58,113-123), 4 a.  workspace: >= 512 floats.                                */
/* ------------------------------------------------------------------------- */
/*   5 -min(a-1, 0) and 6 -min(-a-1, 0): the hinge terms of DiscriminatorAdversarialLoss            */
/*   (adversarial_loss.py:119-123; ties of the min get gradient 1/2 like torch.minimum).            */
enum { PWG_RED_ABS_DIFF = 0, PWG_RED_SQ_DIFF = 1, PWG_RED_SQ = 2, PWG_RED_SQ_DIFF_CONST = 3, PWG_RED_SUM = 4,
       PWG_RED_HINGE_REAL = 5, PWG_RED_HINGE_FAKE = 6 };
int pwg_reduce_forward(const float* a, const float* b, float c, int64_t n, int32_t mode, float scale,
                       float* out, float* workspace, void* stream);
/* da = gout[0] * scale * dterm/da (db = -da); gout is a DEVICE scalar.            */
int pwg_reduce_backward(const float* a, const float* b, float c, int64_t n, int32_t mode, float scale,
                        const float* gout, float* da, float* db, void* stream);

/* Multi-tensor form: the Python loops over discriminators x layers of FeatureMatchLoss.forward
 * (feat_match_loss.py:36-54) and of the adversarial losses (adversarial_loss.py:30-47,79-104) as ONE
 * launch pair:  out[slot] (+)= sum_items scale_item * sum_i term_mode(a_i, b_i | c).
 * `items` is a HOST array (<= PWG_RED_MAX_ITEMS entries; it is copied into the kernel arguments, so
 * a captured hipGraph keeps its own copy); workspace: pwg_multi_reduce_workspace_floats() floats.
 * accumulate != 0 adds to out[] (more than PWG_RED_MAX_ITEMS tensors = several calls).
 * Backward: da = gout[slot] * scale * dterm/da and db = -da into the items' da / db (NULL = skip). */
#define PWG_RED_MAX_ITEMS 64
typedef struct pwg_red_item {
  const float* a;
  const float* b;  /* second operand of the diff modes, else NULL                    */
  float* da;       /* backward only: gradient w.r.t. a (NULL = not needed)           */
  float* db;       /* backward only: gradient w.r.t. b (NULL = not needed)           */
  int64_t n;       /* elements                                                       */
  int32_t mode;    /* PWG_RED_*                                                      */
  int32_t slot;    /* which output scalar this item adds to                          */
  float scale;     /* e.g. 1/n for a mean, times the averaging weights               */
  float c;         /* constant of PWG_RED_SQ_DIFF_CONST                              */
} pwg_red_item;
size_t pwg_multi_reduce_workspace_floats(const pwg_red_item* items, int32_t n_items);
int pwg_multi_reduce_forward(const pwg_red_item* items, int32_t n_items, int32_t n_slots, float* out,
                             int32_t accumulate, float* workspace, void* stream);
int pwg_multi_reduce_backward(const pwg_red_item* items, int32_t n_items, int32_t n_slots, const float* gout,
                              void* stream);

/* ------------------------------------------------------------------------- */
/* Fused multi-tensor optimizer steps over a device table of chunks            */
/* (replaces the per-parameter Python loops of torch.optim.Adam and            */
/* optimizers/radam.py:27-99)                                    */
/* ------------------------------------------------------------------------- */
typedef struct pwg_opt_chunk {
  float* p;        /* parameter slice                                    */
  const float* g;  /* gradient slice                                     */
  float* m;        /* exp_avg                                            */
  float* v;        /* exp_avg_sq                                         */
  float* vmax;     /* max_exp_avg_sq (amsgrad) or NULL                   */
  int32_t n;       /* elements in this slice                             */
  int32_t pad_;
} pwg_opt_chunk;
/* `step` is the 1-based step count AFTER increment, as torch uses it for bias correction;
 * gradients are multiplied by grad_scale first (1/world_size after a sum all-reduce).
 * pwg_adam_step*: weight_decay > 0 is torch.optim.Adam's L2 form (g += wd * p); weight_decay < 0 selects
 * torch.optim.AdamW's DECOUPLED decay of magnitude |weight_decay| (p *= 1 - lr * |wd| before the update).   */
int pwg_adam_step(const void* chunks, int32_t n_chunks, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int32_t step, float grad_scale, void* stream);
int pwg_radam_step(const void* chunks, int32_t n_chunks, float lr, float beta1, float beta2, float eps,
                   float weight_decay, int32_t step, float grad_scale, void* stream);
/* hipGraph-friendly variants: the scalars come from 8 floats in DEVICE memory
 *   [lr, beta1, beta2, eps, weight_decay, step_size, aux, grad_scale]
 * (Adam: step_size = lr/(1-beta1^t), aux = sqrt(1-beta2^t); RAdam: step_size per radam.py:63-86
 * incl. lr, aux = 1 when rectified), refreshed by the host between graph replays.     */
int pwg_adam_step_dev(const void* chunks, int32_t n_chunks, const float* hyper, void* stream);
int pwg_radam_step_dev(const void* chunks, int32_t n_chunks, const float* hyper, void* stream);
/* torch.nn.utils.clip_grad_norm_ (bin/train.py:289-293,329-333): out[0] = total L2 norm,
 * out[1] = applied coefficient; gradients are scaled in place.  workspace >= n_chunks floats. */
int pwg_clip_grad_norm(const void* chunks, int32_t n_chunks, float max_norm, float* out, float* workspace,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PWG_KERNELS_H_ */
