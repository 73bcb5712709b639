/*
 * pcgan_hip.h -- C-ABI of libpcgan_hip.so: the MI355X (gfx950) kernels behind the
 * PC-GAN wsgan_emb training step.
 *
 * The reference (phymhan pc-gan) has no FFI: every op on the hot path is a stock
 * torch.nn module.  Each entry point below therefore names the
 * torch.nn call site in the reference that it replaces (file:line relative to the
 * reference root).  The host side (pc-gan_amd/hip/*.py) binds these with ctypes and
 * wraps them in torch.autograd.Function objects used by the define_G/define_D/
 * define_E/define_IP modules.
 *
 * Conventions
 *   - tensors are NCHW, contiguous, device pointers (tensor.data_ptr()).  ACTIVATION tensors (and their gradients) are
 *     `void*` of the storage type named by the call's `dtype` argument / the descriptor's `dtype` field (PCGAN_F32 or
 *     PCGAN_BF16); everything typed `float*` -- parameters, parameter gradients, biases, statistics, losses, optimizer
 *     state -- is fp32 in either mode, and all arithmetic accumulates in fp32.
 *   - no hidden allocation, no device synchronisation, NO ENVIRONMENT VARIABLES (round 4: the 14 getenv reads of round 3
 *     are gone): the caller provides the workspace (query *_workspace_bytes first) and the hipStream_t
 *     (torch.cuda.current_stream().cuda_stream); every launch is asynchronous on that stream, so calls are
 *     graph-capturable and may run concurrently on distinct streams.  The library's ENTIRE process-global state is the three
 *     items declared at the end of this header, each set only by an explicit call: the routing options (pcgan_set_option:
 *     five integers with measured-best defaults), the non-finite sentinel pointer (pcgan_set_nonfinite_counter) and the
 *     measurement-only kernel timer (pcgan_timer_enable).  Nothing else is mutable between calls.
 *   - return value 0 = ok; non-zero = error, text via pcgan_last_error()
 *     (thread-local).  The Python side turns non-zero into RuntimeError.
 */
#ifndef PCGAN_HIP_H
#define PCGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* pcgan_stream_t; /* hipStream_t */

/* ---- status ------------------------------------------------------------------ */
const char* pcgan_last_error(void);
int pcgan_version(void);
/* number of compute units / arch string of device 0 (diagnostics) */
int pcgan_device_info(int* cu_count, char* arch, int arch_len);

/* ---- convolution family ------------------------------------------------------
 * One descriptor covers nn.Conv2d and (with the roles swapped by the caller)
 * nn.ConvTranspose2d.  Replaces:
 *   ResnetGenerator convs      models/networks.py:578-605
 *   ResnetBlock convs          models/networks.py:621-648 (ReflectionPad2d folded in)
 *   NLayerDiscriminator convs  models/networks.py:747-772
 *   ResNet-18 / Elo head convs models/resnet.py:20-28,134 ; models/networks.py:1020-1026
 *   AlexNetFeature convs       models/networks.py:1223-1233
 * pad_mode: 0 = zero padding, 1 = reflection padding (ReflectionPad2d(pad) + conv pad 0).
 * stride must be 1, 2 or 4.
 */
typedef struct {
    int N, C, H, W; /* input  [N][C][H][W]            */
    int K, R, S;    /* weight [K][C][R][S]            */
    int stride, pad, pad_mode;
    int P, Q;       /* output [N][K][P][Q]            */
    int dtype;      /* storage type of x / y / dy / dx: PCGAN_F32 or PCGAN_BF16 (w, bias, dw are fp32)   */
} pcgan_conv_desc;

enum { PCGAN_ACT_NONE = 0, PCGAN_ACT_RELU = 1, PCGAN_ACT_LRELU = 2, PCGAN_ACT_TANH = 3, PCGAN_ACT_SIGMOID = 4 };
enum { PCGAN_PASS_FWD = 0, PCGAN_PASS_BWD_DATA = 1, PCGAN_PASS_BWD_WEIGHT = 2 };
/* storage type of ACTIVATION tensors (and of their gradients); parameters, parameter gradients, statistics, losses and
 * optimizer state are always fp32, accumulation is always fp32 */
enum { PCGAN_F32 = 0, PCGAN_BF16 = 1 };

size_t pcgan_conv2d_workspace_bytes(const pcgan_conv_desc* d, int pass);

/* y = act(conv(x, w) + bias); bias may be NULL. */
int pcgan_conv2d_fwd(const pcgan_conv_desc* d, const void* x, const float* w, const float* bias,
                     void* y, int act, float slope, void* ws, size_t ws_bytes, pcgan_stream_t s);
/* dx = conv^T(dy, w) (+ bias per dx-channel, used when this entry serves as the
 * forward of nn.ConvTranspose2d, models/networks.py:597-600). */
int pcgan_conv2d_bwd_data(const pcgan_conv_desc* d, const void* dy, const float* w, const float* bias,
                          void* dx, void* ws, size_t ws_bytes, pcgan_stream_t s);
/* Weight packing split out of the two calls above.  fwd/bwd_data re-tile w into the implicit-GEMM A
 * operand on every call (a few us, ~2 % of a step); weights only change once per optimizer step while the
 * reference's step runs each net 2-4 times (models/wsgan_emb_model.py:277-330), so the host can pack once
 * per (weight version, pass) and call the *_packed variants.  `packed` holds pcgan_conv2d_packed_bytes(d,
 * pass) bytes (0 for PCGAN_PASS_BWD_WEIGHT) and is valid for any desc that differs only in N (batch). */
size_t pcgan_conv2d_packed_bytes(const pcgan_conv_desc* d, int pass);
int pcgan_conv2d_pack_weights(const pcgan_conv_desc* d, int pass, const float* w, float* packed,
                              pcgan_stream_t s);
int pcgan_conv2d_fwd_packed(const pcgan_conv_desc* d, const void* x, const float* packed, const float* bias,
                            void* y, int act, float slope, void* ws, size_t ws_bytes, pcgan_stream_t s);
int pcgan_conv2d_bwd_data_packed(const pcgan_conv_desc* d, const void* dy, const float* packed,
                                 const float* bias, void* dx, void* ws, size_t ws_bytes, pcgan_stream_t s);
/* dw[K][C][R][S] (+)= sum_{n,p,q} dy * gather(x).  accumulate != 0 adds into dw -- used with dw = the
 * parameter's slice of the optimizer's flat gradient buffer, which fuses autograd's "grad += dw" pass. */
int pcgan_conv2d_bwd_weight(const pcgan_conv_desc* d, const void* x, const void* dy, float* dw, int accumulate,
                            void* ws, size_t ws_bytes, pcgan_stream_t s);

/* ---- per-channel reductions / pointwise ---------------------------------------- */
/* out[c] (+)= sum over n,h,w of x[n][c][h][w]  (bias gradients); scratch_nc: N*C floats. */
int pcgan_channel_sum(const void* x, float* out, float* scratch_nc, int N, int C, int HW, int accumulate, int dtype,
                      pcgan_stream_t s);
/* dx = dy * act'(y)  where y is the activation OUTPUT (relu/lrelu/tanh/sigmoid). */
int pcgan_act_bwd(const void* dy, const void* y, void* dx, size_t n, int act, float slope, int dtype, pcgan_stream_t s);
/* y = act(x) standalone (nn.ReLU in AlexNetFeature, models/networks.py:1224-1234). */
int pcgan_act_fwd(const void* x, void* y, size_t n, int act, float slope, int dtype, pcgan_stream_t s);
/* out[n][0..C)[hw] = img, out[n][C..C+nz)[hw] = z[n or 0][j] broadcast
 * (torch.cat((input, z_img), 1), models/networks.py:610-611, 781-782).  z_batch is 1 or N. */
int pcgan_concat_z(const void* img, const float* z, void* out, int N, int C, int nz, int HW, int z_batch, int dtype,
                   pcgan_stream_t s);
/* y = a + b; y = alpha * scalar_dev[0] * x (scalar_dev may be NULL): the upstream
 * gradient of a scalar loss stays on the device -- helpers for the autograd glue. */
int pcgan_add(const void* a, const void* b, void* y, size_t n, int dtype, pcgan_stream_t s);
int pcgan_scale(const void* x, const float* scalar_dev, float alpha, void* y, size_t n, int dtype, pcgan_stream_t s);
/* y = x converted between storage types (fp32 -> bf16: round to nearest even; the bf16 path's boundary: images in,
 * parity checks out). */
int pcgan_cast(const void* x, int dtype_x, void* y, int dtype_y, size_t n, pcgan_stream_t s);
/* Dropout2d with an explicit keep mask per (n,c) (models/resnet.py:38-51): y = x*mask[nc]*scale. */
int pcgan_channel_scale(const void* x, const float* mask_nc, void* y, int NC, int HW, float scale, int dtype,
                        pcgan_stream_t s);

/* ---- normalisation (+ fused activation / residual) -----------------------------
 * InstanceNorm2d(affine=False, track_running_stats=True)  models/networks.py:26
 * BatchNorm2d(affine=True) in train mode                   models/networks.py:24,
 *                                                          models/resnet.py:47-51,136
 * plane_stats: per (n,c) plane mean and M2 = sum (x-mean)^2 (exact two-pass). */
int pcgan_plane_stats(const void* x, float* mean_nc, float* m2_nc, int NC, int HW, int dtype, pcgan_stream_t s);
/* merge the N per-plane (mean,M2) of each channel (Chan's formula) into batch
 * statistics: mean_c, var_c (biased) and update running stats
 * (momentum m: r = (1-m) r + m stat, unbiased variance), either pointer may be NULL. */
int pcgan_bn_merge(const float* mean_nc, const float* m2_nc, float* mean_c, float* var_c,
                   float* running_mean, float* running_var, int N, int C, int HW, float momentum,
                   pcgan_stream_t s);
/* instance-norm running-stat update: r_mean = (1-m) r_mean + m * mean_n(mean_nc),
 * r_var = (1-m) r_var + m * mean_n(unbiased var_nc). */
int pcgan_in_running_update(const float* mean_nc, const float* m2_nc, float* running_mean,
                            float* running_var, int N, int C, int HW, float momentum, pcgan_stream_t s);
/* y = act( (x - mean[i]) * rsqrt(var[i] + eps) * gamma[c] + beta[c] + residual )
 * with i = n*C+c (per_plane=1, instance norm: `var` then holds the plane M2 from
 * pcgan_plane_stats and the kernel divides by HW) or i = c (per_plane=0, batch norm or
 * eval-mode running statistics: `var` is the variance).  gamma/beta/residual may be NULL. */
int pcgan_norm_act_fwd(const void* x, const float* mean, const float* var, const float* gamma,
                       const float* beta, const void* residual, void* y, float* y_pmax, int N, int C, int HW,
                       int per_plane, float eps, int act, float slope, int dtype, pcgan_stream_t s);
/* y_pmax / dx_pmax ([N*C], may be NULL) here and y_cmax / dx_cmax ([C], may be NULL) of the fused BatchNorm calls below receive
 * the largest magnitude of each output plane / channel: partial maxima for the fp16 route of the convolution that consumes the
 * tensor (pcgan_conv2d_fwd_packed_hsplit: x_amax, n_amax) -- no separate pcgan_absmax pass. */
/* backward statistics per plane: s1[nc] = sum g, s2[nc] = sum g*xhat where
 * g = dy * act'(y) (y = forward output, used only for the activation mask; may be NULL
 * when act == NONE). */
int pcgan_norm_bwd_stats(const void* dy, const void* x, const void* y, const float* mean,
                         const float* var, float* s1_nc, float* s2_nc, int N, int C, int HW,
                         int per_plane, float eps, int act, float slope, int dtype, pcgan_stream_t s);
/* dx = rstd*gamma*( g - s1/cnt - xhat*s2/cnt ); s1/s2 indexed like mean;
 * d_residual (optional) = g.  For batch norm the caller first sums s1/s2 over n
 * (pcgan_bn_bwd_reduce) which also yields dgamma, dbeta. */
int pcgan_norm_bwd_apply(const void* dy, const void* x, const void* y, const float* mean,
                         const float* var, const float* gamma, const float* s1, const float* s2,
                         void* dx, void* d_residual, float* dx_pmax, int N, int C, int HW, int per_plane, float eps,
                         int act, float slope, int dtype, pcgan_stream_t s);
int pcgan_bn_bwd_reduce(const float* s1_nc, const float* s2_nc, float* s1_c, float* s2_c, int N, int C,
                        pcgan_stream_t s);
/* The two-launch pairs above as ONE launch each, for train-mode BatchNorm2d on tensors too large for the fused kernels below
 * (the Elo encoder's 112^2 / 56^2 / 28^2 maps, the PatchGAN's 32^2 map at batch 32: models/resnet.py:47-71, models/networks.py:756-761).
 * pcgan_bn_stats_merged = pcgan_plane_stats + pcgan_bn_merge (+ num_batches_tracked += 1 when `batches` != NULL);
 * pcgan_bn_bwd_stats_reduced = pcgan_norm_bwd_stats(per_plane = 0) + pcgan_bn_bwd_reduce.  The workgroup whose plane completes a
 * channel ("last arriver", counted on ticket[c]) finishes that channel with the stand-alone kernels' arithmetic in their order, so the
 * results are the same bits.  ticket: C unsigned words owned by the caller, zeroed ONCE when the layer is created; the arrival that finds
 * old + 1 == N is the last of its call and stores 0 back, so every call starts from 0 whatever N the previous call had (partial last
 * batch of an epoch, test() at another batch size) and a captured graph replays; forward and backward use separate arrays; calls sharing an array must be
 * ordered (one stream, or stream dependencies) -- a BatchNorm layer's passes are ordered anyway for its running statistics. */
int pcgan_bn_stats_merged(const void* x, float* mean_nc, float* m2_nc, float* mean_c, float* var_c, float* running_mean,
                          float* running_var, long long* batches, unsigned int* ticket, int N, int C, int HW, float momentum, int dtype,
                          pcgan_stream_t s);
int pcgan_bn_bwd_stats_reduced(const void* dy, const void* x, const void* y, const float* mean_c, const float* var_c, float* s1_nc,
                               float* s2_nc, float* s1_c, float* s2_c, unsigned int* ticket, int N, int C, int HW, float eps, int act,
                               float slope, int dtype, pcgan_stream_t s);
/* BatchNorm2d in training mode for small tensors (used up to N * HW = 8192 per channel), ONE launch per pass: batch statistics,
 * running-statistics update (+ num_batches_tracked when `batches` != NULL), normalise + affine (+ residual) + activation
 * -- replaces nn.BatchNorm2d (+ the following ReLU / LeakyReLU) of the PatchGAN and of the Elo encoder's late stages
 * (models/networks.py:24-26, 756-771; models/resnet.py:58-71).  mean_c / var_c (biased) are kept for the backward pass;
 * backward returns s1_c = d(beta), s2_c = d(gamma) and dx (dx / dres may be NULL). */
int pcgan_bn_fwd_fused(const void* x, const float* gamma, const float* beta, const void* residual, void* y,
                       float* mean_c, float* var_c, float* running_mean, float* running_var, long long* batches, float* y_cmax,
                       int N, int C, int HW, float momentum, float eps, int act, float slope, int dtype, pcgan_stream_t s);
int pcgan_bn_bwd_fused(const void* dy, const void* x, const void* y, const float* mean_c, const float* var_c,
                       const float* gamma, void* dx, void* dres, float* s1_c, float* s2_c, float* dx_cmax, int N, int C, int HW,
                       float eps, int act, float slope, int dtype, pcgan_stream_t s);

/* Fused instance norm (the generator's 23 norm sites per pass, models/networks.py:580-601,633,646): the
 * (n,c) plane stays in registers, so forward = one read + one write (statistics + normalise + residual +
 * activation; mean / M2 are also returned for the backward and the running-stat update) and backward = one
 * read of dy, x (and y for the activation mask) + one write.  Planes that do not fit (HW % 4 != 0 or
 * HW > 65536) fall back to the two-pass kernels above; ws_s1s2 (2*N*C floats) is only used then. */
int pcgan_instnorm_fwd(const void* x, const void* residual, void* y, float* mean_nc, float* m2_nc, float* y_pmax, int N, int C,
                       int HW, float eps, int act, float slope, int dtype, pcgan_stream_t s);
int pcgan_instnorm_bwd(const void* dy, const void* x, const void* y, const float* mean_nc, const float* m2_nc,
                       void* dx, float* dx_psum, float* dx_pmax, float* ws_s1s2, int N, int C, int HW, float eps, int act,
                       float slope, int dtype, pcgan_stream_t s);
/* y_pmax / dx_pmax (may be NULL; register-resident kernels only, see pcgan_instnorm_fused): [N*C] floats that receive the largest
 * magnitude of each output plane -- the fp16 route of the convolution that consumes the tensor scales by the largest of them
 * (pcgan_conv2d_fwd_hsplit with n_amax = N*C), without a separate pcgan_absmax pass over the tensor. */
/* 1 when a plane of HW elements runs in the register-resident kernels.  Only then may pcgan_instnorm_bwd be given
 * dx_psum[N*C]: the sum of dx over each plane, taken from the registers that store dx.  The convolution in front of the
 * norm has its bias gradient = sum over n of these (reference: autograd of nn.Conv2d(bias=True) + nn.InstanceNorm2d,
 * models/networks.py:580-601, 621-648; true value 0, fp32 noise) -- pcgan_sum_planes finishes it without re-reading dx. */
int pcgan_instnorm_fused(int HW);
/* out[c] (+)= sum over n of part_nc[n*C + c]: second stage of pcgan_channel_sum on plane sums that already exist. */
int pcgan_sum_planes(const float* part_nc, float* out, int N, int C, int accumulate, pcgan_stream_t s);

/* ---- pooling / resize ------------------------------------------------------------
 * MaxPool2d(k, stride, pad)   models/resnet.py:138 ; models/networks.py:1225-1235
 * AvgPool2d(H) / MaxPool2d(H) global pooling  models/networks.py:1056-1059
 * F.interpolate(bilinear, align_corners=True)  util/util.py:111-117 */
int pcgan_maxpool_fwd(const void* x, void* y, int32_t* argmax, int NC, int H, int W, int k, int stride,
                      int pad, int P, int Q, int dtype, pcgan_stream_t s);
int pcgan_maxpool_bwd(const void* dy, const int32_t* argmax, void* dx, int NC, int H, int W, int k, int stride,
                      int pad, int P, int Q, int dtype, pcgan_stream_t s);
/* AvgPool2d(3, stride=2, padding=[1, 1], count_include_pad=False)  models/networks.py:1897, 1948 (D_NLayersMulti's down-sampler).
 * count_include_pad=False only: the divisor is the number of taps inside the plane.  fwd: fp32 sum of the in-bounds taps in scan order,
 * one IEEE division, one rounding.  bwd: a gather, dx = [base +] sum over (p, q) ascending of fp32(dy[p][q] / count(p, q)); base may be
 * NULL, dx may be base.  P, Q: floor-mode output sizes; pad > k / 2 and non-positive sizes are refused; NC is not limited to 65535. */
int pcgan_avgpool_fwd(const void* x, void* y, int NC, int H, int W, int k, int stride, int pad, int P, int Q, int dtype,
                      pcgan_stream_t s);
int pcgan_avgpool_bwd(const void* dy, const void* base, void* dx, int NC, int H, int W, int k, int stride, int pad, int P, int Q,
                      int dtype, pcgan_stream_t s);
int pcgan_global_pool_fwd(const void* x, void* y, int32_t* argmax, int NC, int HW, int is_max, int dtype,
                          pcgan_stream_t s);
int pcgan_global_pool_bwd(const void* dy, const int32_t* argmax, void* dx, int NC, int HW, int is_max, int dtype,
                          pcgan_stream_t s);
int pcgan_bilinear_fwd(const void* x, void* y, int NC, int H, int W, int P, int Q, int dtype, pcgan_stream_t s);
int pcgan_bilinear_bwd(const void* dy, void* dx, int NC, int H, int W, int P, int Q, int dtype, pcgan_stream_t s);

/* ---- losses ----------------------------------------------------------------------
 * nn.BCELoss(mean) against a per-sample target broadcast over the patch map
 * (GANLoss, models/networks.py:386-420; log clamped at -100 like torch);
 * nn.L1Loss / nn.MSELoss (models/wsgan_emb_model.py:141-149).
 * Each writes the scalar loss to loss[0] and, when grad != NULL, dloss/dpred * gscale. */
int pcgan_bce_loss(const void* pred, const float* target_n, float* loss, void* grad, int N, int per_n,
                   float gscale, void* ws, size_t ws_bytes, int dtype, pcgan_stream_t s);
int pcgan_l1_loss(const void* a, const void* b, float* loss, void* grad_a, size_t n, float gscale,
                  void* ws, size_t ws_bytes, int dtype, pcgan_stream_t s);
int pcgan_mse_loss(const void* a, const void* b, float* loss, void* grad_a, size_t n, float gscale,
                   void* ws, size_t ws_bytes, int dtype, pcgan_stream_t s);
size_t pcgan_loss_workspace_bytes(size_t n);

/* ---- optimizer -------------------------------------------------------------------
 * torch.optim.Adam(lr, betas=(beta1, 0.999), eps=1e-8) on a flat fp32 parameter
 * buffer (models/wsgan_emb_model.py:153-156).  step is the 1-based step count. */
int pcgan_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float lr,
                    float beta1, float beta2, float eps, int step, pcgan_stream_t s);
/* hipGraph-capturable variant: lr_dev[0] (float) and step_dev[0] (int) live in device
 * memory; the step counter is incremented on the stream before the update reads it. */
int pcgan_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n,
                        const float* lr_dev, int* step_dev, float beta1, float beta2, float eps,
                        pcgan_stream_t s);

/* ---- loader image pipeline ----------------------------------
 * transforms.Resize([loadSize, loadSize], Image.BICUBIC) -> RandomCrop(fineSize) ->
 * RandomHorizontalFlip -> ToTensor -> Normalize(.5, .5) of get_transform
 * (data/base_dataset.py:24-64) and the RGB -> gray mix of the pair dataset
 * (data/wsgan_emb_dataset.py:46-49), for n equally sized uint8 RGB images
 * src[n][H][W][3] -> out[dst][out_channels][FH][FW] fp32.  Pillow's two-pass 22-bit
 * fixed-point resampling (horizontal first, uint8 intermediate): the caller builds the
 * coefficient tables kh[RW][ksize_h] / kv[RH][ksize_v] and bounds bh[RW][2] / bv[RH][2]
 * (first source index, tap count) the way Pillow's precompute_coeffs /
 * normalize_coeffs_8bpc do; a dimension that keeps its size gets the identity table
 * (ksize 1, coefficient 1 << 22).  aug[n][4] (device) = crop x0, crop y0, flip, dst index;
 * the caller guarantees 0 <= x0 <= RW - FW, 0 <= y0 <= RH - FH.  Integer arithmetic up to
 * the last three correctly rounded fp32 operations: bit-exact with the PIL path.
 * pcgan_image_transform_band (host only, bv_host in host memory) picks the band of output
 * rows one workgroup takes and the LDS rows it needs. */
typedef struct {
    int H, W;     /* source image                     */
    int RH, RW;   /* after the resize (loadSize)      */
    int FH, FW;   /* after the crop (fineSize)        */
    int ksize_h, ksize_v;
    int out_channels; /* 3, or 1 = gray mix           */
} pcgan_image_desc;
int pcgan_image_transform_band(const pcgan_image_desc* d, const int32_t* bv_host, int* band, int* max_rows);
int pcgan_image_transform(const pcgan_image_desc* d, const uint8_t* src, const int32_t* kh, const int32_t* bh,
                          const int32_t* kv, const int32_t* bv, const int32_t* aug, float* out, int n, int band,
                          int max_rows, pcgan_stream_t s);
/* The affine modes (get_transform 'resize_affine_crop' / 'resize_affine_center', data/base_dataset.py:41-52:
 * Resize([loadSize, loadSize], BICUBIC) -> RandomAffine(degrees, scale, BICUBIC, fillcolor=127) ->
 * RandomCrop / CenterCrop(fineSize) -> RandomHorizontalFlip -> ToTensor -> Normalize) in two launches:
 * pcgan_image_resize_u8: the resize alone, src[n][H][W][3] -> out[n][RH][RW][3] uint8, same tables and
 * band as pcgan_image_transform with the window the whole image (FH = RH, FW = RW; the bytes the PIL
 * path's Image.resize returns).
 * pcgan_image_affine: Pillow's Image.transform(AFFINE, BICUBIC, fillcolor=127) of the resized images
 * (d->RH x d->RW, mat[n][6] doubles: the inverse matrix, output pixel centre -> input position) read at
 * the crop window (aug[n][4] = crop x0, crop y0, flip, dst index; 0 <= x0 <= RW - FW, 0 <= y0 <= RH - FH
 * checked by the caller), flipped, normalised into out[dst][out_channels][FH][FW] fp32 (1 channel: the
 * gray mix).  Double arithmetic in Pillow's order, bit-exact with the PIL path; the fill is (127, 0, 0),
 * the reference's integer fill colour on an RGB image.  d->H, W, ksize_* are not read. */
int pcgan_image_resize_u8(const pcgan_image_desc* d, const uint8_t* src, const int32_t* kh, const int32_t* bh,
                          const int32_t* kv, const int32_t* bv, uint8_t* out, int n, int band, int max_rows,
                          pcgan_stream_t s);
int pcgan_image_affine(const pcgan_image_desc* d, const uint8_t* resized, const double* mat, const int32_t* aug,
                       float* out, int n, pcgan_stream_t s);

/* ---- convolution on the bf16 matrix pipe (v_mfma_f32_32x32x16_bf16, fp32 accumulators) -----------
 * Same call sites as pcgan_conv2d_fwd_packed for stride-1 convolutions with C % 16 == 0, K >= 32, at most 25 taps
 * (the ResnetBlock convolutions, models/networks.py:621-648).
 *   desc.dtype = PCGAN_F32:  every fp32 operand is split exactly into three bf16 pieces and the six piece products that
 *                            matter are accumulated in fp32: error as the fp32 MFMA path (scripts/micro/bf16_split.hip).
 *                            The host routes the residual-block convolutions here by default (PCGAN_BF16X6=0: fp32 MFMA).
 *   desc.dtype = PCGAN_BF16: the bf16 path: bf16 activations as stored, weights rounded to bf16 by the pack call, one product.
 * Pack once per weight version. */
int pcgan_conv2d_bsplit_supported(const pcgan_conv_desc* d);
size_t pcgan_conv2d_bsplit_packed_bytes(const pcgan_conv_desc* d);
int pcgan_conv2d_bsplit_pack(const pcgan_conv_desc* d, const float* w, void* packed, pcgan_stream_t s);
int pcgan_conv2d_fwd_bsplit(const pcgan_conv_desc* d, const void* x, const void* packed, const float* bias, void* y,
                            int act, float slope, pcgan_stream_t s);
/* the same for the data gradient of nn.ReflectionPad2d(1) + nn.Conv2d(k=3, stride 1) (the ResnetBlock convolutions): row
 * mirrors folded into three per-row-class weight sets by the pack call, column mirrors gathered as a second source. */
int pcgan_conv2d_bsplit_dgrad_supported(const pcgan_conv_desc* d);
size_t pcgan_conv2d_bsplit_dgrad_packed_bytes(const pcgan_conv_desc* d);
int pcgan_conv2d_bsplit_dgrad_pack(const pcgan_conv_desc* d, const float* w, void* packed, pcgan_stream_t s);
int pcgan_conv2d_bwd_data_bsplit(const pcgan_conv_desc* d, const void* dy, const void* packed, void* dx, pcgan_stream_t s);
/* ... and for its weight gradient: the same GEMM with the roles turned (rows = output channels, operand A = dy re-split per
 * call, columns = (c, r, s), reduction over pixels in splits + a fixed-order reduce); ws holds the reflection-padded copy of x,
 * the pieces of dy and the partial sums.  accumulate != 0 adds into dw like pcgan_conv2d_bwd_weight. */
int pcgan_conv2d_bsplit_wgrad_supported(const pcgan_conv_desc* d);
size_t pcgan_conv2d_bsplit_wgrad_workspace_bytes(const pcgan_conv_desc* d);
int pcgan_conv2d_bwd_weight_bsplit(const pcgan_conv_desc* d, const void* x, const void* dy, float* dw, int accumulate, void* ws,
                                   size_t ws_bytes, pcgan_stream_t s);

/* ---- the same residual-block convolutions (nn.ReflectionPad2d(1) + nn.Conv2d(dim, dim, 3), models/networks.py:621-648; fp32
 * tensors) with TWO fp16 pieces per operand and three products -- half the matrix instructions of the three-piece bf16 split at the
 * same measured error (scripts/micro/bf16_split: 5.3e-7 relative L2 at K = 2304, fp32 MFMA 6.1e-7).  fp16 has five exponent
 * bits: every operand tensor is scaled by the power of two that puts its largest magnitude into (2^13, 2^14], and the result is
 * scaled back exactly.  The largest magnitude is a DEVICE value (no host synchronisation): x_amax[0 .. n_amax) holds partial
 * maxima, the kernel takes the largest -- one float written by pcgan_absmax, or the per-plane maxima the producing kernel
 * hands over (pcgan_instnorm_* pmax outputs).  It must be a true bound: a larger element would overflow.
 * pass = PCGAN_PASS_FWD | PCGAN_PASS_BWD_DATA; image width 32 or 64, 128 / width rows dividing the height, gathered channels a
 * multiple of 32, produced channels a multiple of 256.  packed: pcgan_conv2d_hsplit_packed_bytes(d, pass) bytes, valid for any
 * batch size; the pack call also stores the largest magnitude of every weight row in it (one power-of-two scale per row). */
/* out[0 .. slots) = partial maxima of |x| (one per workgroup, 1 <= slots <= 1024; no atomics, nothing to clear beforehand);
 * pcgan_absmax_slots(n) = the count that keeps the pass bandwidth-bound.  Weight tensors use exactly 64 slots. */
int pcgan_absmax_slots(size_t n);
int pcgan_absmax(const void* x, size_t n, int dtype, float* out, int slots, pcgan_stream_t s);
/* Audit of the maxima a tensor carries (the fp16 route trusts them: a claim that is too SMALL overflows an fp16 piece -- the
 * non-finite sentinel below reports that; a claim that is too LARGE, e.g. after the tensor was rewritten with smaller values through
 * `.data` / a raw pointer, pushes the low pieces into subnormals and loses bits silently).  claimed[0 .. n_claimed) = the attached
 * partial maxima, fresh[0 .. n_fresh) = the partials of a pcgan_absmax pass over the tensor as it is now; both are maxima of the same
 * stored values, so they must agree exactly.  counts (three device words owned by the caller): [0] += 1 if the tensor holds more than
 * claimed, [1] += 1 if its largest value is below 2^-8 of the claim, [2] += 1 for any other mismatch.  One tiny launch; the host
 * (hip/ops.py: amax_of) audits every n-th consumption of attached maxima (every one in the test suite). */
int pcgan_amax_audit(const float* claimed, int n_claimed, const float* fresh, int n_fresh, unsigned int* counts, pcgan_stream_t s);
int pcgan_conv2d_hsplit_supported(const pcgan_conv_desc* d, int pass);
size_t pcgan_conv2d_hsplit_packed_bytes(const pcgan_conv_desc* d, int pass);
int pcgan_conv2d_hsplit_pack(const pcgan_conv_desc* d, int pass, const float* w, void* packed, pcgan_stream_t s);
int pcgan_conv2d_fwd_hsplit(const pcgan_conv_desc* d, const void* x, const float* x_amax, int n_amax, const void* packed,
                            const float* bias, void* y, int act, float slope, pcgan_stream_t s);
int pcgan_conv2d_bwd_data_hsplit(const pcgan_conv_desc* d, const void* dy, const float* dy_amax, int n_amax, const void* packed,
                                 void* dx, pcgan_stream_t s);
/* ... the same with dx = conv^T(dy, w) + add: the gradient that reaches a ResnetBlock's input through the skip connection
 * (`x + conv_block(x)`, models/networks.py:650-652) summed in the epilogue instead of by a separate `grad +=` pass.  add may be NULL. */
int pcgan_conv2d_bwd_data_hsplit_add(const pcgan_conv_desc* d, const void* dy, const float* dy_amax, int n_amax, const void* packed,
                                     const void* add, void* dx, pcgan_stream_t s);
/* Every other convolution whose gathered channel count is a multiple of 16 (<= 25 taps, more than 32 produced channels; any
 * stride; forward with zero / reflection padding, data gradient with zero padding -- incl. nn.ConvTranspose2d forward,
 * models/networks.py:584-602, 734-763; models/resnet.py): the fp16 two-piece form of pcgan_conv2d_fwd_packed /
 * pcgan_conv2d_bwd_data_packed.  Same workspace and semantics; packed weights from pcgan_conv2d_hgemm_pack (desc.dtype = PCGAN_BF16:
 * from pcgan_conv2d_pack_weights, w_amax unused); w_amax = the row maxima pcgan_conv2d_hgemm_pack wrote. */
int pcgan_conv2d_hgemm_supported(const pcgan_conv_desc* d, int pass);
/* packed weights of the two calls below: pcgan_conv2d_pack_weights' image with every group of 4 consecutive k of a row PRE-SPLIT into
 * [4 fp16 high pieces | 4 fp16 low pieces] of the weights scaled by ONE POWER OF TWO PER ROW of the pass's weight matrix (forward: per
 * output channel; data gradient: per input channel) -- the weights change once per optimizer step while each net runs 2-4 times in
 * between, so the kernel's weight path is a plain copy, and a filter row far below the tensor's largest weight keeps its 22 bits.
 * w_rowmax (K floats for PCGAN_PASS_FWD, C for PCGAN_PASS_BWD_DATA) is WRITTEN by the pack call -- the largest magnitude of every row --
 * and must be handed to the convolution calls as `w_amax` (their epilogue divides row m by pow2(w_rowmax[m])).
 * Size of packed: pcgan_conv2d_packed_bytes. */
int pcgan_conv2d_hgemm_pack(const pcgan_conv_desc* d, int pass, const float* w, float* w_rowmax, float* packed, pcgan_stream_t s);
int pcgan_conv2d_fwd_packed_hsplit(const pcgan_conv_desc* d, const void* x, const float* x_amax, int n_amax, const float* packed,
                                   const float* w_amax, const float* bias, void* y, int act, float slope, void* ws, size_t ws_bytes,
                                   pcgan_stream_t s);
int pcgan_conv2d_bwd_data_packed_hsplit(const pcgan_conv_desc* d, const void* dy, const float* dy_amax, int n_amax,
                                        const float* packed, const float* w_amax, const float* bias, void* dx, void* ws,
                                        size_t ws_bytes, pcgan_stream_t s);
/* weight gradient on the same route: stride 1 or 2, reflection (stride 1) or zero padding, <= 49 taps, >= 32 output channels -- the
 * residual blocks, the generator's down / up-sampling layers, the PatchGAN's layers (models/networks.py:584-648, 753-775).  Both
 * operands are split on their way to LDS, so there is no packed copy of dy; ws (pcgan_conv2d_hsplit_wgrad_workspace_bytes) holds the
 * padded copy of x (when one is made) and the partial sums of the splits of the pixel reduction, which are combined in a fixed order.
 * Zero padding <= 1: the padding is applied inside the gather (no padded copy); with fp32 tensors the output width may also be ragged
 * (at least 3/4 of its multiple of 16: the PatchGAN's 15 x 15 layer) and K may exceed 256 (row tiles); otherwise (bf16 tensors, other
 * paddings) the output width is a multiple of 16 and K <= 256.  pcgan_conv2d_hsplit_wgrad_inline: 1 when the call makes no padded copy of x (routing: the
 * copy of a 134 MB input costs more than the matrix pipe saves).  accumulate != 0 adds into dw like pcgan_conv2d_bwd_weight.
 * desc.dtype = PCGAN_BF16: the one-product bf16 form (the maxima pointers may be NULL). */
int pcgan_conv2d_hsplit_wgrad_supported(const pcgan_conv_desc* d);
int pcgan_conv2d_hsplit_wgrad_inline(const pcgan_conv_desc* d);
size_t pcgan_conv2d_hsplit_wgrad_workspace_bytes(const pcgan_conv_desc* d);
int pcgan_conv2d_bwd_weight_hsplit(const pcgan_conv_desc* d, const void* x, const float* x_amax, int n_xamax, const void* dy,
                                   const float* dy_amax, int n_dyamax, float* dw, int accumulate, void* ws, size_t ws_bytes,
                                   pcgan_stream_t s);


/* ---- composite: one ResnetBlock per call -----------------------------------------------------------------------------------------
 * `x + conv_block(x)` with conv_block = ReflectionPad2d(1), Conv2d(dim, dim, 3, bias), InstanceNorm2d, ReLU, ReflectionPad2d(1),
 * Conv2d(dim, dim, 3, bias), InstanceNorm2d (models/networks.py:616-652; 9 blocks x 2 generator passes per step).  The per-op entry
 * points above cost the host one call per launch (6 forward, 10 backward per block: ~12 ms of a 32 ms step); these two launch exactly
 * the same kernels with the same arguments in the same order -- results are bit-identical to the per-op sequence -- from ONE call.
 * fp32 tensors on the fp16 two-piece route, or (round 4) bf16 tensors on the one-product forms (pcgan_resblock_supported: the shapes
 * the residual-convolution kernels and pcgan_instnorm_fused take); other shapes use the per-op calls.
 *
 * forward   y1 = conv1(x) ; h = relu(IN(y1)) ; y2 = conv2(h) ; out = IN(y2) + x.  pk1 / pk2: pcgan_conv2d_hsplit_pack(PASS_FWD).
 *           stats[4][N*C] receives mean1, M2_1, mean2, M2_2 (kept for the backward pass); amax[2][N*C] the plane maxima of h and
 *           out (operand maxima of the next convolution); running statistics are updated in place.
 * backward  given dout: dy2 = IN2'(dout) ; dw2 += wgrad(h, dy2), db2 += sum dy2 ; dh = dgrad2(dy2) ; dy1 = (IN1 o relu)'(dh) ;
 *           dw1 += wgrad(x, dy1), db1 += sum dy1 ; dx = dgrad1(dy1) + dout (skip connection).  pk1b / pk2b:
 *           pcgan_conv2d_hsplit_pack(PASS_BWD_DATA).  The weight / bias gradients are launched on `side` (ordered behind the producer of
 *           their operands through `fork_event`, an event the caller owns: pcgan_event_create); the caller joins `side` before it reads
 *           dw / db.  scratch: 5*N*C floats (plane sums and maxima of dy2 / dy1); wgrad_ws: pcgan_resblock_wgrad_workspace_bytes(d),
 *           used on `side` only.  dy2, dh, dy1 are caller-allocated temporaries the size of x. */
typedef struct {
    int N, C, H, W;
    float eps, momentum;
    int dtype; /* PCGAN_F32: the fp16 two-piece route (x_amax / amax used); PCGAN_BF16 (round 4): bf16 tensors on the one-product forms --
                  pk*: pcgan_conv2d_bsplit_pack / pcgan_conv2d_bsplit_dgrad_pack, x_amax / h_amax / amax unused (may be NULL) */
} pcgan_resblock_desc;
typedef void* pcgan_event_t; /* hipEvent_t */
int pcgan_event_create(pcgan_event_t* ev);
int pcgan_event_destroy(pcgan_event_t ev);
int pcgan_resblock_supported(const pcgan_resblock_desc* d);
size_t pcgan_resblock_wgrad_workspace_bytes(const pcgan_resblock_desc* d);
int pcgan_resblock_fwd(const pcgan_resblock_desc* d, const void* x, const float* x_amax, int n_xamax, const void* pk1, const float* b1,
                       const void* pk2, const float* b2, float* rm1, float* rv1, float* rm2, float* rv2, void* y1, void* h, void* y2,
                       void* out, float* stats, float* amax, pcgan_stream_t s);
int pcgan_resblock_bwd(const pcgan_resblock_desc* d, const void* dout, const void* x, const float* x_amax, int n_xamax, const void* y1,
                       const void* h, const float* h_amax, const void* y2, const float* stats, const void* pk1b, const void* pk2b,
                       float* dw1, float* db1, float* dw2, float* db2, void* dy2, void* dh, void* dy1, void* dx, float* scratch,
                       void* wgrad_ws, size_t wgrad_ws_bytes, pcgan_stream_t s, pcgan_stream_t side, pcgan_event_t fork_event);

/* ---- convolutions that gather <= 4 channels, on the same fp16 two-piece route (csrc/thin_conv.hip) --------------------------------------
 * pass = PCGAN_PASS_FWD: C <= 4 input channels, K a multiple of 64 (<= 256), 7x7 stride 1 / 2 or 4x4 stride 2, zero padding or (stride 1)
 * reflection padding -- ReflectionPad2d(3) + Conv2d(input_nc + nz, ngf, 7) of the generator (models/networks.py:578-581), conv1 of the Elo
 * encoder's ResNet-18 (models/resnet.py:108-111), the first PatchGAN layer (models/networks.py:753-755).
 * pass = PCGAN_PASS_BWD_DATA: K <= 4 output channels of the convolution, C a multiple of 64, 7x7 stride 1 -- autograd's data gradient of
 * the generator's head ReflectionPad2d(3) + Conv2d(ngf, output_nc, 7) (models/networks.py:603-605), computed as a forward-form
 * convolution of dy with flipped weights; with reflection padding on the padded grid (ws: pcgan_conv2d_thin_workspace_bytes) and folded.
 * One workgroup = 8 x 32 output pixels x 64 channels; its input window is loaded, scaled and split ONCE into LDS as [position][4 channels],
 * and with k = 4 tap + channel an MFMA lane's 8 consecutive k are two adjacent taps = two 8-byte LDS reads.  packed
 * (pcgan_conv2d_thin_packed_bytes): the weights pre-scaled per output row, pre-split, in MFMA fragment order + the row maxima; x_amax /
 * n_amax as for the other fp16-route calls (partial maxima of |x| on the device).  fp32 tensors only. */
int pcgan_conv2d_thin_supported(const pcgan_conv_desc* d, int pass);
size_t pcgan_conv2d_thin_packed_bytes(const pcgan_conv_desc* d, int pass);
size_t pcgan_conv2d_thin_workspace_bytes(const pcgan_conv_desc* d, int pass);
int pcgan_conv2d_thin_pack(const pcgan_conv_desc* d, int pass, const float* w, void* packed, pcgan_stream_t s);
int pcgan_conv2d_fwd_thin(const pcgan_conv_desc* d, const void* x, const float* x_amax, int n_amax, const void* packed, const float* bias,
                          void* y, int act, float slope, pcgan_stream_t s);
int pcgan_conv2d_bwd_data_thin(const pcgan_conv_desc* d, const void* dy, const float* dy_amax, int n_amax, const void* packed, void* dx,
                               void* ws, size_t ws_bytes, pcgan_stream_t s);

/* A RUN of `nblocks` consecutive ResnetBlocks per call (round 4: the generator's nine blocks, models/networks.py:589-592): the
 * launches of nblocks pcgan_resblock_fwd / _bwd calls, block i reading block i - 1's output and plane maxima, from one host call.
 * Per-block tensors are slices of stacked buffers: y1, h, y2, out [nblocks][N*C*H*W]; stats [nblocks][4*N*C]; amax [nblocks][2*N*C];
 * backward: dy2, dy1 [nblocks][N*C*H*W] (read by `side` after the call), dh [N*C*H*W], dxs [2][N*C*H*W] (gradient handed from block
 * to block), scratch [nblocks][5*N*C]; dx = gradient of the chain's input.  Per-block parameter pointers (packed weights, biases,
 * running statistics, gradient slots; a bias / running-statistics entry may be NULL) come as HOST arrays of nblocks pointers. */
int pcgan_restrunk_fwd(const pcgan_resblock_desc* d, int nblocks, const void* x, const float* x_amax, int n_xamax, const void* const* pk1,
                       const float* const* b1, const void* const* pk2, const float* const* b2, float* const* rm1, float* const* rv1,
                       float* const* rm2, float* const* rv2, void* y1, void* h, void* y2, void* out, float* stats, float* amax,
                       pcgan_stream_t s);
int pcgan_restrunk_bwd(const pcgan_resblock_desc* d, int nblocks, const void* dout, const void* x, const float* x_amax, int n_xamax,
                       const void* y1, const void* h, const void* y2, const void* out, const float* stats, const float* amax,
                       const void* const* pk1b, const void* const* pk2b, float* const* dw1, float* const* db1, float* const* dw2,
                       float* const* db2, void* dy2, void* dh, void* dy1, void* dxs, void* dx, float* scratch, void* wgrad_ws,
                       size_t wgrad_ws_bytes, pcgan_stream_t s, pcgan_stream_t side, pcgan_event_t fork_event);

/* ---- weight gradient of the residual-block convolution, "image-innermost" form (round 4; csrc/wgrad_direct.hip) -------------------------
 * nn.Conv2d(dim, dim, 3) behind nn.ReflectionPad2d(1) in ResnetBlock (models/networks.py:621-648), autograd's weight gradient; fp32 tensors,
 * fp16 two-piece arithmetic as pcgan_conv2d_bwd_weight_hsplit (same operand maxima, same error level).  A transposing pre-pass scales and
 * splits x and dy ONCE into 16-byte records of 8 images per (pixel, channel) -- a filter tap then shifts the pixel, not the position
 * inside a record -- and the main kernel loads every MFMA operand fragment straight from memory: no LDS, no barrier, no split arithmetic
 * in the loop (the per-tap form re-gathers and re-splits x nine times and is LDS-bound).  3x3, stride 1, reflection padding 1,
 * N % 16 == 0, K % 128 == 0, C % 32 == 0.  ws: pcgan_conv2d_wgrad_direct_workspace_bytes(d) bytes (the four piece arrays, the split
 * partials, two scale words).  dw[K][C][3][3], accumulate != 0: dw += (the optimizer's gradient buffer). */
int pcgan_conv2d_wgrad_direct_supported(const pcgan_conv_desc* d);
/* ---- ... and in the "row ring" form (round 4; csrc/wgrad_rowring.hip): a workgroup's column tile is 32 input channels x all nine taps and it
 * walks down a 16-pixel-wide strip of one image, keeping the padded rows in a ring of four LDS slots -- every element of x is loaded and split
 * once per strip instead of once per tap.  Same arguments, workspace rule and results level as pcgan_conv2d_bwd_weight_hsplit, which hands the
 * shapes this form takes to it under option "wgrad_rowring": fp32 or bf16 tensors, 3x3, stride 1, reflection padding 1, W % 16 == 0, K % 128 == 0,
 * C % 32 == 0, H >= 3; bf16 tensors too (one bf16 product per tap, x_amax / dy_amax unused and may be NULL).  Replaces autograd's weight
 * gradient of nn.Conv2d in ResnetBlock (models/networks.py:616-652). */
int pcgan_conv2d_wgrad_rowring_supported(const pcgan_conv_desc* d);
size_t pcgan_conv2d_wgrad_rowring_workspace_bytes(const pcgan_conv_desc* d);
int pcgan_conv2d_bwd_weight_rowring(const pcgan_conv_desc* d, const void* x, const float* x_amax, int n_xamax, const void* dy, const float* dy_amax,
                                    int n_dyamax, float* dw, int accumulate, void* ws, size_t ws_bytes, pcgan_stream_t s);
size_t pcgan_conv2d_wgrad_direct_workspace_bytes(const pcgan_conv_desc* d);
int pcgan_conv2d_bwd_weight_direct(const pcgan_conv_desc* d, const void* x, const float* x_amax, int n_xamax, const void* dy,
                                   const float* dy_amax, int n_dyamax, float* dw, int accumulate, void* ws, size_t ws_bytes, pcgan_stream_t s);

/* ---- Inception-v3 feature network (FID; forward only, fp32 tensors; csrc/inception.hip) ----------------------------------------------
 * Replaces torchvision's Inception3 blocks behind the reference's models/inception.py (InceptionV3, used by compute_fid_score.py:56-57,
 * 260-290): BasicConv2d = Conv2d(bias=False) + eval BatchNorm2d(eps=0.001) + ReLU, the InceptionA..E branch pools, and the input
 * F.upsample(bilinear) + normalize_input of its forward.
 *
 * pcgan_iconv_desc: a convolution with PER-AXIS zero padding (1x7, 7x1, 1x3, 3x1 kernels) whose output is channel slice
 * [k_off, k_off + K) of an NCHW tensor y[N][K_total][P][Q] (a Mixed block's branches write their slices of its output: no concatenation).
 * R, S <= 7, 0 <= pad_h < R, 0 <= pad_w < S, stride 1 or 2, dtype PCGAN_F32 only (bf16 is refused); pcgan_iconv_supported says whether a
 * geometry is taken (0: the reason is in pcgan_last_error()).
 *
 * pcgan_iconv_pack (once per weight load): w[K][C][R][S] fp32 and the eval BatchNorm's gamma, beta, running mean, running var (all four
 * given, or all NULL for a plain convolution) folded in fp32 -- w * gamma / sqrt(var + eps), beta - mean * gamma / sqrt(var + eps) -- into
 * `packed` (pcgan_iconv_packed_bytes(d) bytes, 16-byte aligned): the bias, then the kernel's transposed weight layout.  pool_expand != 0:
 * w is a 1x1 weight w[K][C][1][1] and d describes the 3x3 pad-1 stride-1 convolution it becomes, every tap w / 9 -- avg_pool2d(3, 1, 1,
 * count_include_pad=True) then the 1x1 conv, as one linear map (the pool branches of InceptionA / C / E need no pool pass).
 * pcgan_iconv_fwd: y[:, k_off:k_off+K] = act(conv(x, W') + b'), act = ReLU if relu != 0; channels outside the slice are not touched.
 * Implicit GEMM on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32), no operand scaling; blocked summation (16-term partial sums added
 * in reduction order).
 *
 * pcgan_maxpool_slice_fwd: max_pool2d(k, stride, no padding, floor mode) of x[N][C][H][W] into channels [k_off, k_off + C) of
 * y[N][K_total][P][Q] (the InceptionB / D pool branches; exact).  Unlike pcgan_maxpool_fwd it writes no argmax.
 * pcgan_inception_prep: x[N][3][H][W] -> y[N][3][OH][OW], F.interpolate(mode='bilinear', align_corners=False) with ATen's source index
 * (scale = H / OH in fp32, src = scale * (dst + 0.5) - 0.5 clamped at 0), then y[:, c] = y[:, c] * scale[c] + shift[c] when scale / shift
 * (host arrays of 3 floats, read at the call) are given.  OH == H, OW == W is the affine alone (the resize is then an exact copy). */
typedef struct {
    int N, C, H, W;       /* input  [N][C][H][W]                               */
    int K, R, S;          /* weight [K][C][R][S]                               */
    int stride, pad_h, pad_w;
    int P, Q;             /* output channels [k_off, k_off + K) of [N][K_total][P][Q] */
    int k_off, K_total;
    int dtype;            /* PCGAN_F32 only                                    */
} pcgan_iconv_desc;
int pcgan_iconv_supported(const pcgan_iconv_desc* d);
size_t pcgan_iconv_packed_bytes(const pcgan_iconv_desc* d);
int pcgan_iconv_pack(const pcgan_iconv_desc* d, int pool_expand, const float* w, const float* gamma, const float* beta, const float* mean,
                     const float* var, float eps, void* packed, pcgan_stream_t s);
int pcgan_iconv_fwd(const pcgan_iconv_desc* d, const void* x, const void* packed, void* y, int relu, pcgan_stream_t s);
int pcgan_maxpool_slice_fwd(const void* x, void* y, int N, int C, int H, int W, int k, int stride, int P, int Q, int k_off, int K_total,
                            int dtype, pcgan_stream_t s);
int pcgan_inception_prep(const void* x, void* y, int N, int C, int H, int W, int OH, int OW, const float* scale, const float* shift,
                         int dtype, pcgan_stream_t s);

/* ---- classifier head of the Inception Score (forward only, fp32 tensors; csrc/inception.hip) ------------------------------------------
 * logits[N][K] = x[N][C] W[K][C]^T + b[K] (nn.Linear's layout; b may be NULL) and probs[N][K] = softmax(logits, dim=1).  Replaces
 *   F.softmax(inception_model(x))   util/inception_score.py:38-41 (torchvision inception_v3's fc, then the softmax)
 *   nn.Linear                       models/resnet.py:194 (the fc of the networks.ResNet classifier, models/networks.py:1258-1285)
 * Any N, C, K >= 1.  fp32 accumulation in a fixed order (exact-fp32 MFMA chains over four interleaved quarters of C, the four partial
 * sums added in order, then the bias); softmax = expf(l - row max) / fixed-order row sum, full-precision expf: results are bit-identical
 * from run to run and beside other streams' work (no atomics).  Each workgroup reads its tile of W once per batch tile of 64 rows.
 * logits may be NULL (they are then staged in probs).  dtype PCGAN_F32 only. */
int pcgan_linear_softmax_fwd(const void* x, const float* w, const float* b, void* logits, void* probs, int N, int C, int K, int dtype,
                             pcgan_stream_t s);

/* ---- training pass of the attribute classifier's head (fp32 tensors; csrc/linear_head.hip) --------------------------------------------
 * nn.Linear(C -> K) + nn.CrossEntropyLoss(weight) of the classifier classification.py trains.  Replaces
 *   output = net.forward(img0); loss = criterion(output, label); get_prediction(output)     classification.py:330-332, 376-384
 *   the fc layer at the end of self.model(x)                                                  models/networks.py:1284-1285
 * Sizes: 1 <= N <= 512 rows, C a multiple of 4 in [4, 2048], 1 <= K <= 1024 classes; dtype PCGAN_F32 only (the head stays fp32 beside
 * bf16 activations, as losses and statistics do).  Every sum runs in a fixed order in float64 and is rounded to fp32 once: results are
 * bit-identical from run to run, no float atomics.  x / w / dx / dw that are 16-byte aligned are accessed 128 bits at a time.
 *
 * pcgan_linear_ce_fwd, ONE launch of N workgroups:
 *   logits[n][k]  = sum_c x[n][c] w[k][c] + b[k]                       (b may be NULL)
 *   loss          = sum_n wt[y_n] (-log_softmax(logits[n])[y_n]) / sum_n wt[y_n]     (row maximum subtracted; class_weight NULL = ones)
 *   dlogits[n][k] = wt[y_n] (softmax(logits[n])[k] - [k == y_n]) / sum_n wt[y_n]     (d loss / d logits)
 *   pred[n]       = index of the FIRST maximum of the fp32 logits[n] (numpy.argmax);  correct = #{n : pred[n] == y_n}
 * labels are int64 DEVICE memory, so they are not checked on the host: a label outside [0, K) never indexes anything on the device -- its
 * row is ignored (weight 0: no loss term, zero gradient, never counted correct), as ignore_index rows are in torch.  All rows ignored
 * gives 0 / 0 = NaN, as torch does.  logits, dlogits, loss, pred and correct may each be NULL (not wanted).
 * workspace: pcgan_linear_ce_workspace_bytes(N) bytes (0: N out of range), 8-byte aligned, caller-owned.  Its first word is the arrival
 * ticket of the last-arriver reduction of loss / correct: it must be ZERO before the first call and is left zero by every call, so calls
 * in stream order may share it whatever their N; calls on different streams need one each.
 *
 * pcgan_linear_bwd, ONE launch of N + K workgroups:
 *   dx[n][c] = sum_k dlogits[n][k] w[k][c];   dw[k][c] (+)= sum_n dlogits[n][k] x[n][c];   db[k] (+)= sum_n dlogits[n][k]
 * accumulate != 0 adds dw / db to what the buffers hold (a FusedAdam gradient buffer), else overwrites; dx is always overwritten.  Any of
 * dx, dw, db may be NULL, not all three. */
size_t pcgan_linear_ce_workspace_bytes(int N);
int pcgan_linear_ce_fwd(const void* x, const float* w, const float* b, const int64_t* labels, const float* class_weight, void* logits,
                        void* dlogits, float* loss, int64_t* pred, int32_t* correct, void* workspace, size_t workspace_bytes, int N,
                        int C, int K, int dtype, pcgan_stream_t s);
int pcgan_linear_bwd(const void* dlogits, const void* x, const float* w, void* dx, float* dw, float* db, int N, int C, int K,
                     int accumulate, int dtype, pcgan_stream_t s);

/* ---- end of the attribute regressor: pooling + MSE + "within delta" accuracy + gradient (csrc/pool_mse_head.hip) ---------------------
 * What regression.py's training iteration does after the conv head of networks.RegressionNetwork.  Replaces
 *   output = net.forward(img0); loss = criterion(output, label); get_accuracy(output, label, opt.delta)     regression.py:359-363
 *   nn.AvgPool2d(output.size(2))(output) / nn.MaxPool2d(output.size(2))(output)                             models/networks.py:1115-1118
 * and the backward pass of both.  x is [N][F][HW] in fp32 or bf16 storage (dtype), target [N F] fp32.  pcgan_pool_mse_fwd, ONE launch:
 *   pred[n][f]  = mean (is_max == 0: float64 sum in index order, divided, rounded to fp32 once) or maximum (exact) of the plane;
 *   argmax[n][f] = index of the FIRST maximum (is_max != 0 only; the convention of pcgan_global_pool_fwd)
 *   loss        = sum (pred - target)^2 / (N F)           differences in float64 from the fp32 pred, fixed order, rounded once
 *   hits        = #{ |pred - target| < delta }            in fp32, as torch.abs(pred - target) < delta on the returned pred; strict
 *   dx[n][f][i] = gscale 2 (pred - target) / (N F) (1 / HW for the mean | [i == argmax] for the maximum)
 *                 float64, rounded to fp32 once, then to bf16 (nearest even) in bf16 storage; x's storage type, always all of it written
 * pred, argmax, dx, loss and hits may each be NULL (not wanted); argmax must be given when is_max and dx both are.  Sizes: N, F >= 1,
 * N F <= 2^22, 1 <= HW <= 2^20.  Planes of up to 64 elements (3x3 .. 8x8 maps, the regressor's) are handled 128 per workgroup with one
 * lane per plane; longer ones by a workgroup each.  x / dx aligned to four elements are accessed four elements at a time, otherwise
 * element by element -- the same values either way.  No float atomics: results are bit-identical from run to run.
 * workspace: pcgan_pool_mse_workspace_bytes(N F) bytes (0: N F out of range), 8-byte aligned, caller-owned.  Its first word is the
 * arrival ticket of the last-arriver reduction of loss / hits: it must be ZERO before the first call and is left zero by every call, so
 * calls in stream order may share it whatever their sizes; calls on different streams need one each. */
size_t pcgan_pool_mse_workspace_bytes(int NF);
int pcgan_pool_mse_fwd(const void* x, const float* target, float* pred, int32_t* argmax, void* dx, float* loss, int32_t* hits, void* ws,
                       size_t ws_bytes, int N, int F, int HW, int is_max, float delta, float gscale, int dtype, pcgan_stream_t s);

/* ---- head of the projection discriminator (csrc/proj_head.hip) -------------------------------------------------------------------------
 * NLayerProjectionDiscriminator.forward with proj=True ("cGANs with Projection Discriminator").  Replaces
 *   h = torch.sum(self.phi(input), dim=(2, 3), keepdim=True)                 models/networks.py:830
 *   w_y = self.l_y(y)                                                        models/networks.py:831   (l_y = Conv2d(nz, C, 1))
 *   output = torch.sum(h * w_y, dim=1, keepdim=True) + self.psi(h)           models/networks.py:832   (psi = Conv2d(C, 1, 1, padding=1))
 *   torch.sigmoid(output) if self._sigm                                      models/networks.py:838
 * and autograd's backward through them.  p[B][C][HW] is the trunk's output (dtype: PCGAN_F32 or PCGAN_BF16, NCHW contiguous, any
 * element-aligned address), y[By][nz] fp32 with By = 1 (broadcast over the batch) or B, psi_w[C], psi_b[1], ly_w[C][nz], ly_b[C] fp32.
 *   h[b][c]      = sum of the plane p[b][c]                                   (fp32, kept for the backward pass)
 *   wy[b][c]     = sum_j ly_w[c][j] y[b][j] + ly_b[c]
 *   out[b][0][i][j] = sum_c h[b][c] wy[b][c] + psi_b + [i == j == 1] sum_c psi_w[c] h[b][c]       [B][1][3][3], in p's dtype
 * sigmoid != 0 applies 1 / (1 + exp(-x)) to out.  Sizes: B, C, HW >= 1 (HW <= 2^27, B * C < 2^31), 1 <= nz <= 16.
 *
 * pcgan_proj_head_bwd: g[B][1][3][3] (p's dtype) is d loss / d out; with sigmoid != 0 it is first multiplied by o (1 - o) of the output
 * recomputed in float64 from h.  With G[b] = sum_ij g[b][i][j] and gc[b] = g[b][1][1]:
 *   dp[b][c][:]  = G[b] wy[b][c] + gc[b] psi_w[c]            (p's dtype, always overwritten)
 *   dpsi_w[c]   (+)= sum_b gc[b] h[b][c]         dpsi_b (+)= sum_b G[b]
 *   dly_w[c][j] (+)= sum_b G[b] h[b][c] y[b][j]   dly_b[c] (+)= sum_b G[b] h[b][c]
 *   dy[b][j]     = sum_c G[b] h[b][c] ly_w[c][j]             (summed over b as well when By = 1; always overwritten)
 * Every output may be NULL (not wanted), not all of them.  accumulate != 0 adds the four parameter gradients to what their buffers hold
 * (a FusedAdam gradient buffer: D runs several times per step), else overwrites them.
 * workspace: pcgan_proj_head_bwd_workspace_bytes(B, nz) bytes (0: sizes out of range), 8-byte aligned, caller-owned, no state kept in
 * it between calls.
 *
 * Every sum runs in a fixed order in float64 and is rounded once; no float atomics: results are bit-identical from run to run and beside
 * other streams' work.  Two launches per direction.  p / dp that are 16-byte aligned are accessed 128 bits at a time, otherwise element
 * by element -- the same values either way (planes start element-aligned only when HW is no multiple of 4: 7x7, 15x15, 31x31 maps). */
int pcgan_proj_head_fwd(const void* p, const float* y, const float* psi_w, const float* psi_b, const float* ly_w, const float* ly_b,
                        void* out, float* h, int B, int C, int HW, int nz, int By, int sigmoid, int dtype, pcgan_stream_t s);
size_t pcgan_proj_head_bwd_workspace_bytes(int B, int nz);
int pcgan_proj_head_bwd(const void* g, const float* h, const float* y, const float* psi_w, const float* psi_b, const float* ly_w,
                        const float* ly_b, void* dp, float* dpsi_w, float* dpsi_b, float* dly_w, float* dly_b, float* dy, void* workspace,
                        size_t workspace_bytes, int B, int C, int HW, int nz, int By, int sigmoid, int accumulate, int dtype,
                        pcgan_stream_t s);

/* ---- U-Net skip join (csrc/unet_join.hip) -----------------------------------------------------------------------------------------------
 * UnetSkipConnectionBlock.forward, models/networks.py:729-733: `torch.cat([x, self.model(x)], 1)`, with the ReLU that the parent block
 * applies in place to the whole concatenation (uprelu, models/networks.py:698) optionally folded into either half, and autograd's
 * backward through both.  a[N][Ca][HW], b[N][Cb][HW], out[N][Ca + Cb][HW] and their gradients are activation tensors of `dtype`
 * (PCGAN_F32 or PCGAN_BF16), NCHW contiguous; act_a / act_b are PCGAN_ACT_NONE or PCGAN_ACT_RELU (anything else is refused).
 *   pcgan_skip_join_fwd   out[n][0..Ca) = act_a(a[n]),  out[n][Ca..Ca+Cb) = act_b(b[n])
 *   pcgan_skip_join_bwd   da[n] = dout[n][0..Ca)   where a[n] > 0 under PCGAN_ACT_RELU (+0 elsewhere), everywhere under PCGAN_ACT_NONE;
 *                         db[n] = dout[n][Ca..Ca+Cb) likewise with b.  da or db may be NULL (not wanted), not both; a (b) is read only
 *                         when da (db) is wanted through a ReLU and may be NULL otherwise.
 * out, da and db are fresh buffers of the caller: no output may alias an input.  Every output element is a copy of one input element or
 * zero, so results are bit-exact in both storage types.  One launch per call: a grid-stride loop over out / dout, 16-byte accesses when
 * Ca * HW and Cb * HW are multiples of 4 (fp32) or 8 (bf16) elements and every pointer is 16-byte aligned, element accesses otherwise;
 * no LDS, no atomics, no workspace.  N, Ca, Cb, HW >= 1. */
int pcgan_skip_join_fwd(const void* a, const void* b, void* out, int N, int Ca, int Cb, int HW, int act_a, int act_b, int dtype,
                        pcgan_stream_t s);
int pcgan_skip_join_bwd(const void* dout, const void* a, const void* b, void* da, void* db, int N, int Ca, int Cb, int HW, int act_a,
                        int act_b, int dtype, pcgan_stream_t s);

/* ---- gradient fan-in (csrc/grad_fanin.hip) -----------------------------------------------------------------------------------------------
 * y[i] = ((src[0][i] + src[1][i]) + src[2][i]) + ... : the sum autograd forms with n_src - 1 binary adds when one tensor feeds several
 * consumers, in ONE launch.  srcs is a HOST array of n_src device pointers (1 <= n_src <= PCGAN_ADD_N_MAX; n_src == 1 is a copy); they
 * reach the kernel inside its by-value argument, so there is no device-side pointer table and no upload.  All tensors hold n >= 1
 * elements of `dtype` (PCGAN_F32 or PCGAN_BF16).  The sum runs strictly left to right in fp32 and there is no multiply, so fp32 tensors
 * get the bits of the sequential fp32 sum; bf16 inputs are widened, summed in fp32 and rounded once (RNE) at the store.  y may not
 * overlap a source (refused).  16-byte accesses with an element tail when y and every source are 16-byte aligned, element accesses
 * otherwise; a grid-stride loop on a capped grid; no LDS, no atomics, no workspace.  Bytes moved: (n_src + 1) * n * sizeof(T).
 * Null pointers, n_src out of range, n == 0, an unknown dtype and an aliased y are reported before any launch. */
#define PCGAN_ADD_N_MAX 8
int pcgan_add_n(const void* const* srcs, int n_src, void* y, size_t n, int dtype, pcgan_stream_t s);

/* ---- backward pass of pcgan_concat_z (csrc/concat_bwd.hip) ---------------------------------------------------------------------------------
 * dy[N][C + nz][HW] is an activation tensor of `dtype` (PCGAN_F32 or PCGAN_BF16), contiguous.  In ONE launch:
 *     dimg[N][C][HW]    (dtype)  a bit-exact copy of dy[:, :C]
 *     dz[z_batch][nz]   (fp32)   dz[n][j] = the sum over the plane dy[n][C + j][:], accumulated in fp32 (ratings stay fp32, as in the
 *                                forward kernel); with z_batch == 1 (one rating for the batch) dz[0][j] = ((s_0 + s_1) + ...) + s_{N-1},
 *                                s_n the plane sums in ascending n.
 * dimg or dz may be NULL (not wanted), not both; a NULL output is not computed and its planes of dy are not read, so a dz-only call
 * touches N * nz planes.  The workgroups of the one grid are split between the two jobs; a plane is summed by one 256-lane workgroup
 * (per-lane fp32 partial sums in index order, a wave64 butterfly, the four wave results in wave order through LDS).  No atomics, no
 * workspace, no second launch: the order of the additions is fixed by the launch geometry, two calls give the same bits.  16-byte
 * accesses when HW * sizeof(T) and every pointer handed in are multiples of 16, element accesses otherwise.  dy null, both outputs
 * null, N, C, HW or nz <= 0, z_batch outside {1, N}, an unknown dtype and sizes whose products overflow int are reported before any
 * launch. */
int pcgan_concat_z_bwd(const void* dy, void* dimg, float* dz, int N, int C, int nz, int HW, int z_batch, int dtype, pcgan_stream_t s);

/* ---- Grad-CAM map and heat-map overlay of `siamese.py --mode attention` (csrc/gradcam.hip) ---------------------------------------------------
 * pcgan_gradcam_map replaces GradCAM2.generate of the reference (util/gradcam.py:214-252, called at siamese.py:958): act and grad are
 * [N][C][H][W] activation tensors of `dtype` (PCGAN_F32 or PCGAN_BF16, both the same), map is [N][1][H][W] fp32:
 *     PCGAN_GCAM_RAW      abs(sum_c A)                  grad may be NULL and is neither read nor required
 *     PCGAN_GCAM_PW       relu(sum_c g * A)
 *     PCGAN_GCAM_CW_POS   relu(sum_c w[n][c] * A)       w[n][c] = the mean over the plane of relu(g[n][c][:][:])
 *     PCGAN_GCAM_PW_CW    relu(sum_c (w[n][c] * g) * A)
 * (the reference's grouped conv3d with groups = N is this per-image channel sum; every type returns [N][1][H][W] here).  bf16 is widened
 * exactly, all arithmetic is fp32, one rounding per operation.  ONE launch, no workspace, no atomics, a summation order fixed by the
 * launch geometry: two calls give the same bits.  The weighted types recompute the plane means in every workgroup of an image (LDS holds
 * them: C <= 4096 there).  16-byte accesses when H * W * sizeof(T) and every pointer handed in are multiples of 16, element accesses
 * otherwise.  An unknown type or dtype, N, C, H or W <= 0, a null act or map, a null grad with a type other than raw, more than 4096
 * channels with a weighted type and sizes whose products overflow int are reported before any launch. */
#define PCGAN_GCAM_RAW 0
#define PCGAN_GCAM_PW 1
#define PCGAN_GCAM_CW_POS 2
#define PCGAN_GCAM_PW_CW 3
int pcgan_gradcam_map(const void* act, const void* grad, float* map, int N, int C, int H, int W, int type, int dtype, pcgan_stream_t s);

/* pcgan_heatmap_overlay replaces feature2image, tensor2image and the blend of attention_gradcam (siamese.py:401-410, 965-978), per image n
 * of the batch (the reference takes image_tensor[0]): map is [N][Cm][H][W] fp32 with Cm = 1 (broadcast over the three channels, the
 * reference's expand(1, 3, 224, 224)) or 3, already at image size; img is [N][3][H][W] of `dtype`, the normalised network input; mean and
 * std are HOST arrays of 3 floats.  With lo / hi the smallest / largest of the Cm * H * W map values of image n,
 *     out[n][c][p] = (((map - lo) / (hi - lo)) * 255) * (1 - alpha) + (((img * std[c] + mean[c]) * 255) * alpha)      (fp32, [N][3][H][W])
 *     lohi[n] = {lo, hi}
 * one rounding per operation (the unit is built with -ffp-contract=off).  Where hi == lo the reference divides by zero; here the heat
 * term is 0.  One 1024-lane workgroup per image reduces and then writes, in one launch; no workspace, no atomics.  N, H or W <= 0, Cm
 * outside {1, 3}, a null pointer, an unknown dtype and N * 3 * H * W overflowing int are reported before any launch. */
int pcgan_heatmap_overlay(const float* map, const void* img, const float* mean, const float* std, float alpha, float* out, float* lohi,
                          int N, int Cm, int H, int W, int dtype, pcgan_stream_t s);

/* ---- online pair selection + draw-aware BCE of siamese_online.py (csrc/online_pair.hip) ---------------------------------------------------
 * What the reference's online trainer does between the encoder's forward pass and backward().  Replaces
 *   EmbeddingDistancePairSelector.get_pairs (three .cpu() copies, numpy argsort, LongTensor, .cuda())        siamese_online.py:218-265
 *   OnlineBinaryCrossEntropyLoss.__call__ (LUT[label], index, two logsigmoid, mean)                          siamese_online.py:324-342
 *   get_prediction (sigmoid, the draw band, the compares; stats.mode over one element is the identity)       siamese_online.py:385-394
 *   (feat1.pow(2).mean() + feat2.pow(2).mean()) * lambda_regularization                                      siamese_online.py:630-635
 * and their backward pass, in ONE launch of ONE workgroup: no workspace, no atomics, every order fixed, bit-identical from run to run.
 * f1, f2: [N] fp32 ratings; label: [N] int64 in 0 .. 2 (clamped to that range); key: [N] fp32 or NULL.  1 <= N <= 4096, 1 <= k <= N.
 *   s[n]      = f1[n] - f2[n] (fp32);  key[n] = s[n] * s[n] (fp32, the bits of the reference's (A - B).pow(2)) unless key is given
 *   order     ascending by key, equal keys by ascending index (stable), -0 == +0, NaN after +inf (numpy's order); descending != 0 is the
 *             exact reverse of that list (the reference's [::-1]), so equal keys then come with the higher index first
 *   sel       the first k of the order;  pseudo: the last k, in list order (they overlap when 2 k > N)
 *   target    t[n] = (1, 0.5, 0)[label[n]]: LABEL 0 MEANS "THE FIRST RATES HIGHER" -- the reverse of siamese.py's BinaryNLLLoss (0, 0.5, 1)
 *   loss[0]   = (1 / k) sum over sel of -(t logsigmoid(s) + (1 - t) logsigmoid(-s)),  logsigmoid(x) = min(x, 0) - log1p(exp(-|x|))
 *   loss[1]   = lambda_reg (mean(f1^2) + mean(f2^2))  (0 for lambda_reg == 0);   loss[2] = loss[0] + loss[1]
 *             float64 from the fp32 inputs, each sum in ascending pair index, each of the three rounded to fp32 once
 *   df1[n]    = gscale ( [n in sel] (sigmoid(s) - t) / k + lambda_reg 2 f1[n] / N )       float64, rounded once; ALL N always written
 *   df2[n]    = gscale (-[n in sel] (sigmoid(s) - t) / k + lambda_reg 2 f2[n] / N )
 *   picks     int32 [2 k + N]: sel, pseudo, pred[N];  with p = sigmoid(s) in float64: pred = 1 if |0.5 - p| < draw_thresh, else 0 if
 *             p > 0.5, else 2 (get_prediction with ~idx1 for the `1 - idx1` current torch refuses on bool tensors)
 * draw_thresh, lambda_reg and gscale are fp32 values widened to float64 exactly.  loss, df1, df2 and picks may each be NULL (not wanted).
 * N or k out of range and a null f1 / f2 / label are reported before any launch. */
int pcgan_online_pair_bce(const float* f1, const float* f2, const int64_t* label, const float* key, float* loss, float* df1, float* df2,
                          int32_t* picks, int N, int k, int descending, float draw_thresh, float lambda_reg, float gscale,
                          pcgan_stream_t s);

/* ---- history of generated images (csrc/image_pool.hip) -----------------------------------------------------------------------------------
 * The call site it replaces is the per-image unsqueeze / clone / cat loop of the reference's ImagePool.query, util/image_pool.py:12-32.
 * x and y hold n_img images of n elements of `dtype` (PCGAN_F32 or PCGAN_BF16), pool holds pool_size such images; all contiguous.  plan
 * is a HOST array of n_img int32, one decision per image, carried out IN ORDER i = 0 .. n_img - 1:
 *     plan[i] <  0           pass      y[i] = x[i]
 *     plan[i] == 2 * s       store     pool[s] = x[i]; y[i] = x[i]
 *     plan[i] == 2 * s + 1   exchange  y[i] = old pool[s]; pool[s] = x[i]
 * Later images see earlier images' writes (two images may name one slot: the second receives the first).  The plan reaches the kernel
 * inside its by-value argument, PCGAN_POOL_PLAN_MAX entries per launch; a longer batch takes consecutive launches on the same stream,
 * ceil(n_img / PCGAN_POOL_PLAN_MAX) in all.  A thread owns one index within the image and walks the images serially, so every pool
 * address is read and written by one thread in program order: no atomics, no LDS, no workspace.  Pure copies, bit-exact.  16-byte
 * accesses when x, y, pool and n * sizeof(T) are multiples of 16 bytes, element accesses otherwise; a grid-stride loop on a capped grid.
 * Null pointers, n == 0, n_img < 1, pool_size < 1, a slot outside [0, pool_size), an unknown dtype and any overlap between the byte
 * ranges of x, y and pool are reported before any launch.  pcgan_pool_exchange_launches: kernel launches this entry has issued so far
 * in the process (host counter). */
#define PCGAN_POOL_PLAN_MAX 64
int pcgan_pool_exchange(void* pool, int pool_size, const void* x, void* y, const int* plan, int n_img, size_t n, int dtype,
                        pcgan_stream_t s);
unsigned long long pcgan_pool_exchange_launches(void);

/* ---- kernel timer (measurement only)-----------------------------------------------------------------------------------------------
 * bench.py's roofline block: HIP events on the launch stream around every launch of the three residual-block convolution kernels
 * (kind 0 forward, 1 data gradient, 2 weight gradient incl. its padded copy and reduce, 3 the weight gradient's main kernel),
 * whichever entry point issued them.  pcgan_timer_enable(capacity) creates `capacity` event pairs per kind and switches recording on
 * (0: off, events destroyed); pcgan_timer_read waits for the recorded pairs of one kind, writes their durations in ms (at most cap) and
 * resets that kind; returns the count or -1.  Off by default, never records inside a graph capture. */
/* Non-finite sentinel of the fp16 two-piece route: the kernels that scale their operands by a device-side maximum count the waves that
 * produced an inf / NaN result into *dev_word (a device word the caller owns and zeroes; NULL switches the sentinel off).  An operand
 * element above the maximum its scale came from -- a stale maximum -- overflows fp16 and poisons everything it touches, so a non-zero
 * count means "stale operand maxima or non-finite inputs"; the host checks it where it synchronises anyway. */
int pcgan_set_nonfinite_counter(unsigned int* dev_word);
/* Routing options below the C-ABI (A/B measurement; the defaults are the measured-best settings and need no call).  Set before the
 * calls they affect; *_supported / *_workspace_bytes queries follow the current values.
 *   "bsplit_halo"   1  residual convolutions (3x3 reflect, width 32 / 64) on the window kernel; 0: per-tap gather kernel
 *   "wgrad_gen"     1  weight gradients with zero padding <= 1 apply the padding inside the gather; 0: padded copy of x
 *   "wgrad_padcopy" 0  1: the residual blocks' weight gradient reads a reflection-padded copy of x (round 2's form)
 *   "wgrad_cw"      0  columns per workgroup of the matrix-pipe weight gradient: 0 = as measured (128 for fp32 tensors, 256 for bf16),
 *                      128 / 256 force one form
 *   "hgemm_bf16"    1  bf16 tensors on the one-product bf16 MFMA form of the packed implicit GEMM; 0: fp32 MFMA kernels
 *   "wgrad_direct"  0  1: pcgan_conv2d_bwd_weight_hsplit hands the shapes pcgan_conv2d_wgrad_direct_supported takes to the
 *                      image-innermost form below (round-4 experiment: same results level, no step gain); the workspace query follows
 *   "wgd_look"      3  K steps the operand loads of that form's main kernel run ahead of its MFMAs (2, 3 or 4)
 *   "wgrad_rowring" 1  pcgan_conv2d_bwd_weight_hsplit hands the shapes pcgan_conv2d_wgrad_rowring_supported takes to the row-ring form
 *                      (fp32 tensors: 0.125-0.137 ms against 0.158-0.166 per residual-block call, step + 0.5 %; bf16 tensors: 0.060
 *                      against 0.119, step + 7 %); 0: the per-tap kernel for every shape; 3: the row-ring form for fp32 tensors only
 *   "hgemm_tile"    0  packed implicit GEMM, layers with > 32 output rows: 0 = the library's tile heuristic; BM * 1000 + BP with
 *                      BM, BP in {64, 128} forces the workgroup tile (measurement: scripts/sweep_hgemm.py)
 *   "hgemm_ks"      0  ... and the K split: 0 = heuristic, 1 .. 8 forced (every layer's workspace query then includes the partial sums)
 *   "wgrad_ks"      0  pcgan_conv2d_bwd_weight: 0 = the library's split heuristic; 1 .. 512 forces that many pixel (strip) splits for
 *                      every kernel family, cut to [1, chunks of 32 pixels (strips)] and not held to the heuristic's 8-chunk floor; the
 *                      chunks of a split and the final count are re-derived as always, and the workspace query follows (tests:
 *                      tests/test_gpu_wgrad_generic.py; the host maps no environment variable onto it)
 *   "hwgrad_ks"     0  pcgan_conv2d_bwd_weight_hsplit, per-tap kernel: 0 = the library's split heuristic; 1 .. 512 forces that many splits
 *                      of the pixel reduction, cut to [1, stages of 16 output columns] and not held to the heuristic's 8-stage floor; the
 *                      stages of a split and the final count are re-derived as always, and
 *                      pcgan_conv2d_hsplit_wgrad_workspace_bytes follows (tests: tests/test_gpu_hsplit_wgrad_cases.py; the host maps no
 *                      environment variable onto it)
 * Unknown keys / values return non-zero. */
int pcgan_set_option(const char* key, int value);
int pcgan_get_option(const char* key, int* value);
int pcgan_timer_enable(int capacity);
int pcgan_timer_read(int kind, float* ms, int cap);
/* Launch record of the implicit-GEMM family (host memory, no synchronisation): what the last forward / data-gradient call of
 * pcgan_conv2d_fwd* / pcgan_conv2d_bwd_data* that reached the implicit GEMM launched, after every clamp of a forced "hgemm_tile" /
 * "hgemm_ks".  info[0 .. n) = {sequence number (+1 per recorded launch), form (PCGAN_IGEMM_*), mode (0 forward zero padding, 1 forward
 * reflection padding, 2 data gradient, 3 data gradient gathering reflection mirrors), BM, BP, K split, phases}; entries past
 * PCGAN_IGEMM_LAUNCH_INFO are 0.  PCGAN_IGEMM_SMALLM has no tile: there BM names the kernel (1 strip, 2 few taps, 3 generic), BP the strip
 * kernel's instantiation as NR * 10 + MO (43, 44, 73, 74; 0 for the other two) and the K split is the strip kernel's channel split.
 * The thin kernels do not record; the bsplit entries (per-tap and window kernel) have a record of their own, pcgan_bsplit_last_launch. */
#define PCGAN_IGEMM_LAUNCH_INFO 7
#define PCGAN_IGEMM_HGEMM_F16X2 1  /* hgemm_kernel, fp32 tensors as two scaled fp16 pieces */
#define PCGAN_IGEMM_HGEMM_BF16 2   /* hgemm_kernel, bf16 tensors, one product */
#define PCGAN_IGEMM_IGEMM2_CG16 3  /* igemm2_kernel, chunked K order (multiple of 16 gathered channels), fp32 MFMA */
#define PCGAN_IGEMM_IGEMM2_CG4 4   /* igemm2_kernel, 3- / 4-channel gathered tensor */
#define PCGAN_IGEMM_GENERIC 5      /* igemm_kernel, generic K order */
#define PCGAN_IGEMM_SMALLM 6       /* <= 4 output channels, vector ALU */
int pcgan_igemm_last_launch(int* info, int n);
/* Launch record of pcgan_conv2d_bwd_weight (host memory, no synchronisation; a record of its own: the one above does not move when a weight
 * gradient runs): which instantiation its last call launched, after every clamp of a forced "wgrad_ks".  info[0 .. n) = {sequence number
 * (+1 per recorded launch), family (PCGAN_WGRAD_*), padding mode (0 zero, 1 reflection), BM (0 for the small-M kernels), VECA (dY fetched
 * four pixels at a time; tile kernels only), variant (see the families), storage type (PCGAN_F32 / PCGAN_BF16), splits, units per split
 * (chunks of 32 pixels; strips for PCGAN_WGRAD_STRIP)}; entries past PCGAN_WGRAD_LAUNCH_INFO are 0.  The per-tap (hsplit) weight gradient
 * has a record of its own (pcgan_hwgrad_last_launch below), the bsplit weight gradient too (pcgan_bsplit_last_launch); the row-ring / direct forms do not record. */
#define PCGAN_WGRAD_LAUNCH_INFO 9
#define PCGAN_WGRAD_TILE2 1   /* wgrad2_kernel (tap-aligned K tiles, pipelined); variant = taps per K tile, 2 | 1 */
#define PCGAN_WGRAD_TILE 2    /* wgrad_kernel; variant = KMODE 0 (generic) | 1 (per-thread tap) | 2 (one tap per K tile) */
#define PCGAN_WGRAD_SMALLM 3  /* smallm_wgrad_kernel (<= 4 output channels, multiple of 16 padded channels); variant 0 */
#define PCGAN_WGRAD_STRIP 4   /* smallm_wgrad_strip_kernel (<= 3 output channels, stride 1); variant = NT 4 | 7 */
int pcgan_wgrad_last_launch(int* info, int n);
/* Launch record of the per-tap weight gradient (hsplit_wgrad_kernel; host memory, no synchronisation, a record of its own): written by
 * pcgan_conv2d_bwd_weight_hsplit only when it issues the launch of the per-tap kernel itself (an attempted launch: the record is
 * written before the launch status is read, as pcgan_wgrad_last_launch's is) -- a call it hands to the row-ring or direct form does
 * not move it.  info[0 .. n) = {sequence number (+1 per recorded launch), BM (128 | 256), stride, storage type (PCGAN_F32 / PCGAN_BF16),
 * columns per workgroup (128 | 256), form (0 separable gather of a padded copy or of an unpadded tensor, 1 reflection applied in the
 * gather, 2 GEN: zero padding applied in the gather), padded copy (0 none, 1 made by the element-per-thread kernel, 2 by the
 * wave-per-plane kernel), row tiles, column tiles, splits (after every clamp of a forced "hwgrad_ks"), stages per split, stages in all};
 * entries past PCGAN_HWGRAD_LAUNCH_INFO are 0. */
#define PCGAN_HWGRAD_LAUNCH_INFO 12
int pcgan_hwgrad_last_launch(int* info, int n);
/* Launch record of the bsplit entries (host memory, no synchronisation, a record of its own): written by pcgan_conv2d_fwd_bsplit,
 * pcgan_conv2d_bwd_data_bsplit and pcgan_conv2d_bwd_weight_bsplit when they issue the launch of their main kernel (an attempted launch:
 * the record is written before the launch status is read).  info[0 .. n) = {sequence number (+1 per recorded launch), kernel (0 the
 * per-tap kernel bsplit_conv_fwd_kernel, 1 the window kernel bsplit_halo_kernel), mode (per-tap: 0 forward zero padding, 1 forward
 * reflection padding, 2 data gradient, 3 weight gradient; window: 0 forward, 1 data gradient), BM (128 | 256), storage type (PCGAN_F32 /
 * PCGAN_BF16), row tiles, pixel tiles of 128 pixels (weight gradient: column tiles of 128 columns (c, r, s); data gradient of the per-tap
 * kernel: the tiles of its three row classes together), stages in all, splits of the reduction (1 outside the weight gradient), stages
 * per split, padded copy of the weight gradient (0 none, 1 element-per-thread kernel, 2 wave-per-plane kernel)}; entries past
 * PCGAN_BSPLIT_LAUNCH_INFO are 0. */
#define PCGAN_BSPLIT_LAUNCH_INFO 11
int pcgan_bsplit_last_launch(int* info, int n);

#ifdef __cplusplus
}
#endif
#endif /* PCGAN_HIP_H */
