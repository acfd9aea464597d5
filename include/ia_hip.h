/*
 * ia_hip.h -- C ABI of libia_hip.so, the MI355X (gfx950) backend for the InvertAvatar
 * generator forward pass.
 *
 * This is the drop-in boundary.  Each entry point replaces one
 * pybind11 plugin function or one PyTorch-level stage of the reference and is what a
 * reference-side binding (ctypes) would call.  Conventions:
 *
 *   - plain pointers + explicit sizes/strides, no torch types;
 *   - every pointer is a DEVICE pointer unless its name starts with `h_`;
 *   - the CALLER allocates all outputs and scratch; the library keeps no pointer past
 *     the call and owns no device memory;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *   - return value: 0 on success, negative ia_status on failure; the message of the last
 *     failure on the calling thread is available from ia_last_error();
 *   - nothing throws across the ABI; the library is re-entrant: it keeps no mutable state that a result depends on.  The one
 *     mutable device word per kernel module is the fp16 range watch (a sticky diagnostic flag, OR-ed by the kernels that write the
 *     split format when a value leaves the fp16 range, read and cleared by ia_split_saturation_poll -- an errno, not an input).
 *
 * Element types are named by ia_dtype.  "f16" is IEEE binary16 (the reference's c10::Half).
 */
#ifndef IA_HIP_H_
#define IA_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IA_HIP_ABI_VERSION 7      /* 7 (additive): ia_raycast_scratch_bytes, ia_volume_bricks, ia_raycast_volume, ia_volume_gradient; 7 (additive): ia_query_planes, ia_density_grid, ia_mc_scratch_bytes, ia_mc_count, ia_mc_emit; 7 (r06, additive): ia_tokens_split / _t, ia_layernorm_split, ia_dwconv3x3_tokens_split, ia_im2col_split, ia_linear_sx / _splitk / _splitk_plan, ia_matmul_sx, ia_softmax_split, ia_attention_sx / _supported; 6 (r06): ia_render_rays (+ rgb_split, rgb_split_styles, rgb_split_planes), + ia_render_rays_box, ia_ray_limits_box / _parts; 5 (r05; ia_conv2d_mfma_sx_rgb narrowed to n <= 3 fused ToRGB channels, otherwise additive): ia_conv2d_down_sx / _plan, ia_conv3x3_s2_tiny, ia_bn_train_split, ia_convgru_gates_split / _update_split, ia_dwconv3x3_tokens, ia_se_gate_split, ia_upsample_bilinear_add; 4 (r04): + ia_upconv2d_rows_sx / _plan, ia_mouth_edge_blur, ia_split_saturation_poll, ia_conv2d_sx_supported; - ia_conv2d_small; 3 (r03, additive): ia_torgb, ia_upconv2d_fir_sx; 2 (r03): ia_render_rays (+ u_importance), ia_act_split (+ shift), ia_conv2d_mfma_sx (+ prelu_alpha), ia_uv_rasterize (+ binarize_mask) */

typedef enum ia_status {
    IA_OK = 0,
    IA_ERR_INVALID_ARG = -1,   /* the reference's TORCH_CHECK failures            */
    IA_ERR_UNSUPPORTED = -2,   /* valid per the reference API, no kernel here yet  */
    IA_ERR_LAUNCH = -3,        /* hipGetLastError() after the launch               */
    IA_ERR_NO_DEVICE = -4
} ia_status;

typedef enum ia_dtype { IA_F32 = 0, IA_F16 = 1, IA_F64 = 2 } ia_dtype;

/* Activation ids are the reference's `cuda_idx` (torch_utils/ops/bias_act.py:23-33). */
typedef enum ia_act {
    IA_ACT_LINEAR = 1, IA_ACT_RELU = 2, IA_ACT_LRELU = 3, IA_ACT_TANH = 4, IA_ACT_SIGMOID = 5,
    IA_ACT_ELU = 6, IA_ACT_SELU = 7, IA_ACT_SOFTPLUS = 8, IA_ACT_SWISH = 9
} ia_act;

/* ABI version of the loaded library (== IA_HIP_ABI_VERSION it was built with). */
int ia_version(void);

/* Copies the calling thread's last error message (NUL-terminated, truncated to n) and
 * returns its full length.  Replaces the C++ exception text of TORCH_CHECK
 * (torch_utils/ops/bias_act.cpp:39-55). */
size_t ia_last_error(char* h_buf, size_t n);

/* Number of HIP devices visible, or a negative ia_status. */
int ia_device_count(void);

/*
 * Fused bias + activation + gain + clamp.
 * Replaces bias_act_plugin.bias_act(x, b, xref, yref, dy, grad, dim, act, alpha, gain, clamp)
 * (torch_utils/ops/bias_act.cpp:36-93; kernel bias_act.cu:27-151).
 *   x, y       : `numel` elements of `dtype`, any dense layout (indexing is by memory offset)
 *   b          : `size_b` elements of `dtype` or NULL; element i uses b[(i / step_b) % size_b],
 *                step_b = x.stride(dim) exactly as bias_act.cpp:77
 *   xref/yref/dy : NULL for grad == 0; same layout as x otherwise (bias_act.py:181,200)
 *   grad       : 0 forward, 1 first-order, 2 second-order gradient kernel
 *   clamp < 0  : disabled
 */
int ia_bias_act(const void* x, const void* b, const void* xref, const void* yref, const void* dy, void* y,
                int dtype, int64_t numel, int size_b, int64_t step_b,
                int grad, int act, float alpha, float gain, float clamp, void* stream);

/*
 * Up-sample (zero insert) -> pad/crop -> 2-D FIR -> down-sample, per channel.
 * Replaces upfirdn2d_plugin.upfirdn2d(x, f, upx, upy, downx, downy, padx0, padx1, pady0, pady1,
 * flip, gain) (torch_utils/ops/upfirdn2d.cpp:20-102; kernels upfirdn2d.cu:33-204).
 *   x          : [n, c, in_h, in_w] of `dtype`, element strides x_stride[4] (N,C,H,W order)
 *   f          : [f_h, f_w] float32, element strides f_stride[2] (H,W order)
 *   y          : [n, c, out_h, out_w] of `dtype`, element strides y_stride[4]; the caller sizes
 *                it with out = (in*up + pad0 + pad1 - f + down) / down (upfirdn2d.cpp:39-40)
 *   flip != 0  : correlate with f as given; flip == 0 : true convolution (f flipped)
 */
int ia_upfirdn2d(const void* x, const float* f, void* y, int dtype,
                 int n, int c, int in_h, int in_w, const int64_t* h_x_stride,
                 int f_h, int f_w, const int64_t* h_f_stride,
                 int out_h, int out_w, const int64_t* h_y_stride,
                 int upx, int upy, int downx, int downy, int padx0, int pady0,
                 int flip, float gain, void* stream);

/*
 * ia_upfirdn2d with the tail of a StyleGAN2 SynthesisLayer fused in:
 *     y = clamp(act(FIR(x) + noise * noise_strength + bias[c]) * act_gain)
 * Replaces the upfirdn2d call of conv2d_resample (torch_utils/ops/conv2d_resample.py:128) plus the noise add
 * and bias_act of SynthesisLayer.forward (training/networks_stylegan2.py:318-329) for up-sampling layers.
 *   x  : [n, c, in_h, in_w] contiguous NCHW of `dtype` (f32/f16);  f : [f_h, f_w] contiguous float32
 *   noise : [out_h*out_w] float32 or NULL;  noise_strength : device scalar float32 or NULL (= 1)
 *   bias  : [c] of `dtype` or NULL;  act : IA_ACT_LINEAR | IA_ACT_LRELU;  clamp < 0 disables
 *   up in {1, 2}, 4x4 filter; other shapes return IA_ERR_UNSUPPORTED (use ia_upfirdn2d + ia_bias_act).
 */
int ia_upfirdn2d_bias_act(const void* x, const float* f, const float* noise, const float* noise_strength,
                          const void* bias, void* y, int dtype, int n, int c, int in_h, int in_w,
                          int f_h, int f_w, int out_h, int out_w, int up, int padx0, int pady0,
                          int flip, float fir_gain, int act, float alpha, float act_gain, float clamp, void* stream);

/*
 * Dense fp32 convolution of one StyleGAN2 layer on MFMA (v_mfma_f32_32x32x2_f32), with the modulation,
 * demodulation and the layer tail fused:
 *     y[b,o] = clamp(act(demod[b,o] * conv(x[b] * styles[b,:], w)[o] + noise * noise_strength + bias[o]) * gain) + residual
 * Replaces modulated_conv2d (training/networks_stylegan2.py:34-91) -> conv2d_resample
 * (torch_utils/ops/conv2d_resample.py:114-136) -> cuDNN conv2d / conv_transpose2d
 * (torch_utils/ops/conv2d_gradfix.py:37-45), and for the stride-1 form the bias_act after it (:327-329).
 *   x        : [B, I, H, W] float32 contiguous
 *   wk       : weights repacked as [ksize*ksize][I][O] float32 (tap-major, O contiguous) from the reference's
 *              [O, I, kh, kw]; tap = ky*ksize + kx, no spatial flip
 *   styles   : [B, I] or NULL;  demod : [B, O] or NULL (see ia_modconv_demod)
 *   transposed = 0 : stride 1, zero padding ksize/2 (correlation, as F.conv2d);  y : [B, O, H, W]
 *   transposed = 1 : 3x3, stride 2, no padding = F.conv_transpose2d(x, w^T, stride=2);  y : [B, O, 2H+1, 2W+1];
 *                    only `demod` is applied (noise/bias/residual must be NULL, act linear) -- the FIR and the
 *                    tail follow in ia_upfirdn2d_bias_act
 *   ksplit   : number of stream-K workers per batch element (from ia_conv2d_plan; 0 when the plan has none).  Tiles that
 *              fill whole rounds of the machine run one per workgroup; the (tile, K-chunk) units of the remaining tiles are
 *              cut into `ksplit` equal ranges, and tiles shared between workers are summed in worker order by a
 *              deterministic fix-up pass
 *   scratch  : caller-owned accumulator slabs for that pass, `scratch_bytes` >= the planned size (NULL/0 when the plan needs
 *              none).  Launches that may run concurrently must not share a scratch buffer.
 */
int ia_conv2d_mfma(const float* x, const float* wk, const float* styles, const float* demod,
                   const float* noise, const float* noise_strength, const float* bias, const float* residual,
                   float* y, float* scratch, size_t scratch_bytes,
                   int B, int I, int O, int H, int W, int ksize, int transposed,
                   int act, float alpha, float gain, float clamp, int ksplit, void* stream);

/*
 * ia_conv2d_mfma with fp16 operands on v_mfma_f32_32x32x16_f16 and fp32 accumulation: the arithmetic of the reference's
 * fp16 blocks (modulated_conv2d with x.dtype == float16, training/networks_stylegan2.py:34-91; the SR head with
 * sr_num_fp16_res > 0, training_avatar_texture/superresolution.py:209-216).  The style-scaled input and the weights are
 * rounded to fp16, everything else (demodulation, noise, bias, activation, clamp, storage) stays fp32.
 *   wk_h : weights as fp16, packed [ksize*ksize][I/8][O][8] (channel octets innermost), from the reference's [O, I, kh, kw]
 * Same arguments, plan and scratch as ia_conv2d_mfma.  Covers 3x3 layers that run on the two-stage tiles (stride-1 layers
 * with O >= 128 and >= 32^2 outputs; every stride-2 transposed layer) with I % 8 == 0 and O % 4 == 0; other shapes return
 * IA_ERR_INVALID_ARG and the caller uses ia_conv2d_mfma.
 */
int ia_conv2d_mfma_h(const float* x, const void* wk_h, const float* styles, const float* demod,
                     const float* noise, const float* noise_strength, const float* bias, const float* residual,
                     float* y, float* scratch, size_t scratch_bytes,
                     int B, int I, int O, int H, int W, int ksize, int transposed,
                     int act, float alpha, float gain, float clamp, int ksplit, void* stream);

/*
 * ia_conv2d_mfma with fp32-equivalent products formed from fp16 pairs on v_mfma_f32_32x32x16_f16 (fp32 accumulation):
 * every operand v is split as hi = fp16(v), lo = fp16(v - hi) -- 22 mantissa bits together -- and a*b is taken as
 * a_hi*b_hi + a_hi*b_lo + a_lo*b_hi.  The dropped a_lo*b_lo is <= 2^-22 |a*b|, the size of fp32's own rounding, so the
 * result is an fp32 convolution (measured against an fp64 convolution it is as close as ia_conv2d_mfma) at 3/16 of the fp32
 * MFMA's cycles.  The MFMA flushes fp16 denormals, so every factor is kept a normal number: the weights are scaled by
 * 2^wk_exp at pack time (wk_exp chosen per layer so that max|w| * 2^wk_exp <= 32768), the low parts of the activations by
 * 2^11, and the high part of a weight is multiplied by 2^-11 (exact) where it meets an activation's low part -- all three
 * products then carry the factor 2^wk_exp and go to ONE fp32 accumulator, which is multiplied by 2^-wk_exp at the end.
 * Range: x * style saturates at +-65504 (StyleGAN2 activations are O(1)-O(100); the reference clamps its fp16 blocks at
 * 256); weights below 2^(-3-wk_exp) lose the a_hi*b_lo correction, activations below 2^-14 = 6.1e-5 are carried by their
 * (scaled) low part alone, i.e. with 11 mantissa bits.
 *   wk_split : fp16 [2 (hi, lo)][ksize*ksize][I/8][O][8] of w * 2^wk_exp
 *   wk_exp   : the power of two above
 * Other arguments, plan, scratch and shape coverage as ia_conv2d_mfma_h.
 */
int ia_conv2d_mfma_s(const float* x, const void* wk_split, int wk_exp, const float* styles, const float* demod,
                     const float* noise, const float* noise_strength, const float* bias, const float* residual,
                     float* y, float* scratch, size_t scratch_bytes,
                     int B, int I, int O, int H, int W, int ksize, int transposed,
                     int act, float alpha, float gain, float clamp, int ksplit, void* stream);

/* Host-only planner for ia_conv2d_mfma (form 0), ia_conv2d_mfma_h (form 1) and ia_conv2d_mfma_s (form 2): stream-K worker count
 * (0: none) and the scratch bytes the fix-up pass needs.  The tile family, and with it the plan, depends on the form. */
int ia_conv2d_plan(int B, int I, int O, int H, int W, int ksize, int transposed, int form, int* h_ksplit, size_t* h_scratch_bytes);

/*
 * Demodulation coefficients demod[b,o] = rsqrt(sum_i styles[b,i]^2 * wsq[o,i] + 1e-8) with
 * wsq[o,i] = sum_{ky,kx} w[o,i,ky,kx]^2 (training/networks_stylegan2.py:60-64).
 */
int ia_modconv_demod(const float* styles, const float* wsq, float* demod, int B, int I, int O, void* stream);

#define IA_RENDER_WHITE_BACK 1
#define IA_RENDER_RGB_CHANNEL_MAJOR 2
#define IA_RENDER_DIST_PER_FRAME 4
#define IA_RENDER_FLIP_Z 8            /* ia_render_rays_box only */

/*
 * The fused importance renderer: one launch replaces ImportanceRenderer_bsMotion.forward(evaluation=True)
 * (training_avatar_texture/volumetric_rendering/renderer.py:309-351) together with sample_from_planes (:85-97),
 * OSGDecoder.forward (training_avatar_texture/triplane_v20.py:426-438) and MipRayMarcher2.run_forward
 * (volumetric_rendering/ray_marcher.py:25-57).
 *   planes_cl : [B, 3, plane_h, plane_w, 32] float32 -- the tri-planes in CHANNELS-LAST order (the reference's
 *               [B, 3, 32, H, W] permuted so that a texel's 32 channels are one 128-byte line)
 *   rays_o/d  : [B, R, 3];  jitter : [B, R, 48] in [0,1), the stratified-sampling noise of renderer.py:406
 *   u_importance : NULL = evaluation mode, the importance pass inverts the CDF on the grid linspace(0, 1, 48) (renderer.py:450);
 *               else [B, R, 48] uniform draws in [0,1) (the torch.rand of renderer.py:453), SORTED ascending per ray (the inverse
 *               CDF is monotone, so the fine depths then come out sorted and the merged order equals torch.sort of :361)
 *   dist      : device scalar = mean |ray origin| over the WHOLE batch (renderer.py:311); ray_start/end are
 *               derived from it in-kernel exactly as :313 does in Python doubles
 *   w0,b0,w1,b1 : OSGDecoder parameters net.0.weight [64,32], net.0.bias [64], net.2.weight [33,64], net.2.bias [33]
 *               (un-scaled; lr_multiplier = decoder_lr_mul is applied as FullyConnectedLayer does)
 *   n_coarse / n_importance : must both be 48 (train_avatar_texture.py:341-342); others -> IA_ERR_UNSUPPORTED
 *   flags : bit 0 (IA_RENDER_WHITE_BACK) = rendering_kwargs['white_back']; bit 1 (IA_RENDER_RGB_CHANNEL_MAJOR) = store rgb as
 *          [B, 32, R] -- the feature image [B, 32, nrr, nrr] the super-resolution head reads (triplane_v20.py:313) -- instead of
 *          the renderer's [B, R, 32], which saves the permute + copy between the renderer and the head; bit 2
 *          (IA_RENDER_DIST_PER_FRAME) = `dist` holds B values, frame b uses dist[b]: a batch of frames that the script renders one
 *          call each (eval_seq.py:206-212, where `dist` is every frame's own |ray origin|) keeps those results when batched
 *   rgb  : [B, R, 32] (or [B, 32, R], see flags) composited features scaled to (-1, 1);  depth : [B, R] clamped to the
 *          batch-global sample range (ray_marcher.py:50), with IA_RENDER_DIST_PER_FRAME to every frame's own sample range (what the
 *          one-call-per-frame script computes);  wsum : [B, R] sum of compositing weights
 *   minmax_scratch : 2 * ia_render_rays_grid(B, R) floats of caller scratch; with IA_RENDER_DIST_PER_FRAME 8 * B times that
 *          (one range per wave and frame)
 *   rgb_split : NULL, or a second copy of rgb in the operand format of the convolution that consumes the feature image (the SR head's
 *          first layer, superresolution.py:287 -> block0.conv0): fp16 [B, rgb_split_planes, 4, R, 8] (ia_act_split's format: 2 = hi / lo
 *          planes, 1 = one rounded plane) of rgb[b, c, r] * rgb_split_styles[b, c] ([B, 32] or NULL = unscaled) -- bit for bit what
 *          ia_act_split makes of the channel-major image, without the launch between the renderer and the head (r06)
 *   dbg_* : optional stage outputs for parity tests (NULL in production): fine depths [B,R,48], searchsorted
 *          indices [B,R,48] (int32), merge order [B,R,96] (int32, < 48 = coarse sample, >= 48 = fine sample),
 *          coarse weights [B,R,47], coarse densities [B,R,48]
 */
int ia_render_rays(const float* planes_cl, const float* rays_o, const float* rays_d, const float* jitter,
                   const float* u_importance, const float* dist, const float* w0, const float* b0, const float* w1, const float* b1,
                   float lr_multiplier, float box_warp, int flags,
                   int B, int R, int plane_h, int plane_w, int n_coarse, int n_importance,
                   float* rgb, float* depth, float* wsum, float* minmax_scratch,
                   float* dbg_z_fine, int* dbg_inds, int* dbg_order, float* dbg_w_coarse, float* dbg_sigma_coarse,
                   void* rgb_split, const float* rgb_split_styles, int rgb_split_planes, void* stream);

/* Number of persistent workgroups ia_render_rays launches for (B, R); sizes minmax_scratch. Host-only. */
int ia_render_rays_grid(int B, int R);

/*
 * The same fused launch for the EG3D renderer class, ImportanceRenderer.forward
 * (training_avatar_texture/volumetric_rendering/renderer.py:129-201; run_model :195-202, sample_stratified :224-247,
 * sample_importance / sample_pdf :249-293).  Differences from ia_render_rays:
 *   ray_limits : [B, R, 2] per-ray (near, far) -- rendering_options['ray_start'] == ['ray_end'] == 'auto', the output of
 *               ia_ray_limits_box -- sampled with math_utils.linspace (math_utils.py:101-118) and per-ray noise scale (:236-238);
 *               NULL = the fixed range [ray_start, ray_end] (the options' python doubles) through torch.linspace (:240-242)
 *   u_importance : required -- this class always draws its importance samples (sample_pdf det=False, :280); sorted per ray
 *   flags : IA_RENDER_WHITE_BACK, IA_RENDER_RGB_CHANNEL_MAJOR as above; IA_RENDER_FLIP_Z = the class's flip_z (the z coordinate of
 *          every sample is negated before the plane lookup, :196-197); IA_RENDER_DIST_PER_FRAME is rejected
 * Everything else (decoder, ray marcher, batch-global depth clamp, scratch, debug outputs) as ia_render_rays.
 */
int ia_render_rays_box(const float* planes_cl, const float* rays_o, const float* rays_d, const float* jitter,
                       const float* u_importance, const float* ray_limits, double ray_start, double ray_end,
                       const float* w0, const float* b0, const float* w1, const float* b1,
                       float lr_multiplier, float box_warp, int flags,
                       int B, int R, int plane_h, int plane_w, int n_coarse, int n_importance,
                       float* rgb, float* depth, float* wsum, float* minmax_scratch,
                       float* dbg_z_fine, int* dbg_inds, int* dbg_order, float* dbg_w_coarse, float* dbg_sigma_coarse,
                       void* stream);

/*
 * math_utils.get_ray_limits_box (volumetric_rendering/math_utils.py:46-98): slab test of n_rays rays (rays_o / rays_d [n_rays, 3])
 * against the axis-aligned cube of side box_side_length centred at the origin -> ray_limits [n_rays, 2] = (t_near, t_far),
 * (-1, -2) for a ray that misses.  repair_misses != 0 additionally applies ImportanceRenderer.forward's repair (renderer.py:133-136)
 * on the device, without the reference's `.item()` round trip: if any ray hits, every missing ray gets (min, max) of the hit rays'
 * NEAR limits.  part_scratch: 2 * ia_ray_limits_box_parts(n_rays) floats of caller scratch.
 */
int ia_ray_limits_box(const float* rays_o, const float* rays_d, double box_side_length, int n_rays, int repair_misses,
                      float* ray_limits, float* part_scratch, void* stream);
int ia_ray_limits_box_parts(int n_rays);      /* host-only */

/*
 * Stage entry for parity tests: smoothed inverse-CDF importance resampling (renderer.py:410-469, det=True) and the
 * stable merge order (unify_samples :372-382) from GIVEN coarse depths [nrays,48] and coarse weights [nrays,47].
 * Runs the same device code as ia_render_rays.  z_fine [nrays,48], inds [nrays,48] int32, order [nrays,96] int32.
 */
int ia_importance_stage(const float* z_coarse, const float* w_coarse, float* z_fine, int* inds, int* order,
                        int nrays, void* stream);

/*
 * Mouth-hole mask of the rasterised face alpha, entirely on the device.
 * Replaces the cv2.floodFill round trip of fill_mouth(images, blur_mouth_edge=False)
 * (training_avatar_texture/volumetric_rendering/renderer.py:716-741): v = alpha*255; pixels with
 * v(0,0) <= v <= v(0,0)+254 that are 4-connected to pixel (0,0) are "outside";  mouth = outside ? 0 : (255 - v)/255.
 *   alpha, mouth : [B, H, W] float32 contiguous.  H*(W+4) bytes must fit in LDS (<= 150 KiB; 256x256 is 65 KiB).
 */
int ia_fill_mouth(const float* alpha, float* mouth, int B, int H, int W, void* stream);

/*
 * The soft mouth mask of fill_mouth(images, blur_mouth_edge=True) -- the function's default -- from ia_fill_mouth's result
 * (renderer.py:732-736): copyImg = cv2.blur(cv2.erode(filled, ones(3,3), iterations=3), (5,5));  out = (255 - copyImg) / 255,
 * where filled = 255 on reached pixels (mouth == 0) and alpha*255 elsewhere.  cv2 semantics restated (OpenCV 4.6 is not in
 * this image: parity unpinned by reference tests): erosion border = +inf, box filter on CV_32F sums in double, multiplies by
 * the double 1/25, rounds to float, border BORDER_REFLECT_101.
 *   alpha, mouth, out : [B, H, W] float32 contiguous, H, W >= 3.
 */
int ia_mouth_edge_blur(const float* alpha, const float* mouth, float* out, int B, int H, int W, void* stream);

/*
 * One pyramid level of TriPlaneGenerator.rasterize (training_avatar_texture/triplane_v20.py:328-337) in one pass:
 *     out[:, :C] = AA(grid_sample(texture, uv)) * AA(alpha) + AA(static[:, :, bbox]) * (1 - AA(alpha));  out[:, C] = AA(upper_alpha)
 * where AA = F.interpolate(bilinear, antialias=True) to res x res and grid_sample = bilinear / zeros / align_corners False.
 *   tex_cl      : [B, tex_res, tex_res, C] float32 -- the texture level in CHANNELS-LAST order
 *   uv          : [B, 256, 256, 3] float32 = mesh_condition['uvcoords_image'] (u, v, mask)
 *   upper_alpha : [B, 256, 256] float32 = clamp(mask + upper-mouth mask, 0, 1) (triplane_v20.py:324-326)
 *   sta         : static feature level, NCHW with batch stride `sta_batch_stride` elements (lets plane 0 of a 96-channel
 *                 level be passed without a copy); rows by0:by1, columns bx0:bx1 are resized to res x res
 *   out         : [B, C+1, res, res] float32;   res in {32, 64, 128}
 */
int ia_rasterize_level(const float* tex_cl, const float* uv, const float* upper_alpha, const float* sta, int64_t sta_batch_stride,
                       float* out, int B, int C, int tex_res, int sta_res, int res, int by0, int by1, int bx0, int bx1, void* stream);

/*
 * Tri-plane blend of triplane_v20.py:119-128, written straight in the renderer's layout: the 256^2 face stitch and the
 * mouth-filled alpha are AA-resized to (y1-y0)^2 = 128^2, pasted at rows y0:y1 / columns x0:x1 of plane 0 and blended over
 * the static planes; planes 1-2 are the static planes.
 *   stitch [B,32,256,256], full_alpha [B,256,256], static_planes [B,3*32,256,256] (batch stride in elements given),
 *   planes_cl [B,3,256,256,32] float32.
 */
int ia_blend_planes(const float* stitch, const float* full_alpha, const float* static_planes, int64_t sta_batch_stride,
                    float* planes_cl, int B, int y0, int y1, int x0, int x1, void* stream);

/*
 * Channels-last copy of a feature map, [B,C,H,W] -> [B,H,W,C] (float32, contiguous): the layout ia_rasterize_level gathers its
 * texture level from (`tex_cl`).  Replaces the permute + contiguous copy the gather formulation of TriPlaneGenerator.rasterize
 * (training_avatar_texture/triplane_v20.py:328-337: F.grid_sample over an NCHW texture) needs on this backend; 64 x 64 tiles through
 * LDS, reads and writes in 256-byte runs.
 */
int ia_channels_last(const float* x, float* y, int B, int C, int H, int W, void* stream);

/*
 * Paste of a rasterised condition over features or the skip image inside the face backbone
 * (training_avatar_texture/networks_stylegan2_new.py:537-540):  y = cond[:, :C] * a + x * (1 - a),  a = cond[:, C:C+1].
 *   cond : [B, C+1, H, W] float32 (last channel = alpha);  x, y : [B, C, H, W] float32;  H*W % 4 == 0.
 */
int ia_cond_blend(const float* cond, const float* x, float* y, int B, int C, int H, int W, void* stream);

/*
 * All affine style vectors and demodulation coefficients of one synthesis network in two launches.
 * Replaces, per layer, FullyConnectedLayer.forward of `.affine` (training/networks_stylegan2.py:114-127, called at :318
 * and :353) and the demodulation reduction of modulated_conv2d (:60-64):
 *     styles[b, soff_l + i] = dot(ws[b, widx_l, :], A_l[i, :]) * wgain_l + bias_l[i] * bgain_l
 *     demod[b, doff_l + o]  = rsqrt(sum_i styles[b, soff_l + i]^2 * wsq_l[o, i] + 1e-8)
 *   ws          : [B, num_ws, w_dim] float32
 *   layer_table : device int64 [L][8] = {A ptr ([I,w_dim] f32), bias ptr ([I] f32), wsq ptr ([O,I] f32 or 0), I, O, widx, soff, doff}
 *   layer_gains : device float [L][2] = {weight gain, bias gain}
 *   style_row_layer [style_rows] / demod_row_layer [demod_rows] : device int32 maps from output row to layer
 *   styles : style_rows * B floats, LAYER-major: layer l occupies [B*soff_l, B*(soff_l+I_l)) as a contiguous [B, I_l] matrix;
 *   demod  : demod_rows * B floats, same scheme with doff_l / O_l.  All tables are caller-owned and only read during the call.
 */
int ia_styles_demod(const float* ws, int B, int num_ws, int w_dim, const int64_t* layer_table, const float* layer_gains,
                    const int* style_row_layer, int style_rows, const int* demod_row_layer, int demod_rows,
                    float* styles, float* demod, void* stream);

/*
 * Camera labels -> ray bundles.  Replaces RaySampler_zxc.forward
 * (training_avatar_texture/volumetric_rendering/ray_sampler.py:70-107).
 *   cam : [B, cam_stride] float32, each row = 16 floats cam2world (row-major 4x4) followed by 9 floats intrinsics (row-major 3x3,
 *         normalised by image size) -- i.e. the last 25 entries of the reference's conditioning label `c`
 *   rays_o, rays_d : [B, resolution^2, 3] float32, pixel order row-major (y, x), integer pixel centres (no +0.5)
 */
int ia_ray_sampler(const float* cam, int cam_stride, float* rays_o, float* rays_d, int B, int resolution, int normalize, void* stream);

/*
 * Activations as fp16 hi/lo pairs ("split format"), the input of ia_conv2d_mfma_sx:
 *     xs[b][plane][c/8][y][x][c%8]   fp16, plane 0 = hi = fp16(v), plane 1 = lo = fp16((v - hi) * 2^11),  v = x[b,c,y,x] * styles[b,c]
 * (v saturates at +-65504; |v| < 2^-14 rides entirely in the low plane: the MFMA flushes fp16 denormals).  4 bytes per element,
 * the size of the fp32 tensor; hi + lo * 2^-11 carries 22 mantissa bits.  C % 8 == 0.  styles [B,C] or NULL (= 1).
 * ia_act_split is the stand-alone producer; ia_fir_tail_split and ia_conv2d_mfma_sx emit the format from their epilogues.
 * planes = 2 is the format above; planes = 1 keeps plane 0 only, rounded once (hi = fp16(v), saturating): the operand format of the
 * fp16 blocks (ia_conv2d_mfma_h arithmetic) and the fp16-STORAGE form of their activations, xs[b][c/8][y][x][c%8], 2 bytes / element.
 * shift [B,C] or NULL: v = x * styles + shift -- an eval-mode BatchNorm folded into the staging of the convolution that follows it
 * (inversion encoders, encoder_inversion/models/helpers.py:102-124: BatchNorm2d -> Conv2d 3x3; the zero padding then applies to
 * the normalised tensor, as in the reference).
 */
int ia_act_split(const float* x, const float* styles, const float* shift, void* xs, int planes, int B, int C, int H, int W, void* stream);

/*
 * torch.nn.BatchNorm2d in TRAIN mode followed by ia_act_split, in two launches: xs = split((x - mean_c) * weight_c / sqrt(var_c + eps) +
 * bias_c) with mean / biased variance over (B, H, W) per channel, and the running-statistics update of a train-mode call
 * (running = running + momentum * (batch - running), unbiased variance; num_batches_tracked += 1).  The inversion encoders run the
 * BatchNorms of the e4e trunk and of the decoders' DoubleConv on batch statistics at evaluation time (the reference's eval_seq.py:91-97
 * leaves those modules in train()): encoder_inversion/models/helpers.py:102-124 (BatchNorm2d -> Conv2d 3x3), unet_encoders.py:52-66.
 *   weight, bias [C] or NULL (1 / 0); running_mean, running_var [C] or both NULL; num_batches_tracked: device int64 or NULL;
 *   partials: caller-owned scratch of C * chunks * 2 doubles; chunks = partial sums per channel (1 .. 1024: enough workgroups for
 *   pass 1, e.g. ceil(B*H*W / 8192)); xs, planes as ia_act_split.  C % 8 == 0, B*H*W > 1.
 */
int ia_bn_train_split(const float* x, const float* weight, const float* bias, float* running_mean, float* running_var,
                      long long* num_batches_tracked, double* partials, int chunks, void* xs, int planes, int B, int C, int H, int W,
                      float eps, float momentum, void* stream);

/* 1 for the layer shapes ia_conv2d_mfma_sx covers (3x3, I % 8 == 0, O % 8 == 0, from 8^2; stride-1 layers need O >= 128, W <= 512). */
int ia_conv2d_sx_supported(int I, int O, int H, int W, int ksize, int transposed);

/*
 * ia_conv2d_mfma_s on split-format activations: same layer semantics, tiles, ksplit / scratch (ia_conv2d_plan with form = 3) and
 * results of the same arithmetic (the same products; since r03 the stride-1 kernels pair the odd tap of a chunk with the next chunk's
 * instead of an all-zero tap, so the fp32 sums are added in another order: equal to summation-order level, 2e-6 of a layer's magnitude), but the operand split was done by the producer and both operands reach LDS by DMA
 * (buffer_load ... lds) instead of through registers.  Replaces the same reference chain as ia_conv2d_mfma
 * (training/networks_stylegan2.py:34-91, conv2d_resample.py:114-136) for the 3x3 layers of >= 32^2 (I % 8 == 0, O % 8 == 0).
 *   xs, planes  : input in split format, already multiplied by THIS layer's styles (there is no `styles` argument); planes = 2 with
 *                 wk_split from pack_conv_weight_split (three fp16 products per fp32 product: ia_conv2d_mfma_s arithmetic), planes = 1
 *                 with the one-plane fp16 weights [tap][I/8][O][8] and wk_exp = 0 (fp16 operands: ia_conv2d_mfma_h arithmetic)
 *   y           : [B,O,OH,OW] fp32 or NULL (stride-1 form only: a layer whose result is consumed only in split format)
 *   ys, ys_planes : the result in split format (ys_planes planes), multiplied by styles_next [B,O] (the styles of the consuming layer; NULL = 1), or
 *                 NULL; stride-1 form only (the transposed form's (2H+1)^2 image goes through ia_fir_tail_split)
  * prelu_alpha : NULL, or [O] per-output-channel negative slopes used by IA_ACT_LRELU in place of `alpha` (torch.nn.PReLU of the
 *               inversion encoders' residual units, helpers.py:105).  With demod = BatchNorm scale and bias = BatchNorm shift (per output
 *               channel) the epilogue is conv -> BatchNorm(eval) -> PReLU of those networks; styles / noise stay NULL.
 */
int ia_conv2d_mfma_sx(const void* xs, int planes, const void* wk_split, int wk_exp, const float* demod, const float* noise,
                      const float* noise_strength, const float* bias, const float* residual, float* y, void* ys, int ys_planes,
                      const float* styles_next, float* scratch, size_t scratch_bytes, int B, int I, int O, int H, int W,
                      int transposed, int act, float alpha, const float* prelu_alpha, float gain, float clamp, int ksplit, void* stream);

/*
 * y = bilinear resize of x [planes, H, W] to [planes, OH, OW] with align_corners = True (torch.nn.functional.interpolate's arithmetic)
 * + addend [planes, OH, OW] (NULL: the resize alone).  Replaces `_upsample_add` of the e4e feature pyramid
 * (encoder_inversion/models/e4e.py:48-65): F.interpolate(x, size=y.shape, mode='bilinear', align_corners=True) + y.
 */
int ia_upsample_bilinear_add(const float* x, const float* addend, float* y, int planes, int H, int W, int OH, int OW, void* stream);

/*
 * Depth-wise 3x3 convolution (stride 1, padding 1) of a Mix-FFN on the token grid, channels-last: y[b, n, c] = bias[c] + sum_k
 * w9c[k][c] * x[b, n + offset_k, c] over the H x W grid of tokens n, optionally followed by GELU (erf form).  Replaces DWConv.forward of
 * the transformer-refined decoders of the one-shot encoders (encoder_inversion/models/mmseg/mix_transformer.py:49-58: transpose -> view
 * -> nn.Conv2d(groups = C) -> flatten -> transpose) and the activation after it (:70-77).
 *   x, y [B, H*W, C] float32; w9c [9][C]: the module's weight [C, 1, 3, 3] transposed; bias [C] or NULL; act 0 = none, 1 = GELU.  C % 4 == 0.
 */
int ia_dwconv3x3_tokens(const float* x, const float* w9c, const float* bias, float* y, int B, int H, int W, int C, int act, void* stream);
/* The same convolution (+ GELU) with its result written as the operand of the linear layer behind it (Mix-FFN: dwconv -> GELU -> fc2):
 * xs fp16 [2][C/8][B*H*W][8], ia_tokens_split's format (one launch for both).  C % 16 == 0. */
int ia_dwconv3x3_tokens_split(const float* x, const float* w9c, const float* bias, void* xs, int B, int H, int W, int C, int act, void* stream);

/*
 * 3x3 convolution with stride 2 and padding 1 on an image of 2^2, 4^2 or 8^2 pixels (outputs 1^2, 2^2, 4^2): the last layers of a
 * GradualStyleBlock of the e4e encoder (encoder_inversion/models/e4e.py:22-45: Conv2d(512, 512, 3, 2, 1) + LeakyReLU down to 1x1), cuDNN
 * through torch.nn.Conv2d in the reference.  A matrix-vector product that streams the weight once; fp32 FMAs, deterministic.
 *   x [B,I,H,W], w [O,I,3,3] (the module's own layout), bias [O] or NULL, y [B,O,H/2,W/2]; act IA_ACT_LINEAR or IA_ACT_LRELU (alpha).
 * H == W in {2, 4, 8} and I * (H*W + 1) * 4 bytes <= 160 KB (ia_conv3x3_s2_tiny_supported = 1), else IA_ERR_UNSUPPORTED.
 */
int ia_conv3x3_s2_tiny_supported(int I, int O, int H, int W);
int ia_conv3x3_s2_tiny(const float* x, const float* w, const float* bias, float* y, int B, int I, int O, int H, int W, int act, float alpha,
                       void* stream);

/*
 * 3x3 convolution with STRIDE 2 and padding 1 on split-format activations: y[b,o,r,c] = sum w[o,i,ky,kx] * x[b,i,2r+ky-1,2c+kx-1], on
 * the stride-1 tile families of ia_conv2d_mfma_sx with the point grid laid over every second pixel of the input window (same
 * products as torch.nn.functional.conv2d(stride 2, padding 1): a quarter of the stride-1 layer's).  Replaces the stride-2 layers of
 * the inversion encoders (encoder_inversion/models/helpers.py:102-124, second convolution of the first residual unit of a stage;
 * e4e.py:22-45, GradualStyleBlock), which the reference hands to cuDNN through torch.nn.Conv2d.
 *   xs [B][planes][I/8][H][W][8], wk_split, wk_exp, demod, bias, residual, y, ys, ys_planes, styles_next, act, alpha, prelu_alpha, gain,
 *   clamp: as ia_conv2d_mfma_sx; y / ys / residual have the output size ((H-1)/2+1) x ((W-1)/2+1).
 *   ksplit, scratch: from ia_conv2d_down_plan (same stream-K slabs as ia_conv2d_plan).
 * I % 8 == 0, O % 8 == 0, O >= 64, outputs from 8^2 up, input windows that fit the LDS stages (W <= ~1000); else IA_ERR_UNSUPPORTED
 * from ia_conv2d_down_plan (callers evaluate the layer at stride 1 and sub-sample, or use the library).
 */
int ia_conv2d_down_plan(int B, int I, int O, int H, int W, int* h_ksplit, size_t* h_scratch_bytes);
int ia_conv2d_down_sx(const void* xs, int planes, const void* wk_split, int wk_exp, const float* demod, const float* bias, const float* residual,
                      float* y, void* ys, int ys_planes, const float* styles_next, float* scratch, size_t scratch_bytes, int B, int I, int O,
                      int H, int W, int act, float alpha, const float* prelu_alpha, float gain, float clamp, int ksplit, void* stream);

/*
 * ia_upfirdn2d_bias_act for the 4x4 filter at up = 1 (the FIR + noise + bias + activation tail of an up-sampling SynthesisLayer,
 * training/networks_stylegan2.py:318-329 after conv2d_resample.py:114-131) with the result stored in SPLIT format for the next
 * convolution: ys = split(tail(fir(x)) * styles_next[b, c]) (see ia_act_split; same FIR sums in the same order as
 * ia_upfirdn2d_bias_act).  y (fp32 [n,c,out_h,out_w]) may be NULL when only the split result is consumed.  c % 8 == 0.
 */
int ia_fir_tail_split(const float* x, const float* f, const float* noise, const float* noise_strength, const float* bias,
                      const float* styles_next, float* y, void* ys, int ys_planes, int n, int c, int in_h, int in_w, int out_h, int out_w,
                      int padx0, int pady0, int flip, float fir_gain, int act, float alpha, float act_gain, float clamp, void* stream);

/*
 * ia_conv2d_mfma_sx (stride 1) with the ToRGB layer that consumes its result evaluated in the epilogue: the last block of the SR head
 * (SynthesisBlock.forward, training/networks_stylegan2.py:448-457: conv1, then torgb(x) added to the up-sampled image) reads its
 * 128 x 512^2 activation only through ToRGB, so neither that tensor nor its re-read has to exist.
 *   rgb_out[b,c] = clamp( sum_o (rgb_wk[o,c] * rgb_styles[b,o]) * v[b,o] + rgb_bias[c], rgb_clamp ) + rgb_residual[b,c]
 * with v the layer's own result (after noise / bias / activation / clamp).  rgb_wk [O, rgb_channels] is ia_conv2d_mfma's ksize-1
 * packing of the ToRGB weight (weight_gain folded in), rgb_channels <= 3.  y and ys may both be NULL.  The layer must run in whole
 * rounds of tiles that hold every output channel (O <= 128 at the sizes the planner gives the 128 x 256 tile), else
 * IA_ERR_UNSUPPORTED (callers use ia_conv2d_mfma_sx + ia_conv1x1).  Other arguments as ia_conv2d_mfma_sx.
 */
int ia_conv2d_mfma_sx_rgb(const void* xs, int planes, const void* wk_split, int wk_exp, const float* demod, const float* noise,
                          const float* noise_strength, const float* bias, float* y, void* ys, int ys_planes, const float* styles_next,
                          const float* rgb_wk, const float* rgb_styles, const float* rgb_bias, const float* rgb_residual, float* rgb_out,
                          int rgb_channels, float rgb_clamp, int B, int I, int O, int H, int W, int act, float alpha, float gain, float clamp,
                          void* stream);

/*
 * The stride-2 transposed 3x3 convolution of an up-sampling SynthesisLayer (torch_utils/ops/conv2d_resample.py:114-131 ->
 * conv_transpose2d; training/networks_stylegan2.py:296-305) on split-format activations, evaluated per output ROW phase on the
 * stride-1 tile (128 channels x 256 / 128 points, two accumulator sets = the two column phases): the same products as
 * ia_conv2d_mfma_sx(transposed = 1) -- 9 per input pixel and channel pair, the minimum -- and the same result image
 *   y [B, O, 2H+1, 2W+1] float32 = demod[b][o] * conv_transpose2d(x * styles, w, stride 2)   (summation order differs),
 * which ia_fir_tail_split / ia_upfirdn2d_bias_act turn into the layer's output.  (csrc/conv_up.hip)
 *   xs       : activations as ia_act_split(planes = 2) stores them, already multiplied by this layer's styles
 *   wk_split : the weights of pack_conv_weight_split ([2][9][I/8][O][8] fp16 of w * 2^wk_exp), the ones ia_conv2d_mfma_sx takes
 *   scratch  : ia_upconv2d_rows_plan's byte count (partial sums of the thin edge grids: bottom row / last column of the image)
 * Needs I % 16 == 0, O % 128 == 0, 16 <= H, W <= 1024: ia_upconv2d_rows_plan returns IA_ERR_UNSUPPORTED otherwise.
 */
int ia_upconv2d_rows_plan(int B, int I, int O, int H, int W, size_t* h_scratch_bytes);
int ia_upconv2d_rows_sx(const void* xs, const void* wk_split, int wk_exp, const float* demod, float* y, float* scratch,
                        size_t scratch_bytes, int B, int I, int O, int H, int W, void* stream);

/*
 * An up-sampling SynthesisLayer with FEW input channels as ONE stride-1 launch: the transposed convolution (stride 2) and the 4x4
 * resample FIR that follows it are linear, so their composition is, per output phase (py, px), a 3x3 convolution of the INPUT image
 * with the weights  W'[py,px][dy,dx] = gain * sum_{i,ky: py+i-1-ky = 2dy} sum_{j,kx: px+j-1-kx = 2dx} F[i,j] * w[ky,kx]  (F the
 * flipped filter).  The layer then is a stride-1 convolution with 4 x O output channels -- row ((py * O/32 + o/32) * 2 + px) * 32 +
 * o % 32, so that a wave holds both horizontal phases of its channels -- whose epilogue stores point (r, c) of phase (py, px) at
 * pixel (2r + py, 2c + px): four times the products, but no (2H+1) x (2W+1) fp32 image, no FIR launch
 * and no stream-K tail -- a win when the K loop is short (the 32 -> 256 @128^2 layer of the SR head: 2.4 GFLOP that moved 200 MB).
 * Replaces modulated_conv2d(up=2) -> conv2d_resample (conv_transpose2d, stride 2) -> upfirdn2d(pad [1,1,1,1], gain 4) -> noise ->
 * bias_act of SynthesisLayer.forward (training/networks_stylegan2.py:296-305, torch_utils/ops/conv2d_resample.py:114-131) for such
 * layers; results agree with the two-launch route to fp32 rounding (the same sums in another association).
 *   xs        : split input [B, planes, I/8, H, W, 8], already multiplied by the layer's styles (ia_act_split)
 *   wk_split  : pack_conv_weight_split / _h layout of the COMPOSED weight [4*O, I, 3, 3] (row order above), wk_exp its exponent
 *   demod [B,O], noise [2H*2W], noise_strength, bias [O], styles_next [B,O]: per REAL channel / OUTPUT pixel, any may be NULL
 *   y [B,O,2H,2W] fp32 and / or ys [B, ys_planes, O/8, 2H, 2W, 8] split (at least one)
 * O % 32 == 0 and the 4*O-channel layer must run in whole 128-channel tiles (ia_conv2d_plan(B, I, 4*O, H, W, 3, 0, 3) gives 0
 * workers, at least one such tile per CU); else IA_ERR_UNSUPPORTED (callers use ia_conv2d_mfma_sx(transposed) + ia_fir_tail_split).
 */
int ia_upconv2d_fir_sx(const void* xs, int planes, const void* wk_split, int wk_exp, const float* demod, const float* noise,
                       const float* noise_strength, const float* bias, float* y, void* ys, int ys_planes, const float* styles_next,
                       int B, int I, int O, int H, int W, int act, float alpha, float gain, float clamp, void* stream);

/*
 * ToRGB layer as a streaming kernel: y = clamp((w * styles) (*) x + bias) + residual for a 1x1 modulated convolution without
 * demodulation.  Replaces ToRGBLayer.forward (training/networks_stylegan2.py:353-362: modulated_conv2d(demodulate=False) :34-91 +
 * bias_act(clamp) ) and the skip-image add of SynthesisBlock.forward (:457).  x [B,I,H,W], wk [I,O] (ia_conv2d_mfma's packing
 * for ksize 1, weight_gain folded in), styles [B,I] or NULL, bias [O] or NULL, residual [B,O,H,W] or NULL (added after the
 * clamp), y [B,O,H,W]; clamp < 0 = none.  O <= 96, I % 32 == 0, H*W % 4 == 0, else IA_ERR_UNSUPPORTED (callers use
 * ia_conv2d_mfma).  One launch, no scratch.
 */
int ia_conv1x1(const float* x, const float* wk, const float* styles, const float* bias, const float* residual, float* y,
               int B, int I, int O, int H, int W, float clamp, void* stream);

/*
 * ToRGB layer AND the skip-image branch of its block in one launch:
 *   y = clamp((w * styles) (*) x + bias) + (residual | upsample2d(skip))
 * Replaces ToRGBLayer.forward (training/networks_stylegan2.py:353-362) + `img = upfirdn2d.upsample2d(img, resample_filter)` +
 * `img = img.add_(y)` of SynthesisBlock.forward (:454-457; upsample2d = torch_utils/ops/upfirdn2d.py:315-350: zero insertion x2,
 * padding [2,1,2,1], the 4x4 filter, gain 4).  Same arguments as ia_conv1x1, plus skip [B,O,H/2,W/2] (or NULL) with its resample
 * filter skip_filter [4,4] (upfirdn2d.setup_filter([1,3,3,1])); residual and skip are exclusive.  Every load of a wave (128 input
 * channels x 32 pixels, its weights and styles) is in flight before the first MFMA, wider layers split their channels over the waves
 * of a workgroup; the up-sampling evaluates the 2 x 2 non-zero taps per output pixel in ia_upfirdn2d's order (bit-identical image).
 * C_in in {128, 256, 512, 1024}, C_out <= 96, H and W even when skip is given; else IA_ERR_UNSUPPORTED (callers use ia_conv1x1 +
 * ia_upfirdn2d).  ia_torgb_supported answers that question without a launch (1 = covered).  One launch, no scratch.
 */
int ia_torgb_supported(int I, int O, int H, int W, int with_skip);
int ia_torgb(const float* x, const float* wk, const float* styles, const float* bias, const float* residual, const float* skip,
             const float* skip_filter, float* y, int B, int I, int O, int H, int W, float clamp, void* stream);

/*
 * ia_cond_blend with the result in SPLIT format (ia_act_split) for the one layer that consumes it, multiplied by that layer's
 * styles [B,C] (NULL = 1): ys = split((cond[:, :C] * a + x * (1 - a)) * styles_next), a = cond[:, C]
 * (training_avatar_texture/networks_stylegan2_new.py:539-540 feeding the next block's conv0).  C % 8 == 0.
 */
int ia_cond_blend_split(const float* cond, const float* x, const float* styles_next, void* ys, int B, int C, int H, int W, void* stream);

/*
 * Fused filtered leaky ReLU: bias -> up-sample (zero insert, pad/crop, up-FIR x up^2) -> lrelu(slope) x gain -> clamp -> down-FIR ->
 * decimate, the up-sampled intermediate kept in LDS.
 * Replaces filtered_lrelu_plugin.filtered_lrelu(x, fu, fd, b, si, up, down, px0, px1, py0, py1, sx, sy, gain, slope, clamp,
 * flip_filter, writeSigns) -> (y, so, rc) (torch_utils/ops/filtered_lrelu.cpp:20-22,217; kernels filtered_lrelu.cu:144-1103) for
 * the forward pass without sign tensors (si = None, writeSigns = false: what inference calls); semantics = the reference's own
 * definition of the op, _filtered_lrelu_ref (filtered_lrelu.py:123-155).
 *   x, y   : [n, c, in_h, in_w] / [n, c, out_h, out_w] contiguous NCHW of `dtype` (IA_F32 or IA_F16; f64 -> IA_ERR_UNSUPPORTED,
 *            the caller composes bias_act + upfirdn2d, as the reference does when its plugin returns rc = -1, :225-231)
 *   fu, fd : 2-D float32 filters [fu_h, fu_w] / [fd_h, fd_w], contiguous (separable filters are passed as their outer product),
 *            or NULL with size 1x1 for identity
 *   b      : [c] of `dtype` or NULL
 *   out size must equal (in*up + pad0 + pad1 - (fu - 1) - (fd - 1) + (down - 1)) / down per axis (filtered_lrelu.py:142-143)
 *   clamp < 0 : disabled
 */
int ia_filtered_lrelu(const void* x, const float* fu, const float* fd, const void* b, void* y, int dtype,
                      int n, int c, int in_h, int in_w, int out_h, int out_w, int fu_h, int fu_w, int fd_h, int fd_w,
                      int up, int down, int px0, int px1, int py0, int py1, float gain, float slope, float clamp,
                      int flip_filter, void* stream);

/*
 * ConvGRU cell of the inversion encoder's recurrent up-path (encoder_inversion/models/unet_encoders.py:8-49): the element-wise
 * work around its two convolutions, which stay library convolutions on the caller's side.
 *   ia_convgru_gates : xrh = cat[x, sigmoid(gates_pre[:, :C]) * h]                  ([B,2C,H,W]; the input of conv_hh, :26-27)
 *   ia_convgru_update: z = sigmoid(gates_pre[:, C:]); c = tanh(cand_pre) (PReLU with prelu_weight[C] when non-NULL, :19-20);
 *                      h_out = (1 - z) * h + z * c (:28); with x_next / xh_next also xh_next = cat[x_next, h_out], the input of
 *                      conv_ih of the next time step (:25)
 * gates_pre = conv_ih(cat[x, h]) + bias [B,2C,H,W]; cand_pre = conv_hh(xrh) + bias [B,C,H,W]; all fp32 contiguous, H*W % 4 == 0.
 */
int ia_convgru_gates(const float* gates_pre, const float* x, const float* h, float* xrh, int B, int C, int H, int W, void* stream);
int ia_convgru_update(const float* gates_pre, const float* cand_pre, const float* h, const float* prelu_weight, float* h_out,
                      const float* x_next, float* xh_next, int B, int C, int H, int W, void* stream);

/*
 * ia_convgru_gates / ia_convgru_update with the convolution inputs they produce written in SPLIT format (ia_act_split, two planes):
 * xrh_split = split(cat[x, sigmoid(r_pre) * h]) and xh_next_split = split(cat[x_next, h']) are read by the cell's two
 * ia_conv2d_mfma_sx launches only, so neither their fp32 copies nor the two ia_act_split launches of a step exist.  h_out stays fp32
 * (the cell's output and the next step's state).  Same arithmetic as the fp32 forms.  C % 8 == 0, H * W % 4 == 0.
 */
int ia_convgru_gates_split(const float* gates_pre, const float* x, const float* h, void* xrh_split, int B, int C, int H, int W, void* stream);
int ia_convgru_update_split(const float* gates_pre, const float* cand_pre, const float* h, const float* prelu_weight, float* h_out,
                            const float* x_next, void* xh_next_split, int B, int C, int H, int W, void* stream);

/*
 * Squeeze-and-excitation gate + residual add of an IR-SE50 unit:  out = v * sigmoid(W2 relu(W1 mean_hw(v))) + shortcut.
 * Replaces SEModule.forward and the add of bottleneck_IR_SE.forward (encoder_inversion/models/helpers.py:84-100, :121-124).
 *   v, shortcut : float32 [B, C, H, W] VIEWS given by 4 strides each (floats; batch, channel, row, column) -- the stride-2 output of
 *                 the unit's second convolution and MaxPool2d(1, s) shortcuts are strided views of larger tensors
 *   w1 [R, C], w2 [C, R] : the two bias-free 1x1 convolutions (R = C / reduction <= 64);  pooled_scratch : B * C floats
 *   out : [B, C, H, W] contiguous
 */
int ia_se_gate(const float* v, const int64_t* v_strides, const float* shortcut, const int64_t* shortcut_strides, const float* w1,
               const float* w2, float* pooled_scratch, float* out, int B, int C, int R, int H, int W, void* stream);

/*
 * ia_se_gate with the result ALSO in split format for the convolution that consumes it: ys = split(out * next_scale[b][c] +
 * next_shift[b][c]) (ia_act_split's two-plane format; the eval-mode BatchNorm in front of the next residual unit's first convolution,
 * helpers.py:102-124), or ys = next_scale = next_shift = NULL for the fp32 result alone.  C % 8 == 0.  Same arithmetic as ia_se_gate.
 */
int ia_se_gate_split(const float* v, const int64_t* v_strides, const float* shortcut, const int64_t* shortcut_strides, const float* w1,
                     const float* w2, float* pooled_scratch, float* out, const float* next_scale, const float* next_shift, void* ys,
                     int B, int C, int R, int H, int W, void* stream);

/*
 * Multi-head self-attention in one launch: out = softmax(Q K^T * scale) V per (batch, head), without the [N, M] score matrix.
 * Replaces Attention.forward of the transformer-refined UNet decoders between the projections
 * (encoder_inversion/models/mmseg/mix_transformer.py:83-116 with sr_ratio 1: two batched matmuls, the softmax over [N, M] and
 * the head permutes).  fp32 operands and accumulation (v_mfma_f32_32x32x2_f32), online softmax, fixed summation order.
 *   q   : [B, N, heads * head_dim] float32 (the output of the q projection; head h = columns [h * head_dim, (h + 1) * head_dim))
 *   k, v: [B, M, heads * head_dim] views with their own batch / row strides (the reference's fused kv projection is [B, M, 2 C]:
 *         k = columns [0, C), v = columns [C, 2 C), row stride 2 C)
 *   out : [B, N, heads * head_dim] float32 = (attn @ v).transpose(1, 2).reshape(B, N, C) of the reference
 *   strides in floats, multiples of 4; head_dim must be 256 (the 1024-dim / 4-head blocks) and N * M <= 131072 (the 8^2 / 16^2 token
 *   grids of the first two decoder stages, where the ATen sequence is launch-bound: 21 vs 66 us, 65 vs 139 us; beyond that the
 *   library GEMMs are faster and the caller keeps them): others -> IA_ERR_UNSUPPORTED (ia_attention_supported tells)
 */
int ia_attention_supported(int head_dim, int N, int M);
int ia_attention(const float* q, const float* k, const float* v, float* out, int B, int heads, int N, int M, int head_dim,
                 int64_t q_batch_stride, int64_t q_row_stride, int64_t k_batch_stride, int64_t k_row_stride,
                 int64_t v_batch_stride, int64_t v_row_stride, int64_t out_batch_stride, int64_t out_row_stride,
                 float scale, void* stream);

/*
 * Token-major linear layers of the transformer blocks (encoder_inversion/models/mmseg/mix_transformer.py:18-116: Mlp.fc1 / fc2,
 * Attention.q / kv / proj -- nn.Linear on [B, tokens, C]; :158-190 the blocks that chain them) as fp32-equivalent GEMMs on the fp16
 * pipe: fp32 products from fp16 hi / lo pairs like the 3x3 convolutions (three v_mfma_f32_32x32x16_f16 per k-step, fp32
 * accumulation, lo x lo ~ 2^-22 dropped).  Replaces F.linear (rocBLAS fp32 GEMM) + bias [+ GELU] [+ the residual add of Block.forward].
 *   ia_tokens_split: x [M][K] float32 (M = B * tokens; rows `ld` floats apart, ld = K for a dense matrix) -> xs fp16 [2][K/8][M][8]: hi = fp16(v),
 *       lo = fp16((v - hi) * 2^11) -- the split format of the convolutions with the token in the pixel's place.  One call serves
 *       every linear layer that reads x (q and kv; fc1).  |v| >= 65504 saturates and raises the range-watch word
 *       (ia_split_saturation_poll).  K % 16 == 0, ld % 4 == 0, x 16-byte aligned, else IA_ERR_UNSUPPORTED.
 *   ia_linear_sx: y [M][N] float32 = act(xs . w^T * 2^-wk_exp + bias) + residual
 *       w_split : fp16 [2][1][K/8][N][8], the nn.Linear weight [N][K] as a 1x1 kernel in the convolution weight format
 *                 (hi = fp16(w * 2^wk_exp), lo = fp16(w * 2^wk_exp - hi); the host-side packing of ia_conv2d_mfma_s)
 *       bias    : [N] or NULL;  residual: [M][N] or NULL, added after the activation (x + drop_path(f(x)) of Block.forward)
 *       act     : 0 none, 1 GELU (erf form, nn.GELU default)
 *       deterministic (fixed summation order for a given shape); no workspace.
 */
int ia_tokens_split(const float* x, int64_t ld, void* xs, int M, int K, void* stream);
/*
 * nn.LayerNorm over the last dimension + ia_tokens_split of its result in one launch (Block.forward, mix_transformer.py:140-142: norm1
 * feeds only q / kv, norm2 only fc1): xs = split((x - mean) * rsqrt(var + eps) * gamma + beta), biased variance, two passes in fp32.
 * x [M][K] float32 dense; K 512, 1024 or 2048; gamma, beta [K].
 */
int ia_layernorm_split(const float* x, const float* gamma, const float* beta, float eps, void* xs, int M, int K, void* stream);
/*
 * The overlapping patch embeddings of the same encoders (mix_transformer.py:155-190 OverlapPatchEmbed: a 7x7 stride-2 / stride-4
 * convolution whose output is flattened to tokens) as im2col-free GEMMs: ia_im2col_split writes the patches of an NCHW float32 image
 * straight into the split format of a token matrix -- row m = (b, oy, ox), column k = (c, ky, kx) in the order of
 * conv.weight.reshape(N, C * ksize * ksize), zero columns up to Kp = K rounded up to 16 -- and ia_linear_sx (M = B * OH * OW, K = Kp,
 * weight rows zero-padded the same way) produces the tokens [B, OH * OW, N] + bias directly: no NCHW result, no flatten / transpose.
 *   xs: fp16 [2][Kp/8][M][8];  ksize 7 or 3, zero padding;  OH = (H + 2 pad - ksize) / stride + 1.
 */
int ia_im2col_split(const float* x, void* xs, int B, int C, int H, int W, int ksize, int stride, int pad, void* stream);
/*
 * The same product with K cut into `ksplit` slices over the launch (few rows, very long K: the deepest patch embedding is 64 tokens x
 * 50 176 x 1 024): slice products into scratch [ksplit][M][N], then one pass sums them in slice order and adds the bias.
 * ia_linear_splitk_plan gives the split the library would choose (1 = none) and the scratch it needs; K % (16 * ksplit) == 0.
 */
int ia_linear_splitk_plan(int M, int K, int N, int* ksplit, size_t* scratch_bytes);
int ia_linear_sx_splitk(const void* xs, const void* w_split, int wk_exp, const float* bias, float* y, int M, int K, int N, int ksplit,
                        float* scratch, size_t scratch_bytes, void* stream);
int ia_linear_sx(const void* xs, const void* w_split, int wk_exp, const float* bias, const float* residual, float* y, int M, int K, int N,
                 int act, void* stream);

/*
 * Attention of the same blocks on token grids too large for ia_attention (32^2 / 64^2 tokens: Attention.forward,
 * mix_transformer.py:83-116 -- q @ k^T * scale, softmax, attn @ v as two batched rocBLAS GEMMs, an elementwise scale, a softmax over
 * [heads, N, M] and the head permutes) as three launches on the fp16-pair GEMM, the score matrix in HBM once:
 *   S[z] = scale * Q[z] K[z]^T   (ia_matmul_sx on ia_tokens_split(q), ia_tokens_split(k): head z = columns [z * hd, (z + 1) * hd))
 *   P = softmax(S) written as the next product's operand  (ia_softmax_split)
 *   O[:, z * hd : (z + 1) * hd] = P[z] V[z]   (ia_matmul_sx on P and ia_tokens_split_t(v)), straight into the [N, C] token layout.
 * ia_tokens_split_t: v [M keys][ld] float32, C columns -> vt fp16 [2][M/8][C][8], octets ALONG THE KEYS (M % 16 == 0); perm = 1: the keys of
 *   a 16-key step in the row order of the 32 x 32 MFMA accumulator (octet 2t + h = keys 16t + {0..3, 8..11} + 4h), the order ia_attention_sx reads.
 * ia_softmax_split: s [Z][N][M] float32 -> ps fp16 [2][Z][M/8][N][8]; M % 16 == 0, M <= 4096.
 * ia_matmul_sx: y[z][m][n] = scale * sum_k a[z][m][k] b[z][n][k] for z < batch, both operands token-side splits (low parts at 2^11):
 *   a_rows / b_rows      : rows of the split tensors the operands live in (their octet stride is rows * 16 bytes)
 *   a_plane / b_plane    : bytes from the hi plane to the lo plane;  a_batch / b_batch: bytes per z inside a plane
 *                          (head z of [2][C/8][rows][8]: z * (hd / 8) * rows * 16;  P: (M / 8) * N * 16;  vt: z * hd * 16)
 *   y_batch_stride / y_row_stride in floats.  K % 16 == 0.  Deterministic; no workspace.
 */
int ia_tokens_split_t(const float* v, int64_t ld, void* vt, int M, int C, int perm, void* stream);
int ia_softmax_split(const float* s, void* ps, int Z, int N, int M, void* stream);
/*
 * The same attention in ONE launch, the score matrix never in memory (head_dim 256): a first pass over the keys finds every query's maximum,
 * a second one forms exp(s - max), its sum and the output over 32-key blocks; both products on fp16 pairs.  A wave computes S^T = K Q^T so that a query's keys sit in the registers of two lanes (row maximum / sum are register
 * reductions + one exchange) and its probabilities are, as they stand, a B fragment of O^T = V^T P^T -- no transposition anywhere.
 *   q_split = ia_tokens_split(q [N][C]), k_split = ia_tokens_split(k [M][C]), v_split_t = ia_tokens_split_t(v [M][C], perm = 1);
 *   out [N][C] float32 = (attn @ v).transpose(1, 2).reshape(N, C) of the reference; M % 16 == 0; deterministic.
 */
int ia_attention_sx_supported(int head_dim, int N, int M);
int ia_attention_sx(const void* q_split, const void* k_split, const void* v_split_t, float* out, int heads, int N, int M, int head_dim,
                    float scale, void* stream);
int ia_matmul_sx(const void* a_split, const void* b_split, float* y, int batch, int M, int N, int K, int a_rows, int64_t a_plane_bytes,
                 int64_t a_batch_bytes, int b_rows, int64_t b_plane_bytes, int64_t b_batch_bytes, int64_t y_batch_stride, int64_t y_row_stride,
                 float scale, void* stream);

/*
 * Driver-side UV rasteriser: projected FaceVerse mesh -> uvcoords_image, the mesh condition of TriPlaneGenerator.synthesis.
 * Replaces Faceverse_manager.make_driven_rendering from the rasteriser call on (data_preprocess/FaceVerse/renderer.py:66-82:
 * pytorch3d MeshRasterizer, ortho camera K = [-1,-1,0,0], T = [0,0,10], faces_per_pixel 1 -> render_after_rasterize
 * (volumetric_rendering/renderer.py:556-571) -> x (vis * mask) -> crop -> HWC (u, v, mask >= 0.5)).
 *   verts          : [B, V, 3] float32, the vertices handed to Meshes() (after batch_orth_proj and the z flip, :62-64)
 *   tris           : [F, 3] int32
 *   face_attrs     : [F, 3, 3] float32 = face_vertices(cat[uv * 2 - 1, mask], tris): (u, v, mask) of every corner (:33-34)
 *   zbuf_scratch   : B * crop_w * crop_h * 8 bytes (caller-owned)
 *   uvcoords_image : [B, crop_h, crop_w, 3] float32
 *   binarize_mask  : 1 = channel 2 is (mask >= 0.5) as the script returns it at the native size (:82); 0 = the continuous
 *                    mask * vis * mask product, for a caller that interpolates to another `res` first and thresholds afterwards (:78-82)
 *   raster_size 512, crop (128, 114, 256, 256), blur_radius 1e-6 in the reference (:13-14, :43)
 */
int ia_uv_rasterize(const float* verts, const int* tris, const float* face_attrs, void* zbuf_scratch, float* uvcoords_image,
                    int B, int V, int F, int raster_size, int crop_left, int crop_top, int crop_w, int crop_h, float blur_radius,
                    int binarize_mask, void* stream);

/*
 * Output side: float image batch -> uint8 picture grid, one pass.
 * Replaces layout_grid(img, grid_w, grid_h, float_to_uint8=True, chw_to_hwc) of the reference's scripts
 * (reenact_avatar_next3d.py:117-131): (img * 127.5 + 128).clamp(0, 255).to(uint8), frames tiled row-major into a
 * grid_h x grid_w mosaic, channels moved last when chw_to_hwc != 0.
 *   img : [B, C, H, W] float32 contiguous, B == grid_w * grid_h, C in {1, 3, 4}, W % 4 == 0
 *   out : uint8, [grid_h*H, grid_w*W, C] (chw_to_hwc) or [C, grid_h*H, grid_w*W]; grid_w = 1 gives the batch of
 *         HWC frames [B, H, W, C] that is all-gathered between GPUs / handed to the encoder
 * Bit-exact with the reference's torch expression (one multiply, one add, clamp, truncation).
 */
int ia_layout_grid_u8(const float* img, uint8_t* out, int B, int C, int H, int W, int grid_w, int grid_h, int chw_to_hwc, void* stream);

/*
 * Range check of the split format (debug / test aid).  The hi plane saturates at +-65504 (ia_act_split and every epilogue that writes
 * the format clamp x * style there: ia_common.h split_f16); a value that hit the clamp is no longer the fp32 number the consumer
 * should multiply.  Counts the elements of plane 0 whose magnitude is the fp16 maximum.
 *   xs : split tensor [B][planes][C/8][H*W][8] fp16;  count : device uint32 (overwritten)
 * The generator's activations stay far below the bound (|x * style| < 10^3 on the synthetic and on trained checkpoints); the tests
 * assert a zero count over a full-width frame, and hipops.CHECK_SPLIT_RANGE makes every producer check itself.
 */
int ia_split_saturation_count(const void* xs, int planes, int B, int C, int H, int W, unsigned int* count, void* stream);

/*
 * Always-on range watch of the hi / lo split.  Every producer of split-format activations (ia_act_split, the FIR tails, the
 * convolution epilogues, ia_cond_blend_split) sets a device flag when a value it splits lies outside +-65504 or is not finite
 * (it is clamped, as before).  This call reads the flags of the current device into *h_flagged (0: every split since the last
 * reset was in range), optionally clearing them; it synchronises `stream` (a host read: call it once per frame / clip, outside
 * captured graphs).  h_flagged == NULL with reset != 0 clears the flags in stream order WITHOUT a host synchronisation (the top of
 * a clip).  Real checkpoints cannot clamp silently.
 */
int ia_split_saturation_poll(unsigned int* h_flagged, int reset, void* stream);

/*
 * Input side of a captured frame: n <= 8 device-to-device segment copies in ONE launch (src[k] -> dst[k], nbytes[k] bytes).
 * The frame loop of the reference hands synthesis() fresh tensors every frame (reenact_avatar_next3d.py:196-214: ws, camera,
 * uvcoords_image); a replayed hipGraph reads fixed buffers, so the per-frame inputs are copied into them first -- with this entry
 * point as one kernel instead of one copy launch per tensor (4 x ~12 us on the frame's critical path).
 *   src, dst, nbytes : HOST arrays of n device pointers / byte counts (any alignment; 16-byte aligned segments move as uint4)
 */
int ia_stage_inputs(const void* const* src, void* const* dst, const int64_t* nbytes, int n, void* stream);

/*
 * Avatar geometry (csrc/geometry.hip).  Replaces the point query of TriPlaneGenerator.sample / sample_mixed
 * (training_avatar_texture/triplane_v20.py:341-402: renderer.run_model = sample_from_planes + OSGDecoder.forward) and the
 * chunked lattice helpers of inversion/model_utils.py:90-165; marching cubes has no counterpart in the reference.
 */
#define IA_GEOM_FLIP_Z 1              /* negate z before the plane projection (ImportanceRenderer.flip_z) */

/*
 * Decoder output at points.  planes_cl: [B,3,H,W,32] fp32 (the renderer's channels-last planes, as for ia_render_rays_box);
 * points: [B,M,3]; w0 [64,32], b0 [64], w1 [33,64], b1 [33]: the OSGDecoder's raw FullyConnectedLayer parameters (the library
 * applies the gains lr_multiplier / sqrt(fan_in) and lr_multiplier).  Per point: flip z (flags & IA_GEOM_FLIP_Z), scale by
 * 2 / box_warp, bilinear zero-padded align_corners=False gather of the three planes, mean, softplus(threshold 20) hidden layer.
 *   sigma : [B,M,1] layer-2 row 0
 *   rgb   : [B,M,32] sigmoid(rows 1..32) * 1.002 - 0.001, or NULL (density only: the colour rows are skipped)
 * fp32 VALU arithmetic throughout.
 */
int ia_query_planes(const float* planes_cl, const float* points, const float* w0, const float* b0, const float* w1, const float* b1,
                    float lr_multiplier, float box_warp, int flags, int B, int M, int plane_h, int plane_w,
                    float* sigma, float* rgb, void* stream);

/*
 * Density on an nx x ny x nz lattice without a coordinate tensor: volume[b,i,j,k] (x slowest, z fastest) is sigma of
 * ia_query_planes at the point whose coordinate along axis a is, in fp32 with every operation rounded,
 *     (h_origin[a] - 0.5f * h_cube_length[a]) + idx * (h_cube_length[a] / (n_a - 1)),
 * i.e. bit for bit ia_query_planes on those points.  Each dimension >= 2, nx * ny * nz < 2^31.
 *   h_cube_length, h_origin : HOST arrays of 3 floats;  volume : [B,nx,ny,nz] fp32
 */
int ia_density_grid(const float* planes_cl, const float* w0, const float* b0, const float* w1, const float* b1,
                    float lr_multiplier, float box_warp, int flags, int B, int plane_h, int plane_w, int nx, int ny, int nz,
                    const float* h_cube_length, const float* h_origin, float* volume, void* stream);

/*
 * Marching cubes of {volume > level} (NaN = outside) on an [nx,ny,nz] fp32 volume, each dimension >= 2, nx * ny * nz < 2^31
 * (larger volumes: IA_ERR_INVALID_ARG).  Call order:
 *   1. ia_mc_scratch_bytes -> scratch size (4 bytes per lattice point + 8 bytes per 1024 points);
 *   2. ia_mc_count(volume, level, scratch, totals): totals = device int[2] = {vertex count, triangle count} (-1: over INT32_MAX);
 *   3. the caller reads the totals (one host synchronisation) and allocates verts float [V,3] and faces int32 [F,3];
 *   4. ia_mc_emit with the SAME volume, level and scratch writes them (n_verts / n_faces: the capacities, writes beyond are dropped).
 * One vertex per lattice edge that crosses the level, ordered by owner point (the lower end, linear index) then axis x < y < z,
 * at p0 + t * (p1 - p0), t = (level - v0) / (v1 - v0) clamped to [0,1] (NaN -> 0), coordinates h_origin[a] + idx * h_spacing[a]
 * (fp32, every operation rounded).  Triangles by cell (linear index of the lower corner) then case-table order (csrc/mc_tables.h),
 * indexed into the shared vertices, wound so that normals point toward decreasing density.  No atomics: bit-reproducible.
 */
int ia_mc_scratch_bytes(int nx, int ny, int nz, size_t* h_bytes);
int ia_mc_count(const float* volume, int nx, int ny, int nz, float level, void* scratch, size_t scratch_bytes, int* totals, void* stream);
int ia_mc_emit(const float* volume, int nx, int ny, int nz, float level, const float* h_origin, const float* h_spacing,
               void* scratch, size_t scratch_bytes, float* verts, int64_t n_verts, int* faces, int64_t n_faces, void* stream);

/*
 * Isosurface ray casting over the same volumes (csrc/raycast.hip; no counterpart in the reference).  The lattice and inside rule are
 * those of marching cubes: point (i,j,k) of an [nx,ny,nz] fp32 volume (x slowest) sits at h_lo[a] + idx * h_step[a]; a point is
 * inside iff v > level (NaN: outside); between points the field is the trilinear interpolant.  Each dimension >= 2, nx*ny*nz < 2^31.
 *
 * ia_raycast_scratch_bytes -> size of the brick grid: a float2 {min, max} per brick of 8 x 8 x 8 cells (neighbouring bricks share
 * their boundary points; NaN ignored; an all-NaN brick holds {+inf, -inf}), ceil((n-1)/8) bricks per axis, z fastest.
 * ia_volume_bricks writes it.  It depends on the volume only: reuse it for any level and any number of views.
 */
#define IA_RAYCAST_DENSE 1            /* flags bit 0: walk every cell (no brick skipping; bricks may be NULL).  Results are bit-equal. */

int ia_raycast_scratch_bytes(int nx, int ny, int nz, size_t* h_bytes);
int ia_volume_bricks(const float* volume, int nx, int ny, int nz, void* bricks, size_t bricks_bytes, void* stream);

/*
 * First hit of each ray with {field > level}: rays_o, rays_d [n_rays,3] (device; any camera model), n_rays > 0.
 *   1. the ray o + t d is clipped to the lattice box [lo, lo + (n-1) step] and to t >= t_min; a ray that misses it (or has a zero
 *      or non-finite direction) is a miss;
 *   2. cells are walked in order by a 3-D DDA whose every plane crossing t is computed from the plane index directly;
 *   3. a brick whose max <= level is skipped whole (exact: the trilinear interpolant is bounded by its corners);
 *   4. a cell with a NaN corner, or with every corner <= level, has no surface;
 *   5. within a cell the field along the ray is a cubic in t, split at the roots of its derivative into monotone pieces: the hit is
 *      the first t where the field is > level (at the clipped start of the ray if it is inside already);
 *   6. refined by 20 bisection steps on the cubic (bracket < 2e-6 cell); the bracket's midpoint is reported;
 *   7. normal = -g/|g| (toward decreasing density, as the mesh is wound), 0 if |g| = 0: g = the trilinear interpolation at the hit of
 *      the central-difference gradients at the cell's corners (one-sided at the border, divided by h_step per axis).
 *   8. depth [n_rays] = t (the quantity of image_depth for unit directions), normal [n_rays,3], mask uint8 [n_rays]; a miss writes 0.
 * bricks / bricks_bytes: the grid of ia_volume_bricks for this volume (ignored with IA_RAYCAST_DENSE).  No atomics and no host
 * synchronisation: the output is a pure function of the inputs, the same with and without skipping and for any batching of rays.
 */
int ia_raycast_volume(const float* volume, int nx, int ny, int nz, const float* h_lo, const float* h_step, float level,
                      const void* bricks, size_t bricks_bytes, const float* rays_o, const float* rays_d, int n_rays, float t_min,
                      float* depth, float* normal, unsigned char* mask, int flags, void* stream);

/*
 * The gradient g of step 7 above at arbitrary points [n,3] (clamped into the box) -> grad [n,3]; -g/|g| are the vertex normals of
 * the marching-cubes mesh of the same volume.  n >= 0.
 */
int ia_volume_gradient(const float* volume, int nx, int ny, int nz, const float* h_lo, const float* h_step, const float* points,
                       int n, float* grad, void* stream);

/*
 * Per-frame image metrics (csrc/image_metrics.hip).  Replaces, for evaluation, ssim / msssim of encoder_inversion/criteria/ms_ssim.py
 * (size_average=False, no `normalize`): 11-tap Gaussian window (sigma 1.5), "valid" correlation, per channel, L = data_range,
 *     mu1 = G*a, mu2 = G*b, s1 = G*(a*a) - mu1^2, s2 = G*(b*b) - mu2^2, s12 = G*(a*b) - mu1*mu2, C1 = (0.01 L)^2, C2 = (0.03 L)^2,
 *     cs_map = (2 s12 + C2) / (s1 + s2 + C2),  ssim_map = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1) * cs_map,
 * ssim_k[n], cs_k[n] = their means over (c, y, x) at level k; level k + 1 = 2 x 2 average pool (floor) of level k;
 * ms_ssim[n] = prod_{k<4} cs_k^w_k * ssim_4^w_4, w = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) (a negative mean gives NaN, as in the
 * reference); mse[n], l1[n] = means of (a-b)^2, |a-b| over all pixels of level 0; psnr = 10 log10(L^2 / mse) (+inf for mse = 0).
 *   a, b    : IA_IMAGE_F32_NCHW: float [n,c,h,w];  IA_IMAGE_U8_NHWC: uint8 [n,h,w,c], converted on load (values 0..255)
 *   c in 1..4, levels in 1..5, min(h, w) >> (levels - 1) >= 11 (smaller images are refused; the reference shrinks its window instead)
 *   scratch : ia_image_metrics_scratch_bytes(n, c, h, w, levels) bytes, 8-byte aligned (host arithmetic only): the tiles' partial sums
 *             (doubles) and the pooled image pairs of levels 1..levels-1
 *   out     : float [n, 5 + 2 * levels]: mse, l1, psnr, ssim (= ssim_0), ms_ssim, ssim_0 .. ssim_{levels-1}, cs_0 .. cs_{levels-1}.
 *             MS-SSIM is defined on five levels only: with levels < 5 the column ms_ssim holds NaN (it is not a copy of ssim).
 * `levels` launches + one finalising launch whatever n is; no atomics: the same inputs give the same bits, and a frame's results do
 * not depend on the batch it is part of.  Invalid arguments return IA_ERR_INVALID_ARG before anything is launched.
 */
#define IA_IMAGE_F32_NCHW 0
#define IA_IMAGE_U8_NHWC 1

int ia_image_metrics_scratch_bytes(int n, int c, int h, int w, int levels, size_t* h_bytes);
int ia_image_metrics(const void* a, const void* b, int layout, int n, int c, int h, int w, float data_range, int levels,
                     void* scratch, size_t scratch_bytes, float* out, void* stream);

/*
 * Connected components (csrc/components.hip; no counterpart in the reference): which parts of {volume > level} hang together, how
 * large they are, and a filter that drops the unwanted ones before the volume is meshed or ray-cast.  The lattice and inside rule are
 * those of marching cubes and ray casting: point (i,j,k) of an [nx,ny,nz] fp32 volume (x slowest) is inside iff v > level (NaN:
 * outside).  Each dimension >= 2, nx * ny * nz < 2^31 (otherwise IA_ERR_INVALID_ARG).
 *   connectivity : 26 (indices differ by at most 1 on every axis) or 6 (by exactly 1 on one axis); anything else is refused
 *   labels       : int32 [nx,ny,nz]; 0 outside; components 1..K numbered in increasing order of their smallest linear index
 *                  (i * ny + j) * nz + k
 *   scratch      : ia_components_scratch_bytes bytes (4 per point + 4 per 1024 points), 4-byte aligned; nothing in it survives a call
 *   count        : device int[1] = K; the caller reads it (one host synchronisation) before it sizes `stats`
 * Union-find whose roots are smallest indices (8 x 8 x 64 tiles in LDS, then the tile seams with agent-scope integer atomic min on
 * the parent array, then numbering by a scan): the result does not depend on the order in which the atomics land, so labels are
 * bit-reproducible.  Every loop is lock-free and strictly descending: no workgroup ever waits for another one.
 *
 * ia_component_stats: stats int32 [K,8], row c-1 for label c: point count, smallest linear index, then the inclusive index bounding
 * box imin, jmin, kmin, imax, jmax, kmax (integer atomic add / min / max: bit-reproducible).  K: the count read above; K < 0 or
 * K > nx*ny*nz is refused, K = 0 launches nothing, and labels outside 1..K are ignored (never written through).
 *
 * ia_volume_keep: out[p] = fill where labels[p] is in 1..K and keep_flags[labels[p]] == 0, else volume[p] (bit copy); points of label
 * 0 are never modified.  keep_flags: device uint8 [K+1] ([0] ignored); n = number of points; out may alias volume.  fill = level
 * makes the dropped points outside for marching cubes and ray casting at that level.
 */
int ia_components_scratch_bytes(int nx, int ny, int nz, size_t* h_bytes);
int ia_volume_components(const float* volume, int nx, int ny, int nz, float level, int connectivity, int* labels, void* scratch,
                         size_t scratch_bytes, int* count, void* stream);
int ia_component_stats(const int* labels, int nx, int ny, int nz, int K, int* stats, void* stream);
int ia_volume_keep(const float* volume, const int* labels, int64_t n, const unsigned char* keep_flags, int K, float fill, float* out,
                   void* stream);

/*
 * The same labelling for an indexed triangle mesh: vertices a, b are connected if some face contains both.
 *   faces       : int32 [F,3] (a face with an index outside [0, V) is ignored); 3 F < 2^31
 *   vert_labels : int32 [V], components 1..K in increasing order of their smallest vertex index; a vertex used by no face is a
 *                 component of its own
 *   scratch     : ia_mesh_components_scratch_bytes(V) bytes;  count : device int[1] = K
 * ia_mesh_component_stats: stats int32 [K,3], row c-1: vertex count, face count (a face belongs to the component of its first
 * vertex), smallest vertex index.
 */
int ia_mesh_components_scratch_bytes(int V, size_t* h_bytes);
int ia_mesh_components(const int* faces, int64_t F, int V, int* vert_labels, void* scratch, size_t scratch_bytes, int* count,
                       void* stream);
int ia_mesh_component_stats(const int* faces, int64_t F, int V, const int* vert_labels, int K, int* stats, void* stream);

/*
 * Distance between surfaces (csrc/surface_distance.hip; no counterpart in the reference): exact distance from points to a triangle
 * mesh, and the reductions behind Chamfer distance, Hausdorff distance and F-score.
 *
 * The distance from p to a triangle is the Euclidean distance to the closed triangle (a triangle without area is a segment or a
 * point); the distance to a mesh is the minimum over its usable triangles of ONE fp32 per-triangle function, taken on the pair
 * (distance, index).  The grid only prunes: results are bit-identical with and without it, for every grid resolution, run to run.
 *
 * ia_tri_pack: tris = float4 [F,3] (48 bytes per triangle, 16-byte aligned): A, B, C with A.w = 1 for a usable triangle and 0 for an
 * ignored one (a non-finite coordinate, or an index outside [0, V)).  faces int32 [F,3], F <= 2^25.
 *
 * ia_trigrid_plan (host arithmetic only): from F and the bounding box [lo, hi] of the finite vertices, dims[3] (about one cubic cell
 * per triangle, at most 256 per axis; request[a] > 0 fixes an axis, up to 1024; request may be NULL) and inv_cell[3].  The cell of a
 * coordinate x along an axis is clamp(floor((x - lo) * inv_cell), 0, dims - 1), in fp32.  At most 2^26 cells.
 *
 * ia_trigrid_count: cell_start int32 [ncell + 2] (ncell = dims[0] * dims[1] * dims[2], x slowest).  A usable triangle is counted in
 * every cell its bounding box covers, or, if these are more than 64, as oversize.  On return cell_start[0 .. ncell] are the exclusive
 * offsets (cell_start[ncell] = entries <= 64 F) and cell_start[ncell + 1] = the number of oversize triangles; the caller reads these
 * two (one host synchronisation) and sizes cell_tris = int32 [entries + n_over].
 * ia_trigrid_fill: writes the cells' triangle lists (in any order) and, behind them, the oversize list, which every query tests.
 * scratch: 4 * (ncell + 1) bytes.
 *
 * ia_closest_point: per query point (float32 [N,3]) dist float32 [N], face int32 [N] (the triangle that attains the fp32 minimum; the
 * lowest index among equals), point float32 [N,3] (the closest point on that triangle).  A non-finite query gives NaN / -1 / NaN, a
 * mesh without usable triangles +inf / -1 / NaN.  cell_start == NULL: brute mode, the same kernel body walks all F triangles (lo,
 * inv_cell, dims, cell_tris, entries, n_over are then ignored).  mesh_extent: the largest |coordinate| of the mesh (it scales the
 * safety margin of the shell search; a larger value only costs time).
 *
 * ia_distance_stats: out = double [14]: number of finite entries of dist, their sum, sum of squares and maximum (-inf if none), the
 * sum of |normals_a[i] . normals_b[face[i]]| over finite entries with face in [0, Fb) (0 without normals: face, normals_a, normals_b
 * all NULL), the number of non-finite entries, and for k < n_thresholds <= 8 the number of finite entries <= thresholds[k] (a host
 * array).  Double sums per workgroup, combined in index order by a second launch: no floating-point atomics, bit-equal run to run.
 * scratch: ia_distance_stats_scratch_bytes(N) bytes, 8-byte aligned.
 */
int ia_tri_pack(const float* verts, int V, const int* faces, int64_t F, void* tris, void* stream);
int ia_trigrid_plan(int64_t F, const float* h_lo, const float* h_hi, const int* h_request, int* h_dims, float* h_inv_cell);
int ia_trigrid_count(const void* tris, int64_t F, const float* h_lo, const float* h_inv_cell, const int* h_dims, int* cell_start,
                     void* stream);
int ia_trigrid_fill(const void* tris, int64_t F, const float* h_lo, const float* h_inv_cell, const int* h_dims, const int* cell_start,
                    int entries, int n_over, void* scratch, size_t scratch_bytes, int* cell_tris, void* stream);
int ia_closest_point(const float* points, int64_t N, const void* tris, int64_t F, float mesh_extent, const float* h_lo,
                     const float* h_inv_cell, const int* h_dims, const int* cell_start, const int* cell_tris, int entries, int n_over,
                     float* dist, int* face, float* point, void* stream);
int ia_distance_stats_scratch_bytes(int64_t N, size_t* h_bytes);
int ia_distance_stats(const float* dist, int64_t N, const float* h_thresholds, int n_thresholds, const int* face,
                      const float* normals_a, const float* normals_b, int64_t Fb, void* scratch, size_t scratch_bytes, double* out,
                      void* stream);

/*
 * Mesh simplification by quadric vertex clustering (csrc/simplify.hip; no counterpart in the reference; the definition is written out
 * in invertavatar_amd/geometry.py simplify_mesh and DESIGN.md 4.15).  Additive entry points: the ABI version is unchanged.
 *
 * The cell of a coordinate is the fp32 function of ia_trigrid_plan, clamp(floor((x - lo) * inv_cell), 0, dims - 1); the key of a vertex
 * is its linear cell index (x slowest) as int64, INT64_MAX for a vertex with a non-finite coordinate.  V, F <= 2^28, dims <= 2^20.
 *
 * ia_simplify_plan (host arithmetic only): exactly one of cells[3] (cells per axis), cells_long (cubic cells, that many along the
 * longest axis of the box) and cell_size (the edge) is given (NULL / 0 / 0.0 otherwise) -> dims[3], inv_cell[3] = fp32(1 / cell), cell[3]
 * (double edge per axis; an axis without extent has the edge 1 under cells[3]).
 * ia_simplify_box: box = device float [6], lo and hi of the finite vertices (+inf / -inf without one).  scratch: 24576 bytes.
 * ia_simplify_keys: keys int64 [V].
 * ia_simplify_clusters: from the sorted keys and the permutation that sorted them (int64 [V] both): vert_cluster int32 [V] (ordinal of
 * the vertex's cluster in ascending key order, -1 without a cell), sorted_cluster int32 [V] (the same by sorted position, INT32_MAX
 * without a cell), cluster_start int32 [capacity + 1] (first sorted position; cluster_start[K] = number of vertices with a cell),
 * cluster_key int64 [capacity], count = device int [2]: K and the number of vertices with a cell.  scratch: 4 (V + 1) bytes.
 * ia_simplify_classify: per face (int32 [F,3]; an index outside [0, V) makes it unusable) tri int32 [F,3] (the three cluster ordinals
 * rotated smallest first, INT32_MAX x 3 unless the face is usable with three different clusters), key int64 [F] ((a K + b) K + c, or
 * b K + c when K^3 >= 9e18: sort by key, then stably by a; INT64_MAX for a face that does not survive), ref int32 [K] (1 for a cluster
 * of a surviving face; may be NULL), pairs int32 [3 F] (per corner the cluster the face's quadric goes to, INT32_MAX for an unusable
 * face or a cluster an earlier corner named; may be NULL), count = device int [3]: usable faces, surviving faces, pairs.
 * ia_simplify_face_heads: perm int64 [F] sorts the faces by tri -> face_pos int32 [F + 1]: exclusive count of unique surviving
 * triples before each sorted position, face_pos[F] = F'.       ia_simplify_refs: out_index int32 [K + 1] = exclusive scan of ref.
 * ia_simplify_outputs: vertex_map int64 [V]; for each of the out_index[K] output vertices (at most capacity are written) out_cluster
 * int32 and cluster_size int64.       ia_simplify_faces: faces_out int64 [capacity,3], unique, lexicographically increasing.
 * ia_simplify_accumulate_verts: sums double [K,4]: per cluster the sums of columns col0 .. col0 + ncols (<= 4) of cols double [V,ld]
 * over its vertices, n = number of vertices with a cell.  ia_simplify_accumulate_faces: sums double [K,9]: per cluster the sum over its
 * pairs (pair_order int64 [>= n] and sorted_pairs int32 [>= n]: the stable sort of pairs, n = count[2]) of n n^T (xx xy xz yy yz zz)
 * and -n (n . (A - centre)), n the normal from the two shorter edges, centre the centre of the cluster's cell, all in double.  Both:
 * chunks of 32 entries in index order, partial rows reduced level by level; no floating-point atomics, bit-equal from run to run.
 * scratch: ia_simplify_accumulate_scratch_bytes(n, 4 or 9) bytes, 8-byte aligned.
 * ia_simplify_place: verts_out float32 [n_out,3]: the cluster mean (quadric_sums NULL) or the minimiser of the summed quadric about
 * the mean (cyclic Jacobi, 8 sweeps; eigenvalues <= 1e-3 of the largest dropped) clamped to the cell.
 * ia_simplify_means: out[o, col0 .. col0 + ncols) = sums / cluster size, out double [capacity, ld].
 */
int ia_simplify_plan(const float* h_lo, const float* h_hi, const int* h_cells, int cells_long, double cell_size, int* h_dims,
                     float* h_inv_cell, double* h_cell);
int ia_simplify_box(const float* verts, int64_t V, void* scratch, size_t scratch_bytes, float* box, void* stream);
int ia_simplify_keys(const float* verts, int64_t V, const float* h_lo, const float* h_inv_cell, const int* h_dims, int64_t* keys,
                     void* stream);
int ia_simplify_clusters(const int64_t* sorted_keys, const int64_t* order, int64_t V, int* vert_cluster, int* sorted_cluster,
                         int* cluster_start, int64_t* cluster_key, int64_t capacity, void* scratch, size_t scratch_bytes, int* count,
                         void* stream);
int ia_simplify_classify(const int* faces, int64_t F, int64_t V, const int* vert_cluster, int K, int* tri, int64_t* key, int* ref,
                         int* pairs, int* count, void* stream);
int ia_simplify_face_heads(const int* tri, const int64_t* perm, int64_t F, int* face_pos, void* stream);
int ia_simplify_refs(const int* ref, int K, int* out_index, void* stream);
int ia_simplify_outputs(const int* vert_cluster, int64_t V, const int* ref, const int* out_index, const int* cluster_start, int K,
                        int64_t* vertex_map, int* out_cluster, int64_t* cluster_size, int64_t capacity, void* stream);
int ia_simplify_faces(const int* tri, const int64_t* perm, const int* face_pos, int64_t F, const int* out_index, int K,
                      int64_t* faces_out, int64_t capacity, void* stream);
int ia_simplify_accumulate_scratch_bytes(int64_t n, int width, size_t* h_bytes);
int ia_simplify_accumulate_verts(const double* cols, int ld, int col0, int ncols, const int64_t* order, const int* sorted_cluster,
                                 int64_t n, int64_t V, int K, double* sums, void* scratch, size_t scratch_bytes, void* stream);
int ia_simplify_accumulate_faces(const float* verts, int64_t V, const int* faces, int64_t F, const int64_t* pair_order,
                                 const int* sorted_pairs, int64_t n, const int64_t* cluster_key, int K, const float* h_lo,
                                 const float* h_inv_cell, const double* h_cell, const int* h_dims, double* sums, void* scratch,
                                 size_t scratch_bytes, void* stream);
int ia_simplify_place(const double* vert_sums, const double* quadric_sums, const int* out_cluster, const int* cluster_start,
                      const int64_t* cluster_key, int K, int64_t n_out, const float* h_lo, const float* h_inv_cell, const double* h_cell,
                      const int* h_dims, float* verts_out, int64_t capacity, void* stream);
int ia_simplify_means(const double* vert_sums, const int* out_cluster, const int* cluster_start, int K, int64_t n_out, int ncols,
                      double* out, int ld, int col0, int64_t capacity, void* stream);

/* Mesh smoothing (Taubin lambda | mu, Laplacian) and vertex normals from the mesh (csrc/smooth.hip; definition: geometry.smooth_mesh,
 * geometry.MeshAdjacency, geometry.mesh_normals and their NumPy restatement).  verts float32 [V,3], faces int32 [F,3],
 * V, F <= 2^28.  A face is usable if its indices are distinct, in [0, V), and its vertices finite.
 *
 * ia_mesh_edge_keys: edge_keys int64 [6 F] (per usable face (a,b,c) the keys i V + j of (a,b) (b,a) (b,c) (c,b) (c,a) (a,c); INT64_MAX
 * for an unusable face), vertex_keys int64 [3 F] (v F + f per corner, INT64_MAX likewise).  count = device int [8], cleared here and filled
 * by this and the next two calls: [0] usable faces, [1] 1 if an index is outside [0, V), [2] directed entries with one face, [3] with
 * more than two faces, [4] boundary vertices, [5] largest degree, [6] vertices of degree > 64, [7] E (distinct directed edges).
 * ia_mesh_edge_heads: from the edge keys sorted ascending (stable), scratch (ia_mesh_edge_heads_scratch_bytes(F) bytes) receives the first
 * CSR slot of every workgroup of 256 sorted entries and count[7] = E.
 * ia_mesh_csr: usable = count[0] and E = count[7] as read by the host; scratch as left by ia_mesh_edge_heads; vertex_order int64 [3 F]
 * is the permutation that sorted vertex_keys.  offsets int32 [V + 1], neighbors / edge_faces / run_start int32 [E] (run_start: first
 * sorted position of the slot's entries), slot_keys int64 [E], boundary uint8 [V], face_offsets int32 [V + 1], face_ids int32
 * [3 usable], heavy int32 [V] (the first count[6] entries: vertices of degree > 64, in no particular order).
 * ia_mesh_cotangent: weights float32 [E] = max(0, 1/2 sum cot) over the faces on the edge in face order (double); edge_order int64 [6 F]
 * is the permutation that sorted edge_keys.
 * ia_smooth_pinned: pinned uint8 [V]: non-finite, no neighbour, all weights zero (weights may be NULL: uniform), boundary if
 * fix_boundary, or fixed (uint8 [V], may be NULL).
 * ia_smooth_steps: n_steps Jacobi steps p' = fp32(p + f (sum w p_j / sum w - p)) with the host factors h_factors[n_steps], from verts_a
 * into verts_b and back; the result is in verts_a if n_steps is even, else in verts_b.  No host synchronisation.  heavy / n_heavy: as
 * left by ia_mesh_csr (count[6]).
 * ia_mesh_normals: normals float32 [V,3]: the normalised sum over the vertex's usable faces of the cross product (angle = 0) or of the
 * unit normal times the corner angle (angle = 1); 0 where the sum has no direction.
 */
int ia_mesh_edge_keys(const float* verts, int64_t V, const int* faces, int64_t F, int64_t* edge_keys, int64_t* vertex_keys, int* count,
                      void* stream);
int ia_mesh_edge_heads_scratch_bytes(int64_t F, size_t* h_bytes);
int ia_mesh_edge_heads(const int64_t* sorted_keys, int64_t F, void* scratch, size_t scratch_bytes, int* count, void* stream);
int ia_mesh_csr(const int64_t* sorted_keys, const int64_t* sorted_vertex_keys, const int64_t* vertex_order, int64_t V, int64_t F,
                int64_t usable, int64_t E, const void* scratch, int* offsets, int* neighbors, int* edge_faces, int* run_start,
                int64_t* slot_keys, unsigned char* boundary, int* face_offsets, int* face_ids, int* heavy, int* count, void* stream);
int ia_mesh_cotangent(const float* verts, int64_t V, const int* faces, int64_t F, const int64_t* edge_order, const int64_t* slot_keys,
                      const int* run_start, const int* edge_faces, int64_t E, float* weights, void* stream);
int ia_smooth_pinned(const float* verts, int64_t V, const int* offsets, const float* weights, const unsigned char* boundary,
                     int fix_boundary, const unsigned char* fixed, unsigned char* pinned, void* stream);
int ia_smooth_steps(float* verts_a, float* verts_b, int64_t V, const int* offsets, const int* neighbors, const float* weights,
                    const unsigned char* pinned, const int* heavy, int n_heavy, const double* h_factors, int n_steps, void* stream);
int ia_mesh_normals(const float* verts, int64_t V, const int* faces, int64_t F, const int* face_offsets, const int* face_ids, int angle,
                    float* normals, void* stream);

/* Z-buffer rasteriser for indexed meshes (csrc/mesh_raster.hip; definition: geometry.rasterize_mesh and its NumPy restatement;
 * DESIGN.md 4.18).  verts float32 [V,3], faces int32 [F,3], cams float32 [N,25] on the device (cam2world 4x4, K 3x3 normalised; rows 0
 * and 1 of K are scaled by W and H), V, F <= 2^28, N <= 65535, H, W <= 16384, N F, N V and N H W below 2^31.  Pixel centres are at
 * integer coordinates (column i, row j of RaySampler_zxc).  All launches go to `stream`.
 *
 * ia_mesh_project: proj = N V records of 16 bytes {int32 U, V (screen coordinates in 1/256 pixel), float z (camera depth), int32
 * usable}; a vertex is unusable if a value is not finite, z <= near, or |u| or |v| >= 2^20 pixels.  Reads the N camera labels back once
 * before its launch: a K whose last row is not [0, 0, 1] is IA_ERR_INVALID_ARG.
 * ia_mesh_raster: vis uint64 [N,H,W] = per pixel the least key float_bits(z) << 32 | face over the triangles that cover its centre
 * (integer edge functions, top-left rule; all ones where none does); culled int32 [N] = triangles with an unusable vertex.  Zero-area
 * triangles are skipped, nothing is clipped at the near plane.  cull_back: draw only triangles that face the camera (negative screen
 * area).  A triangle whose viewport-clamped bounding box holds more than oversize_pixels pixels is drawn by a wave of its own; both
 * paths give the same buffer.  scratch: ia_mesh_raster_scratch_bytes(N, F) bytes (not needed when oversize_pixels >= H W).
 * ia_mesh_resolve: per pixel mask uint8, face int32 (-1 on a miss), bary float32 [3] (perspective-correct), depth (ray parameter of the
 * pixel's unit ray, 0 on a miss), normal float32 [3] (unit normal of the winding, or with normals float32 [V,3] their normalised
 * barycentric mix; 0 on a miss) and, with attributes float32 [V,C], C <= 8, their barycentric mix attr_out float32 [N,H,W,C].
 * cull_back as given to ia_mesh_raster.
 */
int ia_mesh_project(const float* verts, int64_t V, const float* cams, int N, int H, int W, float near, void* proj, void* stream);
int ia_mesh_raster_scratch_bytes(int N, int64_t F, size_t* h_bytes);
int ia_mesh_raster(const void* proj, int64_t V, const int* faces, int64_t F, int N, int H, int W, int cull_back, int64_t oversize_pixels,
                   unsigned long long* vis, int* culled, void* scratch, size_t scratch_bytes, void* stream);
int ia_mesh_resolve(const unsigned long long* vis, const void* proj, const float* verts, int64_t V, const int* faces, int64_t F,
                    const float* cams, int N, int H, int W, int cull_back, const float* normals, const float* attributes, int C,
                    unsigned char* mask, int* face, float* bary, float* depth, float* normal, float* attr_out, void* stream);

/*
 * Alignment of a point set to a triangle mesh (csrc/align.hip; no counterpart in the reference; definition: geometry.align_mesh and
 * its NumPy restatement).  The two kernels around ia_closest_point in one ICP iteration.  Additive entry points: the ABI
 * version is unchanged.
 *
 * ia_transform_points: out float32 [N,3] = fp32(M) x for points float32 [N,3]; h_m12 = 12 doubles on the host, the rows of [s R | t],
 * rounded to fp32 here.  Per row ((m0 x + m1 y) + m2 z) + t, every operation rounded on its own.  A non-finite input gives a
 * non-finite output.  out may be points.
 *
 * ia_align_sums: the sums of one iteration over the pairs (src[i], dst[i]) that count: dist[i] finite, face[i] >= 0,
 * dist[i] <= h_max_dist (fp32 compare; +inf: no threshold) and, for mode 1, face[i] < Fb with a finite, non-zero face_normals[face[i]].
 * With p = src[i] - centre and q = dst[i] - centre in double (h_centre: 3 doubles on the host), out is
 *   mode 0 (point), double [20]: n, sum p (3), sum q (3), sum p q^T (9, row-major), sum |p|^2, sum |q|^2, sum |p - q|^2, and in the
 *                                last slot the number of pairs that do not count;
 *   mode 1 (plane), double [56]: the same 19 sums, then with a = (p x n, n, p . n) and b = (q - p) . n the upper triangle of
 *                                sum a a^T (28, row-major), sum a b (7), sum b^2, and in the last slot the pairs that do not count.
 * src, dst float32 [N,3], dist float32 [N], face int32 [N], face_normals float32 [Fb,3] (ignored for mode 0).  A thread sums a
 * contiguous slice in index order, wave and workgroup combine in a fixed order and a second launch adds the workgroups in a fixed order:
 * no floating-point atomics, bit-equal run to run.  scratch: ia_align_sums_scratch_bytes(N, mode) bytes, 8-byte aligned.
 */
int ia_transform_points(const float* points, int64_t N, const double* h_m12, float* out, void* stream);
int ia_align_sums_scratch_bytes(int64_t N, int mode, size_t* h_bytes);
int ia_align_sums(const float* src, const float* dst, const float* dist, const int* face, int64_t N, const float* face_normals,
                  int64_t Fb, const double* h_centre, float h_max_dist, int mode, void* scratch, size_t scratch_bytes, double* out,
                  void* stream);

/*
 * Pose search for global registration (csrc/pose_search.hip; no counterpart in the reference; definition: geometry.pose_scores and
 * its NumPy restatement).  Additive entry point: the ABI version is unchanged.
 *
 * ia_pose_scores: out double [R, shifts^3] = the score of every candidate pose of the points float32 [n,3], n <= 4096, against the
 * unsigned distance lattice dist float32 [nx,ny,nz] (x slowest; point (i,j,k) at h_origin + index * h_spacing, cubic cells):
 *   score[r, k] = sum_i min(d(p_i), h_cap)^2 / n,   p_i = h_scale (R_r (x_i - fp32(h_c_src))) + (fp32(h_c_tgt) + o_k)
 * with rotations float32 [R,9] row-major on the device, o_k = ((a_x, a_y, a_z) - (shifts - 1) / 2) h_shift_step for the offset index
 * k = (a_x shifts + a_y) shifts + a_z (shifts odd, <= 15), and the lookup, per axis u = (p - origin) fp32(1 / h), c = clamp(u, 0,
 * dim - 1), i = min(floor(c), dim - 2), t = c - i:  d = trilinear(dist, i, t) + h |u - c|_2 (lerp(a, b, t) = a + t (b - a) along z,
 * then y, then x).  Float32 per point, every operation rounded on its own; min(d, cap) is squared and summed in double, per thread in
 * index order, then wave, then workgroup in a fixed order: no floating-point atomics, and a candidate's score has the same bits from
 * run to run, in any set or order of candidates and for any split of R.  A non-finite point gives a non-finite score to every
 * candidate (drop such rows first).  h_origin: 3 floats, h_c_src and h_c_tgt: 3 doubles, all on the host; h_cap = +inf: no cap.
 * n = 0 or R = 0: nothing is launched and out is not written.  No scratch.
 */
int ia_pose_scores(const float* points, int n, const float* dist, int nx, int ny, int nz, const float* h_origin, float h_spacing,
                   const float* rotations, int64_t R, const double* h_c_src, const double* h_c_tgt, int shifts, float h_shift_step,
                   float h_scale, float h_cap, double* out, void* stream);

/*
 * Generalised winding number of points with respect to a triangle soup (csrc/winding.hip; no counterpart in the reference;
 * definition: geometry.winding_number and its NumPy restatement): 1 inside a closed outward-wound mesh, 0 outside,
 * in between for an open one.  Additive entry points: the ABI version is unchanged.
 *
 * ia_winding_number: out double [N] for points float32 [N,3] and tris = the F packed triangles of ia_tri_pack (three float4 per
 * triangle; A.w = 0: skipped).  Per pair, in fp32 with every operation rounded on its own, relative to the query (a = A - p, ...):
 * omega = 2 atan2f(a . ((b - a) x (c - a)), (((|a| |b|) |c| + (a . b) |c|) + (b . c) |a|) + (c . a) |b|).  The faces are cut into
 * chunks of `chunk` faces (ia_winding_layout); a chunk's omegas are added in double in face order, the chunk sums in chunk order, and
 * the total is divided by 4 pi.  The result for a point therefore depends on the point and the mesh alone, not on N, the order of the
 * points, how a caller cuts them into calls, or the run; no floating-point atomics.  A non-finite point gives NaN; F = 0 or no usable
 * triangle gives 0.  The cost is N F pairs.  scratch: ia_winding_number_scratch_bytes(N, F) bytes = 8 N ceil(F / chunk), 8-byte
 * aligned; a caller that must bound it cuts the points into several calls.  N >= 0 with 3 N < 2^31, 0 <= F <= 2^25.
 * ia_winding_layout (host only): triangles per LDS tile, faces per chunk and points per workgroup of the kernel, the sizes at which
 * it changes path.
 */
int ia_winding_layout(int* h_tile, int* h_chunk, int* h_points);
int ia_winding_number_scratch_bytes(int64_t N, int64_t F, size_t* h_bytes);
int ia_winding_number(const float* points, int64_t N, const void* tris, int64_t F, void* scratch, size_t scratch_bytes, double* out,
                      void* stream);

/*
 * Fast winding numbers: an implicit cluster tree over the triangles with a far-field expansion per node (csrc/winding_tree.hip; no
 * counterpart in the reference; definition: geometry.WindingTree and its NumPy restatement).  ia_winding_number stays
 * the exact sum these are held to.  Additive entry points: the ABI version is unchanged.
 *
 * ia_winding_tree_layout (host only): faces per leaf L, children per upper node B, floats per node row (20 = 5 float4) and the largest
 * number of levels.  L and B are part of the results.
 * ia_winding_tree_face_keys: keys int32 [F] of the packed triangles of ia_tri_pack: the 30-bit Morton key of the centroid, 10 bits per
 * axis (x lowest), cell = clamp(floor((c - lo) * scale), 0, 1023) in fp32 with c = ((A + B) + C) * fp32(1 / 3); 2^30 for a triangle
 * with A.w = 0.  h_lo: the low corner of the box of the finite vertices, h_scale = fp32(1024) / (its longest side), 0 without extent.
 * ia_winding_tree_point_keys: the same key for points float32 [N,3]; 2^30 for a non-finite point.  (Sorting queries by it brings
 * neighbours into one wave; it changes no result.)
 * ia_winding_tree_gather: sorted[s] = tris[order[s]] for order int32 [F], the stable ascending sort of the face keys (the caller's).
 * ia_winding_tree_plan (host only): for F_usable faces (keys below 2^30) the number of levels, the nodes per level (h_counts: int
 * [max levels], leaves first: ceil(F_usable / L), then ceil(previous / B) down to 1), their total and the bytes of scratch that
 * ia_winding_tree_nodes needs.  F_usable = 0: no level, no node.
 * ia_winding_tree_nodes: nodes float32 [n_nodes, 20], level by level with the leaves first: (c.x, c.y, c.z, r) (D.x, D.y, D.z, A)
 * (Q00 Q01 Q02 Q10) (Q11 Q12 Q20 Q21) (Q22, 0, 0, 0) with A = sum a_t, D = sum a_t n_t, c = sum a_t c_t / A (the mean of the centroids
 * c_t when A = 0), Q = sum (c_t - c) (x) a_t n_t, r = the largest distance of a vertex from c.  Leaf i holds sorted faces [i L,
 * min((i + 1) L, F_usable)) and is summed in double in face order; an upper node is formed in double from its children in child order
 * (Q = sum Q_k + (c_k - c) (x) D_k, r = max |c_k - c| + r_k); every entry is rounded to fp32 once.  No atomics: bit-equal run to run.
 * scratch: the double rows, 8-byte aligned.
 * ia_winding_tree_query: out double [N].  Per point q, depth first from the root, children in index order; at a node, in fp32 with
 * every operation rounded on its own, x = c - q, d2 = (x.x^2 + x.y^2) + x.z^2, far = d2 > (beta r)(beta r).  A far node adds
 * ((D . x + tr Q) - 3 (x^T Q x) / d2) / (d2 sqrt(d2)), a near leaf the solid angles of ia_winding_number of its faces in sorted order,
 * a near upper node is descended.  Terms are fp32, the running sum is double in visiting order, out = sum / 4 pi; NaN for a non-finite
 * point.  A pure function of point, mesh and beta: independent of N, the order of the points and the run.  beta > 1, or +inf (never
 * far: the exact terms).  bound (double [N], or NULL): sum over the far nodes of 3 A r^2 / (4 pi (d - r)^4), which bounds the
 * truncation error.  counts (int32 [N,2], or NULL): far terms and exact pairs of the point.
 */
int ia_winding_tree_layout(int* h_leaf, int* h_branch, int* h_row_floats, int* h_max_levels);
int ia_winding_tree_plan(int64_t F_usable, int* h_levels, int* h_counts, int64_t* h_nodes, size_t* h_scratch_bytes);
int ia_winding_tree_face_keys(const void* tris, int64_t F, const float* h_lo, float h_scale, int* keys, void* stream);
int ia_winding_tree_point_keys(const float* points, int64_t N, const float* h_lo, float h_scale, int* keys, void* stream);
int ia_winding_tree_gather(const void* tris, int64_t F, const int* order, void* sorted, void* stream);
int ia_winding_tree_nodes(const void* sorted, int64_t F_usable, void* scratch, size_t scratch_bytes, void* nodes, int64_t n_nodes,
                          void* stream);
int ia_winding_tree_query(const float* points, int64_t N, const void* sorted, int64_t F_usable, const void* nodes, int64_t n_nodes,
                          float beta, double* out, double* bound, int* counts, void* stream);

/*
 * Closest point on the cluster tree: the query of ia_closest_point by branch and bound over the tree of ia_winding_tree_plan
 * (csrc/closest_tree.hip; no counterpart in the reference; definition: geometry._closest_tree_numpy).  The tree only
 * prunes: dist, face and point are bit-identical to ia_closest_point in the brute mode and through any grid.  Additive entry points:
 * the ABI version is unchanged.
 *
 * ia_tree_boxes: boxes float32 [n_nodes, 8], two float4 per node in the level layout of ia_winding_tree_plan (leaves first):
 * (lo.x, lo.y, lo.z, 0) (hi.x, hi.y, hi.z, 0).  A leaf takes the minimum / maximum per axis over the vertices of its sorted faces
 * [i L, min((i + 1) L, F_usable)), an upper node over its children.  sorted: the triangles of ia_winding_tree_gather.  Min and max
 * are exact and independent of order: bit-equal run to run.
 * ia_closest_point_tree: dist float32 [N], face int32 [N] (an INPUT face index: order[sorted position]), point float32 [N,3] for
 * points float32 [N,3]; order int32 [>= F_usable]: sorted position -> input face.  best = (dist, face), ordered lexicographically,
 * starts at (+inf, -1); a visited leaf evaluates the per-triangle function of ia_closest_point for its faces and keeps the smaller
 * pair.  A node is skipped iff lb is finite and lb - slack > best.dist, where, in fp32 with every operation rounded on its own,
 * g = max(max(lo - p, p - hi), 0) per axis, lb = sqrt((g.x^2 + g.y^2) + g.z^2) and slack = 2^-17 max(|p|_inf, mesh_extent)
 * (= 64 eps32 times that; mesh_extent: the largest |coordinate| of the usable triangles).  A skipped node holds no triangle whose
 * computed distance is <= best.dist, so neither the minimum nor the tie changes.  The walk: each point first descends from the root to
 * the child with the smallest lb (the lowest index among equals) and evaluates that leaf; then depth first from the root, children in
 * index order, passing over that leaf.  The order changes the cost, never the result.  A non-finite point gives NaN / -1 / NaN,
 * F_usable = 0 gives +inf / -1 / NaN.  counts (int32 [N,2], or NULL): boxes tested and point-triangle pairs evaluated for the point,
 * the first descent included.  N >= 0 with 3 N < 2^31, 0 <= F_usable <= 2^25, n_nodes that of ia_winding_tree_plan.
 */
int ia_tree_boxes(const void* sorted, int64_t F_usable, void* boxes, int64_t n_nodes, void* stream);
int ia_closest_point_tree(const float* points, int64_t N, const void* sorted, const int* order, int64_t F_usable, const void* boxes,
                          int64_t n_nodes, float mesh_extent, float* dist, int* face, float* point, int* counts, void* stream);

/*
 * Rays against the mesh on the cluster tree (csrc/ray_tree.hip; no counterpart in the reference; definition:
 * geometry._ray_mesh_numpy, the walk geometry._ray_tree_numpy).  Additive entry points: the ABI version is unchanged.
 *
 * Rays: origins and dirs float32 [N,3], t_lo and t_hi float32 [N] (the ray's own interval; +-inf allowed).  Per triangle, in fp32 with
 * every operation rounded on its own and dot products (x + y) + z, relative to the origin (a = A - o, ...): wa = d . (b x c),
 * wb = d . (c x a), wc = d . (a x b); inside = all three >= 0 or all three <= 0; n = (b - a) x (c - a), den = n . d, t = (n . a) / den.
 * The triangle is accepted iff inside, den != 0, t is finite, t_lo <= t <= t_hi and the point o + t d lies in the
 * triangle's own bounding box grown on every side by 2^-14 max(|o|_inf, |A|_inf, |B|_inf, |C|_inf) (without this clause the edge
 * functions accept, from far away, small triangles that the ray misses by any distance).  The test is NOT watertight: the signs of one
 * triangle are rounded separately, so a ray aimed at a shared edge or vertex can miss both neighbours.
 * first hit (any = 0): the smallest pair (t, input face index) over all accepted usable triangles: hit uint8 [N], t float32 [N],
 * face int32 [N] (order[sorted position]), bary float32 [N,3] = (wa, wb, wc) / ((wa + wb) + wc), point float32 [N,3] = o + t d.
 * No accepted triangle: 0 / +inf / -1 / NaN / NaN.  A ray with a non-finite origin or direction or a NaN interval end: 0 / NaN / -1 /
 * NaN / NaN.  any hit (any = 1): hit only; t, face, bary and point may be NULL and are not written.
 * ia_ray_mesh_brute: every ray against every sorted usable triangle (the triangles of ia_winding_tree_gather): the definition.
 * ia_ray_mesh_tree: the same bits by the walk of ia_closest_point_tree over the boxes of ia_tree_boxes, children in index order.  A
 * node is skipped iff a slab test on its box, grown on every side by s = 2^-12 M with M = max(|o|_inf, mesh_extent),
 * leaves no t in [t_lo, min(t_hi, best t)]: per axis t0 = ((lo - o) - s) (1 / d), t1 = ((hi - o) + s) (1 / d), every t when either is
 * a NaN, 1 / d overflowed for d != 0, or |t0|, |t1| or |1 / d| is below 2^-100; near = the largest min(t0, t1), far = the smallest max(t0, t1), each moved outward by the
 * factor 1 +- 2^-20; skipped iff near > far or near > min(t_hi, best t) or far < t_lo (a NaN compares false: entered).  In the any mode
 * a ray that has a hit tests nothing more.  counts (int32 [N,2], or NULL): boxes tested and ray-triangle pairs of the leaves entered.
 * N >= 0 with 3 N < 2^31, 0 <= F_usable <= 2^25, n_nodes that of ia_winding_tree_plan.
 * ia_ao_rays: for V vertices (verts, normals float32 [V,3], unit normals) and a table float32 [S,3] of local directions (z up), ray
 * v S + s: origin = v + bias n, direction = (t1 x + t2 y) + n z per component with sign = copysign(1, n.z), a = -1 / (sign + n.z),
 * b = (n.x n.y) a, t1 = (1 + ((sign n.x) n.x) a, sign b, -(sign n.x)), t2 = (b, sign + (n.y n.y) a, -n.y) (Duff et al. 2017).  A
 * non-finite normal gives NaN rays.  3 V S < 2^31, 1 <= S <= 65536.
 */
int ia_ray_mesh_brute(const float* origins, const float* dirs, const float* t_lo, const float* t_hi, int64_t N, const void* sorted,
                      const int* order, int64_t F_usable, int any, unsigned char* hit, float* t, int* face, float* bary, float* point,
                      void* stream);
int ia_ray_mesh_tree(const float* origins, const float* dirs, const float* t_lo, const float* t_hi, int64_t N, const void* sorted,
                     const int* order, int64_t F_usable, const void* boxes, int64_t n_nodes, float mesh_extent, int any,
                     unsigned char* hit, float* t, int* face, float* bary, float* point, int* counts, void* stream);
int ia_ao_rays(const float* verts, const float* normals, int64_t V, const float* table, int S, float bias, float* origins, float* dirs,
               void* stream);

/*
 * Texture atlas of a triangle mesh (csrc/texture.hip; no counterpart in the reference; definition: geometry.TextureAtlas,
 * atlas_points, project_texture and sample_texture with their NumPy restatements).  Additive entry points: the ABI
 * version is unchanged.  The texture is size x size texels (4 <= size <= 16384), texel (i, j) = column i, row j, stored [j][i]; faces
 * 2b and 2b + 1 share the square block b of side s >= 4 at ((b % G) s, (b / G) s), G = size / s, 2 G^2 >= F; L = s - 3.  Inside a
 * block the lower face owns li + lj <= s - 1 (corners (0, 0), (L, 0), (0, L)), the upper face li + lj >= s (corners (s-1, s-1),
 * (2, s-1), (s-1, 2)); every other texel is unowned.  fp32, every operation rounded on its own; all launches go to `stream`.
 *
 * ia_atlas_points: per texel face int32 (-1: unowned), bary float32 [3] = ((1 - l1) - l2, l1 = a / L, l2 = c / L) with (a, c) the
 * texel's offset from corner 0 along the two legs (negative l0 on the guard texels: extrapolated, not clamped), point float32 [3] =
 * (l0 A + l1 B) + l2 C and normal float32 [3]: the unit (B - A) x (C - A), or with normals float32 [V,3] their normalised mix; 0 for
 * a face whose cross product has no finite positive length or that indexes outside [0, V).  *degenerate (device int32) counts those
 * faces.  Unowned texels are 0 / -1.
 * ia_texture_project: for T texels (point, normal, face as above) and N <= 256 views: images float32 [N,H,W,C], C <= 8, cams float32
 * [N,25] (the last row of K is taken as [0, 0, 1]), depth float32 and mask uint8 [N,H,W] of ia_mesh_resolve.  A view passes a texel
 * if its projection (that of ia_mesh_project without the snap) is usable with u in [0, W - 1] and v in [0, H - 1], c = n . (o - X) /
 * |o - X| > min_cos, and at pixel (rint u, rint v) mask is set and ||o - X| - depth| <= depth_tol.  Its colour is the bilinear read of
 * the image at (u, v), its weight w = c^power (an integer power <= 64: the product ((c c) c) ...; any other: the fp32 rounding of the
 * double pow).  best = 0: texture = (float)(sum_k (double)(w colour) / sum_k (double)w) in view order, weight = (float)sum w;
 * best = 1: colour and weight of the largest w, the lowest view among equals.  views int32 = views passed, filled uint8 = views > 0;
 * a texel no view passes takes fallback float32 [T,C] (or 0 when NULL) and weight 0.
 * ia_texture_sample: out float32 [P,C] (C <= 64) = the bilinear read of texture float32 [size,size,C] at the uv mix
 * (b0 uv0 + b1 uv1) + b2 uv2 of the corners of face[p] (uv = (x + 0.5) / size), x = u size - 0.5 clamped into the face's block, so
 * that all four texels lie inside it; 0 where face[p] is outside [0, F).
 */
int ia_atlas_points(const float* verts, int64_t V, const int* faces, int64_t F, int size, int s, const float* normals, float* point,
                    int* face, float* bary, float* normal, int* degenerate, void* stream);
int ia_texture_project(const float* point, const float* normal, const int* face, int64_t T, const float* images, const float* cams, int N,
                       int H, int W, int C, const float* depth, const unsigned char* mask, float near, float min_cos, double power,
                       float depth_tol, int best, const float* fallback, float* texture, float* weight, int* views, unsigned char* filled,
                       void* stream);
int ia_texture_sample(const float* texture, int size, int C, int s, int64_t F, const int* face, const float* bary, int64_t P, float* out,
                      void* stream);

/*
 * LPIPS (csrc/lpips.hip): the three kernels the perceptual score needs besides the 3x3 MFMA convolutions.  Replaces, for evaluation,
 * encoder_inversion/criteria/lpips (lpips.py, networks.py, utils.py): torchvision feature stacks, normalize_activation, 1x1 linear
 * layers and spatial means.
 *
 * ia_conv2d_direct: y[n,o,oy,ox] = act(bias[o] + sum_{i,ky,kx} w[o,i,ky,kx] * x[n,i,oy*stride - pad + ky, ox*stride - pad + kx]) with
 * zeros outside the image; act = IA_ACT_RELU (v < 0 ? 0 : v) or IA_ACT_LINEAR.  x [N,I,H,W], w [O,I,k,k] (the module's own layout),
 * bias [O] or NULL, y [N,O,OH,OW] with OH = (H + 2 pad - k) / stride + 1 (floor), all fp32.  1 <= k <= 11, stride 1 or 4,
 * 0 <= pad < k, any channel counts, any H x W with OH, OW >= 1, N <= 65535.  fp32 fused multiply-adds in the order (i, ky, kx) within
 * blocks of max(1, min(16, 144 / k^2)) input channels, whose sums are added in block order: the same bits run to run and for any batch.
 *
 * ia_maxpool2d: y[n,c,oy,ox] = max over the k x k window at (oy*stride, ox*stride), no padding, floor mode: OH = (H - k) / stride + 1.
 * (k, stride) = (3, 2) or (2, 2).  The maximum is taken in row-major window order with `v > m || v != v`, torch.max_pool2d's rule: the
 * results are its bits on finite inputs (and NaN propagates).  y fp32 [N,C,OH,OW] or NULL; ys or NULL: the same values in the split
 * format of ia_act_split (ys_planes = 1 or 2, C % 8 == 0, styles = 1), for a 3x3 MFMA convolution behind the pool.  One of y / ys.
 *
 * ia_lpips_layer: one tap of a batch of N pairs.  f fp32 [2N,C,h,w]: maps n and N + n are the two images of pair n.  At every pixel
 *     fx^_c = fx_c / (sqrt(sum_c fx_c^2) + 1e-10),  fy^ likewise (fp32; the sum of squares in channel order),
 *     d = sum_c (double)lin[c] * (double)(fx^_c - fy^_c)^2   (the difference is formed in fp32 and squared in double, channel order),
 * out[n * out_stride] = (float)(sum over the pixels of d / (h w)).  A thread owns a pixel; a workgroup adds its 256 pixels in double
 * (xor tree in each wave, then the waves in order) into its slot of `scratch`, and a finalising launch adds a frame's slots
 * lane-strided + xor tree: no floating-point atomics.  Identical maps give exactly 0, exchanging the halves of f gives the same bits,
 * a pair's value does not depend on N, and the same inputs give the same bits.  lin [C]; scratch: ia_lpips_layer_scratch_bytes(N, h, w)
 * bytes, 8-byte aligned; N <= 65535.
 */
int ia_conv2d_direct(const float* x, const float* w, const float* bias, float* y, int N, int I, int O, int H, int W, int k, int stride,
                     int pad, int act, void* stream);
int ia_maxpool2d(const float* x, float* y, void* ys, int ys_planes, int N, int C, int H, int W, int k, int stride, void* stream);
int ia_lpips_layer_scratch_bytes(int N, int h, int w, size_t* h_bytes);
int ia_lpips_layer(const float* f, const float* lin, int N, int C, int h, int w, void* scratch, size_t scratch_bytes, float* out,
                   int out_stride, void* stream);

/*
 * Identity similarity (csrc/identity.hip): what the ArcFace IR-SE50 score of encoder_inversion/criteria/id_loss.py (IDLoss) needs besides
 * the residual units on ia_conv2d_mfma_sx / ia_conv2d_down_sx / ia_se_gate.  Additive entry points: the ABI version is unchanged.
 *
 * ia_face_crop_pool: images fp32 [N,3,H,W] (IA_IMAGE_F32_NCHW) or uint8 [N,H,W,3] (IA_IMAGE_U8_NHWC, read as v / 127.5 - 1), H, W >= 256
 * -> y fp32 [N,3,112,112] = AdaptiveAvgPool2d(112)(AdaptiveAvgPool2d(256)(images)[:, :, 35:223, 32:220]); a 256 x 256 frame skips the
 * first pool.  Windows are torch's, [floor(i In / Out), ceil((i + 1) In / Out)); each stage is the fp32 sum of its window in row-major
 * order divided by the window's size.
 *
 * ia_prelu_channels: y = x < 0 ? x * slopes[c] : x on fp32 [B,C,P] (y may be x).
 *
 * ia_conv3x3_small: y[b,o] = prelu(out_scale[o] * sum_{i,ky,kx} wk[ky*3+kx][i][o] * pad0(in_scale[i] * x[b,i] + in_shift[i]) + out_shift[o])
 * for h, w in 1..7, I % 8 == 0, O % 8 == 0: stride 1, and the zero padding is applied AFTER the input affine map (a BatchNorm in front
 * of the convolution).  x [B,I,h,w], wk [9][I][O] (hipops.pack_conv_weight), y [B,O,h,w], all fp32; in_scale / in_shift [I] (both or
 * neither), out_scale / out_shift / slopes [O] or NULL.  fp32 fused multiply-adds: blocks of 8 input channels (72 terms in the order
 * i, ky, kx) summed on their own, four blocks per chunk of 32 channels, one workgroup per chunk; the chunks' sums are added in chunk
 * order by a second launch (no floating-point atomics).  The split depends on I alone: an image's result is the same in any batch.
 * scratch: ia_conv3x3_small_scratch_bytes(B, I, O, h, w) bytes.  B <= 65535.
 *
 * ia_id_head: out[b] = z / ||z||_2 with z[o] = (sum_k wt[o][k] * x[b][k] + bias[o]) * scale[o] + shift[o]; x [B,K], wt [O,K], bias / scale /
 * shift [O] or NULL, out [B,O], fp32.  The BatchNorm2d in front of the reference's Linear is folded into wt and bias by the caller (no
 * padding is involved), scale / shift are its BatchNorm1d.  K is cut into slices of 3136: a thread adds k = t, t + 256, ... of a slice in
 * fp32, a workgroup's 256 sums go through an xor tree per wave and the waves in order, the slices are added in order; ||z|| is the
 * fp32 root of the squares summed in double the same way.  A zero z gives NaN (0 / 0), as torch.div does.
 * scratch: ia_id_head_scratch_bytes(B, K, O) bytes.
 *
 * ia_id_similarity: out[n * out_stride] = sum_d f[n][d] * f[N + n][d] over f [2N,D] fp32: fp32 products added in double, lane-strided over
 * one wave and an xor tree.  Exchanging the halves of f gives the same bits; a pair's value does not depend on N.
 */
int ia_face_crop_pool(const void* images, int layout, float* y, int N, int H, int W, void* stream);
int ia_prelu_channels(const float* x, const float* slopes, float* y, int B, int C, int64_t P, void* stream);
int ia_conv3x3_small_scratch_bytes(int B, int I, int O, int h, int w, size_t* h_bytes);
int ia_conv3x3_small(const float* x, const float* wk, const float* in_scale, const float* in_shift, const float* out_scale,
                     const float* out_shift, const float* slopes, float* y, void* scratch, size_t scratch_bytes, int B, int I, int O,
                     int h, int w, void* stream);
int ia_id_head_scratch_bytes(int B, int K, int O, size_t* h_bytes);
int ia_id_head(const float* x, const float* wt, const float* bias, const float* scale, const float* shift, float* out, void* scratch,
               size_t scratch_bytes, int B, int K, int O, void* stream);
int ia_id_similarity(const float* f, int N, int D, float* out, int out_stride, void* stream);

/*
 * Contextual loss (csrc/contextual.hip): what the CX score of encoder_inversion/criteria/cx_loss.py (CXLoss, contextual_loss with the
 * cosine distance) needs besides the VGG19 trunk on ia_conv2d_direct / ia_maxpool2d / ia_conv2d_mfma_sx.  Additive entry points: the
 * ABI version is unchanged.
 *
 * ia_resize_bilinear: F.interpolate(mode='bilinear', align_corners=False), no antialiasing, any sizes.  src fp32 [N,C,H,W]
 * (IA_IMAGE_F32_NCHW) or uint8 [N,H,W,C] (IA_IMAGE_U8_NHWC, read as v / 127.5 - 1) -> dst fp32 [N,C,OH,OW].  Per axis the source
 * coordinate is s = max(0, (In / Out)(o + 0.5) - 0.5) in double, the taps floor(s) and min(floor(s) + 1, In - 1), the weights
 * w1 = fp32(s - floor(s)), w0 = 1 - w1; dst = wy0 (wx0 v00 + wx1 v01) + wy1 (wx0 v10 + wx1 v11) in fp32.  H == 2 OH and W == 2 OW take a
 * branch with the constant taps (2 o, 2 o + 1) and weights 0.5 -- the 2 x 2 mean, the same bits; general != 0 forces the general path.
 *
 * The head, for N pairs of maps fx, fy fp32 [N,C,P] (P = h w positions) and a table mu of per-channel shifts:
 *     x^_i = (fx_i - mu) / max(||fx_i - mu||_2, 1e-12),  y^_j likewise;   d_ij = 1 - x^_i . y^_j;   m_i = min_j d_ij;
 *     w_ij = exp((1 - clamp(d_ij / (m_i + 1e-5), -10, 10)) / band_width);   s_i = sum_j w_ij;
 *     colmax_j = max_i w_ij / s_i;   cx = (sum_j colmax_j) / P;   cx_loss = -log(cx + 1e-5).
 * ia_cx_layout: tile = rows / columns per workgroup of ia_cx_rows / ia_cx_cols, k_step = the multiple the channel count is padded to.
 * ia_cx_scratch_bytes(N, C, P): bytes for the double [N,C] means, float [N,P] m, double [N,P] s and double [N,P] colmax -- O(N (C + P));
 * the P x P matrix is never stored.  The operands x^, y^ (fp32 [N,P,Cpad] each) are the caller's.
 * ia_cx_channel_mean: mean64[n,c] = (sum_p f[n,c,p]) / P in double (a workgroup per map: lane-strided partials, xor tree per wave, waves
 * in order), mu_frames [N,C] = fp32 of it; mu_batch [C] or NULL = fp32((sum_n mean64[n,c]) / N), frames in order.  No atomics.
 * ia_cx_normalize: f [N,C,P], mu [mu_rows,C] with mu_rows = 1 (one row for the batch) or N -> out [N,P,Cpad], Cpad % k_step == 0, zeros
 * from channel C on.  The difference is fp32, the squared norm is added in double in channel order, the norm rounded to fp32 and the
 * quotient fp32; a NaN norm stays NaN.
 * ia_cx_rows: m [N,P] and s [N,P].  ia_cx_cols: colmax [N,P] from the same operands and that m, s.  Both form the dot products with
 * v_mfma_f32_16x16x4_f32 (x^ as A, y^ as B), 16 channels per fp32 accumulator, the accumulators added in double in channel order, and
 * d = fp32(1 - dot): the same bits of d in both.  t, w and the sums are double.  s_i adds a lane's columns in order and 16 lanes by the
 * xor tree; minima and maxima propagate NaN.  Cpad <= 624 (a 64-row block in LDS), else IA_ERR_UNSUPPORTED; N <= 65535.
 * ia_cx_finish: cx [N] = fp32((sum_j colmax_j) / P) (one wave per frame: lane-strided double partials, xor tree), cx_loss [N] =
 * fp32(-log of the double + 1e-5).  A frame's results depend on its two maps and its mu row alone: the same bits in any batch and run.
 */
int ia_resize_bilinear(const void* src, int layout, float* dst, int N, int C, int H, int W, int OH, int OW, int general, void* stream);
int ia_cx_layout(int* tile, int* k_step);
int ia_cx_scratch_bytes(int N, int C, int64_t P, size_t* h_bytes);
int ia_cx_channel_mean(const float* f, int N, int C, int64_t P, double* mean64, float* mu_frames, float* mu_batch, void* stream);
int ia_cx_normalize(const float* f, const float* mu, int mu_rows, float* out, int N, int C, int64_t P, int cpad, void* stream);
int ia_cx_rows(const float* xh, const float* yh, int N, int64_t P, int cpad, float band_width, float* m, double* s, void* stream);
int ia_cx_cols(const float* xh, const float* yh, const float* m, const double* s, int N, int64_t P, int cpad, float band_width,
               double* colmax, void* stream);
int ia_cx_finish(const double* colmax, int N, int64_t P, float* cx, float* cx_loss, void* stream);

/* ---- non-rigid fitting of a template mesh (csrc/nonrigid.hip; the definition is geometry.nonrigid_align) ----
 * The unknown is one displacement d_i (double) per template vertex x_i (float32 [V,3]); V <= 2^28.
 * ia_nonrigid_terms: the terms of one pairing.  p = fl32(x + d), (dist, face, q) its closest points on the target.  Pair i counts iff
 * dist[i] is finite, face[i] >= 0, dist[i] <= h_max_dist (fp32; +inf: none), pinned[i] == 0, for mode 1 (plane) or use_cos face[i] < Fb
 * with a finite non-zero normal in face_normals [Fb,3], and with use_cos source_normals[i] finite, non-zero and
 * source_normals[i] . face_normals[face[i]] >= normal_cos (in double).  Writes c [V] (1 | 0), n [V,3] (the face normal for a counting
 * pair of mode 1, else 0) and b [V,3] = c (q - x) (mode 0) or c (n (n . (q - x)) + point_share (q - x)) (mode 1), plus beta[i] land[i]
 * where beta (double [V], or NULL) is not 0 and the vertex not pinned; out[0] = sum c |p - q|^2, out[1] = sum c, in double: per
 * workgroup of 256 vertices the butterfly per wave and the waves in order, the workgroups by a second launch in one fixed order.
 * scratch: ia_nonrigid_terms_scratch_bytes(V) bytes.
 * ia_nonrigid_rhs: b from weights c [V], offsets t [V,3], normals n [V,3] (NULL: point), beta / land (or NULL) by the same formulas
 * (an offset with weight 0 is not read into b; pinned rows are 0).
 * ia_nonrigid_solve: conjugate gradients in double on (C + a L + B) x = b from x (in / out, [V,3]; 0 at pinned vertices), for exactly
 * cg_iterations steps of three launches each (four with heavy vertices), no host synchronisation: (L x)_i = deg_i x_i - sum_j x_j over
 * the CSR row (offsets [V+1], neighbors [E]) in ascending j, vertices of degree > 64 (heavy [n_heavy]) by one wave each; C_i = c_i I
 * (n NULL) or c_i (n_i n_i^T + point_share I); B_i = beta_i I; pinned rows and columns are taken out.  Once |r|^2 <= cg_tol^2 |b|^2, or
 * p.Ap <= 0, or a scalar is not finite, every later step changes nothing.  out [5] (device): the energy 1/2 x.Ax - b.x at the start and
 * at the end, the steps taken, |r| / |b|, the freeze flag.  Dot products are per-workgroup partials added again by every workgroup of
 * the next launch in one fixed order: no floating-point atomics, bit-equal run to run.  scratch: ia_nonrigid_solve_scratch_bytes(V).
 * ia_nonrigid_apply: verts[i] = x[i] where pinned or d[i] == 0 (per coordinate), else fl32(x[i] + d[i]).
 */
int ia_nonrigid_terms_scratch_bytes(int64_t V, size_t* h_bytes);
int ia_nonrigid_terms(const float* x, const float* p, const float* q, const float* dist, const int* face, int64_t V,
                      const float* face_normals, int64_t Fb, const float* source_normals, float h_max_dist, int mode, int use_cos,
                      double normal_cos, double point_share, const unsigned char* pinned, const double* beta, const double* land,
                      double* c, double* n, double* b, void* scratch, size_t scratch_bytes, double* out, void* stream);
int ia_nonrigid_rhs(int64_t V, const double* c, const double* t, const double* n, double point_share, const double* beta,
                    const double* land, const unsigned char* pinned, double* b, void* stream);
int ia_nonrigid_solve_scratch_bytes(int64_t V, size_t* h_bytes);
int ia_nonrigid_solve(int64_t V, const int* offsets, const int* neighbors, int64_t E, const int* heavy, int n_heavy, const double* c,
                      const double* n, const double* beta, const unsigned char* pinned, const double* b, double stiffness,
                      double point_share, double* x, int cg_iterations, double cg_tol, void* scratch, size_t scratch_bytes,
                      double* out, void* stream);
int ia_nonrigid_apply(const float* x, const double* d, const unsigned char* pinned, int64_t V, float* verts, void* stream);

/* ---- a set of frames as a distribution (csrc/distribution.hip; the definitions are in distribution_metrics.py) ----
 * All four work on feature sets, float32 [rows, D] row-major and contiguous.  No floating-point atomics: the same call gives the same bits.
 * ia_feature_moments: sum [D] += sum_r x[r,:] and cov [D,D] += sum_r x[r,:] x[r,:]^T for the n rows of one chunk, in double (the
 * products of float32 values are exact in double).  One wave owns a 32 x 32 block of the lower triangle, adds the rows in order, four per
 * v_mfma_f64_16x16x4_f64, and writes the block and its mirror: cov stays symmetric bit for bit.  1 <= D <= 4096; n = 0 does nothing.
 * sum and cov are read and written: the caller zeroes them before the first chunk.
 * ia_kid_subsets: for subset s with rows x_i = gen[idx_gen[s,i]], y_i = real[idx_real[s,i]] (i < m; the indices must be in range, the
 * kernel does not know the sets' sizes) and k(u, v) = (u . v / D + 1)^3:
 *     out[s,0] = sum_{i != j} k(x_i, x_j),  out[s,1] = sum_{i != j} k(y_i, y_j),  out[s,2] = sum_{i,j} k(x_i, y_j).
 * i != j is by position in the subset.  The dot products are fp32 (v_mfma_f32_32x32x2_f32, channels in ascending order); the division,
 * the cube (t t) t and the sums are double: a lane adds its elements in order, a wave its 128 x 128 tiles in order (an off-diagonal
 * tile of a symmetric block counts twice), then the butterfly and the four waves in order.  A subset's three numbers depend on its rows
 * alone: the same bits for any S and any position in the call.
 * ia_knn_radius: r2[j] = the (k + 1)-th smallest of d2(j, i) over all i < N, i = j included and duplicates counted; 0 <= k <= 15, N > k.
 * ia_manifold_covered: covered[p] = 1 iff d2(probe p, manifold j) <= r2[j] for some j < N, else 0.
 * In both d2(a, b) = sum_c (a_c - b_c)^2 in the difference form: the difference rounded to fp32, then fmaf into the sum, c ascending.
 */
int ia_feature_moments(const float* x, int64_t n, int D, double* sum, double* cov, void* stream);
int ia_kid_subsets(const float* gen, const float* real, int D, const int* idx_gen, const int* idx_real, int S, int m, double* out,
                   void* stream);
int ia_knn_radius(const float* feat, int64_t N, int D, int k, float* r2, void* stream);
int ia_manifold_covered(const float* probes, int64_t P, const float* manifold, const float* r2, int64_t N, int D, unsigned char* covered,
                        void* stream);

/*
 * Point clouds on the cluster tree: k nearest points and normals (csrc/point_tree.hip; no counterpart in the reference; definitions:
 * geometry._nearest_numpy, _nearest_tree_numpy, _point_tree_numpy and _point_normals_numpy).  Additive entry points:
 * the ABI version is unchanged.
 *
 * The tree is the level layout of ia_winding_tree_plan over points: the usable (finite) points in the stable ascending order of
 * ia_winding_tree_point_keys (cube: the box of the usable points), L points per leaf, B nodes per parent.
 * ia_point_tree_gather: sorted float4 [n_usable] with sorted[s] = (points[order[s]].xyz, the bits of the int32 order[s]).
 * ia_point_tree_boxes: the rows of ia_tree_boxes over the sorted points: exact min / max, bit-equal run to run.
 * ia_nearest_points_brute: for queries float32 [N,3], dist float32 [N,k] and index int32 [N,k] (input indices).  In fp32 with every
 * operation rounded on its own, d2 = (dx dx + dy dy) + dz dz with dx = x.x - p.x, ...; the result is the k smallest pairs (d2, index)
 * over all usable points other than exclude[i] (int32 [N], or NULL), ascending; dist = sqrt(d2), correctly rounded.  A place is
 * +inf / -1 where the cloud has no further point or dist > max_dist (+inf: no limit), and throughout for a non-finite query.
 * ia_nearest_points_tree: the same bits by the walk of ia_closest_point_tree.  A node is skipped iff lb > the lane's k-th d2 (strictly;
 * +inf while the list is not full), lb = the expression of d2 on g = max(lo - p, 0, p - hi) per axis: rounding is monotone, so
 * lb <= d2 of every point of the box and no margin is needed.  counts (int32 [N,2], or NULL): boxes tested and leaves taken, the first
 * descent included.  1 <= k <= 32 (lists of 1, 4, 8, 16 or 32 places in registers; k is rounded up, which changes no bit),
 * N >= 0 with 3 N < 2^31 and N k < 2^31, 0 <= n_usable <= 2^25, n_nodes that of ia_winding_tree_plan.
 * ia_point_normals: for points float32 [n,3] and index int32 [n,k] (ia_nearest_points_*; entries outside [0, n) are left out), per
 * point in double: the mean of the neighbours added in order, the covariance (xx xy xz yy yz zz) of the differences added in order and
 * divided by their number m, and its eigen-decomposition by 8 cyclic Jacobi sweeps over (0,1) (0,2) (1,2).  eigenvalues double [n,3]
 * ascending, covariance double [n,6], normal float32 [n,3] = the unit eigenvector of the smallest, its largest-magnitude component
 * positive, variation float32 [n] = l0 / ((l0 + l1) + l2); normal and variation are 0 where m < 3 or the trace is not positive.
 * One thread per point, no atomics: bit-equal run to run.
 */
int ia_point_tree_gather(const float* points, int64_t n, const int* order, int64_t n_usable, void* sorted, void* stream);
int ia_point_tree_boxes(const void* sorted, int64_t n_usable, void* boxes, int64_t n_nodes, void* stream);
int ia_nearest_points_brute(const float* queries, int64_t N, const void* sorted, int64_t n_usable, int k, float max_dist,
                            const int* exclude, float* dist, int* index, void* stream);
int ia_nearest_points_tree(const float* queries, int64_t N, const void* sorted, int64_t n_usable, const void* boxes, int64_t n_nodes,
                           int k, float max_dist, const int* exclude, float* dist, int* index, int* counts, void* stream);
int ia_point_normals(const float* points, int64_t n, const int* index, int k, float* normal, float* variation, double* eigenvalues,
                     double* covariance, void* stream);

/*
 * TSDF integration: depth maps fused into a truncated signed distance lattice (csrc/tsdf.hip; no counterpart in the reference;
 * definition: geometry._fuse_numpy).  An additive entry point: the ABI version is unchanged.
 *
 * depth float32 [N,H,W] (the ray parameter of the pixel's unit ray), mask uint8 [N,H,W] or NULL, weights float32 [N,H,W] or NULL,
 * colors float32 [N,C,H,W] (NULL exactly when C = 0), views float32 [N,18]: per view the rotation row-major (9), the origin (3) and
 * rows 0 and 1 of K_res (row 0 of K times W, row 1 times H; pixel centres at integer coordinates).  The lattice is that of ia_mc_*:
 * point (i, j, k) at h_lo + index * h_step in fp32, z fastest.  Per lattice point X, over the views in order, fp32 with every
 * operation rounded on its own: d = X - o, xc_a = (R_0a d_x + R_1a d_y) + R_2a d_z; u = ((k0 xc_x + k1 xc_y) + k2 xc_z) / xc_z,
 * v likewise with k3 .. k5; i = rint(u), j = rint(v) (ties to even); t = depth[n,j,i], w = weights[n,j,i] or 1;
 * s = t - sqrt((d_x d_x + d_y d_y) + d_z d_z).  The view is skipped unless xc_z is finite and > near, u and v are finite,
 * 0 <= i <= W - 1 and 0 <= j <= H - 1 (compared as floats), t is finite and > 0, the mask is set, w is finite and > 0 and
 * s >= -truncation.  Otherwise sum += min(s / truncation, 1) w and weight += w, and where s <= truncation color_sum[c] +=
 * colors[n,c,j,i] w per channel and color_weight += w.  Outputs float32: sum, weight, tsdf = sum / weight (1 where weight is not > 0)
 * [nx,ny,nz], color_sum [nx,ny,nz,C] and color_weight [nx,ny,nz] (C > 0).  accumulate != 0: the sums start from the contents of the
 * output arrays instead of 0, so views [0, N) in one call give the bits of [0, k) followed by [k, N).  One thread per lattice point,
 * no atomics: bit-equal run to run.  N >= 1, 0 <= C <= 8, 1 <= H, W <= 16384, truncation > 0, near >= 0.
 */
int ia_tsdf_integrate(const float* depth, const unsigned char* mask, const float* weights, const float* colors, const float* views, int N,
                      int C, int H, int W, int nx, int ny, int nz, const float* h_lo, const float* h_step, float truncation, float near,
                      int accumulate, float* sum, float* weight, float* tsdf, float* color_sum, float* color_weight, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* IA_HIP_H_ */
