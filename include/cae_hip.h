/* libcae_hip.so -- C ABI of the MI355X-native compress/decompress hot path.
 *
 * The reference (TheJacksonLaboratory/cnn_autoencoder) is pure Python: it has no FFI of its
 * own.  Its native code on this path lives in the third-party package `compressai`
 * (C++ pybind11: `_CXX.pmf_to_quantized_cdf`, `ans.RansEncoder/RansDecoder`) and in the
 * ATen/cuDNN kernels behind `nn.Conv2d` / `nn.ConvTranspose2d` / `GDN`.  Each entry point
 * below names the reference interface (file:line under /root/reference/src) it replaces;
 * INTEGRATION.md shows the ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - every function returns 0 on success, a negative cae_status otherwise;
 *     cae_last_error() returns a thread-local message for the last failure;
 *   - `*_dev` pointers are DEVICE pointers (HBM) of the current HIP device, `stream` is a
 *     hipStream_t passed as void* (NULL = default stream); all launches are asynchronous;
 *   - `*_host` pointers are host memory;
 *   - outputs are caller-allocated, except the variable-length bitstreams returned by
 *     cae_rans_encode_batch (library-allocated, release with cae_free);
 *   - a model handle may be used from several host threads (dask's threaded scheduler calls
 *     codec.encode concurrently, compress.py:121-128): entry points taking a handle
 *     serialise on a per-handle mutex.
 *   - no torch types anywhere in this ABI.
 */
#ifndef CAE_HIP_H
#define CAE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cae_model cae_model_t;

enum cae_status {
    CAE_OK = 0,
    CAE_ERR_ARG = -1,      /* bad argument (the reference raises ValueError) */
    CAE_ERR_HIP = -2,      /* HIP runtime failure */
    CAE_ERR_NOMEM = -3,
    CAE_ERR_UNSUPPORTED = -4,
    CAE_ERR_CORRUPT = -5,  /* bitstream ran past its end */
    CAE_ERR_RANGE = -6     /* cae_seg_range_check: the call left the valid range of f16x3, its results are invalid */
};

enum cae_track { CAE_ANALYSIS = 0, CAE_SYNTHESIS = 1 };
enum cae_pixfmt {
    CAE_FMT_U8_HWC = 0,  /* (n,h,w,c) uint8  -- zarr chunk layout, compress.py:101 */
    CAE_FMT_F32_NCHW = 1 /* (n,c,h,w) float  -- nn.Module call surface */
};

int cae_version(void);
const char *cae_last_error(void);
void cae_free(void *p);

/* ---- model lifecycle ------------------------------------------------------------------
 * Replaces setup_modules / load_state_dict (_autoencoders.py:458-502): the Python side reads
 * the checkpoint dict and hands every layer's tensors over in the reference's own layouts. */
int cae_model_create(int channels_org, int channels_net, int channels_bn, int compression_level,
                     int kernel_size, cae_model_t **out);
void cae_model_destroy(cae_model_t *m);

/* One unit of a track: strided conv (analysis; DownsamplingUnit model.0, _autoencoders.py:78-85;
 * weight (cout,cin,k,k)) or transposed conv (synthesis; UpsamplingUnit model.0, :204-211;
 * weight (cin,cout,k,k)), optional bias (cout), optional GDN/IGDN (model.1, :29-30) given as
 * the EFFECTIVE (re-parametrised, non-negative) beta (cout) and gamma (cout,cout). */
int cae_model_set_layer(cae_model_t *m, int track, int index, int cin, int cout,
                        const float *weight_host, const float *bias_host,
                        const float *beta_eff_host, const float *gamma_eff_host);

/* LeakyReLU / ReLU variants of a unit (DownsamplingUnit _autoencoders.py:62-76,90-92; UpsamplingUnit
 * :187-202,216-218): `act` (0 none, 1 LeakyReLU(0.01), 2 ReLU) is applied after the layer's strided
 * (transposed) convolution; when pre_weight_host is given, a stride-1 convolution cin -> cin (analysis:
 * weight (cin,cin,k,k), reflect padding; synthesis: ConvTranspose2d weight (cin,cin,k,k), padding k//2)
 * plus the same activation runs in front of it.  Call after cae_model_set_layer for the same index.
 * Both arithmetic paths (f16x3: the same split-f16 kernels with stride 1 / the activation in the store epilogue). */
int cae_model_set_layer_act(cae_model_t *m, int track, int index, int act, const float *pre_weight_host,
                            const float *pre_bias_host);

/* Arithmetic of the conv / GDN contraction: 0 = exact fp32 MFMA (v_mfma_f32_32x32x2_f32),
 * 1 = "f16x3": every operand split into two f16 halves, three f16 MFMAs per product, fp32
 * accumulate (same 1e-4 parity bar, ~5x less matrix-pipe time).  Set before
 * cae_model_set_layer.  (No reference counterpart: the reference computes in fp32 on ATen,
 * _autoencoders.py:78-85, :204-211.)
 *
 * ACCURACY of f16x3.  A value v is carried as hi = f16(v), lo = f16(v - hi):
 *   |v - (hi + lo)| <= max(2^-22 |v|, 2^-25).
 * lo falls below the smallest normal f16 (2^-14) as soon as |v| < 2^-3, and is then rounded to a multiple of 2^-24:
 * the relative accuracy is 2^-22 at |v| = 0.25 but 2^-17.4 at 0.01 and 2^-14 at 1e-3.  Typical convolution weights
 * (|w| ~ 0.01-0.05) and most of gamma lie in that band.  A product a b is ah bh + ah bl + al bh (the dropped al bl
 * is below 2^-22 |a b|); the sums accumulate in fp32.  (tests/test_inference_kernels.py pins this model.)
 *
 * VALID RANGE of f16x3.  f16 has 5 exponent bits, so the split format holds finite values with
 * |v| <= 65504, at the accuracy above.
 *   - weights / gamma outside that range: cae_model_set_layer marks the model and every call runs on the
 *     fp32 kernels (cae_model_effective_precision reports 0);
 *   - GDN / IGDN squares: formed from y scaled per pixel by a power of two (largest |y| of the pixel's
 *     channels brought into [64,128)), beta and the result rescaled exactly: any finite pre-GDN magnitude
 *     is in range; accuracy is 2^-22 relative to the pixel's largest channel;
 *   - activations between layers, latents into the synthesis track and float inputs: a value with
 *     |v| > 65504 (or NaN) cannot be stored.  Every kernel that writes the split format then raises the
 *     call's overflow word, and the results of that call are INVALID.  Protocol: after the call, on the
 *     same host thread, t = cae_last_range_ticket(); once the stream work of the call has completed
 *     (stream / event synchronise), cae_range_check(m, t, &over); if over, repeat the call between
 *     cae_thread_force_fp32(1) / (0): it then runs on the exact-fp32 kernels (fp32 range, as the reference).
 *     The Python modules do this automatically.  1024 calls per handle are tracked. */
int cae_model_set_precision(cae_model_t *m, int precision);
int64_t cae_last_range_ticket(void);         /* thread-local; 0 = the call ran on the fp32 kernels: nothing to check */
int cae_range_check(cae_model_t *m, int64_t ticket, int *overflowed);
void cae_thread_force_fp32(int on);          /* thread-local: calls of this thread use the fp32 kernels */
int cae_model_effective_precision(cae_model_t *m, int *precision);

/* Integer tables of the factorized entropy model, as EntropyBottleneck.update() leaves them
 * (_autoencoders.py:502): quantized_cdf (channels, cdf_stride) int32, cdf_length (channels),
 * offset (channels), medians (channels) float. */
int cae_model_set_entropy(cae_model_t *m, int channels, int cdf_stride, const int32_t *quantized_cdf_host,
                          const int32_t *cdf_length_host, const int32_t *offset_host,
                          const float *medians_host);

/* ---- device hot path --------------------------------------------------------------------
 * cae_analysis replaces Analyzer.forward (_autoencoders.py:359-361) including the uint8 ->
 * float/255 conversion of ConvolutionalAutoencoder.encode (:542-545) when fmt is U8_HWC.
 * latents_dev: (n, channels_bn, ceil(h/2^L), ceil(w/2^L)) float NCHW. */
int cae_analysis(cae_model_t *m, const void *tiles_dev, int fmt, int n, int h, int w,
                 float *latents_dev, void *stream);

/* cae_analysis that also writes the output of every unit i < compression_level-1 for which levels_dev[i] is not NULL:
 * (n, cout_i, ceil(h/2^(i+1)), ceil(w/2^(i+1))) float NCHW, the values the next unit reads (f16x3: exactly hi + lo of
 * the stored split value).  levels_dev may be NULL.  The kernels and the latents are the same as cae_analysis's.
 * Every call of the analysis entry points returns CAE_ERR_ARG when a reflect-padded convolution would see an input
 * of k//2 rows or columns or fewer (F.pad(mode='reflect') rejects it, as the reference does). */
int cae_analysis_levels(cae_model_t *m, const void *tiles_dev, int fmt, int n, int h, int w, float *latents_dev,
                        float *const *levels_dev, void *stream);

/* cae_synthesis replaces Synthesizer.forward (_autoencoders.py:442-455) and, for U8_HWC, the
 * x*255 -> clip -> truncating uint8 -> HWC epilogue of ConvolutionalAutoencoder.decode
 * (:576-580).  latents_dev (n, channels_bn, lh, lw) float NCHW; output (n, ., lh*2^L, lw*2^L).
 * bridges_dev: NULL, or an array of compression_level-1 device pointers that receive the
 * intermediate features fx_brg[i] (n, channels_net, lh*2^(i+1), lw*2^(i+1)) float NCHW. */
int cae_synthesis(cae_model_t *m, const float *latents_dev, int n, int lh, int lw,
                  void *out_dev, int fmt, float *const *bridges_dev, void *stream);

/* Residual units (ResidualDownsamplingUnit / ResidualUpsamplingUnit, _autoencoders.py:104-174, :230-304) and, in
 * general, the stride-1 (transposed) convolutions cin -> cin in front of a unit's strided layer.  Stage `stage`
 * (0 or 1) computes  y = post_act( act_or_gdn(conv(x_stage)) [+ unit input] ):  w (cin,cin,k,k) with bias or NULL
 * (BatchNorm folded by the caller), beta/gamma = effective GDN parameters of that stage or NULL, act / post_act as
 * in cae_model_set_layer_act.  cae_model_set_layer_act clears the stages of its layer (and creates stage 0 from
 * its pre-convolution), so call it first.  Precision 1 (f16x3): GDN / residual stages up to 128 channels run
 * on conv_s2_f16_kernel<.., S = 1, RES>; the stages of a wider unit run on the fp32 kernels between two layout
 * conversions (the strided layers stay on f16x3). */
int cae_model_set_layer_stage(cae_model_t *m, int track, int index, int stage, const float *w, const float *bias,
                              const float *beta, const float *gamma, int act, int add_residual, int post_act);

/* Multiscale colour layers (Synthesizer(multiscale_analysis=True), _autoencoders.py:417-436): a stride-1 reflect
 * convolution from the output of synthesis level `index` (< compression_level-1) to the image channels.
 * w: (cout, cin, k, k).  cae_synthesis_multiscale additionally writes colors_dev[i] (n, cout, lh*2^(i+1),
 * lw*2^(i+1)) float NCHW for every non-NULL entry: the reference's x_r[compression_level-1-i]
 * (_autoencoders.py:446-452).  Precision 1 (f16x3): colour layers to at most 32 channels; wider: precision 0.
 * A requested colour layer whose level is k//2 rows or columns or fewer (reflect padding) is CAE_ERR_ARG. */
int cae_model_set_color_layer(cae_model_t *m, int index, int cin, int cout, const float *w, const float *bias);
int cae_synthesis_multiscale(cae_model_t *m, const float *latents_dev, int n, int lh, int lw, void *out_dev, int fmt,
                             float *const *bridges_dev, float *const *colors_dev, void *stream);

/* Fused forms of the codec path (encode: _autoencoders.py:542-551, decode: :568-580): the quantiser runs in the
 * epilogue of the last analysis layer (symbols (n, channels_bn, lh, lw) int32 instead of float latents) and the
 * dequantiser in the layout conversion in front of the first synthesis layer.  Same results as
 * cae_analysis + cae_quantize / cae_dequantize + cae_synthesis; the handle needs cae_model_set_entropy (medians). */
int cae_analysis_symbols(cae_model_t *m, const void *tiles_dev, int fmt, int n, int h, int w, int32_t *symbols_dev,
                         void *stream);
int cae_synthesis_symbols(cae_model_t *m, const int32_t *symbols_dev, int n, int lh, int lw, void *out_dev, int fmt,
                          void *stream);

/* Synthesis that stops at a level: the image at 1 / 2^scale of the resolution.  With L = compression_level, units
 * 0 .. L-1-scale run, then colour layer L-1-scale on that level's activations, and nothing after it.
 * out_dev: (n, C, lh*2^(L-scale), lw*2^(L-scale)) fp32 NCHW, or (n, lh*2^(L-scale), lw*2^(L-scale), C) uint8 HWC with
 * the x255 / clip / truncate epilogue of the full decode (_autoencoders.py:576-580).  scale == 0 is cae_synthesis /
 * cae_synthesis_symbols, unchanged; scale > 0 needs the colour layer of that level (cae_model_set_color_layer).  The
 * workspace is sized for the levels that run.  The f16x3 range guard works as for every call (cae_range_check).
 * Colour layers from at most 128 to at most 4 channels run on color_small_kernel (fp32 vector FMA on both precision
 * paths, only the useful output channels computed; f16x3: on hi + lo of the split rows, fp32 weights, raises the range
 * flag on a non-finite result); wider ones on the generic stride-1 launch followed by a uint8 conversion kernel.
 * CAE_ERR_ARG, before any launch: scale outside 0 .. L-1, colour layer not set, the level k//2 rows or columns or
 * fewer (reflect padding).  CAE_ERR_UNSUPPORTED: f16x3 with more than 32 image channels. */
int cae_synthesis_scale(cae_model_t *m, const float *latents_dev, int n, int lh, int lw, int scale, void *out_dev,
                        int fmt, void *stream);
int cae_synthesis_symbols_scale(cae_model_t *m, const int32_t *symbols_dev, int n, int lh, int lw, int scale,
                                void *out_dev, int fmt, void *stream);

/* One GDN / IGDN layer on an NCHW tensor (compressai.layers.GDN.forward; reference call site
 * _autoencoders.py:29-30).  Uses the beta/gamma of layer `index` of `track`. */
int cae_gdn_forward(cae_model_t *m, int track, int index, const float *x_dev, int n, int h, int w,
                    float *y_dev, void *stream);

/* EntropyBottleneck quantiser (compress(): symbols = round(y - median_c).int(), reference call
 * site _autoencoders.py:549-551; decompress(): y_hat = symbols + median_c, :568-571).
 * count = n * channels * hw elements in NCHW order, hw = spatial size per channel. */
int cae_quantize(cae_model_t *m, const float *latents_dev, int n, int hw, int32_t *symbols_dev, void *stream);
int cae_dequantize(cae_model_t *m, const int32_t *symbols_dev, int n, int hw, float *latents_dev, void *stream);

/* The same quantiser writing the symbols straight into PINNED HOST memory (a device-accessible host
 * pointer, e.g. hipHostMalloc / a pinned torch tensor) from at most `max_blocks` workgroups: the PCIe
 * transfer then runs beside the compute kernels of another stream on a few CUs.  (A hipMemcpyAsync D2H
 * here ran as a blit kernel that filled every CU's wave slots for the 1.8 ms the 100 MB take to cross
 * PCIe and stalled the next layer's kernels for that long; profiles/r01_experiments.md.)  The caller
 * synchronises `stream` (or an event on it) before reading the symbols on the host. */
int cae_quantize_export(cae_model_t *m, const float *latents_dev, int n, int hw, int32_t *symbols_pinned_host,
                        int max_blocks, void *stream);

/* Density network of the factorized prior (compressai EntropyBottleneck parameters `_matrix{i}`,
 * `_bias{i}`, `_factor{i}`, i = 0..n_filters; the reference builds it at _autoencoders.py:476-477 with
 * filters = [r]*K).  The caller passes EFFECTIVE values: matrices[i] = softplus(_matrix{i})
 * (channels, F[i+1], F[i]), biases[i] (channels, F[i+1]), factors[i] = tanh(_factor{i})
 * (channels, F[i+1]; i < n_filters), F = (1, filters..., 1).  likelihood_bound = 1e-9 in the
 * reference (0 disables the lower bound).  Hidden widths up to 8. */
int cae_model_set_density(cae_model_t *m, int channels, int n_filters, const int *filters,
                          const float *const *matrices, const float *const *biases,
                          const float *const *factors, float likelihood_bound);

/* Form of the likelihood p = c(y + 1/2) - c(y - 1/2) in floating point: 0 (default) = sigmoid(u) - sigmoid(l), as
 * compressai >= 1.2.x (`_likelihood` returning (likelihood, lower, upper), the version range the reference requires,
 * requirements.txt:25) is believed to compute it; 1 = the older sign trick |sigmoid(s u) - sigmoid(s l)|,
 * s = -sign(l + u).  Equal in exact arithmetic; in fp32 they differ in the last unit in the upper tail. */
int cae_model_set_likelihood_form(cae_model_t *m, int form);

/* EntropyBottleneck.__call__ in eval mode (reference call site models/tasks/_taskutils.py:97 and
 * the rate term -sum(log2 p) of models/criteria/_ratedist.py:49-54): for latents (n, channels, hw)
 *   y_hat = round(y - median_c) + median_c,
 *   likelihood = max(sigmoid(u) - sigmoid(l), bound), l,u = logits_cumulative(y_hat -/+ 0.5)
 *                (form: cae_model_set_likelihood_form),
 *   bits[i] = -sum log2(likelihood) over tile i (float64, deterministic order).
 * Any of y_hat_dev / likelihood_dev / bits_dev may be NULL.  Needs set_entropy (medians) and
 * set_density.  Calls on one handle must be stream-ordered. */
int cae_likelihood(cae_model_t *m, const float *latents_dev, int n, int hw, float *y_hat_dev,
                   float *likelihood_dev, double *bits_dev, void *stream);

/* Mean structural similarity of two (n, h, w, c) uint8 HWC batches -> ssim_dev[n] (float64): the algorithm of
 * skimage.metrics.structural_similarity(x, x_r, channel_axis=2) as the reference's metrics harness calls it
 * (test_cae.py:55-57): 7x7 uniform window, sample covariance, K1 = 0.01, K2 = 0.03, data range 255, 3-pixel border
 * cropped, mean over channels.  workspace_dev: n * ceil((h-6)/32) * ceil((w-6)/32) doubles. */
int cae_tile_ssim(const uint8_t *a_dev, const uint8_t *b_dev, int n, int h, int w, int c, double *ssim_dev,
                  double *workspace_dev, size_t workspace_elems, void *stream);

/* Mean CIE76 colour difference of two (n, pixels, 3) uint8 RGB batches -> delta_dev[n] (float64): skimage's
 * rgb2lab (sRGB, D65, 2-degree observer) + deltaE_cie76 + mean, as compute_deltaCIELAB does (test_cae.py:21-45).
 * workspace_dev: n * min(ceil(pixels/256), 128) doubles. */
int cae_tile_delta_e(const uint8_t *a_dev, const uint8_t *b_dev, int n, size_t pixels, double *delta_dev,
                     double *workspace_dev, size_t workspace_elems, void *stream);

/* Building blocks of pytorch_msssim.ms_ssim(x_r, x, data_range=255) as compute_ms_ssim calls it (test_cae.py:47-52):
 * uint8 HWC tiles -> planar float32 (n*c planes of h x w); one scale of the index on planar images: ssim_cs_dev[2p] =
 * mean ssim map, [2p+1] = mean contrast-structure map of plane p (11-tap window `window11_dev` applied separably without
 * padding, K = (0.01, 0.03), data range 255; workspace 2 * planes * ceil((h-10)/32) * ceil((w-10)/32) doubles); and the
 * 2x2 average pooling between scales (zero padding of odd sizes, out = floor((s + 2(s%2) - 2)/2) + 1 per side). */
int cae_u8hwc_to_planes(const uint8_t *tiles_dev, int n, int h, int w, int c, float *planes_dev, void *stream);
int cae_avgpool2(const float *in_dev, int planes, int h, int w, float *out_dev, void *stream);
int cae_msssim_level(const float *x_dev, const float *y_dev, int planes, int h, int w, const float *window11_dev,
                     double *ssim_cs_dev, double *workspace_dev, size_t workspace_elems, void *stream);

/* Blocking device -> pinned-host copy on the DMA engines (hsa_amd_memory_async_copy), for symbols on their way
 * to the host coder.  The caller has already waited for the kernels that produce `src_dev` (event / stream
 * synchronise); safe to call from any host thread.  hipMemcpyAsync is not used because the HIP runtime bundled
 * with PyTorch-ROCm 7.0 runs D2H copies as a blit kernel that occupies the CUs for the whole PCIe transfer. */
int cae_copy_to_host(void *dst_pinned_host, const void *src_dev, size_t bytes);

/* Per-tile sum of squared differences of two (n, elems) uint8 batches -> sse_dev[n] (float64).
 * The distortion half of the per-tile statistics record the slide driver all-gathers (the
 * reference's harness computes MSE/PSNR on the host, test_cae.py:55-68).  n is at most 65535, as for cae_tile_ssim
 * and cae_tile_delta_e (one grid row per tile): a larger n is CAE_ERR_ARG before anything is written. */
int cae_tile_sse(const uint8_t *a_dev, const uint8_t *b_dev, int n, size_t elems, double *sse_dev, void *stream);

/* ---- measurement ------------------------------------------------------------------------
 * With profiling on, cae_analysis / cae_synthesis bracket every kernel they launch with HIP
 * events on the caller's stream.  cae_model_get_profile synchronises those events and ADDS the
 * elapsed milliseconds of every call since the last reset into ms[0..n_slots): slot 0 is the
 * input layout conversion, slot 1+i the fused kernel of layer i (conv/deconv + bias + GDN).
 * calls receives the number of profiled calls.  (No reference counterpart: the reference only
 * takes perf_counter wall times, test_cae.py:101-115.) */
int cae_model_set_profiling(cae_model_t *m, int enable);
int cae_model_get_profile(cae_model_t *m, int track, double *ms, int n_slots, int *calls, int reset);

/* Launch shape of the persistent kernels of the f16x3 path on the current device (read-only, for the tests; the
 * launchers compute their grids with the same functions).  kernel: 0 conv_first_f16_kernel, 1 deconv_last_f16_kernel,
 * 2 gdn_f16_kernel on analysis rows (GDN), 3 on synthesis rows (IGDN: the row groups pair even and odd pixels of
 * 64-pixel blocks).  ks: kernel size, 3 or 5, of kernels 0 and 1 (ignored for the others).  n samples of the h x w
 * extent the launcher tiles: the output of the first layer and of the normalisation, the input of the last layer.
 * tiles: what the kernel's loop counts -- tiles of the first and the last layer, 32-pixel wave groups of the
 * normalisation (four per block and turn).  blocks: the grid; block b takes tiles b, b + blocks, ... (the
 * normalisation: wave v of block b groups 4 b + v, 4 b + v + 4 blocks, ...).  CAE_ERR_ARG: an unknown kernel, another
 * ks, n, h or w < 1, a NULL pointer, more than 2^31 - 1 tiles. */
int cae_persistent_launch(int kernel, int ks, int n, int h, int w, int64_t *tiles, int *blocks);

/* ---- training (BASELINE config 5: bf16 convolutions, fp32 GDN) ----------------------------
 * What `loss.backward()` (train_cae_ms.py:214) differentiates on the reference: nn.Conv2d(reflect, stride 2) /
 * nn.ConvTranspose2d(stride 2, output_padding 1) (_autoencoders.py:78-85, :204-211) and compressai GDN / IGDN (:29-30).
 * Stateless launches on caller-owned device buffers.  Layout "T": channels-last [n][h][w][cp], cp = channels padded
 * to a multiple of 32 (<= 192) with zeros; *16 = bf16, *32 = fp32.  Convolutions take bf16 operands and accumulate in
 * fp32 (v_mfma_f32_32x32x16_bf16); GDN is exact fp32 (v_mfma_f32_32x32x2_f32).
 * Packed weights: MFMA B fragments of a (dim0, dim1, k, k) fp32 tensor with dimension `contract_dim` contracted:
 *   nn.Conv2d weight (cout, cin, k, k):          forward contracts dim 1, data gradient dim 0;
 *   nn.ConvTranspose2d weight (cin, cout, k, k): forward contracts dim 0, data gradient dim 1. */
size_t cae_t_packed_bytes(int contract_channels, int out_channels, int kernel_size);
int cae_t_pack_weights(const float *w_dev, int dim0, int dim1, int kernel_size, int contract_dim, void *packed_dev, void *stream);
int cae_t_from_nchw(const float *x_nchw_dev, int n, int c, int h, int w, int cp, void *out16, float *out32, void *stream);
int cae_t_to_nchw(const float *t32, int n, int c, int h, int w, int cp, float *out_nchw_dev, void *stream);
/* Samples each block of the strided / pointwise gather-GEMM kernels walks (the same tile of consecutive samples);
 * 0 (the default): chosen per launch from the batch and the tile count.  A testing knob: it forces ragged sample groups. */
int cae_t_set_samples_per_block(int npb);
/* z = conv(x) (+bias): x16 [n][h][w][cin_p] -> z [n][ceil(h/2)][ceil(w/2)][cout_p] as fp32 and / or bf16 */
int cae_t_conv_forward(const void *x16, int n, int h, int w, int cin_p, const void *packed, int kernel_size, float *z32,
                       void *z16, int cout_p, const float *bias, void *stream);
/* data gradient of that convolution on the EXTENDED domain: gext32 [n][h+2P][w+2P][cin_p], P = k//2, the gradient with
 * respect to the reflect-PADDED input; its consumer folds the border back (cae_t_gdn_backward / cae_t_fold_to_bf16) */
int cae_t_conv_dgrad_ext(const void *gz16, int n, int oh, int ow, int cout_p, const void *packed, int kernel_size, int h,
                         int w, float *gext32, int cin_p, void *stream);
/* z = conv_transpose(x) (+bias): x16 [n][h][w][cin_p] -> z [n][2h][2w][cout_p] */
int cae_t_deconv_forward(const void *x16, int n, int h, int w, int cin_p, const void *packed, int kernel_size, float *z32,
                         void *z16, int cout_p, const float *bias, void *stream);
/* its data gradient: gz16 [n][2h][2w][cout_p] -> gx [n][h][w][cin_p] */
int cae_t_deconv_dgrad(const void *gz16, int n, int h, int w, int cout_p, const void *packed, int kernel_size, float *gx32,
                       void *gx16, int cin_p, void *stream);
/* weight gradient of either layer: gw32 [k*k][ca][cb] = sum over positions of xbig[2 pos + tap - P][a] * ysmall[pos][b].
 * conv: xbig = layer input (reflect = 1), ysmall = output gradient -> grad(cout,cin,k,k)[b][a][tap];
 * conv_transpose: xbig = output gradient (reflect = 0), ysmall = layer input -> grad(cin,cout,k,k)[b][a][tap]. */
int cae_t_wgrad(const void *xbig16, int n, int h, int w, int ca, const void *ysmall16, int oh, int ow, int cb,
                int kernel_size, int reflect, float *gw32, void *stream);
/* GDN / IGDN forward on effective parameters padded to cp (beta padding 1, gamma padding 0): y = z * rsqrt(beta +
 * gamma z^2) (inverse: sqrt). */
int cae_t_gdn_forward(const float *z32, long pixels, int cp, const float *beta, const float *gamma, int inverse, float *y32,
                      void *y16, void *stream);
/* GDN / IGDN backward.  gext32: gradient with respect to the layer output, fp32 [n][h+2 pad][w+2 pad][cp] (pad > 0: the
 * extended-domain gradient of the next convolution, folded here; pad = 0: plain).  gamma_t = gamma transposed.
 * Outputs: gz (bf16 and / or fp32) with respect to z, ggamma [cp][cp], gbeta [cp] with respect to the EFFECTIVE
 * parameters (the reparametrisation and its LowerBound gradient rule live above the ABI); gn_ws32 / gzd_ws32: scratch,
 * pixels * cp floats each. */
int cae_t_gdn_backward(const float *z32, const float *gext32, int n, int h, int w, int pad, int cp, const float *beta,
                       const float *gamma, const float *gamma_t, int inverse, float *gn_ws32, float *gzd_ws32, float *gz32,
                       void *gz16, float *ggamma, float *gbeta, void *stream);
/* LeakyReLU / ReLU units under autograd (DownsamplingUnit _autoencoders.py:62-76,90-92; UpsamplingUnit :187-202,216-218):
 * the strided layers with the activation (1 LeakyReLU(0.01), 2 ReLU) in their epilogue; the stride-1 pre-convolutions as
 * cae_t_corr_s1 -- mode 0 analysis forward (reflect), 1 its data gradient on the extended domain (h + 2P) x (w + 2P),
 * 2 synthesis forward (ConvTranspose2d stride 1, padding k//2), 3 its data gradient; the packed weights carry the
 * contraction (cae_t_pack_weights: contract_dim 1 for modes 0 and 3, 0 for modes 1 and 2) --, their weight gradient
 * cae_t_wgrad_s1 (x and y of equal size; analysis: x = input, reflect; synthesis: x = output gradient, zeros, y = input),
 * and the activation's backward cae_t_act_backward: out = g * (y > 0 ? 1 : slope) with y the activation's OUTPUT and g
 * either bf16 (g16) or the fp32 extended-domain gradient gext32, whose reflect fold is applied in place first. */
int cae_t_conv_forward_act(const void *x16, int n, int h, int w, int cin_p, const void *packed, int ks, float *z32, void *z16,
                           int cout_p, const float *bias, int act, void *stream);
int cae_t_deconv_forward_act(const void *x16, int n, int h, int w, int cin_p, const void *packed, int ks, float *z32, void *z16,
                             int cout_p, const float *bias, int act, void *stream);
int cae_t_corr_s1(const void *x16, int n, int h, int w, int ck, const void *packed, int ks, int mode, float *out32, void *out16,
                  int cn, const float *bias, int act, void *stream);
int cae_t_wgrad_s1(const void *x16, int n, int h, int w, int ca, const void *y16, int cb, int ks, int reflect, float *gw32,
                   void *stream);
int cae_t_act_backward(const void *g16, float *gext32, int pad, const void *y16, int n, int h, int w, int cp, int act,
                       void *out16, void *stream);

/* Edge layers with <= 3 image channels as pointwise GEMMs over K = (tap, channel) <= 32 (instead of padding 3 channels to
 * 32): cae_t_im2col_s2 gathers the stride-2 taps of an NCHW fp32 tensor into [n][oh][ow][32] bf16 (j = tap * c + channel;
 * reflect = 1: the first analysis layer's input (nn.Conv2d reflect, _autoencoders.py:78-85); 0: zeros outside -- the last
 * synthesis layer's output gradient, oh = h / 2); cae_t_pointwise / cae_t_wgrad_pointwise are the 1 x 1 gather-GEMM and
 * its weight gradient on channels-last bf16 tensors; cae_t_col2im_s2 sums the <= 4 products u[pos][(tap, channel)] of every
 * output pixel of ConvTranspose2d(k, 2, k//2, output_padding 1) (:204-211) into NCHW fp32 (+ bias). */
int cae_t_im2col_s2(const float *x_nchw, int n, int c, int h, int w, int oh, int ow, int ks, int reflect, void *out16,
                    void *stream);
int cae_t_col2im_s2(const float *u32, const float *bias, int n, int c, int h, int w, int ks, float *out_nchw, void *stream);
int cae_t_pointwise(const void *x16, int n, int h, int w, int ck, const void *packed, float *out32, void *out16, int cn,
                    const float *bias, int act, void *stream);
int cae_t_wgrad_pointwise(const void *x16, const void *y16, int n, int h, int w, int ca, int cb, float *gw32, void *stream);

/* Multiscale colour layers Conv2d(c_in -> c, k, stride 1, reflect padding k//2) (_autoencoders.py:417-428, c <= 3) as an edge
 * GEMM over K = (tap, channel), kp = pad32(k * k * c) <= 96 columns: cae_t_pointwise forms u[q][(tap, co)] (fp32
 * [n][h][w][kp]); cae_t_col2im_s1r sums out[p][co] = bias[co] + sum_tap u[reflect(p + tap - P)][(tap, co)] into NCHW fp32;
 * cae_t_im2col_s1r is its adjoint gu[q][(tap, co)] = sum over p with reflect(p + tap - P) = q of bf16(g[p][co]) (fp32 sums
 * stored as a bf16 pair: hi in columns [0, kp), lo = the rest in [kp, 2 kp) of each [n][h][w][2 kp] record; contracting
 * both halves against the same weights gives the folded sum to ~2^-17).  cae_t_pointwise_acc is cae_t_pointwise with the result ADDED to out32 (no bias, no
 * activation): the colour layer's data gradient onto the level's gradient.  cae_t_fold_acc adds the reflect fold of an
 * extended-domain gradient to out32 (the padded form's data gradient).  h and w must exceed P (as the reflect pad).
 * cae_t_pyramid_down: one step of DistMSEPyramidLoss's pyramid (_ratedist.py:10-43): 5 x 5 binomial blur, zero padding 2,
 * then bilinear x 0.5 -- NCHW fp32 (n, c, h, w) -> (n, c, h / 2, w / 2). */
int cae_t_col2im_s1r(const float *u32, const float *bias, int n, int c, int h, int w, int ks, int kp, float *out_nchw,
                     void *stream);
int cae_t_im2col_s1r(const float *g_nchw, int n, int c, int h, int w, int ks, int kp, void *out16, void *stream);
int cae_t_pointwise_acc(const void *x16, int n, int h, int w, int ck, const void *packed, float *out32, int cn, void *stream);
int cae_t_fold_acc(const float *gext32, int n, int h, int w, int pad, int cp, float *out32, void *stream);
int cae_t_pyramid_down(const float *x_nchw, int n, int c, int h, int w, float *out_nchw, void *stream);

/* Differentiable MS-SSIM (DistMSSSIMLoss, _ratedist.py:66-90) on planar fp32 images: `planes` = N * C images of h x w,
 * x the reconstruction (carries the gradient), y the target.  `taps_host` points to the `win` window taps in HOST memory
 * (win odd, 1..11; they travel by value with the launch); the window is applied separably without padding, rows first.
 * The images are float32; the local moments and the two index maps are formed in float64 (the variances cancel).
 * cae_t_msssim_level_fwd: one scale -- ssim_cs_dev[2p] = mean ssim map, [2p+1] = mean contrast-structure map of plane p
 * (float64) with the constants c1, c2; workspace_dev: 2 * planes * ceil((h-win+1)/32) * ceil((w-win+1)/32) doubles.
 * cae_t_msssim_level_bwd: its adjoint with respect to x, ADDED to gx_dev (planes * h * w floats):
 * gx += d/dx sum_p (g_ssim_dev[p] * ssim_p + g_cs_dev[p] * cs_p); g_ssim_dev or g_cs_dev may be NULL (zeros);
 * workspace_dev: 3 * planes * (h-win+1) * (w-win+1) floats (the coefficient maps between its two launches).
 * cae_t_avgpool2_bwd: the adjoint of cae_avgpool2 -- g_fine_dev (planes, h, w) = a quarter of the g_coarse_dev sample
 * that covers each pixel (OVERWRITES g_fine_dev; coarse size as cae_avgpool2's output).
 * planes must be 1..65535 for the two level calls (one grid row per plane; CAE_ERR_ARG otherwise): split larger batches.
 * No atomics, fixed summation order: all three are bitwise reproducible. */
int cae_t_msssim_level_fwd(const float *x_dev, const float *y_dev, int planes, int h, int w, const double *taps_host, int win,
                           double c1, double c2, double *ssim_cs_dev, double *workspace_dev, size_t workspace_elems,
                           void *stream);
int cae_t_msssim_level_bwd(const float *x_dev, const float *y_dev, int planes, int h, int w, const double *taps_host, int win,
                           double c1, double c2, const double *g_ssim_dev, const double *g_cs_dev, float *gx_dev,
                           float *workspace_dev, size_t workspace_elems, void *stream);
int cae_t_avgpool2_bwd(const float *g_coarse_dev, int planes, int h, int w, float *g_fine_dev, void *stream);

/* Fused forms (csrc/cae_train_gdn.hpp; cp <= 128): the forward also saves the per-element factor f (y = z f: n^(-1/2),
 * IGDN n^(1/2)) in the register order the backward reads back -- f_saved holds cae_t_gdn_saved_elems(pixels, cp) floats
 * (0: shape not built) -- and the backward is ONE kernel: g_z (bf16), g_gamma, g_beta from z, f and the gradient with
 * respect to y (extended domain with padding `pad`; its reflect fold is applied to gext32 IN PLACE first), without
 * recomputing the norm. */
size_t cae_t_gdn_saved_elems(long pixels, int cp);
int cae_t_gdn_forward_save(const float *z32, long pixels, int cp, const float *beta, const float *gamma, int inverse,
                           void *y16, float *f_saved, void *stream);
int cae_t_gdn_backward_fused(const float *z32, const float *f_saved, float *gext32 /* folded in place */, int n, int h, int w, int pad, int cp,
                             const float *gamma, int inverse, void *gz16, float *ggamma, float *gbeta, void *stream);
int cae_t_fold_to_bf16(const float *gext32, int n, int h, int w, int pad, int cp, void *out16, void *stream);

/* nn.BatchNorm2d in TRAINING mode (batch statistics; the units' optional batch norm, _autoencoders.py:72-73, :87-88, and
 * its backward as torch autograd derives it) on NCHW fp32 tensors (n, c, hw).  Both directions are a pair of per-channel
 * moments and a per-channel affine map:
 *   cae_t_bn_moments   s1[c] = sum a, s2[c] = sum a b   over (n, hw), accumulated in double
 *                      (forward: a = b = x; backward: a = dy, b = x)
 *   cae_t_bn_affine    out = a A[c] + (b ? b B[c] : 0) + C[c]
 *                      (forward: y = x w rstd + (bias - mean w rstd); backward: dx = dy A + x B + C) */
int cae_t_bn_moments(const float *a, const float *b, int n, int c, long hw, double *s1, double *s2, void *stream);
int cae_t_bn_affine(const float *a, const float *b, int n, int c, long hw, const float *A, const float *B, const float *C,
                    float *out, void *stream);
int cae_t_colsum(const void *g16, long pixels, int cp, float *out, void *stream); /* bias gradient */

/* Training-mode density of the entropy bottleneck, fused (csrc/cae_density_train.hip).  Replaces the element-wise graph of
 * compressai's EntropyBottleneck.forward(training=True) / _likelihood / LowerBound under autograd
 * (_autoencoders.py:502 via models/tasks/_taskutils.py:95-108).
 * raw_params: (channels, NP) fp32 = per channel [matrices 0..K | biases 0..K | factors 0..K-1], each in its stored
 * (un-transformed) form and row-major shape; NP = cae_t_density_params(D, K) (0: shape not built; built: D = 3, K = 4).
 * forward: out = y + noise (noise may be NULL), lik = max(p(out), bound); plain = 1: sigmoid(u) - sigmoid(l), 0: sign trick.
 * backward: g_y = g_out (may be NULL) + g_lik dp/dy with the LowerBound rule; g_raw_params (channels, NP), overwritten. */
int cae_t_density_params(int filters_d, int n_filters);
int cae_t_density_forward(const float *y, const float *noise, const float *raw_params, int n, int channels, int hw, int plain,
                          float bound, float *out, float *lik, void *stream);
int cae_t_density_backward(const float *out, const float *g_lik, const float *g_out, const float *raw_params, int n,
                           int channels, int hw, int plain, float bound, float *g_y, float *g_raw_params, void *stream);
/* ---- training input: sample and augment patches on the device (csrc/cae_sampler.hip) ---------------------------------
 * Replaces the per-patch CPU transform of utils/datasets/_augs.py:197-264 (get_zarr_transform, label_density == 0:
 * ToTensor, AddGaussianNoise(0, 0.001), RandomCrop(pad_if_needed) / CenterCrop, Normalize(0.5, 0.5), bilinear
 * RandomRotation(30)).  The random draws stay with the caller; one launch writes the batch train_step takes.
 *
 * pool_dev: uint8 [tiles][h][w][c] on the device, 1 <= c <= 4.  tile_hw_dev: int32 [tiles][2], the valid rows and
 * columns of each tile (the rest is storage padding and counts as outside the image), or NULL: every tile is h x w.
 * Per sample, on the device: int32 tile_dev, y0_dev, x0_dev; optionally float32 cos_dev, sin_dev of the angle (the host
 * computes them in float64 and rounds once; both NULL = no rotation).  out_dev: float [n][c][ps][ps].
 *
 * Patch value.  For patch pixel (py, px) and channel ch, the image pixel is (y0+py, x0+px) of tile `tile`.
 *   - Inside the image, v = clamp(u8 / 255 + noise_std * g, 0, 1).
 *   - Outside the image, v = 0.  This is pad_if_needed's constant fill.  The reference adds noise before the crop, so
 *     padding carries no noise.
 *   - u8 / 255 is the correctly rounded float32 quotient, as torch's .div(255) gives (IEEE division, no reciprocal
 *     multiply).
 *   - Then p = normalize ? (v - 0.5) / 0.5 : v.
 * Noise.  g is a standard normal from a counter-based generator, Philox4x32-10.
 *   - The key is the two halves of `seed` (low word first).
 *   - The counter is (sample_base + sample index, py * ps + px, 0, 0).
 *   - The four output words map through u = (word + 0.5) * 2^-32 and two Box-Muller pairs to four normals: with
 *     r = sqrt(-2 ln u_0), normals 0 and 1 are r cos(2 pi u_1) and r sin(2 pi u_1); words 2 and 3 give normals 2 and 3
 *     likewise.  Channel ch takes normal ch.
 *   - The accurate logf / log1pf / sincospif are used, not the fast intrinsics.  noise_std == 0 means no noise.
 * The value at a patch pixel therefore does not depend on which output pixel reads it, so rotation interpolates one
 * consistent noisy patch, as in the reference.  Results are bitwise repeatable and independent of the launch shape;
 * sample_base lets a batch be produced in several calls.
 * Rotation.  The reference rotates the cropped, normalised patch with zero fill.  With cx = cy = (ps - 1) / 2, output
 * (i, j) reads the patch at
 *     sx = cx + cos a * (j - cx) - sin a * (i - cy)
 *     sy = cy + sin a * (j - cx) + cos a * (i - cy)
 * and takes the four bilinear taps of p.  A tap outside [0, ps) contributes 0, which is 0 after normalisation, i.e.
 * mid-grey.  A positive angle turns the picture counter-clockwise as displayed.  With the rotation pointers NULL, the
 * output is p itself, bit for bit.
 *
 * CAE_ERR_ARG before any launch: c outside 1..4, ps outside 1..16384, n < 0, tiles / h / w < 1 (h, w at most 2^24), a NULL
 * pool / tile / y0 / x0 / out pointer, only one of cos_dev / sin_dev, a negative or non-finite noise_std, more than
 * 2^31 - 1 blocks of 256 work items, and -- when tile_host, a HOST copy of tile_dev, is given -- a tile index outside
 * [0, tiles).  The kernels fault on no device-side value either: a tile index outside [0, tiles) reads as an empty image
 * (all padding), offsets are clamped to where they select only padding, tile_hw entries to [0, h] x [0, w]. */
int cae_t_sample_patches(const uint8_t *pool_dev, int tiles, int h, int w, int c, const int32_t *tile_hw_dev,
                         const int32_t *tile_dev, const int32_t *y0_dev, const int32_t *x0_dev, const int32_t *tile_host,
                         const float *cos_dev, const float *sin_dev, uint64_t seed, uint32_t sample_base, float noise_std,
                         int normalize, int n, int ps, float *out_dev, void *stream);

/* ---- training input with pixel labels: image and mask under one crop and one rotation (csrc/cae_sampler.hip) ---------
 * Replaces the pair transform of utils/datasets/_augs.py:52-82, 240-299 (get_zarr_transform with label_density == 2:
 * the transforms above, then RandomRotationInputTarget(30) = scipy.ndimage.rotate(reshape=False, mode='reflect') with
 * spline order 4 on the image and order 0 on the mask, and MapLabels).  One call writes both batches seg_train's
 * train_step takes.
 *
 * Inputs.  Everything of the entry point above, with the same meaning, and:
 *   labels_dev      uint8 [tiles][h][w][k] on the device, 1 <= k <= 4: the label pool.  It shares the tile geometry of
 *                   the image pool (tile_hw_dev, tile, y0, x0 address both).
 *   map_labels      1: the k channels are summed into one (MapLabels); 0: they stay apart.  kt = map_labels ? 1 : k.
 *   workspace_dev, workspace_bytes   device scratch of at least
 *                       (cos_dev != NULL && ps > 128) ? n * c * ps * ps * sizeof(float) : 0
 *                   bytes (NULL / 0 where that is 0).  What it holds before the call does not matter.
 *   x_dev           float [n][c][ps][ps];   t_dev   float [n][kt][ps][ps].
 *
 * Patch p.  Exactly the p of the contract above: the crop window (y0, x0), u8 / 255 correctly rounded, the Philox noise
 * keyed by (seed, sample_base + sample index, py * ps + px), clamp, normalisation, 0 (-1 after normalisation) outside the
 * tile's valid extent.  (The kernels call the same code.)
 * Mask patch m.  The same window of the label pool as float values, 0 outside the valid extent; with map_labels the sum
 * over the k channels (summing commutes with nearest-neighbour sampling).
 * No rotation (cos_dev == sin_dev == NULL).  x = p bit for bit and t = m exactly.
 * Rotation, about cc = (ps - 1) / 2.  Output pixel (i, j) (row, column) reads the source point
 *     y =  cos a * (i - cc) + sin a * (j - cc) + cc
 *     x = -sin a * (i - cc) + cos a * (j - cc) + cc
 * (the same turn as above: a positive angle is counter-clockwise as displayed).  Every row or column index q that follows
 * is reflected half-sample symmetrically, as often as needed (d c b a | a b c d | d c b a):
 *     refl(q) = r < ps ? r : 2 ps - 1 - r,  r = q mod 2 ps  (0 <= r < 2 ps).
 * Repeated reflection matters where ps is smaller than the tap support.  There is no zero fill.
 *   Mask.   t = m[refl(floor(y + 0.5))][refl(floor(x + 0.5))].
 *   Image.  x = sum over a, b = 0..4 of w(y - (ys + a)) w(x - (xs + b)) coef[refl(ys + a)][refl(xs + b)], with
 *           ys = floor(y + 0.5) - 2, xs = floor(x + 0.5) - 2 and the quartic B-spline
 *               w(d) = d^2 (d^2 / 4 - 5 / 8) + 115 / 192                              |d| < 0.5
 *                      |d| (|d| (|d| (5 / 6 - |d| / 6) - 5 / 4) + 5 / 24) + 55 / 96   |d| < 1.5
 *                      (|d| - 2.5)^4 / 24                                             |d| < 2.5,  else 0.
 *           There is no clipping afterwards: the spline overshoots, as the reference's does.
 *   coef.   The interpolation coefficients of each channel plane of p: every row is filtered, then every column.  A line
 *           c[0..n-1] (n = ps) is scaled by the gain, the product over both poles of (1 - z)(1 - 1 / z) (= 384), and then,
 *           for z1 = sqrt(664 - sqrt(438976)) + sqrt(304) - 19 and after it z2 = sqrt(664 + sqrt(438976)) - sqrt(304) - 19:
 *               c[0]   = c0 + z / (1 - z^(2n)) * (c0 + z^n c[n-1] + sum_{i=1..n-1} z^i (c[i] + z^n c[n-1-i])),  c0 = c[0]
 *               c[i]  += z c[i-1]                 i = 1 .. n-1
 *               c[n-1] *= z / (z - 1)
 *               c[i]   = z (c[i+1] - c[i])        i = n-2 .. 0.
 *           This start is the exact one for the reflected line, so the spline interpolates: at angle 0, x = p up to
 *           rounding for every ps >= 1.  scipy's own result parts from this form below about 12 pixels per side (by
 *           about |z1|^(2n): 3e-3 at n = 2, 5e-8 at n = 8); the contract is the exact form.  The kernels work in float32
 *           and drop terms of the start that are below float32 resolution (z^i from i = 28, z^n from n = 64).
 * Results are bitwise repeatable, independent of the launch shape and of what x_dev, t_dev and the workspace held, and
 * independent of how a batch is split over calls by sample_base.
 *
 * CAE_ERR_ARG before any launch: everything the entry point above refuses (with x_dev as its out_dev), k outside 1..4, a
 * NULL labels_dev or t_dev, and a workspace that is NULL or smaller than the size above where that size is not 0 (the
 * message names the bytes needed).  No device-side value faults here either: tiles, offsets and tile_hw are treated as
 * above, and cos / sin that are NaN or huge are clamped as source coordinates to [-ps, 2 ps] before any integer cast. */
int cae_t_sample_labeled_patches(const uint8_t *pool_dev, const uint8_t *labels_dev, int tiles, int h, int w, int c, int k,
                                 const int32_t *tile_hw_dev, const int32_t *tile_dev, const int32_t *y0_dev,
                                 const int32_t *x0_dev, const int32_t *tile_host, const float *cos_dev, const float *sin_dev,
                                 uint64_t seed, uint32_t sample_base, float noise_std, int normalize, int map_labels, int n,
                                 int ps, void *workspace_dev, size_t workspace_bytes, float *x_dev, float *t_dev,
                                 void *stream);

/* ---- training input: elastic deformation of image and mask patches (csrc/cae_elastic.hip) ---------------------------------
 * Stands where RandomElasticDeformationInput / RandomElasticDeformationInputTarget(sigma) of utils/datasets/_augs.py:26-49,
 * 85-99 stand (get_zarr_transform with elastic_deformation=True): a 3 x 3 grid of random displacements is interpolated to a
 * per-pixel field; the image is resampled through the cubic B-spline, the mask by its nearest neighbour, edges reflected.
 * The contract below is the form of that operation that scipy.ndimage expresses (map_coordinates(order=3, mode='mirror')
 * for the field, spline_filter + map_coordinates(order=3 / 0, mode='reflect') for the planes); parity with the
 * `elasticdeform` package itself is not pinned.  The call works on a batch that already lies in device memory, after
 * either sampler entry point above or on any tensor the caller brings.
 *
 * Inputs.
 *   x_in, x_out     float [n][c][ps][ps], 1 <= c <= 4.
 *   t_in, t_out     float [n][kt][ps][ps], 0 <= kt <= 4; both NULL with kt == 0 (the image-only transform).
 *   coef_dev        float [n][2][3][3] on the device: the spline coefficients of each sample's displacement grid (below).
 *   workspace_dev, workspace_bytes   device scratch of at least cae_t_elastic_deform_workspace(n, c, ps) =
 *                       ps > 128 ? n * c * ps * ps * sizeof(float) : 0
 *                   bytes (NULL / 0 where that is 0).  What it holds before the call does not matter.
 *
 * Displacement field.  The caller draws d[k][a][b], k = 0 for rows and 1 for columns, a, b = 0..2, as N(0, sigma^2) in
 * float64 (np.random.randn(2, 3, 3) * sigma).  Control point (a, b) sits at pixel (a (ps - 1) / 2, b (ps - 1) / 2).  The field
 * is the interpolating cubic B-spline through the nine values with whole-sample mirror extension of the grid
 * (... 2 1 | 0 1 2 | 1 0 ...).  The caller solves for its coefficients in float64 and rounds once to float32 (as cos / sin
 * are handled above): with M = [[2/3, 1/3, 0], [1/6, 2/3, 1/6], [0, 1/3, 2/3]],
 *     coef[k] = M^-1 d[k] M^-T.
 * With the cubic B-spline
 *     beta(r) = 2/3 - r^2 + |r|^3 / 2   |r| < 1
 *               (2 - |r|)^3 / 6         |r| < 2,  else 0,
 * the grid coordinate u_i = 2 i / (ps - 1) of row or column i (0 with ps == 1) and the folded weights
 *     W_0(u) = beta(u),   W_1(u) = beta(u - 1) + beta(u + 1) + beta(u - 3),   W_2(u) = beta(u - 2),
 * the kernels evaluate
 *     D_k(i, j) = sum over a, b = 0..2 of W_a(u_i) W_b(u_j) coef[k][a][b],
 * which equals scipy.ndimage.map_coordinates(d[k], [u_i, u_j], order=3, mode='mirror').
 * Source point.  Output pixel (i, j) (row, column) reads y = i + D_0(i, j), x = j + D_1(i, j), both clamped to [-ps, 2 ps]
 * before any integer cast (a NaN becomes -ps).  Every row or column index q that follows is reflected half-sample
 * symmetrically, as often as needed: refl(q) of the labelled contract above.
 *   Mask.   t_out = t_in[refl(floor(y + 0.5))][refl(floor(x + 0.5))] per channel, an exact copy of a value.
 *   Image.  x_out = sum over a, b = 0..3 of beta(y - (ys + a)) beta(x - (xs + b)) cf[refl(ys + a)][refl(xs + b)], with
 *           ys = floor(y) - 1 and xs = floor(x) - 1.  There is no clipping afterwards.
 *   cf.     The cubic interpolation coefficients of each plane of x_in: every row is filtered, then every column.  A line
 *           c[0..n-1] (n = ps) is scaled by 6 = (1 - z)(1 - 1 / z) and run through the recursion of the labelled contract
 *           above with the single pole z = sqrt(3) - 2:
 *               c[0]   = c0 + z / (1 - z^(2n)) * (c0 + z^n c[n-1] + sum_{i=1..n-1} z^i (c[i] + z^n c[n-1-i])),  c0 = c[0]
 *               c[i]  += z c[i-1]                 i = 1 .. n-1
 *               c[n-1] *= z / (z - 1)
 *               c[i]   = z (c[i+1] - c[i])        i = n-2 .. 0.
 *           This start is the exact one for the reflected line.  scipy's spline_filter1d(order=3, mode='reflect') parts
 *           from it by up to 6e-4 at n = 2, 1e-6 at 5 and 4e-10 at 8 (lines in [-1, 1]) and equals it to rounding from n = 16; the contract is the
 *           exact form.  The filter's l1 gain per axis is 3.  The kernels work in float32 and drop terms of the start that
 *           are below float32 resolution (z^i from i = 22, z^n from n = 64).
 * Zero displacement.  t_out == t_in exactly and x_out == x_in up to rounding, for every ps >= 1.
 * Results are bitwise repeatable and independent of the launch shape and of what x_out, t_out and the workspace held.
 *
 * CAE_ERR_ARG before any launch, with a message in cae_last_error: c outside 1..4, kt outside 0..4, ps outside 1..16384,
 * n < 0, a NULL x_in, x_out or coef_dev, kt > 0 with a NULL t_in or t_out, kt == 0 with a non-NULL t_in or t_out, an output
 * that is also an input, a workspace that is NULL or smaller than the query where that size is not 0 (the message names
 * the bytes), more than 2^31 - 1 blocks.  n == 0 returns CAE_OK with nothing launched.  No device-side value faults:
 * coefficients that are NaN or huge only move clamped coordinates.  The workspace query returns 0 for arguments the call
 * refuses. */
int cae_t_elastic_deform(const float *x_in, const float *t_in, const float *coef_dev, int n, int c, int kt, int ps,
                         void *workspace_dev, size_t workspace_bytes, float *x_out, float *t_out, void *stream);
size_t cae_t_elastic_deform_workspace(int n, int c, int ps);

/* compressai NonNegativeParametrizer (GDN beta / gamma; layers/gdn.py via _autoencoders.py GDN units) under autograd:
 * out = max(x, bound)^2 - pedestal;  g_x = g 2 max(x, bound) where x >= bound or that value is negative (LowerBound rule). */
int cae_t_reparam_forward(const float *x, long n, float bound, float pedestal, float *out, void *stream);
int cae_t_reparam_backward(const float *x, const float *g, long n, float bound, float *gx, void *stream);

/* One clip + Adam step over all parameters of a training step (train_cae_ms.py:221-230: per optimiser
 * clip_grad_norm_(params, max_norm) then torch.optim.Adam.step(), no amsgrad) in two launches.  A group = one optimiser:
 * tensors ordered by group; per group lr, betas, eps, weight_decay, max_norm (<= 0: no clipping) and the 1-based step
 * count of THIS step (bias corrections).  All pointers are device pointers to fp32; partial_ws holds one float per
 * 2048-element chunk (sum over tensors of ceil(numel / 2048)); deterministic (no atomics). */
#define CAE_OPTIM_MAX_TENSORS 64
#define CAE_OPTIM_MAX_GROUPS 8
int cae_t_clip_adam(int ntensors, float *const *params, const float *const *grads, float *const *exp_avg,
                    float *const *exp_avg_sq, const int *numel, const int *group, int ngroups, const float *lr,
                    const float *beta1, const float *beta2, const float *eps, const float *weight_decay,
                    const float *max_norm, const int *step, float *partial_ws, size_t partial_elems, void *stream);

/* ---- host entropy coding ---------------------------------------------------------------
 * Replace compressai._CXX.pmf_to_quantized_cdf and compressai.ans.RansEncoder /
 * RansDecoder (encode_with_indexes / decode_with_indexes), reached from
 * EntropyBottleneck.update / compress / decompress (_autoencoders.py:502, :549-551, :568-571).
 * Streams are coded independently (one per tile), in parallel on `threads` host threads
 * (0 = $CAE_CODER_THREADS, else min(CPUs of this process, 16)).  Symbol order inside a stream is (c, y, x) raster; the CDF row
 * of a symbol is its channel c. */
/* CPUs this process may keep busy: affinity mask, capped by the cgroup CPU quota, divided by LOCAL_WORLD_SIZE. */
int cae_cpu_budget(void);
/* Streams one coder thread walks in lockstep (2 or 4 independent chains per loop iteration; CAE_CODER_LOCKSTEP, else 4
 * when fewer than 16 CPUs are available to this process: fewer CPU-seconds per symbol, half as many work items). */
int cae_coder_lockstep(void);
/* Size of the coder pool a cae_rans_*_batch call with `threads` = requested and n_streams streams uses. */
int cae_coder_threads(int requested, int n_streams);

int cae_pmf_to_quantized_cdf(const float *pmf_host, int n, int precision, uint32_t *cdf_host /* n+1 */);

/* symbols_host: (n_streams, channels, hw) int32.  On success out_bufs[i] (library-allocated,
 * cae_free each) holds stream i and out_lens[i] its byte length. */
int cae_rans_encode_batch(cae_model_t *m, const int32_t *symbols_host, int n_streams, int hw,
                          uint8_t **out_bufs, size_t *out_lens, int threads);
/* The same streams in ONE library-allocated buffer (cae_free): stream i = out_buf[offsets[i] .. offsets[i+1]),
 * offsets has n_streams + 1 entries.  (The batched drivers hand the streams on without per-stream copies.) */
int cae_rans_encode_packed(cae_model_t *m, const int32_t *symbols_host, int n_streams, int hw, uint8_t **out_buf,
                           size_t *offsets, int threads);
/* bufs[i]/lens[i]: stream i.  symbols_host out: (n_streams, channels, hw) int32. */
int cae_rans_decode_batch(cae_model_t *m, const uint8_t *const *bufs, const size_t *lens, int n_streams,
                          int hw, int32_t *symbols_host, int threads);

/* ---- device entropy coding (opt-in) -----------------------------------------------------------
 * The same streams, byte for byte, coded by HIP kernels (csrc/cae_rans_device.hip): one stream per lane, the
 * handle's tables (cae_model_set_entropy) kept on the device and re-uploaded into a fresh buffer after every table
 * change.  Launches are asynchronous on `stream`; the per-stream results are valid once that stream's work is done.
 * Shapes: n_streams 1..65535 (one grid row per stream; CAE_ERR_ARG otherwise: split larger batches), hw >= 1, CDF rows
 * of at most 4096 entries (else CAE_ERR_UNSUPPORTED).  Argument errors return CAE_ERR_ARG before anything touches the
 * device.
 *
 * Encode: symbols_dev (n_streams, channels, hw) int32 -> the streams packed densely into out_dev (stream i =
 * out_dev[offsets_dev[i] .. offsets_dev[i+1]), offsets_dev int64 [n_streams + 1]); status_dev int32 [n_streams] per
 * stream: CAE_OK, CAE_ERR_ARG (a symbol outside the codable range, as the host coder), CAE_ERR_NOMEM (the workspace's
 * word region or out_capacity was too small: repeat with more).  out_dev and workspace_dev 16-byte aligned.  The
 * workspace holds a header plus one capacity region of (exact coder steps + 2) words per stream;
 * cae_rans_encode_workspace gives the size for one word per symbol (enough unless escapes are frequent). */
int cae_rans_encode_workspace(cae_model_t *m, int n_streams, int hw, size_t *bytes);
int cae_rans_encode_device(cae_model_t *m, const int32_t *symbols_dev, int n_streams, int hw, uint8_t *out_dev,
                           size_t out_capacity, int64_t *offsets_dev, int32_t *status_dev, void *workspace_dev,
                           size_t workspace_bytes, void *stream);
/* Decode: bytes_dev[0 .. bytes_len) holds stream i at [offsets_dev[i], offsets_dev[i+1]) -> symbols_dev
 * (n_streams, channels, hw) int32; status_dev per stream: CAE_OK or CAE_ERR_CORRUPT (shorter than the 8-byte coder
 * state, a read past the stream's end, a bypass count above 8, or offsets outside the buffer). */
int cae_rans_decode_device(cae_model_t *m, const uint8_t *bytes_dev, size_t bytes_len, const int64_t *offsets_dev,
                           int n_streams, int hw, int32_t *symbols_dev, int32_t *status_dev, void *stream);

/* ---- codec front door -------------------------------------------------------------------
 * The reference's numcodecs plugin contract as C entry points: ConvolutionalAutoencoder.encode
 * (_autoencoders.py:539-555: (h,w,c) uint8 chunk -> '>QQ' header + rANS payload) and .decode (:557-584: chunk bytes ->
 * (H,W,c) uint8 tile), one chunk per call, called CONCURRENTLY from dask's thread pool on one shared codec
 * (compress.py:121-128, decompress.py:51-58).  Both calls block and are thread-safe without any caller-side lock.  The
 * range coder of a chunk runs in the calling thread; the GPU parts of the calls that are waiting at the same time are
 * launched as ONE batch (chunks of equal shape, at most max_batch) as soon as one of `inflight` device-side slots is
 * free -- no timer: a lone caller is served at once.  Results do not depend on the grouping.
 *
 * analysis / synthesis: the two track handles of the codec (cae_model_set_layer ... and cae_model_set_entropy done on
 * BOTH: the encode side codes with the analysis handle's tables, the decode side with the synthesis handle's); the
 * door does not own them, they must outlive it and must not be re-configured while calls are in flight.  The handles
 * stay usable through the other entry points on any stream (calls on a handle are ordered on the device in call
 * order).  max_batch <= 0: 32; inflight <= 0: 3.  HIP device = the calling thread's current device.
 * cae_door_destroy serves the queued calls first; no call may be running or started once it has been entered. */
typedef struct cae_door cae_door_t;
int cae_door_create(cae_model_t *analysis, cae_model_t *synthesis, int max_batch, int inflight, cae_door_t **out);
void cae_door_destroy(cae_door_t *door);
/* Codec.encode: tile_host (h,w,c) uint8 C-contiguous (any host memory).  *out: library-allocated chunk (cae_free) =
 * 16-byte big-endian (h,w) header + rANS payload, *out_len its length. */
int cae_door_encode(cae_door_t *door, const uint8_t *tile_host, int h, int w, int c, uint8_t **out, size_t *out_len);
/* Shape of the tile a chunk decodes to: H = (h >> L) << L as the reference derives the latent size (floor, :565). */
int cae_door_decode_shape(cae_door_t *door, const uint8_t *chunk_host, size_t len, int *h, int *w, int *c);
/* Codec.decode: chunk bytes -> out_host (H,W,c) uint8 (capacity in bytes >= H*W*c). */
int cae_door_decode(cae_door_t *door, const uint8_t *chunk_host, size_t len, uint8_t *out_host, size_t out_capacity);
/* Counters since creation / the last reset: batches launched, chunks served, batches repeated on the fp32 kernels,
 * then seconds summed over the calls: caller staging (copy into pinned memory / range decode), caller waiting, caller
 * coding (range encode / copy out), and the waiting time split into queue, launch, device, pull (DMA to the host) and
 * wake-up; last: the calls waiting in the queue right now. */
enum cae_door_stat {
    CAE_DOOR_STAT_BATCHES = 0, CAE_DOOR_STAT_CHUNKS, CAE_DOOR_STAT_FP32_REPEATS, CAE_DOOR_STAT_T_STAGE,
    CAE_DOOR_STAT_T_WAIT, CAE_DOOR_STAT_T_CODE, CAE_DOOR_STAT_T_QUEUE, CAE_DOOR_STAT_T_LAUNCH, CAE_DOOR_STAT_T_DEVICE,
    CAE_DOOR_STAT_T_PULL, CAE_DOOR_STAT_T_WAKE, CAE_DOOR_STAT_QUEUED, CAE_DOOR_STATS
};
int cae_door_stats(cae_door_t *door, double *stats /* n */, int n, int reset);
/* on != 0: the dispatcher starts no further batch (calls queue up; CAE_DOOR_STAT_QUEUED = the number waiting); 0: it
 * resumes.  Lets a caller -- and the tests -- form batches deterministically. */
int cae_door_hold(cae_door_t *door, int on);

/* ---- segmentation head -------------------------------------------------------------------------
 * Eval-mode inference of the reference's JNet (models/tasks/_segmenters.py:307-328): the synthesis track of a UNet
 * on the quantised latents and the decoder's per-level features ("bridges").  A handle of its own, separate from
 * the codec model.
 *
 * Arithmetic.  Bottleneck: 1x1 conv (no bias) on the raw latents, GN, ReLU, 3x3 zero-padded conv, GN, ReLU, 2x2
 * stride-2 transposed conv (bias).  Level i: [projection of bridge i: GN, ReLU, 3x3 conv, GN, ReLU; concatenated in
 * front of the running features], 3x3 conv, GN, ReLU, 3x3 conv, GN, ReLU, [2x2 stride-2 transposed conv (bias); not
 * at the last level]; then fc, a 1x1 conv with bias.  GN = GroupNorm with one group per channel: per (sample,
 * channel) the mean and the BIASED variance of the plane, eps 1e-5 inside the root, affine (gamma, beta).  The kernels
 * keep raw fp32 convolution outputs between layers; the consumer stages v = max(fmaf(a, x, b), 0) with
 * a = gamma rstd, b = beta - mean a (one fp32 fmaf, one max), splits v into f16 halves and contracts on
 * v_mfma_f32_32x32x16_f16 (f16x3, ACCURACY above).  Statistics are Welford partials per output tile (sums in
 * double) merged in tile order (Chan, running values in double); nothing is accumulated with atomics: results are
 * bitwise repeatable.  The inputs are never written.
 *
 * VALID RANGE.  Every staged value v (raw latents, transposed-convolution outputs, normalised activations) must be
 * finite with |v| <= 65504.  The staging code raises the call's overflow word otherwise (also on NaN).  The head has
 * no fp32 twin yet: after the stream work of the call has completed, cae_seg_range_check(h, cae_seg_last_ticket())
 * returns CAE_ERR_RANGE for such a call and its logits must not be used.  Weights, gamma and beta outside the f16
 * range are refused by cae_seg_create (CAE_ERR_ARG).  1024 calls per handle are tracked.
 *
 * cae_seg_config: level_channels[i] = channels of level i's unit, up_channels[i] = output channels of its transposed
 * convolution (i < levels - 1; must equal level_channels[i + 1]); the bottleneck's transposed convolution writes
 * level_channels[0]; bridge_channels[i] = channels of bridge i (used when concat_bridges).
 * The stages (one per convolution, in launch order) and the order of the weights are what cae_seg_plan returns: the
 * weights are host arrays in the reference's layouts, stage after stage, n_weights per stage as
 * [_bn1 gamma beta of the bridge's projection] weight [bias] [gamma beta of the GroupNorm behind it]. */
typedef struct cae_seg cae_seg_t;
typedef struct {
    int channels_bn, seg_channels_bn, levels, num_classes, concat_bridges, batch_norm;
    int bridge_channels[8], level_channels[8], up_channels[8];
} cae_seg_config;
/* One stage of the head.  up: the 2x2 stride-2 transposed convolution (ks 1).  norm: a GroupNorm + ReLU follows (applied
 * by the consumer; it has weights only with batch_norm).  bridge: source A is bridge i through the projection's _bn1 and
 * ReLU, -1 otherwise.  src_a_stage / src_b_stage: the stage whose output the source is (A is contracted first); -1: the
 * latents or a bridge, -2: no such source.  src_a_transformed: A is read through its producer's (a, b) and ReLU; B never
 * is.  n_weights: the arrays the stage owns, in the order above. */
typedef struct {
    int ks, cin_a, cin_b, cout, up, biased, norm, bridge, src_a_stage, src_b_stage, src_a_transformed, n_weights;
} cae_seg_stage_info;
/* Needs no device.  Returns the number of stages and fills up to `capacity` records (out may be NULL: just counts), or
 * CAE_ERR_ARG for a config cae_seg_create refuses.  cae_seg_weight_count is the sum of n_weights. */
int cae_seg_plan(const cae_seg_config *cfg, cae_seg_stage_info *out, int capacity);
/* (tests) bytes of the handle's eight workspaces for one cae_seg_forward(n, lh, lw), before rounding; no device.  In
 * order: latents as C8, the two running-feature buffers, the upsampled features, the bridge as C8, its projection, the
 * four (a, b) slots, the statistics partials. */
int cae_seg_workspace_bytes(const cae_seg_config *cfg, int n, int lh, int lw, size_t *out /* 8 */);
/* Optional taps (tests): per stage s of cae_seg_plan raw[s] receives the stage's raw output as NCHW fp32 and ab[s] the
 * (a, b) pairs computed from it, (n, 8 ceil(cout / 8), 2) floats (stages without norm write none); bridge_ab[i] receives
 * the pairs of bridge i, (n, 8 ceil(c / 8), 2).  Any entry may be NULL. */
typedef struct {
    float **raw, **ab, **bridge_ab;
} cae_seg_taps;
int cae_seg_weight_count(const cae_seg_config *cfg);
int cae_seg_create(const cae_seg_config *cfg, const float *const *weights_host, int n_weights, cae_seg_t **out);
void cae_seg_destroy(cae_seg_t *h);
int cae_seg_stage_count(cae_seg_t *h);
/* latents_dev (n, channels_bn, lh, lw), bridges_dev[i] (n, bridge_channels[i], lh 2^(i+1), lw 2^(i+1)) (NULL list when
 * concat_bridges is off), logits_dev (n, num_classes, lh 2^levels, lw 2^levels), all float NCHW on the device.
 * Workspace is owned by the handle and grown on demand; calls on one handle are ordered in call order whatever stream
 * they name. */
int cae_seg_forward(cae_seg_t *h, const float *latents_dev, const float *const *bridges_dev, int n, int lh, int lw,
                    float *logits_dev, const cae_seg_taps *taps, void *stream);
int64_t cae_seg_last_ticket(void); /* thread-local: range ticket of this thread's latest cae_seg_forward */
int cae_seg_range_check(cae_seg_t *h, int64_t ticket); /* CAE_OK, or CAE_ERR_RANGE: the call's logits are invalid */
/* Host packer of the head's weights (tests): halves written by cae_seg_pack, 0 for arguments it refuses.  up: the 2x2
 * stride-2 transposed convolution as four pointwise matrices, rows (2 dy + dx) 8 ceil(cout / 8) + co. */
size_t cae_seg_packed_halves(int cin_a, int cin_b, int cout, int ks, int up);
int cae_seg_pack(const float *w, int cin_a, int cin_b, int cout, int ks, int up, uint16_t *out, size_t capacity);
void cae_seg_tile(int *tx, int *ty); /* output tile of the head's convolution kernel, in pixels */

/* ---- Training the head: backward pass per operation (csrc/cae_seg_train.hip, csrc/cae_kernels_seg_train.hpp) ----
 * All tensors are NCHW fp32 on the device; (a, b) pairs have the layout of cae_seg_taps, (n, 8 ceil(c / 8), 2).  Every
 * entry point is asynchronous on `stream`, returns CAE_ERR_ARG before any launch on bad shapes or NULL pointers and does
 * nothing for n == 0.  Workspaces are the caller's.  flag_dev is a device int the caller zeroed: a staged value outside
 * the valid range of f16x3 (finite, |v| <= 65504) sets it to 1 and the results of the call are then invalid.  Nothing is
 * accumulated with atomics and every merge has a fixed order: results are bitwise repeatable.
 *
 * cae_seg_set_weights: refreshes a handle's packed weights, bias rows, gamma and beta from device tensors, in the order
 * and layouts of cae_seg_create.  It draws a range ticket (cae_seg_last_ticket) of its own: a weight, gamma or beta
 * outside the f16 range makes cae_seg_range_check fail for that ticket, and the handle must not be used until the
 * weights have been set again.
 * cae_seg_pack_dev: cae_seg_pack reading a device weight and writing device halves, byte for byte (flag_dev may be NULL).
 * cae_seg_conv2d: out (n, cout, h, w) = stride-1 zero-padded ks x ks convolution (ks 1 or 3) of v with the device weight
 * w (cout, cin, ks, ks) plus bias (or NULL); v = x (n, cin, h, w) when ab_dev is NULL, else max(fmaf(a, x, b), 0); the
 * forward kernel on freshly packed weights.  With the flipped, transposed weight it is the data gradient of a layer.
 * cae_seg_wgrad: gw (cout, cin_a + cin_b, ks, ks) = sum_{n,y,x} g[n,co,y,x] v[n,ci,y+ky-P,x+kx-P], v the concatenation of
 * up to two sources staged as above (zero outside the plane), products gh vh + gh vl + gl vh on
 * v_mfma_f32_32x32x16_f16 over the pixels.  The pixels are cut into cae_seg_wgrad_splits segments whose partials go to
 * the workspace (cae_seg_wgrad_workspace bytes) and are added in segment order by a second launch.
 * cae_seg_norm_relu_backward: v = relu(GroupNorm_C(x)) of (n, c, hw) planes.  g_u = g_v [fmaf(a, x, b) > 0];
 * dbeta = sum g_u, dgamma = sum g_u xhat over samples and pixels; g_x = gamma rstd (g_u - mean g_u - xhat mean(g_u xhat))
 * per plane, mean and rstd recomputed from x in two passes with double accumulators.  gx_dev may be NULL.  gamma_dev
 * NULL (no normalisation): g_x = g_u only.  Workspace: cae_seg_norm_workspace bytes, 8-byte aligned.
 * cae_seg_channel_sums: out[c] = sum over samples and pixels of g (n, c, hw), double accumulators (bias gradients): plane
 * sums on a fixed tree into the workspace (cae_seg_channel_sums_workspace bytes, 8-byte aligned), then the samples in order. */
int cae_seg_set_weights(cae_seg_t *h, const float *const *weights_dev, int n_weights, void *stream);
int cae_seg_pack_dev(const float *w_dev, int cin_a, int cin_b, int cout, int ks, int up, uint16_t *out_dev, size_t capacity,
                     int *flag_dev, void *stream);
size_t cae_seg_conv2d_workspace(int n, int cin, int cout, int h, int w, int ks);
int cae_seg_conv2d(const float *x_dev, const float *ab_dev, const float *w_dev, const float *bias_dev, int n, int cin,
                   int cout, int h, int w, int ks, float *out_dev, int *flag_dev, void *workspace_dev,
                   size_t workspace_bytes, void *stream);
int cae_seg_wgrad_splits(int n, int h, int w, int cin, int cout, int ks);
size_t cae_seg_wgrad_workspace(int n, int h, int w, int cin, int cout, int ks);
int cae_seg_wgrad(const float *g_dev, const float *xa_dev, const float *aba_dev, int cin_a, const float *xb_dev,
                  const float *abb_dev, int cin_b, int n, int cout, int h, int w, int ks, float *gw_dev, int *flag_dev,
                  void *workspace_dev, size_t workspace_bytes, void *stream);
size_t cae_seg_norm_workspace(int n, int c);
int cae_seg_norm_relu_backward(const float *x_dev, const float *ab_dev, const float *gamma_dev, const float *gv_dev, int n,
                               int c, size_t hw, float *gx_dev, float *dgamma_dev, float *dbeta_dev, void *workspace_dev,
                               size_t workspace_bytes, void *stream);
size_t cae_seg_channel_sums_workspace(int n, int c);
int cae_seg_channel_sums(const float *g_dev, int n, int c, size_t hw, float *out_dev, void *workspace_dev,
                         size_t workspace_bytes, void *stream);

/* ---- Prediction from the head's logits (csrc/cae_seg_predict.hip) ------------------------------
 * What the reference's segmentation harness makes of a model's output (test_cae_classifier.py:46-55 save_pred2zarr,
 * utils/_metrics.py:79-193), in one pass over the logits: class map, optional scores, optional per-image counts.
 * logits_dev (n, c, hw) fp32, the head's NCHW output as it stands (any 4-byte aligned address); target_dev (n, hw)
 * uint8 or NULL; cls_dev (n, hw) uint8; scores_dev (n, c, hw) fp32 or NULL; counts_dev (n, 6) int64 =
 * [tp, tn, fp, fn, p, tp_top] or NULL (needs target_dev).
 *
 * c == 1: cls = logit > t, an exact fp32 compare (false for NaN).  The caller chooses t: the logit of a score
 * threshold, t = (float)log(thr / (1 - thr)) evaluated in double (compute_metrics_per_image compares the sigmoid,
 * _metrics.py:172), or a threshold on the logit itself (save_pred2zarr, test_cae_classifier.py:54).  scores =
 * 1 / (1 + exp(-x)).  The target is binarised as target > 0; counts are the confusion table, p = tp + fn, tp_top = tp.
 * 2 <= c <= 256: cls = index of the largest logit, the lowest index of equal ones (always inside 0..c-1, NaN or not);
 * scores = softmax with the pixel's maximum subtracted; tp = #{cls == target}, fp = fn = hw - tp, tn = 0, p = hw
 * (compute_class_metrics, _metrics.py:94-105); tp_top = #{rank < min(top_k, c)} with rank = #{j : l_j > l_t} +
 * #{j < t : l_j == l_t} of the target's logit l_t.  A target value >= c counts as wrong in tp and tp_top and is never
 * used as an index.
 *
 * Up to 16 classes every logit is read once; above, the planes of a pixel are read three times (the repeats out of the
 * cache).  Counts are exact and bitwise repeatable: integer partials per (image, block) in workspace_dev
 * (cae_seg_predict_workspace bytes, 8-byte aligned; only needed with counts_dev), merged by a second launch in fixed
 * order; no atomics.  Neither outputs nor workspace need initialising.  Launches are asynchronous on `stream`.
 * CAE_ERR_ARG before any launch: c outside 1..256, n < 0, hw < 1, top_k < 1, counts without a target, and for n >= 1
 * a NULL logits_dev / cls_dev or, with counts, a workspace that is NULL, misaligned or too small.  n == 0: CAE_OK,
 * nothing launched.  cae_seg_predict_workspace returns 0 for shapes cae_seg_predict refuses and for n == 0. */
int cae_seg_predict(const float *logits_dev, const uint8_t *target_dev, int n, int c, size_t hw, float t, int top_k,
                    uint8_t *cls_dev, float *scores_dev, int64_t *counts_dev, void *workspace_dev,
                    size_t workspace_bytes, void *stream);
size_t cae_seg_predict_workspace(int n, int c, size_t hw);

/* ---- ROC histograms of a one-class head (csrc/cae_seg_hist.hip) ----------------------------------
 * The threshold-free results of the reference's harness -- the per-image auc (utils/_metrics.py:128-131), the
 * slide-level ROC curve and its AUC (test_cae_classifier.py:233-264, 356-364) -- without sorting a score: the
 * prediction is logit > t, so the curve is fixed by how many positive and how many negative pixels lie at or above each
 * threshold.
 * logits_dev (n, 1, h, w) fp32 contiguous, read where they stand (any 4-byte aligned address); target_dev (n, h, w)
 * uint8 at any address; extent_dev int32 [n][2] = (rows, cols) on the device or NULL: only pixels with y < rows and
 * x < cols are counted, values clamped to 0..h / 0..w, NULL = whole planes.
 *   key:   x' = x + 0.0f (-0 becomes +0), u = the bits of x', key = (u >> 31) ? ~u : (u | 0x80000000); a NaN logit has
 *          key 0: it lies below every threshold, as in cae_seg_predict, where logit > t is false for NaN.
 *   bin:   key >> (32 - bits), 8 <= bits <= 14; monotone in the logit: bin(x) >= j exactly when x >= e_j, the smallest
 *          non-NaN fp32 value of bin j, i.e. x > nextafter(e_j, -inf).  Bins that hold only NaN bit patterns stay
 *          empty, except bin 0.
 *   class: target > 0 is positive, the binarisation of cae_seg_predict.
 *   hist_dev int64 [m][2][2^bits], row 0 the negatives and row 1 the positives; m = n with per_image, else 1 (the sum
 *          over the batch).  Every entry is written, nothing is accumulated into what the buffer held; integers, exact
 *          in any order, and they add across tiles, batches and ranks.
 * From a histogram, with P_j = sum_{b >= j} pos_b and N_j = sum_{b >= j} neg_b: the curve starts at (0, 0) (threshold
 * +inf) and has one point (N_j / N, P_j / P) per non-empty bin from the top down -- exactly the (fp, tp) of
 * cae_seg_predict at t = nextafter(e_j, -inf) -- auc = sum_b pos_b (2 neg_below_b + neg_b) / (2 P N), and the AUC of
 * the unbinned logits lies within auc_slack = sum_b pos_b neg_b / (2 P N) of it (equal when every logit is an e_j).
 *
 * Two launches, asynchronous on `stream`: blocks that count a contiguous span of an image's pixels in an LDS table of
 * 2^(bits+3) bytes and store it as one partial per (image, block) in workspace_dev (cae_seg_roc_workspace bytes,
 * 16-byte aligned), then the sum of the partials in a fixed order.  No global atomics; neither histogram nor workspace
 * needs initialising.  CAE_ERR_ARG before any launch: bits outside 8..14, n < 0, h or w < 1, and for n >= 1 a NULL or
 * misaligned pointer or a workspace that is too small.  n == 0: CAE_OK, nothing launched.  cae_seg_roc_workspace and
 * cae_seg_roc_blocks (blocks per image, for the tests) return 0 for shapes cae_seg_roc_hist refuses and for n == 0. */
int cae_seg_roc_hist(const float *logits_dev, const uint8_t *target_dev, const int32_t *extent_dev, int n, int h, int w,
                     int bits, int per_image, int64_t *hist_dev, void *workspace_dev, size_t workspace_bytes,
                     void *stream);
size_t cae_seg_roc_workspace(int n, int h, int w, int bits);
int cae_seg_roc_blocks(int n, int h, int w, int bits);

/* ---- Score histograms of a head of several classes (csrc/cae_seg_hist.hip) ------------------------
 * What the reference's avg_prec needs -- average_precision_score(one_hot_target, softmax_scores, average='micro')
 * (utils/_metrics.py:90-92) -- without sorting a score: precision and recall at a threshold are fixed by how many
 * positive and how many negative (pixel, class) pairs lie at or above it.
 * scores_dev (n, c, h, w) fp32 contiguous, read as they stand in memory (any 4-byte aligned address): what
 * cae_seg_predict wrote to scores_dev, or any values in [0, 1].  Nothing is recomputed: the histogram is an exact
 * function of these bits.  target_dev (n, h, w) uint8 at any address; extent_dev as for cae_seg_roc_hist.
 *   bin:   B = 2^bits, 8 <= bits <= 14, sh = 31 - bits, u(v) the bits of the float v.
 *          NaN, -0 and s <= 0: bin 0.  0 < s < 0.5: u(s) >> sh.  0.5 <= s < 1: B - 1 - (u(1.0f - s) >> sh); the
 *          subtraction is exact in fp32 (Sterbenz), so no rounding or denormal mode has a say.  s >= 1: B - 1.
 *          u(0.5f) = 0x3F000000 < 2^30: the lower half ends at bin (0x3F000000 >> sh) - 1 and the upper begins at
 *          B - 1 - (0x3F000000 >> sh); the bins between them stay empty.  Monotone non-decreasing in s, with relative
 *          resolution near 0 and near 1: bin(s) >= j exactly when s >= e_j, the smallest score of bin j.
 *   class: for class k the pair (pixel, k) is positive when target == k and negative otherwise.  A pixel whose target
 *          is >= c is unlabelled: it is in no histogram, of no class.  Pixels outside the extent are in none either.
 *   hist_dev int64 [n if per_image else 1][c if per_class else 1][2][2^bits], row 0 the negatives and row 1 the
 *          positives.  The sum over the classes is the micro histogram (positives: the ones of the one-hot target).
 *          Every entry is written, nothing is accumulated into what the buffer held; integers, exact in any order, and
 *          they add across tiles, batches and ranks.
 * From a histogram, walking the non-empty bins from the top down with TP, FP the totals above bin b, p_b and n_b its
 * counts and P = sum p_b: avg_prec = (1 / P) sum_b p_b (TP + p_b) / (TP + FP + p_b + n_b) is the average precision of
 * the scores snapped to their bins (the ties of a bin form one threshold), and that of the unbinned scores lies in
 * [(1 / P) sum_b (p_b - (FP + n_b) ln((T + p_b) / T)), (1 / P) sum_b p_b (TP + p_b) / (TP + FP + p_b)], T = TP + FP + n_b
 * (the term is p_b where T = 0), whatever the order and the ties inside a bin.
 *
 * Two launches, asynchronous on `stream`: blocks that count a contiguous span of one class plane in an LDS table of
 * 2^(bits+3) bytes and store it as one partial per (plane, block) in workspace_dev (cae_seg_score_workspace bytes,
 * 16-byte aligned), then the sum of the partials in a fixed order.  Each plane reads its image's target: 4 c + c bytes
 * per pixel in all.  No global atomics, no floating-point atomics; neither histogram nor workspace needs initialising;
 * results are bitwise repeatable.  CAE_ERR_ARG before any launch: bits outside 8..14, c outside 2..255, n, h or w < 1,
 * planes of more than 2^31 - 1 pixels, a NULL or misaligned pointer, a workspace that is too small.
 * cae_seg_score_workspace returns 0 for shapes cae_seg_score_hist refuses. */
int cae_seg_score_hist(const float *scores_dev, const uint8_t *target_dev, const int32_t *extent_dev, int n, int c, int h,
                       int w, int bits, int per_image, int per_class, int64_t *hist_dev, void *workspace_dev,
                       size_t workspace_bytes, void *stream);
size_t cae_seg_score_workspace(int n, int c, int h, int w, int bits);

/* ---- Objects of a label plane (csrc/cae_seg_objects.hip) -----------------------------------------
 * The object-level half of the reference's harness (--compute-components-metrics, test_cae_classifier.py:97-157 and
 * 267-370): every connected object of the target gets a bounding box, and counts and ROC curve are taken over the pixels
 * of all boxes.  Four entry points; all results are integers and bitwise repeatable.
 *
 * cae_seg_components: target_dev (n, h, w) uint8 at any byte address -> labels_dev (n, h, w) int32 and n_objects_dev
 * int64 [n].  A pixel is foreground when target > 0 and it lies inside the extent (extent_dev int32 [n][2] = (rows,
 * cols) on the device, clamped to 0..h / 0..w as in cae_seg_roc_hist, NULL = whole planes).  Foreground pixels that
 * touch by an edge or a corner (8-connected) belong to one object; with by_value != 0 only when their values are equal
 * (skimage.measure.label of an integer image).  The label of a pixel is 0 on background, else 1 + the smallest
 * row-major index y w + x of its object: canonical, independent of launch shapes and execution order.  n_objects_dev[i]
 * is the number of objects of plane i.  Objects never reach across planes.
 *
 * cae_seg_object_cover: labels_dev as cae_seg_components writes them (same extent) -> cover_dev (n, h, w) uint16, the
 * number of objects of the plane whose box contains the pixel.  Box of an object with pixel rows ymin..ymax and columns
 * xmin..xmax (test_cae_classifier.py:101-109): rows max(0, ymin - 1) .. min(rows, ymax + 2), columns max(0, xmin - 1) ..
 * min(cols, xmax + 2), end exclusive, (rows, cols) the extent.  The reference concatenates the pixels of every box, so a
 * pixel inside k boxes counts k times: every object-level sum is the image-level sum weighted by the cover.
 * cover <= 3 min(h, w) (objects are disjoint, and one whose widened column range holds x has a pixel in columns
 * x-1..x+1), which is why planes with 3 min(h, w) > 65535 are refused.  A label that does not name a root pixel of its
 * plane, or whose root pixel lies outside the extent (labels made with another extent), is ignored, as is every pixel
 * outside the extent; no label is used as an index before it is checked.
 *
 * cae_seg_object_counts: the [tp, tn, fp, fn, p, tp_top] record of cae_seg_predict with every pixel counted cover
 * times, by cae_seg_predict's rules (logit > t; lowest-index argmax, the rank rule of tp_top, a target >= c is wrong);
 * several classes: fp = fn = sum(cover) - tp, tn = 0, p = sum(cover).  logits_dev (n, c, hw) fp32 4-byte aligned,
 * target_dev (n, hw) uint8, cover_dev (n, hw) uint16: any values, not only a cover's.
 *
 * cae_seg_object_roc_hist: the histogram of cae_seg_roc_hist (same key, bin, NaN rule, extent and layout) with every
 * pixel adding its cover instead of 1.
 *
 * Weighted sums are exact for every uint16 weight: lane tallies, block partials and results are 64 bits wide; the one
 * 32-bit accumulator, a block's LDS histogram, is added into the block's 64-bit partial and cleared after at most 65536
 * pixels (65536 x 65535 < 2^32).  Integer global atomics (min / max / add) only: exact in any order.  No launch waits
 * for another block; every walk of the union-find strictly descends (parent <= index at all times).  Neither outputs
 * nor workspaces need initialising; workspaces (the _workspace queries; 8-byte aligned) hold nothing between calls.
 * Launches are asynchronous on `stream`.  CAE_ERR_ARG before any launch: n < 0, h / w / hw < 1, 3 min(h, w) > 65535 or
 * h w > 2^31 - 1 (components, cover), c outside 1..256, top_k < 1, bits outside 8..14, and for n >= 1 a NULL or
 * misaligned pointer or a workspace that is too small.  n == 0: CAE_OK, nothing launched.  The queries return 0 for
 * refused shapes and for n == 0. */
int cae_seg_components(const uint8_t *target_dev, const int32_t *extent_dev, int n, int h, int w, int by_value,
                       int32_t *labels_dev, int64_t *n_objects_dev, void *workspace_dev, size_t workspace_bytes,
                       void *stream);
size_t cae_seg_components_workspace(int n, int h, int w);
int cae_seg_object_cover(const int32_t *labels_dev, const int32_t *extent_dev, int n, int h, int w, uint16_t *cover_dev,
                         void *workspace_dev, size_t workspace_bytes, void *stream);
size_t cae_seg_object_cover_workspace(int n, int h, int w);
int cae_seg_object_counts(const float *logits_dev, const uint8_t *target_dev, const uint16_t *cover_dev, int n, int c,
                          size_t hw, float t, int top_k, int64_t *counts_dev, void *workspace_dev,
                          size_t workspace_bytes, void *stream);
size_t cae_seg_object_counts_workspace(int n, int c, size_t hw);
int cae_seg_object_roc_hist(const float *logits_dev, const uint8_t *target_dev, const uint16_t *cover_dev,
                            const int32_t *extent_dev, int n, int h, int w, int bits, int per_image, int64_t *hist_dev,
                            void *workspace_dev, size_t workspace_bytes, void *stream);
size_t cae_seg_object_roc_workspace(int n, int h, int w, int bits);

/* ---- Weight map of a label plane (csrc/cae_seg_distances.hip) -------------------------------------
 * The reference's WeightsDistances (utils/datasets/_augs.py:102-136), the U-Net border weight
 *   w = class_weights[target] + w_0 exp(-(d1 + d2)^2 / (2 sigma^2)),
 * d1 and d2 the Euclidean distances of the pixel to the nearest and to the second-nearest object of its plane.  The
 * reference runs one full-plane distance transform per object; here the two distances of every pixel come out of two
 * passes whatever the number of objects.
 *
 * cae_seg_object_distances: labels_dev (n, h, w) int32 as cae_seg_components writes them (0 is background, any other
 * value names an object; only that labels differ matters) -> d2_dev (n, 2, h, w) int32.  Plane 0: the squared Euclidean
 * distance to the nearest foreground pixel, 0 on foreground.  Plane 1: the smallest squared distance to a pixel of an
 * object other than the one that gives plane 0 (with equal distances to two objects both planes hold that value).  -1
 * where no such object exists: plane 1 of a plane with one object, both planes of an empty plane.  Exact integers,
 * bitwise repeatable: both are minima over sets that do not depend on the order of evaluation.
 *   Column pass (one lane per column): for every pixel the two nearest foreground pixels of its column that carry
 * distinct labels, as (squared row distance, label) records, from one downward and one upward scan that each keep the
 * latest label and the latest different label.  Two labels per (row, column) are enough: a pixel hidden behind two
 * other labels of its column is farther than both, and one of the two differs from the nearest object.
 *   Row pass (one lane per pixel): the smallest (x - x')^2 + record over both records of all columns x' of the pixel's
 * row, and the smallest of a label other than the best one's; the records pass through LDS in chunks of 256 columns, so
 * w is not bounded by LDS.  w times 2 candidates per pixel.
 *   workspace_dev: cae_seg_object_distances_workspace bytes (16 per pixel), 16-byte aligned.  Neither the output nor
 * the workspace needs initialising.  No atomics; no block waits for another.  Two launches, asynchronous on `stream`.
 * CAE_ERR_ARG before any launch: n < 0, h or w outside 1..32768 (so that every squared distance is below 2^31 - 1),
 * h w > 2^31 - 1, and for n >= 1 a NULL or misaligned pointer or a workspace that is too small.  n == 0: CAE_OK, nothing
 * launched.  The query returns 0 for refused shapes and for n == 0.
 *
 * cae_seg_weight_map: target_dev (n, hw) fp32 holding integer label values (what cae_t_sample_labeled_patches writes),
 * d2_dev as above, n_objects_dev int64 [n] of cae_seg_components, class_weights_dev fp32 [n_class_weights] -> out_dev
 * (n, 2, hw) fp32: plane 0 the weight, plane 1 the target, copied -- the concatenation the reference's weighted loss
 * (BCEWeightedClassLoss) takes.  With k = (int)target, cw = class_weights[k] and d_i = (float)sqrt((double)d2_i), the correctly
 * rounded double root rounded once to fp32 (scipy's float64 distance cast to float32):
 *   n_objects == 0: w = cw
 *   n_objects == 1: w = cw + w_0 expf(-(d_0 d_0) / sigma_2)
 *   n_objects >= 2: w = cw + w_0 expf(-((d_0 + d_1) (d_0 + d_1)) / sigma_2)
 * every operation rounded to fp32 on its own (no fused multiply-add); sigma_2 = 2 sigma^2 is formed by the caller.  An
 * exponential below 2^-126 may be flushed to zero.  A target that is NaN, negative or >= n_class_weights writes NaN as
 * its weight and sets *flag_dev to 1; flag_dev is a device int the caller zeroed, as in the head-training entry points.
 * No target is used as an index before it is checked.  One launch, asynchronous on `stream`.  CAE_ERR_ARG before any
 * launch: n < 0, hw < 1, n_class_weights < 1, sigma_2 not finite and positive, and for n >= 1 a NULL pointer.  n == 0:
 * CAE_OK, nothing launched. */
int cae_seg_object_distances(const int32_t *labels_dev, int n, int h, int w, int32_t *d2_dev, void *workspace_dev,
                             size_t workspace_bytes, void *stream);
size_t cae_seg_object_distances_workspace(int n, int h, int w);
int cae_seg_weight_map(const float *target_dev, const int32_t *d2_dev, const int64_t *n_objects_dev,
                       const float *class_weights_dev, int n_class_weights, float sigma_2, float w_0, int n, size_t hw,
                       float *out_dev, int *flag_dev, void *stream);

/* ---- Tissue mask of a slide (csrc/cae_mask.hip) ----------------------------------------------------
 * The reference's scripts/compute_mask.py on the device: gray, Otsu threshold, small objects out, small holes in,
 * dilation by a disk -- with the labelling of cae_seg_components and the distances of cae_seg_object_distances between
 * the kernels here.  All results are integers or float64 values rounded operation by operation: functions of the input
 * alone, bitwise repeatable.  The host makes the threshold from the 256 counts (tissue.otsu_threshold).
 *
 * cae_mask_gray: img_dev (n, hw, 3) uint8 -> gray_dev (n, hw) float64 and minmax_dev float64 [n][2] = (min, max) of each
 * plane.  gray = (0.2125 r + 0.7154 g) + 0.0721 b with r = R / 255.0 (likewise g, b), every operation rounded on its
 * own.  Gray is never negative, so the range is an integer min / max over the bit patterns.
 *
 * cae_mask_hist: gray_dev and edges_dev float64 [n][257] (numpy.linspace(min, max, 257) of each plane, made by the
 * caller) -> counts_dev int64 [n][256], the counts of numpy.histogram(gray, 256): bin = (int)((x - e[0]) (256 / (e[256]
 * - e[0]))), 256 becomes 255, then one step down where x < e[bin] and one step up where x >= e[bin + 1] below the last
 * bin.  The bin is clamped to 0..255 before it is an index.  A block counts in 32-bit LDS bins and folds them into 64-bit
 * sums every cae_mask_hist_fold() pixels; blocks write partials that a second launch sums.  A plane with min == max
 * gives no meaningful counts (the caller's threshold is then the value itself).
 *
 * cae_mask_threshold: plane_dev (n, hw) uint8 = gray <= thr_dev[n] (float64 [n]), 1 or 0.
 *
 * cae_mask_label: plane_dev (n, h, w) uint8 -> labels_dev (n, h, w) int32 as cae_seg_components writes them (0, or 1 +
 * the smallest row-major index of the object), with connectivity 4 (edges) or 8 (edges and corners).  Foreground is
 * plane != 0, or with of_zero != 0 plane == 0: the objects of the complement.
 *
 * cae_mask_area_filter: labels_dev of cae_mask_label -> every pixel of plane_inout_dev (n, h, w) uint8 whose object has
 * fewer than min_area pixels becomes set_value (0 or 1).  Areas stand in an int32 array addressed by the root pixel
 * (workspace: cae_mask_area_workspace bytes, 4-byte aligned): one launch clears the roots' entries, one counts -- the
 * first lane of every run of equal labels among a wave's 64 consecutive pixels adds the run's length, and a run that
 * goes on into the wave's next 64 pixels is carried there before it is added -- and one rewrites.
 * wide_out_dev (n, h, w) int32, or NULL: the resulting plane as 0 / 1, the form cae_seg_object_distances reads.  A
 * label that does not name a root pixel of its plane is ignored; no label is an index before that is checked.
 *
 * cae_mask_within: d2_dev (n, 2, h w) int32 of cae_seg_object_distances -> plane_dev (n, hw) uint8 = 0 <= d2[n][0] <= r2:
 * the dilation by the disk dx^2 + dy^2 <= r2 (an empty plane, all -1, stays empty).
 *
 * cae_mask_downscale: img_dev uint8, n images of h x w pixels of c channels (1..4), rows row_pitch bytes and images
 * plane_pitch bytes apart -> out_dev (n, ceil(h / f), ceil(w / f), c) uint8, dense: the mean of the f x f block (f in
 * 1..64; only the real pixels of a block on the lower or right edge), (2 sum + count) / (2 count) in integers.
 *
 * Neither outputs nor workspaces need initialising.  Launches are asynchronous on `stream`.  CAE_ERR_ARG before any
 * launch: n < 0, hw / h / w < 1, hw or h w > 2^31 - 1, planes beyond 3 min(h, w) <= 65535 or h, w <= 32768 (label, area
 * filter), connectivity not 4 or 8, min_area < 0, set_value not 0 or 1, r2 < 0, c outside 1..4, f outside 1..64, pitches
 * shorter than a row or an image, and for n >= 1 a NULL or misaligned pointer or a workspace that is too small.  n == 0:
 * CAE_OK, nothing launched.  The queries return 0 for refused shapes and for n == 0. */
int cae_mask_gray(const uint8_t *img_dev, int n, size_t hw, double *gray_dev, double *minmax_dev, void *stream);
int cae_mask_hist(const double *gray_dev, const double *edges_dev, int n, size_t hw, int64_t *counts_dev,
                  void *workspace_dev, size_t workspace_bytes, void *stream);
size_t cae_mask_hist_workspace(int n, size_t hw);
size_t cae_mask_hist_fold(void);
int cae_mask_threshold(const double *gray_dev, const double *thr_dev, int n, size_t hw, uint8_t *plane_dev, void *stream);
int cae_mask_label(const uint8_t *plane_dev, int n, int h, int w, int connectivity, int of_zero, int32_t *labels_dev,
                   void *workspace_dev, size_t workspace_bytes, void *stream);
size_t cae_mask_label_workspace(int n, int h, int w);
int cae_mask_area_filter(const int32_t *labels_dev, int n, int h, int w, int min_area, int set_value,
                         uint8_t *plane_inout_dev, int32_t *wide_out_dev, void *workspace_dev, size_t workspace_bytes,
                         void *stream);
size_t cae_mask_area_workspace(int n, int h, int w);
int cae_mask_within(const int32_t *d2_dev, int n, size_t hw, int r2, uint8_t *plane_dev, void *stream);
int cae_mask_downscale(const uint8_t *img_dev, int n, int h, int w, int c, size_t row_pitch, size_t plane_pitch, int f,
                       uint8_t *out_dev, void *stream);

/* ---- Byte histograms of tiles (csrc/cae_tiles.hip) -------------------------------------------------
 * The look a sparse slide takes at the tiles its tissue mask calls background (zarrio.compress_image with a mask): the
 * squared error of a tile against any fill value is a function of the tile's 256 byte counts.
 * tiles_dev: n contiguous (h, w, c) uint8 tiles, c in 1..4, read where they stand (any byte address).  extent_dev int32
 * [n][2] = (rows, cols) on the device or NULL: only samples with y < rows and x < cols are counted, all c channels of
 * them, values clamped to 0..h / 0..w, NULL = whole tiles (the convention of cae_seg_roc_hist); rows beyond `rows` are
 * never loaded.
 *   hist_dev int64 [n][256]: hist[i][v] = the number of counted samples of tile i with value v.  Every entry is written
 *   on every call, nothing is accumulated into what the buffer held; integers, exact in any order, and
 *   sum_v hist[i][v] = rows_i cols_i c.
 * Two launches, asynchronous on `stream`: blocks that count a contiguous span of a tile's bytes in a uint32 [256] LDS
 * table and store it as one partial per (tile, block) in workspace_dev (cae_tile_byte_hist_workspace bytes, 16-byte
 * aligned), then the sum of the partials in a fixed order.  No global atomics; neither histogram nor workspace needs
 * initialising.  The blocks of a launch are capped, so on large batches a block's lanes take many turns.
 * CAE_ERR_ARG before any launch: n < 0, h or w < 1, c outside 1..4, h w c so large that a block's span would leave 32
 * bits, and for n >= 1 a NULL tiles or histogram pointer, a misaligned extent (4) or histogram (8), or a workspace that
 * is NULL, not 16-byte aligned or too small.  n == 0: CAE_OK, nothing launched.  cae_tile_byte_hist_workspace and
 * cae_tile_byte_hist_blocks (blocks per tile, for the tests) return 0 for shapes cae_tile_byte_hist refuses and for
 * n == 0. */
int cae_tile_byte_hist(const uint8_t *tiles_dev, const int32_t *extent_dev, int n, int h, int w, int c, int64_t *hist_dev,
                       void *workspace_dev, size_t workspace_bytes, void *stream);
size_t cae_tile_byte_hist_workspace(int n, int h, int w, int c);
int cae_tile_byte_hist_blocks(int n, int h, int w, int c);

#ifdef __cplusplus
}
#endif
#endif /* CAE_HIP_H */
