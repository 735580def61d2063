/*
 * wxengine — C ABI of the MI355X-native CrossFormer/WXFormer rollout engine.
 *
 * This is the drop-in boundary for ONE hot path of NCAR/miles-credit: one
 * autoregressive forecast step of `model.type: crossformer`
 * (credit/models/crossformer.py:593-644 CrossFormer.forward, driven by
 *  credit/applications/rollout_to_netcdf.py:274-310).  Plain pointers and sizes
 * only; no torch types.  All `*_dev` pointers are device (HBM) pointers on the
 * GPU the handle was created for; `stream` is a hipStream_t passed as void*
 * (NULL = the default stream).  Every function returns 0 on success and a
 * negative wx_status otherwise; wx_last_error() gives the message (thread-local).
 *
 * The reference is pure Python, so "the reference's FFI for this path" is the
 * model-registry call surface; each entry point cites the
 * reference interface it stands in for.  The ctypes binding a maintainer would add
 * is shown in INTEGRATION.md and implemented in miles-credit_amd/wxengine/engine.py.
 */
#ifndef WXENGINE_H
#define WXENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WX_ABI_VERSION 3

typedef struct wx_engine* wx_handle;

enum wx_status {
  WX_OK = 0,
  WX_ERR_INVALID = -1,     /* bad argument / unsupported configuration (reference: ValueError) */
  WX_ERR_STATE = -2,       /* call order violated, e.g. forward before finalize (RuntimeError) */
  WX_ERR_HIP = -3,         /* a HIP runtime call failed */
  WX_ERR_MISSING = -4,     /* a required state-dict tensor was never loaded */
  WX_ERR_SHAPE = -5        /* tensor shape does not match the configuration */
};

enum wx_arch {
  WX_ARCH_CROSSFORMER = 0, /* credit/models/crossformer.py (model.type: crossformer): ConvTranspose decoder */
  WX_ARCH_WXFORMER = 1,    /* credit/models/wxformer/crossformer.py (model.type: wxformer / wxformer_base): sub-pixel conv
                              + PixelShuffle decoder, ZeroPad2d-wrapped CrossEmbed branches (keys convs.<i>.1.*) */
  WX_ARCH_CROSSFORMER_UPCONV = 2, /* credit/models/crossformer.py with upsample_v_conv=True (:87-92, :560-570): every decoder
                              up-sampling is nn.Upsample(2x bilinear, align_corners=False) + Conv3x3 instead of ConvTranspose */
  WX_ARCH_CAMULATOR = 3    /* credit/models/camulator.py (model.type: camulator): the legacy CrossEmbed (bare Conv2d, keys convs.<i>.*)
                              in front of the wxformer decoder, whose `sharp` convs carry no spectral norm here; frames == 2 enters as
                              the mean of the two frames (F.avg_pool3d), so the first conv takes channels * levels + surface +
                              input_only channels whatever `frames` is.  frames <= 2, no noise layers, not in lat-band mode */
};

enum wx_precision {
  WX_PREC_FP32 = 0,        /* f32 storage, exact-f32 MFMA (v_mfma_f32_16x16x4_f32) */
  WX_PREC_BF16 = 1,        /* bf16 storage + bf16 MFMA, fp32 accumulate / LN / softmax / GN */
  WX_PREC_FP32_SPLIT = 2   /* f32 storage; LayerNorm / GroupNorm / softmax statistics (max, sum, exp on v_exp_f32) in fp32 as in WX_PREC_FP32;
                            * every implicit GEMM as split-bf16 arithmetic: x = x_hi + x_lo, W = W_hi + W_lo, three
                            * v_mfma_f32_16x16x32_bf16 per product (hi.hi + hi.lo + lo.hi), fp32 accumulate -- the fast mode that still
                            * meets the fp32 tolerance against the reference (whose inference is fp32 with TF32 off, credit/seed.py:24-25).
                            * The CrossFormer window attention's two products (Q.K^T and P.V) run in the same three-MFMA form, with the
                            * position bias and the softmax statistics exact, for windows of 17 - 32, 33 - 64, 97 - 112 and 113 - 128
                            * tokens with dim_head 32 on the LDS bias-table path (key-fragment counts 2 / 4 / 7 / 8: every multi-token
                            * window of BASELINE configs 1 - 4); any other window size or head width falls back to the exact-f32 MFMA
                            * products of WX_PREC_FP32.  wx_create (incl. lat-band mode), wx_swin_create and wx_fuxi_create take the mode
                            * (the Swin / FuXi attention kernels stay exact fp32); wx_winattn_create takes FP32 / BF16. */
};

/* The YAML `model:` mapping of the reference constructor
 * (credit/models/crossformer.py:372-401), flattened. */
typedef struct wx_config {
  int32_t abi_version;              /* must be WX_ABI_VERSION */
  int32_t image_height, image_width;
  int32_t frames, output_frames;
  int32_t channels, surface_channels, input_only_channels, output_only_channels, levels;
  int32_t dim[4], depth[4], dim_head;   /* dim_head: 32 (reference default, tuned kernels) or 64 / 128 (general attention kernel); must divide every dim[s].
                                         * 96 exists for wx_winattn_create / wx_swin_create only: no width wx_create takes is a multiple of it.
                                         * dim[s]: a multiple of 32 that doubles per stage and that the LayerNorm kernels take -- 32 / 64 / 128 at
                                         * stage 0 (dim[3] <= 1024), and 256 (dim[3] = 2048) with WX_PREC_BF16; anything else is WX_ERR_INVALID at wx_create */
  int32_t global_window_size[4], local_window_size[4];
  int32_t n_embed_kernels[4];       /* branches per stage (<= 4) */
  int32_t embed_kernels[4][4];      /* cross_embed_kernel_sizes */
  int32_t embed_strides[4];         /* cross_embed_strides */
  int32_t pad_activate;             /* padding_conf: 0 off, 1 mode "earth" (pole flip + 180-degree roll, boundary_padding.py:50-72),
                                       2 mode "mirror" (reflect latitudes, wrap longitudes, :98-117) */
  int32_t pad_lat[2], pad_lon[2];
  int32_t interp;                   /* bilinear resize to (image_height, image_width) */
  int32_t use_spectral_norm;
  int32_t precision;                /* enum wx_precision */
  int32_t max_batch;                /* largest B accepted by wx_forward (>= 1) */
  int32_t arch;                     /* enum wx_arch: which reference class the state dict belongs to */
  /* the noise-injection ensemble (model.type crossformer-ensemble: credit/models/wxformer/crossformer_ensemble.py CrossFormerWithNoise,
     a subclass of the legacy CrossFormer; arch WX_ARCH_CROSSFORMER or WX_ARCH_CROSSFORMER_UPCONV only, not in lat-band mode) */
  int32_t noise_latent_dim;         /* 0 = deterministic model (no noise layers, no extra launches); > 0: Linear(noise_latent_dim, C) styles */
  int32_t encoder_noise;            /* noise layers after encoder stages 0, 1, 2 (keys encoder_noise_layers.{0,1,2}.*) */
  int32_t noise_correlated;         /* one latent z per forward shared by every layer, else a fresh z per layer */
} wx_config;

/* ---- lifecycle -----------------------------------------------------------
 * wx_create      <-> CrossFormer.__init__ via load_model(conf)          (credit/models/__init__.py:301-387)
 * wx_load_tensor <-> nn.Module.load_state_dict(strict=False) per key    (credit/models/base_model.py:57-87)
 * wx_finalize_weights: folds spectral norm (eval-mode W = weight_orig / (u.(W v)),
 *                crossformer.py:23-26), LayerNorm affine into the following 1x1 conv,
 *                evaluates every DynamicPositionBias MLP once (crossformer.py:279-286),
 *                and repacks weights into the MFMA operand layout in HBM.
 * wx_destroy     <-> del model
 */
int wx_create(const wx_config* cfg, int device, wx_handle* out);
int wx_load_tensor(wx_handle h, const char* state_dict_key, const float* host_data, int ndim,
                   const int64_t* shape);
int wx_finalize_weights(wx_handle h);
int wx_destroy(wx_handle h);

/* Number of state-dict tensors the configuration expects, and the i-th key/shape
 * (so a host can enumerate what to feed to wx_load_tensor). */
int wx_num_tensors(wx_handle h);
int wx_tensor_info(wx_handle h, int index, const char** key, int* ndim, int64_t shape[8]);

/* ---- step glue configuration ---------------------------------------------
 * wx_set_denorm       <-> _build_output_denorm (rollout_to_netcdf.py:103-157): per-output-channel mean/std (host ptrs)
 * wx_set_tracer_fixer <-> PostBlock/TracerFixer (credit/postblock/gen1.py:111-167): clamp y[:, i] < thres -> thres
 *                         (thres_max may be NULL); denorm != 0 clamps in physical units using the wx_set_denorm stats
 * wx_set_layout       <-> build_channel_layout (credit/datasets/gen_2/channel_utils.py:161-250), single source:
 *                         x = [n_prog prognostic | n_static | n_dyn dynamic forcing]
 * wx_set_layout_groups <-> the same function for ANY number of data sources (its ChannelGroup list, :140-250): group i covers
 *                         input channels [x_start, x_start+count); kind 0 = prognostic, replaced at the next step by output
 *                         channels [src_start, ...) of y (update_x, :253-291); kind 1 = dynamic_forcing, replaced by channels
 *                         [src_start, ...) of the forcing tensor; kind 2 = fixed (static), carried forward.  The groups must
 *                         cover every input channel exactly once.  Call after wx_finalize_weights.
 */
int wx_set_denorm(wx_handle h, const float* mean, const float* std, int n_out);
int wx_set_tracer_fixer(wx_handle h, const int32_t* inds, const float* thres, const float* thres_max, int n,
                        int denorm);
int wx_set_layout(wx_handle h, int n_prog, int n_static, int n_dyn);
int wx_set_layout_groups(wx_handle h, int n_groups, const int32_t* kind, const int32_t* x_start, const int32_t* src_start,
                         const int32_t* count);

/* ---- the hot path ---------------------------------------------------------
 * wx_forward <-> y = model(x) under eval()/no_grad() (rollout_to_netcdf.py:275):
 *     x_dev  float32 [B, C_in, frames, H, W]  (not modified)
 *     y_dev  float32 [B, C_out, output_frames, H, W]   (tracer fixer applied when configured)
 * wx_step    <-> one iteration of predict()'s loop (rollout_to_netcdf.py:274-310), B = 1:
 *     y = model(x) [+ tracer fixer]; y_phys = y*std + mean; x_next = update_x(x, frc, y).
 *     y_dev / y_phys_dev / x_next_dev may each be NULL to skip that output; frc_dev
 *     float32 [1, n_dyn, 1, H, W] may be NULL when x_next_dev is NULL.
 *     x_next_dev may not alias x_dev.
 */
int wx_forward(wx_handle h, const float* x_dev, float* y_dev, int batch, void* stream);
int wx_step(wx_handle h, const float* x_dev, const float* frc_dev, float* y_dev, float* y_phys_dev,
            float* x_next_dev, void* stream);
/* wx_rollout <-> the whole predict() loop (rollout_to_netcdf.py:262-316), B = 1: n_steps iterations of wx_step with the state
 *     kept in engine-owned buffers, no host code between steps.
 *     x0_dev         float32 [1, C_in, 1, H, W], not modified
 *     frc_dev        HOST array of n_steps device pointers, frc_dev[t] = dynamic forcing [1, n_dyn, 1, H, W] entering the input of
 *                    step t+1 (what update_x receives after step t); NULL entries / NULL array allowed where no next input is built
 *     y_phys_dev     HOST array of n_steps device pointers (or NULL): de-normalised output of step t goes to y_phys_dev[t];
 *                    NULL entries skip that step's output.  Pointers may repeat (a ring the host drains asynchronously).
 *     x_final_dev    optional: receives the model input that would feed step n_steps (needs frc_dev[n_steps-1])
 *     The results are bit-identical to n_steps calls of wx_step.  With WX_GRAPH=1 in the environment every step is replayed from a
 *     captured hipGraph (one per ping-pong parity and y_phys destination); measured slower than eager launches on MI355X (the cost
 *     between dependent kernels is the device-side dispatch boundary, not host launch time), so it is off by default. */
int wx_rollout(wx_handle h, const float* x0_dev, const float* const* frc_dev, int n_steps, float* const* y_phys_dev,
               float* x_final_dev, void* stream);

/* ---- the ensemble's noise (CrossFormerWithNoise; the generator's exact recipe: csrc/wx_noise.h) ------------------------------
 * Six StochasticDecompositionLayers (stochastic_decomposition_layer.py): y = x + ((noise_factor * r) * style) * modulation,
 * style = noise_transform(z), r ~ N(0,1) per element, z ~ N(0,1) per member; after encoder stages 0..2 (in place on the stage
 * output, which is both the skip and the next stage's input) and after up_block1..3 (before the concat).  The engine draws r and z
 * from a counter-based Philox4x32-10 generator keyed by (seed; element, layer, member, step), so every member and step has its own
 * reproducible noise whatever the batch split, precision or launch geometry.
 * wx_set_noise       seed, member of batch row 0 (row b of wx_forward is member member0 + b; wx_step / wx_rollout run member0) and
 *                    the step coordinate of the next forward.  The step lives in device memory and advances by one after every
 *                    wx_forward, wx_step and rollout step (also inside the WX_GRAPH=1 replays).  Defaults: 0, 0, 0.
 * wx_set_noise_tape  replays given draws instead of the generator, in the reference's draw order: per active layer (encoder 0..2, then
 *                    decoder 1..3) the latent z [B][noise_latent_dim] then the pixel noise [B][C][H][W] (with noise_correlated: one
 *                    latent first, then the pixel draws); `draws` is a HOST array of n DEVICE pointers (float32), each covering the
 *                    batch of the next wx_forward.  draws = NULL returns to the generator.  The pointers must stay valid while set.
 * Both reject a model without noise layers.  Debug captures "encoder_noise_layers.K" / "noise_injectN" hold the noisy maps
 * ("layers.K.1" / "up_blockN" stay the pre-noise ones). */
int wx_set_noise(wx_handle h, uint64_t seed, int member0, int step);
int wx_set_noise_tape(wx_handle h, const float* const* draws, int n);

/* ---- window attention as an operator of its own (second architecture) --------------------------------
 * The attention CORE of a windowed transformer block on a token-major map: out = softmax(scores + bias [+ mask]) v per window
 * and head, everything between the qkv projection and the output projection.  Three window kinds:
 *   0  contiguous wsz_y x wsz_x blocks            (CrossFormer short attention, crossformer.py:247-316)
 *   1  dilated wsz x wsz grids                    (CrossFormer long attention)
 *   3  blocks of the map rolled by (-shift_y, -shift_x), pairs across the latitude seam get `mask_value` added
 *      (credit/models/swin.py:451-486 `_shifted_window_attn`, :411-427 `_make_attention_mask`; the FuXi stage
 *      credit/models/fuxi.py:250-260 runs the same operator through timm)
 * scores = q . k * softmax_scale, or -- when logit_scale is given -- normalize(q) . normalize(k) * logit_scale[head]
 * (swin.py:305-309 scaled cosine attention; pass exp(clamp(logit_scale, max = log 100)) as the reference computes it).
 * bias_host: [n_bias_heads][N][N] float32 (N = wsz_y * wsz_x; n_bias_heads = heads, 1 = shared, 0 = none), e.g. the output of
 * swin.py:283-297 `_relative_positional_encodings`.
 *     qkv_dev  [H * W][3 C]  q | k | v, each head-major (what `Linear(dim, 3 dim)` produces), bf16 or float32 per `precision`
 *     out_dev  [H * W][C]    same element type */
typedef struct wx_winattn_desc {
  int32_t precision;           /* WX_PREC_FP32 / WX_PREC_BF16: element type of qkv / out and of the MFMA path */
  int32_t H, W, C, heads, head_dim;
  int32_t wsz_y, wsz_x;        /* wsz_x = 0: square */
  int32_t kind, shift_y, shift_x;
  float softmax_scale;         /* ignored when logit_scale is given */
  float mask_value;            /* kind 3 (the reference: -100) */
  int32_t mask_axes;           /* kind 3: 1 (or 0) = latitude seam only (V2-Cr, swin.py:411-427); 3 = longitude seam too -- the mask of timm's
                                  SwinTransformerV2Block (the class credit/models/fuxi.py:250-260 instantiates): nine img_mask slices over
                                  both axes, i.e. at most 2 x 2 regions inside a window */
} wx_winattn_desc;
typedef struct wx_winattn* wx_winattn_handle;
int wx_winattn_create(const wx_winattn_desc* desc, const float* bias_host, int n_bias_heads, const float* logit_scale_host, int device,
                      wx_winattn_handle* out);
int wx_winattn_apply(wx_winattn_handle w, const void* qkv_dev, void* out_dev, void* stream);
int wx_winattn_destroy(wx_winattn_handle w);

/* ---- a stage of Swin V2 (Cr) transformer blocks (BASELINE config 5) -----------------------------------
 * credit/models/swin.py:484-502 `SwinTransformerV2CrBlock.forward` (res-post-norm: x += norm1(proj(attention(qkv(x)))), then
 * x += norm2(fc2(GELU(fc1(x))))) repeated `depth` times as credit/models/swin.py:560-668 `SwinTransformerV2CrStage` builds it
 * (downscale = False): even blocks unshifted, odd blocks shifted by (shift_y, shift_x) = window // 2.  FuXi's U-Transformer
 * (credit/models/fuxi.py:250-260) runs such a stage -- through timm's class, which is not vendored: parity of THAT class is
 * unpinned, the V2-Cr block above is pinned to the reference's own forward (tests/test_swin.py).
 *   x_in / x_out  [H * W][C] token-major (the reference's BHWC with B = 1), bf16 or float32 per `precision`; may alias
 *   wx_swin_load(block, name, ...): name in {"attn.qkv.weight" [3C][C], "attn.qkv.bias", "attn.proj.weight" [C][C], "attn.proj.bias",
 *     "attn.bias_table" [heads][N][N] (the OUTPUT of swin.py:283-297 for this block's meta MLP), "attn.logit_scale" [heads]
 *     (exp(clamp(.., max = log 100)), swin.py:307), "norm1.weight", "norm1.bias", "mlp.fc1.weight" [hidden][C], "mlp.fc1.bias",
 *     "mlp.fc2.weight" [C][hidden], "mlp.fc2.bias", "norm2.weight", "norm2.bias"}: float32 host data, `count` elements */
typedef struct wx_swin_desc {
  int32_t precision;           /* WX_PREC_FP32 / WX_PREC_BF16 */
  int32_t H, W, C, heads;
  int32_t wsz_y, wsz_x;
  int32_t depth, hidden;       /* hidden = int(C * mlp_ratio) */
  int32_t shift_y, shift_x;    /* of the odd blocks */
  float mask_value;            /* -100 (swin.py:425) */
  float ln_eps;                /* 1e-5 (nn.LayerNorm default) */
  int32_t mask_axes;           /* 1 (or 0): V2-Cr mask, latitude only; 3: timm V2 mask, both axes (see wx_winattn_desc) */
} wx_swin_desc;
typedef struct wx_swin* wx_swin_handle;
int wx_swin_create(const wx_swin_desc* desc, int device, wx_swin_handle* out);
int wx_swin_load(wx_swin_handle s, int block, const char* name, const float* host_data, int64_t count);
int wx_swin_finalize(wx_swin_handle s);
int wx_swin_apply(wx_swin_handle s, const void* x_in_dev, void* x_out_dev, void* stream);
int wx_swin_flops(wx_swin_handle s, double* flops);   /* algorithmic FLOPs of one wx_swin_apply (2*MAC of the Linear layers + attention) */
int wx_swin_destroy(wx_swin_handle s);

/* ---- the FuXi forward (BASELINE config 5) --------------------------------------------------------------------------
 * credit/models/fuxi.py:454-500 (Fuxi.forward) for one sample, padding_conf / post_conf off, image a multiple of the patch
 * (then the trailing F.interpolate(size = image) is the identity), frame_patch_size == frames (the time axis collapses, :470):
 *   x [C_in][frames][H][W] float32 -> CubeEmbedding (:82-143) -> UTransformer (:204-310: DownBlock, zero-pad to the window,
 *   Swin stage, crop, concat, UpBlock) -> fc + patch reshape (:484-488) -> y [C_out][H][W] float32.
 * The stage in the middle is wx_swin above in one of two variants (wx_fuxi_desc.stage_variant): timm's Swin V2 block, which is
 * what the reference instantiates (timm is not vendored: that variant follows timm's published block, parity unpinned), or the V2-Cr
 * block of credit/models/swin.py (pinned to reference goldens).  Everything around the stage follows the reference's own modules.
 *   wx_fuxi_load(name, ...): name = the reference's state-dict key with EFFECTIVE weights (eval-mode spectral norm folded by the
 *     caller, fuxi.py:16-22): "cube_embedding.proj.weight" [dim][C_in][frames][ph][pw], "cube_embedding.proj.bias",
 *     "cube_embedding.norm.{weight,bias}", "u_transformer.down.conv.{weight [dim][dim][3][3],bias}",
 *     "u_transformer.down.b.{0,3}.{weight,bias}" (Conv2d), "u_transformer.down.b.{1,4}.{weight,bias}" (GroupNorm), the same under
 *     "u_transformer.up." with "u_transformer.up.conv.weight" [2 dim][dim][2][2] (ConvTranspose2d), "fc.weight" [C_out ph pw][dim],
 *     "fc.bias", and "u_transformer.layer.blocks.<i>.<wx_swin_load name>" for the stage.
 *   wx_fuxi_debug_map(name in {"embed", "down", "stage", "up"}): an intermediate token map [rows][cols][dim] of the LAST forward,
 *     converted to float32 (tests); host == NULL only reports the shape.  "patches" / "fc" are the two sides of the patch reshapes:
 *     the gathered patch rows [Hp][Wp][k0_padded] the embed GEMM reads (column order = the Conv3d weight's flatten order
 *     ((c frames + t) ph + py) pw + px; pad columns zero) and fc's output [Hp][Wp][nfc_padded] (column (py pw + px) C_out + c).
 *     shape[2] is the map's own width.
 *   wx_fuxi_query(key): one integer fact about the model / its LAST forward, by name (tests assert which kernel a case ran):
 *     "patchify_rows"      1 = the last forward gathered patches with the row kernel (patch width 4, x on a 16-byte boundary), 0 = the
 *                          generic gather; before the first forward, what a 16-byte aligned x takes
 *     "unpatchify_lds"     1 = the patch -> pixel scatter runs through LDS (patch width divides 256, 256 C_out elements fit 64 KiB)
 *     "unpatchify_chunks"  x-chunks of 256 / pw patches per patch sub-row in that kernel (0 with the generic scatter)
 *     "k0", "k0_padded"    C_in frames ph pw, and the row width of the embed GEMM's input (64-byte multiples)
 *     "nfc", "nfc_padded"  C_out ph pw, and fc's output width (multiples of 8)
 *     "fc_dma"             1 = fc runs the LDS-DMA GEMM, 0 = the slow GEMM (nfc_padded < 48)
 *     An unknown key is WX_ERR_INVALID. */
typedef struct wx_fuxi_desc {
  int32_t precision;            /* WX_PREC_FP32 / WX_PREC_BF16 */
  int32_t H, W;                 /* image_height, image_width */
  int32_t C_in, C_out;          /* channels*levels + surface (+ input-only | + output-only) */
  int32_t frames;               /* = frame_patch_size */
  int32_t patch_h, patch_w;
  int32_t dim, heads, window, depth;
  int32_t groups_down, groups_up;   /* to_2tuple(num_groups) */
  int32_t stage_variant;        /* WX_STAGE_TIMM_V2 (what fuxi.py:250-260 builds: timm.models.swin_transformer_v2.SwinTransformerV2Stage --
                                   shift mask over both axes; its q/v bias, 16 sigmoid(cpb_mlp) table and clamped logit scale reach the engine
                                   as "attn.qkv.bias" / "attn.bias_table" / "attn.logit_scale", computed by the host) or WX_STAGE_V2_CR
                                   (credit/models/swin.py's block: latitude-only mask; the variant pinned to reference goldens) */
} wx_fuxi_desc;
#define WX_STAGE_V2_CR 0
#define WX_STAGE_TIMM_V2 1
typedef struct wx_fuxi* wx_fuxi_handle;
int wx_fuxi_create(const wx_fuxi_desc* desc, int device, wx_fuxi_handle* out);
int wx_fuxi_load(wx_fuxi_handle f, const char* name, const float* host_data, int64_t count);
int wx_fuxi_finalize(wx_fuxi_handle f);
int wx_fuxi_forward(wx_fuxi_handle f, const float* x_dev, float* y_dev, void* stream);
int wx_fuxi_debug_map(wx_fuxi_handle f, const char* name, float* host, int64_t capacity, int64_t shape[3]);
int wx_fuxi_query(wx_fuxi_handle f, const char* key, int64_t* value);
int wx_fuxi_flops(wx_fuxi_handle f, double* flops);
int wx_fuxi_destroy(wx_fuxi_handle f);

/* ---- conservation fixers (PostBlock) -------------------------------------------
 * A wx_post is the device-side counterpart of credit/postblock/gen1.py::PostBlock for pressure-level grids: an ordered
 * list of TracerFixer (:111-167), GlobalMassFixer (:170-391), GlobalWaterFixer (:394-569) and GlobalEnergyFixer
 * (:572-822) operating in place on y [C_out][H][W] (float32, one batch item, time collapsed) given the step's input
 * x [C_in][frames][H][W] (last frame used).  It is independent of the model geometry, so it serves both uses the
 * reference has: inside the model (wx_attach_postblock: runs after every forward, before y_phys / x_next are formed)
 * and outside it (rollout_to_netcdf.py:277-284: call wx_post_apply yourself).
 *   wx_post_set_grid  <-> physics_pressure_level(lon2d, lat2d, p_level, midpoint)   (credit/physics_core.py:75-134)
 *   wx_post_set_stats <-> load_transforms(..., scaler_only=True) for `denorm: True` fixers (per-channel mean/std)
 *   n_seconds = 3600 * data.lead_time_periods; rad_inds = {TOA solar, TOA OLR, surf solar, surf LR, surf SH, surf LH}
 *   wx_post_set_grid_sigma <-> physics_hybrid_sigma_level(lon2d, lat2d, coef_a, coef_b, midpoint) (:300-368); the fixers
 *   added afterwards follow the reference's sigma branches (the mass fixer rescales channel `sp_ind`, gen1.py:355-375). */
typedef struct wx_post* wx_post_handle;

/* ---- input side on the device -------------------------------------------------------------
 * credit/preblock/norm.py:78-98 (ERA5Normalizer: (t - mean) / clamp(std, 1e-12) per variable and level) and
 * credit/preblock/concat.py:96-207 (ConcatToTensor: torch.cat of the named fields along the channel dim) in one pass.
 * Field f is a device tensor [batch, n_levels[f], frames, H, W] (fp32); they are written, normalised, into
 * x [batch, sum(n_levels), frames, H, W] in the order given.  mean/std: host arrays with one entry per OUTPUT channel, or
 * both NULL (concatenate only).  The order itself (field-type rank, 3d before 2d, stable) is host logic, see
 * wxengine/preblock.py which mirrors `_channel_sort_key`. */
typedef struct wx_pre* wx_pre_handle;
int wx_pre_create(int n_fields, const int32_t* n_levels, int frames, int H, int W, const float* mean, const float* std,
                  int device, wx_pre_handle* out);
int wx_pre_destroy(wx_pre_handle p);
int wx_pre_channels(wx_pre_handle p, int* channels);
int wx_pre_apply(wx_pre_handle p, const float* const* fields_dev, float* x_dev, int batch, void* stream);

/* ---- gen-2 variable transforms on the device (csrc/wx_pre.h pre_xform_kernel, csrc/wx_unxform.h) -------------------------------
 * The per-step chains of the reference's gen-2 configs (config/gen_2/examples), fused around the two existing passes:
 *   pre : fill_values* -> (log_transform | sqrt_transform)? -> bridgescaler_transform(transform) -> concat
 *   post: reconstruct -> bridgescaler_transform(inverse_transform) -> (exp_transform | square_transform)?
 *   wx_pre_set_transforms <-> FillValues.forward (credit/preblock/fill_values.py:120-171), LogTransform.forward
 *                         (credit/preblock/log.py:84-105) and SqrtTransform.forward (credit/preblock/sqrt.py:52-71), applied by
 *                         wx_pre_apply from then on, per OUTPUT channel c of the block (host arrays of wx_pre_channels entries):
 *       n_rules[c]        0 .. 8 fill rules, rule k of channel c at [c * 8 + k] of rule_op (enum wx_fill_op) / rule_search /
 *                         rule_fill.  Every mask is taken on the ORIGINAL value, a numeric rule never matches NaN, replacements
 *                         happen in rule order (the last matching rule wins); rule_search is ignored for WX_FILL_NAN.  Rules of
 *                         stacked FillValues blocks on one variable are NOT simply concatenated (a later block sees the earlier
 *                         block's output): the host composes them, see wxengine/transforms.py.
 *       kind[c]           enum wx_xform: then log_base(x + eps[c]) - log_eps[c] (base e / 2 / 10, the float32 sum's logarithm
 *                         correctly rounded) or sqrtf(x); eps and log_eps are the reference's Python floats rounded to float32, as adding
 *                         them to a float32 tensor rounds them.  x < -eps and the root of a negative give NaN as in the reference.
 *       then the block's (v - mean) / max(std, 1e-12) and the store.  A block without a table runs the plain kernel, bit for bit.
 *     WX_ERR_INVALID with the reason in wx_last_error(): a null pointer, an unknown kind or op, more than 8 rules, eps <= 0 (or a
 *     non-finite eps / log_eps) on a log channel.
 *   wx_unxform_create / wx_unxform_destroy <-> ExpTransform.__init__ (credit/postblock/exp.py:38-62), SquareTransform.__init__
 *                         (credit/postblock/square.py:36-40) and the scaler's statistics, for a list of n_vars <= 64 variables with
 *                         n_levels[v] levels on an H x W grid: kind[v] (enum wx_xform, inverse direction), eps[v] / log_eps[v]
 *                         (float32 roundings as above), has_stats[v] and mean / std with one entry per (variable, level) in
 *                         variable order (entries of variables without statistics are ignored; both NULL when none has any).
 *   wx_unxform_apply      <-> the scaler's inverse_transform, ExpTransform.forward (exp.py:73-88) and SquareTransform.forward
 *                         (square.py:42-57) of all the variables in ONE launch: p = y * std + mean (a rounded product, then a rounded
 *                         sum; skipped where has_stats[v] == 0), then e^(p + log_eps) - eps | 2^(.) - eps | pow(10, .) - eps | p * p.
 *       src_dev[v]        batch item b at src_dev[v] + b * batch_stride[v] floats: [n_levels[v]][n_time][H][W] contiguous -- the
 *                         channel-slice views Reconstruct makes of y_pred are read where they lie; never modified
 *       dst_dev[v]        [batch][n_levels[v]][n_time][H][W] contiguous, written
 *     16-byte accesses where H * W % 4 == 0 and both pointers of a plane sit on 16 bytes, 4-byte accesses otherwise. */
enum wx_xform {
  WX_XFORM_NONE = 0,
  WX_XFORM_LOG_E = 1,      /* pre: ln(x + eps) - ln(eps)         post: e^(p + ln eps) - eps */
  WX_XFORM_LOG_2 = 2,      /* pre: log2(x + eps) - log2(eps)     post: 2^(p + log2 eps) - eps */
  WX_XFORM_LOG_10 = 3,     /* pre: log10(x + eps) - log10(eps)   post: pow(10, p + log10 eps) - eps */
  WX_XFORM_SQRT = 4        /* pre: sqrt(x)                       post: p * p */
};
enum wx_fill_op { WX_FILL_NAN = 0, WX_FILL_EQ = 1, WX_FILL_NE = 2, WX_FILL_LT = 3, WX_FILL_LE = 4, WX_FILL_GT = 5, WX_FILL_GE = 6 };
#define WX_MAX_FILL_RULES 8
int wx_pre_set_transforms(wx_pre_handle p, const int32_t* kind, const float* eps, const float* log_eps, const int32_t* n_rules,
                          const int32_t* rule_op, const float* rule_search, const float* rule_fill);
typedef struct wx_unxform* wx_unxform_handle;
int wx_unxform_create(int n_vars, const int32_t* n_levels, int H, int W, const int32_t* kind, const float* eps, const float* log_eps,
                      const int32_t* has_stats, const float* mean, const float* std, int device, wx_unxform_handle* out);
int wx_unxform_destroy(wx_unxform_handle u);
int wx_unxform_apply(wx_unxform_handle u, const float* const* src_dev, const int64_t* batch_stride, float* const* dst_dev, int batch,
                     int n_time, void* stream);
int wx_post_create(int H, int W, int c_in, int frames, int c_out, int device, wx_post_handle* out);
int wx_post_destroy(wx_post_handle p);
int wx_post_set_grid(wx_post_handle p, const float* lat2d, const float* lon2d, const float* p_levels, int n_levels,
                     int midpoint);
int wx_post_set_grid_sigma(wx_post_handle p, const float* lat2d, const float* lon2d, const float* coef_a,
                           const float* coef_b, int n_levels, int midpoint, int sp_ind);
int wx_post_set_stats(wx_post_handle p, const float* mean_in, const float* std_in, const float* mean_out,
                      const float* std_out);
int wx_post_add_tracer_fixer(wx_post_handle p, const int32_t* inds, const float* thres, const float* thres_max, int n,
                             int denorm);
int wx_post_add_mass_fixer(wx_post_handle p, int q_start, int fix_level_num, int denorm);
int wx_post_add_water_fixer(wx_post_handle p, int q_start, int precip_ind, int evapor_ind, float n_seconds, int denorm);
int wx_post_add_energy_fixer(wx_post_handle p, int T_start, int q_start, int U_start, int V_start,
                             const int32_t rad_inds[6], const float* gph_surf, float n_seconds, int denorm);
/* GlobalEnergyFixerUpDown (credit/postblock/gen1.py:825-1030): flux_inds = [TOA down solar, TOA up solar, TOA up OLR,
 * surface down solar, surface up solar, surface down LW, surface up LW, SH, LH]. */
int wx_post_add_energy_fixer_updown(wx_post_handle p, int T_start, int q_start, int U_start, int V_start,
                                    const int32_t flux_inds[9], const float* gph_surf, float n_seconds, int denorm);
/* The general energy fixer: R_T = sum toa_sign[k] * y[toa_ind[k]] (<= 4 terms), F_S = sum srf_sign[k] * y[srf_ind[k]] (<= 8).
 * The gen-2 name-keyed fixer (credit/postblock/conservation.py:239-376) maps onto this one (wxengine/conservation.py). */
int wx_post_add_energy_fixer_signed(wx_post_handle p, int T_start, int q_start, int U_start, int V_start, int n_toa,
                                    const int32_t* toa_inds, const float* toa_signs, int n_srf, const int32_t* srf_inds,
                                    const float* srf_signs, const float* gph_surf, float n_seconds, int denorm);
int wx_post_apply(wx_post_handle p, const float* x_dev, float* y_dev, void* stream);
/* Lat-band mode: the block covers rows [row0, row0 + rows) of the grid it was created for (x / y are bands then); call it
 * right after wx_post_create.  lat2d / lon2d / gph_surf passed afterwards are still whole-grid arrays (cell areas need the
 * neighbouring latitudes).  Such a block only runs attached to a lat-band engine (wx_attach_postblock BEFORE
 * wx_band_enable), which completes the global integrals of gen1.py:280-1030 with one exchange per fixer. */
int wx_post_set_band(wx_post_handle p, int row0, int rows);
/* Run `p` inside wx_forward / wx_step (after the tail, before y_phys and x_next); NULL detaches.  The engine does not
 * take ownership. */
int wx_attach_postblock(wx_handle h, wx_post_handle p);

/* ---- pressure-level products on the device (csrc/wx_diag.h) ----------------------------------------------------------
 * The three diagnostics of the gen-2 post-block chain in ONE launch, one thread per column, on the named tensors as they lie in
 * memory ([B][n_levels][n_time][H][W] float32 contiguous; 2-D variables [B][1][n_time][H][W]):
 *   wx_diag_create / wx_diag_destroy  <-> GeopotentialDiagnostic.__init__ (credit/postblock/geopotential.py:132-172),
 *                         PressureInterpDiagnostic.__init__ (credit/postblock/pressure_interp.py:189-241), MSLPDiagnostic.__init__
 *                         (credit/postblock/mslp.py:117-132); 2 <= n_levels <= 137
 *   wx_diag_set_levels    <-> the hybrid coefficients those constructors read from `level_info_file`: a_half / b_half [n_levels + 1]
 *                         (geopotential.py:162-171, p = a + b sp on the interfaces, non-positive -> 0.57 Pa, :32-33) with its
 *                         `flip_vertical` (:70-82), and a_mid / b_mid [n_levels] (pressure_interp.py:225-234); host pointers,
 *                         either pair may be NULL when no requested product needs it.  Levels stored surface -> top are detected
 *                         from a_mid + b_mid * 101325 Pa as :237-241 does and handled by index arithmetic.
 *   wx_diag_set_pressure_levels <-> `pressure_levels` (in Pa here, any order, 1 <= n_plev <= 64) and `temp_height` (:191, :202)
 *   wx_diag_apply         <-> the three forward()s: geopotential (geopotential.py:37-83), interp_column_to_pressure_levels
 *                         (pressure_interp.py:44-130 over _interp_utils.py:14-40: linear in log p, constant extrapolation of
 *                         `fields`, Trenberth Eq. 16 / 15 below ground for T and Z) and mslp_from_surface_pressure (mslp.py:33-80).
 *       T, q, fields[f]   [B][n_levels][n_time][H][W]      sp, t_near_surface  [B][1][n_time][H][W]
 *       phis              [B][1][phis_n_time][H][W], phis_n_time = 1 or n_time
 *       z_model_out       [B][n_levels][n_time][H][W]: the model-level geopotential, or NULL
 *       plev_out          HOST array of n_fields + 2 device pointers [B][n_plev][n_time][H][W]: the fields, then T, then Z; or NULL
 *       mslp_out          [B][1][n_time][H][W], or NULL
 *     A NULL output switches that product off; a product whose inputs or coefficients are missing is WX_ERR_INVALID with the
 *     reason in wx_last_error().  The geopotential that feeds the interpolation stays on the chip.  Chain form (the reference's
 *     separate blocks, where the interpolation takes `geopotential_var` from the batch): with q == NULL and plev_out given,
 *     z_model_out is READ as the model-level geopotential instead of written; the results equal the fused launch bit for bit. */
typedef struct wx_diag* wx_diag_handle;
int wx_diag_create(int H, int W, int n_levels, int device, wx_diag_handle* out);
int wx_diag_destroy(wx_diag_handle d);
int wx_diag_set_levels(wx_diag_handle d, const float* a_half, const float* b_half, const float* a_mid, const float* b_mid,
                       int flip_vertical);
int wx_diag_set_pressure_levels(wx_diag_handle d, const float* p_pa, int n_plev, float temp_height);
int wx_diag_apply(wx_diag_handle d, int batch, int n_time, const float* T, const float* q, const float* sp, const float* phis,
                  int phis_n_time, const float* t_near_surface, const float* const* fields, int n_fields, float* z_model_out,
                  float* const* plev_out, float* mslp_out, void* stream);

/* ---- wind artifact filter on the device (csrc/wx_wind.h) ------------------------------------------------------------------------
 * credit/postblock/wind_filter.py in at most four launches, whatever the number of variables and levels; float32 throughout.
 *   wx_wind_create / wx_wind_destroy <-> WindArtifactFilter.__init__ (wind_filter.py:175-204) and the kernels _compute_blend_mask
 *                         builds at every call (:51-82).  The normalised 1-D Gaussians are computed by the caller with the reference's
 *                         float32 expressions and passed as HOST arrays: smooth_lat / smooth_lon (size int(6 sigma + 1) | 1 per axis),
 *                         falloff_lat (sigma falloff_sigma, size int(4 sigma + 1) | 1) / falloff_lon (sigma 2 falloff_sigma, size
 *                         int(8 sigma + 1) | 1); the 2-D outer products are never formed.  dilation_lat x dilation_lon: the rectangle of
 *                         ones (dilation_meridional x dilation_zonal).  WX_ERR_INVALID with the reason: an even or non-positive size
 *                         (the reference itself fails on an even dilation: its dilated mask comes out one row or column larger than the
 *                         field), a size above 33 along latitude or 65 along longitude, a non-finite weight or threshold, H or W < 1.
 *   wx_wind_apply         <-> WindArtifactFilter.forward (:206-252):
 *       u_dev, v_dev      the mask-level PLANE of U and V: batch item b at u_dev + b * u_batch_stride floats, [H][W] contiguous
 *       src_dev[v]        batch item b at src_dev[v] + b * batch_stride[v] floats: [n_levels[v]][H][W] contiguous (n_time == 1), read
 *                         where it lies -- channel slices of y_pred included -- and never modified; n_vars <= 32, n_levels[v] <= 256
 *       dst_dev[v]        [batch][n_levels[v]][H][W] contiguous, written completely: level l of target_levels (those beyond
 *                         n_levels[v] are skipped, :229-236) becomes m fs + (1 - m) f with fs = the zero-padded Gaussian smoothing of f,
 *                         times min(sqrt(sum m f^2 / (sum m fs^2 + 1e-12)), 4) per batch item and plane when preserve_amplitude; every
 *                         other level is copied.  Must not overlap any input.
 *       mask_out_dev      [batch][H][W]: the blend mask m, or NULL (it then stays in the handle's own buffer)
 *     The mask is complete before any output is written (U and V may be targets); the amplitude sums are double partials added in a
 *     fixed order, so repeated calls give identical bits; a point with m == 0 keeps the bits of its input.  16-byte accesses where
 *     W % 4 == 0 and the plane pointer sits on 16 bytes, 4-byte accesses otherwise (the same results).  batch * sum(n_levels) *
 *     ceil(H / 16) * ceil(W / 64) must stay below 2^31. */
typedef struct wx_wind* wx_wind_handle;
int wx_wind_create(int H, int W, const float* smooth_lat, int n_smooth_lat, const float* smooth_lon, int n_smooth_lon,
                   const float* falloff_lat, int n_falloff_lat, const float* falloff_lon, int n_falloff_lon, int dilation_lat,
                   int dilation_lon, float speed_threshold, int preserve_amplitude, int device, wx_wind_handle* out);
int wx_wind_destroy(wx_wind_handle f);
int wx_wind_apply(wx_wind_handle f, const float* u_dev, int64_t u_batch_stride, const float* v_dev, int64_t v_batch_stride, int n_vars,
                  const float* const* src_dev, const int64_t* batch_stride, const int32_t* n_levels, float* const* dst_dev,
                  const int32_t* target_levels, int n_target_levels, int batch, float* mask_out_dev, void* stream);

/* ---- semi-Lagrangian tracer advection on the device (csrc/wx_advect.h) -------------------------------------------------------------
 * credit/postblock/advect.py in two launches and one scratch volume, whatever the number of tracers; float32 throughout.
 *   wx_advect_create / wx_advect_destroy <-> _SemiLagrangianAdvectionEngine.__init__ (advect.py:216-275) and the metric terms
 *                         _grid_coords / advect_nested rebuild at every call (:295-320, :351-376).  a_half / b_half: [n_levels + 1]
 *                         HOST arrays top -> surface, already sliced by `levels` (:262-264).  row_tables: [6][H] HOST floats the
 *                         caller computes from the latitudes with the reference's float32 expressions, so that the reference's
 *                         results are met to rounding: cos(lat); R * max(cos(lat), coslat_floor); torch.gradient(lat_rad) (signed
 *                         radians per row); and the three coefficients a, b, c of torch.gradient's coordinate-aware difference
 *                         a f[h - 1] + b f[h] + c f[h + 1] (:116) -- on the first and the last row b holds the one-sided spacing
 *                         lat[1] - lat[0] / lat[H - 1] - lat[H - 2] and the difference is (f[h + 1] - f[h]) / b, (f[h] - f[h - 1]) / b.
 *                         The results meet the reference's to rounding ONLY with tables built by these torch expressions
 *                         (wxengine.advect.metric_tables builds them; the C library's cosf is not torch.cos); the cos(lat) floor
 *                         is already inside the second table and is not seen here.
 *                         dlon_rad: deg2rad(lon[1] - lon[0]) (:319).  surface_to_top != 0: the DATA's level axis is flipped
 *                         (level_order = "surface_to_top", :340-345 and :421-422); an index flip, not a copy.  WX_ERR_INVALID with
 *                         the reason: H, W or n_levels < 2 (the reference's torch.gradient raises on a single level), n_iterations
 *                         < 1, a non-finite table entry, time step or floor, a zero spacing, n_levels * H * W >= 2^31.
 *   wx_advect_apply       <-> _SemiLagrangianAdvectionEngine.advect_nested (:325-423), n_time == 1:
 *       u_dev, v_dev      batch item b at u_dev + b * u_batch_stride floats: [n_levels][H][W] contiguous, in the data's level order
 *       sp_dev            surface pressure [Pa], batch item b at sp_dev + b * sp_batch_stride floats: [H][W]
 *       omega_dev         NULL: omega from mass continuity (omega_from_continuity, :121-156, over horizontal_divergence, :85-118);
 *                         otherwise the omega_var tensor [Pa / s], laid out like u_dev (:368-369)
 *       src_dev[t]        tracer t, batch item b at src_dev[t] + b * batch_stride[t] floats: [n_levels][H][W] contiguous, read where
 *                         it lies -- channel slices of y_pred included -- and never modified; n_tracers <= 32.  A tracer may be
 *                         u_dev or v_dev itself: the winds are read from the inputs.
 *       dst_dev[t]        [batch][n_levels][H][W] contiguous, written completely: the trilinear interpolant of the tracer at the
 *                         departure point of the iterative-midpoint back-trajectory (:392-423).  Must not overlap any input.
 *     Sampling in index space (:167-203): the column as a floating remainder modulo W with neighbours i, (i + 1) mod W; row and
 *     level clamped to [0, n - 1], upper neighbour min(i + 1, n - 1).  Zero winds return the input bit for bit; repeated calls give
 *     identical bits.  The handle holds one scratch volume of batch * n_levels * H * W 16-byte velocity records, grown to the
 *     largest batch seen: ONE handle serves ONE stream at a time (two calls on the same handle from different streams would share
 *     the volume).  batch * n_levels * H * W must stay below 2^31; byte offsets are 64-bit. */
typedef struct wx_advect* wx_advect_handle;
int wx_advect_create(int H, int W, int n_levels, const float* a_half, const float* b_half, const float* row_tables, float dlon_rad,
                     float timestep_seconds, int n_iterations, float dp_dlevel_floor, int surface_to_top, int device,
                     wx_advect_handle* out);
int wx_advect_destroy(wx_advect_handle a);
int wx_advect_apply(wx_advect_handle a, const float* u_dev, int64_t u_batch_stride, const float* v_dev, int64_t v_batch_stride,
                    const float* sp_dev, int64_t sp_batch_stride, const float* omega_dev, int64_t omega_batch_stride, int n_tracers,
                    const float* const* src_dev, const int64_t* batch_stride, float* const* dst_dev, int batch, void* stream);

/* ---- hybrid-level interpolation on the device (csrc/wx_hybrid.h) ------------------------------------------------------------------
 * credit/postblock/hybrid_interp.py (and the pre block of credit/preblock/hybrid_interp.py over the same engine): 3-D variables from
 * one set of hybrid sigma-pressure levels onto another, linear in log p with constant extrapolation; float32 throughout.
 *   wx_hybrid_create / wx_hybrid_destroy <-> _HybridLevelInterpEngine.__init__ (hybrid_interp.py:74-106).  a_src / b_src [n_src] and
 *                         a_dst / b_dst [n_dst]: HOST arrays of MIDPOINT coefficients in stored order, as
 *                         load_hybrid_level_coefficients returns them (_interp_utils.py:69-80: vcoord rows, interface averaging,
 *                         the `levels` subset, the float32 cast -- wxengine.hybrid_interp.midpoint_coefficients).  The library
 *                         determines the source orientation from a + b * 101325 Pa itself (:100-106; a source stored surface -> top
 *                         is an index flip of the data's level axis, :133-134, not a copy) and sorts the destination levels by their
 *                         pressure at 101325 Pa; outputs are in the destination's stored order.  WX_ERR_INVALID with the reason:
 *                         n_src outside 2 .. 137 (a single source level has no bracket: the reference's gather fails there), n_dst
 *                         outside 1 .. 137, a null array, a non-finite coefficient, H or W < 1.
 *   wx_hybrid_apply       <-> _HybridLevelInterpEngine.interp_nested (:108-161) over interp_column_hybrid_to_hybrid (:32-63) and
 *                         loglinear_interp_columns (_interp_utils.py:14-40):
 *       src_dev[v]        variable v, batch item b at src_dev[v] + b * batch_stride[v] floats (0 when batch == 1):
 *                         [n_src][n_time][H][W] contiguous, in the data's level order, read where it lies -- channel slices
 *                         included -- and never modified; 1 <= n_vars <= 32, in launches of at most eight (every grouping gives
 *                         the same bits per variable)
 *       dst_dev[v]        [batch][n_dst][n_time][H][W] contiguous, written completely.  Must not overlap any input.
 *       sp_dev            surface pressure [Pa], batch item b at sp_dev + b * sp_batch_stride floats: [n_time][H][W]
 *     p = max(a + b sp, 0.57 Pa) for both level sets from the same sp (:29, :61-62); per destination level the bracket
 *     hi = clamp(#{m : p_dst >= p_src[m]}, 1, n_src - 1), lo = hi - 1 (_interp_utils.py:33-34), the weight
 *     clamp(log(p_dst / p_lo) / log(p_hi / p_lo), 0, 1) (:37, as a quotient of logs of ratios) and y_lo + w (y_hi - y_lo) (:40).
 *     The count holds wherever the column's source pressures are non-decreasing (the reference's precondition); otherwise every
 *     index still lies in [0, n_src - 1].  Repeated calls give identical bits; a level set interpolated onto itself returns the
 *     input's bits at every level but the one of highest pressure.  Nothing is allocated at apply; batch * n_time * H * W must stay
 *     below 2^31. */
typedef struct wx_hybrid* wx_hybrid_handle;
int wx_hybrid_create(int H, int W, int n_src, const float* a_src, const float* b_src, int n_dst, const float* a_dst, const float* b_dst,
                     int device, wx_hybrid_handle* out);
int wx_hybrid_destroy(wx_hybrid_handle h);
int wx_hybrid_apply(wx_hybrid_handle h, int n_vars, const float* const* src_dev, const int64_t* batch_stride, float* const* dst_dev,
                    int batch, int n_time, const float* sp_dev, int64_t sp_batch_stride, void* stream);

/* ---- horizontal regridding on the device (csrc/wx_regrid.h) ----------------------------------------------------------------------
 * credit/preblock/regrid.py::Regridder (registry names `regrid`, `Regridder`): an ESMF sparse weight matrix W [n_b x n_a] applied to
 * every plane of a variable, y[p, r] = sum_j S[r, j] x[p, col[r, j]], float32 throughout.
 *   wx_regrid_create / wx_regrid_destroy <-> Regridder.__init__ and _get_W (regrid.py:54-59, :118-132).  HOST arrays: the coalesced
 *                         matrix as CSR, zero-based -- row_ptr [n_b + 1], col [nnz] and val [nnz] with nnz = row_ptr[n_b]
 *                         (wxengine.regrid.coalesce_weights makes them from the file's 1-based `row`, `col`, `S`, as
 *                         sparse_coo_tensor(...).coalesce() does; a source flip is folded into col by wxengine.regrid.fold_flips).
 *                         The library builds its device format itself: sliced ELL, slice height 64, rows in their order, and
 *                         a list of the rows with more than 64 entries, which one wave each sums.  A row's terms are added in
 *                         their stored order.  WX_ERR_INVALID with the reason, before anything is uploaded: a null array; n_a
 *                         or n_b outside 1 .. 2^31 - 1; row_ptr not starting at 0, decreasing somewhere, or ending at 2^31 or
 *                         more; a col outside [0, n_a) (it would be an out-of-bounds read on the device).
 *   wx_regrid_apply       <-> Regridder._regrid (:134-175) for n_vars variables (1 .. 32) in one launch (two when the matrix has
 *                         long rows):
 *       src_dev[v]        variable v: plane q of batch item b at src_dev[v] + b * batch_stride[v] + q * n_a floats
 *                         (batch_stride is ignored when batch == 1), [planes_per_item[v]][n_a] contiguous per batch item, read
 *                         where it lies -- channel slices of a wider tensor included -- and never written
 *       dst_dev[v]        [batch * planes_per_item[v]][n_b] contiguous, distinct from every source; every element is written
 *                         (0.0f for a destination point without entries), so the buffer may arrive uninitialised
 *     WX_ERR_INVALID: a null handle or pointer, n_vars outside 1 .. 32, batch < 1, a planes_per_item < 1, a negative batch stride,
 *     2^31 or more planes in one variable.  A plane's bits do not depend on the planes and variables it shares a call with; repeated
 *     calls give identical bits.  A NaN in the source reaches exactly the destination points whose rows reference it.  Nothing is
 *     allocated at apply. */
typedef struct wx_regrid* wx_regrid_handle;
int wx_regrid_create(int64_t n_a, int64_t n_b, const int64_t* row_ptr, const int32_t* col, const float* val, int device,
                     wx_regrid_handle* out);
int wx_regrid_destroy(wx_regrid_handle h);
int wx_regrid_apply(wx_regrid_handle h, int n_vars, const float* const* src_dev, const int64_t* batch_stride, const int32_t* planes_per_item,
                    int batch, float* const* dst_dev, void* stream);

/* ---- TISR forcing on the device (csrc/wx_tisr.h) ------------------------------------------------------------------------------------
 * credit/datasets/gen_2/tisr.py::TISRDataset / _compute_tisr: the top-of-atmosphere incident solar radiation accumulated over the
 * window (t - period, t], J/m2, float32 -- a GraphCast / IFS orbital model, an annual TSI table, cos(zenith) floored at 0 at every grid
 * point and sub-step, a trapezoid over n_steps + 1 sub-steps.  The reference's float32 quantisation of time (days since J2000, fractional
 * year) is reproduced; everything else of a sub-step is evaluated in fp64, a point's sum is kept in fp64 and rounded once.
 *   wx_tisr_create / wx_tisr_destroy <-> TISRDataset.__init__.  HOST arrays: lat_host, lon_host [ny][nx] in degrees (a rectangular grid
 *                         as its meshgrid, a curvilinear one as it is) and the TSI table, tsi_times_host [n_tsi] in fractional years,
 *                         ascending, with tsi_values_host [n_tsi] in W/m2 (`time` and `tsi` of total_solar_irradiance_CMIP6_49r1.nc).
 *                         WX_ERR_INVALID with the reason: a null argument; ny or nx < 1 or ny * nx > 2^31 - 1; fewer than two table
 *                         entries; a table that is not finite or does not ascend; a latitude or longitude that is not finite.
 *   wx_tisr_compute       <-> _compute_tisr for n_times target times (any number; 64 go into one pair of launches):
 *       t_end_ns_host     HOST array [n_times], the ends of the windows as Unix nanoseconds (UTC); they travel in the kernel arguments
 *       period_ns         the length of the window; n_steps: num_integration_steps.  The sub-steps are those of pandas' date_range(end =
 *                         t, periods = n_steps + 1, freq = period / n_steps): the step is period_ns / n_steps truncated to whole ns
 *       dst_dev           the plane of target time i is written at dst_dev + i * plane_stride floats, [ny][nx] contiguous; nothing else
 *                         is written, so a plane may be a channel slot of a wider forcing tensor
 *     WX_ERR_INVALID, decided on the host before any launch: a null handle or argument, n_times < 1, n_steps outside 1 .. 2^22 - 1,
 *     period_ns < 1 or < n_steps, plane_stride < ny * nx, a window that leaves the int64 range, a sub-step whose YEAR lies outside
 *     int(tsi_times[0]) .. int(tsi_times[n_tsi - 1]) (the reference's ValueError).  A plane's bits do not depend on the target times it
 *     shares a call with.  The coefficient table is the handle's own and grows with n_steps (at most 64 MB): calls on one handle must
 *     be ordered by one stream. */
typedef struct wx_tisr* wx_tisr_handle;
int wx_tisr_create(int ny, int nx, const float* lat_host, const float* lon_host, int n_tsi, const float* tsi_times_host,
                   const float* tsi_values_host, int device, wx_tisr_handle* out);
int wx_tisr_destroy(wx_tisr_handle h);
int wx_tisr_compute(wx_tisr_handle h, int n_times, const int64_t* t_end_ns_host, int64_t period_ns, int n_steps, float* dst_dev,
                    int64_t plane_stride, void* stream);

/* ---- perturbed initial conditions on the device (csrc/wx_perturb.h) ------------------------------------------------------------------
 * credit/ensemble/gaussian.py::GaussianNoise, color.py::ColorNoise, temporal.py::TemporalNoise and utils.hemispheric_rescale: the
 * ensemble route of applications/rollout_metrics_noisy_ic.py, which works with every deterministic checkpoint.  One handle per grid; one
 * call per member and step on the n_planes = C * T planes of a [1, C, T, H, W] float32 tensor (a plane is H * W contiguous floats).
 *   wx_perturb_create / wx_perturb_destroy: kind 0 white (delta = amplitude * r), kind 1 colour (r filtered per plane:
 *                         irfft2(rfft2(r) * S, s = (H, W)) by dense fp64 DFTs on the matrix cores).  S_host: HOST array [H][W / 2 + 1],
 *                         ColorNoise's float32 `scaling_weights`; ignored (may be NULL) for kind 0.  WX_ERR_INVALID with the reason: an
 *                         unknown kind; H < 1 or W < 2; H * W beyond the generator's counter (2^34); for kind 1 a null or non-finite S,
 *                         or a side above 4096 points (a pass keeps its twiddle table in LDS).
 *   wx_perturb_batch      the number of planes the colour filter takes through its scratch at a time: min(64, 256 MiB / (32 H (W / 2 + 1))).
 *   wx_perturb_apply      r: tape_dev (DEVICE, float32, [n_planes][H][W] contiguous: the reference's torch.randn draws replayed) or, when
 *                         NULL, the engine's generator (Philox4x32-10 / Box-Muller as for wx_set_noise) with the counter (e >> 2, slot 16,
 *                         member, step), e = (p * H + h) * W + x.  A draw depends on (seed, member, step, e) alone.  Then per element, every
 *                         operation rounded once in float32 in the reference's order:
 *                             eps = amplitude * n;  eps *= chan_scale[p];  d = rho * prev + eps;  d *= lat_weight[h];
 *                             delta_out = d;  x_out = x + d
 *       chan_scale_host   HOST array [n_planes] or NULL (TemporalNoise: perturbation_std[c] / amplitude, repeated over the T planes of c)
 *       prev_dev, rho     the member's previous delta (DEVICE) or NULL: no AR(1) term
 *       lat_weight_host   HOST array [H] or NULL (hemispheric_rescale's weights)
 *       x_dev, delta_out_dev, x_out_dev   DEVICE; either output may be NULL, not both; x_out needs x.  Plane p of each lies at
 *                         pointer + p * its stride (in floats, >= H * W): a channel range of a wider tensor is perturbed where it lies and
 *                         nothing outside the planes is written.  x_out may be x and delta_out may be prev (same pointer, same stride).
 *     WX_ERR_INVALID with the reason, nothing launched, copied or written: a null handle; n_planes < 1 or H * W * n_planes > 2^34; no
 *     output; x_out without x; a stride below H * W or one that takes the planes beyond
 *     2^44 floats; a tape that overlaps an output; an input that overlaps an output otherwise than
 *     as the same view.  A plane's bits do not depend on n_planes, the batch split or the other planes.  The scratch is the handle's own:
 *     calls on one handle must be ordered by one stream. */
typedef struct wx_perturb* wx_perturb_handle;
int wx_perturb_create(int H, int W, int kind, const float* S_host, int device, wx_perturb_handle* out);
int wx_perturb_destroy(wx_perturb_handle h);
int wx_perturb_batch(wx_perturb_handle h, int* planes_out);
int wx_perturb_apply(wx_perturb_handle h, int n_planes, const float* tape_dev, uint64_t seed, int member, int step, float amplitude,
                     const float* chan_scale_host, float rho, const float* prev_dev, int64_t prev_stride, const float* lat_weight_host,
                     const float* x_dev, int64_t x_stride, float* delta_out_dev, int64_t delta_stride, float* x_out_dev, int64_t x_out_stride,
                     void* stream);

/* ---- zonal power spectra on the device (csrc/wx_spectrum.h) ---------------------------------------------------------------------------
 * credit/losses/gen_1/power.py::PSDLoss (get_psd and forward) and spectral.py::SpectralLoss2D: the per-latitude DFT along longitude of
 * P planes of a float32 field a and, optionally, of a second field b of the same shape, by a dense fp64 DFT on the matrix cores with the
 * real input folded (half the products), in place of a copy of the fields to the host and torch.fft in float32 there.  Wh = W / 2 + 1,
 * X_k = sum_x r[x] e^{-2 pi i k x / W}, mult_k = 1 for k = 0 and 2 for every other bin (the Nyquist bin of an even W too: the reference's).
 *   wx_spectrum_create / wx_spectrum_destroy: the grid and the latitude weights.  lat_w_host: HOST array [H] or NULL (w = 1).
 *                         WX_ERR_INVALID with the reason: H or W < 2; W > 4096 (the twiddle table lies in LDS); a weight that is not
 *                         finite or is negative; weights that sum to zero.
 *   wx_spectrum_apply     plane p of a (of b) at a_dev + p * a_stride floats (stride >= H * W), [H][W] contiguous, read where it lies
 *                         and never modified; b_dev may be NULL.  Every output is DEVICE memory, written completely, or NULL (not wanted):
 *       psd_a_dev, psd_b_dev             [n_planes][H][Wh] float32: mult_k |X_k|^2 / W^2 (PSDLoss.get_psd), rounded once from fp64
 *       mean_psd_a_dev, mean_psd_b_dev   [n_planes][Wh] float64: sum_h what_h psd[h][k], what = w / sum(w) (1 / H without weights)
 *       mean_amp_a_dev, mean_amp_b_dev   [n_planes][Wh] float64: (sum_h w_h |X_k|) / H -- SpectralLoss2D divides by H, not by sum(w)
 *       scores_dev                       [n_planes][2] float64, over the bins k_init <= k < Wh:
 *                                          [0] mean_k sum_h what_h (log(psd_a + 1e-8) - log(psd_b + 1e-8))^2     (PSDLoss per plane)
 *                                          [1] mean_k (mean_amp_a[k] - mean_amp_b[k])^2                           (SpectralLoss2D per plane)
 *                                        the reference's two scalar losses are the means of these over the planes
 *     WX_ERR_INVALID with the reason, nothing launched or written: a null handle or a null a; n_planes < 1; a stride below H * W or
 *     one that takes the planes beyond 2^44 floats; k_init < 0 or >= Wh; a scores pointer, or any output of b, without b; no output at
 *     all; an output that overlaps an input or another output.
 *     Two launches per call, every sum in fp64 in one fixed order, no atomics: a plane's outputs are bit-identical whatever n_planes, the
 *     split of the planes into calls and the plane's position, and the outputs of a are the same with and without b.  The scratch is
 *     the handle's own and grows only in a call with more tiles than any before: calls on one handle must be ordered by one stream. */
typedef struct wx_spectrum* wx_spectrum_handle;
int wx_spectrum_create(int H, int W, const float* lat_w_host, int device, wx_spectrum_handle* out);
int wx_spectrum_destroy(wx_spectrum_handle h);
int wx_spectrum_apply(wx_spectrum_handle h, int n_planes, const float* a_dev, int64_t a_stride, const float* b_dev, int64_t b_stride, int k_init,
                      float* psd_a_dev, float* psd_b_dev, double* mean_psd_a_dev, double* mean_psd_b_dev, double* mean_amp_a_dev,
                      double* mean_amp_b_dev, double* scores_dev, void* stream);

/* ---- verification metrics on the device (csrc/wx_metrics.h) ----------------------------------------------------------------------
 * credit/metrics/base.py, common.py, anomaly.py: the eight per-variable scores of the gen-2 metrics framework from ONE reduction
 * over prediction, target and climatology, in place of three to eight elementwise passes and a host sync per metric and variable.
 *   wx_metrics_create / wx_metrics_destroy: the grid and the latitude weights.  lat_w: HOST array [H] (the reference's
 *                         cos(lat) / mean, base.py:212) or NULL for w = 1.  WX_ERR_INVALID with the reason: H or W < 1, a
 *                         non-finite weight.
 *   wx_metrics_apply      <-> BaseVariableMetric._score_variable (base.py:329-356), R2ScoreMetric / LogVarianceRatioMetric
 *                         (common.py:113-119, :184-191), _AnomalyMetricBase.forward (anomaly.py:284-291) and _score_anomaly (:335-361):
 *       pred_dev[v], target_dev[v]   variable v, batch item b at pointer + b * batch stride floats (0 when batch == 1):
 *                         [n_levels[v]][n_time[v]][H][W] contiguous, read where it lies -- channel slices included, a view that
 *                         starts one float into its buffer too -- and never modified; 1 <= n_vars <= 32
 *       clim_dev[v]       the climatology of variable v or NULL: level l, time t at clim_dev[v] + l * clim_level_stride[v] +
 *                         t * clim_time_stride[v] floats ([H][W] contiguous; stride 0 = one level / no time axis), shared by the
 *                         batch.  clim_dev itself may be NULL (no variable has one: the stream is not read, the stride arrays are
 *                         not looked at)
 *       scores_dev        [n_vars][8] float32, written completely, in the order rmse, mse, mae, bias, r2score,
 *                         log_variance_ratio, acc, activity; acc and activity are NaN for a variable without climatology
 *     With d = p - t and every mean taken over ALL batch * n_levels * n_time * H * W elements (not divided by the sum of w):
 *     mse = mean(w d^2), rmse = sqrt(mse), mae = mean(w |d|), bias = mean(w d), r2score = 1 - mse / (mean(w (t - tbar)^2) + 1e-12)
 *     with tbar = mean(w t), log_variance_ratio = log10(mean(w (p - pbar)^2) + eps) - log10(mean(w (t - tbar)^2) + eps),
 *     d_f = (p - c) - mean(w (p - c)), d_t = (t - c) - mean(w (t - c)), activity = sqrt(mean(w d_f^2) + 1e-12),
 *     acc = mean(w d_f d_t) / (activity sqrt(mean(w d_t^2) + 1e-12)).
 *     Two reading passes (the means, then the centred sums), every sum and score in fp64, float32 at the output only.  Four launches
 *     per call; no floating-point atomics: repeated calls and any grouping of variables into calls give identical bits.  One handle
 *     serves one stream at a time (its scratch is the handle's); a call with more tiles than any before grows the scratch, every
 *     other call allocates nothing. */
typedef struct wx_metrics* wx_metrics_handle;
int wx_metrics_create(int H, int W, const float* lat_w, int device, wx_metrics_handle* out);
int wx_metrics_destroy(wx_metrics_handle h);
int wx_metrics_apply(wx_metrics_handle h, int n_vars, const float* const* pred_dev, const int64_t* pred_batch_stride,
                     const float* const* target_dev, const int64_t* target_batch_stride, const float* const* clim_dev,
                     const int64_t* clim_level_stride, const int64_t* clim_time_stride, const int32_t* n_levels, const int32_t* n_time,
                     int batch, double eps, float* scores_dev, void* stream);

/* ---- ensemble verification on the device (csrc/wx_ensemble.h) ----------------------------------------------------------------------
 * credit/losses/gen_1/kcrps.py, almost_fair_crps.py, credit/metrics/gen_1/metrics.py:247 (LatWeightedMetricsEnsemble),
 * credit/applications/rollout_metrics_noisy_model.py:107 (calculate_ensemble_metrics): CRPS (biased, fair, almost fair), spread and
 * ensemble-mean error of n_members members against the truth from ONE reading pass of (n_members + 1) * 4 bytes per grid point, in
 * place of a moved-axis copy and a sort copy of the ensemble, an [.., M, M] pairwise tensor and a host round trip per channel.
 *   wx_ensemble_create / wx_ensemble_destroy: the grid, the latitude weights and the member count.  lat_w: HOST array [H] or NULL for
 *                         w = 1.  WX_ERR_INVALID with the reason: n_members outside 2..64, H or W < 1, a non-finite weight.
 *   wx_ensemble_apply:
 *       member_dev[v * n_members + m]   variable v, member m, batch item b at pointer + b * member_batch_stride[v] floats (0 when
 *                         batch == 1): [n_levels[v]][n_time[v]][H][W] contiguous, read where it lies and never modified -- separate
 *                         per-member buffers, channel slices, or the reference's [B * M, ...] tensor (pointer of row m, batch stride
 *                         M * stride(0)); 1 <= n_vars <= 32; a null member pointer is WX_ERR_INVALID
 *       target_dev[v]     the truth of variable v, batch item b at pointer + b * target_batch_stride[v] floats
 *       maps_dev          NULL, or [n_vars * 6] pointers, each NULL (not wanted) or a [batch][n_levels[v]][n_time[v]][H][W] float32
 *                         map written in the same pass, in the order ens_mean, ens_std (ddof 1), ens_abs_err, crps, fair_crps, afcrps.
 *                         A map that overlaps an input, the plane table or another map is WX_ERR_INVALID
 *       planes_dev        [sum_v batch * n_levels[v] * n_time[v]][6] float64, written completely: per plane (v, b, level, t), variables
 *                         in call order, the sums over H x W of  w skill, w pair, w err^2, w |err|, w ss, w sqrt(ss / (M - 1))
 *     Per grid point, with d_i = x_i - y (M = n_members): skill = sum |d_i|, pair = sum_{i<j} |d_i - d_j|, err = sum d_i / M,
 *     ss = sum (d_i - err)^2; w = lat_w[h] or 1, sums not divided by the sum of w.  The maps: ens_mean = y + err,
 *     ens_std = sqrt(ss / (M - 1)), ens_abs_err = |err|, crps = skill / M - pair / M^2, fair_crps = skill / M - pair / (M (M - 1)),
 *     afcrps = skill / M - (1 - (1 - alpha) / M) pair / (M (M - 1)).
 *     The members of a point are sorted in registers; the plane sums are fp64.  Two launches per call; no floating-point atomics:
 *     repeated calls and any grouping of variables into calls give identical bits, with maps or without, as long as the variable
 *     takes the same load path (16-byte loads need W % 4 == 0 and every plane base of its members, truth and maps on 16 bytes; the
 *     scalar path sums a tile in another order, so a layout that changes that alignment changes the last bits).  One handle serves one
 *     stream at a time (its scratch and its pointer table are the handle's); the first call and a call with more tiles than any
 *     before allocate, every other call allocates nothing.  A call does not wait for the kernels enqueued before it; it waits
 *     only for the pointer-table upload of the call four calls earlier (the table is staged through four pinned host slots). */
typedef struct wx_ensemble* wx_ensemble_handle;
int wx_ensemble_create(int H, int W, const float* lat_w, int n_members, int device, wx_ensemble_handle* out);
int wx_ensemble_destroy(wx_ensemble_handle h);
int wx_ensemble_apply(wx_ensemble_handle h, int n_vars, const float* const* member_dev, const int64_t* member_batch_stride,
                      const float* const* target_dev, const int64_t* target_batch_stride, const int32_t* n_levels, const int32_t* n_time,
                      int batch, double alpha, float* const* maps_dev, double* planes_dev, void* stream);

/* ---- lat-band sharding of ONE forecast (BASELINE config 4) -----------------------------------------
 * Replaces credit/domain_parallel (manager.py:22 DomainParallelManager, halo_exchange.py:21-79, layers.py:29-626,
 * sharding.py:13-68) and credit/parallel/domain.py:25-110 (shard_spatial / gather_spatial) for the inference path.
 * Rank r of n owns a window-aligned band of latitude rows of every stage map (csrc/wx_band.h).  A forecast step is a
 * sequence of compute segments separated by EXCHANGES (conv halos, the row redistribution that keeps the dilated "long"
 * attention exact, the GroupNorm sums); the engine packs what it must send into a staging buffer and returns, the
 * caller moves bytes between ranks (torch.distributed P2P over RCCL/xGMI, or any other transport) and resumes:
 *
 *     wx_band_enable(h, rank, n);  wx_band_info(...);  wx_band_set_staging(h, send, sb, recv, rb);
 *     xid = wx_band_begin(h, x_band, frc_band, y_band, y_phys_band, x_next_band, stream, &xid);
 *     while (xid >= 0) { wx_band_exchange(h, xid, sends, ..., recvs, ...);  <move the bytes>;  wx_band_resume(h, &xid); }
 *
 * x / frc / y / y_phys / x_next are BANDS: [channels][own_rows][W] float32, rows own_row0 .. own_row0+own_rows-1 of the grid.
 * Semantics of the step are those of wx_step.  The result equals the unsharded engine's up to fp32 summation order of
 * the GroupNorm statistics (summed in rank order: identical on every rank). */
typedef struct wx_band_msg {
  int32_t peer;      /* the other rank */
  int64_t offset;    /* byte offset in the send (resp. receive) staging buffer */
  int64_t bytes;
} wx_band_msg;
int wx_band_enable(wx_handle h, int rank, int nranks);
int wx_band_info(wx_handle h, int* own_row0, int* own_rows, int64_t* send_bytes, int64_t* recv_bytes, int* n_exchanges);
int wx_band_set_staging(wx_handle h, void* send_dev, int64_t send_bytes, void* recv_dev, int64_t recv_bytes);
/* messages of exchange `xid` for this rank: at most nranks-1 each way */
int wx_band_exchange(wx_handle h, int xid, wx_band_msg* sends, int cap_sends, int* n_sends, wx_band_msg* recvs, int cap_recvs,
                     int* n_recvs);
int wx_band_begin(wx_handle h, const float* x_band, const float* frc_band, float* y_band, float* y_phys_band, float* x_next_band,
                  void* stream, int* next_xid);
int wx_band_resume(wx_handle h, int* next_xid);   /* *next_xid = -1 when the step is complete */
/* Overlap of an exchange with compute (credit/domain_parallel/halo_exchange.py:45-79 waits for its batch_isend_irecv in place):
 * after this call the caller moves the bytes of every exchange on the returned stream (`adopt_stream`, or one the engine creates when
 * it is NULL) instead of the compute stream.  wx_band_begin / wx_band_resume make that stream wait for the pack kernel, launch the
 * part of the NEXT op that does not need the exchange (the interior rows of the 3x3 convolution behind a halo exchange) on the
 * compute stream, and wx_band_resume makes the compute stream wait for whatever the caller has put on the transport stream before
 * it unpacks.  wx_band_step_rccl does the same with its own stream when env WX_BAND_OVERLAP=1.  OFF by default: measured on MI355X
 * (profiles/r03_latband_overlap_virtual_ranks_C3_bf16.txt) the two extra one-row launches and the two cross-stream event edges per exchange cost more than
 * the ~20 us halo exchange they hide. */
int wx_band_comm_stream(wx_handle h, void* adopt_stream, void** stream_out);
/* RCCL transport inside the engine (one process per GPU; xGMI peer-to-peer): rank 0 draws an id, every rank receives it
 * through any side channel (the Python shim broadcasts it with torch.distributed), wx_band_rccl_init creates the
 * communicator (ncclCommInitRank), and wx_band_step_rccl runs a whole step with a grouped ncclSend/ncclRecv per exchange
 * on the compute stream -- no host code between segments.  librccl is bound with dlopen on first use (no link dependency);
 * staging buffers are allocated by the engine when wx_band_set_staging was not called. */
int wx_band_rccl_unique_id(uint8_t id[128]);
int wx_band_rccl_init(wx_handle h, const uint8_t id[128]);
int wx_band_step_rccl(wx_handle h, const float* x_band, const float* frc_band, float* y_band, float* y_phys_band, float* x_next_band,
                      void* stream);
/* Host-only view of the same plan (no GPU needed: the CPU tests check it for every rank of a world):
 * rows owned per stage and the (peer, offset, bytes) messages of every exchange. */
typedef struct wx_band_plan_s* wx_band_plan;
int wx_band_plan_create(const wx_config* cfg, int nranks, wx_band_plan* out);
int wx_band_plan_destroy(wx_band_plan p);
int wx_band_plan_num_exchanges(wx_band_plan p, int* n);
int wx_band_plan_exchange_name(wx_band_plan p, int xid, const char** name);
int wx_band_plan_messages(wx_band_plan p, int xid, int rank, wx_band_msg* sends, int cap_sends, int* n_sends, wx_band_msg* recvs,
                          int cap_recvs, int* n_recvs);
/* which: 0..3 = first row of the short layout at that stage, 4..7 = first PHASE of the long layout, 8 = input/output rows;
 * starts[nranks+1] */
int wx_band_plan_partition(wx_band_plan p, int which, int32_t* starts);

/* ---- introspection for parity tests and the roofline report ----------------
 * wx_debug_read: copy an intermediate activation of the LAST forward (batch item 0) to host as
 *   float32 [C, H, W].  Names follow the reference module tree: "pad", "layers.S.0", "layers.S.1",
 *   "layers.S.1.layers.D.J", "up_block1".."up_block4".  Only valid after
 *   wx_set_debug(h, level) and a forward.  level 1: every name above exists -- the engine leaves the routes whose intermediates
 *   never reach memory (the FeedForward launches that take the attention's out-projection in front / the next to_qkv behind,
 *   the k-blocked attention chain) for their unfused forms.  level 2: the engine runs exactly the kernels it runs with
 *   captures off and captures what those leave in memory: a name whose tensor does not exist on the route taken (the attention
 *   sub-block's output "...D.0" / "...D.2" in front of a FeedForward that took the out-projection) is reported missing;
 *   "<attention>.attn" (the attention output in front of to_out) and "<attention>.qkv" (q|k|v, [3C, H, W]; bf16 engine: the q
 *   channels carry dim_head^-0.5 * log2(e)) are captured wherever they are row-major in memory -- not in the k-blocked chain
 *   nor inside the one-launch attention block.  Level 2 changes no arithmetic: the forward is bit-identical to level 0's.
 *   At either level the decoder's stored intermediates are captured too (not in lat-band mode): "up_blockN.up" (the shortcut),
 *   "up_blockN.c1" / ".n1" / ".c2" (first 3x3 conv, GroupNorm + SiLU, second 3x3 conv), "up_blockN.ps" / "up_block4.ps" (wxformer:
 *   the pixel-shuffled map) and "up_blockN.us" / "up_block4.us" (upsample_v_conv: the upsampled input), N = 1..3.
 *   level 0: off.  No forward is captured into a graph while a level is on.
 * wx_profile: when enabled, every kernel launch is bracketed by HIP events on the launch stream;
 *   wx_profile_read returns per-kernel-class totals since the last wx_profile_reset.  enable: 1 per class ("gemm_ff1"),
 *   2 per class and stage ("gemm_ff1.s2"), 3 additionally tags launches that took a non-default kernel family
 *   ("gemm_ff1.s2@stream": the persistent GEMM) -- what the parity tests use to prove which kernel they exercised.
 */
int wx_set_debug(wx_handle h, int level);
int wx_debug_read(wx_handle h, const char* name, float* host_out, int64_t capacity, int64_t shape[3]);

typedef struct wx_kernel_stat {
  char name[48];
  int64_t launches;
  double ms;          /* summed HIP-event time */
  double flops;       /* algorithmic FLOPs issued by these launches (2*MAC) */
  double bytes;       /* algorithmic HBM bytes (each operand read/written once) */
} wx_kernel_stat;
 /* wx_query: one integer fact about the engine / its LAST forward, by name -- which schedule and precision variant actually ran (what a
 * parity test needs to prove it exercised the path it names; the reference has no counterpart: its "schedule" is ATen's).  Keys:
 *   "launches"           kernel launches of the last forward
 *   "gemm8p_launches"    ... of which ran on the eight-phase kernel (wx_gemm8p.h: the decoder's deep-K convolutions, round 6)
 *   "splitk_gemms"       ... of which were plain convolutions split over K ranges with a fixed-order finish kernel (CrossEmbed GEMMs of
 *                        small maps)
 *   "attn_blk"           attention sub-blocks of the last forward whose q|k|v and attention output travelled k-blocked (round 6)
 *   "attn_nkf_mask"      bit n set: the last forward launched window_attn_kernel with NKF == n key fragments of 16 tokens (n in 1, 2, 4,
 *                        7, 8, 10, 12, 14, 16: windows of <= 16, 32, 64, 112, 128, 160, 192, 224, 256 tokens)
 *   "attn_block_nkf_mask" ... attn_block_kernel (the one-launch attention sub-block, bf16) with NKF == n (n in 1, 2, 4, 7, 8)
 *   "precision"          the wx_config precision the engine was created with
 *   "split_gemms"        GEMM launches of the last forward that ran split-bf16 arithmetic (WX_PREC_FP32_SPLIT)
 *   "ff_split_fused"     ... of whose FeedForward sub-blocks ran as ONE launch (wx_ff_split.h; each counts two split GEMMs), and of those
 *   "ff_split_pre"       how many also applied the attention's out-projection + residual in front (three GEMMs in the launch),
 *   "ff_split_post"      how many also produced the next attention's q|k|v behind (four)
 * Unknown key -> WX_ERR_INVALID. */
int wx_query(wx_handle h, const char* key, int64_t* value);
int wx_profile(wx_handle h, int enable);
int wx_profile_reset(wx_handle h);
int wx_profile_read(wx_handle h, wx_kernel_stat* out, int capacity, int* count);

const char* wx_last_error(void);
const char* wx_version(void);

#ifdef __cplusplus
}
#endif
#endif /* WXENGINE_H */
