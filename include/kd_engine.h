/*
 * kd_engine.h — C ABI of libkd_engine.so, the MI355X (gfx950) denoising engine that sits
 * under the drop-in `imagen_pytorch` package of this repo.
 *
 * The reference (jameshball/kidney-diffusion) has no FFI: its hot path is the Python API of
 * the third-party `imagen-pytorch==1.18.5` (reference requirements.txt:37).  Each entry point
 * below names the reference-side call it replaces (file:line in /root/reference) and, for the
 * arithmetic, the SURVEY.md Appendix A item it implements.
 *
 * Conventions
 *   - every pointer named d_* is a DEVICE pointer (HBM), borrowed, never freed by the library;
 *   - `stream` is a hipStream_t passed as void*; all launches are stream-ordered.  What synchronises:
 *     kd_unet_create[_shared] (allocates, packs the weights, device-synchronises); the FIRST
 *     kd_sample_* call on a plan (hipMalloc of the sampler scratch, capture + instantiate of the step
 *     graph); a kd_sample_* call whose schedule differs from the previous call's (one stream
 *     synchronise + one asynchronous table upload; an unchanged schedule uploads nothing);
 *     kd_unet_profile and the single-kernel test entry points.  Successive calls on one plan must be
 *     issued on one stream (or otherwise ordered): the plan owns ONE workspace;
 *   - every function returns 0 on success, non-zero on failure; kd_last_error() gives the text;
 *   - images are fp32 NCHW exactly as the reference passes them (sample_ultra_res.py:183-195);
 *     feature maps inside the engine are fp32 NHWC (DESIGN.md "Data layout").
 */
#ifndef KD_ENGINE_H
#define KD_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KD_MAX_LEVELS 8

const char* kd_last_error(void);
/* ABI version of this header: bumped whenever an entry point changes its arguments or a struct its layout, so that a
 * caller built against an older header can refuse the library instead of passing short structs.  History:
 *   1  rounds 1-3
 *   2  round 4/5: kd_conv3x3_winograd4_nhwc gained `gemm_bf16x3` (before `stream`); kd_unet_config_t gained
 *      `gemm_bf16x3`, `x3_linear` and `wino4_max_images`, kd_sample_args_t `cond_table_max_mb`; kd_unet_cond_table_refused_bytes, kd_linear_bf16x3 (+ _seg_rows), kd_downsample_bf16x3, kd_layernorm_ex and kd_layernorm_linear_bf16x3 added;
 *      kd_unet_cond_table_build_ms takes a non-const handle (it reads the build's events on demand); later additions that
 *      change no existing entry: kd_linear_skinny, kd_global_context_gate, kd_gate_add_nhwc (+ _chunks), kd_gn_fold_seg,
 *      kd_wf_ab_scale, kd_gn_conv3x3_winograd4_nhwc (the ResnetBlock pieces the plan joins, for unit tests); kd_unet_create_ext
 *      with its struct kd_unet_ext_t for linear attention, kd_linattn_chunk_tokens, kd_linattn_dwconv_nhwc, kd_linattn_context,
 *      kd_linattn_apply; kd_attention_ex and kd_l2norm_heads (the attention core and the qk-norm with the plan's argument
 *      forms, for unit tests); kd_text_select, kd_add_rows_bcast, kd_mean_rows and kd_copy_rows (the text plan's small kernels,
 *      for unit tests); kd_unet_text_cond accepts d_text_mask = NULL (text_mask = None); kd_unet_ext_t gained `cross_embed_downsample`
 *      and `upsample_nearest` at its end (zero = the plans of before); kd_upsample_nearest_conv3x3_nhwc added; kd_unet_create_ext2
 *      with its struct kd_unet_ext2_t for `combine_upsample_fmaps` - kd_unet_create_ext is that call with ext2 = NULL - and
 *      kd_upsample_nearest_gn_conv3x3_nhwc added; kd_unet_config_t::attn_dim_head accepts 32 and 128 beside 64 (kd_attention too);
 *      kd_unet_create_ext3 with its struct kd_unet_ext3_t for `layer_attns_depth` - kd_unet_create_ext2 is that call with
 *      ext3 = NULL - and kd_attention_ex_d, kd_l2norm_heads_d, kd_attention_key_tile added (kd_attention_ex / kd_l2norm_heads
 *      are those with D = 64); kd_unet_poison_scratch added (test infrastructure); kd_sample_args_t gained `seeds` at its end
 *      (NULL = the keying of before) and kd_philox_normal_rows added; kd_sample_start added (the start of a stage, x_T);
 *      kd_solver_sample_loop / kd_solver_sample_steps with their struct kd_solver_schedule_t added (DDIM, DPM-Solver++(2M));
 *      kd_unet_create_ext4 with its struct kd_unet_ext4_t for the first and the last layer's structural switches
 *      (`init_cross_embed`, `init_conv_kernel_size`, `init_cross_embed_kernel_sizes`, `final_conv_kernel_size`,
 *      `final_resnet_block`, `scale_skip_connection`) - kd_unet_create_ext3 is that call with ext4 = NULL - and
 *      kd_final_conv_k_nchw, kd_init_conv_plain_nchw added; kd_tiles_gather and kd_tiles_fuse_update added (fused-tile
 *      canvas sampling); kd_tiles_cond_gather, kd_tiles_gather_lowres and kd_tiles_finalize added (a fused-tile stage at the
 *      sizes of a magnification level); kd_tiles_start, kd_tiles_fuse_update_known and kd_tiles_finalize_known with their
 *      structs kd_tiles_image_t and kd_tiles_mask_t added (a fused-tile canvas that keeps known pixels or starts from an image);
 *      kd_sample_args_t gained `keep_self_cond` at its end (zero = the reset at step 0 of before); kd_tiles_finalize_known
 *      accepts known = mask = NULL (kd_tiles_finalize's bits) - kd_tiles_fuse_update and kd_tiles_finalize are the _known calls
 *      with nothing known, no existing entry changed; kd_tiles_rows_copy and kd_tiles_finalize_rows added (a fused-tile canvas
 *      cut into shards over several devices); kd_solver3_sample_loop / kd_solver3_sample_steps with their struct
 *      kd_solver3_schedule_t - DPM-Solver++(3M), the SDE forms of 2M and 3M - and kd_tiles_fuse_update_hist2 added:
 *      kd_solver_sample_* and kd_tiles_fuse_update_known are those with no second history, no existing entry changed */
#define KD_ENGINE_ABI_VERSION 2
int kd_version(void);
/* sha256 prefix (16 hex digits) of the sources this binary was compiled from (csrc/build_id.py); a build with
 * EXTRA flags carries the suffix "+experiment".  The Python binding refuses a library whose id differs from
 * the sources lying next to it. */
const char* kd_build_id(void);

/* ------------------------------------------------------------------------------------------
 * UNet.  Replaces `Unet(...)` construction + `Unet.forward` of imagen-pytorch as configured at
 * train_ultra_res.py:29-60, train.py:30-65, train_uncond.py:30-61.
 * ---------------------------------------------------------------------------------------- */
typedef struct kd_unet_config {
  int dim;
  int num_levels;
  int dim_mults[KD_MAX_LEVELS];
  int num_resnet_blocks[KD_MAX_LEVELS];
  int layer_attns[KD_MAX_LEVELS];
  int layer_cross_attns[KD_MAX_LEVELS];
  int cond_dim;               /* already defaulted to dim by the host */
  int channels;               /* image channels of x, self_cond, lowres and the output: 1 .. 4 (RGB: 3) */
  int cond_images_channels;   /* 0 / 3 / 4 / 6 */
  int lowres_cond;            /* set by Imagen for unets after the first */
  int memory_efficient;
  int init_conv_to_final_conv_residual;
  int cond_on_text;
  int text_tokens;            /* number of pooled text tokens handed to forward (0 if none) */
  int attn_heads;             /* 8 */
  int attn_dim_head;          /* 32, 64 or 128 (64 with linear attention) */
  int ff_mult_x2;             /* 2*ff_mult, integer (4 for ff_mult=2) */
  int num_time_tokens;        /* 2 */
  int sinu_dim;               /* learned_sinu_pos_emb_dim, 16 */
  int resnet_groups;          /* 8 */
  int attend_at_middle;       /* 1 */
  int use_gca;                /* use_global_context_attn, 1 */
  /* static shape of the plan */
  int batch;
  int image_size;             /* S: x is [batch, channels, S, S] */
  /* 0 = auto: for the ResnetBlock 3x3 convs Winograd F(2x2,3x3) as 16 batched GEMMs from Cin >= 256,
   * the fused Winograd kernel below that where the map is a multiple of 16x16, Cout of 64 and the
   * launch fills the chip, direct implicit GEMM elsewhere; 1 = direct implicit GEMM everywhere
   * (bitwise the k-ordered fmaf chain); 2 = as 0 without the fused kernel; 3 = as 0 with the fused
   * kernel wherever its shape rules allow (tests); n >= 32 = batched-GEMM Winograd from Cin >= n
   * (experiments / tests) */
  int conv_algo;
  /* Attention similarity variant - imagen-pytorch changed it between versions, and the reference's pinned
   * 1.18.5 is not available to check: 0 = q * dim_head^-0.5 . k (the library default
   * the reference's configs get); 1 = `Unet(cosine_sim_attn=True)`: l2norm(q) . l2norm(k) * 16;
   * 2 = learned per-channel `q_scale` / `k_scale` on the normalised q / k, * 8 (later versions; the host
   * switches to it when a checkpoint carries those keys).  Applies to self-, cross- and text-pooling attention. */
  int attn_qk_norm;
  /* Structural forks between library versions, named by a checkpoint's keys / shapes:
   * downsample_conv4 = 1: Downsample is `Conv2d(dim, dim_out, 4, stride 2, pad 1)` (parameters `<pre>.weight`
   * [d_out, d, 4, 4], `<pre>.bias`) instead of pixel-unshuffle + 1x1 conv (`<pre>.1.weight` [d_out, 4 d, 1, 1]);
   * mid_attn_plain = 1: mid_attn is a residual multi-query attention without a feed-forward (parameters
   * `mid_attn.fn.fn.*`) instead of a TransformerBlock (`mid_attn.layers.0.{0,1}.*`). */
  int downsample_conv4;
  int mid_attn_plain;
  /* Batched-GEMM Winograd layers: cap of the V + D transform buffers per slice of tiles in MiB (the map is walked in
   * slices, bit-identical results); 0 = one slice (default: fastest, largest workspace). */
  int wino_slice_mb;
  /* Winograd F(4x4,3x3) (36 batched GEMMs over tiles of 4x4 outputs) for the ResnetBlock 3x3 convs with at least this
   * many input channels whose GEMMs fill the chip; 0 = default (512; 128 where the GEMMs run on bf16x3), < 0 = never.  fp32 throughout; per-conv relative
   * L2 against fp64 3-4e-6 (F(2x2,3x3): 5e-7) - inside the 2e-5 the UNet forward is held to. */
  int wino43_min_cin;
  /* The position GEMMs of those F(4x4,3x3) layers on the bf16 matrix pipe, every fp32 operand carried as three bf16
   * pieces (a = ah + am + al exactly) and six exact products accumulated in fp32 per k-step (kernels_gemm_bf16x3.hip):
   * fp32-class results - error against fp64 not above the fp32 MFMA path's - at 3/8 of its matrix cycles.
   * 0 = default (where tiles % 256 == 0, Cout % 128 == 0; with it F(4x4,3x3) is taken from Cin >= 128), < 0 = never
   * (fp32 MFMA).  The transformed input V reaches the GEMM either as the three planes, written by the input transform
   * (1 = always), or as fp32 that the GEMM's loader waves split on the way into LDS (2 = always): a third less V traffic
   * for vector work beside the MFMA waves.  0 picks per layer: fp32 where the GEMM waits for HBM rather than for the matrix
   * pipe (Cin Cout / (6 Cin + 4 Cout) < 40: the 64 x 64 level and above of the SR UNet), planes elsewhere.  Same results
   * bit for bit either way. */
  int gemm_bf16x3;
  /* Token GEMMs and 1x1 convs (attention projections, feed-forward, skip convs without output statistics) on the same
   * bf16x3 kernel in its epilogue form (bias / residual / gate, strided rows; the fp32 activations are split by the
   * kernel's loader waves): 0 = default (K >= 512 input channels, rows % 256 == 0, Cout % 128 == 0, at least 64 tiles of
   * 256 x 128; needs gemm_bf16x3 >= 0 and conv_algo == 0), n > 0 = K >= n, < 0 = never (conv_buf_kernel, fp32 MFMA). */
  int x3_linear;
  /* F(4x4,3x3) layers - and the 1x1 convs on the bf16x3 kernel - run in sets of at most this many images, one set of
   * launches after the other (V and D of one set) (0 = default: the whole batch, or - where V / D / the maps of the whole
   * batch pass the 4 GB a buffer resource spans, unet3's outer levels at batch 8 - the largest divisor of the batch that
   * fits).  A test knob: results equal the whole-batch plan's to fp32 rounding (the k-cut of left-over tiles follows the
   * tile count). */
  int wino4_max_images;
} kd_unet_config_t;

/* One named parameter tensor of the UNet's state_dict (key WITHOUT the `unets.N.` prefix,
 * e.g. "downs.0.1.block1.project.weight"), fp32, contiguous, torch layout, on the device. */
typedef struct kd_param {
  const char* name;
  const float* d_data;
  int64_t numel;
} kd_param_t;

typedef struct kd_unet kd_unet_t;

/* Builds the execution plan, re-packs the weights into the engine's layouts (copies; the
 * caller may free its tensors afterwards) and allocates the activation workspace. */
int kd_unet_create(const kd_unet_config_t* cfg, const kd_param_t* params, int n_params,
                   kd_unet_t** out);
/* Same, for another (batch, image_size[, conv_algo]) plan of the SAME UNet: the new plan shares the
 * packed weights of `share_with` (and packs only the forms that plan does not have yet), so a UNet
 * sampled at several batch sizes keeps one copy of its weights in HBM.  `params` must hold the same
 * values as when `share_with` was created.  The store lives until the last plan is destroyed. */
int kd_unet_create_shared(const kd_unet_config_t* cfg, const kd_param_t* params, int n_params,
                          const kd_unet_t* share_with, kd_unet_t** out);
/* Same, for a self-conditioned UNet (library `Unet(self_cond=True)`) when self_cond != 0: its init conv reads
 * cat(cond_images, x, self_cond, lowres) (init_conv.convs.*.weight with 3 more input channels), and the samplers carry
 * the thresholded x0 estimate of each step into the next forward.  share_with must have the same self_cond. */
int kd_unet_create_self_cond(const kd_unet_config_t* cfg, const kd_param_t* params, int n_params,
                             const kd_unet_t* share_with, int self_cond, kd_unet_t** out);
/* Structural options beyond kd_unet_config_t, for kd_unet_create_ext: library kwargs the first plans did not have.
 * use_linear_attn[l]: level l's attention slot (downs.l.3 / the matching ups.j.2) holds a LinearAttentionTransformerBlock
 * where layer_attns[l] is 0 (full attention wins); use_linear_cross_attn[l]: the level's first ResnetBlock on each path
 * (downs.l.1, ups.j.0) has cross-attention, and it is a LinearCrossAttention.  Entries from num_levels on are ignored. */
typedef struct kd_unet_ext {
  int self_cond;   /* as kd_unet_create_self_cond */
  int use_linear_attn[KD_MAX_LEVELS];
  int use_linear_cross_attn[KD_MAX_LEVELS];
  /* The library's other resampling layers.  cross_embed_downsample = 1 (`Unet(cross_embed_downsample=True)`, kernel sizes
   * (2, 4)): every Downsample is a CrossEmbedLayer, cat(Conv2d(d, d_out / 2, 2, stride 2), Conv2d(d, d_out - d_out / 2, 4,
   * stride 2, pad 1)) with parameters `<pre>.convs.{0,1}.{weight,bias}`; d_out must be even.  upsample_nearest = 1
   * (`Unet(pixel_shuffle_upsample=False)`): every Upsample is nn.Upsample(2, nearest) -> Conv2d(d, d_out, 3, padding 1),
   * parameters `<pre>.1.{weight,bias}`, no activation; needs d % 8 == 0 and d_out % 32 == 0 (refused at build otherwise). */
  int cross_embed_downsample;
  int upsample_nearest;
} kd_unet_ext_t;
/* kd_unet_create_self_cond with the options of `ext` (NULL = all zero: the plan of kd_unet_create_shared).  An ext with
 * every linear flag zero gives the same plan - the same launches and the same bits - as kd_unet_create_self_cond. */
int kd_unet_create_ext(const kd_unet_config_t* cfg, const kd_param_t* params, int n_params, const kd_unet_t* share_with,
                       const kd_unet_ext_t* ext, kd_unet_t** out);
/* Further structural options, for kd_unet_create_ext2; kd_unet_ext_t keeps its size.  combine_upsample_fmaps = 1
 * (`Unet(combine_upsample_fmaps=True)`): the map of every up level i (after ups.i.2, before its upsample) goes through
 * `upsample_combiner.fmap_convs.i` = GroupNorm(8) -> SiLU -> Conv2d(dim_out_i, dim, 3, padding 1) at full resolution (nearest
 * upsampling by the integer factor between the two maps), and final_res_block reads cat(x, those L maps[, init conv
 * residual]): dim (1 + L) [+ dim] channels.  Needs dim % 32 == 0 and every level's width % 8 == 0 (refused at build otherwise). */
typedef struct kd_unet_ext2 {
  int combine_upsample_fmaps;
} kd_unet_ext2_t;
/* kd_unet_create_ext with the options of `ext2` (NULL = all zero: the plan of kd_unet_create_ext, the same launches and the
 * same bits). */
int kd_unet_create_ext2(const kd_unet_config_t* cfg, const kd_param_t* params, int n_params, const kd_unet_t* share_with,
                        const kd_unet_ext_t* ext, const kd_unet_ext2_t* ext2, kd_unet_t** out);
/* Further structural options, for kd_unet_create_ext3; the older structs keep their size.  layer_attns_depth[l]
 * (`Unet(layer_attns_depth=...)`): the TransformerBlocks of level l (downs.l.3 and the matching ups.j.2) run that many
 * (attention, feed-forward) pairs, parameters `<pre>.layers.{i}.{0,1}.*`; 0 means 1.  mid_attn keeps depth 1, as in the library.
 * A linear-attention level (kd_unet_ext_t::use_linear_attn) takes depth 1 only.  Entries from num_levels on are ignored. */
typedef struct kd_unet_ext3 {
  int layer_attns_depth[KD_MAX_LEVELS];
} kd_unet_ext3_t;
/* kd_unet_create_ext2 with the options of `ext3` (NULL, all zero or all one: the plan of kd_unet_create_ext2, the same
 * launches and the same bits). */
int kd_unet_create_ext3(const kd_unet_config_t* cfg, const kd_param_t* params, int n_params, const kd_unet_t* share_with,
                        const kd_unet_ext_t* ext, const kd_unet_ext2_t* ext2, const kd_unet_ext3_t* ext3, kd_unet_t** out);
/* Further structural options, for kd_unet_create_ext4; the older structs keep their size.  0 is the library's default in
 * every field.
 *   init_plain = 1 (`Unet(init_cross_embed=False)`): the first layer is one Conv2d(init_channels, dim, k, padding k / 2),
 *     parameters `init_conv.{weight,bias}`, k = init_kernel_size (`init_conv_kernel_size`; 0 means 7; odd, 1 .. 15).
 *   n_init_kernel_sizes = 1 .. 4 (`Unet(init_cross_embed_kernel_sizes=...)`; 0 means the three sizes 3, 7, 15):
 *     init_kernel_sizes[i], ascending, odd, 1 .. 15, are the sizes of the CrossEmbedLayer's convs `init_conv.convs.i`, of
 *     widths dim / 2, dim / 4, .., the rest (each a multiple of 4).  Ignored with init_plain.
 *   final_kernel_size (`final_conv_kernel_size`; 0 means 3): 1, 3, 5 or 7, `final_conv.weight` [C][fin][k][k].
 *   no_final_resnet_block = 1 (`Unet(final_resnet_block=False)`): there is no `final_res_block`; final_conv reads
 *     cat(x[, the UpsampleCombiner's maps][, the init conv residual][, lowres_cond_img]).
 *   no_skip_scale = 1 (`Unet(scale_skip_connection=False)`): skip tensors enter the up path unscaled; no scale pass runs.
 *   init_generic = 1 (engine extension, for A/B measurements): the init conv's per-step share runs on the generic conv path
 *     (pack of the planes + one implicit-GEMM conv per kernel size) even where a one-kernel form takes the shape. */
typedef struct kd_unet_ext4 {
  int init_plain;
  int init_kernel_size;
  int init_kernel_sizes[4];
  int n_init_kernel_sizes;
  int final_kernel_size;
  int no_final_resnet_block;
  int no_skip_scale;
  int init_generic;
} kd_unet_ext4_t;
/* kd_unet_create_ext3 with the options of `ext4` (NULL or all zero: the plan of kd_unet_create_ext3, the same launches and
 * the same bits). */
int kd_unet_create_ext4(const kd_unet_config_t* cfg, const kd_param_t* params, int n_params, const kd_unet_t* share_with,
                        const kd_unet_ext_t* ext, const kd_unet_ext2_t* ext2, const kd_unet_ext3_t* ext3,
                        const kd_unet_ext4_t* ext4, kd_unet_t** out);
void kd_unet_destroy(kd_unet_t* u);
/* bytes of HBM held (weights + workspace) and algorithmic MACs of one forward (whole batch) */
int64_t kd_unet_hbm_bytes(const kd_unet_t* u);
int64_t kd_unet_weight_bytes(const kd_unet_t* u);  /* the (possibly shared) packed-weight store alone */
int64_t kd_unet_macs(const kd_unet_t* u);
/* MACs the conv / GEMM launches of one step actually issue on the matrix cores: smaller than
 * kd_unet_macs where a 3x3 conv runs as Winograd F(2x2,3x3) (16/36 of its MACs) and by the
 * step-invariant share of the init / final conv that is hoisted out of the step */
int64_t kd_unet_mfma_macs(const kd_unet_t* u);
/* bf16 MACs the plan's bf16x3 GEMMs issue per forward (six per fp32 MAC of theirs; not included in kd_unet_mfma_macs) */
int64_t kd_unet_mfma_bf16_macs(const kd_unet_t* u);
int kd_unet_num_launches(const kd_unet_t* u);
/* ... of which conditioning launches (functions of log_snr / lowres_log_snr / text only): the sampler replaces them by ONE
 * gather per iteration when it runs from the conditioning table (kd_sample_args_t::cond_table). */
int kd_unet_num_cond_launches(const kd_unet_t* u);
/* device time (ms), row count (*rows) and runs of the conditioning ops (*runs; both may be NULL) of the plan's last
 * conditioning-table build, < 0 if none was built
 * yet.  Rows are built on demand for the schedule steps a call walks, B steps per run of the conditioning ops (their rows
 * are independent over the batch): T / B runs for a whole schedule. */
float kd_unet_cond_table_build_ms(kd_unet_t* u, int* rows, int* runs);
/* > 0: the last sampling call wanted a conditioning table of this many bytes and did not get it (larger than
 * kd_sample_args_t::cond_table_max_mb / an eighth of the free HBM, or the allocation failed): its steps then compute
 * the conditioning themselves - same results, more launches per step */
int64_t kd_unet_cond_table_refused_bytes(const kd_unet_t* u);

/* Step-invariant text conditioning (the text branch of Unet.forward; reached by the
 * reference through sample_cond.py:36-48 / sample.py:51-60): text_to_cond, null-embedding select,
 * PerceiverResampler pooling, to_text_non_attn_cond.  Run once per sample call.
 *   d_text_embeds [B,L,text_embed_dim], d_text_mask [B,L] as floats (!= 0 keeps the token), L <= max_text_len;
 *   d_text_mask = NULL is the library's text_mask = None: all L tokens kept, the rows L .. max_text_len stay the zero padding;
 *   drop = 1 gives the null conditioning (cond_drop_prob = 1, used for classifier-free guidance);
 *   out: d_text_tokens [B,text_tokens,cond_dim], d_text_hiddens [B,time_cond_dim]. */
int kd_unet_text_cond(kd_unet_t* u, const float* d_text_embeds, const float* d_text_mask, int L, int drop,
                      float* d_text_tokens, float* d_text_hiddens, void* stream);

/* Diagnostic: per-launch device time of one forward as CSV "index,label,macs,avg_us,mfma_macs" (macs: the
 * algorithmic MACs of the launch as the reference computes them, mfma_macs: what it issues on the matrix
 * cores; uses the inputs of the preceding kd_unet_forward call; synchronises the stream). */
int kd_unet_profile(kd_unet_t* u, int iters, char* buf, size_t buflen, void* stream);

/* Replaces `unet.forward_with_cond_scale(x, log_snr(t), lowres_cond_img=..,
 * lowres_noise_times=.., cond_images=.., text_embeds=..)` at cond_scale == 1.
 *   d_x            [B,3,S,S]
 *   d_lowres       [B,3,S,S] or NULL (required iff cfg.lowres_cond)
 *   d_cond_images  [B,Cc,S,S] already nearest-resized to S, or NULL (required iff Cc > 0)
 *   d_log_snr      [B] log-SNR of the current time; d_lowres_log_snr [B] or NULL
 *   d_text_tokens  [B,text_tokens,cond_dim] pooled text tokens (pre norm_cond) or NULL
 *   d_text_hiddens [B,time_cond_dim] or NULL
 *   d_out          [B,3,S,S] */
int kd_unet_forward(kd_unet_t* u, const float* d_x, const float* d_lowres,
                    const float* d_cond_images, const float* d_log_snr,
                    const float* d_lowres_log_snr, const float* d_text_tokens,
                    const float* d_text_hiddens, float* d_out, void* stream);
/* Same with the self-conditioning image d_self_cond [B,3,S,S] (NULL = zeros, the library's self_cond = None).  A plan
 * without self_cond ignores it; kd_unet_forward == this with d_self_cond = NULL. */
int kd_unet_forward_self_cond(kd_unet_t* u, const float* d_x, const float* d_self_cond, const float* d_lowres,
                              const float* d_cond_images, const float* d_log_snr, const float* d_lowres_log_snr,
                              const float* d_text_tokens, const float* d_text_hiddens, float* d_out, void* stream);

/* Classifier-free guidance combine of `Unet.forward_with_cond_scale` (sample.py:55-59 reaches it with
 * cond_scale != 1): out = null + (cond - null) * cond_scale over n floats; out may alias cond. */
int kd_cfg_combine(const float* d_cond, const float* d_null, float* d_out, float cond_scale, int64_t n,
                   void* stream);

/* ------------------------------------------------------------------------------------------
 * Sampler.  Replaces `Imagen.p_sample_loop` / `p_sample` / `p_mean_variance` (SURVEY §3.2,
 * A.2) as entered from sample_ultra_res.py:183-195, outpainting.py:146-157,
 * sample_cond.py:40-48, sample_uncond.py:49-55.
 * ---------------------------------------------------------------------------------------- */
enum { KD_OBJ_NOISE = 0, KD_OBJ_V = 1, KD_OBJ_X_START = 2 };

/* Per-(timestep) scalars precomputed by the host in fp32 exactly as the library's torch ops
 * produce them.  All arrays have T entries. */
typedef struct kd_schedule {
  int T;
  const float* log_snr;       /* log_snr(t_k)            -> UNet time input               */
  const float* alpha;         /* sqrt(sigmoid(log_snr))                                    */
  const float* sigma;         /* sqrt(sigmoid(-log_snr))                                   */
  const float* alpha_next;    /* alpha at t_{k+1}                                          */
  const float* sigma_next;    /* sigma at t_{k+1}                                          */
  const float* c;             /* -expm1(log_snr - log_snr_next)                            */
  const float* noise_scale;   /* [t_next != 0] * exp(0.5*log(max(sigma_next^2*c,1e-20)))   */
  /* inpainting re-noise t_next -> t:  x*rn_a + noise*rn_b ; 0-length use allowed if unused */
  const float* rn_a;          /* alpha_t/alpha_next                                         */
  const float* rn_b;          /* (sigma_t*alpha_next - sigma_next*alpha_t)/alpha_next       */
} kd_schedule_t;

typedef struct kd_sample_args {
  int objective;              /* KD_OBJ_*  (train_ultra_res.py:87, train.py:90) */
  int dynamic_threshold;      /* 1: s = max(1, quantile_0.95 |x0|) per sample   */
  float percentile;           /* 0.95 */
  int resample_times;         /* inpaint_resample_times if inpainting else 1 (sample_ultra_res.py:192) */
  /* conditioning, constant over the loop */
  const float* d_lowres;          /* [B,3,S,S] noised low-res conditioning or NULL */
  const float* d_lowres_log_snr;  /* [B] or NULL */
  const float* d_cond_images;     /* [B,Cc,S,S] or NULL */
  const float* d_text_tokens;     /* or NULL */
  const float* d_text_hiddens;    /* or NULL */
  /* inpainting (both NULL or both set): image already normalised to [-1,1] and resized,
   * mask [B,1,S,S] as 0/1 floats (sample_ultra_res.py:149-174) */
  const float* d_inpaint_images;
  const float* d_inpaint_masks;
  /* noise: explicit tensors (parity tests) or on-device Philox (seed) when the pointer is NULL.
   * d_noise_step    [T*R,B,3,S,S]   index (k*R + (R-1-r))
   * d_noise_inpaint [T*R,B,3,S,S]   same indexing (only read when inpainting)
   * d_noise_renoise [T*R,B,3,S,S]   same indexing (only read when inpainting and r != 0) */
  const float* d_noise_step;
  const float* d_noise_inpaint;
  const float* d_noise_renoise;
  uint64_t seed;
  int use_graph;              /* 1: capture one step into a hipGraph and replay it */
  /* classifier-free guidance (sample.py:55-59): pred = null + (cond - null) * cond_scale, two UNet
   * forwards per step when cond_scale != 1; the null conditioning comes from kd_unet_text_cond(drop=1) */
  float cond_scale;           /* 1.0 = off */
  const float* d_null_text_tokens;
  const float* d_null_text_hiddens;
  /* Conditioning table: when the UNet has no text conditioning and (if it is low-res conditioned) the caller states that
   * all B entries of d_lowres_log_snr hold ONE value (what Imagen.sample passes), the time conditioning of a step - time
   * embeddings, FiLM scale / shift of every ResnetBlock, time tokens and their cross-attention K / V - is a function of
   * the schedule index alone: it is computed once per (schedule, value) into a table and restored per iteration by one
   * gather.  Bit-identical results either way.  cond_table: 0 = use it when possible, < 0 = never.  The table is
   * allocated only if T * cond_bytes fits cond_table_max_mb (0 = 4096) and 1/8 of the free HBM (a failed allocation
   * falls back to computing the conditioning in the step); its rows are built for the steps a call walks. */
  int lowres_log_snr_uniform;   /* 1: all entries of d_lowres_log_snr equal lowres_log_snr_value */
  float lowres_log_snr_value;
  int cond_table;
  int cond_table_max_mb;
  /* Per-image Philox keys: a HOST pointer to B values, copied stream-ordered inside the call (the array is free when
   * the call returns), or NULL (a zero-initialised struct): `seed` keys the whole batch tensor as before, the counter
   * being the element index over all B images.  With seeds, image b is keyed seeds[b] and its counter runs inside the
   * image, so it draws bit for bit what a batch-1 call with seed = seeds[b] draws; `seed` is then not read.  Keys and
   * mode live in device memory: the captured step graph serves an int seed, a seed list and any values of either. */
  const uint64_t* seeds;
  /* != 0: a kd_*_sample_steps call that begins at step 0 keeps the self-conditioning carry the plan holds (what
   * kd_sample_set_self_cond left) instead of starting from zeros - a caller that walks the resample slots of step 0 one
   * call each.  0 (a zero-initialised struct): step 0 starts from zeros, as before. */
  int keep_self_cond;
} kd_sample_args_t;

/* Philox stream ids (the `stream_id` of kd_philox_normal; what the sampler draws when a d_noise_* pointer is NULL):
 * purpose in the high 32 bits, iteration k*R + (R-1-r) in the low 32 (k the schedule step, r the resample counting down
 * from R-1; R = 1 without inpainting).  Purposes: 1 the DDPM step's noise (d_noise_step), 2 the noised known pixels of
 * the DDPM inpaint mix (d_noise_inpaint), 3 the DDPM re-noise (d_noise_renoise), 4 the EDM churn (d_noise_step of
 * kd_edm_sample_*), 5 the EDM re-noise (d_noise_renoise), 16 the caller's own draws (the Python package: low 32 bits 1 =
 * low-res augmentation noise, 2 = x_T).  Element j of a stream is component j % 4 of the Philox4x32-10 block at counter
 * (j / 4, stream id) under the key. */
#define KD_PHILOX_PURPOSE_STEP 1
#define KD_PHILOX_PURPOSE_INPAINT 2
#define KD_PHILOX_PURPOSE_RENOISE 3
#define KD_PHILOX_PURPOSE_EDM_CHURN 4
#define KD_PHILOX_PURPOSE_EDM_RENOISE 5
#define KD_PHILOX_PURPOSE_USER 16

/* In: d_img = x_T [B,3,S,S].  Out: d_img = unnormalised sample in [0,1] (clamp, final inpaint
 * paste and (x+1)/2 included).  Runs all T*R denoising iterations on `stream`. */
int kd_sample_loop(kd_unet_t* u, const kd_schedule_t* sched, const kd_sample_args_t* args,
                   float* d_img, void* stream);
/* Runs iterations [k_begin, k_end) only, without the final clamp/unnormalise (used by bench.py
 * to time exactly K steps, and by tests to compare intermediate states).  Self-conditioned plans: k_begin == 0 starts
 * from self_cond = zeros; k_begin > 0 continues from the estimate the plan holds (kd_sample_set_self_cond).
 * sample(skip_steps = s > 0) is kd_sample_set_self_cond(u, NULL, stream) on a self-conditioned plan, then
 * kd_sample_steps(u, ..., s, T) on the x_T of kd_sample_start, then kd_sample_finalize: step k of such a run reads row k
 * of the tables and draws from the stream ids of step k of a full run. */
int kd_sample_steps(kd_unet_t* u, const kd_schedule_t* sched, const kd_sample_args_t* args,
                    float* d_img, int k_begin, int k_end, void* stream);
/* Builds (force != 0: rebuilds) the conditioning-table rows of schedule steps [k_begin, k_end) without sampling, so
 * that the first sampling call of a schedule does not pay for them; *built (may be NULL) = rows built, 0 when the plan
 * runs without a table.  Device time of the build: kd_unet_cond_table_build_ms. */
int kd_sample_build_cond_table(kd_unet_t* u, const kd_schedule_t* sched, const kd_sample_args_t* args, int k_begin,
                               int k_end, int force, int* built, void* stream);
/* The tail of p_sample_loop on its own: clamp(-1,1), paste of the known inpaint pixels,
 * (x+1)/2.  kd_sample_loop == kd_sample_steps(0,T) + kd_sample_finalize. */
int kd_sample_finalize(kd_unet_t* u, const kd_sample_args_t* args, float* d_img, void* stream);
/* What the last executed iteration left behind (parity checks against p_mean_variance of the library):
 * which = 0: the UNet's output eps-hat / v-hat after guidance [B,3,S,S]; 1: the x0 estimate before the
 * threshold clamp [B,3,S,S]; 2: the per-sample dynamic thresholds max(1, quantile_p |x0|) [B].
 * which = 3 / 4 (after an EDM step only, kd_edm_sample_steps): x_hat / d of that step [B,3,S,S].
 * Stream-ordered device-to-device copy into d_out. */
int kd_sample_last(kd_unet_t* u, int which, float* d_out, void* stream);
/* which = 5 (self_cond plans): the self-conditioning planes the plan holds [B,3,S,S] - after a step, the thresholded x0
 * estimate the next forward will read.
 * Self_cond plans: sets that estimate (d_x_start [B,3,S,S], NULL = zeros) before a kd_sample_steps /
 * kd_edm_sample_steps call with k_begin > 0.  NULL is what a run from step skip_steps > 0 starts with (the library's
 * self_cond = None), whatever an earlier call left in the plan. */
int kd_sample_set_self_cond(kd_unet_t* u, const float* d_x_start, void* stream);

/* ------------------------------------------------------------------------------------------
 * Few-step solvers for DDPM-trained UNets (an engine extension; the library has neither): DDIM(eta) and the second-order
 * multistep DPM-Solver++(2M) in its data-prediction form.  An iteration is kd_sample_steps' - inpaint mix, time input,
 * guided forward, x0 estimate, dynamic threshold, re-noise - with one other update:
 *     x <- coef_x[k] x + coef_x0[k] x0c + coef_prev[k] hist + coef_noise[k] N(0,1)
 * x0c = clamp(x0, -s, s) / s the thresholded estimate of this step, hist the x0c the previous step kept.  The host puts
 * the solver into the coefficients (the Python package: solver_tables; DESIGN.md "Few-step solvers").  A term whose
 * coefficient is 0 is left out and its operand is not read: no noise is drawn for a deterministic step, and a first-order
 * step (coef_prev == 0, which the first step a call walks must be) does not depend on what the plan holds.  hist takes a
 * step's x0c in its last resample slot, so all R resamples of step k read the estimate of step k - 1; it lives in the plan
 * from the first call whose schedule has a coef_prev != 0 and persists between calls, as the self-conditioning estimate does.
 * ---------------------------------------------------------------------------------------- */
/* All arrays have T entries; log_snr, alpha, sigma, rn_a, rn_b as in kd_schedule_t - rn_a / rn_b may be NULL without
 * resampling - and the four coefficients are required. */
typedef struct kd_solver_schedule {
  int T;
  const float* log_snr;
  const float* alpha;
  const float* sigma;
  const float* rn_a;
  const float* rn_b;
  const float* coef_x;
  const float* coef_x0;
  const float* coef_prev;
  const float* coef_noise;
} kd_solver_schedule_t;

/* kd_sample_loop with the solver's update: kd_sample_args_t as there; d_noise_step [T*R,B,C,S,S] is read (NULL: Philox
 * purpose 1, the stream ids of kd_sample_loop) only in steps with coef_noise != 0.  The path keeps its own tables and
 * captured iterations, so a plan may alternate between kd_sample_*, kd_edm_sample_* and these without re-capturing. */
int kd_solver_sample_loop(kd_unet_t* u, const kd_solver_schedule_t* sched, const kd_sample_args_t* args, float* d_img,
                          void* stream);
/* Steps [k_begin, k_end) only, without the final clamp / unnormalise; kd_sample_last reports pred / x0 / thresholds as
 * after kd_sample_steps.  k_begin > 0 continues from the self-conditioning estimate and the history the plan holds. */
int kd_solver_sample_steps(kd_unet_t* u, const kd_solver_schedule_t* sched, const kd_sample_args_t* args, float* d_img,
                           int k_begin, int k_end, void* stream);

/* Third order and the SDE forms: DPM-Solver++(3M), and 2M / 3M with noise (the Python package: solver_tables "dpmpp_3m",
 * "dpmpp_2m_sde", "dpmpp_3m_sde").  The update gains one term,
 *     x <- coef_x[k] x + coef_x0[k] x0c + coef_prev[k] h1 + coef_prev2[k] h2 + coef_noise[k] N(0,1)
 * left to right, h1 / h2 the x0c that steps k - 1 / k - 2 kept.  The plan holds the two estimates as a ring indexed by the
 * step's parity, read on the device from the iteration counter: step k reads h1 in slot (k - 1) & 1 and h2 in slot k & 1 and,
 * in its last resample slot, writes its own x0c into slot k & 1, each thread behind its own read - one captured step serves
 * every step and nothing is copied.  Under resampling all R slots of step k read the estimates of steps k - 1 and k - 2.
 * A zero coefficient leaves its operand unread; step 0 must be first order and step 1 at most second order
 * (coef_prev[0] == coef_prev2[0] == coef_prev2[1] == 0, checked when k_begin == 0; a caller that starts at k_begin > 0 keeps
 * the same rule for its first two steps unless it continues a walk), so a call does not depend on what the ring holds.  The
 * ring's second slot lives in the plan from the first call whose coef_prev2 is not all zero and persists like the first.
 * coef_prev2 == NULL or all zero IS kd_solver_sample_*: the same launches, arguments, arithmetic and captured step. */
typedef struct kd_solver3_schedule {
  int T;
  const float* log_snr;
  const float* alpha;
  const float* sigma;
  const float* rn_a;
  const float* rn_b;
  const float* coef_x;
  const float* coef_x0;
  const float* coef_prev;
  const float* coef_noise;
  const float* coef_prev2;
} kd_solver3_schedule_t;
int kd_solver3_sample_loop(kd_unet_t* u, const kd_solver3_schedule_t* sched, const kd_sample_args_t* args, float* d_img,
                           void* stream);
int kd_solver3_sample_steps(kd_unet_t* u, const kd_solver3_schedule_t* sched, const kd_sample_args_t* args, float* d_img,
                            int k_begin, int k_end, void* stream);

/* ------------------------------------------------------------------------------------------
 * EDM sampler.  Replaces `ElucidatedImagen.sample` / `one_unet_sample` / `preconditioned_network_forward` of
 * imagen-pytorch 1.18.x (the sampler of the reference's commented-out constructor, train.py:97-110): Karras et al.'s
 * stochastic Heun sampler - churn, two preconditioned UNet forwards per step (one on the last step), dynamic
 * threshold of each denoised estimate, RePaint re-noise when inpainting.
 * ---------------------------------------------------------------------------------------- */
/* Per-step scalars for steps k = 0..N-1, computed by the host as the library does: sigma_hat = sigma + gamma sigma,
 * churn = sqrt(sigma_hat^2 - sigma^2), euler_step = sigma_next - sigma_hat, heun_step = 0.5 (sigma_next - sigma_hat),
 * renoise = sigma - sigma_next in double, rounded to fp32; c_in / c_skip / c_out / c_noise (the UNet's time input) of
 * sigma_hat and of sigma_next by fp32 torch ops.  A step with sigma_next == 0 (only the last may have it) runs without
 * the second-order correction.  All arrays have N entries. */
typedef struct kd_edm_schedule {
  int N;
  float S_noise;              /* churn noise = S_noise * N(0,1) */
  const float* sigma;
  const float* sigma_hat;
  const float* sigma_next;
  const float* churn;
  const float* euler_step;
  const float* heun_step;
  const float* renoise;
  const float* c_in_hat;
  const float* c_skip_hat;
  const float* c_out_hat;
  const float* c_noise_hat;
  const float* c_in_next;
  const float* c_skip_next;
  const float* c_out_next;
  const float* c_noise_next;
} kd_edm_schedule_t;

/* In: d_img = sigma_0 * N(0,1) [B,3,S,S].  Out: d_img = unnormalised sample in [0,1] (kd_sample_finalize included).
 * kd_sample_args_t as for kd_sample_loop, with these differences: `objective` is ignored (the UNet is EDM-
 * preconditioned); d_noise_step [N*R,B,3,S,S] holds the churn draws N(0,1) (before S_noise), d_noise_renoise the
 * re-noise draws, both indexed (k*R + (R-1-r)); d_noise_inpaint is not read.  The conditioning table holds 2N rows
 * (the time input at sigma_hat and at sigma_next of every step).  One captured graph per step kind (with and without
 * the Heun correction), replayed. */
int kd_edm_sample_loop(kd_unet_t* u, const kd_edm_schedule_t* sched, const kd_sample_args_t* args, float* d_img,
                       void* stream);
/* Steps [k_begin, k_end) only, without the final clamp / unnormalise.  kd_sample_last then reports the last forward of
 * the last iteration: which = 0 its UNet output after guidance, 1 the denoised estimate c_skip x + c_out net before
 * the threshold, 2 the thresholds; 3 x_hat and 4 d = (x_hat - thr(den)) / sigma_hat of that iteration.
 * sample(skip_steps = s > 0) runs [s, N) on x = sigma_0 z + image (kd_sample_start with scale = sigma[0], whatever s
 * is), behind kd_sample_set_self_cond(u, NULL, stream) on a self-conditioned plan, and then kd_sample_finalize. */
int kd_edm_sample_steps(kd_unet_t* u, const kd_edm_schedule_t* sched, const kd_sample_args_t* args, float* d_img,
                        int k_begin, int k_end, void* stream);

/* ------------------------------------------------------------------------------------------
 * Individual kernels, exported so that tests/ can check each one against the oracle through
 * the same ABI the plan uses internally.
 * ---------------------------------------------------------------------------------------- */

/* Test infrastructure, not part of the sampling path: sets every 32-bit word of the plan's scratch to `word` with
 * hipMemsetD32Async on `stream` and reports the bytes filled in *bytes_filled (may be NULL).  At the start of a forward or
 * of a sampling call every byte of that scratch is undefined - nothing initialises it when it is allocated - so results
 * must not change under this call, whatever the word (tests/test_poisoned_scratch_gpu.py: NaN, 1e30, 0).
 *   Filled: the activation workspace (every tensor has its producer in the same forward; the step-invariant planes are
 *   rewritten at the start of every kd_unet_forward and of every sampling call), the conditioning region (written by the
 *   conditioning ops, or restored whole from the table, in every forward), the bf16x3 GEMMs' k-cut slabs if the plan has
 *   such layers, and those of the sampler's buffers that exist: UNet output, guidance output, x0 estimate, thresholds,
 *   times, EDM x_hat / d / UNet input (each written inside an iteration before it is read), the self-conditioning planes
 *   (zeroed at step 0 of a call) and the quantile workspace (integers, every one set by the quantile's first kernel
 *   before another indexes or counts with it).
 *   Left alone, as state that outlives a call: weights and packed weights with the index tables cached beside them, the
 *   device-resident iteration counter and seed, the schedule tables, the conditioning table and its row layout,
 *   captured graphs, and the text conditioning's outputs (the caller's buffers).
 * Call it only where nothing is live: before a whole forward or sampling call - read kd_sample_last first, seed
 * kd_sample_set_self_cond afterwards - and do not run kd_unet_profile behind it (it replays the steps without the
 * step-invariant part). */
int kd_unet_poison_scratch(kd_unet_t* u, uint32_t word, int64_t* bytes_filled, void* stream);

/* 2-D convolution as implicit GEMM on fp32 MFMA.  x: NHWC [B,Hi,Wi,Cin]; w: torch OIHW
 * [Cout,Cin,KH,KW] (re-packed internally on each call of this test entry); y: NHWC.
 * act: 0 none, 1 SiLU, 2 GELU(erf); | 0x100: the row-run K layout of the init convs; | 0x200 (1x1 convs): the
 * upsample form, PixelShuffle(2) of the conv output, y is [B, 2 Ho, 2 Wo, Cout / 4]. */
int kd_conv2d_nhwc(const float* d_x, const float* d_w_oihw, const float* d_bias, float* d_y,
                   int B, int Hi, int Wi, int Cin, int Cout, int KH, int KW, int stride, int pad,
                   int act, void* stream);
/* nn.Upsample(scale_factor 2, nearest) followed by Conv2d(Cin, Cout, 3, padding 1) in one kernel (kernels_resample.hip): four
 * phase GEMMs with K = 4 Cin over the low-res map, the 3x3 taps that fall on one input pixel summed; the upsampled map is
 * never written.  x: NHWC [B,H,W,Cin] dense; w: torch OIHW [Cout,Cin,3,3] (packed into the sixteen summed tap matrices on
 * each call of this test entry); y: NHWC [B,2H,2W] rows of stride ldy (0 = Cout), the result in channels [yoff, yoff + Cout)
 * and nothing else touched.  Needs Cin % 8 == 0, Cout % 32 == 0, ldy % 4 == 0, yoff % 4 == 0. */
int kd_upsample_nearest_conv3x3_nhwc(const float* d_x, const float* d_w_oihw, const float* d_bias, float* d_y, int ldy, int yoff,
                                     int B, int H, int W, int Cin, int Cout, void* stream);
/* nn.Upsample(scale_factor s, nearest), s an integer >= 2, followed by [SiLU(A x + B)] and Conv2d(Cin, Cout, 3, padding 1) in
 * one kernel (kernels_upcombine.hip).  An output pixel is, by its row and its column inside the s x s block of its low-res
 * pixel, of one of 3 x 3 classes (first / interior / last); a class is a small conv over the low-res map with the 3x3 taps
 * that fall on one input pixel summed, so there are nine distinct values per (low-res pixel, output channel) from 25 summed
 * tap matrices, each stored to every pixel of its class.  s = 2 has the four corner classes only.  x: NHWC [B,H,W] rows of
 * stride ldx (0 = Cin); d_ab (may be NULL: x as it is): [B][Cin][2] per-(image, channel) affine in kd_gn_fold_seg's form
 * (times kd_wf_ab_scale()), applied with the SiLU as the patch is loaded - taps off the map are zero AFTER it; w: torch OIHW
 * [Cout,Cin,3,3] (packed on each call of this test entry); y: NHWC [B,sH,sW] rows of stride ldy (0 = Cout), the result in
 * channels [yoff, yoff + Cout) and nothing else touched.  Needs Cin % 8 == 0, Cout % 32 == 0, ldx, ldy, yoff % 4 == 0 and
 * fewer than 2^31 output pixels. */
int kd_upsample_nearest_gn_conv3x3_nhwc(const float* d_x, int ldx, const float* d_ab, const float* d_w_oihw, const float* d_bias,
                                        float* d_y, int ldy, int yoff, int B, int H, int W, int Cin, int Cout, int scale,
                                        void* stream);
/* The same 3x3 / stride-1 / pad-1 convolution through the plan's Winograd F(2x2,3x3) path (used for
 * the deep ResnetBlock convs): fp32, differs from kd_conv2d_nhwc by re-association
 * only.  Needs even H, W; B*H*W/4 % 256 == 0; Cin % 32 == 0; Cout > 32. */
int kd_conv3x3_winograd_nhwc(const float* d_x, const float* d_w_oihw, const float* d_bias, float* d_y,
                             int B, int H, int W, int Cin, int Cout, void* stream);
/* The same convolution (+ optional residual d_res, NHWC with Cout channels) through the plan's Winograd F(4x4,3x3)
 * path for the deepest layers (kernels_wino4.hip): weight transform, input transform, 36 batched GEMMs, output transform.
 * Needs H % 4 == 0, W % 4 == 0, B (H/4) (W/4) % 128 == 0, Cin % 32 == 0, Cout % 64 == 0.  d_out_stats (may be NULL):
 * [B, G, 2] = (mean, rstd) of y per image and group of Cout / G channels from the partial sums the output transform
 * leaves for the next GroupNorm; needs (Cout / G) % 16 == 0.  gemm_bf16x3 = 1: the GEMMs on the bf16 matrix pipe as the
 * plan runs them by default (V in plane form), 2: V as fp32, split by the GEMM's loader waves (kd_unet_config_t::gemm_bf16x3;
 * both need B (H/4) (W/4) % 256 == 0 and Cout % 128 == 0 as well). */
int kd_conv3x3_winograd4_nhwc(const float* d_x, const float* d_w_oihw, const float* d_bias, const float* d_res,
                              float* d_y, int B, int H, int W, int Cin, int Cout, int G, float eps,
                              float* d_out_stats, int gemm_bf16x3, void* stream);
/* C[g][M][N] = A[g][M][K] B[g][N][K]^T (fp32, row-major) through the bf16x3 GEMM of kernels_gemm_bf16x3.hip: both
 * operands split into three bf16 planes, six bf16 MFMAs per k-step, fp32 accumulation.  a_planes != 0: both operands
 * split beforehand (the plan's form: weights once, activations by the kernel that writes them); a_planes = 0: A stays fp32
 * and is split by the kernel's loader waves on its way into LDS.  Same planes, same bits.  Needs M % 256 == 0, N % 128 == 0, K % 32 == 0, 6 G M K and 6 G N K below 2^32 bytes. */
int kd_gemm_bf16x3(const float* d_a, const float* d_b, float* d_c, int G, int M, int N, int K, int a_planes, void* stream);
/* The token-GEMM / 1x1-conv form of the same kernel, as the plan runs the attention projections, the feed-forward and
 * the skip convs with K >= 512 (kd_unet_config_t::x3_linear): y[m][n] = sum_k x[m][k] w[n][k] + bias[n]
 * (+ gate_src[m][n] gate[m / hw][n]) (+ res[m][n]), fp32 rows with strides ldx / ldres / ldgs / ldy (0 = dense), the
 * activations split into their three bf16 pieces by the kernel's loader waves, the weights once.  Optional pointers may
 * be NULL.  d_seg (optional): the (sum, sum of squares) partials of y the launch leaves for a GroupNorm that reads it,
 * fp64 [M / hw][N / 16][hw / rows][2] with rows = kd_linear_bf16x3_seg_rows(M, N, K) (32, or 8 where the tiles are cut in
 * k).  act (0 none, 1 SiLU, 2 GELU, 3 sigmoid) is applied to the product + bias.  pixshuf_wo > 0: the Upsample form
 * (conv1x1 -> SiLU -> PixelShuffle(2)): the rows are the pixels of maps of width pixshuf_wo, d_w's rows are packed
 * n' = (2 i + j) N/4 + c, y is the [4 M][ldy] map of N / 4 channels and the statistics chunks are 4 per 32 input pixels
 * (one per sub-position).  Replaces nn.Linear / 1x1 nn.Conv2d + the residual / GlobalContext-gate adds around them and
 * Upsample's conv + activation + rearrange. */
int kd_linear_bf16x3(const float* d_x, int ldx, const float* d_w, const float* d_bias, const float* d_res, int ldres,
                     const float* d_gate_src, int ldgs, const float* d_gate, int hw, float* d_y, int ldy, int M, int N, int K,
                     int act, int pixshuf_wo, double* d_seg, void* stream);
int kd_linear_bf16x3_seg_rows(int M, int N, int K);
/* The library's Downsample (Rearrange 'b c (h s1) (w s2) -> b (c s1 s2) h w' + Conv2d(4 C, O, 1): a 2 x 2 / stride-2 conv,
 * SURVEY A.1) on the same kernel: x NHWC [B][H][W][ldx] (C channels used), d_w the torch weight [O][4 C], y NHWC
 * [B][H/2][W/2][O]; the kernel's loader waves gather the four input pixels of an output pixel.  d_seg as above with
 * hw = (H/2) (W/2) and rows = kd_linear_bf16x3_seg_rows(B hw, O, 4 C). */
int kd_downsample_bf16x3(const float* d_x, int ldx, const float* d_w, const float* d_bias, float* d_y, int B, int H, int W, int C,
                         int O, double* d_seg, void* stream);
/* ResnetBlock `Block` in one pass over x: conv3x3(SiLU(FiLM(GroupNorm_G(x)))) + bias (+ d_res), the form the
 * plan uses for those layers: statistics, a per-(image, channel) affine fold, and the fused Winograd kernel
 * with the activation applied to the raw patch in LDS (the activated map is never written).  d_scale_shift
 * ([B, 2 Cin] = [scale | shift]) and d_res (NHWC, Cout channels) may be NULL.  Needs H % 16 == 0, W % 16 == 0, Cin % 4 == 0,
 * Cout % 64 == 0 (non-zero return otherwise), Cin <= 2048, Cin % G == 0, (Cin / G) % 4 == 0, 16-byte aligned d_y / d_bias / d_res.  Runs the kernel the plan would
 * pick for the shape: items of 16 x 8 pixels x 128 output channels where Cout % 128 == 0
 * (kernels_wino_fused128.hip), 16 x 16 pixels x 64 channels otherwise (kernels_wino_fused.hip). */
int kd_gn_conv3x3_winograd_fused_nhwc(const float* d_x, const float* d_gamma, const float* d_beta,
                                      const float* d_scale_shift, const float* d_w_oihw,
                                      const float* d_bias, const float* d_res, float* d_y, int B, int H,
                                      int W, int Cin, int Cout, int G, float eps, float* d_out_stats,
                                      int ldx, void* stream);

/* The pieces a ResnetBlock of the plan is joined from, each through the plan's own launches with the plan's argument forms
 * (engine.hip), so that tests can hold every one against a reference by itself.  All synchronise before returning. */
/* y[m][:N] (row stride ldy) = act(W f(x[m][:K]) + bias) for the small-M linears (time MLPs, GlobalContext FCs, time-token
 * projections): x rows of stride ldx, w torch [N][K], bias may be NULL; in_act f / act: 0 none, 1 SiLU, 2 GELU, 3 sigmoid.
 * The plan's dispatch picks the kernel: VALU where K % 4, ldx % 4 or the alignment of x / w rule out 16-byte loads, else
 * a GEMV for M = 1 (K <= 16384), else the MFMA kernel with K split over four waves from K >= 512, one wave below. */
int kd_linear_skinny(const float* d_x, int ldx, const float* d_w, const float* d_bias, float* d_y, int ldy, int M, int K,
                     int N, int in_act, int act, void* stream);
/* GlobalContext gate of x NHWC [B][HW][C]: gate [B][C] = sigmoid(W2 SiLU(W0 pooled + b0) + b2) with pooled[b] =
 * sum_p softmax_p(x[b][p] . wk + bk) x[b][p]; wk [C], bk [1], W0 [hid][C], W2 [C][hid] (torch layouts).  path 0: the
 * plan's choice (fused where C <= 512, hid <= 256 and B > 1), 1: pooling + two kd_linear_skinny launches, 2: the fused
 * gate (refused where it does not apply).  d_pooled (may be NULL; not with the fused gate): [B][C], the pooled vector of
 * path 1.  Needs C % 4 == 0, C <= 2048. */
int kd_global_context_gate(const float* d_x, int B, int HW, int C, const float* d_wk, const float* d_bk, const float* d_w0,
                           const float* d_b0, int hid, const float* d_w2, const float* d_b2, float* d_gate, float* d_pooled,
                           int path, void* stream);
/* y = a * gate[b][c] + r, NHWC [B][HW]: a dense C channels, r / y rows of stride ldr / ldy (0 = C; channel slices of
 * wider maps), d_gate [B][C] or NULL (1).  d_seg (may be NULL, C % 16 == 0): the GroupNorm partials of y the plan leaves
 * for the next layer, fp64 [B][C / 16][kd_gate_add_chunks(B, HW)][2] = (sum, sum of squares) per pixel chunk.  Needs
 * C % 4 == 0, strides multiples of 4 and 16-byte aligned pointers. */
int kd_gate_add_nhwc(const float* d_a, const float* d_gate, const float* d_r, int ldr, float* d_y, int ldy, double* d_seg,
                     int B, int HW, int C, void* stream);
int kd_gate_add_chunks(int B, int HW);
/* The launch shape of an fp32 convolution / token GEMM (ConvShape, csrc/common.h), as the plan builder and the test entry
 * points compute it once per launch.  A pure host function: it touches no device.  geom[22]: B, Hi, Wi, Cin, ldx, Ho, Wo,
 * Cout, KH, KW, stride, pad, rr_cin, act, ldres, ldgs, out_mode (0 NHWC, 1 PixelShuffle, 2 NCHW), ldy, yoff, wz_rows,
 * wz_count, seg_c0 - the fields of the launch's parameters that are no pointers.  has / al16: bits 1 y, 2 bias, 4 residual,
 * 8 gated map, 16 gate, 32 split-K scratch - which of them the launch gets (y always) and which are 16-byte aligned.  cus:
 * compute units of the device.  out[12]: 1 for the generic kernel / 0 for the buffer-load one, tile rows, tile columns,
 * waves along each, grid x, y, z, threads per workgroup, k-splits (1 = none), 16-byte epilogue, chunks per image of the
 * GroupNorm partials the launch can leave (0 = none).  Returns 1 (kd_last_error) where no kernel takes the shape. */
int kd_conv_launch_shape(const int* geom, unsigned has, unsigned al16, int cus, int* out);
/* Linear attention (dim_head 64), the kernels the plan runs, for unit tests.  kd_linattn_dwconv_nhwc: y = depthwise 3x3
 * (zero padding) of x, both [B][H][W][3 heads 64] (q | k | v), weights the library's to_{q,k,v}.2.weight [heads 64][1][3][3];
 * d_part [B][ceil(H W / kd_linattn_chunk_tokens())][heads 64][2] = (max, sum of exp(k - max)) of k per chunk of tokens.
 * kd_linattn_context: d_ctx [B][heads][64][64] = softmax_n(k)^T v over the HW tokens (k / v rows of stride ld, d_part as
 * the conv leaves it) then the null key / value [64] (or NULL) then m context tokens (d_ck / d_cv [B][m] rows of stride
 * ldc).  kd_linattn_apply: out[b][n][h 64 + e] = [SiLU](softmax_d(q) scale . ctx[b][h]). */
int kd_linattn_chunk_tokens(void);
int kd_linattn_dwconv_nhwc(const float* d_x, const float* d_wq, const float* d_wk, const float* d_wv, float* d_y,
                           float* d_part, int B, int H, int W, int heads, void* stream);
int kd_linattn_context(const float* d_k, const float* d_v, int ld, const float* d_part, int HW, const float* d_ck,
                       const float* d_cv, int ldc, int m, const float* d_null_k, const float* d_null_v, float* d_ctx, int B,
                       int heads, void* stream);
int kd_linattn_apply(const float* d_q, int ldq, const float* d_ctx, float* d_out, int ldo, int B, int N, int heads,
                     float scale, int silu, void* stream);
/* GroupNorm statistics from producers' fp64 segment partials [B][nseg][nchunk][2] (sum, sum of squares per 16-channel
 * segment and chunk of HW pixels), of up to two sources: source 0 covers channels [0, 16 nseg0), source 1 (d_seg1 may be
 * NULL) [16 nseg0, C); the GroupNorm sees scale_i * source i, and ab_mul_i goes into the affine's A for its channels (a
 * consumer that reads the source unscaled).  d_stats (may be NULL): [B][G][2] (mean, rstd).  d_ab (may be NULL): [B][C][2]
 * the folded affine (A, B) of GroupNorm (gamma, beta) and FiLM (d_scale_shift rows [scale(C) | shift(C)] of stride
 * ld_ss >= 2 C, may be NULL), times kd_wf_ab_scale() = -log2(e), the form the fused Winograd kernel takes.  Needs
 * (C / G) % 16 == 0. */
int kd_gn_fold_seg(const double* d_seg0, int nseg0, int nchunk0, float scale0, float ab_mul0, const double* d_seg1, int nseg1,
                   int nchunk1, float scale1, float ab_mul1, const float* d_gamma, const float* d_beta,
                   const float* d_scale_shift, int ld_ss, float* d_ab, float* d_stats, int B, int HW, int C, int G, float eps,
                   void* stream);
float kd_wf_ab_scale(void);
/* One F(4x4,3x3) ResnetBlock conv as the plan runs it (engine.hip wino4_block): y [B][H][W][Cout] = conv3x3(SiLU(FiLM(
 * GroupNorm_G(x')))) + bias (+ res), x' = x with channels [skip_c0, Cin) times skip_scale (skip_c0 < 0: none) - x itself
 * is read unscaled, the factor goes into the affine.  x rows of stride ldx (0 = Cin), d_stats [B][G][2] (mean, rstd) of x'
 * (kd_gn_fold_seg), d_scale_shift (may be NULL) FiLM rows of stride ld_ss, d_res (may be NULL) rows of stride ldres
 * (0 = Cout).  d_out_seg (may be NULL): the partials of y the plan leaves for the next GroupNorm, fp64
 * [B][Cout / 16][(H/4) (W/4)][2], one chunk per 4 x 4 tile.  gemm_mode: -1 the 36 position GEMMs on fp32 MFMA, 1 bf16x3 with
 * V as planes, 2 bf16x3 with V as fp32.  The batch runs in sets of images_per_set images (0 = B), one set of launches after
 * the other.  Needs H % 4 == 0, W % 4 == 0, images_per_set (H/4) (W/4) % 128 == 0 (% 256 and Cout % 128 == 0 for
 * bf16x3), Cin % 32 == 0, Cout % 64 == 0. */
int kd_gn_conv3x3_winograd4_nhwc(const float* d_x, int ldx, const float* d_stats, const float* d_gamma, const float* d_beta,
                                 const float* d_scale_shift, int ld_ss, int skip_c0, float skip_scale, const float* d_w_oihw,
                                 const float* d_bias, const float* d_res, int ldres, float* d_y, double* d_out_seg, int B,
                                 int H, int W, int Cin, int Cout, int G, int gemm_mode, int images_per_set, void* stream);

/* (ldx: row stride of d_x in floats, >= Cin and a multiple of 4, 0 = dense: the plan hands this kernel channel-slice
 * views of wider buffers - a skip tensor living in the concat it will join.) */
/* (d_out_stats, may be NULL: [B, G, 2] = (mean, rstd) of y per image and group of Cout / G channels, reduced
 * from the partial sums the kernel's epilogue leaves for the GroupNorm of the next layer; needs
 * (Cout / G) % 16 == 0.) */
/* The UNet's initial cross-embed convolution (three stride-1 convs k = 3 / 7 / 15) over a 3-plane NCHW
 * image in the plan's one-kernel form: y NHWC [B][S][S][n3+n7+n15] = cat(conv3, conv7, conv15)(x) + bias.
 * d_w3 / d_w7 / d_w15: OIHW [n][3][k][k].  Needs S % 32 == 0, n3 <= 64, n7 <= 32, n15 <= 32, each a multiple of 4. */
int kd_init_conv_nchw(const float* d_x, const float* d_w3, const float* d_w7, const float* d_w15,
                      const float* d_bias, float* d_y, int B, int S, int n3, int n7, int n15, void* stream);
/* Same kernel over the per-step planes of any init conv: d_w*: OIHW [n][Itot][k][k], of which input channels c0 .. c0 + 2
 * are x's planes, and with d_self_cond != NULL c0 + 3 .. c0 + 5 its planes (the 6-plane form of self-conditioned UNets).
 * y = conv(planes) + (d_bias | d_res: dense NHWC [B][S][S][n3+n7+n15], may be NULL).  Runs `iters` times; ms != NULL:
 * the device time of one run (ms), averaged over the iters. */
int kd_init_conv_planes_nchw(const float* d_x, const float* d_self_cond, const float* d_w3, const float* d_w7,
                             const float* d_w15, int Itot, int c0, const float* d_bias, const float* d_res, float* d_y, int B,
                             int S, int n3, int n7, int n15, int iters, float* ms, void* stream);
/* The same for images of `channels` = 1 .. 4 planes (kd_init_conv_planes_nchw == this with channels = 3): d_x and
 * d_self_cond are [B][channels][S][S], the per-step planes input channels c0 .. c0 + channels - 1 (x) and, with
 * d_self_cond != NULL, the `channels` after them.  Fails where the kernel's 160 KB of LDS do not hold the shape (8 planes
 * at n3 = 64: the plan runs its generic three-conv path there). */
int kd_init_conv_planes_c_nchw(const float* d_x, const float* d_self_cond, const float* d_w3, const float* d_w7,
                               const float* d_w15, int Itot, int c0, const float* d_bias, const float* d_res, float* d_y, int B,
                               int S, int n3, int n7, int n15, int iters, float* ms, int channels, void* stream);
/* The UNet's final 3x3 conv to the image's `channels` = 1 .. 4 planes through the plan's launches (kernels_final.hip):
 * out NCHW [B][channels][H][W] = conv3x3(cat(feat, lowres)) + bias with d_feat NHWC [B][H][W][Cfeat], d_w_oihw
 * [channels][Cfeat + Cl][3][3] (Cl = channels when d_lowres is given, else 0), d_lowres NCHW [B][channels][H][W] or
 * NULL.  Needs Cfeat % 4 == 0. */
int kd_final_conv_nchw(const float* d_feat, const float* d_w_oihw, const float* d_bias, const float* d_lowres, float* d_out,
                       int B, int H, int W, int Cfeat, int channels, void* stream);
/* The same for `Unet(final_conv_kernel_size=ksize)`, ksize = 1, 3, 5 or 7: d_w_oihw [channels][Cfeat + Cl][ksize][ksize],
 * zero padding ksize / 2.  ksize = 3 runs the launches of kd_final_conv_nchw (the same bits); the other sizes the 1x1 GEMM to
 * the (output, tap) columns and the k x k gather of kernels_final.hip. */
int kd_final_conv_k_nchw(const float* d_feat, const float* d_w_oihw, const float* d_bias, const float* d_lowres, float* d_out,
                         int B, int H, int W, int Cfeat, int channels, int ksize, void* stream);
/* The per-step share of a plain init conv (`Unet(init_cross_embed=False)`) in the plan's one-kernel form (kernels_init.hip):
 * y[b][py][px][0 .. n) (NHWC rows of stride ldy floats, first channel at d_y) = Conv2d(ksize, padding ksize / 2) of the
 * per-step planes + (d_bias [n] | d_res: dense NHWC [B][S][S][n], may both be NULL).  d_x, d_self_cond: [B][channels][S][S]
 * (d_self_cond NULL: x alone), d_w OIHW [n][Itot][ksize][ksize] of whose input channels c0 .. are the per-step planes.
 * d_seg != NULL: the GroupNorm partials of y, [B][n / 16][S * S / 32][2] doubles (sum, sum of squares per 16 channels and
 * run of 32 pixels; needs n % 16 == 0).  Fails - as the plan's predicate does, the plan then takes the generic conv - unless
 * ksize is 3, 5 or 7, S % 32 == 0, n % 4 == 0, n <= 128 and the weights fit the kernel's 160 KB of LDS. */
int kd_init_conv_plain_nchw(const float* d_x, const float* d_self_cond, const float* d_w, int Itot, int c0, const float* d_bias,
                            const float* d_res, float* d_y, int ldy, double* d_seg, int B, int S, int n, int ksize, int channels,
                            int iters, float* ms, void* stream);
/* GroupNorm(G) + optional FiLM (scale+1, shift: [B,2C] = [scale | shift]) + SiLU, NHWC. */
int kd_groupnorm_silu_nhwc(const float* d_x, const float* d_gamma, const float* d_beta,
                           const float* d_scale_shift, float* d_y, int B, int HW, int C, int G,
                           float eps, void* stream);
/* LayerNorm over the last dim of [rows, C]; beta may be NULL (gain-only). */
int kd_layernorm(const float* d_x, const float* d_g, const float* d_beta, float* d_y,
                 int rows, int C, float eps, void* stream);
/* The forms the TransformerBlock's plan uses: y = LN(f(x)) g (+ beta) (+ res) with f = in_act (0 none, 1 SiLU, 2 GELU:
 * FeedForward's Linear -> GELU -> LayerNorm when the GEMM stores the raw product), and, with d_g2 / d_y2 given, also
 * y2 = LN(y) g2 in the same pass (attention's to_out LayerNorm + residual followed by the feed-forward's first). */
int kd_layernorm_ex(const float* d_x, const float* d_g, const float* d_beta, const float* d_res, float* d_y, int rows, int C,
                    float eps, int in_act, const float* d_g2, float* d_y2, void* stream);
/* LayerNorm -> Linear as the TransformerBlock's plan runs them where the GEMM is a bf16x3 one: the LayerNorm leaves
 * y = LN(f(x)) g (+ beta) as the GEMM's three bf16 planes ([3][C / 16][rows][16] bf16 in d_planes, 6 rows C bytes; the
 * planes of a value add up to it exactly), the GEMM reads them with its DMA loaders: d_y [rows, N] (row stride ldy) =
 * y @ w[N, C]^T + bias + res.  rows % 256 == 0, N % 128 == 0, C % 32 == 0, C <= 4096.  Same products in the same order as
 * kd_layernorm_ex followed by kd_linear_bf16x3: bit-identical results. */
int kd_layernorm_linear_bf16x3(const float* d_x, const float* d_g, const float* d_beta, int rows, int C, float eps, int in_act,
                               const float* d_w, const float* d_bias, const float* d_res, int ldres, float* d_y, int ldy,
                               int N, void* d_planes, void* stream);
/* Attention with fp32 softmax.  q [B,Nq,H,D] (already scaled), k/v [B,Nk,Hkv,D] with
 * Hkv in {1,H}; out [B,Nq,H,D].  D must be 32, 64 or 128. */
int kd_attention(const float* d_q, const float* d_k, const float* d_v, float* d_out,
                 int B, int Nq, int Nk, int H, int Hkv, int D, void* stream);
/* The same core with every argument the plan's launches pass (engine.hip transformer() / cross_attn(), text_build.inc), a
 * straight pass-through for unit tests: out[b][i][h 64 + d] (row stride ldo) = softmax_j(scale q[b][i][h] . K[j]) V[j] over the
 * key list cat(null key, segment 0, segment 1).  q rows of stride ldq; d_null_kv [2][64] = (key, value) shared by all heads, or
 * NULL; segment s: k / v [B][n_s] rows of stride ld_s holding Hkv heads of 64 (Hkv = 1: one head shared by all H); a segment
 * with n = 0 may have NULL pointers.  Strides are multiples of 4, pointers 16-byte aligned.  Which of the two kernels runs is
 * the launch's own choice (matrix cores from Nq >= 128 and 16 blocks of 128 queries).  Synchronises before returning. */
int kd_attention_ex(const float* d_q, int ldq, const float* d_null_kv, const float* d_k0, const float* d_v0, int ld0, int n0,
                    const float* d_k1, const float* d_v1, int ld1, int n1, float* d_out, int ldo, int B, int Nq, int H, int Hkv,
                    float scale, void* stream);
/* kd_attention_ex for heads of D = 32, 64 or 128 floats (any other D is refused): every 64 above reads D, d_null_kv is [2][D].
 * kd_attention_ex is this call with D = 64. */
int kd_attention_ex_d(const float* d_q, int ldq, const float* d_null_kv, const float* d_k0, const float* d_v0, int ld0, int n0,
                      const float* d_k1, const float* d_v1, int ld1, int n1, float* d_out, int ldo, int B, int Nq, int H, int Hkv,
                      int D, float scale, void* stream);
/* Keys per LDS tile of the attention kernels' D-wide instantiations (64, 64 and 32 for D = 32, 64 and 128); 0 for any other D.
 * For tests that place keys around a tile's edges. */
int kd_attention_key_tile(int D);
/* The qk-norm of kd_unet_config_t::attn_qk_norm, in place: each of the `heads` 64-wide segments at the start of every row
 * (stride ld >= heads 64) becomes x / max(||x||, 1e-12) (* d_scale_vec [64], may be NULL); columns past the segments are
 * not touched.  Synchronises before returning. */
int kd_l2norm_heads(float* d_x, int ld, int64_t rows, int heads, const float* d_scale_vec, void* stream);
/* The same for segments of D = 32, 64 or 128 floats (d_scale_vec [D], ld >= heads D); kd_l2norm_heads is this call with D = 64. */
int kd_l2norm_heads_d(float* d_x, int ld, int64_t rows, int heads, int D, const float* d_scale_vec, void* stream);
/* The small kernels of the text-conditioning plan (text_build.inc) with the plan's argument forms, straight pass-throughs for
 * unit tests; each synchronises before returning.
 *   kd_text_select:    out [B][P][C]: row p = tok[b][p] where p < L, mask[b][p] != 0 and !drop, else null_embed[p].  tok [B][L][C]
 *                      (no rows past L), mask [B][L] floats, null_embed [P][C], 1 <= L <= P.  d_mask == NULL (text_mask = None):
 *                      every row p < L is kept and the rows p >= L are zero; drop still gives null_embed everywhere.
 *   kd_add_rows_bcast: y[b][r][:] = x[b][r][:] + add[r][:], x / y [B][R][C], add [R][C].
 *   kd_mean_rows:      y[b][:] = mean over r of x[b][r][:], x [B][R][C], y [B][C]; summed in row order in fp32.
 *   kd_copy_rows:      dst[b dst_bstride + r ld_dst + c] = src[b src_bstride + r ld_src + c] for b < B, r < rows, c < C
 *                      (strides in floats; src_bstride = 0 broadcasts one block of rows to every batch element). */
int kd_text_select(const float* d_tok, const float* d_mask, const float* d_null_embed, float* d_out, int B, int L, int P, int C,
                   int drop, void* stream);
int kd_add_rows_bcast(const float* d_x, const float* d_add, float* d_y, int B, int R, int C, void* stream);
int kd_mean_rows(const float* d_x, float* d_y, int B, int R, int C, void* stream);
int kd_copy_rows(const float* d_src, int64_t src_bstride, int ld_src, float* d_dst, int64_t dst_bstride, int ld_dst, int rows,
                 int C, int B, void* stream);
/* Per-sample linear-interpolated quantile of |x| over n values (torch.quantile semantics). */
int kd_quantile_abs(const float* d_x, float* d_out, int B, int64_t n, float q, void* d_workspace,
                    size_t workspace_bytes, void* stream);
size_t kd_quantile_workspace_bytes(int B);
/* Standard-normal Philox4x32-10 fill (the generator kd_sample_loop uses when no noise tensors
 * are given): element i of stream `stream_id` under `seed`. */
int kd_philox_normal(float* d_out, int64_t n, uint64_t seed, uint64_t stream_id, void* stream);
/* The per-image form: row b of d_out [B][n] is what kd_philox_normal writes for (n, seeds[b], stream_id), bit for bit.
 * `seeds` is a HOST pointer to B keys, read before the call returns.  Needs n % 4 == 0, n >= 4 and a 16-byte aligned
 * d_out (refused with an error, nothing launched, otherwise). */
int kd_philox_normal_rows(float* d_out, int B, int64_t n, const uint64_t* seeds, uint64_t stream_id, void* stream);
/* The start of a stage (x_T) in one launch: d_x[b,c,y,x] = scale * z[b,c,y,x] + (2 * d_init[b,c,sy,sx] - 1), d_x [B,C,S,S].
 *   z      N(0,1) of Philox stream (16 << 32) | 2, the x_T draw: under `seed` with the counter over the whole batch tensor
 *          (seeds == NULL: the bits of kd_philox_normal over B C S S elements), under the HOST array `seeds` of B keys with
 *          the counter inside the image (the bits of kd_philox_normal_rows; read before the call returns), or, when
 *          d_noise [B,C,S,S] is given, read from it (seed and seeds are then not used).
 *   scale  1 for the DDPM sampler, sigma_0 for the EDM sampler; scale = 1 gives z's bits.
 *   d_init [B,C,Hs,Ws] in [0,1], or NULL: the image term is left out.  The source pixel is torch's
 *          F.interpolate(mode="nearest"): sy = min((int)floorf((float)y * ((float)Hs / (float)S)), Hs - 1), sx likewise
 *          with Ws; Hs = Ws = S is the identity.  Hs, Ws need not be equal nor multiples of anything.
 * The arithmetic keeps torch's op order without contraction: 2 v, - 1, scale z, the sum.  Needs C S S % 4 == 0 and 16-byte
 * aligned d_x / d_noise (refused with an error, nothing launched, otherwise).  sample() of the Python package starts
 * every stage through this call; init_images / skip_steps then continue with kd_sample_steps / kd_edm_sample_steps from
 * k_begin = skip_steps. */
int kd_sample_start(float* d_x, int B, int C, int S, float scale, uint64_t seed, const uint64_t* seeds, const float* d_noise,
                    const float* d_init, int Hs, int Ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused-tile canvas sampling (an engine extension; MultiDiffusion / Mixture of Diffusers).  An alternative to the
 * reference's sequential outpainting (outpainting.py:146-157, sample_ultra_res.py:183-195): the canvas of a stage is one
 * noisy image d_x [C,Hc,Wc]; at every schedule step every tile of an ny x nx lattice - tile size S, stride st,
 * Hc = (ny - 1) st + S, Wc = (nx - 1) st + S - is denoised by itself (kd_solver_sample_steps(k, k + 1) on gathered tiles,
 * its x0 estimate and thresholds read with kd_sample_last), and one call of kd_tiles_fuse_update averages the thresholded
 * estimates where tiles overlap and runs the solver update on the canvas.  S and st are multiples of 4, so every tile
 * origin and Wc are: all accesses are 16-byte loads and stores.  The Python package: Imagen.sample_tiled.
 * ---------------------------------------------------------------------------------------- */
/* d_tiles[b] = d_canvas[:, y0_b : y0_b + S, x0_b : x0_b + S] for b < B; d_canvas [C,Hc,Wc], d_tiles [B,C,S,S].
 * `origins_yx` is a HOST array [B][2] of (y0, x0), read before the call returns (the origins travel as kernel arguments);
 * origins may repeat and come in any order.  Needs S % 4 == 0, Wc % 4 == 0, every x0 % 4 == 0, every tile inside the
 * canvas and 16-byte aligned pointers (refused with an error, nothing launched, otherwise). */
int kd_tiles_gather(const float* d_canvas, float* d_tiles, int B, int C, int Hc, int Wc, int S, const int* origins_yx,
                    void* stream);
/* The canvas step in one pass, in place on d_x and d_x0bar [C,Hc,Wc].  Per pixel, over the present tiles t that cover it
 * in ascending (row, column) order of their slots:
 *     x0c_t = clamp(x0_t, -s_t, s_t) / s_t,  s_t = max(d_thr[t], 1)  (d_thr == NULL: s_t = 1, the static threshold)
 *     x0bar = (sum w_t x0c_t) / (sum w_t)
 *     x <- A x + B x0bar [+ P hist] [+ Sn z];  hist <- x0bar          (hist: what d_x0bar held on entry)
 * without contraction, the expression and op order of the solver step (kd_solver_sample_steps).  A term whose coefficient
 * is 0 is left out and its operand is not read: P == 0 leaves d_x0bar unread, Sn == 0 draws nothing.  A pixel that no
 * present tile covers is left untouched in both buffers.
 *   d_x0_tiles [N,C,S,S]  the x0 estimates BEFORE the threshold (kd_sample_last which = 1), d_thr [N] (which = 2)
 *   d_tile_of  [ny][nx]   tile index of the slot, or -1: no tile there (entries outside 0 .. N - 1 count as -1)
 *   ramp       0: w = 1.  != 0: w(y, x) = r(y) r(x), r(i) = min(i + 1, S - i, ov) / ov, ov = max(S - st, 1), inside the tile
 *   z          d_noise [C,Hc,Wc], or, when it is NULL, element (c Hc + y) Wc + x of Philox stream `stream_id` under `seed`:
 *              the bits kd_philox_normal writes over C Hc Wc elements - a property of the canvas, not of the tiling.
 * Needs S % 4 == 0, st % 4 == 0, 4 <= st <= S <= 3 st (at most 3 tiles per axis, 9 in all, cover a pixel), 1 <= N <= ny nx
 * and 16-byte aligned pointers (refused with an error, nothing launched, otherwise).
 * kd_tiles_fuse_update == kd_tiles_fuse_update_known with d_hist = d_x0bar_out = d_x0bar, renoise = 0 and known = mask = NULL. */
int kd_tiles_fuse_update(float* d_x, float* d_x0bar, const float* d_x0_tiles, const float* d_thr, const int* d_tile_of, int N,
                         int C, int S, int st, int ny, int nx, int ramp, float A, float B, float P, float Sn,
                         const float* d_noise, uint64_t seed, uint64_t stream_id, void* stream);

/* A stage at the sizes of a magnification level (the mag-2 canvas is 3 x 40960 x 40960): three memory-bound kernels that
 * stream what would otherwise be materialised per tile or per canvas.  The Python package: Imagen.sample_tiled(streamed=,
 * cond_crops=, into=), ultra_res.tiled.fused_level. */
/* The conditioning tiles of a chunk straight from the level above: d_src [Cs,W,W] -> d_tiles [B,Cs,S,S], or [B,2 Cs,S,S]
 * when d_centre_of is given.  Per axis, for output coordinate p of a tile with shift sh (`shifts_yx`: a HOST array [B][2]
 * of (sy, sx), read before the call returns): w = map[p] is a coordinate of the window that starts at `top`, g = top + w;
 * the coordinate is filled when sh > 0 ? g < sh : g >= (W + sh) % W (sh == 0 fills everything: the reference's `[shift:]`
 * slice), else it reads source index (g - sh) mod W.  A pixel is `fill` if either axis is filled, else d_src[c, ry, rx].
 * Channels c < Cs go through d_win_of [S], channels Cs + c (the `v2` centre crop) through d_centre_of [S]; both maps are
 * DEVICE arrays (imagen_pytorch.cond_crop_maps builds them) with entries in [0, W - top) - an entry outside is clamped
 * into that range, so nothing is read outside d_src.  Data movement only: bit-equal to
 * resize_image_to(cond_images_for_grid(...), S) where W >= window.  Needs S % 4 == 0, |sh| < W, 0 <= top < W and a 16-byte
 * aligned d_tiles (refused with an error, nothing launched, otherwise). */
int kd_tiles_cond_gather(const float* d_src, int Cs, int W, float* d_tiles, int B, int S, const int* shifts_yx, int top,
                         const int* d_win_of, const int* d_centre_of, float fill, void* stream);
/* The low-res conditioning tiles of a chunk straight from the previous stage's canvas d_prev [C,Hp,Wp]:
 *     d_tiles[b,c,y,x] = a (2 d_prev[c,iy,ix] - 1) + s z[(c Hc + y0_b + y) Wc + x0_b + x]
 * iy = min((int)floorf((float)(y0_b + y) * ((float)Hp / (float)Hc)), Hp - 1), ix likewise (kd_sample_start's rule, torch's
 * nearest); op order 2 v, - 1, a *, s z, the sum.  z is read from d_noise [C,Hc,Wc] or, when it is NULL, is the element
 * of Philox stream `stream_id` under `seed` - the bits of kd_philox_normal over C Hc Wc elements: overlapping tiles see
 * one conditioning on shared pixels and no canvas-sized buffer exists.  s == 0 leaves the term out, operand unread.
 * `origins_yx` and the preconditions are kd_tiles_gather's. */
int kd_tiles_gather_lowres(const float* d_prev, int Hp, int Wp, float* d_tiles, int B, int C, int Hc, int Wc, int S,
                           const int* origins_yx, float a, float s, const float* d_noise, uint64_t seed, uint64_t stream_id,
                           void* stream);
/* The end of a stage: for every pixel of the canvas d_x [C,Hc,Wc] covered by a present tile (kd_tiles_fuse_update's cover
 * test over d_tile_of [ny][nx]), d_out[c, oy + y, ox + x] = (clamp(x, -1, 1) + 1) * 0.5; every other element of d_out
 * [C,Ho,Wo] is left untouched.  Needs the lattice preconditions of kd_tiles_fuse_update, ox % 4 == 0, Wo % 4 == 0, the
 * canvas inside d_out and 16-byte aligned pointers (refused with an error, nothing launched, otherwise).
 * kd_tiles_finalize == kd_tiles_finalize_known with known = mask = NULL. */
int kd_tiles_finalize(const float* d_x, const int* d_tile_of, int N, int C, int S, int st, int ny, int nx, float* d_out, int Ho,
                      int Wo, int oy, int ox, void* stream);

/* A canvas that keeps known pixels (RePaint mixing at the level of the canvas) or starts from an image: three
 * memory-bound kernels in the conventions of the ones above.  The Python package: Imagen.sample_tiled(known_image=,
 * known_mask=, known_resample_times=, init_canvas=, init_skip_steps=), ultra_res.tiled.fused_level(canvas=, keep=).
 * A source - the known image, the init image, the mask - is described, not copied: base, size and strides in ELEMENTS, so a
 * window of a larger canvas is passed as it lies.  It is seen at the canvas' size [Hc, Wc] through torch's nearest rule as
 * kd_sample_start states it, sy = min((int)floorf((float)y * ((float)H / (float)Hc)), H - 1).  Where H == Hc, W == Wc, the
 * strides are multiples of 4 and the base is aligned (16 bytes the image, 4 the mask) a thread's four x are one load;
 * otherwise they are gathered one by one.  row_stride >= W and plane_stride >= 0 are required; that base and strides stay
 * inside the caller's allocation is the caller's to see to. */
typedef struct kd_tiles_image {   /* [C, H, W] fp32 */
  const float* d;
  int H, W;
  int64_t row_stride, plane_stride;
} kd_tiles_image_t;
typedef struct kd_tiles_mask {   /* [H, W] uint8, non-zero = known */
  const unsigned char* d;
  int H, W;
  int64_t row_stride;
} kd_tiles_mask_t;
/* The mix of one resample slot, x = m ? a (2 kn - 1) + s z : x, with a, s = alpha, sigma of the slot's step; op order 2 v,
 * - 1, a *, s z, the sum, without contraction; s == 0 leaves the term out, operand unread.  z is read from d_mix_noise
 * [C,Hc,Wc] or, when it is NULL, is the canvas element of Philox stream mix_stream_id under `seed`; a float4 whose four
 * mask bytes are clear draws none.  `known` and `mask` come together; both NULL: no mix. */
/* x of a stage in one launch over a rectangular canvas d_x [C,Hc,Wc] (kd_sample_start is square and per batch row):
 *     x = scale z [+ (2 nearest(init) - 1)],  then [the mix]
 * z is read from d_noise or is the canvas element of Philox stream (16 << 32) | 2 under `seed`; with init, known and mask
 * NULL and scale 1 the bits of kd_philox_normal over C Hc Wc elements.  Needs Wc % 4 == 0 and 16-byte aligned d_x and
 * noise tensors (refused with an error, nothing launched, otherwise). */
int kd_tiles_start(float* d_x, int C, int Hc, int Wc, float scale, const float* d_noise, uint64_t seed,
                   const kd_tiles_image_t* init, const kd_tiles_image_t* known, const kd_tiles_mask_t* mask, float mix_a,
                   float mix_s, const float* d_mix_noise, uint64_t mix_stream_id, void* stream);
/* kd_tiles_fuse_update and, on the same pixel in the same pass, [the re-noise x = x rn_a + z rn_b] (renoise != 0; z from
 * d_rn_noise or Philox stream rn_stream_id) then [the mix of the NEXT slot]: a step with known pixels stays one canvas pass.
 * Bit for bit kd_tiles_fuse_update followed by the two expressions; with renoise == 0 and no mask, kd_tiles_fuse_update's
 * bits.  d_hist (read only when P != 0) and d_x0bar_out are given apart and may be one buffer (kd_tiles_fuse_update's in-place
 * form); DPM-Solver++(2M) under resampling keeps them apart, the history taking a step's estimate in its last slot only.
 * A zero coefficient leaves its operand unread.  A float4 whose four mask bytes are all set is known after the mix
 * whatever the update gives: d_x is not read and the update draws nothing there; d_x0bar_out is written all the same.  A
 * pixel that no present tile covers is left untouched in every buffer.  Preconditions: kd_tiles_fuse_update's, d_x apart
 * from d_hist and d_x0bar_out. */
int kd_tiles_fuse_update_known(float* d_x, const float* d_hist, float* d_x0bar_out, const float* d_x0_tiles, const float* d_thr,
                               const int* d_tile_of, int N, int C, int S, int st, int ny, int nx, int ramp, float A, float B,
                               float P, float Sn, const float* d_noise, uint64_t seed, uint64_t stream_id, int renoise,
                               float rn_a, float rn_b, const float* d_rn_noise, uint64_t rn_stream_id,
                               const kd_tiles_image_t* known, const kd_tiles_mask_t* mask, float mix_a, float mix_s,
                               const float* d_mix_noise, uint64_t mix_stream_id, void* stream);
/* kd_tiles_fuse_update_known with a second history (the third-order canvas step of DPM-Solver++(3M) and its SDE form):
 *     x <- A x + B x0bar [+ P hist] [+ P2 hist2] [+ Sn z]
 * left to right, d_hist2 read only when P2 != 0 (NULL is then allowed).  d_x0bar_out may be d_hist2, as it may be d_hist:
 * each thread reads its element before it writes it, so a caller keeps three canvases and rotates the pointers - the
 * estimate of step k overwrites that of step k - 2.  P2 == 0 is kd_tiles_fuse_update_known, bit for bit.  Preconditions:
 * kd_tiles_fuse_update_known's, d_x apart from d_hist2 too. */
int kd_tiles_fuse_update_hist2(float* d_x, const float* d_hist, float* d_x0bar_out, const float* d_x0_tiles, const float* d_thr,
                               const int* d_tile_of, int N, int C, int S, int st, int ny, int nx, int ramp, float A, float B,
                               float P, float Sn, const float* d_noise, uint64_t seed, uint64_t stream_id, int renoise,
                               float rn_a, float rn_b, const float* d_rn_noise, uint64_t rn_stream_id,
                               const kd_tiles_image_t* known, const kd_tiles_mask_t* mask, float mix_a, float mix_s,
                               const float* d_mix_noise, uint64_t mix_stream_id, const float* d_hist2, float P2, void* stream);
/* kd_tiles_finalize with the paste: d_out[c, oy + y, ox + x] = m ? kn : (clamp(x, -1, 1) + 1) * 0.5 on covered pixels,
 * every other element of d_out untouched.  A known pixel is the known image's value copied, not round-tripped through
 * 2 v - 1.  `known` may be the window of d_out that is written (base d_out + oy Wo + ox, size [Hc, Wc], strides Wo and
 * Ho Wo): every thread then reads and writes the same element.  A known image that overlaps d_out in any other way is
 * refused.  `known` and `mask` come together (one without the other is refused); both NULL: no paste, kd_tiles_finalize's
 * bits.  Preconditions: kd_tiles_finalize's. */
int kd_tiles_finalize_known(const float* d_x, const int* d_tile_of, int N, int C, int S, int st, int ny, int nx, float* d_out,
                            int Ho, int Wo, int oy, int ox, const kd_tiles_image_t* known, const kd_tiles_mask_t* mask,
                            void* stream);

/* A canvas cut into shards by lattice rows (Imagen.sample_tiled(devices=...)): every shard holds the whole canvas, steps
 * the band its own tiles cover and fuses it out of its own tiles' estimates and the overlap strips of its neighbours'
 * boundary tiles.  Two additions carry that; no entry above changed.
 *
 * kd_tiles_rows_copy moves row strips of tiles: for i < n, with (ts, td, row0, rows) = desc[i] (a host array [n][4], free
 * on return; 32 descriptors per launch travel as a kernel argument),
 *     dst tile td, rows <- src tile ts, rows          [C, rows, S] each, 16-byte loads and stores, no atomics
 * Either side is an array of tiles [tiles, C, H, S], H = src_rows / dst_rows: H == S is a tile store and the strip lies at
 * its rows row0 .. row0 + rows; H < S is a strip buffer and the strip lies at its top (rows <= H).  So one entry packs the
 * strips of a store into a contiguous buffer, unpacks such a buffer into a store's halo slots, and copies store to store.
 * d_thr_src / d_thr_dst (both or neither): d_thr_dst[td] = d_thr_src[ts], the tiles' dynamic thresholds.  Elements outside
 * the strips keep their bits.  Refused with an error, nothing launched: a NULL or misaligned (16 bytes) d_src / d_dst,
 * d_src == d_dst, S % 4 != 0, a tile index outside [0, tiles), rows outside [0, S] (row0 < 0, rows < 0, row0 + rows > S), a
 * strip taller than a strip buffer.  The caller sees to it that the two buffers do not overlap and that the destination
 * strips are disjoint: two descriptors of one call that name the same destination tile with rows in common (or, with
 * thresholds, the same destination tile at all) would race, the copy having no order among descriptors. */
int kd_tiles_rows_copy(const float* d_src, int src_tiles, int src_rows, float* d_dst, int dst_tiles, int dst_rows,
                       const float* d_thr_src, float* d_thr_dst, int n, int C, int S, const int* desc, void* stream);
/* kd_tiles_finalize_known over the canvas rows y_lo <= y < y_hi alone (0 <= y_lo < y_hi <= Hc): what a shard ends.  oy may
 * be negative when the output is a band that holds the rows written and not the ones above them: oy + y_lo >= 0 and
 * oy + y_hi <= Ho are required in the place of kd_tiles_finalize's 0 <= oy, oy + Hc <= Ho. */
int kd_tiles_finalize_rows(const float* d_x, const int* d_tile_of, int N, int C, int S, int st, int ny, int nx, float* d_out,
                           int Ho, int Wo, int oy, int ox, const kd_tiles_image_t* known, const kd_tiles_mask_t* mask, int y_lo,
                           int y_hi, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KD_ENGINE_H */
