/*
 * sd_engine.h -- C-ABI of the MI355X-native Stable Diffusion denoise engine (libsd_engine.so).
 *
 * The reference (GrafikXxxxxxxYyyyyyyyyyy/StableDiffusion) has no FFI / plugin layer of its own: its
 * hot path is two Python object slots, `SDModelWrapper.base` (UNet2DConditionModel) and
 * `SDModelWrapper.vae` (AutoencoderKL), filled at /root/reference/models/stable_diffusion.py:110-123
 * and called at /root/reference/pipelines/sd_unified_pipeline.py:475-482 (UNet forward) and
 * :523 (VAE decode), :1027-1032 (VAE encode).  The entry points below are what a ctypes binding
 * for those slots binds (INTEGRATION.md shows the stub); each one names the reference interface
 * it replaces.
 *
 * Conventions
 *   - plain C: opaque handles, plain pointers and sizes, int return codes (0 = ok); no torch types.
 *   - every tensor buffer is DEVICE memory owned by the caller; the library owns only its packed
 *     weights and a workspace arena sized on first use of a shape.
 *   - boundary tensors are NCHW fp16, contiguous -- the layout of the reference's tensors; the
 *     engine runs NHWC internally.
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued on it and never synchronise.
 *   - errors: non-zero code + thread-local message from sd_last_error(); the Python shim raises
 *     RuntimeError, matching the reference's plain-exception convention
 *     (sd_unified_pipeline.py:302-306).
 *   - single caller thread per handle (the reference's handler is synchronous, rp_handler.py:44-63).
 */
#ifndef SD_ENGINE_H
#define SD_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SD_OK 0
#define SD_ERR_INVALID 1   /* bad argument / unknown key / shape mismatch */
#define SD_ERR_STATE 2     /* call order violated (e.g. forward before finalize) */
#define SD_ERR_HIP 3       /* HIP runtime error */
#define SD_ERR_UNSUPPORTED 4

#define SD_DTYPE_F16 0
#define SD_DTYPE_F32 1

#define SD_MAX_BLOCKS 4

/* UNet2DConditionModel hyper-parameters; field meaning = diffusers config fields as derived at
 * /root/reference/scripts/convert_from_A1111.py:175-189.  block type 1 = CrossAttn*Block2D, 0 = plain. */
typedef struct sd_unet_config {
    int32_t in_channels;
    int32_t out_channels;
    int32_t num_blocks;
    int32_t block_out_channels[SD_MAX_BLOCKS];
    int32_t down_block_has_attn[SD_MAX_BLOCKS];
    int32_t up_block_has_attn[SD_MAX_BLOCKS];
    int32_t num_heads[SD_MAX_BLOCKS];              /* per down block; reversed for up blocks */
    int32_t transformer_layers[SD_MAX_BLOCKS];     /* per down block; reversed for up blocks */
    int32_t layers_per_block;
    int32_t cross_attention_dim;
    int32_t use_linear_projection;
    int32_t norm_num_groups;
    float   norm_eps;
    int32_t flip_sin_to_cos;
    float   freq_shift;
    int32_t addition_time_embed_dim;               /* 0 = no text_time conditioning (SD1.5) */
    int32_t projection_class_embeddings_input_dim; /* SDXL: 2816; SDXL refiner: 2560 */
    int32_t num_time_ids;                          /* columns of add_time_ids: 0 = 6 (SDXL base); the refiner has 5; 1..8 */
    int32_t time_cond_proj_dim;                    /* 0 = no time_embedding.cond_proj; LCM-distilled UNets: 256; <= 1024 */
} sd_unet_config;

/* AutoencoderKL hyper-parameters (convert_from_A1111.py:490-511). */
typedef struct sd_vae_config {
    int32_t in_channels;      /* 3 */
    int32_t out_channels;     /* 3 */
    int32_t latent_channels;  /* 4 */
    int32_t num_blocks;
    int32_t block_out_channels[SD_MAX_BLOCKS];
    int32_t layers_per_block;
    int32_t norm_num_groups;
} sd_vae_config;

/* CLIP text encoder hyper-parameters (transformers CLIPTextConfig; the reference loads
 * CLIPTextModel / CLIPTextModelWithProjection at models/stable_diffusion.py:124-152). */
typedef struct sd_clip_config {
    int32_t vocab_size;          /* 49408 */
    int32_t hidden_size;         /* 768 (CLIP-L) / 1280 (OpenCLIP bigG) */
    int32_t intermediate_size;   /* 3072 / 5120 */
    int32_t num_layers;          /* 12 / 32 */
    int32_t num_heads;           /* 12 / 20 */
    int32_t max_positions;       /* 77 */
    int32_t hidden_act;          /* 0 quick_gelu, 1 gelu (erf) */
    int32_t projection_dim;      /* 0: CLIPTextModel; > 0: CLIPTextModelWithProjection.text_projection */
    float layer_norm_eps;        /* 1e-5 */
} sd_clip_config;

/* CLIP vision tower hyper-parameters (transformers CLIPVisionConfig): the image encoder an IP-Adapter was trained
 * against. */
typedef struct sd_clip_vision_config {
    int32_t hidden_size;         /* 1024 (ViT-L/14) / 1280 (ViT-H/14) / 1664 (ViT-bigG/14); % 8, <= 2048 */
    int32_t intermediate_size;   /* 4096 / 5120 / 8192 */
    int32_t num_layers;          /* 24 / 32 / 48 */
    int32_t num_heads;           /* 16 / 16 / 16 */
    int32_t image_size;          /* 224; divisible by patch_size */
    int32_t patch_size;          /* 14 */
    int32_t hidden_act;          /* 0 quick_gelu, 1 gelu (erf) */
    int32_t projection_dim;      /* 768 / 1024 / 1280 */
    float layer_norm_eps;        /* 1e-5 */
} sd_clip_vision_config;

typedef struct sd_unet sd_unet;
typedef struct sd_vae sd_vae;
typedef struct sd_clip sd_clip;
typedef struct sd_clip_vision sd_clip_vision;
typedef struct sd_ip_adapter sd_ip_adapter;
typedef struct sd_controlnet sd_controlnet;
typedef struct sd_motion sd_motion;

/* -- library ------------------------------------------------------------------------------- */
const char* sd_last_error(void);
int sd_engine_version(void);
/* Name of the code object's ISA target ("gfx950"). */
const char* sd_engine_arch(void);

/* -- UNet: replaces the object in SDModelWrapper.base (stable_diffusion.py:117-123) ---------- */
int sd_unet_create(const sd_unet_config* cfg, sd_unet** out);
int sd_unet_destroy(sd_unet* u);
/* Number of weight tensors the model expects / name and rank+shape of the i-th one, in
 * diffusers state-dict naming (convert_from_A1111.py:240-485). */
int sd_unet_num_weights(const sd_unet* u);
int sd_unet_weight_info(const sd_unet* u, int index, const char** key, int64_t* shape4, int* ndim);
/* Hand one tensor over (host or device pointer, contiguous, PyTorch layout:
 * conv [Cout,Cin,KH,KW], linear [out,in], vectors [C]).  The library copies + repacks; the
 * caller's buffer can be freed on return.  Replaces state_dict loading done by
 * UNet2DConditionModel.from_pretrained (stable_diffusion.py:117-123). */
int sd_unet_set_weight(sd_unet* u, const char* diffusers_key, const void* data,
                       const int64_t* shape, int ndim, int dtype);
/* All weights present -> pre-pack (fused qkv, GEGLU interleave, time-emb projection stack). */
int sd_unet_finalize(sd_unet* u);
/* UNet2DConditionModel.forward as called at sd_unified_pipeline.py:475-482.
 *   sample     [B,Cin,H,W] f16      latent_model_input
 *   timesteps  [B] f32 (device)     `t` broadcast to the batch
 *   ehs        [B,L,D] f16          prompt_embeds
 *   add_text   [B,P] f16 or NULL    added_cond_kwargs["text_embeds"]  (SDXL, :430-433)
 *   add_time_ids [B,n] f32 or NULL  added_cond_kwargs["time_ids"]; n = num_time_ids (0 in the configuration: 6).
 *                                   The pooled width is P = projection_class_embeddings_input_dim - n * addition_time_embed_dim.
 * Every forward entry below (_ex, _tc, _cn, _cfg) and the graph replay's staging copy take add_time_ids as [B,n].
 *   out        [B,Cout,H,W] f16     noise_pred
 */
int sd_unet_forward(sd_unet* u, const void* sample, const float* timesteps, const void* ehs,
                    int ehs_len, const void* add_text, const float* add_time_ids, void* out,
                    int B, int H, int W, void* stream);
/* Replay the whole forward from a captured hipGraph (one per input shape; inputs / output staged
 * through engine-owned buffers, fenced against `stream` with events).  Host cost per forward drops
 * from ~480 kernel launches to one hipGraphLaunch; results are bitwise those of the eager path.
 * A handle holds one graph.  A call captures -- runs eagerly on the staged copies, then records -- when there is no
 * graph, when (B, H, W, ehs_len, timestep_cond present) differ from the captured call's, or when the workspace or the
 * staging buffer the graph's addresses point into has been reallocated since (a larger forward run with replay off or
 * under sd_prof_enable); every other call replays.  Going back to an earlier shape captures again. */
int sd_unet_use_graph(sd_unet* u, int enable);
/* Captures and replays (see sd_unet_use_graph) of this handle since its creation; either pointer may be NULL.  Calls
 * that do not reach the graph path (replay off, a refused call, a forward under sd_prof_enable) count as neither. */
int sd_unet_graph_stats(const sd_unet* u, int64_t* captures, int64_t* replays);
/* Text K/V reuse across the forwards of ONE denoise loop (sd_unified_pipeline.py:465-507 passes the same
 * prompt_embeds to every step): enable = 1 makes the next forward compute the stacked attn2.to_k / to_v
 * projections of encoder_hidden_states and later forwards with the same (pointer, batch, length) reuse
 * them.  Every call of this function -- with 1 or 0 -- invalidates what is cached: call it (again) whenever
 * the CONTENTS behind the pointer may have changed, i.e. at the start of each pipeline call.  Off by default.
 * Under graph replay (sd_unet_use_graph) nothing is cached, in a replay or in a capturing call: the forward reads staged
 * copies, whose address says nothing about the caller's tensor, so every call projects its own encoder_hidden_states. */
int sd_unet_text_kv_cache(sd_unet* u, int enable);
/* sd_unet_forward with IP-Adapter image prompts (sd_unified_pipeline.py:441-449, diffusers 0.27.2
 * added_cond_kwargs["image_embeds"]):
 *   image_embeds [B,n_img,D_img] f16 or NULL   image encoder embeddings, one row per image (CFG: negative half first)
 * With an adapter attached (sd_unet_set_ip_adapter) image_embeds is required and every cross-attention computes
 *   SDPA(q, K_text, V_text) + scale * SDPA(q, K_ip, V_ip)
 * in one launch per site; n_img * num_tokens <= 64 and ehs_len <= 160, graph replay (sd_unet_use_graph) is
 * rejected (SD_ERR_UNSUPPORTED).  The image K / V follow sd_unet_text_kv_cache: kept across the forwards of one loop
 * for one (pointer, B, n_img), invalidated by every sd_unet_text_kv_cache call.  Without an adapter, image_embeds
 * must be NULL and the call is sd_unet_forward.  With a Resampler adapter (sd_ip_adapter_create_ex) image_embeds means
 * [B,n_img,T_feat,D_emb] f16, the image encoder's penultimate hidden states; everything else holds as stated. */
int sd_unet_forward_ex(sd_unet* u, const void* sample, const float* timesteps, const void* ehs, int ehs_len,
                       const void* add_text, const float* add_time_ids, const void* image_embeds, int n_img, void* out,
                       int B, int H, int W, void* stream);
/* sd_unet_forward_ex of a guidance-embedded UNet (time_cond_proj_dim > 0: Latent Consistency Models; diffusers 0.27.2
 * UNet2DConditionModel.forward(timestep_cond=), TimestepEmbedding.cond_proj):
 *   timestep_cond [B,cond_dim] f32 (device) or NULL   the guidance-scale embedding; cond_dim = time_cond_proj_dim
 * The time embedding's input becomes sinusoid(t) + timestep_cond W_cond^T (no bias), formed by one launch
 * (sd_op_timestep_cond_embedding) in the place of the sinusoid's, so the forward has as many launches as the plain one.
 * NULL skips the projection, as diffusers does: the call is sd_unet_forward_ex.  SD_ERR_INVALID: a non-NULL
 * timestep_cond on a UNet without the projection, cond_dim != time_cond_proj_dim.  An attached IP-Adapter works as in
 * sd_unet_forward_ex; an attached ControlNet is SD_ERR_UNSUPPORTED (diffusers' ControlNetModel has no such projection
 * and no guidance-embedded checkpoint ships one).  FreeU holds as for the other entries.  Graph replay
 * (sd_unet_use_graph) is supported: timestep_cond is staged like timesteps, its presence is part of the graph's shape
 * key, and replay is bitwise the eager result. */
int sd_unet_forward_tc(sd_unet* u, const void* sample, const float* timesteps, const void* ehs, int ehs_len,
                       const void* add_text, const float* add_time_ids, const void* image_embeds, int n_img,
                       const float* timestep_cond, int cond_dim, void* out, int B, int H, int W, void* stream);
/* Attach an IP-Adapter created for this UNet's configuration (NULL detaches: the forward is again exactly the plain
 * one).  One adapter per UNet; attaching it to another UNet detaches it from the first.  The scale (lambda of
 * set_ip_adapter_scale, default 1.0) belongs to the UNet; 0 computes the text attention alone. */
int sd_unet_set_ip_adapter(sd_unet* u, sd_ip_adapter* adapter);
int sd_unet_set_ip_adapter_scale(sd_unet* u, float scale);
/* Attach a ControlNet created for this UNet (sd_controlnet_create; NULL detaches: the forward is again exactly the
 * plain one).  One ControlNet per UNet; attaching it to another UNet detaches it from the first. */
int sd_unet_set_controlnet(sd_unet* u, sd_controlnet* cn);
/* MultiControlNet (diffusers 0.27.2 MultiControlNetModel): attach `count` <= SD_MAX_CONTROLNETS ControlNets, each created
 * for this UNet and finalized, none twice (SD_ERR_INVALID / SD_ERR_STATE, nothing changed); count == 0 detaches all.  The
 * list replaces whatever was attached, and sd_unet_set_controlnet replaces a list by its one net (or none); a net attached
 * to another UNet is detached there.  Everything that rejects an attached ControlNet rejects a list the same way. */
#define SD_MAX_CONTROLNETS 4
int sd_unet_set_controlnets(sd_unet* u, sd_controlnet* const* cns, int count);
/* sd_unet_forward_ex with ControlNet conditioning (diffusers 0.27.2 ControlNetModel feeding
 * down_block_additional_residuals / mid_block_additional_residual):
 *   control_image [n_ctrl,3,8H,8W] f16 in [0, 1]   sample b is conditioned on image b mod n_ctrl (n_ctrl divides B)
 *   cond_scale                                     conditioning_scale; 0 skips the ControlNet (the plain forward)
 * With a ControlNet attached control_image is required; without one it must be NULL and the call is
 * sd_unet_forward_ex.  The ControlNet runs after the UNet's time embedding, its residuals are added in place into the
 * skips and the mid-block output, one GEMM per site with the residual in its epilogue.  Its conditioning embedding and text K / V follow
 * sd_unet_text_kv_cache: kept across one loop for one (pointer, B, n_ctrl, H, W) / (pointer, B, L), invalidated by
 * every sd_unet_text_kv_cache call.  Graph replay (sd_unet_use_graph) is rejected (SD_ERR_UNSUPPORTED). */
int sd_unet_forward_cn(sd_unet* u, const void* sample, const float* timesteps, const void* ehs, int ehs_len,
                       const void* add_text, const float* add_time_ids, const void* image_embeds, int n_img,
                       const void* control_image, int n_ctrl, float cond_scale, void* out, int B, int H, int W,
                       void* stream);
/* sd_unet_forward_cn for the attached list: control_images[i] [n_ctrl[i],3,8H,8W] f16 and cond_scales[i] belong to net i
 * of sd_unet_set_controlnets; n_nets must equal the attached count (SD_ERR_INVALID).  A net at scale 0 does not run and
 * its image may be NULL; with every scale 0 (or no net attached and n_nets == 0) the call is the plain forward; with one
 * running net it is sd_unet_forward_cn with that net attached alone, bit for bit.  Two or more running nets: every
 * residual site's hidden tensors lie side by side in one buffer [rows, n C] and the sum of the residuals
 *   y += sum_i s_i (h_i W_i^T + b_i) = [h_1 | ... | h_n] [s_1 W_1 | ... | s_n W_n]^T + sum_i s_i b_i
 * is one GEMM per site on weights folded by cn_fold_scales_kernel (one launch for all sites, w_cat = fp16(w * s): one
 * rounding), refolded only when the running nets or a scale change -- or, with the K-concatenated form switched off
 * (sd_cn_kcat_force, SD_NO_CN_KCAT=1), one GEMM per net and site.  SD_ERR_INVALID, nothing launched: a NULL image or an
 * n_ctrl that does not divide B for a running net, a NaN scale.  sd_unet_forward_cn (and every other forward) with more
 * than one net attached is SD_ERR_INVALID.  The caches of sd_unet_forward_cn hold per net. */
int sd_unet_forward_mcn(sd_unet* u, const void* sample, const float* timesteps, const void* ehs, int ehs_len,
                        const void* add_text, const float* add_time_ids, const void* image_embeds, int n_img,
                        const void* const* control_images, const int* n_ctrl, const float* cond_scales, int n_nets,
                        void* out, int B, int H, int W, void* stream);
/* Fold launches (cn_fold_scales_kernel) this UNet has issued since its creation. */
int64_t sd_unet_cn_fold_count(const sd_unet* u);
/* How two or more running ControlNets add their residuals, process-wide (tests / tools): -1 the default, 0 chained (one
 * GEMM per net and site), 1 K-concatenated (one GEMM per site on the folded weights).  SD_NO_CN_KCAT=1 in the
 * environment makes the default the chained form. */
int sd_cn_kcat_force(int mode);
/* The UNet forward of one classifier-free-guidance step from the UN-duplicated latents: what
 * sd_cfg_duplicate(latents, in_scale) followed by sd_unet_forward(_ex) returns, negative half first.
 *   latents   [B,C,H,W] f16        timesteps [B] f32 (both halves share them)
 *   ehs       [2B,ehs_len,ctx] f16  add_text / add_time_ids / image_embeds: 2B rows, as sd_unet_forward_ex takes them
 *                                   (add_time_ids [2B,num_time_ids]; with text_time the duplicate path runs)
 *   in_scale  the scheduler's scale_model_input factor, applied as fp16(latents * in_scale)
 *   out       [2B,Cout,H,W] f16
 * With share != 0 and a topology for which sd_unet_cfg_share answers 1, everything in front of the first cross-attention
 * (conv_in, down_blocks.0.resnets.0, the first transformer's norm, proj_in, q|k|v, self-attention, to_out, attn2.to_q)
 * runs once per latent, on B images, and is widened to 2B in one copy launch: the two halves hold the same values there.
 * Otherwise -- share == 0, graph replay on, SD_NO_CFG_SHARE or SD_GN_CAT set in the environment, such a topology -- the
 * engine duplicates into a buffer of its own and runs the ordinary forward: bit for bit the two-call result.  An attached
 * ControlNet needs its control image: use sd_cfg_duplicate + sd_unet_forward_cn. */
int sd_unet_forward_cfg(sd_unet* u, const void* latents, const float* timesteps, const void* ehs, int ehs_len,
                        const void* add_text, const float* add_time_ids, const void* image_embeds, int n_img,
                        float in_scale, int share, void* out, int B, int H, int W, void* stream);
/* 1 when the topology lets sd_unet_forward_cfg share: no per-sample additional embedding (text_time makes the time
 * embedding differ between the halves) and a transformer in down block 0.  Needs no device. */
int sd_unet_cfg_share(const sd_unet_config* cfg);
/* Perturbed-attention guidance (Ahn et al., "Self-Rectifying Diffusion Sampling with Perturbed-Attention Guidance", 2024;
 * diffusers >= 0.30 StableDiffusionPAGPipeline, recalled).  sd_unet_set_pag_layers flags transformers by the site keys
 * the engine names its Transformer2DModels with -- "down_blocks.i.attentions.j", "mid_block.attentions.0",
 * "up_blocks.i.attentions.j" -- count = 0 clears every flag; a key that names no transformer of this topology:
 * SD_ERR_INVALID, nothing changed.  The flags act in sd_unet_forward_pag only; every other forward ignores them.
 *
 * sd_unet_forward_pag: one forward on G + 1 groups of B images, G = 2 with cfg != 0 ([uncond ; text ; perturbed]), else 1
 * ([text ; perturbed]), from the UN-duplicated latents (fp16(latents * in_scale), as sd_unet_forward_cfg):
 *   latents [B,C,H,W] f16   timesteps [B] f32   ehs [G B,ehs_len,ctx] f16   add_text / add_time_ids: G B rows
 *   out     [(G+1) B,Cout,H,W] f16
 * The perturbed group takes the text group's latents, timesteps, ehs and added conditions; in every transformer block of
 * a flagged transformer its attn1 is to_out(to_v(norm1(x))) -- the identity attention map: no softmax, no Q, no K.
 * With share != 0 and the first flagged transformer (in execution order: down, mid, up) behind the network's first, the
 * perturbed group does not exist until that transformer's first attn1: everything before runs on G B images (B up to the
 * first cross-attention where sd_unet_forward_cfg would share) and one copy launch widens what the remainder reads.
 * Otherwise -- share == 0, SD_NO_PAG_SHARE or SD_GN_CAT set in the environment, the first transformer flagged -- the
 * engine duplicates up front and runs (G+1) B images throughout.  The text K / V are projected for G B rows and the
 * perturbed group's are a copy (kept by sd_unet_text_kv_cache with the rest).  FreeU composes.
 * SD_ERR_UNSUPPORTED, nothing launched: a ControlNet attached, an IP-Adapter attached at a non-zero scale, a DeepCache
 * store / reuse mode, graph replay on, a UNet with time_cond_proj_dim (timestep_cond).  SD_ERR_INVALID: no flagged
 * transformer, null or NaN arguments. */
int sd_unet_set_pag_layers(sd_unet* u, const char* const* site_keys, int count);
int sd_unet_forward_pag(sd_unet* u, const void* latents, const float* timesteps, const void* ehs, int ehs_len,
                        const void* add_text, const float* add_time_ids, float in_scale, int cfg, int share, void* out,
                        int B, int H, int W, void* stream);
/* InstructPix2Pix (Brooks et al., "InstructPix2Pix: Learning to Follow Image Editing Instructions", 2023; diffusers 0.27.2
 * StableDiffusionInstructPix2PixPipeline, recalled): the forward of a UNet whose sample is [latents | image latents],
 * from the un-concatenated, un-duplicated inputs.  Defined as sd_unet_forward_ex on the sample
 *   cat([fp16(latents[n % B_lat] * in_scale), n < zero_from ? extra[n % extra_rows] : 0], dim = 1),  n in [0, B)
 * at the timesteps [B_lat] repeated per group of B_lat images (on the device: no host op per step):
 *   latents [B_lat,4,H,W] f16   extra [extra_rows,extra_channels,H,W] f16   timesteps [B_lat] f32
 *   ehs [B,ehs_len,ctx] f16     add_text / add_time_ids: NULL (see below)    out [B,Cout,H,W] f16
 * Where the first block is 320 wide and H W % 128 == 0 (SD_NO_EDGE_KERNELS unset) conv_in is one launch that reads both
 * sources (sd_op_unet_conv_in2) and the sample never exists; otherwise one small launch builds it in the workspace and the
 * forward is sd_unet_forward_ex on it bit for bit.
 * SD_ERR_INVALID: 4 + extra_channels != in_channels, B % B_lat != 0, more than 25 groups, zero_from outside [0, B],
 * extra_rows < 1, null or NaN arguments.  SD_ERR_UNSUPPORTED, nothing launched: graph replay on, a ControlNet attached,
 * a DeepCache store / reuse mode, an IP-Adapter attached at a non-zero scale, a UNet with time_cond_proj_dim, a UNet
 * with text_time conditioning (the time embedding is computed per latent and tiled, and add_text / add_time_ids differ
 * per group: such a UNet takes the 8-channel sample through sd_unet_forward_ex).  These are checked before the shapes. */
int sd_unet_forward_concat(sd_unet* u, const void* latents, int B_lat, float in_scale, const void* extra, int extra_channels,
                           int extra_rows, int zero_from, const float* timesteps, const void* ehs, int ehs_len,
                           const void* add_text, const float* add_time_ids, void* out, int B, int H, int W, void* stream);
/* UNet2DConditionModel.enable_freeu(s1, s2, b1, b2) / disable_freeu() of diffusers 0.27.2 (enable = 0: the factors are
 * ignored and the forward is again exactly the plain one).  On, every resnet of up blocks 0 and 1 reads
 *   cat([hidden with its first C1 / 2 channels times b, fourier_filter(skip, threshold = 1, scale = s)])
 * with (b, s) = (b1, s1) in block 0 and (b2, s2) in block 1 (diffusers' apply_freeu), after any ControlNet residual was
 * added to the skip: one in-place launch per resnet (sd_op_freeu).  Holds for sd_unet_forward, _ex, _cn and _cfg.
 * Non-finite factors: SD_ERR_INVALID.  Graph replay (sd_unet_use_graph) with FreeU on is rejected by the forward
 * (SD_ERR_UNSUPPORTED). */
int sd_unet_set_freeu(sd_unet* u, int enable, float s1, float s2, float b1, float b2);
/* Token merging (Bolya & Hoffman, "Token Merging for Fast Stable Diffusion"; tomesd's apply_patch with its defaults:
 * merge_attn only) for the self-attention of every BasicTransformerBlock whose map is at most max_downsample times
 * smaller than the sample (sample_height / H <= max_downsample, max_downsample in {1, 2, 4, 8}).  Such a block matches
 * its tokens on the residual stream norm1 reads (sd_op_tome_match with site = the block's ordinal among all
 * BasicTransformerBlocks in execution order of the full forward, step = sd_unet_tome_step's), merges the rows of the
 * q|k|v projection (the projections are linear: the mean of projected rows is the projection of the mean), runs the
 * attention on T' = T - r rows and copies its output back through the unmerge map; the q|k|v and out-projection GEMMs
 * stay full-size.  A block with r = 0 runs the plain path bit for bit.  ratio = 0 means off: the other arguments are
 * ignored, the buffer is released and the forward is again exactly the plain one, with the same launches.
 * Holds for sd_unet_forward, _ex, _tc and _cfg and with the DeepCache modes.  With debug taps on (sd_unet_tap) every
 * merging block also records the view its match read, as the input of "tome.<site>".  SD_ERR_INVALID: ratio outside
 * [0, 0.75] or NaN, sx or sy outside 1..8, an unlisted max_downsample.  With it on the forward returns
 * SD_ERR_UNSUPPORTED, nothing launched, for a merging block of more than 16384 tokens or without a whole cell, with
 * graph replay on (sd_unet_use_graph), in sd_unet_forward_pag / sd_unet_forward_concat, and with FreeU on, a ControlNet
 * attached or an IP-Adapter attached (no test composes those with it yet). */
int sd_unet_set_tome(sd_unet* u, double ratio, int max_downsample, int sx, int sy, int use_rand, uint32_t seed);
/* The step index the destination draw of the following forwards hashes (the loop's iteration; 0 until set). */
int sd_unet_tome_step(sd_unet* u, uint32_t step);
/* The merging blocks of the last forward, in execution order: their count, and for the k-th one
 * info5 = (site, H, W, r, T') and, when map_host is non-NULL, its unmerge maps [images, H W] int32 (cap = the entries
 * map_host holds).  The maps live in a buffer the handle keeps (counted in sd_unet_memory's workspace_bytes) until the
 * next forward.  sd_unet_tome_read returns the number of images the block ran on (half the batch inside the shared CFG
 * prefix), or -SD_ERR_*; it synchronises the device. */
int sd_unet_tome_sites(const sd_unet* u);
int sd_unet_tome_read(sd_unet* u, int k, int32_t* info5, int32_t* map_host, int64_t cap);
/* HyperTile (tfernd/HyperTile, as A1111 / Forge / SD.Next / ComfyUI ship it; scale_depth off): the self-attention of
 * every BasicTransformerBlock of a level l <= max_depth (its map is Hs x Ws = H >> l x W >> l) is restricted to the
 * tokens of one spatial tile, and the division nh x nw is drawn anew per step (sd_hypertile_plan with site = the block's
 * ordinal as for token merging, step = sd_unet_hypertile_step's; tile_size in tokens of the site's own level).  The
 * draw is the same for every image of the batch and both CFG halves.  Token (y, x) of image b attends to exactly the
 * tokens of tile (y / th, x / tw) of image b; scale, head split and pre-scaled queries are unchanged.  A site that
 * draws (1, 1) issues the plain launches and is bit for bit the plain block.  nw == 1 cuts the NHWC rows into contiguous
 * bands: the attention kernel runs in place with batch B nh, nothing is copied.  Otherwise the q|k|v rows are gathered
 * into tile order (sd_op_hypertile_gather), the unchanged attention kernel runs with batch B nh nw on th tw tokens and
 * its output is scattered back (sd_op_hypertile_scatter); the gather buffers are workspace, planned for every site
 * that can draw nw > 1.  Only attn1 changes: cross-attention, IP-Adapter, regional weights, FreeU, DeepCache and
 * ControlNet residuals see raster-order rows; a ControlNet's own encoder runs without tiling.  tile_size = 0 means
 * off: the other arguments are ignored and the forward is again exactly the plain one, with the same launches.
 * SD_ERR_INVALID: tile_size < 0, swap_size outside 1..8, max_depth outside 0..3.  SD_ERR_UNSUPPORTED, nothing changed:
 * token merging is on (and sd_unet_set_tome with a ratio > 0 while HyperTile is on): both rewrite attn1's rows.  With
 * it on the forward returns SD_ERR_UNSUPPORTED, nothing launched, with graph replay on (the division changes per step)
 * and in sd_unet_forward_pag (the perturbed branch's identity attention). */
int sd_unet_set_hypertile(sd_unet* u, int tile_size, int swap_size, int max_depth, uint32_t seed);
/* The step index the division draw of the following forwards hashes (the loop's iteration; 0 until set). */
int sd_unet_hypertile_step(sd_unet* u, uint32_t step);
/* The participating sites (level <= max_depth) of the last forward, in execution order: their count, and for the k-th
 * one info8 = (site, Hs, Ws, nh, nw, images, copied 0/1, level).  images is the batch the block ran on (half of it inside
 * the shared CFG prefix); copied says whether the gather / scatter launches ran (nw > 1).  SD_ERR_INVALID for a null
 * argument or k outside [0, sites).  Neither touches the device. */
int sd_unet_hypertile_sites(const sd_unet* u);
int sd_unet_hypertile_read(const sd_unet* u, int k, int32_t* info8);
/* DeepCache (Ma, Fang, Wang, CVPR 2024): reuse the deep features of the UNet across denoising steps.  With
 *   L = layers_per_block, s_0 = conv_in's output, s_j = the output of layer j - 1 of down block 0,
 * layer j of the last up block (j = 0..L) reads cat([hidden, s_{L-j}]).  For a depth d in 1..L the cached feature F_d
 * is the hidden input of layer L - d of the last up block.  Forwards then run in one of three modes:
 *   SD_DC_PLAIN  the forward as without the feature;
 *   SD_DC_STORE  the full forward, bit for bit the plain one with the same launches, which leaves F_d in a buffer the
 *                handle keeps (counted in sd_unet_memory's workspace_bytes);
 *   SD_DC_REUSE  time embedding and text / image K/V as always, conv_in, layers 0..d-1 of down block 0 (no
 *                downsampler), layers L-d..L of the last up block -- the first reading cat([F_d, s_d]) with the stored
 *                F_d and this step's s_d -- and conv_norm_out / conv_out.  No other block, no ControlNet.
 * The stored feature holds for one (B, H, W, shared CFG prefix or not); sd_unet_set_deep_cache, _set_freeu,
 * _set_ip_adapter and _set_controlnet invalidate it.  Holds for sd_unet_forward, _ex, _tc and _cfg.  Errors, nothing
 * launched: a reuse forward without a stored step of the call's shape: SD_ERR_STATE; a store / reuse forward with graph
 * replay on, with a ControlNet that would run (attached, control image given, scale != 0), or with FreeU on and fewer
 * than three blocks (FreeU would touch the last block): SD_ERR_UNSUPPORTED. */
#define SD_DC_PLAIN 0
#define SD_DC_STORE 1
#define SD_DC_REUSE 2
/* depth 0 = off (the forward is again exactly the plain one, the buffer is released); 1..layers_per_block, anything
 * else SD_ERR_INVALID.  Every call resets the mode to SD_DC_PLAIN and invalidates the cache. */
int sd_unet_set_deep_cache(sd_unet* u, int depth);
/* Mode of the following forwards, until changed.  An unknown mode: SD_ERR_INVALID; store / reuse while the depth is 0:
 * SD_ERR_STATE. */
int sd_unet_deep_cache_mode(sd_unet* u, int mode);
/* Regional prompts ("attention couple"; this project's own semantics, not a diffusers 0.27.2 feature): R prompts of
 * L tokens each ride in one encoder_hidden_states of ehs_len = R L tokens, and at every attn2
 *   out[n, t] = sum_r W_l[n % Bw, t, r] softmax(s q[n, t] K[n, rL:(r+1)L]^T) V[n, rL:(r+1)L]
 * in one launch (sd_op_region_cross_attention) in place of the plain cross-attention; attn1 and everything else are
 * unchanged.  weights [Bw, R, H, W] fp32 on the device are the sample-resolution ones (sum 1 over R per pixel is the
 * caller's business); a transformer on an (H >> l, W >> l) map reads their 2x2 mean l times over (sd_op_region_pyramid,
 * one launch on `stream`, into a buffer the handle keeps with a copy of `weights`; both are counted in sd_unet_memory's
 * workspace_bytes, and sd_unet_poison_workspace overwrites the level weights, which the next forward then rebuilds).
 * Forwards issued on `stream` afterwards see them.  1 <= R <= 8, H and W divisible by 2^(blocks-1) (SD_ERR_INVALID),
 * every cross-attention head dim in {32, 40, 64, 80, 160} (SD_ERR_UNSUPPORTED).  weights == NULL or R == 0 clears the
 * regions: the buffers are released and the forward is again exactly the plain one, with the same launches.
 * With regions set, sd_unet_forward, _ex (no image embeds) and _cfg (shared prefix included: the text enters after it)
 * take them; the text-K/V cache composes.  SD_ERR_INVALID: ehs_len % R != 0, B % Bw != 0 (B: the forward's batch, twice
 * the latents' for _cfg), H or W other than the ones set.  SD_ERR_UNSUPPORTED, nothing launched: a ControlNet attached,
 * an IP-Adapter attached at a non-zero scale, sd_unet_forward_pag, _concat, _tc with a timestep_cond, graph replay on,
 * token merging on, a DeepCache store / reuse mode, more than 160 tokens per region. */
int sd_unet_set_regions(sd_unet* u, const float* weights, int Bw, int R, int H, int W, void* stream);
/* Bytes of device memory held (packed weights, workspace).  The workspace is the arena, the DeepCache, token-merging
 * and regional-prompt buffers, the duplicated-latents buffer of sd_unet_forward_cfg / _pag and the staging buffer of
 * graph replay. */
int sd_unet_memory(const sd_unet* u, int64_t* weight_bytes, int64_t* workspace_bytes);

/* -- IP-Adapter: the `encoder_hid_proj` ImageProjection and every attn2's to_k_ip / to_v_ip that diffusers'
 *    load_ip_adapter adds to the UNet (sd_unified_pipeline.py:441-449).  Weight names are diffusers' post-load keys:
 *      encoder_hid_proj.image_projection_layers.0.{image_embeds,norm}.{weight,bias}
 *      <down / up / mid transformer block>.attn2.processor.to_{k,v}_ip.0.weight   [C, cross_attention_dim]
 *    (stablediffusion_amd/ip_adapter.py converts the original files).  image_embed_dim: 1024 (ViT-H/14), 1280
 *    (ViT-bigG), any positive multiple of 64; num_tokens in [1, 16] (4 for the base adapters).  SD_ERR_UNSUPPORTED:
 *    cross_attention_dim % 64 != 0, num_tokens out of range, a head dim outside {32, 40, 64, 80, 160}.  Destroying an
 *    attached adapter detaches it first: the UNet's next forward is the plain one (and rejects image_embeds). ------ */
int sd_ip_adapter_create(const sd_unet* u, int image_embed_dim, int num_tokens, sd_ip_adapter** out);
int sd_ip_adapter_destroy(sd_ip_adapter* a);
int sd_ip_adapter_num_weights(const sd_ip_adapter* a);
int sd_ip_adapter_weight_info(const sd_ip_adapter* a, int index, const char** key, int64_t* shape4, int* ndim);
int sd_ip_adapter_set_weight(sd_ip_adapter* a, const char* key, const void* data, const int64_t* shape, int ndim,
                             int dtype);
int sd_ip_adapter_finalize(sd_ip_adapter* a);
/* -- IP-Adapter Plus: the image projection is the perceiver Resampler of the IP-Adapter repository (diffusers'
 *    IPAdapterPlusImageProjection), restated from memory -- no copy of either is pinned by a test here.  With
 *    lat = latents per image and x = proj_in(features), each of `depth` layers computes
 *      q = to_q(norm2(lat)), [k | v] = to_kv(cat([norm1(x), norm2(lat)])), lat += to_out(softmax(q k^T / 8) v),
 *      lat += W2 gelu_erf(W1 LayerNorm(lat))
 *    and tokens = norm_out(proj_out(lat)), [num_tokens, cross_attention_dim] per image.  Weight names are the original
 *    file's `image_proj.*` suffixes, unchanged, under encoder_hid_proj.image_projection_layers.0. :
 *      latents [1,num_tokens,dim]   proj_in / proj_out .{weight,bias}   norm_out.{weight,bias}
 *      layers.{i}.0.{norm1,norm2}.{weight,bias}   layers.{i}.0.{to_q,to_kv,to_out}.weight   (heads * 64 query rows)
 *      layers.{i}.1.0.{weight,bias}   layers.{i}.1.1.weight [ff_mult dim, dim]   layers.{i}.1.3.weight
 *    followed by the to_{k,v}_ip keys of sd_ip_adapter_create.  The head dim is 64 (dim_head of every published
 *    file).  sd_ip_adapter_create_ex with kind SD_IP_PROJ_LINEAR is sd_ip_adapter_create (the Resampler fields are
 *    ignored).  SD_ERR_UNSUPPORTED: what sd_ip_adapter_create rejects; for the Resampler also dim not a positive
 *    multiple of 64, heads < 1, heads * 64 != dim (another dim_head: published files have dim = heads * 64), depth
 *    outside [1, 16], ff_mult outside [1, 8].  SD_ERR_INVALID: an unknown kind, null arguments.
 *    With a Resampler adapter attached, image_embeds of sd_unet_forward_ex / _tc / _cn / _cfg means
 *    [B, n_img, T_feat, image_embed_dim] f16: the image encoder's hidden_states[-2].  The Resampler runs where the
 *    linear projection runs, once per loop under the image K / V cache rules of sd_unet_forward_ex. ------ */
#define SD_IP_PROJ_LINEAR 0
#define SD_IP_PROJ_RESAMPLER 1
typedef struct sd_ip_projection_config {
    int32_t kind;                /* SD_IP_PROJ_* */
    int32_t image_embed_dim;     /* D_emb: 1280 (ViT-H/14 hidden size) for the published Plus files */
    int32_t num_tokens;          /* tokens per image: the Resampler's queries (16) */
    int32_t dim;                 /* Resampler width: 768 (SD1.5 Plus), 1280 (SDXL Plus) */
    int32_t heads;               /* 12 / 20 */
    int32_t depth;               /* 4 */
    int32_t ff_mult;             /* 4 */
} sd_ip_projection_config;
int sd_ip_adapter_create_ex(const sd_unet* u, const sd_ip_projection_config* cfg, sd_ip_adapter** out);
/* Feature tokens per image the Resampler reads (default 257 = 16 x 16 patches + class token; 1 + (image_size /
 * patch_size)^2 of the tower in use).  Invalidates the image K / V cache of the UNet the adapter is attached to.
 * SD_ERR_INVALID: T_feat < 1; SD_ERR_UNSUPPORTED: T_feat + num_tokens > 320, the keys the attention kernel holds in
 * LDS, or a linear adapter. */
int sd_ip_adapter_set_feature_tokens(sd_ip_adapter* a, int T_feat);
/* The image projection alone, on the adapter's own workspace: image_embeds as the UNet forward takes them for `rows`
 * (= B * n_img) images -> tokens [rows, num_tokens, cross_attention_dim] f16.  Both kinds; for tests and tools. */
int sd_ip_adapter_project(sd_ip_adapter* a, const void* image_embeds, int rows, void* tokens, void* stream);
/* Bytes of device memory held (packed weights, sd_ip_adapter_project's workspace). */
int sd_ip_adapter_memory(const sd_ip_adapter* a, int64_t* weight_bytes, int64_t* workspace_bytes);

/* -- ControlNet (diffusers 0.27.2 ControlNetModel), bound to a UNet.  cn_cfg describes its encoder (the up-path fields
 *    are ignored); weight names are diffusers' (stablediffusion_amd/controlnet.py converts original files):
 *      conv_in, time_embedding, add_embedding (text_time), down_blocks.*, mid_block.*,
 *      controlnet_cond_embedding.{conv_in, blocks.0-5, conv_out}  (conditioning_embedding_out_channels (16,32,96,256)),
 *      controlnet_down_blocks.{0..n-1}, controlnet_mid_block
 *    SD_ERR_INVALID: residual shapes that do not match u's skips (num_blocks, block_out_channels, layers_per_block), a
 *    different cross_attention_dim, in_channels or text_time conditioning.  Heads and transformer depth may differ.
 *    SD_ERR_UNSUPPORTED: conditioning_channels != 3, more than 15 skips.  Destroying an attached ControlNet detaches
 *    it first. ------ */
int sd_controlnet_create(const sd_unet* u, const sd_unet_config* cn_cfg, int conditioning_channels, sd_controlnet** out);
int sd_controlnet_destroy(sd_controlnet* cn);
int sd_controlnet_num_weights(const sd_controlnet* cn);
int sd_controlnet_weight_info(const sd_controlnet* cn, int index, const char** key, int64_t* shape4, int* ndim);
int sd_controlnet_set_weight(sd_controlnet* cn, const char* key, const void* data, const int64_t* shape, int ndim,
                             int dtype);
int sd_controlnet_finalize(sd_controlnet* cn);

/* -- AnimateDiff motion adapter (diffusers 0.27.2 MotionAdapter / UNetMotionModel / TransformerTemporalModel, recalled:
 * the library is not installed where this was written; tests/motion_oracle.py restates the semantics in float) ----------
 * The UNet's batch is V videos of num_frames consecutive frames; the text embedding of a video is repeated per frame.
 * One motion module runs behind every (resnet, transformer) pair of the down and up blocks (behind the resnet in a block
 * without attention) and, with use_mid_block, behind the mid block's transformer, before its second resnet; what goes
 * into a skip connection is the module's output.  A module, on x [V F, C, H, W]:
 *   GroupNorm(32, eps 1e-6) with statistics over a group's channels and all F H W positions of one video; proj_in
 *   (Linear, bias); h += to_out(attn(LN1(h) + pe)); h += to_out2(attn(LN2(h) + pe)); h += FF_geglu(LN3(h)); proj_out;
 *   + x.  Both attentions are self-attention over the F frames of one pixel of one video with num_heads[block] heads
 * (to_q / to_k / to_v without bias), pe[f, 2i] = sin(f 10000^(-2i/C)), pe[f, 2i+1] = cos(same) for
 * f < max_seq_length <= 32.  The position rows are folded into a per-frame fp32 table at sd_motion_finalize
 * (sd_op_motion_pos_bias) and the attention is one launch on the q|k|v rows in place (sd_op_temporal_attention).
 * Weight keys are the diffusers MotionAdapter's ("down_blocks.0.motion_modules.1.transformer_blocks.0.attn1.to_q.weight",
 * "mid_block.motion_modules.0.proj_in.bias", ...) without the stored pos_embed.pe tables. */
typedef struct sd_motion_config {
    int32_t num_blocks;
    int32_t block_out_channels[SD_MAX_BLOCKS];
    int32_t num_heads[SD_MAX_BLOCKS];              /* per down block; reversed for up blocks */
    int32_t layers_per_block;
    int32_t max_seq_length;                        /* 1..32 */
    int32_t use_mid_block;
} sd_motion_config;
/* For the UNet `u`: blocks, channels and layers_per_block must be the UNet's, every head dim C / heads one of 32, 40, 64,
 * 80, 160 and every C a multiple of 64 (SD_ERR_INVALID / SD_ERR_UNSUPPORTED). */
int sd_motion_create(const sd_unet* u, const sd_motion_config* cfg, sd_motion** out);
int sd_motion_destroy(sd_motion* m);              /* detaches it from its UNet first */
int sd_motion_num_weights(const sd_motion* m);
int sd_motion_weight_info(const sd_motion* m, int index, const char** key, int64_t* shape4, int* ndim);
int sd_motion_set_weight(sd_motion* m, const char* key, const void* data, const int64_t* shape, int ndim, int dtype);
int sd_motion_finalize(sd_motion* m);
/* Attach a finalized adapter created for this UNet (NULL detaches: every forward is again exactly the plain one, with the
 * same launches).  Attached, nothing changes either until a call names its frames:
 * sd_unet_forward_motion = sd_unet_forward on B = V num_frames frames with the modules running (num_frames = 0: the plain
 * forward); sd_unet_forward_cfg_ex = sd_unet_forward_cfg with num_frames, on B = V num_frames latents: the shared CFG
 * prefix ends before the first module, the CFG batch is 2V videos.
 * SD_ERR_INVALID: B % num_frames != 0, num_frames < 0 or > max_seq_length, num_frames > 0 without an adapter.
 * SD_ERR_UNSUPPORTED, nothing launched, with num_frames >= 1: graph replay, a DeepCache store / reuse mode, token merging,
 * HyperTile, sd_unet_forward_pag, sd_unet_forward_concat, regional prompts, an attached ControlNet, an IP-Adapter at a
 * non-zero scale (at scale 0 the text attention runs alone and image_embeds may be NULL), FreeU and text_time UNets -- none is
 * composed with frames yet, nothing is ignored.  timestep_cond cannot be expressed with frames: sd_unet_forward_tc names
 * none, and the two entries that do take no timestep_cond.
 * With debug taps on a module records its input and output as "<block>.motion_modules.<j>". */
int sd_unet_set_motion(sd_unet* u, sd_motion* m);
int sd_unet_forward_motion(sd_unet* u, const void* sample, const float* timesteps, const void* ehs, int ehs_len, int num_frames,
                           void* out, int B, int H, int W, void* stream);
int sd_unet_forward_cfg_ex(sd_unet* u, const void* latents, const float* timesteps, const void* ehs, int ehs_len,
                           const void* add_text, const float* add_time_ids, const void* image_embeds, int n_img,
                           float in_scale, int share, int num_frames, void* out, int B, int H, int W, void* stream);

/* -- VAE: replaces the object in SDModelWrapper.vae (stable_diffusion.py:110-116) ------------ */
int sd_vae_create(const sd_vae_config* cfg, sd_vae** out);
int sd_vae_destroy(sd_vae* v);
int sd_vae_num_weights(const sd_vae* v);
int sd_vae_weight_info(const sd_vae* v, int index, const char** key, int64_t* shape4, int* ndim);
int sd_vae_set_weight(sd_vae* v, const char* diffusers_key, const void* data,
                      const int64_t* shape, int ndim, int dtype);
int sd_vae_finalize(sd_vae* v);
/* AutoencoderKL.decode(z)[0] (sd_unified_pipeline.py:523): z [B,4,h,w] f16 -> img [B,3,8h,8w] f16. */
int sd_vae_decode(sd_vae* v, const void* z, void* img, int B, int h, int w, void* stream);
/* AutoencoderKL.encode(x) up to the moments (sd_unified_pipeline.py:1027-1032):
 * img [B,3,H,W] f16 -> moments [B,8,H/8,W/8] f16 (mean | logvar); sampling stays host code. */
int sd_vae_encode(sd_vae* v, const void* img, void* moments, int B, int H, int W, void* stream);
/* `vae.config.force_upcast` (sd_unified_pipeline.py:1020-1036): the reference runs such a VAE (SDXL's) in float32 around
 * encode because its activations leave fp16's range.  The engine instead stores every inter-layer activation of the encoder
 * 2^-shift times smaller -- GroupNorm is invariant to the scale of its input (eps is scaled along), so the encoder computes
 * the same function with fp32 accumulators and statistics as before; shift = 0 (default) is plain fp16 storage.  Applies
 * to the following sd_vae_encode calls of this handle. */
int sd_vae_encode_range_shift(sd_vae* v, int shift);
int sd_vae_memory(const sd_vae* v, int64_t* weight_bytes, int64_t* workspace_bytes);

/* -- Debug taps: the input and the output view of every block of ONE forward, copied as the block read and wrote them
 *    (NHWC f16 with their row stride), for tests that compare each block with a reference on the block's own input.
 *    Off (the default) a forward does nothing for them: the same launches, allocations and bits as without the facility.
 *    sd_unet_tap(u, 1) / sd_vae_tap(v, 1): every following sd_unet_forward / _ex / _tc / _cn (sd_vae_decode / _encode)
 *    replaces the records with its own, in buffers outside the workspace arena; the copies run on the forward's stream
 *    and the forward's output is bit for bit what it is with taps off.  While taps are on, graph replay,
 *    sd_unet_forward_cfg where it would share the CFG prefix, sd_unet_forward_pag, sd_unet_forward_concat and the
 *    DeepCache store / reuse modes return SD_ERR_UNSUPPORTED and launch nothing.  (enable = 0 frees the records.)
 *    Records, in execution order (names are diffusers prefixes):
 *      UNet: "emb" (f32 [B, 4 C0]: silu(time_embedding (+ add_embedding)), the form the device keeps), "conv_in" (its
 *      output; its input is the sample), every "*.resnets.j", "*.attentions.j", "*.downsamplers.0", "*.upsamplers.0"
 *      (an up-path resnet's input is the [x | skip] concatenation), "tail" (input of conv_norm_out -> SiLU -> conv_out;
 *      its output is the forward's).
 *      VAE: "decoder.conv_in" (output of post_quant_conv + conv_in), "decoder.mid_block.resnets.j",
 *      "decoder.mid_block.attentions.0", "decoder.up_blocks.i.resnets.j", "decoder.up_blocks.i.upsamplers.0",
 *      "decoder.tail" (input); "encoder.conv_in", "encoder.down_blocks.i.resnets.j",
 *      "encoder.down_blocks.i.downsamplers.0", "encoder.mid_block.*", "encoder.tail" (input).
 *    A record holds N H W rows of `ld` elements; the view is columns [c0, c0 + C).  kind: SD_TAP_IN / SD_TAP_OUT, and
 *    SD_TAP_PRE = the rows of an output view narrower than its row (ld > C) as they were before the block ran, so a
 *    test can see that the block left the other columns alone.  scale: the activations are stored scale times their
 *    value (sd_vae_encode_range_shift: 2^-shift; 1 otherwise).
 *    _tap_info: SD_ERR_INVALID for a null argument or an index outside [0, _tap_count).  _tap_read synchronises the
 *    device and copies record `index` to host memory `dst`; `bytes` must equal the record's (SD_ERR_INVALID). ---------- */
#define SD_TAP_IN 0
#define SD_TAP_OUT 1
#define SD_TAP_PRE 2
typedef struct sd_tap_info {
    const char* name;   /* owned by the handle, valid until its next forward or sd_*_tap call */
    int32_t kind;       /* SD_TAP_* */
    int32_t dtype;      /* SD_DTYPE_F16 / SD_DTYPE_F32 */
    int32_t N, H, W, C; /* the view: [N, H, W, C] */
    int32_t c0;         /* first column of the view inside a row of the record */
    int64_t ld;         /* elements per row of the record */
    int64_t bytes;
    float scale;
} sd_tap_info;
int sd_unet_tap(sd_unet* u, int enable);
int sd_unet_tap_count(const sd_unet* u);
int sd_unet_tap_info(const sd_unet* u, int index, sd_tap_info* info);
int sd_unet_tap_read(sd_unet* u, int index, void* dst, int64_t bytes);
int sd_vae_tap(sd_vae* v, int enable);
int sd_vae_tap_count(const sd_vae* v);
int sd_vae_tap_info(const sd_vae* v, int index, sd_tap_info* info);
int sd_vae_tap_read(sd_vae* v, int index, void* dst, int64_t bytes);

/* -- Workspace poisoning: a TEST FACILITY, like the taps; no product path calls it.  A handle's scratch memory carries no
 *    state from call to call, so a call's result may not depend on what an earlier call left there, non-finite values
 *    included.  These entries overwrite that memory so that a test can see it: the handle's workspace arena over its whole
 *    capacity and, for the UNet, the buffer of forward_cfg's / forward_pag's duplicated latents and the staging buffer of
 *    graph replay, and the per-level weights of regional prompts (rebuilt by the next forward from the handle's copy of
 *    the caller's weights).  The tagged caches (text / image / ControlNet K/V, the conditioning embedding, the DeepCache
 *    feature, the token-merging plans) and that copy hold state and are left alone.
 *      pattern SD_POISON_NAN: every byte 0xFF (NaN as f16, f32 and f64, -1 as an integer);
 *      pattern SD_POISON_INF: every 16-bit word 0x7C00 (f16 +Inf).
 *    *bytes_filled = the sum of the filled buffers' capacities, which is sd_*_memory's workspace_bytes less (UNet) the
 *    DeepCache and token-merging buffers and the copy of the regional weights; 0 with SD_OK for a handle that has allocated nothing.  The device is
 *    synchronised before the fill and after it.  SD_ERR_INVALID, nothing launched: a null argument, an unknown pattern. */
#define SD_POISON_NAN 0
#define SD_POISON_INF 1
int sd_unet_poison_workspace(sd_unet* u, int pattern, int64_t* bytes_filled);
int sd_vae_poison_workspace(sd_vae* v, int pattern, int64_t* bytes_filled);
int sd_clip_poison_workspace(sd_clip* c, int pattern, int64_t* bytes_filled);
int sd_clip_vision_poison_workspace(sd_clip_vision* c, int pattern, int64_t* bytes_filled);
int sd_ip_adapter_poison_workspace(sd_ip_adapter* a, int pattern, int64_t* bytes_filled);

/* -- CLIP text encoder: replaces SDModelWrapper.text_encoder / .text_encoder_2 as encode_prompt calls
 *    them (sd_unified_pipeline.py:592-608).  Weight names are the
 *    transformers state-dict keys ("text_model.embeddings.token_embedding.weight", ...,
 *    "text_projection.weight"). ------------------------------------------------------------------ */
int sd_clip_create(const sd_clip_config* cfg, sd_clip** out);
int sd_clip_destroy(sd_clip* c);
int sd_clip_num_weights(const sd_clip* c);
int sd_clip_weight_info(const sd_clip* c, int index, const char** key, int64_t* shape4, int* ndim);
int sd_clip_set_weight(sd_clip* c, const char* key, const void* data, const int64_t* shape, int ndim, int dtype);
int sd_clip_finalize(sd_clip* c);
/* text_encoder(input_ids, output_hidden_states=True): ids int32 [B,T] (device).  Outputs, each
 * nullable, all f16 on the device:
 *   hidden_states [num_layers+1, B, T, H]  (embeddings, then every layer's output; no final norm)
 *   last_hidden   [B, T, H]                (final_layer_norm of the last one)
 *   pooled        [B, H]                   (last_hidden at eos_index[b]; pooler_output)
 *   text_embeds   [B, projection_dim]      (text_projection(pooled); needs projection_dim > 0)
 * eos_index int32 [B] (device) is required for pooled / text_embeds: the host picks it the way
 * transformers does (argmax of the ids, or first eos_token_id). */
int sd_clip_forward(sd_clip* c, const int32_t* input_ids, const int32_t* eos_index, void* hidden_states,
                    void* last_hidden, void* pooled, void* text_embeds, int B, int T, void* stream);
/* text_encoder.text_model.final_layer_norm(x) for the clip_skip branch (sd_unified_pipeline.py:608). */
int sd_clip_final_layer_norm(sd_clip* c, const void* x, void* y, int64_t rows, void* stream);
int sd_clip_memory(const sd_clip* c, int64_t* weight_bytes, int64_t* workspace_bytes);

/* -- CLIP vision tower: fills SDModelWrapper.image_encoder for ip_adapter_image (transformers
 *    CLIPVisionModelWithProjection).  Weight names are the transformers state-dict keys
 *    ("vision_model.embeddings.class_embedding", ..., "vision_model.pre_layrnorm.weight" (sic), ...,
 *    "visual_projection.weight").  Create rejects (SD_ERR_UNSUPPORTED, with a message): image_size not divisible by
 *    patch_size, hidden_size not divisible by num_heads or not a multiple of 8, and a head dim that is neither one of
 *    the attention kernels' nor paddable to one of at most 128 (hidden 1664 / 16 heads = 104 runs at 128: the heads
 *    are zero-padded when the weights are packed). ------------------------------------------------------------------ */
int sd_clip_vision_create(const sd_clip_vision_config* cfg, sd_clip_vision** out);
int sd_clip_vision_destroy(sd_clip_vision* c);
int sd_clip_vision_num_weights(const sd_clip_vision* c);
int sd_clip_vision_weight_info(const sd_clip_vision* c, int index, const char** key, int64_t* shape4, int* ndim);
int sd_clip_vision_set_weight(sd_clip_vision* c, const char* key, const void* data, const int64_t* shape, int ndim,
                              int dtype);
int sd_clip_vision_finalize(sd_clip_vision* c);
/* image_encoder(pixel_values, output_hidden_states=True): pixel_values f16 NCHW [B,3,S,S] (device), already
 * normalised.  T = 1 + (S / P)^2 tokens.  Outputs, each nullable, all f16 on the device:
 *   hidden_states [num_layers+1, B, T, H]  ([0] = pre_layrnorm(embeddings), then every layer's output)
 *   last_hidden   [B, T, H]                (= hidden_states[num_layers]: no final norm)
 *   pooled        [B, H]                   (post_layernorm(last_hidden[:, 0]); pooler_output)
 *   image_embeds  [B, projection_dim]      (visual_projection(pooled)) */
int sd_clip_vision_forward(sd_clip_vision* c, const void* pixel_values, void* hidden_states, void* last_hidden,
                           void* pooled, void* image_embeds, int B, void* stream);
int sd_clip_vision_memory(const sd_clip_vision* c, int64_t* weight_bytes, int64_t* workspace_bytes);
/* The embedding stage of the tower alone, one launch: pixels f16 [B,3,S,S], w f16 [H,3,P,P] (patch_embedding.weight, no
 * bias), class_embedding f16 [H], position_embedding f16 [1 + (S/P)^2, H] -> out f16 [B, 1 + (S/P)^2, H] with row stride
 * ld_out elements (>= H, a multiple of 8), BEFORE pre_layrnorm.  fp32 accumulation, one fp16 rounding. */
int sd_op_vit_patch_embed(const void* pixels, const void* w, const void* class_embedding, const void* position_embedding,
                          void* out, int64_t ld_out, int B, int image_size, int patch_size, int hidden, void* stream);

/* -- denoise-step glue (sd_unified_pipeline.py:467-469, :484-489) ---------------------------- */
/* latent_model_input = cat([latents]*2) * in_scale   (in_scale = 1 for DDIM / DPM++) */
int sd_cfg_duplicate(const void* latents, void* out2b, int64_t n_per_batch, int B, float in_scale,
                     void* stream);

/* The CFG combine and the update of every scheduler of the reference's registry (stable_diffusion.py:199-227) whose
 * update is linear in (x, eps, previous x0 prediction) -- DDIM, Euler, DPM-Solver++(2M); noise_pred_2b = [uncond ; text]:
 *   eps = u + g (t - u);  x0 = h_x x + h_eps eps;  x <- c_x x + c_eps eps + c_hist hist;  hist <- x0
 * hist_f32 [n] is the scheduler's history (nullable: then c_hist / h_* are ignored).  Coefficients
 * come from the host scheduler (schedulers.py `fused_plan`), replacing scheduler.step at :489. */
int sd_cfg_linear_step(const void* noise_pred_2b, void* latents, float* hist_f32, int64_t n,
                       float guidance_scale, float c_x, float c_eps, float c_hist, float h_x, float h_eps,
                       void* stream);

/* sd_cfg_linear_step with guidance rescale (Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed",
 * section 3.4; rescale_noise_cfg at sd_unified_pipeline.py:46-57).  Per sample b of n_per_sample elements:
 *   eps = fp16(u + g (t - u));  k_b = 1 + guidance_rescale (std(t_b) / std(eps_b) - 1);  eps <- k_b eps
 * and then the update of sd_cfg_linear_step (hist <- h_x x + h_eps k_b eps).  std is the unbiased one over the whole
 * sample; the statistics are fp32 and centred.  std(eps_b) = 0 gives an infinite or NaN k_b, as the reference function
 * does: no epsilon is added.  Two launches, no host synchronisation.  factors_out [B] f32 (device, nullable) receives
 * k_b.  SD_ERR_INVALID: null noise_pred_2b / latents, B < 1, n_per_sample < 2 (nothing is launched). */
int sd_cfg_rescale_linear_step(const void* noise_pred_2b, void* latents, float* hist_f32, int B, int64_t n_per_sample,
                               float guidance_scale, float guidance_rescale, float c_x, float c_eps, float c_hist,
                               float h_x, float h_eps, float* factors_out, void* stream);

/* Perturbed-attention guidance on the device step.  model_out f16 [rows * n] is [uncond ; text ; perturbed] (rows == 3)
 * or [text ; perturbed] (rows == 2); per element, in fp32 with one rounding to f16:
 *   e = fp16(fmaf(s, t - p, fmaf(g, t - u, u)))   (rows == 3; g = guidance_scale, s = pag_scale)
 *   e = fp16(fmaf(s, t - p, t))                   (rows == 2; guidance_scale is not used)
 * (s == 0 skips the outer fmaf: three rows at s = 0 give sd_cfg_linear_step's eps bit for bit.)
 * sd_pag_linear_step: then exactly sd_cfg_linear_step's update on e (x0 = h_x x + h_eps e; x <- c_x x + c_eps e +
 * c_hist hist; hist <- x0; hist_f32 nullable), one launch.  sd_pag_combine: out_f16 [n] <- e, the one-row model output
 * that sd_lcm_step / sd_sched_affine_step then take with rows = 1 (two launches per step).
 * 16-byte accesses when n % 8 == 0 and every pointer is 16-byte aligned, a scalar kernel otherwise.
 * SD_ERR_INVALID (nothing is launched): rows not 2 or 3, n <= 0, a null model_out / latents / out_f16, a non-finite
 * guidance_scale or pag_scale. */
int sd_pag_linear_step(const void* model_out, int rows, void* latents, float* hist_f32, int64_t n, float guidance_scale,
                       float pag_scale, float c_x, float c_eps, float c_hist, float h_x, float h_eps, void* stream);
int sd_pag_combine(const void* model_out, int rows, void* out_f16, int64_t n, float guidance_scale, float pag_scale,
                   void* stream);

/* InstructPix2Pix's dual guidance on the device step.  model_out f16 [3 n] is [text ; image ; uncond] (t: text and image
 * conditioned, i: image only, u: neither); per element, in fp32 with one rounding to f16:
 *   e = fp16(fmaf(g_i, i - u, fmaf(g_t, t - i, u)))   (g_t = guidance_scale, g_i = image_guidance_scale)
 * (an element with i == u skips the outer fmaf, which would add an exact zero: rows [t ; u ; u] give sd_cfg_linear_step's
 * eps on [u ; t] bit for bit, whatever the signs of its zeros.)
 * sd_ip2p_linear_step: then exactly sd_cfg_linear_step's update on e, one launch.  sd_ip2p_combine: out_f16 [n] <- e, the
 * one-row model output that sd_lcm_step / sd_sched_affine_step then take with rows = 1.
 * 16-byte accesses when n % 8 == 0 and every pointer is 16-byte aligned, a scalar kernel otherwise.
 * SD_ERR_INVALID (nothing is launched): n <= 0, a null model_out / latents / out_f16, a non-finite scale. */
int sd_ip2p_linear_step(const void* model_out, void* latents, float* hist_f32, int64_t n, float guidance_scale,
                        float image_guidance_scale, float c_x, float c_eps, float c_hist, float h_x, float h_eps, void* stream);
int sd_ip2p_combine(const void* model_out, void* out_f16, int64_t n, float guidance_scale, float image_guidance_scale,
                    void* stream);

/* One step of a scheduler that adds noise (LCMScheduler.step; schedulers.py `fused_plan`), one launch:
 *   m   = model_out[i]                                   (rows == 1)
 *   m   = fp16(u + g (t - u)), u = out[i], t = out[n+i]  (rows == 2: [uncond ; text], rounded as sd_cfg_linear_step does)
 *   den = d_x x + d_out m;   denoised[i] = fp16(den)     (denoised nullable)
 *   latents[i] = fp16(p_den den + p_noise noise[i])      (noise nullable: the term is absent, p_noise must be 0)
 * x = latents[i]; all tensors f16, n elements (model_out: rows * n).  den and the update are evaluated in fp64 from the
 * f32 coefficients: d_x x and d_out m cancel (|d| ~ 15 on the first of four steps) and f16 resolves 6e-8 around zero,
 * finer than an fp32 evaluation of the two products (the host scheduler.step computes in fp32: the device step is the
 * more exact of the two).  What the fp64 arithmetic costs next to the four f16 streams: DESIGN.md section 4.
 * 16-byte accesses when n % 8 == 0 and every pointer is 16-byte aligned, a scalar kernel otherwise.
 * SD_ERR_INVALID: rows not 1 or 2, n <= 0, null model_out / latents, a null noise with p_noise != 0. */
int sd_lcm_step(const void* model_out, int rows, void* latents, const void* noise, void* denoised, int64_t n,
                float guidance_scale, float d_x, float d_out, float p_den, float p_noise, void* stream);

/* One step of any scheduler whose update is affine in a slightly larger state than sd_cfg_linear_step's: the sample, the
 * model output, fresh noise and up to four fp32 history tensors the scheduler keeps between steps (euler_a, DPM++ 2M SDE,
 * PNDM, UniPC; schedulers.py `affine_plan`).  Per element i, with the operand vector
 *   v = (x, m, z, h_0 .. h_3),   x = latents[i],  z = noise[i],  h_k = bank[k * bank_stride + i],
 *   m = model_out[i] (rows == 1)  or  fp16(u + g (t - u)), u = model_out[i], t = model_out[n + i] (rows == 2, rounded as
 *       sd_cfg_linear_step and sd_lcm_step round it),
 * the step is up to three rows of coefficients, every one evaluated from the OLD values (all loads precede all stores,
 * so a slot may be read and written in one step):
 *   latents[i] <- fp16(out . v);   bank[write_slot[j] * bank_stride + i] <- fp32(write[j] . v),  j < n_writes.
 * The dot products run in fp64 from the float64 coefficients (predictor / corrector rows cancel) and are rounded once.
 * A coefficient that is exactly 0 contributes nothing and an operand whose column is 0 in every used row is not loaded:
 * an unwritten slot may hold anything, and noise may be NULL when its column is 0.  latents and noise f16 [n], model_out
 * f16 [rows * n], bank f32.  One launch, no host synchronisation; 16-byte accesses when n % 8 == 0, every base is 16-byte
 * aligned and bank_stride % 4 == 0, a scalar kernel otherwise.
 * SD_ERR_INVALID (nothing is launched): rows not 1 or 2, n <= 0, null model_out / latents / plan, n_slots outside 0..4,
 * n_writes outside 0..2, a write_slot >= n_slots or repeated, a null bank or bank_stride < n with n_slots > 0, a null noise
 * with a non-zero z coefficient in a used row, a non-finite coefficient in a used row and column (rows: out and the first
 * n_writes of write; columns: x, m, z and the first n_slots slots -- the rest is ignored). */
#define SD_STEP_MAX_SLOTS 4
#define SD_STEP_MAX_WRITES 2
typedef struct sd_step_plan {
    int32_t n_slots;                                             /* 0..4 fp32 history slots */
    int32_t n_writes;                                            /* 0..2 of them are written this step */
    int32_t write_slot[SD_STEP_MAX_WRITES];                      /* distinct, < n_slots */
    double out[3+SD_STEP_MAX_SLOTS];                             /* latents <- fp16(out . v) */
    double write[SD_STEP_MAX_WRITES][3+SD_STEP_MAX_SLOTS];       /* bank[write_slot[j]] <- fp32(write[j] . v) */
} sd_step_plan;
int sd_sched_affine_step(const void* model_out, int rows, void* latents, const void* noise, float* bank,
                         int64_t bank_stride, int64_t n, float guidance_scale, const sd_step_plan* plan, void* stream);

/* Inpainting with a 4-channel UNet, after every scheduler step (sd_unified_pipeline.py:492-506):
 *   latents <- m latents + (1 - m) (a image_latents + b noise),  m = mask [B,1,H,W] f16 over channels;
 * (a, b) = scheduler.add_noise coefficients at the NEXT timestep, or noise = NULL on the last step. */
int sd_inpaint_blend(void* latents, const void* image_latents, const void* noise, const void* mask,
                     float a, float b, int B, int C, int H, int W, void* stream);

/* -- MultiDiffusion (Bar-Tal et al. 2023; diffusers' StableDiffusionPanoramaPipeline): a large latent canvas is denoised
 * as overlapping [h, w] windows ("views") whose model outputs are averaged where they overlap.  View v = iy * nx + ix
 * sits at (ys[iy], xs[ix]); with wrap_x its columns are taken modulo Wc (a 360-degree panorama).  At most 64 starts per
 * axis; they travel in the launch parameters, so ys / xs are HOST arrays.
 *
 * sd_view_plan: the starts of one axis of length L for windows of `win` at `stride`: 0, stride, 2 stride, .. <= L - win,
 * and a final L - win when the last one is not already there, so every position is covered; L <= win gives the single
 * start 0 (the caller's window is then L).  With wrap: 0, stride, .. < L, and win <= L is required.  A stride above win
 * counts as win (the windows abut), so no position is ever left out.  Needs no device.
 * Returns the count (written to starts[0 .. count)), or -SD_ERR_INVALID: non-positive L / win / stride / cap, a null
 * starts, win > L on a wrapped axis, more than 64 starts, cap below the count.
 *
 * sd_views_gather: windows[v * B + b, c, y, x] = canvas[b, c, ys[iy] + y, (xs[ix] + x) mod Wc], a pure f16 copy of
 * canvas [B, C, Hc, Wc] into windows [ny * nx * B, C, h, w].
 *
 * sd_views_merge: eps_out[g * B + b, c, Y, X] = f16(sum_v wt(Y - ys, X - xs) out_{g,v,b}[c, Y - ys, X - xs] / sum_v wt(..))
 * over the views that cover (Y, X), taken in ascending v, fp32 sums, one rounding; no atomics, so the result is
 * deterministic.  window_weights: a DEVICE [h, w] fp32 profile, or NULL for all ones.  Its values must be finite and
 * positive: they live on the device, so this is not checked, and a sum that is zero or not finite gives inf / nan there.
 * model_out holds the UNet outputs of chunks of views_per_chunk views (the last may be smaller), each [G, size, B, C, h, w]:
 * the row of (g, v, b) is (v / vpc) vpc G B + (g size + v % vpc) B + b.  eps_out is [G * B, C, Hc, Wc]: what a forward of
 * the whole canvas would return to the step entries above.
 *
 * Both: SD_ERR_INVALID with nothing launched for a null pointer, a non-positive size, ny or nx outside 1..64, h > Hc or
 * w > Wc, a start outside the canvas (a window that ends outside it, when not wrapped), a pixel that no view covers,
 * views_per_chunk < 1.  One 16-byte access per 8 halves when w, Wc and every x start are multiples of 8 and the device
 * pointers are 16-byte aligned; one element per thread otherwise. */
int sd_view_plan(int L, int win, int stride, int wrap, int* starts, int cap);
int sd_views_gather(const void* canvas, void* windows, int B, int C, int Hc, int Wc, int h, int w, const int* ys, int ny,
                    const int* xs, int nx, int wrap_x, void* stream);
int sd_views_merge(const void* model_out, void* eps_out, const float* window_weights, int G, int B, int C, int Hc, int Wc,
                   int h, int w, const int* ys, int ny, const int* xs, int nx, int wrap_x, int views_per_chunk, void* stream);

/* -- Tiled VAE: replaces diffusers 0.27.2 AutoencoderKL.tiled_decode / tiled_encode / blend_v / blend_h (what
 * `vae.enable_tiling()` switches on; the semantics are recalled, not pinned: DESIGN.md section 8).  A canvas is cut into
 * tiles of `tile_in` whose starts are `stride_in` apart (diffusers' overlap_size = int(tile_in (1 - f))), every tile runs
 * through the unchanged decoder / encoder at its own size -- tiles at the far border are truncated, down to one latent
 * pixel -- and the outputs are cross-faded over `blend` = int(tile_out f) rows / columns in raster order and cropped to
 * `limit` = tile_out - blend.  decode: in = latents, out = image; encode: in = image, out = moments.
 *
 * sd_vae_tile_plan: the plan of one canvas, host only (needs no device).  h, w: the canvas in INPUT space.  Tile k of an
 * axis starts at k stride_in and has size_y[k] / size_x[k] = min(tile_in, L - k stride_in): all full-size but at most the
 * last two, so there are at most 3 x 3 shape classes (diffusers truncates the tile before the last too whenever
 * L < (n - 2) stride_in + tile_in; with one truncated tile per axis there are the four classes interior / last column /
 * last row / corner).  Class c holds the class_ny[c] x class_nx[c] tiles from (class_iy0[c], class_ix0[c]) on, in raster
 * order, each of input shape class_h[c] x class_w[c].
 * SD_ERR_INVALID: a null plan, a non-positive size, tile_overlap_factor outside [0, 0.5], blend > tile_out / 2 (the two
 * bounds the merge's closed form rests on), more than SD_VAE_TILE_MAX_AXIS = 64 tiles on an axis, tile_sample no
 * multiple of tile_latent, and factors for which the crops would not tile the output canvas: it takes
 * int(tile_latent (1 - f)) tile_sample / tile_latent == tile_sample - int(tile_sample f) (likewise for encode, where H
 * and W must also be multiples of the scale); diffusers returns a canvas of another size there.
 *
 * sd_vae_tile_stack: where the merge expects each tile's output: tile_offsets[iy * nx + ix] = the element offset of tile
 * (iy, ix) in the stack, its B images [B, C, th, tw] together (th, tw in OUTPUT space); *total = the stack's elements.
 * The layout is [class][tile in raster order][b]; it is fixed by the plan, so the merge takes no table.
 *
 * sd_vae_decode_tiled / sd_vae_encode_tiled: sd_vae_decode / sd_vae_encode of a canvas by tiles, tile_sample =
 * tile_latent 2^(blocks - 1).  Tiles of one class, of all B images, are stacked (one gather launch per chunk of
 * tile_batch images, 1..32) and run through the plain decode / encode; one merge launch writes the canvas.  The workspace
 * is then the plain call's for one chunk plus the chunk's input and the stack of tile outputs (sd_vae_memory_tiled).
 * sd_vae_encode_range_shift applies to every tile alike.  Debug taps are NOT supported here: while sd_vae_tap is on both
 * return SD_ERR_UNSUPPORTED with nothing launched.  sd_vae_poison_workspace covers the arena as before; the two tile
 * buffers are written in full before they are read.  A canvas of one tile is that tile's plain call plus a copying merge.
 *
 * sd_vae_memory_tiled: sd_vae_memory, plus *tile_bytes = the chunk-input and tile-stack buffers' capacities (0 until a
 * tiled call has run).  sd_vae_memory's own answer keeps its meaning (the arena).
 *
 * Operator entries (test / tool path): sd_op_vae_tiles_gather copies n <= 32 tiles [th, tw] at (ys[i], xs[i]) of image
 * bs[i] of a canvas [., C, Hc, Wc] with row stride ld (HOST arrays: the tile list travels in the launch parameters) into
 * stack [n, C, th, tw]; sd_op_vae_tiles_merge writes canvas [B, C, out_h, out_w] (row stride ld >= out_w) from `tiles`
 * laid out as sd_vae_tile_stack says, stack_elems = the elements `tiles` holds (checked against the plan's).  iters > 0:
 * *ms_per_launch = the mean of that many launches.  SD_ERR_INVALID with nothing launched: a null pointer, a tile outside
 * the canvas, ld below the width, a stack smaller than the plan's.  Both kernels move 16 bytes per thread when widths,
 * starts, strides (and for the merge tile_out, blend, limit) are multiples of 8 and the pointers 16-byte aligned, one
 * element otherwise. */
#define SD_VAE_TILE_MAX_AXIS 64
#define SD_VAE_TILE_MAX_CLASSES 9
#define SD_VAE_TILE_MAX_BATCH 32
typedef struct sd_vae_tiles {
    int32_t ny, nx;                     /* tiles per axis */
    int32_t tile_in, stride_in;         /* input space */
    int32_t tile_out, blend, limit;     /* output space */
    int32_t scale;                      /* tile_sample / tile_latent */
    int32_t in_h, in_w, out_h, out_w;
    int32_t size_y[SD_VAE_TILE_MAX_AXIS], size_x[SD_VAE_TILE_MAX_AXIS];   /* input space */
    int32_t n_classes;
    int32_t class_h[SD_VAE_TILE_MAX_CLASSES], class_w[SD_VAE_TILE_MAX_CLASSES], class_count[SD_VAE_TILE_MAX_CLASSES];
    int32_t class_iy0[SD_VAE_TILE_MAX_CLASSES], class_ny[SD_VAE_TILE_MAX_CLASSES];
    int32_t class_ix0[SD_VAE_TILE_MAX_CLASSES], class_nx[SD_VAE_TILE_MAX_CLASSES];
} sd_vae_tiles;
int sd_vae_tile_plan(int encode, int h, int w, int tile_sample, int tile_latent, double overlap_factor,
                          sd_vae_tiles* plan);
int sd_vae_tile_stack(const sd_vae_tiles* plan, int B, int C, int64_t* tile_offsets, int64_t* total);
int sd_vae_decode_tiled(sd_vae* v, const void* z, void* img, int B, int h, int w, int tile_latent, double overlap_factor,
                        int tile_batch, void* stream);
int sd_vae_encode_tiled(sd_vae* v, const void* img, void* moments, int B, int H, int W, int tile_latent,
                        double overlap_factor, int tile_batch, void* stream);
int sd_vae_memory_tiled(const sd_vae* v, int64_t* weight_bytes, int64_t* workspace_bytes, int64_t* tile_bytes);
int sd_op_vae_tiles_gather(const void* canvas, int64_t ld, void* stack, const int* bs, const int* ys, const int* xs, int n,
                           int B, int C, int Hc, int Wc, int th, int tw, int iters, float* ms_per_launch, void* stream);
int sd_op_vae_tiles_merge(const void* tiles, int64_t stack_elems, void* canvas, int64_t ld, const sd_vae_tiles* plan,
                          int B, int C, int iters, float* ms_per_launch, void* stream);

/* convert_pt_to_numpy (runpod-worker/handler_logic.py:21-29): decoded images [B,C,H,W] f16 in [-1,1] ->
 * [B,H,W,C] uint8, with the reference's fp16 roundings and truncating cast (bit-exact with running
 * the reference's op sequence on the same fp16 tensor).  C <= 4. */
int sd_images_to_uint8(const void* images_nchw_f16, void* out_nhwc_u8, int B, int C, int H, int W, void* stream);

/* -- per-kernel timing for bench.py's live roofline ----------------------------------------- */
/* While enabled, every conv / norm / attention launch of the models is bracketed by HIP events on
 * the launch stream.  sd_prof_collect synchronises and returns one aggregate per kernel name:
 * algorithmic FLOPs and bytes (2*MAC; inputs + weights + outputs once), summed event time. */
typedef struct sd_prof_entry {
    char kernel[64];
    double flops;
    double bytes;
    double ms;
    int64_t launches;
} sd_prof_entry;
int sd_prof_enable(int on);
int sd_prof_collect(sd_prof_entry* out, int max_entries, int* n_entries);

/* Box probe for bench.py (`box_probe`): model-independent microbenchmarks run in-process next to the timed
 * region so that `value` can be read against the box it ran on (the reference has no counterpart; it serves the
 * measurement contract only).  sd_probe_mfma: `iters` rounds of 16 back-to-back v_mfma_f32_16x16x32_f16 per wave,
 * one wave per SIMD on every CU, random operands -> dense fp16 TFLOP/s.  sd_probe_copy: `iters` passes of a
 * 16-byte-per-lane copy of `bytes` (choose > 256 MiB to pass the Infinity Cache) -> GB/s, read + write. */
int sd_probe_mfma(int iters, float* tflops, void* stream);
int sd_probe_copy(int64_t bytes, int iters, float* gbs, void* stream);
/* L2 -> LDS rate of the LDS-DMA path (buffer_load ... lds) with every CU streaming, the operand path of the GEMM kernels:
 * each block (one per CU, four waves) walks `region_bytes` (a multiple of 4096) `passes` times with `depth` 1-KiB pieces
 * outstanding per wave (1, 2, 4, 8, 16 or 32); shared bit 0: all blocks walk the same region (a weight operand), else each its
 * own (an activation operand); shared bit 1: the same walk with ordinary 16-byte loads into registers.  *gbs = aggregate GB/s.  DESIGN.md section 4 reads the GEMM family's ceiling against it. */
int sd_probe_lds_dma(int64_t region_bytes, int passes, int depth, int shared, float* gbs, void* stream);

/* Tuner / test hook: force the LDS-DMA conv kernel's tile variant (an id of the variant table in csrc/igemm2.hip)
 * and split-K factor for every following launch; variant -1 restores the built-in per-shape choice. */
int sd_igemm_force(int variant, int splits);
/* Tuner / test hook, host only (no device needed): how a convolution / linear launch would be planned.
 *   geom[9]   = N, H, W, Cin, Cout, ksize, stride, upsample2x, pad (-1: the kernel size's default)
 *   flags[10] = geglu, act, residual present, row add present, bias present, ln_parts (> 0: LayerNorm folded in, that
 *               many statistics parts per row), row statistics wanted, GroupNorm summaries wanted for that many
 *               groups, GroupNorm of the input fused in with that many groups, scaled epilogue
 *   out[12]   = kind (the variant id that runs, 100: persistent GEGLU, -1: not an LDS-DMA problem), variant (the tile
 *               the choice landed on), split-K slices, split-K workspace in floats, row statistics from the epilogue
 *               (0 / 1), their parts per row, columns per part, GroupNorm summaries from the launch (0 / 1), pixels per
 *               summary, scales honoured (0 / 1), tile rows, tile columns
 *   name[64]  = the kernel's name as rocprofv3 prints it
 * Returns SD_ERR_INVALID with "igemm2: bad variant" when a forced id is not in the table. */
int sd_igemm_plan(const int* geom, const int* flags, int64_t* out, char* name);
/* The 80-column form of the 3x3 halo kernel (conv3x3_halo_kernel<80>), decided ahead of the planner above for the
 * launches whose 128- / 160-column halo grid leaves compute units idle.  Host only (no device needed).
 *   geom, flags  as sd_igemm_plan
 *   cus          the compute-unit count the rule fills; 0: the device's (256 where there is none)
 *   out[6]     = ok (0: the launch stays with sd_igemm_plan's answer), tile columns, split-K slices, GroupNorm summaries
 *                from the launch (0 / 1), pixels per summary, split-K workspace in floats
 *   name[64]   = the profiler row, empty when not ok
 * SD_NO_HALO80=1 in the environment (read once per process) turns the form off.  sd_op_conv2d_ex reports it as kind 80.
 * sd_halo80_force, tests / tools: -1 the rule, 0 never, 1 whenever the kernel takes the problem (any Cout % 8 == 0,
 * split-K until the grid covers the compute units). */
int sd_halo80_plan(const int* geom, const int* flags, int cus, int64_t* out, char* name);
int sd_halo80_force(int mode);
/* The whole decision for a convolution launch, as the engine's graphs take it (conv_plan), host only (no device needed):
 * the folded upsample where upsample2x = 1 and have_fold says a folded pack is at hand (kind 220, sd_upconv_fold_supported
 * and none of GEGLU / activation / row add / residual / LayerNorm fold / fused input GroupNorm / row statistics), then the
 * 80-column halo tile (kind 80, as sd_halo80_plan), then the variant table (as sd_igemm_plan).
 *   geom, flags, out[12], name[64]  as sd_igemm_plan; variant = kind and 256 tile rows for kinds 220 and 80
 *   cus                             as sd_halo80_plan */
int sd_conv_plan(const int* geom, const int* flags, int have_fold, int cus, int64_t* out, char* name);
/* Test entry: sd_op_conv2d (stride 1, dense operands, bias / residual optional) asking the launch for GroupNorm summaries
 * of its output for gn_groups groups.  summaries (device, summaries_floats floats, at least N * max(64, ceil(OH OW / 64))
 * * gn_groups * 2) receives what the launch left: [(n * S + slab) * gn_groups + g][mean, M2] over *rows pixels per slab,
 * S = OH OW / *rows; *rows = 0 when the launch left none.  ran[4] as sd_op_conv2d_ex. */
int sd_op_conv2d_gnstats(const void* x_nhwc, const void* w_oihw, const void* bias, const void* res_nhwc, void* y_nhwc,
                         int N, int H, int W, int Cin, int Cout, int ksize, int gn_groups, float* summaries,
                         int64_t summaries_floats, int* rows, int* ran, void* stream);

/* -- single operators, exported for the parity tests (tests/test_ops_gpu.py) ----------------- */
/* Implicit-GEMM convolution / linear on NHWC f16:
 *   y[n,oh,ow,co] = bias[co] + rowadd[n,co] + res[n,oh,ow,co]
 *                 + sum_{kh,kw,ci} x[n, (oh*stride+kh-pad)>>up, (ow*stride+kw-pad)>>up, ci] * w[co,kh,kw,ci]
 * w is PyTorch [Cout,Cin,KH,KW] (f16, device), bias [Cout] / rowadd [N,Cout] f32 device (nullable);
 * packed per call by the packers a model load uses (the bias stays f32; GEGLU needs ksize 1) and run through the engine's
 * op_conv halves on a private arena (test path only; synchronises). */
int sd_op_conv2d(const void* x_nhwc, const void* w_oihw, const void* bias, const void* rowadd,
                 const void* res_nhwc, void* y_nhwc, int N, int H, int W, int Cin, int Cout,
                 int ksize, int stride, int upsample2x, int geglu, void* stream);
/* sd_op_conv2d with the operands as the engine passes them, for the element-wise kernel tests (tests/test_conv_gpu.py):
 *   ldx, ldres, ldy   row strides in elements of x, res and y: the dense width (Cin; Cout, or Cout / 2 under geglu) or a
 *                     wider multiple of 8, so that an operand can be a column slice of a wider buffer
 *   pad               -1: the kernel size's default (1 for 3x3, 0 for 1x1); 0 with stride 2 is the VAE encoder's
 *                     downsample (right / bottom zero column), output size as in sd_igemm_plan
 *   act               0 none, 1 quick-GELU, 2 erf-GELU after the bias
 *   acc_scale, bias_scale   y = acc_scale * conv + bias_scale * bias (+ rowadd + res), powers of two
 *   gn_groups         > 0: the launch is also asked for the GroupNorm summaries of y for that many groups (ConvFuse::gn_out,
 *                     a buffer dropped on return); a split launch then reduces with splitk_epilogue_gs_kernel
 *   ran[4]            out: kind and tile variant of the plan the launch ran (as sd_igemm_plan's out[0], out[1]), the
 *                     split-K slices the launcher started (at most the planned count), the reduction kernel behind
 *                     them (0 none, 1 splitk_epilogue_kernel, 2 splitk_epilogue_gs_kernel)
 * SD_ERR_INVALID for a bad stride, and for scales or an activation the planned kernel does not take. */
int sd_op_conv2d_ex(const void* x_nhwc, const void* w_oihw, const void* bias, const void* rowadd,
                    const void* res_nhwc, void* y_nhwc, int N, int H, int W, int Cin, int Cout, int ksize,
                    int stride, int upsample2x, int geglu, int64_t ldx, int64_t ldres, int64_t ldy, int pad, int act,
                    float acc_scale, float bias_scale, int gn_groups, int* ran, void* stream);
/* Nearest-2x upsample + 3x3 conv on folded weights: four 2x2 convolutions on the input map, one per output parity
 * (Upsample2D of the UNet up path and the VAE decoder).
 * sd_upconv_fold_supported: 1 when op_conv runs the folded kernel for an [N, H, W, Cin] input (dense) and Cout output
 *   channels: Cin % 64 == 0, Cout % 8 == 0, a 256-pixel patch 64 / 32 / 16 columns wide tiles the H x W input map,
 *   SD_NO_UPCONV_FOLD unset.  Host only.
 * sd_op_fold_upconv: the folded pack of w_oihw [Cout, Cin, 3, 3] f16 into `out` [4][Cout][4 Cin] f16 (device): parity
 *   panel dy * 2 + dx, K order [Cin / 64][a][b][64]; taps summed in fp32 (kernel rows outside, columns inside), rounded
 *   to f16 once.  Built by the packer of a model load (pack_conv with the fold), which folds for Cout % 8 == 0 only:
 *   SD_ERR_UNSUPPORTED otherwise.
 * sd_op_upconv2x_ex: sd_op_conv2d_ex with ksize 3, stride 1, upsample2x 1 and no GEGLU / activation, packed and
 *   dispatched as the models do it (both packs, op_conv's decision).  gn_summaries (optional, with gn_groups > 0):
 *   receives the GroupNorm summaries the launch left, [N][S][gn_groups][2] floats (mean, M2), in a buffer of at least
 *   N * max(64, ceil(4 H W / 64)) * gn_groups * 2 floats.
 *   ran[4] out: 1 when the folded kernel ran (0: the 9-tap path), summaries per image S (0: none left), output pixels
 *   per summary, 0. */
int sd_upconv_fold_supported(int N, int H, int W, int Cin, int Cout);
int sd_op_fold_upconv(const void* w_oihw, void* out, int Cout, int Cin, void* stream);
int sd_op_upconv2x_ex(const void* x_nhwc, const void* w_oihw, const void* bias, const void* rowadd, const void* res_nhwc,
                      void* y_nhwc, int N, int H, int W, int Cin, int Cout, int64_t ldx, int64_t ldres, int64_t ldy,
                      float acc_scale, float bias_scale, int gn_groups, float* gn_summaries, int* ran, void* stream);
/* conv_out: 3x3 / stride 1 / pad 1 convolution to 1..4 output channels (UNet2DConditionModel.conv_out 320 -> 4,
 * AutoencoderKL decoder.conv_out 128 -> 3; diffusers modules under sd_unified_pipeline.py:475-482, :523) with
 * the NHWC -> NCHW change of layout fused: x NHWC f16, w OIHW f16, bias f32, y NCHW f16.  Cin % 64 == 0. */
int sd_op_conv3x3_small_cout(const void* x_nhwc, const void* w_oihw, const void* bias, void* y_nchw, int N, int H,
                             int W, int Cin, int Cout, void* stream);
/* Convolution followed by GroupNorm (+ SiLU) of its output, the pair ResnetBlock2D issues as
 * conv1 -> norm2 and the VAE decoder as conv2 -> next norm1 (diffusers resnet.py under
 * sd_unified_pipeline.py:475-482, :523).  When the launch allows it the convolution's epilogue leaves
 * the GroupNorm statistics and the GroupNorm makes no pass of its own over y_conv;
 * *stats_from_epilogue (may be NULL) tells which path ran.  y_conv and y_gn are both written. */
int sd_op_conv2d_groupnorm(const void* x_nhwc, const void* w_oihw, const void* bias, const void* rowadd,
                           const void* res_nhwc, void* y_conv_nhwc, const void* gamma, const void* beta,
                           void* y_gn_nhwc, int N, int H, int W, int Cin, int Cout, int ksize, int stride,
                           int upsample2x, int groups, float eps, int silu, int* stats_from_epilogue, void* stream);
/* GroupNorm (+ SiLU) followed by a convolution, the pair ResnetBlock2D issues twice (norm1 -> SiLU -> conv1,
 * norm2 -> SiLU -> conv2; diffusers resnet.py under sd_unified_pipeline.py:475-482, :523):
 *   y = conv(act(GroupNorm(x; gamma, beta, groups, eps))) + bias + rowadd + res
 * For 3x3 / stride-1 convolutions the convolution applies the norm to its input tiles in LDS and the normalised
 * tensor never exists in HBM (*fused = 1: op_gn_conv_fused took it; SD_NO_GN_FUSE=1 turns that off); otherwise a
 * GroupNorm kernel runs first (*fused = 0).  iters > 0: timed like sd_bench_conv2d (the statistics pass is outside the
 * timed launches), ms_per_launch written. */
int sd_op_groupnorm_conv2d(const void* x_nhwc, const void* gamma, const void* beta, int groups, float eps, int silu,
                           const void* w_oihw, const void* bias, const void* rowadd, const void* res_nhwc, void* y_nhwc,
                           int N, int H, int W, int Cin, int Cout, int ksize, int iters, float* ms_per_launch, int* fused,
                           void* stream);
/* The two ends of the UNet as one launch each (edge.hip; diffusers UNet2DConditionModel.forward: conv_in, and
 * conv_norm_out -> conv_act -> conv_out, under sd_unified_pipeline.py:475-482).
 * sd_op_unet_conv_in: y_nhwc [N H W, 320] f16 = conv3x3(x_nchw [N, Cin, H, W] f16; w_oihw [320, Cin, 3, 3] f16) + bias (f32),
 *   9 Cin <= 64 and H W % 128 == 0.  groups > 0: gn_summaries [N][H W / 128][groups][2] f32 (device) receives (mean, M2) of
 *   every 128-pixel tile x group of the stored output -- what the first resnet's GroupNorm merges instead of reading y.
 * sd_op_unet_conv_out: y_nchw [N, Cout <= 4, H, W] f16 = conv3x3(act(GroupNorm(x_nhwc [N H W, 320]; gamma, beta, groups, eps));
 *   w_oihw [Cout, 320, 3, 3]) + bias, act = SiLU when silu != 0; H % 8 == 0, W % 16 == 0, groups <= 32.
 * Both return SD_ERR_INVALID for shapes the one-launch kernels do not take (the UNet then runs its general path);
 * iters > 0: timed like sd_bench_conv2d (packing and the statistics pass outside the timed launches). */
int sd_op_unet_conv_in(const void* x_nchw, const void* w_oihw, const void* bias, void* y_nhwc, float* gn_summaries, int groups,
                       int N, int Cin, int H, int W, int Cout, int iters, float* ms_per_launch, void* stream);
int sd_op_unet_conv_out(const void* x_nhwc, const void* gamma, const void* beta, int groups, float eps, int silu,
                        const void* w_oihw, const void* bias, void* y_nchw, int N, int H, int W, int C, int Cout, int iters,
                        float* ms_per_launch, void* stream);
/* sd_op_unet_conv_out with the operands the UNet gives conv_tail_kernel (sd_op_unet_conv_out is this with ldx = C and no
 * summaries): x_nhwc rows ldx >= C halves apart (ldx % 8 == 0; columns from C on are never read); summaries NULL (a
 * statistics pass of its own) or device floats [N][S][groups][2] = (mean, M2) of every tile of `rows` consecutive pixels x
 * group, the last tile holding the remainder, as a producing convolution's epilogue leaves them: the kernel merges them in
 * its prologue.  SD_ERR_INVALID with nothing launched unless (S - 1) rows < H W <= S rows, and for the shapes
 * sd_op_unet_conv_out refuses.  iters / ms_per_launch as sd_op_unet_conv_in (0 / NULL: one launch, not timed). */
int sd_op_unet_conv_out_ex(const void* x_nhwc, int64_t ldx, const void* gamma, const void* beta, int groups, float eps, int silu,
                           const void* w_oihw, const void* bias, void* y_nchw, int N, int H, int W, int C, int Cout,
                           const float* summaries, int S, int64_t rows, int iters, float* ms_per_launch, void* stream);
/* conv_in from two NCHW sources in one launch (edge.hip: conv_head2_kernel), the concatenated sample never built:
 *   y_nhwc[n] = conv3x3(cat(fp16(a[n % Na] * in_scale), n < zero_from ? b[n % Nb] : 0); w_oihw [320, Ca + Cb, 3, 3]) + bias
 * a [Na, Ca, H, W], b [Nb, Cb, H, W] f16; y_nhwc [N H W, 320] with row stride ldy (>= 320, % 8 == 0); b is not read for
 * n >= zero_from.  9 (Ca + Cb) <= 128, N % Na == 0, H W % 128 == 0, Cout == 320; gn_summaries / groups / iters as
 * sd_op_unet_conv_in.  SD_ERR_INVALID with a message for every other shape, and under SD_NO_EDGE_KERNELS. */
int sd_op_unet_conv_in2(const void* a, int Na, int Ca, float in_scale, const void* b, int Nb, int Cb, int zero_from,
                        const void* w_oihw, const void* bias, void* y_nhwc, int64_t ldy, float* gn_summaries, int groups, int N,
                        int H, int W, int Cout, int iters, float* ms_per_launch, void* stream);
/* The GEGLU feed-forward of BasicTransformerBlock with its norm and residual (diffusers attention.py: norm3 -> FeedForward
 * (GEGLU) -> + hidden_states, under sd_unified_pipeline.py:475-482):
 *   y = x + (h * gelu(g)) W2^T + b2,   [h | g] = LayerNorm(x; gamma, beta, eps) W1^T + b1
 * x, y [M, C] f16; w1 [8C, C], w2 [C, 4C] f16 (PyTorch Linear layout); gamma, beta, b1 [8C], b2 [C] f32.  For C = 320 and
 * M % 128 == 0 one launch keeps the 4C-wide hidden tensor on the CU (*fused = 1, ffn.hip); otherwise the projection with
 * its GEGLU epilogue and the output linear with its residual epilogue run (*fused = 0).  iters > 0: ms_per_launch[0] = the
 * path taken, ms_per_launch[1] = the two-GEMM form on the same operands (packing outside the timed launches). */
int sd_op_ffn_geglu(const void* x, const void* ln_gamma, const void* ln_beta, float ln_eps, const void* w1, const void* b1,
                    const void* w2, const void* b2, void* y, int M, int C, int iters, float* ms_per_launch, int* fused,
                    void* stream);
/* The folded LayerNorm of a transformer block (norm1 / norm2 / norm3 folded into the next linear), in two calls that share
 * the row statistics, so each side's kernel can be forced on its own (sd_igemm_force).
 * Producer: y1 = x W0^T + b0 (+ res); x [M, K], res / y1 [M, C] f16, w0 [C, K] f16, b0 [C] f32.  stat (device, at least
 * M * ceil(C / 64) * 2 floats) receives the row statistics the engine's own producer leaves: *parts (mean, M2) pairs per
 * row, part k over the columns [k *part_w, min((k + 1) *part_w, C)).  *producer: the igemm2 variant whose epilogue wrote
 * them (13 = wsgemm, 18 = igemm3), or -1 for the stand-alone row-statistics kernel.
 * Consumer: y2 = LayerNorm(y1; gamma, beta, eps) W1^T + b1 from those statistics.  geglu = 0: w1 [O, C], the first
 * rows_scaled output columns times row_scale (the query scale of q|k|v); geglu = 1: w1 [2 O, C] = [hidden | gate] rows,
 * b1 [2 O], y2 = hidden * gelu(gate) [M, O].  *consumer: the igemm2 variant (13 / 14 = wsgemm, 18 = igemm3) or 100 for
 * the persistent GEGLU kernel.  The consumer takes any layout with parts * part_w >= C > (parts - 1) * part_w (the last
 * part may be narrower) of at most 20 parts per row, what a consumer kernel holds per row; more is SD_ERR_INVALID with
 * nothing launched and y2 untouched. */
int sd_op_linear_rowstats(const void* x, const void* w0, const void* b0, const void* res, void* y1, float* stat, int M,
                          int K, int C, int* parts, int* part_w, int* producer, void* stream);
int sd_op_ln_linear(const void* y1, const float* stat, int parts, int part_w, const void* gamma, const void* beta, float eps,
                    const void* w1, const void* b1, void* y2, int M, int C, int O, int geglu, int rows_scaled, float row_scale,
                    int* consumer, void* stream);
/* sd_op_ffn_geglu on row statistics of x a producer left (the stat / parts / part_w of sd_op_linear_rowstats) instead of
 * statistics it computes itself: the form the UNet runs.  The same layouts as sd_op_ln_linear: at most 20 parts per row,
 * more is SD_ERR_INVALID with nothing launched and y untouched. */
int sd_op_ln_ffn_geglu(const void* x, const float* stat, int parts, int part_w, const void* ln_gamma, const void* ln_beta,
                       float ln_eps, const void* w1, const void* b1, const void* w2, const void* b2, void* y, int M, int C,
                       int* fused, void* stream);
/* Pack-time fold of a linear `outer` (w_outer [O, J] f16, b_outer [O] f32) over the linear `inner` it follows
 * (w_inner [J, K] f16, b_inner [J] f32) with only inner's residual r in between:
 *   outer(inner(g) + r) = [g | r] W'^T + b',   W' = [W_o W_i | W_o]  ([O, K + J]),   b' = W_o b_i + b_o
 * as the engine packs proj_out over the last ff.net.2 of a transformer.  w_folded [O, K + J] f16 (the product accumulated in
 * fp32 and rounded once), b_folded [O] f32; (K + J) % 64 == 0.  The biases are rounded to f16 on the way in, as every
 * weight of a model is. */
int sd_op_fold_linear(const void* w_outer, const void* b_outer, const void* w_inner, const void* b_inner, void* w_folded,
                      float* b_folded, int O, int J, int K, void* stream);
/* The end of a transformer as the UNet runs it (the last block's feed-forward and proj_out):
 *   y = x_in + proj_out(t3 + FF(LayerNorm(t3; gamma, beta, 1e-5)); w_po, b_po),   FF as in the feed-forward entry above
 * x_in, t3, y [M, C] f16 (M rows = imgs images of M / imgs pixels); w1 [8C, C], w2 [C, 4C], w_po [C, C] f16; gamma, beta,
 * b1, b2, b_po f32 (rounded to f16 on the way in, as a model's weights are).  Packed and run by the functions the UNet
 * uses: proj_out folded over ff.net.2 into one GEMM with K = 5C, or -- for C = 320, where ffn.hip can take the
 * feed-forward, and under SD_NO_POUT_FOLD=1 -- the feed-forward followed by proj_out (*fused = 1 when ffn.hip ran).
 * gn_summaries (optional, with gn_rows): the GroupNorm summaries of y for 32 groups that the last launch leaves, (mean, M2)
 * per image, tile of *gn_rows pixels and group: [imgs][M / imgs / *gn_rows][32][2] floats in a buffer of at least
 * imgs * max(64, ceil(M / imgs / 64)) * 64 floats; *gn_rows = 0 when the launch left none. */
int sd_op_ffn_geglu_proj_out(const void* x_in, const void* t3, const void* ln_gamma, const void* ln_beta, float ln_eps,
                             const void* w1, const void* b1, const void* w2, const void* b2, const void* w_po,
                             const void* b_po, void* y, float* gn_summaries, int* gn_rows, int M, int C, int imgs, int* fused,
                             void* stream);
/* Same operator, timed: `iters` back-to-back launches bracketed by HIP events on `stream`
 * (after two warm-up launches); used by tools/tune_igemm.py to pick tile variants per shape.  The launch is planned once,
 * ahead of the loop: a timed launch is launch_igemm2 on that plan, nothing else. */
int sd_bench_conv2d(const void* x_nhwc, const void* w_oihw, void* y_nhwc, int N, int H, int W, int Cin,
                    int Cout, int ksize, int stride, int upsample2x, int geglu, int iters,
                    float* ms_per_launch, void* stream);
/* GroupNorm (+ optional SiLU) on NHWC f16, fp32 statistics. */
int sd_op_groupnorm(const void* x_nhwc, const void* gamma, const void* beta, void* y_nhwc,
                    int N, int HW, int C, int groups, float eps, int silu, void* stream);
/* Test hook, host only (no device needed): what a GroupNorm launch over x [N, HW, C] with `groups` groups would run
 * (launch_groupnorm, launch_gn_stats and this entry decide through one function, norm_plan).  have_summaries = 1: the
 * caller has S_pre (mean, M2) summaries per image, as a producing convolution leaves them.
 *   out[10] = statistics kernel (0 none, 1 gn_stats_kernel, 2 gn_stats2_kernel), apply kernel (0 gn_fused_kernel<T, NV>,
 *             1 gn_apply_kernel, 2 gn_apply2_kernel<NV>), T of the fused kernel (else 0), NV (0 for gn_apply_kernel),
 *             gn_finalize_kernel runs (0 / 1), S = summaries per image the apply pass (or the finalize) merges, pixels
 *             per summary (ceil(HW / S) for the launch's own statistics pass, 0 = the caller's with have_summaries),
 *             CB = channels per block of the statistics and apply2 kernels, scratch floats the launch needs, caller's
 *             summaries used (0 where the single-kernel form runs anyway)
 * S and pixels per summary describe the statistics pass (sd_op_gn_stats) also where out[0] = 0 without summaries.
 * Replaces nothing by itself: the operators are the GroupNorms of ResnetBlock2D, Transformer2DModel and the VAE decoder
 * under sd_unified_pipeline.py:475-482 and :523. */
int sd_norm_plan(int N, int64_t HW, int C, int groups, int have_summaries, int S_pre, int64_t* out);
/* sd_norm_plan (without summaries) for `count` problems: problems[i * 4 + {0..3}] = N, HW, C, groups -> out[i * 10 ..]. */
int sd_norm_plan_batch(int count, const int64_t* problems, int64_t* out);
/* sd_op_groupnorm with the operands as the engine passes them, for the element-wise kernel tests (tests/test_norm_gpu.py;
 * the GroupNorms under sd_unified_pipeline.py:475-482 and :523):
 *   ldx, ldy     row strides in elements: C or a wider multiple of 8 (a column slice of a concatenation buffer)
 *   summaries    NULL, or device floats [N][S][groups][2] = (mean, M2 = sum (x - mean)^2) of each tile of `rows`
 *                consecutive pixels x the group's channels, the last tile holding the remainder: what a convolution's
 *                epilogue leaves.  The launch then makes no statistics pass over x (unless the map is one the
 *                single-kernel form takes, which ignores them).  SD_ERR_INVALID, nothing launched, unless
 *                (S - 1) * rows < HW <= S * rows: an empty summary is never valid.
 *   ran[10]      out: what ran, as sd_norm_plan's out (pixels per summary = `rows` with summaries)
 * Synchronises. */
int sd_op_groupnorm_ex(const void* x_nhwc, int64_t ldx, const void* gamma, const void* beta, void* y_nhwc, int64_t ldy, int N,
                       int64_t HW, int C, int groups, float eps, int silu, const float* summaries, int S, int64_t rows,
                       int64_t* ran, void* stream);
/* The statistics pass alone (what runs ahead of the apply pass, of sd_op_groupnorm_concat's merge and of the GroupNorm
 * fused into a convolution; sd_unified_pipeline.py:475-482): out_host (HOST floats, at least sd_norm_plan's scratch
 * count) receives [N][*S][groups][2] = (mean, M2) per slab of *rows consecutive pixels; *kernel = 1 gn_stats_kernel,
 * 2 gn_stats2_kernel.  Synchronises. */
int sd_op_gn_stats(const void* x_nhwc, int64_t ldx, int N, int64_t HW, int C, int groups, float* out_host, int* S,
                   int64_t* rows, int* kernel, void* stream);
/* GroupNorm of a channel concatenation [A | B] (diffusers' up blocks: torch.cat([hidden_states, res_hidden_states], 1) ->
 * ResnetBlock2D.norm1, under sd_unified_pipeline.py:475-482) from per-half summaries, the way the UNet runs it on its big
 * maps: statistics of the first Ca channels over sub-groups of width gcd(C / groups, Ca), of the last Cb over their own
 * `groups` groups, one small launch merging them per group of the concatenation, then the apply pass.  x, y [N HW, Ca + Cb]
 * f16.  SD_ERR_INVALID when the halves' sub-groups cannot tile the groups (the UNet then runs an ordinary statistics pass). */
int sd_op_groupnorm_concat(const void* x_nhwc, int Ca, int Cb, const void* gamma, const void* beta, void* y_nhwc, int N, int HW,
                           int groups, float eps, int silu, void* stream);
/* Same operator, timed like sd_bench_conv2d (scratch allocated once, `iters` launches between HIP events). */
int sd_bench_groupnorm(const void* x_nhwc, const void* gamma, const void* beta, void* y_nhwc,
                       int N, int HW, int C, int groups, float eps, int silu, int iters,
                       float* ms_per_launch, void* stream);
/* Timesteps / get_timestep_embedding as UNet2DConditionModel.time_proj and SDXL's add_time_proj issue it
 * (diffusers embeddings.py under sd_unified_pipeline.py:475-482): out[b, :] = [cos(t_b f_i) | sin(t_b f_i)]
 * (flip_sin_to_cos = 1) or [sin | cos], f_i = exp(-ln(1e4) i / (dim/2 - freq_shift)).  t, out: f32 device. */
int sd_op_timestep_sinusoid(const float* t, float* out, int count, int dim, int flip_sin_to_cos, float freq_shift,
                            void* stream);
/* The input of add_embedding.linear_1 (text_time conditioning), one launch:
 *   out[b, :P]             = f32(add_text[b, :])
 *   out[b, P + j*ad + i]   = sd_op_timestep_sinusoid(ids[b, j], dim = ad)[i]      j < n_ids
 * add_text [B,P] f16, ids [B,n_ids] f32, out [B, P + n_ids*ad] f32 (all device).  The sinusoid is the device function
 * sd_op_timestep_sinusoid runs: the bits are equal.  SD_ERR_INVALID (nothing is launched): n_ids outside 1..8, odd or
 * non-positive ad, P <= 0, B < 1, a NULL pointer. */
int sd_op_text_time_input(const void* add_text, const float* ids, float* out, int B, int P, int ad, int n_ids,
                          int flip_sin_to_cos, float freq_shift, void* stream);
/* The input of a guidance-embedded UNet's time embedding (TimestepEmbedding with cond_proj_dim), one launch:
 *   out[b, j] = sinusoid(t_b)[j] + sum_k W[j, k] cond[b, k]
 * t [B], cond [B, cond_dim], out [B, dim] f32; w_f16 [dim, cond_dim] f16 row-major (no bias); fp32 accumulation, the sum
 * added last: cond = 0 gives sd_op_timestep_sinusoid's bits.  dim even, 1 <= cond_dim <= 1024 (SD_ERR_INVALID). */
int sd_op_timestep_cond_embedding(const float* t, const float* cond, const void* w_f16, float* out, int B, int dim,
                                  int cond_dim, int flip_sin_to_cos, float freq_shift, void* stream);
/* The small-batch linear of the time-embedding MLPs (TimestepEmbedding.linear_1 / linear_2, time_emb_proj):
 * y[b, n] = act_out(bias[n] + sum_k act_in(x[b, k]) * W[n, k]), act = SiLU when the flag is set.  x, bias, y f32,
 * W f16 row-major [n_out, k]. */
int sd_op_small_linear(const float* x, const void* w_f16, const float* bias, float* y, int B, int K, int n_out,
                       int silu_in, int silu_out, void* stream);
/* Which kernel sd_op_small_linear (and every launch of the time-embedding path) runs for [B, K] x [n_out, K]^T, decided
 * on the host by the function the launcher itself asks: 1 skinny_linear_kernel (MFMA; B <= 16, K % 32 == 0, K <= 1280,
 * n_out % 16 == 0), 0 small_linear_kernel (GEMV), -1 refused (K % 8 != 0, or an argument below 1).  No device needed. */
int sd_small_linear_plan(int B, int K, int n_out);
/* diffusers 0.27.2 apply_freeu on one concatenation cat_nhwc [N, H, W, C1 + C2] f16, in place:
 *   cat[..., :C1 / 2] *= b;   cat[..., C1:] = fourier_filter(cat[..., C1:], threshold = 1, scale = s) over (H, W)
 * i.e. the skip's frequencies {-1, 0} x {-1, 0} times s and the real part kept, computed in closed form from seven fp32
 * moments per (image, channel) plane and rounded to f16 once; cat[..., C1 / 2 : C1] is not touched.  C1 even, C2 >= 1,
 * finite factors (SD_ERR_INVALID otherwise); H + W <= 4096 (SD_ERR_UNSUPPORTED beyond). */
int sd_op_freeu(void* cat_nhwc, int N, int H, int W, int C1, int C2, float b, float s, void* stream);
/* Token merging, operator by operator (tomesd's bipartite_soft_matching_random2d; sd_unet_set_tome).  An H x W map of
 * T = H W tokens is cut into sy x sx cells; with hsy = H / sy, wsx = W / sx, cell = cy wsx + cx draws
 *   k = use_rand ? mix32(seed, step, site, cell) % (sx sy) : 0,   in uint32 arithmetic
 *   h = seed ^ step 0x9E3779B9 ^ site 0x85EBCA6B ^ cell 0xC2B2AE35;
 *   h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16
 * and its destination token is (cy sy + k / sx, cx sx + k % sx); every other token, the rows and columns past the whole
 * cells included, is a source: Nd = hsy wsx, Ns = T - Nd.  The draw is shared by all images.  r = min(Ns, int(T ratio))
 * sources merge.  Ranks are raster order within each set.  With s[i, j] = <x_i, x_j> / (|x_i| |x_j|) (0 for a zero row),
 * node_max_i = max_j s[i, j] and node_idx_i the lowest destination rank that attains it, the r sources of largest
 * node_max merge (ties to the lower source rank).  The merged sequence has T' = T - r rows: the unmerged sources in
 * source-rank order, then the destinations in destination-rank order, a destination row being the mean over itself
 * and the sources merged into it.  map[t] in [0, T') is the merged row token t reads back.
 *
 * sd_tome_plan: info4 = (Nd, Ns, r, T') and, when dst_tok is non-NULL, the Nd destination tokens in rank order.  Needs
 * no device.  sd_tome_plan_bytes: the size of the opaque plan buffer (device memory) for B images of T tokens.
 *
 * sd_op_tome_match: x [B, H W, C] f16 with row stride ldx (ldx % 8 == 0, C % 32 == 0, 16-byte aligned) -> plan, in
 * three launches: fp32 reciprocal norms and the rank tables; x_src x_dst^T on fp16 MFMAs with fp32 accumulation over
 * all of C, scaled by the two reciprocal norms afterwards, with a running (max, lowest argmax) per source (the scores
 * are never stored); one block per image that selects the r largest by a radix select of the order-preserving bit
 * pattern, compacts the unmerged ranks by a prefix sum and lists every merged row's members in ascending token index.
 * No global atomics: the result is reproducible bit for bit.  map_out [B, T] int32, node_max [B, Ns] f32 and
 * node_idx [B, Ns] int32 (DEVICE, each nullable) receive copies.  SD_ERR_INVALID: bad arguments, r = 0;
 * SD_ERR_UNSUPPORTED, nothing launched: T > 16384, Nd = 0.
 *
 * sd_op_tome_plan_from_map: a plan from a caller's map_host [B, T] (HOST) onto T_merged rows, so that merge / unmerge
 * can be driven with any grouping; every row of [0, T_merged) needs a member.  Synchronises the stream.
 *
 * sd_op_tome_merge: dst [B T', ldd] <- per merged row the mean of its member rows of src [B T, lds] over `cols` columns:
 * f16 in, fp32 sum in ascending token index, one IEEE divide by the member count, one rounding to f16.
 * sd_op_tome_unmerge: dst [B T, ldd] row t <- src [B T', lds] row map[t], a pure copy.  Both use 16-byte accesses when
 * cols, both row strides and both pointers allow and one element per thread otherwise, and touch nothing outside the
 * `cols` columns or beyond the last row.  The plan is device memory the host does not read: a buffer that holds no plan
 * for this T and at least B images (its header says) makes both launches write nothing, and they still return SD_OK. */
int sd_tome_plan(int H, int W, int sx, int sy, double ratio, int use_rand, uint32_t seed, uint32_t step, uint32_t site,
                 int32_t* info4, int32_t* dst_tok);
int64_t sd_tome_plan_bytes(int B, int T);
int sd_op_tome_match(const void* x, int64_t ldx, int B, int H, int W, int C, int sx, int sy, double ratio, int use_rand,
                     uint32_t seed, uint32_t step, uint32_t site, void* plan, int32_t* map_out, float* node_max,
                     int32_t* node_idx, void* stream);
int sd_op_tome_plan_from_map(const int32_t* map_host, int B, int T, int T_merged, void* plan, void* stream);
int sd_op_tome_merge(const void* src, int64_t lds, int cols, const void* plan, int B, int T, void* dst, int64_t ldd,
                     void* stream);
int sd_op_tome_unmerge(const void* src, int64_t lds, int cols, const void* plan, int B, int T, void* dst, int64_t ldd,
                       void* stream);
/* HyperTile, operator by operator (sd_unet_set_hypertile).  One axis of n tokens has the candidate tile extents
 *   extents = the first swap_size divisors e of n with e >= min(tile_size, n), ascending;  counts[i] = n / extents[i]
 * (most tiles first; never empty, e = n divides), and a site draws
 *   nh = counts_h[mix32(seed, step, site, 0) % len(counts_h)],  nw = counts_w[mix32(seed, step, site, 1) % len(counts_w)]
 * with token merging's mix32 (above).  sd_hypertile_plan: out4 = (nh, nw, th, tw) with th = Hs / nh, tw = Ws / nw.  Needs
 * no device.  SD_ERR_INVALID: Hs, Ws or tile_size < 1, Hs Ws > 2^24, swap_size outside 1..8, a null out4.
 *
 * sd_op_hypertile_gather: all images and tiles of src [B Hs Ws, lds] f16 in one launch,
 *   dst row ((b nh + ty) nw + tx) th tw + y tw + x  <-  src row (b Hs + ty th + y) Ws + tx tw + x,  columns [0, cols),
 * a pure copy with 16 bytes per lane.  sd_op_hypertile_scatter: the inverse map (src in tile order, dst in raster
 * order).  Neither writes a column of dst past `cols` or a row past B Hs Ws.  SD_ERR_INVALID with nothing launched
 * unless cols % 8 == 0, both row strides % 8 == 0 and >= cols, both pointers 16-byte aligned, Hs % nh == 0,
 * Ws % nw == 0 and B, nh, nw >= 1. */
int sd_hypertile_plan(int Hs, int Ws, int tile_size, int swap_size, uint32_t seed, uint32_t step, uint32_t site, int32_t* out4);
int sd_op_hypertile_gather(const void* src, int64_t lds, int cols, int B, int Hs, int Ws, int nh, int nw, void* dst, int64_t ldd,
                           void* stream);
int sd_op_hypertile_scatter(const void* src, int64_t lds, int cols, int B, int Hs, int Ws, int nh, int nw, void* dst, int64_t ldd,
                            void* stream);
/* Temporal self-attention of an AnimateDiff motion module (diffusers 0.27.2 TransformerTemporalModel, recalled): every
 * pixel p of every video v attends over its own F frames, in one launch and without a permuted copy on either side.
 * Frame f of the pixel is row (v F + f) HW + p of q, k, v and out (f16, their own row strides: q | k | v are read where the
 * row-wise q|k|v GEMM left them), heads split the columns [h d, (h + 1) d):
 *   out_f = sum_g softmax_g(s (q_f + bias[f, 0:C])(k_g + bias[g, C:2C])^T) (v_g + bias[g, 2C:3C]),   C = heads d,
 * s = 1 / sqrt(d), or 1 with prescaled != 0 (q and its bias already carry log2(e) / sqrt(d), as the UNet's packed query
 * projections do; the exponential is then base 2).  bias [>= F, ldb] f32 is the position term of sd_op_motion_pos_bias,
 * added in fp32 before the operand is rounded to f16; NULL: none.  The softmax is exact over the F keys (one pass, no
 * running maximum); probabilities are rounded to nearest f16 and normalised by the sum of the rounded values, fp32
 * accumulation, f16 store.  F = 1 returns f16(v + bias) bit for bit.  Nothing is read or written outside the V F HW rows
 * and the heads d (3 heads d for the table) columns.
 * 1 <= F <= 32, d in {32, 40, 64, 80, 160}: otherwise SD_ERR_UNSUPPORTED.  SD_ERR_INVALID: row strides not multiples of 8
 * or below heads d, ldb not a multiple of 4 or below 3 heads d, pointers not 16-byte aligned, V F HW >= 2^31.
 * sd_temporal_attention_plan names what runs for a shape, out7 = (head dim, 16-frame tiles per axis, pixels per block,
 * waves per block, contraction of the PV MFMA: 16 = 16x16x16 / 32 = 16x16x32, LDS bytes per block, blocks); the launch
 * dispatches on the same function.  Needs no device.
 * sd_op_motion_pos_bias: out[f, n] = (n < scale_rows ? scale : 1) sum_c pe[f, c] w[n, c] for f < F, n < N, with
 * pe[f, 2i] = sin(f 10000^(-2i/C)), pe[f, 2i+1] = cos(same) and w [N, C] f16 a projection weight BEFORE any LayerNorm
 * fold: (LN(h) + pe_f) W^T = LN(h) W^T + pe_f W^T.  float64 inside, one rounding to f32.  C % 8 == 0, C <= 4096. */
int sd_temporal_attention_plan(int V, int F, int HW, int heads, int d, int64_t* out7);
int sd_op_temporal_attention(const void* q, const void* k, const void* v, void* out, const float* bias, int64_t ldq, int64_t ldk,
                             int64_t ldv, int64_t ldo, int64_t ldb, int V, int F, int HW, int heads, int d, int prescaled,
                             void* stream);
int sd_op_motion_pos_bias(const void* w, int N, int C, int F, float scale, int scale_rows, float* out, int64_t ldo, void* stream);
/* LayerNorm over the last dim of [rows, C] f16. */
int sd_op_layernorm(const void* x, const void* gamma, const void* beta, void* y, int rows, int C,
                    float eps, void* stream);
/* The same with row strides in elements (C or a wider multiple of 8): the LayerNorms of BasicTransformerBlock and CLIP
 * under sd_unified_pipeline.py:475-482.  SD_ERR_INVALID for C % 8 != 0 or C > 2048. */
int sd_op_layernorm_ex(const void* x, int64_t ldx, const void* gamma, const void* beta, void* y, int64_t ldy, int64_t rows,
                       int C, float eps, void* stream);
/* Per-row LayerNorm statistics of x [rows, C] f16 (row stride ldx): stat[row * 2 + {0,1}] = (mean, M2 = sum (x - mean)^2),
 * device floats; the stand-alone producer for the LayerNorm folded into a linear layer (BasicTransformerBlock.norm1-3,
 * sd_unified_pipeline.py:475-482) where the producing GEMM could not emit them.  C a multiple of 8. */
int sd_op_row_stats(const void* x, int64_t ldx, float* stat, int64_t rows, int C, void* stream);
/* softmax(q k^T / sqrt(d)) v.  q [B,Tq,heads*d] (row stride ldq), k/v [B,Tk,heads*d], out like q. */
int sd_op_attention(const void* q, const void* k, const void* v, void* out, int B, int Tq, int Tk,
                    int heads, int d, int ldq, int ldk, int ldv, int ldo, void* stream);
/* The same with options.  causal = 1: key j > query i contributes nothing (CLIP text self-attention).
 * prescaled = 1: q already carries log2(e)/sqrt(d) (the UNet folds it into its query projections),
 * the kernel then skips its per-score scaling. */
int sd_op_attention_ex(const void* q, const void* k, const void* v, void* out, int B, int Tq, int Tk,
                       int heads, int d, int ldq, int ldk, int ldv, int ldo, int causal, int prescaled,
                       void* stream);
/* Test hook, host only (no device needed): which instantiation of the attention kernel sd_op_attention_ex would launch
 * for this problem (the launch dispatches on the same function).  out5 = head dim, 16-query subtiles per wave, keys per
 * tile, accumulator-start form for pre-scaled queries (0 / 1), waves per block; a block holds 16 * out5[1] * out5[4]
 * queries.  SD_ERR_UNSUPPORTED for a head dim the launch rejects.  The SD_ATTN_NWV / SD_ATTN_NWV80 switches are read
 * once per process, as by the launch. */
int sd_attention_plan(int B, int Tq, int Tk, int heads, int d, int causal, int prescaled, int* out5);
/* IP-Adapter's decoupled cross-attention (diffusers IPAdapterAttnProcessor2_0 at every attn2), one launch:
 *   out = softmax(s q k^T) v + ip_scale * softmax(s q k_ip^T) v_ip,   s = 1/sqrt(d), or 1 with prescaled = 1
 * q [B,Tq,heads*d], k / v [B,L,heads*d], k_ip / v_ip [B,T_ip,heads*d], out like q, each with its own row stride
 * (multiples of 8).  d in {32, 40, 64, 80, 160}, 1 <= L <= 160, 1 <= T_ip <= 64 (SD_ERR_UNSUPPORTED otherwise);
 * ip_scale = 0 gives the text attention alone.  iters > 0 (timing; synchronises): ms_per_launch[0..2] = the fused
 * kernel, the text-only attention launch of sd_op_attention_ex on the same operands, and the unfused composition
 * (text attention + image attention + add), `iters` back-to-back launches each between HIP events. */
int sd_op_ip_cross_attention(const void* q, const void* k, const void* v, const void* k_ip, const void* v_ip, void* out,
                             int B, int Tq, int L, int T_ip, int heads, int d, int ldq, int ldk, int ldv, int ldk_ip,
                             int ldv_ip, int ldo, float ip_scale, int prescaled, int iters, float* ms_per_launch,
                             void* stream);
/* Test hook, host only (no device needed): the shape of that launch (which takes its grid and LDS size from the same
 * function).  out4 = query rows per block tile, tiles per (batch, head), blocks per (batch, head), bytes of dynamic LDS.
 * With fewer blocks than tiles a block walks the tiles b, b + blocks, ... against the K / V it staged once.  The same
 * codes as the launch for L, T_ip and d out of range and for a NaN ip_scale; all counts 0 for an empty problem. */
int sd_ip_attention_plan(int B, int Tq, int L, int T_ip, int heads, int d, float ip_scale, int* out4);
/* Regional cross-attention (sd_unet_set_regions), one launch:
 *   out[n, t] = sum_r w[n % Bw, t, r] softmax(s q[n, t] k[n, rL:(r+1)L]^T) v[n, rL:(r+1)L],   s = 1/sqrt(d), or 1 with
 * prescaled = 1.  q / out [B,Tq,heads*d], k / v [B,R L,heads*d], each with its own row stride (multiples of 8);
 * w [Bw,Tq,R] fp32, Bw divides B.  Each segment's softmax is exact; a wave skips a segment that is zero for all 16
 * queries of its tile, and a query whose weight is zero inside a running segment adds an exact zero.  d in
 * {32, 40, 64, 80, 160}, 1 <= R <= 8, 1 <= L <= 160 (SD_ERR_UNSUPPORTED otherwise, nothing launched); SD_ERR_INVALID for a
 * null pointer, a stride that is no multiple of 8, Bw < 1 or B % Bw != 0. */
int sd_op_region_cross_attention(const void* q, const void* k, const void* v, const float* w, void* out, int B, int Tq, int L,
                                 int R, int heads, int d, int ldq, int ldk, int ldv, int ldo, int Bw, int prescaled,
                                 void* stream);
/* Host only (no device needed): how that launch holds the R segments in its 160 KiB of LDS.  out4 = segments per group,
 * groups, bytes of dynamic LDS, query tiles per block.  One group: every segment is resident and a block of four waves
 * walks its share of the 64-query tiles against them (out4[3] = 0: as many as its share).  More: one 128-query tile
 * per block of eight waves (out4[3] = 1), K / V restaged between groups while the output stays in registers.  SD_ERR_UNSUPPORTED for d, R or L
 * outside the launch's. */
int sd_region_plan(int R, int L, int d, int* out4);
/* The per-level weights of sd_unet_set_regions from weights [Bw,R,H,W] fp32, one launch: level l = 0..levels-1 of `out`
 * is [Bw, (H >> l)(W >> l), R] fp32 -- level 0 the input transposed, level l the 2x2 mean of level l - 1 -- back to
 * back.  1 <= levels <= 4, H and W divisible by 2^(levels-1), 1 <= R <= 8 (SD_ERR_INVALID otherwise). */
int sd_op_region_pyramid(const float* weights, float* out, int Bw, int R, int H, int W, int levels, void* stream);
/* The Resampler's perceiver attention (IP-Adapter Plus), one launch, head dim 64:
 *   out = softmax(s q [k_x ; k_l]^T) [v_x ; v_l],   s = 1/8, or 1 with prescaled = 1
 * q / out [B,n_q,heads*64], k_x / v_x [B,T_feat,heads*64] (the projected image features), k_l / v_l [B,n_q,heads*64]
 * (the projected latents), each with its own row stride (multiples of 8; operands 16-byte aligned).  One softmax over
 * both key segments.  1 <= n_q <= 16, T_feat >= 1, T_feat + n_q <= 320 (SD_ERR_UNSUPPORTED otherwise).  iters > 0
 * (timing; synchronises): ms_per_launch[0..1] = this kernel, and the composed form -- two strided copies that build a
 * concatenated [B, T_feat + n_q, 2 heads 64] K|V buffer, then sd_op_attention_ex on it -- `iters` back-to-back
 * repetitions each between HIP events. */
int sd_op_resampler_attention(const void* q, const void* k_x, const void* v_x, const void* k_l, const void* v_l, void* out,
                              int B, int n_q, int T_feat, int heads, int ldq, int ldk_x, int ldv_x, int ldk_l, int ldv_l,
                              int ldo, int prescaled, int iters, float* ms_per_launch, void* stream);

/* ControlNet zero-convs: for every problem, y[m, :C] = fp16(y[m, :C] + scale (x[m, :] w^T + bias)) in place; the
 * columns of y past C (row stride ldy) are left alone.  x [M, C] f16 (ldx % 8 == 0), w [C, C] f16 (row = output
 * channel), bias [C] f32, C % 64 == 0, 1 <= count <= 16; x, w and bias 16-byte aligned, y 8-byte aligned
 * (SD_ERR_UNSUPPORTED otherwise).
 *   mode 0: one grouped launch (cn_residual_kernel);  mode 1: one GEMM launch per problem with the residual and the
 *   scale in its epilogue (the form the UNet forward issues).
 * iters > 0 (timing; synchronises): *ms_per_launch = one application of the mode's launches, averaged over `iters`
 * back-to-back repetitions (y then holds the sum of all of them). */
typedef struct sd_cn_problem {
    const void* x; int64_t ldx;
    const void* w;
    const float* bias;
    void* y; int64_t ldy;
    int M, C;
} sd_cn_problem;
int sd_op_controlnet_residuals(const sd_cn_problem* problems, int count, float scale, int mode, int iters,
                               float* ms_per_launch, void* stream);
/* The MultiControlNet fold alone: w[i] [C, C] f16 and bias[i] [C] f32 (DEVICE pointers in HOST arrays of n entries),
 * scales [n] (host) -> w_cat [C, n C] f16 with w_cat[o, i C + k] = fp16(float(w_i[o, k]) * scales[i]) and b_cat [C] f32 =
 * sum_i scales[i] bias_i in fp32, net order.  Packed as the forward packs a zero-conv and folded by the launch the
 * forward issues.  1 <= n <= 4, C % 64 == 0 (SD_ERR_INVALID); outputs 16-byte aligned.  iters > 0 times the fold launch. */
int sd_op_cn_fold_scales(const void* const* w, const float* const* bias, const float* scales, int n, int C, void* w_cat,
                         float* b_cat, int iters, float* ms_per_launch, void* stream);
/* The residual stage of n ControlNets: for every problem y[m, :C] += sum_i scales[i] (x_i[m, :] w_i^T + bias_i) in place
 * (y's columns past C are left alone).
 *   mode 0: chained, one GEMM per net with its scale and the residual in the epilogue (a net at scale 0 is skipped);
 *   mode 1: the weights folded by one grouped launch (sd_op_cn_fold_scales' kernel), then one GEMM with K = n C per
 *           problem; the sources must be neighbouring column slices of one buffer (x[i] = x[0] + i C, equal ldx).
 * C % 64 == 0, 1 <= count <= 16, 1 <= n <= 4, x 16-byte aligned with ldx % 8 == 0 (SD_ERR_INVALID).  iters > 0
 * (timing; synchronises): ms_per_launch[0] = one application of the mode's GEMMs, and in mode 1 ms_per_launch[1] = the
 * grouped fold launch over all problems (ms_per_launch holds two floats). */
typedef struct sd_cn_multi_problem {
    const void* x[SD_MAX_CONTROLNETS]; int64_t ldx[SD_MAX_CONTROLNETS];
    const void* w[SD_MAX_CONTROLNETS];
    const float* bias[SD_MAX_CONTROLNETS];
    void* y; int64_t ldy;
    int M, C;
} sd_cn_multi_problem;
int sd_op_controlnet_residuals_multi(const sd_cn_multi_problem* problems, int count, const float* scales, int n, int mode,
                                     int iters, float* ms_per_launch, void* stream);
/* The ControlNet's conditioning embedding: image [n,3,8H,8W] f16 -> out [n,H,W,block_out_channels[0]] f16 (NHWC).
 * iters > 0 (timing; synchronises): *ms_per_launch = one embedding, averaged over `iters` runs. */
int sd_op_controlnet_cond_embed(sd_controlnet* cn, const void* image, int n, int H, int W, void* out, int iters,
                                float* ms_per_launch, void* stream);
/* One layer of that embedding alone: y = act(conv3x3(x, w) + bias), pad 1, stride 1 or 2, act = SiLU (silu = 1) or the
 * identity.  x [N,3,IH,IW] f16 NCHW with Cin = 3 (nchw = 1, the control image) or [N,IH,IW,Cin] f16 NHWC with Cin in
 * {16, 32, 96} (nchw = 0); w [Cout,Cin,3,3] f16, bias [Cout] f16, Cout % 16 == 0; y [N,OH,OW,Cout] f16 NHWC with
 * OH = (IH - 1) / stride + 1, OW likewise.  The weights and the bias are packed by the launches a ControlNet's
 * finalisation uses.  SD_ERR_UNSUPPORTED for any other layer (nothing is written). */
int sd_op_cn_cond_conv(const void* x, int nchw, const void* w_oihw_f16, const void* bias_f16, int N, int IH, int IW, int Cin,
                       int Cout, int stride, int silu, void* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SD_ENGINE_H */
