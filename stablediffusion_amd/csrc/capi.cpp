// extern "C" surface of libsd_engine.so -- see include/sd_engine.h for the contract and for the
// reference interfaces (file:line) each entry point replaces.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <new>

#include "model.h"
#include <cstdlib>

using namespace sd;

struct sd_unet { UNet impl; explicit sd_unet(const sd_unet_config& c) : impl(c) {} };
struct sd_vae { VAE impl; explicit sd_vae(const sd_vae_config& c) : impl(c) {} };
struct sd_clip { CLIP impl; explicit sd_clip(const sd_clip_config& c) : impl(c) {} };
struct sd_clip_vision { CLIPVision impl; explicit sd_clip_vision(const sd_clip_vision_config& c) : impl(c) {} };
struct sd_controlnet {
    ControlNet impl;
    sd_controlnet(const sd_unet_config& c, int cc) : impl(c, cc) {}
};
struct sd_motion {
    MotionAdapter impl;
    explicit sd_motion(const sd_motion_config& c) : impl(c) {}
};
struct sd_ip_adapter {
    IPAdapter impl;
    sd_ip_adapter(const sd_unet_config& c, const sd_ip_projection_config& p) : impl(c, p) {}
    ~sd_ip_adapter() { if (impl.attached) impl.attached->set_ip_adapter(nullptr); }
};

namespace {

int weight_info(const WeightStore& ws, int index, const char** key, int64_t* shape4, int* ndim) {
    if (index < 0 || index >= (int)ws.order.size()) { set_error("weight index out of range"); return SD_ERR_INVALID; }
    const std::string& k = ws.order[(size_t)index];
    const RawTensor& t = ws.tensors.at(k);
    *key = k.c_str();
    *ndim = (int)t.shape.size();
    for (int i = 0; i < 4; ++i) shape4[i] = i < *ndim ? t.shape[(size_t)i] : 1;
    return SD_OK;
}

bool bad_cfg(const sd_unet_config* c) {
    if (!c || c->num_blocks < 1 || c->num_blocks > SD_MAX_BLOCKS) return true;
    for (int i = 0; i < c->num_blocks; ++i) {
        if (c->block_out_channels[i] % 64 != 0 || c->block_out_channels[i] % c->norm_num_groups != 0) return true;
        if (c->num_heads[i] <= 0 || c->block_out_channels[i] % c->num_heads[i] != 0) return true;
        if ((c->down_block_has_attn[i] || c->up_block_has_attn[c->num_blocks - 1 - i]) &&
            !attention_supported(c->block_out_channels[i] / c->num_heads[i])) return true;
    }
    if (c->addition_time_embed_dim > 0) {
        // text_time conditioning: add_embedding.linear_1 reads [pooled text | n sinusoids of `ad`] rows of
        // projection_class_embeddings_input_dim halves with 16-byte loads against weight rows packed to a
        // multiple of 64 (UNet::run): anything else reads misaligned / wrong rows silently
        const int ad = c->addition_time_embed_dim, pin = c->projection_class_embeddings_input_dim;
        const int n = c->num_time_ids ? c->num_time_ids : 6;          // (0: a zero-initialised caller's SDXL base)
        // (six ids: the row is assembled at its own width, so it must be the packed K itself; any other count is
        //  built by one launch that pads the row to the packed K with zeros, and pin % 8 is enough)
        if (n < 1 || n > 8 || (ad & 1) || pin % (n == 6 ? 64 : 8) != 0 || pin - n * ad <= 0) return true;
    }
    return c->cross_attention_dim % 64 != 0 || c->in_channels <= 0 || c->in_channels > 16;
}

// columns of add_time_ids a configuration asks for (0 in the struct: 6); only read with text_time conditioning
int time_ids_of(const sd_unet_config& c) { return c.addition_time_embed_dim > 0 ? (c.num_time_ids ? c.num_time_ids : 6) : 0; }

// field by field (no padding bytes compared): the configuration an IP-Adapter was created for
bool same_topology(const sd_unet_config& a, const sd_unet_config& b) {
    if (a.in_channels != b.in_channels || a.out_channels != b.out_channels || a.num_blocks != b.num_blocks ||
        a.layers_per_block != b.layers_per_block || a.cross_attention_dim != b.cross_attention_dim ||
        a.use_linear_projection != b.use_linear_projection || a.norm_num_groups != b.norm_num_groups ||
        a.norm_eps != b.norm_eps || a.flip_sin_to_cos != b.flip_sin_to_cos || a.freq_shift != b.freq_shift ||
        a.addition_time_embed_dim != b.addition_time_embed_dim ||
        a.projection_class_embeddings_input_dim != b.projection_class_embeddings_input_dim ||
        time_ids_of(a) != time_ids_of(b))
        return false;
    for (int i = 0; i < SD_MAX_BLOCKS; ++i)
        if (a.block_out_channels[i] != b.block_out_channels[i] || a.down_block_has_attn[i] != b.down_block_has_attn[i] ||
            a.up_block_has_attn[i] != b.up_block_has_attn[i] || a.num_heads[i] != b.num_heads[i] ||
            a.transformer_layers[i] != b.transformer_layers[i])
            return false;
    return true;
}

// Whether a ControlNet of configuration n can feed a UNet of configuration u: its residuals must have the shapes of
// u's skips and mid-block output, and it must read the same sample, text and text_time conditioning.
// What the six sd_unet_forward* entries share: the null check and the typed pointers of the arguments they all take.
// (For _cfg / _pag `sample` is the un-duplicated latents and B their count: UNet::forward_cfg.)
bool fill_call(const sd_unet* u, const void* sample, const float* timesteps, const void* ehs, int ehs_len, const void* add_text,
               const float* add_time_ids, void* out, int B, int H, int W, UNetCall* c) {
    if (!u || !sample || !timesteps || !ehs || !out) { set_error("null argument"); return false; }
    c->sample = static_cast<const half_t*>(sample);
    c->timesteps = timesteps;
    c->ehs = static_cast<const half_t*>(ehs);
    c->L = ehs_len;
    c->add_text = static_cast<const half_t*>(add_text);
    c->add_time_ids = add_time_ids;
    c->out = static_cast<half_t*>(out);
    c->B = B; c->H = H; c->W = W;
    return true;
}
void with_images(UNetCall* c, const void* image_embeds, int n_img) {
    c->image_embeds = static_cast<const half_t*>(image_embeds);
    c->n_img = image_embeds ? n_img : 0;
}

// sd_*_poison_workspace: fill the `n` scratch buffers of a handle (an empty one is skipped) and report their capacities.
// Synchronised on both sides: nothing enqueued earlier may still write them, and the caller's next launch finds them filled.
struct PoisonBuf { const void* p; size_t bytes; };
int poison_buffers(const PoisonBuf* bufs, int n, int pattern, int64_t* bytes_filled) {
    if (!bytes_filled) { set_error("null argument"); return SD_ERR_INVALID; }
    if (pattern != SD_POISON_NAN && pattern != SD_POISON_INF) {
        set_error("sd_*_poison_workspace: unknown pattern " + std::to_string(pattern));
        return SD_ERR_INVALID;
    }
    *bytes_filled = 0;
    SD_HIP_CHECK(hipDeviceSynchronize());
    for (int i = 0; i < n; ++i) {
        char* p = static_cast<char*>(const_cast<void*>(bufs[i].p));
        const size_t bytes = bufs[i].bytes;
        if (!p || !bytes) continue;
        if (pattern == SD_POISON_NAN) {
            SD_HIP_CHECK(hipMemsetAsync(p, 0xFF, bytes, 0));
        } else {
            SD_HIP_CHECK(hipMemsetD16Async(p, 0x7C00, bytes / 2, 0));
            if (bytes & 1) SD_HIP_CHECK(hipMemsetAsync(p + bytes - 1, 0x7C, 1, 0));
        }
        *bytes_filled += (int64_t)bytes;
    }
    SD_HIP_CHECK(hipDeviceSynchronize());
    return SD_OK;
}
int poison_arena(const sd::Arena& a, int pattern, int64_t* bytes_filled) {
    const PoisonBuf b{a.base(), a.capacity()};
    return poison_buffers(&b, 1, pattern, bytes_filled);
}

// the list / info / read-back trio of the debug taps, shared by the UNet's and the VAE's entries
int tap_switch(sd::TapSink& t, int enable) {
    t.clear();
    t.on = enable != 0;
    t.scale = 1.f;
    return SD_OK;
}
int tap_info(const sd::TapSink& t, int index, sd_tap_info* info) {
    if (!info) { set_error("null argument"); return SD_ERR_INVALID; }
    if (index < 0 || index >= (int)t.entries.size()) { set_error("tap index out of range"); return SD_ERR_INVALID; }
    const sd::TapEntry& e = t.entries[(size_t)index];
    info->name = e.name.c_str();
    info->kind = e.kind;
    info->dtype = e.f32 ? SD_DTYPE_F32 : SD_DTYPE_F16;
    info->N = e.N; info->H = e.H; info->W = e.W; info->C = e.C; info->c0 = e.c0;
    info->ld = e.ld;
    info->bytes = (int64_t)e.bytes;
    info->scale = t.scale;
    return SD_OK;
}
int tap_read(const sd::TapSink& t, int index, void* dst, int64_t bytes) {
    if (!dst) { set_error("null argument"); return SD_ERR_INVALID; }
    if (index < 0 || index >= (int)t.entries.size()) { set_error("tap index out of range"); return SD_ERR_INVALID; }
    const sd::TapEntry& e = t.entries[(size_t)index];
    if (bytes != (int64_t)e.bytes) {
        set_error("tap read: " + std::to_string(bytes) + " bytes asked, the record holds " + std::to_string(e.bytes));
        return SD_ERR_INVALID;
    }
    SD_HIP_CHECK(hipDeviceSynchronize());
    SD_HIP_CHECK(hipMemcpy(dst, e.dev, e.bytes, hipMemcpyDeviceToHost));
    return SD_OK;
}

bool motion_fits(const sd_unet_config& u, const sd_motion_config& m, std::string* why) {
    if (m.num_blocks != u.num_blocks || m.layers_per_block != u.layers_per_block) {
        *why = "num_blocks / layers_per_block differ from the UNet's";
        return false;
    }
    for (int i = 0; i < u.num_blocks; ++i)
        if (m.block_out_channels[i] != u.block_out_channels[i]) { *why = "block_out_channels differ from the UNet's"; return false; }
    return true;
}

bool controlnet_fits(const sd_unet_config& u, const sd_unet_config& n, std::string* why) {
    if (n.num_blocks != u.num_blocks || n.layers_per_block != u.layers_per_block) {
        *why = "num_blocks / layers_per_block differ from the UNet's";
        return false;
    }
    for (int i = 0; i < u.num_blocks; ++i)
        if (n.block_out_channels[i] != u.block_out_channels[i]) { *why = "block_out_channels differ from the UNet's"; return false; }
    if (n.cross_attention_dim != u.cross_attention_dim) { *why = "cross_attention_dim differs from the UNet's"; return false; }
    if (n.in_channels != u.in_channels) { *why = "in_channels differs from the UNet's (9-channel inpaint UNets take no ControlNet)"; return false; }
    if (n.addition_time_embed_dim != u.addition_time_embed_dim ||
        n.projection_class_embeddings_input_dim != u.projection_class_embeddings_input_dim ||
        time_ids_of(n) != time_ids_of(u)) {
        *why = "text_time conditioning differs from the UNet's";
        return false;
    }
    return true;
}

}  // namespace

extern "C" {

const char* sd_last_error(void) { return sd::last_error().c_str(); }
int sd_engine_version(void) { return 1; }
const char* sd_engine_arch(void) { return "gfx950"; }

// ------------------------------------------------------------------------------------------- UNet
int sd_unet_create(const sd_unet_config* cfg, sd_unet** out) {
    if (!out) { set_error("null out"); return SD_ERR_INVALID; }
    if (bad_cfg(cfg)) {
        set_error("sd_unet_create: unsupported config (channels must be multiples of 64 and of the group "
                  "count, head dims in {32,40,64,80,128,160}, cross_attention_dim % 64 == 0, text_time: even "
                  "addition_time_embed_dim, num_time_ids in 1..8 (0: 6) and projection_class_embeddings_input_dim "
                  "> num_time_ids x addition_time_embed_dim, % 64 == 0 with six ids and % 8 == 0 otherwise)");
        return SD_ERR_UNSUPPORTED;
    }
    if (cfg->time_cond_proj_dim < 0 || cfg->time_cond_proj_dim > 1024) {
        set_error("sd_unet_create: time_cond_proj_dim must be in [0, 1024] (0: no time_embedding.cond_proj)");
        return SD_ERR_INVALID;
    }
    *out = new (std::nothrow) sd_unet(*cfg);
    if (!*out) { set_error("out of host memory"); return SD_ERR_INVALID; }
    return SD_OK;
}
int sd_unet_destroy(sd_unet* u) { delete u; return SD_OK; }
int sd_unet_num_weights(const sd_unet* u) { return u ? (int)u->impl.ws.order.size() : 0; }
int sd_unet_weight_info(const sd_unet* u, int index, const char** key, int64_t* shape4, int* ndim) {
    if (!u) { set_error("null handle"); return SD_ERR_INVALID; }
    return weight_info(u->impl.ws, index, key, shape4, ndim);
}
int sd_unet_set_weight(sd_unet* u, const char* key, const void* data, const int64_t* shape, int ndim, int dtype) {
    if (!u || !key || !data || !shape) { set_error("null argument"); return SD_ERR_INVALID; }
    if (u->impl.finalized) { set_error("set_weight after finalize"); return SD_ERR_STATE; }
    return u->impl.ws.set(key, data, shape, ndim, dtype);
}
int sd_unet_finalize(sd_unet* u) {
    if (!u) { set_error("null handle"); return SD_ERR_INVALID; }
    return u->impl.finalize();
}
int sd_unet_forward(sd_unet* u, const void* sample, const float* timesteps, const void* ehs, int ehs_len,
                    const void* add_text, const float* add_time_ids, void* out, int B, int H, int W,
                    void* stream) {
    UNetCall c;
    if (!fill_call(u, sample, timesteps, ehs, ehs_len, add_text, add_time_ids, out, B, H, W, &c)) return SD_ERR_INVALID;
    return u->impl.forward(c, static_cast<hipStream_t>(stream));
}
int sd_unet_use_graph(sd_unet* u, int enable) {
    if (!u) { set_error("null handle"); return SD_ERR_INVALID; }
    u->impl.graph_enabled = enable != 0;
    return SD_OK;
}
int sd_unet_graph_stats(const sd_unet* u, int64_t* captures, int64_t* replays) {
    if (!u) { set_error("null handle"); return SD_ERR_INVALID; }
    if (captures) *captures = u->impl.graph_captures;
    if (replays) *replays = u->impl.graph_replays;
    return SD_OK;
}
int sd_unet_text_kv_cache(sd_unet* u, int enable) {
    if (!u) { set_error("null handle"); return SD_ERR_INVALID; }
    u->impl.kv_cache_on = enable != 0;
    u->impl.kv_tag.clear();             // every call invalidates: the next forward recomputes
    u->impl.ipkv_tag.clear();           // (the IP-Adapter's image K / V alike)
    u->impl.clear_cn_tags();            // (and every ControlNet's conditioning embedding and text K / V)
    return SD_OK;
}
int sd_unet_forward_ex(sd_unet* u, const void* sample, const float* timesteps, const void* ehs, int ehs_len,
                       const void* add_text, const float* add_time_ids, const void* image_embeds, int n_img, void* out,
                       int B, int H, int W, void* stream) {
    UNetCall c;
    if (!fill_call(u, sample, timesteps, ehs, ehs_len, add_text, add_time_ids, out, B, H, W, &c)) return SD_ERR_INVALID;
    with_images(&c, image_embeds, n_img);
    return u->impl.forward(c, static_cast<hipStream_t>(stream));
}
int sd_unet_forward_tc(sd_unet* u, const void* sample, const float* timesteps, const void* ehs, int ehs_len,
                       const void* add_text, const float* add_time_ids, const void* image_embeds, int n_img,
                       const float* timestep_cond, int cond_dim, void* out, int B, int H, int W, void* stream) {
    UNetCall c;
    if (!fill_call(u, sample, timesteps, ehs, ehs_len, add_text, add_time_ids, out, B, H, W, &c)) return SD_ERR_INVALID;
    if (timestep_cond) {
        const int want = u->impl.cfg.time_cond_proj_dim;
        if (want <= 0) { set_error("sd_unet_forward_tc: timestep_cond given but the UNet has no time_cond_proj_dim"); return SD_ERR_INVALID; }
        if (cond_dim != want) {
            set_error("sd_unet_forward_tc: cond_dim " + std::to_string(cond_dim) + " != time_cond_proj_dim " + std::to_string(want));
            return SD_ERR_INVALID;
        }
    }
    with_images(&c, image_embeds, n_img);
    c.tcond = timestep_cond;
    return u->impl.forward(c, static_cast<hipStream_t>(stream));
}
int sd_unet_set_ip_adapter(sd_unet* u, sd_ip_adapter* a) {
    if (!u) { set_error("null handle"); return SD_ERR_INVALID; }
    if (a) {
        if (!a->impl.finalized) { set_error("sd_unet_set_ip_adapter: adapter not finalized"); return SD_ERR_STATE; }
        if (!same_topology(a->impl.cfg, u->impl.cfg)) {
            set_error("sd_unet_set_ip_adapter: the adapter was created for another UNet configuration");
            return SD_ERR_INVALID;
        }
    }
    u->impl.set_ip_adapter(a ? &a->impl : nullptr);
    u->impl.dc_tag.clear();
    return SD_OK;
}
int sd_unet_set_controlnet(sd_unet* u, sd_controlnet* cn) {
    if (!u) { set_error("null handle"); return SD_ERR_INVALID; }
    if (cn) {
        if (!cn->impl.finalized) { set_error("sd_unet_set_controlnet: ControlNet not finalized"); return SD_ERR_STATE; }
        std::string why;
        if (!controlnet_fits(u->impl.cfg, cn->impl.cfg, &why)) { set_error("sd_unet_set_controlnet: " + why); return SD_ERR_INVALID; }
    }
    if (int rc = u->impl.set_controlnet(cn ? &cn->impl : nullptr)) return rc;
    u->impl.dc_tag.clear();
    return SD_OK;
}
int sd_unet_set_controlnets(sd_unet* u, sd_controlnet* const* cns, int count) {
    if (!u || (count > 0 && !cns)) { set_error("null argument"); return SD_ERR_INVALID; }
    if (count < 0 || count > SD_MAX_CONTROLNETS) {
        set_error("sd_unet_set_controlnets: at most " + std::to_string(SD_MAX_CONTROLNETS) + " ControlNets");
        return SD_ERR_INVALID;
    }
    ControlNet* nets[SD_MAX_CONTROLNETS] = {};
    for (int i = 0; i < count; ++i) {
        if (!cns[i]) { set_error("sd_unet_set_controlnets: null ControlNet in the list"); return SD_ERR_INVALID; }
        if (!cns[i]->impl.finalized) { set_error("sd_unet_set_controlnets: ControlNet not finalized"); return SD_ERR_STATE; }
        std::string why;
        if (!controlnet_fits(u->impl.cfg, cns[i]->impl.cfg, &why)) { set_error("sd_unet_set_controlnets: " + why); return SD_ERR_INVALID; }
        for (int j = 0; j < i; ++j)
            if (cns[j] == cns[i]) { set_error("sd_unet_set_controlnets: the same ControlNet twice in the list"); return SD_ERR_INVALID; }
        nets[i] = &cns[i]->impl;
    }
    if (int rc = u->impl.set_controlnets(nets, count)) return rc;
    u->impl.dc_tag.clear();
    return SD_OK;
}
int sd_unet_forward_mcn(sd_unet* u, const void* sample, const float* timesteps, const void* ehs, int ehs_len,
                        const void* add_text, const float* add_time_ids, const void* image_embeds, int n_img,
                        const void* const* control_images, const int* n_ctrl, const float* cond_scales, int n_nets,
                        void* out, int B, int H, int W, void* stream) {
    UNetCall c;
    if (!fill_call(u, sample, timesteps, ehs, ehs_len, add_text, add_time_ids, out, B, H, W, &c)) return SD_ERR_INVALID;
    if (n_nets < 0 || n_nets > SD_MAX_CONTROLNETS || (n_nets > 0 && (!control_images || !n_ctrl || !cond_scales))) {
        set_error("sd_unet_forward_mcn: n_nets outside 0.." + std::to_string(SD_MAX_CONTROLNETS) + " or a null list");
        return SD_ERR_INVALID;
    }
    with_images(&c, image_embeds, n_img);
    c.mcn = true;
    c.n_nets = n_nets;
    for (int i = 0; i < n_nets; ++i) {
        c.mc_control[i] = static_cast<const half_t*>(control_images[i]);
        c.mc_n_ctrl[i] = n_ctrl[i];
        c.mc_scale[i] = cond_scales[i];
    }
    return u->impl.forward(c, static_cast<hipStream_t>(stream));
}
int64_t sd_unet_cn_fold_count(const sd_unet* u) { return u ? u->impl.cn_fold_count : 0; }
int sd_cn_kcat_force(int mode) { cn_kcat_force(mode); return SD_OK; }
int sd_unet_forward_cn(sd_unet* u, const void* sample, const float* timesteps, const void* ehs, int ehs_len,
                       const void* add_text, const float* add_time_ids, const void* image_embeds, int n_img,
                       const void* control_image, int n_ctrl, float cond_scale, void* out, int B, int H, int W,
                       void* stream) {
    UNetCall c;
    if (!fill_call(u, sample, timesteps, ehs, ehs_len, add_text, add_time_ids, out, B, H, W, &c)) return SD_ERR_INVALID;
    with_images(&c, image_embeds, n_img);
    c.control = static_cast<const half_t*>(control_image);
    c.n_ctrl = control_image ? n_ctrl : 0;
    c.cn_scale = cond_scale;
    return u->impl.forward(c, static_cast<hipStream_t>(stream));
}
int sd_unet_forward_cfg(sd_unet* u, const void* latents, const float* timesteps, const void* ehs, int ehs_len,
                        const void* add_text, const float* add_time_ids, const void* image_embeds, int n_img,
                        float in_scale, int share, void* out, int B, int H, int W, void* stream) {
    UNetCall c;
    if (!fill_call(u, latents, timesteps, ehs, ehs_len, add_text, add_time_ids, out, B, H, W, &c)) return SD_ERR_INVALID;
    if (!(in_scale == in_scale)) { set_error("sd_unet_forward_cfg: in_scale is NaN"); return SD_ERR_INVALID; }
    with_images(&c, image_embeds, n_img);
    return u->impl.forward_cfg(c, in_scale, share != 0, static_cast<hipStream_t>(stream));
}
int sd_unet_forward_cfg_ex(sd_unet* u, const void* latents, const float* timesteps, const void* ehs, int ehs_len,
                           const void* add_text, const float* add_time_ids, const void* image_embeds, int n_img,
                           float in_scale, int share, int num_frames, void* out, int B, int H, int W, void* stream) {
    UNetCall c;
    if (!fill_call(u, latents, timesteps, ehs, ehs_len, add_text, add_time_ids, out, B, H, W, &c)) return SD_ERR_INVALID;
    if (!(in_scale == in_scale)) { set_error("sd_unet_forward_cfg_ex: in_scale is NaN"); return SD_ERR_INVALID; }
    with_images(&c, image_embeds, n_img);
    c.num_frames = num_frames;
    return u->impl.forward_cfg(c, in_scale, share != 0, static_cast<hipStream_t>(stream));
}
int sd_unet_forward_motion(sd_unet* u, const void* sample, const float* timesteps, const void* ehs, int ehs_len, int num_frames,
                           void* out, int B, int H, int W, void* stream) {
    UNetCall c;
    if (!fill_call(u, sample, timesteps, ehs, ehs_len, nullptr, nullptr, out, B, H, W, &c)) return SD_ERR_INVALID;
    c.num_frames = num_frames;
    return u->impl.forward(c, static_cast<hipStream_t>(stream));
}
int sd_unet_set_motion(sd_unet* u, sd_motion* m) {
    if (!u) { set_error("null handle"); return SD_ERR_INVALID; }
    if (!u->impl.finalized) { set_error("sd_unet_set_motion before finalize"); return SD_ERR_STATE; }
    if (m) {
        if (!m->impl.finalized) { set_error("sd_unet_set_motion: motion adapter not finalized"); return SD_ERR_STATE; }
        std::string why;
        if (!motion_fits(u->impl.cfg, m->impl.mcfg, &why)) { set_error("sd_unet_set_motion: " + why); return SD_ERR_INVALID; }
    }
    return u->impl.set_motion(m ? &m->impl : nullptr);
}
int sd_motion_create(const sd_unet* u, const sd_motion_config* cfg, sd_motion** out) {
    if (!u || !cfg || !out) { set_error("null argument"); return SD_ERR_INVALID; }
    std::string why;
    if (!motion_fits(u->impl.cfg, *cfg, &why)) { set_error("sd_motion_create: " + why); return SD_ERR_INVALID; }
    if (cfg->max_seq_length < 1 || cfg->max_seq_length > 32) { set_error("sd_motion_create: max_seq_length must be in 1..32"); return SD_ERR_UNSUPPORTED; }
    for (int i = 0; i < cfg->num_blocks; ++i) {
        const int C = cfg->block_out_channels[i], h = cfg->num_heads[i];
        if (h < 1 || C % h != 0 || temporal_attention_plan(1, 1, 1, h, C / h).D == 0 || C % 64 != 0) {
            set_error("sd_motion_create: block " + std::to_string(i) + ": channels must be a multiple of 64 and the head dim one of "
                      "32, 40, 64, 80, 160");
            return SD_ERR_UNSUPPORTED;
        }
    }
    *out = new (std::nothrow) sd_motion(*cfg);
    if (!*out) { set_error("out of host memory"); return SD_ERR_INVALID; }
    return SD_OK;
}
int sd_motion_destroy(sd_motion* m) { delete m; return SD_OK; }
int sd_motion_num_weights(const sd_motion* m) { return m ? (int)m->impl.ws.order.size() : 0; }
int sd_motion_weight_info(const sd_motion* m, int index, const char** key, int64_t* shape4, int* ndim) {
    if (!m) { set_error("null handle"); return SD_ERR_INVALID; }
    return weight_info(m->impl.ws, index, key, shape4, ndim);
}
int sd_motion_set_weight(sd_motion* m, const char* key, const void* data, const int64_t* shape, int ndim, int dtype) {
    if (!m || !key || !data || !shape) { set_error("null argument"); return SD_ERR_INVALID; }
    if (m->impl.finalized) { set_error("set_weight after finalize"); return SD_ERR_STATE; }
    return m->impl.ws.set(key, data, shape, ndim, dtype);
}
int sd_motion_finalize(sd_motion* m) {
    if (!m) { set_error("null handle"); return SD_ERR_INVALID; }
    return m->impl.finalize();
}
int sd_unet_set_pag_layers(sd_unet* u, const char* const* site_keys, int count) {
    if (!u) { set_error("null handle"); return SD_ERR_INVALID; }
    return u->impl.set_pag_layers(site_keys, count);
}
int sd_unet_forward_pag(sd_unet* u, const void* latents, const float* timesteps, const void* ehs, int ehs_len,
                        const void* add_text, const float* add_time_ids, float in_scale, int cfg, int share, void* out,
                        int B, int H, int W, void* stream) {
    UNetCall c;
    if (!fill_call(u, latents, timesteps, ehs, ehs_len, add_text, add_time_ids, out, B, H, W, &c)) return SD_ERR_INVALID;
    if (!(in_scale == in_scale)) { set_error("sd_unet_forward_pag: in_scale is NaN"); return SD_ERR_INVALID; }
    return u->impl.forward_pag(c, in_scale, cfg != 0, share != 0, static_cast<hipStream_t>(stream));
}
int sd_unet_forward_concat(sd_unet* u, const void* latents, int B_lat, float in_scale, const void* extra, int extra_channels,
                           int extra_rows, int zero_from, const float* timesteps, const void* ehs, int ehs_len,
                           const void* add_text, const float* add_time_ids, void* out, int B, int H, int W, void* stream) {
    UNetCall c;
    if (!fill_call(u, latents, timesteps, ehs, ehs_len, add_text, add_time_ids, out, B, H, W, &c)) return SD_ERR_INVALID;
    if (!extra) { set_error("null argument"); return SD_ERR_INVALID; }
    c.extra = static_cast<const half_t*>(extra);
    c.extra_channels = extra_channels; c.extra_rows = extra_rows; c.zero_from = zero_from;
    c.lat_rows = B_lat; c.in_scale = in_scale;
    return u->impl.forward_concat(c, static_cast<hipStream_t>(stream));
}
int sd_unet_tap(sd_unet* u, int enable) {
    if (!u) { set_error("null handle"); return SD_ERR_INVALID; }
    return tap_switch(u->impl.taps, enable);
}
int sd_unet_tap_count(const sd_unet* u) { return u ? (int)u->impl.taps.entries.size() : 0; }
int sd_unet_tap_info(const sd_unet* u, int index, sd_tap_info* info) {
    if (!u) { set_error("null handle"); return SD_ERR_INVALID; }
    return tap_info(u->impl.taps, index, info);
}
int sd_unet_tap_read(sd_unet* u, int index, void* dst, int64_t bytes) {
    if (!u) { set_error("null handle"); return SD_ERR_INVALID; }
    return tap_read(u->impl.taps, index, dst, bytes);
}
int sd_unet_poison_workspace(sd_unet* u, int pattern, int64_t* bytes_filled) {
    if (!u) { set_error("null handle"); return SD_ERR_INVALID; }
    UNet& n = u->impl;
    // (the level weights of regional prompts are scratch too: the next forward rebuilds them from the kept copy)
    const PoisonBuf bufs[4] = {{n.arena.base(), n.arena.capacity()}, {n.cfg_slab.data(), n.cfg_slab.capacity()},
                               {n.io_slab.data(), n.io_slab.capacity()}, {n.region_buf.data(), n.region_buf.capacity()}};
    const int rc = poison_buffers(bufs, 4, pattern, bytes_filled);
    if (rc == SD_OK && n.region_buf.capacity()) n.region_stale = true;
    return rc;
}
int sd_unet_cfg_share(const sd_unet_config* cfg) { return cfg && sd::unet_cfg_share_eligible(*cfg) ? 1 : 0; }
int sd_unet_set_ip_adapter_scale(sd_unet* u, float scale) {
    if (!u) { set_error("null handle"); return SD_ERR_INVALID; }
    if (!(scale == scale)) { set_error("sd_unet_set_ip_adapter_scale: NaN"); return SD_ERR_INVALID; }
    u->impl.ip_scale = scale;
    return SD_OK;
}
int sd_unet_set_freeu(sd_unet* u, int enable, float s1, float s2, float b1, float b2) {
    if (!u) { set_error("null handle"); return SD_ERR_INVALID; }
    u->impl.dc_tag.clear();             // (a DeepCache feature stored under other FreeU settings is stale)
    if (!enable) { u->impl.freeu_on = false; return SD_OK; }
    if (!std::isfinite(s1) || !std::isfinite(s2) || !std::isfinite(b1) || !std::isfinite(b2)) {
        set_error("sd_unet_set_freeu: s1, s2, b1, b2 must be finite");
        return SD_ERR_INVALID;
    }
    u->impl.freeu_on = true;
    u->impl.freeu_s1 = s1; u->impl.freeu_s2 = s2; u->impl.freeu_b1 = b1; u->impl.freeu_b2 = b2;
    return SD_OK;
}
int sd_unet_set_tome(sd_unet* u, double ratio, int max_downsample, int sx, int sy, int use_rand, uint32_t seed) {
    if (!u) { set_error("null handle"); return SD_ERR_INVALID; }
    if (!u->impl.finalized) { set_error("sd_unet_set_tome before finalize"); return SD_ERR_STATE; }
    return u->impl.set_tome(ratio, max_downsample, sx, sy, use_rand, seed);
}
int sd_unet_tome_step(sd_unet* u, uint32_t step) {
    if (!u) { set_error("null handle"); return SD_ERR_INVALID; }
    u->impl.tome.step = step;
    return SD_OK;
}
int sd_unet_tome_sites(const sd_unet* u) { return u ? (int)u->impl.tome_used.size() : 0; }
int sd_unet_tome_read(sd_unet* u, int k, int32_t* info5, int32_t* map_host, int64_t cap) {
    if (!u || !info5) { set_error("null argument"); return -SD_ERR_INVALID; }
    if (k < 0 || k >= (int)u->impl.tome_used.size()) { set_error("sd_unet_tome_read: no such merged block in the last forward"); return -SD_ERR_INVALID; }
    const TomeUsed& t = u->impl.tome_used[(size_t)k];
    info5[0] = t.site; info5[1] = t.H; info5[2] = t.W; info5[3] = t.r; info5[4] = t.Tm;
    if (!map_host) return t.B;
    const int T = t.H * t.W;
    if (cap < (int64_t)t.B * T) { set_error("sd_unet_tome_read: map_host is too small"); return -SD_ERR_INVALID; }
    if (!u->impl.tome_buf.data()) { set_error("sd_unet_tome_read: the maps were released"); return -SD_ERR_STATE; }
    if (hipDeviceSynchronize() != hipSuccess) { set_error("sd_unet_tome_read: device error"); return -SD_ERR_HIP; }
    for (int b = 0; b < t.B; ++b)
        if (tome_plan_read_map(u->impl.tome_buf.data() + t.plan_off, b, T, map_host + (long)b * T)) return -SD_ERR_HIP;
    return t.B;
}
int sd_unet_set_hypertile(sd_unet* u, int tile_size, int swap_size, int max_depth, uint32_t seed) {
    if (!u) { set_error("null handle"); return SD_ERR_INVALID; }
    if (!u->impl.finalized) { set_error("sd_unet_set_hypertile before finalize"); return SD_ERR_STATE; }
    return u->impl.set_hypertile(tile_size, swap_size, max_depth, seed);
}
int sd_unet_hypertile_step(sd_unet* u, uint32_t step) {
    if (!u) { set_error("null handle"); return SD_ERR_INVALID; }
    u->impl.hypertile.step = step;
    return SD_OK;
}
int sd_unet_hypertile_sites(const sd_unet* u) { return u ? (int)u->impl.hypertile_used.size() : 0; }
int sd_unet_hypertile_read(const sd_unet* u, int k, int32_t* info8) {
    if (!u || !info8) { set_error("null argument"); return SD_ERR_INVALID; }
    if (k < 0 || k >= (int)u->impl.hypertile_used.size()) {
        set_error("sd_unet_hypertile_read: no such HyperTile site in the last forward");
        return SD_ERR_INVALID;
    }
    const HyperTileUsed& t = u->impl.hypertile_used[(size_t)k];
    info8[0] = t.site; info8[1] = t.H; info8[2] = t.W; info8[3] = t.nh; info8[4] = t.nw; info8[5] = t.B; info8[6] = t.copied;
    info8[7] = t.level;
    return SD_OK;
}
int sd_unet_set_regions(sd_unet* u, const float* weights, int Bw, int R, int H, int W, void* stream) {
    if (!u) { set_error("null handle"); return SD_ERR_INVALID; }
    return u->impl.set_regions(weights, Bw, R, H, W, static_cast<hipStream_t>(stream));
}
int sd_unet_set_deep_cache(sd_unet* u, int depth) {
    if (!u) { set_error("null handle"); return SD_ERR_INVALID; }
    return u->impl.set_deep_cache(depth);
}
int sd_unet_deep_cache_mode(sd_unet* u, int mode) {
    if (!u) { set_error("null handle"); return SD_ERR_INVALID; }
    if (mode != SD_DC_PLAIN && mode != SD_DC_STORE && mode != SD_DC_REUSE) {
        set_error("sd_unet_deep_cache_mode: unknown mode " + std::to_string(mode));
        return SD_ERR_INVALID;
    }
    if (mode != SD_DC_PLAIN && u->impl.dc_depth == 0) {
        set_error("sd_unet_deep_cache_mode: store / reuse while the depth is 0 (sd_unet_set_deep_cache)");
        return SD_ERR_STATE;
    }
    u->impl.dc_mode = mode;
    return SD_OK;
}

// ------------------------------------------------------------------------------------- IP-Adapter
int sd_ip_adapter_create_ex(const sd_unet* u, const sd_ip_projection_config* p, sd_ip_adapter** out) {
    if (!u || !p || !out) { set_error("null argument"); return SD_ERR_INVALID; }
    if (p->kind != SD_IP_PROJ_LINEAR && p->kind != SD_IP_PROJ_RESAMPLER) {
        set_error("sd_ip_adapter_create: unknown projection kind " + std::to_string(p->kind));
        return SD_ERR_INVALID;
    }
    const sd_unet_config& c = u->impl.cfg;
    const int image_embed_dim = p->image_embed_dim, num_tokens = p->num_tokens;
    if (c.cross_attention_dim % 64 != 0) { set_error("sd_ip_adapter_create: cross_attention_dim % 64 != 0"); return SD_ERR_UNSUPPORTED; }
    if (num_tokens < 1 || num_tokens > 16) { set_error("sd_ip_adapter_create: num_tokens must be in [1, 16]"); return SD_ERR_UNSUPPORTED; }
    if (image_embed_dim <= 0 || image_embed_dim % 64 != 0) {
        set_error("sd_ip_adapter_create: image_embed_dim must be a positive multiple of 64");
        return SD_ERR_UNSUPPORTED;
    }
    for (const auto& site : unet_xattn_sites(c, true)) {
        int heads = 0;
        for (int i = 0; i < c.num_blocks; ++i)
            if (c.block_out_channels[i] == site.second) heads = c.num_heads[i];
        if (heads <= 0 || !ip_attention_supported(site.second / heads)) {
            set_error("sd_ip_adapter_create: head dim of " + site.first + " not in {32, 40, 64, 80, 160}");
            return SD_ERR_UNSUPPORTED;
        }
    }
    sd_ip_projection_config q = *p;
    if (q.kind == SD_IP_PROJ_RESAMPLER) {
        if (q.dim <= 0 || q.dim % 64 != 0) { set_error("sd_ip_adapter_create: Resampler dim must be a positive multiple of 64"); return SD_ERR_UNSUPPORTED; }
        if (q.heads < 1 || (long)q.heads * 64 != q.dim) {
            set_error("sd_ip_adapter_create: Resampler dim_head (dim / heads) must be 64");
            return SD_ERR_UNSUPPORTED;
        }
        if (q.depth < 1 || q.depth > 16) { set_error("sd_ip_adapter_create: Resampler depth must be in [1, 16]"); return SD_ERR_UNSUPPORTED; }
        if (q.ff_mult < 1 || q.ff_mult > 8) { set_error("sd_ip_adapter_create: Resampler ff_mult must be in [1, 8]"); return SD_ERR_UNSUPPORTED; }
    } else {
        q.dim = q.heads = q.depth = q.ff_mult = 0;
    }
    *out = new (std::nothrow) sd_ip_adapter(c, q);
    if (!*out) { set_error("out of host memory"); return SD_ERR_INVALID; }
    return SD_OK;
}
int sd_ip_adapter_create(const sd_unet* u, int image_embed_dim, int num_tokens, sd_ip_adapter** out) {
    sd_ip_projection_config p = {};
    p.kind = SD_IP_PROJ_LINEAR;
    p.image_embed_dim = image_embed_dim;
    p.num_tokens = num_tokens;
    return sd_ip_adapter_create_ex(u, &p, out);
}
int sd_ip_adapter_set_feature_tokens(sd_ip_adapter* a, int T_feat) {
    if (!a) { set_error("null handle"); return SD_ERR_INVALID; }
    if (T_feat < 1) { set_error("sd_ip_adapter_set_feature_tokens: T_feat must be >= 1"); return SD_ERR_INVALID; }
    if (a->impl.kind != SD_IP_PROJ_RESAMPLER) {
        set_error("sd_ip_adapter_set_feature_tokens: a linear adapter reads one embedding per image");
        return SD_ERR_UNSUPPORTED;
    }
    if (T_feat + a->impl.n_tok > resampler_max_keys()) {
        set_error("sd_ip_adapter_set_feature_tokens: T_feat + num_tokens must be <= " + std::to_string(resampler_max_keys()));
        return SD_ERR_UNSUPPORTED;
    }
    a->impl.t_feat = T_feat;
    if (UNet* un = a->impl.attached) {      // the cached image K / V and the arena plan were made for the old count
        un->ipkv_tag.clear();
        un->dc_tag.clear();
        un->reset_plans();
    }
    return SD_OK;
}
int sd_ip_adapter_project(sd_ip_adapter* a, const void* image_embeds, int rows, void* tokens, void* stream) {
    if (!a || !image_embeds || !tokens) { set_error("null argument"); return SD_ERR_INVALID; }
    return a->impl.project(static_cast<const half_t*>(image_embeds), rows, static_cast<half_t*>(tokens),
                           static_cast<hipStream_t>(stream));
}
int sd_ip_adapter_memory(const sd_ip_adapter* a, int64_t* weight_bytes, int64_t* workspace_bytes) {
    if (!a) { set_error("null handle"); return SD_ERR_INVALID; }
    if (weight_bytes) *weight_bytes = a->impl.ws.packed_bytes();
    if (workspace_bytes) *workspace_bytes = (int64_t)a->impl.arena.capacity();
    return SD_OK;
}
int sd_ip_adapter_poison_workspace(sd_ip_adapter* a, int pattern, int64_t* bytes_filled) {
    if (!a) { set_error("null handle"); return SD_ERR_INVALID; }
    return poison_arena(a->impl.arena, pattern, bytes_filled);
}
int sd_ip_adapter_destroy(sd_ip_adapter* a) { delete a; return SD_OK; }
int sd_ip_adapter_num_weights(const sd_ip_adapter* a) { return a ? (int)a->impl.ws.order.size() : 0; }
int sd_ip_adapter_weight_info(const sd_ip_adapter* a, int index, const char** key, int64_t* shape4, int* ndim) {
    if (!a) { set_error("null handle"); return SD_ERR_INVALID; }
    return weight_info(a->impl.ws, index, key, shape4, ndim);
}
int sd_ip_adapter_set_weight(sd_ip_adapter* a, const char* key, const void* data, const int64_t* shape, int ndim,
                             int dtype) {
    if (!a || !key || !data || !shape) { set_error("null argument"); return SD_ERR_INVALID; }
    if (a->impl.finalized) { set_error("set_weight after finalize"); return SD_ERR_STATE; }
    return a->impl.ws.set(key, data, shape, ndim, dtype);
}
int sd_ip_adapter_finalize(sd_ip_adapter* a) {
    if (!a) { set_error("null handle"); return SD_ERR_INVALID; }
    return a->impl.finalize();
}
// ------------------------------------------------------------------------------------- ControlNet
int sd_controlnet_create(const sd_unet* u, const sd_unet_config* cn_cfg, int conditioning_channels, sd_controlnet** out) {
    if (!u || !cn_cfg || !out) { set_error("null argument"); return SD_ERR_INVALID; }
    if (conditioning_channels != 3) { set_error("sd_controlnet_create: conditioning_channels must be 3"); return SD_ERR_UNSUPPORTED; }
    // (only the encoder half of the configuration is read: make the up-path fields consistent for bad_cfg)
    sd_unet_config c = *cn_cfg;
    for (int i = 0; i < SD_MAX_BLOCKS; ++i) c.up_block_has_attn[i] = 0;
    c.time_cond_proj_dim = 0;            // (ControlNetModel has no cond_proj; the UNet rejects timestep_cond with one attached)
    if (bad_cfg(&c)) { set_error("sd_controlnet_create: unsupported encoder configuration"); return SD_ERR_UNSUPPORTED; }
    std::string why;
    if (!controlnet_fits(u->impl.cfg, c, &why)) { set_error("sd_controlnet_create: " + why); return SD_ERR_INVALID; }
    if (u->impl.cfg.in_channels != 4) { set_error("sd_controlnet_create: the UNet must take 4 latent channels"); return SD_ERR_INVALID; }
    if (1 + c.num_blocks * c.layers_per_block + (c.num_blocks - 1) + 1 > kCnMaxProblems) {
        set_error("sd_controlnet_create: more residual sites than one grouped launch takes (16)");
        return SD_ERR_UNSUPPORTED;
    }
    *out = new (std::nothrow) sd_controlnet(c, conditioning_channels);
    if (!*out) { set_error("out of host memory"); return SD_ERR_INVALID; }
    return SD_OK;
}
int sd_controlnet_destroy(sd_controlnet* cn) { delete cn; return SD_OK; }
int sd_controlnet_num_weights(const sd_controlnet* cn) { return cn ? (int)cn->impl.ws.order.size() : 0; }
int sd_controlnet_weight_info(const sd_controlnet* cn, int index, const char** key, int64_t* shape4, int* ndim) {
    if (!cn) { set_error("null handle"); return SD_ERR_INVALID; }
    return weight_info(cn->impl.ws, index, key, shape4, ndim);
}
int sd_controlnet_set_weight(sd_controlnet* cn, const char* key, const void* data, const int64_t* shape, int ndim,
                             int dtype) {
    if (!cn || !key || !data || !shape) { set_error("null argument"); return SD_ERR_INVALID; }
    if (cn->impl.finalized) { set_error("set_weight after finalize"); return SD_ERR_STATE; }
    return cn->impl.ws.set(key, data, shape, ndim, dtype);
}
int sd_controlnet_finalize(sd_controlnet* cn) {
    if (!cn) { set_error("null handle"); return SD_ERR_INVALID; }
    return cn->impl.finalize();
}
int sd_unet_memory(const sd_unet* u, int64_t* weight_bytes, int64_t* workspace_bytes) {
    if (!u) { set_error("null handle"); return SD_ERR_INVALID; }
    if (weight_bytes) *weight_bytes = u->impl.ws.packed_bytes();
    if (workspace_bytes) *workspace_bytes = (int64_t)(u->impl.arena.capacity() + u->impl.dc_buf.capacity() + u->impl.tome_buf.capacity() +
                                                      u->impl.cfg_slab.capacity() + u->impl.io_slab.capacity() +
                                                      u->impl.region_src.capacity() + u->impl.region_buf.capacity());
    return SD_OK;
}

// -------------------------------------------------------------------------------------------- VAE
int sd_vae_create(const sd_vae_config* cfg, sd_vae** out) {
    if (!out || !cfg) { set_error("null argument"); return SD_ERR_INVALID; }
    bool bad = cfg->num_blocks < 1 || cfg->num_blocks > SD_MAX_BLOCKS || cfg->latent_channels > 8;
    for (int i = 0; !bad && i < cfg->num_blocks; ++i)
        bad = cfg->block_out_channels[i] % 64 != 0;
    if (!bad) bad = !attention_supported(cfg->block_out_channels[cfg->num_blocks - 1]);
    if (bad) { set_error("sd_vae_create: unsupported config"); return SD_ERR_UNSUPPORTED; }
    *out = new (std::nothrow) sd_vae(*cfg);
    if (!*out) { set_error("out of host memory"); return SD_ERR_INVALID; }
    return SD_OK;
}
int sd_vae_destroy(sd_vae* v) { delete v; return SD_OK; }
int sd_vae_num_weights(const sd_vae* v) { return v ? (int)v->impl.ws.order.size() : 0; }
int sd_vae_weight_info(const sd_vae* v, int index, const char** key, int64_t* shape4, int* ndim) {
    if (!v) { set_error("null handle"); return SD_ERR_INVALID; }
    return weight_info(v->impl.ws, index, key, shape4, ndim);
}
int sd_vae_set_weight(sd_vae* v, const char* key, const void* data, const int64_t* shape, int ndim, int dtype) {
    if (!v || !key || !data || !shape) { set_error("null argument"); return SD_ERR_INVALID; }
    if (v->impl.finalized) { set_error("set_weight after finalize"); return SD_ERR_STATE; }
    return v->impl.ws.set(key, data, shape, ndim, dtype);
}
int sd_vae_finalize(sd_vae* v) {
    if (!v) { set_error("null handle"); return SD_ERR_INVALID; }
    return v->impl.finalize();
}
int sd_vae_decode(sd_vae* v, const void* z, void* img, int B, int h, int w, void* stream) {
    if (!v || !z || !img) { set_error("null argument"); return SD_ERR_INVALID; }
    return v->impl.decode(static_cast<const half_t*>(z), static_cast<half_t*>(img), B, h, w,
                          static_cast<hipStream_t>(stream));
}
int sd_vae_encode(sd_vae* v, const void* img, void* moments, int B, int H, int W, void* stream) {
    if (!v || !img || !moments) { set_error("null argument"); return SD_ERR_INVALID; }
    return v->impl.encode(static_cast<const half_t*>(img), static_cast<half_t*>(moments), B, H, W,
                          static_cast<hipStream_t>(stream));
}
int sd_vae_encode_range_shift(sd_vae* v, int shift) {
    if (!v || shift < 0 || shift > 14) { set_error("sd_vae_encode_range_shift: shift in 0..14"); return SD_ERR_INVALID; }
    v->impl.encode_shift = shift;
    return SD_OK;
}
int sd_vae_tap(sd_vae* v, int enable) {
    if (!v) { set_error("null handle"); return SD_ERR_INVALID; }
    return tap_switch(v->impl.taps, enable);
}
int sd_vae_tap_count(const sd_vae* v) { return v ? (int)v->impl.taps.entries.size() : 0; }
int sd_vae_tap_info(const sd_vae* v, int index, sd_tap_info* info) {
    if (!v) { set_error("null handle"); return SD_ERR_INVALID; }
    return tap_info(v->impl.taps, index, info);
}
int sd_vae_tap_read(sd_vae* v, int index, void* dst, int64_t bytes) {
    if (!v) { set_error("null handle"); return SD_ERR_INVALID; }
    return tap_read(v->impl.taps, index, dst, bytes);
}
int sd_vae_poison_workspace(sd_vae* v, int pattern, int64_t* bytes_filled) {
    if (!v) { set_error("null handle"); return SD_ERR_INVALID; }
    return poison_arena(v->impl.arena, pattern, bytes_filled);
}
int sd_vae_memory(const sd_vae* v, int64_t* weight_bytes, int64_t* workspace_bytes) {
    if (!v) { set_error("null handle"); return SD_ERR_INVALID; }
    if (weight_bytes) *weight_bytes = v->impl.ws.packed_bytes();
    if (workspace_bytes) *workspace_bytes = (int64_t)v->impl.arena.capacity();
    return SD_OK;
}
int sd_vae_memory_tiled(const sd_vae* v, int64_t* weight_bytes, int64_t* workspace_bytes, int64_t* tile_bytes) {
    if (int rc = sd_vae_memory(v, weight_bytes, workspace_bytes)) return rc;
    if (tile_bytes) *tile_bytes = (int64_t)(v->impl.tile_in.capacity() + v->impl.tile_stack.capacity());
    return SD_OK;
}
int sd_vae_tile_plan(int encode, int h, int w, int tile_sample, int tile_latent, double overlap_factor, sd_vae_tiles* plan) {
    return vae_tile_plan(encode, h, w, tile_sample, tile_latent, overlap_factor, plan) ? SD_ERR_INVALID : SD_OK;
}
int sd_vae_tile_stack(const sd_vae_tiles* plan, int B, int C, int64_t* tile_offsets, int64_t* total) {
    if (!plan || B < 1 || C < 1) { set_error("sd_vae_tile_stack: a plan, B >= 1, C >= 1"); return SD_ERR_INVALID; }
    long class_off[SD_VAE_TILE_MAX_CLASSES];
    const long n = vae_tile_stack(*plan, B, C, nullptr, class_off);
    const bool enc = plan->tile_out < plan->tile_in;
    for (int c = 0; tile_offsets && c < plan->n_classes; ++c) {
        const long oh = enc ? plan->class_h[c] / plan->scale : plan->class_h[c] * plan->scale;
        const long ow = enc ? plan->class_w[c] / plan->scale : plan->class_w[c] * plan->scale;
        for (int t = 0; t < plan->class_count[c]; ++t) {
            const int iy = plan->class_iy0[c] + t / plan->class_nx[c], ix = plan->class_ix0[c] + t % plan->class_nx[c];
            tile_offsets[iy * plan->nx + ix] = class_off[c] + (long)t * B * C * oh * ow;
        }
    }
    if (total) *total = n;
    return SD_OK;
}
int sd_vae_decode_tiled(sd_vae* v, const void* z, void* img, int B, int h, int w, int tile_latent, double overlap_factor,
                        int tile_batch, void* stream) {
    if (!v || !z || !img) { set_error("null argument"); return SD_ERR_INVALID; }
    return v->impl.decode_tiled(static_cast<const half_t*>(z), static_cast<half_t*>(img), B, h, w, tile_latent,
                                overlap_factor, tile_batch, static_cast<hipStream_t>(stream));
}
int sd_vae_encode_tiled(sd_vae* v, const void* img, void* moments, int B, int H, int W, int tile_latent,
                        double overlap_factor, int tile_batch, void* stream) {
    if (!v || !img || !moments) { set_error("null argument"); return SD_ERR_INVALID; }
    return v->impl.encode_tiled(static_cast<const half_t*>(img), static_cast<half_t*>(moments), B, H, W, tile_latent,
                                overlap_factor, tile_batch, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------- CLIP
int sd_clip_create(const sd_clip_config* cfg, sd_clip** out) {
    if (!out || !cfg) { set_error("null argument"); return SD_ERR_INVALID; }
    const bool bad = cfg->vocab_size < 1 || cfg->num_layers < 1 || cfg->num_heads < 1 || cfg->max_positions < 1 ||
                     cfg->hidden_size % 64 != 0 || cfg->intermediate_size % 64 != 0 || cfg->hidden_size > 2048 ||
                     cfg->hidden_size % cfg->num_heads != 0 || !attention_supported(cfg->hidden_size / cfg->num_heads) ||
                     (cfg->hidden_act != 0 && cfg->hidden_act != 1) || cfg->projection_dim < 0;
    if (bad) { set_error("sd_clip_create: unsupported config (hidden / intermediate % 64, head dim, activation)"); return SD_ERR_UNSUPPORTED; }
    *out = new (std::nothrow) sd_clip(*cfg);
    if (!*out) { set_error("out of host memory"); return SD_ERR_INVALID; }
    return SD_OK;
}
int sd_clip_destroy(sd_clip* c) { delete c; return SD_OK; }
int sd_clip_num_weights(const sd_clip* c) { return c ? (int)c->impl.ws.order.size() : 0; }
int sd_clip_weight_info(const sd_clip* c, int index, const char** key, int64_t* shape4, int* ndim) {
    if (!c) { set_error("null handle"); return SD_ERR_INVALID; }
    return weight_info(c->impl.ws, index, key, shape4, ndim);
}
int sd_clip_set_weight(sd_clip* c, const char* key, const void* data, const int64_t* shape, int ndim, int dtype) {
    if (!c || !key || !data || !shape) { set_error("null argument"); return SD_ERR_INVALID; }
    if (c->impl.finalized) { set_error("set_weight after finalize"); return SD_ERR_STATE; }
    return c->impl.ws.set(key, data, shape, ndim, dtype);
}
int sd_clip_finalize(sd_clip* c) {
    if (!c) { set_error("null handle"); return SD_ERR_INVALID; }
    return c->impl.finalize();
}
int sd_clip_forward(sd_clip* c, const int32_t* input_ids, const int32_t* eos_index, void* hidden_states, void* last_hidden,
                    void* pooled, void* text_embeds, int B, int T, void* stream) {
    if (!c || !input_ids) { set_error("null argument"); return SD_ERR_INVALID; }
    return c->impl.forward(input_ids, eos_index, static_cast<half_t*>(hidden_states), static_cast<half_t*>(last_hidden),
                           static_cast<half_t*>(pooled), static_cast<half_t*>(text_embeds), B, T,
                           static_cast<hipStream_t>(stream));
}
int sd_clip_final_layer_norm(sd_clip* c, const void* x, void* y, int64_t rows, void* stream) {
    if (!c || !x || !y || rows < 0) { set_error("bad argument"); return SD_ERR_INVALID; }
    if (rows == 0) return SD_OK;
    return c->impl.final_layer_norm(static_cast<const half_t*>(x), static_cast<half_t*>(y), (long)rows,
                                    static_cast<hipStream_t>(stream));
}
int sd_clip_poison_workspace(sd_clip* c, int pattern, int64_t* bytes_filled) {
    if (!c) { set_error("null handle"); return SD_ERR_INVALID; }
    return poison_arena(c->impl.arena, pattern, bytes_filled);
}
int sd_clip_memory(const sd_clip* c, int64_t* weight_bytes, int64_t* workspace_bytes) {
    if (!c) { set_error("null handle"); return SD_ERR_INVALID; }
    if (weight_bytes) *weight_bytes = c->impl.ws.packed_bytes();
    if (workspace_bytes) *workspace_bytes = (int64_t)c->impl.arena.capacity();
    return SD_OK;
}

// ------------------------------------------------------------------------------------ CLIP vision
int sd_clip_vision_create(const sd_clip_vision_config* cfg, sd_clip_vision** out) {
    if (!out || !cfg) { set_error("null argument"); return SD_ERR_INVALID; }
    if (cfg->hidden_size < 8 || cfg->intermediate_size < 8 || cfg->num_layers < 1 || cfg->num_heads < 1 ||
        cfg->image_size < 1 || cfg->patch_size < 1 || cfg->projection_dim < 1 ||
        (cfg->hidden_act != 0 && cfg->hidden_act != 1)) {
        set_error("sd_clip_vision_create: bad config (sizes must be positive, hidden_act 0 quick_gelu or 1 gelu)");
        return SD_ERR_INVALID;
    }
    if (cfg->image_size % cfg->patch_size != 0) {
        set_error("sd_clip_vision_create: image_size " + std::to_string(cfg->image_size) + " is not divisible by patch_size " +
                  std::to_string(cfg->patch_size));
        return SD_ERR_UNSUPPORTED;
    }
    if (cfg->hidden_size % cfg->num_heads != 0) {
        set_error("sd_clip_vision_create: hidden_size " + std::to_string(cfg->hidden_size) + " is not divisible by num_heads " +
                  std::to_string(cfg->num_heads));
        return SD_ERR_UNSUPPORTED;
    }
    if (cfg->hidden_size % 8 != 0 || cfg->intermediate_size % 8 != 0 || cfg->hidden_size > 2048) {
        set_error("sd_clip_vision_create: hidden_size " + std::to_string(cfg->hidden_size) + " / intermediate_size " +
                  std::to_string(cfg->intermediate_size) + " must be multiples of 8, hidden_size at most 2048");
        return SD_ERR_UNSUPPORTED;
    }
    const int d = cfg->hidden_size / cfg->num_heads;
    if (clip_vision_padded_head_dim(d) == 0) {
        set_error("sd_clip_vision_create: unsupported head dim " + std::to_string(d) +
                  " (heads are zero-padded up to 128 at most)");
        return SD_ERR_UNSUPPORTED;
    }
    *out = new (std::nothrow) sd_clip_vision(*cfg);
    if (!*out) { set_error("out of host memory"); return SD_ERR_INVALID; }
    return SD_OK;
}
int sd_clip_vision_destroy(sd_clip_vision* c) { delete c; return SD_OK; }
int sd_clip_vision_num_weights(const sd_clip_vision* c) { return c ? (int)c->impl.ws.order.size() : 0; }
int sd_clip_vision_weight_info(const sd_clip_vision* c, int index, const char** key, int64_t* shape4, int* ndim) {
    if (!c) { set_error("null handle"); return SD_ERR_INVALID; }
    return weight_info(c->impl.ws, index, key, shape4, ndim);
}
int sd_clip_vision_set_weight(sd_clip_vision* c, const char* key, const void* data, const int64_t* shape, int ndim, int dtype) {
    if (!c || !key || !data || !shape) { set_error("null argument"); return SD_ERR_INVALID; }
    if (c->impl.finalized) { set_error("set_weight after finalize"); return SD_ERR_STATE; }
    return c->impl.ws.set(key, data, shape, ndim, dtype);
}
int sd_clip_vision_finalize(sd_clip_vision* c) {
    if (!c) { set_error("null handle"); return SD_ERR_INVALID; }
    return c->impl.finalize();
}
int sd_clip_vision_forward(sd_clip_vision* c, const void* pixel_values, void* hidden_states, void* last_hidden, void* pooled,
                           void* image_embeds, int B, void* stream) {
    if (!c || !pixel_values) { set_error("null argument"); return SD_ERR_INVALID; }
    return c->impl.forward(static_cast<const half_t*>(pixel_values), static_cast<half_t*>(hidden_states),
                           static_cast<half_t*>(last_hidden), static_cast<half_t*>(pooled), static_cast<half_t*>(image_embeds),
                           B, static_cast<hipStream_t>(stream));
}
int sd_clip_vision_poison_workspace(sd_clip_vision* c, int pattern, int64_t* bytes_filled) {
    if (!c) { set_error("null handle"); return SD_ERR_INVALID; }
    return poison_arena(c->impl.arena, pattern, bytes_filled);
}
int sd_clip_vision_memory(const sd_clip_vision* c, int64_t* weight_bytes, int64_t* workspace_bytes) {
    if (!c) { set_error("null handle"); return SD_ERR_INVALID; }
    if (weight_bytes) *weight_bytes = c->impl.ws.packed_bytes();
    if (workspace_bytes) *workspace_bytes = (int64_t)c->impl.arena.capacity();
    return SD_OK;
}
int sd_op_vit_patch_embed(const void* pixels, const void* w, const void* class_embedding, const void* position_embedding,
                          void* out, int64_t ld_out, int B, int image_size, int patch_size, int hidden, void* stream) {
    if (!pixels || !w || !class_embedding || !position_embedding || !out ||
        (reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(position_embedding)) % 16 != 0) {
        set_error("sd_op_vit_patch_embed: null or misaligned argument (out and position_embedding 16-byte aligned)");
        return SD_ERR_INVALID;
    }
    return launch_vit_patch_embed(static_cast<const half_t*>(pixels), static_cast<const half_t*>(w),
                                  static_cast<const half_t*>(class_embedding), static_cast<const half_t*>(position_embedding),
                                  static_cast<half_t*>(out), (long)ld_out, B, image_size, patch_size, hidden,
                                  static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------- step glue
int sd_cfg_duplicate(const void* latents, void* out2b, int64_t n_per_batch, int B, float in_scale, void* stream) {
    if (!latents || !out2b) { set_error("null argument"); return SD_ERR_INVALID; }
    return launch_cfg_duplicate(static_cast<const half_t*>(latents), static_cast<half_t*>(out2b),
                                (long)n_per_batch * B, in_scale, static_cast<hipStream_t>(stream));
}
int sd_cfg_linear_step(const void* noise_pred_2b, void* latents, float* hist_f32, int64_t n, float guidance_scale,
                       float c_x, float c_eps, float c_hist, float h_x, float h_eps, void* stream) {
    if (!noise_pred_2b || !latents || n < 0) { set_error("sd_cfg_linear_step: bad arguments"); return SD_ERR_INVALID; }
    return launch_cfg_linear(static_cast<const half_t*>(noise_pred_2b), static_cast<half_t*>(latents), hist_f32, (long)n,
                             guidance_scale, c_x, c_eps, c_hist, h_x, h_eps, static_cast<hipStream_t>(stream));
}
int sd_cfg_rescale_linear_step(const void* noise_pred_2b, void* latents, float* hist_f32, int B, int64_t n_per_sample,
                               float guidance_scale, float guidance_rescale, float c_x, float c_eps, float c_hist, float h_x,
                               float h_eps, float* factors_out, void* stream) {
    if (!noise_pred_2b || !latents || B < 1 || n_per_sample < 2) {
        set_error("sd_cfg_rescale_linear_step: bad arguments (non-null tensors, B >= 1, n_per_sample >= 2)");
        return SD_ERR_INVALID;
    }
    return launch_cfg_rescale_linear(static_cast<const half_t*>(noise_pred_2b), static_cast<half_t*>(latents), hist_f32, B,
                                     (long)n_per_sample, guidance_scale, guidance_rescale, c_x, c_eps, c_hist, h_x, h_eps,
                                     factors_out, static_cast<hipStream_t>(stream));
}
int sd_pag_linear_step(const void* model_out, int rows, void* latents, float* hist_f32, int64_t n, float guidance_scale,
                       float pag_scale, float c_x, float c_eps, float c_hist, float h_x, float h_eps, void* stream) {
    if (!model_out || !latents || (rows != 2 && rows != 3) || n <= 0 || !std::isfinite(guidance_scale) || !std::isfinite(pag_scale)) {
        set_error("sd_pag_linear_step: bad arguments (non-null model_out / latents, rows 2 or 3, n > 0, finite scales)");
        return SD_ERR_INVALID;
    }
    return launch_pag_linear(static_cast<const half_t*>(model_out), rows, static_cast<half_t*>(latents), hist_f32, (long)n,
                             guidance_scale, pag_scale, c_x, c_eps, c_hist, h_x, h_eps, static_cast<hipStream_t>(stream));
}
int sd_pag_combine(const void* model_out, int rows, void* out_f16, int64_t n, float guidance_scale, float pag_scale,
                   void* stream) {
    if (!model_out || !out_f16 || (rows != 2 && rows != 3) || n <= 0 || !std::isfinite(guidance_scale) || !std::isfinite(pag_scale)) {
        set_error("sd_pag_combine: bad arguments (non-null model_out / out_f16, rows 2 or 3, n > 0, finite scales)");
        return SD_ERR_INVALID;
    }
    return launch_pag_combine(static_cast<const half_t*>(model_out), rows, static_cast<half_t*>(out_f16), (long)n,
                              guidance_scale, pag_scale, static_cast<hipStream_t>(stream));
}
int sd_ip2p_linear_step(const void* model_out, void* latents, float* hist_f32, int64_t n, float guidance_scale,
                        float image_guidance_scale, float c_x, float c_eps, float c_hist, float h_x, float h_eps, void* stream) {
    if (!model_out || !latents || n <= 0 || !std::isfinite(guidance_scale) || !std::isfinite(image_guidance_scale)) {
        set_error("sd_ip2p_linear_step: bad arguments (non-null model_out / latents, n > 0, finite scales)");
        return SD_ERR_INVALID;
    }
    return launch_ip2p_linear(static_cast<const half_t*>(model_out), static_cast<half_t*>(latents), hist_f32, (long)n,
                              guidance_scale, image_guidance_scale, c_x, c_eps, c_hist, h_x, h_eps, static_cast<hipStream_t>(stream));
}
int sd_ip2p_combine(const void* model_out, void* out_f16, int64_t n, float guidance_scale, float image_guidance_scale,
                    void* stream) {
    if (!model_out || !out_f16 || n <= 0 || !std::isfinite(guidance_scale) || !std::isfinite(image_guidance_scale)) {
        set_error("sd_ip2p_combine: bad arguments (non-null model_out / out_f16, n > 0, finite scales)");
        return SD_ERR_INVALID;
    }
    return launch_ip2p_combine(static_cast<const half_t*>(model_out), static_cast<half_t*>(out_f16), (long)n, guidance_scale,
                               image_guidance_scale, static_cast<hipStream_t>(stream));
}
int sd_lcm_step(const void* model_out, int rows, void* latents, const void* noise, void* denoised, int64_t n,
                float guidance_scale, float d_x, float d_out, float p_den, float p_noise, void* stream) {
    if (!model_out || !latents || (rows != 1 && rows != 2) || n <= 0) {
        set_error("sd_lcm_step: bad arguments (non-null model_out / latents, rows 1 or 2, n > 0)");
        return SD_ERR_INVALID;
    }
    if (!noise && p_noise != 0.f) { set_error("sd_lcm_step: p_noise != 0 needs a noise tensor"); return SD_ERR_INVALID; }
    return launch_lcm_step(static_cast<const half_t*>(model_out), rows, static_cast<half_t*>(latents),
                           static_cast<const half_t*>(noise), static_cast<half_t*>(denoised), (long)n, guidance_scale, d_x,
                           d_out, p_den, p_noise, static_cast<hipStream_t>(stream));
}
int sd_sched_affine_step(const void* model_out, int rows, void* latents, const void* noise, float* bank,
                         int64_t bank_stride, int64_t n, float guidance_scale, const sd_step_plan* plan, void* stream) {
    static_assert(STEP_SLOTS == SD_STEP_MAX_SLOTS && STEP_WRITES == SD_STEP_MAX_WRITES, "sd_step_plan and StepRows differ");
    if (!model_out || !latents || !plan || (rows != 1 && rows != 2) || n <= 0) {
        set_error("sd_sched_affine_step: bad arguments (non-null model_out / latents / plan, rows 1 or 2, n > 0)");
        return SD_ERR_INVALID;
    }
    const int ns = plan->n_slots, nw = plan->n_writes;
    if (ns < 0 || ns > SD_STEP_MAX_SLOTS || nw < 0 || nw > SD_STEP_MAX_WRITES) {
        set_error("sd_sched_affine_step: n_slots must be 0..4 and n_writes 0..2");
        return SD_ERR_INVALID;
    }
    for (int j = 0; j < nw; ++j)
        if (plan->write_slot[j] < 0 || plan->write_slot[j] >= ns || (j == 1 && plan->write_slot[1] == plan->write_slot[0])) {
            set_error("sd_sched_affine_step: write_slot must be distinct slots below n_slots");
            return SD_ERR_INVALID;
        }
    if (ns > 0 && (!bank || bank_stride < n)) {
        set_error("sd_sched_affine_step: n_slots > 0 needs a bank with bank_stride >= n");
        return SD_ERR_INVALID;
    }
    StepRows r = {};                                   // the used rows and columns; everything else stays 0
    r.n_writes = nw;
    for (int j = 0; j < nw; ++j) r.write_slot[j] = plan->write_slot[j];
    bool finite = true, z_used = false;
    for (int row = 0; row <= nw; ++row) {
        const double* src = row == 0 ? plan->out : plan->write[row - 1];
        double* dst = row == 0 ? r.out : r.write[row - 1];
        for (int k = 0; k < 3 + ns; ++k) {
            dst[k] = src[k];
            finite = finite && std::isfinite(src[k]);
        }
        z_used = z_used || dst[2] != 0.0;
    }
    if (!finite) { set_error("sd_sched_affine_step: a coefficient of a used row is not finite"); return SD_ERR_INVALID; }
    if (z_used && !noise) { set_error("sd_sched_affine_step: a non-zero noise coefficient needs a noise tensor"); return SD_ERR_INVALID; }
    return launch_sched_affine_step(static_cast<const half_t*>(model_out), rows, static_cast<half_t*>(latents),
                                    static_cast<const half_t*>(noise), bank, (long)bank_stride, (long)n, guidance_scale, r,
                                    static_cast<hipStream_t>(stream));
}
int sd_images_to_uint8(const void* images_nchw_f16, void* out_nhwc_u8, int B, int C, int H, int W, void* stream) {
    if (!images_nchw_f16 || !out_nhwc_u8 || B < 0 || C < 1 || C > 4 || H < 1 || W < 1) {
        set_error("sd_images_to_uint8: bad arguments (1..4 channels)");
        return SD_ERR_INVALID;
    }
    return launch_image_to_uint8(static_cast<const half_t*>(images_nchw_f16), static_cast<unsigned char*>(out_nhwc_u8), B, C,
                                 (long)H * W, static_cast<hipStream_t>(stream));
}
int sd_inpaint_blend(void* latents, const void* image_latents, const void* noise, const void* mask, float a, float b,
                     int B, int C, int H, int W, void* stream) {
    if (!latents || !image_latents || !mask || B < 0 || C < 1 || H < 1 || W < 1) {
        set_error("sd_inpaint_blend: bad arguments");
        return SD_ERR_INVALID;
    }
    return launch_inpaint_blend(static_cast<half_t*>(latents), static_cast<const half_t*>(image_latents),
                                static_cast<const half_t*>(noise), static_cast<const half_t*>(mask), a, b, B, C,
                                (long)H * W, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------- MultiDiffusion views
int sd_view_plan(int L, int win, int stride, int wrap, int* starts, int cap) {
    if (L < 1 || win < 1 || stride < 1 || !starts || cap < 1) {
        set_error("sd_view_plan: bad arguments (L, win, stride, cap >= 1, non-null starts)");
        return -SD_ERR_INVALID;
    }
    if (wrap && win > L) { set_error("sd_view_plan: a wrapped axis needs win <= L"); return -SD_ERR_INVALID; }
    if (stride > win) stride = win;                  // (a larger stride would leave gaps: the windows abut instead)
    long count;                                      // every start is a multiple of the stride, but for a final L - win
    bool tail = false;
    if (wrap) count = ((long)L + stride - 1) / stride;
    else if (L <= win) count = 1;
    else {
        count = (long)(L - win) / stride + 1;
        tail = (L - win) % stride != 0;
        count += tail;
    }
    if (count > VIEW_MAX_STARTS) { set_error("sd_view_plan: more than 64 starts on one axis"); return -SD_ERR_INVALID; }
    if (count > cap) { set_error("sd_view_plan: `starts` is too small"); return -SD_ERR_INVALID; }
    for (int i = 0; i < (int)count; ++i) starts[i] = i * stride;
    if (tail) starts[count - 1] = L - win;
    return (int)count;
}

namespace {
// The starts of one axis into `dst`, checked: 1..64 of them, each window inside the axis (or, wrapped, starting inside it),
// every position covered.
const char* check_view_axis(const int* starts, int n, int win, int L, bool wrap, int* dst) {
    if (n < 1 || n > VIEW_MAX_STARTS) return "1..64 starts per axis";
    if (win < 1 || win > L) return "a window must fit the canvas (1 <= h <= Hc, 1 <= w <= Wc)";
    std::vector<char> covered((size_t)L, 0);
    for (int i = 0; i < n; ++i) {
        const int s = starts[i];
        if (s < 0 || s >= L || (!wrap && s > L - win)) return "a start outside the canvas";
        for (int k = 0; k < win; ++k) covered[(size_t)((s + k) % L)] = 1;
        dst[i] = s;
    }
    for (int p = 0; p < L; ++p)
        if (!covered[(size_t)p]) return "a pixel that no view covers";
    return nullptr;
}
}  // namespace

int sd_views_gather(const void* canvas, void* windows, int B, int C, int Hc, int Wc, int h, int w, const int* ys, int ny,
                    const int* xs, int nx, int wrap_x, void* stream) {
    if (!canvas || !windows || !ys || !xs || B < 1 || C < 1 || Hc < 1 || Wc < 1) {
        set_error("sd_views_gather: bad arguments (non-null canvas / windows / ys / xs, positive sizes)");
        return SD_ERR_INVALID;
    }
    ViewStarts st = {};
    const char* why = check_view_axis(ys, ny, h, Hc, false, st.ys);
    if (!why) why = check_view_axis(xs, nx, w, Wc, wrap_x != 0, st.xs);
    if (why) { set_error(std::string("sd_views_gather: ") + why); return SD_ERR_INVALID; }
    return launch_views_gather(static_cast<const half_t*>(canvas), static_cast<half_t*>(windows), B, C, Hc, Wc, h, w, st, ny,
                               nx, wrap_x != 0, static_cast<hipStream_t>(stream));
}

int sd_views_merge(const void* model_out, void* eps_out, const float* window_weights, int G, int B, int C, int Hc, int Wc,
                   int h, int w, const int* ys, int ny, const int* xs, int nx, int wrap_x, int views_per_chunk, void* stream) {
    if (!model_out || !eps_out || !ys || !xs || G < 1 || B < 1 || C < 1 || Hc < 1 || Wc < 1 || views_per_chunk < 1) {
        set_error("sd_views_merge: bad arguments (non-null model_out / eps_out / ys / xs, positive sizes, "
                  "views_per_chunk >= 1)");
        return SD_ERR_INVALID;
    }
    ViewStarts st = {};
    const char* why = check_view_axis(ys, ny, h, Hc, false, st.ys);
    if (!why) why = check_view_axis(xs, nx, w, Wc, wrap_x != 0, st.xs);
    if (why) { set_error(std::string("sd_views_merge: ") + why); return SD_ERR_INVALID; }
    return launch_views_merge(static_cast<const half_t*>(model_out), static_cast<half_t*>(eps_out), window_weights, G, B, C,
                              Hc, Wc, h, w, st, ny, nx, wrap_x != 0, views_per_chunk, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------- probe
int sd_probe_mfma(int iters, float* tflops, void* stream) {
    if (iters < 1 || !tflops) { set_error("sd_probe_mfma: bad arguments"); return SD_ERR_INVALID; }
    return probe_mfma(iters, tflops, static_cast<hipStream_t>(stream));
}
int sd_probe_lds_dma(int64_t region_bytes, int passes, int depth, int shared, float* gbs, void* stream) {
    if (!gbs) { set_error("sd_probe_lds_dma: bad arguments"); return SD_ERR_INVALID; }
    return probe_dma((long)region_bytes, passes, depth, shared, gbs, static_cast<hipStream_t>(stream));
}
int sd_probe_copy(int64_t bytes, int iters, float* gbs, void* stream) {
    if (bytes < 4096 || iters < 1 || !gbs) { set_error("sd_probe_copy: bad arguments"); return SD_ERR_INVALID; }
    return probe_copy((long)bytes, iters, gbs, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------ tuning
int sd_igemm_force(int variant, int splits) { igemm2_force(variant, splits); return SD_OK; }

// The problem and the requests the plan entries describe by geom[9] / flags[10] (include/sd_engine.h: sd_igemm_plan).  An
// operand that is "present" is a dummy non-null pointer: the planner only asks whether one is set.
static int plan_problem(const char* entry, const int* geom, const int* flags, const void* out, const void* name,
                        IGemmParams* problem, IGemmRequest* rq) {
    if (!geom || !flags || !out || !name) { set_error(std::string(entry) + ": null argument"); return SD_ERR_INVALID; }
    const int N = geom[0], H = geom[1], W = geom[2], Cin = geom[3], Cout = geom[4], ks = geom[5], stride = geom[6], up = geom[7];
    if (N < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || (ks != 1 && ks != 3) || stride < 1 || up < 0 || up > 1) {
        set_error(std::string(entry) + ": bad geometry"); return SD_ERR_INVALID;
    }
    float* const set = reinterpret_cast<float*>(8);
    const half_t* const seth = reinterpret_cast<const half_t*>(set);
    IGemmParams p = conv_problem(N, H, W, Cin, Cout, ks, stride, up, geom[8]);
    p.x = seth; p.ldx = Cin; p.w = seth; p.y = reinterpret_cast<half_t*>(set);
    p.geglu = flags[0]; p.act = flags[1];
    p.ldy = p.geglu ? Cout / 2 : Cout;
    if (flags[2]) { p.res = seth; p.ldres = p.ldy; }
    if (flags[3]) { p.rowadd = set; p.rowadd_ld = Cout; }
    if (flags[4]) p.bias = set;
    if (flags[5] > 0) { p.ln_stat = set; p.ln_parts = flags[5]; p.ln_part_w = (p.K + flags[5] - 1) / flags[5]; p.ln_C = p.K; p.ln_eps = 1e-5f; p.ln_wsum = set; }
    if (flags[8] > 0) { p.gni_part = set; p.gni_S = 1; p.gni_rows = (long)H * W; p.gni_groups = flags[8]; p.gni_eps = 1e-5f; p.gni_gb = set; }
    if (flags[9]) { p.acc_scale = 0.5f; p.bias_scale = 0.5f; }
    *problem = p;
    *rq = IGemmRequest{flags[6] ? set : nullptr, flags[7] > 0 ? set : nullptr, flags[7]};
    return SD_OK;
}

static int plan_answer(const IGemmPlan& pl, int64_t* out, char* name) {
    if (pl.kind == kKindBadVariant) return SD_ERR_INVALID;
    const int64_t o[12] = {pl.kind, pl.variant, pl.splits, pl.partial_floats, pl.rowstats, pl.rs_parts, pl.rs_part_w,
                           pl.gnstats, pl.gn_rows, pl.scales_ok, pl.bm, pl.bn};
    for (int i = 0; i < 12; ++i) out[i] = o[i];
    snprintf(name, 64, "%s", pl.name);
    return SD_OK;
}

int sd_igemm_plan(const int* geom, const int* flags, int64_t* out, char* name) {
    IGemmParams p;
    IGemmRequest rq;
    if (int rc = plan_problem("sd_igemm_plan", geom, flags, out, name, &p, &rq)) return rc;
    return plan_answer(igemm2_plan(p, rq), out, name);
}

int sd_conv_plan(const int* geom, const int* flags, int have_fold, int cus, int64_t* out, char* name) {
    IGemmParams p;
    IGemmRequest rq;
    if (int rc = plan_problem("sd_conv_plan", geom, flags, out, name, &p, &rq)) return rc;
    if (cus < 0) { set_error("sd_conv_plan: bad geometry"); return SD_ERR_INVALID; }
    return plan_answer(conv_plan(p, have_fold ? p.w : nullptr, rq, cus), out, name);
}

int sd_halo80_force(int mode) { halo80_force(mode); return SD_OK; }

int sd_halo80_plan(const int* geom, const int* flags, int cus, int64_t* out, char* name) {
    IGemmParams p;
    IGemmRequest rq;
    if (int rc = plan_problem("sd_halo80_plan", geom, flags, out, name, &p, &rq)) return rc;
    if (cus < 0) { set_error("sd_halo80_plan: bad geometry"); return SD_ERR_INVALID; }
    // the second stage's answer alone: conv_plan without a folded pack, and nothing where the table's row stays
    const IGemmPlan pl = conv_plan(p, nullptr, rq, cus);
    const bool ok = pl.kind == kKindHalo80;
    const int64_t o[6] = {ok, ok ? pl.bn : 0, ok ? pl.splits : 1, ok && pl.gnstats, ok ? pl.gn_rows : 0, ok ? pl.partial_floats : 0};
    for (int i = 0; i < 6; ++i) out[i] = o[i];
    snprintf(name, 64, "%s", ok ? pl.name : "");
    return SD_OK;
}

// --------------------------------------------------------------------------------------- profiling
int sd_prof_enable(int on) { prof_enable(on != 0); return SD_OK; }
int sd_prof_collect(sd_prof_entry* out, int max_entries, int* n_entries) {
    if (!out || !n_entries) { set_error("null argument"); return SD_ERR_INVALID; }
    std::map<std::string, ProfAgg> agg;
    int rc = prof_collect(&agg);
    if (rc) return rc;
    int n = 0;
    for (const auto& kv : agg) {
        if (n >= max_entries) break;
        sd_prof_entry& e = out[n++];
        snprintf(e.kernel, sizeof(e.kernel), "%s", kv.first.c_str());
        e.flops = kv.second.flops; e.bytes = kv.second.bytes; e.ms = kv.second.ms; e.launches = kv.second.launches;
    }
    *n_entries = n;
    return SD_OK;
}

// ------------------------------------------------------------------------- single-operator entries
// Test / tuner path only: packs the weight on every call (allocation + sync); never used by the models.  The entries
// pack with the engine's packers (a local WeightStore owns the packed buffers and frees them on every return path) and
// run through the engine's op wrappers on a private arena, so they exercise the host code a forward runs.

}  // extern "C"

namespace {
// Two untimed calls of `launch`, then `iters` of them between two events on `s`: *ms = milliseconds per call.
template <class F>
int time_launches(hipStream_t s, int iters, float* ms, F launch) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = 0;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { set_error("hipEventCreate failed"); rc = SD_ERR_HIP; }
    for (int it = 0; it < 2 && !rc; ++it) rc = launch();
    if (!rc) (void)hipEventRecord(e0, s);
    for (int it = 0; it < iters && !rc; ++it) rc = launch();
    if (!rc) {
        float t = 0.f;
        hipError_t e = hipEventRecord(e1, s);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
        if (e != hipSuccess) { set_error(hipGetErrorString(e)); rc = SD_ERR_HIP; }
        *ms = t / (float)iters;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return rc;
}

// `launch` once, or timed when iters > 0 and there is somewhere to put the figure; then waits for the stream.
template <class F>
int launch_or_time(hipStream_t s, int iters, float* ms, F launch) {
    int rc = iters > 0 && ms ? time_launches(s, iters, ms, launch) : launch();
    const hipError_t e = hipStreamSynchronize(s);
    if (!rc && e != hipSuccess) { set_error(hipGetErrorString(e)); rc = SD_ERR_HIP; }
    return rc;
}

// Runs `body(ctx)` once as a planning pass and then for real on a private arena (the op entries' workspace): once, or
// timed (time_launches) with iters > 0.
template <class F>
int run_op_on_arena(hipStream_t s, int iters, float* ms, F body) {
    if (iters > 0 && !ms) { set_error("ms_per_launch required with iters > 0"); return SD_ERR_INVALID; }
    Arena arena;
    Ctx dry{&arena, s, true};
    arena.begin(true);
    body(dry);
    if (dry.err) return dry.err;
    if (int rc = arena.reserve(arena.peak() > 0 ? arena.peak() : 256)) return rc;
    return launch_or_time(s, iters, ms, [&]() {
        Ctx c{&arena, s, false};
        arena.begin(false);
        body(c);
        return c.err;
    });
}

// The entries' operands as the packers take them.  The packers work on the null stream, so an entry waits for its own
// stream first (pack_begin) and for the device afterwards (pack_end).  Biases, gamma and beta arrive as fp32 device
// arrays and reach the packers as fp32 host arrays: nothing rounds them on the way.  A null bias packs as zeros.
int pack_begin(hipStream_t s) { SD_HIP_CHECK(hipStreamSynchronize(s)); return 0; }
int pack_end() { SD_HIP_CHECK(hipDeviceSynchronize()); return 0; }

int host_f32(const void* dev_f32, long n, std::vector<float>* out) {
    out->assign((size_t)n, 0.f);
    if (dev_f32) SD_HIP_CHECK(hipMemcpy(out->data(), dev_f32, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

// w [O][I][ks][ks] f16; geglu: a [hidden | gate] linear, interleaved per 64 rows; fold_up2x: also the folded pack
int pack_conv_op(WeightStore& ws, const void* w, int O, int I, int ks, const void* bias_f32, bool geglu, bool fold_up2x,
                 ConvW* out) {
    std::vector<float> b;
    if (int rc = host_f32(bias_f32, O, &b)) return rc;
    const half_t* wh = static_cast<const half_t*>(w);
    return geglu ? ws.pack_geglu(wh, O, I, b.data(), out) : ws.pack_conv(wh, O, I, ks, ks, b.data(), out, fold_up2x);
}

int pack_norm_op(WeightStore& ws, const void* gamma_f32, const void* beta_f32, int C, NormW* out) {
    std::vector<float> g, b;
    if (int rc = host_f32(gamma_f32, C, &g)) return rc;
    if (int rc = host_f32(beta_f32, C, &b)) return rc;
    return ws.pack_norm(g.data(), b.data(), C, out);
}

View view_of(const void* p, long ld, int C) { return View(const_cast<half_t*>(static_cast<const half_t*>(p)), ld, C); }

// What the conv entries add to the plain sd_op_conv2d; everything is optional.
struct ConvOpts {
    long ldx = 0, ldres = 0, ldy = 0;       // operand strides in elements (0: dense)
    ConvArgs conv;                          // pad, act, acc_scale, bias_scale; conv2d_impl fills in the rest
    // GroupNorm summaries asked of the launch (they pick the split-K reduction kernel), kept for the call only ...
    int gn_groups = 0;
    float* gn_copy = nullptr;               // ... or copied out (sd_op_conv2d_gnstats; gn_copy_floats at most)
    long gn_copy_floats = 0;
    int* gn_rows = nullptr;                 // the pixels per summary (0: none left)
    int* ran = nullptr;                     // kind, variant, split-K slices launched, reduction kernel
    // A GroupNorm (+ SiLU) of norm_groups groups behind the convolution (sd_op_conv2d_groupnorm: y_gn receives it; the
    // conv is asked for its summaries, *fused = it left them) or in front of it (sd_op_groupnorm_conv2d: inside the
    // convolution where the launch takes it, *fused = 1, a GroupNorm kernel first otherwise).
    enum { kNoNorm, kNormBehind, kNormInFront } norm = kNoNorm;
    const void *gamma = nullptr, *beta = nullptr;
    int norm_groups = 0, silu = 0;
    float eps = 0.f;
    void* y_gn = nullptr;
    int* fused = nullptr;
    // timing: `iters` launches of the convolution alone between events, after two warm-ups
    int iters = 0;
    float* ms = nullptr;
};

int conv2d_impl(const void* x, const void* w_oihw, const void* bias_f32, const void* rowadd_f32, const void* res, void* y,
                int N, int H, int W, int Cin, int Cout, int ksize, int stride, int upsample2x, int geglu, void* stream,
                const ConvOpts& o = ConvOpts()) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if ((long)ksize * ksize * Cin % 64 != 0 || Cin % 64 != 0) { set_error("sd_op_conv2d: Cin must be a multiple of 64"); return SD_ERR_INVALID; }
    if (geglu && ksize != 1) { set_error("sd_op_conv2d: GEGLU takes a linear (ksize 1)"); return SD_ERR_INVALID; }
    if (o.fused) *o.fused = 0;
    const bool behind = o.norm == ConvOpts::kNormBehind, in_front = o.norm == ConvOpts::kNormInFront;
    const IGemmParams geo = conv_problem(N, H, W, Cin, Cout, ksize, stride, upsample2x, o.conv.pad);    // (the output map)
    const long HW = (long)H * W, OHW = (long)geo.OH * geo.OW;
    const int ocols = geglu ? Cout / 2 : Cout;
    const int gn_groups = behind ? o.norm_groups : o.gn_groups;
    if (int rc = pack_begin(s)) return rc;
    WeightStore ws;
    ConvW cw;                               // (no folded pack: an upsampling launch here runs the 9-tap kernels)
    NormW nw;
    int rc = pack_conv_op(ws, w_oihw, Cout, Cin, ksize, bias_f32, geglu != 0, false, &cw);
    if (!rc && o.norm) rc = pack_norm_op(ws, o.gamma, o.beta, in_front ? Cin : Cout, &nw);
    if (rc) return rc;
    GnStatBuf gb;
    if (gn_groups > 0 && !(gb.buf = static_cast<float*>(ws.dmalloc((size_t)gnstat_floats(N, OHW, gn_groups) * sizeof(float))))) {
        set_error("hipMalloc failed (GroupNorm summaries)"); return SD_ERR_HIP;
    }
    // SD_BENCH_RES=1 (tuner): time the launch with the fused residual add
    if (o.ms && !res && getenv("SD_BENCH_RES")) {
        const size_t bytes = (size_t)geo.M * ocols * sizeof(half_t);
        void* zero = ws.dmalloc(bytes);
        if (!zero) { set_error("hipMalloc failed (SD_BENCH_RES)"); return SD_ERR_HIP; }
        SD_HIP_CHECK(hipMemsetAsync(zero, 0, bytes, 0));
        res = zero;
    }
    // SD_BENCH_COLD_MB=<n> (tuner): rotate through copies of the packed weights totalling n MB, so
    // every timed launch streams its weights from HBM as it does inside a UNet forward (1.7 GB of
    // weights per forward never stay in the 256 MB Infinity Cache); unset = same buffer every launch.
    char* wring = nullptr;
    long nrot = 1;
    const size_t wbytes = (size_t)weight_rows(Cout) * cw.K * sizeof(half_t);
    const char* cold = o.ms ? getenv("SD_BENCH_COLD_MB") : nullptr;
    if (cold && atol(cold) > 0) {
        nrot = std::min((atol(cold) * 1000000L + (long)wbytes - 1) / (long)wbytes, (long)o.iters + 2);
        if (nrot > 1) {
            if (!(wring = static_cast<char*>(ws.dmalloc(wbytes * (size_t)nrot)))) { set_error("hipMalloc failed (SD_BENCH_COLD_MB)"); return SD_ERR_HIP; }
            for (long r = 0; r < nrot; ++r)
                SD_HIP_CHECK(hipMemcpyAsync(wring + wbytes * (size_t)r, cw.w, wbytes, hipMemcpyDeviceToDevice, 0));
        }
    }
    if ((rc = pack_end())) return rc;

    const View xv = view_of(x, o.ldx ? o.ldx : Cin, Cin), rv = view_of(res, o.ldres ? o.ldres : ocols, ocols);
    const View yv = view_of(y, o.ldy ? o.ldy : ocols, ocols);
    ConvLaunch l;
    bool fused_in_front = false;
    rc = run_op_on_arena(s, 0, nullptr, [&](Ctx& c) {
        ConvArgs f = o.conv;
        f.stride = stride; f.up = upsample2x; f.geglu = geglu;
        f.rowadd = static_cast<const float*>(rowadd_f32); f.rowadd_ld = Cout;
        f.res = rv;
        f.gn_out = gb.buf ? &gb : nullptr; f.gn_groups = gn_groups;
        View cx = xv;                       // what the convolution reads: x, or the output of a GroupNorm kernel in front
        if (in_front && !(fused_in_front = op_gn_conv_fused(c, nw, cw, xv, N, H, W, yv, o.norm_groups, o.eps, o.silu, nullptr, f, &l))) {
            cx = View(c.arena->alloc_h((long)N * HW * Cin), Cin, Cin);
            op_groupnorm(c, nw, xv, cx, N, HW, o.norm_groups, o.eps, o.silu);
        }
        if (!fused_in_front) conv_prepare(c, cw, cx, N, H, W, yv, f, &l);
        if (!c.dry && !c.err) {
            if (o.ms) {                     // the plan is made once: a timed launch costs the host what it costs a forward
                long it = 0;
                c.err = time_launches(s, o.iters, o.ms, [&]() {
                    if (wring) l.p.w = reinterpret_cast<half_t*>(wring + wbytes * (size_t)(it++ % nrot));
                    return launch_igemm2(l.p, l.partial, s, &l.plan);
                });
            } else {
                conv_launch(c, l, yv, nullptr);
            }
        }
        if (behind) op_groupnorm(c, nw, yv, view_of(o.y_gn, Cout, Cout), N, OHW, o.norm_groups, o.eps, o.silu, &gb);
    });
    if (rc) return rc;
    if (o.ran) {
        const IGemmLaunchNote note = igemm2_last_launch();
        o.ran[0] = l.plan.kind; o.ran[1] = l.plan.variant; o.ran[2] = note.splits; o.ran[3] = note.reducer;
    }
    if (o.fused) *o.fused = behind ? gb.st.part != nullptr : fused_in_front;
    if (o.gn_rows) {
        *o.gn_rows = gb.st.part ? (int)gb.st.rows : 0;
        const long n = std::min(gnstat_floats(N, OHW, gn_groups), o.gn_copy_floats);
        if (gb.st.part && o.gn_copy && n > 0) SD_HIP_CHECK(hipMemcpy(o.gn_copy, gb.st.part, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice));
        SD_HIP_CHECK(hipDeviceSynchronize());
    }
    return SD_OK;
}
}  // namespace

extern "C" {

int sd_op_conv2d(const void* x, const void* w_oihw, const void* bias_f32, const void* rowadd_f32, const void* res,
                 void* y, int N, int H, int W, int Cin, int Cout, int ksize, int stride, int upsample2x,
                 int geglu, void* stream) {
    return conv2d_impl(x, w_oihw, bias_f32, rowadd_f32, res, y, N, H, W, Cin, Cout, ksize, stride, upsample2x, geglu, stream);
}

int sd_op_conv2d_ex(const void* x, const void* w_oihw, const void* bias_f32, const void* rowadd_f32, const void* res,
                    void* y, int N, int H, int W, int Cin, int Cout, int ksize, int stride, int upsample2x, int geglu,
                    int64_t ldx, int64_t ldres, int64_t ldy, int pad, int act, float acc_scale, float bias_scale,
                    int gn_groups, int* ran, void* stream) {
    if (!x || !w_oihw || !y || !ran || N < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || (ksize != 1 && ksize != 3) ||
        stride < 1 || upsample2x < 0 || upsample2x > 1 || (geglu && Cout % 2 != 0)) {
        set_error("sd_op_conv2d_ex: bad arguments"); return SD_ERR_INVALID;
    }
    const int ocols = geglu ? Cout / 2 : Cout;
    // a stride is the dense width or a wider multiple of 8 elements (the kernels move 16-byte chunks)
    auto ld_ok = [](int64_t ld, int dense) { return ld == dense || (ld > dense && ld % 8 == 0); };
    if (!ld_ok(ldx, Cin) || !ld_ok(ldy, ocols) || (res && !ld_ok(ldres, ocols))) {
        set_error("sd_op_conv2d_ex: ldx / ldres / ldy must be the dense width or a wider multiple of 8"); return SD_ERR_INVALID;
    }
    if (pad < -1 || pad > 1 || act < 0 || act > 2 || gn_groups < 0 || !(acc_scale > 0.f) || !(bias_scale > 0.f)) {
        set_error("sd_op_conv2d_ex: pad in -1..1, act in 0..2, positive scales"); return SD_ERR_INVALID;
    }
    for (int i = 0; i < 4; ++i) ran[i] = 0;
    ConvOpts o;
    o.ldx = (long)ldx; o.ldres = res ? (long)ldres : 0; o.ldy = (long)ldy;
    o.conv.pad = pad; o.conv.act = act; o.conv.acc_scale = acc_scale; o.conv.bias_scale = bias_scale;
    o.gn_groups = gn_groups; o.ran = ran;
    return conv2d_impl(x, w_oihw, bias_f32, rowadd_f32, res, y, N, H, W, Cin, Cout, ksize, stride, upsample2x, geglu, stream, o);
}

int sd_op_conv2d_gnstats(const void* x, const void* w_oihw, const void* bias_f32, const void* res, void* y, int N, int H,
                         int W, int Cin, int Cout, int ksize, int gn_groups, float* summaries, int64_t summaries_floats,
                         int* rows, int* ran, void* stream) {
    if (!x || !w_oihw || !y || !summaries || !rows || !ran || N < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 ||
        (ksize != 1 && ksize != 3) || gn_groups < 1 || summaries_floats < 0) {
        set_error("sd_op_conv2d_gnstats: bad arguments"); return SD_ERR_INVALID;
    }
    for (int i = 0; i < 4; ++i) ran[i] = 0;
    *rows = 0;
    ConvOpts o;
    o.gn_groups = gn_groups; o.ran = ran;
    o.gn_copy = summaries; o.gn_copy_floats = (long)summaries_floats; o.gn_rows = rows;
    return conv2d_impl(x, w_oihw, bias_f32, nullptr, res, y, N, H, W, Cin, Cout, ksize, 1, 0, 0, stream, o);
}

int sd_op_conv3x3_small_cout(const void* x, const void* w_oihw, const void* bias_f32, void* y_nchw, int N, int H, int W,
                             int Cin, int Cout, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (Cin % 64 != 0 || Cout < 1 || Cout > 4) { set_error("sd_op_conv3x3_small_cout: Cin % 64 == 0, Cout in 1..4"); return SD_ERR_INVALID; }
    if (int rc = pack_begin(s)) return rc;
    WeightStore ws;
    ConvW cw;                               // (the kernel reads the caller's bias as it is)
    int rc = ws.pack_conv(static_cast<const half_t*>(w_oihw), Cout, Cin, 3, 3, nullptr, &cw);
    if (rc || (rc = pack_end())) return rc;
    return launch_or_time(s, 0, nullptr, [&]() {
        return launch_conv3x3_small_cout(static_cast<const half_t*>(x), Cin, cw.w, cw.K, static_cast<const float*>(bias_f32),
                                         static_cast<half_t*>(y_nchw), N, H, W, Cin, Cout, s);
    });
}

int sd_op_conv2d_groupnorm(const void* x, const void* w_oihw, const void* bias_f32, const void* rowadd_f32, const void* res,
                           void* y_conv, const void* gamma_f32, const void* beta_f32, void* y_gn, int N, int H, int W,
                           int Cin, int Cout, int ksize, int stride, int upsample2x, int groups, float eps, int silu,
                           int* stats_from_epilogue, void* stream) {
    ConvOpts o;
    o.norm = ConvOpts::kNormBehind;
    o.gamma = gamma_f32; o.beta = beta_f32; o.norm_groups = groups; o.eps = eps; o.silu = silu;
    o.y_gn = y_gn; o.fused = stats_from_epilogue;
    return conv2d_impl(x, w_oihw, bias_f32, rowadd_f32, res, y_conv, N, H, W, Cin, Cout, ksize, stride, upsample2x, 0, stream, o);
}

int sd_op_groupnorm_conv2d(const void* x, const void* gamma_f32, const void* beta_f32, int groups, float eps, int silu,
                           const void* w_oihw, const void* bias_f32, const void* rowadd_f32, const void* res, void* y, int N,
                           int H, int W, int Cin, int Cout, int ksize, int iters, float* ms_per_launch, int* fused,
                           void* stream) {
    if (!x || !gamma_f32 || !beta_f32 || !w_oihw || !y || groups < 1) { set_error("sd_op_groupnorm_conv2d: bad arguments"); return SD_ERR_INVALID; }
    ConvOpts o;
    o.norm = ConvOpts::kNormInFront;
    o.gamma = gamma_f32; o.beta = beta_f32; o.norm_groups = groups; o.eps = eps; o.silu = silu; o.fused = fused;
    if (iters > 0) { o.iters = iters; o.ms = ms_per_launch; }
    return conv2d_impl(x, w_oihw, bias_f32, rowadd_f32, res, y, N, H, W, Cin, Cout, ksize, 1, 0, 0, stream, o);
}

static int ffn_geglu_impl(const void* x, const float* x_stat, int stat_parts, int stat_w, const void* ln_gamma,
                          const void* ln_beta, float ln_eps, const void* w1, const void* b1, const void* w2, const void* b2,
                          void* y, int M, int C, int iters, float* ms_per_launch, int* fused, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!x || !ln_gamma || !ln_beta || !w1 || !b1 || !w2 || !b2 || !y || M < 1 || C % 64 != 0) { set_error("sd_op_ffn_geglu: bad arguments"); return SD_ERR_INVALID; }
    const int hidden = 4 * C;
    if (int rc = pack_begin(s)) return rc;
    // packed as Encoder::pack_xformer packs a block whose LayerNorm folds into the projection
    WeightStore ws;
    NormW ln3;
    ConvW ff1, ff2;
    int rc;
    if ((rc = pack_norm_op(ws, ln_gamma, ln_beta, C, &ln3)) || (rc = pack_conv_op(ws, w1, 2 * hidden, C, 1, b1, true, false, &ff1)) ||
        (rc = ws.fold_ln(&ff1, ln3, 0, 1.0f)) || (rc = pack_conv_op(ws, w2, C, hidden, 1, b2, false, false, &ff2))) return rc;
    RowStat st;
    st.p = const_cast<float*>(x_stat); st.parts = stat_parts; st.width = stat_w;
    if (!x_stat) {                          // no producer: one part over the whole row
        st.p = static_cast<float*>(ws.dmalloc((size_t)rowstat_floats(M, C) * sizeof(float)));
        if (!st.p) { set_error("hipMalloc failed (row statistics)"); return SD_ERR_HIP; }
        st.parts = 1; st.width = C;
        if ((rc = launch_row_stats(static_cast<const half_t*>(x), C, st.p, M, C, 0))) return rc;
    }
    if ((rc = pack_end())) return rc;
    const View xv = view_of(x, C, C), yv = view_of(y, C, C);
    bool ran_fused = false;
    // ffn.hip's one launch where it takes the problem (unless two_gemms), otherwise the projection with its GEGLU epilogue
    // and the output linear with its residual epilogue: run_xformer_tail's choice and launches
    auto run = [&](bool two_gemms, int n, float* ms) {
        return run_op_on_arena(s, n, ms, [&](Ctx& c) {
            ran_fused = !two_gemms && op_ffn_fused(c, ff1, ff2, xv, st, ln_eps, M, yv);
            if (ran_fused) return;
            View g(c.arena->alloc_h((long)M * hidden), hidden, hidden);
            ConvArgs f_ln3;
            f_ln3.geglu = 1;
            f_ln3.ln_in = &st; f_ln3.ln_eps = ln_eps;
            op_conv(c, ff1, xv, 1, M, 1, g, f_ln3);
            op_conv(c, ff2, g, 1, M, 1, yv, conv_res(xv));
        });
    };
    const int n = ms_per_launch ? iters : 0;
    rc = run(false, n, ms_per_launch);
    if (fused) *fused = ran_fused ? 1 : 0;
    if (rc || n < 1) return rc;
    if (!ran_fused) { ms_per_launch[1] = ms_per_launch[0]; return SD_OK; }
    rc = run(true, n, ms_per_launch + 1);   // [1]: the two-GEMM form on the same operands
    return rc ? rc : run(false, 0, nullptr);                // leave the fused result in y
}

int sd_op_ffn_geglu(const void* x, const void* ln_gamma, const void* ln_beta, float ln_eps, const void* w1, const void* b1,
                    const void* w2, const void* b2, void* y, int M, int C, int iters, float* ms_per_launch, int* fused,
                    void* stream) {
    return ffn_geglu_impl(x, nullptr, 0, 0, ln_gamma, ln_beta, ln_eps, w1, b1, w2, b2, y, M, C, iters, ms_per_launch, fused,
                          stream);
}

// The same feed-forward on the row statistics a producer left (sd_op_linear_rowstats), as the UNet runs it.
int sd_op_ln_ffn_geglu(const void* x, const float* stat, int parts, int part_w, const void* ln_gamma, const void* ln_beta,
                       float ln_eps, const void* w1, const void* b1, const void* w2, const void* b2, void* y, int M, int C,
                       int* fused, void* stream) {
    if (!stat || parts < 1 || part_w < 1 || (long)parts * part_w < C || (long)(parts - 1) * part_w >= C) {
        set_error("sd_op_ln_ffn_geglu: bad statistics layout"); return SD_ERR_INVALID;
    }
    if (parts > igemm2_max_ln_parts()) {         // (ffn_fused_kernel holds as many; the two-GEMM form would fail at its launch)
        set_error("sd_op_ln_ffn_geglu: ln_parts " + std::to_string(parts) + " above the limit of " +
                  std::to_string(igemm2_max_ln_parts()) + " statistics parts per row");
        return SD_ERR_INVALID;
    }
    return ffn_geglu_impl(x, stat, parts, part_w, ln_gamma, ln_beta, ln_eps, w1, b1, w2, b2, y, M, C, 0, nullptr, fused, stream);
}

// The folded-LayerNorm chain of a transformer block at op level (unet.cpp run_xformer), in two calls that share the
// row-statistics buffer so a test can force the producer's and the consumer's kernel separately (sd_igemm_force).
// Producer: y1 = x W0^T + b0 (+ res), an op_conv asked for the row statistics of its output (ConvArgs::stat_out): from
// the GEMM epilogue when the launch can emit them (*producer = its kernel), row_stats_kernel over y1 otherwise (-1).
int sd_op_linear_rowstats(const void* x, const void* w0, const void* b0, const void* res, void* y1, float* stat, int M,
                          int K, int C, int* parts, int* part_w, int* producer, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!x || !w0 || !y1 || !stat || !parts || !part_w || !producer || M < 1 || K % 64 != 0 || K < 64 || C % 8 != 0 || C < 8) {
        set_error("sd_op_linear_rowstats: bad arguments"); return SD_ERR_INVALID;
    }
    if (int rc = pack_begin(s)) return rc;
    WeightStore ws;
    ConvW cw;
    int rc = pack_conv_op(ws, w0, C, K, 1, b0, false, false, &cw);
    if (rc || (rc = pack_end())) return rc;
    RowStat st;
    st.p = stat;
    ConvLaunch l;
    const View yv = view_of(y1, C, C), rv = view_of(res, C, C);
    rc = run_op_on_arena(s, 0, nullptr, [&](Ctx& c) {
        ConvArgs f = conv_res(rv);
        f.stat_out = &st;
        if (conv_prepare(c, cw, view_of(x, K, K), 1, M, 1, yv, f, &l))
            conv_launch(c, l, yv, &st);
    });
    *producer = l.plan.rowstats ? l.plan.kind : -1;
    *parts = st.parts;
    *part_w = st.width;
    return rc;
}

// Consumer: y2 = LayerNorm(y1) W1^T + b1 with the norm folded into W1 (WeightStore::fold_ln) and its statistics from the
// producer's buffer (ConvArgs::ln_in).  geglu = 0: W1 [O, C], the first rows_scaled outputs times row_scale
// (the q of q|k|v); geglu = 1: W1 [2 O, C] = [hidden | gate] rows, y2 = hidden * gelu(gate) [M, O].
int sd_op_ln_linear(const void* y1, const float* stat, int parts, int part_w, const void* gamma, const void* beta, float eps,
                    const void* w1, const void* b1, void* y2, int M, int C, int O, int geglu, int rows_scaled, float row_scale,
                    int* consumer, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!y1 || !stat || !gamma || !beta || !w1 || !y2 || !consumer || M < 1 || C % 64 != 0 || C < 64 || O % 64 != 0 ||
        O < 64 || parts < 1 || part_w < 1 || (long)parts * part_w < C || (long)(parts - 1) * part_w >= C) {
        set_error("sd_op_ln_linear: bad arguments"); return SD_ERR_INVALID;
    }
    if (parts > igemm2_max_ln_parts()) {         // refused ahead of the packing launches; launch_igemm2 holds the same check
        set_error("sd_op_ln_linear: ln_parts " + std::to_string(parts) + " above the limit of " +
                  std::to_string(igemm2_max_ln_parts()) + " statistics parts per row");
        return SD_ERR_INVALID;
    }
    if (int rc = pack_begin(s)) return rc;
    WeightStore ws;
    NormW ln;
    ConvW cw;
    int rc;
    if ((rc = pack_norm_op(ws, gamma, beta, C, &ln)) || (rc = pack_conv_op(ws, w1, geglu ? 2 * O : O, C, 1, b1, geglu != 0, false, &cw)) ||
        (rc = ws.fold_ln(&cw, ln, geglu ? 0 : rows_scaled, row_scale)) || (rc = pack_end())) return rc;
    RowStat st;
    st.p = const_cast<float*>(stat); st.parts = parts; st.width = part_w;
    ConvLaunch l;
    const View yv = view_of(y2, O, O);
    rc = run_op_on_arena(s, 0, nullptr, [&](Ctx& c) {
        ConvArgs f;
        f.geglu = geglu;
        f.ln_in = &st; f.ln_eps = eps;
        if (conv_prepare(c, cw, view_of(y1, C, C), 1, M, 1, yv, f, &l))
            conv_launch(c, l, yv, nullptr);
    });
    *consumer = l.plan.kind;
    return rc;
}

int sd_op_unet_conv_in(const void* x_nchw, const void* w_oihw, const void* bias_f32, void* y_nhwc, float* gn_summaries,
                       int groups, int N, int Cin, int H, int W, int Cout, int iters, float* ms_per_launch, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!x_nchw || !w_oihw || !bias_f32 || !y_nhwc || N < 1 || Cin < 1) { set_error("sd_op_unet_conv_in: bad arguments"); return SD_ERR_INVALID; }
    const long K = 64;
    HeadParams p;
    p.x_nchw = static_cast<const half_t*>(x_nchw); p.w = nullptr; p.K = K; p.bias = nullptr; p.y = static_cast<half_t*>(y_nhwc); p.ldy = Cout;
    p.gnstat_out = groups > 0 ? gn_summaries : nullptr; p.G = groups;
    p.N = N; p.Cin = Cin; p.H = H; p.W = W; p.Cout = Cout;
    // (refused before anything is allocated or launched)
    if (H < 1 || W < 1 || 9 * Cin > K || !conv_head_supported(p)) { set_error("sd_op_unet_conv_in: shape outside the one-launch kernel (Cout 320, 9 Cin <= 64, H W % 128 == 0)"); return SD_ERR_INVALID; }
    if (int rc = pack_begin(s)) return rc;
    WeightStore ws;
    ConvW cw;
    int rc = pack_conv_op(ws, w_oihw, Cout, Cin, 3, bias_f32, false, false, &cw);
    if (rc || (rc = pack_end())) return rc;
    p.w = cw.w; p.K = cw.K; p.bias = cw.bias;
    return launch_or_time(s, iters, ms_per_launch, [&]() { return launch_conv_head(p, s); });
}

int sd_op_unet_conv_in2(const void* a, int Na, int Ca, float in_scale, const void* b, int Nb, int Cb, int zero_from,
                        const void* w_oihw, const void* bias_f32, void* y_nhwc, int64_t ldy, float* gn_summaries, int groups, int N,
                        int H, int W, int Cout, int iters, float* ms_per_launch, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!a || !b || !w_oihw || !bias_f32 || !y_nhwc || N < 1 || Na < 1 || Nb < 1 || Ca < 1 || Cb < 1 || H < 1 || W < 1 ||
        !(in_scale == in_scale)) {
        set_error("sd_op_unet_conv_in2: bad arguments");
        return SD_ERR_INVALID;
    }
    Head2Params p;
    p.a = static_cast<const half_t*>(a); p.Na = Na; p.Ca = Ca; p.in_scale = in_scale;
    p.b = static_cast<const half_t*>(b); p.Nb = Nb; p.Cb = Cb; p.zero_from = zero_from;
    p.K = 128; p.y = static_cast<half_t*>(y_nhwc); p.ldy = ldy;
    p.gnstat_out = groups > 0 ? gn_summaries : nullptr; p.G = groups;
    p.N = N; p.H = H; p.W = W; p.Cout = Cout;
    if (!conv_head2_supported(p)) {
        set_error("sd_op_unet_conv_in2: shape outside the one-launch kernel (Cout 320, 9 (Ca + Cb) <= 128, N % Na == 0, H W % 128 == 0, ldy % 8 == 0)");
        return SD_ERR_INVALID;
    }
    if (int rc = pack_begin(s)) return rc;
    WeightStore ws;
    ConvW cw;
    int rc = pack_conv_op(ws, w_oihw, Cout, Ca + Cb, 3, bias_f32, false, false, &cw);
    if (rc || (rc = pack_end())) return rc;
    p.w = cw.w; p.K = cw.K; p.bias = cw.bias;       // (64 for up to 7 input channels, as a model's conv_in packs)
    return launch_or_time(s, iters, ms_per_launch, [&]() { return launch_conv_head2(p, s); });
}

int sd_op_unet_conv_out_ex(const void* x_nhwc, int64_t ldx, const void* gamma_f32, const void* beta_f32, int groups, float eps,
                           int silu, const void* w_oihw, const void* bias_f32, void* y_nchw, int N, int H, int W, int C, int Cout,
                           const float* summaries, int S, int64_t rows, int iters, float* ms_per_launch, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!x_nhwc || !gamma_f32 || !beta_f32 || !w_oihw || !bias_f32 || !y_nchw || N < 1 || H < 1 || W < 1 || groups < 1 || C < 64 ||
        C % 64 != 0 || Cout < 1) {
        set_error("sd_op_unet_conv_out: bad arguments"); return SD_ERR_INVALID;
    }
    const long HW = (long)H * W;
    if (ldx < C || ldx % 8 != 0) { set_error("sd_op_unet_conv_out: ldx must be at least C and a multiple of 8"); return SD_ERR_INVALID; }
    if (summaries && (S < 1 || rows < 1 || (int64_t)S * rows < HW || (int64_t)(S - 1) * rows >= HW)) {
        set_error("sd_op_unet_conv_out: S summaries of `rows` pixels must cover H W with no empty one"); return SD_ERR_INVALID;
    }
    TailParams p;
    p.x = static_cast<const half_t*>(x_nhwc); p.ldx = ldx;
    p.gn_part = summaries ? summaries : static_cast<const float*>(gamma_f32);      // (own pass: replaced below; non-null for the check)
    p.gn_S = summaries ? S : 1; p.gn_rows = summaries ? rows : HW;
    p.G = groups; p.eps = eps; p.gamma = static_cast<const float*>(gamma_f32); p.beta = static_cast<const float*>(beta_f32); p.silu = silu;
    p.w = nullptr; p.K = 9L * C; p.bias = nullptr; p.y = static_cast<half_t*>(y_nchw);
    p.N = N; p.H = H; p.W = W; p.C = C; p.Cout = Cout;
    if (!conv_tail_supported(p)) { set_error("sd_op_unet_conv_out: shape outside the one-launch kernel (C 320, Cout <= 4, H % 8 == 0, W % 16 == 0, groups <= 32)"); return SD_ERR_INVALID; }
    if (int rc = pack_begin(s)) return rc;
    WeightStore ws;
    ConvW cw;
    int rc = pack_conv_op(ws, w_oihw, Cout, C, 3, bias_f32, false, false, &cw);
    if (!rc && !summaries) {                // the statistics pass, outside the timed launches
        float* scratch = static_cast<float*>(ws.dmalloc((size_t)gn_scratch_floats(N, HW, C, groups) * sizeof(float)));
        if (!scratch) { set_error("hipMalloc failed (GroupNorm scratch)"); return SD_ERR_HIP; }
        GnStats st;
        rc = launch_gn_stats(static_cast<const half_t*>(x_nhwc), ldx, N, HW, C, groups, scratch, &st, 0);
        p.gn_part = st.part; p.gn_S = st.S; p.gn_rows = st.rows;
    }
    if (rc || (rc = pack_end())) return rc;
    p.w = cw.w; p.K = cw.K; p.bias = cw.bias;
    return launch_or_time(s, iters, ms_per_launch, [&]() { return launch_conv_tail(p, s); });
}

int sd_op_unet_conv_out(const void* x_nhwc, const void* gamma_f32, const void* beta_f32, int groups, float eps, int silu,
                        const void* w_oihw, const void* bias_f32, void* y_nchw, int N, int H, int W, int C, int Cout, int iters,
                        float* ms_per_launch, void* stream) {
    return sd_op_unet_conv_out_ex(x_nhwc, C, gamma_f32, beta_f32, groups, eps, silu, w_oihw, bias_f32, y_nchw, N, H, W, C, Cout,
                                  nullptr, 0, 0, iters, ms_per_launch, stream);
}

int sd_bench_conv2d(const void* x, const void* w_oihw, void* y, int N, int H, int W, int Cin, int Cout, int ksize,
                    int stride, int upsample2x, int geglu, int iters, float* ms_per_launch, void* stream) {
    if (iters < 1 || !ms_per_launch) { set_error("sd_bench_conv2d: bad arguments"); return SD_ERR_INVALID; }
    ConvOpts o;
    o.iters = iters; o.ms = ms_per_launch;
    return conv2d_impl(x, w_oihw, nullptr, nullptr, nullptr, y, N, H, W, Cin, Cout, ksize, stride, upsample2x, geglu, stream, o);
}

// Scratch buffers of the entries below: freed on every return path (hipFree waits for the device), including the
// SD_HIP_CHECK early returns.
struct DevScope {
    std::vector<void*> bufs;
    ~DevScope() { for (void* p : bufs) (void)hipFree(p); }
};
#define SD_DEV_ALLOC(scope, ptr, bytes)                                              \
    do {                                                                             \
        SD_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&(ptr)), (bytes)));          \
        (scope).bufs.push_back(ptr);                                                 \
    } while (0)

int sd_op_groupnorm(const void* x, const void* gamma_f32, const void* beta_f32, void* y, int N, int HW, int C,
                    int groups, float eps, int silu, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    DevScope scope;
    float* scratch = nullptr;
    SD_DEV_ALLOC(scope, scratch, (size_t)gn_scratch_floats(N, HW, C, groups) * 4);
    int rc = launch_groupnorm(static_cast<const half_t*>(x), C, static_cast<const float*>(gamma_f32),
                              static_cast<const float*>(beta_f32), static_cast<half_t*>(y), C, N, HW, C, groups,
                              eps, silu, scratch, s);
    hipError_t e = hipStreamSynchronize(s);
    if (!rc && e != hipSuccess) { set_error(hipGetErrorString(e)); rc = SD_ERR_HIP; }
    return rc;
}

static void norm_plan_out(const NormPlan& pl, int64_t* out) {
    const int64_t o[10] = {pl.stats, pl.apply, pl.apply == 0 ? pl.T : 0, pl.NV, pl.finalize, pl.S, pl.rows, pl.CB, pl.scratch,
                           pl.use_pre};
    for (int i = 0; i < 10; ++i) out[i] = o[i];
}

int sd_norm_plan(int N, int64_t HW, int C, int G, int have_summaries, int S_pre, int64_t* out) {
    if (!out) { set_error("sd_norm_plan: null argument"); return SD_ERR_INVALID; }
    if (have_summaries && S_pre < 1) { set_error("sd_norm_plan: summaries need S_pre >= 1"); return SD_ERR_INVALID; }
    const NormPlan pl = norm_plan(N, HW, C, G, have_summaries != 0, S_pre, 0);
    if (!pl.valid) { set_error("sd_norm_plan: N, HW >= 1, C a multiple of 8 and of groups, groups <= 256"); return SD_ERR_INVALID; }
    if (pl.apply == 1 && pl.apply_rows < 1) { set_error("sd_norm_plan: C too large for the apply kernel"); return SD_ERR_UNSUPPORTED; }
    norm_plan_out(pl, out);
    return SD_OK;
}

int sd_norm_plan_batch(int count, const int64_t* problems, int64_t* out) {
    if (count < 0 || !problems || !out) { set_error("sd_norm_plan_batch: bad arguments"); return SD_ERR_INVALID; }
    for (int i = 0; i < count; ++i) {
        const int64_t* q = problems + (size_t)i * 4;
        const int rc = sd_norm_plan((int)q[0], q[1], (int)q[2], (int)q[3], 0, 0, out + (size_t)i * 10);
        if (rc) return rc;
    }
    return SD_OK;
}

int sd_op_groupnorm_ex(const void* x, int64_t ldx, const void* gamma_f32, const void* beta_f32, void* y, int64_t ldy, int N,
                       int64_t HW, int C, int groups, float eps, int silu, const float* summaries, int S, int64_t rows,
                       int64_t* ran, void* stream) {
    if (!x || !gamma_f32 || !beta_f32 || !y || !ran || N < 1 || HW < 1 || C < 8 || groups < 1) {
        set_error("sd_op_groupnorm_ex: bad arguments"); return SD_ERR_INVALID;
    }
    if (ldx < C || ldy < C || ldx % 8 != 0 || ldy % 8 != 0) {
        set_error("sd_op_groupnorm_ex: ldx / ldy must be at least C and a multiple of 8"); return SD_ERR_INVALID;
    }
    if (summaries && (S < 1 || rows < 1 || (int64_t)S * rows < HW || (int64_t)(S - 1) * rows >= HW)) {
        set_error("sd_op_groupnorm_ex: S summaries of `rows` pixels must cover HW with no empty one"); return SD_ERR_INVALID;
    }
    const NormPlan pl = norm_plan(N, HW, C, groups, summaries != nullptr, S, rows);
    if (!pl.valid) { set_error("sd_op_groupnorm_ex: C must be a multiple of 8 and of groups, groups <= 256"); return SD_ERR_INVALID; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    DevScope scope;
    float* scratch = nullptr;
    SD_DEV_ALLOC(scope, scratch, (size_t)pl.scratch * 4);
    GnStats pre;
    pre.part = summaries; pre.S = S; pre.rows = rows;
    NormPlan did;
    int rc = launch_groupnorm(static_cast<const half_t*>(x), ldx, static_cast<const float*>(gamma_f32),
                              static_cast<const float*>(beta_f32), static_cast<half_t*>(y), ldy, N, HW, C, groups, eps, silu,
                              scratch, s, summaries ? &pre : nullptr, &did);
    hipError_t e = hipStreamSynchronize(s);
    if (!rc && e != hipSuccess) { set_error(hipGetErrorString(e)); rc = SD_ERR_HIP; }
    if (!rc) norm_plan_out(did, ran);
    return rc;
}

int sd_op_gn_stats(const void* x, int64_t ldx, int N, int64_t HW, int C, int groups, float* out_host, int* S, int64_t* rows,
                   int* kernel, void* stream) {
    if (!x || !out_host || !S || !rows || !kernel || N < 1 || HW < 1 || C < 8 || groups < 1 || ldx < C || ldx % 8 != 0) {
        set_error("sd_op_gn_stats: bad arguments"); return SD_ERR_INVALID;
    }
    const NormPlan pl = norm_plan(N, HW, C, groups, false, 0, 0);
    if (!pl.valid) { set_error("sd_op_gn_stats: C must be a multiple of 8 and of groups, groups <= 256"); return SD_ERR_INVALID; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    DevScope scope;
    float* scratch = nullptr;
    SD_DEV_ALLOC(scope, scratch, (size_t)pl.scratch * 4);
    GnStats st;
    int rc = launch_gn_stats(static_cast<const half_t*>(x), ldx, N, HW, C, groups, scratch, &st, s);
    hipError_t e = hipStreamSynchronize(s);
    if (!rc && e == hipSuccess) e = hipMemcpy(out_host, scratch, (size_t)N * st.S * groups * 2 * 4, hipMemcpyDeviceToHost);
    if (!rc && e != hipSuccess) { set_error(hipGetErrorString(e)); rc = SD_ERR_HIP; }
    if (!rc) { *S = st.S; *rows = st.rows; *kernel = pl.stats2 ? 2 : 1; }
    return rc;
}

int sd_op_groupnorm_concat(const void* x, int Ca, int Cb, const void* gamma_f32, const void* beta_f32, void* y, int N, int HW,
                           int groups, float eps, int silu, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int C = Ca + Cb;
    if (!x || !gamma_f32 || !beta_f32 || !y || Ca < 8 || Cb < 8 || groups < 1 || C % groups != 0 || Cb % groups != 0) {
        set_error("sd_op_groupnorm_concat: bad arguments"); return SD_ERR_INVALID;
    }
    const int u = gn_cat_unit(Ca, Cb, groups), ub = Cb / groups;
    if (!(u >= 8 || u == 4) || (C / groups) % ub != 0 || Ca % ub != 0 || !(ub >= 8 || ub == 4)) {
        set_error("sd_op_groupnorm_concat: the halves' sub-groups do not tile the groups"); return SD_ERR_INVALID;
    }
    const int Ga = Ca / u;
    DevScope scope;
    float *sa = nullptr, *sb = nullptr, *fin = nullptr, *scratch = nullptr;
    SD_DEV_ALLOC(scope, sa, (size_t)gn_scratch_floats(N, HW, Ca, Ga) * 4);
    SD_DEV_ALLOC(scope, sb, (size_t)gn_scratch_floats(N, HW, Cb, groups) * 4);
    SD_DEV_ALLOC(scope, fin, (size_t)N * groups * 2 * 4);
    SD_DEV_ALLOC(scope, scratch, (size_t)gn_scratch_floats(N, HW, C, groups) * 4);
    const half_t* xh = static_cast<const half_t*>(x);
    GnStats sta, stb, stc;
    int rc = launch_gn_stats(xh, C, N, HW, Ca, Ga, sa, &sta, s);                // the hidden half: Ga sub-groups of width u
    if (!rc) rc = launch_gn_stats(xh + Ca, C, N, HW, Cb, groups, sb, &stb, s);   // the skip half: its own `groups` groups
    if (!rc) rc = launch_gn_cat_finalize(sta, Ga, Ca, stb, groups, Cb, fin, N, HW, groups, s);
    stc.part = fin; stc.S = 1; stc.rows = HW;
    if (!rc) rc = launch_groupnorm(xh, C, static_cast<const float*>(gamma_f32), static_cast<const float*>(beta_f32),
                                   static_cast<half_t*>(y), C, N, HW, C, groups, eps, silu, scratch, s, &stc);
    hipError_t e = hipStreamSynchronize(s);
    if (!rc && e != hipSuccess) { set_error(hipGetErrorString(e)); rc = SD_ERR_HIP; }
    return rc;
}

int sd_bench_groupnorm(const void* x, const void* gamma_f32, const void* beta_f32, void* y, int N, int HW, int C,
                       int groups, float eps, int silu, int iters, float* ms_per_launch, void* stream) {
    if (iters < 1 || !ms_per_launch) { set_error("sd_bench_groupnorm: bad arguments"); return SD_ERR_INVALID; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    DevScope scope;
    float* scratch = nullptr;
    SD_DEV_ALLOC(scope, scratch, (size_t)gn_scratch_floats(N, HW, C, groups) * 4);
    int rc = 0;
    // SD_GN_BENCH_APPLY=1: the statistics pass runs once, outside the timed launches, and every timed launch is the
    // apply pass alone on those summaries -- what a GroupNorm costs when the producing convolution left them
    static const bool apply_only = getenv("SD_GN_BENCH_APPLY") != nullptr;
    GnStats st;
    float* scratch2 = nullptr;
    if (apply_only && gn_wants_stats(HW, C, groups)) {
        SD_DEV_ALLOC(scope, scratch2, (size_t)gn_scratch_floats(N, HW, C, groups) * 4);
        rc = launch_gn_stats(static_cast<const half_t*>(x), C, N, HW, C, groups, scratch2, &st, s);
    }
    if (rc) return rc;
    return time_launches(s, iters, ms_per_launch, [&]() {
        return launch_groupnorm(static_cast<const half_t*>(x), C, static_cast<const float*>(gamma_f32),
                                static_cast<const float*>(beta_f32), static_cast<half_t*>(y), C, N, HW, C, groups,
                                eps, silu, scratch, s, st.part ? &st : nullptr);
    });
}

int sd_op_timestep_sinusoid(const float* t, float* out, int count, int dim, int flip_sin_to_cos, float freq_shift,
                            void* stream) {
    if (!t || !out || count < 1 || dim < 2 || (dim & 1)) { set_error("sd_op_timestep_sinusoid: bad arguments"); return SD_ERR_INVALID; }
    return launch_timestep_sinusoid(t, 1, out, count, dim, flip_sin_to_cos, freq_shift, dim, static_cast<hipStream_t>(stream));
}

int sd_op_text_time_input(const void* add_text, const float* ids, float* out, int B, int P, int ad, int n_ids,
                          int flip_sin_to_cos, float freq_shift, void* stream) {
    if (!add_text || !ids || !out || B < 1 || P <= 0 || ad < 2 || (ad & 1) || n_ids < 1 || n_ids > 8) {
        set_error("sd_op_text_time_input: bad arguments (P > 0, even ad, n_ids in [1, 8])");
        return SD_ERR_INVALID;
    }
    return launch_text_time_input(static_cast<const half_t*>(add_text), ids, out, B, P, ad, n_ids, flip_sin_to_cos,
                                  freq_shift, P + n_ids * ad, static_cast<hipStream_t>(stream));
}

int sd_op_timestep_cond_embedding(const float* t, const float* cond, const void* w_f16, float* out, int B, int dim,
                                  int cond_dim, int flip_sin_to_cos, float freq_shift, void* stream) {
    if (!t || !cond || !w_f16 || !out || B < 1 || dim < 2 || (dim & 1) || cond_dim < 1 || cond_dim > 1024) {
        set_error("sd_op_timestep_cond_embedding: bad arguments (even dim, cond_dim in [1, 1024])");
        return SD_ERR_INVALID;
    }
    return launch_timestep_cond(t, cond, static_cast<const half_t*>(w_f16), cond_dim, out, B, dim, cond_dim, flip_sin_to_cos,
                                freq_shift, static_cast<hipStream_t>(stream));
}

int sd_small_linear_plan(int B, int K, int n_out) {
    if (B < 1 || K < 1 || n_out < 1) { set_error("sd_small_linear_plan: bad arguments"); return -1; }
    return small_linear_plan(B, K, n_out);
}

int sd_op_small_linear(const float* x, const void* w_f16, const float* bias, float* y, int B, int K, int n_out, int silu_in,
                       int silu_out, void* stream) {
    if (!x || !w_f16 || !y || B < 1 || K < 1 || n_out < 1) { set_error("sd_op_small_linear: bad arguments"); return SD_ERR_INVALID; }
    return launch_small_linear(x, K, static_cast<const half_t*>(w_f16), bias, y, n_out, B, K, n_out, silu_in, silu_out,
                               static_cast<hipStream_t>(stream));
}

int sd_op_layernorm(const void* x, const void* gamma_f32, const void* beta_f32, void* y, int rows, int C, float eps,
                    void* stream) {
    return launch_layernorm(static_cast<const half_t*>(x), C, static_cast<const float*>(gamma_f32),
                            static_cast<const float*>(beta_f32), static_cast<half_t*>(y), C, rows, C, eps,
                            static_cast<hipStream_t>(stream));
}

int sd_op_layernorm_ex(const void* x, int64_t ldx, const void* gamma_f32, const void* beta_f32, void* y, int64_t ldy,
                       int64_t rows, int C, float eps, void* stream) {
    if (!x || !gamma_f32 || !beta_f32 || !y || rows < 1 || C < 8 || ldx < C || ldy < C || ldx % 8 != 0 || ldy % 8 != 0) {
        set_error("sd_op_layernorm_ex: bad arguments (ldx / ldy at least C and a multiple of 8)"); return SD_ERR_INVALID;
    }
    return launch_layernorm(static_cast<const half_t*>(x), ldx, static_cast<const float*>(gamma_f32),
                            static_cast<const float*>(beta_f32), static_cast<half_t*>(y), ldy, rows, C, eps,
                            static_cast<hipStream_t>(stream));
}

int sd_op_row_stats(const void* x, int64_t ldx, float* stat, int64_t rows, int C, void* stream) {
    if (!x || !stat || rows < 1 || C < 8 || ldx < C || ldx % 8 != 0) {
        set_error("sd_op_row_stats: bad arguments (ldx at least C and a multiple of 8)"); return SD_ERR_INVALID;
    }
    return launch_row_stats(static_cast<const half_t*>(x), ldx, stat, rows, C, static_cast<hipStream_t>(stream));
}

int sd_op_freeu(void* cat_nhwc, int N, int H, int W, int C1, int C2, float b, float s, void* stream) {
    if (!cat_nhwc) { set_error("sd_op_freeu: null argument"); return SD_ERR_INVALID; }
    return launch_freeu(static_cast<half_t*>(cat_nhwc), (long)C1 + C2, N, H, W, C1, C2, b, s, static_cast<hipStream_t>(stream));
}

int sd_tome_plan(int H, int W, int sx, int sy, double ratio, int use_rand, uint32_t seed, uint32_t step, uint32_t site,
                 int32_t* info4, int32_t* dst_tok) {
    if (!info4) { set_error("sd_tome_plan: null argument"); return SD_ERR_INVALID; }
    TomeGeom g;
    if (tome_geom(H, W, sx, sy, ratio, use_rand, seed, step, site, &g)) return SD_ERR_INVALID;
    info4[0] = g.Nd; info4[1] = g.Ns; info4[2] = g.r; info4[3] = g.Tm;
    if (dst_tok) tome_dst_tokens(g, dst_tok);
    return SD_OK;
}
int64_t sd_tome_plan_bytes(int B, int T) { return tome_plan_bytes(B, T); }
int sd_op_tome_match(const void* x, int64_t ldx, int B, int H, int W, int C, int sx, int sy, double ratio, int use_rand,
                     uint32_t seed, uint32_t step, uint32_t site, void* plan, int32_t* map_out, float* node_max,
                     int32_t* node_idx, void* stream) {
    if (!x || !plan) { set_error("sd_op_tome_match: null argument"); return SD_ERR_INVALID; }
    TomeGeom g;
    if (tome_geom(H, W, sx, sy, ratio, use_rand, seed, step, site, &g)) return SD_ERR_INVALID;
    if (!tome_supported(g)) {
        set_error("sd_op_tome_match: more than 16384 tokens, or a map without a whole cell, is not supported");
        return SD_ERR_UNSUPPORTED;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = launch_tome_match(static_cast<const half_t*>(x), ldx, B, C, g, plan, s)) return rc;
    return tome_plan_fetch(plan, B, g.T, g.Ns, map_out, node_max, node_idx, s);
}
int sd_op_tome_plan_from_map(const int32_t* map_host, int B, int T, int T_merged, void* plan, void* stream) {
    return tome_plan_from_map(map_host, B, T, T_merged, plan, static_cast<hipStream_t>(stream));
}
int sd_op_tome_merge(const void* src, int64_t lds, int cols, const void* plan, int B, int T, void* dst, int64_t ldd,
                     void* stream) {
    return launch_tome_merge(static_cast<const half_t*>(src), lds, cols, plan, B, T, 0, static_cast<half_t*>(dst), ldd,
                             static_cast<hipStream_t>(stream));
}
int sd_op_tome_unmerge(const void* src, int64_t lds, int cols, const void* plan, int B, int T, void* dst, int64_t ldd,
                       void* stream) {
    return launch_tome_unmerge(static_cast<const half_t*>(src), lds, cols, plan, B, T, static_cast<half_t*>(dst), ldd,
                               static_cast<hipStream_t>(stream));
}

int sd_hypertile_plan(int Hs, int Ws, int tile_size, int swap_size, uint32_t seed, uint32_t step, uint32_t site, int32_t* out4) {
    if (!out4) { set_error("sd_hypertile_plan: null argument"); return SD_ERR_INVALID; }
    HyperTileGeom g;
    if (hypertile_plan(Hs, Ws, tile_size, swap_size, seed, step, site, &g)) return SD_ERR_INVALID;
    out4[0] = g.nh; out4[1] = g.nw; out4[2] = g.th; out4[3] = g.tw;
    return SD_OK;
}
int sd_op_hypertile_gather(const void* src, int64_t lds, int cols, int B, int Hs, int Ws, int nh, int nw, void* dst, int64_t ldd,
                           void* stream) {
    return launch_hypertile_gather(static_cast<const half_t*>(src), lds, cols, B, Hs, Ws, nh, nw, static_cast<half_t*>(dst), ldd,
                                   static_cast<hipStream_t>(stream));
}
int sd_op_hypertile_scatter(const void* src, int64_t lds, int cols, int B, int Hs, int Ws, int nh, int nw, void* dst, int64_t ldd,
                            void* stream) {
    return launch_hypertile_scatter(static_cast<const half_t*>(src), lds, cols, B, Hs, Ws, nh, nw, static_cast<half_t*>(dst), ldd,
                                    static_cast<hipStream_t>(stream));
}

int sd_temporal_attention_plan(int V, int F, int HW, int heads, int d, int64_t* out7) {
    if (!out7) { set_error("sd_temporal_attention_plan: null argument"); return SD_ERR_INVALID; }
    const TattnPlan pl = temporal_attention_plan(V, F, HW, heads, d);
    if (pl.D == 0) {
        set_error("temporal_attention: needs V, HW, heads >= 1, 1 <= F <= 32 and a head dim of 32, 40, 64, 80 or 160");
        return SD_ERR_UNSUPPORTED;
    }
    const int64_t o[7] = {pl.D, pl.FT, pl.pixels, pl.waves, pl.pv_k, pl.lds_bytes, pl.blocks};
    for (int i = 0; i < 7; ++i) out7[i] = o[i];
    return SD_OK;
}
int sd_op_temporal_attention(const void* q, const void* k, const void* v, void* out, const float* bias, int64_t ldq, int64_t ldk,
                             int64_t ldv, int64_t ldo, int64_t ldb, int V, int F, int HW, int heads, int d, int prescaled,
                             void* stream) {
    return launch_temporal_attention(static_cast<const half_t*>(q), static_cast<const half_t*>(k), static_cast<const half_t*>(v),
                                     static_cast<half_t*>(out), bias, ldq, ldk, ldv, ldo, ldb, V, F, HW, heads, d, prescaled,
                                     static_cast<hipStream_t>(stream));
}
int sd_op_motion_pos_bias(const void* w, int N, int C, int F, float scale, int scale_rows, float* out, int64_t ldo, void* stream) {
    return launch_motion_pos_bias(static_cast<const half_t*>(w), N, C, F, scale, scale_rows, out, ldo,
                                  static_cast<hipStream_t>(stream));
}

int sd_op_attention(const void* q, const void* k, const void* v, void* out, int B, int Tq, int Tk, int heads, int d,
                    int ldq, int ldk, int ldv, int ldo, void* stream) {
    return launch_attention(static_cast<const half_t*>(q), static_cast<const half_t*>(k),
                            static_cast<const half_t*>(v), static_cast<half_t*>(out), B, Tq, Tk, heads, d, ldq, ldk,
                            ldv, ldo, static_cast<hipStream_t>(stream));
}

int sd_op_attention_ex(const void* q, const void* k, const void* v, void* out, int B, int Tq, int Tk, int heads, int d,
                       int ldq, int ldk, int ldv, int ldo, int causal, int prescaled, void* stream) {
    return launch_attention(static_cast<const half_t*>(q), static_cast<const half_t*>(k),
                            static_cast<const half_t*>(v), static_cast<half_t*>(out), B, Tq, Tk, heads, d, ldq, ldk,
                            ldv, ldo, static_cast<hipStream_t>(stream), causal, prescaled);
}

int sd_attention_plan(int B, int Tq, int Tk, int heads, int d, int causal, int prescaled, int* out5) {
    if (!out5) { set_error("sd_attention_plan: null argument"); return SD_ERR_INVALID; }
    const AttnPlan pl = attention_plan(B, Tq, Tk, heads, d, causal, prescaled);
    if (pl.D == 0) { set_error("attention: unsupported head dim " + std::to_string(d)); return SD_ERR_UNSUPPORTED; }
    const int o[5] = {pl.D, pl.QT, pl.KT, pl.PRESC, pl.NWV};
    for (int i = 0; i < 5; ++i) out5[i] = o[i];
    return SD_OK;
}

int sd_op_ip_cross_attention(const void* q, const void* k, const void* v, const void* k_ip, const void* v_ip, void* out,
                             int B, int Tq, int L, int T_ip, int heads, int d, int ldq, int ldk, int ldv, int ldk_ip,
                             int ldv_ip, int ldo, float ip_scale, int prescaled, int iters, float* ms_per_launch,
                             void* stream) {
    const half_t *qh = static_cast<const half_t*>(q), *kh = static_cast<const half_t*>(k), *vh = static_cast<const half_t*>(v);
    const half_t *kih = static_cast<const half_t*>(k_ip), *vih = static_cast<const half_t*>(v_ip);
    half_t* oh = static_cast<half_t*>(out);
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto fused = [&]() {
        return launch_ip_attention(qh, kh, vh, kih, vih, oh, B, Tq, L, T_ip, heads, d, ldq, ldk, ldv, ldk_ip, ldv_ip, ldo,
                                   ip_scale, prescaled, s);
    };
    int rc = fused();
    if (rc || iters <= 0) return rc;
    if (!ms_per_launch) { set_error("sd_op_ip_cross_attention: ms_per_launch required with iters > 0"); return SD_ERR_INVALID; }
    if (!attention_supported(d)) { set_error("sd_op_ip_cross_attention: timing needs a head dim of the text kernel"); return SD_ERR_UNSUPPORTED; }
    // [0] the fused kernel, [1] the text-only cross-attention launch on the same operands, [2] the unfused
    // composition: text attention, image attention into a scratch tensor, out += ip_scale * scratch
    half_t* tmp = nullptr;
    SD_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&tmp), (size_t)B * Tq * heads * d * sizeof(half_t)));
    const long ldt = (long)heads * d;
    auto text = [&]() {
        return launch_attention(qh, kh, vh, oh, B, Tq, L, heads, d, ldq, ldk, ldv, ldo, s, 0, prescaled);
    };
    auto unfused = [&]() {
        int r = text();
        if (!r) r = launch_attention(qh, kih, vih, tmp, B, Tq, T_ip, heads, d, ldq, ldk_ip, ldv_ip, ldt, s, 0, prescaled);
        if (!r) r = launch_axpy_f16(oh, ldo, tmp, ldt, (long)B * Tq, heads * d, ip_scale, s);
        return r;
    };
    for (int variant = 0; variant < 3 && !rc; ++variant)
        rc = time_launches(s, iters, ms_per_launch + variant, [&]() { return variant == 0 ? fused() : variant == 1 ? text() : unfused(); });
    if (!rc) rc = fused();                  // leave the fused result in out
    if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = SD_ERR_HIP;
    (void)hipFree(tmp);
    return rc;
}

int sd_ip_attention_plan(int B, int Tq, int L, int T_ip, int heads, int d, float ip_scale, int* out4) {
    if (!out4) { set_error("sd_ip_attention_plan: null argument"); return SD_ERR_INVALID; }
    IpPlan pl;
    if (int rc = ip_attention_plan(B, Tq, L, T_ip, heads, d, ip_scale, &pl)) return rc;
    out4[0] = pl.tile_rows; out4[1] = pl.qtiles; out4[2] = pl.qblocks; out4[3] = pl.lds_bytes;
    return SD_OK;
}

int sd_op_region_cross_attention(const void* q, const void* k, const void* v, const float* w, void* out, int B, int Tq, int L,
                                 int R, int heads, int d, int ldq, int ldk, int ldv, int ldo, int Bw, int prescaled,
                                 void* stream) {
    return launch_region_attention(static_cast<const half_t*>(q), static_cast<const half_t*>(k), static_cast<const half_t*>(v),
                                   w, static_cast<half_t*>(out), B, Tq, L, R, heads, d, ldq, ldk, ldv, ldo, Bw, prescaled,
                                   static_cast<hipStream_t>(stream));
}

int sd_op_region_pyramid(const float* weights, float* out, int Bw, int R, int H, int W, int levels, void* stream) {
    return launch_region_pyramid(weights, out, Bw, R, H, W, levels, static_cast<hipStream_t>(stream));
}

int sd_region_plan(int R, int L, int d, int* out4) {
    if (!out4) { set_error("sd_region_plan: null argument"); return SD_ERR_INVALID; }
    RegionPlan pl;
    if (int rc = region_plan(R, L, d, &pl)) return rc;
    out4[0] = pl.seg_per_group; out4[1] = pl.groups; out4[2] = pl.lds_bytes;
    out4[3] = pl.groups > 1 ? 1 : 0;
    return SD_OK;
}

int sd_op_resampler_attention(const void* q, const void* k_x, const void* v_x, const void* k_l, const void* v_l, void* out,
                              int B, int n_q, int T_feat, int heads, int ldq, int ldk_x, int ldv_x, int ldk_l, int ldv_l,
                              int ldo, int prescaled, int iters, float* ms_per_launch, void* stream) {
    if (!q || !k_x || !v_x || !k_l || !v_l || !out) { set_error("sd_op_resampler_attention: null argument"); return SD_ERR_INVALID; }
    const half_t *qh = static_cast<const half_t*>(q), *kxh = static_cast<const half_t*>(k_x), *vxh = static_cast<const half_t*>(v_x);
    const half_t *klh = static_cast<const half_t*>(k_l), *vlh = static_cast<const half_t*>(v_l);
    half_t* oh = static_cast<half_t*>(out);
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto fused = [&]() {
        return launch_resampler_attention(qh, kxh, vxh, klh, vlh, oh, B, n_q, T_feat, heads, ldq, ldk_x, ldv_x, ldk_l, ldv_l,
                                          ldo, prescaled, s);
    };
    int rc = fused();
    if (rc || iters <= 0) return rc;
    if (!ms_per_launch) { set_error("sd_op_resampler_attention: ms_per_launch required with iters > 0"); return SD_ERR_INVALID; }
    // [0] this kernel, [1] the composed form: K and V concatenated into one [B, Tk, 2 A] buffer, then attn_kernel<64>
    const int A = heads * 64, Tk = T_feat + n_q;
    half_t* cat = nullptr;
    SD_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&cat), (size_t)B * Tk * 2 * A * sizeof(half_t)));
    auto composed = [&]() {
        int r = launch_concat_rows_f16(kxh, ldk_x, T_feat, klh, ldk_l, n_q, cat, 2L * A, B, A, s);
        if (!r) r = launch_concat_rows_f16(vxh, ldv_x, T_feat, vlh, ldv_l, n_q, cat + A, 2L * A, B, A, s);
        if (!r) r = launch_attention(qh, cat, cat + A, oh, B, n_q, Tk, heads, 64, ldq, 2L * A, 2L * A, ldo, s, 0, prescaled);
        return r;
    };
    for (int variant = 0; variant < 2 && !rc; ++variant)
        rc = time_launches(s, iters, ms_per_launch + variant, [&]() { return variant == 0 ? fused() : composed(); });
    if (!rc) rc = fused();                  // leave this kernel's result in out
    if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = SD_ERR_HIP;
    (void)hipFree(cat);
    return rc;
}

int sd_op_controlnet_residuals(const sd_cn_problem* problems, int count, float scale, int mode, int iters,
                               float* ms_per_launch, void* stream) {
    if (!problems || count < 1 || count > kCnMaxProblems) { set_error("sd_op_controlnet_residuals: 1..16 problems"); return SD_ERR_INVALID; }
    if (mode != 0 && mode != 1) { set_error("sd_op_controlnet_residuals: mode must be 0 (grouped) or 1 (unfused)"); return SD_ERR_INVALID; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    CnResParams rp;
    rp.scale = scale;
    for (int i = 0; i < count; ++i) {
        const sd_cn_problem& q = problems[i];
        CnResProblem& d = rp.p[rp.count++];
        d.x = static_cast<const half_t*>(q.x); d.ldx = q.ldx; d.w = static_cast<const half_t*>(q.w); d.bias = q.bias;
        d.y = static_cast<half_t*>(q.y); d.ldy = q.ldy; d.M = q.M; d.C = q.C; d.first = rp.total;
        if (q.C <= 0 || q.C % 64 != 0 || q.M <= 0) { set_error("sd_op_controlnet_residuals: C % 64 == 0 and M >= 1 required"); return SD_ERR_UNSUPPORTED; }
        rp.total += cn_residual_tiles(q.M, q.C);
    }
    if (!cn_residual_supported(rp)) { set_error("sd_op_controlnet_residuals: unsupported strides or alignment"); return SD_ERR_UNSUPPORTED; }
    if (mode == 0) return run_op_on_arena(s, iters, ms_per_launch, [&](Ctx& c) { if (!c.dry) c.err = launch_cn_residual(rp, s); });
    // unfused: one GEMM per problem, y = scale (x W^T) + scale b + y, on weights packed as a model's linears are
    if (int rc = pack_begin(s)) return rc;
    WeightStore wst;
    std::vector<ConvW> ws((size_t)count);
    for (int i = 0; i < count; ++i)
        if (int rc = pack_conv_op(wst, problems[i].w, problems[i].C, problems[i].C, 1, problems[i].bias, false, false, &ws[(size_t)i])) return rc;
    if (int rc = pack_end()) return rc;
    if (scale == 0.f) return SD_OK;
    return run_op_on_arena(s, iters, ms_per_launch, [&](Ctx& c) {
        for (int i = 0; i < count; ++i) {
            const sd_cn_problem& q = problems[i];
            View y(static_cast<half_t*>(q.y), q.ldy, q.C);
            ConvArgs f = conv_res(y);
            f.acc_scale = scale; f.bias_scale = scale;
            op_conv(c, ws[(size_t)i], view_of(q.x, q.ldx, q.C), 1, q.M, 1, y, f);
        }
    });
}

int sd_op_cn_fold_scales(const void* const* w, const float* const* bias, const float* scales, int n, int C, void* w_cat,
                         float* b_cat, int iters, float* ms_per_launch, void* stream) {
    if (!w || !bias || !scales || !w_cat || !b_cat) { set_error("sd_op_cn_fold_scales: null argument"); return SD_ERR_INVALID; }
    if (n < 1 || n > kCnMaxNets || C <= 0 || C % 64 != 0) { set_error("sd_op_cn_fold_scales: 1..4 nets, C % 64 == 0 required"); return SD_ERR_INVALID; }
    if ((reinterpret_cast<uintptr_t>(w_cat) & 15) || (reinterpret_cast<uintptr_t>(b_cat) & 15)) { set_error("sd_op_cn_fold_scales: outputs must be 16-byte aligned"); return SD_ERR_UNSUPPORTED; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = pack_begin(s)) return rc;
    WeightStore wst;
    std::vector<ConvW> zs((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (!w[i] || !bias[i]) { set_error("sd_op_cn_fold_scales: null argument"); return SD_ERR_INVALID; }
        if (int rc = pack_conv_op(wst, w[i], C, C, 1, bias[i], false, false, &zs[(size_t)i])) return rc;
    }
    // the fold works on whole packed rows: into packed-size buffers, of which the caller's [C][n C] / [C] are the top
    const long rows = weight_rows(C);
    half_t* wc = static_cast<half_t*>(wst.dmalloc((size_t)rows * n * C * sizeof(half_t)));
    float* bc = static_cast<float*>(wst.dmalloc((size_t)rows * sizeof(float)));
    if (!wc || !bc) { set_error("hipMalloc failed (folded weights)"); return SD_ERR_HIP; }
    if (int rc = pack_end()) return rc;
    CnFoldParams fp;
    fp.n = n; fp.count = 1;
    for (int i = 0; i < n; ++i) { fp.s[0].w[i] = zs[(size_t)i].w; fp.s[0].bias[i] = zs[(size_t)i].bias; fp.scale[i] = scales[i]; }
    fp.s[0].w_cat = wc; fp.s[0].b_cat = bc; fp.s[0].rows = (int)rows; fp.s[0].C = C; fp.s[0].first = 0;
    fp.total = cn_fold_blocks((int)rows, C, n);
    if (iters > 0 && !ms_per_launch) { set_error("ms_per_launch required with iters > 0"); return SD_ERR_INVALID; }
    if (int rc = launch_or_time(s, iters, ms_per_launch, [&]() { return launch_cn_fold_scales(fp, s); })) return rc;
    SD_HIP_CHECK(hipMemcpyAsync(w_cat, wc, (size_t)C * n * C * sizeof(half_t), hipMemcpyDeviceToDevice, s));
    SD_HIP_CHECK(hipMemcpyAsync(b_cat, bc, (size_t)C * sizeof(float), hipMemcpyDeviceToDevice, s));
    SD_HIP_CHECK(hipStreamSynchronize(s));
    return SD_OK;
}

int sd_op_controlnet_residuals_multi(const sd_cn_multi_problem* problems, int count, const float* scales, int n, int mode,
                                     int iters, float* ms_per_launch, void* stream) {
    if (!problems || !scales || count < 1 || count > kCnMaxProblems) { set_error("sd_op_controlnet_residuals_multi: 1..16 problems"); return SD_ERR_INVALID; }
    if (n < 1 || n > kCnMaxNets) { set_error("sd_op_controlnet_residuals_multi: 1..4 nets"); return SD_ERR_INVALID; }
    if (mode != 0 && mode != 1) { set_error("sd_op_controlnet_residuals_multi: mode must be 0 (chained) or 1 (folded, one GEMM)"); return SD_ERR_INVALID; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int i = 0; i < count; ++i) {
        const sd_cn_multi_problem& q = problems[i];
        if (q.C <= 0 || q.C % 64 != 0 || q.M <= 0 || !q.y || q.ldy < q.C) { set_error("sd_op_controlnet_residuals_multi: C % 64 == 0, M >= 1, ldy >= C required"); return SD_ERR_INVALID; }
        for (int j = 0; j < n; ++j)
            if (!q.x[j] || !q.w[j] || !q.bias[j] || q.ldx[j] < q.C || q.ldx[j] % 8 != 0 || (reinterpret_cast<uintptr_t>(q.x[j]) & 15)) {
                set_error("sd_op_controlnet_residuals_multi: null or misaligned source"); return SD_ERR_INVALID;
            }
        if (mode == 1)
            for (int j = 1; j < n; ++j)
                if (q.ldx[j] != q.ldx[0] || static_cast<const half_t*>(q.x[j]) != static_cast<const half_t*>(q.x[0]) + (long)j * q.C) {
                    set_error("sd_op_controlnet_residuals_multi: mode 1 takes sources that are neighbouring column slices of one buffer");
                    return SD_ERR_INVALID;
                }
    }
    if (int rc = pack_begin(s)) return rc;
    WeightStore wst;
    std::vector<ConvW> zs((size_t)count * n);
    std::vector<ConvW> cat((size_t)count);
    CnFoldParams fp;
    fp.n = n;
    for (int i = 0; i < count; ++i) {
        const sd_cn_multi_problem& q = problems[i];
        for (int j = 0; j < n; ++j)
            if (int rc = pack_conv_op(wst, q.w[j], q.C, q.C, 1, q.bias[j], false, false, &zs[(size_t)i * n + j])) return rc;
        if (mode == 1) {
            const long rows = weight_rows(q.C);
            ConvW& zw = cat[(size_t)i];
            zw.w = static_cast<half_t*>(wst.dmalloc((size_t)rows * n * q.C * sizeof(half_t)));
            zw.bias = static_cast<float*>(wst.dmalloc((size_t)rows * sizeof(float)));
            if (!zw.w || !zw.bias) { set_error("hipMalloc failed (folded weights)"); return SD_ERR_HIP; }
            zw.cin = n * q.C; zw.cout = q.C; zw.ks = 1; zw.K = (long)n * q.C;
            CnFoldSite& f = fp.s[fp.count++];
            for (int j = 0; j < n; ++j) { f.w[j] = zs[(size_t)i * n + j].w; f.bias[j] = zs[(size_t)i * n + j].bias; }
            f.w_cat = zw.w; f.b_cat = zw.bias; f.rows = (int)rows; f.C = q.C; f.first = fp.total;
            fp.total += cn_fold_blocks((int)rows, q.C, n);
        }
    }
    for (int j = 0; j < n; ++j) fp.scale[j] = scales[j];
    if (int rc = pack_end()) return rc;
    if (mode == 1) {
        // one grouped fold launch over all problems, as the forward issues it when the scales change (timed on its own)
        if (iters > 0 && !ms_per_launch) { set_error("ms_per_launch required with iters > 0"); return SD_ERR_INVALID; }
        if (int rc = launch_or_time(s, iters, iters > 0 ? ms_per_launch + 1 : nullptr, [&]() { return launch_cn_fold_scales(fp, s); })) return rc;
        return run_op_on_arena(s, iters, ms_per_launch, [&](Ctx& c) {
            for (int i = 0; i < count; ++i) {
                const sd_cn_multi_problem& q = problems[i];
                View y(static_cast<half_t*>(q.y), q.ldy, q.C);
                op_conv(c, cat[(size_t)i], view_of(q.x[0], q.ldx[0], n * q.C), 1, q.M, 1, y, conv_res(y));
            }
        });
    }
    return run_op_on_arena(s, iters, ms_per_launch, [&](Ctx& c) {
        for (int i = 0; i < count; ++i) {
            const sd_cn_multi_problem& q = problems[i];
            View y(static_cast<half_t*>(q.y), q.ldy, q.C);
            for (int j = 0; j < n; ++j) {
                if (scales[j] == 0.f) continue;
                ConvArgs f = conv_res(y);
                f.acc_scale = scales[j]; f.bias_scale = scales[j];
                op_conv(c, zs[(size_t)i * n + j], view_of(q.x[j], q.ldx[j], q.C), 1, q.M, 1, y, f);
            }
        }
    });
}

int sd_op_controlnet_cond_embed(sd_controlnet* cn, const void* image, int n, int H, int W, void* out, int iters,
                                float* ms_per_launch, void* stream) {
    if (!cn || !image || !out) { set_error("null argument"); return SD_ERR_INVALID; }
    if (!cn->impl.finalized) { set_error("sd_op_controlnet_cond_embed: ControlNet not finalized"); return SD_ERR_STATE; }
    if (n < 1 || H < 1 || W < 1) { set_error("sd_op_controlnet_cond_embed: bad shape"); return SD_ERR_INVALID; }
    const int C0 = cn->impl.cfg.block_out_channels[0];
    return run_op_on_arena(static_cast<hipStream_t>(stream), iters, ms_per_launch, [&](Ctx& c) {
        cn->impl.run_cond_embed(c, static_cast<const half_t*>(image), n, H, W, View(static_cast<half_t*>(out), C0, C0));
    });
}

int sd_op_cn_cond_conv(const void* x, int nchw, const void* w_oihw_f16, const void* bias_f16, int N, int IH, int IW, int Cin,
                       int Cout, int stride, int silu, void* y, void* stream) {
    if (!x || !w_oihw_f16 || !bias_f16 || !y) { set_error("sd_op_cn_cond_conv: null argument"); return SD_ERR_INVALID; }
    CnCondConvParams p;
    p.x = static_cast<const half_t*>(x); p.nchw = nchw != 0;
    p.y = static_cast<half_t*>(y);
    p.N = N; p.IH = IH; p.IW = IW; p.Cin = Cin; p.Cout = Cout; p.stride = stride; p.silu = silu != 0;
    if (stride == 1 || stride == 2) { p.OH = (IH - 1) / stride + 1; p.OW = (IW - 1) / stride + 1; }
    if (!cn_cond_conv_supported(p)) { set_error("sd_op_cn_cond_conv: unsupported layer"); return SD_ERR_UNSUPPORTED; }
    // the weights and the bias as ControlNet::finalize packs them, here into the entry's arena
    return run_op_on_arena(static_cast<hipStream_t>(stream), 0, nullptr, [&](Ctx& c) {
        float* w = c.arena->alloc_f((long)Cout * Cin * 9);
        float* b = c.arena->alloc_f(Cout);
        if (c.dry || c.err) return;
        c.err = launch_cn_pack_cond(static_cast<const half_t*>(w_oihw_f16), w, Cout, Cin, c.stream);
        if (!c.err) c.err = launch_f16_to_f32(static_cast<const half_t*>(bias_f16), b, Cout, c.stream);
        p.w = w; p.bias = b;
        if (!c.err) c.err = launch_cn_cond_conv(p, c.stream);
    });
}

int sd_op_fold_linear(const void* w_outer, const void* b_outer, const void* w_inner, const void* b_inner, void* w_folded,
                      float* b_folded, int O, int J, int K, void* stream) {
    if (!w_outer || !b_outer || !w_inner || !b_inner || !w_folded || !b_folded || O < 1 || J < 1 || K < 1 || (K + J) % 64 != 0) {
        set_error("sd_op_fold_linear: bad arguments (K + J must be a multiple of 64)"); return SD_ERR_INVALID;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    SD_HIP_CHECK(hipStreamSynchronize(s));              // the pack helpers work on the null stream
    WeightStore ws;
    const int64_t so[2] = {O, J}, si[2] = {J, K}, sbo[1] = {O}, sbi[1] = {J};
    ws.declare("o.weight", {O, J}); ws.declare("o.bias", {O});
    ws.declare("i.weight", {J, K}); ws.declare("i.bias", {J});
    int rc;
    if ((rc = ws.set("o.weight", w_outer, so, 2, 0)) || (rc = ws.set("o.bias", b_outer, sbo, 1, 1)) ||
        (rc = ws.set("i.weight", w_inner, si, 2, 0)) || (rc = ws.set("i.bias", b_inner, sbi, 1, 1))) return rc;
    ConvW f;
    if ((rc = ws.fold_linear("o", "i", &f))) return rc;
    SD_HIP_CHECK(hipMemcpy(w_folded, f.w, (size_t)O * f.K * sizeof(half_t), hipMemcpyDeviceToDevice));
    SD_HIP_CHECK(hipMemcpy(b_folded, f.bias, (size_t)O * sizeof(float), hipMemcpyDeviceToDevice));
    SD_HIP_CHECK(hipDeviceSynchronize());
    return SD_OK;
}

int sd_upconv_fold_supported(int N, int H, int W, int Cin, int Cout) {
    return upconv_fold_supported(N, H, W, Cin, Cout, Cin) ? 1 : 0;
}

int sd_op_fold_upconv(const void* w_oihw, void* out, int Cout, int Cin, void* stream) {
    if (!w_oihw || !out || Cout < 1 || Cin < 64 || Cin % 64 != 0) {
        set_error("sd_op_fold_upconv: bad arguments (Cin must be a multiple of 64)"); return SD_ERR_INVALID;
    }
    if (Cout % 8 != 0) { set_error("sd_op_fold_upconv: no folded pack is built for Cout % 8 != 0"); return SD_ERR_UNSUPPORTED; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = pack_begin(s)) return rc;
    WeightStore ws;
    ConvW cw;
    if (int rc = ws.pack_conv(static_cast<const half_t*>(w_oihw), Cout, Cin, 3, 3, nullptr, &cw, true)) return rc;
    const long K4 = 4L * Cin, rows = weight_rows(Cout);
    for (int par = 0; par < 4; ++par)           // the panels without their row padding
        SD_HIP_CHECK(hipMemcpyAsync(static_cast<half_t*>(out) + (long)par * Cout * K4, cw.w_up + (long)par * rows * K4,
                                    (size_t)Cout * K4 * sizeof(half_t), hipMemcpyDeviceToDevice, 0));
    return pack_end();
}

int sd_op_upconv2x_ex(const void* x, const void* w_oihw, const void* bias_f32, const void* rowadd_f32, const void* res,
                      void* y, int N, int H, int W, int Cin, int Cout, int64_t ldx, int64_t ldres, int64_t ldy,
                      float acc_scale, float bias_scale, int gn_groups, float* gn_summaries, int* ran, void* stream) {
    if (!x || !w_oihw || !y || !ran || N < 1 || H < 1 || W < 1 || Cin < 64 || Cin % 64 != 0 || Cout < 1 || gn_groups < 0 ||
        !(acc_scale > 0.f) || !(bias_scale > 0.f)) {
        set_error("sd_op_upconv2x_ex: bad arguments (Cin % 64 == 0, positive scales)"); return SD_ERR_INVALID;
    }
    auto ld_ok = [](int64_t ld, int dense) { return ld == dense || (ld > dense && ld % 8 == 0); };
    if (!ld_ok(ldx, Cin) || !ld_ok(ldy, Cout) || (res && !ld_ok(ldres, Cout))) {
        set_error("sd_op_upconv2x_ex: ldx / ldres / ldy must be the dense width or a wider multiple of 8"); return SD_ERR_INVALID;
    }
    for (int i = 0; i < 4; ++i) ran[i] = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = pack_begin(s)) return rc;
    WeightStore ws;
    ConvW cw;                               // both packs, where a model's upsampler conv gets both
    int rc = pack_conv_op(ws, w_oihw, Cout, Cin, 3, bias_f32, false, true, &cw);
    if (rc) return rc;
    GnStatBuf gb;
    if (gn_groups > 0 && !(gb.buf = static_cast<float*>(ws.dmalloc((size_t)gnstat_floats(N, 4L * H * W, gn_groups) * sizeof(float))))) {
        set_error("hipMalloc failed (GroupNorm summaries)"); return SD_ERR_HIP;
    }
    if ((rc = pack_end())) return rc;
    ConvLaunch l;
    const View yv = view_of(y, ldy, Cout), rv = view_of(res, ldres, Cout);
    rc = run_op_on_arena(s, 0, nullptr, [&](Ctx& c) {
        ConvArgs f = conv_res(rv);
        f.up = 1;
        f.rowadd = static_cast<const float*>(rowadd_f32); f.rowadd_ld = Cout;
        f.acc_scale = acc_scale; f.bias_scale = bias_scale;
        f.gn_out = gn_groups > 0 ? &gb : nullptr; f.gn_groups = gn_groups;
        if (conv_prepare(c, cw, view_of(x, ldx, Cin), N, H, W, yv, f, &l)) conv_launch(c, l, yv, nullptr);
    });
    if (rc) return rc;
    ran[0] = l.plan.kind == kKindUpconvFold;
    if (gb.st.part) {
        ran[1] = gb.st.S; ran[2] = (int)gb.st.rows;
        if (gn_summaries)
            SD_HIP_CHECK(hipMemcpyAsync(gn_summaries, gb.st.part, (size_t)N * gb.st.S * gn_groups * 2 * sizeof(float),
                                        hipMemcpyDeviceToDevice, s));
    }
    SD_HIP_CHECK(hipStreamSynchronize(s));
    return SD_OK;
}

int sd_op_ffn_geglu_proj_out(const void* x_in, const void* t3, const void* ln_gamma, const void* ln_beta, float ln_eps,
                             const void* w1, const void* b1, const void* w2, const void* b2, const void* w_po,
                             const void* b_po, void* y, float* gn_summaries, int* gn_rows, int M, int C, int imgs, int* fused,
                             void* stream) {
    if (!x_in || !t3 || !ln_gamma || !ln_beta || !w1 || !b1 || !w2 || !b2 || !w_po || !b_po || !y || M < 1 || C < 64 ||
        C % 64 != 0 || imgs < 1 || M % imgs != 0 || ln_eps != 1e-5f) {
        set_error("sd_op_ffn_geglu_proj_out: bad arguments (C % 64, M % imgs, ln_eps = 1e-5: the transformer's)"); return SD_ERR_INVALID;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    SD_HIP_CHECK(hipStreamSynchronize(s));              // the pack helpers work on the null stream
    const int G = 32;                                   // the UNet's GroupNorm groups
    WeightStore ws;
    const int64_t C8 = 8L * C, C4 = 4L * C;
    const int64_t s1[2] = {C8, C}, s2[2] = {C, C4}, so[2] = {C, C}, sc[1] = {C}, s8[1] = {C8};
    ws.declare("norm3.weight", {C}); ws.declare("norm3.bias", {C});
    ws.declare("ff.net.0.proj.weight", {C8, C}); ws.declare("ff.net.0.proj.bias", {C8});
    ws.declare("ff.net.2.weight", {C, C4}); ws.declare("ff.net.2.bias", {C});
    ws.declare("proj_out.weight", {C, C}); ws.declare("proj_out.bias", {C});
    int rc;
    if ((rc = ws.set("norm3.weight", ln_gamma, sc, 1, 1)) || (rc = ws.set("norm3.bias", ln_beta, sc, 1, 1)) ||
        (rc = ws.set("ff.net.0.proj.weight", w1, s1, 2, 0)) || (rc = ws.set("ff.net.0.proj.bias", b1, s8, 1, 1)) ||
        (rc = ws.set("ff.net.2.weight", w2, s2, 2, 0)) || (rc = ws.set("ff.net.2.bias", b2, sc, 1, 1)) ||
        (rc = ws.set("proj_out.weight", w_po, so, 2, 0)) || (rc = ws.set("proj_out.bias", b_po, sc, 1, 1))) return rc;
    // packed as Encoder::pack_xformer packs the last block of a transformer
    Xformer t;
    t.C = C;
    t.blocks.resize(1);
    TBlock& b = t.blocks[0];
    if ((rc = ws.pack_norm("norm3", &b.ln3)) || (rc = ws.pack_geglu("ff.net.0.proj", &b.ff1))) return rc;
    b.fold = true;
    if ((rc = ws.fold_ln(&b.ff1, b.ln3, 0, 1.0f)) || (rc = pack_xformer_tail(ws, "proj_out", "ff.net.2", &t, &b))) return rc;
    SD_HIP_CHECK(hipDeviceSynchronize());
    const long HW = M / imgs;
    if (gn_summaries && (!gn_rows || !gn_wants_stats(HW, C, G))) {
        set_error("sd_op_ffn_geglu_proj_out: summaries need gn_rows and a map the GroupNorm takes summaries for"); return SD_ERR_INVALID;
    }
    bool ran_fused = false;
    GnStatBuf gb;
    rc = run_op_on_arena(s, 0, nullptr, [&](Ctx& c) {
        Arena& a = *c.arena;
        RowStat st;
        st.p = a.alloc_f(rowstat_floats(M, C));
        st.parts = 1; st.width = C;
        View t3v = xformer_tail_t3(a, t, M);
        View nxt(a.alloc_h((long)M * C), C, C);
        if (!c.dry) {
            hipError_t e = hipMemcpy2DAsync(t3v.p, (size_t)t3v.ld * 2, t3, (size_t)C * 2, (size_t)C * 2, (size_t)M,
                                            hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) { set_error(hipGetErrorString(e)); c.err = SD_ERR_HIP; return; }
            c.err = launch_row_stats(t3v.p, t3v.ld, st.p, M, C, s);
        }
        gb = GnStatBuf();
        gb.buf = gn_summaries;
        ConvArgs fo;
        fo.gn_out = gn_summaries ? &gb : nullptr;
        fo.gn_groups = G;
        View x(const_cast<half_t*>(static_cast<const half_t*>(x_in)), C, C);
        ran_fused = run_xformer_tail(c, t, t3v, st, View(), nxt, x, imgs, (int)HW, 1, View(static_cast<half_t*>(y), C, C), fo);
    });
    if (fused) *fused = ran_fused ? 1 : 0;
    if (gn_rows) *gn_rows = gb.st.part ? (int)gb.st.rows : 0;
    return rc;
}

int sd_op_vae_tiles_gather(const void* canvas, int64_t ld, void* stack, const int* bs, const int* ys, const int* xs, int n,
                           int B, int C, int Hc, int Wc, int th, int tw, int iters, float* ms_per_launch, void* stream) {
    if (!canvas || !stack || !bs || !ys || !xs || n < 1 || n > VAE_TILE_MAX_BATCH || B < 1 || C < 1 || th < 1 || tw < 1 ||
        th > Hc || tw > Wc || ld < Wc) {
        set_error("sd_op_vae_tiles_gather: bad arguments (non-null pointers, 1..32 tiles no larger than the canvas, ld >= Wc)");
        return SD_ERR_INVALID;
    }
    if (iters > 0 && !ms_per_launch) { set_error("ms_per_launch required with iters > 0"); return SD_ERR_INVALID; }
    VaeGatherList l = {};
    for (int i = 0; i < n; ++i) {
        if (bs[i] < 0 || bs[i] >= B || ys[i] < 0 || ys[i] > Hc - th || xs[i] < 0 || xs[i] > Wc - tw) {
            set_error("sd_op_vae_tiles_gather: a tile outside the canvas"); return SD_ERR_INVALID;
        }
        l.b[i] = bs[i]; l.ys[i] = ys[i]; l.xs[i] = xs[i];
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    return launch_or_time(s, iters, ms_per_launch, [&]() {
        return launch_vae_tile_gather(static_cast<const half_t*>(canvas), ld, static_cast<half_t*>(stack), l, n, C, Hc, th, tw, s);
    });
}

int sd_op_vae_tiles_merge(const void* tiles, int64_t stack_elems, void* canvas, int64_t ld, const sd_vae_tiles* plan, int B,
                          int C, int iters, float* ms_per_launch, void* stream) {
    if (!tiles || !canvas || !plan || B < 1 || C < 1) { set_error("sd_op_vae_tiles_merge: null argument, or B or C < 1"); return SD_ERR_INVALID; }
    if (iters > 0 && !ms_per_launch) { set_error("ms_per_launch required with iters > 0"); return SD_ERR_INVALID; }
    if (!vae_tile_plan_valid(*plan)) { set_error("sd_op_vae_tiles_merge: not a plan of sd_vae_tile_plan"); return SD_ERR_INVALID; }
    VaeMergeGeom g;
    const long need = vae_tile_stack(*plan, B, C, &g, nullptr);
    if (stack_elems < need || ld < plan->out_w) {
        set_error("sd_op_vae_tiles_merge: `tiles` is smaller than the plan's stack, or ld below the canvas width");
        return SD_ERR_INVALID;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    return launch_or_time(s, iters, ms_per_launch, [&]() {
        return launch_vae_tile_merge(static_cast<const half_t*>(tiles), static_cast<half_t*>(canvas), ld, g, s);
    });
}

}  // extern "C"
