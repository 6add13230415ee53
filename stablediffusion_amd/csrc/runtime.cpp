// Arena, weight store and op wrappers of the denoise engine (host side, HIP runtime only).
#include "engine.h"

#include <atomic>
#include <cstdio>
#include <mutex>
#include <cstdlib>
#include <cstring>

namespace sd {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }
const std::string& last_error() { return g_last_error; }

// ------------------------------------------------------------------------------------------ Arena
Arena::~Arena() {
    if (base_) (void)hipFree(base_);
}

int Arena::reserve(size_t bytes) {
    if (bytes <= cap_) return 0;
    if (base_) { (void)hipFree(base_); base_ = nullptr; cap_ = 0; }
    SD_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&base_), bytes));
    cap_ = bytes;
    return 0;
}

void* Arena::alloc(size_t bytes) {
    const size_t aligned = (bytes + 255) & ~size_t(255);
    const size_t at = off_;
    off_ += aligned;
    if (off_ > peak_) peak_ = off_;
    if (dry_) return reinterpret_cast<void*>(uintptr_t(0x1000) + at);  // never dereferenced
    if (off_ > cap_) { overflow_ = true; return base_; }
    return base_ + at;
}

// ------------------------------------------------------------------------------------ WeightStore
WeightStore::~WeightStore() {
    free_raw();
    for (void* p : owned_) (void)hipFree(p);
}

void* WeightStore::dmalloc(size_t bytes) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 256) != hipSuccess) return nullptr;
    owned_.push_back(p);
    packed_bytes_ += (int64_t)bytes;
    return p;
}

void WeightStore::declare(const std::string& key, std::vector<int64_t> shape) {
    RawTensor t;
    t.shape = std::move(shape);
    t.numel = 1;
    for (auto s : t.shape) t.numel *= s;
    tensors.emplace(key, std::move(t));
    order.push_back(key);
}

int WeightStore::set(const std::string& key, const void* data, const int64_t* shape, int ndim, int dtype) {
    auto it = tensors.find(key);
    if (it == tensors.end()) { set_error("unknown weight key: " + key); return 1; }
    RawTensor& t = it->second;
    if ((int)t.shape.size() != ndim) { set_error("rank mismatch for " + key); return 1; }
    for (int i = 0; i < ndim; ++i)
        if (t.shape[i] != shape[i]) {
            set_error("shape mismatch for " + key + " at dim " + std::to_string(i) + ": expected " +
                      std::to_string(t.shape[i]) + ", got " + std::to_string(shape[i]));
            return 1;
        }
    if (!t.dev) SD_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&t.dev), (size_t)t.numel * sizeof(half_t)));
    if (dtype == 0) {
        SD_HIP_CHECK(hipMemcpy(t.dev, data, (size_t)t.numel * sizeof(half_t), hipMemcpyDefault));
    } else if (dtype == 1) {
        float* tmp = nullptr;
        SD_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&tmp), (size_t)t.numel * sizeof(float)));
        hipError_t e = hipMemcpy(tmp, data, (size_t)t.numel * sizeof(float), hipMemcpyDefault);
        int rc = 0;
        if (e == hipSuccess) rc = launch_f32_to_f16(tmp, t.dev, t.numel, 0);
        if (e == hipSuccess && rc == 0) e = hipStreamSynchronize(0);
        (void)hipFree(tmp);
        if (e != hipSuccess) { set_error(std::string("set_weight copy: ") + hipGetErrorString(e)); return 3; }
        if (rc) return rc;
    } else {
        set_error("unsupported dtype code");
        return 1;
    }
    return 0;
}

bool WeightStore::complete(std::string* missing) const {
    for (const auto& k : order) {
        auto it = tensors.find(k);
        if (it == tensors.end() || !it->second.dev) {
            if (missing) *missing = k;
            return false;
        }
    }
    return true;
}

const RawTensor* WeightStore::raw(const std::string& key) const {
    auto it = tensors.find(key);
    if (it == tensors.end() || !it->second.dev) return nullptr;
    return &it->second;
}

void WeightStore::free_raw() {
    for (auto& kv : tensors)
        if (kv.second.dev) { (void)hipFree(kv.second.dev); kv.second.dev = nullptr; }
}

int WeightStore::host_floats(const std::string& key, std::vector<float>* out) const {
    const RawTensor* t = raw(key);
    if (!t) { set_error("missing weight: " + key); return 2; }
    std::vector<half_t> h((size_t)t->numel);
    SD_HIP_CHECK(hipMemcpy(h.data(), t->dev, (size_t)t->numel * sizeof(half_t), hipMemcpyDeviceToHost));
    out->resize((size_t)t->numel);
    for (long i = 0; i < t->numel; ++i) (*out)[(size_t)i] = (float)h[(size_t)i];
    return 0;
}

static long round_up(long a, long b) { return (a + b - 1) / b * b; }

static int upload_bias(WeightStore* ws, const float* host, int cout, float** dst) {
    const long padded = weight_rows(cout);
    std::vector<float> buf((size_t)padded, 0.f);
    std::memcpy(buf.data(), host, (size_t)cout * sizeof(float));
    *dst = static_cast<float*>(ws->dmalloc((size_t)padded * sizeof(float)));
    if (!*dst) { set_error("hipMalloc failed (bias)"); return 3; }
    SD_HIP_CHECK(hipMemcpy(*dst, buf.data(), (size_t)padded * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

int WeightStore::pack_conv(const std::string& prefix, ConvW* out, bool has_bias, bool fold_up2x) {
    const RawTensor* w = raw(prefix + ".weight");
    if (!w) { set_error("missing weight: " + prefix + ".weight"); return 2; }
    const int KH = w->shape.size() == 4 ? (int)w->shape[2] : 1;
    const int KW = w->shape.size() == 4 ? (int)w->shape[3] : 1;
    std::vector<float> b;
    if (has_bias)
        if (int rc = host_floats(prefix + ".bias", &b)) return rc;
    return pack_conv(w->dev, (int)w->shape[0], (int)w->shape[1], KH, KW, has_bias ? b.data() : nullptr, out, fold_up2x);
}

int WeightStore::pack_conv(const half_t* w_dev, int O, int I, int KH, int KW, const float* bias_host, ConvW* out,
                           bool fold_up2x) {
    const long K = round_up((long)KH * KW * I, 64);
    const long rows = weight_rows(O);
    out->cin = I; out->cout = O; out->ks = KH; out->K = K;
    out->w = static_cast<half_t*>(dmalloc((size_t)rows * K * sizeof(half_t)));
    if (!out->w) { set_error("hipMalloc failed (weights)"); return 3; }
    SD_HIP_CHECK(hipMemsetAsync(out->w, 0, (size_t)rows * K * sizeof(half_t), 0));
    int rc = launch_pack_conv(w_dev, out->w, O, I, KH, KW, K, 0);
    if (rc) return rc;
    out->w_up = nullptr;
    if (fold_up2x && KH == 3 && KW == 3 && I % 64 == 0 && O % 8 == 0) {
        // 16/9 of the 9-tap pack on top of it; both stay, the map size at launch decides which runs (op_conv)
        const size_t bytes = (size_t)4 * rows * 4 * I * sizeof(half_t);
        out->w_up = static_cast<half_t*>(dmalloc(bytes));
        if (!out->w_up) { set_error("hipMalloc failed (folded upsample weights)"); return 3; }
        SD_HIP_CHECK(hipMemsetAsync(out->w_up, 0, bytes, 0));
        if ((rc = launch_fold_upconv(w_dev, out->w_up, O, I, 0))) return rc;
    }
    out->bias = nullptr;
    return bias_host ? upload_bias(this, bias_host, O, &out->bias) : 0;
}

int WeightStore::pack_rows(const std::vector<std::string>& wkeys, const std::vector<std::string>& bkeys,
                           ConvW* out) {
    long total = 0;
    int I = -1;
    for (const auto& k : wkeys) {
        const RawTensor* w = raw(k);
        if (!w) { set_error("missing weight: " + k); return 2; }
        if (I < 0) I = (int)w->shape[1];
        if ((int)w->shape[1] != I) { set_error("pack_rows: inner dims differ at " + k); return 1; }
        total += w->shape[0];
    }
    if (I % 64 != 0) { set_error("pack_rows: inner dim must be a multiple of 64"); return 1; }
    const long rows = weight_rows(total);
    out->cin = I; out->cout = (int)total; out->ks = 1; out->K = I;
    out->w = static_cast<half_t*>(dmalloc((size_t)rows * I * sizeof(half_t)));
    if (!out->w) { set_error("hipMalloc failed (weights)"); return 3; }
    SD_HIP_CHECK(hipMemsetAsync(out->w, 0, (size_t)rows * I * sizeof(half_t), 0));
    long r = 0;
    for (const auto& k : wkeys) {
        const RawTensor* w = raw(k);
        SD_HIP_CHECK(hipMemcpyAsync(out->w + r * I, w->dev, (size_t)w->numel * sizeof(half_t),
                                    hipMemcpyDeviceToDevice, 0));
        r += w->shape[0];
    }
    out->bias = nullptr;
    if (!bkeys.empty()) {
        std::vector<float> all;
        for (const auto& k : bkeys) {
            std::vector<float> b;
            int rc = host_floats(k, &b);
            if (rc) return rc;
            all.insert(all.end(), b.begin(), b.end());
        }
        if ((long)all.size() != total) { set_error("pack_rows: bias length mismatch"); return 1; }
        int rc = upload_bias(this, all.data(), (int)total, &out->bias);
        if (rc) return rc;
    }
    return 0;
}

// GEGLU projection [8C][C]: rows 0..4C-1 = hidden, 4C..8C-1 = gate (diffusers GEGLU: hidden, gate =
// proj.chunk(2)).  Packed so that every 128-row group holds 64 hidden rows followed by their 64
// gate rows -- the igemm epilogue then finds both halves of out = hidden * gelu(gate) in one tile.
int WeightStore::pack_geglu(const std::string& prefix, ConvW* out) {
    const RawTensor* w = raw(prefix + ".weight");
    if (!w) { set_error("missing weight: " + prefix + ".weight"); return 2; }
    std::vector<float> b;
    if (int rc = host_floats(prefix + ".bias", &b)) return rc;
    return pack_geglu(w->dev, w->shape[0], w->shape[1], b.data(), out);
}

int WeightStore::pack_geglu(const half_t* w_dev, long O, long I, const float* b, ConvW* out) {
    const long half_rows = O / 2;
    if (half_rows % 64 != 0 || I % 64 != 0) { set_error("pack_geglu: dims must be multiples of 64"); return 1; }
    const long rows = weight_rows(O);
    out->cin = (int)I; out->cout = (int)O; out->ks = 1; out->K = I;
    out->w = static_cast<half_t*>(dmalloc((size_t)rows * I * sizeof(half_t)));
    if (!out->w) { set_error("hipMalloc failed (weights)"); return 3; }
    SD_HIP_CHECK(hipMemsetAsync(out->w, 0, (size_t)rows * I * sizeof(half_t), 0));
    std::vector<float> bp((size_t)O, 0.f);
    for (long blk = 0; blk < half_rows / 64; ++blk) {
        SD_HIP_CHECK(hipMemcpyAsync(out->w + (blk * 128) * I, w_dev + (blk * 64) * I,
                                    (size_t)64 * I * sizeof(half_t), hipMemcpyDeviceToDevice, 0));
        SD_HIP_CHECK(hipMemcpyAsync(out->w + (blk * 128 + 64) * I, w_dev + (half_rows + blk * 64) * I,
                                    (size_t)64 * I * sizeof(half_t), hipMemcpyDeviceToDevice, 0));
        for (int e = 0; b && e < 64; ++e) {
            bp[(size_t)(blk * 128 + e)] = b[(size_t)(blk * 64 + e)];
            bp[(size_t)(blk * 128 + 64 + e)] = b[(size_t)(half_rows + blk * 64 + e)];
        }
    }
    return upload_bias(this, bp.data(), (int)O, &out->bias);
}

int WeightStore::pack_norm(const std::string& prefix, NormW* out) {
    std::vector<float> g, b;
    int rc = host_floats(prefix + ".weight", &g);
    if (rc) return rc;
    rc = host_floats(prefix + ".bias", &b);
    if (rc) return rc;
    if (b.size() != g.size()) { set_error("pack_norm: " + prefix + ".weight and .bias differ in length"); return 1; }
    return pack_norm(g.data(), b.data(), (int)g.size(), out);
}

int WeightStore::pack_norm(const float* g, const float* b, int C, NormW* out) {
    const size_t n = (size_t)C;
    out->C = C;
    out->gamma = static_cast<float*>(dmalloc(n * sizeof(float)));
    out->beta = static_cast<float*>(dmalloc(n * sizeof(float)));
    if (!out->gamma || !out->beta) { set_error("hipMalloc failed (norm)"); return 3; }
    SD_HIP_CHECK(hipMemcpy(out->gamma, g, n * sizeof(float), hipMemcpyHostToDevice));
    SD_HIP_CHECK(hipMemcpy(out->beta, b, n * sizeof(float), hipMemcpyHostToDevice));
    out->gb = nullptr;
    if (n % 64 == 0) {                 // packed per 64 channels for the convolution-fused GroupNorm
        std::vector<float> gb(2 * n);
        for (size_t blk = 0; blk < n / 64; ++blk)
            for (int e = 0; e < 64; ++e) {
                gb[blk * 128 + e] = g[blk * 64 + e];
                gb[blk * 128 + 64 + e] = b[blk * 64 + e];
            }
        out->gb = static_cast<float*>(dmalloc(gb.size() * sizeof(float)));
        if (!out->gb) { set_error("hipMalloc failed (norm)"); return 3; }
        SD_HIP_CHECK(hipMemcpy(out->gb, gb.data(), gb.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    return 0;
}

int WeightStore::fold_ln(ConvW* w, const NormW& ln, int rows_scaled, float row_scale) {
    if (ln.C != w->K || w->ks != 1) { set_error("fold_ln: LayerNorm width must equal the linear's K"); return 1; }
    const long padded = weight_rows(w->cout);
    float* nb = static_cast<float*>(dmalloc((size_t)padded * sizeof(float)));
    w->wsum = static_cast<float*>(dmalloc((size_t)padded * sizeof(float)));
    if (!nb || !w->wsum) { set_error("hipMalloc failed (fold_ln)"); return 3; }
    SD_HIP_CHECK(hipMemsetAsync(nb, 0, (size_t)padded * sizeof(float), 0));
    SD_HIP_CHECK(hipMemsetAsync(w->wsum, 0, (size_t)padded * sizeof(float), 0));
    int rc = launch_ln_fold(w->w, w->K, w->cout, ln.gamma, ln.beta, w->bias, nb, w->wsum, rows_scaled, row_scale, 0);
    if (rc) return rc;
    w->bias = nb;
    return 0;
}

int WeightStore::fold_linear(const std::string& outer, const std::string& inner, ConvW* out) {
    const RawTensor* wo = raw(outer + ".weight");
    const RawTensor* wi = raw(inner + ".weight");
    if (!wo || !wi) { set_error("missing weight: " + (wo ? inner : outer) + ".weight"); return 2; }
    for (size_t d = 2; d < wo->shape.size(); ++d)
        if (wo->shape[d] != 1) { set_error("fold_linear: " + outer + " is not pointwise"); return 1; }
    if (wi->shape.size() != 2 || wo->shape.size() < 2 || wo->shape[1] != wi->shape[0]) {
        set_error("fold_linear: " + outer + " does not take the output of " + inner); return 1;
    }
    const int O = (int)wo->shape[0], J = (int)wo->shape[1], Ki = (int)wi->shape[1];
    const long K = round_up((long)Ki + J, 64);
    const long rows = weight_rows(O);
    out->cin = Ki + J; out->cout = O; out->ks = 1; out->K = K;
    out->w = static_cast<half_t*>(dmalloc((size_t)rows * K * sizeof(half_t)));
    if (!out->w) { set_error("hipMalloc failed (weights)"); return 3; }
    SD_HIP_CHECK(hipMemsetAsync(out->w, 0, (size_t)rows * K * sizeof(half_t), 0));
    int rc = launch_fold_linear(wo->dev, wi->dev, out->w, O, J, Ki, K, 0);
    if (rc) return rc;
    std::vector<float> wof, bi, bo, b((size_t)O);
    if ((rc = host_floats(outer + ".weight", &wof))) return rc;
    if ((rc = host_floats(inner + ".bias", &bi))) return rc;
    if ((rc = host_floats(outer + ".bias", &bo))) return rc;
    if ((long)bi.size() != J || (long)bo.size() != O) { set_error("fold_linear: bias length mismatch"); return 1; }
    for (int n = 0; n < O; ++n) {
        double acc = bo[(size_t)n];
        for (int j = 0; j < J; ++j) acc += (double)wof[(size_t)n * J + j] * bi[(size_t)j];
        b[(size_t)n] = (float)acc;
    }
    return upload_bias(this, b.data(), O, &out->bias);
}

// ---------------------------------------------------------------------------------------- profiler
namespace {
// The profiler is process-wide (bench.py brackets one forward at a time); the record list is guarded so that
// two handles driven from two threads cannot corrupt it -- their rows would interleave, nothing worse.
struct ProfRec { std::string name; double flops, bytes; hipEvent_t a, b; };
std::atomic<bool> g_prof_on{false};
std::mutex g_prof_mu;
std::vector<ProfRec> g_prof;
}  // namespace
void prof_enable(bool on) { g_prof_on = on; }
bool prof_enabled() { return g_prof_on; }
void prof_open(hipStream_t s, const char* kernel, double flops, double bytes) {
    if (!g_prof_on) return;
    ProfRec r{kernel, flops, bytes, nullptr, nullptr};
    if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return;
    (void)hipEventRecord(r.a, s);
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof.push_back(r);
}
void prof_close(hipStream_t s) {
    if (!g_prof_on) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (g_prof.empty()) return;
    (void)hipEventRecord(g_prof.back().b, s);
}
int prof_collect(std::map<std::string, ProfAgg>* out) {
    SD_HIP_CHECK(hipDeviceSynchronize());
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto& r : g_prof) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            ProfAgg& a = (*out)[r.name];
            a.flops += r.flops; a.bytes += r.bytes; a.ms += ms; a.launches += 1;
        }
        (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b);
    }
    g_prof.clear();
    return 0;
}

void ctx_gnpool_init(Ctx& c, int N, long HW_max, int G) {
    static const bool off = getenv("SD_NO_GN_EPILOGUE") != nullptr;    // A/B switch: GroupNorm runs its own statistics pass
    c.gn_groups = G;
    c.gn_next = 0;
    for (int i = 0; i < Ctx::kGnPool; ++i) {
        c.gnpool[i].buf = off ? nullptr : c.arena->alloc_f(gnstat_floats(N, HW_max, G));
        c.gnpool[i].st = GnStats();
    }
}

GnStatBuf* ctx_gnbuf(Ctx& c) {
    if (!c.gnpool[0].buf) return nullptr;
    GnStatBuf* b = &c.gnpool[c.gn_next];
    c.gn_next = (c.gn_next + 1) % Ctx::kGnPool;
    b->st = GnStats();
    return b;
}

// ------------------------------------------------------------------------------------- debug taps
void TapSink::clear() {
    if (entries.empty()) return;
    (void)hipDeviceSynchronize();           // copies into the buffers may still be in flight
    for (TapEntry& e : entries)
        if (e.dev) (void)hipFree(e.dev);
    entries.clear();
}

static void tap_copy(Ctx& c, TapEntry e, const void* src) {
    hipError_t err = hipMalloc(&e.dev, e.bytes);
    if (err == hipSuccess) {
        c.tap->entries.push_back(e);        // (owned by the sink from here on)
        err = hipMemcpyAsync(e.dev, src, e.bytes, hipMemcpyDeviceToDevice, c.stream);
    }
    if (err != hipSuccess) { set_error(std::string("tap ") + e.name + ": " + hipGetErrorString(err)); c.err = 3; }
}

void ctx_tap(Ctx& c, const std::string& name, int kind, View v, int N, int H, int W) {
    if (!c.tap || c.dry || c.err) return;
    if (!v.p || v.c0 < 0 || v.c0 + v.C > v.ld) { set_error("tap " + name + ": view does not lie inside its row"); c.err = 1; return; }
    TapEntry e;
    e.name = name; e.kind = kind;
    e.N = N; e.H = H; e.W = W; e.C = v.C; e.ld = v.ld;
    // a full-width view is one block; a narrower one is copied with its rows, from the row start
    e.c0 = v.C == v.ld ? 0 : v.c0;
    e.bytes = (size_t)N * H * W * v.ld * sizeof(half_t);
    tap_copy(c, e, v.p - e.c0);
}

void ctx_tap_f32(Ctx& c, const std::string& name, const float* p, int rows, int cols) {
    if (!c.tap || c.dry || c.err) return;
    TapEntry e;
    e.name = name; e.kind = kTapOut; e.f32 = 1;
    e.N = rows; e.H = 1; e.W = 1; e.C = cols; e.ld = cols;
    e.bytes = (size_t)rows * cols * sizeof(float);
    tap_copy(c, e, p);
}

// -------------------------------------------------------------------------------------------- ops
// The profiler row of a convolution launch: its name and the FLOPs / bytes it is charged.  cin = the channels the weights
// really have (p.Cin is the padded K of a pointwise launch).  SD_PROF_SHAPES=1 (tools/profile_layers.py): one row per
// (kernel or tile variant, split-K, problem shape, fused extras) instead of one per kernel instantiation.
struct ConvProfRow { char name[64]; double flops, bytes; };
static ConvProfRow conv_prof_row(const IGemmPlan& plan, const IGemmParams& p, int cin) {
    static const bool by_shape = getenv("SD_PROF_SHAPES") != nullptr;
    ConvProfRow r;
    const bool fold = plan.kind == kKindUpconvFold;
    if (!by_shape || plan.kind == kKindIgemm1) {
        snprintf(r.name, sizeof(r.name), "%s", plan.name);
    } else {
        char kernel[24];
        if (fold) snprintf(kernel, sizeof(kernel), "up2x2<%d>", plan.bn);
        else if (plan.kind == kKindHalo80) snprintf(kernel, sizeof(kernel), "h80/k%d", plan.splits);
        else snprintf(kernel, sizeof(kernel), "%s%d/k%d", plan.kind == kKindPgemmGeglu ? "pg" : "v", plan.variant, plan.splits);
        snprintf(r.name, sizeof(r.name), "%s %dx%dx%d ks%d%s%s%s%s%s%s", kernel, p.M, p.Cout, p.K, p.KS, p.res ? " res" : "",
                 p.geglu ? " geglu" : "", p.ln_stat ? " ln" : "", p.rowstat_out ? " rs" : "", p.gnstat_out ? " gs" : "",
                 p.gni_part ? " gn" : "");
    }
    // the FLOPs executed: the folded upsample (KS = 2) runs 4 taps, where the 9-tap form of the same launch counts 9/4 of
    // them, and reads four parity panels of K = 4 Cin weights per row
    const double weights = (fold ? 4.0 : 1.0) * p.Cout * p.K;
    const double out_cols = p.geglu ? p.Cout / 2 : p.Cout;
    r.flops = 2.0 * p.M * p.Cout * (double)(p.KS * p.KS) * cin;
    r.bytes = 2.0 * ((double)p.N * p.H * p.W * p.Cin + weights + (double)p.M * out_cols * (p.res ? 2 : 1));
    return r;
}

bool conv_prepare(Ctx& c, const ConvW& w, View x, int N, int H, int W, View y, const ConvArgs& a, ConvLaunch* out) {
    IGemmParams& p = out->p;
    p = conv_problem(N, H, W, w.ks == 1 ? (int)w.K : w.cin, w.cout, w.ks, a.stride, a.up, a.pad);
    p.K = (int)w.K;         // (the pack's K)
    p.x = x.p; p.ldx = x.ld;
    p.w = w.w; p.bias = w.bias;
    p.rowadd = a.rowadd; p.rowadd_ld = a.rowadd_ld;
    p.res = a.res.p; p.ldres = a.res.p ? a.res.ld : 0;
    p.y = y.p; p.ldy = y.ld;
    p.geglu = a.geglu;
    p.act = a.act;
    if (a.ln_in) {
        if (!w.wsum) { set_error("op_conv: LayerNorm statistics passed to a linear without folded weights"); c.err = 1; return false; }
        p.ln_stat = a.ln_in->p; p.ln_parts = a.ln_in->parts; p.ln_part_w = a.ln_in->width; p.ln_C = (int)w.K; p.ln_eps = a.ln_eps; p.ln_wsum = w.wsum;
    }
    if (a.gn_in) {
        p.gni_part = a.gn_in_stats.part; p.gni_S = a.gn_in_stats.S; p.gni_rows = a.gn_in_stats.rows;
        p.gni_groups = a.gn_in_groups; p.gni_eps = a.gn_in_eps; p.gni_silu = a.gn_in_silu;
        p.gni_gb = a.gn_in->gb;
        if (c.dry) p.gni_part = reinterpret_cast<const float*>(8);      // planning pass: only "is set" matters (tile choice)
    }
    if (a.acc_scale != 1.f || a.bias_scale != 1.f) { p.acc_scale = a.acc_scale; p.bias_scale = a.bias_scale; }
    // one plan per launch, the same in the planning and the live pass: the kernel (folded upsample, 80-column halo tile or
    // a row of the table), what it leaves of the requested statistics, the workspace, the name
    IGemmRequest rq{a.stat_out ? a.stat_out->p : nullptr, a.gn_out ? a.gn_out->buf : nullptr, a.gn_groups};
    rq.hint_variant = a.tile_variant; rq.hint_splits = a.tile_splits;
    const IGemmPlan& plan = out->plan = conv_plan(p, a.up == 1 ? w.w_up : nullptr, rq);
    const bool v2 = plan.kind != kKindIgemm1;
    if ((p.acc_scale != 1.f || p.bias_scale != 1.f) && !plan.scales_ok) { set_error("op_conv: output scaling needs the LDS-DMA kernels (not GEGLU / weight-stationary)"); c.err = 1; return false; }
    if (a.ln_in && !v2) { set_error("op_conv: the LayerNorm fold needs the LDS-DMA kernel"); c.err = 1; return false; }
    if (a.act && !v2) { set_error("op_conv: activation epilogue needs the LDS-DMA kernel (Cin % 64, Cout % 8)"); c.err = 1; return false; }
    if (a.gn_out) {
        a.gn_out->st = GnStats();
        if (plan.gnstats) { a.gn_out->st.part = a.gn_out->buf; a.gn_out->st.rows = plan.gn_rows; a.gn_out->st.S = p.OH * p.OW / plan.gn_rows; }
    }
    if (a.stat_out) { a.stat_out->parts = plan.rs_parts; a.stat_out->width = plan.rs_part_w; }
    out->stats_after = a.stat_out && !plan.rowstats;      // (otherwise the GEMM's epilogue writes the row statistics itself)
    out->partial = plan.partial_floats > 0 ? c.arena->alloc_f(plan.partial_floats) : nullptr;
    out->cin = w.cin;
    return !(c.dry || c.err);
}

void conv_launch(Ctx& c, const ConvLaunch& l, View y, RowStat* stat_out) {
    const IGemmParams& p = l.p;
    if (prof_enabled()) {
        const ConvProfRow row = conv_prof_row(l.plan, p, l.cin);
        prof_open(c.stream, row.name, row.flops, row.bytes);
    }
    c.err = launch_igemm2(p, l.partial, c.stream, &l.plan);
    prof_close(c.stream);
    if (l.stats_after && !c.err) {
        prof_open(c.stream, "row_stats_kernel", 0.0, 2.0 * p.M * p.Cout);
        c.err = launch_row_stats(y.p, y.ld, stat_out->p, p.M, p.Cout, c.stream);
        prof_close(c.stream);
    }
}

void op_conv(Ctx& c, const ConvW& w, View x, int N, int H, int W, View y, const ConvArgs& a) {
    ConvLaunch l;
    if (conv_prepare(c, w, x, N, H, W, y, a, &l)) conv_launch(c, l, y, a.stat_out);
}

void op_groupnorm(Ctx& c, const NormW& n, View x, View y, int N, long HW, int G, float eps, int silu,
                  const GnStatBuf* pre) {
    float* scratch = c.arena->alloc_f(gn_scratch_floats(N, HW, n.C, G));
    if (c.dry || c.err) return;
    const GnStats* st = (pre && pre->st.part && gn_wants_stats(HW, n.C, G)) ? &pre->st : nullptr;
    // bytes really moved: the single-kernel form and the apply pass read x and write y; only the
    // stand-alone statistics pass reads x once more
    const bool own_pass = gn_wants_stats(HW, n.C, G) && !st;
    const char* gname = own_pass ? "groupnorm(stats+apply)" : "groupnorm(apply)";
    static thread_local char gbuf[64];
    static const bool gn_by_shape = getenv("SD_PROF_SHAPES") != nullptr;
    if (gn_by_shape && prof_enabled()) {
        snprintf(gbuf, sizeof(gbuf), "gn%s %ldx%d%s", own_pass ? "(stats+apply)" : (st ? "(apply)" : "(fused)"), (long)N * HW, n.C, silu ? " silu" : "");
        gname = gbuf;
    }
    prof_open(c.stream, gname, 0.0, (own_pass ? 6.0 : 4.0) * N * HW * n.C);
    c.err = launch_groupnorm(x.p, x.ld, n.gamma, n.beta, y.p, y.ld, N, HW, n.C, G, eps, silu, scratch, c.stream, st);
    prof_close(c.stream);
}

// the convolution behind a GroupNorm: stride 1, no upsample, default padding, no GEGLU, no activation, whatever `a` says
static ConvArgs gn_conv_args(ConvArgs a) { a.stride = 1; a.up = 0; a.pad = -1; a.geglu = 0; a.act = 0; return a; }

void op_gn_conv(Ctx& c, const NormW& n, const ConvW& w, View x, int N, int H, int W, View y, int G, float eps, int silu,
                const GnStatBuf* pre, const ConvArgs& a) {
    // Off unless SD_GN_FUSE=1: measured slower than GroupNorm kernel + convolution on every UNet shape (the in-LDS
    // transform does not hide behind the MFMAs, profiles/r03_gn_fused_conv.txt); the kernel stays for the operator
    // test (sd_op_groupnorm_conv2d) and as the base of the next attempt.
    static const bool on = getenv("SD_GN_FUSE") != nullptr;
    if (on && op_gn_conv_fused(c, n, w, x, N, H, W, y, G, eps, silu, pre, a)) return;
    const size_t mk = c.arena->mark();
    View hn(c.arena->alloc_h((long)N * H * W * n.C), n.C, n.C);
    op_groupnorm(c, n, x, hn, N, (long)H * W, G, eps, silu, pre);
    op_conv(c, w, hn, N, H, W, y, gn_conv_args(a));
    c.arena->release(mk);
}

bool op_gn_conv_fused(Ctx& c, const NormW& n, const ConvW& w, View x, int N, int H, int W, View y, int G, float eps,
                      int silu, const GnStatBuf* pre, const ConvArgs& a, ConvLaunch* prepared) {
    static const bool off = getenv("SD_NO_GN_FUSE") != nullptr;         // kill switch
    const long HW = (long)H * W;
    // the problem as conv_prepare will pose it (stride 1, no upsample: the only form that follows a GroupNorm)
    IGemmParams q = conv_problem(N, H, W, w.ks == 1 ? (int)w.K : w.cin, w.cout, w.ks, 1, 0, -1);
    q.K = (int)w.K;
    q.x = x.p; q.ldx = x.ld;
    if (off || !n.gb || n.C != q.Cin || !igemm2_gn_fusable(q, G)) return false;
    const size_t mk = c.arena->mark();
    ConvArgs f = gn_conv_args(a);
    f.gn_in = &n; f.gn_in_groups = G; f.gn_in_eps = eps; f.gn_in_silu = silu;
    const long stat_floats = gn_scratch_floats(N, HW, n.C, G);
    float* scratch = c.arena->alloc_f(stat_floats + (long)N * G * 2);   // the statistics pass's summaries | the merged ones
    const bool go = !c.dry && !c.err;
    if (pre && pre->st.part) {
        f.gn_in_stats = pre->st;
    } else if (go) {
        static thread_local char gbuf[64];
        static const bool by_shape = getenv("SD_PROF_SHAPES") != nullptr;
        const char* name = "groupnorm(stats)";
        if (by_shape && prof_enabled()) { snprintf(gbuf, sizeof(gbuf), "gn(stats) %ldx%d", (long)N * HW, n.C); name = gbuf; }
        prof_open(c.stream, name, 0.0, 2.0 * N * HW * n.C);
        c.err = launch_gn_stats(x.p, x.ld, N, HW, n.C, G, scratch, &f.gn_in_stats, c.stream);
        prof_close(c.stream);
    }
    // many summaries per image (the VAE's 512 x 512 maps): merged once by a small kernel, not by every block's prologue
    if (f.gn_in_stats.S > 64 && go && !c.err) {
        prof_open(c.stream, "gn_finalize_kernel", 0.0, 8.0 * N * f.gn_in_stats.S * G);
        c.err = launch_gn_finalize(&f.gn_in_stats, scratch + stat_floats, N, HW, n.C, G, c.stream);
        prof_close(c.stream);
    }
    if (prepared) {
        conv_prepare(c, w, x, N, H, W, y, f, prepared);
        return true;
    }
    op_conv(c, w, x, N, H, W, y, f);
    c.arena->release(mk);
    return true;
}

bool op_ffn_fused(Ctx& c, const ConvW& ff1, const ConvW& ff2, View x, const RowStat& x_stat, float ln_eps, long M, View y) {
    FfnParams p;
    p.x = x.p; p.ldx = x.ld; p.y = y.p; p.ldy = y.ld;
    p.w1 = ff1.w; p.b1 = ff1.bias; p.wsum1 = ff1.wsum;
    p.w1_rows = (int)weight_rows(ff1.cout);
    p.w2 = ff2.w; p.b2 = ff2.bias;
    p.w2_rows = (int)weight_rows(ff2.cout);
    p.ln_stat = x_stat.p; p.ln_parts = x_stat.parts; p.ln_part_w = x_stat.width; p.ln_eps = ln_eps;
    p.M = (int)M; p.C = (int)ff1.K; p.hidden = (int)ff2.K;
    if (c.dry) p.ln_stat = reinterpret_cast<const float*>(8);          // planning pass: only "is set" matters
    if (ff1.ks != 1 || ff2.ks != 1 || ff2.cout != ff1.K || ff1.cout != 2 * ff2.K || x.C != p.C || !ff1.wsum) return false;
    if (!ffn_fused_supported(p)) return false;   // the one predicate of both passes: everything it reads is known when planning
    if (c.dry || c.err) return true;
    prof_open(c.stream, "ffn_fused_kernel", 2.0 * M * ((double)ff1.cout * ff1.K + (double)ff2.cout * ff2.K),
              2.0 * ((double)M * p.C * 2 + (double)ff1.cout * ff1.K + (double)ff2.cout * ff2.K));
    c.err = launch_ffn_fused(p, c.stream);
    prof_close(c.stream);
    return true;
}

void op_layernorm(Ctx& c, const NormW& n, View x, View y, long rows, float eps) {
    if (c.dry || c.err) return;
    prof_open(c.stream, "layernorm_kernel", 0.0, 4.0 * rows * n.C);
    c.err = launch_layernorm(x.p, x.ld, n.gamma, n.beta, y.p, y.ld, rows, n.C, eps, c.stream);
    prof_close(c.stream);
}

void op_attention(Ctx& c, View q, View k, View v, View out, int B, int Tq, int Tk, int heads, int d, int causal,
                  int prescaled) {
    if (c.dry || c.err) return;
    if (prof_enabled()) {
        static thread_local char name[32];
        snprintf(name, sizeof(name), "attn_kernel<%d>", d);
        prof_open(c.stream, name, 4.0 * B * heads * (double)Tq * Tk * d,
                  2.0 * B * heads * d * (2.0 * Tq + 2.0 * Tk));
    }
    c.err = launch_attention(q.p, k.p, v.p, out.p, B, Tq, Tk, heads, d, q.ld, k.ld, v.ld, out.ld, c.stream, causal, prescaled);
    prof_close(c.stream);
}

void op_ip_attention(Ctx& c, View q, View k, View v, View k_ip, View v_ip, View out, int B, int Tq, int L, int T_ip,
                     int heads, int d, float ip_scale) {
    if (c.dry || c.err) return;
    if (prof_enabled()) {
        static thread_local char name[32];
        snprintf(name, sizeof(name), "ip_xattn_kernel<%d>", d);
        prof_open(c.stream, name, 4.0 * B * heads * (double)Tq * (L + T_ip) * d,
                  2.0 * B * heads * d * (2.0 * Tq + 2.0 * L + 2.0 * T_ip));
    }
    c.err = launch_ip_attention(q.p, k.p, v.p, k_ip.p, v_ip.p, out.p, B, Tq, L, T_ip, heads, d, q.ld, k.ld, v.ld, k_ip.ld,
                                v_ip.ld, out.ld, ip_scale, 1, c.stream);
    prof_close(c.stream);
}

void op_region_attention(Ctx& c, View q, View k, View v, const float* w, View out, int B, int Tq, int L, int R, int heads,
                         int d, int Bw) {
    if (c.dry || c.err) return;
    if (prof_enabled()) {
        static thread_local char name[32];
        snprintf(name, sizeof(name), "region_xattn_kernel<%d>", d);
        prof_open(c.stream, name, 4.0 * B * heads * (double)Tq * R * L * d,
                  2.0 * B * heads * d * (2.0 * Tq + 2.0 * R * L) + 4.0 * B * (double)Tq * R);
    }
    c.err = launch_region_attention(q.p, k.p, v.p, w, out.p, B, Tq, L, R, heads, d, q.ld, k.ld, v.ld, out.ld, Bw, 1, c.stream);
    prof_close(c.stream);
}

void op_resampler_attention(Ctx& c, View q, View kx, View vx, View kl, View vl, View out, int B, int n_q, int T_feat,
                            int heads) {
    if (c.dry || c.err) return;
    prof_open(c.stream, "resampler_attn_kernel", 4.0 * B * heads * (double)n_q * (T_feat + n_q) * 64,
              2.0 * B * heads * 64 * (2.0 * n_q + 2.0 * (T_feat + n_q)));
    c.err = launch_resampler_attention(q.p, kx.p, vx.p, kl.p, vl.p, out.p, B, n_q, T_feat, heads, q.ld, kx.ld, vx.ld, kl.ld,
                                       vl.ld, out.ld, 1, c.stream);
    prof_close(c.stream);
}

}  // namespace sd
