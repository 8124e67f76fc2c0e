// lumo_denoise and lumo_denoise_temporal: the entry points of the denoiser (device/denoise.h,
// DESIGN.md §4d; device/denoise_temporal.h, §4e).  A call uploads a frame's beauty film and feature
// planes, runs prepare, (the firefly clamp when the context has it set: device/denoise_firefly.h,
// §4f,) (the reprojection of the context's history,) the variance estimate, the a-trous iterations
// and finish on the context's main stream, and reads the result back.  Neither needs a scene or
// touches the stats or the schedule record.
#include <hip/hip_runtime.h>

#include <cmath>

#include "ctx.h"
#include "denoise.h"
#include "denoise_firefly.h"
#include "denoise_temporal.h"

using namespace lumo;
using namespace lumo::dev;

namespace {

// Device buffers of a call (Ctx::dn_work), grown on demand and kept for the next call.
// DN_FF_CNT, the firefly clamp's counter, exists only on a context that has the clamp set; DN_IN_MOT
// and DN_MOT (the motion plane and k_dn_motion's m) only where lumo_denoise_temporal_motion got a plane.
enum DnBuf { DN_IN_RGB, DN_IN_ALB, DN_IN_NRM, DN_IN_DEP, DN_IN_ADD, DN_PLANES, DN_HIT, DN_OUT, DN_FF_CNT, DN_IN_MOT, DN_MOT,
             DN_BUF_COUNT };
constexpr int DN_NPLANES = 3 + 1 + 1 + 3 + 1 + 2 * 3 + 2;  // the doubles of DnPlanes per pixel

bool fcfg_valid(const lumo_firefly_cfg& f) {
    for (double v : {f.gain, f.normal_cos_min, f.depth_rel_max})
        if (!std::isfinite(v)) return false;
    return f.radius >= 1 && f.radius <= DF_R && f.rank >= 1 && f.rank <= DF_TOP && f.min_alike >= f.rank &&
           f.min_alike <= (2 * DF_R + 1) * (2 * DF_R + 1) - 1 && f.reserved == 0 && f.gain >= 1.0 && f.gain <= 1e6 &&
           f.normal_cos_min >= -1.0 && f.normal_cos_min <= 1.0 && f.depth_rel_max >= 0.0 && f.depth_rel_max <= 1e6;
}

bool cfg_valid(const lumo_denoise_cfg& g) {
    for (double v : {g.sigma_l, g.sigma_z, g.albedo_floor, g.depth_floor, g.lum_floor})
        if (!std::isfinite(v)) return false;
    return g.iterations >= 1 && g.iterations <= DN_MAX_ITER && g.normal_log2_power >= 0 && g.normal_log2_power <= 10 &&
           g.variance_radius >= 1 && g.variance_radius <= DN_VAR_R && (g.demodulate == 0 || g.demodulate == 1);
}

// Events around the stages of a call when the caller asked for their times.
struct DnClock {
    hipStream_t sm;
    bool on;
    hipEvent_t ev[DN_MAX_ITER + 9] = {};  // lumo_denoise_temporal marks N + 9 times
    int n = 0;
    DnClock(hipStream_t s, bool enable) : sm(s), on(enable) {}
    void mark() {
        if (!on) return;
        (void)hipEventCreate(&ev[n]);
        (void)hipEventRecord(ev[n++], sm);
    }
    void read(double* ms) const {  // after the stream is idle: n - 1 intervals
        for (int i = 0; on && i + 1 < n; ++i) {
            float t = 0.0f;
            (void)hipEventElapsedTime(&t, ev[i], ev[i + 1]);
            ms[i] = (double)t;
        }
    }
    ~DnClock() {
        for (int i = 0; i < n; ++i) (void)hipEventDestroy(ev[i]);
    }
};

// What the two entry points share: the checked arguments, the work buffers and the launches.
struct DnCall {
    Ctx* c;
    const lumo_denoise_in* in;
    lumo_denoise_cfg g;
    DnCfg dc;
    DnPlanes P;
    int W, H;
    size_t n;
    size_t bytes[DN_BUF_COUNT];
    unsigned pix_blocks;
    hipStream_t sm;
    hipEvent_t ff_ev[2] = {};  // around the firefly clamp, when the context has it set
    const double* motion_w = nullptr;  // lumo_denoise_temporal_motion's plane (set before alloc)

    ~DnCall() {
        for (hipEvent_t e : ff_ev)
            if (e) (void)hipEventDestroy(e);
    }
    double* buf(int k) const { return static_cast<double*>(c->dn_work[k].p); }

    lumo_status open(void* ctx, const lumo_denoise_in* in_, const lumo_denoise_cfg* cfg, const double* rgb_out) {
        c = static_cast<Ctx*>(ctx), in = in_;
        if (!c || !in || !rgb_out || !in->rgb_w || !in->albedo_w || !in->normal_w || !in->depth_w) return LUMO_ERR_INVALID;
        if (in->width < 1 || in->height < 1 || in->width > (1 << 20) || in->height > (1 << 20)) return LUMO_ERR_INVALID;
        g = {5, 7, 3, 1, 4.0, 1.0, 1e-3, 1e-3, 1e-8, nullptr};
        if (cfg) g = *cfg;
        if (!cfg_valid(g)) return LUMO_ERR_INVALID;
        W = (int)in->width, H = (int)in->height;
        n = (size_t)W * H;
        dc = DnCfg{g.sigma_l, g.sigma_z, g.albedo_floor, g.depth_floor, g.lum_floor, g.normal_log2_power, g.demodulate};
        pix_blocks = (unsigned)((n + 255) / 256);
        sm = c->streams[0];
        c->dn_ff_info = lumo_firefly_info{0, 0.0};  // until this call has run the step
        return LUMO_OK;
    }
    lumo_status alloc() {
        if (c->dn_work.size() < DN_BUF_COUNT) c->dn_work.resize(DN_BUF_COUNT);
        const size_t b[DN_BUF_COUNT] = {32 * n, 32 * n, 32 * n, 32 * n, in->add_rgb ? 24 * n : 0,
                                        sizeof(double) * DN_NPLANES * n, sizeof(uint32_t) * n, 24 * n,
                                        c->dn_ff_on ? sizeof(unsigned long long) : 0, motion_w ? 32 * n : 0,
                                        motion_w ? 24 * n : 0};
        for (int k = 0; k < DN_BUF_COUNT; ++k) {
            bytes[k] = b[k];
            if (k >= DN_FF_CNT && !b[k]) continue;
            const lumo_status st = dev_alloc(*c, c->dn_work[k], bytes[k]);
            if (st) return st;
        }
        double* p = buf(DN_PLANES);
        auto take = [&]() { double* q = p; p += n; return q; };
        for (int k = 0; k < 3; ++k) P.n[k] = take();
        P.z = take(), P.fz = take();
        for (int k = 0; k < 3; ++k) P.div[k] = take();
        P.l = take();
        for (int set = 0; set < 2; ++set) {
            for (int k = 0; k < 3; ++k) P.e[set][k] = take();
            P.var[set] = take();
        }
        P.hit = static_cast<uint32_t*>(c->dn_work[DN_HIT].p);
        return LUMO_OK;
    }
    lumo_status upload() const {
        const double* host[5] = {in->rgb_w, in->albedo_w, in->normal_w, in->depth_w, in->add_rgb};
        for (int k = 0; k < 5; ++k)
            if (host[k]) HIPCHK(hipMemcpyAsync(buf(DN_IN_RGB + k), host[k], bytes[DN_IN_RGB + k], hipMemcpyHostToDevice, sm));
        if (motion_w) HIPCHK(hipMemcpyAsync(buf(DN_IN_MOT), motion_w, bytes[DN_IN_MOT], hipMemcpyHostToDevice, sm));
        return LUMO_OK;
    }
    void prepare() const {
        k_dn_prepare<<<pix_blocks, 256, 0, sm>>>(buf(DN_IN_RGB), buf(DN_IN_ALB), buf(DN_IN_NRM), buf(DN_IN_DEP),
                                                 in->add_rgb ? buf(DN_IN_ADD) : nullptr, P, dc, W, H);
    }
    // Step 1b, after prepare and before anything reads its e or l.  The factor plane is var[1], which
    // nothing holds until the first a-trous iteration writes it.  Off: nothing is launched.
    lumo_status firefly() {
        if (!c->dn_ff_on) return LUMO_OK;
        const lumo_firefly_cfg& f = c->dn_ff;
        const DfCfg fc{f.gain, f.normal_cos_min, f.depth_rel_max, f.radius, f.rank, f.min_alike};
        unsigned long long* cnt = static_cast<unsigned long long*>(c->dn_work[DN_FF_CNT].p);
        for (hipEvent_t& e : ff_ev) HIPCHK(hipEventCreate(&e));
        HIPCHK(hipEventRecord(ff_ev[0], sm));
        HIPCHK(hipMemsetAsync(cnt, 0, sizeof(unsigned long long), sm));
        k_dn_firefly<<<march_grid(1), DN_BW, DnMarch<DF_R>::lds_bytes(1, DF_NV), sm>>>(P, fc, P.var[1], cnt, W, H);
        k_dn_firefly_apply<<<pix_blocks, 256, 0, sm>>>(buf(DN_IN_RGB), in->add_rgb ? buf(DN_IN_ADD) : nullptr, P, P.var[1], n);
        HIPCHK(hipEventRecord(ff_ev[1], sm));
        return LUMO_OK;
    }
    // after the call's stream is idle: what the step did
    lumo_status firefly_read() const {
        if (!c->dn_ff_on) return LUMO_OK;
        unsigned long long count = 0;
        float ms = 0.0f;
        HIPCHK(hipMemcpy(&count, c->dn_work[DN_FF_CNT].p, sizeof(count), hipMemcpyDeviceToHost));
        HIPCHK(hipEventElapsedTime(&ms, ff_ev[0], ff_ev[1]));
        c->dn_ff_info = lumo_firefly_info{(int64_t)count, (double)ms};
        return LUMO_OK;
    }
    // the march kernels: x tiles of DN_BW centres; per residue class mod s, chunks of DN_ROWS rows
    dim3 march_grid(int s) const {
        const int chunks = ((H + s - 1) / s + DN_ROWS - 1) / DN_ROWS;
        return dim3((unsigned)((W + DN_BW - 1) / DN_BW), (unsigned)(s * chunks));
    }
    void variance() const {
        k_dn_variance<<<march_grid(1), DN_BW, DnMarch<DN_VAR_R>::lds_bytes(1, DN_VAR_NV), sm>>>(P, dc, g.variance_radius, W, H);
    }
    void atrous(int i, int from) const {
        const int s = 1 << i;
        k_dn_atrous<<<march_grid(s), DN_BW, DnMarch<DN_AT_R>::lds_bytes(s, DN_AT_NV), sm>>>(P, dc, from, s, W, H);
    }
    void finish(int set) const { k_dn_finish<<<pix_blocks, 256, 0, sm>>>(P, set, buf(DN_OUT), n); }
    lumo_status read_back(int set, double* rgb_out, double* variance_out) const {
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(rgb_out, buf(DN_OUT), 24 * n, hipMemcpyDeviceToHost, sm));
        if (variance_out) HIPCHK(hipMemcpyAsync(variance_out, P.var[set], sizeof(double) * n, hipMemcpyDeviceToHost, sm));
        return LUMO_OK;
    }
};

bool tcfg_valid(const lumo_temporal_cfg& t, int iterations) {
    for (double v : {t.alpha, t.normal_cos_min, t.depth_rel_max})
        if (!std::isfinite(v)) return false;
    return t.alpha >= 0.0 && t.alpha <= 1.0 && t.normal_cos_min >= -1.0 && t.normal_cos_min <= 1.0 &&
           t.depth_rel_max >= 0.0 && t.depth_rel_max <= 1e6 && t.max_history >= 1 && t.max_history <= 1024 &&
           t.min_history >= 1 && t.min_history <= 1025 && t.feedback >= 0 && t.feedback <= iterations &&
           (t.stage_lds == 0 || t.stage_lds == 1);
}

// The history planes of one set in its buffer: DT_NV doubles, then the length and the hit flag.
DtHist hist_planes(const DevBuf& b, size_t n) {
    DtHist h;
    double* p = static_cast<double*>(b.p);
    for (int k = 0; k < DT_NV; ++k) h.v[k] = p + (size_t)k * n;
    h.len = reinterpret_cast<uint32_t*>(p + (size_t)DT_NV * n);
    h.hit = h.len + n;
    return h;
}

DtCam cam_of(const lumo_camera_desc& d) {
    auto get = [](const double (&a)[2][16]) {  // as lumo_camera_set
        Xform x;
        M4* ms[2] = {&x.m, &x.inv};
        for (int q = 0; q < 2; ++q) {
            V4* rows[4] = {&ms[q]->y0, &ms[q]->y1, &ms[q]->y2, &ms[q]->y3};
            for (int r = 0; r < 4; ++r) *rows[r] = V4{a[q][4 * r], a[q][4 * r + 1], a[q][4 * r + 2], a[q][4 * r + 3]};
        }
        return x;
    };
    return DtCam{get(d.world_to_camera), get(d.screen_to_raster), get(d.camera_to_screen)};
}

}  // namespace

extern "C" lumo_status lumo_denoise(void* ctx, const lumo_denoise_in* in, const lumo_denoise_cfg* cfg, double* rgb_out,
                                    double* variance_out) {
    DnCall k;
    lumo_status st = k.open(ctx, in, cfg, rgb_out);
    if (st) return st;
    HIPCHK(hipSetDevice(k.c->device));
    if ((st = k.alloc())) return st;
    DnClock clk(k.sm, k.g.stage_ms != nullptr);

    clk.mark();
    if ((st = k.upload())) return st;
    clk.mark();
    k.prepare();
    if ((st = k.firefly())) return st;
    clk.mark();
    k.variance();
    clk.mark();
    int set = 0;
    for (int i = 0; i < k.g.iterations; ++i, set ^= 1) {
        k.atrous(i, set);
        clk.mark();
    }
    k.finish(set);
    clk.mark();
    if ((st = k.read_back(set, rgb_out, variance_out))) return st;
    clk.mark();
    HIPCHK(hipStreamSynchronize(k.sm));
    if ((st = k.firefly_read())) return st;
    if (k.g.stage_ms) clk.read(k.g.stage_ms);
    return LUMO_OK;
}

extern "C" lumo_status lumo_denoise_set_firefly(void* ctx, const lumo_firefly_cfg* cfg) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c || (cfg && !fcfg_valid(*cfg))) return LUMO_ERR_INVALID;
    c->dn_ff_on = cfg != nullptr;
    if (cfg) c->dn_ff = *cfg;
    return LUMO_OK;
}

extern "C" lumo_status lumo_denoise_firefly_info(void* ctx, lumo_firefly_info* info) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c || !info) return LUMO_ERR_INVALID;
    *info = c->dn_ff_info;
    return LUMO_OK;
}

extern "C" lumo_status lumo_denoise_reset(void* ctx) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c) return LUMO_ERR_INVALID;
    c->dn_hist_w = c->dn_hist_h = 0;
    return LUMO_OK;
}

extern "C" lumo_status lumo_denoise_temporal(void* ctx, const lumo_denoise_in* in, const lumo_camera_desc* camera,
                                             const lumo_denoise_cfg* cfg, const lumo_temporal_cfg* tcfg, double* rgb_out,
                                             double* variance_out, lumo_temporal_info* info) {
    return lumo_denoise_temporal_motion(ctx, in, nullptr, camera, cfg, tcfg, rgb_out, variance_out, info);
}

// motion_w == nullptr: lumo_denoise_temporal, launch for launch.
extern "C" lumo_status lumo_denoise_temporal_motion(void* ctx, const lumo_denoise_in* in, const double* motion_w,
                                                    const lumo_camera_desc* camera, const lumo_denoise_cfg* cfg,
                                                    const lumo_temporal_cfg* tcfg, double* rgb_out, double* variance_out,
                                                    lumo_temporal_info* info) {
    DnCall k;
    lumo_status st = k.open(ctx, in, cfg, rgb_out);
    if (st) return st;
    k.motion_w = motion_w;
    lumo_temporal_cfg t = {0.2, 0.9, 0.1, 32, 4, 1, 1};
    if (tcfg) t = *tcfg;
    if (!camera || camera->width != in->width || camera->height != in->height || !tcfg_valid(t, k.g.iterations))
        return LUMO_ERR_INVALID;
    if (camera->orthographic) return LUMO_ERR_UNSUPPORTED;
    Ctx* c = k.c;
    HIPCHK(hipSetDevice(c->device));
    const bool has_prev = c->dn_hist_w == in->width && c->dn_hist_h == in->height;
    c->dn_hist_w = c->dn_hist_h = 0;  // until this call has written its own: a failed call leaves none
    if ((st = k.alloc())) return st;
    const size_t n = k.n;
    for (DevBuf& b : c->dn_hist)
        if ((st = dev_alloc(*c, b, (sizeof(double) * DT_NV + 2 * sizeof(uint32_t)) * n))) return st;
    if ((st = dev_alloc(*c, c->dn_hist_cnt, sizeof(unsigned long long) * DT_CNT_N))) return st;
    const DtHist prev = hist_planes(c->dn_hist[c->dn_hist_set], n), next = hist_planes(c->dn_hist[c->dn_hist_set ^ 1], n);
    unsigned long long* cnt = static_cast<unsigned long long*>(c->dn_hist_cnt.p);
    const DtCfg tc{t.alpha, t.normal_cos_min, t.depth_rel_max, t.max_history, t.min_history, t.stage_lds, has_prev ? 1 : 0};
    DnClock clk(k.sm, info && info->stage_ms);

    clk.mark();
    if ((st = k.upload())) return st;
    HIPCHK(hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * DT_CNT_N, k.sm));
    clk.mark();
    k.prepare();
    if (motion_w) k_dn_motion<<<k.pix_blocks, 256, 0, k.sm>>>(k.buf(DN_IN_MOT), k.buf(DN_IN_DEP), k.buf(DN_MOT), n);
    if ((st = k.firefly())) return st;
    clk.mark();
    const unsigned tiles = (unsigned)((k.W + DT_BX - 1) / DT_BX) * (unsigned)((k.H + DT_BY - 1) / DT_BY);
    const DtCam cur = cam_of(*camera), prv = cam_of(has_prev ? c->dn_hist_cam : *camera);
    if (motion_w)
        k_dn_reproject<true><<<tiles, DT_THREADS, 0, k.sm>>>(k.P, prev, next, cur, prv, tc, cnt, k.W, k.H, k.buf(DN_MOT));
    else
        k_dn_reproject<false><<<tiles, DT_THREADS, 0, k.sm>>>(k.P, prev, next, cur, prv, tc, cnt, k.W, k.H, nullptr);
    clk.mark();
    k.variance();
    clk.mark();
    k_dn_tvar<<<k.pix_blocks, 256, 0, k.sm>>>(k.P, next, t.min_history, n);
    clk.mark();
    int set = 0;
    for (int i = 0; i <= k.g.iterations; ++i, set ^= 1) {
        if (i == t.feedback) {  // set holds e_acc (i = 0) or the output of iteration i - 1
            k_dn_history<<<k.pix_blocks, 256, 0, k.sm>>>(k.P, set, next, n);
            clk.mark();
        }
        if (i == k.g.iterations) break;
        k.atrous(i, set);
        clk.mark();
    }
    k.finish(set);
    clk.mark();
    if ((st = k.read_back(set, rgb_out, variance_out))) return st;
    clk.mark();
    unsigned long long counts[DT_CNT_N] = {};
    HIPCHK(hipMemcpyAsync(counts, cnt, sizeof(counts), hipMemcpyDeviceToHost, k.sm));
    HIPCHK(hipStreamSynchronize(k.sm));
    if ((st = k.firefly_read())) return st;
    if (info) {
        info->with_history = (int64_t)counts[DT_CNT_WITH];
        info->without_history = (int64_t)counts[DT_CNT_WITHOUT];
        info->blocks_staged = (int64_t)counts[DT_CNT_STAGED];
        info->blocks_direct = (int64_t)counts[DT_CNT_DIRECT];
        if (info->stage_ms) clk.read(info->stage_ms);
    }
    c->dn_hist_set ^= 1;
    c->dn_hist_w = in->width, c->dn_hist_h = in->height;
    c->dn_hist_cam = *camera;
    return LUMO_OK;
}
