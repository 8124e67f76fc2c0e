// lumo_denoise: the entry point of the denoiser (device/denoise.h).  It uploads a
// frame's beauty film and feature planes, runs prepare, the variance estimate, the a-trous
// iterations and finish on the context's main stream, and reads the result back.  It needs no
// scene or camera and touches neither the stats nor the schedule record.
#include <hip/hip_runtime.h>

#include <cmath>

#include "ctx.h"
#include "denoise.h"

using namespace lumo;
using namespace lumo::dev;

namespace {

// Device buffers of a call (Ctx::dn_work), grown on demand and kept for the next call.
enum DnBuf { DN_IN_RGB, DN_IN_ALB, DN_IN_NRM, DN_IN_DEP, DN_IN_ADD, DN_PLANES, DN_HIT, DN_OUT, DN_BUF_COUNT };
constexpr int DN_NPLANES = 3 + 1 + 1 + 3 + 1 + 2 * 3 + 2;  // the doubles of DnPlanes per pixel

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
    hipEvent_t ev[DN_MAX_ITER + 6] = {};
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

}  // namespace

extern "C" lumo_status lumo_denoise(void* ctx, const lumo_denoise_in* in, const lumo_denoise_cfg* cfg, double* rgb_out,
                                    double* variance_out) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c || !in || !rgb_out || !in->rgb_w || !in->albedo_w || !in->normal_w || !in->depth_w) return LUMO_ERR_INVALID;
    if (in->width < 1 || in->height < 1 || in->width > (1 << 20) || in->height > (1 << 20)) return LUMO_ERR_INVALID;
    lumo_denoise_cfg g = {5, 7, 3, 1, 4.0, 1.0, 1e-3, 1e-3, 1e-8, nullptr};
    if (cfg) g = *cfg;
    if (!cfg_valid(g)) return LUMO_ERR_INVALID;
    HIPCHK(hipSetDevice(c->device));
    const int W = (int)in->width, H = (int)in->height;
    const size_t n = (size_t)W * H;
    if (c->dn_work.size() < DN_BUF_COUNT) c->dn_work.resize(DN_BUF_COUNT);
    const size_t bytes[DN_BUF_COUNT] = {32 * n, 32 * n, 32 * n, 32 * n, in->add_rgb ? 24 * n : 0,
                                        sizeof(double) * DN_NPLANES * n, sizeof(uint32_t) * n, 24 * n};
    for (int k = 0; k < DN_BUF_COUNT; ++k) {
        const lumo_status st = dev_alloc(*c, c->dn_work[k], bytes[k]);
        if (st) return st;
    }
    auto buf = [&](int k) { return static_cast<double*>(c->dn_work[k].p); };
    DnPlanes P;
    {
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
    }
    const DnCfg dc{g.sigma_l, g.sigma_z, g.albedo_floor, g.depth_floor, g.lum_floor, g.normal_log2_power, g.demodulate};
    hipStream_t sm = c->streams[0];
    DnClock clk(sm, g.stage_ms != nullptr);

    clk.mark();
    const double* host[5] = {in->rgb_w, in->albedo_w, in->normal_w, in->depth_w, in->add_rgb};
    for (int k = 0; k < 5; ++k)
        if (host[k]) HIPCHK(hipMemcpyAsync(buf(DN_IN_RGB + k), host[k], bytes[DN_IN_RGB + k], hipMemcpyHostToDevice, sm));
    clk.mark();
    const unsigned pix_blocks = (unsigned)((n + 255) / 256);
    k_dn_prepare<<<pix_blocks, 256, 0, sm>>>(buf(DN_IN_RGB), buf(DN_IN_ALB), buf(DN_IN_NRM), buf(DN_IN_DEP),
                                             in->add_rgb ? buf(DN_IN_ADD) : nullptr, P, dc, W, H);
    clk.mark();
    // the march kernels: x tiles of DN_BW centres; per residue class mod s, chunks of DN_ROWS rows
    auto march_grid = [&](int s) {
        const int chunks = ((H + s - 1) / s + DN_ROWS - 1) / DN_ROWS;
        return dim3((unsigned)((W + DN_BW - 1) / DN_BW), (unsigned)(s * chunks));
    };
    k_dn_variance<<<march_grid(1), DN_BW, DnMarch<DN_VAR_R>::lds_bytes(1, DN_VAR_NV), sm>>>(P, dc, g.variance_radius, W, H);
    clk.mark();
    int set = 0;
    for (int i = 0; i < g.iterations; ++i, set ^= 1) {
        const int s = 1 << i;
        k_dn_atrous<<<march_grid(s), DN_BW, DnMarch<DN_AT_R>::lds_bytes(s, DN_AT_NV), sm>>>(P, dc, set, s, W, H);
        clk.mark();
    }
    k_dn_finish<<<pix_blocks, 256, 0, sm>>>(P, set, buf(DN_OUT), n);
    clk.mark();
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rgb_out, buf(DN_OUT), 24 * n, hipMemcpyDeviceToHost, sm));
    if (variance_out) HIPCHK(hipMemcpyAsync(variance_out, P.var[set], sizeof(double) * n, hipMemcpyDeviceToHost, sm));
    clk.mark();
    HIPCHK(hipStreamSynchronize(sm));
    if (g.stage_ms) clk.read(g.stage_ms);
    return LUMO_OK;
}
