// The context's life and its execution options (host code only: no kernel is defined or launched
// here): lumo_create / lumo_destroy, the option table behind lumo_set_option / lumo_get_option and
// the environment's overrides, the status strings.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <strings.h>
#include <unistd.h>  // environ
#include <new>

#include "ctx.h"
#include "launch.h"

namespace lumo {
namespace dev {

hipError_t& last_hip_error() {
    static thread_local hipError_t e = hipSuccess;
    return e;
}

lumo_status dev_alloc(const Ctx& c, DevBuf& b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.bytes >= bytes) return LUMO_OK;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
    if (hipMalloc(&b.p, bytes) != hipSuccess) return LUMO_ERR_OOM;
    b.bytes = bytes;
    if (c.o.poison) {  // debug: new buffers all ones (NaN, -1)
        // hipMemset runs on the null stream, which the context's non-blocking streams do not wait
        // for: finish it here, or it could land after the render's own initialisation
        (void)hipMemset(b.p, 0xFF, bytes);
        (void)hipStreamSynchronize(nullptr);
    }
    return LUMO_OK;
}

void free_scene(Ctx& c) {
    for (DevBuf& b : c.scene_bufs)
        if (b.p) (void)hipFree(b.p);
    c.scene_bufs.clear();
    c.has_scene = false;
}

}  // namespace dev
}  // namespace lumo

using namespace lumo;
using namespace lumo::dev;

namespace {

// ------------------------------------------------------------------ options (LUMO_OPT_*)
// One row per option, in the order of the LUMO_OPT_* enum: the environment variable that overrides
// its default at lumo_create, its field of Opts and its static range.  opt_range, set_opt, get_opt,
// the environment loop of lumo_create and warn_unknown_env all read this table.
struct OptDef {
    int id;  // LUMO_OPT_*: the row's index (checked below)
    const char* env;
    int64_t Opts::*field;
    int64_t lo, hi;
};
constexpr OptDef kOpts[] = {
    {LUMO_OPT_TIMING, "LUMO_TIMING", &Opts::timing, 0, 1},
    {LUMO_OPT_LDS_STAGING, "LUMO_LDS", &Opts::lds, 0, 1},
    {LUMO_OPT_TOP_STAGING, "LUMO_TOP", &Opts::top, 0, 1},
    {LUMO_OPT_FUSED, "LUMO_FUSED", &Opts::fused, -1, 1},
    {LUMO_OPT_TAIL_BELOW, "LUMO_TAIL", &Opts::tail_below, 0, (int64_t)1 << 31},
    {LUMO_OPT_PIPELINE, "LUMO_PIPELINE", &Opts::pipeline, 0, 3},
    {LUMO_OPT_HEADS, "LUMO_HEADS", &Opts::heads, 0, 64},
    {LUMO_OPT_MERGE_PASSES, "LUMO_MERGE", &Opts::merge, 0, MAX_MERGE},
    {LUMO_OPT_DYN_FETCH, "LUMO_DYN", &Opts::dyn, 0, 1},
    {LUMO_OPT_BOUNCE_THREADS, "LUMO_BOUNCE_THREADS", &Opts::bounce_threads, 64, BLOCK},  // 64, 128 or BLOCK (set_opt)
    {LUMO_OPT_SPLIT_PIPE, "LUMO_SPLIT_PIPE", &Opts::split_pipe, 1, 4},
    {LUMO_OPT_SPLIT_GROUPS, "LUMO_SPLIT_GROUPS", &Opts::split_groups, 1, 4},
    {LUMO_OPT_BDPT_TAIL, "LUMO_BDPT_TAIL", &Opts::bdpt_tail, 0, (int64_t)1 << 31},
    {LUMO_OPT_BOUNCE_AHEAD, "LUMO_BOUNCE_AHEAD", &Opts::bounce_ahead, 1, Ctx::SNAP_RING / 4 - 1},
    {LUMO_OPT_LDS_GRID, "LUMO_LDS_GRID", &Opts::lds_grid, 1, 1 << 20},
    {LUMO_OPT_TOP_GRID, "LUMO_TOP_GRID", &Opts::top_grid, 1, 1 << 20},
    {LUMO_OPT_TOP_KB, "LUMO_TOP_KB", &Opts::top_kb, 0, 160},  // hi: the device's LDS per CU (opt_range)
    {LUMO_OPT_KD_LDS, "LUMO_KD_LDS", &Opts::kd_lds, 0, 64},
    {LUMO_OPT_STACK_CLASS, "LUMO_STACK_CLASS", &Opts::stack_class, 0, 64},  // 0 or a STACK_CLASSES entry (set_opt)
    {LUMO_OPT_FULL_KERNELS, "LUMO_FULL_KERNELS", &Opts::full_kernels, 0, 1},
    {LUMO_OPT_POISON, "LUMO_POISON", &Opts::poison, 0, 1},
    {LUMO_OPT_TAIL_PRIORITY, "LUMO_TAIL_PRIORITY", &Opts::tail_priority, 0, 1},  // recreates the tail stream (set_opt)
    {LUMO_OPT_TOP_KD, "LUMO_TOP_KD", &Opts::top_kd, 0, 1},
    {LUMO_OPT_TAIL_BOUNCES, "LUMO_TAIL_BOUNCES", &Opts::tail_bounces, -1, 16},
    {LUMO_OPT_FILM_FIRST, "LUMO_FILM_FIRST", &Opts::film_first, 0, 1},
    {LUMO_OPT_BDPT_TOP, "LUMO_BDPT_TOP", &Opts::bdpt_top, 0, 1},
    {LUMO_OPT_BDPT_GROUPS, "LUMO_BDPT_GROUPS", &Opts::bdpt_groups, 1, 4},
    {LUMO_OPT_RAY_SORT, "LUMO_RAY_SORT", &Opts::ray_sort, -1, 2},
    {LUMO_OPT_ACCEL, "LUMO_ACCEL", &Opts::accel, 0, 1},
};
constexpr bool opts_in_enum_order() {
    for (int k = 0; k < LUMO_OPT_COUNT; ++k)
        if (kOpts[k].id != k) return false;
    return true;
}
static_assert(sizeof(kOpts) / sizeof(kOpts[0]) == LUMO_OPT_COUNT && opts_in_enum_order(),
              "kOpts: one row per LUMO_OPT_*, in the enum's order");

// A LUMO_* variable that names no option (e.g. a misspelt LUMO_TAIL_BELOW for LUMO_TAIL) would
// otherwise be ignored without a trace: warn once per process.  LUMO_AMD_LIB and
// LUMO_BENCH_BACKEND are read by the Python side.
void warn_unknown_env() {
    static bool done = false;
    if (done) return;
    done = true;
    for (char** ev = environ; ev && *ev; ++ev) {
        const char* kv = *ev;
        if (std::strncmp(kv, "LUMO_", 5) != 0) continue;
        const char* eq = std::strchr(kv, '=');
        const size_t n = eq ? (size_t)(eq - kv) : std::strlen(kv);
        auto same = [&](const char* name) { return std::strlen(name) == n && std::strncmp(name, kv, n) == 0; };
        bool known = same("LUMO_AMD_LIB") || same("LUMO_BENCH_BACKEND");
        for (const OptDef& d : kOpts) known = known || same(d.env);
        if (!known) fprintf(stderr, "lumo_amd: %.*s names no option; ignored\n", (int)n, kv);
    }
}

void opt_range(const Ctx& c, int k, int64_t& lo, int64_t& hi) {
    lo = kOpts[k].lo;
    hi = k == LUMO_OPT_TOP_KB ? (int64_t)(c.lds_cu / 1024) : kOpts[k].hi;
}

// The pipelined passes' tail stream (streams[1]), (re)created at normal or the device's highest
// priority: the workgroups of its kernels are then dispatched ahead of the head streams' as CUs
// free up.
lumo_status make_tail_stream(Ctx& c, int high) {
    (void)hipSetDevice(c.device);
    hipStream_t& tail = c.streams[1];
    if (tail) {
        (void)hipStreamSynchronize(tail);
        (void)hipStreamDestroy(tail);
        tail = nullptr;
    }
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) greatest = least = 0;
    if (hipStreamCreateWithPriority(&tail, hipStreamNonBlocking, high ? greatest : least) != hipSuccess) {
        last_hip_error() = hipErrorInvalidValue;
        return LUMO_ERR_HIP;
    }
    return LUMO_OK;
}

lumo_status set_opt(Ctx& c, int k, int64_t v) {
    if (k < 0 || k >= LUMO_OPT_COUNT) return LUMO_ERR_INVALID;
    int64_t lo, hi;
    opt_range(c, k, lo, hi);
    if (v < lo || v > hi) return LUMO_ERR_INVALID;
    if (k == LUMO_OPT_BOUNCE_THREADS && v != 64 && v != 128 && v != BLOCK) return LUMO_ERR_INVALID;
    if (k == LUMO_OPT_STACK_CLASS && v != 0 &&
        std::find(std::begin(STACK_CLASSES), std::end(STACK_CLASSES), (int)v) == std::end(STACK_CLASSES))
        return LUMO_ERR_INVALID;
    if (k == LUMO_OPT_TAIL_PRIORITY && v != c.o.tail_priority) {
        const lumo_status e = make_tail_stream(c, (int)v);
        if (e) return e;
    }
    c.o.*kOpts[k].field = v;
    return LUMO_OK;
}

int64_t get_opt(const Ctx& c, int k) { return c.o.*kOpts[k].field; }

}  // namespace

extern "C" {

int lumo_abi_version(void) { return LUMO_ABI_VERSION; }

int lumo_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* lumo_status_str(lumo_status st) {
    switch (st) {
        case LUMO_OK: return "ok";
        case LUMO_ERR_INVALID: return "invalid argument";
        case LUMO_ERR_NO_DEVICE: return "no gfx950 device";
        case LUMO_ERR_HIP: return hipGetErrorString(last_hip_error());
        case LUMO_ERR_NO_SCENE: return "no scene uploaded";
        case LUMO_ERR_NO_CAMERA: return "no camera set";
        case LUMO_ERR_UNSUPPORTED: return "unsupported";
        case LUMO_ERR_OOM: return "out of device memory";
        default: return "unknown";
    }
}

lumo_status lumo_create(int device, void** ctx_out) {
    if (!ctx_out) return LUMO_ERR_INVALID;
    *ctx_out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return LUMO_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return LUMO_ERR_NO_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return LUMO_ERR_NO_DEVICE;
    HIPCHK(hipSetDevice(device));
    Ctx* c = new (std::nothrow) Ctx();
    if (!c) return LUMO_ERR_OOM;
    c->device = device;
    // the per-device defaults: grids from the CU count, the TOP budget from the CU's LDS
    const int cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    c->o.top_grid = std::max(1, cus / 2);
    c->o.lds_grid = cus * 3 / 2;
    if (prop.maxSharedMemoryPerMultiProcessor > 0) c->lds_cu = prop.maxSharedMemoryPerMultiProcessor;
    if (prop.sharedMemPerBlock > 0) c->lds_block = std::min(c->lds_cu, (size_t)prop.sharedMemPerBlock);
    c->o.top_kb = (int64_t)(c->lds_cu / 1024);
    if (hipStreamCreateWithFlags(&c->streams[0], hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return LUMO_ERR_HIP;
    }
    if (make_tail_stream(*c, (int)c->o.tail_priority) != LUMO_OK ||
        hipStreamCreateWithFlags(&c->streams[2], hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->streams[3], hipStreamNonBlocking) != hipSuccess) {
        (void)hipStreamDestroy(c->streams[0]);
        delete c;
        return LUMO_ERR_HIP;
    }
    for (int i = 0; i < 4; ++i) {
        (void)hipEventCreateWithFlags(&c->pass_ev[i], hipEventDisableTiming);
        (void)hipEventCreateWithFlags(&c->tail_ev[i], hipEventDisableTiming);
        (void)hipEventCreateWithFlags(&c->cam_ev[i], hipEventDisableTiming);
        (void)hipEventCreateWithFlags(&c->film_ev[i], hipEventDisableTiming);
    }
    for (int i = 0; i < Ctx::SNAP_RING; ++i) (void)hipEventCreateWithFlags(&c->snap_ev[i], hipEventDisableTiming);
    for (int i = 0; i < 4; ++i) (void)hipEventCreateWithFlags(&c->bd_ev[i], hipEventDisableTiming);
    if (hipHostMalloc(reinterpret_cast<void**>(&c->bd_totals_h), sizeof(uint32_t) * 8) != hipSuccess) {
        (void)hipStreamDestroy(c->streams[0]);
        delete c;
        return LUMO_ERR_OOM;
    }
    if (hipHostMalloc(reinterpret_cast<void**>(&c->snap), sizeof(uint32_t) * CNT_N * Ctx::SNAP_RING) != hipSuccess) {
        (void)hipStreamDestroy(c->streams[0]);
        delete c;
        return LUMO_ERR_OOM;
    }
    // the environment's overrides of the defaults: integers; the 0 / 1 switches also take
    // on / off, true / false, yes / no.  A value that does not parse is ignored and an
    // out-of-range one clamped, each with a one-line warning on stderr
    for (int k = 0; k < LUMO_OPT_COUNT; ++k) {
        const char* name = kOpts[k].env;
        const char* e = std::getenv(name);
        if (!e || !*e) continue;
        int64_t lo = 0, hi = 0;
        opt_range(*c, k, lo, hi);
        char* end = nullptr;
        int64_t v = (int64_t)std::strtoll(e, &end, 10);
        if (end == e || *end != '\0') {
            auto is = [&](const char* w) { return strcasecmp(e, w) == 0; };
            const bool sw = lo == 0 && hi == 1;
            if (sw && (is("on") || is("true") || is("yes"))) {
                v = 1;
            } else if (sw && (is("off") || is("false") || is("no"))) {
                v = 0;
            } else {
                fprintf(stderr, "lumo_amd: %s=%s is not a number; ignored\n", name, e);
                continue;
            }
        }
        if (v < lo || v > hi) {
            const int64_t cl = std::min(hi, std::max(lo, v));
            fprintf(stderr, "lumo_amd: %s=%s outside [%lld, %lld]; using %lld\n", name, e, (long long)lo,
                    (long long)hi, (long long)cl);
            v = cl;
        }
        if (set_opt(*c, k, v) != LUMO_OK)
            fprintf(stderr, "lumo_amd: %s=%s not accepted; default kept\n", name, e);
    }
    warn_unknown_env();
    *ctx_out = c;
    return LUMO_OK;
}

void lumo_destroy(void* ctx) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (hipStream_t s : c->streams) (void)hipStreamSynchronize(s);
    free_scene(*c);
    for (DevBuf& b : c->work)
        if (b.p) (void)hipFree(b.p);
    for (DevBuf& b : c->gwork)
        if (b.p) (void)hipFree(b.p);
    for (int i = 0; i < Ctx::SNAP_RING; ++i) (void)hipEventDestroy(c->snap_ev[i]);
    if (c->snap) (void)hipHostFree(c->snap);
    if (c->bd_totals_h) (void)hipHostFree(c->bd_totals_h);
    for (int i = 0; i < 4; ++i) (void)hipEventDestroy(c->bd_ev[i]);
    for (int i = 0; i < 4; ++i) {
        (void)hipEventDestroy(c->pass_ev[i]);
        (void)hipEventDestroy(c->tail_ev[i]);
        (void)hipEventDestroy(c->cam_ev[i]);
        (void)hipEventDestroy(c->film_ev[i]);
    }
    for (int i = 3; i >= 0; --i) (void)hipStreamDestroy(c->streams[i]);
    delete c;
}

lumo_status lumo_set_option(void* ctx, int32_t option, int64_t value) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c) return LUMO_ERR_INVALID;
    return set_opt(*c, option, value);
}

lumo_status lumo_get_option(void* ctx, int32_t option, int64_t* value) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c || !value || option < 0 || option >= LUMO_OPT_COUNT) return LUMO_ERR_INVALID;
    *value = get_opt(*c, option);
    return LUMO_OK;
}

}  // extern "C"
