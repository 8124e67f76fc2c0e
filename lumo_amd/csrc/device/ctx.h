// The context of the C ABI and what the device translation units share of it: device buffers,
// launch timing, the execution options and the error plumbing.  kernels.hip holds the kernels and
// the schedulers, ctx.hip the context's life and the options, upload.hip the scene and the camera.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../../include/lumo_amd.h"
#include "state.h"

namespace lumo {
namespace dev {

#define HIPCHK(x)                                \
    do {                                         \
        hipError_t e__ = (x);                    \
        if (e__ != hipSuccess) {                 \
            last_hip_error() = e__;              \
            return LUMO_ERR_HIP;                 \
        }                                        \
    } while (0)

hipError_t& last_hip_error();  // of the calling thread (lumo_status_str)

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

// Per-launch HIP event pairs, resolved at the synchronisation points the host loop already
// has (queue-count readbacks), so timing adds no extra stalls.
struct Timing {
    std::vector<hipEvent_t> free_ev;
    struct Pending {
        int stage;
        hipEvent_t a, b;
    };
    std::vector<Pending> pending;
    hipEvent_t get() {
        if (free_ev.empty()) {
            hipEvent_t e;
            (void)hipEventCreate(&e);
            return e;
        }
        hipEvent_t e = free_ev.back();
        free_ev.pop_back();
        return e;
    }
    ~Timing() {
        for (hipEvent_t e : free_ev) (void)hipEventDestroy(e);
        for (const Pending& p : pending) {
            (void)hipEventDestroy(p.a);
            (void)hipEventDestroy(p.b);
        }
    }
};

// Execution options of a context (lumo_set_option; include/lumo_amd.h LUMO_OPT_*).  None of them
// changes a result.  Defaults here, then the environment at lumo_create.  Every field is an
// int64_t (the API's value type) so that one table row per option (ctx.hip kOpts) can name it.
struct Opts {
    int64_t timing = 0;
    int64_t lds = 1;                   // whole scene in LDS when it fits (48 KiB)
    int64_t top = 1;                   // TOP staging of larger scenes
    int64_t fused = -1;                // n_shadow == 1: k_bounce_q instead of closest / shade / shadow (-1: when LDS-staged)
    int64_t tail_below = 1u << 16;     // n_shadow == 1: k_bounce_q tail mode below this many live paths
                                       // (split passes; C2 4-spp frame 332 ms at 2^18, 312-319 ms at 2^16)
    int64_t pipeline = 3;              // fused passes overlapped (render_pipelined): 0 off, else head streams (1-3)
    int64_t heads = 0;                 // pipelined passes: fused bounces per pass before the tail kernel (0: auto)
    int64_t merge = 0;                 // pipelined passes: passes merged into one head unit (0: auto)
    int64_t dyn = 0;                   // k_bounce_q: blocks fetch their paths from a counter (1) or take
                                       // static grid-stride stripes (0; with lds_grid 384: C1 2 150 vs
                                       // 2 350 ms per frame, 1/8 share 291 vs 367 ms, profiles/r05/ab/r05z*)
    int64_t bounce_threads = BLOCK;    // k_bounce_q (fused, not tail): threads per block (64, 128 or 256)
    int64_t split_pipe = 4;            // split schedule: units in flight (render_split_pipelined; 1 = sequential)
    int64_t split_groups = 2;          // split schedule: independent task groups
    int64_t bdpt_tail = 1u << 16;      // BDPT walks: k_bdpt_tail below this many live subpaths (0: never)
    int64_t bounce_ahead = 3;          // bounces enqueued ahead of the host's count snapshots
    int64_t lds_grid = 384;            // grid cap of the LDS-staged kernels: 1.5 blocks per CU (set from the
                                       // CU count at creation); the three head streams' launches and the
                                       // tail stream's share the CUs instead of queueing behind each other
    int64_t top_grid = 128;            // TOP kernels: blocks of 1 024 threads, one per CU on half the CUs (set from
                                       // the CU count at creation), so the split pipeline's concurrent units
                                       // share the GPU: C2 4-spp 305 -> 288 ms, C3 64-spp 4 084 -> 4 007 ms, its
                                       // 1/8 share 723 -> 692 ms against one block on every CU (r05t*)
    int64_t top_kb = 160;              // TOP set budget (KiB), at most the CU's LDS
    int64_t kd_lds = 8;                // kd stack entries per thread in LDS in TOP kernels when room is left (C2 -3 %)
    int64_t stack_class = 0;           // kd stack class override (0: the scene's need)
    int64_t full_kernels = 0;          // general feature kernels for lean scenes too
    int64_t poison = 0;                // new device buffers filled with 0xFF (reads before writes show as NaN / -1)
    int64_t tail_priority = 0;         // the pipelined passes' tail / film / ring stream at high priority
    int64_t top_kd = 1;                // the TOP set's spare LDS holds the top treelets of the largest kd tree
    int64_t tail_bounces = -1;         // fused pipeline: fused bounces per pass on the tail stream before the tail kernel (-1 auto)
    int64_t bdpt_top = 1;              // BDPT connection visibility of large scenes with TOP staging
    int64_t film_first = 0;            // fused pipeline, film on the tail stream: the film before the unit's last ring
    int64_t bdpt_groups = 2;           // BDPT: task groups rendered as concurrent pass chains (render_bdpt_groups)
    int64_t ray_sort = -1;             // split bounces: closest-hit rays sorted (1 octant major, 2 origin major;
                                       // -1 auto: 1 for deep kd trees, stack class >= 32: C2 4-spp frame
                                       // 309 / 312 -> 302 ms; C3, class 24: 556 -> 563 ms, so off there)
    int64_t accel = 0;                 // upload: 0 lumo's BVHs + kd-trees, 1 the wide BVH (wbvh.h)
};

struct Ctx {
    int device = 0;
    size_t lds_cu = 160 * 1024;     // LDS per CU (hipDeviceProp_t::maxSharedMemoryPerMultiProcessor)
    size_t lds_block = 160 * 1024;  // LDS one block may allocate (sharedMemPerBlock)
    Opts o;
    // 0: the main stream; 1: the pipelined passes' tail, film and ring (make_tail_stream recreates
    // it); 2, 3: further head streams of the pipelined passes.  The split and BDPT schedules run
    // unit / group k on stream k.
    hipStream_t streams[4] = {};
    hipEvent_t pass_ev[4] = {}, tail_ev[4] = {}, cam_ev[4] = {}, film_ev[4] = {};
    bool has_scene = false, has_camera = false;
    DScene sc{};
    DCam cam{};
    std::vector<DevBuf> scene_bufs;
    std::vector<DevBuf> work;  // grown on demand
    lumo_stats stats{};
    lumo_schedule_info sched{};  // of the last render
    Timing tm;
    int tone_map = LUMO_TONEMAP_NONE;  // of the lumo_render_tiles call in progress
    double tone_arg = 0.0;
    // per-bounce queue-count snapshots (pinned) and their completion events
    static constexpr int SNAP_RING = 64;
    uint32_t* snap = nullptr;
    hipEvent_t snap_ev[SNAP_RING];
    // integrator of the call in progress (BDPT: vertex storage per subpath, optional splat film)
    int integrator = LUMO_INTEGRATOR_PATH_TRACE;
    int max_vertices = 64;
    double* splat_film = nullptr;
    int debug_integrator = LUMO_INTEGRATOR_PATH_TRACE;  // lumo_debug_paths
    int sampler = LUMO_SAMPLER_MULTI_JITTERED;          // of the lumo_render_tiles call in progress
    int debug_sampler = LUMO_SAMPLER_MULTI_JITTERED;    // lumo_debug_paths
    size_t split_sets_bytes = 0;  // work buffers already held by the extra pass sets (free-memory check)
    // Launch intervals of the timed stages (ms from ref_ev, recorded before the first timed launch
    // after a stats reset): their union is a stage's busy time, which does not count twice the
    // time that launches on different streams overlap (lumo_stats_busy_ms)
    hipEvent_t ref_ev = nullptr;
    bool ref_recorded = false;
    std::vector<std::pair<float, float>> intervals[LUMO_STAGE_COUNT];
    // BDPT task groups (render_bdpt_groups): per-group work buffers, pinned item totals, events
    std::vector<DevBuf> gwork;
    uint32_t* bd_totals_h = nullptr;
    hipEvent_t bd_ev[4] = {};
    V3 sort_lo{0.0, 0.0, 0.0}, sort_scale{0.0, 0.0, 0.0};  // ray sorting: the scene's world box -> 512 cells per axis
    int w_nodes = 0, w_tris = 0, w_stack = 0, w_depth = 0;     // the uploaded wide BVH (lumo_scene_info)
};

lumo_status dev_alloc(const Ctx& c, DevBuf& b, size_t bytes);
void free_scene(Ctx& c);

template <typename T>
lumo_status upload(Ctx& c, const T* host, size_t count, const T** dptr) {
    c.scene_bufs.emplace_back();
    DevBuf& b = c.scene_bufs.back();
    const lumo_status st = dev_alloc(c, b, sizeof(T) * count);
    if (st) return st;
    if (count && host) HIPCHK(hipMemcpy(b.p, host, sizeof(T) * count, hipMemcpyHostToDevice));
    *dptr = static_cast<const T*>(b.p);
    return LUMO_OK;
}

}  // namespace dev
}  // namespace lumo
