// The schedule of a render, decided once from the options, the scene's class, the render's size and
// the free device memory, before anything is allocated (device/kernels.hip render_impl); and the
// cut of a render's tasks into groups of consecutive tasks.  Plain C++: no device header, so the
// host sanitizer build (tools/sanitize) checks it against recorded plans.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../../include/lumo_amd.h"

namespace lumo {
namespace dev {

// Merged passes: by default as many as bring a unit to about kMergeTarget paths (a full 1024^2 frame: 1).
constexpr uint64_t kMergeTarget = (uint64_t)1 << 21;
// Device memory left free by the split schedule's extra pass sets.
constexpr size_t kSplitMargin = (size_t)8 << 30;

struct SchedIn {
    // execution options (ctx.h Opts)
    int64_t fused, lds, pipeline, heads, merge, tail_bounces, split_pipe, split_groups, bdpt_groups;
    bool bdpt;        // integrator
    bool dump;        // a path dump (lumo_debug_paths)
    int n_shadow;     // shadow rays per bounce of the scene
    bool staged;      // the scene is packed for whole-scene LDS staging
    bool fused_fits;  // ... and fits a block's LDS beside the fused kernel's parked NEE records
    int max_merge;    // passes per unit at most (state.h MAX_MERGE)
    int rr_depth;     // Russian roulette from this depth on (state.h RR_DEPTH)
    int N, n_tasks;   // slots and tasks of the render
    uint64_t max_samples;
    // split schedule: bytes of one extra pass set, set_bytes_fixed + set_bytes_slot x (slots N x M);
    // the free device memory (known: the query succeeded) and the bytes extra sets already hold
    size_t set_bytes_slot, set_bytes_fixed, free_hbm, held;
    bool hbm_known;
};

struct SchedPlan {
    int schedule;  // LUMO_SCHED_*; BDPT with one group runs its chain as LUMO_SCHED_SEQUENTIAL
    bool fused;    // the fused bounce kernel instead of closest / shade / visibility
    int M;         // merged passes per unit (1 unless a pipeline runs)
    int K;         // split schedule: units in flight; BDPT: groups
    int G;         // task groups
    int head_streams, head_bounces, tail_bounces;  // fused pipeline (else 0)
};

namespace plan_detail {
inline bool fused(const SchedIn& in) {
    return in.n_shadow == 1 && (in.fused < 0 ? (in.lds && in.staged && in.fused_fits) : in.fused != 0);
}
inline bool pipe(const SchedIn& in) { return !in.bdpt && fused(in) && in.pipeline; }
inline int split_groups(const SchedIn& in) { return std::max(1, std::min((int)in.split_groups, in.n_tasks)); }
}  // namespace plan_detail

// The split schedule's pipeline is tried: the plan then depends on the free device memory.
inline bool plan_reads_hbm(const SchedIn& in) {
    const uint64_t split_units = in.max_samples * (uint64_t)plan_detail::split_groups(in);
    return !in.bdpt && !plan_detail::pipe(in) && !in.dump && in.pipeline && in.split_pipe > 1 && split_units > 1;
}

inline SchedPlan plan_schedule(const SchedIn& in) {
    SchedPlan p{LUMO_SCHED_SEQUENTIAL, plan_detail::fused(in), 1, 1, 1, 0, 0, 0};
    if (in.bdpt) {
        // concurrent chains of passes for several tasks; one chain for a single task, on request
        // (LUMO_OPT_BDPT_GROUPS 1) and for a path dump
        p.G = in.dump ? 1 : std::max(1, std::min(std::min((int)in.bdpt_groups, 4), in.n_tasks));
        if (p.G > 1) {
            p.schedule = LUMO_SCHED_BDPT_GROUPS;
            p.K = p.G;
        }
        return p;
    }
    // fused bounces (n_shadow == 1, the scene and the fused kernel's parked NEE records fit the LDS
    // of a block) run in the fused pipeline; else the split schedule's pipeline, when the free
    // device memory allows
    const bool pipe = plan_detail::pipe(in), split_try = plan_reads_hbm(in);
    if (!pipe && !split_try) return p;
    // merged passes: units of about kMergeTarget paths
    int M = (int)std::min<uint64_t>((uint64_t)in.max_merge, (kMergeTarget + in.N - 1) / (uint64_t)in.N);
    // the split schedule merges passes only on request: at C3's 1/8 share merged units made the
    // frame slower (M = 2 / 4 / 8: 723 -> 761 / 807 / 812 ms; the unit's large head launches
    // hold the CUs while the latency-bound per-pass bounces of the group's chain wait; round 5)
    if (split_try) M = 1;
    if (in.merge > 0) M = (int)in.merge;
    M = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)M, in.max_samples));
    if ((uint64_t)in.N * (uint64_t)M > ((uint64_t)1 << 30)) M = 1;
    if (pipe) {
        p.schedule = LUMO_SCHED_FUSED_PIPELINE;
        p.M = M;
        p.head_streams = std::min(std::max((int)in.pipeline, 1), 3);
        // bounces on the head stream: through the RR bounce when a pass holds many paths; with fewer
        // (a rank's share of a multi-GPU run) the RR bounce goes to the tail kernel too, so the head
        // stream never waits for the previous pass's ring (362^2: 509 -> 434 ms).  Merged units
        // (M > 1) always stop before it.
        p.head_bounces = in.heads > 0 ? (int)in.heads : (in.N >= (1 << 21) ? in.rr_depth + 1 : in.rr_depth);
        if (M > 1) p.head_bounces = std::min(p.head_bounces, in.rr_depth);
        // fused bounces on the tail stream: 2 for one-pass units (a full frame: its chain of tails
        // and rings has room, and the bulk of the paths left after the head bounces runs at full
        // throughput; C1 2 467 -> 2 380 ms), none for merged units (a rank's share: the tail stream
        // is the critical chain)
        p.tail_bounces = in.tail_bounces >= 0 ? (int)in.tail_bounces : (M == 1 ? 2 : 0);
        return p;
    }
    // split schedule: units in flight, as many as split_pipe and the free device memory allow
    if (!in.hbm_known) return p;
    const size_t per_set = in.set_bytes_fixed + in.set_bytes_slot * (size_t)in.N * (size_t)M;
    const uint64_t units = (in.max_samples + (uint64_t)M - 1) / (uint64_t)M * (uint64_t)plan_detail::split_groups(in);
    int K = std::min(std::min((int)in.split_pipe, 4), (int)std::min<uint64_t>(units, 4));
    while (K > 1 && (size_t)(K - 1) * per_set + kSplitMargin > in.free_hbm + in.held) K--;
    if (K > 1) {
        p.schedule = LUMO_SCHED_SPLIT_PIPELINE;
        p.M = M;
        p.K = K;
        p.G = std::max(1, std::min((int)in.split_groups, std::min(K, in.n_tasks)));
    }
    return p;
}

// The tasks cut into G groups of consecutive tasks [t_lo, t_hi) of about N / G slots each, at least
// one task in every group (G <= n_tasks).  first: the tasks' first slots (n_tasks + 1 entries).
inline std::vector<std::pair<int, int>> task_groups(const int32_t* first, int n_tasks, int N, int G) {
    std::vector<std::pair<int, int>> r((size_t)G);
    for (int g = 0, t = 0; g < G; ++g) {
        const int lo = t;
        const int64_t target = (int64_t)N * (g + 1) / G;
        while (t < n_tasks && (g == G - 1 || first[t + 1] <= target || t == lo)) ++t;
        t = std::max(std::min(t, n_tasks - (G - 1 - g)), lo + 1);  // >= 1 task here and in every later group
        r[(size_t)g] = {lo, t};
    }
    return r;
}

}  // namespace dev
}  // namespace lumo
