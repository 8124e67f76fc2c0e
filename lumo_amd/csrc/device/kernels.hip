// MI355X wavefront path tracer: HIP kernels for gfx950, the schedulers that launch them and the
// entry points of the C ABI that render, trace or time.  (The context and its options: ctx.hip;
// the scene upload and the camera: upload.hip; what the three share: ctx.h.)
//
// One path slot per (tile task, pixel).  Per sample pass:
//   k_camera   MultiJittered sample + camera ray + hero wavelengths  (integrator.rs:45-70)
//   repeat until no path is alive:
//     k_closest  Scene::hit for the active queue                     (scene.rs:119-147)
//     k_shade    BSDF sample, NEE shadow-ray records, spawn, RR       (path_trace.rs:18-77,
//                                                                      integrator.rs:87-137)
//     k_shadow   Scene::hit_light + MIS for the shadow records of each  (integrator.rs:74-184)
//                path, folded into its radiance in lumo's order
//   k_finish   per-sample XYZ -> white balance -> RGB, luminance, cost (film/tile.rs:65-66, task.rs:64-69)
//   k_film     tile-clipped Gaussian splat as a deterministic gather   (film/tile.rs:65-111)
//   k_ring     adaptive-RR ring buffer + delta of the next pass        (task.rs:28-69)
// Active-path queues are compacted with wave64 ballot + mbcnt prefix sums and one atomic per
// wavefront.  All arithmetic is IEEE f64 without contraction (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <type_traits>
#include <vector>

#include "../../../include/lumo_amd.h"
#include "../common/sched_plan.h"

#define LUMO_MAIN_TU
#include "launch.h"
#include "scan.h"
#include "pt.h"
#include "ctx.h"

using namespace lumo;
using namespace lumo::dev;

namespace {

// Per-slot outputs of pass m of a merged unit (render_pipelined): virtual slots [m N, (m + 1) N).
__host__ __device__ inline Paths pass_view(const Paths& P, int m, int N) {
    Paths V = P;
    const size_t o = (size_t)m * (size_t)N;
    V.rad = P.rad + 4 * o;
    V.lam = P.lam + 4 * o;
    V.raster = P.raster + 2 * o;
    V.depth = P.depth + o;
    V.queries = P.queries + o;
    V.p_valid = P.p_valid + o;
    return V;
}

// ------------------------------------------------------------------ init
// Pixel sampler seeds: the tile stream's first P outputs.
__global__ void k_init_seeds(Tasks T, Paths S, int n_tasks) {
    const int ti = blockIdx.x * blockDim.x + threadIdx.x;
    if (ti >= n_tasks) return;
    Xorshift r = xs_new(T.t[ti].seed);
    for (int s = T.first[ti]; s < T.first[ti + 1]; ++s) S.pseed[s] = xs_u64(r);
}

// SamplerType::new (samplers.rs:26-37) per pixel: the sampler's Xorshift::new(seed) (Uniform,
// Jittered, MultiJittered) and, for MultiJitteredSampler::new (samplers.rs:148-171), its two
// Fisher-Yates permutations; the state starts at the batch's first sample s0.  Sobol keeps no RNG
// (its seed is the pixel seed, read by k_camera).
__global__ void k_init_mj(Tasks T, Paths S, int n, int dim_stride) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const lumo_tile_task& t = T.t[S.task[s]];
    S.mj_state[s] = t.batch * SAMPLES_INCREMENT;
    Xorshift r = xs_new(S.pseed[s]);
    if (T.sampler != LUMO_SAMPLER_MULTI_JITTERED) {
        S.mj_rng[2 * s] = r.hi;
        S.mj_rng[2 * s + 1] = r.lo;
        return;
    }
    const uint64_t dim = (uint64_t)ceil(sqrt((double)t.total_samples));
    uint16_t* px = S.perm + (size_t)s * 2 * dim_stride;
    uint16_t* py = px + dim_stride;
    for (int which = 0; which < 2; ++which) {
        uint16_t* p = which == 0 ? px : py;
        for (uint64_t i = 0; i < dim; ++i) p[i] = (uint16_t)i;
        for (uint64_t i = 0; i + 1 < dim; ++i) {
            const uint64_t rnd = xs_u64(r);
            const uint64_t j = i + rnd % (dim - i);
            const uint16_t tmp = p[i];
            p[i] = p[j];
            p[j] = tmp;
        }
    }
    S.mj_rng[2 * s] = r.hi;
    S.mj_rng[2 * s + 1] = r.lo;
}

// SobolSampler (samplers.rs:196-248, sobol_seq.rs): direction numbers m_i << (63 - i) of the two
// dimensions (sobol_seq.rs:10-13, map_m_v :32-39).  The point after `n` steps from 0 is the XOR of
// the directions at the set bits of the Gray code n ^ (n >> 1) (each step XORs the direction at
// trailing_zeros(n), the bit in which consecutive Gray codes differ); BATCH_STATES[b] is the
// point at n = 256 b, so the same closed form covers every batch.
__device__ __forceinline__ uint64_t sobol_dir(int dimension, int i) {
    const uint64_t m1[10] = {1, 1, 7, 15, 5, 19, 69, 51, 121, 695};
    const uint64_t m2[10] = {1, 1, 7, 7, 7, 53, 57, 229, 473, 533};
    return (dimension == 0 ? m1[i] : m2[i]) << (63 - i);
}
__device__ __forceinline__ uint64_t sobol_point(int dimension, uint64_t n) {
    const uint64_t g = n ^ (n >> 1);
    uint64_t x = 0;
    for (int i = 0; i < 10; ++i)
        if ((g >> i) & 1) x ^= sobol_dir(dimension, i);
    return x;
}

// Sampler::next for the pixel's sampler (samplers.rs:61-248); `st` is the state before the call.
__device__ __forceinline__ V2 sampler_next(int kind, const lumo_tile_task& t, const uint16_t* px, const uint16_t* py,
                                           uint64_t st, Xorshift& mr, uint64_t pixel_seed) {
    if (kind == LUMO_SAMPLER_UNIFORM) return xs_vec2(mr);  // UniformSampler::next (:73-84)
    if (kind == LUMO_SAMPLER_SOBOL) {  // SobolSampler::next (:236-248): step, then shuffle the point
        const uint64_t a = sobol_point(0, st + 1) ^ pixel_seed, b = sobol_point(1, st + 1) ^ pixel_seed;
        const double s64 = 0x1p-64;  // Float::powi(2.0, -64)
        return V2{(double)a * s64, (double)b * s64};
    }
    const uint64_t dim = (uint64_t)ceil(sqrt((double)t.total_samples));
    const V2 scale0 = V2{1.0 / (double)dim, (double)dim / (double)t.total_samples};
    const uint64_t x0 = st % dim, y0 = st / dim;
    const V2 offset0 = scale0 * V2{(double)x0, (double)y0};
    if (kind == LUMO_SAMPLER_JITTERED) return scale0 * xs_vec2(mr) + offset0;  // JitteredSampler::next (:113-131)
    // MultiJitteredSampler::next (samplers.rs:174-193)
    const V2 scale1 = scale0 / (double)dim;
    const V2 offset1 = scale1 * V2{(double)px[y0], (double)py[x0]};
    const V2 rsq = scale1 * xs_vec2(mr);
    return offset0 + offset1 + rsq;
}

__device__ __forceinline__ uint64_t wf_path_seed(uint64_t pixel_seed, uint64_t k) {
    return splitmix64(pixel_seed ^ splitmix64(k + 1));
}

// ------------------------------------------------------------------ camera (passes pass0 .. pass0 + npass - 1)
// QUEUE (path tracer): the camera paths enter the queue-order state qs[0]; otherwise (BDPT) the
// ray, throughput, wavelengths and RNG stay per slot and the slot ids are queued in q0.
// npass > 1 (merged passes of the fused pipeline, render_pipelined): each thread generates its
// slot's samples of npass consecutive passes in pass order (the sampler state is per slot), and
// the path of pass pass0 + m carries the virtual slot s + m * vstride, where that pass's per-slot
// outputs (raster, validity, final radiance, ...) live.
template <bool QUEUE>
__global__ __launch_bounds__(BLOCK) void k_camera(Tasks T, Paths S, DCam cam, int n, int dim_stride, uint32_t pass0,
                                                  int s0, int npass, int vstride) {
    const int s = s0 + (int)(blockIdx.x * blockDim.x + threadIdx.x);  // slots [s0, n)
    for (int m = 0; m < npass; ++m) {
        const uint32_t pass = pass0 + (uint32_t)m;
        const int v = s + m * vstride;  // virtual slot of this pass
        bool active = false;
        Ray ray{V3{0, 0, 0}, V3{0, 0, 0}};
        double L[NS] = {0.0, 0.0, 0.0, 0.0};
        Xorshift r{0, 0};
        int task = 0;
        if (s < n) {
            task = S.task[s];
            const lumo_tile_task& t = T.t[task];
            active = pass < t.samples;
            S.p_valid[v] = active ? 1u : 0u;
            if (active) {
                Xorshift mr{S.mj_rng[2 * s], S.mj_rng[2 * s + 1]};
                const uint64_t st = S.mj_state[s];
                const uint16_t* px = S.perm + (size_t)s * 2 * dim_stride;
                const V2 rs = sampler_next(T.sampler, t, px, px + dim_stride, st, mr, S.pseed[s]);
                S.mj_state[s] = st + 1;
                S.mj_rng[2 * s] = mr.hi;
                S.mj_rng[2 * s + 1] = mr.lo;
                const int j = S.pix[s];
                const uint64_t W = t.px_max[0] - t.px_min[0];
                const V2 xy = V2{(double)(t.px_min[0] + (uint64_t)j % W), (double)(t.px_min[1] + (uint64_t)j / W)};
                const V2 raster = xy + rs;
                // Integrator::integrate: lens sample (2 draws), then wavelengths (1 draw)
                r = xs_new(wf_path_seed(S.pseed[s], pass));
                const V2 lens = xs_vec2(r);
                const V3 screen = xf_pt_inv(cam.sctr, V3{raster.x, raster.y, 0.0});
                // Camera::generate_ray (camera.rs:257-268): Perspective aims from the origin through the
                // normalised camera-space point; Orthographic starts at the point, along +z
                const V3 cpt = xf_pt_inv(cam.cts, screen);
                const V3 wl0 = cam.orthographic ? V3{0.0, 0.0, 1.0} : normalize(cpt);
                V3 xo_local = cam.orthographic ? cpt : V3{0, 0, 0}, wi_local = wl0;
                if (cam.lens_radius != 0.0) {  // camera.rs:221-243
                    const V2 lxy = cam.lens_radius * square_to_disk(lens);
                    const V3 lz = V3{lxy.x, lxy.y, 0.0};
                    const V3 focus = (cam.focal_length / wl0.z) * wl0;
                    xo_local = xo_local + lz;
                    wi_local = focus - lz;
                }
                ray = ray_new(xf_pt_inv(cam.wtc, xo_local), xf_dir_inv(cam.wtc, wi_local));
                wl_sample(xs_float(r), L);
                S.raster[2 * v] = raster.x;
                S.raster[2 * v + 1] = raster.y;
                if (!QUEUE) {
                    stv3(S.ro, s, ray.o);
                    stv3(S.rd, s, ray.d);
                    stc(S.gath, s, cfill(1.0));
                    stc(S.rad, s, cfill(0.0));
                    for (int i = 0; i < NS; ++i) S.lam[4 * s + i] = L[i];
                    S.rng[2 * s] = r.hi;
                    S.rng[2 * s + 1] = r.lo;
                    S.depth[s] = 0;
                    S.flags[s] = 1u;  // last_specular
                    S.queries[s] = 0;
                }
            }
        }
        if (QUEUE) {
            const uint32_t q = block_slot(active, S.counts + CNT_NEXT);
            if (active) {
                const QState& Q = S.qs[0];
                qv3(Q, QD_O, q, ray.o);
                qv3(Q, QD_D, q, ray.d);
                qc(Q, QD_G, q, cfill(1.0));
                qc(Q, QD_R, q, cfill(0.0));
                for (int i = 0; i < NS; ++i) Q.D(QD_L + i, q) = L[i];
                Q.R(0, q) = r.hi;
                Q.R(1, q) = r.lo;
                Q.I(QI_SLOT, q) = v;
                Q.I(QI_TASK, q) = task;
                Q.I(QI_DEPTH, q) = 0;
                Q.I(QI_FLAGS, q) = QF_SPECULAR;  // last_specular starts true (path_trace.rs:14)
                Q.I(QI_QUERIES, q) = 0;
            }
        } else {
            block_append(active, s, S.q0, S.counts + CNT_NEXT);
        }
    }
}

// Start of a bounce: the alive queue just built becomes the current one.
__global__ void k_bounce_begin(uint32_t* counts, unsigned long long* headq) {
    if (threadIdx.x == 0) {
        atomicAdd(headq, (unsigned long long)counts[CNT_NEXT]);  // this bounce's closest queries (streams run concurrently)
        counts[CNT_CUR] = counts[CNT_NEXT];
        counts[CNT_NEXT] = 0;
        counts[CNT_FETCH_B] = 0;
        counts[CNT_FETCH_C] = 0;
        counts[CNT_FETCH_T] = 0;
        for (int b = 0; b < NB; ++b) counts[CNT_BUCKET0 + b] = 0;
        for (int k = 0; k < SHQ_CLASSES; ++k) counts[CNT_SHQ + k] = 0;
    }
}

// Ray sorting (LUMO_OPT_RAY_SORT): a counting sort of a bounce's live closest-hit rays on a 12-bit
// key (scan.h rs_key: the direction octant and the origin's cell among 8 per axis of the objects
// BVH's world box), so that neighbouring lanes walk alike rays.  It changes which lane walks which
// ray, nothing else (k_closest_q writes each hit at its ray's own position).  Two launches: keys +
// histogram, then the histogram's scan + scatter into perm (the walk order of queue positions).
__global__ __launch_bounds__(RS_BLOCK) void k_rsort_keys(QState cur, const uint32_t* counts, uint32_t n, V3 lo,
                                                         V3 scale, int mode, uint32_t* keys, uint32_t* ws) {
    const uint32_t q = blockIdx.x * RS_BLOCK + threadIdx.x;
    const bool live = q < n && q < counts[CNT_CUR];
    uint32_t key = 0;
    if (live) {
        const V3 o = qv3(cur, QD_O, q), d = qv3(cur, QD_D, q);
        key = rs_key(o.x, o.y, o.z, d.x, d.y, d.z, lo.x, lo.y, lo.z, scale.x, scale.y, scale.z, mode);
        keys[q] = key;
    }
    rs_count_block(key, live, ws);
}
__global__ __launch_bounds__(RS_BLOCK) void k_rsort_scatter(const uint32_t* keys, const uint32_t* counts, uint32_t n,
                                                            uint32_t* ws, uint32_t* perm) {
    const uint32_t q = blockIdx.x * RS_BLOCK + threadIdx.x;
    const bool live = q < n && q < counts[CNT_CUR];
    rs_scatter_block(live ? keys[q] : 0u, live, q, ws, perm);
}
// ... of a BDPT walk bounce: the queue holds slot ids, the rays live per slot; the sorted values are
// the slot ids in walk order (a queue in their own right)
__global__ __launch_bounds__(RS_BLOCK) void k_rsort_keys_slots(const int32_t* queue, const double* ro, const double* rd,
                                                               const uint32_t* counts, uint32_t n, V3 lo, V3 scale,
                                                               int mode, uint32_t* keys, uint32_t* ws) {
    const uint32_t q = blockIdx.x * RS_BLOCK + threadIdx.x;
    const bool live = q < n && q < counts[CNT_CUR];
    uint32_t key = 0;
    if (live) {
        const int s = queue[q];
        const V3 o = ldv3(ro, s), d = ldv3(rd, s);
        key = rs_key(o.x, o.y, o.z, d.x, d.y, d.z, lo.x, lo.y, lo.z, scale.x, scale.y, scale.z, mode);
        keys[q] = key;
    }
    rs_count_block(key, live, ws);
}
__global__ __launch_bounds__(RS_BLOCK) void k_rsort_scatter_slots(const int32_t* queue, const uint32_t* keys,
                                                                  const uint32_t* counts, uint32_t n, uint32_t* ws,
                                                                  uint32_t* perm) {
    const uint32_t q = blockIdx.x * RS_BLOCK + threadIdx.x;
    const bool live = q < n && q < counts[CNT_CUR];
    rs_scatter_block(live ? keys[q] : 0u, live, live ? (uint32_t)queue[q] : 0u, ws, perm);
}

// Setup zeroing of a render's accumulators and counters in one launch instead of a fill per
// buffer (every buffer is a hipMalloc allocation or a whole field of one, 4-byte granular).
struct ZeroList {
    static constexpr int MAX = 16;
    uint32_t* p[MAX];
    uint64_t words[MAX];
    int n = 0;
    bool overflow = false;  // more than MAX buffers added: the caller fails instead of launching
    void add(void* ptr, size_t bytes) {
        if (n == MAX) {
            overflow = true;
            return;
        }
        p[n] = static_cast<uint32_t*>(ptr);
        words[n] = bytes / 4;
        ++n;
    }
};
__global__ __launch_bounds__(BLOCK) void k_zero_list(ZeroList z) {
    const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
    for (int k = 0; k < z.n; ++k)
        for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < z.words[k]; i += stride) z.p[k][i] = 0u;
}

// The queue of a merged unit after its head bounces, split by pass (render_pipelined): the entry of
// a path of pass m (virtual slot in [m N, (m + 1) N)) goes to segment m of `dst` (entries m N + k),
// counted in CNT_NEXT of counts + (1 + m) CNT_N (zeroed by the caller; k_bounce_begin then starts
// the pass's bounce as usual).  Entries keep every
// plane; each pass's tail kernel then runs on full waves of its own paths.  Positions within a
// segment follow the block-aggregated atomics, a lane assignment only.
__global__ __launch_bounds__(BLOCK) void k_split_passes(QState src, QState dst, uint32_t* counts, int N, int M) {
    __shared__ uint32_t hist[MAX_MERGE], seg_base[MAX_MERGE];
    const uint32_t count = counts[CNT_NEXT];  // the last head bounce's continuing paths
    for (uint32_t b0 = blockIdx.x * blockDim.x; b0 < count; b0 += gridDim.x * blockDim.x) {
        if (threadIdx.x < MAX_MERGE) hist[threadIdx.x] = 0u;
        __syncthreads();
        const uint32_t q = b0 + threadIdx.x;
        int m = -1;
        uint32_t rank = 0;
        if (q < count) {
            m = src.I(QI_SLOT, q) / N;
            rank = atomicAdd(&hist[m], 1u);
        }
        __syncthreads();
        if (threadIdx.x < M && hist[threadIdx.x])
            seg_base[threadIdx.x] = atomicAdd(counts + (1 + threadIdx.x) * CNT_N + CNT_NEXT, hist[threadIdx.x]);
        __syncthreads();
        if (m >= 0) {
            const size_t d = (size_t)m * N + seg_base[m] + rank;
            for (int k = 0; k < QD_N; ++k) dst.D(k, d) = src.D(k, q);
            for (int k = 0; k < 2; ++k) dst.R(k, d) = src.R(k, q);
            for (int k = 0; k < QI_N; ++k) dst.I(k, d) = src.I(k, q);
        }
        __syncthreads();
    }
}

// Segment m (entries m N ..) of a queue as a queue of its own.
QState segment(const QState& Q, int m, int N) {
    QState V = Q;
    const size_t o = (size_t)m * (size_t)N;
    V.d += o;
    V.r += o;
    V.i += o;
    return V;
}

// Queue counters (and optionally one more word) zeroed in-stream: a kernel instead of a fill.
__global__ void k_zero_counts(uint32_t* counts, uint32_t* extra) {
    if (threadIdx.x < CNT_N) counts[threadIdx.x] = 0u;
    if (extra && threadIdx.x == 0) *extra = 0u;
}

// ------------------------------------------------------------------ finish + film + ring
// ToneMap::map (tone_mapping.rs:38-63), then XYZ -> white balance -> colour space
// (film/tile.rs:65-66, space.rs:125-151)
__device__ __forceinline__ V3 sample_rgb(const DScene& sc, const DCam& cam, const DColor& c, const double* L,
                                         int tone_map, double tone_arg) {
    DColor tc = c;
    if (tone_map == LUMO_TONEMAP_CLAMP) {
        for (int i = 0; i < NS; ++i) {
            double v = tc.s[i];
            if (v < 0.0) v = 0.0;
            if (v > tone_arg) v = tone_arg;
            tc.s[i] = v;
        }
    } else if (tone_map == LUMO_TONEMAP_REINHARD) {
        tc = c / (1.0 + luminance(sc, c, L));
    }
    return m3_mul_vec(cam.x2r, m3_mul_vec(cam.wb, color_xyz(sc, tc, L)));
}

// Per sample: luminance and cost for the ring, tone map -> XYZ -> WB -> RGB for the film.
// debug_assertions sample checks of ToneMap::map (tone_mapping.rs:42-56), counted: 1 NaN, 2 negative,
// 3 suspiciously large (max > 1000), in lumo's precedence; 0 otherwise.
__device__ __forceinline__ int sample_check(const DColor& c) {
    bool nan = false, neg = false;
    double mx = -DINF;
    for (int i = 0; i < NS; ++i) {
        nan = nan || c.s[i] != c.s[i];
        neg = neg || c.s[i] < 0.0;
        mx = rmax(mx, c.s[i]);
    }
    return nan ? 1 : (neg ? 2 : (mx > 1000.0 ? 3 : 0));
}
// Wave-aggregated check counters; every lane of the wave must call it.
__device__ __forceinline__ void count_checks(int cat, unsigned long long* dst) {
    const uint64_t m1 = __ballot(cat == 1), m2 = __ballot(cat == 2), m3 = __ballot(cat == 3);
    if (lane_id() == 0) {
        if (m1) atomicAdd(dst, (unsigned long long)__popcll(m1));
        if (m2) atomicAdd(dst + 1, (unsigned long long)__popcll(m2));
        if (m3) atomicAdd(dst + 2, (unsigned long long)__popcll(m3));
    }
}

// (the sample's luminance and cost for the adaptive-RR ring are k_ring's, from the same values)
__device__ __forceinline__ V3 finish_one(const DScene& sc, const Paths& S, const DCam& cam, int s, uint32_t pass,
                                         const Dump& dump, int dump_p, int tone_map, double tone_arg) {
    double L[NS];
    for (int i = 0; i < NS; ++i) L[i] = S.lam[4 * s + i];
    const DColor c = ldc(S.rad, s);
    const V3 rgb = sample_rgb(sc, cam, c, L, tone_map, tone_arg);
    if (dump.rad) {
        const size_t o = (size_t)pass * dump_p + S.pix[s];
        for (int i = 0; i < NS; ++i) {
            dump.rad[4 * o + i] = c.s[i];
            dump.lam[4 * o + i] = L[i];
        }
        dump.raster[2 * o] = S.raster[2 * s];
        dump.raster[2 * o + 1] = S.raster[2 * s + 1];
        dump.depth[o] = S.depth[s];
    }
    return rgb;
}

__global__ __launch_bounds__(BLOCK) void k_finish(DScene sc, Paths S, DCam cam, int n, uint32_t pass, Dump dump,
                                                   int dump_p, int tone_map, double tone_arg, int s0) {
    const int s = s0 + (int)(blockIdx.x * blockDim.x + threadIdx.x);  // slots [s0, n)
    int cat = 0;
    if (s < n && S.p_valid[s]) {
        cat = sample_check(ldc(S.rad, s));
        stv3(S.p_rgb, s, finish_one(sc, S, cam, s, pass, dump, dump_p, tone_map, tone_arg));
    }
    count_checks(cat, S.checks);
}

// Filter footprints up to FILM_R pixels: each source sample's separable Gaussian terms
// max(gauss(v) - gauss(r), 0) for its 2r+1 columns / rows are computed once per sample (by the
// sample's own thread, into LDS) instead of once per (sample, destination) pair; the gather reads
// them in the same order, so the film is bit-identical.
constexpr int FILM_R = 2;
struct FilmTerms {
    const double* wx;  // [2 * FILM_R + 1][BLOCK]: column term of source k at gx = px_k - r + i
    const double* wy;
    int r;
};

__device__ __forceinline__ double gauss(double x, double sigma) {
    return lm_exp(-(x * x) / (2.0 * sigma * sigma)) / sqrt(rmax(2.0 * PI * sigma * sigma, 0.0));
}

// FilmTile::add_sample as a gather: destination pixel j of task t (slot s) receives, in source
// raster order, the samples whose (tile-clipped) 3x3 footprint contains it.  Sources farther
// than 2 px cannot.  `src` reads a source sample by its pixel index within the tile.
template <class Src>
__device__ __forceinline__ void film_gather_acc(double* acc, const lumo_tile_task& t, const DCam& cam, int j,
                                                const Src& src, const FilmTerms* terms = nullptr) {
    const int W = (int)(t.px_max[0] - t.px_min[0]), H = (int)(t.px_max[1] - t.px_min[1]);
    const int dx = j % W, dy = j / W;
    const uint64_t gx = t.px_min[0] + dx, gy = t.px_min[1] + dy;
    const uint64_t r = (uint64_t)ceil(cam.fr - 0.5);
    const double gr = gauss(cam.fr, cam.fsig);
    for (int sy = dy - 2; sy <= dy + 1; ++sy) {
        if (sy < 0 || sy >= H) continue;
        for (int sx = dx - 2; sx <= dx + 1; ++sx) {
            if (sx < 0 || sx >= W) continue;
            const int k = sy * W + sx;
            if (!src.valid(k)) continue;
            const double rx = src.rx(k), ry = src.ry(k);
            const uint64_t px = rx > 0.0 ? (uint64_t)floor(rx) : 0, py = ry > 0.0 ? (uint64_t)floor(ry) : 0;
            const uint64_t mix = std::max(px >= r ? px - r : 0, t.px_min[0]);
            const uint64_t miy = std::max(py >= r ? py - r : 0, t.px_min[1]);
            const uint64_t mxx = std::min(px + r, t.px_max[0] - 1), mxy = std::min(py + r, t.px_max[1] - 1);
            if (gx < mix || gx > mxx || gy < miy || gy > mxy) continue;
            double w;
            if (terms) {  // the source's precomputed terms (px - r <= gx <= px + r)
                w = terms->wx[(int)(gx + r - px) * BLOCK + k] * terms->wy[(int)(gy + r - py) * BLOCK + k];
            } else {
                const double vx = rx - (0.5 + (double)gx), vy = ry - (0.5 + (double)gy);
                w = rmax(gauss(vx, cam.fsig) - gr, 0.0) * rmax(gauss(vy, cam.fsig) - gr, 0.0);
            }
            if (w != 0.0) {
                const V3 c = src.rgb(k) * w;
                acc[0] += c.x;
                acc[1] += c.y;
                acc[2] += c.z;
                acc[3] += w;
            }
        }
    }
}
template <class Src>
__device__ __forceinline__ void film_gather(const Paths& S, const lumo_tile_task& t, const DCam& cam, int s, int j,
                                            const Src& src, const FilmTerms* terms = nullptr) {
    double acc[4] = {S.film[4 * s], S.film[4 * s + 1], S.film[4 * s + 2], S.film[4 * s + 3]};
    film_gather_acc(acc, t, cam, j, src, terms);
    for (int i = 0; i < 4; ++i) S.film[4 * s + i] = acc[i];
}

struct HbmSrc {  // sources read from the per-slot buffers k_finish wrote
    const Paths& S;
    int first;
    __device__ bool valid(int k) const { return S.p_valid[first + k] != 0; }
    __device__ double rx(int k) const { return S.raster[2 * (first + k)]; }
    __device__ double ry(int k) const { return S.raster[2 * (first + k) + 1]; }
    __device__ V3 rgb(int k) const { return ldv3(S.p_rgb, first + k); }
};

__global__ __launch_bounds__(BLOCK) void k_film(Paths S, Tasks T, DCam cam, int n, int s0) {
    const int s = s0 + (int)(blockIdx.x * blockDim.x + threadIdx.x);  // slots [s0, n)
    if (s >= n) return;
    const int ti = S.task[s];
    film_gather(S, T.t[ti], cam, s, S.pix[s], HbmSrc{S, T.first[ti]});
}

// film_gather_acc with the source terms staged (r <= FILM_R): source k's footprint origin
// (ox, oy) = (px - r, py - r) relative to the tile, precomputed once per source (INT_MIN/4 for an
// invalid sample), so destination (dx, dy) takes source k iff 0 <= dx - ox <= 2r and
// 0 <= dy - oy <= 2r: the tile-clipped [px - r, px + r] test of film_gather_acc for destinations
// inside the tile.  Same sources in the same order, same weights and additions.
__device__ __forceinline__ void film_gather_staged(double* acc, const lumo_tile_task& t, int j, const double* rgb,
                                                   const int* l_ox, const int* l_oy, const FilmTerms& terms) {
    const int W = (int)(t.px_max[0] - t.px_min[0]), H = (int)(t.px_max[1] - t.px_min[1]);
    const int dx = j % W, dy = j / W;
    const unsigned r2 = 2u * (unsigned)terms.r;
    for (int sy = dy - 2; sy <= dy + 1; ++sy) {
        if (sy < 0 || sy >= H) continue;
        for (int sx = dx - 2; sx <= dx + 1; ++sx) {
            if (sx < 0 || sx >= W) continue;
            const int k = sy * W + sx;
            const unsigned ix = (unsigned)(dx - l_ox[k]), iy = (unsigned)(dy - l_oy[k]);
            if (ix > r2 || iy > r2) continue;
            const double w = terms.wx[(int)ix * BLOCK + k] * terms.wy[(int)iy * BLOCK + k];
            if (w != 0.0) {
                const V3 c = V3{rgb[3 * k], rgb[3 * k + 1], rgb[3 * k + 2]} * w;
                acc[0] += c.x;
                acc[1] += c.y;
                acc[2] += c.z;
                acc[3] += w;
            }
        }
    }
}

struct LdsSrc {  // sources staged in LDS by k_finish_film
    const double* rgb_;
    const double* ras;
    const uint32_t* ok;
    __device__ bool valid(int k) const { return ok[k] != 0; }
    __device__ double rx(int k) const { return ras[2 * k]; }
    __device__ double ry(int k) const { return ras[2 * k + 1]; }
    __device__ V3 rgb(int k) const { return V3{rgb_[3 * k], rgb_[3 * k + 1], rgb_[3 * k + 2]}; }
};


// k_finish + k_film for tasks of at most BLOCK pixels (lumo's 16x16 tiles): one block per task,
// the tile's sample RGB and raster positions staged in LDS instead of a round trip through HBM.
// npass consecutive passes (a merged unit of render_pipelined; pass m's per-slot outputs at
// virtual slots + m * vstride) in pass order, the tile's film accumulators held in registers
// across them.  Same arithmetic and additions in the same order as one k_finish + k_film per
// pass, so the film is bit-identical.
#ifndef LUMO_FILM_WAVES  // k_finish_film: 129 VGPRs gave 3 waves / SIMD; 4 fit its LDS (4 x 33 KB per CU)
#define LUMO_FILM_WAVES 4
#endif
__global__ __launch_bounds__(BLOCK, LUMO_FILM_WAVES) void k_finish_film(DScene sc, Paths S0, Tasks T, DCam cam, uint32_t pass0,
                                                        Dump dump, int dump_p, int tone_map, double tone_arg, int t0,
                                                        int npass, int vstride) {
    __shared__ double l_rgb[3 * BLOCK];
    __shared__ double l_ras[2 * BLOCK];
    __shared__ uint32_t l_ok[BLOCK];
    __shared__ double l_wx[(2 * FILM_R + 1) * BLOCK], l_wy[(2 * FILM_R + 1) * BLOCK];
    __shared__ int l_ox[BLOCK], l_oy[BLOCK];  // staged terms: each source's footprint origin in the tile
    const int ti = t0 + (int)blockIdx.x;  // tasks [t0, t0 + gridDim.x)
    const int first = T.first[ti];
    const int P = T.first[ti + 1] - first;
    const int j = threadIdx.x;
    const int s = first + j;
    const int r = (int)ceil(cam.fr - 0.5);
    const bool pre = r <= FILM_R;  // uniform
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (j < P)
        for (int i = 0; i < 4; ++i) acc[i] = S0.film[4 * s + i];
    for (int m = 0; m < npass; ++m) {
        const Paths S = pass_view(S0, m, vstride);
        if (j < P) {
            const bool ok = S.p_valid[s] != 0;
            l_ok[j] = ok ? 1u : 0u;
            l_ox[j] = l_oy[j] = INT_MIN / 4;
            if (ok) {
                const V3 rgb = finish_one(sc, S, cam, s, pass0 + (uint32_t)m, dump, dump_p, tone_map, tone_arg);
                l_rgb[3 * j] = rgb.x;
                l_rgb[3 * j + 1] = rgb.y;
                l_rgb[3 * j + 2] = rgb.z;
                const double rx = S.raster[2 * s], ry = S.raster[2 * s + 1];
                l_ras[2 * j] = rx;
                l_ras[2 * j + 1] = ry;
                if (pre) {  // this sample's column / row terms, as film_gather computes them
                    const double gr = gauss(cam.fr, cam.fsig);
                    const int64_t px = rx > 0.0 ? (int64_t)floor(rx) : 0, py = ry > 0.0 ? (int64_t)floor(ry) : 0;
                    l_ox[j] = (int)(px - r - (int64_t)T.t[ti].px_min[0]);
                    l_oy[j] = (int)(py - r - (int64_t)T.t[ti].px_min[1]);
                    for (int i = 0; i <= 2 * r; ++i) {
                        const double gx = (double)(px - r + i), gy = (double)(py - r + i);
                        l_wx[i * BLOCK + j] = rmax(gauss(rx - (0.5 + gx), cam.fsig) - gr, 0.0);
                        l_wy[i * BLOCK + j] = rmax(gauss(ry - (0.5 + gy), cam.fsig) - gr, 0.0);
                    }
                }
            }
        }
        __syncthreads();
        count_checks(j < P && l_ok[j] ? sample_check(ldc(S.rad, s)) : 0, S.checks);
        const FilmTerms terms{l_wx, l_wy, r};
        if (j < P) {
            if (pre)
                film_gather_staged(acc, T.t[ti], j, l_rgb, l_ox, l_oy, terms);
            else
                film_gather_acc(acc, T.t[ti], cam, j, LdsSrc{l_rgb, l_ras, l_ok});
        }
        __syncthreads();  // the next pass overwrites the staged samples
    }
    if (j < P)
        for (int i = 0; i < 4; ++i) S0.film[4 * s + i] = acc[i];
}

// task.rs:42-53 + 64-69: ring update in pixel order, then delta for the next pass.
// One wave per task.  The pass's samples land in ring slots (ptr + j) % n; when a tile has more
// pixels than ring slots only the last writer of a slot (no j + n < P) stores.  The variance
// sums stay sequential in slot order (lane 0, from LDS) so they round exactly like task.rs.
// `zero_counts` (when set): the pass's queue counters, zeroed by block 0 for the next pass that
// uses them (every kernel of the pass that reads them precedes the ring on its stream), so a pass
// starts without a fill of its own.
__global__ __launch_bounds__(64) void k_ring(DScene sc, Paths S, Tasks T, int n_tasks, int update, uint32_t* zero_counts,
                                             int t0) {
    const int ti = t0 + (int)blockIdx.x;  // tasks [t0, n_tasks)
    if (ti >= n_tasks) return;
    const int lane = threadIdx.x;
    if (zero_counts && blockIdx.x == 0 && lane < CNT_N) zero_counts[lane] = 0u;
    __shared__ double lum[SAMPLES_INCREMENT];
    __shared__ unsigned long long cst[SAMPLES_INCREMENT];
    const lumo_tile_task& t = T.t[ti];
    const int n = (int)t.samples;
    uint64_t* rc = T.ring_cost + (size_t)ti * SAMPLES_INCREMENT;
    double* rl = T.ring_lum + (size_t)ti * SAMPLES_INCREMENT;
    for (int r = lane; r < n; r += 64) {
        lum[r] = rl[r];
        cst[r] = rc[r];
    }
    __syncthreads();
    const int f0 = T.first[ti];
    const int P = T.first[ti + 1] - f0;
    if (update && S.p_valid[f0]) {
        const uint32_t ptr = T.ring_ptr[ti];
        unsigned long long rays = 0, q = 0;
        for (int j = lane; j < P; j += 64) {
            const int sl = f0 + j;
            const uint32_t cost = S.depth[sl];  // sample.cost
            rays += cost;
            q += S.queries[sl];
            if (j + n >= P) {
                const int r = (int)((ptr + (uint32_t)j) % (uint32_t)n);
                lum[r] = luminance(sc, ldc(S.rad, sl), S.lam + 4 * (size_t)sl);  // sample.color.luminance(&lambda)
                cst[r] = cost;
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            rays += __shfl_down(rays, off);
            q += __shfl_down(q, off);
        }
        if (lane == 0) {
            T.num_rays[ti] += rays;
            T.queries[ti] += q;
            T.ring_ptr[ti] = (uint32_t)((ptr + (uint32_t)P) % (uint32_t)n);
        }
        __syncthreads();
        for (int r = lane; r < n; r += 64) {
            rl[r] = lum[r];
            rc[r] = cst[r];
        }
    }
    __syncthreads();
    if (lane == 0) {
        // task.rs:57-63: the three sums are independent chains, each in lumo's slot order, so one
        // loop carries them side by side (the adds of one chain are exactly task.rs's)
        double f = 0.0, f2 = 0.0;
        uint64_t cost = 0;
        for (int i = 0; i < n; ++i) {
            const double l = lum[i];
            f = f + l;
            f2 = f2 + l * l;
            cost += cst[i];
        }
        const double var = f2 - f * f / (double)n;
        const double delta = !(var <= 0.0) ? sqrt(var / (double)cost) : 1e-5;
        T.delta[ti] = delta;
    }
}

// ------------------------------------------------------------------ feature buffers (lumo_render_features)
#include "features.h"

// ------------------------------------------------------------------ BDPT splats -> film taps
// FilmTile::add_sample with splat = true (film/tile.rs:65-111): tone map, XYZ, white balance,
// RGB, then the Gaussian taps over the whole image (not the tile).  MODE 0 counts the taps of
// each slot, 1 writes them from the slot's offset (lumo's order: slot = pixel order within the
// task, tasks in order), 2 adds them into a full-frame film.
template <int MODE>
__global__ __launch_bounds__(BLOCK) void k_bdpt_taps(DScene sc, Paths S, Bdpt B, Bdpt R, DCam cam, int n, int tone_map,
                                                      double tone_arg, uint32_t* cnt, const uint32_t* off,
                                                      lumo_splat* out, double* film) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n) return;
    if (!S.p_valid[slot]) {
        if (MODE == 0) cnt[slot] = 0;
        return;
    }
    const int ri = B.redo_index[slot];  // re-run samples keep their splats in the redo store
    const SplatStore& sp = ri >= 0 ? R.sp : B.sp;
    const int si = ri >= 0 ? ri : slot;
    const int nsp = sp.n[si];
    const uint64_t r = (uint64_t)ceil(cam.fr - 0.5);
    const uint64_t rx = (uint64_t)cam.width, ry = (uint64_t)cam.height;
    const double gr = gauss(cam.fr, cam.fsig);
    uint32_t k = MODE == 1 ? off[slot] : 0u;
    for (int j = 0; j < nsp; ++j) {
        const V2 raster{sp.D(0, j, si), sp.D(1, j, si)};
        V3 rgb{0.0, 0.0, 0.0};
        if (MODE != 0) {
            DColor c;
            double L[NS];
            for (int i = 0; i < NS; ++i) {
                c.s[i] = sp.D(2 + i, j, si);
                L[i] = sp.D(6 + i, j, si);
            }
            rgb = sample_rgb(sc, cam, c, L, tone_map, tone_arg);
        }
        const uint64_t pxx = raster.x > 0.0 ? (uint64_t)floor(raster.x) : 0, pxy = raster.y > 0.0 ? (uint64_t)floor(raster.y) : 0;
        const uint64_t mix = pxx >= r ? pxx - r : 0, miy = pxy >= r ? pxy - r : 0;
        const uint64_t mxx = std::min(pxx + r, rx - 1), mxy = std::min(pxy + r, ry - 1);
        for (uint64_t fy = miy; fy <= mxy; ++fy) {
            for (uint64_t fx = mix; fx <= mxx; ++fx) {
                const double vx = raster.x - (0.5 + (double)fx), vy = raster.y - (0.5 + (double)fy);
                const double wt = rmax(gauss(vx, cam.fsig) - gr, 0.0) * rmax(gauss(vy, cam.fsig) - gr, 0.0);
                if (wt == 0.0) continue;
                if (MODE == 0) {
                    k++;
                } else {
                    const V3 c = rgb * wt;
                    if (MODE == 1) {
                        lumo_splat& o = out[k++];
                        o.x = (uint32_t)fx;
                        o.y = (uint32_t)fy;
                        o.rgb[0] = c.x;
                        o.rgb[1] = c.y;
                        o.rgb[2] = c.z;
                    } else {
                        double* f = film + 3 * (fy * rx + fx);
                        atomicAdd(f, c.x);
                        atomicAdd(f + 1, c.y);
                        atomicAdd(f + 2, c.z);
                    }
                }
            }
        }
    }
    if (MODE == 0) cnt[slot] = k;
}
// first tap of each task in this pass (exclusive scan gathered at the tasks' first slots)
// (tasks t0 .. t0 + n_tasks - 1 whose slots start at s0: cnt / off are that range's, from its first slot)
__global__ void k_task_tap_ranges(Tasks T, const uint32_t* cnt, const uint32_t* off, int n_tasks, int n,
                                  uint64_t* ranges, int t0 = 0, int s0 = 0) {
    const int ti = blockIdx.x * blockDim.x + threadIdx.x;
    if (ti > n_tasks) return;
    ranges[ti] = ti < n_tasks ? (uint64_t)off[T.first[t0 + ti] - s0] : (uint64_t)off[n - 1] + cnt[n - 1];
}

// ------------------------------------------------------------------ PMC calibration (lumo_debug_stream)
// Streams of known byte counts with the access width the path kernels use (8-B f64 per lane,
// coalesced): the rocprofv3 FETCH_SIZE / WRITE_SIZE of these kernels calibrate the counters for
// that width (MI355X_MICROARCH.md: only 16-B/lane streams are calibrated there).
__global__ __launch_bounds__(BLOCK) void k_calib_read8(const double* __restrict__ in, size_t n, double* out) {
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * BLOCK) acc += in[i];
    if (acc == 12345.678) out[blockIdx.x] = acc;  // keeps the loads; never true for the zeroed input
}
__global__ __launch_bounds__(BLOCK) void k_calib_write8(double* __restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * BLOCK) out[i] = (double)i;
}

// ================================================================== host side

int ceil_div(uint64_t a, uint64_t b) { return (int)((a + b - 1) / b); }

// Buffers of a pass set (alloc_pass_set below): the per-pass outputs and counters, the ping-pong
// queues, the closest hits and NEE records, the ray sorting buffers.
enum SetField {
    F_RAD, F_LAM, F_RASTER, F_DEPTH, F_QUERIES, F_P_VALID, F_COUNTS,
    F_QS0_D, F_QS0_R, F_QS0_I, F_QS1_D, F_QS1_R, F_QS1_I,
    F_HQ_T, F_HQ_I, F_SQ_D, F_SQ_I, F_SQ_HD, F_SQ_HI, F_SQ_HR, F_SQ_QL,
    F_SORT_KEYS, F_SORT_ORDER, F_SORT_WS, F_SET_COUNT
};
// Work-buffer carve-out (one allocation per field, grown on demand)
enum WorkId {
    W_RO, W_RD, W_GATH, W_RNG, W_FLAGS, W_TASK, W_PIX, W_PSEED, W_MJRNG, W_MJSTATE, W_PERM,
    W_HIT_T, W_HIT_KIND, W_HIT_OBJ, W_HIT_TRI, W_SH_O, W_SH_D, W_SH_LIGHT, W_P_RGB, W_FILM, W_Q0, W_Q1,
    W_TCOUNT, W_TASKS, W_FIRST, W_RING_COST, W_RING_LUM, W_RING_PTR, W_DELTA, W_NUM_RAYS,
    W_TQUERIES, W_DUMP_RAD, W_DUMP_LAM, W_DUMP_RASTER, W_DUMP_DEPTH, W_DUMP_DELTA,
    W_BD_LD, W_BD_LI, W_BD_CD, W_BD_CI, W_BD_SP, W_BD_SPN, W_BD_OVF, W_BD_CNT, W_BD_OFF,
    W_BD_FILM, W_BD_REDO_INDEX, W_BD_NL, W_BD_NC, W_BD_NITEMS, W_BD_IOFF, W_BD_DRAWS, W_BD_OK, W_BD_ITOTAL, W_BD_PDF,
    W_BD_WDEPTH, W_BD_CAMO, W_BD_CAMD, W_BD_RNG0, W_BD_LAM0, W_BD_NB, W_BD_OFFB,
    W_CHECKS, W_BD_LM, W_BD_LMF, W_BD_CM, W_BD_CMF,
    W_FT_ALB, W_FT_NRM, W_FT_DEP, W_FT_FILM_A, W_FT_FILM_N, W_FT_FILM_D, W_FT_DUMP_I, W_FT_DUMP_D,
    W_SET0,  // pass set k's field f: W_SET0 + k * F_SET_COUNT + f
    W_COUNT = W_SET0 + 4 * F_SET_COUNT
};

template <typename T>
T* wbuf(Ctx& c, int id, size_t count, lumo_status& st) {
    if (c.work.size() < W_COUNT) c.work.resize(W_COUNT);
    const lumo_status s = dev_alloc(c, c.work[id], sizeof(T) * count);
    if (s) st = s;
    return static_cast<T*>(c.work[id].p);
}

struct StageTimer {
    Ctx& c;
    bool on;
    int stage;
    hipStream_t sm;
    hipEvent_t a{}, b{};
    StageTimer(Ctx& cc, bool enable, int st, hipStream_t stream = nullptr)
        : c(cc), on(enable), stage(st), sm(stream ? stream : cc.streams[0]) {
        if (on) {
            a = c.tm.get();
            b = c.tm.get();
            if (!c.ref_recorded) {
                if (!c.ref_ev) (void)hipEventCreate(&c.ref_ev);
                (void)hipEventRecord(c.ref_ev, sm);
                c.ref_recorded = true;
            }
            (void)hipEventRecord(a, sm);
        }
        c.stats.launches[stage] += 1;
    }
    ~StageTimer() {
        if (on) {
            (void)hipEventRecord(b, sm);
            c.tm.pending.push_back({stage, a, b});
        }
    }
};

// Adds the elapsed time of every completed timer pair; pairs still in flight stay pending (the
// end of lumo_render_tiles synchronises, so all are resolved by its last call).
void resolve_timers(Ctx& c) {
    Timing& t = c.tm;
    std::vector<Timing::Pending> still;
    for (auto& p : t.pending) {
        if (hipEventQuery(p.b) != hipSuccess) {
            still.push_back(p);
            continue;
        }
        float ms = 0.f, t0 = 0.f, t1 = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) c.stats.kernel_ms[p.stage] += ms;
        if (c.ref_ev && hipEventElapsedTime(&t0, c.ref_ev, p.a) == hipSuccess &&
            hipEventElapsedTime(&t1, c.ref_ev, p.b) == hipSuccess)
            c.intervals[p.stage].push_back({t0, t1});
        t.free_ev.push_back(p.a);
        t.free_ev.push_back(p.b);
    }
    t.pending.swap(still);
}

// Union length of the launch intervals of the stages in `mask` (ms).
double busy_ms(const Ctx& c, uint32_t mask) {
    std::vector<std::pair<float, float>> iv;
    for (int k = 0; k < LUMO_STAGE_COUNT; ++k)
        if (mask & (1u << k)) iv.insert(iv.end(), c.intervals[k].begin(), c.intervals[k].end());
    std::sort(iv.begin(), iv.end());
    double total = 0.0, lo = 0.0, hi = 0.0;
    bool open = false;
    for (const auto& x : iv) {
        if (open && x.first <= hi) {
            hi = std::max(hi, (double)x.second);
            continue;
        }
        if (open) total += hi - lo;
        lo = x.first;
        hi = x.second;
        open = true;
    }
    if (open) total += hi - lo;
    return total;
}

// Feature-class dispatch (DScene::full: 0 lean, 1 full, 2 full + textures): f(FX) with FX an
// integral_constant, as by_stack_class below.
template <typename F>
void by_fx(int fx, F&& f) {
    if (fx == 2)
        f(std::integral_constant<int, 2>{});
    else if (fx)
        f(std::integral_constant<int, 1>{});
    else
        f(std::integral_constant<int, 0>{});
}

// The (a) items' evaluation: the two trace lists (camera, light connections), then per slot the rest.
void launch_eval_a(int fx, int grid, int grid_slots, hipStream_t sm, const DScene& sc, const Paths& S, const DCam& cam,
                   const Bdpt& B, const Bdpt& R, const BItems& I, int n, const uint32_t* totals) {
    by_fx(fx, [&](auto FX) {
        constexpr int fxc = decltype(FX)::value;
        k_bdpt_eval_a<fxc, 0><<<grid, BLOCK, 0, sm>>>(sc, S, cam, B, R, I, n, totals);
        k_bdpt_eval_a<fxc, 1><<<grid, BLOCK, 0, sm>>>(sc, S, cam, B, R, I, n, totals);
        k_bdpt_eval_a<fxc, 2><<<grid_slots, BLOCK, 0, sm>>>(sc, S, cam, B, R, I, n, totals);
    });
}

// Stack-class dispatch (launch.h STACK_CLASSES).
template <typename F>
void by_stack_class(int cls, F&& f) {
    switch (cls) {
        case 0: f(std::integral_constant<int, 0>{}); break;  // the wide accel's walks (dscene.h wide_walk)
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
        case 16: f(std::integral_constant<int, 16>{}); break;
        case 24: f(std::integral_constant<int, 24>{}); break;
        case 32: f(std::integral_constant<int, 32>{}); break;
        case 48: f(std::integral_constant<int, 48>{}); break;
        default: f(std::integral_constant<int, 64>{}); break;
    }
}

// Traversal launch: stack class x LDS staging.  With LDS staging the grid is capped (persistent
// grid-stride loop) so each workgroup copies the packed scene once per launch.
// allow_top: the kernel has a TOP-staged variant (k_closest_q, k_shadow_q, k_bdpt_vis); it is used
// when the whole scene does not fit in LDS but its top levels were packed at upload (DScene::top).
template <typename F>
void launch_trav(Ctx& c, uint64_t count, F&& f, hipStream_t stream = nullptr, bool allow_top = false) {
    const bool lds = c.o.lds && c.sc.hot_bytes > 0;
    const bool top = !lds && allow_top && c.o.top && c.sc.top_bytes > 0;
    const int grid_full = ceil_div(count, BLOCK);
    TravLaunch l{lds ? std::min(grid_full, (int)c.o.lds_grid) : grid_full, lds ? (size_t)c.sc.hot_bytes : 0, lds,
                 c.sc.full, stream ? stream : c.streams[0]};
    if (top) {
        l.top = true;
        l.grid = std::min(ceil_div(count, TOP_BLOCK), (int)c.o.top_grid);
        l.shm = c.sc.top_shm;
    }
    by_stack_class(c.sc.stack_class, [&](auto K) { f(K, l); });
}

// Ray sorting of the split bounces' closest-hit rays (0: off)
int ray_sort_mode(const Ctx& c) { return c.o.ray_sort >= 0 ? (int)c.o.ray_sort : (c.sc.stack_class >= 32 ? 1 : 0); }

// A pass set: what one unit of passes in flight needs of its own.  Set 0 is the render's own Paths;
// the pipelined schedules run their further units on sets 1..3.  Its buffers, as one list: the
// per-pass outputs and counters (SET_OUT) and the ping-pong queues (SET_QUEUES), of `NV` virtual
// slots (M merged passes' outputs and paths); for the split bounces the closest hits, the NEE
// records and the ray sorting buffers (SET_HITS), of `cap` paths.
enum { SET_OUT = 1, SET_QUEUES = 2, SET_HITS = 4, SET_ALL = 7 };
struct SetRow {
    int field, part;
    size_t size, per_slot, per_cap, fixed;  // elements of `size` bytes: per_slot x NV + per_cap x cap + fixed
};
std::vector<SetRow> set_rows(int ns, bool sort) {
    const size_t pairs = (size_t)NB * (size_t)ns;  // NEE pairs per path: bucket segments of `cap` paths each
    std::vector<SetRow> r = {
        {F_RAD, SET_OUT, 8, 4, 0, 0},       {F_LAM, SET_OUT, 8, 4, 0, 0},     {F_RASTER, SET_OUT, 8, 2, 0, 0},
        {F_DEPTH, SET_OUT, 4, 1, 0, 0},     {F_QUERIES, SET_OUT, 4, 1, 0, 0}, {F_P_VALID, SET_OUT, 4, 1, 0, 0},
        {F_COUNTS, SET_OUT, 4, 0, 0, (size_t)CNT_N * (1 + MAX_MERGE)},  // + the merged passes' queues
        {F_QS0_D, SET_QUEUES, 8, QD_N, 0, 0},  {F_QS0_R, SET_QUEUES, 8, 2, 0, 0},  {F_QS0_I, SET_QUEUES, 4, QI_N, 0, 0},
        {F_QS1_D, SET_QUEUES, 8, QD_N, 0, 0},  {F_QS1_R, SET_QUEUES, 8, 2, 0, 0},  {F_QS1_I, SET_QUEUES, 4, QI_N, 0, 0},
        {F_HQ_T, SET_HITS, 8, 0, 1, 0},     {F_HQ_I, SET_HITS, 4, 0, 3, 0},
        {F_SQ_D, SET_HITS, 8, 0, SD_N * pairs, 0},  {F_SQ_I, SET_HITS, 4, 0, SI_N * pairs, 0},
        {F_SQ_HD, SET_HITS, 8, 0, (size_t)(ns > 1 ? SH_N : SH_N1) * NB, 0},
        {F_SQ_HI, SET_HITS, 4, 0, (size_t)SHI_N * NB, 0}};
    if (ns > 1) {
        r.push_back({F_SQ_HR, SET_HITS, 8, 0, 2 * pairs, 0});
        r.push_back({F_SQ_QL, SET_HITS, 4, 0, SHQ_CLASSES * pairs, 0});
    }
    if (sort) {  // keys and walk order, and the counting sort's workspace (scan.h RS_WORDS)
        r.push_back({F_SORT_KEYS, SET_HITS, 4, 0, 1, 0});
        r.push_back({F_SORT_ORDER, SET_HITS, 4, 0, 1, 0});
        r.push_back({F_SORT_WS, SET_HITS, 4, 0, 0, RS_WORDS});
    }
    return r;
}
// Device bytes of one extra pass set of the split schedule (cap == NV): *fixed + *slot x NV.
void split_set_bytes(const Ctx& c, size_t* slot, size_t* fixed) {
    *slot = *fixed = 0;
    for (const SetRow& r : set_rows(c.sc.n_shadow, ray_sort_mode(c) != 0)) {
        *slot += r.size * (r.per_slot + r.per_cap);
        *fixed += r.size * r.fixed;
    }
}
// Allocates the `parts` of pass set k into Q (its other members are left as they are).
void alloc_pass_set(Ctx& c, Paths& Q, int k, int parts, size_t NV, size_t cap, lumo_status& st) {
    const int ns = c.sc.n_shadow;
    void* p[F_SET_COUNT] = {};
    for (const SetRow& r : set_rows(ns, ray_sort_mode(c) != 0))
        if (r.part & parts)
            p[r.field] = wbuf<char>(c, W_SET0 + k * F_SET_COUNT + r.field,
                                    r.size * (r.per_slot * NV + r.per_cap * cap + r.fixed), st);
    if (parts & SET_OUT) {
        Q.rad = (double*)p[F_RAD];
        Q.lam = (double*)p[F_LAM];
        Q.raster = (double*)p[F_RASTER];
        Q.depth = (uint32_t*)p[F_DEPTH];
        Q.queries = (uint32_t*)p[F_QUERIES];
        Q.p_valid = (uint32_t*)p[F_P_VALID];
        Q.counts = (uint32_t*)p[F_COUNTS];
    }
    if (parts & SET_QUEUES)
        for (int h = 0; h < 2; ++h)
            Q.qs[h] = QState{(double*)p[F_QS0_D + 3 * h], (uint64_t*)p[F_QS0_R + 3 * h],
                             (int32_t*)p[F_QS0_I + 3 * h], NV};
    if (parts & SET_HITS) {
        Q.hq = HitQ{(double*)p[F_HQ_T], (int32_t*)p[F_HQ_I], cap, nullptr, (uint32_t*)p[F_SORT_KEYS],
                    (uint32_t*)p[F_SORT_ORDER], (uint32_t*)p[F_SORT_WS]};
        Q.sq = ShadowQ{};
        Q.sq.seg = (uint32_t)cap;
        Q.sq.hcap = cap * NB;
        Q.sq.cap = Q.sq.hcap * (size_t)ns;
        Q.sq.d = (double*)p[F_SQ_D];
        Q.sq.i = (int32_t*)p[F_SQ_I];
        Q.sq.hd = (double*)p[F_SQ_HD];
        Q.sq.hi = (int32_t*)p[F_SQ_HI];
        Q.sq.hr = (uint64_t*)p[F_SQ_HR];
        Q.sq.ql = (int32_t*)p[F_SQ_QL];
        // the sort's workspace: zeroed here and by every sort's last block
        if (Q.hq.ws && !st && hipMemset(Q.hq.ws, 0, sizeof(uint32_t) * RS_WORDS) != hipSuccess) st = LUMO_ERR_HIP;
    }
}

// Error returns of the multi-stream schedulers: work already queued on the other streams may still
// use the buffers the next call re-initialises on stream 0, so every stream is drained before the
// error is reported.
struct JoinOnError {
    Ctx& c;
    bool ok = false;
    ~JoinOnError() {
        if (ok) return;
        for (int i : {1, 2, 3, 0})
            if (c.streams[i]) (void)hipStreamSynchronize(c.streams[i]);
    }
};

// One render_impl call: the tasks' slots, the plan, the device state and what the schedulers report.
struct Render {
    const lumo_tile_task* tasks;
    size_t n_tasks;
    lumo_tile_result* out;
    Dump* dump_host;  // a path dump (one task): the host arrays, dump_samples passes
    uint64_t dump_samples;
    std::vector<int32_t> first, task_of, pix_of;  // first slot of each task; task and pixel of each slot
    int N = 0, dim_stride = 0;
    uint64_t max_samples = 0, max_P = 0;
    SchedPlan plan{};
    Paths P[4] = {};  // the pass sets; P[0] is the render's own, the others share its per-slot state
    Tasks T{};
    Dump D{};
    int dump_p = 0;
    Bdpt B{};     // subpath vertices (the task groups add their redo lists and stores, render_bdpt_groups)
    BItems BI{};  // connection work items
    uint32_t* items_total = nullptr;
    bool splat_lists = true;
    uint32_t *tap_cnt = nullptr, *tap_off = nullptr;
    double* dfilm = nullptr;
    size_t film_n = 0;
    std::vector<uint64_t> n_splats;
    uint64_t bounces = 0;  // bounces that ran paths, from the count snapshots
    bool features = false;  // a feature render (render_features_impl): camera paths only, no NEE records
};

// Count snapshots of a chain of bounces.  Bounces are enqueued ahead of the host's knowledge of the
// queue counts: each bounce ends with an async copy of its counters into a pinned ring (slots
// [base, base + len) of c.snap) and the host reads the snapshots back as their events complete.
// Launch grids use the last known alive count `ub` as an upper bound (counts never grow within a
// pass); the kernels read the exact counts from device memory.  A segment (a pass, a walk) is
// `done` once a snapshot of it shows no path alive; the bounces enqueued past that point see empty
// queues and exit at once, and their snapshots are consumed for the statistics by a later segment's
// polls or re-recorded.  Snapshots are numbered over all segments; those issued before seg_first
// update neither ub nor done.
struct SnapCursor {
    int base = 0, len = Ctx::SNAP_RING;
    int issued = 0, consumed = 0, seg_first = 0;
    uint32_t ub = 0;
    bool done = false;
    int outstanding() const { return issued - consumed; }
    void begin_segment(uint32_t ub0) {
        seg_first = issued;
        ub = ub0;
        done = false;
    }
    lumo_status record(Ctx& c, const uint32_t* counts, hipStream_t sm) {
        const int slot = base + issued % len;
        HIPCHK(hipMemcpyAsync(c.snap + CNT_N * slot, counts, sizeof(uint32_t) * CNT_N, hipMemcpyDeviceToHost, sm));
        HIPCHK(hipEventRecord(c.snap_ev[slot], sm));
        issued++;
        return LUMO_OK;
    }
    // Takes the snapshots that have arrived, waiting for one while more than `keep` are outstanding
    // (kNoWait: never).
    static constexpr int kNoWait = Ctx::SNAP_RING;
    lumo_status poll(Ctx& c, int keep, uint64_t& bounces) {
        while (consumed < issued && !(done && consumed >= seg_first)) {
            const int slot = base + consumed % len;
            if (issued - consumed > keep) {
                HIPCHK(hipEventSynchronize(c.snap_ev[slot]));
            } else if (hipEventQuery(c.snap_ev[slot]) != hipSuccess) {
                break;
            }
            const uint32_t* k = c.snap + CNT_N * slot;
            bounces += k[CNT_CUR] > 0 ? 1 : 0;
            if (consumed >= seg_first) {
                ub = k[CNT_NEXT];
                done = ub == 0;
            }
            consumed++;
        }
        return LUMO_OK;
    }
};

// Film of a unit's `mu` passes from `pass0` (pass m's per-slot outputs `stride` virtual slots after
// pass m - 1's in P) for tasks [t0, t1) whose tiles hold at most BLOCK pixels: one block per tile
// (lumo's 16x16 tiles), the passes in pass order.
void film_tiles(Ctx& c, const Render& R, hipStream_t sm, const Paths& P, uint64_t pass0, int mu, int stride, int t0,
                int t1) {
    StageTimer tm(c, c.o.timing, ST_FILM, sm);
    k_finish_film<<<t1 - t0, BLOCK, 0, sm>>>(c.sc, P, R.T, c.cam, (uint32_t)pass0, R.D, R.dump_p, c.tone_map, c.tone_arg,
                                             t0, mu, stride);
}
// Film of one pass (per-slot outputs V) for slots [s0, s1): tiles of any size.
void film_large(Ctx& c, const Render& R, hipStream_t sm, const Paths& V, uint64_t pass, int s0, int s1) {
    const int g = ceil_div(s1 - s0, BLOCK);
    {
        StageTimer tm(c, c.o.timing, ST_FINISH, sm);
        k_finish<<<g, BLOCK, 0, sm>>>(c.sc, V, c.cam, s1, (uint32_t)pass, R.D, R.dump_p, c.tone_map, c.tone_arg, s0);
    }
    StageTimer tm(c, c.o.timing, ST_FILM, sm);
    k_film<<<g, BLOCK, 0, sm>>>(V, R.T, c.cam, s1, s0);
}

// A merged unit's queue `head` of n_head paths after its head bounces, split by pass into segments
// of `other` (the other ping-pong queue), each with counters of its own after the unit's.
void split_merged_head(hipStream_t sm, const Paths& P, const QState& head, const QState& other, uint64_t n_head, int N,
                       int mu) {
    ZeroList z;
    z.add(P.counts + CNT_N, sizeof(uint32_t) * CNT_N * (size_t)mu);
    k_zero_list<<<1, BLOCK, 0, sm>>>(z);
    k_split_passes<<<std::min(ceil_div(n_head, BLOCK), 4096), BLOCK, 0, sm>>>(head, other, P.counts, N, mu);
}

// One fused bounce (pt.h k_bounce_q) over at most `count` paths of queue `cur`; tail: the tail
// kernel, which runs the paths of a queue shorter than `skip` to their end.
void launch_fused_bounce(Ctx& c, hipStream_t sm, const Paths& P, const Tasks& T, const QState& cur, const QState& nxt,
                         uint64_t count, uint32_t skip, bool tail) {
    launch_trav(
        c, count,
        [&](auto K, const TravLaunch& l) {
            launch_bounce_q<decltype(K)::value>(l, c.sc, P, T, cur, nxt, skip, tail, tail ? 0 : (int)c.o.dyn,
                                                tail ? BLOCK : (int)c.o.bounce_threads);
        },
        sm);
}

// Pipelined passes (n_shadow == 1, fused bounces).  Russian roulette reads the pass's adaptive
// delta only from depth RR_DEPTH on (path_trace.rs:60-69), and that delta needs the previous
// pass's film + ring.  So on a head stream each unit runs its camera and its first bounces as
// fused launches, then hands its queue to stream B, which runs the tail kernel (every remaining
// path to its end), the film and the ring; meanwhile the next unit starts.  The latency-bound
// tail, film and ring of one unit thus overlap the heavy first bounces of the next.
//
// A unit is M consecutive passes (merged passes; M = 1 on a full frame).  Its camera kernel
// generates every slot's samples of those passes in pass order and its head bounces run all of
// their paths as one queue (M times the paths per launch: a rank's share of a multi-GPU frame
// holds a few hundred thousand slots per pass, too few to keep the GPU busy).  With M > 1 the
// head bounces stop before RR_DEPTH, so they read no delta; stream B then runs the unit's tails
// pass by pass (the tail kernel takes only that pass's virtual slots), each followed by the
// pass's film and ring, so every pass's Russian roulette sees the delta of the ring before it.
//
// NA head streams (1 to 3) rotate over the units, so consecutive units' first bounces also run
// concurrently; NA + 1 sets of queues, counters and per-slot outputs, a set reused only after
// the unit NA + 1 back has issued its ring.  Every per-path operation and every film / ring sum
// is the one the sequential loop performs, in the same order: bit-identical.
lumo_status render_pipelined(Ctx& c, Render& R) {
    const Tasks& T = R.T;
    const Dump& D = R.D;
    const int N = R.N, n_tasks = (int)R.n_tasks, M = R.plan.M, heads = R.plan.head_bounces, bb = R.plan.tail_bounces;
    const uint64_t max_samples = R.max_samples;
    const bool tiles = R.max_P <= BLOCK;  // one film block per tile
    const int NA = R.plan.head_streams, NSETS = NA + 1;
    JoinOnError join{c};
    Paths* P3 = R.P;
    hipStream_t As[3] = {c.streams[0], c.streams[2], c.streams[3]};
    hipStream_t B = c.streams[1];
    hipStream_t F = NA <= 2 ? c.streams[3] : B;  // the films (four streams: the device's hardware queues)
    // each set's counters start zeroed; from then on every unit's last ring zeroes its set's counters
    {
        ZeroList z;
        for (int k = 1; k < NSETS; ++k) z.add(P3[k].counts, sizeof(uint32_t) * CNT_N);
        k_zero_list<<<1, BLOCK, 0, As[0]>>>(z);
    }
    // every event starts "done" after the setup enqueued on stream 0 (tasks, zeroing, the initial
    // ring): unit u waits for unit u - NSETS's ring and film before reusing its set, for unit u - 1's
    // camera (the sampler state is per slot) and, before a bounce RR_DEPTH, for unit u - 1's ring
    for (int k = 0; k < 4; ++k) {
        HIPCHK(hipEventRecord(c.pass_ev[k], As[0]));
        HIPCHK(hipEventRecord(c.cam_ev[k], As[0]));
        HIPCHK(hipEventRecord(c.film_ev[k], As[0]));
    }
    HIPCHK(hipStreamWaitEvent(B, c.pass_ev[0], 0));
    const int gN = ceil_div(N, BLOCK);
    const uint64_t units = (max_samples + (uint64_t)M - 1) / (uint64_t)M;
    for (uint64_t u = 0; u < units; ++u) {
        const uint64_t p0 = u * (uint64_t)M;
        const int mu = (int)std::min<uint64_t>((uint64_t)M, max_samples - p0);  // passes of this unit
        const int set = (int)(u % NSETS), prev = (int)((u + NSETS - 1) % NSETS);
        hipStream_t A = As[u % NA];
        Paths& P = P3[set];
        // ---- head stream: camera + the first bounces of the unit's passes
        HIPCHK(hipStreamWaitEvent(A, c.pass_ev[set], 0));  // unit u - NSETS done with this set (its ring zeroed the counters)
        HIPCHK(hipStreamWaitEvent(A, c.film_ev[set], 0));  // ... and its film
        if (NA > 1) HIPCHK(hipStreamWaitEvent(A, c.cam_ev[prev], 0));  // the previous unit's camera
        {
            StageTimer tm(c, c.o.timing, ST_CAMERA, A);
            k_camera<true><<<gN, BLOCK, 0, A>>>(T, P, c.cam, N, R.dim_stride, (uint32_t)p0, 0, mu, N);
        }
        HIPCHK(hipEventRecord(c.cam_ev[set], A));
        for (int b = 0; b < heads; ++b) {
            if (b == RR_DEPTH) HIPCHK(hipStreamWaitEvent(A, c.pass_ev[prev], 0));  // this pass's delta (M == 1)
            k_bounce_begin<<<1, 64, 0, A>>>(P.counts, P.tcount + TC_HEADQ);
            StageTimer tm(c, c.o.timing, ST_CLOSEST, A);
            launch_fused_bounce(c, A, P, T, P.qs[b & 1], P.qs[(b + 1) & 1], (uint64_t)N * mu, 0u, false);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c.tail_ev[set], A));
        // ---- stream B: per pass, the rest of its paths, its film and its ring
        HIPCHK(hipStreamWaitEvent(B, c.tail_ev[set], 0));
        // the unit's queue split by pass (M > 1) into segments of the other ping-pong queue, each
        // with counters of its own; then per pass: tail_bounces more fused bounces over its paths
        // (past Russian roulette, after the previous pass's ring on this stream), the tail kernel
        // for the rest, the ring
        const QState& Qh = P.qs[heads & 1];
        const QState& Qs = P.qs[(heads + 1) & 1];
        if (mu > 1) split_merged_head(B, P, Qh, Qs, (uint64_t)N * mu, N, mu);
        for (int m = 0; m < mu; ++m) {
            const uint64_t pass = p0 + (uint64_t)m;
            Paths V = pass_view(P, m, N);
            Paths Pm = P;  // this pass's paths: its own counters, its queue segment (virtual slots)
            Pm.counts = mu > 1 ? P.counts + (size_t)(1 + m) * CNT_N : P.counts;
            const QState q0 = mu > 1 ? segment(Qs, m, N) : Qh, q1 = mu > 1 ? segment(Qh, m, N) : Qs;
            if (D.delta) HIPCHK(hipMemcpyAsync(D.delta + pass, T.delta, sizeof(double), hipMemcpyDeviceToDevice, B));
            for (int b = 0; b < bb; ++b) {
                k_bounce_begin<<<1, 64, 0, B>>>(Pm.counts, P.tcount + TC_HEADQ);
                StageTimer tm(c, c.o.timing, ST_CLOSEST, B);
                launch_fused_bounce(c, B, Pm, T, (b & 1) ? q1 : q0, (b & 1) ? q0 : q1, (uint64_t)N, 0u, false);
            }
            k_bounce_begin<<<1, 64, 0, B>>>(Pm.counts, P.tcount + TC_HEADQ);
            {
                StageTimer tm(c, c.o.timing, ST_RESOLVE, B);
                launch_fused_bounce(c, B, Pm, T, (bb & 1) ? q1 : q0, (bb & 1) ? q0 : q1, (uint64_t)N, 0xffffffffu,
                                    true);
            }
            // the ring (which computes the samples' luminance itself): the next pass's Russian
            // roulette waits for it; the film is off that chain (film_first: the unit's film before
            // its last ring when they share stream B)
            if (tiles && F == B && c.o.film_first && m == mu - 1) film_tiles(c, R, B, P, p0, mu, N, 0, n_tasks);
            {
                StageTimer tm(c, c.o.timing, ST_RING, B);
                k_ring<<<n_tasks, 64, 0, B>>>(c.sc, V, T, n_tasks, 1, m == mu - 1 ? P.counts : nullptr, 0);
            }
            HIPCHK(hipGetLastError());
            if (!tiles) film_large(c, R, B, V, pass, 0, N);  // tiles larger than a block: per pass, on B
        }
        HIPCHK(hipEventRecord(c.pass_ev[set], B));
        // the film of the unit's passes, one launch in pass order (after the previous unit's film on
        // the same stream), on a stream of its own when one is free
        if (tiles && !(F == B && c.o.film_first)) {
            if (F != B) HIPCHK(hipStreamWaitEvent(F, c.pass_ev[set], 0));
            film_tiles(c, R, F, P, p0, mu, N, 0, n_tasks);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipEventRecord(c.film_ev[set], tiles ? F : B));
        if (c.o.timing) resolve_timers(c);
    }
    // the results are copied on stream 0: after every set's last unit and film
    for (int k = 0; k < NSETS; ++k) {
        HIPCHK(hipStreamWaitEvent(As[0], c.pass_ev[k], 0));
        HIPCHK(hipStreamWaitEvent(As[0], c.film_ev[k], 0));
    }
    join.ok = true;
    return LUMO_OK;
}

// One path-tracing bounce of the split (not fused-LDS) schedule on stream `sm`: the tail kernel when
// few paths are alive (n_shadow == 1), then the fused bounce (fused_now) or closest hit -> shading
// (+ NEE pair generation when n_shadow > 1) -> visibility (+ the NEE fold).  `ub` is an upper bound
// on the live count (grids); the kernels read the exact count from S.counts.  allow_tail = false:
// the bounce must not run paths through Russian roulette (a merged head, which reads no delta).
constexpr uint32_t kSortMin = 1u << 15;  // ray sorting only for bounces with at least this many rays
void issue_split_bounce(Ctx& c, const Paths& S, const Tasks& T, const QState& cur, const QState& nxt, uint32_t ub,
                        hipStream_t sm, bool fused_now, bool allow_tail = true) {
    const int ns = c.sc.n_shadow;
    // n_shadow == 1: the tail kernel takes the bounce when fewer than c.o.tail_below paths are alive
    // (decided on the device from the exact count); the bounce kernels skip it.  (A tail kernel for
    // n_shadow > 1, each thread tracing its path's 2 x n_shadow visibility rays per bounce in turn,
    // made C3's 1/8 share 720 -> 1 300-2 460 ms at thresholds 2^12-2^16: rejected, round 5)
    // (launched only once the last count the host has seen is below 4x the threshold:
    // before that the bounce kernels get threshold 0 and take every path)
    const uint32_t skip = (allow_tail && ns == 1 && (uint64_t)ub < 4ull * c.o.tail_below) ? (uint32_t)c.o.tail_below : 0u;
    if (skip > 0) {
        StageTimer tm(c, c.o.timing, ST_RESOLVE, sm);
        launch_fused_bounce(c, sm, S, T, cur, nxt, std::min(ub, skip), skip, true);
    }
    if (fused_now) {  // one fused kernel per bounce (pt.h k_bounce_q)
        StageTimer tm(c, c.o.timing, ST_CLOSEST, sm);
        launch_fused_bounce(c, sm, S, T, cur, nxt, ub, skip, false);
        return;
    }
    {   // the closest hits; with ray sorting, the rays' sort order first (timed as one closest-hit launch)
        Paths Sc = S;
        StageTimer tm(c, c.o.timing, ST_CLOSEST, sm);
        const int sort_mode = ray_sort_mode(c);
        if (sort_mode && S.hq.keys && ub >= kSortMin && (uint64_t)ub <= S.hq.cap) {
            const int g = ceil_div(ub, RS_BLOCK);
            k_rsort_keys<<<g, RS_BLOCK, 0, sm>>>(cur, S.counts, ub, c.sort_lo, c.sort_scale, sort_mode, S.hq.keys,
                                                 S.hq.ws);
            k_rsort_scatter<<<g, RS_BLOCK, 0, sm>>>(S.hq.keys, S.counts, ub, S.hq.ws, S.hq.order);
            Sc.hq.perm = S.hq.order;
            c.stats.sorted_bounces += 1;
        }
        launch_trav(
            c, ub, [&](auto K, const TravLaunch& l) { launch_closest_q<decltype(K)::value>(l, c.sc, Sc, cur, skip); },
            sm, true);
    }
    {
        StageTimer tm(c, c.o.timing, ST_SHADE, sm);
        const int g = ceil_div(ub, BLOCK);
        if (ns > 1) {  // NEE pairs by k_nee_gen, one thread per pair
            const int gp = std::min(ceil_div((uint64_t)ub * (uint32_t)ns, BLOCK), 1 << 16);
            by_fx(c.sc.full, [&](auto FX) {
                k_shade_q<decltype(FX)::value, true><<<g, BLOCK, 0, sm>>>(c.sc, S, T, cur, nxt, skip);
                k_nee_gen<decltype(FX)::value><<<gp, BLOCK, 0, sm>>>(c.sc, S);
            });
        } else {
            by_fx(c.sc.full, [&](auto FX) {
                k_shade_q<decltype(FX)::value, false><<<g, BLOCK, 0, sm>>>(c.sc, S, T, cur, nxt, skip);
            });
        }
    }
    {
        StageTimer tm(c, c.o.timing, ST_SHADOW, sm);
        // n_shadow > 1: one thread per visibility query (the records that need a walk, k_nee_gen)
        launch_trav(
            c, (uint64_t)ub * (uint32_t)ns * (ns > 1 ? 2u : 1u),
            [&](auto K, const TravLaunch& l) { launch_shadow_q<decltype(K)::value>(l, c.sc, S, nxt); }, sm,
            true);
    }
    if (ns > 1) {
        StageTimer tm(c, c.o.timing, ST_RESOLVE, sm);
        k_nee_fold<<<std::min(ceil_div(ub, BLOCK), 1 << 14), BLOCK, 0, sm>>>(S, nxt, ns);
    }
}

// Pipelined passes of the split schedule (closest hit / shading / visibility kernels: scenes too
// large for the fused LDS kernel, n_shadow > 1).  A pass whose queue has shrunk to a few thousand
// paths runs latency-bound launches (one long walk sets a kernel's duration: C3 at one rank's 1/8
// share spent ~0.4 ms per closest / visibility launch for every bounce past the fifth), so several
// units run at once on their own streams and pass sets (queues, counters, hits, NEE records,
// per-slot outputs).
//
// Russian roulette reads a task's adaptive delta from depth RR_DEPTH on (path_trace.rs:60-69) and
// the delta of pass p needs the film and ring of pass p - 1 *of the same task* (task.rs:28-53); the
// sampler state is per slot.  So the tasks are cut into G groups of consecutive tasks (about equal
// slots) whose pass chains are independent, and the units of work are (group g, passes p0 ..
// p0 + mu - 1), issued in the order n = u * G + g on pass set / stream n % K (K >= G).
//
// Merged passes (M > 1: a pass holds few paths, e.g. one rank's share of a multi-GPU frame): the
// unit's camera generates the samples of its mu passes in pass order into one queue (pass m's
// per-slot outputs at virtual slots s + m N), and its first RR_DEPTH bounces (the head, which reads
// no delta) run them as one queue, mu times the paths per launch.  k_split_passes then cuts the
// queue into one segment per pass, each with its own counters, and the passes run their remaining
// bounces one after the other, each followed by its ring: every pass's Russian roulette sees the
// delta of the ring before it.  One film launch takes the unit's passes in pass order.
//
// Unit (g, u) waits for unit (g, u - 1)'s camera before its own, and for its last ring before the
// first bounce that reads the delta: bounce RR_DEPTH of a one-pass unit (or any bounce that may run
// the tail kernel: n_shadow == 1, it takes paths through Russian roulette), the first per-pass
// bounce of a merged unit; and for its film before its own film.  Set reuse (unit n + K, started
// once unit n has issued its last ring) is ordered by its stream.  The host runs every in-flight
// unit's bounce loop (count snapshots `ahead` launches back, as the sequential loop), blocks only on
// the oldest unit, which never waits for a unit the host has not finished issuing, and enqueues
// every wait after the record it waits for.  Every per-path operation and every film / ring sum of
// a task is the sequential loop's, in the same order: bit-identical.
lumo_status render_split_pipelined(Ctx& c, Render& R) {
    const Tasks& T = R.T;
    const int N = R.N, K = R.plan.K, G = R.plan.G, M = R.plan.M;
    const uint64_t max_samples = R.max_samples;
    const bool fused_now = R.plan.fused;
    const std::vector<int32_t>& first = R.first;
    uint64_t& bounces = R.bounces;
    JoinOnError join{c};
    const int ns = c.sc.n_shadow;
    const std::vector<std::pair<int, int>> groups = task_groups(first.data(), (int)R.n_tasks, N, G);
    Paths* P = R.P;
    {
        ZeroList z;
        for (int k = 1; k < K; ++k) z.add(P[k].counts, sizeof(uint32_t) * CNT_N);
        if (z.n) k_zero_list<<<1, BLOCK, 0, c.streams[0]>>>(z);
    }
    for (int k = 0; k < 4; ++k) {
        HIPCHK(hipEventRecord(c.pass_ev[k], c.streams[0]));
        HIPCHK(hipEventRecord(c.film_ev[k], c.streams[0]));
    }
    // The render's setup (task and pixel tables, seeds, sampler permutations, the initial ring) and
    // the sets' counter zeroing ran on stream 0: every other stream waits for them before its first
    // unit (a pass-0 unit waits for nothing else).  Without this wait a unit on another stream
    // could start on stale counters and tables: found by poisoning fresh buffers (LUMO_POISON).
    for (int k = 1; k < K; ++k) HIPCHK(hipStreamWaitEvent(c.streams[k], c.pass_ev[0], 0));
    const int SEG = Ctx::SNAP_RING / 4;  // snapshot slots per set
    const int ahead = std::max(1, std::min((int)c.o.bounce_ahead, SEG - 1));
    // A unit's bounce loops: seg -1 the merged head (mu > 1), then seg m = its pass m (a one-pass unit
    // starts at seg 0 with its head included).  Snapshots are numbered over the whole unit; those of an
    // earlier segment are consumed for the statistics only.
    struct PS {
        uint64_t unit, pass0;
        int g, set, mu, seg;
        int seg_issued, head_issued;
        bool waited;
        SnapCursor s;
    };
    std::deque<PS> act;
    std::vector<uint64_t> finished(G, 0);  // passes of each group whose last ring has been issued
    const uint64_t per_group = (max_samples + (uint64_t)M - 1) / (uint64_t)M;
    const uint64_t units = per_group * (uint64_t)G;
    uint64_t next = 0;
    auto group_slots = [&](int g) { return (uint32_t)(first[groups[g].second] - first[groups[g].first]); };
    auto start = [&]() -> lumo_status {
        const int set = (int)(next % K), g = (int)(next % G);
        const uint64_t pass0 = (next / G) * (uint64_t)M;
        const int mu = (int)std::min<uint64_t>((uint64_t)M, max_samples - pass0);
        hipStream_t sm = c.streams[set];
        const int s0 = first[groups[g].first], s1 = first[groups[g].second];
        if (pass0 > 0) HIPCHK(hipStreamWaitEvent(sm, c.cam_ev[(next - G) % K], 0));  // sampler state per slot
        {
            StageTimer tm(c, c.o.timing, ST_CAMERA, sm);
            k_camera<true><<<ceil_div(s1 - s0, BLOCK), BLOCK, 0, sm>>>(T, P[set], c.cam, s1, R.dim_stride,
                                                                        (uint32_t)pass0, s0, mu, N);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c.cam_ev[set], sm));
        PS ps{next, pass0, g, set, mu, mu > 1 ? -1 : 0, 0, 0, pass0 == 0, SnapCursor{set * SEG, SEG}};
        ps.s.begin_segment(group_slots(g) * (uint32_t)mu);
        act.push_back(ps);
        next++;
        return LUMO_OK;
    };
    auto ready = [&](const PS& ps) { return ps.waited || finished[ps.g] >= ps.pass0; };
    auto wait_prev = [&](PS& ps) -> lumo_status {  // unit (g, u - 1)'s last ring, already issued
        if (!ps.waited) HIPCHK(hipStreamWaitEvent(c.streams[ps.set], c.pass_ev[(ps.unit - G) % K], 0));
        ps.waited = true;
        return LUMO_OK;
    };
    // the tail kernel (n_shadow == 1, launched once few paths are alive) runs paths to their end,
    // through Russian roulette, in whatever bounce it is launched: such a bounce needs the delta too
    auto tail_possible = [&](const PS& ps) {
        return ns == 1 && c.o.tail_below > 0 && (uint64_t)ps.s.ub < 4ull * c.o.tail_below;
    };
    // the queues and counters of the unit's current segment
    auto seg_paths = [&](const PS& ps) {
        Paths Q = P[ps.set];
        if (ps.seg >= 0 && ps.mu > 1) Q.counts = P[ps.set].counts + (size_t)(1 + ps.seg) * CNT_N;
        return Q;
    };
    auto seg_queue = [&](const PS& ps, int parity) {
        const Paths& Q = P[ps.set];
        if (ps.seg < 0 || ps.mu == 1) return Q.qs[parity];
        // pass m's paths: segment m of the queue k_split_passes wrote (the other parity than the head's last)
        return segment(Q.qs[(ps.head_issued + 1 + parity) & 1], ps.seg, N);
    };
    // bounce of the current segment: a merged head never reads the delta (no tail kernel); every
    // per-pass bounce of a merged unit does (depth >= RR_DEPTH)
    auto needs_delta = [&](const PS& ps) {
        if (ps.seg < 0) return false;
        return ps.mu > 1 || ps.seg_issued >= RR_DEPTH || tail_possible(ps);
    };
    auto issue = [&](PS& ps) -> lumo_status {
        hipStream_t sm = c.streams[ps.set];
        if (needs_delta(ps)) {
            const lumo_status w = wait_prev(ps);
            if (w) return w;
        }
        Paths Q = seg_paths(ps);
        k_bounce_begin<<<1, 64, 0, sm>>>(Q.counts, Q.tcount + TC_HEADQ);
        issue_split_bounce(c, Q, T, seg_queue(ps, ps.seg_issued & 1), seg_queue(ps, (ps.seg_issued + 1) & 1), ps.s.ub,
                           sm, fused_now, ps.seg >= 0);
        HIPCHK(hipGetLastError());
        const lumo_status e = ps.s.record(c, Q.counts, sm);
        if (e) return e;
        ps.seg_issued++;
        if (ps.seg < 0) ps.head_issued++;
        return LUMO_OK;
    };
    // the merged head is over (RR_DEPTH bounces, or no path left): its queue split by pass
    auto split = [&](PS& ps) -> lumo_status {
        hipStream_t sm = c.streams[ps.set];
        const Paths& Q = P[ps.set];
        split_merged_head(sm, Q, Q.qs[ps.head_issued & 1], Q.qs[(ps.head_issued + 1) & 1],
                          (uint64_t)group_slots(ps.g) * (uint64_t)ps.mu, N, ps.mu);
        HIPCHK(hipGetLastError());
        ps.seg = 0;
        ps.seg_issued = 0;
        ps.s.begin_segment(group_slots(ps.g));
        return LUMO_OK;
    };
    // the ring of the segment's pass (task.rs:28-69, from the pass's final radiance); after the
    // unit's last pass its film (after the group's previous film: the film accumulates in pass order)
    auto finish = [&](PS& ps) -> lumo_status {
        hipStream_t sm = c.streams[ps.set];
        const Paths& Q = P[ps.set];
        const int t0 = groups[ps.g].first, t1 = groups[ps.g].second, s0 = first[t0], s1 = first[t1];
        const lumo_status w = wait_prev(ps);
        if (w) return w;
        const int m = ps.seg;
        const bool last = m == ps.mu - 1;
        {
            StageTimer tm(c, c.o.timing, ST_RING, sm);
            k_ring<<<t1 - t0, 64, 0, sm>>>(c.sc, pass_view(Q, m, N), T, t1, 1, last ? Q.counts : nullptr, t0);
        }
        HIPCHK(hipGetLastError());
        if (!last) {  // the unit's next pass: its bounces follow this ring on the stream
            ps.seg = m + 1;
            ps.seg_issued = 0;
            ps.s.begin_segment(group_slots(ps.g));
            return LUMO_OK;
        }
        HIPCHK(hipEventRecord(c.pass_ev[ps.set], sm));
        if (ps.pass0 > 0) HIPCHK(hipStreamWaitEvent(sm, c.film_ev[(ps.unit - G) % K], 0));
        if (R.max_P <= BLOCK)
            film_tiles(c, R, sm, Q, ps.pass0, ps.mu, N, t0, t1);
        else
            for (int k = 0; k < ps.mu; ++k) film_large(c, R, sm, pass_view(Q, k, N), ps.pass0 + (uint64_t)k, s0, s1);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c.film_ev[ps.set], sm));
        finished[ps.g] = ps.pass0 + (uint64_t)ps.mu;
        ps.seg = ps.mu;  // unit complete
        if (c.o.timing) resolve_timers(c);
        return LUMO_OK;
    };
    // unit n reuses the set of unit n - K: it starts once that unit has issued its last ring (units
    // of different groups finish out of order, so a free slot in `act` does not mean a free set)
    auto set_free = [&](int set) {
        for (const PS& ps : act)
            if (ps.set == set) return false;
        return true;
    };
    lumo_status e = LUMO_OK;
    while (next < units || !act.empty()) {
        bool progress = false;
        if ((int)act.size() < K && next < units && set_free((int)(next % K))) {
            if ((e = start())) return e;
            progress = true;
        }
        for (size_t i = 0; i < act.size(); ++i) {
            PS& ps = act[i];
            if ((e = ps.s.poll(c, SnapCursor::kNoWait, bounces))) return e;
            if (ps.seg < 0) {  // merged head: RR_DEPTH bounces, then the split
                if (ps.s.done || ps.seg_issued == RR_DEPTH) {
                    if ((e = split(ps))) return e;
                    progress = true;
                } else if (ps.s.outstanding() < ahead) {
                    if ((e = issue(ps))) return e;
                    progress = true;
                }
                continue;
            }
            if (ps.s.done) {
                if (ready(ps)) {  // the group's previous unit has issued its last ring
                    if ((e = finish(ps))) return e;
                    progress = true;
                    if (ps.seg == ps.mu) {
                        act.erase(act.begin() + (std::ptrdiff_t)i);
                        break;
                    }
                }
                continue;
            }
            // a bounce that reads the delta waits until the group's previous unit has issued its ring
            const bool may = !needs_delta(ps) || ready(ps);
            if (may && ps.s.outstanding() < ahead) {
                if ((e = issue(ps))) return e;
                progress = true;
            }
        }
        if (!progress) {
            PS& f = act.front();  // the oldest unit waits for nothing the host has not issued: its next snapshot
            if ((e = f.s.poll(c, f.s.outstanding() - 1, bounces))) return e;
        }
    }
    // the results are copied on stream 0: after every set's last unit
    for (int k = 1; k < K; ++k) {
        HIPCHK(hipStreamWaitEvent(c.streams[0], c.pass_ev[k], 0));
        HIPCHK(hipStreamWaitEvent(c.streams[0], c.film_ev[k], 0));
    }
    join.ok = true;
    return LUMO_OK;
}

// BDPT, the one pass body of the bidirectional integrator (bdpt.h): light subpaths, then camera
// subpaths, bounce by bounce through k_closest + k_bdpt_step (k_bdpt_tail ahead of them once few
// subpaths are alive); re-runs of the samples that did not fit; connection items; fold; film, ring
// and splat taps.  Stage slots: walks = CLOSEST + SHADE, re-runs + fold = RESOLVE.
//
// The tasks are cut into G groups of consecutive tasks (G = 1: one chain on stream 0, also what a
// path dump runs, its Dump `D` written by the film kernels), each rendered as its own chain of
// passes on its own stream, with its own view
// of the per-slot buffers (offset to its first slot), its own walk queues, counters, redo list and
// store, connection item lists and scan storage.  lumo's adaptive Russian roulette reads a task's
// delta in the walks (path_gen.rs:133-145) and the delta of pass p needs that task's ring of pass
// p - 1 (task.rs:28-53): within a group the passes follow one another on the group's stream;
// groups share nothing but the scene, the task table and the splat film
// (atomics: its sum order is unspecified anyway), so their chains overlap freely: one group's
// latency-bound walk tails and connection traces run beside the other's item kernels.  The host
// drives every group's pass as a state machine (walk bounces issued `ahead` of their count
// snapshots; the item totals read back through pinned memory when their event completes), so it
// waits for nothing a group needs.  Every per-sample operation, every item and every film / ring
// sum of a task is the same for every G, in the same order: bit-identical.  (Per-task splat lists,
// the test / library path, are read back with a blocking wait per pass.)
enum BdPhase { BD_LIGHT = 0, BD_CAMERA, BD_TOTALS, BD_DONE };
struct BdGroup {
    int t0, t1, s0, n;
    hipStream_t sm;
    Paths S;
    Bdpt B, R;
    BItems I;
    uint32_t* totals;  // device: (a), (b) item totals of the pass
    uint64_t pass = 0;
    int phase = BD_LIGHT;
    SnapCursor s;  // the walks' count snapshots
    int walk = 0;  // bounces of the current walk
    bool sort_ws_zeroed = false;  // the walk sort's workspace (zeroed once, then by every sort)
};

// Per-group work buffers (k: BdBuf), grown on demand like the render's own.
enum BdBuf { BG_TERM_A, BG_TERM_B, BG_BLIST, BG_AT, BG_AKIND, BG_AOBJ, BG_ATRI, BG_ALIST, BG_SCAN, BG_RANGES, BG_TAPS,
             BG_RLD, BG_RLI, BG_RCD, BG_RCI, BG_RSP, BG_RSPN, BG_RDRAWS, BG_ROK, BG_RLM, BG_RLMF, BG_RCM, BG_RCMF,
             BG_REDO, BG_SK0, BG_SV0, BG_STMP, BG_COUNT };
template <typename T>
T* gbuf(Ctx& c, int g, int k, size_t count, lumo_status& st) {
    if (c.gwork.size() < (size_t)4 * BG_COUNT) c.gwork.resize((size_t)4 * BG_COUNT);
    const lumo_status s = dev_alloc(c, c.gwork[(size_t)g * BG_COUNT + k], sizeof(T) * count);
    if (s) st = s;
    return static_cast<T*>(c.gwork[(size_t)g * BG_COUNT + k].p);
}

// A store of `n` slots carved out of one of `total` slots at slot s0 (every plane is (fields x V) x
// slots with the slot index innermost of the (v, slot) pair, so a group's range is contiguous).
VStore vstore_part(const VStore& v, int s0, int n) {
    const size_t o = (size_t)v.V * (size_t)s0;
    return VStore{v.d + o * VD_N, v.i + o * VI_N, v.V, n, v.m + 2 * o, v.mf + o};
}

// The view of slots s0 .. of the per-slot state: every per-slot pointer offset to slot s0 (a range of
// consecutive slots is contiguous in every buffer).
Paths slot_view(const Paths& S, int s0, int dim_stride) {
    Paths P = S;
    const size_t o = (size_t)s0;
    auto at = [o](auto*& p, size_t per_slot) { p += per_slot * o; };
    at(P.ro, 3), at(P.rd, 3), at(P.gath, 4), at(P.rad, 4), at(P.lam, 4), at(P.raster, 2), at(P.rng, 2);
    at(P.depth, 1), at(P.flags, 1), at(P.queries, 1), at(P.task, 1), at(P.pix, 1), at(P.pseed, 1);
    at(P.mj_rng, 2), at(P.mj_state, 1), at(P.perm, 2 * (size_t)dim_stride);
    at(P.hit_t, 1), at(P.hit_kind, 1), at(P.hit_obj, 1), at(P.hit_tri, 1);
    at(P.p_rgb, 3), at(P.p_valid, 1), at(P.film, 4), at(P.q0, 1), at(P.q1, 1);
    return P;
}
BItems slot_view(const BItems& BI, int s0) {
    BItems I = BI;
    const size_t o = (size_t)s0;
    auto at = [o](auto*& p, size_t per_slot) { p += per_slot * o; };
    at(I.nl, 1), at(I.nc, 1), at(I.n_a, 1), at(I.off_a, 1), at(I.n_b, 1), at(I.off_b, 1), at(I.pdf, 1), at(I.wdepth, 1);
    at(I.cam_o, 3), at(I.cam_d, 3), at(I.rng0, 2), at(I.lam0, 4);
    return I;
}

lumo_status render_bdpt_groups(Ctx& c, Render& R) {
    const Paths& S = R.P[0];
    const Tasks& T = R.T;
    const Dump& D = R.D;
    const Bdpt& B = R.B;
    const int N = R.N, G = R.plan.G;
    const uint64_t max_samples = R.max_samples;
    const std::vector<int32_t>& first = R.first;
    lumo_tile_result* out = R.out;
    std::vector<uint64_t>& n_splats = R.n_splats;
    uint64_t& bounces = R.bounces;
    double* dfilm = R.dfilm;
    lumo_status st = LUMO_OK;
    JoinOnError join{c};
    std::vector<BdGroup> gr(G);
    const int V = B.lp.V, VR = BDPT_MAX_DEPTH + 1;
    const int SEG = Ctx::SNAP_RING / 4;  // snapshot slots per group
    const std::vector<std::pair<int, int>> groups = task_groups(first.data(), (int)R.n_tasks, N, G);
    for (int g = 0; g < G; ++g) {
        BdGroup& q = gr[g];
        q.t0 = groups[g].first;
        q.t1 = groups[g].second;
        q.s0 = first[q.t0];
        q.n = first[q.t1] - q.s0;
        q.sm = c.streams[g];
        q.s = SnapCursor{g * SEG, SEG};
        const size_t o = (size_t)q.s0;
        q.S = slot_view(S, q.s0, R.dim_stride);
        q.S.counts = S.counts + (size_t)g * CNT_N;  // zeroed at setup, then by the group's rings
        Bdpt& X = q.B;
        X = B;
        X.lp = vstore_part(B.lp, q.s0, q.n);
        X.cp = vstore_part(B.cp, q.s0, q.n);
        X.sp = SplatStore{B.sp.d + (size_t)10 * V * o, B.sp.n + o, V, q.n};
        X.draws = B.draws + (size_t)5 * V * o;
        X.ok = B.ok + (size_t)V * o;
        X.overflow = B.overflow + 2 * g;  // per group: overflow flag, redo count
        X.redo_count = X.overflow + 1;
        X.redo_cap = (uint32_t)std::min(q.n, 4096);
        X.redo_list = gbuf<int32_t>(c, g, BG_REDO, X.redo_cap, st);
        X.redo_index = B.redo_index + o;
        const int NR = (int)X.redo_cap;
        Bdpt& RR = q.R;  // storage for lumo's deepest subpaths of the group's re-runs
        RR = X;
        RR.lp = VStore{gbuf<double>(c, g, BG_RLD, (size_t)VD_N * VR * NR, st), gbuf<int32_t>(c, g, BG_RLI, (size_t)VI_N * VR * NR, st),
                       VR, NR, gbuf<double>(c, g, BG_RLM, (size_t)2 * VR * NR, st), gbuf<int32_t>(c, g, BG_RLMF, (size_t)VR * NR, st)};
        RR.cp = VStore{gbuf<double>(c, g, BG_RCD, (size_t)VD_N * VR * NR, st), gbuf<int32_t>(c, g, BG_RCI, (size_t)VI_N * VR * NR, st),
                       VR, NR, gbuf<double>(c, g, BG_RCM, (size_t)2 * VR * NR, st), gbuf<int32_t>(c, g, BG_RCMF, (size_t)VR * NR, st)};
        RR.sp = SplatStore{gbuf<double>(c, g, BG_RSP, (size_t)10 * VR * NR, st), gbuf<int32_t>(c, g, BG_RSPN, NR, st), VR, NR};
        RR.draws = gbuf<double>(c, g, BG_RDRAWS, (size_t)5 * VR * NR, st);
        RR.ok = gbuf<int32_t>(c, g, BG_ROK, (size_t)VR * NR, st);
        q.I = slot_view(R.BI, q.s0);
        q.totals = R.items_total + 8 * g;
    }
    if (st) return st;
    // every group stream waits for the render's setup on stream 0 (tables, seeds, zeroing, ring)
    HIPCHK(hipEventRecord(c.pass_ev[0], c.streams[0]));
    for (int g = 1; g < G; ++g) HIPCHK(hipStreamWaitEvent(c.streams[g], c.pass_ev[0], 0));
    const int ahead = std::max(1, std::min((int)c.o.bounce_ahead, SEG - 1));
    const int fx = c.sc.full;
    // walks: sorted on request (LUMO_OPT_RAY_SORT 1 / 2), and only with concurrent groups
    const int walk_sort = G > 1 && c.o.ray_sort > 0 ? (int)c.o.ray_sort : 0;
    auto start_walk = [&](BdGroup& q, int phase) {
        q.phase = phase;
        q.walk = 0;
        q.s.begin_segment((uint32_t)q.n);
    };
    auto start_pass = [&](BdGroup& q) -> lumo_status {
        // a path dump (one task, one group): the delta this pass's Russian roulette reads
        if (D.delta) HIPCHK(hipMemcpyAsync(D.delta + q.pass, T.delta, sizeof(double), hipMemcpyDeviceToDevice, q.sm));
        {
            StageTimer tm(c, c.o.timing, ST_CAMERA, q.sm);
            k_camera<false><<<ceil_div(q.n, BLOCK), BLOCK, 0, q.sm>>>(T, q.S, c.cam, q.n, R.dim_stride, (uint32_t)q.pass, 0,
                                                                       1, 0);
        }
        k_zero_counts<<<1, 64, 0, q.sm>>>(q.S.counts, q.B.redo_count);  // drop k_camera's queue; no re-runs yet
        by_fx(fx, [&](auto FX) {
            k_bdpt_light_init<decltype(FX)::value><<<ceil_div(q.n, BLOCK), BLOCK, 0, q.sm>>>(c.sc, q.S, q.B, q.I, q.n);
        });
        HIPCHK(hipGetLastError());
        start_walk(q, BD_LIGHT);
        return LUMO_OK;
    };
    // one walk bounce (k_bdpt_tail ahead of it once few subpaths are alive, then k_closest +
    // k_bdpt_step), its count snapshot recorded on the group's stream
    auto issue_walk = [&](BdGroup& q, int gi) -> lumo_status {
        const int mode = q.phase == BD_LIGHT ? TR_IMPORTANCE : TR_RADIANCE;
        int32_t* qa = (q.walk & 1) ? q.S.q1 : q.S.q0;
        int32_t* qb = (q.walk & 1) ? q.S.q0 : q.S.q1;
        const uint32_t ub = q.s.ub;
        k_bounce_begin<<<1, 64, 0, q.sm>>>(q.S.counts, q.S.tcount + TC_HEADQ);
        const uint32_t skip = (uint64_t)ub < 4ull * c.o.bdpt_tail ? (uint32_t)c.o.bdpt_tail : 0u;
        if (walk_sort && skip == 0 && ub >= kSortMin) {  // the walk's rays sorted (lane order only)
            StageTimer tm(c, c.o.timing, ST_CLOSEST, q.sm);
            const size_t nq = (size_t)q.n;
            uint32_t* keys = gbuf<uint32_t>(c, gi, BG_SK0, nq, st);
            uint32_t* order = gbuf<uint32_t>(c, gi, BG_SV0, nq, st);
            uint32_t* ws = gbuf<uint32_t>(c, gi, BG_STMP, RS_WORDS, st);
            if (st) return st;
            if (!q.sort_ws_zeroed) {
                HIPCHK(hipMemsetAsync(ws, 0, sizeof(uint32_t) * RS_WORDS, q.sm));
                q.sort_ws_zeroed = true;
            }
            const int g = ceil_div(ub, RS_BLOCK);
            k_rsort_keys_slots<<<g, RS_BLOCK, 0, q.sm>>>(qa, q.S.ro, q.S.rd, q.S.counts, ub, c.sort_lo, c.sort_scale,
                                                         walk_sort, keys, ws);
            k_rsort_scatter_slots<<<g, RS_BLOCK, 0, q.sm>>>(qa, keys, q.S.counts, ub, ws, order);
            c.stats.sorted_bounces += 1;
            qa = reinterpret_cast<int32_t*>(order);
        }
        if (skip > 0) {
            StageTimer tm(c, c.o.timing, ST_RESOLVE, q.sm);
            launch_trav(c, std::min(ub, skip), [&](auto K, const TravLaunch& l) {
                launch_bdpt_tail<decltype(K)::value>(l, c.sc, q.S, T, q.B, q.I, mode, qa, skip);
            }, q.sm);
        }
        {
            StageTimer tm(c, c.o.timing, ST_CLOSEST, q.sm);
            launch_trav(c, ub, [&](auto K, const TravLaunch& l) {
                launch_closest<decltype(K)::value>(l, c.sc, q.S, qa, skip);
            }, q.sm);
        }
        {
            StageTimer tm(c, c.o.timing, ST_SHADE, q.sm);
            by_stack_class(c.sc.stack_class, [&](auto K) {
                launch_bdpt_step<decltype(K)::value>(ceil_div(ub, BLOCK), q.sm, fx, c.sc, q.S, T, q.B, q.I, mode, qa, qb,
                                                     skip);
            });
        }
        HIPCHK(hipGetLastError());
        const lumo_status e = q.s.record(c, q.S.counts, q.sm);
        if (e) return e;
        q.walk++;
        return LUMO_OK;
    };
    // both walks done: re-runs, the item lists' scans and totals (read back through pinned memory)
    auto after_walks = [&](BdGroup& q, int gi) -> lumo_status {
        {
            StageTimer tm(c, c.o.timing, ST_RESOLVE, q.sm);
            launch_trav(c, (uint64_t)q.B.redo_cap, [&](auto K, const TravLaunch& l) {
                launch_bdpt_redo<decltype(K)::value>(l, c.sc, q.S, T, c.cam, q.B, q.R, q.I);
            }, q.sm);
        }
        for (int k = 0; k < 2; ++k) {
            uint32_t* cnt = k == 0 ? q.I.n_a : q.I.n_b;
            uint32_t* off = k == 0 ? q.I.off_a : q.I.off_b;
            uint32_t* sums = gbuf<uint32_t>(c, gi, BG_SCAN, (size_t)scan_blocks(q.n), st);
            if (st) return st;
            HIPCHK(exclusive_scan(cnt, off, q.n, sums, q.sm));
        }
        k_bdpt_total<<<1, 64, 0, q.sm>>>(q.I, q.n, q.totals);
        HIPCHK(hipMemcpyAsync(c.bd_totals_h + 2 * gi, q.totals, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, q.sm));  // (a), (b)
        HIPCHK(hipEventRecord(c.bd_ev[gi], q.sm));
        q.phase = BD_TOTALS;
        return LUMO_OK;
    };
    // the totals are known: connection items, fold, film, ring, splat taps; then the next pass
    auto items = [&](BdGroup& q, int gi) -> lumo_status {
        const uint32_t tot[2] = {c.bd_totals_h[2 * gi], c.bd_totals_h[2 * gi + 1]};
        auto cap = [](uint32_t x) { return (size_t)std::max<uint64_t>(1, (uint64_t)x + x / 4); };  // grown with headroom
        const size_t ca = cap(tot[0]), cb = cap(tot[1]);
        const size_t need[BG_SCAN] = {4 * ca * 8, 4 * cb * 8, 2 * cb * 4, ca * 8, ca * 4, ca * 4, ca * 4, 2 * ca * 4};
        for (int k = 0; k < BG_SCAN; ++k)  // a buffer that grows is freed: nothing of this group may be using it
            if (c.gwork.size() > (size_t)gi * BG_COUNT + k && c.gwork[(size_t)gi * BG_COUNT + k].bytes < need[k]) {
                HIPCHK(hipStreamSynchronize(q.sm));
                break;
            }
        q.I.term_a = gbuf<double>(c, gi, BG_TERM_A, 4 * ca, st);
        q.I.term_b = gbuf<double>(c, gi, BG_TERM_B, 4 * cb, st);
        q.I.blist = gbuf<int32_t>(c, gi, BG_BLIST, 2 * cb, st);
        q.I.blist_cap = cb;
        q.I.a_t = gbuf<double>(c, gi, BG_AT, ca, st);
        q.I.a_kind = gbuf<int32_t>(c, gi, BG_AKIND, ca, st);
        q.I.a_obj = gbuf<int32_t>(c, gi, BG_AOBJ, ca, st);
        q.I.a_tri = gbuf<int32_t>(c, gi, BG_ATRI, ca, st);
        q.I.alist = gbuf<int32_t>(c, gi, BG_ALIST, 2 * ca, st);
        q.I.alist_cap = ca;
        if (st) return st;
        if (tot[0] > 0) {
            {
                StageTimer tm(c, c.o.timing, ST_BD_TRACE_A, q.sm);
                k_bdpt_alists<<<ceil_div(q.n, BLOCK), BLOCK, 0, q.sm>>>(q.B, q.R, q.I, q.n, q.totals);
                for (int kind = 0; kind < 2; ++kind)
                    launch_trav(c, (uint64_t)tot[0], [&](auto K, const TravLaunch& l) {
                        launch_bdpt_trace_a<decltype(K)::value>(l, c.sc, q.S, c.cam, q.B, q.R, q.I, q.n, q.totals, kind);
                    }, q.sm);
            }
            StageTimer tm(c, c.o.timing, ST_BD_EVAL_A, q.sm);
            launch_eval_a(fx, std::min(ceil_div(tot[0], BLOCK), 1 << 16), ceil_div(q.n, BLOCK), q.sm, c.sc, q.S, c.cam,
                          q.B, q.R, q.I, q.n, q.totals);
        }
        if (tot[1] > 0) {
            {
                StageTimer tm(c, c.o.timing, ST_BD_VIS, q.sm);
                k_bdpt_blists<<<ceil_div(q.n, BLOCK), BLOCK, 0, q.sm>>>(q.B, q.R, q.I, q.n, q.totals);
                // textured scenes (fx 2) have no TOP variant: their full-grid launch
                launch_trav(c, (uint64_t)tot[1], [&](auto K, const TravLaunch& l) {
                    launch_bdpt_vis<decltype(K)::value>(l, c.sc, q.S, q.B, q.R, q.I, q.n, q.totals);
                }, q.sm, c.o.bdpt_top != 0 && fx != 2);
            }
            StageTimer tm(c, c.o.timing, ST_BD_PATHS, q.sm);
            const int grid = std::min(ceil_div(tot[1], BLOCK), 1 << 16);
            by_fx(fx, [&](auto FX) {
                k_bdpt_paths<decltype(FX)::value><<<grid, BLOCK, 0, q.sm>>>(c.sc, q.S, c.cam, q.B, q.R, q.I, q.n,
                                                                           q.totals);
            });
        }
        {
            StageTimer tm(c, c.o.timing, ST_RESOLVE, q.sm);
            k_bdpt_fold<<<ceil_div(q.n, BLOCK), BLOCK, 0, q.sm>>>(q.S, q.B, q.R, q.I, q.n);
        }
        HIPCHK(hipGetLastError());
        const int s1 = q.s0 + q.n;
        // film and ring from the render's whole per-slot view, this group's tasks
        if (R.max_P <= BLOCK)
            film_tiles(c, R, q.sm, S, q.pass, 1, 0, q.t0, q.t1);
        else
            film_large(c, R, q.sm, S, q.pass, q.s0, s1);
        {
            StageTimer tm(c, c.o.timing, ST_RING, q.sm);
            k_ring<<<q.t1 - q.t0, 64, 0, q.sm>>>(c.sc, S, T, q.t1, 1, q.S.counts, q.t0);
        }
        HIPCHK(hipGetLastError());
        if (dfilm) {
            k_bdpt_taps<2><<<ceil_div(q.n, BLOCK), BLOCK, 0, q.sm>>>(c.sc, q.S, q.B, q.R, c.cam, q.n, c.tone_map,
                                                                      c.tone_arg, nullptr, nullptr, nullptr, dfilm);
            HIPCHK(hipGetLastError());
        } else if (R.splat_lists) {  // this pass's taps in lumo's order, appended per task (blocking)
            uint32_t* cnt = R.tap_cnt + q.s0;
            uint32_t* off = R.tap_off + q.s0;
            k_bdpt_taps<0><<<ceil_div(q.n, BLOCK), BLOCK, 0, q.sm>>>(c.sc, q.S, q.B, q.R, c.cam, q.n, c.tone_map,
                                                                      c.tone_arg, cnt, nullptr, nullptr, nullptr);
            uint32_t* sums = gbuf<uint32_t>(c, gi, BG_SCAN, (size_t)scan_blocks(q.n), st);
            if (st) return st;
            HIPCHK(exclusive_scan(cnt, off, q.n, sums, q.sm));
            const int ntg = q.t1 - q.t0;
            uint64_t* ranges = gbuf<uint64_t>(c, gi, BG_RANGES, (size_t)ntg + 1, st);
            if (st) return st;
            k_task_tap_ranges<<<ceil_div(ntg + 1, BLOCK), BLOCK, 0, q.sm>>>(T, cnt, off, ntg, q.n, ranges, q.t0, q.s0);
            std::vector<uint64_t> ranges_h((size_t)ntg + 1);
            HIPCHK(hipMemcpyAsync(ranges_h.data(), ranges, sizeof(uint64_t) * (ntg + 1), hipMemcpyDeviceToHost, q.sm));
            HIPCHK(hipStreamSynchronize(q.sm));
            const uint64_t total = ranges_h[ntg];
            if (total > 0) {
                if (c.gwork[(size_t)gi * BG_COUNT + BG_TAPS].bytes < sizeof(lumo_splat) * total)
                    HIPCHK(hipStreamSynchronize(q.sm));
                lumo_splat* dtaps = gbuf<lumo_splat>(c, gi, BG_TAPS, total, st);
                if (st) return st;
                k_bdpt_taps<1><<<ceil_div(q.n, BLOCK), BLOCK, 0, q.sm>>>(c.sc, q.S, q.B, q.R, c.cam, q.n, c.tone_map,
                                                                          c.tone_arg, nullptr, off, dtaps, nullptr);
                HIPCHK(hipGetLastError());
                std::vector<lumo_splat> taps_h(total);
                HIPCHK(hipMemcpyAsync(taps_h.data(), dtaps, sizeof(lumo_splat) * total, hipMemcpyDeviceToHost, q.sm));
                HIPCHK(hipStreamSynchronize(q.sm));
                for (int i = 0; i < ntg; ++i) {
                    const int ti = q.t0 + i;
                    for (uint64_t k = ranges_h[i]; k < ranges_h[i + 1]; ++k) {
                        if (n_splats[ti] < out[ti].splat_cap) out[ti].splats[n_splats[ti]] = taps_h[k];
                        n_splats[ti]++;
                    }
                }
            }
        }
        if (c.o.timing) resolve_timers(c);
        q.pass++;
        if (q.pass < max_samples) return start_pass(q);
        q.phase = BD_DONE;
        return LUMO_OK;
    };
    lumo_status e = LUMO_OK;
    for (int g = 0; g < G; ++g)
        if ((e = start_pass(gr[g]))) return e;
    for (;;) {
        bool all_done = true;
        for (int g = 0; g < G; ++g) {
            BdGroup& q = gr[g];
            if (q.phase == BD_DONE) continue;
            all_done = false;
            if (q.phase == BD_TOTALS) {
                if (hipEventQuery(c.bd_ev[g]) == hipSuccess && (e = items(q, g))) return e;
                continue;
            }
            if ((e = q.s.poll(c, SnapCursor::kNoWait, bounces))) return e;
            if (q.s.done) {  // the walk has ended
                if (q.phase == BD_LIGHT) {
                    k_zero_counts<<<1, 64, 0, q.sm>>>(q.S.counts, nullptr);
                    k_bdpt_cam_init<<<ceil_div(q.n, BLOCK), BLOCK, 0, q.sm>>>(q.S, q.B, q.I, c.cam, q.n);
                    HIPCHK(hipGetLastError());
                    start_walk(q, BD_CAMERA);
                } else if ((e = after_walks(q, g))) {
                    return e;
                }
            } else if (q.s.outstanding() < ahead) {
                if ((e = issue_walk(q, g))) return e;
            }
        }
        if (all_done) break;
    }
    // the results are copied on stream 0: after every group's last pass
    for (int g = 1; g < G; ++g) {
        HIPCHK(hipEventRecord(c.pass_ev[g], c.streams[g]));
        HIPCHK(hipStreamWaitEvent(c.streams[0], c.pass_ev[g], 0));
    }
    join.ok = true;
    return LUMO_OK;
}

// The sequential loop: path tracing pass after pass on stream 0, without a pipeline.  It is the
// baseline the pipelines are compared against and the route of a path dump of the split bounces.
lumo_status render_sequential(Ctx& c, Render& R) {
    const Paths& S = R.P[0];
    const Tasks& T = R.T;
    const int N = R.N, n_tasks = (int)R.n_tasks;
    hipStream_t sm = c.streams[0];
    // the host blocks only on the snapshot of the bounce `ahead` launches back (SnapCursor)
    const int ahead = (int)c.o.bounce_ahead;
    for (uint64_t pass = 0; pass < R.max_samples; ++pass) {
        if (R.dump_host) HIPCHK(hipMemcpyAsync(R.D.delta + pass, T.delta, sizeof(double), hipMemcpyDeviceToDevice, sm));
        // S.counts: zeroed at setup, then by the ring at the end of every pass
        {
            StageTimer tm(c, c.o.timing, ST_CAMERA);
            k_camera<true><<<ceil_div(N, BLOCK), BLOCK, 0, sm>>>(T, S, c.cam, N, R.dim_stride, (uint32_t)pass, 0, 1, 0);
        }
        HIPCHK(hipGetLastError());
        // Bounce loop over the alive queue (filled by the camera kernel just launched); the parity
        // of the bounce selects the ping-pong queues.
        SnapCursor s;  // the whole ring; the previous pass's slots and events are simply re-recorded
        s.begin_segment((uint32_t)N);
        for (;;) {
            lumo_status e = s.poll(c, ahead - 1, R.bounces);
            if (e) return e;
            if (s.done) break;
            k_bounce_begin<<<1, 64, 0, sm>>>(S.counts, S.tcount + TC_HEADQ);
            issue_split_bounce(c, S, T, S.qs[s.issued & 1], S.qs[(s.issued + 1) & 1], s.ub, sm, R.plan.fused);
            HIPCHK(hipGetLastError());
            if ((e = s.record(c, S.counts, sm))) return e;
        }
        // The bounces issued past the first empty snapshot see empty queues; nothing waits for
        // them: the stream orders them before the film kernels launched next (waiting here
        // left the GPU idle for a host round trip per pass).
        if (c.o.timing) resolve_timers(c);
        if (R.max_P <= BLOCK)
            film_tiles(c, R, sm, S, pass, 1, 0, 0, n_tasks);
        else
            film_large(c, R, sm, S, pass, 0, N);
        {
            StageTimer tm(c, c.o.timing, ST_RING);
            k_ring<<<n_tasks, 64, 0, sm>>>(c.sc, S, T, n_tasks, 1, S.counts, 0);
        }
        HIPCHK(hipGetLastError());
    }
    return LUMO_OK;
}

// render_impl step 1: the tasks validated, one slot per pixel of every task.
lumo_status build_slots(Render& R) {
    R.first.resize(R.n_tasks + 1);
    uint64_t max_total = 1;
    for (size_t i = 0; i < R.n_tasks; ++i) {
        const lumo_tile_task& t = R.tasks[i];
        if (!(t.px_max[0] > t.px_min[0] && t.px_max[1] > t.px_min[1]) || t.samples == 0 ||
            t.samples > SAMPLES_INCREMENT || t.total_samples == 0 ||
            t.px_max[0] > (uint64_t)1 << 31 || t.px_max[1] > (uint64_t)1 << 31)
            return LUMO_ERR_INVALID;
        const uint64_t P = (t.px_max[0] - t.px_min[0]) * (t.px_max[1] - t.px_min[1]);
        R.max_P = std::max(R.max_P, P);
        R.first[i] = (int32_t)R.task_of.size();
        for (uint64_t j = 0; j < P; ++j) {
            R.task_of.push_back((int32_t)i);
            R.pix_of.push_back((int32_t)j);
        }
        if (R.task_of.size() > (1u << 30)) return LUMO_ERR_INVALID;
        max_total = std::max(max_total, t.total_samples);
        R.max_samples = std::max(R.max_samples, t.samples);
    }
    R.first[R.n_tasks] = (int32_t)R.task_of.size();
    R.N = (int)R.task_of.size();
    R.dim_stride = (int)std::ceil(std::sqrt((double)max_total));
    return R.dim_stride > 65535 ? LUMO_ERR_INVALID : LUMO_OK;
}

// Step 2: the schedule (sched_plan.h), from the options, the scene, the render's size and, where the
// split schedule's pipeline is a candidate, the free device memory.
SchedPlan plan_render(const Ctx& c, const Render& R) {
    SchedIn in{};
    in.fused = c.o.fused, in.lds = c.o.lds, in.pipeline = c.o.pipeline, in.heads = c.o.heads, in.merge = c.o.merge;
    in.tail_bounces = c.o.tail_bounces, in.split_pipe = c.o.split_pipe, in.split_groups = c.o.split_groups;
    in.bdpt_groups = c.o.bdpt_groups;
    in.bdpt = c.integrator == LUMO_INTEGRATOR_BDPT;
    in.dump = R.dump_host != nullptr;
    in.n_shadow = c.sc.n_shadow, in.max_merge = MAX_MERGE, in.rr_depth = RR_DEPTH;
    in.staged = c.sc.hot_bytes > 0;
    in.fused_fits = (size_t)(c.sc.hot_bytes + 15u) / 16u * 16u +
                        (size_t)PARK_DOUBLES * sizeof(double) * (size_t)c.o.bounce_threads <= c.lds_block;
    in.N = R.N, in.n_tasks = (int)R.n_tasks, in.max_samples = R.max_samples;
    if (plan_reads_hbm(in)) {
        size_t total_b = 0;
        split_set_bytes(c, &in.set_bytes_slot, &in.set_bytes_fixed);
        in.held = c.split_sets_bytes;
        in.hbm_known = hipMemGetInfo(&in.free_hbm, &total_b) == hipSuccess;
    }
    return plan_schedule(in);
}

// Step 3: the work buffers of the planned schedule: its pass sets, the per-slot state, the task
// table, the dump and, for BDPT, the subpath and item stores.
lumo_status alloc_render(Ctx& c, Render& R) {
    const SchedPlan& plan = R.plan;
    const int N = R.N;
    const size_t n_tasks = R.n_tasks;
    const bool bdpt = c.integrator == LUMO_INTEGRATOR_BDPT;
    lumo_status st = LUMO_OK;
    // M merged passes' outputs and paths per set; a merged unit of the split schedule runs its head
    // bounces on the M passes' paths at once, the fused kernel needs no more hits and records than
    // one pass's (MI355X has the HBM for the worst case)
    const size_t NV = (size_t)N * (size_t)plan.M;
    const size_t cap = plan.schedule == LUMO_SCHED_FUSED_PIPELINE ? (size_t)N : NV;
    Paths& S = R.P[0];
    alloc_pass_set(c, S, 0, bdpt ? SET_OUT : (R.features ? SET_OUT | SET_QUEUES : SET_ALL), NV, cap, st);
    // per slot: camera sampler, raster, final values; BDPT also its walk state
    S.task = wbuf<int32_t>(c, W_TASK, N, st);
    S.pix = wbuf<int32_t>(c, W_PIX, N, st);
    S.pseed = wbuf<uint64_t>(c, W_PSEED, N, st);
    S.mj_rng = wbuf<uint64_t>(c, W_MJRNG, 2 * (size_t)N, st);
    S.mj_state = wbuf<uint64_t>(c, W_MJSTATE, N, st);
    S.perm = wbuf<uint16_t>(c, W_PERM, 2 * (size_t)R.dim_stride * N, st);
    if (bdpt) {
        S.ro = wbuf<double>(c, W_RO, 3 * (size_t)N, st);
        S.rd = wbuf<double>(c, W_RD, 3 * (size_t)N, st);
        S.gath = wbuf<double>(c, W_GATH, 4 * (size_t)N, st);
        S.rng = wbuf<uint64_t>(c, W_RNG, 2 * (size_t)N, st);
        S.flags = wbuf<uint32_t>(c, W_FLAGS, N, st);
        S.hit_t = wbuf<double>(c, W_HIT_T, N, st);
        S.hit_kind = wbuf<int32_t>(c, W_HIT_KIND, N, st);
        S.hit_obj = wbuf<int32_t>(c, W_HIT_OBJ, N, st);
        S.hit_tri = wbuf<int32_t>(c, W_HIT_TRI, N, st);
        S.q0 = wbuf<int32_t>(c, W_Q0, N, st);
        S.q1 = wbuf<int32_t>(c, W_Q1, N, st);
    }
    S.p_rgb = wbuf<double>(c, W_P_RGB, 3 * (size_t)N, st);
    S.film = wbuf<double>(c, W_FILM, 4 * (size_t)N, st);
    S.tcount = wbuf<unsigned long long>(c, W_TCOUNT, TC_ALL + TC_STATS, st);
    S.checks = wbuf<unsigned long long>(c, W_CHECKS, 3, st);
    // the pipelines' further sets: the fused pipeline's share set 0's hits and NEE records
    if (plan.schedule == LUMO_SCHED_FUSED_PIPELINE || plan.schedule == LUMO_SCHED_SPLIT_PIPELINE) {
        const bool split = plan.schedule == LUMO_SCHED_SPLIT_PIPELINE;
        const int sets = split ? plan.K : plan.head_streams + 1;
        for (int k = 1; k < sets; ++k) {
            R.P[k] = S;
            alloc_pass_set(c, R.P[k], k, split ? SET_ALL : SET_OUT | SET_QUEUES, NV, cap, st);
        }
        if (split && !st) {
            size_t slot = 0, fixed = 0;
            split_set_bytes(c, &slot, &fixed);
            c.split_sets_bytes = std::max(c.split_sets_bytes, (size_t)(plan.K - 1) * (fixed + slot * NV));
        }
    }
    Tasks& T = R.T;
    T.t = wbuf<lumo_tile_task>(c, W_TASKS, n_tasks, st);
    T.first = wbuf<int32_t>(c, W_FIRST, n_tasks + 1, st);
    T.ring_cost = wbuf<uint64_t>(c, W_RING_COST, SAMPLES_INCREMENT * n_tasks, st);
    T.ring_lum = wbuf<double>(c, W_RING_LUM, SAMPLES_INCREMENT * n_tasks, st);
    T.ring_ptr = wbuf<uint32_t>(c, W_RING_PTR, n_tasks, st);
    T.delta = wbuf<double>(c, W_DELTA, n_tasks, st);
    T.sampler = c.sampler;
    T.num_rays = wbuf<unsigned long long>(c, W_NUM_RAYS, n_tasks, st);
    T.queries = wbuf<unsigned long long>(c, W_TQUERIES, n_tasks, st);
    if (R.dump_host) {
        R.dump_p = N;  // single task
        const size_t m = (size_t)R.dump_samples * N;
        R.D.rad = wbuf<double>(c, W_DUMP_RAD, 4 * m, st);
        R.D.lam = wbuf<double>(c, W_DUMP_LAM, 4 * m, st);
        R.D.raster = wbuf<double>(c, W_DUMP_RASTER, 2 * m, st);
        R.D.depth = wbuf<unsigned long long>(c, W_DUMP_DEPTH, m, st);
        R.D.delta = wbuf<double>(c, W_DUMP_DELTA, R.dump_samples, st);
    }
    if (bdpt) {
        Bdpt& B = R.B;
        BItems& BI = R.BI;
        const int V = c.max_vertices;
        B.lp = VStore{wbuf<double>(c, W_BD_LD, (size_t)VD_N * V * N, st), wbuf<int32_t>(c, W_BD_LI, (size_t)VI_N * V * N, st), V, N,
                      wbuf<double>(c, W_BD_LM, (size_t)2 * V * N, st), wbuf<int32_t>(c, W_BD_LMF, (size_t)V * N, st)};
        B.cp = VStore{wbuf<double>(c, W_BD_CD, (size_t)VD_N * V * N, st), wbuf<int32_t>(c, W_BD_CI, (size_t)VI_N * V * N, st), V, N,
                      wbuf<double>(c, W_BD_CM, (size_t)2 * V * N, st), wbuf<int32_t>(c, W_BD_CMF, (size_t)V * N, st)};
        B.sp = SplatStore{wbuf<double>(c, W_BD_SP, (size_t)10 * V * N, st), wbuf<int32_t>(c, W_BD_SPN, N, st), V, N};
        B.overflow = wbuf<uint32_t>(c, W_BD_OVF, 8, st);  // (overflow, redo count) per task group
        B.redo_count = B.overflow + 1;
        B.redo_index = wbuf<int32_t>(c, W_BD_REDO_INDEX, N, st);
        B.draws = wbuf<double>(c, W_BD_DRAWS, (size_t)5 * V * N, st);
        B.ok = wbuf<int32_t>(c, W_BD_OK, (size_t)V * N, st);
        BI.nl = wbuf<int32_t>(c, W_BD_NL, N, st);
        BI.nc = wbuf<int32_t>(c, W_BD_NC, N, st);
        BI.n_a = wbuf<uint32_t>(c, W_BD_NITEMS, N, st);
        BI.off_a = wbuf<uint32_t>(c, W_BD_IOFF, N, st);
        BI.n_b = wbuf<uint32_t>(c, W_BD_NB, N, st);
        BI.off_b = wbuf<uint32_t>(c, W_BD_OFFB, N, st);
        BI.pdf = wbuf<double>(c, W_BD_PDF, N, st);
        BI.wdepth = wbuf<int32_t>(c, W_BD_WDEPTH, N, st);
        BI.cam_o = wbuf<double>(c, W_BD_CAMO, 3 * (size_t)N, st);
        BI.cam_d = wbuf<double>(c, W_BD_CAMD, 3 * (size_t)N, st);
        BI.rng0 = wbuf<uint64_t>(c, W_BD_RNG0, 2 * (size_t)N, st);
        BI.lam0 = wbuf<double>(c, W_BD_LAM0, 4 * (size_t)N, st);
        R.items_total = wbuf<uint32_t>(c, W_BD_ITOTAL, 32, st);  // (a), (b) and the item lists' counts per task group
        for (size_t i = 0; i < n_tasks && R.out; ++i) R.splat_lists = R.splat_lists && R.out[i].splats != nullptr;
        if (!R.out) R.splat_lists = false;
        if (R.splat_lists) {
            R.tap_cnt = wbuf<uint32_t>(c, W_BD_CNT, N, st);
            R.tap_off = wbuf<uint32_t>(c, W_BD_OFF, N, st);
        } else if (c.splat_film) {
            R.film_n = (size_t)3 * (size_t)c.cam.width * (size_t)c.cam.height;
            R.dfilm = wbuf<double>(c, W_BD_FILM, R.film_n, st);
        } else if (R.out) {
            return LUMO_ERR_INVALID;  // BDPT splats need per-task lists or a splat film
        }
    }
    return st;
}

// Step 4, on stream 0: the task and slot tables, the zeroing, the seeds and sampler permutations,
// the initial ring.
lumo_status setup_render(Ctx& c, Render& R) {
    const Paths& S = R.P[0];
    const Tasks& T = R.T;
    const int N = R.N;
    const size_t n_tasks = R.n_tasks;
    hipStream_t sm = c.streams[0];
    HIPCHK(hipMemcpyAsync(T.t, R.tasks, sizeof(lumo_tile_task) * n_tasks, hipMemcpyHostToDevice, sm));
    HIPCHK(hipMemcpyAsync(T.first, R.first.data(), sizeof(int32_t) * (n_tasks + 1), hipMemcpyHostToDevice, sm));
    HIPCHK(hipMemcpyAsync(S.task, R.task_of.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, sm));
    HIPCHK(hipMemcpyAsync(S.pix, R.pix_of.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, sm));
    {
        ZeroList z;
        z.add(T.ring_cost, sizeof(uint64_t) * SAMPLES_INCREMENT * n_tasks);
        z.add(T.ring_lum, sizeof(double) * SAMPLES_INCREMENT * n_tasks);
        z.add(T.ring_ptr, sizeof(uint32_t) * n_tasks);
        z.add(T.num_rays, sizeof(unsigned long long) * n_tasks);
        z.add(T.queries, sizeof(unsigned long long) * n_tasks);
        z.add(S.film, sizeof(double) * 4 * N);
        z.add(S.tcount, sizeof(unsigned long long) * (TC_ALL + TC_STATS));
        z.add(S.checks, sizeof(unsigned long long) * 3);
        z.add(S.counts, sizeof(uint32_t) * CNT_N * 4);  // + the BDPT task groups' counters
        if (c.integrator == LUMO_INTEGRATOR_BDPT) {
            z.add(R.B.overflow, sizeof(uint32_t) * 8);
            if (R.dfilm) z.add(R.dfilm, sizeof(double) * R.film_n);
        }
        if (z.overflow) return LUMO_ERR_INVALID;
        k_zero_list<<<std::min(ceil_div((uint64_t)4 * N, BLOCK), 2048), BLOCK, 0, sm>>>(z);
    }
    k_init_seeds<<<ceil_div(n_tasks, BLOCK), BLOCK, 0, sm>>>(T, S, (int)n_tasks);
    k_init_mj<<<ceil_div(N, BLOCK), BLOCK, 0, sm>>>(T, S, N, R.dim_stride);
    k_ring<<<(int)n_tasks, 64, 0, sm>>>(c.sc, S, T, (int)n_tasks, 0, nullptr, 0);
    HIPCHK(hipGetLastError());
    return LUMO_OK;
}

// Step 6: the tiles, counters and dump read back on stream 0; the results and statistics filled.
lumo_status read_back(Ctx& c, Render& R) {
    const Paths& S = R.P[0];
    const Tasks& T = R.T;
    const int N = R.N;
    const size_t n_tasks = R.n_tasks;
    lumo_tile_result* out = R.out;
    const std::vector<int32_t>& first = R.first;
    const bool bdpt = c.integrator == LUMO_INTEGRATOR_BDPT;
    hipStream_t sm = c.streams[0];
    // Per-task {sum w*rgb, sum w} tiles: straight into the caller's buffers when they are laid out
    // back to back in slot order (the Python wrapper allocates them so), else via a host copy.
    bool direct = out != nullptr && n_tasks > 0 && out[0].rgb_w != nullptr;
    for (size_t i = 1; i < n_tasks && direct; ++i)
        direct = out[i].rgb_w == out[0].rgb_w + 4 * (size_t)first[i];
    std::vector<double> film(direct ? 0 : (size_t)4 * N);
    std::vector<unsigned long long> rays(n_tasks), queries(n_tasks);
    HIPCHK(hipMemcpyAsync(direct ? out[0].rgb_w : film.data(), S.film, sizeof(double) * 4 * N, hipMemcpyDeviceToHost,
                          sm));
    HIPCHK(hipMemcpyAsync(rays.data(), T.num_rays, sizeof(unsigned long long) * n_tasks, hipMemcpyDeviceToHost, sm));
    HIPCHK(hipMemcpyAsync(queries.data(), T.queries, sizeof(unsigned long long) * n_tasks, hipMemcpyDeviceToHost,
                          sm));
    unsigned long long tc[TC_ALL], checks[3];
    HIPCHK(hipMemcpyAsync(tc, S.tcount, sizeof(tc), hipMemcpyDeviceToHost, sm));
    HIPCHK(hipMemcpyAsync(checks, S.checks, sizeof(checks), hipMemcpyDeviceToHost, sm));
    if (R.dump_host) {
        const Dump& D = R.D;
        const size_t m = (size_t)R.dump_samples * N;
        HIPCHK(hipMemcpyAsync(R.dump_host->rad, D.rad, sizeof(double) * 4 * m, hipMemcpyDeviceToHost, sm));
        HIPCHK(hipMemcpyAsync(R.dump_host->lam, D.lam, sizeof(double) * 4 * m, hipMemcpyDeviceToHost, sm));
        HIPCHK(hipMemcpyAsync(R.dump_host->raster, D.raster, sizeof(double) * 2 * m, hipMemcpyDeviceToHost, sm));
        HIPCHK(hipMemcpyAsync(R.dump_host->depth, D.depth, sizeof(unsigned long long) * m, hipMemcpyDeviceToHost, sm));
        HIPCHK(hipMemcpyAsync(R.dump_host->delta, D.delta, sizeof(double) * R.dump_samples, hipMemcpyDeviceToHost, sm));
    }
    HIPCHK(hipStreamSynchronize(sm));
    if (c.o.timing) resolve_timers(c);
    bool splat_oom = false;
    if (bdpt) {
        uint32_t ovf[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // (overflow, redo count) per task group
        HIPCHK(hipMemcpy(ovf, R.B.overflow, sizeof(ovf), hipMemcpyDeviceToHost));
        if (ovf[0] | ovf[2] | ovf[4] | ovf[6]) return LUMO_ERR_UNSUPPORTED;  // more long subpaths in one pass than a redo list holds
        if (R.dfilm) {
            std::vector<double> f(R.film_n);
            HIPCHK(hipMemcpy(f.data(), R.dfilm, sizeof(double) * R.film_n, hipMemcpyDeviceToHost));
            for (size_t k = 0; k < R.film_n; ++k) c.splat_film[k] += f[k];
        }
        for (size_t i = 0; i < n_tasks && out; ++i) {
            out[i].num_splats = R.n_splats[i];
            splat_oom = splat_oom || (R.splat_lists && R.n_splats[i] > out[i].splat_cap);
        }
    }
    for (size_t i = 0; i < n_tasks; ++i) {
        if (!out) break;
        const lumo_tile_task& t = R.tasks[i];
        const size_t P = (size_t)(first[i + 1] - first[i]);
        if (out[i].rgb_w && !direct)
            std::memcpy(out[i].rgb_w, film.data() + 4 * (size_t)first[i], sizeof(double) * 4 * P);
        out[i].num_camera_rays = P * t.samples;
        out[i].num_rays = rays[i];
        out[i].num_queries = queries[i];
    }
    unsigned long long total_q = 0;
    for (size_t i = 0; i < n_tasks; ++i) total_q += queries[i];
    // per-slot query counters: PT 1 per closest + 1 per valid record; BDPT walk traces (the
    // bounce snapshots) + connection / re-run queries
    const uint64_t closest_q = tc[TC_HEADQ] + tc[TC_TAILQ];  // bounce heads + the tail kernel's further bounces
    c.stats.closest_queries += closest_q;
    c.stats.shadow_queries += total_q >= closest_q ? total_q - closest_q : 0;
    c.stats.bounces += R.bounces;
    c.stats.samples_nan += checks[0];
    c.stats.samples_neg += checks[1];
    c.stats.samples_large += checks[2];
    for (int k = 0; k < 2; ++k) {
        c.stats.aabb_tests[k] += tc[k * TC_N + TC_AABB];
        c.stats.kd_nodes[k] += tc[k * TC_N + TC_KD];
        c.stats.tri_tests[k] += tc[k * TC_N + TC_TRI];
    }
    c.stats.shadow_resolved += tc[TC_RESOLVED];
    c.stats.tail_queries += tc[TC_TAILQ];
#if LUMO_SHADOW_STATS || LUMO_PHASE_CLOCKS
    {
        unsigned long long ss[TC_STATS];
        HIPCHK(hipMemcpy(ss, S.tcount + TC_ALL, sizeof(ss), hipMemcpyDeviceToHost));
        fprintf(stderr, LUMO_SHADOW_STATS ? "LUMO_SHADOW_STATS" : "LUMO_PHASE_CLOCKS");
        for (int k = 0; k < TC_STATS; ++k) fprintf(stderr, " %llu", ss[k]);
        fprintf(stderr, "\n");
    }
#endif
    return splat_oom ? LUMO_ERR_OOM : LUMO_OK;
}

// A render: validate and build slots, plan, allocate, set up on stream 0, run the planned
// scheduler, read back.
lumo_status render_impl(Ctx& c, const lumo_tile_task* tasks, size_t n_tasks, lumo_tile_result* out, Dump* dump_host,
                        uint64_t dump_samples) {
    if (!c.has_scene) return LUMO_ERR_NO_SCENE;
    if (!c.has_camera) return LUMO_ERR_NO_CAMERA;
    if (n_tasks == 0) return LUMO_OK;
    Render R{tasks, n_tasks, out, dump_host, dump_samples};
    R.n_splats.assign(n_tasks, 0);
    lumo_status st = build_slots(R);
    if (st) return st;
    const SchedPlan& p = R.plan = plan_render(c, R);
    c.sched = lumo_schedule_info{p.schedule, p.head_streams, p.head_bounces, p.M,
                                 p.K,        p.G,            p.fused ? 1 : 0, p.tail_bounces};
    if ((st = alloc_render(c, R))) return st;
    if ((st = setup_render(c, R))) return st;
    switch (p.schedule) {
        case LUMO_SCHED_FUSED_PIPELINE: st = render_pipelined(c, R); break;
        case LUMO_SCHED_SPLIT_PIPELINE: st = render_split_pipelined(c, R); break;
        case LUMO_SCHED_BDPT_GROUPS: st = render_bdpt_groups(c, R); break;
        default:  // one chain of passes on stream 0: BDPT's pass body with one group, or the path tracer's loop
            st = c.integrator == LUMO_INTEGRATOR_BDPT ? render_bdpt_groups(c, R) : render_sequential(c, R);
    }
    if (st) return st;
    return read_back(c, R);
}

// A feature render (features.h): render_impl's steps 1, 3 and 4 (slots, work buffers, setup on
// stream 0), then per pass on stream 0 the camera, one closest-hit launch over its queue (queue 0,
// no ray sort), k_features and the pass's share of the three planes.  It plans no schedule and
// leaves the record of lumo_last_schedule alone.  The camera rays count as closest queries with the
// traversal counters of class 0.
constexpr int FT_DUMP_DOUBLES = 28;  // t 1, p 3, ng 3, ns 3, n 3, uv 2, albedo 4, albedo_rgb 3, raster 2, lambda 4
lumo_status render_features_impl(Ctx& c, const lumo_tile_task* tasks, size_t n_tasks, lumo_feature_planes* out,
                                 const lumo_feature_dump* dump) {
    if (!c.has_scene) return LUMO_ERR_NO_SCENE;
    if (!c.has_camera) return LUMO_ERR_NO_CAMERA;
    if (n_tasks == 0) return LUMO_OK;
    Render R{tasks, n_tasks, nullptr, nullptr, 0};
    R.features = true;
    lumo_status st = build_slots(R);
    if (st) return st;
    R.plan = SchedPlan{LUMO_SCHED_SEQUENTIAL, false, 1, 1, 1, 0, 0, 0};
    if ((st = alloc_render(c, R))) return st;
    const int N = R.N, n_t = (int)n_tasks;
    Paths& S = R.P[0];
    S.hq = HitQ{wbuf<double>(c, W_SET0 + F_HQ_T, N, st), wbuf<int32_t>(c, W_SET0 + F_HQ_I, 3 * (size_t)N, st),
                (size_t)N, nullptr, nullptr, nullptr, nullptr};
    Feat F{};
    F.alb = wbuf<double>(c, W_FT_ALB, 3 * (size_t)N, st);
    F.nrm = wbuf<double>(c, W_FT_NRM, 3 * (size_t)N, st);
    F.dep = wbuf<double>(c, W_FT_DEP, 2 * (size_t)N, st);
    F.film_a = wbuf<double>(c, W_FT_FILM_A, 4 * (size_t)N, st);
    F.film_n = wbuf<double>(c, W_FT_FILM_N, 4 * (size_t)N, st);
    F.film_d = wbuf<double>(c, W_FT_FILM_D, 4 * (size_t)N, st);
    const size_t m = dump ? (size_t)tasks[0].samples * (size_t)N : 0;  // a dump: one task
    int32_t* di = nullptr;
    double* dd = nullptr;
    if (dump) {
        di = wbuf<int32_t>(c, W_FT_DUMP_I, 5 * m, st);
        dd = wbuf<double>(c, W_FT_DUMP_D, FT_DUMP_DOUBLES * m, st);
        F.d = FeatDump{di, di + m, di + 2 * m, di + 3 * m, di + 4 * m,
                       dd, dd + m, dd + 4 * m, dd + 7 * m, dd + 10 * m, dd + 13 * m, dd + 15 * m, dd + 19 * m,
                       dd + 22 * m, dd + 24 * m};
        F.dump_p = N;
    }
    if (st) return st;
    if ((st = setup_render(c, R))) return st;
    hipStream_t sm = c.streams[0];
    {
        ZeroList z;
        z.add(F.film_a, sizeof(double) * 4 * N);
        z.add(F.film_n, sizeof(double) * 4 * N);
        z.add(F.film_d, sizeof(double) * 4 * N);
        k_zero_list<<<std::min(ceil_div((uint64_t)4 * N, BLOCK), 2048), BLOCK, 0, sm>>>(z);
    }
    const int gN = ceil_div(N, BLOCK);
    for (uint64_t pass = 0; pass < R.max_samples; ++pass) {
        {   // S.counts: zeroed at setup, then at the end of every pass
            StageTimer tm(c, c.o.timing, ST_CAMERA, sm);
            k_camera<true><<<gN, BLOCK, 0, sm>>>(R.T, S, c.cam, N, R.dim_stride, (uint32_t)pass, 0, 1, 0);
        }
        k_bounce_begin<<<1, 64, 0, sm>>>(S.counts, S.tcount + TC_HEADQ);
        {
            StageTimer tm(c, c.o.timing, ST_CLOSEST, sm);
            launch_trav(
                c, (uint64_t)N,
                [&](auto K, const TravLaunch& l) { launch_closest_q<decltype(K)::value>(l, c.sc, S, S.qs[0], 0u); }, sm,
                true);
        }
        {
            StageTimer tm(c, c.o.timing, ST_SHADE, sm);
            by_fx(c.sc.full, [&](auto FX) {
                k_features<decltype(FX)::value><<<gN, BLOCK, 0, sm>>>(c.sc, S, F, c.cam, S.qs[0], (uint32_t)pass);
            });
        }
        {
            StageTimer tm(c, c.o.timing, ST_FILM, sm);
            if (R.max_P <= BLOCK)
                k_feature_film<<<n_t, BLOCK, 0, sm>>>(S, F, R.T, c.cam, 0);
            else
                k_feature_gather<<<gN, BLOCK, 0, sm>>>(S, F, R.T, c.cam, N);
        }
        k_zero_counts<<<1, 64, 0, sm>>>(S.counts, nullptr);
        HIPCHK(hipGetLastError());
        if (c.o.timing) resolve_timers(c);
    }
    // the planes: straight into the caller's buffers when they lie back to back in slot order
    const double* films[3] = {F.film_a, F.film_n, F.film_d};
    std::vector<double> host;
    for (int k = 0; k < 3 && out; ++k) {
        auto plane = [&](size_t i) { return k == 0 ? out[i].albedo_w : (k == 1 ? out[i].normal_w : out[i].depth_w); };
        bool any = false, direct = plane(0) != nullptr;
        for (size_t i = 0; i < n_tasks; ++i) {
            any = any || plane(i) != nullptr;
            direct = direct && plane(i) == plane(0) + 4 * (size_t)R.first[i];
        }
        if (!any) continue;
        if (direct) {
            HIPCHK(hipMemcpyAsync(plane(0), films[k], sizeof(double) * 4 * N, hipMemcpyDeviceToHost, sm));
            continue;
        }
        host.resize((size_t)4 * N);
        HIPCHK(hipMemcpyAsync(host.data(), films[k], sizeof(double) * 4 * N, hipMemcpyDeviceToHost, sm));
        HIPCHK(hipStreamSynchronize(sm));
        for (size_t i = 0; i < n_tasks; ++i)
            if (plane(i))
                std::memcpy(plane(i), host.data() + 4 * (size_t)R.first[i],
                            sizeof(double) * 4 * (size_t)(R.first[i + 1] - R.first[i]));
    }
    if (dump) {
        int32_t* const hi[5] = {dump->kind, dump->object, dump->prim, dump->material, dump->backface};
        double* const hd[10] = {dump->t, dump->p, dump->ng, dump->ns, dump->n, dump->uv, dump->albedo, dump->albedo_rgb,
                                dump->raster, dump->lambda_};
        const int per[10] = {1, 3, 3, 3, 3, 2, 4, 3, 2, 4};
        for (int k = 0; k < 5; ++k)
            if (hi[k]) HIPCHK(hipMemcpyAsync(hi[k], di + k * m, sizeof(int32_t) * m, hipMemcpyDeviceToHost, sm));
        size_t o = 0;
        for (int k = 0; k < 10; ++k) {
            if (hd[k]) HIPCHK(hipMemcpyAsync(hd[k], dd + o * m, sizeof(double) * per[k] * m, hipMemcpyDeviceToHost, sm));
            o += (size_t)per[k];
        }
    }
    unsigned long long tc[TC_ALL];
    HIPCHK(hipMemcpyAsync(tc, S.tcount, sizeof(tc), hipMemcpyDeviceToHost, sm));
    HIPCHK(hipStreamSynchronize(sm));
    if (c.o.timing) resolve_timers(c);
    c.stats.closest_queries += tc[TC_HEADQ];
    c.stats.aabb_tests[0] += tc[TC_AABB];
    c.stats.kd_nodes[0] += tc[TC_KD];
    c.stats.tri_tests[0] += tc[TC_TRI];
    return LUMO_OK;
}

// The task list of a call cut so that at most max_paths slots are in flight (lumo_render_tiles'
// chunking): the end of the chunk that starts at task i.
size_t chunk_end(const lumo_tile_task* tasks, size_t n, size_t i, size_t max_paths) {
    size_t j = i, paths = 0;
    while (j < n) {
        const size_t P = (tasks[j].px_max[0] - tasks[j].px_min[0]) * (tasks[j].px_max[1] - tasks[j].px_min[1]);
        if (j > i && paths + P > max_paths) break;
        paths += P;
        ++j;
    }
    return j;
}

}  // namespace

// ================================================================== C ABI
extern "C" {

lumo_status lumo_render_tiles(void* ctx, const lumo_tile_task* tasks, size_t n, const lumo_render_cfg* cfg,
                              lumo_tile_result* out) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c || (!tasks && n) || (!out && n)) return LUMO_ERR_INVALID;
    if (cfg && cfg->rng_mode != LUMO_RNG_WAVEFRONT) return LUMO_ERR_UNSUPPORTED;
    if (cfg && cfg->integrator != LUMO_INTEGRATOR_PATH_TRACE && cfg->integrator != LUMO_INTEGRATOR_BDPT)
        return LUMO_ERR_UNSUPPORTED;
    if (cfg && (cfg->max_vertices < 0 || cfg->max_vertices > BDPT_MAX_DEPTH + 1)) return LUMO_ERR_INVALID;
    if (cfg && (cfg->tone_map < LUMO_TONEMAP_NONE || cfg->tone_map > LUMO_TONEMAP_REINHARD)) return LUMO_ERR_INVALID;
    const int sampler = cfg ? cfg->sampler : LUMO_SAMPLER_MULTI_JITTERED;
    if (sampler < LUMO_SAMPLER_MULTI_JITTERED || sampler > LUMO_SAMPLER_SOBOL) return LUMO_ERR_INVALID;
    for (size_t i = 0; i < n && sampler == LUMO_SAMPLER_SOBOL; ++i)
        if (tasks[i].total_samples > 1023) return LUMO_ERR_INVALID;  // sobol_seq.rs SOBOL_MAX_LEN (lumo panics)
    if (cfg && cfg->integrator == LUMO_INTEGRATOR_BDPT && c->has_camera && c->cam.orthographic)
        return LUMO_ERR_UNSUPPORTED;  // camera.rs:348-351: no importance for Orthographic (lumo panics)
    HIPCHK(hipSetDevice(c->device));
    struct CallScope {  // tone map and integrator settings apply to this call only
        Ctx* c;
        ~CallScope() {
            c->tone_map = LUMO_TONEMAP_NONE;
            c->integrator = LUMO_INTEGRATOR_PATH_TRACE;
            c->splat_film = nullptr;
            c->sampler = LUMO_SAMPLER_MULTI_JITTERED;
        }
    } scope{c};
    c->sampler = sampler;
    c->tone_map = cfg ? cfg->tone_map : LUMO_TONEMAP_NONE;
    c->tone_arg = cfg ? cfg->tone_arg : 0.0;
    c->integrator = cfg ? cfg->integrator : LUMO_INTEGRATOR_PATH_TRACE;
    c->max_vertices = (cfg && cfg->max_vertices > 0) ? cfg->max_vertices : 128;
    c->splat_film = cfg ? cfg->splat_film : nullptr;
    size_t max_paths = (cfg && cfg->max_paths > 0) ? (size_t)cfg->max_paths : (size_t)1 << 30;
    if (c->integrator == LUMO_INTEGRATOR_BDPT)  // BDPT storage: ~64 KB per slot at 128 vertices -> 64 GB
        max_paths = std::min(max_paths, (size_t)(((size_t)1 << 27) / (size_t)c->max_vertices));
    size_t i = 0;
    while (i < n) {  // chunk the task list so that at most max_paths slots are in flight
        size_t j = i, paths = 0;
        while (j < n) {
            const size_t P = (tasks[j].px_max[0] - tasks[j].px_min[0]) * (tasks[j].px_max[1] - tasks[j].px_min[1]);
            if (j > i && paths + P > max_paths) break;
            paths += P;
            ++j;
        }
        const lumo_status st = render_impl(*c, tasks + i, j - i, out + i, nullptr, 0);
        if (st) return st;
        i = j;
    }
    return LUMO_OK;
}

lumo_status lumo_trace(void* ctx, const lumo_ray_soa* rays, size_t n, lumo_hit_soa* hits, int any_hit) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c || !rays || !hits || !rays->origin || !rays->dir || (any_hit && !rays->light)) return LUMO_ERR_INVALID;
    if (!c->has_scene) return LUMO_ERR_NO_SCENE;
    if (n == 0) return LUMO_OK;
    HIPCHK(hipSetDevice(c->device));
    if (any_hit)
        for (size_t i = 0; i < n; ++i)
            if (rays->light[i] < 0 || rays->light[i] >= c->sc.n_lights) return LUMO_ERR_INVALID;
    lumo_status st = LUMO_OK;
    double* o = wbuf<double>(*c, W_SH_O, 3 * n, st);
    double* d = wbuf<double>(*c, W_SH_D, 3 * n, st);
    int32_t* light = wbuf<int32_t>(*c, W_SH_LIGHT, n, st);
    double* t = wbuf<double>(*c, W_HIT_T, n, st);
    int32_t* kind = wbuf<int32_t>(*c, W_HIT_KIND, n, st);
    int32_t* obj = wbuf<int32_t>(*c, W_HIT_OBJ, n, st);
    int32_t* prim = wbuf<int32_t>(*c, W_HIT_TRI, n, st);
    unsigned long long* tc = wbuf<unsigned long long>(*c, W_TCOUNT, TC_ALL + TC_STATS, st);
    if (st) return st;
    hipStream_t sm = c->streams[0];
    HIPCHK(hipMemcpyAsync(o, rays->origin, sizeof(double) * 3 * n, hipMemcpyHostToDevice, sm));
    HIPCHK(hipMemcpyAsync(d, rays->dir, sizeof(double) * 3 * n, hipMemcpyHostToDevice, sm));
    if (any_hit) HIPCHK(hipMemcpyAsync(light, rays->light, sizeof(int32_t) * n, hipMemcpyHostToDevice, sm));
    HIPCHK(hipMemsetAsync(tc, 0, sizeof(unsigned long long) * (TC_ALL + TC_STATS), sm));
    const bool top = c->o.top && c->sc.top_bytes > 0 && !(c->o.lds && c->sc.hot_bytes > 0);
    const int grid = top ? std::min(ceil_div(n, TOP_BLOCK), (int)c->o.top_grid) : ceil_div(n, BLOCK);
    by_stack_class(c->sc.stack_class, [&](auto K) {
        launch_trace<decltype(K)::value>(grid, sm, c->sc, o, d, light, (int)n, any_hit, t, kind, obj, prim, tc, top);
    });
    HIPCHK(hipGetLastError());
    if (hits->t) HIPCHK(hipMemcpyAsync(hits->t, t, sizeof(double) * n, hipMemcpyDeviceToHost, sm));
    if (hits->kind) HIPCHK(hipMemcpyAsync(hits->kind, kind, sizeof(int32_t) * n, hipMemcpyDeviceToHost, sm));
    if (hits->object) HIPCHK(hipMemcpyAsync(hits->object, obj, sizeof(int32_t) * n, hipMemcpyDeviceToHost, sm));
    if (hits->prim) HIPCHK(hipMemcpyAsync(hits->prim, prim, sizeof(int32_t) * n, hipMemcpyDeviceToHost, sm));
    unsigned long long tch[2 * TC_N];
    HIPCHK(hipMemcpyAsync(tch, tc, sizeof(unsigned long long) * TC_N, hipMemcpyDeviceToHost, sm));
    HIPCHK(hipStreamSynchronize(sm));
    const int k = any_hit ? 1 : 0;  // traversal counters of the batch: class 0 closest, 1 visibility
    c->stats.aabb_tests[k] += tch[TC_AABB];
    c->stats.kd_nodes[k] += tch[TC_KD];
    c->stats.tri_tests[k] += tch[TC_TRI];
    (any_hit ? c->stats.shadow_queries : c->stats.closest_queries) += n;
    return LUMO_OK;
}

lumo_status lumo_stats_get(void* ctx, lumo_stats* stats) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c || !stats) return LUMO_ERR_INVALID;
    *stats = c->stats;
    return LUMO_OK;
}

// Diagnostics: one k_calib_read8 and one k_calib_write8 launch over n doubles (PMC calibration).
lumo_status lumo_debug_stream(void* ctx, size_t n) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c || n == 0) return LUMO_ERR_INVALID;
    HIPCHK(hipSetDevice(c->device));
    double* buf = nullptr;
    HIPCHK(hipMalloc(&buf, sizeof(double) * n + sizeof(double) * 4096));
    HIPCHK(hipMemsetAsync(buf, 0, sizeof(double) * n, c->streams[0]));
    k_calib_read8<<<2048, BLOCK, 0, c->streams[0]>>>(buf, n, buf + n);
    k_calib_write8<<<2048, BLOCK, 0, c->streams[0]>>>(buf, n);
    const hipError_t e = hipStreamSynchronize(c->streams[0]);
    (void)hipFree(buf);
    HIPCHK(e);
    return LUMO_OK;
}

// Diagnostics: the device exclusive scan (scan.h) of n host uint32 counts into out (host).
lumo_status lumo_debug_scan(void* ctx, const uint32_t* in, uint32_t* out, size_t n) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c || !in || !out || n > 0xffffffffu) return LUMO_ERR_INVALID;
    if (n == 0) return LUMO_OK;  // nothing to scan: out is left untouched
    HIPCHK(hipSetDevice(c->device));
    uint32_t* buf = nullptr;
    const size_t nb = (size_t)scan_blocks((uint32_t)n);
    HIPCHK(hipMalloc(&buf, sizeof(uint32_t) * (2 * n + nb)));
    hipError_t e = hipMemcpyAsync(buf, in, sizeof(uint32_t) * n, hipMemcpyHostToDevice, c->streams[0]);
    if (e == hipSuccess) e = exclusive_scan(buf, buf + n, (uint32_t)n, buf + 2 * n, c->streams[0]);
    if (e == hipSuccess) e = hipMemcpyAsync(out, buf + n, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c->streams[0]);
    if (e == hipSuccess) e = hipStreamSynchronize(c->streams[0]);
    (void)hipFree(buf);
    HIPCHK(e);
    return LUMO_OK;
}

lumo_status lumo_last_schedule(void* ctx, lumo_schedule_info* info) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c || !info) return LUMO_ERR_INVALID;
    *info = c->sched;
    return LUMO_OK;
}

lumo_status lumo_stats_reset(void* ctx) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c) return LUMO_ERR_INVALID;
    std::memset(&c->stats, 0, sizeof(c->stats));
    for (auto& v : c->intervals) v.clear();
    c->ref_recorded = false;
    return LUMO_OK;
}

lumo_status lumo_stats_busy_ms(void* ctx, uint32_t stage_mask, double* ms) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c || !ms) return LUMO_ERR_INVALID;
    *ms = busy_ms(*c, stage_mask);
    return LUMO_OK;
}

// Diagnostics: per-bounce trace of one slot.  The device-side trace log was removed from the
// hot shade kernel (a global compare per path per bounce); per-path dumps (lumo_debug_paths)
// remain the parity instrument.
lumo_status lumo_debug_trace(void* ctx, const lumo_tile_task* task, int pass, int pixel, double* out, int* n_out) {
    (void)ctx; (void)task; (void)pass; (void)pixel; (void)out; (void)n_out;
    return LUMO_ERR_UNSUPPORTED;
}

lumo_status lumo_debug_paths(void* ctx, const lumo_tile_task* task, lumo_path_dump* dump) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c || !task || !dump || !dump->radiance || !dump->lambda_ || !dump->raster || !dump->depth || !dump->delta)
        return LUMO_ERR_INVALID;
    HIPCHK(hipSetDevice(c->device));
    Dump D{dump->radiance, dump->lambda_, dump->raster, dump->delta,
           reinterpret_cast<unsigned long long*>(dump->depth)};
    if (c->debug_sampler == LUMO_SAMPLER_SOBOL && task->total_samples > 1023) return LUMO_ERR_INVALID;
    if (c->debug_integrator == LUMO_INTEGRATOR_BDPT && c->has_camera && c->cam.orthographic) return LUMO_ERR_UNSUPPORTED;
    c->integrator = c->debug_integrator;
    c->sampler = c->debug_sampler;
    const lumo_status st = render_impl(*c, task, 1, nullptr, &D, task->samples);
    c->integrator = LUMO_INTEGRATOR_PATH_TRACE;
    c->sampler = LUMO_SAMPLER_MULTI_JITTERED;
    return st;
}

// Feature planes of n tasks (features.h); the sampler applies to this call only.
lumo_status lumo_render_features(void* ctx, const lumo_tile_task* tasks, size_t n, const lumo_feature_cfg* cfg,
                                 lumo_feature_planes* out) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c || (!tasks && n) || (!out && n)) return LUMO_ERR_INVALID;
    const int sampler = cfg ? cfg->sampler : LUMO_SAMPLER_MULTI_JITTERED;
    if (sampler < LUMO_SAMPLER_MULTI_JITTERED || sampler > LUMO_SAMPLER_SOBOL) return LUMO_ERR_INVALID;
    for (size_t i = 0; i < n && sampler == LUMO_SAMPLER_SOBOL; ++i)
        if (tasks[i].total_samples > 1023) return LUMO_ERR_INVALID;  // sobol_seq.rs SOBOL_MAX_LEN (lumo panics)
    HIPCHK(hipSetDevice(c->device));
    const size_t max_paths = (cfg && cfg->max_paths > 0) ? (size_t)cfg->max_paths : (size_t)1 << 30;
    c->sampler = sampler;
    lumo_status st = LUMO_OK;
    if (n == 0) st = render_features_impl(*c, tasks, 0, out, nullptr);  // the scene and camera checks
    for (size_t i = 0; i < n && !st;) {
        const size_t j = chunk_end(tasks, n, i, max_paths);
        st = render_features_impl(*c, tasks + i, j - i, out + i, nullptr);
        i = j;
    }
    c->sampler = LUMO_SAMPLER_MULTI_JITTERED;
    return st;
}

// Test hook: the per-sample feature records of one task, with lumo_debug_set_sampler's sampler.
lumo_status lumo_debug_features(void* ctx, const lumo_tile_task* task, lumo_feature_dump* dump) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c || !task || !dump) return LUMO_ERR_INVALID;
    if (c->debug_sampler == LUMO_SAMPLER_SOBOL && task->total_samples > 1023) return LUMO_ERR_INVALID;
    HIPCHK(hipSetDevice(c->device));
    c->sampler = c->debug_sampler;
    const lumo_status st = render_features_impl(*c, task, 1, nullptr, dump);
    c->sampler = LUMO_SAMPLER_MULTI_JITTERED;
    return st;
}

// Pixel sampler used by lumo_debug_paths (test hook).
lumo_status lumo_debug_set_sampler(void* ctx, int sampler) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c || sampler < LUMO_SAMPLER_MULTI_JITTERED || sampler > LUMO_SAMPLER_SOBOL) return LUMO_ERR_INVALID;
    c->debug_sampler = sampler;
    return LUMO_OK;
}

// Integrator used by lumo_debug_paths (test hook; BDPT splats are not collected there).
lumo_status lumo_debug_set_integrator(void* ctx, int integrator) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c || (integrator != LUMO_INTEGRATOR_PATH_TRACE && integrator != LUMO_INTEGRATOR_BDPT)) return LUMO_ERR_INVALID;
    c->debug_integrator = integrator;
    return LUMO_OK;
}

}  // extern "C"
