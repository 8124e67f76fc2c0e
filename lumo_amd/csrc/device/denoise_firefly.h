// The denoiser's firefly clamp (step 1b of lumo_denoise and lumo_denoise_temporal; include/lumo_amd.h
// gives the definition operation by operation, DESIGN.md §4f the design).  Included by denoise.hip alone.
//
//   k_dn_firefly        (2R+1)^2 window at unit stride: the rank-th largest luminance among a hit
//                       pixel's alike neighbours bounds its own; writes the pixel's factor g
//   k_dn_firefly_apply  one thread per pixel: where g is not 1, c g -> e and l, as k_dn_prepare
//
// A neighbour must see step 1's l whatever the clamp does to it, and blocks run in any order, so
// the window kernel changes no plane it or another block stages: it writes only g (1.0 where the
// pixel stays) to a plane that is free between prepare and the first a-trous iteration, and the
// streaming kernel that follows rewrites e and l of the clamped pixels from the input planes, which
// are still resident, with k_dn_prepare's operations.
//
// The window kernel is k_dn_variance's march (DnMarch<3> at step 1, the same five planes and the
// hit flags in the ring, the radius a kernel argument), so it has that kernel's LDS footprint and
// bounds logic.  The order statistic needs no sort: a lane keeps the DF_TOP = 8 largest luminances
// it has met in a sorted register array, and a new value is passed down the array by
// compare-exchange (the larger stays, the smaller moves on; what leaves the end is dropped).  The
// array is indexed by unrolled constants only, so it lives in 16 VGPRs and nothing goes to
// scratch; the rank-th entry is picked by a chain of selects.  Ties are values: whichever of two
// equal luminances stays, the array holds the same numbers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "denoise.h"

namespace lumo {
namespace dev {

constexpr int DF_R = 3, DF_NV = 5;  // the widest window; ring planes l, n (3), z
constexpr int DF_TOP = 8;           // the largest rank

// lumo_firefly_cfg as the kernel takes it (validated)
struct DfCfg {
    double gain, normal_cos_min, depth_rel_max;
    int radius, rank, min_alike;
};

// `v` into the descending array `t`
__device__ __forceinline__ void df_insert(double (&t)[DF_TOP], double v) {
#pragma unroll
    for (int i = 0; i < DF_TOP; ++i) {
        const bool up = v > t[i];
        const double hi = up ? v : t[i], lo = up ? t[i] : v;
        t[i] = hi;
        v = lo;
    }
}

// Step 1b's decision.  g: one double per pixel; clamped: the count of pixels with l > b.
__global__ __launch_bounds__(DN_BW) void k_dn_firefly(DnPlanes P, DfCfg cfg, double* g, unsigned long long* clamped,
                                                      int W, int H) {
    extern __shared__ double dn_lds[];
    __shared__ unsigned wave_count[DN_BW / 64];
    DnMarch<DF_R> m;
    if (!m.init(W, H, 1)) return;
    double* ring = dn_lds;
    uint32_t* ring_hit = reinterpret_cast<uint32_t*>(ring + (size_t)m.RING * DF_NV * m.wl);
    const double* const src[DF_NV] = {P.l, P.n[0], P.n[1], P.n[2], P.z};
    auto at = [&](int j, int x, int k) { return ring[(size_t)(m.slot(j) * DF_NV + k) * m.wl + m.col(x)]; };
    const int x = m.x0 + (int)threadIdx.x;
    const int radius = cfg.radius;
    unsigned count = 0;  // of the wave, the same in all its lanes
    for (int j = m.j0 - DF_R; j < m.j0 + DF_R; ++j) m.load_row(j, src, P.hit, ring, ring_hit);
    for (int j = m.j0; j < m.j1; ++j) {
        m.load_row(j + DF_R, src, P.hit, ring, ring_hit);
        __syncthreads();
        bool over = false;
        if (x < W) {
            double gp = 1.0;
            if (ring_hit[m.slot(j) * m.wl + m.col(x)]) {
                const double lp = at(j, x, 0), np[3] = {at(j, x, 1), at(j, x, 2), at(j, x, 3)}, zp = at(j, x, 4);
                const double zmax = cfg.depth_rel_max * zp;
                double top[DF_TOP];
#pragma unroll
                for (int i = 0; i < DF_TOP; ++i) top[i] = -INFINITY;
                int alike = 0;
                for (int dy = -radius; dy <= radius; ++dy) {
                    if (!m.row_in(j + dy)) continue;
                    for (int dx = -radius; dx <= radius; ++dx) {
                        if (!m.col_in(x + dx) || (dx == 0 && dy == 0)) continue;
                        if (!ring_hit[m.slot(j + dy) * m.wl + m.col(x + dx)]) continue;
                        const double d = (np[0] * at(j + dy, x + dx, 1) + np[1] * at(j + dy, x + dx, 2)) +
                                         np[2] * at(j + dy, x + dx, 3);
                        if (!(d >= cfg.normal_cos_min)) continue;
                        if (!(fabs(at(j + dy, x + dx, 4) - zp) <= zmax)) continue;
                        ++alike;
                        df_insert(top, at(j + dy, x + dx, 0));
                    }
                }
                if (alike >= cfg.min_alike) {
                    double v = top[0];  // the rank-th largest
#pragma unroll
                    for (int i = 1; i < DF_TOP; ++i) v = i < cfg.rank ? top[i] : v;
                    const double b = cfg.gain * v;
                    if (lp > b) {
                        gp = b / lp;
                        over = true;
                    }
                }
            }
            g[(size_t)m.y_of(j) * W + x] = gp;
        }
        count += (unsigned)__popcll(__ballot(over));
        __syncthreads();  // the next row replaces row j - R
    }
    if (threadIdx.x % 64 == 0) wave_count[threadIdx.x / 64] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = 0;
        for (int w = 0; w < DN_BW / 64; ++w) total += wave_count[w];
        if (total) atomicAdd(clamped, total);
    }
}

// Step 1b's effect on a clamped pixel: c as k_dn_prepare computes it, scaled, demodulated by the
// divisor that kernel stored.  A pixel with g = 1 keeps the e and l it has (c 1 = c).
__global__ __launch_bounds__(256) void k_dn_firefly_apply(const double* rgb_w, const double* add_rgb, DnPlanes P,
                                                          const double* g, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double gi = g[i];
    if (gi == 1.0) return;
    double e[3];
    for (int k = 0; k < 3; ++k) {
        double c = dn_ratio(rgb_w[4 * i + k], rgb_w[4 * i + 3]);
        if (add_rgb) c = c + add_rgb[3 * i + k];
        c = c * gi;
        e[k] = c / P.div[k][i];
        P.e[0][k][i] = e[k];
    }
    P.l[i] = dn_lum(e[0], e[1], e[2]);
}

}  // namespace dev
}  // namespace lumo
