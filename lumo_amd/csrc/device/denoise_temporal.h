// The temporal denoiser's kernels (lumo_denoise_temporal; include/lumo_amd.h gives the definition
// operation by operation, DESIGN.md §4e the design).  Included by denoise.hip alone.
//
//   k_dn_reproject  steps 2-5: a pixel's world position, its raster point in the previous frame,
//                   the bilinear (else 3 x 3) gather of the previous call's history, the blend
//   k_dn_tvar       step 6, one thread per pixel: the temporal variance where the history is long
//   k_dn_history    one thread per pixel: the feedback iteration's colour into the history
//   k_dn_motion     lumo_denoise_temporal_motion only: the per-pixel motion m that k_dn_reproject<true>
//                   adds to the world position before it projects it (DESIGN.md §4g "Motion")
//
// The history is double-buffered (DtHist prev / next): k_dn_reproject reads `prev` at positions that
// follow from the camera's motion while it and k_dn_history write `next`, so no kernel reads a plane
// the same call has written.  Planes are structure-of-arrays as denoise.h's.
//
// k_dn_reproject.  A pixel gathers 4 (or 9) history pixels of 11 values each; neighbouring pixels
// share most of them.  A block owns DT_BX x DT_BY = 32 x 8 pixels: 32 lanes along x read and write
// the current planes in 256-byte row segments, and 8 rows keep the footprint in the previous frame
// near square, so that its bounding box grows slowly when the camera rolls (32 x 8 rotated by t
// covers (32 cos t + 8 sin t) x (32 sin t + 8 cos t); a 64 x 4 block would load 67 x 7 = 469 history
// pixels for its 256 at rest, this one 35 x 11 = 385).  Every lane computes its q; the block reduces
// the bounding box of all its taps (the bilinear 2 x 2 widened to the 3 x 3 fallback's reach,
// x0 - 1 .. x0 + 2) with wave shuffles and one LDS step.  A box of at most DT_CAP pixels is staged
// in LDS row by row, coalesced, and every lane taps from there; a larger one (a strong roll, a zoom
// out, a block astride a depth edge whose halves move apart) takes the direct form, the same
// dt_gather reading global memory.  One function, two sources: the same operations in the same
// order, hence the same bits.  DT_CAP = 768 pixels x 80 bytes = 60 KiB: two blocks share a CU's
// 160 KiB.  Images narrower than a wave or shorter than a block run the same code: lanes outside
// the image take part in the reduction and the staging and write nothing.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "../common/vec.h"
#include "denoise.h"

namespace lumo {
namespace dev {

constexpr int DT_BX = 32, DT_BY = 8, DT_THREADS = DT_BX * DT_BY;
constexpr int DT_CAP = 768;  // history pixels a block's LDS tile holds
enum { DT_E = 0, DT_M1 = 3, DT_M2 = 4, DT_N = 5, DT_Z = 8, DT_NV = 9 };  // the history's f64 planes
enum { DT_CNT_WITH = 0, DT_CNT_WITHOUT, DT_CNT_STAGED, DT_CNT_DIRECT, DT_CNT_N };

struct DtHist {
    double* v[DT_NV];
    uint32_t *len, *hit;
};
struct DtCam {
    Xform wtc, sctr, cts;
};
// lumo_temporal_cfg as the kernels take it (validated); has_prev = 0: a first frame
struct DtCfg {
    double alpha, normal_cos_min, depth_rel_max;
    int max_history, min_history, stage_lds, has_prev;
};

// Step 1's addition of lumo_denoise_temporal_motion, one thread per pixel: m = motion_w[0..2] /
// depth_w[1] (0 where no sample hit) into three planes of n doubles.
__global__ __launch_bounds__(256) void k_dn_motion(const double* motion_w, const double* depth_w, double* m, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int k = 0; k < 3; ++k) m[(size_t)k * n + i] = dn_ratio(motion_w[4 * i + k], depth_w[4 * i + 1]);
}

// Steps 2 and 3 and step 4's u, v: false when the pixel has no history whatever the taps hold.
// MOTION: the point is carried back by the pixel's motion m first (P' = P + m); without it m is unused
// and nothing is added.
template <bool MOTION>
__device__ __forceinline__ bool dt_project(const DtCam& cur, const DtCam& prv, int x, int y, double z, V3 m, int W, int H,
                                           double& u, double& v, double& zp) {
    const V3 screen = xf_pt_inv(cur.sctr, V3{(double)x + 0.5, (double)y + 0.5, 0.0});
    const V3 cpt = xf_pt_inv(cur.cts, screen);
    const V3 o = xf_pt_inv(cur.wtc, V3{0.0, 0.0, 0.0});
    const V3 d = normalize(xf_dir_inv(cur.wtc, normalize(cpt)));
    V3 P = o + z * d;
    if constexpr (MOTION) P = P + m;
    const V3 cp = xf_pt(prv.wtc, P);
    if (!(cp.z > 0.0)) return false;
    const V3 q = xf_pt(prv.sctr, xf_pt(prv.cts, cp));
    if (!isfinite(q.x) || !isfinite(q.y)) return false;
    u = q.x - 0.5, v = q.y - 0.5;
    // farther out no tap of either pattern lies inside the image (and floor() stays an int)
    if (!(u >= -2.0 && u < (double)W + 1.0 && v >= -2.0 && v < (double)H + 1.0)) return false;
    zp = distance(P, xf_pt_inv(prv.wtc, V3{0.0, 0.0, 0.0}));
    return true;
}

// The two sources of a tap: value k (a DT_* plane), length and hit flag of history pixel (x, y),
// which lies inside the image (and, for the tile, inside the block's box).
struct DtGlobal {
    DtHist h;
    int W;
    __device__ __forceinline__ size_t at(int x, int y) const { return (size_t)y * W + x; }
    __device__ __forceinline__ double val(int k, size_t i) const { return h.v[k][i]; }
    __device__ __forceinline__ uint32_t len(size_t i) const { return h.len[i]; }
    __device__ __forceinline__ uint32_t hit(size_t i) const { return h.hit[i]; }
};
struct DtTile {
    const double* v;  // DT_NV planes of DT_CAP
    const uint32_t *l, *h;
    int bx0, by0, bw;
    __device__ __forceinline__ size_t at(int x, int y) const { return (size_t)((y - by0) * bw + (x - bx0)); }
    __device__ __forceinline__ double val(int k, size_t i) const { return v[k * DT_CAP + i]; }
    __device__ __forceinline__ uint32_t len(size_t i) const { return l[i]; }
    __device__ __forceinline__ uint32_t hit(size_t i) const { return h[i]; }
};

// Step 4: the history of e0..2, m1, m2 into hist[] and its length; false: none.
template <class Src>
__device__ __forceinline__ bool dt_gather(const Src& S, const DtCfg& cfg, const DnGuide& p, double u, double v, double zp,
                                          int W, int H, double (&hist)[5], uint32_t& len) {
    double sw = 0.0, s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    uint32_t best = 0;
    auto tap = [&](int xt, int yt, double w) {
        if (xt < 0 || xt >= W || yt < 0 || yt >= H) return;
        const size_t i = S.at(xt, yt);
        if (!S.hit(i)) return;
        const double c = (p.n[0] * S.val(DT_N, i) + p.n[1] * S.val(DT_N + 1, i)) + p.n[2] * S.val(DT_N + 2, i);
        if (!(c >= cfg.normal_cos_min)) return;
        if (!(fabs(S.val(DT_Z, i) - zp) <= cfg.depth_rel_max * zp)) return;
        sw = sw + w;
        for (int k = 0; k < 5; ++k) s[k] = s[k] + w * S.val(DT_E + k, i);
        const uint32_t l = S.len(i);
        best = l > best ? l : best;
    };
    const double fu = floor(u), fv = floor(v);
    const int x0 = (int)fu, y0 = (int)fv;
    const double wx[2] = {1.0 - (u - fu), u - fu}, wy[2] = {1.0 - (v - fv), v - fv};
    for (int j = 0; j < 2; ++j)
        for (int i = 0; i < 2; ++i) tap(x0 + i, y0 + j, wx[i] * wy[j]);
    if (!(sw > 0.0)) {
        sw = 0.0, best = 0;
        for (int k = 0; k < 5; ++k) s[k] = 0.0;
        const int cx = (int)floor(u + 0.5), cy = (int)floor(v + 0.5);
        for (int j = -1; j <= 1; ++j)
            for (int i = -1; i <= 1; ++i) tap(cx + i, cy + j, 1.0);
        if (!(sw > 0.0)) return false;
    }
    for (int k = 0; k < 5; ++k) hist[k] = s[k] / sw;
    len = best;
    return true;
}

// Steps 2-5.  Reads P's guides, l and e[0] (k_dn_prepare's) and the history `prev`; writes e_acc to
// P.e[0], its luminance to P.l (step 6's input), and m1, m2, N, n, z, hit to `next`.  cnt: DT_CNT_*.
// MOTION: mot holds k_dn_motion's three planes; else it is not read.
template <bool MOTION>
__global__ __launch_bounds__(DT_THREADS) void k_dn_reproject(DnPlanes P, DtHist prev, DtHist next, DtCam cur, DtCam prv,
                                                             DtCfg cfg, unsigned long long* cnt, int W, int H,
                                                             const double* mot) {
    __shared__ double tile[DT_NV * DT_CAP];
    __shared__ uint32_t tile_len[DT_CAP], tile_hit[DT_CAP];
    __shared__ int wave_box[DT_THREADS / 64][4];
    const int tid = (int)threadIdx.x, tiles_x = (W + DT_BX - 1) / DT_BX;
    const int x = (int)(blockIdx.x % tiles_x) * DT_BX + tid % DT_BX, y = (int)(blockIdx.x / tiles_x) * DT_BY + tid / DT_BX;
    const bool inside = x < W && y < H;
    const size_t i = inside ? (size_t)y * W + x : 0;

    DnGuide p{{0.0, 0.0, 0.0}, 0.0, 0u};
    double u = 0.0, v = 0.0, zp = 0.0;
    bool cand = false;  // the pixel's taps decide whether it has history
    if (inside) {
        p = DnGuide{{P.n[0][i], P.n[1][i], P.n[2][i]}, P.z[i], P.hit[i]};
        V3 m{0.0, 0.0, 0.0};
        if constexpr (MOTION) {
            const size_t n = (size_t)W * H;
            m = V3{mot[i], mot[n + i], mot[2 * n + i]};
        }
        cand = cfg.has_prev && p.hit && dt_project<MOTION>(cur, prv, x, y, p.z, m, W, H, u, v, zp);
    }
    // the box of the block's taps: x0 - 1 .. x0 + 2 covers the 2 x 2 and the 3 x 3 around x0 or x0 + 1
    int box[4] = {INT_MAX, INT_MAX, INT_MIN, INT_MIN};  // min x, min y, max x, max y
    if (cand) {
        const int x0 = (int)floor(u), y0 = (int)floor(v);
        box[0] = x0 - 1, box[1] = y0 - 1, box[2] = x0 + 2, box[3] = y0 + 2;
    }
    for (int o = 32; o > 0; o >>= 1)
        for (int k = 0; k < 4; ++k) {
            const int other = __shfl_xor(box[k], o);
            box[k] = k < 2 ? (other < box[k] ? other : box[k]) : (other > box[k] ? other : box[k]);
        }
    if (tid % 64 == 0)
        for (int k = 0; k < 4; ++k) wave_box[tid / 64][k] = box[k];
    __syncthreads();
    for (int w = 0; w < DT_THREADS / 64; ++w)
        for (int k = 0; k < 4; ++k) {
            const int other = wave_box[w][k];
            box[k] = k < 2 ? (other < box[k] ? other : box[k]) : (other > box[k] ? other : box[k]);
        }
    const bool any = box[0] <= box[2];
    const int bx0 = box[0] > 0 ? box[0] : 0, by0 = box[1] > 0 ? box[1] : 0;
    const int bx1 = box[2] < W - 1 ? box[2] : W - 1, by1 = box[3] < H - 1 ? box[3] : H - 1;
    const int bw = any && bx1 >= bx0 ? bx1 - bx0 + 1 : 0, bh = any && by1 >= by0 ? by1 - by0 + 1 : 0;
    const long long box_px = (long long)bw * bh;  // 0: no pixel of the block has a tap to read
    const bool staged = cfg.stage_lds && box_px > 0 && box_px <= DT_CAP;  // the same for the whole block

    if (staged) {
        for (int t = tid; t < (int)box_px; t += DT_THREADS) {
            const size_t g = (size_t)(by0 + t / bw) * W + (size_t)(bx0 + t % bw);
            for (int k = 0; k < DT_NV; ++k) tile[k * DT_CAP + t] = prev.v[k][g];
            tile_len[t] = prev.len[g];
            tile_hit[t] = prev.hit[g];
        }
        __syncthreads();
    }
    double hist[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    uint32_t len = 0;
    bool found = false;
    if (cand)
        found = staged ? dt_gather(DtTile{tile, tile_len, tile_hit, bx0, by0, bw}, cfg, p, u, v, zp, W, H, hist, len)
                       : dt_gather(DtGlobal{prev, W}, cfg, p, u, v, zp, W, H, hist, len);
    if (inside) {
        const double l = P.l[i];
        double xin[5] = {P.e[0][0][i], P.e[0][1][i], P.e[0][2][i], l, l * l};
        uint32_t N = 1;
        if (found) {
            N = len + 1 < (uint32_t)cfg.max_history ? len + 1 : (uint32_t)cfg.max_history;
            const double r = 1.0 / (double)N, a = cfg.alpha > r ? cfg.alpha : r;
            for (int k = 0; k < 5; ++k) xin[k] = (1.0 - a) * hist[k] + a * xin[k];
            for (int k = 0; k < 3; ++k) P.e[0][k][i] = xin[k];
            P.l[i] = dn_lum(xin[0], xin[1], xin[2]);
        }
        next.v[DT_M1][i] = xin[3];
        next.v[DT_M2][i] = xin[4];
        next.len[i] = N;
        for (int k = 0; k < 3; ++k) next.v[DT_N + k][i] = p.n[k];
        next.v[DT_Z][i] = p.z;
        next.hit[i] = p.hit;
    }
    const unsigned long long with = __popcll(__ballot(found)), without = __popcll(__ballot(inside && !found));
    if (tid % 64 == 0) {
        if (with) atomicAdd(&cnt[DT_CNT_WITH], with);
        if (without) atomicAdd(&cnt[DT_CNT_WITHOUT], without);
    }
    if (tid == 0 && box_px > 0) atomicAdd(&cnt[staged ? DT_CNT_STAGED : DT_CNT_DIRECT], 1ull);  // a block that tapped
}

// Step 6: where the history is long enough the accumulated moments replace k_dn_variance's estimate.
__global__ __launch_bounds__(256) void k_dn_tvar(DnPlanes P, DtHist next, int min_history, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || next.len[i] < (uint32_t)min_history) return;
    const double m1 = next.v[DT_M1][i], v = next.v[DT_M2][i] - m1 * m1;
    P.var[0][i] = v > 0.0 ? v : 0.0;
}

// Step 7's feedback: colour set `set` (the feedback iteration's output) becomes the colour history.
__global__ __launch_bounds__(256) void k_dn_history(DnPlanes P, int set, DtHist next, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int k = 0; k < 3; ++k) next.v[DT_E + k][i] = P.e[set][k][i];
}

}  // namespace dev
}  // namespace lumo
