// The denoiser's kernels: an edge-avoiding a-trous wavelet filter guided by the feature planes,
// with albedo demodulation and a spatial variance estimate (the spatial part of SVGF; DESIGN.md
// §4d gives the definition operation by operation).  Included by denoise.hip alone.
//
// All arithmetic is f64, written as the definition writes it and never contracted to an FMA, so a
// numpy restatement with the same exp (lm_exp) reproduces the result bit for bit.
//
// Planes are structure-of-arrays, one double per pixel, so that a wave's 64 lanes (64 consecutive
// x of one image row) read one contiguous row segment per plane.
//   k_dn_prepare   one thread per pixel: the frame's four input planes -> colour, guides, divisor
//   k_dn_variance  (2r+1)^2 window at unit stride: the luminance's weighted variance
//   k_dn_atrous    one iteration at step s: 5 x 5 taps at (s dx, s dy)
//   k_dn_finish    one thread per pixel: remodulate, interleave
//
// The two window kernels share one shape (DnMarch).  In y a block owns rows of one residue class
// mod s: the 2R+1 rows a centre row's taps touch are then consecutive rows of that sub-lattice,
// and the block marches down DN_ROWS of them with the live 2R+1 in an LDS ring, so a row is loaded
// once per march and not once per output row.  In x the ring holds the block's DN_BW centres and
// the R s columns on either side.  What only the centre needs (the depth slope, the variance's 3 x 3
// binomial, the per-centre parts of the weights' denominators) stays in registers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../common/lmath.h"

namespace lumo {
namespace dev {

constexpr int DN_BW = 128;   // centres per block along x: two waves
constexpr int DN_ROWS = 16;  // sub-lattice rows a block marches over (it loads DN_ROWS + 2R)
constexpr int DN_MAX_ITER = 5;  // steps 1, 2, 4, 8, 16

// The filter's constants as the kernels take them (lumo_denoise_cfg, validated).
struct DnCfg {
    double sigma_l, sigma_z, albedo_floor, depth_floor, lum_floor;
    int k, demodulate;
};

// The work planes of a frame of P pixels.
struct DnPlanes {
    double *n[3], *z, *fz, *div[3], *l;  // guides, depth slope, demodulation divisor, first luminance
    uint32_t* hit;
    double *e[2][3], *var[2];            // irradiance and variance, ping-pong
};

__device__ __forceinline__ double dn_ratio(double a, double b) { return b == 0.0 ? 0.0 : a / b; }
__device__ __forceinline__ double dn_max(double x, double floor_) { return x > floor_ ? x : floor_; }  // NaN -> floor
__device__ __forceinline__ double dn_lum(double e0, double e1, double e2) {
    return (0.2126 * e0 + 0.7152 * e1) + 0.0722 * e2;
}
__device__ __forceinline__ int dn_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }
// depth of pixel i from its depth_w record (sum w t hit, sum w hit, 0, sum w)
__device__ __forceinline__ double dn_depth(const double* depth_w, size_t i) {
    return dn_ratio(depth_w[4 * i], depth_w[4 * i + 1]);
}

// Step 1.  Reads the four input planes (4 doubles per pixel) and the optional add_rgb (3 per pixel).
__global__ __launch_bounds__(256) void k_dn_prepare(const double* rgb_w, const double* albedo_w, const double* normal_w,
                                                    const double* depth_w, const double* add_rgb, DnPlanes P, DnCfg cfg,
                                                    int W, int H) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)W * H) return;
    const int x = (int)(i % W), y = (int)(i / W);
    const double cov = dn_ratio(depth_w[4 * i + 1], depth_w[4 * i + 3]);
    const double z = dn_depth(depth_w, i);
    const double zx = dn_depth(depth_w, (size_t)y * W + dn_clamp(x + 1, W));
    const double zy = dn_depth(depth_w, (size_t)dn_clamp(y + 1, H) * W + x);
    const double ax = fabs(zx - z), ay = fabs(zy - z);
    P.z[i] = z;
    P.fz[i] = ax > ay ? ax : ay;
    P.hit[i] = cov > 0.0 ? 1u : 0u;
    const double nx = normal_w[4 * i], ny = normal_w[4 * i + 1], nz = normal_w[4 * i + 2];
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    P.n[0][i] = dn_ratio(nx, len);
    P.n[1][i] = dn_ratio(ny, len);
    P.n[2][i] = dn_ratio(nz, len);
    double e[3];
    for (int k = 0; k < 3; ++k) {
        double c = dn_ratio(rgb_w[4 * i + k], rgb_w[4 * i + 3]);
        if (add_rgb) c = c + add_rgb[3 * i + k];
        const double a = dn_ratio(albedo_w[4 * i + k], albedo_w[4 * i + 3]);
        const double div = cfg.demodulate ? dn_max(a + (1.0 - cov), cfg.albedo_floor) : 1.0;
        P.div[k][i] = div;
        e[k] = c / div;
        P.e[0][k][i] = e[k];
    }
    P.l[i] = dn_lum(e[0], e[1], e[2]);
}

// ------------------------------------------------------------------------------------------------
// The march of one block and all of its bounds logic: which sub-lattice rows and image columns
// exist (a tap outside the image is skipped), where a row or column lives in the ring.  Images
// narrower than a wave or shorter than a ring need nothing special: rows and columns that do not
// exist are neither loaded nor read.
template <int R>
struct DnMarch {
    static constexpr int RING = 2 * R + 1;
    int W, H, s;
    int x0;      // image x of the block's first centre
    int wl;      // ring width: DN_BW + 2 R s columns, ring column c is image x0 - R s + c
    int r;       // the block's rows are y = r + j s
    int nj;      // sub-lattice rows in the image
    int j0, j1;  // the block's centre rows [j0, j1)

    // false: the block has no row (the grid is sized for the fullest residue class)
    __device__ bool init(int W_, int H_, int s_) {
        W = W_, H = H_, s = s_;
        x0 = (int)blockIdx.x * DN_BW;
        wl = DN_BW + 2 * R * s;
        const int chunks = (int)gridDim.y / s;
        r = (int)blockIdx.y / chunks;
        nj = r < H ? (H - r + s - 1) / s : 0;
        j0 = ((int)blockIdx.y % chunks) * DN_ROWS;
        j1 = j0 + DN_ROWS < nj ? j0 + DN_ROWS : nj;
        return j0 < j1;
    }
    __device__ int y_of(int j) const { return r + j * s; }
    __device__ bool row_in(int j) const { return j >= 0 && j < nj; }
    __device__ bool col_in(int x) const { return x >= 0 && x < W; }
    __device__ int slot(int j) const { return (j + RING) % RING; }  // j >= -R
    __device__ int col(int x) const { return x - (x0 - R * s); }

    // Row j of the sub-lattice into its ring slot: NV planes and the hit flags.  Coalesced: the
    // block's threads take consecutive ring columns.
    template <int NV>
    __device__ void load_row(int j, const double* const (&src)[NV], const uint32_t* hit, double* ring,
                             uint32_t* ring_hit) const {
        if (!row_in(j)) return;
        const size_t row = (size_t)y_of(j) * W;
        const int sl = slot(j);
        for (int c = (int)threadIdx.x; c < wl; c += DN_BW) {
            const int x = x0 - R * s + c;
            if (!col_in(x)) continue;
            for (int k = 0; k < NV; ++k) ring[(size_t)(sl * NV + k) * wl + c] = src[k][row + x];
            ring_hit[sl * wl + c] = hit[row + x];
        }
    }
    // LDS bytes of a block: RING rows of NV doubles and a flag per column
    static size_t lds_bytes(int s, int nv) { return (size_t)RING * (DN_BW + 2 * R * s) * (nv * sizeof(double) + sizeof(uint32_t)); }
};

// Step 2: the guides' weight of tap q for centre p at pixel offset (ox, oy).  False: the weight is
// 0 (exactly one of the two is a hit).  `zden_a` = sigma_z fz_p and `zden_b` = depth_floor z_p are
// the centre's parts of dz's denominator.
struct DnGuide {
    double n[3], z;
    uint32_t hit;
};
__device__ __forceinline__ bool dn_pair(const DnGuide& p, const DnGuide& q, int ox, int oy, double zden_a, double zden_b,
                                        int k, double& wn, double& dz) {
    wn = 1.0, dz = 0.0;
    if (!p.hit && !q.hit) return true;
    if (p.hit != q.hit) return false;
    double d = (p.n[0] * q.n[0] + p.n[1] * q.n[1]) + p.n[2] * q.n[2];
    d = d > 0.0 ? d : 0.0;
    for (int i = 0; i < k; ++i) d = d * d;
    wn = d;
    const double fx = (double)ox, fy = (double)oy;
    dz = fabs(p.z - q.z) / (zden_a * sqrt(fx * fx + fy * fy) + zden_b);
    return true;
}
__device__ __forceinline__ double dn_falloff(double m) { return lm_exp(-(m < 700.0 ? m : 700.0)); }  // NaN -> 700

// Step 3.  Ring planes: l, n (3), z.
constexpr int DN_VAR_R = 3, DN_VAR_NV = 5;
__global__ __launch_bounds__(DN_BW) void k_dn_variance(DnPlanes P, DnCfg cfg, int radius, int W, int H) {
    extern __shared__ double dn_lds[];
    DnMarch<DN_VAR_R> m;
    if (!m.init(W, H, 1)) return;
    double* ring = dn_lds;
    uint32_t* ring_hit = reinterpret_cast<uint32_t*>(ring + (size_t)m.RING * DN_VAR_NV * m.wl);
    const double* const src[DN_VAR_NV] = {P.l, P.n[0], P.n[1], P.n[2], P.z};
    auto at = [&](int j, int x, int k) { return ring[(size_t)(m.slot(j) * DN_VAR_NV + k) * m.wl + m.col(x)]; };
    auto guide = [&](int j, int x) {
        return DnGuide{{at(j, x, 1), at(j, x, 2), at(j, x, 3)}, at(j, x, 4), ring_hit[m.slot(j) * m.wl + m.col(x)]};
    };
    const int x = m.x0 + (int)threadIdx.x;
    for (int j = m.j0 - DN_VAR_R; j < m.j0 + DN_VAR_R; ++j) m.load_row(j, src, P.hit, ring, ring_hit);
    for (int j = m.j0; j < m.j1; ++j) {
        m.load_row(j + DN_VAR_R, src, P.hit, ring, ring_hit);
        __syncthreads();
        if (x < W) {
            const size_t i = (size_t)m.y_of(j) * W + x;
            const DnGuide p = guide(j, x);
            const double za = cfg.sigma_z * P.fz[i], zb = cfg.depth_floor * p.z;
            double sw = 0.0, s1 = 0.0, s2 = 0.0;
            for (int dy = -radius; dy <= radius; ++dy) {
                if (!m.row_in(j + dy)) continue;
                for (int dx = -radius; dx <= radius; ++dx) {
                    if (!m.col_in(x + dx)) continue;
                    const double lq = at(j + dy, x + dx, 0);
                    double w = 1.0;
                    if (dx != 0 || dy != 0) {
                        double wn, dz;
                        if (!dn_pair(p, guide(j + dy, x + dx), dx, dy, za, zb, cfg.k, wn, dz)) continue;
                        w = wn * dn_falloff(dz);
                    }
                    sw = sw + w;
                    s1 = s1 + w * lq;
                    s2 = s2 + w * (lq * lq);
                }
            }
            const double m1 = s1 / sw, m2 = s2 / sw;
            const double v = m2 - m1 * m1;
            P.var[0][i] = v > 0.0 ? v : 0.0;
        }
        __syncthreads();  // the next row replaces row j - R
    }
}

// Step 4, one iteration: reads set `from`, writes the other.  Ring planes: e (3), var, n (3), z.
constexpr int DN_AT_R = 2, DN_AT_NV = 8;
__global__ __launch_bounds__(DN_BW) void k_dn_atrous(DnPlanes P, DnCfg cfg, int from, int s, int W, int H) {
    extern __shared__ double dn_lds[];
    DnMarch<DN_AT_R> m;
    if (!m.init(W, H, s)) return;
    double* ring = dn_lds;
    uint32_t* ring_hit = reinterpret_cast<uint32_t*>(ring + (size_t)m.RING * DN_AT_NV * m.wl);
    const double* const src[DN_AT_NV] = {P.e[from][0], P.e[from][1], P.e[from][2], P.var[from], P.n[0], P.n[1], P.n[2], P.z};
    const double* var = P.var[from];
    auto at = [&](int j, int x, int k) { return ring[(size_t)(m.slot(j) * DN_AT_NV + k) * m.wl + m.col(x)]; };
    auto guide = [&](int j, int x) {
        return DnGuide{{at(j, x, 4), at(j, x, 5), at(j, x, 6)}, at(j, x, 7), ring_hit[m.slot(j) * m.wl + m.col(x)]};
    };
    const double b[5] = {1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};
    const double g[3] = {1.0 / 4.0, 1.0 / 2.0, 1.0 / 4.0};  // the 3 x 3 binomial's factors
    const int x = m.x0 + (int)threadIdx.x;
    for (int j = m.j0 - DN_AT_R; j < m.j0 + DN_AT_R; ++j) m.load_row(j, src, P.hit, ring, ring_hit);
    for (int j = m.j0; j < m.j1; ++j) {
        m.load_row(j + DN_AT_R, src, P.hit, ring, ring_hit);
        __syncthreads();
        if (x < W) {
            const int y = m.y_of(j);
            const size_t i = (size_t)y * W + x;
            const DnGuide p = guide(j, x);
            const double lp = dn_lum(at(j, x, 0), at(j, x, 1), at(j, x, 2));
            double gv = 0.0;  // unit stride whatever the step: from HBM / L2, coordinates clamped
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx)
                    gv = gv + (g[dy + 1] * g[dx + 1]) * var[(size_t)dn_clamp(y + dy, H) * W + dn_clamp(x + dx, W)];
            const double lden = cfg.sigma_l * sqrt(gv) + cfg.lum_floor;
            const double za = cfg.sigma_z * P.fz[i], zb = cfg.depth_floor * p.z;
            double sw = 0.0, se[3] = {0.0, 0.0, 0.0}, sv = 0.0;
            for (int dy = -2; dy <= 2; ++dy) {
                if (!m.row_in(j + dy)) continue;
                for (int dx = -2; dx <= 2; ++dx) {
                    const int xq = x + dx * s;
                    if (!m.col_in(xq)) continue;
                    const double eq[3] = {at(j + dy, xq, 0), at(j + dy, xq, 1), at(j + dy, xq, 2)};
                    double w = b[dy + 2] * b[dx + 2];
                    if (dx != 0 || dy != 0) {
                        double wn, dz;
                        if (!dn_pair(p, guide(j + dy, xq), dx * s, dy * s, za, zb, cfg.k, wn, dz)) continue;
                        const double dl = fabs(lp - dn_lum(eq[0], eq[1], eq[2])) / lden;
                        w = (w * wn) * dn_falloff(dz + dl);
                    }
                    sw = sw + w;
                    for (int k = 0; k < 3; ++k) se[k] = se[k] + w * eq[k];
                    sv = sv + (w * w) * at(j + dy, xq, 3);
                }
            }
            for (int k = 0; k < 3; ++k) P.e[from ^ 1][k][i] = se[k] / sw;
            P.var[from ^ 1][i] = sv / (sw * sw);
        }
        __syncthreads();  // the next row replaces row j - R
    }
}

// Step 5.  rgb_out: 3 doubles per pixel.
__global__ __launch_bounds__(256) void k_dn_finish(DnPlanes P, int set, double* rgb_out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int k = 0; k < 3; ++k) rgb_out[3 * i + k] = P.e[set][k][i] * P.div[k][i];
}

}  // namespace dev
}  // namespace lumo
