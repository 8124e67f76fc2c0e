// Device builder of the wide BVH (wbvh.h): an LBVH.  The kernels, in the order
// device/wbvh_dev.hip launches them:
//   k_wb_prims                  one thread per primitive: its segment (binary search), f64 box, ids
//   k_wb_cb_partial / _final    per-tree centroid bounds, a two-launch block reduction (min / max only)
//   k_wb_morton                 63-bit Morton key of the centroid within its tree's centroid bounds
//   k_rx_hist / k_rx_scatter    stable LSD radix sort, 8-bit digits: LDS histograms per block, global
//                               offsets through scan.h's exclusive scan, scatter ranks from wave64
//                               ballots and mbcnt.  The tree index is the most significant digit(s), so
//                               one sort of the whole array sorts every tree's segment on its own
//   k_wb_radix                  Karras's binary radix tree, one thread per internal node
//   k_wb_fit                    bottom-up boxes, counts and object flags behind one counter per node
//   k_wb_recflag / k_wb_records leaf triangle records in sorted order (positions from a scan)
//   k_wb_openflag               an upper bound of the wide nodes (binary nodes that are no leaves)
//   k_wb_roots_* / k_wb_open / k_wb_emit   collapse to 4 children and breadth-first layout, level by level
//   k_wb_need / k_wb_rootneed   walk-stack need, deepest level first, BLASes before the world trees
//   k_wb_rootarea / k_wb_stats_*  max |coordinate| and the SAH cost, fixed-order block reductions
// Indices: a primitive has an index (segment order) and, after the sort, a position.  Tree t owns
// indices and positions tree_base[t] .. tree_base[t + 1] - 1; its internal node i lives at global
// slot tree_base[t] + i (i < size - 1), its leaf j at position tree_base[t] + j.  A binary child is
// an int32: >= 0 an internal slot, < 0 the leaf at position ~c.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../../include/lumo_amd.h"
#include "../common/wbvh.h"
#include "../common/wbvh_dev_prep.h"
#include "scan.h"

namespace lumo {
namespace dev {

constexpr int WB_BLOCK = 256;
constexpr int WB_RED_GRID = 64;   // blocks per tree of the centroid-bound reduction
constexpr int WB_STAT_GRID = 256;  // blocks of the max_abs / SAH reduction
constexpr int RX_ITEMS = 8;       // keys per thread of a sort block
constexpr int RX_TILE = WB_BLOCK * RX_ITEMS;
constexpr int RX_BINS = 256;
constexpr int RX_WAVES = WB_BLOCK / 64;
constexpr int32_t WB_HASOBJ = 1 << 30;  // in icount: the subtree holds an object leaf

struct WbBox {
    double lo[3], hi[3];
};

struct WbScal {  // what the host reads back
    int32_t blas_need, max_stack;
    float max_abs;
    int32_t pad;
    double sah;
};

struct WbWork {
    int32_t n_prims, n_trees, n_segs, leaf_max;
    const wbvh::DevSeg* segs;
    const int32_t* tree_base;  // n_trees + 1
    const double* obj_box;
    const double* vertices;
    const lumo_triangle* tris;
    WbBox* pbox;     // per primitive index
    int32_t* ptri;   // global triangle, or -1: object leaf
    int32_t* pobj;
    WbBox* cbound;   // per tree: centroid bounds
    WbBox* cpart;    // n_trees x WB_RED_GRID partials
    uint64_t* key;   // per position, sorted
    uint32_t* idx;   // per position: primitive index
    int32_t* child;  // 2 per internal slot
    int32_t* iparent;
    int32_t* lparent;
    int32_t* ifirst;  // leftmost position of the slot's range
    WbBox* ibox;
    int32_t* icount;  // primitives of the subtree | WB_HASOBJ
    uint32_t* iflag;  // arrivals at the slot (k_wb_fit)
    uint32_t* rec_pos;  // per position: triangle records before it
    int32_t* root_ref;  // per tree
    int32_t* wtree;     // per wide node: its tree
    int32_t* need;      // per wide node: walk-stack need
    wbvh::Node* nodes;
    double* tv;
    WbScal* scal;
};

// last t with tree_base[t] <= i (empty trees share a base with their successor, which wins)
__device__ __forceinline__ int wb_tree_of(const int32_t* tree_base, int n_trees, int i) {
    int lo = 0, hi = n_trees - 1;
    while (lo < hi) {
        const int m = (lo + hi + 1) >> 1;
        if (tree_base[m] <= i) lo = m; else hi = m - 1;
    }
    return lo;
}

__device__ __forceinline__ double wb_half_area(const WbBox& b) {
    const double dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
    if (!(dx >= 0.0) || !(dy >= 0.0) || !(dz >= 0.0)) return 0.0;
    return dx * dy + dy * dz + dz * dx;
}

__global__ __launch_bounds__(WB_BLOCK) void k_wb_fill(uint32_t* p, uint32_t v, uint32_t n) {
    const uint32_t i = blockIdx.x * WB_BLOCK + threadIdx.x;
    if (i < n) p[i] = v;
}

// ---------------------------------------------------------------- 1. primitive boxes
__global__ __launch_bounds__(WB_BLOCK) void k_wb_prims(WbWork w) {
    const int i = blockIdx.x * WB_BLOCK + threadIdx.x;
    if (i >= w.n_prims) return;
    int lo = 0, hi = w.n_segs - 1;
    while (lo < hi) {  // the last segment that starts at or before i
        const int m = (lo + hi + 1) >> 1;
        if (w.segs[m].first <= i) lo = m; else hi = m - 1;
    }
    const wbvh::DevSeg s = w.segs[lo];
    WbBox b;
    int32_t tri = -1;
    if (s.tri_base >= 0) {
        tri = s.tri_base + (i - s.first);
        const lumo_triangle t = w.tris[tri];
        for (int a = 0; a < 3; ++a) {
            b.lo[a] = HUGE_VAL;
            b.hi[a] = -HUGE_VAL;
        }
        for (int k = 0; k < 3; ++k) {
            const double* v = w.vertices + 3 * (size_t)t.v[k];
            for (int a = 0; a < 3; ++a) {
                b.lo[a] = v[a] < b.lo[a] ? v[a] : b.lo[a];
                b.hi[a] = b.hi[a] < v[a] ? v[a] : b.hi[a];
            }
        }
    } else {
        const double* q = w.obj_box + 6 * (size_t)(~s.tri_base);
        for (int a = 0; a < 3; ++a) {
            b.lo[a] = q[a];
            b.hi[a] = q[3 + a];
        }
    }
    w.pbox[i] = b;
    w.ptri[i] = tri;
    w.pobj[i] = s.obj;
}

// Block reduction of a box (min of lo, max of hi) over WB_BLOCK or fewer threads; thread 0 has it.
template <int N>
__device__ __forceinline__ void wb_block_minmax(WbBox& b, double (*lds)[N]) {
    const int t = threadIdx.x;
    for (int a = 0; a < 3; ++a) {
        lds[a][t] = b.lo[a];
        lds[3 + a][t] = b.hi[a];
    }
    __syncthreads();
    for (int d = N / 2; d > 0; d >>= 1) {
        if (t < d)
            for (int a = 0; a < 3; ++a) {
                const double x = lds[a][t + d], y = lds[3 + a][t + d];
                if (x < lds[a][t]) lds[a][t] = x;
                if (y > lds[3 + a][t]) lds[3 + a][t] = y;
            }
        __syncthreads();
    }
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = lds[a][0];
        b.hi[a] = lds[3 + a][0];
    }
}

// grid (WB_RED_GRID, trees): block x of tree y strides over the tree's primitives
__global__ __launch_bounds__(WB_BLOCK) void k_wb_cb_partial(WbWork w) {
    __shared__ double lds[6][WB_BLOCK];
    const int t = blockIdx.y;
    const int b0 = w.tree_base[t], b1 = w.tree_base[t + 1];
    WbBox c;
    for (int a = 0; a < 3; ++a) {
        c.lo[a] = HUGE_VAL;
        c.hi[a] = -HUGE_VAL;
    }
    for (int64_t i = (int64_t)b0 + blockIdx.x * WB_BLOCK + threadIdx.x; i < b1; i += WB_RED_GRID * WB_BLOCK) {
        const WbBox& p = w.pbox[i];
        for (int a = 0; a < 3; ++a) {
            const double x = 0.5 * p.lo[a] + 0.5 * p.hi[a];
            if (x < c.lo[a]) c.lo[a] = x;
            if (x > c.hi[a]) c.hi[a] = x;
        }
    }
    wb_block_minmax<WB_BLOCK>(c, lds);
    if (threadIdx.x == 0) w.cpart[(size_t)t * WB_RED_GRID + blockIdx.x] = c;
}

__global__ __launch_bounds__(WB_RED_GRID) void k_wb_cb_final(WbWork w) {
    __shared__ double lds[6][WB_RED_GRID];
    WbBox c = w.cpart[(size_t)blockIdx.x * WB_RED_GRID + threadIdx.x];
    wb_block_minmax<WB_RED_GRID>(c, lds);
    if (threadIdx.x == 0) w.cbound[blockIdx.x] = c;
}

// ---------------------------------------------------------------- 2. Morton keys
__device__ __forceinline__ uint64_t wb_spread21(uint64_t x) {  // 21 bits -> every third bit
    x &= 0x1fffffull;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}
// cell of c in [lo, hi] cut into 2^21: a zero (or NaN) extent and a NaN give cell 0
__device__ __forceinline__ uint64_t wb_cell(double c, double lo, double hi) {
    const double ext = hi - lo;
    if (!(ext > 0.0)) return 0;
    const double x = (c - lo) / ext * 2097152.0;
    if (!(x >= 0.0)) return 0;
    return x >= 2097151.0 ? 2097151ull : (uint64_t)x;
}

__global__ __launch_bounds__(WB_BLOCK) void k_wb_morton(WbWork w) {
    const int i = blockIdx.x * WB_BLOCK + threadIdx.x;
    if (i >= w.n_prims) return;
    const WbBox cb = w.cbound[wb_tree_of(w.tree_base, w.n_trees, i)];
    const WbBox p = w.pbox[i];
    uint64_t k = 0;
    for (int a = 0; a < 3; ++a)
        k |= wb_spread21(wb_cell(0.5 * p.lo[a] + 0.5 * p.hi[a], cb.lo[a], cb.hi[a])) << (2 - a);
    w.key[i] = k;
    w.idx[i] = (uint32_t)i;
}

// ---------------------------------------------------------------- 3. stable radix sort
// digit of pass p: bits 8p .. 8p + 7 of the key for p < 8, then of the primitive's tree
__device__ __forceinline__ uint32_t rx_digit(uint64_t key, uint32_t id, int pass, const int32_t* tree_base, int n_trees) {
    if (pass < 8) return (uint32_t)(key >> (8 * pass)) & 255u;
    return ((uint32_t)wb_tree_of(tree_base, n_trees, (int)id) >> (8 * (pass - 8))) & 255u;
}

// hist[digit * gridDim.x + block]: digit-major, so one exclusive scan of the whole table gives
// every (digit, block) its first output position
__global__ __launch_bounds__(WB_BLOCK) void k_rx_hist(const uint64_t* key, const uint32_t* idx, uint32_t n, int pass,
                                                      const int32_t* tree_base, int n_trees, uint32_t* hist) {
    __shared__ uint32_t h[RX_BINS];
    h[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * RX_TILE;
    for (int k = 0; k < RX_ITEMS; ++k) {
        const size_t i = base + (size_t)k * WB_BLOCK + threadIdx.x;
        if (i < n) atomicAdd(&h[rx_digit(key[i], idx[i], pass, tree_base, n_trees)], 1u);  // integer counts
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = h[threadIdx.x];
}

// Stable scatter.  The block walks its tile in rows of WB_BLOCK elements (element order = row, wave,
// lane).  Within a wave, the lanes with the same digit are found by 8 ballots; a lane's rank among
// them is mbcnt of that mask, the first of them posts the wave's count.  A position is the digit's
// running offset + the counts of the earlier waves of the row + the rank: no atomic, so equal
// digits keep their order.
__global__ __launch_bounds__(WB_BLOCK) void k_rx_scatter(const uint64_t* key, const uint32_t* idx, uint32_t n, int pass,
                                                         const int32_t* tree_base, int n_trees, const uint32_t* offs,
                                                         uint64_t* key_out, uint32_t* idx_out) {
    __shared__ uint32_t run[RX_BINS];
    __shared__ uint32_t wcnt[RX_WAVES][RX_BINS];
    const int t = threadIdx.x, wave = t >> 6;
    run[t] = offs[(size_t)t * gridDim.x + blockIdx.x];
    for (int v = 0; v < RX_WAVES; ++v) wcnt[v][t] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * RX_TILE;
    for (int k = 0; k < RX_ITEMS; ++k) {
        if (base + (size_t)k * WB_BLOCK >= n) break;  // uniform over the block
        const size_t i = base + (size_t)k * WB_BLOCK + t;
        const bool valid = i < n;
        const uint64_t ky = valid ? key[i] : 0;
        const uint32_t id = valid ? idx[i] : 0;
        const uint32_t d = valid ? rx_digit(ky, id, pass, tree_base, n_trees) : 0;
        unsigned long long same = __ballot(valid);
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bb = __ballot(valid && bit);
            same &= bit ? bb : ~bb;
        }
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(same >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)same, 0u));
        if (valid && rank == 0) wcnt[wave][d] = (uint32_t)__popcll(same);
        __syncthreads();
        if (valid) {
            uint32_t pos = run[d] + rank;
            for (int v = 0; v < wave; ++v) pos += wcnt[v][d];
            if (pos < n) {  // always, when the histogram was of these digits
                key_out[pos] = ky;
                idx_out[pos] = id;
            }
        }
        __syncthreads();
        uint32_t s = 0;
        for (int v = 0; v < RX_WAVES; ++v) {
            s += wcnt[v][t];
            wcnt[v][t] = 0;
        }
        run[t] += s;
        __syncthreads();
    }
}

// ---------------------------------------------------------------- 4. binary radix tree (Karras 2012)
__device__ __forceinline__ int wb_delta(const uint64_t* key, int64_t i, int64_t j, int n) {
    if (j < 0 || j >= n) return -1;
    const uint64_t x = key[i] ^ key[j];
    return x ? __clzll((long long)x) : 64 + __clz((int)((uint32_t)i ^ (uint32_t)j));
}

__global__ __launch_bounds__(WB_BLOCK) void k_wb_radix(WbWork w) {
    const int g = blockIdx.x * WB_BLOCK + threadIdx.x;
    if (g >= w.n_prims) return;
    const int t = wb_tree_of(w.tree_base, w.n_trees, g);
    const int b0 = w.tree_base[t], n = w.tree_base[t + 1] - b0;
    const int64_t i = g - b0;
    if (i >= n - 1) return;
    const uint64_t* key = w.key + b0;
    const int d = wb_delta(key, i, i + 1, n) - wb_delta(key, i, i - 1, n) > 0 ? 1 : -1;
    const int dmin = wb_delta(key, i, i - d, n);
    int64_t lmax = 2;
    while (wb_delta(key, i, i + lmax * d, n) > dmin) lmax *= 2;
    int64_t l = 0;
    for (int64_t s = lmax / 2; s >= 1; s /= 2)
        if (wb_delta(key, i, i + (l + s) * d, n) > dmin) l += s;
    const int64_t j = i + l * d;
    const int dnode = wb_delta(key, i, j, n);
    int64_t s = 0, step = l;
    do {
        step = (step + 1) >> 1;
        if (wb_delta(key, i, i + (s + step) * d, n) > dnode) s += step;
    } while (step > 1);
    int64_t gamma = i + s * d + (d < 0 ? -1 : 0);
    gamma = gamma < 0 ? 0 : (gamma > n - 2 ? n - 2 : gamma);  // in range already when the keys are sorted
    const int64_t first = i < j ? i : j, last = i < j ? j : i;
    const int32_t left = (int32_t)(b0 + gamma), right = left + 1;
    if (first == gamma) {
        w.child[2 * (size_t)g] = ~left;
        w.lparent[left] = g;
    } else {
        w.child[2 * (size_t)g] = left;
        w.iparent[left] = g;
    }
    if (last == gamma + 1) {
        w.child[2 * (size_t)g + 1] = ~right;
        w.lparent[right] = g;
    } else {
        w.child[2 * (size_t)g + 1] = right;
        w.iparent[right] = g;
    }
    w.ifirst[g] = (int32_t)(b0 + first);
    if (i == 0) w.iparent[g] = -1;
}

// ---------------------------------------------------------------- 5. bottom-up boxes
// box, primitive count and object flag of a binary child
__device__ __forceinline__ void wb_child_data(const WbWork& w, int32_t c, WbBox& b, int32_t& cnt) {
    if (c < 0) {
        const uint32_t p = w.idx[~c];
        b = w.pbox[p];
        cnt = 1 | (w.ptri[p] < 0 ? WB_HASOBJ : 0);
    } else {
        b = w.ibox[c];
        cnt = w.icount[c];
    }
}

// One thread per leaf climbs.  At a slot the first arrival leaves; the second, after the fence,
// reads both children (the other's were written before its own fence and arrival) and goes on.
// Nobody waits.
__global__ __launch_bounds__(WB_BLOCK) void k_wb_fit(WbWork w) {
    const int g = blockIdx.x * WB_BLOCK + threadIdx.x;
    if (g >= w.n_prims) return;
    const int t = wb_tree_of(w.tree_base, w.n_trees, g);
    if (w.tree_base[t + 1] - w.tree_base[t] < 2) return;  // a tree of one leaf has no slot
    int32_t cur = w.lparent[g];
    while (cur >= 0) {
        if (atomicAdd(&w.iflag[cur], 1u) == 0u) return;
        __threadfence();
        WbBox a, b;
        int32_t ca, cb;
        wb_child_data(w, w.child[2 * (size_t)cur], a, ca);
        wb_child_data(w, w.child[2 * (size_t)cur + 1], b, cb);
        for (int x = 0; x < 3; ++x) {
            a.lo[x] = b.lo[x] < a.lo[x] ? b.lo[x] : a.lo[x];
            a.hi[x] = a.hi[x] < b.hi[x] ? b.hi[x] : a.hi[x];
        }
        w.ibox[cur] = a;
        w.icount[cur] = ((ca & ~WB_HASOBJ) + (cb & ~WB_HASOBJ)) | ((ca | cb) & WB_HASOBJ);
        __threadfence();
        cur = w.iparent[cur];
    }
}

// ---------------------------------------------------------------- leaves and their records
__device__ __forceinline__ bool wb_is_leaf(const WbWork& w, int32_t c) {
    if (c < 0) return true;
    const int32_t k = w.icount[c];
    return !(k & WB_HASOBJ) && k <= w.leaf_max;
}
__device__ __forceinline__ int32_t wb_leaf_ref(const WbWork& w, int32_t c) {
    if (c < 0) {
        const uint32_t p = w.idx[~c];
        return w.ptri[p] < 0 ? wbvh::make_leaf(w.pobj[p], 0) : wbvh::make_leaf((int32_t)w.rec_pos[~c], 1);
    }
    return wbvh::make_leaf((int32_t)w.rec_pos[w.ifirst[c]], w.icount[c]);
}
__device__ __forceinline__ WbBox wb_box_of(const WbWork& w, int32_t c) { return c < 0 ? w.pbox[w.idx[~c]] : w.ibox[c]; }

__global__ __launch_bounds__(WB_BLOCK) void k_wb_recflag(WbWork w, uint32_t* flag) {
    const int g = blockIdx.x * WB_BLOCK + threadIdx.x;
    if (g < w.n_prims) flag[g] = w.ptri[w.idx[g]] >= 0 ? 1u : 0u;
}

// the 80-byte record of the triangle at position g (wbvh.h TV): A, B, C, then (tri, obj)
__global__ __launch_bounds__(WB_BLOCK) void k_wb_records(WbWork w) {
    const int g = blockIdx.x * WB_BLOCK + threadIdx.x;
    if (g >= w.n_prims) return;
    const uint32_t p = w.idx[g];
    const int32_t tri = w.ptri[p];
    if (tri < 0) return;
    double* rec = w.tv + wbvh::TV * (size_t)w.rec_pos[g];
    const lumo_triangle t = w.tris[tri];
    for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a) rec[3 * k + a] = w.vertices[3 * (size_t)t.v[k] + a];
    int32_t* ids = reinterpret_cast<int32_t*>(rec + 9);
    ids[0] = tri;
    ids[1] = w.pobj[p];
}

// flag[g] = 1 when slot g exists and is no leaf: their number bounds the wide nodes
__global__ __launch_bounds__(WB_BLOCK) void k_wb_openflag(WbWork w, uint32_t* flag) {
    const int g = blockIdx.x * WB_BLOCK + threadIdx.x;
    if (g >= w.n_prims) return;
    const int t = wb_tree_of(w.tree_base, w.n_trees, g);
    const bool slot = g - w.tree_base[t] < w.tree_base[t + 1] - w.tree_base[t] - 1;
    flag[g] = slot && !wb_is_leaf(w, g) ? 1u : 0u;
}

// ---------------------------------------------------------------- 6. collapse, breadth-first layout
// the root slot of tree t when the tree's root is a wide node, else -1
__device__ __forceinline__ int32_t wb_root_slot(const WbWork& w, int t) {
    const int b0 = w.tree_base[t], n = w.tree_base[t + 1] - b0;
    return n >= 2 && !wb_is_leaf(w, b0) ? b0 : -1;
}
__global__ __launch_bounds__(WB_BLOCK) void k_wb_roots_count(WbWork w, uint32_t* cnt) {
    const int t = blockIdx.x * WB_BLOCK + threadIdx.x;
    if (t < w.n_trees) cnt[t] = wb_root_slot(w, t) >= 0 ? 1u : 0u;
}
__global__ __launch_bounds__(WB_BLOCK) void k_wb_roots_emit(WbWork w, const uint32_t* pos, int32_t* items) {
    const int t = blockIdx.x * WB_BLOCK + threadIdx.x;
    if (t >= w.n_trees) return;
    const int b0 = w.tree_base[t], n = w.tree_base[t + 1] - b0;
    const int32_t slot = wb_root_slot(w, t);
    if (slot >= 0) {
        w.root_ref[t] = (int32_t)pos[t];
        items[pos[t]] = slot;
        w.wtree[pos[t]] = t;
    } else {
        w.root_ref[t] = n == 0 ? wbvh::NONE : wb_leaf_ref(w, n == 1 ? ~b0 : b0);
    }
}

// the host's rule (wbvh_build.h collapse): open the largest-area child that is no leaf, in place
__device__ __forceinline__ int wb_collapse(const WbWork& w, int32_t b, int32_t* out) {
    int n = 2;
    out[0] = w.child[2 * (size_t)b];
    out[1] = w.child[2 * (size_t)b + 1];
    while (n < wbvh::WIDTH) {
        int best = -1;
        double ba = -1.0;
        for (int k = 0; k < n; ++k) {
            if (wb_is_leaf(w, out[k])) continue;
            const double a = wb_half_area(w.ibox[out[k]]);
            if (a > ba) {
                ba = a;
                best = k;
            }
        }
        if (best < 0) break;
        const int32_t x = out[best];
        for (int k = n; k > best + 1; --k) out[k] = out[k - 1];
        out[best] = w.child[2 * (size_t)x];
        out[best + 1] = w.child[2 * (size_t)x + 1];
        n++;
    }
    return n;
}

// Kernel A: the children of every item of the level (kept for kernel B) and how many are nodes
__global__ __launch_bounds__(WB_BLOCK) void k_wb_open(WbWork w, const int32_t* items, uint32_t n_items, int32_t* kids,
                                                      uint32_t* n_kids, uint32_t* cnt) {
    const uint32_t k = blockIdx.x * WB_BLOCK + threadIdx.x;
    if (k >= n_items) return;
    int32_t out[wbvh::WIDTH] = {wbvh::NONE, wbvh::NONE, wbvh::NONE, wbvh::NONE};
    const int n = wb_collapse(w, items[k], out);
    uint32_t inner = 0;
    for (int j = 0; j < wbvh::WIDTH; ++j) {
        kids[4 * (size_t)k + j] = out[j];
        if (j < n && !wb_is_leaf(w, out[j])) inner++;
    }
    n_kids[k] = (uint32_t)n;
    cnt[k] = inner;
}

__device__ __forceinline__ float wb_f_down(double x) {
    float f = (float)x;
    if ((double)f > x) f = nextafterf(f, -HUGE_VALF);
    return f;
}
__device__ __forceinline__ float wb_f_up(double x) {
    float f = (float)x;
    if ((double)f < x) f = nextafterf(f, HUGE_VALF);
    return f;
}

// Kernel B: item k is node level_base + k; its node children take next_base + pos[k] + their rank
__global__ __launch_bounds__(WB_BLOCK) void k_wb_emit(WbWork w, uint32_t n_items, const int32_t* kids,
                                                      const uint32_t* n_kids, const uint32_t* pos, int32_t level_base,
                                                      int32_t next_base, int32_t* next_items) {
    const uint32_t k = blockIdx.x * WB_BLOCK + threadIdx.x;
    if (k >= n_items) return;
    const int n = (int)n_kids[k];
    const int32_t tree = w.wtree[level_base + k];
    wbvh::Node nd;
    nd.n = n;
    nd.pad0 = nd.pad1 = nd.pad2 = 0;
    uint32_t at = pos[k];
    for (int j = 0; j < wbvh::WIDTH; ++j) {
        nd.ref[j] = wbvh::NONE;
        for (int a = 0; a < 3; ++a) {
            nd.lo[a][j] = 1.0f;
            nd.hi[a][j] = -1.0f;
        }
        if (j >= n) continue;
        const int32_t c = kids[4 * (size_t)k + j];
        const WbBox b = wb_box_of(w, c);
        for (int a = 0; a < 3; ++a) {
            nd.lo[a][j] = wb_f_down(b.lo[a]);
            nd.hi[a][j] = wb_f_up(b.hi[a]);
        }
        if (wb_is_leaf(w, c)) {
            nd.ref[j] = wb_leaf_ref(w, c);
        } else {
            nd.ref[j] = next_base + (int32_t)at;
            next_items[at] = c;
            w.wtree[next_base + at] = tree;
            at++;
        }
    }
    w.nodes[level_base + k] = nd;
}

// ---------------------------------------------------------------- 7. derived values
__device__ __forceinline__ int wb_ref_need(const WbWork& w, int32_t r, bool world, int blas_need) {
    if (r == wbvh::NONE) return 0;
    if (!wbvh::is_leaf(r)) return w.need[r];
    return world && wbvh::leaf_count(r) == 0 ? 1 + blas_need : 0;
}
// nodes [lo, hi) of one level; pass 0 the BLAS nodes, pass 1 the world trees' (blas_need known)
__global__ __launch_bounds__(WB_BLOCK) void k_wb_need(WbWork w, int32_t lo, int32_t hi, int pass) {
    const int32_t i = lo + (int32_t)(blockIdx.x * WB_BLOCK + threadIdx.x);
    if (i >= hi) return;
    const bool world = w.wtree[i] < 2;
    if ((pass == 0) == world) return;
    const int blas_need = pass ? w.scal->blas_need : 0;
    const wbvh::Node& nd = w.nodes[i];
    int m = 0;
    for (int k = 0; k < nd.n; ++k) {
        const int x = wb_ref_need(w, nd.ref[k], world, blas_need);
        m = x > m ? x : m;
    }
    w.need[i] = nd.n - 1 + m;
}
// one block.  pass 0: blas_need = the largest need of a BLAS root; pass 1: max_stack of the world roots
__global__ __launch_bounds__(WB_BLOCK) void k_wb_rootneed(WbWork w, int pass) {
    __shared__ int lds[WB_BLOCK];
    int m = 0;
    if (pass == 0) {
        for (int t = 2 + threadIdx.x; t < w.n_trees; t += WB_BLOCK) {
            const int x = wb_ref_need(w, w.root_ref[t], false, 0);
            m = x > m ? x : m;
        }
    } else if (threadIdx.x < 2) {
        m = wb_ref_need(w, w.root_ref[threadIdx.x], true, w.scal->blas_need);
    }
    lds[threadIdx.x] = m;
    __syncthreads();
    for (int d = WB_BLOCK / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d && lds[threadIdx.x + d] > lds[threadIdx.x]) lds[threadIdx.x] = lds[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (pass == 0) w.scal->blas_need = lds[0]; else w.scal->max_stack = lds[0];
    }
}

__device__ __forceinline__ double wb_child_area(const wbvh::Node& nd, int k) {
    WbBox b;
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = nd.lo[a][k];
        b.hi[a] = nd.hi[a][k];
    }
    return wb_half_area(b);
}
// per tree: the half-area of the union of the root node's child boxes (0: the root is no node)
__global__ __launch_bounds__(WB_BLOCK) void k_wb_rootarea(WbWork w, double* rarea) {
    const int t = blockIdx.x * WB_BLOCK + threadIdx.x;
    if (t >= w.n_trees) return;
    const int32_t r = w.root_ref[t];
    double area = 0.0;
    if (r >= 0) {
        const wbvh::Node& nd = w.nodes[r];
        WbBox b;
        for (int a = 0; a < 3; ++a) {
            b.lo[a] = HUGE_VAL;
            b.hi[a] = -HUGE_VAL;
        }
        for (int k = 0; k < nd.n; ++k)
            for (int a = 0; a < 3; ++a) {
                if ((double)nd.lo[a][k] < b.lo[a]) b.lo[a] = nd.lo[a][k];
                if ((double)nd.hi[a][k] > b.hi[a]) b.hi[a] = nd.hi[a][k];
            }
        area = wb_half_area(b);
    }
    rarea[t] = area;
}
// max |coordinate| and the SAH terms of the nodes: block b strides from b, fixed grid, so the
// order of the sum does not depend on the run.  part: gridDim.x (max, sum) pairs.
__device__ __forceinline__ void wb_block_stat(float& mx, double& sum, float* lm, double* ls) {
    const int t = threadIdx.x;
    lm[t] = mx;
    ls[t] = sum;
    __syncthreads();
    for (int d = WB_BLOCK / 2; d > 0; d >>= 1) {
        if (t < d) {
            if (lm[t + d] > lm[t]) lm[t] = lm[t + d];
            ls[t] += ls[t + d];
        }
        __syncthreads();
    }
    mx = lm[0];
    sum = ls[0];
}
__global__ __launch_bounds__(WB_BLOCK) void k_wb_stats_partial(WbWork w, int32_t n_nodes, const double* rarea, float* pmax,
                                                               double* psum) {
    __shared__ float lm[WB_BLOCK];
    __shared__ double ls[WB_BLOCK];
    float mx = 0.0f;
    double sum = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * WB_BLOCK + threadIdx.x; i < n_nodes; i += (int64_t)gridDim.x * WB_BLOCK) {
        const wbvh::Node& nd = w.nodes[i];
        const double ra = rarea[w.wtree[i]];
        for (int k = 0; k < nd.n; ++k) {
            for (int a = 0; a < 3; ++a) {
                const float x = fabsf(nd.lo[a][k]), y = fabsf(nd.hi[a][k]);
                mx = x > mx ? x : mx;
                mx = y > mx ? y : mx;
            }
            if (ra > 0.0) {
                const int32_t c = nd.ref[k];
                const int wt = wbvh::is_leaf(c) && wbvh::leaf_count(c) > 1 ? wbvh::leaf_count(c) : 1;
                sum += wb_child_area(nd, k) / ra * wt;
            }
        }
    }
    wb_block_stat(mx, sum, lm, ls);
    if (threadIdx.x == 0) {
        pmax[blockIdx.x] = mx;
        psum[blockIdx.x] = sum;
    }
}
__global__ __launch_bounds__(WB_BLOCK) void k_wb_stats_final(WbWork w, int n_part, const float* pmax, const double* psum) {
    __shared__ float lm[WB_BLOCK];
    __shared__ double ls[WB_BLOCK];
    float mx = (int)threadIdx.x < n_part ? pmax[threadIdx.x] : 0.0f;
    double sum = (int)threadIdx.x < n_part ? psum[threadIdx.x] : 0.0;
    wb_block_stat(mx, sum, lm, ls);
    if (threadIdx.x == 0) {
        w.scal->max_abs = mx;
        w.scal->sah = sum;
    }
}

}  // namespace dev
}  // namespace lumo
