// Refit of the wide BVH after its vertices moved (wbvh.h; DESIGN.md §4g "Refit"): the topology of
// every tree stays (ref, n, record order, roots), every box and every copy of a vertex is brought up
// to date.  The kernels, in the order device/wbvh_dev.hip launches them:
//   k_rf_protect         once per upload: the vertices of lights and of objects that are no kd mesh
//   k_rf_parents         once per upload: (parent, slot) and the interior-child count of every node
//   k_rf_trees           once per upload: the root of every node's tree (k_wb_stats_partial's wtree)
//   k_rf_stage_vertices  new values against the present ones: non-finite, protected and changed, changed
//   k_rf_records         leaf records and soup rows from the new vertices, one LDS tile per block
//   k_rf_fit             the boxes bottom-up, a quad of lanes per node; BLASes, then the world trees
//   k_rf_rootarea        per root node the area k_wb_rootarea gives its tree
//   k_rf_copy            the refreshed arrays into the staged sets (hot / TOP), 16 B per lane
//   k_rf_mark            lumo_scene_motion_mark: the vertices into the previous vertices, 16 B per lane
// The roundings (wb_f_down / wb_f_up) and the reductions (k_wb_stats_*) are the builder's own.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "state.h"
#include "wbvh_dev.h"

namespace lumo {
namespace dev {

constexpr int RF_QUADS = WB_BLOCK / 4;  // nodes per block of k_rf_fit
enum { RF_NONFINITE = 0, RF_PROTECTED, RF_CHANGED, RF_FLAGS };

struct RfWork {
    int32_t n_nodes, n_recs, n_lights, n_objs;
    int32_t oroot, lroot;  // the world trees' roots: every other tree is a BLAS
    const double* vertices;
    const lumo_triangle* tris;
    const lumo_object* objs;
    const lumo_object* lights;
    const lumo_transform* xforms;
    const int32_t* oblas;
    const int32_t* lblas;
    wbvh::Node* nodes;
    double* wtv;   // leaf records
    double* soup;  // DScene::tv
    int32_t* parent;   // per node: parent << 2 | slot; -1: a root
    uint32_t* kids;    // per node: interior children
    uint32_t* arrive;  // per node: interior children that are done
    int32_t* wtree;    // per node: its tree's root node
    WbBox* box;        // per node: the f64 union of its child boxes
    double* rarea;     // per root node
};

__device__ __forceinline__ void rf_empty(WbBox& b) {
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = HUGE_VAL;
        b.hi[a] = -HUGE_VAL;
    }
}
__device__ __forceinline__ int rf_mesh_tris(const lumo_object& o) {
    return o.type == LUMO_OBJ_SPHERE ? 0 : (o.type == LUMO_OBJ_TRIANGLE ? 1 : o.num_tris);
}

// ---------------------------------------------------------------- once per upload
// Block b: light b, then object b - n_lights.  A light's kd tree, a Rectangle's parameters and the
// area of either are host-made from these vertices, so they must stay where they are.
__global__ __launch_bounds__(WB_BLOCK) void k_rf_protect(RfWork w, int32_t n_vertices, int32_t n_triangles, uint8_t* prot) {
    const int b = blockIdx.x;
    const lumo_object& o = b < w.n_lights ? w.lights[b] : w.objs[b - w.n_lights];
    if (b >= w.n_lights && o.type == LUMO_OBJ_KDMESH) return;
    const int nt = rf_mesh_tris(o);
    for (int k = threadIdx.x; k < nt; k += WB_BLOCK) {
        const int64_t ti = (int64_t)o.tri_base + k;
        if (ti < 0 || ti >= n_triangles) continue;
        for (int j = 0; j < 3; ++j) {
            const int32_t v = w.tris[ti].v[j];
            if (v >= 0 && v < n_vertices) prot[v] = 1;
        }
    }
}

// parent must be all -1 before: a node nobody names is a root
__global__ __launch_bounds__(WB_BLOCK) void k_rf_parents(RfWork w) {
    const int i = blockIdx.x * WB_BLOCK + threadIdx.x;
    if (i >= w.n_nodes) return;
    const wbvh::Node& nd = w.nodes[i];
    uint32_t inner = 0;
    for (int k = 0; k < nd.n && k < wbvh::WIDTH; ++k) {
        const int32_t r = nd.ref[k];
        if (r > i && r < w.n_nodes) {  // level-major: a child lies behind its parent
            w.parent[r] = (i << 2) | k;
            inner++;
        }
    }
    w.kids[i] = inner;
}

__global__ __launch_bounds__(WB_BLOCK) void k_rf_trees(RfWork w) {
    const int i = blockIdx.x * WB_BLOCK + threadIdx.x;
    if (i >= w.n_nodes) return;
    int32_t r = i;
    for (int32_t p = w.parent[r]; p >= 0; p = w.parent[r]) r = p >> 2;  // strictly decreasing
    w.wtree[i] = r;
}

// ---------------------------------------------------------------- 1. the new values
// One thread per vertex of the range.  Nothing is written but the flags: the caller copies the range
// over DScene::vertices only when the first two are clear, so a refusal leaves the scene as it was.
__global__ __launch_bounds__(WB_BLOCK) void k_rf_stage_vertices(const double* vnew, const double* vertices,
                                                               const uint8_t* prot, int32_t first, int32_t count,
                                                               uint32_t* flags) {
    const int j = blockIdx.x * WB_BLOCK + threadIdx.x;
    bool changed = false, bad = false;
    if (j < count) {
        for (int a = 0; a < 3; ++a) {
            const double x = vnew[3 * (size_t)j + a];
            bad = bad || !isfinite(x);
            changed = changed || __double_as_longlong(x) != __double_as_longlong(vertices[3 * ((size_t)first + j) + a]);
        }
        if (bad) atomicOr(&flags[RF_NONFINITE], 1u);
        if (changed && prot[first + j]) atomicOr(&flags[RF_PROTECTED], 1u);
    }
    const unsigned long long m = __ballot(changed);  // one integer atomic per wave
    if (m && mbcnt64(m) == 0 && changed) atomicAdd(&flags[RF_CHANGED], (uint32_t)__popcll(m));
}

// ---------------------------------------------------------------- 2. records and soup
// One thread per leaf record.  The record names its triangle; the three vertices are gathered into
// the block's LDS tile (WB_BLOCK x 80 B, contiguous in wtv), which then goes out 16 B per lane:
// written per thread, the 80-B stride would touch every 128-B line ten times.  The soup row of the
// triangle is scattered anyway and is written in place.
__global__ __launch_bounds__(WB_BLOCK) void k_rf_records(RfWork w) {
    __shared__ __attribute__((aligned(16))) unsigned long long tile[WB_BLOCK * wbvh::TV];
    const int base = blockIdx.x * WB_BLOCK;
    const int n = w.n_recs - base < WB_BLOCK ? w.n_recs - base : WB_BLOCK;
    const int t = threadIdx.x;
    if (t < n) {
        const unsigned long long* rec = reinterpret_cast<const unsigned long long*>(w.wtv) + wbvh::TV * ((size_t)base + t);
        const unsigned long long ids = rec[9];  // (tri, obj): kept
        const int32_t tri = (int32_t)(uint32_t)ids;
        const lumo_triangle tr = w.tris[tri];
        double* row = w.soup + TV_STRIDE * (size_t)tri;
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) {
                const double x = w.vertices[3 * (size_t)tr.v[k] + a];
                tile[wbvh::TV * t + 3 * k + a] = (unsigned long long)__double_as_longlong(x);
                row[3 * k + a] = x;
            }
        tile[wbvh::TV * t + 9] = ids;
    }
    __syncthreads();
    const uint4* src = reinterpret_cast<const uint4*>(tile);
    uint4* dst = reinterpret_cast<uint4*>(w.wtv + wbvh::TV * (size_t)base);  // 80 * base: 16-B aligned
    for (int i = t; i < n * (wbvh::TV / 2); i += WB_BLOCK) dst[i] = src[i];
}

// ---------------------------------------------------------------- 3. boxes, bottom-up
// wbvh_build.h's xf_point / xf_box, operation for operation (f64, no contraction): the instance and
// sphere boxes then equal the builders' bit for bit.
__device__ __forceinline__ void rf_xf_box(const lumo_transform& T, const WbBox& in, WbBox& out) {
    rf_empty(out);
    for (int c = 0; c < 8; ++c) {
        const double p[3] = {(c & 1) ? in.hi[0] : in.lo[0], (c & 2) ? in.hi[1] : in.lo[1], (c & 4) ? in.hi[2] : in.lo[2]};
        double o[4];
        for (int r = 0; r < 4; ++r) o[r] = T.m[4 * r] * p[0] + T.m[4 * r + 1] * p[1] + T.m[4 * r + 2] * p[2] + T.m[4 * r + 3];
        for (int a = 0; a < 3; ++a) {
            const double q = o[a] / o[3];
            out.lo[a] = q < out.lo[a] ? q : out.lo[a];
            out.hi[a] = out.hi[a] < q ? q : out.hi[a];
        }
    }
    double mag = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double x = fabs(out.lo[a]), y = fabs(out.hi[a]);
        const double m = x < y ? y : x;
        mag = mag < m ? m : mag;
    }
    const double pad = mag * 1e-9;
    for (int a = 0; a < 3; ++a) {
        out.lo[a] -= pad;
        out.hi[a] += pad;
    }
}

// exact f64 bounds of the records of a triangle leaf
__device__ __forceinline__ void rf_leaf_box(const RfWork& w, int32_t ref, WbBox& b) {
    rf_empty(b);
    const int first = wbvh::leaf_first(ref), cnt = wbvh::leaf_count(ref);
    if (first < 0 || first + cnt > w.n_recs) return;
    for (int j = 0; j < cnt; ++j) {
        const double* rec = w.wtv + wbvh::TV * ((size_t)first + j);
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) {
                const double x = rec[3 * k + a];
                b.lo[a] = x < b.lo[a] ? x : b.lo[a];
                b.hi[a] = b.hi[a] < x ? x : b.hi[a];
            }
    }
}

// the world box of an object leaf: a sphere, or an instance of the BLAS whose root is blas
__device__ __forceinline__ void rf_object_box(const RfWork& w, const lumo_object& o, int32_t blas, WbBox& b) {
    WbBox local;
    if (o.type == LUMO_OBJ_SPHERE) {
        const double r = fabs(o.radius);
        for (int a = 0; a < 3; ++a) {
            local.lo[a] = -r;
            local.hi[a] = r;
        }
    } else if (blas >= 0 && blas < w.n_nodes) {
        local = w.box[blas];  // of the first sweep
    } else if (blas != wbvh::NONE && wbvh::leaf_count(blas) > 0) {
        rf_leaf_box(w, blas, local);
    } else {
        rf_empty(local);
    }
    if (o.xform >= 0) rf_xf_box(w.xforms[o.xform], local, b); else b = local;
}

__device__ __forceinline__ double rf_quad_min(double x) {
    double y = __shfl_xor(x, 1);
    x = y < x ? y : x;
    y = __shfl_xor(x, 2);
    return y < x ? y : x;
}
__device__ __forceinline__ double rf_quad_max(double x) {
    double y = __shfl_xor(x, 1);
    x = x < y ? y : x;
    y = __shfl_xor(x, 2);
    return x < y ? y : x;
}

// Four adjacent lanes own one node, one lane per child slot; a quad starts at a node without an
// interior child and climbs.  At a node: every lane finds the f64 box of its child (a leaf's from
// the records, an object leaf's from its shape, an interior child's from `box`, which that child's
// quad wrote before its fence and arrival), rounds it outward into its slot, the quad unites the
// four and lane 0 stores the union, fences and counts itself in at the parent.  The quad that makes
// the parent's count complete goes on there; nobody waits.  sweep 0: the BLASes; 1: the world trees.
// arrive must be all 0 before sweep 0.  min / max are exact, so the result does not depend on timing.
__global__ __launch_bounds__(WB_BLOCK) void k_rf_fit(RfWork w, int sweep) {
    const int slot = threadIdx.x & 3;
    int32_t node = blockIdx.x * RF_QUADS + (threadIdx.x >> 2);
    if (node >= w.n_nodes || w.kids[node] != 0) return;  // uniform over the quad
    const int32_t root = w.wtree[node];
    const bool world = root == w.oroot || root == w.lroot;
    if (world != (sweep == 1)) return;
    const lumo_object* table = root == w.lroot ? w.lights : w.objs;
    const int32_t* blas = root == w.lroot ? w.lblas : w.oblas;
    const int n_table = root == w.lroot ? w.n_lights : w.n_objs;
    const int quad0 = lane_id() & ~3;
    for (;;) {
        wbvh::Node& nd = w.nodes[node];
        WbBox b;
        rf_empty(b);
        if (slot < nd.n) {
            const int32_t r = nd.ref[slot];
            if (r >= 0) {
                if (r < w.n_nodes) b = w.box[r];
            } else if (wbvh::leaf_count(r) > 0) {
                rf_leaf_box(w, r, b);
            } else if (world && wbvh::leaf_first(r) < n_table) {
                rf_object_box(w, table[wbvh::leaf_first(r)], blas[wbvh::leaf_first(r)], b);
            }
            for (int a = 0; a < 3; ++a) {
                nd.lo[a][slot] = wb_f_down(b.lo[a]);
                nd.hi[a][slot] = wb_f_up(b.hi[a]);
            }
        }
        for (int a = 0; a < 3; ++a) {
            b.lo[a] = rf_quad_min(b.lo[a]);
            b.hi[a] = rf_quad_max(b.hi[a]);
        }
        const int32_t p = w.parent[node];
        uint32_t before = 0;
        if (slot == 0) {
            w.box[node] = b;
            __threadfence();
            if (p >= 0) before = atomicAdd(&w.arrive[p >> 2], 1u);
        }
        before = __shfl(before, quad0);
        if (p < 0 || before + 1 != w.kids[p >> 2]) return;
        __threadfence();
        node = p >> 2;
    }
}

// ---------------------------------------------------------------- 4. derived values, staged sets
// k_wb_rootarea's rule, per root node: the half-area of the union of its child boxes
__global__ __launch_bounds__(WB_BLOCK) void k_rf_rootarea(RfWork w) {
    const int i = blockIdx.x * WB_BLOCK + threadIdx.x;
    if (i >= w.n_nodes || w.parent[i] >= 0) return;
    const wbvh::Node& nd = w.nodes[i];
    WbBox b;
    rf_empty(b);
    for (int k = 0; k < nd.n; ++k)
        for (int a = 0; a < 3; ++a) {
            if ((double)nd.lo[a][k] < b.lo[a]) b.lo[a] = nd.lo[a][k];
            if ((double)nd.hi[a][k] > b.hi[a]) b.hi[a] = nd.hi[a][k];
        }
    w.rarea[i] = wb_half_area(b);
}

__global__ __launch_bounds__(WB_BLOCK) void k_rf_copy(uint4* dst, const uint4* src, size_t n16) {
    for (size_t i = (size_t)blockIdx.x * WB_BLOCK + threadIdx.x; i < n16; i += (size_t)gridDim.x * WB_BLOCK) dst[i] = src[i];
}

// lumo_scene_motion_mark: the vertex array into the previous vertices, 16 B per lane; n doubles, of
// which an odd last one goes alone (3 per vertex: the byte count is a multiple of 8 only)
__global__ __launch_bounds__(WB_BLOCK) void k_rf_mark(double* dst, const double* src, size_t n) {
    const size_t n16 = n / 2, first = (size_t)blockIdx.x * WB_BLOCK + threadIdx.x;
    const double2* s2 = reinterpret_cast<const double2*>(src);
    double2* d2 = reinterpret_cast<double2*>(dst);
    for (size_t i = first; i < n16; i += (size_t)gridDim.x * WB_BLOCK) d2[i] = s2[i];
    if (first == 0 && (n & 1)) dst[n - 1] = src[n - 1];
}

}  // namespace dev
}  // namespace lumo
