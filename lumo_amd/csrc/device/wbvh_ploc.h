// Clustered variant of the device builder: parallel locally-ordered clustering
// (PLOC, Meister & Bittner 2018) in place of steps 4 and 5 of wbvh_dev.h.  The binary tree is built
// bottom-up: the live clusters of every tree lie in one compact array in Morton order (a tree's
// clusters stay contiguous: compaction is stable), and an iteration merges every pair of clusters
// that are each other's nearest neighbour by the half-area of the union box, searched within
// +-radius positions.  The kernels, in the order device/wbvh_dev.hip launches them:
//   k_pl_init                   one cluster per sorted primitive: ref ~position, tree, f64 box
//   per iteration, n live clusters (the host reads the number of merges back, 4 bytes):
//     k_pl_nearest              a block stages its 256 clusters and a halo of `radius` on both sides in
//                               LDS (structure of arrays, conflict-free); each thread scans its window
//     k_pl_pair                 instead, after max_iter iterations: clusters 2k and 2k + 1 of each tree
//     k_pl_flag                 "leads a merge" and "survives" per cluster, one array of 2n flags for
//                               one exclusive scan; the live count of every tree
//     k_pl_merge                a leader makes the internal slot (children, parent links, union box,
//                               count, object flag: final, no fit pass) and every survivor moves to its
//                               scanned position of the other buffer: merge and stable compaction in one
//   k_pl_order                  relabel: PLOC subtrees are no ranges of the Morton order, so every leaf
//                               climbs to its root for its in-order position; idx, the leaf refs of
//                               child, lparent and ifirst follow
// Slots: tree t with `live` clusters has made size - live merges, into the slots tree_base[t] + live - 1
// .. tree_base[t] + size - 2.  The merges of an iteration take tree_base[t] + live - 2 downward in
// cluster order (rank from the scan), so the last merge of a tree lands on tree_base[t]: wbvh_dev.h's
// convention, and steps 6 to 8 run unchanged.  No atomic anywhere: two builds are byte-identical.
//
// Progress.  d(i, j), the half-area of the union, is symmetric bit for bit (min / max commute; a NaN
// counts as +inf), and a thread keeps the smallest d, the smaller j on ties.  In a tree of two or
// more clusters let d* be the least d over its pairs within the radius (neighbours are such a pair),
// a the smallest index in any pair that attains d*, b its smallest partner among them.  nn[a] = b:
// nothing is below d*, and b is the smallest j that ties.  nn[b] = a: a attains d*, and a j < a with
// d(b, j) = d* would be an index in such a pair below a.  So every such tree merges at least one pair
// per iteration.  That can still be one pair only (nested boxes), hence max_iter and k_pl_pair, which
// halves every tree.
#pragma once
#include "wbvh_dev.h"

namespace lumo {
namespace dev {

constexpr int PL_RADIUS_MAX = 64;
constexpr int PL_SPAN = WB_BLOCK + 2 * PL_RADIUS_MAX;  // clusters a block stages at most

struct PlWork {
    int32_t radius;
    int32_t *cref[2], *ctree[2];  // live clusters: binary ref, tree; read from [cur], survivors to [cur ^ 1]
    WbBox* cbox[2];
    int32_t* cstart[2];  // per tree: the position of its first live cluster
    int32_t* tlive;      // per tree: live clusters at the start of the iteration
    int32_t* nn;         // per cluster: its nearest neighbour, -1: none (alone in its tree)
    uint32_t *flag, *scan;  // 2n: [0, n) leads a merge, [n, 2n) survives; the exclusive scan
    int32_t* lpar;       // per old position: 2 * parent slot + side of the leaf
    uint32_t* idx_out;   // idx after the relabel
};

__device__ __forceinline__ WbBox pl_union(const WbBox& a, const WbBox& b) {
    WbBox u;
    for (int x = 0; x < 3; ++x) {
        u.lo[x] = b.lo[x] < a.lo[x] ? b.lo[x] : a.lo[x];
        u.hi[x] = a.hi[x] < b.hi[x] ? b.hi[x] : a.hi[x];
    }
    return u;
}

__global__ __launch_bounds__(WB_BLOCK) void k_pl_init(WbWork w, PlWork pl) {
    const int g = blockIdx.x * WB_BLOCK + threadIdx.x;
    if (g >= w.n_prims) return;
    const int t = wb_tree_of(w.tree_base, w.n_trees, g);
    pl.cref[0][g] = ~g;
    pl.ctree[0][g] = t;
    pl.cbox[0][g] = w.pbox[w.idx[g]];
    if (g == w.tree_base[t]) pl.cstart[0][t] = g;
}

__global__ __launch_bounds__(WB_BLOCK) void k_pl_nearest(PlWork pl, int cur, int n) {
    __shared__ double sb[6][PL_SPAN];
    __shared__ int32_t st[PL_SPAN];
    const int r = pl.radius, first = (int)(blockIdx.x * WB_BLOCK) - r;
    for (int k = threadIdx.x; k < WB_BLOCK + 2 * r; k += WB_BLOCK) {
        const int j = first + k;
        int32_t t = -1;  // outside the array: no tree's
        if (j >= 0 && j < n) {
            t = pl.ctree[cur][j];
            const WbBox b = pl.cbox[cur][j];
            for (int a = 0; a < 3; ++a) {
                sb[a][k] = b.lo[a];
                sb[3 + a][k] = b.hi[a];
            }
        }
        st[k] = t;
    }
    __syncthreads();
    const int li = threadIdx.x + r, i = first + li;
    if (i >= n) return;
    const int32_t t = st[li];
    WbBox me;
    for (int a = 0; a < 3; ++a) {
        me.lo[a] = sb[a][li];
        me.hi[a] = sb[3 + a][li];
    }
    int best = -1;
    double bd = 0.0;
    for (int k = li - r; k <= li + r; ++k) {
        if (k == li || st[k] != t) continue;
        WbBox o;
        for (int a = 0; a < 3; ++a) {
            o.lo[a] = sb[a][k];
            o.hi[a] = sb[3 + a][k];
        }
        double d = wb_half_area(k < li ? pl_union(o, me) : pl_union(me, o));  // the pair in array order: d(i, j) == d(j, i)
        if (!(d == d)) d = HUGE_VAL;
        if (best < 0 || d < bd) {
            bd = d;
            best = k;
        }
    }
    pl.nn[i] = best < 0 ? -1 : first + best;
}

__global__ __launch_bounds__(WB_BLOCK) void k_pl_pair(PlWork pl, int cur, int n) {
    const int i = blockIdx.x * WB_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t t = pl.ctree[cur][i], s = pl.cstart[cur][t];
    const int j = s + ((i - s) ^ 1);
    pl.nn[i] = j < n && pl.ctree[cur][j] == t ? j : -1;
}

__global__ __launch_bounds__(WB_BLOCK) void k_pl_flag(PlWork pl, int cur, int n) {
    const int i = blockIdx.x * WB_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int j = pl.nn[i];
    const bool mutual = j >= 0 && j < n && pl.nn[j] == i;
    pl.flag[i] = mutual && i < j ? 1u : 0u;
    pl.flag[(size_t)n + i] = mutual && j < i ? 0u : 1u;  // the pair's second cluster goes
    const int32_t t = pl.ctree[cur][i];
    if (i == n - 1 || pl.ctree[cur][i + 1] != t) pl.tlive[t] = i + 1 - pl.cstart[cur][t];
}

// primitive count and object flag of a cluster
__device__ __forceinline__ int32_t pl_count(const WbWork& w, int32_t ref) {
    if (ref >= 0) return w.icount[ref];
    return 1 | (w.ptri[w.idx[~ref]] < 0 ? WB_HASOBJ : 0);
}
__device__ __forceinline__ void pl_set_parent(const WbWork& w, const PlWork& pl, int32_t ref, int32_t slot, int side) {
    if (ref >= 0) w.iparent[ref] = slot; else pl.lpar[~ref] = 2 * slot + side;
}

__global__ __launch_bounds__(WB_BLOCK) void k_pl_merge(WbWork w, PlWork pl, int cur, int n) {
    const int i = blockIdx.x * WB_BLOCK + threadIdx.x;
    if (i >= n || !pl.flag[(size_t)n + i]) return;
    const uint32_t p = pl.scan[(size_t)n + i] - pl.scan[n];  // scan[n]: the merges; p: the survivors before i
    if (p >= (uint32_t)n) return;  // never: p counts clusters before i
    const int32_t t = pl.ctree[cur][i];
    if (i == 0 || pl.ctree[cur][i - 1] != t) pl.cstart[cur ^ 1][t] = (int32_t)p;  // a tree's first cluster never goes
    int32_t ref = pl.cref[cur][i];
    WbBox box = pl.cbox[cur][i];
    if (pl.flag[i]) {
        const int j = pl.nn[i];
        const int32_t b0 = w.tree_base[t], size = w.tree_base[t + 1] - b0;
        const int32_t rank = (int32_t)(pl.scan[i] - pl.scan[pl.cstart[cur][t]]);
        const int32_t s = b0 + pl.tlive[t] - 2 - rank;
        if (s < b0 || s > b0 + size - 2) return;  // never: a tree of `live` clusters merges at most live - 1 pairs
        const int32_t rb = pl.cref[cur][j], ca = pl_count(w, ref), cb = pl_count(w, rb);
        box = pl_union(box, pl.cbox[cur][j]);
        w.child[2 * (size_t)s] = ref;
        w.child[2 * (size_t)s + 1] = rb;
        pl_set_parent(w, pl, ref, s, 0);
        pl_set_parent(w, pl, rb, s, 1);
        w.ibox[s] = box;
        w.icount[s] = ((ca & ~WB_HASOBJ) + (cb & ~WB_HASOBJ)) | ((ca | cb) & WB_HASOBJ);
        w.iparent[s] = -1;  // until a later merge takes it
        ref = s;
    }
    pl.cref[cur ^ 1][p] = ref;
    pl.ctree[cur ^ 1][p] = t;
    pl.cbox[cur ^ 1][p] = box;
}

// One thread per leaf.  Its new position within the tree is the number of primitives to its left:
// on the climb, the count of the left sibling wherever the path comes up from a right child.  The
// slots the path reaches through left children only have this leaf as their leftmost: their ifirst.
__global__ __launch_bounds__(WB_BLOCK) void k_pl_order(WbWork w, PlWork pl) {
    const int g = blockIdx.x * WB_BLOCK + threadIdx.x;
    if (g >= w.n_prims) return;
    const int t = wb_tree_of(w.tree_base, w.n_trees, g);
    const int32_t b0 = w.tree_base[t], size = w.tree_base[t + 1] - b0;
    if (size < 2) {  // a tree of one leaf has no slot
        pl.idx_out[g] = w.idx[g];
        return;
    }
    const int32_t lp = pl.lpar[g];
    int32_t cur = lp >> 1, sum = 0, lead = 0;
    bool right = lp & 1, leftmost = true;
    for (int32_t step = 0; step < size; ++step) {  // a path has fewer than `size` slots
        if (right) {
            const int32_t l = w.child[2 * (size_t)cur];
            sum += l < 0 ? 1 : w.icount[l] & ~WB_HASOBJ;
            leftmost = false;
        } else if (leftmost) {
            lead++;
        }
        const int32_t up = w.iparent[cur];
        if (up < 0) break;
        right = w.child[2 * (size_t)up + 1] == cur;  // cur >= 0: no leaf ref, whatever its state, equals it
        cur = up;
    }
    if (sum >= size) return;  // never: the primitives to the left of one are fewer than all
    const int32_t pos = b0 + sum;
    pl.idx_out[pos] = w.idx[g];
    w.lparent[pos] = lp >> 1;
    w.child[2 * (size_t)(lp >> 1) + (lp & 1)] = ~pos;  // this leaf's own entry: nobody else compares it
    cur = lp >> 1;
    for (int32_t k = 0; k < lead; ++k) {
        w.ifirst[cur] = pos;
        cur = w.iparent[cur];
    }
}

}  // namespace dev
}  // namespace lumo
