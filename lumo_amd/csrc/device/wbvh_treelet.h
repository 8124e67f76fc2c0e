// Treelet restructuring of the clustered binary tree (Karras & Aila 2013, §3): a pass
// between the last merge of wbvh_ploc.h and its relabel k_pl_order.  The objective is the sum of
// wb_half_area(box) over the internal binary slots; include/lumo_amd.h states the construction.
//   k_tl_area_partial / _final  the objective over all trees, a fixed-order block reduction
//   k_tl_pass                   one pass, bottom-up
// k_tl_pass, one wave per block.  A lane per primitive climbs from its leaf as in k_wb_fit: at a slot
// the first arrival stops, the second carries on after the fence, so a slot is visited when both of
// its subtrees are finished and nobody waits for another wave.  A lane that stops stays in the wave:
// the wave finds the lanes that stand on a slot of gamma primitives or more by ballot and handles
// their treelets one after another, all 64 lanes on one treelet:
//   formation  lane k < 7 holds treelet leaf k in registers; the leaf to open is an argmax over 7
//              shuffles, the leaves behind it move up one lane, two lanes load the children
//   areas      the 7 leaf boxes lie in LDS (structure of arrays); lane l unions subsets l and l + 64
//   DP         by subset size k = 2 .. 7.  A subset has 2^(k-1) - 1 partitions that keep its lowest
//              leaf on the left, so 2^(k-1) lanes take one subset and 64 / 2^(k-1) subsets run side
//              by side (20 rounds in all); the minimum over (cost, P) is a butterfly of k - 1 xor
//              shuffles within the group.  a, c (128 x 8 B each) and the best P (128 B) live in LDS
//   rebuild    lane 0 lists the 6 subsets of the optimal topology in pre-order; lanes 0 .. 5 write one
//              slot each: children, their parent links, the union box, count and object flag
// Unrelated slots have disjoint subtrees, and a treelet lies within the subtree of its root, which is
// finished: no other wave reads or writes what a treelet rewrites, and the result does not depend on
// timing.  The only atomics are the integer arrival counter and the two integer tallies.  Every loop
// has a static bound.  The arrival counters (w.iflag, which the clustered build does not use
// otherwise) are cleared by k_wb_fill on the build's stream before every pass.
#pragma once
#include "wbvh_ploc.h"

namespace lumo {
namespace dev {

constexpr int TL_BLOCK = 64;   // one wave
constexpr int TL_LEAVES = 7;
constexpr int TL_SETS = 1 << TL_LEAVES;
constexpr int TL_GAMMA = 7;    // lumo_wide_treelet_cfg.gamma = 0
constexpr int TL_GAMMA_MAX = 1 << 20;
constexpr int TL_PASSES_MAX = 8;

struct TlStat {  // what the host reads back
    unsigned long long tried, replaced;
    double area[2];  // the objective before the first pass and after the last
};

// the non-empty subsets of 7 leaves by size, ascending within a size; off[k]: the first of size k
struct TlTab {
    uint8_t s[TL_SETS];
    uint8_t off[TL_LEAVES + 2];
    constexpr TlTab() : s{}, off{} {
        int n = 0;
        for (int k = 1; k <= TL_LEAVES; ++k) {
            off[k] = (uint8_t)n;
            for (int m = 1; m < TL_SETS; ++m) {
                int bits = 0;
                for (int b = 0; b < TL_LEAVES; ++b) bits += (m >> b) & 1;
                if (bits == k) s[n++] = (uint8_t)m;
            }
        }
        off[TL_LEAVES + 1] = (uint8_t)n;
    }
};
static __constant__ const TlTab TL_TAB = TlTab();

__device__ __forceinline__ double tl_area(const WbBox& b) {
    const double a = wb_half_area(b);
    return a == a ? a : HUGE_VAL;
}

// ---------------------------------------------------------------- the objective
// block b strides from b over the slots, fixed grid: the order of the sum does not depend on the run
__global__ __launch_bounds__(WB_BLOCK) void k_tl_area_partial(WbWork w, double* part) {
    __shared__ float lm[WB_BLOCK];
    __shared__ double ls[WB_BLOCK];
    float mx = 0.0f;
    double sum = 0.0;
    for (int64_t g = (int64_t)blockIdx.x * WB_BLOCK + threadIdx.x; g < w.n_prims; g += (int64_t)gridDim.x * WB_BLOCK) {
        const int t = wb_tree_of(w.tree_base, w.n_trees, (int)g);
        if (g - w.tree_base[t] < w.tree_base[t + 1] - w.tree_base[t] - 1) sum += tl_area(w.ibox[g]);
    }
    wb_block_stat(mx, sum, lm, ls);
    if (threadIdx.x == 0) part[blockIdx.x] = sum;
}
__global__ __launch_bounds__(WB_BLOCK) void k_tl_area_final(int n_part, const double* part, TlStat* st, int which) {
    __shared__ float lm[WB_BLOCK];
    __shared__ double ls[WB_BLOCK];
    float mx = 0.0f;
    double sum = (int)threadIdx.x < n_part ? part[threadIdx.x] : 0.0;
    wb_block_stat(mx, sum, lm, ls);
    if (threadIdx.x == 0) st->area[which] = sum;
}

// ---------------------------------------------------------------- one pass
// half-area of a treelet leaf that can be opened (an internal slot); -1: a primitive
__device__ __forceinline__ double tl_open_area(const WbWork& w, int32_t ref) {
    return ref >= 0 && ref < w.n_prims ? tl_area(w.ibox[ref]) : -1.0;
}

struct TlLds {
    double box[6][8];  // the treelet leaves' boxes: lo x y z, hi x y z
    double a[TL_SETS], c[TL_SETS];
    double cost[8];    // of the present topology, per internal node
    int32_t ref[8], cnt[8];
    int32_t slot[8], ch[8][2];  // the 6 internal slots, the root first, then as they were opened; their children
    uint8_t p[TL_SETS], at[TL_SETS];  // the best partition; a subset's place in `node`
    uint8_t mask[8], node[8], stk[8];
    int32_t ok;
};

// the union of the boxes of `set`, ascending
__device__ __forceinline__ WbBox tl_union(const TlLds& s, int set) {
    WbBox u{};
    bool any = false;
    for (int k = 0; k < TL_LEAVES; ++k) {
        if (!((set >> k) & 1)) continue;
        WbBox b;
        for (int x = 0; x < 3; ++x) {
            b.lo[x] = s.box[x][k];
            b.hi[x] = s.box[3 + x][k];
        }
        u = any ? pl_union(u, b) : b;
        any = true;
    }
    return u;
}

// The treelet at slot R, by the whole wave (R is the same in every lane).  Returns 0: skipped,
// 1: tried, 2: replaced.
__device__ __forceinline__ int tl_treelet(const WbWork& w, const PlWork& pl, TlLds& s, int32_t R, int lane) {
    // formation: lane k holds leaf k
    int32_t lref = lane < 2 ? w.child[2 * (size_t)R + lane] : -1;
    double la = lane < 2 ? tl_open_area(w, lref) : -1.0;
    if (lane == 0) s.slot[0] = R;
    if (lane < 2) s.ch[0][lane] = lref;
    int nl = 2;
    for (int e = 1; e < TL_LEAVES - 1; ++e) {
        int best = -1;
        double ba = -1.0;
        for (int k = 0; k < TL_LEAVES; ++k) {
            const double a = __shfl(la, k);
            if (k < nl && a > ba) {  // the first of the largest
                ba = a;
                best = k;
            }
        }
        best = __builtin_amdgcn_readfirstlane(best);
        if (best < 0) break;
        const int32_t x = __shfl(lref, best), up = __shfl_up(lref, 1);
        const double ua = __shfl_up(la, 1);
        if (lane > best + 1) {
            lref = up;
            la = ua;
        }
        if (lane == best || lane == best + 1) {
            lref = w.child[2 * (size_t)x + (lane - best)];
            la = tl_open_area(w, lref);
            s.ch[e][lane - best] = lref;
        }
        if (lane == 0) s.slot[e] = x;
        nl++;
    }
    if (nl < TL_LEAVES) return 0;
    const bool mine = lane < TL_LEAVES;
    const bool bad = mine && !(lref < 0 ? ~lref < w.n_prims : lref < w.n_prims);
    if (__ballot(bad)) return 0;  // never: every ref of a tree is a slot or a position
    if (mine) {
        const WbBox b = lref < 0 ? w.pbox[w.idx[~lref]] : w.ibox[lref];
        for (int x = 0; x < 3; ++x) {
            s.box[x][lane] = b.lo[x];
            s.box[3 + x][lane] = b.hi[x];
        }
        s.ref[lane] = lref;
        s.cnt[lane] = pl_count(w, lref);
    }
    __syncthreads();
    // areas of the subsets, 2 per lane
    for (int h = 0; h < 2; ++h) {
        const int set = lane + 64 * h;  // the empty set: the zero box, area 0
        s.a[set] = tl_area(tl_union(s, set));
        s.c[set] = 0.0;  // the singletons'; the others' follow
    }
    __syncthreads();
    // the cost of the present topology with the DP's own sums: one of its candidates, so c(all) <= it
    if (lane == 0) {
        for (int i = TL_LEAVES - 2; i >= 0; --i) {
            int m = 0;
            double below = 0.0;
            for (int side = 0; side < 2; ++side) {
                const int32_t c = s.ch[i][side];
                int sm = 0;
                for (int j = i + 1; j < TL_LEAVES - 1; ++j)
                    if (c >= 0 && s.slot[j] == c) {
                        sm = s.mask[j];
                        below += s.cost[j];
                    }
                if (!sm)
                    for (int k = 0; k < TL_LEAVES; ++k)
                        if (s.ref[k] == c) sm = 1 << k;
                m |= sm;
            }
            s.mask[i] = (uint8_t)m;
            s.cost[i] = s.a[m & (TL_SETS - 1)] + below;
        }
        s.ok = s.mask[0] == TL_SETS - 1;
    }
    // c(S) = a(S) + min over P of c(P) + c(S \ P), by size
    for (int k = 2; k <= TL_LEAVES; ++k) {
        const int group = 1 << (k - 1), per = 64 >> (k - 1), first = TL_TAB.off[k], count = TL_TAB.off[k + 1] - first;
        const int sub = lane >> (k - 1), j = lane & (group - 1);
        for (int r = 0; r * per < count; ++r) {
            const int si = r * per + sub;
            const bool valid = si < count;
            const int S = valid ? TL_TAB.s[first + si] : 0;
            int P = S & -S, rest = S ^ P, jj = j;  // P: the lowest leaf, and bit i of j at the i-th other leaf of S
            for (int b = 0; b < TL_LEAVES; ++b)
                if ((rest >> b) & 1) {
                    if (jj & 1) P |= 1 << b;
                    jj >>= 1;
                }
            const bool use = valid && P != S;
            double cost = use ? s.c[P] + s.c[S ^ P] : HUGE_VAL;
            int bp = use ? P : 255;
            for (int d = 1; d < group; d <<= 1) {
                const double oc = __shfl_xor(cost, d);
                const int op = __shfl_xor(bp, d);
                if (oc < cost || (oc == cost && op < bp)) {
                    cost = oc;
                    bp = op;
                }
            }
            if (valid && j == 0) {
                s.c[S] = s.a[S] + cost;
                s.p[S] = (uint8_t)bp;
            }
        }
        __syncthreads();
    }
    // the optimal topology in pre-order (node, left, right), left the part with the lowest leaf
    if (lane == 0 && s.ok) {
        int n = 0, sp = 0;
        s.stk[sp++] = TL_SETS - 1;
        for (int it = 0; it < TL_LEAVES - 1 && sp > 0; ++it) {
            const int m = s.stk[--sp], P = s.p[m], Q = m ^ P;
            if (P == 0 || Q == 0 || (P & ~m)) break;  // never: the DP chose a proper part of m
            s.node[n] = (uint8_t)m;
            s.at[m] = (uint8_t)n;
            n++;
            if (__popc(Q) > 1) s.stk[sp++] = (uint8_t)Q;
            if (__popc(P) > 1) s.stk[sp++] = (uint8_t)P;
        }
        s.ok = n == TL_LEAVES - 1 && sp == 0;
    }
    __syncthreads();
    const bool replace = s.ok && s.c[TL_SETS - 1] < s.cost[0];
    if (replace && lane < TL_LEAVES - 1) {  // node `lane` of the pre-order takes slot `lane`
        const int m = s.node[lane];
        const int32_t slot = s.slot[lane];
        int32_t total = 0;
        for (int side = 0; side < 2; ++side) {
            const int part = side ? m ^ s.p[m] : s.p[m];
            int32_t ref;
            if (__popc(part) == 1) {
                ref = s.ref[__ffs(part) - 1];
                pl_set_parent(w, pl, ref, slot, side);
            } else {
                ref = s.slot[s.at[part] & 7];
                w.iparent[ref] = slot;
            }
            w.child[2 * (size_t)slot + side] = ref;
        }
        for (int k = 0; k < TL_LEAVES; ++k)
            if ((m >> k) & 1) total = ((total & ~WB_HASOBJ) + (s.cnt[k] & ~WB_HASOBJ)) | ((total | s.cnt[k]) & WB_HASOBJ);
        w.ibox[slot] = tl_union(s, m);
        w.icount[slot] = total;
    }
    __threadfence();
    __syncthreads();  // LDS is free for the next treelet
    return replace ? 2 : 1;
}

__global__ __launch_bounds__(TL_BLOCK) void k_tl_pass(WbWork w, PlWork pl, int32_t gamma, TlStat* st) {
    __shared__ TlLds s;
    const int lane = threadIdx.x, g = blockIdx.x * TL_BLOCK + lane;
    int32_t cur = -1;
    if (g < w.n_prims) {
        const int t = wb_tree_of(w.tree_base, w.n_trees, g);
        if (w.tree_base[t + 1] - w.tree_base[t] >= 2) cur = pl.lpar[g] >> 1;  // a tree of one leaf has no slot
    }
    unsigned tried = 0, replaced = 0;
    for (int32_t step = 0; step < w.n_prims; ++step) {  // a path has fewer slots than the tree primitives
        if (cur >= 0 && atomicAdd(&w.iflag[cur], 1u) == 0u) cur = -1;  // the first arrival stops
        if (!__ballot(cur >= 0)) break;
        __threadfence();
        unsigned long long todo = __ballot(cur >= 0 && (w.icount[cur] & ~WB_HASOBJ) >= gamma);
        for (int it = 0; it < 64 && todo; ++it, todo &= todo - 1) {
            const int32_t R = __builtin_amdgcn_readfirstlane(__shfl(cur, __ffsll((long long)todo) - 1));
            const int did = __builtin_amdgcn_readfirstlane(tl_treelet(w, pl, s, R, lane));
            tried += did >= 1;
            replaced += did == 2;
        }
        if (cur >= 0) cur = w.iparent[cur];  // -1 above a root
    }
    if (lane == 0 && tried) {
        atomicAdd(&st->tried, (unsigned long long)tried);
        atomicAdd(&st->replaced, (unsigned long long)replaced);
    }
}

}  // namespace dev
}  // namespace lumo
