// Device builder of the wide BVH: the launches of the kernels of wbvh_dev.h,
// wbvh_ploc.h and wbvh_treelet.h, and the entry points lumo_scene_set_wide_build,
// lumo_scene_wide_build_info, lumo_scene_set_wide_cluster, lumo_scene_wide_cluster_info,
// lumo_scene_set_wide_treelet, lumo_scene_wide_treelet_info and lumo_debug_wide_export.
// lumo_scene_upload (upload.hip) calls wide_build_device when the context asks for this builder.
// Also the refit of a tree of either builder after its vertices moved (the kernels of wbvh_refit.h):
// lumo_scene_update_vertices and lumo_scene_refit_info.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "ctx.h"
#include "wbvh_dev.h"
#include "wbvh_ploc.h"
#include "wbvh_refit.h"
#include "wbvh_treelet.h"

using namespace lumo;
using namespace lumo::dev;

namespace {

// workspace of one build: freed when the build returns
struct Bufs {
    std::vector<DevBuf> v;
    ~Bufs() {
        for (DevBuf& b : v)
            if (b.p) (void)hipFree(b.p);
    }
    template <typename T>
    lumo_status get(const Ctx& c, T** p, size_t count) {
        v.emplace_back();
        const lumo_status st = dev_alloc(c, v.back(), sizeof(T) * std::max<size_t>(count, 1));
        *p = static_cast<T*>(v.back().p);
        return st;
    }
    template <typename T>
    lumo_status put(const Ctx& c, const T** p, const std::vector<T>& host) {
        T* q = nullptr;
        const lumo_status st = get(c, &q, host.size());
        if (st) return st;
        if (!host.empty()) HIPCHK(hipMemcpy(q, host.data(), sizeof(T) * host.size(), hipMemcpyHostToDevice));
        *p = q;
        return LUMO_OK;
    }
};

// lumo_wide_cluster_cfg.max_iter = 0: nearest-neighbour iterations before adjacent clusters are paired;
// twice the largest count measured, 78
constexpr int PL_ITER_CAP = 156;

inline int blocks(size_t n) { return (int)((n + WB_BLOCK - 1) / WB_BLOCK); }

#define WB_TRY(x)                      \
    do {                               \
        const lumo_status s__ = (x);   \
        if (s__) return s__;           \
    } while (0)

struct Events {
    hipEvent_t a = nullptr, b = nullptr, c = nullptr, d = nullptr, e = nullptr, f = nullptr;  // the build; its clustering; its treelet passes
    uint32_t* pinned = nullptr;
    ~Events() {
        for (hipEvent_t x : {a, b, c, d, e, f})
            if (x) (void)hipEventDestroy(x);
        if (pinned) (void)hipHostFree(pinned);
    }
};

}  // namespace

namespace lumo {
namespace dev {

void wide_dev_free(WideDev& wd) {
    for (DevBuf* b : {&wd.nodes, &wd.tv})
        if (b->p) {
            (void)hipFree(b->p);
            *b = DevBuf{};
        }
}

lumo_status wide_build_device(Ctx& c, const wbvh::DevPrep& prep, int num_triangles, WideDev& out) {
    out = WideDev{};
    const int T = (int)prep.tree_base.size() - 1;
    if (T < 2 || T > 65535 || !prep.ok) return LUMO_OK;  // 65535: the tree is a grid dimension (k_wb_cb_partial)
    const size_t N = (size_t)prep.tree_base[T];
    for (const wbvh::DevSeg& s : prep.segs)
        if (s.tri_base >= 0 && (s.count <= 0 || (int64_t)s.tri_base + s.count > num_triangles)) return LUMO_OK;
    out.root_ref.assign(T, wbvh::NONE);
    if (N == 0) {  // no primitive anywhere: every root NONE
        WB_TRY(dev_alloc(c, out.nodes, 0));
        WB_TRY(dev_alloc(c, out.tv, 0));
        out.ok = true;
        return LUMO_OK;
    }
    hipStream_t sm = c.streams[0];
    Bufs ws;
    Events ev;
    HIPCHK(hipEventCreate(&ev.a));
    HIPCHK(hipEventCreate(&ev.b));
    HIPCHK(hipEventCreate(&ev.c));
    HIPCHK(hipEventCreate(&ev.d));
    HIPCHK(hipEventCreate(&ev.e));
    HIPCHK(hipEventCreate(&ev.f));
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&ev.pinned), sizeof(uint32_t) * 2));
    WbWork w{};
    w.n_prims = (int32_t)N;
    w.n_trees = T;
    w.n_segs = (int32_t)prep.segs.size();
    w.leaf_max = c.wb_cfg.leaf_max;
    w.vertices = c.sc.vertices;
    w.tris = c.sc.tris;
    WB_TRY(ws.put(c, &w.segs, prep.segs));
    WB_TRY(ws.put(c, &w.tree_base, prep.tree_base));
    WB_TRY(ws.put(c, &w.obj_box, prep.obj_box));
    uint64_t* key[2];
    uint32_t* idx[2];
    uint32_t *flag, *hist, *offs, *sums;
    const int rx_blocks = (int)((N + RX_TILE - 1) / RX_TILE);
    const size_t n_hist = (size_t)RX_BINS * rx_blocks;
    WB_TRY(ws.get(c, &w.pbox, N));
    WB_TRY(ws.get(c, &w.ptri, N));
    WB_TRY(ws.get(c, &w.pobj, N));
    WB_TRY(ws.get(c, &w.cbound, (size_t)T));
    WB_TRY(ws.get(c, &w.cpart, (size_t)T * WB_RED_GRID));
    for (int k = 0; k < 2; ++k) {
        WB_TRY(ws.get(c, &key[k], N));
        WB_TRY(ws.get(c, &idx[k], N));
    }
    WB_TRY(ws.get(c, &w.child, 2 * N));
    WB_TRY(ws.get(c, &w.iparent, N));
    WB_TRY(ws.get(c, &w.lparent, N));
    WB_TRY(ws.get(c, &w.ifirst, N));
    WB_TRY(ws.get(c, &w.ibox, N));
    WB_TRY(ws.get(c, &w.icount, N));
    WB_TRY(ws.get(c, &w.iflag, N));
    WB_TRY(ws.get(c, &w.rec_pos, N));
    WB_TRY(ws.get(c, &w.root_ref, (size_t)T));
    WB_TRY(ws.get(c, &w.scal, 1));
    WB_TRY(ws.get(c, &flag, N));
    WB_TRY(ws.get(c, &hist, n_hist));
    WB_TRY(ws.get(c, &offs, n_hist));
    WB_TRY(ws.get(c, &sums, (size_t)scan_blocks((uint32_t)std::max({n_hist, N, (size_t)T}))));
    // the clustered build (wbvh_ploc.h): the live clusters twice (120 B per primitive); its flags and
    // their scan take the key buffers, which nobody reads after the sort, the relabelled idx the spare one
    PlWork pl{};
    uint32_t* pl_sums = nullptr;
    TlStat* tl_stat = nullptr;
    double* tl_part = nullptr;
    const int tl_passes = c.wt_cfg.passes, tl_gamma = c.wt_cfg.gamma > 0 ? c.wt_cfg.gamma : TL_GAMMA;
    pl.radius = c.wc_cfg.radius;
    if (pl.radius > 0) {
        for (int k = 0; k < 2; ++k) {
            WB_TRY(ws.get(c, &pl.cref[k], N));
            WB_TRY(ws.get(c, &pl.ctree[k], N));
            WB_TRY(ws.get(c, &pl.cbox[k], N));
            WB_TRY(ws.get(c, &pl.cstart[k], (size_t)T));
        }
        WB_TRY(ws.get(c, &pl.tlive, (size_t)T));
        WB_TRY(ws.get(c, &pl.nn, N));
        WB_TRY(ws.get(c, &pl.lpar, N));
        WB_TRY(ws.get(c, &pl_sums, (size_t)scan_blocks((uint32_t)(2 * N))));
        // the treelet passes (wbvh_treelet.h) need nothing per primitive: their arrival counters are
        // w.iflag, which only the LBVH's fit uses before the collapse
        WB_TRY(ws.get(c, &tl_stat, 1));
        WB_TRY(ws.get(c, &tl_part, (size_t)WB_STAT_GRID));
    }
    WB_TRY(dev_alloc(c, out.tv, sizeof(double) * wbvh::TV * (size_t)prep.n_tris));
    w.tv = static_cast<double*>(out.tv.p);
    // scan[n - 1] + in[n - 1] of an exclusive scan: its total (one small read-back and a wait)
    auto total = [&](const uint32_t* in, const uint32_t* scan, size_t n, uint32_t* sum) -> lumo_status {
        HIPCHK(hipMemcpyAsync(ev.pinned, in + n - 1, sizeof(uint32_t), hipMemcpyDeviceToHost, sm));
        HIPCHK(hipMemcpyAsync(ev.pinned + 1, scan + n - 1, sizeof(uint32_t), hipMemcpyDeviceToHost, sm));
        HIPCHK(hipStreamSynchronize(sm));
        *sum = ev.pinned[0] + ev.pinned[1];
        return LUMO_OK;
    };
    const int nb = blocks(N), tb = blocks((size_t)T);

    HIPCHK(hipEventRecord(ev.a, sm));
    // 1. boxes, centroid bounds  2. keys
    w.key = key[0];
    w.idx = idx[0];
    k_wb_fill<<<1, WB_BLOCK, 0, sm>>>(reinterpret_cast<uint32_t*>(w.scal), 0u, (uint32_t)(sizeof(WbScal) / 4));
    k_wb_fill<<<nb, WB_BLOCK, 0, sm>>>(w.iflag, 0u, (uint32_t)N);
    k_wb_prims<<<nb, WB_BLOCK, 0, sm>>>(w);
    k_wb_cb_partial<<<dim3(WB_RED_GRID, T), WB_BLOCK, 0, sm>>>(w);
    k_wb_cb_final<<<T, WB_RED_GRID, 0, sm>>>(w);
    k_wb_morton<<<nb, WB_BLOCK, 0, sm>>>(w);
    // 3. sort by (tree, key): the 8 key digits, then the tree's
    const int passes = 8 + (T <= 256 ? 1 : (T <= 65536 ? 2 : 3));
    int cur = 0;
    for (int p = 0; p < passes; ++p) {
        k_rx_hist<<<rx_blocks, WB_BLOCK, 0, sm>>>(key[cur], idx[cur], (uint32_t)N, p, w.tree_base, T, hist);
        HIPCHK(exclusive_scan(hist, offs, (uint32_t)n_hist, sums, sm));
        k_rx_scatter<<<rx_blocks, WB_BLOCK, 0, sm>>>(key[cur], idx[cur], (uint32_t)N, p, w.tree_base, T, offs, key[cur ^ 1],
                                                     idx[cur ^ 1]);
        cur ^= 1;
    }
    w.key = key[cur];
    w.idx = idx[cur];
    if (pl.radius > 0) {
        // 4'. clusters  5'. merge mutual nearest neighbours until every tree is one cluster  5''. relabel
        pl.flag = reinterpret_cast<uint32_t*>(key[0]);
        pl.scan = reinterpret_cast<uint32_t*>(key[1]);
        pl.idx_out = idx[cur ^ 1];
        const int max_iter = c.wc_cfg.max_iter > 0 ? c.wc_cfg.max_iter : PL_ITER_CAP;
        size_t roots = 0;  // clusters left when every tree is done
        for (int t = 0; t < T; ++t) roots += prep.tree_base[t + 1] > prep.tree_base[t];
        HIPCHK(hipEventRecord(ev.c, sm));
        k_pl_init<<<nb, WB_BLOCK, 0, sm>>>(w, pl);
        int pc = 0;
        for (size_t n = N; n > roots;) {
            const bool nearest = out.cluster.iterations < max_iter;
            if (nearest)
                k_pl_nearest<<<blocks(n), WB_BLOCK, 0, sm>>>(pl, pc, (int)n);
            else
                k_pl_pair<<<blocks(n), WB_BLOCK, 0, sm>>>(pl, pc, (int)n);
            k_pl_flag<<<blocks(n), WB_BLOCK, 0, sm>>>(pl, pc, (int)n);
            HIPCHK(exclusive_scan(pl.flag, pl.scan, (uint32_t)(2 * n), pl_sums, sm));
            k_pl_merge<<<blocks(n), WB_BLOCK, 0, sm>>>(w, pl, pc, (int)n);
            HIPCHK(hipMemcpyAsync(ev.pinned, pl.scan + n, sizeof(uint32_t), hipMemcpyDeviceToHost, sm));  // the merges
            HIPCHK(hipStreamSynchronize(sm));
            const uint32_t merged = ev.pinned[0];
            if (merged > n - roots || (!nearest && merged == 0)) return LUMO_ERR_INVALID;  // cannot happen
            (nearest ? out.cluster.iterations : out.cluster.paired_iterations)++;
            n -= merged;
            pc ^= 1;
        }
        // 5t. the objective, and the treelet passes over the finished binary tree (gamma stays)
        const int ag = std::min(nb, WB_STAT_GRID);
        k_wb_fill<<<1, WB_BLOCK, 0, sm>>>(reinterpret_cast<uint32_t*>(tl_stat), 0u, (uint32_t)(sizeof(TlStat) / 4));
        k_tl_area_partial<<<ag, WB_BLOCK, 0, sm>>>(w, tl_part);
        k_tl_area_final<<<1, WB_BLOCK, 0, sm>>>(ag, tl_part, tl_stat, 0);
        if (tl_passes > 0) {
            HIPCHK(hipEventRecord(ev.e, sm));
            for (int p = 0; p < tl_passes; ++p) {
                k_wb_fill<<<nb, WB_BLOCK, 0, sm>>>(w.iflag, 0u, (uint32_t)N);
                k_tl_pass<<<(int)((N + TL_BLOCK - 1) / TL_BLOCK), TL_BLOCK, 0, sm>>>(w, pl, tl_gamma, tl_stat);
            }
            HIPCHK(hipEventRecord(ev.f, sm));
            k_tl_area_partial<<<ag, WB_BLOCK, 0, sm>>>(w, tl_part);
            k_tl_area_final<<<1, WB_BLOCK, 0, sm>>>(ag, tl_part, tl_stat, 1);
        }
        k_pl_order<<<nb, WB_BLOCK, 0, sm>>>(w, pl);
        HIPCHK(hipEventRecord(ev.d, sm));
        w.idx = pl.idx_out;
        out.cluster.radius_used = pl.radius;
    } else {
        // 4. radix tree  5. boxes bottom-up
        k_wb_radix<<<nb, WB_BLOCK, 0, sm>>>(w);
        k_wb_fit<<<nb, WB_BLOCK, 0, sm>>>(w);
    }
    // the records in sorted order
    k_wb_recflag<<<nb, WB_BLOCK, 0, sm>>>(w, flag);
    HIPCHK(exclusive_scan(flag, w.rec_pos, (uint32_t)N, sums, sm));
    k_wb_records<<<nb, WB_BLOCK, 0, sm>>>(w);
    // 6. collapse.  The wide nodes are at most the binary nodes that are no leaves.
    uint32_t cap = 0;
    k_wb_openflag<<<nb, WB_BLOCK, 0, sm>>>(w, flag);
    HIPCHK(exclusive_scan(flag, w.iflag, (uint32_t)N, sums, sm));  // iflag: free after k_wb_fit
    HIPCHK(hipGetLastError());
    WB_TRY(total(flag, w.iflag, N, &cap));
    const size_t lists = std::max<size_t>({(size_t)cap, (size_t)T, 1});
    uint32_t *cnt, *pos, *n_kids;
    int32_t *kids, *items[2];
    double* rarea;
    float* pmax;
    double* psum;
    WB_TRY(ws.get(c, &cnt, lists));
    WB_TRY(ws.get(c, &pos, lists));
    WB_TRY(ws.get(c, &n_kids, lists));
    WB_TRY(ws.get(c, &kids, 4 * lists));
    WB_TRY(ws.get(c, &items[0], lists));
    WB_TRY(ws.get(c, &items[1], lists));
    WB_TRY(ws.get(c, &w.wtree, lists));
    WB_TRY(ws.get(c, &w.need, lists));
    WB_TRY(ws.get(c, &rarea, (size_t)T));
    WB_TRY(ws.get(c, &pmax, (size_t)WB_STAT_GRID));
    WB_TRY(ws.get(c, &psum, (size_t)WB_STAT_GRID));
    WB_TRY(dev_alloc(c, out.nodes, sizeof(wbvh::Node) * (size_t)cap));
    w.nodes = static_cast<wbvh::Node*>(out.nodes.p);
    uint32_t n_items = 0;
    k_wb_roots_count<<<tb, WB_BLOCK, 0, sm>>>(w, cnt);
    HIPCHK(exclusive_scan(cnt, pos, (uint32_t)T, sums, sm));
    WB_TRY(total(cnt, pos, (size_t)T, &n_items));
    k_wb_roots_emit<<<tb, WB_BLOCK, 0, sm>>>(w, pos, items[0]);
    std::vector<int32_t> level_start;
    uint32_t base = 0;
    cur = 0;
    while (n_items > 0) {
        level_start.push_back((int32_t)base);
        if ((size_t)base + n_items > cap) return LUMO_ERR_INVALID;  // cannot happen: cap counts every candidate
        uint32_t next = 0;
        k_wb_open<<<blocks(n_items), WB_BLOCK, 0, sm>>>(w, items[cur], n_items, kids, n_kids, cnt);
        HIPCHK(exclusive_scan(cnt, pos, n_items, sums, sm));
        WB_TRY(total(cnt, pos, n_items, &next));
        if ((size_t)base + n_items + next > cap) return LUMO_ERR_INVALID;
        k_wb_emit<<<blocks(n_items), WB_BLOCK, 0, sm>>>(w, n_items, kids, n_kids, pos, (int32_t)base,
                                                        (int32_t)(base + n_items), items[cur ^ 1]);
        base += n_items;
        n_items = next;
        cur ^= 1;
    }
    level_start.push_back((int32_t)base);
    const int levels = (int)level_start.size() - 1;
    // 7. stack need (deepest level first, BLASes before the world trees), max_abs, SAH cost
    for (int pass = 0; pass < 2; ++pass) {
        for (int l = levels - 1; l >= 0; --l)
            k_wb_need<<<blocks((size_t)(level_start[l + 1] - level_start[l])), WB_BLOCK, 0, sm>>>(w, level_start[l],
                                                                                                 level_start[l + 1], pass);
        k_wb_rootneed<<<1, WB_BLOCK, 0, sm>>>(w, pass);
    }
    if (base > 0) {
        const int grid = std::min(blocks(base), WB_STAT_GRID);
        k_wb_rootarea<<<tb, WB_BLOCK, 0, sm>>>(w, rarea);
        k_wb_stats_partial<<<grid, WB_BLOCK, 0, sm>>>(w, (int32_t)base, rarea, pmax, psum);
        k_wb_stats_final<<<1, WB_BLOCK, 0, sm>>>(w, grid, pmax, psum);
    }
    HIPCHK(hipEventRecord(ev.b, sm));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(sm));
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b));
    if (pl.radius > 0) {
        float cms = 0.0f;
        HIPCHK(hipEventElapsedTime(&cms, ev.c, ev.d));
        TlStat ts{};
        HIPCHK(hipMemcpy(&ts, tl_stat, sizeof(ts), hipMemcpyDeviceToHost));
        out.treelet.area_before = ts.area[0];
        out.treelet.area_after = ts.area[tl_passes > 0 ? 1 : 0];
        if (tl_passes > 0) {
            float tms = 0.0f;
            HIPCHK(hipEventElapsedTime(&tms, ev.e, ev.f));
            out.treelet.passes_used = tl_passes;
            out.treelet.tried = (int64_t)ts.tried;
            out.treelet.replaced = (int64_t)ts.replaced;
            out.treelet.treelet_ms = (double)tms;
            cms -= tms;  // the passes lie between the last merge and the relabel
        }
        out.cluster.cluster_ms = (double)cms;
    }
    WbScal sc{};
    HIPCHK(hipMemcpy(&sc, w.scal, sizeof(sc), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out.root_ref.data(), w.root_ref, sizeof(int32_t) * (size_t)T, hipMemcpyDeviceToHost));
    out.n_nodes = (int)base;
    out.n_tv = (int)prep.n_tris;
    out.levels = levels;
    out.max_stack = sc.max_stack;
    out.max_abs = sc.max_abs;
    out.sah = sc.sah;
    out.ms = (double)ms;
    out.ok = sc.max_stack <= c.wb_cfg.stack_limit && base < (uint32_t)INT32_MAX / 2;
    return LUMO_OK;
}

}  // namespace dev
}  // namespace lumo

namespace {

// ---------------------------------------------------------------- refit (wbvh_refit.h)
template <typename T>
lumo_status rf_get(Ctx& c, T** p, size_t count) {
    c.scene_bufs.emplace_back();
    const lumo_status st = dev_alloc(c, c.scene_bufs.back(), sizeof(T) * std::max<size_t>(count, 1));
    *p = static_cast<T*>(c.scene_bufs.back().p);
    return st;
}

RfWork rf_work(const Ctx& c) {
    const DScene& s = c.sc;
    const Refit& r = c.rf;
    RfWork w{};
    w.n_nodes = c.w_nodes;
    w.n_recs = c.w_tris;
    w.n_lights = s.n_lights;
    w.n_objs = s.n_objs;
    w.oroot = s.w_oroot;
    w.lroot = s.w_lroot;
    w.vertices = s.vertices;
    w.tris = s.tris;
    w.objs = s.objs;
    w.lights = s.lights;
    w.xforms = s.xforms;
    w.oblas = s.w_oblas;
    w.lblas = s.w_lblas;
    w.nodes = const_cast<wbvh::Node*>(s.wnodes);
    w.wtv = const_cast<double*>(s.wtv);
    w.soup = const_cast<double*>(s.tv);
    w.parent = r.parent;
    w.kids = r.kids;
    w.arrive = r.arrive;
    w.wtree = r.wtree;
    w.box = reinterpret_cast<WbBox*>(r.box);
    w.rarea = r.rarea;
    return w;
}

// max_abs and the SAH cost of the nodes as they lie, by the builder's reductions; leaves them in scal
void rf_stats(const Ctx& c, const RfWork& w, hipStream_t sm) {
    if (w.n_nodes <= 0) return;
    WbWork b{};
    b.nodes = w.nodes;
    b.wtree = w.wtree;
    b.scal = static_cast<WbScal*>(c.rf.scal);
    const int grid = std::min(blocks((size_t)w.n_nodes), WB_STAT_GRID);
    k_rf_rootarea<<<blocks((size_t)w.n_nodes), WB_BLOCK, 0, sm>>>(w);
    k_wb_stats_partial<<<grid, WB_BLOCK, 0, sm>>>(b, w.n_nodes, w.rarea, c.rf.pmax, c.rf.psum);
    k_wb_stats_final<<<1, WB_BLOCK, 0, sm>>>(b, grid, c.rf.pmax, c.rf.psum);
}

lumo_status rf_read_scal(const Ctx& c, hipStream_t sm, WbScal* sc) {
    *sc = WbScal{};
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(sm));
    if (c.w_nodes > 0) HIPCHK(hipMemcpy(sc, c.rf.scal, sizeof(*sc), hipMemcpyDeviceToHost));
    return LUMO_OK;
}

// the first update after an upload: the workspace (72 B per node, 25 B per vertex), the protected
// vertices, the parent links and the cost of the tree as built
lumo_status rf_init(Ctx& c) {
    Refit& r = c.rf;
    const size_t nv = (size_t)c.n_vertices, nn = (size_t)c.w_nodes;
    uint32_t* prot32 = nullptr;
    WbScal* scal = nullptr;
    WB_TRY(rf_get(c, &prot32, (nv + 3) / 4));
    WB_TRY(rf_get(c, &r.vnew, 3 * nv));
    WB_TRY(rf_get(c, &r.flags, (size_t)RF_FLAGS));
    WB_TRY(rf_get(c, &r.parent, nn));
    WB_TRY(rf_get(c, &r.wtree, nn));
    WB_TRY(rf_get(c, &r.kids, nn));
    WB_TRY(rf_get(c, &r.arrive, nn));
    WB_TRY(rf_get(c, &r.box, 6 * nn));
    WB_TRY(rf_get(c, &r.rarea, nn));
    WB_TRY(rf_get(c, &r.pmax, (size_t)WB_STAT_GRID));
    WB_TRY(rf_get(c, &r.psum, (size_t)WB_STAT_GRID));
    WB_TRY(rf_get(c, &scal, 1));
    r.prot = reinterpret_cast<uint8_t*>(prot32);
    r.scal = scal;
    hipStream_t sm = c.streams[0];
    const RfWork w = rf_work(c);
    if (nv > 0) k_wb_fill<<<blocks((nv + 3) / 4), WB_BLOCK, 0, sm>>>(prot32, 0u, (uint32_t)((nv + 3) / 4));
    if (w.n_lights + w.n_objs > 0)
        k_rf_protect<<<w.n_lights + w.n_objs, WB_BLOCK, 0, sm>>>(w, c.n_vertices, c.n_triangles, r.prot);
    if (nn > 0) {
        k_wb_fill<<<blocks(nn), WB_BLOCK, 0, sm>>>(reinterpret_cast<uint32_t*>(r.parent), ~0u, (uint32_t)nn);
        k_rf_parents<<<blocks(nn), WB_BLOCK, 0, sm>>>(w);
        k_rf_trees<<<blocks(nn), WB_BLOCK, 0, sm>>>(w);
        rf_stats(c, w, sm);
    }
    WbScal sc;
    WB_TRY(rf_read_scal(c, sm, &sc));
    r.info = lumo_refit_info{};
    r.info.sah_build = sc.sah;
    r.ready = true;
    return LUMO_OK;
}

}  // namespace

extern "C" {

lumo_status lumo_scene_update_vertices(void* ctx, int32_t first, int32_t count, const double* xyz) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c || !xyz) return LUMO_ERR_INVALID;
    if (!c->has_scene) return LUMO_ERR_NO_SCENE;
    if (!c->sc.accel) return LUMO_ERR_UNSUPPORTED;
    if (first < 0 || count < 0 || (int64_t)first + count > c->n_vertices) return LUMO_ERR_INVALID;
    HIPCHK(hipSetDevice(c->device));
    if (!c->rf.ready) WB_TRY(rf_init(*c));
    Refit& r = c->rf;
    DScene& s = c->sc;
    hipStream_t sm = c->streams[0];
    Events ev;
    HIPCHK(hipEventCreate(&ev.a));
    HIPCHK(hipEventCreate(&ev.b));
    const size_t n3 = 3 * (size_t)count;
    if (count > 0) HIPCHK(hipMemcpy(r.vnew, xyz, sizeof(double) * n3, hipMemcpyHostToDevice));
    HIPCHK(hipEventRecord(ev.a, sm));
    // 1. the new values against the present ones: one read-back decides
    uint32_t flags[RF_FLAGS] = {};
    k_wb_fill<<<1, WB_BLOCK, 0, sm>>>(r.flags, 0u, (uint32_t)RF_FLAGS);
    if (count > 0) {
        k_rf_stage_vertices<<<blocks((size_t)count), WB_BLOCK, 0, sm>>>(r.vnew, s.vertices, r.prot, first, count, r.flags);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(sm));
        HIPCHK(hipMemcpy(flags, r.flags, sizeof(flags), hipMemcpyDeviceToHost));
    }
    if (flags[RF_NONFINITE]) return LUMO_ERR_INVALID;
    if (flags[RF_PROTECTED]) return LUMO_ERR_UNSUPPORTED;
    if (count > 0)
        HIPCHK(hipMemcpyAsync(const_cast<double*>(s.vertices) + 3 * (size_t)first, r.vnew, sizeof(double) * n3,
                              hipMemcpyDeviceToDevice, sm));
    // 2. records and soup  3. boxes: the BLASes, then the world trees  4. max_abs, cost, staged sets
    const RfWork w = rf_work(*c);
    if (w.n_recs > 0) k_rf_records<<<blocks((size_t)w.n_recs), WB_BLOCK, 0, sm>>>(w);
    if (w.n_nodes > 0) {
        const int grid = (w.n_nodes + RF_QUADS - 1) / RF_QUADS;
        k_wb_fill<<<blocks((size_t)w.n_nodes), WB_BLOCK, 0, sm>>>(r.arrive, 0u, (uint32_t)w.n_nodes);
        k_rf_fit<<<grid, WB_BLOCK, 0, sm>>>(w, 0);
        k_rf_fit<<<grid, WB_BLOCK, 0, sm>>>(w, 1);
        rf_stats(*c, w, sm);
    }
    auto restage = [&](const char* set, uint32_t off, const void* src, size_t bytes) {
        const size_t n16 = bytes / 16;  // rows of 80 B, nodes of 128 B
        if (n16 == 0) return;
        k_rf_copy<<<std::min(blocks(n16), WB_STAT_GRID), WB_BLOCK, 0, sm>>>(
            reinterpret_cast<uint4*>(const_cast<char*>(set) + off), static_cast<const uint4*>(src), n16);
    };
    if (s.hot_bytes > 0) {
        restage(s.hot, s.off_tv, s.tv, sizeof(double) * TV_STRIDE * (size_t)c->n_triangles);
        restage(s.hot, s.off_wnodes, s.wnodes, sizeof(wbvh::Node) * (size_t)w.n_nodes);
        restage(s.hot, s.off_wtv, s.wtv, sizeof(double) * wbvh::TV * (size_t)w.n_recs);
    }
    if (s.top_bytes > 0 && s.top_wnodes > 0)
        restage(s.top, s.off_top_wnodes, s.wnodes, sizeof(wbvh::Node) * (size_t)s.top_wnodes);
    HIPCHK(hipEventRecord(ev.b, sm));
    WbScal sc;
    WB_TRY(rf_read_scal(*c, sm, &sc));
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b));
    s.w_maxabs = (double)sc.max_abs;  // the kernels take DScene by value at every launch
    r.info.changed = (int64_t)flags[RF_CHANGED];
    r.info.updates++;
    r.info.refit_ms = (double)ms;
    r.info.sah_cost = sc.sah;
    r.info.max_abs = sc.max_abs;
    return LUMO_OK;
}

// The present vertices become the previous ones of the motion feature (device/motion.h).
lumo_status lumo_scene_motion_mark(void* ctx) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c) return LUMO_ERR_INVALID;
    if (!c->has_scene) return LUMO_ERR_NO_SCENE;
    HIPCHK(hipSetDevice(c->device));
    const size_t n = 3 * (size_t)c->n_vertices;
    if (!c->vprev) WB_TRY(rf_get(*c, &c->vprev, n));
    hipStream_t sm = c->streams[0];
    if (n > 0) k_rf_mark<<<std::min(blocks((n + 1) / 2), WB_STAT_GRID), WB_BLOCK, 0, sm>>>(c->vprev, c->sc.vertices, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(sm));
    return LUMO_OK;
}

lumo_status lumo_scene_refit_info(void* ctx, lumo_refit_info* info) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c || !info) return LUMO_ERR_INVALID;
    if (!c->has_scene) return LUMO_ERR_NO_SCENE;
    *info = c->rf.info;
    return LUMO_OK;
}

lumo_status lumo_scene_set_wide_build(void* ctx, const lumo_wide_build_cfg* cfg) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c) return LUMO_ERR_INVALID;
    const lumo_wide_build_cfg v = cfg ? *cfg : lumo_wide_build_cfg{0, 8, 64, 0};
    if (v.builder < 0 || v.builder > 1 || v.leaf_max < 1 || v.leaf_max > 8 || v.stack_limit < 1 ||
        v.stack_limit > wbvh::STACK || v.reserved != 0)
        return LUMO_ERR_INVALID;
    c->wb_cfg = v;
    return LUMO_OK;
}

lumo_status lumo_scene_wide_build_info(void* ctx, lumo_wide_build_info* info) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c || !info) return LUMO_ERR_INVALID;
    if (!c->has_scene) return LUMO_ERR_NO_SCENE;
    *info = c->wb_info;
    return LUMO_OK;
}

lumo_status lumo_scene_set_wide_cluster(void* ctx, const lumo_wide_cluster_cfg* cfg) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c) return LUMO_ERR_INVALID;
    const lumo_wide_cluster_cfg v = cfg ? *cfg : lumo_wide_cluster_cfg{};
    if (v.radius < 0 || v.radius > PL_RADIUS_MAX || v.max_iter < 0 || v.max_iter > 4096 || v.reserved[0] != 0 ||
        v.reserved[1] != 0)
        return LUMO_ERR_INVALID;
    c->wc_cfg = v;
    return LUMO_OK;
}

lumo_status lumo_scene_wide_cluster_info(void* ctx, lumo_wide_cluster_info* info) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c || !info) return LUMO_ERR_INVALID;
    if (!c->has_scene) return LUMO_ERR_NO_SCENE;
    *info = c->wc_info;
    return LUMO_OK;
}

lumo_status lumo_scene_set_wide_treelet(void* ctx, const lumo_wide_treelet_cfg* cfg) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c) return LUMO_ERR_INVALID;
    const lumo_wide_treelet_cfg v = cfg ? *cfg : lumo_wide_treelet_cfg{};
    if (v.passes < 0 || v.passes > TL_PASSES_MAX || (v.gamma != 0 && (v.gamma < TL_LEAVES || v.gamma > TL_GAMMA_MAX)) ||
        v.reserved[0] != 0 || v.reserved[1] != 0)
        return LUMO_ERR_INVALID;
    c->wt_cfg = v;
    return LUMO_OK;
}

lumo_status lumo_scene_wide_treelet_info(void* ctx, lumo_wide_treelet_info* info) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c || !info) return LUMO_ERR_INVALID;
    if (!c->has_scene) return LUMO_ERR_NO_SCENE;
    *info = c->wt_info;
    return LUMO_OK;
}

lumo_status lumo_debug_wide_export(void* ctx, int64_t* info, void* nodes, double* tv, int32_t* obj_blas,
                                   int32_t* light_blas) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c || !info) return LUMO_ERR_INVALID;
    if (!c->has_scene) return LUMO_ERR_NO_SCENE;
    HIPCHK(hipSetDevice(c->device));
    const DScene& s = c->sc;
    const bool on = s.accel != 0;
    info[0] = on;
    info[1] = on ? c->w_nodes : 0;
    info[2] = on ? c->w_tris : 0;
    info[3] = on ? c->w_stack : 0;
    info[4] = on ? c->w_depth : 0;
    info[5] = on ? s.w_oroot : wbvh::NONE;
    info[6] = on ? s.w_lroot : wbvh::NONE;
    info[7] = 0;
    if (!on) return LUMO_OK;
    if (nodes && c->w_nodes)
        HIPCHK(hipMemcpy(nodes, s.wnodes, sizeof(wbvh::Node) * (size_t)c->w_nodes, hipMemcpyDeviceToHost));
    if (tv && c->w_tris)
        HIPCHK(hipMemcpy(tv, s.wtv, sizeof(double) * wbvh::TV * (size_t)c->w_tris, hipMemcpyDeviceToHost));
    if (obj_blas && s.n_objs > 0)
        HIPCHK(hipMemcpy(obj_blas, s.w_oblas, sizeof(int32_t) * (size_t)s.n_objs, hipMemcpyDeviceToHost));
    if (light_blas && s.n_lights > 0)
        HIPCHK(hipMemcpy(light_blas, s.w_lblas, sizeof(int32_t) * (size_t)s.n_lights, hipMemcpyDeviceToHost));
    return LUMO_OK;
}

}  // extern "C"
