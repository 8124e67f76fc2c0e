// Scene upload, camera and scene information (host code only: no kernel is defined or launched
// here): the device layouts of lumo's structures (breadth-first BVHs, kd treelets, the LDS-staged
// sets), the optional wide accel, the scene's stack and feature classes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <vector>

#include "../host/wbvh.h"
#include "ctx.h"
#include "launch.h"

using namespace lumo;
using namespace lumo::dev;

extern "C" {

lumo_status lumo_scene_upload(void* ctx, const lumo_scene_desc* d) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c || !d) return LUMO_ERR_INVALID;
    if (d->num_lights <= 0 || d->num_light_nodes <= 0 || d->num_dense_spectra < 3 || !d->materials) return LUMO_ERR_INVALID;
    for (int i = 0; i < d->num_materials; ++i) {
        const lumo_material& m = d->materials[i];
        if (m.kind < LUMO_MAT_BLANK || m.kind > LUMO_MAT_MF_DIELECTRIC) return LUMO_ERR_UNSUPPORTED;
        if (m.kind >= LUMO_MAT_MF_DIFFUSE &&
            (m.eta_idx < 0 || m.eta_idx >= d->num_dense_spectra || m.k_idx < 0 || m.k_idx >= d->num_dense_spectra ||
             !(m.roughness > 0.0 && m.roughness <= 1.0)))
            return LUMO_ERR_INVALID;
        if (m.kind == LUMO_MAT_LIGHT && (m.illuminant < 0 || m.illuminant >= d->num_dense_spectra))
            return LUMO_ERR_INVALID;
        for (int t : {m.albedo_tex, m.ks_tex, m.tf_tex})
            if (t < -1 || t >= d->num_textures) return LUMO_ERR_INVALID;
        if (m.normal_map < -1 || m.normal_map >= d->num_normal_maps) return LUMO_ERR_INVALID;
    }
    // texture tables (texture.rs): checkerboard children precede their parent, so sampling ends
    for (int i = 0; i < d->num_textures; ++i) {
        const lumo_texture& t = d->textures[i];
        const bool ok = t.kind == LUMO_TEX_SOLID || t.kind == LUMO_TEX_MANDELBROT ||
                        (t.kind == LUMO_TEX_IMAGE && t.width > 0 && t.height > 0 && t.first >= 0 &&
                         (int64_t)t.first + (int64_t)t.width * t.height <= d->num_texels) ||
                        (t.kind == LUMO_TEX_CHECKERBOARD && t.first >= 0 && t.first < i && t.second >= 0 && t.second < i) ||
                        (t.kind == LUMO_TEX_MARBLE && t.first >= 0 && t.first < d->num_perlin);
        if (!ok) return LUMO_ERR_INVALID;
    }
    for (int i = 0; i < d->num_normal_maps; ++i) {
        const lumo_normal_map& n = d->normal_maps[i];
        if (!(n.width > 0 && n.height > 0 && n.first >= 0 &&
              (int64_t)n.first + (int64_t)n.width * n.height <= d->num_normal_texels))
            return LUMO_ERR_INVALID;
    }
    for (int i = 0; i < d->num_lights + d->num_objects; ++i) {
        const lumo_object& o = i < d->num_lights ? d->lights[i] : d->objects[i - d->num_lights];
        if (o.type < LUMO_OBJ_KDMESH || o.type > LUMO_OBJ_SPHERE) return LUMO_ERR_UNSUPPORTED;
        if (o.type == LUMO_OBJ_SPHERE && !(o.radius != 0.0 && o.area > 0.0)) return LUMO_ERR_INVALID;
        if (o.xform >= d->num_transforms || (o.xform >= 0 && !d->transforms)) return LUMO_ERR_INVALID;
        if (o.type == LUMO_OBJ_TRIANGLE && (o.tri_base < 0 || o.tri_base >= d->num_triangles)) return LUMO_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(c->device));
    free_scene(*c);
    DScene& s = c->sc;
    lumo_status st = LUMO_OK;
    auto chk = [&](lumo_status x) {
        if (x && !st) st = x;
    };
    chk(upload(*c, d->vertices, (size_t)3 * d->num_vertices, &s.vertices));
    c->sort_lo = V3{0.0, 0.0, 0.0};  // no world box: every origin in cell 0 (the octant still sorts)
    c->sort_scale = V3{0.0, 0.0, 0.0};
    if (d->num_object_nodes > 0 && d->object_nodes) {  // ray sorting's cells: the objects BVH's world box
        const lumo_bvh_node& r = d->object_nodes[0];
        double lo[3], sc3[3];
        for (int a = 0; a < 3; ++a) {
            lo[a] = r.bmin[a];
            const double ext = r.bmax[a] - r.bmin[a];
            sc3[a] = ext > 0.0 && std::isfinite(ext) ? 8.0 / ext : 0.0;  // 8 cells per axis (scan.h rs_key)
        }
        c->sort_lo = V3{lo[0], lo[1], lo[2]};
        c->sort_scale = V3{sc3[0], sc3[1], sc3[2]};
    }
    chk(upload(*c, d->normals, (size_t)3 * d->num_normals, &s.normals));
    chk(upload(*c, d->uvs, (size_t)2 * d->num_uvs, &s.uvs));
    chk(upload(*c, d->triangles, (size_t)d->num_triangles, &s.tris));
    chk(upload(*c, d->kd_nodes, (size_t)d->num_kd_nodes, &s.kd));
    chk(upload(*c, d->kd_items, (size_t)d->num_kd_items, &s.kd_items));
    // device BVHs (DBvh, dscene.h): right child -> escape index (lumo's preorder successor of the
    // subtree), left child explicit, nodes stored breadth-first so the top levels are a prefix.
    // A leaf of exactly one un-instanced kd mesh / rectangle whose kd boundary is bitwise the
    // node's box gets BVH_SAME_BOX in its count: the walk tests that box once (bvh_traverse).
    bool bvh_ok = true;
    auto escapes = [&](const lumo_bvh_node* nodes, int n, const int32_t* items, int n_items, const lumo_object* objs,
                       int n_objs, std::vector<DBvh>& out) {
        out.assign(n > 0 ? n : 0, DBvh{});
        if (n <= 0) return;
        std::vector<int32_t> esc(n, -1);
        for (int i = 0; i < n; ++i) {  // parents precede children (preorder)
            const lumo_bvh_node& b = nodes[i];
            if (b.count == 0) {
                if (i + 1 >= n || (b.right >= n)) {
                    bvh_ok = false;
                    return;
                }
                esc[i + 1] = b.right >= 0 ? b.right : esc[i];
                if (b.right >= 0) esc[b.right] = esc[i];
            }
        }
        std::vector<int32_t> order, at(n, -1);  // breadth-first order; at[old] = new index
        order.reserve(n);
        order.push_back(0);
        at[0] = 0;
        for (size_t h = 0; h < order.size(); ++h) {
            const int i = order[h];
            if (nodes[i].count != 0) continue;
            for (const int ch : {i + 1, nodes[i].right}) {
                if (ch < 0) continue;
                if (at[ch] >= 0) {  // not a tree
                    bvh_ok = false;
                    return;
                }
                at[ch] = (int32_t)order.size();
                order.push_back(ch);
            }
        }
        if ((int)order.size() != n) {  // unreachable nodes: not lumo's layout
            bvh_ok = false;
            return;
        }
        for (int k = 0; k < n; ++k) {
            const int i = order[k];
            DBvh& o = out[k];
            for (int a = 0; a < 3; ++a) {
                o.bmin[a] = nodes[i].bmin[a];
                o.bmax[a] = nodes[i].bmax[a];
            }
            o.escape = esc[i] >= 0 ? at[esc[i]] : -1;
            o.left = nodes[i].count == 0 ? at[i + 1] : -1;
            o.first = nodes[i].first;
            o.count = nodes[i].count;
            if (o.count == 1 && o.first >= 0 && o.first < n_items && items[o.first] >= 0 && items[o.first] < n_objs) {
                const lumo_object& ob = objs[items[o.first]];
                if ((ob.type == LUMO_OBJ_KDMESH || ob.type == LUMO_OBJ_RECTANGLE) && ob.xform < 0 &&
                    std::memcmp(ob.bmin, o.bmin, sizeof(o.bmin)) == 0 && std::memcmp(ob.bmax, o.bmax, sizeof(o.bmax)) == 0)
                    o.count |= BVH_SAME_BOX;
            }
        }
    };
    std::vector<DBvh> obvh, lbvh;
    escapes(d->object_nodes, d->num_object_nodes, d->object_items, d->num_object_items, d->objects, d->num_objects, obvh);
    escapes(d->light_nodes, d->num_light_nodes, d->light_items, d->num_light_items, d->lights, d->num_lights, lbvh);
    if (!bvh_ok) {
        free_scene(*c);
        return LUMO_ERR_INVALID;
    }
    chk(upload(*c, obvh.data(), obvh.size(), &s.onodes));
    chk(upload(*c, d->object_items, (size_t)d->num_object_items, &s.oitems));
    chk(upload(*c, lbvh.data(), lbvh.size(), &s.lnodes));
    chk(upload(*c, d->light_items, (size_t)d->num_light_items, &s.litems));
    chk(upload(*c, d->alias_prob, (size_t)d->num_lights, &s.alias_prob));
    chk(upload(*c, d->alias_idx, (size_t)d->num_lights, &s.alias_idx));
    chk(upload(*c, d->alias_pdf, (size_t)d->num_lights, &s.alias_pdf));
    chk(upload(*c, d->materials, (size_t)d->num_materials, &s.mats));
    chk(upload(*c, d->dense_spectra, (size_t)95 * d->num_dense_spectra, &s.dense));
    chk(upload(*c, d->transforms, (size_t)d->num_transforms, &s.xforms));
    chk(upload(*c, d->textures, (size_t)d->num_textures, &s.textures));
    chk(upload(*c, d->texels, (size_t)d->num_texels, &s.texels));
    chk(upload(*c, d->normal_maps, (size_t)d->num_normal_maps, &s.nmaps));
    chk(upload(*c, d->normal_texels, (size_t)3 * d->num_normal_texels, &s.ntexels));
    chk(upload(*c, d->perlin, (size_t)d->num_perlin, &s.perlin));
    // device-only layouts: triangle vertex soup and 16-B kd nodes
    std::vector<double> tv((size_t)TV_STRIDE * d->num_triangles, 0.0);
    for (int i = 0; i < d->num_triangles; ++i)
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) tv[(size_t)TV_STRIDE * i + 3 * k + a] = d->vertices[3 * d->triangles[i].v[k] + a];
    // kd trees in cache-line treelets: each tree (from each distinct kd_root) is cut into groups of
    // up to 8 nodes (128 B) taken breadth-first from a group root, so a node's children and
    // grandchildren are usually in the line the node itself came in; trees under 8 nodes are
    // packed without alignment.  Children are stored as explicit indices (DKd::left).
    std::vector<int32_t> kd_new(d->num_kd_nodes, -1);
    std::vector<DKd> kdp;
    std::vector<std::pair<size_t, size_t>> kd_trees;  // [first, end) of each tree's treelets in kdp
    {
        std::vector<int32_t> order;  // old indices in new order (-1: padding)
        auto kid = [&](int i, int which) { return which == 0 ? i + 1 : d->kd_nodes[i].right; };
        auto valid = [&](int i) { return i >= 0 && i < d->num_kd_nodes; };
        auto place_tree = [&](int root) {
            if (!valid(root) || kd_new[root] >= 0) return;
            struct Extent {
                std::vector<std::pair<size_t, size_t>>& v;
                std::vector<int32_t>& o;
                size_t lo;
                ~Extent() { v.emplace_back(lo, o.size()); }
            } extent{kd_trees, order, order.size()};
            int size = 0;  // nodes of the tree (bounded walk)
            {
                std::vector<int32_t> st{root};
                while (!st.empty() && size <= 8) {
                    const int i = st.back();
                    st.pop_back();
                    size++;
                    if (!d->kd_nodes[i].leaf) {
                        for (int w = 0; w < 2; ++w)
                            if (valid(kid(i, w))) st.push_back(kid(i, w));
                    }
                }
            }
            std::deque<int32_t> groups{root};
            while (!groups.empty()) {
                const int g = groups.front();
                groups.pop_front();
                if (size > 8)
                    while (order.size() % 8) order.push_back(-1);  // start a 128-B line
                std::deque<int32_t> bfs{g};
                int used = 0;
                while (!bfs.empty()) {
                    const int i = bfs.front();
                    bfs.pop_front();
                    if (used == 8) {
                        groups.push_back(i);
                        continue;
                    }
                    kd_new[i] = (int32_t)order.size();
                    order.push_back(i);
                    used++;
                    if (!d->kd_nodes[i].leaf)
                        for (int w = 0; w < 2; ++w)
                            if (valid(kid(i, w)) && kd_new[kid(i, w)] < 0) bfs.push_back(kid(i, w));
                }
            }
        };
        for (int i = 0; i < d->num_objects; ++i)
            if (d->objects[i].type == LUMO_OBJ_KDMESH || d->objects[i].type == LUMO_OBJ_RECTANGLE) place_tree(d->objects[i].kd_root);
        for (int i = 0; i < d->num_lights; ++i)
            if (d->lights[i].type == LUMO_OBJ_KDMESH || d->lights[i].type == LUMO_OBJ_RECTANGLE) place_tree(d->lights[i].kd_root);
        kdp.assign(order.size(), DKd{});
        for (size_t j = 0; j < order.size(); ++j) {
            const int i = order[j];
            if (i < 0) continue;
            const lumo_kd_node& n = d->kd_nodes[i];
            DKd k{};
            if (n.leaf) {
                k.u.leaf.first = n.first;
                k.u.leaf.count = n.count;
                k.meta = 3;
                k.left = -1;
            } else {
                if (!valid(n.right) || !valid(i + 1) || n.axis < 0 || n.axis > 2 || kd_new[n.right] >= (1 << 29))
                    chk(LUMO_ERR_INVALID);
                k.u.point = n.point;
                k.meta = (kd_new[n.right] << 2) | n.axis;
                k.left = kd_new[i + 1];
            }
            kdp[j] = k;
        }
    }
    auto relaid = [&](const lumo_object* src, int n) {  // objects / lights with their new kd roots
        std::vector<lumo_object> v(src, src + n);
        for (lumo_object& o : v)
            if ((o.type == LUMO_OBJ_KDMESH || o.type == LUMO_OBJ_RECTANGLE) && o.kd_root >= 0 &&
                o.kd_root < d->num_kd_nodes)
                o.kd_root = kd_new[o.kd_root];
        return v;
    };
    const std::vector<lumo_object> objs_dev = relaid(d->objects, d->num_objects);
    const std::vector<lumo_object> lights_dev = relaid(d->lights, d->num_lights);
    auto trav_view = [](const std::vector<lumo_object>& v) {  // DObj (dscene.h): what the walks read
        std::vector<DObj> t(v.size());
        for (size_t i = 0; i < v.size(); ++i) {
            const lumo_object& o = v[i];
            DObj& x = t[i];
            for (int a = 0; a < 3; ++a) {
                x.bmin[a] = o.bmin[a];
                x.bmax[a] = o.bmax[a];
            }
            if (o.type == LUMO_OBJ_SPHERE) x.bmin[0] = o.radius;
            x.kd_root = o.kd_root;
            x.tri_base = o.tri_base;
            x.item_base = o.item_base;
            x.tx = ((o.xform + 1) << 2) | o.type;
        }
        return t;
    };
    const std::vector<DObj> tobjs = trav_view(objs_dev), tlights = trav_view(lights_dev);
    chk(upload(*c, objs_dev.data(), objs_dev.size(), &s.objs));
    chk(upload(*c, lights_dev.data(), lights_dev.size(), &s.lights));
    chk(upload(*c, tobjs.data(), tobjs.size(), &s.tobjs));
    chk(upload(*c, tlights.data(), tlights.size(), &s.tlights));
    chk(upload(*c, tv.data(), tv.size(), &s.tv));
    chk(upload(*c, kdp.data(), kdp.size(), &s.kdp));
    // wide accel (LUMO_OPT_ACCEL = 1, wbvh.h): built from the scene description.  The sampled light's
    // own hit keeps lumo's kd walk with a WL_STK-entry stack, so every light's kd tree must fit it;
    // a scene the build refuses keeps lumo's structures (lumo_scene_info.accel = 0).
    wbvh::Accel acc;
    s.accel = 0;
    s.w_oroot = s.w_lroot = wbvh::NONE;
    s.wnodes = s.wnodes_lds = nullptr;
    s.wtv = nullptr;
    s.w_oblas = s.w_lblas = nullptr;
    s.wn_lds = s.top_wnodes = 0;
    s.w_maxabs = 0.0;
    s.off_top_wnodes = 0;
    s.off_wnodes = s.off_wtv = s.off_woblas = s.off_wlblas = 0;
    c->w_nodes = c->w_tris = c->w_stack = c->w_depth = 0;
    if (c->o.accel && !st) {
        acc = wbvh::build_accel(*d);  // refuses light kd trees deeper than WL_STK
        if (acc.ok) {
            s.accel = 1;
            s.w_oroot = acc.obj_root;
            s.w_lroot = acc.light_root;
            s.w_maxabs = (double)acc.max_abs;
            chk(upload(*c, acc.nodes.data(), acc.nodes.size(), &s.wnodes));
            chk(upload(*c, acc.tv.data(), acc.tv.size(), &s.wtv));
            chk(upload(*c, acc.obj_blas.data(), acc.obj_blas.size(), &s.w_oblas));
            chk(upload(*c, acc.light_blas.data(), acc.light_blas.size(), &s.w_lblas));
            c->w_nodes = (int)acc.nodes.size();
            c->w_tris = (int)(acc.tv.size() / wbvh::TV);
            c->w_stack = acc.max_stack;
            c->w_depth = acc.depth;
        } else {
            fprintf(stderr, "lumo_amd: the wide accel refused this scene (a light kd tree deeper than %d or a "
                    "walk stack of %d); walking lumo's structures\n", WL_STK, acc.max_stack);
        }
    }
    if (st) {
        free_scene(*c);
        return st;
    }
    s.n_onodes = d->num_object_nodes;
    s.n_lnodes = d->num_light_nodes;
    s.n_lights = d->num_lights;
    s.n_objs = d->num_objects;
    {   // packed traversal set for LDS staging (scenes up to 48 KiB)
        std::vector<char> hot;
        auto put = [&](const void* p, size_t bytes) -> uint32_t {
            const size_t off = (hot.size() + 15) & ~(size_t)15;
            hot.resize(off + ((bytes + 15) & ~(size_t)15), 0);
            if (bytes) std::memcpy(hot.data() + off, p, bytes);
            return (uint32_t)off;
        };
        s.off_onodes = put(obvh.data(), sizeof(DBvh) * obvh.size());
        s.off_oitems = put(d->object_items, sizeof(int32_t) * d->num_object_items);
        s.off_lnodes = put(lbvh.data(), sizeof(DBvh) * lbvh.size());
        s.off_litems = put(d->light_items, sizeof(int32_t) * d->num_light_items);
        s.off_objs = put(objs_dev.data(), sizeof(lumo_object) * objs_dev.size());
        s.off_lights = put(lights_dev.data(), sizeof(lumo_object) * lights_dev.size());
        s.off_kdp = put(kdp.data(), sizeof(DKd) * kdp.size());
        s.off_kd_items = put(d->kd_items, sizeof(int32_t) * d->num_kd_items);
        s.off_tris = put(d->triangles, sizeof(lumo_triangle) * d->num_triangles);
        s.off_tv = put(tv.data(), sizeof(double) * tv.size());
        s.off_xforms = put(d->transforms, sizeof(lumo_transform) * d->num_transforms);
        s.off_tobjs = put(tobjs.data(), sizeof(DObj) * tobjs.size());
        s.off_tlights = put(tlights.data(), sizeof(DObj) * tlights.size());
        if (s.accel) {
            s.off_wnodes = put(acc.nodes.data(), sizeof(wbvh::Node) * acc.nodes.size());
            s.off_wtv = put(acc.tv.data(), sizeof(double) * acc.tv.size());
            s.off_woblas = put(acc.obj_blas.data(), sizeof(int32_t) * acc.obj_blas.size());
            s.off_wlblas = put(acc.light_blas.data(), sizeof(int32_t) * acc.light_blas.size());
        }
        s.hot_bytes = 0;
        if (hot.size() <= 48 * 1024) {
            const char* dp = nullptr;
            chk(upload(*c, hot.data(), hot.size(), &dp));
            if (st) {
                free_scene(*c);
                return st;
            }
            s.hot = dp;
            s.hot_bytes = (uint32_t)hot.size();
        }
    }
    {   // TOP set for larger scenes (DScene::top): the object items and traversal records, the
        // objects BVH and as much of the lights BVH as fits, both breadth-first prefixes
        s.top = nullptr;
        s.top_bytes = 0;
        s.top_onodes = s.top_lnodes = 0;
        s.onodes_lds = s.lnodes_lds = nullptr;
        s.n_onodes_lds = s.n_lnodes_lds = 0;
        const size_t cap = std::min((size_t)c->o.top_kb * 1024, c->lds_cu);
        const size_t budget = cap > 256 ? cap - 256 : 0;  // 256 B: the kernels' static LDS
        const size_t objs_b = ((sizeof(int32_t) * d->num_object_items + 15) & ~(size_t)15) + sizeof(DObj) * tobjs.size();
        const size_t wobjs_b = ((sizeof(DObj) * tobjs.size() + 15) & ~(size_t)15);
        if (s.accel && s.hot_bytes == 0 && budget >= 4096 && wobjs_b + 16 * sizeof(wbvh::Node) <= budget) {
            // wide accel: the object records (object leaves) and a breadth-first prefix of the nodes
            // (the top levels of every tree, wbvh_build.h); no kd stack or treelets (the light's own
            // kd walk reads HBM)
            std::vector<char> top;
            auto put = [&](const void* p, size_t bytes) -> uint32_t {
                const size_t off = (top.size() + 15) & ~(size_t)15;
                top.resize(off + ((bytes + 15) & ~(size_t)15), 0);
                if (bytes) std::memcpy(top.data() + off, p, bytes);
                return (uint32_t)off;
            };
            s.off_top_oitems = 0;
            s.off_top_tobjs = put(tobjs.data(), sizeof(DObj) * tobjs.size());
            const size_t left = budget - top.size();
            const size_t nw = std::min(acc.nodes.size(), left / sizeof(wbvh::Node));
            s.off_top_wnodes = put(acc.nodes.data(), sizeof(wbvh::Node) * nw);
            s.top_wnodes = (int32_t)nw;
            s.top_onodes = s.top_lnodes = 0;
            s.off_top_onodes = s.off_top_lnodes = 0;
            s.kst_cfg = 0;
            s.top_kd_lo = s.top_kd_n = 0;
            s.off_top_kd = 0;
            const char* dp = nullptr;
            chk(upload(*c, top.data(), top.size(), &dp));
            if (st) {
                free_scene(*c);
                return st;
            }
            s.top = dp;
            s.top_bytes = (uint32_t)top.size();
        } else if (!s.accel && s.hot_bytes == 0 && budget >= 4096 && objs_b + 64 * sizeof(DBvh) <= budget) {
            std::vector<char> top;
            auto put = [&](const void* p, size_t bytes) -> uint32_t {
                const size_t off = (top.size() + 15) & ~(size_t)15;
                top.resize(off + ((bytes + 15) & ~(size_t)15), 0);
                if (bytes) std::memcpy(top.data() + off, p, bytes);
                return (uint32_t)off;
            };
            s.off_top_oitems = put(d->object_items, sizeof(int32_t) * d->num_object_items);
            s.off_top_tobjs = put(tobjs.data(), sizeof(DObj) * tobjs.size());
            size_t left = budget - top.size();
            const size_t no = std::min(obvh.size(), left / sizeof(DBvh));
            s.off_top_onodes = put(obvh.data(), sizeof(DBvh) * no);
            left = budget - top.size();
            const size_t nl = std::min(lbvh.size(), left / sizeof(DBvh));
            s.off_top_lnodes = put(lbvh.data(), sizeof(DBvh) * nl);
            s.top_onodes = (int32_t)no;
            s.top_lnodes = (int32_t)nl;
            // kd stack entries per thread in LDS after the TOP set (TOP_BLOCK threads, 12 B each),
            // within the same budget (LUMO_OPT_TOP_KB caps the TOP kernels' whole LDS use)
            const size_t aligned = (top.size() + 15) & ~(size_t)15;
            const size_t lim = std::min(cap, c->lds_block);
            size_t room = lim > aligned + 256 ? lim - aligned - 256 : 0;
            s.kst_cfg = c->o.kd_lds > 0 ? (int32_t)std::min<size_t>((size_t)c->o.kd_lds, room / (12 * (size_t)TOP_BLOCK)) : 0;
            room -= 12 * (size_t)TOP_BLOCK * s.kst_cfg;
            // then, in what is left, the first treelets of the largest kd tree (its top levels: the
            // trees are laid out breadth-first by 128-B treelet, so they are a prefix of its range)
            s.top_kd_lo = s.top_kd_n = 0;
            s.off_top_kd = 0;
            size_t big = 0, big_lo = 0;
            for (const auto& tr : kd_trees)
                if (tr.second - tr.first > big) {
                    big = tr.second - tr.first;
                    big_lo = tr.first;
                }
            if (c->o.top_kd && big > 8 && room >= 16 * 64 + 16) {
                const size_t nk = std::min(big, (room - 16) / sizeof(DKd));
                s.off_top_kd = put(kdp.data() + big_lo, sizeof(DKd) * nk);
                s.top_kd_lo = (int32_t)big_lo;
                s.top_kd_n = (int32_t)nk;
            }
            const char* dp = nullptr;
            chk(upload(*c, top.data(), top.size(), &dp));
            if (st) {
                free_scene(*c);
                return st;
            }
            s.top = dp;
            s.top_bytes = (uint32_t)top.size();
        } else {
            s.kst_cfg = 0;
            s.top_kd_lo = s.top_kd_n = 0;
            s.off_top_kd = 0;
        }
        s.kst_n = 0;
        s.top_shm = ((s.top_bytes + 15u) & ~15u) + (uint32_t)(12 * (size_t)TOP_BLOCK * s.kst_cfg);
    }
    int n = d->num_lights, lg = 0;
    while (n > 1) {
        n >>= 1;
        lg++;
    }
    s.n_shadow = lg > 1 ? lg : 1;  // scene.rs:90-92
    // deepest pending-stack use: BVH (right children pending on a root-leaf path) and kd trees
    auto bvh_need = [&](const lumo_bvh_node* nodes, int n) {
        std::vector<int> pend(n > 0 ? n : 1, 0);
        int mx = 0;
        for (int i = 0; i < n; ++i) {  // parents precede children in lumo's layout
            if (nodes[i].count == 0) {
                const int p = pend[i] + (nodes[i].right >= 0 ? 1 : 0);
                if (i + 1 < n) pend[i + 1] = std::max(pend[i + 1], p);
                if (nodes[i].right >= 0 && nodes[i].right < n) pend[nodes[i].right] = std::max(pend[nodes[i].right], pend[i]);
                mx = std::max(mx, p);
            }
        }
        return mx;
    };
    const int need_b = std::max({1, bvh_need(d->object_nodes, d->num_object_nodes),
                                 bvh_need(d->light_nodes, d->num_light_nodes)});
    int need_k = 1;
    {
        std::vector<int> depth(d->num_kd_nodes > 0 ? d->num_kd_nodes : 1, 0);
        for (int i = 0; i < d->num_kd_nodes; ++i) {
            if (!d->kd_nodes[i].leaf) {
                if (i + 1 < d->num_kd_nodes) depth[i + 1] = std::max(depth[i + 1], depth[i] + 1);
                const int r = d->kd_nodes[i].right;
                if (r >= 0 && r < d->num_kd_nodes) depth[r] = std::max(depth[r], depth[i] + 1);
                need_k = std::max(need_k, depth[i] + 1);
            }
        }
    }
    if (need_b > 64 || need_k > 64) {
        free_scene(*c);
        return LUMO_ERR_UNSUPPORTED;  // lumo's fixed [_; 64] stacks would overflow too
    }
    auto fits = [&](int cls) { return cls >= need_k; };
    s.stack_class = 64;
    for (int cls : STACK_CLASSES)
        if (fits(cls)) {
            s.stack_class = cls;
            break;
        }
    if (c->o.stack_class > 0 && fits(c->o.stack_class)) s.stack_class = c->o.stack_class;  // A/B override
    if (s.accel) s.stack_class = 0;  // the wide walks (by_stack_class)
    // feature class: the lean kernels cover kd meshes / rectangles with Lambertian + Light only
    bool full = d->num_transforms > 0;
    for (int i = 0; i < d->num_materials; ++i)
        full = full || (d->materials[i].kind != LUMO_MAT_LAMBERTIAN && d->materials[i].kind != LUMO_MAT_LIGHT &&
                        d->materials[i].kind != LUMO_MAT_BLANK);
    for (int i = 0; i < d->num_objects; ++i)
        full = full || (d->objects[i].type != LUMO_OBJ_KDMESH && d->objects[i].type != LUMO_OBJ_RECTANGLE);
    for (int i = 0; i < d->num_lights; ++i) full = full || d->lights[i].type != LUMO_OBJ_RECTANGLE;
    bool textured = false;  // textures and bump maps: feature class 2 (the only kernels that sample them)
    for (int i = 0; i < d->num_materials; ++i) {
        const lumo_material& m = d->materials[i];
        textured = textured || m.albedo_tex >= 0 || m.ks_tex >= 0 || m.tf_tex >= 0 || m.normal_map >= 0;
    }
    full = full || c->o.full_kernels != 0;  // A/B switch
    s.full = textured ? 2 : (full ? 1 : 0);
    c->has_scene = true;
    return LUMO_OK;
}

lumo_status lumo_camera_set(void* ctx, const lumo_camera_desc* d) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c || !d) return LUMO_ERR_INVALID;
    if (d->orthographic != 0 && d->orthographic != 1) return LUMO_ERR_INVALID;
    if (d->width <= 0 || d->height <= 0 || !(d->filter_radius > 0.0) || !(d->filter_sigma > 0.0)) return LUMO_ERR_INVALID;
    // 3x3 gather footprint; refused before anything is written, so the context keeps its camera
    if (!(d->filter_radius < 1e9) || (uint64_t)std::ceil(d->filter_radius - 0.5) != 1) return LUMO_ERR_UNSUPPORTED;
    auto get = [](const double (&a)[2][16]) {
        Xform x;
        M4* ms[2] = {&x.m, &x.inv};
        for (int q = 0; q < 2; ++q) {
            V4* rows[4] = {&ms[q]->y0, &ms[q]->y1, &ms[q]->y2, &ms[q]->y3};
            for (int r = 0; r < 4; ++r) *rows[r] = V4{a[q][4 * r], a[q][4 * r + 1], a[q][4 * r + 2], a[q][4 * r + 3]};
        }
        return x;
    };
    auto m3 = [](const double* a) { return M3{V3{a[0], a[1], a[2]}, V3{a[3], a[4], a[5]}, V3{a[6], a[7], a[8]}}; };
    c->cam.wtc = get(d->world_to_camera);
    c->cam.sctr = get(d->screen_to_raster);
    c->cam.cts = get(d->camera_to_screen);
    c->cam.lens_radius = d->lens_radius;
    c->cam.focal_length = d->focal_length;
    c->cam.wb = m3(d->white_balance);
    c->cam.x2r = m3(d->xyz_to_rgb);
    c->cam.fr = d->filter_radius;
    c->cam.fsig = d->filter_sigma;
    c->cam.width = (double)d->width;
    c->cam.height = (double)d->height;
    c->cam.orthographic = d->orthographic;
    {   // CameraConfig::new (camera.rs:47-76): image plane area at z = 1
        const DCam& k = c->cam;
        V3 p_min3 = xf_pt_inv(k.sctr, V3{0.0, 0.0, 0.0});
        V3 p_max3 = xf_pt_inv(k.sctr, V3{k.width, k.height, 0.0});
        p_min3 = xf_pt_inv(k.cts, p_min3);
        p_max3 = xf_pt_inv(k.cts, p_max3);
        const V2 p_min = V2{p_min3.x, p_min3.y} / (p_min3.z == 0.0 ? 1.0 : p_min3.z);
        const V2 p_max = V2{p_max3.x, p_max3.y} / (p_max3.z == 0.0 ? 1.0 : p_max3.z);
        const V2 pd = p_max - p_min;
        c->cam.image_plane_area = fabs(pd.x * pd.y);
    }
    c->has_camera = true;
    return LUMO_OK;
}

lumo_status lumo_scene_info(void* ctx, lumo_scene_info_t* info) {
    Ctx* c = static_cast<Ctx*>(ctx);
    if (!c || !info) return LUMO_ERR_INVALID;
    if (!c->has_scene) return LUMO_ERR_NO_SCENE;
    info->stack_class = c->sc.stack_class;
    info->lds_bytes = c->o.lds ? (int32_t)c->sc.hot_bytes : 0;
    info->full_kernels = c->sc.full;
    info->n_shadow = c->sc.n_shadow;
    const bool top = c->o.top && c->sc.top_bytes > 0 && !(c->o.lds && c->sc.hot_bytes > 0);
    info->top_bytes = top ? (int32_t)c->sc.top_bytes : 0;
    info->top_object_nodes = c->sc.top_onodes;
    info->top_light_nodes = c->sc.top_lnodes;
    info->top_kd_nodes = top ? c->sc.top_kd_n : 0;
    info->top_shm = top ? (int32_t)c->sc.top_shm : 0;
    info->accel = c->sc.accel;
    info->wide_nodes = c->w_nodes;
    info->wide_tris = c->w_tris;
    info->wide_stack = c->w_stack;
    info->wide_depth = c->w_depth;
    info->top_wide_nodes = top ? c->sc.top_wnodes : 0;
    return LUMO_OK;
}

}  // extern "C"
