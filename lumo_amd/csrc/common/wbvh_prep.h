// Host side of the device builder of the wide BVH (device/wbvh_dev.hip), beside
// wbvh::build (wbvh_build.h, which stays as it is: the oracle includes it):
// * prepare(): the O(objects) part of a build.  Per tree (world objects, world lights, one BLAS per
//   distinct (tri_base, count)) the list of primitive segments, either a run of triangles of one
//   object or one object leaf (a sphere, an instance) with its f64 world box by build's own rules
//   (xf_box, |radius|); and build's refusal of light kd trees deeper than LIGHT_KD_STACK.
// * sah_cost(): the SAH cost of a finished wide tree, the figure both builders report.
// Include after wbvh_build.h (host/wbvh.cpp does).
#pragma once
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "wbvh_build.h"
#include "wbvh_dev_prep.h"

namespace lumo {
namespace wbvh {
namespace {

inline DevPrep prepare(const lumo_scene_desc& d) {
    DevPrep p;
    for (int i = 0; i < d.num_lights; ++i) {  // as build: the deepest kd path of a light's tree
        const lumo_object& o = d.lights[i];
        if (!(o.type == LUMO_OBJ_KDMESH || o.type == LUMO_OBJ_RECTANGLE) || o.kd_root < 0) continue;
        std::vector<std::pair<int, int>> stk{{o.kd_root, 1}};
        while (!stk.empty()) {
            const std::pair<int, int> e = stk.back();
            stk.pop_back();
            if (e.first < 0 || e.first >= d.num_kd_nodes) continue;
            if (e.second > LIGHT_KD_STACK) return p;  // ok = false
            if (!d.kd_nodes[e.first].leaf) {
                stk.push_back({e.first + 1, e.second + 1});
                stk.push_back({d.kd_nodes[e.first].right, e.second + 1});
            }
        }
    }
    struct Blas {
        double lo[3], hi[3];  // exact f64 bounds of the mesh's vertices
    };
    std::vector<std::vector<DevSeg>> trees(2);  // segments with `first` relative to their tree
    std::vector<int64_t> size(2, 0);
    std::vector<Blas> blas;  // of tree 2 + k
    std::map<std::pair<int32_t, int32_t>, int> blas_of;
    auto add_space = [&](const lumo_object* objs, int n, int space) {
        for (int i = 0; i < n; ++i) {
            const lumo_object& o = objs[i];
            if (o.xform < 0 && is_mesh(o)) {
                const int nt = mesh_tris(o);
                if (nt <= 0) continue;
                trees[space].push_back(DevSeg{(int32_t)size[space], o.tri_base, nt, i});
                size[space] += nt;
                continue;
            }
            if (o.type != LUMO_OBJ_SPHERE && mesh_tris(o) <= 0) continue;  // an instance of no triangles
            double llo[3], lhi[3], wlo[3], whi[3];
            if (o.type == LUMO_OBJ_SPHERE) {
                const double r = std::fabs(o.radius);
                for (int a = 0; a < 3; ++a) {
                    llo[a] = -r;
                    lhi[a] = r;
                }
            } else {
                const std::pair<int32_t, int32_t> key{o.tri_base, mesh_tris(o)};
                auto it = blas_of.find(key);
                int t;
                if (it == blas_of.end()) {
                    t = (int)trees.size();
                    trees.emplace_back();
                    trees.back().push_back(DevSeg{0, key.first, key.second, -1});
                    size.push_back(key.second);
                    Blas b;
                    Prim q;
                    for (int a = 0; a < 3; ++a) {
                        b.lo[a] = HUGE_VAL;
                        b.hi[a] = -HUGE_VAL;
                    }
                    for (int k = 0; k < key.second; ++k) {
                        tri_box(d, key.first + k, q);
                        grow(b.lo, b.hi, q.lo, q.hi);
                    }
                    blas.push_back(b);
                    blas_of[key] = t;
                } else {
                    t = it->second;
                }
                p.inst_tree.push_back({space * (1 << 30) + i, t});
                for (int a = 0; a < 3; ++a) {
                    llo[a] = blas[t - 2].lo[a];
                    lhi[a] = blas[t - 2].hi[a];
                }
            }
            if (o.xform >= 0) {
                xf_box(d.transforms[o.xform], llo, lhi, wlo, whi);
            } else {
                for (int a = 0; a < 3; ++a) {
                    wlo[a] = llo[a];
                    whi[a] = lhi[a];
                }
            }
            trees[space].push_back(DevSeg{(int32_t)size[space], ~(int32_t)(p.obj_box.size() / 6), 1, i});
            size[space] += 1;
            p.obj_box.insert(p.obj_box.end(), wlo, wlo + 3);
            p.obj_box.insert(p.obj_box.end(), whi, whi + 3);
        }
    };
    add_space(d.objects, d.num_objects, 0);
    add_space(d.lights, d.num_lights, 1);
    int64_t base = 0;
    for (size_t t = 0; t < trees.size(); ++t) {
        p.tree_base.push_back((int32_t)base);
        for (DevSeg s : trees[t]) {
            s.first += (int32_t)base;
            if (s.tri_base >= 0) p.n_tris += s.count;
            p.segs.push_back(s);
        }
        base += size[t];
    }
    p.tree_base.push_back((int32_t)base);
    p.ok = base < ((int64_t)1 << 30) && p.n_tris < ((int64_t)1 << 27);  // the leaf ref's 27 bits of `first`
    return p;
}

// Σ over the nodes of a tree of (child half-area / the root node's half-area) x (1 for an interior
// child, its triangle count for a leaf, 1 for an object leaf), summed over the trees whose root is
// a node.  The root node's area is that of the union of its child boxes.
inline double sah_cost(const Accel& a) {
    auto area = [](const Node& n, int k) {
        const double lo[3] = {n.lo[0][k], n.lo[1][k], n.lo[2][k]}, hi[3] = {n.hi[0][k], n.hi[1][k], n.hi[2][k]};
        return half_area(lo, hi);
    };
    std::set<int32_t> roots{a.obj_root, a.light_root};
    roots.insert(a.obj_blas.begin(), a.obj_blas.end());
    roots.insert(a.light_blas.begin(), a.light_blas.end());
    double cost = 0.0;
    for (const int32_t root : roots) {
        if (root < 0) continue;  // NONE, or a single leaf
        const Node& r = a.nodes[root];
        double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
        for (int k = 0; k < r.n; ++k)
            for (int x = 0; x < 3; ++x) {
                lo[x] = std::min(lo[x], (double)r.lo[x][k]);
                hi[x] = std::max(hi[x], (double)r.hi[x][k]);
            }
        const double ra = half_area(lo, hi);
        if (!(ra > 0.0)) continue;
        std::vector<int32_t> stk{root};
        while (!stk.empty()) {
            const Node& n = a.nodes[stk.back()];
            stk.pop_back();
            for (int k = 0; k < n.n; ++k) {
                const int32_t c = n.ref[k];
                const int w = is_leaf(c) ? std::max(1, leaf_count(c)) : 1;
                cost += area(n, k) / ra * w;
                if (!is_leaf(c)) stk.push_back(c);
            }
        }
    }
    return cost;
}

inline int tree_count(const Accel& a) {
    std::set<int32_t> roots{a.obj_root, a.light_root};
    roots.insert(a.obj_blas.begin(), a.obj_blas.end());
    roots.insert(a.light_blas.begin(), a.light_blas.end());
    roots.erase(NONE);
    return (int)roots.size();
}

}  // namespace
}  // namespace wbvh
}  // namespace lumo
