// What the host prepares for the device builder of the wide BVH (wbvh_prep.h prepare(), compiled by
// g++ in host/wbvh.cpp) and device/wbvh_dev.hip consumes: plain data, no build code.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

namespace lumo {
namespace wbvh {

// A run of primitives of one tree, in primitive order.  tri_base >= 0: triangles tri_base ..
// tri_base + count - 1 of object `obj` (-1 in a BLAS).  tri_base < 0: one object leaf (count 1) of
// object `obj`, its world box the six doubles at obj_box[6 * ~tri_base].
struct DevSeg {
    int32_t first;  // primitive index of the run's first primitive (over all trees)
    int32_t tri_base, count, obj;
};

struct DevPrep {
    std::vector<DevSeg> segs;           // all trees, ordered by first
    std::vector<int32_t> tree_base;     // trees + 1 primitive offsets: 0 world objects, 1 world lights, 2.. BLASes
    std::vector<double> obj_box;        // lo[3], hi[3] per object leaf
    std::vector<std::pair<int, int>> inst_tree;  // (space * 2^30 + index, tree) of every instance
    int64_t n_tris = 0;                 // leaf triangle records of the finished trees
    bool ok = false;                    // false: refused on the host (a light kd tree too deep, or too large)
};

}  // namespace wbvh
}  // namespace lumo
