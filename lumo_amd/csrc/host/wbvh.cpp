// The wide BVH build (common/wbvh_build.h) compiled once, by g++ like the oracle's copy of it, so
// the upload (device/upload.hip) and the oracle lay out the same nodes and leaf records; and the
// host preparation of the device builder (common/wbvh_prep.h), which shares build's box rules.
#include "wbvh.h"

#include "../common/wbvh_build.h"
#include "../common/wbvh_prep.h"

namespace lumo {
namespace wbvh {

Accel build_accel(const lumo_scene_desc& d) { return build(d); }
DevPrep prepare_device_build(const lumo_scene_desc& d) { return prepare(d); }
double accel_sah_cost(const Accel& a) { return sah_cost(a); }
int accel_tree_count(const Accel& a) { return tree_count(a); }

}  // namespace wbvh
}  // namespace lumo
