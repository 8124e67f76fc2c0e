// Host entry of the wide BVH build (common/wbvh_build.h), called by lumo_scene_upload, and the host
// part of the device builder (common/wbvh_prep.h).
#pragma once
#include "../../../include/lumo_amd.h"
#include "../common/wbvh_accel.h"
#include "../common/wbvh_dev_prep.h"

namespace lumo {
namespace wbvh {

Accel build_accel(const lumo_scene_desc& d);
DevPrep prepare_device_build(const lumo_scene_desc& d);
double accel_sah_cost(const Accel& a);
int accel_tree_count(const Accel& a);

}  // namespace wbvh
}  // namespace lumo
