// api_occupancy.h — the handle of the occupancy map, for the host units that work on it: api_occupancy.hip (the map itself and its
// distance field) and api_raycast.hip (the ray cast).
#pragma once
#include "api_voxelmap.h"

struct loamx_occupancy_map : loamx::VoxelMapBase {  // ones: keys; zeros: counts and counters
  loamx_occupancy_params params = {};
  loamx::OccRule rule = {};
  loamx::OccStateRule state_rule = {};
  loamx::OccTable t = {};
  void* dist_block = nullptr;  // the staging of the distance field, allocated at the first distance call, grown when one needs more
  size_t dist_bytes = 0;
};

namespace loamx {

// a null map or a map of another context: refused in the occupancy map's words (api_occupancy.hip)
int occupancy_map_check(loamx_ctx* ctx, const loamx_occupancy_map* map);

}  // namespace loamx
