// api_surfel.h — the surfel map's handle, shared by api_surfel.hip (which creates, fills and reads it) and api_localize.hip
// (which reads its table and rule).
#pragma once
#include "api_voxelmap.h"

struct loamx_surfel_map : loamx::VoxelMapBase {  // ones: keys + first; zeros: sums, count, counters and lengths
  loamx_surfel_map_params params = {};
  loamx::CloudRule rule = {};
  loamx::SurfelTable t = {};
  uint32_t* d_slot = nullptr;   // scratch of a round of an add: [kCloudChunkPoints]
  uint8_t* d_keep = nullptr;    // [max(kCloudChunkPoints, max_voxels)] (add and emit)
  uint32_t* d_tiles = nullptr;  // the compaction's tiles for as many
};
