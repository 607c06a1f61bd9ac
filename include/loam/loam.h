/** @brief Convenience header including the whole loam API (MI355X back end). */
#pragma once
#include "cloudmap.h"
#include "common.h"
#include "features.h"
#include "geometry.h"
#include "kdtree.h"
#include "occupancy.h"
#include "organize.h"
#include "place.h"
#include "posegraph.h"
#include "registration.h"
#include "segment.h"
#include "visibility.h"
