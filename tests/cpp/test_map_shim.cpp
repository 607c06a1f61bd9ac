// test_map_shim.cpp — the map upkeep members of loam::TargetIndex (include/loam/registration.h: insertFiltered, crop,
// edgePoints / planarPoints) through the C++ headers, on inputs whose outcome can be written down by hand.
// Built and run by tests/test_gpu_map_cpp_shim.py (needs a GPU).
#include <cstdio>
#include <limits>
#include <vector>

#include "loam/loam.h"

using namespace loam;

static int g_failures = 0, g_checks = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    g_checks++;                                                            \
    if (!(cond)) {                                                         \
      g_failures++;                                                        \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
    }                                                                      \
  } while (0)

struct Point {
  double x, y, z;
  Point(double x, double y, double z) : x(x), y(y), z(z) {}
};

int main() {
  // a 10 x 10 lattice of planar points, one per half-metre voxel (at the voxel centres), and a row of edge points
  LoamFeatures<Point> base;
  for (int i = 0; i < 10; i++)
    for (int j = 0; j < 10; j++) base.planar_points.push_back(Point(0.5 * i + 0.25, 0.5 * j + 0.25, 0.25));
  for (int i = 0; i < 10; i++) base.edge_points.push_back(Point(0.5 * i + 0.25, 0.25, 1.25));
  TargetIndex map = TargetIndex::build(base);
  CHECK(map.numEdgePoints() == 10 && map.numPlanarPoints() == 100);

  // a scan displaced by (5, 0, 0): per kind, two points in every voxel of the lattice next door, and the scan carries
  // them in the frame in which they coincide with the base — world_T_scan moves them over
  LoamFeatures<Point> scan;
  for (int i = 0; i < 10; i++)
    for (int j = 0; j < 10; j++) {
      scan.planar_points.push_back(Point(0.5 * i + 0.125, 0.5 * j + 0.125, 0.125));
      scan.planar_points.push_back(Point(0.5 * i + 0.375, 0.5 * j + 0.375, 0.375));
    }
  for (int i = 0; i < 10; i++) scan.edge_points.push_back(Point(0.5 * i + 0.125, 0.125, 1.125));
  const Pose3d world_T_scan(Quaterniond::Identity(), Vector3d(5.0, 0.0, 0.0));
  // at the identity every voxel is taken by the base
  std::pair<size_t, size_t> added = map.insertFiltered(scan, Pose3d::Identity(), 0.5, 0.5);
  CHECK(added.first == 0 && added.second == 0);
  CHECK(map.numEdgePoints() == 10 && map.numPlanarPoints() == 100);
  // moved over, the first point of every voxel is added
  added = map.insertFiltered(scan, world_T_scan, 0.5, 0.5);
  CHECK(added.first == 10 && added.second == 100);
  // ... once
  added = map.insertFiltered(scan, world_T_scan, 0.5, 0.5);
  CHECK(added.first == 0 && added.second == 0);
  CHECK(map.numEdgePoints() == 20 && map.numPlanarPoints() == 200);

  const std::vector<Vector3d> planar = map.planarPoints(), edge = map.edgePoints();
  CHECK(planar.size() == 200 && edge.size() == 20);
  bool same = true;
  for (size_t k = 0; k < 100; k++) {  // the base as given, then the FIRST point of every voxel, moved (exact: x + 5 with x a multiple of 1/8)
    const Point& b = base.planar_points[k];
    const Point& s = scan.planar_points[2 * k];
    same = same && planar[k](0) == b.x && planar[k](1) == b.y && planar[k](2) == b.z;
    same = same && planar[100 + k](0) == s.x + 5.0 && planar[100 + k](1) == s.y && planar[100 + k](2) == s.z;
  }
  CHECK(same);
  CHECK(edge[10](0) == 5.125 && edge[19](0) == 9.625 && edge[19](2) == 1.125);

  // an unfiltered kind: leaf <= 0 adds every point
  added = map.insertFiltered(scan, world_T_scan, 0.0, 0.5);
  CHECK(added.first == 10 && added.second == 0);

  // the window: x in [4, 8] keeps base columns i = 8, 9 (x = 4.25, 4.75) and the moved columns i = 0 .. 5 (x <= 7.875)
  const double inf = std::numeric_limits<double>::infinity();
  std::pair<size_t, size_t> removed = map.crop(Vector3d(4.0, -inf, -inf), Vector3d(8.0, inf, inf));
  CHECK(map.numPlanarPoints() == 20 + 60 && removed.second == 120);
  CHECK(map.numEdgePoints() == 2 + 6 + 6 && removed.first == 16);
  const std::vector<Vector3d> kept = map.planarPoints();
  bool inside = kept.size() == 80, ordered = true;
  for (const Vector3d& p : kept) inside = inside && p(0) >= 4.0 && p(0) <= 8.0;
  for (size_t k = 1; k < 20 && k < kept.size(); k++) ordered = ordered && (kept[k](0) > kept[k - 1](0) || kept[k](1) > kept[k - 1](1));
  CHECK(inside && ordered);

  bool threw = false;
  try {
    map.crop(Vector3d(1.0, 0.0, 0.0), Vector3d(0.0, 1.0, 1.0));
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
