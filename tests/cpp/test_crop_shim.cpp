// test_crop_shim.cpp — CloudMap::crop, SurfelMap::crop and OccupancyMap::crop (include/loam) through the C++ headers: after the same
// adds and the same crops the header's maps read back the bytes of maps of the C ABI that were cropped around a DEVICE pose with
// the same centre (loamx_cloud_map_crop / loamx_surfel_map_crop / loamx_occupancy_crop), and the counts agree.
//   test_crop_shim IN   IN: doubles {n_clouds, n_points, leaf, max_voxels, centre[3], n_boxes, (lo[3], hi[3]) per box, adds_before_box
//                       per box, offsets[n_clouds + 1], poses[n_clouds][7], points[n_points][3]}: cloud c is added before the first
//                       box b with adds_before_box[b] > c
// Built and run by tests/test_gpu_crop_modules.py (needs a GPU), which writes the inputs of the model comparison of
// tests/test_gpu_crop.py.
#include <cmath>
#include <cstdio>
#include <cstring>
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

struct PointD {
  double x, y, z;
};

struct Maps {
  CloudMap cloud;
  SurfelMap surfel;
  OccupancyMap occupancy;
  loamx_cloud_map* c_cloud = nullptr;
  loamx_surfel_map* c_surfel = nullptr;
  loamx_occupancy_map* c_occupancy = nullptr;
  Maps(const CloudMapParams& a, const SurfelMapParams& b, const OccupancyParams& c, size_t max_voxels)
      : cloud(a, max_voxels), surfel(b, max_voxels), occupancy(c, max_voxels) {}
};

static void compare(const Maps& m, loamx_ctx* ctx, const std::array<int32_t, 3>& vmin, const std::array<uint32_t, 3>& dims) {
  {
    const CloudMapPoints got = m.cloud.points();
    const size_t room = got.size() + 1;
    std::vector<double> xyz(3 * room);
    std::vector<uint32_t> counts(room), first(room);
    size_t n = 0;
    CHECK(loamx_cloud_map_emit(ctx, m.c_cloud, 1, xyz.data(), counts.data(), first.data(), room, &n) == LOAMX_OK);
    CHECK(n == got.size());
    if (n == got.size() && n) {
      CHECK(std::memcmp(xyz.data(), got.xyz.data(), 3 * n * sizeof(double)) == 0);
      CHECK(std::memcmp(counts.data(), got.counts.data(), n * sizeof(uint32_t)) == 0);
      CHECK(std::memcmp(first.data(), got.first.data(), n * sizeof(uint32_t)) == 0);
    }
    loamx_cloud_map_stats cs;
    CHECK(loamx_cloud_map_stats_read(ctx, m.c_cloud, &cs) == LOAMX_OK);
    const CloudMapStats s = m.cloud.stats();
    CHECK(s.voxels == cs.voxels && s.voxels == n && s.points_offered == cs.points_offered && s.points_used == cs.points_used && s.overflow == 0);
  }
  {
    const std::vector<Surfel> got = m.surfel.surfels();
    std::vector<Surfel> want(got.size() + 1);
    size_t n = 0;
    CHECK(loamx_surfel_map_emit_host(ctx, m.c_surfel, 1, want.data(), want.size(), &n) == LOAMX_OK);
    CHECK(n == got.size());
    if (n == got.size() && n) CHECK(std::memcmp(want.data(), got.data(), n * sizeof(Surfel)) == 0);
    CHECK(m.surfel.stats().voxels == n && m.surfel.stats().overflow == 0);
  }
  {
    const OccupancyCells got = m.occupancy.box(vmin, dims);
    const size_t n = (size_t)dims[0] * dims[1] * dims[2];
    std::vector<uint32_t> counts(2 * n);
    std::vector<uint8_t> states(n);
    CHECK(loamx_occupancy_box(ctx, m.c_occupancy, vmin.data(), dims.data(), counts.data(), states.data()) == LOAMX_OK);
    CHECK(got.size() == n && std::memcmp(counts.data(), got.counts.data(), 2 * n * sizeof(uint32_t)) == 0);
    CHECK(got.size() == n && std::memcmp(states.data(), got.states.data(), n) == 0);
    loamx_occupancy_stats cs;
    CHECK(loamx_occupancy_stats_read(ctx, m.c_occupancy, &cs) == LOAMX_OK);
    CHECK(m.occupancy.stats().voxels == cs.voxels && cs.overflow == 0);
  }
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::printf("usage: %s IN\n", argv[0]);
    return 2;
  }
  std::vector<double> in;
  {
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
      std::printf("cannot read %s\n", argv[1]);
      return 2;
    }
    double v;
    while (std::fread(&v, sizeof(v), 1, f) == 1) in.push_back(v);
    std::fclose(f);
  }
  size_t at = 0;
  const size_t n_clouds = (size_t)in[at++], n_points = (size_t)in[at++];
  const double leaf = in[at++];
  const size_t max_voxels = (size_t)in[at++];
  std::array<double, 3> centre;
  for (int a = 0; a < 3; a++) centre[a] = in[at++];
  const size_t n_boxes = (size_t)in[at++];
  std::vector<std::array<double, 3>> lo(n_boxes), hi(n_boxes);
  for (size_t b = 0; b < n_boxes; b++) {
    for (int a = 0; a < 3; a++) lo[b][a] = in[at++];
    for (int a = 0; a < 3; a++) hi[b][a] = in[at++];
  }
  std::vector<size_t> adds_before(n_boxes);
  for (size_t b = 0; b < n_boxes; b++) adds_before[b] = (size_t)in[at++];
  const double* offsets = &in[at];
  at += n_clouds + 1;
  const double* poses = &in[at];
  at += 7 * n_clouds;
  const double* points = &in[at];
  CHECK(at + 3 * n_points == in.size());
  if (g_failures) return 1;

  CloudMapParams cp;
  SurfelMapParams sp;
  OccupancyParams op;
  cp.leaf = sp.leaf = op.leaf = leaf;
  cp.min_range = sp.min_range = op.min_range = 0.01;
  cp.max_range = sp.max_range = op.max_range = 80.0;
  Maps m(cp, sp, op, max_voxels);
  loamx_ctx* ctx = gpu::defaultContext();
  loamx_cloud_map_params ccp = {leaf, 0.01, 80.0};
  loamx_surfel_map_params csp = {leaf, 0.01, 80.0};
  loamx_occupancy_params cop;
  loamx_default_occupancy_params(&cop);
  cop.leaf = leaf, cop.min_range = 0.01, cop.max_range = 80.0;
  CHECK(loamx_cloud_map_create(ctx, &ccp, max_voxels, &m.c_cloud) == LOAMX_OK);
  CHECK(loamx_surfel_map_create(ctx, &csp, max_voxels, &m.c_surfel) == LOAMX_OK);
  CHECK(loamx_occupancy_create(ctx, &cop, max_voxels, &m.c_occupancy) == LOAMX_OK);

  // the centre in a device pose whose quaternion is no unit quaternion, and the counts in device memory
  void* d_block = nullptr;
  CHECK(loamx_dev_alloc(ctx, 7 * sizeof(double) + 4 * sizeof(uint32_t), &d_block) == LOAMX_OK);
  const double pose[7] = {0.7, -0.1, 0.6, 0.4, centre[0], centre[1], centre[2]};
  CHECK(loamx_copy_to_device(ctx, d_block, pose, sizeof(pose)) == LOAMX_OK);
  const double* d_pose = static_cast<const double*>(d_block);
  uint32_t* d_counts = reinterpret_cast<uint32_t*>(static_cast<char*>(d_block) + sizeof(pose));

  const std::array<int32_t, 3> vmin = {-14, -14, -6};
  const std::array<uint32_t, 3> dims = {34, 28, 12};
  size_t added = 0;
  for (size_t b = 0; b <= n_boxes; b++) {
    const size_t until = b < n_boxes ? adds_before[b] : n_clouds;
    for (; added < until && added < n_clouds; added++) {
      const size_t p0 = (size_t)offsets[added], p1 = (size_t)offsets[added + 1];
      std::vector<PointD> pts;
      for (size_t i = p0; i < p1; i++) pts.push_back(PointD{points[3 * i], points[3 * i + 1], points[3 * i + 2]});
      const std::vector<double> xyz = gpu::pack<FieldAccessor>(pts);
      const Pose3d at_pose = Pose3d::fromArray(poses + 7 * added);
      double back[7];
      at_pose.toArray(back);
      m.cloud.add(pts, at_pose), m.surfel.add(pts, at_pose), m.occupancy.add(pts, at_pose);
      CHECK(loamx_cloud_map_add_cloud(ctx, m.c_cloud, xyz.data(), 3, pts.size(), back) == LOAMX_OK);
      CHECK(loamx_surfel_map_add_cloud_host(ctx, m.c_surfel, xyz.data(), 3, pts.size(), back) == LOAMX_OK);
      CHECK(loamx_occupancy_add_cloud(ctx, m.c_occupancy, xyz.data(), 3, pts.size(), back) == LOAMX_OK);
    }
    compare(m, ctx, vmin, dims);
    if (b == n_boxes) break;
    uint32_t counts[4];
    const MapCrop a = m.cloud.crop(lo[b], hi[b], centre);
    CHECK(loamx_cloud_map_crop(ctx, m.c_cloud, d_pose, lo[b].data(), hi[b].data(), d_counts) == LOAMX_OK);
    CHECK(loamx_copy_to_host(ctx, counts, d_counts, sizeof(counts)) == LOAMX_OK);
    CHECK(a.kept == counts[0] && a.removed == counts[1] && counts[2] == 0 && counts[3] == 0 && a.kept > 50 && a.removed > 50);
    const MapCrop s = m.surfel.crop(lo[b], hi[b], centre);
    CHECK(loamx_surfel_map_crop(ctx, m.c_surfel, d_pose, lo[b].data(), hi[b].data(), d_counts) == LOAMX_OK);
    CHECK(loamx_copy_to_host(ctx, counts, d_counts, sizeof(counts)) == LOAMX_OK);
    CHECK(s.kept == counts[0] && s.removed == counts[1] && counts[2] == 0 && s.kept > 50 && s.removed > 50);
    const MapCrop o = m.occupancy.crop(lo[b], hi[b], centre);
    CHECK(loamx_occupancy_crop(ctx, m.c_occupancy, d_pose, lo[b].data(), hi[b].data(), d_counts) == LOAMX_OK);
    CHECK(loamx_copy_to_host(ctx, counts, d_counts, sizeof(counts)) == LOAMX_OK);
    CHECK(o.kept == counts[0] && o.removed == counts[1] && counts[2] == 0 && o.kept > 50 && o.removed > 50);
    compare(m, ctx, vmin, dims);
  }
  // the default centre is the origin; a centre that is not finite and a box with lo > hi are refused and change nothing
  const MapCrop all = m.cloud.crop({-1e9, -1e9, -1e9}, {1e9, 1e9, 1e9});
  CHECK(all.removed == 0 && all.kept == m.cloud.stats().voxels);
  int threw = 0;
  try {
    m.surfel.crop({-1.0, -1.0, -1.0}, {1.0, 1.0, 1.0}, {0.0, NAN, 0.0});
  } catch (const std::runtime_error&) {
    threw++;
  }
  try {
    m.occupancy.crop({1.0, -1.0, -1.0}, {-1.0, 1.0, 1.0});
  } catch (const std::runtime_error&) {
    threw++;
  }
  CHECK(threw == 2);
  compare(m, ctx, vmin, dims);

  loamx_dev_free(ctx, d_block);
  loamx_cloud_map_destroy(ctx, m.c_cloud), loamx_surfel_map_destroy(ctx, m.c_surfel), loamx_occupancy_destroy(ctx, m.c_occupancy);
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
