// test_place_shim.cpp — loam::PlaceDatabase (include/loam/place.h) through the C++ headers: descriptors and search records are
// the C ABI's (loamx_place_descriptor[_f32] / loamx_place_search on the same packed points and a database of its own), for
// double and float points; a scan turned by k sectors is found with shift k and PlaceMatch::initialGuess is that yaw.
// Built and run by tests/test_gpu_place_modules.py (needs a GPU).
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
struct PointF {
  float x, y, z, intensity;
};

// synthetic scan `which` of pair `pair`, turned about z by `sectors` x 2 pi / 60 (the sensor turns counter-clockwise: the
// points turn clockwise in its frame)
static std::vector<PointD> scan(uint64_t pair, uint32_t which, int sectors) {
  const uint32_t H = 16, W = 240, n = H * W;
  std::vector<double> xyz(n * 3);
  loamx_synth_scan_host(7, pair, which, H, W, 0.01, xyz.data());
  const double a = -6.283185307179586 * sectors / 60.0, c = std::cos(a), s = std::sin(a);
  std::vector<PointD> out;
  for (uint32_t i = 0; i < n; i++) out.push_back(PointD{c * xyz[3 * i] - s * xyz[3 * i + 1], s * xyz[3 * i] + c * xyz[3 * i + 1], xyz[3 * i + 2]});
  return out;
}

int main() {
  PlaceParams params;
  CHECK(params.n_rings == 20 && params.n_sectors == 60 && params.max_range == 80.0 && params.z_offset == 2.0 && params.z_scale == 64.0);
  loamx_place_params cp;
  loamx_default_place_params(&cp);
  CHECK(cp.n_rings == params.n_rings && cp.n_sectors == params.n_sectors && cp.max_range == params.max_range && cp.z_offset == params.z_offset &&
        cp.z_scale == params.z_scale);

  PlaceDatabase db(params);
  loamx_ctx* ctx = gpu::defaultContext();
  loamx_place_db* cdb = nullptr;
  CHECK(loamx_place_db_create(ctx, &cp, &cdb) == LOAMX_OK);
  std::vector<double> dirs(120);
  CHECK(loamx_place_db_sector_dirs(cdb, dirs.data()) == LOAMX_OK && dirs == db.sectorDirections());
  CHECK(db.size() == 0 && db.cells() == 1200);

  // five places; descriptors through the header equal the C ABI's, as doubles and as floats
  std::vector<PlaceDescriptor> descs;
  void* d_desc = nullptr;
  CHECK(loamx_dev_alloc(ctx, 1200 * sizeof(uint16_t), &d_desc) == LOAMX_OK);
  for (uint64_t place = 0; place < 5; place++) {
    const std::vector<PointD> pts = scan(place, 0, 0);
    const PlaceDescriptor d = db.descriptor(pts);
    const std::vector<double> xyz = gpu::pack<FieldAccessor>(pts);
    PlaceDescriptor want(1200);
    CHECK(loamx_place_descriptor(ctx, cdb, xyz.data(), 3, pts.size(), want.data()) == LOAMX_OK);
    CHECK(d == want);
    size_t filled = 0;
    for (uint16_t v : d) filled += v != 0;
    CHECK(filled > 50);
    std::vector<PointF> ptsf;
    for (const PointD& p : pts) ptsf.push_back(PointF{(float)p.x, (float)p.y, (float)p.z, 1.0f});
    const std::vector<float> xyzf = gpu::packFloat(ptsf);
    CHECK(loamx_place_descriptor_f32(ctx, cdb, xyzf.data(), 3, ptsf.size(), want.data()) == LOAMX_OK);
    CHECK(db.descriptor(ptsf) == want);
    CHECK(db.add(d) == (uint32_t)place);
    uint32_t first = 99;
    CHECK(loamx_copy_to_device(ctx, d_desc, d.data(), 1200 * sizeof(uint16_t)) == LOAMX_OK);
    CHECK(loamx_place_db_add_dev(ctx, cdb, static_cast<const uint16_t*>(d_desc), 1, &first) == LOAMX_OK && first == (uint32_t)place);
    descs.push_back(d);
  }
  CHECK(db.size() == 5);

  // the scan of place 3 as a sensor turned by 17 sectors sees it: the records are the C ABI's, the first is place 3 with shift 17
  const PlaceDescriptor q = db.descriptor(scan(3, 0, 17));
  for (uint32_t id_end : {0xFFFFFFFFu, 5u, 3u, 0u}) {
    const std::vector<PlaceMatch> got = db.search(q, 4, id_end);
    loamx_place_match want[4];
    CHECK(loamx_place_search(ctx, cdb, q.data(), 1, &id_end, 4, want) == LOAMX_OK);
    CHECK(got.size() == 4);
    for (size_t i = 0; i < got.size() && i < 4; i++) {
      CHECK(got[i].id == want[i].id && got[i].shift == want[i].shift && got[i].key_dist == want[i].key_dist);
      CHECK(std::memcmp(&got[i].distance, &want[i].distance, sizeof(double)) == 0);
      CHECK(got[i].valid() == (i < (id_end > 5 ? 5u : id_end)));
    }
    if (id_end >= 4) {
      CHECK(got[0].id == 3 && got[0].shift == 17 && got[0].distance < got[1].distance);
      const Pose3d guess = got[0].initialGuess();
      const double yaw = 6.283185307179586476925286766559 * 17.0 / 60.0;
      CHECK(std::fabs(guess.rotation.w() - std::cos(yaw / 2)) < 1e-15 && std::fabs(guess.rotation.z() - std::sin(yaw / 2)) < 1e-15);
      CHECK(guess.rotation.x() == 0.0 && guess.rotation.y() == 0.0 && guess.translation[0] == 0.0 && guess.translation[2] == 0.0);
      CHECK(got[0].yaw() == yaw);
    }
  }
  // an entry against itself
  const std::vector<PlaceMatch> self = db.search(descs[2], 1);
  CHECK(self.size() == 1 && self[0].id == 2 && self[0].shift == 0 && self[0].distance == 0.0 && self[0].key_dist == 0);

  bool threw = false;
  try {
    db.search(PlaceDescriptor(7), 1);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);
  threw = false;
  try {
    PlaceParams bad;
    bad.n_sectors = 2;
    PlaceDatabase refused(bad);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);

  loamx_dev_free(ctx, d_desc);
  loamx_place_db_destroy(ctx, cdb);
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
