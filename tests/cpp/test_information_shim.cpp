// test_information_shim.cpp — loam::registrationInformation (include/loam/registration.h) through the C++ headers on one
// synthetic 16 x 256 scan pair: the record is the C ABI's (loamx_registration_information on the same packed points), against
// the target and against a TargetIndex; covariance() and degenerateDirections() against the record's own eigenpairs.
// Built and run by tests/test_gpu_information_modules.py (needs a GPU).
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

struct Point {
  double x, y, z;
  Point(double x, double y, double z) : x(x), y(y), z(z) {}
};

static std::vector<Point> synth_scan(uint32_t which) {
  std::vector<double> xyz(16 * 256 * 3);
  loamx_synth_scan_host(3, 2, which, 16, 256, 0.01, xyz.data());
  std::vector<Point> out;
  for (size_t i = 0; i < xyz.size(); i += 3) out.push_back(Point(xyz[i], xyz[i + 1], xyz[i + 2]));
  return out;
}

static bool same_record(const RegistrationInformation& r, const loamx_reg_information& c) {
  return std::memcmp(r.information, c.information, sizeof(c.information)) == 0 &&
         std::memcmp(r.eigenvalues, c.eigenvalues, sizeof(c.eigenvalues)) == 0 &&
         std::memcmp(r.eigenvectors, c.eigenvectors, sizeof(c.eigenvectors)) == 0 &&
         std::memcmp(r.gradient, c.gradient, sizeof(c.gradient)) == 0 && r.weighted_sq_error == c.weighted_sq_error &&
         r.n_edge == c.n_edge && r.n_plane == c.n_plane && r.n_huber == c.n_huber && r.n_dropped == c.n_dropped;
}

int main() {
  const LidarParams lidar(16, 256, 1.0, 120.0);
  const LoamFeatures<Point> target = extractFeatures(synth_scan(0), lidar), source = extractFeatures(synth_scan(1), lidar);
  CHECK(target.planar_points.size() > 512 && source.edge_points.size() > 20);
  const Pose3d registered = registerFeatures(source, target, Pose3d::Identity());
  const RegistrationInformation info = registrationInformation(source, target, registered);
  CHECK(info.n_edge > 30 && info.n_plane > 500 && info.n_dropped == 0);

  // the C ABI on the same points
  const std::vector<double> se = gpu::pack<FieldAccessor>(source.edge_points), sp = gpu::pack<FieldAccessor>(source.planar_points);
  const std::vector<double> te = gpu::pack<FieldAccessor>(target.edge_points), tp = gpu::pack<FieldAccessor>(target.planar_points);
  const loamx_reg_params rp = gpu::toC(RegistrationParams());
  double pose[7];
  registered.toArray(pose);
  loamx_reg_information c{};
  CHECK(loamx_registration_information(gpu::defaultContext(), se.data(), source.edge_points.size(), sp.data(), source.planar_points.size(),
                                       te.data(), target.edge_points.size(), tp.data(), target.planar_points.size(), pose, &rp, &c) == LOAMX_OK);
  CHECK(same_record(info, c));
  const TargetIndex index = TargetIndex::build(target);
  CHECK(same_record(registrationInformation(source, index, registered), c));

  // eigenpairs: ascending, H v = lambda v
  bool ascending = true, eigen = true;
  for (int i = 0; i + 1 < 6; i++) ascending = ascending && info.eigenvalues[i] <= info.eigenvalues[i + 1];
  for (int i = 0; i < 6; i++)
    for (int a = 0; a < 6; a++) {
      double hv = 0.0;
      for (int b = 0; b < 6; b++) hv += info.information[6 * a + b] * info.eigenvectors[6 * i + b];
      eigen = eigen && std::fabs(hv - info.eigenvalues[i] * info.eigenvectors[6 * i + a]) <= 1e-9 * info.eigenvalues[5];
    }
  CHECK(ascending && eigen && info.eigenvalues[0] > 100.0);

  // covariance: H cov = sigma^2 I for a full-rank H
  const std::vector<double> cov = info.covariance();
  const double sigma2 = info.weighted_sq_error / static_cast<double>(info.n_edge + info.n_plane - 6);
  bool inverse = cov.size() == 36;
  for (int a = 0; a < 6 && inverse; a++)
    for (int b = 0; b < 6; b++) {
      double hc = 0.0;
      for (int k = 0; k < 6; k++) hc += info.information[6 * a + k] * cov[6 * k + b];
      inverse = inverse && std::fabs(hc - (a == b ? sigma2 : 0.0)) <= 1e-9 * sigma2;
    }
  CHECK(inverse && sigma2 > 0.0);
  CHECK(info.degenerateDirections(100.0).empty());
  const std::vector<std::vector<double>> low = info.degenerateDirections(0.5 * (info.eigenvalues[2] + info.eigenvalues[3]));
  CHECK(low.size() == 3 && low[2].size() == 6 && low[2][0] == info.eigenvectors[12] && low[2][5] == info.eigenvectors[17]);
  // a threshold above every eigenvalue but the largest keeps one direction: cov = sigma^2 v5 v5^T / lambda5
  const std::vector<double> one = info.covariance(0.999);
  CHECK(std::fabs(one[0] - sigma2 * info.eigenvectors[30] * info.eigenvectors[30] / info.eigenvalues[5]) <= 1e-15 * std::fabs(one[0]) + 1e-300);

  // too few rows: no variance
  bool threw = false;
  try {
    RegistrationInformation empty{};
    empty.covariance();
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);
  // refusals arrive as exceptions
  threw = false;
  try {
    RegistrationParams bad;
    bad.num_plane_neighbors = 17;
    registrationInformation(source, target, registered, bad);
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
