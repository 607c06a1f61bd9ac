// TEST-ONLY: surfel_math.h (the arithmetic of the surfel map kernels) compiled for the host as a program of its own, for
// tests/test_surfel_hostcheck.py (the file formats: tests/surfel_common.py).
//   hostcheck_surfel points IN OUT   a header and n x 3 doubles -> per point what, key and the twelve words of surfel_point
//   hostcheck_surfel finish IN OUT   records of a voxel's sums  -> loamx_surfel records
// The `san` target builds the same file with -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../loam_amd/csrc/surfel_math.h"

using namespace loamx;

static_assert(sizeof(loamx_surfel) == 128, "loamx_surfel is 128 bytes");

struct PointIn {
  uint64_t n;
  double leaf, min_r2, max_r2;
  uint64_t has_pose;
  double pose[7];
};
struct PointOut {
  uint64_t what, key, m[12];
};
struct FinishIn {
  uint64_t key, s[3], S[6];
  int64_t W[3];
  uint32_t count, first;
  double leaf;
};
static_assert(sizeof(PointIn) == 96 && sizeof(PointOut) == 112 && sizeof(FinishIn) == 120, "the formats of tests/surfel_common.py");

static bool read_all(const char* path, std::vector<char>& buf) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long size = ftell(f);
  fseek(f, 0, SEEK_SET);
  buf.resize(size > 0 ? (size_t)size : 0);
  const bool ok = buf.empty() || fread(buf.data(), 1, buf.size(), f) == buf.size();
  fclose(f);
  return ok;
}

static bool write_all(const char* path, const void* p, size_t bytes) {
  FILE* f = fopen(path, "wb");
  if (!f) return false;
  const bool ok = bytes == 0 || fwrite(p, 1, bytes, f) == bytes;
  return fclose(f) == 0 && ok;
}

static int run_points(const std::vector<char>& in, const char* out_path) {
  PointIn h;
  if (in.size() < sizeof(h)) return 2;
  memcpy(&h, in.data(), sizeof(h));
  if (in.size() != sizeof(h) + h.n * 3 * sizeof(double)) return 2;
  std::vector<double> pts(h.n * 3);
  if (h.n) memcpy(pts.data(), in.data() + sizeof(h), pts.size() * sizeof(double));
  std::vector<PointOut> out(h.n);
  for (uint64_t i = 0; i < h.n; i++) {
    PointOut& r = out[i];
    memset(&r, 0, sizeof(r));
    Vec3 p = v3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
    int what = cloud_validity(p, h.min_r2, h.max_r2);
    if (what == kCloudUsed) {
      Vec3 o = v3(0.0, 0.0, 0.0);
      if (h.has_pose) p = pose_act(h.pose, p), o = v3(h.pose[4], h.pose[5], h.pose[6]);
      uint64_t key = 0;
      uint32_t u[3];
      unsigned long long m[kSurfelMoments] = {};
      if (cloud_cell(p, h.leaf, key, u)) surfel_point(u, o, p, h.leaf, m);
      else what = kCloudOutside;
      r.key = key;
      for (int k = 0; k < kSurfelMoments; k++) r.m[k] = m[k];
    }
    r.what = (uint64_t)what;
  }
  return write_all(out_path, out.data(), out.size() * sizeof(PointOut)) ? 0 : 3;
}

static int run_finish(const std::vector<char>& in, const char* out_path) {
  if (in.size() % sizeof(FinishIn)) return 2;
  const size_t n = in.size() / sizeof(FinishIn);
  std::vector<loamx_surfel> out(n);
  for (size_t i = 0; i < n; i++) {
    FinishIn f;
    memcpy(&f, in.data() + i * sizeof(f), sizeof(f));
    if (f.count == 0) return 2;
    out[i] = surfel_finish(f.key, f.s, f.S, f.W, f.count, f.first, f.leaf);
  }
  return write_all(out_path, out.data(), n * sizeof(loamx_surfel)) ? 0 : 3;
}

int main(int argc, char** argv) {
  if (argc != 4) {
    fprintf(stderr, "usage: %s points|finish IN OUT\n", argv[0]);
    return 1;
  }
  std::vector<char> in;
  if (!read_all(argv[2], in)) {
    fprintf(stderr, "cannot read %s\n", argv[2]);
    return 2;
  }
  int rc = 1;
  if (!strcmp(argv[1], "points")) rc = run_points(in, argv[3]);
  else if (!strcmp(argv[1], "finish")) rc = run_finish(in, argv[3]);
  if (rc) fprintf(stderr, "hostcheck_surfel %s: error %d\n", argv[1], rc);
  return rc;
}
