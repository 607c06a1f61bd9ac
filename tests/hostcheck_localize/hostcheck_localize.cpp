// TEST-ONLY: localize_math.h (the arithmetic of the surfel localisation kernels) compiled for the host, with a loop that runs the
// whole solve in the kernels' orders: chunks of kLocChunk points, thread t of 256 takes points t, t + 256, ..., the shuffle tree
// 32 .. 1 per wavefront, the four wavefronts in order, the chunks in order. One function takes a blob and returns a blob (the
// formats: tests/localize_common.py); it is exported from libhostcheck_localize.so and, with -DHOSTCHECK_LOCALIZE_MAIN, wrapped in
// a program `hostcheck_localize_san IN OUT` that the `san` target builds with -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <unordered_map>
#include <vector>

#include "../../loam_amd/csrc/localize_math.h"

using namespace loamx;

struct Params {  // loamx_localize_params
  uint32_t neighborhood, min_points;
  double planarity, max_distance, huber_delta;
  uint32_t max_iterations, min_rows;
  double rot_thresh, pos_thresh, min_eig_per_row;
};
struct Head {
  uint64_t n_vox, n_rows, stride, n_clouds;
  double leaf, min_range, max_range;
  Params params;
};
struct VoxIn {
  uint64_t key, s[3], S[6];
  int64_t W[3];
  uint32_t count, first;
};
static_assert(sizeof(Params) == 64 && sizeof(Head) == 120 && sizeof(VoxIn) == 112 && sizeof(LocResult) == 128 && sizeof(loamx_reg_information) == 696,
              "the formats of tests/localize_common.py");

// per-point outcome of the last evaluation: 0 .. 6 the chosen candidate of a point that gave a row
enum { kOutUnused = -1, kOutNoSurfel = -2, kOutGated = -3, kOutNotFinite = -4 };

typedef std::unordered_map<uint64_t, LocPlane> Planes;

static int point_outcome(const LocAcc& before, const LocAcc& after, int best) {
  if (after.c[kLocRows] != before.c[kLocRows]) return best;
  if (after.c[kLocGated] != before.c[kLocGated]) return kOutGated;
  return kOutNotFinite;
}

// one evaluation of a cloud's n points at pose T: the sums in the kernels' order, the counters, and (chosen may be null) the outcomes
static void evaluate(const LocRule& R, const Planes& planes, const double* pts, uint64_t stride, uint64_t n, const double T[7], double sums[kInfoSums],
                     uint32_t cnt[kLocCounters], int32_t* chosen) {
  for (int j = 0; j < kInfoSums; j++) sums[j] = 0.0;
  for (int j = 0; j < kLocCounters; j++) cnt[j] = 0u;
  const int nk = R.neighborhood == 7u ? kLocCandidates : 1;
  std::vector<LocAcc> acc(kLocThreads);
  for (uint64_t base = 0; base < n; base += kLocChunk) {
    for (int t = 0; t < kLocThreads; t++) {
      LocAcc& A = acc[t];
      loc_acc_clear(A);
      for (int it = 0; it < kLocItems; it++) {
        const uint64_t i = base + (uint64_t)it * kLocThreads + t;
        if (i >= n) break;
        const double* q = pts + i * stride;
        Vec3 v;
        uint64_t home;
        if (!loc_move(R, T, v3(q[0], q[1], q[2]), v, home)) {
          A.c[kLocUnused]++;
          if (chosen) chosen[i] = kOutUnused;
          continue;
        }
        int best = -1;
        double best_d2 = 0.0;
        LocPlane best_plane;
        memset(&best_plane, 0, sizeof(best_plane));
        for (int k = 0; k < nk; k++) {
          uint64_t key;
          if (!loc_candidate_key(home, k, key)) continue;
          const Planes::const_iterator f = planes.find(key);
          if (f == planes.end()) continue;
          loc_offer(v, f->second, k, best_d2, best, best_plane);
        }
        if (best < 0) {
          A.c[kLocNoSurfel]++;
          if (chosen) chosen[i] = kOutNoSurfel;
          continue;
        }
        const LocAcc before = A;
        loc_accumulate(R, v, best_plane, true, A);
        if (chosen) chosen[i] = point_outcome(before, A, best);
      }
    }
    double v[kLocThreads];
    for (int j = 0; j < kInfoSums; j++) {
      for (int t = 0; t < kLocThreads; t++) v[t] = acc[t].s[j];
      sums[j] += loc_chunk_sum(v);
    }
    for (int j = 0; j < kLocCounters; j++)
      for (int t = 0; t < kLocThreads; t++) cnt[j] += acc[t].c[j];
  }
}

// in: Head, vox[n_vox], points[n_rows * stride], offsets[n_clouds + 1], poses[n_clouds * 7]
// out: poses[n_clouds * 7], LocResult[n_clouds], loamx_reg_information[n_clouds], int32 chosen[n_rows]
static int run_blob(const char* in, uint64_t in_bytes, std::vector<char>& out) {
  Head h;
  if (in_bytes < sizeof(h)) return 2;
  memcpy(&h, in, sizeof(h));
  if (h.stride < 3 || h.n_vox > (1ull << 32) || h.n_rows > (1ull << 32) || h.n_clouds > (1ull << 24) || h.stride > 64) return 2;
  const uint64_t o_vox = sizeof(h), o_pts = o_vox + h.n_vox * sizeof(VoxIn), o_off = o_pts + h.n_rows * h.stride * sizeof(double);
  const uint64_t o_pose = o_off + (h.n_clouds + 1) * sizeof(uint64_t), end = o_pose + h.n_clouds * 7 * sizeof(double);
  if (in_bytes != end) return 2;
  std::vector<VoxIn> vox(h.n_vox);
  std::vector<double> pts(h.n_rows * h.stride), poses(h.n_clouds * 7);
  std::vector<uint64_t> off(h.n_clouds + 1);
  if (!vox.empty()) memcpy(vox.data(), in + o_vox, vox.size() * sizeof(VoxIn));
  if (!pts.empty()) memcpy(pts.data(), in + o_pts, pts.size() * sizeof(double));
  memcpy(off.data(), in + o_off, off.size() * sizeof(uint64_t));
  if (!poses.empty()) memcpy(poses.data(), in + o_pose, poses.size() * sizeof(double));
  for (uint64_t c = 0; c < h.n_clouds; c++)
    if (off[c + 1] < off[c] || off[c + 1] > h.n_rows) return 2;

  LocRule R;
  R.leaf = h.leaf, R.min_r2 = h.min_range * h.min_range, R.max_r2 = h.max_range * h.max_range;
  R.planarity = h.params.planarity, R.max_distance = h.params.max_distance == 0.0 ? h.leaf : h.params.max_distance;
  R.huber_delta = h.params.huber_delta, R.min_points = h.params.min_points, R.neighborhood = h.params.neighborhood;
  LocSolve P;
  P.rot_thresh = h.params.rot_thresh, P.pos_thresh = h.params.pos_thresh, P.min_eig_per_row = h.params.min_eig_per_row;
  P.max_iterations = h.params.max_iterations, P.min_rows = h.params.min_rows;

  Planes planes;
  for (const VoxIn& e : vox) {
    if (e.count == 0) return 2;
    planes[e.key] = loc_plane_of(surfel_finish(e.key, e.s, e.S, e.W, e.count, e.first, h.leaf), R.min_points, R.planarity);
  }

  const uint64_t o_res = h.n_clouds * 7 * sizeof(double), o_info = o_res + h.n_clouds * sizeof(LocResult);
  const uint64_t o_chosen = o_info + h.n_clouds * sizeof(loamx_reg_information);
  out.assign(o_chosen + h.n_rows * sizeof(int32_t), 0);
  std::vector<int32_t> chosen(h.n_rows, kOutUnused);
  for (uint64_t c = 0; c < h.n_clouds; c++) {
    const uint64_t n = off[c + 1] - off[c];
    const double* cp = pts.data() + off[c] * h.stride;
    LocState S;
    loc_state_init(S, poses.data() + 7 * c, P.max_iterations);
    double sums[kInfoSums];
    uint32_t cnt[kLocCounters];
    for (uint32_t it = 0; it < P.max_iterations && !S.done; it++) {
      evaluate(R, planes, cp, h.stride, n, S.pose, sums, cnt, nullptr);
      loc_iterate(S, P, sums, cnt[kLocRows]);
    }
    evaluate(R, planes, cp, h.stride, n, S.pose, sums, cnt, chosen.data() + off[c]);
    LocResult res;
    loamx_reg_information info;
    memset(&res, 0, sizeof(res)), memset(&info, 0, sizeof(info));
    loc_finish(S, P, sums, cnt, res, &info);
    memcpy(out.data() + c * 7 * sizeof(double), S.pose, 7 * sizeof(double));
    memcpy(out.data() + o_res + c * sizeof(res), &res, sizeof(res));
    memcpy(out.data() + o_info + c * sizeof(info), &info, sizeof(info));
  }
  if (h.n_rows) memcpy(out.data() + o_chosen, chosen.data(), h.n_rows * sizeof(int32_t));
  return 0;
}

extern "C" int hostcheck_localize(const void* in, uint64_t in_bytes, void* out, uint64_t out_cap, uint64_t* out_bytes) {
  std::vector<char> o;
  const int rc = run_blob(static_cast<const char*>(in), in_bytes, o);
  if (rc) return rc;
  *out_bytes = o.size();
  if (o.size() > out_cap) return 3;
  if (!o.empty()) memcpy(out, o.data(), o.size());
  return 0;
}

// loc_candidate_key on its own: 1 and *key_out = the key of candidate k of the home voxel, 0 where the neighbour leaves |v| < 2^20
extern "C" int hostcheck_candidate_key(uint64_t home, int32_t k, uint64_t* key_out) {
  uint64_t key = 0;
  const bool ok = loc_candidate_key(home, k, key);
  *key_out = key;
  return ok ? 1 : 0;
}

#ifdef HOSTCHECK_LOCALIZE_MAIN
int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 1;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  fseek(f, 0, SEEK_END);
  const long size = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<char> in(size > 0 ? (size_t)size : 0), out;
  const bool ok = in.empty() || fread(in.data(), 1, in.size(), f) == in.size();
  fclose(f);
  if (!ok) return 2;
  const int rc = run_blob(in.data(), in.size(), out);
  if (rc) {
    fprintf(stderr, "hostcheck_localize: error %d\n", rc);
    return rc;
  }
  f = fopen(argv[2], "wb");
  if (!f) return 3;
  const bool wrote = out.empty() || fwrite(out.data(), 1, out.size(), f) == out.size();
  return fclose(f) == 0 && wrote ? 0 : 3;
}
#endif
