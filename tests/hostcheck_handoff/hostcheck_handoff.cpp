// hostcheck_handoff.cpp — TEST-ONLY stand-alone program (tests/test_handoff_hostcheck.py): the plane k-NN's round 1 split over two
// kernels — select without verification (knn_lean_round1<.., HANDOFF = 3>: the search-over threshold taken in front of the walk,
// positions and count word from the keys alone), then the checks on the gathered points (knn_handoff_verify, what fit_one runs) —
// against the one function of round 6 (knn_lean_round1 -> knn_lean_finish) and against a brute-force exact k-NN written here.
// Per query: undecided-or-not, kept and all positions must be equal between the two forms; a decided query must hold the
// brute-force answer. One line per case: name queries undecided_old undecided_new refused_by_verify mismatches brute_mismatches.
// Exit status 1 if any mismatch. Never linked into libloamx.so.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../loam_amd/csrc/reg_math.h"

using namespace loamx;

namespace {
constexpr int KM = 5;

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
};

struct HostGrid {
  GridDesc g;
  std::vector<uint32_t> cell_start;
  std::vector<GridPoint> sp;
  std::vector<float> rel;
};

// the cell-sorted target set with a GIVEN cell edge (origin = the bounding box's minimum), laid out as the device tables
void build_grid(const std::vector<Vec3>& pts, double h, HostGrid& G) {
  const uint32_t n = (uint32_t)pts.size();
  Vec3 lo = pts[0], hi = pts[0];
  for (const Vec3& p : pts) {
    lo = v3(std::min(lo.x, p.x), std::min(lo.y, p.y), std::min(lo.z, p.z));
    hi = v3(std::max(hi.x, p.x), std::max(hi.y, p.y), std::max(hi.z, p.z));
  }
  G.g.ox = lo.x, G.g.oy = lo.y, G.g.oz = lo.z, G.g.h = h, G.g.inv_h = 1.0 / h, G.g.n_points = n;
  G.g.nx = (int32_t)floor((hi.x - lo.x) / h) + 1, G.g.ny = (int32_t)floor((hi.y - lo.y) / h) + 1, G.g.nz = (int32_t)floor((hi.z - lo.z) / h) + 1;
  const uint32_t ncell = (uint32_t)(G.g.nx * G.g.ny * G.g.nz);
  G.cell_start.assign(ncell + 1 + 4, 0);  // (+4 spare entries, as the device tables)
  std::vector<uint32_t> cell(n);
  for (uint32_t i = 0; i < n; i++) cell[i] = grid_cell_of_point(G.g, pts[i]), G.cell_start[cell[i] + 1]++;
  for (uint32_t c = 0; c < ncell; c++) G.cell_start[c + 1] += G.cell_start[c];
  for (uint32_t c = ncell + 1; c < ncell + 5; c++) G.cell_start[c] = n;
  std::vector<uint32_t> cursor(G.cell_start.begin(), G.cell_start.end() - 1);
  G.sp.assign((size_t)n + kGridPad, GridPoint{0, 0, 0, 0xFFFFFFFFu, 0});
  for (uint32_t k = 0; k < n; k++) G.sp[cursor[cell[k]]++] = GridPoint{pts[k].x, pts[k].y, pts[k].z, k, 0};
  const size_t plane = G.sp.size();
  G.rel.assign(3 * plane, kRelPad);
  for (uint32_t p = 0; p < n; p++) {
    G.rel[p] = (float)(G.sp[p].x - G.g.ox), G.rel[plane + p] = (float)(G.sp[p].y - G.g.oy);
    G.rel[2 * plane + p] = (float)(G.sp[p].z - G.g.oz);
  }
}

struct Tally {
  unsigned long queries = 0, undecided_old = 0, undecided_new = 0, refused = 0, mismatches = 0, brute_mismatches = 0, short_lists = 0;
};

// exact k-NN over the whole set: the k smallest (d2, position), d2 as the kernels evaluate it; kept = the leading ones
// within the radius (sqrt(d2) < max_dist, kdtree.cpp:25). `unique` = the answer does not depend on how ties are broken.
int brute(const HostGrid& G, Vec3 q, int k, double max_dist, uint32_t pos[KM], bool* unique) {
  std::vector<std::pair<double, uint32_t>> all;
  for (uint32_t p = 0; p < G.g.n_points; p++) {
    const double dx = q.x - G.sp[p].x, dy = q.y - G.sp[p].y, dz = q.z - G.sp[p].z;
    all.push_back({dx * dx + dy * dy + dz * dz, p});
  }
  std::sort(all.begin(), all.end());
  int kept = 0;
  *unique = true;
  for (int j = 0; j < k && j < (int)all.size(); j++) {
    pos[j] = all[j].second;
    if (j + 1 < (int)all.size() && all[j].first == all[j + 1].first) *unique = false;
    if (kept == j && (!(max_dist > 0.0) || sqrt(all[j].first) < max_dist)) kept++;
  }
  return kept;
}

void run_query(const HostGrid& G, Vec3 q, int k, double max_dist, Tally& T) {
  const double pass_max = knn_radius_pass_max(max_dist);
  const uint32_t plane = (uint32_t)G.sp.size();
  uint32_t rows_old[kLeanRowWords] = {}, rows_new[kLeanRowWords] = {};
  uint32_t pos_old[KM], pos_new[KM], word = 0;
  const int old_r = knn_lean_round1<KM>(G.g, G.cell_start.data(), G.sp.data(), G.rel.data(), plane, q, k, max_dist, pass_max, pos_old, rows_old, 1);
  int new_r = knn_lean_round1<KM, KnnSameQuery, 3>(G.g, G.cell_start.data(), G.sp.data(), G.rel.data(), plane, q, k, max_dist, pass_max, pos_new,
                                                   rows_new, 1, KnnSameQuery(), &word);
  if (new_r >= 0 && word != 0u) {  // the fit's side: gather the neighbours from the positions (fit_one), verify
    const int shift = KM - (k < KM ? k : KM);
    GridPoint nb[KM];
    for (int j = 0; j < KM; j++) {
      const uint32_t at = shift + j < KM ? pos_new[shift + j] : 0u;
      nb[j] = G.sp[at < plane ? at : 0u];
    }
    new_r = knn_handoff_verify<KM>(word, q, nb, k, pass_max, knn_f32_err_unit(G.g));
    if (new_r < 0) T.refused++;
  }
  T.queries++;
  T.undecided_old += old_r < 0, T.undecided_new += new_r < 0;
  bool same = (old_r < 0) == (new_r < 0);
  if (same && old_r >= 0) {
    same = old_r == new_r;
    for (int j = 0; j < KM; j++) same = same && pos_old[j] == pos_new[j];
    uint32_t bpos[KM];
    bool unique;
    const int bk = brute(G, q, k, max_dist, bpos, &unique);
    const int shift = KM - (k < KM ? k : KM);
    bool ok = unique ? bk == new_r : true;
    for (int j = 0; ok && unique && j < new_r; j++) ok = bpos[j] == pos_new[shift + j];
    if (!unique) ok = false;  // a decided query never has an exact tie among its k + 1 nearest
    if (!ok) T.brute_mismatches++;
    if (G.g.n_points >= (uint32_t)k && new_r < k) T.short_lists++;
  }
  if (!same) T.mismatches++;
}

void report(const char* name, const Tally& T) {
  printf("%s %lu %lu %lu %lu %lu %lu %lu\n", name, T.queries, T.undecided_old, T.undecided_new, T.refused, T.mismatches, T.brute_mismatches,
         T.short_lists);
}

std::vector<Vec3> random_box(Rng& R, uint32_t n, double edge) {
  std::vector<Vec3> pts(n);
  for (Vec3& p : pts) p = v3(edge * R.uni(), edge * R.uni(), edge * R.uni());
  return pts;
}
}  // namespace

int main(int argc, char** argv) {
  // sizes: n_a points in a box of edge_a metres, n_b in one of edge_b, cell `cell`. (600 points in the 4 m box are 9 per cubic
  // metre: the fifth neighbour is 0.5 m away, as far as the block's faces, and round 1 queues 28 % of the queries whatever its
  // form; in a 2 m box they have the 5 000-point set's density.)
  const uint32_t n_a = argc > 1 ? (uint32_t)atoi(argv[1]) : 600u, n_b = argc > 2 ? (uint32_t)atoi(argv[2]) : 5000u;
  const double edge_a = argc > 3 ? atof(argv[3]) : 2.0, edge_b = argc > 4 ? atof(argv[4]) : 4.0, cell = argc > 5 ? atof(argv[5]) : 0.5;
  const double max_dist = 4.0 * cell;  // (the scan-pair grids: a cell is a quarter of the radius)
  unsigned long bad = 0;
  Rng R{20240711};
  for (int which = 0; which < 2; which++) {  // ---- random sets, queries all over the box
    const double edge = which ? edge_b : edge_a;
    HostGrid G;
    build_grid(random_box(R, which ? n_b : n_a, edge), cell, G);
    Tally T;
    for (int i = 0; i < 2000; i++) run_query(G, v3(edge * R.uni(), edge * R.uni(), edge * R.uni()), 5, max_dist, T);
    report(which ? "random_b" : "random_a", T);
    bad += T.mismatches + T.brute_mismatches;
    Tally C;  // ---- queries in the corner cells and outside the grid (up to three cells off: out = 1 is searched, beyond is queued or empty)
    for (int i = 0; i < 1500; i++) {
      double c[3];
      for (double& v : c) {
        const int side = (int)(R.next() % 3);
        const double off = (R.uni() * 3.5 - 3.0) * cell;  // -3 .. +0.5 cells from the face
        v = side == 0 ? -off : (side == 1 ? edge + off : edge * R.uni());
      }
      run_query(G, v3(c[0], c[1], c[2]), 5, (i & 1) ? max_dist : 0.0, C);
    }
    report(which ? "corners_b" : "corners_a", C);
    bad += C.mismatches + C.brute_mismatches;
  }
  {  // ---- fewer than five points in range: a sparse set, and radii below the neighbours' distances
    HostGrid G;
    build_grid(random_box(R, 40, edge_b), cell, G);
    Tally T;
    for (int i = 0; i < 2000; i++) run_query(G, v3(edge_b * R.uni(), edge_b * R.uni(), edge_b * R.uni()), 5, (i % 3 == 0) ? 0.6 * cell : max_dist, T);
    report("sparse", T);
    bad += T.mismatches + T.brute_mismatches;
    HostGrid G3;  // (a set of three points)
    build_grid(random_box(R, 3, 0.4), cell, G3);
    Tally T3;
    for (int i = 0; i < 200; i++) run_query(G3, v3(0.4 * R.uni(), 0.4 * R.uni(), 0.4 * R.uni()), 5, (i & 1) ? max_dist : 0.0, T3);
    report("three_points", T3);
    bad += T3.mismatches + T3.brute_mismatches;
  }
  {  // ---- the lattice: 9 x 9 x 8 points at 0.1 m, queries on lattice points, on the midpoints of its edges (exact ties) and a
     // millimetre off lattice points (FP32 keys that differ by a few units of their resolution: some decided, some not)
    std::vector<Vec3> pts;
    for (int z = 0; z < 8; z++)
      for (int y = 0; y < 9; y++)
        for (int x = 0; x < 9; x++) pts.push_back(v3(0.1 * x, 0.1 * y, 0.1 * z));
    HostGrid G;
    build_grid(pts, 0.25, G);
    Tally T;
    for (size_t i = 0; i < pts.size(); i++) {
      run_query(G, pts[i], 5, 1.0, T);
      run_query(G, v3(pts[i].x + 0.05, pts[i].y, pts[i].z), 5, 1.0, T);
      if (i % 2 == 0) run_query(G, v3(pts[i].x + 1e-3 * R.uni(), pts[i].y + 1e-3 * R.uni(), pts[i].z + 1e-3 * R.uni()), 5, 1.0, T);
    }
    report("lattice", T);
    bad += T.mismatches + T.brute_mismatches;
  }
  return bad ? 1 : 0;
}
