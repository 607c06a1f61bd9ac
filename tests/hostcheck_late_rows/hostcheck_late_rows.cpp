// hostcheck_late_rows.cpp — TEST-ONLY stand-alone program (tests/test_late_rows_hostcheck.py): the exact search of one query by a
// row of 16 lanes (reg_math.h: knn_exact_block_row16, what associate_fit_late_kernel runs) in its host form — a plain loop over 16
// virtual lanes in place of the DPP row minimum — against the one-lane search it replaces (knn_search). Per query: where the row
// decides, kept and the KnnResult (the k slots: distances bit for bit, positions, original indices; worst, count) must be knn_search's;
// where it does not, the reason must be one of the three it may give (the search goes on beyond the block, starts away from the
// query's cell, or the block holds more than kRow16Cap candidates). Then the selection step alone (knn_row16_select) on
// candidate lists dealt to the lanes at random against one list that saw them all.
// One line per case: name queries decided fallback_far fallback_guard fallback_cap mismatches short_lists max_block.
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
};

// the cell-sorted target set with a GIVEN cell edge (origin = the bounding box's minimum), laid out as the device tables; points
// of one cell in the order `order` gives them (the device's builds leave that order to their atomics)
void build_grid(const std::vector<Vec3>& pts, double h, HostGrid& G, Rng* shuffle = nullptr) {
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
  std::vector<uint32_t> cell(n), order(n);
  for (uint32_t i = 0; i < n; i++) cell[i] = grid_cell_of_point(G.g, pts[i]), G.cell_start[cell[i] + 1]++, order[i] = i;
  if (shuffle)
    for (uint32_t i = n; i > 1; i--) std::swap(order[i - 1], order[shuffle->next() % i]);
  for (uint32_t c = 0; c < ncell; c++) G.cell_start[c + 1] += G.cell_start[c];
  for (uint32_t c = ncell + 1; c < ncell + 5; c++) G.cell_start[c] = n;
  std::vector<uint32_t> cursor(G.cell_start.begin(), G.cell_start.end() - 1);
  G.sp.assign((size_t)n + kGridPad, GridPoint{0, 0, 0, 0xFFFFFFFFu, 0});
  for (uint32_t k : order) G.sp[cursor[cell[k]]++] = GridPoint{pts[k].x, pts[k].y, pts[k].z, k, 0};
}

struct Tally {
  unsigned long queries = 0, decided = 0, far = 0, guard = 0, cap = 0, mismatches = 0, short_lists = 0, max_block = 0;
};

// the k slots of the result (knn_insert keeps KM slots whatever k is: what lies behind the k-th depends on the order the candidates
// came in, and nothing reads it — knn_finish, knn_done and knn_shift_positions stop at k), worst and count
bool same_result(const KnnResult<KM>& a, const KnnResult<KM>& b, int k) {
  return memcmp(a.d2, b.d2, k * sizeof(double)) == 0 && memcmp(a.pos, b.pos, k * sizeof(uint32_t)) == 0 &&
         memcmp(a.orig, b.orig, k * sizeof(uint32_t)) == 0 && memcmp(&a.worst, &b.worst, sizeof(double)) == 0 && a.count == b.count;
}

// points in the 3x3x3 block of the query's cell (clamped to the grid), counted here from the table
uint32_t block_population(const HostGrid& G, Vec3 q) {
  const GridDesc& g = G.g;
  const int32_t cx = grid_cell_coord(q.x, g.ox, g.inv_h), cy = grid_cell_coord(q.y, g.oy, g.inv_h), cz = grid_cell_coord(q.z, g.oz, g.inv_h);
  uint32_t pop = 0;
  for (int32_t iz = cz - 1; iz <= cz + 1; iz++)
    for (int32_t iy = cy - 1; iy <= cy + 1; iy++)
      for (int32_t ix = cx - 1; ix <= cx + 1; ix++)
        if (ix >= 0 && ix < g.nx && iy >= 0 && iy < g.ny && iz >= 0 && iz < g.nz) {
          const uint32_t c = (uint32_t)((iz * g.ny + iy) * g.nx + ix);
          pop += G.cell_start[c + 1] - G.cell_start[c];
        }
  return pop;
}

void run_query(const HostGrid& G, Vec3 q, int k, double max_dist, Tally& T) {
  uint32_t rows[18] = {};
  KnnResult<KM> want, got;
  const int want_kept = knn_search(G.g, G.cell_start.data(), G.sp.data(), q, k, max_dist, want, rows, 1);
  int got_kept = -1;
  const bool decided = knn_exact_block_row16<KM, kRow16Lanes>(G.g, G.cell_start.data(), G.sp.data(), q, k, max_dist, 0, got, got_kept);
  T.queries++;
  const GridDesc& g = G.g;
  const int32_t cx = grid_cell_coord(q.x, g.ox, g.inv_h), cy = grid_cell_coord(q.y, g.oy, g.inv_h), cz = grid_cell_coord(q.z, g.oz, g.inv_h);
  const int32_t out = grid_outside_distance(g, cx, cy, cz);
  const uint32_t pop = block_population(G, q);
  if (decided) {
    T.decided++;
    if (pop > T.max_block && out <= 1) T.max_block = pop;
    if (got_kept != want_kept || !same_result(got, want, k)) T.mismatches++;
    if (pop > kRow16Cap && !(max_dist > 0.0)) T.mismatches++;  // (no radius: no row is left out, the whole block counts against the capacity)
    if (want_kept < k) T.short_lists++;
  } else {
    // one of the three reasons, told apart here: away from the grid; more candidates than the row holds; or a block that does not
    // prove its list — which the one-lane search's own test says of the block's k best (it then went on to shell 2)
    if (out > 1) T.far++;
    else if (pop > kRow16Cap) T.cap++;
    else {
      T.guard++;
      // the k best of the block alone, by a search over a radius-free copy of the test: the one-lane search was not done at w = 1
      KnnResult<KM> blk;
      knn_init(blk);
      knn_round1(g, G.cell_start.data(), G.sp.data(), q, k, knn_radius_bound(max_dist), cx, cy, cz, blk, rows, 1);
      if (knn_done(g, q, k, max_dist, cx, cy, cz, blk, 1)) T.mismatches++;  // the block did decide: no reason to refuse
    }
    if (got_kept != 0) T.mismatches++;
  }
}

void report(const char* name, const Tally& T) {
  printf("%s %lu %lu %lu %lu %lu %lu %lu %lu\n", name, T.queries, T.decided, T.far, T.guard, T.cap, T.mismatches, T.short_lists, T.max_block);
}

std::vector<Vec3> random_box(Rng& R, uint32_t n, double ex, double ey, double ez) {
  std::vector<Vec3> pts(n);
  for (Vec3& p : pts) p = v3(ex * R.uni(), ey * R.uni(), ez * R.uni());
  return pts;
}

// ---- the selection step alone: n candidates with few distinct distances (ties) dealt to the 16 lanes at random
unsigned long deal_case(Rng& R, Tally& T) {
  unsigned long bad = 0;
  for (int rep = 0; rep < 4000; rep++) {
    const int k = 1 + (int)(R.next() % KM), n = (int)(R.next() % 41);  // 0 .. 40 candidates: fewer than k among them
    KnnResult<KM> lanes[kRow16Lanes], one, out;
    for (auto& l : lanes) knn_init(l);
    knn_init(one);
    std::vector<uint32_t> origs(n);
    for (int c = 0; c < n; c++) origs[c] = (uint32_t)c * 7u + 3u;
    for (int c = n; c > 1; c--) std::swap(origs[c - 1], origs[R.next() % c]);
    for (int c = 0; c < n; c++) {
      const double d2 = 0.25 * (double)(R.next() % 6);  // six distinct distances: most candidates tie with others
      const uint32_t pos = 1000u + (uint32_t)c;
      KnnResult<KM>& l = lanes[rep % 3 == 0 ? c % kRow16Lanes : (int)(R.next() % kRow16Lanes)];  // (the kernel's deal, or any other)
      if (d2 <= l.worst) knn_insert(l, k, d2, pos, origs[c]);
      if (d2 <= one.worst) knn_insert(one, k, d2, pos, origs[c]);
    }
    knn_row16_select<KM, kRow16Lanes>(lanes, k, out);
    T.queries++, T.decided++;
    if (n < k) T.short_lists++;
    if (!same_result(out, one, k)) T.mismatches++, bad++;
  }
  return bad;
}
}  // namespace

int main() {
  const double cell = 0.5, max_dist = 4.0 * cell;  // (the scan-pair grids: a cell is a quarter of the radius)
  unsigned long bad = 0;
  Rng R{20240913};
  const auto add = [&](const char* name, const Tally& T) { report(name, T), bad += T.mismatches; };
  for (int which = 0; which < 2; which++) {  // ---- random sets: 450 points in a 2 m box, 3 000 in a 4 m box (~50 / m^3: 160 - 190 in a 3x3x3 block); k = 1 .. 5
    const double edge = which ? 4.0 : 2.0;
    HostGrid G;
    build_grid(random_box(R, which ? 3000u : 450u, edge, edge, edge), cell, G, &R);
    Tally T;
    for (int i = 0; i < 2500; i++) run_query(G, v3(edge * R.uni(), edge * R.uni(), edge * R.uni()), 1 + i % 5, (i % 7 == 0) ? 0.0 : max_dist, T);
    add(which ? "random_b" : "random_a", T);
    Tally C;  // ---- queries in the corner cells and outside the grid (up to three cells off: one cell off is searched, beyond is not the row's)
    for (int i = 0; i < 1500; i++) {
      double c[3];
      for (double& v : c) {
        const int side = (int)(R.next() % 3);
        const double off = (R.uni() * 3.5 - 3.0) * cell;  // -3 .. +0.5 cells from the face
        v = side == 0 ? -off : (side == 1 ? edge + off : edge * R.uni());
      }
      run_query(G, v3(c[0], c[1], c[2]), 1 + i % 5, (i & 1) ? max_dist : 0.0, C);
    }
    add(which ? "corners_b" : "corners_a", C);
  }
  {  // ---- fewer than five points in range: a sparse set, radii below the neighbours' distances, a set of three points
    HostGrid G;
    build_grid(random_box(R, 40, 4.0, 4.0, 4.0), cell, G);
    Tally T;
    for (int i = 0; i < 2000; i++) run_query(G, v3(4.0 * R.uni(), 4.0 * R.uni(), 4.0 * R.uni()), 5, (i % 3 == 0) ? 0.6 * cell : max_dist, T);
    add("sparse", T);
    HostGrid D;  // (a dense set under radii that keep 0 .. 5 of the five nearest: the radius filter's prefix)
    build_grid(random_box(R, 5000, 4.0, 4.0, 4.0), cell, D);
    Tally Tr;
    for (int i = 0; i < 2000; i++) run_query(D, v3(4.0 * R.uni(), 4.0 * R.uni(), 4.0 * R.uni()), 5, 0.04 + 0.12 * R.uni(), Tr);
    add("radius", Tr);
    HostGrid G3;
    build_grid(random_box(R, 3, 0.4, 0.4, 0.4), cell, G3);
    Tally T3;
    for (int i = 0; i < 200; i++) run_query(G3, v3(0.4 * R.uni(), 0.4 * R.uni(), 0.4 * R.uni()), 1 + i % 5, (i & 1) ? max_dist : 0.0, T3);
    add("three_points", T3);
  }
  {  // ---- a coplanar set (nz = 1)
    std::vector<Vec3> pts = random_box(R, 1500, 6.0, 4.0, 0.0);
    HostGrid G;
    build_grid(pts, cell, G, &R);
    Tally T;
    for (int i = 0; i < 1500; i++) run_query(G, v3(6.0 * R.uni(), 4.0 * R.uni(), (R.uni() - 0.5) * 0.8), 1 + i % 5, (i & 1) ? max_dist : 0.0, T);
    add("flat", T);
  }
  {  // ---- exact ties: the 9 x 9 x 8 lattice at 0.125 m (every squared distance exact), queries on lattice points (six equidistant
     // neighbours), on edge midpoints and face centres; the cell order shuffled so that (d2, orig) and not the storage order decides
    std::vector<Vec3> pts;
    for (int z = 0; z < 8; z++)
      for (int y = 0; y < 9; y++)
        for (int x = 0; x < 9; x++) pts.push_back(v3(0.125 * x, 0.125 * y, 0.125 * z));
    HostGrid G;
    build_grid(pts, 0.25, G, &R);
    Tally T;
    for (size_t i = 0; i < pts.size(); i++) {
      run_query(G, pts[i], 1 + (int)(i % 5), 1.0, T);
      run_query(G, v3(pts[i].x + 0.0625, pts[i].y, pts[i].z), 5, 1.0, T);
      run_query(G, v3(pts[i].x + 0.0625, pts[i].y + 0.0625, pts[i].z), 5, (i & 1) ? 1.0 : 0.0, T);
    }
    add("lattice", T);
  }
  {  // ---- duplicated target points: every point of a random set three times over (distance ties that only orig orders)
    std::vector<Vec3> base = random_box(R, 500, 3.0, 3.0, 3.0), pts;
    for (int rep = 0; rep < 3; rep++) pts.insert(pts.end(), base.begin(), base.end());
    HostGrid G;
    build_grid(pts, cell, G, &R);
    Tally T;
    for (int i = 0; i < 1500; i++) run_query(G, i % 4 == 0 ? base[R.next() % base.size()] : v3(3.0 * R.uni(), 3.0 * R.uni(), 3.0 * R.uni()), 1 + i % 5, max_dist, T);
    add("duplicates", T);
  }
  for (int which = 0; which < 2; which++) {  // ---- one crowded cell: 252 points (the row holds them) and 300 (it does not)
    const uint32_t n = which ? 300u : 252u;
    std::vector<Vec3> pts = random_box(R, n, 0.1, 0.1, 0.1);
    for (Vec3& p : pts) p = v3(p.x + 3.2, p.y + 3.2, p.z + 3.2);
    pts.push_back(v3(0, 0, 0)), pts.push_back(v3(6.4, 6.4, 6.4));  // (the box: 13^3 cells of 0.5 m, the cluster inside one of them)
    HostGrid G;
    build_grid(pts, cell, G, &R);
    Tally T;
    for (int i = 0; i < 300; i++) run_query(G, v3(3.2 + 0.1 * R.uni(), 3.2 + 0.1 * R.uni(), 3.2 + 0.1 * R.uni()), 1 + i % 5, max_dist, T);
    add(which ? "crowded_300" : "crowded_252", T);
  }
  {
    Tally T;
    deal_case(R, T);
    add("deal", T);
  }
  return bad ? 1 : 0;
}
