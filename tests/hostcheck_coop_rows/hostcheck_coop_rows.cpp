// hostcheck_coop_rows.cpp — TEST-ONLY stand-alone program (tests/test_coop_rows_hostcheck.py): the cooperative search of one
// query by a row of L lanes (reg_math.h: knn_coop_search_rows, what associate_knn_coop_kernel runs) in its host form — plain
// loops over L virtual lanes in place of the ballot, the lane read and the DPP row minimum — against the one-lane searches on
// the same GridDesc, table and points: knn_search_keyed (return code, the KM position slots) for every query and, where the keys
// decide, knn_search (the exact collector: count and positions).
//   hostcheck_coop_rows <case file> ...   a case file: int32 n_tgt, n_query, k, expect; double radius; n_tgt x 3 doubles;
//                                          n_query x 3 doubles (written by the test). expect: -1 / -2 = every query must return
//                                          that code, 0 = whatever the one-lane search returns
// The grid is the kernels' (grid_choose over the bounding box, the scan-pair cell cap). One line per case and L = 16, 32, 64:
//   name L k queries decided undecided not_applicable mismatches short_lists max_shells
// then the draws alone (knn_row_draw) on keys dealt to the lanes at random against one sorted list: "deal L ...", and the deal of
// list entries to workgroups, rows and turns: "entries <rows per wavefront> 0 deals deals 0 0 mismatches <deals with a second
// turn> <most turns>".
// Exit status 1 if any mismatch. Never linked into libloamx.so.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../loam_amd/csrc/reg_math.h"

using namespace loamx;

namespace {
struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
};

struct HostGrid {
  GridDesc g;
  std::vector<uint32_t> cell_start;
  std::vector<GridPoint> sp;
};

// the cell-sorted target set as the device builds lay it out (points of a cell by original index)
void build_grid(const std::vector<double>& pts, double max_dist, HostGrid& G) {
  const uint32_t n = (uint32_t)(pts.size() / 3);
  Vec3 lo = v3(pts[0], pts[1], pts[2]), hi = lo;
  for (uint32_t i = 0; i < n; i++) {
    const Vec3 p = v3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
    lo = v3(std::min(lo.x, p.x), std::min(lo.y, p.y), std::min(lo.z, p.z));
    hi = v3(std::max(hi.x, p.x), std::max(hi.y, p.y), std::max(hi.z, p.z));
  }
  grid_choose(G.g, lo, hi, n, max_dist, kGridCellsCap);
  const uint32_t ncell = (uint32_t)(G.g.nx * G.g.ny * G.g.nz);
  G.cell_start.assign(ncell + 1 + 4, 0);  // (+4 spare entries, as the device tables)
  std::vector<uint32_t> cell(n);
  for (uint32_t i = 0; i < n; i++) cell[i] = grid_cell_of_point(G.g, v3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2])), G.cell_start[cell[i] + 1]++;
  for (uint32_t c = 0; c < ncell; c++) G.cell_start[c + 1] += G.cell_start[c];
  for (uint32_t c = ncell + 1; c < ncell + 5; c++) G.cell_start[c] = n;
  std::vector<uint32_t> cursor(G.cell_start.begin(), G.cell_start.end() - 1);
  G.sp.assign((size_t)n + kGridPad, GridPoint{0, 0, 0, 0xFFFFFFFFu, 0});
  for (uint32_t k = 0; k < n; k++) G.sp[cursor[cell[k]]++] = GridPoint{pts[3 * k], pts[3 * k + 1], pts[3 * k + 2], k, 0};
}

struct Tally {
  unsigned long queries = 0, decided = 0, undecided = 0, na = 0, mismatches = 0, short_lists = 0;
  int max_shells = 0;
};

// the shells the cooperative search may walk for this query (its own arithmetic, repeated: the test wants to know that the
// later shells are reached)
int shells_of(const GridDesc& g, Vec3 q, double max_dist) {
  const int32_t cx = grid_cell_coord(q.x, g.ox, g.inv_h), cy = grid_cell_coord(q.y, g.oy, g.inv_h), cz = grid_cell_coord(q.z, g.oz, g.inv_h);
  const int32_t out = grid_outside_distance(g, cx, cy, cz);
  if (!(max_dist > 0.0)) return 0;
  return (int)(ceil(max_dist * g.inv_h) + 1.0 + (double)out);
}

template <int KM, int L>
void run_query(const HostGrid& G, Vec3 q, int k, double max_dist, double pass_max, int expect, Tally& T) {
  std::vector<uint32_t> rows(kLeanRowWords, 0u);  // (one lane's list, the size the kernel gives it)
  uint32_t want[KM], got[KM];
  const int want_kept = knn_search_keyed<KM>(G.g, G.cell_start.data(), G.sp.data(), q, k, max_dist, pass_max, want, rows.data(), 1);
  const int got_kept = knn_coop_search_rows<KM, L, L>(G.g, G.cell_start.data(), G.sp.data(), q, k, max_dist, pass_max, 0, got);
  T.queries++;
  if (expect < 0 && got_kept != expect) T.mismatches++;
  if (got_kept == -2) {  // not applicable: the kernel's caller runs the one-lane search
    T.na++;
    return;
  }
  if (got_kept != want_kept || memcmp(got, want, sizeof(got)) != 0) T.mismatches++;
  if (got_kept < 0) {
    T.undecided++;
    return;
  }
  T.decided++;
  const int kk = k < KM ? k : KM;
  if (got_kept < kk) T.short_lists++;
  const int s = shells_of(G.g, q, max_dist);
  if (s > T.max_shells) T.max_shells = s;
  KnnResult<KM> r;
  const int exact_kept = knn_search(G.g, G.cell_start.data(), G.sp.data(), q, kk, max_dist, r, rows.data(), 1);
  uint32_t shifted[KM];
  knn_shift_positions<KM>(r.pos, kk, shifted);  // neighbour j is slot (KM - k) + j
  if (exact_kept != got_kept) T.mismatches++;
  for (int j = 0; j < got_kept; j++)
    if (shifted[(KM - kk) + j] != got[(KM - kk) + j]) {
      T.mismatches++;
      break;
    }
}

template <int KM>
unsigned long run_case(const char* name, const HostGrid& G, const std::vector<double>& qs, int k, double max_dist, int expect) {
  const double pass_max = knn_radius_pass_max(max_dist);
  unsigned long bad = 0;
  for (int L : {16, 32, 64}) {
    Tally T;
    for (size_t i = 0; i < qs.size() / 3; i++) {
      const Vec3 q = v3(qs[3 * i], qs[3 * i + 1], qs[3 * i + 2]);
      if (L == 16) run_query<KM, 16>(G, q, k, max_dist, pass_max, expect, T);
      else if (L == 32) run_query<KM, 32>(G, q, k, max_dist, pass_max, expect, T);
      else run_query<KM, 64>(G, q, k, max_dist, pass_max, expect, T);
    }
    printf("%s %d %d %lu %lu %lu %lu %lu %lu %d\n", name, L, k, T.queries, T.decided, T.undecided, T.na, T.mismatches, T.short_lists, T.max_shells);
    bad += T.mismatches;
  }
  return bad;
}

bool read_case(const char* path, std::vector<double>& tgt, std::vector<double>& qs, int& k, int& expect, double& r) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  int32_t head[4];
  bool ok = fread(head, sizeof(int32_t), 4, f) == 4 && fread(&r, sizeof(double), 1, f) == 1 && head[0] > 0 && head[1] >= 0;
  if (ok) {
    tgt.resize((size_t)head[0] * 3), qs.resize((size_t)head[1] * 3);
    ok = fread(tgt.data(), sizeof(double), tgt.size(), f) == tgt.size() && fread(qs.data(), sizeof(double), qs.size(), f) == qs.size();
    k = head[2], expect = head[3];
  }
  fclose(f);
  return ok;
}

// ---- the draws alone: n keys with few distinct distances dealt to the L lanes at random; k + 1 draws against the sorted list
template <int KM, int L>
unsigned long deal_case(Rng& R) {
  Tally T;
  for (int rep = 0; rep < 4000; rep++) {
    const int k = 1 + (int)(R.next() % KM), n = (int)(R.next() % 41);  // 0 .. 40 candidates: fewer than k + 1 among them
    KnnKeys<KM> lanes[L];
    for (auto& l : lanes) knn_init(l, k, 64u);
    std::vector<double> all;
    for (int c = 0; c < n; c++) {
      const double key = knn_key_pack(0.25 * (double)(R.next() % 6), (uint32_t)c, lanes[0].mask, true);  // six distances: most keys tie but for their position
      knn_key_insert(lanes[rep % 3 == 0 ? c % L : (int)(R.next() % L)], key);  // (the kernel's deal, or any other)
      all.push_back(key);
    }
    std::sort(all.begin(), all.end());
    double last = -1.0;
    bool same = true;
    for (int t = 0; t <= k; t++) {
      last = knn_row_draw<KM, L, L>(lanes, last);
      same = same && last == (t < n ? all[t] : knn_key_empty());
    }
    T.queries++, T.decided++;
    if (n < k) T.short_lists++;
    if (!same) T.mismatches++;
  }
  printf("deal %d %d %lu %lu %lu %lu %lu %lu %d\n", L, KM, T.queries, T.decided, T.undecided, T.na, T.mismatches, T.short_lists, 0);
  return T.mismatches;
}

// ---- the kernel's deal of a pair's listed entries to workgroups, rows and turns (associate_knn_coop_kernel's loop, stepped with the
// kernel's own knn_coop_deal_first / knn_coop_deal_step): lists of 0 .. 700 entries with random reason bits over 1 .. 70 or 4 096
// workgroups of `rows` rows. Every entry must be taken exactly once: a wide or tied one by the whole wavefront of the workgroup
// whose turn holds it, a plain one by its row t mod (rows x workgroups), in turn t / (rows x workgroups).
unsigned long entry_deal_case(Rng& R, uint32_t rows) {
  Tally T;
  for (int rep = 0; rep < 4000; rep++) {
    const uint32_t listed = (uint32_t)(R.next() % 701), blocks = rep % 5 == 0 ? 4096u : 1u + (uint32_t)(R.next() % 70);
    std::vector<uint8_t> plain(listed), by_row(listed, 0), by_wave(listed, 0);
    for (auto& f : plain) f = R.next() % 3 != 0;
    bool ok = true;
    uint32_t max_turn = 0;
    for (uint32_t chunk = 0; chunk < blocks; chunk++) {
      uint32_t turn = 0;
      for (uint32_t t0 = knn_coop_deal_first(chunk, rows); t0 < listed; t0 += knn_coop_deal_step(blocks, rows), turn++) {
        for (uint32_t t = t0; t < t0 + rows && t < listed; t++)  // the turn's whole-wavefront entries
          if (!plain[t]) by_wave[t]++;
        for (uint32_t row = 0; row < rows; row++) {  // its rows
          const uint32_t t = t0 + row;
          if (t >= listed || !plain[t]) continue;
          by_row[t]++;
          ok = ok && t % (rows * blocks) == chunk * rows + row && t / (rows * blocks) == turn;
        }
        max_turn = turn > max_turn ? turn : max_turn;
      }
    }
    for (uint32_t t = 0; t < listed; t++) ok = ok && by_row[t] == (plain[t] ? 1 : 0) && by_wave[t] == (plain[t] ? 0 : 1);
    T.queries++, T.decided++;
    if (max_turn >= 1) T.short_lists++;  // (deals that reached a second turn)
    if ((int)max_turn + 1 > T.max_shells) T.max_shells = (int)max_turn + 1;
    if (!ok) T.mismatches++;
  }
  printf("entries %u 0 %lu %lu %lu %lu %lu %lu %d\n", rows, T.queries, T.decided, T.undecided, T.na, T.mismatches, T.short_lists, T.max_shells);
  return T.mismatches;
}
}  // namespace

int main(int argc, char** argv) {
  unsigned long bad = 0;
  for (int a = 1; a < argc; a++) {
    std::vector<double> tgt, qs;
    int k = 0, expect = 0;
    double r = 0.0;
    if (!read_case(argv[a], tgt, qs, k, expect, r)) {
      fprintf(stderr, "cannot read %s\n", argv[a]);
      return 2;
    }
    HostGrid G;
    build_grid(tgt, r, G);
    std::string name = argv[a];
    name = name.substr(name.find_last_of('/') + 1);
    name = name.substr(0, name.find_last_of('.'));
    if (k <= 5) bad += run_case<5>(name.c_str(), G, qs, k, r, expect);
    else if (k <= 8) bad += run_case<8>(name.c_str(), G, qs, k, r, expect);
    else bad += run_case<16>(name.c_str(), G, qs, k, r, expect);
  }
  Rng R{20241020};
  bad += deal_case<5, 16>(R) + deal_case<5, 32>(R) + deal_case<8, 16>(R) + deal_case<16, 32>(R);
  bad += entry_deal_case(R, 4) + entry_deal_case(R, 2);  // (rows of 16 lanes: four per wavefront; of 32: two)
  return bad ? 1 : 0;
}
