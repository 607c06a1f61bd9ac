// api_index.hip — the persistent target index (a map that outlives the calls) and its upkeep: insert, voxel-filtered insert,
// crop, read-back.
#include "api_host.h"
#include "map_math.h"

using namespace loamx;

/* ---- persistent target index ---------------------------------------------------------------------------- */
namespace {
void index_free(loamx_target_index* idx) {
  for (int k = 0; k < 2; k++) {
    if (idx->desc[k]) (void)hipFree(idx->desc[k]);
    if (idx->cells[k]) (void)hipFree(idx->cells[k]);
    if (idx->sorted[k]) (void)hipFree(idx->sorted[k]);
    if (idx->rel[k]) (void)hipFree(idx->rel[k]);
    if (idx->pts[k]) (void)hipFree(idx->pts[k]);
    if (idx->sorted2[k]) (void)hipFree(idx->sorted2[k]);
    if (idx->rel2[k]) (void)hipFree(idx->rel2[k]);
  }
  for (int k = 0; k < 2; k++) {
    if (idx->vox[k].keys) (void)hipFree(idx->vox[k].keys);
    if (idx->vox[k].owner) (void)hipFree(idx->vox[k].owner);
  }
  if (idx->counts) (void)hipFree(idx->counts);
  if (idx->scratch) (void)hipFree(idx->scratch);
  delete idx;
}

// Makes room for `extra` more points of kind k (amortised doubling; the old points are copied over on the device).
int index_reserve(loamx_ctx* ctx, loamx_target_index* idx, int k, size_t extra) {
  const size_t need = idx->n[k] + extra;
  if (need <= idx->cap[k] && idx->pts[k]) return LOAMX_OK;
  size_t cap = idx->cap[k] ? idx->cap[k] : 1;
  while (cap < need) cap *= 2;
  if (idx->cap[k] == 0) cap = need ? need : 1;  // the first build is sized exactly
  double* pts = nullptr;
  GridPoint* sorted = nullptr;
  float* rel = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&pts), cap * 24) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&sorted), (cap + kGridPad) * sizeof(GridPoint)) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&rel), 3 * (cap + kGridPad) * sizeof(float)) != hipSuccess) {
    if (pts) (void)hipFree(pts);
    if (sorted) (void)hipFree(sorted);
    if (rel) (void)hipFree(rel);
    return fail(ctx, LOAMX_ERR_HIP, "hipMalloc failed for the target index");
  }
  if (idx->pts[k] && idx->n[k])
    HIP_TRY(ctx, hipMemcpyAsync(pts, idx->pts[k], idx->n[k] * 24, hipMemcpyDeviceToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (idx->pts[k]) (void)hipFree(idx->pts[k]);
  if (idx->sorted[k]) (void)hipFree(idx->sorted[k]);
  if (idx->rel[k]) (void)hipFree(idx->rel[k]);
  if (idx->sorted2[k]) (void)hipFree(idx->sorted2[k]);  // (the twins are made again, at the new capacity, by the next merge)
  if (idx->rel2[k]) (void)hipFree(idx->rel2[k]);
  idx->sorted2[k] = nullptr, idx->rel2[k] = nullptr;
  idx->pts[k] = pts, idx->sorted[k] = sorted, idx->rel[k] = rel, idx->cap[k] = cap;
  idx->n_at_build[k] = 0, idx->grid_valid[k] = false;  // (the cell-sorted arrays are gone: this kind is rebuilt)
  return LOAMX_OK;
}

// (Re)builds the grids of the kinds in `kinds` (bit 0 edge, bit 1 planar) from idx->pts: cell edge, dimensions and order
// chosen afresh for the set as it is now.
int index_build(loamx_ctx* ctx, loamx_target_index* idx, unsigned kinds = 3u) {
  hipStream_t s = ctx->stream;
  const uint32_t counts[2] = {(uint32_t)idx->n[0], (uint32_t)idx->n[1]};
  HIP_TRY(ctx, hipMemcpyAsync(idx->counts, counts, sizeof(counts), hipMemcpyHostToDevice, s));
  RegConfig C{};
  C.flags = ctx->reg_flags;
  RegBatch B{};
  B.n_pairs = 1, B.in_pitch = 1;
  for (int k = 0; k < 2; k++) {
    C.kind[k].r = idx->radius[k];
    B.kind[k].stride = idx->cap[k], B.kind[k].tgt = idx->pts[k], B.kind[k].n_tgt = idx->counts + k;
  }
  // map-sized sets get a cell table of up to kGridMapCellsCap entries (the scan-sized table of 65 536 would put
  // hundreds of points of a million-point map into every cell); tables and cursors grow with the set
  size_t scratch_need = kGridBigScratchBytes;
  for (int k = 0; k < 2; k++) {
    if (!(kinds & (1u << k))) continue;
    const int mc = ctx->map_cells_log2;  // experiment knob (16 = the scan-sized table)
    // default: about one table entry per two points, between 2^18 and 2^22 (measured on a 1.02 M-point map, registration of
    // a 128 x 2048 scan: 2^17 6.22, 2^18 6.10, 2^19 5.23, 2^20 6.04, 2^21 6.88 ms — finer cells shorten the candidate
    // streams of the dense cells near the sensor, coarser ones keep k points inside the 3x3x3 block)
    uint32_t dflt = kGridMapCellsCap;
    while (dflt < (1u << 22) && (size_t)dflt * 2 < idx->n[k]) dflt <<= 1;
    idx->cells_cap[k] = idx->n[k] > 200000 ? (mc >= 8 && mc <= 24 ? (1u << mc) : dflt) : 0u;
    if (idx->cells_cap[k] <= kGridCellsCap) idx->cells_cap[k] = 0u;
    const size_t cap = idx->cells_cap[k] ? idx->cells_cap[k] : kGridCellsCap;
    const size_t need = (cap + 1 + 4) * sizeof(uint32_t);  // (+4: the search reads four entries at a time)
    if (idx->cells_alloc[k] < need) {
      HIP_TRY(ctx, hipStreamSynchronize(s));
      if (idx->cells[k]) (void)hipFree(idx->cells[k]);
      idx->cells[k] = nullptr, idx->cells_alloc[k] = 0;
      HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&idx->cells[k]), need));
      idx->cells_alloc[k] = need;
    }
    if (64 + (cap + cap / 4096 + 8) * sizeof(uint32_t) > scratch_need) scratch_need = 64 + (cap + cap / 4096 + 8) * sizeof(uint32_t);  // (box keys, cursors, tile sums)
  }
  if (idx->scratch_alloc < scratch_need) {
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if (idx->scratch) (void)hipFree(idx->scratch);
    idx->scratch = nullptr, idx->scratch_alloc = 0;
    HIP_TRY(ctx, hipMalloc(&idx->scratch, scratch_need));
    idx->scratch_alloc = scratch_need;
  }
  B.sort_scratch = static_cast<GridPoint*>(idx->scratch);
  for (int k = 0; k < 2; k++)
    B.kind[k].grid = index_grid_set(idx, k);
  untimed(ctx);
  GridBuildForm form[2] = {{kGridBuildNone, 0u, 0u}, {kGridBuildNone, 0u, 0u}};
  {
    TimedScope t(ctx, LOAMX_K_GRID, 0.0);
    for (int k = 0; k < 2; k++)
      if (kinds & (1u << k)) form[k] = launch_grid_build_target(B, C, k, s);
  }
  int rc = check_launch(ctx, "grid_build_kernel");
  if (rc != LOAMX_OK) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(s));
  for (int k = 0; k < 2; k++)
    if (kinds & (1u << k)) {
      idx->n_at_build[k] = idx->n[k], idx->grid_valid[k] = true, idx->full_builds++;
      idx->build_form[k] = form[k], idx->table_valid[k] = idx->n[k] >= form[k].table_min_points;
      idx->last_op[k] = LOAMX_INDEX_OP_FULL_BUILD, idx->kind_builds[k]++;
    }
  return LOAMX_OK;
}

// May kind k take `add` more points by a merge into its existing grid (index_insert_* kernels)? Map-sized sets only (a
// scan-sized set is rebuilt by one workgroup in ~0.1 ms), while the set has not doubled since its grid was chosen (the
// cell edge follows the density) and stays on the same side of the map-table threshold.
bool index_can_merge(const loamx_target_index* idx, int k, size_t add) {
  const size_t n_old = idx->n[k], n_new = n_old + add;
  return idx->n_at_build[k] > kGridSmallCap && n_old >= idx->n_at_build[k] && n_new <= 2 * idx->n_at_build[k] && n_new <= idx->cap[k] &&
         (n_new > 200000) == (idx->cells_cap[k] != 0u);
}

// First half of an insert: the new points go to a staging buffer (stage[k]: device pointers) and are looked at there
// (loamx.h: "Non-finite input"): a refused insert must leave the index as it was, and making room (index_reserve) already
// re-allocates its arrays.
int index_stage(loamx_ctx* ctx, const loamx_target_index* idx, const double* const host[2], const size_t add[2], double* stage[2]) {
  for (int k = 0; k < 2; k++) {
    if (idx->n[k] + add[k] > 0x0FFFFFFFull) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "feature set too large");
    if (add[k] && !host[k]) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null point array");
  }
  hipStream_t s = ctx->stream;
  ENSURE(ctx, WS_FIT_IN, (add[0] + add[1] ? add[0] + add[1] : 1) * 24);
  stage[0] = wsp<double>(ctx, WS_FIT_IN), stage[1] = wsp<double>(ctx, WS_FIT_IN) + add[0] * 3;
  for (int k = 0; k < 2; k++)
    if (add[k]) HIP_TRY(ctx, hipMemcpyAsync(stage[k], host[k], add[k] * 24, hipMemcpyHostToDevice, s));
  int rc = finite_begin(ctx);
  if (rc != LOAMX_OK) return rc;
  for (int k = 0; k < 2; k++) finite_add(ctx, stage[k], false, nullptr, 1, add[k], 1);
  return finite_end(ctx);
}

// Second half: appends add[k] staged DEVICE points (finite, at most 0x0FFFFFFF with the set) to each kind — the uploaded
// points of the plain insert, or what the voxel filter kept of them.
int index_append_staged(loamx_ctx* ctx, loamx_target_index* idx, const double* const stage[2], const size_t add[2]) {
  hipStream_t s = ctx->stream;
  for (int k = 0; k < 2; k++) {  // all the room first: a failed allocation leaves the index as it was
    int rc = index_reserve(ctx, idx, k, add[k]);
    if (rc != LOAMX_OK) return rc;
  }
  const size_t n_old[2] = {idx->n[0], idx->n[1]};
  unsigned rebuild = 0u;
  bool merge[2] = {false, false};
  for (int k = 0; k < 2; k++)  // the new points behind the sets
    if (add[k]) HIP_TRY(ctx, hipMemcpyAsync(idx->pts[k] + idx->n[k] * 3, stage[k], add[k] * 24, hipMemcpyDeviceToDevice, s));
  for (int k = 0; k < 2; k++) {
    merge[k] = add[k] != 0 && index_can_merge(idx, k, add[k]);
    // a kind that receives nothing keeps its grid — also one grown by merges since its last full build (the size
    // at the last full build was compared here, and an edge-only insert re-sorted a million-point planar map)
    if (!merge[k] && (add[k] != 0 || !idx->grid_valid[k])) rebuild |= 1u << k;
    // (from here on the grid no longer describes the set — n has grown — until the build or the merge below has
    // succeeded; a failure in between must leave the flag down, so that the next insert rebuilds)
    if (add[k] != 0) idx->grid_valid[k] = false;
    idx->n[k] += add[k];
  }
  // ---- merges: count the new points per cell (and learn whether they all lie inside the grid), then move + scatter
  uint32_t* ws[2] = {nullptr, nullptr};
  for (int k = 0; k < 2; k++) {
    if (!merge[k]) continue;
    const size_t cells = idx->cells_cap[k] ? idx->cells_cap[k] : kGridCellsCap;
    const size_t need = index_insert_ws_bytes(cells, add[k]);
    // (the two kinds share idx->scratch: the planar kind's part sits behind the edge kind's)
    const size_t off = k == 1 && merge[0] ? ((index_insert_ws_bytes(idx->cells_cap[0] ? idx->cells_cap[0] : kGridCellsCap, add[0]) + 255) & ~(size_t)255) : 0;
    if (idx->scratch_alloc < off + need) {
      HIP_TRY(ctx, hipStreamSynchronize(s));
      void* bigger = nullptr;
      HIP_TRY(ctx, hipMalloc(&bigger, 2 * (off + need)));
      if (idx->scratch) (void)hipFree(idx->scratch);
      idx->scratch = bigger, idx->scratch_alloc = 2 * (off + need);
      if (k == 1 && merge[0]) {  // (the edge kind's counts were in the old block: once more)
        const GridSet gs0 = index_grid_set(idx, 0);
        ws[0] = static_cast<uint32_t*>(idx->scratch);
        launch_index_insert_count(gs0, idx->cells_cap[0] ? idx->cells_cap[0] : kGridCellsCap, idx->pts[0] + n_old[0] * 3, (uint32_t)add[0], ws[0], s);
      }
    }
    ws[k] = reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(idx->scratch) + off);
    const GridSet gs = index_grid_set(idx, k);
    untimed(ctx);
    launch_index_insert_count(gs, cells, idx->pts[k] + n_old[k] * 3, (uint32_t)add[k], ws[k], s);
  }
  for (int k = 0; k < 2; k++) {
    if (!merge[k]) continue;
    HIP_TRY(ctx, hipMemcpyAsync(&ctx->h_pinned[32 + k], ws[k], sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  }
  if (merge[0] || merge[1]) HIP_TRY(ctx, hipStreamSynchronize(s));
  for (int k = 0; k < 2; k++) {
    if (!merge[k]) continue;
    if (ctx->h_pinned[32 + k] != 0u) {  // a new point outside the grid: this kind is rebuilt around the larger set
      merge[k] = false, rebuild |= 1u << k, idx->grid_valid[k] = false;
      continue;
    }
    if (!idx->sorted2[k]) {
      if (hipMalloc(reinterpret_cast<void**>(&idx->sorted2[k]), (idx->cap[k] + kGridPad) * sizeof(GridPoint)) != hipSuccess ||
          hipMalloc(reinterpret_cast<void**>(&idx->rel2[k]), 3 * (idx->cap[k] + kGridPad) * sizeof(float)) != hipSuccess) {
        if (idx->sorted2[k]) (void)hipFree(idx->sorted2[k]);
        idx->sorted2[k] = nullptr, idx->rel2[k] = nullptr;
        merge[k] = false, rebuild |= 1u << k, idx->grid_valid[k] = false;  // (no room for the twins: the rebuild needs none)
        continue;
      }
    }
    const size_t cells = idx->cells_cap[k] ? idx->cells_cap[k] : kGridCellsCap;
    const GridSet gs = index_grid_set(idx, k);
    launch_index_insert_merge(gs, cells, (uint32_t)n_old[k], idx->pts[k] + n_old[k] * 3, (uint32_t)add[k], ws[k], idx->sorted2[k], idx->rel2[k], s);
    int rc = check_launch(ctx, "index_insert kernels");
    if (rc != LOAMX_OK) return rc;
    std::swap(idx->sorted[k], idx->sorted2[k]);
    std::swap(idx->rel[k], idx->rel2[k]);
    idx->grid_valid[k] = true;
    idx->merges++;
    idx->last_op[k] = LOAMX_INDEX_OP_MERGE, idx->kind_merges[k]++;
  }
  if (rebuild) return index_build(ctx, idx, rebuild);
  HIP_TRY(ctx, hipStreamSynchronize(s));
  return LOAMX_OK;
}

int index_append(loamx_ctx* ctx, loamx_target_index* idx, const double* edge, size_t n_e, const double* planar, size_t n_p) {
  const double* const host[2] = {edge, planar};
  const size_t add[2] = {n_e, n_p};
  double* stage[2];
  int rc = index_stage(ctx, idx, host, add, stage);
  if (rc != LOAMX_OK) return rc;
  return index_append_staged(ctx, idx, stage, add);
}

/* ---- map upkeep (loamx.h): voxel-filtered insert, crop, read-back ----------------------------------------------------- */
const char* const kVoxelRangeMsg = "a point's voxel coordinate floor(p / leaf) is outside (-2^20, 2^20)";

bool pose_finite(const double* pose) { return !pose || host_all_finite(pose, false, 7); }
// the pose the launchers take: nullptr for the identity (given as NULL or exactly {0,0,0,1,0,0,0}), so that nothing is computed
const double* pose_or_null(const double* pose) { return pose && !pose_is_identity(pose) ? pose : nullptr; }

// the flag words + the two kept counts of one call: [0, kMapFlagWords) flags, then one count per kind
int map_words_begin(loamx_ctx* ctx, uint32_t** words) {
  ENSURE(ctx, WS_MAP_WORDS, (kMapFlagWords + 2) * sizeof(uint32_t));
  *words = wsp<uint32_t>(ctx, WS_MAP_WORDS);
  untimed(ctx);
  HIP_TRY(ctx, hipMemsetAsync(*words, 0, (kMapFlagWords + 2) * sizeof(uint32_t), ctx->stream));
  return LOAMX_OK;
}
// the one read-back of a call (synchronises); returns the host copy in the pinned area
int map_words_end(loamx_ctx* ctx, const uint32_t* words, const uint32_t** host) {
  uint32_t* h = &ctx->h_pinned[40];
  HIP_TRY(ctx, hipMemcpyAsync(h, words, (kMapFlagWords + 2) * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *host = h;
  return LOAMX_OK;
}

// scratch of one filter / crop pass over n points, carved out of one buffer
struct MapTmp {
  double* moved;    // [n][3] transformed points
  uint32_t* slot;   // [n]
  uint32_t* tiles;  // map_compact_ws_bytes(n)
  uint8_t* keep;    // [n]
};
size_t map_tmp_bytes(size_t n) { return n * 24 + ((n * 4 + 7) & ~(size_t)7) + ((map_compact_ws_bytes(n) + 7) & ~(size_t)7) + n; }
MapTmp map_tmp_carve(void* base, size_t n) {
  unsigned char* p = static_cast<unsigned char*>(base);
  MapTmp t;
  t.moved = reinterpret_cast<double*>(p), p += n * 24;
  t.slot = reinterpret_cast<uint32_t*>(p), p += (n * 4 + 7) & ~(size_t)7;
  t.tiles = reinterpret_cast<uint32_t*>(p), p += (map_compact_ws_bytes(n) + 7) & ~(size_t)7;
  t.keep = p;
  return t;
}

// Brings kind k's occupancy table to "describes pts[k][0, n[k]) at `leaf`, with room for n_add more points below half
// load". (Re)built from the map's own points when there is none, after a crop or a failed call (vox_valid), when the leaf
// differs from the last call's or when the points would pass half of the slots; otherwise caught up with the points plain
// inserts have added since. A map point without a voxel at this leaf raises kMapFlagBadMapPoint.
int index_voxel_table(loamx_ctx* ctx, loamx_target_index* idx, int k, double leaf, size_t n_add, uint32_t* d_flags) {
  hipStream_t s = ctx->stream;
  VoxelTable& t = idx->vox[k];
  const size_t points = idx->n[k] + n_add;
  const bool fits = t.keys && (((size_t)1 << t.log2_cap) >= 2 * points);
  if (!fits || !idx->vox_valid[k] || idx->vox_leaf[k] != leaf || idx->vox_n[k] > idx->n[k]) {
    if (!fits) {  // 3 x the points, rounded up to a power of two: the map grows by half before the next rebuild at the earliest
      HIP_TRY(ctx, hipStreamSynchronize(s));
      if (t.keys) (void)hipFree(t.keys);
      if (t.owner) (void)hipFree(t.owner);
      t.keys = nullptr, t.owner = nullptr, idx->vox_valid[k] = false;
      t.log2_cap = voxel_table_log2(3 * points);
      if (hipMalloc(reinterpret_cast<void**>(&t.keys), sizeof(unsigned long long) << t.log2_cap) != hipSuccess ||
          hipMalloc(reinterpret_cast<void**>(&t.owner), sizeof(uint32_t) << t.log2_cap) != hipSuccess) {
        if (t.keys) (void)hipFree(t.keys);
        t.keys = nullptr, t.owner = nullptr;
        return fail(ctx, LOAMX_ERR_HIP, "hipMalloc failed for the occupancy table");
      }
    }
    HIP_TRY(ctx, hipMemsetAsync(t.keys, 0xFF, sizeof(unsigned long long) << t.log2_cap, s));
    HIP_TRY(ctx, hipMemsetAsync(t.owner, 0xFF, sizeof(uint32_t) << t.log2_cap, s));
    idx->vox_leaf[k] = leaf, idx->vox_n[k] = 0, idx->vox_valid[k] = true;
  }
  if (idx->vox_n[k] < idx->n[k]) {
    launch_voxel_claim(idx->pts[k] + idx->vox_n[k] * 3, (uint32_t)(idx->n[k] - idx->vox_n[k]), nullptr, leaf, t, (uint32_t)idx->vox_n[k], nullptr,
                       nullptr, d_flags, kMapFlagBadMapPoint, s);
    idx->vox_n[k] = idx->n[k];
  }
  return LOAMX_OK;
}
}  // namespace

extern "C" {

void loamx_target_index_destroy(loamx_ctx* ctx, loamx_target_index* index) {
  if (!index) return;
  if (ctx) {
    ApiLock lock(ctx);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  index_free(index);
}

int loamx_target_index_create(loamx_ctx* ctx, const double* tgt_edge, size_t n_te, const double* tgt_planar, size_t n_tp,
                              const loamx_reg_params* reg, loamx_target_index** out) {
  if (!ctx || !out) return LOAMX_ERR_BAD_PARAM;
  *out = nullptr;
  API_ENTER(ctx);
  RegConfig C;
  int rc = make_reg_config(ctx, reg, C);
  if (rc != LOAMX_OK) return rc;
  loamx_target_index* idx = new loamx_target_index;
  idx->radius[kEdge] = C.kind[kEdge].r, idx->radius[kPlane] = C.kind[kPlane].r;
  bool ok = hipMalloc(reinterpret_cast<void**>(&idx->counts), 2 * sizeof(uint32_t)) == hipSuccess;
  for (int k = 0; k < 2 && ok; k++) ok = hipMalloc(reinterpret_cast<void**>(&idx->desc[k]), sizeof(GridDesc)) == hipSuccess;  // (tables: index_build)
  rc = ok ? index_append(ctx, idx, tgt_edge, n_te, tgt_planar, n_tp) : fail(ctx, LOAMX_ERR_HIP, "hipMalloc failed for the target index");
  if (rc != LOAMX_OK) {
    index_free(idx);
    return rc;
  }
  *out = idx;
  return LOAMX_OK;
}

int loamx_target_index_insert(loamx_ctx* ctx, loamx_target_index* index, const double* edge, size_t n_edge, const double* planar,
                              size_t n_planar) {
  if (!ctx || !index) return LOAMX_ERR_BAD_PARAM;
  API_ENTER(ctx);
  if (n_edge == 0 && n_planar == 0) return LOAMX_OK;
  return index_append(ctx, index, edge, n_edge, planar, n_planar);
}

int loamx_target_index_stats(const loamx_target_index* index, uint64_t* full_builds, uint64_t* merges) {
  if (!index) return LOAMX_ERR_BAD_PARAM;
  if (full_builds) *full_builds = index->full_builds;
  if (merges) *merges = index->merges;
  return LOAMX_OK;
}

int loamx_target_index_size(const loamx_target_index* index, size_t* n_edge, size_t* n_planar) {
  if (!index) return LOAMX_ERR_BAD_PARAM;
  if (n_edge) *n_edge = index->n[0];
  if (n_planar) *n_planar = index->n[1];
  return LOAMX_OK;
}

int loamx_target_index_census(loamx_ctx* ctx, const loamx_target_index* index, int which_set, loamx_index_census* out) {
  if (!ctx || !index) return LOAMX_ERR_BAD_PARAM;
  API_ENTER(ctx);
  if (!out) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  if (which_set != 0 && which_set != 1) return fail(ctx, LOAMX_ERR_BAD_PARAM, "which_set: 0 = edge points, 1 = planar points");
  const int k = which_set;
  if (!index->grid_valid[k]) return fail(ctx, LOAMX_ERR_BAD_PARAM, "this kind has no grid (its last build or insert failed)");
  hipStream_t s = ctx->stream;
  untimed(ctx);
  GridDesc g;
  HIP_TRY(ctx, hipMemcpyAsync(&g, index->desc[k], sizeof(GridDesc), hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  const size_t n = index->n[k], stride = index->cap[k] + kGridPad;
  const GridBuildForm& f = index->build_form[k];
  const uint64_t ncell = (uint64_t)g.nx * (uint64_t)g.ny * (uint64_t)g.nz;
  out->n = n, out->capacity = index->cap[k];
  out->origin[0] = g.ox, out->origin[1] = g.oy, out->origin[2] = g.oz;
  out->h = g.h, out->inv_h = g.inv_h;
  out->nx = g.nx, out->ny = g.ny, out->nz = g.nz, out->n_points = g.n_points;
  out->build = f.form;
  out->table_entries = index->cells_cap[k] ? index->cells_cap[k] : kGridCellsCap;
  out->table_valid = index->table_valid[k] ? 1u : 0u;
  const uint32_t units = f.unit_cells ? (uint32_t)((ncell + f.unit_cells - 1) / f.unit_cells) : 0u;
  out->lds_passes = f.form == kGridBuildBig ? 0u : units;
  out->scan_tiles = f.form == kGridBuildBig ? units : 0u;
  out->last_op = index->last_op[k];
  out->full_builds = index->kind_builds[k], out->merges = index->kind_merges[k];
  if (ncell > out->table_entries) return fail(ctx, LOAMX_ERR_HIP, "the grid has more cells than its table has entries");
  if (out->cell_start && out->table_valid) {
    if (out->cell_start_cap < ncell + 1) return fail(ctx, LOAMX_ERR_BAD_PARAM, "cell_start_cap: nx * ny * nz + 1 entries are needed");
    HIP_TRY(ctx, hipMemcpyAsync(out->cell_start, index->cells[k], (ncell + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  }
  if ((out->xyz || out->orig) && out->points_cap < n) return fail(ctx, LOAMX_ERR_BAD_PARAM, "points_cap: n entries are needed");
  std::vector<GridPoint> sorted;
  if ((out->xyz || out->orig) && n) {
    sorted.resize(n);
    HIP_TRY(ctx, hipMemcpyAsync(sorted.data(), index->sorted[k], n * sizeof(GridPoint), hipMemcpyDeviceToHost, s));
  }
  if (out->rel) {
    if (out->rel_cap < n + kGridPad) return fail(ctx, LOAMX_ERR_BAD_PARAM, "rel_cap: n + 4 entries per plane are needed");
    for (int c = 0; c < 3; c++)
      HIP_TRY(ctx, hipMemcpyAsync(out->rel + c * out->rel_cap, index->rel[k] + c * stride, (n + kGridPad) * sizeof(float), hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(ctx, hipStreamSynchronize(s));
  for (size_t p = 0; p < sorted.size(); p++) {
    if (out->xyz) out->xyz[3 * p] = sorted[p].x, out->xyz[3 * p + 1] = sorted[p].y, out->xyz[3 * p + 2] = sorted[p].z;
    if (out->orig) out->orig[p] = sorted[p].orig;
  }
  return LOAMX_OK;
}

/* ---- map upkeep ------------------------------------------------------------------------------------------------------ */
int loamx_target_index_points(loamx_ctx* ctx, const loamx_target_index* index, int which_set, size_t first, size_t count, double* xyz_out) {
  if (!ctx || !index) return LOAMX_ERR_BAD_PARAM;
  API_ENTER(ctx);
  if (which_set != 0 && which_set != 1) return fail(ctx, LOAMX_ERR_BAD_PARAM, "which_set: 0 = edge points, 1 = planar points");
  const size_t n = index->n[which_set];
  if (first > n || count > n - first) return fail(ctx, LOAMX_ERR_BAD_PARAM, "first + count lies beyond the set");
  if (count == 0) return LOAMX_OK;
  if (!xyz_out) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  untimed(ctx);
  HIP_TRY(ctx, hipMemcpyAsync(xyz_out, index->pts[which_set] + first * 3, count * 24, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LOAMX_OK;
}

int loamx_voxel_filter_dev(loamx_ctx* ctx, const double* d_xyz, size_t n, const double pose[7], double leaf, double* d_xyz_out,
                           uint32_t* d_src_idx, uint32_t* d_n_out) {
  API_ENTER(ctx);
  if (!d_n_out || (n && (!d_xyz || !d_xyz_out))) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  if (n && d_xyz_out == d_xyz) return fail(ctx, LOAMX_ERR_BAD_PARAM, "the voxel filter does not work in place");
  if (leaf != leaf) return fail(ctx, LOAMX_ERR_BAD_PARAM, "leaf is NaN");
  if (!pose_finite(pose)) return fail(ctx, LOAMX_ERR_BAD_PARAM, "non-finite pose");
  if (n > 0x0FFFFFFFull) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "too many points in one call");
  hipStream_t s = ctx->stream;
  const double* P = pose_or_null(pose);
  untimed(ctx);
  if (leaf <= 0.0 || n == 0) {  // the transform alone (n == 0: the zero count)
    launch_map_transform(d_xyz, (uint32_t)n, P, d_xyz_out, d_src_idx, d_n_out, nullptr, s);
    CHECK_LAUNCH(ctx, "map_transform_kernel");
    return LOAMX_OK;
  }
  // call-local table (at most half full: 2 n slots or more) and scratch in the workspace. Dropped points (non-finite, or
  // out of range) only raise words nobody waits for here: the call does not synchronise.
  uint32_t* words = nullptr;
  int rc = map_words_begin(ctx, &words);
  if (rc != LOAMX_OK) return rc;
  VoxelTable t{nullptr, nullptr, voxel_table_log2(2 * n)};
  const size_t slots = (size_t)1 << t.log2_cap;
  ENSURE(ctx, WS_VOX_TABLE, slots * 12);
  ENSURE(ctx, ctx->wsk[WSK_MAP_TMP][0], map_tmp_bytes(n));
  t.keys = wsp<unsigned long long>(ctx, WS_VOX_TABLE), t.owner = reinterpret_cast<uint32_t*>(t.keys + slots);
  const MapTmp tmp = map_tmp_carve(ctx->wsk[WSK_MAP_TMP][0].p, n);
  HIP_TRY(ctx, hipMemsetAsync(t.keys, 0xFF, slots * 12, s));
  launch_voxel_claim(d_xyz, (uint32_t)n, P, leaf, t, 0u, tmp.moved, tmp.slot, words, kMapFlagBadPoint, s);
  launch_voxel_keep(t, tmp.slot, (uint32_t)n, 0u, tmp.keep, s);
  launch_map_compact(tmp.moved, tmp.keep, (uint32_t)n, tmp.tiles, d_xyz_out, d_src_idx, d_n_out, nullptr, nullptr, 0u, s);
  CHECK_LAUNCH(ctx, "voxel filter kernels");
  return LOAMX_OK;
}

int loamx_target_index_insert_filtered(loamx_ctx* ctx, loamx_target_index* index, const double* edge, size_t n_edge, const double* planar,
                                       size_t n_planar, const double world_T_scan[7], double edge_leaf, double planar_leaf, size_t* n_edge_added,
                                       size_t* n_planar_added) {
  if (!ctx || !index) return LOAMX_ERR_BAD_PARAM;
  API_ENTER(ctx);
  if (n_edge_added) *n_edge_added = 0;
  if (n_planar_added) *n_planar_added = 0;
  if (edge_leaf != edge_leaf || planar_leaf != planar_leaf) return fail(ctx, LOAMX_ERR_BAD_PARAM, "leaf is NaN");
  if (!pose_finite(world_T_scan)) return fail(ctx, LOAMX_ERR_BAD_PARAM, kNonFiniteMsg);
  if (n_edge == 0 && n_planar == 0) return LOAMX_OK;
  loamx_target_index* idx = index;
  const double* const host[2] = {edge, planar};
  const size_t add[2] = {n_edge, n_planar};
  const double leaf[2] = {edge_leaf, planar_leaf};
  double* stage[2];
  int rc = index_stage(ctx, idx, host, add, stage);
  if (rc != LOAMX_OK) return rc;
  hipStream_t s = ctx->stream;
  const double* P = pose_or_null(world_T_scan);
  uint32_t* words = nullptr;
  rc = map_words_begin(ctx, &words);
  if (rc != LOAMX_OK) return rc;
  // both kinds are filtered into the workspace before anything is read back: the index itself is not touched until the
  // one read-back below has shown that the call goes through
  double* out[2] = {nullptr, nullptr};
  for (int k = 0; k < 2; k++) {  // (all the room first: nothing below leaves early with claims in a table)
    if (!add[k]) continue;
    ENSURE(ctx, ctx->wsk[WSK_MAP_OUT][k], add[k] * 24);
    if (leaf[k] > 0.0) ENSURE(ctx, ctx->wsk[WSK_MAP_TMP][k], map_tmp_bytes(add[k]));
  }
  for (int k = 0; k < 2; k++) {
    if (!add[k]) continue;
    out[k] = wskp<double>(ctx, WSK_MAP_OUT, k);
    if (leaf[k] <= 0.0) {  // transformed, unfiltered
      launch_map_transform(stage[k], (uint32_t)add[k], P, out[k], nullptr, words + kMapFlagWords + k, words, s);
      continue;
    }
    const MapTmp tmp = map_tmp_carve(ctx->wsk[WSK_MAP_TMP][k].p, add[k]);
    rc = index_voxel_table(ctx, idx, k, leaf[k], add[k], words);
    if (rc != LOAMX_OK) {
      idx->vox_valid[0] = idx->vox_valid[1] = false;
      return rc;
    }
    const uint32_t base = (uint32_t)idx->n[k];
    launch_voxel_claim(stage[k], (uint32_t)add[k], P, leaf[k], idx->vox[k], base, tmp.moved, tmp.slot, words, kMapFlagBadPoint, s);
    launch_voxel_keep(idx->vox[k], tmp.slot, (uint32_t)add[k], base, tmp.keep, s);
    launch_map_compact(tmp.moved, tmp.keep, (uint32_t)add[k], tmp.tiles, out[k], nullptr, words + kMapFlagWords + k, &idx->vox[k], tmp.slot, base, s);
  }
  rc = check_launch(ctx, "voxel filter kernels");
  const uint32_t* h = nullptr;
  if (rc == LOAMX_OK) rc = map_words_end(ctx, words, &h);
  if (rc == LOAMX_OK && h[kMapFlagGaveUp]) rc = fail(ctx, LOAMX_ERR_HIP, "the occupancy table's probe sequence gave up (table full)");
  if (rc == LOAMX_OK && (h[kMapFlagBadPoint] || h[kMapFlagBadMapPoint])) rc = fail(ctx, LOAMX_ERR_UNSUPPORTED, kVoxelRangeMsg);
  if (rc != LOAMX_OK) {  // the tables hold claims of points that were not inserted: built again by the next call
    idx->vox_valid[0] = idx->vox_valid[1] = false;
    return rc;
  }
  const size_t kept[2] = {add[0] ? h[kMapFlagWords + 0] : 0u, add[1] ? h[kMapFlagWords + 1] : 0u};
  if (n_edge_added) *n_edge_added = kept[0];
  if (n_planar_added) *n_planar_added = kept[1];
  if (kept[0] == 0 && kept[1] == 0) return LOAMX_OK;  // (no voxel was claimed either: the tables describe the map as before)
  const bool tabled[2] = {kept[0] && leaf[0] > 0.0, kept[1] && leaf[1] > 0.0};
  for (int k = 0; k < 2; k++)
    if (tabled[k]) idx->vox_valid[k] = false;  // ... until the points are really in the map
  rc = index_append_staged(ctx, idx, out, kept);
  if (rc != LOAMX_OK) return rc;
  for (int k = 0; k < 2; k++)
    if (tabled[k]) idx->vox_valid[k] = true, idx->vox_n[k] = idx->n[k];
  return LOAMX_OK;
}

int loamx_target_index_crop(loamx_ctx* ctx, loamx_target_index* index, const double lo[3], const double hi[3], size_t* n_edge_removed,
                            size_t* n_planar_removed) {
  if (!ctx || !index) return LOAMX_ERR_BAD_PARAM;
  API_ENTER(ctx);
  if (n_edge_removed) *n_edge_removed = 0;
  if (n_planar_removed) *n_planar_removed = 0;
  if (!lo || !hi) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  for (int c = 0; c < 3; c++)
    if (!(lo[c] <= hi[c])) return fail(ctx, LOAMX_ERR_BAD_PARAM, "crop box: lo <= hi on every axis (and no NaN)");
  loamx_target_index* idx = index;
  if (idx->n[0] == 0 && idx->n[1] == 0) return LOAMX_OK;
  hipStream_t s = ctx->stream;
  uint32_t* words = nullptr;
  int rc = map_words_begin(ctx, &words);
  if (rc != LOAMX_OK) return rc;
  double* out[2] = {nullptr, nullptr};
  for (int k = 0; k < 2; k++) {
    const size_t n = idx->n[k];
    if (!n) continue;
    ENSURE(ctx, ctx->wsk[WSK_MAP_OUT][k], n * 24);
    ENSURE(ctx, ctx->wsk[WSK_MAP_TMP][k], map_tmp_bytes(n));
    out[k] = wskp<double>(ctx, WSK_MAP_OUT, k);
    const MapTmp tmp = map_tmp_carve(ctx->wsk[WSK_MAP_TMP][k].p, n);
    launch_crop_keep(idx->pts[k], (uint32_t)n, lo, hi, tmp.keep, s);
    launch_map_compact(idx->pts[k], tmp.keep, (uint32_t)n, tmp.tiles, out[k], nullptr, words + kMapFlagWords + k, nullptr, nullptr, 0u, s);
  }
  CHECK_LAUNCH(ctx, "crop kernels");
  const uint32_t* h = nullptr;
  rc = map_words_end(ctx, words, &h);
  if (rc != LOAMX_OK) return rc;
  unsigned rebuild = 0u;
  size_t removed[2] = {0, 0};
  for (int k = 0; k < 2; k++) {
    if (!idx->n[k]) continue;
    const size_t kept = h[kMapFlagWords + k];
    removed[k] = idx->n[k] - kept;
    if (!removed[k]) continue;  // (a kind that loses nothing is not touched)
    if (kept) HIP_TRY(ctx, hipMemcpyAsync(idx->pts[k], out[k], kept * 24, hipMemcpyDeviceToDevice, s));
    idx->n[k] = kept, idx->grid_valid[k] = false, rebuild |= 1u << k;
    idx->vox_valid[k] = false;  // (the indices have shifted)
  }
  if (n_edge_removed) *n_edge_removed = removed[0];
  if (n_planar_removed) *n_planar_removed = removed[1];
  return rebuild ? index_build(ctx, idx, rebuild) : LOAMX_OK;
}

}  // extern "C"
