// api_host.h — what the host translation units of libloamx.so (api_*.hip) share: the context and the persistent index,
// workspace and error helpers, the timing scopes, the extraction driver and the pieces of the registration driver.
// Host only: no *_kernels.hip includes it. Every function declared here has its one definition in the unit named beside it.
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "loamx_internal.h"

namespace loamx {

enum WsId {
  WS_XYZ = 0, WS_CURV, WS_MASK,
  WS_SORT_SCRATCH, WS_SORT_SCRATCH_SRC, WS_NASSOC, WS_STATE, WS_PARTIALS, WS_MOM_PARTIALS, WS_MOMENTS, WS_FLAGGED_LIST, WS_FLAGGED_COUNT,
  WS_LINE_TOT, WS_EXTRACT_EVENTS, WS_BOX, WS_FINITE_FLAG, WS_COUNTERS, WS_ITERINFO, WS_STREAM_IN0, WS_STREAM_IN1, WS_STREAM_RES,
  WS_FIT_IN, WS_FIT_OUT, WS_FCOUNTS, WS_RESULTS, WS_INIT, WS_STREAM_INIT,
  WS_VOX_TABLE, WS_MAP_WORDS, WS_INFO_PARTIALS, WS_INFO, WS_LIVE,
  WS_ORG_WINNER, WS_ORG_RANGE, WS_ORG_CELL, WS_ORG_COUNTS, WS_ORG_IN, WS_ORG_RINGS, WS_ORG_OUT,
  WS_PLACE_TABLE, WS_PLACE_QKEYS, WS_PLACE_QNORMS, WS_PLACE_CAND_A, WS_PLACE_CAND_B, WS_PLACE_MATCH, WS_PLACE_IN, WS_PLACE_OUT,
  WS_PGO_WORK, WS_PGO_POSES, WS_PGO_FIXED, WS_PGO_EDGES, WS_PGO_OUT,
  WS_CLOUD_IN, WS_CLOUD_POSE, WS_CLOUD_OUT,
  WS_SEG_BYTES, WS_SEG_WORDS, WS_SEG_COUNTS, WS_SEG_IN, WS_SEG_OUT,
  WS_VIS_RANGES, WS_VIS_CENSUS, WS_VIS_KEEP, WS_VIS_TILES, WS_VIS_IN, WS_VIS_SCANS, WS_VIS_POSES, WS_VIS_OUT,
  WS_OCC_IN, WS_OCC_POSE, WS_OCC_OUT, WS_RAY_CENSUS,
  WS_SURFEL_IN, WS_SURFEL_POSE, WS_SURFEL_OUT,
  WS_LOC_IN, WS_LOC_POSE, WS_LOC_OUT,
  WS_COUNT
};
// the buffers that exist once per feature kind: loamx_ctx::wsk[id][kEdge | kPlane]
enum WsKindId {
  WSK_STAGE = 0, WSK_CNT, WSK_IDX, WSK_N, WSK_XYZ,
  WSK_GRID_DESC, WSK_CELLS, WSK_SORTED, WSK_REL, WSK_SGRID_DESC, WSK_SCELLS, WSK_SSORTED, WSK_ASSOC, WSK_NN, WSK_RNN, WSK_NEAREST,
  WSK_REST, WSK_EXACT, WSK_DUMP, WSK_SRC, WSK_TGT, WSK_MAP_TMP, WSK_MAP_OUT, WSK_CENSUS,
  WSK_COUNT
};

struct Buf {
  void* p = nullptr;
  size_t cap = 0;
};

struct PendingEvent {
  int kernel;
  hipEvent_t e0, e1;
  double bytes;
  bool own_e0;  // false: e0 is the previous scope's e1 (back-to-back scopes share the event between them)
};

}  // namespace loamx

struct loamx_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  bool max_counts_clean = false;     // write_results_kernel has reset RegBatch::max_counts for the next call
  hipStream_t aux_stream = nullptr;  // edge association chain, forked from / joined into `stream` with the two events
  hipEvent_t ev_fork = nullptr, ev_mid = nullptr, ev_join = nullptr;
  hipEvent_t ev_counts = nullptr;     // marks the read-back of the largest source set sizes (reg_prepare)
  hipStream_t aux2_stream = nullptr;  // the plane queue chain (so that it does not wait behind the edge chain)
  hipEvent_t ev_join2 = nullptr;
  std::string last_error;
  loamx::Buf ws[loamx::WS_COUNT];
  loamx::Buf wsk[loamx::WSK_COUNT][2];
  uint32_t* h_pinned = nullptr;  // small pinned readback area
  bool timing = false;
  std::vector<loamx::PendingEvent> pending;
  std::vector<hipEvent_t> event_pool;
  hipEvent_t tail_event = nullptr;  // end event of the last timed scope ...
  bool tail_fresh = false;          // ... and nothing has been enqueued on the stream since
  loamx_kernel_stat stats[LOAMX_K_COUNT] = {};

  // debug / measurement switches (loamx_ctx_set_option; defaults from LOAMX_<NAME>, read once at creation)
  uint32_t extract_flags = 0;  // kFlag* of extract_math.h
  uint32_t reg_flags = 0;      // kRegFlag* of loamx_internal.h
  int map_cells_log2 = 0;      // cell table of a map-sized persistent index (0: kGridMapCellsCap)
  int stream_chunk_pairs = 0;  // pairs per uploaded chunk of loamx_register_scan_pairs (0: kStreamChunkPairs)
  hipStream_t copy_stream = nullptr;  // uploads of loamx_register_scan_pairs (created on first use)
  hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_free[2] = {nullptr, nullptr};

  uint32_t last_extract_route = 0;  // LOAMX_ROUTE_* of the last extract_dev call (loamx_ctx_last_extract_route)
  // the last reg_solve's call as loamx_ctx_last_solve_census reads it: device pointers into the workspace (and to the call's
  // count arrays), good from reg_solve until the next reg_prepare sizes the workspace anew
  loamx::RegBatch last_solve_batch = {};
  uint32_t last_solve_flags = 0;  // RegConfig::flags of that call
  bool last_solve_valid = false;
  // the last reg_dump's association census per feature kind (loamx_ctx_last_assoc_census): host copies, complete when reg_dump
  // returns; the pointers of `c` are unused, the per-entry arrays live in the vectors. Good until the next reg_prepare.
  struct AssocCensusKept {
    loamx_assoc_census c;
    std::vector<uint32_t> entry;  // the queue's entries: query index | reason bits
    std::vector<int32_t> after_rest, before_fit;
    std::vector<uint32_t> late;   // the late list's queries
    uint32_t coop_forms[2] = {0, 0};  // listed entries associate_knn_coop_kernel gave a row of lanes / a whole wavefront (loamx_ctx_last_assoc_coop_forms)
  } last_assoc_census[2];
  bool last_assoc_census_valid = false;

  // the last segmentation call (loamx_ctx_last_segment_census): its edge counts are n_scans words of WS_SEG_COUNTS
  struct {
    bool valid = false, tiles = false;
    uint32_t H = 0, W = 0, n_scans = 0;
  } last_segment;
  // the last visibility votes call (loamx_ctx_last_visibility_census): its pair counts are two words of WS_VIS_CENSUS
  struct {
    bool valid = false, counted = false;  // counted: kernels ran and left the words (otherwise both counts are 0)
    uint32_t form = 0, scan_chunks = 0;
  } last_visibility;

  // the last ray cast or render call (loamx_ctx_last_raycast_census): its counters are the words of WS_RAY_CENSUS
  struct {
    bool counted = false;  // a kernel ran and left the words (otherwise every count is 0)
    uint64_t rays = 0;
  } last_raycast;

  unsigned long long sweep_slots_base[2] = {0, 0};
  unsigned long long features_base = 0;  // events[2] at the last loamx_ctx_reset_kernel_stats
  std::mutex mu;
};

struct loamx_target_index {
  loamx::GridDesc* desc[2] = {nullptr, nullptr};     // [edge, plane], one GridDesc each
  uint32_t* cells[2] = {nullptr, nullptr};           // kGridCellsCap + 1 entries each
  loamx::GridPoint* sorted[2] = {nullptr, nullptr};  // n + kGridPad entries each
  float* rel[2] = {nullptr, nullptr};                // 3 x (n + kGridPad) single-precision offsets (FP32 pre-selection)
  double* pts[2] = {nullptr, nullptr};               // the points in insertion order (index = `orig` of the sorted copy)
  size_t n[2] = {0, 0};
  size_t cap[2] = {0, 0};                            // points the buffers above hold without growing
  double radius[2] = {0, 0};
  uint32_t* counts = nullptr;                        // device copy of n[] for the build kernels
  void* scratch = nullptr;                           // box keys + cursors of the multi-workgroup build
  uint32_t cells_cap[2] = {0, 0};                    // 0: kGridCellsCap; map-sized sets own a larger cell table
  size_t cells_alloc[2] = {0, 0}, scratch_alloc = 0;
  // incremental insert (index_merge): twin buffers of sorted / rel, the set size at the last full build of the kind
  // (a kind that has doubled since is rebuilt: its cell edge is chosen for the density it had then), event counters
  loamx::GridPoint* sorted2[2] = {nullptr, nullptr};
  float* rel2[2] = {nullptr, nullptr};
  size_t n_at_build[2] = {0, 0};
  bool grid_valid[2] = {false, false};  // the kind's cell-sorted arrays + table describe idx->pts[k][0 .. n[k]) (full build or merges since)
  uint64_t full_builds = 0, merges = 0;  // per kind: a call that rebuilds both kinds counts two
  // what loamx_target_index_census reports per kind: the launcher's choice at the kind's last full build, whether that build
  // (or a merge since) left a written cell table, the last operation (LOAMX_INDEX_OP_*) and the kind's own event counts
  loamx::GridBuildForm build_form[2] = {{0u, 0u, 0u}, {0u, 0u, 0u}};
  bool table_valid[2] = {false, false};
  uint32_t last_op[2] = {0u, 0u};
  uint64_t kind_builds[2] = {0, 0}, kind_merges[2] = {0, 0};
  // occupancy table of the filtered insert, one per kind (loamx_internal.h: VoxelTable; built by the first filtered insert).
  // While vox_valid[k]: owner[slot] = lowest index in pts[k] of any point of that voxel at leaf vox_leaf[k], over the
  // points [0, vox_n[k]) — plain inserts leave vox_n behind n, the next filtered insert catches up.
  loamx::VoxelTable vox[2] = {{nullptr, nullptr, 0u}, {nullptr, nullptr, 0u}};
  double vox_leaf[2] = {0, 0};
  size_t vox_n[2] = {0, 0};
  bool vox_valid[2] = {false, false};
};

namespace loamx {

/* ---- errors, workspace (api_core.hip) ------------------------------------------------------------------------------- */
int fail(loamx_ctx* ctx, int code, const std::string& msg);  // keeps msg as the context's last error, returns code

#define HIP_TRY(ctx, expr)                                                                          \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess)                                                                           \
      return fail(ctx, LOAMX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));           \
  } while (0)

// grows b to `bytes` (synchronises the context's stream before it frees the old block)
int ensure(loamx_ctx* ctx, Buf& b, size_t bytes);
int ensure(loamx_ctx* ctx, int id, size_t bytes);  // ctx->ws[id]
#define ENSURE(ctx, id, bytes)                       \
  do {                                               \
    int rc_ = ensure(ctx, id, bytes);                \
    if (rc_ != LOAMX_OK) return rc_;                 \
  } while (0)

template <typename T>
T* wsp(loamx_ctx* ctx, int id) {
  return reinterpret_cast<T*>(ctx->ws[id].p);
}
template <typename T>
T* wskp(loamx_ctx* ctx, int id, int kind) {
  return reinterpret_cast<T*>(ctx->wsk[id][kind].p);
}

int check_launch(loamx_ctx* ctx, const char* what);
#define CHECK_LAUNCH(ctx, what)                      \
  do {                                               \
    int rc_ = check_launch(ctx, what);               \
    if (rc_ != LOAMX_OK) return rc_;                 \
  } while (0)

// Every entry point that touches the context holds its mutex from here to its return. API_LOCK: the null test and the lock;
// API_ENTER: the same, then the context's device is selected for the calling thread. Each expands to several statements (the
// lock has to outlive the macro): only as a statement of its own at function scope, with the context named `ctx`.
struct ApiLock {
  std::lock_guard<std::mutex> guard;
  explicit ApiLock(loamx_ctx* ctx) : guard(ctx->mu) {}
};
#define API_LOCK(ctx)                                \
  if (!ctx) return LOAMX_ERR_BAD_PARAM;              \
  loamx::ApiLock api_lock_(ctx)
#define API_ENTER(ctx)                               \
  API_LOCK(ctx);                                     \
  HIP_TRY(ctx, hipSetDevice(ctx->device))

/* ---- timing (api_core.hip) ------------------------------------------------------------------------------------------ */
hipEvent_t take_event(loamx_ctx* ctx);
int resolve_events(loamx_ctx* ctx);

struct TimedScope {
  loamx_ctx* ctx;
  PendingEvent pe;
  bool on, attach;
  LaunchScope ls;
  // attach: the events ride on the scope's own kernels (single-stream scopes); otherwise marker events around it. kernel < 0:
  // what the scope holds has no row of its own and is never timed
  TimedScope(loamx_ctx* c, int kernel, double bytes, bool attach_ = false) : ctx(c), on(c->timing && kernel >= 0), attach(attach_) {
    if (on) {
      pe.kernel = kernel, pe.bytes = bytes;
      if (attach) {
        pe.own_e0 = true;
        pe.e0 = take_event(ctx), pe.e1 = take_event(ctx);
        ls = LaunchScope{pe.e0, pe.e1, true};
        g_launch_scope = &ls;
        return;
      }
      // back-to-back scopes share one event: half the event packets between the kernels
      pe.own_e0 = !(ctx->tail_fresh && ctx->tail_event);
      pe.e0 = pe.own_e0 ? take_event(ctx) : ctx->tail_event;
      pe.e1 = take_event(ctx);
      if (pe.own_e0) (void)hipEventRecord(pe.e0, ctx->stream);
    }
  }
  ~TimedScope() {
    if (on) {
      if (attach) {
        g_launch_scope = nullptr;
        if (ls.first) {  // no kernel was launched inside: nothing to time
          ctx->event_pool.push_back(pe.e0), ctx->event_pool.push_back(pe.e1);
        } else {
          ctx->pending.push_back(pe);
        }
        ctx->tail_fresh = false;
        return;
      }
      (void)hipEventRecord(pe.e1, ctx->stream);
      ctx->pending.push_back(pe);
      ctx->tail_event = pe.e1, ctx->tail_fresh = true;
    }
  }
};
// call before enqueueing anything outside a TimedScope: the next scope must record its own start
inline void untimed(loamx_ctx* ctx) { ctx->tail_fresh = false; }

/* ---- non-finite input (loamx.h: "Non-finite input"; api_core.hip) --------------------------------------------------- */
extern const char* const kNonFiniteMsg;
bool host_all_finite(const void* p, bool f32, size_t n_scalars);
// The check itself runs on the device in every case (a CPU loop over a 128 x 2048 scan costs more than its upload): zero the
// flag word, one finite_kernel launch per array, a 4-byte read-back. Host entry points do it on their uploaded copies before
// they launch anything else (one extra stream synchronisation, ~30 us); "_dev" entry points only under CHECK_FINITE.
int finite_begin(loamx_ctx* ctx);
// d_n == nullptr: `stride` points per set
void finite_add(loamx_ctx* ctx, const void* d_pts, bool f32, const uint32_t* d_n, size_t n_sets, size_t stride, uint32_t pitch);
int finite_end(loamx_ctx* ctx);
// begin, one array, end; looks only under CHECK_FINITE unless `force`
int dev_check_finite(loamx_ctx* ctx, const void* d_pts, bool f32, const uint32_t* d_n, size_t n_sets, size_t stride, uint32_t pitch, bool force = false);
// begin, n doubles counted as scalars (poses, motions: the buffer need not end on a whole point), end; looks always
int check_finite_scalars(loamx_ctx* ctx, const double* d, size_t n);

/* ---- parameter translation (api_core.hip) --------------------------------------------------------------------------- */
int make_extract_params(loamx_ctx* ctx, const loamx_lidar_params* lidar, const loamx_fe_params* fe, ExtractParams& P);
int make_reg_config(loamx_ctx* ctx, const loamx_reg_params* r, RegConfig& C);
inline size_t edge_capacity(const ExtractParams& P) { return (size_t)P.H * P.S * P.cap_edge; }
inline size_t planar_capacity(const ExtractParams& P) { return (size_t)P.H * P.S * P.cap_planar; }

/* ---- extraction over device-resident scans (api_extract.hip) -------------------------------------------------------- */
// Bounding boxes of the feature sets of every scan, taken by the selection's copy phase (select_rows_kernel with the fused
// compaction): min / max[scan][kind][axis] as ordered keys; valid while *bad == 0 (a tied or given-up line sends its scan through
// compact_kernel, which takes no boxes). All nullptr when the extraction went another way.
struct ExtractBoxes {
  const unsigned long long *min = nullptr, *max = nullptr;
  const uint32_t* bad = nullptr;
};
// d_xyz: double, or float when f32 (FP32-input path)
int extract_dev(loamx_ctx* ctx, const void* d_xyz, bool f32, size_t n_scans, const ExtractParams& P, uint32_t* d_edge_idx,
                uint32_t* d_n_edge, double* d_edge_xyz, uint32_t* d_planar_idx, uint32_t* d_n_planar,
                double* d_planar_xyz, bool only_curvature_mask, ExtractBoxes* boxes = nullptr);

/* ---- registration over device-resident feature sets (api_register.hip) ---------------------------------------------- */
struct RegInputs {
  size_t n_pairs;
  uint32_t in_pitch;
  struct Kind {  // as RegKind
    size_t stride;
    const double *src, *tgt;
    const uint32_t *n_src, *n_tgt;
  } kind[2];
  const double* init;
  ExtractBoxes boxes;  // (optional) bounding boxes of the sets, left by the extraction that produced them
  uint32_t src_box_offset;  // RegBatch::src_box_offset: scans from a pair's target box to its source box; 0: target boxes only
};

struct RegPrepareOpts {
  bool want_iter_info;      // room for loamx_iter_info records (WS_ITERINFO), bound to RegBatch::iter_info
  bool want_nearest;        // a hook of reg_solve will read RegKind::nearest
  bool want_info_partials;  // room for reg_information's partial sums (WS_INFO_PARTIALS)
  // The caller wants ONE association pass and no solve (reg_dump, reg_information(false)). The reference's associateEdges /
  // associatePlanes (registration.cpp:23-103) do not know max_iterations; here a pair with max_iterations == 0 is never active
  // (state_init_kernel), so its association kernels would return at once and the pass would read workspace nobody wrote:
  // max_iterations == 0 becomes 1, one iteration's worth of "active".
  bool one_pass;
};

// host-side hook called after the association kernels of iteration `it` (detail capture)
typedef int (*AfterAssocHook)(loamx_ctx*, const RegBatch&, uint32_t it, void* user);

// A registration call is reg_prepare followed by one of
//   reg_dump                                   loamx_associate
//   reg_information(activate = false)          the information matrices at given poses (they arrive as RegInputs::init)
//   reg_solve                                  the registration
//   reg_solve, reg_information(true)           ... and the information matrices at its final estimates
// No pairs: reg_prepare leaves B.n_pairs == 0 and enqueues nothing, and so does each of the others.
//
// reg_prepare: size checks, B, the scratch table, the per-pair state, the index builds (the target's unless `prebuilt` holds
// it) and the read-back of the largest set sizes: B is ready for association passes when it returns.
int reg_prepare(loamx_ctx* ctx, const RegInputs& in, RegConfig& C, const loamx_target_index* prebuilt, const RegPrepareOpts& opts, RegBatch& B);
// the partial sums reg_prepare made room for under want_info_partials: what reg_information takes as info_partials
inline InfoPartial* reg_info_partials(loamx_ctx* ctx) { return wsp<InfoPartial>(ctx, WS_INFO_PARTIALS); }
// the ICF loop (up to C.max_iterations, stops when the host sees no active pair) and the result records
int reg_solve(loamx_ctx* ctx, const RegBatch& B, const RegConfig& C, loamx_reg_result* d_results, AfterAssocHook hook, void* hook_user);
// ONE association pass at the initial estimate of the one pair, read out into the host arrays of *dump (synchronises)
int reg_dump(loamx_ctx* ctx, const RegBatch& B, const RegConfig& C, const loamx_assoc_dump* dump, const size_t n_src[2]);
// ONE association pass at the pairs' current estimates, then the information kernels: one record per pair in d_info.
// activate: behind reg_solve, where every pair has stopped (see the definition)
int reg_information(loamx_ctx* ctx, const RegBatch& B, const RegConfig& C, InfoPartial* info_partials, loamx_reg_information* d_info, bool activate);

/* ---- the clouds of a call, kOrgChunkClouds at a time (their offsets travel as a kernel argument) ------------------------------ */
// for (CloudChunks ch(offsets, n_clouds); ch.next();): clouds c0 .. c0 + nc - 1, their offsets in `offs` (the entries behind the
// last cloud repeat its end), `largest`: the points of the chunk's largest cloud
struct CloudChunks {
  const size_t* offsets;
  size_t n_clouds, c0 = 0;
  uint32_t nc = 0;
  OrgOffsets offs;
  unsigned long long largest = 0;
  CloudChunks(const size_t* offsets_, size_t n_clouds_) : offsets(offsets_), n_clouds(n_clouds_) {}
  bool next() {
    c0 += nc;
    if (c0 >= n_clouds) return false;
    nc = (uint32_t)(n_clouds - c0 < kOrgChunkClouds ? n_clouds - c0 : kOrgChunkClouds);
    largest = 0;
    for (uint32_t c = 0; c <= kOrgChunkClouds; c++) offs.off[c] = offsets[c0 + (c < nc ? c : nc)];
    for (uint32_t c = 0; c < nc; c++) largest = offs.off[c + 1] - offs.off[c] > largest ? offs.off[c + 1] - offs.off[c] : largest;
    return true;
  }
};

/* ---- persistent index ------------------------------------------------------------------------------------------------ */
// kind k of a persistent index as the search and build kernels take it
inline GridSet index_grid_set(const loamx_target_index* idx, int k) {
  return GridSet{idx->desc[k], idx->cells[k], idx->sorted[k], idx->cap[k] + kGridPad, idx->rel[k], idx->cells_cap[k]};
}

}  // namespace loamx
