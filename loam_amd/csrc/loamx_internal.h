// loamx_internal.h — declarations shared by the .hip translation units of libloamx.so.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/loamx.h"
#include "extract_math.h"
#include "reg_math.h"
#include "organize_math.h"
#include "place_math.h"
#include "segment_math.h"
#include "visibility_math.h"
#include "occupancy_math.h"
#include "raycast_math.h"
#include "xcd_map.h"

namespace loamx {

/* ---- kernel launches with timing attached (api_host.h: TimedScope) ---------------------------------------
 * While a timing scope of the calling thread is in "attach" mode, the first kernel launched records the scope's
 * start event with its own begin and every kernel re-records the stop event with its end (the last one
 * stands): hipExtLaunchKernelGGL takes the timestamps from the dispatch itself, so no marker packets sit between
 * the kernels of the timed region (barrier-style hipEventRecord cost 2.5 % of the step). */
struct LaunchScope {
  hipEvent_t start, stop;
  bool first;
};
extern thread_local LaunchScope* g_launch_scope;
// LOAMX_DEBUG_SYNC=1 (read once): every launch is followed by a stream synchronisation and a line on stderr with the
// kernel's name and the status — the last line before a GPU fault names the kernel that faulted (debugging only)
extern int g_debug_sync;
template <typename F, typename... Args>
inline void launch_kernel_named(const char* name, F kernel, const dim3& grid, const dim3& block, size_t shmem, hipStream_t s, Args... args) {
  LaunchScope* sc = g_launch_scope;
  if (g_debug_sync) fprintf(stderr, "[loamx] launch %s grid %u x %u block %u\n", name, grid.x, grid.y, block.x), fflush(stderr);
  if (sc) {
    hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)shmem, s, sc->first ? sc->start : nullptr, sc->stop, 0, args...);
    sc->first = false;
  } else {
    hipLaunchKernelGGL(kernel, grid, block, shmem, s, args...);
  }
  if (g_debug_sync) {
    const hipError_t e = hipStreamSynchronize(s);
    fprintf(stderr, "[loamx]   done %s: %s\n", name, hipGetErrorString(e)), fflush(stderr);
  }
}
#define launch_kernel(kernel, ...) launch_kernel_named(#kernel, kernel, __VA_ARGS__)

/* ---- extraction (extract_kernels.hip) ---------------------------------------------------------- */
constexpr int kMaxNeighborPoints = 16;  // LDS halo bound of curvature_valid_kernel
constexpr int kMaxLineWidth = 4096;     // select_kernel keeps one line's curvature + mask in LDS

// LOAMX_ROUTE_* bits of the extraction the calling thread is enqueueing (loamx_ctx_last_extract_route): every launcher below
// notes its choice here at the branch that makes it; extract_dev clears the word and keeps it on the context (host side only)
extern thread_local uint32_t g_extract_route;

// staging layout written by select_kernel: per (scan, line, sector) a fixed slot of cap entries
struct ExtractStage {
  uint32_t* edge_stage;    // [n_scans][H][S][cap_edge]
  uint32_t* planar_stage;  // [n_scans][H][S][cap_planar]
  uint32_t* edge_cnt;      // [n_scans][H][S]
  uint32_t* planar_cnt;    // [n_scans][H][S]
};

// d_xyz: n_scans x H x W x 3 scalars, double or (f32) float
// Outputs select_mis_kernel writes itself when the compaction is fused into the selection (see the kernel).
struct ExtractFused {
  unsigned long long* line_tot;  // [n_lines] published totals of every scan line (bit 63), or the tie mark (bit 62); zeroed before the launch
  uint32_t fuse;                 // 1: select_mis_kernel writes the final arrays itself (chained scan over line_tot)
  const void* xyz;               // the scans (double, or float when f32)
  uint32_t f32;
  uint32_t* edge_idx;            // outputs as launch_compact
  uint32_t* n_edge;
  double* edge_xyz;
  size_t edge_stride;
  uint32_t* planar_idx;
  uint32_t* n_planar;
  double* planar_xyz;
  size_t planar_stride;
  uint32_t* error;  // flag word (zeroed before every launch, next to line_tot). Bit 0: a wavefront gave up waiting for the
                    // lines before it (or they are tied): the fallback compaction gathers the batch from the stage arrays;
                    // bit 1: some line is tied (replay_kernel has work)
  unsigned long long* events;  // [3] cumulative: scan lines replayed in the reference's tie order, give-up fallbacks taken, features written by the fused path
  // optional (select_rows_kernel with the fused compaction only): bounding boxes of every scan's edge / planar features as ordered
  // keys (dbl_key), box_min / box_max[scan][kind][axis], kind 0 = edge, 1 = planar; the caller presets them (all ones / zero).
  // Complete iff the flag word *error stays zero (no line gave up or was tied: those scans went through compact_kernel).
  unsigned long long* box_min;
  unsigned long long* box_max;
  // select_rows_kernel only (round 5). no_stage: the stage arrays and per-sector counts — the fallback compaction's input — are
  // not written; only_if: the launch leaves at once unless this word is non-zero. launch_select runs the fused selection
  // without the stage arrays (4 B per feature saved) and, behind it, the plain one under only_if = error: when a line gave up
  // or was tied, that second launch produces what replay_kernel / compact_kernel read; otherwise it costs its launch.
  uint32_t no_stage;
  const uint32_t* only_if;
};
// doubles as unsigned keys with the same order (for atomicMin / atomicMax)
__device__ __forceinline__ unsigned long long dbl_key(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_dbl(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

void launch_curvature_valid(const void* d_xyz, bool f32, size_t n_scans, const ExtractParams& P, double* d_curv,
                            uint8_t* d_mask, hipStream_t s);
// fz != nullptr: the selection may also write the final feature arrays (returns true if it did: no
// launch_compact needed); otherwise, or when it returns false, stage + counts only.
bool launch_select(const double* d_curv, const uint8_t* d_mask, size_t n_scans, const ExtractParams& P,
                   const ExtractStage& st, const ExtractFused* fz, hipStream_t s, bool* rows_ran = nullptr);
// will launch_select run the kernel that fills ExtractFused::box_* (select_rows_kernel with the fused compaction)?
bool launch_select_takes_boxes(const ExtractParams& P);
// edge_stride / planar_stride: entries per scan in the output arrays
// rows a5-a10 in one kernel (extract_fused_kernel); false: not applicable to these parameters, nothing was launched
bool launch_extract_fused(const void* d_xyz, bool f32, size_t n_scans, const ExtractParams& P, const ExtractStage& st,
                          const ExtractFused& fz, double* d_curv, uint8_t* d_mask, hipStream_t s);
// rows a5-a10 in one kernel, four scan lines per wavefront (opt-in: context option FUSED_ROWS). false: not requested or not
// applicable to these parameters, nothing was launched
bool launch_extract_rows_fused(const void* d_xyz, bool f32, size_t n_scans, const ExtractParams& P, const ExtractStage& st,
                               const ExtractFused& fz, double* d_curv, uint8_t* d_mask, hipStream_t s);
// the tie path: scan lines the selection kernel marked are redone in the reference's std::sort order (stage + counts)
bool launch_extract_split_ok(const ExtractParams& P, size_t n_scans);
void launch_extract_init(unsigned long long* line_tot, size_t n_tot, unsigned long long* box_min, unsigned long long* box_max, size_t n_box,
                         hipStream_t s);
void launch_replay(const double* d_curv, const uint8_t* d_mask, size_t n_scans, const ExtractParams& P, const ExtractStage& st,
                   const ExtractFused& fz, hipStream_t s);
// only_if != nullptr: every workgroup first reads *only_if and leaves if it is 0 (the fused compaction's fallback)
void launch_compact(const void* d_xyz, bool f32, size_t n_scans, const ExtractParams& P, const ExtractStage& st,
                    uint32_t* d_edge_idx, uint32_t* d_n_edge, double* d_edge_xyz, size_t edge_stride,
                    uint32_t* d_planar_idx, uint32_t* d_n_planar, double* d_planar_xyz, size_t planar_stride,
                    hipStream_t s, const uint32_t* only_if = nullptr, unsigned long long* fallback_counter = nullptr);

/* ---- registration (register_kernels.hip) ------------------------------------------------------- */
constexpr int kEdge = 0, kPlane = 1;  // feature kinds, in the order of loamx_target_index, kAssocEdges / kAssocPlanes and n_assoc[8 * pair + ...]
struct RegKindConfig {
  // (members in the order at which the queue kernels keep their scalar-register spill counts: allocation follows the kernel argument's layout)
  int k;        // neighbours searched
  double r;     // search radius
  int min_pts;  // fewest neighbours inside the radius a line / plane fit takes
  double pass;  // knn_radius_pass_max(r): largest squared distance that passes the strict radius filter
};
struct RegConfig {
  RegKindConfig kind[2];
  double min_line_cond, max_avg_plane_dist;
  uint32_t max_iterations;
  double rot_thresh, pos_thresh;
  uint32_t min_associations;
  uint32_t flags;  // the context's switches (loamx_ctx_set_option): kRegFlag*
};
constexpr uint32_t kRegFlagNoMoments = 1u;     // never use the moments: every evaluation streams the records
constexpr uint32_t kRegFlagNoPackedGrid = 2u;  // scan-sized sets through the single-workgroup index build with the 32-bit table
constexpr uint32_t kRegFlagNoBigGrid = 4u;     // map-sized sets through the single-workgroup build as well
constexpr uint32_t kRegFlagNoGridSide = 8u;    // source index builds behind the target builds on the context stream
constexpr uint32_t kRegFlagPoison = 16u;       // registration scratch starts as 0xFF bytes
constexpr uint32_t kRegFlagQueueTwoStage = 32u;  // queue chain: always lean 5x5x5 search + listed leftovers (launch_associate)
constexpr uint32_t kRegFlagQueueOneStage = 64u;  // queue chain: always the FP64 search over all rounds in one kernel
constexpr uint32_t kRegFlagForceRccl = 256u;     // a one-rank communicator really enqueues ncclAllGather / ncclBroadcast / ncclAllReduce (host side only)
constexpr uint32_t kRegFlagNoCoopLeft = 512u;    // listed queue leftovers one lane per query (associate_knn_left_kernel, round 3), not one wavefront per query
constexpr uint32_t kRegFlagNoCoopRows = 131072u;  // plain leftovers of a lean set one wavefront per query too (associate_knn_coop_kernel until round 10), not one row of lanes
constexpr uint32_t kRegFlagNoRefMoments = 1024u;  // first ICF iteration as in round 3: five sweeps of the records, no moments
constexpr uint32_t kRegFlagNoSmallSets = 8192u;     // edge-sized sets through grid_build_kernel like every other set
constexpr uint32_t kRegFlagCheckFinite = 4096u;     // the "_dev" entry points look for non-finite input coordinates first (host side only)
constexpr uint32_t kRegFlagNoExtractBoxes = 2048u;  // the index builds take their bounding boxes themselves even when the extraction left them
constexpr uint32_t kRegFlagNoMixedAssoc = 128u;  // edge and plane first kernels as separate launches on two streams (launch_associate)
constexpr uint32_t kRegFlagNoLiveDeal = 32768u;   // ICF iterations 3+: every pair keeps its place in the grids (xcd_pair_map), finished or not — no deal of the live pairs (xcd_live_map)
constexpr uint32_t kRegFlagForceLate = 16384u;    // plane fit of the mixed launch: every selection it has to verify is refused (all of them take the late list: associate_fit_late_kernel)

// One target feature set's spatial index (device pointers into the workspace)
struct GridSet {
  GridDesc* desc;        // [n_pairs]
  uint32_t* cell_start;  // [n_pairs][kGridCellsCap + 1]
  GridPoint* sorted;     // [n_pairs][stride] points re-ordered cell by cell (32 B each: xyz + original index)
  size_t stride;
  float* rel;            // [n_pairs][3][stride] single-precision offsets of the sorted points from the grid origin
                         // (x plane, y plane, z plane) for the FP32 pre-selection; nullptr for source sets
  uint32_t cells_cap;    // 0: kGridCellsCap. A persistent index of a map-sized set (one "pair") may own a larger
                         // cell table: a million-point map at the scan's cell edge puts hundreds of points in a cell
};

// What the registration holds once per feature kind (RegBatch::kind[kEdge], [kPlane]).
// Association records: structure-of-arrays over the whole batch (field-major) so the residual
// sweep streams each field with fully coalesced 8-byte loads.
//   edges : 9 fields (moved point xyz, line a xyz, line b xyz) x n_pairs x stride
//   planes: 7 fields (moved point xyz, normal xyz, d)          x n_pairs x stride
// An invalid slot has NaN in field 0.
struct RegKind {
  size_t stride;  // capacity (points) of one feature set; also the slot pitch of the association / grid arrays
  // Input feature sets of pair p start at base + p * in_pitch * stride * 3 and their counts at n[p * in_pitch] (RegBatch::in_pitch)
  const double* src;
  const uint32_t* n_src;
  const double* tgt;
  const uint32_t* n_tgt;
  GridSet grid;      // target sets: searched
  GridSet src_grid;  // source sets: only their cell-sorted order is used (coherent queries)
  uint32_t knn_mode;      // 0: grid and brute-force k-NN kernels both launched (target sizes on both sides of kBruteMax, or
                          // unknown); 1: grid only; 2: brute force only
  uint32_t assoc_blocks;  // workgroups per pair of the association kernels; 0xFFFFFFFF = by capacity
  double* rec;        // [9 | 7][n_pairs * stride] association records
  uint32_t* nn;       // [1 + kMaxK][n_pairs * stride] neighbour count, then positions in the sorted target
  uint32_t* rnn;      // as nn, for the queued queries, indexed by queue position
  uint32_t* nearest;  // [n_pairs * stride] nearest target index (detail capture)
  uint32_t* rest;     // [n_pairs * stride] queue of the queries round 1 of the k-NN did not finish
  uint32_t* exact;    // queue of the queries the keyed collector could not decide (exact collector re-runs them)
};

// The pairs that go on, listed on the device at the end of an ICF iteration for the kernels of the next one (xcd_map.h:
// xcd_live_map). Two lists, used alternately: the kernels of iteration i read list i % 2 while its solve fills list (i + 1) % 2.
// A list counts only while its stamp is the iteration that reads it; everything else — the first two iterations, an association
// pass outside a solve, the next call — finds no stamp of its own and places by xcd_pair_map.
// Where the lists exist, a list's entry count IS the count of the pairs that go on (RegBatch::n_active without them): one atomic
// per pair gives the pair its place in the list, and the host reads n[(it + 1) % 2] behind iteration it (RegBatch::live_count).
struct LiveLists {
  uint32_t iter;      // ICF iterations begun in this call: state_init_kernel 0, lm_begin_kernel + 1 (behind the association kernels)
  uint32_t n[2];      // entries of list 0 / 1 (outer_update_pair)
  uint32_t stamp[2];  // the iteration list 0 / 1 is for; 0: none (lists are for iterations >= kLiveFirstIter)
  uint32_t pad[3];
  // uint32_t pairs[2][n_pairs] behind it (RegBatch::live_pairs)
};
constexpr uint32_t kLiveFirstIter = 2u;  // (until then next to every pair goes on: the deal would only shuffle them)

struct PairState {
  double est[7];
  LmState lm;
  uint32_t active;       // outer loop still running
  uint32_t termination;
  uint32_t iterations;
  uint32_t first_sweep;  // next sweep is the iteration-0 evaluation
  uint32_t stream_planes;  // 1: the next sweep streams this pair's plane records (its moments cannot stand in for them)
  uint32_t use_moments;    // this ICF iteration runs the moment pass for the pair
  // First ICF iteration (round 4): after its first evaluation (a sweep at the identity update) the moments are taken
  // relative to the first candidate instead of the identity: mom_ref_on = 1, mom_ref = that candidate (lm_step_pair)
  uint32_t mom_ref_on;
  double mom_ref[7];
};

constexpr int kSweepThreads = 256;
#ifndef LOAMX_SWEEP_ITEMS
#define LOAMX_SWEEP_ITEMS 16  // measured per launch: 4 -> 0.268 ms, 8 -> 0.179, 16 -> 0.148 (56 % of HBM peak), 32 -> 0.150, 64 -> 0.206
#endif
constexpr int kSweepItems = LOAMX_SWEEP_ITEMS;  // association slots per thread
constexpr int kSweepChunk = kSweepThreads * kSweepItems;
// what lm_pair_loop_kernel keeps in LDS for the length of a pair's solve (register_kernels.hip: light_eval)
constexpr uint32_t kEdgeCache = 320;   // records (9 doubles each: 23 KB); a scan yields ~290 edge features
constexpr uint32_t kListCache = 64;    // moment tiles of a pair (4 per chunk of kSweepChunk slots)
constexpr uint32_t kFlatCache = 192;   // records (7 doubles each: 10.5 KB); more than that: the tile-by-tile walk

struct RegBatch {
  size_t n_pairs;
  uint32_t in_pitch;  // 1 for separate input arrays, 2 when source and target scans are interleaved (RegKind::src)
  RegKind kind[2];
  const double* init;  // may be null
  GridPoint* sort_scratch;      // [n_pairs][largest stride] scratch of the multi-workgroup target builds
  GridPoint* sort_scratch_src;  // the same for the ordered source builds (they run next to the target builds on another stream)
  uint32_t* n_assoc;  // [n_pairs][8]: valid edge / plane associations of the current iteration [0,1], lengths of the
                      // queues rest [2,3] and exact [4,5]
  PairState* state;      // [n_pairs]
  double* partials;      // [n_pairs][blocks_per_pair][kAccSize]
  double* mom_partials;  // [n_pairs][mom_blocks_per_pair][4][kMomSize + 2] wavefront tiles of the moment pass
  double* moments;       // [n_pairs][kMomSize + 2] plane moment matrix (16x16), max |s0|, max |v|^2 (reg_math.h)
  uint32_t mom_blocks_per_pair;
  uint32_t* flagged_list;   // [n_pairs][mom_blocks_per_pair][4 wavefronts][kSweepChunk / 4] plane slots the moments leave out, in slot order
  uint32_t* flagged_count;  // [n_pairs][mom_blocks_per_pair][4]
  uint32_t blocks_per_pair;
  uint32_t* n_active;    // device counter read back by the host after every outer iteration (with live lists: live_count)
  unsigned long long* sweep_slots;  // [0,1] edge / plane association slots streamed by sweep_kernel (roofline bytes);
                                    // [2,3] assoc_slots; [4] plane slots streamed by the moment pass
  unsigned long long* assoc_slots;  // [2] edge / plane source features processed by associate_kernel
  unsigned long long* grid_bytes;   // roofline bytes of the single-workgroup index builds (may be null)
  loamx_iter_info* iter_info;  // optional [n_pairs][max_iterations]
  uint32_t* max_counts;   // [6] over the active pairs (state_init_kernel; read back by the host): largest source edge / planar
                          // count, largest target edge / planar count, smallest target edge / planar count
  uint32_t want_nearest;  // 1: a detail hook will read RegKind::nearest (RegistrationDetail pairs); 0: the fit kernels skip that write
  uint32_t ref_moments;   // 1: the first ICF iteration takes its moments at its first candidate after ONE sweep (enqueue_icf_iteration)
  // optional: bounding boxes of the input feature sets, computed by the extraction that produced them (ExtractFused::box_*):
  // [scan][kind][axis] keys, scan = pair * in_pitch (+ src_box_offset for the pair's source scan). Used by the index builds
  // in place of their own read pass while *box_bad == 0; nullptr: the builds compute the boxes.
  const unsigned long long* box_min;
  const unsigned long long* box_max;
  const uint32_t* box_bad;
  uint32_t src_box_offset;  // scans from a pair's target box to its source box (1: the source scan lies one scan behind the target
                            // scan, in interleaved pairs and in a sequence alike); 0: the source sets have no boxes
  LiveLists* live;       // null: no deal of the live pairs (fewer than 8 pairs, NO_LIVE_DEAL)
  // the device counter of the pairs that go on after ICF iteration `it` of the call, for the host's read-back
  const uint32_t* live_count(uint32_t it) const { return (live && it + 1u >= kLiveFirstIter) ? &live->n[(it + 1u) & 1u] : n_active; }
  uint32_t* live_pairs;  // [2][n_pairs]
  uint32_t want_nn_counts;  // 1: an association dump will read the verified neighbour counts fit_one leaves in RegKind::nn (reg_dump)
  uint32_t small_edge_sets;  // 1: pairs whose TARGET edge set holds at most kBruteMax points get both edge sets from small_sets_build_kernel;
                             // 2: the target is a persistent index whose edge set is that small: every source edge set in its given order
};

// scratch the multi-workgroup build of a map-sized target set needs per pair (at B.sort_scratch + pair * stride points)
// (box keys, one cursor per cell, the tile sums of the table scan)
constexpr size_t kGridBigScratchBytes = 64 + ((size_t)kGridCellsCap + kGridCellsCap / 4096 + 8) * sizeof(uint32_t);
// cell table of a map-sized persistent index. Measured on a 1.02 M-point map (config 5; index build / registration
// of a 39 k-feature scan): 2^16 cells 1.04 / 6.71 ms, 2^17 1.07 / 5.97, 2^18 1.38 / 5.88, 2^19 1.77 / 5.71,
// 2^20 2.49 / 5.74, 2^21 4.75 / 8.19 (cells too small for the 5th neighbour: more second rounds)
constexpr uint32_t kGridSmallCap = 20480;  // sets up to this size are indexed by the packed single-workgroup build (no scratch)
constexpr uint32_t kBruteMax = 512;  // target sets up to this size are searched by associate_knn_brute_kernel
constexpr uint32_t kGridMapCellsCap = 1u << 18;
// scan-sized sets (the capacity bounds the count) take the packed cell table + LDS lists and need no scratch copy;
// the workspace is sized with the same predicate the launcher routes by
inline bool grid_small(size_t stride, uint32_t reg_flags) { return stride <= kGridSmallCap && !(reg_flags & kRegFlagNoPackedGrid); }
void launch_grid_build_targets(const RegBatch& B, const RegConfig& C, hipStream_t s);
void launch_grid_build_sources(const RegBatch& B, const RegConfig& C, hipStream_t s);
// What the launcher chose for a target build, reported where it chooses the kernel (loamx_target_index_census hands it on: a
// read-out, never a second copy of grid_small / grid_big). form: LOAMX_INDEX_BUILD_* of loamx.h.
constexpr uint32_t kGridBuildNone = 0u, kGridBuildPacked = 1u, kGridBuildSingle = 2u, kGridBuildBig = 3u;
struct GridBuildForm {
  uint32_t form;
  uint32_t unit_cells;        // cells per LDS pass of the single-workgroup kernels / table entries per scan tile of the gridbig_* kernels
  uint32_t table_min_points;  // the kernel writes the cell table of a set of at least this many points (0: of every set)
};
GridBuildForm launch_grid_build_target(const RegBatch& B, const RegConfig& C, int kind, hipStream_t s);  // one feature kind
void launch_grid_build_source(const RegBatch& B, const RegConfig& C, int kind, hipStream_t s);
void launch_state_init(const RegBatch& B, const RegConfig& C, hipStream_t s);
// The association census of an association dump (loamx_ctx_last_assoc_census). Per feature kind: what
// launch_associate chose, noted at the branch that chooses it (a read-out, never a second copy of a predicate), and the
// device words assoc_census_kernel fills at the two points of the chain whose words later kernels overwrite. Only reg_dump
// hands one to launch_associate: no other caller launches anything for it.
struct AssocCensusForm {
  uint32_t search;           // LOAMX_ASSOC_SEARCH_*: bit 0 the brute-force kernel was launched, bit 1 the grid kernel
  uint32_t km;               // neighbour slots of the instantiation (5 / 8 / 16)
  uint32_t mixed_launch;     // the first kernels of both kinds ran as ONE launch each
  uint32_t one_stage;        // queue_one_stage's answer (0 where no queue chain was launched)
  uint32_t leftover_kernel;  // LOAMX_ASSOC_LEFTOVER_*
  uint32_t rest_blocks, coop_blocks;  // workgroups per pair of the queue kernels / of the cooperative kernel (0: not launched)
};
struct AssocCensusBuf {
  uint32_t* counts;     // [8] zeroed by the caller: [0..2] verified / unverified / queued count words behind round 1,
                        // [3] negative counts behind associate_knn_rest_kernel, [4] in front of associate_fit_queued_kernel,
                        // [5] / [6] listed entries associate_knn_coop_kernel gave a row of lanes / a whole wavefront
  int32_t* after_rest;  // [stride] the counts by queue position behind associate_knn_rest_kernel ...
  int32_t* before_fit;  // ... and in front of associate_fit_queued_kernel
};
struct AssocCensusRun {
  AssocCensusForm form[2];
  AssocCensusBuf buf[2];
};
// what the queue kernels decide from a queue's length and its entries, through the functions the kernels themselves call:
// out = {rest_spread, left_spread, lean_set, rest_searched}; rest = the queue's `queued` entries (host copy)
void assoc_census_derive(const AssocCensusForm& F, size_t n_pairs, const GridDesc& g, const uint32_t* rest, uint32_t queued, uint32_t listed,
                         uint32_t out[4]);
// aux == nullptr: everything on s; aux2 == nullptr: the plane queue chain follows the edge chain on aux
// knn_scope != nullptr: the plane round-1 k-NN kernel is launched with that timing scope attached
// census != nullptr (reg_dump, one pair): the choices are noted in census->form and assoc_census_kernel reads the chain's words
constexpr uint32_t kAssocEdges = 1u, kAssocPlanes = 2u;
void launch_associate(const RegBatch& B, const RegConfig& C, hipStream_t s, hipStream_t aux, hipStream_t aux2, hipEvent_t ev_fork,
                      hipEvent_t ev_mid, hipEvent_t ev_join, hipEvent_t ev_join2, LaunchScope* knn_scope = nullptr,
                      uint32_t what = kAssocEdges | kAssocPlanes, AssocCensusRun* census = nullptr);
#ifdef LOAMX_NN_SAME_STATS
void debug_nn_same(const RegBatch& B, uint32_t it, hipStream_t s);
#endif
void launch_lm_begin(const RegBatch& B, const RegConfig& C, hipStream_t s);
void launch_sweep(const RegBatch& B, hipStream_t s);
void launch_lm_pair_loop(const RegBatch& B, const RegConfig& C, hipStream_t s);
void launch_lm_step(const RegBatch& B, hipStream_t s);
void launch_moments(const RegBatch& B, hipStream_t s);
void launch_outer_update(const RegBatch& B, const RegConfig& C, hipStream_t s);
void launch_write_results(const RegBatch& B, loamx_reg_result* d_results, hipStream_t s);

// incremental insert into a persistent index whose grid stays (register_kernels.hip); `cells` = entries of the cell table
size_t index_insert_ws_bytes(size_t cells, size_t n_add);
void launch_index_insert_count(const GridSet& gs, size_t cells, const double* d_add, uint32_t n_add, void* ws, hipStream_t s);
void launch_index_insert_merge(const GridSet& gs, size_t cells, uint32_t n_old, const double* d_add, uint32_t n_add, void* ws,
                               GridPoint* sorted2, float* rel2, hipStream_t s);

// direct read-outs of rows a16-a19 (loamx_fit_lines / _planes, loamx_knn_search, loamx_associate)
constexpr int kFitMaxK = 32;  // point sets of the host-callable fits (the association kernels keep <= kMaxK neighbours)
struct AssocDumpSet {  // device arrays of one feature kind, indexed by the caller's source index
  uint32_t* nn_count;  // [n_src]
  uint32_t* nn_idx;    // [n_src][k]
  uint8_t* valid;      // [n_src]
  double* moved;       // [n_src][3]
  double* prim;        // [n_src][6] line a, b | [n_src][4] plane normal, d
};
void launch_fit_sets(bool plane, const double* d_pts, size_t n_sets, int k, double* d_prim, double* d_aux, hipStream_t s);
void launch_knn_queries(const GridSet& gs, const double* d_q, size_t n_q, int k, double max_dist, uint32_t* d_idx, uint32_t* d_count,
                        hipStream_t s);
void launch_assoc_dump(const RegBatch& B, const RegConfig& C, const AssocDumpSet (&out)[2], hipStream_t s);

/* ---- registration information matrix (info_kernels.hip; arithmetic: info_math.h) -------------------------------- */
// what information_kernel leaves per (pair, chunk of the pair's association slots): the 21 + 6 + 1 sums of info_math.h
// (InfoAcc::s) and the counters n_edge, n_plane, n_huber, n_dropped
struct InfoPartial {
  double s[28];
  uint32_t c[4];
};
uint32_t info_blocks_per_pair(size_t edge_stride, size_t plane_stride);  // partials per pair at these capacities
// marks every pair active for ONE more association pass (the association kernels leave at once for a pair that has stopped);
// est, termination and iterations are not touched
void launch_info_activate(const RegBatch& B, hipStream_t s);
// behind launch_associate: partials[n_pairs][info_blocks_per_pair], one record per pair
void launch_information(const RegBatch& B, InfoPartial* partials, loamx_reg_information* d_info, hipStream_t s);

/* ---- non-finite input check of the "_dev" entry points (context option CHECK_FINITE; synth_kernels.hip) --------- */
// sets of `stride` points, `pitch` sets apart; d_n: points held by set i at d_n[i * pitch], or nullptr = all `stride`
void launch_check_finite(const void* d_pts, bool f32, const uint32_t* d_n, size_t n_sets, size_t stride, uint32_t pitch, uint32_t* d_flag,
                         hipStream_t s);
void launch_check_finite_scalars(const double* d_v, size_t n_scalars, uint32_t* d_flag, hipStream_t s);

/* ---- scan sequences (sequence_kernels.hip): trajectory of the per-pair results, motion correction of scans ------ */
// column blocks per scan (blockIdx.x = scan * col_blocks + column block), shares of the lines (gridDim.y), lines per share (the
// last share may hold fewer), lines a thread keeps in flight; all 0 but the last for an empty call
struct DeskewGeometry {
  uint32_t col_blocks, groups, lines_per_block, unroll;
};
DeskewGeometry deskew_launch_geometry(size_t n_scans, uint32_t H, uint32_t W);
void launch_deskew(const void* d_xyz, void* d_out, bool f32, size_t n_scans, uint32_t H, uint32_t W, const double* d_motion, double rho,
                   hipStream_t s);
void launch_trajectory(const loamx_reg_result* d_results, size_t n_pairs, const double origin[7], double* d_world_T_scan, hipStream_t s);

/* ---- unordered clouds into scans (organize_kernels.hip; the rule: organize_math.h and loamx.h) -------------------------- */
constexpr uint32_t kOrgChunkClouds = 256;  // clouds per launch: their offsets travel as a kernel argument (no staging copy)
// the clouds of one launch: cloud c holds the points off[c] .. off[c + 1] - 1 of the call's array
struct OrgOffsets {
  unsigned long long off[kOrgChunkClouds + 1];
};
// words of a cloud's counters in the workspace (filled is written by the gather, the finish kernel derives the collisions)
enum { kOrgFilled = 0, kOrgInvalid = 1, kOrgOutside = 2, kOrgCounterWords = 4 };
// One chunk of at most kOrgChunkClouds clouds, max_points = its largest cloud (> 0). winner: n_clouds x H W words, range (only
// when `nearest`): as many 64-bit words, both set to 0xFF bytes by the caller; cell (only when `nearest`): one word per point of
// the chunk; counters: n_clouds x kOrgCounterWords zeroed words. d_scans / d_src_idx / d_stats: the chunk's share of the outputs.
void launch_organize(const void* d_points, bool f32, uint32_t stride, const uint16_t* d_rings, const OrgOffsets& offs, uint32_t n_clouds,
                     unsigned long long max_points, const OrgTables& L, bool nearest, uint32_t* winner, unsigned long long* range,
                     uint32_t* cell, uint32_t* counters, void* d_scans, uint32_t* d_src_idx, uint32_t* d_stats, hipStream_t s);

}  // namespace loamx
// a scan layout (api_organize.hip creates and frees it; api_visibility.hip reads its shape and device tables)
struct loamx_scan_layout {
  int device = 0;
  uint32_t H = 0, W = 0, clockwise = 0, keep = 0;
  std::vector<double> col_dirs, line_tans;  // the uploaded bytes (loamx_scan_layout_tables)
  std::vector<uint16_t> ring_map;
  double* d_col_dirs = nullptr;
  double* d_line_tans = nullptr;
  uint16_t* d_ring_map = nullptr;
};
namespace loamx {

/* ---- place recognition (place_kernels.hip; the rule: place_math.h and loamx.h) ---------------------------------------------- */
constexpr uint32_t kPlaceSelectChunk = 1024;  // records a workgroup of the selection ranks at once
// one candidate of the key stage: squared key distance and entry id (kPlaceNoKeyDist / kPlaceNoId: none)
struct PlaceCand {
  unsigned long long dist;
  uint32_t id, pad;
};
// the stored entries of a database as the kernels read them
struct PlaceEntries {
  const uint16_t* desc;             // [n][R S]
  const uint32_t* keys;             // [n][R]
  const unsigned long long* norms;  // [n][S]
  uint32_t n;
};
// One chunk of at most kOrgChunkClouds clouds, max_points = its largest cloud. table: n_clouds x R S zeroed words;
// d_desc: the chunk's share of the output.
void launch_place_descriptors(const void* d_points, bool f32, uint32_t stride, const OrgOffsets& offs, uint32_t n_clouds,
                              unsigned long long max_points, const PlaceShape& P, const double* d_dirs, uint32_t* table, uint16_t* d_desc,
                              hipStream_t s);
// ring keys [n][R] and column norms [n][S] of n descriptors
void launch_place_keys(const uint16_t* d_desc, size_t n, const PlaceShape& P, uint32_t* d_keys, unsigned long long* d_norms, hipStream_t s);
// chunks of the key stage's first pass over n_entries entries (>= 1) and the records its passes leave per query in each of the
// two buffers at most
uint32_t place_select_chunks(uint32_t n_entries);
size_t place_select_records(uint32_t n_entries, uint32_t K);
// the id_end of the queries of one launch: they travel as a kernel argument like OrgOffsets (no staging copy of a host array)
constexpr uint32_t kPlaceIdEndQueries = 256;
struct PlaceIdEnd {
  uint32_t v[kPlaceIdEndQueries];
  uint32_t given;
};
// The K entries nearest by (key distance, id) among those with id < min(E.n, id_end[q]) for n_queries queries (id_end: HOST
// array or nullptr; with one, n_queries <= kPlaceIdEndQueries); the result, ascending, stands in the buffer the function
// returns (one of the two given).
PlaceCand* launch_place_key_stage(const PlaceEntries& E, const PlaceShape& P, const uint32_t* d_qkeys, const uint32_t* id_end, uint32_t n_queries,
                                  uint32_t K, PlaceCand* buf_a, PlaceCand* buf_b, hipStream_t s);
// the shift distance of every candidate, then the records of each query ascending by (distance, id) in d_out
void launch_place_shift_stage(const PlaceEntries& E, const PlaceShape& P, const uint16_t* d_qdesc, const unsigned long long* d_qnorms,
                              const PlaceCand* cands, uint32_t n_queries, uint32_t K, loamx_place_match* d_tmp, loamx_place_match* d_out,
                              hipStream_t s);

// arrays carved out of one device block start on 256-byte boundaries (the pose graph's workspace, the maps' blocks and outputs)
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

/* ---- pose graph (posegraph_kernels.hip; the rule: posegraph_math.h and loamx.h) ----------------------------------------------- */
// byte offsets of a solve's arrays in its one workspace block (every array starts on a 256-byte boundary)
struct PgoLayout {
  size_t state;                    // PgoState[2]
  size_t zeroed, zeroed_bytes;     // the bad-edge count and the degrees: zeroed before every solve
  size_t off, cursor, list, fixed;
  size_t blocks, pose_blocks;
  size_t vec[6];                   // x, r, z, q, p[0], p[1]
  size_t cand;
  size_t cost_part, cand_cost_part, rz_part, pq_part, max_part;
  size_t bytes;
};
PgoLayout pgo_layout(size_t n_poses, size_t n_edges);
// the whole solve, enqueued: n_poses, n_edges >= 1 and < 2^31, params checked by the caller; ws: pgo_layout(...).bytes
void launch_pgo_solve(double* d_poses, size_t n_poses, const uint8_t* d_fixed, const loamx_pgo_edge* d_edges, size_t n_edges,
                      const loamx_pgo_params& params, loamx_pgo_summary* d_summary, void* ws, hipStream_t s);
void launch_pgo_nothing(const loamx_pgo_params& params, loamx_pgo_summary* d_summary, hipStream_t s);
size_t pgo_readout_ws_bytes(size_t n_edges);
void launch_pgo_linearize_readout(const double* d_poses, const loamx_pgo_edge* d_edges, size_t n_edges, double huber_delta,
                                  loamx_pgo_linearization* d_lin, double* cost_part, hipStream_t s);
void launch_pgo_edges_from_results(const loamx_reg_result* d_results, const loamx_reg_information* d_info, size_t n_pairs, uint32_t first_id,
                                   loamx_pgo_edge* d_edges, hipStream_t s);

/* ---- map upkeep (map_kernels.hip): voxel filter against an occupancy table, crop, the stable compaction they share --- */
constexpr uint32_t kMapTile = 256;             // points per tile of the compaction (one workgroup)
constexpr uint32_t kMapNoSlot = 0xFFFFFFFFu;   // slot of a point that has no voxel (or whose probe gave up)
// words of the flag array the claim kernel raises (zeroed by the caller, read back by the host entry points)
enum { kMapFlagGaveUp = 0, kMapFlagBadPoint = 1, kMapFlagBadMapPoint = 2, kMapFlagWords = 4 };
// Open-addressed occupancy table: 2^log2_cap slots, keys[slot] = voxel key (map_math.h) or all ones (empty), owner[slot] =
// lowest index of a point in that voxel (all ones before the first claim). Both arrays start as 0xFF bytes.
struct VoxelTable {
  unsigned long long* keys;
  uint32_t* owner;
  uint32_t log2_cap;
};
// log2 of the slots of a table (this one, the cloud map's, the occupancy map's) with room for slots_min: voxel_hash takes 4 .. 32 bits
inline uint32_t voxel_table_log2(size_t slots_min) {
  uint32_t l = 4;
  while (((size_t)1 << l) < slots_min) l++;
  return l;
}
void launch_voxel_claim(const double* d_pts, uint32_t n, const double* pose, double leaf, const VoxelTable& t, uint32_t base, double* d_moved,
                        uint32_t* d_slot, uint32_t* d_flags, uint32_t bad_word, hipStream_t s);
void launch_voxel_keep(const VoxelTable& t, const uint32_t* d_slot, uint32_t n, uint32_t base, uint8_t* d_keep, hipStream_t s);
void launch_crop_keep(const double* d_pts, uint32_t n, const double lo[3], const double hi[3], uint8_t* d_keep, hipStream_t s);
void launch_map_transform(const double* d_pts, uint32_t n, const double* pose, double* d_out, uint32_t* d_src_idx, uint32_t* d_n_out,
                          uint32_t* d_flags, hipStream_t s);
size_t map_compact_ws_bytes(size_t n);
void launch_map_compact(const double* d_in, const uint8_t* d_keep, uint32_t n, uint32_t* d_tiles, double* d_out, uint32_t* d_src_idx,
                        uint32_t* d_total, const VoxelTable* fix, const uint32_t* d_slot, uint32_t owner_base, hipStream_t s);

/* ---- cloud map and the listed voxel table it shares with the surfel map (cloudmap_kernels.hip, listed_kernels.hip,
 *      listed_accumulate.h; the rule: cloudmap_math.h and loamx.h) --------------------------------------------------------------- */
constexpr uint32_t kCloudChunkPoints = 1u << 22;  // points per round of launches of an add (its scratch is sized for them at create)
constexpr uint32_t kRegFlagNoCloudmapCombine = 65536u;  // (loamx_ctx::reg_flags) one claim per point, no run combining
// counter words of a map: [kCloudUsed .. kCloudOutside] of cloudmap_math.h, then the overflow and the claims (run heads: CAS
// chains begun); the rest pads the array to 64 bytes
enum { kCloudWordOverflow = 4, kCloudWordClaims = 5, kCloudWords = 8 };
// length words: voxels in the list; new voxels of the chunk in flight (the compaction's total)
enum { kCloudLenListed = 0, kCloudLenPending = 1, kCloudLens = 4 };
struct CloudRule {
  double leaf, min_r2, max_r2;
};
// The listed voxel table of the cloud map and of the surfel map. Open-addressed as VoxelTable: 2^log2_cap slots; keys and first start
// as 0xFF bytes, everything else as zero bytes. The 64-bit words of a slot are its owner's compile-time constant, not a field:
constexpr uint32_t kCloudSlotWords = 3;    // sums of the points' 32-bit offsets inside the voxel
constexpr uint32_t kSurfelSlotWords = 12;  // s[3], S[6], W[3] (surfel_math.h: kSurfelMoments)
struct ListedTable {
  unsigned long long* keys;     // [cap] voxel key (map_math.h) or all ones (empty)
  uint32_t* first;              // [cap] lowest running index of a point of the voxel
  unsigned long long* payload;  // [cap][words of a slot]
  uint32_t* count;              // [cap]
  uint32_t log2_cap;
  uint32_t max_voxels;
  uint32_t* list;               // [max_voxels] slots in order of first appearance
  unsigned long long* words;    // [kCloudWords]
  uint32_t* lens;               // [kCloudLens]
};
// Points p0 .. p0 + n - 1 of the call's array (0 < n <= kCloudChunkPoints), which lie in the clouds of `offs`; g0: the running
// index of point p0; d_poses: the pose of offs' first cloud onwards, or nullptr. d_slot: n words.
typedef void ListedAccumulate(const void* d_points, bool f32, uint32_t stride, const OrgOffsets& offs, uint32_t n_clouds, unsigned long long p0,
                              uint32_t n, uint32_t g0, const double* d_poses, const CloudRule& rule, const ListedTable& t, bool combine, uint32_t* d_slot,
                              hipStream_t s);
ListedAccumulate launch_cloud_accumulate, launch_surfel_accumulate;
// behind the accumulate of the same points: their new voxels join the list. d_keep: n bytes; d_tiles: map_compact_ws_bytes(n)
void launch_listed_list(const ListedTable& t, const uint32_t* d_slot, uint32_t n, uint32_t g0, uint8_t* d_keep, uint32_t* d_tiles, hipStream_t s);
// the first half of an emit: the flags of the listed voxels with at least min_points points, the tile offsets, *d_n_out their number.
// d_keep: max_voxels bytes; d_tiles: map_compact_ws_bytes(max_voxels)
void launch_listed_emit_flags(const ListedTable& t, uint32_t min_points, uint8_t* d_keep, uint32_t* d_tiles, uint32_t* d_n_out, hipStream_t s);
// the whole emit of the cloud map: the flags, then the centroids. Writes *d_n_out in every case.
void launch_cloud_emit(const ListedTable& t, double leaf, uint32_t min_points, uint8_t* d_keep, uint32_t* d_tiles, double* d_xyz_out,
                       uint32_t* d_count_out, uint32_t* d_first_out, size_t capacity, uint32_t* d_n_out, hipStream_t s);

/* ---- scan segmentation (segment_kernels.hip; the rule: segment_math.h and loamx.h) ------------------------------------------- */
constexpr uint32_t kSegTileLines = 16, kSegTileCols = 256;  // the tile a workgroup labels in LDS (loamx_ctx_last_segment_census)
constexpr uint32_t kSegMaxScans = 65535;                    // scans per call: the scan is the launch grid's y
constexpr uint32_t kSegStatWords = 8;
constexpr uint32_t kRegFlagNoSegmentTiles = 262144u;      // (loamx_ctx::reg_flags) every connected edge through the global union
constexpr uint32_t kSegBlock = 256;                         // cells per workgroup of the per-cell kernels (and per compaction block)
// scratch of one call, all per scan back to back (HW = H W cells, nb = ceil(HW / kSegBlock))
struct SegScratch {
  uint8_t* cls;         // [HW] kSegInvalid / kSegGround / kSegNode
  uint8_t* ebits;       // [HW] connected edges handed to the global merge: bit 0 right, bit 1 up
  uint32_t* parent;     // [HW] nodes only
  uint32_t* root;       // [HW] kSegNoLabel for the others
  uint32_t* size;       // [HW] at the roots
  uint32_t* line_max;   // [HW] at the roots
  uint32_t* block_cnt;  // [nb] accepted roots per block, then their exclusive prefix sum
  uint32_t* stats;      // [kSegStatWords], zeroed before the launch
  uint32_t* edges;      // [1] per scan: edges handed to the global merge, zeroed before the launch
};
struct SegOutputs {
  uint8_t* classes;
  uint32_t *labels, *sizes;
  void* filtered;  // the input's scalar type; may be the input itself
  loamx_segment_cluster* clusters;
  size_t max_clusters;
  uint32_t* stats;
};
void launch_segment(const void* d_scans, bool f32, uint32_t n_scans, const SegParams& P, bool tiles, const SegScratch& ws, const SegOutputs& out,
                    hipStream_t s);

/* ---- map cleaning (visibility_kernels.hip; the rule: visibility_math.h and loamx.h) ------------------------------------------------ */
constexpr uint32_t kVisScanChunk = 32;            // scans per workgroup row of the votes kernel (more when n_scans > 65535 x 32)
constexpr size_t kVisLdsTableBytes = 48u << 10;   // layout tables up to this size are staged in LDS
constexpr uint32_t kRegFlagNoVisibilityRanges = 524288u;  // (loamx_ctx::reg_flags) the window reads the scans' points, no first launch that writes every cell's squared range
inline size_t vis_table_bytes(uint32_t H, uint32_t W) { return (2 * (size_t)W + (size_t)H + 1) * sizeof(double); }
struct VisVotesCall {
  const double* d_points;
  uint32_t stride, n_points;
  const void* d_scans;
  bool f32;
  const double* d_ranges;  // n_scans x H W squared ranges (launch_visibility_ranges); nullptr: the window reads the scans
  uint32_t n_scans, chunk;
  const double* d_poses;
  OrgTables tab;
  VisRule rule;
  bool atomic;  // the counts are added to the votes (zeroed or kept by the caller); false: stored
  loamx_visibility_tally* d_votes;
  unsigned long long* d_census;  // [2] in-range pairs, projected pairs: added to
};
void launch_visibility_ranges(const void* d_scans, bool f32, unsigned long long n_cells, double min2, double* d_ranges, hipStream_t s);
void launch_visibility_votes(const VisVotesCall& c, hipStream_t s);
void launch_visibility_filter(const loamx_visibility_tally* d_votes, uint32_t n, uint32_t min_through, double through_ratio, const double* d_points,
                              uint32_t stride, uint8_t* d_keep, uint32_t* d_tiles, uint8_t* d_dynamic_out, double* d_xyz_out, uint32_t* d_index_out,
                              size_t capacity, uint32_t* d_n_out, hipStream_t s);

/* ---- occupancy map (occupancy_kernels.hip; the rule: occupancy_math.h and loamx.h) ------------------------------------------------ */
constexpr uint32_t kOccChunkRays = 1u << 30;                 // rays per launch of an add
constexpr uint32_t kRegFlagNoOccupancyCombine = 1048576u;   // (loamx_ctx::reg_flags) one claim per visit, no run combining
// counter words of a map (the rays offered are the host's)
enum {
  kOccWordHit = 0, kOccWordInvalid, kOccWordShort, kOccWordLong, kOccWordOutside, kOccWordVisits, kOccWordVoxels, kOccWordClaims,
  kOccWordOverflow, kOccWords = 16
};
// Open-addressed table as ListedTable: 2^log2_cap slots; keys start as 0xFF bytes, counts and words as zero bytes.
struct OccTable {
  unsigned long long* keys;    // [cap] voxel key (map_math.h) or all ones (empty)
  unsigned long long* counts;  // [cap] hits << 32 | passes
  unsigned long long* words;   // [kOccWords]
  uint32_t log2_cap;
};
// Rays p0 .. p0 + n - 1 of the call's array (0 < n <= kOccChunkRays), which lie in the clouds of `offs`; d_poses: the pose of
// offs' first cloud onwards, or nullptr
void launch_occupancy_walk(const void* d_points, bool f32, uint32_t stride, const OrgOffsets& offs, uint32_t n_clouds, unsigned long long p0,
                           uint32_t n, const double* d_poses, const OccRule& rule, const OccTable& t, bool combine, hipStream_t s);
// read-only, behind the walks on the same stream; the two outputs of the first two may each be nullptr
void launch_occupancy_query(const OccTable& t, double leaf, const OccStateRule& sr, const double* d_points, uint32_t stride, unsigned long long n,
                            uint32_t* d_counts_out, uint8_t* d_state_out, hipStream_t s);
struct OccBox {
  int32_t vmin[3];
  uint32_t dims[3];
};
void launch_occupancy_box(const OccTable& t, const OccStateRule& sr, const OccBox& box, uint32_t* d_counts_out, uint8_t* d_state_out, hipStream_t s);
void launch_occupancy_slice(const OccTable& t, const OccStateRule& sr, const OccBox& box, uint8_t* d_grid_out, hipStream_t s);

/* ---- occupancy distance field (distance_kernels.hip; the rule: distance_math.h and loamx.h) ----------------------------------------- */
constexpr uint32_t kRegFlagNoDistanceEarlyExit = 8388608u;  // (loamx_ctx::reg_flags) the y- and z-pass walk the whole window of +-R
// a call's box and what follows from it: the extended box e = dims + 2R (a slice: e[2] = 1, its columns take their state over
// `levels` levels) and W, the 64-bit mask words of a row
struct DistGeom {
  int32_t vmin[3];
  uint32_t dims[3];
  uint32_t e[3];
  uint32_t R, W, levels;
  uint32_t unknown_is_obstacle, slice;
};
DistGeom make_dist_geom(const int32_t* vmin, const uint32_t* dims, uint32_t R, bool unknown_is_obstacle, bool slice);
// the staging of a call in one block: the mask, the x-pass's offsets, the y-pass's dwords (a box only)
struct DistStaging {
  unsigned long long* mask;  // [e[2] e[1]][W]
  int16_t* dx;               // [e[2] e[1]][dims[0]]
  uint32_t* dxy;             // [e[2]][dims[1]][dims[0]]
};
DistStaging dist_staging_carve(void* block, const DistGeom& g, size_t* bytes);  // (block may be nullptr: only the size is wanted)
// mask, x, y (and z) on a box with no dimension of 0; each output may be nullptr. The table is only read.
void launch_distance(const OccTable& t, const OccStateRule& sr, double leaf, const DistGeom& g, const DistStaging& w, bool early, uint16_t* d_d2_out,
                     int16_t* d_offset_out, float* d_metres_out, hipStream_t s);

/* ---- occupancy ray casting (raycast_kernels.hip; the rule: raycast_math.h and loamx.h) ------------------------------------------------- */
constexpr uint32_t kRegFlagRaycastCombine = 16777216u;  // (loamx_ctx::reg_flags) one look-up per run of lanes in the same voxel; unset: every lane its own
// counter words of a call (the rays are the host's): tested visits, look-ups, then the rays by status in the order of LOAMX_RAY_*
enum { kRayWordVisits = 0, kRayWordProbes = 1, kRayWordStatus = 2, kRayCensusWords = kRayWordStatus + kRayStatuses };
// n > 0 segments origin -> end, `stride` doubles apart: one record each. The table is only read; d_census is added to.
void launch_raycast(const OccTable& t, double leaf, const OccStateRule& sr, const RayRule& rule, const double* d_origins, const double* d_ends,
                    uint32_t stride, unsigned long long n, RayRecord* d_records, unsigned long long* d_census, bool combine, hipStream_t s);
// the n_beams beams of d_dirs at each of n_poses poses (n_poses n_beams > 0 rays, pose-major); each output may be nullptr
void launch_raycast_render(const OccTable& t, double leaf, const OccStateRule& sr, const RayRule& rule, const double* d_dirs, uint32_t n_beams,
                           const double* d_poses, unsigned long long n_poses, double max_range, double* d_scans, double* d_ranges,
                           RayRecord* d_records, unsigned long long* d_census, bool combine, hipStream_t s);

/* ---- surfel map (surfel_kernels.hip; the rule: surfel_math.h and loamx.h) ----------------------------------------------------------- */
constexpr uint32_t kRegFlagNoSurfelCombine = 2097152u;  // (loamx_ctx::reg_flags) one claim per point, no run combining
// the table is a ListedTable of kSurfelSlotWords words per slot, with the cloud map's counter and length words; the add is
// launch_surfel_accumulate and launch_listed_list (above). The whole emit: the flags, then the records (skipped when only the
// number is asked for). Writes *d_n_out in every case.
void launch_surfel_emit(const ListedTable& t, double leaf, uint32_t min_points, uint8_t* d_keep, uint32_t* d_tiles, loamx_surfel* d_out,
                        double* d_xyz_out, double* d_normal_out, size_t capacity, uint32_t* d_n_out, hipStream_t s);
// read-only, behind the adds on the same stream; each output may be nullptr
void launch_surfel_query(const ListedTable& t, double leaf, uint32_t min_points, const double* d_points, uint32_t stride, unsigned long long n,
                         loamx_surfel* d_out, double* d_distance_out, uint32_t* d_count_out, hipStream_t s);

/* ---- surfel localisation (localize_kernels.hip; the rule: localize_math.h and loamx.h) ------------------------------------------- */
constexpr uint32_t kRegFlagNoLocalizePlanes = 4194304u;  // (loamx_ctx::reg_flags) no plane cache: every candidate through surfel_of_slot
struct LocPlane;   // localize_math.h
struct LocRule;
struct LocSolve;
struct LocState;
struct LocResult;
// what localize_accumulate_kernel leaves per (cloud, chunk of the cloud's points): the sums of info_math.h and the counters
struct LocPartial {
  double s[28];
  uint32_t c[8];
};
size_t localize_partials(size_t max_points);  // partials a launch of at most kOrgChunkClouds clouds and max_points points can write
// the plane cache (cache may be nullptr: the plain form) and the state of the call's n_clouds clouds from d_poses_in
void launch_localize_planes(const ListedTable& t, double leaf, uint32_t min_points, double planarity, LocPlane* cache, const double* d_poses_in,
                            uint32_t n_clouds, uint32_t max_iterations, LocState* state, hipStream_t s);
// one evaluation of the clouds of `offs` (at most kOrgChunkClouds, `largest` the points of the largest) at the poses of `state`
// (the state of offs' first cloud onwards); final_pass: clouds that have stopped are evaluated too
void launch_localize_accumulate(const void* d_points, bool f32, uint32_t stride, const OrgOffsets& offs, uint32_t n_clouds, unsigned long long largest,
                                const LocState* state, const LocRule& rule, const ListedTable& t, const LocPlane* cache, bool final_pass,
                                LocPartial* partials, hipStream_t s);
// behind it: one iteration of the solve per cloud, or (final_pass) the poses, result records and information records (d_info may be
// nullptr), each from offs' first cloud onwards
void launch_localize_step(const OrgOffsets& offs, uint32_t n_clouds, LocState* state, const LocSolve& P, const LocPartial* partials, bool final_pass,
                          double* d_poses_out, LocResult* d_results, loamx_reg_information* d_info, hipStream_t s);

/* ---- map window (crop_kernels.hip; the rule: crop_math.h and loamx.h) -------------------------------------------------------------- */
// One of the three voxel tables as the crop sees it: key slots, `payload_words` 64-bit words per slot, and what only the listed
// maps have (nullptr in the occupancy map, whose entries are its slots).
struct CropTable {
  unsigned long long* keys;     // [cap]
  unsigned long long* payload;  // [cap][payload_words]: the cloud map's sums, the surfel map's moments, the occupancy map's counts
  uint32_t* first;              // [cap] or nullptr
  uint32_t* count;              // [cap] or nullptr
  uint32_t* list;               // [entries] slots in order of first appearance, or nullptr: entry j is slot j
  uint32_t* listed;             // the list's length (lens + kCloudLenListed), nullptr without a list
  unsigned long long* voxels;   // the occupancy map's voxel counter (words + kOccWordVoxels), nullptr with a list
  uint32_t log2_cap, payload_words;
  uint32_t entries;             // max_voxels with a list, 2^log2_cap without
};
enum { kCropCtlKept = 0, kCropCtlSkip = 1, kCropCtlWords = 4 };
// the scratch of a crop (a handle's, allocated at its first crop): flags, tiles and control words, then the staged voxels
struct CropScratch {
  uint8_t* keep;                // [entries]
  uint32_t* tiles;              // map_compact_ws_bytes(entries)
  uint32_t* ctl;                // [kCropCtlWords]
  unsigned long long* keys;     // [entries]
  unsigned long long* payload;  // [payload_words][entries]
  uint32_t* first;              // [entries] (unused without CropTable::first)
  uint32_t* count;              // [entries]
};
size_t crop_scratch_bytes(const CropTable& t);
CropScratch crop_scratch_carve(void* block, const CropTable& t);
// six launches: flags, the two of the tile offsets, gather, reset, scatter (which also commits the length). d_pose, d_counts_out: may
// be nullptr.
void launch_voxel_crop(const CropTable& t, const CropScratch& w, double leaf, const double* d_pose, const double lo[3], const double hi[3],
                       uint32_t* d_counts_out, hipStream_t s);

/* ---- synthetic generator (synth_kernels.hip) --------------------------------------------------- */
void launch_synth_pairs(uint64_t seed, uint64_t first_pair, size_t n_pairs, uint32_t H, uint32_t W, double sigma,
                        double* d_xyz, hipStream_t s);

}  // namespace loamx
