// api_register.hip — registration: the pieces of the driver over device-resident feature sets (reg_prepare, then reg_solve /
// reg_dump / reg_information), the one-pair entry points from host memory, the fits and the k-NN search, the batch forms.
#include "api_host.h"

using namespace loamx;

namespace {

// the association kernels of one ICF iteration (all feature kinds, all chains), timed as LOAMX_K_ASSOC
int enqueue_association(loamx_ctx* ctx, const RegBatch& B, const RegConfig& C, uint32_t what = kAssocEdges | kAssocPlanes,
                        AssocCensusRun* census = nullptr) {
  hipStream_t s = ctx->stream;
  {
    TimedScope t(ctx, LOAMX_K_ASSOC, 0.0);
    // (a single scan-sized pair cannot fill the chip twice over: the forks and joins only add latency there —
    // one 64 x 1024 pair 1.15 ms with the auxiliary streams, 1.10 ms without; one 128 x 2048 scan against a
    // 1 M-point map the other way round: 5.9 vs 6.8 ms)
    const bool side = (size_t)B.n_pairs * B.kind[kPlane].assoc_blocks >= 128;
    // sub-scope: the plane round-1 k-NN kernel alone (events attached to its own dispatch)
    PendingEvent knn{};
    LaunchScope knn_ls{nullptr, nullptr, true};
    if (ctx->timing) {
      knn.kernel = LOAMX_K_KNN_PLANE, knn.bytes = 0.0, knn.own_e0 = true;
      knn.e0 = take_event(ctx), knn.e1 = take_event(ctx);
      knn_ls = LaunchScope{knn.e0, knn.e1, true};
    }
    launch_associate(B, C, s, side ? ctx->aux_stream : nullptr, side ? ctx->aux2_stream : nullptr, ctx->ev_fork, ctx->ev_mid, ctx->ev_join,
                     ctx->ev_join2, ctx->timing ? &knn_ls : nullptr, what, census);
    if (ctx->timing) {
      if (knn_ls.first) ctx->event_pool.push_back(knn.e0), ctx->event_pool.push_back(knn.e1);  // (kernel not launched)
      else ctx->pending.push_back(knn);
    }
  }
  CHECK_LAUNCH(ctx, "associate_kernel");
  return LOAMX_OK;
}

// the launch sequence of one ICF iteration on ctx->stream (+ the auxiliary streams); `it` only selects between the
// first iteration's sequence (no moment pass) and the later ones'
int enqueue_icf_iteration(loamx_ctx* ctx, const RegBatch& B, const RegConfig& C, uint32_t it, AfterAssocHook hook, void* hook_user) {
  hipStream_t s = ctx->stream;
  {
    const int rc_assoc = enqueue_association(ctx, B, C);
    if (rc_assoc != LOAMX_OK) return rc_assoc;
  }
#ifdef LOAMX_NN_SAME_STATS
  debug_nn_same(B, it, s);
#endif
  if (hook) {
    untimed(ctx);
    int rc = hook(ctx, B, it, hook_user);
    if (rc != LOAMX_OK) return rc;
  }
  {
    TimedScope t(ctx, LOAMX_K_LM, 0.0, true);
    launch_lm_begin(B, C, s);
  }
  // The first ICF iteration (state_init: stream_planes = 1, use_moments = 0): ONE sweep of the records at the identity update
  // and its bookkeeping step, which fixes the first candidate; the moments are then taken at that candidate and the solve
  // goes on as in the later iterations (round 4; until then five sweeps + five steps: 1.07 of the step's 11.3 ms).
  const bool ref_first = it == 0 && B.ref_moments != 0u;
  if (ref_first) {
    {
      TimedScope t(ctx, LOAMX_K_SWEEP, 0.0, true);
      launch_sweep(B, s);
    }
    TimedScope t(ctx, LOAMX_K_LM, 0.0, true);
    launch_lm_step(B, s);
  }
  if (it > 0 || ref_first) {
    TimedScope t(ctx, LOAMX_K_MOMENT, 0.0, true);
    launch_moments(B, s);
  }
  if (it > 0 || ref_first) {
    // one workgroup per pair runs the whole solve off the moments (and streams by itself whatever they cannot cover)
    TimedScope t(ctx, LOAMX_K_LM, 0.0, true);
    launch_lm_pair_loop(B, C, s);  // (ends with the pair's outer update)
  } else {
    for (int k = 0; k < 5; k++) {  // iteration-0 evaluation + max_num_iterations = 4 candidates
      {
        TimedScope t(ctx, LOAMX_K_SWEEP, 0.0, true);
        launch_sweep(B, s);
      }
      {
        TimedScope t(ctx, LOAMX_K_LM, 0.0, true);
        launch_lm_step(B, s);
      }
    }
  }
  CHECK_LAUNCH(ctx, "sweep/lm kernels");
  if (it == 0 && !ref_first) {  // (otherwise: inside lm_pair_loop_kernel; the active-pair counter is reset by lm_begin_kernel)
    TimedScope t(ctx, LOAMX_K_LM, 0.0, true);
    launch_outer_update(B, C, s);
  }
  CHECK_LAUNCH(ctx, "outer_update_kernel");
  return LOAMX_OK;
}

}  // namespace

namespace loamx {

int reg_prepare(loamx_ctx* ctx, const RegInputs& in, RegConfig& C, const loamx_target_index* prebuilt, const RegPrepareOpts& opts, RegBatch& B) {
  B = RegBatch{};
  ctx->last_solve_valid = false;  // (the workspace the solve readout points into may move below)
  ctx->last_assoc_census_valid = false;  // (the census is its own dump's: a later call of any kind ends it)
  if (in.n_pairs == 0) return LOAMX_OK;
  if (opts.one_pass && C.max_iterations == 0) C.max_iterations = 1;
  untimed(ctx);
  if (in.n_pairs > 0x7FFFFFFFull / 128) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "too many pairs in one call");
  const size_t np = in.n_pairs, es = in.kind[kEdge].stride ? in.kind[kEdge].stride : 1, ps = in.kind[kPlane].stride ? in.kind[kPlane].stride : 1;
  if (es > 0x3FFFFFFFull || ps > 0x3FFFFFFFull) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "feature set too large");  // (queue entries: 30-bit query index + 2 flags)
  B.n_pairs = np, B.in_pitch = in.in_pitch, B.init = in.init;
  for (int k = 0; k < 2; k++) {
    RegKind& K = B.kind[k];
    K.stride = k ? ps : es;
    K.src = in.kind[k].src, K.n_src = in.kind[k].n_src, K.tgt = in.kind[k].tgt, K.n_tgt = in.kind[k].n_tgt;
    K.grid.stride = K.stride + kGridPad, K.src_grid.stride = K.stride;  // (src_grid.rel stays null: source sets are not searched)
    K.assoc_blocks = 0xFFFFFFFFu, K.knn_mode = 0u;
  }
  if (!(C.flags & kRegFlagNoExtractBoxes)) B.box_min = in.boxes.min, B.box_max = in.boxes.max, B.box_bad = in.boxes.bad, B.src_box_offset = in.src_box_offset;
  B.blocks_per_pair = (uint32_t)((es + ps + kSweepChunk - 1) / kSweepChunk);
  B.mom_blocks_per_pair = (uint32_t)((ps + kSweepChunk - 1) / kSweepChunk);
  // The registration's scratch, each buffer described once: where it lives, its size, the RegBatch field it binds to. SCRATCH
  // allocates (one hipMalloc per buffer, grown as by ENSURE), fills with 0xFF bytes under DEBUG_POISON and binds.
  auto scratch = [&](Buf& b, size_t bytes, auto*& field) -> int {
    ENSURE(ctx, b, bytes);
    if ((C.flags & kRegFlagPoison) && b.p) HIP_TRY(ctx, hipMemsetAsync(b.p, 0xFF, b.cap, ctx->stream));
    field = reinterpret_cast<std::remove_reference_t<decltype(field)>>(b.p);
    return LOAMX_OK;
  };
#define SCRATCH(buf, bytes, field)                \
  do {                                            \
    int rc_ = scratch(buf, bytes, field);         \
    if (rc_ != LOAMX_OK) return rc_;              \
  } while (0)
  // per kind: K = the kind's RegKind, st = its stride, km = the neighbour list positions the kernel variant in use keeps (5, 8 or
  // 16 — launch_associate), rec = the fields of its association record
#define SCRATCH_K(id, bytes, field)                                                                        \
  for (int k = 0; k < 2; k++) {                                                                            \
    RegKind& K = B.kind[k];                                                                                \
    const size_t st = K.stride, km = C.kind[k].k <= 5 ? 5 : (C.kind[k].k <= 8 ? 8 : kMaxK), rec = k ? 7 : 9; \
    SCRATCH(ctx->wsk[id][k], bytes, K.field);                                                              \
  }
  SCRATCH_K(WSK_GRID_DESC, np * sizeof(GridDesc), grid.desc)
  SCRATCH_K(WSK_CELLS, (np * (size_t)(kGridCellsCap + 1) + 4) * sizeof(uint32_t), grid.cell_start)  // (+4: the search reads four entries at a time)
  SCRATCH_K(WSK_SORTED, np * (st + kGridPad) * sizeof(GridPoint), grid.sorted)
  SCRATCH_K(WSK_REL, np * 3 * (st + kGridPad) * sizeof(float), grid.rel)
  SCRATCH_K(WSK_SGRID_DESC, np * sizeof(GridDesc), src_grid.desc)
  SCRATCH_K(WSK_SCELLS, np * (size_t)(kGridCellsCap + 1) * sizeof(uint32_t), src_grid.cell_start)
  SCRATCH_K(WSK_SSORTED, np * st * sizeof(GridPoint), src_grid.sorted)
  SCRATCH(ctx->ws[WS_SORT_SCRATCH], np * (es > ps ? es : ps) * sizeof(GridPoint), B.sort_scratch);
  // (sets the packed build takes are ordered in LDS and need no scratch: the predicate is the launcher's own)
  SCRATCH(ctx->ws[WS_SORT_SCRATCH_SRC], grid_small(es > ps ? es : ps, C.flags) ? sizeof(GridPoint) : np * (es > ps ? es : ps) * sizeof(GridPoint), B.sort_scratch_src);
  SCRATCH_K(WSK_ASSOC, rec * np * st * sizeof(double), rec)
  SCRATCH_K(WSK_NN, (1 + km) * np * st * sizeof(uint32_t), nn)
  SCRATCH_K(WSK_RNN, (1 + km) * np * st * sizeof(uint32_t), rnn)
  SCRATCH_K(WSK_NEAREST, np * st * sizeof(uint32_t), nearest)
  SCRATCH_K(WSK_REST, np * st * sizeof(uint32_t), rest)
  SCRATCH_K(WSK_EXACT, np * st * sizeof(uint32_t), exact)
  SCRATCH(ctx->ws[WS_NASSOC], np * 8 * sizeof(uint32_t), B.n_assoc);
  SCRATCH(ctx->ws[WS_STATE], np * sizeof(PairState), B.state);
  SCRATCH(ctx->ws[WS_PARTIALS], np * B.blocks_per_pair * kAccSize * sizeof(double), B.partials);
  SCRATCH(ctx->ws[WS_MOM_PARTIALS], np * B.mom_blocks_per_pair * 4 * (size_t)(kMomSize + 2) * sizeof(double), B.mom_partials);
  SCRATCH(ctx->ws[WS_MOMENTS], np * (size_t)(kMomSize + 2) * sizeof(double), B.moments);
  SCRATCH(ctx->ws[WS_FLAGGED_LIST], np * (size_t)B.mom_blocks_per_pair * kSweepChunk * sizeof(uint32_t), B.flagged_list);
  SCRATCH(ctx->ws[WS_FLAGGED_COUNT], np * (size_t)B.mom_blocks_per_pair * 4 * sizeof(uint32_t), B.flagged_count);
  // the live lists (xcd_map.h) only where the deal exists: at least 8 pairs (below, xcd_pair_map spreads chunks, not pairs)
  if (np >= 8 && !(C.flags & kRegFlagNoLiveDeal)) {
    SCRATCH(ctx->ws[WS_LIVE], sizeof(LiveLists) + 2 * np * sizeof(uint32_t), B.live);
    B.live_pairs = reinterpret_cast<uint32_t*>(B.live + 1);
  }
  if (opts.want_info_partials) {
    InfoPartial* info_partials = nullptr;  // (bound nowhere in B: the callers hand reg_info_partials(ctx) to reg_information)
    SCRATCH(ctx->ws[WS_INFO_PARTIALS], np * info_blocks_per_pair(es, ps) * sizeof(InfoPartial), info_partials);
  }
#undef SCRATCH_K
#undef SCRATCH
  {
    const bool fresh = ctx->ws[WS_COUNTERS].cap == 0;
    ENSURE(ctx, WS_COUNTERS, 128);
    untimed(ctx);
    if (fresh) HIP_TRY(ctx, hipMemsetAsync(ctx->ws[WS_COUNTERS].p, 0, 128, ctx->stream));
  }
  if (opts.want_iter_info) ENSURE(ctx, WS_ITERINFO, np * (size_t)(C.max_iterations ? C.max_iterations : 1) * sizeof(loamx_iter_info));
  // counters: [0] n_active (u32), [8..48) sweep / association / moment slot counters (5 x u64), [48..56) index-build bytes
  B.n_active = wsp<uint32_t>(ctx, WS_COUNTERS);
  B.sweep_slots = reinterpret_cast<unsigned long long*>(wsp<unsigned char>(ctx, WS_COUNTERS) + 8);
  B.assoc_slots = B.sweep_slots + 2;
  B.grid_bytes = B.sweep_slots + 5;
  B.iter_info = opts.want_iter_info ? wsp<loamx_iter_info>(ctx, WS_ITERINFO) : nullptr;
  B.want_nearest = opts.want_nearest ? 1u : 0u;
  B.ref_moments = (C.flags & (kRegFlagNoMoments | kRegFlagNoRefMoments)) ? 0u : 1u;
  B.max_counts = wsp<uint32_t>(ctx, WS_COUNTERS) + 16;  // bytes 64..88
  B.small_edge_sets = (C.flags & kRegFlagNoSmallSets) ? 0u : (!prebuilt ? 1u : (prebuilt->n[0] <= kBruteMax ? 2u : 0u));
  hipStream_t s = ctx->stream;
  // The per-pair state first: its kernel also finds the largest source sets, which come back to the host while
  // the index builds run (an event right behind the copy: the builds are already queued when the host waits).
  untimed(ctx);
  if (!ctx->max_counts_clean) {  // (write_results_kernel leaves them ready for the next call: no copy kernel in front of state_init_kernel then)
    const uint32_t init[6] = {0u, 0u, 0u, 0u, 0xFFFFFFFFu, 0xFFFFFFFFu};
    memcpy(&ctx->h_pinned[8], init, sizeof(init));
    HIP_TRY(ctx, hipMemcpyAsync(B.max_counts, &ctx->h_pinned[8], sizeof(init), hipMemcpyHostToDevice, s));
  }
  ctx->max_counts_clean = false;
  launch_state_init(B, C, s);
  CHECK_LAUNCH(ctx, "state_init_kernel");
  if (!ctx->ev_counts) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_counts, hipEventDisableTiming));
  HIP_TRY(ctx, hipMemcpyAsync(&ctx->h_pinned[16], B.max_counts, 6 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipEventRecord(ctx->ev_counts, s));

  if (prebuilt) {  // persistent target index: only the source sets are (re)ordered
    for (int k = 0; k < 2; k++) B.kind[k].grid = index_grid_set(prebuilt, k);
  }
  {
    TimedScope t(ctx, LOAMX_K_GRID, 0.0);
    // the source builds next to the target builds on the auxiliary stream: every workgroup of one build kernel is in
    // the same phase at the same time (reads, then writes), two different kernels side by side even the HBM demand
    // out (measured 1.19 -> 1.11 ms per step). For a single pair too since round 3 (the two planar builds are one
    // workgroup of 45 and 83 us each: side by side 100 instead of 150 us; one pair 0.82 -> 0.80 ms).
    // (Round 3: the first ICF iteration's edge chains right behind the edge builds on the auxiliary stream, i.e. next to
    // the planar index builds instead of next to the plane k-NN kernel: 11.60 / 11.72 vs 11.65 / 11.53 ms per step —
    // what the k-NN kernel gains the HBM-bound builds lose. Not kept.)
    // (the fork waits on the event already recorded behind the counts' copy: one marker packet fewer in front of the builds)
    const bool side = !(C.flags & kRegFlagNoGridSide) && ctx->aux_stream && !prebuilt && hipStreamWaitEvent(ctx->aux_stream, ctx->ev_counts, 0) == hipSuccess;
    if (!prebuilt) launch_grid_build_targets(B, C, s);
    launch_grid_build_sources(B, C, side ? ctx->aux_stream : s);
    if (side && hipEventRecord(ctx->ev_join, ctx->aux_stream) == hipSuccess) (void)hipStreamWaitEvent(s, ctx->ev_join, 0);
  }
  CHECK_LAUNCH(ctx, "grid_build_kernel");
  HIP_TRY(ctx, hipEventSynchronize(ctx->ev_counts));
  // the counts read back: [16, 17] largest source edge / planar set, [18, 19] largest and [20, 21] smallest target set
  for (int k = 0; k < 2; k++) {
    B.kind[k].assoc_blocks = (ctx->h_pinned[16 + k] + 255u) / 256u;  // kAssocThreads queries per workgroup
    // which of the two k-NN kernels of a feature kind has work at all (target sizes relative to kBruteMax)
    const uint32_t tmax = prebuilt ? (uint32_t)prebuilt->n[k] : ctx->h_pinned[18 + k], tmin = prebuilt ? tmax : ctx->h_pinned[20 + k];
    B.kind[k].knn_mode = tmin > tmax ? 0u : (tmin > kBruteMax ? 1u : (tmax <= kBruteMax ? 2u : 0u));
  }
  return LOAMX_OK;
}

int reg_dump(loamx_ctx* ctx, const RegBatch& B, const RegConfig& C, const loamx_assoc_dump* dump, const size_t n_src[2]) {
  if (B.n_pairs == 0) return LOAMX_OK;
  hipStream_t s = ctx->stream;
  if (B.n_pairs != 1) return fail(ctx, LOAMX_ERR_BAD_PARAM, "association dump: one pair at a time");
  RegBatch Bd = B;
  Bd.want_nn_counts = 1u;  // (assoc_dump_kernel reads the verified counts out of nn: only here does fit_one write them back)
  // the association census (loamx_ctx_last_assoc_census): only here is launch_associate handed a census to fill
  AssocCensusRun census = {};
  for (int kind = 0; kind < 2; kind++) {
    const size_t st = B.kind[kind].stride, bytes = 8 * sizeof(uint32_t) + 2 * st * sizeof(int32_t);
    ENSURE(ctx, ctx->wsk[WSK_CENSUS][kind], bytes);
    HIP_TRY(ctx, hipMemsetAsync(ctx->wsk[WSK_CENSUS][kind].p, 0, bytes, s));
    census.buf[kind].counts = wskp<uint32_t>(ctx, WSK_CENSUS, kind);
    census.buf[kind].after_rest = reinterpret_cast<int32_t*>(census.buf[kind].counts + 8);
    census.buf[kind].before_fit = census.buf[kind].after_rest + st;
  }
  int rc_a = enqueue_association(ctx, Bd, C, kAssocEdges | kAssocPlanes, &census);
  if (rc_a != LOAMX_OK) return rc_a;
  untimed(ctx);
  const size_t n[2] = {n_src[kEdge], n_src[kPlane]}, kq[2] = {(size_t)C.kind[kEdge].k, (size_t)C.kind[kPlane].k}, pw[2] = {6, 4};
  AssocDumpSet D[2] = {};
  for (int kind = 0; kind < 2; kind++) {
    const size_t bytes = n[kind] * (24 + 8 * pw[kind] + 4 + 4 * kq[kind] + 1) + 64;
    ENSURE(ctx, ctx->wsk[WSK_DUMP][kind], bytes);
    unsigned char* base = wskp<unsigned char>(ctx, WSK_DUMP, kind);
    HIP_TRY(ctx, hipMemsetAsync(base, 0, bytes, s));  // (features beyond the capacity, if any, read as "no neighbours")
    D[kind].moved = reinterpret_cast<double*>(base);
    D[kind].prim = D[kind].moved + 3 * n[kind];
    D[kind].nn_count = reinterpret_cast<uint32_t*>(D[kind].prim + pw[kind] * n[kind]);
    D[kind].nn_idx = D[kind].nn_count + n[kind];
    D[kind].valid = reinterpret_cast<uint8_t*>(D[kind].nn_idx + kq[kind] * n[kind]);
    if (n[kind] == 0) D[kind].nn_count = nullptr;
  }
  launch_assoc_dump(B, C, D, s);
  CHECK_LAUNCH(ctx, "assoc_dump_kernel");
  struct Out { void* host; const void* dev; size_t bytes; };
  const Out outs[10] = {
      {dump->edge_nn_count, D[0].nn_count, 4 * n[0]}, {dump->edge_nn_idx, D[0].nn_idx, 4 * kq[0] * n[0]}, {dump->edge_valid, D[0].valid, n[0]},
      {dump->edge_moved, D[0].moved, 24 * n[0]}, {dump->edge_lines, D[0].prim, 48 * n[0]},
      {dump->plane_nn_count, D[1].nn_count, 4 * n[1]}, {dump->plane_nn_idx, D[1].nn_idx, 4 * kq[1] * n[1]}, {dump->plane_valid, D[1].valid, n[1]},
      {dump->plane_moved, D[1].moved, 24 * n[1]}, {dump->plane_planes, D[1].prim, 32 * n[1]}};
  for (const Out& o : outs)
    if (o.host && o.bytes && o.dev) HIP_TRY(ctx, hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, s));
  if (dump->queue_lengths) HIP_TRY(ctx, hipMemcpyAsync(dump->queue_lengths, B.n_assoc + 2, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  // the census, kept on the context as host copies: the workspace may be handed on by the next call
  uint32_t na[8];
  HIP_TRY(ctx, hipMemcpy(na, B.n_assoc, sizeof(na), hipMemcpyDeviceToHost));
  for (int kind = 0; kind < 2; kind++) {
    const RegKind& K = B.kind[kind];
    const AssocCensusForm& F = census.form[kind];
    loamx_ctx::AssocCensusKept& keep = ctx->last_assoc_census[kind];
    loamx_assoc_census& c = keep.c;
    c = loamx_assoc_census{};
    GridDesc g;
    uint32_t counts[8];
    HIP_TRY(ctx, hipMemcpy(&g, K.grid.desc, sizeof(g), hipMemcpyDeviceToHost));
    if (F.km == 0u) g = GridDesc{};  // (the kind was not launched: whatever the descriptor holds is an earlier call's)
    HIP_TRY(ctx, hipMemcpy(counts, census.buf[kind].counts, sizeof(counts), hipMemcpyDeviceToHost));
    c.n_src = (uint32_t)(n[kind] < K.stride ? n[kind] : K.stride), c.n_tgt = g.n_points, c.stride = K.stride;
    c.km = F.km, c.search = F.search, c.mixed_launch = F.mixed_launch, c.one_stage = F.one_stage, c.leftover_kernel = F.leftover_kernel;
    c.rest_blocks = F.rest_blocks, c.coop_blocks = F.coop_blocks;
    c.origin[0] = g.ox, c.origin[1] = g.oy, c.origin[2] = g.oz, c.h = g.h, c.nx = g.nx, c.ny = g.ny, c.nz = g.nz, c.n_points = g.n_points;
    c.verified = counts[0], c.unverified = counts[1], c.queued_words = counts[2];
    keep.coop_forms[0] = counts[5], keep.coop_forms[1] = counts[6];  // (no census field: the kernel's own count of its two forms)
    c.queued = na[2 + kind], c.listed = na[4 + kind], c.exact = counts[4], c.leftover_finished = counts[3] - counts[4], c.late = na[6 + kind];
    const uint32_t q = c.queued < K.stride ? c.queued : (uint32_t)K.stride;
    keep.entry.assign(q, 0u), keep.after_rest.assign(q, 0), keep.before_fit.assign(q, 0);
    if (q) {
      HIP_TRY(ctx, hipMemcpy(keep.entry.data(), K.rest, q * sizeof(uint32_t), hipMemcpyDeviceToHost));
      HIP_TRY(ctx, hipMemcpy(keep.after_rest.data(), census.buf[kind].after_rest, q * sizeof(int32_t), hipMemcpyDeviceToHost));
      HIP_TRY(ctx, hipMemcpy(keep.before_fit.data(), census.buf[kind].before_fit, q * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    uint32_t derived[4];  // (from the entries as the kernels read them: index in the source set's cell order | reason bits)
    assoc_census_derive(F, B.n_pairs, g, keep.entry.data(), q, na[4 + kind], derived);
    c.rest_spread = derived[0], c.left_spread = derived[1], c.lean_set = derived[2], c.rest_searched = derived[3];
    // the late list: the tail of K.exact, filled from its end (fit_one)
    const uint32_t nl = c.late < K.stride ? c.late : (uint32_t)K.stride;
    keep.late.assign(nl, 0u);
    if (nl) HIP_TRY(ctx, hipMemcpy(keep.late.data(), K.exact + (K.stride - nl), nl * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (q || nl) {  // kept by the CALLER's source index: the cell-sorted copy of the source set names it
      std::vector<GridPoint> sorted(c.n_src);
      HIP_TRY(ctx, hipMemcpy(sorted.data(), K.src_grid.sorted, (size_t)c.n_src * sizeof(GridPoint), hipMemcpyDeviceToHost));
      for (uint32_t t = 0; t < q; t++) {
        const uint32_t i = keep.entry[t] & 0x3FFFFFFFu;
        keep.entry[t] = (keep.entry[t] & ~0x3FFFFFFFu) | (i < c.n_src ? (sorted[i].orig & 0x3FFFFFFFu) : 0x3FFFFFFFu);
      }
      std::vector<uint32_t> tail(keep.late);
      for (uint32_t t = 0; t < nl; t++) {  // (entry t of the list sits at stride - 1 - t)
        const uint32_t i = tail[nl - 1 - t];
        keep.late[t] = i < c.n_src ? sorted[i].orig : 0xFFFFFFFFu;
      }
    }
    for (uint32_t t = 0; t < q; t++) {
      if (keep.entry[t] & LOAMX_ASSOC_REASON_WIDE) c.queued_wide++;
      else if (keep.entry[t] & LOAMX_ASSOC_REASON_TIED) c.queued_tied++;
      else c.queued_plain++;
    }
  }
  ctx->last_assoc_census_valid = true;
  return LOAMX_OK;
}

// One association pass at the pairs' current estimates, then the information kernels. Behind a registration every pair has
// stopped and the association kernels would leave at once: info_activate_kernel marks the pairs active for this one pass
// (nothing reads `active` afterwards: the next call starts from state_init_kernel; the queue lengths in n_assoc are zero,
// lm_begin_kernel cleared them when the pair's last iteration began).
int reg_information(loamx_ctx* ctx, const RegBatch& B, const RegConfig& C, InfoPartial* info_partials, loamx_reg_information* d_info, bool activate) {
  if (B.n_pairs == 0) return LOAMX_OK;
  hipStream_t s = ctx->stream;
  untimed(ctx);
  if (activate) launch_info_activate(B, s);
  const int rc_a = enqueue_association(ctx, B, C);
  if (rc_a != LOAMX_OK) return rc_a;
  {
    TimedScope t(ctx, LOAMX_K_INFORMATION, 0.0, true);
    launch_information(B, info_partials, d_info, s);
  }
  CHECK_LAUNCH(ctx, "information_kernel");
  return LOAMX_OK;
}

int reg_solve(loamx_ctx* ctx, const RegBatch& B, const RegConfig& C, loamx_reg_result* d_results, AfterAssocHook hook, void* hook_user) {
  if (B.n_pairs == 0) return LOAMX_OK;
  hipStream_t s = ctx->stream;
  ctx->last_solve_batch = B, ctx->last_solve_flags = C.flags, ctx->last_solve_valid = true;  // (loamx_ctx_last_solve_census)
  // (Replaying an ICF iteration as a hipGraph was measured in round 2 — captured once, cached, ~110 kernel nodes over
  // three streams: 13.6 vs 13.1 ms per 1 024-pair step and 1.06 vs 1.07 ms for one pair. The GPU-side turnaround of
  // dependent kernels bounds both, not the host's launch rate, and the graph loses the stream priorities; removed.)
  for (uint32_t it = 0; it < C.max_iterations; it++) {
    {
      const int rc_body = enqueue_icf_iteration(ctx, B, C, it, hook, hook_user);
      if (rc_body != LOAMX_OK) return rc_body;
    }
    if (it + 1 < C.max_iterations && it > (B.n_pairs >= 256 ? 1u : 0u)) {
      // one 4-byte readback per outer iteration: stop as soon as every pair has terminated. Not after the first
      // iteration: a registration that starts more than the convergence thresholds away from its answer cannot
      // converge there, so the second iteration is enqueued without waiting (if every pair did stop — too few
      // associations everywhere — its kernels find no active pair and return). A large batch does not wait after
      // the second iteration either: that hundreds of pairs all stop there is as good as excluded, and the
      // synchronisation idles the GPU for ~35 us (a single pair does wait: a third iteration would cost it 0.3 ms)
      // The results go out BEFORE the host waits: when this was the last iteration (the usual case where the host looks at
      // all) they are written while the read-back travels, instead of ~26 us of idle GPU later; otherwise they are written
      // again at the end.
      untimed(ctx);
      HIP_TRY(ctx, hipMemcpyAsync(ctx->h_pinned, B.live_count(it), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      launch_write_results(B, d_results, s);
      CHECK_LAUNCH(ctx, "write_results_kernel");
      HIP_TRY(ctx, hipStreamSynchronize(s));
      if (ctx->h_pinned[0] == 0) {
        ctx->max_counts_clean = true;
        return LOAMX_OK;
      }
    }
  }
  untimed(ctx);
  launch_write_results(B, d_results, s);
  CHECK_LAUNCH(ctx, "write_results_kernel");
  ctx->max_counts_clean = true;
  return LOAMX_OK;
}

}  // namespace loamx

namespace {
struct DetailHook {
  loamx_reg_detail* detail;
  size_t n_src[2];
};
int detail_hook(loamx_ctx* ctx, const RegBatch& B, uint32_t it, void* user) {
  DetailHook* h = static_cast<DetailHook*>(user);
  loamx_reg_detail* d = h->detail;
  if (!d) return LOAMX_OK;
  for (int kind = 0; kind < 2; kind++) {
    const size_t n = h->n_src[kind];
    uint32_t* base = kind ? d->plane_pairs : d->edge_pairs;
    const size_t cap = kind ? d->pairs_cap_plane : d->pairs_cap_edge;
    uint32_t* out_n = kind ? d->n_plane_pairs : d->n_edge_pairs;
    if (!base || !out_n) continue;
    out_n[it] = 0;
    if (cap == 0 || n == 0) continue;
    uint32_t* out = base + (size_t)it * 2 * cap;
    std::vector<uint32_t> nearest(n);
    HIP_TRY(ctx, hipMemcpyAsync(nearest.data(), B.kind[kind].nearest, n * sizeof(uint32_t),
                                hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    size_t m = 0;
    for (size_t i = 0; i < n; i++) {
      if (nearest[i] == 0xFFFFFFFFu) continue;
      if (m < cap) out[2 * m] = (uint32_t)i, out[2 * m + 1] = nearest[i];
      m++;
    }
    out_n[it] = (uint32_t)(m < cap ? m : cap);
  }
  return LOAMX_OK;
}
}  // namespace

extern "C" {

struct HostSets {  // one scan's feature sets in host memory, [edge, plane]
  const double* pts[2];
  size_t n[2];
};
// what a one-pair call is for, and where its outcome goes
struct HostOutput {
  enum Kind { kResult, kDump, kInfo } kind;
  loamx_reg_result* result;     // kResult: the registration ...
  loamx_reg_detail* detail;     // ... and (optional) its per-iteration detail
  const loamx_assoc_dump* dump;  // kDump: one association pass at init_pose, read out
  loamx_reg_information* info;  // kInfo: the information matrix at init_pose
  static HostOutput to_result(loamx_reg_result* r, loamx_reg_detail* d) { return {kResult, r, d, nullptr, nullptr}; }
  static HostOutput to_dump(const loamx_assoc_dump* d) { return {kDump, nullptr, nullptr, d, nullptr}; }
  static HostOutput to_info(loamx_reg_information* i) { return {kInfo, nullptr, nullptr, nullptr, i}; }
};
static int register_features_impl(loamx_ctx* ctx, const loamx_target_index* index, const HostSets& src, HostSets tgt, const double init_pose[7],
                                  const loamx_reg_params* reg, const HostOutput& out) {
  API_ENTER(ctx);
  loamx_reg_result* const result = out.result;
  loamx_reg_detail* const detail = out.detail;
  if ((out.kind == HostOutput::kResult && !result) || !init_pose) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  for (int k = 0; k < 2; k++)
    if ((src.n[k] && !src.pts[k]) || (!index && tgt.n[k] && !tgt.pts[k])) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  RegConfig C;
  int rc = make_reg_config(ctx, reg, C);
  if (rc != LOAMX_OK) return rc;
  if (index) {
    if (index->radius[kEdge] != C.kind[kEdge].r || index->radius[kPlane] != C.kind[kPlane].r)
      return fail(ctx, LOAMX_ERR_BAD_PARAM, "registration params do not match the ones the target index was built with");
    // (an insert that failed between growing a set and rebuilding its grid leaves n ahead of the grid)
    for (int k = 0; k < 2; k++)
      if (index->n[k] != 0 && !index->grid_valid[k])
        return fail(ctx, LOAMX_ERR_BAD_PARAM, "the target index is inconsistent (an insert into it failed): insert again or build a new one");
    tgt.n[kEdge] = tgt.n[kPlane] = 0;  // the target lives in the index
  }
  size_t stride[2];
  for (int k = 0; k < 2; k++) {
    stride[k] = src.n[k] > tgt.n[k] ? src.n[k] : tgt.n[k];
    if (stride[k] > 0x3FFFFFFFull) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "feature set too large");  // (queue entries: 30-bit query index + 2 flags)
  }
  if (!host_all_finite(init_pose, false, 7)) return fail(ctx, LOAMX_ERR_BAD_PARAM, kNonFiniteMsg);
  hipStream_t s = ctx->stream;
  for (int k = 0; k < 2; k++) {
    ENSURE(ctx, ctx->wsk[WSK_SRC][k], (stride[k] ? stride[k] : 1) * 3 * sizeof(double));
    ENSURE(ctx, ctx->wsk[WSK_TGT][k], (stride[k] ? stride[k] : 1) * 3 * sizeof(double));
  }
  ENSURE(ctx, WS_FCOUNTS, 4 * sizeof(uint32_t));
  ENSURE(ctx, WS_RESULTS, sizeof(loamx_reg_result));
  ENSURE(ctx, WS_INIT, 7 * sizeof(double));
  if (out.kind == HostOutput::kInfo) ENSURE(ctx, WS_INFO, sizeof(loamx_reg_information));
  for (int k = 0; k < 2; k++) {
    if (src.n[k]) HIP_TRY(ctx, hipMemcpyAsync(ctx->wsk[WSK_SRC][k].p, src.pts[k], src.n[k] * 24, hipMemcpyHostToDevice, s));
    if (tgt.n[k]) HIP_TRY(ctx, hipMemcpyAsync(ctx->wsk[WSK_TGT][k].p, tgt.pts[k], tgt.n[k] * 24, hipMemcpyHostToDevice, s));
  }
  const uint32_t counts[4] = {(uint32_t)src.n[kEdge], (uint32_t)src.n[kPlane], (uint32_t)tgt.n[kEdge], (uint32_t)tgt.n[kPlane]};
  {  // non-finite coordinates are refused before anything else is launched (loamx.h: "Non-finite input")
    rc = finite_begin(ctx);
    if (rc != LOAMX_OK) return rc;
    for (int k = 0; k < 2; k++)
      finite_add(ctx, ctx->wsk[WSK_SRC][k].p, false, nullptr, 1, src.n[k], 1), finite_add(ctx, ctx->wsk[WSK_TGT][k].p, false, nullptr, 1, tgt.n[k], 1);
    rc = finite_end(ctx);
    if (rc != LOAMX_OK) return rc;
  }
  HIP_TRY(ctx, hipMemcpyAsync(ctx->ws[WS_FCOUNTS].p, counts, sizeof(counts), hipMemcpyHostToDevice, s));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->ws[WS_INIT].p, init_pose, 7 * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));  // `counts` is a stack array
  RegInputs in{};
  in.n_pairs = 1, in.in_pitch = 1;
  const uint32_t* fc = wsp<uint32_t>(ctx, WS_FCOUNTS);
  for (int k = 0; k < 2; k++)
    in.kind[k] = RegInputs::Kind{stride[k], wskp<double>(ctx, WSK_SRC, k), wskp<double>(ctx, WSK_TGT, k), fc + k, fc + 2 + k};
  in.init = wsp<double>(ctx, WS_INIT);
  DetailHook hook{detail, {src.n[kEdge], src.n[kPlane]}};
  if (detail) detail->n_iter_info = 0;
  RegPrepareOpts opts{};
  opts.want_iter_info = detail && detail->iter_info, opts.want_nearest = detail != nullptr;
  opts.want_info_partials = out.kind == HostOutput::kInfo, opts.one_pass = out.kind != HostOutput::kResult;
  RegBatch B;
  rc = reg_prepare(ctx, in, C, index, opts, B);
  if (rc != LOAMX_OK) return rc;
  if (out.kind == HostOutput::kDump) return reg_dump(ctx, B, C, out.dump, src.n);
  if (out.kind == HostOutput::kInfo) {
    rc = reg_information(ctx, B, C, reg_info_partials(ctx), wsp<loamx_reg_information>(ctx, WS_INFO), false);
    if (rc != LOAMX_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out.info, ctx->ws[WS_INFO].p, sizeof(loamx_reg_information), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return LOAMX_OK;
  }
  rc = reg_solve(ctx, B, C, wsp<loamx_reg_result>(ctx, WS_RESULTS), detail ? detail_hook : nullptr, &hook);
  if (rc != LOAMX_OK) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(result, ctx->ws[WS_RESULTS].p, sizeof(loamx_reg_result), hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  if (detail && detail->iter_info && result->iterations) {
    HIP_TRY(ctx, hipMemcpy(detail->iter_info, ctx->ws[WS_ITERINFO].p, result->iterations * sizeof(loamx_iter_info),
                           hipMemcpyDeviceToHost));
    detail->n_iter_info = result->iterations;
  }
  return LOAMX_OK;
}

int loamx_register_features(loamx_ctx* ctx, const double* src_edge, size_t n_se, const double* src_planar, size_t n_sp,
                            const double* tgt_edge, size_t n_te, const double* tgt_planar, size_t n_tp,
                            const double init_pose[7], const loamx_reg_params* reg, loamx_reg_result* result,
                            loamx_reg_detail* detail) {
  return register_features_impl(ctx, nullptr, {{src_edge, src_planar}, {n_se, n_sp}}, {{tgt_edge, tgt_planar}, {n_te, n_tp}}, init_pose,
                                reg, HostOutput::to_result(result, detail));
}

int loamx_register_features_indexed(loamx_ctx* ctx, const loamx_target_index* index, const double* src_edge, size_t n_se,
                                    const double* src_planar, size_t n_sp, const double init_pose[7],
                                    const loamx_reg_params* reg, loamx_reg_result* result, loamx_reg_detail* detail) {
  if (!index) return LOAMX_ERR_BAD_PARAM;
  return register_features_impl(ctx, index, {{src_edge, src_planar}, {n_se, n_sp}}, {{nullptr, nullptr}, {0, 0}}, init_pose, reg,
                                HostOutput::to_result(result, detail));
}

/* ---- registration information matrix, one pair from host memory ---------------------------------------------- */
int loamx_registration_information(loamx_ctx* ctx, const double* src_edge, size_t n_se, const double* src_planar, size_t n_sp,
                                   const double* tgt_edge, size_t n_te, const double* tgt_planar, size_t n_tp, const double pose[7],
                                   const loamx_reg_params* reg, loamx_reg_information* info) {
  if (!info) return LOAMX_ERR_BAD_PARAM;
  return register_features_impl(ctx, nullptr, {{src_edge, src_planar}, {n_se, n_sp}}, {{tgt_edge, tgt_planar}, {n_te, n_tp}}, pose, reg,
                                HostOutput::to_info(info));
}

int loamx_registration_information_indexed(loamx_ctx* ctx, const loamx_target_index* index, const double* src_edge, size_t n_se,
                                           const double* src_planar, size_t n_sp, const double pose[7], const loamx_reg_params* reg,
                                           loamx_reg_information* info) {
  if (!index || !info) return LOAMX_ERR_BAD_PARAM;
  return register_features_impl(ctx, index, {{src_edge, src_planar}, {n_se, n_sp}}, {{nullptr, nullptr}, {0, 0}}, pose, reg,
                                HostOutput::to_info(info));
}

/* ---- solve readout (debug / tests): copies of what the last reg_solve left in the workspace, no kernel involved ---- */
int loamx_ctx_last_solve_census(loamx_ctx* ctx, size_t pair, loamx_solve_census* out) {
  if (!out) return LOAMX_ERR_BAD_PARAM;
  API_ENTER(ctx);
  if (!ctx->last_solve_valid) return fail(ctx, LOAMX_ERR_BAD_PARAM, "no registration on this context to read (or its workspace has been handed on since)");
  const RegBatch& B = ctx->last_solve_batch;
  if (pair >= B.n_pairs) return fail(ctx, LOAMX_ERR_BAD_PARAM, "pair out of range");
  hipStream_t s = ctx->stream;
  untimed(ctx);
  HIP_TRY(ctx, hipStreamSynchronize(s));
  PairState S;
  uint32_t n_raw[2] = {0, 0};
  HIP_TRY(ctx, hipMemcpy(&S, B.state + pair, sizeof(S), hipMemcpyDeviceToHost));
  for (int k = 0; k < 2; k++) HIP_TRY(ctx, hipMemcpy(&n_raw[k], B.kind[k].n_src + pair * B.in_pitch, sizeof(uint32_t), hipMemcpyDeviceToHost));
  uint32_t* const counts_out = out->tile_counts;
  const size_t cap = counts_out ? out->tile_counts_cap : 0;
  *out = loamx_solve_census{};
  out->tile_counts = counts_out, out->tile_counts_cap = cap;
  out->iterations = S.iterations, out->termination = S.termination, out->use_moments = S.use_moments, out->mom_ref_on = S.mom_ref_on;
  for (int i = 0; i < 7; i++) out->mom_ref[i] = S.mom_ref[i];
  out->tiles = B.mom_blocks_per_pair * 4;
  out->edge_stride = B.kind[kEdge].stride, out->planar_stride = B.kind[kPlane].stride;
  out->n_se = n_raw[kEdge] < B.kind[kEdge].stride ? n_raw[kEdge] : (uint32_t)B.kind[kEdge].stride;  // (as the kernels clamp them)
  out->n_sp = n_raw[kPlane] < B.kind[kPlane].stride ? n_raw[kPlane] : (uint32_t)B.kind[kPlane].stride;
  out->sweep_chunk = (uint32_t)kSweepChunk, out->edge_cache = kEdgeCache, out->list_cache = kListCache, out->flat_cache = kFlatCache;
  uint32_t live = 0;
  while (live < out->tiles && (size_t)(live / 4) * kSweepChunk < out->n_sp) live++;
  out->live_tiles = live;
  // Did moment_kernel and lm_pair_loop_kernel run in the pair's last completed iteration? In every iteration but the first
  // unless NO_MOMENTS; in the first one when the moments were taken at its first candidate. Otherwise nobody wrote the tile
  // counts and the maxima (or an earlier call did): they are not looked at.
  const bool lists = !(ctx->last_solve_flags & kRegFlagNoMoments) && (S.iterations >= 2u || S.mom_ref_on != 0u);
  if (!lists) return LOAMX_OK;  // walk = LOAMX_WALK_NONE
  double maxima[2];
  HIP_TRY(ctx, hipMemcpy(maxima, B.moments + pair * (size_t)(kMomSize + 2) + kMomSize, sizeof(maxima), hipMemcpyDeviceToHost));
  out->s0max = maxima[0], out->v2max = maxima[1];
  std::vector<uint32_t> cnt(live);
  if (live) HIP_TRY(ctx, hipMemcpy(cnt.data(), B.flagged_count + pair * (size_t)out->tiles, live * sizeof(uint32_t), hipMemcpyDeviceToHost));
  for (uint32_t t = 0; t < live; t++) {
    out->listed_total += cnt[t];
    if (t < cap) counts_out[t] = cnt[t];
  }
  // lm_pair_loop_kernel: the flat list needs the tile counts in LDS (tiles <= kListCache) and room for the records
  out->walk = out->tiles > kListCache ? LOAMX_WALK_TILED_BY_TILES : (out->listed_total > kFlatCache ? LOAMX_WALK_TILED_BY_COUNT : LOAMX_WALK_FLAT);
  return LOAMX_OK;
}

/* ---- association readout (debug / tests): the census the last loamx_associate left on the context, no device access ---- */
int loamx_ctx_last_assoc_census(loamx_ctx* ctx, int which_kind, loamx_assoc_census* out) {
  if (!out) return LOAMX_ERR_BAD_PARAM;
  API_LOCK(ctx);
  if (which_kind != 0 && which_kind != 1) return fail(ctx, LOAMX_ERR_BAD_PARAM, "which_kind: 0 = edges, 1 = planes");
  if (!ctx->last_assoc_census_valid) return fail(ctx, LOAMX_ERR_BAD_PARAM, "no association dump on this context to read (or another call came after it)");
  const loamx_ctx::AssocCensusKept& keep = ctx->last_assoc_census[which_kind];
  uint32_t *const eq = out->entry_query, *const er = out->entry_reason;
  int32_t *const ar = out->count_after_rest, *const bf = out->count_before_fit;
  const size_t cap = out->entries_cap, lcap = out->late_cap;
  uint32_t* const lq = out->late_query;
  *out = keep.c;
  out->late_query = lq, out->late_cap = lcap;
  for (size_t t = 0; lq && t < keep.late.size() && t < lcap; t++) lq[t] = keep.late[t];
  out->entry_query = eq, out->entry_reason = er, out->count_after_rest = ar, out->count_before_fit = bf, out->entries_cap = cap;
  for (size_t t = 0; t < keep.entry.size() && t < cap; t++) {
    if (eq) eq[t] = keep.entry[t] & 0x3FFFFFFFu;
    if (er) er[t] = keep.entry[t] & (LOAMX_ASSOC_REASON_WIDE | LOAMX_ASSOC_REASON_TIED);
    if (ar) ar[t] = keep.after_rest[t];
    if (bf) bf[t] = keep.before_fit[t];
  }
  return LOAMX_OK;
}

int loamx_ctx_last_assoc_coop_forms(loamx_ctx* ctx, int which_kind, uint32_t out[2]) {
  if (!out) return LOAMX_ERR_BAD_PARAM;
  API_LOCK(ctx);
  if (which_kind != 0 && which_kind != 1) return fail(ctx, LOAMX_ERR_BAD_PARAM, "which_kind: 0 = edges, 1 = planes");
  if (!ctx->last_assoc_census_valid) return fail(ctx, LOAMX_ERR_BAD_PARAM, "no association dump on this context to read (or another call came after it)");
  out[0] = ctx->last_assoc_census[which_kind].coop_forms[0], out[1] = ctx->last_assoc_census[which_kind].coop_forms[1];
  return LOAMX_OK;
}

/* ---- rows a16-a19 one by one ------------------------------------------------------------------------------ */
int loamx_associate(loamx_ctx* ctx, const double* src_edge, size_t n_se, const double* src_planar, size_t n_sp, const double* tgt_edge,
                    size_t n_te, const double* tgt_planar, size_t n_tp, const double pose[7], const loamx_reg_params* reg,
                    loamx_assoc_dump* out) {
  if (!out) return LOAMX_ERR_BAD_PARAM;
  return register_features_impl(ctx, nullptr, {{src_edge, src_planar}, {n_se, n_sp}}, {{tgt_edge, tgt_planar}, {n_te, n_tp}}, pose, reg,
                                HostOutput::to_dump(out));
}

static int fit_sets(loamx_ctx* ctx, bool plane, const double* points, size_t n_sets, size_t k, double* prim_out, double* aux_out) {
  API_ENTER(ctx);
  if (n_sets == 0) return LOAMX_OK;
  if (!points || !prim_out) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  if (k < (plane ? 3u : 2u)) return fail(ctx, LOAMX_ERR_BAD_PARAM, plane ? "fitPlane needs k >= 3 points" : "fitLine needs k >= 2 points");
  if (k > (size_t)kFitMaxK) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "point sets of more than 32 points are not supported by the fit kernels");
  if (n_sets > 0x7FFFFFFFull / 64) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "too many point sets in one call");
  const size_t pw = plane ? 4 : 6;
  untimed(ctx);
  ENSURE(ctx, WS_FIT_IN, n_sets * k * 24);
  ENSURE(ctx, WS_FIT_OUT, n_sets * (pw + 1) * sizeof(double));
  double* d_prim = wsp<double>(ctx, WS_FIT_OUT);
  double* d_aux = d_prim + n_sets * pw;
  hipStream_t s = ctx->stream;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->ws[WS_FIT_IN].p, points, n_sets * k * 24, hipMemcpyHostToDevice, s));
  {
    int rc = dev_check_finite(ctx, ctx->ws[WS_FIT_IN].p, false, nullptr, 1, n_sets * k, 1, true);
    if (rc != LOAMX_OK) return rc;
  }
  launch_fit_sets(plane, wsp<double>(ctx, WS_FIT_IN), n_sets, (int)k, d_prim, d_aux, s);
  CHECK_LAUNCH(ctx, "fit_sets_kernel");
  HIP_TRY(ctx, hipMemcpyAsync(prim_out, d_prim, n_sets * pw * sizeof(double), hipMemcpyDeviceToHost, s));
  if (aux_out) HIP_TRY(ctx, hipMemcpyAsync(aux_out, d_aux, n_sets * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  return LOAMX_OK;
}

int loamx_fit_lines(loamx_ctx* ctx, const double* points, size_t n_sets, size_t k, double* lines_out, double* cond_out) {
  return fit_sets(ctx, false, points, n_sets, k, lines_out, cond_out);
}
int loamx_fit_planes(loamx_ctx* ctx, const double* points, size_t n_sets, size_t k, double* planes_out, double* avg_dist_out) {
  return fit_sets(ctx, true, points, n_sets, k, planes_out, avg_dist_out);
}

int loamx_knn_search(loamx_ctx* ctx, const loamx_target_index* index, int which_set, const double* queries, size_t n_queries, size_t k,
                     double max_dist, uint32_t* indices_out, uint32_t* counts_out) {
  if (!ctx || !index) return LOAMX_ERR_BAD_PARAM;
  API_ENTER(ctx);
  if (which_set != 0 && which_set != 1) return fail(ctx, LOAMX_ERR_BAD_PARAM, "which_set: 0 = edge points, 1 = planar points");
  if (index->n[which_set] != 0 && !index->grid_valid[which_set])
    return fail(ctx, LOAMX_ERR_BAD_PARAM, "the target index is inconsistent (an insert into it failed): insert again or build a new one");
  if (n_queries == 0) return LOAMX_OK;
  if (!queries || !indices_out || !counts_out) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  if (k == 0) {
    memset(counts_out, 0, n_queries * sizeof(uint32_t));
    return LOAMX_OK;
  }
  if (k > (size_t)kMaxK) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "k > 16 neighbours not supported by the search kernels");
  if (n_queries > 0x7FFFFFFFull / 64) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "too many queries in one call");
  untimed(ctx);
  ENSURE(ctx, WS_FIT_IN, n_queries * 24);
  ENSURE(ctx, WS_FIT_OUT, n_queries * (k + 1) * sizeof(uint32_t));
  uint32_t* d_idx = wsp<uint32_t>(ctx, WS_FIT_OUT);
  uint32_t* d_cnt = d_idx + n_queries * k;
  hipStream_t s = ctx->stream;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->ws[WS_FIT_IN].p, queries, n_queries * 24, hipMemcpyHostToDevice, s));
  {
    int rc = dev_check_finite(ctx, ctx->ws[WS_FIT_IN].p, false, nullptr, 1, n_queries, 1, true);
    if (rc != LOAMX_OK) return rc;
  }
  launch_knn_queries(index_grid_set(index, which_set), wsp<double>(ctx, WS_FIT_IN), n_queries, (int)k, max_dist, d_idx, d_cnt, s);
  CHECK_LAUNCH(ctx, "knn_queries_kernel");
  HIP_TRY(ctx, hipMemcpyAsync(indices_out, d_idx, n_queries * k * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipMemcpyAsync(counts_out, d_cnt, n_queries * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  return LOAMX_OK;
}

/* ---- device-resident batch entry points ----------------------------------------------------------- */
// (d_info != nullptr: loamx_registration_information_batch_dev — d_init holds the poses, d_results is not used)
static int register_features_batch(loamx_ctx* ctx, size_t n_pairs, const double* d_src_edge, const uint32_t* d_n_src_edge,
                                   const double* d_src_planar, const uint32_t* d_n_src_planar, const double* d_tgt_edge,
                                   const uint32_t* d_n_tgt_edge, const double* d_tgt_planar, const uint32_t* d_n_tgt_planar,
                                   size_t edge_stride, size_t planar_stride, const double* d_init, const loamx_reg_params* reg,
                                   loamx_reg_result* d_results, loamx_reg_information* d_info) {
  API_ENTER(ctx);
  RegConfig C;
  int rc = make_reg_config(ctx, reg, C);
  if (rc != LOAMX_OK) return rc;
  RegInputs in{};
  in.n_pairs = n_pairs, in.in_pitch = 1, in.init = d_init;
  in.kind[kEdge] = RegInputs::Kind{edge_stride, d_src_edge, d_tgt_edge, d_n_src_edge, d_n_tgt_edge};
  in.kind[kPlane] = RegInputs::Kind{planar_stride, d_src_planar, d_tgt_planar, d_n_src_planar, d_n_tgt_planar};
  if (ctx->reg_flags & kRegFlagCheckFinite) {
    for (int role = 0; role < 2; role++)  // the source sets, then the target sets
      for (const RegInputs::Kind& K : in.kind) {
        rc = dev_check_finite(ctx, role ? K.tgt : K.src, false, role ? K.n_tgt : K.n_src, n_pairs, K.stride, 1);
        if (rc != LOAMX_OK) return rc;
      }
    if (d_init && n_pairs) {
      rc = check_finite_scalars(ctx, d_init, n_pairs * 7);
      if (rc != LOAMX_OK) return rc;
    }
  }
  RegPrepareOpts opts{};
  opts.want_info_partials = opts.one_pass = d_info != nullptr;
  RegBatch B;
  rc = reg_prepare(ctx, in, C, nullptr, opts, B);
  if (rc != LOAMX_OK) return rc;
  if (d_info) return reg_information(ctx, B, C, reg_info_partials(ctx), d_info, false);
  return reg_solve(ctx, B, C, d_results, nullptr, nullptr);
}

int loamx_register_features_batch_dev(loamx_ctx* ctx, size_t n_pairs, const double* d_src_edge,
                                      const uint32_t* d_n_src_edge, const double* d_src_planar,
                                      const uint32_t* d_n_src_planar, const double* d_tgt_edge,
                                      const uint32_t* d_n_tgt_edge, const double* d_tgt_planar,
                                      const uint32_t* d_n_tgt_planar, size_t edge_stride, size_t planar_stride,
                                      const double* d_init, const loamx_reg_params* reg, loamx_reg_result* d_results) {
  return register_features_batch(ctx, n_pairs, d_src_edge, d_n_src_edge, d_src_planar, d_n_src_planar, d_tgt_edge, d_n_tgt_edge, d_tgt_planar,
                                 d_n_tgt_planar, edge_stride, planar_stride, d_init, reg, d_results, nullptr);
}

int loamx_registration_information_batch_dev(loamx_ctx* ctx, size_t n_pairs, const double* d_src_edge,
                                             const uint32_t* d_n_src_edge, const double* d_src_planar,
                                             const uint32_t* d_n_src_planar, const double* d_tgt_edge,
                                             const uint32_t* d_n_tgt_edge, const double* d_tgt_planar,
                                             const uint32_t* d_n_tgt_planar, size_t edge_stride, size_t planar_stride,
                                             const double* d_pose, const loamx_reg_params* reg, loamx_reg_information* d_info) {
  if (!ctx) return LOAMX_ERR_BAD_PARAM;
  if (n_pairs != 0 && (!d_info || !d_n_src_edge || !d_n_src_planar || !d_n_tgt_edge || !d_n_tgt_planar || !d_src_edge || !d_src_planar ||
                       !d_tgt_edge || !d_tgt_planar)) {
    ApiLock lock(ctx);
    return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  }
  return register_features_batch(ctx, n_pairs, d_src_edge, d_n_src_edge, d_src_planar, d_n_src_planar, d_tgt_edge, d_n_tgt_edge, d_tgt_planar,
                                 d_n_tgt_planar, edge_stride, planar_stride, d_pose, reg, nullptr, d_info);
}

}  // extern "C"
