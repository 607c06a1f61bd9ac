// api_place.hip — place recognition (loamx.h, "place recognition"): the database handle with its host-computed sector table and
// its device-resident entries, the descriptor, add and search entry points and their host forms.
#include "api_host.h"

struct loamx_place_db {
  int device = 0;
  loamx::PlaceShape shape = {};
  std::vector<double> dirs;  // the uploaded bytes (loamx_place_db_sector_dirs)
  double* d_dirs = nullptr;
  uint16_t* d_desc = nullptr;             // [cap][R S]
  uint32_t* d_keys = nullptr;             // [cap][R]
  unsigned long long* d_norms = nullptr;  // [cap][S]
  size_t n = 0, cap = 0;
};

using namespace loamx;

namespace {

constexpr size_t kPlaceFirstCap = 256;                  // entries of a database's first allocation; it doubles from there
constexpr size_t kPlaceCandBytes = (size_t)64 << 20;    // per candidate buffer: the queries of a search go in groups that fit
constexpr size_t kPlaceMaxQueryGroup = 65535;           // (blockIdx.y)

void db_free(loamx_place_db* db) {
  if (db->d_dirs) (void)hipFree(db->d_dirs);
  if (db->d_desc) (void)hipFree(db->d_desc);
  if (db->d_keys) (void)hipFree(db->d_keys);
  if (db->d_norms) (void)hipFree(db->d_norms);
  delete db;
}

PlaceEntries db_entries(const loamx_place_db* db) { return PlaceEntries{db->d_desc, db->d_keys, db->d_norms, (uint32_t)db->n}; }

int db_check(loamx_ctx* ctx, const loamx_place_db* db) {
  if (!db) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null place database");
  if (db->device != ctx->device) return fail(ctx, LOAMX_ERR_BAD_PARAM, "the place database was created on another device");
  return LOAMX_OK;
}

// room for `want` entries: new arrays, the old entries copied on the stream, one synchronisation, the old arrays freed
int db_grow(loamx_ctx* ctx, loamx_place_db* db, size_t want) {
  if (want <= db->cap) return LOAMX_OK;
  size_t cap = db->cap ? db->cap * 2 : kPlaceFirstCap;
  if (cap < want) cap = want;
  if (cap > kPlaceMaxEntries) cap = kPlaceMaxEntries;
  const size_t RS = (size_t)db->shape.R * db->shape.S;
  uint16_t* desc = nullptr;
  uint32_t* keys = nullptr;
  unsigned long long* norms = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&desc), cap * RS * sizeof(uint16_t));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&keys), cap * db->shape.R * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&norms), cap * db->shape.S * sizeof(unsigned long long));
  if (e == hipSuccess && db->n) {
    e = hipMemcpyAsync(desc, db->d_desc, db->n * RS * sizeof(uint16_t), hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(keys, db->d_keys, db->n * db->shape.R * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(norms, db->d_norms, db->n * db->shape.S * sizeof(unsigned long long), hipMemcpyDeviceToDevice, ctx->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // (the copies, and kernels still reading the old arrays)
  if (e != hipSuccess) {
    if (desc) (void)hipFree(desc);
    if (keys) (void)hipFree(keys);
    if (norms) (void)hipFree(norms);
    return fail(ctx, LOAMX_ERR_HIP, std::string("place database growth: ") + hipGetErrorString(e));
  }
  if (db->d_desc) (void)hipFree(db->d_desc);
  if (db->d_keys) (void)hipFree(db->d_keys);
  if (db->d_norms) (void)hipFree(db->d_norms);
  db->d_desc = desc, db->d_keys = keys, db->d_norms = norms, db->cap = cap;
  return LOAMX_OK;
}

// the argument checks the device and the host descriptor forms share
int descriptors_check(loamx_ctx* ctx, const loamx_place_db* db, const void* points, size_t stride, const size_t* offsets, size_t n_clouds,
                      const void* desc) {
  int rc = db_check(ctx, db);
  if (rc != LOAMX_OK) return rc;
  if (stride < 3) return fail(ctx, LOAMX_ERR_BAD_PARAM, "point_stride must be >= 3");
  if (stride > 0xFFFFFFFFull) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "point_stride does not fit 32 bits");
  if (n_clouds == 0) return LOAMX_OK;
  if (!offsets || !desc) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  for (size_t c = 0; c < n_clouds; c++) {
    if (offsets[c + 1] < offsets[c]) return fail(ctx, LOAMX_ERR_BAD_PARAM, "cloud_offsets must ascend");
    if (offsets[c + 1] - offsets[c] > 0xFFFFFFFEull) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "a cloud of more than 2^32 - 2 points");
  }
  if (offsets[n_clouds] > offsets[0] && !points) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null points");
  return LOAMX_OK;
}

// the clouds of the call chunk by chunk (the caller holds ctx->mu, has selected the device and checked the arguments)
int descriptors_locked(loamx_ctx* ctx, const loamx_place_db* db, const void* d_points, bool f32, size_t stride, const size_t* offsets,
                       size_t n_clouds, uint16_t* d_desc) {
  const size_t RS = (size_t)db->shape.R * db->shape.S;
  const size_t most_clouds = n_clouds < kOrgChunkClouds ? n_clouds : kOrgChunkClouds;
  ENSURE(ctx, WS_PLACE_TABLE, most_clouds * RS * sizeof(uint32_t));
  untimed(ctx);
  for (CloudChunks ch(offsets, n_clouds); ch.next();) {
    HIP_TRY(ctx, hipMemsetAsync(ctx->ws[WS_PLACE_TABLE].p, 0, ch.nc * RS * sizeof(uint32_t), ctx->stream));
    launch_place_descriptors(d_points, f32, (uint32_t)stride, ch.offs, ch.nc, ch.largest, db->shape, db->d_dirs, wsp<uint32_t>(ctx, WS_PLACE_TABLE),
                             d_desc + ch.c0 * RS, ctx->stream);
    CHECK_LAUNCH(ctx, "place descriptor kernels");
  }
  return LOAMX_OK;
}

int descriptors_dev(loamx_ctx* ctx, const loamx_place_db* db, const void* d_points, bool f32, size_t stride, const size_t* offsets, size_t n_clouds,
                    uint16_t* d_desc) {
  API_ENTER(ctx);
  int rc = descriptors_check(ctx, db, d_points, stride, offsets, n_clouds, d_desc);
  if (rc != LOAMX_OK || n_clouds == 0) return rc;
  return descriptors_locked(ctx, db, d_points, f32, stride, offsets, n_clouds, d_desc);
}

int descriptor_host(loamx_ctx* ctx, const loamx_place_db* db, const void* points, bool f32, size_t stride, size_t n, uint16_t* desc) {
  API_ENTER(ctx);
  const size_t offsets[2] = {0, n};
  int rc = descriptors_check(ctx, db, points, stride, offsets, 1, desc);
  if (rc != LOAMX_OK) return rc;
  const size_t RS = (size_t)db->shape.R * db->shape.S, in_bytes = n * stride * (f32 ? sizeof(float) : sizeof(double));
  untimed(ctx);
  ENSURE(ctx, WS_PLACE_IN, in_bytes);
  ENSURE(ctx, WS_PLACE_OUT, RS * sizeof(uint16_t));
  if (n) HIP_TRY(ctx, hipMemcpyAsync(ctx->ws[WS_PLACE_IN].p, points, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  rc = descriptors_locked(ctx, db, ctx->ws[WS_PLACE_IN].p, f32, stride, offsets, 1, wsp<uint16_t>(ctx, WS_PLACE_OUT));
  if (rc != LOAMX_OK) {
    (void)hipStreamSynchronize(ctx->stream);  // (the upload must not outlive the caller's array)
    return rc;
  }
  HIP_TRY(ctx, hipMemcpyAsync(desc, ctx->ws[WS_PLACE_OUT].p, RS * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LOAMX_OK;
}

int search_check(loamx_ctx* ctx, const loamx_place_db* db, const void* query, size_t n_queries, uint32_t K, const void* out) {
  int rc = db_check(ctx, db);
  if (rc != LOAMX_OK) return rc;
  if (K < 1 || K > kPlaceMaxCandidates) return fail(ctx, LOAMX_ERR_BAD_PARAM, "num_candidates must be 1 .. 64");
  if (n_queries && (!query || !out)) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  return LOAMX_OK;
}

// the queries group by group: keys and norms of the group, key stage, shift stage (the caller holds ctx->mu and has checked)
int search_locked(loamx_ctx* ctx, const loamx_place_db* db, const uint16_t* d_query, size_t n_queries, const uint32_t* id_end, uint32_t K,
                  loamx_place_match* d_out) {
  const PlaceShape& P = db->shape;
  const PlaceEntries E = db_entries(db);
  const size_t RS = (size_t)P.R * P.S, per_query = place_select_records(E.n, K) * sizeof(PlaceCand);
  size_t group = kPlaceCandBytes / per_query;
  group = group < 1 ? 1 : group > kPlaceMaxQueryGroup ? kPlaceMaxQueryGroup : group;
  if (id_end && group > kPlaceIdEndQueries) group = kPlaceIdEndQueries;
  group = group > n_queries ? n_queries : group;
  ENSURE(ctx, WS_PLACE_QKEYS, group * P.R * sizeof(uint32_t));
  ENSURE(ctx, WS_PLACE_QNORMS, group * P.S * sizeof(unsigned long long));
  ENSURE(ctx, WS_PLACE_CAND_A, group * per_query);
  ENSURE(ctx, WS_PLACE_CAND_B, group * per_query);
  ENSURE(ctx, WS_PLACE_MATCH, group * K * sizeof(loamx_place_match));
  untimed(ctx);
  for (size_t q0 = 0; q0 < n_queries; q0 += group) {
    const uint32_t nq = (uint32_t)(n_queries - q0 < group ? n_queries - q0 : group);
    launch_place_keys(d_query + q0 * RS, nq, P, wsp<uint32_t>(ctx, WS_PLACE_QKEYS), wsp<unsigned long long>(ctx, WS_PLACE_QNORMS), ctx->stream);
    const PlaceCand* cands = launch_place_key_stage(E, P, wsp<uint32_t>(ctx, WS_PLACE_QKEYS), id_end ? id_end + q0 : nullptr,
                                                    nq, K, wsp<PlaceCand>(ctx, WS_PLACE_CAND_A), wsp<PlaceCand>(ctx, WS_PLACE_CAND_B), ctx->stream);
    launch_place_shift_stage(E, P, d_query + q0 * RS, wsp<unsigned long long>(ctx, WS_PLACE_QNORMS), cands, nq, K,
                             wsp<loamx_place_match>(ctx, WS_PLACE_MATCH), d_out + q0 * K, ctx->stream);
    CHECK_LAUNCH(ctx, "place search kernels");
  }
  return LOAMX_OK;
}

}  // namespace

extern "C" {

void loamx_default_place_params(loamx_place_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->n_rings = 20, p->n_sectors = 60, p->max_range = 80.0, p->z_offset = 2.0, p->z_scale = 64.0;
}

int loamx_place_db_create(loamx_ctx* ctx, const loamx_place_params* params, loamx_place_db** out) {
  API_ENTER(ctx);
  if (!params || !out) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null argument");
  *out = nullptr;
  if (params->n_rings == 0 || params->n_sectors == 0) return fail(ctx, LOAMX_ERR_BAD_PARAM, "n_rings and n_sectors must be >= 1");
  if (!isfinite(params->max_range) || !(params->max_range > 0.0)) return fail(ctx, LOAMX_ERR_BAD_PARAM, "max_range must be finite and positive");
  if (!isfinite(params->z_scale) || !(params->z_scale > 0.0)) return fail(ctx, LOAMX_ERR_BAD_PARAM, "z_scale must be finite and positive");
  if (!isfinite(params->z_offset)) return fail(ctx, LOAMX_ERR_BAD_PARAM, "z_offset is not finite");
  if (params->n_rings > kPlaceMaxRings) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "n_rings > 64 not supported");
  if (params->n_sectors < kPlaceMinSectors || params->n_sectors > kPlaceMaxSectors)
    return fail(ctx, LOAMX_ERR_UNSUPPORTED, "n_sectors outside 3 .. 360 not supported");
  loamx_place_db* db = new loamx_place_db;
  db->device = ctx->device;
  db->shape.R = params->n_rings, db->shape.S = params->n_sectors;
  db->shape.ring_scale = (double)params->n_rings / params->max_range;
  db->shape.z_offset = params->z_offset, db->shape.z_scale = params->z_scale;
  db->dirs.resize(2 * (size_t)params->n_sectors);
  organize_column_dirs(0.0, false, params->n_sectors, db->dirs.data());
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&db->d_dirs), db->dirs.size() * sizeof(double));
  if (e == hipSuccess) e = hipMemcpy(db->d_dirs, db->dirs.data(), db->dirs.size() * sizeof(double), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    db_free(db);
    return fail(ctx, LOAMX_ERR_HIP, std::string("place database sector table: ") + hipGetErrorString(e));
  }
  *out = db;
  return LOAMX_OK;
}

void loamx_place_db_destroy(loamx_ctx* ctx, loamx_place_db* db) {
  if (!db) return;
  if (ctx) {
    std::lock_guard<std::mutex> guard(ctx->mu);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);  // (kernels still reading the entries)
    db_free(db);
    return;
  }
  db_free(db);
}

int loamx_place_db_sector_dirs(const loamx_place_db* db, double* dirs) {
  if (!db || !dirs) return LOAMX_ERR_BAD_PARAM;
  memcpy(dirs, db->dirs.data(), db->dirs.size() * sizeof(double));
  return LOAMX_OK;
}

int loamx_place_db_size(const loamx_place_db* db, size_t* n_entries) {
  if (!db || !n_entries) return LOAMX_ERR_BAD_PARAM;
  *n_entries = db->n;
  return LOAMX_OK;
}

int loamx_place_descriptors_dev(loamx_ctx* ctx, const loamx_place_db* db, const double* d_points, size_t point_stride, const size_t* cloud_offsets,
                                size_t n_clouds, uint16_t* d_desc) {
  return descriptors_dev(ctx, db, d_points, false, point_stride, cloud_offsets, n_clouds, d_desc);
}
int loamx_place_descriptors_dev_f32(loamx_ctx* ctx, const loamx_place_db* db, const float* d_points, size_t point_stride, const size_t* cloud_offsets,
                                    size_t n_clouds, uint16_t* d_desc) {
  return descriptors_dev(ctx, db, d_points, true, point_stride, cloud_offsets, n_clouds, d_desc);
}
int loamx_place_descriptor(loamx_ctx* ctx, const loamx_place_db* db, const double* points, size_t point_stride, size_t n_points, uint16_t* desc) {
  return descriptor_host(ctx, db, points, false, point_stride, n_points, desc);
}
int loamx_place_descriptor_f32(loamx_ctx* ctx, const loamx_place_db* db, const float* points, size_t point_stride, size_t n_points, uint16_t* desc) {
  return descriptor_host(ctx, db, points, true, point_stride, n_points, desc);
}

int loamx_place_db_add_dev(loamx_ctx* ctx, loamx_place_db* db, const uint16_t* d_desc, size_t n, uint32_t* first_id) {
  API_ENTER(ctx);
  int rc = db_check(ctx, db);
  if (rc != LOAMX_OK) return rc;
  if (n == 0) {
    if (first_id) *first_id = (uint32_t)db->n;
    return LOAMX_OK;
  }
  if (!d_desc) return fail(ctx, LOAMX_ERR_BAD_PARAM, "null descriptors");
  if (n > kPlaceMaxEntries || db->n + n > kPlaceMaxEntries) return fail(ctx, LOAMX_ERR_UNSUPPORTED, "a place database holds at most 2^24 entries");
  rc = db_grow(ctx, db, db->n + n);
  if (rc != LOAMX_OK) return rc;
  const size_t RS = (size_t)db->shape.R * db->shape.S;
  untimed(ctx);
  HIP_TRY(ctx, hipMemcpyAsync(db->d_desc + db->n * RS, d_desc, n * RS * sizeof(uint16_t), hipMemcpyDeviceToDevice, ctx->stream));
  launch_place_keys(db->d_desc + db->n * RS, n, db->shape, db->d_keys + db->n * db->shape.R, db->d_norms + db->n * db->shape.S, ctx->stream);
  CHECK_LAUNCH(ctx, "place key kernel");
  if (first_id) *first_id = (uint32_t)db->n;
  db->n += n;
  return LOAMX_OK;
}

int loamx_place_db_read(loamx_ctx* ctx, const loamx_place_db* db, size_t first, size_t count, uint16_t* desc, uint32_t* keys, uint64_t* norms) {
  API_ENTER(ctx);
  int rc = db_check(ctx, db);
  if (rc != LOAMX_OK) return rc;
  if (first > db->n || count > db->n - first) return fail(ctx, LOAMX_ERR_BAD_PARAM, "entries beyond the database's size");
  if (count == 0) return LOAMX_OK;
  const size_t R = db->shape.R, S = db->shape.S;
  if (desc) HIP_TRY(ctx, hipMemcpyAsync(desc, db->d_desc + first * R * S, count * R * S * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream));
  if (keys) HIP_TRY(ctx, hipMemcpyAsync(keys, db->d_keys + first * R, count * R * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (norms) HIP_TRY(ctx, hipMemcpyAsync(norms, db->d_norms + first * S, count * S * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LOAMX_OK;
}

int loamx_place_search_dev(loamx_ctx* ctx, const loamx_place_db* db, const uint16_t* d_query_desc, size_t n_queries, const uint32_t* id_end,
                           uint32_t num_candidates, loamx_place_match* d_out) {
  API_ENTER(ctx);
  int rc = search_check(ctx, db, d_query_desc, n_queries, num_candidates, d_out);
  if (rc != LOAMX_OK || n_queries == 0) return rc;
  return search_locked(ctx, db, d_query_desc, n_queries, id_end, num_candidates, d_out);
}

int loamx_place_search(loamx_ctx* ctx, const loamx_place_db* db, const uint16_t* query_desc, size_t n_queries, const uint32_t* id_end,
                       uint32_t num_candidates, loamx_place_match* out) {
  API_ENTER(ctx);
  int rc = search_check(ctx, db, query_desc, n_queries, num_candidates, out);
  if (rc != LOAMX_OK || n_queries == 0) return rc;
  const size_t in_bytes = n_queries * db->shape.R * db->shape.S * sizeof(uint16_t), out_bytes = n_queries * num_candidates * sizeof(loamx_place_match);
  untimed(ctx);
  ENSURE(ctx, WS_PLACE_IN, in_bytes);
  ENSURE(ctx, WS_PLACE_OUT, out_bytes);
  HIP_TRY(ctx, hipMemcpyAsync(ctx->ws[WS_PLACE_IN].p, query_desc, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  rc = search_locked(ctx, db, wsp<uint16_t>(ctx, WS_PLACE_IN), n_queries, id_end, num_candidates, wsp<loamx_place_match>(ctx, WS_PLACE_OUT));
  if (rc != LOAMX_OK) {
    (void)hipStreamSynchronize(ctx->stream);  // (the upload must not outlive the caller's array)
    return rc;
  }
  HIP_TRY(ctx, hipMemcpyAsync(out, ctx->ws[WS_PLACE_OUT].p, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LOAMX_OK;
}

}  // extern "C"
