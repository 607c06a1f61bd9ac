// api_comm.hip — multi-GPU batch mode: RCCL gather of the result records. The one unit that knows RCCL.
#include <dlfcn.h>
#include <rccl/rccl.h>  // types and prototypes only: the library itself is opened on first use (struct Rccl below)

#include "api_host.h"

using namespace loamx;

struct loamx_comm {
  ncclComm_t comm = nullptr;
  bool owned = false;
  int world = 1, rank = 0, device = 0;
  double* d_scalar = nullptr;  // barrier / max-reduce scratch (device)
  uint64_t enqueued[LOAMX_COMM_STAT_COUNT] = {};  // what loamx_gather_results_dev / loamx_comm_barrier really enqueued
};

namespace {
// RCCL is opened when the first loamx_comm_* entry point runs: single-GPU users and the host entry points load
// libloamx.so on a machine without librccl. (In a process that imported torch first, "librccl.so.1" resolves to the copy
// torch already mapped: same SONAME.)
struct Rccl {
#define LOAMX_RCCL_FN(name) decltype(&::nccl##name) name = nullptr;
  LOAMX_RCCL_FN(CommCount) LOAMX_RCCL_FN(CommUserRank) LOAMX_RCCL_FN(CommCuDevice) LOAMX_RCCL_FN(GetUniqueId)
  LOAMX_RCCL_FN(CommInitRank) LOAMX_RCCL_FN(GetErrorString) LOAMX_RCCL_FN(CommDestroy) LOAMX_RCCL_FN(AllGather)
  LOAMX_RCCL_FN(GroupStart) LOAMX_RCCL_FN(GroupEnd) LOAMX_RCCL_FN(Broadcast) LOAMX_RCCL_FN(AllReduce)
#undef LOAMX_RCCL_FN
  std::string error;
  bool ok = false;
  Rccl() {
    void* h = nullptr;
    // LOAMX_RCCL_LIB names the one library to open (a site-specific build; the tests point it at a missing file)
    const char* forced = getenv("LOAMX_RCCL_LIB");
    std::string why;
    for (const char* n : {forced ? forced : "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      if ((h = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
      // dlerror() clears the message it returns: read it ONCE per failed attempt (the first attempt's message is kept)
      const char* e = dlerror();
      if (why.empty()) why = std::string(n) + ": " + (e ? e : "?");
      if (forced) break;
    }
    if (!h) {
      error = "librccl not found: " + why;
      return;
    }
    bool all = true;
#define LOAMX_RCCL_FN(name) all &= (name = reinterpret_cast<decltype(name)>(dlsym(h, "nccl" #name))) != nullptr;
    LOAMX_RCCL_FN(CommCount) LOAMX_RCCL_FN(CommUserRank) LOAMX_RCCL_FN(CommCuDevice) LOAMX_RCCL_FN(GetUniqueId)
    LOAMX_RCCL_FN(CommInitRank) LOAMX_RCCL_FN(GetErrorString) LOAMX_RCCL_FN(CommDestroy) LOAMX_RCCL_FN(AllGather)
    LOAMX_RCCL_FN(GroupStart) LOAMX_RCCL_FN(GroupEnd) LOAMX_RCCL_FN(Broadcast) LOAMX_RCCL_FN(AllReduce)
#undef LOAMX_RCCL_FN
    ok = all;
    if (!ok) error = "librccl lacks an expected ncclXxx symbol";
  }
};
const Rccl& rccl() {
  static const Rccl r;
  return r;
}
#define RCCL_NEED(ctx)                                                          \
  do {                                                                          \
    if (!rccl().ok) return fail(ctx, LOAMX_ERR_COMM, rccl().error);             \
  } while (0)
#define NCCL_TRY(ctx, expr)                                                                        \
  do {                                                                                             \
    ncclResult_t r_ = (expr);                                                                      \
    if (r_ != ncclSuccess) return fail(ctx, LOAMX_ERR_COMM, std::string(#expr) + ": " + rccl().GetErrorString(r_)); \
  } while (0)

int comm_finish_init(loamx_ctx* ctx, loamx_comm* c) {
  NCCL_TRY(ctx, rccl().CommCount(c->comm, &c->world));
  NCCL_TRY(ctx, rccl().CommUserRank(c->comm, &c->rank));
  NCCL_TRY(ctx, rccl().CommCuDevice(c->comm, &c->device));
  if (c->device != ctx->device) return fail(ctx, LOAMX_ERR_BAD_PARAM, "communicator and context live on different devices");
  HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&c->d_scalar), 2 * sizeof(double)));
  return LOAMX_OK;
}
}  // namespace

extern "C" {

void loamx_shard_range(size_t total_pairs, int world_size, int rank, size_t* first, size_t* count) {
  const size_t w = world_size > 0 ? (size_t)world_size : 1, r = rank > 0 ? (size_t)rank : 0;
  const size_t base = total_pairs / w, rem = total_pairs % w;
  if (first) *first = r * base + (r < rem ? r : rem);
  if (count) *count = r < w ? base + (r < rem ? 1 : 0) : 0;
}

int loamx_comm_get_unique_id(unsigned char id_out[LOAMX_COMM_ID_BYTES]) {
  static_assert(LOAMX_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "id size");
  if (!id_out) return LOAMX_ERR_BAD_PARAM;
  if (!rccl().ok) return LOAMX_ERR_COMM;
  ncclUniqueId id;
  if (rccl().GetUniqueId(&id) != ncclSuccess) return LOAMX_ERR_COMM;
  memcpy(id_out, id.internal, NCCL_UNIQUE_ID_BYTES);
  return LOAMX_OK;
}

int loamx_comm_create(loamx_ctx* ctx, const unsigned char id[LOAMX_COMM_ID_BYTES], int world_size, int rank, loamx_comm** out) {
  if (!ctx || !id || !out) return LOAMX_ERR_BAD_PARAM;
  *out = nullptr;
  API_LOCK(ctx);
  if (world_size < 1 || rank < 0 || rank >= world_size) return fail(ctx, LOAMX_ERR_BAD_PARAM, "bad world size / rank");
  RCCL_NEED(ctx);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ncclUniqueId uid;
  memcpy(uid.internal, id, NCCL_UNIQUE_ID_BYTES);
  loamx_comm* c = new loamx_comm;
  c->owned = true;
  ncclResult_t r = rccl().CommInitRank(&c->comm, world_size, uid, rank);
  if (r != ncclSuccess) {
    delete c;
    return fail(ctx, LOAMX_ERR_COMM, std::string("ncclCommInitRank: ") + rccl().GetErrorString(r));
  }
  int rc = comm_finish_init(ctx, c);
  if (rc != LOAMX_OK) {
    loamx_comm_destroy(c);
    return rc;
  }
  *out = c;
  return LOAMX_OK;
}

int loamx_comm_wrap(loamx_ctx* ctx, void* nccl_comm, loamx_comm** out) {
  if (!ctx || !nccl_comm || !out) return LOAMX_ERR_BAD_PARAM;
  *out = nullptr;
  API_LOCK(ctx);
  RCCL_NEED(ctx);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  loamx_comm* c = new loamx_comm;
  c->comm = static_cast<ncclComm_t>(nccl_comm), c->owned = false;
  int rc = comm_finish_init(ctx, c);
  if (rc != LOAMX_OK) {
    loamx_comm_destroy(c);
    return rc;
  }
  *out = c;
  return LOAMX_OK;
}

void loamx_comm_destroy(loamx_comm* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->d_scalar) (void)hipFree(c->d_scalar);
  if (c->owned && c->comm && rccl().ok) (void)rccl().CommDestroy(c->comm);
  delete c;
}

int loamx_comm_info(const loamx_comm* c, int* world_size, int* rank, int* device) {
  if (!c) return LOAMX_ERR_BAD_PARAM;
  if (world_size) *world_size = c->world;
  if (rank) *rank = c->rank;
  if (device) *device = c->device;
  return LOAMX_OK;
}

int loamx_gather_results_dev(loamx_ctx* ctx, loamx_comm* c, const loamx_reg_result* d_local, size_t n_local, size_t total_pairs,
                             loamx_reg_result* d_all) {
  if (!ctx || !c || !d_all || (n_local && !d_local)) return LOAMX_ERR_BAD_PARAM;
  API_ENTER(ctx);
  size_t first = 0, count = 0;
  loamx_shard_range(total_pairs, c->world, c->rank, &first, &count);
  if (count != n_local) return fail(ctx, LOAMX_ERR_BAD_PARAM, "n_local is not this rank's shard of total_pairs (loamx_shard_range)");
  if (total_pairs == 0) return LOAMX_OK;
  untimed(ctx);
  hipStream_t s = ctx->stream;
  static_assert(sizeof(loamx_reg_result) == 64, "record size");
  // One rank: a device copy — unless option FORCE_RCCL is set, which sends the one-rank communicator through BOTH collective
  // forms below (the all-gather, then the grouped broadcast in place: same bytes), so that they have executed before
  // the first multi-GPU node runs them.
  const bool forced = c->world == 1 && (ctx->reg_flags & kRegFlagForceRccl) != 0;
  if (c->world == 1 && !forced) {
    if (d_all != d_local) HIP_TRY(ctx, hipMemcpyAsync(d_all, d_local, n_local * sizeof(loamx_reg_result), hipMemcpyDeviceToDevice, s));
    c->enqueued[LOAMX_COMM_STAT_MEMCPY]++;
    return LOAMX_OK;
  }
  if (total_pairs % (size_t)c->world == 0) {  // equal shards: one all-gather of n_local * 64 bytes per rank
    NCCL_TRY(ctx, rccl().AllGather(d_local, d_all, n_local * sizeof(loamx_reg_result), ncclChar, c->comm, s));
    c->enqueued[LOAMX_COMM_STAT_ALL_GATHER]++;
    if (!forced) return LOAMX_OK;
    d_local = d_all;  // (forced: the broadcast form runs in place on what the all-gather delivered)
  }
  // uneven shards (sizes differ by one): every rank broadcasts its block to its place, as one grouped operation
  NCCL_TRY(ctx, rccl().GroupStart());
  for (int r = 0; r < c->world; r++) {
    size_t f = 0, n = 0;
    loamx_shard_range(total_pairs, c->world, r, &f, &n);
    if (n == 0) continue;
    ncclResult_t rr = rccl().Broadcast(r == c->rank ? static_cast<const void*>(d_local) : static_cast<const void*>(d_all + f), d_all + f,
                                    n * sizeof(loamx_reg_result), ncclChar, r, c->comm, s);
    if (rr != ncclSuccess) {
      (void)rccl().GroupEnd();
      return fail(ctx, LOAMX_ERR_COMM, std::string("ncclBroadcast: ") + rccl().GetErrorString(rr));
    }
    c->enqueued[LOAMX_COMM_STAT_BROADCAST]++;
  }
  NCCL_TRY(ctx, rccl().GroupEnd());
  return LOAMX_OK;
}

int loamx_comm_stats(const loamx_comm* c, uint64_t counts[LOAMX_COMM_STAT_COUNT]) {
  if (!c || !counts) return LOAMX_ERR_BAD_PARAM;
  for (int i = 0; i < LOAMX_COMM_STAT_COUNT; i++) counts[i] = c->enqueued[i];
  return LOAMX_OK;
}

int loamx_comm_barrier(loamx_ctx* ctx, loamx_comm* c, double* max_value) {
  if (!ctx || !c) return LOAMX_ERR_BAD_PARAM;
  API_ENTER(ctx);
  untimed(ctx);
  hipStream_t s = ctx->stream;
  const double v = max_value ? *max_value : 0.0;
  HIP_TRY(ctx, hipMemcpyAsync(c->d_scalar, &v, sizeof(double), hipMemcpyHostToDevice, s));
  if (c->world > 1 || (ctx->reg_flags & kRegFlagForceRccl)) {
    NCCL_TRY(ctx, rccl().AllReduce(c->d_scalar, c->d_scalar + 1, 1, ncclDouble, ncclMax, c->comm, s));
    c->enqueued[LOAMX_COMM_STAT_ALL_REDUCE]++;
  } else {
    HIP_TRY(ctx, hipMemcpyAsync(c->d_scalar + 1, c->d_scalar, sizeof(double), hipMemcpyDeviceToDevice, s));
    c->enqueued[LOAMX_COMM_STAT_MEMCPY]++;
  }
  double o = 0.0;
  HIP_TRY(ctx, hipMemcpyAsync(&o, c->d_scalar + 1, sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  if (max_value) *max_value = o;
  return LOAMX_OK;
}

}  // extern "C"
