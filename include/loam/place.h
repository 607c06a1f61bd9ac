/** @brief Extension (not in the reference): place recognition on the device.
 *
 * Drift from scan-to-scan registration is unbounded; a mapper bounds it by noticing that it has been somewhere before. A
 * PlaceDatabase holds one descriptor per scan — the Scan Context form: a polar grid of maximum heights, n_rings x n_sectors
 * uint16 — and search returns the stored scans nearest to a query under every column shift, with the shift as a yaw guess for
 * the registration that makes the loop edge (PlaceMatch::initialGuess). The rule is written out in loamx.h
 * ("place recognition"); results do not depend on how the device schedules its threads.
 */
#pragma once
#include <cmath>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <vector>

#include "common.h"
#include "geometry.h"

namespace loam {

/// loamx_place_params; the defaults are loamx_default_place_params'
struct PlaceParams {
  uint32_t n_rings = 20;
  uint32_t n_sectors = 60;
  double max_range = 80.0;
  double z_offset = 2.0;  ///< sensor height above ground: makes heights positive
  double z_scale = 64.0;  ///< codes per metre
};

/// One record of a search (loamx_place_match)
struct PlaceMatch {
  static constexpr uint32_t kNoEntry = 0xFFFFFFFFu;
  uint32_t id = kNoEntry;       ///< the stored scan, or kNoEntry when fewer entries were eligible than candidates asked for
  uint32_t shift = 0;           ///< sectors the query sensor is turned counter-clockwise relative to the entry's
  uint64_t key_dist = ~0ull;    ///< squared ring-key distance
  double distance = 2.0;        ///< 0 .. 1; 2 without an entry
  uint32_t n_sectors = 60;      ///< of the database that made the record
  bool valid() const { return id != kNoEntry; }
  /// rotation about z by shift x 2 pi / n_sectors, in radians
  double yaw() const { return 6.283185307179586476925286766559 * (double)shift / (double)n_sectors; }
  /// entry_T_query as the shift alone suggests it: the yaw, no translation
  Pose3d initialGuess() const {
    const double h = 0.5 * yaw();
    return Pose3d(Quaterniond(std::cos(h), 0.0, 0.0, std::sin(h)), Vector3d::Zero());
  }
};

using PlaceDescriptor = std::vector<uint16_t>;  ///< n_rings x n_sectors, row-major [ring][sector]

/// The database (loamx_place_db): parameters, sector table and stored entries on the device. Cheap to copy (shared handle).
class PlaceDatabase {
 public:
  explicit PlaceDatabase(const PlaceParams& params = PlaceParams()) : params_(params) {
    loamx_ctx* ctx = gpu::defaultContext();
    loamx_place_params p;
    loamx_default_place_params(&p);
    p.n_rings = params.n_rings, p.n_sectors = params.n_sectors, p.max_range = params.max_range;
    p.z_offset = params.z_offset, p.z_scale = params.z_scale;
    loamx_place_db* h = nullptr;
    gpu::check(ctx, loamx_place_db_create(ctx, &p, &h));
    handle_ = std::shared_ptr<loamx_place_db>(h, [](loamx_place_db* d) { loamx_place_db_destroy(gpu::defaultContext(), d); });
  }
  const PlaceParams& params() const { return params_; }
  size_t cells() const { return (size_t)params_.n_rings * params_.n_sectors; }
  size_t size() const {
    size_t n = 0;
    loamx_place_db_size(handle_.get(), &n);
    return n;
  }
  /// u_k of the sector boundaries, n_sectors x 2, exactly as the kernels use them
  std::vector<double> sectorDirections() const {
    std::vector<double> v(2 * (size_t)params_.n_sectors);
    loamx_place_db_sector_dirs(handle_.get(), v.data());
    return v;
  }
  /// The descriptor of a scan or of an unordered cloud in the sensor frame; the database is not changed. Float fields read
  /// through FieldAccessor travel as floats, like the scans of extractFeatures.
  template <template <typename> class Accessor = FieldAccessor, typename PointType, typename Alloc>
  PlaceDescriptor descriptor(const std::vector<PointType, Alloc>& points) const {
    PlaceDescriptor d(cells());
    loamx_ctx* ctx = gpu::defaultContext();
    if constexpr (gpu::float_scan_v<Accessor, PointType>) {
      const std::vector<float> xyz = gpu::packFloat(points);
      gpu::check(ctx, loamx_place_descriptor_f32(ctx, handle_.get(), xyz.data(), 3, points.size(), d.data()));
    } else {
      const std::vector<double> xyz = gpu::pack<Accessor>(points);
      gpu::check(ctx, loamx_place_descriptor(ctx, handle_.get(), xyz.data(), 3, points.size(), d.data()));
    }
    return d;
  }
  /// Appends one descriptor; returns its id (ids are consecutive from 0)
  uint32_t add(const PlaceDescriptor& desc) {
    if (desc.size() != cells()) throw std::runtime_error("loam::PlaceDatabase::add: a descriptor holds n_rings x n_sectors codes");
    loamx_ctx* ctx = gpu::defaultContext();
    void* d = nullptr;
    gpu::check(ctx, loamx_dev_alloc(ctx, desc.size() * sizeof(uint16_t), &d));
    uint32_t first = 0;
    int rc = loamx_copy_to_device(ctx, d, desc.data(), desc.size() * sizeof(uint16_t));
    if (rc == LOAMX_OK) rc = loamx_place_db_add_dev(ctx, handle_.get(), static_cast<const uint16_t*>(d), 1, &first);
    if (rc == LOAMX_OK) rc = loamx_ctx_synchronize(ctx);
    loamx_dev_free(ctx, d);
    gpu::check(ctx, rc);
    return first;
  }
  /// The num_candidates (1 .. 64) records of one query among the entries with id < id_end, ascending by (distance, id)
  std::vector<PlaceMatch> search(const PlaceDescriptor& query, uint32_t num_candidates, uint32_t id_end = 0xFFFFFFFFu) const {
    if (query.size() != cells()) throw std::runtime_error("loam::PlaceDatabase::search: a descriptor holds n_rings x n_sectors codes");
    loamx_ctx* ctx = gpu::defaultContext();
    std::vector<loamx_place_match> rec(num_candidates);
    gpu::check(ctx, loamx_place_search(ctx, handle_.get(), query.data(), 1, &id_end, num_candidates, rec.data()));
    std::vector<PlaceMatch> out(rec.size());
    for (size_t i = 0; i < rec.size(); i++) {
      out[i].id = rec[i].id, out[i].shift = rec[i].shift, out[i].key_dist = rec[i].key_dist, out[i].distance = rec[i].distance;
      out[i].n_sectors = params_.n_sectors;
    }
    return out;
  }
  loamx_place_db* handle() const { return handle_.get(); }

 private:
  PlaceParams params_;
  std::shared_ptr<loamx_place_db> handle_;
};

}  // namespace loam
