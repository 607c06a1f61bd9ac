// loam_bindings.cpp — pybind11 module `loam_python` (re-exported as `loam`), same surface as the
// reference's python/loam_bindings.cpp:24-144: LidarParams, Pose3d, Quaterniond,
// FeatureExtractionParams, LoamFeatures, extractFeatures, computeCurvature, computeValidPoints,
// RegistrationParams, RegistrationIterationInfo, RegistrationTerminationType, RegistrationDetail,
// registerFeatures — with the same keyword arguments; plus extensions the reference does not have: registerScanSequence
// and deskewScan (include/loamx.h: "scan sequences"), and the class TargetIndex with a registerFeatures overload that
// takes it (scan-to-map: "persistent target index" and "map upkeep"), and OrganizeParams / ScanLayout / organizeCloud, the way
// in for clouds that are not organised scans yet ("unordered clouds into scans"), and PlaceParams / PlaceMatch / PlaceDatabase
// ("place recognition"), and PoseGraphParams / PoseGraphSummary / PoseGraph ("pose graph"), and SegmentationParams / segmentScan
// ("scan segmentation"), and VisibilityParams / visibilityVotes / removeDynamicPoints ("map cleaning"). Point clouds are
// contiguous (N,3) float64 arrays handed to the C ABI without per-point objects (a list of 3-vectors is converted once).
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>
#include <optional>

#include "loam/loam.h"

namespace py = pybind11;
using Arr = py::array_t<double, py::array::c_style | py::array::forcecast>;
// float32 scans (PCL-style sensors data) are taken as they are (no cast: only a C-contiguous float32 array
// matches) and go through the FP32-input entry points of the C ABI
using ArrF = py::array_t<float, py::array::c_style>;

namespace {

struct PyFeatures {
  Arr edge_points;
  Arr planar_points;
  PyFeatures() : edge_points(std::vector<py::ssize_t>{0, 3}), planar_points(std::vector<py::ssize_t>{0, 3}) {}
};

template <typename A>
size_t check_points(const A& a, const char* what) {
  if (a.ndim() == 1 && a.shape(0) == 0) return 0;
  if (a.ndim() != 2 || a.shape(1) != 3) throw std::runtime_error(std::string(what) + ": expected an (N, 3) array of points");
  return (size_t)a.shape(0);
}

template <typename A>
Arr gather_points(const A& scan, const std::vector<uint32_t>& idx, size_t n) {
  Arr out(std::vector<py::ssize_t>{(py::ssize_t)n, 3});
  const auto* src = scan.data();
  double* dst = out.mutable_data();
  for (size_t i = 0; i < n; i++)
    for (int k = 0; k < 3; k++) dst[3 * i + k] = (double)src[3 * (size_t)idx[i] + k];
  return out;
}

// one body for float64 and float32 scans: the C ABI entry points differ only in the scalar type
inline int c_extract(loamx_ctx* c, const double* x, size_t n, const loamx_lidar_params* l, const loamx_fe_params* f, uint32_t* e,
                     size_t ec, size_t* ne, uint32_t* p, size_t pc, size_t* np) {
  return loamx_extract_features(c, x, n, l, f, e, ec, ne, p, pc, np);
}
inline int c_extract(loamx_ctx* c, const float* x, size_t n, const loamx_lidar_params* l, const loamx_fe_params* f, uint32_t* e,
                     size_t ec, size_t* ne, uint32_t* p, size_t pc, size_t* np) {
  return loamx_extract_features_f32(c, x, n, l, f, e, ec, ne, p, pc, np);
}
inline int c_curvature(loamx_ctx* c, const double* x, size_t n, const loamx_lidar_params* l, const loamx_fe_params* f, double* o) {
  return loamx_compute_curvature(c, x, n, l, f, o);
}
inline int c_curvature(loamx_ctx* c, const float* x, size_t n, const loamx_lidar_params* l, const loamx_fe_params* f, double* o) {
  return loamx_compute_curvature_f32(c, x, n, l, f, o);
}
inline int c_valid(loamx_ctx* c, const double* x, size_t n, const loamx_lidar_params* l, const loamx_fe_params* f, uint8_t* o) {
  return loamx_compute_valid_points(c, x, n, l, f, o);
}
inline int c_valid(loamx_ctx* c, const float* x, size_t n, const loamx_lidar_params* l, const loamx_fe_params* f, uint8_t* o) {
  return loamx_compute_valid_points_f32(c, x, n, l, f, o);
}

inline int c_sequence(loamx_ctx* c, const double* x, size_t n, const loamx_lidar_params* l, const loamx_fe_params* f, const loamx_reg_params* r,
                      const double* init, loamx_reg_result* out) {
  return loamx_register_scan_sequence(c, x, n, l, f, r, init, out);
}
inline int c_sequence(loamx_ctx* c, const float* x, size_t n, const loamx_lidar_params* l, const loamx_fe_params* f, const loamx_reg_params* r,
                      const double* init, loamx_reg_result* out) {
  return loamx_register_scan_sequence_f32(c, x, n, l, f, r, init, out);
}
inline int c_deskew(loamx_ctx* c, const double* in, const loamx_lidar_params* l, const double* motion, double rho, double* out) {
  return loamx_deskew_scans_dev(c, in, 1, l, motion, rho, out);
}
inline int c_deskew(loamx_ctx* c, const float* in, const loamx_lidar_params* l, const double* motion, double rho, float* out) {
  return loamx_deskew_scans_dev_f32(c, in, 1, l, motion, rho, out);
}


// organizeCloud: (N, 3) or (N, k >= 3) points as they lie in the array (the stride is the row length), rings or None
inline int c_organize(loamx_ctx* c, const loamx_scan_layout* l, const double* p, size_t stride, const uint16_t* r, size_t n, double* s, uint32_t* i,
                      uint32_t* st) {
  return loamx_organize_cloud(c, l, p, stride, r, n, s, i, st);
}
inline int c_organize(loamx_ctx* c, const loamx_scan_layout* l, const float* p, size_t stride, const uint16_t* r, size_t n, float* s, uint32_t* i,
                      uint32_t* st) {
  return loamx_organize_cloud_f32(c, l, p, stride, r, n, s, i, st);
}
using ArrRings = py::array_t<uint16_t, py::array::c_style | py::array::forcecast>;

// PlaceDatabase: descriptors are (n_rings, n_sectors) uint16 arrays; points as for organizeCloud
using ArrDesc = py::array_t<uint16_t, py::array::c_style | py::array::forcecast>;
inline int c_place_descriptor(loamx_ctx* c, const loamx_place_db* d, const double* p, size_t stride, size_t n, uint16_t* out) {
  return loamx_place_descriptor(c, d, p, stride, n, out);
}
inline int c_place_descriptor(loamx_ctx* c, const loamx_place_db* d, const float* p, size_t stride, size_t n, uint16_t* out) {
  return loamx_place_descriptor_f32(c, d, p, stride, n, out);
}
template <typename T>
py::array_t<uint16_t> place_descriptor(const loam::PlaceDatabase& db, const py::array_t<T, py::array::c_style>& points) {
  if (points.ndim() != 2 || points.shape(1) < 3) throw std::runtime_error("points: expected an (N, 3) or (N, 4) array");
  py::array_t<uint16_t> desc({(py::ssize_t)db.params().n_rings, (py::ssize_t)db.params().n_sectors});
  loamx_ctx* ctx = loam::gpu::defaultContext();
  {
    py::gil_scoped_release release;
    loam::gpu::check(ctx, c_place_descriptor(ctx, db.handle(), points.data(), (size_t)points.shape(1), (size_t)points.shape(0), desc.mutable_data()));
  }
  return desc;
}
inline loam::PlaceDescriptor place_desc_arg(const loam::PlaceDatabase& db, const ArrDesc& desc) {
  if ((size_t)desc.size() != db.cells()) throw std::runtime_error("descriptor: expected an (n_rings, n_sectors) uint16 array");
  return loam::PlaceDescriptor(desc.data(), desc.data() + desc.size());
}
// CloudMap: points as for organizeCloud; the pose is world_T_sensor or None (the points are in the map frame already)
inline int c_cloud_map_add(loamx_ctx* c, loamx_cloud_map* m, const double* p, size_t stride, size_t n, const double* pose) {
  return loamx_cloud_map_add_cloud(c, m, p, stride, n, pose);
}
inline int c_cloud_map_add(loamx_ctx* c, loamx_cloud_map* m, const float* p, size_t stride, size_t n, const double* pose) {
  return loamx_cloud_map_add_cloud_f32(c, m, p, stride, n, pose);
}
template <typename T>
void cloud_map_add(loam::CloudMap& map, const py::array_t<T, py::array::c_style>& points, const std::optional<loam::Pose3d>& world_T_sensor) {
  if (points.ndim() != 2 || points.shape(1) < 3) throw std::runtime_error("points: expected an (N, 3) or (N, 4) array");
  double pose[7];
  if (world_T_sensor) world_T_sensor->toArray(pose);
  loamx_ctx* ctx = loam::gpu::defaultContext();
  py::gil_scoped_release release;
  loam::gpu::check(ctx, c_cloud_map_add(ctx, map.handle(), points.data(), (size_t)points.shape(1), (size_t)points.shape(0),
                                        world_T_sensor ? pose : nullptr));
}
// SurfelMap: points and pose as for CloudMap
inline int c_surfel_map_add(loamx_ctx* c, loamx_surfel_map* m, const double* p, size_t stride, size_t n, const double* pose) {
  return loamx_surfel_map_add_cloud_host(c, m, p, stride, n, pose);
}
inline int c_surfel_map_add(loamx_ctx* c, loamx_surfel_map* m, const float* p, size_t stride, size_t n, const double* pose) {
  return loamx_surfel_map_add_cloud_host_f32(c, m, p, stride, n, pose);
}
template <typename T>
void surfel_map_add(loam::SurfelMap& map, const py::array_t<T, py::array::c_style>& points, const std::optional<loam::Pose3d>& world_T_sensor) {
  if (points.ndim() != 2 || points.shape(1) < 3) throw std::runtime_error("points: expected an (N, 3) or (N, 4) array");
  double pose[7];
  if (world_T_sensor) world_T_sensor->toArray(pose);
  loamx_ctx* ctx = loam::gpu::defaultContext();
  py::gil_scoped_release release;
  loam::gpu::check(ctx, c_surfel_map_add(ctx, map.handle(), points.data(), (size_t)points.shape(1), (size_t)points.shape(0),
                                         world_T_sensor ? pose : nullptr));
}
// SurfelMap.localize: points as for add, from init = map_T_cloud -> (pose, result, information)
inline int c_localize(loamx_ctx* c, loamx_surfel_localizer* l, const double* p, size_t stride, size_t n, const double* pose, const loamx_localize_params* lp,
                      loamx_localize_result* res, loamx_reg_information* info) {
  return loamx_surfel_localizer_run_host(c, l, p, stride, n, pose, lp, res, info);
}
inline int c_localize(loamx_ctx* c, loamx_surfel_localizer* l, const float* p, size_t stride, size_t n, const double* pose, const loamx_localize_params* lp,
                      loamx_localize_result* res, loamx_reg_information* info) {
  return loamx_surfel_localizer_run_host_f32(c, l, p, stride, n, pose, lp, res, info);
}
template <typename T>
py::tuple surfel_map_localize(loam::SurfelMap& map, const py::array_t<T, py::array::c_style>& points, const loam::Pose3d& init,
                              const loam::LocalizeParams& params) {
  if (points.ndim() != 2 || points.shape(1) < 3) throw std::runtime_error("points: expected an (N, 3) or (N, 4) array");
  loamx_localize_params p;
  loamx_default_localize_params(&p);
  p.neighborhood = params.neighborhood, p.min_points = params.min_points, p.planarity = params.planarity;
  p.max_distance = params.max_distance, p.huber_delta = params.huber_delta, p.max_iterations = params.max_iterations;
  p.min_rows = params.min_rows, p.rotation_convergence_thresh = params.rotation_convergence_thresh;
  p.position_convergence_thresh = params.position_convergence_thresh, p.min_eigenvalue_per_row = params.min_eigenvalue_per_row;
  double pose[7];
  init.toArray(pose);
  loamx_ctx* ctx = loam::gpu::defaultContext();
  loamx_surfel_localizer* loc = map.localizer((size_t)points.shape(0));
  loam::LocalizeResult res;
  loamx_reg_information info;
  {
    py::gil_scoped_release release;
    loam::gpu::check(ctx, c_localize(ctx, loc, points.data(), (size_t)points.shape(1), (size_t)points.shape(0), pose, &p, &res, &info));
  }
  return py::make_tuple(loam::Pose3d::fromArray(res.pose), res, loam::gpu::fromC(info));
}
// surfels as a dict of arrays: mean (n, 3), cov (n, 6), eval (n, 3), normal (n, 3), count (n,), first (n,)
inline py::dict surfel_arrays(const std::vector<loam::Surfel>& s) {
  const py::ssize_t n = (py::ssize_t)s.size();
  Arr mean(std::vector<py::ssize_t>{n, 3}), cov(std::vector<py::ssize_t>{n, 6}), eval(std::vector<py::ssize_t>{n, 3}), normal(std::vector<py::ssize_t>{n, 3});
  py::array_t<uint32_t> count(n), first(n);
  for (py::ssize_t i = 0; i < n; i++) {
    std::memcpy(mean.mutable_data() + 3 * i, s[i].mean, sizeof(s[i].mean));
    std::memcpy(cov.mutable_data() + 6 * i, s[i].cov, sizeof(s[i].cov));
    std::memcpy(eval.mutable_data() + 3 * i, s[i].eval, sizeof(s[i].eval));
    std::memcpy(normal.mutable_data() + 3 * i, s[i].normal, sizeof(s[i].normal));
    count.mutable_data()[i] = s[i].count, first.mutable_data()[i] = s[i].first;
  }
  py::dict d;
  d["mean"] = mean, d["cov"] = cov, d["eval"] = eval, d["normal"] = normal, d["count"] = count, d["first"] = first;
  return d;
}
// OccupancyMap: points and pose as for CloudMap
inline int c_occupancy_add(loamx_ctx* c, loamx_occupancy_map* m, const double* p, size_t stride, size_t n, const double* pose) {
  return loamx_occupancy_add_cloud(c, m, p, stride, n, pose);
}
inline int c_occupancy_add(loamx_ctx* c, loamx_occupancy_map* m, const float* p, size_t stride, size_t n, const double* pose) {
  return loamx_occupancy_add_cloud_f32(c, m, p, stride, n, pose);
}
template <typename T>
void occupancy_add(loam::OccupancyMap& map, const py::array_t<T, py::array::c_style>& points, const std::optional<loam::Pose3d>& world_T_sensor) {
  if (points.ndim() != 2 || points.shape(1) < 3) throw std::runtime_error("points: expected an (N, 3) or (N, 4) array");
  double pose[7];
  if (world_T_sensor) world_T_sensor->toArray(pose);
  loamx_ctx* ctx = loam::gpu::defaultContext();
  py::gil_scoped_release release;
  loam::gpu::check(ctx, c_occupancy_add(ctx, map.handle(), points.data(), (size_t)points.shape(1), (size_t)points.shape(0),
                                        world_T_sensor ? pose : nullptr));
}
// vmin (3 ints) and dims (3 non-negative ints) of a voxel box
inline void occupancy_box_args(const std::array<int64_t, 3>& vmin, const std::array<int64_t, 3>& dims, std::array<int32_t, 3>& v, std::array<uint32_t, 3>& d) {
  for (int a = 0; a < 3; a++) {
    if (vmin[a] < INT32_MIN || vmin[a] > INT32_MAX || dims[a] < 0 || dims[a] > (int64_t)UINT32_MAX) throw std::runtime_error("box: vmin or dims out of range");
    v[a] = (int32_t)vmin[a], d[a] = (uint32_t)dims[a];
  }
}
// the numpy dtype of loamx_ray_record (40 bytes) and the C struct of a RaycastParams
inline py::dtype ray_record_dtype() {
  py::list fields;
  fields.append(py::make_tuple("status", "<u4")), fields.append(py::make_tuple("visits", "<u4"));
  fields.append(py::make_tuple("voxel", "<i4", py::make_tuple(3))), fields.append(py::make_tuple("n_unknown", "<u4"));
  fields.append(py::make_tuple("t_enter", "<f8")), fields.append(py::make_tuple("t_exit", "<f8"));
  return py::dtype::from_args(fields);
}
inline loamx_raycast_params raycast_params(const loam::RaycastParams& params) {
  loamx_raycast_params p;
  loamx_default_raycast_params(&p);
  p.skip_start = params.skip_start, p.unknown_stops = params.unknown_stops ? 1u : 0u, p.max_steps = params.max_steps, p.hit_at = params.hit_at;
  return p;
}
// OccupancyMap.distanceBox / distanceSlice: (d2, offset, metres) shaped like box() / slice()
inline py::tuple occupancy_distance(loam::OccupancyMap& map, const std::array<int64_t, 3>& vmin, const std::array<int64_t, 3>& dims,
                                    const loam::DistanceParams& params, bool slice) {
  std::array<int32_t, 3> v;
  std::array<uint32_t, 3> d;
  occupancy_box_args(vmin, dims, v, d);
  std::vector<py::ssize_t> shape{(py::ssize_t)d[1], (py::ssize_t)d[0]};
  if (!slice) shape.insert(shape.begin(), (py::ssize_t)d[2]);
  std::vector<py::ssize_t> shape_off = shape;
  shape_off.push_back(slice ? 2 : 3);
  py::array_t<uint16_t> d2(shape);
  py::array_t<int16_t> offset(shape_off);
  py::array_t<float> metres(shape);
  loamx_distance_params p;
  loamx_default_distance_params(&p);
  p.max_dist_voxels = params.max_dist_voxels, p.unknown_is_obstacle = params.unknown_is_obstacle ? 1u : 0u;
  loamx_ctx* ctx = loam::gpu::defaultContext();
  loam::gpu::check(ctx, (slice ? loamx_occupancy_distance_slice_host : loamx_occupancy_distance_box_host)(
                            ctx, map.handle(), v.data(), d.data(), &p, d2.mutable_data(), offset.mutable_data(), metres.mutable_data()));
  return py::make_tuple(d2, offset, metres);
}
template <typename T>
py::tuple organize_cloud(const py::array_t<T, py::array::c_style>& points, const loam::ScanLayout& layout, const std::optional<ArrRings>& rings) {
  if (points.ndim() != 2 || points.shape(1) < 3) throw std::runtime_error("points: expected an (N, 3) or (N, 4) array");
  const size_t n = (size_t)points.shape(0), stride = (size_t)points.shape(1);
  if (rings && (rings->ndim() != 1 || (size_t)rings->shape(0) != n)) throw std::runtime_error("rings: expected one ring number per point");
  py::array_t<T> scan(std::vector<py::ssize_t>{(py::ssize_t)layout.cells(), 3});
  py::array_t<uint32_t> src((py::ssize_t)layout.cells());
  uint32_t stats[4];
  loamx_ctx* ctx = loam::gpu::defaultContext();
  {
    py::gil_scoped_release release;
    loam::gpu::check(ctx, c_organize(ctx, layout.handle(), points.data(), stride, rings ? rings->data() : nullptr, n, scan.mutable_data(),
                                     src.mutable_data(), stats));
  }
  return py::make_tuple(scan, src);
}

// visibilityVotes: map points (N, 3) or (N, k) float64, scans (n_scans, H W, 3) as they lie in the array, one pose per scan
// -> votes (N, 4) uint32 [through, agree, occluded, empty]
inline int c_visibility_votes(loamx_ctx* c, const loamx_scan_layout* l, const double* m, size_t stride, size_t n, const double* s, size_t ns,
                              const double* poses, const loamx_visibility_params* p, loamx_visibility_tally* v) {
  return loamx_visibility_votes(c, l, m, stride, n, s, ns, poses, p, v);
}
inline int c_visibility_votes(loamx_ctx* c, const loamx_scan_layout* l, const double* m, size_t stride, size_t n, const float* s, size_t ns,
                              const double* poses, const loamx_visibility_params* p, loamx_visibility_tally* v) {
  return loamx_visibility_votes_f32(c, l, m, stride, n, s, ns, poses, p, v);
}
template <typename T>
py::array_t<uint32_t> visibility_votes(const py::array_t<double, py::array::c_style>& map_points, const py::array_t<T, py::array::c_style>& scans,
                                       const std::vector<loam::Pose3d>& world_T_scan, const loam::ScanLayout& layout,
                                       const loam::VisibilityParams& params) {
  if (map_points.ndim() != 2 || map_points.shape(1) < 3) throw std::runtime_error("map_points: expected an (N, 3) or (N, k) float64 array");
  const size_t n = (size_t)map_points.shape(0), n_scans = world_T_scan.size();
  if ((size_t)scans.size() != n_scans * layout.cells() * 3) throw std::runtime_error("scans: expected (n_scans, H W, 3) with one pose per scan");
  std::vector<double> poses(7 * n_scans);
  for (size_t i = 0; i < n_scans; i++) world_T_scan[i].toArray(poses.data() + 7 * i);
  py::array_t<uint32_t> votes(std::vector<py::ssize_t>{(py::ssize_t)n, 4});
  static_assert(sizeof(loamx_visibility_tally) == 4 * sizeof(uint32_t), "votes travel as rows of four words");
  const loamx_visibility_params vp = loam::gpu::toC(params);
  loamx_ctx* ctx = loam::gpu::defaultContext();
  {
    py::gil_scoped_release release;
    loam::gpu::check(ctx, c_visibility_votes(ctx, layout.handle(), map_points.data(), (size_t)map_points.shape(1), n, scans.data(), n_scans, poses.data(),
                                             &vp, reinterpret_cast<loamx_visibility_tally*>(votes.mutable_data())));
  }
  return votes;
}
// removeDynamicPoints: -> (dynamic (N,) uint8, static_index (K,) uint32, static_points (K, 3) float64)
py::tuple remove_dynamic_points(const py::array_t<double, py::array::c_style>& map_points,
                                const py::array_t<uint32_t, py::array::c_style | py::array::forcecast>& votes, const loam::VisibilityParams& params) {
  if (map_points.ndim() != 2 || map_points.shape(1) < 3) throw std::runtime_error("map_points: expected an (N, 3) or (N, k) float64 array");
  const size_t n = (size_t)map_points.shape(0), stride = (size_t)map_points.shape(1);
  if (votes.ndim() != 2 || (size_t)votes.shape(0) != n || votes.shape(1) != 4) throw std::runtime_error("votes: expected an (N, 4) uint32 array");
  struct P3 {
    double x, y, z;
  };
  std::vector<P3> pts(n);
  for (size_t i = 0; i < n; i++) pts[i] = P3{map_points.data()[i * stride], map_points.data()[i * stride + 1], map_points.data()[i * stride + 2]};
  std::vector<loam::VisibilityVotes> v(n);
  if (n) std::memcpy(v.data(), votes.data(), n * sizeof(loam::VisibilityVotes));
  const auto cleaned = loam::removeDynamicPoints(pts, v, params);
  const size_t k = cleaned.static_index.size();
  py::array_t<uint8_t> dynamic((py::ssize_t)n);
  py::array_t<uint32_t> index((py::ssize_t)k);
  py::array_t<double> kept(std::vector<py::ssize_t>{(py::ssize_t)k, 3});
  if (n) std::memcpy(dynamic.mutable_data(), cleaned.dynamic.data(), n);
  if (k) std::memcpy(index.mutable_data(), cleaned.static_index.data(), k * sizeof(uint32_t));
  if (k) std::memcpy(kept.mutable_data(), cleaned.static_points.data(), k * sizeof(P3));
  return py::make_tuple(dynamic, index, kept);
}

// segmentScan: an organised (H W, 3) scan as it lies in the array -> (classes, labels, sizes, filtered, clusters (n, 4), stats (8,))
inline int c_segment(loamx_ctx* c, const double* s, const loamx_lidar_params* l, const loamx_segment_params* p, uint8_t* cl, uint32_t* la, uint32_t* sz,
                     double* f, loamx_segment_cluster* k, size_t cap, uint32_t* st) {
  return loamx_segment_scan(c, s, l, p, cl, la, sz, f, k, cap, st);
}
inline int c_segment(loamx_ctx* c, const float* s, const loamx_lidar_params* l, const loamx_segment_params* p, uint8_t* cl, uint32_t* la, uint32_t* sz,
                     float* f, loamx_segment_cluster* k, size_t cap, uint32_t* st) {
  return loamx_segment_scan_f32(c, s, l, p, cl, la, sz, f, k, cap, st);
}
template <typename T>
py::tuple segment_scan(const py::array_t<T, py::array::c_style>& scan, const loam::LidarParams& lidar, const loam::SegmentationParams& params) {
  const size_t n = lidar.scan_lines * lidar.points_per_line;
  if (scan.ndim() != 2 || scan.shape(1) != 3) throw std::runtime_error("scan: expected an (N, 3) array");
  if ((size_t)scan.shape(0) != n) throw std::runtime_error("LOAM: provided lidar scan size does not match provided lidar parameters");
  py::array_t<uint8_t> classes((py::ssize_t)n);
  py::array_t<uint32_t> labels((py::ssize_t)n), sizes((py::ssize_t)n), stats((py::ssize_t)8);
  py::array_t<T> filtered(std::vector<py::ssize_t>{(py::ssize_t)n, 3});
  std::vector<loamx_segment_cluster> recs(n);
  const loamx_lidar_params lp = loam::gpu::toC(lidar);
  const loamx_segment_params sp = loam::gpu::toC(params);
  loamx_ctx* ctx = loam::gpu::defaultContext();
  {
    py::gil_scoped_release release;
    loam::gpu::check(ctx, c_segment(ctx, scan.data(), &lp, &sp, classes.mutable_data(), labels.mutable_data(), sizes.mutable_data(),
                                    filtered.mutable_data(), recs.data(), n, stats.mutable_data()));
  }
  const size_t written = stats.data()[7];
  py::array_t<uint32_t> clusters(std::vector<py::ssize_t>{(py::ssize_t)written, 4});
  if (written) std::memcpy(clusters.mutable_data(), recs.data(), written * sizeof(loamx_segment_cluster));
  return py::make_tuple(classes, labels, sizes, filtered, clusters, stats);
}

loam::Vector3d vec_from(const Arr& a) {
  if (a.size() != 3) throw std::runtime_error("expected a 3-vector");
  return loam::Vector3d(a.data()[0], a.data()[1], a.data()[2]);
}
Arr vec_to(const loam::Vector3d& v) {
  Arr out(3);
  for (int i = 0; i < 3; i++) out.mutable_data()[i] = v(i);
  return out;
}

void scan_size_check(size_t n, const loam::LidarParams& lp) {
  if (n != lp.scan_lines * lp.points_per_line) {
    std::stringstream msg;
    msg << "LOAM: provided lidar scan size ( " << n << ")  does not match provided lidar parameters (" << lp.scan_lines
        << " x " << lp.points_per_line << ")";
    throw std::runtime_error(msg.str());
  }
}

template <typename A>
PyFeatures extract_features(const A& scan, const loam::LidarParams& lp, const loam::FeatureExtractionParams& params) {
  const size_t n = check_points(scan, "input_scan");
  scan_size_check(n, lp);
  PyFeatures out;
  if (n == 0) return out;
  loamx_ctx* ctx = loam::gpu::defaultContext();
  const loamx_lidar_params clp = loam::gpu::toC(lp);
  const loamx_fe_params cfp = loam::gpu::toC(params);
  std::vector<uint32_t> e(loamx_edge_capacity(&clp, &cfp) + 1), p(loamx_planar_capacity(&clp, &cfp) + 1);
  size_t ne = 0, np = 0;
  {
    py::gil_scoped_release release;
    loam::gpu::check(ctx, c_extract(ctx, scan.data(), n, &clp, &cfp, e.data(), e.size(), &ne, p.data(), p.size(), &np));
  }
  out.edge_points = gather_points(scan, e, ne);
  out.planar_points = gather_points(scan, p, np);
  return out;
}

template <typename A>
Arr compute_curvature(const A& scan, const loam::LidarParams& lp, const loam::FeatureExtractionParams& params) {
  const size_t n = check_points(scan, "input_scan");
  scan_size_check(n, lp);
  Arr out((py::ssize_t)n);
  if (n == 0) return out;
  loamx_ctx* ctx = loam::gpu::defaultContext();
  const loamx_lidar_params clp = loam::gpu::toC(lp);
  const loamx_fe_params cfp = loam::gpu::toC(params);
  loam::gpu::check(ctx, c_curvature(ctx, scan.data(), n, &clp, &cfp, out.mutable_data()));
  return out;
}

template <typename A>
py::array_t<bool> compute_valid_points(const A& scan, const loam::LidarParams& lp, const loam::FeatureExtractionParams& params) {
  const size_t n = check_points(scan, "input_scan");
  scan_size_check(n, lp);
  py::array_t<bool> out((py::ssize_t)n);
  if (n == 0) return out;
  loamx_ctx* ctx = loam::gpu::defaultContext();
  const loamx_lidar_params clp = loam::gpu::toC(lp);
  const loamx_fe_params cfp = loam::gpu::toC(params);
  static_assert(sizeof(bool) == 1, "bool must be one byte");
  loam::gpu::check(ctx, c_valid(ctx, scan.data(), n, &clp, &cfp, reinterpret_cast<uint8_t*>(out.mutable_data())));
  return out;
}

// Extension: n consecutive scans as one (n, N, 3) array (or anything numpy stacks into one) -> the n - 1 poses
// target_T_source of the consecutive pairs, every scan extracted once (loamx_register_scan_sequence)
template <typename A>
std::vector<loam::Pose3d> register_scan_sequence(const A& scans, const loam::LidarParams& lp, const loam::FeatureExtractionParams& fe,
                                                 const loam::RegistrationParams& rp, const std::optional<std::vector<loam::Pose3d>>& inits) {
  if (scans.ndim() != 3 || scans.shape(2) != 3) throw std::runtime_error("scans: expected an (n_scans, N, 3) array");
  const size_t n_scans = (size_t)scans.shape(0);
  scan_size_check((size_t)scans.shape(1), lp);
  const size_t n_pairs = n_scans < 2 ? 0 : n_scans - 1;
  if (inits && inits->size() != n_pairs) throw std::runtime_error("inits: expected one pose per consecutive pair (n_scans - 1)");
  std::vector<loam::Pose3d> out;
  if (n_pairs == 0) return out;
  std::vector<double> init;
  if (inits) {
    init.resize(7 * n_pairs);
    for (size_t i = 0; i < n_pairs; i++) (*inits)[i].toArray(&init[7 * i]);
  }
  loamx_ctx* ctx = loam::gpu::defaultContext();
  const loamx_lidar_params clp = loam::gpu::toC(lp);
  const loamx_fe_params cfp = loam::gpu::toC(fe);
  const loamx_reg_params crp = loam::gpu::toC(rp);
  std::vector<loamx_reg_result> res(n_pairs);
  {
    py::gil_scoped_release release;
    loam::gpu::check(ctx, c_sequence(ctx, scans.data(), n_scans, &clp, &cfp, &crp, inits ? init.data() : nullptr, res.data()));
  }
  for (const loamx_reg_result& r : res) out.push_back(loam::Pose3d::fromArray(r.pose));
  return out;
}

// Extension: motion correction of one scan (loamx_deskew_scans_dev); motion = start_T_end of the sweep
template <typename A>
A deskew_scan(const A& scan, const loam::LidarParams& lp, const loam::Pose3d& motion, double ref_fraction) {
  using T = typename A::value_type;
  const size_t n = check_points(scan, "scan");
  scan_size_check(n, lp);
  A out(std::vector<py::ssize_t>{(py::ssize_t)n, 3});
  if (n == 0) return out;
  loamx_ctx* ctx = loam::gpu::defaultContext();
  const loamx_lidar_params clp = loam::gpu::toC(lp);
  double m[7];
  motion.toArray(m);
  void *d_xyz = nullptr, *d_m = nullptr;
  const size_t bytes = n * 3 * sizeof(T);
  loam::gpu::check(ctx, loamx_dev_alloc(ctx, bytes, &d_xyz));
  int rc = loamx_dev_alloc(ctx, sizeof(m), &d_m);
  if (rc == LOAMX_OK) rc = loamx_copy_to_device(ctx, d_xyz, scan.data(), bytes);
  if (rc == LOAMX_OK) rc = loamx_copy_to_device(ctx, d_m, m, sizeof(m));
  if (rc == LOAMX_OK) rc = c_deskew(ctx, static_cast<const T*>(d_xyz), &clp, static_cast<const double*>(d_m), ref_fraction, static_cast<T*>(d_xyz));
  if (rc == LOAMX_OK) rc = loamx_copy_to_host(ctx, out.mutable_data(), d_xyz, bytes);  // (on the context's stream, behind the kernel; synchronous)
  std::string err = rc == LOAMX_OK ? std::string() : std::string(loamx_last_error(ctx));
  loamx_dev_free(ctx, d_xyz);
  if (d_m) loamx_dev_free(ctx, d_m);
  if (rc != LOAMX_OK) throw std::runtime_error(!err.empty() ? err : std::string(loamx_status_string(rc)));
  return out;
}

// (N,3) arrays as feature sets of row views, without copying the coordinates twice
struct Row {
  const double* p;
  double operator()(int i) const { return p[i]; }
};
std::vector<Row> to_rows(const Arr& a, const char* what) {
  const size_t n = check_points(a, what);
  std::vector<Row> r(n);
  for (size_t i = 0; i < n; i++) r[i] = Row{a.data() + 3 * i};
  return r;
}
loam::LoamFeatures<Row> to_features(const PyFeatures& f, const char* edge_name, const char* planar_name) {
  loam::LoamFeatures<Row> out;
  out.edge_points = to_rows(f.edge_points, edge_name);
  out.planar_points = to_rows(f.planar_points, planar_name);
  return out;
}
Arr rows_to_array(const std::vector<double>& xyz) {
  Arr out(std::vector<py::ssize_t>{(py::ssize_t)(xyz.size() / 3), 3});
  if (!xyz.empty()) std::memcpy(out.mutable_data(), xyz.data(), xyz.size() * sizeof(double));
  return out;
}
// rows x cols doubles as a new array (cols == 1: a vector of `rows` entries)
Arr matrix_to_array(const double* v, size_t rows, size_t cols) {
  Arr out(cols == 1 ? std::vector<py::ssize_t>{(py::ssize_t)rows} : std::vector<py::ssize_t>{(py::ssize_t)rows, (py::ssize_t)cols});
  if (rows * cols) std::memcpy(out.mutable_data(), v, rows * cols * sizeof(double));
  return out;
}

}  // namespace

PYBIND11_MODULE(loam_python, m) {
  m.doc() = "loam (MI355X back end): LOAM feature extraction and registration";

  py::class_<loam::LidarParams>(m, "LidarParams")
      .def(py::init<size_t, size_t, double, double>(), py::arg("scan_lines"), py::arg("points_per_line"),
           py::arg("min_range"), py::arg("max_range"))
      .def_readonly("scan_lines", &loam::LidarParams::scan_lines)
      .def_readonly("points_per_line", &loam::LidarParams::points_per_line)
      .def_readonly("min_range", &loam::LidarParams::min_range)
      .def_readonly("max_range", &loam::LidarParams::max_range);

  py::class_<loam::Quaterniond>(m, "Quaterniond")
      .def(py::init<double, double, double, double>(), py::arg("w"), py::arg("x"), py::arg("y"), py::arg("z"))
      .def("w", [](const loam::Quaterniond& q) { return q.w(); })
      .def("x", [](const loam::Quaterniond& q) { return q.x(); })
      .def("y", [](const loam::Quaterniond& q) { return q.y(); })
      .def("z", [](const loam::Quaterniond& q) { return q.z(); });

  py::class_<loam::Pose3d>(m, "Pose3d")
      .def(py::init([](const loam::Quaterniond& q, const Arr& t) { return loam::Pose3d(q, vec_from(t)); }),
           py::arg("rotation"), py::arg("translation"))
      .def_static("Identity", &loam::Pose3d::Identity)
      .def("inverse", &loam::Pose3d::inverse)
      .def("compose", &loam::Pose3d::compose, py::arg("other"))
      .def("act", [](const loam::Pose3d& p, const Arr& pt) { return vec_to(p.act(vec_from(pt))); }, py::arg("point"))
      .def("matrix",
           [](const loam::Pose3d& p) {
             const loam::Matrix4d mm = p.matrix();
             Arr out(std::vector<py::ssize_t>{4, 4});
             for (int i = 0; i < 4; i++)
               for (int j = 0; j < 4; j++) out.mutable_at(i, j) = mm(i, j);
             return out;
           })
      .def_readwrite("rotation", &loam::Pose3d::rotation)
      .def_property(
          "translation", [](const loam::Pose3d& p) { return vec_to(p.translation); },
          [](loam::Pose3d& p, const Arr& t) { p.translation = vec_from(t); });

  py::class_<loam::FeatureExtractionParams>(m, "FeatureExtractionParams")
      .def(py::init<>())
      .def_readwrite("neighbor_points", &loam::FeatureExtractionParams::neighbor_points)
      .def_readwrite("number_sectors", &loam::FeatureExtractionParams::number_sectors)
      .def_readwrite("max_edge_feats_per_sector", &loam::FeatureExtractionParams::max_edge_feats_per_sector)
      .def_readwrite("max_planar_feats_per_sector", &loam::FeatureExtractionParams::max_planar_feats_per_sector)
      .def_readwrite("edge_feat_threshold", &loam::FeatureExtractionParams::edge_feat_threshold)
      .def_readwrite("planar_feat_threshold", &loam::FeatureExtractionParams::planar_feat_threshold)
      .def_readwrite("occlusion_thresh", &loam::FeatureExtractionParams::occlusion_thresh)
      .def_readwrite("parallel_thresh", &loam::FeatureExtractionParams::parallel_thresh);

  py::class_<PyFeatures>(m, "LoamFeatures")
      .def(py::init<>())
      .def_readwrite("edge_points", &PyFeatures::edge_points)
      .def_readwrite("planar_points", &PyFeatures::planar_points);

  m.def("extractFeatures", &extract_features<ArrF>, py::arg("input_scan"), py::arg("lidar_params"),
        py::arg("params") = loam::FeatureExtractionParams());
  m.def("extractFeatures", &extract_features<Arr>, py::arg("input_scan"), py::arg("lidar_params"),
        py::arg("params") = loam::FeatureExtractionParams());
  m.def("computeCurvature", &compute_curvature<ArrF>, py::arg("input_scan"), py::arg("lidar_params"),
        py::arg("params") = loam::FeatureExtractionParams());
  m.def("computeCurvature", &compute_curvature<Arr>, py::arg("input_scan"), py::arg("lidar_params"),
        py::arg("params") = loam::FeatureExtractionParams());
  m.def("computeValidPoints", &compute_valid_points<ArrF>, py::arg("input_scan"), py::arg("lidar_params"),
        py::arg("params") = loam::FeatureExtractionParams());
  m.def("computeValidPoints", &compute_valid_points<Arr>, py::arg("input_scan"), py::arg("lidar_params"),
        py::arg("params") = loam::FeatureExtractionParams());

  py::class_<loam::RegistrationParams>(m, "RegistrationParams")
      .def(py::init<>())
      .def_readwrite("num_edge_neighbors", &loam::RegistrationParams::num_edge_neighbors)
      .def_readwrite("max_edge_neighbor_dist", &loam::RegistrationParams::max_edge_neighbor_dist)
      .def_readwrite("min_line_fit_points", &loam::RegistrationParams::min_line_fit_points)
      .def_readwrite("min_line_condition_number", &loam::RegistrationParams::min_line_condition_number)
      .def_readwrite("num_plane_neighbors", &loam::RegistrationParams::num_plane_neighbors)
      .def_readwrite("max_plane_neighbor_dist", &loam::RegistrationParams::max_plane_neighbor_dist)
      .def_readwrite("min_plane_fit_points", &loam::RegistrationParams::min_plane_fit_points)
      .def_readwrite("max_avg_point_plane_dist", &loam::RegistrationParams::max_avg_point_plane_dist)
      .def_readwrite("max_iterations", &loam::RegistrationParams::max_iterations)
      .def_readwrite("rotation_convergence_thresh", &loam::RegistrationParams::rotation_convergence_thresh)
      .def_readwrite("position_convergence_thresh", &loam::RegistrationParams::position_convergence_thresh)
      .def_readwrite("min_associations", &loam::RegistrationParams::min_associations);

  py::class_<loam::RegistrationDetail::IterationInfo>(m, "RegistrationIterationInfo")
      .def(py::init<const loam::Pose3d, const std::vector<std::pair<size_t, size_t>>,
                    const std::vector<std::pair<size_t, size_t>>, const loam::Pose3d>(),
           py::arg("target_T_source_init"), py::arg("edge_associations"), py::arg("plane_associations"),
           py::arg("estimate_update"))
      .def_readwrite("target_T_source_init", &loam::RegistrationDetail::IterationInfo::target_T_source_init)
      .def_readwrite("edge_associations", &loam::RegistrationDetail::IterationInfo::edge_associations)
      .def_readwrite("plane_associations", &loam::RegistrationDetail::IterationInfo::plane_associations)
      .def_readwrite("estimate_update", &loam::RegistrationDetail::IterationInfo::estimate_update);

  py::enum_<loam::RegistrationDetail::TerminationType>(m, "RegistrationTerminationType")
      .value("CONVERGED", loam::RegistrationDetail::TerminationType::CONVERGED)
      .value("MAX_ITER", loam::RegistrationDetail::TerminationType::MAX_ITER)
      .value("INSUFFICIENT_ASSOCIATIONS", loam::RegistrationDetail::TerminationType::INSUFFICIENT_ASSOCIATIONS)
      .export_values();

  py::class_<loam::RegistrationDetail, std::shared_ptr<loam::RegistrationDetail>>(m, "RegistrationDetail")
      .def(py::init<>())
      .def_readwrite("iteration_info", &loam::RegistrationDetail::iteration_info)
      .def_readwrite("termination_type", &loam::RegistrationDetail::termination_type);

  m.def(
      "registerFeatures",
      [](const PyFeatures& source, const PyFeatures& target, const loam::Pose3d& init,
         const loam::RegistrationParams& params, std::shared_ptr<loam::RegistrationDetail> detail) {
        const loam::LoamFeatures<Row> s = to_features(source, "source.edge_points", "source.planar_points");
        const loam::LoamFeatures<Row> t = to_features(target, "target.edge_points", "target.planar_points");
        py::gil_scoped_release release;
        return loam::registerFeatures<loam::ParenAccessor>(s, t, init, params, detail);
      },
      py::arg("source"), py::arg("target"), py::arg("target_T_source_init"),
      py::arg("params") = loam::RegistrationParams(), py::arg("detail") = std::shared_ptr<loam::RegistrationDetail>());

  // ---- extensions (no counterpart in the reference's module) ----
  // scan-to-map: a target (local map) whose index stays on the device and is kept up there
  py::class_<loam::TargetIndex>(m, "TargetIndex")
      .def(py::init([](const PyFeatures& features, const loam::RegistrationParams& params) {
             const loam::LoamFeatures<Row> f = to_features(features, "features.edge_points", "features.planar_points");
             py::gil_scoped_release release;
             return loam::TargetIndex::build<loam::ParenAccessor>(f, params);
           }),
           py::arg("features"), py::arg("params") = loam::RegistrationParams())
      .def(
          "insert",
          [](loam::TargetIndex& t, const PyFeatures& features) {
            const loam::LoamFeatures<Row> f = to_features(features, "features.edge_points", "features.planar_points");
            py::gil_scoped_release release;
            t.insert<loam::ParenAccessor>(f);
          },
          py::arg("features"))
      .def(
          "insertFiltered",
          [](loam::TargetIndex& t, const PyFeatures& features, const loam::Pose3d& world_T_scan, double edge_leaf, double planar_leaf) {
            const loam::LoamFeatures<Row> f = to_features(features, "features.edge_points", "features.planar_points");
            py::gil_scoped_release release;
            return t.insertFiltered<loam::ParenAccessor>(f, world_T_scan, edge_leaf, planar_leaf);
          },
          py::arg("features"), py::arg("world_T_scan") = loam::Pose3d::Identity(), py::arg("edge_leaf") = 0.2, py::arg("planar_leaf") = 0.4)
      .def(
          "crop", [](loam::TargetIndex& t, const Arr& lo, const Arr& hi) { return t.crop(vec_from(lo), vec_from(hi)); }, py::arg("lo"),
          py::arg("hi"))
      .def("edgePoints", [](const loam::TargetIndex& t) { return rows_to_array(t.edgePointRows()); })
      .def("planarPoints", [](const loam::TargetIndex& t) { return rows_to_array(t.planarPointRows()); })
      .def("numEdgePoints", &loam::TargetIndex::numEdgePoints)
      .def("numPlanarPoints", &loam::TargetIndex::numPlanarPoints);
  m.def(
      "registerFeatures",
      [](const PyFeatures& source, const loam::TargetIndex& target, const loam::Pose3d& init, const loam::RegistrationParams& params,
         std::shared_ptr<loam::RegistrationDetail> detail) {
        const loam::LoamFeatures<Row> s = to_features(source, "source.edge_points", "source.planar_points");
        py::gil_scoped_release release;
        return loam::registerFeatures<loam::ParenAccessor>(s, target, init, params, detail);
      },
      py::arg("source"), py::arg("target_index"), py::arg("target_T_source_init"), py::arg("params") = loam::RegistrationParams(),
      py::arg("detail") = std::shared_ptr<loam::RegistrationDetail>());
  // the information matrix of a pair's residuals at a pose (include/loamx.h: loamx_reg_information)
  py::class_<loam::RegistrationInformation>(m, "RegistrationInformation")
      .def_property_readonly("information", [](const loam::RegistrationInformation& r) { return matrix_to_array(r.information, 6, 6); })
      .def_property_readonly("eigenvalues", [](const loam::RegistrationInformation& r) { return matrix_to_array(r.eigenvalues, 6, 1); })
      .def_property_readonly("eigenvectors", [](const loam::RegistrationInformation& r) { return matrix_to_array(r.eigenvectors, 6, 6); })
      .def_property_readonly("gradient", [](const loam::RegistrationInformation& r) { return matrix_to_array(r.gradient, 6, 1); })
      .def_readonly("weighted_sq_error", &loam::RegistrationInformation::weighted_sq_error)
      .def_readonly("n_edge", &loam::RegistrationInformation::n_edge)
      .def_readonly("n_plane", &loam::RegistrationInformation::n_plane)
      .def_readonly("n_huber", &loam::RegistrationInformation::n_huber)
      .def_readonly("n_dropped", &loam::RegistrationInformation::n_dropped)
      .def(
          "covariance",
          [](const loam::RegistrationInformation& r, double rel_threshold) {
            if (r.n_edge + r.n_plane <= 6) throw py::value_error("covariance: not more than 6 residual rows");
            return matrix_to_array(r.covariance(rel_threshold).data(), 6, 6);
          },
          py::arg("rel_threshold") = 1e-12)
      .def(
          "degenerateDirections",
          [](const loam::RegistrationInformation& r, double min_eigenvalue) {
            std::vector<double> flat;
            for (const std::vector<double>& v : r.degenerateDirections(min_eigenvalue)) flat.insert(flat.end(), v.begin(), v.end());
            return matrix_to_array(flat.data(), flat.size() / 6, 6);
          },
          py::arg("min_eigenvalue"));
  m.def(
      "registrationInformation",
      [](const PyFeatures& source, const PyFeatures& target, const loam::Pose3d& pose, const loam::RegistrationParams& params) {
        const loam::LoamFeatures<Row> s = to_features(source, "source.edge_points", "source.planar_points");
        const loam::LoamFeatures<Row> t = to_features(target, "target.edge_points", "target.planar_points");
        py::gil_scoped_release release;
        return loam::registrationInformation<loam::ParenAccessor>(s, t, pose, params);
      },
      py::arg("source"), py::arg("target"), py::arg("target_T_source"), py::arg("params") = loam::RegistrationParams());
  m.def(
      "registrationInformation",
      [](const PyFeatures& source, const loam::TargetIndex& target, const loam::Pose3d& pose, const loam::RegistrationParams& params) {
        const loam::LoamFeatures<Row> s = to_features(source, "source.edge_points", "source.planar_points");
        py::gil_scoped_release release;
        return loam::registrationInformation<loam::ParenAccessor>(s, target, pose, params);
      },
      py::arg("source"), py::arg("target_index"), py::arg("target_T_source"), py::arg("params") = loam::RegistrationParams());
  // unordered clouds into organised scans (include/loamx.h: "unordered clouds into scans"): extensions like TargetIndex
  py::enum_<loam::OrganizeKeep>(m, "OrganizeKeep").value("First", loam::OrganizeKeep::First).value("Nearest", loam::OrganizeKeep::Nearest);
  py::class_<loam::OrganizeParams>(m, "OrganizeParams")
      .def(py::init<>())
      .def_readwrite("azimuth_zero", &loam::OrganizeParams::azimuth_zero)
      .def_readwrite("clockwise", &loam::OrganizeParams::clockwise)
      .def_readwrite("keep", &loam::OrganizeParams::keep)
      .def_readwrite("elevations", &loam::OrganizeParams::elevations)
      .def_readwrite("fov_bottom", &loam::OrganizeParams::fov_bottom)
      .def_readwrite("fov_top", &loam::OrganizeParams::fov_top)
      .def_readwrite("ring_map", &loam::OrganizeParams::ring_map);
  py::class_<loam::ScanLayout>(m, "ScanLayout")
      .def(py::init<const loam::LidarParams&, const loam::OrganizeParams&>(), py::arg("lidar_params"), py::arg("params") = loam::OrganizeParams())
      .def_property_readonly("scan_lines", &loam::ScanLayout::scanLines)
      .def_property_readonly("points_per_line", &loam::ScanLayout::pointsPerLine)
      .def("columnDirections", [](const loam::ScanLayout& l) { return matrix_to_array(l.columnDirections().data(), l.pointsPerLine(), 2); })
      .def("lineTangents", [](const loam::ScanLayout& l) { return matrix_to_array(l.lineTangents().data(), l.scanLines() + 1, 1); });
  m.def("organizeCloud", &organize_cloud<float>, py::arg("points"), py::arg("layout"), py::arg("rings") = py::none());
  m.def("organizeCloud", &organize_cloud<double>, py::arg("points"), py::arg("layout"), py::arg("rings") = py::none());
  // scan segmentation (include/loamx.h: "scan segmentation"): an extension of the reference's surface like organizeCloud
  py::class_<loam::SegmentationParams>(m, "SegmentationParams")
      .def(py::init<>())
      .def_readwrite("ground_lines", &loam::SegmentationParams::ground_lines)
      .def_readwrite("ground_angle", &loam::SegmentationParams::ground_angle)
      .def_readwrite("segment_angle", &loam::SegmentationParams::segment_angle)
      .def_readwrite("min_cluster_points", &loam::SegmentationParams::min_cluster_points)
      .def_readwrite("min_tall_cluster_points", &loam::SegmentationParams::min_tall_cluster_points)
      .def_readwrite("min_tall_cluster_lines", &loam::SegmentationParams::min_tall_cluster_lines)
      .def_readwrite("drop_outliers", &loam::SegmentationParams::drop_outliers)
      .def_readwrite("drop_ground", &loam::SegmentationParams::drop_ground);
  m.def("segmentScan", &segment_scan<float>, py::arg("scan"), py::arg("lidar_params"), py::arg("params") = loam::SegmentationParams());
  m.def("segmentScan", &segment_scan<double>, py::arg("scan"), py::arg("lidar_params"), py::arg("params") = loam::SegmentationParams());

  // map cleaning (include/loamx.h: "map cleaning"): an extension of the reference's surface like segmentScan
  py::class_<loam::VisibilityParams>(m, "VisibilityParams")
      .def(py::init<>())
      .def_readwrite("min_range", &loam::VisibilityParams::min_range)
      .def_readwrite("max_range", &loam::VisibilityParams::max_range)
      .def_readwrite("margin", &loam::VisibilityParams::margin)
      .def_readwrite("margin_rel", &loam::VisibilityParams::margin_rel)
      .def_readwrite("window_lines", &loam::VisibilityParams::window_lines)
      .def_readwrite("window_cols", &loam::VisibilityParams::window_cols)
      .def_readwrite("min_through", &loam::VisibilityParams::min_through)
      .def_readwrite("through_ratio", &loam::VisibilityParams::through_ratio);
  m.def("visibilityVotes", &visibility_votes<float>, py::arg("map_points"), py::arg("scans"), py::arg("world_T_scan"), py::arg("layout"),
        py::arg("params") = loam::VisibilityParams());
  m.def("visibilityVotes", &visibility_votes<double>, py::arg("map_points"), py::arg("scans"), py::arg("world_T_scan"), py::arg("layout"),
        py::arg("params") = loam::VisibilityParams());
  m.def("removeDynamicPoints", &remove_dynamic_points, py::arg("map_points"), py::arg("votes"), py::arg("params") = loam::VisibilityParams());
  // place recognition (include/loamx.h: "place recognition"): an extension like TargetIndex
  py::class_<loam::PlaceParams>(m, "PlaceParams")
      .def(py::init<>())
      .def_readwrite("n_rings", &loam::PlaceParams::n_rings)
      .def_readwrite("n_sectors", &loam::PlaceParams::n_sectors)
      .def_readwrite("max_range", &loam::PlaceParams::max_range)
      .def_readwrite("z_offset", &loam::PlaceParams::z_offset)
      .def_readwrite("z_scale", &loam::PlaceParams::z_scale);
  py::class_<loam::PlaceMatch>(m, "PlaceMatch")
      .def_readonly("id", &loam::PlaceMatch::id)
      .def_readonly("shift", &loam::PlaceMatch::shift)
      .def_readonly("key_dist", &loam::PlaceMatch::key_dist)
      .def_readonly("distance", &loam::PlaceMatch::distance)
      .def_property_readonly("valid", &loam::PlaceMatch::valid)
      .def_property_readonly("yaw", &loam::PlaceMatch::yaw)
      .def("initialGuess", &loam::PlaceMatch::initialGuess);
  py::class_<loam::PlaceDatabase>(m, "PlaceDatabase")
      .def(py::init<const loam::PlaceParams&>(), py::arg("params") = loam::PlaceParams())
      .def_property_readonly("params", &loam::PlaceDatabase::params)
      .def("size", &loam::PlaceDatabase::size)
      .def("__len__", &loam::PlaceDatabase::size)
      .def("sectorDirections", [](const loam::PlaceDatabase& d) { return matrix_to_array(d.sectorDirections().data(), d.params().n_sectors, 2); })
      .def("descriptor", &place_descriptor<float>, py::arg("points"))
      .def("descriptor", &place_descriptor<double>, py::arg("points"))
      .def("add", [](loam::PlaceDatabase& d, const ArrDesc& desc) { return d.add(place_desc_arg(d, desc)); }, py::arg("descriptor"))
      .def(
          "search",
          [](const loam::PlaceDatabase& d, const ArrDesc& query, uint32_t num_candidates, std::optional<uint32_t> id_end) {
            return d.search(place_desc_arg(d, query), num_candidates, id_end.value_or(0xFFFFFFFFu));
          },
          py::arg("query"), py::arg("num_candidates"), py::arg("id_end") = py::none());
  // cloud map (include/loamx.h: "cloud map"): an extension like TargetIndex
  py::class_<loam::CloudMapParams>(m, "CloudMapParams")
      .def(py::init<>())
      .def_readwrite("leaf", &loam::CloudMapParams::leaf)
      .def_readwrite("min_range", &loam::CloudMapParams::min_range)
      .def_readwrite("max_range", &loam::CloudMapParams::max_range);
  py::class_<loam::CloudMap>(m, "CloudMap")
      .def(py::init<const loam::CloudMapParams&, size_t>(), py::arg("params") = loam::CloudMapParams(), py::arg("max_voxels") = (size_t)1 << 20)
      .def_property_readonly("params", &loam::CloudMap::params)
      .def_property_readonly("max_voxels", &loam::CloudMap::maxVoxels)
      .def("add", &cloud_map_add<float>, py::arg("points"), py::arg("world_T_sensor") = py::none())
      .def("add", &cloud_map_add<double>, py::arg("points"), py::arg("world_T_sensor") = py::none())
      .def("clear", &loam::CloudMap::clear)
      .def(
          "crop",
          [](loam::CloudMap& map, const std::array<double, 3>& lo, const std::array<double, 3>& hi, const std::array<double, 3>& center) {
            const loam::MapCrop c = map.crop(lo, hi, center);
            return py::make_tuple(c.kept, c.removed);
          },
          py::arg("lo"), py::arg("hi"), py::arg("center") = std::array<double, 3>{0.0, 0.0, 0.0})
      .def(
          "points",
          [](const loam::CloudMap& map, uint32_t min_points) {
            const loam::CloudMapPoints p = map.points(min_points);
            py::array_t<uint32_t> counts((py::ssize_t)p.size()), first((py::ssize_t)p.size());
            if (p.size()) {
              std::memcpy(counts.mutable_data(), p.counts.data(), p.size() * sizeof(uint32_t));
              std::memcpy(first.mutable_data(), p.first.data(), p.size() * sizeof(uint32_t));
            }
            Arr xyz(std::vector<py::ssize_t>{(py::ssize_t)p.size(), 3});
            if (p.size()) std::memcpy(xyz.mutable_data(), p.xyz.data(), p.xyz.size() * sizeof(double));
            return py::make_tuple(xyz, counts, first);
          },
          py::arg("min_points") = 1)
      .def("stats", [](const loam::CloudMap& map) {
        const loam::CloudMapStats s = map.stats();
        py::dict d;
        d["voxels"] = s.voxels, d["points_offered"] = s.points_offered, d["points_used"] = s.points_used, d["invalid"] = s.invalid;
        d["range"] = s.range, d["outside"] = s.outside, d["overflow"] = s.overflow;
        return d;
      });
  // surfel map (include/loamx.h: "surfel map"): an extension like CloudMap
  py::class_<loam::SurfelMapParams>(m, "SurfelMapParams")
      .def(py::init<>())
      .def_readwrite("leaf", &loam::SurfelMapParams::leaf)
      .def_readwrite("min_range", &loam::SurfelMapParams::min_range)
      .def_readwrite("max_range", &loam::SurfelMapParams::max_range);
  py::class_<loam::LocalizeParams>(m, "LocalizeParams")
      .def(py::init<>())
      .def_readwrite("neighborhood", &loam::LocalizeParams::neighborhood)
      .def_readwrite("min_points", &loam::LocalizeParams::min_points)
      .def_readwrite("planarity", &loam::LocalizeParams::planarity)
      .def_readwrite("max_distance", &loam::LocalizeParams::max_distance)
      .def_readwrite("huber_delta", &loam::LocalizeParams::huber_delta)
      .def_readwrite("max_iterations", &loam::LocalizeParams::max_iterations)
      .def_readwrite("min_rows", &loam::LocalizeParams::min_rows)
      .def_readwrite("rotation_convergence_thresh", &loam::LocalizeParams::rotation_convergence_thresh)
      .def_readwrite("position_convergence_thresh", &loam::LocalizeParams::position_convergence_thresh)
      .def_readwrite("min_eigenvalue_per_row", &loam::LocalizeParams::min_eigenvalue_per_row);
  py::class_<loam::LocalizeResult>(m, "LocalizeResult")
      .def_property_readonly("pose", [](const loam::LocalizeResult& r) { return matrix_to_array(r.pose, 7, 1); })
      .def_readonly("initial_cost", &loam::LocalizeResult::initial_cost)
      .def_readonly("final_cost", &loam::LocalizeResult::final_cost)
      .def_readonly("last_rotation", &loam::LocalizeResult::last_rotation)
      .def_readonly("last_translation", &loam::LocalizeResult::last_translation)
      .def_readonly("iterations", &loam::LocalizeResult::iterations)
      .def_readonly("termination", &loam::LocalizeResult::termination)
      .def_readonly("n_rows", &loam::LocalizeResult::n_rows)
      .def_readonly("n_huber", &loam::LocalizeResult::n_huber)
      .def_readonly("n_no_surfel", &loam::LocalizeResult::n_no_surfel)
      .def_readonly("n_gated", &loam::LocalizeResult::n_gated)
      .def_readonly("n_unused", &loam::LocalizeResult::n_unused)
      .def_readonly("used_mask", &loam::LocalizeResult::used_mask)
      .def_readonly("n_rows_initial", &loam::LocalizeResult::n_rows_initial)
      .def("tobytes", [](const loam::LocalizeResult& r) { return py::bytes(reinterpret_cast<const char*>(&r), sizeof(r)); });
  py::class_<loam::SurfelMap>(m, "SurfelMap")
      .def(py::init<const loam::SurfelMapParams&, size_t>(), py::arg("params") = loam::SurfelMapParams(), py::arg("max_voxels") = (size_t)1 << 20)
      .def_property_readonly("params", &loam::SurfelMap::params)
      .def_property_readonly("max_voxels", &loam::SurfelMap::maxVoxels)
      .def("add", &surfel_map_add<float>, py::arg("points"), py::arg("world_T_sensor") = py::none())
      .def("add", &surfel_map_add<double>, py::arg("points"), py::arg("world_T_sensor") = py::none())
      .def("clear", &loam::SurfelMap::clear)
      .def(
          "crop",
          [](loam::SurfelMap& map, const std::array<double, 3>& lo, const std::array<double, 3>& hi, const std::array<double, 3>& center) {
            const loam::MapCrop c = map.crop(lo, hi, center);
            return py::make_tuple(c.kept, c.removed);
          },
          py::arg("lo"), py::arg("hi"), py::arg("center") = std::array<double, 3>{0.0, 0.0, 0.0})
      .def("localize", &surfel_map_localize<float>, py::arg("points"), py::arg("init"), py::arg("params") = loam::LocalizeParams())
      .def("localize", &surfel_map_localize<double>, py::arg("points"), py::arg("init"), py::arg("params") = loam::LocalizeParams())
      .def(
          "surfels", [](const loam::SurfelMap& map, uint32_t min_points) { return surfel_arrays(map.surfels(min_points)); }, py::arg("min_points") = 1)
      .def(
          "query",
          [](const loam::SurfelMap& map, const Arr& points, uint32_t min_points) {
            if (points.ndim() != 2 || points.shape(1) < 3) throw std::runtime_error("points: expected an (N, 3) or (N, 4) array");
            const size_t n = (size_t)points.shape(0), stride = (size_t)points.shape(1);
            std::vector<double> xyz(3 * n);
            for (size_t i = 0; i < n; i++)
              for (size_t a = 0; a < 3; a++) xyz[3 * i + a] = points.data()[i * stride + a];
            const loam::SurfelQuery q = map.query(xyz, min_points);
            py::dict d = surfel_arrays(q.surfels);
            Arr dist((py::ssize_t)n);
            if (n) std::memcpy(dist.mutable_data(), q.distances.data(), n * sizeof(double));
            d["distance"] = dist;
            return d;
          },
          py::arg("points"), py::arg("min_points") = 1)
      .def("stats", [](const loam::SurfelMap& map) {
        const loam::SurfelMapStats s = map.stats();
        py::dict d;
        d["voxels"] = s.voxels, d["points_offered"] = s.points_offered, d["points_used"] = s.points_used, d["invalid"] = s.invalid;
        d["range"] = s.range, d["outside"] = s.outside, d["overflow"] = s.overflow;
        return d;
      });
  // occupancy map (include/loamx.h: "occupancy map"): an extension like CloudMap
  py::class_<loam::OccupancyParams>(m, "OccupancyParams")
      .def(py::init<>())
      .def_readwrite("leaf", &loam::OccupancyParams::leaf)
      .def_readwrite("min_range", &loam::OccupancyParams::min_range)
      .def_readwrite("max_range", &loam::OccupancyParams::max_range)
      .def_readwrite("end_margin", &loam::OccupancyParams::end_margin)
      .def_readwrite("clip_long", &loam::OccupancyParams::clip_long)
      .def_readwrite("min_hits", &loam::OccupancyParams::min_hits)
      .def_readwrite("occ_ratio", &loam::OccupancyParams::occ_ratio)
      .def_readwrite("min_passes", &loam::OccupancyParams::min_passes);
  py::class_<loam::DistanceParams>(m, "DistanceParams")
      .def(py::init<>())
      .def_readwrite("max_dist_voxels", &loam::DistanceParams::max_dist_voxels)
      .def_readwrite("unknown_is_obstacle", &loam::DistanceParams::unknown_is_obstacle);
  py::class_<loam::RaycastParams>(m, "RaycastParams")
      .def(py::init<>())
      .def_readwrite("skip_start", &loam::RaycastParams::skip_start)
      .def_readwrite("unknown_stops", &loam::RaycastParams::unknown_stops)
      .def_readwrite("max_steps", &loam::RaycastParams::max_steps)
      .def_property(
          "hit_at", [](const loam::RaycastParams& p) { return (uint32_t)p.hit_at; },
          [](loam::RaycastParams& p, uint32_t v) { p.hit_at = static_cast<loam::RaycastParams::HitAt>(v); });
  py::class_<loam::OccupancyMap> occupancy_map(m, "OccupancyMap");
  occupancy_map.attr("DIST_FAR") = (int)loam::DistanceField::FAR;
  occupancy_map.attr("RAY_CLEAR") = (int)loam::RayRecord::CLEAR, occupancy_map.attr("RAY_HIT") = (int)loam::RayRecord::HIT;
  occupancy_map.attr("RAY_UNKNOWN") = (int)loam::RayRecord::UNKNOWN, occupancy_map.attr("RAY_TRUNCATED") = (int)loam::RayRecord::TRUNCATED;
  occupancy_map.attr("RAY_OUTSIDE") = (int)loam::RayRecord::OUTSIDE, occupancy_map.attr("RAY_INVALID") = (int)loam::RayRecord::INVALID;
  occupancy_map.attr("RAY_AT_ENTER") = (int)loam::RaycastParams::AT_ENTER, occupancy_map.attr("RAY_AT_MIDDLE") = (int)loam::RaycastParams::AT_MIDDLE;
  occupancy_map.attr("UNKNOWN") = (int)loam::Occupancy::UNKNOWN;
  occupancy_map.attr("FREE") = (int)loam::Occupancy::FREE;
  occupancy_map.attr("OCCUPIED") = (int)loam::Occupancy::OCCUPIED;
  occupancy_map
      .def(py::init<const loam::OccupancyParams&, size_t>(), py::arg("params") = loam::OccupancyParams(), py::arg("max_voxels") = (size_t)1 << 20)
      .def_property_readonly("params", &loam::OccupancyMap::params)
      .def_property_readonly("max_voxels", &loam::OccupancyMap::maxVoxels)
      .def("add", &occupancy_add<float>, py::arg("points"), py::arg("world_T_sensor") = py::none())
      .def("add", &occupancy_add<double>, py::arg("points"), py::arg("world_T_sensor") = py::none())
      .def("clear", &loam::OccupancyMap::clear)
      .def(
          "crop",
          [](loam::OccupancyMap& map, const std::array<double, 3>& lo, const std::array<double, 3>& hi, const std::array<double, 3>& center) {
            const loam::MapCrop c = map.crop(lo, hi, center);
            return py::make_tuple(c.kept, c.removed);
          },
          py::arg("lo"), py::arg("hi"), py::arg("center") = std::array<double, 3>{0.0, 0.0, 0.0})
      .def(
          "query",
          [](const loam::OccupancyMap& map, const Arr& points) {
            if (points.ndim() != 2 || points.shape(1) < 3) throw std::runtime_error("points: expected an (N, 3) or (N, 4) array");
            const py::ssize_t n = points.shape(0);
            py::array_t<uint32_t> counts(std::vector<py::ssize_t>{n, 2});
            py::array_t<uint8_t> states(n);
            loamx_ctx* ctx = loam::gpu::defaultContext();
            loam::gpu::check(ctx, loamx_occupancy_query(ctx, map.handle(), points.data(), (size_t)points.shape(1), (size_t)n, counts.mutable_data(),
                                                        states.mutable_data()));
            return py::make_tuple(counts, states);
          },
          py::arg("points"))
      .def(
          "box",
          [](const loam::OccupancyMap& map, const std::array<int64_t, 3>& vmin, const std::array<int64_t, 3>& dims) {
            std::array<int32_t, 3> v;
            std::array<uint32_t, 3> d;
            occupancy_box_args(vmin, dims, v, d);
            py::array_t<uint32_t> counts(std::vector<py::ssize_t>{(py::ssize_t)d[2], (py::ssize_t)d[1], (py::ssize_t)d[0], 2});
            py::array_t<uint8_t> states(std::vector<py::ssize_t>{(py::ssize_t)d[2], (py::ssize_t)d[1], (py::ssize_t)d[0]});
            loamx_ctx* ctx = loam::gpu::defaultContext();
            loam::gpu::check(ctx, loamx_occupancy_box(ctx, map.handle(), v.data(), d.data(), counts.mutable_data(), states.mutable_data()));
            return py::make_tuple(counts, states);
          },
          py::arg("vmin"), py::arg("dims"))
      .def(
          "slice",
          [](const loam::OccupancyMap& map, const std::array<int64_t, 3>& vmin, const std::array<int64_t, 3>& dims) {
            std::array<int32_t, 3> v;
            std::array<uint32_t, 3> d;
            occupancy_box_args(vmin, dims, v, d);
            py::array_t<uint8_t> grid(std::vector<py::ssize_t>{(py::ssize_t)d[1], (py::ssize_t)d[0]});
            loamx_ctx* ctx = loam::gpu::defaultContext();
            loam::gpu::check(ctx, loamx_occupancy_slice(ctx, map.handle(), v.data(), d.data(), grid.mutable_data()));
            return grid;
          },
          py::arg("vmin"), py::arg("dims"))
      .def(
          "distanceBox",
          [](loam::OccupancyMap& map, const std::array<int64_t, 3>& vmin, const std::array<int64_t, 3>& dims, const loam::DistanceParams& params) {
            return occupancy_distance(map, vmin, dims, params, false);
          },
          py::arg("vmin"), py::arg("dims"), py::arg("params") = loam::DistanceParams())
      .def(
          "distanceSlice",
          [](loam::OccupancyMap& map, const std::array<int64_t, 3>& vmin, const std::array<int64_t, 3>& dims, const loam::DistanceParams& params) {
            return occupancy_distance(map, vmin, dims, params, true);
          },
          py::arg("vmin"), py::arg("dims"), py::arg("params") = loam::DistanceParams())
      .def(
          "castRays",
          [](const loam::OccupancyMap& map, const Arr& origins, const Arr& ends, const loam::RaycastParams& params) {
            if (origins.ndim() != 2 || origins.shape(1) < 3 || ends.ndim() != 2 || ends.shape(0) != origins.shape(0) || ends.shape(1) != origins.shape(1))
              throw std::runtime_error("origins, ends: expected two (N, 3) arrays of the same shape");
            const py::ssize_t n = origins.shape(0);
            py::array records(ray_record_dtype(), std::vector<py::ssize_t>{n});
            const loamx_raycast_params p = raycast_params(params);
            loamx_ctx* ctx = loam::gpu::defaultContext();
            loam::gpu::check(ctx, loamx_occupancy_cast_rays_host(ctx, map.handle(), origins.data(), ends.data(), (size_t)origins.shape(1), (size_t)n, &p,
                                                                 static_cast<loamx_ray_record*>(records.mutable_data())));
            return records;
          },
          py::arg("origins"), py::arg("ends"), py::arg("params") = loam::RaycastParams())
      .def(
          "renderScans",
          [](const loam::OccupancyMap& map, const Arr& dirs, const Arr& poses, double max_range, const loam::RaycastParams& params) {
            if (dirs.ndim() != 2 || dirs.shape(1) != 3) throw std::runtime_error("dirs: expected an (n_beams, 3) array");
            if (poses.ndim() != 2 || poses.shape(1) != 7) throw std::runtime_error("poses: expected an (n_poses, 7) array (qx qy qz qw tx ty tz)");
            const py::ssize_t nb = dirs.shape(0), np_ = poses.shape(0);
            Arr scans(std::vector<py::ssize_t>{np_, nb, 3}), ranges(std::vector<py::ssize_t>{np_, nb});
            py::array records(ray_record_dtype(), std::vector<py::ssize_t>{np_, nb});
            const loamx_raycast_params p = raycast_params(params);
            loamx_ctx* ctx = loam::gpu::defaultContext();
            loam::gpu::check(ctx, loamx_occupancy_render_scans_host(ctx, map.handle(), dirs.data(), (size_t)nb, poses.data(), (size_t)np_, max_range, &p,
                                                                    scans.mutable_data(), ranges.mutable_data(),
                                                                    static_cast<loamx_ray_record*>(records.mutable_data())));
            return py::make_tuple(scans, ranges, records);
          },
          py::arg("dirs"), py::arg("poses"), py::arg("max_range"), py::arg("params") = loam::RaycastParams())
      .def("stats", [](const loam::OccupancyMap& map) {
        const loam::OccupancyStats s = map.stats();
        py::dict d;
        d["rays_offered"] = s.rays_offered, d["rays_hit"] = s.rays_hit, d["invalid"] = s.invalid, d["range_short"] = s.range_short;
        d["range_long"] = s.range_long, d["outside"] = s.outside, d["visits"] = s.visits, d["voxels"] = s.voxels, d["overflow"] = s.overflow;
        return d;
      });
  py::class_<loam::PoseGraphParams>(m, "PoseGraphParams")
      .def(py::init<>())
      .def_readwrite("max_iterations", &loam::PoseGraphParams::max_iterations)
      .def_readwrite("max_pcg_iterations", &loam::PoseGraphParams::max_pcg_iterations)
      .def_readwrite("pcg_tolerance", &loam::PoseGraphParams::pcg_tolerance)
      .def_readwrite("initial_lambda", &loam::PoseGraphParams::initial_lambda)
      .def_readwrite("cost_tolerance", &loam::PoseGraphParams::cost_tolerance)
      .def_readwrite("step_tolerance", &loam::PoseGraphParams::step_tolerance)
      .def_readwrite("huber_delta", &loam::PoseGraphParams::huber_delta);
  py::enum_<loam::PoseGraphSummary::TerminationType>(m, "PoseGraphTerminationType")
      .value("COST_CONVERGED", loam::PoseGraphSummary::TerminationType::COST_CONVERGED)
      .value("STEP_CONVERGED", loam::PoseGraphSummary::TerminationType::STEP_CONVERGED)
      .value("MAX_ITERATIONS", loam::PoseGraphSummary::TerminationType::MAX_ITERATIONS)
      .value("LAMBDA_OVERFLOW", loam::PoseGraphSummary::TerminationType::LAMBDA_OVERFLOW)
      .value("NOTHING_TO_DO", loam::PoseGraphSummary::TerminationType::NOTHING_TO_DO)
      .value("BAD_INPUT", loam::PoseGraphSummary::TerminationType::BAD_INPUT);
  py::class_<loam::PoseGraphSummary>(m, "PoseGraphSummary")
      .def_readonly("initial_cost", &loam::PoseGraphSummary::initial_cost)
      .def_readonly("final_cost", &loam::PoseGraphSummary::final_cost)
      .def_readonly("lambda_", &loam::PoseGraphSummary::lambda)
      .def_readonly("max_update", &loam::PoseGraphSummary::max_update)
      .def_readonly("iterations", &loam::PoseGraphSummary::iterations)
      .def_readonly("accepted", &loam::PoseGraphSummary::accepted)
      .def_readonly("pcg_iterations", &loam::PoseGraphSummary::pcg_iterations)
      .def_readonly("termination_type", &loam::PoseGraphSummary::termination_type)
      .def_readonly("n_bad_edges", &loam::PoseGraphSummary::n_bad_edges);
  py::class_<loam::PoseGraph>(m, "PoseGraph")
      .def(py::init<const loam::PoseGraphParams&>(), py::arg("params") = loam::PoseGraphParams())
      .def_property("params", [](const loam::PoseGraph& g) { return g.params(); },
                    [](loam::PoseGraph& g, const loam::PoseGraphParams& p) { g.params() = p; })
      .def("addPose", &loam::PoseGraph::addPose, py::arg("world_T_pose"))
      .def("setFixed", &loam::PoseGraph::setFixed, py::arg("id"), py::arg("fixed") = true)
      .def(
          "addEdge",
          [](loam::PoseGraph& g, size_t a, size_t b, const loam::Pose3d& a_T_b, const loam::RegistrationInformation& info) {
            g.addEdge(a, b, a_T_b, info);
          },
          py::arg("a"), py::arg("b"), py::arg("a_T_b"), py::arg("information"))
      .def(
          "addEdge",
          [](loam::PoseGraph& g, size_t a, size_t b, const loam::Pose3d& a_T_b, const Arr& info) {
            if (info.size() != 36) throw std::runtime_error("loam.PoseGraph.addEdge: the information matrix holds 6 x 6 entries");
            g.addEdge(a, b, a_T_b, info.data());
          },
          py::arg("a"), py::arg("b"), py::arg("a_T_b"), py::arg("information"))
      .def("numPoses", &loam::PoseGraph::numPoses)
      .def("numEdges", &loam::PoseGraph::numEdges)
      .def("pose", &loam::PoseGraph::pose, py::arg("id"))
      .def("fixed", &loam::PoseGraph::fixed, py::arg("id"))
      .def("optimize", &loam::PoseGraph::optimize);
  m.def("registerScanSequence", &register_scan_sequence<ArrF>, py::arg("scans"), py::arg("lidar_params"),
        py::arg("fe_params") = loam::FeatureExtractionParams(), py::arg("reg_params") = loam::RegistrationParams(),
        py::arg("inits") = py::none());
  m.def("registerScanSequence", &register_scan_sequence<Arr>, py::arg("scans"), py::arg("lidar_params"),
        py::arg("fe_params") = loam::FeatureExtractionParams(), py::arg("reg_params") = loam::RegistrationParams(),
        py::arg("inits") = py::none());
  m.def("deskewScan", &deskew_scan<ArrF>, py::arg("scan"), py::arg("lidar_params"), py::arg("motion"), py::arg("ref_fraction") = 1.0);
  m.def("deskewScan", &deskew_scan<Arr>, py::arg("scan"), py::arg("lidar_params"), py::arg("motion"), py::arg("ref_fraction") = 1.0);
}
