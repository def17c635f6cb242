// registration_pipeline.hpp — header-only, ROS-free C++ restatement of the scan-to-map sequence that calls the solver.
//
// SURVEY.md §8(f)-1.  Mirrors OdometryPipeline::ICP_processing of the reference for the `estimator == ICP`
// configuration (/root/reference/svn-icp/src/core/OdometryPipeline.cpp:556-647): crop (:692-704) -> uniform
// down-sample, map cloud at 0.5·voxel and solver cloud at 1.5·voxel of that (:559-560, :684-690) -> constant-twist pose
// prediction (:706-737) -> particle prior (:661-667) -> local-map range query (:577-581, VoxelHashMap.cpp:48-58) ->
// solver (svnicp_hip_shim.hpp, :582-607) -> pose = prediction · correction (updater_, :37-46) -> map insert (:627,
// VoxelHashMap.cpp:22-42).  The reference does this with PCL / GTSAM / tsl::robin_map on the host; none of them exists
// in this image, so the few operations needed are written out here (float32 points like pcl::PointXYZ, float64 poses).
// The Python module svn-icp_amd/pipeline.py is the same sequence and serves as the cross-check in the tests.
// With PipelineConfig::deskew the scan is first motion-compensated as OdometryPipeline::deskew_pointcloud does (:357-447,
// run when the pose buffer holds two poses, :551-554); see deskew_pointcloud below.
// With PipelineConfig::segmentation the raw scan is first range-image segmented as ImageProjection::cloudHandler does
// (USE_Segmentation, :328-355); see segment_scan below.
//
// Where PCL / the hash map leave an order unspecified (iteration order of occupied leaves / voxels) this code emits
// ascending leaf / voxel index; the solver's result does not depend on the order of the target points except through
// exact ties.  Parity of the solver call itself is pinned by the tests against the CPU oracle on the very inputs this
// class hands to the solver (`Tap`).
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <functional>
#include <limits>
#include <map>
#include <memory>
#include <numeric>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "svnicp_hip_shim.hpp"

namespace svnicp {

// ------------------------------------------------------------------------------------------------ SE(3), gtsam::Pose3 semantics
struct Pose3 {
  std::array<double, 9> R{1, 0, 0, 0, 1, 0, 0, 0, 1};  // row-major
  std::array<double, 3> t{0, 0, 0};

  Pose3 operator*(const Pose3& o) const {
    Pose3 r;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) r.R[3 * i + j] = R[3 * i] * o.R[j] + R[3 * i + 1] * o.R[3 + j] + R[3 * i + 2] * o.R[6 + j];
      r.t[i] = R[3 * i] * o.t[0] + R[3 * i + 1] * o.t[1] + R[3 * i + 2] * o.t[2] + t[i];
    }
    return r;
  }
  Pose3 inverse() const {
    Pose3 r;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) r.R[3 * i + j] = R[3 * j + i];
    for (int i = 0; i < 3; ++i) r.t[i] = -(r.R[3 * i] * t[0] + r.R[3 * i + 1] * t[1] + r.R[3 * i + 2] * t[2]);
    return r;
  }
};

namespace detail {
inline std::array<double, 9> hat(const double w[3]) { return {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0}; }
inline std::array<double, 9> mul3(const std::array<double, 9>& a, const std::array<double, 9>& b) {
  std::array<double, 9> c{};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
  return c;
}
inline std::array<double, 9> lin3(double a, double b, const std::array<double, 9>& K, double c, const std::array<double, 9>& K2) {
  std::array<double, 9> r{};
  for (int i = 0; i < 9; ++i) r[i] = b * K[i] + c * K2[i];
  r[0] += a; r[4] += a; r[8] += a;
  return r;
}
}  // namespace detail

inline std::array<double, 9> so3_exp(const double w[3]) {  // Rot3::Expmap
  const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const auto K = detail::hat(w);
  const auto K2 = detail::mul3(K, K);
  if (th < 1e-10) return detail::lin3(1.0, 1.0, K, 0.5, K2);
  return detail::lin3(1.0, std::sin(th) / th, K, (1.0 - std::cos(th)) / (th * th), K2);
}
inline std::array<double, 3> so3_log(const std::array<double, 9>& R) {  // Rot3::Logmap
  const double c = std::max(-1.0, std::min(1.0, 0.5 * (R[0] + R[4] + R[8] - 1.0)));
  const double th = std::acos(c);
  const double v[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  const double f = th < 1e-10 ? 0.5 : th / (2.0 * std::sin(th));
  return {f * v[0], f * v[1], f * v[2]};
}
inline Pose3 se3_exp(const double xi[6]) {  // Pose3::Expmap, xi = [omega, v]
  const double* w = xi;
  const double* v = xi + 3;
  const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const auto K = detail::hat(w);
  const auto K2 = detail::mul3(K, K);
  const auto V = th < 1e-10 ? detail::lin3(1.0, 0.5, K, 0.0, K2)
                            : detail::lin3(1.0, (1.0 - std::cos(th)) / (th * th), K, (th - std::sin(th)) / (th * th * th), K2);
  Pose3 T;
  T.R = so3_exp(w);
  for (int i = 0; i < 3; ++i) T.t[i] = V[3 * i] * v[0] + V[3 * i + 1] * v[1] + V[3 * i + 2] * v[2];
  return T;
}
inline std::array<double, 6> se3_log(const Pose3& T) {  // Pose3::Logmap -> [omega, v]
  const auto w = so3_log(T.R);
  const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const auto K = detail::hat(w.data());
  const auto K2 = detail::mul3(K, K);
  const auto Vi = th < 1e-10 ? detail::lin3(1.0, -0.5, K, 0.0, K2)
                             : detail::lin3(1.0, -0.5, K, 1.0 / (th * th) - (1.0 + std::cos(th)) / (2.0 * th * std::sin(th)), K2);
  std::array<double, 6> xi{w[0], w[1], w[2], 0, 0, 0};
  for (int i = 0; i < 3; ++i) xi[3 + i] = Vi[3 * i] * T.t[0] + Vi[3 * i + 1] * T.t[1] + Vi[3 * i + 2] * T.t[2];
  return xi;
}
// svnicp::tensor2gtsamPose3 (src/core/ICPUtils.cpp:84-98): [x,y,z,rx,ry,rz] -> Pose3(Rot3::Expmap(r), t)
inline Pose3 correction_to_pose(const std::array<double, 6>& x) {
  Pose3 T;
  T.R = so3_exp(x.data() + 3);
  T.t = {x[0], x[1], x[2]};
  return T;
}

// ------------------------------------------------------------------------------------------------ clouds (pcl::PointXYZ = 3 x float32)
using Cloud = std::vector<std::array<float, 3>>;

// OdometryPipeline::crop_pointcloud (:692-704): keep min_range² < |p|² < max_range²; scan_max_range_ is updated to the
// largest SQUARED norm seen (:699) and is later used as a length (:578) — mirrored as is
inline Cloud crop_pointcloud(const Cloud& in, double min_range, double max_range, double* scan_max_range) {
  Cloud out;
  out.reserve(in.size());
  for (const auto& p : in) {
    // float32, left to right, as pt.x * pt.x + pt.y * pt.y + pt.z * pt.z on pcl::PointXYZ (:698); volatile keeps a host
    // compiler from contracting the sums into fused multiply-adds
    volatile float xx = p[0] * p[0], yy = p[1] * p[1], zz = p[2] * p[2];
    volatile float xy = xx + yy;
    const double n2 = (double)(float)(xy + zz);
    if (n2 > *scan_max_range) *scan_max_range = n2;
    if (n2 < max_range * max_range && n2 > min_range * min_range) out.push_back(p);
  }
  return out;
}

// ------------------------------------------------------------------------------------------------ deskew (:357-447)
// The same float32 / float64 steps as pipeline.py (kitti_correct_and_stamp, deskew_pointcloud) and csrc/scan_prep.hip
// (k_deskew_stamps, k_deskew_crop).  Parity unpinned: GTSAM and Eigen are absent, Pose3::Expmap is se3_exp above and
// transformFrom is R·p + t with each row summed left to right.
constexpr double kKittiVerticalAngleOffset = (0.205 * 3.14159265358979323846) / 180.0;   // :386

// per-point stamp field of PointField type UINT32 / FLOAT32 / FLOAT64, widened to double (:372-381, :403-413)
template <typename T>
inline std::vector<double> widen_stamps(const T* p, size_t n) {
  std::vector<double> o(n);
  for (size_t i = 0; i < n; ++i) o[i] = static_cast<double>(p[i]);
  return o;
}

// the KITTI branch (:385-401): p in double; axis = (p x z).normalized() = (y, -x, 0)/|.| (Eigen's normalized() leaves a zero
// vector as it is); AngleAxisd(0.205 deg, axis) * p stored into the float32 point; stamp 0.5 * (yaw / pi + 1) with the float
// yaw = -atan2(y, x) of the corrected float32 coordinates (formed as the double atan2 rounded once to float: the correctly
// rounded float result).  The rotation matrix is Eigen 3's AngleAxis::toRotationMatrix() (sin*axis, (1-c)*axis, diagonal
// last), the product summed left to right — unpinned (Eigen absent).
inline void kitti_correct_and_stamp(const Cloud& in, Cloud* out, std::vector<double>* stamps) {
  const double sn = std::sin(kKittiVerticalAngleOffset), c = std::cos(kKittiVerticalAngleOffset);
  out->resize(in.size());
  stamps->resize(in.size());
  for (size_t i = 0; i < in.size(); ++i) {
    const double x = in[i][0], y = in[i][1], z = in[i][2];
    double ax = y, ay = -x;
    const double az = 0.0;
    const double nn = (ax * ax + ay * ay) + az * az;
    if (nn > 0.0) { const double r = std::sqrt(nn); ax = ax / r; ay = ay / r; }
    const double sx = sn * ax, sy = sn * ay, sz = sn * az;
    const double cx = (1.0 - c) * ax, cy = (1.0 - c) * ay, cz = (1.0 - c) * az;
    const double R[9] = {cx * ax + c, cx * ay - sz, cx * az + sy, cx * ay + sz, cy * ay + c, cy * az - sx, cx * az - sy, cy * az + sx, cz * az + c};
    for (int d = 0; d < 3; ++d) (*out)[i][d] = (float)((R[3 * d] * x + R[3 * d + 1] * y) + R[3 * d + 2] * z);
    const float yaw = (float)(-std::atan2((double)(*out)[i][1], (double)(*out)[i][0]));
    (*stamps)[i] = 0.5 * ((double)yaw / 3.14159265358979323846 + 1.0);
  }
}

// OdometryPipeline::deskew_pointcloud (:357-447).  stamps: the widened per-point times, or nullptr (no "t" / "timestamp" /
// "time" field, :364-367: all zero -> the raw frame).  kitti: stamps from kitti_correct_and_stamp instead.  min / max
// (:414-417); min == max returns the UNMODIFIED frame (:418); else s = (t - min)/(max - min) (:419-423) and
// p' = float32(Pose3::Expmap((s - 0.5) * delta).transformFrom(double(p))) (:436-445); delta = Pose3::Logmap(start^-1 * finish)
// of the last two buffered poses (:427-432), [omega, v].  Deliberate deviation: non-finite stamps take no part in min / max
// (std::minmax_element's answer depends on where a NaN sits) and their points come out NaN, which the crop drops.
inline Cloud deskew_pointcloud(const Cloud& in, const std::vector<double>* stamps, const std::array<double, 6>& delta, bool kitti) {
  Cloud corrected;
  std::vector<double> kst;
  const Cloud* src = &in;
  if (kitti) {
    kitti_correct_and_stamp(in, &corrected, &kst);
    src = &corrected;
    stamps = &kst;
  }
  if (!stamps) return in;
  if (stamps->size() != in.size()) throw std::invalid_argument("deskew_pointcloud: one stamp per point");
  bool any = false;
  double tmin = 0, tmax = 0;
  for (double t : *stamps)
    if (std::isfinite(t)) {
      if (!any || t < tmin) tmin = t;
      if (!any || t > tmax) tmax = t;
      any = true;
    }
  if (!any || tmin == tmax) return in;   // :418, *frame
  Cloud out(in.size());
  for (size_t i = 0; i < in.size(); ++i) {
    const double t = (*stamps)[i];
    if (!std::isfinite(t)) { out[i] = {NAN, NAN, NAN}; continue; }
    const double sp = (t - tmin) / (tmax - tmin) - 0.5;
    double xi[6];
    for (int k = 0; k < 6; ++k) xi[k] = sp * delta[k];
    const Pose3 T = se3_exp(xi);
    const double x = (*src)[i][0], y = (*src)[i][1], z = (*src)[i][2];
    for (int d = 0; d < 3; ++d) out[i][d] = (float)(((T.R[3 * d] * x + T.R[3 * d + 1] * y) + T.R[3 * d + 2] * z) + T.t[d]);
  }
  return out;
}

// pcl::UniformSampling with setRadiusSearch(radius) (:684-690): grid of leaf size `radius` anchored at floor(min/leaf);
// per occupied leaf the point closest to the leaf centre survives (first one wins ties); leaves in ascending index
inline Cloud downsample_uniform(const Cloud& in, double radius) {
  if (in.empty() || radius <= 0) return in;
  const double inv = 1.0 / radius;
  int64_t mn[3], mx[3];
  for (int d = 0; d < 3; ++d) { mn[d] = INT64_MAX; mx[d] = INT64_MIN; }
  for (const auto& p : in)
    for (int d = 0; d < 3; ++d) {
      const int64_t c = (int64_t)std::floor((double)p[d] * inv);
      mn[d] = std::min(mn[d], c); mx[d] = std::max(mx[d], c);
    }
  const int64_t dx = mx[0] - mn[0] + 1, dy = mx[1] - mn[1] + 1;
  struct Rec { int64_t leaf; double d2; size_t idx; };
  std::vector<Rec> recs(in.size());
  for (size_t i = 0; i < in.size(); ++i) {
    int64_t ijk[3];
    double d2 = 0;
    for (int d = 0; d < 3; ++d) {
      ijk[d] = (int64_t)std::floor((double)in[i][d] * inv) - mn[d];
      const double c = ((double)(ijk[d] + mn[d]) + 0.5) * radius;
      d2 += ((double)in[i][d] - c) * ((double)in[i][d] - c);
    }
    recs[i] = {ijk[0] + ijk[1] * dx + ijk[2] * dx * dy, d2, i};
  }
  std::sort(recs.begin(), recs.end(), [](const Rec& a, const Rec& b) {
    if (a.leaf != b.leaf) return a.leaf < b.leaf;
    if (a.d2 != b.d2) return a.d2 < b.d2;
    return a.idx < b.idx;
  });
  Cloud out;
  for (size_t i = 0; i < recs.size(); ++i)
    if (i == 0 || recs[i].leaf != recs[i - 1].leaf) out.push_back(in[recs[i].idx]);
  return out;
}

// ------------------------------------------------------------------------------------------------ range-image segmentation
// LeGO-LOAM's ImageProjection::cloudHandler (include/segmentation/ImageProjection.h), which OdometryPipeline::lidar_msg_cb runs
// on every raw scan when USE_Segmentation is set (:328-355); the pipeline consumes segmentedCloud_ (GetSegmentedCloudPure,
// :533-534).  The contract is written out in include/svnicp_hip.h; the same float32 / float64 steps are in pipeline.py
// (segment_scan) and csrc/range_segment.hip.  Deliberate deviation: atan2f / sinf / cosf are the float64 functions of the float32
// operands rounded once.  The components are found by the reference's own BFS (labelComponents, :435-531).
struct SegImages {
  std::vector<int32_t> owner;    // winning input index per pixel, -1 empty
  std::vector<float> range;      // rangeMat_, -100000 empty
  std::vector<int8_t> ground;    // groundMat_
  std::vector<int32_t> label;    // labelMat_
};

namespace seg_detail {
constexpr double kPi = 3.14159265358979323846;
inline float atan2_f32(float y, float x) { return (float)std::atan2((double)y, (double)x); }
inline float deg_f32(float a) { return (float)((double)(a * 180.0f) / kPi); }
// projectPointCloud's per-point part (:240, :281-325), the one statement of the projection on the host (segment_images and
// VoxelHashMap::ClearSeenThrough): -> the point takes part; row, col, r its pixel and range
inline bool range_project(float x, float y, float z, const svnicp_seg_params& prm, int* row, int* col, float* r) {
  const int N = prm.n_scan, H = prm.horizon_scan;
  if (!(std::isfinite(x) && std::isfinite(y) && std::isfinite(z))) return false;   // removeNaNFromPointCloud (:240)
  const float va = deg_f32(atan2_f32(z, std::sqrt(x * x + y * y)));
  const float q = (va + prm.ang_bottom) / prm.ang_res_y;
  if (!(q > -1.0f && q < (float)N)) return false;                            // size_t conversion as on x86-64
  *row = (int)q;
  const float h = deg_f32(atan2_f32(x, y));
  double c = -std::round(((double)h - 90.0) / (double)prm.ang_res_x) + (double)(H / 2);
  if (c >= (double)H) c -= (double)H;
  if (!(c >= 0.0 && c < (double)H)) return false;
  *col = (int)c;
  *r = std::sqrt((x * x + y * y) + z * z);
  return !(*r < prm.min_range);
}
}  // namespace seg_detail

// the sensor ImageProjection.h compiles in (HDL-64E, :63-68) and the constants of :112-116 (= svnicp_seg_default_params(SVNICP_SEG_HDL64E))
inline svnicp_seg_params seg_hdl64e_params() {
  svnicp_seg_params s;
  s.struct_size = (int32_t)sizeof(svnicp_seg_params);
  s.n_scan = 64; s.horizon_scan = 2250; s.ground_scan_ind = 7;
  s.ang_res_x = (float)(360.0 / float(2250)); s.ang_res_y = (float)(26.8 / float(64 - 1)); s.ang_bottom = (float)24.8;
  s.min_range = 1.0f; s.mount_angle = 0.0f; s.segment_theta = (float)(60.0 / 180.0 * seg_detail::kPi);
  s.valid_point_num = 5; s.valid_line_num = 3;
  return s;
}

inline SegImages segment_images(const Cloud& pts, const svnicp_seg_params& prm) {
  using namespace seg_detail;
  const int N = prm.n_scan, H = prm.horizon_scan, G = prm.ground_scan_ind;
  const size_t NP = (size_t)N * H;
  SegImages im;
  im.owner.assign(NP, -1);
  im.range.assign(NP, -100000.0f);
  im.ground.assign(NP, 0);
  im.label.assign(NP, 0);
  for (size_t i = 0; i < pts.size(); ++i) {                                  // projectPointCloud (:281-325)
    int row, col;
    float r;
    if (!range_project(pts[i][0], pts[i][1], pts[i][2], prm, &row, &col, &r)) continue;
    const size_t p = (size_t)row * H + (size_t)col;
    im.owner[p] = (int32_t)i;                                                // the last point wins
    im.range[p] = r;
  }
  auto flat = [&](int32_t a, int32_t b) {                                    // groundRemoval's test, lower a, upper b
    const float dx = pts[b][0] - pts[a][0], dy = pts[b][1] - pts[a][1], dz = pts[b][2] - pts[a][2];
    const float ang = deg_f32(atan2_f32(dz, std::sqrt(dx * dx + dy * dy)));
    return std::fabs(ang - prm.mount_angle) <= 10.0f;
  };
  for (int j = 0; j < H; ++j)                                                // groundRemoval (:329-374), its own loop order
    for (int i = 0; i < G; ++i) {
      const int32_t lo = im.owner[(size_t)i * H + j], up = im.owner[(size_t)(i + 1) * H + j];
      if (lo < 0 || up < 0) { im.ground[(size_t)i * H + j] = -1; continue; }
      if (flat(lo, up)) { im.ground[(size_t)i * H + j] = 1; im.ground[(size_t)(i + 1) * H + j] = 1; }
    }
  for (size_t p = 0; p < NP; ++p)
    if (im.ground[p] == 1 || im.owner[p] < 0) im.label[p] = -1;
  const float alpha_x = (float)((double)prm.ang_res_x / 180.0 * kPi), alpha_y = (float)((double)prm.ang_res_y / 180.0 * kPi);
  const float sx = (float)std::sin((double)alpha_x), cx = (float)std::cos((double)alpha_x);
  const float sy = (float)std::sin((double)alpha_y), cy = (float)std::cos((double)alpha_y);
  std::vector<int> queue(NP), pushed(NP);
  int32_t label_count = 1;
  const int nbr[4][2] = {{-1, 0}, {0, 1}, {0, -1}, {1, 0}};
  for (int row = 0; row < N; ++row)                                          // cloudSegmentation (:379-383)
    for (int col = 0; col < H; ++col) {
      if (im.label[(size_t)row * H + col] != 0) continue;
      std::vector<bool> line(N, false);                                      // labelComponents (:435-531)
      size_t qs = 0, qe = 0, np = 0;
      queue[qe++] = row * H + col;
      pushed[np++] = row * H + col;
      while (qs < qe) {
        const int from = queue[qs++];
        const int fr = from / H, fc = from % H;
        im.label[from] = label_count;
        for (const auto& d : nbr) {
          const int tr = fr + d[0];
          int tc = fc + d[1];
          if (tr < 0 || tr >= N) continue;
          if (tc < 0) tc = H - 1;
          if (tc >= H) tc = 0;
          const int to = tr * H + tc;
          if (im.label[to] != 0) continue;
          const float d1 = std::max(im.range[from], im.range[to]), d2 = std::min(im.range[from], im.range[to]);
          const float s = d[0] == 0 ? sx : sy, c = d[0] == 0 ? cx : cy;
          if (atan2_f32(d2 * s, d1 - d2 * c) > prm.segment_theta) {
            queue[qe++] = to;
            im.label[to] = label_count;
            line[tr] = true;
            pushed[np++] = to;
          }
        }
      }
      bool feasible = np >= 30;
      if (!feasible && np >= (size_t)prm.valid_point_num) {
        int lines = 0;
        for (int r = 0; r < N; ++r) lines += line[r] ? 1 : 0;
        feasible = lines >= prm.valid_line_num;
      }
      if (feasible) ++label_count;
      else for (size_t k = 0; k < np; ++k) im.label[pushed[k]] = 999999;
    }
  return im;
}

// segmentedCloud_ (:384-414) and the input index of each of its points
inline Cloud segment_scan(const Cloud& pts, const svnicp_seg_params& prm, std::vector<int64_t>* src_index = nullptr) {
  const SegImages im = segment_images(pts, prm);
  const int N = prm.n_scan, H = prm.horizon_scan;
  Cloud out;
  if (src_index) src_index->clear();
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < H; ++j) {
      const size_t p = (size_t)i * H + j;
      const int32_t lab = im.label[p];
      const bool g = im.ground[p] == 1;
      if (!(lab > 0 || g) || lab == 999999) continue;
      if (g && j % 5 != 0 && j > 5 && j < H - 5) continue;                  // most ground points are skipped
      out.push_back(pts[(size_t)im.owner[p]]);
      if (src_index) src_index->push_back(im.owner[p]);
    }
  return out;
}

// what a coarse-to-fine pose search returns (svnicp_map_search_poses, include/svnicp_hip.h; the helpers are further down)
using Lattice = std::vector<std::array<int32_t, 6>>;   // integer vectors on the finest lattice of a search
struct MapSearchLevel {   // one level: its nodes, and the indices of the kept ones in rank order
  Lattice lattice;
  std::vector<double> poses12, records;
  std::vector<int32_t> kept;
};
struct MapSearchResult {
  int levels = 0, active_axes = 0;
  int64_t nodes_scored = 0;
  std::vector<int64_t> level_count;
  std::vector<int32_t> level_kept;
  std::array<double, 6> fine_step{}, best_correction{};
  std::array<int32_t, 6> best_lattice{};
  std::array<double, 12> best_pose{};
  std::array<double, 4> best_record{}, zero_record{};
  double cost_level0 = 0;   // the best cost of level 0
  // the kept nodes of the last level in rank order
  Lattice top_lattice;
  std::vector<std::array<double, 6>> top_corrections;
  std::vector<double> top_poses12, top_records;
  std::vector<MapSearchLevel> level;   // every level (the host restatement only)
};

// ------------------------------------------------------------------------------------------------ local map
// svnicp::VoxelHashMap (src/core/VoxelHashMap.cpp:22-101): voxel -> at most max_points points in insertion order; voxel index
// = coordinates / voxel_size truncated TOWARD ZERO (Eigen cast<int>, :29); a voxel is dropped when its FIRST point is
// farther than max_range from the current position (:89-97) and selected by GetMap(pose, r) when that point is closer
// than r (:48-58).  An ordered map stands in for tsl::robin_map: deterministic iteration (ascending voxel index).
class VoxelHashMap {
 public:
  VoxelHashMap(double voxel_size, double max_range, int max_points) : voxel_size_(voxel_size), max_range_(max_range), max_points_(max_points) {}
  bool Empty() const { return map_.empty(); }
  size_t Size() const { return map_.size(); }
  void Clear() { map_.clear(); }

  void AddPointCloud(const Cloud& cloud, const Pose3& pose) {
    // pcl::transformPointCloud with gtsam's double Matrix4 (VoxelHashMap.cpp:23-25): formed in double from the widened float32
    // point, left to right, rounded once to float32 (the expression of map_table.hip and pipeline.py)
    const float vs = (float)voxel_size_;
    for (const auto& p : cloud) {
      std::array<float, 3> q;
      for (int i = 0; i < 3; ++i)
        q[i] = (float)(((pose.R[3 * i] * (double)p[0] + pose.R[3 * i + 1] * (double)p[1]) + pose.R[3 * i + 2] * (double)p[2]) + pose.t[i]);
      const Key k{(int64_t)std::trunc(q[0] / vs), (int64_t)std::trunc(q[1] / vs), (int64_t)std::trunc(q[2] / vs)};
      auto& v = map_[k];
      if ((int)v.size() < max_points_) v.push_back(q);
    }
    RemoveFarPointCloud(pose.t);
  }
  // visibility-based clearing (include/svnicp_hip.h: svnicp_map_clear_seen_through, the same steps in the same float32 /
  // float64 order as pipeline.py and csrc/map_visibility.hip): a stored point is dropped when the scan's beam in its direction
  // returned from clearly behind it.  Throws std::invalid_argument where the C call answers SVNICP_ERR_INVALID.
  svnicp_visibility_stats ClearSeenThrough(const Cloud& scan, const Pose3& pose, const svnicp_seg_params& sensor, const svnicp_visibility_opt& opt) {
    const int N = sensor.n_scan, H = sensor.horizon_scan;
    if (sensor.struct_size != (int32_t)sizeof(svnicp_seg_params) || opt.struct_size != (int32_t)sizeof(svnicp_visibility_opt) ||
        !(N >= 1 && N <= 128 && H >= 1 && (int64_t)N * H <= (int64_t)1 << 19) ||
        !(std::isfinite(sensor.ang_res_x) && sensor.ang_res_x > 0 && std::isfinite(sensor.ang_res_y) && sensor.ang_res_y > 0 &&
          std::isfinite(sensor.ang_bottom) && std::isfinite(sensor.min_range)) ||
        !(opt.window_rows >= 0 && opt.window_rows <= 4 && opt.window_cols >= 0 && opt.window_cols <= 8) ||
        !(std::isfinite(opt.margin_abs) && opt.margin_abs >= 0 && std::isfinite(opt.margin_rel) && opt.margin_rel >= 0) ||
        !(std::isfinite(opt.max_range) && opt.max_range > 0))
      throw std::invalid_argument("VoxelHashMap::ClearSeenThrough: bad sensor or options");
    svnicp_visibility_stats st{0, 0, 0, 0};
    if (scan.empty() || map_.empty()) return st;
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<float> img((size_t)N * H, inf);                                // the minimum-range image, +inf = empty
    for (const auto& p : scan) {
      int row, col;
      float r;
      if (!seg_detail::range_project(p[0], p[1], p[2], sensor, &row, &col, &r)) continue;
      float& px = img[(size_t)row * H + col];
      if (r < px) px = r;
    }
    for (float v : img) st.pixels_filled += v < inf ? 1 : 0;
    for (auto it = map_.begin(); it != map_.end();) {
      Cloud& v = it->second;
      size_t w = 0;
      for (size_t i = 0; i < v.size(); ++i) {
        const double d0 = (double)v[i][0] - pose.t[0], d1 = (double)v[i][1] - pose.t[1], d2 = (double)v[i][2] - pose.t[2];
        const float s0 = (float)((pose.R[0] * d0 + pose.R[3] * d1) + pose.R[6] * d2);   // R^T d, rounded once
        const float s1 = (float)((pose.R[1] * d0 + pose.R[4] * d1) + pose.R[7] * d2);
        const float s2 = (float)((pose.R[2] * d0 + pose.R[5] * d1) + pose.R[8] * d2);
        int row, col;
        float rm;
        bool remove = false;
        if (seg_detail::range_project(s0, s1, s2, sensor, &row, &col, &rm) && !(rm > opt.max_range) && img[(size_t)row * H + col] < inf) {
          float r_min = inf;
          for (int rr = std::max(0, row - opt.window_rows); rr <= std::min(N - 1, row + opt.window_rows); ++rr)   // rows do not wrap
            for (int dc = -opt.window_cols; dc <= opt.window_cols; ++dc)
              r_min = std::min(r_min, img[(size_t)rr * H + (size_t)(((col + dc) % H + H) % H)]);                  // columns wrap
          ++st.points_tested;
          const float margin = std::fmax(opt.margin_abs, opt.margin_rel * r_min);
          remove = rm < r_min - margin;
        }
        if (remove) ++st.points_removed;
        else v[w++] = v[i];
      }
      v.resize(w);
      if (v.empty()) { it = map_.erase(it); ++st.voxels_emptied; }
      else ++it;
    }
    return st;
  }
  // how well the scan `rows` (sensor frame) fits the map at each of C poses (poses12: [C][12], R row-major then t, map <- sensor)
  // -> [C][4] {located, inliers, sum_d2, cost}: include/svnicp_hip.h's svnicp_map_score_poses restated, the float32 / float64
  // steps and the order of the sums (rows ascending, from 0.0) those of pipeline.py's VoxelHashMap.score_poses.  Throws
  // std::invalid_argument where the C call answers SVNICP_ERR_INVALID.
  std::vector<double> ScorePoses(const Cloud& rows, const std::vector<double>& poses12, double gate) const {
    const size_t C = poses12.size() / 12;
    if (poses12.size() % 12 != 0 || C < 1 || C > ((size_t)1 << 20)) throw std::invalid_argument("VoxelHashMap::ScorePoses: need 1 <= C <= 2^20 poses of 12 doubles");
    if (!(std::isfinite(gate) && gate > 0 && gate <= voxel_size_))
      throw std::invalid_argument("VoxelHashMap::ScorePoses: the gate must be finite, > 0 and <= voxel_size");
    const double thr2 = gate * gate;
    const float vs = (float)voxel_size_;
    const int64_t lim = (int64_t)1 << 20, n = (int64_t)rows.size();
    std::vector<double> out(4 * C, 0.0);
    for (size_t ci = 0; ci < C; ++ci) {
      const double* R = &poses12[12 * ci];
      const double* t = R + 9;
      int64_t located = 0, inliers = 0;
      double sum = 0.0;
      for (const auto& p : rows) {
        float c[3];
        int64_t v[3];
        bool ok = true;
        for (int d = 0; d < 3; ++d) {
          c[d] = (float)(((R[3 * d] * (double)p[0] + R[3 * d + 1] * (double)p[1]) + R[3 * d + 2] * (double)p[2]) + t[d]);
          const float f = std::trunc(c[d] / vs);
          ok = ok && f >= (float)-lim && f < (float)lim;   // also false for NaN and inf
          v[d] = ok ? (int64_t)f : 0;
        }
        if (!ok) continue;
        bool have = false;
        double best = 0.0;
        for (int j = 0; j < 27; ++j) {
          const Key w{v[0] + (j / 9 - 1), v[1] + ((j / 3) % 3 - 1), v[2] + (j % 3 - 1)};
          if (w[0] < -lim || w[0] >= lim || w[1] < -lim || w[1] >= lim || w[2] < -lim || w[2] >= lim) continue;   // no such voxel
          const auto it = map_.find(w);
          if (it == map_.end()) continue;
          const size_t cnt = std::min(it->second.size(), (size_t)max_points_);
          for (size_t k = 0; k < cnt; ++k) {
            const auto& q = it->second[k];
            const double dx = (double)q[0] - (double)c[0], dy = (double)q[1] - (double)c[1], dz = (double)q[2] - (double)c[2];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (!have || d2 < best) { best = d2; have = true; }
          }
        }
        if (!have) continue;
        ++located;
        if (best < thr2) { ++inliers; sum += best; }
      }
      out[4 * ci] = (double)located; out[4 * ci + 1] = (double)inliers; out[4 * ci + 2] = sum;
      out[4 * ci + 3] = n > 0 ? (sum + (double)(n - inliers) * thr2) / (double)n : thr2;
    }
    return out;
  }
  // svnicp_map_search_poses restated from ScorePoses and the lattice helpers below (search_lattice, search_children,
  // search_rank), the lattice and the ranks with the bits of pipeline.py's VoxelHashMap.search_poses; every level is kept.
  // Throws std::invalid_argument where the C call answers SVNICP_ERR_INVALID.
  MapSearchResult SearchPoses(const Cloud& rows, const Pose3& guess, const std::array<double, 6>& extent, const std::array<double, 6>& step,
                              int levels, int keep, double gate) const;
  Cloud GetMap() const {
    Cloud out;
    for (const auto& kv : map_) out.insert(out.end(), kv.second.begin(), kv.second.end());
    return out;
  }
  Cloud GetMap(const Pose3& pose, double max_range) const {
    Cloud out;
    for (const auto& kv : map_)
      if (dist2(kv.second.front(), pose.t) < max_range * max_range) out.insert(out.end(), kv.second.begin(), kv.second.end());
    return out;
  }

 private:
  using Key = std::array<int64_t, 3>;
  static double dist2(const std::array<float, 3>& p, const std::array<double, 3>& c) {
    double s = 0;
    for (int i = 0; i < 3; ++i) s += ((double)p[i] - c[i]) * ((double)p[i] - c[i]);
    return s;
  }
  void RemoveFarPointCloud(const std::array<double, 3>& pos) {
    for (auto it = map_.begin(); it != map_.end();)
      it = dist2(it->second.front(), pos) > max_range_ * max_range_ ? map_.erase(it) : std::next(it);
  }
  double voxel_size_, max_range_;
  int max_points_;
  std::map<Key, Cloud> map_;
};

// The same map resident in HBM (svnicp_map_* of the C ABI, csrc/voxel_map.hip): AddPointCloud uploads only the new points, a
// query leaves float64 rows in device memory for SVNICP::add_cloud_device_target.  Same voxel order as the host map above.
class DeviceVoxelMap {
 public:
  DeviceVoxelMap(double voxel_size, double max_range, int max_points, int device = 0) {
    if (svnicp_map_create(device, voxel_size, max_range, max_points, 0, &m_) != 0) throw std::runtime_error(svnicp_map_last_error(nullptr));
  }
  ~DeviceVoxelMap() { svnicp_map_destroy(m_); }
  DeviceVoxelMap(const DeviceVoxelMap&) = delete;
  DeviceVoxelMap& operator=(const DeviceVoxelMap&) = delete;
  bool Empty() { return Size() == 0; }
  size_t Size() { int64_t n = 0; chk(svnicp_map_size(m_, &n)); return (size_t)n; }
  void AddPointCloud(const Cloud& cloud, const Pose3& pose) {
    chk(svnicp_map_add_cloud(m_, cloud.empty() ? nullptr : &cloud[0][0], (int64_t)cloud.size(), SVNICP_MEM_HOST, pose.R.data(), pose.t.data()));
  }
  void AddPointCloudDevice(const float* dev_xyz, int64_t n, const Pose3& pose) {   // float32 rows already in HBM (DevicePrep)
    chk(svnicp_map_add_cloud(m_, dev_xyz, n, SVNICP_MEM_DEVICE, pose.R.data(), pose.t.data()));
  }
  // visibility-based clearing (svnicp_map_clear_seen_through) with a scan on the host / already in HBM
  svnicp_visibility_stats ClearSeenThrough(const Cloud& scan, const Pose3& pose, const svnicp_seg_params& sensor, const svnicp_visibility_opt& opt) {
    svnicp_visibility_stats st{};
    chk(svnicp_map_clear_seen_through(m_, scan.empty() ? nullptr : &scan[0][0], (int64_t)scan.size(), SVNICP_MEM_HOST, pose.R.data(), pose.t.data(),
                                      &sensor, &opt, &st));
    return st;
  }
  svnicp_visibility_stats ClearSeenThroughDevice(const float* dev_xyz, int64_t n, const Pose3& pose, const svnicp_seg_params& sensor,
                                                 const svnicp_visibility_opt& opt) {
    svnicp_visibility_stats st{};
    chk(svnicp_map_clear_seen_through(m_, dev_xyz, n, SVNICP_MEM_DEVICE, pose.R.data(), pose.t.data(), &sensor, &opt, &st));
    return st;
  }
  // -> number of points; the rows are at points_devptr()
  int64_t GetMap(const Pose3& pose, double max_range) { int64_t n = 0; chk(svnicp_map_query(m_, pose.t.data(), max_range, &n)); return n; }
  int64_t GetMap() { int64_t n = 0; chk(svnicp_map_query(m_, nullptr, -1.0, &n)); return n; }
  const double* points_devptr() { return static_cast<const double*>(svnicp_map_points_devptr(m_)); }
  std::vector<double> download() {
    int64_t n = 0;
    chk(svnicp_map_download(m_, nullptr, 0, &n));
    std::vector<double> o((size_t)3 * n);
    if (n) chk(svnicp_map_download(m_, o.data(), n, &n));
    return o;
  }
  // normals of the rows of the last GetMap from the 27-voxel neighbourhoods of the map (svnicp_map_query_normals)
  // -> rows with a normal; the rows ([count][3], 0 = no normal) are at normals_devptr()
  int64_t QueryNormals(int normal_k) { int64_t n = 0; chk(svnicp_map_query_normals(m_, normal_k, &n)); return n; }
  const double* normals_devptr() { return static_cast<const double*>(svnicp_map_normals_devptr(m_)); }
  // how well a scan fits the map at each of C poses (svnicp_map_score_poses; VoxelHashMap::ScorePoses is the host restatement)
  // -> [C][4] {located, inliers, sum_d2, cost}; rows on the host / already in HBM (DevicePrep::source_f32)
  std::vector<double> ScorePoses(const Cloud& rows, const std::vector<double>& poses12, double gate) {
    return score(rows.empty() ? nullptr : &rows[0][0], (int64_t)rows.size(), SVNICP_MEM_HOST, poses12, gate);
  }
  std::vector<double> ScorePosesDevice(const float* dev_xyz, int64_t n, const std::vector<double>& poses12, double gate) {
    return score(dev_xyz, n, SVNICP_MEM_DEVICE, poses12, gate);
  }
  std::vector<double> download_normals() {   // test tap
    int64_t n = 0;
    chk(svnicp_map_download_normals(m_, nullptr, 0, &n));
    std::vector<double> o((size_t)3 * n);
    if (n) chk(svnicp_map_download_normals(m_, o.data(), n, &n));
    return o;
  }
  // coarse-to-fine search around `guess` (svnicp_map_search_poses; VoxelHashMap::SearchPoses is the host restatement): the
  // struct's fields, the kept nodes of the last level (svnicp_map_search_top) and level 0's best cost; rows on the host / in HBM
  MapSearchResult SearchPoses(const Cloud& rows, const Pose3& guess, const std::array<double, 6>& extent, const std::array<double, 6>& step,
                              int levels, int keep, double gate) {
    return search(rows.empty() ? nullptr : &rows[0][0], (int64_t)rows.size(), SVNICP_MEM_HOST, guess, extent, step, levels, keep, gate);
  }
  MapSearchResult SearchPosesDevice(const float* dev_xyz, int64_t n, const Pose3& guess, const std::array<double, 6>& extent,
                                    const std::array<double, 6>& step, int levels, int keep, double gate) {
    return search(dev_xyz, n, SVNICP_MEM_DEVICE, guess, extent, step, levels, keep, gate);
  }

 private:
  MapSearchResult search(const float* xyz, int64_t n, int mem, const Pose3& guess, const std::array<double, 6>& extent,
                         const std::array<double, 6>& step, int levels, int keep, double gate) {
    svnicp_map_search_opt opt{};
    std::copy(extent.begin(), extent.end(), opt.extent);
    std::copy(step.begin(), step.end(), opt.step);
    opt.levels = levels; opt.keep = keep; opt.max_corr_dist = gate;
    svnicp_map_search s{};
    chk(svnicp_map_search_poses(m_, xyz, n, mem, guess.R.data(), guess.t.data(), &opt, &s));
    MapSearchResult r;
    r.levels = s.levels; r.active_axes = s.active_axes; r.nodes_scored = s.nodes_scored;
    r.level_count.assign(s.level_count, s.level_count + s.levels);
    r.level_kept.assign(s.level_kept, s.level_kept + s.levels);
    std::copy(s.fine_step, s.fine_step + 6, r.fine_step.begin());
    std::copy(s.best_lattice, s.best_lattice + 6, r.best_lattice.begin());
    std::copy(s.best_correction, s.best_correction + 6, r.best_correction.begin());
    std::copy(s.best_pose, s.best_pose + 12, r.best_pose.begin());
    std::copy(s.best_record, s.best_record + 4, r.best_record.begin());
    std::copy(s.zero_record, s.zero_record + 4, r.zero_record.begin());
    const int n_top = s.level_kept[s.levels - 1];
    r.top_lattice.resize((size_t)n_top); r.top_corrections.resize((size_t)n_top);
    r.top_poses12.resize((size_t)12 * n_top); r.top_records.resize((size_t)4 * n_top);
    int got = 0;
    chk(svnicp_map_search_top(m_, n_top, &r.top_lattice[0][0], &r.top_corrections[0][0], r.top_poses12.data(), r.top_records.data(), &got));
    std::vector<double> rec0((size_t)4 * s.level_count[0]);
    std::vector<int32_t> kept0((size_t)s.level_kept[0]);
    chk(svnicp_map_search_level(m_, 0, s.level_count[0], nullptr, nullptr, rec0.data(), kept0.data(), nullptr, nullptr));
    r.cost_level0 = rec0[(size_t)4 * kept0[0] + 3];
    return r;
  }
  std::vector<double> score(const float* xyz, int64_t n, int mem, const std::vector<double>& poses12, double gate) {
    const int64_t C = (int64_t)(poses12.size() / 12);
    std::vector<double> out((size_t)SVNICP_MAP_SCORE_FIELDS * (size_t)std::max<int64_t>(C, 0));
    chk(svnicp_map_score_poses(m_, xyz, n, mem, poses12.data(), C, SVNICP_MEM_HOST, gate, out.data()));
    return out;
  }
  void chk(int rc) { if (rc != 0) throw std::runtime_error(svnicp_map_last_error(m_)); }
  svnicp_map* m_ = nullptr;
};

// ------------------------------------------------------------------------------------------------ search grid and seed
// Candidates are CORRECTIONS in the solver's parametrisation [x, y, z, rx, ry, rz]: node x gives the pose
// guess * correction_to_pose(x), which is how a particle's total pose is composed, so the best nodes can be handed to the solver
// as particles unchanged.  The same helpers, with the same order of the nodes, are in pipeline.py.
constexpr double kGridSlack = 1e-9;   // extent / step may miss an integer by a rounding: 10 deg / 2.5 deg is 4

// Per axis the offsets are k * step, k = -m..m, m = floor(extent / step); extent 0 fixes the axis.  Lexicographic order, x
// slowest; *zero_index is the node of the zero correction.  Throws std::invalid_argument for a negative or non-finite extent, a
// step <= 0 on an axis with an extent, and more than 2^20 nodes.
inline std::vector<std::array<double, 6>> correction_grid(const std::array<double, 6>& extent, const std::array<double, 6>& step, size_t* zero_index = nullptr) {
  int64_t m[6];
  size_t count = 1, zero = 0;
  for (int d = 0; d < 6; ++d) {
    if (!(std::isfinite(extent[d]) && extent[d] >= 0)) throw std::invalid_argument("correction_grid: extents must be finite and >= 0");
    m[d] = 0;
    if (extent[d] != 0.0) {
      if (!(std::isfinite(step[d]) && step[d] > 0)) throw std::invalid_argument("correction_grid: an axis with a non-zero extent needs a finite step > 0");
      m[d] = (int64_t)std::floor(extent[d] / step[d] + kGridSlack);
    }
    if (m[d] > ((int64_t)1 << 19)) throw std::invalid_argument("correction_grid: more than 2^20 nodes");
    count *= (size_t)(2 * m[d] + 1);
    if (count > ((size_t)1 << 20)) throw std::invalid_argument("correction_grid: more than 2^20 nodes");
    zero = zero * (size_t)(2 * m[d] + 1) + (size_t)m[d];
  }
  std::vector<std::array<double, 6>> nodes(count);
  for (size_t i = 0; i < count; ++i) {
    size_t r = i;
    for (int d = 5; d >= 0; --d) {
      const int64_t w = 2 * m[d] + 1, k = (int64_t)(r % (size_t)w) - m[d];
      r /= (size_t)w;
      nodes[i][d] = (double)k * (m[d] ? step[d] : 0.0);
    }
  }
  if (zero_index) *zero_index = zero;
  return nodes;
}

// guess * correction_to_pose(x) per node -> [C][12], R row-major then t (svnicp_map_score_poses' layout)
inline std::vector<double> correction_poses(const Pose3& guess, const std::vector<std::array<double, 6>>& nodes) {
  std::vector<double> out(12 * nodes.size());
  for (size_t i = 0; i < nodes.size(); ++i) {
    const Pose3 T = guess * correction_to_pose(nodes[i]);
    std::copy(T.R.begin(), T.R.end(), out.begin() + 12 * i);
    std::copy(T.t.begin(), T.t.end(), out.begin() + 12 * i + 9);
  }
  return out;
}

// the indices of the P best nodes of a scoring ([C][4] records), ordered by (cost, index): ties in cost go to the lower index
inline std::vector<size_t> seed_from_scores(const std::vector<double>& scores, size_t P) {
  const size_t C = scores.size() / 4;
  if (P < 1 || P > C) throw std::invalid_argument("seed_from_scores: need 1 <= P <= number of nodes");
  std::vector<size_t> order(C);
  std::iota(order.begin(), order.end(), (size_t)0);
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return scores[4 * a + 3] < scores[4 * b + 3]; });
  order.resize(P);
  return order;
}

// ---- the coarse-to-fine search: the lattice of svnicp_map_search_poses (include/svnicp_hip.h), as in pipeline.py -------------
struct SearchLattice {
  std::array<int64_t, 6> m{};     // level 0: j = -m..m per axis
  std::array<double, 6> fine{};   // step / 3^(levels-1), 0 on an axis without a usable step
  std::vector<int> active;        // the axes with m >= 1
  Lattice level0;                 // j * 3^(levels-1), lexicographic, x slowest
  size_t zero = 0;                // level 0's node of the zero correction
  std::vector<int64_t> count;     // nodes per level
  std::vector<int32_t> kept;      // min(keep, count)
};
inline int64_t pow3(int e) { int64_t p = 1; while (e-- > 0) p *= 3; return p; }

// throws std::invalid_argument for what the C call refuses: levels outside 1..8, keep outside 1..1024, a bad extent or step, a
// level over 2^20 nodes, m * 3^(levels-1) + (3^(levels-1) - 1) / 2 >= 2^20
inline SearchLattice search_lattice(const std::array<double, 6>& extent, const std::array<double, 6>& step, int levels, int keep) {
  if (levels < 1 || levels > SVNICP_MAP_SEARCH_MAX_LEVELS) throw std::invalid_argument("search_lattice: need 1 <= levels <= 8");
  if (keep < 1 || keep > SVNICP_MAP_SEARCH_MAX_KEEP) throw std::invalid_argument("search_lattice: need 1 <= keep <= 1024");
  const int64_t top = pow3(levels - 1), lim = (int64_t)1 << 20;
  SearchLattice L;
  int64_t c0 = 1;
  for (int a = 0; a < 6; ++a) {
    const double e = extent[a], s = step[a];
    if (!(std::isfinite(e) && e >= 0)) throw std::invalid_argument("search_lattice: extents must be finite and >= 0");
    int64_t m = 0;
    if (e != 0.0) {
      if (!(std::isfinite(s) && s > 0)) throw std::invalid_argument("search_lattice: an axis with a non-zero extent needs a finite step > 0");
      const double q = std::floor(e / s + kGridSlack);
      m = q < (double)lim ? (int64_t)q : lim;
    }
    if (m * top + (top - 1) / 2 >= lim) throw std::invalid_argument("search_lattice: lattice overflow");
    L.m[a] = m;
    L.fine[a] = (std::isfinite(s) && s > 0) ? s / (double)top : 0.0;
    if (m >= 1) L.active.push_back(a);
    c0 *= 2 * m + 1;
    if (c0 > lim) throw std::invalid_argument("search_lattice: a level holds more than 2^20 nodes");
    L.zero = L.zero * (size_t)(2 * m + 1) + (size_t)m;
  }
  const int64_t children = pow3((int)L.active.size());
  for (int l = 0; l < levels; ++l) {
    const int64_t c = l == 0 ? c0 : (int64_t)L.kept.back() * children;
    if (c > lim) throw std::invalid_argument("search_lattice: a level holds more than 2^20 nodes");
    L.count.push_back(c);
    L.kept.push_back((int32_t)std::min<int64_t>(keep, c));
  }
  L.level0.resize((size_t)c0);
  for (size_t i = 0; i < (size_t)c0; ++i) {
    size_t r = i;
    for (int a = 5; a >= 0; --a) {
      const int64_t w = 2 * L.m[a] + 1;
      L.level0[i][a] = (int32_t)(((int64_t)(r % (size_t)w) - L.m[a]) * top);
      r /= (size_t)w;
    }
  }
  return L;
}

// the nodes of level `level`+1 from the kept nodes of level `level` in rank order: child index = rank * 3^A + offset index
inline Lattice search_children(const Lattice& kept_lattice, int level, int levels, const std::vector<int>& active) {
  const int64_t scale = pow3(levels - 2 - level), children = pow3((int)active.size());
  Lattice out;
  out.reserve(kept_lattice.size() * (size_t)children);
  for (const auto& parent : kept_lattice)
    for (int64_t o = 0; o < children; ++o) {
      std::array<int32_t, 6> k = parent;
      int64_t r = o;
      for (int j = (int)active.size() - 1; j >= 0; --j) { k[active[j]] += (int32_t)((r % 3 - 1) * scale); r /= 3; }
      out.push_back(k);
    }
  return out;
}

// the indices of the min(keep, count) best nodes in rank order: ascending (cost, lattice vector lexicographic, x first)
inline std::vector<int32_t> search_rank(const std::vector<double>& records, const Lattice& lattice, int keep) {
  if (records.size() != 4 * lattice.size()) throw std::invalid_argument("search_rank: one record per lattice vector");
  std::vector<int32_t> order(lattice.size());
  std::iota(order.begin(), order.end(), 0);
  std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
    const double ca = records[4 * (size_t)a + 3], cb = records[4 * (size_t)b + 3];
    return ca != cb ? ca < cb : lattice[a] < lattice[b];
  });
  order.resize(std::min(order.size(), (size_t)keep));
  return order;
}

// x = (double)k * fine: one multiplication per entry
inline std::vector<std::array<double, 6>> search_corrections(const Lattice& lattice, const std::array<double, 6>& fine) {
  std::vector<std::array<double, 6>> x(lattice.size());
  for (size_t i = 0; i < lattice.size(); ++i)
    for (int a = 0; a < 6; ++a) x[i][a] = (double)lattice[i][a] * fine[a];
  return x;
}

inline MapSearchResult VoxelHashMap::SearchPoses(const Cloud& rows, const Pose3& guess, const std::array<double, 6>& extent,
                                                 const std::array<double, 6>& step, int levels, int keep, double gate) const {
  if (!(std::isfinite(gate) && gate > 0 && gate <= voxel_size_))
    throw std::invalid_argument("VoxelHashMap::SearchPoses: the gate must be finite, > 0 and <= voxel_size");
  for (int i = 0; i < 9; ++i) if (!std::isfinite(guess.R[i])) throw std::invalid_argument("VoxelHashMap::SearchPoses: the guess must be finite");
  for (int i = 0; i < 3; ++i) if (!std::isfinite(guess.t[i])) throw std::invalid_argument("VoxelHashMap::SearchPoses: the guess must be finite");
  const SearchLattice L = search_lattice(extent, step, levels, keep);
  MapSearchResult r;
  r.levels = levels; r.active_axes = (int)L.active.size();
  r.level_count = L.count; r.level_kept = L.kept; r.fine_step = L.fine;
  for (int l = 0; l < levels; ++l) {
    MapSearchLevel lv;
    if (l == 0) lv.lattice = L.level0;
    else {
      Lattice parents;
      for (int32_t i : r.level.back().kept) parents.push_back(r.level.back().lattice[(size_t)i]);
      lv.lattice = search_children(parents, l - 1, levels, L.active);
    }
    lv.poses12 = correction_poses(guess, search_corrections(lv.lattice, L.fine));
    lv.records = ScorePoses(rows, lv.poses12, gate);
    lv.kept = search_rank(lv.records, lv.lattice, keep);
    r.nodes_scored += (int64_t)lv.lattice.size();
    r.level.push_back(std::move(lv));
  }
  const MapSearchLevel& last = r.level.back();
  for (int32_t i : last.kept) {
    r.top_lattice.push_back(last.lattice[(size_t)i]);
    r.top_poses12.insert(r.top_poses12.end(), last.poses12.begin() + 12 * (size_t)i, last.poses12.begin() + 12 * (size_t)i + 12);
    r.top_records.insert(r.top_records.end(), last.records.begin() + 4 * (size_t)i, last.records.begin() + 4 * (size_t)i + 4);
  }
  r.top_corrections = search_corrections(r.top_lattice, L.fine);
  r.best_lattice = r.top_lattice[0]; r.best_correction = r.top_corrections[0];
  std::copy(r.top_poses12.begin(), r.top_poses12.begin() + 12, r.best_pose.begin());
  std::copy(r.top_records.begin(), r.top_records.begin() + 4, r.best_record.begin());
  std::copy(r.level[0].records.begin() + 4 * L.zero, r.level[0].records.begin() + 4 * L.zero + 4, r.zero_record.begin());
  r.cost_level0 = r.level[0].records[4 * (size_t)r.level[0].kept[0] + 3];
  return r;
}

// crop_pointcloud + the two uniform samplings on the device (svnicp_prep_*, csrc/scan_prep.hip): the raw scan is uploaded
// once; the cropped cloud, the map cloud (float32) and the source cloud (float64 rows) stay in HBM
class DevicePrep {
 public:
  explicit DevicePrep(int device = 0) { if (svnicp_prep_create(device, &p_) != 0) throw std::runtime_error(svnicp_prep_last_error(nullptr)); }
  ~DevicePrep() { svnicp_prep_destroy(p_); }
  DevicePrep(const DevicePrep&) = delete;
  DevicePrep& operator=(const DevicePrep&) = delete;
  void scan(const Cloud& points, double min_range, double max_range, double voxel_size, double* scan_max_range) {
    if (svnicp_prep_scan(p_, points.empty() ? nullptr : &points[0][0], (int64_t)points.size(), SVNICP_MEM_HOST, min_range, max_range, voxel_size,
                         scan_max_range, &n_cropped, &n_map, &n_source) != 0)
      throw std::runtime_error(svnicp_prep_last_error(p_));
  }
  // deskew (OdometryPipeline.cpp:357-447) ahead of the same crop + samplings; stamps of SVNICP_STAMP_* type or nullptr
  void scan_deskew(const Cloud& points, const void* stamps, int stamp_type, const std::array<double, 6>& delta, bool kitti, double min_range,
                   double max_range, double voxel_size, double* scan_max_range) {
    if (svnicp_prep_scan_deskew(p_, points.empty() ? nullptr : &points[0][0], stamps, stamp_type, (int64_t)points.size(), SVNICP_MEM_HOST,
                                delta.data(), kitti ? SVNICP_DESKEW_KITTI : 0, min_range, max_range, voxel_size, scan_max_range, &n_cropped,
                                &n_map, &n_source) != 0)
      throw std::runtime_error(svnicp_prep_last_error(p_));
  }
  // range-image segmentation (ImageProjection::cloudHandler) -> number of points of the segmented cloud, kept in HBM
  int64_t segment(const Cloud& points, const svnicp_seg_params& prm) {
    int64_t n = 0;
    if (svnicp_prep_segment(p_, points.empty() ? nullptr : &points[0][0], (int64_t)points.size(), SVNICP_MEM_HOST, &prm, &n) != 0)
      throw std::runtime_error(svnicp_prep_last_error(p_));
    return n;
  }
  const float* segmented() { return svnicp_prep_segmented_devptr(p_); }
  // crop + samplings (or, with delta, deskew without stamps first) of a cloud already in HBM
  void scan_device(const float* xyz, int64_t n, const std::array<double, 6>* delta, bool kitti, double min_range, double max_range,
                   double voxel_size, double* scan_max_range) {
    const int rc = delta ? svnicp_prep_scan_deskew(p_, xyz, nullptr, SVNICP_STAMP_F64, n, SVNICP_MEM_DEVICE, delta->data(),
                                                   kitti ? SVNICP_DESKEW_KITTI : 0, min_range, max_range, voxel_size, scan_max_range,
                                                   &n_cropped, &n_map, &n_source)
                         : svnicp_prep_scan(p_, xyz, n, SVNICP_MEM_DEVICE, min_range, max_range, voxel_size, scan_max_range, &n_cropped,
                                            &n_map, &n_source);
    if (rc != 0) throw std::runtime_error(svnicp_prep_last_error(p_));
  }
  Cloud download_deskewed() {   // test tap
    int64_t n = 0;
    if (svnicp_prep_download_deskewed(p_, nullptr, 0, &n) != 0) throw std::runtime_error(svnicp_prep_last_error(p_));
    Cloud o((size_t)n);
    if (n && svnicp_prep_download_deskewed(p_, &o[0][0], n, &n) != 0) throw std::runtime_error(svnicp_prep_last_error(p_));
    return o;
  }
  const float* cropped() { return svnicp_prep_cropped_devptr(p_); }
  const float* map_cloud() { return svnicp_prep_map_cloud_devptr(p_); }
  const double* source() { return svnicp_prep_source_devptr(p_); }
  const float* source_f32() { return svnicp_prep_source_f32_devptr(p_); }
  std::vector<double> download_source() {   // test tap
    std::vector<float> f((size_t)3 * n_source);
    int64_t n = 0;
    if (n_source && svnicp_prep_download(p_, 2, f.data(), n_source, &n) != 0) throw std::runtime_error(svnicp_prep_last_error(p_));
    return std::vector<double>(f.begin(), f.end());
  }
  int64_t n_cropped = 0, n_map = 0, n_source = 0;

 private:
  svnicp_prep* p_ = nullptr;
};

// ------------------------------------------------------------------------------------------------ prediction
// OdometryPipeline::pose_prediction (:706-737): constant twist between the last two poses scaled by the time ratio;
// identity / last pose while fewer than two poses exist
inline Pose3 pose_prediction(const std::vector<Pose3>& poses, const std::vector<double>& times, double new_time) {
  if (poses.empty()) return Pose3{};
  if (poses.size() < 2) return poses.back();
  const Pose3& T0 = poses[poses.size() - 2];
  const Pose3& T1 = poses.back();
  const double dt = times.back() - times[times.size() - 2];
  const auto xi = se3_log(T0.inverse() * T1);
  const double ratio = (new_time - times.back()) / dt;
  double sx[6];
  for (int i = 0; i < 6; ++i) sx[i] = ratio * xi[i];
  return T1 * se3_exp(sx);
}

// ------------------------------------------------------------------------------------------------ the sequence
struct PipelineConfig {  // field names follow the node's parameters (OdometryPipeline.cpp parameter block; config/*.yaml)
  double min_range = 1.0, max_range = 100.0, voxel_size = 1.0;
  double map_voxel_size = 1.0, map_range = 100.0;
  int map_voxel_max_points = 20;
  int particle_count = 128;
  SteinICPParam solver;
  uint64_t seed = 0;
  int device = 0;
  bool gpu_map = false;  // keep the local map in HBM (DeviceVoxelMap): the target never crosses PCIe
  bool gpu_prep = false; // with gpu_map: crop and both uniform samplings on the device (DevicePrep): the raw scan is uploaded, no host pass over the points
  bool deskew = false;   // deskew_cloud (config/ICP_parameters.yaml:18): motion compensation ahead of the crop once two poses exist (:551-554)
  bool kitti = false;    // with deskew: the KITTI branch (cloud_topic "/kitti/velo/pointcloud", :385-401) instead of per-point stamps
  bool segmentation = false;   // USE_Segmentation (:180, :328-355): range-image segmentation of the raw scan first; the segmented
                               // cloud has no time field (:363-381), so per-point stamps are dropped (KITTI deskew still runs)
  svnicp_seg_params seg_params = seg_hdl64e_params();
  bool plane = false;          // the Huber-weighted point-to-plane residual (svnicp_set_residual; not in the reference)
  double huber_delta = 0.1;    // with plane: weight 1 up to this |r|, huber_delta / |r| beyond
  int normal_k = 16;           // with plane: neighbours a target normal is estimated from (4..64)
  bool gicp = false;           // the generalized-ICP residual (svnicp_set_residual_gicp; not in the reference): huber_delta and normal_k as
                               // with plane; the source's normals come from the solver's own pass over the source
  double gicp_epsilon = 1e-3;  // with gicp: a surface's covariance along its normal, in units of the in-plane one ([1e-6, 1])
  bool map_normals = false;    // with plane or gicp, and gpu_map: the target's normals come from the map's own voxels
                               // (DeviceVoxelMap::QueryNormals) instead of the solver's pass over the target
  double eval_dist = 0.0;      // > 0: every registered scan is evaluated at its result pose with this inlier gate
                               // (svnicp_evaluate) before the map update; 0 = off, no call is made
  std::string information = "off";   // "point" | "plane": after that evaluate, the Gauss-Newton information matrix of its pairs
                                     // (svnicp_eval_information) in ScanResult::information; needs eval_dist > 0.  "gicp": the same in
                                     // the generalized-ICP objective (svnicp_eval_information_gicp, with gicp_epsilon); only with
                                     // the gicp residual.  "off": no call
  double info_huber = HUGE_VAL;      // with information: its Huber delta (+inf = unweighted)
  double weight_dist = 0.0;    // > 0: every registration ends with one scoring of the particles at this gate and soft-min weights
                               // (svnicp_set_particle_weighting): correction, variance, cov and weights are the weighted figures
  double weight_temperature = 0.0;   // with weight_dist: the soft-min temperature in m^2, > 0
  std::string weight_cost = "point"; // with weight_dist: "point" = the mean truncated squared point distance (no call changes);
                                     // "solved" = the residual the registration runs with, plane or generalized-ICP, with the
                                     // solver's huber_delta and epsilon (svnicp_set_particle_weighting_objective)
  // mode_link_trans >= 0 (with mode_link_rot >= 0): after every registration the particles are grouped into modes
  // (svnicp_particle_modes) in ScanResult::modes; negative (the default) = off, no call is made
  double mode_link_trans = -1.0, mode_link_rot = -1.0;
  int mode_max = 8;                  // with the links: modes reported in full (1..SVNICP_MODES_MAX)
  bool mode_select_heaviest = false; // the correction is the first mode's mean instead of the global mean, and the pose, the
                                     // evaluate, the information and the map update follow it; needs the links
  // clear_seen_through: after every successful registration the map points the cropped scan sees through at the result pose are
  // dropped (ClearSeenThrough, sensor = seg_params) right before the map update, count in ScanResult::cleared; off: no call
  bool clear_seen_through = false;
  int clear_window_rows = 1, clear_window_cols = 1;         // the pixel window the minimum is taken over (0..4, 0..8)
  double clear_margin_abs = 0.3, clear_margin_rel = 0.02;   // m, ratio of the range
  double clear_max_range = 0.0;                             // map points farther than this from the sensor are left alone; 0 = max_range
  // seed_grid = (extent6, step6) of correction_grid: before every registration the scan's rows are scored against the map at the
  // grid's nodes around the prediction (ScorePoses), result in ScanResult::seed; empty (the default) = off, no call is made
  std::optional<std::pair<std::array<double, 6>, std::array<double, 6>>> seed_grid;
  double seed_gate = 0.0;           // with seed_grid: the inlier gate of that scoring, at most map_voxel_size; 0 = map_voxel_size
  std::string seed_mode = "best";   // "best": the initial mean becomes prediction * correction_to_pose(best node), the particles are
                                    // drawn as ever; "top": the mean stays the prediction, the particles are the particle_count best nodes
  int seed_levels = 1;              // with seed_grid: > 1 = coarse-to-fine (SearchPoses): seed_grid is level 0, every further level is three
                                    // times finer and expands the seed_keep best nodes of the one before; 1 = the flat grid
  int seed_keep = 8;                // with seed_levels > 1: nodes of a level that are expanded ("top": at least particle_count are kept)
  double seed_skip_fitness = 0.0;   // with seed_grid: > 0 = the prediction alone is scored first, and with inliers / rows at or above this
                                    // no search is made and the registration starts as without seeding; 0 = every scan is searched
  // prior_sigma = six standard deviations > 0 (m, m, m, rad, rad, rad): every registration runs with a Gaussian prior on the
  // correction (svnicp_set_pose_prior) centred on the registration's initial mean — the zero correction; with seed_mode "best"
  // that is the SEEDED mean, not the prediction — with information prior_point_sigma^2 diag(1 / sigma^2), and
  // ScanResult::prior_chi2 is filled; empty (the default) = off, no call is made
  std::optional<std::array<double, 6>> prior_sigma;
  double prior_point_sigma = 1.0;   // with prior_sigma: the point noise in m that turns the metric sigmas into the cost's units
};

struct ScanResult {
  double stamp = 0;
  Pose3 pose, initial_guess;
  bool aligned = false;
  int state = 0;
  std::array<double, 6> correction{}, variance{};
  std::vector<double> cov, particles, weights;
  int64_t with_normal = -1;   // cfg.map_normals: target rows the map gave a normal
  // cfg.eval_dist > 0: the result pose against the whole target (svnicp_evaluate); -1 = off, plane figures -1 without normals
  double fitness = -1, inlier_rmse = -1, plane_rmse = -1;
  int64_t plane_inliers = -1;
  std::optional<svnicp_information> information;   // cfg.information != "off": H, b, eigen-structure, rank, step, cov at the result pose
  std::optional<svnicp_modes> modes;               // cfg.mode_link_*: the modes of the final particle set, heaviest first
  int64_t cleared = -1;                            // cfg.clear_seen_through: map points the scan saw through and the map dropped
  double prior_chi2 = -1;                          // cfg.prior_sigma: e^T diag(1 / sigma^2) e of the returned correction (the prior's mean is
                                                   // the zero correction), the innovation statistic a gate would read; -1 = off
  struct Seed {
    size_t index = 0;                      // the best node
    double cost = 0, cost_zero = 0;        // its cost; the cost of the zero correction (the prediction)
    std::array<double, 6> correction{};    // the correction applied to the initial mean ("top": zeros)
    Pose3 prediction;                      // the constant-velocity prediction the grid is centred on
    std::vector<size_t> nodes;             // "top": the nodes handed over as particles, best first
    // cfg.seed_skip_fitness > 0: was the search made, and inliers / rows of the prediction alone (-1 where it was not computed)
    bool searched = true;
    double fitness_zero = -1;
    // cfg.seed_levels > 1 (index and nodes are unused then): the search's levels, the best node's lattice vector, the finest
    // step, the nodes scored, the best cost of level 0, and with "top" the lattice vectors handed over as particles
    int levels = 1;
    std::array<int32_t, 6> lattice{};
    std::array<double, 6> fine_step{};
    int64_t nodes_scored = 0;
    double cost_level0 = 0;
    Lattice node_lattice;
  };
  std::optional<Seed> seed;                        // cfg.seed_grid
};

// what the pipeline handed to the solver for one scan (test tap: the oracle is run on exactly these)
struct Tap {
  std::vector<double> source, target, particles;  // [B][3], [M][3], [6][P]
  Pose3 initial_guess;
};

// particle prior bounds, OdometryPipeline.cpp:661-667
constexpr double kPriorUb[6] = {0.3, 0.2, 0.1, 0.004, 0.004, 0.012};

class RegistrationPipeline {
 public:
  explicit RegistrationPipeline(const PipelineConfig& cfg)
      : cfg_(cfg), map_(cfg.map_voxel_size, cfg.map_range, cfg.map_voxel_max_points), rng_(cfg.seed * 0x9e3779b97f4a7c15ull + 0x2545f4914f6cdd1dull) {
    if (!(std::isfinite(cfg.weight_dist) && cfg.weight_dist >= 0)) throw std::invalid_argument("PipelineConfig: weight_dist must be finite and >= 0 (0 = equal weights)");
    if (cfg.weight_dist > 0 && !(std::isfinite(cfg.weight_temperature) && cfg.weight_temperature > 0))
      throw std::invalid_argument("PipelineConfig: weight_dist > 0 needs a finite weight_temperature > 0 (m^2)");
    if (cfg.weight_cost != "point" && cfg.weight_cost != "solved") throw std::invalid_argument("PipelineConfig: weight_cost must be \"point\" or \"solved\"");
    if (cfg.weight_cost != "point" && !(cfg.weight_dist > 0))
      throw std::invalid_argument("PipelineConfig: weight_cost \"solved\" needs weight_dist > 0 (it names the cost of that weighting)");
    if (cfg.information != "off" && cfg.information != "point" && cfg.information != "plane" && cfg.information != "gicp")
      throw std::invalid_argument("PipelineConfig: information must be \"off\", \"point\" or \"plane\"");
    if (cfg.information == "gicp" && !cfg.gicp && cfg.solver.residual != "gicp")
      throw std::invalid_argument("PipelineConfig: information \"gicp\" needs solver.residual == \"gicp\" (only then does the context hold the normals of both clouds)");
    if (cfg.information != "off" && !(cfg.eval_dist > 0)) throw std::invalid_argument("PipelineConfig: information needs eval_dist > 0 (its rows are the evaluate's)");
    if (cfg.information != "off" && !(cfg.info_huber > 0)) throw std::invalid_argument("PipelineConfig: info_huber must be > 0 (+inf = unweighted)");
    if (cfg.prior_sigma) {
      for (const double v : *cfg.prior_sigma)
        if (!(std::isfinite(v) && v > 0)) throw std::invalid_argument("PipelineConfig: prior_sigma must be six finite standard deviations > 0 (m, m, m, rad, rad, rad)");
      if (!(std::isfinite(cfg.prior_point_sigma) && cfg.prior_point_sigma > 0)) throw std::invalid_argument("PipelineConfig: prior_point_sigma must be finite and > 0 (m)");
    }
    if (cfg.map_normals && !cfg.gpu_map) throw std::invalid_argument("PipelineConfig: map_normals needs gpu_map (the normals are computed from the device map)");
    if (cfg.plane && cfg.gicp) throw std::invalid_argument("PipelineConfig: plane and gicp are two residuals, choose one");
    if (cfg.map_normals && !cfg.plane && !cfg.gicp) throw std::invalid_argument("PipelineConfig: map_normals needs plane or gicp (point mode uses no normals)");
    const bool mode_link = !(cfg.mode_link_trans < 0 && cfg.mode_link_rot < 0);
    if (mode_link && !(std::isfinite(cfg.mode_link_trans) && cfg.mode_link_trans >= 0 && std::isfinite(cfg.mode_link_rot) && cfg.mode_link_rot >= 0))
      throw std::invalid_argument("PipelineConfig: mode_link must be (link_trans, link_rot), both finite and >= 0");
    if (mode_link && !(cfg.mode_max >= 1 && cfg.mode_max <= SVNICP_MODES_MAX)) throw std::invalid_argument("PipelineConfig: mode_max must lie in 1..32");
    if (cfg.mode_select_heaviest && !mode_link) throw std::invalid_argument("PipelineConfig: mode_select \"heaviest\" needs mode_link (the modes are what it selects from)");
    if (cfg.seed_mode != "best" && cfg.seed_mode != "top") throw std::invalid_argument("PipelineConfig: seed_mode must be \"best\" or \"top\"");
    if (!(std::isfinite(cfg.seed_gate) && cfg.seed_gate >= 0 && cfg.seed_gate <= cfg.map_voxel_size))
      throw std::invalid_argument("PipelineConfig: seed_gate must be finite, >= 0 (0 = map_voxel_size) and at most map_voxel_size");
    if (cfg.seed_grid) {
      seed_nodes_ = correction_grid(cfg.seed_grid->first, cfg.seed_grid->second, &seed_zero_);   // throws for a bad grid
      if (cfg.seed_mode == "top" && cfg.seed_levels == 1 && seed_nodes_.size() < (size_t)cfg.particle_count)
        throw std::invalid_argument("PipelineConfig: seed_mode \"top\" needs at least particle_count nodes in seed_grid");
    }
    if (cfg.seed_levels < 1 || cfg.seed_levels > SVNICP_MAP_SEARCH_MAX_LEVELS) throw std::invalid_argument("PipelineConfig: seed_levels must lie in 1..8");
    if (cfg.seed_keep < 1 || cfg.seed_keep > SVNICP_MAP_SEARCH_MAX_KEEP) throw std::invalid_argument("PipelineConfig: seed_keep must lie in 1..1024");
    if (!(std::isfinite(cfg.seed_skip_fitness) && cfg.seed_skip_fitness >= 0 && cfg.seed_skip_fitness <= 1))
      throw std::invalid_argument("PipelineConfig: seed_skip_fitness must lie in [0, 1] (0 = every scan is searched)");
    if (!cfg.seed_grid && (cfg.seed_levels > 1 || cfg.seed_skip_fitness > 0))
      throw std::invalid_argument("PipelineConfig: seed_levels > 1 and seed_skip_fitness > 0 need seed_grid (level 0 of the search)");
    if (cfg.seed_grid && cfg.seed_levels > 1) {
      if (cfg.seed_mode == "top" && cfg.particle_count > SVNICP_MAP_SEARCH_MAX_KEEP)
        throw std::invalid_argument("PipelineConfig: seed_mode \"top\" with seed_levels > 1 hands over at most 1024 nodes (particle_count)");
      const SearchLattice L = search_lattice(cfg.seed_grid->first, cfg.seed_grid->second, cfg.seed_levels, seed_search_keep());   // throws
      if (cfg.seed_mode == "top" && L.count.back() < (int64_t)cfg.particle_count)
        throw std::invalid_argument("PipelineConfig: seed_mode \"top\" needs at least particle_count nodes in the last level of the search");
    }
    if (cfg.clear_seen_through) {
      clear_opt_ = svnicp_visibility_opt{(int32_t)sizeof(svnicp_visibility_opt), cfg.clear_window_rows, cfg.clear_window_cols, (float)cfg.clear_margin_abs,
                                         (float)cfg.clear_margin_rel, (float)(cfg.clear_max_range > 0 ? cfg.clear_max_range : cfg.max_range)};
      if (!(std::isfinite(cfg.clear_max_range) && cfg.clear_max_range >= 0)) throw std::invalid_argument("PipelineConfig: clear_max_range must be finite and >= 0 (0 = max_range)");
      VoxelHashMap(1.0, 1.0, 1).ClearSeenThrough(Cloud{}, Pose3{}, cfg.seg_params, clear_opt_);   // validates sensor and options (throws)
    }
    if (cfg.plane) { cfg_.solver.residual = "plane"; cfg_.solver.huber_delta = cfg.huber_delta; cfg_.solver.normal_k = cfg.normal_k; }
    if (cfg.gicp) { cfg_.solver.residual = "gicp"; cfg_.solver.huber_delta = cfg.huber_delta; cfg_.solver.normal_k = cfg.normal_k; cfg_.solver.gicp_epsilon = cfg.gicp_epsilon; }
    if (cfg.gpu_map) dmap_ = std::make_unique<DeviceVoxelMap>(cfg.map_voxel_size, cfg.map_range, cfg.map_voxel_max_points, cfg.device);
    if (cfg.gpu_map && cfg.gpu_prep) dprep_ = std::make_unique<DevicePrep>(cfg.device);
  }

  // replaces the built-in uniform prior sampler (svnicp::initialize_particles, ICPUtils.cpp:45-58): fills [6][P] row-major
  void set_particle_source(std::function<void(int, double*)> f) { particle_source_ = std::move(f); }
  void set_tap(Tap* t) { tap_ = t; }
  const VoxelHashMap& map() const { return map_; }
  size_t map_voxels() { return dmap_ ? dmap_->Size() : map_.Size(); }
  size_t bytes_h2d() const { return bytes_h2d_; }   // cloud bytes sent to the GPU so far (source scans + map traffic)
  const std::vector<Pose3>& poses() const { return poses_; }

  // one pass of ICP_processing's loop body for one LiDAR frame (points: n x 3 float32, sensor frame)
  ScanResult process_scan(const Cloud& points, double stamp) { return process(points, stamp, nullptr); }
  // ... with the scan's per-point time field (widened to double), used when cfg.deskew is set
  ScanResult process_scan(const Cloud& points, double stamp, const std::vector<double>& point_stamps) {
    return process(points, stamp, &point_stamps);
  }

 private:
  ScanResult process(const Cloud& points, double stamp, const std::vector<double>* point_stamps) {
    ScanResult res;
    res.stamp = stamp;
    Cloud cropped, to_map, source;
    const bool deskew = cfg_.deskew && poses_.size() >= 2;                                             // :552
    std::array<double, 6> delta{};
    if (deskew) delta = se3_log(poses_[poses_.size() - 2].inverse() * poses_.back());                  // :427-432
    if (cfg_.segmentation) point_stamps = nullptr;                                                     // segmentedCloud_: no time field
    if (dprep_ && cfg_.segmentation) {                                                                 // :331-343 on the device
      const int64_t n = dprep_->segment(points, cfg_.seg_params);
      bytes_h2d_ += points.size() * 12;
      dprep_->scan_device(dprep_->segmented(), n, deskew ? &delta : nullptr, cfg_.kitti, cfg_.min_range, cfg_.max_range, cfg_.voxel_size,
                          &scan_max_range_);
    } else if (dprep_) {
      if (deskew) {                                                                                    // :551-560 on the device
        const bool st = point_stamps && !cfg_.kitti;
        dprep_->scan_deskew(points, st ? point_stamps->data() : nullptr, SVNICP_STAMP_F64, delta, cfg_.kitti, cfg_.min_range, cfg_.max_range,
                            cfg_.voxel_size, &scan_max_range_);
        bytes_h2d_ += points.size() * 12 + (st ? point_stamps->size() * 8 : 0);
      } else {
        dprep_->scan(points, cfg_.min_range, cfg_.max_range, cfg_.voxel_size, &scan_max_range_);       // :556-560 on the device
        bytes_h2d_ += points.size() * 12;
      }
    } else {
      const Cloud segmented = cfg_.segmentation ? segment_scan(points, cfg_.seg_params) : Cloud{};     // :331-343
      const Cloud& raw = cfg_.segmentation ? segmented : points;
      const Cloud deskewed = deskew ? deskew_pointcloud(raw, point_stamps, delta, cfg_.kitti) : Cloud{};   // :553
      cropped = crop_pointcloud(deskew ? deskewed : raw, cfg_.min_range, cfg_.max_range, &scan_max_range_);   // :556
      to_map = downsample_uniform(cropped, 0.5 * cfg_.voxel_size);                                     // :559
      source = downsample_uniform(to_map, 1.5 * cfg_.voxel_size);                                      // :560
    }
    Pose3 guess = pose_prediction(poses_, times_, stamp);                                              // :563-564
    std::vector<double> init = sample_particles();                                                     // :573
    res.initial_guess = guess;
    if (dmap_ ? dmap_->Empty() : map_.Empty()) {                                                       // :585-593
      // the reference's downsample_uniform filters its input IN PLACE (:684-690): at :585 *cropped_cloud already holds the
      // 0.5-voxel sampling, and that is what seeds the map
      if (dprep_) dmap_->AddPointCloudDevice(dprep_->map_cloud(), dprep_->n_map, guess);
      else if (dmap_) { dmap_->AddPointCloud(to_map, guess); bytes_h2d_ += to_map.size() * 12; }
      else map_.AddPointCloud(to_map, guess);
      poses_.push_back(guess); times_.push_back(stamp);
      res.pose = guess;
      return res;
    }
    std::vector<double> src64;
    if (!dprep_) src64 = widen(source);                                                                // ICPUtils.cpp:27-43
    if (!solver_) solver_ = std::make_unique<SVNICP>(cfg_.solver, init, ParticleWeightOpt{cfg_.weight_dist > 0, cfg_.weight_dist, cfg_.weight_temperature, cfg_.weight_cost}, cfg_.device);
    bool search = (bool)cfg_.seed_grid;
    const double gate = cfg_.seed_gate > 0 ? cfg_.seed_gate : cfg_.map_voxel_size;
    double fitness_zero = -1;
    if (search && cfg_.seed_skip_fitness > 0) {   // the only policy: the prediction alone first (one pose, the same call)
      const std::vector<double> one = correction_poses(guess, {std::array<double, 6>{}});
      std::vector<double> rec;
      const int64_t n = dprep_ ? dprep_->n_source : (int64_t)source.size();
      if (dprep_) rec = dmap_->ScorePosesDevice(dprep_->source_f32(), dprep_->n_source, one, gate);
      else if (dmap_) { rec = dmap_->ScorePoses(source, one, gate); bytes_h2d_ += source.size() * 12; }
      else rec = map_.ScorePoses(source, one, gate);
      fitness_zero = n > 0 ? rec[1] / (double)n : 0.0;
      if (fitness_zero >= cfg_.seed_skip_fitness) {
        search = false;
        ScanResult::Seed sd;
        sd.searched = false; sd.fitness_zero = fitness_zero; sd.cost_zero = rec[3]; sd.prediction = guess;
        res.seed = sd;
      }
    }
    if (search && cfg_.seed_levels > 1) {   // coarse-to-fine: seed_grid is level 0
      const auto& [ext, stp] = *cfg_.seed_grid;
      const int keep = seed_search_keep();
      const int64_t n = dprep_ ? dprep_->n_source : (int64_t)source.size();
      MapSearchResult sr;
      if (dprep_) sr = dmap_->SearchPosesDevice(dprep_->source_f32(), dprep_->n_source, guess, ext, stp, cfg_.seed_levels, keep, gate);
      else if (dmap_) { sr = dmap_->SearchPoses(source, guess, ext, stp, cfg_.seed_levels, keep, gate); bytes_h2d_ += source.size() * 12; }
      else sr = map_.SearchPoses(source, guess, ext, stp, cfg_.seed_levels, keep, gate);
      ScanResult::Seed sd;
      sd.cost = sr.best_record[3]; sd.cost_zero = sr.zero_record[3]; sd.cost_level0 = sr.cost_level0; sd.prediction = guess;
      sd.levels = sr.levels; sd.lattice = sr.best_lattice; sd.fine_step = sr.fine_step; sd.nodes_scored = sr.nodes_scored;
      sd.fitness_zero = fitness_zero >= 0 ? fitness_zero : (n > 0 ? sr.zero_record[1] / (double)n : 0.0);
      if (cfg_.seed_mode == "top") {
        const int P = cfg_.particle_count;
        sd.node_lattice.assign(sr.top_lattice.begin(), sr.top_lattice.begin() + P);
        for (int d = 0; d < 6; ++d)
          for (int p = 0; p < P; ++p) init[(size_t)d * P + p] = sr.top_corrections[(size_t)p][d];
      } else {
        sd.correction = sr.best_correction;
        guess = guess * correction_to_pose(sd.correction);
        res.initial_guess = guess;
      }
      res.seed = sd;
    } else if (search) {   // the flat grid: every node is scored, and the best node is taken as it comes
      const std::vector<double> poses12 = correction_poses(guess, seed_nodes_);
      std::vector<double> scores;
      if (dprep_) scores = dmap_->ScorePosesDevice(dprep_->source_f32(), dprep_->n_source, poses12, gate);   // not uploaded again
      else if (dmap_) { scores = dmap_->ScorePoses(source, poses12, gate); bytes_h2d_ += source.size() * 12; }
      else scores = map_.ScorePoses(source, poses12, gate);
      const bool top = cfg_.seed_mode == "top";
      const std::vector<size_t> order = seed_from_scores(scores, top ? (size_t)cfg_.particle_count : 1);
      ScanResult::Seed sd;
      sd.index = order[0]; sd.cost = scores[4 * order[0] + 3]; sd.cost_zero = scores[4 * seed_zero_ + 3]; sd.prediction = guess;
      sd.fitness_zero = fitness_zero;
      if (top) {
        sd.nodes = order;
        const int P = cfg_.particle_count;
        for (int d = 0; d < 6; ++d)
          for (int p = 0; p < P; ++p) init[(size_t)d * P + p] = seed_nodes_[order[p]][d];
      } else {
        sd.correction = seed_nodes_[order[0]];
        guess = guess * correction_to_pose(sd.correction);
        res.initial_guess = guess;
      }
      res.seed = sd;
    }
    std::vector<double> tgt64;
    if (dmap_) {
      int64_t M = dmap_->GetMap(guess, scan_max_range_ + 10.0);                                        // :577-578
      if (M == 0) M = dmap_->GetMap();                                                                 // :579-581
      if (cfg_.map_normals) res.with_normal = dmap_->QueryNormals(cfg_.normal_k);
      if (dprep_) {
        solver_->add_cloud_device(dprep_->source(), dprep_->n_source, dmap_->points_devptr(), M, init.data(), cfg_.particle_count);
        if (tap_) src64 = dprep_->download_source();
      } else {
        solver_->add_cloud_device_target(src64.data(), (int64_t)source.size(), dmap_->points_devptr(), M, init.data(), cfg_.particle_count);
        bytes_h2d_ += src64.size() * 8;
      }
      if (cfg_.map_normals) solver_->set_target_normals_device(dmap_->normals_devptr(), M);   // right after the target they belong to
      if (tap_) tgt64 = dmap_->download();
    } else {
      Cloud target = map_.GetMap(guess, scan_max_range_ + 10.0);                                       // :577-578
      if (target.empty()) target = map_.GetMap();                                                      // :579-581
      tgt64 = widen(target);
      solver_->add_cloud(src64.data(), (int64_t)source.size(), tgt64.data(), (int64_t)target.size(), init.data(), cfg_.particle_count);  // :582
      bytes_h2d_ += (src64.size() + tgt64.size()) * 8;
    }
    if (cfg_.prior_sigma) {   // centred on the initial mean set below: the zero correction
      const double zero6[6] = {0, 0, 0, 0, 0, 0};
      double info[36] = {};
      for (int i = 0; i < 6; ++i) info[7 * i] = cfg_.prior_point_sigma * cfg_.prior_point_sigma / ((*cfg_.prior_sigma)[i] * (*cfg_.prior_sigma)[i]);
      solver_->set_pose_prior(zero6, info);
    }
    solver_->set_initial_mean(guess.R.data(), guess.t.data());                                         // :598
    if (tap_) { tap_->source = src64; tap_->target = tgt64; tap_->particles = init; tap_->initial_guess = guess; }
    res.state = (int)solver_->stein_align();                                                           // :599
    if (res.state != ALIGN_SUCCESS) { res.pose = guess; return res; }                                  // :599-601
    res.aligned = true;
    res.correction = solver_->get_transformation();                                                    // :602
    res.variance = solver_->get_distribution();
    res.cov = solver_->get_cov_matrix();
    res.particles = solver_->get_particles();
    res.weights = solver_->get_particle_weight();
    if (cfg_.mode_link_trans >= 0) {   // no policy here: "heaviest" is the caller's choice, made once in the configuration
      res.modes = solver_->particle_modes(cfg_.mode_link_trans, cfg_.mode_link_rot, cfg_.mode_max);
      const svnicp_modes& m = *res.modes;
      bool finite = m.n_reported > 0;
      for (int i = 0; i < 6; ++i) finite = finite && std::isfinite(m.mean[0][i]);
      if (cfg_.mode_select_heaviest && finite)
        for (int i = 0; i < 6; ++i) res.correction[i] = m.mean[0][i];
    }
    res.pose = guess * correction_to_pose(res.correction);                                             // updater_, :37-46
    if (cfg_.prior_sigma) {   // no policy here: the number a gate would read
      res.prior_chi2 = 0.0;
      for (int i = 0; i < 6; ++i) { const double z = res.correction[i] / (*cfg_.prior_sigma)[i]; res.prior_chi2 += z * z; }
    }
    if (cfg_.eval_dist > 0) {   // the number a caller may gate the map update on (no policy here)
      const svnicp_eval ev = solver_->evaluate(cfg_.eval_dist, res.pose.R.data(), res.pose.t.data());
      res.fitness = ev.fitness; res.inlier_rmse = ev.inlier_rmse;
      if (ev.has_normals) { res.plane_rmse = ev.plane_rmse; res.plane_inliers = ev.plane_inliers; }
      if (cfg_.information == "gicp")   // what a filter or a gate may read; no policy here either
        res.information = solver_->information_gicp(cfg_.info_huber, cfg_.solver.gicp_epsilon);
      else if (cfg_.information != "off")
        res.information = solver_->information(cfg_.information == "plane" ? SVNICP_INFO_PLANE : SVNICP_INFO_POINT, cfg_.info_huber);
    }
    if (cfg_.clear_seen_through) {   // no policy here either: every registered scan clears, with the densest cloud the step has
      if (dprep_) res.cleared = dmap_->ClearSeenThroughDevice(dprep_->cropped(), dprep_->n_cropped, res.pose, cfg_.seg_params, clear_opt_).points_removed;
      else if (dmap_) { res.cleared = dmap_->ClearSeenThrough(cropped, res.pose, cfg_.seg_params, clear_opt_).points_removed; bytes_h2d_ += cropped.size() * 12; }
      else res.cleared = map_.ClearSeenThrough(cropped, res.pose, cfg_.seg_params, clear_opt_).points_removed;
    }
    // … and at :630 *voxelized_cloud_toMap holds the 1.5-voxel sampling (the second in-place filter, :560): the map is updated
    // with the same points the solver registered
    if (dprep_) dmap_->AddPointCloudDevice(dprep_->source_f32(), dprep_->n_source, res.pose);          // :630
    else if (dmap_) { dmap_->AddPointCloud(source, res.pose); bytes_h2d_ += source.size() * 12; }
    else map_.AddPointCloud(source, res.pose);
    poses_.push_back(res.pose); times_.push_back(stamp);
    return res;
  }

  static std::vector<double> widen(const Cloud& c) {
    std::vector<double> o(3 * c.size());
    for (size_t i = 0; i < c.size(); ++i)
      for (int d = 0; d < 3; ++d) o[3 * i + d] = (double)c[i][d];
    return o;
  }
  std::vector<double> sample_particles() {
    const int P = cfg_.particle_count;
    std::vector<double> init((size_t)6 * P, 0.0);
    if (particle_source_) { particle_source_(P, init.data()); return init; }
    if (P == 1) return init;  // ICPUtils.cpp:49-50
    for (int d = 0; d < 6; ++d)
      for (int p = 0; p < P; ++p) init[(size_t)d * P + p] = (2.0 * uniform01() - 1.0) * kPriorUb[d];
    return init;
  }
  double uniform01() {  // splitmix64 -> 53-bit uniform
    uint64_t z = (rng_ += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
  }

  PipelineConfig cfg_;
  svnicp_visibility_opt clear_opt_{};
  // the `keep` of the coarse-to-fine search: "top" needs particle_count nodes out of the last level
  int seed_search_keep() const { return cfg_.seed_mode == "top" ? std::max(cfg_.seed_keep, cfg_.particle_count) : cfg_.seed_keep; }
  std::vector<std::array<double, 6>> seed_nodes_;   // cfg.seed_grid: the grid's nodes and the index of the zero correction
  size_t seed_zero_ = 0;
  VoxelHashMap map_;
  std::vector<Pose3> poses_;
  std::vector<double> times_;
  double scan_max_range_ = 0.0;
  uint64_t rng_;
  std::function<void(int, double*)> particle_source_;
  Tap* tap_ = nullptr;
  std::unique_ptr<SVNICP> solver_;
  std::unique_ptr<DeviceVoxelMap> dmap_;
  std::unique_ptr<DevicePrep> dprep_;
  size_t bytes_h2d_ = 0;
};

}  // namespace svnicp
