// range_project_device.hpp — the range-image projection of one float32 point, stated once for the device.
//
// projectPointCloud of LeGO-LOAM's ImageProjection (include/segmentation/ImageProjection.h:281-325) as include/svnicp_hip.h
// writes it out: finite check, row from the elevation, column from the azimuth, range, minimum range.  k_seg_project
// (range_segment.hip) and the visibility kernels of the voxel map (map_visibility.hip) call this one function, so a map point and a
// scan point fall into a pixel by the same arithmetic.  Every atan2f is the float64 function of the float32 operands rounded
// once; everything else is IEEE + - * / sqrt under -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace svnicp {

struct RangeSensor {   // the fields of svnicp_seg_params the projection reads
  int N, H;            // n_scan, horizon_scan
  float res_x, res_y, bottom, min_range;
};

constexpr double kRangePi = 3.14159265358979323846;

// the project's atan2f: float64 atan2 of the float32 operands, rounded once
__device__ __forceinline__ float atan2_f32(float y, float x) { return (float)::atan2((double)y, (double)x); }
// float(double(a * 180.0f) / M_PI)
__device__ __forceinline__ float deg_f32(float a) { return (float)((double)(a * 180.0f) / kRangePi); }

// -> true when the point lands in the image: row in [0, N), col in [0, H), r its range (>= min_range)
__device__ __forceinline__ bool range_project(float x, float y, float z, const RangeSensor& S, int& row, int& col, float& r) {
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return false;           // removeNaNFromPointCloud (:240)
  const float va = deg_f32(atan2_f32(z, sqrtf(x * x + y * y)));
  const float q = (va + S.bottom) / S.res_y;
  if (!(q > -1.0f && q < (float)S.N)) return false;                         // size_t conversion: (-1, 0) is row 0 (x86-64)
  row = (int)q;
  const float h = deg_f32(atan2_f32(x, y));
  double c = -round(((double)h - 90.0) / (double)S.res_x) + (double)(S.H / 2);
  if (c >= (double)S.H) c -= (double)S.H;
  if (!(c >= 0.0 && c < (double)S.H)) return false;                         // negative: wraps in size_t, dropped
  col = (int)c;
  r = sqrtf((x * x + y * y) + z * z);
  return !(r < S.min_range);
}

}  // namespace svnicp
