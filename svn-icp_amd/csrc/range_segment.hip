// range_segment.hip — range-image segmentation of a raw scan on the device (svnicp_prep_segment).
//
// LeGO-LOAM's ImageProjection::cloudHandler (/root/reference/svn-icp/include/segmentation/ImageProjection.h), which
// OdometryPipeline::lidar_msg_cb runs on each raw scan when USE_Segmentation is set (OdometryPipeline.cpp:328-355).  The
// contract is written out in include/svnicp_hip.h; the host restatements are pipeline.py / registration_pipeline.hpp
// (segment_scan), and the three agree bit for bit.  Every atan2f / sinf / cosf of the reference is the float64 function of the
// float32 operands rounded once (the documented deviation); everything else is IEEE + - * / sqrt, -ffp-contract=off.
//
// Kernels, all on the prep object's stream, one host synchronisation at the end:
//   k_seg_project  per point: finite check, row / column / range; atomicMax of the input index into the owner image, so the
//                  last point in input order wins whatever the schedule (projectPointCloud, :281-325).
//   k_seg_pixel    per pixel: range from the owner, the closed form of groundRemoval's overwrites (:329-374; it reads rows
//                  r-1..r+1 of the column), label init (:360-366), union-find parent and per-root statistics cleared.
//   k_seg_union    per label-0 pixel: the right (wrapping) and down edge predicates of labelComponents (:486-497) and a
//                  union by atomicMin on the parent image.  A parent only ever decreases and points into the same
//                  component, so once every union has finished each component has one root: its minimum pixel index, which
//                  is the row-major first pixel, the seed of the reference's BFS (:379-383).  Independent of scheduling.
//   k_seg_stats    per label-0 pixel: flatten (parent = root), size by atomicAdd, row mask of the non-root members by
//                  atomicOr (lineCountFlag is set on push only, :501: the seed's row counts only through another member).
//   k_seg_flags    per pixel: (valid root << 32) | keep — the validity test of :516-529 and the keep rule of :384-414.
//   exclusive scan of the packed flags (rocprim): the high half numbers the valid roots in seed order (label - 1), the low
//                  half is the output position.
//   k_seg_emit     per pixel: the final label, and the winning point's xyz and input index at its output position.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include <rocprim/device/device_scan.hpp>

#include "../../include/svnicp_hip.h"
#include "prep_state.hpp"
#include "range_project_device.hpp"

namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr float kEmptyRange = -100000.0f;   // rangeMat_ of an empty pixel (resetParameters)
constexpr int kInvalidLabel = 999999;       // :527

struct SegK {
  int N, H, G;
  float res_x, res_y, bottom, min_range, mount, theta;
  float sx, cx, sy, cy;   // sin / cos of segmentAlphaX / segmentAlphaY, float64 functions rounded once (host)
  int vpn, vln;
};

using svnicp::atan2_f32;   // range_project_device.hpp: the projection and its two float helpers, shared with map_visibility.hip
using svnicp::deg_f32;

__device__ __forceinline__ float point_range(const float* __restrict__ in, int o) {
  const float x = in[3 * (size_t)o], y = in[3 * (size_t)o + 1], z = in[3 * (size_t)o + 2];
  return sqrtf((x * x + y * y) + z * z);
}

__global__ __launch_bounds__(256) void k_seg_project(const float* __restrict__ in, int64_t n, SegK K, int* __restrict__ owner) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const svnicp::RangeSensor S{K.N, K.H, K.res_x, K.res_y, K.bottom, K.min_range};
  int row, col;
  float r;
  if (!svnicp::range_project(in[3 * i], in[3 * i + 1], in[3 * i + 2], S, row, col, r)) return;   // projectPointCloud (:281-325)
  atomicMax(&owner[row * K.H + col], (int)i);                            // the last point in input order wins
}

// groundRemoval's pair test: lower pixel owner a, upper pixel owner b, both filled
__device__ __forceinline__ bool flat_pair(const float* __restrict__ in, int a, int b, float mount) {
  const float dx = in[3 * (size_t)b] - in[3 * (size_t)a];
  const float dy = in[3 * (size_t)b + 1] - in[3 * (size_t)a + 1];
  const float dz = in[3 * (size_t)b + 2] - in[3 * (size_t)a + 2];
  const float ang = deg_f32(atan2_f32(dz, sqrtf(dx * dx + dy * dy)));
  return fabsf(ang - mount) <= 10.0f;
}

__global__ __launch_bounds__(256) void k_seg_pixel(const float* __restrict__ in, const int* __restrict__ owner, SegK K, float* __restrict__ range,
                                                   signed char* __restrict__ ground, int* __restrict__ label, int* __restrict__ parent,
                                                   int* __restrict__ size, unsigned* __restrict__ rows) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= K.N * K.H) return;
  const int r = p / K.H;
  const int o = owner[p];
  range[p] = o >= 0 ? point_range(in, o) : kEmptyRange;
  int g = 0;
  if (r <= K.G) {   // ground(r) = -1 if pair (r, r+1) is invalid, else 1 if pair (r, r+1) or (r-1, r) is flat, else 0
    bool up_invalid = false, flat = false;
    if (r < K.G) {
      const int ou = owner[p + K.H];
      if (o < 0 || ou < 0) up_invalid = true;
      else flat = flat_pair(in, o, ou, K.mount);
    }
    if (!up_invalid && !flat && r >= 1) {
      const int od = owner[p - K.H];
      if (o >= 0 && od >= 0) flat = flat_pair(in, od, o, K.mount);
    }
    g = up_invalid ? -1 : (flat ? 1 : 0);
  }
  ground[p] = (signed char)g;
  const int lab = (g == 1 || o < 0) ? -1 : 0;
  label[p] = lab;
  parent[p] = lab == 0 ? p : -1;
  size[p] = 0;
  rows[4 * p] = 0u; rows[4 * p + 1] = 0u; rows[4 * p + 2] = 0u; rows[4 * p + 3] = 0u;
}

__device__ __forceinline__ int load_parent(int* P, int x) { return __hip_atomic_load(&P[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int find_root(int* P, int x) {
  int y = load_parent(P, x);
  while (y != x) { x = y; y = load_parent(P, x); }
  return x;
}

// union with minimum-index roots: the larger root is hooked under the smaller one by atomicMin; a failed hook (the root had
// been hooked meanwhile) retries from the roots it now sees.  Parents only decrease and stay inside the component.
__device__ void unite(int* P, int a, int b) {
  a = find_root(P, a);
  b = find_root(P, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&P[a], b);
    if (old == a) return;
    a = find_root(P, old);
    b = find_root(P, b);
  }
}

// labelComponents' edge test (:486-497): atan2f(d2 * sin(alpha), d1 - d2 * cos(alpha)) > segmentTheta
__device__ __forceinline__ bool seg_link(float ra, float rb, float s, float c, float theta) {
  const float d1 = fmaxf(ra, rb), d2 = fminf(ra, rb);
  return atan2_f32(d2 * s, d1 - d2 * c) > theta;
}

__global__ __launch_bounds__(256) void k_seg_union(const float* __restrict__ range, const int* __restrict__ label, SegK K, int* parent) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= K.N * K.H || label[p] != 0) return;
  const int r = p / K.H, j = p - r * K.H;
  const float rp = range[p];
  const int qr = r * K.H + (j + 1 == K.H ? 0 : j + 1);                     // the image margin wraps (:479-482)
  if (qr != p && label[qr] == 0 && seg_link(rp, range[qr], K.sx, K.cx, K.theta)) unite(parent, p, qr);
  if (r + 1 < K.N) {
    const int qd = p + K.H;
    if (label[qd] == 0 && seg_link(rp, range[qd], K.sy, K.cy, K.theta)) unite(parent, p, qd);
  }
}

__global__ __launch_bounds__(256) void k_seg_stats(const int* __restrict__ label, SegK K, int* parent, int* __restrict__ size,
                                                   unsigned* __restrict__ rows) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= K.N * K.H || label[p] != 0) return;
  const int root = find_root(parent, p);
  __hip_atomic_store(&parent[p], root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  atomicAdd(&size[root], 1);
  if (p != root) {
    const int r = p / K.H;
    atomicOr(&rows[4 * root + (r >> 5)], 1u << (r & 31));
  }
}

__device__ __forceinline__ bool root_valid(const int* __restrict__ size, const unsigned* __restrict__ rows, int root, const SegK& K) {
  const int s = size[root];
  if (s >= 30) return true;
  if (s < K.vpn) return false;
  const int lines = __popc(rows[4 * root]) + __popc(rows[4 * root + 1]) + __popc(rows[4 * root + 2]) + __popc(rows[4 * root + 3]);
  return lines >= K.vln;
}

__global__ __launch_bounds__(256) void k_seg_flags(const int* __restrict__ label, const int* __restrict__ parent, const int* __restrict__ size,
                                                   const unsigned* __restrict__ rows, const signed char* __restrict__ ground, SegK K,
                                                   unsigned long long* __restrict__ flags) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= K.N * K.H) return;
  const int j = p % K.H;
  unsigned long long f = 0;
  if (label[p] == 0) {
    const int root = parent[p];
    const bool valid = root_valid(size, rows, root, K);
    f = valid ? 1ull : 0ull;                                                // a valid component's pixels are all kept
    if (valid && root == p) f |= 1ull << 32;
  } else if (ground[p] == 1) {                                              // most ground pixels are skipped (:400-403)
    f = (j % 5 != 0 && j > 5 && j < K.H - 5) ? 0ull : 1ull;
  }
  flags[p] = f;
}

__global__ __launch_bounds__(256) void k_seg_emit(const float* __restrict__ in, const int* __restrict__ owner, const int* __restrict__ parent,
                                                  const unsigned long long* __restrict__ flags, const unsigned long long* __restrict__ pre,
                                                  SegK K, int* __restrict__ label, float* __restrict__ out, int* __restrict__ out_index) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= K.N * K.H) return;
  if (label[p] == 0) {
    const int root = parent[p];
    label[p] = (flags[root] >> 32) ? 1 + (int)(pre[root] >> 32) : kInvalidLabel;   // labelCount_ starts at 1 (:95 of the reset)
  }
  if (flags[p] & 1ull) {
    const size_t k = (size_t)(pre[p] & 0xffffffffull);
    const int o = owner[p];
    out[3 * k] = in[3 * (size_t)o]; out[3 * k + 1] = in[3 * (size_t)o + 1]; out[3 * k + 2] = in[3 * (size_t)o + 2];
    out_index[k] = o;
  }
}

svnicp_seg_params make_params(int n, int h, float rx, float ry, float bottom, int g) {
  svnicp_seg_params s;
  s.struct_size = (int32_t)sizeof(svnicp_seg_params);
  s.n_scan = n; s.horizon_scan = h; s.ground_scan_ind = g;
  s.ang_res_x = rx; s.ang_res_y = ry; s.ang_bottom = bottom;
  s.min_range = 1.0f;                                    // sensorMinimumRange (:112)
  s.mount_angle = 0.0f;                                  // sensorMountAngle (:113)
  s.segment_theta = (float)(60.0 / 180.0 * kPi);         // segmentTheta (:114)
  s.valid_point_num = 5; s.valid_line_num = 3;           // (:115-116)
  return s;
}

}  // namespace

extern "C" {

int svnicp_seg_default_params(int sensor, svnicp_seg_params* out) {
  if (!out) return SVNICP_ERR_INVALID;
  switch (sensor) {   // ImageProjection.h:46-110, each value as the header's expression evaluates it
    case SVNICP_SEG_VLP16: *out = make_params(16, 1800, (float)0.2, (float)2.0, (float)(15.0 + 0.1), 7); break;
    case SVNICP_SEG_HDL32E: *out = make_params(32, 1800, (float)(360.0 / float(1800)), (float)(41.33 / float(32 - 1)), (float)30.67, 20); break;
    case SVNICP_SEG_HDL64E: *out = make_params(64, 2250, (float)(360.0 / float(2250)), (float)(26.8 / float(64 - 1)), (float)24.8, 7); break;
    case SVNICP_SEG_VLS128: *out = make_params(128, 1800, (float)0.2, (float)0.3, (float)25.0, 10); break;
    case SVNICP_SEG_RS32: *out = make_params(32, 2000, (float)0.18, 40 / static_cast<float>(32 - 1), (float)25.0, 2); break;
    case SVNICP_SEG_OS1_16: *out = make_params(16, 1024, (float)(360.0 / float(1024)), (float)(33.2 / float(16 - 1)), (float)(16.6 + 0.1), 7); break;
    case SVNICP_SEG_OS1_64: *out = make_params(64, 1024, (float)(360.0 / float(1024)), (float)(33.2 / float(64 - 1)), (float)(16.6 + 0.1), 15); break;
    case SVNICP_SEG_OS0_128: *out = make_params(128, 1024, (float)(360.0 / float(1024)), 90 / float(128 - 1), (float)(45 + 0.1), 11); break;
    default: return SVNICP_ERR_INVALID;
  }
  return SVNICP_OK;
}

int svnicp_prep_segment(svnicp_prep* p, const float* xyz, int64_t n, int mem_kind, const svnicp_seg_params* params, int64_t* n_segmented) {
  if (!p || !n_segmented || n < 0 || (n > 0 && !xyz) || n > 0x7fffffffLL)
    return fail(p, SVNICP_ERR_INVALID, "svnicp_prep_segment: bad argument");
  svnicp_seg_params prm;
  if (params) {
    if (params->struct_size != (int32_t)sizeof(svnicp_seg_params))
      return fail(p, SVNICP_ERR_INVALID, "svnicp_prep_segment: struct_size != sizeof(svnicp_seg_params)");
    prm = *params;
  } else {
    svnicp_seg_default_params(SVNICP_SEG_HDL64E, &prm);
  }
  if (!(prm.ground_scan_ind >= 1 && prm.ground_scan_ind < prm.n_scan && prm.n_scan <= 128))
    return fail(p, SVNICP_ERR_INVALID, "svnicp_prep_segment: need 1 <= ground_scan_ind < n_scan <= 128");
  if (!(prm.horizon_scan >= 1 && (int64_t)prm.n_scan * prm.horizon_scan <= (int64_t)1 << 19))
    return fail(p, SVNICP_ERR_INVALID, "svnicp_prep_segment: need horizon_scan >= 1 and n_scan * horizon_scan <= 2^19");
  if (!(std::isfinite(prm.ang_res_x) && prm.ang_res_x > 0.0f && std::isfinite(prm.ang_res_y) && prm.ang_res_y > 0.0f))
    return fail(p, SVNICP_ERR_INVALID, "svnicp_prep_segment: ang_res_x / ang_res_y must be finite and positive");
  if (!(std::isfinite(prm.ang_bottom) && std::isfinite(prm.min_range) && std::isfinite(prm.mount_angle) && std::isfinite(prm.segment_theta)))
    return fail(p, SVNICP_ERR_INVALID, "svnicp_prep_segment: ang_bottom / min_range / mount_angle / segment_theta must be finite");
  HIPCHK(p, hipSetDevice(p->device));
  auto& S = p->seg;
  S.n_out = 0;
  *n_segmented = 0;
  SegK K;
  K.N = prm.n_scan; K.H = prm.horizon_scan; K.G = prm.ground_scan_ind;
  K.res_x = prm.ang_res_x; K.res_y = prm.ang_res_y; K.bottom = prm.ang_bottom;
  K.min_range = prm.min_range; K.mount = prm.mount_angle; K.theta = prm.segment_theta;
  const float ax = (float)((double)prm.ang_res_x / 180.0 * kPi), ay = (float)((double)prm.ang_res_y / 180.0 * kPi);   // :119-120
  K.sx = (float)std::sin((double)ax); K.cx = (float)std::cos((double)ax);
  K.sy = (float)std::sin((double)ay); K.cy = (float)std::cos((double)ay);
  K.vpn = prm.valid_point_num; K.vln = prm.valid_line_num;
  const int64_t npix = (int64_t)K.N * K.H;
  S.n_pix = npix;
  const float* din = xyz;
  if (n > 0 && mem_kind != SVNICP_MEM_DEVICE) {
    HIPCHK(p, S.in.ensure((size_t)n * 3));
    HIPCHK(p, hipMemcpyAsync(S.in.p, xyz, (size_t)n * 12, hipMemcpyHostToDevice, p->stream));
    din = S.in.p;
  }
  const int64_t cap_out = n < npix ? n : npix;   // at most one point per pixel
  HIPCHK(p, S.xyz.ensure((size_t)(cap_out > 0 ? cap_out : 1) * 3)); HIPCHK(p, S.index.ensure((size_t)(cap_out > 0 ? cap_out : 1)));
  HIPCHK(p, S.owner.ensure((size_t)npix)); HIPCHK(p, S.parent.ensure((size_t)npix)); HIPCHK(p, S.size.ensure((size_t)npix));
  HIPCHK(p, S.range.ensure((size_t)npix)); HIPCHK(p, S.ground.ensure((size_t)npix)); HIPCHK(p, S.rows.ensure((size_t)npix * 4));
  HIPCHK(p, S.label.ensure((size_t)npix)); HIPCHK(p, S.flags.ensure((size_t)npix)); HIPCHK(p, S.pre.ensure((size_t)npix));
  HIPCHK(p, hipMemsetAsync(S.owner.p, 0xff, (size_t)npix * 4, p->stream));   // -1: empty
  if (n > 0) {
    hipLaunchKernelGGL(k_seg_project, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, p->stream, din, n, K, S.owner.p);
    HIPCHK(p, hipGetLastError());
  }
  const unsigned gp = (unsigned)((npix + 255) / 256);
  hipLaunchKernelGGL(k_seg_pixel, dim3(gp), dim3(256), 0, p->stream, din, S.owner.p, K, S.range.p, S.ground.p, S.label.p, S.parent.p,
                     S.size.p, S.rows.p);
  hipLaunchKernelGGL(k_seg_union, dim3(gp), dim3(256), 0, p->stream, S.range.p, S.label.p, K, S.parent.p);
  hipLaunchKernelGGL(k_seg_stats, dim3(gp), dim3(256), 0, p->stream, S.label.p, K, S.parent.p, S.size.p, S.rows.p);
  hipLaunchKernelGGL(k_seg_flags, dim3(gp), dim3(256), 0, p->stream, S.label.p, S.parent.p, S.size.p, S.rows.p, S.ground.p, K, S.flags.p);
  HIPCHK(p, hipGetLastError());
  size_t b = 0;
  HIPCHK(p, rocprim::exclusive_scan(nullptr, b, S.flags.p, S.pre.p, 0ull, (size_t)npix, rocprim::plus<unsigned long long>(), p->stream));
  HIPCHK(p, S.tmp.ensure(b));
  HIPCHK(p, rocprim::exclusive_scan(S.tmp.p, b, S.flags.p, S.pre.p, 0ull, (size_t)npix, rocprim::plus<unsigned long long>(), p->stream));
  hipLaunchKernelGGL(k_seg_emit, dim3(gp), dim3(256), 0, p->stream, din, S.owner.p, S.parent.p, S.flags.p, S.pre.p, K, S.label.p, S.xyz.p,
                     S.index.p);
  HIPCHK(p, hipGetLastError());
  unsigned long long last[2] = {0, 0};
  HIPCHK(p, hipMemcpyAsync(&last[0], S.pre.p + (npix - 1), 8, hipMemcpyDeviceToHost, p->stream));
  HIPCHK(p, hipMemcpyAsync(&last[1], S.flags.p + (npix - 1), 8, hipMemcpyDeviceToHost, p->stream));
  HIPCHK(p, hipStreamSynchronize(p->stream));   // the only host synchronisation: the cloud is complete when the call returns
  S.n_out = (int64_t)((last[0] + last[1]) & 0xffffffffull);
  *n_segmented = S.n_out;
  return SVNICP_OK;
}

const float* svnicp_prep_segmented_devptr(svnicp_prep* p) { return p ? p->seg.xyz.p : nullptr; }
const int32_t* svnicp_prep_segmented_index_devptr(svnicp_prep* p) { return p ? p->seg.index.p : nullptr; }

int svnicp_prep_download_segmented(svnicp_prep* p, float* out_xyz, int32_t* out_index, int64_t cap_points, int64_t* n_out) {
  if (!p || !n_out) return SVNICP_ERR_INVALID;
  HIPCHK(p, hipSetDevice(p->device));
  *n_out = p->seg.n_out;
  const int64_t n = p->seg.n_out < cap_points ? p->seg.n_out : cap_points;
  if (n > 0 && out_xyz) HIPCHK(p, hipMemcpyAsync(out_xyz, p->seg.xyz.p, (size_t)n * 12, hipMemcpyDeviceToHost, p->stream));
  if (n > 0 && out_index) HIPCHK(p, hipMemcpyAsync(out_index, p->seg.index.p, (size_t)n * 4, hipMemcpyDeviceToHost, p->stream));
  HIPCHK(p, hipStreamSynchronize(p->stream));
  return SVNICP_OK;
}

int svnicp_prep_download_seg_images(svnicp_prep* p, int32_t* owner, float* range, int8_t* ground, int32_t* label, int64_t cap_pixels) {
  if (!p) return SVNICP_ERR_INVALID;
  if (cap_pixels < p->seg.n_pix) return fail(p, SVNICP_ERR_INVALID, "svnicp_prep_download_seg_images: cap_pixels < n_scan * horizon_scan");
  HIPCHK(p, hipSetDevice(p->device));
  const size_t np = (size_t)p->seg.n_pix;
  if (np > 0) {
    if (owner) HIPCHK(p, hipMemcpyAsync(owner, p->seg.owner.p, np * 4, hipMemcpyDeviceToHost, p->stream));
    if (range) HIPCHK(p, hipMemcpyAsync(range, p->seg.range.p, np * 4, hipMemcpyDeviceToHost, p->stream));
    if (ground) HIPCHK(p, hipMemcpyAsync(ground, p->seg.ground.p, np, hipMemcpyDeviceToHost, p->stream));
    if (label) HIPCHK(p, hipMemcpyAsync(label, p->seg.label.p, np * 4, hipMemcpyDeviceToHost, p->stream));
  }
  HIPCHK(p, hipStreamSynchronize(p->stream));
  return SVNICP_OK;
}

}  // extern "C"
