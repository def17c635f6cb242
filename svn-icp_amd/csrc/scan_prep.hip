// scan_prep.hip — the per-scan pre-processing of the scan-to-map loop, on the device.
//
// what OdometryPipeline::ICP_processing does to a scan before the solver sees it
// (/root/reference/svn-icp/src/core/OdometryPipeline.cpp):
//   crop_pointcloud      (:692-704)  keep min_range² < |p|² < max_range²; scan_max_range_ = largest SQUARED norm seen (:699)
//   uniform down-sample  (:684-690)  pcl::UniformSampling, leaf 0.5·voxel  -> the cloud that goes into the local map (:559)
//   uniform down-sample              leaf 1.5·voxel of THAT cloud          -> the source cloud of the registration (:560)
// The reference runs these with PCL on the host and uploads the results; here the raw float32 scan is uploaded once and the
// three clouds stay in HBM: the cropped and map clouds feed svnicp_map_add_cloud(…, SVNICP_MEM_DEVICE), the source cloud
// (float64 rows) feeds svnicp_set_source(…, SVNICP_MEM_DEVICE).
//
// UniformSampling as restated in svn-icp_amd/host/registration_pipeline.hpp (the cross-check of the tests): a grid of leaf
// size r anchored at floor(min/r); per occupied leaf the point closest to the leaf centre survives, the first one in input
// order on ties; leaves are emitted in ascending linear index.  Device form: leaf keys -> stable radix sort of (leaf, input
// index) -> runs; per run the smallest squared distance (64-bit atomicMin on the bits of a non-negative double), then the
// lowest sorted position among the points that attain it (stable sort: lowest input index) — the same winner as the
// sequential loop, independent of scheduling.  Same arithmetic, same order of additions as the host code (float32 points
// widened to float64).  HBM-bound integer/byte work; nothing here touches the matrix pipe.
//
// Deskew (svnicp_prep_scan_deskew): OdometryPipeline::deskew_pointcloud (:357-447), which the reference runs ahead of the crop
// when deskew_cloud_ is set and the pose buffer holds two poses (:551-554).  k_deskew_stamps widens the per-point stamps
// (uint32 / float32 / float64, :372-381, :403-413) to double — or, in KITTI mode (:385-401), rotates each point by 0.205° about
// (p × ẑ).normalized() into scratch and derives its stamp from the yaw — and reduces min / max over the FINITE stamps (one
// pair of atomics per workgroup, enc_f64).  k_deskew_crop replaces k_prep_crop on this path: per point s = (t − min)/(max − min)
// (:419-423), Pose3::Expmap((s − 0.5)·δ).transformFrom(p) in float64 (:436-445), rounded once to float32 into the kept
// deskewed buffer (min == max: the raw point, :418), then k_prep_crop's predicate and squared-norm maximum.  The expressions
// are those of registration_pipeline.hpp (se3_exp, deskew_pointcloud, kitti_correct_and_stamp) and pipeline.py, in the same
// order; only sin / cos / atan2 may differ from the host libm in the last bit.  After it, the exclusive scan, k_prep_compact
// and the two samplings run as in svnicp_prep_scan, on the deskewed points.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "../../include/svnicp_hip.h"
#include "kernels.hpp"
#include "prep_state.hpp"

namespace {


__device__ __forceinline__ unsigned long long enc_f64(double v) {   // order-preserving double -> uint64
  const long long b = __double_as_longlong(v);
  return b < 0 ? ~(unsigned long long)b : ((unsigned long long)b | 0x8000000000000000ull);
}
__device__ __forceinline__ double dec_f64(unsigned long long e) {
  const unsigned long long b = (e & 0x8000000000000000ull) ? (e & 0x7fffffffffffffffull) : ~e;
  return __longlong_as_double((long long)b);
}

// crop: keep flag per point, largest squared norm of ALL points (one atomic per workgroup)
__global__ __launch_bounds__(256) void k_prep_crop(const float* __restrict__ in, int64_t n, double min2, double max2, int* __restrict__ keep,
                                                   unsigned long long* __restrict__ max_n2) {
  __shared__ double s_m[4];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double n2 = -1.0;
  if (i < n) {
    const float x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
    n2 = (double)((x * x + y * y) + z * z);           // float32, left to right, as pt.x*pt.x + pt.y*pt.y + pt.z*pt.z of
                                                      // OdometryPipeline.cpp:698 (this library is built with -ffp-contract=off)
    keep[i] = (n2 < max2 && n2 > min2) ? 1 : 0;
    if (!(n2 == n2)) n2 = -1.0;                       // a NaN point is dropped and does not count for the range
  }
  double m = n2;
  for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
  if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmax(fmax(s_m[0], s_m[1]), fmax(s_m[2], s_m[3]));
    if (m >= 0.0) atomicMax(max_n2, enc_f64(m));
  }
}

__global__ __launch_bounds__(256) void k_prep_compact(const float* __restrict__ in, int64_t n, const int* __restrict__ keep, const int* __restrict__ off,
                                                      float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !keep[i]) return;
  const size_t o = (size_t)off[i] * 3;
  out[o] = in[3 * i]; out[o + 1] = in[3 * i + 1]; out[o + 2] = in[3 * i + 2];
}

// grid bounds of a cloud: min / max of floor(p / leaf) per axis; bounds[0..2] = min, [3..5] = max (as long long)
__global__ __launch_bounds__(256) void k_ds_bounds(const float* __restrict__ in, int64_t n, double inv, long long* __restrict__ bounds) {
  __shared__ long long s_lo[4][3], s_hi[4][3];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  long long lo[3] = {INT64_MAX, INT64_MAX, INT64_MAX}, hi[3] = {INT64_MIN, INT64_MIN, INT64_MIN};
  if (i < n) {
#pragma unroll
    for (int d = 0; d < 3; ++d) { const long long c = (long long)floor((double)in[3 * i + d] * inv); lo[d] = c; hi[d] = c; }
  }
#pragma unroll
  for (int d = 0; d < 3; ++d)
    for (int off = 32; off > 0; off >>= 1) {
      const long long a = __shfl_xor(lo[d], off, 64), b = __shfl_xor(hi[d], off, 64);
      lo[d] = a < lo[d] ? a : lo[d]; hi[d] = b > hi[d] ? b : hi[d];
    }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int d = 0; d < 3; ++d) { s_lo[wave][d] = lo[d]; s_hi[wave][d] = hi[d]; }
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int d = threadIdx.x;
    long long l = s_lo[0][d], h = s_hi[0][d];
    for (int w = 1; w < 4; ++w) { l = s_lo[w][d] < l ? s_lo[w][d] : l; h = s_hi[w][d] > h ? s_hi[w][d] : h; }
    if (l <= h) { atomicMin(&bounds[d], l); atomicMax(&bounds[3 + d], h); }
  }
}

// leaf key, squared distance to the leaf centre, input index
__global__ __launch_bounds__(256) void k_ds_keys(const float* __restrict__ in, int64_t n, double radius, double inv, const long long* __restrict__ bounds,
                                                 unsigned long long* __restrict__ key, unsigned long long* __restrict__ d2bits, int* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long long dx = bounds[3] - bounds[0] + 1, dy = bounds[4] - bounds[1] + 1;
  long long ijk[3];
  double d2 = 0.0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {   // registration_pipeline.hpp: downsample_uniform, same expressions
    const double v = (double)in[3 * i + d];
    ijk[d] = (long long)floor(v * inv) - bounds[d];
    const double c = ((double)(ijk[d] + bounds[d]) + 0.5) * radius;
    d2 += (v - c) * (v - c);
  }
  key[i] = (unsigned long long)(ijk[0] + ijk[1] * dx + ijk[2] * dx * dy);
  d2bits[i] = (unsigned long long)__double_as_longlong(d2);   // d2 >= 0 (or NaN): the bit pattern orders like the value
  idx[i] = (int)i;
}

__global__ __launch_bounds__(256) void k_ds_run_flags(const unsigned long long* __restrict__ skey, int64_t n, int* __restrict__ flag) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) flag[j] = (j == 0 || skey[j] != skey[j - 1]) ? 1 : 0;
}

// run id of sorted position j = (exclusive prefix of the flags) + flag - 1
__global__ __launch_bounds__(256) void k_ds_min_d2(const int* __restrict__ flag, const int* __restrict__ pre, const int* __restrict__ sidx,
                                                   const unsigned long long* __restrict__ d2bits, int64_t n, unsigned long long* __restrict__ run_min) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) atomicMin(&run_min[pre[j] + flag[j] - 1], d2bits[sidx[j]]);
}
__global__ __launch_bounds__(256) void k_ds_min_pos(const int* __restrict__ flag, const int* __restrict__ pre, const int* __restrict__ sidx,
                                                    const unsigned long long* __restrict__ d2bits, int64_t n,
                                                    const unsigned long long* __restrict__ run_min, int* __restrict__ run_pos) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int r = pre[j] + flag[j] - 1;
  if (d2bits[sidx[j]] == run_min[r]) atomicMin(&run_pos[r], (int)j);
}
__global__ __launch_bounds__(256) void k_ds_gather(const float* __restrict__ in, const int* __restrict__ sidx, const int* __restrict__ run_pos, int runs,
                                                   float* __restrict__ out, double* __restrict__ out64) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= runs) return;
  const int p = run_pos[r];
  const int i = sidx[p];
  const float x = in[3 * (size_t)i], y = in[3 * (size_t)i + 1], z = in[3 * (size_t)i + 2];
  out[3 * (size_t)r] = x; out[3 * (size_t)r + 1] = y; out[3 * (size_t)r + 2] = z;
  if (out64) { out64[3 * (size_t)r] = (double)x; out64[3 * (size_t)r + 1] = (double)y; out64[3 * (size_t)r + 2] = (double)z; }   // ICPUtils.cpp:27-43
}

// ---- deskew (OdometryPipeline.cpp:357-447)
struct Twist { double v[6]; };   // delta_xi = Pose3::Logmap(start^-1 * finish), [omega, v]

// registration_pipeline.hpp: se3_exp (Pose3::Expmap) followed by transformFrom, row-major R, each row summed left to right
__device__ __forceinline__ void se3_exp_apply(const double xi[6], double px, double py, double pz, float* q) {
  const double w0 = xi[0], w1 = xi[1], w2 = xi[2];
  const double th = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
  const double K[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
  double K2[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) K2[3 * i + j] = K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j];
  double ra, rb, vb, vc;
  if (th < 1e-10) { ra = 1.0; rb = 0.5; vb = 0.5; vc = 0.0; }
  else {
    const double sn = sin(th), cs = cos(th);
    ra = sn / th; rb = (1.0 - cs) / (th * th); vb = (1.0 - cs) / (th * th); vc = (th - sn) / (th * th * th);
  }
  double R[9], V[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) { R[i] = ra * K[i] + rb * K2[i]; V[i] = vb * K[i] + vc * K2[i]; }
  R[0] += 1.0; R[4] += 1.0; R[8] += 1.0; V[0] += 1.0; V[4] += 1.0; V[8] += 1.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double t = V[3 * i] * xi[3] + V[3 * i + 1] * xi[4] + V[3 * i + 2] * xi[5];
    q[i] = (float)(((R[3 * i] * px + R[3 * i + 1] * py) + R[3 * i + 2] * pz) + t);
  }
}

// stamps widened to double (KITTI: corrected point into kpts + its stamp); max of enc(t) -> dscal[1], max of ~enc(t) (the
// minimum) -> dscal[2], finite stamps only; 0 = nothing seen (enc of a non-NaN double is neither 0 nor ~0)
__global__ __launch_bounds__(256) void k_deskew_stamps(const float* __restrict__ in, const void* __restrict__ stamps, int type, int kitti,
                                                       double ksin, double kcos, int64_t n, float* __restrict__ kpts, double* __restrict__ st,
                                                       unsigned long long* __restrict__ dscal) {
  __shared__ unsigned long long s_hi[4], s_lo[4];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long hi = 0, lo = 0;
  if (i < n) {
    double t;
    if (kitti) {   // :385-401, the expressions of kitti_correct_and_stamp (AngleAxis::toRotationMatrix of Eigen 3; unpinned)
      const double x = (double)in[3 * i], y = (double)in[3 * i + 1], z = (double)in[3 * i + 2];
      double ax = y, ay = -x;
      const double az = 0.0;
      const double nn = (ax * ax + ay * ay) + az * az;
      if (nn > 0.0) { const double r = sqrt(nn); ax = ax / r; ay = ay / r; }   // Eigen normalized(): a zero vector stays zero
      const double sx = ksin * ax, sy = ksin * ay, sz = ksin * az;
      const double cx = (1.0 - kcos) * ax, cy = (1.0 - kcos) * ay, cz = (1.0 - kcos) * az;
      const double R[9] = {cx * ax + kcos, cx * ay - sz, cx * az + sy, cx * ay + sz, cy * ay + kcos, cy * az - sx, cx * az - sy, cy * az + sx,
                           cz * az + kcos};
      float q[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) q[d] = (float)((R[3 * d] * x + R[3 * d + 1] * y) + R[3 * d + 2] * z);
      kpts[3 * i] = q[0]; kpts[3 * i + 1] = q[1]; kpts[3 * i + 2] = q[2];
      const float yaw = (float)(-atan2((double)q[1], (double)q[0]));   // the float yaw of :397, correctly rounded
      t = 0.5 * ((double)yaw / 3.14159265358979323846 + 1.0);
    } else if (type == SVNICP_STAMP_F64) {
      t = static_cast<const double*>(stamps)[i];
    } else if (type == SVNICP_STAMP_F32) {
      t = (double)static_cast<const float*>(stamps)[i];
    } else {
      t = (double)static_cast<const uint32_t*>(stamps)[i];
    }
    st[i] = t;
    if (isfinite(t)) { hi = enc_f64(t); lo = ~hi; }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long a = __shfl_xor(hi, off, 64), b = __shfl_xor(lo, off, 64);
    hi = a > hi ? a : hi; lo = b > lo ? b : lo;
  }
  if ((threadIdx.x & 63) == 0) { s_hi[threadIdx.x >> 6] = hi; s_lo[threadIdx.x >> 6] = lo; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) { hi = s_hi[w] > hi ? s_hi[w] : hi; lo = s_lo[w] > lo ? s_lo[w] : lo; }
    if (hi) atomicMax(&dscal[1], hi);
    if (lo) atomicMax(&dscal[2], lo);
  }
}

// deskewed point -> out (kept), then k_prep_crop's predicate and squared-norm maximum (dscal[0]) on it
__global__ __launch_bounds__(256) void k_deskew_crop(const float* __restrict__ in, const float* __restrict__ kpts, const double* __restrict__ st,
                                                     int64_t n, Twist delta, double min2, double max2, float* __restrict__ out,
                                                     int* __restrict__ keep, unsigned long long* dscal) {
  __shared__ double s_m[4];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double n2 = -1.0;
  if (i < n) {
    const unsigned long long hi = dscal[1], lo = dscal[2];   // written by the previous launch
    const double tmax = dec_f64(hi), tmin = dec_f64(~lo);
    float q[3];
    if (hi == 0 || tmin == tmax) {                          // no (finite) stamps, or min == max: *frame, the raw point (:418)
      q[0] = in[3 * i]; q[1] = in[3 * i + 1]; q[2] = in[3 * i + 2];
    } else {
      const double t = st[i];
      if (!isfinite(t)) {                                   // deliberate deviation (header): a point without a valid stamp is NaN
        q[0] = q[1] = q[2] = __builtin_nanf("");
      } else {
        const float* src = kpts ? kpts : in;                // KITTI: the corrected copy (frame_points, :361, :392-394)
        const double sp = (t - tmin) / (tmax - tmin) - 0.5;   // :419-423, then (s - 0.5) of :439
        double xi[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) xi[k] = sp * delta.v[k];
        se3_exp_apply(xi, (double)src[3 * i], (double)src[3 * i + 1], (double)src[3 * i + 2], q);
      }
    }
    out[3 * i] = q[0]; out[3 * i + 1] = q[1]; out[3 * i + 2] = q[2];
    const float x = q[0], y = q[1], z = q[2];
    n2 = (double)((x * x + y * y) + z * z);           // k_prep_crop's arithmetic (OdometryPipeline.cpp:698)
    keep[i] = (n2 < max2 && n2 > min2) ? 1 : 0;
    if (!(n2 == n2)) n2 = -1.0;
  }
  double m = n2;
  for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
  if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmax(fmax(s_m[0], s_m[1]), fmax(s_m[2], s_m[3]));
    if (m >= 0.0) atomicMax(&dscal[0], enc_f64(m));
  }
}

// out (+ out64) = UniformSampling(in[0..n), radius); *n_out = number of occupied leaves
int downsample(svnicp_prep* p, const float* in, int64_t n, double radius, GrowBuf<float>& out, GrowBuf<double>* out64, int64_t* n_out) {
  *n_out = 0;
  if (n <= 0) return SVNICP_OK;
  if (!(radius > 0.0)) {   // the host code returns the cloud unchanged
    HIPCHK(p, out.ensure((size_t)n * 3));
    HIPCHK(p, hipMemcpyAsync(out.p, in, (size_t)n * 12, hipMemcpyDeviceToDevice, p->stream));
    *n_out = n;
    return SVNICP_OK;
  }
  const double inv = 1.0 / radius;
  const unsigned g = (unsigned)((n + 255) / 256);
  HIPCHK(p, p->key.ensure((size_t)n)); HIPCHK(p, p->skey.ensure((size_t)n)); HIPCHK(p, p->d2bits.ensure((size_t)n));
  HIPCHK(p, p->idx.ensure((size_t)n)); HIPCHK(p, p->sidx.ensure((size_t)n)); HIPCHK(p, p->flag.ensure((size_t)n)); HIPCHK(p, p->pre.ensure((size_t)n));
  HIPCHK(p, p->run_min.ensure((size_t)n)); HIPCHK(p, p->run_pos.ensure((size_t)n));
  long long* bounds = reinterpret_cast<long long*>(p->scal.p + 1);
  const long long init_b[6] = {INT64_MAX, INT64_MAX, INT64_MAX, INT64_MIN, INT64_MIN, INT64_MIN};
  HIPCHK(p, hipMemcpyAsync(bounds, init_b, sizeof init_b, hipMemcpyHostToDevice, p->stream));
  hipLaunchKernelGGL(k_ds_bounds, dim3(g), dim3(256), 0, p->stream, in, n, inv, bounds);
  hipLaunchKernelGGL(k_ds_keys, dim3(g), dim3(256), 0, p->stream, in, n, radius, inv, bounds, p->key.p, p->d2bits.p, p->idx.p);
  HIPCHK(p, hipGetLastError());
  size_t b1 = 0, b2 = 0;
  HIPCHK(p, rocprim::radix_sort_pairs(nullptr, b1, p->key.p, p->skey.p, p->idx.p, p->sidx.p, (size_t)n, 0, 64, p->stream));
  HIPCHK(p, rocprim::exclusive_scan(nullptr, b2, p->flag.p, p->pre.p, 0, (size_t)n, rocprim::plus<int>(), p->stream));
  HIPCHK(p, p->tmp.ensure(b1 > b2 ? b1 : b2));
  HIPCHK(p, rocprim::radix_sort_pairs(p->tmp.p, b1, p->key.p, p->skey.p, p->idx.p, p->sidx.p, (size_t)n, 0, 64, p->stream));   // stable
  hipLaunchKernelGGL(k_ds_run_flags, dim3(g), dim3(256), 0, p->stream, p->skey.p, n, p->flag.p);
  HIPCHK(p, hipGetLastError());
  HIPCHK(p, rocprim::exclusive_scan(p->tmp.p, b2, p->flag.p, p->pre.p, 0, (size_t)n, rocprim::plus<int>(), p->stream));
  HIPCHK(p, hipMemsetAsync(p->run_min.p, 0xff, (size_t)n * 8, p->stream));
  HIPCHK(p, hipMemsetAsync(p->run_pos.p, 0x7f, (size_t)n * 4, p->stream));
  hipLaunchKernelGGL(k_ds_min_d2, dim3(g), dim3(256), 0, p->stream, p->flag.p, p->pre.p, p->sidx.p, p->d2bits.p, n, p->run_min.p);
  hipLaunchKernelGGL(k_ds_min_pos, dim3(g), dim3(256), 0, p->stream, p->flag.p, p->pre.p, p->sidx.p, p->d2bits.p, n, p->run_min.p, p->run_pos.p);
  HIPCHK(p, hipGetLastError());
  int last[2] = {0, 0};
  HIPCHK(p, hipMemcpyAsync(&last[0], p->pre.p + (n - 1), sizeof(int), hipMemcpyDeviceToHost, p->stream));
  HIPCHK(p, hipMemcpyAsync(&last[1], p->flag.p + (n - 1), sizeof(int), hipMemcpyDeviceToHost, p->stream));
  HIPCHK(p, hipStreamSynchronize(p->stream));
  const int runs = last[0] + last[1];
  HIPCHK(p, out.ensure((size_t)runs * 3));
  if (out64) HIPCHK(p, out64->ensure((size_t)runs * 3));
  hipLaunchKernelGGL(k_ds_gather, dim3((unsigned)((runs + 255) / 256)), dim3(256), 0, p->stream, in, p->sidx.p, p->run_pos.p, runs, out.p,
                     out64 ? out64->p : (double*)nullptr);
  HIPCHK(p, hipGetLastError());
  *n_out = runs;
  return SVNICP_OK;
}

// the common tail of svnicp_prep_scan and svnicp_prep_scan_deskew: compact the kept points of in[0..n) (p->keep, written by the
// crop kernel, which also left the largest squared norm, encoded, in scal[0]) and run the two uniform samplings (:559-560)
int compact_and_sample(svnicp_prep* p, const char* who, const float* in, int64_t n, const unsigned long long* scal, double voxel_size,
                       double* scan_max_range, int64_t* n_cropped, int64_t* n_map, int64_t* n_source) {
  size_t b = 0;
  HIPCHK(p, rocprim::exclusive_scan(nullptr, b, p->keep.p, p->off.p, 0, (size_t)n, rocprim::plus<int>(), p->stream));
  HIPCHK(p, p->tmp.ensure(b));
  HIPCHK(p, rocprim::exclusive_scan(p->tmp.p, b, p->keep.p, p->off.p, 0, (size_t)n, rocprim::plus<int>(), p->stream));
  int last[2] = {0, 0};
  unsigned long long enc = 0;
  HIPCHK(p, hipMemcpyAsync(&last[0], p->off.p + (n - 1), sizeof(int), hipMemcpyDeviceToHost, p->stream));
  HIPCHK(p, hipMemcpyAsync(&last[1], p->keep.p + (n - 1), sizeof(int), hipMemcpyDeviceToHost, p->stream));
  HIPCHK(p, hipMemcpyAsync(&enc, scal, 8, hipMemcpyDeviceToHost, p->stream));
  HIPCHK(p, hipStreamSynchronize(p->stream));   // the only host synchronisation before the samplings
  if (enc) {
    const unsigned long long bits = (enc & 0x8000000000000000ull) ? (enc & 0x7fffffffffffffffull) : ~enc;
    double m;
    std::memcpy(&m, &bits, 8);
    if (m > *scan_max_range) *scan_max_range = m;       // :699 (a squared norm, kept as the reference keeps it; deskewed cloud: :556)
  }
  const int64_t nc = (int64_t)last[0] + last[1];
  HIPCHK(p, p->cropped.ensure((size_t)(nc > 0 ? nc : 1) * 3));
  hipLaunchKernelGGL(k_prep_compact, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, p->stream, in, n, p->keep.p, p->off.p, p->cropped.p);
  HIPCHK(p, hipGetLastError());
  p->n_cropped = nc;
  int rc = downsample(p, p->cropped.p, nc, 0.5 * voxel_size, p->map_cloud, nullptr, &p->n_map);
  if (rc) return rc;
  rc = downsample(p, p->map_cloud.p, p->n_map, 1.5 * voxel_size, p->source, &p->source64, &p->n_source);
  if (rc) return rc;
  if (!(1.5 * voxel_size > 0.0) && p->n_source > 0)   // unchanged cloud: still hand out float64 rows
    return fail(p, SVNICP_ERR_INVALID, std::string(who) + ": voxel_size must be positive");
  HIPCHK(p, hipStreamSynchronize(p->stream));   // the clouds are complete when the call returns (other streams read them)
  *n_cropped = p->n_cropped; *n_map = p->n_map; *n_source = p->n_source;
  return SVNICP_OK;
}

}  // namespace

extern "C" {

int svnicp_prep_create(int device, svnicp_prep** out) {
  if (!out) return SVNICP_ERR_INVALID;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
    return fail<svnicp_prep>(nullptr, SVNICP_ERR_NO_DEVICE, "svnicp_prep_create: no HIP device visible (this library has no CPU path)");
  svnicp_prep* p = new svnicp_prep();
  p->device = device;
  if (hipSetDevice(device) != hipSuccess || p->stream.create(hipStreamDefault) != hipSuccess || p->scal.ensure(8) != hipSuccess) {
    delete p;
    return fail<svnicp_prep>(nullptr, SVNICP_ERR_HIP, "svnicp_prep_create: stream / allocation failed");
  }
  *out = p;
  return SVNICP_OK;
}

void svnicp_prep_destroy(svnicp_prep* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  delete p;
}

const char* svnicp_prep_last_error(const svnicp_prep* p) { return p ? p->err.c_str() : svnicp_prep::create_error().c_str(); }

int svnicp_prep_scan(svnicp_prep* p, const float* xyz, int64_t n, int mem_kind, double min_range, double max_range, double voxel_size,
                     double* scan_max_range, int64_t* n_cropped, int64_t* n_map, int64_t* n_source) {
  if (!p || !scan_max_range || !n_cropped || !n_map || !n_source || n < 0 || (n > 0 && !xyz) || n > 0x7fffffffLL)
    return fail(p, SVNICP_ERR_INVALID, "svnicp_prep_scan: bad argument");
  HIPCHK(p, hipSetDevice(p->device));
  p->n_cropped = p->n_map = p->n_source = 0;
  *n_cropped = *n_map = *n_source = 0;
  if (n == 0) return SVNICP_OK;
  const float* din = xyz;
  if (mem_kind != SVNICP_MEM_DEVICE) {
    HIPCHK(p, p->in.ensure((size_t)n * 3));
    HIPCHK(p, hipMemcpyAsync(p->in.p, xyz, (size_t)n * 12, hipMemcpyHostToDevice, p->stream));
    din = p->in.p;
  }
  // ---- crop (:692-704)
  HIPCHK(p, p->keep.ensure((size_t)n)); HIPCHK(p, p->off.ensure((size_t)n));
  HIPCHK(p, hipMemsetAsync(p->scal.p, 0, 8, p->stream));   // encoded doubles are > 0 for every value >= -inf: 0 = nothing seen
  const unsigned g = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(k_prep_crop, dim3(g), dim3(256), 0, p->stream, din, n, min_range * min_range, max_range * max_range, p->keep.p, p->scal.p);
  HIPCHK(p, hipGetLastError());
  return compact_and_sample(p, "svnicp_prep_scan", din, n, p->scal.p, voxel_size, scan_max_range, n_cropped, n_map, n_source);
}

const float* svnicp_prep_cropped_devptr(svnicp_prep* p) { return p ? p->cropped.p : nullptr; }
const float* svnicp_prep_map_cloud_devptr(svnicp_prep* p) { return p ? p->map_cloud.p : nullptr; }
const double* svnicp_prep_source_devptr(svnicp_prep* p) { return p ? p->source64.p : nullptr; }
const float* svnicp_prep_source_f32_devptr(svnicp_prep* p) { return p ? p->source.p : nullptr; }

int svnicp_prep_scan_deskew(svnicp_prep* p, const float* xyz, const void* stamps, int stamp_type, int64_t n, int mem_kind,
                            const double delta_xi[6], int flags, double min_range, double max_range, double voxel_size,
                            double* scan_max_range, int64_t* n_cropped, int64_t* n_map, int64_t* n_source) {
  if (!p || !scan_max_range || !n_cropped || !n_map || !n_source || n < 0 || (n > 0 && !xyz) || n > 0x7fffffffLL)
    return fail(p, SVNICP_ERR_INVALID, "svnicp_prep_scan_deskew: bad argument");
  if (stamp_type != SVNICP_STAMP_F64 && stamp_type != SVNICP_STAMP_F32 && stamp_type != SVNICP_STAMP_U32)
    return fail(p, SVNICP_ERR_INVALID, "svnicp_prep_scan_deskew: unknown stamp_type");
  if (!delta_xi) return fail(p, SVNICP_ERR_INVALID, "svnicp_prep_scan_deskew: delta_xi is NULL");
  for (int k = 0; k < 6; ++k)
    if (!std::isfinite(delta_xi[k])) return fail(p, SVNICP_ERR_INVALID, "svnicp_prep_scan_deskew: delta_xi is not finite");
  if (flags & ~SVNICP_DESKEW_KITTI) return fail(p, SVNICP_ERR_INVALID, "svnicp_prep_scan_deskew: unknown flags");
  HIPCHK(p, hipSetDevice(p->device));
  p->n_cropped = p->n_map = p->n_source = p->n_deskewed = 0;
  *n_cropped = *n_map = *n_source = 0;
  if (n == 0) return SVNICP_OK;
  const bool kitti = (flags & SVNICP_DESKEW_KITTI) != 0;
  const float* din = xyz;
  const void* dst = kitti ? nullptr : stamps;   // KITTI derives its stamps from the points (:385-401)
  if (mem_kind != SVNICP_MEM_DEVICE) {
    HIPCHK(p, p->in.ensure((size_t)n * 3));
    HIPCHK(p, hipMemcpyAsync(p->in.p, xyz, (size_t)n * 12, hipMemcpyHostToDevice, p->stream));
    din = p->in.p;
    if (dst) {
      const size_t bytes = (size_t)n * (stamp_type == SVNICP_STAMP_F64 ? 8 : 4);
      HIPCHK(p, p->stamps_in.ensure(bytes));
      HIPCHK(p, hipMemcpyAsync(p->stamps_in.p, dst, bytes, hipMemcpyHostToDevice, p->stream));
      dst = p->stamps_in.p;
    }
  }
  // ---- deskew (:357-447) fused with the crop (:692-704)
  HIPCHK(p, p->deskewed.ensure((size_t)n * 3)); HIPCHK(p, p->keep.ensure((size_t)n)); HIPCHK(p, p->off.ensure((size_t)n));
  HIPCHK(p, p->dscal.ensure(3));
  if (kitti) HIPCHK(p, p->kpts.ensure((size_t)n * 3));
  if (kitti || dst) HIPCHK(p, p->st.ensure((size_t)n));
  HIPCHK(p, hipMemsetAsync(p->dscal.p, 0, 24, p->stream));   // 0 = nothing seen (max norm, max stamp, min stamp)
  const unsigned g = (unsigned)((n + 255) / 256);
  if (kitti || dst) {   // no stamp field: min == max == 0, the raw frame (:418); k_deskew_crop sees dscal[1] == 0
    constexpr double kVerticalAngleOffset = (0.205 * 3.14159265358979323846) / 180.0;   // :386
    hipLaunchKernelGGL(k_deskew_stamps, dim3(g), dim3(256), 0, p->stream, din, dst, stamp_type, kitti ? 1 : 0, std::sin(kVerticalAngleOffset),
                       std::cos(kVerticalAngleOffset), n, kitti ? p->kpts.p : (float*)nullptr, p->st.p, p->dscal.p);
    HIPCHK(p, hipGetLastError());
  }
  Twist tw;
  for (int k = 0; k < 6; ++k) tw.v[k] = delta_xi[k];
  hipLaunchKernelGGL(k_deskew_crop, dim3(g), dim3(256), 0, p->stream, din, kitti ? (const float*)p->kpts.p : (const float*)nullptr,
                     (kitti || dst) ? (const double*)p->st.p : (const double*)nullptr, n, tw, min_range * min_range, max_range * max_range,
                     p->deskewed.p, p->keep.p, p->dscal.p);
  HIPCHK(p, hipGetLastError());
  p->n_deskewed = n;
  return compact_and_sample(p, "svnicp_prep_scan_deskew", p->deskewed.p, n, p->dscal.p, voxel_size, scan_max_range, n_cropped, n_map, n_source);
}

const float* svnicp_prep_deskewed_devptr(svnicp_prep* p) { return p ? p->deskewed.p : nullptr; }

int svnicp_prep_download_deskewed(svnicp_prep* p, float* out_xyz, int64_t cap_points, int64_t* n_out) {
  if (!p || !n_out) return SVNICP_ERR_INVALID;
  HIPCHK(p, hipSetDevice(p->device));
  *n_out = p->n_deskewed;
  const int64_t n = p->n_deskewed < cap_points ? p->n_deskewed : cap_points;
  if (n > 0 && out_xyz) {
    HIPCHK(p, hipMemcpyAsync(out_xyz, p->deskewed.p, (size_t)n * 12, hipMemcpyDeviceToHost, p->stream));
    HIPCHK(p, hipStreamSynchronize(p->stream));
  }
  return SVNICP_OK;
}

int svnicp_prep_download(svnicp_prep* p, int which, float* out_xyz, int64_t cap_points, int64_t* n_out) {
  if (!p || !n_out || which < 0 || which > 2) return SVNICP_ERR_INVALID;
  HIPCHK(p, hipSetDevice(p->device));
  const int64_t n_all = which == 0 ? p->n_cropped : which == 1 ? p->n_map : p->n_source;
  const float* src = which == 0 ? p->cropped.p : which == 1 ? p->map_cloud.p : p->source.p;
  *n_out = n_all;
  const int64_t n = n_all < cap_points ? n_all : cap_points;
  if (n > 0 && out_xyz) {
    HIPCHK(p, hipMemcpyAsync(out_xyz, src, (size_t)n * 12, hipMemcpyDeviceToHost, p->stream));
    HIPCHK(p, hipStreamSynchronize(p->stream));
  }
  return SVNICP_OK;
}

}  // extern "C"
