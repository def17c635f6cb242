// prep_state.hpp — the svnicp_prep object, shared by scan_prep.hip (crop, deskew, uniform samplings) and range_segment.hip
// (range-image segmentation).  One stream per object; every buffer grows on demand and is reused across scans.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

namespace svnicp_prep_detail {

template <typename T>
struct PBuf {
  T* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t n) {
    if (n <= cap && p) return hipSuccess;
    if (p) (void)hipFree(p);
    if (cap > 0) n += n / 2;   // scans vary in size: do not re-allocate for every small growth
    p = nullptr; cap = 0;
    if (n == 0) n = 1;
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T));
    if (e == hipSuccess) cap = n;
    return e;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// range_segment.hip's buffers: their own allocations, so the segmented cloud can be the input of svnicp_prep_scan(_deskew)
struct SegBufs {
  PBuf<float> in, xyz;                       // uploaded raw scan; segmented cloud
  PBuf<int> index;                           // input index of each segmented point
  PBuf<int> owner, parent, size;             // per pixel: winning input index, union-find parent, component size (at roots)
  PBuf<float> range;                         // per pixel
  PBuf<signed char> ground;                  // per pixel
  PBuf<unsigned> rows;                       // per pixel: 4-word row mask of the non-seed members (at roots)
  PBuf<int> label;                           // per pixel
  PBuf<unsigned long long> flags, pre;       // per pixel: (valid root << 32) | keep, and its exclusive scan
  PBuf<char> tmp;
  int64_t n_out = 0, n_pix = 0;
  void release() {
    in.release(); xyz.release(); index.release(); owner.release(); parent.release(); size.release(); range.release();
    ground.release(); rows.release(); label.release(); flags.release(); pre.release(); tmp.release();
  }
};

}  // namespace svnicp_prep_detail

struct svnicp_prep {
  template <typename T> using PBuf = svnicp_prep_detail::PBuf<T>;
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  PBuf<float> in, cropped, map_cloud, source;
  PBuf<double> source64;
  PBuf<int> keep, off, idx, sidx, flag, pre, run_pos;
  PBuf<unsigned long long> key, skey, d2bits, run_min, scal;   // scal: [0] max squared norm (encoded) [1..6] grid bounds
  PBuf<char> tmp;
  int64_t n_cropped = 0, n_map = 0, n_source = 0;
  PBuf<float> deskewed, kpts;
  PBuf<double> st;
  PBuf<char> stamps_in;
  PBuf<unsigned long long> dscal;
  int64_t n_deskewed = 0;
  svnicp_prep_detail::SegBufs seg;
};
