// prep_state.hpp — the svnicp_prep object, shared by scan_prep.hip (crop, deskew, uniform samplings) and range_segment.hip
// (range-image segmentation).  One stream per object; every buffer grows on demand and is reused across scans.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "device_buffer.hpp"

// range_segment.hip's buffers: their own allocations, so the segmented cloud can be the input of svnicp_prep_scan(_deskew)
struct SegBufs {
  GrowBuf<float> in, xyz;                       // uploaded raw scan; segmented cloud
  GrowBuf<int> index;                           // input index of each segmented point
  GrowBuf<int> owner, parent, size;             // per pixel: winning input index, union-find parent, component size (at roots)
  GrowBuf<float> range;                         // per pixel
  GrowBuf<signed char> ground;                  // per pixel
  GrowBuf<unsigned> rows;                       // per pixel: 4-word row mask of the non-seed members (at roots)
  GrowBuf<int> label;                           // per pixel
  GrowBuf<unsigned long long> flags, pre;       // per pixel: (valid root << 32) | keep, and its exclusive scan
  GrowBuf<char> tmp;
  int64_t n_out = 0, n_pix = 0;
};

struct svnicp_prep {
  int device = 0;
  svnicp_host::Stream stream;   // before the buffers: destroyed after them
  std::string err;
  // what svnicp_prep_last_error(nullptr) returns: shared by scan_prep.hip and range_segment.hip
  static std::string& create_error() { thread_local std::string s; return s; }
  GrowBuf<float> in, cropped, map_cloud, source;
  GrowBuf<double> source64;
  GrowBuf<int> keep, off, idx, sidx, flag, pre, run_pos;
  GrowBuf<unsigned long long> key, skey, d2bits, run_min, scal;   // scal: [0] max squared norm (encoded) [1..6] grid bounds
  GrowBuf<char> tmp;
  int64_t n_cropped = 0, n_map = 0, n_source = 0;
  GrowBuf<float> deskewed, kpts;
  GrowBuf<double> st;
  GrowBuf<char> stamps_in;
  GrowBuf<unsigned long long> dscal;
  int64_t n_deskewed = 0;
  SegBufs seg;
};
