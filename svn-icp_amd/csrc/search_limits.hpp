// search_limits.hpp — the size limit of k_stein_search_bf16's 32-bit pair offsets (host and device; no HIP needed, so the
// CPU tests compile it on its own).
#pragma once
#include <cstdint>

namespace svnicp {

// A wave step stores each lane's slot byte (kbest, [B][Ppad]) and target index (kidx, [B][Ppad]) and loads its winner's
// candidate (cand, [B][K]) through a 32-bit BYTE offset from the row of the step's FIRST point, whose 64-bit address is
// wave-uniform (scalar registers).  A lane's point is at most kSearchPointsPerStep − 1 rows past that row, and its column
// is below one row's width, so every offset is below 4 · kSearchPointsPerStep · max(Ppad, K) bytes.
constexpr int64_t kSearchPointsPerStep = 4;   // 64 / particles per group, at 16-particle groups

constexpr int64_t search_offset_bound(int Ppad, int K) {   // exclusive bound of the byte offsets, in 64 bits
  return 4 * kSearchPointsPerStep * (int64_t)(Ppad > K ? Ppad : K);
}
constexpr bool search_offsets_fit(int Ppad, int K) { return search_offset_bound(Ppad, K) <= ((int64_t)1 << 32); }

}  // namespace svnicp
