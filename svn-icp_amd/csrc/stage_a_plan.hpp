// stage_a_plan.hpp — the rules of stage A (the exact top-K search): which of the four kernels a registration gets, the
// target layout that kernel wants, and every size its scratch follows (host only; no HIP needed, so the CPU tests compile
// it on its own).  The kernels' own constants are tied to these by static_assert in their .hip files.
#pragma once
#include <cstddef>
#include <cstdint>

namespace svnicp {

// the four kernel families
enum class KnnKernel { Stream /* knn_topk.hip */, SeededScan /* knn_scan.hip */, Tiles /* knn_tiles.hip */, Brute /* knn_brute.hip */ };
// option "knn": auto, or one kernel asked for (v1 | v2 | tiles | brute)
struct KnnOption { bool automatic = true; KnnKernel kernel = KnnKernel::Stream; };
// the order of the target's SoA copies: none (brute force reads the cloud as given), a pseudo-random bijection (streaming
// and seeded-scan kernels), the Morton curve in tiles of kTileSlots (tile kernels)
enum class TargetLayout { None, Hashed, Morton };

constexpr int kTileSlots = 512;          // targets per tile, and per wave step of the seeded scan; the SoA is padded to it
constexpr int kMaxTiles = 8192;          // tile bitmap of the tile kernels (M <= 4 M points)
constexpr int kTilesBase = 512, kTilesChunk = 512, kTilesChunks = 31;   // 512 + 31 * 512 = 16384 survivors per query at most
constexpr int kMatrixKMax = 128;         // tile and brute-force kernels: K they are built for
constexpr int kScanKMax = 200;           // seeded scan
constexpr double kBrutePairsMax = 268435456.0;   // 2^28 (query, target) pairs (2.4e8: 0.20 ms against 0.37 ms for the tile chain with its sorts; 5.4e8: 0.41 against 0.42)
constexpr int kFallbackGrid = 256;       // workgroups of the streaming kernel when it only redoes failed queries
constexpr int kFallbackSlicedMax = 512;  // up to this many failed queries are redone by target slices (all CUs per query)
constexpr int kFallbackQW = 2;           // … two queries per wave, so a few hundred failures still run in parallel

inline int64_t knn_padded_targets(int64_t M) { return ((M + kTileSlots - 1) / kTileSlots) * kTileSlots; }  // multiple of both kernels' steps
inline int knn_pool_size(int K) {   // pool capacity of the streaming kernel: a power of two >= K + 128
  int S = 256;
  while (S < K + 128) S <<= 1;
  return S;
}
inline int knn_slice_count(int K) {  // slices x K entries must fit the merge kernel's 8192-entry LDS sort
  int kp = 1;
  while (kp < K) kp <<= 1;
  int ns = 8192 / kp;
  return ns > 64 ? 64 : (ns < 1 ? 1 : ns);
}
inline bool knn_tiles_applicable(int64_t Mp, int K) {
  return K <= kMatrixKMax && Mp >= 16 * kTileSlots && (Mp % kTileSlots) == 0 && Mp / kTileSlots <= kMaxTiles;
}
// seed parameters: sample Ms ≈ Mp·12/K slots (a multiple of the step), threshold = lane-minimum of rank
// ≈ 2.6·K·Ms/Mp.  Returns false when the fast variant does not apply (large K, small M).
inline bool knn_scan_plan(int64_t Mp, int K, int64_t* Ms, int* seed_rank, int* S2) {
  if (K > kScanKMax || Mp < 16 * kTileSlots || (Mp % kTileSlots) != 0) return false;
  double F = 12.5 / (double)K;
  if (F > 0.25) F = 0.25;
  int64_t ms = (int64_t)((double)Mp * F / kTileSlots + 0.5) * kTileSlots;
  if (ms < kTileSlots) ms = kTileSlots;
  if (ms > Mp) ms = Mp;
  int j = (int)(2.6 * (double)K * (double)ms / (double)Mp + 0.5);
  if (j < 4) j = 4;
  if (j > 44) j = 44;
  *Ms = ms;
  *seed_rank = j - 1;
  *S2 = 1024;
  return true;
}
// the sizes the brute-force kernel is for: every pair is scored twice (float32)
inline bool knn_brute_applicable(int64_t B, int64_t M, int K) {
  return K >= 1 && K <= kMatrixKMax && B >= 1 && M >= 1 && M < (1ll << 31) && (double)B * (double)M <= kBrutePairsMax;
}
// words of chunk_tab (tile kernels) for `rows` query rows
inline size_t tiles_chunk_tab_words(int64_t rows) { return (size_t)rows * kTilesChunks + 16 + (size_t)(rows + 63) / 64 + 1; }

struct StageAPlan {
  KnnKernel kernel = KnnKernel::Stream;
  TargetLayout layout = TargetLayout::Hashed;
  int64_t rows = 0, Mp = 0;    // query rows the scratch is sized for; padded target slots
  int K = 0;                   // the K the choice was made for
  int64_t scan_Ms = 0;         // SeededScan: slots of the seed sample …
  int scan_rank = 0;           // … and the rank its threshold is taken at
  int S2 = 0;                  // SeededScan, Tiles: most survivors a query may hold
  int sliced_max = 0;          // SeededScan, Tiles: failed queries redone by target slices up to this many (0: list mode only)
  int arena_cap = 0;           // Tiles: overflow chunks of the shared arena
  bool has_fallback() const { return kernel == KnnKernel::SeededScan || kernel == KnnKernel::Tiles; }
  // can this plan's kernel search with Kq neighbours instead of K?  The seeded scan's sample and rank are made for K alone;
  // the tile and brute-force kernels take any Kq they are built for; the streaming kernel takes any
  bool can_search(int Kq) const {
    if (kernel == KnnKernel::SeededScan) return Kq == K;
    return kernel == KnnKernel::Stream || Kq <= kMatrixKMax;
  }
};

// The choice, in this order:
//  1. automatic without brute force: tiles where they apply (K <= 128, 16 to 8192 tiles), else the seeded scan where it
//     applies (K <= 200, at least 16 tiles), else the streaming kernel;
//  2. option v1: the streaming kernel; option v2: the seeded scan where it applies, else the streaming kernel;
//  3. option tiles is rule 1 (a size the tile kernels do not take gets what rule 1 gives it, never brute force);
//  4. option brute: brute force for K <= 128 and M < 2^31 whatever the pair count; for K > 128 it is rule 1;
//  5. automatic: brute force up to 2^28 pairs (knn_brute_applicable), else rule 1.
inline StageAPlan plan_stage_a(int64_t rows, int64_t M, int K, KnnOption opt, int fallback_sliced_max) {
  StageAPlan p;
  p.rows = rows; p.K = K; p.Mp = knn_padded_targets(M);
  const bool scan_ok = knn_scan_plan(p.Mp, K, &p.scan_Ms, &p.scan_rank, &p.S2);
  p.kernel = knn_tiles_applicable(p.Mp, K) ? KnnKernel::Tiles : scan_ok ? KnnKernel::SeededScan : KnnKernel::Stream;
  if (opt.automatic) {
    if (knn_brute_applicable(rows, M, K)) p.kernel = KnnKernel::Brute;
  } else if (opt.kernel == KnnKernel::Stream) {
    p.kernel = KnnKernel::Stream;
  } else if (opt.kernel == KnnKernel::SeededScan) {
    p.kernel = scan_ok ? KnnKernel::SeededScan : KnnKernel::Stream;
  } else if (opt.kernel == KnnKernel::Brute && K <= kMatrixKMax && M < (1ll << 31)) {
    p.kernel = KnnKernel::Brute;
  }
  p.layout = p.kernel == KnnKernel::Brute ? TargetLayout::None : p.kernel == KnnKernel::Tiles ? TargetLayout::Morton : TargetLayout::Hashed;
  if (p.kernel == KnnKernel::Tiles) {
    // survivors of the f32 pre-filter: 512 slots per query (median 127 at C3) + a shared arena of 512-slot chunks for the
    // heavy tail (C3: 0.4 % of the queries, 0.17 M entries; C5: 4 %, 3.1 M entries, up to 9016 per query)
    p.S2 = kTilesBase + kTilesChunks * kTilesChunk;
    p.arena_cap = (int)(rows / 4 > 32768 ? rows / 4 : 32768);
  }
  if (p.has_fallback()) {   // option fallback_sliced_max: -1 the default, 0 forces the list-mode fallback
    p.sliced_max = fallback_sliced_max >= 0 && fallback_sliced_max < kFallbackSlicedMax ? fallback_sliced_max : kFallbackSlicedMax;
  }
  return p;
}

}  // namespace svnicp
