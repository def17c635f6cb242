// voxel_table_device.hpp — the voxel map's hash table as device code sees it, stated once: the packed key of a voxel index, the
// hash, and the bounded read-only lookup.  Used by map_table.hip (insert, rehash), map_normals.hip, map_visibility.hip and
// map_score.hip.  Layout (voxel_map.hip's header comment): open addressing with linear probing over keys[cap], cap a power of
// two; a key is the three voxel indices, each offset by 2^20 into 21 bits; kEmpty ends a probe sequence, kTomb (a removed
// voxel) does not.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace svnicp {

constexpr unsigned long long kEmpty = ~0ull;
constexpr unsigned long long kTomb = ~0ull - 1ull;
constexpr int kOff = 1 << 20;  // voxel indices in [-2^20, 2^20)

__device__ __forceinline__ unsigned long long hash_key(unsigned long long k) {  // splitmix64 finaliser
  k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
  k ^= k >> 27; k *= 0x94d049bb133111ebull;
  k ^= k >> 31;
  return k;
}

__device__ __forceinline__ bool voxel_in_range(long long v0, long long v1, long long v2) {   // outside: no such voxel
  return v0 >= -kOff && v0 < kOff && v1 >= -kOff && v1 < kOff && v2 >= -kOff && v2 < kOff;
}

// valid for voxel_in_range indices only: anything else would alias into another voxel's bits
__device__ __forceinline__ unsigned long long pack_key(long long v0, long long v1, long long v2) {
  return ((unsigned long long)(v0 + kOff) << 42) | ((unsigned long long)(v1 + kOff) << 21) | (unsigned long long)(v2 + kOff);
}

// the slot that holds `key`, or -1: bounded (a full table ends the loop), goes on past kTomb, stops at kEmpty; the table is
// only read
__device__ __forceinline__ int64_t find_slot(const unsigned long long* __restrict__ keys, int64_t cap, unsigned long long key) {
  unsigned long long h = hash_key(key) & (unsigned long long)(cap - 1);
  for (int64_t probe = 0; probe < cap; ++probe) {
    const unsigned long long cur = keys[h];
    if (cur == key) return (int64_t)h;
    if (cur == kEmpty) return -1;
    h = (h + 1) & (unsigned long long)(cap - 1);
  }
  return -1;
}

// wave helper of the map kernels that compact in place (select_smallest of map_normals.hip, k_vis_clear)
__device__ __forceinline__ int lanes_below(unsigned long long mask) {   // set bits of mask that belong to lanes below this one
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

}  // namespace svnicp
