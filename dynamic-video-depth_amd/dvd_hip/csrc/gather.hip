// Batched pair permutation (gfx950): dst_k[b] = src_k[perm[b]] for a table of up to DVD_GATHER_MAX per-pair tensors in ONE launch.
//
// What it is for: a step that mixes frame gaps works on pairs sorted by their Euler step count (models/scene_flow_motion_field.py,
// gap_plan), so a device-resident batch of ~20 tensors -- images, flows, masks, cameras, time stamps; 0.75 GB at 48 pairs of
// 384 x 672 -- is re-ordered once per step, and the exported `pred` surfaces once more with the inverse permutation.  The
// reference has no counterpart (it runs one pair per step); torch.index_select per tensor is what this replaces.
//
// HBM bound, no reuse: no LDS, no atomics.  The table travels in the kernel arguments (1.3 KB), the work is cut into tiles of
// one pair of one tensor x 1024 accesses (16 KB with 16-byte accesses); a block copies a tile with four loads in flight per
// lane and then four stores, and walks the tile list grid-stride.  A tensor whose bytes per pair and base addresses are
// multiples of 16 moves as uint4, one with multiples of 4 (t_1: 12 bytes per pair) as dwords, anything else as bytes.

#include "dvd_common.h"

namespace dvd {

struct GatherEntry {
  const char* src;
  char* dst;
  long long bpp;  // bytes per pair
  int tile0;      // first tile of this entry in the launch's tile list
  int tpp;        // tiles per pair
  int vec;        // bytes per access: 16, 4 or 1
  int pad;
};
struct GatherTable {
  GatherEntry e[DVD_GATHER_MAX];
  int n, B, tiles;
};

constexpr int kGatherAcc = 4;                    // accesses per lane and tile
constexpr int kGatherTile = 256 * kGatherAcc;    // accesses per tile

template <typename T>
__device__ __forceinline__ void gather_tile(const char* __restrict__ s, char* __restrict__ d, long long n) {
  const T* __restrict__ sp = reinterpret_cast<const T*>(s);
  T* __restrict__ dp = reinterpret_cast<T*>(d);
  const int i0 = threadIdx.x, i1 = i0 + 256, i2 = i0 + 512, i3 = i0 + 768;
  static_assert(kGatherAcc == 4, "gather_tile is written out for four accesses per lane");
  T v0 = {}, v1 = {}, v2 = {}, v3 = {};
  if (i0 < n) v0 = sp[i0];
  if (i1 < n) v1 = sp[i1];
  if (i2 < n) v2 = sp[i2];
  if (i3 < n) v3 = sp[i3];
  if (i0 < n) dp[i0] = v0;
  if (i1 < n) dp[i1] = v1;
  if (i2 < n) dp[i2] = v2;
  if (i3 < n) dp[i3] = v3;
}

__global__ __launch_bounds__(256) void gather_pairs_kernel(const GatherTable tab, const int* __restrict__ perm) {
  for (int t = blockIdx.x; t < tab.tiles; t += gridDim.x) {
    // which tensor: tile0 is increasing, so its index is a count over constant indices; the entry itself is then read from
    // the kernel-argument segment with a wave-uniform index (scalar loads, nothing lives in scratch or LDS)
    int k = 0;
#pragma unroll
    for (int i = 1; i < DVD_GATHER_MAX; ++i) k += (i < tab.n && t >= tab.e[i].tile0) ? 1 : 0;
    const char* src = tab.e[k].src;
    char* dst = tab.e[k].dst;
    const long long bpp = tab.e[k].bpp;
    const int tile0 = tab.e[k].tile0, tpp = tab.e[k].tpp, vec = tab.e[k].vec;
    const int r = t - tile0, b = r / tpp, c = r - b * tpp;
    const int p = perm[b];
    if ((unsigned)p >= (unsigned)tab.B) continue;      // an index outside the batch copies nothing (never reads out of bounds)
    const long long off = (long long)c * kGatherTile * vec;
    const char* s = src + (long long)p * bpp + off;
    char* d = dst + (long long)b * bpp + off;
    const long long n = (bpp - off) / vec;         // accesses left in this pair (gather_tile takes at most kGatherTile)
    if (vec == 16)
      gather_tile<uint4>(s, d, n);
    else if (vec == 4)
      gather_tile<unsigned>(s, d, n);
    else
      gather_tile<unsigned char>(s, d, n);
  }
}

}  // namespace dvd

extern "C" {

int dvd_gather_pairs(const dvd_gather_item* items, int n_items, const int* perm, int B, dvd_stream_t stream) {
  using namespace dvd;
  DVD_REQUIRE(items && perm && B > 0, "gather_pairs: null pointer / empty batch");
  DVD_REQUIRE(n_items > 0 && n_items <= DVD_GATHER_MAX, "gather_pairs: %d tensors (1..%d per launch)", n_items, DVD_GATHER_MAX);
  GatherTable tab;
  tab.n = n_items;
  tab.B = B;
  long long tiles = 0;
  double bytes = 4.0 * B;
  for (int k = 0; k < n_items; ++k) {
    const dvd_gather_item& it = items[k];
    DVD_REQUIRE(it.src && it.dst && it.bytes_per_pair > 0, "gather_pairs: tensor %d: null pointer / size", k);
    const uintptr_t s = (uintptr_t)it.src, d = (uintptr_t)it.dst;
    const unsigned long long span = (unsigned long long)it.bytes_per_pair * (unsigned long long)B;
    DVD_REQUIRE(s != d && (s < d ? d - s : s - d) >= span, "gather_pairs: tensor %d: src and dst must not overlap", k);
    const uintptr_t bits = s | d | (uintptr_t)it.bytes_per_pair;
    GatherEntry& e = tab.e[k];
    e.src = static_cast<const char*>(it.src);
    e.dst = static_cast<char*>(it.dst);
    e.bpp = it.bytes_per_pair;
    e.vec = (bits & 15) == 0 ? 16 : ((bits & 3) == 0 ? 4 : 1);
    const long long per_tile = (long long)kGatherTile * e.vec;
    const long long tpp = (it.bytes_per_pair + per_tile - 1) / per_tile;
    DVD_REQUIRE(tiles + tpp * B < (1LL << 30), "gather_pairs: too much work for one launch");
    e.tile0 = (int)tiles;
    e.tpp = (int)tpp;
    e.pad = 0;
    tiles += tpp * B;
    bytes += 2.0 * (double)span;
  }
  for (int k = n_items; k < DVD_GATHER_MAX; ++k) tab.e[k] = tab.e[0];
  tab.tiles = (int)tiles;
  bytes_add(DVD_BYTES_GATHER, bytes);
  const int grid = (int)(tiles < 4096 ? tiles : 4096);       // 16 blocks per CU in flight, grid-stride beyond
  hipLaunchKernelGGL(gather_pairs_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), tab, perm);
  DVD_LAUNCH_OK();
  return DVD_OK;
}

}  // extern "C"
