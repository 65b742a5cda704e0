// Batch assembly out of a device-resident frame store (gfx950): ONE launch writes every per-pair tensor of a step from
// per-FRAME and per-PAIR tables, dst_k[b] = op_k(src_k[index[row_k][b]]) for a table of up to DVD_STORE_MAX tensors.
//
// What it is for: datasets/frame_store.py holds a video once -- every frame's image, depths and camera tables, every flow
// pair's flows and occlusion masks -- and a step's batch is three index rows (f_1, f_2, pair) plus this launch.  It is the
// re-arrangement scripts/preprocess/davis/generate_sequence_midas.py:117-170 does on the host when it writes the pair packs,
// followed by the reader's datasets/davis_sequence.py:98-115; every value is copied or converted exactly, none is computed.
//
// HBM bound, no reuse: no LDS, no atomics.  The scheme is that of gather.hip: the table travels in the kernel arguments, the
// work is cut into tiles of one destination row of one tensor x 1024 accesses, a block moves a tile with four loads in flight
// per lane and then four stores, and walks the tile list grid-stride.  The access width of a tensor follows from the alignment
// of its bases and row size: 16, 4 or 1 bytes for COPY; for MASK and FILL, whose destination is fp32, 16 (four pixels) or 4.

#include "dvd_common.h"

namespace dvd {

struct StoreEntry {
  const char* src;
  char* dst;
  long long bpr;   // bytes per destination row
  int rows;        // rows of the source table
  int tile0;       // first tile of this entry in the launch's tile list
  int tpr;         // tiles per destination row
  int vec;         // bytes per destination access: 16, 4 or 1
  int op;          // DVD_STORE_COPY / MASK / FILL
  int sel;         // which index row selects the source row
};
struct StoreTable {
  StoreEntry e[DVD_STORE_MAX];
  int n, B, tiles;
};

constexpr int kStoreAcc = 4;                   // accesses per lane and tile
constexpr int kStoreTile = 256 * kStoreAcc;    // accesses per tile

template <typename T>
__device__ __forceinline__ void store_copy_tile(const char* __restrict__ s, char* __restrict__ d, long long n) {
  const T* __restrict__ sp = reinterpret_cast<const T*>(s);
  T* __restrict__ dp = reinterpret_cast<T*>(d);
  const int i0 = threadIdx.x, i1 = i0 + 256, i2 = i0 + 512, i3 = i0 + 768;
  static_assert(kStoreAcc == 4, "the tile movers are written out for four accesses per lane");
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

// uint8 occlusion mask -> the training mask, 1 - ceil(m) of the writer (:144-147): exact for every uint8 value
__device__ __forceinline__ float mask_of(unsigned m) { return 1.0f - (float)m; }
__device__ __forceinline__ float4 mask_of4(uchar4 m) { return make_float4(mask_of(m.x), mask_of(m.y), mask_of(m.z), mask_of(m.w)); }

// S: source access (uchar4 or unsigned char), D: destination access (float4 or float); n accesses left in this row
template <typename S, typename D, typename F>
__device__ __forceinline__ void store_mask_tile(const char* __restrict__ s, char* __restrict__ d, long long n, F conv) {
  const S* __restrict__ sp = reinterpret_cast<const S*>(s);
  D* __restrict__ dp = reinterpret_cast<D*>(d);
  const int i0 = threadIdx.x, i1 = i0 + 256, i2 = i0 + 512, i3 = i0 + 768;
  S v0 = {}, v1 = {}, v2 = {}, v3 = {};
  if (i0 < n) v0 = sp[i0];
  if (i1 < n) v1 = sp[i1];
  if (i2 < n) v2 = sp[i2];
  if (i3 < n) v3 = sp[i3];
  if (i0 < n) dp[i0] = conv(v0);
  if (i1 < n) dp[i1] = conv(v1);
  if (i2 < n) dp[i2] = conv(v2);
  if (i3 < n) dp[i3] = conv(v3);
}

template <typename D>
__device__ __forceinline__ void store_fill_tile(D v, char* __restrict__ d, long long n) {
  D* __restrict__ dp = reinterpret_cast<D*>(d);
  const int i0 = threadIdx.x, i1 = i0 + 256, i2 = i0 + 512, i3 = i0 + 768;
  if (i0 < n) dp[i0] = v;
  if (i1 < n) dp[i1] = v;
  if (i2 < n) dp[i2] = v;
  if (i3 < n) dp[i3] = v;
}

__global__ __launch_bounds__(256) void store_gather_kernel(const StoreTable tab, const int* __restrict__ index,
                                                           const long long index_stride) {
  for (int t = blockIdx.x; t < tab.tiles; t += gridDim.x) {
    // which tensor: tile0 is increasing, so its index is a count over constant indices; the entry itself is then read from
    // the kernel-argument segment with a wave-uniform index (scalar loads, nothing lives in scratch or LDS)
    int k = 0;
#pragma unroll
    for (int i = 1; i < DVD_STORE_MAX; ++i) k += (i < tab.n && t >= tab.e[i].tile0) ? 1 : 0;
    const char* src = tab.e[k].src;
    char* dst = tab.e[k].dst;
    const long long bpr = tab.e[k].bpr;
    const int rows = tab.e[k].rows, tile0 = tab.e[k].tile0, tpr = tab.e[k].tpr, vec = tab.e[k].vec, op = tab.e[k].op;
    const int sel = tab.e[k].sel;
    const int r = t - tile0, b = r / tpr, c = r - b * tpr;
    const int p = index[(long long)sel * index_stride + b];
    if ((unsigned)p >= (unsigned)rows) continue;       // an index outside its table copies nothing (never reads out of bounds)
    const long long off = (long long)c * kStoreTile * vec;    // byte offset of this tile in the destination row
    char* d = dst + (long long)b * bpr + off;
    const long long n = (bpr - off) / vec;             // accesses left in this row (the movers take at most kStoreTile)
    if (op == DVD_STORE_COPY) {
      const char* s = src + (long long)p * bpr + off;
      if (vec == 16)
        store_copy_tile<uint4>(s, d, n);
      else if (vec == 4)
        store_copy_tile<unsigned>(s, d, n);
      else
        store_copy_tile<unsigned char>(s, d, n);
    } else if (op == DVD_STORE_MASK) {                 // source row: bpr / 4 bytes, one per fp32 of the destination
      const char* s = src + ((long long)p * bpr + off) / 4;
      if (vec == 16)
        store_mask_tile<uchar4, float4>(s, d, n, [](uchar4 m) { return mask_of4(m); });
      else
        store_mask_tile<unsigned char, float>(s, d, n, [](unsigned char m) { return mask_of(m); });
    } else {                                           // DVD_STORE_FILL: the one fp32 of table row p
      const float v = reinterpret_cast<const float*>(src)[p];
      if (vec == 16)
        store_fill_tile<float4>(make_float4(v, v, v, v), d, n);
      else
        store_fill_tile<float>(v, d, n);
    }
  }
}

}  // namespace dvd

extern "C" {

int dvd_store_gather(const dvd_store_item* items, int n_items, const int* index, long long index_stride, int B,
                     dvd_stream_t stream) {
  using namespace dvd;
  DVD_REQUIRE(items && index && B > 0, "store_gather: null pointer / empty batch");
  DVD_REQUIRE(n_items > 0 && n_items <= DVD_STORE_MAX, "store_gather: %d tensors (1..%d per launch)", n_items, DVD_STORE_MAX);
  DVD_REQUIRE(index_stride >= B, "store_gather: index rows of stride %lld overlap at %d pairs", index_stride, B);
  StoreTable tab;
  tab.n = n_items;
  tab.B = B;
  long long tiles = 0;
  double bytes = 0.0;
  unsigned used_rows = 0;
  for (int k = 0; k < n_items; ++k) {
    const dvd_store_item& it = items[k];
    DVD_REQUIRE(it.src && it.dst && it.bytes_per_row > 0 && it.src_rows > 0, "store_gather: tensor %d: null pointer / size", k);
    DVD_REQUIRE(it.index_row >= 0 && it.index_row < 3, "store_gather: tensor %d: index row %d (0..2)", k, it.index_row);
    DVD_REQUIRE(it.op == DVD_STORE_COPY || it.op == DVD_STORE_MASK || it.op == DVD_STORE_FILL, "store_gather: tensor %d: "
                "operation %d", k, it.op);
    const uintptr_t s = (uintptr_t)it.src, d = (uintptr_t)it.dst;
    const unsigned long long span = (unsigned long long)it.bytes_per_row * (unsigned long long)B;
    // bytes of the source table this entry may read
    const unsigned long long row_src = it.op == DVD_STORE_COPY ? (unsigned long long)it.bytes_per_row
                                       : (it.op == DVD_STORE_MASK ? (unsigned long long)it.bytes_per_row / 4 : 4ULL);
    const unsigned long long span_src = row_src * (unsigned long long)it.src_rows;
    DVD_REQUIRE(d + span <= s || s + span_src <= d, "store_gather: tensor %d: src and dst must not overlap", k);
    StoreEntry& e = tab.e[k];
    e.src = static_cast<const char*>(it.src);
    e.dst = static_cast<char*>(it.dst);
    e.bpr = it.bytes_per_row;
    e.rows = it.src_rows;
    e.op = it.op;
    e.sel = it.index_row;
    if (it.op == DVD_STORE_COPY) {
      const uintptr_t bits = s | d | (uintptr_t)it.bytes_per_row;
      e.vec = (bits & 15) == 0 ? 16 : ((bits & 3) == 0 ? 4 : 1);
      bytes += 2.0 * (double)span;
    } else {
      DVD_REQUIRE(((d | (uintptr_t)it.bytes_per_row) & 3) == 0, "store_gather: tensor %d: an fp32 destination needs 4-byte "
                  "alignment", k);
      const bool d16 = ((d | (uintptr_t)it.bytes_per_row) & 15) == 0;
      if (it.op == DVD_STORE_MASK) {
        e.vec = (d16 && (s & 3) == 0) ? 16 : 4;      // (a row of bpr / 4 source bytes is then a multiple of 4 as well)
        bytes += 1.25 * (double)span;
      } else {
        DVD_REQUIRE((s & 3) == 0, "store_gather: tensor %d: an fp32 table needs 4-byte alignment", k);
        e.vec = d16 ? 16 : 4;
        bytes += (double)span + 4.0 * B;
      }
    }
    const long long per_tile = (long long)kStoreTile * e.vec;
    const long long tpr = (it.bytes_per_row + per_tile - 1) / per_tile;
    DVD_REQUIRE(tiles + tpr * B < (1LL << 30), "store_gather: too much work for one launch");
    e.tile0 = (int)tiles;
    e.tpr = (int)tpr;
    tiles += tpr * B;
    used_rows |= 1u << it.index_row;
  }
  for (int k = n_items; k < DVD_STORE_MAX; ++k) tab.e[k] = tab.e[0];
  tab.tiles = (int)tiles;
  for (int r = 0; r < 3; ++r) bytes += (used_rows >> r & 1) ? 4.0 * B : 0.0;
  bytes_add(DVD_BYTES_GATHER, bytes);
  const int grid = (int)(tiles < 4096 ? tiles : 4096);       // 16 blocks per CU in flight, grid-stride beyond
  hipLaunchKernelGGL(store_gather_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), tab, index, index_stride);
  DVD_LAUNCH_OK();
  return DVD_OK;
}

}  // extern "C"
