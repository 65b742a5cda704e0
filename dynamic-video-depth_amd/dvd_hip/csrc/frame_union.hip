// The depth net once per DISTINCT frame of a step (gfx950; opt.share_frames, models/frame_union.py): the three row movers
// between the step's two per-pair image sets and the union of their frames.
//
//   dvd_union_gather   img_u[u] = (set[u] ? img_2 : img_1)[row[u]]                       2B images -> U_pad union rows
//   dvd_union_scatter  depth_1[b] = D[u1[b]], depth_2[b] = D[u2[b]]                      U_pad depth maps -> 2B, ONE launch
//   dvd_union_reduce   G[u] = sum over the row's CSR entries of (set ? g_d2 : g_d1)[row] 2B depth gradients -> U_pad
//
// The reference evaluates net_depth(img_1) and net_depth(img_2) with the net in eval() mode (models/scene_flow_motion_field.py
// :157,168: BatchNorm statistics are fixed), so an image shown k times has ONE depth map and the sum of its k depth gradients
// is what its one backward pass starts from.  Nothing but copies and sequential fp32 adds happens here: the reduction walks a
// row's contributors in list order, one add each, no atomics and no scaling, so its result is bit-reproducible.
//
// HBM bound, no reuse: no LDS, no atomics.  The scheme is that of frame_store.hip: the work is cut into tiles of one
// destination row x 1024 accesses, a block moves a tile with four loads in flight per lane and then four stores, and walks the
// tile list grid-stride.  Accesses are 16 bytes where the row size and every base address are multiples of 16, dwords otherwise.
// An index outside its table reads and writes nothing.

#include "dvd_common.h"

namespace dvd {

constexpr int kUnionAcc = 4;                   // accesses per lane and tile
constexpr int kUnionTile = 256 * kUnionAcc;    // accesses per tile

template <typename T>
__device__ __forceinline__ void union_copy_tile(const char* __restrict__ s, char* __restrict__ d, long long n) {
  const T* __restrict__ sp = reinterpret_cast<const T*>(s);
  T* __restrict__ dp = reinterpret_cast<T*>(d);
  const int i0 = threadIdx.x, i1 = i0 + 256, i2 = i0 + 512, i3 = i0 + 768;
  static_assert(kUnionAcc == 4, "the tile movers are written out for four accesses per lane");
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

__device__ __forceinline__ void acc_add(float& a, float v) { a = a + v; }
__device__ __forceinline__ void acc_add(float4& a, float4 v) {
  a.x = a.x + v.x;
  a.y = a.y + v.y;
  a.z = a.z + v.z;
  a.w = a.w + v.w;
}

// rows: rows of each of the two source sets; a (set, row) outside {0, 1} x [0, rows) copies nothing
template <typename T>
__global__ __launch_bounds__(256) void union_gather_kernel(const char* __restrict__ src_1, const char* __restrict__ src_2,
                                                           char* __restrict__ out, const int* __restrict__ set,
                                                           const int* __restrict__ row, const int U_pad, const int rows,
                                                           const long long bpr, const int tpr) {
  const long long tiles = (long long)U_pad * tpr;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int u = (int)(t / tpr), c = (int)(t - (long long)u * tpr);
    const int s = set[u], r = row[u];
    if ((unsigned)s > 1u || (unsigned)r >= (unsigned)rows) continue;
    const long long off = (long long)c * kUnionTile * (long long)sizeof(T);
    union_copy_tile<T>((s ? src_2 : src_1) + (long long)r * bpr + off, out + (long long)u * bpr + off,
                       (bpr - off) / (long long)sizeof(T));
  }
}

// destination row j < 2B: j < B is depth_1[j] = D[u1[j]], else depth_2[j - B] = D[u2[j - B]]; u12 = [u1 | u2] as handed over
template <typename T>
__global__ __launch_bounds__(256) void union_scatter_kernel(const char* __restrict__ D, char* __restrict__ dst_1,
                                                            char* __restrict__ dst_2, const int* __restrict__ u1,
                                                            const int* __restrict__ u2, const int B, const int U_pad,
                                                            const long long bpr, const int tpr) {
  const long long tiles = 2LL * B * tpr;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int j = (int)(t / tpr), c = (int)(t - (long long)j * tpr);
    const int b = j < B ? j : j - B;
    const int u = j < B ? u1[b] : u2[b];
    if ((unsigned)u >= (unsigned)U_pad) continue;
    const long long off = (long long)c * kUnionTile * (long long)sizeof(T);
    union_copy_tile<T>(D + (long long)u * bpr + off, (j < B ? dst_1 : dst_2) + (long long)b * bpr + off,
                       (bpr - off) / (long long)sizeof(T));
  }
}

// entries[e] = set * B + row, e in [offsets[u], offsets[u + 1]) for union row u; T: float or float4
template <typename T>
__global__ __launch_bounds__(256) void union_reduce_kernel(const char* __restrict__ g_1, const char* __restrict__ g_2,
                                                           char* __restrict__ G, const int* __restrict__ offsets,
                                                           const int* __restrict__ entries, const int U_pad, const int B,
                                                           const long long bpr, const int tpr) {
  const long long tiles = (long long)U_pad * tpr;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int u = (int)(t / tpr), c = (int)(t - (long long)u * tpr);
    int e0 = offsets[u], e1 = offsets[u + 1];
    e0 = e0 < 0 ? 0 : e0;                              // a range outside the entry list contributes nothing
    e1 = e1 > 2 * B ? 2 * B : e1;
    const long long off = (long long)c * kUnionTile * (long long)sizeof(T);
    const long long n = (bpr - off) / (long long)sizeof(T);
    const int i0 = threadIdx.x, i1 = i0 + 256, i2 = i0 + 512, i3 = i0 + 768;
    T a0 = {}, a1 = {}, a2 = {}, a3 = {};
    for (int e = e0; e < e1; ++e) {                    // list order, left to right: one fp32 add per contributor
      const int sr = entries[e];
      if ((unsigned)sr >= 2u * (unsigned)B) continue;
      const char* g = (sr < B ? g_1 + (long long)sr * bpr : g_2 + (long long)(sr - B) * bpr) + off;
      const T* __restrict__ gp = reinterpret_cast<const T*>(g);
      T v0 = {}, v1 = {}, v2 = {}, v3 = {};
      if (i0 < n) v0 = gp[i0];
      if (i1 < n) v1 = gp[i1];
      if (i2 < n) v2 = gp[i2];
      if (i3 < n) v3 = gp[i3];
      acc_add(a0, v0);
      acc_add(a1, v1);
      acc_add(a2, v2);
      acc_add(a3, v3);
    }
    T* __restrict__ dp = reinterpret_cast<T*>(G + (long long)u * bpr + off);
    if (i0 < n) dp[i0] = a0;
    if (i1 < n) dp[i1] = a1;
    if (i2 < n) dp[i2] = a2;
    if (i3 < n) dp[i3] = a3;
  }
}

// access width of a launch and its tiles per row; false: too much work for one launch
static bool union_shape(uintptr_t bits, long long bpr, long long dst_rows, int* vec, int* tpr, int* grid) {
  *vec = (bits & 15) == 0 ? 16 : 4;
  const long long per_tile = (long long)kUnionTile * *vec;
  const long long t = (bpr + per_tile - 1) / per_tile;
  if (t * dst_rows >= (1LL << 30)) return false;
  *tpr = (int)t;
  const long long tiles = t * dst_rows;
  *grid = (int)(tiles < 4096 ? tiles : 4096);          // 16 blocks per CU in flight, grid-stride beyond
  return true;
}

static bool disjoint(uintptr_t a, unsigned long long na, uintptr_t b, unsigned long long nb) { return a + na <= b || b + nb <= a; }

}  // namespace dvd

extern "C" {

int dvd_union_gather(const void* img_1, const void* img_2, void* out, const int* set, const int* row, int U_pad, int B,
                     long long bytes_per_row, dvd_stream_t stream) {
  using namespace dvd;
  DVD_REQUIRE(img_1 && img_2 && out && set && row, "union_gather: null pointer");
  DVD_REQUIRE(U_pad > 0 && B > 0 && bytes_per_row > 0, "union_gather: empty union / batch / row");
  const uintptr_t s1 = (uintptr_t)img_1, s2 = (uintptr_t)img_2, d = (uintptr_t)out;
  const uintptr_t bits = s1 | s2 | d | (uintptr_t)bytes_per_row;
  DVD_REQUIRE((bits & 3) == 0, "union_gather: rows of dwords need 4-byte alignment");
  const unsigned long long src_span = (unsigned long long)bytes_per_row * B, dst_span = (unsigned long long)bytes_per_row * U_pad;
  DVD_REQUIRE(disjoint(d, dst_span, s1, src_span) && disjoint(d, dst_span, s2, src_span), "union_gather: out overlaps a source");
  int vec, tpr, grid;
  DVD_REQUIRE(union_shape(bits, bytes_per_row, U_pad, &vec, &tpr, &grid), "union_gather: too much work for one launch");
  bytes_add(DVD_BYTES_GATHER, 2.0 * (double)dst_span + 8.0 * U_pad);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const char *a = static_cast<const char*>(img_1), *b = static_cast<const char*>(img_2);
  if (vec == 16)
    hipLaunchKernelGGL(union_gather_kernel<uint4>, dim3(grid), dim3(256), 0, st, a, b, static_cast<char*>(out), set, row, U_pad, B,
                       bytes_per_row, tpr);
  else
    hipLaunchKernelGGL(union_gather_kernel<unsigned>, dim3(grid), dim3(256), 0, st, a, b, static_cast<char*>(out), set, row, U_pad,
                       B, bytes_per_row, tpr);
  DVD_LAUNCH_OK();
  return DVD_OK;
}

int dvd_union_scatter(const void* D, void* depth_1, void* depth_2, const int* u1, const int* u2, int B, int U_pad,
                      long long bytes_per_row, dvd_stream_t stream) {
  using namespace dvd;
  DVD_REQUIRE(D && depth_1 && depth_2 && u1 && u2, "union_scatter: null pointer");
  DVD_REQUIRE(U_pad > 0 && B > 0 && bytes_per_row > 0, "union_scatter: empty union / batch / row");
  const uintptr_t s = (uintptr_t)D, d1 = (uintptr_t)depth_1, d2 = (uintptr_t)depth_2;
  const uintptr_t bits = s | d1 | d2 | (uintptr_t)bytes_per_row;
  DVD_REQUIRE((bits & 3) == 0, "union_scatter: rows of dwords need 4-byte alignment");
  const unsigned long long src_span = (unsigned long long)bytes_per_row * U_pad, dst_span = (unsigned long long)bytes_per_row * B;
  DVD_REQUIRE(disjoint(s, src_span, d1, dst_span) && disjoint(s, src_span, d2, dst_span) && disjoint(d1, dst_span, d2, dst_span),
              "union_scatter: the union and the two destinations must not overlap");
  int vec, tpr, grid;
  DVD_REQUIRE(union_shape(bits, bytes_per_row, 2LL * B, &vec, &tpr, &grid), "union_scatter: too much work for one launch");
  bytes_add(DVD_BYTES_GATHER, 4.0 * (double)dst_span + 8.0 * B);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const char* a = static_cast<const char*>(D);
  if (vec == 16)
    hipLaunchKernelGGL(union_scatter_kernel<uint4>, dim3(grid), dim3(256), 0, st, a, static_cast<char*>(depth_1),
                       static_cast<char*>(depth_2), u1, u2, B, U_pad, bytes_per_row, tpr);
  else
    hipLaunchKernelGGL(union_scatter_kernel<unsigned>, dim3(grid), dim3(256), 0, st, a, static_cast<char*>(depth_1),
                       static_cast<char*>(depth_2), u1, u2, B, U_pad, bytes_per_row, tpr);
  DVD_LAUNCH_OK();
  return DVD_OK;
}

int dvd_union_reduce(const float* g_d1, const float* g_d2, float* G, const int* offsets, const int* entries, int U_pad, int B,
                     long long floats_per_row, dvd_stream_t stream) {
  using namespace dvd;
  DVD_REQUIRE(g_d1 && g_d2 && G && offsets && entries, "union_reduce: null pointer");
  DVD_REQUIRE(U_pad > 0 && B > 0 && floats_per_row > 0, "union_reduce: empty union / batch / row");
  DVD_REQUIRE(B < (1 << 29), "union_reduce: %d pairs", B);
  const long long bpr = floats_per_row * 4;
  const uintptr_t s1 = (uintptr_t)g_d1, s2 = (uintptr_t)g_d2, d = (uintptr_t)G;
  const uintptr_t bits = s1 | s2 | d | (uintptr_t)bpr;
  DVD_REQUIRE((bits & 3) == 0, "union_reduce: fp32 rows need 4-byte alignment");
  const unsigned long long src_span = (unsigned long long)bpr * B, dst_span = (unsigned long long)bpr * U_pad;
  DVD_REQUIRE(disjoint(d, dst_span, s1, src_span) && disjoint(d, dst_span, s2, src_span), "union_reduce: G overlaps a source");
  int vec, tpr, grid;
  DVD_REQUIRE(union_shape(bits, bpr, U_pad, &vec, &tpr, &grid), "union_reduce: too much work for one launch");
  bytes_add(DVD_BYTES_GATHER, 2.0 * (double)src_span + (double)dst_span + 4.0 * (U_pad + 1 + 2.0 * B));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const char *a = reinterpret_cast<const char*>(g_d1), *b = reinterpret_cast<const char*>(g_d2);
  if (vec == 16)
    hipLaunchKernelGGL(union_reduce_kernel<float4>, dim3(grid), dim3(256), 0, st, a, b, reinterpret_cast<char*>(G), offsets,
                       entries, U_pad, B, bpr, tpr);
  else
    hipLaunchKernelGGL(union_reduce_kernel<float>, dim3(grid), dim3(256), 0, st, a, b, reinterpret_cast<char*>(G), offsets,
                       entries, U_pad, B, bpr, tpr);
  DVD_LAUNCH_OK();
  return DVD_OK;
}

}  // extern "C"
