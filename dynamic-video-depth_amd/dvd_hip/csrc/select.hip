// The exact median of num / den per segment: an order statistic on the device, without a sort and without a key array (gfx950)
//
// What it serves (reference, /root/reference): scripts/preprocess/shutterstock/generate_frame_midas.py:153-160 --
// `scales.append(np.median(nn_depth[idx, idy] / mvs_depth[idx, idy]))` over `np.where(mvs_depth > 1e-3)` -- and the median
// alignment of a predicted depth to its ground truth (models/score_depth.py).
//
// An element of segment s is selected iff den > den_min (a NaN fails) and its mask byte, if a mask is given, is non-zero.  Its
// key is the correctly rounded fp32 quotient num / den (IEEE division; the unit is built with -ffp-contract=off).  With the n
// selected quotients sorted, the result is numpy's median, bit for bit: v[(n-1)/2] for odd n, (v[n/2-1] + v[n/2]) / 2 with the
// sum formed first in fp32 for even n, NaN for n = 0 and NaN if any selected quotient is a NaN; +-inf sort as the extremes.
//
// Most-significant-digit radix select, four passes of 8 bits over the order-preserving uint32 image of the key, following the
// two ranks n/2-1 (n/2 for odd n) and n/2 at once:
//   hist pass p   re-reads num, den and the mask (8-9 B per element), recomputes the quotient and keeps the elements whose top
//                 8 p bits equal the prefix a rank has fixed so far; their next digit is counted in a block-private LDS histogram
//                 of 32-bit counters (2 x 256; one table serves both ranks while their prefixes agree), and the non-zero bins are
//                 added to the segment's table in global memory with 32-bit integer atomics.  Pass 0 also counts the NaNs.
//   pick pass p   one block per segment scans the 256 bins, fixes the next digit of both ranks and their remaining ranks on the
//                 device; pass 0 first derives n and the two ranks from the total, pass 3 writes median and count.
// Nothing synchronises with the host and no rank leaves the device.  Only integers are added, so the result is the same bits
// from run to run and for every grid.  A launch has at most kSelectMaxBlocks blocks; a block walks the rest of its segment
// grid-stride.  Counts stay below 2^31 (S * L < 2^31 is required), so 32-bit counters cannot overflow.

#include <stdint.h>

#include "dvd_post.h"

namespace dvd {

constexpr int kSelectMaxBlocks = 2048;      // blocks of 256 threads per histogram launch, over all segments
constexpr int kSelectBins = 256;
constexpr int kSelectPasses = 4;
constexpr int kSelectStateWords = 8;        // prefix[2], rank[2], n, n_nan, 2 spare
constexpr int kSelectSegWords = kSelectStateWords + kSelectPasses * 2 * kSelectBins;
static_assert(kSelectSegWords * 4 == DVD_RATIO_MEDIAN_WORKSPACE_PER_SEGMENT, "workspace size of dvd_hip.h");

// per segment in the workspace: state words, then hist[pass][rank][bin]
__device__ __forceinline__ unsigned int* select_state(unsigned int* ws, int s) { return ws + (size_t)s * kSelectSegWords; }
__device__ __forceinline__ unsigned int* select_hist(unsigned int* ws, int s, int pass) {
  return ws + (size_t)s * kSelectSegWords + kSelectStateWords + pass * 2 * kSelectBins;
}

// order-preserving image of an fp32 value: negative values are flipped entirely, the others get the sign bit set
__device__ __forceinline__ unsigned int select_key(float q) {
  const unsigned int u = __float_as_uint(q);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float select_value(unsigned int k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

template <int PX, bool MASK>
__global__ __launch_bounds__(256) void ratio_hist_kernel(const float* __restrict__ num, const float* __restrict__ den,
                                                         const unsigned char* __restrict__ mask, float den_min, long long L,
                                                         unsigned int* __restrict__ ws, int pass) {
  __shared__ unsigned int bins[2][kSelectBins];
  __shared__ unsigned int n_nan;
  const int s = blockIdx.y;
  bins[0][threadIdx.x] = 0u, bins[1][threadIdx.x] = 0u;
  if (threadIdx.x == 0) n_nan = 0u;
  const unsigned int* st = select_state(ws, s);
  const unsigned int pre0 = st[0], pre1 = st[1];      // written by the pick kernel of the pass before (zero in pass 0)
  const bool split = pre0 != pre1;                    // uniform over the segment
  const int shift = 24 - 8 * pass;
  __syncthreads();
  const size_t base = (size_t)s * (size_t)L;
  unsigned int nans = 0u;
  for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * PX; i < L; i += (long long)gridDim.x * 256 * PX) {
    float a[PX], b[PX];
    unsigned int m[PX];
    ldpx<PX>(num + base + i, a);      // PX == 4: L % 4 == 0 and 16-byte aligned bases, so i + 3 < L
    ldpx<PX>(den + base + i, b);
    if (MASK) ldpx_bytes<PX>(mask + base + i, m);
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      if (!(b[k] > den_min) || (MASK && m[k] == 0u)) continue;
      const float q = a[k] / b[k];
      if (q != q) ++nans;       // (still binned, so that n counts it; the result is NaN whatever its rank)
      const unsigned int key = select_key(q);
      const unsigned int digit = (key >> shift) & 255u;
      const unsigned int top = pass == 0 ? 0u : key >> (shift + 8);
      if (top == pre0) atomicAdd(&bins[0][digit], 1u);
      if (split && top == pre1) atomicAdd(&bins[1][digit], 1u);
    }
  }
  if (pass == 0 && nans) atomicAdd(&n_nan, nans);
  __syncthreads();
  unsigned int* hist = select_hist(ws, s, pass);
  const unsigned int c0 = bins[0][threadIdx.x], c1 = bins[1][threadIdx.x];
  if (c0) atomicAdd(hist + threadIdx.x, c0);
  if (c1) atomicAdd(hist + kSelectBins + threadIdx.x, c1);
  if (pass == 0 && threadIdx.x == 0 && n_nan) atomicAdd(select_state(ws, s) + 5, n_nan);
}

// One block per segment; thread j < 2 follows rank j.
__global__ __launch_bounds__(256) void ratio_pick_kernel(unsigned int* __restrict__ ws, int pass, float* __restrict__ median,
                                                         long long* __restrict__ count) {
  __shared__ unsigned int bins[2][kSelectBins];
  __shared__ unsigned int out_key[2];
  const int s = blockIdx.x;
  unsigned int* st = select_state(ws, s);
  const unsigned int* hist = select_hist(ws, s, pass);
  const bool split = st[0] != st[1];
  bins[0][threadIdx.x] = hist[threadIdx.x];
  bins[1][threadIdx.x] = hist[(split ? kSelectBins : 0) + threadIdx.x];
  __syncthreads();
  if (threadIdx.x < 2) {
    const int j = threadIdx.x;
    unsigned int rank;
    if (pass == 0) {
      unsigned int n = 0u;
      for (int d = 0; d < kSelectBins; ++d) n += bins[0][d];
      if (j == 0) st[4] = n;
      rank = (j == 0 && !(n & 1u) && n > 0u) ? n / 2u - 1u : n / 2u;
    } else {
      rank = st[2 + j];
    }
    // the bin that holds the rank: the last one if none before it does (always the case for a live rank; n = 0 ends there too)
    unsigned int below = 0u;
    int d = 0;
    for (; d < kSelectBins - 1; ++d) {
      const unsigned int c = bins[j][d];
      if (rank < below + c) break;
      below += c;
    }
    const unsigned int prefix = (st[j] << 8) | (unsigned int)d;
    out_key[j] = prefix;
    // (st[0] and st[1] were both read into `split` above the barrier; below it thread j alone reads and writes st[j], st[2 + j])
    st[j] = prefix;
    st[2 + j] = rank >= below ? rank - below : 0u;
  }
  __syncthreads();
  if (pass == kSelectPasses - 1 && threadIdx.x == 0) {
    const unsigned int n = st[4], n_nan = st[5];
    float r;
    if (n == 0u || n_nan != 0u) {
      r = __uint_as_float(0x7FC00000u);
    } else {
      const float lo = select_value(out_key[0]), hi = select_value(out_key[1]);
      r = (n & 1u) ? hi : (lo + hi) / 2.0f;
    }
    median[s] = r;
    count[s] = (long long)n;
  }
}

template <int PX>
static void select_hist_launch(bool with_mask, dim3 grid, hipStream_t st, const float* num, const float* den,
                               const unsigned char* mask, float den_min, long long L, unsigned int* ws, int pass) {
  if (with_mask)
    hipLaunchKernelGGL((ratio_hist_kernel<PX, true>), grid, dim3(256), 0, st, num, den, mask, den_min, L, ws, pass);
  else
    hipLaunchKernelGGL((ratio_hist_kernel<PX, false>), grid, dim3(256), 0, st, num, den, mask, den_min, L, ws, pass);
}

}  // namespace dvd

extern "C" {

int dvd_ratio_median(const float* num, const float* den, const unsigned char* mask, float den_min, int S, long long L,
                     float* median, long long* count, void* workspace, size_t workspace_bytes, dvd_stream_t stream) {
  using namespace dvd;
  DVD_REQUIRE(num && den && median && count && workspace, "ratio_median: null pointer");
  DVD_REQUIRE(S > 0 && S <= 65535 && L > 0, "ratio_median: bad sizes S=%d L=%lld", S, L);
  DVD_REQUIRE(L < (1LL << 31) && (long long)S * L < (1LL << 31), "ratio_median: S * L = %d * %lld must stay below 2^31", S, L);
  DVD_REQUIRE(den_min == den_min, "ratio_median: den_min is NaN");
  DVD_REQUIRE(aligned_to(num, 4) && aligned_to(den, 4) && aligned_to(median, 4) && aligned_to(count, 8) &&
                  aligned_to(workspace, 4),
              "ratio_median: misaligned pointer (num, den, median, workspace: 4 bytes; count: 8 bytes)");
  DVD_REQUIRE(workspace_bytes >= (size_t)S * DVD_RATIO_MEDIAN_WORKSPACE_PER_SEGMENT,
              "ratio_median: workspace of %zu bytes below S * %d", workspace_bytes, DVD_RATIO_MEDIAN_WORKSPACE_PER_SEGMENT);
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned int* ws = static_cast<unsigned int*>(workspace);
  const int rc = zero_words(ws, S * kSelectSegWords, st);
  if (rc != DVD_OK) return rc;
  const bool v4 = (L % 4 == 0) && aligned_to(num, 16) && aligned_to(den, 16) && aligned_to(mask, 4);
  const int px = v4 ? 4 : 1;
  long long bx = (L + 256 * px - 1) / (256 * px);
  const long long cap = kSelectMaxBlocks / S > 1 ? kSelectMaxBlocks / S : 1;
  if (bx > cap) bx = cap;
  dim3 grid((unsigned)bx, (unsigned)S);
  bytes_add(DVD_BYTES_GEOMETRY, (double)kSelectPasses * (double)S * (double)L * (mask ? 9.0 : 8.0));
  for (int pass = 0; pass < kSelectPasses; ++pass) {
    if (v4)
      select_hist_launch<4>(mask != nullptr, grid, st, num, den, mask, den_min, L, ws, pass);
    else
      select_hist_launch<1>(mask != nullptr, grid, st, num, den, mask, den_min, L, ws, pass);
    hipLaunchKernelGGL(ratio_pick_kernel, dim3((unsigned)S), dim3(256), 0, st, ws, pass, median, count);
  }
  DVD_LAUNCH_OK();
  return DVD_OK;
}

}  // extern "C"
