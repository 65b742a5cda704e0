// What the post-processing units share beyond the projection (track_cam.h, track_sample.h): the host's alignment and log2
// helpers, the PX-wide loads and stores of a thread that owns 4 horizontally adjacent pixels or one, the exact fixed-point block
// sums of eval.hip and depth_score.hip, and the median of a column held in LDS of track_filter.hip and triangulate.hip.  One copy
// each, so that units which promise one another the same bits get them from the same function.
#pragma once

#include <stdint.h>

#include "dvd_io.h"

namespace dvd {

// n a power of two; a null pointer is aligned to anything (an optional tensor never decides the vector path)
inline bool aligned_to(const void* p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

inline int ceil_log2(long long n) {
  int k = 0;
  while ((1LL << k) < n) ++k;
  return k;
}

// PX = 4: one 16-byte access (floats) or one dword (bytes), the base aligned to it; PX = 1: one element
template <int PX>
__device__ __forceinline__ void ldpx(const float* src, float v[PX]) {
  if (PX == 4)
    *reinterpret_cast<float4*>(v) = ld4(src);
  else
    v[0] = src[0];
}

template <int PX>
__device__ __forceinline__ void stpx(float* dst, const float v[PX]) {
  if (PX == 4)
    st4(dst, make_float4(v[0], v[1], v[2], v[3]));
  else
    dst[0] = v[0];
}

template <int PX>
__device__ __forceinline__ void ldpx_bytes(const unsigned char* src, unsigned int v[PX]) {
  if (PX == 4) {
    const unsigned int m4 = *reinterpret_cast<const unsigned int*>(src);
    v[0] = m4 & 255u, v[1] = (m4 >> 8) & 255u, v[2] = (m4 >> 16) & 255u, v[3] = m4 >> 24;
  } else {
    v[0] = src[0];
  }
}

// (every v[i] <= 255)
template <int PX>
__device__ __forceinline__ void stpx_bytes(unsigned char* dst, const unsigned int v[PX]) {
  if (PX == 4)
    *reinterpret_cast<unsigned int*>(dst) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
  else
    dst[0] = (unsigned char)v[0];
}

// q(x) = llrint(x * 2^shift), scale = 2^shift: the term of an exact integer sum
__device__ __forceinline__ long long fixed_q(float x, double scale) { return llrint((double)x * scale); }

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
  return v;
}

// dst[k] += the sum of acc[k] over a block of 256 threads, k < K <= 256: a shuffle tree over the 64 lanes, LDS across the four
// waves, then one integer atomicAdd per non-zero word.  Every thread of the block calls it (it holds a barrier).
template <int K>
__device__ __forceinline__ void block_add_i64(const long long acc[K], unsigned long long* dst) {
  __shared__ long long red[4][K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const long long v = wave_sum_i64(acc[k]);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    const long long v = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    if (v != 0) atomicAdd(dst + threadIdx.x, (unsigned long long)v);
  }
}

// np.median of the n values q[0], q[stride], ..., q[(n - 1) * stride] (a thread's own column of LDS), `empty` for n == 0: the
// elements of rank (n - 1) / 2 and n / 2 by rank counting, n^2 reads; equal values are ordered by their position
__device__ __forceinline__ float column_median(const float* q, int stride, int n, float empty) {
  const int m_lo = (n - 1) >> 1, m_hi = n >> 1;
  float e_lo = empty, e_hi = empty;
  for (int j = 0; j < n; ++j) {
    const float e = q[j * stride];
    int rank = 0;
    for (int l = 0; l < n; ++l) {
      const float f = q[l * stride];
      rank += (f < e || (f == e && l < j)) ? 1 : 0;
    }
    e_lo = rank == m_lo ? e : e_lo;
    e_hi = rank == m_hi ? e : e_hi;
  }
  return (n & 1) ? e_lo : (e_lo + e_hi) * 0.5f;
}

}  // namespace dvd
