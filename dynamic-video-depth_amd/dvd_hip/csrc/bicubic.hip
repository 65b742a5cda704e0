// Bicubic resize of fp32 planes (align_corners=True) and its backward (gfx950).
//
// What it replaces: the two F.interpolate(mode='bicubic', align_corners=True) calls with which the reference's MidasNet
// works at a resolution of its own (third_party/MiDaS.py:221-222 on the normalised image, :244-245 on the depth), and --
// fused into the taps of the first one -- the input normalisation (x - mean) / std of :213-218.
// Arithmetic follows ATen's upsample_bicubic2d in fp32 (this unit is built with -ffp-contract=off):
//   scale = (in - 1) / (out - 1) (0 if out == 1);  src = scale * dst, i = floor(src), t = src - i;
//   taps i-1 .. i+2 clamped into [0, in-1];  A = -0.75:
//   w0 = ((A u - 5A) u + 8A) u - 4A, u = t + 1;     w1 = ((A + 2) u - (A + 3)) u u + 1, u = t;
//   w2 = w1's form with u = 1 - t;                   w3 = w0's form with u = (1 - t) + 1;
//   a row is x0 w0 + x1 w1 + x2 w2 + x3 w3, the result the same expression over the four row values.
//
// Roofline: HBM -- one read of the input planes, one write of the output planes; the 16 taps of an output pixel are
// L1/L2 resident (neighbouring threads read neighbouring columns of the same four rows).
// Backward: gx = A^T gy in GATHER form, separable: pass 1 sums over the output rows that read an input row
// (tmp[p][iy][ox]), pass 2 over the output columns that read an input column.  Every element is one thread's sum in
// ascending output order: no atomics, no memset, independent of the grid, bit-identical from call to call.  Because of the
// border clamp, index 0 and index in-1 collect the taps that fell outside.  Any ratio of sizes is legal: the candidate
// outputs of an input index are a bracket computed from 1 / scale (a margin wider than its rounding error), and every
// candidate is then tested EXACTLY with the forward's own index arithmetic, so the bracket only has to be wide enough.

#include "dvd_common.h"

namespace dvd {

struct CAxis {
  int n_in, n_out;
  float scale;
};

// ATen's get_cubic_upsample_coefficients
__device__ __forceinline__ void cubic_weights(float t, float (&w)[4]) {
  const float A = -0.75f;
  const float x1 = t;
  const float u0 = x1 + 1.0f;
  w[0] = ((A * u0 - 5.0f * A) * u0 + 8.0f * A) * u0 - 4.0f * A;
  w[1] = ((A + 2.0f) * x1 - (A + 3.0f)) * x1 * x1 + 1.0f;
  const float x2 = 1.0f - t;
  const float u3 = x2 + 1.0f;
  w[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
  w[3] = ((A * u3 - 5.0f * A) * u3 + 8.0f * A) * u3 - 4.0f * A;
}

// the four (clamped) taps of output index dst and their weights
__device__ __forceinline__ void cubic_taps(const CAxis& a, int dst, int (&idx)[4], float (&w)[4]) {
  const float src = a.scale * (float)dst;
  const float fl = floorf(src);
  cubic_weights(src - fl, w);
  const int i = (int)fl;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int j = i - 1 + k;
    j = j < 0 ? 0 : j;
    idx[k] = j < a.n_in - 1 ? j : a.n_in - 1;
  }
}

// One thread per output pixel, columns fastest.  mean / std: per-channel constants or null (both or neither).
__global__ __launch_bounds__(256) void bicubic_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, CAxis ay, CAxis ax,
                                                          unsigned total, const float* __restrict__ mean,
                                                          const float* __restrict__ stdv, int channels) {
  const unsigned idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const unsigned row = idx / (unsigned)ax.n_out;               // plane * H_out + oy
  const int ox = (int)(idx - row * (unsigned)ax.n_out);
  const unsigned p = row / (unsigned)ay.n_out;
  const int oy = (int)(row - p * (unsigned)ay.n_out);
  int xi[4], yi[4];
  float wx[4], wy[4];
  cubic_taps(ax, ox, xi, wx);
  cubic_taps(ay, oy, yi, wy);
  const bool norm = mean != nullptr;
  float m = 0.0f, s = 1.0f;
  if (norm) {
    const int c = (int)(p % (unsigned)channels);
    m = mean[c];
    s = stdv[c];
  }
  const float* plane = x + (size_t)p * ay.n_in * ax.n_in;
  float r[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float* rp = plane + (size_t)yi[k] * ax.n_in;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = rp[xi[j]];
      if (norm) v[j] = (v[j] - m) / s;        // a true division, as the reference's (x - mean) / std
    }
    r[k] = v[0] * wx[0] + v[1] * wx[1] + v[2] * wx[2] + v[3] * wx[3];
  }
  y[idx] = r[0] * wy[0] + r[1] * wy[1] + r[2] * wy[2] + r[3] * wy[3];
}

// Outputs that can read input index i: those with floor(scale * o) in [i-2, i+1], at the borders also everything below /
// above (the clamp).  [lo, hi] is a superset, clipped to the axis.
__device__ __forceinline__ void dst_bracket(const CAxis& a, int i, int& lo, int& hi) {
  lo = 0;
  hi = a.n_out - 1;
  if (a.scale > 0.0f) {
    const float inv = 1.0f / a.scale;
    if (i > 0) {
      const float l = floorf(((float)i - 2.0f) * inv) - 2.0f;
      lo = l > 0.0f ? (l < (float)hi ? (int)l : hi) : 0;
    }
    if (i < a.n_in - 1) {
      const float h = ceilf(((float)i + 2.0f) * inv) + 2.0f;
      hi = h < (float)hi ? (int)h : hi;
    }
  }
}

// the weight with which output index o reads input index i (0 if it does not)
__device__ __forceinline__ float tap_weight(const CAxis& a, int o, int i) {
  int idx[4];
  float w[4];
  cubic_taps(a, o, idx, w);
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) s += idx[k] == i ? w[k] : 0.0f;
  return s;
}

// pass 1: tmp[p][iy][ox] = sum over oy of wy(oy -> iy) * gy[p][oy][ox];  one thread per tmp element, ox fastest
__global__ __launch_bounds__(256) void bicubic_bwd_rows_kernel(const float* __restrict__ gy, float* __restrict__ tmp, CAxis ay,
                                                               int W_out, unsigned total) {
  const unsigned idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const unsigned row = idx / (unsigned)W_out;                  // plane * H_in + iy
  const int ox = (int)(idx - row * (unsigned)W_out);
  const unsigned p = row / (unsigned)ay.n_in;
  const int iy = (int)(row - p * (unsigned)ay.n_in);
  int lo, hi;
  dst_bracket(ay, iy, lo, hi);
  const float* g = gy + (size_t)p * ay.n_out * W_out + ox;
  float acc = 0.0f;
  for (int oy = lo; oy <= hi; ++oy) {
    const float w = tap_weight(ay, oy, iy);
    if (w != 0.0f) acc += w * g[(size_t)oy * W_out];
  }
  tmp[idx] = acc;
}

// pass 2: gx[p][iy][ix] = sum over ox of wx(ox -> ix) * tmp[p][iy][ox];  one thread per gx element, ix fastest
__global__ __launch_bounds__(256) void bicubic_bwd_cols_kernel(const float* __restrict__ tmp, float* __restrict__ gx, CAxis ax,
                                                               unsigned total) {
  const unsigned idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const unsigned row = idx / (unsigned)ax.n_in;                // plane * H_in + iy
  const int ix = (int)(idx - row * (unsigned)ax.n_in);
  int lo, hi;
  dst_bracket(ax, ix, lo, hi);
  const float* t = tmp + (size_t)row * ax.n_out;
  float acc = 0.0f;
  for (int ox = lo; ox <= hi; ++ox) {
    const float w = tap_weight(ax, ox, ix);
    if (w != 0.0f) acc += w * t[ox];
  }
  gx[idx] = acc;
}

static CAxis make_caxis(int n_in, int n_out) {
  CAxis a;
  a.n_in = n_in;
  a.n_out = n_out;
  a.scale = n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.0f;
  return a;
}

}  // namespace dvd

extern "C" {

int dvd_bicubic_fwd(const float* x, float* y, long long planes, int H_in, int W_in, int H_out, int W_out, const float* mean,
                    const float* std, int channels, dvd_stream_t stream) {
  DVD_REQUIRE(x && y, "bicubic fwd: null pointer");
  DVD_REQUIRE(planes > 0 && H_in > 0 && W_in > 0 && H_out > 0 && W_out > 0, "bicubic fwd: bad shape");
  DVD_REQUIRE((mean == nullptr) == (std == nullptr), "bicubic fwd: mean and std go together");
  DVD_REQUIRE(mean == nullptr || (channels > 0 && planes % channels == 0),
              "bicubic fwd: planes must be a multiple of the number of normalised channels");
  const long long total = planes * H_out * W_out;
  DVD_REQUIRE(total < (1LL << 32) - 256 && planes * H_in * W_in < (1LL << 32) - 256, "bicubic fwd: too large");
  dvd::bytes_add(DVD_BYTES_UPSAMPLE_FWD, (double)planes * ((double)H_in * W_in + (double)H_out * W_out) * 4);
  const dvd::CAxis ay = dvd::make_caxis(H_in, H_out), ax = dvd::make_caxis(W_in, W_out);
  hipLaunchKernelGGL(dvd::bicubic_fwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     x, y, ay, ax, (unsigned)total, mean, std, channels);
  DVD_LAUNCH_OK();
  return DVD_OK;
}

size_t dvd_bicubic_bwd_workspace_bytes(long long planes, int H_in, int W_in, int H_out, int W_out) {
  (void)W_in;
  (void)H_out;
  if (planes <= 0 || H_in <= 0 || W_out <= 0) return 0;
  return (size_t)planes * (size_t)H_in * (size_t)W_out * sizeof(float);
}

int dvd_bicubic_bwd(const float* gy, float* gx, long long planes, int H_in, int W_in, int H_out, int W_out, void* workspace,
                    size_t workspace_bytes, dvd_stream_t stream) {
  DVD_REQUIRE(gy && gx && workspace, "bicubic bwd: null pointer");
  DVD_REQUIRE(planes > 0 && H_in > 0 && W_in > 0 && H_out > 0 && W_out > 0, "bicubic bwd: bad shape");
  if (workspace_bytes < dvd_bicubic_bwd_workspace_bytes(planes, H_in, W_in, H_out, W_out)) {
    dvd::set_error("bicubic bwd: workspace too small");
    return DVD_ENOSPC;
  }
  const long long n_tmp = planes * H_in * W_out, n_gx = planes * H_in * W_in;
  DVD_REQUIRE(n_tmp < (1LL << 32) - 256 && n_gx < (1LL << 32) - 256 && planes * H_out * W_out < (1LL << 32) - 256,
              "bicubic bwd: too large");
  dvd::bytes_add(DVD_BYTES_UPSAMPLE_BWD, (double)planes * ((double)H_in * W_in + (double)H_out * W_out) * 4);
  const dvd::CAxis ay = dvd::make_caxis(H_in, H_out), ax = dvd::make_caxis(W_in, W_out);
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* tmp = static_cast<float*>(workspace);
  hipLaunchKernelGGL(dvd::bicubic_bwd_rows_kernel, dim3((unsigned)((n_tmp + 255) / 256)), dim3(256), 0, s, gy, tmp, ay, W_out,
                     (unsigned)n_tmp);
  DVD_LAUNCH_OK();
  hipLaunchKernelGGL(dvd::bicubic_bwd_cols_kernel, dim3((unsigned)((n_gx + 255) / 256)), dim3(256), 0, s, tmp, gx, ax,
                     (unsigned)n_gx);
  DVD_LAUNCH_OK();
  return DVD_OK;
}

}  // extern "C"
