// Forward bilinear splat of world points into target cameras, with a soft z-buffer (gfx950).
//
// The scatter that goes with dvd_track_project's gather (csrc/track.hip): every source pixel carries a world point and C
// values; the point is projected into the camera of its image's target view exactly as track.hip projects it,
//     I = ((P - t) @ R) @ K_T ;  z = I.z ;  (u, v) = I.xy / (z + 1e-8)
// (project_point of track_cam.h, -ffp-contract=off), and its values are spread over the four pixels around (u, v) with the
// bilinear weights.  Among the points that reach a pixel only those within z_tol of the nearest one are blended.
//
// Three launches over a workspace that the caller clears (zbuf to 0xFF bytes, acc to 0):
//   dvd_splat_zmin        zbuf[V,H,W] (unsigned int) <- atomicMin of the bit pattern of z over the counting taps.  z > z_near
//                         >= 0, so z is a positive float and positive floats order as their bit patterns.
//   dvd_splat_accumulate  the same projection again (bit-identical z); a counting tap with z <= zmin * (1 + z_tol) adds
//                         llrintf(ldexpf(x, shift)) for x = w and x = w * clamp(c, +-value_bound) / value_bound, c = 0 .. C-1,
//                         into the C + 1 contiguous 64-bit words acc[V,H,W,C+1] of its pixel, by integer atomicAdd.
//   dvd_splat_resolve     one writer per target pixel: weight = acc_w * 2^-shift, hit = weight >= w_min, image = value_bound *
//                         acc_c / acc_w where hit (fill elsewhere), depth = zmin where hit (0 elsewhere).
//
// Integer min and integer add commute and are exact, so the result does not depend on the order in which points, blocks,
// source images or launches arrive: two runs give the same bits.  No float atomics.  Overflow cannot happen: |x| <= 1, so a
// term is at most 2^shift in magnitude, a pixel receives at most one tap of each point, and the caller states a bound n_max on
// the points one view receives with shift <= 62 - ceil_log2(n_max): |sum| <= 2^62.  shift <= 40 keeps ldexpf and llrintf
// exact for fp32 terms that are not tiny; what is dropped below 2^-shift is the quantisation the tests account for.
//
// A point is live iff its valid byte is set (or there is no valid map), all its values are finite, z > z_near, z is finite
// and -1 < u < W, -1 < v < H.  All of that is decided in float, with comparisons that are false for a NaN, before anything is
// converted to an integer: for a live point floor(u) is in [-1, W-1] and floor(v) in [-1, H-1], and every tap is tested
// against the image before it is addressed.  A tap counts iff it is inside the image and its weight is >= w_tap.
// One thread per source pixel, grid (pixels, S): the view of an image and its camera are uniform over a block.  An image
// whose view is < 0 or >= V is skipped: nothing of it is read and nothing written.

#include <float.h>

#include "track_cam.h"
#include "warp_pixel.h"

namespace dvd {

constexpr int kSplatMaxC = 8;

struct SplatArgs {
  const float* points;            // [S,3,H,W] (planar) or [S,H,W,3]
  const float* values;            // [S,C,H,W]
  const unsigned char* valid;     // [S,H,W] or null
  const int* view;                // [S]
  const float *R, *t, *K;         // [V,3,3], [V,3], [V,3,3]
  unsigned int* zbuf;             // [V,H,W]
  unsigned long long* acc;        // [V,H,W,C+1]
  int V, C, H, W, HW, shift;
  float z_near, z_tol, w_tap, value_bound, wf, hf;
};

struct SplatTaps {
  float z;
  int x0, y0;          // the north-west tap; the others are +1 in x and / or y
  float w[4];          // NW, NE, SW, SE
  float val[kSplatMaxC];
};

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= FLT_MAX; }      // false for NaN and +-inf

// Source pixel p of image s: is the point live, and if so its depth, taps, weights and values.  The ONE function both
// passes go through, so both see the same bits.
template <bool PLANAR>
__device__ __forceinline__ bool splat_point(const SplatArgs& a, const TrackCam& c, int s, int p, SplatTaps& tp) {
  const size_t pix = (size_t)s * a.HW + p;
  if (a.valid && a.valid[pix] == 0) return false;
  bool ok = true;
#pragma unroll
  for (int ch = 0; ch < kSplatMaxC; ++ch) {
    if (ch < a.C) {
      tp.val[ch] = a.values[((size_t)s * a.C + ch) * a.HW + p];
      ok = ok && finite_f(tp.val[ch]);
    }
  }
  if (!ok) return false;
  float P[3][1];
  load_points<1, PLANAR>(a.points, (size_t)s, p, a.HW, P);
  float u, v, I2;
  project_uvz(c, P[0][0], P[1][0], P[2][0], u, v, I2);
  // every comparison is false for a NaN; u, v are finite and within (-1, W) x (-1, H) behind this line
  if (!(I2 > a.z_near && finite_f(I2) && u > -1.0f && u < a.wf && v > -1.0f && v < a.hf)) return false;
  const float x0f = floorf(u), y0f = floorf(v);
  const float fx = u - x0f, fy = v - y0f;
  const float gx = 1.0f - fx, gy = 1.0f - fy;
  tp.z = I2;
  tp.x0 = (int)x0f, tp.y0 = (int)y0f;
  tp.w[0] = gx * gy, tp.w[1] = fx * gy, tp.w[2] = gx * fy, tp.w[3] = fx * fy;
  return true;
}

// tap i of a live point: inside the image and heavy enough -> its pixel index within the view, else -1
__device__ __forceinline__ int splat_tap(const SplatArgs& a, const SplatTaps& tp, int i) {
  const int x = tp.x0 + (i & 1), y = tp.y0 + (i >> 1);
  const bool in = x >= 0 && x < a.W && y >= 0 && y < a.H;
  return (in && tp.w[i] >= a.w_tap) ? y * a.W + x : -1;
}

template <bool PLANAR>
__global__ __launch_bounds__(256) void splat_zmin_kernel(const SplatArgs a) {
  const int s = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int vw = a.view[s];      // uniform over the block
  if (vw < 0 || vw >= a.V || p >= a.HW) return;
  TrackCam c;
  load_track_cam(a.R, a.t, a.K, vw, c);
  SplatTaps tp;
  if (!splat_point<PLANAR>(a, c, s, p, tp)) return;
  unsigned int* zb = a.zbuf + (size_t)vw * a.HW;
  const unsigned int zbits = __float_as_uint(tp.z);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int o = splat_tap(a, tp, i);
    if (o >= 0) atomicMin(zb + o, zbits);
  }
}

__device__ __forceinline__ unsigned long long splat_fixed(float x, int shift) {
  return (unsigned long long)llrintf(ldexpf(x, shift));      // two's complement: a negative term adds as its 64-bit wrap
}

template <bool PLANAR>
__global__ __launch_bounds__(256) void splat_accumulate_kernel(const SplatArgs a) {
  const int s = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int vw = a.view[s];
  if (vw < 0 || vw >= a.V || p >= a.HW) return;
  TrackCam c;
  load_track_cam(a.R, a.t, a.K, vw, c);
  SplatTaps tp;
  if (!splat_point<PLANAR>(a, c, s, p, tp)) return;
  const unsigned int* zb = a.zbuf + (size_t)vw * a.HW;
  unsigned long long* ac = a.acc + (size_t)vw * a.HW * (a.C + 1);
  const float tol = 1.0f + a.z_tol;
  float q[kSplatMaxC];
#pragma unroll
  for (int ch = 0; ch < kSplatMaxC; ++ch)
    q[ch] = (ch < a.C) ? fminf(fmaxf(tp.val[ch], -a.value_bound), a.value_bound) / a.value_bound : 0.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int o = splat_tap(a, tp, i);
    if (o < 0) continue;
    // pass a wrote this word with a z no larger than ours; an empty word (all ones, a NaN) accepts nothing
    const float zmin = __uint_as_float(zb[o]);
    if (!(tp.z <= zmin * tol)) continue;
    // the C + 1 words of the pixel back to back: they lie in one or two 32-byte sectors
    unsigned long long* dst = ac + (size_t)o * (a.C + 1);
    const float w = tp.w[i];
    atomicAdd(dst, splat_fixed(w, a.shift));
#pragma unroll
    for (int ch = 0; ch < kSplatMaxC; ++ch)
      if (ch < a.C) atomicAdd(dst + 1 + ch, splat_fixed(w * q[ch], a.shift));
  }
}

struct ResolveArgs {
  const unsigned int* zbuf;
  const unsigned long long* acc;
  float *image, *depth, *weight;
  unsigned char* hit;
  int V, C, HW, shift;
  float w_min, value_bound, fill;
};

template <int PX>
__global__ __launch_bounds__(256) void splat_resolve_kernel(const ResolveArgs a) {
  const int vw = blockIdx.y;
  const int p0 = (blockIdx.x * 256 + threadIdx.x) * PX;
  if (p0 >= a.HW) return;
  const size_t pix = (size_t)vw * a.HW + p0;
  float img[kSplatMaxC][PX], dep[PX], wgt[PX];
  unsigned int hit[PX];
#pragma unroll
  for (int i = 0; i < PX; ++i) {
    const unsigned long long* src = a.acc + (pix + i) * (a.C + 1);
    const long long aw = (long long)src[0];
    wgt[i] = ldexpf((float)aw, -a.shift);
    hit[i] = (wgt[i] >= a.w_min) ? 1u : 0u;
    dep[i] = hit[i] ? __uint_as_float(a.zbuf[pix + i]) : 0.0f;
#pragma unroll
    for (int ch = 0; ch < kSplatMaxC; ++ch) {
      if (ch < a.C) {
        // the quotient of two exact integers, rounded once to fp32
        const float r = hit[i] ? (float)((double)(long long)src[1 + ch] / (double)aw) : 0.0f;
        img[ch][i] = hit[i] ? a.value_bound * r : a.fill;
      }
    }
  }
#pragma unroll
  for (int ch = 0; ch < kSplatMaxC; ++ch) {
    if (ch < a.C) stpx<PX>(a.image + ((size_t)vw * a.C + ch) * a.HW + p0, img[ch]);
  }
  stpx<PX>(a.depth + pix, dep);
  stpx<PX>(a.weight + pix, wgt);
  stpx_bytes<PX>(a.hit + pix, hit);
}

static int splat_shape_ok(const char* who, int V, int C, int H, int W) {
  DVD_REQUIRE(V > 0 && V <= 65535, "%s: bad number of views V=%d", who, V);
  DVD_REQUIRE(C >= 1 && C <= kSplatMaxC, "%s: C=%d values per point, 1 .. %d are supported", who, C, kSplatMaxC);
  DVD_REQUIRE(H >= 2 && W >= 2 && (long long)H * W < (1LL << 30), "%s: bad image size H=%d W=%d", who, H, W);
  return DVD_OK;
}

static int splat_source_ok(const char* who, int S, float z_near, float w_tap) {
  DVD_REQUIRE(S > 0 && S <= 65535, "%s: bad number of source images S=%d", who, S);
  DVD_REQUIRE(z_near >= 0.0f && z_near <= FLT_MAX, "%s: z_near=%g must be finite and >= 0", who, (double)z_near);
  DVD_REQUIRE(w_tap > 0.0f && w_tap <= 0.25f, "%s: w_tap=%g must be in (0, 0.25]", who, (double)w_tap);
  return DVD_OK;
}

}  // namespace dvd

extern "C" {

size_t dvd_splat_workspace_bytes(int V, int C, int H, int W) {
  if (V <= 0 || C < 1 || C > dvd::kSplatMaxC || H < 2 || W < 2) return 0;
  return (size_t)V * H * W * (sizeof(unsigned int) + (size_t)(C + 1) * sizeof(unsigned long long));
}

int dvd_splat_zmin(const float* points, int points_planar, const float* values, const unsigned char* valid, const int* view,
                   const float* R, const float* t, const float* K_T, int V, unsigned int* zbuf, int S, int C, int H, int W,
                   float z_near, float w_tap, dvd_stream_t stream) {
  using namespace dvd;
  DVD_REQUIRE(points && values && view && R && t && K_T && zbuf, "splat_zmin: null pointer");
  if (int st = splat_shape_ok("splat_zmin", V, C, H, W)) return st;
  if (int st = splat_source_ok("splat_zmin", S, z_near, w_tap)) return st;
  SplatArgs a = {};
  a.points = points, a.values = values, a.valid = valid, a.view = view, a.R = R, a.t = t, a.K = K_T, a.zbuf = zbuf;
  a.V = V, a.C = C, a.H = H, a.W = W, a.HW = H * W, a.z_near = z_near, a.w_tap = w_tap, a.wf = (float)W, a.hf = (float)H;
  bytes_add(DVD_BYTES_GEOMETRY, (double)S * a.HW * (12.0 + 4.0 * C + (valid ? 1.0 : 0.0) + 4 * 4.0));
  dim3 grid((a.HW + 255) / 256, S), block(256);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (points_planar)
    hipLaunchKernelGGL((splat_zmin_kernel<true>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((splat_zmin_kernel<false>), grid, block, 0, s, a);
  DVD_LAUNCH_OK();
  return DVD_OK;
}

int dvd_splat_accumulate(const float* points, int points_planar, const float* values, const unsigned char* valid,
                         const int* view, const float* R, const float* t, const float* K_T, int V, const unsigned int* zbuf,
                         unsigned long long* acc, int S, int C, int H, int W, float z_near, float z_tol, float w_tap,
                         float value_bound, int shift, long long n_max, dvd_stream_t stream) {
  using namespace dvd;
  DVD_REQUIRE(points && values && view && R && t && K_T && zbuf && acc, "splat_accumulate: null pointer");
  if (int st = splat_shape_ok("splat_accumulate", V, C, H, W)) return st;
  if (int st = splat_source_ok("splat_accumulate", S, z_near, w_tap)) return st;
  DVD_REQUIRE(z_tol >= 0.0f && z_tol <= FLT_MAX, "splat_accumulate: z_tol=%g must be finite and >= 0", (double)z_tol);
  DVD_REQUIRE(value_bound > 0.0f && value_bound <= FLT_MAX, "splat_accumulate: value_bound=%g must be finite and > 0",
              (double)value_bound);
  DVD_REQUIRE(shift >= 1 && shift <= 40, "splat_accumulate: shift=%d outside 1 .. 40", shift);
  // the sum of n_max terms of magnitude <= 2^shift must stay below 2^62
  DVD_REQUIRE(n_max >= 1 && n_max < (1LL << 61) && shift + ceil_log2(n_max) <= 62,
              "splat_accumulate: shift=%d overflows 64 bits for n_max=%lld points per view", shift, n_max);
  SplatArgs a = {};
  a.points = points, a.values = values, a.valid = valid, a.view = view, a.R = R, a.t = t, a.K = K_T;
  a.zbuf = const_cast<unsigned int*>(zbuf), a.acc = acc;
  a.V = V, a.C = C, a.H = H, a.W = W, a.HW = H * W, a.shift = shift;
  a.z_near = z_near, a.z_tol = z_tol, a.w_tap = w_tap, a.value_bound = value_bound, a.wf = (float)W, a.hf = (float)H;
  bytes_add(DVD_BYTES_GEOMETRY, (double)S * a.HW * (12.0 + 4.0 * C + (valid ? 1.0 : 0.0) + 4 * (4.0 + 8.0 * (C + 1))));
  dim3 grid((a.HW + 255) / 256, S), block(256);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (points_planar)
    hipLaunchKernelGGL((splat_accumulate_kernel<true>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((splat_accumulate_kernel<false>), grid, block, 0, s, a);
  DVD_LAUNCH_OK();
  return DVD_OK;
}

int dvd_splat_resolve(const unsigned int* zbuf, const unsigned long long* acc, int V, int C, int H, int W, int shift,
                      float w_min, float value_bound, float fill, float* image, float* depth, float* weight,
                      unsigned char* hit, dvd_stream_t stream) {
  using namespace dvd;
  DVD_REQUIRE(zbuf && acc && image && depth && weight && hit, "splat_resolve: null pointer");
  if (int st = splat_shape_ok("splat_resolve", V, C, H, W)) return st;
  DVD_REQUIRE(shift >= 1 && shift <= 40, "splat_resolve: shift=%d outside 1 .. 40", shift);
  DVD_REQUIRE(w_min > 0.0f && w_min <= FLT_MAX, "splat_resolve: w_min=%g must be finite and > 0", (double)w_min);
  DVD_REQUIRE(value_bound > 0.0f && value_bound <= FLT_MAX, "splat_resolve: value_bound=%g must be finite and > 0",
              (double)value_bound);
  ResolveArgs a = {};
  a.zbuf = zbuf, a.acc = acc, a.image = image, a.depth = depth, a.weight = weight, a.hit = hit;
  a.V = V, a.C = C, a.HW = H * W, a.shift = shift, a.w_min = w_min, a.value_bound = value_bound, a.fill = fill;
  bytes_add(DVD_BYTES_GEOMETRY, (double)V * a.HW * (4.0 + 8.0 * (C + 1) + 4.0 * (C + 2) + 1.0));
  const bool v4 = (W % 4 == 0) && aligned_to(zbuf, 16) && aligned_to(acc, 16) && aligned_to(image, 16) &&
                  aligned_to(depth, 16) && aligned_to(weight, 16) && aligned_to(hit, 16);
  const int px = v4 ? 4 : 1;
  dim3 grid((a.HW + 256 * px - 1) / (256 * px), V), block(256);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (v4)
    hipLaunchKernelGGL((splat_resolve_kernel<4>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((splat_resolve_kernel<1>), grid, block, 0, s, a);
  DVD_LAUNCH_OK();
  return DVD_OK;
}

}  // extern "C"
