// Geometry-aware temporal depth filter: every pixel's depth fused along its own two-sided 3D track (gfx950).
//
// The slab of models/tracks.py holds, for image b, the world point of every pixel of frame start[b] carried to the frames
// start[b] + k + k0, k = 0 .. T1-1 (row o = -k0 is the start frame itself).  dvd_track_project_from would write, per row, where
// the point lands (z, inside) and the depth that frame claims there (depth_at): 17 B per point and row, which a filter then
// reduces to 9 B per pixel.  Here the row loop runs inside the thread instead: each row is projected and sampled by the very
// function track.hip calls (project_sample, track_sample.h; both units built with -ffp-contract=off, so z, depth_at and inside
// are the same bits), gated, and fused in registers:
//     counts    inside && z >= z_near && D > 0 && z <= D * (1 + tol) && D <= z * (1 + tol)       r = D / z
//     row o     always counts, r = 1, no projection
//     mean      acc += w[k] * r ; ws += w[k]  in ascending k;   ratio = acc / ws
//     median    np.median of the counting samples
//     depth_out = d0 * ratio ;  spread = max r - min r ;  count = number of counting rows
// A pixel whose own depth is not > 0 (NaN included) keeps it: ratio 1, count 0, spread 0.
//
// The ratio is taken along the TARGET camera's ray (D against z) and applied along the START camera's ray (d0): the usual
// small-disagreement approximation of consistent-video-depth filters.
//
// One thread per 4 horizontally adjacent pixels where the width is a multiple of 4 and the bases are 16-byte aligned, one
// pixel per thread otherwise; grid (pixel blocks, B); each row's camera is uniform over the block.  The mean needs no sample
// storage.  The median's up to 33 samples per pixel would be a run-time indexed private array, i.e. scratch memory; they live
// in LDS instead, [T1][256] floats per block (33 KB at the cap, 9 KB at radius 4; a block of the median covers 256 pixels
// whatever the path), each pixel's column touched by its own thread only -- no barrier -- and the middle elements are picked
// by rank counting (n^2 LDS reads, n <= 33).  No atomics, every output element is written by exactly one thread with plain
// vector stores: bitwise reproducible.

#include <float.h>

#include "track_sample.h"

namespace dvd {

constexpr int kFilterMaxRows = 33;      // a window of at most 16 frames on either side
constexpr int kFilterBlockPixels = 256; // pixels per block of the median (its LDS columns)

struct FilterArgs {
  const float* points;        // [T1,B,3,H,W] (planar) or [T1,B,H,W,3]
  const int* start;           // [B]
  const float *R, *t, *K;     // [N,3,3], [N,3], [N,3,3]
  const float* depth_all;     // [N,1,H,W]
  const float* weights;       // [T1]
  float *depth_out, *ratio, *spread;   // [B,1,H,W]   (ratio, spread may be null)
  unsigned char* count;       // [B,H,W] or null
  int T1, B, N, HW, k0;
  float tl, z_near;           // 1 + tol
  TrackView view;
};

template <int PX, bool PLANAR, bool MEDIAN>
__global__ __launch_bounds__(256) void track_filter_kernel(const FilterArgs a) {
  constexpr int NT = MEDIAN ? kFilterBlockPixels / PX : 256;      // threads per block
  extern __shared__ float smp[];                                  // MEDIAN: [T1][256], column = pixel of the block
  const int b = blockIdx.y;
  const int p0 = (blockIdx.x * NT + threadIdx.x) * PX;
  if (p0 >= a.HW) return;
  const size_t pix = (size_t)b * a.HW + p0;
  const int s = a.start[b];                 // uniform over the block
  const bool live = s >= 0 && s < a.N;      // (a start that is no frame: nothing is read, the image comes out as zeros)
  const int o = -a.k0;
  const int col = threadIdx.x * PX;         // the thread's first LDS column (median)
  float d0[PX], acc[PX], ws[PX], lo[PX], hi[PX];
  int n[PX];
#pragma unroll
  for (int i = 0; i < PX; ++i) {
    d0[i] = acc[i] = ws[i] = 0.0f;
    lo[i] = INFINITY, hi[i] = -INFINITY;
    n[i] = 0;
  }
  if (live) {
    const float* ds = a.depth_all + (size_t)s * a.HW + p0;
    ldpx<PX>(ds, d0);
    const int y = p0 / a.view.W, x = p0 - y * a.view.W;
    const float yf = (float)y;
    for (int k = 0; k < a.T1; ++k) {
      float r[PX];
      bool counts[PX];
      if (k == o) {
#pragma unroll
        for (int i = 0; i < PX; ++i) r[i] = 1.0f, counts[i] = true;
      } else {
        const long long gl = (long long)s + k + a.k0;
        if (gl < 0 || gl >= (long long)a.N) continue;
        const int g = (int)gl;
        TrackCam c;
        load_track_cam(a.R, a.t, a.K, g, c);
        float P[3][PX];
        load_points<PX, PLANAR>(a.points, (size_t)k * a.B + b, p0, a.HW, P);
        const float* dg = a.depth_all + (size_t)g * a.HW;
#pragma unroll
        for (int i = 0; i < PX; ++i) {
          const TrackHit h = project_sample(c, dg, a.view, P[0][i], P[1][i], P[2][i], (float)(x + i), yf);
          counts[i] = h.in && h.z >= a.z_near && h.d > 0.0f && h.z <= h.d * a.tl && h.d <= h.z * a.tl;
          r[i] = h.d / h.z;
        }
      }
      const float w = MEDIAN ? 0.0f : a.weights[k];
#pragma unroll
      for (int i = 0; i < PX; ++i) {
        if (!counts[i]) continue;
        if (MEDIAN) {
          smp[n[i] * kFilterBlockPixels + col + i] = r[i];
        } else {
          acc[i] += w * r[i];
          ws[i] += w;
        }
        lo[i] = r[i] < lo[i] ? r[i] : lo[i];
        hi[i] = r[i] > hi[i] ? r[i] : hi[i];
        ++n[i];
      }
    }
  }
  float dep[PX], rat[PX], spr[PX];
  unsigned int cnt[PX];
#pragma unroll
  for (int i = 0; i < PX; ++i) {
    float ratio = 1.0f;
    if (live && d0[i] > 0.0f) {
      ratio = MEDIAN ? column_median(smp + col + i, kFilterBlockPixels, n[i], 1.0f) : acc[i] / ws[i];
      dep[i] = d0[i] * ratio, rat[i] = ratio, spr[i] = hi[i] - lo[i], cnt[i] = (unsigned int)n[i];
    } else {
      dep[i] = d0[i], rat[i] = 1.0f, spr[i] = 0.0f, cnt[i] = 0u;
    }
  }
  stpx<PX>(a.depth_out + pix, dep);
  if (a.ratio) stpx<PX>(a.ratio + pix, rat);
  if (a.spread) stpx<PX>(a.spread + pix, spr);
  if (a.count) stpx_bytes<PX>(a.count + pix, cnt);
}

template <int PX, bool PLANAR>
static void track_filter_launch(const FilterArgs& a, int mode, hipStream_t s) {
  if (mode == 1) {
    dim3 grid((a.HW + kFilterBlockPixels - 1) / kFilterBlockPixels, a.B), block(kFilterBlockPixels / PX);
    const size_t lds = (size_t)a.T1 * kFilterBlockPixels * sizeof(float);
    hipLaunchKernelGGL((track_filter_kernel<PX, PLANAR, true>), grid, block, lds, s, a);
  } else {
    dim3 grid((a.HW + 256 * PX - 1) / (256 * PX), a.B), block(256);
    hipLaunchKernelGGL((track_filter_kernel<PX, PLANAR, false>), grid, block, 0, s, a);
  }
}

}  // namespace dvd

extern "C" {

int dvd_track_filter(const float* points, int points_planar, const int* start, const float* R, const float* t,
                     const float* K_T, const float* depth_all, int N, const float* weights, int mode, float tol, float z_near,
                     float* depth_out, float* ratio, unsigned char* count, float* spread, int T1, int B, int H, int W, int k0,
                     dvd_stream_t stream) {
  using namespace dvd;
  DVD_REQUIRE(points && start && R && t && K_T && depth_all && weights && depth_out, "track_filter: null pointer");
  DVD_REQUIRE(T1 >= 1 && T1 <= kFilterMaxRows, "track_filter: T1=%d outside 1 .. %d rows", T1, kFilterMaxRows);
  DVD_REQUIRE(k0 <= 0 && k0 > -T1, "track_filter: the start frame's row %d is outside the %d rows of the slab", -k0, T1);
  DVD_REQUIRE(mode == 0 || mode == 1, "track_filter: mode=%d is neither 0 (mean) nor 1 (median)", mode);
  DVD_REQUIRE(tol >= 0.0f && tol <= FLT_MAX, "track_filter: tol=%g must be finite and >= 0", (double)tol);
  DVD_REQUIRE(z_near >= 0.0f && z_near <= FLT_MAX, "track_filter: z_near=%g must be finite and >= 0", (double)z_near);
  if (int st = track_shape_ok("track_filter", T1, B, N, H, W)) return st;
  FilterArgs a = {};
  a.points = points, a.start = start, a.R = R, a.t = t, a.K = K_T, a.depth_all = depth_all, a.weights = weights;
  a.depth_out = depth_out, a.ratio = ratio, a.spread = spread, a.count = count;
  a.T1 = T1, a.B = B, a.N = N, a.HW = H * W, a.k0 = k0;
  a.tl = 1.0f + tol, a.z_near = z_near;
  a.view = track_view(H, W);
  // the other rows' points and the frames they sample, the start frames' own depth, the outputs
  const double px = (double)B * a.HW;
  bytes_add(DVD_BYTES_GEOMETRY, px * (12.0 * (T1 - 1) + 4.0 + 4.0 + (ratio ? 4.0 : 0.0) + (count ? 1.0 : 0.0) + (spread ? 4.0 : 0.0)) +
                                    4.0 * (double)(N < T1 + B ? N : T1 + B) * a.HW);
  const bool v4 = (W % 4 == 0) && aligned_to(points, 16) && aligned_to(depth_all, 16) && aligned_to(depth_out, 16) &&
                  aligned_to(ratio, 16) && aligned_to(count, 16) && aligned_to(spread, 16);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (v4 && points_planar)
    track_filter_launch<4, true>(a, mode, s);
  else if (v4)
    track_filter_launch<4, false>(a, mode, s);
  else if (points_planar)
    track_filter_launch<1, true>(a, mode, s);
  else
    track_filter_launch<1, false>(a, mode, s);
  DVD_LAUNCH_OK();
  return DVD_OK;
}

}  // extern "C"
