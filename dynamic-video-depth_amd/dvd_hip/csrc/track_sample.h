// One world point into one camera of the per-frame tables, with the target frame's depth sampled where it lands: the per-row
// arithmetic shared by csrc/track.hip (which writes every row out) and csrc/track_filter.hip (which gates and fuses the rows
// in registers).  Projection as in track_cam.h; the coordinate chain (sample_coord) and the tap arithmetic (bilinear) are
// those of the fused warp+loss kernel (warp_pixel.h).  Both units are built with -ffp-contract=off and call THIS function,
// so the same point, table row and depth map give the same bits in either of them.
#pragma once

#include "track_cam.h"
#include "warp_pixel.h"

namespace dvd {

struct TrackView {
  int H, W;
  float half_w, half_h, wmax, hmax;
};

inline TrackView track_view(int H, int W) {
  TrackView v;
  v.H = H, v.W = W;
  v.half_w = (float)((W - 1) / 2.0), v.half_h = (float)((H - 1) / 2.0), v.wmax = (float)(W - 1), v.hmax = (float)(H - 1);
  return v;
}

// what every launch over a slab of track rows checks and how it picks its 16-byte path
inline bool track_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline int track_shape_ok(const char* who, int T1, int B, int N, int H, int W) {
  DVD_REQUIRE(T1 > 0 && T1 <= 65535 && B > 0 && B <= 65535 && N > 0, "%s: bad sizes T1=%d B=%d N=%d", who, T1, B, N);
  DVD_REQUIRE(H >= 2 && W >= 2 && (long long)H * W < (1LL << 30), "%s: bad image size H=%d W=%d", who, H, W);
  return DVD_OK;
}

struct TrackHit {
  float u, v;        // pixel position in the target camera
  float dx, dy;      // the module's displacement field: (u, v) minus the pixel's own (x, y)
  float z;           // third component of the projection
  float d;           // bilinear border-clamped sample of dg at (u, v); 0 behind the camera or without a depth map
  unsigned int in;   // 1 where the point is in front of the camera and lands inside the image
};

// the point P of source pixel (xf, yf) into camera c; dg: the target frame's depth [H,W] or null
__device__ __forceinline__ TrackHit project_sample(const TrackCam& c, const float* __restrict__ dg, const TrackView& w,
                                                   float P0, float P1, float P2, float xf, float yf) {
  TrackHit h;
  float I0, I1, I2;
  project_point(c, P0, P1, P2, I0, I1, I2);
  const float den = I2 + 1e-8f;
  const float ui = I0 / den, vi = I1 / den;
  const float dx = ui - xf, dy = vi - yf;
  const bool front = I2 > 0.0f;
  h.in = (front && ui >= 0.0f && ui <= w.wmax && vi >= 0.0f && vi <= w.hmax) ? 1u : 0u;
  h.d = 0.0f;
  if (dg && front) {
    // always inside [0, W-1] x [0, H-1]: sample_coord clamps, and its fmaxf / fminf turn a NaN into 0
    const float ix = sample_coord(xf, dx, w.half_w, w.wmax);
    const float iy = sample_coord(yf, dy, w.half_h, w.hmax);
    const float x0f = floorf(ix), y0f = floorf(iy);
    const float ww = ix - x0f, we = 1.0f - ww, wn = iy - y0f, ws = 1.0f - wn;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const bool in_e = (x0 + 1) < w.W, in_s = (y0 + 1) < w.H;
    const int o = y0 * w.W + x0;
    const float dnw = dg[o], dne = in_e ? dg[o + 1] : 0.0f, dsw = in_s ? dg[o + w.W] : 0.0f,
                dse = (in_e && in_s) ? dg[o + w.W + 1] : 0.0f;
    h.d = bilinear(dnw, dne, dsw, dse, ws * we, ws * ww, wn * we, wn * ww);
  }
  h.u = ui, h.v = vi, h.dx = dx, h.dy = dy, h.z = I2;
  return h;
}

}  // namespace dvd
