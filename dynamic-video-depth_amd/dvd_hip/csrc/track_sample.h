// One world point into one camera of the per-frame tables, and what the target frame holds where it lands: the only place that
// decides `inside` for a track point and builds its bilinear taps.  csrc/track.hip writes every row out, csrc/track_filter.hip
// gates and fuses the rows in registers (both through project_sample) and csrc/eval.hip scores them (the same three parts, the
// taps shared by the depth and the colour planes).  The projection and its perspective divide are project_uvz of track_cam.h,
// which csrc/splat.hip and dvd_project_bwd call directly; the coordinate chain (sample_coord) and the tap arithmetic (bilinear)
// are those of the fused warp+loss kernel (warp_pixel.h).  All these units are built with -ffp-contract=off and call THESE functions, so the same point, table row and
// plane give the same bits in any of them.
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

// what every launch over a slab of track rows checks
inline int track_shape_ok(const char* who, int T1, int B, int N, int H, int W) {
  DVD_REQUIRE(T1 > 0 && T1 <= 65535 && B > 0 && B <= 65535 && N > 0, "%s: bad sizes T1=%d B=%d N=%d", who, T1, B, N);
  DVD_REQUIRE(H >= 2 && W >= 2 && (long long)H * W < (1LL << 30), "%s: bad image size H=%d W=%d", who, H, W);
  return DVD_OK;
}

struct TrackProj {
  float u, v;        // pixel position in the target camera
  float dx, dy;      // the module's displacement field: (u, v) minus the pixel's own (x, y)
  float z;           // third component of the projection
  bool front;        // z > 0
  unsigned int in;   // 1 where the point is in front of the camera and lands inside the image
};

// the point P of source pixel (xf, yf) into camera c
__device__ __forceinline__ TrackProj track_project(const TrackCam& c, const TrackView& w, float P0, float P1, float P2, float xf,
                                                   float yf) {
  TrackProj h;
  project_uvz(c, P0, P1, P2, h.u, h.v, h.z);
  h.dx = h.u - xf, h.dy = h.v - yf;
  h.front = h.z > 0.0f;
  h.in = (h.front && h.u >= 0.0f && h.u <= w.wmax && h.v >= 0.0f && h.v <= w.hmax) ? 1u : 0u;
  return h;
}

struct TrackTaps {
  int o, W;                          // offset of the NW tap in a plane [H,W]; NE, SW, SE are o + 1, o + W, o + W + 1
  bool in_e, in_s;                   // a tap past the east / south edge is not read: its value is 0
  float w_nw, w_ne, w_sw, w_se;
};

// the four taps around (x, y) + (dx, dy): always inside [0, W-1] x [0, H-1], because sample_coord clamps and its fmaxf / fminf
// turn a NaN into 0
__device__ __forceinline__ TrackTaps track_taps(const TrackView& w, float xf, float yf, float dx, float dy) {
  TrackTaps t;
  const float ix = sample_coord(xf, dx, w.half_w, w.wmax);
  const float iy = sample_coord(yf, dy, w.half_h, w.hmax);
  const float x0f = floorf(ix), y0f = floorf(iy);
  const float ww = ix - x0f, we = 1.0f - ww, wn = iy - y0f, ws = 1.0f - wn;
  const int x0 = (int)x0f, y0 = (int)y0f;
  t.in_e = (x0 + 1) < w.W, t.in_s = (y0 + 1) < w.H;
  t.o = y0 * w.W + x0, t.W = w.W;
  t.w_nw = ws * we, t.w_ne = ws * ww, t.w_sw = wn * we, t.w_se = wn * ww;
  return t;
}

// bilinear border-clamped sample of one plane [H,W] through a tap set
__device__ __forceinline__ float tap_sample(const float* __restrict__ plane, const TrackTaps& t) {
  return bilinear(plane[t.o], t.in_e ? plane[t.o + 1] : 0.0f, t.in_s ? plane[t.o + t.W] : 0.0f,
                  (t.in_e && t.in_s) ? plane[t.o + t.W + 1] : 0.0f, t.w_nw, t.w_ne, t.w_sw, t.w_se);
}

struct TrackHit : TrackProj {
  float d;           // bilinear border-clamped sample of dg at (u, v); 0 behind the camera or without a depth map
};

// ... and the target frame's depth there; dg: that frame's depth [H,W] or null
__device__ __forceinline__ TrackHit project_sample(const TrackCam& c, const float* __restrict__ dg, const TrackView& w,
                                                   float P0, float P1, float P2, float xf, float yf) {
  TrackHit h;
  static_cast<TrackProj&>(h) = track_project(c, w, P0, P1, P2, xf, yf);
  h.d = (dg && h.front) ? tap_sample(dg, track_taps(w, xf, yf, h.dx, h.dy)) : 0.0f;
  return h;
}

}  // namespace dvd
