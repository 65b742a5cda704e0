// Query-point tracks: a list of chosen, sub-pixel points of any frames instead of every pixel of whole frames (gfx950).
//
// csrc/track.hip, csrc/eval.hip and csrc/track_filter.hip tie the point slab [T1,B,3,H,W] to the image grid: the camera row is
// uniform per block, the source pixel is the thread's own (x, y), and H, W are both the slab shape and the image size.  Here a
// slab row is [3,Q] (what dvd_sf_mlp_fwd takes as n_pix = Q points with a time stamp each), query q lives in frame frame[q]
// at the position xy[q] of that frame, and every thread loads its own camera row (the tables are N x 84 B and stay in cache).
//
//   dvd_point_seed     depth_all[frame] at xy by DIRECT bilinear taps (clamp, floor, weights from x - floor(x); none of
//                      sample_coord's normalise / de-normalise roundings: at an integer position the weights are exactly
//                      (1, 0, 0, 0)), combined by bilinear() of warp_pixel.h, then unproject_point (unproject_point.h) -- the
//                      body of unproject_fwd_kernel, so an integer query has the bits dvd_unproject_fwd gives that pixel
//   dvd_point_project  row j of query q into the camera of frame g = frame[q] + j + k0 through project_sample of
//                      track_sample.h with the query's own position as the source pixel, so an integer query has the bits
//                      dvd_track_project_from gives that pixel; plus eval.hip's occlusion rule and the target frame
//   dvd_point_score    the TAP-Vid counts of predicted tracks against annotated ones: 19 exact 64-bit integers per slab row
//
// One point per thread, 256-thread blocks, plain stores, one writer per output element; the score's only atomics are the
// integer adds of block_add_i64 (dvd_post.h), so every result is bitwise reproducible and independent of the grid.  Built with
// -ffp-contract=off like every geometry unit.  Per point: seed 12 B read + 17 or 21 B written + 4 taps; project 12 B read +
// 22 B written + 4 taps + the query's 13 B; score 13 B read + 9 B of ground truth gathered with stride N.

#include <float.h>

#include "track_sample.h"
#include "unproject_point.h"

namespace dvd {

constexpr float kPointCap = 1024.0f;      // the error of word 18 is capped here (2^10)
constexpr int kPointCapLog2 = 10;
constexpr int kPointSums = 19;
constexpr int kPointThr = 5;

// the four taps around (x, y) itself: clamped to the image, a NaN becomes 0 (fmaxf drops it), weights from x - floor(x)
__device__ __forceinline__ TrackTaps direct_taps(const TrackView& w, float x, float y) {
  TrackTaps t;
  const float ix = fminf(w.wmax, fmaxf(x, 0.0f));
  const float iy = fminf(w.hmax, fmaxf(y, 0.0f));
  const float x0f = floorf(ix), y0f = floorf(iy);
  const float ww = ix - x0f, we = 1.0f - ww, wn = iy - y0f, ws = 1.0f - wn;
  const int x0 = (int)x0f, y0 = (int)y0f;
  t.in_e = (x0 + 1) < w.W, t.in_s = (y0 + 1) < w.H;
  t.o = y0 * w.W + x0, t.W = w.W;
  t.w_nw = ws * we, t.w_ne = ws * ww, t.w_sw = wn * we, t.w_se = wn * ww;
  return t;
}

struct SeedArgs {
  const int* frame;               // [Q]
  const float* xy;                // [Q,2]
  const float* depth_all;         // [N,1,H,W]
  const float *R_T, *t, *Ki;      // [N,3,3] camera->world, [N,3], [N,3,3] (K^-1)^T
  const float* ts;                // [N] or null
  float* points;                  // [3,Q]
  float* t_out;                   // [Q] or null
  unsigned char* ok;              // [Q]
  int Q, N, HW;
  TrackView view;
};

__global__ __launch_bounds__(256) void point_seed_kernel(const SeedArgs a) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= a.Q) return;
  const int f = a.frame[q];
  const float x = a.xy[2 * (size_t)q], y = a.xy[2 * (size_t)q + 1];
  float P0 = 0.0f, P1 = 0.0f, P2 = 0.0f, ts = 0.0f;
  unsigned char ok = 0;
  if (f >= 0 && f < a.N) {
    if (a.ts) ts = a.ts[f];
    const float d = tap_sample(a.depth_all + (size_t)f * a.HW, direct_taps(a.view, x, y));
    const bool in_img = x >= 0.0f && x <= a.view.wmax && y >= 0.0f && y <= a.view.hmax;      // (a NaN fails)
    if (in_img && d > 0.0f && d <= FLT_MAX) {
      float Ki[9], R[9], t[3];
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        Ki[i] = a.Ki[(size_t)f * 9 + i];
        R[i] = a.R_T[(size_t)f * 9 + i];
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) t[i] = a.t[(size_t)f * 3 + i];
      unproject_point(x, y, d, Ki, R, t, P0, P1, P2);
      ok = 1;
    }
  }
  a.points[q] = P0;
  a.points[(size_t)a.Q + q] = P1;
  a.points[2 * (size_t)a.Q + q] = P2;
  if (a.t_out) a.t_out[q] = ts;
  a.ok[q] = ok;
}

struct PointProjArgs {
  const float* points;            // [T1,3,Q]
  const int* frame;               // [Q]
  const float* xy;                // [Q,2]
  const unsigned char* ok;        // [Q] or null (every query counts)
  const float *R, *t, *K;         // [N,3,3] world->camera, [N,3], [N,3,3]
  const float* depth_all;         // [N,1,H,W]
  float *uv, *z, *depth_at;       // [T1,Q,2], [T1,Q], [T1,Q]
  unsigned char *inside, *visible;
  int* target;                    // [T1,Q]
  int Q, N, HW, k0;
  float tol;                      // 1 + z_tol
  TrackView view;
};

__global__ __launch_bounds__(256) void point_project_kernel(const PointProjArgs a) {
  const int q = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
  if (q >= a.Q) return;
  const size_t idx = (size_t)j * a.Q + q;
  const int f = a.frame[q];
  const long long gl = (long long)f + j + a.k0;
  const bool live = f >= 0 && f < a.N && gl >= 0 && gl < (long long)a.N && (!a.ok || a.ok[q] != 0);
  float u = 0.0f, v = 0.0f, z = 0.0f, d = 0.0f;
  unsigned int in = 0u, vis = 0u;
  int g = -1;
  if (live) {
    g = (int)gl;
    TrackCam c;
    load_track_cam(a.R, a.t, a.K, g, c);
    const float* p = a.points + (size_t)j * 3 * a.Q + q;
    const float P0 = p[0], P1 = p[a.Q], P2 = p[2 * (size_t)a.Q];
    const TrackHit h = project_sample(c, a.depth_all + (size_t)g * a.HW, a.view, P0, P1, P2, a.xy[2 * (size_t)q],
                                      a.xy[2 * (size_t)q + 1]);
    u = h.u, v = h.v, z = h.z, d = h.d, in = h.in;
    vis = (h.in && !(h.z > h.d * a.tol)) ? 1u : 0u;
  }
  a.uv[2 * idx] = u;
  a.uv[2 * idx + 1] = v;
  a.z[idx] = z;
  a.depth_at[idx] = d;
  a.inside[idx] = (unsigned char)in;
  a.visible[idx] = (unsigned char)vis;
  a.target[idx] = g;
}

struct PointScoreArgs {
  const float* uv;                // [T1,Q,2]
  const unsigned char* visible;   // [T1,Q]
  const int* target;              // [T1,Q]
  const float* gt_uv;             // [Q,N,2]
  const unsigned char* gt_state;  // [Q,N]
  unsigned long long* sums;       // [T1,19]
  int Q, N, origin;
  float sx, sy;
  float thr2[kPointThr];
  double scale;                   // 2^shift
};

__global__ __launch_bounds__(256) void point_score_kernel(const PointScoreArgs a) {
  const int q = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;      // the row is uniform over the block
  long long acc[kPointSums];
#pragma unroll
  for (int k = 0; k < kPointSums; ++k) acc[k] = 0;
  if (q < a.Q && j != a.origin) {
    const size_t idx = (size_t)j * a.Q + q;
    const int g = a.target[idx];
    if (g >= 0 && g < a.N) {                       // (a target outside the annotation's frames reads nothing)
      const size_t at = (size_t)q * a.N + g;
      const unsigned int st = a.gt_state[at];
      if (st < 2u) {
        const bool vis_gt = st == 0u, vis = a.visible[idx] != 0;
        const float du = (a.uv[2 * idx] - a.gt_uv[2 * at]) * a.sx;
        const float dv = (a.uv[2 * idx + 1] - a.gt_uv[2 * at + 1]) * a.sy;
        const float e2 = du * du + dv * dv;
        acc[0] += 1;
        acc[1] += vis_gt ? 1 : 0;
        acc[2] += (vis == vis_gt) ? 1 : 0;
#pragma unroll
        for (int i = 0; i < kPointThr; ++i) {
          const bool within = e2 < a.thr2[i];      // strict; a NaN is never within
          acc[3 + i] += (vis_gt && within) ? 1 : 0;
          acc[8 + i] += (vis_gt && within && vis) ? 1 : 0;
          acc[13 + i] += (vis && (!vis_gt || !within)) ? 1 : 0;
        }
        // sqrtf is the compiler's correctly rounded IEEE square root (what numpy's float32 sqrt gives); this toolchain's
        // __fsqrt_rn is the 1-ulp native one unless OCML_BASIC_ROUNDED_OPERATIONS is defined.  fminf takes a NaN as the cap.
        if (vis_gt) acc[18] += fixed_q(fminf(sqrtf(e2), kPointCap), a.scale);
      }
    }
  }
  block_add_i64<kPointSums>(acc, a.sums + (size_t)j * kPointSums);
}

// what the three entries check of the list and the tables
static int point_shape_ok(const char* who, int T1, int Q, int N) {
  DVD_REQUIRE(T1 > 0 && T1 <= 65535 && Q > 0 && Q < (1 << 30) && N > 0, "%s: bad sizes T1=%d Q=%d N=%d", who, T1, Q, N);
  return DVD_OK;
}

static int point_image_ok(const char* who, int H, int W) {
  DVD_REQUIRE(H >= 2 && W >= 2 && (long long)H * W < (1LL << 30), "%s: bad image size H=%d W=%d", who, H, W);
  return DVD_OK;
}

}  // namespace dvd

extern "C" {

int dvd_point_seed(const int* frame, const float* xy, const float* depth_all, const float* R_T, const float* t,
                   const float* K_inv_T, const float* ts_vali, int N, float* points, float* t_out, unsigned char* ok, int Q,
                   int H, int W, dvd_stream_t stream) {
  using namespace dvd;
  DVD_REQUIRE(frame && xy && depth_all && R_T && t && K_inv_T && points && ok, "point_seed: null pointer");
  DVD_REQUIRE((ts_vali != nullptr) == (t_out != nullptr), "point_seed: ts_vali and t go together (both or none)");
  if (int st = point_shape_ok("point_seed", 1, Q, N)) return st;
  if (int st = point_image_ok("point_seed", H, W)) return st;
  SeedArgs a = {};
  a.frame = frame, a.xy = xy, a.depth_all = depth_all, a.R_T = R_T, a.t = t, a.Ki = K_inv_T, a.ts = ts_vali;
  a.points = points, a.t_out = t_out, a.ok = ok;
  a.Q = Q, a.N = N, a.HW = H * W;
  a.view = track_view(H, W);
  bytes_add(DVD_BYTES_GEOMETRY, (double)Q * (12.0 + 16.0 + 13.0 + (t_out ? 8.0 : 0.0)));
  hipLaunchKernelGGL(point_seed_kernel, dim3((Q + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  DVD_LAUNCH_OK();
  return DVD_OK;
}

int dvd_point_project(const float* points, const int* frame, const float* xy, const unsigned char* ok, int k0, const float* R,
                      const float* t, const float* K_T, const float* depth_all, int N, float z_tol, float* uv, float* z,
                      float* depth_at, unsigned char* inside, unsigned char* visible, int* target, int T1, int Q, int H, int W,
                      dvd_stream_t stream) {
  using namespace dvd;
  DVD_REQUIRE(points && frame && xy && R && t && K_T && depth_all && uv && z && depth_at && inside && visible && target,
              "point_project: null pointer");
  if (int st = point_shape_ok("point_project", T1, Q, N)) return st;
  if (int st = point_image_ok("point_project", H, W)) return st;
  DVD_REQUIRE(k0 > -(1 << 30) && k0 < (1 << 30), "point_project: bad row offset k0=%d", k0);
  DVD_REQUIRE(z_tol >= 0.0f && z_tol <= FLT_MAX, "point_project: z_tol=%g must be finite and >= 0", (double)z_tol);
  PointProjArgs a = {};
  a.points = points, a.frame = frame, a.xy = xy, a.ok = ok, a.R = R, a.t = t, a.K = K_T, a.depth_all = depth_all;
  a.uv = uv, a.z = z, a.depth_at = depth_at, a.inside = inside, a.visible = visible, a.target = target;
  a.Q = Q, a.N = N, a.HW = H * W, a.k0 = k0;
  a.tol = 1.0f + z_tol;
  a.view = track_view(H, W);
  bytes_add(DVD_BYTES_GEOMETRY, (double)T1 * Q * (12.0 + 13.0 + 16.0 + 22.0));
  hipLaunchKernelGGL(point_project_kernel, dim3((Q + 255) / 256, T1), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  DVD_LAUNCH_OK();
  return DVD_OK;
}

int dvd_point_score(const float* uv, const unsigned char* visible, const int* target, int origin, const float* gt_uv,
                    const unsigned char* gt_state, int N, float sx, float sy, const float* thr2, int shift, long long* sums,
                    int T1, int Q, dvd_stream_t stream) {
  using namespace dvd;
  DVD_REQUIRE(uv && visible && target && gt_uv && gt_state && thr2 && sums, "point_score: null pointer");
  if (int st = point_shape_ok("point_score", T1, Q, N)) return st;
  DVD_REQUIRE(origin >= -1 && origin < T1, "point_score: origin row %d outside -1 .. %d", origin, T1 - 1);
  DVD_REQUIRE(sx > 0.0f && sx <= FLT_MAX && sy > 0.0f && sy <= FLT_MAX, "point_score: sx=%g, sy=%g must be finite and > 0",
              (double)sx, (double)sy);
  for (int i = 0; i < kPointThr; ++i)
    DVD_REQUIRE(thr2[i] > (i ? thr2[i - 1] : 0.0f) && thr2[i] <= FLT_MAX,
                "point_score: the squared thresholds must be finite, positive and ascending (entry %d is %g)", i, (double)thr2[i]);
  // a row sums Q terms of at most 2^10 * 2^shift each: they must stay below 2^62
  DVD_REQUIRE(shift >= 1 && shift <= 32 && shift + kPointCapLog2 + ceil_log2(Q) <= 62,
              "point_score: shift=%d outside 1 .. min(32, 62 - 10 - ceil_log2(Q)) for Q=%d", shift, Q);
  PointScoreArgs a = {};
  a.uv = uv, a.visible = visible, a.target = target, a.gt_uv = gt_uv, a.gt_state = gt_state;
  a.sums = reinterpret_cast<unsigned long long*>(sums);
  a.Q = Q, a.N = N, a.origin = origin, a.sx = sx, a.sy = sy;
  for (int i = 0; i < kPointThr; ++i) a.thr2[i] = thr2[i];
  a.scale = (double)(1ULL << shift);
  bytes_add(DVD_BYTES_GEOMETRY, (double)T1 * Q * (13.0 + 9.0));
  hipLaunchKernelGGL(point_score_kernel, dim3((Q + 255) / 256, T1), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  DVD_LAUNCH_OK();
  return DVD_OK;
}

}  // extern "C"
