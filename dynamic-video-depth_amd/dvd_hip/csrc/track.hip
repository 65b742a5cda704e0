// World points -> pixel positions in a sequence of target cameras, with the target frame's depth sampled there (gfx950).
//
// Replaces project_ptcld.forward (/root/reference/losses/scene_flow_projection.py:27-44)
//     Q = (P - t) @ R_T ;  I = Q @ K ;  (u, v) = I.xy / (I.z + 1e-8)
// and, for the depth sample, BackwardWarp (:289-297) fed with that module's displacement field (u - x, v - y):
// F.grid_sample(depth, (x, y) + displacement, bilinear, padding 'border', align_corners=True) -- the coordinate chain
// (sample_coord) and the tap arithmetic (bilinear) are those of the fused warp+loss kernel (warp_pixel.h), as in
// dvd_flow_warp_fwd; one point into one camera is project_sample (track_sample.h), shared with csrc/track_filter.hip.  The cameras are rows of per-frame tables: image b of step k looks up frame start[b] + k, so ONE launch
// projects every step of an integrated trajectory (models/tracks.py); a frame past the end of the tables writes zeros and
// reads nothing.  dvd_track_project_from adds a row offset k0 (frame start[b] + k + k0; negative for a slab that also holds
// the rows BEFORE the start frame, csrc/invert.hip) and gives zeros on either side of the video.  dvd_project_bwd is the 2x3
// Jacobian of (u, v) w.r.t. P, transposed, per point.
//
// A pure map plus one 4-tap gather: 12 B read and 17 B written per point, plus the taps; no atomics, every output element
// is written by exactly one thread with plain vector stores, so results are bitwise reproducible.  One thread per 4
// horizontally adjacent pixels where the width is a multiple of 4 (16-byte accesses, the four `inside` bytes as one dword),
// one pixel per thread otherwise.  Same fp32 operation order as torch's CPU matmul (dvd_common.h), built with
// -ffp-contract=off; the division is the compiler's IEEE division (z is not bounded away from 0 here).

#include "track_sample.h"

namespace dvd {

struct TrackArgs {
  const float* points;        // [T1,B,3,H,W] (planar) or [T1,B,H,W,3]
  const int* start;           // [B]
  const float *R, *t, *K;     // [N,3,3], [N,3], [N,3,3]
  const float* depth_all;     // [N,1,H,W] or null
  float *uv, *z, *depth_at;   // [T1,B,H,W,2], [T1,B,H,W], [T1,B,H,W]   (z, depth_at may be null)
  unsigned char* inside;      // [T1,B,H,W] or null
  const float* g_uv;          // backward: [T1,B,H,W,2]
  float* g_points;            // backward: the layout of points
  int B, N, HW, displacement, accumulate;
  int k0;                     // row k looks up frame start[b] + k + k0 (0 for every entry but dvd_track_project_from)
  TrackView view;             // the image size and the constants of the sampling chain (track_sample.h)
};

// the table row of image b at step k, or -1 where the video has ended or not begun (or the start is not a frame at all)
__device__ __forceinline__ int target_frame(const TrackArgs& a, int b, int k) {
  const int s = a.start[b];
  const long long g = (long long)s + k + a.k0;
  return (s >= 0 && g >= 0 && g < (long long)a.N) ? (int)g : -1;
}

template <int PX, bool PLANAR>
__global__ __launch_bounds__(256) void track_project_kernel(const TrackArgs a) {
  const int b = blockIdx.y, k = blockIdx.z;
  const int p0 = (blockIdx.x * 256 + threadIdx.x) * PX;
  if (p0 >= a.HW) return;
  const size_t img = (size_t)k * a.B + b;
  const size_t pix = img * a.HW + p0;
  const int g = target_frame(a, b, k);      // uniform over the block
  float u[PX], v[PX], zz[PX], d[PX];
  unsigned int in[PX];
#pragma unroll
  for (int i = 0; i < PX; ++i) {
    u[i] = v[i] = zz[i] = d[i] = 0.0f;
    in[i] = 0u;
  }
  if (g >= 0) {
    TrackCam c;
    load_track_cam(a.R, a.t, a.K, g, c);
    float P[3][PX];
    load_points<PX, PLANAR>(a.points, img, p0, a.HW, P);
    const int y = p0 / a.view.W, x = p0 - y * a.view.W;
    const float yf = (float)y;
    const float* dg = a.depth_all ? a.depth_all + (size_t)g * a.HW : nullptr;
#pragma unroll
    for (int i = 0; i < PX; ++i) {
      const TrackHit h = project_sample(c, dg, a.view, P[0][i], P[1][i], P[2][i], (float)(x + i), yf);
      in[i] = h.in;
      d[i] = h.d;
      u[i] = a.displacement ? h.dx : h.u;
      v[i] = a.displacement ? h.dy : h.v;
      zz[i] = h.z;
    }
  }
  if (PX == 4) {
    st4(a.uv + pix * 2, make_float4(u[0], v[0], u[1], v[1]));
    st4(a.uv + pix * 2 + 4, make_float4(u[2], v[2], u[3], v[3]));
  } else {
    a.uv[pix * 2] = u[0];
    a.uv[pix * 2 + 1] = v[0];
  }
  if (a.z) stpx<PX>(a.z + pix, zz);
  if (a.depth_all) stpx<PX>(a.depth_at + pix, d);
  if (a.inside) stpx_bytes<PX>(a.inside + pix, in);
}

// g_P (+)= J^T g_uv with u = I0 / den, v = I1 / den, den = I2 + 1e-8:
//   g_I = (g_u / den, g_v / den, -(g_u u + g_v v) / den) ;  g_P = (g_I @ K^T) @ R_T^T
template <int PX, bool PLANAR>
__global__ __launch_bounds__(256) void project_bwd_kernel(const TrackArgs a) {
  const int b = blockIdx.y, k = blockIdx.z;
  const int p0 = (blockIdx.x * 256 + threadIdx.x) * PX;
  if (p0 >= a.HW) return;
  const size_t img = (size_t)k * a.B + b;
  const size_t pix = img * a.HW + p0;
  const int g = target_frame(a, b, k);
  float G[3][PX];
#pragma unroll
  for (int i = 0; i < PX; ++i) G[0][i] = G[1][i] = G[2][i] = 0.0f;
  if (g >= 0) {
    TrackCam c;
    load_track_cam(a.R, a.t, a.K, g, c);
    float P[3][PX], gu[PX], gv[PX];
    load_points<PX, PLANAR>(a.points, img, p0, a.HW, P);
    if (PX == 4) {
      const float4 lo = ld4(a.g_uv + pix * 2), hi = ld4(a.g_uv + pix * 2 + 4);
      gu[0] = lo.x, gv[0] = lo.y, gu[1] = lo.z, gv[1] = lo.w;
      gu[2] = hi.x, gv[2] = hi.y, gu[3] = hi.z, gv[3] = hi.w;
    } else {
      gu[0] = a.g_uv[pix * 2];
      gv[0] = a.g_uv[pix * 2 + 1];
    }
#pragma unroll
    for (int i = 0; i < PX; ++i) {
      float ui, vi, I2;
      project_uvz(c, P[0][i], P[1][i], P[2][i], ui, vi, I2);
      const float den = I2 + 1e-8f;
      const float gI0 = gu[i] / den, gI1 = gv[i] / den;
      const float gI2 = -(gu[i] * ui + gv[i] * vi) / den;
      float q0, q1, q2;
      rowvec_mat3_T(gI0, gI1, gI2, c.K, q0, q1, q2);
      rowvec_mat3_T(q0, q1, q2, c.R, G[0][i], G[1][i], G[2][i]);
    }
  }
  if (PLANAR) {
    float* o = a.g_points + img * 3 * a.HW + p0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float* dst = o + (size_t)ch * a.HW;
      float old[PX];
      if (a.accumulate) {
        ldpx<PX>(dst, old);
#pragma unroll
        for (int i = 0; i < PX; ++i) G[ch][i] += old[i];
      }
      stpx<PX>(dst, G[ch]);
    }
  } else {
    float* o = a.g_points + pix * 3;
    float w[3 * PX];
#pragma unroll
    for (int i = 0; i < PX; ++i) {
      w[3 * i] = G[0][i];
      w[3 * i + 1] = G[1][i];
      w[3 * i + 2] = G[2][i];
    }
    // (3 * PX floats: three 16-byte accesses, or three scalars)
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      float old[PX];
      if (a.accumulate) {
        ldpx<PX>(o + PX * q, old);
#pragma unroll
        for (int i = 0; i < PX; ++i) w[PX * q + i] += old[i];
      }
      stpx<PX>(o + PX * q, w + PX * q);
    }
  }
}

static int track_project_launch(const float* points, int points_planar, const int* start, const float* R, const float* t,
                                const float* K_T, const float* depth_all, int N, float* uv, int displacement, float* z,
                                float* depth_at, unsigned char* inside, int T1, int B, int H, int W, int k0,
                                dvd_stream_t stream) {
  DVD_REQUIRE(points && start && R && t && K_T && uv, "track_project: null pointer");
  DVD_REQUIRE(!depth_all || depth_at, "track_project: depth_all without depth_at");
  if (int st = track_shape_ok("track_project", T1, B, N, H, W)) return st;
  TrackArgs a = {};
  a.points = points, a.start = start, a.R = R, a.t = t, a.K = K_T, a.depth_all = depth_all;
  a.uv = uv, a.z = z, a.depth_at = depth_all ? depth_at : nullptr, a.inside = inside;
  a.B = B, a.N = N, a.HW = H * W, a.displacement = displacement, a.k0 = k0;
  a.view = track_view(H, W);
  const double pts = (double)T1 * B * a.HW;
  bytes_add(DVD_BYTES_GEOMETRY, pts * (12.0 + 8.0 + (z ? 4.0 : 0.0) + (inside ? 1.0 : 0.0) + (depth_all ? 4.0 : 0.0)) +
                                    (depth_all ? 4.0 * (double)(N < T1 + B ? N : T1 + B) * a.HW : 0.0));
  const bool v4 = (W % 4 == 0) && aligned_to(points, 16) && aligned_to(uv, 16) && aligned_to(z, 16) &&
                  aligned_to(a.depth_at, 16) && aligned_to(inside, 16);
  const int px = v4 ? 4 : 1;
  dim3 grid((a.HW + 256 * px - 1) / (256 * px), B, T1), block(256);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (v4 && points_planar)
    hipLaunchKernelGGL((track_project_kernel<4, true>), grid, block, 0, s, a);
  else if (v4)
    hipLaunchKernelGGL((track_project_kernel<4, false>), grid, block, 0, s, a);
  else if (points_planar)
    hipLaunchKernelGGL((track_project_kernel<1, true>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((track_project_kernel<1, false>), grid, block, 0, s, a);
  DVD_LAUNCH_OK();
  return DVD_OK;
}

}  // namespace dvd

extern "C" {

int dvd_track_project(const float* points, int points_planar, const int* start, const float* R, const float* t,
                      const float* K_T, const float* depth_all, int N, float* uv, int displacement, float* z,
                      float* depth_at, unsigned char* inside, int T1, int B, int H, int W, dvd_stream_t stream) {
  return dvd::track_project_launch(points, points_planar, start, R, t, K_T, depth_all, N, uv, displacement, z, depth_at, inside,
                                   T1, B, H, W, 0, stream);
}

int dvd_track_project_from(const float* points, int points_planar, const int* start, const float* R, const float* t,
                           const float* K_T, const float* depth_all, int N, float* uv, int displacement, float* z,
                           float* depth_at, unsigned char* inside, int T1, int B, int H, int W, int k0, dvd_stream_t stream) {
  DVD_REQUIRE(k0 > -(1 << 30) && k0 < (1 << 30), "track_project_from: bad row offset k0=%d", k0);
  return dvd::track_project_launch(points, points_planar, start, R, t, K_T, depth_all, N, uv, displacement, z, depth_at, inside,
                                   T1, B, H, W, k0, stream);
}

int dvd_project_bwd(const float* g_uv, const float* points, int points_planar, const int* start, const float* R,
                    const float* t, const float* K_T, int N, float* g_points, int accumulate, int T1, int B, int H, int W,
                    dvd_stream_t stream) {
  using namespace dvd;
  DVD_REQUIRE(g_uv && points && start && R && t && K_T && g_points, "project_bwd: null pointer");
  if (int st = track_shape_ok("project_bwd", T1, B, N, H, W)) return st;
  TrackArgs a = {};
  a.points = points, a.start = start, a.R = R, a.t = t, a.K = K_T, a.g_uv = g_uv, a.g_points = g_points;
  a.B = B, a.N = N, a.HW = H * W, a.accumulate = accumulate;
  bytes_add(DVD_BYTES_GEOMETRY, (double)T1 * B * a.HW * (accumulate ? 44.0 : 32.0));
  const bool v4 = (W % 4 == 0) && aligned_to(points, 16) && aligned_to(g_uv, 16) && aligned_to(g_points, 16);
  const int px = v4 ? 4 : 1;
  dim3 grid((a.HW + 256 * px - 1) / (256 * px), B, T1), block(256);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (v4 && points_planar)
    hipLaunchKernelGGL((project_bwd_kernel<4, true>), grid, block, 0, s, a);
  else if (v4)
    hipLaunchKernelGGL((project_bwd_kernel<4, false>), grid, block, 0, s, a);
  else if (points_planar)
    hipLaunchKernelGGL((project_bwd_kernel<1, true>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((project_bwd_kernel<1, false>), grid, block, 0, s, a);
  DVD_LAUNCH_OK();
  return DVD_OK;
}

}  // extern "C"
