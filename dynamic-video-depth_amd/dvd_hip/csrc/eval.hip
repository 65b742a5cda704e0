// A finished optimisation scored along its tracks: how well do depth, scene flow, cameras and optical flow agree? (gfx950)
//
// Row r of image b holds the world points of frame source[b]'s pixels, integrated along the scene-flow field to the time of
// frame g = source[b] + k_first + r (models/tracks.py).  Every point is projected into the camera of g by the functions
// dvd_track_project projects it with (track_project, track_taps, tap_sample of track_sample.h, -ffp-contract=off: the same
// point and table row give the same u, v, z and the same taps, bit for bit) and compared with what frame g holds there:
//     inside    z > 0 && 0 <= u <= W - 1 && 0 <= v <= H - 1
//     d         depth_all[g] at (u, v), bilinear, border                               (where inside)
//     occluded  z > d * (1 + z_tol)            seen = inside && !occluded
//     rel       min(|z - d| / max(d, d_min), 1)                                        (where seen)
//     photo     min((|c0 - o0| + |c1 - o1| + |c2 - o2|) / 3, 1024),  c = img_all[g] at (u, v) with the taps and weights of d,
//               o = the pixel's own colour in img_all[source[b]]                       (where seen)
//     epe       min(hypot((u - x) - flow.x, (v - y) - flow.y), 1024)  where the row has a flow pair, the pixel's mask byte is 0
//               and z > 0 -- whether inside or not, like the training's flow loss
// and the block reduces n_inside, n_occluded, sum q(rel), sum q(photo), n_flow, sum q(epe) with q(x) = llrint((double)x *
// 2^shift) to six 64-bit integers: per-thread registers, a shuffle tree over the 64 lanes, LDS across the four waves, then at
// most six integer atomicAdd per block (zeros are skipped).  Integer adds commute and are exact, so sums[T,B,6] is bitwise
// reproducible and independent of the grid; no float atomics, no ticket.  Every term is finite and <= 2^10 (fminf drops a
// NaN), so a row of H*W points stays below 2^(10 + shift + ceil_log2(H*W)) <= 2^62.
// Per point 12 B of points + 12 B own colour + 9 B flow and mask are streamed; the 16 taps come through the caches.  One thread
// per 4 horizontally adjacent pixels where W % 4 == 0 and the bases are 16-byte aligned, one pixel per thread otherwise.  A row
// whose frame g is past the end of the tables reads nothing and adds nothing (its maps are -1).

#include <float.h>

#include "track_sample.h"

namespace dvd {

constexpr float kEvalCap = 1024.0f;
constexpr int kEvalCapLog2 = 10;
constexpr int kEvalSums = 6;

struct EvalArgs {
  const float* points;          // [T,B,3,H,W]
  const int* source;            // [B]
  const float *R, *t, *K;       // [N,3,3], [N,3], [N,3,3]
  const float* depth_all;       // [N,1,H,W]
  const float* img_all;         // [N,3,H,W]
  const int* pair_row;          // [T,B] or null
  const float* flow;            // [P,H,W,2] or null
  const unsigned char* mask;    // [P,H,W] or null
  unsigned long long* sums;     // [T,B,6], step stride sums_stride
  float* maps;                  // [T,B,3,H,W], step stride maps_stride, or null
  long long sums_stride, maps_stride;
  int B, N, P, HW, k_first;
  float tol, d_min;
  TrackView view;               // the image size and the constants of the sampling chain (track_sample.h)
  double scale;                 // 2^shift
};

template <int PX, bool FLOW, bool MAPS>
__global__ __launch_bounds__(256) void eval_tracks_kernel(const EvalArgs a) {
  const int b = blockIdx.y, r = blockIdx.z;
  const int p0 = (blockIdx.x * 256 + threadIdx.x) * PX;
  const bool have = p0 < a.HW;
  // the frame this row looks into: uniform over the block
  const int s = a.source[b];
  const long long gl = (long long)s + a.k_first + r;
  const bool live = s >= 0 && gl < (long long)a.N;
  float rel[PX], photo[PX], epe[PX];
#pragma unroll
  for (int i = 0; i < PX; ++i) rel[i] = photo[i] = epe[i] = -1.0f;
  long long acc[kEvalSums] = {0, 0, 0, 0, 0, 0};
  if (live && have) {
    const int g = (int)gl;
    TrackCam c;
    load_track_cam(a.R, a.t, a.K, g, c);
    const size_t img = (size_t)r * a.B + b;
    float P[3][PX];
    load_points<PX, true>(a.points, img, p0, a.HW, P);
    const int y = p0 / a.view.W, x = p0 - y * a.view.W;
    const float yf = (float)y;
    const float* dg = a.depth_all + (size_t)g * a.HW;
    const float* cg = a.img_all + (size_t)g * 3 * a.HW;
    const float* own = a.img_all + (size_t)s * 3 * a.HW + p0;
    float o0[PX], o1[PX], o2[PX];
    ldpx<PX>(own, o0);
    ldpx<PX>(own + a.HW, o1);
    ldpx<PX>(own + 2 * (size_t)a.HW, o2);
    // the row of this (step, image) in the flow tensors, or -1; a row the tensors do not have counts as none
    int row = -1;
    if (FLOW) {
      row = a.pair_row[img];
      if (row >= a.P) row = -1;
    }
    float fl[2 * PX];
    unsigned int mk[PX];
#pragma unroll
    for (int i = 0; i < PX; ++i) fl[2 * i] = fl[2 * i + 1] = 0.0f, mk[i] = 1u;
    if (FLOW && row >= 0) {
      const size_t fp = (size_t)row * a.HW + p0;
      if (PX == 4) {
        ldpx<4>(a.flow + 2 * fp, fl);
        ldpx<4>(a.flow + 2 * fp + 4, fl + 4);
      } else {
        fl[0] = a.flow[2 * fp], fl[1] = a.flow[2 * fp + 1];
      }
      ldpx_bytes<PX>(a.mask + fp, mk);
    }
#pragma unroll
    for (int i = 0; i < PX; ++i) {
      const float xf = (float)(x + i);
      const TrackProj h = track_project(c, a.view, P[0][i], P[1][i], P[2][i], xf, yf);
      if (h.in) {
        const TrackTaps tp = track_taps(a.view, xf, yf, h.dx, h.dy);      // one tap set for the depth and the three colours
        const float d = tap_sample(dg, tp);
        const bool occluded = h.z > d * a.tol;
        acc[0] += 1;
        if (occluded) {
          acc[1] += 1;
        } else {
          rel[i] = fminf(fabsf(h.z - d) / fmaxf(d, a.d_min), 1.0f);
          float col[3];
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) col[ch] = tap_sample(cg + (size_t)ch * a.HW, tp);
          const float l1 = (fabsf(col[0] - o0[i]) + fabsf(col[1] - o1[i])) + fabsf(col[2] - o2[i]);
          photo[i] = fminf(l1 / 3.0f, kEvalCap);
          acc[2] += fixed_q(rel[i], a.scale);
          acc[3] += fixed_q(photo[i], a.scale);
        }
      }
      if (FLOW && row >= 0 && mk[i] == 0u && h.front) {
        epe[i] = fminf(hypotf(h.dx - fl[2 * i], h.dy - fl[2 * i + 1]), kEvalCap);
        acc[4] += 1;
        acc[5] += fixed_q(epe[i], a.scale);
      }
    }
  }
  if (MAPS && have) {
    float* m = a.maps + (size_t)r * a.maps_stride + (size_t)b * 3 * a.HW + p0;
    stpx<PX>(m, rel);
    stpx<PX>(m + a.HW, photo);
    stpx<PX>(m + 2 * (size_t)a.HW, epe);
  }
  if (!live) return;      // uniform over the block: nothing to add
  block_add_i64<kEvalSums>(acc, a.sums + (size_t)r * a.sums_stride + (size_t)b * kEvalSums);
}

template <int PX>
static void eval_launch(const EvalArgs& a, dim3 grid, hipStream_t s) {
  dim3 block(256);
  const bool flow = a.pair_row != nullptr, maps = a.maps != nullptr;
  if (flow && maps)
    hipLaunchKernelGGL((eval_tracks_kernel<PX, true, true>), grid, block, 0, s, a);
  else if (flow)
    hipLaunchKernelGGL((eval_tracks_kernel<PX, true, false>), grid, block, 0, s, a);
  else if (maps)
    hipLaunchKernelGGL((eval_tracks_kernel<PX, false, true>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((eval_tracks_kernel<PX, false, false>), grid, block, 0, s, a);
}

}  // namespace dvd

extern "C" {

int dvd_eval_tracks(const float* points, const int* source, int k_first, const float* R, const float* t, const float* K_T,
                    int N, const float* depth_all, const float* img_all, const int* pair_row, const float* flow_1_2,
                    const unsigned char* mask, int P, float z_tol, float d_min, int shift, long long* sums,
                    long long sums_step_stride, float* maps, long long maps_step_stride, int T, int B, int H, int W,
                    dvd_stream_t stream) {
  using namespace dvd;
  DVD_REQUIRE(points && source && R && t && K_T && depth_all && img_all && sums, "eval_tracks: null pointer");
  const int n_flow = (pair_row ? 1 : 0) + (flow_1_2 ? 1 : 0) + (mask ? 1 : 0);
  DVD_REQUIRE(n_flow == 0 || n_flow == 3, "eval_tracks: pair_row, flow_1_2 and mask go together (all three or none)");
  DVD_REQUIRE(n_flow == 0 || P > 0, "eval_tracks: bad number of flow pairs P=%d", P);
  DVD_REQUIRE(T > 0 && T <= 65535 && B > 0 && B <= 65535 && N > 0, "eval_tracks: bad sizes T=%d B=%d N=%d", T, B, N);
  DVD_REQUIRE(H >= 2 && W >= 2 && (long long)H * W < (1LL << 30), "eval_tracks: bad image size H=%d W=%d", H, W);
  DVD_REQUIRE(k_first == 0 || k_first == 1, "eval_tracks: k_first=%d must be 0 or 1", k_first);
  DVD_REQUIRE(z_tol >= 0.0f && z_tol <= FLT_MAX, "eval_tracks: z_tol=%g must be finite and >= 0", (double)z_tol);
  DVD_REQUIRE(d_min > 0.0f && d_min <= FLT_MAX, "eval_tracks: d_min=%g must be finite and > 0", (double)d_min);
  const long long HW = (long long)H * W;
  // a row sums H*W terms of at most 2^10 * 2^shift each: they must stay below 2^62
  DVD_REQUIRE(shift >= 1 && shift <= 32 && shift + kEvalCapLog2 + ceil_log2(HW) <= 62,
              "eval_tracks: shift=%d outside 1 .. min(32, 62 - 10 - ceil_log2(H * W)) for H=%d W=%d", shift, H, W);
  DVD_REQUIRE(sums_step_stride >= (long long)B * kEvalSums, "eval_tracks: sums step stride %lld below B * 6", sums_step_stride);
  DVD_REQUIRE(!maps || maps_step_stride >= (long long)B * 3 * HW, "eval_tracks: maps step stride %lld below B * 3 * H * W",
              maps_step_stride);
  EvalArgs a = {};
  a.points = points, a.source = source, a.R = R, a.t = t, a.K = K_T, a.depth_all = depth_all, a.img_all = img_all;
  a.pair_row = pair_row, a.flow = flow_1_2, a.mask = mask;
  a.sums = reinterpret_cast<unsigned long long*>(sums), a.maps = maps;
  a.sums_stride = sums_step_stride, a.maps_stride = maps ? maps_step_stride : 0;
  a.B = B, a.N = N, a.P = P, a.HW = (int)HW, a.k_first = k_first;
  a.tol = 1.0f + z_tol, a.d_min = d_min;
  a.view = track_view(H, W);
  a.scale = (double)(1ULL << shift);
  const double pts = (double)T * B * HW;
  const long long frames = N < T + B ? N : T + B;      // distinct target frames whose depth and colours feed the taps
  bytes_add(DVD_BYTES_GEOMETRY, pts * (12.0 + 12.0 + (pair_row ? 9.0 : 0.0) + (maps ? 12.0 : 0.0)) + 16.0 * (double)frames * HW);
  const bool v4 = (W % 4 == 0) && aligned_to(points, 16) && aligned_to(img_all, 16) && aligned_to(flow_1_2, 16) &&
                  aligned_to(mask, 16) && aligned_to(maps, 16) && (maps_step_stride % 4 == 0 || !maps);
  const int px = v4 ? 4 : 1;
  dim3 grid((unsigned)((HW + 256 * px - 1) / (256 * px)), B, T);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (v4)
    eval_launch<4>(a, grid, s);
  else
    eval_launch<1>(a, grid, s);
  DVD_LAUNCH_OK();
  return DVD_OK;
}

}  // extern "C"
