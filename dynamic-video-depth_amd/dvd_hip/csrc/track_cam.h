// The camera row, the projection core and the point loads shared by the kernels that push world points into a camera of the
// per-frame tables: csrc/track.hip (a gather at the projected position) and csrc/splat.hip (a scatter to it).
//
//     Q = (P - t) @ R_T ;  I = Q @ K        (project_ptcld.forward, the reference's losses/scene_flow_projection.py:27-44)
//
// in the fp32 operation order of torch's CPU matmul (rowvec_mat3, dvd_common.h).  Both units are built with
// -ffp-contract=off, so the same point and the same table row give the same bits in either of them.
#pragma once

#include "dvd_post.h"

namespace dvd {

struct TrackCam {
  float R[9], K[9], t[3];
};

// row g of the tables R [N,3,3], t [N,3], K [N,3,3]
__device__ __forceinline__ void load_track_cam(const float* __restrict__ R, const float* __restrict__ t,
                                               const float* __restrict__ K, int g, TrackCam& c) {
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    c.R[i] = R[(size_t)g * 9 + i];
    c.K[i] = K[(size_t)g * 9 + i];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) c.t[i] = t[(size_t)g * 3 + i];
}

// I = ((P - t) @ R_T) @ K: the one projection core of the forward, the backward and the splat
__device__ __forceinline__ void project_point(const TrackCam& c, float P0, float P1, float P2, float& I0, float& I1,
                                              float& I2) {
  float Q0, Q1, Q2;
  rowvec_mat3(P0 - c.t[0], P1 - c.t[1], P2 - c.t[2], c.R, Q0, Q1, Q2);
  rowvec_mat3(Q0, Q1, Q2, c.K, I0, I1, I2);
}

// ... and its perspective divide: (u, v) = I.xy / (I.z + 1e-8), z = I.z (the compiler's IEEE division; z is not bounded away
// from 0 here).  Every unit that needs a pixel position takes it from here.
__device__ __forceinline__ void project_uvz(const TrackCam& c, float P0, float P1, float P2, float& u, float& v, float& z) {
  float I0, I1;
  project_point(c, P0, P1, P2, I0, I1, z);
  const float den = z + 1e-8f;
  u = I0 / den, v = I1 / den;
}

// PX horizontally adjacent points of image `img`, from pixel p0 on: planar [.,3,H,W] or interleaved [.,H,W,3]
template <int PX, bool PLANAR>
__device__ __forceinline__ void load_points(const float* __restrict__ base, size_t img, int p0, int HW, float P[3][PX]) {
  if (PLANAR) {
    const float* s = base + img * 3 * HW + p0;
#pragma unroll
    for (int c = 0; c < 3; ++c) ldpx<PX>(s + (size_t)c * HW, P[c]);
  } else {
    const float* s = base + (img * HW + p0) * 3;
    float v[3 * PX];
    if (PX == 4) {
#pragma unroll
      for (int q = 0; q < 3; ++q) *reinterpret_cast<float4*>(v + 4 * q) = *reinterpret_cast<const float4*>(s + 4 * q);
    } else {
      v[0] = s[0];
      v[1] = s[1];
      v[2] = s[2];
    }
#pragma unroll
    for (int i = 0; i < PX; ++i) {
      P[0][i] = v[3 * i];
      P[1][i] = v[3 * i + 1];
      P[2][i] = v[3 * i + 2];
    }
  }
}

}  // namespace dvd
