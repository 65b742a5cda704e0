// The world point of pixel position (xf, yf) at depth d:
//     ray = (x, y, 1) @ K_inv ;  p_cam = d * ray ;  P = p_cam @ R + t        (unproject_ptcld.forward)
// in the fp32 operation order of torch's CPU matmul (rowvec_mat3, dvd_common.h).  The one per-point body of csrc/unproject.hip
// (every pixel of a frame) and csrc/point_track.hip (a query at any position of its frame); both units are built with
// -ffp-contract=off, so the same position, depth and camera give the same bits in either.
#pragma once

#include "dvd_common.h"

namespace dvd {

__device__ __forceinline__ void unproject_point(const float xf, const float yf, const float d, const float* __restrict__ Ki,
                                                const float* __restrict__ R, const float* __restrict__ t, float& P0,
                                                float& P1, float& P2) {
  float r0, r1, r2, q0, q1, q2;
  rowvec_mat3(xf, yf, 1.0f, Ki, r0, r1, r2);
  rowvec_mat3(d * r0, d * r1, d * r2, R, q0, q1, q2);
  P0 = q0 + t[0];
  P1 = q1 + t[1];
  P2 = q2 + t[2];
}

}  // namespace dvd
