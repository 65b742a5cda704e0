// One fixed-point update of the inverse Euler step (gfx950): y_out = p - sf, with max |y_out - y_old| per image.
//
// A forward step of the scene-flow chain is x -> x + s f(x, t) (models/tracks.py); the point y that this step carries to p is the
// fixed point of y <- p - s f(y, t).  The MLP forward delivers sf = s f(y_old, t) (dvd_sf_mlp_fwd, sf_out); this kernel forms
// the next iterate and, in the same pass, how far it moved: resid[b] = max(resid[b], max over image b of |y_out - y_old|), the
// convergence measure Model.track reports.  A NaN difference counts as +Inf (amax_acc), as with dvd_amax.
//
// A pure map: 12 B read and 4 B written per value (8 + 4 where y_old is p).  Every element is read and written by the one
// thread that owns it, so y_old may alias p or y_out.  The residual goes through wave_amax_to: a max over non-negative
// floats taken as unsigned integers, so it does not depend on the order of the waves and is bitwise reproducible.  16-byte
// accesses where H * W is a multiple of 4 and the bases are 16-byte aligned, one value per thread otherwise.  Built with
// -ffp-contract=off like the rest of the geometry (one subtraction per value: the flag only keeps the unit with its class).

#include "dvd_post.h"
#include "dvd_split.h"

namespace dvd {

// (no __restrict__: y_old may be p or y_out)
template <int PX>
__global__ __launch_bounds__(256) void invert_update_kernel(const float* p, const float* sf, const float* y_old, float* y_out,
                                                            float* resid, long long per_img) {
  const int b = blockIdx.y;
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * PX;
  float m = 0.0f;
  if (i < per_img) {                          // (no early return: every lane takes part in the wave's max)
    const long long at = (long long)b * per_img + i;
    if (PX == 4) {
      const float4 a = ld4(p + at), s = ld4(sf + at), o = ld4(y_old + at);
      const float4 y = make_float4(a.x - s.x, a.y - s.y, a.z - s.z, a.w - s.w);
      st4(y_out + at, y);
      m = amax_acc(amax_acc(amax_acc(amax_acc(m, y.x - o.x), y.y - o.y), y.z - o.z), y.w - o.w);
    } else {
      const float o = y_old[at];
      const float y = p[at] - sf[at];
      y_out[at] = y;
      m = amax_acc(m, y - o);
    }
  }
  if (resid) wave_amax_to(m, resid + b);
}

}  // namespace dvd

extern "C" {

int dvd_track_invert_update(const float* p, const float* sf, const float* y_old, float* y_out, float* resid, int B, int HW,
                            dvd_stream_t stream) {
  using namespace dvd;
  DVD_REQUIRE(p && sf && y_old && y_out, "track_invert_update: null pointer");
  DVD_REQUIRE(B > 0 && B <= 65535, "track_invert_update: bad batch B=%d (1 .. 65535 images per launch)", B);
  DVD_REQUIRE(HW > 0 && HW < (1 << 30), "track_invert_update: bad image size H*W=%d", HW);
  const long long per_img = 3LL * HW;
  bytes_add(DVD_BYTES_GEOMETRY, (double)B * per_img * (y_old == p ? 12.0 : 16.0));
  const bool v4 = (HW % 4 == 0) && aligned_to(p, 16) && aligned_to(sf, 16) && aligned_to(y_old, 16) && aligned_to(y_out, 16);
  const int px = v4 ? 4 : 1;
  dim3 grid((unsigned)((per_img + 256 * px - 1) / (256 * px)), B), block(256);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (v4)
    hipLaunchKernelGGL((invert_update_kernel<4>), grid, block, 0, s, p, sf, y_old, y_out, resid, per_img);
  else
    hipLaunchKernelGGL((invert_update_kernel<1>), grid, block, 0, s, p, sf, y_old, y_out, resid, per_img);
  DVD_LAUNCH_OK();
  return DVD_OK;
}

}  // extern "C"
