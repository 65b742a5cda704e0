// Stored optical flows chained into the frame gaps nobody computed (gfx950).
//
// A gap-g flow is g gap-1 flows followed one after another -- or fewer, longer stored ones.  Per chain b of the table
// links [B, L, 2] = (pair, dir), 1 <= L <= 32, one thread per pixel x0 = (u, v) walks the links in order from x_0 = x0:
//     dir 0   follows flow_1_2[pair], whose validity is mask_2[pair]
//     dir 1   follows flow_2_1[pair], whose validity is mask_1[pair]          (dvd_triangulate's convention)
//     pair = -1 ends the chain; every later link of the row is ignored
// Link k at x_k = (px, py), every multiply and add a separate fp32 operation (-ffp-contract=off):
//     breaks unless 0 <= px <= W-1 && 0 <= py <= H-1 (a NaN fails), and where pair is outside 0 .. P-1 (nothing is read)
//     ix = floorf(px), iy = floorf(py), wx = px - ix, wy = py - iy
//     taps (ix, iy) (ix+1, iy) (ix, iy+1) (ix+1, iy+1) with weights (1-wx)(1-wy), wx(1-wy), (1-wx)wy, wx wy
//     a tap whose weight is exactly 0 is neither read nor tested: a position on the last row or column stays inside the image
//     breaks if the link's mask is non-zero at any tap that is read
//     f = ((t00 * w00 + t10 * w10) + t01 * w01) + t11 * w11 per component, an unread tap as +0
//     x_{k+1} = x_k + f;  breaks if a component of x_{k+1} is a NaN or an Inf (what keeps the outputs finite)
// Row k of flow_out is x_{k+1} - x0 and stays at the last value before a break ((0, 0) if link 0 broke); row k of broken is 0
// while the chain is whole, then 1 + the index of the link that broke.  Rows past a chain's end: flow 0, broken 255.
//
// A gather-bound kernel.  A wave's 64 pixels are neighbours in a row, and a flow field is smooth, so their taps are neighbours
// too: the two taps of a tap row are two float2, 16 adjacent bytes, and a wave's 64 tap pairs fall into the same few 128-byte
// lines its neighbours read (about 512 contiguous bytes per tap row, 64 contiguous mask bytes); the second tap row is the
// first one of the wave one image row below.  What has to come from HBM is therefore one float2 and one mask byte per pixel
// and link, 9 bytes, against 9 bytes written: 18 bytes per pixel and link; the four-fold re-reads are L1 / L2 hits.  No tap
// address depends on anything but a position already tested against the image, and the +1 taps are clamped besides, so no flow
// value can make a thread address out of range.  The links row, pair and dir are uniform over the block (scalar loads).  No
// atomics, one writer per element, plain vector stores: the same inputs give the same bits.

#include <float.h>
#include <stdint.h>

#include "dvd_common.h"

namespace dvd {

constexpr int kChainMaxLinks = 32;
constexpr int kChainBlock = 256;

struct ChainArgs {
  const float *flow_1_2, *flow_2_1;            // [P,H,W,2]
  const unsigned char *mask_1, *mask_2;        // [P,H,W]
  const int* links;                            // [B,L,2]
  float* flow_out;                             // [L,B,H,W,2], rows flow_stride floats apart
  unsigned char* broken;                       // [L,B,H,W]
  long long flow_stride;
  int P, L, B, H, W, HW;
};

__global__ __launch_bounds__(kChainBlock) void flow_chain_kernel(const ChainArgs a) {
  const int b = blockIdx.y;
  const int p = blockIdx.x * kChainBlock + threadIdx.x;
  if (p >= a.HW) return;
  const int v = p / a.W, u = p - v * a.W;
  const float x0 = (float)u, y0 = (float)v;
  const float xmax = (float)(a.W - 1), ymax = (float)(a.H - 1);
  const size_t at = (size_t)b * a.HW + p, plane = (size_t)a.B * a.HW;
  const int* row = a.links + (size_t)b * a.L * 2;          // uniform over the block
  float px = x0, py = y0, dx = 0.0f, dy = 0.0f;
  unsigned char brk = 0;
  int k = 0;
  for (; k < a.L; ++k) {
    const int pair = row[2 * k], dir = row[2 * k + 1];
    if (pair == -1) break;
    if (brk == 0) {
      bool ok = pair >= 0 && pair < a.P && px >= 0.0f && px <= xmax && py >= 0.0f && py <= ymax;
      if (ok) {
        const float fx = floorf(px), fy = floorf(py);
        const float wx = px - fx, wy = py - fy;
        const float ux = 1.0f - wx, uy = 1.0f - wy;
        const float w00 = ux * uy, w10 = wx * uy, w01 = ux * wy, w11 = wx * wy;
        const int ix = (int)fx, iy = (int)fy;
        // (a +1 tap with a weight other than 0 is inside: wx != 0 means px > ix, so ix + 1 <= W-1; the clamp costs nothing)
        const int ix1 = ix + 1 < a.W ? ix + 1 : a.W - 1, iy1 = iy + 1 < a.H ? iy + 1 : a.H - 1;
        const float2* fl = reinterpret_cast<const float2*>(dir ? a.flow_2_1 : a.flow_1_2) + (size_t)pair * a.HW;
        const unsigned char* mk = (dir ? a.mask_1 : a.mask_2) + (size_t)pair * a.HW;
        const int r0 = iy * a.W, r1 = iy1 * a.W;
        float2 t00 = make_float2(0.0f, 0.0f), t10 = t00, t01 = t00, t11 = t00;
        unsigned int m = 0;
        if (w00 != 0.0f) t00 = fl[r0 + ix], m |= mk[r0 + ix];
        if (w10 != 0.0f) t10 = fl[r0 + ix1], m |= mk[r0 + ix1];
        if (w01 != 0.0f) t01 = fl[r1 + ix], m |= mk[r1 + ix];
        if (w11 != 0.0f) t11 = fl[r1 + ix1], m |= mk[r1 + ix1];
        const float sx = ((t00.x * w00 + t10.x * w10) + t01.x * w01) + t11.x * w11;
        const float sy = ((t00.y * w00 + t10.y * w10) + t01.y * w01) + t11.y * w11;
        const float nx = px + sx, ny = py + sy;
        ok = m == 0 && fabsf(nx) <= FLT_MAX && fabsf(ny) <= FLT_MAX;          // (a NaN fails)
        if (ok) {
          px = nx, py = ny;
          dx = px - x0, dy = py - y0;
        }
      }
      if (!ok) brk = (unsigned char)(k + 1);
    }
    *reinterpret_cast<float2*>(a.flow_out + (size_t)k * a.flow_stride + at * 2) = make_float2(dx, dy);
    a.broken[(size_t)k * plane + at] = brk;
  }
  for (; k < a.L; ++k) {                                    // rows past the chain's end
    *reinterpret_cast<float2*>(a.flow_out + (size_t)k * a.flow_stride + at * 2) = make_float2(0.0f, 0.0f);
    a.broken[(size_t)k * plane + at] = 255;
  }
}

}  // namespace dvd

extern "C" {

int dvd_flow_chain(const float* flow_1_2, const float* flow_2_1, const unsigned char* mask_1, const unsigned char* mask_2, int P,
                   const int* links, long long live_links, float* flow_out, long long flow_stride, unsigned char* broken, int L,
                   int B, int H, int W, dvd_stream_t stream) {
  using namespace dvd;
  DVD_REQUIRE(flow_1_2 && flow_2_1 && mask_1 && mask_2 && links && flow_out && broken, "flow_chain: null pointer");
  DVD_REQUIRE(L >= 1 && L <= kChainMaxLinks, "flow_chain: L=%d outside 1 .. %d links per chain", L, kChainMaxLinks);
  DVD_REQUIRE(B >= 1 && B <= 65535, "flow_chain: B=%d outside 1 .. 65535 chains per launch", B);
  DVD_REQUIRE(H >= 2 && W >= 2 && (long long)H * W < (1ll << 30), "flow_chain: images of %d x %d; the sampling rule needs H, W >= 2 and H * W < 2^30", H, W);
  DVD_REQUIRE(P >= 1, "flow_chain: P=%d pairs", P);
  DVD_REQUIRE(flow_stride >= (long long)B * H * W * 2 && flow_stride % 2 == 0,
              "flow_chain: a row stride of %lld floats, below the B * H * W * 2 = %lld of a row (or odd)", flow_stride, (long long)B * H * W * 2);
  DVD_REQUIRE(live_links >= 0 && live_links <= (long long)B * L, "flow_chain: live_links=%lld outside 0 .. B * L", live_links);
  DVD_REQUIRE(((uintptr_t)flow_1_2 | (uintptr_t)flow_2_1 | (uintptr_t)flow_out) % 8 == 0 && (uintptr_t)links % 4 == 0,
              "flow_chain: misaligned pointer (flows 8 bytes, links 4)");
  ChainArgs a = {};
  a.flow_1_2 = flow_1_2, a.flow_2_1 = flow_2_1, a.mask_1 = mask_1, a.mask_2 = mask_2, a.links = links;
  a.flow_out = flow_out, a.broken = broken, a.flow_stride = flow_stride;
  a.P = P, a.L = L, a.B = B, a.H = H, a.W = W, a.HW = H * W;
  // per live link a flow vector and a mask byte of every pixel; a flow vector and a byte written per pixel of every row
  bytes_add(DVD_BYTES_GEOMETRY, (double)a.HW * 9.0 * ((double)live_links + (double)B * L));
  dim3 grid((a.HW + kChainBlock - 1) / kChainBlock, B), block(kChainBlock);
  hipLaunchKernelGGL(flow_chain_kernel, grid, block, 0, static_cast<hipStream_t>(stream), a);
  DVD_LAUNCH_OK();
  return DVD_OK;
}

}  // extern "C"
