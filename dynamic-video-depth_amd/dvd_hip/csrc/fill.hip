// Push-pull hole filling of V images of C channels (gfx950): the known pixels are averaged down a 2x pyramid, every unknown
// pixel is taken from the coarse-to-fine bilinear interpolation of the levels above it.
//
//   level 0   a = known != 0 ? bias^power : 0 (the power by repeated multiplication, 1 without a bias); a pixel whose a is not
//             finite or not > 0 is unknown, and so is one whose bias is not > 0 where an even power would hide it; the value
//             of an unknown pixel is replaced by 0 before anything is computed from it
//   pull      level l + 1 is (ceil(H_l / 2), ceil(W_l / 2)); with the children (2y+dy, 2x+dx) in the order (0,0) (0,1) (1,0) (1,1)
//             (a child outside the level counts as a = 0, v = 0):  A = ((a0 + a1) + a2) + a3,  n = #{a_c > 0},
//             S = ((a0 v0 + a1 v1) + a2 v2) + a3 v3;  n > 0: v' = S / A, a' = A / n;  else v' = 0, a' = 0
//   push      a pixel with a_l > 0 keeps v_l; any other takes 0.75 * (0.75 P[yp][xp] + 0.25 P[yp][xn]) + 0.25 * (0.75 P[yn][xp] +
//             0.25 P[yn][xn]) of the completed level above, yp = y >> 1, yn = clamp(yp + (y odd ? 1 : -1)), x alike
//   level     0 where the pixel is known, else the lowest level at which an ancestor (y >> k, x >> k) is known; a view without
//             a known pixel is `fill` everywhere and its level 255
//
// Every statement is fp32 in exactly this order (-ffp-contract=off), so the result is a function of the view alone: it does
// not depend on V, on the grid or on the run.  No atomics.  Three launches, whatever H, W and V:
//   fill_pull_kernel   a 256-thread block owns a 32 x 32 tile of level 0 whose origin is a multiple of 32, so levels 1 .. 5 of
//                      the tile nest inside it.  It reads `known`, `bias` and the C planes once, PX pixels per access, reduces
//                      levels 1 .. 5 in LDS and writes them to the workspace, C + 1 planes per level (a, then the values).
//   fill_mid_kernel    one block per view holds level 5 and everything above it in LDS: pulls up to 1 x 1, pushes back down and
//                      writes the completed level 5 over the workspace's, with the known-ancestor level in place of a.
//                      Pulling on past 1 x 1 (an image of at most 32 x 32 reaches it below level 5) changes nothing: the only
//                      child hands its a on unchanged, and the 1 x 1 pixel of the true top keeps its own value on the way down.
//   fill_push_kernel   per level-0 tile: the completed levels 4 .. 1 of the tile with a halo of one pixel, rebuilt in LDS from
//                      the workspace.  One pixel is enough at every level because tiles are 32-aligned: the halo pixel
//                      2^k a - 1 is odd and needs the parents p, p + 1, the halo pixel 2^k a + 2^k is even and needs p, p - 1.
//                      Neighbouring tiles rebuild the shared pixels from the same inputs by the same statements.  Memory is
//                      visited in two rounds, each issued at once (weights and workspace, then the level-0 values), not level
//                      by level: a tile's time is its chain of memory latencies, not its bytes.
// LDS of the middle kernel bounds the image: ceil(H / 32) * ceil(W / 32) <= kFillMaxTiles = 2048 (768 x 1344 has 1008; 1024 x
// 2048 is the largest 1:2 image).  A strip 1 x n halves in one direction only, so the levels above n pixels hold at most
// n + 12 more: 2 * 2048 + 16 pixels of C + 1 <= 9 floats, 148,032 of the 163,840 bytes.

#include <float.h>

#include "dvd_post.h"

namespace dvd {

constexpr int kFillMaxC = 8;
constexpr int kFillTop = 5;                                  // levels 1 .. kFillTop live in the workspace
constexpr int kFillTile = 1 << kFillTop;                     // 32
constexpr int kFillMaxTiles = 2048;
constexpr int kFillMidPixels = 2 * kFillMaxTiles + 16;
constexpr int kFillMidLevels = 16;
constexpr int kFillMidThreads = 1024;
constexpr float kFillEmpty = 255.0f;
// a tile's levels 0 .. 5 back to back: 32^2, 16^2, .. 1
constexpr int kPullPix = 1024 + 256 + 64 + 16 + 4 + 1;
__constant__ int kPullOff[6] = {0, 1024, 1280, 1344, 1360, 1364};
// the push kernel's levels 1 .. 5 with their halo: 18^2, 10^2, 6^2, 4^2, 3^2 (index 0 unused)
constexpr int kPushPix = 324 + 100 + 36 + 16 + 9;
__constant__ int kPushOff[6] = {0, 0, 324, 424, 460, 476};

struct FillArgs {
  const float* values;            // [V,C,H,W]
  const unsigned char* known;     // [V,H,W]
  const float* bias;              // [V,1,H,W] or null
  float* out_values;              // [V,C,H,W]; may be `values`
  unsigned char* out_level;       // [V,H,W]
  float* ws;
  int V, C, H, W, power, inplace;
  float fill;
  int h[kFillTop + 1], w[kFillTop + 1];      // the sizes of levels 0 .. 5
  long long off[kFillTop + 1];               // where level l = 1 .. 5 starts in a view's workspace, in floats
  long long view_stride;                     // floats of workspace per view
};

struct FillMid {                  // level 5 + k, k = 0 .. n - 1, of a view as the middle kernel holds them in LDS
  int n, plane;                   // plane: pixels of all its levels
  int h[kFillMidLevels], w[kFillMidLevels], off[kFillMidLevels];
};

// The pull of one pixel from its four children.
struct FillPull {
  float A;
  int n;
  __device__ __forceinline__ FillPull(float a0, float a1, float a2, float a3)
      : A(((a0 + a1) + a2) + a3), n((a0 > 0.0f) + (a1 > 0.0f) + (a2 > 0.0f) + (a3 > 0.0f)) {}
  __device__ __forceinline__ float weight() const { return n > 0 ? A / (float)n : 0.0f; }
};

__device__ __forceinline__ float fill_pull_value(const FillPull& p, float a0, float v0, float a1, float v1, float a2, float v2,
                                                 float a3, float v3) {
  const float S = ((a0 * v0 + a1 * v1) + a2 * v2) + a3 * v3;
  return p.n > 0 ? S / p.A : 0.0f;
}

// The push of one pixel: P points at the completed level above (row length wp), already offset so that (yp, xp) etc. index it
__device__ __forceinline__ float fill_push_value(const float* P, int wp, int yp, int yn, int xp, int xn) {
  const float top = 0.75f * P[yp * wp + xp] + 0.25f * P[yp * wp + xn];
  const float bot = 0.75f * P[yn * wp + xp] + 0.25f * P[yn * wp + xn];
  return 0.75f * top + 0.25f * bot;
}

// parent and clamped neighbour of coordinate x in a level above of n pixels
__device__ __forceinline__ void fill_parents(int x, int n, int& xp, int& xn) {
  xp = x >> 1;
  xn = xp + ((x & 1) ? 1 : -1);
  xn = xn < 0 ? 0 : (xn > n - 1 ? n - 1 : xn);
}

// four horizontally adjacent pixels of a plane from (y, x), x a multiple of 4; 0 outside the image
template <int PX>
__device__ __forceinline__ void fill_load4(const float* plane, int y, int x, int H, int W, float v[4]) {
  v[0] = v[1] = v[2] = v[3] = 0.0f;
  if (y >= H) return;
  const float* src = plane + (size_t)y * W + x;
  if (PX == 4) {
    if (x < W) ldpx<4>(src, v);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (x + i < W) ldpx<1>(src + i, v + i);
  }
}

// the level-0 weights of those four pixels: the ONE function both the pull and the push go through
template <int PX>
__device__ __forceinline__ void fill_weights(const FillArgs& a, int vw, int y, int x, float a0[4]) {
  unsigned int k[4] = {0u, 0u, 0u, 0u};
  float b[4] = {1.0f, 1.0f, 1.0f, 1.0f};
  const bool biased = a.bias != nullptr && a.power > 0;
  if (y < a.H) {
    const size_t base = ((size_t)vw * a.H + y) * a.W + x;
    if (PX == 4) {
      if (x < a.W) {
        ldpx_bytes<4>(a.known + base, k);
        if (biased) ldpx<4>(a.bias + base, b);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (x + i < a.W) {
          ldpx_bytes<1>(a.known + base + i, k + i);
          if (biased) ldpx<1>(a.bias + base + i, b + i);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float p = 1.0f;
    for (int j = 0; j < a.power; ++j) p *= b[i];
    a0[i] = (k[i] != 0u && b[i] > 0.0f && p > 0.0f && p <= FLT_MAX) ? p : 0.0f;      // false for a NaN
  }
}

template <int PX>
__global__ __launch_bounds__(256) void fill_pull_kernel(const FillArgs a) {
  extern __shared__ float lds[];      // C + 1 planes of kPullPix floats: a, then the values
  const int vw = blockIdx.z, Y0 = blockIdx.y * kFillTile, X0 = blockIdx.x * kFillTile;
  const int ty = threadIdx.x >> 3, tx = (threadIdx.x & 7) * 4;
  const int y = Y0 + ty, x = X0 + tx;
  const size_t HW = (size_t)a.H * a.W;
  float a0[4], v[kFillMaxC][4];
  fill_weights<PX>(a, vw, y, x, a0);
  // every plane's load is issued before the first is used: one trip to memory, not C
#pragma unroll
  for (int c = 0; c < kFillMaxC; ++c)
    if (c < a.C) fill_load4<PX>(a.values + ((size_t)vw * a.C + c) * HW, y, x, a.H, a.W, v[c]);
#pragma unroll
  for (int i = 0; i < 4; ++i) lds[ty * kFillTile + tx + i] = a0[i];
#pragma unroll
  for (int c = 0; c < kFillMaxC; ++c) {
    if (c < a.C) {
#pragma unroll
      for (int i = 0; i < 4; ++i) lds[(1 + c) * kPullPix + ty * kFillTile + tx + i] = a0[i] > 0.0f ? v[c][i] : 0.0f;
    }
  }
  __syncthreads();
  float* wsv = a.ws + (size_t)vw * a.view_stride;
  for (int l = 1; l <= kFillTop; ++l) {
    const int n = kFillTile >> l, ns = 2 * n, src = kPullOff[l - 1], dst = kPullOff[l];
    const int hl = a.h[l], wl = a.w[l];
    for (int idx = threadIdx.x; idx < n * n * (a.C + 1); idx += 256) {
      const int plane = idx / (n * n), p = idx - plane * n * n;
      const int py = p / n, px = p - py * n;
      const int c0 = src + (2 * py) * ns + 2 * px;
      const float* A = lds + c0;
      const FillPull pull(A[0], A[1], A[ns], A[ns + 1]);
      float r;
      if (plane == 0) {
        r = pull.weight();
      } else {
        const float* Vs = lds + plane * kPullPix + c0;
        r = fill_pull_value(pull, A[0], Vs[0], A[1], Vs[1], A[ns], Vs[ns], A[ns + 1], Vs[ns + 1]);
      }
      lds[plane * kPullPix + dst + p] = r;
      const int gy = (Y0 >> l) + py, gx = (X0 >> l) + px;
      if (gy < hl && gx < wl) wsv[a.off[l] + ((size_t)plane * hl + gy) * wl + gx] = r;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kFillMidThreads) void fill_mid_kernel(const FillArgs a, const FillMid g) {
  __shared__ float lds[(kFillMaxC + 1) * kFillMidPixels];      // C + 1 planes of g.plane floats
  const int P = g.plane, n5 = g.h[0] * g.w[0];
  float* wsv = a.ws + (size_t)blockIdx.x * a.view_stride + a.off[kFillTop];
  for (int base = threadIdx.x; base < n5 * (a.C + 1); base += 4 * kFillMidThreads) {      // four loads in flight per thread
    float r[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = base + u * kFillMidThreads;
      r[u] = idx < n5 * (a.C + 1) ? wsv[idx] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = base + u * kFillMidThreads, plane = idx / n5;
      if (idx < n5 * (a.C + 1)) lds[plane * P + (idx - plane * n5)] = r[u];
    }
  }
  __syncthreads();
  for (int k = 1; k < g.n; ++k) {
    const int h = g.h[k], w = g.w[k], hs = g.h[k - 1], ws = g.w[k - 1], src = g.off[k - 1], dst = g.off[k];
    for (int idx = threadIdx.x; idx < h * w * (a.C + 1); idx += kFillMidThreads) {
      const int plane = idx / (h * w), p = idx - plane * h * w;
      const int py = p / w, px = p - py * w;
      const bool in_x = 2 * px + 1 < ws, in_y = 2 * py + 1 < hs;
      const int c0 = src + (2 * py) * ws + 2 * px;
      const float* A = lds + c0;
      const float a0 = A[0], a1 = in_x ? A[1] : 0.0f, a2 = in_y ? A[ws] : 0.0f, a3 = (in_x && in_y) ? A[ws + 1] : 0.0f;
      const FillPull pull(a0, a1, a2, a3);
      float r;
      if (plane == 0) {
        r = pull.weight();
      } else {
        const float* Vs = lds + plane * P + c0;
        r = fill_pull_value(pull, a0, Vs[0], a1, in_x ? Vs[1] : 0.0f, a2, in_y ? Vs[ws] : 0.0f, a3,
                            (in_x && in_y) ? Vs[ws + 1] : 0.0f);
      }
      lds[plane * P + dst + p] = r;
    }
    __syncthreads();
  }
  // from here on the a of a finished level is replaced by the level of its nearest known ancestor
  const int top = g.n - 1;
  if (threadIdx.x == 0) lds[g.off[top]] = lds[g.off[top]] > 0.0f ? (float)(kFillTop + top) : kFillEmpty;
  __syncthreads();
  for (int k = top - 1; k >= 0; --k) {
    const int h = g.h[k], w = g.w[k], hp = g.h[k + 1], wp = g.w[k + 1];
    for (int p = threadIdx.x; p < h * w; p += kFillMidThreads) {      // one thread per pixel: it alone reads and replaces a_l of it
      const int py = p / w, px = p - py * w;
      int yp, yn, xp, xn;
      fill_parents(py, hp, yp, yn);
      fill_parents(px, wp, xp, xn);
      const float al = lds[g.off[k] + p];
      if (!(al > 0.0f)) {
        for (int c = 1; c <= a.C; ++c) lds[c * P + g.off[k] + p] = fill_push_value(lds + c * P + g.off[k + 1], wp, yp, yn, xp, xn);
      }
      lds[g.off[k] + p] = al > 0.0f ? (float)(kFillTop + k) : lds[g.off[k + 1] + yp * wp + xp];
    }
    __syncthreads();
  }
  for (int idx = threadIdx.x; idx < n5 * (a.C + 1); idx += kFillMidThreads) {
    const int plane = idx / n5;
    wsv[idx] = lds[plane * P + (idx - plane * n5)];
  }
}

template <int PX>
__global__ __launch_bounds__(256) void fill_push_kernel(const FillArgs a) {
  extern __shared__ float lds[];      // C + 1 planes of kPushPix floats: a, later the known-ancestor level; then the values
  const int vw = blockIdx.z, Y0 = blockIdx.y * kFillTile, X0 = blockIdx.x * kFillTile;
  const float* wsv = a.ws + (size_t)vw * a.view_stride;
  const int ty = threadIdx.x >> 3, tx = (threadIdx.x & 7) * 4;
  const int y = Y0 + ty, x = X0 + tx;
  const bool inside = y < a.H && x < a.W;
  const size_t HW = (size_t)a.H * a.W;
  // Memory is visited in two rounds, each issued at once: the level-0 weights and the workspace's levels 5 .. 1 of the tile
  // and its halo now, the level-0 values once the weights say whether anything is to be written.  The levels are then
  // completed in LDS alone, while the values are on their way.
  float a0[4];
  fill_weights<PX>(a, vw, y, x, a0);
  // (the kPushPix = 485 pixels of the five levels lie back to back: pixel q of the plane is thread q's, and q + 256's)
  float w[2][kFillMaxC + 1];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int q = threadIdx.x + 256 * r;
    const int l = q < kPushOff[2] ? 1 : q < kPushOff[3] ? 2 : q < kPushOff[4] ? 3 : q < kPushOff[5] ? 4 : 5;
    const int n = (kFillTile >> l) + 2, p = q - kPushOff[l], ly = p / n;
    const int gy = (Y0 >> l) - 1 + ly, gx = (X0 >> l) - 1 + (p - ly * n), hl = a.h[l], wl = a.w[l];
    const bool in = q < kPushPix && gy >= 0 && gy < hl && gx >= 0 && gx < wl;      // a pixel outside its level is never read below
    const float* src = wsv + a.off[l] + (in ? (size_t)gy * wl + gx : 0);
#pragma unroll
    for (int c = 0; c <= kFillMaxC; ++c) w[r][c] = (in && c <= a.C) ? src[(size_t)c * hl * wl] : 0.0f;
  }
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int q = threadIdx.x + 256 * r;
#pragma unroll
    for (int c = 0; c <= kFillMaxC; ++c)
      if (q < kPushPix && c <= a.C) lds[c * kPushPix + q] = w[r][c];
  }
  bool keep = a.inplace != 0;      // every pixel of the access is known and the output is the input: nothing to write
#pragma unroll
  for (int i = 0; i < 4; ++i) keep = keep && (a0[i] > 0.0f || x + i >= a.W);
  float v[kFillMaxC][4];
  if (inside && !keep) {
#pragma unroll
    for (int c = 0; c < kFillMaxC; ++c)
      if (c < a.C) fill_load4<PX>(a.values + ((size_t)vw * a.C + c) * HW, y, x, a.H, a.W, v[c]);
  }
  __syncthreads();
  // level 5 came completed, with the level of its nearest known ancestor in place of a; levels 4 .. 1 follow it
  for (int l = kFillTop - 1; l >= 1; --l) {
    const int n = (kFillTile >> l) + 2, np = (kFillTile >> (l + 1)) + 2;
    const int oy = (Y0 >> l) - 1, ox = (X0 >> l) - 1, poy = (Y0 >> (l + 1)) - 1, pox = (X0 >> (l + 1)) - 1;
    const int hl = a.h[l], wl = a.w[l], hp = a.h[l + 1], wp = a.w[l + 1];
    for (int p = threadIdx.x; p < n * n; p += 256) {      // one thread per pixel: it alone reads and replaces a_l of it
      const int ly = p / n, lx = p - ly * n;
      const int gy = oy + ly, gx = ox + lx;
      if (gy < 0 || gy >= hl || gx < 0 || gx >= wl) continue;
      int yp, yn, xp, xn;
      fill_parents(gy, hp, yp, yn);
      fill_parents(gx, wp, xp, xn);
      yp -= poy, yn -= poy, xp -= pox, xn -= pox;                   // into the halo region of the level above
      const float al = lds[kPushOff[l] + p];
      if (!(al > 0.0f)) {
        for (int c = 1; c <= a.C; ++c)
          lds[c * kPushPix + kPushOff[l] + p] = fill_push_value(lds + c * kPushPix + kPushOff[l + 1], np, yp, yn, xp, xn);
      }
      lds[kPushOff[l] + p] = al > 0.0f ? (float)l : lds[kPushOff[l + 1] + yp * np + xp];
    }
    __syncthreads();
  }
  if (!inside) return;
  const int np = kFillTile / 2 + 2, poy = (Y0 >> 1) - 1, pox = (X0 >> 1) - 1;
  int yp, yn, xp[4], xn[4];
  fill_parents(y, a.h[1], yp, yn);
  yp -= poy, yn -= poy;
  unsigned int lvl[4];
  float kl[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    // (a pixel past the row's end, PX = 1 only, is computed from clamped parents and never stored)
    fill_parents(x + i < a.W ? x + i : a.W - 1, a.w[1], xp[i], xn[i]);
    xp[i] -= pox, xn[i] -= pox;
    kl[i] = lds[kPushOff[1] + yp * np + xp[i]];
    lvl[i] = a0[i] > 0.0f ? 0u : (unsigned int)kl[i];
  }
  const size_t pix = ((size_t)vw * a.H + y) * a.W + x;
  if (PX == 4) {
    stpx_bytes<4>(a.out_level + pix, lvl);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (x + i < a.W) stpx_bytes<1>(a.out_level + pix + i, lvl + i);
  }
  if (keep) return;
#pragma unroll
  for (int c = 0; c < kFillMaxC; ++c) {
    if (c < a.C) {
      const float* P = lds + (1 + c) * kPushPix + kPushOff[1];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (!(a0[i] > 0.0f)) v[c][i] = kl[i] == kFillEmpty ? a.fill : fill_push_value(P, np, yp, yn, xp[i], xn[i]);
      }
      float* dst = a.out_values + ((size_t)vw * a.C + c) * HW + (size_t)y * a.W + x;
      if (PX == 4) {
        stpx<4>(dst, v[c]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (x + i < a.W && !(a.inplace && a0[i] > 0.0f)) stpx<1>(dst + i, v[c] + i);
      }
    }
  }
}

// The sizes of levels 0 .. 5, their places in a view's workspace and the middle kernel's levels; false for a refused shape.
static bool fill_geometry(int V, int C, int H, int W, FillArgs& a, FillMid& g) {
  if (V < 1 || V > 65535 || C < 1 || C > kFillMaxC || H < 1 || W < 1 || (long long)H * W >= (1LL << 30)) return false;
  const long long tiles = (long long)((H + kFillTile - 1) / kFillTile) * ((W + kFillTile - 1) / kFillTile);
  if (tiles > kFillMaxTiles) return false;
  a.V = V, a.C = C, a.H = H, a.W = W;
  a.h[0] = H, a.w[0] = W;
  long long off = 0;
  for (int l = 1; l <= kFillTop; ++l) {
    a.h[l] = (a.h[l - 1] + 1) / 2, a.w[l] = (a.w[l - 1] + 1) / 2;
    a.off[l] = off;
    off += (long long)(C + 1) * a.h[l] * a.w[l];
  }
  a.off[0] = 0;
  a.view_stride = off;
  g.n = 0, g.plane = 0;
  for (int h = a.h[kFillTop], w = a.w[kFillTop];; h = (h + 1) / 2, w = (w + 1) / 2) {
    if (g.n == kFillMidLevels) return false;
    g.h[g.n] = h, g.w[g.n] = w, g.off[g.n] = g.plane;
    g.plane += h * w;
    ++g.n;
    if (h == 1 && w == 1) break;
  }
  return g.plane <= kFillMidPixels;
}

}  // namespace dvd

extern "C" {

size_t dvd_fill_workspace_bytes(int V, int C, int H, int W) {
  dvd::FillArgs a = {};
  dvd::FillMid g = {};
  if (!dvd::fill_geometry(V, C, H, W, a, g)) return 0;
  return (size_t)V * (size_t)a.view_stride * sizeof(float);
}

int dvd_fill_holes(const float* values, const unsigned char* known, const float* bias, int power, float fill, int V, int C,
                   int H, int W, float* out_values, unsigned char* out_level, void* workspace, dvd_stream_t stream) {
  using namespace dvd;
  DVD_REQUIRE(values && known && out_values && out_level && workspace, "fill_holes: null pointer");
  DVD_REQUIRE(power >= 0 && power <= 4, "fill_holes: power=%d outside 0 .. 4", power);
  DVD_REQUIRE(V >= 1 && V <= 65535, "fill_holes: V=%d outside 1 .. 65535 views", V);
  DVD_REQUIRE(C >= 1 && C <= kFillMaxC, "fill_holes: C=%d channels, 1 .. %d are supported", C, kFillMaxC);
  DVD_REQUIRE(H >= 1 && W >= 1 && (long long)H * W < (1LL << 30), "fill_holes: images of %d x %d", H, W);
  FillArgs a = {};
  FillMid g = {};
  DVD_REQUIRE(fill_geometry(V, C, H, W, a, g), "fill_holes: %d x %d has more than %d tiles of 32 x 32 (level 5 and above are held in LDS)",
              H, W, kFillMaxTiles);
  DVD_REQUIRE(aligned_to(values, 4) && aligned_to(bias, 4) && aligned_to(out_values, 4) && aligned_to(workspace, 4),
              "fill_holes: a float pointer is not 4-byte aligned");
  a.values = values, a.known = known, a.bias = bias, a.out_values = out_values, a.out_level = out_level;
  a.ws = static_cast<float*>(workspace);
  a.power = power, a.fill = fill, a.inplace = out_values == values ? 1 : 0;
  const double px = (double)V * H * W, lv = (double)V * (double)a.view_stride * 4.0;
  // both tile kernels read values, known and bias; the pull writes the pyramid, the push reads it (halo not counted) and
  // writes values and level; the middle kernel reads and writes level 5
  bytes_add(DVD_BYTES_GEOMETRY, px * (2.0 * (4.0 * C + 1.0 + (bias && power ? 4.0 : 0.0)) + 4.0 * C + 1.0) + 2.0 * lv +
                                    2.0 * V * (C + 1) * 4.0 * a.h[kFillTop] * a.w[kFillTop]);
  const bool v4 = (W % 4 == 0) && aligned_to(values, 16) && aligned_to(bias, 16) && aligned_to(out_values, 16) &&
                  aligned_to(known, 4) && aligned_to(out_level, 4);
  dim3 grid((W + kFillTile - 1) / kFillTile, (H + kFillTile - 1) / kFillTile, V), block(256);
  const size_t pull_lds = (size_t)(C + 1) * kPullPix * sizeof(float), push_lds = (size_t)(C + 1) * kPushPix * sizeof(float);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (v4)
    hipLaunchKernelGGL((fill_pull_kernel<4>), grid, block, pull_lds, s, a);
  else
    hipLaunchKernelGGL((fill_pull_kernel<1>), grid, block, pull_lds, s, a);
  DVD_LAUNCH_OK();
  hipLaunchKernelGGL(fill_mid_kernel, dim3(V), dim3(kFillMidThreads), 0, s, a, g);
  DVD_LAUNCH_OK();
  if (v4)
    hipLaunchKernelGGL((fill_push_kernel<4>), grid, block, push_lds, s, a);
  else
    hipLaunchKernelGGL((fill_push_kernel<1>), grid, block, push_lds, s, a);
  DVD_LAUNCH_OK();
  return DVD_OK;
}

}  // extern "C"
