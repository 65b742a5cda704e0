// Triangulated depth and epipolar motion cue from stored flow and cameras (gfx950).
//
// A flow vector and two cameras are two rays.  For a static point they meet; for a moving one the flow leaves the epipolar
// line.  Per query frame a (frames[b]) and pixel x = (u, v, 1) the kernel walks the frame's row of the observation table
// obs [B, M, 3] = (pair, other frame, dir), pair = -1 being padding anywhere in the row:
//     dir 0   flow_1_2[pair] with mask_2[pair]   (a is the pair's first frame)
//     dir 1   flow_2_1[pair] with mask_1[pair]   (a is the pair's second frame)
// the pairing of the training loss (ops.warp_loss_fused).  Per observation, with the tables' own rows of both frames (R camera
// to world, row-major; c = t the camera centre; K_T, K_inv_T the transposed intrinsics), every multiply and add a separate fp32
// operation (-ffp-contract=off), every 3-term sum as (p0 + p1) + p2, divisions and the square root IEEE:
//     x' = x + flow
//     d1 = R_a (K_a^-1 x)     d2 = R_b (K_b^-1 x')     bl = c_b - c_a
//     A = d1.d1   Bq = d1.d2   C = d2.d2   E = d1.bl   F = d2.bl   den = A C - Bq Bq
//     s1 = (E C - Bq F) / den      s2 = (Bq E - A F) / den      sin2 = den / (A C)
//     h0 = K_b (R_b^T (c_a - c_b))   h1 = K_b (R_b^T d1)   l = h0 x h1
//     e = |(l0 x'0 + l1 x'1) + l2| / sqrt(l0 l0 + l1 l1),  then e = e <= 1e30 ? e : 1e30   (a NaN becomes 1e30)
//     usable      mask byte == 0  &&  0 <= x'0 <= W-1  &&  0 <= x'1 <= H-1  &&  sin2 >= sin2_min
//     consistent  usable && e <= epi_tol && z_near <= s1 <= 1e30 && z_near <= s2 <= 1e30
// Every comparison is written so that a NaN fails it.  The fusion over the consistent observations, in ascending table order:
//     mean     depth = (sum of sin2 * s1) / (sum of sin2)
//     median   the exact median of the s1; (lo + hi) * 0.5 of the two middle ones for an even count
//     depth = 0 where count < min_count;  spread = (max s1 - min s1) / depth, at most 1e30, 0 where depth == 0
//     epi = (sum of e over the usable observations) / usable, -1 where usable == 0
// sin2_min > 0 and the caps of 1e30 keep every sum of at most 32 terms finite: no output ever holds a NaN or an Inf.
//
// Nothing is gathered: the thread reads its OWN pixel of each flow and mask and nothing at the target x', so no flow value can
// make it address out of range; pair and frame indices outside the stores skip the row (they are uniform over the block, as are
// both cameras: scalar loads).  One thread per pixel, grid (ceil(HW / 256), B): a wave reads 512 contiguous bytes of flow as
// float2 and 64 of mask per observation and writes 256 contiguous bytes per fp32 output.  The median's up to 32 samples per pixel
// would be a run-time indexed private array, i.e. scratch memory; they live in LDS instead, [M][256] floats per block (32 KiB at
// the cap), each pixel's column touched by its own thread only -- no barrier -- and the middle elements are picked by rank
// counting (column_median, dvd_post.h).  No atomics, one writer per output element: the same inputs give the same bits.

#include <float.h>

#include "dvd_post.h"

namespace dvd {

constexpr int kTriMaxObs = 32;
constexpr int kTriBlock = 256;
constexpr float kTriCap = 1e30f;

struct TriArgs {
  const float *flow_1_2, *flow_2_1;            // [P,H,W,2]
  const unsigned char *mask_1, *mask_2;        // [P,H,W]
  const int *obs, *frames;                     // [B,M,3], [B]
  const float *R, *t, *K_T, *K_inv_T;          // [N,3,3], [N,3], [N,3,3], [N,3,3]
  float *depth, *epi, *spread;                 // [B,1,H,W]
  unsigned char *count, *usable;               // [B,H,W]
  int P, N, M, B, H, W, HW, min_count;
  float epi_tol, sin2_min, z_near;
};

struct TriCam {
  float R[9], t[3], K[9], Ki[9];               // K, Ki: the transposed tables' rows
};

__device__ __forceinline__ void load_tri_cam(const TriArgs& a, int f, TriCam& c) {
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    c.R[i] = a.R[(size_t)f * 9 + i];
    c.K[i] = a.K_T[(size_t)f * 9 + i];
    c.Ki[i] = a.K_inv_T[(size_t)f * 9 + i];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) c.t[i] = a.t[(size_t)f * 3 + i];
}

__device__ __forceinline__ float dot3(const float* p, const float* q) { return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]; }

template <bool MEDIAN>
__global__ __launch_bounds__(kTriBlock) void triangulate_kernel(const TriArgs a) {
  extern __shared__ float smp[];               // MEDIAN: [M][256], column = pixel of the block
  const int b = blockIdx.y;
  const int p = blockIdx.x * kTriBlock + threadIdx.x;
  if (p >= a.HW) return;
  const size_t pix = (size_t)b * a.HW + p;
  const int fa = a.frames[b];                  // uniform over the block
  const int col = threadIdx.x;
  float acc = 0.0f, ws = 0.0f, esum = 0.0f, lo = INFINITY, hi = -INFINITY;
  int n = 0, nu = 0;
  if (fa >= 0 && fa < a.N) {                   // (a query frame that is no frame: nothing is read, count = usable = 0)
    TriCam ca;
    load_tri_cam(a, fa, ca);
    const int v = p / a.W, u = p - v * a.W;
    const float uf = (float)u, vf = (float)v;
    const float xmax = (float)(a.W - 1), ymax = (float)(a.H - 1);
    float r1[3], d1[3];
    rowvec_mat3(uf, vf, 1.0f, ca.Ki, r1[0], r1[1], r1[2]);
    rowvec_mat3_T(r1[0], r1[1], r1[2], ca.R, d1[0], d1[1], d1[2]);
    const float A = dot3(d1, d1);
    const int* row = a.obs + (size_t)b * a.M * 3;
    for (int m = 0; m < a.M; ++m) {
      const int pair = row[3 * m], fb = row[3 * m + 1], dir = row[3 * m + 2];
      if (pair < 0 || pair >= a.P || fb < 0 || fb >= a.N) continue;          // padding, or an index outside the stores
      const size_t at = (size_t)pair * a.HW + p;
      const float2 fl = reinterpret_cast<const float2*>(dir ? a.flow_2_1 : a.flow_1_2)[at];
      const unsigned char mk = (dir ? a.mask_1 : a.mask_2)[at];
      TriCam cb;
      load_tri_cam(a, fb, cb);
      const float xp = uf + fl.x, yp = vf + fl.y;
      float r2[3], d2[3], bl[3], g[3], q[3], h0[3], h1[3];
      rowvec_mat3(xp, yp, 1.0f, cb.Ki, r2[0], r2[1], r2[2]);
      rowvec_mat3_T(r2[0], r2[1], r2[2], cb.R, d2[0], d2[1], d2[2]);
#pragma unroll
      for (int i = 0; i < 3; ++i) bl[i] = cb.t[i] - ca.t[i], g[i] = ca.t[i] - cb.t[i];
      const float Bq = dot3(d1, d2), C = dot3(d2, d2), E = dot3(d1, bl), F = dot3(d2, bl);
      const float AC = A * C;
      const float den = AC - Bq * Bq;
      const float s1 = (E * C - Bq * F) / den, s2 = (Bq * E - A * F) / den;
      const float sin2 = den / AC;
      rowvec_mat3(g[0], g[1], g[2], cb.R, q[0], q[1], q[2]);
      rowvec_mat3(q[0], q[1], q[2], cb.K, h0[0], h0[1], h0[2]);
      rowvec_mat3(d1[0], d1[1], d1[2], cb.R, q[0], q[1], q[2]);
      rowvec_mat3(q[0], q[1], q[2], cb.K, h1[0], h1[1], h1[2]);
      const float l0 = h0[1] * h1[2] - h0[2] * h1[1];
      const float l1 = h0[2] * h1[0] - h0[0] * h1[2];
      const float l2 = h0[0] * h1[1] - h0[1] * h1[0];
      float e = fabsf((l0 * xp + l1 * yp) + l2) / sqrtf(l0 * l0 + l1 * l1);
      e = e <= kTriCap ? e : kTriCap;
      const bool use = mk == 0 && xp >= 0.0f && xp <= xmax && yp >= 0.0f && yp <= ymax && sin2 >= a.sin2_min;
      const bool con = use && e <= a.epi_tol && s1 >= a.z_near && s1 <= kTriCap && s2 >= a.z_near && s2 <= kTriCap;
      if (use) {
        esum += e;
        ++nu;
      }
      if (con) {
        if (MEDIAN) {
          smp[n * kTriBlock + col] = s1;
        } else {
          acc += sin2 * s1;
          ws += sin2;
        }
        lo = s1 < lo ? s1 : lo;
        hi = s1 > hi ? s1 : hi;
        ++n;
      }
    }
  }
  float dep = 0.0f, spr = 0.0f;
  if (n >= a.min_count && n > 0) {
    dep = MEDIAN ? column_median(smp + col, kTriBlock, n, 0.0f) : acc / ws;
    if (dep != 0.0f) {
      spr = (hi - lo) / dep;
      spr = spr <= kTriCap ? spr : kTriCap;
    }
  }
  a.depth[pix] = dep;
  a.spread[pix] = spr;
  a.epi[pix] = nu > 0 ? esum / (float)nu : -1.0f;
  a.count[pix] = (unsigned char)n;
  a.usable[pix] = (unsigned char)nu;
}

}  // namespace dvd

extern "C" {

int dvd_triangulate(const float* flow_1_2, const float* flow_2_1, const unsigned char* mask_1, const unsigned char* mask_2, int P,
                    const int* obs, const int* frames, long long live_rows, const float* R, const float* t, const float* K_T,
                    const float* K_inv_T, int N, int mode, float epi_tol, float sin2_min, float z_near, int min_count,
                    float* depth, unsigned char* count, unsigned char* usable, float* epi, float* spread, int M, int B, int H,
                    int W, dvd_stream_t stream) {
  using namespace dvd;
  DVD_REQUIRE(frames && R && t && K_T && K_inv_T && depth && count && usable && epi && spread, "triangulate: null pointer");
  DVD_REQUIRE(M >= 0 && M <= kTriMaxObs, "triangulate: M=%d outside 0 .. %d observations per frame", M, kTriMaxObs);
  DVD_REQUIRE(M == 0 || (flow_1_2 && flow_2_1 && mask_1 && mask_2 && obs), "triangulate: null flow, mask or obs with M=%d", M);
  DVD_REQUIRE(mode == 0 || mode == 1, "triangulate: mode=%d is neither 0 (mean) nor 1 (median)", mode);
  DVD_REQUIRE(B >= 1 && B <= 65535, "triangulate: B=%d outside 1 .. 65535 frames per launch", B);
  DVD_REQUIRE(H >= 1 && W >= 1 && (long long)H * W < (1ll << 30), "triangulate: images of %d x %d", H, W);
  DVD_REQUIRE(P >= 0 && N >= 1, "triangulate: P=%d pairs, N=%d frames", P, N);
  DVD_REQUIRE(live_rows >= 0 && live_rows <= (long long)B * M, "triangulate: live_rows=%lld outside 0 .. B * M", live_rows);
  DVD_REQUIRE(epi_tol >= 0.0f && epi_tol <= FLT_MAX, "triangulate: epi_tol=%g must be finite and >= 0", (double)epi_tol);
  DVD_REQUIRE(sin2_min > 0.0f && sin2_min <= 1.0f, "triangulate: sin2_min=%g must be in (0, 1]", (double)sin2_min);
  DVD_REQUIRE(z_near >= 0.0f && z_near <= FLT_MAX, "triangulate: z_near=%g must be finite and >= 0", (double)z_near);
  DVD_REQUIRE(min_count >= 1 && min_count <= 255, "triangulate: min_count=%d outside 1 .. 255", min_count);
  TriArgs a = {};
  a.flow_1_2 = flow_1_2, a.flow_2_1 = flow_2_1, a.mask_1 = mask_1, a.mask_2 = mask_2, a.obs = obs, a.frames = frames;
  a.R = R, a.t = t, a.K_T = K_T, a.K_inv_T = K_inv_T;
  a.depth = depth, a.epi = epi, a.spread = spread, a.count = count, a.usable = usable;
  a.P = P, a.N = N, a.M = M, a.B = B, a.H = H, a.W = W, a.HW = H * W, a.min_count = min_count;
  a.epi_tol = epi_tol, a.sin2_min = sin2_min, a.z_near = z_near;
  // per live observation a flow vector and a mask byte of every pixel; three fp32 and two byte outputs per query pixel
  bytes_add(DVD_BYTES_GEOMETRY, (double)a.HW * (9.0 * (double)live_rows + 14.0 * B));
  dim3 grid((a.HW + kTriBlock - 1) / kTriBlock, B), block(kTriBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mode == 1)
    hipLaunchKernelGGL((triangulate_kernel<true>), grid, block, (size_t)M * kTriBlock * sizeof(float), s, a);
  else
    hipLaunchKernelGGL((triangulate_kernel<false>), grid, block, 0, s, a);
  DVD_LAUNCH_OK();
  return DVD_OK;
}

}  // extern "C"
