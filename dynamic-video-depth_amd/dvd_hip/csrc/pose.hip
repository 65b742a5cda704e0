// Normal equations of the camera refinement from stored flow and depth (gfx950): preprocess.refine_cameras' one launch per
// Levenberg-Marquardt evaluation.
//
// The rows are (pair, a, b, dir), two per stored pair: dir 0 reads flow_1_2[pair] with mask_2[pair], dir 1 flow_2_1[pair] with
// mask_1[pair] (dvd_triangulate's pairing).  Per pixel x = (u, v, 1) of frame a, with the tables' rows of both frames (R camera
// to world, row-major; c = t; K_T, K_inv_T the transposed intrinsics), every multiply and add a separate fp32 operation
// (-ffp-contract=off), every 3-term sum as (p0 + p1) + p2, the divisions IEEE:
//     ray = K_a^-1 x      Ds = D_a(x) * s_a      P = Ds * ray      X = R_a P      Z = X + (c_a - c_b)      Y = R_b^T Z
//     q = K_b Y           proj = q.xy / q.z      x' = x.xy + flow  r = proj - x'
//     considered   mask byte == 0 && D > 0 && D <= FLT_MAX && weight > 0 && 0 <= x'0 <= W-1 && 0 <= x'1 <= H-1
//     gate         0 not considered;  1 considered && q.z >= z_near (live);  2 considered otherwise
// Every comparison is written so that a NaN fails it.  Up to here the kernel is an operation-for-operation contract
// (tests/pose_spec.py restates it); what follows is fp32 arithmetic in no promised order (explicit fused multiply-adds).
// A live observation has |r| = sqrt(r0 r0 + r1 r1), Huber's rho = |r|^2 / 2 and IRLS weight 1 inside the threshold,
// huber (|r| - huber / 2) and huber / |r| outside, both times weight_a(x), and the 2 x 13 Jacobian of r in the local unknowns
// [tau_a, omega_a, sigma_a, tau_b, omega_b] (c += R tau, R <- R Exp(omega), s = exp(sigma)):
//     A = Pi K_b,  Pi = (1 / q.z) [[1, 0, -proj_0], [0, 1, -proj_1]]       B = A M,  M = R_b^T R_a
//     J = [ B | B (e_k x P) | B P | -A | A (Y x e_k) ]
// A thread accumulates over its run of at most kPoseRun pixels, in fp32: the upper triangle of J^T w J (91), J^T w r (13), the
// cost, sum w |r|^2, sum w, the weight of the observations that failed the q.z gate, and the two counts.  The 110 values are
// reduced over the wave by a shuffle tree in fp32 (at most 64 * kPoseRun terms), over the four waves and everything after in
// float64: one partial per (row, block) in the workspace, which a second kernel sums in ascending block order.  No atomics, one
// writer per element, plain vector stores: the same inputs give the same bits.
//
// Nothing is gathered: a thread reads its own pixel of the flow, the mask, the depth and the weight, so no value can make it
// address out of range; a row whose pair or frames lie outside the stores is skipped by the whole block (both cameras, like
// the row itself, are uniform over the block: scalar loads).

#include <float.h>
#include <math.h>

#include "dvd_post.h"

namespace dvd {

constexpr int kPoseBlock = 256;
constexpr int kPoseRun = 16;                             // pixels per thread: what is summed in fp32 before float64 takes over
constexpr int kPosePix = kPoseBlock * kPoseRun;          // pixels per block
constexpr int kPoseSums = 106;                           // 91 + 13 + cost + sum w |r|^2
constexpr int kPoseAcc = 108;                            // ... + sum w + the weight behind the q.z gate
constexpr int kPoseChunk = 9;                            // accumulators whose shuffles are in flight together
constexpr int kPoseCols = 109;                          // a partial: the sums (penalty folded into the cost), sum w, two counts

struct PoseArgs {
  const float *flow_1_2, *flow_2_1;            // [P,H,W,2]
  const unsigned char *mask_1, *mask_2;        // [P,H,W]
  const float *depth, *weight;                 // [N,H,W]; weight may be null (all ones)
  const float *R, *t, *K_T, *K_inv_T, *scale;  // [N,3,3], [N,3], [N,3,3], [N,3,3], [N]
  const int* rows;                             // [R,4]
  double* partial;                             // [R, nblk, kPoseCols]
  float* resid;                                // [R,H,W,2] or null
  unsigned char* gate;                         // [R,H,W] or null
  int P, N, HW, W, nblk;
  float huber, z_near, penalty, xmax, ymax;
};

__device__ __forceinline__ float wave_sum_f32(float v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
  return v;
}

template <bool MAPS>
__global__ __launch_bounds__(kPoseBlock) void pose_normal_eq_kernel(const PoseArgs a) {
  __shared__ float red[4][kPoseAcc + 2];
  const int row = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
  const int pair = a.rows[4 * row], fa = a.rows[4 * row + 1], fb = a.rows[4 * row + 2], dir = a.rows[4 * row + 3];
  const bool valid = pair >= 0 && pair < a.P && fa >= 0 && fa < a.N && fb >= 0 && fb < a.N;      // uniform over the block
  const int p0 = blk * kPosePix + tid;
  double* part = a.partial + ((size_t)row * a.nblk + blk) * kPoseCols;
  if (!valid) {                                // nothing is read; zero sums, and zero maps
    if (tid < kPoseCols) part[tid] = 0.0;
    if (MAPS) {
#pragma unroll 1
      for (int k = 0; k < kPoseRun; ++k) {
        const int p = p0 + k * kPoseBlock;
        if (p < a.HW) {
          const size_t at = (size_t)row * a.HW + p;
          reinterpret_cast<float2*>(a.resid)[at] = make_float2(0.0f, 0.0f);
          a.gate[at] = 0;
        }
      }
    }
    return;
  }
  float Ra[9], Rb[9], Kb[9], Kia[9], d[3], M[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    Ra[i] = a.R[(size_t)fa * 9 + i];
    Rb[i] = a.R[(size_t)fb * 9 + i];
    Kb[i] = a.K_T[(size_t)fb * 9 + i];
    Kia[i] = a.K_inv_T[(size_t)fa * 9 + i];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) d[i] = a.t[(size_t)fa * 3 + i] - a.t[(size_t)fb * 3 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) M[3 * i + j] = (Rb[i] * Ra[j] + Rb[3 + i] * Ra[3 + j]) + Rb[6 + i] * Ra[6 + j];
  const float sa = a.scale[fa];
  const float2* flow = reinterpret_cast<const float2*>(dir ? a.flow_2_1 : a.flow_1_2) + (size_t)pair * a.HW;
  const unsigned char* mask = (dir ? a.mask_1 : a.mask_2) + (size_t)pair * a.HW;
  const float* depth = a.depth + (size_t)fa * a.HW;
  const float* weight = a.weight ? a.weight + (size_t)fa * a.HW : nullptr;

  float acc[kPoseAcc];
#pragma unroll
  for (int k = 0; k < kPoseAcc; ++k) acc[k] = 0.0f;
  int n_live = 0, n_behind = 0;
#pragma unroll 1
  for (int k = 0; k < kPoseRun; ++k) {
    const int p = p0 + k * kPoseBlock;
    if (p >= a.HW) break;
    const float2 fl = flow[p];
    const unsigned char mk = mask[p];
    const float D = depth[p];
    const float wgt = weight ? weight[p] : 1.0f;
    const int v = p / a.W, u = p - v * a.W;
    const float uf = (float)u, vf = (float)v;
    // ---- the contract
    float ray[3], P[3], X[3], Y[3], q[3];
    rowvec_mat3(uf, vf, 1.0f, Kia, ray[0], ray[1], ray[2]);
    const float Ds = D * sa;
    P[0] = Ds * ray[0], P[1] = Ds * ray[1], P[2] = Ds * ray[2];
    rowvec_mat3_T(P[0], P[1], P[2], Ra, X[0], X[1], X[2]);
    rowvec_mat3(X[0] + d[0], X[1] + d[1], X[2] + d[2], Rb, Y[0], Y[1], Y[2]);
    rowvec_mat3(Y[0], Y[1], Y[2], Kb, q[0], q[1], q[2]);
    const float pj0 = q[0] / q[2], pj1 = q[1] / q[2];
    const float xp = uf + fl.x, yp = vf + fl.y;
    const float r0 = pj0 - xp, r1 = pj1 - yp;
    const bool ok = mk == 0 && D > 0.0f && D <= FLT_MAX && wgt > 0.0f && xp >= 0.0f && xp <= a.xmax && yp >= 0.0f && yp <= a.ymax;
    const bool live = ok && q[2] >= a.z_near;
    if (MAPS) {
      const size_t at = (size_t)row * a.HW + p;
      reinterpret_cast<float2*>(a.resid)[at] = live ? make_float2(r0, r1) : make_float2(0.0f, 0.0f);
      a.gate[at] = live ? 1 : (ok ? 2 : 0);
    }
    // ---- the sums
    if (ok && !live) {
      acc[107] += wgt;
      ++n_behind;
    }
    if (live) {
      ++n_live;
      const float nr2 = fmaf(r0, r0, r1 * r1);
      const float nr = sqrtf(nr2);
      const bool inside = nr <= a.huber;
      const float w = inside ? wgt : wgt * (a.huber / nr);
      const float rho = inside ? 0.5f * nr2 : a.huber * (nr - 0.5f * a.huber);
      acc[104] = fmaf(wgt, rho, acc[104]);
      acc[105] = fmaf(w, nr2, acc[105]);
      acc[106] += w;
      const float iz = 1.0f / q[2];
      float J0[13], J1[13];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        float* J = i ? J1 : J0;
        const float pj = i ? pj1 : pj0;
        float A[3], B[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) A[j] = fmaf(-pj, Kb[3 * j + 2], Kb[3 * j + i]) * iz;         // K_b[i][j] = K_T[j][i]
#pragma unroll
        for (int j = 0; j < 3; ++j) B[j] = fmaf(A[2], M[6 + j], fmaf(A[1], M[3 + j], A[0] * M[j]));
        J[0] = B[0], J[1] = B[1], J[2] = B[2];
        J[3] = fmaf(B[2], P[1], -(B[1] * P[2]));
        J[4] = fmaf(B[0], P[2], -(B[2] * P[0]));
        J[5] = fmaf(B[1], P[0], -(B[0] * P[1]));
        J[6] = fmaf(B[2], P[2], fmaf(B[1], P[1], B[0] * P[0]));
        J[7] = -A[0], J[8] = -A[1], J[9] = -A[2];
        J[10] = fmaf(A[1], Y[2], -(A[2] * Y[1]));
        J[11] = fmaf(A[2], Y[0], -(A[0] * Y[2]));
        J[12] = fmaf(A[0], Y[1], -(A[1] * Y[0]));
      }
      int k2 = 0;
#pragma unroll
      for (int i = 0; i < 13; ++i) {
        const float w0 = w * J0[i], w1 = w * J1[i];
        acc[91 + i] = fmaf(w1, r1, fmaf(w0, r0, acc[91 + i]));
#pragma unroll
        for (int j = i; j < 13; ++j, ++k2) acc[k2] = fmaf(w1, J1[j], fmaf(w0, J0[j], acc[k2]));
      }
    }
  }
  // ---- the block's partial: fp32 over the wave, float64 from there
  const int lane = tid & (kWave - 1), wave = tid >> 6;
  // wave_sum_f32's tree, v += shfl_down(v, off) for off = 32 .. 1, on kPoseChunk values at a time: their shuffles are issued
  // together and waited for once per step (one value after another, each of the 648 shuffles waits for its own round trip)
  static_assert(kPoseAcc % kPoseChunk == 0, "the accumulators are reduced in whole chunks");
#pragma unroll
  for (int c0 = 0; c0 < kPoseAcc; c0 += kPoseChunk) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      float other[kPoseChunk];
#pragma unroll
      for (int i = 0; i < kPoseChunk; ++i) other[i] = __shfl_down(acc[c0 + i], off, kWave);
#pragma unroll
      for (int i = 0; i < kPoseChunk; ++i) acc[c0 + i] += other[i];
    }
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < kPoseChunk; ++i) red[wave][c0 + i] = acc[c0 + i];
    }
  }
  {
    const float s0 = wave_sum_f32((float)n_live), s1 = wave_sum_f32((float)n_behind);      // at most 64 * kPoseRun: exact
    if (lane == 0) red[wave][kPoseAcc] = s0, red[wave][kPoseAcc + 1] = s1;
  }
  __syncthreads();
  if (tid < kPoseCols) {
    const int k = tid < 107 ? tid : tid + 1;                                              // 107, 108 -> the counts' columns
    double s = ((double)red[0][k] + (double)red[1][k]) + ((double)red[2][k] + (double)red[3][k]);
    if (tid == 104) {
      const double behind = ((double)red[0][107] + (double)red[1][107]) + ((double)red[2][107] + (double)red[3][107]);
      s += behind * (double)a.penalty;
    }
    part[tid] = s;
  }
}

// sums [R,106], wsum [R], counts [R,2]: the partials of a row in ascending block order
__global__ __launch_bounds__(128) void pose_sum_partials_kernel(const double* partial, int nblk, double* sums, double* wsum,
                                                                long long* counts) {
  const int row = blockIdx.x, k = threadIdx.x;
  if (k >= kPoseCols) return;
  const double* p = partial + (size_t)row * nblk * kPoseCols + k;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += p[(size_t)b * kPoseCols];
  if (k < kPoseSums)
    sums[(size_t)row * kPoseSums + k] = s;
  else if (k == kPoseSums)
    wsum[row] = s;
  else
    counts[(size_t)row * 2 + (k - kPoseSums - 1)] = (long long)s;
}

inline long long pose_blocks(long long HW) { return (HW + kPosePix - 1) / kPosePix; }

}  // namespace dvd

extern "C" {

size_t dvd_pose_workspace_bytes(int R, int H, int W) {
  if (R <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)R * (size_t)dvd::pose_blocks((long long)H * W) * dvd::kPoseCols * sizeof(double);
}

int dvd_pose_normal_eq(const float* flow_1_2, const float* flow_2_1, const unsigned char* mask_1, const unsigned char* mask_2, int P,
                       const float* depth, const float* weight, const float* R, const float* t, const float* K_T,
                       const float* K_inv_T, const float* scale, int N, const int* rows, float huber, float z_near, float penalty,
                       void* workspace, size_t workspace_bytes, double* sums, double* wsum, long long* counts, float* resid,
                       unsigned char* gate, int n_rows, int H, int W, dvd_stream_t stream) {
  using namespace dvd;
  DVD_REQUIRE(flow_1_2 && flow_2_1 && mask_1 && mask_2 && depth && R && t && K_T && K_inv_T && scale && rows && workspace && sums &&
                  wsum && counts,
              "pose_normal_eq: null pointer");
  DVD_REQUIRE((resid == nullptr) == (gate == nullptr), "pose_normal_eq: resid and gate are written together: one is null");
  DVD_REQUIRE(n_rows >= 1 && n_rows <= 65535, "pose_normal_eq: R=%d outside 1 .. 65535 rows per launch", n_rows);
  DVD_REQUIRE(H >= 1 && W >= 1 && (long long)H * W < (1ll << 30), "pose_normal_eq: images of %d x %d", H, W);
  DVD_REQUIRE(P >= 1 && N >= 1, "pose_normal_eq: P=%d pairs, N=%d frames", P, N);
  DVD_REQUIRE(huber > 0.0f && huber <= FLT_MAX, "pose_normal_eq: huber=%g must be finite and > 0", (double)huber);
  DVD_REQUIRE(z_near > 0.0f && z_near <= FLT_MAX, "pose_normal_eq: z_near=%g must be finite and > 0", (double)z_near);
  DVD_REQUIRE(penalty >= 0.0f && penalty <= FLT_MAX, "pose_normal_eq: penalty=%g must be finite and >= 0", (double)penalty);
  DVD_REQUIRE(workspace_bytes >= dvd_pose_workspace_bytes(n_rows, H, W), "pose_normal_eq: workspace of %zu bytes, %zu needed",
              workspace_bytes, dvd_pose_workspace_bytes(n_rows, H, W));
  DVD_REQUIRE(aligned_to(workspace, 8) && aligned_to(flow_1_2, 8) && aligned_to(flow_2_1, 8) && aligned_to(resid, 8),
              "pose_normal_eq: the workspace, the flows and resid must be 8-byte aligned");
  PoseArgs a = {};
  a.flow_1_2 = flow_1_2, a.flow_2_1 = flow_2_1, a.mask_1 = mask_1, a.mask_2 = mask_2, a.depth = depth, a.weight = weight;
  a.R = R, a.t = t, a.K_T = K_T, a.K_inv_T = K_inv_T, a.scale = scale, a.rows = rows;
  a.partial = static_cast<double*>(workspace), a.resid = resid, a.gate = gate;
  a.P = P, a.N = N, a.HW = H * W, a.W = W, a.nblk = (int)pose_blocks(a.HW);
  a.huber = huber, a.z_near = z_near, a.penalty = penalty, a.xmax = (float)(W - 1), a.ymax = (float)(H - 1);
  // per row a flow vector, a mask byte, a depth and a weight of every pixel; with the maps a residual and a gate byte more
  bytes_add(DVD_BYTES_GEOMETRY, (double)n_rows * a.HW * ((weight ? 17.0 : 13.0) + (resid ? 9.0 : 0.0)));
  dim3 grid(a.nblk, n_rows), block(kPoseBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (resid)
    hipLaunchKernelGGL((pose_normal_eq_kernel<true>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((pose_normal_eq_kernel<false>), grid, block, 0, s, a);
  DVD_LAUNCH_OK();
  hipLaunchKernelGGL(pose_sum_partials_kernel, dim3(n_rows), dim3(128), 0, s, a.partial, a.nblk, sums, wsum, counts);
  DVD_LAUNCH_OK();
  return DVD_OK;
}

}  // extern "C"
