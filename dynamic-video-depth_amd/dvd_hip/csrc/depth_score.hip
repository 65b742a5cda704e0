// A predicted depth scored against its ground truth: the error terms of the depth-estimation literature, reduced on chip to
// exact integer sums per frame and region (gfx950).
//
// What it extends (reference, /root/reference): the validation of models/scene_flow_motion_field.py (`_vali_on_batch`,
// disp_vali's threshold gt > 1e-2) knows one scalar; the numbers a paper reports -- abs-rel, sq-rel, RMSE, log-RMSE, the
// delta < 1.25^k accuracies, over all / static / dynamic pixels, after aligning the prediction by one scale -- are computed here.
//
// Per pixel of frame n, in fp32 (the unit is built with -ffp-contract=off):
//     q        scale[n] * pred                  (scale lives on the device: dvd_ratio_median's output, or ones)
//     counted  gt > g_min && pred > 0 && q is finite && the mask byte, if a mask is given, is non-zero
//     d        q - g
//     abs_rel  min(|d| / g, 1024)     sq_rel  min(d * d / g, 1024)     sq  min(d * d, 1024)
//     l        min(max(logf(q) - logf(g), -32), 32)          l2  min(l * l, 1024)
//     delta_k  max(q / g, g / q) < 1.25^k,  k = 1, 2, 3
// (fminf / fmaxf drop a NaN, so every term is finite and at most 2^10 in magnitude.)  Region 0 is every counted pixel, region 1
// those with seg <= 0.5 (static), region 2 those with seg > 0.5 (dynamic); without seg rows 1 and 2 receive nothing.
// Nine words per (frame, region): n, sum q(abs_rel), sum q(sq_rel), sum q(sq), sum q(l2), sum q(l), n_delta1, n_delta2, n_delta3
// with q(x) = llrint((double)x * 2^shift); l is signed and summed in two's complement.  Per-thread registers, a shuffle tree
// over the 64 lanes, LDS across the four waves, then at most nine integer atomicAdd per block and region (zeros are skipped):
// integer adds commute and are exact, so the sums are bitwise reproducible and independent of the grid.
// 8 B per pixel are streamed (+ 4 with seg, + 1 with a mask, + 13 with maps).  One thread per 4 horizontally adjacent pixels
// where W % 4 == 0 and the bases are 16-byte aligned, one pixel per thread otherwise; a block walks up to four strips of 256
// threads of its frame, grid-stride, before it reduces (27 64-bit wave reductions per block with seg are the cost to amortise).

#include <float.h>

#include "dvd_post.h"

namespace dvd {

constexpr float kScoreCap = 1024.0f;
constexpr int kScoreCapLog2 = 10;
constexpr float kScoreLogCap = 32.0f;
constexpr int kScoreSums = 9;
constexpr int kScoreRegions = 3;
constexpr int kScoreTrips = 4;      // strips of 256 threads a block walks (the grid is sized for it; any grid gives the same sums)

struct ScoreArgs {
  const float *pred, *gt, *scale, *seg;      // [N,1,H,W], [N,1,H,W], [N], [N,H,W] or null
  const unsigned char* mask;                 // [N,H,W] or null
  unsigned long long* sums;                  // [N,3,9]
  float* maps;                               // [N,3,H,W] or null
  unsigned char* counted;                    // [N,H,W] or null (with maps)
  int HW;
  float g_min;
  double scale2;                             // 2^shift
};

template <int PX, bool SEG, bool MASK, bool MAPS>
__global__ __launch_bounds__(256) void depth_score_kernel(const ScoreArgs a) {
  constexpr int R = SEG ? kScoreRegions : 1;
  constexpr int kStatic = SEG ? 1 : 0, kDynamic = SEG ? 2 : 0;      // (rows that exist only with seg)
  const int n = blockIdx.y;
  long long acc[R * kScoreSums];      // [region][word]
#pragma unroll
  for (int k = 0; k < R * kScoreSums; ++k) acc[k] = 0;
  const float sc = a.scale[n];
  // a block walks up to kScoreTrips strips of its frame, so that the reduction below is paid once per 4096 (1024) pixels
  for (int p0 = (blockIdx.x * 256 + threadIdx.x) * PX; p0 < a.HW; p0 += gridDim.x * 256 * PX) {
    const size_t o = (size_t)n * a.HW + p0;
    float p[PX], g[PX], sg[PX], m_abs[PX], m_sq[PX], m_l[PX];
    unsigned int mk[PX], cnt[PX];
    ldpx<PX>(a.pred + o, p);
    ldpx<PX>(a.gt + o, g);
    if (SEG) ldpx<PX>(a.seg + o, sg);
    if (MASK) ldpx_bytes<PX>(a.mask + o, mk);
#pragma unroll
    for (int i = 0; i < PX; ++i) {
      const float q = sc * p[i];
      const bool ok = g[i] > a.g_min && p[i] > 0.0f && fabsf(q) <= FLT_MAX && (!MASK || mk[i] != 0u);
      m_abs[i] = m_sq[i] = m_l[i] = 0.0f;
      cnt[i] = ok ? 1u : 0u;
      if (!ok) continue;
      const float d = q - g[i];
      const float dd = d * d;
      const float abs_rel = fminf(fabsf(d) / g[i], kScoreCap);
      const float sq_rel = fminf(dd / g[i], kScoreCap);
      const float sq = fminf(dd, kScoreCap);
      const float l = fminf(fmaxf(logf(q) - logf(g[i]), -kScoreLogCap), kScoreLogCap);
      const float l2 = fminf(l * l, kScoreCap);
      const float ratio = fmaxf(q / g[i], g[i] / q);
      long long t[kScoreSums];
      t[0] = 1;
      t[1] = fixed_q(abs_rel, a.scale2);
      t[2] = fixed_q(sq_rel, a.scale2);
      t[3] = fixed_q(sq, a.scale2);
      t[4] = fixed_q(l2, a.scale2);
      t[5] = fixed_q(l, a.scale2);
      t[6] = ratio < 1.25f ? 1 : 0;
      t[7] = ratio < 1.5625f ? 1 : 0;
      t[8] = ratio < 1.953125f ? 1 : 0;
      m_abs[i] = abs_rel, m_sq[i] = sq, m_l[i] = l;
#pragma unroll
      for (int k = 0; k < kScoreSums; ++k) acc[k] += t[k];
      if (SEG) {
        const bool stat = sg[i] <= 0.5f, dyn = sg[i] > 0.5f;      // a NaN is neither
#pragma unroll
        for (int k = 0; k < kScoreSums; ++k) {
          acc[kStatic * kScoreSums + k] += stat ? t[k] : 0;
          acc[kDynamic * kScoreSums + k] += dyn ? t[k] : 0;
        }
      }
    }
    if (MAPS) {
      float* m = a.maps + (size_t)n * 3 * a.HW + p0;
      stpx<PX>(m, m_abs);
      stpx<PX>(m + a.HW, m_sq);
      stpx<PX>(m + 2 * (size_t)a.HW, m_l);
      stpx_bytes<PX>(a.counted + o, cnt);
    }
  }
  block_add_i64<R * kScoreSums>(acc, a.sums + (size_t)n * kScoreRegions * kScoreSums);
}

template <int PX, bool SEG, bool MASK>
static void score_launch2(const ScoreArgs& a, dim3 grid, hipStream_t s) {
  if (a.maps)
    hipLaunchKernelGGL((depth_score_kernel<PX, SEG, MASK, true>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((depth_score_kernel<PX, SEG, MASK, false>), grid, dim3(256), 0, s, a);
}

template <int PX>
static void score_launch(const ScoreArgs& a, dim3 grid, hipStream_t s) {
  if (a.seg && a.mask)
    score_launch2<PX, true, true>(a, grid, s);
  else if (a.seg)
    score_launch2<PX, true, false>(a, grid, s);
  else if (a.mask)
    score_launch2<PX, false, true>(a, grid, s);
  else
    score_launch2<PX, false, false>(a, grid, s);
}

}  // namespace dvd

extern "C" {

int dvd_depth_score(const float* pred, const float* gt, const float* scale, const float* seg, const unsigned char* mask,
                    float g_min, int shift, long long* sums, float* maps, unsigned char* counted, int N, int H, int W,
                    dvd_stream_t stream) {
  using namespace dvd;
  DVD_REQUIRE(pred && gt && scale && sums, "depth_score: null pointer");
  DVD_REQUIRE((maps != nullptr) == (counted != nullptr), "depth_score: maps and counted go together (both or none)");
  DVD_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0, "depth_score: bad sizes N=%d H=%d W=%d", N, H, W);
  const long long HW = (long long)H * W;
  DVD_REQUIRE(HW < (1LL << 30) && (long long)N * HW < (1LL << 40), "depth_score: image too large N=%d H=%d W=%d", N, H, W);
  DVD_REQUIRE(g_min >= 0.0f && g_min <= FLT_MAX, "depth_score: g_min=%g must be finite and >= 0", (double)g_min);
  // N * H * W terms of at most 2^10 * 2^shift each can meet in one pooled sum: they must stay below 2^62
  DVD_REQUIRE(shift >= 1 && shift <= 32 && shift + kScoreCapLog2 + ceil_log2((long long)N * HW) <= 62,
              "depth_score: shift=%d outside 1 .. min(32, 62 - 10 - ceil_log2(N * H * W)) for N=%d H=%d W=%d", shift, N, H, W);
  DVD_REQUIRE(aligned_to(pred, 4) && aligned_to(gt, 4) && aligned_to(scale, 4) && aligned_to(seg, 4) &&
                  aligned_to(maps, 4) && aligned_to(sums, 8),
              "depth_score: misaligned pointer (floats: 4 bytes; sums: 8 bytes)");
  ScoreArgs a = {};
  a.pred = pred, a.gt = gt, a.scale = scale, a.seg = seg, a.mask = mask;
  a.sums = reinterpret_cast<unsigned long long*>(sums), a.maps = maps, a.counted = counted;
  a.HW = (int)HW, a.g_min = g_min, a.scale2 = (double)(1ULL << shift);
  bytes_add(DVD_BYTES_GEOMETRY, (double)N * HW * (8.0 + (seg ? 4.0 : 0.0) + (mask ? 1.0 : 0.0) + (maps ? 13.0 : 0.0)));
  const bool v4 = (W % 4 == 0) && aligned_to(pred, 16) && aligned_to(gt, 16) && aligned_to(seg, 16) &&
                  aligned_to(mask, 4) && aligned_to(maps, 16) && aligned_to(counted, 4);
  const int px = v4 ? 4 : 1;
  const long long strips = (HW + 256 * px - 1) / (256 * px);
  dim3 grid((unsigned)((strips + kScoreTrips - 1) / kScoreTrips), (unsigned)N);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (v4)
    score_launch<4>(a, grid, s);
  else
    score_launch<1>(a, grid, s);
  DVD_LAUNCH_OK();
  return DVD_OK;
}

}  // extern "C"
