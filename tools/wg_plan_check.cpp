// Host check of the weight-gradient work plan (dvd_hip/csrc/wg3_plan.h): for every decoder, encoder and stem shape of the
// headline step (48 images at 384x672) and for the shapes of tests/test_46_wgrad_live_steps_gpu.py it walks every slice of
// every launch exactly as the kernels do and checks that
//   * every (image, strip, row) is covered exactly once, by a launch whose K-step count is the strip's live count;
//   * the most expensive slice of a launch is within one row step of the launch's mean (cost = row steps x K steps);
//   * the partial slices the launches write are disjoint and inside what wg_partial_floats() sizes the workspace for;
//   * a slice walks a few segments only (each pays the warm-up rows once).
// The round-robin deal kept for A/B is walked too (cover only).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I dynamic-video-depth_amd/dvd_hip/csrc tools/wg_plan_check.cpp -o wg_plan_check
#include <algorithm>
#include <cstdio>
#include <vector>

#include "wg3_plan.h"

struct Launch {          // what a kernel reads of its arguments (Wg3Args)
  int N, H, strip0, ncols, S, deal, RS, nrseg;
};

static int g_fail = 0;
#define CHECK(c, ...)            \
  do {                           \
    if (!(c)) {                  \
      ++g_fail;                  \
      std::printf("  FAIL: ");   \
      std::printf(__VA_ARGS__);  \
      std::printf("\n");         \
    }                            \
  } while (0)

static void check_plan(const char* name, const dvd::Wg3Plan& p, int N, int H, int W, int taps, int Cout_total, int Cin, bool rowsum) {
  std::vector<int> seen((size_t)N * p.nstrips * H, 0);
  std::vector<int> slice_used(std::max(p.Stot, p.S), 0);
  int max_seg = 0;
  double worst = 0.0;
  for (int c = 0; c < p.ncls; ++c) {
    const dvd::WgClass& k = p.cls[c];
    const Launch a{N, H, k.strip0, k.ncols, k.S, 0, p.RS, p.nrseg};
    long long total = 0, mx = 0;
    int lseg = 0;
    for (int b = 0; b < k.S; ++b) {
      CHECK(k.slice0 + b < p.Stot, "%s: slice %d outside Stot %d", name, k.slice0 + b, p.Stot);
      if (k.slice0 + b < (int)slice_used.size()) ++slice_used[k.slice0 + b];
      int cur, end, segs = 0;
      long long cost = 0;
      dvd::wg_walk_begin(a, b, cur, end);
      while (cur < end) {
        int n, strip, r0, r1, next;
        dvd::wg_walk_segment(a, cur, end, n, strip, r0, r1, next);
        CHECK(n >= 0 && n < N && strip >= 0 && strip < p.nstrips && r0 >= 0 && r0 < r1 && r1 <= H && next > cur,
              "%s: bad segment n %d strip %d rows [%d, %d)", name, n, strip, r0, r1);
        if (!(n >= 0 && n < N && strip >= 0 && strip < p.nstrips && r0 >= 0 && r0 < r1 && r1 <= H && next > cur)) return;
        CHECK(dvd::wg_strip_steps(W, strip) == k.nk, "%s: strip %d has %d live K steps, its launch runs %d", name, strip,
              dvd::wg_strip_steps(W, strip), k.nk);
        for (int r = r0; r < r1; ++r) ++seen[((size_t)n * p.nstrips + strip) * H + r];
        cost += (long long)(r1 - r0) * k.nk;
        ++segs;
        cur = next;
      }
      total += cost;
      mx = std::max(mx, cost);
      lseg = std::max(lseg, segs);
    }
    const double mean = (double)total / k.S;
    worst = std::max(worst, (mx - mean) / k.nk);
    CHECK(mx - mean <= k.nk, "%s: launch %d: slowest slice %lld, mean %.2f K steps", name, c, mx, mean);
    const int q = N * k.ncols * H / k.S;
    CHECK(lseg <= (q + H - 1) / H + 2, "%s: launch %d: %d segments in a slice", name, c, lseg);
    max_seg = std::max(max_seg, lseg);
  }
  for (size_t i = 0; i < seen.size(); ++i)
    if (seen[i] != 1) {
      CHECK(false, "%s: row step %zu covered %d times", name, i, seen[i]);
      break;
    }
  for (int s = 0; s < p.Stot; ++s) CHECK(slice_used[s] == 1, "%s: partial slice %d written by %d launches", name, s, slice_used[s]);
  const size_t need = (size_t)p.Stot * taps * Cout_total * Cin + (rowsum ? (size_t)p.Stot * Cout_total : 0);
  CHECK(dvd::wg_partial_floats(p, taps, Cout_total, Cin, rowsum) >= need, "%s: workspace too small", name);
  // the deal: cover, and its slices inside the workspace
  std::fill(seen.begin(), seen.end(), 0);
  const Launch d{N, H, 0, p.nstrips, p.S, 1, p.RS, p.nrseg};
  long long dmx = 0, dtot = 0;
  for (int b = 0; b < p.S; ++b) {
    int cur, end;
    long long cost = 0;
    dvd::wg_walk_begin(d, b, cur, end);
    while (cur < end) {
      int n, strip, r0, r1, next;
      dvd::wg_walk_segment(d, cur, end, n, strip, r0, r1, next);
      for (int r = r0; r < r1; ++r) ++seen[((size_t)n * p.nstrips + strip) * H + r];
      cost += (long long)(r1 - r0) * 4;
      cur = next;
    }
    dmx = std::max(dmx, cost);
    dtot += cost;
  }
  for (size_t i = 0; i < seen.size(); ++i)
    if (seen[i] != 1) {
      CHECK(false, "%s: deal: row step %zu covered %d times", name, i, seen[i]);
      break;
    }
  CHECK(dvd::wg_partial_floats(p, taps, Cout_total, Cin, rowsum) >= (size_t)p.S * taps * Cout_total * Cin + (rowsum ? (size_t)p.S * Cout_total : 0),
        "%s: workspace too small for the deal", name);
  long long live = 0;
  for (int s = 0; s < p.nstrips; ++s) live += (long long)N * H * dvd::wg_strip_steps(W, s);
  std::printf("%-34s launches %d slices", name, p.ncls);
  for (int c = 0; c < p.ncls; ++c) std::printf(" %dx(NK %d)", p.cls[c].S, p.cls[c].nk);
  std::printf("  max segments %d  slowest - mean %.2f row steps | deal: %d slices, slowest / mean %.3f, K steps %lld -> %lld\n", max_seg,
              worst, p.S, (double)dmx * p.S / dtot, dtot, live);
}

int main() {
  struct Dense { int N, Cin, Cout, H, W, G; };
  const Dense dense[] = {
      // decoder (MiDaS refinement blocks and head) at 48 images
      {48, 256, 256, 96, 168, 1}, {48, 512, 256, 48, 84, 1}, {48, 256, 256, 48, 84, 1}, {48, 1024, 256, 24, 42, 1},
      {48, 256, 256, 24, 42, 1}, {48, 2048, 256, 12, 21, 1}, {48, 256, 256, 12, 21, 1}, {48, 256, 128, 192, 336, 1},
      {48, 128, 32, 384, 672, 1},
      // encoder: the grouped conv2 of ResNeXt stage 4 (64 per group: the dense kernel)
      {48, 2048, 2048, 12, 21, 32},
      // tests
      {1, 64, 64, 9, 5, 1}, {2, 64, 64, 12, 21, 1}, {3, 80, 72, 17, 42, 1}, {2, 64, 64, 24, 64, 1}, {2, 64, 64, 9, 70, 1},
      {3, 80, 72, 24, 84, 1}, {2, 64, 64, 13, 100, 1}, {1, 64, 64, 16, 168, 1}, {1, 64, 64, 1, 70, 1}, {1, 64, 64, 2, 130, 1},
  };
  char name[96];
  for (const Dense& s : dense) {
    dvd::Wg3Plan p;
    dvd::wg3_plan(s.N, s.Cin / s.G, s.Cout / s.G, s.H, s.W, s.G, p);
    std::snprintf(name, sizeof name, "3x3 %dx%d->%d g%d %dx%d", s.N, s.Cin, s.Cout, s.G, s.H, s.W);
    check_plan(name, p, s.N, s.H, s.W, 9, s.Cout, s.Cin / s.G, true);
  }
  const Dense grouped[] = {
      {48, 512, 512, 48, 84, 32}, {48, 1024, 1024, 24, 42, 32},                    // ResNeXt stages 2 and 3
      {2, 96, 96, 9, 70, 3}, {3, 64, 64, 24, 84, 4}, {1, 96, 96, 12, 21, 3}, {2, 64, 64, 17, 42, 4}, {1, 96, 96, 10, 5, 3},
      {2, 64, 64, 11, 100, 4}, {1, 96, 96, 16, 168, 3}, {2, 96, 96, 9, 64, 3},
  };
  for (const Dense& s : grouped) {
    dvd::Wg3Plan p;
    dvd::wg3g_plan(s.N, s.Cin / s.G, s.Cout / s.G, s.H, s.W, s.G, p);
    std::snprintf(name, sizeof name, "3x3g %dx%d->%d g%d %dx%d", s.N, s.Cin, s.Cout, s.G, s.H, s.W);
    check_plan(name, p, s.N, s.H, s.W, 9, s.Cout, s.Cin / s.G, true);
  }
  struct K { int N, Cin, Cout, H, W, KS; };
  const K ks[] = {{48, 12, 64, 192, 336, 5}, {2, 12, 40, 21, 37, 5}, {2, 12, 40, 24, 70, 5}, {2, 32, 32, 30, 70, 7}, {1, 32, 32, 50, 100, 11}};
  for (const K& s : ks) {
    dvd::Wg3Plan p;
    if (!dvd::wgk_plan(s.N, s.Cin, s.Cout, s.H, s.W, s.KS, false, p)) {
      ++g_fail;
      continue;
    }
    std::snprintf(name, sizeof name, "%dx%d %dx%d->%d %dx%d", s.KS, s.KS, s.N, s.Cin, s.Cout, s.H, s.W);
    check_plan(name, p, s.N, s.H, s.W, s.KS * s.KS, s.Cout, s.Cin, false);
  }
  std::printf(g_fail ? "%d checks FAILED\n" : "all checks passed\n", g_fail);
  return g_fail ? 1 : 0;
}
