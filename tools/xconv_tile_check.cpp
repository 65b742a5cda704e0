// Host check of the tile choice and the position -> LDS-cell mapping of the convolution kernels
// (dvd_hip/csrc/xconv_tile.h, used by csrc/xconv.hip).  For every launch below it builds the plan the host code builds and
// walks every position of every block the way xconv_kernel does, and checks that
//   * every output pixel of the image is owned by exactly one (block, position);
//   * every cell a position reads, plus the largest tap offset, is below the plane's cell count (npos);
//   * every cell the staging code writes is below the plane's spare cell (npos - 1);
//   * the LDS of the launch is within the budget of its block shape, and a launch keeps the blocks per CU and the staging
//     family (register prefetch, FI <= 3, or direct) it has with haloed positions (dvd_xconv_select(8));
//   * FI is what the tile needs and within its bound; the grid is within the launch limits;
//   * no launch has more blocks than with haloed positions; 1x1 launches have the identical tile.
// Launches: a tile depends on the per-group output channels only through the block shape (<= 32, <= 64, < 256, >= 256), on
// the input channels only through "multiple of 16 or not", and on the image only through H x W of one plane.  So the list is
// every block-shape class x kernel size {1, 3, 5, 7, 11} x every resolution of the depth networks' pyramids (768x1344 of
// BASELINE configs[4] and 384x672 of the headline step and the hourglass, halved down to 3x6), stride 1, stride-2 forward and
// its backward-data, fp32 and fp16 storage, under every dvd_xconv_select value -- a superset of the MiDaS, configs[4] and
// hourglass launches -- plus the shapes of tests/test_47_xconv_dense_positions_gpu.py and tests/test_06_xconv_gpu.py.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I dynamic-video-depth_amd/dvd_hip/csrc tools/xconv_tile_check.cpp -o xconv_tile_check
#include <algorithm>
#include <cstdio>
#include <vector>

#include "xconv_tile.h"

static int g_fail = 0;
static long long g_launches = 0, g_blocks = 0;
#define CHECK(c, ...)            \
  do {                           \
    if (!(c)) {                  \
      ++g_fail;                  \
      std::printf("  FAIL: ");   \
      std::printf(__VA_ARGS__);  \
      std::printf("\n");         \
    }                            \
  } while (0)

static int lds_tier(size_t lds) { return lds <= (size_t)dvd::kXLdsBudgetB1 ? 3 : (lds <= (size_t)dvd::kXLdsBudget ? 2 : 1); }

struct Shape {
  int Cin, Cout, H, W, KS, groups;      // channels PER GROUP; H x W: the full-resolution side
  bool s2;                              // stride-2 forward (its backward-data is a stride-1 plan on H x W)
};

// returns false where no tile exists (checked against the haloed plan by the caller)
static bool walk(const char* what, const Shape& s, bool in16, int sel, dvd::XPlan& p) {
  if (!dvd::xconv_plan(s.Cin, s.Cout, s.H, s.W, s.KS, s.s2, in16, sel, p)) return false;
  ++g_launches;
  const dvd::XCfg& c = p.c;
  const dvd::XTile& t = p.t;
  const int NQ = c.NQ(), NT = c.NT(), H = p.Hh, W = p.Ww, KS = s.KS, pad = KS / 2;
  char id[200];
  std::snprintf(id, sizeof id, "%s Cin %d Cout %d %dx%d k%d%s%s sel %d: %dx%d tile (P %d, PQ %d)", what, s.Cin, s.Cout, s.H, s.W, KS,
                s.s2 ? " s2" : "", in16 ? " fp16" : "", sel, t.TR, t.TC, t.P, t.PQ);
  CHECK(t.TR >= 1 && t.TC >= 1 && t.PQ >= t.TC && t.PQ <= t.P && (long long)t.TR * t.PQ <= NQ, "%s: %d x %d positions > %d", id,
        t.TR, t.PQ, NQ);
  CHECK(t.ntr == (H + t.TR - 1) / t.TR && t.ntc == (W + t.TC - 1) / t.TC, "%s: grid %d x %d", id, t.ntr, t.ntc);
  CHECK(t.P == (s.s2 ? t.TC + 1 : t.TC + 2 * pad), "%s: pitch", id);
  CHECK(t.NV == (s.s2 ? (2 * t.TR + 1) * (2 * t.TC + 1) : (t.TR + 2 * pad) * t.P), "%s: NV %d", id, t.NV);
  CHECK(t.FI == (2 * t.NV + NT - 1) / NT, "%s: FI %d", id, t.FI);
  CHECK(t.FI <= (s.s2 ? 4 * dvd::kXMaxFIDirect : dvd::kXMaxFIDirect), "%s: FI %d beyond the direct-staging bound", id, t.FI);
  CHECK(t.lds == dvd::xconv_lds(c, t.npos), "%s: lds", id);
  const size_t budget = c.NT() >= 512 ? dvd::kXLdsBudgetOne : (c.b1 && !s.s2 ? dvd::kXLdsBudgetB1 : dvd::kXLdsBudgetOne);
  CHECK(t.lds <= budget, "%s: %zu bytes of LDS > %zu", id, t.lds, budget);
  CHECK((long long)t.ntr * t.ntc <= 2147483647ll && (long long)p.mblocks * s.groups <= 65535, "%s: grid limits", id);
  // largest tap offset
  int maxtap = 0;
  for (int ky = 0; ky < KS; ++ky)
    for (int kx = 0; kx < KS; ++kx) maxtap = std::max(maxtap, dvd::xconv_tapoff(ky, kx, t.P, p.S2));
  // staged cells (locate() of the kernel): below the spare cell
  int maxstaged = 0;
  for (int q = 0; q < t.NV; ++q) {
    int lp = q;
    if (s.s2) {
      const int PI = 2 * t.TC + 1, rr = q / PI, cc = q - rr * PI;
      lp = ((rr & 1) * 2 + (cc & 1)) * p.S2 + (rr >> 1) * t.P + (cc >> 1);
    }
    maxstaged = std::max(maxstaged, lp);
  }
  CHECK(maxstaged < t.npos - 1, "%s: staged cell %d reaches the spare cell %d", id, maxstaged, t.npos - 1);
  // cells read: the same for every block
  for (int q = 0; q < NQ; ++q) {
    const int cell = sel == dvd::kXSelHalo || KS > 1 ? dvd::xconv_cell(q, t.PQ, t.P, t.TR) : q;      // (kOne: the cell is q)
    const int kone = KS == 1 ? q : cell;                                                              // both 1x1 code paths
    CHECK(cell >= 0 && cell + maxtap < t.npos && kone + maxtap < t.npos, "%s: position %d reads cell %d + %d >= %d", id, q,
          std::max(cell, kone), maxtap, t.npos);
    if (q / t.PQ < t.TR && q % t.PQ < t.TC && !s.s2)      // an output's taps stay inside the staged tile
      CHECK(cell + maxtap < t.NV, "%s: position %d reads cell %d + %d outside the staged tile of %d", id, q, cell, maxtap, t.NV);
  }
  // ownership
  std::vector<unsigned char> seen((size_t)H * W, 0);
  for (int b = 0; b < t.ntr * t.ntc; ++b) {
    ++g_blocks;
    const int tr = b / t.ntc, tc = b - tr * t.ntc, r0 = tr * t.TR, c0 = tc * t.TC;
    const int TRv = std::min(H - r0, t.TR), TCv = std::min(W - c0, t.TC);
    CHECK(TRv >= 1 && TCv >= 1, "%s: empty block %d", id, b);
    for (int q = 0; q < NQ; ++q) {
      const int rr = q / t.PQ, cc = q - rr * t.PQ;
      if (rr < TRv && cc < TCv) {
        unsigned char& n = seen[(size_t)(r0 + rr) * W + c0 + cc];
        if (n < 255) ++n;
      }
    }
  }
  long long bad = 0;
  for (unsigned char n : seen) bad += n != 1;
  CHECK(bad == 0, "%s: %lld of %d x %d outputs not owned exactly once", id, bad, H, W);
  return true;
}

static void check_shape(const char* what, const Shape& s) {
  for (int in16 = 0; in16 <= 1; ++in16) {
    if (in16 && s.Cin % 16) continue;                      // fp16 storage needs whole chunks
    dvd::XPlan halo;
    const bool has_halo = walk(what, s, in16 != 0, dvd::kXSelHalo, halo);
    for (int sel = 0; sel < dvd::kXSelHalo; ++sel) {
      if (s.s2 && (sel == 4 || s.Cin % 16)) continue;     // the strided forms exist on the buffer-addressed loop only
      if (in16 && sel == 4) continue;
      // the haloed plan of the same block shape: sel 1-7 force shapes, so compare with the haloed TILE of that shape
      dvd::XPlan p;
      const bool ok = walk(what, s, in16 != 0, sel, p);
      dvd::XTile h;
      int S2h = 0;
      const bool hok = s.s2 ? dvd::pick_tile_s2(p.Hh, p.Ww, p.c, h, S2h, true) : dvd::pick_tile(p.Hh, p.Ww, s.KS, p.c, h, true);
      CHECK(ok == hok, "%s Cin %d Cout %d %dx%d k%d sel %d: dense plan %d, haloed plan %d", what, s.Cin, s.Cout, s.H, s.W, s.KS,
            sel, (int)ok, (int)hok);
      if (!ok || !hok) continue;
      const dvd::XTile& t = p.t;
      char id[200];
      std::snprintf(id, sizeof id, "%s Cin %d Cout %d %dx%d k%d%s%s sel %d", what, s.Cin, s.Cout, s.H, s.W, s.KS, s.s2 ? " s2" : "",
                    in16 ? " fp16" : "", sel);
      CHECK(t.ntr * t.ntc <= h.ntr * h.ntc, "%s: %d blocks, haloed %d", id, t.ntr * t.ntc, h.ntr * h.ntc);
      CHECK(lds_tier(t.lds) >= std::min(lds_tier(h.lds), p.c.NT() >= 512 ? 1 : (p.c.b1 ? 3 : 2)),
            "%s: %zu bytes of LDS drop a block per CU (haloed %zu)", id, t.lds, h.lds);
      if (!s.s2) CHECK((t.FI <= dvd::kXMaxFI) == (h.FI <= dvd::kXMaxFI), "%s: FI %d, haloed %d: another staging family", id, t.FI, h.FI);
      if (s.KS == 1)
        CHECK(t.TR == h.TR && t.TC == h.TC && t.P == h.P && t.PQ == h.PQ && t.ntr == h.ntr && t.ntc == h.ntc && t.NV == h.NV &&
                  t.npos == h.npos && t.FI == h.FI && t.lds == h.lds, "%s: the 1x1 tile changed", id);
    }
    (void)has_halo;
  }
}

static void eff_row(const char* name, int Cin, int Cout, int H, int W, int KS) {
  dvd::XPlan a, b;
  if (!dvd::xconv_plan(Cin, Cout, H, W, KS, false, false, dvd::kXSelHalo, a) || !dvd::xconv_plan(Cin, Cout, H, W, KS, false, false, 0, b))
    return;
  const double ea = (double)H * W / ((double)a.t.ntr * a.t.ntc * a.c.NQ()), eb = (double)H * W / ((double)b.t.ntr * b.t.ntc * b.c.NQ());
  std::printf("| %-44s | %3dx%-3d %.3f | %3dx%-3d %.3f | %5d / %5d = %.3f |\n", name, a.t.TR, a.t.TC, ea, b.t.TR, b.t.TC, eb,
              b.t.ntr * b.t.ntc, a.t.ntr * a.t.ntc, (double)(b.t.ntr * b.t.ntc) / (a.t.ntr * a.t.ntc));
}

int main() {
  // ---- the sweep
  const int chan[] = {16, 32, 64, 128, 256, 272};          // per group: every block-shape class, one ragged
  const int cins[] = {16, 20};                             // buffer-addressed and generic main loop
  for (int top = 0; top < 2; ++top) {
    int H = top ? 384 : 768, W = top ? 672 : 1344;
    for (; H >= 3; H = (H + 1) / 2, W = (W + 1) / 2)
      for (int KS : {1, 3, 5, 7, 11})
        for (int M : chan)
          for (int Cin : cins) {
            if ((long long)H * W * std::max(M, Cin) >= (1ll << 31)) continue;
            check_shape("sweep", Shape{Cin, M, H, W, KS, 1, false});
            if (KS == 3 && Cin % 16 == 0) check_shape("sweep", Shape{Cin, M, H, W, 3, 32, true});
          }
  }
  // ---- the shapes of the tests (forward and backward-data: the channel counts swap roles)
  const int tests[][7] = {   // Cin, Cout (per group), H, W, KS, groups, stride
      {32, 32, 5, 7, 3, 1, 1},     {32, 32, 16, 16, 3, 1, 1},  {256, 256, 12, 21, 3, 1, 1}, {256, 256, 13, 45, 3, 1, 1},
      {272, 288, 9, 14, 3, 1, 1},  {256, 128, 20, 36, 3, 1, 1}, {32, 32, 1, 40, 3, 1, 1},    {32, 32, 40, 1, 3, 1, 1},
      {16, 64, 12, 20, 5, 1, 1},   {32, 32, 9, 12, 11, 1, 1},  {64, 256, 11, 17, 5, 1, 1},  {32, 32, 9, 23, 3, 2, 1},
      {64, 64, 7, 10, 3, 2, 1},    {32, 32, 10, 14, 3, 2, 2},  {32, 32, 11, 15, 3, 2, 2},   {64, 256, 6, 10, 1, 1, 1},
      // tests/test_06_xconv_gpu.py
      {256, 256, 24, 42, 3, 1, 1}, {256, 256, 48, 84, 3, 1, 1}, {1024, 256, 12, 21, 3, 1, 1}, {128, 32, 30, 70, 3, 1, 1},
      {20, 40, 11, 19, 3, 1, 1},   {48, 64, 19, 23, 5, 1, 1},  {32, 32, 21, 33, 7, 1, 1},   {32, 32, 24, 40, 11, 1, 1},
      {3, 64, 16, 24, 7, 1, 1},    {256, 512, 10, 15, 3, 1, 1}, {256, 64, 10, 13, 7, 1, 1},  {256, 32, 9, 12, 11, 1, 1},
      {16, 256, 7, 9, 3, 1, 1},
      // the ResNeXt stem: its forward stays on haloed positions (xconv_keeps_halo_positions), its backward-data does not
      {12, 64, 192, 336, 5, 1, 1}};
  for (const auto& r : tests) {
    check_shape("test fwd", Shape{r[0], r[1], r[2], r[3], r[4], r[5], r[6] == 2});
    check_shape("test bwd", Shape{r[1], r[0], r[2], r[3], r[4], r[5], false});
  }
  // ---- the headline step's k >= 3 layers (48 images at 384x672), haloed and dense positions
  std::printf("| layer | haloed: TR x TC, eff | dense: TR x TC, eff | blocks dense / haloed |\n|---|---|---|---|\n");
  eff_row("256->256 at 96x168", 256, 256, 96, 168, 3);
  eff_row("128->256 at 192x336 (backward-data)", 128, 256, 192, 336, 3);
  eff_row("256->256 at 48x84", 256, 256, 48, 84, 3);
  eff_row("256->256 at 24x42", 256, 256, 24, 42, 3);
  eff_row("256->256 at 12x21", 256, 256, 12, 21, 3);
  eff_row("256->128 at 192x336", 256, 128, 192, 336, 3);
  eff_row("128->32 at 384x672", 128, 32, 384, 672, 3);
  eff_row("32->128 at 384x672 (backward-data)", 32, 128, 384, 672, 3);
  eff_row("grouped, 32 per group, 24x42", 32, 32, 24, 42, 3);
  eff_row("grouped pairs (32 per group), 48x84", 32, 32, 48, 84, 3);
  eff_row("grouped, 64 per group, 12x21", 64, 64, 12, 21, 3);
  eff_row("stem, 5x5 at 192x336 (12->64)", 12, 64, 192, 336, 5);
  eff_row("stem backward-data, 5x5 (64->12)", 64, 12, 192, 336, 5);
  std::printf("%lld launches, %lld blocks walked\n", g_launches, g_blocks);
  if (g_fail) {
    std::printf("%d checks FAILED\n", g_fail);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
