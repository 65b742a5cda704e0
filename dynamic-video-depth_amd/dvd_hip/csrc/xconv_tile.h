// Block shape and image tile of the implicit-GEMM convolution kernels of csrc/xconv.hip: pure functions of the shape, shared
// by the host code (grid, LDS, kernel arguments) and the kernel (which LDS cell a GEMM column reads).  Plain C++: a host
// program can include it (tools/xconv_tile_check.cpp does, and checks cover, LDS bounds and budgets block by block).
//
// Positions and cells.  A block computes NQ = TN * WN * 32 GEMM columns ("positions") and stages the haloed tile of its
// TR x TC outputs as (TR + 2 pad) rows of P = TC + 2 pad LDS cells (stride 2: four phase planes of (TR + 1) rows of
// P = TC + 1 cells).  Position q is the output (q / PQ, q % PQ) of the tile and reads, for tap (ky, kx), the cell
// (q / PQ) * P + q % PQ + tapoff(ky, kx):
//   * dense positions (PQ = TC): every position below TR * TC is an output, so a tile needs TR * TC <= NQ;
//   * haloed positions (PQ = P; rounds 2-6, kept for A/B as dvd_xconv_select(8) and for the 1x1 kernels, where pad = 0
//     makes the two the same thing): positions are the cells themselves, TR * P <= NQ, and the 2 pad halo columns of
//     every tile row are computed and dropped -- 8-50 % of a launch's MFMAs on the shapes of the depth networks.
// Positions at or beyond TR * PQ read cell 0 and are never stored.
#pragma once
#include <cstddef>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DVD_XTILE_HD __host__ __device__
#else
#define DVD_XTILE_HD
#endif

namespace dvd {

// LDS cell (relative to the tile's origin, tap offset not included) that position q reads
DVD_XTILE_HD inline int xconv_cell(int q, int PQ, int P, int TR) {
  const int rr = q / PQ;
  return rr < TR ? rr * P + (q - rr * PQ) : 0;
}
// LDS offset of tap (ky, kx); S2 > 0: the phase planes of the stride-2 forward
DVD_XTILE_HD inline int xconv_tapoff(int ky, int kx, int P, int S2) {
  return S2 ? ((ky & 1) * 2 + (kx & 1)) * S2 + (ky >> 1) * P + (kx >> 1) : ky * P + kx;
}

struct XCfg {
  int TM, TN, WM, WN;
  bool b1 = false;        // single activation stage, three blocks per CU
  bool in16 = false;      // fp16 activations: one split term in LDS
  int blockM() const { return TM * WM * 32; }
  int NQ() const { return TN * WN * 32; }
  int NT() const { return 64 * WM * WN; }
};
// Block shapes.  Every activation element a block stages is split into its two fp16 terms ONCE per block (VALU work) and
// read from LDS once per 32-channel tile row, so the split / LDS cost per MFMA falls with the number of output channels a
// block owns: with >= 256 of them a block takes 256 channels (wave tile 128 channels x 64 positions: 48 MFMAs against 18
// fragment reads per K step, round 2: 24 against 12) -- 256 x 128 positions at two blocks per CU for 1x1 kernels, 256 x 256
// positions in ONE 512-thread block per CU for k >= 3.
// sel: the test / A-B hook (dvd_xconv_select): 0 auto, 1 round-2 shapes only, 2 force 256x128, 3 force 256x256, 4 round-2
// shapes on the generic (pointer-addressed) main loop, 5 128 x 128 blocks with one activation stage at three blocks per CU,
// 6 1x1 kernels without the two-chunk loop (kOne), 7 kOne with the narrow epilogue, 8 automatic shapes on haloed positions
// with the tile choice of rounds 2-6
constexpr int kXSelHalo = 8;
inline XCfg pick_cfg(int M, int KS, int sel) {
  if (M <= 32) return {1, 2, 1, 4};     // 32 channels x 256 positions
  if (M <= 64) return {2, 2, 1, 4};     // 64 x 256
  if (M > 64 && sel == 5) return {2, 2, 2, 2, true};
  if (M >= 256 && sel != 1 && sel != 4) {
    if (sel == 2) return {4, 2, 2, 2};
    if (sel == 3) return {4, 2, 2, 4};
    return KS == 1 ? XCfg{4, 2, 2, 2} : XCfg{4, 2, 2, 4};
  }
  return {2, 2, 2, 2};                  // 128 x 128
}
constexpr int kXLdsBudget = 78 * 1024;    // two blocks per CU
constexpr int kXLdsBudgetOne = 156 * 1024;
constexpr int kXLdsBudgetB1 = 52 * 1024;  // three blocks per CU
constexpr int kXMaxFI = 3;       // register-prefetched staging; larger halos use the direct-staging kernels
constexpr int kXMaxFIDirect = 16;

struct XTile {
  int TR, TC, P, PQ, ntr, ntc, NV, npos, FI;
  size_t lds;
};
inline size_t xconv_lds(const XCfg& c, int npos) {
  const int AU = c.WM * c.TM * 128, NT = c.NT();
  const int AS = (AU + NT - 1) / NT * NT;
  return ((size_t)2 * AS + (size_t)(c.b1 ? 4 : 8) * npos / (c.in16 ? 2 : 1)) * 16;
}
// Haloed positions: TR x TC outputs, TR * (TC + 2 pad) <= NQ positions; choose the split of the width that wastes the
// fewest positions, subject to the LDS budget and the staging-iteration bound.
inline bool pick_tile_halo_budget(int H, int W, int KS, const XCfg& c, XTile& best, int budget) {
  const int pad = KS / 2, NQ = c.NQ(), NT = c.NT();
  double best_eff = -1.0;
  for (int nct = 1; nct <= W; ++nct) {
    int TC = (W + nct - 1) / nct;
    if (KS == 1) TC = (TC + 7) & ~7;                     // whole 16-byte runs per lane in the wide epilogue of the 1x1 kernels
    const int P = TC + 2 * pad;
    if (P > NQ) continue;
    const int ntc = (W + TC - 1) / TC;
    const int npos = NQ + (KS - 1) * (P + 1) + 1;        // + the spare cell of the staging code
    if (xconv_lds(c, npos) > (size_t)budget) continue;
    int trmax = NQ / P;
    if (trmax > H) trmax = H;
    for (int tr0 = trmax; tr0 >= 1; --tr0) {
      const int ntr = (H + tr0 - 1) / tr0;
      const int TR = (H + ntr - 1) / ntr;               // even out the rows
      const int NV = (TR + 2 * pad) * P;
      const int FI = (2 * NV + NT - 1) / NT;
      if (FI > kXMaxFIDirect) continue;
      // useful positions per computed position, minus what the halo costs in staging work
      const double eff = (double)H * W / ((double)ntr * ntc * NQ) - 0.02 * (double)NV / (TR * TC) - 1e-6 * nct;
      if (eff > best_eff) {
        best_eff = eff;
        best = {TR, TC, P, P, ntr, ntc, NV, npos, FI, xconv_lds(c, npos)};
      }
      break;                                             // smaller TR only lowers the efficiency
    }
    if (TC <= 8) break;
  }
  return best_eff > -1.0;
}
// Dense positions (k >= 3): TR * TC <= NQ, and a plane of the stage holds the haloed tile and the staging code's spare cell
// (the largest cell a live position reads is (TR - 1) P + TC - 1 + (KS - 1)(P + 1) = NV - 1).  Same score as above (the
// halo still costs staging work).  The epilogue stores runs of TC outputs, and at equal positions per block the score
// prefers square tiles (fewest halo cells) however narrow: where a tile at least 32 outputs wide (a full 128-byte line per
// run) scores within kXWideSlack of the best one, the best such tile is taken.  fi_min, fi_max: see pick_tile.
constexpr double kXWideSlack = 0.02;
constexpr int kXWideTC = 32;
inline bool pick_tile_dense_budget(int H, int W, int KS, const XCfg& c, XTile& best, int budget, int fi_min, int fi_max) {
  const int pad = KS / 2, NQ = c.NQ(), NT = c.NT();
  double best_eff = -1.0, wide_eff = -1.0;
  XTile wide{};
  for (int nct = 1; nct <= W; ++nct) {
    const int TC = (W + nct - 1) / nct;
    if (TC > NQ) continue;
    const int P = TC + 2 * pad;
    const int ntc = (W + TC - 1) / TC;
    int trmax = NQ / TC;
    if (trmax > H) trmax = H;
    for (int tr0 = trmax; tr0 >= 1; --tr0) {
      const int ntr = (H + tr0 - 1) / tr0;
      const int TR = (H + ntr - 1) / ntr;               // even out the rows
      const int NV = (TR + 2 * pad) * P;
      const int npos = NV + 1;
      const int FI = (2 * NV + NT - 1) / NT;
      if (FI > fi_max || xconv_lds(c, npos) > (size_t)budget) continue;      // (a lower tile may fit)
      if (FI < fi_min) break;
      const double eff = (double)H * W / ((double)ntr * ntc * NQ) - 0.02 * (double)NV / (TR * TC) - 1e-6 * nct;
      const XTile t = {TR, TC, P, TC, ntr, ntc, NV, npos, FI, xconv_lds(c, npos)};
      if (eff > best_eff) {
        best_eff = eff;
        best = t;
      }
      if (TC >= kXWideTC && eff > wide_eff) {
        wide_eff = eff;
        wide = t;
      }
      break;
    }
    if (TC <= 8) break;
  }
  if (wide_eff > -1.0 && wide_eff >= best_eff - kXWideSlack) best = wide;
  return best_eff > -1.0;
}

// Launches that stay on haloed positions because dense positions timed slower on them (profiles/xconv_dense_positions_ab.json):
// the forward of the ResNeXt stem alone, 12 -> 64 channels, 5x5 at 192x336 on the generic main loop -- 0.720 ms per 48 images
// on haloed positions (8x28), 0.742 with the same tile and 0.737 with 12x20 on dense positions, against 0.004 between its
// haloed runs.  One chunk of channels under 25 taps on 64-channel blocks has the fewest MFMAs per fragment read of all
// launches, so the seam of the dense rows (cells 2 pad = 4 further on, a 2-way bank conflict) is the likely cost; counters
// were not taken.  Nothing else matches: the predicate names the layer, and fp16 storage needs whole 16-channel chunks.
inline bool xconv_keeps_halo_positions(int Cin, int Cout, int H, int W, int KS, bool s2) {
  return KS == 5 && H == 192 && W == 336 && Cin == 12 && Cout == 64 && !s2;
}

// halo: the tile choice and position mapping of rounds 2-6 (dvd_xconv_select(8); always for 1x1 kernels, whose tile and
// LDS layout are the same under both).  The dense choice is made inside the LDS tier (blocks per CU) and the staging family
// (register prefetch, FI <= kXMaxFI, or direct) the haloed choice lands in, so a stride-1 shape never changes its kernel
// or its occupancy (the stride-2 forward keeps its LDS tier only, see pick_tile_s2); the haloed tile itself is legal under
// the dense mapping and is what a shape falls back to.
inline bool pick_tile(int H, int W, int KS, const XCfg& c, XTile& best, bool halo) {
  // two blocks per CU where the haloed tile allows it, one block (big kernels: k >= 7; the 512-thread shape) otherwise
  int budgets[2] = {kXLdsBudget, kXLdsBudgetOne};
  int nb = 2;
  if (c.NT() >= 512) { budgets[0] = kXLdsBudgetOne; nb = 1; }
  else if (c.b1) { budgets[0] = kXLdsBudgetB1; nb = 1; }      // three blocks per CU, or not this shape
  for (int i = 0; i < nb; ++i) {
    XTile h;
    if (!pick_tile_halo_budget(H, W, KS, c, h, budgets[i])) continue;
    best = h;
    if (halo || KS == 1) return true;
    const XTile same = {h.TR, h.TC, h.P, h.TC, h.ntr, h.ntc, h.NV, h.NV + 1, h.FI, xconv_lds(c, h.NV + 1)};
    XTile d;
    if (!pick_tile_dense_budget(H, W, KS, c, d, budgets[i], h.FI <= kXMaxFI ? 1 : kXMaxFI + 1,
                                h.FI <= kXMaxFI ? kXMaxFI : kXMaxFIDirect) ||
        d.ntr * d.ntc > h.ntr * h.ntc)
      d = same;
    best = d;
    return true;
  }
  return false;
}

// Stride-2 forward (XArgs::S2): TR x TC OUTPUTS per block in a pitch of P = TC + 1, four phase planes of (TR + 1) * P cells.
// Haloed positions: TR * P <= NQ, and the last phase plane is read up to position NQ - 1: 3 planes + NQ + the spare cell.
// Dense positions: TR * TC <= NQ, and the last plane is staged and read below cell TR * P: 3 planes + TR * P + the spare cell.
// The dense choice is held to the haloed tile's LDS tier (blocks per CU) and block count, not to its staging-iteration
// count: a shape may move between the register-prefetch instantiations (FI <= kXMaxFI) and the direct one.  Both stage the
// same cells and run the same K order, so results do not change.
inline bool pick_tile_s2_budget(int Ho, int Wo, const XCfg& c, XTile& best, int& S2, int budget, bool halo) {
  const int NQ = c.NQ(), NT = c.NT();
  double best_eff = -1.0;
  for (int nct = 1; nct <= Wo; ++nct) {
    const int TC = (Wo + nct - 1) / nct, P = TC + 1, PQ = halo ? P : TC;
    if (PQ > NQ) continue;
    const int ntc = (Wo + TC - 1) / TC;
    int trmax = NQ / PQ;
    if (trmax > Ho) trmax = Ho;
    const int ntr = (Ho + trmax - 1) / trmax;
    const int TR = (Ho + ntr - 1) / ntr;
    const int s2 = (TR + 1) * P;
    const int npos = 3 * s2 + (halo ? NQ : TR * P) + 1;
    const int NV = (2 * TR + 1) * (2 * TC + 1);
    const int FI = (2 * NV + NT - 1) / NT;
    if (xconv_lds(c, npos) <= (size_t)budget && FI <= 4 * kXMaxFIDirect) {
      const double eff = (double)Ho * Wo / ((double)ntr * ntc * NQ) - 1e-6 * nct;
      if (eff > best_eff) {
        best_eff = eff;
        best = {TR, TC, P, PQ, ntr, ntc, NV, npos, FI, xconv_lds(c, npos)};
        S2 = s2;
      }
    }
    if (TC <= 4) break;
  }
  return best_eff > -1.0;
}
inline bool pick_tile_s2(int Ho, int Wo, const XCfg& c, XTile& best, int& S2, bool halo) {
  const int budgets[2] = {kXLdsBudget, kXLdsBudgetOne};
  for (int budget : budgets) {
    XTile h;
    int sh = 0;
    if (!pick_tile_s2_budget(Ho, Wo, c, h, sh, budget, true)) continue;
    best = h;
    S2 = sh;
    if (halo) return true;
    XTile d;
    int sd = 0;
    // (inside the haloed tile's LDS tier: these kernels run three blocks per CU where the tile allows it)
    const int tier = h.lds <= (size_t)kXLdsBudgetB1 ? kXLdsBudgetB1 : budget;
    if (pick_tile_s2_budget(Ho, Wo, c, d, sd, tier, false) && d.ntr * d.ntc <= h.ntr * h.ntc) {
      best = d;
      S2 = sd;
    } else {                                             // the haloed tile on dense positions
      best.PQ = h.TC;
      best.npos = 3 * sh + h.TR * h.P + 1;
      best.lds = xconv_lds(c, best.npos);
    }
    return true;
  }
  return false;
}

// What a launch of dvd_xconv_fwd[_h] runs: block shape, tile, grid.  Cin / Cout are PER GROUP; H x W the full-resolution
// side (the input of a stride-2 forward, the output otherwise); sel the dvd_xconv_select value.
struct XPlan {
  XCfg c;
  XTile t;
  int S2;                 // cells per phase plane (stride-2 forward), else 0
  int Hh, Ww;             // the output plane the tiles cut (1x1: one row of H * W)
  bool fast;
  int mblocks;
};
inline bool xconv_plan(int Cin, int Cout, int H, int W, int KS, bool s2, bool in16, int sel, XPlan& p) {
  // buffer-addressed main loop: whole 16-channel chunks, 31-bit byte offsets inside one image's input channels and
  // inside the packed weights of one block row
  p.fast = (Cin % 16 == 0) && ((long long)Cin * H * W * 4 < (1ll << 31)) &&
           ((long long)8 * ((Cin + 15) / 16) * KS * KS * 2048 < (1ll << 31)) && sel != 4;
  // (stride 2: four input cells per output -- blocks of at most 128 channels, fp32 activations on ONE activation stage)
  p.c = pick_cfg((p.fast && !s2) ? Cout : (Cout < 128 ? Cout : 128), KS, sel);
  if (!p.fast) p.c.b1 = false;   // the wide shapes exist as FAST kernels only
  if (s2) p.c.b1 = true;
  if (in16) p.c.b1 = false;
  p.c.in16 = in16;
  p.Hh = H;
  p.Ww = W;
  if (KS == 1) {           // no spatial structure: one row of H * W positions
    p.Hh = 1;
    p.Ww = H * W;
  }
  p.S2 = 0;
  const bool halo = sel == kXSelHalo || xconv_keeps_halo_positions(Cin, Cout, H, W, KS, s2);
  bool ok;
  if (s2) {
    p.Hh = (H + 1) / 2;
    p.Ww = (W + 1) / 2;
    ok = pick_tile_s2(p.Hh, p.Ww, p.c, p.t, p.S2, halo);
  } else {
    if (p.c.b1 && !pick_tile(p.Hh, p.Ww, KS, p.c, p.t, halo)) p.c.b1 = false;     // (large kernels: the haloed tile needs more LDS)
    ok = pick_tile(p.Hh, p.Ww, KS, p.c, p.t, halo);
  }
  p.mblocks = (Cout + p.c.blockM() - 1) / p.c.blockM();
  return ok;
}

}  // namespace dvd
