// The work plan of the row-walking weight-gradient kernels of csrc/xwgrad3.hip (xwgrad3_kernel, xwgrad3g_kernel,
// xwgradk_kernel): a pure function of the shape, shared by the host (grids, workspace) and the kernels (which rows a slice
// walks).  Plain C++: a host program can include it (tools/wg_plan_check.cpp does, and checks cover, balance and workspace).
//
// Work.  An image is cut into column strips of 64 pixels; a ROW STEP is one image row of one strip; its cost is the number
// of 16-pixel K steps that hold pixels of the row: 4 for every strip but the last one, nkt = ceil((W - 64 (nstrips - 1)) / 16)
// for the last.  The number of K steps is a compile-time count of the kernels, so the strips of one cost form a CLASS with a
// launch of its own: the full strips (4 K steps) and, where nkt < 4, the last strip (nkt K steps).  Inside a class every row
// step costs the same; its U = N * ncols * H row steps are numbered u = (n * ncols + strip - strip0) * H + row and slice b of
// the class's S walks the contiguous run [b q + min(b, m), +q (+1 if b < m)) with q = U / S, m = U % S: every row step
// belongs to exactly one slice, the slices of a launch differ by at most one row step -- derived from b by arithmetic,
// nothing is uploaded.  A run crosses a strip's end every H row steps; each piece of a run (a SEGMENT: rows [r0, r1) of one
// strip of one image) pays the warm-up rows of the walk once, and a slice has at most ceil(q / H) + 2 of them.
// The launches of a layer write disjoint ranges of partial slices ([slice0, slice0 + S)); one reduction adds them in order.
// With two classes each launch is ONE round of blocks over the CUs (the launches run one behind the other, each balanced in
// itself); a single class keeps the slice count of the deal it replaces.
// That deal -- whole work items of RS rows of a strip, round robin over the slices, four K steps everywhere -- is kept for A/B
// (dvd_xwgrad_select(3)).
#pragma once
#include <cstddef>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DVD_PLAN_HD __host__ __device__
#else
#define DVD_PLAN_HD
#endif

namespace dvd {

constexpr int kW3Strip = 64;                  // pixels per row step
constexpr int kW3KPix = 16;                   // pixels per K step (v_mfma_f32_32x32x16_f16)
constexpr int kW3GPitch = 128 + 16;           // bytes per gy row in LDS (64 fp16 + pad: conflict-free 16-byte reads across rows)
constexpr int kW3XPitch = 160 + 16;           // bytes per x row in LDS (80 fp16 + pad)
constexpr int kW3CB = 64;                     // channels per block, both operands
constexpr int kW3LdsBytes = 2 * 2 * kW3CB * kW3GPitch + 2 * kW3CB * 4 * kW3XPitch;   // + 16 spare bytes (idle staging items)
constexpr int kWgCB = 32;
constexpr int kWgLdsBytes = 2 * 2 * kWgCB * kW3GPitch + 2 * kWgCB * 4 * kW3XPitch;    // 63 488

struct WgClass {
  int strip0, ncols;                          // the strips [strip0, strip0 + ncols) of every image
  int nk;                                     // live K steps of their row steps (1 .. 4)
  int S, slice0;                              // slices of the launch, the first partial slice it writes
};
struct Wg3Plan {
  int nstrips, RS, nrseg, S, nco, nci;        // S, RS, nrseg: the round-robin deal
  int nkt;                                    // K steps of a row step of the last strip (1 .. 4)
  int ncls, Stot;                             // launches by cost class, the partial slices they write in all
  WgClass cls[2];
  size_t lds;
};

DVD_PLAN_HD inline int wg_strips(int W) { return (W + kW3Strip - 1) / kW3Strip; }
// live K steps of strip `strip`
DVD_PLAN_HD inline int wg_strip_steps(int W, int strip) {
  const int w = W - strip * kW3Strip;
  return w >= kW3Strip ? kW3Strip / kW3KPix : (w + kW3KPix - 1) / kW3KPix;
}
// the row steps [u0, u1) of slice b of S over U row steps
DVD_PLAN_HD inline void wg_slice_units(int b, int S, int U, int& u0, int& u1) {
  const int q = U / S, m = U - q * S;
  u0 = b * q + (b < m ? b : m);
  u1 = u0 + q + (b < m ? 1 : 0);
}

// The segments of a slice, in walking order: `cur` runs from the slice's first row step (or work item) to `end`.
// A: the launch's parameters -- N, H, strip0, ncols, S and, for the round-robin deal of whole items (deal != 0), RS, nrseg.
template <class A>
DVD_PLAN_HD inline void wg_walk_begin(const A& a, int b, int& cur, int& end) {
  if (a.deal) {
    cur = b;
    end = a.N * a.ncols * a.nrseg;
  } else {
    wg_slice_units(b, a.S, a.N * a.ncols * a.H, cur, end);
  }
}
// the segment at `cur`: rows [r0, r1) of strip `strip` of image n; next: where the segment behind it starts
template <class A>
DVD_PLAN_HD inline void wg_walk_segment(const A& a, int cur, int end, int& n, int& strip, int& r0, int& r1, int& next) {
  if (a.deal) {
    n = cur / (a.ncols * a.nrseg);
    const int rem = cur - n * (a.ncols * a.nrseg);
    strip = rem / a.nrseg;
    r0 = (rem - strip * a.nrseg) * a.RS;
    r1 = (r0 + a.RS) < a.H ? (r0 + a.RS) : a.H;
    next = cur + a.S;
  } else {
    const int col = cur / a.H;
    n = col / a.ncols;
    strip = a.strip0 + col - n * a.ncols;
    r0 = cur - col * a.H;
    r1 = (end - cur) < (a.H - r0) ? r0 + (end - cur) : a.H;
    next = cur + r1 - r0;
  }
}

// ---- slices and work items per shape (Cin / Cout per group).  RS / nrseg: the items of the round-robin deal; they also fix S.
inline void wg_plan_items(int N, int H, int W, int pairs, int round_blocks, int S, int min_rs, Wg3Plan& p) {
  p.nstrips = wg_strips(W);
  p.nkt = wg_strip_steps(W, p.nstrips - 1);
  // rows per item: enough items to feed S slices evenly (>= 4 per slice), at least min_rs rows (warm-up rows per item)
  int RS = H;
  while (RS > min_rs && (long long)N * p.nstrips * ((H + RS - 1) / RS) < 4LL * S) RS = (RS + 1) / 2;
  p.RS = RS;
  p.nrseg = (H + RS - 1) / RS;
  const long long items = (long long)N * p.nstrips * p.nrseg;
  if (S > items) S = (int)items;
  p.S = S;
  // launches by cost class
  if (p.nstrips == 1 || p.nkt == 4) {
    p.ncls = 1;
    p.cls[0] = WgClass{0, p.nstrips, p.nkt, S, 0};
  } else {
    int Sc = round_blocks / pairs;                 // one round of blocks per launch
    if (Sc > N * H / min_rs) Sc = N * H / min_rs;  // (at least min_rs rows of the last strip per slice: the warm-up rows)
    if (Sc < 1) Sc = 1;
    p.ncls = 2;
    p.cls[0] = WgClass{0, p.nstrips - 1, 4, Sc, 0};
    p.cls[1] = WgClass{p.nstrips - 1, 1, p.nkt, Sc, Sc};
  }
  p.Stot = p.cls[p.ncls - 1].slice0 + p.cls[p.ncls - 1].S;
}
inline void wg3_plan(int N, int Cin, int Cout, int H, int W, int G, Wg3Plan& p) {
  p.nco = (Cout + kW3CB - 1) / kW3CB;
  p.nci = (Cin + kW3CB - 1) / kW3CB;
  const int pairs = p.nco * p.nci * G;
  // one block per CU is resident: a whole number of rounds over the 256 CUs, each block a few work items long
  wg_plan_items(N, H, W, pairs, 256, pairs >= 256 ? 1 : (512 + pairs - 1) / pairs, 8, p);
  p.lds = (size_t)kW3LdsBytes + 16;
}
// 32 x 32 channel blocks of three waves (xwgrad3g_kernel)
inline void wg3g_plan(int N, int Cin, int Cout, int H, int W, int G, Wg3Plan& p) {
  p.nco = (Cout + kWgCB - 1) / kWgCB;
  p.nci = (Cin + kWgCB - 1) / kWgCB;
  const int pairs = p.nco * p.nci * G;
  wg_plan_items(N, H, W, pairs, 512, pairs >= 512 ? 1 : (512 + pairs - 1) / pairs, 8, p);        // two blocks per CU are resident
  p.lds = (size_t)kWgLdsBytes;
}
// 5x5 / 7x7 / 11x11 (xwgradk_kernel)
inline bool wgk_plan(int N, int Cin, int Cout, int H, int W, int KS, bool h16, Wg3Plan& p) {
  if (KS != 5 && KS != 7 && KS != 11) return false;
  p.nco = (Cout + 31) / 32;
  p.nci = (Cin + 31) / 32;
  const int pairs = p.nco * p.nci;
  wg_plan_items(N, H, W, pairs, 256, pairs >= 256 ? 1 : (256 + pairs - 1) / pairs, 4 * KS, p);   // one block per CU; KS - 1 warm-up rows per item
  const int nterm = h16 ? 1 : 2;                               // fp16 operands: one term, half the LDS
  p.lds = (size_t)2 * nterm * 32 * kW3GPitch + (size_t)nterm * (KS + 1) * 32 * kW3XPitch;
  return true;
}
// floats of partial sums a layer's launches write: one [taps][Cout_total][Cin per group] block per slice (+ the RSUM row sums);
// the larger of the class launches' and the deal's (either may be selected when the launch comes)
inline size_t wg_partial_floats(const Wg3Plan& p, int taps, int Cout_total, int Cin_per_group, bool rowsum) {
  const int S = p.Stot > p.S ? p.Stot : p.S;
  return (size_t)S * taps * Cout_total * Cin_per_group + (rowsum ? (size_t)S * Cout_total : 0);
}

}  // namespace dvd
