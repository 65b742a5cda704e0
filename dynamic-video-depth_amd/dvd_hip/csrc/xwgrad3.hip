// Backward-weight of the dense 3x3 stride-1 "same" convolutions on the 16-bit matrix cores with fp32-class
// accuracy (the two-term fp16 split of csrc/dvd_split.h: both operands scaled by a power of two from their tensors'
// max|.| scalars, three partial products per fp32 product, fp32 accumulation), deterministic (no atomics):
//   dW[co][ci][ky][kx] = sum_{n, r, c} gy[n][co][r][c] * act(x)[n][ci][r + ky - 1][c + kx - 1]
//
// What it replaces (reference, /root/reference): the autograd weight gradient of the 3x3 nn.Conv2d of the MiDaS
// decoder (third_party/midas_blocks.py:102-168, MiDaS.py:186-195); MIOpen's igemm_wrw (atomics, 113 TF/s) and the
// exact-fp32 kernel of csrc/xwgrad.hip (86 TF/s: the fp32 MFMA rate is the ceiling there).
//
// Mapping.  GEMM M = output channel, N = input channel, K = pixels.  v_mfma_f32_32x32x16_f16: lane l holds
// A[co = l&31][8 consecutive pixels, run (l>>5)] = gy and B[the same 8 pixels shifted by the tap][ci = l&31] = x.
// Pixels are contiguous in NCHW, so both operands are read as 16-byte runs along x; the run of tap kx = 1 is a
// cell of the LDS row, the runs of kx = 0 / 2 start one pixel earlier / later and are assembled from the cell and
// one dword of its neighbour with v_alignbit_b32 (five of them give both shifted fragments of a term).
// A block owns 64 output x 64 input channels and walks DOWN a 64-pixel-wide column strip of an image, one row
// per step: the gy row (64 channels x 64 pixels) and ONE new x row (64 channels x 80 pixels: the strip, one
// 8-pixel cell left and right) are staged per step -- the x rows a step needs live in a rolling buffer of four --
// scaled and split into the two fp16 terms on the way in; the next step's rows are requested before the MFMAs of the
// current one.  Wave (pm, pn, ky) of the 12 keeps the three accumulators of kernel row ky for its 32 x 32 pair.
// Every block writes its partial sums; xwgrad3_reduce_kernel adds them in slice order.
// Round 4: the row step exists in two instantiations -- FW (buffer loads, no branch, the staging of item i
// between the MFMAs of K step i; taken whenever rows start dword-aligned) and the round-3 one (per-element guarded loads ahead
// of the MFMAs; what is left for it: fp16 rows of odd width); xwgrad3g_kernel is the same walk on 32 x 32 channel blocks of
// three waves for grouped layers with at most 32 channels per group; xwgrad1b_kernel (1x1, wide layers) has an FW form too.
//
// Five kernel families live here: xwgrad3_kernel (3x3, 64 x 64 channel blocks), xwgrad3g_kernel (3x3 grouped, 32 x 32),
// xwgradk_kernel (5x5 / 7x7 / 11x11) -- the three that walk down column strips by the plan of wg3_plan.h -- and the 1x1 pair
// xwgrad1s_kernel (128 x 128 blocks) and xwgrad1b_kernel (256 x 256, wide layers).  All write per-slice partials that
// xwgrad3_reduce_kernel adds.  Which family and instantiation serves a shape, with which launches and how much workspace, is
// decided in ONE place, wg_route() in the host section at the end: the size queries, dvd_xwgrad_rowsum_in_kernel and the launch
// path of every entry point read its answer.  A new route belongs there and nowhere else.
#include <type_traits>

#include "dvd_split.h"
#include "wg3_plan.h"

namespace dvd {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2v __attribute__((ext_vector_type(2)));

static int g_w1_variant = 0;      // test / A-B hook (dvd_xwgrad_select): 0 auto, 1 always the 128 x 128 blocks
static int g_w3_variant = 0;      // 1 (hook value 2): the 3x3 kernel's round-3 row step (staging ahead of the MFMAs) on every shape
static int g_w3_deal = 0;         // 1 (hook value 3): four K steps per row step and the round-robin deal of whole items (wg3_plan.h)

struct Wg3Args {
  const void* __restrict__ x;         // float, or _Float16 in the H16 kernels (fp16 activation storage, BASELINE configs[4])
  const void* __restrict__ gy;
  const float* __restrict__ x_amax;   // device scalars: max|x|, max|gy| (or upper bounds) of the whole tensors (fp32 kernels)
  const float* __restrict__ g_amax;
  const float* __restrict__ out_scale;  // H16: device scalar the result is multiplied by (1 / loss scale of the fp16 gradients), or null
  float* __restrict__ partial;   // [S][9][Cout][Cin]
  // RSUM kernels (fp32 xwgrad1b FW / xwgrad3g): [S][G * Cout] per-slice sums of the gy rows the block stages, or null
  float* __restrict__ rowsum_partial = nullptr;
  int N, Cin, Cout, H, W;        // Cin / Cout per group
  int G, nco;                    // groups, output-channel blocks per group
  int nstrips, RS, nrseg, S;     // column strips per image, rows per work item, row segments per image, slices
  int strip0, ncols;             // this launch walks the strips [strip0, strip0 + ncols) of every image ...
  int slice0, deal;              // ... and writes the partial slices [slice0, slice0 + S); deal: whole items, round robin (wg3_plan.h)
  int relu_in;
};


// ---- fp16 operands (H16 kernels): both tensors are stored as _Float16 and ARE the matrix operands -- one term each, no scale,
// no split: the staging is a copy and a product is ONE MFMA instead of three.  The fp16 gradients carry the step's loss scale;
// the kernels multiply their result by *out_scale (its inverse).
template <bool H16>
struct Quad {
  typedef float4 type;
};
template <>
struct Quad<true> {
  typedef uint2 type;
};
__device__ __forceinline__ unsigned relu_h2(unsigned v) {
  const f16x2 z = {(_Float16)0.0f, (_Float16)0.0f};
  return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(f16x2, v), z));
}
// elements p[px .. px + 3] of a row of n elements (zero outside [0, n)); vec: the quad is inside the row and 4-element aligned
template <bool H16>
__device__ __forceinline__ typename Quad<H16>::type load_quad(const void* row, int px, int n, bool vec, bool relu) {
  if constexpr (H16) {
    const unsigned short* p = static_cast<const unsigned short*>(row);
    uint2 v = make_uint2(0u, 0u);
    if (vec) {
      v = *reinterpret_cast<const uint2*>(p + px);
    } else {
      unsigned e0 = (px >= 0 && px < n) ? p[px] : 0u, e1 = (px + 1 >= 0 && px + 1 < n) ? p[px + 1] : 0u;
      unsigned e2 = (px + 2 >= 0 && px + 2 < n) ? p[px + 2] : 0u, e3 = (px + 3 >= 0 && px + 3 < n) ? p[px + 3] : 0u;
      v = make_uint2(e0 | (e1 << 16), e2 | (e3 << 16));
    }
    if (relu) v = make_uint2(relu_h2(v.x), relu_h2(v.y));
    return v;
  } else {
    const float* p = static_cast<const float*>(row);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (vec) {
      v = *reinterpret_cast<const float4*>(p + px);
    } else {
      if (px >= 0 && px < n) v.x = p[px];
      if (px + 1 >= 0 && px + 1 < n) v.y = p[px + 1];
      if (px + 2 >= 0 && px + 2 < n) v.z = p[px + 2];
      if (px + 3 >= 0 && px + 3 < n) v.w = p[px + 3];
    }
    if (relu) v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
    return v;
  }
}
template <bool H16>
__device__ __forceinline__ typename Quad<H16>::type zero_quad() {
  if constexpr (H16) return make_uint2(0u, 0u);
  else return make_float4(0.f, 0.f, 0.f, 0.f);
}
// split (fp32) or copy (fp16) a staged quad into the LDS row(s): 8 bytes per term
template <bool H16>
__device__ __forceinline__ void store_quad(unsigned char* dst, int tstride, const typename Quad<H16>::type& q, float sc) {
  if constexpr (H16) {
    *reinterpret_cast<uint2*>(dst) = q;
  } else {
    unsigned h0, l0, h1, l1;
    split_pair_f16(q.x * sc, q.y * sc, h0, l0);
    split_pair_f16(q.z * sc, q.w * sc, h1, l1);
    *reinterpret_cast<uint2*>(dst) = make_uint2(h0, h1);
    *reinterpret_cast<uint2*>(dst + tstride) = make_uint2(l0, l1);
  }
}
// fp16 rows are staged 8 pixels (16 bytes) per item: with 4-pixel items the H16 kernels issued twice the loads of the fp32
// kernels per byte and sat on the load-instruction rate (3x3 256 -> 256: the matrix pipe 24 % busy at one MFMA per product).
// p[px .. px + 7] of a row of n elements (zero outside); a8: rows are 16-byte aligned (n % 8 == 0), a4: 8-byte aligned
__device__ __forceinline__ uint4 load_oct_h(const void* row, int px, int n, bool a8, bool a4, bool relu) {
  const unsigned short* p = static_cast<const unsigned short*>(row);
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (a8 && px >= 0 && px + 7 < n) {
    v = *reinterpret_cast<const uint4*>(p + px);
  } else if (a4) {
    if (px >= 0 && px + 3 < n) {
      const uint2 t = *reinterpret_cast<const uint2*>(p + px);
      v.x = t.x;
      v.y = t.y;
    }
    if (px + 4 >= 0 && px + 7 < n) {
      const uint2 t = *reinterpret_cast<const uint2*>(p + px + 4);
      v.z = t.x;
      v.w = t.y;
    }
  } else {
    unsigned e[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) e[i] = (px + i >= 0 && px + i < n) ? p[px + i] : 0u;
    v = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
  }
  if (relu) v = make_uint4(relu_h2(v.x), relu_h2(v.y), relu_h2(v.z), relu_h2(v.w));
  return v;
}

constexpr int kW3NT = 768;                    // 12 waves: 2 x 2 tile pairs x 3 kernel rows (strip, pitches, LDS bytes: wg3_plan.h)

// Live K steps: a row step runs NK = ceil(min(64, W - c0) / 16) K steps, the ones that hold pixels of the row.
// NK is a template parameter of the three walking kernels -- the staging registers stay indexed by constants, the row step
// stays one basic block, and a kernel holds ONE row loop (four loops behind a block-uniform switch cost xwgrad3_kernel 40
// VGPRs and put 112 dwords into scratch) -- and the strips of one NK are a launch of their own (wg3_plan.h).  Every staging
// item is still loaded and stored (the ones wholly past the row's end as zeros), so no LDS cell a live K step reads -- the
// neighbour dwords of the first and last live cell included -- ever holds another segment's data; item i rides behind K step
// i % NK.
// The walk of a slice is the same in every lane: its state and results are kept in scalar registers.
#define DVD_WG_WALK_BEGIN(a)                             \
  int wcur, wend;                                        \
  wg_walk_begin(a, (int)blockIdx.x, wcur, wend);         \
  wcur = __builtin_amdgcn_readfirstlane(wcur);           \
  wend = __builtin_amdgcn_readfirstlane(wend);           \
  while (wcur < wend)
#define DVD_WG_WALK_SEGMENT(a)                                               \
  int wn, wstrip, wr0, wr1, wnext;                                           \
  wg_walk_segment(a, wcur, wend, wn, wstrip, wr0, wr1, wnext);               \
  wcur = __builtin_amdgcn_readfirstlane(wnext);                              \
  const int n = __builtin_amdgcn_readfirstlane(wn), c0 = __builtin_amdgcn_readfirstlane(wstrip) * kW3Strip; \
  const int r0 = __builtin_amdgcn_readfirstlane(wr0), r1 = __builtin_amdgcn_readfirstlane(wr1);

// FW (host: rows of fp16 elements start dword-aligned, i.e. W even; any W for fp32): every staging item is a 16-byte run of one
// row (a run crossing the row's end is loaded whole and its tail zeroed on the way to LDS, as in xwgrad3g_kernel) or nothing,
// so the loads are raw BUFFER loads with a per-thread offset computed once per work item (channels past the tensor
// and columns outside the image fall out of the resource's range and read 0) -- no branch in the row step.  With the body one
// basic block, the staging work of item i (split + LDS store of the row loaded a step ago, request of the row two steps ahead)
// sits between the MFMAs of K step i: round 3 ran `barrier | all staging | all MFMAs` in every wave, the 12 waves in lock step
// behind the barrier, and the counters showed matrix pipe and VALU taking turns (55 % busy at 5.5 VALU per MFMA).
template <bool H16, bool FW, int NK = 4>
__global__ __launch_bounds__(kW3NT) void xwgrad3_kernel(const Wg3Args a) {
  constexpr int EB = H16 ? 2 : 4;                // bytes per element in HBM
  constexpr int NTERM = H16 ? 1 : 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem3[];
  // sG [buffer 2][term 2][co 64][kW3GPitch], sX [term 2][slot 4][ci 64][kW3XPitch] (slot-major: a channel stride of
  // 44 dwords keeps the 16-byte fragment reads of 32 channels conflict free; 4 x 44 did not)
  unsigned char* sG = smem3;
  unsigned char* sX = smem3 + 2 * 2 * kW3CB * kW3GPitch;
  const float sx = H16 ? 1.0f : pow2_scale(a.x_amax[0]), sg = H16 ? 1.0f : pow2_scale(a.g_amax[0]);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ky = wave % 3, pn = (wave / 3) & 1, pm = wave / 6;
  const int grp = blockIdx.z / a.nco;                      // group of a grouped convolution (0 for dense)
  const int co0 = (blockIdx.z - grp * a.nco) * kW3CB, ci0 = blockIdx.y * kW3CB;
  const size_t plane = (size_t)a.H * a.W;

  // staging assignment: a thread stages QW consecutive pixels of one channel row (fp32: 4 = 16 bytes; fp16: 8 = 16 bytes).
  //   fp32: gy row 64 channels x 16 items, x row 64 x 20 -> 3 per thread;  fp16: 64 x 8 and 64 x 10 -> 2 per thread
  constexpr int QW = H16 ? 8 : 4, GPR = 64 / QW, XPR = 80 / QW;
  constexpr int GQ = kW3CB * GPR, XQ = kW3CB * XPR, NQ = (GQ + XQ + kW3NT - 1) / kW3NT;
  typedef std::conditional_t<H16, uint4, float4> StgT;
  StgT stg[NQ];
  const bool wvec = (a.W & 3) == 0, wvec8 = (a.W & 7) == 0;
  auto zero_item = [&]() -> StgT {
    if constexpr (H16) return make_uint4(0u, 0u, 0u, 0u);
    else return make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto load_item = [&](const unsigned char* row, int px, bool relu) -> StgT {
    if constexpr (H16) return load_oct_h(row, px, a.W, wvec8, wvec, relu);
    else return load_quad<false>(row, px, a.W, wvec && px >= 0 && px + 3 < a.W, relu);
  };
  auto stage_load = [&](int n, int c0, int r, bool with_g) {   // gy row r (if with_g) and x row r + 1
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int q = i * kW3NT + tid;
      StgT v = zero_item();
      if (q < GQ) {
        const int ch = q / GPR, px = c0 + (q - ch * GPR) * QW;
        if (with_g && (co0 + ch) < a.Cout && r < a.H) {
          const unsigned char* p = static_cast<const unsigned char*>(a.gy) +
                                   ((((size_t)n * a.G + grp) * a.Cout + co0 + ch) * plane + (size_t)r * a.W) * EB;
          v = load_item(p, px, false);
        }
      } else if (q < GQ + XQ) {
        const int qq = q - GQ;
        const int ch = qq / XPR, px = c0 - 8 + (qq - ch * XPR) * QW;
        const int row = r + 1;
        if ((ci0 + ch) < a.Cin && row >= 0 && row < a.H) {
          const unsigned char* p = static_cast<const unsigned char*>(a.x) +
                                   ((((size_t)n * a.G + grp) * a.Cin + ci0 + ch) * plane + (size_t)row * a.W) * EB;
          v = load_item(p, px, a.relu_in != 0);
        }
      }
      stg[i] = v;
    }
  };
  auto stage_store = [&](int xslot, int gbuf) {      // split (fp32) or copy (fp16) and write: 4 pixels = 8 bytes per term
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int q = i * kW3NT + tid;
      if (q >= GQ + XQ) continue;
      const float sc = q < GQ ? sg : sx;
      unsigned char* dst;
      int tstride;
      if (q < GQ) {
        const int ch = q / GPR;
        dst = sG + gbuf * (2 * kW3CB * kW3GPitch) + ch * kW3GPitch + (q - ch * GPR) * (QW * 2);
        tstride = kW3CB * kW3GPitch;
      } else {
        const int qq = q - GQ, ch = qq / XPR;
        dst = sX + (xslot * kW3CB + ch) * kW3XPitch + (qq - ch * XPR) * (QW * 2);
        tstride = kW3CB * 4 * kW3XPitch;
      }
      if constexpr (H16) *reinterpret_cast<uint4*>(dst) = stg[i];
      else store_quad<false>(dst, tstride, stg[i], sc);
    }
  };

  f32x16 acc[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) acc[k] = (f32x16){0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int half = lane >> 5;
  const unsigned char* ga = sG + (pm * 32 + (lane & 31)) * kW3GPitch + half * 16;
  const unsigned char* xa = sX + (pn * 32 + (lane & 31)) * kW3XPitch + 16 + half * 16;   // cell 1 + half of slot 0

  // ---- FW staging (see the kernel's header): per-thread constants of the NQ staging items
  bool f_isg[NQ];          // wave-uniform: the item is a gy run (else an x run)
  int f_ch[NQ], f_pq[NQ], f_lds[NQ];
  if constexpr (FW) {
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int q = i * kW3NT + tid;
      f_isg[i] = __builtin_amdgcn_readfirstlane(q < GQ ? 1 : 0) != 0;          // GQ is a multiple of 64
      const int qq = f_isg[i] ? q : q - GQ;
      const int pr = f_isg[i] ? GPR : XPR;
      f_ch[i] = qq / pr;
      const int cell = qq - f_ch[i] * pr;
      f_pq[i] = cell * QW - (f_isg[i] ? 0 : 8);
      // items past the two rows (fp16: the last six waves of item 1) load nothing and store into the spare 16 bytes
      f_lds[i] = q >= GQ + XQ ? kW3LdsBytes
                              : (f_isg[i] ? f_ch[i] * kW3GPitch : (int)(sX - smem3) + f_ch[i] * kW3XPitch) + cell * (QW * 2);
      if (q >= GQ + XQ) f_ch[i] = 1 << 20;                                       // beyond any resource's range
    }
  }
  u32x4 fstg[NQ];
  int f_voff[NQ];
  float f_sc[H16 ? 1 : NQ][4];          // fp32: the operand scale per element of the run, 0 past the row's end (xwgrad3g_kernel)
  unsigned f_msk[H16 ? NQ : 1][4];      // fp16: all-ones / zero halves
  __amdgpu_buffer_rsrc_t srdX, srdG;
  const float relu_lo = a.relu_in ? 0.0f : -__builtin_inff();
  const unsigned relu_lo_h = a.relu_in ? 0u : 0xfc00fc00u;                      // packed halves: 0 | -inf
  auto f_load = [&](int i, int rg, bool with_g) {                               // item i of (gy row rg, x row rg + 1)
    const int row = f_isg[i] ? rg : rg + 1;
    const bool ok = row >= 0 && row < a.H && (with_g || !f_isg[i]);              // wave-uniform
    const int vo = ok ? f_voff[i] : (int)0x80000000;
    const int so = ok ? row * a.W * EB : 0;
    fstg[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(f_isg[i] ? srdG : srdX, vo, so, 0));
  };
  auto f_store = [&](int i, int xslot, int gbuf) {
    unsigned char* dst = smem3 + f_lds[i] + (f_isg[i] ? gbuf * (2 * kW3CB * kW3GPitch) : xslot * (kW3CB * kW3XPitch));
    if constexpr (H16) {
      u32x4 v = fstg[i];
      const f16x2 lo = __builtin_bit_cast(f16x2, f_isg[i] ? 0xfc00fc00u : relu_lo_h);   // ReLU of the activations (no-op against -inf)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        v[j] = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(f16x2, (unsigned)v[j]), lo)) & f_msk[i][j];
      *reinterpret_cast<u32x4*>(dst) = v;
    } else {
      const float lo = f_isg[i] ? -__builtin_inff() : relu_lo;
      const float v0 = fmaxf(__uint_as_float(fstg[i][0]), lo) * f_sc[i][0], v1 = fmaxf(__uint_as_float(fstg[i][1]), lo) * f_sc[i][1];
      const float v2 = fmaxf(__uint_as_float(fstg[i][2]), lo) * f_sc[i][2], v3 = fmaxf(__uint_as_float(fstg[i][3]), lo) * f_sc[i][3];
      unsigned h0, l0, h1, l1;
      split_pair_f16(v0, v1, h0, l0);
      split_pair_f16(v2, v3, h1, l1);
      *reinterpret_cast<uint2*>(dst) = make_uint2(h0, h1);
      *reinterpret_cast<uint2*>(dst + (f_isg[i] ? kW3CB * kW3GPitch : kW3CB * 4 * kW3XPitch)) = make_uint2(l0, l1);
    }
  };

  DVD_WG_WALK_BEGIN(a) {
    DVD_WG_WALK_SEGMENT(a)
    if constexpr (FW) {
      // this image's 64 channels of either tensor as buffer resources: channels past the tensor are out of range
      const int nci = (a.Cin - ci0) < kW3CB ? (a.Cin - ci0) : kW3CB, nco = (a.Cout - co0) < kW3CB ? (a.Cout - co0) : kW3CB;
      const unsigned char* xb = static_cast<const unsigned char*>(a.x) + (((size_t)n * a.G + grp) * a.Cin + ci0) * plane * EB;
      const unsigned char* gb = static_cast<const unsigned char*>(a.gy) + (((size_t)n * a.G + grp) * a.Cout + co0) * plane * EB;
      srdX = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(const_cast<unsigned char*>(xb)), 0, nci * (int)plane * EB, 0x00020000);
      srdG = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(const_cast<unsigned char*>(gb)), 0, nco * (int)plane * EB, 0x00020000);
#pragma unroll
      for (int i = 0; i < NQ; ++i) {
        // a run that crosses the end of its row is loaded anyway and the elements past the row are zeroed on the way to LDS
        const int px = c0 + f_pq[i];
        const int nv = px < 0 ? 0 : ((a.W - px) < QW ? (a.W - px) : QW);
        f_voff[i] = (nv > 0 && f_ch[i] < kW3CB) ? (f_ch[i] * (int)plane + px) * EB : (int)0x80000000;
        if constexpr (H16) {
#pragma unroll
          for (int j = 0; j < 4; ++j) f_msk[i][j] = (2 * j < nv ? 0xffffu : 0u) | (2 * j + 1 < nv ? 0xffff0000u : 0u);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) f_sc[i][e] = e < nv ? (f_isg[i] ? sg : sx) : 0.0f;
        }
      }
    }
    auto load_all = [&](int rg, bool with_g) {
      if constexpr (FW) {
#pragma unroll
        for (int i = 0; i < NQ; ++i) f_load(i, rg, with_g);
      } else {
        stage_load(n, c0, rg, with_g);
      }
    };
    auto store_all = [&](int xslot, int gbuf) {
      if constexpr (FW) {
#pragma unroll
        for (int i = 0; i < NQ; ++i) f_store(i, xslot, gbuf);
      } else {
        stage_store(xslot, gbuf);
      }
    };
    // Four x-row slots (row & 3) and two gy buffers (row & 1): step r reads x rows r - 1 .. r + 1 and gy row r while the
    // rows of step r + 1 (x row r + 2, gy row r + 1: loaded during step r - 1) are split and stored and the rows of step
    // r + 2 are requested -- ONE barrier per step, and no phase in which every wave of the block does staging work while
    // the matrix pipe idles (round 2 stored between two barriers).
    __syncthreads();                               // the previous item's MFMAs have read their operands
    load_all(r0 - 2, false);
    store_all((r0 - 1) & 3, (r0 + 1) & 1);         // x row r0 - 1 (the gy half of these two stores is zeros into the idle buffer)
    load_all(r0 - 1, false);
    store_all(r0 & 3, (r0 + 1) & 1);               // x row r0
    load_all(r0, true);
    store_all((r0 + 1) & 3, r0 & 1);               // gy row r0, x row r0 + 1
    load_all(r0 + 1, true);                        // gy row r0 + 1, x row r0 + 2 in registers
    for (int r = r0; r < r1; ++r) {
      __syncthreads();                             // the rows of step r are complete; step r - 1 has been read by every wave
      if constexpr (!FW) {
        stage_store((r + 2) & 3, (r + 1) & 1);     // for step r + 1 (x row r - 2 / gy row r - 1 are no longer needed)
        stage_load(n, c0, r + 2, true);            // for step r + 2: in flight under this step's MFMAs
      }
      const int slot = (r - 1 + ky) & 3;           // x row r - 1 + ky
      const unsigned char* xr = xa + slot * (kW3CB * kW3XPitch);
      const unsigned char* gr = ga + (r & 1) * (2 * kW3CB * kW3GPitch);
#pragma unroll
      for (int s = 0; s < NK; ++s) {               // the live K steps of 16 pixels
        f16x8 A[NTERM], B[3][NTERM];
#pragma unroll
        for (int t = 0; t < NTERM; ++t) {
          A[t] = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(gr + t * (kW3CB * kW3GPitch) + s * 32));
          const unsigned char* xc = xr + t * (kW3CB * 4 * kW3XPitch) + s * 32;
          const u32x4 cur = *reinterpret_cast<const u32x4*>(xc);
          const unsigned prev3 = *reinterpret_cast<const unsigned*>(xc - 4);
          const unsigned next0 = *reinterpret_cast<const unsigned*>(xc + 16);
          const unsigned t0 = __builtin_amdgcn_alignbit(cur.x, prev3, 16), t1 = __builtin_amdgcn_alignbit(cur.y, cur.x, 16),
                         t2 = __builtin_amdgcn_alignbit(cur.z, cur.y, 16), t3 = __builtin_amdgcn_alignbit(cur.w, cur.z, 16),
                         t4 = __builtin_amdgcn_alignbit(next0, cur.w, 16);
          B[0][t] = __builtin_bit_cast(f16x8, (u32x4){t0, t1, t2, t3});   // kx = 0: pixels shifted by -1
          B[1][t] = __builtin_bit_cast(f16x8, cur);                        // kx = 1
          B[2][t] = __builtin_bit_cast(f16x8, (u32x4){t1, t2, t3, t4});   // kx = 2: shifted by +1
        }
#define DVD_W3TERM(SA, SB)                                                                                  \
  _Pragma("unroll") for (int kx = 0; kx < 3; ++kx) acc[kx] =                                                \
      __builtin_amdgcn_mfma_f32_32x32x16_f16(A[SA], B[kx][SB], acc[kx], 0, 0, 0);
        if constexpr (!H16) {
          DVD_W3TERM(NTERM - 1, 0)
          DVD_W3TERM(0, NTERM - 1)
        }
        DVD_W3TERM(0, 0)
#undef DVD_W3TERM
        if constexpr (FW) {
          // staging item i rides behind the MFMAs of K step i % NK: store the run loaded a step ago (for step r + 1), then
          // request the same run two rows further down (for step r + 2)
#pragma unroll
          for (int i = s; i < NQ; i += NK) {
            f_store(i, (r + 2) & 3, (r + 1) & 1);
            f_load(i, r + 2, true);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  }
  // partial[s][tap][G * Cout][Cin]
  float* dst = a.partial + (size_t)(a.slice0 + blockIdx.x) * 9 * a.G * a.Cout * a.Cin;
  const float unscale = H16 ? (a.out_scale ? a.out_scale[0] : 1.0f) : 1.0f / (sx * sg);          // fp32: exact power of two
#pragma unroll
  for (int kx = 0; kx < 3; ++kx) {
    const int tap = ky * 3 + kx;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + pm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const int ci = ci0 + pn * 32 + (lane & 31);
      if (co < a.Cout && ci < a.Cin) dst[((size_t)tap * a.G * a.Cout + grp * a.Cout + co) * a.Cin + ci] = acc[kx][r] * unscale;
    }
  }
}

// ---- 5x5 / 7x7 / 11x11 (round 4): the same walk with KS kernel rows.  Replaces the weight gradient of the hourglass's large
// inception branches (third_party/hourglass.py:21-57) -- MIOpen in round 3, the exact-fp32 MFMA kernel of csrc/xwgrad.hip at the
// start of round 4 (37 % of an hourglass step: fp32 MFMAs run at the vector rate).  A block owns 32 output x 32 input channels;
// wave ky keeps the KXN accumulators of kernel row ky for the columns [KX0, KX0 + KXN) (an 11-wide row takes two launches so
// that the accumulators fit the register file); KS + 1 x-row slots roll through LDS (rows r - pad .. r + pad are read while
// row r + pad + 1 is stored).  The fragment of column offset s is eight pixels starting s pixels off the lane's cell: the
// lane reads the cell and both neighbours as 16-byte cells (conflict free) and takes the run out of the 12 dwords -- a plain
// register selection for even s, v_alignbit for odd s (one shared chain of alignbits serves all odd offsets).
// H16 (fp16 activation storage): the fp16 tensors themselves are the operands -- one term, no operand scale, the staging a copy,
// ONE MFMA per product instead of three, the LDS of the second term not allocated; the result is multiplied by *out_scale.
template <bool H16, int KS, int KX0, int KXN, int NK = 4>
__global__ __launch_bounds__(64 * KS) void xwgradk_kernel(const Wg3Args a) {
  constexpr int PAD = KS / 2, NS = KS + 1, CB = 32, NT = 64 * KS;
  constexpr int EB = H16 ? 2 : 4, NTERM = H16 ? 1 : 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem3[];
  constexpr int kGBuf = NTERM * CB * kW3GPitch;                // one gy buffer: [term NTERM][co 32][kW3GPitch]
  unsigned char* sG = smem3;                                   // [buffer 2][term][co 32][kW3GPitch]
  unsigned char* sX = smem3 + 2 * kGBuf;                       // [term][slot NS][ci 32][kW3XPitch]
  constexpr int kXTerm = NS * CB * kW3XPitch;
  const float sx = H16 ? 1.0f : pow2_scale(a.x_amax[0]), sg = H16 ? 1.0f : pow2_scale(a.g_amax[0]);
  const int tid = threadIdx.x, lane = tid & 63, ky = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int co0 = blockIdx.z * CB, ci0 = blockIdx.y * CB;
  const size_t plane = (size_t)a.H * a.W;
  constexpr int GQ = CB * 16, XQ = CB * 20, NQ = (GQ + XQ + NT - 1) / NT;
  typename Quad<H16>::type stg[NQ];
  const bool wvec = (a.W & 3) == 0;
  auto slot_of = [](int row) { return (row + 64) % NS; };      // rows >= -PAD
  auto stage_load = [&](int n, int c0, int grow, int xrow) {   // gy row `grow` (< 0: none) and x row `xrow`
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int q = i * NT + tid;
      typename Quad<H16>::type v = zero_quad<H16>();
      if (q < GQ) {
        const int ch = q >> 4, px = c0 + ((q & 15) << 2);
        if (grow >= 0 && (co0 + ch) < a.Cout && grow < a.H)
          v = load_quad<H16>(static_cast<const unsigned char*>(a.gy) + (((size_t)n * a.Cout + co0 + ch) * plane + (size_t)grow * a.W) * EB,
                             px, a.W, wvec && px + 3 < a.W, false);
      } else if (q < GQ + XQ) {
        const int qq = q - GQ;
        const int ch = qq / 20, px = c0 - 8 + ((qq - ch * 20) << 2);
        if ((ci0 + ch) < a.Cin && xrow >= 0 && xrow < a.H)
          v = load_quad<H16>(static_cast<const unsigned char*>(a.x) + (((size_t)n * a.Cin + ci0 + ch) * plane + (size_t)xrow * a.W) * EB,
                             px, a.W, wvec && px >= 0 && px + 3 < a.W, a.relu_in != 0);
      }
      stg[i] = v;
    }
  };
  auto stage_store = [&](int xslot, int gbuf) {
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int q = i * NT + tid;
      if (q >= GQ + XQ) continue;
      if (q < GQ) {
        store_quad<H16>(sG + gbuf * kGBuf + (q >> 4) * kW3GPitch + ((q & 15) << 3), CB * kW3GPitch, stg[i], sg);
      } else {
        const int qq = q - GQ, ch = qq / 20;
        store_quad<H16>(sX + (xslot * CB + ch) * kW3XPitch + ((qq - ch * 20) << 3), kXTerm, stg[i], sx);
      }
    }
  };
  f32x16 acc[KXN];
#pragma unroll
  for (int k = 0; k < KXN; ++k) acc[k] = (f32x16){0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int half = lane >> 5;
  const unsigned char* ga = sG + (lane & 31) * kW3GPitch + half * 16;
  const unsigned char* xa = sX + (lane & 31) * kW3XPitch + 16 + half * 16;     // cell 1 + half of slot 0

  DVD_WG_WALK_BEGIN(a) {
    DVD_WG_WALK_SEGMENT(a)
    __syncthreads();                               // the previous item's MFMAs have read their operands
    for (int j = -PAD; j < PAD; ++j) {             // x rows r0 - pad .. r0 + pad - 1 (the gy halves: zeros into the idle buffer)
      stage_load(n, c0, -1, r0 + j);
      stage_store(slot_of(r0 + j), (r0 + 1) & 1);
    }
    stage_load(n, c0, r0, r0 + PAD);
    stage_store(slot_of(r0 + PAD), r0 & 1);        // gy row r0, x row r0 + pad
    stage_load(n, c0, r0 + 1, r0 + 1 + PAD);       // in registers: the rows step r0 stores for step r0 + 1
    for (int r = r0; r < r1; ++r) {
      __syncthreads();                             // the rows of step r are complete; step r - 1 has been read by every wave
      stage_store(slot_of(r + 1 + PAD), (r + 1) & 1);
      stage_load(n, c0, r + 2, r + 2 + PAD);
      const unsigned char* xr = xa + slot_of(r - PAD + ky) * (CB * kW3XPitch);
      const unsigned char* gr = ga + (r & 1) * kGBuf;
#pragma unroll
      for (int s = 0; s < NK; ++s) {               // the live K steps of 16 pixels
        f16x8 A[NTERM];
        unsigned d[NTERM][12];                     // per term: previous cell, the lane's cell, next cell (24 pixels)
#pragma unroll
        for (int t = 0; t < NTERM; ++t) {
          A[t] = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(gr + t * (CB * kW3GPitch) + s * 32));
          const unsigned char* xc = xr + t * kXTerm + s * 32;
          const u32x4 p = *reinterpret_cast<const u32x4*>(xc - 16), c = *reinterpret_cast<const u32x4*>(xc),
                      nn = *reinterpret_cast<const u32x4*>(xc + 16);
          d[t][0] = p.x; d[t][1] = p.y; d[t][2] = p.z; d[t][3] = p.w;
          d[t][4] = c.x; d[t][5] = c.y; d[t][6] = c.z; d[t][7] = c.w;
          d[t][8] = nn.x; d[t][9] = nn.y; d[t][10] = nn.z; d[t][11] = nn.w;
        }
#pragma unroll
        for (int kx = 0; kx < KXN; ++kx) {
          const int sh = KX0 + kx - PAD;           // column offset in pixels (compile-time after unrolling)
          const int st = 8 + sh;                   // first pixel of the run inside the 24-pixel window (3 .. 13)
          f16x8 B[NTERM];
#pragma unroll
          for (int t = 0; t < NTERM; ++t) {
            u32x4 f;
            if ((st & 1) == 0) {
              const int j = st >> 1;
              f = (u32x4){d[t][j], d[t][j + 1], d[t][j + 2], d[t][j + 3]};
            } else {
              const int j = (st - 1) >> 1;
              f = (u32x4){__builtin_amdgcn_alignbit(d[t][j + 1], d[t][j], 16), __builtin_amdgcn_alignbit(d[t][j + 2], d[t][j + 1], 16),
                          __builtin_amdgcn_alignbit(d[t][j + 3], d[t][j + 2], 16), __builtin_amdgcn_alignbit(d[t][j + 4], d[t][j + 3], 16)};
            }
            B[t] = __builtin_bit_cast(f16x8, f);
          }
          if constexpr (H16) {
            acc[kx] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[0], B[0], acc[kx], 0, 0, 0);
          } else {
            acc[kx] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[1], B[0], acc[kx], 0, 0, 0);     // small terms first
            acc[kx] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[0], B[1], acc[kx], 0, 0, 0);
            acc[kx] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[0], B[0], acc[kx], 0, 0, 0);
          }
        }
      }
    }
  }
  float* dst = a.partial + (size_t)(a.slice0 + blockIdx.x) * (KS * KS) * a.Cout * a.Cin;      // partial[s][tap][Cout][Cin]
  const float unscale = H16 ? (a.out_scale ? a.out_scale[0] : 1.0f) : 1.0f / (sx * sg);
#pragma unroll
  for (int kx = 0; kx < KXN; ++kx) {
    const int tap = ky * KS + KX0 + kx;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const int ci = ci0 + (lane & 31);
      if (co < a.Cout && ci < a.Cin) dst[((size_t)tap * a.Cout + co) * a.Cin + ci] = acc[kx][r] * unscale;
    }
  }
}

// ---- grouped 3x3 with at most 32 channels per group on either side (ResNeXt stages 2 and 3: 16 / 32 per group) -----------
// On xwgrad3_kernel's 64 x 64 channel blocks only one of the four 32 x 32 tile pairs of a block holds data (16 per group: a
// quarter of that pair): three of twelve waves did useful MFMAs while all twelve staged zeros -- 0.42 ms per stage-3 layer
// at 48 x 1024 x 24 x 42 against 0.1 ms of HBM traffic, 4 % of a step for 1 % of its FLOPs.  Here a block is one 32 x 32
// pair and three waves (one per kernel row); two blocks share a CU.  Same walk, same row step as xwgrad3_kernel<., FW>
// (buffer loads, the staging of item i between the MFMAs), same per-element products in the same order: bit-identical sums.
// Rows need not be whole staging items: a run that crosses the end of its row is loaded anyway (dword-aligned 16-byte buffer
// loads) and the elements past the row are zeroed on the way to LDS -- for fp32 by the per-element operand scale the split
// multiplies by anyway (0 instead of 2^e), for fp16 by a mask -- so the 42- and 21-pixel rows of stages 3 and 4 take the
// same path as the rest.
constexpr int kWgNT = 192;

// RSUM (fp32 only; host: a.rowsum_partial is set): the kernel also sums the gy rows it stages, per output channel -- the shift
// gradient of a BatchNorm fused behind the convolution (conv._XConvBn), which otherwise takes a pass over gy of its own.  A thread
// stages the same (at most three) gy channel rows for the whole walk, so it keeps one accumulator per gy item and adds the four
// scaled, row-end-masked values the split consumes anyway; rows the walk stages beyond its segment (the look-ahead row r1) are
// gated out, so every element of a (group, co block) counts exactly once over the slices.  Without RSUM the code is unchanged.
template <bool H16, bool RSUM = false, int NK = 4>
__global__ __launch_bounds__(kWgNT) void xwgrad3g_kernel(const Wg3Args a) {
  static_assert(!(H16 && RSUM), "the channel sums exist for fp32 gradients");
  constexpr int EB = H16 ? 2 : 4, NTERM = H16 ? 1 : 2, CB = kWgCB;
  constexpr int QW = H16 ? 8 : 4, GPR = 64 / QW, XPR = 80 / QW, GQ = CB * GPR, XQ = CB * XPR, NQ = (GQ + XQ) / kWgNT;
  static_assert((GQ + XQ) % kWgNT == 0 && GQ % 64 == 0, "staging items divide evenly over the threads, wave-uniform kind");
  constexpr int NG = (GQ + kWgNT - 1) / kWgNT;      // staging items of a thread that can be gy runs: i < NG
  float rs[RSUM ? NG : 1];
#pragma unroll
  for (int i = 0; i < (RSUM ? NG : 1); ++i) rs[i] = 0.0f;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem3[];
  unsigned char* sG = smem3;                                   // [buffer 2][term 2][co 32][kW3GPitch]
  unsigned char* sX = smem3 + 2 * 2 * CB * kW3GPitch;          // [term 2][slot 4][ci 32][kW3XPitch]
  const float sx = H16 ? 1.0f : pow2_scale(a.x_amax[0]), sg = H16 ? 1.0f : pow2_scale(a.g_amax[0]);
  const int tid = threadIdx.x, lane = tid & 63, ky = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = blockIdx.z / a.nco;
  const int co0 = (blockIdx.z - grp * a.nco) * CB, ci0 = blockIdx.y * CB;
  const size_t plane = (size_t)a.H * a.W;

  bool isg[NQ];
  int f_ch[NQ], f_pq[NQ], f_lds[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    const int q = i * kWgNT + tid;
    isg[i] = __builtin_amdgcn_readfirstlane(q < GQ ? 1 : 0) != 0;
    const int qq = isg[i] ? q : q - GQ, pr = isg[i] ? GPR : XPR;
    f_ch[i] = qq / pr;
    const int cell = qq - f_ch[i] * pr;
    f_pq[i] = cell * QW - (isg[i] ? 0 : 8);
    f_lds[i] = (isg[i] ? f_ch[i] * kW3GPitch : (int)(sX - smem3) + f_ch[i] * kW3XPitch) + cell * (QW * 2);
  }
  u32x4 fstg[NQ];
  int f_voff[NQ];
  float f_sc[H16 ? 1 : NQ][4];          // fp32: the operand scale per element of the run, 0 past the row's end
  unsigned f_msk[H16 ? NQ : 1][4];      // fp16: all-ones / zero halves
  __amdgpu_buffer_rsrc_t srdX, srdG;
  const float relu_lo = a.relu_in ? 0.0f : -__builtin_inff();
  const unsigned relu_lo_h = a.relu_in ? 0u : 0xfc00fc00u;
  auto f_load = [&](int i, int rg, bool with_g) {
    const int row = isg[i] ? rg : rg + 1;
    const bool ok = row >= 0 && row < a.H && (with_g || !isg[i]);
    const int vo = ok ? f_voff[i] : (int)0x80000000;
    const int so = ok ? row * a.W * EB : 0;
    fstg[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(isg[i] ? srdG : srdX, vo, so, 0));
  };
  auto f_store = [&](int i, int xslot, int gbuf, bool g_live) {        // g_live (wave-uniform): the gy row belongs to this item's rows
    unsigned char* dst = smem3 + f_lds[i] + (isg[i] ? gbuf * (2 * CB * kW3GPitch) : xslot * (CB * kW3XPitch));
    if constexpr (H16) {
      u32x4 v = fstg[i];
      const f16x2 lo = __builtin_bit_cast(f16x2, isg[i] ? 0xfc00fc00u : relu_lo_h);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        v[j] = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(f16x2, (unsigned)v[j]), lo)) & f_msk[i][j];
      *reinterpret_cast<u32x4*>(dst) = v;
    } else {
      const float lo = isg[i] ? -__builtin_inff() : relu_lo;
      const float v0 = fmaxf(__uint_as_float(fstg[i][0]), lo) * f_sc[i][0], v1 = fmaxf(__uint_as_float(fstg[i][1]), lo) * f_sc[i][1];
      const float v2 = fmaxf(__uint_as_float(fstg[i][2]), lo) * f_sc[i][2], v3 = fmaxf(__uint_as_float(fstg[i][3]), lo) * f_sc[i][3];
      if constexpr (RSUM) {
        if (i < NG && isg[i]) rs[i] += g_live ? (v0 + v1) + (v2 + v3) : 0.0f;
      }
      unsigned h0, l0, h1, l1;
      split_pair_f16(v0, v1, h0, l0);
      split_pair_f16(v2, v3, h1, l1);
      *reinterpret_cast<uint2*>(dst) = make_uint2(h0, h1);
      *reinterpret_cast<uint2*>(dst + (isg[i] ? CB * kW3GPitch : CB * 4 * kW3XPitch)) = make_uint2(l0, l1);
    }
  };

  f32x16 acc[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) acc[k] = (f32x16){0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int half = lane >> 5;
  const unsigned char* ga = sG + (lane & 31) * kW3GPitch + half * 16;
  const unsigned char* xa = sX + (lane & 31) * kW3XPitch + 16 + half * 16;     // cell 1 + half of slot 0

  DVD_WG_WALK_BEGIN(a) {
    DVD_WG_WALK_SEGMENT(a)
    {
      const int nci = (a.Cin - ci0) < CB ? (a.Cin - ci0) : CB, nco = (a.Cout - co0) < CB ? (a.Cout - co0) : CB;
      const unsigned char* xb = static_cast<const unsigned char*>(a.x) + (((size_t)n * a.G + grp) * a.Cin + ci0) * plane * EB;
      const unsigned char* gb = static_cast<const unsigned char*>(a.gy) + (((size_t)n * a.G + grp) * a.Cout + co0) * plane * EB;
      srdX = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(const_cast<unsigned char*>(xb)), 0, nci * (int)plane * EB, 0x00020000);
      srdG = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(const_cast<unsigned char*>(gb)), 0, nco * (int)plane * EB, 0x00020000);
#pragma unroll
      for (int i = 0; i < NQ; ++i) {
        const int px = c0 + f_pq[i];
        const int nv = px < 0 ? 0 : ((a.W - px) < QW ? (a.W - px) : QW);       // elements of the run inside the row (<= 0: none)
        f_voff[i] = nv > 0 ? (f_ch[i] * (int)plane + px) * EB : (int)0x80000000;
        if constexpr (H16) {
#pragma unroll
          for (int j = 0; j < 4; ++j) f_msk[i][j] = (2 * j < nv ? 0xffffu : 0u) | (2 * j + 1 < nv ? 0xffff0000u : 0u);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) f_sc[i][e] = e < nv ? (isg[i] ? sg : sx) : 0.0f;
        }
      }
    }
    auto load_all = [&](int rg, bool with_g) {
#pragma unroll
      for (int i = 0; i < NQ; ++i) f_load(i, rg, with_g);
    };
    auto store_all = [&](int xslot, int gbuf) {       // (the prologue's gy rows: zeros, then row r0)
#pragma unroll
      for (int i = 0; i < NQ; ++i) f_store(i, xslot, gbuf, true);
    };
    __syncthreads();                               // the previous item's MFMAs have read their operands
    load_all(r0 - 2, false);
    store_all((r0 - 1) & 3, (r0 + 1) & 1);         // x row r0 - 1 (the gy half: zeros into the idle buffer)
    load_all(r0 - 1, false);
    store_all(r0 & 3, (r0 + 1) & 1);               // x row r0
    load_all(r0, true);
    store_all((r0 + 1) & 3, r0 & 1);               // gy row r0, x row r0 + 1
    load_all(r0 + 1, true);                        // gy row r0 + 1, x row r0 + 2 in registers
    for (int r = r0; r < r1; ++r) {
      __syncthreads();                             // the rows of step r are complete; step r - 1 has been read by every wave
      const int slot = (r - 1 + ky) & 3;           // x row r - 1 + ky
      const unsigned char* xr = xa + slot * (CB * kW3XPitch);
      const unsigned char* gr = ga + (r & 1) * (2 * CB * kW3GPitch);
#pragma unroll
      for (int s = 0; s < NK; ++s) {               // the live K steps of 16 pixels
        f16x8 A[NTERM], B[3][NTERM];
#pragma unroll
        for (int t = 0; t < NTERM; ++t) {
          A[t] = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(gr + t * (CB * kW3GPitch) + s * 32));
          const unsigned char* xc = xr + t * (CB * 4 * kW3XPitch) + s * 32;
          const u32x4 cur = *reinterpret_cast<const u32x4*>(xc);
          const unsigned prev3 = *reinterpret_cast<const unsigned*>(xc - 4);
          const unsigned next0 = *reinterpret_cast<const unsigned*>(xc + 16);
          const unsigned t0 = __builtin_amdgcn_alignbit(cur.x, prev3, 16), t1 = __builtin_amdgcn_alignbit(cur.y, cur.x, 16),
                         t2 = __builtin_amdgcn_alignbit(cur.z, cur.y, 16), t3 = __builtin_amdgcn_alignbit(cur.w, cur.z, 16),
                         t4 = __builtin_amdgcn_alignbit(next0, cur.w, 16);
          B[0][t] = __builtin_bit_cast(f16x8, (u32x4){t0, t1, t2, t3});
          B[1][t] = __builtin_bit_cast(f16x8, cur);
          B[2][t] = __builtin_bit_cast(f16x8, (u32x4){t1, t2, t3, t4});
        }
#define DVD_W3TERM(SA, SB)                                                                                  \
  _Pragma("unroll") for (int kx = 0; kx < 3; ++kx) acc[kx] =                                                \
      __builtin_amdgcn_mfma_f32_32x32x16_f16(A[SA], B[kx][SB], acc[kx], 0, 0, 0);
        if constexpr (!H16) {
          DVD_W3TERM(NTERM - 1, 0)
          DVD_W3TERM(0, NTERM - 1)
        }
        DVD_W3TERM(0, 0)
#undef DVD_W3TERM
        // the staging items i = s, s + NK, .. ride behind the MFMAs of K step s (for step r + 1 / r + 2, as in xwgrad3_kernel)
#pragma unroll
        for (int i = s; i < NQ; i += NK) {
          f_store(i, (r + 2) & 3, (r + 1) & 1, r + 1 < r1);      // gy row r + 1: the look-ahead past the last row is staged, not summed
          f_load(i, r + 2, true);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  float* dst = a.partial + (size_t)(a.slice0 + blockIdx.x) * 9 * a.G * a.Cout * a.Cin;        // partial[s][tap][G * Cout][Cin]
  const float unscale = H16 ? (a.out_scale ? a.out_scale[0] : 1.0f) : 1.0f / (sx * sg);
#pragma unroll
  for (int kx = 0; kx < 3; ++kx) {
    const int tap = ky * 3 + kx;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const int ci = ci0 + (lane & 31);
      if (co < a.Cout && ci < a.Cin) dst[((size_t)tap * a.G * a.Cout + grp * a.Cout + co) * a.Cin + ci] = acc[kx][r] * unscale;
    }
  }
  if constexpr (RSUM) {
    // the 16 lanes (run cells) of a channel row, in a fixed order; the operand scale is a power of two: unscaling is exact
    const float inv_sg = 1.0f / sg;
#pragma unroll
    for (int i = 0; i < NG; ++i) {
      float v = rs[i];
#pragma unroll
      for (int m = 1; m < GPR; m <<= 1) v += __shfl_xor(v, m, 64);
      if (isg[i] && (tid & (GPR - 1)) == 0 && blockIdx.y == 0 && f_ch[i] < a.Cout - co0)
        a.rowsum_partial[(size_t)(a.slice0 + blockIdx.x) * a.G * a.Cout + grp * a.Cout + co0 + f_ch[i]] = v * inv_sg;
    }
  }
}

// gw[co][ci][tap] = sum_s partial[s][tap][co][ci], ascending s (two interleaved chains); blocks from nmain on (RSUM launches):
// rowsum[c] = sum_s rpartial[s][c], ascending s, in double
__global__ __launch_bounds__(256) void xwgrad3_reduce_kernel(const float* __restrict__ partial, float* __restrict__ gw, int S,
                                                             int T, int Cout, int Cin, unsigned nmain,
                                                             const float* __restrict__ rpartial, float* __restrict__ rowsum,
                                                             int RC) {
  if (blockIdx.x >= nmain) {
    const int c = (int)(blockIdx.x - nmain) * 256 + threadIdx.x;
    if (c >= RC) return;
    double t = 0.0;
    int s = 0;
    for (; s + 16 <= S; s += 16) {                 // sixteen independent loads, then the adds in slice order
      float v[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = rpartial[(size_t)(s + j) * RC + c];
#pragma unroll
      for (int j = 0; j < 16; ++j) t += (double)v[j];
    }
    for (; s < S; ++s) t += (double)rpartial[(size_t)s * RC + c];
    rowsum[c] = (float)t;
    return;
  }
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;   // over [tap][co][ci]
  const long long per = (long long)T * Cout * Cin;
  if (i >= per) return;
  float s0 = 0.0f, s1 = 0.0f;
  int s = 0;
  for (; s + 1 < S; s += 2) {
    s0 += partial[(size_t)s * per + i];
    s1 += partial[(size_t)(s + 1) * per + i];
  }
  if (s < S) s0 += partial[(size_t)s * per + i];
  const int ci = (int)(i % Cin);
  const int co = (int)((i / Cin) % Cout);
  const int tap = (int)(i / ((long long)Cin * Cout));
  gw[((size_t)co * Cin + ci) * T + tap] = s0 + s1;
}

// ---- 1x1: dW[co][ci] = sum_{n, p} gy[n][co][p] * act(x)[n][ci][p] -- a plain "NT" GEMM with K = pixels contiguous in
// both operands.  A block owns 128 x 128 channels (8 waves: 4 x 2, one output-channel tile x two input-channel tiles
// each) and walks over chunks of 32 consecutive pixels of the flattened images; two blocks share a CU so that one
// block's staging (load, split, LDS write, barrier) overlaps the other's MFMAs.
constexpr int kW1Chunk = 32;
constexpr int kW1Pitch = 64 + 16;             // bytes per channel row in LDS (32 fp16 + pad)
constexpr int kW1CB = 128;
constexpr int kW1NT = 512;

template <bool H16>
__global__ __launch_bounds__(kW1NT, 2) void xwgrad1s_kernel(const Wg3Args a) {
  constexpr int EB = H16 ? 2 : 4;
  constexpr int NTERM = H16 ? 1 : 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem3[];
  unsigned char* sG = smem3;                               // [term 2][co 128][kW1Pitch]
  unsigned char* sX = smem3 + 2 * kW1CB * kW1Pitch;        // [term 2][ci 128][kW1Pitch]
  const float sx = H16 ? 1.0f : pow2_scale(a.x_amax[0]), sg = H16 ? 1.0f : pow2_scale(a.g_amax[0]);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pn = wave & 1, pm = wave >> 1;
  const int co0 = blockIdx.z * kW1CB, ci0 = blockIdx.y * kW1CB;
  const int HW = a.H * a.W;
  const size_t plane = (size_t)HW;
  const int cpi = (HW + kW1Chunk - 1) / kW1Chunk;          // chunks per image
  const int items = a.N * cpi;
  // staging: 128 channels x 8 quads per operand = 2048 quads -> 4 per thread (2 gy + 2 x)
  typename Quad<H16>::type stg[4];
  const bool hvec = (HW & 3) == 0;
  auto stage_load = [&](int item) {
    const int n = item / cpi, p0 = (item - n * cpi) * kW1Chunk;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = (i & 1) * kW1NT + tid;                 // 0 .. 1023
      const int ch = q >> 3, px = p0 + ((q & 7) << 2);
      const bool isx = i >= 2;
      const int C = isx ? a.Cin : a.Cout, c = (isx ? ci0 : co0) + ch;
      typename Quad<H16>::type v = zero_quad<H16>();
      if (c < C) {
        const unsigned char* p = static_cast<const unsigned char*>(isx ? a.x : a.gy) + ((size_t)n * C + c) * plane * EB;
        v = load_quad<H16>(p, px, HW, hvec && px + 3 < HW, isx && a.relu_in);
      }
      stg[i] = v;
    }
  };
  auto stage_store = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = (i & 1) * kW1NT + tid;
      const float sc = i >= 2 ? sx : sg;
      unsigned char* dst = (i >= 2 ? sX : sG) + (q >> 3) * kW1Pitch + ((q & 7) << 3);
      constexpr int tstride = kW1CB * kW1Pitch;
      store_quad<H16>(dst, tstride, stg[i], sc);
    }
  };
  f32x16 acc[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) acc[k] = (f32x16){0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int half = lane >> 5;
  const unsigned char* ga = sG + (pm * 32 + (lane & 31)) * kW1Pitch + half * 16;
  const unsigned char* xa = sX + (pn * 64 + (lane & 31)) * kW1Pitch + half * 16;

  int item = blockIdx.x;
  if (item < items) stage_load(item);
  for (; item < items; item += a.S) {
    __syncthreads();
    stage_store();
    __syncthreads();
    if (item + a.S < items) stage_load(item + a.S);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      f16x8 A[NTERM], B[2][NTERM];
#pragma unroll
      for (int t = 0; t < NTERM; ++t) {
        A[t] = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(ga + t * (kW1CB * kW1Pitch) + s * 32));
        B[0][t] = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(xa + t * (kW1CB * kW1Pitch) + s * 32));
        B[1][t] = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(xa + 32 * kW1Pitch + t * (kW1CB * kW1Pitch) + s * 32));
      }
#define DVD_W1TERM(SA, SB)                                                                                \
  _Pragma("unroll") for (int j = 0; j < 2; ++j) acc[j] =                                                  \
      __builtin_amdgcn_mfma_f32_32x32x16_f16(A[SA], B[j][SB], acc[j], 0, 0, 0);
      if constexpr (!H16) {
        DVD_W1TERM(NTERM - 1, 0)
        DVD_W1TERM(0, NTERM - 1)
      }
      DVD_W1TERM(0, 0)
#undef DVD_W1TERM
    }
  }
  float* dst = a.partial + (size_t)blockIdx.x * a.Cout * a.Cin;       // partial[s][co][ci]
  const float unscale = H16 ? (a.out_scale ? a.out_scale[0] : 1.0f) : 1.0f / (sx * sg);
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + pm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const int ci = ci0 + pn * 64 + j * 32 + (lane & 31);
      if (co < a.Cout && ci < a.Cin) dst[(size_t)co * a.Cin + ci] = acc[j][r] * unscale;
    }
}

// ---- 1x1, wide layers: one 512-thread workgroup owns 256 x 256 channels (the whole weight matrix of a ResNeXt stage-1 /
// decoder 1x1; a 256 x 256 block of the wider ones) for a run of 16-pixel chunks.  With 128 x 128 blocks each operand row
// is read by two workgroups and the kernel sits on the HBM roofline of that blocking (32 FLOP/B -> ~160 TF/s, measured
// 156-179); 256 x 256 halves the traffic.  The structure is the scene-flow MLP's weight-gradient kernel (csrc/sf_mlp.hip
// dw_body): 512 channel rows x 16 pixels are loaded as fp32, split and written to a double-buffered LDS stage while the
// MFMAs of the previous chunk run, one barrier per chunk, wave (wr, wc) keeps rows [64 wr, +64) x columns [128 wc, +128) in
// 128 accumulators.  Each slice writes its partial matrix; xwgrad3_reduce_kernel sums them in slice order (deterministic).
constexpr int kWbPitch = 48;                       // bytes per channel row of a 16-pixel chunk in LDS (32 + 16 pad)
constexpr int kWbTerm = 256 * kWbPitch;            // one split term of one operand
constexpr int kWbBuf = 2 * 2 * kWbTerm;            // gy terms, then x terms
constexpr size_t kWbLds = 2 * (size_t)kWbBuf;      // double buffered: 98 304

// FW (host: H * W a multiple of 16, so every 16-pixel chunk is whole): the staging loads are raw buffer loads (channel rows past
// the tensor fall out of the resource's range and read 0), a column tile's MFMAs are followed by the split + LDS store of ONE
// staging item and the request of the same item two chunks ahead -- round 3 ran `barrier | requests | all MFMAs | all splits`
// with both waves of a SIMD in the same phase (matrix pipe 37 % busy) and one chunk of latency cover for the HBM request.
// RSUM (fp32 FW only; host: a.rowsum_partial is set): the kernel also sums the gy rows it stages -- a thread stages the same two
// gy rows, tid >> 2 and 128 + (tid >> 2), for its whole slice, so f_store of the two gy items adds the item's four raw values
// behind the column tile's MFMAs, where it consumes the loaded registers for the split anyway (the scene-flow MLP's dw_body sums
// its bias gradient the same way).  The kernel has two registers to spare -- the plain FW form allocates 254 of the 256 VGPRs
// a wave of a 512-thread block may have; with one accumulator per row (two registers) this form spilled 19 -- so the four lanes
// of a row share ONE accumulator register for both rows (256 VGPRs, no scratch: one more live register here is a spill): the
// item's sum is folded across lanes q and q ^ 2 first, lanes 0 / 1 of a quad keep row tid >> 2, lanes 2 / 3 keep row
// 128 + (tid >> 2).  Chunks past the slice's end add zeros.  The blocks of input channel block 0 report;
// without RSUM the code is unchanged.
template <bool H16, bool FW, bool RSUM = false>
__global__ __launch_bounds__(512) void xwgrad1b_kernel(const Wg3Args a) {
  static_assert(!RSUM || (FW && !H16), "the channel sums exist in the fp32 FW form");
  constexpr int EB = H16 ? 2 : 4;
  constexpr int NTERM = H16 ? 1 : 2;
  float rs = 0.0f;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem3[];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = w >> 1, wc = w & 1;
  const int i32 = lane & 31, hh = lane >> 5;
  const int co0 = blockIdx.z * 256, ci0 = blockIdx.y * 256, s = blockIdx.x;
  const int HW = a.H * a.W;
  const size_t plane = (size_t)HW;
  const int cpi = (HW + 15) / 16;                              // 16-pixel chunks per image
  const long long items = (long long)a.N * cpi;
  const long long t0 = items * s / a.S, t1 = items * (s + 1) / a.S;
  const int n_it = (int)(t1 - t0);
  const float sx = H16 ? 1.0f : pow2_scale(a.x_amax[0]), sg = H16 ? 1.0f : pow2_scale(a.g_amax[0]);

  f32x16 acc[2][4];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = (f32x16){0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

  // staging: 512 rows x 4 quads of 4 pixels -> 4 float4 per thread; q = i * 512 + tid, row = q >> 2 (0..255 gy, 256..511 x)
  // (16-byte staging items for fp16 rows, as in xwgrad3_kernel, were tried here too: 3-10 % slower on the 1x1 shapes; not kept)
  typedef typename Quad<H16>::type QT;
  QT sg0[4], sg1[4];
  auto stage_load = [&](int it, QT (&st)[4]) {
    const long long item = t0 + it;
    const int n = (int)(item / cpi), p0 = (int)(item - (long long)n * cpi) * 16;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = i * 128 + (tid >> 2), quad = tid & 3;
      const bool isx = i >= 2;
      const int r = row & 255;
      const int C = isx ? a.Cin : a.Cout, c = (isx ? ci0 : co0) + r;
      const int px = p0 + quad * 4;
      QT v = zero_quad<H16>();
      if (c < C && px < HW)                                      // HW % 4 == 0 (host): a quad is inside or outside as a whole
        v = load_quad<H16>(static_cast<const unsigned char*>(isx ? a.x : a.gy) + ((size_t)n * C + c) * plane * EB, px, HW, true,
                           isx && a.relu_in);
      st[i] = v;
    }
  };
  auto stage_store = [&](int buf, const QT (&st)[4]) {
    unsigned char* base = smem3 + buf * kWbBuf;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = i * 128 + (tid >> 2), quad = tid & 3;
      const float sc = i >= 2 ? sx : sg;
      unsigned char* dst = base + (i >= 2 ? 2 * kWbTerm : 0) + (row & 255) * kWbPitch + quad * 8;
      store_quad<H16>(dst, kWbTerm, st[i], sc);
    }
  };
  // Fragments of chunk it + 1 are read from LDS DURING the MFMAs of chunk it (the rolling prefetch of csrc/xconv.hip: one
  // 512-thread block per CU runs in lock step, so fragment reads placed right after the barrier leave the matrix pipe idle
  // while all eight waves queue on LDS): the gy fragments into a second register set, the x fragments of column tile c into
  // the registers that tile's MFMAs have just released.  Chunk it is therefore loaded during step it - 3, split and stored
  // during step it - 2 (into the buffer whose fragments were read during step it - 3), read during step it - 1.
  const unsigned char* gb0 = smem3 + (64 * wr + i32) * kWbPitch + hh * 16;
  const unsigned char* hb0 = smem3 + 2 * kWbTerm + (128 * wc + i32) * kWbPitch + hh * 16;
  u32x4 Bf[4][NTERM];
  auto read_a = [&](int buf, u32x4 (&A)[2][NTERM]) {
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int t = 0; t < NTERM; ++t) A[r][t] = *reinterpret_cast<const u32x4*>(gb0 + buf * kWbBuf + t * kWbTerm + r * 32 * kWbPitch);
  };
  auto read_b = [&](int buf, int c) {
#pragma unroll
    for (int t = 0; t < NTERM; ++t) Bf[c][t] = *reinterpret_cast<const u32x4*>(hb0 + buf * kWbBuf + t * kWbTerm + c * 32 * kWbPitch);
  };
  auto mfma_roll = [&](int nbuf, const u32x4 (&A)[2][NTERM], u32x4 (&An)[2][NTERM]) {    // MFMAs on (A, Bf); next fragments from nbuf
    read_a(nbuf, An);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#define DVD_WB_TERM(SA, SB)                                                                                   \
  _Pragma("unroll") for (int r = 0; r < 2; ++r) acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(           \
      __builtin_bit_cast(f16x8, A[r][SA]), __builtin_bit_cast(f16x8, Bf[c][SB]), acc[r][c], 0, 0, 0);
      if constexpr (!H16) {
        DVD_WB_TERM(NTERM - 1, 0)
        DVD_WB_TERM(0, NTERM - 1)
      }
      DVD_WB_TERM(0, 0)
#undef DVD_WB_TERM
      __builtin_amdgcn_sched_barrier(0);           // the reload stays behind this column tile's MFMAs
      read_b(nbuf, c);
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  if constexpr (FW) {
    if (n_it > 0) {
      const int nco = (a.Cout - co0) < 256 ? (a.Cout - co0) : 256, nci = (a.Cin - ci0) < 256 ? (a.Cin - ci0) : 256;
      // item i of a thread: channel row i * 128 + (tid >> 2) (0..255 gy, 256..511 x), quad tid & 3 of the chunk's 16 pixels
      int voff[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) voff[h] = ((h * 128 + (tid >> 2)) * (int)plane + (tid & 3) * 4) * EB;
      u32x4 f0[4], f1[4];                                              // fp16 rows: 8 bytes per item, in the low half
      const float relu_lo = a.relu_in ? 0.0f : -__builtin_inff();
      const unsigned relu_lo_h = a.relu_in ? 0u : 0xfc00fc00u;
      auto f_load = [&](int it, int i, u32x4 (&st)[4]) {
        // chunks past the slice's end read zeros (an offset beyond the range): the loop always runs whole pairs of chunks
        const bool live = it < n_it;
        const long long item = t0 + (live ? it : 0);
        const int n = (int)(item / cpi), p0 = (int)(item - (long long)n * cpi) * 16;     // wave-uniform
        const int vo = live ? voff[i & 1] : (int)0x80000000;
        const bool isx = i >= 2;
        const unsigned char* base = static_cast<const unsigned char*>(isx ? a.x : a.gy) +
                                    ((size_t)n * (isx ? a.Cin : a.Cout) + (isx ? ci0 : co0)) * plane * EB;
        const __amdgpu_buffer_rsrc_t srd = __builtin_amdgcn_make_buffer_rsrc(
            uniform_ptr(const_cast<unsigned char*>(base)), 0, (isx ? nci : nco) * (int)plane * EB, 0x00020000);
        if constexpr (H16) {
          const u32x2v v = __builtin_bit_cast(u32x2v, __builtin_amdgcn_raw_buffer_load_b64(srd, vo, p0 * EB, 0));
          st[i] = (u32x4){v[0], v[1], 0u, 0u};
        } else {
          st[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(srd, vo, p0 * EB, 0));
        }
      };
      auto f_store = [&](int buf, int i, const u32x4 (&st)[4]) {
        const bool isx = i >= 2;
        const int row = i * 128 + (tid >> 2), quad = tid & 3;
        unsigned char* dst = smem3 + buf * kWbBuf + (isx ? 2 * kWbTerm : 0) + (row & 255) * kWbPitch + quad * 8;
        if constexpr (H16) {
          unsigned v0 = st[i][0], v1 = st[i][1];
          if (isx) {
            const f16x2 lo = __builtin_bit_cast(f16x2, relu_lo_h);
            v0 = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(f16x2, v0), lo));
            v1 = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(f16x2, v1), lo));
          }
          *reinterpret_cast<uint2*>(dst) = make_uint2(v0, v1);
        } else {
          const float sc = isx ? sx : sg;
          const float lo = isx ? relu_lo : -__builtin_inff();
          if constexpr (RSUM) {
            if (!isx) {
              float t = (__uint_as_float(st[i][0]) + __uint_as_float(st[i][1])) + (__uint_as_float(st[i][2]) + __uint_as_float(st[i][3]));
              t += __uint_as_float(__builtin_amdgcn_mov_dpp(__float_as_uint(t), 0x4E, 0xf, 0xf, true));     // quad_perm [2, 3, 0, 1]
              rs += ((tid & 2) != 0) == ((i & 1) != 0) ? t : 0.0f;
            }
          }
          const float v0 = fmaxf(__uint_as_float(st[i][0]), lo) * sc, v1 = fmaxf(__uint_as_float(st[i][1]), lo) * sc;
          const float v2 = fmaxf(__uint_as_float(st[i][2]), lo) * sc, v3 = fmaxf(__uint_as_float(st[i][3]), lo) * sc;
          unsigned h0, l0, h1, l1;
          split_pair_f16(v0, v1, h0, l0);
          split_pair_f16(v2, v3, h1, l1);
          *reinterpret_cast<uint2*>(dst) = make_uint2(h0, h1);
          *reinterpret_cast<uint2*>(dst + kWbTerm) = make_uint2(l0, l1);
        }
      };
      // MFMAs of one chunk on (A, Bf), next fragments from nbuf; behind column tile c: item c of `st` is stored into buffer
      // sbuf (chunk `it_st`, requested two chunks ago) and requested again for chunk it_ld
      auto mfma_fw = [&](int nbuf, const u32x4 (&A)[2][NTERM], u32x4 (&An)[2][NTERM], int sbuf, u32x4 (&st)[4], int it_ld) {
        read_a(nbuf, An);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#define DVD_WB_TERM(SA, SB)                                                                                   \
  _Pragma("unroll") for (int r = 0; r < 2; ++r) acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(           \
      __builtin_bit_cast(f16x8, A[r][SA]), __builtin_bit_cast(f16x8, Bf[c][SB]), acc[r][c], 0, 0, 0);
          if constexpr (!H16) {
            DVD_WB_TERM(NTERM - 1, 0)
            DVD_WB_TERM(0, NTERM - 1)
          }
          DVD_WB_TERM(0, 0)
#undef DVD_WB_TERM
          read_b(nbuf, c);
          f_store(sbuf, c, st);
          f_load(it_ld, c, st);
          __builtin_amdgcn_sched_barrier(0);
        }
      };
#pragma unroll
      for (int i = 0; i < 4; ++i) f_load(0, i, f0);
#pragma unroll
      for (int i = 0; i < 4; ++i) f_load(1, i, f1);
#pragma unroll
      for (int i = 0; i < 4; ++i) f_store(0, i, f0);
#pragma unroll
      for (int i = 0; i < 4; ++i) f_load(2, i, f0);
#pragma unroll
      for (int i = 0; i < 4; ++i) f_store(1, i, f1);
#pragma unroll
      for (int i = 0; i < 4; ++i) f_load(3, i, f1);
      __syncthreads();
      u32x4 A0[2][NTERM], A1[2][NTERM];
      read_a(0, A0);
#pragma unroll
      for (int c = 0; c < 4; ++c) read_b(0, c);
      for (int it = 0; it < n_it; it += 2) {
        __syncthreads();                   // chunk it + 1 is complete in buffer 1; buffer 0 has been read by every wave
        mfma_fw(1, A0, A1, 0, f0, it + 4);                  // chunk it; chunk it + 2 -> buffer 0; request chunk it + 4
        __syncthreads();
        mfma_fw(0, A1, A0, 1, f1, it + 5);                         // chunk it + 1 (zeros past the end); it + 3 -> buffer 1
      }
    }
  } else
  if (n_it > 0) {
    const int last = n_it - 1;
    auto clamp = [&](int i) { return i < last ? i : last; };
    stage_load(0, sg0);
    stage_store(0, sg0);
    stage_load(clamp(1), sg0);
    stage_store(1, sg0);
    stage_load(clamp(2), sg0);
    __syncthreads();
    u32x4 A0[2][NTERM], A1[2][NTERM];
    read_a(0, A0);
#pragma unroll
    for (int c = 0; c < 4; ++c) read_b(0, c);
    for (int it = 0; it < n_it; it += 2) {
      __syncthreads();                     // chunk it + 1 is complete in buffer 1; buffer 0 has been read by every wave
      stage_load(clamp(it + 3), sg1);
      __builtin_amdgcn_sched_barrier(0);   // the loads stay above the MFMAs
      mfma_roll(1, A0, A1);                // chunk it
      stage_store(0, sg0);                 // chunk it + 2 (past the end: a copy of the last chunk into an idle buffer)
      __syncthreads();
      stage_load(clamp(it + 4), sg0);
      __builtin_amdgcn_sched_barrier(0);
      if (it + 1 < n_it) mfma_roll(0, A1, A0);   // chunk it + 1
      stage_store(1, sg1);                 // chunk it + 3
    }
  }
  float* dst = a.partial + (size_t)s * a.Cout * a.Cin;       // partial[s][co][ci]
  const float unscale = H16 ? (a.out_scale ? a.out_scale[0] : 1.0f) : 1.0f / (sx * sg);
#pragma unroll
  for (int rr = 0; rr < 2; ++rr)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + 64 * wr + 32 * rr + (r & 3) + 8 * (r >> 2) + 4 * hh, ci = ci0 + 128 * wc + 32 * c + i32;
        if (co < a.Cout && ci < a.Cin) dst[(size_t)co * a.Cin + ci] = acc[rr][c][r] * unscale;
      }
  if constexpr (RSUM) {
    // lanes q and q ^ 1 hold the two halves of a row's sum
    const float v = rs + __uint_as_float(__builtin_amdgcn_mov_dpp(__float_as_uint(rs), 0xB1, 0xf, 0xf, true));   // quad_perm [1, 0, 3, 2]
    const int co = co0 + (tid & 2) * 64 + (tid >> 2);
    if ((tid & 1) == 0 && blockIdx.y == 0 && co < a.Cout) a.rowsum_partial[(size_t)s * a.Cout + co] = v;
  }
}

// out[c] = sum over images and pixels of g[n][c][:]: one block per channel, fixed order (per-thread strided partial sums, then
// a fixed tree).  What the row-sum entry points fall back to where no RSUM kernel serves the shape.  (Summing the gy rows inside
// round 3's xwgrad1b_kernel cost that kernel 10 % -- its staging sat ahead of all MFMAs; the FW form took it: DESIGN.md 7.1.)
__global__ __launch_bounds__(256) void chansum_kernel(const float* __restrict__ g, int N, int C, int HW, float* __restrict__ out) {
  const int c = blockIdx.x;
  float v = 0.0f;
  for (int n = 0; n < N; ++n) {
    const float* p = g + ((size_t)n * C + c) * HW;
    for (int i = threadIdx.x; i < HW; i += 256) v += p[i];
  }
  __shared__ float red[4];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) out[c] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- host.  wg_route decides which kernel serves a shape, with which launches and how much workspace; the size queries,
// dvd_xwgrad_rowsum_in_kernel and the one launch path (xwgrad_impl) read its answer and decide nothing themselves.
enum WgFamily { kWg3, kWg3g, kWgK, kWg1s, kWg1b };       // xwgrad3_ / xwgrad3g_ / xwgradk_ / xwgrad1s_ / xwgrad1b_kernel

struct WgRoute {
  WgFamily fam;
  bool fw;                 // xwgrad3_kernel / xwgrad1b_kernel: the FW instantiation
  bool rsum;               // the kernel has an RSUM form for this storage: it can deliver the row sums of gy itself
  int KS, G, Cin, Cout;    // kernel size, groups, channels per group
  int flop_class, nthreads;
  Wg3Plan p;               // channel blocks (grid y, z / G) and LDS bytes; the walking kernels: their plan (wg3_plan.h)
  int nl;                  // launches ...
  WgClass L[2];            // ... and what each walks (the 1x1 kernels: one launch, only S counts)
  int S;                   // the partial slices the launches write in all
  size_t floats[2];        // what a size query answers for the route: workspace floats without / with the per-slice row sums
};

// the launches of a layer: one per cost class of the plan, or the one launch of the round-robin deal (dvd_xwgrad_select(3))
static int wg_launches(const Wg3Plan& p, WgClass (&L)[2], int& slices) {
  if (g_w3_deal) {
    L[0] = WgClass{0, p.nstrips, 4, p.S, 0};
    slices = p.S;
    return 1;
  }
  for (int c = 0; c < p.ncls; ++c) L[c] = p.cls[c];
  slices = p.Stot;
  return p.ncls;
}

// Channel counts are totals over the G groups; false: no kernel for the shape (KS other than 1, 3, 5, 7, 11; groups only for 3x3).
// force: the route under dvd_xwgrad_select(1) / (2) whatever is selected now (0: as selected).
static bool wg_route(int KS, int N, int Cin_total, int Cout_total, int H, int W, int G, bool h16, WgRoute& r, int force = 0) {
  if (N <= 0 || Cin_total <= 0 || Cout_total <= 0 || H <= 0 || W <= 0 || G <= 0 || Cin_total % G || Cout_total % G) return false;
  if (G > 1 && KS != 3) return false;
  const bool narrow1 = force == 1 || g_w1_variant == 1;     // hook value 1: always the 128 x 128 blocks
  const bool round3 = force == 2 || g_w3_variant == 1;      // hook value 2: no FW instantiation, no 32 x 32 blocks
  const int Cin = Cin_total / G, Cout = Cout_total / G;
  const long long HW = (long long)H * W;
  // a buffer resource spans `rows` channel rows of one image: they must lie within 31 bits
  auto in_range = [&](int rows) { return rows * HW * (h16 ? 2 : 4) < (1ll << 31); };
  r = WgRoute{};
  r.KS = KS; r.G = G; r.Cin = Cin; r.Cout = Cout;
  if (KS == 1) {
    // the 256 x 256 blocks when both channel counts fill them reasonably and rows are float4 aligned
    const bool wide = Cin >= 192 && Cout >= 192 && (HW & 3) == 0 && !narrow1;
    r.fam = wide ? kWg1b : kWg1s;
    r.fw = wide && HW % 16 == 0 && in_range(256) && !round3;      // whole 16-pixel chunks
    r.rsum = r.fw && !h16;
    const int cb = wide ? 256 : kW1CB, chunk = wide ? 16 : kW1Chunk;
    r.p.nco = (Cout + cb - 1) / cb;
    r.p.nci = (Cin + cb - 1) / cb;
    r.p.lds = wide ? kWbLds : (size_t)2 * 2 * kW1CB * kW1Pitch;
    r.nthreads = wide ? 512 : kW1NT;
    r.flop_class = wide ? DVD_FLOP_XWGRAD1B : DVD_FLOP_XWGRAD1S;
    // whole rounds over the resident blocks: one 256 x 256 block per CU (one round over the 256 CUs), two 128 x 128 blocks
    // per CU (two rounds over 512 slots)
    const int pairs = r.p.nco * r.p.nci, slots = wide ? 256 : 512, blocks = wide ? 256 : 1024;
    const int rounds = pairs >= slots ? 1 : (blocks + pairs - 1) / pairs;
    const long long items = (long long)N * ((HW + chunk - 1) / chunk);
    r.S = rounds > items ? (int)items : rounds;
    r.nl = 1;
    r.L[0] = WgClass{0, 0, 4, r.S, 0};
    // (the size query answers for the count before the clamp by the items, as it always has)
    for (int i = 0; i < 2; ++i) r.floats[i] = (size_t)rounds * Cout * Cin + (i ? (size_t)rounds * Cout : 0);
    return true;
  }
  if (KS == 3) {
    // 32 x 32 channel blocks of three waves (xwgrad3g_kernel): grouped layers with at most 32 channels per group on both sides;
    // rows of fp16 elements must start dword-aligned for its buffer loads (even widths)
    const bool small = G > 1 && Cin <= kWgCB && Cout <= kWgCB && !round3 && (!h16 || W % 2 == 0) && in_range(32);
    r.fam = small ? kWg3g : kWg3;
    if (small) wg3g_plan(N, Cin, Cout, H, W, G, r.p);
    else wg3_plan(N, Cin, Cout, H, W, G, r.p);
    // whole 16-byte staging items: the branch-free row step
    r.fw = !small && (!h16 || W % 2 == 0) && in_range(64) && !round3;
    r.rsum = small && !h16;
    r.nthreads = small ? kWgNT : kW3NT;
    r.flop_class = small ? DVD_FLOP_XWGRAD3G : DVD_FLOP_XWGRAD3;
  } else {
    if (!wgk_plan(N, Cin, Cout, H, W, KS, h16, r.p)) return false;
    r.fam = kWgK;
    r.nthreads = 64 * KS;
    r.flop_class = DVD_FLOP_XWGRADK;
  }
  r.nl = wg_launches(r.p, r.L, r.S);
  for (int i = 0; i < 2; ++i) r.floats[i] = wg_partial_floats(r.p, KS * KS, Cout_total, Cin, i != 0);
  return true;
}

// What a size query answers: the largest workspace over the routes a launch may take -- the query does not know the storage
// (fp32 or fp16), and the hook may be set between the query and the launch.  0: no kernel for the shape.
static size_t wg_query_bytes(int KS, int N, int Cin_total, int Cout_total, int H, int W, int G, bool rowsum) {
  size_t n = 0;
  for (int force = 0; force < 3; ++force)
    for (int h16 = 0; h16 < 2; ++h16) {
      WgRoute r;
      if (!wg_route(KS, N, Cin_total, Cout_total, H, W, G, h16 != 0, r, force)) return 0;
      if (r.floats[rowsum] > n) n = r.floats[rowsum];
    }
  return n * sizeof(float);
}

static void wg_args_class(Wg3Args& a, const Wg3Plan& p, const WgClass& c) {
  a.nstrips = p.nstrips; a.RS = p.RS; a.nrseg = p.nrseg;
  a.strip0 = c.strip0; a.ncols = c.ncols; a.S = c.S; a.slice0 = c.slice0;
  a.deal = g_w3_deal ? 1 : 0;
}
// f(std::integral_constant<int, NK>) for the run-time K-step count nk
template <class F>
static int wg_with_nk(int nk, F&& f) {
  switch (nk) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    default: return f(std::integral_constant<int, 4>{});
  }
}

typedef void (*WgKernel)(const Wg3Args);

// The instantiation key of a launch: what wg_kernels() switches on and dvd_xwgrad_describe reports.  nk: the NK template
// argument, 0 where the instantiation has none to choose (the guarded row step of xwgrad3_kernel keeps four K steps, the dead
// ones over zeros; the 1x1 kernels).  fw / rsum: the FW / RSUM template arguments (false where the family has no such form).
struct WgKey {
  WgFamily fam;
  int KS;
  bool h16, fw, rsum;
  int nk;
};
// rsum: the caller wants the row sums AND the route has an RSUM form (gy_rowsum && r.rsum)
static WgKey wg_key(const WgRoute& r, bool h16, bool rsum, int nk) {
  WgKey k{r.fam, r.KS, h16, false, false, 0};
  nk = nk >= 1 && nk <= 3 ? nk : 4;
  switch (r.fam) {
    case kWg3:
      k.fw = r.fw;
      k.nk = r.fw ? nk : 0;
      break;
    case kWg3g:
      k.rsum = rsum && !h16;
      k.nk = nk;
      break;
    case kWgK:
      k.nk = nk;
      break;
    case kWg1b:
      k.fw = r.fw;
      k.rsum = rsum && r.fw && !h16;
      break;
    case kWg1s:
      break;
  }
  return k;
}

// The instantiation of a key.  11x11 runs two, kernel columns 0 .. 5 and 6 .. 10: disjoint taps of the same partials.
static void wg_kernels(const WgKey& key, WgKernel (&k)[2]) {
  k[0] = k[1] = nullptr;
  const bool h16 = key.h16;
  switch (key.fam) {
    case kWg3:
      if (!key.fw) {
        if (h16) k[0] = xwgrad3_kernel<true, false>;
        else k[0] = xwgrad3_kernel<false, false>;
        break;
      }
      wg_with_nk(key.nk, [&](auto nkc) -> int {
        constexpr int NK = decltype(nkc)::value;
        if (h16) k[0] = xwgrad3_kernel<true, true, NK>;
        else k[0] = xwgrad3_kernel<false, true, NK>;
        return 0;
      });
      break;
    case kWg3g:
      wg_with_nk(key.nk, [&](auto nkc) -> int {
        constexpr int NK = decltype(nkc)::value;
        if (h16) k[0] = xwgrad3g_kernel<true, false, NK>;
        else if (key.rsum) k[0] = xwgrad3g_kernel<false, true, NK>;
        else k[0] = xwgrad3g_kernel<false, false, NK>;
        return 0;
      });
      break;
    case kWgK: {
      auto pick = [&](auto h, auto nkc) -> int {
        constexpr bool H16 = decltype(h)::value;
        constexpr int NK = decltype(nkc)::value;
        if (key.KS == 5) k[0] = xwgradk_kernel<H16, 5, 0, 5, NK>;
        else if (key.KS == 7) k[0] = xwgradk_kernel<H16, 7, 0, 7, NK>;
        else k[0] = xwgradk_kernel<H16, 11, 0, 6, NK>, k[1] = xwgradk_kernel<H16, 11, 6, 5, NK>;
        return 0;
      };
      wg_with_nk(key.nk, [&](auto nkc) -> int { return h16 ? pick(std::true_type{}, nkc) : pick(std::false_type{}, nkc); });
      break;
    }
    case kWg1b:
      if (h16 && key.fw) k[0] = xwgrad1b_kernel<true, true>;
      else if (h16) k[0] = xwgrad1b_kernel<true, false>;
      else if (key.rsum) k[0] = xwgrad1b_kernel<false, true, true>;
      else if (key.fw) k[0] = xwgrad1b_kernel<false, true>;
      else k[0] = xwgrad1b_kernel<false, false>;
      break;
    case kWg1s:
      if (h16) k[0] = xwgrad1s_kernel<true>;
      else k[0] = xwgrad1s_kernel<false>;
      break;
  }
}

// What an entry point does for a shape, storage and row-sum request under the current hook: the route, whether the kernel sums
// the gy rows itself, and the workspace the launches need.  xwgrad_impl launches from it, dvd_xwgrad_describe reports it.
struct WgCall {
  WgRoute r;
  bool rsum;               // the kernel sums the rows it stages (the RSUM form)
  bool chansum;            // row sums wanted on a route without one: the chansum_kernel pass
  size_t per, npart, need; // floats of one partial slice, of all slices; workspace bytes
};
static bool wg_call(int KS, int N, int Cin_total, int Cout_total, int H, int W, int groups, bool h16, bool want_rowsum, WgCall& c) {
  if (!wg_route(KS, N, Cin_total, Cout_total, H, W, groups, h16, c.r)) return false;
  c.rsum = want_rowsum && c.r.rsum;
  c.chansum = want_rowsum && !c.rsum;
  c.per = (size_t)KS * KS * Cout_total * c.r.Cin;
  c.npart = (size_t)c.r.S * c.per;
  c.need = (c.npart + (c.rsum ? (size_t)c.r.S * Cout_total : 0)) * sizeof(float);
  return true;
}
// bytes an operand's base address must be a multiple of: the kernels read rows (1x1: planes) in the widest items their length
// allows -- 16 bytes where a row is whole 16-byte items, 8 / 4 where it is whole 8- / 4-byte ones, single elements otherwise
static size_t wg_operand_align(int KS, int H, int W, bool h16) {
  const long long row = (KS == 1 ? (long long)H * W : (long long)W) * (h16 ? 2 : 4);
  return row % 16 == 0 ? 16 : row % 8 == 0 ? 8 : row % 4 == 0 ? 4 : 2;
}

static int wg_launch(WgKernel kern, const WgRoute& r, const Wg3Args& a, hipStream_t s) {
  DVD_HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)r.p.lds));
  hipLaunchKernelGGL(kern, dim3(a.S, r.p.nci, r.p.nco * r.G), dim3(r.nthreads), r.p.lds, s, a);
  DVD_LAUNCH_OK();
  return DVD_OK;
}

// Every entry point: the checks, the route, its launches, the reduction over the slices.  kxk: the 5x5 / 7x7 / 11x11 entry points.
// gy_rowsum (fp32 only, may be null): receives the per-channel sums of gy -- from the weight-gradient kernel itself where the
// route has an RSUM form, else from chansum_kernel.
static int xwgrad_impl(int KS, bool kxk, const void* x, const float* x_amax, const void* gy, const float* gy_amax, float* gw,
                       void* workspace, size_t workspace_bytes, int N, int Cin_total, int Cout_total, int H, int W, int groups,
                       int relu_in, bool h16, const float* out_scale, float* gy_rowsum, dvd_stream_t stream) {
  const char* name = kxk ? "xwgradk" : KS == 1 ? "xwgrad1s" : "xwgrad3";
  DVD_REQUIRE(x && gy && gw && workspace, "%s: null pointer", name);
  DVD_REQUIRE(h16 || (x_amax && gy_amax), kxk ? "%s: null pointer" : "%s: the operands' max|.| scalars are missing (dvd_amax)", name);
  DVD_REQUIRE(N > 0 && Cin_total > 0 && Cout_total > 0 && H > 0 && W > 0, "%s: bad shape", name);
  DVD_REQUIRE(groups > 0 && Cin_total % groups == 0 && Cout_total % groups == 0, "%s: %d groups do not divide the channels", name, groups);
  DVD_REQUIRE((long long)H * W * (long long)(Cin_total > Cout_total ? Cin_total : Cout_total) < (1ll << 31),
              "%s: image too large for 32-bit offsets", name);
  DVD_REQUIRE(!(h16 && gy_rowsum), "%s: the channel sums exist for fp32 gradients", name);
  WgCall c;
  DVD_REQUIRE((!kxk || KS > 3) && wg_call(KS, N, Cin_total, Cout_total, H, W, groups, h16, gy_rowsum != nullptr, c),
              "%s: kernel size %d (5, 7 and 11 are covered)", name, KS);
  const WgRoute& r = c.r;
  const bool rsum = c.rsum;                                          // the kernel sums the rows it stages
  const size_t per = c.per, npart = c.npart, need = c.need;
  const size_t al = wg_operand_align(KS, H, W, h16);
  DVD_REQUIRE((reinterpret_cast<size_t>(x) | reinterpret_cast<size_t>(gy)) % al == 0,
              "%s: x and gy must be %zu-byte aligned for rows of %d elements", name, al, KS == 1 ? H * W : W);
  DVD_REQUIRE((reinterpret_cast<size_t>(gw) | reinterpret_cast<size_t>(workspace) | reinterpret_cast<size_t>(gy_rowsum)) % sizeof(float) == 0,
              "%s: gw, the row sums and the workspace must be 4-byte aligned", name);
  if (workspace_bytes < need) {
    set_error("%s: workspace %zu < %zu bytes", name, workspace_bytes, need);
    return DVD_ENOSPC;
  }
  DVD_REQUIRE((long long)r.p.nco * groups <= 65535 && r.p.nci <= 65535, "%s: too many channel blocks", name);
  Wg3Args a;
  a.x = x;
  a.gy = gy;
  a.x_amax = x_amax;
  a.g_amax = gy_amax;
  a.out_scale = out_scale;
  a.partial = static_cast<float*>(workspace);
  a.rowsum_partial = rsum ? a.partial + npart : nullptr;
  a.N = N; a.Cin = r.Cin; a.Cout = r.Cout; a.H = H; a.W = W;
  a.G = groups; a.nco = r.p.nco;
  a.relu_in = relu_in ? 1 : 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  flops_add(r.flop_class, 2.0 * (KS * KS) * N * (double)Cout_total * r.Cin * (double)H * W);
  for (int l = 0; l < r.nl; ++l) {
    wg_args_class(a, r.p, r.L[l]);
    WgKernel k[2];
    wg_kernels(wg_key(r, h16, rsum, r.L[l].nk), k);
    for (int j = 0; j < 2 && k[j]; ++j)
      if (int e = wg_launch(k[j], r, a, s)) return e;
  }
  const unsigned nmain = (unsigned)((per + 255) / 256), nrs = rsum ? (unsigned)((Cout_total + 255) / 256) : 0u;
  hipLaunchKernelGGL(xwgrad3_reduce_kernel, dim3(nmain + nrs), dim3(256), 0, s, a.partial, gw, r.S, KS * KS, Cout_total, r.Cin, nmain,
                     a.rowsum_partial, gy_rowsum, Cout_total);
  DVD_LAUNCH_OK();
  if (c.chansum) {                               // no RSUM kernel on this route: one fixed-order pass over gy
    hipLaunchKernelGGL(chansum_kernel, dim3(Cout_total), dim3(256), 0, s, static_cast<const float*>(gy), N, Cout_total, H * W, gy_rowsum);
    DVD_LAUNCH_OK();
  }
  return DVD_OK;
}
}  // namespace dvd

extern "C" {

// the dW partials, then the row-sum partials of dvd_xwgrad3_rowsum / dvd_xwgrad1s_rowsum: [S][Cout]
size_t dvd_xwgrad3_workspace_bytes(int N, int Cin, int Cout, int H, int W, int groups) {
  return dvd::wg_query_bytes(3, N, Cin, Cout, H, W, groups, true);
}
size_t dvd_xwgrad1s_workspace_bytes(int N, int Cin, int Cout, int H, int W) { return dvd::wg_query_bytes(1, N, Cin, Cout, H, W, 1, true); }
// 5x5 / 7x7 / 11x11
size_t dvd_xwgradk_workspace_bytes(int N, int Cin, int Cout, int H, int W, int KS) {
  return KS > 3 ? dvd::wg_query_bytes(KS, N, Cin, Cout, H, W, 1, false) : 0;
}

int dvd_xwgrad_rowsum_in_kernel(int N, int Cin, int Cout, int H, int W, int KS, int groups) {
  dvd::WgRoute r;
  return (KS == 1 || KS == 3) && dvd::wg_route(KS, N, Cin, Cout, H, W, groups, false, r) && r.rsum ? 1 : 0;
}

int dvd_xwgrad_describe(int KS, int N, int Cin_total, int Cout_total, int H, int W, int groups, int in_f16, int with_rowsum,
                        int* out) {
  DVD_REQUIRE(out, "xwgrad_describe: null pointer");
  // the row sums exist for the fp32 1x1 and 3x3 entry points; groups other than 1 only for 3x3 (wg_route refuses them too)
  DVD_REQUIRE(!(with_rowsum && (in_f16 || KS > 3)), "xwgrad_describe: no row sums for fp16 gradients or %dx%d kernels", KS, KS);
  dvd::WgCall c;
  DVD_REQUIRE(dvd::wg_call(KS, N, Cin_total, Cout_total, H, W, groups, in_f16 != 0, with_rowsum != 0, c),
              "xwgrad_describe: no weight-gradient kernel for this shape");
  for (int i = 0; i < DVD_WDESC_INTS; ++i) out[i] = 0;
  const dvd::WgRoute& r = c.r;
  dvd::WgKey key{};
  for (int l = 0; l < r.nl; ++l) {
    key = dvd::wg_key(r, in_f16 != 0, c.rsum, r.L[l].nk);
    int* o = out + DVD_WDESC_L0 + l * DVD_WDESC_L_INTS;
    o[DVD_WDESC_L_NK] = r.L[l].nk;
    o[DVD_WDESC_L_KEY_NK] = key.nk;
    o[DVD_WDESC_L_S] = r.L[l].S;
    o[DVD_WDESC_L_SLICE0] = r.L[l].slice0;
    o[DVD_WDESC_L_STRIP0] = r.L[l].strip0;
    o[DVD_WDESC_L_NCOLS] = r.L[l].ncols;
  }
  dvd::WgKernel k[2];
  dvd::wg_kernels(key, k);
  out[DVD_WDESC_FAMILY] = (int)key.fam;
  out[DVD_WDESC_KS] = key.KS;
  out[DVD_WDESC_H16] = key.h16 ? 1 : 0;
  out[DVD_WDESC_FW] = key.fw ? 1 : 0;
  out[DVD_WDESC_RSUM] = key.rsum ? 1 : 0;
  out[DVD_WDESC_LAUNCHES] = r.nl;
  out[DVD_WDESC_SECOND] = k[1] ? 1 : 0;
  out[DVD_WDESC_NCO] = r.p.nco;
  out[DVD_WDESC_NCI] = r.p.nci;
  out[DVD_WDESC_LDS_BYTES] = (int)r.p.lds;
  out[DVD_WDESC_THREADS] = r.nthreads;
  out[DVD_WDESC_SLICES] = r.S;
  out[DVD_WDESC_WS_BYTES_LO] = (int)(c.need & 0x7fffffffu);
  out[DVD_WDESC_WS_BYTES_HI] = (int)(c.need >> 31);
  out[DVD_WDESC_CHANSUM] = c.chansum ? 1 : 0;
  out[DVD_WDESC_DEAL] = dvd::g_w3_deal && KS != 1 ? 1 : 0;
  out[DVD_WDESC_ALIGN] = (int)dvd::wg_operand_align(KS, H, W, in_f16 != 0);
  return DVD_OK;
}

int dvd_xwgrad_select(int variant) {
  DVD_REQUIRE(variant >= 0 && variant <= 3, "xwgrad_select: variant %d", variant);
  dvd::g_w1_variant = variant == 1 ? 1 : 0;
  dvd::g_w3_variant = variant == 2 ? 1 : 0;
  dvd::g_w3_deal = variant == 3 ? 1 : 0;
  return DVD_OK;
}

int dvd_xwgrad3(const float* x, const float* x_amax, const float* gy, const float* gy_amax, float* gw, void* workspace,
                size_t workspace_bytes, int N, int Cin_total, int Cout_total, int H, int W, int groups, int relu_in,
                dvd_stream_t stream) {
  return dvd::xwgrad_impl(3, false, x, x_amax, gy, gy_amax, gw, workspace, workspace_bytes, N, Cin_total, Cout_total, H, W, groups,
                          relu_in, false, nullptr, nullptr, stream);
}

int dvd_xwgrad3_rowsum(const float* x, const float* x_amax, const float* gy, const float* gy_amax, float* gw, float* gy_rowsum,
                       void* workspace, size_t workspace_bytes, int N, int Cin_total, int Cout_total, int H, int W, int groups,
                       int relu_in, dvd_stream_t stream) {
  return dvd::xwgrad_impl(3, false, x, x_amax, gy, gy_amax, gw, workspace, workspace_bytes, N, Cin_total, Cout_total, H, W, groups,
                          relu_in, false, nullptr, gy_rowsum, stream);
}

int dvd_xwgrad3_h(const void* x, const void* gy, const float* out_scale, float* gw, void* workspace, size_t workspace_bytes, int N,
                  int Cin_total, int Cout_total, int H, int W, int groups, int relu_in, dvd_stream_t stream) {
  return dvd::xwgrad_impl(3, false, x, nullptr, gy, nullptr, gw, workspace, workspace_bytes, N, Cin_total, Cout_total, H, W, groups,
                          relu_in, true, out_scale, nullptr, stream);
}

int dvd_xwgradk(const float* x, const float* x_amax, const float* gy, const float* gy_amax, float* gw, void* workspace,
                size_t workspace_bytes, int N, int Cin, int Cout, int H, int W, int KS, int relu_in, dvd_stream_t stream) {
  return dvd::xwgrad_impl(KS, true, x, x_amax, gy, gy_amax, gw, workspace, workspace_bytes, N, Cin, Cout, H, W, 1, relu_in, false,
                          nullptr, nullptr, stream);
}

int dvd_xwgradk_h(const void* x, const void* gy, const float* out_scale, float* gw, void* workspace, size_t workspace_bytes, int N,
                  int Cin, int Cout, int H, int W, int KS, int relu_in, dvd_stream_t stream) {
  return dvd::xwgrad_impl(KS, true, x, nullptr, gy, nullptr, gw, workspace, workspace_bytes, N, Cin, Cout, H, W, 1, relu_in, true,
                          out_scale, nullptr, stream);
}

int dvd_xwgrad1s(const float* x, const float* x_amax, const float* gy, const float* gy_amax, float* gw, void* workspace,
                 size_t workspace_bytes, int N, int Cin, int Cout, int H, int W, int relu_in, dvd_stream_t stream) {
  return dvd::xwgrad_impl(1, false, x, x_amax, gy, gy_amax, gw, workspace, workspace_bytes, N, Cin, Cout, H, W, 1, relu_in, false,
                          nullptr, nullptr, stream);
}

int dvd_xwgrad1s_rowsum(const float* x, const float* x_amax, const float* gy, const float* gy_amax, float* gw, float* gy_rowsum,
                        void* workspace, size_t workspace_bytes, int N, int Cin, int Cout, int H, int W, int relu_in,
                        dvd_stream_t stream) {
  return dvd::xwgrad_impl(1, false, x, x_amax, gy, gy_amax, gw, workspace, workspace_bytes, N, Cin, Cout, H, W, 1, relu_in, false,
                          nullptr, gy_rowsum, stream);
}

int dvd_xwgrad1s_h(const void* x, const void* gy, const float* out_scale, float* gw, void* workspace, size_t workspace_bytes, int N,
                   int Cin, int Cout, int H, int W, int relu_in, dvd_stream_t stream) {
  return dvd::xwgrad_impl(1, false, x, nullptr, gy, nullptr, gw, workspace, workspace_bytes, N, Cin, Cout, H, W, 1, relu_in, true,
                          out_scale, nullptr, stream);
}

}  // extern "C"

