/*
 * dvd_hip.h -- C ABI of libdvd_hip.so, the MI355X (gfx950) kernels behind the
 * dynamic-video-depth test-time-optimisation inner loop.
 *
 * The reference (google/dynamic-video-depth) has NO native boundary: its
 * operator API is Python classes.  Each entry point below therefore names the
 * reference Python interface it replaces (file:line under /root/reference) and
 * is what the host-side mirror in dynamic-video-depth_amd/dvd_hip binds with
 * ctypes (INTEGRATION.md shows the stub a reference maintainer would add).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 unless noted;
 *     the caller (PyTorch's caching allocator) owns all memory, the library
 *     never allocates or frees; scratch is passed in (`*_workspace_bytes`).
 *   - all work is enqueued on `stream` (a hipStream_t) and returns at once.
 *   - return value: DVD_OK or a negative dvd_status; text via dvd_last_error()
 *     (thread local).  Nothing throws across the ABI.
 *   - tensors: depth [B,1,H,W]; flow [B,H,W,2] (x then y, pixels);
 *     mask [B,H,W]; scene flow / world points planar [B,3,H,W] unless a
 *     `*_interleaved` ([B,H,W,3]) variant is named; camera blocks as in the
 *     reference data files: row-vector convention, matrices stored transposed,
 *     each [B,3,3] or [B,3] (SURVEY.md section 8 header;
 *     scripts/preprocess/davis/generate_sequence_midas.py:69-76).
 */
#ifndef DVD_HIP_H
#define DVD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVD_ABI_VERSION 8

typedef void* dvd_stream_t; /* hipStream_t */

typedef enum dvd_status {
  DVD_OK = 0,
  DVD_EINVAL = -1, /* bad shape / null pointer / unsupported option */
  DVD_EHIP = -2,   /* a HIP runtime call failed; see dvd_last_error() */
  DVD_ENOSPC = -3  /* workspace too small */
} dvd_status;

int dvd_abi_version(void);
const char* dvd_last_error(void);
/* Static properties the host needs for sizing (CU count etc.). */
int dvd_device_cu_count(void);

/* Algorithmic work (2 x multiply-accumulates) the matrix kernels were LAUNCHED with since the last reset, per kernel class --
 * the class is the template the dispatcher picked, so a profiler trace's per-kernel time and this table join on the kernel
 * name (bench.py `roofline_mfma`, tools/mfma_roofline.py).  Counted on the host at launch / graph-capture time; a replayed
 * graph does not count again.  Measurement aid with no counterpart in the reference; out[i] = class i, n <= DVD_FLOP_CLASSES. */
enum {
  DVD_FLOP_XCONV_1X1_WIDE = 0, /* xconv_kernel<4,2,2,2,FitOne>: 1x1, >= 256 rows, one position tile per block row       */
  DVD_FLOP_XCONV_WIDE = 1,     /* xconv_kernel<4,2,2,{2,4},*>: >= 256 output rows per group (3x3 and larger, other 1x1)   */
  DVD_FLOP_XCONV_128 = 2,      /* xconv_kernel<2,2,2,2,*>: 128 x 128 blocks                                                */
  DVD_FLOP_XCONV_SMALL = 3,    /* xconv_kernel<{1,2},2,1,4,*>: <= 64 rows per group (grouped 3x3 of ResNeXt, thin layers)  */
  DVD_FLOP_XWGRAD3 = 4,        /* xwgrad3_kernel: dense 3x3 weight gradient                                                */
  DVD_FLOP_XWGRAD3G = 5,       /* xwgrad3g_kernel: grouped 3x3 weight gradient                                             */
  DVD_FLOP_XWGRAD1B = 6,       /* xwgrad1b_kernel: wide 1x1 weight gradient                                                */
  DVD_FLOP_XWGRAD1S = 7,       /* xwgrad1s_kernel: other 1x1 weight gradients                                              */
  DVD_FLOP_XWGRADK = 8,        /* xwgradk_kernel: 5x5 / 7x7 / 11x11 weight gradients                                       */
  DVD_FLOP_MLP_FWD = 9,        /* mlp_fwd_kernel                                                                           */
  DVD_FLOP_MLP_DX = 10,        /* mlp_bwd_dx_kernel                                                                        */
  DVD_FLOP_MLP_DW = 11,        /* mlp_bwd_dw_kernel                                                                        */
  DVD_FLOP_CLASSES = 12
};
int dvd_flop_counters(double* out, int n, int reset);
/* The same accounting for the memory-bound helper kernels of a step (ABI 7; bench.py's roofline_helpers): every launch adds the
 * bytes it must move -- each operand tensor read once, each result written once -- to its class.  out[i] = class i. */
enum {
  DVD_BYTES_BNRELU_FWD = 0, /* bnrelu_fwd_kernel: x (+ residual) in, y out                                                       */
  DVD_BYTES_BNRELU_BWD = 1, /* bnrelu_bwd kernels: gy, y / x in, gx (+ g_residual) out, per-channel sums                          */
  DVD_BYTES_UPSAMPLE_FWD = 2, /* bilinear up-sampling and the bicubic resize, forward                                         */
  DVD_BYTES_UPSAMPLE_BWD = 3, /* ... and their backward                                                                        */
  DVD_BYTES_AMAX = 4,       /* amax_kernel: one read of the tensor                                                                */
  DVD_BYTES_PACK = 5,       /* weight maximum + fragment packing of the convolution weights                                       */
  DVD_BYTES_POOL = 6,       /* max-pool of the stem, forward and backward                                                         */
  DVD_BYTES_GCONV = 7,      /* grouped 3x3 with 8 channels per group on the vector unit (ResNeXt stage 1), all three passes       */
  DVD_BYTES_ELEMENTWISE = 8,/* scale_add, mul_mask, acc_reg, cast_scale, depth head                                               */
  DVD_BYTES_ADAM = 9,       /* the fused optimiser step: param, grad(s), optimiser state in, param and state out (Adam or SGD)     */
  DVD_BYTES_GEOMETRY = 10,  /* unproject forward / backward                                                                       */
  DVD_BYTES_GATHER = 11,    /* dvd_gather_pairs: every tensor of the table read once and written once, + the permutation          */
  DVD_BYTES_CLASSES = 12
};
int dvd_byte_counters(double* out, int n, int reset);

/* Camera block of a batch of frame pairs (the eight tensors the reference
 * forwards take by name: losses/scene_flow_projection.py:114,222). */
typedef struct dvd_cameras {
  const float* R_1;   /* [B,3,3] cam1->world, stored transposed   */
  const float* R_2;   /* [B,3,3] cam2->world, stored transposed   */
  const float* R_1_T; /* [B,3,3] world->cam1                       */
  const float* R_2_T; /* [B,3,3] world->cam2                       */
  const float* t_1;   /* [B,3] camera centre 1 (world)             */
  const float* t_2;   /* [B,3]                                     */
  const float* K;     /* [B,3,3] intrinsics^T                      */
  const float* K_inv; /* [B,3,3] (intrinsics^-1)^T                 */
} dvd_cameras;

/* ------------------------------------------------------------------------
 * unproject: depth -> world points.
 * Replaces unproject_ptcld.forward (losses/scene_flow_projection.py:54-67)
 * and the `global_p1` half of flow_by_depth.forward (:127-131).
 * out_planar != 0: [B,3,H,W] (what the scene-flow MLP consumes,
 * models/scene_flow_motion_field.py:245); else [B,H,W,3].
 * bwd: g_depth (+)= (g_points @ R_1^T) . ray ;  accumulate != 0 adds. */
int dvd_unproject_fwd(const float* depth, const float* R, const float* t, const float* K_inv,
                      float* points, int out_planar, int B, int H, int W, dvd_stream_t stream);
int dvd_unproject_bwd(const float* g_points, int planar, const float* R, const float* K_inv,
                      const float* scale_or_null, float* g_depth, int accumulate,
                      int B, int H, int W, dvd_stream_t stream);

/* ------------------------------------------------------------------------
 * Fused warp + reprojection + masked losses, forward AND backward in one
 * launch (the HBM-bound kernel of BASELINE.json).
 * Replaces, for the training step, the chain
 *   flow_by_depth.forward            losses/scene_flow_projection.py:114-153
 *   scene_flow_projection_slack.fwd  losses/scene_flow_projection.py:222-278
 *   F.grid_sample (bilinear, border) losses/scene_flow_projection.py:112,220
 *   Model._calc_loss / disp_loss     models/scene_flow_motion_field.py:140-150,285-324
 * and their autograd backward.
 *
 * sums[0..3] (device) receive  S0=sum m, S1=sum m*flow_err, S2=sum m*disp_err,
 * S3=sum m*sf_err  (un-normalised; deterministic two-stage reduction).
 * Gradients are written UN-NORMALISED, i.e. as if the loss were
 *   flow_mul*S1 + disp_mul*(use_disp ? S2 : S3);
 * the global 1/(S0+1e-8) (after the data-parallel all-reduce of the sums,
 * SURVEY.md section 8e) is applied by the consumers through a device scalar
 * (dvd_loss_finalize writes it).  g_depth_2 (bilinear scatter) is accumulated in Q31.32 fixed point in the LDS
 * windows of the tiles (ds_add_u64: integer adds commute, so the result is bitwise reproducible), cells only one
 * window covers are stored directly, the halo ring is summed over the <= 4 overlapping windows in a fixed order; only
 * taps that leave a window (|flow - pair mean| > 8 px) go through a record list and global fp32 atomics.  No memset of
 * g_depth_2 is needed. */
typedef struct dvd_warp_cfg {
  int B, H, W;
  int midas_mask;  /* 1: m *= [depth_1<100]*[W2.z<100]   (model:286-289)        */
  int crit_l2;     /* 1: squared flow error (warm phase, model:291), 0: L1      */
  int disp_mode;   /* 0:|z1-z2|  1:use_disp  2:use_disp_ratio  (model:140-150)  */
  int loss_on_sf;  /* 1: second loss term is sf_loss (not use_disp, model:310)  */
  float flow_mul;  /* already multiplied by `steps` when --weight_steps         */
  float disp_mul;
} dvd_warp_cfg;

size_t dvd_warp_loss_workspace_bytes(int B, int H, int W);
/* Test hook (process wide; not an environment switch): variant 0 = production -- since ABI 7 the strip kernel
 * (csrc/warp_strip.hip) for a backward call with the shipped flag set and W % 4 == 0 at tile = -1, the tiled LDS
 * kernel otherwise; 1 = reference variant with global gathers + hardware atomics; 2 = the tiled LDS kernel of rounds 2-5
 * whatever the call; tile = -1 (auto) or an index of the tile-shape table.  The third argument is RESERVED: pass 0.  It used
 * to choose 2 or 4 pixels per thread-step; that number is fixed by the tile shape now, and any other value is rejected
 * (DVD_EINVAL).  Every combination computes the same function. */
int dvd_warp_loss_select(int variant, int tile, int reserved);
/* Test hook (ABI 7): rows = image rows per unit of the strip kernel -- 0 = chosen from the shape and the device's block slots,
 * else a multiple of the shape's step height, at least two steps (more, shorter units: more seams between units); shape = 0
 * (production: 96-column strips in 32-row steps, 12 rows of vertical halo, 768-thread blocks), 1 (64 x 16, 512 threads),
 * 2 (96 x 16, 384 threads), 3 (as 0 with 8 rows of vertical halo).
 * dvd_warp_loss_workspace_bytes follows both. */
int dvd_warp_loss_strip_select(int rows, int shape);
int dvd_warp_loss_fused(const dvd_warp_cfg* cfg, const float* depth_1, const float* depth_2,
                        const float* flow_1_2, const float* mask_2, const float* sf_1_2,
                        const dvd_cameras* cams, void* workspace, size_t workspace_bytes,
                        float* sums /*[4]*/, float* g_depth_1, float* g_depth_2, float* g_sf_1_2,
                        dvd_stream_t stream);
/* Forward only (validation / logging): same sums, no gradients. */
int dvd_warp_loss_fwd(const dvd_warp_cfg* cfg, const float* depth_1, const float* depth_2,
                      const float* flow_1_2, const float* mask_2, const float* sf_1_2,
                      const dvd_cameras* cams, void* workspace, size_t workspace_bytes,
                      float* sums, dvd_stream_t stream);
/* scalars[0]=1/(S0+1e-8) [1]=loss [2]=flow_loss [3]=disp_loss [4]=sf_loss
 * [5]=S0; reads sums after the caller's (optional) all-reduce. */
int dvd_loss_finalize(const dvd_warp_cfg* cfg, const float* sums, float* scalars /*[8]*/,
                      dvd_stream_t stream);

/* ------------------------------------------------------------------------
 * Scene-flow field MLP (fused; fp16 matrix cores on two-term split, power-of-two scaled operands = fp32-class accuracy).
 * Replaces SceneFlowFieldNet.forward (networks/sceneflow_field.py:43-53):
 *   PeriodicEmbed of t and xyz (networks/blocks.py:19-34), 1x1 conv C_in->256,
 *   4 x (256->256), each + LeakyReLU(0.2), then 256->3 (blocks.py:50-102),
 * the division by sf_mag_div and one Euler step of
 * Model.forward_sf_net_multi_step (models/scene_flow_motion_field.py:346-367),
 * and their autograd backward.  Width 256 / 4 hidden layers are what the
 * reference Model builds (scene_flow_motion_field.py:107).
 *
 * Pixels are processed in tiles of 64; `n_pix` = B*H*W, p/sf tensors are planar
 * [B,3,H,W] (pix_per_img = H*W), t is [B,1,H,W].
 * Weights are the reference state_dict tensors convs.{0..5}.conv.{weight,bias}
 * (weight [out,in] row-major); dvd_sf_mlp_pack re-orders them into MFMA
 * fragment order (both orientations) inside `packed`.
 * `stash` (forward, optional) receives the embedding, the five hidden
 * activations (fp32, [channel][64 pixels] rows per tile) and one sign bit per
 * hidden unit, 5.72 KB per pixel; the backward kernels consume it. */
typedef struct dvd_mlp_desc {
  int n_freq_xyz;      /* 16 */
  int n_freq_t;        /* 16; ignored if !time_dependent */
  int time_dependent;  /* 1: input = [embed(t), embed(xyz)] */
  const float* freqs_xyz; /* device [n_freq_xyz] = linspace(1, n+1, n) as torch computes it */
  const float* freqs_t;   /* device [n_freq_t] */
  int stash_f16;          /* ABI 4: 1 = the five hidden activations of the stash are stored as _Float16 (3.2 KB per pixel instead of
                           * 5.7): the weight-gradient kernel then contracts fp32 gradients (two terms) against fp16 activations (one
                           * term, 2 MFMAs per product).  Losses and the input gradient do not depend on it. */
  float* fwd_monitor;     /* ABI 7, with stash_f16: a device float (slot [6] of the loss-scale state, dvd_gscale_*) that every
                           * stashing forward folds max |hidden activation| into (NaN counted as +Inf) -- an activation beyond
                           * fp16's range is stored as Inf and poisons the weight gradients: the step's guard skips it.  Or null. */
} dvd_mlp_desc;

/* Test / A-B hook (process wide, ABI 6): waves per workgroup of the forward / dX kernels.  4 (default) = two 256-thread
 * workgroups per CU, each wave two 32-channel row tiles; 8 = one 512-thread workgroup per CU (rounds 2-4).  Outputs, stashes
 * and input gradients are BIT-identical between the two (same products, same order); 0 = back to the default. */
int dvd_sf_mlp_select(int waves_per_workgroup);
int dvd_sf_mlp_in_channels(const dvd_mlp_desc* d);             /* 132 for the shipped config */
size_t dvd_sf_mlp_packed_bytes(const dvd_mlp_desc* d);
size_t dvd_sf_mlp_stash_bytes(const dvd_mlp_desc* d, long long n_pix);
size_t dvd_sf_mlp_gstash_bytes(long long n_pix);
int dvd_sf_mlp_pack(const dvd_mlp_desc* d, const float* const W[6], const float* const b[6],
                    void* packed, dvd_stream_t stream);
/* sf = MLP(p, t + t_offset) * out_scale;  optional fused Euler bookkeeping:
 * p_next = p + sf (may alias nothing), acc (in/out) += sf.  Any of sf_out,
 * p_next, acc may be null. */
int dvd_sf_mlp_fwd(const dvd_mlp_desc* d, const void* packed, const float* p, const float* t,
                   float t_offset, float out_scale, long long n_pix, int pix_per_img,
                   float* sf_out, float* p_next, float* acc, void* stash, dvd_stream_t stream);
/* Backward w.r.t. the input points and all pre-activations:
 *   g_out = gscale * (scale_ptr ? *scale_ptr : 1) * g_out1 + (g_out2 ? g_out2 : 0)
 *   g_p   = J^T (out_scale * g_out)  + (g_p_add ? g_p_add : 0)
 * writes the pre-activation gradients of layers 0..4 to `gstash` and
 * ACCUMULATES the last layer's dW (gW5 [3,256]) and db (gb5 [3]): per-workgroup shares (in the weight-gradient
 * workspace at the end of `gstash`, which must have dvd_sf_mlp_gstash_bytes(n_pix)) summed in fixed order by a second
 * kernel, one atomic add per element and call -- bitwise reproducible from call to call. */
int dvd_sf_mlp_bwd_dx(const dvd_mlp_desc* d, const void* packed, const void* stash, float out_scale,
                      const float* g_out1, float gscale, const float* scale_ptr, const float* g_out2,
                      const float* g_p_add, long long n_pix, int pix_per_img, float* g_p, void* gstash,
                      float* gW5, float* gb5, dvd_stream_t stream);
/* dW_l += G_l . H_{l-1}^T and db_l += rowsum(G_l) for l = 0..4 (accumulating; per-workgroup partial
 * matrices in the tail of `gstash`, summed in fixed order: bitwise reproducible), gW[l] in the
 * reference layout [out,in]. */
int dvd_sf_mlp_bwd_dw(const dvd_mlp_desc* d, const void* stash, void* gstash, long long n_pix,
                      float* const gW[5], float* const gb[5], dvd_stream_t stream);

/* ------------------------------------------------------------------------
 * Elementwise helpers of the step.
 * dvd_scale_add: out = scale * (scale_ptr ? *scale_ptr : 1) * a + (b ? b : 0).
 *   Applies the late 1/(sum(mask)+1e-8) of Model._calc_loss
 *   (models/scene_flow_motion_field.py:297-306) from a device scalar.
 * dvd_acc_reg: the elementwise half of Model._opt_reg (:326-344):
 *   g_sf1 = coef * sign(sf1 - sf0),  abs_sum (+)= sum |sf1 - sf0|   (coef = acc_mul/(3N+1e-6)).
 * dvd_adam_step: torch.optim.Adam step (:113-115,212-213; betas from
 *   options/options_train.py:84-87) on a flat buffer with grad = s*grad1 + grad2. */
int dvd_scale_add(float* out, const float* a, float scale, const float* scale_ptr, const float* b,
                  long long n, dvd_stream_t stream);
/* The tail of the MiDaS depth head in one pass each way (ABI 7): depth = 10000 / clamp(relu(v), min = 1e-2) of
 * third_party/MiDaS.py:192-195,240-242 -- as torch evaluates it: reciprocal, then x 10000 (bit-identical); backward
 * g_v = -(g_depth * 10000) / v^2 where v >= 1e-2, else 0 (autograd's formula with clamp's mask).  16-byte aligned pointers, any n. */
int dvd_depth_tail_fwd(const float* v, float* depth, long long n, dvd_stream_t stream);
int dvd_depth_tail_bwd(const float* v, const float* g_depth, float* g_v, long long n, dvd_stream_t stream);
/* out[b,c,p] = a[b,c,p] * mask[b,p]: `sf_1_2 *= motion_seg_1` of --use_motion_seg
 * (models/scene_flow_motion_field.py:253-254) and the matching gradient mask; out may alias a. */
int dvd_mul_mask(float* out, const float* a, const float* mask, int B, int C, long long HW, dvd_stream_t stream);
size_t dvd_acc_reg_workspace_bytes(void);
int dvd_acc_reg(const float* sf0, const float* sf1, float coef, float* g_sf1, void* workspace,
                float* abs_sum, int accumulate, long long n, dvd_stream_t stream);
int dvd_adam_step(float* param, const float* grad1, float scale, const float* scale_ptr,
                  const float* grad2, float* exp_avg, float* exp_avg_sq, long long n, float lr,
                  float beta1, float beta2, float eps, int step, dvd_stream_t stream);

/* ------------------------------------------------------------------------
 * Per-pixel surfaces of the warp modules (forward values; the training gradient path is
 * dvd_warp_loss_fused, which never materialises them).  Replaces, for visualisation / export /
 * inference callers (models/scene_flow_motion_field.py:215-225, models/video_base.py:105-126),
 *   flow_by_depth.forward                losses/scene_flow_projection.py:114-153
 *   scene_flow_projection_slack.forward  losses/scene_flow_projection.py:222-278
 * Every output is optional (NULL = not wanted).  3-vectors are interleaved [B,H,W,3] (the
 * reference's [B,H,W,1,3]), flows [B,H,W,2], depths [B,1,H,W].  sflow_1_2 is the reference's
 * interleaved scene flow [B,H,W,(1,)3] or NULL for zero.  Same fp32 operation order as the
 * reference, so index masks and tap indices are bit-identical to its CPU path. */
typedef struct dvd_surfaces {
  float* global_p1;          /* P1 = (d1 (x,y,1) K_inv) R_1 + t_1                      (:127-131,235-237) */
  float* warped_global_p2;   /* bilinear sample of frame 2's world points at the flow target (:133-135) */
  float* sf_by_depth;        /* warped_global_p2 - global_p1                              (:136)         */
  float* staticflow_1_2;     /* rigid-scene flow (= flow_by_depth's dflow_1_2)           (:138-149,267) */
  float* dflow_1_2;          /* flow of the scene-flow-advected point                     (:244-265)     */
  float* depth_image_1_2;    /* z of the advected point in image 2                        (:268)         */
  float* depth_warp_1_2;     /* bilinear sample of depth_2                                (:274-276)     */
  float* p1_camera_2;        /* (P1 + sflow - t_2) R_2_T                                  (:244)         */
  float* warped_p2_camera_2; /* bilinear sample of frame 2's camera-space points          (:240-242)     */
} dvd_surfaces;
int dvd_warp_surfaces(const float* depth_1, const float* depth_2, const float* flow_1_2, const float* sflow_1_2,
                      const dvd_cameras* cams, const dvd_surfaces* out, int B, int H, int W, dvd_stream_t stream);
/* Vector-Jacobian product of dvd_warp_surfaces: g_surfaces holds the upstream gradient of every surface that has one
 * (NULL = none), in the surface's layout; writes d/d depth_1, d/d depth_2 (zeroed inside; the flow is data, so the taps
 * are a scatter-add) and, if not NULL, d/d sflow_1_2.  This is the autograd backward of the reference's module forms
 * flow_by_depth / scene_flow_projection_slack (losses/scene_flow_projection.py:114-153,222-278), including the gradient
 * cut at behind-camera pixels (:253-263). */
int dvd_warp_surfaces_bwd(const float* depth_1, const float* depth_2, const float* flow_1_2, const float* sflow_1_2,
                          const dvd_cameras* cams, const dvd_surfaces* g_surfaces, float* g_depth_1, float* g_depth_2,
                          float* g_sflow_1_2, int B, int H, int W, dvd_stream_t stream);

/* Stand-alone flow warp: BackwardWarp.forward (losses/scene_flow_projection.py:281-307) =
 * F.grid_sample(buffer, (x,y)+flow, bilinear, padding_mode='border', align_corners=True) on
 * buffer [B,C,H,W]; bwd = its gradient w.r.t. the buffer (bilinear scatter-add; g_buffer is
 * zeroed inside the call). */
int dvd_flow_warp_fwd(const float* buffer, const float* flow_1_2, float* out, int B, int C, int H, int W,
                      dvd_stream_t stream);
int dvd_flow_warp_bwd(const float* g_out, const float* flow_1_2, float* g_buffer, int B, int C, int H, int W,
                      dvd_stream_t stream);

/* ------------------------------------------------------------------------
 * Grouped 3x3 convolution, 8 channels per group, stride 1, pad 1, NCHW fp32.
 * Replaces the `conv2` of the ResNeXt-101 32x8d stage-1 bottlenecks inside the MiDaS encoder
 * (third_party/midas_blocks.py:35-50 -> torchvision ResNet(Bottleneck, groups=32,
 * width_per_group=8): stage 1 is 256 channels = 32 groups x 8) -- forward, backward-data and
 * backward-weight of nn.Conv2d(C, C, 3, padding=1, groups=C/8, bias=False).
 * x, y, gy, gx: [N,C,H,W]; w, gw: [C,8,3,3].  bwd_weight needs a workspace
 * (per-tile partial sums, reduced in a fixed order: deterministic); accumulate != 0 adds into gw. */
int dvd_gconv3x3_c8_fwd(const float* x, const float* w, float* y, int N, int C, int H, int W,
                        dvd_stream_t stream);
int dvd_gconv3x3_c8_bwd_data(const float* gy, const float* w, float* gx, int N, int C, int H, int W,
                             dvd_stream_t stream);
size_t dvd_gconv3x3_c8_wgrad_workspace_bytes(int N, int C, int H, int W);
int dvd_gconv3x3_c8_bwd_weight(const float* x, const float* gy, float* gw, int accumulate, void* workspace,
                               size_t workspace_bytes, int N, int C, int H, int W, dvd_stream_t stream);

/* The same convolution with the eval-mode BatchNorm + ReLU site behind it inside the kernels (fp32 storage; additions within
 * ABI 8), so that no pre-BN tensor and no pass of csrc/bnrelu.hip exists for the layer.  s = gamma / sqrt(var + eps).
 *   bn_fwd:        y = max(0, conv(x, w) * s + (beta - mean * s)); max|y| is folded into y_amax (optional, zeroed by the caller).
 *   bn_bwd_data:   gx = conv_transpose(g * s, w) for the masked, UNSCALED gradient g = gy * [y > 0]; mask_src (optional, the
 *                  layer's saved input): gx *= [mask_src > 0]; max|gx| is folded into gx_amax (optional, zeroed by the caller).
 *   bn_bwd_weight: gw = the weight gradient of the unscaled g (dvd_convbn_finalize derives dW, dgamma from it) and
 *                  g_chansum[c] = sum_{n,p} g[n][c][p] (dbeta), both summed in a fixed order (deterministic). */
int dvd_gconv3x3_c8_bn_fwd(const float* x, const float* w, const float* gamma, const float* beta, const float* mean,
                           const float* var, float eps, float* y, float* y_amax, int N, int C, int H, int W,
                           dvd_stream_t stream);
int dvd_gconv3x3_c8_bn_bwd_data(const float* g, const float* w, const float* gamma, const float* var, float eps,
                                const float* mask_src, float* gx, float* gx_amax, int N, int C, int H, int W,
                                dvd_stream_t stream);
size_t dvd_gconv3x3_c8_bn_wgrad_workspace_bytes(int N, int C, int H, int W);
int dvd_gconv3x3_c8_bn_bwd_weight(const float* x, const float* g, float* gw, float* g_chansum, void* workspace,
                                  size_t workspace_bytes, int N, int C, int H, int W, dvd_stream_t stream);

/* Same convolution with 32 channels per group (fp32 MFMA): the stride-1 bottlenecks of ResNeXt
 * stage 3 (width 1024 = 32 groups x 32).  w, gw: [C,32,3,3].  All three entry points take a workspace
 * of dvd_gconv3x3_c32_workspace_bytes (fragment-ordered weights for fwd / bwd_data, per-block
 * partial sums for bwd_weight). */
size_t dvd_gconv3x3_c32_workspace_bytes(int N, int C, int H, int W);
int dvd_gconv3x3_c32_fwd(const float* x, const float* w, float* y, void* workspace, size_t workspace_bytes, int N,
                         int C, int H, int W, dvd_stream_t stream);
int dvd_gconv3x3_c32_bwd_data(const float* gy, const float* w, float* gx, void* workspace, size_t workspace_bytes,
                              int N, int C, int H, int W, dvd_stream_t stream);
int dvd_gconv3x3_c32_bwd_weight(const float* x, const float* gy, float* gw, int accumulate, void* workspace,
                                size_t workspace_bytes, int N, int C, int H, int W, dvd_stream_t stream);

/* ------------------------------------------------------------------------
 * Fused eval-mode BatchNorm (+ residual add) (+ ReLU), NCHW fp32.  Replaces
 * relu(bn(x)) / relu(bn3(x) + skip) of the ResNeXt bottlenecks of the MiDaS encoder (torchvision
 * resnet.py Bottleneck via third_party/midas_blocks.py:35-50); the depth nets are in eval mode while
 * training (models/scene_flow_motion_field.py:157,168), so running statistics are used and gamma/beta
 * still get gradients.  y = max(0, x*s[c] + b[c] (+ residual)), s = gamma/sqrt(var+eps), b = beta - mean*s.
 * bwd: gx = g*s, g_residual = g, g_beta = sum g, g_gamma = sum g*(x-mean)/sqrt(var+eps), g = gy*[y>0];
 * any of gx, g_residual, g_gamma, g_beta may be NULL; channel sums are deterministic (two stages).  g_amax (optional):
 * device scalar into which max|g| is folded (atomic max; zero it first) -- the operand scale of the gradient kernels
 * that consume g (dvd_xconv_fwd / dvd_xwgrad*). */
int dvd_bnrelu_fwd(const float* x, const float* residual, const float* gamma, const float* beta, const float* mean,
                   const float* var, float eps, float* y, int N, int C, int HW, int relu, dvd_stream_t stream);
size_t dvd_bnrelu_bwd_workspace_bytes(int N, int C, int HW);
int dvd_bnrelu_bwd(const float* gy, const float* y, const float* x, const float* gamma, const float* mean,
                   const float* var, float eps, float* gx, float* g_residual, float* g_gamma, float* g_beta,
                   void* workspace, size_t workspace_bytes, int N, int C, int HW, int relu, float* g_amax, dvd_stream_t stream);

/* ------------------------------------------------------------------------
 * Bilinear up-sampling of [planes, H_in, W_in] -> [planes, H_out, W_out] (planes = N*C) and its backward.
 * Replaces F.interpolate(mode='bilinear') of the MiDaS decoder: align_corners=True at the end of every
 * FeatureFusionBlock (third_party/midas_blocks.py:164-166), align_corners=False in the output head
 * (midas_blocks.py:71-99, MiDaS.py:190).  Same source-index / weight formulas as ATen. */
int dvd_upsample_bilinear_fwd(const float* x, float* y, long long planes, int H_in, int W_in, int H_out, int W_out,
                              int align_corners, dvd_stream_t stream);
int dvd_upsample_bilinear_bwd(const float* gy, float* gx, long long planes, int H_in, int W_in, int H_out,
                              int W_out, int align_corners, dvd_stream_t stream);

/* ------------------------------------------------------------------------
 * Bicubic resize of fp32 planes [planes, H_in, W_in] -> [planes, H_out, W_out] with align_corners=True, and its backward
 * (additive in ABI 8).  Replaces the two F.interpolate(mode='bicubic', align_corners=True) calls of a MidasNet with a working
 * resolution: third_party/MiDaS.py:221-222 (image -> working size) and :244-245 (depth -> frame size).  ATen's
 * upsample_bicubic2d arithmetic in fp32 (A = -0.75, taps clamped at the border).  Any sizes, 1 included.
 * fwd: mean / std are device pointers to `channels` floats, or both NULL; when set every tap is normalised first,
 * (x - mean[c]) / std[c] with c = plane % channels -- the input normalisation of MiDaS.py:213-218 fused into the resize.
 * bwd: gx = A^T gy as a gather in a fixed order (no atomics: bit-identical from call to call); the image needs no gradient,
 * so there is no normalised form.  workspace: dvd_bicubic_bwd_workspace_bytes(...) bytes, written before it is read. */
int dvd_bicubic_fwd(const float* x, float* y, long long planes, int H_in, int W_in, int H_out, int W_out, const float* mean,
                    const float* std, int channels, dvd_stream_t stream);
size_t dvd_bicubic_bwd_workspace_bytes(long long planes, int H_in, int W_in, int H_out, int W_out);
int dvd_bicubic_bwd(const float* gy, float* gx, long long planes, int H_in, int W_in, int H_out, int W_out, void* workspace,
                    size_t workspace_bytes, dvd_stream_t stream);

/* ------------------------------------------------------------------------
 * max|x| of a tensor into a device scalar: out[0] = max(out[0], max|x|) (atomic; zero `out` first, or pass a running
 * bound).  The matrix kernels derive the power-of-two scale of their fp16 operand split from such scalars on the device;
 * nothing reads them on the host.  x: any 4-byte aligned address (a misaligned head is read by scalar loads). */
int dvd_amax(const float* x, long long n, float* out, dvd_stream_t stream);

/* out[c] = sum over n, p of x[n][c][p] of an NCHW fp32 tensor (HW pixels per plane) -- the bias gradient of a convolution,
 * conv.py _XConv.backward (the reference leaves it to autograd: torch.nn.Conv2d(bias=True), third_party/midas_blocks.py) --
 * and, when amax_out is not NULL, amax_out[0] = max(amax_out[0], max|x|) from the same read (dvd_amax's contract).
 * Deterministic: fixed summation order.  workspace: dvd_chansum_workspace_bytes(N, C) bytes of device memory. */
size_t dvd_chansum_workspace_bytes(int N, int C);
int dvd_chansum(const float* x, int N, int C, long long HW, float* out, float* amax_out, void* workspace, size_t workspace_bytes,
                dvd_stream_t stream);

/* ------------------------------------------------------------------------
 * Dense stride-1 "same" convolution (odd k x k up to 11, any channel counts), NCHW fp32, on the 16-bit
 * matrix cores with every fp32 operand, scaled by a power of two, split into two fp16 terms (three partial
 * products, fp32 accumulation: fp32-class accuracy, csrc/dvd_split.h, csrc/xconv.hip).  Replaces the dense
 * nn.Conv2d forward and backward-data of the depth networks:
 *   third_party/midas_blocks.py:102-168 (ResidualConvUnit / FeatureFusionBlock 3x3),
 *   third_party/MiDaS.py:186-195 (scratch.layerK_rn, output_conv),
 *   third_party/midas_blocks.py:35-50 (1x1 convolutions of the ResNeXt-101 32x8d bottlenecks),
 *   third_party/hourglass.py:21-57 (1x1 / k x k inception branches).
 * dvd_xconv_pack re-orders w [Cout,Cin,k,k] into MFMA fragment order, already split (once per weight
 * update); transposed != 0 packs the backward-data operator (channel roles swapped, taps flipped), which
 * is then run by the same dvd_xconv_fwd with Cin/Cout exchanged.
 * dvd_xconv_fwd: y = act_out( conv(act_in(x)) + bias + res' ) * [mask_src > 0]
 *   flags bit0: act_in = ReLU on the input as it is staged (conv(relu(x)) of ResidualConvUnit),
 *         bit1: act_out = ReLU, bit2: res' = relu(residual) instead of residual;
 *   bias [Cout], residual / mask_src [N,Cout,H,W] may be NULL.  mask_src is the ReLU mask of the
 *   backward-data pass (gx = dgrad(gy) * [x > 0]).
 *   Stride 2 (3x3 kernels, nn.Conv2d(.., 3, stride=2, padding=1): torchvision's Bottleneck.conv2 at the entry of ResNeXt
 *   stages 2-4, reached through third_party/midas_blocks.py:35-50).  H x W are the dimensions of the FULL-resolution tensor:
 *         bit3: stride-2 forward -- x is [N,Cin,H,W], y (and residual / mask_src) [N,Cout,(H+1)/2,(W+1)/2]; the haloed input
 *               tile is staged in LDS as four phase planes, every tap stays one constant LDS offset;
 *         bit4: backward-data of that convolution -- x is the gradient [N,Cin,(H+1)/2,(W+1)/2] of the strided output (Cin =
 *               the convolution's output channels, weights packed transposed), y [N,Cout,H,W]; the kernel stages the
 *               gradient AS IF zero-interleaved (v[2i][2j] = g[i][j]): the interleaved tensor is never written to HBM. */
/* Channel counts are totals; groups > 1 = grouped convolution with weight [Cout][Cin / groups][k][k] (nn.Conv2d's
 * layout): the 64-channels-per-group 3x3 convolutions of ResNeXt stage 4 run here with groups = 32. */
size_t dvd_xconv_packed_bytes(int Cout, int Cin, int KS, int groups, int transposed);
int dvd_xconv_pack(const float* w, void* packed, int Cout, int Cin, int KS, int groups, int transposed, dvd_stream_t stream);
/* Eval-mode BatchNorm of the convolution's output fused into the epilogue (the depth nets are always in eval mode while
 * training, models/scene_flow_motion_field.py:157,168):  y = act((conv(x) + bias - mean) / sqrt(var + eps) * gamma + beta
 * + residual).  gamma / beta null = BatchNorm2d(affine=False) (hourglass.py:21-57).  bn null = no BatchNorm. */
typedef struct dvd_bn_params {
  const float* gamma;
  const float* beta;
  const float* mean;
  const float* var;
  float eps;
} dvd_bn_params;
/* x_amax: device scalar holding max|x| of the WHOLE input tensor, or an upper bound of it (written by dvd_amax or by the
 * producing kernel through its y_amax): the power-of-two operand scale of the two-term fp16 split is derived from it on the
 * device (csrc/dvd_split.h).  y_amax (optional): device scalar into which max|y| of this launch is folded with an atomic
 * max -- zero it (or pass a running bound) before the launch. */
int dvd_xconv_fwd(const float* x, const float* x_amax, const void* packed, const float* bias, const float* residual,
                  const float* mask_src, const dvd_bn_params* bn, float* y, float* y_amax, int N, int Cin, int Cout, int H,
                  int W, int KS, int groups, int flags, dvd_stream_t stream);
/* Test / A-B hook (process wide, like dvd_warp_loss_select): block shape of dvd_xconv_fwd for >= 256 output channels.
 * 0 = automatic (256 channels x 128 positions for 1x1 kernels, 256 x 256 for k >= 3), 1 = round 2's 128 x 128 blocks,
 * 2 / 3 = force 256 x 128 / 256 x 256, 4 = round 2's blocks on the generic pointer-addressed main loop (the path shapes
 * with Cin % 16 != 0 take), 5 = 128 x 128 blocks with one activation stage at three blocks per CU, 6 = 1x1 kernels without
 * their two-chunk loop, 7 = 1x1 kernels with the narrow (dword) epilogue instead of the LDS-transposed 16-byte one,
 * 8 = automatic block shapes with the GEMM columns of a k x k tile on the cells of the HALOED tile and the tile choice that
 * goes with it (rounds 2-6; 0-7 compute the tile's outputs only, csrc/xconv_tile.h, which also names the one launch that
 * stays on haloed positions in every setting).
 * Results are identical in every setting (same products, same K order). */
int dvd_xconv_select(int cfg);
/* What dvd_xconv_fwd (in_f16 = out_f16 = 0) / dvd_xconv_fwd_h (in_f16 = 1) would launch for these arguments, under the current
 * dvd_xconv_select value: pure host code, no HIP call, usable without a GPU.  Returns what the launch would return for the
 * shape (DVD_EINVAL with the same message for what it refuses; pointers and N are not its business).  operands_aligned16:
 * whether y, residual and mask_src all sit at 16-byte aligned addresses (null counts as aligned).  out receives
 * DVD_XDESC_INTS ints, indexed by the constants below.  The launch code switches on the same decision (csrc/xconv.hip,
 * XDecision): this is the dispatch, not a copy of it.  tests/xconv_spec.py lists the classes the suite must reach. */
enum {
  DVD_XDESC_TM = 0, DVD_XDESC_TN, DVD_XDESC_WM, DVD_XDESC_WN, /* wave tile and waves per block of xconv_kernel                 */
  DVD_XDESC_B1,        /* one activation stage in LDS                                                                        */
  DVD_XDESC_FAST,      /* buffer-addressed main loop (0: the generic loop, Cin / groups % 16 != 0)                           */
  DVD_XDESC_FIT,       /* staging family, DVD_XFIT_*                                                                         */
  DVD_XDESC_IN16, DVD_XDESC_OUT16,
  DVD_XDESC_WIDE,      /* the LDS-transposed 16-byte epilogue runs (a DVD_XFIT_ONE kernel with whole aligned runs)           */
  DVD_XDESC_S2, DVD_XDESC_ZI,
  DVD_XDESC_TR, DVD_XDESC_TC, DVD_XDESC_P, DVD_XDESC_PQ, DVD_XDESC_NTR, DVD_XDESC_NTC, /* tile, csrc/xconv_tile.h             */
  DVD_XDESC_MBLOCKS,   /* channel blocks per group                                                                           */
  DVD_XDESC_LDS_BYTES, DVD_XDESC_THREADS,
  DVD_XDESC_ITEMS,     /* staging items per thread and chunk                                                                 */
  DVD_XDESC_INTS = 24
};
enum {
  DVD_XFIT_DIRECT = 0, /* item by item, nothing kept in registers across the matrix instructions (wide halos, stride 2)       */
  DVD_XFIT_1 = 1, DVD_XFIT_2 = 2, DVD_XFIT_3 = 3, /* register-prefetched staging, items per thread                            */
  DVD_XFIT_ONE = 11    /* the two-chunk loop of the 1x1 kernels with >= 256 output channels per group                         */
};
int dvd_xconv_describe(int Cin_total, int Cout_total, int H, int W, int KS, int groups, int flags, int in_f16, int out_f16,
                       int operands_aligned16, int* out);
/* Transposed / forward packing with every weight of output channel co scaled by gamma[co] / sqrt(var[co] + eps): the
 * backward-data pass through a fused BatchNorm is dvd_xconv_fwd on the masked, UNSCALED output gradient. */
int dvd_xconv_pack_scaled(const float* w, void* packed, int Cout, int Cin, int KS, int groups, int transposed,
                          const float* bn_gamma, const float* bn_var, float bn_eps, dvd_stream_t stream);
/* All packings of a network in TWO launches (round 6).  items[i] describes one dvd_xconv_pack / dvd_xconv_pack_scaled call
 * (var == NULL: unscaled); `packed` buffers of dvd_xconv_packed_bytes each, all distinct.  `table`: device memory of
 * dvd_xconv_pack_table_bytes(n) that the launches read; upload != 0 (re)writes it from `items` with a blocking copy -- pass it
 * once per item list, OUTSIDE a graph capture -- upload == 0 reuses what the last upload left (`items` must be the same list).
 * The packed bytes are identical to n single calls.  The reference has no counterpart: nn.Conv2d consumes its fp32 weight
 * directly (third_party/midas_blocks.py:35-50); the packing is the operand format of this library's matrix kernels. */
typedef struct dvd_xpack_item {
  const float* w;
  void* packed;
  const float* gamma;   /* may be NULL (scale 1 / sqrt(var + eps)) */
  const float* var;     /* NULL: no BatchNorm scale */
  float eps;
  int Cout, Cin, KS, groups, transposed;
} dvd_xpack_item;
size_t dvd_xconv_pack_table_bytes(int n);
int dvd_xconv_pack_many(const dvd_xpack_item* items, int n, void* table, size_t table_bytes, int upload, dvd_stream_t stream);
/* After the weight-gradient kernel ran on the unscaled masked gradient (dW holds dWu [Cout][K]): scales dW in place and
 * derives the BatchNorm-gamma and convolution-bias gradients (csrc/bnrelu.hip); dbeta = per-channel sum of the masked
 * gradient (dvd_bnrelu_bwd with x = null). */
int dvd_convbn_finalize(const float* W, float* dW, const float* dbeta, const float* gamma, const float* mean, const float* var,
                        float eps, const float* conv_bias, int Cout, int K, float* dgamma, float* dconv_bias, dvd_stream_t stream);
/* Backward-weight of the same convolutions (k = 1 and 3), exact fp32 MFMA, deterministic two-stage sum
 * (csrc/xwgrad.hip): gw[Cout,Cin,k,k] = sum_{n,p} gy[n,co,p] * act(x)[n,ci,p + tap], act = ReLU if relu_in.
 * Replaces the autograd weight gradient of the nn.Conv2d named above (MIOpen accumulates it with atomics). */
size_t dvd_xwgrad_workspace_bytes(int N, int Cin, int Cout, int H, int W, int KS);
int dvd_xwgrad(const float* x, const float* gy, float* gw, void* workspace, size_t workspace_bytes, int N, int Cin,
               int Cout, int H, int W, int KS, int relu_in, dvd_stream_t stream);

/* The 3x3 case on the 16-bit matrix cores with the two-term fp16 split of dvd_xconv_fwd (fp32-class accuracy,
 * deterministic; csrc/xwgrad3.hip): what the MiDaS decoder's weight gradients run on.  x_amax / gy_amax: device scalars
 * with max|x| / max|gy| (or upper bounds) of the whole tensors, see dvd_xconv_fwd. */
size_t dvd_xwgrad3_workspace_bytes(int N, int Cin, int Cout, int H, int W, int groups);
int dvd_xwgrad3(const float* x, const float* x_amax, const float* gy, const float* gy_amax, float* gw, void* workspace,
                size_t workspace_bytes, int N, int Cin, int Cout, int H, int W, int groups, int relu_in, dvd_stream_t stream);
/* ... and the 1x1 case (ResNeXt bottleneck convolutions), same arithmetic: a K-contiguous "NT" GEMM over the pixels. */
size_t dvd_xwgrad1s_workspace_bytes(int N, int Cin, int Cout, int H, int W);
int dvd_xwgrad1s(const float* x, const float* x_amax, const float* gy, const float* gy_amax, float* gw, void* workspace,
                 size_t workspace_bytes, int N, int Cin, int Cout, int H, int W, int relu_in, dvd_stream_t stream);
/* The same, and additionally (gy_rowsum != NULL) gy_rowsum[co] = sum over images and pixels of gy[n][co][:] -- the bias
 * gradient of the convolution / the shift gradient of a BatchNorm fused behind it (nn.Conv2d bias, BatchNorm2d.bias of the
 * ResNeXt bottlenecks behind third_party/midas_blocks.py:35-50), deterministic: wide layers with H * W a multiple of 16 sum the
 * rows inside the weight-gradient kernel, which stages them anyway (per-slice partial sums behind the dW partials in the
 * workspace, added in slice order by the same reduction launch); every other shape takes one extra fixed-order pass over gy.
 * Workspace: dvd_xwgrad1s_workspace_bytes. */
int dvd_xwgrad1s_rowsum(const float* x, const float* x_amax, const float* gy, const float* gy_amax, float* gw, float* gy_rowsum,
                        void* workspace, size_t workspace_bytes, int N, int Cin, int Cout, int H, int W, int relu_in,
                        dvd_stream_t stream);
/* dvd_xwgrad3 plus gy_rowsum (may be NULL), the same sums for the 3x3 case: grouped layers with at most 32 channels per group on
 * both sides (ResNeXt stages 1-3) sum inside the weight-gradient kernel, every other shape by the extra pass.
 * Workspace: dvd_xwgrad3_workspace_bytes. */
int dvd_xwgrad3_rowsum(const float* x, const float* x_amax, const float* gy, const float* gy_amax, float* gw, float* gy_rowsum,
                       void* workspace, size_t workspace_bytes, int N, int Cin, int Cout, int H, int W, int groups, int relu_in,
                       dvd_stream_t stream);
/* 1 if the fp32 weight-gradient kernel that serves this shape (as selected now, see dvd_xwgrad_select) delivers gy_rowsum itself,
 * 0 if dvd_xwgrad1s_rowsum (KS = 1, groups = 1) / dvd_xwgrad3_rowsum (KS = 3) would take the extra pass over gy: a caller that
 * has a pass over gy of its own anyway keeps that one. */
int dvd_xwgrad_rowsum_in_kernel(int N, int Cin, int Cout, int H, int W, int KS, int groups);
/* Test / A-B hook (process wide): 0 = automatic (256 x 256-channel workgroups for wide 1x1 layers, 128 x 128 otherwise),
 * 1 = always 128 x 128, 2 = round 3's row step everywhere (no buffer-load / interleaved-staging instantiations of the 3x3 and
 * wide 1x1 kernels, grouped layers on the 64 x 64 channel blocks), 3 = the 3x3 / k x k walks with four K steps per row step
 * and whole work items dealt round robin to the slices (instead of the live K steps of a strip and one launch per strip class
 * cut into equal row counts, csrc/wg3_plan.h).  Same products and the same per-element summation order
 * within a slice; the number of slices (partial sums added at the end) differs, so results agree to fp32 rounding, not bitwise. */
int dvd_xwgrad_select(int variant);
/* Alignment of the operands of every dvd_xwgrad3* / dvd_xwgrad1s* / dvd_xwgradk* entry point (checked: DVD_EINVAL before any
 * launch).  The kernels read a row of x and gy (W elements; for the 1x1 entry points a whole plane, H * W elements) in the widest
 * items its length allows, so x and gy must sit at a multiple of
 *     16 bytes where a row is a whole number of 16-byte items (fp32: W % 4 == 0, fp16: W % 8 == 0),
 *      8 bytes where it is a whole number of 8-byte items,
 *      4 bytes where it is a whole number of dwords (every fp32 row; fp16 rows of even length: the buffer loads of the
 *              branch-free row step take dword-aligned 16-byte runs),
 *      2 bytes otherwise (fp16 rows of odd length: element loads).
 * Every row of a contiguous tensor then starts on that boundary too.  gw, gy_rowsum and the workspace: 4 bytes.
 *
 * What the entry points above would launch for a shape, under the current dvd_xwgrad_select value: pure host code, no HIP call,
 * usable without a GPU.  KS = 1: dvd_xwgrad1s[_rowsum / _h], 3: dvd_xwgrad3[_rowsum / _h], 5 / 7 / 11: dvd_xwgradk[_h]; in_f16:
 * the _h entry point; with_rowsum: a gy_rowsum pointer is passed (fp32, KS 1 or 3).  DVD_EINVAL for every shape the size queries
 * answer 0 for, and for row sums where no entry point takes them.  out receives DVD_WDESC_INTS ints.  The launch path switches
 * on the same key (csrc/xwgrad3.hip, WgKey / WgCall): this is the dispatch, not a copy of it.  tests/wgrad_spec.py lists the
 * instantiations the suite must reach. */
enum {
  DVD_WDESC_FAMILY = 0,  /* DVD_WFAM_*                                                                                       */
  DVD_WDESC_KS, DVD_WDESC_H16,
  DVD_WDESC_FW, DVD_WDESC_RSUM, /* the FW / RSUM template arguments of the instantiation (0 where the family has no such form) */
  DVD_WDESC_LAUNCHES,    /* 1 or 2 (one per strip class, csrc/wg3_plan.h); an 11x11 launch is two kernels (DVD_WDESC_SECOND)   */
  DVD_WDESC_L0,          /* first launch: DVD_WDESC_L_INTS ints, the second launch right behind it                           */
  DVD_WDESC_SECOND = DVD_WDESC_L0 + 12, /* every launch runs a second kernel (11x11: kernel columns 6 .. 10)                  */
  DVD_WDESC_NCO, DVD_WDESC_NCI,         /* channel blocks per group: grid z / groups, grid y                                 */
  DVD_WDESC_LDS_BYTES, DVD_WDESC_THREADS,
  DVD_WDESC_SLICES,      /* partial slices the launches write in all                                                          */
  DVD_WDESC_WS_BYTES_LO, DVD_WDESC_WS_BYTES_HI, /* workspace bytes the call needs, exactly: LO + HI * 2^31                    */
  DVD_WDESC_CHANSUM,     /* the row sums come from the extra fixed-order pass over gy                                         */
  DVD_WDESC_DEAL,        /* whole work items dealt round robin (dvd_xwgrad_select(3))                                         */
  DVD_WDESC_ALIGN,       /* bytes x and gy must be aligned to                                                                 */
  DVD_WDESC_INTS = 32
};
enum {                   /* per launch                                                                                        */
  DVD_WDESC_L_NK = 0,    /* live K steps per row step of the strips it walks (1 .. 4)                                         */
  DVD_WDESC_L_KEY_NK,    /* the NK template argument; 0: the instantiation has none (guarded 3x3 row step, 1x1 kernels)       */
  DVD_WDESC_L_S, DVD_WDESC_L_SLICE0,      /* slices of the launch (grid x), the first partial slice it writes                  */
  DVD_WDESC_L_STRIP0, DVD_WDESC_L_NCOLS,  /* the column strips [strip0, strip0 + ncols) of every image (0, 0 for 1x1)          */
  DVD_WDESC_L_INTS = 6
};
enum { DVD_WFAM_XWGRAD3 = 0, DVD_WFAM_XWGRAD3G, DVD_WFAM_XWGRADK, DVD_WFAM_XWGRAD1S, DVD_WFAM_XWGRAD1B };
int dvd_xwgrad_describe(int KS, int N, int Cin_total, int Cout_total, int H, int W, int groups, int in_f16, int with_rowsum,
                        int* out);
/* The weight gradient (as dvd_xwgrad3) of dense 5x5 / 7x7 / 11x11 stride-1 "same" convolutions (round 4: third_party/hourglass.py:21-57, the inception
 * branches; round 3 left their weight gradient to MIOpen): split-operand MFMA, 32 x 32 channels per block, one wave per kernel
 * row, deterministic.  gw [Cout][Cin][KS][KS]. */
size_t dvd_xwgradk_workspace_bytes(int N, int Cin, int Cout, int H, int W, int KS);
int dvd_xwgradk(const float* x, const float* x_amax, const float* gy, const float* gy_amax, float* gw, void* workspace,
                size_t workspace_bytes, int N, int Cin, int Cout, int H, int W, int KS, int relu_in, dvd_stream_t stream);

/* ------------------------------------------------------------------------
 * Flow-consistency (occlusion) + out-of-bounds mask of one direction of a frame pair.
 * Replaces scripts/preprocess/davis/generate_flows.py:57-82,139-148:
 *   mask = clip([ || grid_sample(flow_a, (x,y)+flow_b, zeros padding, align_corners) + flow_b || > 1 ]
 *               + [ (x,y)+flow_b outside the image ], 0, 1)
 * mask_1 = f(flow_a = flow_1_2, flow_b = flow_2_1), mask_2 = f(flow_2_1, flow_1_2); flows [B,H,W,2], mask [B,H,W]
 * in {0,1} (1 = occluded / leaves the image; the training masks are 1 - mask, generate_sequence_midas.py:144-147).
 * Same fp32 operation order as the reference's numpy / ATen path: the integer masks are bit-identical. */
int dvd_flow_consistency_mask(const float* flow_a, const float* flow_b, float* mask, int B, int H, int W,
                              dvd_stream_t stream);

/* ------------------------------------------------------------------------
 * fp16 ACTIVATION STORAGE (round 4; BASELINE.json configs[4]: "fp16 activations with fp32 loss accumulation").
 * Reference: the same layers as the fp32 entry points above (third_party/MiDaS.py:186-246, third_party/midas_blocks.py:35-168);
 * the reference itself has no reduced-precision mode.  Every tensor between the encoder stem and the depth head is stored as
 * _Float16 in HBM; the image, the depth map, parameters, parameter gradients, loss sums and optimiser state stay fp32 and every
 * accumulation is fp32.  An fp16 activation IS the matrix operand (one term, no scale): activation x two-term weight = 2 MFMAs per
 * product instead of 3, activation x activation (weight gradients) = 1 instead of 3.
 *   "_h" entry points: activations / gradients are _Float16 (void*).
 *   "_t" entry points: `f16` selects the storage (0 = float, 1 = _Float16) of the activation / gradient tensors.
 *   out_scale: device scalar the PARAMETER gradients are multiplied by -- 1 / (loss scale of the fp16 gradients), state[1] of the
 *   loss-scale state below (null = 1). */
/* dvd_xconv_fwd with fp16 input; out_f16 = 0 writes fp32 (then residual / mask_src are fp32 too).  Needs Cin / groups % 16 == 0. */
int dvd_xconv_fwd_h(const void* x, const void* packed, const float* bias, const void* residual, const void* mask_src,
                    const dvd_bn_params* bn, void* y, float* y_amax, int N, int Cin_total, int Cout_total, int H, int W, int KS,
                    int groups, int flags, int out_f16, dvd_stream_t stream);
int dvd_xwgrad3_h(const void* x, const void* gy, const float* out_scale, float* gw, void* workspace, size_t workspace_bytes, int N,
                  int Cin_total, int Cout_total, int H, int W, int groups, int relu_in, dvd_stream_t stream);
int dvd_xwgrad1s_h(const void* x, const void* gy, const float* out_scale, float* gw, void* workspace, size_t workspace_bytes, int N,
                   int Cin, int Cout, int H, int W, int relu_in, dvd_stream_t stream);
/* ABI 8: dvd_xwgradk with fp16 operands -- the 5x5 / 7x7 / 11x11 weight gradients of the hourglass's inception branches
 * (third_party/hourglass.py:21-57) under fp16 activation storage.  Same walk, plan and workspace (dvd_xwgradk_workspace_bytes) as
 * dvd_xwgradk; one v_mfma_f32_32x32x16_f16 per product, fp32 accumulation, result times out_scale[0]; deterministic. */
int dvd_xwgradk_h(const void* x, const void* gy, const float* out_scale, float* gw, void* workspace, size_t workspace_bytes, int N,
                  int Cin, int Cout, int H, int W, int KS, int relu_in, dvd_stream_t stream);
int dvd_bnrelu_fwd_t(const void* x, const void* residual, const float* gamma, const float* beta, const float* mean,
                     const float* var, float eps, void* y, int f16, int N, int C, int HW, int relu, dvd_stream_t stream);
int dvd_bnrelu_bwd_t(const void* gy, const void* y, const void* x, const float* gamma, const float* mean, const float* var,
                     float eps, void* gx, void* g_residual, float* g_gamma, float* g_beta, void* workspace,
                     size_t workspace_bytes, int f16, const float* out_scale, int N, int C, int HW, int relu, float* g_amax,
                     dvd_stream_t stream);
/* The same with the maxima the consuming convolutions take their operand scale from (round 6; before: a dvd_amax pass over
 * the tensor): y_amax[0] = max(y_amax[0], max|y|); gx_amax[0] = max(gx_amax[0], max|gx|) (exact: |gamma / sqrt(var + eps)| *
 * max|g| per channel).  NULL: not wanted.  fp32 and fp16 storage alike. */
int dvd_bnrelu_fwd_m(const void* x, const void* residual, const float* gamma, const float* beta, const float* mean,
                     const float* var, float eps, void* y, int f16, int N, int C, int HW, int relu, float* y_amax,
                     dvd_stream_t stream);
int dvd_bnrelu_bwd_m(const void* gy, const void* y, const void* x, const float* gamma, const float* mean, const float* var,
                     float eps, void* gx, void* g_residual, float* g_gamma, float* g_beta, void* workspace,
                     size_t workspace_bytes, int f16, const float* out_scale, int N, int C, int HW, int relu, float* g_amax,
                     float* gx_amax, dvd_stream_t stream);
int dvd_upsample_bilinear_fwd_t(const void* x, void* y, int f16, long long planes, int H_in, int W_in, int H_out, int W_out,
                                int align_corners, dvd_stream_t stream);
int dvd_upsample_bilinear_bwd_t(const void* gy, void* gx, int f16, long long planes, int H_in, int W_in, int H_out, int W_out,
                                int align_corners, dvd_stream_t stream);
int dvd_gconv3x3_c8_fwd_t(const void* x, const float* w, void* y, int f16, int N, int C, int H, int W, dvd_stream_t stream);
int dvd_gconv3x3_c8_bwd_data_t(const void* gy, const float* w, void* gx, int f16, int N, int C, int H, int W,
                               dvd_stream_t stream);
int dvd_gconv3x3_c8_bwd_weight_t(const void* x, const void* gy, float* gw, int accumulate, void* workspace,
                                 size_t workspace_bytes, int f16, const float* out_scale, int N, int C, int H, int W,
                                 dvd_stream_t stream);
/* The depth head `ReLU -> Conv2d(C, 1, 1)` (third_party/MiDaS.py:192-194), the fp16 / fp32 boundary: y fp32 [N,1,H,W] from
 * x [N,C,H,W] (C <= 64, H * W % 4 == 0); backward: gx = S * w[c] * gy * [x > 0] (storage of x), gw [C], gb [1] fp32 from the
 * unscaled fp32 gy; gscale_state: the loss-scale state (null: S = 1).  Deterministic (fixed-order partial sums). */
/* fwd_amax (optional): max |y| of the head output is folded into it (NaN counted as +Inf) -- slot [6] of the loss-scale state,
 * the forward monitor of the fp16 overflow guard. */
int dvd_head1x1_fwd(const void* x, int f16, const float* w, const float* bias, float* y, float* fwd_amax, int N, int C, int HW,
                    int relu_in, dvd_stream_t stream);
size_t dvd_head1x1_bwd_workspace_bytes(int C);
int dvd_head1x1_bwd(const void* x, int f16, const float* w, const float* gy, const float* gscale_state, void* gx, float* gw,
                    float* gb, void* workspace, size_t workspace_bytes, int N, int C, int HW, int relu_in, dvd_stream_t stream);
/* ABI 8: the hourglass's depth head `pred_layer = Conv2d(C, 1, 3, padding 1)` (reference third_party/hourglass.py:175-182), the
 * fp16 / fp32 boundary of that net: y fp32 [N,1,H,W] = bias + conv(x), x _Float16 [N,C,H,W] (C <= 64); max |y| folded into
 * fwd_amax (optional, the forward monitor [6] of the loss-scale state).  Backward: gx = S * conv_transpose(gy, w) as _Float16
 * (max |S gx| folded into gscale_state[3]), gw [C][3][3] and gb [1] fp32 from the unscaled fp32 gy; gscale_state null: S = 1.
 * Deterministic (fixed-order partial sums). */
int dvd_head3x3_fwd(const void* x, const float* w, const float* bias, float* y, float* fwd_amax, int N, int C, int H, int W,
                    dvd_stream_t stream);
size_t dvd_head3x3_bwd_workspace_bytes(int N, int C, int H, int W);
int dvd_head3x3_bwd(const void* x, const float* w, const float* gy, const float* gscale_state, void* gx, float* gw, float* gb,
                    void* workspace, size_t workspace_bytes, int N, int C, int H, int W, dvd_stream_t stream);
/* ABI 8: y = a + b of two _Float16 tensors (n elements), max |y| folded into fwd_amax (optional; NaN counted as +Inf): the sums of
 * the hourglass's two parallel paths (third_party/hourglass.py:60-158) under the overflow guard. */
int dvd_add_f16(const void* a, const void* b, void* y, long long n, float* fwd_amax, dvd_stream_t stream);
/* Loss scale of the fp16 gradients, kept on the device (state: 16 floats since ABI 7; [0] = S, [1] = 1 / S, [2] = target exponent,
 * [3] = observed max |S g| this step, [4] = skip flag, [5] = skipped steps, [6] = forward monitor: max |activation| the fp16-output
 * convolution epilogues and the depth head folded in this step -- every maximum counts a NaN as +Inf).  begin: S = 2^(target - ceil(log2(max|g| * max|w|)))
 * from the device scalar max|g_out| and the n_w head weights; end (once per step, before the optimiser): overflow -> skip flag +
 * back-off, small observed maximum -> raise the target; an ACTIVATION beyond fp16's range ([6] >= 65504) -> skip flag only.  Policy and thresholds: csrc/a16.hip.
 * ABI 7: [8] = this step was skipped for an activation overflow, [9] = steps skipped for that reason so far (the (flag, count) pair
 * for dvd_adam_step_guarded of a network whose fp32 gradients survive a mere loss-scale overflow), [10] = consecutive such skips;
 * step_begin (first launch of every TRAINING step) clears the forward monitor [6], which every fp16 forward -- validation and
 * inference included -- folds into. */
int dvd_gscale_init(float* state, float target_exponent, dvd_stream_t stream);
int dvd_gscale_step_begin(float* state, dvd_stream_t stream);
int dvd_gscale_begin(float* state, const float* g_amax, const float* w, int n_w, dvd_stream_t stream);
int dvd_gscale_end(float* state, dvd_stream_t stream);
/* out[i] = scale[0] * in[i] as fp32 (n % 4 == 0): the gradient leaving the fp16 region towards the fp32 stem. */
int dvd_cast_scale_f32(const void* in, int f16, float* out, long long n, const float* scale, dvd_stream_t stream);
/* dvd_adam_step that does nothing when skip_flag[0] != 0 (state[4] above): the GradScaler "skipped step".  skip_flag points INTO
 * the loss-scale state: skip_flag[1] (state[5], the steps skipped so far) is subtracted from `step` for Adam's bias correction,
 * so that skipped steps do not advance the optimiser (round 5). */
int dvd_adam_step_guarded(float* param, const float* grad1, float scale, const float* scale_ptr, const float* grad2,
                          float* exp_avg, float* exp_avg_sq, long long n, float lr, float beta1, float beta2, float eps,
                          int step, const float* skip_flag, dvd_stream_t stream);
/* dvd_sgd_step: torch.optim.SGD as the reference builds it under --optim sgd (models/netinterface.py:96-102,126-135: momentum =
 * opt.sgd_momentum, dampening = opt.sgd_dampening, weight_decay = opt.wdecay; defaults options/options_train.py:88-93; no
 * nesterov) on a flat buffer with grad = s*grad1 + grad2 as in dvd_adam_step:  d = g + wd p;  buf = d at the first step, else
 * momentum buf + (1 - dampening) d;  p -= lr (momentum != 0 ? buf : d).  momentum_buf may be null when momentum == 0. */
int dvd_sgd_step(float* param, const float* grad1, float scale, const float* scale_ptr, const float* grad2, float* momentum_buf,
                 long long n, float lr, float momentum, float dampening, float weight_decay, int step, dvd_stream_t stream);
/* dvd_sgd_step that does nothing -- momentum buffer untouched -- when skip_flag[0] != 0, and takes step - skip_flag[1] as the
 * effective step, as dvd_adam_step_guarded does (torch.amp's GradScaler skips optimizer.step(), models/netinterface.py:96-102):
 * effective step 1 is the first step of torch.optim.SGD (buf = d, no dampening), decided on the device. */
int dvd_sgd_step_guarded(float* param, const float* grad1, float scale, const float* scale_ptr, const float* grad2,
                         float* momentum_buf, long long n, float lr, float momentum, float dampening, float weight_decay, int step,
                         const float* skip_flag, dvd_stream_t stream);

/* nn.MaxPool2d(3, stride 2, padding 1) of the ResNeXt stem (third_party/midas_blocks.py:35-45), ATen's semantics (the first
 * maximum of a window takes the gradient).  x fp32 [planes][H][W] -> y [planes][Ho][Wo] (Ho = (H - 1) / 2 + 1) in fp32 or
 * _Float16 (y_f16: the fp32 -> fp16 boundary of fp16 activation storage), index: one byte per output (winner's window position).
 * Backward: gx fp32 = out_scale[0] * (gather of gy over the windows that contain the pixel); deterministic. */
int dvd_maxpool3s2_fwd(const float* x, void* y, int y_f16, unsigned char* index, long long planes, int H, int W,
                       dvd_stream_t stream);
int dvd_maxpool3s2_bwd(const void* gy, int gy_f16, const unsigned char* index, float* gx, const float* out_scale,
                       long long planes, int H, int W, dvd_stream_t stream);
/* x[:, :, ::2, ::2] as a contiguous tensor [planes][(H + 1) / 2][(W + 1) / 2] and its backward (zeros with gy at the even
 * positions), fp32 or _Float16 (ABI 7): the sub-sampling around the stride-2 convolutions of a ResNeXt stage's entry
 * (third_party/midas_blocks.py:35-50 via torchvision's Bottleneck.conv2 / downsample). */
int dvd_subsample2_fwd(const void* x, void* y, int f16, long long planes, int H, int W, dvd_stream_t stream);
int dvd_subsample2_bwd(const void* gy, void* gx, int f16, long long planes, int H, int W, dvd_stream_t stream);
/* nn.AvgPool2d(k, stride, pad) with PyTorch's defaults (count_include_pad, floor mode) on [planes, H, W] tensors, fp32 or fp16
 * (f16 != 0): AvgPool2d(2) of the hourglass (third_party/hourglass.py:60-158), AvgPool2d(3, 2, 1) of FCNUnet
 * (networks/FCNUnet.py:64); ATen's arithmetic (fp32 window sum / (k * k); backward: gy / (k * k) summed over the windows that
 * hold the pixel).  y / gy are [planes, (H + 2 pad - k) / stride + 1, (W + 2 pad - k) / stride + 1]. */
int dvd_avgpool_fwd(const void* x, void* y, int f16, long long planes, int H, int W, int k, int stride, int pad,
                    dvd_stream_t stream);
int dvd_avgpool_bwd(const void* gy, void* gx, int f16, long long planes, int H, int W, int k, int stride, int pad,
                    dvd_stream_t stream);


/* Batched pair permutation (an addition within ABI 8; no counterpart in the reference, which runs one pair per step): ONE launch
 * that copies dst_k[b] = src_k[perm[b]], b < B, for every tensor k of a table of n_items <= DVD_GATHER_MAX per-pair tensors of
 * any element type (bytes_per_pair = bytes of one index of dim 0).  A step that mixes frame gaps brings its batch into
 * gap-grouped order with it, and its exports back into the caller's order with the inverse permutation
 * (models/scene_flow_motion_field.py).  `items` is a HOST array (it travels in the kernel arguments), `perm` a DEVICE array of B
 * ints in [0, B) -- an index outside the batch copies nothing for that pair.  16-byte accesses where a tensor's two base addresses
 * and bytes_per_pair are multiples of 16, 4-byte accesses for multiples of 4, bytes otherwise.  src and dst of a tensor must not
 * overlap; more than DVD_GATHER_MAX tensors, an overlap or a null pointer return DVD_EINVAL before anything is launched. */
#define DVD_GATHER_MAX 32
typedef struct dvd_gather_item {
  const void* src;
  void* dst;
  long long bytes_per_pair;
} dvd_gather_item;
int dvd_gather_pairs(const dvd_gather_item* items, int n_items, const int* perm, int B, dvd_stream_t stream);

/* Batch assembly out of a device-resident frame store (an addition within ABI 8; csrc/frame_store.hip): ONE launch that writes
 * row b < B of every tensor k of a table of n_items <= DVD_STORE_MAX tensors from row index[index_row_k * index_stride + b] of
 * that tensor's source table.  It is the re-arrangement of frames and flow pairs into per-pair tensors that the reference does
 * on the host -- scripts/preprocess/davis/generate_sequence_midas.py:117-170 when it writes the pair packs, then
 * datasets/davis_sequence.py:98-115 when it reads them -- done per step on the device (datasets/frame_store.py).
 * `items` is a HOST array (it travels in the kernel arguments); `index` is a DEVICE array of three rows of ints, index_stride
 * (>= B) ints apart: by convention row 0 = first frame, 1 = second frame, 2 = flow pair.  src_rows is the number of rows of
 * the source table: an index outside [0, src_rows) writes nothing for that pair and reads nothing.  Operations, with
 * bytes_per_row the bytes of one DESTINATION row:
 *   DVD_STORE_COPY  dst row = src row (bytes_per_row bytes each), any element type; 16-byte accesses where both bases and
 *                   bytes_per_row are multiples of 16, 4-byte accesses for multiples of 4, bytes otherwise;
 *   DVD_STORE_MASK  src rows of bytes_per_row / 4 uint8, dst fp32: dst = 1.0f - (float)src, which is the writer's
 *                   1 - ceil(mask) (:144-147) for every uint8 value;
 *   DVD_STORE_FILL  src one fp32 per row, dst fp32: every element of the destination row is that value (time-stamp planes).
 * No arithmetic other than that conversion happens here.  Null pointers, an empty batch, more than DVD_STORE_MAX tensors, an
 * unknown operation or index row, a misaligned fp32 side or overlapping src / dst return DVD_EINVAL before any HIP call.
 * The launch's algorithmic bytes are counted under DVD_BYTES_GATHER. */
#define DVD_STORE_MAX 32
enum { DVD_STORE_COPY = 0, DVD_STORE_MASK = 1, DVD_STORE_FILL = 2 };
typedef struct dvd_store_item {
  const void* src;
  void* dst;
  long long bytes_per_row;
  int src_rows;
  int index_row;
  int op;
  int pad;
} dvd_store_item;
int dvd_store_gather(const dvd_store_item* items, int n_items, const int* index, long long index_stride, int B,
                     dvd_stream_t stream);

/* The depth net once per DISTINCT frame of a step (additions within ABI 8; csrc/frame_union.hip, models/frame_union.py,
 * opt.share_frames).  The reference evaluates net_depth(img_1) and net_depth(img_2) with the net in eval() mode, so an image
 * that several pairs of a step show has one depth map; these three launches move rows between the step's two per-pair sets
 * (B rows each) and the union of their frames (U_pad rows).  Rows are fp32 (any bytes_per_row that is a multiple of 4); every
 * index array is a DEVICE array of ints; 16-byte accesses where the row size and every base address are multiples of 16, dwords
 * otherwise.  Copies and sequential fp32 adds only: no atomics, no scaling, results are bit-reproducible.  Null pointers, empty
 * sizes, misaligned or overlapping buffers return DVD_EINVAL before any HIP call; bytes are counted under DVD_BYTES_GATHER.
 *   dvd_union_gather   out[u] = (set[u] ? img_2 : img_1)[row[u]], u < U_pad; a set outside {0, 1} or a row outside [0, B)
 *                      reads and writes nothing for that union row.
 *   dvd_union_scatter  ONE launch: depth_1[b] = D[u1[b]], depth_2[b] = D[u2[b]], b < B; an index outside [0, U_pad) writes
 *                      nothing for that image.
 *   dvd_union_reduce   G[u] = 0 + g[e_0] + g[e_1] + ... over entries[offsets[u] .. offsets[u + 1]) in list order, left to
 *                      right, where an entry is set * B + row and g = set ? g_d2 : g_d1 (floats_per_row floats per row); a
 *                      row without entries is zero; an entry outside [0, 2B) (or the part of a range outside the list) adds
 *                      nothing.  offsets holds U_pad + 1 ints, entries 2B. */
int dvd_union_gather(const void* img_1, const void* img_2, void* out, const int* set, const int* row, int U_pad, int B,
                     long long bytes_per_row, dvd_stream_t stream);
int dvd_union_scatter(const void* D, void* depth_1, void* depth_2, const int* u1, const int* u2, int B, int U_pad,
                      long long bytes_per_row, dvd_stream_t stream);
int dvd_union_reduce(const float* g_d1, const float* g_d2, float* G, const int* offsets, const int* entries, int U_pad, int B,
                     long long floats_per_row, dvd_stream_t stream);

/* Long-range tracks: world points into a sequence of target cameras (additions within ABI 8; csrc/track.hip, models/tracks.py).
 * dvd_track_project replaces project_ptcld.forward (losses/scene_flow_projection.py:27-44) and, for depth_at, BackwardWarp
 * (:289-297) applied to that module's displacement field; dvd_project_bwd is what autograd derives from :38-41 for global_p1.
 *   points     [T1, B, 3, H, W] (points_planar != 0: the layout the scene-flow MLP's p_next writes, one slab row per
 *              integration step) or [T1, B, H, W, 3]
 *   start      DEVICE array of B ints: image b of step k is projected into frame g = start[b] + k
 *   R, t, K_T  the per-frame tables [N, 3, 3], [N, 3], [N, 3, 3]: world->camera rotation (the reference's R_1_T), camera
 *              centre, transposed intrinsics (the reference's K), as datasets/frame_store.py keeps them
 *   depth_all  [N, 1, H, W] or NULL
 * Outputs, per point, with I = ((P - t_g) @ R_g) @ K_T_g in torch's fp32 operation order:
 *   uv         [T1, B, H, W, 2] = I.xy / (I.z + 1e-8); with displacement != 0 minus the pixel's own (x, y), which is
 *              project_ptcld's return value
 *   z          [T1, B, H, W] = I.z (may be NULL)
 *   depth_at   [T1, B, H, W] = depth_all[g] sampled at uv by grid_sample's rule (bilinear, border, align_corners=True), 0
 *              where z <= 0; not written when depth_all is NULL
 *   inside     uint8 [T1, B, H, W] = z > 0 && 0 <= u <= W - 1 && 0 <= v <= H - 1 (may be NULL)
 * Where g >= N (the video has ended; a negative start counts the same) every output is 0 and no table is read.  No index
 * derived from the data leaves a table: the sampling position is clamped to the image, NaN included.  No atomics; every
 * output element has one writer.  16-byte accesses (and the four `inside` bytes of a thread as one dword) where W is a
 * multiple of 4 and the bases are 16-byte aligned, one pixel per thread otherwise.
 * dvd_project_bwd: g_points (+)= J^T g_uv, J the 2x3 Jacobian of uv w.r.t. the point (0 where g >= N); g_points has the
 * layout of points; the cameras get no gradient.  T1, B <= 65535, H, W >= 2; bytes are counted under DVD_BYTES_GEOMETRY. */
int dvd_track_project(const float* points, int points_planar, const int* start, const float* R, const float* t,
                      const float* K_T, const float* depth_all, int N, float* uv, int displacement, float* z,
                      float* depth_at, unsigned char* inside, int T1, int B, int H, int W, dvd_stream_t stream);
int dvd_project_bwd(const float* g_uv, const float* points, int points_planar, const int* start, const float* R,
                    const float* t, const float* K_T, int N, float* g_points, int accumulate, int T1, int B, int H, int W,
                    dvd_stream_t stream);

/* Backward-in-time advection: two-sided tracks (additions within ABI 8; csrc/invert.hip, csrc/track.hip, models/tracks.py).
 * One Euler step of the chain, x -> x + s f(x, t), is a near-identity map; the point y it carries to p is the fixed point of
 * y <- p - s f(y, t).  dvd_sf_mlp_fwd delivers sf = s f(y_old, t) into its sf_out; dvd_track_invert_update forms the next
 * iterate and measures how far it moved:
 *   p, sf, y_old, y_out  [B, 3, H, W] fp32 (planar);  y_out = p - sf
 *   resid      [B] or NULL: resid[b] = max(resid[b], max over image b of |y_out - y_old|) -- the caller zeroes it; a NaN
 *              difference counts as +Inf, as with dvd_amax; a max of non-negative floats as unsigned integers, so it does
 *              not depend on the order of the waves
 * y_old may alias p or y_out (every element is read and written by one thread).  16-byte accesses where HW = H * W is a
 * multiple of 4 and the four bases are 16-byte aligned, one value per thread otherwise.  B <= 65535, HW < 2^30: DVD_EINVAL
 * before any launch otherwise.  Bytes are counted under DVD_BYTES_GEOMETRY.
 * dvd_track_project_from is dvd_track_project with a row offset: image b of row k is projected into frame
 * g = start[b] + k + k0, and every output is 0 where g < 0 or g >= N (a start frame inside the video keeps the rows that have
 * a frame although start[b] + k0 < 0).  k0 = 0 is dvd_track_project, bit for bit. */
int dvd_track_invert_update(const float* p, const float* sf, const float* y_old, float* y_out, float* resid, int B, int HW,
                            dvd_stream_t stream);
int dvd_track_project_from(const float* points, int points_planar, const int* start, const float* R, const float* t,
                           const float* K_T, const float* depth_all, int N, float* uv, int displacement, float* z,
                           float* depth_at, unsigned char* inside, int T1, int B, int H, int W, int k0, dvd_stream_t stream);

/* Geometry-aware temporal depth filter along two-sided tracks (an addition within ABI 8; csrc/track_filter.hip,
 * models/filter.py).  points, start, the tables, depth_all (required here) and k0 are dvd_track_project_from's: row k of image b
 * is the world point of every pixel of frame start[b] in frame g = start[b] + k + k0; row o = -k0 is the start frame itself
 * (0 <= o < T1 <= 33).  Per pixel p of image b, with d0 = depth_all[start[b]][p]:
 *   every row k != o whose frame exists is projected and sampled exactly as dvd_track_project_from does it (the same z,
 *   depth_at = D and inside, bit for bit) and COUNTS iff  inside && z >= z_near && D > 0 && z <= D * (1 + tol) &&
 *   D <= z * (1 + tol);  its sample is r = D / z.  Row o always counts with r = 1.
 *   mode 0   ratio = (sum of weights[k] * r) / (sum of weights[k]) over the counting rows in ascending k, every multiply and
 *            add a separate fp32 operation;  weights: device fp32 [T1], >= 0, weights[o] > 0 (the caller's duty)
 *   mode 1   ratio = the median of the counting samples ((a + b) * 0.5f of the two middle ones for an even count); weights
 *            is not read but must not be NULL
 *   depth_out [B,1,H,W] = d0 * ratio;  ratio [B,1,H,W];  count uint8 [B,H,W] = counting rows, 1 .. 33;  spread [B,1,H,W] =
 *            largest minus smallest counting r.  ratio, count, spread may be NULL.
 *   !(d0 > 0), NaN included:  depth_out = d0, ratio = 1, count = 0, spread = 0.
 * The ratio is taken along the target camera's ray and applied along the start camera's.  No atomics, one writer per output
 * element, plain vector stores: the same inputs give the same bits.  16-byte accesses where W is a multiple of 4 and the
 * bases are 16-byte aligned, one pixel per thread otherwise; the median keeps its samples in LDS (T1 * 1 KiB per block).
 * DVD_EINVAL before any launch for a null pointer, T1 outside 1 .. 33, o outside the slab, a mode other than 0 / 1, tol or
 * z_near negative or not finite, and dvd_track_project's shape rules.  Bytes are counted under DVD_BYTES_GEOMETRY. */
int dvd_track_filter(const float* points, int points_planar, const int* start, const float* R, const float* t,
                     const float* K_T, const float* depth_all, int N, const float* weights, int mode, float tol, float z_near,
                     float* depth_out, float* ratio, unsigned char* count, float* spread, int T1, int B, int H, int W, int k0,
                     dvd_stream_t stream);

/* Triangulated depth and epipolar motion cue from stored flow and cameras (an addition within ABI 8; csrc/triangulate.hip,
 * preprocess.triangulate_depth).  For query frame a = frames[b] and pixel x = (u, v, 1), row b of the observation table
 *   obs      int32 [B, M, 3], rows (pair, other frame, dir), M <= 32; pair = -1 is padding and may stand anywhere in a row
 *   dir 0    reads flow_1_2[pair] with mask_2[pair] (a is the pair's first frame)
 *   dir != 0 reads flow_2_1[pair] with mask_1[pair] (a is the pair's second frame)
 *   flows    fp32 [P, H, W, 2];  masks uint8 [P, H, W], 0 = valid;  frames int32 [B]
 *   R, t, K_T, K_inv_T   the per-frame tables [N,3,3], [N,3], [N,3,3], [N,3,3]: R camera to world (row-major), t the camera
 *            centre, K_T and K_inv_T the transposed intrinsics and their inverse
 * is walked in ascending order.  Per observation, with b the other frame, every multiply and add a separate fp32 operation,
 * every three-term sum as (p0 + p1) + p2, divisions and the square root IEEE:
 *   x' = x + flow;  d1 = R_a (K_a^-1 x);  d2 = R_b (K_b^-1 x');  bl = t_b - t_a
 *   A = d1.d1, Bq = d1.d2, C = d2.d2, E = d1.bl, F = d2.bl, den = A C - Bq Bq
 *   s1 = (E C - Bq F) / den (the planar depth in frame a),  s2 = (Bq E - A F) / den,  sin2 = den / (A C)
 *   h0 = K_b (R_b^T (t_a - t_b)),  h1 = K_b (R_b^T d1),  l = h0 x h1,
 *   e = |(l0 x'0 + l1 x'1) + l2| / sqrt(l0 l0 + l1 l1) (epipolar distance in pixels), replaced by 1e30 unless e <= 1e30
 *   usable      mask byte == 0 && 0 <= x'0 <= W-1 && 0 <= x'1 <= H-1 && sin2 >= sin2_min
 *   consistent  usable && e <= epi_tol && z_near <= s1 <= 1e30 && z_near <= s2 <= 1e30
 * (a NaN fails every comparison).  Outputs per query pixel:
 *   depth  [B,1,H,W]  mode 0: (sum of sin2 * s1) / (sum of sin2) over the consistent observations;  mode 1: their exact
 *                     median, (lo + hi) * 0.5f of the two middle ones for an even count;  0 where count < min_count
 *   count, usable  uint8 [B,H,W]  the number of consistent and of usable observations
 *   epi    [B,1,H,W]  (sum of e over the usable observations) / usable;  -1 where usable == 0
 *   spread [B,1,H,W]  (largest - smallest consistent s1) / depth, at most 1e30;  0 where depth == 0
 * No output ever holds a NaN or an Inf.  The kernel reads only the query pixel's own element of each flow and mask (nothing
 * is gathered at x'), and skips a row whose pair is outside 0 .. P-1 or whose frame is outside 0 .. N-1; a query frame
 * outside 0 .. N-1 gives depth = spread = 0, epi = -1, count = usable = 0.  live_rows: the number of rows with pair >= 0 over
 * the B frames (byte accounting only).  One thread per pixel, grid (ceil(H W / 256), B); the median keeps its samples in LDS
 * (M * 1 KiB per block).  DVD_EINVAL before any launch for a null pointer, M outside 0 .. 32, B outside 1 .. 65535,
 * H * W >= 2^30, a mode other than 0 / 1, epi_tol or z_near negative or not finite, sin2_min outside (0, 1], min_count outside
 * 1 .. 255.  Bytes are counted under DVD_BYTES_GEOMETRY: H W (9 live_rows + 14 B). */
int dvd_triangulate(const float* flow_1_2, const float* flow_2_1, const unsigned char* mask_1, const unsigned char* mask_2, int P,
                    const int* obs, const int* frames, long long live_rows, const float* R, const float* t, const float* K_T,
                    const float* K_inv_T, int N, int mode, float epi_tol, float sin2_min, float z_near, int min_count,
                    float* depth, unsigned char* count, unsigned char* usable, float* epi, float* spread, int M, int B, int H,
                    int W, dvd_stream_t stream);

/* Forward splat of world points into target cameras with a soft z-buffer (additions within ABI 8; csrc/splat.hip,
 * models/render.py): the scatter that goes with dvd_track_project's gather.  It draws a frame, pushed along the scene-flow
 * field by the Euler chain of Model.forward_sf_net_multi_step (models/scene_flow_motion_field.py:360-367), in the camera of
 * another frame or in one that never existed; the projection is project_ptcld.forward
 * (losses/scene_flow_projection.py:27-44) through the same device function as dvd_track_project.
 *   points     [S, 3, H, W] (points_planar != 0) or [S, H, W, 3]: world points of S source images
 *   values     [S, C, H, W], 1 <= C <= 8: what is drawn (colours)
 *   valid      uint8 [S, H, W] or NULL: a zero byte drops the point
 *   view       DEVICE array of S ints: the target view of every source image; < 0 or >= V skips the image (nothing of it is
 *              read, nothing written).  Any number of images may share a view.
 *   R, t, K_T  the camera tables of the V views, [V, 3, 3], [V, 3], [V, 3, 3], as dvd_track_project takes them
 *   zbuf       unsigned int [V, H, W], cleared to 0xFF bytes by the caller;  acc  unsigned long long [V, H, W, C + 1],
 *              cleared to 0 by the caller.  dvd_splat_workspace_bytes(V, C, H, W) is the size of both together (0 for sizes
 *              the entries refuse); it needs no GPU.
 * Per point I = ((P - t_v) @ R_v) @ K_T_v, z = I.z, (u, v) = I.xy / (z + 1e-8).  The point is live iff its valid byte is
 * non-zero, every value is finite, z > z_near, z is finite, -1 < u < W and -1 < v < H -- decided in float before any
 * conversion to an integer, so no index derived from the data leaves the image.  Its taps are (floor u + i, floor v + j),
 * i, j in {0, 1}, with the bilinear weights w; a tap counts iff it is inside the image and w >= w_tap.
 *   dvd_splat_zmin        zbuf <- min over the counting taps of the bit pattern of z (integer atomicMin; z > 0)
 *   dvd_splat_accumulate  a counting tap with z <= zmin * (1 + z_tol) adds llrintf(ldexpf(x, shift)) for x = w and for
 *                         x = w * clamp(c, +-value_bound) / value_bound per channel to the pixel's words of acc (64-bit integer
 *                         atomicAdd, two's complement).  n_max: the caller's bound on the number of points one view receives
 *                         over ALL accumulate calls into this workspace; shift + ceil_log2(n_max) <= 62 is required, which
 *                         makes overflow impossible (every term is at most 2^shift in magnitude).  May be called several
 *                         times (chunks of source images) between one dvd_splat_zmin pass over all of them and the resolve.
 *   dvd_splat_resolve     per target pixel: weight [V,1,H,W] = acc_w * 2^-shift; hit uint8 [V,H,W] = weight >= w_min; image
 *                         [V,C,H,W] = value_bound * acc_c / acc_w where hit, else fill; depth [V,1,H,W] = zmin where hit, else
 *                         0.  Plain stores, one writer per element; 4 pixels per thread where W % 4 == 0 and the bases are
 *                         16-byte aligned.
 * Integer min and add commute: the result is bitwise independent of source order, launch order and run.  Refused with
 * DVD_EINVAL before any HIP call: a null pointer, C outside 1..8, H or W < 2, S or V outside 1..65535, z_near < 0, z_tol < 0,
 * w_tap outside (0, 0.25], w_min <= 0, value_bound <= 0, shift outside 1..40 or too large for n_max.  Bytes are counted
 * under DVD_BYTES_GEOMETRY. */
size_t dvd_splat_workspace_bytes(int V, int C, int H, int W);
int dvd_splat_zmin(const float* points, int points_planar, const float* values, const unsigned char* valid, const int* view,
                   const float* R, const float* t, const float* K_T, int V, unsigned int* zbuf, int S, int C, int H, int W,
                   float z_near, float w_tap, dvd_stream_t stream);
int dvd_splat_accumulate(const float* points, int points_planar, const float* values, const unsigned char* valid,
                         const int* view, const float* R, const float* t, const float* K_T, int V, const unsigned int* zbuf,
                         unsigned long long* acc, int S, int C, int H, int W, float z_near, float z_tol, float w_tap,
                         float value_bound, int shift, long long n_max, dvd_stream_t stream);
int dvd_splat_resolve(const unsigned int* zbuf, const unsigned long long* acc, int V, int C, int H, int W, int shift,
                      float w_min, float value_bound, float fill, float* image, float* depth, float* weight,
                      unsigned char* hit, dvd_stream_t stream);

/* A finished optimisation scored along its tracks (an addition within ABI 8; csrc/eval.hip, models/evaluate.py): frame f
 * pushed along the scene-flow field to the time of frame g should agree with frame g wherever it is visible there.
 *   points     [T, B, 3, H, W], planar: row r of image b holds the world points of frame source[b]'s pixels at the time of
 *              frame g = source[b] + k_first + r (the slab models/tracks.py integrates; k_first = 1 skips its row 0)
 *   source     DEVICE array of B ints;  k_first  0 or 1.  Where g >= N (or source[b] < 0) the row is dead: it reads nothing,
 *              adds nothing, and its maps are -1.
 *   R, t, K_T  the per-frame tables [N, 3, 3], [N, 3], [N, 3, 3] as dvd_track_project takes them
 *   depth_all  [N, 1, H, W] refined depth;  img_all  [N, 3, H, W] colours
 *   pair_row   DEVICE int [T, B]: the row of the flow pair (source[b], g) in flow_1_2 / mask, or -1 (a row >= P counts as -1);
 *   flow_1_2   [P, H, W, 2];  mask  uint8 [P, H, W], 0 = valid.  All three or none.
 * Per point, in fp32 with the operations of dvd_track_project (the same u, v, z and taps, bit for bit):
 *   inside     z > 0 && 0 <= u <= W - 1 && 0 <= v <= H - 1;   d = depth_all[g] at (u, v) (bilinear, border) where inside
 *   occluded   z > d * (1 + z_tol);   seen = inside && !occluded
 *   rel        min(|z - d| / max(d, d_min), 1)                                     where seen
 *   photo      min((|c0 - o0| + |c1 - o1| + |c2 - o2|) / 3, 1024), c = img_all[g] at (u, v) with d's taps and weights,
 *              o = the pixel's own colour in img_all[source[b]]                    where seen
 *   epe        min(hypot((u - x) - flow.x, (v - y) - flow.y), 1024)                where pair_row >= 0, mask == 0 and z > 0
 *   sums       long long [T, B, 6], ACCUMULATED into (the caller clears it): n_inside, n_occluded, sum q(rel), sum q(photo),
 *              n_flow, sum q(epe), q(x) = llrint((double)x * 2^shift).  1 <= shift <= min(32, 62 - 10 - ceil_log2(H * W)), so
 *              a row cannot overflow.  Consecutive steps are sums_step_stride elements apart (>= B * 6): a launch over a
 *              chunk of images may write its columns of a larger tensor.
 *   maps       float [T, B, 3, H, W] or NULL: rel, photo, epe -- the very fp32 values that were quantised -- and -1 where the
 *              point does not count; steps maps_step_stride elements apart (>= B * 3 * H * W).
 * The block reduces in 64-bit integers (registers, a shuffle tree, LDS) and issues at most six integer atomicAdd: the sums
 * are bitwise reproducible and independent of the grid.  Refused with DVD_EINVAL before any HIP call: a null pointer, the
 * three flow arguments not all-or-none, T or B outside 1..65535, H or W < 2, H * W >= 2^30, k_first not 0 or 1, z_tol < 0 or
 * NaN, d_min <= 0 or NaN, a shift outside its range, a step stride below its row.  Bytes are counted under DVD_BYTES_GEOMETRY. */
int dvd_eval_tracks(const float* points, const int* source, int k_first, const float* R, const float* t, const float* K_T,
                    int N, const float* depth_all, const float* img_all, const int* pair_row, const float* flow_1_2,
                    const unsigned char* mask, int P, float z_tol, float d_min, int shift, long long* sums,
                    long long sums_step_stride, float* maps, long long maps_step_stride, int T, int B, int H, int W,
                    dvd_stream_t stream);

/* The exact median of num / den per segment (an addition within ABI 8; csrc/select.hip): the reference's
 * `np.median(nn_depth[idx, idy] / mvs_depth[idx, idy])` over `np.where(mvs_depth > 1e-3)`
 * (scripts/preprocess/shutterstock/generate_frame_midas.py:153-160), and the median alignment of models/score_depth.py.
 *   num, den   float [S, L]: S contiguous segments of L elements;  mask  uint8 [S, L] or NULL
 *   An element is selected iff den > den_min (a NaN fails) and its mask byte, if given, is non-zero; its key is the correctly
 *   rounded fp32 quotient num / den.
 *   median     float [S]: numpy's median of the selected quotients, bit for bit -- with the n values sorted, v[(n-1)/2] for
 *              odd n, (v[n/2-1] + v[n/2]) / 2 with the sum formed first in fp32 for even n, NaN for n = 0, NaN if any selected
 *              quotient is a NaN; +-inf sort as the extremes.   count  long long [S]: n.
 *   workspace  at least S * DVD_RATIO_MEDIAN_WORKSPACE_PER_SEGMENT bytes of device memory, 4-byte aligned; cleared by the entry.
 * A most-significant-digit radix select (4 passes of 8 bits) that follows both middle ranks at once: per pass a histogram
 * kernel re-reads num, den and the mask (no key array is written) and a one-block-per-segment kernel fixes the next digit on the
 * device.  Nothing synchronises with the host; only integers are added, so the result is the same bits from run to run and for
 * every grid.  Refused with DVD_EINVAL before any HIP call: a null pointer, S outside 1..65535, L < 1, S * L >= 2^31, a NaN
 * den_min, a misaligned pointer, a workspace that is too small.  Bytes are counted under DVD_BYTES_GEOMETRY. */
#define DVD_RATIO_MEDIAN_WORKSPACE_PER_SEGMENT 8224
int dvd_ratio_median(const float* num, const float* den, const unsigned char* mask, float den_min, int S, long long L,
                     float* median, long long* count, void* workspace, size_t workspace_bytes, dvd_stream_t stream);

/* A predicted depth scored against its ground truth (an addition within ABI 8; csrc/depth_score.hip, models/score_depth.py):
 * the error terms behind abs-rel, sq-rel, RMSE, log-RMSE and the delta < 1.25^k accuracies, where the reference's validation
 * (models/scene_flow_motion_field.py `_vali_on_batch`, disp_vali's gt > 1e-2) knows one scalar.
 *   pred, gt   float [N, 1, H, W];  scale  DEVICE float [N] (dvd_ratio_median's output, or ones)
 *   seg        float [N, H, W] or NULL;  mask  uint8 [N, H, W] or NULL, non-zero = allowed
 * Per pixel in fp32: q = scale[n] * pred; it counts iff gt > g_min, pred > 0, q is finite and the mask allows it.  d = q - g,
 *   abs_rel = min(|d| / g, 1024), sq_rel = min(d * d / g, 1024), sq = min(d * d, 1024),
 *   l = min(max(logf(q) - logf(g), -32), 32), l2 = min(l * l, 1024), delta_k = max(q / g, g / q) < 1.25^k for k = 1, 2, 3.
 *   sums       long long [N, 3, 9], ACCUMULATED into (the caller clears it).  Row 0: every counted pixel, row 1: seg <= 0.5
 *              (static), row 2: seg > 0.5 (dynamic); without seg rows 1 and 2 receive nothing.  Words: n, sum q(abs_rel),
 *              sum q(sq_rel), sum q(sq), sum q(l2), sum q(l) (signed, two's complement), n_delta1, n_delta2, n_delta3, with
 *              q(x) = llrint((double)x * 2^shift).  1 <= shift <= min(32, 62 - 10 - ceil_log2(N * H * W)): neither a row nor the
 *              rows of a video pooled can overflow.
 *   maps       float [N, 3, H, W] or NULL: abs_rel, sq, l -- the very fp32 values that were quantised -- and 0 where the pixel
 *              does not count;  counted  uint8 [N, H, W] (with maps, both or none): 1 where it counts.
 * The block reduces in 64-bit integers (registers, a shuffle tree, LDS) and issues at most nine integer atomicAdd per region:
 * the sums are bitwise reproducible and independent of the grid.  Refused with DVD_EINVAL before any HIP call: a null pointer,
 * maps without counted or the reverse, N outside 1..65535, H or W < 1, H * W >= 2^30, g_min < 0 or not finite, a shift outside
 * its range, a misaligned pointer.  Bytes are counted under DVD_BYTES_GEOMETRY. */
int dvd_depth_score(const float* pred, const float* gt, const float* scale, const float* seg, const unsigned char* mask,
                    float g_min, int shift, long long* sums, float* maps, unsigned char* counted, int N, int H, int W,
                    dvd_stream_t stream);

/* Push-pull hole filling (additions within ABI 8; csrc/fill.hip, ops.fill_holes, Model.render(inpaint=True),
 * preprocess.triangulate_depth(densify=True)): what a splat or a triangulation left empty, from a 2x pyramid of what it did not.
 *   values  float [V, C, H, W], 1 <= C <= 8;  known  uint8 [V, H, W];  bias  float [V, 1, H, W] or NULL;  power 0 .. 4
 *   level 0   a = known != 0 ? bias^power : 0, the power by repeated multiplication (1 without bias or with power 0).  A pixel
 *             whose a is not finite or not > 0 is unknown, and so is one whose bias (where it is used) is not > 0, which an
 *             even power would hide; the value of an unknown pixel is never read into a result.
 *   pull      level l + 1 is (ceil(H_l / 2), ceil(W_l / 2)), up to 1 x 1.  Over the children (2y+dy, 2x+dx) inside the level, in
 *             the order (0,0) (0,1) (1,0) (1,1):  A = sum a_c, n = #{a_c > 0};  n > 0: v' = (sum a_c v_c) / A, a' = A / n;
 *             else v' = a' = 0.  (The mean as the carried weight keeps a within the range of the level-0 weights.)
 *   push      a pixel with a_l > 0 keeps v_l; any other takes the bilinear sample of the completed level above at
 *             ((y + .5) / 2 - .5, (x + .5) / 2 - .5): 0.75 of the parent x >> 1 and 0.25 of its neighbour on the pixel's side,
 *             the neighbour's index clamped to the level; horizontal pairs first, then the vertical pair.
 *   out_values  the completed values; known pixels are the input bits.  out_values == values is allowed (any other overlap is not).
 *   out_level   uint8 [V, H, W]: 0 known, k >= 1 the lowest level at which an ancestor (y >> k, x >> k) is known, 255 for a
 *               view without a known pixel, whose values all become `fill`.
 * Every statement is a separate fp32 operation in the order written, sums from left to right, divisions IEEE.  Three launches
 * whatever V, H and W (32 x 32 tiles pull levels 1 .. 5 into the workspace; one block per view finishes level 5 and above in
 * LDS; the tiles push back down); no atomics, nothing synchronises with the host.  A view's result does not depend on V or on
 * the views it shares a call with, and two runs give the same bits.  Vector accesses need W % 4 == 0 and 16-byte aligned float
 * (4-byte aligned byte) tensors; anything else takes the one-pixel path.
 *   workspace   dvd_fill_workspace_bytes(V, C, H, W) bytes, 4-byte aligned, uncleared: 4 V (C + 1) sum_{l=1..5} H_l W_l.  The
 *               function returns 0 for arguments dvd_fill_holes refuses.
 * DVD_EINVAL before any HIP call: a null pointer (bias excepted), power outside 0 .. 4, V outside 1 .. 65535, C outside 1 .. 8,
 * H or W < 1, H * W >= 2^30, ceil(H / 32) * ceil(W / 32) > 2048 (the one-block-per-view kernel holds level 5 and above in
 * 148,032 of the 163,840 bytes of LDS), a misaligned float pointer.  Weights are expected below FLT_MAX / 4.  Bytes are counted
 * under DVD_BYTES_GEOMETRY. */
size_t dvd_fill_workspace_bytes(int V, int C, int H, int W);
int dvd_fill_holes(const float* values, const unsigned char* known, const float* bias, int power, float fill, int V, int C,
                   int H, int W, float* out_values, unsigned char* out_level, void* workspace, dvd_stream_t stream);

/* Query-point tracks (additions within ABI 8; csrc/point_track.hip, models/point_tracks.py): Q chosen, sub-pixel points of any
 * frames instead of every pixel of whole frames, and their score against annotated trajectories (the TAP-Vid protocol).  A
 * slab row is [3, Q] -- what dvd_sf_mlp_fwd takes as n_pix = Q points with a time stamp each -- so the queries integrate in
 * one launch per step, forwards and (dvd_track_invert_update) backwards.
 *   frame      DEVICE int [Q]: the frame a query lives in;  xy  float [Q, 2]: its position there, pixel centres at integers
 *   tables     as datasets/frame_store.py keeps them: R_T [N,3,3] camera->world, t [N,3], K_inv_T [N,3,3], ts_vali [N] for the
 *              seed (dvd_unproject_fwd's R, t, K_inv per frame); R [N,3,3] world->camera, t, K_T [N,3,3] for the projection
 *   depth_all  [N, 1, H, W]
 * dvd_point_seed: d = depth_all[frame] at (x, y) by direct bilinear taps -- x clamped to [0, W-1] (a NaN becomes 0), x0 =
 * floorf(x), weights from x - x0, a tap past the east or south edge reads as 0, the taps combined as dvd_track_project combines
 * them -- so the weights at an integer position are exactly (1, 0, 0, 0); then P = (d * ((x, y, 1) @ K_inv)) @ R + t by the
 * device function dvd_unproject_fwd runs per pixel: an integer query has that pixel's bits.
 *   points     [3, Q] planar;  t_out  [Q] = ts_vali[frame], with ts_vali both or none (a time-independent field);
 *   ok         uint8 [Q] = frame in 0 .. N-1 && d finite and > 0 && 0 <= x <= W-1 && 0 <= y <= H-1; otherwise the point is 0
 *              (and t_out 0 where the frame is no frame)
 * dvd_point_project: row j of query q looks into frame g = frame[q] + j + k0 with the functions of dvd_track_project_from and
 * the query's own (x, y) as the source pixel: an integer query has the bits that entry gives the pixel.
 *   points     [T1, 3, Q];  ok  uint8 [Q] or NULL (every query counts)
 *   uv [T1, Q, 2], z, depth_at [T1, Q], inside uint8 [T1, Q]   as dvd_track_project defines them
 *   visible    uint8 [T1, Q] = inside && !(z > depth_at * (1 + z_tol)), 1 + z_tol formed once in fp32 (dvd_eval_tracks' rule)
 *   target     int [T1, Q] = g, or -1
 * A row whose g is outside 0 .. N-1, whose frame is, or whose query is not ok writes zeros and -1 and reads nothing else.
 * dvd_point_score: predictions (uv, visible, target of dvd_point_project) against
 *   gt_uv      float [Q, N, 2], frame-major;  gt_state  uint8 [Q, N]: 0 visible, 1 occluded, >= 2 not annotated
 * Row j of query q is an evaluation point iff 0 <= target < N, j != origin (-1: no origin row) and gt_state[q][target] < 2.
 * In fp32, every operation separate: du = (u - gu) * sx, dv = (v - gv) * sy, e2 = du * du + dv * dv, within_i = e2 < thr2[i]
 * (strict; a NaN is never within), vis_gt = gt_state == 0.
 *   thr2       HOST array of 5 squared thresholds, finite, positive, ascending
 *   sums       long long [T1, 19], ACCUMULATED into (the caller clears it), per slab row: n_eval, n_gt_visible, n_occ_agree
 *              (visible == vis_gt), 5 x n_within (vis_gt && within), 5 x n_tp (vis_gt && within && visible), 5 x n_fp (visible
 *              && (!vis_gt || !within)), sum over vis_gt points of q(min(sqrt(e2), 1024)), q(x) = llrint((double)x * 2^shift),
 *              the square root correctly rounded, a NaN taken as the cap.  1 <= shift <= min(32, 62 - 10 - ceil_log2(Q)).
 * One point per thread, plain stores, one writer per element; the score reduces in 64-bit integers (registers, a shuffle tree,
 * LDS) and issues at most 19 integer atomicAdd per block: the same bits for any grid.  DVD_EINVAL before any HIP call: a null
 * pointer (ok, ts_vali / t_out excepted), T1 outside 1..65535, Q outside 1..2^30-1, N < 1, H or W < 2, H * W >= 2^30, |k0| >=
 * 2^30, z_tol < 0 or not finite, origin outside -1..T1-1, sx or sy not finite and > 0, bad thresholds, a shift outside its
 * range.  Bytes are counted under DVD_BYTES_GEOMETRY. */
int dvd_point_seed(const int* frame, const float* xy, const float* depth_all, const float* R_T, const float* t,
                   const float* K_inv_T, const float* ts_vali, int N, float* points, float* t_out, unsigned char* ok, int Q,
                   int H, int W, dvd_stream_t stream);
int dvd_point_project(const float* points, const int* frame, const float* xy, const unsigned char* ok, int k0, const float* R,
                      const float* t, const float* K_T, const float* depth_all, int N, float z_tol, float* uv, float* z,
                      float* depth_at, unsigned char* inside, unsigned char* visible, int* target, int T1, int Q, int H, int W,
                      dvd_stream_t stream);
int dvd_point_score(const float* uv, const unsigned char* visible, const int* target, int origin, const float* gt_uv,
                    const unsigned char* gt_state, int N, float sx, float sy, const float* thr2, int shift, long long* sums,
                    int T1, int Q, dvd_stream_t stream);

/* Stored optical flows chained into frame gaps nobody computed (an addition within ABI 8; csrc/flow_chain.hip, ops.flow_chain,
 * preprocess.chain_flows): a gap-g flow is g gap-1 flows -- or fewer, longer stored ones -- followed one after another.
 *   flow_1_2, flow_2_1   float [P, H, W, 2];  mask_1, mask_2  uint8 [P, H, W], 0 = valid  (a FrameStore's tensors)
 *   links      DEVICE int [B, L, 2], rows (pair, dir), 1 <= L <= 32.  dir 0 follows flow_1_2[pair], whose validity is
 *              mask_2[pair]; dir 1 follows flow_2_1[pair] with mask_1[pair] (dvd_triangulate's convention).  pair = -1 ends a
 *              chain: every later link of that row is ignored.
 *   live_links the number of links before the rows' ends.  The table is on the device, so the entry cannot count them: the value
 *              only feeds dvd_byte_counters, the kernel never reads it, and the caller answers for it (ops.flow_chain counts
 *              them on the host copy it uploads).
 * One thread per pixel x0 = (u, v) of chain b walks the links in order from x_0 = x0.  Link k (0-based) at x_k = (px, py), every
 * multiply and add a separate fp32 operation:
 *   it breaks unless 0 <= px <= W-1 && 0 <= py <= H-1 (a NaN fails); a pair outside -1 .. P-1 breaks it and reads nothing
 *   ix = floorf(px), iy = floorf(py), wx = px - ix, wy = py - iy; the taps (ix, iy), (ix+1, iy), (ix, iy+1), (ix+1, iy+1) have
 *   the weights (1-wx)(1-wy), wx(1-wy), (1-wx)wy, wx wy.  A tap whose weight is exactly 0 is neither read nor tested, which
 *   holds a position on the last row or column inside the image.
 *   it breaks if the link's mask is non-zero at any tap that is read
 *   f = ((t00 * w00 + t10 * w10) + t01 * w01) + t11 * w11 per component; an unread tap contributes 0 * w, which is +0
 *   x_{k+1} = x_k + f; it breaks if a component of x_{k+1} is a NaN or an Inf, so that no output ever is one
 *   flow_out   float [L, B, H, W, 2], row k = x_{k+1} - x0; after a break the last value before it, (0, 0) if link 0 broke.
 *              Rows are flow_stride floats apart (>= B * H * W * 2, even).
 *   broken     uint8 [L, B, H, W]: 0 while the chain is whole, then 1 + the index of the link that broke, in all later rows
 *   Rows past a chain's end are 0 in flow_out and 255 in broken.
 * No atomics, one writer per element, plain vector stores: the same inputs give the same bits.  Grid (ceil(H W / 256), B).
 * DVD_EINVAL before any HIP call: a null pointer, L outside 1..32, B outside 1..65535, H or W < 2, H * W >= 2^30, P < 1, a stride
 * below B * H * W * 2 or odd, live_links outside 0 .. B * L, a misaligned pointer.  Bytes are counted under DVD_BYTES_GEOMETRY. */
int dvd_flow_chain(const float* flow_1_2, const float* flow_2_1, const unsigned char* mask_1, const unsigned char* mask_2, int P,
                   const int* links, long long live_links, float* flow_out, long long flow_stride, unsigned char* broken, int L,
                   int B, int H, int W, dvd_stream_t stream);

/* Normal equations of the camera refinement from stored flow and depth (additions within ABI 8; csrc/pose.hip,
 * ops.pose_normal_eq, preprocess.refine_cameras): one launch reduces, per observation row, the Gauss-Newton system of the
 * robust reprojection error of a stored flow in the poses of its two frames and the depth scale of the first.
 *   rows     DEVICE int32 [R, 4], rows (pair, a, b, dir): dir 0 reads flow_1_2[pair] with mask_2[pair], dir != 0 flow_2_1[pair]
 *            with mask_1[pair] (dvd_triangulate's pairing); a is the frame the flow leaves, b the one it reaches
 *   flows    fp32 [P, H, W, 2];  masks uint8 [P, H, W], 0 = valid;  depth fp32 [N, H, W] (planar depth per frame);
 *   weight   fp32 [N, H, W] or null (all ones): what is static;  scale fp32 [N]: s = exp(sigma), the per-frame depth scale
 *   R, t, K_T, K_inv_T   the per-frame tables of dvd_triangulate (R camera to world, c = t)
 * Per pixel x = (u, v, 1) of frame a, every multiply and add a separate fp32 operation, every three-term sum as (p0 + p1) + p2,
 * the divisions IEEE:
 *   ray = K_a^-1 x;  Ds = D_a(x) * s_a;  P = Ds * ray;  X = R_a P;  Z = X + (c_a - c_b);  Y = R_b^T Z;  q = K_b Y
 *   proj = q.xy / q.z;  x' = x.xy + flow;  r = proj - x'
 *   considered  mask byte == 0 && D > 0 && D <= FLT_MAX && weight > 0 && 0 <= x'0 <= W-1 && 0 <= x'1 <= H-1
 *   live        considered && q.z >= z_near            (a NaN fails every comparison)
 * A live observation enters with Huber's loss on |r|, threshold huber in pixels: rho = |r|^2 / 2 and IRLS weight 1 inside,
 * huber (|r| - huber / 2) and huber / |r| outside, both times weight_a(x) (w below is that product), and with the 2 x 13 Jacobian
 * of r in the local unknowns [tau_a, omega_a, sigma_a, tau_b, omega_b] (c += R tau, R <- R Exp(omega), s = exp(sigma)):
 *   J = Pi K_b [ M | -M [P]x | M P | -I | [Y]x ],  M = R_b^T R_a,  Pi = (1 / q.z) [[1, 0, -proj_0], [0, 1, -proj_1]]
 * Outputs, per row:
 *   sums    float64 [R, 106]: the upper triangle of J^T w J row-major (91), J^T w r (13), the cost = sum of weight * rho over
 *           the live + penalty * (sum of weight over the considered that are not live), and sum of w |r|^2 over the live
 *   wsum    float64 [R]: sum of w over the live;   counts  int64 [R, 2]: the live, and the considered that are not live
 *   resid   fp32 [R, H, W, 2] and gate uint8 [R, H, W], both or neither (null): r where live, (0, 0) elsewhere; 0 not
 *           considered, 1 live, 2 considered but q.z < z_near
 * penalty is the cost, per unit weight, of an observation a step has pushed behind its camera (preprocess passes Huber's rho of
 * a residual as long as the image's diagonal), so that no step lowers the cost that way.  A thread sums at most 16 pixels in fp32,
 * the wave's 64 lanes are added in fp32, everything after in float64: one partial per (row, block of 4096 pixels) in the
 * workspace (dvd_pose_workspace_bytes(R, H, W) bytes, 8-byte aligned), summed by a second kernel in ascending block order.  No
 * atomics, one writer per element: the same inputs give the same bits.  A row whose pair is outside 0 .. P-1 or whose frames are
 * outside 0 .. N-1 is skipped: zero sums and counts (and zero maps).  Grid (ceil(H W / 4096), R).  DVD_EINVAL before any HIP
 * call: a null pointer, one of resid / gate without the other, R outside 1 .. 65535, H * W >= 2^30, P < 1, N < 1, huber or z_near
 * not positive and finite, penalty negative or not finite, a workspace that is too small or misaligned.  Bytes are counted
 * under DVD_BYTES_GEOMETRY: R H W (8 flow + 1 mask + 4 depth + 4 weight if given + 9 with the maps). */
size_t dvd_pose_workspace_bytes(int R, int H, int W);
int dvd_pose_normal_eq(const float* flow_1_2, const float* flow_2_1, const unsigned char* mask_1, const unsigned char* mask_2, int P,
                       const float* depth, const float* weight, const float* R, const float* t, const float* K_T,
                       const float* K_inv_T, const float* scale, int N, const int* rows, float huber, float z_near, float penalty,
                       void* workspace, size_t workspace_bytes, double* sums, double* wsum, long long* counts, float* resid,
                       unsigned char* gate, int n_rows, int H, int W, dvd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DVD_HIP_H */
