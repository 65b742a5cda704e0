"""A refined depth scored against the ground truth of the frame files: the numbers a paper reports.

`Model.evaluate` is a number that needs no ground truth; this is its converse.  Every frame file carries `depth_mvs`, which the
frame store holds in HBM.  The prediction is aligned to it by one scale -- a median of ratios, per video or per frame, from the
exact device median of ops.ratio_median (csrc/select.hip) -- and ONE fused kernel (ops.depth_score, csrc/depth_score.hip) reduces
abs-rel, sq-rel, RMSE, log-RMSE, the scale-invariant log error and the delta < 1.25^k accuracies to 64-bit integer sums per frame
and region (all / static / dynamic pixels by the store's motion segmentation).

  alignment   the uint8 mask of the pixels that can count (gt > g_min, and the caller's mask) is one elementwise pass; the median
              of gt / pred over them is four histogram passes over gt and pred; its scale stays on the device
  score       one pass over pred, gt (and seg, mask) -> sums [N,3,9]
  afterwards  a handful of float64 divisions on [N,3] and [3] tensors

Nothing here synchronises with the device.  The sums are integers added by integer atomics, so the result is the same bits from
run to run.
"""
import torch

from .. import ops

ALIGN = ('none', 'median_frame', 'median_video')
G_MIN = 1e-2            # disp_vali's threshold on the ground truth


def _quotient(total, count, shift):
    """total * 2^-shift / count in float64, NaN where count is 0."""
    nan = torch.full((), float('nan'), dtype=torch.float64, device=total.device)
    return torch.where(count > 0, total.double() * (2.0 ** -shift) / count.double(), nan)


def derive(sums, shift):
    """The reported quantities from sums [...,9] (ops.SCORE_SUMS): float64 tensors of sums' leading shape, NaN where n = 0."""
    n = sums[..., 0]
    mean_l2, mean_l = _quotient(sums[..., 4], n, shift), _quotient(sums[..., 5], n, shift)
    return {'abs_rel': _quotient(sums[..., 1], n, shift), 'sq_rel': _quotient(sums[..., 2], n, shift),
            'rmse': _quotient(sums[..., 3], n, shift).sqrt(), 'rmse_log': mean_l2.sqrt(), 'silog': mean_l2 - mean_l * mean_l,
            'd1': _quotient(sums[..., 6], n, 0), 'd2': _quotient(sums[..., 7], n, 0), 'd3': _quotient(sums[..., 8], n, 0)}


def align_scale(depth, gt, align, mask=None, g_min=G_MIN):
    """The scale [N] fp32 on the device that `align` gives the prediction: ones, the median of gt / depth over every frame's
    countable pixels (gt > g_min, depth > 0, the mask), or that median over the pixels of all frames, repeated."""
    N, _, H, W = depth.shape
    if align == 'none':
        return torch.ones(N, device=depth.device, dtype=torch.float32)
    keep = gt > g_min
    if mask is not None:
        keep = keep & (mask != 0).reshape(gt.shape)
    keep = keep.to(torch.uint8)
    if align == 'median_frame':
        return ops.ratio_median(gt.reshape(N, H * W), depth.reshape(N, H * W), mask=keep.reshape(N, H * W))['median']
    return ops.ratio_median(gt.reshape(1, -1), depth.reshape(1, -1), mask=keep.reshape(1, -1))['median'].expand(N).contiguous()


def score_depth(model, store, depth=None, gt=None, align='median_video', regions=True, mask=None, maps=False):
    """Model.score_depth: see there."""
    if align not in ALIGN:
        raise ValueError('score_depth: align must be one of %s, got %r' % (', '.join(ALIGN), align))
    N, H, W = store.cat.n_frames, store.H, store.W
    if depth is None:
        depth = model.video_depth(store.frames(model._chunk()))
    if gt is None:
        gt = store.depth_mvs
    depth, gt = ops._dev32(depth, 'depth'), ops._dev32(gt, 'gt')
    for name, t in (('depth', depth), ('gt', gt)):
        if tuple(t.shape) != (N, 1, H, W):
            raise ValueError('score_depth: %s must be [%d,1,%d,%d], got %s' % (name, N, H, W, tuple(t.shape)))
    if torch.is_tensor(mask) and mask.dtype == torch.bool:       # (preprocess.triangulate_depth's 'static': the same bytes, 0 / 1)
        mask = mask.view(torch.uint8)
    if mask is not None and not (torch.is_tensor(mask) and mask.dtype == torch.uint8 and tuple(mask.shape) == (N, H, W)):
        raise ValueError('score_depth: mask must be a uint8 or bool tensor [%d,%d,%d]' % (N, H, W))
    seg = store.motion_seg if regions else None
    with torch.no_grad():
        scale = align_scale(depth, gt, align, mask=mask)
        res = ops.depth_score(depth, gt, scale, seg=seg, mask=mask, g_min=G_MIN, maps=maps)
        sums, shift = res['sums'], res['shift']
        # (without a motion segmentation rows 1 and 2 stay zero: n = 0 there, and every derived quantity is NaN)
        out = {'sums': sums, 'shift': shift, 'scale': scale, 'n': sums[..., 0]}
        out.update(derive(sums, shift))
        pooled = sums.sum(0)
        out['video'] = dict(derive(pooled, shift), n=pooled[..., 0])
    if maps:
        out['maps'], out['counted'] = res['maps'], res['counted']
    return out
