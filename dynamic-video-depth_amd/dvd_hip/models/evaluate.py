"""A finished optimisation scored along its tracks: a number that needs no ground truth.

Frame f rendered at the time and camera of frame g should look like frame g wherever it is visible.  The pixels of every start
frame are un-projected with their refined depth, pushed along the scene-flow field by the Euler chain of models/tracks.py, and
every step is compared with the frame it lands in by ONE fused kernel (ops.eval_tracks, csrc/eval.hip): the depth it finds
there (depth_rel), the colour it finds there (photo), how much of it is hidden behind a nearer surface (occluded) and, where the
store holds the optical flow of the pair, how far the induced motion is from that flow (flow_epe) -- the quantity the flow loss
of the training minimises, now along the whole track.

  per chunk of start frames   tracks.start_slab -> tracks.integrate -> one ops.eval_tracks over rows 1 .. n_steps, reduced on
                              chip to six 64-bit integers per (step, start frame) in the caller-order rows of one tensor
  afterwards                  a handful of float64 divisions on [K,B] tensors, and _vali_on_batch's disparity MSE per frame

`evaluate_plan` is the host-side half; `evaluate` is what `Model.evaluate` runs.  Nothing here synchronises with the device.
The sums are integers added by integer atomics, so the result is the same bits from run to run and for every chunk size.
"""
import numpy as np
import torch

from .. import ops
from . import tracks


def evaluate_plan(cat, start, n_steps):
    """(steps_valid, pair_row): track_plan's steps with a target frame per start frame, and the int32 [n_steps, B] table of
    the row of the flow pair (start[b], start[b] + k) in the store's flow tensors for step k = row + 1, -1 where the catalogue
    holds no such pair (a gap it was not built with, the last pair of a gap, which the writer leaves out, or a step past the
    end of the video).  ValueError in the cases of track_plan."""
    valid = tracks.track_plan(cat.n_frames, start, n_steps)
    start = [int(s) for s in (start.cpu().tolist() if torch.is_tensor(start) else np.asarray(start).reshape(-1).tolist())]
    rows = {p: j for j, p in enumerate(cat.pairs)}
    table = np.full((int(n_steps), len(start)), -1, dtype=np.int32)
    for b, s in enumerate(start):
        for k in range(1, valid[b] + 1):
            table[k - 1, b] = rows.get((s, s + k), -1)
    return valid, table


def _mean(total, count, shift):
    """total * 2^-shift / count in float64, NaN where count is 0."""
    nan = torch.full((), float('nan'), dtype=torch.float64, device=total.device)
    return torch.where(count > 0, total.double() * (2.0 ** -shift) / count.double(), nan)


def disparity_mse(depth, gt):
    """Per frame, _vali_on_batch's score: mse_loss(depth2disp(depth) * vali, depth2disp(gt) * vali), vali = gt > 1e-2, the mean
    over all pixels -- in float64.  depth, gt: [N,1,H,W] -> [N]."""
    def disp(d):
        ok = (d > 1e-2).double()
        return (1 / (d + (1 - ok) * 1e-8)) * ok
    depth, gt = depth.double(), gt.double()
    vali = (gt > 1e-2).double()
    return ((disp(depth) * vali - disp(gt) * vali) ** 2).flatten(1).mean(1)


def evaluate(model, store, start=None, n_steps=None, depth=None, chunk=None, maps=False, z_tol=0.05):
    """Model.evaluate: see there."""
    opt = model.opt
    if opt.use_cnn:
        raise NotImplementedError('Model.evaluate integrates the scene-flow MLP kernels; the --use_cnn U-Net branch has no '
                                  'stash-free forward to chain and is not supported')
    cat = store.cat
    N, H, W = cat.n_frames, store.H, store.W
    if start is None:
        start = list(range(N - 1))
    if n_steps is None:
        n_steps = max(cat.gaps)
    valid, table = evaluate_plan(cat, start, n_steps)
    start = [int(s) for s in (start.cpu().tolist() if torch.is_tensor(start) else np.asarray(start).reshape(-1).tolist())]
    B, K = len(start), int(n_steps)
    if chunk is None:
        chunk = tracks.default_chunk(K, H, W)
    if isinstance(chunk, bool) or int(chunk) != chunk or chunk < 1:
        raise ValueError('evaluate: chunk must be a positive number of start frames, got %r' % (chunk,))
    chunk = int(chunk)
    dev, T = store.device, store.tables
    if depth is None:
        depth = model.video_depth(store.frames(model._chunk()))
    depth = ops._dev32(depth, 'depth')
    if tuple(depth.shape) != (N, 1, H, W):
        raise ValueError('evaluate: depth must be [%d,1,%d,%d], got %s' % (N, H, W, tuple(depth.shape)))
    model.eval()
    with torch.no_grad():
        sums = torch.zeros(K, B, 6, device=dev, dtype=torch.int64)
        point_maps = torch.empty(K, B, 3, H, W, device=dev) if maps else None
        source = torch.tensor(start, dtype=torch.int32).to(dev, non_blocking=True)
        params = model.net_sceneflow.parameter_list()
        model._mlp.pack(params[0::2], params[1::2])
        for b0 in range(0, B, chunk):
            b1 = min(b0 + chunk, B)
            points, ts = tracks.start_slab(model, store, depth, start[b0:b1], K + 1)
            tracks.integrate(model._mlp, points, ts, valid[b0:b1], 1.0 / (N + 0.0), 1.0 / opt.sf_mag_div, b1 - b0)
            ops.eval_tracks(points[1:], source[b0:b1], T, depth, store.img, k_first=1,
                            pairs=(np.ascontiguousarray(table[:, b0:b1]), store.flow_1_2, store.mask_2), z_tol=z_tol,
                            sums=sums[:, b0:b1], maps=point_maps[:, b0:b1] if maps else False,
                            host_source=start[b0:b1])
        shift = ops.eval_shift(H * W)
        n_inside, n_occluded, n_flow = sums[..., 0], sums[..., 1], sums[..., 4]
        seen = n_inside - n_occluded
        out = {'sums': sums, 'shift': shift, 'n_inside': n_inside, 'n_occluded': n_occluded, 'n_flow': n_flow,
               'depth_rel': _mean(sums[..., 2], seen, shift), 'photo': _mean(sums[..., 3], seen, shift),
               'flow_epe': _mean(sums[..., 5], n_flow, shift)}
        pooled = sums.sum(1)
        p_seen = pooled[:, 0] - pooled[:, 1]
        out['by_step'] = {'depth_rel': _mean(pooled[:, 2], p_seen, shift), 'photo': _mean(pooled[:, 3], p_seen, shift),
                          'flow_epe': _mean(pooled[:, 5], pooled[:, 4], shift),
                          'occluded': _mean(pooled[:, 1], pooled[:, 0], 0)}
        out['disp_mse'] = disparity_mse(depth, store.depth_mvs)
    if maps:
        out['maps'] = point_maps
    out['steps_valid'] = torch.tensor(valid, dtype=torch.int32).to(dev, non_blocking=True)
    return out
