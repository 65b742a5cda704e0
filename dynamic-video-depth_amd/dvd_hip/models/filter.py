"""Geometry-aware temporal depth filter: the refined depth of a video made consistent along its own 3D tracks.

After the optimisation every frame's refined depth is still an independent network output; Model.evaluate's depth_rel measures
what disagreement is left, and this is the stage that removes it.  Every pixel of a frame follows its two-sided track
(models/tracks.py: `radius` Euler steps forwards, `radius` inverted steps backwards) into the neighbouring frames and reads the
depth they claim where the point lands; ONE fused launch per chunk of frames (ops.track_filter, csrc/track_filter.hip) gates the
neighbours -- inside the image, not occluded, not in gross disagreement -- and fuses the ratios D / z of the rest with the
pixel's own.  The ratio is taken along the neighbour camera's ray and applied along the frame's own: the usual approximation
for small disagreements.

Composed from Model.track the same filter would write uv, z, depth_at and inside for every row (17 B per point and row) and
keep the whole [2 radius + 1, B, 3, H, W] slab of all frames alive; here a chunk's slab is the only large buffer, whatever the
length of the video, and 13 B per pixel leave the kernel.

`filter_plan` is the host-side half (validation, which rows of every window have a frame), `filter_weights` the row weights;
`filter_depth` is what Model.filter_depth runs.  Nothing here synchronises with the device.
"""
import numpy as np
import torch

from .. import ops
from . import tracks

MAX_RADIUS = (ops.FILTER_MAX_ROWS - 1) // 2      # 16
WEIGHTS = ('gauss', 'box')


def filter_weights(radius, weights='gauss', sigma=None):
    """The fp32 row weights [2 radius + 1] of a window: 'gauss' exp(-j^2 / (2 sigma^2)) at row distance j (sigma default
    radius / 2; float64, rounded once), 'box' all ones, or a sequence of 2 radius + 1 finite values >= 0 whose middle one is
    > 0, taken as given.  ValueError otherwise."""
    n = 2 * radius + 1
    if isinstance(weights, str):
        if weights not in WEIGHTS:
            raise ValueError("filter_depth: weights must be 'gauss', 'box' or %d values, got %r" % (n, weights))
        if weights == 'box':
            return np.ones(n, dtype=np.float32)
        sigma = radius / 2.0 if sigma is None else sigma
        if isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.integer, np.floating)) or not sigma > 0 or \
                not np.isfinite(sigma):
            raise ValueError('filter_depth: sigma must be a finite number > 0, got %r' % (sigma,))
        j = np.arange(-radius, radius + 1, dtype=np.float64)
        return np.exp(-(j * j) / (2.0 * float(sigma) ** 2)).astype(np.float32)
    try:
        w = np.asarray(weights.cpu() if torch.is_tensor(weights) else weights, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("filter_depth: weights must be 'gauss', 'box' or %d values, got %r" % (n, weights))
    if w.shape != (n,) or not np.all(np.isfinite(w)) or np.any(w < 0) or not w[radius] > 0:
        raise ValueError("filter_depth: weights must be 'gauss', 'box' or %d finite values >= 0 with the middle one > 0, got %r"
                         % (n, weights))
    return w.astype(np.float32)


def filter_plan(n_frames, frames, radius, mode='mean', weights='gauss', passes=1):
    """Per frame of `frames`, how many rows of its window have a frame after it and before it -> (steps_valid,
    steps_valid_back) = (track_plan, track_plan_back) with n_steps = n_back = radius.  ValueError in their cases (an empty
    list, a frame that is no frame of the video), for a radius outside 1 .. 16, an unknown mode or weights, or passes < 1."""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= radius <= MAX_RADIUS:
        raise ValueError('filter_plan: radius must be an integer in 1 .. %d, got %r' % (MAX_RADIUS, radius))
    if mode not in ops.FILTER_MODES:
        raise ValueError('filter_plan: mode must be one of %s, got %r' % (', '.join(sorted(ops.FILTER_MODES)), mode))
    if isinstance(weights, str) and weights not in WEIGHTS:
        raise ValueError("filter_plan: weights must be 'gauss', 'box' or %d values, got %r" % (2 * radius + 1, weights))
    if isinstance(passes, bool) or not isinstance(passes, (int, np.integer)) or passes < 1:
        raise ValueError('filter_plan: passes must be an integer >= 1, got %r' % (passes,))
    try:
        return tracks.track_plan(n_frames, frames, int(radius)), tracks.track_plan_back(n_frames, frames, int(radius))
    except ValueError as e:
        raise ValueError(str(e).replace('track_plan_back:', 'filter_plan:').replace('track_plan:', 'filter_plan:')
                         .replace('n_steps', 'radius').replace('n_back', 'radius'))


def _one_pass(model, store, depth, start, valid, valid_back, radius, w, mode, tol, z_near, chunk, n_iter):
    """One filter of the frames `start` with `depth` as both the un-projected and the sampled depth -> ops.track_filter's dict
    over all of them; a chunk's slab is freed before the next one is made."""
    N, H, W, B, T1 = store.cat.n_frames, store.H, store.W, len(start), 2 * radius + 1
    dev, opt = store.device, model.opt
    out = {'depth': torch.empty(B, 1, H, W, device=dev), 'ratio': torch.empty(B, 1, H, W, device=dev),
           'count': torch.empty(B, H, W, device=dev, dtype=torch.uint8), 'spread': torch.empty(B, 1, H, W, device=dev)}
    time_step, out_scale = 1.0 / (N + 0.0), 1.0 / opt.sf_mag_div
    for b0 in range(0, B, chunk):
        b1 = min(b0 + chunk, B)
        points, ts = tracks.start_slab(model, store, depth, start[b0:b1], T1, row=radius)
        tracks.integrate(model._mlp, points[radius:], ts, valid[b0:b1], time_step, out_scale, b1 - b0)
        tracks.integrate_back(model._mlp, points[:radius + 1], ts, valid_back[b0:b1], time_step, out_scale, b1 - b0,
                              n_iter=n_iter)
        ops.track_filter(points, start[b0:b1], store.tables, depth, w, k0=-radius, mode=mode, tol=tol, z_near=z_near,
                         out={k: v[b0:b1] for k, v in out.items()})
        del points, ts
    return out


def filter_depth(model, store, frames=None, radius=4, weights='gauss', sigma=None, mode='mean', tol=0.1, z_near=1e-3,
                 depth=None, chunk=None, n_iter=4, passes=1):
    """Model.filter_depth: see there."""
    opt = model.opt
    if opt.use_cnn:
        raise NotImplementedError('Model.filter_depth integrates the scene-flow MLP kernels; the --use_cnn U-Net branch has no '
                                  'stash-free forward to chain and is not supported')
    N, H, W = store.cat.n_frames, store.H, store.W
    every = frames is None
    if every:
        frames = list(range(N))
    valid, valid_back = filter_plan(N, frames, radius, mode=mode, weights=weights, passes=passes)
    radius, passes = int(radius), int(passes)
    if passes > 1 and not every:
        raise ValueError('filter_depth: passes=%d needs every frame of the video (frames=None): a pass reads the depth the one '
                         'before it wrote' % passes)
    w = filter_weights(radius, weights, sigma)
    if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)) or n_iter < 1:
        raise ValueError('filter_depth: n_iter must be an integer >= 1, got %r' % (n_iter,))
    start = [int(s) for s in (frames.cpu().tolist() if torch.is_tensor(frames) else np.asarray(frames).reshape(-1).tolist())]
    if chunk is None:
        chunk = tracks.default_chunk(2 * radius, H, W)
    if isinstance(chunk, bool) or int(chunk) != chunk or chunk < 1:
        raise ValueError('filter_depth: chunk must be a positive number of frames, got %r' % (chunk,))
    dev = store.device
    if depth is None:
        depth = model.video_depth(store.frames(model._chunk()))
    depth = ops._dev32(depth, 'depth')
    if tuple(depth.shape) != (N, 1, H, W):
        raise ValueError('filter_depth: depth must be [%d,1,%d,%d], got %s' % (N, H, W, tuple(depth.shape)))
    model.eval()
    with torch.no_grad():
        params = model.net_sceneflow.parameter_list()
        model._mlp.pack(params[0::2], params[1::2])
        out, ratio = None, None
        for _ in range(passes):
            out = _one_pass(model, store, depth if out is None else out['depth'], start, valid, valid_back, radius, w, mode, tol,
                            z_near, int(chunk), int(n_iter))
            ratio = out['ratio'] if ratio is None else ratio * out['ratio']
        out['ratio'] = ratio
    out['steps_valid'] = torch.tensor(valid, dtype=torch.int32).to(dev, non_blocking=True)
    out['steps_valid_back'] = torch.tensor(valid_back, dtype=torch.int32).to(dev, non_blocking=True)
    return out
