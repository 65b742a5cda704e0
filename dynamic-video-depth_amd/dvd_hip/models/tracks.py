"""Long-range 3D tracks out of an optimised model: where is a pixel of frame f in frame f + k?

The scene-flow MLP is a velocity field; the reference integrates it over any number of frames
(Model.forward_sf_net_multi_step, models/scene_flow_motion_field.py:360-367), projects world points into a camera
(losses.scene_flow_projection.project_ptcld, :21-44) and samples a map at the projected position (BackwardWarp, :281-307).
Here the three are chained on the device for every start frame of a video at once:

  step 0        ops.unproject of the start frame's refined depth with its own camera
  step k -> k+1 one stash-free forward of the MLP kernels, whose p_next output IS row k + 1 of the result
  afterwards    ONE dvd_track_project launch over all rows: pixel position, depth and visibility in frame f + k

`track_plan` is the host-side half (validation, how many steps of every start frame have a target frame); `video_depth` and
`track` are what `Model.video_depth` / `Model.track` run.  Nothing here synchronises with the device.

Two-sided tracks (n_back >= 1): the field also runs backwards.  One Euler step x -> x + s f(x, t) is a near-identity map, and
the point it carries to p is the fixed point of y <- p - s f(y, t): ops.invert_step, n_iter stash-free forwards each followed
by one dvd_track_invert_update (csrc/invert.hip).  The slab then holds n_back rows before the start frame -- row n_back is the
start frame, row j is frame start + j - n_back -- and ONE dvd_track_project_from launch (k0 = -n_back) projects all of them.
"""
import numpy as np
import torch

from .. import ops

SLAB_BYTES = 8 << 30        # default bound on the world points one pass integrates (chunk start frames x all steps)


def track_plan(n_frames, start, n_steps):
    """Per start frame, how many of the steps 1 .. n_steps have a target frame: min(n_steps, n_frames - 1 - start).
    ValueError for an empty start list, a start that is negative, not integral or not a frame, or n_steps < 1."""
    if isinstance(n_frames, bool) or int(n_frames) != n_frames or n_frames < 1:
        raise ValueError('track_plan: n_frames must be a positive integer, got %r' % (n_frames,))
    if isinstance(n_steps, bool) or not isinstance(n_steps, (int, np.integer)) or n_steps < 1:
        raise ValueError('track_plan: n_steps must be an integer >= 1, got %r' % (n_steps,))
    if torch.is_tensor(start):
        start = start.cpu().tolist()
    start = list(np.asarray(start).reshape(-1).tolist()) if isinstance(start, np.ndarray) else list(start)
    if not start:
        raise ValueError('track_plan: no start frames')
    out = []
    for s in start:
        if isinstance(s, bool) or not isinstance(s, (int, float, np.integer, np.floating)) or s != s or int(s) != s:
            raise ValueError('track_plan: start frame %r is not an integer' % (s,))
        s = int(s)
        if s < 0 or s >= n_frames:
            raise ValueError('track_plan: start frame %d is outside the %d frames of the video' % (s, n_frames))
        out.append(min(int(n_steps), int(n_frames) - 1 - s))
    return out


def track_plan_back(n_frames, start, n_back):
    """Per start frame, how many of the backward steps 1 .. n_back have a target frame: min(n_back, start).  ValueError in
    track_plan's cases (an empty start list, a start that is no frame of the video, n_back < 1)."""
    try:
        track_plan(n_frames, start, n_back)
    except ValueError as e:
        raise ValueError(str(e).replace('track_plan:', 'track_plan_back:').replace('n_steps', 'n_back'))
    if torch.is_tensor(start):
        start = start.cpu().tolist()
    return [min(int(n_back), int(s)) for s in np.asarray(start).reshape(-1).tolist()]


def default_chunk(n_steps, H, W, slab_bytes=SLAB_BYTES):
    """Start frames per pass so that their [n_steps + 1, chunk, 3, H, W] fp32 world points fit into slab_bytes."""
    return max(1, int(slab_bytes // ((n_steps + 1) * 3 * H * W * 4)))


def _runs(valid, b0, b1, k):
    """Maximal runs [r0, r1) of the rows b0 .. b1 that still have a target frame after step k."""
    out, r0 = [], None
    for b in range(b0, b1):
        if valid[b] > k:
            r0 = b if r0 is None else r0
        elif r0 is not None:
            out.append((r0, b))
            r0 = None
    if r0 is not None:
        out.append((r0, b1))
    return out


def video_depth(model, frames):
    """Refined depth of every frame of the validation view `frames` -> [N,1,H,W] on the device: the depth net exactly as
    Model._predict_on_batch(is_train=False) runs it, batch by batch."""
    model.eval()
    out = []
    with torch.no_grad():
        for batch in frames:
            model.load_batch(batch)
            inp = model._input
            fid = inp.frame_id_1 if not model.opt.midas else None
            out.append(model._depth.forward(inp.img, fid))
    if not out:
        raise ValueError('video_depth: no frames')
    return torch.cat(out, 0).contiguous()


def integrate(mlp, points, ts, valid, time_step, out_scale, chunk):
    """The Euler chain on the slab: points [T1,B,3,H,W] with row 0 filled; row k + 1 of image b is written by the MLP
    forward of row k while image b has a target frame (valid[b] > k) and is left as it is otherwise.  ts: [B,1,H,W] or None."""
    T1, B = points.shape[:2]
    for b0 in range(0, B, chunk):
        b1 = min(b0 + chunk, B)
        for k in range(T1 - 1):
            for r0, r1 in _runs(valid, b0, b1, k):
                mlp.forward(points[k, r0:r1], None if ts is None else ts[r0:r1], t_offset=k * time_step, out_scale=out_scale,
                            p_next=points[k + 1, r0:r1])


def integrate_back(mlp, points, ts, valid_back, time_step, out_scale, chunk, n_iter=4, resid=None):
    """The chain run backwards on the slab: points [n_back + 1,B,3,H,W] with its LAST row (the start frames) filled; row
    n_back - j of image b is the inverse Euler step (ops.invert_step, t_offset = -j * time_step) of row n_back - j + 1 while
    image b has a frame there (valid_back[b] >= j) and is left as it is otherwise.  resid: fp32 [n_back,B] or None; row j - 1
    receives the last iteration's residual of step j (rows without a frame are not written).  ts as in `integrate`."""
    n_back, B = points.shape[0] - 1, points.shape[1]
    scratch = torch.empty((min(chunk, B),) + tuple(points.shape[2:]), device=points.device)
    for b0 in range(0, B, chunk):
        b1 = min(b0 + chunk, B)
        for j in range(1, n_back + 1):
            for r0, r1 in _runs(valid_back, b0, b1, j - 1):
                ops.invert_step(mlp, points[n_back - j + 1, r0:r1], None if ts is None else ts[r0:r1], -j * time_step, out_scale,
                                n_iter=n_iter, out=points[n_back - j, r0:r1], resid=None if resid is None else resid[j - 1, r0:r1],
                                scratch=scratch[:r1 - r0])


def start_slab(model, store, depth, start, T1, row=0):
    """The zeroed slab [T1,B,3,H,W] of the start frames `start` with row `row` filled -- their refined depth un-projected with
    their own cameras -- and their time stamps [B,1,H,W] (None for a time-independent field)."""
    dev, T, H, W = store.device, store.tables, store.H, store.W
    B = len(start)
    # the start frames' rows of the store, by the store's own gather (one launch): depth, camera, time stamp
    d0 = torch.empty(B, 1, H, W, device=dev)
    R0, K0, t0 = torch.empty(B, 3, 3, device=dev), torch.empty(B, 3, 3, device=dev), torch.empty(B, 3, device=dev)
    entries = [(depth, d0, 'copy', 0), (T['R_T'], R0, 'copy', 0), (T['K_inv_T'], K0, 'copy', 0), (T['t'], t0, 'copy', 0)]
    ts = None
    if model.opt.time_dependent:
        ts = torch.empty(B, 1, H, W, device=dev)
        entries.append((T['ts_vali'], ts, 'fill', 0))
    ops.store_gather(entries, np.array([start, start, start], dtype=np.int32))
    points = torch.zeros(T1, B, 3, H, W, device=dev)
    ops.unproject(d0, R0, t0, K0, planar=True, out=points[row])
    return points, ts


def track(model, store, start, n_steps, depth=None, chunk=None, n_back=0, n_iter=4):
    """Model.track: see there."""
    opt = model.opt
    if opt.use_cnn:
        raise NotImplementedError('Model.track integrates the scene-flow MLP kernels; the --use_cnn U-Net branch has no '
                                  'stash-free forward to chain and is not supported')
    N, H, W = store.cat.n_frames, store.H, store.W
    if isinstance(n_back, bool) or not isinstance(n_back, (int, np.integer)) or n_back < 0:
        raise ValueError('track: n_back must be an integer >= 0, got %r' % (n_back,))
    n_back = int(n_back)
    if n_back and (isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)) or n_iter < 1):
        raise ValueError('track: n_iter must be an integer >= 1, got %r' % (n_iter,))
    valid_back = track_plan_back(N, start, n_back) if n_back else None
    # (a two-sided track may have no forward rows at all; a one-sided one keeps track_plan's n_steps >= 1)
    if n_back and not isinstance(n_steps, bool) and isinstance(n_steps, (int, np.integer)) and n_steps == 0:
        valid = [0] * len(valid_back)
    else:
        valid = track_plan(N, start, n_steps)
    start = [int(s) for s in (start.cpu().tolist() if torch.is_tensor(start) else np.asarray(start).reshape(-1).tolist())]
    B, T1 = len(start), n_back + int(n_steps) + 1
    if chunk is None:
        chunk = default_chunk(n_back + n_steps, H, W)
    if isinstance(chunk, bool) or int(chunk) != chunk or chunk < 1:
        raise ValueError('track: chunk must be a positive number of start frames, got %r' % (chunk,))
    dev, T = store.device, store.tables
    if depth is None:
        depth = model.video_depth(store.frames(model._chunk()))
    depth = ops._dev32(depth, 'depth')
    if tuple(depth.shape) != (N, 1, H, W):
        raise ValueError('track: depth must be [%d,1,%d,%d], got %s' % (N, H, W, tuple(depth.shape)))
    model.eval()
    with torch.no_grad():
        points, ts = start_slab(model, store, depth, start, T1, row=n_back)
        params = model.net_sceneflow.parameter_list()
        model._mlp.pack(params[0::2], params[1::2])
        integrate(model._mlp, points[n_back:], ts, valid, 1.0 / (N + 0.0), 1.0 / opt.sf_mag_div, int(chunk))
        if n_back:
            resid = torch.zeros(n_back, B, device=dev)
            integrate_back(model._mlp, points[:n_back + 1], ts, valid_back, 1.0 / (N + 0.0), 1.0 / opt.sf_mag_div, int(chunk),
                           n_iter=int(n_iter), resid=resid)
        out = ops.track_project(points, start, T, depth_all=depth, k0=-n_back)
    out['points'] = points
    out['steps_valid'] = torch.tensor(valid, dtype=torch.int32).to(dev, non_blocking=True)
    if n_back:
        out['origin'] = n_back
        out['steps_valid_back'] = torch.tensor(valid_back, dtype=torch.int32).to(dev, non_blocking=True)
        out['resid'] = resid
    return out
