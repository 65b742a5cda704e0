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


def start_slab(model, store, depth, start, T1):
    """The zeroed slab [T1,B,3,H,W] of the start frames `start` with row 0 filled -- their refined depth un-projected with
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
    ops.unproject(d0, R0, t0, K0, planar=True, out=points[0])
    return points, ts


def track(model, store, start, n_steps, depth=None, chunk=None):
    """Model.track: see there."""
    opt = model.opt
    if opt.use_cnn:
        raise NotImplementedError('Model.track integrates the scene-flow MLP kernels; the --use_cnn U-Net branch has no '
                                  'stash-free forward to chain and is not supported')
    N, H, W = store.cat.n_frames, store.H, store.W
    valid = track_plan(N, start, n_steps)
    start = [int(s) for s in (start.cpu().tolist() if torch.is_tensor(start) else np.asarray(start).reshape(-1).tolist())]
    B, T1 = len(start), int(n_steps) + 1
    if chunk is None:
        chunk = default_chunk(n_steps, H, W)
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
        points, ts = start_slab(model, store, depth, start, T1)
        params = model.net_sceneflow.parameter_list()
        model._mlp.pack(params[0::2], params[1::2])
        integrate(model._mlp, points, ts, valid, 1.0 / (N + 0.0), 1.0 / opt.sf_mag_div, int(chunk))
        out = ops.track_project(points, start, T, depth_all=depth)
    out['points'] = points
    out['steps_valid'] = torch.tensor(valid, dtype=torch.int32).to(dev, non_blocking=True)
    return out
