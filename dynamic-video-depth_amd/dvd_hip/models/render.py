"""The video re-rendered from its own geometry and motion: frames splatted along their tracks into any camera.

A source frame f is un-projected with its refined depth and its own camera, pushed along the scene-flow field to the time of a
target frame g by g - f Euler steps of the MLP (the chain of models/tracks.py; Model.forward_sf_net_multi_step,
models/scene_flow_motion_field.py:360-367), and drawn -- colours, depth, coverage -- in the camera of g or in a camera that
never existed, by the forward splat of csrc/splat.hip.  Several sources of one view share its z-buffer, so frames fill one
another's holes and the nearest surface wins.

  per chunk of source images   ops.store_gather (depth, camera, time stamp) -> ops.unproject -> the Euler chain on two
                               ping-pong buffers; the last row of every source lands in one [S,3,H,W] tensor
  afterwards                   ONE ops.splat over all sources of all views: two clears and three launches

With backward=True a source may also be LATER than its target: it is carried back by f - g inverse Euler steps
(ops.invert_step, the backward half of models/tracks.py) on the same ping-pong buffers plus one that holds the field's output,
so a view is filled from both sides and the disocclusions only later frames see stop being holes.

`render_plan` is the host-side half (validation, the flat list of sources and their step counts); `render` is what
`Model.render` runs.  Nothing here synchronises with the device.
"""
import numpy as np
import torch

from .. import ops
from ..datasets import frame_store
from . import tracks


def _frame(what, f, n_frames):
    if isinstance(f, bool) or not isinstance(f, (int, float, np.integer, np.floating)) or f != f or int(f) != f:
        raise ValueError('render_plan: %s %r is not an integer' % (what, f))
    f = int(f)
    if f < 0 or f >= n_frames:
        raise ValueError('render_plan: %s %d is outside the %d frames of the video' % (what, f, n_frames))
    return f


def _as_list(x):
    if torch.is_tensor(x):
        return x.cpu().tolist()
    if isinstance(x, np.ndarray):
        return x.tolist()
    return list(x)


def render_plan(n_frames, target, sources, advect=True, backward=False):
    """The flat source list of a render: (source frames, their view index, their Euler step counts), each of length S.
    target: V frame indices; sources: V lists of frame indices, sources[v] drawn into view v.  ValueError for an empty list, a
    frame that is not an integer or not in the video, a length mismatch and, with advect, a source later than its target (the
    field integrates forwards only) unless backward, which makes the step counts signed: g - f < 0 for a source that is
    carried back in time.  Without advect every step count is 0 and any frames go together."""
    if isinstance(n_frames, bool) or int(n_frames) != n_frames or n_frames < 1:
        raise ValueError('render_plan: n_frames must be a positive integer, got %r' % (n_frames,))
    n_frames = int(n_frames)
    target = _as_list(target)
    if np.ndim(target) != 1:
        raise ValueError('render_plan: target must be a flat list of frame indices')
    sources = _as_list(sources)
    if not target:
        raise ValueError('render_plan: no target views')
    if len(sources) != len(target):
        raise ValueError('render_plan: %d source lists for %d target views' % (len(sources), len(target)))
    frames, view, steps = [], [], []
    for v, (g, src) in enumerate(zip(target, sources)):
        g = _frame('target frame', g, n_frames)
        if isinstance(src, (str, bytes)) or not hasattr(src, '__iter__'):
            raise ValueError('render_plan: the sources of view %d must be a list of frame indices, got %r' % (v, src))
        src = _as_list(src)
        if not src:
            raise ValueError('render_plan: view %d has no source frames' % v)
        for f in src:
            f = _frame('source frame', f, n_frames)
            if advect and f > g and not backward:
                raise ValueError('render_plan: source frame %d is later than its target frame %d; the scene-flow field '
                                 'integrates forwards only (advect=False renders held time)' % (f, g))
            frames.append(f)
            view.append(v)
            steps.append(g - f if advect else 0)
    return frames, view, steps


def view_tables(store, target, cam_c2w=None, K=None):
    """The camera table rows of the V views on the host -> {'R', 't', 'K_T'}: rows `target` of the store's tables, or, for
    novel cameras, rows filled by the store's own _set_camera_row from cam_c2w [V,4,4] (camera-to-world poses) and / or K
    [V,3,3] (intrinsics); whichever is None comes from the target frames."""
    V, host = len(target), store.host_tables
    if cam_c2w is None and K is None:
        idx = torch.tensor(target, dtype=torch.long)
        return {k: host[k][idx].contiguous() for k in ops.TRACK_TABLES}

    def arr(x, shape, name):
        x = np.asarray(x.detach().cpu() if torch.is_tensor(x) else x)
        if x.shape != shape or x.dtype.kind != 'f':
            raise ValueError('render: %s must be a float array %s, got %s %s' % (name, shape, x.dtype, x.shape))
        return x

    poses = arr(cam_c2w, (V, 4, 4), 'cam_c2w') if cam_c2w is not None else host['cam_c2w'][target].numpy()
    # (without K the target frame's own intrinsics, in the precision the tables keep them)
    Ks = arr(K, (V, 3, 3), 'K') if K is not None else host['K_T'][target].transpose(1, 2).contiguous().numpy()
    tab = frame_store._new_tables(V)
    for v in range(V):
        frame_store._set_camera_row(tab, v, poses[v], Ks[v])
    return {k: tab[k] for k in ops.TRACK_TABLES}


def _segments(flags, b0, b1):
    """Maximal runs [r0, r1, flag) of the rows b0 .. b1 over which `flags` is constant."""
    out, r0 = [], b0
    for b in range(b0 + 1, b1 + 1):
        if b == b1 or flags[b] != flags[r0]:
            out.append((r0, b, flags[r0]))
            r0 = b
    return out


def advect_points(model, store, depth, frames, steps, chunk, n_iter=4):
    """World points of the source frames at their targets' times -> [S,3,H,W]: un-projected refined depth, then steps[s]
    stash-free Euler steps of the MLP, or -steps[s] inverse steps (ops.invert_step with n_iter iterations) where steps[s] < 0.
    A chunk of source images goes through the chain at once on two ping-pong buffers (and one for the field's output where a
    source goes back); the step that finishes a source writes straight into its row of the result."""
    opt, dev, T = model.opt, store.device, store.tables
    N, H, W = store.cat.n_frames, store.H, store.W
    S = len(frames)
    out = torch.empty(S, 3, H, W, device=dev)
    any_steps = any(steps)
    if any_steps:
        params = model.net_sceneflow.parameter_list()
        model._mlp.pack(params[0::2], params[1::2])
        ping = [torch.empty(min(chunk, S), 3, H, W, device=dev) for _ in range(2)]
        sf = torch.empty(min(chunk, S), 3, H, W, device=dev) if min(steps) < 0 else None
    time_step, out_scale = 1.0 / (N + 0.0), 1.0 / opt.sf_mag_div
    for c0 in range(0, S, chunk):
        c1 = min(c0 + chunk, S)
        B, fr, st = c1 - c0, frames[c0:c1], steps[c0:c1]
        # the sources' rows of the store, by the store's own gather (one launch): depth, camera, time stamp
        d0 = torch.empty(B, 1, H, W, device=dev)
        R0, K0, t0 = torch.empty(B, 3, 3, device=dev), torch.empty(B, 3, 3, device=dev), torch.empty(B, 3, device=dev)
        entries = [(depth, d0, 'copy', 0), (T['R_T'], R0, 'copy', 0), (T['K_inv_T'], K0, 'copy', 0), (T['t'], t0, 'copy', 0)]
        ts = None
        if any(st) and opt.time_dependent:
            ts = torch.empty(B, 1, H, W, device=dev)
            entries.append((T['ts_vali'], ts, 'fill', 0))
        ops.store_gather(entries, np.array([fr, fr, fr], dtype=np.int32))
        # step 0: a source that is not advected is finished by its un-projection
        for r0, r1, moving in _segments([s != 0 for s in st], 0, B):
            dst = ping[0][r0:r1] if moving else out[c0 + r0:c0 + r1]
            ops.unproject(d0[r0:r1], R0[r0:r1], t0[r0:r1], K0[r0:r1], planar=True, out=dst)
        for k in range(max(max(st), 0)):
            src, nxt = ping[k % 2], ping[(k + 1) % 2]
            for r0, r1 in tracks._runs(st, 0, B, k):                      # the rows that still have step k to do ...
                for q0, q1, last in _segments([s == k + 1 for s in st], r0, r1):      # ... and whether it is their last
                    model._mlp.forward(src[q0:q1], None if ts is None else ts[q0:q1], t_offset=k * time_step,
                                       out_scale=out_scale, p_next=out[c0 + q0:c0 + q1] if last else nxt[q0:q1])
        back = [max(-s, 0) for s in st]
        for j in range(1, max(back) + 1):                                 # inverse step j: from frame f - j + 1 to f - j
            src, nxt = ping[(j - 1) % 2], ping[j % 2]
            for r0, r1 in tracks._runs(back, 0, B, j - 1):
                for q0, q1, last in _segments([s == j for s in back], r0, r1):
                    ops.invert_step(model._mlp, src[q0:q1], None if ts is None else ts[q0:q1], -j * time_step, out_scale,
                                    n_iter=n_iter, out=out[c0 + q0:c0 + q1] if last else nxt[q0:q1], scratch=sf[q0:q1])
    return out


def render(model, store, target, sources, cam_c2w=None, K=None, depth=None, advect=True, chunk=None, valid=None,
           backward=False, n_iter=4, inpaint=False, bg_power=2, **splat_params):
    """Model.render: see there."""
    opt = model.opt
    if not isinstance(inpaint, (bool, np.bool_)):
        raise ValueError('render: inpaint must be True or False, got %r' % (inpaint,))
    if isinstance(bg_power, (bool, np.bool_)) or not isinstance(bg_power, (int, np.integer)) or not 0 <= bg_power <= 4:
        raise ValueError('render: bg_power must be an integer in 0 .. 4, got %r' % (bg_power,))
    if advect and opt.use_cnn:
        raise NotImplementedError('Model.render integrates the scene-flow MLP kernels; the --use_cnn U-Net branch has no '
                                  'stash-free forward to chain and is not supported (advect=False renders held time)')
    unknown = set(splat_params) - set(ops.SPLAT_DEFAULTS)
    if unknown:
        raise TypeError('render: unknown splat parameters %s (known: %s)' % (sorted(unknown), ', '.join(sorted(ops.SPLAT_DEFAULTS))))
    splat_params.setdefault('value_bound', 1.0)
    N, H, W = store.cat.n_frames, store.H, store.W
    frames, view, steps = render_plan(N, target, sources, advect, backward=bool(backward))
    if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)) or n_iter < 1:
        raise ValueError('render: n_iter must be an integer >= 1, got %r' % (n_iter,))
    target = [int(g) for g in _as_list(target)]
    V = len(target)
    if chunk is None:
        chunk = tracks.default_chunk(1, H, W)
    if isinstance(chunk, bool) or int(chunk) != chunk or chunk < 1:
        raise ValueError('render: chunk must be a positive number of source images, got %r' % (chunk,))
    dev = store.device
    tabs = {k: v.to(dev, non_blocking=True) for k, v in view_tables(store, target, cam_c2w, K).items()}
    if depth is None:
        depth = model.video_depth(store.frames(model._chunk()))
    depth = ops._dev32(depth, 'depth')
    if tuple(depth.shape) != (N, 1, H, W):
        raise ValueError('render: depth must be [%d,1,%d,%d], got %s' % (N, H, W, tuple(depth.shape)))
    if valid is not None and not (torch.is_tensor(valid) and valid.is_cuda and valid.dtype == torch.uint8 and
                                  tuple(valid.shape) == (N, H, W)):
        raise ValueError('render: valid must be a GPU uint8 tensor [%d,%d,%d]' % (N, H, W))
    model.eval()
    with torch.no_grad():
        points = advect_points(model, store, depth, frames, steps, int(chunk), n_iter=int(n_iter))
        # the sources' colours and masks, in the order of the points (one more launch of the store's gather)
        S = len(frames)
        colours = torch.empty(S, 3, H, W, device=dev)
        entries = [(store.img, colours, 'copy', 0)]
        mask = None
        if valid is not None:
            mask = torch.empty(S, H, W, device=dev, dtype=torch.uint8)
            entries.append((valid.contiguous(), mask, 'copy', 0))
        ops.store_gather(entries, np.array([frames, frames, frames], dtype=np.int32))
        res = ops.splat(points, colours, view, tabs, V, valid=mask, planar=True, **splat_params)
        if inpaint:
            inpaint_views(res, int(bg_power), splat_params.get('fill', ops.SPLAT_DEFAULTS['fill']))
        return res


def inpaint_views(res, bg_power, fill):
    """Fill the holes of a splat's result in place (ops.fill_holes, three launches): image and depth jointly as 4 channels,
    known = hit, a hit pixel weighted by depth^bg_power.  image and depth are replaced by the completed ones -- their hit pixels
    keep their bits --, 'level' is added, hit and weight stay.  A view that nothing hit is `fill` in all four channels."""
    joint = torch.cat((res['image'], res['depth']), dim=1)
    filled = ops.fill_holes(joint, res['hit'], bias=res['depth'], power=bg_power, fill=fill, out={'values': joint})
    C = res['image'].shape[1]
    res['image'], res['depth'], res['level'] = joint[:, :C], joint[:, C:], filled['level']
    return res
