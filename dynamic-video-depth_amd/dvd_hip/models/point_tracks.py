"""Query-point tracks out of an optimised model, and their score against annotated trajectories.

`Model.track` follows every pixel of whole frames.  Here the queries are a list: Q chosen points (frame, x, y), at sub-pixel
positions, of any frames of the video -- annotated key points, a tracking benchmark's queries, the corners of an inserted
object.  A slab row is [3,Q]; the MLP kernels take it as one launch of Q points with a time stamp each:

  seed        ops.point_seed: the refined depth of each query's own frame at its position, un-projected with that frame's camera
  step k      one stash-free forward of the MLP kernels (p_next is the next row), t_offset = k / N
  step -j     one ops.invert_step (n_iter forwards), t_offset = -j / N
  afterwards  ONE ops.point_project launch: pixel position, depth, visibility and target frame of every row

`score_tracks` then compares the tracks with annotated ones by ONE ops.point_score launch: the TAP-Vid protocol (position
accuracy at 1, 2, 4, 8 and 16 px, occlusion accuracy and the Jaccard of the two) from exact 64-bit integer counts, pooled and
per temporal distance.  Nothing here synchronises with the device.
"""
import numpy as np
import torch

from .. import ops
from .tracks import SLAB_BYTES


def _annotations(what, gt_uv, gt_state):
    """Host annotations -> (float array [T,N,2], uint8-valued integer array [T,N])."""
    uv, st = np.asarray(gt_uv), np.asarray(gt_state)
    if uv.ndim != 3 or uv.shape[2] != 2 or st.shape != uv.shape[:2] or uv.shape[0] < 1 or uv.shape[1] < 1:
        raise ValueError('%s: gt_uv must be [T,N,2] and gt_state [T,N], got %s and %s' % (what, uv.shape, st.shape))
    return uv, st


def queries_first(gt_uv, gt_state):
    """The "query first" protocol: per track its first visible annotation.  gt_uv [T,N,2], gt_state [T,N] (0 visible) host
    arrays -> (queries float64 [Q,3] of (frame, x, y), track int64 [Q]); a track that is never visible has no query."""
    uv, st = _annotations('queries_first', gt_uv, gt_state)
    vis = st == 0
    track = np.nonzero(vis.any(1))[0]
    frame = vis[track].argmax(1)
    pos = uv[track, frame].astype(np.float64).reshape(-1, 2)
    return np.concatenate([frame[:, None].astype(np.float64), pos], 1), track.astype(np.int64)


def queries_strided(gt_uv, gt_state, stride=5):
    """The "query strided" protocol: every visible annotation on the frames 0, stride, 2 stride, ... -> (queries float64 [Q,3],
    track int64 [Q]), frame-major; gt_uv[track], gt_state[track] is the ground truth repeated per query."""
    uv, st = _annotations('queries_strided', gt_uv, gt_state)
    if isinstance(stride, bool) or int(stride) != stride or stride < 1:
        raise ValueError('queries_strided: stride must be an integer >= 1, got %r' % (stride,))
    rows = []
    for f in range(0, uv.shape[1], int(stride)):
        for k in np.nonzero(st[:, f] == 0)[0]:
            rows.append((float(f), float(uv[k, f, 0]), float(uv[k, f, 1]), int(k)))
    arr = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    return arr[:, :3].copy(), arr[:, 3].astype(np.int64)


def check_queries(what, queries, N, H, W):
    """queries: host [Q,3] of (frame, x, y) -> (frame int32 [Q], xy float32 [Q,2]).  ValueError for an empty list, a frame that
    is not integral or not a frame, a position outside [0,W-1] x [0,H-1], or a NaN."""
    if torch.is_tensor(queries):
        queries = queries.cpu().numpy()
    try:
        q = np.asarray(queries, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('%s: queries must be a host array [Q,3] of (frame, x, y)' % what)
    if q.ndim != 2 or q.shape[1] != 3:
        raise ValueError('%s: queries must be a host array [Q,3] of (frame, x, y), got shape %s' % (what, q.shape))
    if q.shape[0] < 1:
        raise ValueError('%s: no queries' % what)
    if q.shape[0] >= 1 << 30:
        raise ValueError('%s: at most 2^30 - 1 queries, got %d' % (what, q.shape[0]))
    if not np.all(np.isfinite(q)):
        raise ValueError('%s: a query holds a NaN or an Inf' % what)
    f = q[:, 0]
    if np.any(f != np.floor(f)) or f.min() < 0 or f.max() >= N:
        raise ValueError('%s: query frames must be integers in 0 .. %d, got %g .. %g' % (what, N - 1, f.min(), f.max()))
    xy = q[:, 1:].astype(np.float32)
    if xy[:, 0].min() < 0 or xy[:, 0].max() > W - 1 or xy[:, 1].min() < 0 or xy[:, 1].max() > H - 1:
        raise ValueError('%s: query positions must lie in [0, %d] x [0, %d]' % (what, W - 1, H - 1))
    return f.astype(np.int32), np.ascontiguousarray(xy)


def _count(what, name, v, lo):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
        raise ValueError('%s: %s must be an integer >= %d, got %r' % (what, name, lo, v))
    return int(v)


def default_chunk(T1, slab_bytes=SLAB_BYTES):
    """Queries per pass so that their [T1, 3, chunk] fp32 world points fit into slab_bytes."""
    return max(1, int(slab_bytes // (T1 * 12)))


def track_points(model, store, queries, n_steps=None, n_back=None, depth=None, z_tol=0.05, n_iter=4, chunk=None):
    """Model.track_points: see there.  All queries take all n_steps forward and n_back backward steps, whatever their frame;
    the rows that fall off the video are masked by the projection (zeros, target -1) -- at most 2 x wasted MLP work on a
    workload that is tiny beside a dense track."""
    what = 'track_points'
    opt = model.opt
    if opt.use_cnn:
        raise NotImplementedError('Model.track_points integrates the scene-flow MLP kernels; the --use_cnn U-Net branch has no '
                                  'stash-free forward to chain and is not supported')
    N, H, W = store.cat.n_frames, store.H, store.W
    frame, xy = check_queries(what, queries, N, H, W)
    Q = len(frame)
    n_steps = N - 1 - int(frame.min()) if n_steps is None else _count(what, 'n_steps', n_steps, 0)
    n_back = int(frame.max()) if n_back is None else _count(what, 'n_back', n_back, 0)
    if n_back:
        _count(what, 'n_iter', n_iter, 1)
    T1 = n_back + n_steps + 1
    if T1 > 65535:
        raise ValueError('%s: at most 65535 rows, got n_back + n_steps + 1 = %d' % (what, T1))
    if chunk is None:
        chunk = default_chunk(T1)
    if isinstance(chunk, bool) or int(chunk) != chunk or chunk < 1:
        raise ValueError('%s: chunk must be a positive number of queries, got %r' % (what, chunk))
    chunk = min(int(chunk), Q)
    if isinstance(z_tol, bool) or not isinstance(z_tol, (int, float, np.integer, np.floating)) or not 0 <= z_tol < float('inf'):
        raise ValueError('%s: z_tol must be a finite number >= 0, got %r' % (what, z_tol))
    dev, T = store.device, store.tables
    if depth is None:
        depth = model.video_depth(store.frames(model._chunk()))
    depth = ops._dev32(depth, 'depth')
    if tuple(depth.shape) != (N, 1, H, W):
        raise ValueError('%s: depth must be [%d,1,%d,%d], got %s' % (what, N, H, W, tuple(depth.shape)))
    time_step, out_scale = 1.0 / (N + 0.0), 1.0 / opt.sf_mag_div
    model.eval()
    with torch.no_grad():
        frame_d = torch.from_numpy(frame).to(dev)
        xy_d = torch.from_numpy(xy).to(dev)
        points = torch.zeros(T1, 3, Q, device=dev)
        ok = torch.empty(Q, device=dev, dtype=torch.uint8)
        resid = torch.zeros(n_back, device=dev)
        params = model.net_sceneflow.parameter_list()
        model._mlp.pack(params[0::2], params[1::2])
        for q0 in range(0, Q, chunk):
            q1 = min(q0 + chunk, Q)
            n = q1 - q0
            whole = n == Q
            slab = points if whole else torch.zeros(T1, 3, n, device=dev)
            seed = ops.point_seed(frame_d[q0:q1], xy_d[q0:q1], depth, T, time_stamps=bool(opt.time_dependent),
                                  out={'points': slab[n_back], 'ok': ok[q0:q1]}, host_frame=frame[q0:q1])
            ts = seed['t'].view(1, 1, 1, n) if opt.time_dependent else None
            rows = slab.view(T1, 1, 3, 1, n)
            for k in range(n_steps):
                model._mlp.forward(rows[n_back + k], ts, t_offset=k * time_step, out_scale=out_scale, p_next=rows[n_back + k + 1])
            if n_back:
                scratch = torch.empty(1, 3, 1, n, device=dev)
                r = torch.zeros(n_back, 1, device=dev)
                for j in range(1, n_back + 1):
                    ops.invert_step(model._mlp, rows[n_back - j + 1], ts, -j * time_step, out_scale, n_iter=int(n_iter),
                                    out=rows[n_back - j], resid=r[j - 1], scratch=scratch)
                torch.maximum(resid, r[:, 0], out=resid)
            if not whole:
                points[:, :, q0:q1].copy_(slab)
        out = ops.point_project(points, frame_d, xy_d, T, depth, k0=-n_back, z_tol=float(z_tol), ok=ok, host_frame=frame)
    out.update(points=points, ok=ok, origin=n_back, resid=resid)
    return out


def _ratio(num, den):
    nan = torch.full((), float('nan'), dtype=torch.float64, device=num.device)
    return torch.where(den > 0, num.double() / den.double(), nan)


def derive(sums, shift):
    """The reported quantities from sums [...,19] (ops.POINT_SUMS): float64 tensors, NaN where a denominator is 0."""
    n_eval, n_vis = sums[..., 0], sums[..., 1]
    within = _ratio(sums[..., 3:8], n_vis[..., None])
    jac = _ratio(sums[..., 8:13], n_vis[..., None] + sums[..., 13:18])
    return {'n_eval': n_eval, 'n_gt_visible': n_vis, 'occlusion_accuracy': _ratio(sums[..., 2], n_eval), 'pts_within': within,
            'jaccard': jac, 'average_pts_within': within.mean(-1), 'average_jaccard': jac.mean(-1),
            'mean_err': _ratio(sums[..., 18], n_vis) * (2.0 ** -shift)}


def score_tracks(model, store, queries, gt_uv, gt_state, thresholds=ops.POINT_THRESHOLDS, px_scale=(1.0, 1.0), **track_args):
    """Model.score_tracks: see there."""
    what = 'score_tracks'
    N = store.cat.n_frames
    q = np.asarray(queries.cpu() if torch.is_tensor(queries) else queries)
    Q = int(q.shape[0]) if q.ndim == 2 else -1

    def host(v):
        return np.asarray(v.cpu() if torch.is_tensor(v) else v)

    if not (torch.is_tensor(gt_uv) and gt_uv.is_cuda):
        gt_uv = host(gt_uv)
    if not (torch.is_tensor(gt_state) and gt_state.is_cuda):
        gt_state = host(gt_state)
    if tuple(gt_uv.shape) != (Q, N, 2) or tuple(gt_state.shape) != (Q, N):
        raise ValueError('%s: gt_uv must be [%d,%d,2] and gt_state [%d,%d] (one trajectory per query, frame-major), got %s and %s' % (
            what, Q, N, Q, N, tuple(gt_uv.shape), tuple(gt_state.shape)))
    ops.point_thr2(thresholds)          # (refused before the tracks are integrated)
    tr = track_points(model, store, queries, **track_args)
    dev = store.device
    if not torch.is_tensor(gt_uv):
        gt_uv = torch.from_numpy(np.ascontiguousarray(gt_uv, dtype=np.float32)).to(dev)
    if not torch.is_tensor(gt_state):
        if gt_state.dtype.kind not in 'iub' or (gt_state.size and (gt_state.min() < 0 or gt_state.max() > 255)):
            raise ValueError('%s: gt_state must hold integers in 0 .. 255' % what)
        gt_state = torch.from_numpy(np.ascontiguousarray(gt_state.astype(np.uint8))).to(dev)
    with torch.no_grad():
        res = ops.point_score(tr['uv'], tr['visible'], tr['target'], gt_uv, gt_state, origin=tr['origin'], thresholds=thresholds,
                              px_scale=tuple(px_scale) if isinstance(px_scale, (tuple, list)) else px_scale)
        sums, shift = res['sums'], res['shift']
        out = derive(sums.sum(0), shift)
        out['by_offset'] = derive(sums, shift)
    out.update(sums=sums, shift=shift, tracks=tr)
    return out
