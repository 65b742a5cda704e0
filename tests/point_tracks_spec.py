"""Query-point tracks restated for the tests (test infrastructure; numpy and plain torch on the CPU).

What dvd_point_seed, dvd_point_project and dvd_point_score compute (csrc/point_track.hip), from the formulas and nothing of the
product:
  seed, project   float64: tracks_spec.sample_border and tracks_spec.project's formula, per point with its own frame
  *_fp32          the same formulas as the fp32 torch expressions the reference would evaluate (F.grid_sample bilinear / border /
                  align_corners=True plus the matmuls): their distance from float64 is what fp32 can do on the given inputs
  score_mirror    the float32 operations of the kernel in the kernel's order, counts and llrint in integers: equal bit for bit
  score_loop      an independent, slow per-point loop of the metric definitions, to check the mirror
and the generators of the cases the GPU tests run, so that the CPU tests can check what they promise.
"""
import numpy as np
import torch

import tracks_spec as S

CAP = 1024.0
N_SUMS = 19


def eval_shift(n):
    return min(32, 62 - 10 - (int(n) - 1).bit_length())


# -- seed and project ----------------------------------------------------------------------------------------------------------
def _sample(img, u, v, dtype):
    """One frame's map [H,W] at the positions (u, v): tracks_spec.sample_border in float64; in fp32 the torch call the reference
    makes, F.grid_sample(bilinear, border, align_corners=True) of the normalised positions."""
    if dtype == torch.float64:
        return S.sample_border(img, u, v)
    import torch.nn.functional as F
    H, W = img.shape
    grid = torch.stack([u / ((W - 1) / 2.0) - 1, v / ((H - 1) / 2.0) - 1], -1).view(1, 1, -1, 2)
    return F.grid_sample(img.view(1, 1, H, W), grid, mode='bilinear', padding_mode='border', align_corners=True).view(-1)


def _seed(frame, xy, depth_all, R_T, t, K_inv_T, dtype):
    frame = torch.as_tensor(np.asarray(frame).astype(np.int64))
    xy = torch.as_tensor(np.asarray(xy)).to(dtype)
    depth_all, R_T, t, K_inv_T = (torch.as_tensor(np.asarray(v)).to(dtype) for v in (depth_all, R_T, t, K_inv_T))
    N, _, H, W = depth_all.shape
    Q = len(frame)
    P = torch.zeros(3, Q, dtype=dtype)
    ok = torch.zeros(Q, dtype=torch.bool)
    x, y = xy[:, 0], xy[:, 1]
    in_img = (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
    for f in range(N):                                  # the queries of one frame at a time
        rows = torch.nonzero((frame == f) & in_img)[:, 0]
        if not len(rows):
            continue
        d = _sample(depth_all[f, 0], x[rows], y[rows], dtype)
        good = torch.isfinite(d) & (d > 0)
        ray = torch.stack([x[rows], y[rows], torch.ones_like(d)], -1) @ K_inv_T[f]
        pts = (d[:, None] * ray) @ R_T[f] + t[f]
        P[:, rows[good]] = pts[good].T
        ok[rows[good]] = True
    return P, ok


def seed(frame, xy, depth_all, R_T, t, K_inv_T):
    """-> (points float64 [3,Q], ok bool [Q]): depth_all[frame] at xy (bilinear, border), un-projected with the frame's camera;
    a query whose frame is no frame, whose position is outside the image or whose depth is not finite and > 0 is not ok: 0."""
    return _seed(frame, xy, depth_all, R_T, t, K_inv_T, torch.float64)


def seed_fp32(frame, xy, depth_all, R_T, t, K_inv_T):
    """`seed` as the fp32 torch expressions of the reference: grid_sample plus the matmuls."""
    return _seed(frame, xy, depth_all, R_T, t, K_inv_T, torch.float32)[0]


def _project(points, frame, xy, k0, R, t, K_T, depth_all, z_tol, ok, dtype):
    points = torch.as_tensor(np.asarray(points)).to(dtype)
    R, t, K_T, depth_all = (torch.as_tensor(np.asarray(v)).to(dtype) for v in (R, t, K_T, depth_all))
    frame = torch.as_tensor(np.asarray(frame).astype(np.int64))
    T1, _, Q = points.shape
    N, _, H, W = depth_all.shape
    ok = torch.ones(Q, dtype=torch.bool) if ok is None else torch.as_tensor(np.asarray(ok)).bool()
    uv = torch.zeros(T1, Q, 2, dtype=dtype)
    z, depth_at = torch.zeros(T1, Q, dtype=dtype), torch.zeros(T1, Q, dtype=dtype)
    inside = torch.zeros(T1, Q, dtype=torch.bool)
    g_all = frame[None, :] + torch.arange(T1)[:, None] + k0
    live = ok[None, :] & (frame >= 0)[None, :] & (frame < N)[None, :] & (g_all >= 0) & (g_all < N)
    target = torch.where(live, g_all, torch.full_like(g_all, -1))
    for g in range(N):                                  # the rows that look into one frame at a time
        jj, qq = torch.nonzero(target == g, as_tuple=True)
        if not len(jj):
            continue
        I = ((points[jj, :, qq] - t[g]) @ R[g]) @ K_T[g]
        c = I[:, :2] / (I[:, 2:] + 1e-8)
        front = I[:, 2] > 0
        d = _sample(depth_all[g, 0], c[:, 0], c[:, 1], dtype)
        uv[jj, qq], z[jj, qq] = c, I[:, 2]
        depth_at[jj, qq] = torch.where(front, d, torch.zeros_like(d))
        inside[jj, qq] = front & (c[:, 0] >= 0) & (c[:, 0] <= W - 1) & (c[:, 1] >= 0) & (c[:, 1] <= H - 1)
    visible = inside & ~(z > depth_at * (1.0 + z_tol))
    return {'uv': uv, 'z': z, 'depth_at': depth_at, 'inside': inside, 'visible': visible, 'target': target}


def project(points, frame, xy, k0, R, t, K_T, depth_all, z_tol=0.05, ok=None):
    """Row j of query q into frame frame[q] + j + k0, float64 -> uv [T1,Q,2], z, depth_at [T1,Q], inside, visible (bool),
    target (int64, -1 where the row has no frame or the query is not ok; such a row is zeros)."""
    return _project(points, frame, xy, k0, R, t, K_T, depth_all, z_tol, ok, torch.float64)


def project_fp32(points, frame, xy, k0, R, t, K_T, depth_all, z_tol=0.05, ok=None):
    return _project(points, frame, xy, k0, R, t, K_T, depth_all, z_tol, ok, torch.float32)


def decision_margins(spec, depth_all, z_tol):
    """How far every live row of a float64 projection is from changing a flag -> (edge [T1,Q] px, |z| [T1,Q], |z - d (1 +
    z_tol)| / d [T1,Q] for the points inside (inf elsewhere)), inf on rows without a frame."""
    N, _, H, W = np.asarray(depth_all).shape
    edge, absz = S.edge_distance(spec['uv'], spec['z'], H, W)
    live = spec['target'] >= 0
    inf = torch.full_like(edge, float('inf'))
    d = spec['depth_at']
    occ = torch.where(spec['inside'] & (d > 0), (spec['z'] - d * (1 + z_tol)).abs() / d.clamp(min=1e-30), inf)
    return torch.where(live, edge, inf), torch.where(live, absz, inf), torch.where(live, occ, inf)


# -- cases of the GPU tests ----------------------------------------------------------------------------------------------------
def smooth_depth(N, H, W, seed):
    """Smooth, positive depth maps [N,1,H,W] float32: 2 + a low-frequency wave of amplitude 0.3."""
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    out = np.empty((N, 1, H, W), np.float32)
    for n in range(N):
        a, b, c = rng.uniform(0.05, 0.15, 3)
        out[n, 0] = 2.0 + 0.3 * np.sin(a * xx + b * yy + c * n + rng.uniform(0, 6))
    return out


def subpixel_seed_queries(N, H, W, Q, seed):
    """Q queries at sub-pixel positions of random frames; the first ones sit in the last column / row (x0 = W - 1, y0 = H - 1)
    and on a corner."""
    rng = np.random.RandomState(seed)
    frame = rng.randint(0, N, Q).astype(np.int32)
    xy = np.stack([rng.uniform(0, W - 1, Q), rng.uniform(0, H - 1, Q)], 1).astype(np.float32)
    fixed = [(W - 1, 3.25), (4.5, H - 1), (W - 1, H - 1), (0, 0), (W - 1.5, H - 1.25)]
    for i, p in enumerate(fixed[:Q]):
        xy[i] = p
    return frame, xy


def constructed_project_case(tabs, depth_all, T1, Q, k0, seed, z_tol=0.05):
    """World points whose projections are clear of every decision, by construction: per row (j, q) with a target frame g a
    chosen (u*, v*, z*) of g's camera is un-projected in float64.  u*, v* lie >= 1e-2 px from every image edge, inside or
    outside; z* is behind the camera (<= -0.05) or d(u*, v*) * f with f in [0.5, 0.97] or [1.15, 2] -- seen or occluded under
    z_tol = 0.05 with a margin of ~0.08 d.  -> (points float32 [T1,3,Q], frame int32 [Q], xy float32 [Q,2])."""
    rng = np.random.RandomState(seed)
    depth = torch.as_tensor(np.asarray(depth_all)).double()
    N, _, H, W = depth.shape
    R_T, t, Ki = (torch.as_tensor(np.asarray(tabs[k])).double() for k in ('R_T', 't', 'K_inv_T'))
    frame = rng.randint(0, N, Q).astype(np.int32)
    xy = np.stack([rng.uniform(0, W - 1, Q), rng.uniform(0, H - 1, Q)], 1).astype(np.float32)

    def coord(n):
        """[T1,Q] positions along an axis of n pixels: a quarter outside the image on either side, the rest inside."""
        inner = rng.uniform(1e-2, n - 1 - 1e-2, (T1, Q))
        outer = np.where(rng.rand(T1, Q) < 0.5, rng.uniform(-3.0, -1e-2, (T1, Q)), rng.uniform(n - 1 + 1e-2, n + 2.0, (T1, Q)))
        return torch.from_numpy(np.where(rng.randint(0, 4, (T1, Q)) == 0, outer, inner))

    u, v = coord(W), coord(H)
    kind = rng.randint(0, 5, (T1, Q))
    f = np.where(kind <= 2, rng.uniform(0.5, 0.97, (T1, Q)), rng.uniform(1.15, 2.0, (T1, Q)))
    behind = -rng.uniform(0.05, 1.0, (T1, Q))
    points = torch.from_numpy(rng.uniform(-1, 1, (T1, 3, Q)))          # (a row without a frame is never read)
    g_all = torch.from_numpy(frame.astype(np.int64))[None, :] + torch.arange(T1)[:, None] + k0
    for g in range(N):
        jj, qq = torch.nonzero(g_all == g, as_tuple=True)
        if not len(jj):
            continue
        d = S.sample_border(depth[g, 0], u[jj, qq], v[jj, qq])
        z = torch.where(torch.from_numpy(kind == 0)[jj, qq], torch.from_numpy(behind)[jj, qq], d * torch.from_numpy(f)[jj, qq])
        ray = torch.stack([u[jj, qq], v[jj, qq], torch.ones_like(z)], -1) @ Ki[g]
        points[jj, :, qq] = (z[:, None] * ray) @ R_T[g] + t[g]
    return points.float().numpy(), frame, xy


def score_case(T1, Q, N, origin, seed, thresholds=(1.0, 2.0, 4.0, 8.0, 16.0), sx=1.0, sy=1.0):
    """Predictions and a ground truth that exercise every branch of the score: errors exactly ON a squared threshold, gt occluded
    with the prediction visible and the reverse, unannotated states 2 and 255, rows without a frame, NaN and Inf predictions and
    errors above the cap.  -> dict of uv float32 [T1,Q,2], visible uint8 [T1,Q], target int32 [T1,Q], gt_uv float32 [Q,N,2],
    gt_state uint8 [Q,N]."""
    rng = np.random.RandomState(seed)
    frame = rng.randint(0, N, Q)
    target = (frame[None, :] + np.arange(T1)[:, None] - max(origin, 0)).astype(np.int64)
    target[(target < 0) | (target >= N)] = -1
    gt_uv = rng.uniform(0, 40, (Q, N, 2)).astype(np.float32)
    gt_state = rng.choice(np.array([0, 0, 0, 1, 2, 255], np.uint8), (Q, N))
    visible = (rng.rand(T1, Q) < 0.6).astype(np.uint8)
    uv = np.zeros((T1, Q, 2), np.float32)
    for j in range(T1):
        for q in range(Q):
            g = target[j, q]
            gu = gt_uv[q, max(g, 0)]
            kind = rng.randint(0, 10)
            if kind == 0:                                  # exactly on a threshold: du = thr (dyadic offsets of dyadic anchors)
                gt_uv[q, max(g, 0)] = np.floor(gu)
                uv[j, q] = gt_uv[q, max(g, 0)] + np.float32([thresholds[rng.randint(0, 5)], 0.0])
            elif kind == 1:
                uv[j, q] = [np.nan, gu[1]] if rng.rand() < 0.5 else [gu[0], np.inf]
            elif kind == 2:
                uv[j, q] = gu + np.float32([3000.0, -2000.0])      # above the cap
            else:
                uv[j, q] = gu + rng.uniform(-1, 1, 2).astype(np.float32) * np.float32(2.0 ** rng.randint(-2, 5))
    return {'uv': uv, 'visible': visible, 'target': target.astype(np.int32), 'gt_uv': gt_uv, 'gt_state': gt_state}


MODEL_QUERY_SEED = 5          # (changed, never the cap, if the queries it gives exceed the 0.5 % cap under the spec alone)


def model_queries(N, H, W, Q, seed=MODEL_QUERY_SEED):
    """Q sub-pixel queries [Q,3] of (frame, x, y) for the model-level tests, frames mixed."""
    rng = np.random.RandomState(seed)
    return np.stack([rng.randint(0, N, Q).astype(np.float64), rng.uniform(0, W - 1, Q), rng.uniform(0, H - 1, Q)], 1)


def pipeline(sd, tabs, depth_all, queries, n_steps, time_dependent=True, z_tol=0.05, inv_div=1.0 / 100.0):
    """Forward query tracks in float64: `seed`, tracks_spec.integrate on a [1,3,1,Q] slab, `project` (k0 = 0).  tabs: the six
    tables by name; sd: the scene-flow network's state dict.  -> project's dict plus points [T1,3,Q] and ok."""
    q = np.asarray(queries, np.float64)
    frame, xy = q[:, 0].astype(np.int64), q[:, 1:].astype(np.float32)
    N = np.asarray(depth_all).shape[0]
    P0, ok = seed(frame, xy, depth_all, tabs['R_T'], tabs['t'], tabs['K_inv_T'])
    Q = len(frame)
    ts = torch.as_tensor(np.asarray(tabs['ts_vali'])).double()[frame].view(1, 1, 1, Q) if time_dependent else None
    pts = S.integrate(sd, P0.view(1, 3, 1, Q), ts, 1.0 / N, [n_steps], n_steps, inv_div)[:, 0, :, 0, :]      # [T1,3,Q]
    out = project(pts, frame, xy, 0, tabs['R'], tabs['t'], tabs['K_T'], depth_all, z_tol, ok.numpy())
    out['points'], out['ok'] = pts, ok
    return out


def flag_skip(spec, depth_all, z_tol, edge=1e-3, zmin=1e-4, occ=1e-4):
    """[T1,Q] bool: the live rows whose flags hang on the last bits -- within `edge` px of an image edge, |z| < zmin, or
    |z - d (1 + z_tol)| < occ * d -- and the fraction of the live rows they are."""
    e, az, oc = decision_margins(spec, depth_all, z_tol)
    live = spec['target'] >= 0
    skip = live & ((e < edge) | (az < zmin) | (oc < occ))
    return skip, (float(skip.sum()) / max(1, int(live.sum())))


# -- the score -----------------------------------------------------------------------------------------------------------------
def thr2_of(thresholds):
    thr = np.asarray(thresholds, dtype=np.float32)
    return (thr * thr).astype(np.float32)


def score_mirror(uv, visible, target, origin, gt_uv, gt_state, thresholds=(1, 2, 4, 8, 16), sx=1.0, sy=1.0, shift=None):
    """The kernel's float32 operations in its order, vectorised -> int64 [T1,19]."""
    uv, gt_uv = np.asarray(uv, np.float32), np.asarray(gt_uv, np.float32)
    visible, target, gt_state = np.asarray(visible) != 0, np.asarray(target).astype(np.int64), np.asarray(gt_state)
    T1, Q = target.shape
    N = gt_state.shape[1]
    shift = eval_shift(Q) if shift is None else shift
    sx, sy, thr2 = np.float32(sx), np.float32(sy), thr2_of(thresholds)
    live = (target >= 0) & (target < N) & (np.arange(T1)[:, None] != origin)
    g = np.where(live, target, 0)
    qq = np.broadcast_to(np.arange(Q)[None, :], (T1, Q))
    st = gt_state[qq, g]
    ev = live & (st < 2)
    vis_gt = ev & (st == 0)
    with np.errstate(all='ignore'):
        du = ((uv[..., 0] - gt_uv[qq, g, 0]) * sx).astype(np.float32)
        dv = ((uv[..., 1] - gt_uv[qq, g, 1]) * sy).astype(np.float32)
        e2 = ((du * du).astype(np.float32) + (dv * dv).astype(np.float32)).astype(np.float32)
        err = np.fmin(np.sqrt(e2).astype(np.float32), np.float32(CAP))
    sums = np.zeros((T1, N_SUMS), np.int64)
    sums[:, 0] = ev.sum(1)
    sums[:, 1] = vis_gt.sum(1)
    sums[:, 2] = (ev & (visible == (st == 0))).sum(1)
    for i in range(5):
        with np.errstate(invalid='ignore'):
            within = e2 < thr2[i]
        sums[:, 3 + i] = (vis_gt & within).sum(1)
        sums[:, 8 + i] = (vis_gt & within & visible).sum(1)
        sums[:, 13 + i] = (ev & visible & (~(st == 0) | ~within)).sum(1)
    q = np.rint(np.where(vis_gt, err, 0).astype(np.float64) * float(2 ** shift)).astype(np.int64)
    sums[:, 18] = q.sum(1)
    return sums


def score_loop(uv, visible, target, origin, gt_uv, gt_state, thresholds=(1, 2, 4, 8, 16), sx=1.0, sy=1.0, shift=None):
    """The metric definitions, point by point, in Python integers -> list of T1 lists of 19 ints."""
    import math
    T1, Q = np.asarray(target).shape
    N = np.asarray(gt_state).shape[1]
    shift = eval_shift(Q) if shift is None else shift
    f32 = np.float32
    thr2 = [f32(f32(t) * f32(t)) for t in thresholds]
    out = [[0] * N_SUMS for _ in range(T1)]
    for j in range(T1):
        for q in range(Q):
            g = int(target[j][q])
            if g < 0 or g >= N or j == origin or int(gt_state[q][g]) >= 2:
                continue
            vis_gt, vis = int(gt_state[q][g]) == 0, bool(visible[j][q])
            with np.errstate(all='ignore'):
                du = f32(f32(f32(uv[j][q][0]) - f32(gt_uv[q][g][0])) * f32(sx))
                dv = f32(f32(f32(uv[j][q][1]) - f32(gt_uv[q][g][1])) * f32(sy))
                e2 = f32(f32(du * du) + f32(dv * dv))
            row = out[j]
            row[0] += 1
            row[1] += vis_gt
            row[2] += vis == vis_gt
            for i in range(5):
                within = bool(e2 < thr2[i])
                row[3 + i] += vis_gt and within
                row[8 + i] += vis_gt and within and vis
                row[13 + i] += vis and (not vis_gt or not within)
            if vis_gt:
                with np.errstate(all='ignore'):
                    e = float(f32(np.sqrt(e2)))
                e = CAP if (math.isnan(e) or e > CAP) else e
                row[18] += int(round(e * 2.0 ** shift))      # (round() on a float rounds half to even, as llrint does)
    return [[int(v) for v in row] for row in out]
