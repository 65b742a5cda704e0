"""The forward splat and Model.render restated in float64 (test infrastructure; plain numpy / torch on the CPU).

What dvd_splat_zmin / _accumulate / _resolve and Model.render compute, from the rules of include/dvd_hip.h and nothing of the
product, without the fixed-point quantisation of the accumulators:
  project   I = ((P - t) @ R) @ K_T ;  z = I.z ;  (u, v) = I.xy / (z + 1e-8)          (tracks_spec.project's formula)
  live      valid byte set, every value finite, z > z_near, z finite, -1 < u < W, -1 < v < H
  taps      (floor u + i, floor v + j) with the bilinear weights w; a tap counts iff it is inside the image and w >= w_tap
  zmin      per target pixel, the least z over the counting taps
  accepted  z <= zmin * (1 + z_tol);  weight = sum w;  image = sum w * clamp(c, +-bound) / sum w
  hit       weight >= w_min;  image = fill and depth = 0 elsewhere, depth = zmin where hit
Inputs are the fp32 values the kernels get (the parameters rounded to fp32 as the C ABI rounds them), promoted; `dtype` is the
precision of every operation: float64 is the specification, float32 the same expressions in the kernels' precision -- its
distance from the float64 result is what fp32 can do on the given inputs.

`fragile` marks the target pixels whose outcome hangs on last bits; `render` chains tracks_spec.unproject, the Euler steps
of tracks_spec.integrate and `splat`.
"""
import numpy as np
import torch

import tracks_spec

DEFAULTS = dict(z_near=1e-3, z_tol=0.05, w_tap=1.0 / 64, w_min=0.25, value_bound=1.0, fill=0.0)
W_EPS, Z_EPS = 1e-4, 1e-5


def _np(a, dtype):
    return np.ascontiguousarray(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a), dtype=dtype)


def splat(points, values, view, R, t, K_T, n_views, valid=None, planar=True, dtype=np.float64, **params):
    """-> dict of image [V,C,H,W], depth [V,1,H,W], weight [V,1,H,W], hit bool [V,H,W], zmin [V,H,W] (inf where empty) and
    'taps': per inside tap of a live point its view, pixel, weight, depth and whether it counts / is accepted."""
    p = dict(DEFAULTS)
    p.update(params)
    z_near, z_tol, w_tap, w_min, bound, fill = (dtype(np.float32(p[k])) for k in ('z_near', 'z_tol', 'w_tap', 'w_min',
                                                                                  'value_bound', 'fill'))
    points, values = _np(points, dtype), _np(values, dtype)
    if not planar:
        points = np.ascontiguousarray(points.transpose(0, 3, 1, 2))
    R, t, K_T = _np(R, dtype), _np(t, dtype), _np(K_T, dtype)
    S, C, H, W = values.shape
    V, HW = int(n_views), H * W
    view = [int(v) for v in np.asarray(view).reshape(-1)]
    one = dtype(1.0)
    tv, tp, tw, tz, tc = [], [], [], [], []
    for s in range(S):
        g = view[s]
        if g < 0 or g >= V:
            continue
        P = points[s].reshape(3, HW).T
        val = values[s].reshape(C, HW).T
        with np.errstate(all='ignore'):
            I = ((P - t[g]) @ R[g]) @ K_T[g]
            z = I[:, 2]
            den = z + dtype(1e-8)
            u, v = I[:, 0] / den, I[:, 1] / den
            live = np.isfinite(val).all(1) & (z > z_near) & np.isfinite(z) & (u > -1) & (u < W) & (v > -1) & (v < H)
            if valid is not None:
                live &= _np(valid, np.uint8)[s].reshape(HW) != 0
            u, v = np.where(live, u, 0).astype(dtype), np.where(live, v, 0).astype(dtype)
            x0, y0 = np.floor(u), np.floor(v)
            fx, fy = u - x0, v - y0
        for i in range(4):
            x, y = x0.astype(np.int64) + (i & 1), y0.astype(np.int64) + (i >> 1)
            w = (fx if i & 1 else one - fx) * (fy if i >> 1 else one - fy)
            m = live & (x >= 0) & (x < W) & (y >= 0) & (y < H)
            tv.append(np.full(int(m.sum()), g, dtype=np.int64))
            tp.append((y * W + x)[m])
            tw.append(w[m])
            tz.append(z[m])
            tc.append(val[m])
    cat = lambda parts, shape, dt: np.concatenate(parts) if parts else np.zeros(shape, dt)      # noqa: E731
    tv, tp = cat(tv, (0,), np.int64), cat(tp, (0,), np.int64)
    tw, tz, tc = cat(tw, (0,), dtype), cat(tz, (0,), dtype), cat(tc, (0, C), dtype)
    flat = tv * HW + tp
    counts = tw >= w_tap
    zmin = np.full(V * HW, np.inf, dtype=dtype)
    np.minimum.at(zmin, flat[counts], tz[counts])
    limit = zmin[flat] * (one + z_tol)
    accepted = counts & (tz <= limit)
    weight = np.zeros(V * HW, dtype=dtype)
    np.add.at(weight, flat[accepted], tw[accepted])
    acc = np.zeros((V * HW, C), dtype=dtype)
    np.add.at(acc, flat[accepted], tw[accepted, None] * (np.clip(tc[accepted], -bound, bound) / bound))
    hit = weight >= w_min
    with np.errstate(all='ignore'):
        image = np.where(hit[:, None], bound * acc / weight[:, None], fill).astype(dtype)
    depth = np.where(hit, zmin, 0).astype(dtype)
    return {'image': image.reshape(V, H, W, C).transpose(0, 3, 1, 2).copy(), 'depth': depth.reshape(V, 1, H, W),
            'weight': weight.reshape(V, 1, H, W), 'hit': hit.reshape(V, H, W), 'zmin': zmin.reshape(V, H, W),
            'taps': {'flat': flat, 'w': tw, 'z': tz, 'limit': limit, 'counts': counts, 'accepted': accepted},
            'params': {'w_tap': w_tap, 'w_min': w_min}}


def fragile(res):
    """bool [V,H,W]: the target pixels of a `splat` result whose outcome depends on last bits -- a tap reaching the pixel has
    |w - w_tap| < 1e-4, or a counting tap (accepted or rejected) has |z - zmin (1 + z_tol)| < 1e-5 relative, or the pixel has
    |weight - w_min| < 1e-4."""
    T, shape = res['taps'], res['hit'].shape
    out = np.zeros(int(np.prod(shape)), dtype=bool)
    near_w = np.abs(T['w'] - res['params']['w_tap']) < W_EPS
    with np.errstate(all='ignore'):
        near_z = T['counts'] & (np.abs(T['z'] - T['limit']) < Z_EPS * T['limit'])
    out[T['flat'][near_w | near_z]] = True
    out |= np.abs(res['weight'].reshape(-1) - res['params']['w_min']) < W_EPS
    return out.reshape(shape)


def fragile_share(res):
    return float(fragile(res).mean())


def taps_per_pixel(res):
    """The largest number of accepted taps one target pixel sums: the n of the quantisation term n * 2^-shift * bound."""
    T = res['taps']
    f = T['flat'][T['accepted']]
    return int(np.bincount(f).max()) if f.size else 0


def view_rows(tab_R, tab_t, tab_K_T, target):
    idx = [int(g) for g in target]
    return np.asarray(tab_R)[idx], np.asarray(tab_t)[idx], np.asarray(tab_K_T)[idx]


def render_points(sd, depth, frames, steps, tab_R_T, tab_t, tab_K_inv_T, ts_vali, n_frames, inv_div, dtype=np.float64):
    """World points of the source frames after steps[s] Euler steps -> [S,3,H,W].  float64: tracks_spec.unproject and
    tracks_spec.integrate.  float32: the same chain with the points held in fp32 between the steps (the MLP itself stays
    helpers.mlp_oracle_f64, which embeds in fp32 as the kernels do).  ts_vali None: a time-independent network; sd None with
    all steps 0: no network at all."""
    import helpers
    depth = _np(depth, np.float32)
    S, H, W = len(frames), depth.shape[2], depth.shape[3]
    p0 = tracks_spec.unproject(depth[frames], np.asarray(tab_R_T)[frames], np.asarray(tab_t)[frames],
                               np.asarray(tab_K_inv_T)[frames])
    n_steps = max(steps)
    if n_steps == 0:
        return p0.numpy().astype(dtype)
    ts = None
    if ts_vali is not None:
        ts = torch.from_numpy(np.asarray(ts_vali))[frames].view(S, 1, 1, 1).expand(S, 1, H, W)
    if dtype == np.float64:
        pts = tracks_spec.integrate(sd, p0, ts, 1.0 / n_frames, list(steps), n_steps, inv_div)
        return np.stack([pts[steps[s], s].numpy() for s in range(S)])
    sd = {k: v.double() for k, v in sd.items()}
    p = p0.float()
    for k in range(n_steps):
        rows = [s for s in range(S) if steps[s] > k]
        tt = None if ts is None else ts.double()[rows] + k * (1.0 / n_frames)
        sf = helpers.mlp_oracle_f64(sd, p[rows].double(), tt).float() * np.float32(inv_div)
        p[rows] = p[rows] + sf
    return p.numpy()


def render(sd, depth, img, target, sources, tab, n_frames, inv_div, advect=True, time_dependent=True, cam=None, valid=None,
           dtype=np.float64, **params):
    """Model.render from its inputs: depth [N,1,H,W], img [N,3,H,W], tab: the store's tables by name (R_T, R, t, K_T, K_inv_T,
    ts_vali), cam: (R, t, K_T) rows of the V views for novel cameras (default: rows `target` of the tables)."""
    frames, view, steps = [], [], []
    for v, (g, src) in enumerate(zip(target, sources)):
        for f in src:
            frames.append(int(f))
            view.append(v)
            steps.append(int(g) - int(f) if advect else 0)
    pts = render_points(sd, depth, frames, steps, tab['R_T'], tab['t'], tab['K_inv_T'], tab['ts_vali'] if time_dependent else None,
                        n_frames, inv_div, dtype=dtype)
    R, t, K_T = cam if cam is not None else view_rows(tab['R'], tab['t'], tab['K_T'], target)
    colours = _np(img, np.float32)[frames]
    mask = None if valid is None else _np(valid, np.uint8)[frames]
    return splat(pts, colours, view, R, t, K_T, len(target), valid=mask, planar=True, dtype=dtype, value_bound=1.0, **params)


def worst(a, b, mask=None):
    return tracks_spec.worst(a, b, mask)


# -- inputs the tests share -------------------------------------------------------------------------------------------------
def scene(S, V, H, W, C=3, seed=0, planar=True):
    """Smooth depth with a step edge seen from S cameras a few hundredths of a radian and a few tenths of a unit apart, drawn
    into V views: dict of fp32 points, values, view, R, t, K_T (numpy).  Source s looks at view s % V."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    f = 0.9 * W
    K = np.array([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1.0]])

    def pose(k, shift):
        th, ph = 0.03 * k + shift, -0.02 * k
        Ry = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(ph), -np.sin(ph)], [0, np.sin(ph), np.cos(ph)]])
        return Ry @ Rx, np.array([0.15 * k + 2 * shift, -0.1 * k, 0.05 * k])

    pts = np.zeros((S, 3, H, W))
    for s in range(S):
        Rc, tc = pose(s, 0.0)
        depth = 2.5 + 0.3 * np.sin(0.4 * xx + s) + 0.2 * np.cos(0.5 * yy) + 1.5 * (xx > 0.55 * W + s)
        ray = np.stack([xx, yy, np.ones_like(xx)], -1).reshape(-1, 3) @ np.linalg.inv(K).T
        P = (depth.reshape(-1, 1) * ray) @ Rc.T + tc
        pts[s] = P.T.reshape(3, H, W)
    R, t, K_T = np.zeros((V, 3, 3)), np.zeros((V, 3)), np.zeros((V, 3, 3))
    for v in range(V):
        Rc, tc = pose(v, 0.011)
        R[v], t[v], K_T[v] = Rc, tc, K.T
    values = rng.random((S, C, H, W))
    out = {'points': pts.astype(np.float32), 'values': values.astype(np.float32), 'view': [s % V for s in range(S)],
           'R': R.astype(np.float32), 't': t.astype(np.float32), 'K_T': K_T.astype(np.float32), 'n_views': V}
    if not planar:
        out['points'] = np.ascontiguousarray(out['points'].transpose(0, 2, 3, 1))
    return out


def two_planes(H=4, W=8):
    """Two fronto-parallel planes at z = 2 (colour 0.25) and z = 4 (colour 0.75) whose points land on the pixel centres of
    one identity-pose view: every weight is exactly 1."""
    f = 6.0
    K = np.array([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1.0]])
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    ray = np.stack([xx, yy, np.ones_like(xx)], -1).reshape(-1, 3) @ np.linalg.inv(K).T
    pts = np.stack([(z * ray).T.reshape(3, H, W) for z in (2.0, 4.0)])
    values = np.stack([np.full((1, H, W), 0.25), np.full((1, H, W), 0.75)])
    return {'points': pts.astype(np.float32), 'values': values.astype(np.float32), 'view': [0, 0],
            'R': np.eye(3, dtype=np.float32)[None], 't': np.zeros((1, 3), np.float32), 'K_T': K.T.astype(np.float32)[None],
            'n_views': 1}


def hostile(H=11, W=21):
    """The general scene into view 0 plus one more source image into view 1, a camera at the origin with f = 4 and the
    principal point at (2, 2): a point (X, Y, 1) lands at u = 4 X + 2, v = 4 Y + 2 exactly in fp32.  The image is a plane at
    z = 2 landing at (x + 0.3, y + 0.4); its first rows are overwritten with what a kernel must survive: NaN and +-inf
    coordinates, z = 0 and z < 0, u at exactly -1, 0, W - 1 and W, |u| and |v| = 1e9, and non-finite values."""
    base = scene(3, 1, H, W, C=3, seed=21)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    P = np.stack([(xx + 0.3 - 2) * 2 / 4, (yy + 0.4 - 2) * 2 / 4, np.full_like(xx, 2.0)]).astype(np.float32)
    vals = np.random.default_rng(22).random((3, H, W)).astype(np.float32)
    at = lambda u: (u - 2.0) / 4.0      # noqa: E731
    nan, inf = np.nan, np.inf
    bad = [(nan, 0, 1), (0, nan, 1), (0, 0, nan), (inf, 0, 1), (-inf, 0, 1), (0, inf, 1), (0, 0, inf), (0, 0, -inf), (inf, inf, inf),
           (0.1, 0.1, 0.0), (0.1, 0.1, -1.0), (0.1, 0.1, -0.0), (0.0, 0.0, 0.0), (0.1, 0.1, 1e-3), (0.1, 0.1, 1e-30),
           (at(-1), 0.125, 1), (at(0), 0.125, 1), (at(W - 1), 0.125, 1), (at(W), 0.125, 1), (0.125, at(-1), 1), (0.125, at(0), 1),
           (0.125, at(H - 1), 1), (0.125, at(H), 1), (1e9 / 4, 0.125, 1), (-1e9 / 4, 0.125, 1), (0.125, 1e9 / 4, 1),
           (0.125, -1e9 / 4, 1), (3e38, 3e38, 1), (-3e38, 3e38, 3e38), (1e9, 1e9, 1e-20), (at(-1), at(-1), 1),
           (at(W), at(H), 1), (at(W - 1), at(H - 1), 1), (at(-0.5), at(-0.5), 1), (at(W - 0.5), at(H - 0.5), 1)]
    assert len(bad) <= 2 * W
    for i, b in enumerate(bad):
        P[:, i // W, i % W] = np.array(b, dtype=np.float32)
    for i, b in enumerate((nan, inf, -inf)):      # ordinary points with a value that is not finite
        vals[i, 3, 2 + i] = b
    K1 = np.array([[4.0, 0, 2.0], [0, 4.0, 2.0], [0, 0, 1.0]])
    return {'points': np.concatenate([base['points'], P[None]]), 'values': np.concatenate([base['values'], vals[None]]),
            'view': [0, 0, 0, 1], 'R': np.concatenate([base['R'], np.eye(3, dtype=np.float32)[None]]),
            't': np.concatenate([base['t'], np.zeros((1, 3), np.float32)]),
            'K_T': np.concatenate([base['K_T'], K1.T.astype(np.float32)[None]]), 'n_views': 2, 'planar': True}


def run(case, dtype=np.float64, **params):
    return splat(case['points'], case['values'], case['view'], case['R'], case['t'], case['K_T'], case['n_views'],
                 valid=case.get('valid'), planar=case.get('planar', True), dtype=dtype, **params)


# the input sets of tests/test_48_splat_gpu.py: name -> (builder, splat parameters); test_splat_cpu.py checks the fragile cap
# of every one of them under the spec alone
def _with(case, **kw):
    case.update(kw)
    return case


def _masked(case, seed):
    S, _, H, W = case['values'].shape
    case['valid'] = (np.random.default_rng(seed).random((S, H, W)) > 0.2).astype(np.uint8)
    return case


def _scaled(case, lo, hi):
    case['values'] = (lo + (hi - lo) * case['values']).astype(np.float32)
    return case


CASES = {
    'general_11x21': (lambda: _with(scene(3, 2, 11, 21, C=3, seed=1), planar=True), {}),
    'general_12x20': (lambda: _with(scene(4, 2, 12, 20, C=3, seed=2), planar=True), {}),
    'one_view_16x24': (lambda: _with(scene(4, 1, 16, 24, C=3, seed=3), planar=True), {}),
    'c1_11x21': (lambda: _with(scene(3, 2, 11, 21, C=1, seed=4), planar=True), {}),
    'c8_12x20': (lambda: _with(scene(3, 1, 12, 20, C=8, seed=5), planar=True), {}),
    'interleaved_11x21': (lambda: _with(scene(3, 2, 11, 21, C=3, seed=6, planar=False), planar=False), {}),
    'interleaved_12x20': (lambda: _with(scene(3, 2, 12, 20, C=3, seed=7, planar=False), planar=False), {}),
    'skipped_views': (lambda: _with(scene(4, 2, 12, 20, C=3, seed=8), planar=True, view=[0, -1, 1, 2]), {}),
    'valid_mask': (lambda: _masked(_with(scene(3, 2, 11, 21, C=3, seed=9), planar=True), 10), {}),
    'negative_bound_4': (lambda: _scaled(_with(scene(3, 2, 11, 21, C=3, seed=12), planar=True), -3.5, 3.5), {'value_bound': 4.0}),
    'clamped': (lambda: _scaled(_with(scene(3, 2, 12, 20, C=3, seed=13), planar=True), -2.0, 2.0), {'value_bound': 1.0}),
    'two_planes': (lambda: _with(two_planes(), planar=True), {}),
    'hostile': (hostile, {}),
}
FRAGILE_CAP = 0.03


# -- Model.render on the store of tests/golden/tracks_b3_11x21_t4.npz (tests/test_49_render_gpu.py) ---------------------------
RENDER_FX = 'tracks_b3_11x21_t4'
RENDER_IMG_SEED = 5          # store_spec.random_tree(N, H, W, [1], 5): the store test_45 builds
RENDER_CASES = {
    'advect': dict(target=[3, 5], sources=[[1, 2, 3], [5]], advect=True, time_dependent=True, novel=False),
    'notime': dict(target=[3, 5], sources=[[1, 2, 3], [5]], advect=True, time_dependent=False, novel=False),
    'novel': dict(target=[3, 5], sources=[[1, 2, 3], [4, 5]], advect=True, time_dependent=True, novel=True),
    'held': dict(target=[3, 5], sources=[[2, 3, 4], [6, 5]], advect=False, time_dependent=True, novel=False),
    'own': dict(target=[2], sources=[[2]], advect=True, time_dependent=True, novel=False),
    'masked': dict(target=[3, 5], sources=[[1, 2, 3], [4, 5]], advect=True, time_dependent=True, novel=False, masked=True),
}


def left_half_mask(N, H, W):
    """uint8 [N,H,W]: the `valid` map of the 'masked' case -- the left half of every frame is dropped."""
    m = np.ones((N, H, W), dtype=np.uint8)
    m[:, :, : W // 2] = 0
    return m


def novel_poses(pose_c2w, target):
    """The target frames' camera-to-world poses with a small extra rotation about the camera's own y and x axes: float64
    [V,4,4]."""
    th, ph = 0.02, -0.015
    Ry = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(ph), -np.sin(ph)], [0, np.sin(ph), np.cos(ph)]])
    out = np.asarray(pose_c2w, dtype=np.float64)[[int(g) for g in target]].copy()
    out[:, :3, :3] = out[:, :3, :3] @ (Ry @ Rx)
    return out


def camera_rows(pose_c2w, K):
    """(R, t, K_T) fp32 rows of cameras given as camera-to-world poses [V,4,4] and intrinsics [V,3,3]: a point goes into
    the camera as (P - t) @ R with R the pose's rotation and t its translation, then through K."""
    pose_c2w, K = np.asarray(pose_c2w), np.asarray(K)
    return (pose_c2w[:, :3, :3].astype(np.float32), pose_c2w[:, :3, 3].astype(np.float32),
            np.ascontiguousarray(K.transpose(0, 2, 1)).astype(np.float32))


def render_case(fx, img, sd, name, dtype=np.float64, depth=None, **params):
    """`render` for RENDER_CASES[name] on the fixture's tables and depth; img [N,3,H,W]; sd: the network's state dict."""
    c = RENDER_CASES[name]
    tab = {k[4:]: fx[k] for k in fx if k.startswith('tab_')}
    cam = None
    if c['novel']:
        cam = camera_rows(novel_poses(fx['in_pose_c2w'], c['target']), fx['in_intrinsics'][c['target']])
    valid = left_half_mask(int(fx['N']), int(fx['H']), int(fx['W'])) if c.get('masked') else None
    return render(sd, fx['in_depth'] if depth is None else depth, img, c['target'], c['sources'], tab, int(fx['N']), 1.0 / 100.0,
                  advect=c['advect'], time_dependent=c['time_dependent'], cam=cam, valid=valid, dtype=dtype, **params)


def compare(name, got, r64, r32, params, shift, measured):
    """A kernel result `got` (numpy arrays) against the specification r64, with the fp32 specification r32 as the yardstick:
    shapes and dtypes; `hit` equal on every pixel that is not fragile; `fill` / 0 where nothing hit; and per quantity the
    distance from r64 on the non-fragile pixels at most
        4 x yardstick + n x 2^-shift x value_bound + 2^-24 x max|quantity|
    (fp32 with another operation order; the accumulators' quantisation, n = taps_per_pixel, none for the depth; the rounding of
    a result stored as fp32) and at most 4 x measured[quantity], the distance measured on the MI355X.  -> the distances."""
    import helpers
    V, C, H, W = r64['image'].shape
    assert got['image'].shape == (V, C, H, W) and got['image'].dtype == np.float32
    assert got['depth'].shape == got['weight'].shape == (V, 1, H, W) and got['hit'].shape == (V, H, W)
    assert got['hit'].dtype == np.uint8 and set(np.unique(got['hit'])) <= {0, 1}
    ok = ~fragile(r64)
    assert 1.0 - ok.mean() <= FRAGILE_CAP
    hit = got['hit'].astype(bool)
    bad = int(((hit != r64['hit']) & ok).sum())
    print('%s: %.2f %% fragile, %.0f %% hit, %d hit mismatches' % (name, 100 * (1 - ok.mean()), 100 * r64['hit'].mean(), bad))
    assert bad == 0
    assert not ((r64['hit'] != r32['hit']) & ok).any()
    fill = np.float32(params.get('fill', 0.0))
    assert (got['image'][np.broadcast_to(~hit[:, None], got['image'].shape)] == fill).all() and not got['depth'][~hit[:, None]].any()
    bound_v = float(np.float32(params.get('value_bound', 1.0)))
    quant = taps_per_pixel(r64) * 2.0 ** -shift
    out = {}
    for q in ('image', 'depth', 'weight'):
        m = np.broadcast_to((ok if q == 'weight' else ok & r64['hit'])[:, None], r64[q].shape)
        d_kernel, d_yard = worst(got[q], r64[q], m), worst(r32[q], r64[q], m)
        extra = {'image': quant * bound_v, 'weight': quant, 'depth': 0.0}[q] + 2.0 ** -24 * float(np.abs(r64[q][m]).max())
        limit = 4 * d_yard + extra
        helpers.log_measured('%s/%s' % (name, q), d_kernel, limit)
        print('measured %s/%s %.4g (yardstick %.4g, limit %.4g, 4 x measured %.4g)' % (name, q, d_kernel, d_yard, limit,
                                                                                       4 * measured[q]))
        assert d_kernel <= limit, (name, q, d_kernel, limit)
        assert d_kernel <= 4 * measured[q], (name, q, d_kernel, 4 * measured[q])
        out[q] = d_kernel
    return out
