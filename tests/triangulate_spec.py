"""Executable specification of the triangulation kernel (csrc/triangulate.hip, include/dvd_hip.h: dvd_triangulate) and the
synthetic video its tests use (test infrastructure; the product keeps no CPU path).

`observe` and `fuse` with dtype=np.float32 are the CONTRACT, operation for operation: numpy rounds every elementwise multiply,
add, subtract, divide and square root of float32 arrays once, IEEE, which is what the kernel does (built with
-ffp-contract=off).  The order of the operations:

  * K^-1 x and K y through the TRANSPOSED tables as a row vector times a row-major matrix, `_rowvec`:
        o_j = (v0 * M[0][j] + v1 * M[1][j]) + v2 * M[2][j]            (x's third component is the constant 1)
  * R y (camera to world) through the table R as `_matvec`:  o_i = (M[i][0] * v0 + M[i][1] * v1) + M[i][2] * v2
  * R^T y through the table R as `_rowvec`
  * every dot product as (p0 * q0 + p1 * q1) + p2 * q2
  * the cross product l = h0 x h1 as  l0 = h0_1 h1_2 - h0_2 h1_1,  l1 = h0_2 h1_0 - h0_0 h1_2,  l2 = h0_0 h1_1 - h0_1 h1_0
  * l . x' as (l0 * x'0 + l1 * x'1) + l2;  the norm as sqrt(l0 * l0 + l1 * l1)
  * den = A * C - Bq * Bq with AC = A * C formed once and used again in sin2 = den / AC
  * s1 = (E * C - Bq * F) / den,  s2 = (Bq * E - A * F) / den
  * the sums of the fusion in ascending table order, starting from 0; w * s1 is a multiply, then an add

dtype=np.float64 is the reference (the same statements on the same fp32 inputs).  `decided` flags an observation whose gates
are clear of their thresholds in the float64 reference, so that fp32 rounding does not flip them.  Its margin on sin2, 1e-3 of
the threshold, is smaller than fp32's own error of den = A C - Bq Bq at the default threshold (about 3e-3 of sin2 there): the
tests' scene, seed 0, has no observation in that gap; seed 2 has one.

Tables are numpy arrays in the FrameStore's layout: R [N,3,3] camera to world, t [N,3], K_T, K_inv_T [N,3,3] transposed.
"""
import numpy as np

CAP = 1e30
SIN2_MIN = 7.615242e-05          # ops.TRI_SIN2_MIN: sin^2 of 0.5 degrees
# worst distance of the kernel from the float64 reference on scene(24, 40, 7, seed=0, noise=0.4), measured on the MI355X
# (tests/test_61_triangulate_kernel_gpu.py; depth relative, epi in pixels); the tests' bound is 4 x this
MEASURED = {'median/depth': 1.212e-3, 'median/epi': 5.09e-6, 'mean/depth': 1.137e-3, 'mean/epi': 5.09e-6}
DEFAULTS = dict(epi_tol=1.0, sin2_min=SIN2_MIN, z_near=1e-3, min_count=2)


def _rowvec(v0, v1, v2, M):
    return [(v0 * M[0, j] + v1 * M[1, j]) + v2 * M[2, j] for j in range(3)]


def _matvec(M, v):
    return [(M[i, 0] * v[0] + M[i, 1] * v[1]) + M[i, 2] * v[2] for i in range(3)]


def _dot(p, q):
    return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]


def observe(flow, mask, tables, a, b, dtype=np.float32, epi_tol=1.0, sin2_min=SIN2_MIN, z_near=1e-3, **_):
    """One observation of query frame a against frame b for every pixel.  flow [H,W,2] fp32 (leaving a), mask [H,W] uint8.
    -> dict of s1, s2, sin2, e, xp, yp (dtype [H,W]) and usable, consistent (bool [H,W])."""
    H, W = mask.shape
    Ra, ta, Kia = (np.asarray(tables[k][a]).astype(dtype) for k in ('R', 't', 'K_inv_T'))
    Rb, tb, Kb, Kib = (np.asarray(tables[k][b]).astype(dtype) for k in ('R', 't', 'K_T', 'K_inv_T'))
    vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    uf, vf, one = uu.astype(dtype), vv.astype(dtype), dtype(1.0)
    thr = {k: dtype(np.float32(v)) for k, v in (('epi_tol', epi_tol), ('sin2_min', sin2_min), ('z_near', z_near))}
    cap = dtype(np.float32(CAP))
    fl = np.asarray(flow).astype(dtype)
    with np.errstate(all='ignore'):
        xp, yp = uf + fl[..., 0], vf + fl[..., 1]
        d1 = _matvec(Ra, _rowvec(uf, vf, one, Kia))
        d2 = _matvec(Rb, _rowvec(xp, yp, one, Kib))
        bl = [tb[i] - ta[i] for i in range(3)]
        g = [ta[i] - tb[i] for i in range(3)]
        A, Bq, C, E, F = _dot(d1, d1), _dot(d1, d2), _dot(d2, d2), _dot(d1, bl), _dot(d2, bl)
        AC = A * C
        den = AC - Bq * Bq
        s1, s2 = (E * C - Bq * F) / den, (Bq * E - A * F) / den
        sin2 = den / AC
        h0 = _rowvec(*_rowvec(g[0], g[1], g[2], Rb), Kb)
        h1 = _rowvec(*_rowvec(d1[0], d1[1], d1[2], Rb), Kb)
        l0 = h0[1] * h1[2] - h0[2] * h1[1]
        l1 = h0[2] * h1[0] - h0[0] * h1[2]
        l2 = h0[0] * h1[1] - h0[1] * h1[0]
        e = np.abs((l0 * xp + l1 * yp) + l2) / np.sqrt(l0 * l0 + l1 * l1)
        e = np.where(e <= cap, e, cap)
        usable = (np.asarray(mask) == 0) & (xp >= 0) & (xp <= dtype(W - 1)) & (yp >= 0) & (yp <= dtype(H - 1)) & (sin2 >= thr['sin2_min'])
        consistent = usable & (e <= thr['epi_tol']) & (s1 >= thr['z_near']) & (s1 <= cap) & (s2 >= thr['z_near']) & (s2 <= cap)
    full = lambda x: np.broadcast_to(x, (H, W)).astype(dtype)
    return {'s1': full(s1), 's2': full(s2), 'sin2': full(sin2), 'e': full(e), 'xp': xp, 'yp': yp, 'usable': usable,
            'consistent': consistent}


def decided(o, H, W, epi_tol=1.0, sin2_min=SIN2_MIN, z_near=1e-3, **_):
    """bool [H,W]: every gate of the (float64) observation `o` is clear of its threshold -- |e - epi_tol| >= 1e-3 px,
    |sin2 - sin2_min| >= 1e-3 sin2_min, |s - z_near| >= 1e-4 z_near for both s, and x' at least 1e-3 px from the image border
    (on either side of it).  A NaN is undecided."""
    et, sm, zn = (float(np.float32(v)) for v in (epi_tol, sin2_min, z_near))
    with np.errstate(all='ignore'):
        ok = np.abs(o['e'] - et) >= 1e-3
        ok &= np.abs(o['sin2'] - sm) >= 1e-3 * sm
        ok &= (np.abs(o['s1'] - zn) >= 1e-4 * zn) & (np.abs(o['s2'] - zn) >= 1e-4 * zn)
        for x, hi in ((o['xp'], W - 1.0), (o['yp'], H - 1.0)):
            ok &= (np.abs(x) >= 1e-3) & (np.abs(x - hi) >= 1e-3)
    return ok


def fuse(obs, mode='median', min_count=2, dtype=np.float32, **_):
    """The observations of one query frame (dicts of `observe`, in table order) -> depth, epi, spread (dtype [H,W]) and count,
    usable (uint8 [H,W])."""
    shape = obs[0]['s1'].shape if obs else None
    if shape is None:
        raise ValueError('fuse: no observation; use `empty`')
    zero = np.zeros(shape, dtype)
    acc, ws, esum = zero.copy(), zero.copy(), zero.copy()
    lo, hi = np.full(shape, np.inf, dtype), np.full(shape, -np.inf, dtype)
    n, nu = np.zeros(shape, np.int64), np.zeros(shape, np.int64)
    with np.errstate(all='ignore'):
        for o in obs:
            use, con, s1 = o['usable'], o['consistent'], o['s1']
            esum = np.where(use, esum + o['e'], esum)
            nu += use
            acc = np.where(con, acc + o['sin2'] * s1, acc)
            ws = np.where(con, ws + o['sin2'], ws)
            lo = np.where(con & (s1 < lo), s1, lo)
            hi = np.where(con & (s1 > hi), s1, hi)
            n += con
        if mode == 'median':
            S = np.sort(np.stack([np.where(o['consistent'], o['s1'], dtype(np.inf)) for o in obs], 0), axis=0)
            m_lo, m_hi = np.maximum(n - 1, 0) // 2, n // 2
            e_lo = np.take_along_axis(S, m_lo[None], 0)[0]
            e_hi = np.take_along_axis(S, np.minimum(m_hi, len(obs) - 1)[None], 0)[0]
            dep = np.where(n % 2 == 1, e_lo, (e_lo + e_hi) * dtype(0.5))
        elif mode == 'mean':
            dep = acc / ws
        else:
            raise ValueError(mode)
        dep = np.where((n >= min_count) & (n > 0), dep, dtype(0))
        spr = (hi - lo) / dep
        cap = dtype(np.float32(CAP))
        spr = np.where(dep != 0, np.where(spr <= cap, spr, cap), dtype(0))
        epi = np.where(nu > 0, esum / np.maximum(nu, 1).astype(dtype), dtype(-1))
    return {'depth': dep.astype(dtype), 'epi': epi.astype(dtype), 'spread': spr.astype(dtype), 'count': n.astype(np.uint8),
            'usable': nu.astype(np.uint8)}


def empty(H, W, dtype=np.float32):
    """What a frame without an observation gives."""
    return {'depth': np.zeros((H, W), dtype), 'epi': np.full((H, W), -1, dtype), 'spread': np.zeros((H, W), dtype),
            'count': np.zeros((H, W), np.uint8), 'usable': np.zeros((H, W), np.uint8)}


def pipeline(flow_1_2, flow_2_1, mask_1, mask_2, obs, frames, tables, mode='median', dtype=np.float32, **params):
    """ops.triangulate restated: the table `obs` [B,M,3] walked per frame.  -> dict of depth, epi, spread [B,1,H,W], count,
    usable [B,H,W], and decided [B,H,W] (every live observation of the pixel is decided -- meaningful for dtype=np.float64)."""
    p = dict(DEFAULTS)
    p.update(params)
    H, W = flow_1_2.shape[1:3]
    out = {k: [] for k in ('depth', 'epi', 'spread', 'count', 'usable', 'decided')}
    for i, a in enumerate(frames):
        seen, dec = [], np.ones((H, W), bool)
        for pair, b, d in (np.asarray(obs[i]).reshape(-1, 3).tolist() if len(obs) else []):
            if pair < 0:
                continue
            o = observe((flow_2_1 if d else flow_1_2)[pair], (mask_1 if d else mask_2)[pair], tables, int(a), int(b), dtype, **p)
            dec &= decided(o, H, W, **p)
            seen.append(o)
        r = fuse(seen, mode, p['min_count'], dtype) if seen else empty(H, W, dtype)
        r['decided'] = dec
        for k in out:
            out[k].append(r[k][None] if k in ('depth', 'epi', 'spread') else r[k])
    return {k: np.stack(v, 0) for k, v in out.items()}


# ---- the synthetic video ---------------------------------------------------------------------------------------------------

DISC_Z, DISC_R, DISC_V = 2.1, 0.3, (0.0, 0.15, 0.0)      # a fronto-parallel disc in front of the surface, moving ALONG y per frame
DISC_C0 = (0.36, -0.45)                                  # its centre in frame 0 (world x, y)


def _surface(x, y):
    return 3.6 + 0.7 * np.sin(0.7 * x) + 0.5 * np.cos(0.9 * y)          # world z of the static surface: 2.4 .. 4.8


def scene_cameras(H, W, N):
    """poses camera-to-world [N,4,4] and intrinsics [N,3,3], fp32: a camera moving sideways (0.12 i along x) with a small
    rotation (0.01 i rad about y)."""
    poses = np.tile(np.eye(4, dtype=np.float32), (N, 1, 1))
    for i in range(N):
        th = 0.01 * i
        poses[i, :3, :3] = [[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]]
        poses[i, :3, 3] = [0.12 * i, 0.0, 0.0]
    K = np.array([[0.9 * W, 0, (W - 1) / 2.0], [0, 0.9 * W, (H - 1) / 2.0], [0, 0, 1.0]], dtype=np.float32)
    return poses, np.tile(K, (N, 1, 1))


def tables_of(poses, intrinsics):
    """The FrameStore's camera tables of these files, by its own expressions (datasets/frame_store.py: _set_camera_row)."""
    N = len(poses)
    tab = {'R': np.zeros((N, 3, 3), np.float32), 't': np.zeros((N, 3), np.float32), 'K_T': np.zeros((N, 3, 3), np.float32),
           'K_inv_T': np.zeros((N, 3, 3), np.float32), 'R_T': np.zeros((N, 3, 3), np.float32)}
    for i in range(N):
        tab['R'][i], tab['R_T'][i], tab['t'][i] = poses[i, :3, :3], poses[i, :3, :3].T, poses[i, :3, 3]
        tab['K_T'][i], tab['K_inv_T'][i] = intrinsics[i].T, np.linalg.inv(intrinsics[i]).T
    return tab


def _bilinear_zeros(img, x, y):
    """F.grid_sample(align_corners=True, padding 'zeros') of img [H,W,C] at pixel positions (x, y), in float64."""
    H, W, _ = img.shape
    x0, y0 = np.floor(x), np.floor(y)
    out = 0.0
    for dx in (0, 1):
        for dy in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            w = (1 - np.abs(x - xi)) * (1 - np.abs(y - yi))
            ok = (xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1)
            v = img[np.clip(yi, 0, H - 1).astype(int), np.clip(xi, 0, W - 1).astype(int)]
            out = out + np.where(ok, w, 0.0)[..., None] * v
    return out


def consistency_masks(f12, f21):
    """flow_consistency_masks' rule restated (generate_flows.py:139-148): mask_k = [|warp(other flow) + own flow| > 1] or the
    target leaves the image; (mask_1, mask_2) uint8 [H,W]."""
    out = []
    for fa, fb in ((f12, f21), (f21, f12)):
        H, W, _ = fb.shape
        vv, uu = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
        tx, ty = uu + fb[..., 0], vv + fb[..., 1]
        err = np.linalg.norm(_bilinear_zeros(fa.astype(np.float64), tx, ty) + fb, axis=-1)
        out.append(((err > 1) | (tx < 0) | (tx > W - 1) | (ty < 0) | (ty > H - 1)).astype(np.uint8))
    return out[0], out[1]


def scene(H, W, N, seed=0, noise=0.0, gaps=(1, 2, 3, 4), masks='consistency'):
    """The test video -> dict: poses, intrinsics, tables, pairs [(f_1, f_2)] (gaps in order, f_1 ascending, every pair of the
    video), depth [N,H,W] float64 (true planar depth), disc bool [N,H,W], flow_1_2 / flow_2_1 fp32 [P,H,W,2] (un-project with the
    true depth, move the disc's points with the disc, re-project, all in float64; plus Gaussian noise of `noise` px; cast),
    mask_1 / mask_2 uint8 [P,H,W] (`masks`: 'consistency' or 'zero')."""
    rng = np.random.default_rng(seed)
    poses, Ks = scene_cameras(H, W, N)
    P64, K64 = poses.astype(np.float64), Ks.astype(np.float64)
    vv, uu = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    pix = np.stack([uu, vv, np.ones_like(uu)], -1)
    depth, disc, world = np.zeros((N, H, W)), np.zeros((N, H, W), bool), np.zeros((N, H, W, 3))
    vel = np.array(DISC_V)
    for i in range(N):
        ray = pix @ np.linalg.inv(K64[i]).T @ P64[i, :3, :3].T           # world direction with camera z = 1: s is the planar depth
        c = P64[i, :3, 3]
        s = np.full((H, W), 3.5)
        for _ in range(80):                                             # fixed point of the ray / height-field intersection
            s = (_surface(c[0] + s * ray[..., 0], c[1] + s * ray[..., 1]) - c[2]) / ray[..., 2]
        sd = (DISC_Z - c[2]) / ray[..., 2]
        hx, hy = c[0] + sd * ray[..., 0] - (DISC_C0[0] + i * vel[0]), c[1] + sd * ray[..., 1] - (DISC_C0[1] + i * vel[1])
        disc[i] = hx * hx + hy * hy < DISC_R ** 2
        depth[i] = np.where(disc[i], sd, s)
        world[i] = c + depth[i][..., None] * ray

    def flow(a, b):
        Pw = world[a] + np.where(disc[a][..., None], (b - a) * vel, 0.0)
        q = (Pw - P64[b, :3, 3]) @ P64[b, :3, :3] @ K64[b].T
        f = q[..., :2] / q[..., 2:] - pix[..., :2]
        return (f + noise * rng.standard_normal(f.shape)).astype(np.float32)

    pairs = [(a, a + g) for g in gaps for a in range(N - g)]
    f12 = np.stack([flow(a, b) for a, b in pairs], 0)
    f21 = np.stack([flow(b, a) for a, b in pairs], 0)
    if masks == 'zero':
        m1 = m2 = np.zeros((len(pairs), H, W), np.uint8)
    else:
        mm = [consistency_masks(f12[j], f21[j]) for j in range(len(pairs))]
        m1, m2 = np.stack([m[0] for m in mm], 0), np.stack([m[1] for m in mm], 0)
    return {'poses': poses, 'intrinsics': Ks, 'tables': tables_of(poses, Ks), 'pairs': pairs, 'depth': depth, 'disc': disc,
            'flow_1_2': f12, 'flow_2_1': f21, 'mask_1': m1, 'mask_2': m2, 'H': H, 'W': W, 'N': N}


def plan(pairs, frames, gaps=None):
    """preprocess.triangulate_plan restated: per frame the pairs that hold it, by |gap|, forward first, then pair index."""
    rows = []
    for f in frames:
        r = [(abs(b - a), 0 if a == f else 1, j, b if a == f else a) for j, (a, b) in enumerate(pairs)
             if f in (a, b) and (gaps is None or abs(b - a) in gaps)]
        rows.append([(j, o, d) for _, d, j, o in sorted(r)])
    M = max(len(r) for r in rows)
    obs = np.full((len(rows), M, 3), -1, np.int32)
    for i, r in enumerate(rows):
        for m, row in enumerate(r):
            obs[i, m] = row
    return obs


def against_reference(got, ref, min_count=2):
    """An fp32 result (the kernel's, or the fp32 contract's) against the float64 reference `ref` of `pipeline` over the pixels
    whose observations are all decided -> dict: excluded (share of pixels left out), counts_equal, depth (worst relative
    difference where both report a depth) and epi (worst difference in PIXELS where a usable observation exists: e has no scale
    of its own -- it is ~0 on a perfectly static pixel -- so a relative figure would measure nothing)."""
    ok = ref['decided']
    both = ok & (ref['count'] >= min_count) & (np.asarray(got['count']) >= min_count)
    seen = ok & (ref['usable'] > 0)
    return {'excluded': float((~ok).mean()),
            'counts_equal': bool(np.array_equal(np.asarray(got['count'])[ok], ref['count'][ok]) and
                                 np.array_equal(np.asarray(got['usable'])[ok], ref['usable'][ok])),
            'depth': worst_rel(np.asarray(got['depth'])[:, 0], ref['depth'][:, 0], both),
            'epi': float(np.max(np.abs(np.asarray(got['epi'], np.float64)[:, 0] - ref['epi'][:, 0])[seen])) if seen.any() else 0.0}


def worst_rel(a, b, where):
    """max |a - b| / |b| over `where`, in float64 (0 if `where` is empty)."""
    a, b = np.asarray(a, np.float64)[where], np.asarray(b, np.float64)[where]
    return float(np.max(np.abs(a - b) / np.abs(b))) if a.size else 0.0
