"""Executable specification of the camera refinement (csrc/pose.hip, include/dvd_hip.h: dvd_pose_normal_eq;
preprocess.refine_plan / refine_cameras) -- test infrastructure; the product keeps no CPU path.  The video is
triangulate_spec.scene.

`normal_eq` with dtype=np.float32 is the CONTRACT of the per-pixel quantities `resid` and `gate`, operation for operation:
numpy rounds every elementwise multiply, add, subtract and divide of float32 arrays once, IEEE, which is what the kernel does
(built with -ffp-contract=off).  Per row (pair, a, b, dir) and pixel x = (u, v, 1) of frame a, with the tables' rows of both
frames (R camera to world, c = t, K_T and K_inv_T transposed), triangulate_spec's `_rowvec` / `_matvec`:

    ray = _rowvec(u, v, 1, K_inv_T[a])          Ds = D * s_a          P_i = Ds * ray_i
    X = _matvec(R[a], P)       Z_i = X_i + (t[a]_i - t[b]_i)       Y = _rowvec(Z, R[b])       q = _rowvec(Y, K_T[b])
    proj = (q_0 / q_2, q_1 / q_2)      x' = (u + flow_0, v + flow_1)      r = proj - x'

    considered   mask byte == 0 && D > 0 && D <= FLT_MAX && weight > 0 && 0 <= x'_0 <= W-1 && 0 <= x'_1 <= H-1
    gate         0 not considered;  1 considered && q_2 >= z_near (live);  2 considered && !(q_2 >= z_near)
    resid        r where gate == 1, (0, 0) elsewhere

(a NaN fails every comparison).  s_a, huber, z_near and the penalty reach the kernel as float32: s_a = float32(exp(sigma_a)),
penalty = float32(huber * (hypot(W, H) - huber / 2)) of the float32 huber -- Huber's rho of a residual as long as the image's
diagonal, hypot(W, H)^2 / 2 should huber exceed it -- both formed in float64 on the host.

dtype=np.float64 is the reference of the sums (the same statements on the same fp32 inputs) and of the Jacobian: with
|r| = sqrt(r_0 r_0 + r_1 r_1), Huber's rho and IRLS weight times weight_a(x), M = R_b^T R_a, [v]x the cross-product matrix,
Pi = (1 / q_2) [[1, 0, -proj_0], [0, 1, -proj_1]] and the 13 unknowns [tau_a, omega_a, sigma_a, tau_b, omega_b] of the row

    J = Pi K_b [ M | -M [P]x | M P | -I | [Y]x ]                                     (2 x 13)
    sums[0:91]   upper triangle of J^T w J, row-major (i <= j)       sums[91:104]  J^T w r
    sums[104]    cost = sum weight * rho over the live + penalty * (sum of weight over gate == 2)
    sums[105]    sum of w |r|^2 over the live           wsum = sum of w over the live          counts = (#gate == 1, #gate == 2)

`refine` restates preprocess.refine_cameras' Levenberg-Marquardt loop over any `evaluate` (the float64 `normal_eq` here; the
kernel's in tests/test_72_refine_cameras_gpu.py).
"""
import numpy as np

from triangulate_spec import _matvec, _rowvec

NS = 106
TRI = [(i, j) for i in range(13) for j in range(i, 13)]          # the order of sums[0:91]
# worst distance of the kernel from the float64 reference measured on the MI355X (tests/test_71_pose_kernel_gpu.py: per row
# ||got - ref||_F / ||ref||_F over the three shapes; tests/test_72_refine_cameras_gpu.py: refine_cameras against `refine`,
# absolute, in the Frobenius norm of R, the 2-norm of c and |scale|); the tests' bound is 4 x this
MEASURED = {'sums/JtJ': 3.038e-7, 'sums/Jtr': 2.920e-6, 'sums/cost': 8.209e-7, 'sums/wr2': 6.985e-7, 'sums/wsum': 3.595e-7, 'refine/R': 1.342e-7, 'refine/c': 4.221e-7, 'refine/scale': 1.192e-7}


def plan(pairs, gaps=None):
    """preprocess.refine_plan restated: rows (pair, a, b, dir), pairs in stored order, dir 0 before dir 1."""
    rows = []
    for j, (a, b) in enumerate(pairs):
        if gaps is None or abs(b - a) in gaps:
            rows += [(j, a, b, 0), (j, b, a, 1)]
    return np.array(rows, np.int32).reshape(-1, 4)


def params32(H, W, huber=1.0, z_near=1e-3):
    """(huber, z_near, penalty) as the float32 values the kernel receives."""
    h, far = float(np.float32(huber)), float(np.hypot(float(W), float(H)))
    return np.float32(h), np.float32(z_near), np.float32(h * (far - h / 2) if far > h else far * far / 2)


def scales32(log_scale, N):
    return np.ones(N, np.float32) if log_scale is None else np.exp(np.asarray(log_scale, np.float64)).astype(np.float32)


def row_eq(flow, mask, depth, weight, tables, a, b, s_a, huber, z_near, pen, dtype=np.float32, jacobian=True):
    """One row -> dict: resid [H,W,2] dtype, gate uint8 [H,W], and (jacobian) sums [106], wsum, counts [2] in float64
    arithmetic of dtype-typed per-pixel quantities (meaningful as a reference for dtype=np.float64)."""
    H, W = mask.shape
    Ra, ta, Kia = (np.asarray(tables[k][a]).astype(dtype) for k in ('R', 't', 'K_inv_T'))
    Rb, tb, Kb = (np.asarray(tables[k][b]).astype(dtype) for k in ('R', 't', 'K_T'))
    vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    uf, vf, one = uu.astype(dtype), vv.astype(dtype), dtype(1.0)
    fl, D = np.asarray(flow).astype(dtype), np.asarray(depth).astype(dtype)
    wgt = np.ones((H, W), dtype) if weight is None else np.asarray(weight).astype(dtype)
    hub, zn, pen = dtype(np.float32(huber)), dtype(np.float32(z_near)), dtype(np.float32(pen))
    with np.errstate(all='ignore'):
        ray = _rowvec(uf, vf, one, Kia)
        Ds = D * dtype(np.float32(s_a))
        P = [Ds * ray[i] for i in range(3)]
        X = _matvec(Ra, P)
        Z = [X[i] + (ta[i] - tb[i]) for i in range(3)]
        Y = _rowvec(Z[0], Z[1], Z[2], Rb)
        q = _rowvec(Y[0], Y[1], Y[2], Kb)
        proj = [q[0] / q[2], q[1] / q[2]]
        xp, yp = uf + fl[..., 0], vf + fl[..., 1]
        r = [proj[0] - xp, proj[1] - yp]
        ok = (np.asarray(mask) == 0) & (D > 0) & (D <= dtype(np.finfo(np.float32).max)) & (wgt > 0)
        ok &= (xp >= 0) & (xp <= dtype(W - 1)) & (yp >= 0) & (yp <= dtype(H - 1))
        live = ok & (q[2] >= zn)
        gate = np.where(live, 1, np.where(ok, 2, 0)).astype(np.uint8)
        resid = np.stack([np.where(live, r[0], dtype(0)), np.where(live, r[1], dtype(0))], -1).astype(dtype)
    out = {'resid': resid, 'gate': gate, 'qz': np.broadcast_to(q[2], (H, W)).astype(dtype)}
    if not jacobian:
        return out
    f8 = np.float64
    with np.errstate(all='ignore'):
        r0, r1 = np.where(live, r[0], 0).astype(f8), np.where(live, r[1], 0).astype(f8)
        nr2 = r0 * r0 + r1 * r1
        nr = np.sqrt(nr2)
        h = f8(hub)
        inside = nr <= h
        irls = np.where(inside, 1.0, h / np.where(inside, 1.0, nr))
        rho = np.where(inside, 0.5 * nr2, h * (nr - 0.5 * h))
        w8 = wgt.astype(f8)
        w = np.where(live, w8 * irls, 0.0)
        iz = np.where(live, 1.0 / np.where(live, q[2], 1).astype(f8), 0.0)
        pj = [np.where(live, proj[i], 0).astype(f8) for i in range(2)]
        K = Kb.astype(f8).T                                                    # K_b itself
        A = [[(K[i, j] - pj[i] * K[2, j]) * iz for j in range(3)] for i in range(2)]
        M = Rb.astype(f8).T @ Ra.astype(f8)
        Pf = [np.where(live, P[i], 0).astype(f8) * np.ones((H, W)) for i in range(3)]
        Yf = [np.where(live, Y[i], 0).astype(f8) * np.ones((H, W)) for i in range(3)]
        J = []
        for i in range(2):
            B = [A[i][0] * M[0, k] + A[i][1] * M[1, k] + A[i][2] * M[2, k] for k in range(3)]
            J.append(B + [B[2] * Pf[1] - B[1] * Pf[2], B[0] * Pf[2] - B[2] * Pf[0], B[1] * Pf[0] - B[0] * Pf[1],
                          B[0] * Pf[0] + B[1] * Pf[1] + B[2] * Pf[2], -A[i][0], -A[i][1], -A[i][2],
                          A[i][1] * Yf[2] - A[i][2] * Yf[1], A[i][2] * Yf[0] - A[i][0] * Yf[2], A[i][0] * Yf[1] - A[i][1] * Yf[0]])
        J = np.stack([np.stack(j, -1) for j in J], -2)                         # [H,W,2,13]
        rr = np.stack([r0, r1], -1)
        JtJ = np.einsum('hwij,hw,hwik->jk', J, w, J)
        Jtr = np.einsum('hwij,hw,hwi->j', J, w, rr)
        sums = np.zeros(NS)
        sums[:91] = [JtJ[i, j] for i, j in TRI]
        sums[91:104] = Jtr
        sums[104] = np.where(live, w8 * rho, 0.0).sum() + f8(pen) * np.where(gate == 2, w8, 0.0).sum()
        sums[105] = (w * nr2).sum()
    out.update(sums=sums, wsum=float(w.sum()), counts=np.array([(gate == 1).sum(), (gate == 2).sum()], np.int64))
    return out


def normal_eq(flow_1_2, flow_2_1, mask_1, mask_2, depth, weight, rows, tables, log_scale=None, huber=1.0, z_near=1e-3,
              dtype=np.float32, jacobian=True, P=None):
    """ops.pose_normal_eq restated -> dict of resid [R,H,W,2], gate [R,H,W], qz [R,H,W] and (jacobian) sums float64 [R,106],
    wsum float64 [R], counts int64 [R,2].  depth [N,H,W] (or [N,1,H,W]), weight [N,H,W] or None.  A row whose pair or frame
    lies outside the stores gives zeros."""
    depth = np.asarray(depth)
    depth = depth.reshape(depth.shape[0], depth.shape[-2], depth.shape[-1])
    N, H, W = depth.shape
    P = len(flow_1_2) if P is None else P
    hub, zn, pen = params32(H, W, huber, z_near)
    sc = scales32(log_scale, N)
    out = {k: [] for k in ('resid', 'gate', 'qz') + (('sums', 'wsum', 'counts') if jacobian else ())}
    zero = {'resid': np.zeros((H, W, 2), dtype), 'gate': np.zeros((H, W), np.uint8), 'qz': np.zeros((H, W), dtype),
            'sums': np.zeros(NS), 'wsum': 0.0, 'counts': np.zeros(2, np.int64)}
    for pair, a, b, d in np.asarray(rows).reshape(-1, 4).tolist():
        if not (0 <= pair < P and 0 <= a < N and 0 <= b < N):
            r = zero
        else:
            r = row_eq((flow_2_1 if d else flow_1_2)[pair], (mask_1 if d else mask_2)[pair], depth[a],
                       None if weight is None else weight[a], tables, a, b, sc[a], hub, zn, pen, dtype, jacobian)
        for k in out:
            out[k].append(r[k])
    return {k: np.stack(v, 0) if k != 'wsum' else np.array(v, np.float64) for k, v in out.items()}


def decided(ref, z_near=1e-3):
    """bool [R,H,W]: the one gate that rounding can flip, q_2 >= z_near, is clear of its threshold in the float64 reference
    `ref` of normal_eq: |q_2 - z_near| >= 1e-4 z_near.  (The other gates are single fp32 operations on the inputs.)  A NaN is
    undecided."""
    zn = float(np.float32(z_near))
    with np.errstate(all='ignore'):
        return np.abs(ref['qz'].astype(np.float64) - zn) >= 1e-4 * zn


# ---- the Levenberg-Marquardt loop ------------------------------------------------------------------------------------------

def hat(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def exp_so3(w):
    """Rodrigues in float64."""
    w = np.asarray(w, np.float64)
    th = float(np.sqrt(w @ w))
    K = hat(w)
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * (K @ K)
    return np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / (th * th)) * (K @ K)


def retract(poses, sigma, dx):
    """poses float64 [N,4,4], sigma [N], dx [7N] -> the stepped copies: c += R tau, R <- R Exp(omega), sigma += dsigma."""
    p, s = poses.copy(), sigma.copy()
    for f in range(len(poses)):
        d = dx[7 * f:7 * f + 7]
        if not d.any():
            continue
        p[f, :3, 3] = poses[f, :3, 3] + poses[f, :3, :3] @ d[0:3]
        p[f, :3, :3] = poses[f, :3, :3] @ exp_so3(d[3:6])
        s[f] = sigma[f] + d[6]
    return p, s


def assemble(sums, rows, N):
    """The rows' 13 x 13 blocks -> (H [7N,7N], g [7N], cost), float64."""
    Hm, g = np.zeros((7 * N, 7 * N)), np.zeros(7 * N)
    for s, (_, a, b, _) in zip(sums, np.asarray(rows).tolist()):
        idx = np.r_[7 * a:7 * a + 7, 7 * b:7 * b + 6]
        blk = np.zeros((13, 13))
        for k, (i, j) in enumerate(TRI):
            blk[i, j] = blk[j, i] = s[k]
        Hm[np.ix_(idx, idx)] += blk
        g[idx] += s[91:104]
    return Hm, g, float(np.sum(sums[:, 104]))


def free_columns(rows, N, anchor, scales):
    seen = set(np.asarray(rows)[:, 1:3].ravel().tolist())
    return [i for i in range(7 * N) if i // 7 != anchor and i // 7 in seen and (scales or i % 7 != 6)]


STALL = 5                    # preprocess.POSE_STALL


def refine(evaluate, poses, rows, anchor=0, scales=False, max_iter=30, rel_tol=1e-9):
    """refine_cameras' loop.  evaluate(poses float64 [N,4,4], sigma float64 [N]) -> (sums float64 [R,106], anything).
    -> dict: poses, sigma (float64), cost (the history), iterations, accepted, converged, first / last (evaluate's second
    value at the start and at the accepted end)."""
    N = len(poses)
    poses, sigma = np.array(poses, np.float64), np.zeros(N)
    free = free_columns(rows, N, anchor, scales)
    sums, first = evaluate(poses, sigma)
    Hm, g, cost = assemble(sums, rows, N)
    hist, lam, accepted, rejected, converged, last, it = [cost], 1e-3, 0, 0, False, first, 0
    for it in range(1, max_iter + 1):
        Hf, gf = Hm[np.ix_(free, free)], g[free]
        A = Hf + lam * np.diag(np.diag(Hf))
        try:
            step = np.linalg.solve(A, -gf)
        except np.linalg.LinAlgError:
            step = np.linalg.lstsq(A, -gf, rcond=None)[0]
        dx = np.zeros(7 * N)
        dx[free] = step
        p2, s2 = retract(poses, sigma, dx)
        sums2, aux2 = evaluate(p2, s2)
        H2, g2, c2 = assemble(sums2, rows, N)
        if c2 < cost:
            drop = cost - c2
            small = drop < rel_tol * cost
            poses, sigma, Hm, g, cost, last = p2, s2, H2, g2, c2, aux2
            lam, accepted, rejected = lam / 10, accepted + 1, 0
            hist.append(cost)
            if small:
                converged = True
                break
        else:
            lam, rejected = lam * 10, rejected + 1
            hist.append(cost)
            if accepted and rejected >= STALL:          # no step lowers the cost any more: it is at its rounding floor
                converged = True
                break
    return {'poses': poses, 'sigma': sigma, 'cost': hist, 'iterations': it, 'accepted': accepted, 'converged': converged,
            'first': first, 'last': last}


def tables_from(poses, base):
    """`base`'s tables with R, t (and R_T) of fp32 `poses` [N,4,4]: what refine_cameras hands to the kernel."""
    p = np.asarray(poses, np.float32)
    tab = {k: np.array(v) for k, v in base.items()}
    tab['R'], tab['t'] = np.ascontiguousarray(p[:, :3, :3]), np.ascontiguousarray(p[:, :3, 3])
    if 'R_T' in tab:
        tab['R_T'] = np.ascontiguousarray(p[:, :3, :3].transpose(0, 2, 1))
    return tab


def evaluator(sc, depth, weight, rows, huber=1.0, z_near=1e-3, round32=False, base=None):
    """`evaluate` for `refine` from the float64 normal_eq over a scene.  round32: poses rounded to fp32 and log-scales through
    float32(exp(.)), as the product does before each launch; otherwise everything stays float64."""
    base = sc['tables'] if base is None else base

    def evaluate(poses, sigma):
        if round32:
            tab, ls = tables_from(poses.astype(np.float32), base), sigma
            dep = depth
        else:
            tab = {k: np.asarray(v, np.float64) for k, v in base.items()}
            tab['R'], tab['t'] = poses[:, :3, :3], poses[:, :3, 3]
            tab['K_inv_T'] = np.linalg.inv(tab['K_T'])                 # (the inverse in float64 too, not the table's fp32 one)
            dep, ls = np.asarray(depth, np.float64).reshape(len(poses), sc['H'], sc['W']) * np.exp(sigma)[:, None, None], None
        out = normal_eq64(sc, dep, weight, rows, tab, ls, huber, z_near)
        return out['sums'], out
    return evaluate


def normal_eq64(sc, depth, weight, rows, tables, log_scale, huber, z_near):
    """normal_eq in float64 whose tables and depth may themselves be float64 (row_eq casts its inputs to dtype: nothing is
    lost)."""
    return normal_eq(sc['flow_1_2'], sc['flow_2_1'], sc['mask_1'], sc['mask_2'], depth, weight, rows, tables, log_scale, huber,
                     z_near, np.float64)


def perturbed(sc, seed=5, deg=1.0, shift=0.03):
    """The tests' start: frames 1 .. N-1 of the scene's true poses turned by Exp(deg * U(-1,1)^3) and moved by
    shift * U(-1,1)^3 (one generator, frame by frame, rotation first) -> float64 [N,4,4]."""
    rng = np.random.default_rng(seed)
    p = sc['poses'].astype(np.float64).copy()
    for f in range(1, len(p)):
        p[f, :3, :3] = p[f, :3, :3] @ exp_so3(np.deg2rad(deg) * rng.uniform(-1, 1, 3))
        p[f, :3, 3] += shift * rng.uniform(-1, 1, 3)
    return p


def depth_scales(sc, seed=5):
    """The scales the scale tests divide the depth by: exp(0.1 * U(-1,1)) per frame with s_0 = 1, drawn from `perturbed`'s
    generator after its own draws."""
    rng = np.random.default_rng(seed)
    rng.uniform(-1, 1, (len(sc['poses']) - 1, 2, 3))
    s = np.exp(0.1 * rng.uniform(-1, 1, len(sc['poses'])))
    s[0] = 1.0
    return s


def pose_errors(p, true):
    """(worst Frobenius norm of R - R_true, worst 2-norm of c - c_true) over the frames."""
    p, true = np.asarray(p, np.float64), np.asarray(true, np.float64)
    return (max(np.linalg.norm(p[f, :3, :3] - true[f, :3, :3]) for f in range(len(p))),
            max(np.linalg.norm(p[f, :3, 3] - true[f, :3, 3]) for f in range(len(p))))


def rel_rows(got, ref):
    """Worst over the rows of ||got - ref||_F / ||ref||_F (rows whose reference is all zero must be zero, and count as 0)."""
    got, ref = np.asarray(got, np.float64).reshape(len(ref), -1), np.asarray(ref, np.float64).reshape(len(ref), -1)
    worst = 0.0
    for g, r in zip(got, ref):
        n = np.linalg.norm(r)
        worst = max(worst, np.linalg.norm(g - r) / n if n > 0 else (0.0 if not g.any() else np.inf))
    return float(worst)
