"""The camera refinement on the host: the specification's Jacobian against finite differences, what its Levenberg-Marquardt
loop recovers on the synthetic video (tests/pose_spec.py over triangulate_spec.scene), and the host-only plumbing of
preprocess.refine_plan / refine_cameras and ops.pose_normal_eq.

Measured here with the float64 specification on scene(24, 40, 7, seed=0, noise=0), frames 1 .. 6 perturbed by 1 degree and
0.03 (3.2e-2 in R, 4.4e-2 in c): the static weight brings every frame to 1.3e-9 / 4.8e-9 of the truth, log-scales to 3.8e-9;
the bound of these tests is 1e-6.  With all-ones weight the moving disc (10 % of the observations of a 24 x 40 image) pulls a
Huber loss to a wrong solution of LOWER cost than the true poses have -- which is why `weight` exists; the last recovery test
documents that instead of asserting a recovery.
"""
import types

import numpy as np
import pytest
import torch

import pose_spec as S
import triangulate_spec as T

H, W, N = 24, 40, 7


class _Ctx(object):
    pass


@pytest.fixture(scope='module')
def ctx():
    c = _Ctx()
    c.sc = T.scene(H, W, N, seed=0, noise=0.0)
    c.rows = S.plan(c.sc['pairs'])
    c.static = (~c.sc['disc']).astype(np.float32)
    c.true = c.sc['poses'].astype(np.float64)
    c.start = S.perturbed(c.sc)
    return c


def test_plan_and_scene(ctx):
    assert ctx.rows.shape == (36, 4) and ctx.rows[:2].tolist() == [[0, 0, 1, 0], [0, 1, 0, 1]]
    eR, ec = S.pose_errors(ctx.start, ctx.true)
    assert 2e-2 < eR < 5e-2 and 2e-2 < ec < 6e-2
    assert np.array_equal(ctx.start[0], ctx.true[0])


def test_jacobian_against_central_differences(ctx):
    """J^T r of the specification (huber = inf: the cost is sum w |r|^2 / 2 and its gradient J^T w r) against central
    differences of the float64 cost, step 1e-6, all 13 parameters of four rows: relative error at most 1e-6."""
    sc, inf = ctx.sc, 1e6
    sigma = np.zeros(N)
    worst = []
    for ri in (0, 3, 17, 35):
        row = ctx.rows[ri:ri + 1]
        ev = S.evaluator(sc, sc['depth'], ctx.static, row, huber=inf)
        g = ev(ctx.start, sigma)[0][0, 91:104]
        fd = np.zeros(13)
        for k in range(13):
            f, kk = (row[0, 1], k) if k < 7 else (row[0, 2], k - 7)
            cost = []
            for e in (1e-6, -1e-6):
                dx = np.zeros(7 * N)
                dx[7 * f + kk] = e
                p, s = S.retract(ctx.start, sigma, dx)
                cost.append(ev(p, s)[0][0, 104])
            fd[k] = (cost[0] - cost[1]) / 2e-6
        rel = np.abs(fd - g).max() / np.abs(g).max()
        print('row %d: J^T r against central differences %.3g' % (ri, rel))
        worst.append(rel)
    assert all(rel <= 1e-6 for rel in worst), worst


def test_the_blocks_are_those_of_the_jacobian(ctx):
    """The 91 stored entries are the upper triangle of a positive semi-definite 13 x 13 block, and cost, sum w |r|^2 and the
    counts agree with the per-pixel maps."""
    out = S.normal_eq64(ctx.sc, ctx.sc['depth'], ctx.static, ctx.rows[:4], S.tables_from(ctx.start, ctx.sc['tables']), None, 1.0, 1e-3)
    for r in range(4):
        blk = np.zeros((13, 13))
        for k, (i, j) in enumerate(S.TRI):
            blk[i, j] = blk[j, i] = out['sums'][r, k]
        assert np.linalg.eigvalsh(blk).min() > -1e-9 * np.abs(blk).max()
        assert out['counts'][r, 0] == (out['gate'][r] == 1).sum() and out['counts'][r, 1] == 0
        assert 0 < out['sums'][r, 105] and out['wsum'][r] <= out['counts'][r, 0]


def _recover(ctx, depth, weight, scales):
    return S.refine(S.evaluator(ctx.sc, depth, weight, ctx.rows), ctx.start, ctx.rows, scales=scales)


def test_recovery_with_the_static_weight(ctx):
    res = _recover(ctx, ctx.sc['depth'], ctx.static, False)
    eR, ec = S.pose_errors(res['poses'], ctx.true)
    print('recovery: R %.3g, c %.3g after %d iterations (%d accepted), cost %.3g -> %.3g' % (
        eR, ec, res['iterations'], res['accepted'], res['cost'][0], res['cost'][-1]))
    assert eR <= 1e-6 and ec <= 1e-6
    assert res['converged'] and res['cost'][-1] < 1e-6 * res['cost'][0] and not res['sigma'].any()
    assert np.array_equal(res['poses'][0], ctx.true[0])


def test_recovery_of_the_depth_scales(ctx):
    s = S.depth_scales(ctx.sc)
    res = _recover(ctx, ctx.sc['depth'] / s[:, None, None], ctx.static, True)
    eR, ec = S.pose_errors(res['poses'], ctx.true)
    es = np.abs(res['sigma'] - np.log(s)).max()
    print('recovery with scales: R %.3g, c %.3g, log-scale %.3g after %d iterations' % (eR, ec, es, res['iterations']))
    assert eR <= 1e-6 and ec <= 1e-6 and es <= 1e-6
    assert res['sigma'][0] == 0.0


def test_huber_alone_prefers_a_wrong_solution(ctx):
    """No recovery is asserted with weight=None: started AT the true poses, the loop moves to a solution whose cost is lower
    than the true poses' (the disc's residuals are bought down with small errors everywhere)."""
    ev = S.evaluator(ctx.sc, ctx.sc['depth'], None, ctx.rows)
    at_truth = S.assemble(ev(ctx.true, np.zeros(N))[0], ctx.rows, N)[2]
    res = S.refine(ev, ctx.start, ctx.rows)
    print('huber alone: cost at the true poses %.6g, at the end %.6g' % (at_truth, res['cost'][-1]))
    assert res['cost'][-1] < at_truth


# ---- plumbing ---------------------------------------------------------------------------------------------------------------

def test_refine_plan(ctx):
    from dvd_hip import preprocess
    pairs = ctx.sc['pairs']
    rows = preprocess.refine_plan(pairs, N)
    assert rows.dtype == np.int32 and np.array_equal(rows, ctx.rows)
    sub = preprocess.refine_plan(pairs, N, gaps=[2, 4])
    assert np.array_equal(sub, S.plan(pairs, (2, 4))) and len(sub) == 2 * (5 + 3)
    assert np.array_equal(preprocess.refine_plan([(3, 1)], 4), [[0, 3, 1, 0], [0, 1, 3, 1]])
    for kw, word in ((dict(pairs=[(0, 7)]), 'pair 0'), (dict(pairs=[(2, 2)]), 'pair 0'), (dict(gaps=[0]), 'gaps'), (dict(gaps=[]), 'gaps'),
                     (dict(gaps=[9]), 'no row'), (dict(pairs=[]), 'no row'), (dict(n_frames=0), 'n_frames')):
        with pytest.raises(ValueError, match=word):
            preprocess.refine_plan(**dict(dict(pairs=pairs, n_frames=N), **kw))


def _fake_store(ctx):
    cat = types.SimpleNamespace(pairs=list(ctx.sc['pairs']), n_frames=N)
    tab = {k: torch.from_numpy(np.array(v)) for k, v in ctx.sc['tables'].items()}
    return types.SimpleNamespace(cat=cat, H=H, W=W, device=torch.device('cpu'), depth_pred=torch.ones(N, 1, H, W), tables=tab,
                                 host_tables=tab, flow_1_2=None, flow_2_1=None, mask_1=None, mask_2=None)


def test_refine_cameras_names_the_argument_it_refuses(ctx):
    from dvd_hip import preprocess
    store = _fake_store(ctx)
    nan = float('nan')
    for kw, word in ((dict(depth=torch.ones(N, H, W)), 'depth'), (dict(depth=torch.ones(N, 1, H, W).double()), 'depth'),
                     (dict(depth=np.ones((N, 1, H, W), np.float32)), 'depth'), (dict(weight=torch.ones(N, 1, H, W)), 'weight'),
                     (dict(weight=torch.ones(N, H, W).bool()), 'weight'), (dict(gaps=[0]), 'gaps'), (dict(gaps=[11]), 'no row'),
                     (dict(anchor=N), 'anchor'), (dict(anchor=-1), 'anchor'), (dict(anchor=1.5), 'anchor'), (dict(anchor=True), 'anchor'),
                     (dict(scales=1), 'scales'), (dict(huber=0), 'huber'), (dict(huber=nan), 'huber'), (dict(huber='1'), 'huber'),
                     (dict(z_near=0.0), 'z_near'), (dict(z_near=float('inf')), 'z_near'), (dict(max_iter=0), 'max_iter'),
                     (dict(max_iter=2.5), 'max_iter'), (dict(rel_tol=-1e-9), 'rel_tol'), (dict(rel_tol=nan), 'rel_tol'),
                     (dict(tables={'R': store.tables['R']}), 'tables'), (dict(tables=dict(store.tables, t=store.tables['t'][:-1])), 'tables'),
                     (dict(tables=3), 'tables')):
        with pytest.raises(ValueError, match=word):
            preprocess.refine_cameras(store, **kw)
    with pytest.raises(RuntimeError, match='GPU tensor'):                # everything on the host is in order: the wrapper refuses
        preprocess.refine_cameras(store)


def test_pose_normal_eq_refuses_cpu_tensors(ctx):
    from dvd_hip import ops
    sc = ctx.sc
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    tab = {k: t(v) for k, v in sc['tables'].items()}
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ops.pose_normal_eq(t(sc['flow_1_2']), t(sc['flow_2_1']), t(sc['mask_1']), t(sc['mask_2']),
                           t(sc['depth'].astype(np.float32))[:, None], None, ctx.rows, tab, None, 1.0, 1e-3)
    for kw, word in ((dict(huber=0.0), 'huber'), (dict(z_near=-1.0), 'z_near'), (dict(rows=np.zeros((0, 4), np.int32)), 'rows'),
                     (dict(rows=np.zeros((3, 3), np.int32)), 'rows'), (dict(rows=[[0, 0, 1, 2]]), 'dir'),
                     (dict(log_scale=[0.0] * (N - 1)), 'log_scale'), (dict(log_scale=[float('nan')] * N), 'log_scale')):
        args = dict(flow_1_2=None, flow_2_1=None, mask_1=None, mask_2=None, depth=None, weight=None, rows=ctx.rows, tables=tab,
                    log_scale=[0.0] * N, huber=1.0, z_near=1e-3)
        with pytest.raises(RuntimeError, match=word):
            ops.pose_normal_eq(**dict(args, **kw))


def test_the_entry_validates_before_any_hip_call():
    from dvd_hip import _lib
    lib = _lib.load()
    import ctypes
    p = ctypes.c_void_p(64)                                              # never dereferenced: validation comes first
    nul = ctypes.c_void_p(0)

    def call(flow=p, rows=p, R=1, H=4, W=4, huber=1.0, z_near=1e-3, ws=p, ws_bytes=1 << 20, sums=p):
        return lib.dvd_pose_normal_eq(flow, p, p, p, 1, p, nul, p, p, p, p, p, 2, rows, huber, z_near, 10.0, ws, ws_bytes, sums, p, p,
                                      nul, nul, R, H, W, nul)
    for kw, word in ((dict(flow=nul), b'null'), (dict(rows=nul), b'null'), (dict(sums=nul), b'null'), (dict(ws=nul), b'null'),
                     (dict(R=0), b'R='), (dict(R=65536), b'R='), (dict(H=1 << 15, W=1 << 15), b'images'), (dict(huber=0.0), b'huber'),
                     (dict(huber=float('inf')), b'huber'), (dict(z_near=float('nan')), b'z_near'), (dict(z_near=0.0), b'z_near'),
                     (dict(ws_bytes=8), b'workspace')):
        assert call(**kw) == _lib.DVD_EINVAL, kw
        assert word in lib.dvd_last_error(), (kw, lib.dvd_last_error())
    assert lib.dvd_pose_workspace_bytes(3, 24, 40) == 3 * 1 * 109 * 8
    assert lib.dvd_pose_workspace_bytes(2, 72, 120) == 2 * 3 * 109 * 8
    assert lib.dvd_pose_workspace_bytes(0, 4, 4) == 0
