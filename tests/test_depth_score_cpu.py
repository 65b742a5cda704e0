"""CPU-only checks of the depth metrics (csrc/select.hip, csrc/depth_score.hip, ops.ratio_median, ops.depth_score,
preprocess.calibrate_scale / scale_poses): the two C entries exist, are declared, and refuse bad arguments before any HIP call;
the specification's median (tests/depth_score_spec.py) is np.median bit for bit and equals the stated rule on every data class the
GPU tests use; scale_poses is the reference's three statements; the calibration fixture regenerates from the reference's own
statements -- plus the condition every GPU comparison rests on: under the specification alone, at most 1 % of the pixels of every
input set the GPU tests use are fragile."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import depth_score_spec as D
import helpers

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
REF = '/root/reference'
P = ctypes.c_void_p(64)      # a non-null, 64-byte aligned pointer that is never followed: every call below is refused first


def _lib():
    from dvd_hip import _lib
    return _lib, _lib.load()


def _err(lib):
    return lib.dvd_last_error().decode()


def _median(lib, **over):
    a = dict(num=P, den=P, mask=P, den_min=0.0, S=3, L=1000, median=P, count=P, ws=P, ws_bytes=3 * 8224)
    a.update(over)
    return lib.dvd_ratio_median(a['num'], a['den'], a['mask'], a['den_min'], a['S'], a['L'], a['median'], a['count'], a['ws'],
                                a['ws_bytes'], None)


def _score(lib, **over):
    a = dict(pred=P, gt=P, scale=P, seg=P, mask=P, g_min=1e-2, shift=32, sums=P, maps=P, counted=P, N=3, H=11, W=21)
    a.update(over)
    return lib.dvd_depth_score(a['pred'], a['gt'], a['scale'], a['seg'], a['mask'], a['g_min'], a['shift'], a['sums'], a['maps'],
                               a['counted'], a['N'], a['H'], a['W'], None)


def test_the_symbols_exist_are_declared_and_the_abi_version_is_8():
    from dvd_hip import build, ops
    _l, lib = _lib()
    header = open(os.path.join(os.path.dirname(HERE), 'include', 'dvd_hip.h')).read()
    for name in ('dvd_ratio_median', 'dvd_depth_score'):
        assert name in _l.SIGNATURES and hasattr(lib, name) and ('int %s(const float* ' % name) in header
    assert '#define DVD_ABI_VERSION 8' in header and _l.ABI_VERSION == 8 and lib.dvd_abi_version() == 8
    assert ('#define DVD_RATIO_MEDIAN_WORKSPACE_PER_SEGMENT %d' % _l.RATIO_MEDIAN_WORKSPACE_PER_SEGMENT) in header
    assert ('select.hip', ['-ffp-contract=off']) in build.SOURCES and ('depth_score.hip', ['-ffp-contract=off']) in build.SOURCES
    assert {'ratio_hist_kernel', 'ratio_pick_kernel', 'depth_score_kernel'} <= set(ops.BYTE_CLASS_KERNELS['geometry'])


def test_ratio_median_refuses_bad_arguments_without_launching():
    _l, lib = _lib()
    nan = float('nan')
    odd = ctypes.c_void_p(66)
    bad = [dict(num=None), dict(den=None), dict(median=None), dict(count=None), dict(ws=None),
           dict(S=0), dict(S=-1), dict(S=65536, ws_bytes=1 << 40), dict(L=0), dict(L=-5),
           dict(S=1, L=1 << 31), dict(S=2, L=1 << 30), dict(S=3, L=(1 << 31) // 3 + 1), dict(S=65535, L=32769, ws_bytes=1 << 40),
           dict(den_min=nan), dict(num=odd), dict(den=odd), dict(median=odd), dict(count=ctypes.c_void_p(68)), dict(ws=odd),
           dict(ws_bytes=3 * 8224 - 1), dict(ws_bytes=0)]
    for over in bad:
        assert _median(lib, **over) == _l.DVD_EINVAL, over
        assert 'ratio_median' in _err(lib), over
    assert _median(lib, num=None) == _l.DVD_EINVAL and 'null' in _err(lib)
    assert _median(lib, S=2, L=1 << 30) == _l.DVD_EINVAL and '2^31' in _err(lib)
    assert _median(lib, num=odd) == _l.DVD_EINVAL and 'misaligned' in _err(lib)


def test_depth_score_refuses_bad_arguments_without_launching():
    from dvd_hip import ops
    _l, lib = _lib()
    nan = float('nan')
    odd = ctypes.c_void_p(66)
    bad = [dict(pred=None), dict(gt=None), dict(scale=None), dict(sums=None), dict(maps=None), dict(counted=None),
           dict(N=0), dict(N=65536), dict(H=0), dict(W=0), dict(H=32768, W=32768, shift=1),
           dict(g_min=-1.0), dict(g_min=nan), dict(g_min=float('inf')),
           dict(shift=0), dict(shift=33), dict(shift=-3),
           dict(N=80, H=384, W=672, shift=28), dict(N=5, H=1024, W=1024, shift=30),
           dict(pred=odd), dict(gt=odd), dict(scale=odd), dict(seg=odd), dict(maps=odd), dict(sums=ctypes.c_void_p(68))]
    for over in bad:
        assert _score(lib, **over) == _l.DVD_EINVAL, over
        assert 'depth_score' in _err(lib), over
    assert _score(lib, pred=None) == _l.DVD_EINVAL and 'null' in _err(lib)
    assert _score(lib, maps=None) == _l.DVD_EINVAL and 'both or none' in _err(lib)
    # the shift follows ops.eval_shift's rule on the pixels that can meet in one pooled sum, N * H * W; one more is refused
    for N, H, W in ((3, 11, 21), (80, 384, 672), (7, 1024, 1024), (1, 1, 1), (300, 2048, 2048)):
        shift = ops.eval_shift(N * H * W)
        assert shift == D.shift_for(N * H * W) and (N * H * W) * (1 << 10) * (1 << shift) <= 1 << 62
        if shift < 32:
            assert _score(lib, N=N, H=H, W=W, shift=shift + 1) == _l.DVD_EINVAL and 'shift' in _err(lib)
    assert ops.eval_shift(80 * 384 * 672) == 27


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from dvd_hip import ops, preprocess
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ops.ratio_median(torch.zeros(2, 8), torch.ones(2, 8))
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ops.depth_score(torch.ones(1, 1, 4, 4), torch.ones(1, 1, 4, 4), torch.ones(1))
    with pytest.raises(RuntimeError, match='GPU tensor'):
        preprocess.calibrate_scale(torch.ones(2, 4, 4), torch.ones(2, 4, 4))


@pytest.mark.parametrize('case', D.median_cases(), ids=lambda c: c[0])
def test_the_specs_median_is_numpys_and_equals_the_stated_rule(case):
    name, num, den, mask, den_min = case
    med, cnt = D.median(num, den, mask, den_min)
    assert med.dtype == np.float32 and cnt.dtype == np.int64
    rule = D.median_by_rule(num, den, mask, den_min)
    assert np.array_equal(med, rule, equal_nan=True), (name, med, rule)
    # ... and against numpy called here, on quotients formed here
    for s in range(num.shape[0]):
        sel = den[s] > np.float32(den_min)
        if mask is not None:
            sel &= mask[s] != 0
        with np.errstate(all='ignore'):
            q = num[s][sel] / den[s][sel]
        assert q.dtype == np.float32 and cnt[s] == q.size
        if q.size:
            with np.errstate(all='ignore'):
                m = np.median(q)
            assert m.dtype == np.float32 and np.array_equal(m, med[s], equal_nan=True)
        else:
            assert np.isnan(med[s])


def test_the_median_cases_hold_what_their_names_say():
    cases = {c[0]: c for c in D.median_cases()}
    med = {k: D.median(*c[1:])[0] for k, c in cases.items()}
    cnt = {k: D.median(*c[1:])[1] for k, c in cases.items()}
    assert np.isnan(med['empty_between'][1]) and cnt['empty_between'].tolist()[1] == 0 and np.isfinite(med['empty_between'][[0, 2]]).all()
    assert med['two_values_even_split'][0] == np.float32(np.float32(1.5 - 2.25) / 2)
    assert np.isnan(med['minus_inf_plus_inf'][:2]).all() and med['minus_inf_plus_inf'][2] == np.inf
    assert np.isnan(med['nan_selected'][1]) and np.isfinite(med['nan_selected'][[0, 2]]).all()
    assert np.isfinite(med['nan_masked_out']).all() and cnt['nan_masked_out'].tolist() == [300, 299, 300]
    assert cnt['den_equal_den_min'].max() <= 200 and cnt['nan_denominator'].tolist() == [299, 299]
    assert med['duplicated_middle/L1000'][0] == med['duplicated_middle/L1001'][0] == np.float32(0.7853982)
    assert cnt['equal_70000'].tolist() == [70000] and cnt['every_other'].tolist() == [500] * 3
    assert (np.abs(med['denormals/L257']) < np.finfo(np.float32).tiny).all()
    for kind, (S, L) in D.BEYOND_CAP.items():
        px = 1 if kind == 'scalar' else 4
        blocks = D.SELECT_MAX_BLOCKS // S
        assert (L % 4 == 0) == (px == 4) and -(-L // (256 * px)) > blocks          # the grid is capped
        second = L - blocks * 256 * px                                             # what the second trip walks
        assert (blocks - 1) * 256 * px < second < blocks * 256 * px                # every block has one; the last is ragged
        assert second - (blocks - 1) * 256 * px == px                              # ... and no shorter segment does


@pytest.mark.parametrize('shape', D.SCORE_SHAPES)
def test_fragile_share_of_the_score_cases_is_within_the_cap(shape):
    case = D.score_case(*shape)
    for seg in (case['seg'], None):
        for mask in (case['mask'], None):
            r64 = D.score(case['pred'], case['gt'], case['scale'], seg, mask)
            r32 = D.score(case['pred'], case['gt'], case['scale'], seg, mask, dtype=np.float32)
            share = D.fragile_share(r64)
            print('%dx%d seg=%s mask=%s: %.2f %% fragile, %.0f %% counted' % (shape + (seg is not None, mask is not None, 100 * share,
                                                                                      100 * r64['counted'].mean())))
            assert share <= D.FRAGILE_CAP
            solid = ~r64['fragile']
            # outside the fragile set fp32 and float64 agree about what counts and where: the yardstick of the GPU tests is defined
            assert not ((r64['region'] != r32['region']) & solid[:, None]).any()
            assert not ((r64['delta'] != r32['delta']) & solid[:, None]).any()
    if shape != (1, 1):
        full = D.score(case['pred'], case['gt'], case['scale'], case['seg'], case['mask'])
        # every branch is taken: holes, non-positive predictions, masked pixels, both regions, capped terms, all three deltas
        assert full['region'][:, 1].any() and full['region'][:, 2].any() and not full['counted'].all()
        assert (full['abs_rel'] == D.CAP).any() and (full['sq'] == D.CAP).any()
        assert 0 < full['delta'][:, 0].sum() < full['delta'][:, 1].sum() < full['delta'][:, 2].sum() < full['counted'].sum()
        assert ((case['pred'][:, 0] <= 0) & (case['gt'][:, 0] > D.G_MIN)).any()


def test_the_pipeline_inputs_have_a_fragile_share_within_the_cap():
    """The depth and ground truth Model.score_depth is tested on (tests/test_55_score_depth_gpu.py): the 7 frames of the track
    fixture, its input depth against the depth_mvs of the tree built from it, with the medians of the specification."""
    import eval_spec as E
    fx = helpers.load_golden(E.PIPE_FX)
    tree = E.pipeline_tree(fx)
    depth, gt = fx['in_depth'].astype(np.float32), tree['fr_depth_mvs'][:, None].astype(np.float32)
    N = depth.shape[0]
    keep = (gt > np.float32(D.G_MIN)).astype(np.uint8).reshape(N, -1)
    per_frame = D.median(gt.reshape(N, -1), depth.reshape(N, -1), keep)[0]
    video = D.median(gt.reshape(1, -1), depth.reshape(1, -1), keep.reshape(1, -1))[0]
    for scale in (np.ones(N, dtype=np.float32), per_frame, np.repeat(video, N)):
        r64 = D.score(depth, gt, scale)
        assert D.fragile_share(r64) <= D.FRAGILE_CAP and r64['counted'].any()


def test_scale_poses_is_the_references_three_statements():
    from dvd_hip import preprocess
    r = np.random.RandomState(5)
    for dtype in (np.float64, np.float32):
        poses = np.tile(np.eye(4), (6, 1, 1))
        for i in range(6):
            q, _ = np.linalg.qr(r.randn(3, 3))
            poses[i, :3, :3], poses[i, :3, 3] = q, r.randn(3) * 2.0
        poses = poses.astype(dtype)
        for s in (np.float32(1.8731), 0.41):
            want = []
            for i in range(6):
                T_G_1 = np.array(poses[i])
                T_G_1[:3, 3] *= s
                T_G_1 = np.linalg.inv(T_G_1)
                T_G_1 = T_G_1.astype(np.float32)
                want.append(T_G_1)
            keep = poses.copy()
            got = preprocess.scale_poses(poses, s)
            assert got.dtype == np.float32 and got.shape == (6, 4, 4) and np.array_equal(got, np.stack(want))
            assert np.array_equal(poses, keep)                                   # the caller's poses are not scaled in place
            assert np.array_equal(preprocess.scale_poses(torch.from_numpy(poses), s), got)
    with pytest.raises(RuntimeError, match='scale_poses'):
        preprocess.scale_poses(np.eye(4), 1.0)


def test_the_calibration_fixture_holds_what_the_generator_describes():
    fx = helpers.load_golden('scale_calib')
    nn, mvs, thresh = fx['in_nn_depth'], fx['in_mvs_depth'], float(fx['thresh'])
    assert nn.shape == mvs.shape == (5, 24, 40) and nn.dtype == mvs.dtype == np.float32 and thresh == 1e-3
    selected = (mvs > thresh).reshape(5, -1).sum(1)
    assert selected.tolist() == fx['selected'].tolist() and selected[0] % 2 == 0 and selected[1] % 2 == 1
    assert 0.2 < selected.sum() / mvs.size < 0.4
    # the specification gives the reference's recorded numbers, bit for bit
    med, cnt = D.median(nn.reshape(5, -1), mvs.reshape(5, -1), None, thresh)
    assert cnt.tolist() == selected.tolist() and np.array_equal(med, fx['scales']) and fx['scales'].dtype == np.float32
    assert fx['s'].dtype == np.float32 and np.mean(med) == fx['s']


@pytest.mark.skipif(not os.path.isdir(REF), reason='the reference tree is only present in the build container')
def test_the_calibration_fixture_regenerates_bit_identically(tmp_path):
    env = dict(os.environ, DVD_GOLDEN_OUT=str(tmp_path), OMP_NUM_THREADS='4')
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, 'make_scale_golden.py')], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    new = np.load(os.path.join(tmp_path, 'scale_calib.npz'), allow_pickle=False)
    old = np.load(os.path.join(GOLDEN, 'scale_calib.npz'), allow_pickle=False)
    assert sorted(new.files) == sorted(old.files)
    bad = [k for k in new.files
           if not (new[k].shape == old[k].shape and new[k].dtype == old[k].dtype and new[k].tobytes() == old[k].tobytes())]
    assert not bad, 'not bit-identical: %s' % bad
