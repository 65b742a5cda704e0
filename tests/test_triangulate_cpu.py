"""Host side of the triangulation feature (preprocess.triangulate_plan, ops.triangulate's refusals, the C ABI's declaration) and
the properties of its specification (tests/triangulate_spec.py) that the GPU tests rest on.  No device is needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import triangulate_spec as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the plan ---------------------------------------------------------------------------------------------------------------

def _pairs(N, gaps):
    return [(a, a + g) for g in gaps for a in range(N - g)]


def test_plan_orders_by_gap_forward_first_and_pads():
    from dvd_hip import preprocess
    pairs = _pairs(7, (1, 2, 3, 4))
    frames, obs = preprocess.triangulate_plan(pairs, 7)
    assert frames.dtype == np.int32 and frames.tolist() == list(range(7))
    assert obs.dtype == np.int32 and obs.shape == (7, 6, 3)
    at = {p: j for j, p in enumerate(pairs)}
    # frame 3 sees every gap in both directions: |gap| ascending, forward (dir 0) before backward (dir 1)
    assert obs[3].tolist() == [[at[(3, 4)], 4, 0], [at[(2, 3)], 2, 1], [at[(3, 5)], 5, 0], [at[(1, 3)], 1, 1],
                               [at[(3, 6)], 6, 0], [at[(0, 3)], 0, 1]]
    # the first frame has forward observations only, the last backward ones only; both are padded with -1
    assert obs[0].tolist() == [[at[(0, g)], g, 0] for g in (1, 2, 3, 4)] + [[-1] * 3] * 2
    assert obs[6].tolist() == [[at[(6 - g, 6)], 6 - g, 1] for g in (1, 2, 3, 4)] + [[-1] * 3] * 2
    assert np.array_equal(obs, T.plan(pairs, range(7)))
    # every live row names a pair that holds the frame, on the right side
    for f in range(7):
        for j, other, d in obs[f].tolist():
            if j >= 0:
                assert pairs[j] == ((f, other) if d == 0 else (other, f))


def test_plan_frames_gaps_and_a_frame_without_a_pair():
    from dvd_hip import preprocess
    pairs = _pairs(7, (1, 2, 3, 4))
    frames, obs = preprocess.triangulate_plan(pairs, 7, frames=[5, 2], gaps=[2, 4])
    assert frames.tolist() == [5, 2] and obs.shape == (2, 3, 3)
    at = {p: j for j, p in enumerate(pairs)}
    assert obs[0].tolist() == [[at[(3, 5)], 3, 1], [at[(1, 5)], 1, 1], [-1, -1, -1]]       # (5, 7) does not exist
    assert obs[1].tolist() == [[at[(2, 4)], 4, 0], [at[(0, 2)], 0, 1], [at[(2, 6)], 6, 0]]
    assert np.array_equal(obs, T.plan(pairs, [5, 2], gaps=(2, 4)))
    # the writer's default pair set leaves out the last pair of every gap: the last frame has no pair at all
    short = [(a, a + g) for g in (1, 2) for a in range(7 - 1 - g)]
    frames, obs = preprocess.triangulate_plan(short, 7)
    assert obs.shape == (7, 4, 3) and (obs[6] == -1).all() and (obs[5, 2:] == -1).all() and obs[5, :2].tolist() == [[4, 4, 1], [8, 3, 1]]
    frames, obs = preprocess.triangulate_plan(short, 7, frames=[6])
    assert obs.shape == (1, 0, 3)
    for kw in (dict(frames=[7]), dict(frames=[]), dict(frames=[-1]), dict(gaps=[0]), dict(gaps=[])):
        with pytest.raises(ValueError, match='triangulate_plan'):
            preprocess.triangulate_plan(pairs, 7, **kw)
    with pytest.raises(ValueError, match='triangulate_plan'):
        preprocess.triangulate_plan([(0, 9)], 7)


def test_plan_caps_a_frame_at_32_observations():
    from dvd_hip import preprocess
    gaps16 = tuple(range(1, 17))
    frames, obs = preprocess.triangulate_plan(_pairs(40, gaps16), 40)
    assert obs.shape == (40, 32, 3) and (obs[20, :, 0] >= 0).all()
    with pytest.raises(ValueError, match='frame 17 has 34 observations, at most 32'):
        preprocess.triangulate_plan(_pairs(40, tuple(range(1, 18))), 40)
    preprocess.triangulate_plan(_pairs(40, tuple(range(1, 18))), 40, gaps=gaps16)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------

def test_header_sources_and_binding_agree():
    from dvd_hip import _lib, build, ops
    src = open(os.path.join(ROOT, 'include', 'dvd_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'\bint\s+dvd_triangulate\s*\(([^)]*)\)\s*;', code)
    assert m, 'include/dvd_hip.h does not declare dvd_triangulate'
    want = []
    for prm in m.group(1).split(','):
        prm = ' '.join(prm.split())
        if '*' in prm or prm.startswith('dvd_stream_t'):
            want.append(ctypes.c_void_p)
        elif prm.startswith('long long'):
            want.append(ctypes.c_longlong)
        elif prm.startswith('float'):
            want.append(ctypes.c_float)
        else:
            assert prm.startswith('int '), prm
            want.append(ctypes.c_int)
    res, args = _lib.SIGNATURES['dvd_triangulate']
    assert res is ctypes.c_int and list(args) == want
    assert ('triangulate.hip', ['-ffp-contract=off']) in build.SOURCES
    assert _lib.ABI_VERSION == 8
    assert 'triangulate_kernel' in ops.BYTE_CLASS_KERNELS['geometry']
    assert ops.TRI_MAX_OBS == 32 and abs(ops.TRI_SIN2_MIN - np.sin(np.radians(0.5)) ** 2) < 1e-10 and ops.TRI_SIN2_MIN == T.SIN2_MIN
    # the entry refuses bad arguments before any HIP call
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    good = [p, p, p, p, 1, p, p, 1, p, p, p, p, 2, 1, 1.0, 1e-4, 1e-3, 2, p, p, p, p, p, 1, 1, 4, 4, None]
    for at, bad, word in ((23, 33, b'M=33'), (24, 65536, b'B=65536'), (13, 2, b'mode=2'), (15, 0.0, b'sin2_min'), (15, float('nan'), b'sin2_min'),
                          (14, float('inf'), b'epi_tol'), (16, -1.0, b'z_near'), (17, 0, b'min_count'), (18, None, b'null'),
                          (0, None, b'null'), (7, 2, b'live_rows'), (25, 1 << 15, b'images')):
        a = list(good)
        a[at] = bad
        if at == 25:
            a[26] = 1 << 15
        assert lib.dvd_triangulate(*a) == _lib.DVD_EINVAL, (at, bad)
        assert word in lib.dvd_last_error(), (word, lib.dvd_last_error())


# ---- the wrapper's refusals that need no device --------------------------------------------------------------------------

def test_wrapper_refuses_before_it_touches_a_device():
    from dvd_hip import ops
    f = torch.zeros(2, 4, 5, 2)
    m = torch.zeros(2, 4, 5, dtype=torch.uint8)
    tab = {'R': torch.eye(3).repeat(3, 1, 1), 't': torch.zeros(3, 3), 'K_T': torch.eye(3).repeat(3, 1, 1), 'K_inv_T': torch.eye(3).repeat(3, 1, 1)}
    obs = np.array([[[0, 1, 0], [-1, -1, -1]]], np.int32)
    call = lambda **kw: ops.triangulate(**dict(dict(flow_1_2=f, flow_2_1=f, mask_1=m, mask_2=m, obs=obs, frames=[0], tables=tab), **kw))
    for kw, word in ((dict(mode='max'), 'mode'), (dict(epi_tol=-1.0), 'epi_tol'), (dict(epi_tol=float('nan')), 'epi_tol'),
                     (dict(sin2_min=0.0), 'sin2_min'), (dict(sin2_min=1.5), 'sin2_min'), (dict(z_near=float('inf')), 'z_near'),
                     (dict(z_near='1'), 'z_near'), (dict(min_count=0), 'min_count'), (dict(min_count=2.5), 'min_count'),
                     (dict(min_count=True), 'min_count'), (dict(frames=[]), 'frames'), (dict(frames=[0.5]), 'frames'),
                     (dict(frames=[[0]]), 'frames'), (dict(obs=np.zeros((1, 33, 3), np.int32)), 'M=33'),
                     (dict(obs=np.zeros((2, 1, 3), np.int32)), 'obs'), (dict(obs=np.zeros((1, 1, 2), np.int32)), 'obs'),
                     (dict(obs=np.zeros((1, 1, 3), np.float32)), 'obs'), (dict(), 'flow_1_2 must be a GPU tensor'),
                     (dict(flow_1_2=f.double()), 'flow_1_2 must be a GPU tensor')):
        with pytest.raises(RuntimeError, match=word):
            call(**kw)


# ---- the specification ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def clean():
    sc = T.scene(24, 40, 7, seed=0, noise=0.0)
    obs = T.plan(sc['pairs'], range(7))
    out = T.pipeline(sc['flow_1_2'], sc['flow_2_1'], sc['mask_1'], sc['mask_2'], obs, range(7), sc['tables'], 'median', np.float64)
    return sc, obs, out


def test_scene_is_what_the_issue_describes(clean):
    sc, obs, _ = clean
    assert 2.0 < sc['depth'].min() and sc['depth'].max() < 5.0
    assert all(20 <= int(d.sum()) <= 400 for d in sc['disc'])            # the disc is in view in every frame
    assert sc['flow_1_2'].dtype == np.float32 and sc['flow_1_2'].shape == (18, 24, 40, 2) and sc['mask_1'].dtype == np.uint8
    assert 0.01 < sc['mask_1'].mean() < 0.5 and 0.01 < sc['mask_2'].mean() < 0.5
    assert obs.shape == (7, 6, 3)


def test_float64_spec_recovers_the_true_depth_on_static_pixels(clean):
    sc, _, out = clean
    static = ~sc['disc'] & (out['count'] >= 2)
    assert static.mean() > 0.6
    for mode in ('median', 'mean'):
        o = out if mode == 'median' else T.pipeline(sc['flow_1_2'], sc['flow_2_1'], sc['mask_1'], sc['mask_2'], T.plan(sc['pairs'], range(7)),
                                                    range(7), sc['tables'], mode, np.float64)
        worst = T.worst_rel(o['depth'][:, 0], sc['depth'], static)
        print('float64 spec against the true depth (%s): %.3g relative' % (mode, worst))
        assert worst <= 1e-5
    assert float(out['epi'][:, 0][static].max()) < 1e-3 and float(out['spread'][:, 0][static].max()) < 1e-5


def test_the_disc_has_no_consistent_observation_at_any_gap(clean):
    sc, obs, out = clean
    on = sc['disc']
    assert (out['count'][on] == 0).all()
    moving = (out['usable'] >= 2) & (out['count'] == 0)
    assert moving[on].mean() > 0.8 and not moving[~on].any()
    # ... and that holds gap by gap: the epipolar distance of every usable observation of a disc pixel is beyond the tolerance
    for f in range(7):
        for pair, other, d in obs[f].tolist():
            if pair < 0:
                continue
            o = T.observe((sc['flow_2_1'] if d else sc['flow_1_2'])[pair], (sc['mask_1'] if d else sc['mask_2'])[pair], sc['tables'], f, other,
                          np.float64)
            assert not o['consistent'][on[f]].any(), (f, other)
            if (o['usable'] & on[f]).any():
                assert float(o['e'][o['usable'] & on[f]].min()) > 2.0, (f, other)


def test_undecided_share_of_the_noisy_scene_is_within_the_cap():
    sc = T.scene(24, 40, 7, seed=0, noise=0.4)
    obs = T.plan(sc['pairs'], range(7))
    total = undecided = 0
    for f in range(7):
        for pair, other, d in obs[f].tolist():
            if pair < 0:
                continue
            o = T.observe((sc['flow_2_1'] if d else sc['flow_1_2'])[pair], (sc['mask_1'] if d else sc['mask_2'])[pair], sc['tables'], f, other,
                          np.float64)
            dec = T.decided(o, 24, 40)
            total += dec.size
            undecided += int((~dec).sum())
    print('undecided observations: %d of %d' % (undecided, total))
    assert total == 2 * 18 * 24 * 40
    assert undecided <= 0.01 * total


def test_fp32_contract_stays_finite_on_hostile_input():
    sc = T.scene(5, 7, 3, seed=1, noise=0.0, gaps=(1, 2))
    f12 = sc['flow_1_2'].copy()
    f12[0, 0, 0] = np.nan
    f12[0, 0, 1] = np.inf
    f12[0, 0, 2] = 1e30
    tab = {k: v.copy() for k, v in sc['tables'].items()}
    tab['t'][2] = tab['t'][0]                                              # zero baseline between frames 0 and 2
    tab['R'][2] = tab['R'][0]
    for mode in ('mean', 'median'):
        out = T.pipeline(f12, sc['flow_2_1'], sc['mask_1'] * 0, sc['mask_2'] * 0, T.plan(sc['pairs'], range(3)), range(3), tab, mode, np.float32)
        for k in ('depth', 'epi', 'spread'):
            assert np.isfinite(out[k]).all(), (mode, k)
