"""The temporal depth filter, the host side: the C entry in the header / the exports / the bindings / the build list, what the
library, ops.track_filter and filter_plan refuse before anything is launched, and the specification (tests/filter_spec.py) on
its own -- a static camera, an occluder, the median -- and on the exact inputs of the GPU end-to-end test
(tests/filter_cases.py), where the share of pixels with a sample whose gate hangs on the last bits must stay within 2 %."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import filter_cases as C
import filter_spec as F
import helpers
from dvd_hip.models.filter import filter_weights          # the weights of the specification tests are the feature's own

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_is_in_the_header_the_exports_the_bindings_and_the_build_list():
    from dvd_hip import _lib, build
    src = open(os.path.join(ROOT, 'include', 'dvd_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    lib = _lib.load()
    assert lib.dvd_abi_version() == _lib.ABI_VERSION == 8 and re.search(r'#define\s+DVD_ABI_VERSION\s+8\b', src)
    assert re.search(r'\bint\s+dvd_track_filter\s*\(', code)
    assert 'dvd_track_filter' in _lib.SIGNATURES and hasattr(ctypes.CDLL(lib._name), 'dvd_track_filter')
    res, args = _lib.SIGNATURES['dvd_track_filter']
    assert res is ctypes.c_int and len(args) == 22 and args[9] is ctypes.c_int and args[10] is args[11] is ctypes.c_float
    assert ('track_filter.hip', ['-ffp-contract=off']) in build.SOURCES
    assert os.path.exists(os.path.join(os.path.dirname(build.__file__), 'csrc', 'track_filter.hip'))


def _call(lib, **over):
    one = ctypes.c_void_p(16)                                        # never dereferenced: the checks come first
    a = dict(points=one, planar=1, start=one, R=one, t=one, K_T=one, depth_all=one, N=7, weights=one, mode=0, tol=0.1,
             z_near=1e-3, depth_out=one, ratio=None, count=None, spread=None, T1=7, B=3, H=11, W=21, k0=-3, stream=None)
    assert not set(over) - set(a)
    a.update(over)
    return lib.dvd_track_filter(*a.values())


def test_library_refuses_bad_arguments_before_any_hip_call():
    from dvd_hip import _lib
    lib = _lib.load()
    for name in ('points', 'start', 'R', 't', 'K_T', 'depth_all', 'weights', 'depth_out'):
        assert _call(lib, **{name: None}) == _lib.DVD_EINVAL, name
        assert b'null' in lib.dvd_last_error()
    for T1, k0 in [(0, 0), (34, -16), (-1, 0)]:
        assert _call(lib, T1=T1, k0=k0) == _lib.DVD_EINVAL
        assert b'33' in lib.dvd_last_error()
    for T1, k0 in [(7, 1), (7, -7), (1, -1), (33, -33)]:            # the start frame's row is outside the slab
        assert _call(lib, T1=T1, k0=k0) == _lib.DVD_EINVAL
        assert b'outside' in lib.dvd_last_error()
    for mode in (-1, 2):
        assert _call(lib, mode=mode) == _lib.DVD_EINVAL
        assert b'mode' in lib.dvd_last_error()
    for bad in (-0.1, float('nan'), float('inf')):
        assert _call(lib, tol=bad) == _lib.DVD_EINVAL
        assert b'tol' in lib.dvd_last_error()
        assert _call(lib, z_near=bad) == _lib.DVD_EINVAL
        assert b'z_near' in lib.dvd_last_error()
    for over in (dict(B=0), dict(B=65536), dict(N=0), dict(H=1), dict(W=1), dict(H=1 << 15, W=1 << 15)):     # track_shape_ok
        assert _call(lib, **over) == _lib.DVD_EINVAL, over


def test_ops_track_filter_checks_before_it_launches():
    from dvd_hip import ops
    tabs = {'R': torch.eye(3)[None], 't': torch.zeros(1, 3), 'K_T': torch.eye(3)[None]}
    p, d = torch.zeros(3, 1, 3, 4, 4), torch.ones(1, 1, 4, 4)
    good = dict(weights=[1.0, 1.0, 1.0], k0=-1)

    def call(match, **over):
        kw = dict(good)
        kw.update(over)
        with pytest.raises(RuntimeError, match=match):
            ops.track_filter(p, [0], tabs, d, **kw)

    call('GPU tensor')                                               # every host check passed: the CPU tensor is what is left
    call('k0', k0=-0.5)
    call('mode', mode='mode')
    call('mode', mode=0)
    for bad in (-1.0, float('nan'), float('inf'), None, True):
        call('tol', tol=bad)
        call('z_near', z_near=bad)
    call('want', want=('depth_at',))
    call('weights', weights='gauss')
    call('weights', weights=[[1.0, 1.0, 1.0]])
    call('weights', weights=[])
    call('weights', weights=[1.0] * 34, k0=-16)
    call('weights', weights=[1.0, float('nan'), 1.0], k0=0)
    call('weights', weights=[1.0, float('inf'), 1.0], k0=0)
    call('weights', weights=[1.0, -1.0, 1.0], k0=0)
    call('weights', weights=[1.0, 1e39, 1.0], k0=0)                  # not finite as fp32
    call('outside', k0=-3)
    call('outside', k0=1)
    call('must be > 0', weights=[1.0, 0.0, 1.0])


def test_filter_plan_counts_and_refusals():
    from dvd_hip.models.filter import MAX_RADIUS, filter_plan
    assert MAX_RADIUS == 16
    assert filter_plan(7, C.START, 3) == ([3, 3, 0], [1, 3, 3])
    assert filter_plan(7, [0, 6], 16, mode='median', weights='box', passes=3) == ([6, 0], [0, 6])
    assert filter_plan(7, torch.tensor([2]), np.int64(2), weights=[1, 2, 3, 2, 1]) == ([2], [2])
    for kw in (dict(radius=0), dict(radius=17), dict(radius=2.0), dict(radius=True), dict(mode='max'), dict(mode=None),
               dict(weights='triangle'), dict(passes=0), dict(passes=1.5), dict(passes=True), dict(frames=[]),
               dict(frames=[7]), dict(frames=[-1]), dict(frames=[1.5]), dict(n_frames=0)):
        a = dict(n_frames=7, frames=[1], radius=2)
        a.update(kw)
        with pytest.raises(ValueError, match='filter_plan'):
            filter_plan(**a)
    # the weights: gauss in float64 rounded once, sigma = radius / 2 by default
    w = filter_weights(4)
    j = np.arange(-4, 5, dtype=np.float64)
    assert w.dtype == np.float32 and np.array_equal(w, np.exp(-j * j / 8.0).astype(np.float32)) and w[4] == 1.0
    assert np.array_equal(filter_weights(2, 'gauss', sigma=0.5), np.exp(-np.arange(-2, 3.0) ** 2 / 0.5).astype(np.float32))
    assert np.array_equal(filter_weights(3, 'box'), np.ones(7, np.float32))
    assert np.array_equal(filter_weights(1, [0, 2, 0.5]), np.array([0, 2, 0.5], np.float32))
    for radius, weights, sigma in [(2, 'triangle', None), (2, [1, 1, 1], None), (1, [1, 0, 1], None), (1, [1, 1, -1], None),
                                   (1, [1, 1, float('nan')], None), (2, 'gauss', 0.0), (2, 'gauss', float('nan')),
                                   (2, 'gauss', -1.0)]:
        with pytest.raises(ValueError, match='filter_depth'):
            filter_weights(radius, weights, sigma)


# -- the specification on its own ------------------------------------------------------------------------------------------
def _static_rows(n, H, W):
    """A static camera and a zero field, analytically: every row of frame s is the frame's own pixels at depth S c_s, and the
    frame g they look into claims S c_g there.  The window spans the whole video (radius n - 1)."""
    _, S, c = C.static_video(n, H, W)
    radius = n - 1
    T1 = 2 * radius + 1
    g = np.arange(n)[None, :] + np.arange(T1)[:, None] - radius                       # [T1,B]: the frame row k of frame b sees
    exist = (g >= 0) & (g < n)
    z = np.broadcast_to((S[None, None] * c[None, :, None, None]), (T1, n, H, W)).copy()
    D = S[None, None] * np.where(exist, c[np.clip(g, 0, n - 1)], 0.0)[:, :, None, None]
    z[~exist] = 0.0
    inside = np.broadcast_to(exist[:, :, None, None], (T1, n, H, W)).copy()
    d0 = S[None] * c[:, None, None]
    return dict(z=z, depth_at=D, inside=inside, d0=d0, frames_exist=exist, weights=filter_weights(radius, 'box'), origin=radius), S, c, g


def test_static_camera_every_frame_becomes_the_mean():
    n, H, W = 7, 11, 21
    rows, S, c, _ = _static_rows(n, H, W)
    out = F.fuse(mode='mean', tol=0.1, z_near=1e-3, dtype=np.float64, **rows)
    want = S * c.mean()
    assert np.abs(out['depth'][:, 0] / want[None] - 1.0).max() <= 1e-12
    assert np.abs(out['ratio'][:, 0] * c[:, None, None] / c.mean() - 1.0).max() <= 1e-12
    assert np.all(out['count'] == n) and out['count'].dtype == np.uint8
    assert np.abs(out['spread'][:, 0] - ((c.max() - c.min()) / c)[:, None, None]).max() <= 1e-12
    # the fp32 form says the same within fp32 rounding of n terms
    o32 = F.fuse(mode='mean', tol=0.1, z_near=1e-3, dtype=np.float32, **rows)
    assert o32['depth'].dtype == np.float32 and np.abs(o32['depth'][:, 0] / want[None] - 1.0).max() <= 1e-6


def test_an_occluder_in_one_neighbour_is_gated_out():
    n, H, W = 7, 11, 21
    rows, S, c, g = _static_rows(n, H, W)
    base = F.fuse(mode='mean', dtype=np.float64, **rows)
    occ = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in rows.items()}
    hole = (slice(3, 7), slice(5, 12))
    sees4 = g == 4                                                   # [T1,B]: the samples that look into frame 4
    sees4[occ['origin']] = False                                     # (frame 4's own depth is not touched)
    for k, b in zip(*np.nonzero(sees4)):
        occ['depth_at'][(k, b) + hole] *= 0.5                        # a surface at half the depth in front of the point
    out = F.fuse(mode='mean', dtype=np.float64, **occ)
    # the other frames' result is the mean of the six frames that are left, inside the hole; unchanged outside it
    others = [b for b in range(n) if b != 4]
    want = S * np.delete(c, 4).mean()
    assert np.abs(out['depth'][others, 0][(slice(None),) + hole] / want[hole][None] - 1.0).max() <= 1e-12
    assert np.all(out['count'][others][(slice(None),) + hole] == n - 1)
    mask = np.ones((H, W), bool)
    mask[hole] = False
    assert np.array_equal(out['depth'][:, 0][:, mask], base['depth'][:, 0][:, mask]) and np.array_equal(out['depth'][4], base['depth'][4])
    # a gross disagreement the other way (the neighbour claims twice the depth) is gated too, so is a sample outside the
    # image, one nearer than z_near, and one from a frame that does not exist
    for change in ('far', 'outside', 'near', 'no_frame'):
        alt = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in rows.items()}
        k, b = alt['origin'] + 1, 2
        if change == 'far':
            alt['depth_at'][k, b] *= 2.0
        elif change == 'outside':
            alt['inside'][k, b] = False
        elif change == 'near':
            alt['z'][k, b], alt['depth_at'][k, b] = 5e-4, 5e-4
        else:
            alt['frames_exist'][k, b] = False
        o = F.fuse(mode='mean', dtype=np.float64, **alt)
        assert np.all(o['count'][b] == n - 1) and np.all(o['count'][[0, 1, 3, 4, 5, 6]] == n), change
        assert np.abs(o['depth'][b, 0] / (S * np.delete(c, 3).mean()) - 1.0).max() <= 1e-12, change


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_the_median_is_numpys_for_even_and_odd_counts(dtype):
    rng = np.random.RandomState(5)
    T1, B, H, W = 8, 2, 5, 6
    z = rng.uniform(1.0, 4.0, (T1, B, H, W))
    D = z * rng.uniform(0.85, 1.15, (T1, B, H, W))                   # about a third of the samples fail a gate
    inside = rng.uniform(size=(T1, B, H, W)) > 0.1
    d0 = rng.uniform(1.0, 4.0, (B, H, W))
    d0[0, 0, 0], d0[0, 0, 1] = 0.0, np.nan
    exist = np.ones((T1, B), bool)
    exist[0, 1] = False
    out = F.fuse(z, D, inside, d0, exist, np.ones(T1), 3, 'median', 0.1, 1e-3, dtype)
    counts, r = F.gates(z, D, inside, exist, 3, 0.1, 1e-3, dtype)
    seen = set()
    for b in range(B):
        for y in range(H):
            for x in range(W):
                if not d0[b, y, x] > 0:
                    assert out['count'][b, y, x] == 0 and out['ratio'][b, 0, y, x] == 1 and out['spread'][b, 0, y, x] == 0
                    assert np.array_equal(out['depth'][b, 0, y, x], dtype(d0[b, y, x]), equal_nan=True)
                    continue
                smp = r[counts[:, b, y, x], b, y, x]
                seen.add(len(smp) % 2)
                assert out['count'][b, y, x] == len(smp) >= 1
                assert out['ratio'][b, 0, y, x] == np.median(smp), (b, y, x)
                assert out['spread'][b, 0, y, x] == smp.max() - smp.min()
                assert out['depth'][b, 0, y, x] == dtype(d0[b, y, x]) * np.median(smp)
    assert seen == {0, 1} and out['ratio'].dtype == dtype


def _net(seed, time_dependent):
    from dvd_hip.networks.sceneflow_field import SceneFlowFieldNet
    return helpers.seeded_fill_(SceneFlowFieldNet(net_width=256, n_layers=4, time_dependent=time_dependent, N_freq_xyz=16,
                                                  N_freq_t=16), seed)


@pytest.mark.parametrize('time_dependent', [True, False])
@pytest.mark.parametrize('mode', ['mean', 'median'])
def test_undecided_share_on_the_inputs_of_the_gpu_end_to_end_test(time_dependent, mode):
    """The condition of tests/test_60_filter_depth_gpu.py's comparison: on its exact inputs the fp32 and the float64 form
    agree on the gate of every decided sample, and at most 2 % of the pixels have an undecided one."""
    fx = helpers.load_golden(C.FX)
    sd = _net(int(fx['seed']) + (0 if time_dependent else 1), time_dependent).state_dict()
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    depth, tabs = C.e2e_depth(fx), C.tables(fx)
    ts = C.time_stamps(fx, C.START, time_dependent)
    w = filter_weights(C.RADIUS)
    p64 = F.pipeline(sd, depth, tabs, ts, C.START, C.RADIUS, w, mode, C.TOL, C.Z_NEAR, dtype=np.float64)
    p32 = F.pipeline(sd, depth, tabs, ts, C.START, C.RADIUS, w, mode, C.TOL, C.Z_NEAR, dtype=np.float32)
    dec = p64['decided']
    assert np.array_equal(p32['counts'][dec], p64['counts'][dec])
    share = float((~dec.all(0)).mean())
    gated = 1.0 - p64['counts'][p64['rows']['live'].numpy()].mean()
    print('undecided share %.4f, %.1f %% of the samples with a frame gated out' % (share, 100 * gated))
    assert share <= 0.02
    assert 0.02 < gated < 0.9                                        # the gates do drop samples, and do let samples through
    # where every sample is decided the two forms agree to fp32 rounding
    ok = dec.all(0)
    assert np.abs(p32['ratio'][:, 0][ok].astype(np.float64) - p64['ratio'][:, 0][ok]).max() < 1e-4
