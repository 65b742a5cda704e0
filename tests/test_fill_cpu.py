"""Host side of push-pull hole filling (the C ABI's declaration and refusals, ops.fill_holes' refusals) and the properties of its
specification (tests/fill_spec.py) that the GPU tests rest on.  No device is needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import fill_spec as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the specification on the case table --------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def runs():
    """Every case of the table with C = 4 and a depth-like bias squared, in float64: computed once, shared, never written to."""
    out = {}
    for name in F.CASES:
        case = F.make(name)
        out[name] = (case, F.fill(case['values'], case['known'], case['bias'], 2, case['fill']))
    return out


def _known(case, power=2):
    return np.stack([F.weights(case['known'][i], case['bias'][i, 0], power, np.float64) > 0 for i in range(len(case['known']))])


def test_the_table_holds_what_the_tests_need():
    shapes = {(H, W) for H, W, _, _ in F.CASES.values()}
    assert {(2, 2), (1, 7), (11, 21), (33, 65), (70, 45), (97, 130)} <= shapes
    assert any(W % 4 == 0 and H > 32 for H, W in shapes) and any(V == 3 for _, _, V, _ in F.CASES.values())
    for name in F.CASES:
        case = F.make(name)
        again = F.make(name)
        assert all(np.array_equal(case[k], again[k], equal_nan=True) for k in ('values', 'known', 'bias')), name
        assert case['values'].dtype == case['bias'].dtype == np.float32 and case['known'].dtype == np.uint8
        empty = ~_known(case).any(axis=(1, 2))
        assert empty.tolist() == ([False, True, False] if name == 'one_empty' else [False] * len(empty)), name
        if name not in ('all_known', '2x2', '1x7'):
            assert np.isnan(case['values']).any(), name             # an unknown pixel may hold anything
    hole = F.make('97x130')
    assert not hole['known'][0, 20:70, 45:85].any() and 0.01 < hole['known'].mean() < 0.03
    bad = F.make('bad_bias')
    b = bad['bias'][:, 0][bad['known'] != 0]
    assert (b == 0).any() and (b < 0).any() and np.isinf(b).any() and np.isnan(b).any()
    assert int((bad['known'] != 0).sum()) - int(_known(bad).sum()) == 8


def test_known_pixels_are_unchanged_and_level_is_zero_exactly_there(runs):
    for name, (case, out) in runs.items():
        k = _known(case)
        kc = np.broadcast_to(k[:, None], case['values'].shape)
        assert np.array_equal(out['values'][kc], case['values'][kc].astype(np.float64)), name
        assert np.array_equal(out['level'] == 0, k), name
        assert np.isfinite(out['values']).all(), name
        r32 = F.fill(case['values'], case['known'], case['bias'], 2, case['fill'], dtype=np.float32)
        assert r32['values'].dtype == np.float32 and np.array_equal(r32['values'][kc].view(np.int32), case['values'][kc].view(np.int32))
        assert np.array_equal(r32['level'], out['level']), name


def test_filled_values_lie_within_the_range_of_the_views_known_values(runs):
    for name, (case, out) in runs.items():
        k = _known(case)
        for v in range(len(k)):
            if not k[v].any():
                continue
            for c in range(case['values'].shape[1]):
                lo, hi = case['values'][v, c][k[v]].min(), case['values'][v, c][k[v]].max()
                got = out['values'][v, c]
                # a weighted mean in floating point may leave the range of its terms by a rounding: values are in [0, 1]
                assert got.min() >= lo - 1e-12 and got.max() <= hi + 1e-12, (name, v, c)


def test_a_constant_image_stays_constant():
    for name in ('11x21', '33x65', '97x130'):
        case = F.make(name)
        const = np.full_like(case['values'], 0.375)                  # dyadic: with equal weights every sum is exact
        for dtype in (np.float64, np.float32):
            out = F.fill(const, case['known'], None, 0, 0.0, dtype=dtype)
            assert (out['values'] == 0.375).all(), (name, dtype)
        out = F.fill(const, case['known'], case['bias'], 2, 0.0)
        assert np.abs(out['values'] - 0.375).max() < 1e-14, name


def test_an_all_unknown_view_gives_fill_and_255(runs):
    case, out = runs['one_empty']
    assert (out['values'][1] == case['fill']).all() and (out['level'][1] == F.EMPTY).all()
    assert (out['level'][[0, 2]] != F.EMPTY).all() and (out['values'][[0, 2]] != case['fill']).all()
    # a view's result does not depend on its neighbours
    alone = F.fill(case['values'][2:], case['known'][2:], case['bias'][2:], 2, case['fill'])
    assert np.array_equal(alone['values'][0], out['values'][2]) and np.array_equal(alone['level'][0], out['level'][2])


def test_level_measures_the_distance_to_the_nearest_data(runs):
    case, out = runs['corner']
    H, W = case['known'].shape[1:]
    y, x = np.mgrid[0:H, 0:W]
    want = np.zeros((H, W), np.int32)
    for k in range(1, 8):
        want[(want == 0) & ((y >> k) == ((H - 1) >> k)) & ((x >> k) == ((W - 1) >> k))] = k
    want[H - 1, W - 1] = 0
    assert np.array_equal(out['level'][0], want) and out['level'].max() == 6
    # one known pixel: every pixel is that pixel's value, up to the roundings of the interpolation
    v = case['values'][0, :, H - 1, W - 1].astype(np.float64)
    assert np.abs(out['values'][0] - v[:, None, None]).max() < 1e-14
    assert runs['97x130'][1]['level'].max() >= 6 and runs['97x130'][1]['level'][0, 45, 65] >= 5


def test_the_weight_decides_what_a_coarse_pixel_holds():
    """Two known pixels of a 2 x 2 image, one near (bias 1) and one far (bias 9): the two unknown ones take the weighted mean."""
    values = np.array([[[[1.0, 0.0], [0.0, 5.0]]]], np.float32)
    known = np.array([[[1, 0], [0, 1]]], np.uint8)
    bias = np.array([[[[1.0, 3.0], [3.0, 9.0]]]], np.float32)
    for power, mean in ((0, 3.0), (1, (1 + 45) / 10.0), (2, (1 + 405) / 82.0)):
        out = F.fill(values, known, bias, power, 0.0)
        assert np.allclose(out['values'][0, 0], [[1.0, mean], [mean, 5.0]], rtol=0, atol=1e-14), power
        assert out['level'].tolist() == [[[0, 1], [1, 0]]]


# ---- the C ABI --------------------------------------------------------------------------------------------------------------

def _declared(code, name):
    m = re.search(r'\b(\w+)\s+%s\s*\(([^)]*)\)\s*;' % name, code)
    assert m, 'include/dvd_hip.h does not declare %s' % name
    want = []
    for prm in m.group(2).split(','):
        prm = ' '.join(prm.split())
        if '*' in prm or prm.startswith('dvd_stream_t'):
            want.append(ctypes.c_void_p)
        elif prm.startswith('float'):
            want.append(ctypes.c_float)
        else:
            assert prm.startswith('int '), prm
            want.append(ctypes.c_int)
    return m.group(1), want


def _workspace_bytes(V, C, H, W):
    n = 0
    for _ in range(5):
        H, W = (H + 1) // 2, (W + 1) // 2
        n += H * W
    return 4 * V * (C + 1) * n


def test_header_sources_and_binding_agree():
    from dvd_hip import _lib, build, ops
    src = open(os.path.join(ROOT, 'include', 'dvd_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    res, want = _declared(code, 'dvd_fill_holes')
    assert res == 'int' and _lib.SIGNATURES['dvd_fill_holes'] == (ctypes.c_int, want)
    res, want = _declared(code, 'dvd_fill_workspace_bytes')
    assert res == 'size_t' and _lib.SIGNATURES['dvd_fill_workspace_bytes'] == (ctypes.c_size_t, want)
    assert ('fill.hip', ['-ffp-contract=off']) in build.SOURCES
    assert _lib.ABI_VERSION == 8
    lib = _lib.load()                                      # (it fails for a symbol the library does not export)
    assert lib.dvd_abi_version() == 8
    for k in ('fill_pull_kernel', 'fill_mid_kernel', 'fill_push_kernel'):
        assert k in ops.BYTE_CLASS_KERNELS['geometry']
    assert (ops.FILL_MAX_C, ops.FILL_MAX_TILES, ops.FILL_EMPTY) == (8, 2048, F.EMPTY)


def test_workspace_bytes_is_the_sum_of_the_level_sizes():
    from dvd_hip import _lib
    lib = _lib.load()
    for V, C, H, W in ((1, 1, 1, 1), (1, 4, 2, 2), (3, 8, 11, 21), (2, 4, 33, 65), (1, 1, 97, 130), (16, 4, 384, 672), (1, 4, 768, 1344),
                       (1, 8, 1024, 2048), (1, 1, 1, 65536), (65535, 1, 1, 1)):
        assert lib.dvd_fill_workspace_bytes(V, C, H, W) == _workspace_bytes(V, C, H, W), (V, C, H, W)
    # refused: no views, too many, no or too many channels, no pixels, more than 2048 tiles of 32 x 32
    for V, C, H, W in ((0, 4, 8, 8), (65536, 4, 8, 8), (-1, 4, 8, 8), (1, 0, 8, 8), (1, 9, 8, 8), (1, 4, 0, 8), (1, 4, 8, 0),
                       (1, 4, 1024, 2049), (1, 1, 1, 65537), (1, 1, 1 << 15, 1 << 15)):
        assert lib.dvd_fill_workspace_bytes(V, C, H, W) == 0, (V, C, H, W)


def test_the_entry_refuses_bad_arguments_before_any_hip_call():
    from dvd_hip import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    good = [p, p, p, 2, 0.0, 1, 4, 8, 8, p, p, p, None]
    for at, bad, word in ((0, None, b'null'), (1, None, b'null'), (9, None, b'null'), (10, None, b'null'), (11, None, b'null'),
                          (3, 5, b'power=5'), (3, -1, b'power=-1'), (5, 0, b'V=0'), (5, 65536, b'V=65536'), (6, 0, b'C=0'),
                          (6, 9, b'C=9'), (7, 0, b'images'), (8, 1 << 30, b'images'), (8, 32 * 2048 + 1, b'tiles'),
                          (0, ctypes.c_void_p(18), b'aligned'), (2, ctypes.c_void_p(17), b'aligned')):
        a = list(good)
        a[at] = bad
        assert lib.dvd_fill_holes(*a) == _lib.DVD_EINVAL, (at, bad)
        assert word in lib.dvd_last_error(), (word, lib.dvd_last_error())


# ---- the wrappers' refusals that need no device ---------------------------------------------------------------------------

def test_wrapper_refuses_before_it_touches_a_device():
    from dvd_hip import ops
    with pytest.raises(RuntimeError, match='values must be a GPU tensor'):
        ops.fill_holes(torch.zeros(1, 3, 4, 5), torch.ones(1, 4, 5, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='values must be a GPU tensor'):
        ops.fill_holes(np.zeros((1, 3, 4, 5), np.float32), torch.ones(1, 4, 5, dtype=torch.uint8))


def test_render_and_triangulate_depth_validate_the_new_arguments_on_the_host():
    import inspect
    from dvd_hip import preprocess
    from dvd_hip.models import render
    from dvd_hip.models.scene_flow_motion_field import Model
    for fn in (render.render, Model.render):
        sig = inspect.signature(fn).parameters
        assert sig['inpaint'].default is False and sig['bg_power'].default == 2
    assert inspect.signature(preprocess.triangulate_depth).parameters['densify'].default is False
    model = type('M', (), {'opt': type('O', (), {'use_cnn': False})()})()
    for kw in (dict(inpaint=1), dict(inpaint='yes'), dict(inpaint=None), dict(bg_power=5), dict(bg_power=-1), dict(bg_power=2.0),
               dict(bg_power=True), dict(bg_power=None)):
        with pytest.raises(ValueError, match='inpaint|bg_power'):
            render.render(model, None, [0], [[0]], **kw)
    with pytest.raises(ValueError, match='densify'):
        preprocess.triangulate_depth(None, densify=1)
