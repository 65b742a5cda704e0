"""The float64 specification, the exact data and the case table of tests/test_69_xconv_classes_gpu.py (tests/xconv_spec.py),
checked without a GPU:

  1. spec() equals F.conv2d / F.conv_transpose2d plus the unfused ATen ops (F.batch_norm, relu, add, mask) in float64 for
     every flag, packing and BatchNorm variant, on real-valued data -- a second, independent way to the same operator;
  2. the premises of "the kernel's arithmetic is exact" hold for every case of the table: the K sums stay below 2^24 quanta,
     every scaled operand is one fp16 term with a zero low term (pow2_scale and split_pair_f16 of csrc/dvd_split.h emulated in
     numpy), every result is an fp32 number (below 2^15 for fp16 outputs), the BatchNorm pair is exact in fp32;
  3. the table reaches every class of xconv_spec.REQUIRED, as dvd_xconv_describe (pure host code) reports the launches;
  4. dvd_xconv_describe answers what csrc/xconv_tile.h gives for the table's first rows (PINNED, computed with a host program
     that includes the header), honours dvd_xconv_select and refuses what the launch refuses."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import xconv_spec as X


@pytest.fixture(scope='module')
def lib():
    from dvd_hip import _lib
    return _lib.load()


# ---- 1 ------------------------------------------------------------------------------------------------------------------
def _unfused(case, d, epi):
    """The same function from the ATen operators, no autograd: conv_transpose2d is the backward-data operator."""
    _, Cin, Cout, H, W, k, G, mode, N = case
    kw = X.spec_args(case, d, epi)
    x, w = kw['x'].double(), kw['w'].double()
    if 'scaled' in kw:
        g, var, eps = kw['scaled']
        w = w * (g.double() / torch.sqrt(var.double() + eps))[:, None, None, None]
    fl = kw['flags']
    if fl & X.RELU_IN:
        x = torch.relu(x)
    if mode == 'zi':
        Hq, Wq = x.shape[2:]
        y = F.conv_transpose2d(x, w, None, stride=2, padding=1, output_padding=(H - (2 * Hq - 1), W - (2 * Wq - 1)), groups=G)
    elif kw['transposed']:
        y = F.conv_transpose2d(x, w, None, stride=1, padding=k // 2, groups=G)
    else:
        y = F.conv2d(x, w, None, stride=2 if mode == 's2' else 1, padding=k // 2, groups=G)
    if kw.get('bias') is not None:
        y = y + kw['bias'].double()[None, :, None, None]
    if kw.get('bn') is not None:
        g, b, m, v, eps = kw['bn']
        y = F.batch_norm(y, m.double(), v.double(), None if g is None else g.double(), None if b is None else b.double(), False, 0.0, eps)
    if kw.get('residual') is not None:
        r = kw['residual'].double()
        y = y + (torch.relu(r) if fl & X.RES_RELU else r)
    if kw.get('mask_src') is not None:
        y = torch.where(kw['mask_src'] > 0, y, torch.zeros_like(y))
    return torch.relu(y) if fl & X.RELU_OUT else y


SPEC_CASES = ['k3 32-40 9x13', 'k1 32-72 8x18', 'k5 16-24 9x12', 'k3 g3 72-120 9x13', 'k3 g2 64-64 9x23', 's2 16-32 10x14',
              's2 32-64 11x15', 's2 g2 64-64 10x14', 'zi 16-32 10x14', 'zi 32-64 11x15', 'zi g2 64-64 11x14', 'zi 16-32 1x40',
              's2 16-32 40x1']


@pytest.mark.parametrize('name', SPEC_CASES)
def test_spec_equals_the_unfused_operators(name):
    case = X.CASE[name]
    d = X.real_data(case)
    for epi in X.EPILOGUES:
        kw = X.spec_args(case, d, epi)
        v, y, amax = X.spec(**kw)
        want = _unfused(case, d, epi)
        assert v.shape == want.shape == X.shapes_of(case)[1]
        err = float((v - want).abs().max())
        assert err <= 1e-12 * max(1.0, float(want.abs().max())), '%s, %s: %.3e' % (name, epi[0], err)
        assert amax == float(want.abs().max()) or abs(amax - float(want.abs().max())) < 1e-12
        assert y.dtype == torch.float32 and torch.equal(y, v.float())
        p = X.parts(**kw)
        # the terms the real-valued bound of the GPU test is built from add up to v (before mask and output ReLU)
        if kw.get('mask_src') is None and not kw['flags'] & X.RELU_OUT:
            assert float((p['z'] * p['s'][None, :, None, None] + p['shift'][None, :, None, None] + p['res'] - v).abs().max()) < 1e-9


# ---- 2 ------------------------------------------------------------------------------------------------------------------
def _pow2_scale(amax):
    """csrc/dvd_split.h: pow2_scale."""
    a = np.float32(amax)
    u = int(a.view(np.uint32))
    e = (u >> 23) & 0xff
    if not a > 0 or e == 0xff:
        return np.float32(1.0)
    se = min(max(267 - e, 1), 254)
    return np.uint32(se << 23).view(np.float32)


def _one_term(t, s):
    """split_pair_f16 of t * s: -> True when h carries everything (finite h, low term identically zero)."""
    xs = (t.numpy().astype(np.float32) * np.float32(s)).astype(np.float32)
    h = xs.astype(np.float16)
    low = (xs - h.astype(np.float32)).astype(np.float16)
    return bool(np.isfinite(h).all()) and not low.any()


@pytest.mark.parametrize('case', X.CASES, ids=[c[0] for c in X.CASES])
def test_exactness_premises(case):
    d = X.exact_data(case)
    name, Cin, Cout, H, W, k, G, mode, N = case
    for t in ('x', 'residual', 'mask'):
        assert d[t].abs().max() <= 4 and torch.equal(d[t], d[t].round()) and torch.equal(d[t].half().float(), d[t])
    assert float(d['x'].abs().max()) == 4.0                                   # the true maximum the tests pass (and twice it)
    assert (d['mask'] == 0).any() and (d['mask'] < 0).any() and (d['mask'] > 0).any()
    # activations: one fp16 term under the scale of the true maximum and of twice the maximum
    for amax in (4.0, 8.0):
        assert _one_term(d['x'], _pow2_scale(amax)) and _one_term(d['x'].clamp_min(0), _pow2_scale(amax))
    # BatchNorm pair, computed as the kernel does in fp32, equals the float64 pair
    for bn in (d['bn'], d['bn_plain']):
        g, b, m, v, eps = bn
        assert eps == 0.0
        sc32 = (g if g is not None else torch.ones_like(v)) / torch.sqrt(v + torch.tensor(eps))
        sh32 = (b if b is not None else torch.zeros_like(v)) - m * sc32
        s64, h64 = X.bn_pair(bn, Cout)
        assert sc32.dtype == torch.float32 and torch.equal(sc32.double(), s64) and torch.equal(sh32.double(), h64)
    for epi in X.EPILOGUES:
        kw = X.spec_args(case, d, epi)
        # the packed weights as xconv_weight makes them (fp32), their scale from the true maximum
        w = kw['w']
        quantum = 1.0
        if 'scaled' in kw:
            g, var, eps = kw['scaled']
            sc = g / torch.sqrt(var + torch.tensor(eps))
            assert torch.equal(sc.double(), g.double() / torch.sqrt(var.double()))
            w = w * sc[:, None, None, None]
            quantum = 0.125                                                 # |gamma| >= 1/2, sqrt(var) <= 4
            assert torch.equal((w / quantum).round() * quantum, w)
        assert _one_term(w, _pow2_scale(float(w.abs().max()))), '%s: weights are not one fp16 term' % epi[0]
        # K sums: every partial sum, in any order, is an integer number of quanta below 2^24
        kabs = dict(kw, x=kw['x'].abs(), w=kw['w'].abs(), flags=kw['flags'] & (X.S2 | X.ZI), bias=None, residual=None, mask_src=None,
                    bn=None)
        if 'scaled' in kw:
            kabs['scaled'] = (kw['scaled'][0].abs(), kw['scaled'][1], kw['scaled'][2])
        ksum = float(X.parts(**kabs)['v'].max())
        assert 0 < ksum / quantum < 2 ** 24, '%s: K sum %g' % (epi[0], ksum)
        v, y, amax = X.spec(**kw)
        assert torch.equal(v.float().double(), v), '%s: a result is no fp32 number' % epi[0]
        assert amax == float(np.float32(amax)) and amax > 0
        if X.H16 in X.storages_of(case):
            assert float(v.abs().max()) < 2 ** 15, '%s: fp16 output overflows' % epi[0]
            assert torch.isfinite(v.half()).all()


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def _descriptions(lib):
    out = []
    for case in X.CASES:
        for st in X.storages_of(case):
            status, d = X.describe(lib, case, st)
            assert status == 0, '%s %s: %s' % (case[0], st, lib.dvd_last_error())
            out.append((case[0], d))
    return out


def test_the_table_reaches_every_class(lib):
    assert lib.dvd_xconv_select(0) == 0
    ds = _descriptions(lib)
    missing = [name for name, want in X.REQUIRED if not any(X.matches(d, want) for _, d in ds)]
    assert not missing, 'no case of xconv_spec.CASES reaches: %s' % '; '.join(missing)
    # groups: 2 groups at 32 and at 64 channels per group, 3 groups at 24 -> 40 on the generic loop with a ragged block per group
    by = dict(((n, d['storage']), d) for n, d in ds)
    assert by[('k3 g2 64-64 9x23', X.F32)]['cfg'] == (1, 2, 1, 4) and by[('k3 g2 128-128 7x10', X.F32)]['cfg'] == (2, 2, 1, 4)
    g3 = by[('k3 g3 72-120 9x13', X.F32)]
    assert not g3['fast'] and g3['ragged_block'] and X.storages_of(X.CASE['k3 g3 72-120 9x13']) == (X.F32,)
    # every misaligned-operand case is a wide-epilogue case that falls back to the narrow epilogue of the same kernel
    for name in X.WIDE_MISALIGNED:
        for st in X.STORAGES:
            a, b = X.describe(lib, X.CASE[name], st, True)[1], X.describe(lib, X.CASE[name], st, False)[1]
            assert a['wide'] == 1 and b['wide'] == 0 and b['fit'] == X.FIT_ONE
            assert {k: v for k, v in a.items() if k != 'wide'} == {k: v for k, v in b.items() if k != 'wide'}


# ---- 4 ------------------------------------------------------------------------------------------------------------------
# case -> (cfg, b1 (fp32), fit, items per thread, TR, TC, P, PQ, ntr * ntc, mblocks, wide), from csrc/xconv_tile.h under select 0
PINNED = {
    'k1 16-24 5x7': ((1, 2, 1, 4), 0, 1, 1, 1, 40, 40, 40, 1, 1, 0),
    'k1 32-40 6x12': ((2, 2, 1, 4), 0, 1, 1, 1, 72, 72, 72, 1, 1, 0),
    'k1 32-72 8x18': ((2, 2, 2, 2), 0, 1, 1, 1, 72, 72, 72, 2, 1, 0),
    'k1 32-288 8x18': ((4, 2, 2, 2), 0, 11, 1, 1, 72, 72, 72, 2, 2, 1),
    'k1 32-288 7x19': ((4, 2, 2, 2), 0, 11, 1, 1, 72, 72, 72, 2, 2, 0),
    'k1 32-256 12x20': ((4, 2, 2, 2), 0, 11, 1, 1, 120, 120, 120, 2, 1, 1),
    'k3 16-24 5x7': ((1, 2, 1, 4), 0, 1, 1, 5, 7, 9, 7, 1, 1, 0),
    'k3 32-40 9x13': ((2, 2, 1, 4), 0, 2, 2, 9, 13, 15, 13, 1, 1, 0),
    'k3 32-72 9x13': ((2, 2, 2, 2), 0, 2, 2, 9, 13, 15, 13, 1, 1, 0),
    'k3 32-288 9x14': ((4, 2, 2, 4), 0, 1, 1, 9, 14, 16, 14, 1, 2, 0),
    'k3 16-256 13x23': ((4, 2, 2, 4), 0, 1, 1, 13, 12, 14, 12, 2, 1, 0),
    'k5 16-24 9x12': ((1, 2, 1, 4), 0, 2, 2, 9, 12, 16, 12, 1, 1, 0),
    'k5 16-64 12x20': ((2, 2, 1, 4), 0, 3, 3, 12, 20, 24, 20, 1, 1, 0),
    'k7 16-32 9x12': ((1, 2, 1, 4), 0, 3, 3, 9, 12, 18, 12, 1, 1, 0),
    'k7 16-72 10x13': ((2, 2, 2, 2), 0, 2, 2, 10, 7, 13, 7, 2, 1, 0),
    'k11 16-32 9x12': ((1, 2, 1, 4), 0, 0, 4, 9, 12, 22, 12, 1, 1, 0),
    'k11 16-256 9x12': ((4, 2, 2, 4), 0, 2, 2, 9, 12, 22, 12, 1, 1, 0),
    's2 16-32 10x14': ((1, 2, 1, 4), 1, 2, 2, 5, 7, 8, 7, 1, 1, 0),
    's2 32-64 11x15': ((2, 2, 1, 4), 1, 2, 2, 6, 8, 9, 8, 1, 1, 0),
    's2 32-128 11x15': ((2, 2, 2, 2), 1, 2, 2, 6, 8, 9, 8, 1, 1, 0),
    's2 16-256 9x13': ((2, 2, 2, 2), 1, 2, 2, 5, 7, 8, 7, 1, 2, 0),
    's2 32-64 41x59': ((2, 2, 1, 4), 1, 0, 8, 7, 30, 31, 30, 3, 1, 0),
    'k3 3-24 7x9': ((1, 2, 1, 4), 0, 1, 1, 7, 9, 11, 9, 1, 1, 0),
    'k3 20-40 11x19': ((2, 2, 1, 4), 0, 3, 3, 11, 19, 21, 19, 1, 1, 0),
    'k3 12-72 9x13': ((2, 2, 2, 2), 0, 2, 2, 9, 13, 15, 13, 1, 1, 0),
    'k3 20-288 9x13': ((2, 2, 2, 2), 0, 2, 2, 9, 13, 15, 13, 1, 3, 0),
    'k1 5-1 17x29': ((1, 2, 1, 4), 0, 2, 2, 1, 248, 248, 248, 2, 1, 0),
    'k7 3-64 16x24': ((2, 2, 1, 4), 0, 0, 4, 16, 12, 18, 12, 2, 1, 0),
}


def test_describe_agrees_with_the_tile_header(lib):
    assert lib.dvd_xconv_select(0) == 0
    assert list(PINNED) == [c[0] for c in X.CASES[:28]]
    for name, (cfg, b1, fit, items, TR, TC, P, PQ, tiles, mblocks, wide) in PINNED.items():
        case = X.CASE[name]
        for st in X.storages_of(case):
            status, d = X.describe(lib, case, st)
            assert status == 0, name
            got = (d['cfg'], d['b1'], d['fit'], d['items'], d['TR'], d['TC'], d['P'], d['PQ'], d['ntr'] * d['ntc'], d['mblocks'], d['wide'])
            assert got == (cfg, b1 if st == X.F32 else 0, fit, items, TR, TC, P, PQ, tiles, mblocks, wide), '%s %s' % (name, st)
            assert d['threads'] == 64 * cfg[2] * cfg[3] and d['fast'] == int((case[1] // case[6]) % 16 == 0)
            assert (d['in16'], d['out16']) == (int(st != X.F32), int(st == X.H16))
            assert (d['s2'], d['zi']) == (int(case[7] == 's2'), int(case[7] == 'zi')) and 0 < d['lds'] <= 160 * 1024


def test_describe_honours_the_select_hook(lib):
    wide = X.CASE['k1 32-288 8x18']
    try:
        for sel, want in ((0, dict(fit=11, wide=1)), (6, dict(fit=1, wide=0)), (7, dict(fit=11, wide=0)), (1, dict(cfg=(2, 2, 2, 2), wide=0)),
                          (4, dict(fast=0, cfg=(2, 2, 2, 2)))):
            assert lib.dvd_xconv_select(sel) == 0
            status, d = X.describe(lib, wide, X.F32)
            assert status == 0 and X.matches(d, want), (sel, d)
        assert lib.dvd_xconv_select(8) == 0
        d8 = X.describe(lib, X.CASE['k3 32-40 9x13'], X.F32)[1]
        assert d8['PQ'] == d8['P']                                    # haloed positions
    finally:
        assert lib.dvd_xconv_select(0) == 0
    assert X.describe(lib, X.CASE['k3 32-40 9x13'], X.F32)[1]['PQ'] == 13


def test_describe_refuses_what_the_launch_refuses(lib):
    from dvd_hip import _lib
    out = (ctypes.c_int * 24)()
    p = ctypes.cast(out, ctypes.c_void_p)
    bad = [((16, 32, 8, 8, 3, 1, 0, 0, 1, 1), b'fp32 input with fp16 output'),
           ((20, 32, 8, 8, 3, 1, 0, 1, 1, 1), b'fp16 activations need input channels in multiples of 16'),
           ((20, 32, 8, 8, 3, 1, 8, 0, 0, 1), b'strided forms need input channels'),
           ((16, 32, 8, 8, 5, 1, 8, 0, 0, 1), b'strided forms exist for 3x3'),
           ((16, 32, 8, 8, 3, 1, 24, 0, 0, 1), b'different launches'),
           ((16, 32, 8, 8, 4, 1, 0, 0, 0, 1), b'kernel size 4'),
           ((16, 32, 8, 8, 13, 1, 0, 0, 0, 1), b'kernel size 13'),
           ((16, 32, 8, 8, 3, 3, 0, 0, 0, 1), b'groups do not divide'),
           ((16, 32, 0, 8, 3, 1, 0, 0, 0, 1), b'bad shape'),
           ((16, 4096, 1024, 1024, 3, 1, 0, 0, 0, 1), b'too large for 32-bit offsets')]
    for args, msg in bad:
        assert lib.dvd_xconv_describe(*args, p) == _lib.DVD_EINVAL, args
        assert msg in lib.dvd_last_error(), (args, lib.dvd_last_error())
    assert lib.dvd_xconv_describe(16, 32, 8, 8, 3, 1, 0, 0, 0, 1, None) == _lib.DVD_EINVAL
    # every case the fp16 storages leave out is refused for them
    for case in X.CASES:
        for st in set(X.STORAGES) - set(X.storages_of(case)):
            assert X.describe(lib, case, st)[0] == _lib.DVD_EINVAL, case[0]
