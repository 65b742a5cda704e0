"""ops.fill_holes (csrc/fill.hip) on the GPU against its float64 specification (tests/fill_spec.py).

Cases (fill_spec.CASES): 2 x 2 and 1 x 7 (the smallest pyramids), 11 x 21 (one partial tile), 33 x 65 and 70 x 45 (several tiles,
odd sizes, holes across tile borders), 36 x 64 (the four-pixel accesses over several tiles), 97 x 130 with a 50 x 40 hole and 2 %
known elsewhere (the middle kernel, levels >= 6), one known pixel in a corner, all pixels known, one of three views empty, and a
bias holding 0, a negative value, Inf and NaN on known pixels.  Each with C = 1, 4, 8 and power 0 and 2, the bias in [0.5, 20].
Unknown pixels of the input hold NaNs here and there: nothing may be read from them.

Exact, on every pixel: `level` is the specification's (no decision depends on a rounding), known pixels come back bit for bit,
V = 3 gives the bits of three V = 1 calls, two runs give the same bits, out_values aliasing values and a base that is not
16-byte aligned change no bit.

Values: per case the limit is 4 x the largest distance between the float32 and the float64 evaluation of the specification on
that case plus 2 ulp of max|values|, the rule of tests/test_48_splat_gpu.py, computed here.  Measured on the MI355X, worst over
the 66 cases of this file (values in [0, 1]):
    kernels               1.70e-7    (97x130, C = 8, power 2: 21 % of its limit of 7.99e-7, the closest any case comes)
    fp32 specification    1.70e-7    (the yardstick)
The two rows are equal because on every case the kernels returned the bits of the float32 evaluation of the specification:
every statement of csrc/fill.hip is the specification's, in its order.  That is reported, not required: the assertion is the limit.
"""
import functools

import numpy as np
import pytest
import torch

import fill_spec as F
import helpers

pytestmark = pytest.mark.gpu

DEV = 'cuda'
# what the MI355X gave over the cases of this file (recorded for later comparison, asserted nowhere)
MEASURED = {'values': 1.70e-7, 'closest': ('97x130', 8, 2, 0.21), 'equals_fp32_spec': True}


@functools.lru_cache(maxsize=None)
def _spec(name, C, power):
    case = F.make(name, C=C)
    r64 = F.fill(case['values'], case['known'], case['bias'], power, case['fill'])
    r32 = F.fill(case['values'], case['known'], case['bias'], power, case['fill'], dtype=np.float32)
    for r in (r64, r32):
        for v in r.values():
            v.setflags(write=False)
    return case, r64, r32


def _run(case, power, **kw):
    from dvd_hip import ops
    out = ops.fill_holes(helpers.t(case['values'], DEV), helpers.t(case['known'], DEV), helpers.t(case['bias'], DEV), power,
                         case['fill'], **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(a, b, what):
    for k in ('values', 'level'):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)


@pytest.mark.parametrize('power', [0, 2])
@pytest.mark.parametrize('C', [1, 4, 8])
@pytest.mark.parametrize('name', sorted(F.CASES))
def test_against_the_specification(name, C, power):
    case, r64, r32 = _spec(name, C, power)
    got = _run(case, power)
    assert got['values'].dtype == np.float32 and got['values'].shape == case['values'].shape
    assert got['level'].dtype == np.uint8 and got['level'].shape == case['known'].shape
    assert np.array_equal(got['level'], r64['level']), 'level differs on %d pixels' % int((got['level'] != r64['level']).sum())
    known = np.broadcast_to((r64['level'] == 0)[:, None], case['values'].shape)
    assert np.array_equal(_bits(got['values'][known]), _bits(case['values'][known]))
    assert np.isfinite(got['values']).all()
    d, lim = F.worst(got['values'], r64['values']), F.limit(case, r64, r32)
    same32 = np.array_equal(_bits(got['values']), _bits(r32['values']))
    print('fill/%s C=%d power=%d: kernels %.4g, fp32 spec %.4g, limit %.4g (%.0f %%), bits of the fp32 spec: %s' % (
        name, C, power, d, F.worst(r32['values'], r64['values']), lim, 100 * d / lim, same32))
    helpers.log_measured('fill/%s/C%d/p%d' % (name, C, power), d, lim)
    assert d <= lim
    if name == 'all_known':
        assert np.array_equal(_bits(got['values']), _bits(case['values'])) and not got['level'].any()
    if name == 'one_empty':
        assert (got['values'][1] == np.float32(case['fill'])).all() and (got['level'][1] == F.EMPTY).all()


def test_a_view_does_not_depend_on_the_views_it_shares_the_call_with():
    case, _, _ = _spec('one_empty', 4, 2)
    both = _run(case, 2)
    for v in range(3):
        one = _run({k: (a[v:v + 1] if k != 'fill' else a) for k, a in case.items()}, 2)
        _same({k: a[v:v + 1] for k, a in both.items()}, one, v)


def test_two_runs_an_aliased_output_and_preallocated_tensors_give_the_same_bits():
    from dvd_hip import ops
    for name, C in (('97x130', 8), ('36x64', 4), ('70x45', 1)):
        case, _, _ = _spec(name, C, 2)
        first = _run(case, 2)
        _same(_run(case, 2), first, (name, 'again'))
        values, known, bias = (helpers.t(case[k], DEV) for k in ('values', 'known', 'bias'))
        V, _, H, W = values.shape
        ws = ops.fill_workspace(V, C, H, W, DEV)
        ws.fill_(float('nan'))                                       # the workspace comes uncleared
        level = torch.full((V, H, W), 77, device=DEV, dtype=torch.uint8)
        out = ops.fill_holes(values, known, bias, 2, case['fill'], out={'values': values, 'level': level}, workspace=ws)
        assert out['values'] is values and out['level'] is level
        torch.cuda.synchronize()
        _same({k: v.cpu().numpy() for k, v in out.items()}, first, (name, 'in place'))


def test_a_base_that_is_not_16_byte_aligned_takes_the_one_pixel_path():
    from dvd_hip import ops
    case, _, _ = _spec('36x64', 4, 2)
    first = _run(case, 2)

    def shifted(a, by):
        flat = torch.zeros(a.size + by, dtype=torch.from_numpy(a[:0]).dtype, device=DEV)
        flat[by:] = helpers.t(a, DEV).reshape(-1)
        return flat[by:].view(a.shape)

    values, known, bias = shifted(case['values'], 1), shifted(case['known'], 3), shifted(case['bias'], 3)
    assert values.data_ptr() % 16 == 4 and known.data_ptr() % 4 == 3 and values.is_contiguous()
    out = ops.fill_holes(values, known, bias, 2, case['fill'],
                         out={'values': shifted(np.zeros_like(case['values']), 2), 'level': shifted(np.zeros_like(case['known']), 1)})
    torch.cuda.synchronize()
    _same({k: v.cpu().numpy() for k, v in out.items()}, first, 'shifted')
    # in place too
    out = ops.fill_holes(values, known, bias, 2, case['fill'], out={'values': values})
    torch.cuda.synchronize()
    _same({k: v.cpu().numpy() for k, v in out.items()}, first, 'shifted, in place')


def test_no_bias_is_power_zero_and_the_wrapper_refuses_what_the_kernels_do_not_take():
    from dvd_hip import ops
    case, r64, _ = _spec('33x65', 4, 0)
    values, known, bias = (helpers.t(case[k], DEV) for k in ('values', 'known', 'bias'))
    want = _run(case, 0)
    for kw in (dict(bias=None, power=0), dict(bias=None, power=3), dict(bias=bias, power=0)):
        out = ops.fill_holes(values, known, fill=case['fill'], **kw)
        torch.cuda.synchronize()
        _same({k: v.cpu().numpy() for k, v in out.items()}, want, kw['power'])
    for kw, word in ((dict(power=5), 'power'), (dict(power=-1), 'power'), (dict(power=1.5), 'power'), (dict(fill='0'), 'fill'),
                     (dict(known=known.float()), 'known'), (dict(known=known[:, :-1]), 'known'), (dict(known=None), 'known'),
                     (dict(bias=bias[:, 0]), 'bias'), (dict(bias=bias.double()), 'bias'), (dict(values=values[0]), 'values'),
                     (dict(values=values.repeat(1, 3, 1, 1)), 'values'), (dict(out={'level': torch.zeros(1, 33, 65, device=DEV)}), 'level'),
                     (dict(workspace=torch.zeros(8, device=DEV)), 'workspace')):
        with pytest.raises(RuntimeError, match=word):
            ops.fill_holes(**dict(dict(values=values, known=known, bias=bias, power=2), **kw))
    with pytest.raises(RuntimeError, match='tiles'):
        ops.fill_holes(torch.zeros(1, 1, 8, 32 * 2048 + 1, device=DEV), torch.zeros(1, 8, 32 * 2048 + 1, device=DEV, dtype=torch.uint8))
