"""dvd_depth_score on the GPU (csrc/depth_score.hip, ops.depth_score) against its specification (tests/depth_score_spec.py).

Inputs: depth_score_spec.score_case -- 3 seeded frames with holes in the ground truth, non-positive and wild predictions (the caps
are reached), a motion segmentation with values between 0 and 1, a mask.  Shapes, the smallest that reach every path: 1 x 1,
11 x 21 (W % 4 != 0: one pixel per thread), 12 x 24 (four pixels per thread, one block, one trip), 36 x 40 (four pixels per
thread: one block, a second, partial trip); with and without seg, with and without a mask, and as views two floats into their
buffers (W % 4 == 0 but no 16-byte alignment: the one-pixel path -- 36 x 40 is then two blocks of three trips, the last partial).  tests/test_depth_score_cpu.py shows that at most 1 % of the pixels of each case are fragile.

1. counted and regions: on non-fragile pixels `counted` is the specification's; the rows' n are the counts of `counted` under the
   fp32 comparison of seg with 0.5, exactly; n and the three delta counts are within the row's fragile pixels of the specification.
2. sums against the maps, bit for bit: sums == sum of round(maps.double() * 2^shift) over `counted` for abs_rel, sq and l, and for
   l^2 formed in fp32 from the l map.
3. maps against the specification in float64: within 4 x the distance of the SAME specification evaluated in fp32 on the same
   pixels (the project's rule for eval.hip and splat.hip: a different but legal fp32 operation order, logf's last bit), plus
   2^-24 * max|value| where that distance is 0.  sums within n * (map bound) + n_fragile * cap + n * 2^-(shift+1).
   Measured on the MI355X (worst kernel / fp32-specification distance ratio over the cases): see DESIGN.md section 7 and
   profiles/depth_score_parity_measured.jsonl.
4. two runs give equal bits; maps on or off, and two halves of N written into the rows of one tensor, give the same sums; a second
   launch doubles them; a frame with scale = NaN or without a valid pixel leaves zeros; hostile pixels leave the others alone; a
   prediction gt * c with c a power of two scores zero after the median alignment.
"""
import numpy as np
import pytest
import torch

import depth_score_spec as D
import helpers

pytestmark = pytest.mark.gpu

DEV = 'cuda'
_CACHE = {}


def _spec(shape, with_seg, with_mask):
    """The case and its float64 / fp32 specification runs: computed once per variant, never written to."""
    key = (shape, with_seg, with_mask)
    if key not in _CACHE:
        case = D.score_case(*shape)
        seg, mask = (case['seg'] if with_seg else None), (case['mask'] if with_mask else None)
        _CACHE[key] = (case, D.score(case['pred'], case['gt'], case['scale'], seg, mask),
                       D.score(case['pred'], case['gt'], case['scale'], seg, mask, dtype=np.float32))
    return _CACHE[key]


def _offset(a, lead):
    """The array as a contiguous view `lead` elements into a larger device buffer."""
    flat = torch.zeros(a.size + lead, device=DEV, dtype=helpers.t(a).dtype)
    flat[lead:].copy_(helpers.t(a, DEV).flatten())
    return flat[lead:].view(*a.shape)


def _kernel(case, with_seg, with_mask, offset=False, **kw):
    from dvd_hip import ops
    put = (lambda a, lead: _offset(a, lead)) if offset else (lambda a, lead: helpers.t(a, DEV))
    pred, gt = put(case['pred'], 2), put(case['gt'], 2)
    seg = put(case['seg'], 2) if with_seg else None
    mask = put(case['mask'], 3) if with_mask else None
    return ops.depth_score(pred, gt, helpers.t(case['scale'], DEV), seg=seg, mask=mask, **kw)


def _check_sums_against_maps(res, seg):
    """sums == what the maps and `counted` say, bit for bit."""
    sums, maps, counted = res['sums'].cpu(), res['maps'].cpu(), res['counted'].cpu().bool()
    two = float(2 ** res['shift'])
    N = sums.shape[0]
    regions = [counted]
    if seg is not None:
        sg = torch.from_numpy(seg)
        regions += [counted & (sg <= 0.5), counted & (sg > 0.5)]
    l = maps[:, 2]
    log_sq = torch.minimum(l * l, torch.tensor(D.CAP))                      # fp32, as the kernel forms it
    for r, reg in enumerate(regions):
        fixed = lambda m: ((m.double() * two).round().to(torch.int64) * reg).flatten(1).sum(1)
        assert torch.equal(sums[:, r, 0], reg.flatten(1).sum(1)), r
        assert torch.equal(sums[:, r, 1], fixed(maps[:, 0])) and torch.equal(sums[:, r, 3], fixed(maps[:, 1])), r
        assert torch.equal(sums[:, r, 5], fixed(l)) and torch.equal(sums[:, r, 4], fixed(log_sq)), r
    if seg is None:
        assert not bool(sums[:, 1:].any())
    assert not bool(maps[~counted[:, None].expand(N, 3, *counted.shape[1:])].any())      # 0 where the pixel does not count
    return sums, maps, counted


@pytest.mark.parametrize('offset', (False, True))
@pytest.mark.parametrize('with_mask', (True, False))
@pytest.mark.parametrize('with_seg', (True, False))
@pytest.mark.parametrize('shape', D.SCORE_SHAPES)
def test_kernel_against_the_specification(shape, with_seg, with_mask, offset):
    case, r64, r32 = _spec(shape, with_seg, with_mask)
    N, H, W = case['N'], case['H'], case['W']
    res = _kernel(case, with_seg, with_mask, offset=offset, maps=True)
    torch.cuda.synchronize()
    shift = res['shift']
    assert shift == r64['shift'] == 32 and res['sums'].shape == (N, 3, 9) and res['sums'].dtype == torch.int64
    assert res['maps'].shape == (N, 3, H, W) and res['counted'].shape == (N, H, W) and res['counted'].dtype == torch.uint8
    name = '%dx%d/%s/%s/%s' % (H, W, 'seg' if with_seg else 'noseg', 'mask' if with_mask else 'nomask', 'view' if offset else 'base')

    # 2. sums against the maps, bit for bit
    sums, maps, counted = _check_sums_against_maps(res, case['seg'] if with_seg else None)

    # 1. counted and the counts against the specification
    solid = ~r64['fragile']
    assert not ((counted.numpy() != r64['counted']) & solid).any(), name
    for n in range(N):
        for r in range(3):
            for i in (0, 6, 7, 8):
                assert abs(int(sums[n, r, i]) - r64['sums'][n][r][i]) <= r64['n_fragile'][n][r], (name, n, r, D.SUMS[i])

    # 3. maps and sums against the specification
    both = counted.numpy() & r64['counted'] & r32['counted'] & solid
    bound = {}
    for q in D.TERMS:
        a, b = r64[q], r32[q].astype(np.float64)
        d_fp32 = float(np.abs(a - b)[both].max()) if both.any() else 0.0
        bound[q] = 4.0 * d_fp32 if d_fp32 > 0 else 2.0 ** -24 * (float(np.abs(a[both]).max()) if both.any() else 0.0)
        if q in D.MAPS:
            g = maps[:, D.MAPS.index(q)].double().numpy()
            d_kernel = float(np.abs(g - a)[both].max()) if both.any() else 0.0
            helpers.log_measured('depth_score/%s/%s' % (name, q), d_kernel, bound[q])
            print('measured depth_score/%s/%s %.4g over %d pixels (fp32 specification %.4g, bound %.4g)' % (
                name, q, d_kernel, int(both.sum()), d_fp32, bound[q]))
            assert d_kernel <= bound[q], (name, q, d_kernel, bound[q])
    two = float(2 ** shift)
    for n in range(N):
        for r in range(3):
            s_got, s_spec, n_frag = sums[n, r].tolist(), r64['sums'][n][r], r64['n_fragile'][n][r]
            cnt = max(s_got[0], s_spec[0])
            for i, q in enumerate(D.TERMS, 1):
                limit = cnt * bound[q] + n_frag * D.TERM_CAPS[q] + cnt * 2.0 ** -(shift + 1)
                assert abs(s_got[i] - s_spec[i]) / two <= limit, (name, n, r, q, s_got[i] / two, s_spec[i] / two, limit)


@pytest.mark.parametrize('shape', D.SCORE_SHAPES)
def test_the_sums_are_reproducible_and_independent_of_maps_and_of_the_split(shape):
    case, _, _ = _spec(shape, True, True)
    N = case['N']
    first = _kernel(case, True, True, maps=True)
    again = _kernel(case, True, True, maps=True)
    assert torch.equal(first['sums'], again['sums']) and torch.equal(first['maps'], again['maps'])
    assert torch.equal(first['counted'], again['counted'])
    bare = _kernel(case, True, True)
    assert 'maps' not in bare and 'counted' not in bare and torch.equal(bare['sums'], first['sums'])
    view = _kernel(case, True, True, offset=True, maps=True)                 # the one-pixel path gives the same bits
    assert torch.equal(view['sums'], first['sums']) and torch.equal(view['maps'], first['maps'])
    # two halves of N written into the rows of one tensor
    sums = torch.zeros(N, 3, 9, device=DEV, dtype=torch.int64)
    for rows in (slice(0, 2), slice(2, N)):
        part = {k: (v[rows] if isinstance(v, np.ndarray) else v) for k, v in case.items()}
        _kernel(part, True, True, sums=sums[rows], shift=first['shift'])
    assert torch.equal(sums, first['sums'])
    # ... and accumulation means accumulation
    twice = _kernel(case, True, True, sums=first['sums'].clone())
    assert torch.equal(twice['sums'], 2 * first['sums'])
    noseg = _kernel(case, False, True)
    assert torch.equal(noseg['sums'][:, 0], first['sums'][:, 0]) and not bool(noseg['sums'][:, 1:].any())


def test_a_frame_with_a_nan_scale_or_without_a_valid_pixel_leaves_zeros():
    case = dict(D.score_case(12, 24))
    case['scale'] = np.array([np.nan, 0.5, 0.6], dtype=np.float32)
    gt = case['gt'].copy()
    gt[2] = 0.005                                                           # below g_min everywhere
    case['gt'] = gt
    res = _kernel(case, True, True, maps=True)
    sums = res['sums'].cpu()
    assert not bool(sums[0].any()) and not bool(sums[2].any()) and bool(sums[1, :, 0].all())
    assert not bool(res['counted'][0].any()) and not bool(res['counted'][2].any()) and not bool(res['maps'][0].any())
    inf = dict(case, scale=np.array([np.inf, 0.5, -np.inf], dtype=np.float32), gt=D.score_case(12, 24)['gt'])
    sums = _kernel(inf, True, True)['sums'].cpu()
    assert not bool(sums[0].any()) and not bool(sums[2].any()) and bool(sums[1, :, 0].all())


@pytest.mark.parametrize('shape', ((11, 21), (12, 24)))
def test_hostile_pixels_leave_the_others_alone(shape):
    case = D.score_case(*shape)
    clean = _kernel(case, True, False, maps=True)
    nan, inf = np.float32('nan'), np.float32('inf')
    hostile = [(nan, None), (inf, None), (-inf, None), (0.0, None), (-2.0, None),
               (None, nan), (None, inf), (None, -inf), (None, 0.0), (None, -2.0), (nan, nan), (inf, inf), (0.0, 0.0)]
    pred, gt = case['pred'].copy(), case['gt'].copy()
    H, W = shape
    r = np.random.RandomState(3)
    where = r.permutation(H * W)[:len(hostile)]
    cannot_count = np.zeros((case['N'], H, W), dtype=bool)
    for n in range(case['N']):
        for (p, g), at in zip(hostile, where):
            y, x = divmod(int(at), W)
            if p is not None:
                pred[n, 0, y, x] = p
            if g is not None:
                gt[n, 0, y, x] = g
            cannot_count[n, y, x] = not (g is not None and g == inf and p is None)      # gt = +inf > g_min: it counts, capped
    res = _kernel(dict(case, pred=pred, gt=gt), True, False, maps=True)
    _check_sums_against_maps(res, case['seg'])
    others = np.ones((case['N'], H, W), dtype=bool)
    for at in where:
        others[:, at // W, at % W] = False
    others = torch.from_numpy(others)
    assert torch.equal(res['counted'].cpu()[others], clean['counted'].cpu()[others])
    sel = others[:, None].expand(-1, 3, -1, -1)
    assert torch.equal(res['maps'].cpu()[sel], clean['maps'].cpu()[sel])
    assert not bool(res['counted'].cpu()[torch.from_numpy(cannot_count)].any())
    assert bool(torch.isfinite(res['maps']).all())
    # (the sums are the sums of these maps, checked above: what the other pixels add is what they add in the clean run)
    only_dead = _kernel(dict(case, pred=pred, gt=np.where(np.isposinf(gt), np.float32(0), gt)), True, False)
    masked_out = _kernel(dict(case, mask=others.to(torch.uint8).numpy()), True, True)
    assert torch.equal(only_dead['sums'], masked_out['sums'])


@pytest.mark.parametrize('c', (4.0, 0.125))
@pytest.mark.parametrize('shape', ((11, 21), (36, 40)))
def test_a_prediction_off_by_a_power_of_two_scores_zero_after_the_median_alignment(shape, c):
    from dvd_hip import ops
    case = D.score_case(*shape)
    N, H, W = case['N'], case['H'], case['W']
    gt = helpers.t(case['gt'], DEV)
    pred = gt * c
    keep = (gt > D.G_MIN).to(torch.uint8)
    for segments in (1, N):
        med = ops.ratio_median(gt.reshape(segments, -1), pred.reshape(segments, -1), mask=keep.reshape(segments, -1))
        scale = med['median'].expand(N).contiguous()
        assert scale.tolist() == [1.0 / c] * N and int(med['count'].sum()) == int(keep.sum())
        sums = ops.depth_score(pred, gt, scale, seg=helpers.t(case['seg'], DEV))['sums'].cpu()
        assert torch.equal(sums[:, 0, 0], keep.flatten(1).sum(1).cpu()) and bool(sums[:, 0, 0].all())
        assert not bool(sums[:, :, 1:6].any())
        for k in (6, 7, 8):
            assert torch.equal(sums[..., k], sums[..., 0])
