"""dvd_eval_tracks on the GPU (csrc/eval.hip, ops.eval_tracks) against its float64 specification (tests/eval_spec.py).

Inputs: eval_spec.kernel_case -- seeded synthetic videos of 5 frames (store_spec.random_tree: cameras, flows, masks) with a depth
step edge that occludes, 3 start frames x 3 rows of which the last start frame runs past the end of the video, some points behind
the camera and some far outside the image; points from tracks_spec.unproject in float64, cast to fp32.  Shapes, the smallest that
reach every path: 11 x 21 (one pixel per thread, one block per row), 17 x 19 (two blocks, the second partial), 12 x 24 (four
pixels per thread, one block), 36 x 40 (two blocks, the second partial); k_first 0 and 1; with and without flow pairs.
tests/test_eval_cpu.py shows that at most 1 % of the live points of each case are fragile.

1. maps against the spec: on non-fragile points "counts" agrees exactly, values within 4 x the worst distance of the fp32 run of
   the spec from its float64 run on the same inputs -- and within 4 x the kernel's own recorded distance (MEASURED, DESIGN.md
   section 7; measured on the MI355X, worst over the 16 cases):
                            rel        photo      epe
       kernel, measured     1.42e-6    1.00e-6    1.03e-4     (epe is largest on the points far outside the image, |u| ~ 300)
       fp32 specification   9.4e-7     8.5e-7     9.7e-5      (worst case each; the kernel / fp32 ratio is at most 1.5)
2. sums against the maps, bit for bit: sums == sum of round(maps.double() * 2^shift) over the counted points; the counts are the
   counts of non-negative map entries and of dvd_track_project's own `inside` / depth_at flags (the same u, v, z, d bit for bit),
   and where a point is seen the rel map is min(|z - d| / max(d, d_min), 1) in float32 of dvd_track_project's z and depth_at.
3. sums against the spec: counts within the row's fragile points, value sums within n * (map bound) + n_fragile * cap +
   n * 2^-(shift+1).
4. two runs give equal bits; maps on or off, and two halves of B accumulated into one tensor, give the same sums; dead rows are
   exactly zero and their maps -1.
"""
import numpy as np
import pytest
import torch

import eval_spec as E
import helpers

pytestmark = pytest.mark.gpu

DEV = 'cuda'
QUANTITIES = ('rel', 'photo', 'epe')
CAPS = {'rel': 1.0, 'photo': E.CAP, 'epe': E.CAP}
# worst distance of the kernel's maps from the float64 specification over the 16 cases, measured on the MI355X; the kernel
# must stay below 4 x this (and below 4 x the fp32 specification's own distance on each case)
MEASURED = {'rel': 1.42e-6, 'photo': 1.00e-6, 'epe': 1.03e-4}

_CACHE = {}


def _spec(shape, k_first):
    """The case and its float64 / fp32 specification runs (with pairs): computed once per (shape, k_first), never written to."""
    key = (shape, k_first)
    if key not in _CACHE:
        case = E.kernel_case(shape[0], shape[1], k_first)
        _CACHE[key] = (case, E.run_case(case), E.run_case(case, dtype=torch.float32))
    return _CACHE[key]


def _without_pairs(res):
    """What the spec gives without pairs: the same rel and photo, epe counting nowhere."""
    out = dict(res)
    out['maps'] = res['maps'].clone()
    out['maps'][:, :, 2] = -1.0
    out['sums'] = [[row[:4] + [0, 0] for row in step] for step in res['sums']]
    return out


def _kernel(case, with_pairs, maps=True, sums=None, cols=None):
    from dvd_hip import ops
    c = slice(None) if cols is None else cols
    tables = {k: helpers.t(case[k], DEV) for k in ('R', 't', 'K_T')}
    pairs = None
    if with_pairs:
        pairs = (np.ascontiguousarray(case['pair_row'][:, c]), helpers.t(case['flow_1_2'], DEV), helpers.t(case['mask'], DEV))
    return ops.eval_tracks(helpers.t(case['points'], DEV)[:, c], case['source'][c], tables, helpers.t(case['depth_all'], DEV),
                           helpers.t(case['img_all'], DEV), k_first=case['k_first'], pairs=pairs, sums=sums, maps=maps)


def _map_distances(got, r64, r32):
    """Per quantity: (kernel vs float64, fp32 spec vs float64) worst distance over the points that count in all three and are
    not fragile; and the number of non-fragile points where `counts` disagrees."""
    solid = ~r64['fragile']
    out, disagree = {}, 0
    for i, q in enumerate(QUANTITIES):
        g, a, b = got[:, :, i].double(), r64['maps'][:, :, i], r32['maps'][:, :, i].double()
        disagree += int((((g >= 0) != (a >= 0)) & solid).sum())
        both = (g >= 0) & (a >= 0) & (b >= 0) & solid
        out[q] = (float((g - a).abs()[both].max()) if bool(both.any()) else 0.0,
                  float((b - a).abs()[both].max()) if bool(both.any()) else 0.0, int(both.sum()))
    return out, disagree


@pytest.mark.parametrize('with_pairs', (True, False))
@pytest.mark.parametrize('k_first', (0, 1))
@pytest.mark.parametrize('shape', E.KERNEL_SHAPES)
def test_kernel_against_the_specification(shape, k_first, with_pairs):
    from dvd_hip import ops
    case, r64, r32 = _spec(shape, k_first)
    if not with_pairs:
        r64, r32 = _without_pairs(r64), _without_pairs(r32)
    T, B, H, W = case['T'], case['B'], case['H'], case['W']
    res = _kernel(case, with_pairs)
    torch.cuda.synchronize()
    shift = res['shift']
    assert shift == r64['shift'] == 32 and res['sums'].shape == (T, B, 6) and res['sums'].dtype == torch.int64
    assert res['maps'].shape == (T, B, 3, H, W)
    got, sums = res['maps'].cpu(), res['sums'].cpu()
    name = '%dx%d/k%d/%s' % (H, W, k_first, 'pairs' if with_pairs else 'nopairs')

    # 1. maps against the spec
    dist, disagree = _map_distances(got, r64, r32)
    assert disagree == 0, name
    bound = {}
    for q in QUANTITIES:
        d_kernel, d_fp32, n = dist[q]
        bound[q] = 4.0 * d_fp32
        helpers.log_measured('eval/%s/%s' % (name, q), d_kernel, bound[q])
        print('measured eval/%s/%s %.4g over %d points (fp32 specification %.4g, recorded %s)' % (
            name, q, d_kernel, n, d_fp32, MEASURED[q]))
    for q in QUANTITIES:
        assert dist[q][0] <= bound[q], (name, q, dist[q])
        if MEASURED[q] is not None:
            assert dist[q][0] <= 4.0 * MEASURED[q], (name, q, dist[q][0], MEASURED[q])
    assert with_pairs == bool((got[:, :, 2] >= 0).any())

    # 2. sums against the maps, bit for bit; the counts against the maps and against dvd_track_project's flags
    counted = got >= 0
    q_maps = (got.double() * float(2 ** shift)).round().to(torch.int64) * counted
    want = q_maps.flatten(3).sum(3)                                           # [T,B,3]
    assert torch.equal(sums[..., 2], want[..., 0]) and torch.equal(sums[..., 3], want[..., 1]), name
    assert torch.equal(sums[..., 5], want[..., 2]), name
    n_counted = counted.flatten(3).sum(3)
    assert torch.equal(sums[..., 0] - sums[..., 1], n_counted[..., 0]) and torch.equal(n_counted[..., 0], n_counted[..., 1])
    assert torch.equal(sums[..., 4], n_counted[..., 2])
    tables = {k: helpers.t(case[k], DEV) for k in ('R', 't', 'K_T')}
    proj = ops.track_project(helpers.t(case['points'], DEV), (case['source'] + k_first).tolist(), tables,
                             depth_all=helpers.t(case['depth_all'], DEV))
    inside = proj['inside'].cpu().bool()
    tol = (np.float32(1.0) + np.float32(0.05)).item()
    occluded = inside & (proj['z'].cpu() > proj['depth_at'].cpu() * torch.tensor(tol, dtype=torch.float32))
    assert torch.equal(sums[..., 0], inside.flatten(2).sum(2)) and torch.equal(sums[..., 1], occluded.flatten(2).sum(2)), name
    assert torch.equal(counted[:, :, 0], inside & ~occluded), name
    # ... and the rel map itself: float32 arithmetic on dvd_track_project's z and depth_at of the same slab, bit for bit
    seen = counted[:, :, 0].numpy()
    z, d = proj['z'].cpu().numpy(), proj['depth_at'].cpu().numpy()
    with np.errstate(all='ignore'):                                           # (points that are not seen may divide by anything)
        rel = np.minimum(np.abs(z - d) / np.maximum(d, np.float32(1e-3)), np.float32(1.0))
    assert rel.dtype == np.float32 and seen.any()
    assert np.array_equal(got[:, :, 0].numpy()[seen].view(np.uint32), rel[seen].view(np.uint32)), name

    # 3. sums against the spec
    scale = float(2 ** shift)
    for r in range(T):
        for b in range(B):
            s_got, s_spec, n_frag = sums[r, b].tolist(), r64['sums'][r][b], r64['n_fragile'][r][b]
            for i in (0, 1, 4):
                assert abs(s_got[i] - s_spec[i]) <= n_frag, (name, r, b, E.SUMS[i], s_got, s_spec, n_frag)
            n_seen, n_flow = max(s_got[0] - s_got[1], s_spec[0] - s_spec[1]), max(s_got[4], s_spec[4])
            for i, q, n in ((2, 'rel', n_seen), (3, 'photo', n_seen), (5, 'epe', n_flow)):
                limit = n * bound[q] + n_frag * CAPS[q] + n * 2.0 ** -(shift + 1)
                assert abs(s_got[i] - s_spec[i]) / scale <= limit, (name, r, b, q, s_got[i] / scale, s_spec[i] / scale, limit)

    # 4. dead rows: the last start frame's later rows look past the end of the video
    live = r64['live']
    assert not bool(live.all()) and not bool(sums[~live].any()) and bool((got[~live] == -1).all())
    assert bool(sums[live][:, 0].all())


@pytest.mark.parametrize('shape', E.KERNEL_SHAPES)
def test_the_sums_are_reproducible_and_independent_of_maps_and_of_the_split(shape):
    case, _, _ = _spec(shape, 1)
    T, B = case['T'], case['B']
    first = _kernel(case, True)
    again = _kernel(case, True)
    assert torch.equal(first['sums'], again['sums']) and torch.equal(first['maps'], again['maps'])
    bare = _kernel(case, True, maps=False)
    assert 'maps' not in bare and torch.equal(bare['sums'], first['sums'])
    # two halves of B accumulated into the columns of one tensor
    sums = torch.zeros(T, B, 6, device=DEV, dtype=torch.int64)
    maps = torch.full((T, B, 3, case['H'], case['W']), 7.0, device=DEV)
    _kernel(case, True, maps=maps[:, :2], sums=sums[:, :2], cols=slice(0, 2))
    _kernel(case, True, maps=maps[:, 2:], sums=sums[:, 2:], cols=slice(2, B))
    assert torch.equal(sums, first['sums']) and torch.equal(maps, first['maps'])
    # ... and accumulation means accumulation
    twice = _kernel(case, True, maps=False, sums=first['sums'].clone())
    assert torch.equal(twice['sums'], 2 * first['sums'])
    nopairs = _kernel(case, False, maps=False)
    assert torch.equal(nopairs['sums'][..., :4], first['sums'][..., :4]) and not bool(nopairs['sums'][..., 4:].any())
