"""ops.flow_chain (csrc/flow_chain.hip) against its fp32 contract, tests/flow_chain_spec.py: BIT FOR BIT on both outputs, and
never a NaN or an Inf.  The largest case is 33 x 258 with 32 links.

Against the float64 reference on the gap-1 chains of scene(24, 40, 7, noise=0.4) (the last test): `broken` is equal on every
pixel whose float64 walk is decided, and the flow is compared on those that are unbroken besides.  The bound is 4 x the worst
distance measured on the MI355X, flow_chain_spec.MEASURED -- the margin triangulate_spec.MEASURED uses, for the same reason:
other shapes and seeds.  (The kernel equals the fp32 contract bit for bit, so this is also the contract's distance.)
"""
import numpy as np
import pytest
import torch

import flow_chain_spec as C
import helpers
import triangulate_spec as T

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _fields(P, H, W, seed, sigma=1.5, masked=0.05):
    """Random smooth-less flows of `sigma` px and masks with a share `masked` of set bytes: every tap pattern, many breaks."""
    rng = np.random.default_rng(seed)
    f12 = rng.normal(0, sigma, (P, H, W, 2)).astype(np.float32)
    f21 = rng.normal(0, sigma, (P, H, W, 2)).astype(np.float32)
    m1 = (rng.random((P, H, W)) < masked).astype(np.uint8) * rng.integers(1, 256, (P, H, W)).astype(np.uint8)
    m2 = (rng.random((P, H, W)) < masked).astype(np.uint8) * rng.integers(1, 256, (P, H, W)).astype(np.uint8)
    return f12, f21, m1, m2


def _gpu(fields, links, out=None):
    from dvd_hip import ops
    res = ops.flow_chain(*(helpers.t(a, DEV) for a in fields), links, out=out)
    return {k: res[k].cpu().numpy() for k in ('flow', 'broken')}


def _check(fields, links, what='', out=None):
    got, want = _gpu(fields, links, out), C.chain(*fields, links, np.float32)
    for k in ('flow', 'broken'):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, want[k].shape)
        assert np.isfinite(got[k]).all(), (what, k)
        same = _bits(got[k]) == _bits(want[k])
        assert same.all(), (what, k, int((~same).sum()), got[k][~same][:4], want[k][~same][:4])
    return got


def _links(rng, B, L, P, lengths=None):
    """B chains of L links over P pairs with both dirs; lengths: links before the -1 of each chain (None: all L)."""
    ln = np.stack([rng.integers(0, P, (B, L)), rng.integers(0, 2, (B, L))], -1).astype(np.int32)
    for b, n in enumerate(lengths or []):
        ln[b, n:] = -1
    return ln


@pytest.mark.parametrize('H,W', [(5, 7), (24, 40), (33, 258)])
@pytest.mark.parametrize('L', [1, 3, 32])
@pytest.mark.parametrize('B', [1, 5])
def test_shapes_lengths_and_chains(H, W, L, B):
    rng = np.random.default_rng(H * 1000 + L * 10 + B)
    P = 4
    # (32 links of 1.5 px would leave nothing whole: the long chains walk smaller steps through fewer masked bytes)
    fields = _fields(P, H, W, seed=H + L + B, sigma=1.5 if L <= 3 else 0.4, masked=0.05 if L <= 3 else 0.004)
    links = _links(rng, B, L, P)
    got = _check(fields, links, what=(H, W, L, B))
    assert got['flow'].shape == (L, B, H, W, 2) and got['broken'].shape == (L, B, H, W)
    if (H, W) != (5, 7):
        last = got['broken'][L - 1]
        assert (last == 0).mean() > 0.05 and (last != 0).mean() > 0.02, (float((last == 0).mean()))      # whole and broken chains
        if L > 1:
            assert len(np.unique(last)) > 2                                                      # ... broken at different links


def test_unequal_lengths_both_dirs_and_a_minus_one_in_the_middle():
    H, W, P = 24, 40, 5
    fields = _fields(P, H, W, seed=11, sigma=0.8, masked=0.02)
    rng = np.random.default_rng(12)
    links = _links(rng, 6, 7, P, lengths=[7, 1, 4, 0, 3, 6])
    links[2, 5:] = [[1, 0], [2, 1]]                                       # live-looking rows AFTER the -1 of chain 2: ignored
    links[4, 0], links[4, 1], links[4, 2] = (3, 0), (3, 1), (0, 1)       # both dirs in one chain: there, back, and on
    got = _check(fields, links, what='ragged')
    assert (got['broken'][4:, 2] == 255).all() and (got['flow'][4:, 2] == 0).all() and (got['broken'][3, 2] != 255).all()
    assert (got['broken'][:, 3] == 255).all() and (got['flow'][:, 3] == 0).all()             # a chain that ends at once
    assert (got['broken'][1:, 1] == 255).all() and (got['broken'][0, 1] <= 1).all()
    # a chain is its own result whatever it shares a launch with
    alone = _check(fields, links[4:5], what='alone')
    for k in ('flow', 'broken'):
        assert np.array_equal(_bits(alone[k][:, 0]), _bits(got[k][:, 4])), k
    # a pair that is no pair cannot get past the wrapper
    from dvd_hip import ops
    dev = [helpers.t(a, DEV) for a in fields]
    bad_pair, bad_low, bad_dir = links.copy(), links.copy(), links.copy()
    bad_pair[0, 2, 0], bad_low[0, 2, 0], bad_dir[0, 2, 1] = P, -2, 2
    for kw, word in ((dict(links=bad_pair), 'links names pairs'), (dict(links=bad_low), 'links names pairs'), (dict(links=bad_dir), 'dir column'),
                     (dict(flow_2_1=dev[1][:-1]), 'flow_2_1'), (dict(flow_1_2=dev[0].transpose(1, 2)), 'flow_1_2'),
                     (dict(mask_1=dev[2].float()), 'mask_1'), (dict(mask_2=None), 'mask_2'), (dict(mask_2=dev[3].cpu()), 'mask_2'),
                     (dict(zip(('flow_1_2', 'flow_2_1', 'mask_1', 'mask_2'), (d[:, :1].contiguous() for d in dev))), 'H, W >= 2'),
                     (dict(out={'flow': torch.empty(7, 6, H, W, 2, device=DEV).transpose(0, 1)}), r"out\['flow'\]"),
                     (dict(out={'flow': torch.empty(7, 6, H, W, 2, device=DEV, dtype=torch.float64)}), r"out\['flow'\]"),
                     (dict(out={'broken': torch.empty(7, 6, H, W, device=DEV)}), r"out\['broken'\]")):
        with pytest.raises(RuntimeError, match=word):
            ops.flow_chain(**dict(dict(flow_1_2=dev[0], flow_2_1=dev[1], mask_1=dev[2], mask_2=dev[3], links=links), **kw))


def test_hostile_input_and_the_last_row_and_column():
    h, w = 5, 7
    rng = np.random.default_rng(4)
    f12 = rng.normal(0, 0.3, (2, h, w, 2)).astype(np.float32)
    f21 = rng.normal(0, 0.3, (2, h, w, 2)).astype(np.float32)
    m1, m2 = np.zeros((2, h, w), np.uint8), np.zeros((2, h, w), np.uint8)
    f12[0, 0, 0], f12[0, 0, 1], f12[0, 0, 2], f12[0, 1, 1] = np.nan, (np.inf, 0), (1e30, -1e30), (3e38, 3e38)
    f12[0, 2, 3], f12[1, 2, 4] = (1.0, 0.0), (2.0, 2.0)                  # exactly onto (4, 2), then exactly onto W-1, H-1
    f12[0, 3, 3], m2[1, 3, 3] = (0.0, 0.0), 1
    f12[0, 4, 6], f12[1, 4, 6] = (0.0, 0.0), (0.0, 0.0)                  # the corner pixel stays on the corner
    f12[0, 3, 0] = (-0.5, 0.0)
    f12[0, 1, 4], m2[1, 1, 5] = (0.5, 0.0), 255
    f21[1, 0, 0], m2[1, 1, 1] = (1e-30, 1e-30), 1                        # wx * wy underflows to exactly 0: (1, 1) is not read or tested
    links = np.array([[[0, 0], [1, 0], [1, 1]], [[1, 1], [1, 0], [0, 0]], [[0, 0], [-1, 0], [1, 0]]], np.int32)
    got = _check((f12, f21, m1, m2), links, what='hostile')
    br = got['broken']
    assert (br[:, 0, 0, 0] == 1).all() and (br[:, 0, 0, 1] == 1).all() and br[:, 0, 0, 2].tolist() == [0, 2, 2]
    assert br[:, 0, 2, 3].tolist() == [0, 0, br[2, 0, 2, 3]] and got['flow'][1, 0, 2, 3].tolist() == [3.0, 2.0]
    assert br[:2, 1, 0, 0].tolist() == [0, 0]
    assert br[:, 0, 3, 3].tolist() == [0, 2, 2] and br[:, 0, 1, 4].tolist() == [0, 2, 2] and br[:, 0, 4, 6].tolist()[:2] == [0, 0]


def test_a_strided_destination_and_two_runs():
    from dvd_hip import ops
    H, W, P, B, L = 24, 40, 4, 3, 5
    fields = _fields(P, H, W, seed=21, sigma=0.8, masked=0.02)
    links = _links(np.random.default_rng(22), B, L, P, lengths=[5, 2, 4])
    want = _check(fields, links, what='plain')
    big = torch.full((L, B + 2, H, W, 2), -7.0, device=DEV)
    out = {'flow': big[:, 1:1 + B], 'broken': torch.empty(L, B, H, W, device=DEV, dtype=torch.uint8)}
    dev = [helpers.t(a, DEV) for a in fields]
    res = ops.flow_chain(*dev, links, out=out)
    assert res['flow'] is out['flow'] and res['broken'] is out['broken'] and not res['flow'].is_contiguous()
    assert np.array_equal(_bits(res['flow'].cpu().numpy()), _bits(want['flow'])) and np.array_equal(res['broken'].cpu().numpy(), want['broken'])
    assert (big[:, 0] == -7).all() and (big[:, B + 1:] == -7).all()      # nothing is written between the rows
    again = ops.flow_chain(*dev, links)
    assert torch.equal(again['flow'].view(torch.int32), res['flow'].contiguous().view(torch.int32)) and torch.equal(again['broken'], res['broken'])


def test_against_the_float64_reference():
    N = 7
    sc = T.scene(24, 40, N, seed=0, noise=0.4, gaps=(1,))
    fields = tuple(sc[k] for k in ('flow_1_2', 'flow_2_1', 'mask_1', 'mask_2'))
    worst, n_cmp, n_all = 0.0, 0, 0
    for g in (2, 3, 4):
        _, fwd, bwd = C.gap1_links(N, g)
        for links in (fwd, bwd):
            got, ref = _gpu(fields, links), C.chain(*fields, links, np.float64)
            ok = ref['decided']
            n_all += ok.size
            n_cmp += int(ok.sum())
            assert np.array_equal(got['broken'][:, ok], ref['broken'][:, ok]), g
            whole = ok[None] & (ref['broken'] == 0)
            worst = max(worst, C.distance(got['flow'], ref['flow'], whole)[0])
    assert n_all - n_cmp <= 0.01 * n_all                                 # (tests/test_flow_chain_cpu.py asserts the same cap on the spec alone)
    bound = 4.0 * C.MEASURED['flow']
    helpers.log_measured('flow_chain/flow', worst, bound)
    print('measured flow_chain/flow %.4g px (bound %.4g); undecided %d of %d' % (worst, bound, n_all - n_cmp, n_all))
    assert worst <= bound
