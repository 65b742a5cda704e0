"""Host side of the flow-chaining feature (preprocess.chain_plan, ops.flow_chain's refusals, the C ABI's declaration) and the
properties of its specification (tests/flow_chain_spec.py) that the GPU tests rest on.  No device is needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import flow_chain_spec as C
import triangulate_spec as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WELL_BELOW = 0.25          # px: 'well below' the consistency rule's 1 px, fixed before anything was measured


def _pairs(N, gaps):
    return [(a, a + g) for g in gaps for a in range(N - g)]


# ---- the plan ---------------------------------------------------------------------------------------------------------------

def test_plan_order_padding_and_directions():
    from dvd_hip import preprocess
    pairs = _pairs(7, (1,))
    new, fwd, bwd = preprocess.chain_plan(pairs, 7, [3, 2, 2])
    assert new == [(a, a + 2) for a in range(5)] + [(a, a + 3) for a in range(4)]        # gaps ascending, f_1 ascending
    assert fwd.dtype == bwd.dtype == np.int32 and fwd.shape == bwd.shape == (9, 3, 2)
    assert fwd[0].tolist() == [[0, 0], [1, 0], [-1, -1]] and bwd[0].tolist() == [[1, 1], [0, 1], [-1, -1]]
    assert fwd[8].tolist() == [[3, 0], [4, 0], [5, 0]] and bwd[8].tolist() == [[5, 1], [4, 1], [3, 1]]
    for got, want in zip((new, fwd, bwd), C.chain_plan(pairs, 7, [3, 2, 2])):
        assert np.array_equal(got, want)
    # every chain is a path: link k leaves the frame link k-1 reached
    for (a, b), row in zip(new, fwd.tolist()):
        f = a
        for j, d in row:
            if j >= 0:
                assert d == 0 and pairs[j][0] == f
                f = pairs[j][1]
        assert f == b


def test_plan_is_greedy_skips_stored_pairs_and_honours_base():
    from dvd_hip import preprocess
    pairs = _pairs(12, (1, 2, 3, 4))
    at = {p: j for j, p in enumerate(pairs)}
    new, fwd, bwd = preprocess.chain_plan(pairs, 12, [4, 7, 8])
    assert new == [(a, a + 7) for a in range(5)] + [(a, a + 8) for a in range(4)]        # gap 4 is held in full: nothing to do
    assert fwd.shape == (9, 2, 2)
    assert fwd[0].tolist() == [[at[(0, 4)], 0], [at[(4, 7)], 0]] and bwd[0].tolist() == [[at[(4, 7)], 1], [at[(0, 4)], 1]]
    assert fwd[5].tolist() == [[at[(0, 4)], 0], [at[(4, 8)], 0]]
    new1, fwd1, bwd1 = preprocess.chain_plan(pairs, 12, [7], base=[1])
    assert fwd1.shape == (5, 7, 2) and fwd1[2, :, 0].tolist() == [at[(f, f + 1)] for f in range(2, 9)] and (fwd1[..., 1] == 0).all()
    assert bwd1[2, :, 0].tolist() == [at[(f, f + 1)] for f in range(8, 1, -1)] and (bwd1[..., 1] == 1).all()
    for got, want in zip((new, fwd, bwd), C.chain_plan(pairs, 12, [4, 7, 8])):
        assert np.array_equal(got, want)
    for got, want in zip((new1, fwd1, bwd1), C.chain_plan(pairs, 12, [7], base=[1])):
        assert np.array_equal(got, want)
    # a gap that is held in part: only the missing pair is planned, from what IS stored
    part = _pairs(8, (1,)) + [(a, a + 2) for a in range(6) if a != 3]
    new, fwd, bwd = preprocess.chain_plan(part, 8, [2])
    assert new == [(3, 5)] and fwd.tolist() == [[[3, 0], [4, 0]]] and bwd.tolist() == [[[4, 1], [3, 1]]]
    # the writer's default pair set leaves out the last pair of every gap: the last frame has no pair, so no chain reaches it
    short = [(a, a + g) for g in (1, 2) for a in range(8 - 1 - g)]
    with pytest.raises(ValueError, match=r'pair \(4, 7\) cannot be reached'):
        preprocess.chain_plan(short, 8, [3])


def test_plan_unreachable_pairs_and_the_32_link_cap():
    from dvd_hip import ops, preprocess
    assert ops.CHAIN_MAX_LINKS == C.MAX_LINKS == 32
    pairs = _pairs(40, (1,))
    new, fwd, _ = preprocess.chain_plan(pairs, 40, [32])
    assert fwd.shape == (8, 32, 2) and (fwd[..., 0] >= 0).all()
    with pytest.raises(ValueError, match=r'pair \(0, 33\) needs more than 32 links'):
        preprocess.chain_plan(pairs, 40, [33])
    preprocess.chain_plan(pairs + _pairs(40, (2,)), 40, [33])                               # 16 x 2 + 1: 17 links
    with pytest.raises(ValueError, match=r'pair \(0, 33\) needs more than 32 links'):
        preprocess.chain_plan(pairs + _pairs(40, (2,)), 40, [33], base=[1])
    # a hole in the gap-1 pairs: the first pair that has to cross it is named
    holed = [p for p in _pairs(7, (1,)) if p != (3, 4)]
    with pytest.raises(ValueError, match=r'pair \(2, 4\) cannot be reached'):
        preprocess.chain_plan(holed, 7, [2])
    with pytest.raises(ValueError, match=r'pair \(0, 2\) cannot be reached'):
        preprocess.chain_plan(_pairs(7, (1, 3)), 7, [2], base=[3])
    with pytest.raises(ValueError, match=r'pair \(0, 7\) cannot be reached'):                # 3 + 3 leaves 1, and base has no 1
        preprocess.chain_plan(_pairs(12, (1, 2, 3)), 12, [7], base=[2, 3])
    for kw in (dict(gaps=[]), dict(gaps=[0]), dict(gaps=[1.5]), dict(gaps=None), dict(gaps=[2], base=[]), dict(gaps=[2], base=[0])):
        with pytest.raises(ValueError, match='chain_plan'):
            preprocess.chain_plan(_pairs(7, (1,)), 7, **kw)
    with pytest.raises(ValueError, match='chain_plan'):
        preprocess.chain_plan([(0, 9)], 7, [2])
    new, fwd, bwd = preprocess.chain_plan(_pairs(7, (1, 2)), 7, [1, 2])                     # nothing is missing
    assert new == [] and fwd.shape == bwd.shape == (0, 1, 2)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------

def test_header_sources_and_binding_agree():
    from dvd_hip import _lib, build, ops
    src = open(os.path.join(ROOT, 'include', 'dvd_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'\bint\s+dvd_flow_chain\s*\(([^)]*)\)\s*;', code)
    assert m, 'include/dvd_hip.h does not declare dvd_flow_chain'
    want = []
    for prm in m.group(1).split(','):
        prm = ' '.join(prm.split())
        if '*' in prm or prm.startswith('dvd_stream_t'):
            want.append(ctypes.c_void_p)
        elif prm.startswith('long long'):
            want.append(ctypes.c_longlong)
        else:
            assert prm.startswith('int '), prm
            want.append(ctypes.c_int)
    res, args = _lib.SIGNATURES['dvd_flow_chain']
    assert res is ctypes.c_int and list(args) == want
    assert ('flow_chain.hip', ['-ffp-contract=off']) in build.SOURCES
    assert _lib.ABI_VERSION == 8
    assert 'flow_chain_kernel' in ops.BYTE_CLASS_KERNELS['geometry']
    # the entry refuses bad arguments before any HIP call
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    #       f12 f21 m1 m2 P  links live out stride broken L  B  H  W  stream
    good = [p, p, p, p, 3, p, 2, p, 2 * 1 * 4 * 5, p, 2, 1, 4, 5, None]
    for at, bad, word in ((0, None, b'null'), (3, None, b'null'), (5, None, b'null'), (7, None, b'null'), (9, None, b'null'),
                          (10, 0, b'L=0'), (10, 33, b'L=33'), (11, 0, b'B=0'), (11, 65536, b'B=65536'), (12, 1, b'images of 1 x 5'),
                          (13, 1, b'images of 4 x 1'), (8, 2 * 4 * 5 - 2, b'row stride'), (8, 2 * 4 * 5 + 1, b'row stride'),
                          (6, 3, b'live_links'), (4, 0, b'P=0'), (7, ctypes.c_void_p(20), b'misaligned')):
        a = list(good)
        a[at] = bad
        assert lib.dvd_flow_chain(*a) == _lib.DVD_EINVAL, (at, bad)
        assert word in lib.dvd_last_error(), (word, lib.dvd_last_error())
    a = list(good)
    a[12], a[13], a[8] = 1 << 15, 1 << 15, 1 << 40
    assert lib.dvd_flow_chain(*a) == _lib.DVD_EINVAL and b'2^30' in lib.dvd_last_error()


# ---- the wrapper's refusals that need no device --------------------------------------------------------------------------

def test_wrapper_refuses_before_it_touches_a_device():
    from dvd_hip import ops
    f = torch.zeros(2, 4, 5, 2)
    m = torch.zeros(2, 4, 5, dtype=torch.uint8)
    links = np.array([[[0, 0], [1, 1], [-1, -1]]], np.int32)
    call = lambda **kw: ops.flow_chain(**dict(dict(flow_1_2=f, flow_2_1=f, mask_1=m, mask_2=m, links=links), **kw))
    for kw, word in ((dict(links=np.zeros((1, 33, 2), np.int32)), 'L=33'), (dict(links=np.zeros((1, 0, 2), np.int32)), 'L=0'),
                     (dict(links=np.zeros((0, 2, 2), np.int32)), 'chains per launch'), (dict(links=np.zeros((1, 2, 3), np.int32)), 'links'),
                     (dict(links=np.zeros((2, 2), np.int32)), 'links'), (dict(links=np.zeros((1, 2, 2), np.float32)), 'links'),
                     (dict(links='abc'), 'links'), (dict(), 'flow_1_2 must be a GPU tensor'),
                     (dict(flow_1_2=f.double()), 'flow_1_2 must be a GPU tensor')):
        with pytest.raises(RuntimeError, match=word):
            call(**kw)


# ---- the specification ----------------------------------------------------------------------------------------------------

H, W, N = 24, 40, 7


@pytest.fixture(scope='module')
def clean():
    """The noise-free scene, and per gap g the float64 chains of its gap-1 flows: computed once, never written to."""
    sc = T.scene(H, W, N, seed=0, noise=0.0)
    n1 = N - 1                                                           # the gap-1 pairs come first
    assert sc['pairs'][:n1] == [(a, a + 1) for a in range(n1)]
    g1 = {k: sc[k][:n1] for k in ('flow_1_2', 'flow_2_1', 'mask_1', 'mask_2')}
    runs = {}
    for g in (2, 3, 4):
        new, fwd, bwd = C.gap1_links(N, g)
        runs[g] = (new, fwd, C.chain(g1['flow_1_2'], g1['flow_2_1'], g1['mask_1'], g1['mask_2'], fwd, np.float64))
    return sc, g1, runs


def _direct(sc, new):
    rows = [sc['pairs'].index(p) for p in new]
    return sc['flow_1_2'][rows], sc['mask_2'][rows]


def _walk_stays_on(sc, new, res, fwd, inside):
    """bool [B,H,W]: every tap of every link of the (float64) walk is a pixel of `inside[frame]` -- the walk of a chain of gap-1
    flows from frame a is in frame a + k at link k."""
    B, L = fwd.shape[:2]
    vv, uu = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    on = np.ones((B, H, W), bool)
    for b, (a, _) in enumerate(new):
        for k in range(L):
            x = uu + (res['flow'][k - 1, b, ..., 0] if k else 0.0)
            y = vv + (res['flow'][k - 1, b, ..., 1] if k else 0.0)
            x0, y0 = np.clip(np.floor(x), 0, W - 1).astype(int), np.clip(np.floor(y), 0, H - 1).astype(int)
            x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
            m = inside[a + k]
            on[b] &= m[y0, x0] & m[y0, x1] & m[y1, x0] & m[y1, x1]
    return on


def test_float64_chain_of_gap_1_flows_against_the_direct_flow(clean):
    sc, _, runs = clean
    stale = []
    for g, (new, fwd, res) in runs.items():
        flow, broken = C.last_rows(res, fwd)
        direct, dmask = _direct(sc, new)
        static = np.stack([~sc['disc'][a] for a, _ in new], 0)
        whole = static & (broken == 0)
        share = whole.sum() / float(static.sum())
        where = whole & (dmask == 0)
        worst, mean = C.distance(flow, direct, where)
        print('chain of gap-1 flows to gap %d against the direct flow, static pixels: worst %.4g px, mean %.4g px over %d pixels; '
              'unbroken share of the static pixels %.3f' % (g, worst, mean, int(where.sum()), share))
        assert share >= 0.5, (g, share)                                  # otherwise the comparison is hollow
        assert where.sum() > 0.4 * static.sum()
        # A static pixel of frame a whose walk passes the disc's rim in a later frame takes a tap from the MOVING surface there:
        # that is the flow field's discontinuity, not interpolation error, and such a pixel is not static along its walk.  So
        # 'static' is asked of every tap of every link here (the same rule the disc's test applies from the other side).  A
        # static point that passes under the rim follows the disc for a link (flow_chain_spec.MEASURED_CHAIN_RIM, kept current
        # below).  What bounds THOSE pixels is the composed pair's consistency rule, which preprocess.chain_flows applies:
        # test_the_composed_masks_bound_every_static_pixel_the_rim_included asserts it on the whole population.
        off = _walk_stays_on(sc, new, res, fwd, ~sc['disc'])
        rim = where & ~off
        d = np.linalg.norm(flow.astype(np.float64) - direct, axis=-1)
        print('    of these, %d pass the rim of the disc: worst %.4g px there, %d beyond %.2f px; away from the rim: worst %.4g px, mean %.4g px'
              % (int(rim.sum()), float(d[rim].max()) if rim.any() else 0.0, int((d[rim] > WELL_BELOW).sum()), WELL_BELOW,
                 *C.distance(flow, direct, where & off)))
        assert rim.sum() <= 0.05 * where.sum(), (g, int(rim.sum()))          # (the rim is a small part of the comparison)
        if not abs(worst - C.MEASURED_CHAIN_RIM[g]) <= 0.05 * C.MEASURED_CHAIN_RIM[g]:
            stale.append((g, 'rim', worst))
        worst, mean = C.distance(flow, direct, where & off)
        assert worst <= WELL_BELOW, 'the test scene is wrong for this purpose: gap %d is %.3g px from the direct flow' % (g, worst)
        if not (worst <= 1.5 * C.MEASURED_CHAIN[g][0] and mean <= 1.5 * C.MEASURED_CHAIN[g][1]):
            stale.append((g, worst, mean))
    assert not stale, 'flow_chain_spec.MEASURED_CHAIN / MEASURED_CHAIN_RIM is out of date: measured (gap, worst, mean) %s' % stale


def test_the_composed_masks_bound_every_static_pixel_the_rim_included(clean):
    """The population of the comparison above WITHOUT the walk's rule -- static in its own frame, direct mask 0 -- and with the
    composed pair's own mask in place of `broken == 0`: what preprocess.chain_flows hands to the store as usable (the fp32
    pipeline, flow_chain_spec.chain_flows).  The rim pixels are in it unless the consistency rule of the composed pair caught
    them, and it must have: up to 3.6 px otherwise.  Both sides, each flow with the mask that belongs to it: flow_1_2 with
    mask_2 in the pair's first frame, flow_2_1 with mask_1 in its second -- with the sides swapped this fails."""
    sc, g1, _ = clean
    out = C.chain_flows(g1['flow_1_2'], g1['flow_2_1'], g1['mask_1'], g1['mask_2'], sc['pairs'][:N - 1], N, (2, 3, 4))
    rows = [sc['pairs'].index(p) for p in out['pairs']]
    for flow_key, mask_key, end in (('flow_1_2', 'mask_2', 0), ('flow_2_1', 'mask_1', 1)):
        for g in (2, 3, 4):
            sel = [i for i, (a, b) in enumerate(out['pairs']) if b - a == g]
            direct, dmask = sc[flow_key][[rows[i] for i in sel]], sc[mask_key][[rows[i] for i in sel]]
            static = np.stack([~sc['disc'][out['pairs'][i][end]] for i in sel], 0)
            where = static & (out[mask_key][sel] == 0) & (dmask == 0)
            worst, mean = C.distance(out[flow_key][sel], direct, where)
            unmasked = static & (out['broken_' + mask_key[-1]][sel] == 0) & (dmask == 0)
            print('%s of gap %d, static pixels with the composed %s and the direct one 0: worst %.4g px, mean %.4g px over a share of '
                  '%.3f of the static pixels (unbroken only: worst %.4g px)'
                  % (flow_key, g, mask_key, worst, mean, where.sum() / float(static.sum()), C.distance(out[flow_key][sel], direct, unmasked)[0]))
            assert where.sum() >= 0.4 * static.sum(), (flow_key, g)           # otherwise the comparison is hollow
            assert worst <= WELL_BELOW, (flow_key, g, worst)
            # every broken chain is masked, and nothing else but the consistency rule sets a byte
            assert (out[mask_key][sel][out['broken_' + mask_key[-1]][sel] != 0] == 1).all() and set(np.unique(out[mask_key])) <= {0, 1}


def test_a_chain_through_the_moving_disc_follows_the_disc(clean):
    sc, _, runs = clean
    for g, (new, fwd, res) in runs.items():
        flow, broken = C.last_rows(res, fwd)
        direct, dmask = _direct(sc, new)
        disc = np.stack([sc['disc'][a] for a, _ in new], 0)
        # a disc pixel whose walk samples disc pixels only: at the rim a tap takes the background's flow, which is no error of the
        # chain but the flow field's own discontinuity
        on = disc & _walk_stays_on(sc, new, res, fwd, sc['disc']) & (broken == 0) & (dmask == 0)
        worst, mean = C.distance(flow, direct, on)
        print('gap %d on the disc: worst %.4g px, mean %.4g px over %d pixels (static: %.4g)' % (g, worst, mean, int(on.sum()), C.MEASURED_CHAIN[g][0]))
        assert on.sum() >= 20 * len(new), (g, int(on.sum()))
        assert worst <= WELL_BELOW, (g, worst)
        # ... and it does follow it: the disc's flow is not the background's there
        assert float(np.abs(flow[on][:, 1]).mean()) > 1.5 * g


def test_undecided_share_of_the_noisy_scene_is_within_the_cap():
    sc = T.scene(H, W, N, seed=0, noise=0.4, gaps=(1,))
    total = undecided = 0
    for g in (2, 3, 4):
        _, fwd, bwd = C.gap1_links(N, g)
        for links in (fwd, bwd):
            dec = C.chain(sc['flow_1_2'], sc['flow_2_1'], sc['mask_1'], sc['mask_2'], links, np.float64)['decided']
            total += dec.size
            undecided += int((~dec).sum())
    print('undecided pixels: %d of %d' % (undecided, total))
    assert total == 2 * (5 + 4 + 3) * H * W
    assert undecided <= 0.01 * total


def test_hostile_input_leaves_the_flow_finite_and_broken_as_specified():
    h, w = 5, 7
    rng = np.random.default_rng(4)
    f12 = rng.normal(0, 0.3, (2, h, w, 2)).astype(np.float32)
    f21 = rng.normal(0, 0.3, (2, h, w, 2)).astype(np.float32)
    m1, m2 = np.zeros((2, h, w), np.uint8), np.zeros((2, h, w), np.uint8)
    f12[0, 0, 0] = np.nan
    f12[0, 0, 1] = (np.inf, 0)
    f12[0, 0, 2] = (1e30, -1e30)
    f12[0, 1, 1] = (3e38, 3e38)
    f12[0, 2, 3] = (1.0, 0.0)                                            # lands exactly on (4, 2), whose own flow ...
    f12[1, 2, 4] = (2.0, 2.0)                                            # ... lands exactly on the last row and column (6, 4)
    f12[0, 3, 3] = (0.0, 0.0)                                            # stays: the second link samples (3, 3) alone
    m2[1, 3, 3] = 1                                                      # ... which is masked there
    f12[0, 4, 6] = (0.0, 0.0)                                            # the corner pixel stays on the corner
    f12[1, 4, 6] = (0.0, 0.0)
    f12[0, 3, 0] = (-0.5, 0.0)                                           # leaves the image to the left
    f12[0, 1, 4] = (0.5, 0.0)                                            # half way to (5, 1), which is masked in pair 1
    m2[1, 1, 5] = 255
    links = np.array([[[0, 0], [1, 0], [1, 1]], [[0, 0], [7, 0], [1, 0]], [[0, 0], [-1, 0], [1, 0]]], np.int32)
    for dtype in (np.float32, np.float64):
        r = C.chain(f12, f21, m1, m2, links, dtype)
        assert np.isfinite(r['flow']).all(), dtype
        fl, br = r['flow'], r['broken']
        for y, x in ((0, 0), (0, 1)):                                    # a NaN, an Inf: link 0 breaks, the flow stays 0
            assert (br[:, 0, y, x] == 1).all() and (fl[:, 0, y, x] == 0).all(), (y, x)
        # 3e38 is finite, and so is 1 + 3e38: like 1e30 it is a step out of the image, which breaks the NEXT link
        assert br[:, 0, 1, 1].tolist() == [0, 2, 2] and np.isfinite(fl[:, 0, 1, 1]).all() and fl[2, 0, 1, 1, 0] > 2e38
        assert br[:, 0, 0, 2].tolist() == [0, 2, 2] and fl[1, 0, 0, 2].tolist() == fl[0, 0, 0, 2].tolist() == [dtype(np.float32(1e30)), dtype(np.float32(-1e30))]
        assert br[:, 0, 3, 0].tolist() == [0, 2, 2] and fl[2, 0, 3, 0].tolist() == [-0.5, 0.0]
        assert br[:, 0, 2, 3].tolist()[:2] == [0, 0] and fl[1, 0, 2, 3].tolist() == [3.0, 2.0]          # ON W-1, H-1 and whole
        assert br[2, 0, 2, 3] == 0                                       # ... and the third link samples (6, 4) alone, in bounds
        assert br[:, 0, 3, 3].tolist() == [0, 2, 2] and fl[2, 0, 3, 3].tolist() == [0.0, 0.0]          # the masked tap
        assert br[:, 0, 4, 6].tolist()[:2] == [0, 0]
        assert br[:, 0, 1, 4].tolist() == [0, 2, 2] and fl[2, 0, 1, 4].tolist() == [0.5, 0.0]          # a masked tap of two
        # a pair that is no pair breaks every pixel still alive at that link; a -1 ends the chain whatever follows
        assert (br[1:, 1][:, br[0, 1] == 0] == 2).all() and (br[1:, 1][:, br[0, 1] == 1] == 1).all()
        assert np.array_equal(fl[1, 1], fl[0, 1]) and np.array_equal(fl[2, 1], fl[0, 1])
        assert (br[1:, 2] == 255).all() and (fl[1:, 2] == 0).all() and np.array_equal(br[0, 2], br[0, 0])
