"""preprocess.chain_flows and FrameStore.add_pairs (dvd_hip/preprocess.py, datasets/frame_store.py, csrc/flow_chain.hip).

The store is built the way tests/test_62_triangulate_depth_gpu.py builds its own -- a tree of frame and flow files written by
tests/store_spec.py, read back by Catalogue / FrameStore -- from triangulate_spec.scene(24, 40, 7, noise=0.4, gaps=(1,)): the
gap-1 pairs alone, flows with 0.4 px of noise, consistency masks.

Exact: chain_flows is the specification's pipeline (flow_chain_spec.chain_flows), bit for bit, for any `chunk`; after add_pairs
the loader's items are store_spec.assemble of the grown tensors, and a store that never calls it gives the triangulation the
specification gives for the gap-1 pairs.  Ordered, not bounded: with the chained gaps 2 to 4 the triangulated depth of the
static pixels is closer to the true depth than from the gap-1 pairs alone (both errors are printed).
"""
import numpy as np
import pytest
import torch

import flow_chain_spec as C
import helpers
import store_spec
import triangulate_spec as T

pytestmark = pytest.mark.gpu

DEV = 'cuda'
H, W, N = 24, 40, 7
CHAINED = (2, 3, 4)
PAIR_KEYS = ('flow_1_2', 'flow_2_1', 'mask_1', 'mask_2')
KEYS = PAIR_KEYS + ('broken_1', 'broken_2', 'n_links')
TRI_KEYS = ('depth', 'count', 'usable', 'epi', 'spread')


def _tree(sc, seed=5):
    rng = np.random.default_rng(seed)
    return {'gaps': np.array([1]), 'fr_img': rng.random((N, H, W, 3)).astype(np.float32),
            'fr_depth_pred': sc['depth'].astype(np.float32), 'fr_depth_mvs': sc['depth'].astype(np.float32),
            'fr_pose_c2w': sc['poses'], 'fr_intrinsics': sc['intrinsics'], 'fl_ids': np.array(sc['pairs']),
            'fl_flow_1_2': sc['flow_1_2'], 'fl_flow_2_1': sc['flow_2_1'], 'fl_mask_1': sc['mask_1'], 'fl_mask_2': sc['mask_2']}


def _store(tmp, sc):
    from dvd_hip.datasets.frame_store import Catalogue, FrameStore
    store_spec.write_tree(str(tmp), _tree(sc))
    return FrameStore(Catalogue(str(tmp), store_spec.TRACK, [1], all_pairs=True), DEV)


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(got, want, keys, what=''):
    for k in keys:
        assert tuple(got[k].shape) == tuple(want[k].shape), (what, k, tuple(got[k].shape), tuple(want[k].shape))
        assert _bits(got[k]).dtype == _bits(want[k]).dtype, (what, k)
        diff = _bits(got[k]) != _bits(want[k])
        assert not diff.any(), (what, k, int(diff.sum()))


class _Ctx(object):
    pass


@pytest.fixture(scope='module')
def ctx(tmp_path_factory):
    """The scene, the gap-1 store and what it gives BEFORE anything is added (read-only), a second store of the same files that
    the chained pairs are added to, and the specification's pipeline: computed once, shared."""
    from dvd_hip import preprocess
    c = _Ctx()
    c.sc = T.scene(H, W, N, seed=0, noise=0.4, gaps=(1,))
    c.plain = _store(tmp_path_factory.mktemp('plain'), c.sc)
    c.store = _store(tmp_path_factory.mktemp('chained'), c.sc)
    assert c.store.cat.pairs == c.sc['pairs'] == [(a, a + 1) for a in range(N - 1)]
    c.tri_plain = preprocess.triangulate_depth(c.plain)
    c.early = c.store.loader(4)                                          # a loader made BEFORE the pairs are added
    c.early_len = len(c.early)
    c.nbytes = c.store.nbytes
    c.chained = preprocess.chain_flows(c.store, CHAINED)
    c.spec = C.chain_flows(c.sc['flow_1_2'], c.sc['flow_2_1'], c.sc['mask_1'], c.sc['mask_2'], c.sc['pairs'], N, CHAINED)
    c.store.add_pairs(c.chained)
    c.tri = preprocess.triangulate_depth(c.store)
    torch.cuda.synchronize()
    return c


def test_chain_flows_is_the_specifications_pipeline_for_any_chunk(ctx):
    from dvd_hip import preprocess
    got, want = ctx.chained, ctx.spec
    assert set(got) == set(KEYS) | {'pairs'}
    assert got['pairs'] == want['pairs'] == [(a, a + g) for g in CHAINED for a in range(N - g)]
    assert all(got[k].is_cuda for k in KEYS) and got['n_links'].tolist() == [g for g in CHAINED for _ in range(N - g)]
    assert got['flow_1_2'].dtype == torch.float32 and got['mask_1'].dtype == got['broken_2'].dtype == torch.uint8
    _same(got, want, KEYS, 'one launch')
    assert torch.isfinite(got['flow_1_2']).all() and torch.isfinite(got['flow_2_1']).all()
    # the masks are 0 / 1 and hold every broken chain.  (0.4 px of noise sets a fifth of the gap-1 masks, a link reads up to four
    # taps, and a chain has up to four links: three quarters of the chains break, and a tenth of the pixels stays usable.)
    for side in ('1', '2'):
        m, b = got['mask_' + side], got['broken_' + side]
        assert int(m.max()) == 1 and bool((m[b != 0] == 1).all()) and 0.3 < float((b != 0).float().mean()) < 0.9
        assert 0.05 < float((m == 0).float().mean()) < 0.3
    for chunk in (1, 5, 100):
        _same(preprocess.chain_flows(ctx.plain, CHAINED, chunk=chunk), want, KEYS, chunk)
    _same(preprocess.chain_flows(ctx.plain, [3], base=[1]), C.chain_flows(*(ctx.sc[k] for k in PAIR_KEYS), ctx.sc['pairs'], N, [3], base=[1]),
          KEYS, 'base')
    for kw in (dict(chunk=0), dict(chunk=1.5)):
        with pytest.raises(ValueError, match='chain_flows'):
            preprocess.chain_flows(ctx.plain, CHAINED, **kw)
    with pytest.raises(ValueError, match='chain_flows|chain_plan'):
        preprocess.chain_flows(ctx.plain, [1])
    with pytest.raises(ValueError, match=r'pair \(0, 2\) cannot be reached'):
        preprocess.chain_flows(ctx.plain, [2], base=[2])


def test_add_pairs_grows_the_catalogue_and_the_store(ctx):
    s, cat, n = ctx.store, ctx.store.cat, len(ctx.spec['pairs'])
    assert cat.pairs == ctx.sc['pairs'] + ctx.spec['pairs'] and cat.gaps == [1, 2, 3, 4]
    assert len(cat.pair_files) == len(cat.pairs) and cat.pair_files[N - 1:] == [None] * n and all(cat.pair_files[:N - 1])
    assert s.nbytes == ctx.nbytes + n * (4 * H * W * 4 + 2 * H * W)
    for k in PAIR_KEYS:
        t = getattr(s, k)
        assert t.shape[0] == N - 1 + n and t.is_contiguous()
        assert torch.equal(t[:N - 1], getattr(ctx.plain, k)) and np.array_equal(_bits(t[N - 1:]), _bits(ctx.spec[k])), k
    # a second add of the same pairs is refused, whole or in part, and so is what is no set of pairs of this store
    with pytest.raises(RuntimeError, match=r'holds the pair \(0, 2\) already'):
        s.add_pairs(ctx.chained)
    one = {k: (v[:1] if torch.is_tensor(v) else v[:1]) for k, v in ctx.chained.items()}
    for bad, word in ((dict(one, pairs=[(0, 1)]), 'already'), (dict(one, pairs=[(0, N)]), 'no forward pair'), (dict(one, pairs=[(3, 3)]), 'no forward pair'),
                      (dict(one, pairs=[(0, 5), (0, 5)], **{k: ctx.chained[k][:2] for k in PAIR_KEYS}), 'already'),
                      (dict(one, pairs=[(0, 5)], flow_1_2=one['flow_1_2'].cpu()), 'flow_1_2'), (dict(one, pairs=[(0, 5)], mask_2=one['mask_2'].float()), 'mask_2'),
                      (dict(one, pairs=[(0, 5)], flow_2_1=ctx.chained['flow_2_1'][:2]), 'flow_2_1'), ({'pairs': [(0, 5)]}, 'expected a dict'),
                      (dict(one, pairs=[]), 'no pair')):
        with pytest.raises(RuntimeError, match=word):
            s.add_pairs(bad)
    assert len(cat.pairs) == N - 1 + n and s.flow_1_2.shape[0] == N - 1 + n                  # a refusal changes nothing
    # the budget check is repeated
    from dvd_hip.datasets.frame_store import Catalogue, FrameStore
    tight = FrameStore(Catalogue(ctx.plain.cat.root, store_spec.TRACK, [1], all_pairs=True), DEV, budget_gb=(ctx.nbytes + 1000) / 2 ** 30)
    with pytest.raises(RuntimeError, match='store_gb'):
        tight.add_pairs(ctx.chained)
    assert len(tight.cat.pairs) == N - 1


def test_the_loader_yields_chained_pairs_like_stored_ones(ctx):
    s = ctx.store
    fields = {k: (v.cpu() if v is not None else None) for k, v in s.fields().items()}
    loader = s.loader(4)
    steps = s.cat.steps(4, 0)
    assert len(loader) == len(steps) == -(-len(s.cat.pairs) // 4)
    seen = 0
    for item, step in zip(loader, steps):
        want = store_spec.assemble(fields, step)
        for k, v in want.items():
            assert torch.equal(item[k][0].cpu(), v), k
        for i, (a, b, p) in enumerate(step):
            if p >= N - 1:                                               # a chained pair: the chained tensors themselves
                seen += 1
                assert (a, b) == ctx.spec['pairs'][p - (N - 1)] and item['pair_path'][i] == (None,)
                assert np.array_equal(_bits(item['flow_1_2'][0, i]), _bits(ctx.spec['flow_1_2'][p - (N - 1)]))
                assert np.array_equal(item['mask_2'][0, i, :, :, 0, 0].cpu().numpy(), 1.0 - ctx.spec['mask_2'][p - (N - 1)])
    assert seen == len(ctx.spec['pairs'])
    # a loader made before add_pairs keeps drawing from the pairs it saw: the same steps as a store that never added any
    assert len(ctx.early) == ctx.early_len == len(ctx.plain.loader(4)) == 2
    for a, b in zip(ctx.early, ctx.plain.loader(4)):
        name = lambda item: [p[0] and p[0].rsplit('/', 1)[-1] for p in item['pair_path']]        # (the two trees differ in their root)
        assert name(a) == name(b) and all(name(a))
        for k in ('flow_1_2', 'mask_1', 'img_2', 'fid_1', 'fid_2'):
            assert torch.equal(a[k], b[k]), k


def test_triangulation_sees_the_chained_pairs_and_gets_closer_to_the_truth(ctx):
    from dvd_hip import preprocess
    # a store that never calls add_pairs gives what the specification gives for the gap-1 pairs: today's bits
    tab = {k: v.numpy() for k, v in ctx.plain.host_tables.items()}
    want = T.pipeline(*(ctx.sc[k] for k in PAIR_KEYS), T.plan(ctx.sc['pairs'], range(N)), range(N), tab, 'median', np.float32)
    _same(ctx.tri_plain, want, TRI_KEYS, 'gap 1 only')
    _same(preprocess.triangulate_depth(ctx.plain), ctx.tri_plain, TRI_KEYS, 'again')
    # ... and the grown store what it gives for all of its pairs
    grown = {k: np.concatenate([ctx.sc[k], ctx.spec[k]], 0) for k in PAIR_KEYS}
    pairs = ctx.sc['pairs'] + ctx.spec['pairs']
    _same(ctx.tri, T.pipeline(*(grown[k] for k in PAIR_KEYS), T.plan(pairs, range(N)), range(N), tab, 'median', np.float32), TRI_KEYS, 'grown')
    # observations: 2 per interior frame from the gap-1 pairs; with gaps 1 to 4 every pair of the 7 frames that holds the frame,
    # 4 on the end frames and 6 on frames 2 to 4 (8 in a video long enough to have four frames on either side)
    assert int(ctx.tri_plain['usable'].max()) == 2
    rows = [int((r[:, 0] >= 0).sum()) for r in T.plan(pairs, range(N))]
    per_frame = [int(ctx.tri['usable'][f].max()) for f in range(N)]
    print('usable observations per frame at most:', per_frame, 'of', rows)
    assert rows == [4, 5, 6, 6, 6, 5, 4] and max(per_frame) == 6 and all(4 <= u <= r for u, r in zip(per_frame, rows))
    # on static pixels the depth is closer to the truth
    true = helpers.t(ctx.sc['depth'].astype(np.float32), DEV)[:, None]
    static = ~helpers.t(ctx.sc['disc'], DEV)[:, None]
    err = {}
    for name, tri in (('gap 1 only', ctx.tri_plain), ('with chained gaps 2-4', ctx.tri)):
        ok = static & (tri['depth'] > 0)
        rel = ((tri['depth'] / true - 1).abs())[ok]
        err[name] = (float(rel.mean()), float(rel.median()), float(ok.float().mean()))
        print('triangulated depth against the true depth on static pixels, %s: mean %.4g, median %.4g relative over a share of %.3f'
              % ((name,) + err[name]))
    assert err['with chained gaps 2-4'][0] < err['gap 1 only'][0] and err['with chained gaps 2-4'][1] < err['gap 1 only'][1]
    assert err['with chained gaps 2-4'][2] >= err['gap 1 only'][2] > 0.3
