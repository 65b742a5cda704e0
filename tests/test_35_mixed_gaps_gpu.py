"""One optimisation step over pairs of DIFFERENT frame gaps, each integrated over its own number of Euler steps.

Expected values: tests/golden/fullstep_mixed_*.npz, combined in float64 from the REAL reference's steps on the uniform-gap
sub-batches (tests/golden/make_golden_mixed.py; the reference itself cannot run a mixed batch).  Bounds of test 1: those of
tests/test_30_full_step_gpu.py::test_train_on_batch_matches_reference for the uniform-gap hourglass fixtures; of tests 2-3:
those of test_pair_chunking_is_invisible; of test 4: those of test_two_rank_data_parallel_step_equals_single_process.  Every
test prints what it measured before it asserts."""
import ctypes
import importlib
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu

FIXTURES = ['fullstep_mixed_hourglass_b4_32x48_train', 'fullstep_mixed_hourglass_b4_32x48_warm',
            'fullstep_mixed_hourglass_b4_32x48_wsteps']
LOSSES = ('loss', 'flow_loss_1_2', 'disp_loss_1_2', 'sf_loss', 'acc_reg')


def _model(gd, **over):
    from dvd_hip.models.scene_flow_motion_field import Model
    o = dict(helpers.FULL_STEP_OPT)
    o.update(midas=False, full_logdir='/tmp')
    o.update({str(k): (bool(v) if isinstance(o.get(str(k)), bool) else float(v)) for k, v in zip(gd['over_keys'], gd['over_vals'])})
    o.update(over)
    opt = SimpleNamespace(**o)
    with warnings.catch_warnings():          # checkpoints are absent: random weights announced
        warnings.simplefilter('ignore')
        model = Model(opt, None)
    seed = int(gd['seed'])
    helpers.seeded_fill_(model.net_depth, seed)
    helpers.seeded_fill_(model.net_sceneflow, seed + 1)
    model.to(torch.device('cuda'))
    return model, opt


def _batch(gd, order=None):
    """The fixture's batch (its own, ungrouped pair order), or its pairs in `order`."""
    B = int(gd['B'])
    out = {}
    for k, v in gd.items():
        if k.startswith('in_'):
            t = torch.from_numpy(np.ascontiguousarray(v))
            if order is not None and t.dim() > 0 and t.shape[0] == B:
                t = t[list(order)].contiguous()
            out[k[3:]] = t
    return out


def _step(model, gd, batch):
    log = model._train_on_batch(int(gd['epoch']), 0, helpers.loader_batch(batch))
    torch.cuda.synchronize()
    return log


@pytest.mark.parametrize('name', FIXTURES)
def test_mixed_step_matches_the_reference_combination(name):
    """On the parent commit this fails: every pair was integrated over round(mean gap) = 2 Euler steps."""
    gd = helpers.load_golden(name)
    model, opt = _model(gd)
    log = _step(model, gd, _batch(gd))
    assert model.steps == 4 and model.steps_per_pair == [2, 1, 4, 1]
    measured = {'test': name,
                'loss_rel': max(abs(log[k] - float(gd['log_' + k])) / abs(float(gd['log_' + k]))
                                for k in ('loss', 'flow_loss_1_2', 'disp_loss_1_2', 'sf_loss')),
                'acc_reg_rel': abs(log['acc_reg'] - float(gd['log_acc_reg'])) / max(abs(float(gd['log_acc_reg'])), 1e-30)}
    names = [str(n) for n in gd['param_names']]
    want_g, want_p = dict(zip(names, gd['grad_norms'])), dict(zip(names, gd['param_norms_after']))
    norms, elems = {}, {}
    for prefix, net in (('depth', model.net_depth), ('sf', model.net_sceneflow)):
        for k, p in net.named_parameters():
            key = prefix + '/' + k
            if want_g[key] != 0.0:
                norms[key] = abs(float(p.grad.double().norm()) - want_g[key]) / want_g[key]
    for k in [k for k in gd if k.startswith('g_sf/') or k.startswith('g_depth/')]:
        prefix, pname = k.split('/', 1)
        p = dict((model.net_sceneflow if prefix == 'g_sf' else model.net_depth).named_parameters())[pname]
        elems[k] = np.abs(p.grad.cpu().numpy() - gd[k]) / np.abs(gd[k]).max()
        measured['elem_' + k] = float(elems[k].max())
    measured['grad_norm_worst_rel'] = max(norms.values())
    print('measured parity:', measured)
    assert log['size'] == opt.batch_size
    for k in ('loss', 'total_loss', 'flow_loss_1_2', 'disp_loss_1_2', 'sf_loss'):
        np.testing.assert_allclose(log[k], float(gd['log_' + k]), rtol=1e-5, err_msg=k)
    np.testing.assert_allclose(log['acc_reg'], float(gd['log_acc_reg']), rtol=5e-6, atol=1e-9)
    for prefix, net in (('depth', model.net_depth), ('sf', model.net_sceneflow)):
        for k, p in net.named_parameters():
            key = prefix + '/' + k
            if want_g[key] == 0.0:       # warm phase: frozen depth net
                assert prefix == 'depth'
                continue
            assert norms[key] < 1.5e-3, '%s grad norm off by %g' % (key, norms[key])
            lr = opt.lr * (opt.scene_lr_mul if prefix == 'sf' else 1.0)
            assert abs(float(p.data.double().norm()) - want_p[key]) <= 2 * lr * p.numel() ** 0.5 + 1e-5 * want_p[key], key
    for k, err in elems.items():
        prefix, pname = k.split('/', 1)
        p = dict((model.net_sceneflow if prefix == 'g_sf' else model.net_depth).named_parameters())[pname]
        tol = 1e-3 if prefix == 'g_sf' else 8e-3
        assert (err > tol).sum() <= max(2, err.size // 5000), '%s: %d elements off (worst %.2e)' % (k, (err > tol).sum(), err.max())
        lr = opt.lr * (opt.scene_lr_mul if prefix == 'g_sf' else 1.0)
        assert np.abs(p.data.cpu().numpy() - gd[k.replace('g_', 'p_', 1)]).max() <= 3 * lr + 1e-7, k


def _same_step(a, b, ma, mb, what):
    ga, gb = ma._flat_sf.grad, mb._flat_sf.grad
    da, db = ma._flat_depth.grad, mb._flat_depth.grad
    print(what, {k: abs(a[k] - b[k]) / max(abs(a[k]), 1e-30) for k in LOSSES},
          'sf grad %.2e, depth grad %.2e of max|g|' % (float((ga - gb).abs().max() / ga.abs().max()),
                                                       float((da - db).abs().max() / da.abs().max().clamp_min(1e-30))))
    for k in LOSSES:
        np.testing.assert_allclose(a[k], b[k], rtol=1e-5, atol=1e-9, err_msg=k)
    assert float((ga - gb).abs().max()) <= 1e-4 * float(ga.abs().max())
    assert float((da - db).abs().max()) <= 1e-4 * float(da.abs().max())


@pytest.mark.parametrize('name', ['fullstep_mixed_hourglass_b4_32x48_train', 'fullstep_mixed_hourglass_b4_32x48_wsteps'])
@pytest.mark.parametrize('whole_gb,recompute', [(160.0, 1), (0.0, 1), (0.0, 0)])
def test_the_three_schedules_agree_on_a_mixed_batch(whole_gb, recompute, name):
    gd = helpers.load_golden(name)
    m1, _ = _model(gd)
    m2, _ = _model(gd, mlp_stash_gb=1e-6, depth_chunk=1, mlp_whole_batch_gb=whole_gb, mlp_recompute=recompute)
    a, b = _step(m1, gd, _batch(gd)), _step(m2, gd, _batch(gd))
    # one pair per chunk, and no chunk across a gap group (grouped order: gaps 1, 1, 2, 4)
    assert m2._last_chunks == [(0, 1, 1), (1, 2, 1), (2, 3, 2), (3, 4, 4)]
    assert m1._last_chunks == [(0, 2, 1), (2, 3, 2), (3, 4, 4)]
    _same_step(a, b, m1, m2, 'schedule whole_gb=%g recompute=%d:' % (whole_gb, recompute))


def test_pair_order_does_not_matter_and_exports_keep_the_callers_order():
    gd = helpers.load_golden('fullstep_mixed_hourglass_b4_32x48_train')
    orders = {'fixture': [0, 1, 2, 3], 'grouped': [1, 3, 0, 2], 'reversed': [3, 2, 1, 0]}
    runs = {}
    for tag, order in orders.items():
        model, _ = _model(gd)
        batch = _batch(gd, order)
        kept = {k: v.clone() for k, v in batch.items()}
        given = helpers.loader_batch(batch)
        log = model._train_on_batch(int(gd['epoch']), 0, given)
        torch.cuda.synchronize()
        assert model.steps_per_pair == [[2, 1, 4, 1][b] for b in order]
        for k, v in kept.items():               # the caller's batch (stripped of the loader dimension) is not reordered
            assert torch.equal(given[k].cpu(), v), k
        pred = {k: v.cpu() for k, v in model._predict_on_batch(is_train=True).items()}
        out = model.pack_output({k: v.numpy() for k, v in pred.items()}, batch)
        np.testing.assert_array_equal(out['flow_1_2'], kept['flow_1_2'].numpy())
        runs[tag] = (log, model, pred)
    a, ma, pa = runs['fixture']
    for tag in ('grouped', 'reversed'):
        b, mb, pb = runs[tag]
        _same_step(a, b, ma, mb, 'order %s:' % tag)
        worst = 0.0
        for k, v in pa.items():
            # pair j of this run is pair order[j] of the fixture-order run
            want = v[orders[tag]]
            err = float((pb[k] - want).abs().max()) / max(float(want.abs().max()), 1e-30)
            worst = max(worst, err)
            assert err <= 1e-4, (tag, k, err)
        print('order %s: exported pred tensors differ by at most %.2e of their maximum' % (tag, worst))


@pytest.mark.timeout(600)
def test_one_process_equals_two_ranks_that_hold_one_gap_each():
    """The four pairs that the two ranks of test_30's 'mixed_gap' mode hold (two at gap 1, two at gap 2, same seeds), in ONE
    process: the mixed step equals the two-rank step."""
    from dvd_hip import synthetic
    t30 = importlib.import_module('test_30_full_step_gpu')
    name = 'fullstep_hourglass_b2_32x48_train'
    gd = helpers.load_golden(name)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model, opt, _ = t30._build(gd)
    shards = [synthetic.make_batch(2, int(gd['H']), int(gd['W']), gap=1 + r, seed=99 + r) for r in range(2)]
    batch = {k: (torch.cat([s[k] for s in shards], 0) if shards[0][k].dim() > 0 else shards[0][k]) for k in shards[0]}
    ref = model._train_on_batch(int(gd['epoch']), 0, helpers.loader_batch(batch))
    torch.cuda.synchronize()
    assert model.steps_per_pair == [1, 1, 2, 2] and model.steps == 2
    ref_sf, ref_depth, ref_g = (model._flat_sf.flat.cpu().numpy(), model._flat_depth.flat.cpu().numpy(),
                                model._flat_sf.grad.cpu().numpy())
    res = t30._run_two_ranks(name, 'mixed_gap')
    for rank, log, sf, depth, g in res:
        print('rank %d:' % rank, {k: abs(log[k] - ref[k]) / max(abs(ref[k]), 1e-30) for k in LOSSES},
              'sf grad %.2e of max|g|' % (np.abs(g - ref_g).max() / np.abs(ref_g).max()))
    for rank, log, sf, depth, g in res:
        for k in LOSSES:
            np.testing.assert_allclose(log[k], ref[k], rtol=1e-5, atol=1e-9, err_msg='rank %d %s' % (rank, k))
        assert np.abs(g - ref_g).max() <= 2e-4 * np.abs(ref_g).max()
        assert np.abs(sf - ref_sf).max() <= 2.5 * opt.lr * opt.scene_lr_mul          # Adam's first step is ~lr*sign(g)
        assert np.abs(depth - ref_depth).max() <= 2.5 * opt.lr


def test_nothing_of_a_mixed_plan_is_left_behind():
    from dvd_hip import ops, synthetic
    gd = helpers.load_golden('fullstep_mixed_hourglass_b4_32x48_train')
    uniform = synthetic.make_batch(4, 32, 48, gap=2, seed=int(gd['seed']) + 2)
    fresh, _ = _model(gd)
    _step(fresh, gd, dict(uniform))
    model, _ = _model(gd)
    c0 = ops.flop_counters()['gather']
    _step(model, gd, _batch(gd))
    c1 = ops.flop_counters()['gather']
    assert c1 > c0, 'the mixed step in fixture order did not launch dvd_gather_pairs'
    assert model.steps == 4 and model.steps_per_pair == [2, 1, 4, 1] and len(model._last_chunks) == 3
    log = _step(model, gd, dict(uniform))
    c2 = ops.flop_counters()['gather']
    print('gather bytes: mixed step %.0f, uniform step after it %.0f; chunks %s' % (c1 - c0, c2 - c1, model._last_chunks))
    assert isinstance(model.steps, int) and model.steps == 2
    assert model.steps_per_pair == [2, 2, 2, 2]
    assert model._last_chunks == fresh._last_chunks == [(0, 4, 2)]
    assert model._inv_perm is None
    assert c2 == c1, 'a uniform step launched dvd_gather_pairs'
    assert np.isfinite(log['loss'])


def test_a_pair_without_a_frame_gap_is_rejected_by_name():
    gd = helpers.load_golden('fullstep_mixed_hourglass_b4_32x48_train')
    model, _ = _model(gd)
    batch = _batch(gd)
    batch['time_stamp_2'][2] = batch['time_stamp_1'][2]
    with pytest.raises(ValueError, match='pair 2'):
        model._train_on_batch(int(gd['epoch']), 0, helpers.loader_batch(batch))


def test_the_feeder_can_stage_a_mixed_batch_in_grouped_order():
    """Host batches: DeviceFeeder(group_gaps=True) sorts while it fills the pinned buffers; the model finds the batch grouped
    and launches no permutation, and the step is the one of the fixture order."""
    from dvd_hip import ops
    from dvd_hip.datasets.davis_sequence import DeviceFeeder
    gd = helpers.load_golden('fullstep_mixed_hourglass_b4_32x48_train')
    m1, _ = _model(gd)
    a = _step(m1, gd, _batch(gd))
    host = helpers.loader_batch(_batch(gd))
    host['pair_path'] = [('p%d' % b,) for b in range(4)]
    staged = list(DeviceFeeder([host], 'cuda', group_gaps=True))
    assert len(staged) == 1 and staged[0]['pair_path'] == [('p1',), ('p3',), ('p0',), ('p2',)]
    assert torch.equal(staged[0]['img_1'][0].cpu(), host['img_1'][0][[1, 3, 0, 2]])
    assert torch.equal(staged[0]['t_2'][0].cpu(), host['t_2'][0][[1, 3, 0, 2]])
    m2, _ = _model(gd)
    c0 = ops.flop_counters()['gather']
    b = m2._train_on_batch(int(gd['epoch']), 0, dict(staged[0]))
    torch.cuda.synchronize()
    assert ops.flop_counters()['gather'] == c0 and m2.steps_per_pair == [1, 1, 2, 4]
    _same_step(a, b, m1, m2, 'feeder-grouped batch:')
    plain = list(DeviceFeeder([host], 'cuda'))[0]                  # the default leaves the order alone
    assert torch.equal(plain['img_1'].cpu(), host['img_1']) and plain['pair_path'] == host['pair_path']


def test_gather_pairs_equals_index_select_exactly():
    from dvd_hip import _lib, ops
    dev = torch.device('cuda')
    g = torch.Generator().manual_seed(7)
    for B in (5, 1):
        tensors = [torch.randn(B, 3, 32, 48, generator=g),                    # 16-byte aligned planes
                   torch.randn(B, 1, 1, 1, 3, generator=g),                   # 12 bytes per pair (t_1)
                   torch.randn(B, 7, 11, generator=g),                        # odd-sized: 308 bytes per pair, dword path
                   torch.randint(0, 255, (B, 13), generator=g, dtype=torch.uint8),    # 13 bytes per pair, byte path
                   torch.randn(B, 5000, generator=g),                         # more than one 16 KB tile per pair
                   torch.randn(B, generator=g),                               # frame ids
                   torch.randint(0, 1000, (B, 3, 3), generator=g, dtype=torch.int64)]
        tensors = [t.to(dev) for t in tensors]
        perm = torch.randperm(B, generator=g)
        out = ops.gather_pairs(tensors, perm.to(dev))
        torch.cuda.synchronize()
        for t, o in zip(tensors, out):
            assert o.dtype == t.dtype and o.shape == t.shape
            assert torch.equal(o, torch.index_select(t, 0, perm.to(dev))), (B, tuple(t.shape))
        # the identity, and a permutation followed by its inverse
        for t, o in zip(tensors, ops.gather_pairs(tensors, list(range(B)))):
            assert torch.equal(o, t)
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(B)
        for t, o in zip(tensors, ops.gather_pairs(out, inv.to(dev).to(torch.int32))):
            assert torch.equal(o, t)
    # more tensors than one launch takes: the binding splits the table
    many = [torch.randn(3, 4 + i, device=dev) for i in range(40)]
    for t, o in zip(many, ops.gather_pairs(many, [2, 0, 1])):
        assert torch.equal(o, t[[2, 0, 1]])
    # argument checks on the host side of the ABI: nothing is launched
    lib = _lib.load()
    a, b = torch.zeros(4, 8, device=dev), torch.zeros(4, 8, device=dev)
    pd = torch.arange(4, dtype=torch.int32, device=dev)
    items = (_lib.GatherItem * 33)()
    for it in items:
        it.src, it.dst, it.bytes_per_pair = a.data_ptr(), b.data_ptr(), 32
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    before = ops.flop_counters()['gather']
    assert lib.dvd_gather_pairs(items, 33, ctypes.c_void_p(pd.data_ptr()), 4, stream) == _lib.DVD_EINVAL
    items[0].dst = a.data_ptr()
    assert lib.dvd_gather_pairs(items, 1, ctypes.c_void_p(pd.data_ptr()), 4, stream) == _lib.DVD_EINVAL      # src == dst
    assert b'overlap' in lib.dvd_last_error()
    items[0].dst = a.data_ptr() + 32
    assert lib.dvd_gather_pairs(items, 1, ctypes.c_void_p(pd.data_ptr()), 4, stream) == _lib.DVD_EINVAL      # overlapping ranges
    assert ops.flop_counters()['gather'] == before
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ops.gather_pairs([torch.zeros(2, 2)], [0, 1])
