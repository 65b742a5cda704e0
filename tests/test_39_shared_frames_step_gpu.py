"""opt.share_frames: the depth net once per DISTINCT frame of a step (models/frame_union.py, csrc/frame_union.hip).

Expected values: tests/golden/fullstep_shared_hourglass_b4_32x48_train.npz -- ONE step of the REAL reference on the four pairs
(0,1), (1,2), (2,3), (3,4) of a 5-frame 32 x 48 video (tests/golden/make_golden_shared.py).  The reference runs its depth net
on all eight images; the shared step runs it on five (quantum 1) or on eight union rows of which three are padding (quantum 8).
Bounds: those tests/test_35_mixed_gaps_gpu.py applies to a step against its fixture -- losses rtol 1e-5, acc_reg 5e-6,
gradient norms 1.5e-3, gradient elements 1e-3 (scene-flow MLP) / 8e-3 (depth net) of max|g| on all but max(2, n / 5000)
elements, parameters after Adam within 2 lr sqrt(n) + 1e-5 |p| in norm and 3 lr + 1e-7 per element -- also where two HIP steps
are compared with one another.  Every test prints what it measured before it asserts.

Measured on MI355X when the feature was built:
  against the fixture, unshared / quantum 1 / quantum 8 alike: losses 1.6e-7 relative, acc_reg 1.4e-7, worst gradient norm 1.3e-5,
  worst gradient element 1.4e-4 (scene-flow MLP) and 3.0e-6 (depth net) of max|g|;
  shared against unshared HIP step: losses equal, depth-net gradient elements within 1.5e-6 of max|g| (warm-up: all equal);
  shared against unshared depth maps on this fixture: bitwise equal (0.0) -- the per-tensor operand scales of the chunks of 4 + 4,
  5 and 8 images came out the same powers of two here; that is not a property of the kernels and is not asserted;
  convolution work of a step, shared (quantum 1) over unshared: 0.625000 eagerly and through the kept slots' graphs.
"""
import importlib
import os

import numpy as np
import pytest
import torch

import helpers
import store_spec

pytestmark = pytest.mark.gpu

NAME = 'fullstep_shared_hourglass_b4_32x48_train'
CHAIN = [(0, 1), (1, 2), (2, 3), (3, 4)]
t35 = importlib.import_module('test_35_mixed_gaps_gpu')


@pytest.fixture(scope='module')
def gd():
    return helpers.load_golden(NAME)


# -- what a step is compared with ---------------------------------------------------------------------------------------
def _params(model):
    for prefix, net in (('depth', model.net_depth), ('sf', model.net_sceneflow)):
        for k, p in net.named_parameters():
            yield prefix + '/' + k, p


def _want_of_fixture(gd):
    names = [str(n) for n in gd['param_names']]
    return {'log': {k[4:]: float(v) for k, v in gd.items() if k.startswith('log_')},
            'grad_norms': dict(zip(names, gd['grad_norms'].tolist())),
            'param_norms_after': dict(zip(names, gd['param_norms_after'].tolist())),
            'elems': {k[2:]: (gd[k], gd['p_' + k[2:]]) for k in gd if k.startswith('g_sf/') or k.startswith('g_depth/')}}


def _want_of_model(model, log, warm=False):
    """Another HIP step as the expected value: every parameter's gradient and value, element by element."""
    want = {'log': dict(log), 'grad_norms': {}, 'param_norms_after': {}, 'elems': {}}
    for key, p in _params(model):
        frozen = p.grad is None or (warm and key.startswith('depth/'))
        want['grad_norms'][key] = 0.0 if frozen else float(p.grad.double().norm())
        want['param_norms_after'][key] = float(p.data.double().norm())
        if not frozen:
            want['elems'][key] = (p.grad.cpu().numpy().copy(), p.data.cpu().numpy().copy())
    return want


def _check(tag, model, opt, log, want):
    """The bounds of tests/test_35_mixed_gaps_gpu.py::test_mixed_step_matches_the_reference_combination."""
    params = dict(_params(model))
    measured = {'loss_rel': max(abs(log[k] - want['log'][k]) / abs(want['log'][k])
                                for k in ('loss', 'flow_loss_1_2', 'disp_loss_1_2', 'sf_loss')),
                'acc_reg_rel': abs(log['acc_reg'] - want['log']['acc_reg']) / max(abs(want['log']['acc_reg']), 1e-30)}
    norms = {k: abs(float(params[k].grad.double().norm()) - g) / g for k, g in want['grad_norms'].items() if g != 0.0}
    elems = {k: np.abs(params[k].grad.cpu().numpy() - g) / np.abs(g).max() for k, (g, _) in want['elems'].items()
             if np.abs(g).max() > 0.0}
    measured['grad_norm_worst_rel'] = max(norms.values()) if norms else 0.0
    measured['elem_worst_sf'] = max([float(e.max()) for k, e in elems.items() if k.startswith('sf/')] or [0.0])
    measured['elem_worst_depth'] = max([float(e.max()) for k, e in elems.items() if k.startswith('depth/')] or [0.0])
    print('measured parity (%s):' % tag, measured)
    for k in ('loss', 'total_loss', 'flow_loss_1_2', 'disp_loss_1_2', 'sf_loss'):
        np.testing.assert_allclose(log[k], want['log'][k], rtol=1e-5, err_msg='%s %s' % (tag, k))
    np.testing.assert_allclose(log['acc_reg'], want['log']['acc_reg'], rtol=5e-6, atol=1e-9, err_msg=tag)
    for key, p in params.items():
        if want['grad_norms'][key] == 0.0:          # warm phase: frozen depth net
            continue
        assert norms[key] < 1.5e-3, '%s: %s grad norm off by %g' % (tag, key, norms[key])
        lr = opt.lr * (opt.scene_lr_mul if key.startswith('sf/') else 1.0)
        assert abs(float(p.data.double().norm()) - want['param_norms_after'][key]) <= \
            2 * lr * p.numel() ** 0.5 + 1e-5 * want['param_norms_after'][key], (tag, key)
    for key, err in elems.items():
        sf = key.startswith('sf/')
        tol = 1e-3 if sf else 8e-3
        assert (err > tol).sum() <= max(2, err.size // 5000), '%s: %s: %d elements off (worst %.2e)' % (
            tag, key, (err > tol).sum(), err.max())
        lr = opt.lr * (opt.scene_lr_mul if sf else 1.0)
        assert np.abs(params[key].data.cpu().numpy() - want['elems'][key][1]).max() <= 3 * lr + 1e-7, (tag, key)
    return measured


def _step(model, batch, epoch):
    log = model._train_on_batch(epoch, 0, helpers.loader_batch({k: (v.clone() if torch.is_tensor(v) else v)
                                                                for k, v in batch.items()}))
    torch.cuda.synchronize()
    return log


def _video_batch(tmp, seed, gaps, pairs, n_frames=5, H=32, W=48):
    """`pairs` of the seeded video of make_golden_shared.py (random_tree draws the frames first: the same frames whatever the
    gaps; the flows of a tree with other gaps are other draws), as the pack path hands them over."""
    from dvd_hip.datasets.frame_store import frame_tables
    fx = store_spec.random_tree(n_frames, H, W, gaps, seed=seed)
    store_spec.write_tree(tmp, fx)
    fdir = os.path.join(tmp, 'frames_midas', store_spec.TRACK)
    fields = store_spec.fixture_fields(fx, frame_tables(sorted(os.path.join(fdir, f) for f in os.listdir(fdir))))
    rows = store_spec.pair_rows(fx)
    batch = store_spec.assemble(fields, [(a, b, rows[(a, b)]) for a, b in pairs])
    del batch['depth_1'], batch['depth_pred_1']
    batch['frame_id_1'] = torch.tensor([float(a) for a, _ in pairs])
    batch['frame_id_2'] = torch.tensor([float(b) for _, b in pairs])
    batch['time_step'] = torch.tensor(1.0 / n_frames, dtype=torch.float64)
    return batch


def test_the_fixture_video_is_rebuilt_here_bit_for_bit(gd, tmp_path):
    """(so the other batches of this file are drawn from the fixture's video)"""
    batch = _video_batch(str(tmp_path), int(gd['seed']) + 2, (1,), CHAIN)
    for k, v in t35._batch(gd).items():
        assert v.dtype == batch[k].dtype and torch.equal(v.reshape(batch[k].shape), batch[k]), k      # (time_step: [1] and 0-d)
    assert torch.equal(batch['img_2'][:3], batch['img_1'][1:])


# -- the step against the reference ---------------------------------------------------------------------------------------
RUNS = {}


@pytest.fixture(scope='module', autouse=True)
def _release_runs():
    yield
    RUNS.clear()            # the models of this file (their graphs and pools) do not outlive it
    import gc
    gc.collect()
    torch.cuda.empty_cache()


def _run(gd, tag, **over):
    if tag not in RUNS:
        model, opt = t35._model(gd, **over)
        log = _step(model, t35._batch(gd), int(gd['epoch']))
        RUNS[tag] = (model, opt, log, model._last['depth_1'].clone(), model._last['depth_2'].clone())
    return RUNS[tag]


@pytest.mark.parametrize('tag,over', [('off', {}), ('q1', {'share_frames': 1, 'share_quantum': 1}),
                                      ('q8', {'share_frames': 1, 'share_quantum': 8}), ('default_quantum', {'share_frames': 1})])
def test_step_matches_the_reference(gd, tag, over):
    model, opt, log, _, _ = _run(gd, tag, **over)
    _check(tag, model, opt, log, _want_of_fixture(gd))


def test_the_depth_net_runs_once_per_distinct_frame(gd):
    """The test that fails without the feature: eight images go through the depth net, whatever the batch shows."""
    off, q1, q8 = (_run(gd, tag, **over)[0] for tag, over in (('off', {}), ('q1', {'share_frames': 1, 'share_quantum': 1}),
                                                                ('q8', {'share_frames': 1, 'share_quantum': 8})))
    assert off.depth_images_last_step == 8 and off.last_union is None
    assert q1.depth_images_last_step == 5 and q1.last_union == {'U': 5, 'U_pad': 5, 'B': 4}
    assert q8.depth_images_last_step == 8 and q8.last_union == {'U': 5, 'U_pad': 8, 'B': 4}
    for m in (q1, q8):                            # per-pair tensors, as without sharing
        assert m._last['depth_1'].shape == m._last['depth_2'].shape == (4, 1, 32, 48)
        assert torch.equal(m._last['depth_2'][:3], m._last['depth_1'][1:])          # ONE depth map per frame
        pred = m._predict_on_batch(is_train=True)
        assert pred['sf_1_2'].shape == (4, 3, 32, 48)


def test_shared_and_unshared_depth_maps(gd):
    """Not bitwise equal, and not asserted beyond the fixture bounds: the matrix kernels split their fp16 operands with ONE
    power-of-two scale per tensor (csrc/dvd_split.h), so an image's result depends on its chunk-mates."""
    off = _run(gd, 'off')
    for tag, over in (('q1', {'share_frames': 1, 'share_quantum': 1}), ('q8', {'share_frames': 1, 'share_quantum': 8})):
        run = _run(gd, tag, **over)
        worst = max(float(((a - b).abs() / b.abs().clamp_min(1e-30)).max()) for a, b in ((run[3], off[3]), (run[4], off[4])))
        print('shared (%s) against unshared depth maps: largest relative difference %.3e' % (tag, worst))
        assert np.isfinite(worst)


def _conv_work(fn):
    from dvd_hip import ops
    before = ops.executed_flops()
    out = fn()
    torch.cuda.synchronize()
    after = ops.executed_flops()
    return out, sum(after[k] - before[k] for k in ops.FLOP_CLASSES if not k.startswith('mlp_'))


def test_convolution_work_is_five_eighths(gd):
    """ops' FLOP counters over one step: every convolution and weight gradient of the depth net is linear in the number of
    images, so the shared step (quantum 1) does 5/8 of the unshared step's -- eagerly (depth_graphs=0: forward, then
    forward + backward per image) and through the kept slots' graphs (a second step: replays only)."""
    batch, epoch = t35._batch(gd), int(gd['epoch'])
    for graphs in (0, 1):
        work = {}
        for tag, over in (('off', {}), ('q1', {'share_frames': 1, 'share_quantum': 1})):
            model, opt = t35._model(gd, depth_graphs=graphs, **over)
            if graphs:
                _step(model, batch, epoch)            # captures; its warm-up passes count as well
            log, work[tag] = _conv_work(lambda: _step(model, batch, epoch))
            assert np.isfinite(log['loss'])
            if not graphs:                            # (and the eager step against the reference)
                _check('%s, depth_graphs=0' % tag, model, opt, log, _want_of_fixture(gd))
        print('depth_graphs=%d: convolution work per step %.6e (unshared) %.6e (shared): ratio %.6f' % (
            graphs, work['off'], work['q1'], work['q1'] / work['off']))
        assert work['off'] > 0 and abs(work['q1'] / work['off'] - 5.0 / 8.0) < 1e-9


# -- other coverage -----------------------------------------------------------------------------------------------------
def test_a_warm_up_step(gd):
    """epoch <= warm_sf: no depth-net backward; the shared step against the unshared HIP step."""
    batch = t35._batch(gd)
    m0, opt = t35._model(gd)
    want = _want_of_model(m0, _step(m0, batch, 1), warm=True)
    for q in (1, 8):
        m1, _ = t35._model(gd, share_frames=1, share_quantum=q)
        log = _step(m1, batch, 1)
        assert m1.warm and m1.depth_images_last_step == (5 if q == 1 else 8)
        assert float(m1._flat_depth.grad.abs().max()) == 0.0
        _check('warm-up, quantum %d' % q, m1, opt, log, want)


def test_new_tail_shapes_work_and_old_ones_are_reused(gd, tmp_path):
    """depth_chunk 4, quantum 1, lr 0 (so every step runs on the same weights and can be compared with the unshared step):
    the chain (5 rows: chunks of 4 + 1), then two pairs twice (3 rows: one chunk of 3, a new shape in slot 0), then the chain
    again -- the one-image slot of the first step is still there and is replayed, not captured again."""
    seed = int(gd['seed']) + 2
    chain = t35._batch(gd)
    twice = _video_batch(str(tmp_path), seed, (1,), [(0, 1), (1, 2), (0, 1), (1, 2)])
    shared, opt = t35._model(gd, share_frames=1, share_quantum=1, depth_chunk=4, lr=0.0)
    plain, _ = t35._model(gd, depth_chunk=4, lr=0.0)
    epoch = int(gd['epoch'])
    seen = []
    for i, (batch, rows) in enumerate(((chain, 5), (twice, 3), (chain, 5))):
        want = _want_of_model(plain, _step(plain, batch, epoch))
        log = _step(shared, batch, epoch)
        assert shared.last_union['U_pad'] == rows and shared.depth_images_last_step == rows
        _check('step %d (%d union rows)' % (i, rows), shared, opt, log, want)
        seen.append({k: v for k, v in shared._depth_graphs.items() if v is not None})
    shapes = [sorted((k[1], k[2][0]) for k in s if k[0] == 'keep') for s in seen]
    print('kept slots (slot, images) per step:', shapes)
    assert shapes[0] == [(0, 4), (1, 1)] and shapes[1] == [(0, 3), (1, 1)] and shapes[2] == [(0, 4), (1, 1)]
    tail = [k for k in seen[0] if k[0] == 'keep' and k[1] == 1][0]
    assert seen[2][tail] is seen[0][tail], 'the one-image tail slot was captured again'


def test_a_mixed_gap_batch_of_the_same_video(gd, tmp_path):
    """Gaps 2, 1, 2, 1 over the fixture's frames: the step groups the pairs by gap first, the union is taken in that order."""
    pairs = [(0, 2), (1, 2), (2, 4), (2, 3)]
    batch = _video_batch(str(tmp_path), int(gd['seed']) + 2, (1, 2), pairs)
    epoch = int(gd['epoch'])
    m0, opt = t35._model(gd)
    want = _want_of_model(m0, _step(m0, batch, epoch))
    assert m0.steps_per_pair == [2, 1, 2, 1]
    for q in (1, 8):
        m1, _ = t35._model(gd, share_frames=1, share_quantum=q)
        log = _step(m1, batch, epoch)
        assert m1.steps_per_pair == [2, 1, 2, 1] and m1.last_union == {'U': 5, 'U_pad': 5 if q == 1 else 8, 'B': 4}
        _check('mixed gaps, quantum %d' % q, m1, opt, log, want)
        # exports come back in the caller's pair order: pair 1 and pair 3 show frame 2 second / first
        pred = m1._predict_on_batch(is_train=True)
        assert pred['sf_1_2'].shape == (4, 3, 32, 48)


def test_use_embedding(gd):
    """--use_embedding: the hourglass takes the frame id of every image; the union rows carry theirs (eager path)."""
    batch, epoch = t35._batch(gd), int(gd['epoch'])
    m0, opt = t35._model(gd, use_embedding=True)
    want = _want_of_model(m0, _step(m0, batch, epoch))
    for q in (1, 8):
        m1, _ = t35._model(gd, use_embedding=True, share_frames=1, share_quantum=q)
        log = _step(m1, batch, epoch)
        assert m1.depth_images_last_step == (5 if q == 1 else 8)
        _check('use_embedding, quantum %d' % q, m1, opt, log, want)


def test_ids_come_from_store_items_as_well(gd):
    """`fid_1` / `fid_2` (int64, as StoreLoader items carry them) are read before `frame_id_*`."""
    batch = t35._batch(gd)
    batch['fid_1'], batch['fid_2'] = batch['frame_id_1'].long(), batch['frame_id_2'].long()
    batch['frame_id_1'], batch['frame_id_2'] = batch['fid_1'], batch['fid_2']
    model, opt = t35._model(gd, share_frames=1, share_quantum=1)
    log = _step(model, batch, int(gd['epoch']))
    assert model.last_union == {'U': 5, 'U_pad': 5, 'B': 4}
    _check('int64 ids', model, opt, log, _want_of_fixture(gd))


def test_a_batch_without_ids_is_refused_by_name(gd):
    batch = {k: v for k, v in t35._batch(gd).items() if not k.startswith('frame_id')}
    model, _ = t35._model(gd, share_frames=1)
    with pytest.raises(ValueError, match='share_frames needs the frame id'):
        model._train_on_batch(int(gd['epoch']), 0, helpers.loader_batch(batch))
    with pytest.raises(ValueError, match='share_quantum'):
        t35._model(gd, share_frames=1, share_quantum=0)


def test_default_off(monkeypatch):
    """With opt.share_frames absent a step is the parent's: the losses of fullstep_hourglass_b2_32x48_train through the normal
    path, no union, and not one call into the union code."""
    from dvd_hip import ops, synthetic
    g2 = helpers.load_golden('fullstep_hourglass_b2_32x48_train')
    calls = []
    for name in ('UnionTables', 'union_gather', 'union_scatter', 'union_reduce'):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, (lambda real, name: lambda *a, **k: (calls.append(name), real(*a, **k))[1])(real, name))
    g2 = dict(g2, over_keys=g2.get('over_keys', np.array([])), over_vals=g2.get('over_vals', np.array([])))
    model, opt = t35._model(g2)
    assert not hasattr(opt, 'share_frames') and not hasattr(opt, 'share_quantum')
    c0 = ops.flop_counters()['gather']
    batch = synthetic.make_batch(int(g2['B']), int(g2['H']), int(g2['W']), gap=int(g2['gap']), seed=int(g2['seed']) + 2)
    log = _step(model, batch, int(g2['epoch']))
    print('default-off step:', {k: (log[k], float(g2['log_' + k])) for k in t35.LOSSES})
    for k in ('loss', 'total_loss', 'flow_loss_1_2', 'disp_loss_1_2', 'sf_loss'):
        np.testing.assert_allclose(log[k], float(g2['log_' + k]), rtol=1e-5, err_msg=k)
    np.testing.assert_allclose(log['acc_reg'], float(g2['log_acc_reg']), rtol=5e-6, atol=1e-9)
    assert model.last_union is None and model.depth_images_last_step == 2 * int(g2['B'])
    assert calls == [] and ops.flop_counters()['gather'] == c0
    # ... and the same model class with the switch on does call them
    gd = helpers.load_golden(NAME)
    m1, _ = t35._model(gd, share_frames=1)
    _step(m1, t35._batch(gd), int(gd['epoch']))
    # (the hourglass takes frame ids: the images and the ids of the union rows are two gathers)
    assert calls == ['UnionTables', 'union_gather', 'union_gather', 'union_scatter', 'union_reduce'], calls
