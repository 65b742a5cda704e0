"""MiDaS at a working resolution in a full optimisation step: the reference's dataset-name rule against a fixture of the REAL
reference (tests/golden/make_golden_resize.py: opt.dataset = 'cube_synthetic', 120 x 200 frames through MidasNet(resize=[224,
384])), and the explicit switch opt.midas_resize.

Bounds of the fixture case = those tests/test_30_full_step_gpu.py applies to fullstep_midas_b2_192x384_train:

  quantity                                   measured on MI355X   bound     1 vs 8 CPU threads of the reference
  logged losses (rel)                        1.8e-6               1e-5      1.1e-7
  acc_reg (rel)                              1.4e-7               5e-6      1.4e-7
  per-parameter gradient norms (rel)         5.9e-4               1.5e-3    2.9e-4
  MLP gradient elements / max|g|             2.0e-4               1e-3      8.2e-5
  depth-net gradient elements / max|g|       1.6e-3               8e-3      1.3e-3

The last column is the reference against itself (make_golden_resize.py --spread): every entry is below a third of its bound, so
the case is well conditioned (seeds 167, 179, 181 and 193 of the same construction are not, and were passed over).
"""
import os
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu

FIXTURE = 'fullstep_midas_b1_120x200_cube_train'
LOG_KEYS = ('loss', 'flow_loss_1_2', 'disp_loss_1_2', 'sf_loss')


def _build(seed, B, H, W, gap=1, **over):
    from dvd_hip import synthetic
    from dvd_hip.models.scene_flow_motion_field import Model
    o = dict(helpers.FULL_STEP_OPT)
    o.update(midas=True, full_logdir=tempfile.mkdtemp())
    o.update(over)
    opt = SimpleNamespace(**o)
    with pytest.warns(UserWarning):          # checkpoints are absent: random weights announced
        model = Model(opt, None)
    helpers.seeded_fill_(model.net_depth, seed)
    helpers.seeded_fill_(model.net_sceneflow, seed + 1)
    with torch.no_grad():
        model.net_depth.scratch.output_conv[4].weight.mul_(30.0)
        model.net_depth.scratch.output_conv[4].bias.fill_(2000.0)
    model.to(torch.device('cuda'))
    return model, opt, synthetic.make_batch(B, H, W, gap=gap, seed=seed + 2)


def test_dataset_name_rule_matches_the_reference_step():
    gd = helpers.load_golden(FIXTURE)
    over = {str(k): str(v) for k, v in zip(gd['over_keys'], gd['over_vals'])}
    assert over == {'dataset': 'cube_synthetic'}
    model, opt, batch = _build(int(gd['seed']), int(gd['B']), int(gd['H']), int(gd['W']), int(gd['gap']), **over)
    assert list(model.net_depth.resize) == [224, 384] and model._depth.resize == (224, 384)
    log = model._train_on_batch(int(gd['epoch']), 0, helpers.loader_batch(batch))
    torch.cuda.synchronize()
    measured = {'test': FIXTURE,
                'loss_rel': max(abs(log[k] - float(gd['log_' + k])) / abs(float(gd['log_' + k])) for k in LOG_KEYS),
                'acc_reg_rel': abs(log['acc_reg'] - float(gd['log_acc_reg'])) / max(abs(float(gd['log_acc_reg'])), 1e-30)}
    names = [str(n) for n in gd['param_names']]
    want_g, want_p = dict(zip(names, gd['grad_norms'])), dict(zip(names, gd['param_norms_after']))
    worst, worst_k, failures = 0.0, None, []
    for prefix, net in (('depth', model.net_depth), ('sf', model.net_sceneflow)):
        lr = opt.lr * (opt.scene_lr_mul if prefix == 'sf' else 1.0)
        for k, p in net.named_parameters():
            key = prefix + '/' + k
            if want_g[key] == 0.0:       # refinenet4.resConfUnit1 is never used (third_party/MiDaS.py:234)
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, key
                continue
            rel = abs(float(p.grad.double().norm()) - want_g[key]) / want_g[key]
            if rel > worst:
                worst, worst_k = rel, key
            if not abs(float(p.data.double().norm()) - want_p[key]) <= 2 * lr * p.numel() ** 0.5 + 1e-5 * want_p[key]:
                failures.append('parameter norm after the step: ' + key)
    measured['grad_norm_worst_rel'] = worst
    for k in [k for k in gd if k.startswith('g_sf/') or k.startswith('g_depth/')]:
        prefix, pname = k.split('/', 1)
        p = dict((model.net_sceneflow if prefix == 'g_sf' else model.net_depth).named_parameters())[pname]
        want = gd[k]
        err = np.abs(p.grad.cpu().numpy() - want) / np.abs(want).max()
        tol = 1e-3 if prefix == 'g_sf' else 8e-3
        measured['elem_' + k] = float(err.max())
        if (err > tol).sum() > max(2, want.size // 5000):
            failures.append('%s: %d elements off (worst %.2e)' % (k, (err > tol).sum(), err.max()))
        lr = opt.lr * (opt.scene_lr_mul if prefix == 'g_sf' else 1.0)
        if not np.abs(p.data.cpu().numpy() - gd[k.replace('g_', 'p_', 1)]).max() <= 3 * lr + 1e-7:
            failures.append('parameters after the step: ' + k)
    print('measured parity:', measured, 'worst gradient norm:', worst_k)
    helpers.log_measured(FIXTURE + '/loss_rel', measured['loss_rel'], 1e-5)
    helpers.log_measured(FIXTURE + '/acc_reg_rel', measured['acc_reg_rel'], 5e-6)
    helpers.log_measured(FIXTURE + '/grad_norm_worst_rel', worst, 1.5e-3)
    for k, v in measured.items():
        if k.startswith('elem_'):
            helpers.log_measured(FIXTURE + '/' + k, v, 1e-3 if k.startswith('elem_g_sf') else 8e-3)
    assert log['size'] == opt.batch_size
    for k in LOG_KEYS + ('total_loss',):
        np.testing.assert_allclose(log[k], float(gd['log_' + k]), rtol=1e-5, err_msg=k)
    np.testing.assert_allclose(log['acc_reg'], float(gd['log_acc_reg']), rtol=5e-6, atol=1e-9)
    assert worst < 1.5e-3, '%s: gradient norm off by %.3e' % (worst_k, worst)
    assert not failures, '\n'.join(failures)


def test_explicit_switch_with_graphs_equals_eager_and_overrides_the_dataset_rule():
    """opt.midas_resize = (64, 96) on 48 x 80 frames, under a dataset name whose rule would say [224, 384]: one step through
    captured graphs equals the step with --depth_graphs 0 (test_30's graph-versus-eager bound with this package's deterministic
    kernels: logs 1e-5 relative, depth-net gradient 2e-3 of max|g|), and inference returns depth at the frame size."""
    runs = []
    for graphs in (1, 0):
        model, opt, batch = _build(223, 1, 48, 80, dataset='cube_synthetic', midas_resize=(64, 96), depth_graphs=graphs,
                                   depth_chunk=1)
        assert list(model.net_depth.resize) == [64, 96] and model._depth.resize == (64, 96)
        log = model._train_on_batch(6, 0, helpers.loader_batch(dict(batch)))
        torch.cuda.synchronize()
        live = sorted(k[0] for k, v in model._depth_graphs.items() if v is not None)
        assert live == (['keep', 'keep'] if graphs else []), live
        runs.append((log, model._flat_depth.grad.clone(), model, batch))
    (la, ga, model, batch), (lb, gb, _, _) = runs
    for k in ('loss', 'flow_loss_1_2', 'disp_loss_1_2', 'sf_loss', 'acc_reg'):
        assert np.isfinite(la[k])
        np.testing.assert_allclose(la[k], lb[k], rtol=1e-5, atol=1e-9, err_msg=k)
    assert float(gb.abs().max()) > 0.0
    rel = float((ga - gb).abs().max() / gb.abs().max())
    helpers.log_measured('midas_resize_graph_vs_eager', rel, 2e-3)
    print('graph vs eager: %.3e of max|g|' % rel)
    assert rel <= 2e-3
    # a second step replays only; then inference on the same model: 48 x 80 depth
    assert np.isfinite(model._train_on_batch(6, 1, helpers.loader_batch(dict(batch)))['loss'])
    model.opt.output_dir, model.opt.epoch = tempfile.mkdtemp(), 7
    test_batch = {'img': batch['img_1'], 'R_1': batch['R_1'], 't_1': batch['t_1'], 'K_inv': batch['K_inv'],
                  'time_stamp_1': batch['time_stamp_1'], 'frame_id_1': batch['frame_id_1'], 'pair_path': ['a']}
    pred = model.test_on_batch(0, test_batch)
    assert pred['depth'].shape == (1, 1, 48, 80) and np.isfinite(pred['depth']).all()
    assert os.path.exists(os.path.join(model.opt.output_dir, 'epoch0007_test', 'batch0000.npz'))
