#!/usr/bin/env python
"""Generate the `--optim sgd` trajectory fixtures (traj*sgd_*.npz) from the REAL reference.

Run in the build container only (it imports /root/reference):

    python tests/golden/make_golden_sgd.py            # all three
    python tests/golden/make_golden_sgd.py hourglass  # the two hourglass cases (tests/test_sgd_fixtures_regenerate_cpu.py)
    python tests/golden/make_golden_sgd.py --spread NAME    # condition (a) below: the series at 2 and at 8 threads

Same construction as make_golden.py's case_trajectory (the unmodified reference `Model`, seeded weights, one synthetic batch
repeated), with `--optim sgd` and the three flags the reference's NetInterface reads under it (netinterface.py:130-133), which
helpers.FULL_STEP_OPT does not carry: sgd_momentum, sgd_dampening, wdecay.  Every option that differs from FULL_STEP_OPT is
recorded as strings in `opt_keys` / `opt_vals`; `epochs` is the epoch passed to each step.

How the learning rates were chosen (checked on the CPU before committing; `--spread NAME` prints both figures):
  (a) two CPU runs of the reference that differ only in torch.set_num_threads (2 vs 8) agree to <= 1e-6 relative in every
      logged loss at every step (the criterion make_golden.py used for traj5_midas);
  (b) the reference's loss changes by >= 1e-4 relative between consecutive steps, so that the direction of every step is a
      real check.
Measured (max over the five logged losses and all steps of |a - b| / |b|, 2 vs 8 threads; smallest relative loss change):
  traj5sgd_hourglass_b2_32x48      lr 1e-4, MLP x 10:   spread 5.1e-7,  smallest change 2.6e-3
  traj5sgd_midas_b1_64x96          lr 1e-6, MLP x 1000: spread 8.7e-7,  smallest change 2.8e-4
  traj3sgd_hourglass_b2_32x48_m0   lr 1e-4, MLP x 10:   spread 1.1e-7,  smallest change 5.0e-2
"""
import os
import sys
import tempfile
import unittest.mock as mock
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the reference, the package and the repository root on sys.path)

sys.path.insert(0, os.path.join(MG.ROOT, 'tests'))
import helpers  # noqa: E402

KEYS = ('loss', 'flow_loss_1_2', 'disp_loss_1_2', 'sf_loss', 'acc_reg')


def _reference_model(o, seed, midas):
    import third_party.hourglass as RH
    import third_party.MiDaS as RM
    import visualize.html_visualizer as HV
    from models.scene_flow_motion_field import Model
    from oracle import resnext

    class _Loggers(object):
        def add_logger(self, *a):
            pass

        def get_html_logger(self):
            return None
    real_load = torch.load
    with mock.patch.object(HV, 'Pool', lambda n: None), \
            mock.patch.object(torch.hub, 'load', lambda repo, entry, *a, **k: resnext.resnext101_32x8d()), \
            mock.patch.object(RM.BaseModel, 'load', lambda self, path: None), \
            mock.patch.object(torch, 'load', lambda path, *a, **k: RH.HourglassModel().state_dict()
                              if 'pretrained_depth_ckpt' in str(path) else real_load(path, *a, **k)):
        model = Model(SimpleNamespace(**o), _Loggers())
    assert isinstance(model._optimizers[0], torch.optim.SGD)
    helpers.seeded_fill_(model.net_depth, seed)
    helpers.seeded_fill_(model.net_sceneflow, seed + 1)
    if midas:
        with torch.no_grad():
            model.net_depth.scratch.output_conv[4].weight.mul_(30.0)
            model.net_depth.scratch.output_conv[4].bias.fill_(2000.0)
    model.to(torch.device('cpu'))
    return model


def run_case(midas, B, H, W, gap, epochs, seed, over):
    """-> (model, series, option overrides) after len(epochs) reference steps on one batch."""
    o = dict(helpers.FULL_STEP_OPT)
    o.update(midas=midas, full_logdir=tempfile.mkdtemp())
    o.update(over)
    model = _reference_model(o, seed, midas)
    batch = MG.synthetic.make_batch(B, H, W, gap=gap, seed=seed + 2)
    series = {k: [] for k in KEYS}
    for i, ep in enumerate(epochs):
        log = model._train_on_batch(ep, i, helpers.loader_batch({k: (v.clone() if torch.is_tensor(v) else v)
                                                                 for k, v in batch.items()}))
        for k in KEYS:
            series[k].append(float(log[k]))
    return model, series


def case_sgd_trajectory(name, midas, B, H, W, gap, epochs, seed, over, keep_uncertainty=False):
    model, series = run_case(midas, B, H, W, gap, epochs, seed, over)
    keys = sorted(over)
    out = {'B': np.array(B), 'H': np.array(H), 'W': np.array(W), 'gap': np.array(gap), 'seed': np.array(seed),
           'midas': np.array(int(midas)), 'steps': np.array(len(epochs)), 'epochs': np.array(epochs),
           'opt_keys': np.array(keys), 'opt_vals': np.array([repr(over[k]) if not isinstance(over[k], str) else over[k]
                                                             for k in keys])}
    for k in KEYS:
        out['series_' + k] = np.array(series[k], dtype=np.float64)
    names, pnorm = [], []
    for prefix, net in (('depth', model.net_depth), ('sf', model.net_sceneflow)):
        for k, p in net.named_parameters():
            names.append(prefix + '/' + k)
            pnorm.append(float(p.data.double().norm()))
    out['param_names'] = np.array(names)
    out['param_norms_after'] = np.array(pnorm)
    for k, p in model.net_sceneflow.named_parameters():
        if k in ('convs.0.conv.weight', 'convs.5.conv.weight', 'convs.5.conv.bias'):
            out['p_sf/' + k] = p.data.numpy()
    dkeep = (['scratch.output_conv.4.weight', 'scratch.output_conv.2.weight', 'pretrained.layer4.2.bn3.weight'] if midas else
             ['net_depth.pred_layer.weight', 'net_depth.seq.1.weight'])
    for k, p in model.net_depth.named_parameters():
        if k in dkeep or (keep_uncertainty and 'uncertainty_layer' in k):
            out['p_depth/' + k] = p.data.numpy()
    # which parameters the reference's SGD holds a momentum buffer for after the last step
    out['depth_state_params'] = np.array(sorted(model._optimizers[0].state_dict()['state']), dtype=np.int64)
    np.savez_compressed(os.path.join(MG.OUT_DIR, name + '.npz'), **out)
    print('wrote', name, series['loss'])


SGD = dict(optim='sgd')
CASES = {
    # momentum 0.9, no dampening, no decay; two warm steps (epoch 1 <= warm_sf = 5): the MLP's momentum buffer starts at
    # step 1, the depth net's at step 3
    'traj5sgd_hourglass_b2_32x48': dict(midas=False, B=2, H=32, W=48, gap=1, epochs=[1, 1, 6, 6, 6], seed=151,
                                        over=dict(SGD, sgd_momentum=0.9, sgd_dampening=0.0, wdecay=0.0, lr=1e-4,
                                                  scene_lr_mul=10.0)),
    # every term: momentum, dampening and weight decay; MiDaS at the shipped learning rates (make_golden.py, traj5_midas)
    'traj5sgd_midas_b1_64x96': dict(midas=True, B=1, H=64, W=96, gap=1, epochs=[6, 6, 6, 6, 6], seed=157,
                                    over=dict(SGD, sgd_momentum=0.9, sgd_dampening=0.5, wdecay=1e-4, lr=1e-6,
                                              scene_lr_mul=1000.0)),
    # plain SGD with weight decay: the hourglass' uncertainty head gets no gradient, so the reference neither decays it nor
    # keeps state for it -- its parameters after the last step are stored
    'traj3sgd_hourglass_b2_32x48_m0': dict(midas=False, B=2, H=32, W=48, gap=1, epochs=[6, 6, 6], seed=163,
                                           over=dict(SGD, sgd_momentum=0.0, sgd_dampening=0.0, wdecay=1e-3, lr=1e-4,
                                                     scene_lr_mul=10.0), keep_uncertainty=True),
}
GROUPS = {'hourglass': ('traj5sgd_hourglass_b2_32x48', 'traj3sgd_hourglass_b2_32x48_m0'), 'midas': ('traj5sgd_midas_b1_64x96',)}


def spread(name):
    """Condition (a) and (b) of the module docstring for one case."""
    c = dict(CASES[name])
    c.pop('keep_uncertainty', None)
    runs = []
    for t in (2, 8):
        torch.set_num_threads(t)
        runs.append(run_case(**c)[1])
    sp = max(abs(a - b) / max(abs(b), 1e-30) for k in KEYS for a, b in zip(runs[0][k], runs[1][k]))
    loss = runs[1]['loss']
    change = min(abs(loss[i] - loss[i - 1]) / abs(loss[i - 1]) for i in range(1, len(loss)))
    print(name, 'thread spread %.3e' % sp, 'smallest relative loss change %.3e' % change, 'loss', loss)
    return sp, change


def main():
    if sys.argv[1:2] == ['--spread']:
        for n in sys.argv[2:] or list(CASES):
            spread(n)
        return
    torch.set_num_threads(4)
    names = []
    for arg in sys.argv[1:]:
        names += list(GROUPS[arg]) if arg in GROUPS else [arg]
    for n in names or list(CASES):
        case_sgd_trajectory(n, **CASES[n])


if __name__ == '__main__':
    main()
