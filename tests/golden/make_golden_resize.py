#!/usr/bin/env python
"""Generate the MiDaS working-resolution fixture (fullstep_midas_b1_120x200_cube_train.npz) from the REAL reference.

Run in the build container only (it imports /root/reference):

    python tests/golden/make_golden_resize.py            # write the fixture
    python tests/golden/make_golden_resize.py --spread [SEED ...]   # the step at 1 and at 8 threads: well conditioned?

Same construction as make_golden.py's case_full_step (the unmodified reference `Model`, the same patches, oracle/resnext.py as
the encoder torch.hub would return, seeded weights and a calibrated head, one synthetic batch, one `_train_on_batch`), with
`opt.dataset = 'cube_synthetic'`: the reference's own dataset-name rule (models/scene_flow_motion_field.py:84-94) then builds
MidasNet(resize=[224, 384]) with no patch, and the 120 x 200 frames -- no multiple of 32 -- go through both bicubic resizes
(third_party/MiDaS.py:221-222, :244-245).  A generator of its own because case_full_step stores its option overrides as floats;
here `over_keys` / `over_vals` are strings.

Conditioning (`--spread`, measured on the CPU before committing; the bounds are those tests/test_30_full_step_gpu.py applies to
fullstep_midas_b2_192x384_train, and a case counts as well conditioned when two runs of the reference that differ only in
torch.set_num_threads stay within a third of each):
                                            1 vs 8 threads   bound
  logged losses (rel)                       1.1e-7           1e-5
  acc_reg (rel)                             1.4e-7           5e-6
  per-parameter gradient norms (rel)        2.9e-4           1.5e-3
  MLP gradient elements / max|g|            8.2e-5           1e-3
  depth-net gradient elements / max|g|      1.3e-3           8e-3
Seed 197 is the best conditioned of eight tried: 173 and 191 also pass (norms 4.3e-4), 167 and 193 miss the third in the
gradient norms (8.2e-4, 1.0e-3), and 179 and 181 are chaotic (norms off by more than 1).
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

NAME = 'fullstep_midas_b1_120x200_cube_train'
CASE = dict(B=1, H=120, W=200, gap=1, epoch=6, seed=197, over=dict(dataset='cube_synthetic'))
LOSS_KEYS = ('loss', 'total_loss', 'flow_loss_1_2', 'disp_loss_1_2', 'sf_loss')
SF_KEEP = ('convs.0.conv.weight', 'convs.3.conv.bias', 'convs.5.conv.weight', 'convs.5.conv.bias')
DEPTH_KEEP = ('scratch.output_conv.4.weight', 'scratch.output_conv.2.weight', 'pretrained.layer1.0.weight',
              'pretrained.layer4.2.bn3.weight')


def run_step(B, H, W, gap, epoch, seed, over):
    """One `_train_on_batch` of the real reference -> (model, batch_log)."""
    import third_party.MiDaS as RM
    import visualize.html_visualizer as HV
    from models.scene_flow_motion_field import Model
    from oracle import resnext          # independent restatement of torchvision's ResNeXt-101 32x8d (NOT the product's)
    o = dict(helpers.FULL_STEP_OPT)
    o.update(midas=True, full_logdir=tempfile.mkdtemp())
    o.update(over)

    class _Loggers(object):
        def add_logger(self, *a):
            pass

        def get_html_logger(self):
            return None
    with mock.patch.object(HV, 'Pool', lambda n: None), \
            mock.patch.object(torch.hub, 'load', lambda repo, entry, *a, **k: resnext.resnext101_32x8d()), \
            mock.patch.object(RM.BaseModel, 'load', lambda self, path: None):
        model = Model(SimpleNamespace(**o), _Loggers())
    assert list(model.net_depth.resize) == [224, 384]        # the reference's own rule, no patch
    helpers.seeded_fill_(model.net_depth, seed)
    helpers.seeded_fill_(model.net_sceneflow, seed + 1)
    with torch.no_grad():
        model.net_depth.scratch.output_conv[4].weight.mul_(30.0)
        model.net_depth.scratch.output_conv[4].bias.fill_(2000.0)
    model.to(torch.device('cpu'))
    batch = MG.synthetic.make_batch(B, H, W, gap=gap, seed=seed + 2)
    log = model._train_on_batch(epoch, 0, helpers.loader_batch(batch))
    return model, log


def collect(model, log):
    out = {}
    for k, v in log.items():
        out['log_' + k] = np.array(float(v), dtype=np.float64)
    names, gnorm, pnorm = [], [], []
    for prefix, net in (('depth', model.net_depth), ('sf', model.net_sceneflow)):
        for k, p in net.named_parameters():
            names.append(prefix + '/' + k)
            gnorm.append(0.0 if p.grad is None else float(p.grad.double().norm()))
            pnorm.append(float(p.data.double().norm()))
    out['param_names'] = np.array(names)
    out['grad_norms'] = np.array(gnorm)
    out['param_norms_after'] = np.array(pnorm)
    for prefix, net, keep in (('sf', model.net_sceneflow, SF_KEEP), ('depth', model.net_depth, DEPTH_KEEP)):
        for k, p in net.named_parameters():
            if k in keep and p.grad is not None:
                out['g_%s/%s' % (prefix, k)] = p.grad.numpy().copy()
                out['p_%s/%s' % (prefix, k)] = p.data.numpy().copy()
    return out


def write(name=NAME, case=CASE):
    model, log = run_step(**case)
    over = case['over']
    out = {'B': np.array(case['B']), 'H': np.array(case['H']), 'W': np.array(case['W']), 'gap': np.array(case['gap']),
           'epoch': np.array(case['epoch']), 'seed': np.array(case['seed']), 'midas': np.array(1),
           'over_keys': np.array(sorted(over)), 'over_vals': np.array([str(over[k]) for k in sorted(over)])}
    out.update(collect(model, log))
    np.savez_compressed(os.path.join(MG.OUT_DIR, name + '.npz'), **out)
    print('wrote', name, {k: float(v) for k, v in log.items()})


def spread(case=CASE):
    runs = []
    for n in (1, 8):
        torch.set_num_threads(n)
        runs.append(collect(*run_step(**case)))
    a, b = runs
    res = {'loss': max(abs(float(a['log_' + k]) - float(b['log_' + k])) / abs(float(b['log_' + k])) for k in LOSS_KEYS),
           'acc': abs(float(a['log_acc_reg']) - float(b['log_acc_reg'])) / max(abs(float(b['log_acc_reg'])), 1e-30),
           'norm': max(abs(x - y) / y for x, y in zip(a['grad_norms'], b['grad_norms']) if y > 0)}
    for prefix in ('sf', 'depth'):
        res[prefix] = max(float(np.abs(a[k] - b[k]).max() / np.abs(b[k]).max()) for k in a if k.startswith('g_%s/' % prefix))
    print('1 vs 8 threads:', {k: '%.2e' % v for k, v in res.items()})
    return res


if __name__ == '__main__':
    if sys.argv[1:2] == ['--spread']:          # (--spread SEED ...: try other seeds)
        for seed in [int(a) for a in sys.argv[2:]] or [CASE['seed']]:
            print('seed', seed)
            spread(dict(CASE, seed=seed))
    else:
        torch.set_num_threads(4)
        write()
