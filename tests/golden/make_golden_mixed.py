#!/usr/bin/env python
"""Generate the mixed-frame-gap full-step fixtures (fullstep_mixed_*.npz) from the REAL reference.

Run in the build container only (it imports /root/reference):

    python tests/golden/make_golden_mixed.py            # all three (tests/test_mixed_fixtures_regenerate_cpu.py)
    python tests/golden/make_golden_mixed.py NAME ...

The reference cannot run a batch that mixes frame gaps (it integrates every pair over round(mean gap) Euler steps), but its
step is linear where it matters, so the expected values of ONE mixed step come from the UNMODIFIED reference
`Model._train_on_batch` on the uniform-gap sub-batches of the mixed batch.  With g over the gap groups, eps = 1e-8,
S0_g = sum of the loss mask of group g (the hourglass: mask_2.sum(), _calc_loss:286-289), n_g pairs per group, n = sum n_g:

    each loss term       L = sum_g L_g (S0_g + eps) / (sum_g S0_g + eps)
    main-loss gradient   the same combination of G_g, the reference's gradient with --acc_mul 0
                         (--weight_steps: the reference's G_g carries its factor steps_g already)
    regulariser          acc_reg = sum_g R_g (3 n_g HW + 1e-6) / (3 n HW + 1e-6), and the same for its gradient, which is the
                         difference of the reference's gradients with and without --acc_mul
    parameters after     the reference's own torch.optim.Adam objects (netinterface.py:96-97,127-129), stepped once on the
                         combined gradient

all combined in float64.  Every run of this script first repeats the check of that algebra: a UNIFORM 4-pair gap-1 batch
(synthetic.make_batch(4, 32, 48, gap=1, seed=4242), options and seeds of fullstep_hourglass_b2_32x48_train), split 2 + 2 and
combined as above, against the reference's own whole-batch step, within the bounds tests/test_35_mixed_gaps_gpu.py applies to
the HIP step (losses rtol 1e-5, acc_reg rtol 5e-6, gradient norms 1.5e-3, elements 1e-3 / 8e-3 of max|g| for the scene-flow /
depth network); it refuses to write fixtures otherwise.  Measured when the fixtures were made: 7e-8 relative in the four
losses, 1.4e-7 in acc_reg, 2.2e-6 of max|g| in the worst gradient element.

How the seed was chosen (a criterion on the REFERENCE alone, as make_golden_sgd.py's condition (a); nothing of the HIP step enters):
at 32x48 the hourglass's deepest level is 2x3 pixels, and a pre-activation within fp32 rounding of 0 there flips a ReLU when
the summation order changes -- the reference's own gradient norms then depend on its thread count.  A case is only written if
every combined per-parameter gradient norm agrees to <= 1.5e-5 relative (1 % of the GPU test's bound of 1.5e-3) between
reference runs at 1, 2 and 8 threads (`conditioning`, repeated at every run); the seed is the first from 211 upwards that
satisfies it.  Measured on the `train` case: seed 211 2.8e-4, 212 3.1e-7, 213 6.8e-4, 214 1.2e-6, 215 2.3e-5, 216 3.1e-6,
217 1.0e-4, 218 3.2e-6 -- the ill-conditioned seeds stand two to three orders apart from the others.  Hence 212.

The fixtures store what the fullstep_* fixtures store (make_golden.py::case_full_step), plus the inputs (`in_*`),
`steps_per_pair` and the per-group parts (`group_*`).
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

LOSS_KEYS = ('loss', 'total_loss', 'flow_loss_1_2', 'disp_loss_1_2', 'sf_loss')
EPS = 1e-8


def _reference_model(o, seed):
    import third_party.hourglass as RH
    import visualize.html_visualizer as HV
    from models.scene_flow_motion_field import Model

    class _Loggers(object):
        def add_logger(self, *a):
            pass

        def get_html_logger(self):
            return None
    real_load = torch.load
    with mock.patch.object(HV, 'Pool', lambda n: None), \
            mock.patch.object(torch, 'load', lambda path, *a, **k: RH.HourglassModel().state_dict()
                              if 'pretrained_depth_ckpt' in str(path) else real_load(path, *a, **k)):
        model = Model(SimpleNamespace(**o), _Loggers())
    helpers.seeded_fill_(model.net_depth, seed)
    helpers.seeded_fill_(model.net_sceneflow, seed + 1)
    model.to(torch.device('cpu'))
    return model


def _params(model):
    for prefix, net in (('depth', model.net_depth), ('sf', model.net_sceneflow)):
        for k, p in net.named_parameters():
            yield prefix + '/' + k, p


def _options(over):
    o = dict(helpers.FULL_STEP_OPT)
    o.update(midas=False, full_logdir=tempfile.mkdtemp())
    o.update(over)
    return o


def reference_step(batch, epoch, seed, over):
    """One step of a fresh reference model on `batch` -> (log, {name: gradient as float64 or None})."""
    model = _reference_model(_options(over), seed)
    log = model._train_on_batch(epoch, 0, helpers.loader_batch({k: (v.clone() if torch.is_tensor(v) else v)
                                                                for k, v in batch.items()}))
    return ({k: float(v) for k, v in log.items()},
            {k: (None if p.grad is None else p.grad.detach().double().clone()) for k, p in _params(model)})


def sub_batch(batch, pairs):
    B = batch['flow_1_2'].shape[0]
    return {k: (v[pairs].contiguous() if (torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == B) else v)
            for k, v in batch.items()}


def combine(batch, groups, epoch, seed, over):
    """groups: [(steps, [pair indices])].  -> (log, {name: combined float64 gradient or None}, per-group parts)."""
    o = _options(over)
    warm = epoch <= o['warm_sf']
    with_reg = o['interp_steps'] > 0 and (not warm or o['warm_reg']) and o['acc_mul'] > 0
    H, W = batch['flow_1_2'].shape[1:3]
    n = sum(len(p) for _, p in groups)
    S0 = [float(batch['mask_2'][p].double().sum()) for _, p in groups]
    w_main = [(s + EPS) / (sum(S0) + EPS) for s in S0]
    w_reg = [(3.0 * len(p) * H * W + 1e-6) / (3.0 * n * H * W + 1e-6) for _, p in groups]
    log = {k: 0.0 for k in LOSS_KEYS + ('acc_reg',)}
    grads, parts = {}, {'log': [], 'S0': S0, 'grad_norms': []}
    for (steps, pairs), wm, wr in zip(groups, w_main, w_reg):
        sb = sub_batch(batch, pairs)
        log_a, g_all = reference_step(sb, epoch, seed, over)
        if with_reg:
            _log_m, g_main = reference_step(sb, epoch, seed, dict(over, acc_mul=0.0))
        else:
            g_main = g_all
        parts['log'].append(log_a)
        parts['grad_norms'].append({k: (0.0 if g is None else float(g.norm())) for k, g in g_all.items()})
        for k in LOSS_KEYS:
            log[k] += log_a[k] * wm
        log['acc_reg'] += float(log_a['acc_reg']) * wr
        for k, gm in g_main.items():
            ga = g_all[k]
            if ga is None and gm is None:
                grads.setdefault(k, None)
                continue
            gm = torch.zeros_like(ga) if gm is None else gm
            ga = gm if ga is None else ga
            c = gm * wm + (ga - gm) * wr
            grads[k] = c if grads.get(k) is None else grads[k] + c
    return log, grads, parts


def step_on(grads, seed, over):
    """The reference's own optimisers, stepped once on the combined gradient -> the model."""
    model = _reference_model(_options(over), seed)
    for k, p in _params(model):
        p.grad = None if grads[k] is None else grads[k].float()
    for optimizer in model._optimizers:
        optimizer.step()
    return model


def self_check():
    """The algebra on a uniform batch: split 2 + 2 and combined against the reference's whole-batch step, within the bounds of
    the GPU test.  Returns the measured figures; raises if a bound is missed."""
    seed, epoch = 101, 6            # fullstep_hourglass_b2_32x48_train
    batch = MG.synthetic.make_batch(4, 32, 48, gap=1, seed=4242)
    log_w, g_w = reference_step(batch, epoch, seed, {})
    log_c, g_c, _ = combine(batch, [(1, [0, 1]), (1, [2, 3])], epoch, seed, {})
    m = {'loss_rel': max(abs(log_c[k] - log_w[k]) / abs(log_w[k]) for k in LOSS_KEYS),
         'acc_reg_rel': abs(log_c['acc_reg'] - log_w['acc_reg']) / abs(log_w['acc_reg']), 'norm_rel': 0.0, 'elem': 0.0}
    bad = []
    for k, gw in g_w.items():
        if gw is None:
            assert g_c[k] is None, k
            continue
        if float(gw.norm()) == 0.0:
            continue
        rel = abs(float(g_c[k].norm()) - float(gw.norm())) / float(gw.norm())
        err = (g_c[k] - gw).abs() / gw.abs().max()
        m['norm_rel'], m['elem'] = max(m['norm_rel'], rel), max(m['elem'], float(err.max()))
        tol = 1e-3 if k.startswith('sf/') else 8e-3
        if rel >= 1.5e-3 or int((err > tol).sum()) > max(2, gw.numel() // 5000):
            bad.append(k)
    print('self-check (uniform batch split 2 + 2 against the whole-batch step):', m)
    if m['loss_rel'] > 1e-5 or m['acc_reg_rel'] > 5e-6 or bad:
        raise SystemExit('the split-and-combine algebra does not reproduce the reference\'s whole-batch step: %s %s' % (m, bad))
    return m


def conditioning(batch, groups, epoch, seed, over):
    """Largest relative difference of a combined per-parameter gradient norm between reference runs at 1, 2 and 8 threads."""
    runs = []
    for t in (1, 2, 8):
        torch.set_num_threads(t)
        runs.append(combine(batch, groups, epoch, seed, over)[1])
    torch.set_num_threads(4)
    norms = [{k: float(g.norm()) for k, g in r.items() if g is not None} for r in runs]
    return max(abs(a[k] - norms[2][k]) / norms[2][k] for a in norms[:2] for k in a if norms[2][k] > 0.0)


def case_mixed(name, gaps, epoch, seed, over):
    B, H, W = len(gaps), 32, 48
    batch = MG.synthetic.make_batch(B, H, W, gap=gaps, seed=seed + 2)
    groups = [(g, [b for b in range(B) if gaps[b] == g]) for g in sorted(set(gaps))]
    spread = conditioning(batch, groups, epoch, seed, over)
    print(name, 'thread spread of the reference\'s combined gradient norms: %.3e' % spread)
    if spread > 1.5e-5:
        raise SystemExit('%s: the reference\'s own gradient norms move by %.3e with its thread count (limit 1.5e-5): this seed '
                         'is ill-conditioned, take the next' % (name, spread))
    log, grads, parts = combine(batch, groups, epoch, seed, over)
    model = step_on(grads, seed, over)
    keys = sorted(over)
    out = {'B': np.array(B), 'H': np.array(H), 'W': np.array(W), 'epoch': np.array(epoch), 'seed': np.array(seed),
           'midas': np.array(0), 'steps_per_pair': np.array(gaps, dtype=np.int64),
           'over_keys': np.array(keys), 'over_vals': np.array([float(over[k]) for k in keys])}
    for k, v in batch.items():
        out['in_' + k] = v.numpy()
    for k, v in log.items():
        out['log_' + k] = np.array(v, dtype=np.float64)
    out['group_steps'] = np.array([g for g, _ in groups], dtype=np.int64)
    out['group_size'] = np.array([len(p) for _, p in groups], dtype=np.int64)
    out['group_pairs'] = np.array([b for _, p in groups for b in p], dtype=np.int64)
    out['group_S0'] = np.array(parts['S0'], dtype=np.float64)
    for k in LOSS_KEYS + ('acc_reg',):
        out['group_log_' + k] = np.array([float(pl[k]) for pl in parts['log']], dtype=np.float64)
    names, gnorm, pnorm = [], [], []
    for k, p in _params(model):
        names.append(k)
        gnorm.append(0.0 if grads[k] is None else float(grads[k].norm()))
        pnorm.append(float(p.data.double().norm()))
    out['param_names'] = np.array(names)
    out['grad_norms'] = np.array(gnorm)
    # (per group: the norms of the reference's own gradient on that sub-batch, regulariser included)
    out['group_grad_norms'] = np.array([[gn[k] for k in names] for gn in parts['grad_norms']])
    out['param_norms_after'] = np.array(pnorm)
    keep = {'sf/' + k: 'sf/' for k in ('convs.0.conv.weight', 'convs.3.conv.bias', 'convs.5.conv.weight', 'convs.5.conv.bias')}
    keep.update({'depth/' + k: 'depth/' for k in ('net_depth.pred_layer.weight', 'net_depth.seq.0.weight', 'net_depth.seq.1.weight')})
    for k, p in _params(model):
        if k in keep and grads[k] is not None:
            prefix, pname = k.split('/', 1)
            out['g_%s/%s' % (prefix, pname)] = grads[k].float().numpy()
            out['p_%s/%s' % (prefix, pname)] = p.data.numpy()
    np.savez_compressed(os.path.join(MG.OUT_DIR, name + '.npz'), **out)
    print('wrote', name, log)


GAPS = [2, 1, 4, 1]          # in THIS (ungrouped) order
CASES = {
    'fullstep_mixed_hourglass_b4_32x48_train': dict(gaps=GAPS, epoch=6, seed=212, over={}),
    'fullstep_mixed_hourglass_b4_32x48_warm': dict(gaps=GAPS, epoch=1, seed=212, over={}),
    'fullstep_mixed_hourglass_b4_32x48_wsteps': dict(gaps=GAPS, epoch=6, seed=212, over={'weight_steps': True}),
}


def main():
    torch.set_num_threads(4)
    self_check()
    for n in sys.argv[1:] or list(CASES):
        case_mixed(n, **CASES[n])


if __name__ == '__main__':
    main()
