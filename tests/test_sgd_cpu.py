"""`--optim sgd` without a GPU: the model accepts it, the C ABI carries dvd_sgd_step[_guarded], and flat.FlatNet's SGD state
interchanges with torch.optim.SGD -- and with the REAL reference's checkpoints (skipped where /root/reference is absent)."""
import copy
import ctypes
import os
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import helpers
import ref_exec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sgd_opt(**kw):
    o = dict(helpers.FULL_STEP_OPT)
    o.update(optim='sgd', sgd_momentum=0.9, sgd_dampening=0.0, wdecay=0.0)
    o.update(kw)
    return o


def _model(o):
    from dvd_hip.models.scene_flow_motion_field import Model
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return Model(SimpleNamespace(**o), None)


def test_model_accepts_optim_sgd_with_the_reference_optim_params():
    m = _model(_sgd_opt(sgd_momentum=0.8, sgd_dampening=0.25, wdecay=1e-4))
    assert m.optim_params == {'momentum': 0.8, 'dampening': 0.25, 'weight_decay': 1e-4}    # netinterface.py:130-133
    # without the three flags: options_train.py:88-93's defaults
    o = dict(helpers.FULL_STEP_OPT, optim='sgd')
    assert _model(o).optim_params == {'momentum': 0.9, 'dampening': 0, 'weight_decay': 0.0}
    with pytest.raises(NotImplementedError):
        _model(dict(helpers.FULL_STEP_OPT, optim='rmsprop'))


def test_sgd_entry_points_are_declared_exported_and_bound():
    import re
    from dvd_hip import _lib, build
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dvd_hip.h')).read(), flags=re.S)
    lib = ctypes.CDLL(build.build_library())
    for name in ('dvd_sgd_step', 'dvd_sgd_step_guarded'):
        assert re.search(r'\b%s\s*\(' % name, src), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.load().dvd_abi_version() == 8
    # argument validation happens before any HIP call: a null parameter pointer, and momentum without a buffer
    st = _lib.load().dvd_sgd_step_guarded(None, None, 1.0, None, None, None, 4, 0.1, 0.0, 0.0, 0.0, 1, None, None)
    assert st == _lib.DVD_EINVAL
    from dvd_hip import ops
    assert 'sgd_kernel' in ops.BYTE_CLASS_KERNELS['adam']


class _Net(torch.nn.Module):
    """Ragged parameter sizes and a head that no loss reaches (like the hourglass' uncertainty layer)."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.a = torch.nn.Linear(5, 3)
        self.dead = torch.nn.Linear(3, 2)
        self.b = torch.nn.Conv2d(3, 7, 3)

    def loss(self, x):
        return self.b(self.a(x).view(1, 3, 1, 1).expand(1, 3, 4, 4)).square().sum()


def _torch_sgd(momentum, dampening, wd, steps):
    net = _Net()
    opt = torch.optim.SGD(net.parameters(), lr=0.05, momentum=momentum, dampening=dampening, weight_decay=wd)
    for k in range(steps):
        opt.zero_grad()
        net.loss(torch.linspace(-1, 1, 5) * (k + 1)).backward()
        opt.step()
    return net, opt


def _flat_sgd(momentum, dampening, wd):
    from dvd_hip import flat
    return flat.FlatNet.sgd(_Net(), 0.05, momentum=momentum, dampening=dampening, weight_decay=wd)


def _same_state(a, b):
    assert a['param_groups'] == b['param_groups'], (a['param_groups'], b['param_groups'])
    assert sorted(a['state']) == sorted(b['state'])
    for i in a['state']:
        assert sorted(a['state'][i]) == sorted(b['state'][i]) == ['momentum_buffer']
        assert torch.equal(a['state'][i]['momentum_buffer'], b['state'][i]['momentum_buffer']), i


@pytest.mark.parametrize('momentum,dampening,wd,steps', [(0.9, 0.0, 1e-3, 2), (0.9, 0.5, 0.0, 3), (0.0, 0.0, 1e-3, 2),
                                                         (0.9, 0.0, 0.0, 0)],
                         ids=['m0.9-wd', 'm0.9-damp', 'm0', 'never-stepped'])
def test_flatnet_sgd_state_dict_round_trips_with_torch_sgd(momentum, dampening, wd, steps):
    net, opt = _torch_sgd(momentum, dampening, wd, steps)
    ref = opt.state_dict()
    if momentum == 0 or steps == 0:
        assert ref['state'] == {}
    else:
        assert 2 not in ref['state'] and 3 not in ref['state'] and len(ref['state']) == 4    # the dead head has no state
    # torch -> FlatNet -> torch layout
    fn = _flat_sgd(momentum, dampening, wd)
    assert fn.exp_avg is None and fn.exp_avg_sq is None and (fn.momentum_buf is None) == (momentum == 0)
    assert fn.state_dict()['state'] == {}                                   # before any step
    fn.load_state_dict(ref)
    mine = fn.state_dict()
    _same_state(mine, ref)
    # FlatNet's file -> a fresh torch.optim.SGD, which then reports the same state
    net2, opt2 = _torch_sgd(momentum, dampening, wd, 0)
    opt2.load_state_dict(copy.deepcopy(mine))
    _same_state(opt2.state_dict(), ref)
    if ref['state']:
        assert fn.step_count == 1          # a loaded buffer counts as initialised: the next step is not a first step
        for i in ref['state']:
            assert torch.equal(fn.view(fn.momentum_buf, i), ref['state'][i]['momentum_buffer'])
        assert not fn.view(fn.momentum_buf, 2).any() and not fn.view(fn.momentum_buf, 3).any()


def test_flatnet_sgd_keeps_this_runs_hyper_parameters():
    _, opt = _torch_sgd(0.9, 0.0, 0.0, 2)
    fn = _flat_sgd(0.5, 0.1, 1e-4)
    fn.load_state_dict(opt.state_dict())
    g = fn.state_dict()['param_groups'][0]
    assert (g['lr'], g['momentum'], g['dampening'], g['weight_decay']) == (0.05, 0.5, 0.1, 1e-4)


def test_adam_checkpoint_into_an_sgd_flatnet_warns_and_starts_empty():
    net = _Net()
    adam = torch.optim.Adam(net.parameters(), lr=1e-3)
    net.loss(torch.ones(5)).backward()
    adam.step()
    fn = _flat_sgd(0.9, 0.0, 0.0)
    fn.momentum_buf.fill_(7.0)
    with pytest.warns(UserWarning, match='momentum_buffer'):
        fn.load_state_dict(adam.state_dict())
    assert not fn.momentum_buf.any() and fn.step_count == 0
    assert fn.state_dict()['state'] == {}
    # what the reference does: torch.optim.SGD accepts the Adam state and starts its buffers empty
    sgd = torch.optim.SGD(_Net().parameters(), lr=0.05, momentum=0.9)
    sgd.load_state_dict(adam.state_dict())
    assert all('momentum_buffer' not in s for s in sgd.state.values())


def test_flatnet_sgd_live_ranges_follow_absorbed_gradients():
    """The parameters the engine produced a gradient for (absorb_grads) are the ones the SGD launch covers; the dead head's
    segment (with its padding) is left out, the rest merges into contiguous ranges, fixed from the first step on."""
    fn = _flat_sgd(0.9, 0.0, 1e-3)
    fn.detach_grads()
    fn.module.loss(torch.ones(5)).backward()
    fn.absorb_grads()
    o = fn.offsets
    assert fn.live_ranges() == [(0, o[2]), (o[4], fn.numel)]
    fn._seen[2] = True                      # frozen: later recordings do not change the set
    assert fn.live_ranges() == [(0, o[2]), (o[4], fn.numel)]
    assert _flat_sgd(0.9, 0.0, 0.0).live_ranges() == [(0, fn.numel)]     # nothing recorded: every parameter


# ---------------------------------------------------------------------------------------------------------------------
# the real reference


@pytest.mark.skipif(not ref_exec.available(), reason='reference checkout not present')
def test_sgd_checkpoints_interchange_with_the_reference_netinterface(tmp_path):
    from dvd_hip import flat, synthetic
    o = _sgd_opt(midas=False, full_logdir=str(tmp_path), sgd_momentum=0.9, sgd_dampening=0.1, wdecay=1e-3)
    ck_ref, ck_mine = str(tmp_path / 'ref.pt'), str(tmp_path / 'mine.pt')
    batch = synthetic.make_batch(1, 32, 48, gap=1, seed=9)
    with ref_exec.on_reference_path():
        ref = ref_exec.reference_model(o)
        assert isinstance(ref._optimizers[0], torch.optim.SGD)
        helpers.seeded_fill_(ref.net_depth, 21)
        helpers.seeded_fill_(ref.net_sceneflow, 22)
        ref.to(torch.device('cpu'))
        ref._train_on_batch(6, 0, helpers.loader_batch(batch))          # non-warm: both optimisers get state
        ref._train_on_batch(6, 1, helpers.loader_batch(batch))
        ref.save_state_dict(ck_ref, save_optimizer=True, additional_values={'epoch': 6})
        ref_opt = [copy.deepcopy(op.state_dict()) for op in ref._optimizers]
    dead = [i for i, (name, _) in enumerate(ref.net_depth.named_parameters()) if i not in ref_opt[0]['state']]
    assert dead and all('uncertainty' in n for i, (n, _) in enumerate(ref.net_depth.named_parameters()) if i in dead)
    # ---- reference file -> product, before .to()
    mine = _model(o)
    assert mine.load_state_dict(ck_ref) == {'epoch': 6}
    assert mine._pending_optimizer_state is not None and len(mine._pending_optimizer_state) == 2
    flats = [flat.FlatNet.sgd(mine.net_depth, o['lr'], **mine.optim_params),
             flat.FlatNet.sgd(mine.net_sceneflow, o['lr'] * o['scene_lr_mul'], **mine.optim_params)]
    for fn, st in zip(flats, mine._pending_optimizer_state):
        fn.load_state_dict(st)
    for fn, st in zip(flats, ref_opt):
        got = fn.state_dict()
        assert sorted(got['state']) == sorted(st['state']) and len(st['state']) > 0    # the same parameters without state
        for i in st['state']:
            assert torch.equal(got['state'][i]['momentum_buffer'], st['state'][i]['momentum_buffer']), i
            assert torch.equal(fn.view(fn.momentum_buf, i), st['state'][i]['momentum_buffer']), i
        assert got['param_groups'][0] == st['param_groups'][0]
    # ---- product file -> a fresh reference model, which keeps training
    mine._optimizers = flats
    mine.save_state_dict(ck_mine, save_optimizer=True, additional_values={'epoch': 7})
    with ref_exec.on_reference_path():
        ref2 = ref_exec.reference_model(o)
        ref2.to(torch.device('cpu'))
        assert ref2.load_state_dict(ck_mine) == {'epoch': 7}
        for op, st in zip(ref2._optimizers, ref_opt):
            got = op.state_dict()
            assert sorted(got['state']) == sorted(st['state'])
            for i in st['state']:
                assert torch.equal(got['state'][i]['momentum_buffer'], st['state'][i]['momentum_buffer'])
        log = ref2._train_on_batch(6, 2, helpers.loader_batch(batch))
        assert np.isfinite(log['loss'])
