"""The host-only argument checks the post-processing wrappers of dvd_hip/ops.py share (_int_arg, _real_arg, _host_ids): every
edge of each, on the host alone -- no GPU, and the library is never loaded."""
import numpy as np
import pytest
import torch

from dvd_hip import ops

INF, NAN = float('inf'), float('nan')


def _refused(fn, *args, **kw):
    with pytest.raises(RuntimeError, match='unit: name must'):
        fn('unit', 'name', *args, **kw)


def test_int_arg_takes_integers_in_the_closed_range_and_nothing_else():
    for v in (1, 255, 7, np.int32(1), np.int64(255), np.uint8(255), 1.0, 255.0, np.float32(7.0), torch.tensor(7), np.array(3)):
        got = ops._int_arg('unit', 'name', v, 1, 255)
        assert type(got) is int and got == int(v)
    assert ops._int_arg('unit', 'name', -3, -3, 0) == -3 and ops._int_arg('unit', 'name', 0, -3, 0) == 0
    for v in (0, 256, -1, True, False, np.bool_(True), 1.5, NAN, INF, -INF, None, '1', [1], 1 + 0j, np.float64(2.5), torch.tensor(1.5),
              torch.tensor([1, 2])):
        _refused(ops._int_arg, v, 1, 255)
    # where floats are not taken, an integral float is refused like any other
    assert ops._int_arg('unit', 'name', np.int16(2), 1, 255, floats=False) == 2
    for v in (2.0, np.float32(2.0), True, NAN, INF):
        _refused(ops._int_arg, v, 1, 255, floats=False)


def test_real_arg_closed_and_open_ends():
    # [0, inf): the default
    for v in (0, 0.0, -0.0, 1, 2.5, np.float32(0.25), np.float64(3.0), np.int32(4), 3.0e38):
        got = ops._real_arg('unit', 'name', v)
        assert type(got) is float and got == v
    for v in (-1e-30, -1, NAN, INF, -INF, True, False, np.bool_(False), None, '1', [1.0], 1e39, np.float64(1e39), 10 ** 400):
        _refused(ops._real_arg, v)                                    # (1e39, 10^400: finite in float64 / as an int, Inf as float32)
    # (0, 1]: open below, closed above
    for v in (1e-30, 0.5, 1, 1.0, np.float32(1.0)):
        assert ops._real_arg('unit', 'name', v, lo_open=True, hi=1.0) == v
    for v in (0, 0.0, -0.0, -0.5, 1.0000001, 2, NAN, INF, True):
        _refused(ops._real_arg, v, lo_open=True, hi=1.0)
    # [0, 0.25] and a lower end that is not 0
    assert ops._real_arg('unit', 'name', 0.25, hi=0.25) == 0.25 and ops._real_arg('unit', 'name', 0, hi=0.25) == 0.0
    _refused(ops._real_arg, 0.2500001, hi=0.25)
    assert ops._real_arg('unit', 'name', -2.0, lo=-2.0) == -2.0
    _refused(ops._real_arg, -2.0, lo=-2.0, lo_open=True)
    _refused(ops._real_arg, -3e38 * 10, lo=-INF)                      # -3e39: above the lower end, but -Inf as float32


def test_splat_params_keep_the_kernels_rules():
    p = ops._splat_params('splat', z_near=0, z_tol=0.0, w_tap=0.25, w_min=1e-6, value_bound=2, fill=NAN)
    assert all(type(v) is float for v in p.values()) and p['w_tap'] == 0.25 and p['fill'] != p['fill']
    assert ops._splat_params('splat', fill=-INF) == {'fill': -INF}
    for kw in (dict(z_near=-1e-9), dict(z_tol=NAN), dict(w_tap=0.0), dict(w_tap=0.26), dict(w_min=0.0), dict(value_bound=0.0),
               dict(value_bound=INF), dict(z_near=1e39)):
        with pytest.raises(RuntimeError, match=next(iter(kw))):
            ops._splat_params('splat', **kw)


def test_host_ids():
    ids = ops._host_ids('unit', 'name', [0, 2, 1], (3,), 0, 3)
    assert ids.dtype.kind == 'i' and ids.tolist() == [0, 2, 1]
    assert ops._host_ids('unit', 'name', (4, 5), (2,), 4, 6).tolist() == [4, 5]
    assert ops._host_ids('unit', 'name', torch.tensor([[0, 1], [2, -1]], dtype=torch.int32), (2, 2), -1, 3).tolist() == [[0, 1], [2, -1]]
    assert ops._host_ids('unit', 'name', np.array([3, 4], np.uint8), (None,)).tolist() == [3, 4]      # any extent, no range
    # an integral float array is taken, and comes back as integers
    ids = ops._host_ids('unit', 'name', np.array([0.0, 2.0, 1.0], np.float32), (3,), 0, 3)
    assert ids.dtype.kind == 'i' and ids.tolist() == [0, 2, 1]
    # ... a non-integral one, or any float array where floats are not taken, is not
    for bad in (np.array([0.0, 0.5, 1.0]), [0, 1.5, 2], [0.0, NAN, 1.0], [0.0, INF, 1.0]):
        _refused(ops._host_ids, bad, (3,), 0, 3)
    _refused(ops._host_ids, np.array([0.0, 2.0, 1.0]), (3,), 0, 3, floats=False)
    # a wrong length, a wrong rank, nothing at all, things that are no ids
    for bad in ([0, 1], [0, 1, 2, 0], [[0, 1, 2]], [], 1, None, ['a', 'b', 'c'], [True, False, True], [[0, 1], [2]]):
        _refused(ops._host_ids, bad, (3,), 0, 3)
    _refused(ops._host_ids, [[0, 1, 2]], (None,))
    with pytest.raises(RuntimeError, match=r'unit: name must hold \[2, any, 3\] integral ids'):       # a free extent reads as one
        ops._host_ids('unit', 'name', np.zeros((1, 4, 3), np.int32), (2, None, 3))
    # an id out of range, at either end; the upper end is exclusive
    for bad in ([0, 1, 3], [-1, 1, 2]):
        with pytest.raises(RuntimeError, match='unit: the ids of name span'):
            ops._host_ids('unit', 'name', bad, (3,), 0, 3)
    assert ops._host_ids('unit', 'name', [-1, 1, 3], (3,)).tolist() == [-1, 1, 3]                       # (not asked to)


def test_the_wrappers_refuse_host_arguments_through_the_shared_checks():
    """Each wrapper's own names reach the messages, and host data is refused before a tensor is looked at (all tensors here
    are CPU tensors, which every wrapper refuses last)."""
    tabs = {'R': torch.eye(3)[None], 't': torch.zeros(1, 3), 'K_T': torch.eye(3)[None]}
    pts = torch.zeros(1, 1, 3, 4, 4)
    for k0 in (0.5, True, NAN, 1 << 30):
        with pytest.raises(RuntimeError, match='track_project: k0'):
            ops.track_project(pts, [0], tabs, k0=k0)
        with pytest.raises(RuntimeError, match='track_filter: k0'):
            ops.track_filter(pts, [0], tabs, torch.ones(1, 1, 4, 4), [1.0], k0=k0)
    with pytest.raises(RuntimeError, match='track_filter: tol'):
        ops.track_filter(pts, [0], tabs, torch.ones(1, 1, 4, 4), [1.0], tol=1e39)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ops.track_project(pts, [0], tabs, k0=-1.0)                     # an integral float is an integer; the CPU tensor is what is left
