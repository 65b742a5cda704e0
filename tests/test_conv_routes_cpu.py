"""Which kernels conv.py launches for which layer, pinned row by row (tests/golden/conv_routes.json).

Every row is one (layer, dtype, device, entry point, DVD_AB switch) combination; it stores the ordered list of launches of one
forward + backward and the STATS deltas (or the error the entry raises).  The library is a stand-in that records every call as
`name(pointer arguments|integer arguments)` -- T a tensor, N a null pointer, B a struct -- and computes nothing; a tensor
subclass reports is_cuda, and every tensor handed to a launch reports it from then on, so a composition (convolution, then
bn_eval_relu) is recorded whole.  The helpers that would launch on their own are recorded as pseudo-launches: `amax` (a max|.|
pass that no producer made unnecessary), `chansum`, `pack` (which weight shape is packed how) and `aten_conv2d`.

The recording was made from the tree in which the four module classes and conv_bn_act each carried their own copy of the
routing predicates.  Routing by hyper-parameters instead of by class changed the rows listed in `_twin`; those store the
earlier list and the current one side by side ([earlier, current]); the test asserts the current one and that it is the row of
the class the layer is now indistinguishable from.  No other row may carry two lists.

`python tests/test_conv_routes_cpu.py OUT.json` writes the current tree's rows."""
import contextlib
import ctypes
import functools
import json
import os

import pytest
import torch
from torch import nn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_routes.json')

DTYPES = ('fp32', 'fp16')
DEVICES = ('gpu', 'cpu')
ENTRIES = ('forward', 'cba_relu', 'cba_norelu', 'cba_res', 'cba_alias', 'cba_noaffine', 'x2d', 'x2d_fused')
# the DVD_AB switches one at a time; 'in_kernel0': no switch, dvd_xwgrad_rowsum_in_kernel answers 0
SWITCHES = ('none', 'gconv32', 'no_s2', 'no_alias', 'no_maskfuse', 'no_xwgrad3', 'in_kernel0')
LAYERS = ('x_k1', 'x_k3', 'x_k5', 'x_k7', 'x_k11', 'x_k3_c24', 'x_k1_s2', 'x_k3_s2', 'x_k3_s2_c24', 'x_k3_s2_g32', 'x_k3_s3', 'x_g64',
          'x_g32', 'x_g16', 'x_g8', 'x_k3_p0', 'x_k3_c8', 'c8', 'c8_1', 'c16', 'c16_s2', 'c32')


def _layers(C):
    X = C.XConv2d
    return {
        'x_k1': lambda: X(64, 64, 1),
        'x_k3': lambda: X(64, 64, 3, padding=1),
        'x_k5': lambda: X(32, 32, 5, padding=2),
        'x_k7': lambda: X(32, 32, 7, padding=3),
        'x_k11': lambda: X(32, 32, 11, padding=5),
        'x_k3_c24': lambda: X(24, 24, 3, padding=1),
        'x_k1_s2': lambda: X(64, 64, 1, stride=2, bias=False),
        'x_k3_s2': lambda: X(64, 64, 3, stride=2, padding=1),
        'x_k3_s2_c24': lambda: X(24, 24, 3, stride=2, padding=1),
        'x_k3_s2_g32': lambda: X(64, 64, 3, stride=2, padding=1, groups=2, bias=False),
        'x_k3_s3': lambda: X(64, 64, 3, stride=3, padding=1),
        'x_g64': lambda: X(128, 128, 3, padding=1, groups=2, bias=False),
        'x_g32': lambda: X(64, 64, 3, padding=1, groups=2, bias=False),
        'x_g16': lambda: X(64, 64, 3, padding=1, groups=4, bias=False),
        'x_g8': lambda: X(16, 16, 3, padding=1, groups=2, bias=False),
        'x_k3_p0': lambda: X(64, 64, 3, padding=0),
        'x_k3_c8': lambda: X(8, 8, 3, padding=1, bias=False),
        'c8': lambda: C.GroupedConv3x3C8(16),
        'c8_1': lambda: C.GroupedConv3x3C8(8),
        'c16': lambda: C.GroupedConv3x3C16(64),
        'c16_s2': lambda: C.GroupedConv3x3C16(64, stride=2),
        'c32': lambda: C.GroupedConv3x3C32(64),
    }


def _twin(layer, dtype, dev, switch):
    """The layer whose row a row that changed by design must now equal, or None: the row may not have changed."""
    if dev != 'gpu':
        return None
    if layer == 'x_g16':            # an XConv2d with 16 / 8 channels per group: the routes of GroupedConv3x3C16 / C8 (was ATen)
        return 'c16'
    if layer == 'x_g8':
        return 'c8'
    if layer == 'x_k3_c8':          # one group of 8, bias-free: the bare forward is GroupedConv3x3C8(8)'s (gconv; was xconv).  Every
        return 'c8_1'               # entry that fuses stays on the dense xconv kernel for both
    if switch == 'gconv32' and layer == 'x_g32' and dtype == 'fp32':      # the legacy kernels, as GroupedConv3x3C32
        return 'c32'
    # ... and the other half of that class dependence: csrc/gconv32.hip is fp32 only, so under DVD_AB=gconv32 an fp16
    # GroupedConv3x3C32 stays on the grouped xconv kernels like the XConv2d of the same hyper-parameters (was ATen)
    if switch == 'gconv32' and layer == 'c32' and dtype == 'fp16':
        return 'x_g32'
    return None


class _Gpu(torch.Tensor):
    @property
    def is_cuda(self):
        return True


class _Lib(object):
    """Records `name(pointers|integers)` for every entry point; size queries answer a constant."""

    def __init__(self, log, in_kernel):
        self._log, self._in_kernel = log, in_kernel

    def __getattr__(self, name):
        def call(*args):
            ptrs, ints = '', []
            for a in args:
                if a is None:
                    ptrs += 'N'
                elif torch.is_tensor(a):
                    ptrs += 'T'
                    if type(a) is torch.Tensor:          # a kernel's operand lives on the GPU
                        a.__class__ = _Gpu
                elif isinstance(a, (bool, int)):
                    ints.append(int(a))
                elif isinstance(a, (ctypes.c_size_t, ctypes.c_longlong)):
                    ints.append(int(a.value))
                elif not isinstance(a, float):
                    ptrs += 'B'
            if name.endswith('_bytes'):
                return 64
            self._log.append('%s(%s|%s)' % (name, ptrs, ','.join(map(str, ints))))
            return self._in_kernel if name == 'dvd_xwgrad_rowsum_in_kernel' else 0
        return call


@contextlib.contextmanager
def _stand_ins(C, log, in_kernel):
    import torch.nn.functional as F
    lib = _Lib(log, in_kernel)

    def known_amax(t):
        hit = getattr(t, '_dvd_amax', None)
        return hit[1] if (hit is not None and hit[0] == t._version) else None

    def set_amax(t, am):
        if am is not None:
            t._dvd_amax = (t._version, am)
        return t

    def amax_of(t):
        am = known_amax(t)
        if am is None:
            log.append('amax(%d)' % t.numel())
            am = torch.zeros(1)
            set_amax(t, am)
        return am

    def chansum(t, want_amax=False):
        log.append('chansum(%d)' % int(bool(want_amax)))
        if want_amax:
            set_amax(t, torch.zeros(1))
        return torch.zeros(t.shape[1])

    def pack(kind):
        def packed(weight, *args):
            groups = args[1] if kind == 'FT' else args[0]
            log.append('pack(%s|%s,%d)' % ('FT'[int(bool(args[0]))] if kind == 'FT' else kind,
                                           ','.join(map(str, weight.shape)), groups))
            return torch.zeros(8, dtype=torch.uint8)
        return packed

    def xconv_packed(weight, transposed, groups=1):
        return pack('FT')(weight, transposed, groups)

    real_conv2d = F.conv2d

    def conv2d(x, w, b=None, stride=1, *a, **kw):
        log.append('aten_conv2d(%s)' % (stride[0] if isinstance(stride, (tuple, list)) else stride))
        return real_conv2d(x, w, b, stride, *a, **kw)

    patches = [(C, '_p', lambda t: t), (C, '_stream', lambda: 0),
               (C, '_workspace', lambda nbytes, device: torch.empty(int(nbytes), dtype=torch.uint8)),
               (C, 'amax_of', amax_of), (C, 'new_scalar', lambda device: torch.zeros(1)), (C, 'known_amax', known_amax),
               (C, 'set_amax', set_amax), (C, 'chansum', chansum), (C, 'xconv_packed', xconv_packed),
               (C, 'xconv_packed_scaled', pack('Ts')), (C._lib, 'load', lambda: lib), (C._lib, 'check', lambda rc, name: None),
               (F, 'conv2d', conv2d)]
    saved = [(o, n, getattr(o, n)) for o, n, _ in patches]
    state, stats, ab = C.GRAD_SCALE['state'], dict(C.STATS), dict(C.AB)
    try:
        for o, n, v in patches:
            setattr(o, n, v)
        C.set_grad_scale_state(torch.zeros(16))
        yield
    finally:
        for o, n, v in saved:
            setattr(o, n, v)
        C.set_grad_scale_state(state)
        C.STATS.update(stats)
        C.AB.update(ab)


def _run_entry(C, conv, bns, x, entry):
    k, st, pad = conv.kernel_size[0], conv.stride[0], conv.padding[0]
    oh, ow = [(n + 2 * pad - k) // st + 1 for n in x.shape[2:]]
    res = torch.ones(1, conv.out_channels, oh, ow, dtype=x.dtype).as_subclass(type(x))
    if entry == 'forward':
        outs = [conv(x)]
    elif entry == 'cba_relu':
        outs = [C.conv_bn_act(conv, bns[0], x)]
    elif entry == 'cba_norelu':
        outs = [C.conv_bn_act(conv, bns[0], x, relu=False)]
    elif entry == 'cba_res':
        outs = [C.conv_bn_act(conv, bns[0], x, residual=res)]
    elif entry == 'cba_alias':
        outs = list(C.conv_bn_act(conv, bns[0], x, alias=True))
    elif entry == 'cba_noaffine':
        outs = [C.conv_bn_act(conv, bns[1], x)]
    elif entry == 'x2d':
        outs = [C.xconv2d(conv, x)]
    else:
        outs = list(C.xconv2d(conv, x, relu_in=True, residual=res, alias=True))
    torch.autograd.backward(outs, [torch.ones_like(o) for o in outs])


def _record_rows():
    """-> (records, rows): rows[layer]['dtype/device/entry'] = one index into records per switch."""
    from dvd_hip import conv as C
    assert not any(C.AB.values())
    records, index, rows = [], {}, {}
    log = []
    for in_kernel in (1, 0):
        with _stand_ins(C, log, in_kernel):
            for layer, make in _layers(C).items():
                conv = make()                       # (the values play no part: nothing is computed from them)
                bns = [nn.BatchNorm2d(conv.out_channels).eval(), nn.BatchNorm2d(conv.out_channels, affine=False).eval()]
                for dtype in DTYPES:
                    for dev in DEVICES:
                        for entry in ENTRIES:
                            for switch in (SWITCHES[:-1] if in_kernel else SWITCHES[-1:]):
                                del log[:]
                                for key in C.STATS:
                                    C.STATS[key] = 0
                                if switch in C.AB:
                                    C.AB[switch] = True
                                leaf = torch.ones(1, conv.in_channels, 6, 8, dtype=torch.float16 if dtype == 'fp16' else torch.float32,
                                                  requires_grad=True)
                                x = leaf * 1.0
                                try:
                                    _run_entry(C, conv, bns, x.as_subclass(_Gpu) if dev == 'gpu' else x, entry)
                                    rec = {'launches': list(log), 'stats': [C.STATS[key] for key in sorted(C.STATS)]}
                                except (RuntimeError, NotImplementedError, TypeError) as e:
                                    rec = {'error': '%s: %s' % (type(e).__name__, str(e).split('\n')[0][:60])}
                                finally:
                                    if switch in C.AB:
                                        C.AB[switch] = False
                                ser = json.dumps(rec, sort_keys=True)
                                if ser not in index:
                                    index[ser] = len(records)
                                    records.append(rec)
                                rows.setdefault(layer, {}).setdefault('%s/%s/%s' % (dtype, dev, entry), []).append(index[ser])
    return records, rows


@functools.lru_cache(maxsize=None)
def _current():
    return _record_rows()


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_matrix_is_the_recorded_one():
    from dvd_hip import conv as C
    rows = _golden()['rows']
    assert sorted(rows) == sorted(_layers(C)) == sorted(LAYERS)
    for layer, cells in rows.items():
        assert sorted(cells) == sorted('%s/%s/%s' % (d, v, e) for d in DTYPES for v in DEVICES for e in ENTRIES), layer
        assert all(len(v) == len(SWITCHES) for v in cells.values()), layer


@pytest.mark.parametrize('layer', LAYERS)
def test_rows_launch_what_was_recorded(layer):
    gold = _golden()
    records, rows = _current()
    bad = []
    for cell, want in gold['rows'][layer].items():
        dtype, dev, _ = cell.split('/')
        for switch, w, g in zip(SWITCHES, want, rows[layer][cell]):
            got = records[g]
            if isinstance(w, list):                 # changed by design: [earlier, current]
                twin = _twin(layer, dtype, dev, switch)
                assert twin is not None, 'row %s %s %s carries two lists but may not differ' % (layer, cell, switch)
                assert gold['records'][w[0]] != gold['records'][w[1]], (layer, cell, switch)
                if got != records[rows[twin][cell][SWITCHES.index(switch)]]:
                    bad.append((cell, switch, 'is not the row of %s' % twin, got))
                w = w[1]
            if got != gold['records'][w]:
                bad.append((cell, switch, gold['records'][w], got))
    assert not bad, '%d rows differ, the first: %r' % (len(bad), bad[0])


if __name__ == '__main__':
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'dynamic-video-depth_amd'))
    recs, rws = _record_rows()
    with open(sys.argv[1], 'w') as out:
        json.dump({'records': recs, 'rows': rws}, out, separators=(',', ':'), sort_keys=True)
        out.write('\n')
