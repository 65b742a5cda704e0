"""Host dispatch of dvd_hip/conv.py on the CPU: which weight-gradient entry point `xconv_wgrad` chooses for a kernel size, group
count and dtype (and with which integer arguments), and the per-weight cache protocol of `xconv_packed` /
`xconv_packed_scaled` (key, buffer reuse, the capture rule, the pack plan).  The library is a recording stand-in, as in
tests/test_fused_joins_wiring_cpu.py: only the dtypes and shapes of the tensors matter.  The kernels themselves are tested on the
GPU (tests/test_06_xconv_gpu.py, tests/test_10_act_fp16_gpu.py, tests/test_14_hourglass_act_fp16_gpu.py)."""
import pytest
import torch


class _RecordingLib(object):
    """Every dvd_* entry point: size queries answer a constant, launches are recorded as (name, arguments)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith('dvd_'):
            raise AttributeError(name)
        if name.endswith('_bytes'):
            return lambda *args: 64 if name == 'dvd_xconv_packed_bytes' else 16

        def launch(*args):
            self.calls.append((name, args))
            return 0
        return launch

    def count(self, name):
        return sum(1 for n, _ in self.calls if n == name)


@pytest.fixture
def recording(monkeypatch):
    from dvd_hip import conv as C
    lib = _RecordingLib()
    state = {'capturing': False, 'amax_calls': 0}

    def amax_of(t):
        state['amax_calls'] += 1
        return torch.zeros(1)

    monkeypatch.setattr(C, '_p', lambda t: t)
    monkeypatch.setattr(C, '_stream', lambda: 'stream')
    monkeypatch.setattr(C, '_workspace', lambda nbytes, device: torch.empty(int(nbytes), dtype=torch.uint8))
    monkeypatch.setattr(C, 'amax_of', amax_of)
    monkeypatch.setattr(C._lib, 'load', lambda: lib)
    monkeypatch.setattr(C._lib, 'check', lambda rc, name: None)
    monkeypatch.setattr(C, 'PACK_PLAN', C._PackPlan())
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: state['capturing'])   # (raises without a device)
    before = C.GRAD_SCALE['state']
    C.set_grad_scale_state(torch.zeros(16))
    try:
        yield C, lib, state
    finally:
        C.set_grad_scale_state(before)


def _ints(args):
    return [a for a in args if isinstance(a, int) and not isinstance(a, bool)]


def _wgrad(C, lib, ks, groups, dtype, relu_in=False, x_dtype=None, **kw):
    x = torch.zeros(1, 64, 4, 4, dtype=x_dtype or dtype)
    gy = torch.zeros(1, 64, 4, 4, dtype=dtype)
    del lib.calls[:]
    gw = C.xconv_wgrad(x, gy, (64, 64 // groups, ks, ks), relu_in, groups, **kw)
    assert gw.shape == (64, 64 // groups, ks, ks) and gw.dtype == torch.float32
    assert len(lib.calls) == 1
    return lib.calls[0]


# (kernel size, groups) -> entry point, and the integer that follows N, Cin, Cout, H, W in its argument list (groups for the 3x3
# kernels, the kernel size for the k x k ones, nothing for the 1x1 ones)
_WGRAD_CASES = [(1, 1, 'dvd_xwgrad1s_rowsum', 'dvd_xwgrad1s_h', []), (3, 1, 'dvd_xwgrad3', 'dvd_xwgrad3_h', [1]),
                (3, 2, 'dvd_xwgrad3', 'dvd_xwgrad3_h', [2]), (5, 1, 'dvd_xwgradk', 'dvd_xwgradk_h', [5]),
                (7, 1, 'dvd_xwgradk', 'dvd_xwgradk_h', [7]), (11, 1, 'dvd_xwgradk', 'dvd_xwgradk_h', [11])]


@pytest.mark.parametrize('relu_in', [False, True])
@pytest.mark.parametrize('ks,groups,name32,name16,extra', _WGRAD_CASES)
def test_wgrad_dispatch_fp32(recording, ks, groups, name32, name16, extra, relu_in):
    C, lib, state = recording
    rowsum = torch.zeros(64)
    name, args = _wgrad(C, lib, ks, groups, torch.float32, relu_in, rowsum=rowsum)
    # a 3x3 with a sums tensor takes the entry point that fills it (and only then: the second call below)
    assert name == ('dvd_xwgrad3_rowsum' if ks == 3 else name32)
    assert _ints(args) == [1, 64, 64, 4, 4] + extra + [int(relu_in)]
    # the per-channel sums go to the 1x1 and 3x3 launches and to no other
    assert any(a is rowsum for a in args) == (ks in (1, 3))
    # no fp32 form takes the loss-scale state
    gs = C.GRAD_SCALE['state']
    assert not any(torch.is_tensor(a) and a.numel() == 1 and a.data_ptr() == gs.data_ptr() + 4 for a in args)
    # the operands' scales are reduced here only when the caller did not supply them
    assert state['amax_calls'] == 2
    xa, ga = torch.zeros(1), torch.zeros(1)
    name, args = _wgrad(C, lib, ks, groups, torch.float32, relu_in, x_amax=xa, g_amax=ga)
    assert name == name32 and state['amax_calls'] == 2
    assert any(a is xa for a in args) and any(a is ga for a in args)


@pytest.mark.parametrize('relu_in', [False, True])
@pytest.mark.parametrize('ks,groups,name32,name16,extra', _WGRAD_CASES)
def test_wgrad_dispatch_fp16(recording, ks, groups, name32, name16, extra, relu_in):
    C, lib, state = recording
    name, args = _wgrad(C, lib, ks, groups, torch.float16, relu_in)
    assert name == name16
    assert _ints(args) == [1, 64, 64, 4, 4] + extra + [int(relu_in)]
    # the fp16 forms multiply by 1 / (loss scale): slot 1 of the state; they take no operand scale
    gs = C.GRAD_SCALE['state']
    assert any(torch.is_tensor(a) and a.numel() == 1 and a.data_ptr() == gs.data_ptr() + 4 for a in args)
    assert state['amax_calls'] == 0


def test_wgrad_exact_fp32_switch(recording):
    C, lib, state = recording
    assert not C.AB['no_xwgrad3']
    C.AB['no_xwgrad3'] = True
    try:
        for ks in (1, 3, 5):
            name, args = _wgrad(C, lib, ks, 1, torch.float32, True)
            assert name == 'dvd_xwgrad' and _ints(args) == [1, 64, 64, 4, 4, ks, 1]
        name, args = _wgrad(C, lib, 3, 2, torch.float32)                     # the grouped 3x3 has no other kernel
        assert name == 'dvd_xwgrad3' and _ints(args) == [1, 64, 64, 4, 4, 2, 0]
    finally:
        C.AB['no_xwgrad3'] = False


@pytest.mark.parametrize('ks,groups,dtype,x_dtype', [(5, 2, torch.float32, None), (5, 2, torch.float16, None),
                                                     (9, 1, torch.float32, None), (9, 1, torch.float16, None),
                                                     (3, 1, torch.float16, torch.float32)])
def test_wgrad_unsupported_shapes_raise(recording, ks, groups, dtype, x_dtype):
    C, lib, state = recording
    with pytest.raises(RuntimeError):
        _wgrad(C, lib, ks, groups, dtype, x_dtype=x_dtype)
    assert not lib.calls


def _packs(lib):
    return lib.count('dvd_xconv_pack'), lib.count('dvd_xconv_pack_scaled'), lib.count('dvd_xconv_pack_many')


def test_packed_cache_follows_the_weight(recording):
    C, lib, state = recording
    from dvd_hip import ops
    w = torch.zeros(64, 64, 3, 3)
    for transposed in (False, True):
        before = _packs(lib)[0]
        p = C.xconv_packed(w, transposed)
        assert p.numel() == 64 and p.dtype == torch.uint8 and _packs(lib)[0] == before + 1
        assert C.xconv_packed(w, transposed) is p and _packs(lib)[0] == before + 1          # nothing changed: nothing launched
        w.add_(1.0)                                                                            # the version counter moves
        assert C.xconv_packed(w, transposed) is p and _packs(lib)[0] == before + 2
        epoch = ops.WEIGHT_EPOCH[0]
        ops.WEIGHT_EPOCH[0] = epoch + 1                                                        # an optimiser step of the fused Adam
        try:
            assert C.xconv_packed(w, transposed) is p and _packs(lib)[0] == before + 3
            assert C.xconv_packed(w, transposed) is p and _packs(lib)[0] == before + 3
        finally:
            ops.WEIGHT_EPOCH[0] = epoch
    assert _packs(lib)[1:] == (0, 0)


def test_packed_kinds_never_share_a_buffer(recording):
    C, lib, state = recording
    w = torch.zeros(64, 64, 3, 3)
    gamma, var = torch.ones(64), torch.ones(64)
    f, t = C.xconv_packed(w, False), C.xconv_packed(w, True)
    ts = C.xconv_packed_scaled(w, 1, gamma, var, 1e-5)
    assert _packs(lib) == (2, 1, 0)
    assert len({id(f), id(t), id(ts)}) == 3 and len({f.data_ptr(), t.data_ptr(), ts.data_ptr()}) == 3
    # each is served from its own entry afterwards
    assert C.xconv_packed(w, False) is f and C.xconv_packed(w, True) is t
    assert C.xconv_packed_scaled(w, 1, gamma, var, 1e-5) is ts
    assert _packs(lib) == (2, 1, 0)


def test_scaled_packing_follows_gamma_var_and_eps(recording):
    C, lib, state = recording
    w = torch.zeros(64, 64, 3, 3)
    gamma, var = torch.ones(64), torch.ones(64)
    ts = C.xconv_packed_scaled(w, 1, gamma, var, 1e-5)
    assert C.xconv_packed_scaled(w, 1, gamma, var, 1e-5) is ts and _packs(lib) == (0, 1, 0)
    gamma.mul_(2.0)
    assert C.xconv_packed_scaled(w, 1, gamma, var, 1e-5) is ts and _packs(lib) == (0, 2, 0)
    assert C.xconv_packed_scaled(w, 1, gamma, var, 1e-3) is ts and _packs(lib) == (0, 3, 0)
    var.add_(1.0)
    assert C.xconv_packed_scaled(w, 1, gamma, var, 1e-3) is ts and _packs(lib) == (0, 4, 0)
    w.add_(1.0)
    assert C.xconv_packed_scaled(w, 1, gamma, var, 1e-3) is ts and _packs(lib) == (0, 5, 0)
    assert C.xconv_packed_scaled(w, 1, gamma, var, 1e-3) is ts and _packs(lib) == (0, 5, 0)
    # a BatchNorm without affine parameters: gamma None
    assert C.xconv_packed_scaled(w, 1, None, var, 1e-3) is ts and _packs(lib) == (0, 6, 0)
    assert C.xconv_packed_scaled(w, 1, None, var, 1e-3) is ts and _packs(lib) == (0, 6, 0)


def test_capture_without_a_plan_entry_packs_into_fresh_buffers(recording):
    C, lib, state = recording
    gamma, var = torch.ones(64), torch.ones(64)
    fresh, cached = torch.zeros(64, 64, 3, 3), torch.zeros(64, 64, 3, 3)
    held = [C.xconv_packed(cached, False), C.xconv_packed(cached, True), C.xconv_packed_scaled(cached, 1, gamma, var, 1e-5)]
    entries = dict(cached._dvd_xpack)
    assert len(entries) == 3
    state['capturing'] = True
    try:
        for w in (fresh, cached):
            for call in (lambda: C.xconv_packed(w, False), lambda: C.xconv_packed(w, True),
                         lambda: C.xconv_packed_scaled(w, 1, gamma, var, 1e-5)):
                before = sum(_packs(lib))
                a, b = call(), call()
                held += [a, b]
                assert sum(_packs(lib)) == before + 2 and _packs(lib)[2] == 0        # the launch is part of every capture
                assert a.numel() == b.numel() == 64
        assert len({id(p) for p in held}) == len(held) == 15                          # never a cached buffer, never one twice
        # the per-weight cache is neither created nor filled nor changed under capture
        assert getattr(fresh, '_dvd_xpack', None) is None
        assert set(cached._dvd_xpack) == set(entries)
        assert all(cached._dvd_xpack[k][0] == entries[k][0] and cached._dvd_xpack[k][1] is entries[k][1] for k in entries)
    finally:
        state['capturing'] = False
    # ... and serves the eager calls afterwards as if nothing had happened
    before = _packs(lib)
    assert C.xconv_packed(cached, False) is held[0] and C.xconv_packed(cached, True) is held[1]
    assert C.xconv_packed_scaled(cached, 1, gamma, var, 1e-5) is held[2] and _packs(lib) == before


def test_capture_with_a_plan_entry_returns_the_plans_buffer(recording):
    C, lib, state = recording
    w = torch.zeros(64, 64, 3, 3)
    gamma, var = torch.ones(64), torch.ones(64)
    # the eager (warm-up) calls leave their requests; extend() -- what a graph's owner calls before it opens a capture -- plans them
    eager = [C.xconv_packed(w, False), C.xconv_packed(w, True), C.xconv_packed_scaled(w, 1, gamma, var, 1e-5)]
    C.PACK_PLAN.extend()
    assert _packs(lib) == (2, 1, 1) and C.PACK_PLAN.launches == 1
    state['capturing'] = True
    try:
        got = [C.xconv_packed(w, False), C.xconv_packed(w, True), C.xconv_packed_scaled(w, 1, gamma, var, 1e-5)]
        want = [C.PACK_PLAN.lookup(w, 'F'), C.PACK_PLAN.lookup(w, 'T'), C.PACK_PLAN.lookup(w, 'Ts', gamma, var, 1e-5)]
        assert all(g is p and p is not None for g, p in zip(got, want))
        assert len({id(p) for p in got + eager}) == 6                  # the plan's buffers, not the per-weight cache's
        assert _packs(lib) == (2, 1, 1)
        # another BatchNorm's scale is not what the plan holds: packed inside the capture
        other = C.xconv_packed_scaled(w, 1, gamma, var, 1e-3)
        assert other is not want[2] and _packs(lib) == (2, 2, 1)
    finally:
        state['capturing'] = False
