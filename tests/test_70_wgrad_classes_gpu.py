"""Every kernel instantiation of csrc/xwgrad3.hip against the float64 specification, bit for bit.

The weight-gradient entry points (dvd_xwgrad3 / 1s / k, their _rowsum and _h forms) dispatch to 53 instantiations of five kernel
families, by storage, kernel size, groups, channels per group, W % 64, W % 2, H * W % 4 / % 16, the row-sum pointer and the
dvd_xwgrad_select hook.  tests/wgrad_spec.py holds the specification (written from include/dvd_hip.h), the case table and the list
of instantiations; tests/test_wgrad_spec_cpu.py proves on the CPU, with dvd_xwgrad_describe (the dispatch itself), that the table
reaches every one of them and that with the table's data every product, partial sum and unscale of the kernels is exact.  So here
every gw must EQUAL the specification's, whatever lane, slice or launch computed an element and in whatever order -- under every
hook the case lists, with max|.| scalars that are exact or upper bounds -- and on split_data (fp32) the value with the low terms
of the two-term split, sum (h h' + h l' + l h'): one wrong neighbour dword of a shifted fragment, one tap or row of a warm-up too
few, a strip's last column dropped all fail, with no tolerance to hide in.

Per launch: gw lies inside a buffer of 0xff bytes with 256 guard bytes on either side; the workspace is exactly the bytes
dvd_xwgrad_describe reports, pre-filled with 0xff (NaNs: a partial nobody wrote shows) and followed by 256 guard bytes; four bytes
less are refused with DVD_ENOSPC before anything is written.  The row sums of the _rowsum entry points equal gy.sum exactly on
both routes (the RSUM kernels and the chansum_kernel pass), and gw is the same bits with and without the sums pointer.

Real-valued cases follow, one per family and storage on instantiations no earlier test visibly reached, with the project's
norm-wise bound 2e-5 max|dW| (tests/test_46_wgrad_live_steps_gpu.py); the measured values are logged (helpers.log_measured,
profiles/wgrad_classes_parity_measured.jsonl)."""
import ctypes

import pytest
import torch

import helpers
import wgrad_spec as S

pytestmark = pytest.mark.gpu

GUARD = 256
TOL = 2e-5
_REF = {}            # case -> float64 references, shared by the storages and hooks
_DEV = {}            # (case, storage, data set) -> device operands
_RAN = set()         # instantiation keys that test_exact launched
_DONE = set()        # (case, storage) that test_exact ran to its end


@pytest.fixture(scope='module', autouse=True)
def _free():
    yield
    _REF.clear()
    _DEV.clear()


@pytest.fixture(scope='module')
def lib():
    from dvd_hip import _lib
    L = _lib.load()
    yield L
    assert L.dvd_xwgrad_select(0) == 0


def _ref(case):
    name = case[0]
    if name not in _REF:
        _REF.clear()                       # the storages of a case follow each other
        KS, N, Cin, Cout, H, W, G = S.shape_of(case)
        ex, sp = S.exact_data(case), S.split_data(case)
        dW, rows = S.spec(ex['x'], ex['gy'], KS, G, case[9])
        kern, truth = S.split_expected(case, sp)
        _REF[name] = {'exact': ex, 'split': sp, 'dW': dW, 'rows': rows, 'split_kernel': kern, 'split_truth': truth}
    return _REF[name]


def _at(t, dtype, offset=0):
    """t on the GPU in `dtype`, `offset` bytes behind a 256-byte boundary."""
    t = t.to(dtype)
    nbytes = t.numel() * t.element_size()
    buf = torch.zeros(256 + offset + nbytes + 32, dtype=torch.uint8, device='cuda')
    pad = (-buf.data_ptr()) % 256
    v = buf[pad + offset:pad + offset + nbytes].view(dtype).view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 256 == offset
    return v


def _guarded(shape):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((GUARD + 4 * n + GUARD,), 0xff, dtype=torch.uint8, device='cuda')
    return buf, buf[GUARD:GUARD + 4 * n].view(torch.float32).view(shape)


def _intact(buf, nbytes):
    return bool((buf[:GUARD] == 0xff).all()) and bool((buf[GUARD + nbytes:] == 0xff).all())


def _launch(lib, case, storage, x, gy, x_amax=0.0, gy_amax=0.0, rowsum=False, relu=None, short=0, out_scale=S.H16_OUT_SCALE):
    """One call of the entry point that serves (case, storage, rowsum) -> (status, gw, row sums or None, description).
    Asserts the guards round gw, the row sums and behind the workspace.  short: bytes taken off the workspace size."""
    from dvd_hip.ops import _p, _stream
    KS, N, Cin, Cout, H, W, G = S.shape_of(case)
    relu = case[9] if relu is None else relu
    status, d = S.describe(lib, case, storage, rowsum)
    assert status == 0
    need = d['need']
    gbuf, gw = _guarded((Cout, Cin // G, KS, KS))
    ws = torch.full((need + GUARD,), 0xff, dtype=torch.uint8, device='cuda')
    rbuf, rs = _guarded((Cout,)) if rowsum else (None, None)
    tail = (_p(ws), ctypes.c_size_t(need - short), N, Cin, Cout, H, W) + ((G,) if KS == 3 else (KS,) if KS > 3 else ()) + (
        int(relu), _stream())
    stem = 'dvd_xwgrad1s' if KS == 1 else 'dvd_xwgrad3' if KS == 3 else 'dvd_xwgradk'
    if storage == S.H16:
        sc = None if out_scale is None else torch.full((1,), float(out_scale), device='cuda')
        st = getattr(lib, stem + '_h')(_p(x), _p(gy), _p(sc), _p(gw), *tail)
    else:
        xa, ga = torch.full((1,), float(x_amax), device='cuda'), torch.full((1,), float(gy_amax), device='cuda')
        if rowsum:
            st = getattr(lib, stem + '_rowsum')(_p(x), _p(xa), _p(gy), _p(ga), _p(gw), _p(rs), *tail)
        else:
            st = getattr(lib, stem)(_p(x), _p(xa), _p(gy), _p(ga), _p(gw), *tail)
    torch.cuda.synchronize()
    tag = '%s %s' % (case[0], storage)
    assert _intact(gbuf, gw.numel() * 4), '%s: the guard bytes around gw were written' % tag
    assert bool((ws[need:] == 0xff).all()), '%s: written behind the %d workspace bytes dvd_xwgrad_describe reports' % (tag, need)
    if rowsum:
        assert _intact(rbuf, Cout * 4), '%s: the guard bytes around the row sums were written' % tag
    if st != 0:
        assert bool((gbuf == 0xff).all()) and bool((ws == 0xff).all()), '%s: a refused call wrote something' % tag
    return st, gw, rs, d


def _operands(case, storage, which):
    key = (case[0], storage, which)
    if key not in _DEV:
        if len(_DEV) > 4:
            _DEV.clear()
        data = _ref(case)[which]
        _DEV[key] = (_at(data['x'], S.DTYPE[storage]), _at(data['gy'], S.DTYPE[storage]), data['x_amax'], data['gy_amax'])
    return _DEV[key]


def _same(got, want, tag):
    got = got.cpu()
    want = want.float()
    if not bool(torch.isfinite(got).all()) or not torch.equal(got, want):
        bad = (got != want) | ~torch.isfinite(got)
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError('%s: %d of %d values differ from the specification, the first at %s: %r, expected %r' % (
            tag, int(bad.sum()), got.numel(), idx, float(got[idx]), float(want[idx])))
    return got


PARAMS = [(c, st) for c in S.CASES for st in S.storages_of(c)]


@pytest.mark.parametrize('case,storage', PARAMS, ids=['%s-%s' % (c[0].replace(' ', '_'), st) for c, st in PARAMS])
def test_exact(lib, case, storage):
    from dvd_hip import _lib
    ref = _ref(case)
    x, gy, xa, ga = _operands(case, storage, 'exact')
    scale = S.H16_OUT_SCALE if storage == S.H16 else 1.0
    want = ref['dW'] * scale
    try:
        for hook in case[11]:
            _lib.check(lib.dvd_xwgrad_select(hook), 'dvd_xwgrad_select')
            st, gw, _, d = _launch(lib, case, storage, x, gy, xa, ga)
            keys = ', '.join(sorted(S.keys_of(d)))
            tag = '%s %s hook %d | %s' % (case[0], storage, hook, keys)
            assert st == 0, '%s: %s' % (tag, lib.dvd_last_error())
            plain = _same(gw, want, tag)
            _RAN.update(S.keys_of(d))
            if case[10] and storage == S.F32:
                # the row sums: from the kernel where the route has an RSUM form, else from the extra pass; the same gw bits
                st, gw, rs, d = _launch(lib, case, storage, x, gy, xa, ga, rowsum=True)
                tag = '%s %s hook %d with row sums | %s' % (case[0], storage, hook, ', '.join(sorted(S.keys_of(d))))
                assert st == 0, '%s: %s' % (tag, lib.dvd_last_error())
                assert d['rsum'] + d['chansum'] == 1
                assert torch.equal(gw.cpu(), plain), '%s: gw differs from the call without the sums pointer' % tag
                _same(rs, ref['rows'], tag + ' (row sums, %s)' % ('in the kernel' if d['rsum'] else 'extra pass'))
                _RAN.update(S.keys_of(d))
        _lib.check(lib.dvd_xwgrad_select(0), 'dvd_xwgrad_select')
        tag = '%s %s' % (case[0], storage)
        # four bytes less than the described workspace: refused, nothing written (checked in _launch)
        st, _, _, _ = _launch(lib, case, storage, x, gy, xa, ga, short=4)
        assert st == _lib.DVD_ENOSPC, '%s: a workspace four bytes short returned %d' % (tag, st)
        if storage == S.F32:
            # max|.| may be an upper bound: the same bits at 64 times the true maxima
            st, gw, _, _ = _launch(lib, case, storage, x, gy, 64.0 * xa, 64.0 * ga)
            assert st == 0
            _same(gw, want, tag + ' (amax = 64 max|.|)')
            if case[10]:
                st, gw, rs, _ = _launch(lib, case, storage, x, gy, 64.0 * xa, 64.0 * ga, rowsum=True)
                assert st == 0
                _same(gw, want, tag + ' (amax = 64 max|.|, with row sums)')
                _same(rs, ref['rows'], tag + ' (amax = 64 max|.|, row sums)')
        # all-zero operands with a zero max|.| scalar: exactly 0, finite
        zx, zg = torch.zeros_like(x), torch.zeros_like(gy)
        for xx, gg, a, b, what in ((zx, gy, 0.0, ga, 'x = 0'), (x, zg, xa, 0.0, 'gy = 0'), (zx, zg, 0.0, 0.0, 'both 0')):
            st, gw, _, _ = _launch(lib, case, storage, xx, gg, a, b)
            assert st == 0
            _same(gw, torch.zeros_like(want), '%s (%s)' % (tag, what))
        if storage == S.F32:
            # the low terms of the split: sum (h h' + h l' + l h'), exactly
            x, gy, xa, ga = _operands(case, storage, 'split')
            st, gw, _, d = _launch(lib, case, storage, x, gy, xa, ga)
            assert st == 0
            got = _same(gw, ref['split_kernel'], tag + ' split_data | ' + ', '.join(sorted(S.keys_of(d))))
            # ... which is the float64 truth but for the l l' term the arithmetic drops: 49 / 4 of 2^-22 per product at the most
            assert float((got.double() - ref['split_truth']).abs().max()) <= (S.SPLIT_BUDGET + 1) * 3.5 * 3.5 * 2.0 ** -22
        _DONE.add((case[0], storage))
    finally:
        _lib.check(lib.dvd_xwgrad_select(0), 'dvd_xwgrad_select')


def test_every_required_key_ran():
    """When the whole table ran (no selection by -k or node id), every instantiation of REQUIRED was launched on the GPU."""
    if _DONE == {(c[0], st) for c, st in PARAMS}:
        missing = sorted(set(S.REQUIRED) - _RAN)
        assert not missing, 'never launched: %s' % missing


@pytest.mark.parametrize('name,KS,N,Cin,Cout,H,W', S.OLD_CASES, ids=[c[0].replace(' ', '_') for c in S.OLD_CASES])
def test_exact_fp32_kernel(lib, name, KS, N, Cin, Cout, H, W):
    """dvd_xwgrad (csrc/xwgrad.hip, what DVD_AB=no_xwgrad3 runs): fp32 MFMA on unscaled operands, exact on integers."""
    from dvd_hip.ops import _p, _stream
    case = (name, KS, N, Cin, Cout, H, W, 1, (S.F32,), 1, False, (0,))
    d = S.exact_data(case)
    want = S.spec(d['x'], d['gy'], KS, 1, 1)[0]
    x, gy = _at(d['x'], torch.float32), _at(d['gy'], torch.float32)
    nws = lib.dvd_xwgrad_workspace_bytes(N, Cin, Cout, H, W, KS)
    assert nws > 0
    for relu, w in ((1, want), (0, S.spec(d['x'], d['gy'], KS, 1, 0)[0])):
        gbuf, gw = _guarded((Cout, Cin, KS, KS))
        ws = torch.full((nws + GUARD,), 0xff, dtype=torch.uint8, device='cuda')
        st = lib.dvd_xwgrad(_p(x), _p(gy), _p(gw), _p(ws), ctypes.c_size_t(nws), N, Cin, Cout, H, W, KS, relu, _stream())
        torch.cuda.synchronize()
        assert st == 0, lib.dvd_last_error()
        assert _intact(gbuf, gw.numel() * 4) and bool((ws[nws:] == 0xff).all())
        _same(gw, w, '%s relu_in %d' % (name, relu))


# ---- alignment (include/dvd_hip.h: the operands of the weight-gradient entry points) ----------------------------------------
# (case, storage, bytes x and gy must be aligned to)
ALIGNED = [('w3 4x3', S.H16, 2), ('w3 6x65', S.F32, 4), ('g3 2x6', S.H16, 4), ('k5 3x22', S.F32, 8), ('k7 2x42', S.H16, 4),
           ('s1 29x43', S.H16, 2), ('b1 12x21', S.H16, 8), ('b1 12x21', S.F32, 16), ('w3 5x64', S.F32, 16), ('g3 5x64', S.H16, 16)]


@pytest.mark.parametrize('name,storage,align', ALIGNED, ids=['%s-%s' % (n.replace(' ', '_'), s) for n, s, _ in ALIGNED])
def test_operand_alignment(lib, name, storage, align):
    """x and gy at the weakest alignment the contract allows (`align` bytes behind a 256-byte boundary) give the same bits; half
    of it is refused before any launch."""
    from dvd_hip import _lib
    case = S.CASE[name]
    ref = _ref(case)
    d = S.describe(lib, case, storage)[1]
    assert d['align'] == align
    data = ref['exact']
    want = ref['dW'] * (S.H16_OUT_SCALE if storage == S.H16 else 1.0)
    if align < 16:
        x, gy = _at(data['x'], S.DTYPE[storage], align), _at(data['gy'], S.DTYPE[storage], align)
        st, gw, _, _ = _launch(lib, case, storage, x, gy, data['x_amax'], data['gy_amax'])
        assert st == 0, lib.dvd_last_error()
        _same(gw, want, '%s %s, operands %d bytes off' % (name, storage, align))
    half = align // 2
    if half >= (2 if storage == S.H16 else 4):
        good = _at(data['x'], S.DTYPE[storage]), _at(data['gy'], S.DTYPE[storage])
        off = _at(data['x'], S.DTYPE[storage], half), _at(data['gy'], S.DTYPE[storage], half)
        for x, gy in ((off[0], good[1]), (good[0], off[1])):
            st, _, _, _ = _launch(lib, case, storage, x, gy, data['x_amax'], data['gy_amax'])
            assert st == _lib.DVD_EINVAL and b'aligned' in lib.dvd_last_error()


# ---- real-valued data, with the project's bound -------------------------------------------------------------------------------
# (case, storage, hook, with row sums): instantiations no earlier test visibly reached
REAL = [('k7 3x22', S.F32, 0, False), ('k7 2x42', S.H16, 0, False), ('k11 3x22', S.F32, 0, False), ('k11 5x65', S.H16, 0, False),
        ('k5 3x22', S.H16, 0, False), ('b1 12x21', S.F32, 0, True), ('b1 14x26', S.H16, 0, False), ('g3 5x64', S.H16, 0, False),
        ('g3 3x42', S.F32, 0, True), ('w3 5x64', S.F32, 2, False), ('w3 6x65', S.H16, 0, False), ('s1 12x21', S.F32, 0, True),
        ('s1 29x43', S.H16, 0, False)]


@pytest.mark.parametrize('name,storage,hook,rowsum', REAL, ids=['%s-%s' % (n.replace(' ', '_'), s) for n, s, _, _ in REAL])
def test_real_valued(lib, name, storage, hook, rowsum):
    """randn data against the float64 gradient of the operands as stored: max |err| <= 2e-5 max|dW| (tests/test_46); the row sums
    within L 2^-24 sum|g| for L = the number of gy values of a channel (any order of fp32 additions)."""
    from dvd_hip import _lib
    case = S.CASE[name]
    KS, N, Cin, Cout, H, W, G = S.shape_of(case)
    d = S.real_data(case)
    xs, gs = d['x'].to(S.DTYPE[storage]), d['gy'].to(S.DTYPE[storage])
    want, rows = S.spec(xs, gs, KS, G, case[9])
    x, gy = _at(xs, S.DTYPE[storage]), _at(gs, S.DTYPE[storage])
    try:
        _lib.check(lib.dvd_xwgrad_select(hook), 'dvd_xwgrad_select')
        st, gw, rs, dd = _launch(lib, case, storage, x, gy, float(xs.abs().max()), float(gs.abs().max()), rowsum=rowsum, out_scale=None)
    finally:
        _lib.check(lib.dvd_xwgrad_select(0), 'dvd_xwgrad_select')
    assert st == 0, lib.dvd_last_error()
    keys = ', '.join(sorted(S.keys_of(dd)))
    got = gw.cpu().double()
    e = float((got - want).abs().max() / want.abs().max())
    print('%s %s | %s: |err| / max|dW| = %.3g (bound %.3g)' % (name, storage, keys, e, TOL))
    helpers.log_measured('test_70 real %s %s | %s: of max|dW|' % (name, storage, keys), e, TOL)
    assert bool(torch.isfinite(got).all()) and e <= TOL, '%s %s | %s: %.3g of max|dW|' % (name, storage, keys, e)
    if rowsum:
        L = N * H * W
        err = float(((rs.cpu().double() - rows).abs() / gs.double().abs().sum((0, 2, 3))).max())
        helpers.log_measured('test_70 real %s %s row sums: of sum|g|' % (name, storage), err, L * 2.0 ** -24)
        assert err <= L * 2.0 ** -24
