"""Every kernel class and every epilogue of csrc/xconv.hip against the float64 specification, bit for bit.

dvd_xconv_fwd[_h] dispatches to several dozen instantiations of xconv_kernel (block shape x staging family x main loop x
storage), each with a narrow or a wide epilogue and up to seven optional operands.  tests/xconv_spec.py holds the specification
(written from include/dvd_hip.h), the case table and the list of classes; tests/test_xconv_spec_cpu.py proves on the CPU, with
dvd_xconv_describe, that the table reaches every class, and that with the table's small-integer data every product, partial sum,
unscale and epilogue step of the kernel is exact.  So here every output must EQUAL the specification's, whatever lane computed it
and in whatever order: a lane that writes the wrong channel, a clamp that reads the neighbour's BatchNorm pair, a ragged run that
is dropped or a store one run too far all fail, with no tolerance to hide in.

Per launch: y lies inside a buffer of NaN bytes with 256 guard bytes on either side (an output nobody wrote, or a store past the
end, shows); the max|y| scalar, zeroed, must come back as max|v| exactly, and pre-set to twice that must stay.  The calls go to
the C entry points through ctypes: fp16 -> fp32 (dvd_xconv_fwd_h with out_f16 = 0) and the strided forms with residual / mask are
documented modes the Python layer never uses.

A handful of real-valued cases follow, against the same specification with a per-element bound (see test_real_valued)."""
import ctypes

import pytest
import torch

import helpers
import xconv_spec as X

pytestmark = pytest.mark.gpu

GUARD = 256
_REF = {}            # (case, epilogue) -> (v, amax): one float64 reference, shared by the storages


def _ref(case, data, epi):
    key = (case[0], epi[0])
    if key not in _REF:
        v, _, amax = X.spec(**X.spec_args(case, data, epi))
        _REF[key] = (v, amax)
    return _REF[key]


@pytest.fixture(scope='module', autouse=True)
def _free():
    yield
    _REF.clear()
    _DATA.clear()


_DATA = {}


def _data(case):
    if case[0] not in _DATA:
        _DATA.clear()                      # the storages of a case follow each other
        _DATA[case[0]] = X.exact_data(case)
    return _DATA[case[0]]


def _guarded(shape, dtype, offset=0):
    """-> (buffer of 0xff bytes, y inside it): GUARD bytes in front (+ offset), at least GUARD behind."""
    n = 1
    for s in shape:
        n *= s
    nbytes = n * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((GUARD + offset + nbytes + GUARD + 16,), 0xff, dtype=torch.uint8, device='cuda')
    assert buf.data_ptr() % 16 == 0
    y = buf[GUARD + offset:GUARD + offset + nbytes].view(dtype).view(shape)
    return buf, y


def _guards_intact(buf, y, offset):
    nbytes = y.numel() * y.element_size()
    return bool((buf[:GUARD + offset] == 0xff).all()) and bool((buf[GUARD + offset + nbytes:] == 0xff).all())


def _at(t, dtype, offset=0):
    """t on the GPU in `dtype`, `offset` bytes off a 16-byte boundary."""
    if t is None:
        return None
    t = t.to(dtype)
    if not offset:
        return t.cuda().contiguous()
    buf = torch.zeros(t.numel() * t.element_size() + 32, dtype=torch.uint8, device='cuda')
    v = buf[16 + offset:16 + offset + t.numel() * t.element_size()].view(dtype).view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == offset
    return v


class _Launcher(object):
    """The packings and device operands of one (case, storage, data); run(epilogue) -> (y, buffer, y_amax scalar)."""

    def __init__(self, case, storage, data):
        from dvd_hip import _lib
        from dvd_hip.ops import _p, _stream
        self.lib, self._lib, self._p, self._stream = _lib.load(), _lib, _p, _stream
        self.case, self.storage, self.data = case, storage, data
        name, self.Cin, self.Cout, self.H, self.W, self.k, self.G, self.mode, self.N = case
        self.ti, self.to = X.IN_DTYPE[storage], X.OUT_DTYPE[storage]
        self.x = data['x'].to(self.ti).cuda()
        self.packs = {}
        self.dev = {}

    def pack(self, pk):
        if pk not in self.packs:
            tr = pk[0] == 't'
            w = self.data['wt' if tr else 'wf'].cuda().contiguous()
            co, ci = (self.Cin, self.Cout) if tr else (self.Cout, self.Cin)           # the FORWARD convolution's channel totals
            nbytes = self.lib.dvd_xconv_packed_bytes(co, ci, self.k, self.G, int(tr))
            assert nbytes > 0
            packed = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
            if len(pk) > 1:
                g, var, eps = self.data['scale_t' if tr else 'scale_f']
                g, var = g.cuda(), var.cuda()
                st = self.lib.dvd_xconv_pack_scaled(self._p(w), self._p(packed), co, ci, self.k, self.G, int(tr), self._p(g), self._p(var),
                                                    float(eps), self._stream())
            else:
                st = self.lib.dvd_xconv_pack(self._p(w), self._p(packed), co, ci, self.k, self.G, int(tr), self._stream())
            self._lib.check(st, 'dvd_xconv_pack')
            self.packs[pk] = packed
        return self.packs[pk]

    def operand(self, name, offset=0):
        key = (name, offset)
        if key not in self.dev:
            t = self.data[name]
            if name in ('bn', 'bn_plain'):
                g, b, m, v, eps = t
                keep = [None if q is None else q.cuda() for q in (g, b, m, v)]
                self.dev[key] = (keep, self._lib.BnParams(*[None if q is None else q.data_ptr() for q in keep], float(eps)))
            elif name == 'bias':
                self.dev[key] = t.cuda()
            else:
                self.dev[key] = _at(t, self.to, offset)
        return self.dev[key]

    def run(self, epi, y_amax0=0.0, x_amax=4.0, offset=0):
        ename, flags, ops, pk = epi
        flags |= X.mode_flags(self.mode)
        packed = self.pack(X.packing_of(self.mode, pk))
        bias = self.operand('bias') if 'bias' in ops else None
        res = self.operand('residual', offset) if 'residual' in ops else None
        mask = self.operand('mask') if 'mask' in ops else None
        bn = None
        for o in ops:
            if o in ('bn', 'bn_plain'):
                bn = ctypes.byref(self.operand(o)[1])
        buf, y = _guarded(X.shapes_of(self.case)[1], self.to, offset)
        ya = torch.full((1,), float(y_amax0), device='cuda')
        p, dims = self._p, (self.N, self.Cin, self.Cout, self.H, self.W, self.k, self.G, flags)
        if self.storage == X.F32:
            xa = torch.full((1,), float(x_amax), device='cuda')
            st = self.lib.dvd_xconv_fwd(p(self.x), p(xa), p(packed), p(bias), p(res), p(mask), bn, p(y), p(ya), *dims, self._stream())
        else:
            st = self.lib.dvd_xconv_fwd_h(p(self.x), p(packed), p(bias), p(res), p(mask), bn, p(y), p(ya), *dims,
                                          int(self.storage == X.H16), self._stream())
        self._lib.check(st, 'dvd_xconv_fwd')
        torch.cuda.synchronize()
        return y, buf, ya


def _first_diff(got, want):
    bad = (got != want) | torch.isnan(got)
    idx = bad.nonzero()
    n, c, yy, xx = [int(i) for i in idx[0]]
    return int(bad.sum()), (n, c, yy, xx), float(got[n, c, yy, xx]), float(want[n, c, yy, xx])


def _check_exact(L, epi, key, what='', **kw):
    offset = kw.get('offset', 0)
    v, amax = _ref(L.case, L.data, epi)
    want = v.to(L.to)
    tag = '%s | %s%s' % (key, epi[0], what)
    y, buf, ya = L.run(epi, **kw)
    got = y.cpu()
    assert _guards_intact(buf, y, offset), '%s: the guard bytes around y were written' % tag
    if torch.isnan(got).any() or not torch.equal(got, want):
        cnt, where, g, w = _first_diff(got, want)
        raise AssertionError('%s: %d of %d outputs differ from the specification, the first at (n, c, y, x) = %s: %r, expected %r' % (
            tag, cnt, got.numel(), where, g, w))
    assert float(ya) == amax, '%s: max|y| %r, expected %r' % (tag, float(ya), amax)
    return got


PARAMS = [(c, st) for c in X.CASES for st in X.storages_of(c)]
# the fp16 -> fp32 kernels first: they ran nowhere before this file
PARAMS.sort(key=lambda cs: cs[1] != X.H32)


@pytest.mark.parametrize('case,storage', PARAMS, ids=['%s-%s' % (c[0].replace(' ', '_'), st) for c, st in PARAMS])
def test_exact(case, storage):
    L = _Launcher(case, storage, _data(case))
    status, d = X.describe(L.lib, case, storage)
    assert status == 0
    key = X.key_of(d)
    for epi in X.EPILOGUES:
        _check_exact(L, epi, key)
        # a running bound in the max|y| scalar stays
        amax = _ref(case, L.data, epi)[1]
        y, buf, ya = L.run(epi, y_amax0=2.0 * amax)
        assert float(ya) == 2.0 * amax, '%s | %s: a running bound of %r became %r' % (key, epi[0], 2.0 * amax, float(ya))
    if storage == X.F32:
        # max|x| may be an upper bound: the same bits with twice the true maximum.  (fp32 input only: the fp16 entry point takes
        # no x_amax, an fp16 activation is the matrix operand unscaled, so the other two storages have no such variant)
        for epi in (X.EPILOGUES[2], X.EPILOGUES[10]):
            _check_exact(L, epi, key, ' (x_amax = 2 max|x|)', x_amax=8.0)
        if len(X.storages_of(case)) == 1:
            # fp16 activations need whole 16-channel chunks per group: refused before any launch
            y = torch.empty(X.shapes_of(case)[1], device='cuda')
            for out16 in (0, 1):
                st = L.lib.dvd_xconv_fwd_h(L._p(L.x), L._p(L.pack('f')), None, None, None, None, L._p(y), None, L.N, L.Cin, L.Cout,
                                           L.H, L.W, L.k, L.G, X.mode_flags(L.mode), out16, L._stream())
                assert st == L._lib.DVD_EINVAL and b'multiples of 16' in L.lib.dvd_last_error()


@pytest.mark.parametrize('storage', X.STORAGES)
@pytest.mark.parametrize('name', X.WIDE_MISALIGNED)
def test_misaligned_operands_take_the_narrow_epilogue(name, storage):
    """residual and y four (fp32) / two (fp16) bytes off a 16-byte boundary: the wide epilogue's 16-byte runs are not allowed,
    the same kernel runs its narrow epilogue and gives the same bits."""
    case = X.CASE[name]
    L = _Launcher(case, storage, _data(case))
    wide, narrow = X.describe(L.lib, case, storage, True)[1], X.describe(L.lib, case, storage, False)[1]
    assert wide['wide'] == 1 and narrow['wide'] == 0 and narrow['fit'] == X.FIT_ONE
    off = 2 if storage == X.H16 else 4
    for epi in (X.EPILOGUES[2], X.EPILOGUES[7], X.EPILOGUES[9]):
        a = _check_exact(L, epi, X.key_of(wide))
        b = _check_exact(L, epi, X.key_of(narrow), ' (operands %d bytes off)' % off, offset=off)
        assert torch.equal(a, b)


# ---- real-valued data, with a bound ------------------------------------------------------------------------------------------
REAL = [('k3 16-24 5x7', X.H32, 7), ('k3 32-40 9x13', X.H32, 7), ('k3 32-72 9x13', X.H32, 7), ('k3 32-288 9x14', X.H32, 7),
        ('k1 32-288 8x18', X.F32, 7), ('k1 32-288 8x18', X.H16, 7), ('k1 32-288 8x18', X.H32, 7),
        ('s2 32-64 11x15', X.F32, 2), ('zi 32-64 11x15', X.F32, 2)]


@pytest.mark.parametrize('name,storage,epi', REAL, ids=['%s-%s' % (n.replace(' ', '_'), s) for n, s, _ in REAL])
def test_real_valued(name, storage, epi):
    """randn data (BatchNorm eps = 1e-5, var in [0.3, 2]) against the specification evaluated on the operands as stored.  Per element

        |y - v| <= 4e-6 max|z| |s_c| + 2^-22 (|z s_c| + |shift_c| + |res'|)   [+ 1.01 * 2^-11 |v| for fp16 output]

    with z = conv + bias and (s_c, shift_c) the BatchNorm pair: the accumulation bound of tests/test_06_xconv_gpu.py carried
    through the linear epilogue, four fp32 roundings of the epilogue's own terms, and the output rounding of
    tests/test_10 (H_EPS).  ReLU is 1-Lipschitz, the mask exact."""
    case, epi = X.CASE[name], X.EPILOGUES[epi]
    d = X.real_data(case)
    d['x'] = d['x'].to(X.IN_DTYPE[storage]).float()                    # the operands as the kernel reads them
    for t in ('residual', 'mask'):
        d[t] = d[t].to(X.OUT_DTYPE[storage]).float()
    L = _Launcher(case, storage, d)
    key = X.key_of(X.describe(L.lib, case, storage)[1])
    xa = float(L.x.abs().max()) if storage == X.F32 else 0.0
    y, buf, ya = L.run(epi, x_amax=xa)
    assert _guards_intact(buf, y, 0)
    p = X.parts(**X.spec_args(case, d, epi))
    s, sh = p['s'][None, :, None, None].abs(), p['shift'][None, :, None, None].abs()
    bound = 4e-6 * float(p['z'].abs().max()) * s + 2.0 ** -22 * ((p['z'] * s).abs() + sh + p['res'].abs())
    if storage == X.H16:
        bound = bound + 1.01 * 2.0 ** -11 * p['v'].abs()
    got = y.cpu().double()
    assert torch.isfinite(got).all()
    ratio = float(((got - p['v']).abs() / bound).max())
    print('%s | %s: worst |y - v| / bound = %.3f' % (key, epi[0], ratio))
    helpers.log_measured('test_69 real %s %s' % (name, storage), ratio, 1.0)
    assert ratio <= 1.0, '%s | %s: |y - v| reaches %.3f of the bound' % (key, epi[0], ratio)
    ref_amax = float(p['v'].abs().max())
    assert abs(float(ya) - ref_amax) <= float(bound.max()) + 2.0 ** -11 * ref_amax
