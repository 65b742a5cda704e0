"""The grid-stride kernels of csrc/a16.hip, csrc/pool.hip and csrc/gather.hip BEYOND their launch caps.

Each of these kernels launches at most a fixed number of blocks and covers the rest of the tensor in further trips of a
grid-stride loop, where an item's image / plane / tensor index is recomputed from the flat index.  At the shipped workload every
launch is far beyond its cap; the shapes here are the smallest that reach a second trip with a ragged last trip and an image
(plane, pair) boundary inside it.

All inputs are small integers (tests/boundary_spec.py; tests/test_boundary_spec_cpu.py proves on the CPU that every sum stays
below 2^24 and every stored value is exact in its format), so the kernels' fp32 / fp16 arithmetic is exact in any order and
every result must EQUAL the float64 reference (cast to the kernel's storage) bit for bit: one dropped, duplicated or misplaced
item fails, whatever the summation order."""
import ctypes

import pytest
import torch

import boundary_spec as S

pytestmark = pytest.mark.gpu

# ---- the launch caps, as the kernels' host code has them ---------------------------------------------------------------
A16_BLOCK = 256                 # csrc/a16.hip:384  blocks_for: `(items + 255) / 256` -- items per block
A16_MAX_BLOCKS = 2048           # csrc/a16.hip:385  blocks_for: `if (b > 2048) b = 2048`
A16_CAP_ITEMS = A16_MAX_BLOCKS * A16_BLOCK          # 524 288 items in one trip (head1x1: 4 pixels per item; add_f16 vector: 4)
H3_WGRAD_MAX_CHUNKS = 256       # csrc/a16.hip:359  head3x3_chunks: `c > 256 ? 256 : c`
H3_WGRAD_CHUNK_PIXELS = 1024    # csrc/a16.hip:358  head3x3_chunks: `(total + 1023) / 1024`
H3_WGRAD_CAP_PIXELS = H3_WGRAD_MAX_CHUNKS * H3_WGRAD_CHUNK_PIXELS      # 262 144 pixels: beyond it a chunk outgrows 1 024
SUBSAMPLE_MAX_BLOCKS = 16384    # csrc/pool.hip:222 and :236  `if (blocks > 16384) blocks = 16384` (blocks of 256)
SUBSAMPLE_CAP_ITEMS = SUBSAMPLE_MAX_BLOCKS * 256    # 4 194 304
AVGPOOL_MAX_BLOCKS = 32768      # csrc/pool.hip:253 and :270  `if (blocks > 32768) blocks = 32768` (blocks of 256)
AVGPOOL_CAP_ITEMS = AVGPOOL_MAX_BLOCKS * 256        # 8 388 608
GATHER_MAX_TILES = 4096         # csrc/gather.hip:115  `tiles < 4096 ? tiles : 4096` (one block per tile)

DEV = torch.device('cuda')
_CACHE = {}


def _shared(key, make):
    """One reference at a time, shared by the parameter cases that follow each other; the previous one is freed."""
    if key not in _CACHE:
        _CACHE.clear()
        torch.cuda.empty_cache()
        _CACHE[key] = make()
    return _CACHE[key]


@pytest.fixture(autouse=True, scope='module')
def _free_references():
    yield
    _CACHE.clear()
    torch.cuda.empty_cache()


@pytest.fixture
def state():
    from dvd_hip import conv as C, ops
    st = ops.gscale_new(DEV)
    C.set_grad_scale_state(st)
    yield st
    C.set_grad_scale_state(None)


FRESH = [1.0, 1.0, 4.0] + [0.0] * 13


def _same(got, want64, what='result'):
    """The kernel's tensor against the float64 reference cast to the kernel's storage, bit for bit.  A failure says how many
    elements differ and where the first one is (its flat index tells the trip of the grid-stride loop it belongs to)."""
    got, want = got.detach(), want64.to(got.dtype).to(got.device)
    assert got.shape == want.shape, '%s: shape %s, expected %s' % (what, tuple(got.shape), tuple(want.shape))
    if not torch.equal(got, want):
        bad = (got != want).reshape(-1).nonzero().reshape(-1)
        i = int(bad[0])
        raise AssertionError('%s: %d of %d elements differ, the first at flat index %d: %r, expected %r' % (
            what, bad.numel(), got.numel(), i, float(got.reshape(-1)[i]), float(want.reshape(-1)[i])))
    return True


def _head_checks(conv, run, x, gy, ref, dtype, st):
    f16 = dtype == torch.float16
    scale = 2.0 if f16 else 1.0                     # max|gy| * max|w| = 4 and the initial target 4: S = 2 (fp32 features: none)
    xg = x.to(dtype).to(DEV).requires_grad_(True)
    gyd = gy.float().to(DEV)
    y = run(xg)
    assert y.dtype == torch.float32 and _same(y, ref['y'], 'y')
    if f16:
        assert float(st[6]) == float(ref['y'].abs().max())
    passes = []
    for _ in range(2):                               # a second backward gives the same bits
        xg.grad = conv.weight.grad = conv.bias.grad = None
        st[3] = 0.0
        y.backward(gyd, retain_graph=True)
        passes.append((xg.grad, conv.weight.grad, conv.bias.grad, st.tolist()))
    gx, gw, gb, after = passes[0]
    assert gx.dtype == dtype and _same(gx, scale * ref['gx'], 'gx')
    assert _same(gw.view(-1), ref['gw'].reshape(-1), 'gw') and _same(gb, ref['gb'], 'gb')
    if f16:
        assert after[0] == 2.0 and after[1] == 0.5
        assert after[3] == float((scale * ref['gx']).abs().max())
    else:
        assert after == FRESH                        # fp32 features carry no loss scale
    for a, b in zip(passes[0][:3], passes[1][:3]):
        assert torch.equal(a, b)
    assert passes[0][3] == passes[1][3]


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32], ids=['f16', 'f32'])       # (the upper one varies fastest)
@pytest.mark.parametrize('relu_in', [True, False], ids=['relu', 'norelu'])
def test_head1x1_beyond_the_block_cap_is_exact(dtype, relu_in, state):
    """conv.head1x1 at 5 x 3 x 500 x 1000: 625 000 four-pixel items against one trip of 524 288 -- the second trip starts
    inside image 4 and fills 394 blocks, the last of them partly."""
    from dvd_hip import conv as C

    def make():
        x, w, b, gy = S.head1x1_exact_inputs()
        return x, w, b, gy, S.head1x1_ref(x, w, b, gy, relu_in)
    x, w, b, gy, ref = _shared(('head1x1', relu_in), make)
    N, Cc, H, W = x.shape
    assert N * (H * W // 4) > A16_CAP_ITEMS
    conv = torch.nn.Conv2d(Cc, 1, 1).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(w.view(1, Cc, 1, 1))
        conv.bias.copy_(b)
    _head_checks(conv, lambda t: C.head1x1(conv, t, relu_in=relu_in), x, gy, ref, dtype, state)


def test_head3x3_beyond_the_block_and_chunk_caps_is_exact(state):
    """conv.head3x3 at 3 x 5 x 300 x 700 (fp16): 630 000 pixels against 524 288 per trip of the forward / backward-data
    kernels, and against the 262 144 beyond which the weight gradient's 256 chunks outgrow 1 024 pixels (2 461 here: ten
    trips per thread, chunks that straddle the images); C = 5 leaves three of the eight channel slots of a block empty."""
    from dvd_hip import conv as C
    x, w, b, gy = S.head3x3_exact_inputs()
    N, Cc, H, W = x.shape
    assert N * H * W > A16_CAP_ITEMS and N * H * W > H3_WGRAD_CAP_PIXELS and Cc % 8
    ref = S.head3x3_ref(x, w, b, gy)
    conv = torch.nn.Conv2d(Cc, 1, 3, padding=1).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    assert C.head3x3_supported(conv, x.half().to(DEV))
    _head_checks(conv, lambda t: C.head3x3(conv, t), x, gy, ref, torch.float16, state)


GUARD = 777.0


def _offset_view(values, offset):
    """A contiguous fp16 view `offset` elements into a guard-filled device buffer, holding `values` (None: left as guards)."""
    n = values if isinstance(values, int) else values.numel()
    buf = torch.full((n + 16,), GUARD, device=DEV, dtype=torch.float16)
    view = buf[offset:offset + n]
    if not isinstance(values, int):
        view.copy_(values.to(DEV))
    return buf, view


@pytest.mark.parametrize('n,offset,vector', [(S.ADD_F16_VEC_N, 4, True), (S.ADD_F16_SCALAR_N, 4, False),
                                             (S.ADD_F16_VEC_N, 1, False)], ids=['vector', 'odd', 'misaligned'])
def test_add_f16_beyond_the_block_cap_is_exact(n, offset, vector, state):
    """dvd_add_f16 on its vector path (n % 4 == 0, 8-byte aligned: 525 001 groups of four against 524 288 per trip) and on
    its scalar path, taken for an odd n and for views that start 2 bytes into their buffers: through conv.add_f16, and once
    more into a view between guard elements, which must stay untouched."""
    from dvd_hip import _lib, conv as C
    from dvd_hip.ops import _p, _stream
    a, b = S.add_f16_exact_inputs(n)
    want = a + b
    (_, av), (_, bv) = _offset_view(a, offset), _offset_view(b, offset)
    assert av.is_contiguous() and av.data_ptr() % 8 == bv.data_ptr() % 8 == (2 * offset) % 8
    assert vector == (n % 4 == 0 and av.data_ptr() % 8 == 0)
    assert (n // 4 if vector else n) > A16_CAP_ITEMS
    y = C.add_f16(av, bv)
    assert y.dtype == torch.float16 and _same(y, want, 'y')
    assert float(state[6]) == float(want.abs().max())
    state[6] = 0.0
    ybuf, yv = _offset_view(n, offset)
    _lib.check(_lib.load().dvd_add_f16(_p(av), _p(bv), _p(yv), ctypes.c_longlong(n), _p(state[6:7]), _stream()), 'dvd_add_f16')
    assert _same(yv, want, 'y between the guards') and float(state[6]) == float(want.abs().max())
    assert bool((ybuf[:offset] == GUARD).all()) and bool((ybuf[offset + n:] == GUARD).all())


@pytest.mark.parametrize('n', S.TO_HALF_N)
def test_to_half_backward_beyond_the_block_cap_is_exact(n, state):
    """The backward of conv.to_half (dvd_cast_scale_f32: 525 001 groups of four against 524 288 per trip; n % 4 != 0: the
    ATen expression) hands the fp32 stem the fp16 gradient times state[1], here 1 / 8: exact for every fp16 value."""
    from dvd_hip import conv as C
    g = S.small_ints((n,), 41, -1000, 1000)
    if n % 4 == 0:
        assert n // 4 > A16_CAP_ITEMS
    state[1] = 0.125
    x = torch.zeros(n, device=DEV, requires_grad=True)
    C.to_half(x).backward(g.half().to(DEV))
    assert x.grad.dtype == torch.float32 and _same(x.grad, g * 0.125, 'gradient')


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16], ids=['f32', 'f16'])
def test_subsample2_beyond_the_block_cap_is_exact(dtype):
    """conv._subsample(x, 2) at 3 x 4 x 1201 x 1403 (odd both ways): 5.06 M outputs and 10.1 M backward pairs against
    4 194 304 per trip."""
    from dvd_hip import conv as C

    def make():
        x, gy = S.pool_exact_inputs(S.SUBSAMPLE_SHAPE, S.subsample_out_shape(S.SUBSAMPLE_SHAPE), 1, 1024, 51)
        x, gy = x.to(DEV), gy.to(DEV)
        return (x, gy) + S.subsample_ref(x, gy)
    x, gy, y_ref, gx_ref = _shared('subsample', make)
    N, Cc, H, W = x.shape
    assert y_ref.numel() > SUBSAMPLE_CAP_ITEMS and N * Cc * H * ((W + 1) // 2) > SUBSAMPLE_CAP_ITEMS
    a = x.to(dtype, copy=True).requires_grad_(True)          # (a leaf of its own: x is shared between the cases)
    y = C._subsample(a, 2)
    assert type(y.grad_fn).__name__.startswith('_Subsample2')
    assert y.is_contiguous() and y.dtype == dtype and _same(y, y_ref, 'y')
    y.backward(gy.to(dtype))
    assert a.grad.dtype == dtype and _same(a.grad, gx_ref, 'gx')


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16], ids=['f32', 'f16'])
@pytest.mark.parametrize('k,st,pad', S.AVGPOOL_CFGS)
def test_avgpool_beyond_the_block_cap_is_exact(dtype, k, st, pad):
    """conv.AvgPool2d(2) and AvgPool2d(3, 2, 1) at 4 x 6 x 1201 x 1403: 10.1 M outputs and 40.4 M inputs against 8 388 608
    per trip.  The values are 36 * {-3..3}: multiples of 4 and of 9, so every window mean and every gy / k^2 is an integer."""
    from dvd_hip import conv as C

    def make():
        x, gy = S.pool_exact_inputs(S.AVGPOOL_SHAPE, S.avgpool_out_shape(S.AVGPOOL_SHAPE, k, st, pad), 36, 3, 61)
        x, gy = x.to(DEV), gy.to(DEV)
        y_ref, gx_ref = S.avgpool_ref(x, k, st, pad, gy)
        return x, gy, y_ref.float(), gx_ref.float()          # (exact: tests/test_boundary_spec_cpu.py)
    x, gy, y_ref, gx_ref = _shared(('avgpool', k, st, pad), make)
    assert y_ref.numel() > AVGPOOL_CAP_ITEMS and x.numel() > AVGPOOL_CAP_ITEMS
    a = x.to(dtype, copy=True).requires_grad_(True)          # (a leaf of its own: x is shared between the cases)
    y = C.AvgPool2d(k, st, pad)(a)
    assert type(y.grad_fn).__name__.startswith('_AvgPool')
    assert y.dtype == dtype and _same(y, y_ref, 'y')
    y.backward(gy.to(dtype))
    assert a.grad.dtype == dtype and _same(a.grad, gx_ref, 'gx')
    del a, y


@pytest.mark.parametrize('launch', [S.GATHER_LAUNCH_1, S.GATHER_LAUNCH_2], ids=['uint4_then_small', 'dword'])
def test_gather_pairs_beyond_the_tile_cap_is_exact(launch):
    """ops.gather_pairs with more tiles than the 4 096 blocks of a launch.  First launch: a (5, 3 500 000) fp32 tensor on
    the 16-byte path (855 tiles per pair, 4 275 tiles) in front of three small tensors, whose tiles only the second trip
    reaches; second launch: (5, 1 000 001) fp32 on the dword path (977 tiles per pair)."""
    from dvd_hip import ops
    tiles = S.gather_tiles(launch)
    assert S.GATHER_B * sum(t for t, _ in tiles) > GATHER_MAX_TILES
    tensors = [t.to(DEV) for t in S.gather_inputs(launch, 71)]
    assert all(t.data_ptr() % 16 == 0 for t in tensors)
    perm = torch.randperm(S.GATHER_B, generator=torch.Generator().manual_seed(79))
    assert sorted(perm.tolist()) == list(range(S.GATHER_B)) and bool((perm != torch.arange(S.GATHER_B)).all())
    out = ops.gather_pairs(tensors, perm.to(DEV))
    for t, o in zip(tensors, out):
        assert o.dtype == t.dtype and o.shape == t.shape
        assert _same(o, torch.index_select(t, 0, perm.to(DEV)), 'permuted %s' % (tuple(t.shape),))
    for t, o in zip(tensors, ops.gather_pairs(tensors, list(range(S.GATHER_B)))):
        assert _same(o, t, 'identity %s' % (tuple(t.shape),))
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(S.GATHER_B)
    for t, o in zip(tensors, ops.gather_pairs(out, inv.to(DEV).to(torch.int32))):
        assert _same(o, t, 'permuted and back %s' % (tuple(t.shape),))
