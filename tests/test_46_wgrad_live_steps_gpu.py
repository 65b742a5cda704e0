"""The row-walking weight-gradient kernels (csrc/xwgrad3.hip: xwgrad3_kernel, xwgrad3g_kernel, xwgradk_kernel) run only the
K steps of a 64-pixel strip that hold pixels of the row -- NK = ceil(min(64, W - c0) / 16), a template parameter, one launch per
strip class -- and cut every launch into slices of equal row counts (csrc/wg3_plan.h).  What replaces the reference's autograd
weight gradient of nn.Conv2d (third_party/midas_blocks.py:102-168, MiDaS.py:186-195, hourglass.py:21-57).

Every case compares against float64 F.conv2d autograd on the CPU:
  * fp32 operands: max |err| <= 2e-5 * max |dW| (the bound of tests/test_06_xconv_gpu.py);
  * fp16 operands (even widths): the same 2e-5 * max |dW| against the float64 gradient of the fp16-rounded tensors (the bound
    tests/test_10_act_fp16_gpu.py applies to the H16 weight gradient);
  * the row sums of dvd_xwgrad3_rowsum: L * 2^-24 * sum|g| per channel, L the longest add chain of the launch (the bound of
    tests/test_40_wgrad_rowsum_gpu.py), counted below from the plan the way the kernel walks it.
Widths: 5 / 21 / 42 / 64 (NK 1 .. 4), 70 / 84 / 100 (a full strip and an NK 1 / 2 / 3 tail), 168 (the 96x168 level); heights
9 .. 24 and 1 .. 3 images, so that slices end inside strips and cross images; 64 -> 64 and 80 -> 72 channels (ragged blocks);
grouped 32 and 16 per group; KS = 5 at W = 37 and 70.  The stale-LDS cases put values of 1e3 next to values of 1 in neighbouring
strips: what one segment of the walk leaves in LDS must never reach the next one's products.  Two calls give the same bits, and
the round-robin deal kept for A/B (dvd_xwgrad_select(3)) meets the same bound."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from helpers import log_measured

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TOL = 2e-5


def _ceil(a, b):
    return (a + b - 1) // b


def _ref(x, gy, Cout, Cin_g, KS, G, relu_in):
    xd = x.double().relu() if relu_in else x.double()
    wd = torch.zeros(Cout, Cin_g, KS, KS, dtype=torch.float64, requires_grad=True)
    F.conv2d(xd, wd, None, padding=KS // 2, groups=G).backward(gy.double())
    return wd.grad


def _call(x, gy, KS, G, relu_in, sums=False, half=False):
    """-> (gw, row sums or None) through the C entry points, the workspace pre-filled with NaNs."""
    from dvd_hip import _lib
    from dvd_hip.ops import _p, _stream, amax
    lib = _lib.load()
    N, Cin, H, W = x.shape
    Cout = gy.shape[1]
    xc, gc = x.cuda(), gy.cuda()
    gw = torch.full((Cout, Cin // G, KS, KS), float('nan'), device='cuda')
    dims = (N, Cin, Cout, H, W) + ((G,) if KS == 3 else (KS,))
    nws = (lib.dvd_xwgrad3_workspace_bytes if KS == 3 else lib.dvd_xwgradk_workspace_bytes)(*dims)
    ws = torch.full((nws,), 0xff, device='cuda', dtype=torch.uint8)          # NaNs: a partial that nobody wrote shows
    tail = (_p(ws), ctypes.c_size_t(nws)) + dims + (int(relu_in), _stream())
    rs = torch.full((Cout,), float('nan'), device='cuda') if sums else None
    if half:
        xc, gc = xc.half(), gc.half()
        name = 'dvd_xwgrad3_h' if KS == 3 else 'dvd_xwgradk_h'
        _lib.check(getattr(lib, name)(_p(xc), _p(gc), _p(None), _p(gw), *tail), name)
    else:
        xa, ga = amax(xc), amax(gc)
        if sums:
            _lib.check(lib.dvd_xwgrad3_rowsum(_p(xc), _p(xa), _p(gc), _p(ga), _p(gw), _p(rs), *tail), 'dvd_xwgrad3_rowsum')
        else:
            name = 'dvd_xwgrad3' if KS == 3 else 'dvd_xwgradk'
            _lib.check(getattr(lib, name)(_p(xc), _p(xa), _p(gc), _p(ga), _p(gw), *tail), name)
    torch.cuda.synchronize()
    return gw, rs


def _err(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


def _data(N, Cin, Cout, H, W, seed, half=False):
    g = torch.Generator().manual_seed(seed)
    x, gy = torch.randn(N, Cin, H, W, generator=g), torch.randn(N, Cout, H, W, generator=g)
    if half:
        x, gy = x.half().float(), gy.half().float()
    return x, gy


def _check(tag, x, gy, KS, G, relu_in, half=False):
    want = _ref(x, gy, gy.shape[1], x.shape[1] // G, KS, G, relu_in)
    gw, _ = _call(x, gy, KS, G, relu_in, half=half)
    e = _err(gw, want)
    log_measured('wgrad live steps %s: of max|dW|' % tag, e, TOL)
    print('%s: |err| / max|dW| = %.3g (bound %.3g)' % (tag, e, TOL))
    assert bool(torch.isfinite(gw).all()) and e <= TOL, '%s: %.3g of max|dW|' % (tag, e)
    return want, gw


# N, Cin, Cout, H, W, relu_in
DENSE = [
    (1, 64, 64, 9, 5, 0),         # NK 1
    (2, 80, 72, 12, 21, 1),       # NK 2; ragged channel blocks
    (3, 64, 64, 17, 42, 0),       # NK 3; slices end inside strips and cross images
    (2, 80, 72, 24, 64, 0),       # NK 4, one strip
    (2, 64, 64, 9, 70, 1),        # a full strip and an NK 1 tail
    (3, 80, 72, 24, 84, 0),       # ... an NK 2 tail; nine slices per launch, three to a strip
    (2, 64, 64, 13, 100, 0),      # ... an NK 3 tail
    (1, 80, 72, 16, 168, 1),      # W of the 96x168 level: two full strips and an NK 3 tail
]


@pytest.mark.parametrize('N,Cin,Cout,H,W,relu_in', DENSE)
def test_dense_3x3(N, Cin, Cout, H, W, relu_in):
    x, gy = _data(N, Cin, Cout, H, W, 46 + W)
    _check('3x3 %dx%d->%d %dx%d' % (N, Cin, Cout, H, W), x, gy, 3, 1, relu_in)


@pytest.mark.parametrize('N,Cin,Cout,H,W,relu_in', [c for c in DENSE if c[4] % 2 == 0])
def test_dense_3x3_fp16(N, Cin, Cout, H, W, relu_in):
    x, gy = _data(N, Cin, Cout, H, W, 146 + W, half=True)
    _check('3x3 fp16 %dx%d->%d %dx%d' % (N, Cin, Cout, H, W), x, gy, 3, 1, relu_in, half=True)


def _chain_3x3g(N, G, H, W):
    """The longest add chain of a row-sum accumulator of xwgrad3g_kernel<fp32, RSUM>, from the plan (csrc/wg3_plan.h wg3g_plan;
    one 32 x 32 block per group): a slice of a launch walks at most q + 1 rows in at most ceil(q / H) + 2 segments; per segment
    the accumulator takes three prologue stores, per row one (4 values: 2 adds, then 1); then the butterfly over the 16 lanes
    of a row (4) and the rounding of the double sum over the slices."""
    nstrips = _ceil(W, 64)
    wt = W - 64 * (nstrips - 1)
    nkt = _ceil(wt, 16)
    S = 1 if G >= 512 else _ceil(512, G)
    RS = H
    while RS > 8 and N * nstrips * _ceil(H, RS) < 4 * S:
        RS = (RS + 1) // 2
    S = min(S, N * nstrips * _ceil(H, RS))
    if nstrips == 1 or nkt == 4:
        launches = [(nstrips, S)]
    else:
        Sc = max(1, min(512 // G, N * H // 8))
        launches = [(nstrips - 1, Sc), (1, Sc)]
    L = 0
    for ncols, Sl in launches:
        q = N * ncols * H // Sl
        L = max(L, 2 + (q + 1) + 3 * (_ceil(q, H) + 2) + 4 + 1)
    return L


# N, C, G, H, W, relu_in: 32 per group (G = 3) and 16 per group (G = 4)
GROUPED = [
    (1, 96, 3, 10, 5, 0),
    (1, 96, 3, 12, 21, 1),
    (2, 64, 4, 17, 42, 0),
    (2, 96, 3, 9, 64, 0),
    (2, 96, 3, 9, 70, 1),
    (3, 64, 4, 24, 84, 0),
    (2, 64, 4, 11, 100, 1),
    (1, 96, 3, 16, 168, 0),
]


@pytest.mark.parametrize('N,C,G,H,W,relu_in', GROUPED)
def test_grouped_3x3_and_row_sums(N, C, G, H, W, relu_in):
    from dvd_hip import _lib
    x, gy = _data(N, C, C, H, W, 246 + W)
    tag = '3x3 grouped %dx%d g%d %dx%d' % (N, C, G, H, W)
    want, gw = _check(tag, x, gy, 3, G, relu_in)
    assert _lib.load().dvd_xwgrad_rowsum_in_kernel(N, C, C, H, W, 3, G) == 1
    gw_s, sums = _call(x, gy, 3, G, relu_in, sums=True)
    e = _err(gw_s, want)
    assert bool(torch.isfinite(gw_s).all()) and e <= TOL, '%s (RSUM): %.3g of max|dW|' % (tag, e)
    L = _chain_3x3g(N, G, H, W)
    err = float(((sums.double().cpu() - gy.double().sum((0, 2, 3))).abs() / gy.double().abs().sum((0, 2, 3))).max())
    log_measured('wgrad live steps %s row sums: of sum|g|' % tag, err, L * U)
    print('%s: row sums L = %d, |err| / sum|g| = %.3g (bound %.3g)' % (tag, L, err, L * U))
    assert bool(torch.isfinite(sums).all()) and err <= L * U, '%s: row sums %.3g of sum|g| > %d * 2^-24' % (tag, err, L)


@pytest.mark.parametrize('N,C,G,H,W,relu_in', [c for c in GROUPED if c[4] % 2 == 0])
def test_grouped_3x3_fp16(N, C, G, H, W, relu_in):
    x, gy = _data(N, C, C, H, W, 346 + W, half=True)
    _check('3x3 grouped fp16 %dx%d g%d %dx%d' % (N, C, G, H, W), x, gy, 3, G, relu_in, half=True)


@pytest.mark.parametrize('N,Cin,Cout,H,W,half', [(2, 12, 40, 21, 37, False), (2, 12, 40, 24, 70, False), (2, 12, 40, 24, 70, True)])
def test_5x5(N, Cin, Cout, H, W, half):
    x, gy = _data(N, Cin, Cout, H, W, 446 + W, half=half)
    _check('5x5 %s%dx%d->%d %dx%d' % ('fp16 ' if half else '', N, Cin, Cout, H, W), x, gy, 5, 1, 0, half=half)


@pytest.mark.parametrize('G', [1, 3])
@pytest.mark.parametrize('large_in_tail', [False, True])
def test_no_lds_leak_between_segments(G, large_in_tail):
    """W = 70, two images: columns 8 .. 63 of x and gy are about 1e3 and the tail strip's columns about 1 (and the mirror case).
    The segments of a slice follow each other through the same LDS rows: data of the neighbouring strip that a segment found
    there would show as a gross error against float64."""
    N, C, H, W = 2, 64 if G == 1 else 96, 12, 70
    x, gy = _data(N, C, C, H, W, 546 + G)
    big = torch.ones(W)
    if large_in_tail:
        big[64:] = 1e3
    else:
        big[8:64] = 1e3
    x, gy = x * big, gy * big
    _check('3x3 g%d W 70, 1e3 %s' % (G, 'in the tail strip' if large_in_tail else 'in columns 8..63'), x, gy, 3, G, 0)


@pytest.mark.parametrize('KS,N,Cin,Cout,G,H,W', [(3, 3, 80, 72, 1, 24, 84), (3, 2, 96, 96, 3, 9, 70), (5, 2, 12, 40, 1, 24, 70)])
def test_deterministic_and_the_deal_meets_the_bound(KS, N, Cin, Cout, G, H, W):
    from dvd_hip import _lib
    lib = _lib.load()
    x, gy = _data(N, Cin, Cout, H, W, 646 + KS + G)
    want = _ref(x, gy, Cout, Cin // G, KS, G, 0)
    a, _ = _call(x, gy, KS, G, 0)
    b, _ = _call(x, gy, KS, G, 0)
    assert torch.equal(a, b), 'two calls on the same inputs differ'
    assert _err(a, want) <= TOL
    try:
        _lib.check(lib.dvd_xwgrad_select(3), 'dvd_xwgrad_select')
        d, _ = _call(x, gy, KS, G, 0)
    finally:
        _lib.check(lib.dvd_xwgrad_select(0), 'dvd_xwgrad_select')
    e = _err(d, want)
    print('k%d %dx%d->%d g%d %dx%d: the deal %.3g, the class launches %.3g of max|dW|' % (KS, N, Cin, Cout, G, H, W, e, _err(a, want)))
    assert bool(torch.isfinite(d).all()) and e <= TOL
