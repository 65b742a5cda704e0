"""Per-channel sums of the output gradient from the weight-gradient kernels that stage it anyway (csrc/xwgrad3.hip, the RSUM
forms of xwgrad1b_kernel<fp32, FW> and xwgrad3g_kernel<fp32>; entry points dvd_xwgrad1s_rowsum / dvd_xwgrad3_rowsum): the shift
gradient of a BatchNorm fused behind the convolution (torchvision's Bottleneck behind third_party/midas_blocks.py:35-50), which
conv._XConvBn.backward takes from there instead of a pass of its own over the gradient.

Every case asserts
  (a) the weight gradient is bit-identical to the same call without the sums pointer,
  (b) two runs give bit-identical sums,
  (c) against float64 gy.sum((0, 2, 3)) every channel is within L * 2^-24 * sum|g| of that channel: the bound of fp32
      summation along an add chain of depth L (each add rounds by at most 2^-24 of a partial sum, which is at most sum|g|).
      L is the longest per-thread add chain of the launch, counted below from the slice count and the shape the way the kernel
      walks them (adds of the zeros of idle stages included); the partials of the slices are added in double.
The shapes are the smallest that reach each path: one and several chunks per slice, an odd chunk count that the slices do not
divide (the zero chunk of the pair loop, slices that cross images), a partial output-channel block, two input-channel blocks
(one reports), the non-FW and narrow routes (fallback pass); grouped: 32 and 16 per group, rows of 42 and 21 pixels (runs that
cross row ends), two column strips, several row segments per image (the look-ahead row past a segment must not count twice)."""
import ctypes

import pytest
import torch

from helpers import log_measured

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _ceil(a, b):
    return (a + b - 1) // b


def _chain_chansum(N, HW):
    """chansum_kernel: 256 threads stride over the N * HW elements of a channel, a 64-lane butterfly, a tree over four waves."""
    return N * _ceil(HW, 256) + 6 + 2


def _chain_1x1(N, Cin, Cout, HW):
    """-> (L, route).  The wide FW kernel (csrc/xwgrad3.hip wg_route, KS = 1): a slice is n_it consecutive 16-pixel
    chunks; a lane adds, per chunk it stores (two in the prologue, two per pair of the loop), the quad's tree (2 adds), the fold
    across lanes (1) and BOTH gy items into its accumulator (its own row's, and a zero for the other row); then one add across
    lanes and the rounding of the double sum over the slices."""
    if not (Cin >= 192 and Cout >= 192 and HW % 4 == 0 and HW % 16 == 0):
        return _chain_chansum(N, HW), 'pass'
    pairs = _ceil(Cout, 256) * _ceil(Cin, 256)
    items = N * (HW // 16)
    S = min(1 if pairs >= 256 else _ceil(256, pairs), items)
    n_it = max(items * (s + 1) // S - items * s // S for s in range(S))
    stored = 2 + 2 * _ceil(n_it, 2)
    return 3 + 2 * stored + 1 + 1, 'kernel S=%d n_it<=%d' % (S, n_it)


def _chain_3x3(N, Cin, Cout, H, W, G):
    """-> (L, route).  The 32 x 32 grouped kernel (wg_route, wg3g_plan): a slice walks ceil(items / S) work items of at most RS
    rows; per item a thread's accumulator takes three prologue stores and one store per row (4 values: 2 adds, then 1), then the
    butterfly over the 16 lanes of a row (4) and the rounding of the double sum over the slices."""
    if not (G > 1 and Cin // G <= 32 and Cout // G <= 32):
        return _chain_chansum(N, H * W), 'pass'
    nstrips = _ceil(W, 64)
    S = 1 if G >= 512 else _ceil(512, G)
    RS = H
    while RS > 8 and N * nstrips * _ceil(H, RS) < 4 * S:
        RS = (RS + 1) // 2
    items = N * nstrips * _ceil(H, RS)
    S = min(S, items)
    return 2 + _ceil(items, S) * (3 + RS) + 4 + 1, 'kernel S=%d RS=%d items=%d' % (S, RS, items)


def _run(ks, N, Cin, Cout, H, W, G, with_sums):
    from dvd_hip import _lib
    from dvd_hip.ops import _p, _stream, amax
    lib = _lib.load()
    g = torch.Generator().manual_seed(1000 * ks + Cin + Cout + H * W)
    x = torch.randn(N, Cin, H, W, generator=g).cuda()
    gy = torch.randn(N, Cout, H, W, generator=g).cuda()          # seeded, zero mean
    xa, ga = amax(x), amax(gy)
    gw = torch.empty(Cout, Cin // G, ks, ks, device='cuda')
    dims = (N, Cin, Cout, H, W) + ((G,) if ks == 3 else ())
    nws = getattr(lib, 'dvd_xwgrad3_workspace_bytes' if ks == 3 else 'dvd_xwgrad1s_workspace_bytes')(*dims)
    ws = torch.full((nws,), 0xff, device='cuda', dtype=torch.uint8)          # NaNs: a partial that nobody wrote shows
    sums = torch.full((Cout,), float('nan'), device='cuda') if with_sums else None
    tail = (_p(ws), ctypes.c_size_t(nws)) + dims + (0, _stream())
    if with_sums:
        name = 'dvd_xwgrad3_rowsum' if ks == 3 else 'dvd_xwgrad1s_rowsum'
        _lib.check(getattr(lib, name)(_p(x), _p(xa), _p(gy), _p(ga), _p(gw), _p(sums), *tail), name)
    else:
        name = 'dvd_xwgrad3' if ks == 3 else 'dvd_xwgrad1s'
        _lib.check(getattr(lib, name)(_p(x), _p(xa), _p(gy), _p(ga), _p(gw), *tail), name)
    torch.cuda.synchronize()
    return gy, gw, sums


def _check(ks, N, Cin, Cout, H, W, G, L, route, want_route):
    from dvd_hip import _lib
    assert route.startswith(want_route), 'the case is meant for the %s route, the planner says %s' % (want_route, route)
    assert _lib.load().dvd_xwgrad_rowsum_in_kernel(N, Cin, Cout, H, W, ks, G) == int(want_route == 'kernel')
    gy, gw, sums = _run(ks, N, Cin, Cout, H, W, G, True)
    _, gw_plain, _ = _run(ks, N, Cin, Cout, H, W, G, False)
    _, gw2, sums2 = _run(ks, N, Cin, Cout, H, W, G, True)
    assert bool(torch.isfinite(gw).all()) and torch.equal(gw, gw_plain), '(a) the weight gradient changed with the sums pointer'
    assert torch.equal(gw, gw2) and torch.equal(sums, sums2), '(b) the sums differ from run to run'
    want = gy.double().sum((0, 2, 3))
    scale = gy.double().abs().sum((0, 2, 3))
    err = float(((sums.double() - want).abs() / scale).max())
    log_measured('wgrad rowsum k%d %dx%d->%d g%d %dx%d (%s): of sum|g|' % (ks, N, Cin, Cout, G, H, W, route), err, L * U)
    print('k%d N%d %d->%d g%d %dx%d %s: L = %d, |err| / sum|g| = %.3g (bound %.3g)' % (ks, N, Cin, Cout, G, H, W, route, L, err, L * U))
    assert bool(torch.isfinite(sums).all()) and err <= L * U, '(c) %.3g of sum|g| > %d * 2^-24' % (err, L)


@pytest.mark.parametrize('N,Cin,Cout,H,W,route', [
    (2, 256, 256, 8, 8, 'kernel'),        # one chunk per slice: the second chunk of the pair loop is the zero chunk
    (3, 256, 320, 16, 47, 'kernel'),      # 141 chunks over 128 slices (1 or 2 each, slices cross images); rows past Cout in block 1
    (2, 512, 256, 8, 24, 'kernel'),       # two input-channel blocks: one reports
    (4, 1024, 1024, 20, 20, 'kernel'),    # 16 slices of 6 or 7 chunks (odd counts), 4 x 4 channel blocks
    (2, 256, 256, 12, 21, 'pass'),        # H * W = 252: rows of whole quads but no whole chunks -> the round-3 row step + the pass
    (2, 256, 64, 8, 8, 'pass'),           # narrow: the 128 x 128 kernel + the pass
])
def test_dense_1x1_rowsum(N, Cin, Cout, H, W, route):
    L, got = _chain_1x1(N, Cin, Cout, H * W)
    _check(1, N, Cin, Cout, H, W, 1, L, got, route)


@pytest.mark.parametrize('N,C,G,H,W,route', [
    (2, 1024, 32, 24, 42, 'kernel'),      # 32 per group, rows of 42 pixels, four row segments of 6 rows per image
    (2, 1024, 32, 12, 21, 'kernel'),      # rows of 21 pixels: every run crosses a row end or starts past it
    (3, 512, 32, 10, 72, 'kernel'),       # 16 per group (half a channel block), two column strips, two row segments
    (2, 256, 4, 9, 20, 'pass'),           # 64 per group: the 64 x 64 kernel + the pass
    (2, 64, 1, 9, 20, 'pass'),            # dense 3x3
])
def test_grouped_3x3_rowsum(N, C, G, H, W, route):
    L, got = _chain_3x3(N, C, C, H, W, G)
    _check(3, N, C, C, H, W, G, L, got, route)
