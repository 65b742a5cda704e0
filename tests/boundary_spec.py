"""References and input builders of the fp16-boundary, pooling and gather tests (tests/test_50_fp16_boundary_gpu.py,
tests/test_51_beyond_the_grid_gpu.py, tests/test_boundary_spec_cpu.py).

Every reference here is plain torch / numpy in float64 and knows nothing of the kernels: the 1x1 and 3x3 depth heads of
csrc/a16.hip written out from their definition (`Conv2d(C, 1, 1)(relu(x))`, `Conv2d(C, 1, 3, padding=1)(x)` and their
gradients), the two poolings of csrc/pool.hip, and the loss-scale rules of csrc/a16.hip's header comment
(dvd_gscale_begin, dvd_gscale_end) as small Python models.

Two kinds of inputs:
  * exact-integer inputs (small_ints): every product and every partial sum of the cases below is an integer below 2^24, so
    fp32 (and fp16 where the kernel stores fp16) arithmetic is exact in ANY order and a kernel must equal the float64
    reference bit for bit.  tests/test_boundary_spec_cpu.py checks that claim for every case on the CPU;
  * random fp16-valued / fp32 inputs with rounding-error bounds derived from the operation count (the *_bounds functions).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24          # unit round-off of fp32
U16 = 2.0 ** -11          # unit round-off of fp16
SUB16 = 2.0 ** -25        # half the spacing of fp16 subnormals
EXACT_LIMIT = 2.0 ** 24   # integers below it are exact in fp32
GS_OVERFLOW = np.float32(46340.95)      # 2^15.5 in fp32: an observed max |S g| at or beyond it skips the step (csrc/a16.hip)
F16_MAX = np.float32(65504.0)

# ---- the cases that cross a launch cap (part 1) ------------------------------------------------------------------------
HEAD1X1_SHAPE = (5, 3, 500, 1000)           # N * H * W / 4 = 625 000 items
HEAD3X3_SHAPE = (3, 5, 300, 700)            # 630 000 pixels; C = 5: a partial channel group of the weight gradient
ADD_F16_VEC_N = 2100004                     # 525 001 groups of four
ADD_F16_SCALAR_N = 600001                   # odd: one element per item
TO_HALF_N = (2100004, 2100003)              # the kernel; the ATen fall-back of conv._ToHalf
SUBSAMPLE_SHAPE = (3, 4, 1201, 1403)        # 5.06 M outputs, 10.1 M backward pairs
AVGPOOL_SHAPE = (4, 6, 1201, 1403)          # 10.1 M outputs, 40.4 M inputs
AVGPOOL_CFGS = ((2, 2, 0), (3, 2, 1))       # (kernel, stride, padding): the hourglass's and FCNUnet's
GATHER_B = 5
GATHER_LAUNCH_1 = (((5, 3500000), torch.float32), ((5, 7, 11), torch.float32), ((5, 13), torch.uint8), ((5,), torch.float32))
GATHER_LAUNCH_2 = (((5, 1000001), torch.float32),)
GATHER_TILE_ACCESSES = 1024                 # accesses per tile (csrc/gather.hip kGatherTile)


def small_ints(shape, seed, lo=-2, hi=2, mul=1, plant=None, dtype=torch.float64):
    """CPU tensor (float64 unless told otherwise) of integers mul * {lo..hi}, seeded; plant: that value (times mul) at the
    first and -it at the last position, so the extreme the loss scale is computed from is certainly there."""
    g = torch.Generator().manual_seed(seed)
    t = (torch.randint(lo, hi + 1, tuple(shape), generator=g, dtype=torch.int16) * mul).to(dtype)
    if plant is not None:
        t.view(-1)[0] = plant * mul
        t.view(-1)[-1] = -plant * mul
    return t


def head1x1_exact_inputs():
    """(x, w, b, gy) of the 1x1 head's case: {-2..2} everywhere, a +-2 planted in w and gy (max|gy| * max|w| = 4 -> S = 2)."""
    N, C, H, W = HEAD1X1_SHAPE
    return (small_ints(HEAD1X1_SHAPE, 11), small_ints((C,), 12, plant=2), torch.tensor([2.0], dtype=torch.float64),
            small_ints((N, 1, H, W), 13, plant=2))


def head3x3_exact_inputs():
    N, C, H, W = HEAD3X3_SHAPE
    return (small_ints(HEAD3X3_SHAPE, 21), small_ints((1, C, 3, 3), 22, plant=2), torch.tensor([-2.0], dtype=torch.float64),
            small_ints((N, 1, H, W), 23, plant=2))


def add_f16_exact_inputs(n):
    """Two summands of integers in [-1000, 1000]: they and their sum (at most 2000 < 2048) are exact in fp16."""
    return small_ints((n,), 31, -1000, 1000), small_ints((n,), 32, -1000, 1000)


def pool_exact_inputs(shape, out_shape, mul, hi, seed):
    """(x, gy) as fp32 CPU tensors (exact: integers) for a pooling case; the references cast them to float64 themselves."""
    return (small_ints(shape, seed, -hi, hi, mul, dtype=torch.float32),
            small_ints(out_shape, seed + 1, -hi, hi, mul, dtype=torch.float32))


def survives(t, dtype):
    """Does the float64 tensor t come back unchanged from a round trip through dtype?"""
    return bool(torch.equal(t.to(dtype).double(), t))


# ---- the depth heads ---------------------------------------------------------------------------------------------------
def head1x1_ref(x, w, b, gy, relu_in, S=1.0):
    """Conv2d(C, 1, 1)(relu(x)) and its gradients in float64 from the definition.  x [N,C,H,W], w [C], b scalar tensor or
    None, gy [N,1,H,W].  Returns a dict: y, gx (times the loss scale S), gw, gb (None without a bias), and the sums of
    absolute terms behind every accumulated quantity (y_abs per pixel, gw_abs per channel, gb_abs)."""
    x, w, gy = x.double(), w.double().view(1, -1, 1, 1), gy.double()
    a = x.clamp(min=0) if relu_in else x
    bias = 0.0 if b is None else b.double().view(())
    out = {'y': (w * a).sum(1, keepdim=True) + bias,
           'y_abs': (w.abs() * a.abs()).sum(1, keepdim=True) + abs(bias),
           'gx': S * w * gy * ((x > 0).double() if relu_in else 1.0),
           'gw': (gy * a).sum((0, 2, 3)), 'gw_abs': (gy * a).abs().sum((0, 2, 3)),
           'gb': None if b is None else gy.sum().view(1), 'gb_abs': gy.abs().sum().view(1)}
    return out


def head3x3_ref(x, w, b, gy, S=1.0):
    """Conv2d(C, 1, 3, padding=1)(x) and its gradients: F.conv2d in float64 and its autograd.  w [1,C,3,3].  Same dict as
    head1x1_ref; gx_abs is the sum of the absolute terms of every gx element (its rounding bound needs it)."""
    def run(x, w, b, gy):
        xd = x.double().detach().requires_grad_(True)
        wd = w.double().detach().requires_grad_(True)
        bd = None if b is None else b.double().detach().view(1).requires_grad_(True)
        y = F.conv2d(xd, wd, bd, padding=1)
        y.backward(gy.double())
        return y.detach(), xd.grad, wd.grad, None if bd is None else bd.grad

    y, gx, gw, gb = run(x, w, b, gy)
    # the same convolution of the absolute values: the sums of absolute terms behind y, gx and gw
    y_abs, gx_abs, gw_abs, _ = run(x.abs(), w.abs(), None if b is None else b.abs(), gy.abs())
    return {'y': y, 'y_abs': y_abs, 'gx': S * gx, 'gx_abs': S * gx_abs, 'gw': gw, 'gw_abs': gw_abs, 'gb': gb,
            'gb_abs': gy.double().abs().sum().view(1)}


def head3x3_chunk(total):
    """Pixels per block of the 3x3 head's weight gradient, from the documented rule: ceil(total / 1024) chunks, at most 256."""
    chunks = min(256, max(1, -(-total // 1024)))
    return -(-total // chunks)


def head1x1_bounds(ref, C, f16):
    """|error| bounds of dvd_head1x1_* against head1x1_ref (fp32 FMA chains; fp16: one more rounding at the store).
    y: a chain of C FMAs behind the bias.  gx: one fp32 product (and one rounding to fp16).  gw, gb: the longest path of
    sequential fp32 adds is a 4-term chain, 6 wave steps and 2 adds; the blocks' partials are added in double."""
    v = ref['gx'].abs()
    return {'y': (C + 2) * U32 * ref['y_abs'],
            'gx': (U16 + 2 * U32) * v + SUB16 if f16 else U32 * v,
            'gw': 16 * U32 * ref['gw_abs'], 'gb': 16 * U32 * ref['gb_abs']}


def head3x3_bounds(ref, C, total):
    """|error| bounds of dvd_head3x3_* against head3x3_ref: y is a chain of 9 C FMAs behind the bias; gx a chain of 9 FMAs
    (10 roundings allowed) rounded once more to fp16; gw / gb one FMA per pixel of the thread's share of its chunk, then 6
    wave steps, 2 adds and the conversion of the double sum."""
    steps = -(-head3x3_chunk(total) // 256) + 10
    return {'y': (9 * C + 2) * U32 * ref['y_abs'],
            'gx': U16 * ref['gx'].abs() + 10 * U32 * (1 + U16) * ref['gx_abs'] + SUB16,
            'gw': steps * U32 * ref['gw_abs'], 'gb': steps * U32 * ref['gb_abs']}


# ---- pooling -----------------------------------------------------------------------------------------------------------
def avgpool_ref(x, k, st, pad, gy):
    """F.avg_pool2d (PyTorch's defaults) and its autograd in float64 on x's device -> (y, gx)."""
    xd = x.double().detach().requires_grad_(True)
    y = F.avg_pool2d(xd, k, st, pad)
    y.backward(gy.double())
    return y.detach(), xd.grad


def avgpool_out_shape(shape, k, st, pad):
    N, C, H, W = shape
    return (N, C, (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1)


def subsample_ref(x, gy):
    """x[:, :, ::2, ::2] and its autograd in float64 -> (y, gx)."""
    xd = x.double().detach().requires_grad_(True)
    y = xd[:, :, ::2, ::2].contiguous()
    y.backward(gy.double())
    return y.detach(), xd.grad


def subsample_out_shape(shape):
    N, C, H, W = shape
    return (N, C, (H + 1) // 2, (W + 1) // 2)


# ---- gather ------------------------------------------------------------------------------------------------------------
def gather_tiles(launch, base_alignment=16):
    """(tiles per pair, bytes per access) of every tensor of one dvd_gather_pairs launch, from the rule in csrc/gather.hip's
    header: 16-byte accesses when the bytes per pair (and the base addresses) are multiples of 16, dwords for multiples of 4,
    bytes otherwise; a tile is 1024 accesses of one pair."""
    out = []
    for shape, dtype in launch:
        bpp = int(np.prod(shape[1:], dtype=np.int64)) * torch.empty(0, dtype=dtype).element_size()
        bits = bpp | base_alignment
        vec = 16 if bits % 16 == 0 else (4 if bits % 4 == 0 else 1)
        out.append((-(-bpp // (GATHER_TILE_ACCESSES * vec)), vec))
    return out


def gather_inputs(launch, seed):
    """Seeded CPU tensors of one launch: integer-valued floats (no NaN: torch.equal must be able to confirm a copy)."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 255, shape, generator=g, dtype=torch.uint8) if dtype == torch.uint8 else
            torch.randint(-2 ** 23, 2 ** 23, shape, generator=g, dtype=torch.int32).to(dtype) for shape, dtype in launch]


# ---- the loss-scale rules (csrc/a16.hip, header comment) ---------------------------------------------------------------
def gscale_begin_ref(g_amax, w_amax, target):
    """S of dvd_gscale_begin: the power of two 2^clamp(int(target) - e, -120, 120) with max|g| * max|w| = f * 2^e, f in
    [0.5, 1), the product formed in fp32; 1 when the product is 0, Inf, NaN or >= 3e38."""
    with np.errstate(over='ignore', invalid='ignore'):
        m = np.float32(g_amax) * np.float32(w_amax)
    if not (m > 0 and m < np.float32(3.0e38)):
        return 1.0
    _, e = np.frexp(m)
    return 2.0 ** min(max(int(target) - int(e), -120), 120)


def gscale_end_model(st):
    """dvd_gscale_end on a list of the state's 16 floats -> the state after it.  obs = [3] is the step's max |S g|, fwd = [6]
    the forward monitor.  An activation at or beyond fp16's maximum skips the step for both networks ([4], [8]; counters [5],
    [9], run length [10]) and leaves the target alone; obs >= 2^15.5 skips the depth net's step and backs the target off by
    ceil(log2(obs) - 13) octaves (8 when obs is not finite); else the target moves by rint(13 - log2(obs)) octaves, at most
    4 upwards, and not at all when obs is 0.  The target stays within [-24, 14]; [3] and [6] are cleared."""
    s = [float(v) for v in st]
    obs, fwd, target = np.float32(s[3]), np.float32(s[6]), s[2]
    if not fwd < F16_MAX:
        s[4], s[5], s[8], s[9], s[10] = 1.0, s[5] + 1, 1.0, s[9] + 1, s[10] + 1
    elif not obs < GS_OVERFLOW:
        s[4], s[5], s[8], s[10] = 1.0, s[5] + 1, 0.0, 0.0
        target -= math.ceil(float(np.log2(obs)) - 13.0) if obs < np.float32(3.0e38) else 8.0
    else:
        s[4], s[8], s[10] = 0.0, 0.0, 0.0
        if obs > 0:
            target += min(float(np.rint(np.float32(13.0) - np.log2(obs))), 4.0)
    s[2], s[3], s[6] = min(max(target, -24.0), 14.0), 0.0, 0.0
    return s
