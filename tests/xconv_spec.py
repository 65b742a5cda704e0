"""What dvd_xconv_fwd[_h] computes, in float64 on the CPU, written from include/dvd_hip.h alone -- and the data, the case table
and the class list of tests/test_69_xconv_classes_gpu.py.

    y = act_out( BN( conv(act_in(x)) + bias ) + res' ) * [mask_src > 0]

  flags bit 0: act_in = ReLU, bit 1: act_out = ReLU, bit 2: res' = relu(residual),
        bit 3: the convolution is F.conv2d(stride=2, padding=1),
        bit 4: the convolution is the gradient of that one with respect to its input (x is the gradient of the strided output);
  BN(z) = (z - mean) / sqrt(var + eps) * gamma + beta   (gamma / beta None = 1 / 0), bn None = identity;
  transposed: the backward-data operator of the stride-1 convolution with weight w (dvd_xconv_pack(.., transposed = 1));
  scaled = (gamma | None, var, eps): every weight of w's output channel co times gamma[co] / sqrt(var[co] + eps)
  (dvd_xconv_pack_scaled).  w is always the weight of the FORWARD convolution, [Cout][Cin / groups][k][k].

The backward operators come from float64 autograd of F.conv2d, not from a hand-written transposed convolution.

Exact data (exact_data): small integers and power-of-two BatchNorm pairs, for which every product, every partial sum in any
order, the unscale, the epilogue and the fused multiply-add are exact in the kernel's fp32 arithmetic, so the kernel must
reproduce spec()'s y bit for bit.  tests/test_xconv_spec_cpu.py proves those premises for every case of the table below, and
proves with dvd_xconv_describe that the table reaches every class of REQUIRED.  A new instantiation of xconv_kernel comes with
a row in CASES and an entry in REQUIRED."""
import zlib

import torch
import torch.nn.functional as F

F32, H16, H32 = 'f32', 'h16', 'h32'          # storage: fp32 -> fp32, fp16 -> fp16, fp16 -> fp32 (dvd_xconv_fwd_h, out_f16 = 0)
STORAGES = (F32, H16, H32)
IN_DTYPE = {F32: torch.float32, H16: torch.float16, H32: torch.float16}
OUT_DTYPE = {F32: torch.float32, H16: torch.float16, H32: torch.float32}

RELU_IN, RELU_OUT, RES_RELU, S2, ZI = 1, 2, 4, 8, 16


def bn_pair(bn, C):
    """-> (scale, shift) of the header's formula as float64 vectors; (1, 0) without BatchNorm."""
    if bn is None:
        return torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    gamma, beta, mean, var, eps = bn
    s = 1.0 / torch.sqrt(var.double() + float(eps))
    if gamma is not None:
        s = s * gamma.double()
    return s, (beta.double() if beta is not None else 0.0) - mean.double() * s


def parts(x, w, groups=1, flags=0, bias=None, residual=None, mask_src=None, bn=None, transposed=False, scaled=None, out_hw=None):
    """The terms of the formula in float64: z = conv + bias, (s, shift) the BatchNorm pair, res the residual term as added,
    v the result before the cast.  out_hw: the full-resolution (H, W) of flags bit 4 (the gradient's shape leaves it open)."""
    x = x.double()
    w = w.double()
    k = w.shape[-1]
    if scaled is not None:
        g, var, eps = scaled
        sc = 1.0 / torch.sqrt(var.double() + float(eps))
        if g is not None:
            sc = sc * g.double()
        w = w * sc[:, None, None, None]
    if flags & RELU_IN:
        x = x.clamp_min(0.0)
    stride = 2 if flags & (S2 | ZI) else 1
    if transposed or (flags & ZI):
        # the input gradient of u -> F.conv2d(u, w) at the output gradient x (linear in u: any u serves)
        N = x.shape[0]
        H, W = out_hw if flags & ZI else x.shape[2:]
        u = torch.zeros(N, w.shape[1] * groups, H, W, dtype=torch.float64, requires_grad=True)
        out = F.conv2d(u, w, None, stride=stride, padding=k // 2, groups=groups)
        assert out.shape == x.shape, 'gradient %s of an output %s' % (tuple(x.shape), tuple(out.shape))
        conv, = torch.autograd.grad(out, u, x)
    else:
        conv = F.conv2d(x, w, None, stride=stride, padding=k // 2, groups=groups)
    C = conv.shape[1]
    z = conv + (bias.double()[None, :, None, None] if bias is not None else 0.0)
    s, shift = bn_pair(bn, C)
    if bn is not None:
        gamma, beta, mean, var, eps = bn
        v = (z - mean.double()[None, :, None, None]) / torch.sqrt(var.double() + float(eps))[None, :, None, None]
        if gamma is not None:
            v = v * gamma.double()[None, :, None, None]
        if beta is not None:
            v = v + beta.double()[None, :, None, None]
    else:
        v = z.clone()
    res = torch.zeros_like(v)
    if residual is not None:
        res = residual.double()
        if flags & RES_RELU:
            res = res.clamp_min(0.0)
        v = v + res
    if mask_src is not None:
        v = v * (mask_src.double() > 0).double()
    if flags & RELU_OUT:
        v = v.clamp_min(0.0)
    return {'z': z, 's': s, 'shift': shift, 'res': res, 'v': v}


def spec(x, w, groups=1, flags=0, bias=None, residual=None, mask_src=None, bn=None, transposed=False, scaled=None,
         out_dtype=torch.float32, out_hw=None):
    """-> (v, y, amax): the value before the cast to the output storage, v cast once, and max|v| (the kernel folds its
    max|y| scalar from the fp32 value before the cast)."""
    v = parts(x, w, groups, flags, bias, residual, mask_src, bn, transposed, scaled, out_hw)['v']
    return v, v.to(out_dtype), float(v.abs().max())


# ---- the case table -----------------------------------------------------------------------------------------------------
# (name, Cin, Cout, H, W, k, groups, mode, N).  Cin -> Cout are the LAUNCH's channel totals, H x W the full-resolution side.
# mode 'fwd': stride 1; 's2': flags bit 3 (x is H x W, y (H+1)/2 x (W+1)/2); 'zi': flags bit 4 (x is (H+1)/2 x (W+1)/2, y H x W).
# The first 28 rows are the smallest shapes per class (one or two blocks each, ragged channel blocks at 24, 40, 72 and 288);
# tests/test_xconv_spec_cpu.py pins what dvd_xconv_describe answers for them (PINNED).
CASES = [
    ('k1 16-24 5x7', 16, 24, 5, 7, 1, 1, 'fwd', 3),
    ('k1 32-40 6x12', 32, 40, 6, 12, 1, 1, 'fwd', 2),
    ('k1 32-72 8x18', 32, 72, 8, 18, 1, 1, 'fwd', 2),
    ('k1 32-288 8x18', 32, 288, 8, 18, 1, 1, 'fwd', 2),              # one-loop, wide epilogue, ragged channel block and pixel tile
    ('k1 32-288 7x19', 32, 288, 7, 19, 1, 1, 'fwd', 2),              # the same kernel, narrow epilogue (133 pixels)
    ('k1 32-256 12x20', 32, 256, 12, 20, 1, 1, 'fwd', 2),            # wide, full channel blocks
    ('k3 16-24 5x7', 16, 24, 5, 7, 3, 1, 'fwd', 3),
    ('k3 32-40 9x13', 32, 40, 9, 13, 3, 1, 'fwd', 2),
    ('k3 32-72 9x13', 32, 72, 9, 13, 3, 1, 'fwd', 2),
    ('k3 32-288 9x14', 32, 288, 9, 14, 3, 1, 'fwd', 2),              # 512 threads
    ('k3 16-256 13x23', 16, 256, 13, 23, 3, 1, 'fwd', 2),            # ... ragged last tile column
    ('k5 16-24 9x12', 16, 24, 9, 12, 5, 1, 'fwd', 2),
    ('k5 16-64 12x20', 16, 64, 12, 20, 5, 1, 'fwd', 2),
    ('k7 16-32 9x12', 16, 32, 9, 12, 7, 1, 'fwd', 2),
    ('k7 16-72 10x13', 16, 72, 10, 13, 7, 1, 'fwd', 2),
    ('k11 16-32 9x12', 16, 32, 9, 12, 11, 1, 'fwd', 2),              # direct staging
    ('k11 16-256 9x12', 16, 256, 9, 12, 11, 1, 'fwd', 2),
    ('s2 16-32 10x14', 16, 32, 10, 14, 3, 1, 's2', 2),
    ('s2 32-64 11x15', 32, 64, 11, 15, 3, 1, 's2', 2),
    ('s2 32-128 11x15', 32, 128, 11, 15, 3, 1, 's2', 2),
    ('s2 16-256 9x13', 16, 256, 9, 13, 3, 1, 's2', 2),
    ('s2 32-64 41x59', 32, 64, 41, 59, 3, 1, 's2', 2),               # direct staging, three tiles
    ('k3 3-24 7x9', 3, 24, 7, 9, 3, 1, 'fwd', 3),                    # generic loop
    ('k3 20-40 11x19', 20, 40, 11, 19, 3, 1, 'fwd', 2),
    ('k3 12-72 9x13', 12, 72, 9, 13, 3, 1, 'fwd', 2),
    ('k3 20-288 9x13', 20, 288, 9, 13, 3, 1, 'fwd', 2),
    ('k1 5-1 17x29', 5, 1, 17, 29, 1, 1, 'fwd', 2),
    ('k7 3-64 16x24', 3, 64, 16, 24, 7, 1, 'fwd', 2),
    # ---- beyond the seed rows
    ('k1 32-256 8x8', 32, 256, 8, 8, 1, 1, 'fwd', 2),                # wide, full channel blocks, ONE pixel tile
    ('k1 32-288 8x16', 32, 288, 8, 16, 1, 1, 'fwd', 2),              # wide, ragged channel block, one full pixel tile
    ('k1 32-288 8x17', 32, 288, 8, 17, 1, 1, 'fwd', 2),              # wide, 136 pixels in tiles of 72: a ragged last pixel tile
    ('k1 32-256 8x17', 32, 256, 8, 17, 1, 1, 'fwd', 2),              # ... with full channel blocks
    ('k3 16-256 7x37', 16, 256, 7, 37, 3, 1, 'fwd', 2),              # 512 threads: ragged last tile row (4 + 3 rows)
    ('k7 16-256 4x46', 16, 256, 4, 46, 7, 1, 'fwd', 2),              # 512 threads, FI 3
    ('k11 16-256 4x45', 16, 256, 4, 45, 11, 1, 'fwd', 2),            # 512 threads, direct staging
    ('k1 32-72 12x20', 32, 72, 12, 20, 1, 1, 'fwd', 2),              # 1x1, FI 1, two pixel tiles of 128 positions
    ('k3 32-320 13x23', 32, 320, 13, 23, 3, 1, 'fwd', 2),            # 512 threads: ragged tile column AND ragged channel block
    ('k3 32-72 17x19', 32, 72, 17, 19, 3, 1, 'fwd', 2),              # 256 threads: ragged last tile row
    ('k3 32-136 9x25', 32, 136, 9, 25, 3, 1, 'fwd', 2),              # (2,2,2,2): two channel blocks, the last ragged; ragged column
    ('k3 32-72 23x29', 32, 72, 23, 29, 3, 1, 'fwd', 2),              # FI 3 on 256 threads
    ('k5 32-256 12x20', 32, 256, 12, 20, 5, 1, 'fwd', 2),            # 512 threads, wider halo
    ('k3 g2 64-64 9x23', 64, 64, 9, 23, 3, 2, 'fwd', 2),             # grouped, 32 per group
    ('k3 g2 128-128 7x10', 128, 128, 7, 10, 3, 2, 'fwd', 2),         # grouped, 64 per group
    ('k1 g2 64-576 8x18', 64, 576, 8, 18, 1, 2, 'fwd', 2),           # grouped wide epilogue: per-channel operands at grp * Cout + co
    ('k3 g3 72-120 9x13', 72, 120, 9, 13, 3, 3, 'fwd', 2),           # 24 -> 40 per group: generic loop, ragged block in every group
    ('s2 g2 64-64 10x14', 64, 64, 10, 14, 3, 2, 's2', 2),
    ('s2 16-32 1x40', 16, 32, 1, 40, 3, 1, 's2', 2),                 # one-row image
    ('s2 16-32 40x1', 16, 32, 40, 1, 3, 1, 's2', 2),                 # one-column image
    ('s2 32-160 11x15', 32, 160, 11, 15, 3, 1, 's2', 2),             # two channel blocks of 128, the last ragged
    ('zi 16-32 10x14', 16, 32, 10, 14, 3, 1, 'zi', 2),
    ('zi 32-64 11x15', 32, 64, 11, 15, 3, 1, 'zi', 2),
    ('zi 32-72 11x15', 32, 72, 11, 15, 3, 1, 'zi', 2),
    ('zi 32-288 9x13', 32, 288, 9, 13, 3, 1, 'zi', 2),
    ('zi g2 64-64 11x14', 64, 64, 11, 14, 3, 2, 'zi', 2),
    ('zi 16-32 1x40', 16, 32, 1, 40, 3, 1, 'zi', 2),
    ('zi 16-32 40x1', 16, 32, 40, 1, 3, 1, 'zi', 2),
    ('zi 16-32 1x127', 16, 32, 1, 127, 3, 1, 'zi', 2),               # 3 x 129 haloed cells on 256 threads: direct staging
    ('zi 32-64 41x59', 32, 64, 41, 59, 3, 1, 'zi', 2),               # several tiles, ragged
]
CASE = {c[0]: c for c in CASES}
WIDE_MISALIGNED = ('k1 32-288 8x18', 'k1 32-256 12x20')               # the cases that also run with operands off 16 bytes


def mode_flags(mode):
    return {'fwd': 0, 's2': S2, 'zi': ZI}[mode]


def storages_of(case):
    """fp16 activations exist where the input channels per group are whole 16-channel chunks."""
    _, Cin, _, _, _, _, G, _, _ = case
    return STORAGES if (Cin // G) % 16 == 0 else (F32,)


def shapes_of(case):
    """-> (x shape, y shape) of the launch."""
    _, Cin, Cout, H, W, _, _, mode, N = case
    q = ((H + 1) // 2, (W + 1) // 2)
    return (N, Cin) + (q if mode == 'zi' else (H, W)), (N, Cout) + (q if mode == 's2' else (H, W))


# Epilogues: (name, flags, operands, packing).  Packing 'f': forward, 't': transposed (the backward-data operator, flipped taps),
# 'ts' / 'fs': the same through dvd_xconv_pack_scaled.  The strided forms keep the packing their operator needs: the stride-2
# forward runs every epilogue on the forward order ('t' -> 'f', 'ts' -> 'fs'), its backward-data on the transposed order.
EPILOGUES = [
    ('none', 0, (), 'f'),
    ('bias', 0, ('bias',), 'f'),
    ('bias+residual', 0, ('bias', 'residual'), 'f'),
    ('relu_in+bias+relu(residual)', RELU_IN | RES_RELU, ('bias', 'residual'), 'f'),
    ('relu_out', RELU_OUT, (), 'f'),
    ('bn affine+relu_out', RELU_OUT, ('bn',), 'f'),
    ('bn plain+bias', 0, ('bn_plain', 'bias'), 'f'),
    ('bn affine+bias+residual+relu_out', RELU_OUT, ('bn', 'bias', 'residual'), 'f'),
    ('mask', 0, ('mask',), 't'),
    ('mask+residual', 0, ('mask', 'residual'), 't'),
    ('mask on the scaled packing', 0, ('mask',), 'ts'),
]


def packing_of(mode, pk):
    if mode == 's2':
        return {'f': 'f', 't': 'f', 'ts': 'fs'}[pk]
    if mode == 'zi':
        return {'f': 't', 't': 't', 'ts': 'ts'}[pk]
    return pk


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _pick(g, n, values):
    return torch.tensor(values)[torch.randint(0, len(values), (n,), generator=g)].float()


def exact_data(case):
    """Everything a case's launches read, as fp32 CPU tensors (every value is exact in fp16 too):
    x, residual, mask in [-4, 4]; wf / wt the forward convolution's weight for the forward / transposed packings, in [-2, 2];
    bias in [-8, 8]; bn (eps = 0, var in {1/4, 1, 4, 16}, gamma in {+-1/2, +-1, +-2}, integer mean and beta); the pair (gamma,
    var) of the scaled packing, indexed by the weight's output channel."""
    name, Cin, Cout, H, W, k, G, mode, N = case
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    xs, ys = shapes_of(case)
    d = {'x': _ints(g, xs, -4, 4), 'residual': _ints(g, ys, -4, 4), 'mask': _ints(g, ys, -4, 4),
         'wf': _ints(g, (Cout, Cin // G, k, k), -2, 2), 'wt': _ints(g, (Cin, Cout // G, k, k), -2, 2),
         'bias': _ints(g, (Cout,), -8, 8)}
    d['x'].view(-1)[0] = 4.0                       # the true maximum is 4
    gam = [-2.0, -1.0, -0.5, 0.5, 1.0, 2.0]
    var = [0.25, 1.0, 4.0, 16.0]
    d['bn'] = (_pick(g, Cout, gam), _ints(g, (Cout,), -4, 4), _ints(g, (Cout,), -4, 4), _pick(g, Cout, var), 0.0)
    d['bn_plain'] = (None, None, d['bn'][2], d['bn'][3], 0.0)
    d['scale_f'] = (_pick(g, Cout, gam), _pick(g, Cout, var), 0.0)       # forward order: w's output channels are the launch's
    d['scale_t'] = (_pick(g, Cin, gam), _pick(g, Cin, var), 0.0)         # transposed: they are the launch's INPUT channels
    return d


def real_data(case):
    """The same operands from randn; BatchNorm with eps = 1e-5, var in [0.3, 2]."""
    name, Cin, Cout, H, W, k, G, mode, N = case
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) ^ 0x5eed)
    xs, ys = shapes_of(case)
    r = lambda *s: torch.randn(*s, generator=g)
    d = {'x': r(*xs), 'residual': r(*ys), 'mask': r(*ys), 'wf': r(Cout, Cin // G, k, k) * 0.1, 'wt': r(Cin, Cout // G, k, k) * 0.1,
         'bias': r(Cout)}
    var = lambda n: 0.3 + 1.7 * torch.rand(n, generator=g)
    d['bn'] = (r(Cout), r(Cout), r(Cout), var(Cout), 1e-5)
    d['bn_plain'] = (None, None, d['bn'][2], d['bn'][3], 1e-5)
    d['scale_f'] = (r(Cout), var(Cout), 1e-5)
    d['scale_t'] = (r(Cin), var(Cin), 1e-5)
    return d


def spec_args(case, data, epi):
    """-> the keyword arguments of spec() / parts() for one epilogue of a case (out_dtype excepted)."""
    _, _, _, H, W, _, G, mode, _ = case
    _, flags, ops, pk = epi
    pk = packing_of(mode, pk)
    tr = pk[0] == 't'
    kw = dict(x=data['x'], w=data['wt'] if tr else data['wf'], groups=G, flags=flags | mode_flags(mode),
              transposed=tr and mode != 'zi', out_hw=(H, W))
    if len(pk) > 1:
        kw['scaled'] = data['scale_t'] if tr else data['scale_f']
    for o in ops:
        if o in ('bn', 'bn_plain'):
            kw['bn'] = data[o]
        elif o == 'mask':
            kw['mask_src'] = data['mask']
        else:
            kw[o] = data[o]
    return kw


# ---- dvd_xconv_describe ---------------------------------------------------------------------------------------------------
DESC_FIELDS = ('TM', 'TN', 'WM', 'WN', 'b1', 'fast', 'fit', 'in16', 'out16', 'wide', 's2', 'zi', 'TR', 'TC', 'P', 'PQ', 'ntr',
               'ntc', 'mblocks', 'lds', 'threads', 'items')       # include/dvd_hip.h: DVD_XDESC_*
FIT_DIRECT, FIT_ONE = 0, 11                                     # DVD_XFIT_*


def describe(lib, case, storage, aligned=True):
    """-> (status, dict of DESC_FIELDS plus what the shape adds: ragged last tile row / column / channel block)."""
    import ctypes
    _, Cin, Cout, H, W, k, G, mode, _ = case
    out = (ctypes.c_int * 24)()
    st = lib.dvd_xconv_describe(Cin, Cout, H, W, k, G, mode_flags(mode), int(storage != F32), int(storage == H16), int(aligned),
                                ctypes.cast(out, ctypes.c_void_p))
    d = dict(zip(DESC_FIELDS, list(out)))
    if st == 0:
        Ho, Wo = (1, H * W) if k == 1 else (((H + 1) // 2, (W + 1) // 2) if mode == 's2' else (H, W))
        d['cfg'] = (d['TM'], d['TN'], d['WM'], d['WN'])
        d['ragged_row'] = int(Ho % d['TR'] != 0 and d['ntr'] > 1)
        d['ragged_col'] = int(Wo % d['TC'] != 0 and d['ntc'] > 1)
        d['one_tile'] = int(d['ntr'] * d['ntc'] == 1)
        d['ragged_block'] = int((Cout // G) % (32 * d['TM'] * d['WM']) != 0)
        d['many_blocks'] = int(d['mblocks'] > 1)
        d['odd'] = (H % 2, W % 2)
        d['one_row'], d['one_col'] = int(H == 1), int(W == 1)
        d['storage'] = storage
        d['kge3'] = int(k >= 3)
    return st, d


def key_of(d):
    return 'cfg %s%s %s fit %d %s%s%s tile %dx%d/%d/%d blocks %dx%d' % (
        d['cfg'], ' b1' if d['b1'] else '', 'fast' if d['fast'] else 'generic', d['fit'], d['storage'], ' wide' if d['wide'] else '',
        ' s2' if d['s2'] else (' zi' if d['zi'] else ''), d['TR'], d['TC'], d['P'], d['PQ'], d['ntr'] * d['ntc'], d['mblocks'])


def _req():
    """The classes the table must reach under dvd_xconv_select(0): (name, fields a description must match)."""
    R = []
    shapes = [(1, 2, 1, 4), (2, 2, 1, 4), (2, 2, 2, 2), (4, 2, 2, 2), (4, 2, 2, 4)]
    for st in STORAGES:
        for cfg in shapes:
            R.append(('%s on the fast loop, %s' % (cfg, st), dict(cfg=cfg, fast=1, storage=st)))
        for fit in (FIT_ONE, 1, 2, 3, FIT_DIRECT):
            R.append(('fit %d, 256 threads, %s' % (fit, st), dict(fit=fit, threads=256, storage=st, s2=0)))
        # 512 threads is the (4,2,2,4) shape, which pick_cfg hands out for k >= 3 only: never the one-loop
        for fit in (1, 2, 3, FIT_DIRECT):
            R.append(('fit %d, 512 threads, %s' % (fit, st), dict(fit=fit, threads=512, storage=st)))
        for cfg in shapes[:3]:
            R.append(('s2 %s, %s' % (cfg, st), dict(s2=1, cfg=cfg, storage=st, b1=int(st == F32))))
            R.append(('zi %s, %s' % (cfg, st), dict(zi=1, cfg=cfg, storage=st)))
        R.append(('s2 register-prefetched, %s' % st, dict(s2=1, storage=st, fit=2)))
        R.append(('s2 direct, %s' % st, dict(s2=1, storage=st, fit=FIT_DIRECT)))
        R.append(('zi register-prefetched, %s' % st, dict(zi=1, storage=st, fit=2)))
        R.append(('zi direct, %s' % st, dict(zi=1, storage=st, fit=FIT_DIRECT)))
        for form in ('s2', 'zi'):
            R.append(('%s even H and W, %s' % (form, st), {form: 1, 'odd': (0, 0), 'storage': st}))
            R.append(('%s odd H and W, %s' % (form, st), {form: 1, 'odd': (1, 1), 'storage': st}))
            R.append(('%s one-row image, %s' % (form, st), {form: 1, 'one_row': 1, 'storage': st}))
            R.append(('%s one-column image, %s' % (form, st), {form: 1, 'one_col': 1, 'storage': st}))
        for rb in (0, 1):
            R.append(('wide epilogue, one pixel tile, ragged block %d, %s' % (rb, st), dict(wide=1, one_tile=1, ragged_block=rb, storage=st)))
            R.append(('wide epilogue, ragged last pixel tile, ragged block %d, %s' % (rb, st),
                      dict(wide=1, ragged_col=1, ragged_block=rb, storage=st)))
        R.append(('narrow epilogue on a one-loop kernel, %s' % st, dict(fit=FIT_ONE, wide=0, storage=st)))
    for cfg in shapes[:3]:
        R.append(('%s on the generic loop' % (cfg,), dict(cfg=cfg, fast=0, storage=F32)))
    for th in (256, 512):
        R.append(('ragged last tile row, k >= 3, %d threads' % th, dict(ragged_row=1, threads=th, kge3=1)))
        R.append(('ragged last tile column, k >= 3, %d threads' % th, dict(ragged_col=1, threads=th, kge3=1)))
    # (pick_cfg hands out (1,2,1,4) for at most 32 and (2,2,1,4) for at most 64 channels per group, their blockM(): those two
    #  shapes never have a second channel block, at stride 2 neither, where the channel count is capped at 128 first)
    for cfg in shapes[2:]:
        R.append(('several channel blocks, the last ragged, %s' % (cfg,), dict(cfg=cfg, many_blocks=1, ragged_block=1)))
    return R


REQUIRED = _req()


def matches(d, want):
    return all(d.get(k) == v for k, v in want.items())
