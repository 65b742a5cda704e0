"""What the weight-gradient entry points of csrc/xwgrad3.hip compute, in float64 on the CPU, written from include/dvd_hip.h alone
-- and the data, the case table and the list of kernel instantiations of tests/test_70_wgrad_classes_gpu.py.

    dW[co][ci][ky][kx] = out_scale * sum_{n, r, c} gy[n][co][r][c] * act(x)[n][ci][r + ky - KS/2][c + kx - KS/2]

act = ReLU if relu_in, x zero outside the image, groups as in F.conv2d; out_scale exists for the fp16 entry points (the inverse
loss scale) and is 1 elsewhere.  The row sums of dvd_xwgrad1s_rowsum / dvd_xwgrad3_rowsum are gy.sum((0, 2, 3)).  dW comes from
float64 autograd of F.conv2d(padding = KS // 2, groups), not from a hand-written correlation.

Two data sets make the kernels' fp32 arithmetic exact, so that a kernel must reproduce the specification bit for bit whatever
lane, slice or launch computed an element and in whatever order:

  exact_data   integers in [-3, 3].  The two-term fp16 split (csrc/dvd_split.h) of an integer times a power of two has l = 0, every
               product and every partial sum is an integer multiple of one power of two well inside 24 bits, the unscale is a
               power of two, xwgrad3_reduce_kernel adds exact values: the result depends neither on the slice count nor on the hook.
  split_data   x = a + b 2^-12 with |a| in 4 .. 7 and integer |b| <= 7 (so h = a 2^11, l = b / 2 under the kernel's scale: the low
               terms are live), gy the same on so few pixels per plane that sum |h h'| + |h l'| + |l h'| stays below 2^24 units of
               the accumulator's granularity 2^10.  The kernel then computes sum (h h' + h l' + l h') exactly; the l l' term it
               drops by design is what separates that from the float64 truth.  split_expected returns both.  (fp32 entry points:
               an fp16 operand has no low term.)

tests/test_wgrad_spec_cpu.py proves those premises for every row of CASES by emulating the kernel arithmetic in numpy, and proves
with dvd_xwgrad_describe (pure host code) that the table reaches every instantiation of REQUIRED.  A new instantiation in
wg_kernels() comes with a row in CASES and an entry in REQUIRED."""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

F32, H16 = 'f32', 'h16'
BOTH = (F32, H16)
DTYPE = {F32: torch.float32, H16: torch.float16}
H16_OUT_SCALE = 2.0 ** -3

FAMILIES = ('xwgrad3', 'xwgrad3g', 'xwgradk', 'xwgrad1s', 'xwgrad1b')      # DVD_WFAM_*
BLOCK = {'xwgrad3': 64, 'xwgrad3g': 32, 'xwgradk': 32, 'xwgrad1s': 128, 'xwgrad1b': 256}      # channels per block, both sides


def wgrad(x, gy, KS, G=1):
    """float64 autograd weight gradient of F.conv2d(x, w, padding=KS // 2, groups=G) at the output gradient gy."""
    x, gy = x.double(), gy.double()
    w = torch.zeros(gy.shape[1], x.shape[1] // G, KS, KS, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, None, padding=KS // 2, groups=G)
    gw, = torch.autograd.grad(y, w, gy)
    return gw


def spec(x, gy, KS, G=1, relu_in=0, out_scale=1.0):
    """-> (dW, row sums), float64."""
    xd = x.double().clamp_min(0.0) if relu_in else x.double()
    return wgrad(xd, gy, KS, G) * float(out_scale), gy.double().sum((0, 2, 3))


# ---- the case table -----------------------------------------------------------------------------------------------------
# (name, KS, N, Cin, Cout, H, W, G, storage, relu_in, rowsum, hooks).  Channel counts are totals over the G groups.  rowsum: the
# case also runs the _rowsum entry point (fp32).  hooks: the dvd_xwgrad_select values the case runs under (0 = automatic;
# 1: 1x1 on the 128 x 128 blocks; 2: no FW form, no 32 x 32 blocks; 3: the round-robin deal, four K steps everywhere).
# Shapes are the smallest that reach a key: one or two channel blocks, a few rows of at most three strips.  Per walking family
# (xwgrad3, xwgrad3g, xwgradk 5 / 7 / 11): H = 1, H = 2, W = 1 and 3 (narrower than an 8-pixel cell), W = 64 / 65 / 128 + 16
# (strip boundaries; 65 and 144 launch a full-strip class and an NK 1 tail), W = 22 / 42 (NK 2 / 3), N = 3 with one or two
# slices per class that cross images (W = 65), odd W under fp16 (the guarded row step; xwgrad3g hands those to xwgrad3_kernel),
# one case ragged on both sides of the block and one with two blocks on each side (xwgrad3g: at most 32 channels per group is what
# routes to it, so its second block is the second group).  1x1: H * W in {4, 12, 16, 252}, odd H * W, and N * chunks odd and
# above the slice count (29 x 43 on 3 x 3 blocks of 128: 117 chunks over 114 slices; 16 x 23 and 14 x 26 on 2 x 2 blocks of
# 256: 69 over 64).
ALL = (0, 1, 2, 3)
CASES = [
    # xwgrad3_kernel: 64 x 64 channel blocks
    ('w3 3x1', 3, 2, 8, 8, 3, 1, 1, BOTH, 1, False, (0, 2, 3)),
    ('w3 4x3', 3, 2, 8, 8, 4, 3, 1, BOTH, 0, True, (0, 1)),                  # fp16: odd W, the guarded row step
    ('w3 2x6', 3, 1, 8, 8, 2, 6, 1, BOTH, 0, False, (0,)),                  # H = 2; fp16 FW NK 1
    ('w3 3x22', 3, 1, 8, 8, 3, 22, 1, BOTH, 1, False, (0, 3)),              # NK 2
    ('w3 1x42', 3, 2, 8, 8, 1, 42, 1, BOTH, 0, False, (0, 2)),              # H = 1; NK 3
    ('w3 5x64', 3, 3, 80, 72, 5, 64, 1, BOTH, 1, True, ALL),                # two ragged blocks on each side; NK 4
    ('w3 6x65', 3, 3, 8, 8, 6, 65, 1, BOTH, 0, False, (0, 2, 3)),           # NK 4 + NK 1 launches, two slices each across three images
    ('w3 3x144', 3, 2, 8, 8, 3, 144, 1, BOTH, 1, False, (0, 3)),            # two full strips and a 16-pixel tail
    ('w3 17x21', 3, 3, 8, 8, 17, 21, 1, BOTH, 0, False, (0, 3)),            # six slices of 9 / 8 rows over three images of 17
    ('w3 g2 4x21', 3, 2, 128, 128, 4, 21, 2, BOTH, 0, True, (0, 3)),        # grouped, 64 -> 64 per group: stays on the 64 x 64 blocks
    # xwgrad3g_kernel: 32 x 32, grouped layers with at most 32 channels per group
    ('g3 3x1', 3, 2, 16, 16, 3, 1, 2, BOTH, 1, True, (0, 2, 3)),
    ('g3 4x3', 3, 2, 16, 16, 4, 3, 2, BOTH, 0, True, (0,)),
    ('g3 2x6', 3, 1, 24, 40, 2, 6, 2, BOTH, 1, True, ALL),                  # 12 -> 20 per group: ragged; H = 2; NK 1
    ('g3 1x22', 3, 2, 16, 16, 1, 22, 2, BOTH, 0, True, (0, 3)),             # H = 1; NK 2
    ('g3 3x42', 3, 1, 16, 16, 3, 42, 2, BOTH, 1, True, (0,)),               # NK 3
    ('g3 5x64', 3, 3, 96, 96, 5, 64, 3, BOTH, 0, True, ALL),                # full 32 x 32 blocks, three groups; NK 4 (fp16: the width test_46 left out)
    ('g3 6x65', 3, 3, 16, 16, 6, 65, 2, BOTH, 1, True, (0, 2, 3)),          # NK 4 + NK 1; fp16 (odd W) runs on xwgrad3_kernel's guarded step
    ('g3 3x144', 3, 2, 24, 40, 3, 144, 2, BOTH, 0, True, (0, 3)),
    ('g3 17x22', 3, 3, 16, 16, 17, 22, 2, BOTH, 0, True, (0, 3)),
]
for _k in (5, 7, 11):
    CASES += [
        ('k%d 1x3' % _k, _k, 2, 8, 8, 1, 3, 1, BOTH, 1, False, (0, 3)),                 # H = 1: fewer rows than the walk's warm-up
        ('k%d 2x1' % _k, _k, 2, 8, 8, 2, 1, 1, BOTH, 0, False, (0,)),
        ('k%d 3x22' % _k, _k, 1, 8, 8, 3, 22, 1, BOTH, 0, False, (0, 3)),               # NK 2
        ('k%d 2x42' % _k, _k, 2, 8, 8, 2, 42, 1, BOTH, 1, False, (0,)),                 # NK 3
        ('k%d 5x64' % _k, _k, 3, 40, 36, 5, 64, 1, BOTH, 0, False, ALL),                # two ragged blocks on each side; NK 4
        # NK 4 + NK 1, one slice each across three images; 5x5: two slices of 21 rows per class over images of 14
        ('k%d %dx65' % (_k, 14 if _k == 5 else 5), _k, 3, 8, 8, 14 if _k == 5 else 5, 65, 1, BOTH, 1, False, (0, 3)),
        ('k%d 3x144' % _k, _k, 2, 12, 20, 3, 144, 1, BOTH, 0, False, (0, 3)),           # ragged single block
    ]
CASES += [
    # xwgrad1s_kernel: 128 x 128, chunks of 32 pixels
    ('s1 2x2', 1, 3, 40, 24, 2, 2, 1, BOTH, 1, True, ALL),                              # ragged single block
    ('s1 3x4', 1, 2, 8, 8, 3, 4, 1, BOTH, 0, True, (0,)),
    ('s1 4x4', 1, 2, 8, 8, 4, 4, 1, BOTH, 0, True, (0,)),
    ('s1 12x21', 1, 2, 136, 130, 12, 21, 1, BOTH, 1, True, (0, 3)),                     # two blocks on each side; H * W = 252
    ('s1 29x43', 1, 3, 264, 264, 29, 43, 1, BOTH, 0, True, (0,)),                       # 117 chunks over 114 slices; odd H * W: element loads
    # xwgrad1b_kernel: 256 x 256, chunks of 16 pixels, both channel counts >= 192 and H * W % 4 == 0
    ('b1 2x2', 1, 3, 200, 196, 2, 2, 1, BOTH, 1, True, ALL),                            # ragged single block; not FW (H * W % 16)
    ('b1 3x4', 1, 2, 200, 196, 3, 4, 1, BOTH, 0, True, (0,)),
    ('b1 4x4', 1, 3, 200, 196, 4, 4, 1, BOTH, 1, True, ALL),                            # FW; fp32 with row sums: RSUM
    ('b1 12x21', 1, 2, 200, 196, 12, 21, 1, BOTH, 0, True, (0,)),                       # 252 pixels: 15 chunks and 12 pixels
    ('b1 16x23', 1, 3, 264, 260, 16, 23, 1, BOTH, 1, True, ALL),                        # two ragged blocks on each side; FW; 69 chunks, 64 slices
    ('b1 14x26', 1, 3, 264, 260, 14, 26, 1, BOTH, 0, True, (0,)),                       # ... not FW
]
CASE = {c[0]: c for c in CASES}
assert len(CASE) == len(CASES)

# the exact-fp32 kernel of csrc/xwgrad.hip (dvd_xwgrad, what DVD_AB=no_xwgrad3 runs): (name, KS, N, Cin, Cout, H, W)
OLD_CASES = [('old k1', 1, 2, 12, 20, 3, 5), ('old k3', 3, 2, 12, 20, 3, 5), ('old k5', 5, 2, 12, 20, 3, 5),
             ('old k7', 7, 2, 12, 20, 3, 5), ('old k11', 11, 2, 12, 20, 3, 5)]

# ---- every instantiation key, written out from the template arguments in wg_kernels() (csrc/xwgrad3.hip) ------------------
REQUIRED = (
    ['xwgrad3 %s %s' % (st, f) for st in BOTH for f in ('FW NK1', 'FW NK2', 'FW NK3', 'FW NK4', 'nonFW')] +
    ['xwgrad3g %s NK%d' % (st, nk) for st in ('f32', 'f32 RSUM', 'h16') for nk in (1, 2, 3, 4)] +
    ['xwgradk %s k%d NK%d' % (st, k, nk) for st in BOTH for k in (5, 7, 11) for nk in (1, 2, 3, 4)] +
    ['xwgrad1b f32 RSUM', 'xwgrad1b f32 FW', 'xwgrad1b f32 nonFW', 'xwgrad1b h16 FW', 'xwgrad1b h16 nonFW'] +
    ['xwgrad1s f32', 'xwgrad1s h16'] +
    ['deal'])                                    # dvd_xwgrad_select(3): the walking kernels on whole work items
assert len(REQUIRED) == 53 + 1 and len(set(REQUIRED)) == len(REQUIRED)


def storages_of(case):
    return case[8]


def shape_of(case):
    name, KS, N, Cin, Cout, H, W, G = case[:8]
    return KS, N, Cin, Cout, H, W, G


# ---- dvd_xwgrad_describe ------------------------------------------------------------------------------------------------
WDESC_INTS, L0, L_INTS = 32, 6, 6                                   # include/dvd_hip.h: DVD_WDESC_*
HEAD = ('family', 'ks', 'h16', 'fw', 'rsum', 'launches')
LAUNCH = ('nk', 'key_nk', 'S', 'slice0', 'strip0', 'ncols')
TAIL = ('second', 'nco', 'nci', 'lds', 'threads', 'slices', 'ws_lo', 'ws_hi', 'chansum', 'deal', 'align')


def describe(lib, case, storage, rowsum=False):
    """-> (status, dict or None) for the case's shape under the CURRENT dvd_xwgrad_select value."""
    import ctypes
    KS, N, Cin, Cout, H, W, G = shape_of(case)
    out = (ctypes.c_int * WDESC_INTS)()
    st = lib.dvd_xwgrad_describe(KS, N, Cin, Cout, H, W, G, int(storage == H16), int(bool(rowsum)), ctypes.addressof(out))
    if st != 0:
        return st, None
    d = dict(zip(HEAD, out[:len(HEAD)]))
    d['L'] = [dict(zip(LAUNCH, out[L0 + i * L_INTS:L0 + (i + 1) * L_INTS])) for i in range(d['launches'])]
    d.update(zip(TAIL, out[L0 + 2 * L_INTS:L0 + 2 * L_INTS + len(TAIL)]))
    d['need'] = d['ws_lo'] + (d['ws_hi'] << 31)
    return st, d


def keys_of(d):
    """The instantiation keys of a described call, one per launch (REQUIRED's spelling), and 'deal' under hook 3."""
    fam, st = FAMILIES[d['family']], H16 if d['h16'] else F32
    keys = set()
    for launch in d['L']:
        nk = launch['key_nk']
        if fam == 'xwgrad3':
            keys.add('xwgrad3 %s %s' % (st, 'FW NK%d' % nk if d['fw'] else 'nonFW'))
        elif fam == 'xwgrad3g':
            keys.add('xwgrad3g %s%s NK%d' % (st, ' RSUM' if d['rsum'] else '', nk))
        elif fam == 'xwgradk':
            keys.add('xwgradk %s k%d NK%d' % (st, d['ks'], nk))
        elif fam == 'xwgrad1b':
            keys.add('xwgrad1b %s %s' % (st, 'RSUM' if d['rsum'] else 'FW' if d['fw'] else 'nonFW'))
        else:
            keys.add('xwgrad1s %s' % st)
    if d['deal']:
        keys.add('deal')
    return keys


def runs_of(case):
    """(storage, rowsum, hook) of every launch configuration tests/test_70 runs for the case."""
    out = []
    for st in storages_of(case):
        for hook in case[11]:
            out.append((st, False, hook))
            if case[10] and st == F32:
                out.append((st, True, hook))
    return out


# ---- data ---------------------------------------------------------------------------------------------------------------
def _gen(case, salt):
    return torch.Generator().manual_seed(zlib.crc32(('%s/%s' % (case[0], salt)).encode()))


def exact_data(case):
    """Integers in [-3, 3] (both extremes present; x with -0.0 among its zeros), exact in fp16 as well."""
    KS, N, Cin, Cout, H, W, G = shape_of(case)
    g = _gen(case, 'exact')
    x = torch.randint(-3, 4, (N, Cin, H, W), generator=g).float()
    gy = torch.randint(-3, 4, (N, Cout, H, W), generator=g).float()
    for t in (x, gy):
        f = t.view(-1)
        f[0], f[-1] = 3.0, -3.0
    xf = x.view(-1)
    zeros = (xf == 0).nonzero().view(-1)
    xf[zeros[::2]] = -0.0
    return {'x': x, 'gy': gy, 'x_amax': 3.0, 'gy_amax': 3.0}


SPLIT_BUDGET = 80            # nonzero gy pixels per output channel: 80 (49 2^22 + 2 * 49 2^10) < 2^34 = 2^24 units of 2^10


def _edge_columns(W, strip):
    e = set()
    for c0 in range(0, W, strip):
        e.add(c0)
        e.add(min(c0 + strip, W) - 1)
    return sorted(e)


def _ab(shape, g):
    a = torch.randint(4, 8, shape, generator=g).double() * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)
    b = torch.randint(-7, 8, shape, generator=g).double()
    # |a| = 4 sits on a binade's lower edge, where fp16 is twice as fine below: b points away from zero there, so h = a 2^11
    b = torch.where(a.abs() == 4, b.abs() * a.sign(), b)
    return a + b * 2.0 ** -12


def split_data(case):
    """x = a + b 2^-12 everywhere; gy the same on at most SPLIT_BUDGET pixels per output channel (all images together), in every
    row: the first and last column of every strip (1x1: of every 16-pixel chunk of the flattened plane) first, the rest of the
    budget on the other columns, both rotating with the row and the channel -- every output channel has its own dW, so between
    them the channels put a gradient on every column (every position of an 8-pixel cell and of a 16-pixel K step, each next to
    every tap's neighbour) and on every strip edge.  max|a| = 7 sits in both tensors."""
    KS, N, Cin, Cout, H, W, G = shape_of(case)
    g = _gen(case, 'split')
    x = _ab((N, Cin, H, W), g)
    x.view(-1)[0] = 7.0 + 5 * 2.0 ** -12
    full = _ab((N, Cout, H, W), g)
    rows, width, strip = (1, H * W, 16) if KS == 1 else (H, W, 64)
    assert N * rows <= SPLIT_BUDGET
    edges = _edge_columns(width, strip)
    others = [c for c in range(width) if c not in set(edges)]
    m = max(1, min(width, SPLIT_BUDGET // (N * rows)))
    keep = torch.zeros(N, Cout, rows, width, dtype=torch.bool)
    for n in range(N):
        for r in range(rows):
            for co in range(Cout):
                turn = (n * rows + r) * Cout + co
                if m > len(edges):
                    cols = edges + [others[(turn * (m - len(edges)) + j) % len(others)] for j in range(min(m - len(edges), len(others)))]
                else:                 # too few per row for all the edges: edges and other columns take turns
                    order = (edges + others) if turn % 2 == 0 else (others + edges)
                    cols = [order[(turn // 2 * m + j) % len(order)] for j in range(m)]
                keep[n, co, r, cols] = True
    gy = torch.where(keep.view(N, Cout, H, W), full, torch.zeros_like(full))
    gy[0, :, 0, 0] = -(7.0 + 3 * 2.0 ** -12)                    # (column 0 of row 0 is an edge: within the budget's slack below)
    assert int((gy != 0).sum((0, 2, 3)).max()) <= SPLIT_BUDGET + 1
    x32, gy32 = x.float(), gy.float()
    assert torch.equal(x32.double(), x) and torch.equal(gy32.double(), gy)
    return {'x': x32, 'gy': gy32, 'x_amax': float(x32.abs().max()), 'gy_amax': float(gy32.abs().max())}


# ---- the kernel arithmetic of csrc/dvd_split.h, emulated ------------------------------------------------------------------
def pow2_scale(amax):
    """2^e with amax 2^e in [2^13, 2^14); 1 for 0, Inf, NaN."""
    a = np.float32(amax)
    if not (a > 0) or not np.isfinite(a):
        return 1.0
    e = (int(a.view(np.uint32)) >> 23) & 0xff
    se = min(max(267 - e, 1), 254)
    return float(np.uint32(se << 23).view(np.float32))


def split_terms(t, amax, relu=False):
    """-> (h, l, scale): the two fp16 terms (as float64 tensors) of act(t) * scale, rounded to nearest even as the hardware
    conversion does; the products and differences in between are fp32."""
    s = pow2_scale(amax)
    v = t.float().clamp_min(0.0) if relu else t.float()
    xs = (v.numpy().astype(np.float32) * np.float32(s)).astype(np.float32)
    h = xs.astype(np.float16)
    l = (xs - h.astype(np.float32)).astype(np.float32).astype(np.float16)
    return torch.from_numpy(h.astype(np.float64)), torch.from_numpy(l.astype(np.float64)), s


def split_expected(case, data):
    """-> (what the fp32 kernels compute: sum (h h' + h l' + l h') / (scale scale'), the float64 truth)."""
    KS, N, Cin, Cout, H, W, G = shape_of(case)
    xh, xl, sx = split_terms(data['x'], data['x_amax'], case[9])
    gh, gl, sg = split_terms(data['gy'], data['gy_amax'])
    kern = (wgrad(xh, gh, KS, G) + wgrad(xl, gh, KS, G) + wgrad(xh, gl, KS, G)) / (sx * sg)
    return kern, spec(data['x'], data['gy'], KS, G, case[9])[0]


def granule(*ts):
    """The largest power of two every entry of the tensors is an integer multiple of."""
    v = torch.cat([t.reshape(-1) for t in ts]).abs().unique()
    v = v[v != 0]
    if v.numel() == 0:
        return 1.0
    k = 40
    while k > -60 and not bool(((v / 2.0 ** k) == (v / 2.0 ** k).round()).all()):
        k -= 1
    return 2.0 ** k


def worst_partial_sum(case, xh, xl, gh, gl):
    """max over the accumulators of sum |terms| -- a bound on every partial sum in every order -- in units of the terms' common
    granularity."""
    KS, N, Cin, Cout, H, W, G = shape_of(case)
    unit = min(granule(a) * granule(b) for a, b in ((xh, gh), (xl, gh), (xh, gl)) if bool(a.any()) and bool(b.any()))
    tot = wgrad(xh.abs(), gh.abs(), KS, G) + wgrad(xl.abs(), gh.abs(), KS, G) + wgrad(xh.abs(), gl.abs(), KS, G)
    return float(tot.max()) / unit


# ---- real-valued data -----------------------------------------------------------------------------------------------------
def real_data(case):
    KS, N, Cin, Cout, H, W, G = shape_of(case)
    g = _gen(case, 'real')
    return {'x': torch.randn(N, Cin, H, W, generator=g), 'gy': torch.randn(N, Cout, H, W, generator=g)}
