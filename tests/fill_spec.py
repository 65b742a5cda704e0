"""The specification of push-pull hole filling (csrc/fill.hip, ops.fill_holes) in numpy, in the dtype it is asked for, and the
case table of the tests.

    level 0   a = known != 0 ? bias^power : 0, the power by repeated multiplication (1 without bias or with power 0); a pixel
              whose a is not finite or not > 0 is unknown, and so is one whose bias (where it is used) is not > 0, which an
              even power would hide; the value of an unknown pixel is never read into a result
    pull      level l + 1 is (ceil(H_l / 2), ceil(W_l / 2)), up to the 1 x 1 level L.  Over the children (2y+dy, 2x+dx) inside
              the level, in the order (0,0) (0,1) (1,0) (1,1):  A = sum a_c, n = #{a_c > 0};
              n > 0: v' = (sum a_c v_c) / A, a' = A / n;  else v' = a' = 0
    push      from level L - 1 down to 0 a pixel with a_l > 0 keeps v_l; any other takes the bilinear sample of the completed
              level above at ((y + .5) / 2 - .5, (x + .5) / 2 - .5): 0.75 x the parent x >> 1 plus 0.25 x the neighbour
              (x >> 1) + (x odd ? 1 : -1), its index clamped to the level; horizontal pairs first, then the vertical pair.
              a_L == 0: the view has no known pixel and all its values become `fill`
    level     0 known, k >= 1 the lowest level at which an ancestor (y >> k, x >> k) is known, 255 for such a view

Every product, sum and quotient is one operation of `dtype`, sums run from left to right; a child outside the level enters
its sums as a = 0, v = 0 (adding +0 changes no sum).  In float32 this is, statement for statement, what the kernels execute.
"""
import numpy as np

EMPTY = 255


def weights(known, bias, power, dtype):
    """a0 [H,W] of one view."""
    p = np.ones(known.shape, dtype)
    ok = known != 0
    if bias is not None and int(power) > 0:
        b = np.asarray(bias).astype(dtype)
        for _ in range(int(power)):
            with np.errstate(all='ignore'):
                p = p * b
        with np.errstate(invalid='ignore'):
            ok = ok & (b > 0)
    with np.errstate(invalid='ignore'):
        ok = ok & np.isfinite(p) & (p > 0)
    return np.where(ok, p, dtype(0)).astype(dtype)


def _children(x):
    """[..., h, w] -> its four child planes [..., ceil(h/2), ceil(w/2)] in the order (0,0) (0,1) (1,0) (1,1), 0 outside."""
    h, w = x.shape[-2:]
    pad = np.zeros(x.shape[:-2] + (h + (h & 1), w + (w & 1)), x.dtype)
    pad[..., :h, :w] = x
    return pad[..., 0::2, 0::2], pad[..., 0::2, 1::2], pad[..., 1::2, 0::2], pad[..., 1::2, 1::2]


def pull(a, v):
    """One level up: a [h,w], v [C,h,w] -> (a', v')."""
    dtype = a.dtype.type
    a0, a1, a2, a3 = _children(a)
    v0, v1, v2, v3 = _children(v)
    A = ((a0 + a1) + a2) + a3
    n = (a0 > 0).astype(np.int32) + (a1 > 0) + (a2 > 0) + (a3 > 0)
    S = ((a0 * v0 + a1 * v1) + a2 * v2) + a3 * v3
    some = n > 0
    with np.errstate(all='ignore'):
        an = np.where(some, A / np.maximum(n, 1).astype(dtype), dtype(0)).astype(dtype)
        vn = np.where(some, S / np.where(some, A, dtype(1)), dtype(0)).astype(dtype)
    return an, vn


def _parents(n, n_up):
    x = np.arange(n)
    xp = x >> 1
    xn = np.clip(xp + np.where(x & 1, 1, -1), 0, n_up - 1)
    return xp, xn


def push(a, v, up):
    """One level down: a [h,w], v [C,h,w] of this level, `up` [C,h',w'] the completed level above -> the completed v."""
    dtype = a.dtype.type
    h, w = a.shape
    yp, yn = _parents(h, up.shape[-2])
    xp, xn = _parents(w, up.shape[-1])
    q, r = dtype(0.75), dtype(0.25)
    top = q * up[:, yp][:, :, xp] + r * up[:, yp][:, :, xn]
    bot = q * up[:, yn][:, :, xp] + r * up[:, yn][:, :, xn]
    return np.where(a > 0, v, q * top + r * bot).astype(dtype)


def fill_view(values, known, bias=None, power=0, fill=0.0, dtype=np.float64):
    """values [C,H,W], known [H,W], bias [H,W] or None -> (completed values [C,H,W] of `dtype`, level uint8 [H,W])."""
    dtype = np.dtype(dtype).type
    a = weights(known, bias, power, dtype)
    v = np.where(a > 0, np.asarray(values).astype(dtype), dtype(0)).astype(dtype)
    As, Vs = [a], [v]
    while As[-1].shape != (1, 1):
        a, v = pull(As[-1], Vs[-1])
        As.append(a)
        Vs.append(v)
    H, W = known.shape
    if not As[-1][0, 0] > 0:
        return np.full(v.shape[:1] + (H, W), dtype(fill), dtype), np.full((H, W), EMPTY, np.uint8)
    done = Vs[-1]
    for lv in range(len(As) - 2, -1, -1):
        done = push(As[lv], Vs[lv], done)
    level = np.full((H, W), EMPTY, np.int32)
    y, x = np.mgrid[0:H, 0:W]
    for k in range(len(As) - 1, -1, -1):
        level = np.where(As[k][y >> k, x >> k] > 0, k, level)
    # a known pixel is its input, bit for bit, in whatever dtype the input came
    return done, level.astype(np.uint8)


def fill(values, known, bias=None, power=0, fill=0.0, dtype=np.float64):
    """values [V,C,H,W], known [V,H,W], bias [V,1,H,W] or None -> {'values', 'level'}: every view on its own."""
    out = [fill_view(values[i], known[i], None if bias is None else bias[i, 0], power, fill, dtype) for i in range(len(values))]
    return {'values': np.stack([o[0] for o in out]), 'level': np.stack([o[1] for o in out])}


# -- the case table -----------------------------------------------------------------------------------------------------------
def _smooth(rng, V, C, H, W):
    """Values in [0, 1]: a smooth field plus noise, so that both interpolation and averaging have something to get wrong."""
    y, x = np.mgrid[0:H, 0:W]
    ph = rng.random((V, C, 1, 1)) * 6.0
    f = 0.5 + 0.3 * np.sin(0.31 * x + ph) * np.cos(0.23 * y - ph) + 0.2 * (rng.random((V, C, H, W)) - 0.5)
    return np.clip(f, 0.0, 1.0).astype(np.float32)


def make(name, C=4, seed=0):
    """-> dict(values [V,C,H,W] fp32, known uint8 [V,H,W], bias fp32 [V,1,H,W] in [0.5, 20], fill)."""
    H, W, V, kind = CASES[name]
    rng = np.random.default_rng([seed, sorted(CASES).index(name), C])
    values = _smooth(rng, V, C, H, W)
    bias = (0.5 + 19.5 * rng.random((V, 1, H, W))).astype(np.float32)
    known = (rng.random((V, H, W)) < 0.5).astype(np.uint8)
    if kind == 'hole':                       # a 50 x 40 hole and 2 % known elsewhere: levels >= 6 decide the middle of the hole
        known = (rng.random((V, H, W)) < 0.02).astype(np.uint8)
        known[:, 20:70, 45:85] = 0
    elif kind == 'corner':
        known[:] = 0
        known[:, H - 1, W - 1] = 1
    elif kind == 'all':
        known[:] = 1
    elif kind == 'one_empty':
        known[1] = 0
    elif kind == 'borders':                  # holes across the borders of the 32 x 32 tiles, and data only next to them
        known = (rng.random((V, H, W)) < 0.3).astype(np.uint8)
        known[:, 28:37, :] = 0
        known[:, :, 30:35] = 0
        known[:, :, 60:] = 0
    elif kind == 'bad_bias':                 # known pixels whose weight is 0, negative, Inf or NaN count as unknown
        flat = bias.reshape(V, -1)
        idx = rng.permutation(H * W)[:8]
        for j, bad in enumerate((0.0, -3.0, np.inf, np.nan)):
            flat[:, idx[2 * j:2 * j + 2]] = bad
            known.reshape(V, -1)[:, idx[2 * j:2 * j + 2]] = 1
    # what an unknown pixel holds must not matter: poison a few of them
    poison = (known == 0) & (rng.random((V, H, W)) < 0.1)
    values[np.broadcast_to(poison[:, None], values.shape)] = np.nan
    return {'values': values, 'known': known, 'bias': bias, 'fill': -7.5}


# name -> (H, W, V, kind)
CASES = {
    '2x2': (2, 2, 1, 'random'),
    '1x7': (1, 7, 1, 'random'),
    '11x21': (11, 21, 2, 'random'),                  # one partial tile
    '33x65': (33, 65, 1, 'borders'),                 # several tiles, odd sizes, holes across tile borders
    '70x45': (70, 45, 1, 'borders'),
    '36x64': (36, 64, 1, 'random'),                  # W % 4 == 0: the four-pixel accesses
    '97x130': (97, 130, 1, 'hole'),                  # the middle kernel, levels >= 6
    'corner': (33, 40, 1, 'corner'),
    'all_known': (12, 20, 1, 'all'),
    'one_empty': (11, 24, 3, 'one_empty'),
    'bad_bias': (11, 21, 1, 'bad_bias'),
}


def worst(got, want):
    """The largest |got - want|; a NaN on either side counts as infinitely far."""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    return float(np.where(np.isnan(d), np.inf, d).max()) if d.size else 0.0


def limit(case, r64, r32):
    """4 x the distance of the float32 from the float64 evaluation of the specification on this case, plus 2 ulp of the largest
    value that counts (the rule of tests/test_48_splat_gpu.py)."""
    top = np.float32(np.abs(r64['values']).max())
    return 4.0 * worst(r32['values'], r64['values']) + 2.0 * float(np.spacing(top))
