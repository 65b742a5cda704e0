"""Specification of the depth metrics (csrc/select.hip, csrc/depth_score.hip, models/score_depth.py): test infrastructure, plain
numpy on the CPU, nothing of the product.

  median(num, den, mask, den_min)   fp32 quotients by numpy, then np.median per segment: numpy IS the yardstick
  median_by_rule(...)               the same from the stated rule (sorted values, the two middle ranks, the sum first in fp32)
  score(...)                        the per-pixel terms in float64 (or, as the yardstick of the fp32 kernel, in fp32), with the sums
                                    as exact integers of round(x * 2^shift) over its own maps
  fragile                           pixels whose float64 decision hangs on last bits: gt within 1e-6 relative of g_min, seg within
                                    1e-6 of 0.5, a delta ratio within 1e-5 relative of 1.25^k, a term within 1e-5 relative of its cap
and the seeded input sets the CPU and GPU tests share.
"""
import numpy as np

CAP = 1024.0
LOG_CAP = 32.0
G_MIN = 1e-2
FRAGILE_CAP = 0.01
SUMS = ('n', 'abs_rel', 'sq_rel', 'sq', 'log_sq', 'log', 'n_d1', 'n_d2', 'n_d3')
TERMS = ('abs_rel', 'sq_rel', 'sq', 'log_sq', 'log')            # the value sums, words 1..5
TERM_CAPS = {'abs_rel': CAP, 'sq_rel': CAP, 'sq': CAP, 'log_sq': CAP, 'log': LOG_CAP}
MAPS = ('abs_rel', 'sq', 'log')                                 # what the kernel's maps hold
DELTAS = (1.25, 1.5625, 1.953125)
FLT_MAX = float(np.finfo(np.float32).max)


def ceil_log2(n):
    return (int(n) - 1).bit_length()


def shift_for(n_pixels):
    return min(32, 62 - 10 - ceil_log2(n_pixels))


# -- the median ----------------------------------------------------------------------------------------------------------------
def _selected(num, den, mask, den_min, s):
    sel = den[s] > np.float32(den_min)
    if mask is not None:
        sel = sel & (mask[s] != 0)
    with np.errstate(all='ignore'):
        return (num[s][sel] / den[s][sel]).astype(np.float32)


def median(num, den, mask=None, den_min=0.0):
    """num, den fp32 [S,L], mask uint8 [S,L] or None -> (median fp32 [S], count int64 [S]): np.median of the fp32 quotients."""
    import warnings
    num, den = np.asarray(num, dtype=np.float32), np.asarray(den, dtype=np.float32)
    S = num.shape[0]
    med, cnt = np.empty(S, dtype=np.float32), np.empty(S, dtype=np.int64)
    for s in range(S):
        q = _selected(num, den, mask, den_min, s)
        cnt[s] = q.size
        with warnings.catch_warnings(), np.errstate(all='ignore'):
            warnings.simplefilter('ignore')
            med[s] = np.median(q) if q.size else np.float32('nan')
    return med, cnt


def median_by_rule(num, den, mask=None, den_min=0.0):
    """The same by the stated rule: with the n selected values sorted, v[(n-1)/2] for odd n, (v[n/2-1] + v[n/2]) / 2 with the sum
    formed first in fp32 for even n, NaN for n = 0 or if any value is a NaN."""
    num, den = np.asarray(num, dtype=np.float32), np.asarray(den, dtype=np.float32)
    S = num.shape[0]
    med = np.empty(S, dtype=np.float32)
    for s in range(S):
        v = np.sort(_selected(num, den, mask, den_min, s))
        n = v.size
        if n == 0 or np.isnan(v).any():
            med[s] = np.float32('nan')
        elif n % 2:
            med[s] = v[(n - 1) // 2]
        else:
            with np.errstate(all='ignore'):
                med[s] = np.float32(np.float32(v[n // 2 - 1] + v[n // 2]) / np.float32(2))
    return med


def _bits(u):
    return np.asarray(u, dtype=np.uint32).view(np.float32)


MEDIAN_L = (1, 2, 3, 4, 255, 256, 257, 1000, 4099)
MEDIAN_S = (1, 3, 5)
# the launch cap of csrc/select.hip (kSelectMaxBlocks = 2048 blocks of 256 threads over all segments) and the smallest segment
# lengths at which every block of a segment makes a second trip whose last block is ragged: one element per thread (odd L), one
# segment: 2048 * 256 + 2047 * 256 + 1; four elements per thread, four segments of 512 blocks: 512 * 1024 + 511 * 1024 + 4
SELECT_MAX_BLOCKS = 2048
BEYOND_CAP = {'scalar': (1, SELECT_MAX_BLOCKS * 256 + (SELECT_MAX_BLOCKS - 1) * 256 + 1),
              'vector': (4, (SELECT_MAX_BLOCKS // 4) * 1024 + (SELECT_MAX_BLOCKS // 4 - 1) * 1024 + 4)}


def median_cases():
    """[(name, num, den, mask or None, den_min)]: every data class of the median tests, seeded."""
    out = []
    one = lambda a: np.ones_like(a, dtype=np.float32)
    for S in MEDIAN_S:
        for L in MEDIAN_L:
            r = np.random.RandomState(1000 * S + L)
            num = r.randn(S, L).astype(np.float32)
            den = (r.rand(S, L) * 2.0 - 0.2).astype(np.float32)          # a tenth is not selected (den <= 0)
            out.append(('signed/S%d/L%d' % (S, L), num, den, None, 0.0))
    r = np.random.RandomState(7)
    num, den = r.randn(3, 1000).astype(np.float32), (r.rand(3, 1000) + 0.5).astype(np.float32)
    out.append(('every_other', num, den, (np.arange(3000).reshape(3, 1000) % 2).astype(np.uint8), 0.0))
    num, den = r.randn(3, 257).astype(np.float32), (r.rand(3, 257) + 0.5).astype(np.float32)
    den[1] = 0.0
    out.append(('empty_between', num, den, None, 0.0))
    for L in (1000, 1001):
        num = np.full((1, L), 2.5, dtype=np.float32)
        out.append(('all_equal/L%d' % L, num, one(num), None, 0.0))
    num = np.where(r.permutation(1000) < 500, np.float32(1.5), np.float32(-2.25)).astype(np.float32)[None]
    out.append(('two_values_even_split', num, one(num), None, 0.0))
    num = np.where(r.rand(2, 999) < 0.5, np.float32(1.5), np.float32(-2.25)).astype(np.float32)
    out.append(('two_values', num, one(num), None, 0.0))
    for L in (1000, 1001):
        num = _bits(np.uint32(0x40490F00) | r.randint(0, 256, size=(2, L)).astype(np.uint32))
        out.append(('last_digit/L%d' % L, num, one(num), None, 0.0))
        num = _bits((r.randint(0, 256, size=(2, L)).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00123456))
        out.append(('first_digit/L%d' % L, num, one(num), None, 0.0))
    for L in (1000, 1001):
        lo, hi = r.randn(L // 2 - 20).astype(np.float32) - 10.0, r.randn(L - L // 2 - 20).astype(np.float32) + 10.0
        num = np.concatenate([lo, np.full(40, 0.7853982, dtype=np.float32), hi]).astype(np.float32)
        out.append(('duplicated_middle/L%d' % L, r.permutation(num)[None], np.ones((1, L), dtype=np.float32), None, 0.0))
    num = np.full((1, 70000), 1.7, dtype=np.float32)
    out.append(('equal_70000', num, one(num), None, 0.0))
    num = np.full((1, 70001), 1.7, dtype=np.float32)
    num[0, 123] = -3.0
    out.append(('equal_70000_and_one', num, one(num), None, 0.0))
    for L in (256, 257):
        mag = r.randint(1, 1 << 23, size=(2, L)).astype(np.uint32)
        num = _bits(mag | (r.randint(0, 2, size=(2, L)).astype(np.uint32) << np.uint32(31)))
        out.append(('denormals/L%d' % L, num, one(num), None, 0.0))
    for L in (4, 5, 256, 257):
        num = np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0], dtype=np.float32)[r.randint(0, 6, size=(2, L))]
        out.append(('signed_zeros/L%d' % L, num, one(num), None, 0.0))
    inf = np.float32('inf')
    for L in (256, 257):
        num = r.randn(2, L).astype(np.float32)
        num[:, :40], num[:, 40:90] = inf, -inf
        out.append(('infinities/L%d' % L, r.permutation(num.T).T.copy(), one(num), None, 0.0))
    num = np.array([[-inf, inf], [inf, -inf], [inf, inf]], dtype=np.float32)
    out.append(('minus_inf_plus_inf', num, one(num), None, 0.0))
    num = np.array([[-inf, inf, inf, -inf], [-inf, 1.0, inf, inf]], dtype=np.float32)
    out.append(('infinities_even', num, one(num), None, 0.0))
    num, den = r.randn(3, 300).astype(np.float32), (r.rand(3, 300) + 0.5).astype(np.float32)
    num[1, 17] = np.float32('nan')
    out.append(('nan_selected', num, den, None, 0.0))
    mask = np.ones((3, 300), dtype=np.uint8)
    mask[1, 17] = 0
    out.append(('nan_masked_out', num, den, mask, 0.0))
    num, den = r.randn(3, 300).astype(np.float32), (r.rand(3, 300) + 0.25).astype(np.float32)
    den[:, ::3] = 0.5
    out.append(('den_equal_den_min', num, den, None, 0.5))
    num, den = r.randn(2, 300).astype(np.float32), (r.rand(2, 300) + 0.5).astype(np.float32)
    den[0, 5], den[1, 6] = np.float32('nan'), np.float32('nan')
    out.append(('nan_denominator', num, den, None, 0.0))
    return out


def beyond_cap_case(kind):
    S, L = BEYOND_CAP[kind]
    r = np.random.RandomState(S * 31 + 5)
    num = r.randn(S, L).astype(np.float32)
    den = (r.rand(S, L) * 2.0 - 0.2).astype(np.float32)
    return num, den


# -- the score -----------------------------------------------------------------------------------------------------------------
def score(pred, gt, scale, seg=None, mask=None, g_min=G_MIN, shift=None, dtype=np.float64):
    """pred, gt fp32 [N,1,H,W]; scale fp32 [N]; seg fp32 [N,H,W] or None; mask uint8 [N,H,W] or None.  The terms in `dtype`
    (float64: the specification; float32: the yardstick of an fp32 implementation, operation by operation as specified).
    -> dict: counted, region [N,3,H,W] bool, the five term maps, delta [N,3,H,W] bool, sums [N][3][9] Python integers,
    fragile [N,H,W] bool, n_fragile [N][3], shift."""
    pred, gt = np.asarray(pred, dtype=np.float32), np.asarray(gt, dtype=np.float32)
    N, _, H, W = pred.shape
    if shift is None:
        shift = shift_for(N * H * W)
    T = dtype
    p, g = pred[:, 0].astype(T), gt[:, 0].astype(T)
    sc = np.asarray(scale, dtype=np.float32).astype(T)[:, None, None]
    gm = T(np.float32(g_min))
    with np.errstate(all='ignore'):
        q = sc * p
        counted = (g > gm) & (p > 0) & (np.abs(q) <= T(FLT_MAX))
        if mask is not None:
            counted = counted & (np.asarray(mask) != 0)
        d = q - g
        dd = d * d
        cap, lcap = T(CAP), T(LOG_CAP)
        raw_l = np.log(q) - np.log(g)
        raw = {'abs_rel': np.abs(d) / g, 'sq_rel': dd / g, 'sq': dd, 'log': raw_l, 'log_sq': raw_l * raw_l}      # before the caps
        terms = {k: np.fmin(raw[k], cap) for k in ('abs_rel', 'sq_rel', 'sq')}
        terms['log'] = np.fmin(np.fmax(raw_l, -lcap), lcap)
        terms['log_sq'] = np.fmin(terms['log'] * terms['log'], cap)
        ratio = np.fmax(q / g, g / q)
        delta = np.stack([ratio < T(t) for t in DELTAS], 1) & counted[:, None]
    terms = {k: np.where(counted, v, T(0)).astype(T) for k, v in terms.items()}
    region = np.zeros((N, 3, H, W), dtype=bool)
    region[:, 0] = counted
    if seg is not None:
        sg = np.asarray(seg, dtype=np.float32)
        region[:, 1], region[:, 2] = counted & (sg <= np.float32(0.5)), counted & (sg > np.float32(0.5))
    # fragile: where the decision of the float64 run hangs on last bits
    with np.errstate(all='ignore'):
        g64, q64 = gt[:, 0].astype(np.float64), np.asarray(scale, dtype=np.float32).astype(np.float64)[:, None, None] * pred[:, 0]
        fragile = np.abs(g64 - float(np.float32(g_min))) <= 1e-6 * float(np.float32(g_min))
        fragile |= np.abs(np.abs(q64) - FLT_MAX) <= 1e-6 * FLT_MAX
        if seg is not None:
            fragile |= np.abs(np.asarray(seg, dtype=np.float64) - 0.5) <= 1e-6
        r64 = np.fmax(q64 / g64, g64 / q64)
        for t in DELTAS:
            fragile |= counted & (np.abs(r64 - t) <= 1e-5 * t)
        for k in TERMS:
            # (the term before its cap: a term far beyond the cap is capped in every arithmetic)
            fragile |= counted & (np.abs(np.abs(raw[k].astype(np.float64)) - TERM_CAPS[k]) <= 1e-5 * TERM_CAPS[k])
    two = float(2 ** shift)
    fixed = {k: np.rint(terms[k].astype(np.float64) * two).astype(np.int64) for k in TERMS}
    sums = [[[0] * 9 for _ in range(3)] for _ in range(N)]
    n_fragile = [[0] * 3 for _ in range(N)]
    for n in range(N):
        for r in range(3):
            m = region[n, r]
            row = [int(m.sum())] + [sum(int(v) for v in fixed[k][n][m]) for k in TERMS]
            row += [int((delta[n, j] & m).sum()) for j in range(3)]
            sums[n][r] = row
            # (a fragile pixel may enter or leave any row of its frame: seg near 0.5 moves it between rows 1 and 2)
            n_fragile[n][r] = int(fragile[n].sum())
    out = dict(terms)
    out.update(counted=counted, region=region, delta=delta, sums=sums, fragile=fragile, n_fragile=n_fragile, shift=shift)
    return out


def fragile_share(res):
    """Fragile pixels as a share of all pixels of the input set."""
    return float(res['fragile'].mean())


def derive(row, shift):
    """The reported quantities from one row of nine integers, in float64 (NaN for n = 0)."""
    n = row[0]
    if n == 0:
        return {k: float('nan') for k in ('abs_rel', 'sq_rel', 'rmse', 'rmse_log', 'silog', 'd1', 'd2', 'd3')}
    two = 2.0 ** -shift
    m = [float(np.float64(v) * two / np.float64(n)) for v in row[1:6]]
    return {'abs_rel': m[0], 'sq_rel': m[1], 'rmse': float(np.sqrt(m[2])), 'rmse_log': float(np.sqrt(m[3])),
            'silog': m[3] - m[4] * m[4], 'd1': row[6] / n, 'd2': row[7] / n, 'd3': row[8] / n}


SCORE_SHAPES = ((1, 1), (11, 21), (12, 24), (36, 40))
SCORE_N = 3


def score_case(H, W, seed=0):
    """Seeded inputs of the kernel tests: N = 3 frames; a ground truth with holes (15 % at or below g_min), a prediction off by
    a factor of about 1.7 with log-normal noise, a few wild predictions that reach the caps, a few non-positive ones; a motion
    segmentation of zeros, ones and a few values in between; a mask that drops a tenth."""
    N = SCORE_N
    r = np.random.RandomState(100 * H + W + 7919 * seed)
    gt = (0.5 + 7.5 * r.rand(N, 1, H, W)).astype(np.float32)
    hole = r.rand(N, 1, H, W) < 0.15
    gt[hole] = np.where(r.rand(int(hole.sum())) < 0.5, 0.0, 0.004).astype(np.float32)
    pred = (gt * 1.7 * np.exp(0.25 * r.randn(N, 1, H, W))).astype(np.float32)
    pred[hole] = (1.0 + r.rand(int(hole.sum()))).astype(np.float32)
    wild = r.rand(N, 1, H, W) < 0.03
    pred[wild] *= np.float32(3000.0)
    pred[r.rand(N, 1, H, W) < 0.03] = np.float32(0.0)
    pred[r.rand(N, 1, H, W) < 0.01] = np.float32(-1.5)
    seg = (r.rand(N, H, W) < 0.35).astype(np.float32)
    soft = r.rand(N, H, W) < 0.1
    seg[soft] = r.rand(int(soft.sum())).astype(np.float32)
    mask = (r.rand(N, H, W) < 0.9).astype(np.uint8) * np.uint8(3)
    scale = np.array([1.0 / 1.7, 0.5, 0.61], dtype=np.float32)
    return {'pred': pred, 'gt': gt, 'seg': seg, 'mask': mask, 'scale': scale, 'N': N, 'H': H, 'W': W}
