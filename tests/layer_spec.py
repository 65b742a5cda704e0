"""Float64 specification of the element-wise and small-window layers between the matrix kernels of a depth-net step, and a
restatement of their host dispatch: csrc/bnrelu.hip (BatchNorm + residual + ReLU), csrc/upsample.hip (bilinear resize),
csrc/pool.hip maxpool3s2_* (max-pool 3/2/1) and csrc/gconv.hip (plain 8-per-group 3x3).  Plain numpy / torch on the CPU.

Three kinds of things live here, shared by tests/test_layer_spec_cpu.py and tests/test_68_layer_kernels_gpu.py:
  * the operations in float64, each with the same operation on absolute values (`M`, the scale of the rounding error);
  * the path predicates: which loop, tile or kernel the host code picks for a shape, with the source line quoted beside each;
  * the case tables of the GPU test, every row naming the path it is there for (the CPU test holds the rows to the predicates),
    and the rounding counts `c` of the bounds |got - spec| <= c * 2^-24 * M (derived in the GPU test's docstrings)."""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24                  # unit roundoff of fp32
F32 = np.float32


# ============================================================================================================================
# BatchNorm (eval) + residual + ReLU                                                                       csrc/bnrelu.hip
# ============================================================================================================================
BN_EPS = 1e-5
K_BN_CHUNK = 4096               # bnrelu.hip:24   `constexpr int kBnChunk = 4096`


def bn_eps32(eps=BN_EPS):
    """The eps the kernels see: the entry points take a `float`."""
    return float(F32(eps))


def bn_scale(gamma, beta, mean, var, eps=BN_EPS):
    """(s, b, rstd) in float64 from the fp32 parameters: s = gamma / sqrt(var + eps), b = beta - mean * s."""
    gamma, beta, mean, var = (np.asarray(a, dtype=np.float64) for a in (gamma, beta, mean, var))
    rstd = 1.0 / np.sqrt(var + bn_eps32(eps))
    s = gamma * rstd
    return s, beta - mean * s, rstd


def _c(v):
    return v[None, :, None, None]


def bn_forward(x, r, gamma, beta, mean, var, relu, eps=BN_EPS):
    """-> (y, pre, M): pre = x s + b (+ r), y = max(0, pre) with relu else pre, M = |x||s| + |beta| + |mean||s| + |r|."""
    x = np.asarray(x, dtype=np.float64)
    s, b, _ = bn_scale(gamma, beta, mean, var, eps)
    pre = x * _c(s) + _c(b)
    M = np.abs(x) * _c(np.abs(s)) + _c(np.abs(np.asarray(beta, dtype=np.float64)) + np.abs(np.asarray(mean, dtype=np.float64)) * np.abs(s))
    if r is not None:
        r = np.asarray(r, dtype=np.float64)
        pre = pre + r
        M = M + np.abs(r)
    return (np.maximum(pre, 0.0) if relu else pre), pre, M


def bn_backward(gy, mask, x, gamma, mean, var, eps=BN_EPS):
    """The backward with the ReLU mask GIVEN (the kernel masks with its own stored y; None: no ReLU).
    -> dict gx, gr, ggamma, gbeta and M_gx = |g||s|, M_gbeta = sum |g|, M_ggamma = rstd sum |g||x - mean|."""
    gy, x = np.asarray(gy, dtype=np.float64), np.asarray(x, dtype=np.float64)
    mean64 = np.asarray(mean, dtype=np.float64)
    s, _, rstd = bn_scale(gamma, np.zeros_like(mean64), mean, var, eps)
    g = gy if mask is None else gy * np.asarray(mask, dtype=np.float64)
    d = x - _c(mean64)
    return dict(gx=g * _c(s), gr=g, gbeta=g.sum((0, 2, 3)), ggamma=(g * d).sum((0, 2, 3)) * rstd,
                M_gx=np.abs(g) * _c(np.abs(s)), M_gbeta=np.abs(g).sum((0, 2, 3)),
                M_ggamma=(np.abs(g) * np.abs(d)).sum((0, 2, 3)) * rstd)


# ---- host dispatch ------------------------------------------------------------------------------------------------------
def bn_chunks(HW):
    """bnrelu.hip:299  `const int chunks = (HW + dvd::kBnChunk - 1) / dvd::kBnChunk;`"""
    return (HW + K_BN_CHUNK - 1) // K_BN_CHUNK


def bn_vec(HW):
    """bnrelu.hip:40 and :117  `if ((HW & 3) == 0)`: the 16-byte loop, else the scalar loop."""
    return HW % 4 == 0


def bn_bwd_npb(N, C, HW):
    """Images of a channel per block of bnrelu_bwd_kernel.  bnrelu.hip:301-307
         int npb = 1;
         if (chunks == 1 && HW <= dvd::kBnChunk / 2) {
           npb = dvd::kBnChunk / HW;
           while (npb > 1 && (long long)C * ((N + npb - 1) / npb) < 1024) npb >>= 1;
           if (npb > N) npb = N;
           if (npb < 1) npb = 1;
         }"""
    npb = 1
    if bn_chunks(HW) == 1 and HW <= K_BN_CHUNK // 2:
        npb = K_BN_CHUNK // HW
        while npb > 1 and C * ((N + npb - 1) // npb) < 1024:
            npb >>= 1
        npb = max(1, min(npb, N))
    return npb


def bn_records(N, C, HW):
    """bnrelu.hip:308  `const int records = npb > 1 ? (N + npb - 1) / npb : N * chunks;`  (per channel)"""
    npb = bn_bwd_npb(N, C, HW)
    return (N + npb - 1) // npb if npb > 1 else N * bn_chunks(HW)


def bn_last_chunk(HW):
    """Elements of a plane's last chunk: bnrelu.hip:113  `lo = chunk * kBnChunk, hi = min(HW, lo + kBnChunk)`."""
    return HW - (bn_chunks(HW) - 1) * K_BN_CHUNK


def bn_thread_trips(N, C, HW):
    """The most loop trips one thread of bnrelu_bwd_kernel adds into its two sums: thread 0 of a full block.  A trip takes a
    quad (bnrelu.hip:118 `i += 1024`) or an element (:138 `i += 256`); an npb block repeats them for its images (:115)."""
    per_trip = 1024 if bn_vec(HW) else 256
    span = min(HW, K_BN_CHUNK)
    return min(bn_bwd_npb(N, C, HW), N) * ((span + per_trip - 1) // per_trip)


# ---- rounding counts (derivations: the docstring of the GPU test) -------------------------------------------------------------
def bn_c_y(res):
    return 7 if res else 6


BN_C_GX = 4
WAVE_TREE = 6 + 2               # wave_sum's six shuffle-adds, then (a + b) + (c + d) over the four waves
STORE = 1                       # the double sum over the records, rounded once to the fp32 result


def bn_c_gbeta(N, C, HW):
    trips = bn_thread_trips(N, C, HW)
    return (2 if bn_vec(HW) else 0) + (trips - 1) + WAVE_TREE + STORE


def bn_c_ggamma(N, C, HW):
    trips = bn_thread_trips(N, C, HW)
    return 1 + (4 if bn_vec(HW) else 1) * trips + WAVE_TREE + STORE


# ---- cases ----------------------------------------------------------------------------------------------------------------------
# shape -> the path it is there for: npb, records per channel, 16-byte loop, chunks, elements of the last chunk
BN_PATHS = {
    (5, 512, 4, 4): dict(npb=4, records=2, vec=True, chunks=1, last=16),          # the second block holds one image
    (5, 512, 3, 5): dict(npb=4, records=2, vec=False, chunks=1, last=15),         # the same on the scalar loop
    (3, 1024, 2, 3): dict(npb=3, records=1, vec=False, chunks=1, last=6),         # npb = N: one record per channel
    (2, 3, 50, 82): dict(npb=1, records=4, vec=True, chunks=2, last=4),           # a last chunk of one quad, N > 1
    (1, 2, 17, 241): dict(npb=1, records=2, vec=False, chunks=2, last=1),         # a last chunk of one element
    (2, 2, 64, 64): dict(npb=1, records=2, vec=True, chunks=1, last=4096),        # exactly one chunk
}
# (shape, residual, relu, affine, x requires grad, gamma / beta frozen): every option both ways, every shape at least once,
# relu=False and a missing gx on an npb > 1 shape
BN_CASES = [
    ((5, 512, 4, 4), True, True, True, True, False),
    ((5, 512, 4, 4), False, False, True, True, False),
    ((5, 512, 3, 5), False, False, True, True, False),
    ((5, 512, 3, 5), True, True, True, False, False),
    ((3, 1024, 2, 3), True, True, True, True, False),
    ((3, 1024, 2, 3), False, True, False, True, False),
    ((2, 3, 50, 82), False, True, True, True, True),
    ((2, 3, 50, 82), True, True, True, False, True),
    ((2, 3, 50, 82), True, True, True, True, False),
    ((1, 2, 17, 241), True, True, False, True, False),
    ((1, 2, 17, 241), False, True, True, True, False),
    ((2, 2, 64, 64), True, False, True, True, False),
    ((2, 2, 64, 64), False, True, True, True, False),
]


def bn_case_id(case):
    (N, C, H, W), res, relu, affine, xgrad, frozen = case
    return '%dx%dx%dx%d%s%s%s%s%s' % (N, C, H, W, '_res' if res else '', '' if relu else '_norelu', '' if affine else '_noaffine',
                                       '' if xgrad else '_nogx', '_frozen' if frozen else '')


def bn_inputs(case):
    """Seeded fp32 inputs of a case: some negative gamma, var down to 0.05, mean of the size of x; with C >= 3 channel 0 has
    beta = -100 (fully masked behind a ReLU) and the last channel gy == 0.  affine=False: gamma = 1, beta = 0."""
    (N, C, H, W), res, relu, affine, _, _ = case
    g = torch.Generator().manual_seed(680000 + 1000 * C + 10 * H + W + 7 * int(res) + 3 * int(relu))
    gamma = 1.0 + 0.3 * torch.randn(C, generator=g)
    gamma[1::3] = -gamma[1::3]
    beta = 0.2 * torch.randn(C, generator=g)
    mean = torch.randn(C, generator=g)
    var = 0.05 + 2.0 * torch.rand(C, generator=g)
    var[1 % C] = 0.05
    x = torch.randn(N, C, H, W, generator=g)
    r = torch.randn(N, C, H, W, generator=g) if res else None
    gy = torch.randn(N, C, H, W, generator=g)
    if C >= 3:
        beta[0] = -100.0
        gy[:, C - 1] = 0.0
    if not affine:
        gamma, beta = torch.ones(C), torch.zeros(C)
    return dict(x=x, r=r, gy=gy, gamma=gamma, beta=beta, mean=mean, var=var)


# ============================================================================================================================
# Bilinear resize                                                                                         csrc/upsample.hip
# ============================================================================================================================
def up_scale(n_in, n_out, align):
    """upsample.hip:315-318 (make_axis), in fp32:
         if (align) a.scale = n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.0f;
         else       a.scale = (float)n_in / (float)n_out;"""
    if align:
        return F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0.0)
    return F32(n_in) / F32(n_out)


def up_axis(n_in, n_out, align):
    """-> (i0, i1, w0, w1): the source coordinate in FLOAT32 exactly as upsample.hip:28-41 (src_index; -ffp-contract=off) forms
    it -- align: s = scale * dst; else s = max(0, scale * (dst + 0.5) - 0.5); i0 = min(int(s), n_in - 1), i1 = i0 + (i0 < n_in - 1),
    w1 = s - i0 (exact in fp32) -- and w0 = 1 - w1 in float64 (the kernel's fp32 difference is one of the counted roundings)."""
    scale = up_scale(n_in, n_out, align)
    dst = np.arange(n_out, dtype=np.float32)
    if align:
        s = scale * dst
    else:
        s = np.maximum(F32(0.0), scale * (dst + F32(0.5)) - F32(0.5))
    assert s.dtype == np.float32
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    w1 = s - i0.astype(np.float32)
    assert w1.dtype == np.float32
    w1 = w1.astype(np.float64)
    return i0, i1, 1.0 - w1, w1


def up_matrix(n_in, n_out, align):
    """The interpolation matrix [n_out, n_in] of an axis (float64 entries)."""
    i0, i1, w0, w1 = up_axis(n_in, n_out, align)
    m = np.zeros((n_out, n_in))
    o = np.arange(n_out)
    np.add.at(m, (o, i0), w0)
    np.add.at(m, (o, i1), w1)
    return m


def up_forward(x, out_hw, align):
    """-> (y, M): y = My x Mx^T and M = |My| |x| |Mx|^T over the last two axes."""
    x = np.asarray(x, dtype=np.float64)
    my, mx = up_matrix(x.shape[-2], out_hw[0], align), up_matrix(x.shape[-1], out_hw[1], align)
    return my @ x @ mx.T, np.abs(my) @ np.abs(x) @ np.abs(mx).T


def up_backward(gy, in_hw, align):
    """-> (gx, M): gx = My^T gy Mx and M = |My|^T |gy| |Mx|."""
    gy = np.asarray(gy, dtype=np.float64)
    my, mx = up_matrix(in_hw[0], gy.shape[-2], align), up_matrix(in_hw[1], gy.shape[-1], align)
    return my.T @ gy @ mx, np.abs(my).T @ np.abs(gy) @ np.abs(mx)


def up_taps(n_in, n_out, align):
    """The most non-zero taps (output, i0 or i1) that land on one input index of an axis: the length of the backward kernels'
    fma chain along that axis (a candidate with weight 0 adds exactly nothing)."""
    i0, i1, w0, w1 = up_axis(n_in, n_out, align)
    n = np.zeros(n_in, dtype=np.int64)
    np.add.at(n, i0, (w0 != 0).astype(np.int64))
    np.add.at(n, i1, (w1 != 0).astype(np.int64))
    return int(n.max())


UP_C_FWD = 8                    # per axis: w0 = 1 - w1, two products, one sum


def up_c_bwd(in_hw, out_hw, align):
    """Per axis: the weight (w0 = 1 - w1, and w0 + w1 where both taps land on the last index) and one fma per non-zero tap."""
    return (2 + up_taps(in_hw[1], out_hw[1], align)) + (2 + up_taps(in_hw[0], out_hw[0], align))


# ---- host dispatch ------------------------------------------------------------------------------------------------------
def _covered(n_in, n_out, align, k, smin):
    """upsample.hip:365  `covered = [](const Axis& a, int k, float smin) { return a.scale >= smin || a.n_out <= k; }`"""
    return bool(up_scale(n_in, n_out, align) >= smin) or n_out <= k


THIRD, P4 = F32(1.0) / F32(3.0), F32(0.4)


def up_bwd_route(in_hw, out_hw, align):
    """'sep' | 'gather6' | 'gather8' | 'refused'.  upsample.hip:366-385
         DVD_REQUIRE(covered(ay, 8, 1.0f / 3.0f) && covered(ax, 8, 1.0f / 3.0f), "... factors above 3 are not covered");
         if (covered(ay, 6, 0.4f) && covered(ax, 6, 0.4f) && ax.scale >= 0.4f && (W_out & 3) == 0 && H_out > H_in)  -> sep
         if (covered(ay, 6, 0.4f) && covered(ax, 6, 0.4f)) -> upsample_bilinear_bwd_kernel<6>, else <8>"""
    (H, W), (Ho, Wo) = in_hw, out_hw
    if not (_covered(H, Ho, align, 8, THIRD) and _covered(W, Wo, align, 8, THIRD)):
        return 'refused'
    six = _covered(H, Ho, align, 6, P4) and _covered(W, Wo, align, 6, P4)
    if six and bool(up_scale(W, Wo, align) >= P4) and Wo % 4 == 0 and Ho > H:
        return 'sep'
    return 'gather6' if six else 'gather8'


def up_bwd_segments(H_in):
    """upsample.hip:370  `nseg = (H_in + dvd::kSegRows - 1) / dvd::kSegRows` with kSegRows = 16 (:226)."""
    return (H_in + 15) // 16


def up_fwd_vec(W_out):
    """upsample.hip:67  `const bool vec = (ax.n_out & 3) == 0;`  (one 16-byte store per quad, else scalar stores)"""
    return W_out % 4 == 0


def up_fwd_window(W_in, W_out, align):
    """Per quad of output columns: does the forward read one 4-wide window (True) or gather its eight taps?  upsample.hip:76-79
         int xs = x0[0] < ax.n_in - 4 ? x0[0] : ax.n_in - 4;
         bool window = ax.n_in >= 4 && xs >= 0;
         for (j) window = window && x0[j] >= xs && x1[j] - xs <= 3;      (columns past the row take the last column's taps, :65)"""
    i0, i1, _, _ = up_axis(W_in, W_out, align)
    out = []
    for q in range((W_out + 3) // 4):
        cols = [min(4 * q + j, W_out - 1) for j in range(4)]
        xs = min(int(i0[cols[0]]), W_in - 4)
        out.append(W_in >= 4 and xs >= 0 and all(i0[c] >= xs and i1[c] - xs <= 3 for c in cols))
    return out


# ---- cases ----------------------------------------------------------------------------------------------------------------------
# x2 through conv.upsample_bilinear2x: (N, C, H, W) -> per align_corners (False, True): backward route, and what else the
# shape is there for.  `window`: 'all' / 'none' / 'mixed' over the quads of a row.
UP_X2 = {
    (1, 3, 1, 4): dict(route=('sep', 'sep'), vec=True, segs=1, yscale_align=0.0),                       # vertical scale 0
    (1, 3, 2, 4): dict(route=('sep', 'sep'), vec=True, segs=1, yscale_align=float(THIRD)),              # 1/3, through n_out <= 6
    (1, 3, 3, 6): dict(route=('sep', 'sep'), vec=True, segs=1, yscale_align=float(P4)),                 # exactly 0.4f
    (2, 2, 17, 4): dict(route=('sep', 'sep'), vec=True, segs=2),                 # the second segment is one row; 34 rows per plane
    (1, 2, 33, 42): dict(route=('sep', 'sep'), vec=True, segs=3),
    (1, 2, 5, 2): dict(route=('sep', 'gather6'), vec=True, segs=1, window='none'),
    (1, 2, 2, 1): dict(route=('gather6', 'gather6'), vec=False, window='none'),
    (1, 2, 1, 1): dict(route=('gather6', 'gather6'), vec=False, window='none'),
    (1, 2, 2, 3): dict(route=('gather6', 'gather6'), vec=False, window='none'),
    (3, 1, 3, 5): dict(route=('gather6', 'gather6'), vec=False, window='all'),
}
# other sizes through the C entry points: (planes, (H, W), (Ho, Wo), align) -> route
UP_DIRECT = [
    (3, (4, 6), (12, 18), False, 'gather8'),          # x3, scale == 1.0f / 3.0f
    (3, (4, 6), (10, 15), True, 'gather8'),           # aligned: 3/9 and 5/14
    (3, (4, 6), (10, 15), False, 'gather6'),          # 0.4f on both axes, W_out % 4 != 0
    (2, (2, 2), (8, 8), False, 'gather8'),            # x4, admitted because n_out <= 8
    (2, (2, 2), (8, 8), True, 'gather8'),
    (2, (3, 3), (12, 12), False, 'refused'),
    (2, (3, 3), (12, 12), True, 'refused'),
]
REFUSED_MESSAGE = 'factors above 3'


def up_inputs(planes_shape, out_hw, seed):
    g = torch.Generator().manual_seed(681000 + seed)
    x = torch.randn(*planes_shape, generator=g)
    gy = torch.randn(*(tuple(planes_shape[:-2]) + tuple(out_hw)), generator=g)
    return x, gy


# ============================================================================================================================
# Max-pool 3 / 2 / 1                                                                                          csrc/pool.hip
# ============================================================================================================================
def maxpool_out(n):
    """pool.hip:282  `Ho = (H - 1) / 2 + 1`"""
    return (n - 1) // 2 + 1


def maxpool_forward(x):
    """x [..., H, W] -> (y, pos): the window of output (oy, ox) covers rows 2 oy - 1 .. 2 oy + 1 clipped to the image (padding
    is never looked at), scanned row-major; a later element wins only if it is strictly greater or NaN.  pos = ky * 3 + kx of
    the winner."""
    x = np.asarray(x)
    H, W = x.shape[-2:]
    Ho, Wo = maxpool_out(H), maxpool_out(W)
    lead = x.shape[:-2]
    y = np.zeros(lead + (Ho, Wo), dtype=x.dtype)
    pos = np.zeros(lead + (Ho, Wo), dtype=np.int64)
    with np.errstate(invalid='ignore'):
        for oy in range(Ho):
            for ox in range(Wo):
                best, bi = None, None
                for ky in range(3):
                    for kx in range(3):
                        iy, ix = 2 * oy - 1 + ky, 2 * ox - 1 + kx
                        if not (0 <= iy < H and 0 <= ix < W):
                            continue
                        v = x[..., iy, ix]
                        if best is None:
                            best, bi = v.copy(), np.full(lead, ky * 3 + kx, dtype=np.int64)
                        else:
                            take = (v > best) | np.isnan(v)
                            best = np.where(take, v, best)
                            bi = np.where(take, ky * 3 + kx, bi)
                y[..., oy, ox], pos[..., oy, ox] = best, bi
    return y, pos


def maxpool_backward(gy, pos, in_hw, out_scale=1.0):
    """Every gy goes to its window's winner, times out_scale (float64)."""
    gy = np.asarray(gy, dtype=np.float64)
    H, W = in_hw
    Ho, Wo = gy.shape[-2:]
    gx = np.zeros(gy.shape[:-2] + (H, W))
    flat_g, flat_p, flat_x = gy.reshape(-1, Ho, Wo), pos.reshape(-1, Ho, Wo), gx.reshape(-1, H, W)
    for p in range(flat_g.shape[0]):
        for oy in range(Ho):
            for ox in range(Wo):
                k = int(flat_p[p, oy, ox])
                flat_x[p, 2 * oy - 1 + k // 3, 2 * ox - 1 + k % 3] += flat_g[p, oy, ox]
    return gx * out_scale


def maxpool_flat_index(pos, in_hw):
    """The winner as the flat input index F.max_pool2d(return_indices=True) reports."""
    Ho, Wo = pos.shape[-2:]
    oy, ox = np.meshgrid(np.arange(Ho), np.arange(Wo), indexing='ij')
    return (2 * oy - 1 + pos // 3) * in_hw[1] + (2 * ox - 1 + pos % 3)


MAXPOOL_SIZES = [(1, 1), (1, 2), (2, 1), (3, 1), (5, 7), (6, 4), (12, 18)]
MAXPOOL_PLANES = (2, 5)         # N, C: plane 0 signed noise, the others carry the special windows


def maxpool_inputs(hw):
    """-> (x [2,5,H,W] fp32, gy [2,5,Ho,Wo] of small integers |gy| <= 8).  Planes (n = 0): 0 signed noise; 1 every element below
    zero (every border window's real elements lose against a padding of 0); 2 all -inf; 3 noise with one NaN; 4 a plateau (ties
    everywhere, the first maximum must win).  n = 1: signed noise with ties from a coarse grid, a NaN in plane 3's last element."""
    H, W = hw
    g = torch.Generator().manual_seed(682000 + 100 * H + W)
    x = torch.randn(2, 5, H, W, generator=g)
    x[0, 1] = -0.5 - torch.rand(H, W, generator=g)
    x[0, 2] = float('-inf')
    x[0, 3, H // 2, W // 2] = float('nan')
    x[0, 4] = 1.25
    x[1] = torch.round(2.0 * x[1]) / 2.0
    x[1, 3, H - 1, W - 1] = float('nan')
    gy = torch.randint(-8, 9, (2, 5, maxpool_out(H), maxpool_out(W)), generator=g).float()
    return x, gy


# ============================================================================================================================
# Grouped 3x3 convolution, 8 channels per group                                                              csrc/gconv.hip
# ============================================================================================================================
def gconv_spec(x, w, gy):
    """float64 F.conv2d (padding 1, groups C / 8): y, gx, gw -- and the same three of the absolute values (M_y, M_gx, M_gw)."""
    out = {}
    for tag, f in (('', lambda t: t.double()), ('M_', lambda t: t.double().abs())):
        x64, w64 = f(x).requires_grad_(True), f(w).requires_grad_(True)
        y = F.conv2d(x64, w64, None, 1, 1, 1, x.shape[1] // 8)
        y.backward(f(gy))
        out[tag + 'y'], out[tag + 'gx'], out[tag + 'gw'] = y.detach().numpy(), x64.grad.numpy(), w64.grad.numpy()
    return out


def gconv_fwd_tile(W):
    """gconv.hip:241  `if (W % 84 == 0)` -> the (84, 12) tile, else (64, 16)."""
    return (84, 12) if W % 84 == 0 else (64, 16)


def gconv_wgrad_tile(W):
    """gconv.hip:543  `static inline int wgrad_tile_w(int W) { return W % 56 == 0 ? 56 : 64; }`"""
    return 56 if W % 56 == 0 else 64


def gconv_vec(W):
    """gconv.hip:90 and :300  `(W & 3) == 0`: 16-byte staging, else the scalar staging."""
    return W % 4 == 0


def gconv_fwd_grid(H, W):
    """(tiles per row, tile rows, columns of the last tile, rows of the last tile row): gconv.hip:242 / :246."""
    tw, th = gconv_fwd_tile(W)
    tx, ty = (W + tw - 1) // tw, (H + th - 1) // th
    return tx, ty, W - (tx - 1) * tw, H - (ty - 1) * th


def gconv_wgrad_grid(H, W):
    """(tiles per band, bands): gconv.hip:596  `tx = (W + tw - 1) / tw, bands = (H + dvd::kWT_H - 1) / dvd::kWT_H` (kWT_H = 8)."""
    tw = gconv_wgrad_tile(W)
    return (W + tw - 1) // tw, (H + 7) // 8


GCONV_C_FWD = 72                # 8 source channels x 9 taps, one fma each


def gconv_c_gw(N, H, W):
    """A lane's chain over the W pixels of a row (products with staged zeros add exactly nothing), the 8 rows of a band, the records
    of a residue class mod 4 (gconv_wgrad_reduce_kernel), the classes as (0 + 1) + (2 + 3)."""
    records = N * gconv_wgrad_grid(H, W)[1]
    return W + 7 + max(records // 4 + records % 4 - 1, 0) + 2


# (N, C, H, W) -> forward tile, weight-gradient tile, 16-byte staging, forward grid (tiles per row, tile rows, last columns, last rows)
GCONV_CASES = {
    (2, 16, 13, 84): dict(fwd=(84, 12), wg=64, vec=True, grid=(1, 2, 84, 1)),       # test_42's four: a last tile row of one line
    (1, 8, 17, 67): dict(fwd=(64, 16), wg=64, vec=False, grid=(2, 2, 3, 1)),        # scalar staging, partial tiles on both edges
    (2, 24, 9, 56): dict(fwd=(64, 16), wg=56, vec=True, grid=(1, 1, 56, 9)),
    (1, 16, 8, 168): dict(fwd=(84, 12), wg=56, vec=True, grid=(2, 1, 84, 8)),       # two tiles per row, one band
    (1, 8, 1, 1): dict(fwd=(64, 16), wg=64, vec=False, grid=(1, 1, 1, 1)),
    (1, 16, 3, 5): dict(fwd=(64, 16), wg=64, vec=False, grid=(1, 1, 5, 3)),
    (1, 8, 12, 84): dict(fwd=(84, 12), wg=64, vec=True, grid=(1, 1, 84, 12)),       # exactly one 84 x 12 tile
    (1, 8, 13, 168): dict(fwd=(84, 12), wg=56, vec=True, grid=(2, 2, 84, 1)),       # second tile row of one line, 56-wide wgrad tiles
    (1, 8, 8, 60): dict(fwd=(64, 16), wg=64, vec=True, grid=(1, 1, 60, 8)),         # 16-byte staging with a partial tile
}


def gconv_inputs(shape):
    N, C, H, W = shape
    g = torch.Generator().manual_seed(683000 + 1000 * C + 10 * H + W)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(C, 8, 3, 3, generator=g) * 0.2
    gy = torch.randn(N, C, H, W, generator=g)
    return x, w, gy


# ============================================================================================================================
# The error norm
# ============================================================================================================================
def ratio(got, spec, M, c):
    """max over the elements of |got - spec| / (c * 2^-24 * M); where M == 0 the values must be equal (else inf)."""
    got, spec, M = (np.asarray(a, dtype=np.float64) for a in (got, spec, M))
    assert got.shape == spec.shape == M.shape, (got.shape, spec.shape, M.shape)
    if got.size == 0:
        return 0.0
    err = np.abs(got - spec)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(M > 0, err / (c * U * M), np.where(err == 0, 0.0, np.inf))
    q = np.where(np.isnan(q), np.inf, q)
    return float(q.max())


def rounded_to_half(t):
    """The fp16-valued fp32 tensor the fp16-storage kernels see."""
    return None if t is None else t.half().float()
