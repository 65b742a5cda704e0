"""The kernels that turn gradients into a step, each against a plain float64 (or bit-exact torch) reference: fused Adam
(csrc/elementwise.hip dvd_adam_step_guarded, ops.adam_step, flat.FlatNet), scale_add, mul_mask, acc_reg, depth_tail
(elementwise.hip), unproject_backward (unproject.hip) and amax (amax.hip).

The element counts are the ones where these kernels go wrong: n < 4, the scalar tail (n % 4 = 1, 2, 3), the grid-stride loop
(more than 2048 blocks x 256 threads x 4 elements) and views that start 4 bytes into a 16-byte line.  Every tolerance is
about 2.5-4x the worst value measured on MI355X, logged through helpers.log_measured next to its bound."""
import copy
import math
import multiprocessing as mp

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
BIG = 2_100_003                  # > 2048 * 256 * 4: every block of the grid-stride loop takes a second turn; n % 4 = 3
SIZES = [1, 2, 3, 4, 5, 6, 7, 1029, BIG]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits_or_both_nan(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(_bits(a[~na]), _bits(b[~nb]))


def _offset_view(n, off, device='cuda'):
    """n floats that start `off` floats after a 256-byte aligned allocation."""
    buf = torch.zeros(n + off + 4, device=device)
    return buf[off:off + n]


# ---------------------------------------------------------------------------------------------------------------------
# Adam


def _grad(n, k, seed, scale=1.0):
    """Fresh fp32 gradient of step k: magnitudes log-uniform over 1e-6 .. 1e2 with random signs, ~5% exact zeros (and every
    97th element zero at every step: its moments stay 0), ~7% around 1e-8 (sqrt(v) next to eps)."""
    g = torch.Generator().manual_seed(seed * 7919 + k)
    mag = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 8.0 - 6.0)
    sel = torch.rand(n, generator=g, dtype=torch.float64)
    mag = torch.where((sel >= 0.05) & (sel < 0.12), 1e-8 * (0.3 + 3.0 * torch.rand(n, generator=g, dtype=torch.float64)), mag)
    x = torch.where(torch.rand(n, generator=g) < 0.5, -mag, mag) * scale
    x[sel < 0.05] = 0.0
    x[::97] = 0.0
    return x.float()


def _adam64(p0, grads, lr, b1, b2, eps=1e-8, variant=None):
    """Float64 Adam written out, for the deliberately wrong variants the bound has to reject.  'bias_prev' takes the bias
    correction of step k - 1 from step 2 on (at step 1 it would divide by 0: caught by any bound)."""
    p, m, v, out = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), []
    for k, g in enumerate(grads, 1):
        if variant != 'no_update':
            m = b1 * m + (1 - b1) * g
            v = b2 * v + (1 - b2) * g * g
            kk = max(k - 1, 1) if variant == 'bias_prev' else k
            bc1, bc2 = 1 - b1 ** kk, 1 - b2 ** kk
            if variant == 'sqrt_v_eps':
                den = torch.sqrt(v / bc2 + eps)
            else:
                den = torch.sqrt(v) / math.sqrt(bc2) + eps
            p = p - (lr / bc1) * m / den
        out.append(p.clone())
    return out


def _p_err(p, rp, k, lr):
    """|p - p64| in units of lr, less the storage rounding of p itself (at most half an ulp, 2^-24 |p|, per step): what is
    left is the error of the k updates."""
    p = p.double().cpu()
    return float((((p - rp).abs() - k * 2.0 ** -24 * rp.abs()).clamp_min(0.0) / lr).max())


def _errs(p, m, v, rp, rm, rv, mabs, lr, k):
    """(p error in units of lr (_p_err), |m - m64| / m_abs, |v - v64| / v_abs), maxima over the elements.  m_abs, v_abs: the
    float64 moments of |g1 s| + |g2| and its square, the scale of the moments' rounding errors (s g1 + g2 may cancel to ~0,
    and m with it).  A moment that must be exactly 0 and is not gives an error of ~1e300."""
    ep = _p_err(p, rp, k, lr)
    em = float(((m.double().cpu() - rm).abs() / mabs[0].clamp_min(1e-300)).max())
    ev = float(((v.double().cpu() - rv).abs() / mabs[1].clamp_min(1e-300)).max())
    return ep, em, ev


def _abs_moments(mabs, ga, b1, b2):
    return (b1 * mabs[0] + (1 - b1) * ga, b2 * mabs[1] + (1 - b2) * ga * ga)


# float64 Adam against the kernel over 20 steps.  Worst measured on MI355X over sizes, betas, lr and the gradient combinations
# (bit for bit what a CPU emulation of the kernel's fp32 arithmetic gives): |dp| / lr 1.75e-4 (s g1 + g2 rounded in fp32 where
# it cancels and sqrt(v) is small), |dm| / m_abs 8.0e-7, |dv| / v_abs 1.36e-5 (the float betas of the C ABI:
# 1 - 0.999f = 0.99998713e-3).  The wrong variants land at 0.38 (bias correction of step k - 1) .. 24 (grad2 dropped) in p.
ADAM_P, ADAM_M, ADAM_V = 6e-4, 3e-6, 5e-5

ADAM_CASES = [  # betas, lr, scale, *scale_ptr, grad2
    ((0.5, 0.9), 1e-4, 0.5, 1.0 / 3.0, True),
    ((0.5, 0.9), 1e-3, 0.5, None, True),
    ((0.9, 0.999), 1e-4, 1.0, 1.0 / 3.0, False),
    ((0.9, 0.999), 1e-3, 1.0, None, False),
]


def _adam_kernel_run(p0, g1s, g2s, case, skips=None):
    from dvd_hip import ops
    (b1, b2), lr, scale, sp, _ = case
    sp_t = torch.tensor([sp], device='cuda') if sp is not None else None
    p = p0.clone().cuda()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    skip = torch.zeros(2, device='cuda') if skips is not None else None
    out = []
    for k in range(len(g1s)):
        if skips is not None:
            skip.copy_(torch.tensor(skips[k], dtype=torch.float32))
        ops.adam_step(p, g1s[k].cuda(), m, v, k + 1, lr, b1, b2, 1e-8, scale=scale, scale_ptr=sp_t,
                      grad2=None if g2s is None else g2s[k].cuda(), skip_ptr=skip)
        out.append((p.cpu(), m.cpu(), v.cpu()))
    return out


def _effective(g1, g2, scale, sp):
    s = scale * (float(torch.tensor(sp, dtype=torch.float32)) if sp is not None else 1.0)   # (0.5 * fp32(1/3): exact in fp32)
    ge = s * g1.double()
    ga = (s * g1.double()).abs()
    if g2 is not None:
        ge = ge + g2.double()
        ga = ga + g2.double().abs()
    return ge, ga


@pytest.mark.parametrize('n', [1, 2, 3, 6, 4099, BIG])
@pytest.mark.parametrize('case', ADAM_CASES, ids=['b0.5-lr1e-4-s0.5x1/3-g2', 'b0.5-lr1e-3-s0.5-g2', 'b0.9-lr1e-4-sx1/3',
                                                  'b0.9-lr1e-3'])
def test_adam_matches_float64_adam_over_20_steps(n, case):
    """dvd_adam_step_guarded (no skip pointer) against torch.optim.Adam(foreach=False) on float64 copies fed the same
    gradients, after every one of K = 20 steps: param, exp_avg, exp_avg_sq.  Bounds (ADAM_*) about 3.5x the worst measured on
    MI355X.  On the same data the bound must reject, on the CPU: no update, bias correction of step k - 1, sqrt(v + eps) for
    sqrt(v) + eps, and grad2 dropped.  Two runs give the same bits."""
    (b1, b2), lr, scale, sp, with_g2 = case
    K, seed = 20, n + int(1e4 * lr) + int(10 * b1)
    p0 = (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 0.1).float()
    g1s = [_grad(n, k, seed) for k in range(K)]
    g2s = [_grad(n, k, seed + 1, 0.5) for k in range(K)] if with_g2 else None
    runs = [_adam_kernel_run(p0, g1s, g2s, case) for _ in range(2)]
    got = runs[0]
    for a, b in zip(runs[0][-1], runs[1][-1]):
        assert torch.equal(_bits(a), _bits(b)), 'two identical Adam runs differ'

    ref = p0.double().clone().requires_grad_(False)
    opt = torch.optim.Adam([ref], lr=lr, betas=(b1, b2), eps=1e-8, foreach=False)
    mabs = (torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64))
    geffs, worst = [], [0.0, 0.0, 0.0]
    for k in range(K):
        ge, ga = _effective(g1s[k], None if g2s is None else g2s[k], scale, sp)
        geffs.append(ge)
        ref.grad = ge.clone()
        opt.step()
        mabs = _abs_moments(mabs, ga, b1, b2)
        st = opt.state[ref]
        e = _errs(*got[k], ref.detach(), st['exp_avg'], st['exp_avg_sq'], mabs, lr, k + 1)
        worst = [max(w, x) for w, x in zip(worst, e)]
        assert e[0] <= ADAM_P and e[1] <= ADAM_M and e[2] <= ADAM_V, 'step %d: %s' % (k + 1, e)
    name = 'test_15_adam_%s_n%d' % ('_'.join(str(x) for x in case[:2]), n)
    for what, w, bound in zip(('p_over_lr', 'm_rel', 'v_rel'), worst, (ADAM_P, ADAM_M, ADAM_V)):
        helpers.log_measured('%s_%s' % (name, what), w, bound)

    if n < 1000:
        return
    # the bound discriminates: each wrong Adam, in float64 on the same data, lands outside it
    refs = _adam64(p0.double(), geffs, lr, b1, b2)
    assert max(_p_err(b, a, k, lr) for k, (a, (b, _, _)) in enumerate(zip(refs, got), 1)) <= ADAM_P   # (the written-out form)
    variants = {'no_update': geffs, 'bias_prev': geffs, 'sqrt_v_eps': geffs}
    if with_g2:
        variants['grad2_dropped'] = [_effective(g, None, scale, sp)[0] for g in g1s]
    for var, gs in variants.items():
        wrong = _adam64(p0.double(), gs, lr, b1, b2, variant=None if var == 'grad2_dropped' else var)
        e = max(_p_err(a, b, k, lr) for k, (a, b) in enumerate(zip(wrong, refs), 1))
        helpers.log_measured('%s_mutant_%s_p_over_lr' % (name, var), e, ADAM_P)
        assert e > ADAM_P, '%s is inside the Adam bound (%g <= %g)' % (var, e, ADAM_P)


@pytest.mark.parametrize('n', [3, 4099, BIG])
def test_guarded_adam_skips_bitwise_and_corrects_at_the_effective_step(n):
    """Sequence run, run, skip, run, run with the (flag, count) pair of the loss-scale state: at the skipped step p, m and v
    keep their bits; afterwards the kernel (step k, count 1) equals float64 Adam at step k - 1 -- within the bounds of the
    unguarded test."""
    case = ((0.5, 0.9), 1e-4, 1.0, None, False)
    seed = n + 17
    p0 = (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 0.1).float()
    g1s = [_grad(n, k, seed) for k in range(5)]
    skips = [(0, 0), (0, 0), (1, 1), (0, 1), (0, 1)]
    got = _adam_kernel_run(p0, g1s, None, case, skips=skips)
    ref = p0.double().clone()
    opt = torch.optim.Adam([ref], lr=1e-4, betas=(0.5, 0.9), eps=1e-8, foreach=False)
    mabs, worst = (torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)), [0.0, 0.0, 0.0]
    for k in range(5):
        if skips[k][0]:
            for a, b in zip(got[k], got[k - 1]):
                assert torch.equal(_bits(a), _bits(b)), 'a skipped step changed the state'
            continue
        ref.grad = g1s[k].double()
        opt.step()
        mabs = _abs_moments(mabs, g1s[k].double().abs(), 0.5, 0.9)
        st = opt.state[ref]
        e = _errs(*got[k], ref.detach(), st['exp_avg'], st['exp_avg_sq'], mabs, 1e-4, k + 1 - skips[k][1])
        worst = [max(w, x) for w, x in zip(worst, e)]
        assert e[0] <= ADAM_P and e[1] <= ADAM_M and e[2] <= ADAM_V, 'step %d: %s' % (k + 1, e)
    helpers.log_measured('test_15_guarded_adam_n%d_p_over_lr' % n, worst[0], ADAM_P)


# ---------------------------------------------------------------------------------------------------------------------
# FlatNet


class _Ragged(torch.nn.Module):
    """Parameter sizes that are not multiples of 4 (15, 3, 189, 7, 1) and, with `big`, ~100k elements: enough for 7 real
    buckets of parallel.bucket_bounds."""

    def __init__(self, big=False):
        super().__init__()
        self.lin = torch.nn.Linear(5, 3)
        self.conv = torch.nn.Conv2d(3, 7, 3)
        self.one = torch.nn.Parameter(torch.randn(1))
        if big:
            self.big = torch.nn.Linear(317, 313)


def _flat_grads(fn, k, seed):
    for i, p in enumerate(fn.params):
        fn.view(fn.grad, i).copy_(_grad(p.numel(), k, seed + 31 * i).view_as(p))


def _flat_vs_float64(fn, ref_params, opt, k, mabs):
    worst = [0.0, 0.0, 0.0]
    for i, rp in enumerate(ref_params):
        st = opt.state[rp]
        e = _errs(fn.view(fn.flat, i), fn.view(fn.exp_avg, i), fn.view(fn.exp_avg_sq, i), rp.detach(), st['exp_avg'],
                  st['exp_avg_sq'], mabs[i], fn.lr, k + 1)
        worst = [max(w, x) for w, x in zip(worst, e)]
    return worst


def _run_flat_against_float64(fn, steps, seed, step_fn):
    ref_params = [p.detach().double().cpu().clone() for p in fn.params]
    opt = torch.optim.Adam(ref_params, lr=fn.lr, betas=fn.betas, eps=fn.eps, foreach=False)
    mabs = [(torch.zeros(p.shape, dtype=torch.float64), torch.zeros(p.shape, dtype=torch.float64)) for p in ref_params]
    worst = [0.0, 0.0, 0.0]
    for k in range(steps):
        _flat_grads(fn, k, seed)
        step_fn()
        for i, rp in enumerate(ref_params):
            rp.grad = fn.view(fn.grad, i).double().cpu()
            mabs[i] = _abs_moments(mabs[i], rp.grad.abs(), *fn.betas)
        opt.step()
        e = _flat_vs_float64(fn, ref_params, opt, k, mabs)
        worst = [max(w, x) for w, x in zip(worst, e)]
        assert e[0] <= ADAM_P and e[1] <= ADAM_M and e[2] <= ADAM_V, 'step %d: %s' % (k + 1, e)
    return worst


def _padding(fn):
    used = torch.zeros(fn.numel, dtype=torch.bool)
    for p, o in zip(fn.params, fn.offsets):
        used[o:o + p.numel()] = True
    return ~used


def test_flatnet_adam_matches_float64_adam_and_keeps_padding_zero():
    """FlatNet.adam_step over 10 steps on Linear(5, 3) + Conv2d(3, 7, 3) + a 1-element parameter (segments padded to 16
    bytes) against torch.optim.Adam(foreach=False) on float64 copies; the padding between segments stays 0 in all four
    buffers."""
    from dvd_hip import flat
    torch.manual_seed(0)
    fn = flat.FlatNet(_Ragged().cuda(), 1e-3, (0.5, 0.9))
    pad = _padding(fn)
    assert int(pad.sum()) > 0
    worst = _run_flat_against_float64(fn, 10, 5, fn.adam_step)
    helpers.log_measured('test_15_flatnet_p_over_lr', worst[0], ADAM_P)
    for buf in (fn.flat, fn.grad, fn.exp_avg, fn.exp_avg_sq):
        assert torch.equal(buf.cpu()[pad], torch.zeros(int(pad.sum())))


def test_flatnet_warm_steps_take_bias_correction_at_the_effective_step():
    """A net that counts skipped steps (FlatNet.skip_count, a view of the loss-scale state) and a step that passes no skip
    pointer -- what the warm steps call: Adam runs at step_count - skipped, as state_dict() reports.
    Two steps were skipped before; three more against float64 Adam from step 1.  No host read is added."""
    from dvd_hip import flat
    torch.manual_seed(1)
    fn = flat.FlatNet(_Ragged().cuda(), 1e-3, (0.5, 0.9))
    st = torch.zeros(16, device='cuda')
    st[5] = 2.0
    fn.skip_count = st[5:6]
    fn.step_count = 2
    worst = _run_flat_against_float64(fn, 3, 9, fn.adam_step)
    helpers.log_measured('test_15_flatnet_warm_skip_p_over_lr', worst[0], ADAM_P)
    assert float(fn.state_dict()['state'][0]['step']) == 3.0 and fn.step_count == 5
    assert st.tolist() == [0.0] * 5 + [2.0] + [0.0] * 10          # the loss-scale state is read, never written


def _bucket_child(q):
    try:
        from dvd_hip import flat, parallel
        parallel.init_one_rank('nccl')
        assert parallel.is_distributed() and parallel.world_size() == 1
        torch.manual_seed(2)
        base = _Ragged(big=True)
        out = {}
        for nb in (1, 3, 4, 7):
            for warm in (False, True):
                a = flat.FlatNet(copy.deepcopy(base).cuda(), 1e-3, (0.5, 0.9))
                b = flat.FlatNet(copy.deepcopy(base).cuda(), 1e-3, (0.5, 0.9))
                if warm:                 # skip count 2, no skip pointer (warm steps): both paths take the effective step
                    for fn in (a, b):
                        fn.skip_count = torch.full((1,), 2.0, device='cuda')
                        fn.step_count = 2
                p_init = a.flat.clone()
                for k in range(3):
                    _flat_grads(a, k, 40 + nb)
                    _flat_grads(b, k, 40 + nb)
                    a.adam_step()
                    b.all_reduce_and_adam_step(nb)
                torch.cuda.synchronize()
                same = all(torch.equal(_bits(x), _bits(y)) for x, y in ((a.flat, b.flat), (a.grad, b.grad),
                                                                        (a.exp_avg, b.exp_avg), (a.exp_avg_sq, b.exp_avg_sq)))
                moved = not torch.equal(a.flat, p_init)
                out[(nb, warm)] = (same, moved, len(parallel.bucket_bounds(b.numel, nb)), a.step_count)
        parallel.shutdown()
        q.put(out)
    except BaseException as e:     # noqa: BLE001 -- hand the failure to the parent instead of a silent exit code
        import traceback
        q.put({'error': '%s\n%s' % (e, traceback.format_exc())})


@pytest.mark.timeout(600)
def test_flatnet_bucketed_all_reduce_adam_equals_adam_step_bitwise():
    """FlatNet.all_reduce_and_adam_step(n_buckets) for n_buckets 1, 3, 4, 7 -- under a ONE-rank RCCL group with
    parallel.force_distributed (the pattern of test_33), so the bucketed path really runs -- is bit-identical to adam_step over
    3 steps: a bucket updated twice or skipped, or bias correction taken at another step, changes bits.  With a skip count
    and no skip pointer (warm steps) as well."""
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    p = ctx.Process(target=_bucket_child, args=(q,))
    p.start()
    out = q.get(timeout=500)
    p.join(60)
    assert 'error' not in out, out.get('error')
    for (nb, warm), (same, moved, real, steps) in out.items():
        assert real == nb, 'only %d buckets for n_buckets=%d: the module is too small' % (real, nb)
        assert moved and steps == (5 if warm else 3)
        assert same, 'bucketed Adam (n_buckets=%d, warm=%s) differs from adam_step' % (nb, warm)


# ---------------------------------------------------------------------------------------------------------------------
# elementwise helpers


def _wide(n, seed, device='cuda'):
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (torch.rand(n, generator=g) * 12.0 - 6.0)
    return torch.where(torch.rand(n, generator=g) < 0.5, -mag, mag).float().to(device)


SCALE_ADD_ULP = 1.0      # in units of 2^-23 (|s a| + |b|): one rounding each for s a and + b; measured worst 0.91


@pytest.mark.parametrize('n', SIZES)
def test_scale_add_against_float64(n):
    """out = scale * (*scale_ptr) * a + b against float64, within 2^-23 (|s a| + |b|) elementwise: with and without b and
    scale_ptr, out separate, aliasing a and aliasing b."""
    from dvd_hip import ops
    a0, b0 = _wide(n, n), _wide(n, n + 1)
    sp = torch.tensor([1.0 / 3.0], device='cuda')
    worst = 0.0
    for use_b in (True, False):
        for use_sp in (True, False):
            s64 = 0.5 * (float(sp) if use_sp else 1.0)
            ref = s64 * a0.double().cpu() + (b0.double().cpu() if use_b else 0.0)
            mag = (s64 * a0.double().cpu()).abs() + (b0.double().cpu().abs() if use_b else 0.0)
            for alias in ('none', 'a', 'b') if use_b else ('none', 'a'):
                a, b = a0.clone(), b0.clone()
                out = a if alias == 'a' else (b if alias == 'b' else torch.full_like(a, float('nan')))
                r = ops.scale_add(out, a, 0.5, sp if use_sp else None, b if use_b else None)
                assert r is out
                e = float(((out.double().cpu() - ref).abs() / (EPS32 * mag).clamp_min(1e-300)).max())
                worst = max(worst, e)
                assert e <= SCALE_ADD_ULP, (use_b, use_sp, alias, e)
                if alias != 'a':
                    assert torch.equal(_bits(a), _bits(a0))
                if use_b and alias != 'b':
                    assert torch.equal(_bits(b), _bits(b0))
    helpers.log_measured('test_15_scale_add_n%d_ulps' % n, worst, SCALE_ADD_ULP)


def test_16_byte_kernels_refuse_a_view_4_bytes_into_a_line():
    """scale_add, Adam, acc_reg and depth_tail read 16 bytes at a time: a view that starts 4 bytes into a line is refused with
    an error, never read from the wrong address."""
    from dvd_hip import conv, ops
    n = 37
    x, y = _offset_view(n, 1), _offset_view(n, 0)
    with pytest.raises(RuntimeError, match='aligned'):
        ops.scale_add(y, x, 2.0)
    with pytest.raises(RuntimeError, match='aligned'):
        ops.adam_step(x, y, y.clone(), y.clone(), 1, 1e-3, 0.5, 0.9)
    with pytest.raises(RuntimeError, match='aligned'):
        ops.acc_reg(x, y, 1.0, y.clone(), torch.zeros(1, device='cuda'))
    with pytest.raises(RuntimeError, match='aligned'):
        conv.depth_tail(x)


@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (2, 3, 1, 1), (3, 1, 5, 7), (2, 3, 17, 13), (5, 3, 1, 9), (2, 3, 331, 447)])
@pytest.mark.parametrize('inplace', [False, True])
@pytest.mark.parametrize('off', [0, 1])
def test_mul_mask_bitwise(shape, inplace, off):
    """out[b, c] = a[b, c] * mask[b] bit for bit against torch: B, C and HW ragged (HW = 1, C = 1), more elements than one
    pass of the grid (2 x 3 x 331 x 447), in place as the model calls it on the gradient, views 4 bytes into a line."""
    from dvd_hip import ops
    B, C, H, W = shape
    n = B * C * H * W
    a = _offset_view(n, off).view(B, C, H, W)
    a.copy_(_wide(n, n).view(B, C, H, W))
    m = _offset_view(B * H * W, 3 - 2 * off).view(B, 1, H, W)
    g = torch.Generator().manual_seed(n)
    m.copy_(torch.where(torch.rand(B, 1, H, W, generator=g) < 0.3, 0.0, torch.rand(B, 1, H, W, generator=g) * 2).cuda())
    ref = a.cpu() * m.cpu()
    out = a if inplace else torch.empty_like(a)
    r = ops.mul_mask(out, a, m)
    assert r is out
    assert torch.equal(_bits(out), _bits(ref))


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('accumulate', [0, 1])
def test_acc_reg_sign_bitwise_and_sum_against_float64(n, accumulate):
    """g = coef * sign(sf1 - sf0) bit for bit (d = 0 gives 0; ~1/8 of the elements), and sum |sf1 - sf0| against float64, into
    a non-zero abs_sum with accumulate 0 and 1; BIG uses all 2048 partials.  Bound: 2e-7 of the sum (fp32 sums per thread and
    wave, float64 over the partials; measured worst 4.9e-8)."""
    from dvd_hip import ops
    sf0 = _wide(n, 3 * n) * 1e-3
    sf1 = sf0 + _wide(n, 3 * n + 1) * 1e-3
    eq = torch.rand(n, generator=torch.Generator().manual_seed(n)) < 0.125
    sf1[eq.cuda()] = sf0[eq.cuda()]
    coef = 0.37
    g1 = torch.full_like(sf0, float('nan'))
    abs_sum = torch.tensor([1234.5], device='cuda')
    ops.acc_reg(sf0, sf1, coef, g1, abs_sum, accumulate=bool(accumulate))
    d = sf1.cpu() - sf0.cpu()
    assert torch.equal(g1.cpu(), coef * torch.sign(d)) and bool((g1.cpu()[d == 0] == 0).all())
    ref = (sf1.double().cpu() - sf0.double().cpu()).abs().sum().item() + (1234.5 if accumulate else 0.0)
    e = abs(float(abs_sum) - ref) / ref
    helpers.log_measured('test_15_acc_reg_n%d_acc%d_rel' % (n, accumulate), e, 2e-7)
    assert e <= 2e-7


UNPROJECT_ULP = 6.0      # |g - g64| / (2^-24 (|scale| (|gP| |R|^T) . (|xy1| |K_inv|) + |out0|)); measured worst 1.6


@pytest.mark.parametrize('B,H,W', [(1, 1, 1), (2, 7, 9), (1, 5, 13), (3, 12, 16), (2, 33, 47)])
@pytest.mark.parametrize('planar', [True, False])
@pytest.mark.parametrize('mode', ['plain', 'scale_accumulate', 'offset_out'])
def test_unproject_backward_against_float64_autograd(B, H, W, planar, mode):
    """g_depth (+)= scale * ((g_P @ R^T) . ray) against float64 autograd of oracle/geometry.py::unproject: planar [B,3,H,W] and
    [B,H,W,3] point gradients, odd H and W (one pixel per thread) and W % 4 == 0 (four), a scale pointer with accumulate=True
    into a non-zero output, and an output view 4 bytes into a line (falls back to one pixel per thread)."""
    from dvd_hip import ops, synthetic
    from oracle import geometry as G
    cams = synthetic.make_batch(B, H, W, with_images=False, seed=B * 100 + H)
    R, Kinv, t = cams['R_1'], cams['K_inv'], cams['t_1']
    g = torch.Generator().manual_seed(H * W)
    gP = torch.randn((B, 3, H, W) if planar else (B, H, W, 3), generator=g)
    depth = (1.0 + 4.0 * torch.rand(B, 1, H, W, generator=g)).double().requires_grad_(True)
    grid = G.pixel_grid(H, W).double()
    P = G.unproject(depth, R.double(), t.double(), Kinv.double(), grid=grid)
    gP5 = (gP.permute(0, 2, 3, 1) if planar else gP).reshape(B, H, W, 1, 3).double()
    P.backward(gP5)
    ray = torch.matmul(grid.abs(), Kinv.double().abs())          # |x| |K_inv|: the scale of the ray's own rounding
    mag = (torch.matmul(gP5.abs(), R.double().abs().transpose(-1, -2)) * ray).sum(-1).view(B, 1, H, W)
    scale, out0 = 1.0, torch.zeros(B, 1, H, W)
    kw = {}
    if mode == 'scale_accumulate':
        scale, out0 = 0.37, torch.randn(B, 1, H, W, generator=g) * 5
        kw = dict(scale=torch.tensor([0.37], device='cuda'), accumulate=True)
    out = _offset_view(B * H * W, 1 if mode == 'offset_out' else 0).view(B, 1, H, W)
    out.copy_(out0.cuda())
    r = ops.unproject_backward(gP.cuda(), planar, R.cuda(), Kinv.cuda(), out=out, **kw)
    assert r.data_ptr() == out.data_ptr()
    sc = float(torch.tensor(scale, dtype=torch.float32))
    ref = sc * depth.grad + out0.double()
    e = float(((out.double().cpu() - ref).abs() / (2.0 ** -24 * (sc * mag + out0.double().abs())).clamp_min(1e-300)).max())
    helpers.log_measured('test_15_unproject_bwd_%dx%dx%d_%s_%s_ulps' % (B, H, W, planar, mode), e, UNPROJECT_ULP)
    assert e <= UNPROJECT_ULP


def _amax_into(x, out):
    from dvd_hip import _lib, ops
    import ctypes
    _lib.check(_lib.load().dvd_amax(ops._p(x), ctypes.c_longlong(x.numel()), ops._p(out), ops._stream()), 'dvd_amax')
    return out


@pytest.mark.parametrize('off', [0, 1, 2, 3])
def test_amax_exact_at_every_alignment_and_non_finite(off):
    """max|x| exactly, for views 0-3 floats into an aligned buffer, n = 1..9 with the maximum at every position, and n = 1029
    and BIG with the maximum at the head, the tail and the middle; NaN anywhere or +-Inf gives +Inf; a preset larger value in
    `out` (a running bound) is kept, a smaller one raised."""
    from dvd_hip import ops
    cases = [(n, pos) for n in range(1, 10) for pos in range(n)] + [(n, pos) for n in (1029, BIG) for pos in (0, 1, 2, n // 2, n - 1)]
    for n, pos in cases:
        x = _offset_view(n, off)
        x.copy_(torch.rand(n, generator=torch.Generator().manual_seed(n + pos)).cuda() * 2 - 1)
        x[pos] = -3.5
        assert float(ops.amax(x)) == 3.5, (n, pos)
        assert float(_amax_into(x, torch.tensor([7.25], device='cuda'))) == 7.25
        assert float(_amax_into(x, torch.tensor([1.0], device='cuda'))) == 3.5
        for bad in (float('nan'), float('inf'), float('-inf')):
            if n > 9 and pos not in (0, n - 1):
                continue
            y = x.clone() if off == 0 else _offset_view(n, off).copy_(x)
            y[pos] = bad
            assert float(ops.amax(y)) == float('inf'), (n, pos, bad)


# ---------------------------------------------------------------------------------------------------------------------
# depth tail


def _tail_values():
    f = np.float32
    v = [np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-2, 1e-40, -1e-40, 1e-45, 1.1754944e-38, 1.0, 5.0, -1.0, 1e30, 3.4e38]
    up = dn = f(1e-2)
    for _ in range(4):                                  # neighbours of the clamp's bound
        up, dn = np.nextafter(up, f(1)), np.nextafter(dn, f(0))
        v += [up, dn]
    rnd = torch.randn(997, generator=torch.Generator().manual_seed(5)) * 0.05
    return torch.cat([torch.tensor(np.array(v, dtype=np.float32)), rnd])


def test_depth_tail_non_finite_forward_and_backward_match_torch_bitwise():
    """10000 / clamp(relu(v), min=1e-2) bit for bit against CPU torch, NaN for NaN, for NaN, +-Inf, +-0, 1e-2 and its
    neighbours, denormals (fmaxf made a NaN depth 1e6); the backward against CPU autograd bit for bit,
    with an output gradient of 1 (NaN -> 0, +Inf -> -0, -Inf / +-0 / 1e-40 -> 0, 1e-2 -> -1e8) and a random one.  Element
    counts 1 .. 7 and the whole list (n % 4 = 1)."""
    from dvd_hip import conv
    vals = _tail_values()
    go_r = torch.randn(vals.shape, generator=torch.Generator().manual_seed(6))
    for n in list(range(1, 8)) + [vals.numel()]:
        for lo in (0, 1, 2) if n < 8 else (0,):
            v = vals[lo:lo + n].clone()
            for go in (torch.ones(n), go_r[lo:lo + n].clone()):
                a = v.cuda().requires_grad_(True)
                b = v.clone().requires_grad_(True)
                out = conv.depth_tail(a)
                ref = 10000 / torch.clamp(F.relu(b), min=1e-2)
                assert _same_bits_or_both_nan(out, ref), (n, lo, out, ref)
                out.backward(go.cuda())
                ref.backward(go)
                assert _same_bits_or_both_nan(a.grad, b.grad), (n, lo, a.grad, b.grad)
    a = torch.tensor([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, 1e-2], device='cuda').requires_grad_(True)
    d = conv.depth_tail(a)
    d.backward(torch.ones_like(d))
    assert torch.isnan(d[0]) and d[1:].tolist() == [0.0, 1e6, 1e6, 1e6, 1e6, 1e6]
    assert _bits(a.grad).tolist() == _bits(torch.tensor([0.0, -0.0, 0.0, 0.0, 0.0, 0.0, -1e8])).tolist()


@pytest.mark.timeout(600)
def test_nan_in_the_fp32_midas_head_reaches_the_depth_map():
    """End to end: the fp32 MidasNet forward (the fused head: conv.head1x1 + conv.depth_tail) with a NaN planted in the input
    of the depth tail -- the 1x1 head's bias, as a diverged step leaves it -- gives a NaN depth map, as the reference's
    `10000 / clamp(output_conv(y), 1e-2)` does; before, every pixel read 1e6."""
    from dvd_hip.third_party.MiDaS import MidasNet, calibrate_head_for_random_init
    torch.manual_seed(0)
    net = calibrate_head_for_random_init(MidasNet(non_negative=True, normalize_input=True)).cuda().eval()
    x = torch.rand(1, 3, 64, 96, device='cuda')
    with torch.no_grad():
        d0 = net(x)
        assert bool(torch.isfinite(d0).all())
        net.scratch.output_conv[4].bias.fill_(float('nan'))
        d1 = net(x)
    assert d1.shape == d0.shape and bool(torch.isnan(d1).all())
