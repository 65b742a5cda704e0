"""Fused SGD (`--optim sgd`: csrc/elementwise.hip sgd_kernel, dvd_sgd_step_guarded, ops.sgd_step, flat.FlatNet.sgd) against
float64 torch.optim.SGD(foreach=False), its skip pair, the bucketed all-reduce path and its HBM footprint.

The kernel's bound is DERIVED, not measured.  Every fp32 operation rounds its result by at most u = 2^-24 of its magnitude,
and that magnitude is at most the sum of the absolute values of its terms.  So, per element and step, with the float64
reference's values and E_* the accumulated error of each fp32 quantity:
  g = s g1 + g2          s = sa * (*sa_ptr), s g1, + g2: 3 roundings         E_g = 3u A_g,   A_g = |s g1| + |g2|
  d = g + wd p           wd to fp32, wd p, + : 3                             E_d = E_g + wd E_p + 3u A_d,   A_d = A_g + wd |p|
  buf = d (first step), else (buf m) + (1 - dampening) d:
                         m and 1 - dampening to fp32, two products, + : 5 (on terms of size m B and (1 - dampening) A_d)
                                                                             E_b = m E_b + (1 - dampening) E_d + 3u B',
                                                                             B' = m B + (1 - dampening) A_d
  p = p - lr upd         lr to fp32, lr upd, - : 3                           E_p = E_p + lr E_upd + 3u (|p| + lr U)
(upd = buf, U = B with momentum; upd = d, U = A_d without).  A fused multiply-add rounds once where two operations would
round twice, so contraction stays inside the bound.  The second-order terms (u^2 and smaller) and the float64 reference's own
rounding (2^-53 per operation) are covered by a factor 1.01.  The test asserts |p - p64| <= E_p and |buf - buf64| <= E_b
element by element after every step; on the CPU it shows that the bound rejects dampening applied at the first step, a
dropped weight decay, a dropped grad2 and a step that uses the previous step's buffer."""
import copy
import multiprocessing as mp

import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SLACK = 1.01
BIG = 2_100_003                  # > 2048 * 256 * 4: every block of the grid-stride loop takes a second turn; n % 4 = 3


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _grad(n, k, seed, scale=1.0):
    """Fresh fp32 gradient of step k: magnitudes log-uniform over 1e-6 .. 1e1, random signs, ~5% zeros and every 97th element
    zero at every step (there only the weight decay moves p)."""
    g = torch.Generator().manual_seed(seed * 7919 + k)
    mag = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 7.0 - 6.0)
    x = torch.where(torch.rand(n, generator=g) < 0.5, -mag, mag) * scale
    x[torch.rand(n, generator=g) < 0.05] = 0.0
    x[::97] = 0.0
    return x.float()


def _effective(g1, g2, scale, sp):
    """(s g1 + g2 in float64, |s g1| + |g2|) with the kernel's s = scale * fp32(*scale_ptr) (exact in fp32 for these cases)."""
    s = scale * (float(torch.tensor(sp, dtype=torch.float32)) if sp is not None else 1.0)
    ge, ga = s * g1.double(), (s * g1.double()).abs()
    if g2 is not None:
        ge, ga = ge + g2.double(), ga + g2.double().abs()
    return ge, ga


class _Bound(object):
    """The error recurrence of the module docstring, fed the float64 reference's values step by step."""

    def __init__(self, n, lr, momentum, dampening, wd):
        self.lr, self.m, self.omd, self.wd = lr, momentum, 1.0 - dampening, wd
        z = torch.zeros(n, dtype=torch.float64)
        self.Ep, self.Eb, self.B, self.first = z.clone(), z.clone(), z.clone(), True

    def step(self, ga, p_prev):
        pa = p_prev.abs()
        Ed, Ad = 3 * U * ga, ga
        if self.wd != 0:
            Ad = ga + self.wd * pa
            Ed = Ed + self.wd * self.Ep + 3 * U * Ad
        if self.m != 0:
            if self.first:
                self.Eb, self.B = Ed, Ad
            else:
                Bn = self.m * self.B + self.omd * Ad
                self.Eb = self.m * self.Eb + self.omd * Ed + 3 * U * Bn
                self.B = Bn
            Eu, Ua = self.Eb, self.B
        else:
            Eu, Ua = Ed, Ad
        self.first = False
        self.Ep = self.Ep + self.lr * Eu + 3 * U * (pa + self.lr * Ua)

    def p_ratio(self, p, p64):
        return float(((p.double().cpu() - p64).abs() / (SLACK * self.Ep).clamp_min(1e-300)).max())

    def b_ratio(self, b, b64):
        return float(((b.double().cpu() - b64).abs() / (SLACK * self.Eb).clamp_min(1e-300)).max())


def _sgd64(p0, gs, lr, momentum, dampening, wd, variant=None):
    """float64 SGD written out, and the wrong variants the bound has to reject."""
    p, buf, out = p0.clone(), None, []
    for g in gs:
        d = g if (wd == 0 or variant == 'no_decay') else g + wd * p
        if momentum != 0:
            prev = buf if buf is not None else torch.zeros_like(p)
            if buf is None:
                buf = (1 - dampening) * d if variant == 'damp_first' else d.clone()
            else:
                buf = momentum * buf + (1 - dampening) * d
            d = prev if variant == 'buf_prev' else buf
        p = p - lr * d
        out.append(p.clone())
    return out


def _kernel_run(p0, g1s, g2s, case, skips=None):
    from dvd_hip import ops
    lr, momentum, dampening, wd, scale, sp, _ = case
    sp_t = torch.tensor([sp], device='cuda') if sp is not None else None
    p = p0.clone().cuda()
    buf = torch.zeros_like(p) if momentum != 0 else None
    skip = torch.zeros(2, device='cuda') if skips is not None else None
    out = []
    for k in range(len(g1s)):
        if skips is not None:
            skip.copy_(torch.tensor(skips[k], dtype=torch.float32))
        ops.sgd_step(p, g1s[k].cuda(), buf, k + 1, lr, momentum, dampening, wd, scale=scale, scale_ptr=sp_t,
                     grad2=None if g2s is None else g2s[k].cuda(), skip_ptr=skip)
        out.append((p.cpu(), None if buf is None else buf.cpu()))
    return out


CASES = [  # lr, momentum, dampening, weight decay, scale, *scale_ptr, grad2
    (0.1, 0.9, 0.0, 1e-4, 0.5, 1.0 / 3.0, True),
    (0.1, 0.9, 0.5, 1e-4, 1.0, None, False),
    (0.1, 0.9, 0.5, 0.0, 0.5, 1.0 / 3.0, True),
    (1e-2, 0.0, 0.0, 0.0, 1.0, 1.0 / 3.0, True),
    (0.1, 0.0, 0.0, 1e-4, 1.0, None, False),
]
IDS = ['m0.9-wd-s-g2', 'm0.9-d0.5-wd', 'm0.9-d0.5-s-g2', 'm0-s-g2', 'm0-wd']


@pytest.mark.parametrize('n', [1, 2, 3, 6, 4099, BIG])
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_sgd_matches_float64_sgd_over_20_steps(n, case):
    lr, momentum, dampening, wd, scale, sp, with_g2 = case
    K, seed = 20, n + int(100 * lr) + int(10 * momentum) + int(4 * dampening) + int(1e4 * wd)
    p0 = (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 0.1).float()
    g1s = [_grad(n, k, seed) for k in range(K)]
    g2s = [_grad(n, k, seed + 1, 0.5) for k in range(K)] if with_g2 else None
    runs = [_kernel_run(p0, g1s, g2s, case) for _ in range(2)]
    got = runs[0]
    for a, b in zip(runs[0][-1], runs[1][-1]):
        assert a is None or torch.equal(_bits(a), _bits(b)), 'two identical SGD runs differ'

    ref = p0.double().clone()
    opt = torch.optim.SGD([ref], lr=lr, momentum=momentum, dampening=dampening, weight_decay=wd, foreach=False)
    bound = _Bound(n, lr, momentum, dampening, wd)
    geffs, worst = [], [0.0, 0.0]
    for k in range(K):
        ge, ga = _effective(g1s[k], None if g2s is None else g2s[k], scale, sp)
        geffs.append(ge)
        bound.step(ga, ref.detach())
        ref.grad = ge.clone()
        opt.step()
        ep = bound.p_ratio(got[k][0], ref.detach())
        eb = bound.b_ratio(got[k][1], opt.state[ref]['momentum_buffer']) if momentum != 0 else 0.0
        worst = [max(worst[0], ep), max(worst[1], eb)]
        assert ep <= 1.0 and eb <= 1.0, 'step %d: |dp| / bound %.3g, |dbuf| / bound %.3g' % (k + 1, ep, eb)
    name = 'test_16_sgd_%s_n%d' % (IDS[CASES.index(case)], n)
    helpers.log_measured(name + '_p_over_bound', worst[0], 1.0)
    helpers.log_measured(name + '_buf_over_bound', worst[1], 1.0)

    if n < 1000:
        return
    # the bound discriminates: each wrong SGD, in float64 on the same data, lands outside it
    right = _sgd64(p0.double(), geffs, lr, momentum, dampening, wd)

    def over_bound(p64):        # after the last step, against the bound of the last step
        return float(((p64 - right[-1]).abs() / (SLACK * bound.Ep).clamp_min(1e-300)).max())
    assert float((right[-1] - ref.detach()).abs().max()) <= 1e-12 * max(1.0, float(ref.detach().abs().max()))   # (the form)
    variants = []
    if momentum != 0:
        variants.append(('buf_prev', geffs))
        if dampening != 0:
            variants.append(('damp_first', geffs))
    if wd != 0:
        variants.append(('no_decay', geffs))
    if with_g2:
        variants.append(('grad2_dropped', [_effective(g, None, scale, sp)[0] for g in g1s]))
    assert variants
    for var, gs in variants:
        wrong = _sgd64(p0.double(), gs, lr, momentum, dampening, wd, variant=None if var == 'grad2_dropped' else var)
        e = over_bound(wrong[-1])
        helpers.log_measured('%s_mutant_%s_over_bound' % (name, var), e, 1.0)
        assert e > 1.0, '%s is inside the SGD bound (%.3g)' % (var, e)


@pytest.mark.parametrize('n', [3, 4099, BIG])
def test_guarded_sgd_skips_bitwise_and_starts_the_buffer_at_the_first_real_step(n):
    """Skip pairs [1,0], [0,1], [0,1], [1,1], [0,2] at steps 1..5 (momentum 0.9, dampening 0.5, no decay, s = 1, no grad2):
    skipped steps leave p and buf bit-identical; the first non-skipped step (step 2, effective step 1) leaves buf equal to its
    g1 bit for bit -- no dampening --; the series equals float64 torch.optim.SGD fed the non-skipped gradients only, within the
    bound of the unguarded test."""
    case = (0.1, 0.9, 0.5, 0.0, 1.0, None, False)
    seed = n + 29
    p0 = (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 0.1).float()
    g1s = [_grad(n, k, seed) for k in range(5)]
    skips = [(1, 0), (0, 1), (0, 1), (1, 1), (0, 2)]
    got = _kernel_run(p0, g1s, None, case, skips=skips)
    assert torch.equal(_bits(got[0][0]), _bits(p0)) and not got[0][1].any(), 'a skipped first step touched p or buf'
    assert torch.equal(_bits(got[1][1]), _bits(g1s[1])), 'the first real step did not set buf = g'
    for a, b in zip(got[3], got[2]):
        assert torch.equal(_bits(a), _bits(b)), 'a skipped step changed the state'
    ref = p0.double().clone()
    opt = torch.optim.SGD([ref], lr=0.1, momentum=0.9, dampening=0.5, foreach=False)
    bound, worst = _Bound(n, 0.1, 0.9, 0.5, 0.0), 0.0
    for k in range(5):
        if skips[k][0]:
            continue
        bound.step(g1s[k].double().abs(), ref.detach())
        ref.grad = g1s[k].double()
        opt.step()
        e = max(bound.p_ratio(got[k][0], ref.detach()), bound.b_ratio(got[k][1], opt.state[ref]['momentum_buffer']))
        worst = max(worst, e)
        assert e <= 1.0, 'step %d: %.3g of the bound' % (k + 1, e)
    helpers.log_measured('test_16_guarded_sgd_n%d_over_bound' % n, worst, 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# FlatNet


class _Ragged(torch.nn.Module):
    """Parameter sizes that are not multiples of 4, ~100k elements (7 real buckets of parallel.bucket_bounds; the 317 x 313
    weight spans several, so bucket bounds fall inside it) and two parameters that get no gradient (`dead`)."""

    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(5, 3)
        self.dead = torch.nn.Linear(7, 3)
        self.conv = torch.nn.Conv2d(3, 7, 3)
        self.big = torch.nn.Linear(317, 313)
        self.one = torch.nn.Parameter(torch.randn(1))

    DEAD = (2, 3)


def _feed(fn, k, seed):
    """The engine's view: fresh gradients for the live parameters only, absorbed into the flat buffer."""
    fn.grad.zero_()
    fn.detach_grads()
    for i, p in enumerate(fn.params):
        if i not in _Ragged.DEAD:
            p.grad = _grad(p.numel(), k, seed + 31 * i).view_as(p).cuda()
    fn.absorb_grads()


def _bucket_child(q):
    try:
        from dvd_hip import flat, parallel
        parallel.init_one_rank('nccl')
        assert parallel.is_distributed() and parallel.world_size() == 1
        torch.manual_seed(2)
        base = _Ragged()
        out = {}
        for nb in (1, 3, 4, 7):
            for momentum, wd in ((0.9, 1e-3), (0.0, 1e-3)):
                a = flat.FlatNet.sgd(copy.deepcopy(base).cuda(), 0.1, momentum=momentum, dampening=0.25, weight_decay=wd)
                b = flat.FlatNet.sgd(copy.deepcopy(base).cuda(), 0.1, momentum=momentum, dampening=0.25, weight_decay=wd)
                p_init = a.flat.clone()
                for k in range(3):
                    _feed(a, k, 40 + nb)
                    _feed(b, k, 40 + nb)
                    a.step()
                    b.all_reduce_and_step(nb)
                torch.cuda.synchronize()
                pairs = [(a.flat, b.flat), (a.grad, b.grad)] + ([(a.momentum_buf, b.momentum_buf)] if momentum else [])
                same = all(torch.equal(_bits(x), _bits(y)) for x, y in pairs)
                dead_kept = all(torch.equal(_bits(b.view(b.flat, i)), _bits(b.view(p_init, i))) for i in _Ragged.DEAD)
                dead_empty = momentum == 0 or not any(b.view(b.momentum_buf, i).any() for i in _Ragged.DEAD)
                inside = nb == 1 or any(o < lo < o + p.numel() for lo, _ in parallel.bucket_bounds(b.numel, nb)
                                        for o, p in zip(b.offsets, b.params))
                moved = not torch.equal(b.flat, p_init)
                out[(nb, momentum)] = (same, dead_kept, dead_empty, inside, moved,
                                       len(parallel.bucket_bounds(b.numel, nb)), len(b.live_ranges()),
                                       sorted(b.state_dict()['state']))
        parallel.shutdown()
        q.put(out)
    except BaseException as e:     # noqa: BLE001 -- hand the failure to the parent instead of a silent exit code
        import traceback
        q.put({'error': '%s\n%s' % (e, traceback.format_exc())})


@pytest.mark.timeout(600)
def test_flatnet_bucketed_all_reduce_sgd_equals_step_bitwise():
    """FlatNet.all_reduce_and_step(n_buckets) of an SGD net for n_buckets 1, 3, 4, 7 -- under a ONE-rank RCCL group, so the
    bucketed path really runs -- is bit-identical to step() over 3 steps, with two dead parameters (left out of every launch:
    their values and momentum buffers stay as they were, and they hold no state) and bucket bounds inside a parameter."""
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    p = ctx.Process(target=_bucket_child, args=(q,))
    p.start()
    out = q.get(timeout=500)
    p.join(60)
    assert 'error' not in out, out.get('error')
    for (nb, momentum), (same, dead_kept, dead_empty, inside, moved, real, ranges, state) in out.items():
        assert real == nb and inside, 'n_buckets=%d: %d buckets, a bound inside a parameter: %s' % (nb, real, inside)
        assert ranges == 2 and moved
        assert dead_kept and dead_empty, 'a dead parameter was stepped (n_buckets=%d, momentum %g)' % (nb, momentum)
        assert state == ([i for i in range(9) if i not in _Ragged.DEAD] if momentum else []), state
        assert same, 'bucketed SGD (n_buckets=%d, momentum %g) differs from step()' % (nb, momentum)


def test_flatnet_sgd_matches_float64_sgd_and_skips_dead_parameters():
    """FlatNet.sgd over 10 steps on ragged segments with two dead parameters and weight decay: live parameters against
    torch.optim.SGD(foreach=False) on float64 copies whose dead parameters have .grad None (the kernel bound, per parameter);
    dead parameters and every padding element keep their bits; the state has the same keys as torch's."""
    from dvd_hip import flat
    torch.manual_seed(4)
    fn = flat.FlatNet.sgd(_Ragged().cuda(), 0.1, momentum=0.9, dampening=0.5, weight_decay=1e-3)
    init = fn.flat.clone()
    refs = [p.detach().double().cpu().clone() for p in fn.params]
    opt = torch.optim.SGD(refs, lr=0.1, momentum=0.9, dampening=0.5, weight_decay=1e-3, foreach=False)
    bounds = [_Bound(p.numel(), 0.1, 0.9, 0.5, 1e-3) for p in refs]
    worst = 0.0
    for k in range(10):
        _feed(fn, k, 5)
        fn.step()
        for i, rp in enumerate(refs):
            rp.grad = None if i in _Ragged.DEAD else fn.view(fn.grad, i).double().cpu()
            if rp.grad is not None:
                bounds[i].step(rp.grad.abs().reshape(-1), rp.detach().reshape(-1))
        opt.step()
        for i, rp in enumerate(refs):
            if i in _Ragged.DEAD:
                continue
            e = max(bounds[i].p_ratio(fn.view(fn.flat, i).reshape(-1), rp.detach().reshape(-1)),
                    bounds[i].b_ratio(fn.view(fn.momentum_buf, i).reshape(-1), opt.state[rp]['momentum_buffer'].reshape(-1)))
            worst = max(worst, e)
            assert e <= 1.0, 'step %d, parameter %d: %.3g of the bound' % (k + 1, i, e)
    helpers.log_measured('test_16_flatnet_sgd_over_bound', worst, 1.0)
    used = torch.zeros(fn.numel, dtype=torch.bool)
    for i, (p, o) in enumerate(zip(fn.params, fn.offsets)):
        if i not in _Ragged.DEAD:
            used[o:o + p.numel()] = True
    assert torch.equal(_bits(fn.flat.cpu()[~used]), _bits(init.cpu()[~used]))       # dead parameters and padding
    assert not fn.momentum_buf.cpu()[~used].any()
    assert sorted(fn.state_dict()['state']) == sorted(opt.state_dict()['state'])


# ---------------------------------------------------------------------------------------------------------------------
# HBM


def _midas_model(optim, **over):
    import warnings
    from types import SimpleNamespace
    from dvd_hip.models.scene_flow_motion_field import Model
    o = dict(helpers.FULL_STEP_OPT, midas=True, full_logdir='/tmp', optim=optim)
    o.update(over)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return Model(SimpleNamespace(**o), None)


def _to_delta(model):
    import gc
    gc.collect()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    model.to(torch.device('cuda'))
    torch.cuda.synchronize()
    return torch.cuda.memory_allocated() - before


@pytest.mark.timeout(600)
def test_sgd_flatnet_of_midas_holds_one_buffer_less_than_adam():
    """MiDaS: Adam holds four flat fp32 buffers per net (parameters, gradients, two moments), SGD three (two at momentum 0).
    `Model.to` allocates at least 421 MB less with SGD -- one depth-net buffer -- and at least two buffers less at momentum 0."""
    import gc
    deltas, numel = {}, None
    for key, optim, over in (('adam', 'adam', {}), ('sgd', 'sgd', dict(sgd_momentum=0.9)), ('sgd0', 'sgd', dict(sgd_momentum=0.0))):
        m = _midas_model(optim, **over)
        deltas[key] = _to_delta(m)
        bufs = [b for b in (m._flat_depth.flat, m._flat_depth.grad, m._flat_depth.exp_avg, m._flat_depth.exp_avg_sq,
                            m._flat_depth.momentum_buf) if b is not None]
        assert len(bufs) == {'adam': 4, 'sgd': 3, 'sgd0': 2}[key], (key, len(bufs))
        assert all(b.numel() == m._flat_depth.numel and b.dtype == torch.float32 for b in bufs)
        numel = m._flat_depth.numel
        del m, bufs
        gc.collect()
        torch.cuda.empty_cache()
    one = 4 * numel
    print('Model.to allocations', deltas, 'one depth-net buffer', one)
    helpers.log_measured('test_16_hbm_adam_minus_sgd_bytes', deltas['adam'] - deltas['sgd'], 421e6)
    assert one >= 421e6
    assert deltas['adam'] - deltas['sgd'] >= one
    assert deltas['adam'] - deltas['sgd0'] >= 2 * one
