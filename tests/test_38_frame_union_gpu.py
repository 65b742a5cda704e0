"""csrc/frame_union.hip on the GPU: dvd_union_gather / dvd_union_scatter / dvd_union_reduce against a plain-torch restatement
written here.  The kernels copy rows and add fp32 values one after the other in list order, so every comparison is bit for bit.
Id patterns: those of tests/test_frame_union_cpu.py (B = 4), at quantum 1 and quantum 8."""
import ctypes

import numpy as np
import pytest
import torch

from test_frame_union_cpu import PATTERNS

pytestmark = pytest.mark.gpu

DEV = 'cuda'
PATTERN = 0xA5
SIZES = [(1, 1), (5, 7), (3, 16), (16, 24), (67, 69)]


def _guarded(shape, dtype=torch.float32, pad=64):
    """A tensor inside a larger buffer filled with a byte pattern: (buffer, view, pad)."""
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    buf = torch.full((pad + n + pad,), PATTERN, dtype=torch.uint8, device=DEV)
    return buf, buf[pad:pad + n].view(dtype).view(shape), pad


def _intact(buf, pad):
    return bool((buf[:pad] == PATTERN).all()) and bool((buf[-pad:] == PATTERN).all())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


# -- the restatement --------------------------------------------------------------------------------------------------
def spec_gather(img_1, img_2, plan):
    return torch.stack([(img_2 if s else img_1)[r] for s, r in plan['src']])


def spec_scatter(D, plan):
    return torch.stack([D[u] for u in plan['u1']]), torch.stack([D[u] for u in plan['u2']])


def spec_reduce(g_d1, g_d2, plan):
    rows = []
    for u in range(plan['U_pad']):
        acc = torch.zeros_like(g_d1[0])
        for s, r in plan['entries'][plan['offsets'][u]:plan['offsets'][u + 1]]:
            acc = acc + (g_d2 if s else g_d1)[r]          # one fp32 add per contributor, in list order
        rows.append(acc)
    return torch.stack(rows)


def _tables(f1, f2, quantum):
    from dvd_hip import ops
    from dvd_hip.models.frame_union import plan_union
    plan = plan_union(f1, f2, quantum)
    return plan, ops.UnionTables(plan, DEV)


def _rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    # values of mixed magnitude and sign, so that the ORDER of a row's additions shows in the last bit
    return (torch.randn(shape, generator=g) * torch.exp(4 * torch.randn(shape, generator=g))).to(DEV)


@pytest.mark.parametrize('quantum', [1, 8])
@pytest.mark.parametrize('H,W', SIZES)
def test_three_kernels_against_the_restatement(H, W, quantum):
    """1 x 1; 5 x 7 (dwords); 3 x 16 and 16 x 24 (16-byte accesses: every base below is 64-byte aligned and the rows are
    multiples of 16); 67 x 69 (18 492-byte depth rows and 55 476-byte image rows: dwords, several tiles per row)."""
    from dvd_hip import ops
    for k, (name, f1, f2) in enumerate(PATTERNS):
        plan, tab = _tables(f1, f2, quantum)
        B, U_pad = 4, plan['U_pad']
        img_1, img_2 = _rand((B, 3, H, W), 10 * k + H), _rand((B, 3, H, W), 10 * k + H + 1)
        buf, img_u, pad = _guarded((U_pad, 3, H, W))
        assert ops.union_gather(img_1, img_2, tab, out=img_u) is img_u
        assert _same_bits(img_u, spec_gather(img_1, img_2, plan)) and _intact(buf, pad), (name, 'gather')
        for u in range(plan['U'], U_pad):                 # padding rows equal union row 0
            assert _same_bits(img_u[u], img_u[0]), (name, u)

        D = _rand((U_pad, 1, H, W), 10 * k + H + 2)
        (b1, d1, p1), (b2, d2, p2) = _guarded((B, 1, H, W)), _guarded((B, 1, H, W))
        ops.union_scatter(D, tab, out=(d1, d2))
        w1, w2 = spec_scatter(D, plan)
        assert _same_bits(d1, w1) and _same_bits(d2, w2) and _intact(b1, p1) and _intact(b2, p2), (name, 'scatter')

        g1, g2 = _rand((B, 1, H, W), 10 * k + H + 3), _rand((B, 1, H, W), 10 * k + H + 4)
        bg, G, pg = _guarded((U_pad, 1, H, W))
        ops.union_reduce(g1, g2, tab, out=G)
        assert _same_bits(G, spec_reduce(g1, g2, plan)) and _intact(bg, pg), (name, 'reduce')
        assert bool((_bits(G[plan['U']:]) == 0).all()), (name, 'padding rows of reduce are +0.0')
        # what the sum is for: every image's gradient arrives exactly once
        if name == 'distinct':
            assert _same_bits(G[:4], 0.0 + g1) and _same_bits(G[4:8], 0.0 + g2)

        # gather followed by scatter gives back the per-pair images (same id = same image: build them that way)
        frames = _rand((16, 3, H, W), 99 + H)
        s1, s2 = frames[f1].contiguous(), frames[f2].contiguous()
        e1, e2 = ops.union_scatter(ops.union_gather(s1, s2, tab), tab)
        assert _same_bits(e1, s1) and _same_bits(e2, s2), (name, 'round trip')
    torch.cuda.synchronize()


def test_more_tiles_than_the_grid():
    """67 x 69 x 3 rows take 14 tiles on the dword path: some 330 union rows make 4 600 tiles, more than the 4 096-block grid, so
    the grid-stride loop runs; ids repeat, so the reduction has rows of several contributors."""
    from dvd_hip import ops
    rng = np.random.RandomState(7)
    B = 200
    f1, f2 = rng.randint(0, 1000, size=B), rng.randint(0, 1000, size=B)
    plan, tab = _tables(f1, f2, 1)
    assert plan['U'] >= 293 and max(np.diff(plan['offsets'])) >= 3
    a, b = _rand((B, 3, 67, 69), 1), _rand((B, 3, 67, 69), 2)
    assert _same_bits(ops.union_gather(a, b, tab), spec_gather(a, b, plan))
    G = ops.union_reduce(a, b, tab)
    assert _same_bits(G, spec_reduce(a, b, plan))
    d1, d2 = ops.union_scatter(G, tab)
    w1, w2 = spec_scatter(G, plan)
    assert _same_bits(d1, w1) and _same_bits(d2, w2)


def test_a_source_sliced_at_an_offset_of_four_bytes():
    """A 3-channel source that starts 4 bytes into its allocation: rows of 3 x 16 x 24 floats are multiples of 16 bytes, the base
    is not, so the launch takes dwords -- and must not touch the float in front of the slice or behind it."""
    from dvd_hip import ops
    plan, tab = _tables([0, 1, 2, 3], [1, 2, 3, 4], 8)
    n = 4 * 3 * 16 * 24
    raw = _rand((2, n + 8), 3)
    img_1, img_2 = raw[0, 1:n + 1].view(4, 3, 16, 24), raw[1, 1:n + 1].view(4, 3, 16, 24)
    assert img_1.data_ptr() % 16 == 4 and img_1.is_contiguous()
    buf, img_u, pad = _guarded((8, 3, 16, 24), pad=68)            # ... and a destination 4 bytes off as well
    assert img_u.data_ptr() % 16 == 4
    ops.union_gather(img_1, img_2, tab, out=img_u)
    assert _same_bits(img_u, spec_gather(img_1, img_2, plan)) and _intact(buf, pad)
    g1, g2 = raw[0, 1:1 + 4 * 384].view(4, 1, 16, 24), raw[1, 1:1 + 4 * 384].view(4, 1, 16, 24)
    bg, G, pg = _guarded((8, 1, 16, 24), pad=68)
    ops.union_reduce(g1, g2, tab, out=G)
    assert _same_bits(G, spec_reduce(g1, g2, plan)) and _intact(bg, pg)
    (b1, d1, p1), (b2, d2, p2) = _guarded((4, 1, 16, 24), pad=68), _guarded((4, 1, 16, 24))
    ops.union_scatter(G, tab, out=(d1, d2))
    w1, w2 = spec_scatter(G, plan)
    assert _same_bits(d1, w1) and _same_bits(d2, w2) and _intact(b1, p1) and _intact(b2, p2)


def test_frame_ids_travel_through_the_gather_as_well():
    """The hourglass's per-frame embedding takes the ids of the union rows: int64 and fp32 id vectors, 8 / 4 bytes per row."""
    from dvd_hip import ops
    plan, tab = _tables([7, 2, 7, 5], [2, 0, 5, 7], 8)
    for dtype in (torch.int64, torch.float32):
        f1, f2 = torch.tensor([7, 2, 7, 5], dtype=dtype, device=DEV), torch.tensor([2, 0, 5, 7], dtype=dtype, device=DEV)
        got = ops.union_gather(f1, f2, tab)
        assert got.dtype == dtype and got.tolist() == plan['frames'] + [7] * 4


def test_two_runs_are_bitwise_equal():
    from dvd_hip import ops
    plan, tab = _tables([9, 9, 9, 9], [9, 9, 9, 9], 8)          # eight contributors of one row
    g1, g2 = _rand((4, 1, 67, 69), 5), _rand((4, 1, 67, 69), 6)
    first = ops.union_reduce(g1, g2, tab)
    for _ in range(3):
        assert _same_bits(ops.union_reduce(g1, g2, tab), first)
    assert _same_bits(first, spec_reduce(g1, g2, plan))
    a = ops.union_gather(g1, g2, tab)
    assert _same_bits(ops.union_gather(g1, g2, tab), a)
    d = ops.union_scatter(a, tab)
    e = ops.union_scatter(a, tab)
    assert _same_bits(d[0], e[0]) and _same_bits(d[1], e[1])


def test_the_kernels_skip_an_index_outside_its_table():
    """The guards inside the kernels, reached through the C ABI (the ops wrappers refuse such tables first).  Every buffer is
    rows 1.. of a larger allocation, so an index just outside its table would read or write valid memory if a guard were
    missing; the row of such an index must stay untouched (gather, scatter) or receive nothing from it (reduce)."""
    from dvd_hip import _lib
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def p(t):
        return ctypes.c_void_p(t.data_ptr())

    B, n = 3, 300                                                   # 1200-byte rows: the 16-byte path
    big_1, big_2 = torch.rand(B + 2, n, device=DEV), torch.rand(B + 2, n, device=DEV)
    img_1, img_2 = big_1[1:1 + B], big_2[1:1 + B]
    # gather: union rows 1, 3, 4, 5 carry a bad set or row
    sets = torch.tensor([0, 2, 1, 0, -1, 1], dtype=torch.int32, device=DEV)
    rows = torch.tensor([2, 0, 1, 3, 0, -1], dtype=torch.int32, device=DEV)
    out = torch.full((6, n), 7.0, device=DEV)
    assert lib.dvd_union_gather(p(img_1), p(img_2), p(out), p(sets), p(rows), 6, B, 4 * n, stream) == _lib.DVD_OK
    torch.cuda.synchronize()
    assert torch.equal(out[0], img_1[2]) and torch.equal(out[2], img_2[1])
    assert bool((out[[1, 3, 4, 5]] == 7.0).all())
    # scatter: U_pad = 4 rows of a union of 6; indices 4, 5 and -1 are outside
    D = torch.rand(8, n, device=DEV)[1:7]
    u1 = torch.tensor([3, 4, 0], dtype=torch.int32, device=DEV)
    u2 = torch.tensor([-1, 1, 5], dtype=torch.int32, device=DEV)
    d1, d2 = torch.full((B, n), 7.0, device=DEV), torch.full((B, n), 7.0, device=DEV)
    assert lib.dvd_union_scatter(p(D), p(d1), p(d2), p(u1), p(u2), B, 4, 4 * n, stream) == _lib.DVD_OK
    torch.cuda.synchronize()
    assert torch.equal(d1[0], D[3]) and torch.equal(d1[2], D[0]) and torch.equal(d2[1], D[1])
    assert bool((d1[1] == 7.0).all()) and bool((d2[[0, 2]] == 7.0).all())
    # reduce: entries 6 (= 2B), -1 and 7 add nothing; a range that runs past the entry list is cut at 2B entries
    entries = torch.tensor([0, 6, 4, -1, 2, 7, 5, 5, 5], dtype=torch.int32, device=DEV)[:6]
    offsets = torch.tensor([0, 3, 5, 9], dtype=torch.int32, device=DEV)
    G = torch.full((3, n), 7.0, device=DEV)
    assert lib.dvd_union_reduce(p(img_1), p(img_2), p(G), p(offsets), p(entries), 3, B, n, stream) == _lib.DVD_OK
    torch.cuda.synchronize()
    zero = torch.zeros(n, device=DEV)
    assert torch.equal(G[0], zero + img_1[0] + img_2[1]) and torch.equal(G[1], zero + img_1[2])
    assert torch.equal(G[2], zero)                                   # entry 7 is outside, entries 6..8 of the range do not exist
    assert lib.dvd_union_gather(None, p(img_2), p(out), p(sets), p(rows), 6, B, 4 * n, stream) == _lib.DVD_EINVAL
    assert lib.dvd_union_reduce(p(img_1), p(img_2), p(img_1), p(offsets), p(entries), 3, B, n, stream) == _lib.DVD_EINVAL


def test_the_wrappers_validate_before_they_launch():
    from dvd_hip import ops
    from dvd_hip.models.frame_union import plan_union
    good = plan_union([0, 1, 2, 3], [1, 2, 3, 4], 8)
    img_1, img_2 = torch.rand(4, 3, 5, 7, device=DEV), torch.rand(4, 3, 5, 7, device=DEV)
    D = torch.rand(8, 1, 5, 7, device=DEV)
    g = torch.rand(4, 1, 5, 7, device=DEV)

    def broken(**changes):
        plan = {k: list(v) if isinstance(v, list) else v for k, v in good.items()}
        for k, (i, v) in changes.items():
            plan[k][i] = v
        return ops.UnionTables(plan, DEV)

    c0 = ops.flop_counters()['gather']
    bad = [
        ('outside', lambda: ops.union_gather(img_1, img_2, broken(src=(2, (0, 4))))),
        ('outside', lambda: ops.union_gather(img_1, img_2, broken(src=(5, (2, 0))))),
        ('outside', lambda: ops.union_gather(img_1, img_2, broken(src=(1, (0, -1))))),
        ('outside', lambda: ops.union_scatter(D, broken(u1=(0, 8)))),
        ('outside', lambda: ops.union_scatter(D, broken(u2=(3, -1)))),
        ('outside', lambda: ops.union_reduce(g, g.clone(), broken(entries=(7, (2, 0))))),
        ('outside', lambda: ops.union_reduce(g, g.clone(), broken(offsets=(8, 9)))),
        ('not decrease', lambda: ops.union_reduce(g, g.clone(), broken(offsets=(2, 0)))),
        ('GPU tensor', lambda: ops.union_gather(img_1.cpu(), img_2, broken())),
        ('contiguous', lambda: ops.union_gather(img_1.transpose(2, 3), img_2.transpose(2, 3), broken())),
        ('4 rows', lambda: ops.union_gather(img_1[:3], img_2[:3], broken())),
        ('differ', lambda: ops.union_gather(img_1, img_2[:, :2].contiguous(), broken())),
        ('8 rows', lambda: ops.union_scatter(D[:5], broken())),
        ('float32', lambda: ops.union_reduce(g.double(), g.double(), broken())),
        ('8 rows', lambda: ops.union_reduce(g, g.clone(), broken(), out=torch.empty(5, 1, 5, 7, device=DEV))),
        ('dwords', lambda: ops.union_gather(torch.zeros(4, 3, dtype=torch.uint8, device=DEV),
                                            torch.zeros(4, 3, dtype=torch.uint8, device=DEV), broken())),
    ]
    for match, call in bad:
        with pytest.raises(RuntimeError, match=match):
            call()
    torch.cuda.synchronize()
    assert ops.flop_counters()['gather'] == c0, 'a refused call reached the library'
    tab = broken()
    img_u = ops.union_gather(img_1, img_2, tab)                      # and the valid calls of the same tensors go through
    assert _same_bits(img_u, spec_gather(img_1, img_2, good))
    assert _same_bits(ops.union_reduce(g, g.clone(), tab), spec_reduce(g, g, good))
    # bytes: gather reads and writes U_pad rows + two index ints per row
    assert ops.flop_counters()['gather'] - c0 == 2 * img_u.numel() * 4 + 8 * 8 + (2 * 4 + 8) * 35 * 4 + 4 * (9 + 8)
