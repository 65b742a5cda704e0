"""tests/wgrad_spec.py is sound, proven without a GPU:

  (a) its case table reaches every instantiation key of REQUIRED -- as dvd_xwgrad_describe, the dispatch itself, reports the
      launches under each hook value the table uses -- and every edge of EDGES per family; no key is reached that REQUIRED does
      not list, and every row of the table is the only one to reach something, so removing any one row fails this file;
  (b) for every case and both data sets the exactness premises hold in the kernel's arithmetic, emulated in numpy (pow2_scale,
      fp16 rounding to nearest even of h and l, the three products): exact_data has l = 0, split_data has h + l = x 2^e with live
      low terms, and sum |terms| of every accumulator -- a bound on every partial sum in every order -- is below 2^24 units;
  (c) dvd_xwgrad_describe answers DVD_EINVAL exactly where the size queries answer 0;
  (d) the workspace bytes it reports never exceed the matching dvd_xwgrad*_workspace_bytes."""
import ctypes
import json
import os

import pytest
import torch

import wgrad_spec as S

HERE = os.path.dirname(os.path.abspath(__file__))
WALKING = ('xwgrad3', 'xwgrad3g', 'xwgradk5', 'xwgradk7', 'xwgradk11')
# what every family's rows must show between them (the issue's list of edges)
EDGES = {g: ['H=1', 'H=2', 'W=1', 'W=3', 'W=64', 'W=65', 'W=144', 'N=3 slices cross images', 'ragged blocks', 'one ragged block', 'two blocks',
             'fp16 odd W', 'hook 1', 'hook 2', 'hook 3'] for g in WALKING}
EDGES['xwgrad3'] = EDGES['xwgrad3'] + ['uneven slices', 'groups']
EDGES['xwgrad3g'] = EDGES['xwgrad3g'] + ['uneven slices']
EDGES['xwgradk5'] = EDGES['xwgradk5'] + ['slices end inside images']
EDGES['xwgrad1s'] = ['HW=4', 'HW=12', 'HW=16', 'HW=252', 'odd chunks above the slices', 'ragged blocks', 'one ragged block', 'two blocks',
                     'fp16 odd HW', 'hook 1', 'hook 2', 'hook 3']
EDGES['xwgrad1b'] = ['HW=4', 'HW=12', 'HW=16', 'HW=252', 'odd chunks above the slices, FW', 'odd chunks above the slices, not FW', 'ragged blocks', 'one ragged block', 'two blocks',
                     'hook 1', 'hook 2', 'hook 3']


@pytest.fixture(scope='module')
def lib():
    from dvd_hip import _lib
    L = _lib.load()
    yield L
    assert L.dvd_xwgrad_select(0) == 0


def _under(lib, hook):
    assert lib.dvd_xwgrad_select(hook) == 0


def _slice_units(b, Sl, U):
    """csrc/wg3_plan.h wg_slice_units: the row steps [u0, u1) of slice b of Sl over U."""
    q, m = divmod(U, Sl)
    u0 = b * q + min(b, m)
    return u0, u0 + q + (1 if b < m else 0)


def _group(d):
    fam = S.FAMILIES[d['family']]
    return fam + str(d['ks']) if fam == 'xwgradk' else fam


def _items_of(lib, case):
    """Everything a row contributes: its instantiation keys, and (family, edge) pairs for the family that serves it under the
    automatic selection in fp32."""
    name, KS, N, Cin, Cout, H, W, G, storages, relu_in, rowsum, hooks = case
    items = set()
    for st, rs, hook in S.runs_of(case):
        _under(lib, hook)
        status, d = S.describe(lib, case, st, rs)
        assert status == 0, (name, st, rs, hook)
        items |= S.keys_of(d)
    _under(lib, 0)
    d = S.describe(lib, case, S.F32)[1]
    grp, fam = _group(d), S.FAMILIES[d['family']]
    edges = ['hook %d' % h for h in hooks if h]
    cb = S.BLOCK[fam]
    if (Cin // G) % cb and (Cout // G) % cb:
        edges.append('ragged blocks')
        if d['nco'] == d['nci'] == 1:
            edges.append('one ragged block')
    if (d['nco'] >= 2 and d['nci'] >= 2) or (fam == 'xwgrad3g' and G >= 2):
        edges.append('two blocks')
    if G > 1:
        edges.append('groups')
    if KS == 1:
        HW = H * W
        edges.append('HW=%d' % HW)
        chunks = N * -(-HW // (16 if fam == 'xwgrad1b' else 32))
        if chunks % 2 and chunks > d['slices']:
            edges.append('odd chunks above the slices' + ((', FW' if d['fw'] else ', not FW') if fam == 'xwgrad1b' else ''))
        if S.H16 in storages and HW % 2:
            edges.append('fp16 odd HW')
    else:
        edges += ['H=%d' % H, 'W=%d' % W]
        if S.H16 in storages and W % 2:
            edges.append('fp16 odd W')
        for launch in d['L']:
            U = N * launch['ncols'] * H
            if U % launch['S']:
                edges.append('uneven slices')
            for b in range(launch['S']):
                u0, u1 = _slice_units(b, launch['S'], U)
                if u1 % H:
                    edges.append('slices end inside images')
                if N == 3 and u0 // H // launch['ncols'] != (u1 - 1) // H // launch['ncols']:
                    edges.append('N=3 slices cross images')
    return items | {(grp, e) for e in edges}


@pytest.fixture(scope='module')
def items(lib):
    return {c[0]: _items_of(lib, c) for c in S.CASES}


def test_the_table_reaches_every_key_and_edge(items):
    reached = set().union(*items.values())
    keys = {i for i in reached if isinstance(i, str)}
    missing = [k for k in S.REQUIRED if k not in keys]
    assert not missing, 'no row of CASES reaches %s' % missing
    assert keys <= set(S.REQUIRED), 'reached but not listed in REQUIRED: %s' % sorted(keys - set(S.REQUIRED))
    missing = [(g, e) for g in EDGES for e in EDGES[g] if (g, e) not in reached]
    assert not missing, 'no row of CASES shows %s' % missing


def test_every_row_is_needed(items):
    """Each row is the only one to reach some required key or edge: the coverage test above fails when any one row is removed."""
    required = set(S.REQUIRED) | {(g, e) for g in EDGES for e in EDGES[g]}
    for name in items:
        others = set().union(*[v for k, v in items.items() if k != name])
        assert (items[name] & required) - others, 'row %r reaches nothing that another row does not' % name


def test_every_hook_value_is_used():
    assert {h for c in S.CASES for h in c[11]} == {0, 1, 2, 3}


@pytest.mark.parametrize('case', S.CASES, ids=[c[0].replace(' ', '_') for c in S.CASES])
def test_exactness_premises(case):
    KS, N, Cin, Cout, H, W, G = S.shape_of(case)
    relu = case[9]
    # exact_data, fp32 entry points: at the exact maxima and at 64 times that
    d = S.exact_data(case)
    assert float(d['x'].abs().max()) == d['x_amax'] == 3.0 and float(d['gy'].abs().max()) == d['gy_amax'] == 3.0
    assert bool((d['x'] < 0).any()) and bool(torch.signbit(d['x'][d['x'] == 0]).any()), 'relu_in needs negative values and -0.0'
    for up in (1.0, 64.0):
        xh, xl, sx = S.split_terms(d['x'], d['x_amax'] * up, relu)
        gh, gl, sg = S.split_terms(d['gy'], d['gy_amax'] * up)
        assert not bool(xl.any()) and not bool(gl.any()), 'exact_data: a low term is not 0'
        assert torch.equal(xh / sx, d['x'].double().clamp_min(0.0) if relu else d['x'].double()) and torch.equal(gh / sg, d['gy'].double())
        assert S.worst_partial_sum(case, xh, xl, gh, gl) < 2.0 ** 24
    # fp16 entry points: the operands are the matrix operands, one product each, the result times 2^-3
    x16, g16 = d['x'].half().double(), d['gy'].half().double()
    assert torch.equal(x16, d['x'].double()) and torch.equal(g16, d['gy'].double())
    worst = S.worst_partial_sum(case, x16.clamp_min(0.0) if relu else x16, torch.zeros_like(x16), g16, torch.zeros_like(g16))
    assert worst < 2.0 ** 24 and S.H16_OUT_SCALE == 2.0 ** -3
    # the row sums: fp32 sums of the (scaled) gy values in any order, then double
    assert float(d['gy'].double().abs().sum((0, 2, 3)).max()) < 2.0 ** 24
    # the specification itself is an fp32 value
    want = S.spec(d['x'], d['gy'], KS, G, relu)[0]
    assert torch.equal(want.float().double(), want)

    # split_data (fp32 entry points)
    d = S.split_data(case)
    assert int(d['x_amax']) == 7 and int(d['gy_amax']) == 7
    xh, xl, sx = S.split_terms(d['x'], d['x_amax'], relu)
    gh, gl, sg = S.split_terms(d['gy'], d['gy_amax'])
    assert sx == sg == 2.0 ** 11
    xa = d['x'].double().clamp_min(0.0) if relu else d['x'].double()
    assert torch.equal((xh + xl) / sx, xa) and torch.equal((gh + gl) / sg, d['gy'].double()), 'split_data: h + l is not the operand'
    assert bool(xl.any()) and bool(gl.any()), 'split_data: the low terms are all 0'
    assert S.granule(xh) == S.granule(gh) == 2.0 ** 11 and S.granule(xl) == S.granule(gl) == 0.5, 'split_data: h = a 2^11, l = b / 2'
    assert S.worst_partial_sum(case, xh, xl, gh, gl) < 2.0 ** 24, 'split_data: an accumulator can leave 24 bits'
    kern, truth = S.split_expected(case, d)
    assert torch.equal(kern.float().double(), kern)
    # the dropped l l' term is all that separates the two
    ll = S.wgrad(xl, gl, KS, G) / (sx * sg)
    assert torch.equal(kern + ll, truth) and bool((kern != truth).any())
    # gy is nonzero in every row, and on the first and last column of every strip
    rows, width, strip = (1, H * W, 16) if KS == 1 else (H, W, 64)
    nz = (d['gy'] != 0).view(N, Cout, rows, width)
    assert bool(nz.any(3).any(1).all()), 'split_data: a row without a gradient'
    cols = nz.any(2).any(1).any(0)
    assert all(bool(cols[c]) for c in S._edge_columns(width, strip)), 'split_data: a strip edge without a gradient'
    assert bool(cols.all()), 'split_data: a column (a position of a cell / of a K step) where no channel has a gradient'


BAD = [(0, 64, 64, 8, 8), (2, 0, 64, 8, 8), (2, 64, 0, 8, 8), (2, 64, 64, 0, 8), (2, 64, 64, 8, 0), (-1, 64, 64, 8, 8),
       (2, 64, 64, 8, -8)]               # the list of tests/test_wgrad_routes_cpu.py


def _desc(lib, KS, N, Cin, Cout, H, W, G, h16=0, rs=0):
    out = (ctypes.c_int * S.WDESC_INTS)()
    return lib.dvd_xwgrad_describe(KS, N, Cin, Cout, H, W, G, h16, rs, ctypes.addressof(out)), out


def _query(lib, KS, N, Cin, Cout, H, W, G):
    if KS == 1:
        return lib.dvd_xwgrad1s_workspace_bytes(N, Cin, Cout, H, W) if G == 1 else 0
    if KS == 3:
        return lib.dvd_xwgrad3_workspace_bytes(N, Cin, Cout, H, W, G)
    return lib.dvd_xwgradk_workspace_bytes(N, Cin, Cout, H, W, KS) if G == 1 else 0


@pytest.mark.parametrize('select', [0, 1, 2, 3])
def test_describe_refuses_exactly_what_the_size_queries_refuse(lib, select):
    from dvd_hip import _lib
    _under(lib, select)
    shapes = [(KS,) + bad + (1,) for bad in BAD for KS in (1, 3, 5, 7, 11)]
    shapes += [(3, 2, 64, 96, 8, 8, G) for G in (0, -2, 3, 5, 1, 2, 32)]
    shapes += [(KS, 2, 32, 32, 16, 16, 1) for KS in (0, 1, 2, 3, 4, 5, 6, 7, 9, 11, 13, -5)]
    shapes += [(KS, 2, 64, 64, 8, 8, 2) for KS in (1, 5, 7, 11)]                     # groups only for 3x3
    shapes += [S.shape_of(c) for c in S.CASES]
    n_bad = 0
    for sh in shapes:
        for h16 in (0, 1):
            status, out = _desc(lib, *sh, h16=h16)
            assert status in (0, _lib.DVD_EINVAL)
            assert (status == _lib.DVD_EINVAL) == (_query(lib, *sh) == 0), (sh, h16)
            n_bad += status != 0
    assert n_bad >= 2 * (len(BAD) * 5 + 4 + 7 + 4)
    # row sums: where an entry point takes the pointer (fp32, 1x1 and 3x3)
    assert _desc(lib, 3, 2, 64, 64, 8, 8, 1, 0, 1)[0] == 0 and _desc(lib, 1, 2, 64, 64, 8, 8, 1, 0, 1)[0] == 0
    assert _desc(lib, 3, 2, 64, 64, 8, 8, 1, 1, 1)[0] == _lib.DVD_EINVAL
    assert _desc(lib, 5, 2, 64, 64, 8, 8, 1, 0, 1)[0] == _lib.DVD_EINVAL
    assert lib.dvd_xwgrad_describe(3, 2, 64, 64, 8, 8, 1, 0, 0, None) == _lib.DVD_EINVAL


@pytest.mark.parametrize('select', [0, 1, 2, 3])
def test_described_workspace_fits_the_size_query(lib, select):
    """For the table and for every shape of tests/golden/wgrad_routes.json (the headline step's layers among them)."""
    with open(os.path.join(HERE, 'golden', 'wgrad_routes.json')) as f:
        shapes = [tuple(s) for s in json.load(f)['shapes']]
    shapes += [S.shape_of(c) for c in S.CASES]
    _under(lib, select)
    exact = 0
    for sh in shapes:
        q = _query(lib, *sh)
        assert q > 0, sh
        for h16, rs in ((0, 0), (1, 0)) + (((0, 1),) if sh[0] in (1, 3) else ()):
            status, out = _desc(lib, *sh, h16=h16, rs=rs)
            assert status == 0, (sh, h16, rs)
            d = dict(zip(S.TAIL, out[S.L0 + 2 * S.L_INTS:]))
            need = d['ws_lo'] + (d['ws_hi'] << 31)
            assert 0 < need <= q, (sh, h16, rs, need, q)
            exact += need == q
            # the row sums come from exactly one place
            rsum = out[4]
            assert (rsum + d['chansum'] == 1) if rs else (rsum == 0 and d['chansum'] == 0)
            if rs and select == 0:
                assert rsum == lib.dvd_xwgrad_rowsum_in_kernel(sh[1], sh[2], sh[3], sh[4], sh[5], sh[0], sh[6])
    assert exact > 0


def test_describe_reports_the_plan(lib):
    """Pinned by hand from csrc/wg3_plan.h for one shape per walking family: 3 images of 6 x 65, 8 -> 8 channels."""
    _under(lib, 0)
    d = S.describe(lib, S.CASE['w3 6x65'], S.F32)[1]
    # pairs = 1: two classes, Sc = min(256, N H / 8) = 2 slices each; the tail strip has one live K step
    assert (d['family'], d['fw'], d['launches'], d['slices'], d['threads'], d['nco'], d['nci']) == (0, 1, 2, 4, 768, 1, 1)
    assert d['L'] == [dict(nk=4, key_nk=4, S=2, slice0=0, strip0=0, ncols=1), dict(nk=1, key_nk=1, S=2, slice0=2, strip0=1, ncols=1)]
    assert d['need'] == 4 * 9 * 8 * 8 * 4 and d['align'] == 4 and d['second'] == 0
    d = S.describe(lib, S.CASE['w3 6x65'], S.H16)[1]                     # odd fp16 rows: the guarded step, no NK argument
    assert d['fw'] == 0 and [l['key_nk'] for l in d['L']] == [0, 0] and [l['nk'] for l in d['L']] == [4, 1] and d['align'] == 2
    d = S.describe(lib, S.CASE['k11 5x65'], S.H16)[1]
    # min_rs = 44 rows: Sc = max(1, 15 / 44) = 1; LDS one term: 2 * 32 * 144 + 12 * 32 * 176
    assert (d['family'], d['ks'], d['second'], d['threads'], d['lds'], d['slices']) == (2, 11, 1, 704, 2 * 32 * 144 + 12 * 32 * 176, 2)
    _under(lib, 3)
    d = S.describe(lib, S.CASE['w3 6x65'], S.F32)[1]
    # the deal: RS = H (6 <= 8), items = 3 images x 2 strips = 6 slices, one launch of four K steps over both strips
    assert d['deal'] == 1 and d['L'] == [dict(nk=4, key_nk=4, S=6, slice0=0, strip0=0, ncols=2)] and d['need'] == 6 * 9 * 64 * 4
    _under(lib, 0)
