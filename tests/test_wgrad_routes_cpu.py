"""The routing of the weight-gradient entry points (csrc/xwgrad3.hip, wg_route): which kernel serves a shape decides whether the
kernel delivers the row sums of gy itself (dvd_xwgrad_rowsum_in_kernel, what conv._XConvBn asks) and how much workspace a 1x1 call
needs (dvd_xwgrad1s_workspace_bytes).  Both are pure host code, so they run here without a GPU.

tests/golden/wgrad_routes.json holds what the library answered before the host code got its single routing function, for every
weight-gradient shape of the headline step (the lists of tools/wg_plan_check.cpp, the 1x1 layers of ResNeXt at 96x168 .. 12x21),
the shapes of tests/test_40_wgrad_rowsum_gpu.py and tests/test_46_wgrad_live_steps_gpu.py, and edge shapes (H * W no multiple of
16 / of 4, odd W, 191 / 192 channels, 32 / 33 channels per group), each under dvd_xwgrad_select(0), (1) and (2)."""
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def lib():
    from dvd_hip import _lib
    return _lib.load()


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(HERE, 'golden', 'wgrad_routes.json')) as f:
        return json.load(f)


@pytest.mark.parametrize('select', [0, 1, 2])
def test_routes_match_the_recorded_ones(lib, golden, select):
    want = golden['select'][str(select)]
    assert len(golden['shapes']) == len(want['rowsum_in_kernel']) == len(want['xwgrad1s_workspace_bytes']) >= 80
    try:
        assert lib.dvd_xwgrad_select(select) == 0
        for (KS, N, Cin, Cout, H, W, G), rik, ws in zip(golden['shapes'], want['rowsum_in_kernel'], want['xwgrad1s_workspace_bytes']):
            tag = 'select(%d) k%d %dx%d->%d g%d %dx%d' % (select, KS, N, Cin, Cout, G, H, W)
            assert lib.dvd_xwgrad_rowsum_in_kernel(N, Cin, Cout, H, W, KS, G) == rik, tag
            assert (ws is not None) == (KS == 1), tag
            if KS == 1:
                assert lib.dvd_xwgrad1s_workspace_bytes(N, Cin, Cout, H, W) == ws, tag
    finally:
        assert lib.dvd_xwgrad_select(0) == 0


def test_the_fixture_reaches_every_route(golden):
    """Both answers of the row-sum query occur for 1x1 and for 3x3 shapes, and hook value 2 (no FW form, no 32 x 32 blocks)
    turns every one of them off."""
    ks = [s[0] for s in golden['shapes']]
    auto = golden['select']['0']['rowsum_in_kernel']
    for k in (1, 3):
        assert {r for kk, r in zip(ks, auto) if kk == k} == {0, 1}
    assert not any(r for kk, r in zip(ks, auto) if kk > 3)
    assert not any(golden['select']['2']['rowsum_in_kernel'])


@pytest.mark.parametrize('select', [0, 1, 2])
def test_invalid_shapes_answer_zero(lib, select):
    try:
        assert lib.dvd_xwgrad_select(select) == 0
        for bad in [(0, 64, 64, 8, 8), (2, 0, 64, 8, 8), (2, 64, 0, 8, 8), (2, 64, 64, 0, 8), (2, 64, 64, 8, 0), (-1, 64, 64, 8, 8),
                    (2, 64, 64, 8, -8)]:
            assert lib.dvd_xwgrad1s_workspace_bytes(*bad) == 0
            assert lib.dvd_xwgrad3_workspace_bytes(*bad, 1) == 0
            assert lib.dvd_xwgradk_workspace_bytes(*bad, 5) == 0
            for KS in (1, 3, 5):
                assert lib.dvd_xwgrad_rowsum_in_kernel(*bad, KS, 1) == 0
        for G in (0, -2, 3, 5):                       # no groups, or groups that do not divide both channel counts
            assert lib.dvd_xwgrad3_workspace_bytes(2, 64, 96, 8, 8, G) == 0
            assert lib.dvd_xwgrad_rowsum_in_kernel(2, 64, 96, 8, 8, 3, G) == 0
        for KS in (0, 1, 2, 3, 4, 6, 9, 13, -5):      # the k x k query covers 5, 7 and 11
            assert lib.dvd_xwgradk_workspace_bytes(2, 32, 32, 16, 16, KS) == 0
        for KS in (5, 7, 11):
            assert lib.dvd_xwgradk_workspace_bytes(2, 32, 32, 16, 16, KS) > 0
            assert lib.dvd_xwgrad_rowsum_in_kernel(2, 32, 32, 16, 16, KS, 1) == 0
        assert lib.dvd_xwgrad_rowsum_in_kernel(2, 1024, 1024, 8, 8, 1, 32) == 0          # 1x1 is dense only
    finally:
        assert lib.dvd_xwgrad_select(0) == 0
