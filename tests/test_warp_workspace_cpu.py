"""CPU-only checks of the warp+loss host code: the workspace size both kernel generations ask for, against the values the
library returned before their two layouts were merged into one function (tests/golden/warp_workspace_bytes.json), and the
reserved third argument of dvd_warp_loss_select.  Nothing is launched: the plans only need the CU count, which is taken as
256 (the MI355X's) when no device is present."""
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'warp_workspace_bytes.json')
SHAPES = [(1, 2, 2), (2, 40, 67), (2, 48, 64), (2, 64, 100), (3, 96, 160), (2, 128, 192), (2, 160, 192), (3, 192, 288),
          (48, 384, 672)]
# the default hooks and every dvd_warp_loss_strip_select(rows, shape) setting of tests/test_00_warp_loss_gpu.py
STRIP_SELECT = {'default': (0, 0), 'rows64_shape0': (64, 0), 'rows32_shape1': (32, 1), 'shape2': (0, 2), 'shape3': (0, 3)}


@pytest.fixture
def lib():
    from dvd_hip import _lib
    lib = _lib.load()
    assert lib.dvd_warp_loss_select(0, -1, 0) == _lib.DVD_OK
    assert lib.dvd_warp_loss_strip_select(0, 0) == _lib.DVD_OK
    yield lib
    lib.dvd_warp_loss_select(0, -1, 0)
    lib.dvd_warp_loss_strip_select(0, 0)


def test_golden_file_covers_the_shapes_and_settings():
    gd = json.load(open(GOLDEN))
    assert [tuple(s) for s in gd['shapes']] == SHAPES
    assert {k: tuple(v) for k, v in gd['strip_select'].items()} == STRIP_SELECT
    assert set(gd['bytes']) == set(STRIP_SELECT) and all(len(v) == len(SHAPES) for v in gd['bytes'].values())


@pytest.mark.parametrize('setting', sorted(STRIP_SELECT))
def test_workspace_bytes_are_what_the_two_separate_layouts_gave(lib, setting):
    from dvd_hip import _lib
    gd = json.load(open(GOLDEN))
    rows, shape = STRIP_SELECT[setting]
    assert lib.dvd_warp_loss_strip_select(rows, shape) == _lib.DVD_OK
    got = [int(lib.dvd_warp_loss_workspace_bytes(*s)) for s in SHAPES]
    assert got == gd['bytes'][setting]


def test_third_argument_of_the_select_hook_is_reserved(lib):
    from dvd_hip import _lib
    assert lib.dvd_warp_loss_select(0, -1, 0) == _lib.DVD_OK
    for px in (2, 4):
        assert lib.dvd_warp_loss_select(0, -1, px) == _lib.DVD_EINVAL
        assert b'fixed by the tile shape' in lib.dvd_last_error()
    # the Python hook keeps `px` as the same reserved argument: 0 from an older caller is fine, anything else is refused
    from dvd_hip import ops
    ops.warp_loss_select(variant='tiles', tile=-1, px=0)
    ops.warp_loss_select()
    with pytest.raises(RuntimeError, match='fixed by the tile shape'):
        ops.warp_loss_select(px=4)
    # a rejected call changes nothing: the sizes are still those of the default hooks
    gd = json.load(open(GOLDEN))
    assert int(lib.dvd_warp_loss_workspace_bytes(*SHAPES[-1])) == gd['bytes']['default'][-1]
