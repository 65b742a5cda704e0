"""Host-side geometry of the scene-flow MLP kernels (csrc/sf_mlp.hip: make_geometry, make_pack_layout, the stash layouts)
for every input layer the GPU sweep of tests/test_02b_sf_mlp_geometry_gpu.py runs: the input channel count and the sizes of
the packed-weight buffer and of the two stashes, restated here from the layout comments of the kernels' source.  The size
functions are host-only: no GPU, no launch."""
import ctypes

import pytest

GEOMETRIES = [(16, 16, False), (0, 0, False), (2, 0, True), (4, 2, True), (12, 10, True), (16, 0, True), (20, 20, True),
              (16, 16, True)]
# c_in, c_in16, K steps of layer 0, row tiles of W_0^T -- the table of the sweep
EXPECTED = {(16, 16, False): (99, 112, 7, 4), (0, 0, False): (3, 16, 1, 1), (2, 0, True): (16, 16, 1, 1),
            (4, 2, True): (32, 32, 2, 1), (12, 10, True): (96, 96, 6, 3), (16, 0, True): (100, 112, 7, 4),
            (20, 20, True): (164, 176, 11, 6), (16, 16, True): (132, 144, 9, 5)}
WIDTH, TILE, HIDDEN, DW_SLICES = 256, 64, 5, 51


def _shape(nx, nt, td):
    c_in = 3 + 6 * nx + ((1 + 2 * nt) if td else 0)
    c_in16 = -(-c_in // 16) * 16
    return c_in, c_in16, c_in16 // 16, -(-c_in // 32)


def _packed_floats(ks0, rt0):
    units = 0                                     # 16-byte units: [(row tile, K step, term)][64 lanes]
    for layer in range(HIDDEN):
        nk, rtb = (ks0, rt0) if layer == 0 else (WIDTH // 16, WIDTH // 32)
        units += 8 * nk * 2 * 64                  # forward orientation: 8 row tiles of 32 outputs
        units += rtb * 16 * 2 * 64                # backward orientation: 16 K steps over the 256 outputs
    return units * 4 + 3 * WIDTH + HIDDEN * WIDTH + 4 + 8      # + W_5, the biases (the last padded to 4), max|W_l|


def _stash_floats(c_in16, n_pix, f16):
    tiles = -(-n_pix // TILE)
    per_tile = c_in16 * TILE + HIDDEN * (WIDTH * TILE // (2 if f16 else 1)) + HIDDEN * 512
    return tiles * per_tile + 16


def _gstash_floats(n_pix):
    tiles = -(-n_pix // TILE)
    return tiles * HIDDEN * WIDTH * TILE + HIDDEN * DW_SLICES * (WIDTH * WIDTH + WIDTH)


@pytest.mark.parametrize('geom', GEOMETRIES, ids=lambda g: 'x%d_t%d_%s' % (g[0], g[1], 'T' if g[2] else 'F'))
def test_sizes_follow_the_documented_layouts(geom):
    from dvd_hip import _lib
    from oracle import sceneflow_mlp as M
    lib = _lib.load()
    nx, nt, td = geom
    c_in, c_in16, ks0, rt0 = _shape(nx, nt, td)
    assert (c_in, c_in16, ks0, rt0) == EXPECTED[geom]
    assert M.layer_dims(n_freq_xyz=nx, n_freq_t=nt, time_dependent=td)[0] == c_in
    for f16 in (0, 1):
        desc = _lib.MlpDesc(nx, nt, int(td), 0, 0, f16, 0)         # (the size functions do not read the frequency tables)
        assert lib.dvd_sf_mlp_in_channels(ctypes.byref(desc)) == c_in
        assert lib.dvd_sf_mlp_packed_bytes(ctypes.byref(desc)) == 4 * _packed_floats(ks0, rt0)
        for n_pix in (1, 64, 65, 3 * 17 * 23, 2 * 24 * 40, 3 * 96 * 115):
            assert lib.dvd_sf_mlp_stash_bytes(ctypes.byref(desc), n_pix) == 4 * _stash_floats(c_in16, n_pix, bool(f16)), (f16, n_pix)
            assert lib.dvd_sf_mlp_gstash_bytes(n_pix) == 4 * _gstash_floats(n_pix)


def test_time_independent_geometry_ignores_the_time_frequencies():
    from dvd_hip import _lib
    lib = _lib.load()
    a, b = _lib.MlpDesc(16, 16, 0, 0, 0, 0, 0), _lib.MlpDesc(16, 0, 0, 0, 0, 0, 0)
    assert lib.dvd_sf_mlp_in_channels(ctypes.byref(a)) == lib.dvd_sf_mlp_in_channels(ctypes.byref(b)) == 99
    assert lib.dvd_sf_mlp_packed_bytes(ctypes.byref(a)) == lib.dvd_sf_mlp_packed_bytes(ctypes.byref(b))
