"""CPU-only checks of the track evaluation (csrc/eval.hip, ops.eval_tracks) and of Model.evaluate's host half
(models/evaluate.py): the C entry exists, is declared, and refuses bad arguments before any HIP call; the fixed-point shift
with its overflow argument restated as arithmetic; evaluate_plan on catalogues with gaps [1] and [1, 2]; the float64
specification (tests/eval_spec.py) on cases whose answer is known -- plus the condition every GPU comparison rests on: under the
specification alone, at most 1 % of the live points of every input set the GPU tests use are fragile."""
import ctypes
import os

import numpy as np
import pytest
import torch

import eval_spec as E
import helpers
import store_spec
import tracks_spec as S


def _lib():
    from dvd_hip import _lib
    return _lib, _lib.load()


def _err(lib):
    return lib.dvd_last_error().decode()


P = ctypes.c_void_p(64)      # a non-null pointer that is never followed: every call below is refused before any HIP call


def _eval(lib, **over):
    a = dict(points=P, source=P, k_first=1, R=P, t=P, K_T=P, N=5, depth_all=P, img_all=P, pair_row=P, flow=P, mask=P, P=6,
             z_tol=0.05, d_min=1e-3, shift=32, sums=P, sums_stride=18, maps=P, maps_stride=3 * 3 * 11 * 21, T=3, B=3, H=11, W=21)
    a.update(over)
    return lib.dvd_eval_tracks(a['points'], a['source'], a['k_first'], a['R'], a['t'], a['K_T'], a['N'], a['depth_all'],
                               a['img_all'], a['pair_row'], a['flow'], a['mask'], a['P'], a['z_tol'], a['d_min'], a['shift'],
                               a['sums'], a['sums_stride'], a['maps'], a['maps_stride'], a['T'], a['B'], a['H'], a['W'], None)


def test_the_symbol_exists_is_declared_and_refuses_bad_arguments():
    _l, lib = _lib()
    assert 'dvd_eval_tracks' in _l.SIGNATURES and hasattr(lib, 'dvd_eval_tracks')
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dvd_hip.h')).read()
    assert 'int dvd_eval_tracks(const float* points, const int* source, int k_first,' in header
    assert '#define DVD_ABI_VERSION 8' in header
    nan = float('nan')
    bad = [dict(points=None), dict(source=None), dict(R=None), dict(t=None), dict(K_T=None), dict(depth_all=None),
           dict(img_all=None), dict(sums=None),
           dict(pair_row=None), dict(flow=None), dict(mask=None), dict(pair_row=None, flow=None), dict(flow=None, mask=None),
           dict(pair_row=None, mask=None),
           dict(T=0), dict(T=65536), dict(B=0), dict(B=65536), dict(T=-1), dict(N=0),
           dict(H=1), dict(W=1), dict(H=32768, W=32768, shift=22), dict(H=1 << 15, W=1 << 16, shift=1),
           dict(k_first=2), dict(k_first=-1),
           dict(z_tol=-0.01), dict(z_tol=nan), dict(d_min=0.0), dict(d_min=-1.0), dict(d_min=nan),
           dict(shift=0), dict(shift=33), dict(shift=-4), dict(H=1024, W=1025, shift=32, maps=None),
           dict(sums_stride=17), dict(maps_stride=3 * 3 * 11 * 21 - 1)]
    for over in bad:
        assert _eval(lib, **over) == _l.DVD_EINVAL, over
        assert 'eval_tracks' in _err(lib), over
    assert _eval(lib, points=None) == _l.DVD_EINVAL and 'null' in _err(lib)
    assert _eval(lib, mask=None) == _l.DVD_EINVAL and 'all three or none' in _err(lib)


def test_ops_eval_tracks_refuses_cpu_tensors_and_lists_its_kernel():
    from dvd_hip import ops
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ops.eval_tracks(torch.zeros(1, 1, 3, 4, 4), [0], {}, torch.zeros(2, 1, 4, 4), torch.zeros(2, 3, 4, 4))
    assert 'eval_tracks_kernel' in ops.BYTE_CLASS_KERNELS['geometry']
    from dvd_hip import build
    assert ('eval.hip', ['-ffp-contract=off']) in build.SOURCES


def test_shift_rule_keeps_a_row_of_capped_terms_below_2_to_62():
    from dvd_hip import ops
    _l, lib = _lib()
    for H, W in ((2, 2), (11, 21), (17, 19), (12, 24), (36, 40), (384, 672), (1024, 1024), (1024, 1025), (2048, 2048),
                 (4096, 4096), (16384, 32768), (32767, 32768)):
        n = H * W
        shift = ops.eval_shift(n)
        assert shift == E.shift_for(n) == min(32, 62 - 10 - E.ceil_log2(n))
        assert 1 <= shift <= 32
        # n terms of at most CAP = 2^10, each rounded to an integer of at most 2^10 * 2^shift: exact Python integers
        assert n * (1 << 10) * (1 << shift) <= 1 << 62, (H, W)
        if n < (1 << 30) and shift < 32:
            # the entry refuses the next larger shift where the formula, not the cap of 32, is the limit ...
            assert _eval(lib, H=H, W=W, shift=shift + 1, maps=None) == _l.DVD_EINVAL and 'shift' in _err(lib)
    assert ops.eval_shift(384 * 672) == 32 and ops.eval_shift(1 << 20) == 32 and ops.eval_shift((1 << 20) + 1) == 31
    with pytest.raises(RuntimeError):
        ops.eval_shift(0)


def _catalogue(root, n_frames, gaps):
    from dvd_hip.datasets.frame_store import Catalogue
    store_spec.write_tree(root, store_spec.random_tree(n_frames, 4, 6, gaps, 1))
    return Catalogue(root, store_spec.TRACK, gaps)


def test_evaluate_plan(tmp_path):
    from dvd_hip.models.evaluate import evaluate_plan
    one = _catalogue(str(tmp_path / 'one'), 6, [1])
    assert one.pairs == [(0, 1), (1, 2), (2, 3), (3, 4)]                      # the writer leaves out (4, 5)
    valid, table = evaluate_plan(one, [0, 3, 4, 5], 2)
    assert valid == [2, 2, 1, 0] and table.dtype == np.int32 and table.shape == (2, 4)
    assert table.tolist() == [[0, 3, -1, -1], [-1, -1, -1, -1]]              # (4, 5) omitted; no gap 2 in this catalogue
    two = _catalogue(str(tmp_path / 'two'), 6, [1, 2])
    assert two.pairs == [(0, 1), (1, 2), (2, 3), (3, 4), (0, 2), (1, 3), (2, 4)]
    valid, table = evaluate_plan(two, [0, 2, 3, 4], 3)
    assert valid == [3, 3, 2, 1]
    assert table.tolist() == [[0, 2, 3, -1], [4, 6, -1, -1], [-1, -1, -1, -1]]      # (3, 5) and (4, 5) omitted; no gap 3
    assert evaluate_plan(two, torch.tensor([1]), 1)[1].tolist() == [[1]]
    valid, table = evaluate_plan(two, np.array([5]), 2)                        # the last frame has nowhere to go
    assert valid == [0] and table.tolist() == [[-1], [-1]]
    for start, n_steps in (([], 1), ([6], 1), ([-1], 1), ([1.5], 1), ([0], 0), ([0], 1.0), ([True], 1)):
        with pytest.raises(ValueError, match='track_plan'):
            evaluate_plan(two, start, n_steps)


def _static_case(H=9, W=13):
    """Two frames with one camera, one smooth depth and one image; the points of frame 0 looked at in frame 1."""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    depth = np.tile((3.0 + 0.3 * np.sin(0.4 * xx) + 0.2 * np.cos(0.3 * yy)).astype(np.float32), (2, 1, 1, 1))
    img = np.tile(np.stack([0.5 + 0.4 * np.sin(0.3 * (c + 1) * xx + 0.2 * yy) for c in range(3)]).astype(np.float32), (2, 1, 1, 1))
    poses = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    K = np.tile(np.array([[0.9 * W, 0, (W - 1) / 2.0], [0, 0.9 * W, (H - 1) / 2.0], [0, 0, 1.0]], dtype=np.float32), (2, 1, 1))
    tab = E.camera_tables(poses, K)
    p0 = S.unproject(depth[:1], tab['R_T'][:1], tab['t'][:1], tab['K_inv_T'][:1])
    return {'points': p0[None].float().numpy(), 'source': [0], 'k_first': 1, 'R': tab['R'], 't': tab['t'], 'K_T': tab['K_T'],
            'depth_all': depth, 'img_all': img, 'H': H, 'W': W}


def _run(case, **kw):
    kw = dict(kw)
    pairs = kw.pop('pairs', None)
    return E.evaluate(case['points'], case['source'], case['k_first'], case['R'], case['t'], case['K_T'], case['depth_all'],
                      case['img_all'], pairs=pairs, **kw)


def test_spec_identical_frames_and_one_camera_agree_with_themselves():
    case = _static_case()
    H, W = case['H'], case['W']
    res = _run(case)
    rel, photo = res['maps'][0, 0, 0], res['maps'][0, 0, 1]
    inner = ~S.border_pixels(H, W)
    assert bool((rel[inner] >= 0).all()) and bool((photo[inner] >= 0).all()) and not bool(res['occluded'].any())
    assert float(rel[rel >= 0].max()) < 1e-6 and float(photo[photo >= 0].max()) < 1e-6
    assert bool((res['maps'][0, 0, 2] == -1).all())                         # no pairs: epe counts nowhere
    n_in, n_occ, s_rel, s_photo, n_flow, s_epe = res['sums'][0][0]
    assert n_in >= (H - 2) * (W - 2) and (n_occ, n_flow, s_epe) == (0, 0, 0)
    assert s_rel <= n_in * 1e-6 * 2 ** res['shift'] and s_photo <= n_in * 1e-6 * 2 ** res['shift']


def test_spec_a_point_behind_the_target_surface_is_occluded_and_counts_in_nothing_else():
    case = _static_case()
    H, W = case['H'], case['W']
    pts = torch.from_numpy(case['points']).double()
    deep = torch.zeros(H, W, dtype=torch.bool)
    deep[2:5, 3:8] = True
    pts[0, 0][:, deep] *= 1.2            # the camera sits at the origin: along the ray, 20 % deeper, beyond z_tol = 5 %
    res = _run(dict(case, points=pts.float().numpy()))
    assert bool(res['occluded'][0, 0][deep].all()) and int(res['occluded'].sum()) == int(deep.sum())
    assert bool((res['maps'][0, 0, :, deep] == -1).all())
    assert res['sums'][0][0][1] == int(deep.sum()) and res['sums'][0][0][0] >= int(deep.sum())
    assert float(res['maps'][0, 0, 0][~deep].max()) < 1e-6
    within = _run(dict(case, points=pts.float().numpy()), z_tol=0.25)       # a wider tolerance sees them: rel = 0.2
    assert not bool(within['occluded'].any())
    np.testing.assert_allclose(within['maps'][0, 0, 0][deep].numpy(), 0.2, atol=1e-5)
    # ... and nearer than the surface is never occluded, whatever the distance
    pts[0, 0][:, deep] *= 0.5 / 1.2
    near = _run(dict(case, points=pts.float().numpy()))
    assert not bool(near['occluded'].any())
    np.testing.assert_allclose(near['maps'][0, 0, 0][deep].numpy(), 0.5, atol=1e-5)


def test_spec_flow_equal_to_the_true_displacement_has_no_error_and_a_masked_pixel_does_not_count():
    case = _static_case()
    H, W = case['H'], case['W']
    pts = torch.from_numpy(case['points']).double()
    pts[0, 0, 0] += 0.1                  # the scene moved to the right
    pts[0, 0, 2, 0, 0] = -1.0            # one point behind the camera
    case = dict(case, points=pts.float().numpy())
    plain = _run(case)
    xx, yy = S._pixel_grid(H, W)
    flow = torch.stack([plain['uv'][0, 0, ..., 0] - xx, plain['uv'][0, 0, ..., 1] - yy], -1)[None].float().numpy()
    mask = np.zeros((1, H, W), dtype=np.uint8)
    mask[0, 4, 5], mask[0, 1, 1] = 1, 255
    res = _run(case, pairs=([[0]], flow, mask))
    epe = res['maps'][0, 0, 2]
    assert float(epe[4, 5]) == -1 and float(epe[1, 1]) == -1 and float(epe[0, 0]) == -1
    counted = epe >= 0
    assert int(counted.sum()) == H * W - 3 == res['sums'][0][0][4]
    assert float(epe[counted].max()) < 1e-5
    # epe does not ask for `inside`: points that left the image on the right still count
    assert bool((counted & ~res['inside'][0, 0]).any())
    off = _run(case, pairs=([[0]], flow + np.array([3.0, 4.0], dtype=np.float32), mask))
    np.testing.assert_allclose(off['maps'][0, 0, 2][counted].numpy(), 5.0, atol=1e-4)
    assert bool((_run(case, pairs=([[-1]], flow, mask))['maps'][0, 0, 2] == -1).all())
    far = _run(case, pairs=([[0]], flow + np.float32(5000.0), mask))        # capped
    assert float(far['maps'][0, 0, 2].max()) == E.CAP


def _sd(fx):
    from dvd_hip.networks.sceneflow_field import SceneFlowFieldNet
    net = SceneFlowFieldNet(net_width=256, n_layers=4, time_dependent=True, N_freq_xyz=16, N_freq_t=16)
    helpers.seeded_fill_(net, int(fx['seed']))                               # the network of tests/test_45 and test_52
    return {k: v.detach() for k, v in net.state_dict().items()}


def _report(name, r64, r32):
    share = E.fragile_share(r64)
    live = r64['live'][:, :, None, None].expand_as(r64['fragile'])
    seen = (r64['maps'][:, :, 0] >= 0)
    print('%s: %.2f %% fragile; of the live points %.0f %% inside, %.0f %% occluded, %.0f %% with flow' % (
        name, 100 * share, 100 * float(r64['inside'][live].double().mean()), 100 * float(r64['occluded'][live].double().mean()),
        100 * float((r64['maps'][:, :, 2] >= 0)[live].double().mean())))
    assert share <= E.FRAGILE_CAP
    # outside the fragile set fp32 and float64 agree about what counts: the yardstick of the GPU tests is defined
    assert not (((r64['maps'] >= 0) != (r32['maps'] >= 0)) & ~r64['fragile'][:, :, None]).any()
    return seen, live


@pytest.mark.parametrize('k_first', (0, 1))
@pytest.mark.parametrize('shape', E.KERNEL_SHAPES)
def test_fragile_share_of_the_kernel_cases_is_within_the_cap(shape, k_first):
    case = E.kernel_case(shape[0], shape[1], k_first)
    r64, r32 = E.run_case(case), E.run_case(case, dtype=torch.float32)
    seen, live = _report('%dx%d k_first=%d' % (shape + (k_first,)), r64, r32)
    # the case exercises every branch: seen, occluded, outside, behind, with and without flow, a dead row
    assert bool(seen.any()) and bool(r64['occluded'].any()) and bool((~r64['inside'] & live).any())
    assert bool((~r64['front'] & live).any()) and bool((r64['maps'][:, :, 2] >= 0).any())
    assert not bool(r64['live'].all()) and bool(r64['live'][:, :2].all())
    assert float(r64['occluded'][live].double().mean()) > 0.02 and float(seen[live].double().mean()) > 0.4
    assert (case['pair_row'] >= 0).any() and (case['pair_row'][case['pair_row'].shape[0] - 1] == -1).any()


def test_fragile_share_of_the_pipeline_case_is_within_the_cap():
    fx = helpers.load_golden(E.PIPE_FX)
    case = E.pipeline_case(fx, _sd(fx))
    assert case['steps_valid'] == [4, 3, 1]
    assert case['pair_row'].tolist() == [[0, 3, -1], [5, 8, -1], [-1, -1, -1], [-1, -1, -1]]
    r64, r32 = E.run_case(case), E.run_case(case, dtype=torch.float32)
    seen, live = _report('pipeline', r64, r32)
    assert bool(seen.any()) and r64['live'].tolist() == [[v >= k for v in (4, 3, 1)] for k in range(1, 5)]
