"""dvd_ratio_median on the GPU (csrc/select.hip, ops.ratio_median) against numpy: bit for bit.

The yardstick is tests/depth_score_spec.py's median: fp32 quotients formed by numpy, then np.median per segment
(tests/test_depth_score_cpu.py shows that it equals the stated rule on every data class).  Compared with np.array_equal(...,
equal_nan=True), `count` exactly.  Data classes (depth_score_spec.median_cases), the smallest shapes at which a radix select can
go wrong: segment lengths 1, 2, 3, 4, 255, 256, 257, 1000, 4099 x 1, 3, 5 segments of random signed ratios; a mask that keeps
every other element; a segment without a selected element between two ordinary ones; all values equal; two distinct values;
values that share their top 24 bits; values that differ in the first digit only; the median duplicated across the middle (both
ranks in one bin on every pass); 70 000 equal values (a 16-bit bin counter would overflow); denormals; +0 / -0; +-inf with the
(-inf + inf) even case; a NaN numerator selected and masked out; den equal to den_min; a NaN denominator.

Beyond the launch cap (csrc/select.hip: kSelectMaxBlocks = 2048 blocks of 256 threads over all segments of a launch, a block
walks the rest of its segment grid-stride): the smallest segment at which every block makes a second trip and the last block's is
ragged -- one element per thread (odd L), one segment: L = 2048 * 256 + 2047 * 256 + 1 = 1 048 321; four elements per thread,
four segments of 512 blocks each: L = 512 * 1024 + 511 * 1024 + 4 = 1 047 556.

Also: two runs give equal bits; S segments in one call equal S one-segment calls; preprocess.calibrate_scale returns the scales
and the s the reference recorded for tests/golden/scale_calib.npz, exactly.
"""
import numpy as np
import pytest
import torch

import depth_score_spec as D
import helpers

pytestmark = pytest.mark.gpu

DEV = 'cuda'
CASES = D.median_cases()


def _run(num, den, mask, den_min):
    from dvd_hip import ops
    res = ops.ratio_median(helpers.t(num, DEV), helpers.t(den, DEV), None if mask is None else helpers.t(mask, DEV), den_min)
    assert res['median'].dtype == torch.float32 and res['count'].dtype == torch.int64 and res['median'].is_cuda
    return res['median'].cpu().numpy(), res['count'].cpu().numpy()


@pytest.mark.parametrize('case', CASES, ids=lambda c: c[0])
def test_median_equals_numpy_bit_for_bit(case):
    name, num, den, mask, den_min = case
    want, n = D.median(num, den, mask, den_min)
    got, count = _run(num, den, mask, den_min)
    assert got.shape == want.shape and np.array_equal(count, n), (name, count, n)
    assert np.array_equal(got, want, equal_nan=True), (name, got, want)
    # two runs give equal bits
    again, _ = _run(num, den, mask, den_min)
    assert again.tobytes() == got.tobytes(), name
    # S segments in one call equal S one-segment calls
    if num.shape[0] > 1:
        for s in range(num.shape[0]):
            one, c1 = _run(num[s:s + 1], den[s:s + 1], None if mask is None else mask[s:s + 1], den_min)
            assert one.tobytes() == got[s:s + 1].tobytes() and c1[0] == count[s], (name, s)


def test_views_into_a_buffer_take_the_scalar_path_and_agree():
    """The same data at a base two floats into its buffer (not 16-byte aligned: one element per thread) and at an aligned base
    (L % 4 == 0: four per thread) give the same bits."""
    from dvd_hip import ops
    name, num, den, mask, den_min = [c for c in CASES if c[0] == 'every_other'][0]
    S, L = num.shape
    want, n = D.median(num, den, mask, den_min)
    buf_n, buf_d = torch.zeros(S * L + 2, device=DEV), torch.zeros(S * L + 2, device=DEV)
    buf_m = torch.zeros(S * L + 3, device=DEV, dtype=torch.uint8)
    buf_n[2:].copy_(helpers.t(num, DEV).flatten()), buf_d[2:].copy_(helpers.t(den, DEV).flatten())
    buf_m[3:].copy_(helpers.t(mask, DEV).flatten())
    res = ops.ratio_median(buf_n[2:].view(S, L), buf_d[2:].view(S, L), buf_m[3:].view(S, L), den_min)
    assert np.array_equal(res['median'].cpu().numpy(), want) and np.array_equal(res['count'].cpu().numpy(), n)


@pytest.mark.parametrize('kind', sorted(D.BEYOND_CAP))
def test_beyond_the_launch_cap(kind):
    num, den = D.beyond_cap_case(kind)
    want, n = D.median(num, den, None, 0.0)
    got, count = _run(num, den, None, 0.0)
    assert np.array_equal(count, n) and np.array_equal(got, want, equal_nan=True), (kind, got, want, count, n)


def test_calibrate_scale_returns_the_references_scales():
    from dvd_hip import preprocess
    fx = helpers.load_golden('scale_calib')
    nn, mvs = helpers.t(fx['in_nn_depth'], DEV), helpers.t(fx['in_mvs_depth'], DEV)
    scales, s = preprocess.calibrate_scale(nn, mvs, thresh=float(fx['thresh']))
    assert scales.is_cuda and scales.dtype == torch.float32 and scales.shape == (5,)
    assert np.array_equal(scales.cpu().numpy(), fx['scales'])
    assert np.asarray(s).dtype == np.float32 and s == fx['s']
    scales4, s4 = preprocess.calibrate_scale(nn[:, None], mvs[:, None])                    # [N,1,H,W], the default threshold
    assert torch.equal(scales4, scales) and s4 == s
