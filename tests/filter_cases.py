"""Inputs shared by the temporal-filter tests (tests/test_filter_cpu.py, test_59_track_filter_gpu.py, test_60_filter_depth_gpu.py),
so that the condition the CPU test checks on the reference -- at most 2 % of the pixels have a sample whose gate hangs on the
last bits -- is checked on exactly what the GPU tests run."""
import numpy as np
import torch

FX = 'tracks_b3_11x21_t4'
START, RADIUS = [1, 3, 6], 3
TOL, Z_NEAR = 0.1, 1e-3
# The fixture's depth is white noise in 1 .. 6: neighbouring frames disagree by a factor of up to 6 and nearly every sample
# fails the gates.  Its variation about 3.5 is scaled down to +-4.4 %, inside tol = 0.1 for most samples and outside for some.
DEPTH_MID, DEPTH_SCALE = 3.5, 0.035


def e2e_depth(fx):
    """[N,1,H,W] fp32: the fixture's depth with its variation about DEPTH_MID scaled by DEPTH_SCALE."""
    d = fx['in_depth'].astype(np.float64)
    return (DEPTH_MID + DEPTH_SCALE * (d - DEPTH_MID)).astype(np.float32)


def tables(fx):
    return {k: fx['tab_' + k] for k in ('R_T', 'K_inv_T', 'R', 't', 'K_T')}


def time_stamps(fx, start, time_dependent):
    H, W, B = int(fx['H']), int(fx['W']), len(start)
    return torch.from_numpy(fx['tab_ts_vali'])[start].view(B, 1, 1, 1).expand(B, 1, H, W) if time_dependent else None


def surface(H, W):
    """A smooth positive surface S(x, y) [H,W] float64 for the constructed static videos."""
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    return 3.0 + 0.5 * np.sin(0.31 * xx + 0.2) * np.cos(0.23 * yy) + 0.02 * xx


def frame_scales(n):
    """c_g, one per frame, spread by +-4.5 % about 1 in a fixed irregular order: the largest ratio of two of them is 1.094,
    so with tol = 0.1 no frame gates another out (at +-5 % the extremes, 1.05 / 0.95 = 1.105, would)."""
    base = np.array([0.97, 1.045, 0.955, 1.02, 1.04, 0.96, 1.01, 0.98, 1.03, 0.99], dtype=np.float64)
    return base[np.arange(n) % len(base)]


def static_video(n, H, W):
    """depth [n,1,H,W] fp32 = S * c_g, and (S, c) in float64."""
    S, c = surface(H, W), frame_scales(n)
    return (S[None, None] * c[:, None, None, None]).astype(np.float32), S, c
