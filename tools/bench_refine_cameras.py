#!/usr/bin/env python
"""Measure the camera refinement (ops.pose_normal_eq, preprocess.refine_cameras; csrc/pose.hip) on a synthetic video of --frames
frames at 384 x 672 with flow pairs of gaps 1 to 4 (tools/bench_triangulate.py's size).  Prints one JSON line and, with --out,
writes it as a profile stamped with build.source_digest(('pose.hip',)).

  evaluation       median device-event ms of ONE evaluation of the normal equations over all rows (the dvd_pose_normal_eq
                   launch and its small sum kernel, after a warm-up run), outputs preallocated, enqueued while the device is
                   still busy clearing 4 GiB (so the host wrapper's time is not in the figure and the caches are cold); the
                   algorithmic bytes rows * H W * (8 flow + 1 mask + 4 depth + 4 weight), which is what the library counts
                   (dvd_byte_counters, class geometry), and that rate next to the 8 TB/s HBM3E peak
  refine_cameras   the whole call from cameras perturbed by --deg degrees and --shift: wall ms, iterations, accepted steps, the
                   cost after each, and `to_floor`, the iterations after which the cost stays within 1 % of its last value

The store is tools/bench_frame_store.py's synthetic one with its random flows replaced by the geometric flow of
tools/bench_splat.py's smooth depth (which is also the store's depth_pred) plus --noise px of noise; 10 % of the mask bytes are
set; the weight is all ones (it is read all the same).  The feature has no counterpart before it, so no figure here is a
threshold.

    python tools/bench_refine_cameras.py --out profiles/pose.json

bench.py is not touched by this tool."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'dynamic-video-depth_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_frame_store import synthetic_store  # noqa: E402
from bench_splat import HBM_PEAK_GBPS, smooth_depth  # noqa: E402
from bench_triangulate import geometric_flows  # noqa: E402


def perturbed_tables(store, deg, shift, seed=5):
    """The store's tables with every frame but the first turned by Exp(deg * U(-1,1)^3) and moved by shift * U(-1,1)^3."""
    from dvd_hip.datasets.frame_store import camera_tables
    from dvd_hip.preprocess import _exp_so3
    rng = np.random.default_rng(seed)
    poses = store.host_tables['cam_c2w'].numpy().astype(np.float64)
    for f in range(1, len(poses)):
        poses[f, :3, :3] = poses[f, :3, :3] @ _exp_so3(np.deg2rad(deg) * rng.uniform(-1, 1, 3))
        poses[f, :3, 3] += shift * rng.uniform(-1, 1, 3)
    return {k: v.to(store.device) for k, v in camera_tables(store.host_tables, poses).items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=80)
    ap.add_argument('--height', type=int, default=384)
    ap.add_argument('--width', type=int, default=672)
    ap.add_argument('--gaps', type=str, default='1,2,3,4')
    ap.add_argument('--noise', type=float, default=0.3)
    ap.add_argument('--deg', type=float, default=0.5)
    ap.add_argument('--shift', type=float, default=0.02)
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    from dvd_hip import build, ops, preprocess
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    N, H, W = a.frames, a.height, a.width
    gaps = [int(g) for g in a.gaps.split(',')]
    store = synthetic_store(N, H, W, gaps, device)
    store.depth_pred.copy_(smooth_depth(N, H, W, device))
    geometric_flows(store, store.depth_pred, a.noise)
    rows = preprocess.refine_plan(store.cat.pairs, N)
    R = len(rows)
    weight = torch.ones(N, H, W, device=device)
    start = perturbed_tables(store, a.deg, a.shift)
    out = {'sums': torch.empty(R, ops.POSE_SUMS, device=device, dtype=torch.float64), 'wsum': torch.empty(R, device=device, dtype=torch.float64),
           'counts': torch.empty(R, 2, device=device, dtype=torch.int64)}
    ballast = torch.empty(1 << 30, device=device, dtype=torch.uint8)

    def launch():
        ops.pose_normal_eq(store.flow_1_2, store.flow_2_1, store.mask_1, store.mask_2, store.depth_pred, weight, rows, start, None,
                           1.0, 1e-3, out=out)

    b0 = ops.flop_counters()['geometry']
    launch()
    nbytes = ops.flop_counters()['geometry'] - b0
    assert nbytes == float(R) * H * W * 17.0
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(4):                                         # device work in front of the first event: the host wrapper's
            ballast.zero_()                                        # time is spent while the device is busy; the caches are cold
        e0.record()
        launch()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    t = statistics.median(ms)
    counts = out['counts'].cpu().numpy()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ref = preprocess.refine_cameras(store, weight=weight, tables=start)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    cost = ref['cost']
    to_floor = next(i for i, c in enumerate(cost) if all(abs(v - cost[-1]) <= 0.01 * cost[-1] for v in cost[i:]))
    true = store.host_tables['cam_c2w'].numpy().astype(np.float64)
    got, first = ref['poses'].numpy().astype(np.float64), start['cam_c2w'].cpu().numpy().astype(np.float64)
    seen = sorted(set(rows[:, 1:3].ravel().tolist()))                 # (the writer's pair set leaves the last frame without a pair)
    err = lambda p: [float(max(np.linalg.norm(p[f, :3, :3] - true[f, :3, :3]) for f in seen)),
                     float(max(np.linalg.norm(p[f, :3, 3] - true[f, :3, 3]) for f in seen))]
    line = json.dumps({
        'metric': 'refine_cameras at %dx%d: %d frames, gaps %s, %d pairs, %d rows' % (H, W, N, a.gaps, len(store.cat.pairs), R),
        'data': 'synthetic: geometric flow of a smooth depth with a step edge plus %.2f px of noise, 10 %% of the mask bytes set; cameras '
                'perturbed by %.2f degrees and %.3f' % (a.noise, a.deg, a.shift),
        'device': torch.cuda.get_device_name(device), 'source_digest': build.source_digest(('pose.hip',)), 'reps': a.reps,
        'evaluation': {'ms': t, 'ms_min': min(ms), 'MB_algorithmic': nbytes / 1e6, 'GBps': nbytes / t / 1e6,
                       'frac_of_hbm_peak': nbytes / t / 1e6 / HBM_PEAK_GBPS, 'live_share': float(counts[:, 0].sum()) / (R * H * W),
                       'workspace_MB': ops._lib.load().dvd_pose_workspace_bytes(R, H, W) / 1e6},
        'refine_cameras': {'wall_ms': wall, 'iterations': ref['iterations'], 'accepted': ref['accepted'], 'converged': ref['converged'],
                           'to_floor': to_floor, 'cost': cost, 'frames_with_a_pair': len(seen), 'error_R_c_before': err(first), 'error_R_c_after': err(got),
                           'rms_before_px': float(ref['rms_before'].mean()), 'rms_after_px': float(ref['rms_after'].mean())},
        'bytes_model': '17 B per row and pixel (flow 8, mask 1, depth 4, weight 4)',
        'timing_includes': 'evaluation: the upload of the rows, the launch and the sum kernel, enqueued while the device clears 4 GiB in '
                           'front of the first event; refine_cameras: everything, host included',
        'hbm_peak_GBps': HBM_PEAK_GBPS, 'hbm_peak_allocated_GB': torch.cuda.max_memory_allocated(device) / 2 ** 30})
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
