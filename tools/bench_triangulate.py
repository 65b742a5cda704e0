#!/usr/bin/env python
"""Measure the triangulation kernel (ops.triangulate, preprocess.triangulate_depth; csrc/triangulate.hip) on a synthetic video of
--frames frames at 384 x 672 with flow pairs of gaps 1 to 4.  Prints one JSON line and, with --out, writes it as a profile
stamped with build.source_digest(('triangulate.hip',)).

  kernel[mode]        median device-event ms of the ONE dvd_triangulate launch over all frames (after a warm-up run), outputs
                      preallocated, the launch enqueued while the device is still busy clearing 4 GiB (so the host wrapper's
                      time is not in the figure and the caches are cold); the algorithmic bytes the library counts for it
                      (dvd_byte_counters, class geometry: 9 B per live observation and pixel, 14 B of outputs per pixel) and
                      that rate next to the 8 TB/s HBM3E peak
  triangulate_depth   the whole call (the plan on the host, allocation, the launch, the two boolean maps), median ms

The store is tools/bench_frame_store.py's synthetic one (the writer's pair set; cameras 0.05 along x and 0.01 rad about y per
frame) with its random flows replaced by the geometric flow of tools/bench_splat.py's smooth depth plus 0.3 px of noise, so that
most observations are consistent and the median has its samples to sort; 10 % of the mask bytes are set.  The feature has no
counterpart before it, so no figure here is a threshold.

    python tools/bench_triangulate.py --out profiles/triangulate.json

bench.py is not touched by this tool."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'dynamic-video-depth_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import torch  # noqa: E402

from bench_frame_store import synthetic_store  # noqa: E402
from bench_splat import HBM_PEAK_GBPS, smooth_depth  # noqa: E402


def geometric_flows(store, depth, noise, seed=7):
    """flow_1_2 / flow_2_1 of every pair from un-projecting with `depth` [N,1,H,W] and re-projecting (torch, set-up only)."""
    T, H, W, dev = store.tables, store.H, store.W, store.device
    g = torch.Generator(device=dev).manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing='ij')
    pix = torch.stack([x, y, torch.ones_like(x)], -1)

    def flow(a, b):
        world = (pix @ T['K_inv_T'][a] @ T['R_T'][a]) * depth[a, 0][..., None] + T['t'][a]
        q = (world - T['t'][b]) @ T['R'][b] @ T['K_T'][b]
        f = q[..., :2] / q[..., 2:] - pix[..., :2]
        return f + noise * torch.randn(f.shape, device=dev, generator=g)

    for j, (a, b) in enumerate(store.cat.pairs):
        store.flow_1_2[j].copy_(flow(a, b))
        store.flow_2_1[j].copy_(flow(b, a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=80)
    ap.add_argument('--height', type=int, default=384)
    ap.add_argument('--width', type=int, default=672)
    ap.add_argument('--gaps', type=str, default='1,2,3,4')
    ap.add_argument('--noise', type=float, default=0.3)
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    from dvd_hip import build, ops, preprocess
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    N, H, W = a.frames, a.height, a.width
    gaps = [int(g) for g in a.gaps.split(',')]
    store = synthetic_store(N, H, W, gaps, device)
    geometric_flows(store, smooth_depth(N, H, W, device), a.noise)
    frames, obs = preprocess.triangulate_plan(store.cat.pairs, N)
    live = int((obs[..., 0] >= 0).sum())
    out = {k: torch.empty((N, 1, H, W) if chan else (N, H, W), device=device, dtype=dt) for k, dt, chan in ops.TRI_OUT}

    ballast = torch.empty(1 << 30, device=device, dtype=torch.uint8)

    def timed(fn, head_start=False):
        fn()                                                       # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if head_start:                                         # device work in front of the first event: the host wrapper's time
                for _ in range(4):                                 # is spent while the device is still busy, and the caches are cold
                    ballast.zero_()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    res = {}
    for mode in ('mean', 'median'):
        def launch():
            ops.triangulate(store.flow_1_2, store.flow_2_1, store.mask_1, store.mask_2, obs, frames, store.tables, mode=mode, out=out)
        b0 = ops.flop_counters()['geometry']
        launch()
        nbytes = ops.flop_counters()['geometry'] - b0
        assert nbytes == float(H * W) * (9.0 * live + 14.0 * N)
        ms = timed(launch, head_start=True)
        t = statistics.median(ms)
        whole = timed(lambda: preprocess.triangulate_depth(store, mode=mode))
        res[mode] = {'ms': t, 'ms_min': min(ms), 'MB_algorithmic': nbytes / 1e6, 'GBps': nbytes / t / 1e6,
                     'frac_of_hbm_peak': nbytes / t / 1e6 / HBM_PEAK_GBPS,
                     'triangulate_depth_ms': statistics.median(whole),
                     'static_share': float((out['count'] >= 2).float().mean()), 'mean_count': float(out['count'].float().mean()),
                     'mean_usable': float(out['usable'].float().mean())}
    line = json.dumps({
        'metric': 'triangulate at %dx%d: %d frames, gaps %s, %d pairs, %d live observations (M = %d)' % (
            H, W, N, a.gaps, len(store.cat.pairs), live, obs.shape[1]),
        'data': 'synthetic: geometric flow of a smooth depth with a step edge plus %.2f px of noise, 10 %% of the mask bytes set' % a.noise,
        'device': torch.cuda.get_device_name(device), 'source_digest': build.source_digest(('triangulate.hip',)), 'reps': a.reps,
        'kernel': res, 'bytes_model': '9 B per live observation and pixel (flow 8, mask 1), 14 B of outputs per pixel',
        'timing_includes': 'kernel: the upload of the table and the launch, enqueued while the device clears 4 GiB in front of the first '
                           'event (the host wrapper does not hold the device up); triangulate_depth: everything, host included',
        'hbm_peak_GBps': HBM_PEAK_GBPS,
        'hbm_peak_allocated_GB': torch.cuda.max_memory_allocated(device) / 2 ** 30})
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
