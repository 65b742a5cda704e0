#!/usr/bin/env python
"""Measure the flow-chaining kernel (ops.flow_chain, preprocess.chain_flows; csrc/flow_chain.hip) on a synthetic store of
--frames frames at 384 x 672 that holds the gap-1 pairs only: gaps 2 to 8 are chained from them.  Prints one JSON line and,
with --out, writes it as a profile stamped with build.source_digest(('flow_chain.hip',)).

  kernel[gap]     median device-event ms of ONE dvd_flow_chain launch over --chains forward chains of that gap (L = gap links),
                  outputs preallocated, enqueued while the device is still busy clearing 4 GiB (the host wrapper's time is not in
                  the figure and the caches are cold); the algorithmic bytes the library counts for it (dvd_byte_counters, class
                  geometry: 9 B read per live link and pixel, 9 B written per row and pixel) and that rate next to the HBM peak
  chain_flows     the whole call for gaps 2 .. 8 (the plan on the host, both directions, the row picks, the consistency masks),
                  median ms, and the share of the composed pixels that stay usable

The store is tools/bench_frame_store.py's synthetic one with its random flows replaced by the geometric flow of
tools/bench_splat.py's smooth depth plus --noise px of noise and the consistency masks of those flows
(preprocess.flow_consistency_masks).  It is built with one frame more than asked for and then cut, because the writer's pair set
leaves out the last pair of a gap and a chain needs every link.  The feature has no counterpart before it, so no figure here is
a threshold.

    python tools/bench_flow_chain.py --out profiles/flow_chain.json

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
from bench_triangulate import geometric_flows  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=80)
    ap.add_argument('--height', type=int, default=384)
    ap.add_argument('--width', type=int, default=672)
    ap.add_argument('--gaps', type=str, default='2,3,4,5,6,7,8')
    ap.add_argument('--chains', type=int, default=32)
    ap.add_argument('--noise', type=float, default=0.1)
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    from dvd_hip import build, ops, preprocess
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    N, H, W = a.frames, a.height, a.width
    gaps = [int(g) for g in a.gaps.split(',')]
    store = synthetic_store(N + 1, H, W, [1], device)
    geometric_flows(store, smooth_depth(N + 1, H, W, device), a.noise)
    store.cat.frame_files = store.cat.frame_files[:N]                   # N frames and every gap-1 pair between them
    assert store.cat.pairs == [(f, f + 1) for f in range(N - 1)]
    m1, m2 = preprocess.flow_consistency_masks(store.flow_1_2, store.flow_2_1)
    store.mask_1.copy_(m1)
    store.mask_2.copy_(m2)
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
    for g in gaps:
        _, fwd, _ = preprocess.chain_plan(store.cat.pairs, N, [g])
        links = fwd[:a.chains]
        B, L = links.shape[:2]
        out = {'flow': torch.empty(L, B, H, W, 2, device=device), 'broken': torch.empty(L, B, H, W, device=device, dtype=torch.uint8)}

        def launch():
            ops.flow_chain(store.flow_1_2, store.flow_2_1, store.mask_1, store.mask_2, links, out=out)
        b0 = ops.flop_counters()['geometry']
        launch()
        nbytes = ops.flop_counters()['geometry'] - b0
        assert nbytes == float(H * W) * 9.0 * (2 * B * L)
        ms = timed(launch, head_start=True)
        t = statistics.median(ms)
        res[str(g)] = {'chains': B, 'links': L, 'ms': t, 'ms_min': min(ms), 'MB_algorithmic': nbytes / 1e6, 'GBps': nbytes / t / 1e6,
                       'frac_of_hbm_peak': nbytes / t / 1e6 / HBM_PEAK_GBPS, 'whole_share': float((out['broken'][L - 1] == 0).float().mean())}
        del out
    whole = timed(lambda: preprocess.chain_flows(store, gaps))
    chained = preprocess.chain_flows(store, gaps)
    line = json.dumps({
        'metric': 'flow_chain at %dx%d: %d frames, gaps %s chained from gap 1, %d new pairs' % (H, W, N, a.gaps, len(chained['pairs'])),
        'data': 'synthetic: geometric flow of a smooth depth with a step edge plus %.2f px of noise, consistency masks of those flows' % a.noise,
        'device': torch.cuda.get_device_name(device), 'source_digest': build.source_digest(('flow_chain.hip',)), 'reps': a.reps,
        'kernel': res, 'bytes_model': '9 B read per live link and pixel (flow 8, mask 1), 9 B written per row and pixel',
        'chain_flows_ms': statistics.median(whole), 'usable_share': float((chained['mask_2'] == 0).float().mean()),
        'timing_includes': 'kernel: the upload of the table and the launch, enqueued while the device clears 4 GiB in front of the first '
                           'event (the host wrapper does not hold the device up); chain_flows: everything, host included',
        'hbm_peak_GBps': HBM_PEAK_GBPS,
        'hbm_peak_allocated_GB': torch.cuda.max_memory_allocated(device) / 2 ** 30})
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
