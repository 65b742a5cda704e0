#!/usr/bin/env python
"""Measure the render path (ops.splat, Model.render; csrc/splat.hip, dvd_hip/models/render.py) on a synthetic video at
384 x 672: --views views, each drawn from --sources earlier frames advected to the view's time.  Prints one JSON line and, with
--out, writes it as a profile stamped with build.source_digest(('splat.hip',)).

  zmin / accumulate / resolve   median device-event ms of each of the three launches over the final world points of all sources,
                                the algorithmic bytes the library counts for the launch (dvd_byte_counters, class geometry:
                                points, values and the outputs once, 4 taps per point with 4 B per atomicMin and 8 B per 64-bit
                                atomicAdd) and that rate next to the 8 TB/s HBM3E peak
  clears                        median ms of the two workspace clears
  render                        median device-event ms of the whole Model.render call: the store's gathers, ops.unproject, the
                                Euler chain of the MLP, the clears and the three launches

The depth is smooth with a step edge (random depth would scatter every point to an unrelated pixel, which no video does).  The
feature has no counterpart before it, so no figure here is a threshold.

    python tools/bench_splat.py --out profiles/splat.json

bench.py is not touched by this tool; model and options come from its make_opt / build_model, the store from
tools/bench_frame_store.py's synthetic_store."""
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

import bench  # noqa: E402
from bench_frame_store import synthetic_store  # noqa: E402

HBM_PEAK_GBPS = 8000.0            # MI355X: HBM3E peak (data sheet)


def smooth_depth(N, H, W, device):
    """[N,1,H,W]: a slowly varying surface between 2 and 3.3 with a step of 1.5 that moves a few pixels per frame."""
    y = torch.arange(H, device=device, dtype=torch.float32).view(1, H, 1)
    x = torch.arange(W, device=device, dtype=torch.float32).view(1, 1, W)
    n = torch.arange(N, device=device, dtype=torch.float32).view(N, 1, 1)
    d = 2.5 + 0.3 * torch.sin(x / 40.0 + 0.2 * n) + 0.2 * torch.cos(y / 30.0) + 1.5 * (x > 0.55 * W + 3.0 * n)
    return d.view(N, 1, H, W).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=8)
    ap.add_argument('--sources', type=int, default=4)
    ap.add_argument('--height', type=int, default=bench.H)
    ap.add_argument('--width', type=int, default=bench.W)
    ap.add_argument('--depth', choices=('midas', 'hourglass'), default='hourglass', help='the model\'s depth net (not run here)')
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    from dvd_hip import build, ops
    from dvd_hip.models import render as R
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    V, K, H, W = a.views, a.sources, a.height, a.width
    N = V + K - 1
    store = synthetic_store(N, H, W, [1], device)
    opt = bench.make_opt(depth_chunk=4, depth_graphs=True, midas=a.depth == 'midas')
    model = bench.build_model(opt, device, seed=0)
    depth = smooth_depth(N, H, W, device)
    target = [K - 1 + v for v in range(V)]
    sources = [[g - k for k in range(K)] for g in target]          # every view from its own frame and the K - 1 before it
    frames, view, steps = R.render_plan(N, target, sources, True)
    S = len(frames)

    def event():
        return torch.cuda.Event(enable_timing=True)

    # the whole call
    out = model.render(store, target, sources, depth=depth)       # warm-up of every kernel, and the result
    torch.cuda.synchronize()
    render_ms = []
    for _ in range(a.reps):
        e0, e1 = event(), event()
        e0.record()
        model.render(store, target, sources, depth=depth)
        e1.record()
        torch.cuda.synchronize()
        render_ms.append(e0.elapsed_time(e1))

    # the three launches over the same points
    model.eval()
    with torch.no_grad():
        points = R.advect_points(model, store, depth, frames, steps, S)
    values = store.img[frames].contiguous()
    tabs = {k: store.tables[k][target].contiguous() for k in ops.TRACK_TABLES}
    view_dev = torch.tensor(view, dtype=torch.int32, device=device)
    n_max = K * H * W
    shift = ops.splat_shift(n_max)
    zbuf, acc = ops.splat_workspace(V, 3, H, W, device)
    res = ops.splat_resolve(zbuf, acc, shift)                     # output buffers, reused below
    src = (points, values, view_dev, tabs, V)
    ms = {'clears': [], 'zmin': [], 'accumulate': [], 'resolve': []}
    nbytes = {}
    for rep in range(a.reps + 1):
        ev = [event() for _ in range(5)]
        ev[0].record()
        ops.splat_clear(zbuf, acc)
        ev[1].record()
        b0 = ops.flop_counters()['geometry']
        ops.splat_zmin(zbuf, *src, host_view=view)
        ev[2].record()
        b1 = ops.flop_counters()['geometry']
        ops.splat_accumulate(zbuf, acc, shift, n_max, *src, host_view=view)
        ev[3].record()
        b2 = ops.flop_counters()['geometry']
        ops.splat_resolve(zbuf, acc, shift, out=res)
        ev[4].record()
        b3 = ops.flop_counters()['geometry']
        torch.cuda.synchronize()
        nbytes = {'zmin': b1 - b0, 'accumulate': b2 - b1, 'resolve': b3 - b2}
        if rep:                                                    # (the first pass is the warm-up)
            for i, k in enumerate(('clears', 'zmin', 'accumulate', 'resolve')):
                ms[k].append(ev[i].elapsed_time(ev[i + 1]))
    for k in res:
        assert torch.equal(res[k], out[k]), k                      # the passes timed here ARE what Model.render ran

    def kernel(k):
        t = statistics.median(ms[k])
        return {'ms': t, 'MB_algorithmic': nbytes[k] / 1e6, 'GBps': nbytes[k] / t / 1e6,
                'frac_of_hbm_peak': nbytes[k] / t / 1e6 / HBM_PEAK_GBPS}

    three = sum(statistics.median(ms[k]) for k in ('zmin', 'accumulate', 'resolve'))
    line = json.dumps({
        'metric': 'render at %dx%d: %d views from %d sources each (%d source images, 0 .. %d Euler steps)' % (H, W, V, K, S, K - 1),
        'data': 'synthetic, smooth depth with a step edge', 'device': torch.cuda.get_device_name(device),
        'source_digest': build.source_digest(('splat.hip',)), 'reps': a.reps, 'shift': shift,
        'zmin': kernel('zmin'), 'accumulate': kernel('accumulate'), 'resolve': kernel('resolve'),
        'clears_ms': statistics.median(ms['clears']), 'three_launches_ms': three,
        'three_launches_MB': sum(nbytes.values()) / 1e6,
        'three_launches_frac_of_hbm_peak': sum(nbytes.values()) / three / 1e6 / HBM_PEAK_GBPS,
        'timing_includes': 'the host wrapper (validation) of every launch',
        'render': {'ms': statistics.median(render_ms), 'ms_min': min(render_ms), 'euler_steps': sum(steps)},
        'hit_fraction': float(out['hit'].float().mean()), 'hbm_peak_GBps': HBM_PEAK_GBPS,
        'hbm_peak_allocated_GB': torch.cuda.max_memory_allocated(device) / 2 ** 30})
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
