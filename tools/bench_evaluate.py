#!/usr/bin/env python
"""Measure the evaluation path (ops.eval_tracks, Model.evaluate; csrc/eval.hip, dvd_hip/models/evaluate.py) on a synthetic video
at 384 x 672: --starts start frames x --steps steps.  Prints one JSON line and, with --out, writes it as a profile stamped with
build.source_digest(('eval.hip',)).

  kernel / kernel_maps     median device-event ms of the one dvd_eval_tracks launch over the integrated points of all start
                           frames, without and with the three per-point maps, the algorithmic bytes the library counts for it
                           (dvd_byte_counters, class geometry: per point 12 B of points + 12 B own colour + 9 B flow and mask
                           [+ 12 B of maps], and the depth and colours of the distinct target frames once: 16 B per pixel) and
                           that rate next to the 8 TB/s HBM3E peak
  evaluate / evaluate_maps median device-event ms of the whole Model.evaluate call: the store's gather, ops.unproject, the Euler
                           chain of the MLP, the clear of the sums, the launch, the float64 means and the disparity MSE

The depth is smooth with a step edge (tools/bench_splat.py's).  The feature has no counterpart before it, so no figure here is a
threshold.

    python tools/bench_evaluate.py --out profiles/evaluate.json

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
from bench_splat import HBM_PEAK_GBPS, smooth_depth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--starts', type=int, default=8)
    ap.add_argument('--steps', type=int, default=4)
    ap.add_argument('--height', type=int, default=bench.H)
    ap.add_argument('--width', type=int, default=bench.W)
    ap.add_argument('--depth', choices=('midas', 'hourglass'), default='hourglass', help='the model\'s depth net (not run here)')
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    from dvd_hip import build, ops
    from dvd_hip.models import evaluate as EV
    from dvd_hip.models import tracks
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    B, K, H, W = a.starts, a.steps, a.height, a.width
    N = B + K
    store = synthetic_store(N, H, W, list(range(1, K + 1)), device)
    opt = bench.make_opt(depth_chunk=4, depth_graphs=True, midas=a.depth == 'midas')
    model = bench.build_model(opt, device, seed=0)
    depth = smooth_depth(N, H, W, device)
    start = list(range(B))

    def event():
        return torch.cuda.Event(enable_timing=True)

    def timed(fn):
        fn()                                                       # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = event(), event()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    # the whole call
    whole = {m: timed(lambda m=m: model.evaluate(store, start, K, depth=depth, maps=m)) for m in (False, True)}
    out = model.evaluate(store, start, K, depth=depth, maps=True)

    # the one launch over the same points
    valid, table = EV.evaluate_plan(store.cat, start, K)
    model.eval()
    with torch.no_grad():
        points, ts = tracks.start_slab(model, store, depth, start, K + 1)
        tracks.integrate(model._mlp, points, ts, valid, 1.0 / N, 1.0 / opt.sf_mag_div, B)
    source = torch.tensor(start, dtype=torch.int32, device=device)
    pair_row = torch.from_numpy(table).to(device)
    sums = torch.zeros(K, B, 6, device=device, dtype=torch.int64)
    maps = torch.empty(K, B, 3, H, W, device=device)
    nbytes = {}

    def launch(with_maps):
        sums.zero_()
        b0 = ops.flop_counters()['geometry']
        ops.eval_tracks(points[1:], source, store.tables, depth, store.img, k_first=1, pairs=(pair_row, store.flow_1_2, store.mask_2),
                        sums=sums, maps=maps if with_maps else False, host_source=start)
        nbytes[with_maps] = ops.flop_counters()['geometry'] - b0

    ms = {m: timed(lambda m=m: launch(m)) for m in (False, True)}
    assert torch.equal(sums, out['sums']) and torch.equal(maps, out['maps'])      # the launch timed here IS what evaluate ran

    def kernel(m):
        t = statistics.median(ms[m])
        return {'ms': t, 'ms_min': min(ms[m]), 'MB_algorithmic': nbytes[m] / 1e6, 'GBps': nbytes[m] / t / 1e6,
                'frac_of_hbm_peak': nbytes[m] / t / 1e6 / HBM_PEAK_GBPS}

    by = {k: [float(x) for x in v.cpu().tolist()] for k, v in out['by_step'].items()}
    line = json.dumps({
        'metric': 'evaluate at %dx%d: %d start frames x %d steps (%d points)' % (H, W, B, K, B * K * H * W),
        'data': 'synthetic, smooth depth with a step edge', 'device': torch.cuda.get_device_name(device),
        'source_digest': build.source_digest(('eval.hip',)), 'reps': a.reps, 'shift': out['shift'],
        'kernel': kernel(False), 'kernel_maps': kernel(True),
        'timing_includes': 'the clear of the sums and the host wrapper (validation) of the launch',
        'evaluate': {'ms': statistics.median(whole[False]), 'ms_min': min(whole[False])},
        'evaluate_maps': {'ms': statistics.median(whole[True]), 'ms_min': min(whole[True])},
        'euler_steps': int(sum(valid)), 'by_step': by, 'hbm_peak_GBps': HBM_PEAK_GBPS,
        'hbm_peak_allocated_GB': torch.cuda.max_memory_allocated(device) / 2 ** 30})
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
