#!/usr/bin/env python
"""Measure push-pull hole filling (ops.fill_holes; csrc/fill.hip) on synthetic renders: V views of 3 colours and a depth (C = 4)
with the depth squared as bias, the shape Model.render(inpaint=True) calls it with, at 1 x and 16 x 384 x 672 and at 1 x and
16 x 768 x 1344.  Prints one JSON line and, with --out, writes it as a profile stamped with build.source_digest(('fill.hip',)).

  per shape   median and least device-event ms of the whole call (three launches and the host wrapper), in place and into a
              second buffer, over --reps calls in one timed window per repetition; the algorithmic bytes the library counts for
              the call (dvd_byte_counters, class geometry: values, known and bias read by both tile kernels, the pyramid
              written and read once, values and level written) and that rate next to the 8 TB/s HBM3E peak
  launches    the same call captured into a HIP graph and replayed: what remains once the host wrapper and the launch gaps are
              taken out of the call

The known map is a render's: a band along two borders missing, a disocclusion strip behind a step edge, and 5 % splat gaps.  The
feature has no counterpart before it, so no figure here is a threshold.

    python tools/bench_fill.py --out profiles/fill.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'dynamic-video-depth_amd'))

import torch  # noqa: E402

HBM_PEAK_GBPS = 8000.0            # MI355X: HBM3E peak (data sheet)
SHAPES = ((1, 384, 672), (16, 384, 672), (1, 768, 1344), (16, 768, 1344))


def synthetic_render(V, H, W, device, seed=0):
    """(joint [V,4,H,W]: colours and depth, hit uint8 [V,H,W], depth [V,1,H,W]) of a render with holes."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    y = torch.arange(H, dtype=torch.float32).view(1, H, 1)
    x = torch.arange(W, dtype=torch.float32).view(1, 1, W)
    n = torch.arange(V, dtype=torch.float32).view(V, 1, 1)
    edge = 0.55 * W + 3.0 * n
    depth = 2.5 + 0.3 * torch.sin(x / 40.0 + 0.2 * n) + 0.2 * torch.cos(y / 30.0) + 1.5 * (x > edge)
    hit = torch.rand(V, H, W, generator=g) > 0.05
    hit &= (x >= W // 24) & (y < H - H // 16)                       # the borders of a camera that has moved
    hit &= ~((x > edge - W // 32) & (x <= edge))                    # the disocclusion behind the step edge
    colours = torch.rand(V, 3, H, W, generator=g)
    depth = depth.view(V, 1, H, W) * hit[:, None]
    joint = torch.cat((colours * hit[:, None], depth), dim=1)
    return joint.to(device).contiguous(), hit.to(torch.uint8).to(device).contiguous(), depth.to(device).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--calls', type=int, default=20, help='calls per timed window')
    ap.add_argument('--power', type=int, default=2)
    ap.add_argument('--shapes', type=str, default=None, help='e.g. 16x384x672,1x768x1344 (default: the four of SHAPES)')
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    from dvd_hip import build, ops
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)

    def timed(fn):
        fn()                                                         # warm-up of this shape
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / a.calls)
        return {'ms': statistics.median(ms), 'ms_min': min(ms)}

    shapes = []
    for V, H, W in (SHAPES if a.shapes is None else [tuple(int(n) for n in sh.split('x')) for sh in a.shapes.split(',')]):
        joint, hit, depth = synthetic_render(V, H, W, device)
        C = joint.shape[1]
        ws = ops.fill_workspace(V, C, H, W, device)
        out = {'values': torch.empty_like(joint), 'level': torch.empty_like(hit)}
        b0 = ops.flop_counters()['geometry']
        ref = ops.fill_holes(joint, hit, depth, a.power, 0.0, out=out, workspace=ws)
        nbytes = ops.flop_counters()['geometry'] - b0
        torch.cuda.synchronize()
        want = {k: v.clone() for k, v in ref.items()}
        r = {'V': V, 'C': C, 'H': H, 'W': W, 'MB_algorithmic': nbytes / 1e6, 'workspace_MB': ws.numel() * 4 / 1e6,
             'hole_fraction': 1.0 - float(hit.float().mean()), 'max_level': int(want['level'].max())}
        r['call'] = timed(lambda: ops.fill_holes(joint, hit, depth, a.power, 0.0, out=out, workspace=ws))
        # in place: after the first call every pixel that was unknown holds its filled value, which the kernels write again
        inplace = joint.clone()
        r['call_in_place'] = timed(lambda: ops.fill_holes(inplace, hit, depth, a.power, 0.0, out={'values': inplace, 'level': out['level']},
                                                          workspace=ws))
        assert torch.equal(inplace, want['values'])
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                                # (no allocation inside: outputs and workspace are given)
            ops.fill_holes(joint, hit, depth, a.power, 0.0, out=out, workspace=ws)
        out['values'].zero_()
        r['launches'] = timed(graph.replay)
        for k in want:
            assert torch.equal(out[k], want[k]), k                   # every timed variant computed the same bits
        for k in ('call', 'call_in_place', 'launches'):
            r[k]['GBps'] = nbytes / r[k]['ms'] / 1e6
            r[k]['frac_of_hbm_peak'] = r[k]['GBps'] / HBM_PEAK_GBPS
        shapes.append(r)
        del joint, hit, depth, ws, out, inplace, graph
    line = json.dumps({
        'metric': 'ops.fill_holes, C = 4 (colours and depth), bias = depth, power %d: three launches per call' % a.power,
        'data': 'synthetic render: missing borders, a disocclusion strip, 5 % splat gaps',
        'device': torch.cuda.get_device_name(device), 'source_digest': build.source_digest(('fill.hip',)), 'reps': a.reps,
        'calls_per_window': a.calls, 'launches_per_call': 3, 'shapes': shapes,
        'timing': 'call: device events around the host wrapper and its three launches; launches: the same captured into a graph',
        'hbm_peak_GBps': HBM_PEAK_GBPS})
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
