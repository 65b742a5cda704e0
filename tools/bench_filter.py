#!/usr/bin/env python
"""Measure the temporal depth filter (Model.filter_depth; dvd_hip/models/filter.py, csrc/track_filter.hip) on a synthetic video
of --frames frames of 384 x 672 with a window of --radius frames on either side.  Prints one JSON line and, with --out, writes
it as a profile stamped with build.source_digest(('track_filter.hip',)).

  fused        event-timed dvd_track_filter over the slab of ALL frames, in both modes, and the bytes it moves: 12 B read per
               point and neighbour row, 4 B of the frame's own depth read and 13 B written per pixel, every depth map of the
               video read once for the gather
  composed     what it replaces on the same slab: ops.track_project (12 B read, 17 B written per point and row) and the torch
               reductions that gate and fuse its z / depth_at / inside into the same four outputs (mean mode)
  filter_depth the whole call: the store's gather, the un-projection, 2 radius Euler chains (one forward per forward step,
               n_iter per backward step) and the fused launch, chunk by chunk; peak memory allocated while it ran

All of them are device-event times after a warm-up run, the mean over --reps runs.  The tool asserts nothing, and no figure
here is a threshold.

    python tools/bench_filter.py --out profiles/filter.json

bench.py is not touched by this tool; model and options come from its make_opt / build_model, the store from
tools/bench_frame_store.py's synthetic_store."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'dynamic-video-depth_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import torch  # noqa: E402

import bench  # noqa: E402
from bench_frame_store import synthetic_store  # noqa: E402
from bench_tracks import HBM_PEAK_GBPS, timed  # noqa: E402


def composed(ops, points, start_dev, start, T, depth, w_dev, radius, tol, z_near, pre):
    """ops.track_project and the torch reductions of the mean mode -> depth, ratio, count, spread."""
    rows = ops.track_project(points, start_dev, T, depth_all=depth, out=pre, host_start=start, k0=-radius)
    z, D, inside = rows['z'], rows['depth_at'], rows['inside']
    tl = 1.0 + tol
    counts = (inside != 0) & (z >= z_near) & (D > 0) & (z <= D * tl) & (D <= z * tl)
    r = D / z
    counts[radius] = True
    r[radius] = 1.0
    w = w_dev.view(-1, 1, 1, 1)
    zero = torch.zeros((), device=z.device)
    acc = torch.where(counts, w * r, zero).sum(0)
    ws = torch.where(counts, w.expand_as(r), zero).sum(0)
    ratio = acc / ws
    spread = torch.where(counts, r, -torch.inf).amax(0) - torch.where(counts, r, torch.inf).amin(0)
    d0 = depth[start_dev.long(), 0]
    return d0 * ratio, ratio, counts.sum(0).to(torch.uint8), spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=80)
    ap.add_argument('--radius', type=int, default=4)
    ap.add_argument('--height', type=int, default=bench.H)
    ap.add_argument('--width', type=int, default=bench.W)
    ap.add_argument('--depth', choices=('midas', 'hourglass'), default='midas')
    ap.add_argument('--depth_batch', type=int, default=8, help='frames per batch of the validation view')
    ap.add_argument('--chunk', type=int, default=None, help='frames per pass of filter_depth (default: its own)')
    ap.add_argument('--tol', type=float, default=0.1)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    from dvd_hip import build, ops
    from dvd_hip.models import tracks
    from dvd_hip.models.filter import filter_weights
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    N, H, W, radius = a.frames, a.height, a.width, a.radius
    T1 = 2 * radius + 1
    store = synthetic_store(N, H, W, [1], device)
    opt = bench.make_opt(depth_chunk=a.depth_batch, depth_graphs=True, midas=a.depth == 'midas')
    model = bench.build_model(opt, device, seed=0)
    start = list(range(N))
    depth = model.video_depth(store.frames(a.depth_batch))
    T = store.tables
    w = filter_weights(radius)
    w_dev = torch.from_numpy(w).to(device)
    start_dev = torch.tensor(start, dtype=torch.int32, device=device)

    # the whole call first: warm-up of every kernel, and its peak memory on its own
    torch.cuda.reset_peak_memory_stats(device)
    base = torch.cuda.memory_allocated(device)
    keep = {}

    def run_all():
        keep['out'] = model.filter_depth(store, None, radius, depth=depth, chunk=a.chunk, tol=a.tol)
    all_ms = timed(run_all, a.reps)
    peak_call = torch.cuda.max_memory_allocated(device) - base
    ref = keep.pop('out')

    tr = model.track(store, start, radius, depth=depth, n_back=radius)
    points = tr['points']
    pre = {k: tr[k] for k in ('uv', 'z', 'depth_at', 'inside')}
    outs = {k: torch.empty_like(ref[k]) for k in ('depth', 'ratio', 'count', 'spread')}
    fused = {}
    for mode in ('mean', 'median'):
        def run_fused():
            ops.track_filter(points, start_dev, T, depth, w, k0=-radius, mode=mode, tol=a.tol, out=outs, host_start=start)
        fused[mode] = timed(run_fused, max(a.reps, 10))
    same = bool(torch.equal(ops.track_filter(points, start_dev, T, depth, w, k0=-radius, tol=a.tol, host_start=start)['depth'], ref['depth']))

    def run_composed():
        keep['c'] = composed(ops, points, start_dev, start, T, depth, w_dev, radius, a.tol, 1e-3, pre)
    composed_ms = timed(run_composed, max(a.reps, 10))

    def run_project():
        ops.track_project(points, start_dev, T, depth_all=depth, out=pre, host_start=start, k0=-radius)
    project_ms = timed(run_project, max(a.reps, 10))
    # (the two differ where a gate hangs on the last bits -- torch divides and multiplies in another order -- and where the
    #  frame's own depth is not > 0, which the composition does not treat)
    differing = float(((keep['c'][0].unsqueeze(1) / ref['depth'] - 1).abs() > 1e-5).float().mean())

    px = float(N * H * W)
    live = float(sum(tracks.track_plan(N, start, radius)) + sum(tracks.track_plan_back(N, start, radius))) * H * W
    fused_bytes = 12.0 * live + (4.0 + 13.0) * px + 4.0 * px
    project_bytes = 29.0 * T1 * px + 4.0 * px
    composed_bytes = project_bytes + 9.0 * T1 * px + 13.0 * px       # the rows read back once (at least) by the reductions
    res = {'metric': 'temporal depth filter at %dx%d, %d frames, radius %d' % (H, W, N, radius), 'data': 'synthetic',
           'device': torch.cuda.get_device_name(device), 'depth_net': a.depth,
           'source_digest': build.source_digest(('track_filter.hip',)),
           'fused': {'ms_mean': fused['mean'], 'ms_median': fused['median'], 'MB_algorithmic': fused_bytes / 1e6,
                     'GBps_mean': fused_bytes / fused['mean'] / 1e6, 'frac_of_hbm_peak_mean': fused_bytes / fused['mean'] / 1e6 / HBM_PEAK_GBPS,
                     'bytes_model': '12 B read per point and neighbour row with a frame, 4 + 13 B per pixel, every depth map once',
                     'timing_includes': 'the host wrapper (validation, upload of the weights) of every launch',
                     'same_bits_as_filter_depth': same, 'mean_count': float(ref['count'].float().mean())},
           'composed': {'ms': composed_ms, 'ms_track_project': project_ms, 'MB_algorithmic_at_least': composed_bytes / 1e6,
                        'MB_track_project': project_bytes / 1e6, 'MB_rows_kept': 17.0 * T1 * px / 1e6,
                        'share_of_pixels_differing_from_fused': differing},
           'filter_depth': {'ms_total': all_ms, 'ms_per_frame': all_ms / N, 'frames_per_pass': a.chunk or min(N, tracks.default_chunk(2 * radius, H, W)),
                            'mlp_passes_per_frame': radius * (1 + 4), 'fused_share': fused['mean'] / all_ms,
                            'peak_allocated_GB': peak_call / 2 ** 30, 'slab_GB': 12.0 * T1 * px / 2 ** 30}}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
