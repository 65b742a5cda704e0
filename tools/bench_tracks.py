#!/usr/bin/env python
"""Measure the long-range track path (Model.video_depth, Model.track; dvd_hip/models/tracks.py) on a synthetic video of
--frames frames of 384 x 672, --steps Euler steps from every frame.  Prints one JSON line and, with --out, writes it as a profile
stamped with build.source_digest(('track.hip',)).

  video_depth  ms per frame of the depth net over the store's validation view (after a warm-up pass that captures its graphs)
  chain        ms per (frame . step) of the chain: the store's gather, ops.unproject and every stash-free MLP forward
  project      event-timed dvd_track_project over all rows, its algorithmic bytes -- 12 B read and 17 B written per point, plus
               every depth map of the video read once for the gather -- over that time, next to the 8 TB/s HBM3E peak; once
               through ops.track_project (with the wrapper's validation) and once as back-to-back calls of the C entry

  back         (--n_back K) the chain run backwards from every frame: ms per (frame . backward step) of tracks.integrate_back
               (n_iter stash-free MLP forwards + n_iter dvd_track_invert_update launches per step), and the update kernel alone
               over all frames -- 48 B per point (three planes of three values read, one written) over its time

All of them are device-event times after a warm-up.  The feature has no counterpart before it, so no figure here is a threshold.

    python tools/bench_tracks.py --out profiles/tracks.json

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

HBM_PEAK_GBPS = 8000.0            # MI355X: HBM3E peak (data sheet)


def timed(fn, reps):
    """Mean device time of fn() in ms over reps runs, after one untimed run."""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def bench_back(a, model, opt, tracks, ops, p0, ts, start, chunk):
    """The backward half: tracks.integrate_back from the un-projected frames p0 [N,3,H,W], and one update launch on its own."""
    N, _, H, W = p0.shape
    valid_back = tracks.track_plan_back(N, start, a.n_back)
    slab = torch.zeros(a.n_back + 1, N, 3, H, W, device=p0.device)
    slab[a.n_back].copy_(p0)
    resid = torch.zeros(a.n_back, N, device=p0.device)

    def run_back():
        tracks.integrate_back(model._mlp, slab, ts if opt.time_dependent else None, valid_back, 1.0 / N, 1.0 / opt.sf_mag_div,
                              chunk, n_iter=a.n_iter, resid=resid)
    back_ms = timed(run_back, a.reps)
    sf, y = torch.zeros_like(p0), p0.clone()
    r = torch.zeros(N, device=p0.device)

    def run_update():
        ops.invert_update(p0, sf, y, out=y, resid=r)          # the iterate updated in place: every round but the first
    update_ms = timed(run_update, max(a.reps, 10))
    nbytes = 48.0 * N * H * W
    frame_steps = sum(valid_back)
    return {'n_back': a.n_back, 'n_iter': a.n_iter, 'ms_total': back_ms, 'frame_steps': frame_steps,
            'ms_per_frame_step': back_ms / frame_steps, 'resid_max': float(resid.max()),
            'update': {'ms': update_ms, 'points': N * H * W, 'MB_algorithmic': nbytes / 1e6, 'GBps': nbytes / update_ms / 1e6,
                       'frac_of_hbm_peak': nbytes / update_ms / 1e6 / HBM_PEAK_GBPS,
                       'bytes_model': '36 B read + 12 B written per point (p, sf and the iterate read, the iterate written in place)',
                       'timing_includes': 'the host wrapper (validation) of every launch'}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=80)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--height', type=int, default=bench.H)
    ap.add_argument('--width', type=int, default=bench.W)
    ap.add_argument('--depth', choices=('midas', 'hourglass'), default='midas')
    ap.add_argument('--depth_batch', type=int, default=8, help='frames per batch of the validation view')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--n_back', type=int, default=0, help='also time this many backward steps from every frame (0: not at all)')
    ap.add_argument('--n_iter', type=int, default=4, help='fixed-point iterations per backward step')
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    from dvd_hip import build, ops
    from dvd_hip.models import tracks
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    N, H, W, n_steps = a.frames, a.height, a.width, a.steps
    store = synthetic_store(N, H, W, [1], device)
    opt = bench.make_opt(depth_chunk=a.depth_batch, depth_graphs=True, midas=a.depth == 'midas')
    model = bench.build_model(opt, device, seed=0)
    start = list(range(N))
    valid = tracks.track_plan(N, start, n_steps)
    frame_steps = sum(valid)

    keep = {}

    def run_depth():
        keep['depth'] = model.video_depth(store.frames(a.depth_batch))
    depth_ms = timed(run_depth, a.reps)
    depth = keep['depth']

    out = model.track(store, start, n_steps, depth=depth)          # the whole path once: warm-up of every kernel, and the result
    points = out['points']
    T = store.tables
    ts = torch.empty(N, 1, H, W, device=device)
    d0 = torch.empty(N, 1, H, W, device=device)
    R0, K0, t0 = torch.empty(N, 3, 3, device=device), torch.empty(N, 3, 3, device=device), torch.empty(N, 3, device=device)
    import numpy as np
    index = np.array([start, start, start], dtype=np.int32)
    chunk = tracks.default_chunk(n_steps, H, W)

    def run_chain():
        ops.store_gather([(depth, d0, 'copy', 0), (T['R_T'], R0, 'copy', 0), (T['K_inv_T'], K0, 'copy', 0), (T['t'], t0, 'copy', 0),
                          (T['ts_vali'], ts, 'fill', 0)], index)
        ops.unproject(d0, R0, t0, K0, planar=True, out=points[0])
        tracks.integrate(model._mlp, points, ts if opt.time_dependent else None, valid, 1.0 / N, 1.0 / opt.sf_mag_div, chunk)
    chain_ms = timed(run_chain, a.reps)

    pre = {k: out[k] for k in ('uv', 'z', 'depth_at', 'inside')}
    start_dev = torch.tensor(start, dtype=torch.int32, device=device)

    def run_project():
        ops.track_project(points, start_dev, T, depth_all=depth, out=pre, host_start=start)
    project_ms = timed(run_project, max(a.reps, 10))

    # the launch alone: the C entry with every argument prepared, nothing of the Python wrapper between two launches
    import ctypes
    from dvd_hip import _lib
    lib, ptr = _lib.load(), lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = (ptr(points), 1, ptr(start_dev), ptr(T['R']), ptr(T['t']), ptr(T['K_T']), ptr(depth), N, ptr(pre['uv']), 0,
            ptr(pre['z']), ptr(pre['depth_at']), ptr(pre['inside']), n_steps + 1, N, H, W, stream)

    def run_launch():
        _lib.check(lib.dvd_track_project(*args), 'dvd_track_project')
    launch_ms = timed(run_launch, max(a.reps, 10))
    n_points = (n_steps + 1) * N * H * W
    nbytes = 29.0 * n_points + 4.0 * N * H * W
    res = {'metric': 'long-range tracks at %dx%d, %d frames, %d steps from every frame' % (H, W, N, n_steps),
           'data': 'synthetic', 'device': torch.cuda.get_device_name(device), 'depth_net': a.depth,
           'source_digest': build.source_digest(('track.hip',)),
           'video_depth': {'ms_total': depth_ms, 'ms_per_frame': depth_ms / N, 'frames_per_batch': a.depth_batch},
           'chain': {'ms_total': chain_ms, 'frame_steps': frame_steps, 'ms_per_frame_step': chain_ms / frame_steps,
                     'start_frames_per_pass': min(chunk, N)},
           'project': {'ms': project_ms, 'points': n_points, 'MB_algorithmic': nbytes / 1e6, 'GBps': nbytes / project_ms / 1e6,
                       'hbm_peak_GBps': HBM_PEAK_GBPS, 'frac_of_hbm_peak': nbytes / project_ms / 1e6 / HBM_PEAK_GBPS,
                       'bytes_model': '12 B read + 17 B written per point, every depth map read once',
                       'timing_includes': 'the host wrapper (validation) of every launch',
                       'ms_launch_only': launch_ms, 'GBps_launch_only': nbytes / launch_ms / 1e6,
                       'frac_of_hbm_peak_launch_only': nbytes / launch_ms / 1e6 / HBM_PEAK_GBPS,
                       'inside_fraction': float(out['inside'].float().mean())},
           'hbm_peak_allocated_GB': torch.cuda.max_memory_allocated(device) / 2 ** 30}
    if a.n_back > 0:
        res['back'] = bench_back(a, model, opt, tracks, ops, points[0], ts, start, chunk)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
