#!/usr/bin/env python
"""Measure query-point tracks (ops.point_seed / point_project / point_score; csrc/point_track.hip) next to the scene-flow MLP
steps that carry the points: Q in {256, 16 384, 1 048 576} queries of a 60-frame video at 384 x 672, in a slab of T1 = 60 rows
with the queries' own row in the middle, as Model.track_points lays it out.  Prints one JSON line and, with --out, writes it as a
profile stamped with build.source_digest(('point_track.hip',)).

  per Q   median and least device-event ms of each launch over --reps timed windows of --calls calls: the seed, one stash-free
          MLP forward of Q points (a forward step of the chain), one inverse step (n_iter = 4 forwards and updates), the ONE
          projection of all T1 rows and the ONE score of them; the algorithmic bytes the library counts for the three new
          kernels (dvd_byte_counters, class geometry) and that rate next to the 8 TB/s HBM3E peak
  chain   what a whole Model.track_points + score costs at that Q from those parts -- seed + 59 steps + project + score, the
          steps forward or inverse by where the query's frame lies (a query takes all steps on both sides) -- and the MLP's
          share of it

Cameras are a slow pan over a smooth synthetic depth; the MLP has random weights (its cost does not depend on them).  The feature
has no counterpart before it, so no figure here is a threshold.

    python tools/bench_point_tracks.py --out profiles/point_tracks.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'dynamic-video-depth_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBPS = 8000.0            # MI355X: HBM3E peak (data sheet)
QS = (256, 16384, 1048576)
N_FRAMES, H, W = 60, 384, 672


def synthetic_video(device):
    """(tables of N_FRAMES cameras panning along x, depth [N,1,H,W])."""
    n = torch.arange(N_FRAMES, dtype=torch.float32)
    K = torch.tensor([[0.9 * W, 0.0, (W - 1) / 2.0], [0.0, 0.9 * W, (H - 1) / 2.0], [0.0, 0.0, 1.0]])
    eye = torch.eye(3).expand(N_FRAMES, 3, 3).contiguous()
    t = torch.stack([0.01 * n, torch.zeros_like(n), torch.zeros_like(n)], 1)
    tabs = {'R': eye, 'R_T': eye.clone(), 't': t, 'K_T': K.T.expand(N_FRAMES, 3, 3).contiguous(),
            'K_inv_T': torch.linalg.inv(K).T.expand(N_FRAMES, 3, 3).contiguous(), 'ts_vali': n / N_FRAMES}
    y = torch.arange(H, dtype=torch.float32).view(1, H, 1)
    x = torch.arange(W, dtype=torch.float32).view(1, 1, W)
    depth = 2.5 + 0.3 * torch.sin(x / 40.0 + 0.2 * n.view(-1, 1, 1)) + 0.2 * torch.cos(y / 30.0)
    return {k: v.to(device).contiguous() for k, v in tabs.items()}, depth.view(N_FRAMES, 1, H, W).to(device).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--calls', type=int, default=10, help='calls per timed window')
    ap.add_argument('--queries', type=str, default=None, help='e.g. 256,16384 (default: the three of QS)')
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

    def counted(fn):
        b0 = ops.flop_counters()['geometry']
        fn()
        return ops.flop_counters()['geometry'] - b0

    tabs, depth = synthetic_video(device)
    mlp = ops.SceneFlowMLPKernels(device, n_freq_xyz=16, n_freq_t=16, time_dependent=True)
    g = torch.Generator().manual_seed(0)
    dims = [mlp.c_in] + [256] * 5
    mlp.pack([(torch.randn(256 if i < 5 else 3, dims[i], generator=g) / dims[i] ** 0.5).to(device) for i in range(6)],
             [torch.zeros(256 if i < 5 else 3, device=device) for i in range(6)])
    T1, time_step, out_scale = N_FRAMES, 1.0 / N_FRAMES, 1.0 / 100.0
    results = []
    for Q in (QS if a.queries is None else [int(v) for v in a.queries.split(',')]):
        rng = np.random.RandomState(Q)
        frame = rng.randint(0, N_FRAMES, Q).astype(np.int32)
        frame_d = torch.from_numpy(frame).to(device)
        xy = torch.from_numpy(np.stack([rng.uniform(0, W - 1, Q), rng.uniform(0, H - 1, Q)], 1).astype(np.float32)).to(device)
        points = torch.zeros(T1, 3, Q, device=device)
        rows = points.view(T1, 1, 3, 1, Q)
        so = {'points': points[0], 'ok': torch.empty(Q, device=device, dtype=torch.uint8), 't': torch.empty(Q, device=device)}
        seed = lambda: ops.point_seed(frame_d, xy, depth, tabs, out=so, host_frame=frame)      # noqa: E731
        seed()
        ts = so['t'].view(1, 1, 1, Q)
        step = lambda: mlp.forward(rows[0], ts, t_offset=time_step, out_scale=out_scale, p_next=rows[1])      # noqa: E731
        scratch = torch.empty(1, 3, 1, Q, device=device)
        back = lambda: ops.invert_step(mlp, rows[0], ts, -time_step, out_scale, n_iter=4, out=rows[2], scratch=scratch)  # noqa: E731
        for k in range(T1 - 1):                                       # a real slab for the projection: the chain from row 0
            mlp.forward(rows[k], ts, t_offset=k * time_step, out_scale=out_scale, p_next=rows[k + 1])
        k0 = -(N_FRAMES // 2)
        po = ops.point_project(points, frame_d, xy, tabs, depth, k0=k0, ok=so['ok'], host_frame=frame)
        project = lambda: ops.point_project(points, frame_d, xy, tabs, depth, k0=k0, ok=so['ok'], out=po, host_frame=frame)  # noqa: E731
        gt_uv = (po['uv'].permute(1, 0, 2) + 1.5).contiguous()        # [Q,T1,2] -> the frames of the rows that have one
        gt = torch.zeros(Q, N_FRAMES, 2, device=device)
        gt_state = torch.full((Q, N_FRAMES), 2, device=device, dtype=torch.uint8)
        live = po['target'].T >= 0
        qi = torch.arange(Q, device=device)[:, None].expand(Q, T1)[live]
        gi = po['target'].T[live].long()
        gt[qi, gi] = gt_uv[live]
        gt_state[qi, gi] = 0
        sums = torch.zeros(T1, len(ops.POINT_SUMS), device=device, dtype=torch.int64)
        score = lambda: ops.point_score(po['uv'], po['visible'], po['target'], gt, gt_state, origin=-k0, sums=sums)  # noqa: E731
        r = {'Q': Q, 'T1': T1, 'frames': N_FRAMES, 'H': H, 'W': W, 'live_rows': int(live.sum()),
             'visible_fraction': float(po['visible'].float().sum() / max(1, int(live.sum())))}
        for name, fn in (('seed', seed), ('project', project), ('score', score)):
            r[name] = timed(fn)
            r[name]['MB_algorithmic'] = counted(fn) / 1e6
            r[name]['GBps'] = r[name]['MB_algorithmic'] / r[name]['ms']
            r[name]['frac_of_hbm_peak'] = r[name]['GBps'] / HBM_PEAK_GBPS
        r['mlp_forward_step'] = timed(step)
        r['mlp_inverse_step'] = timed(back)
        # a whole track + score from its parts: a query at frame f takes all T1 - 1 steps on both sides of f; with the origin row
        # in the middle of the slab that is (T1 - 1) / 2 forward and as many inverse steps
        n_fwd = (T1 - 1) - (T1 - 1) // 2
        n_inv = (T1 - 1) // 2
        mlp_ms = n_fwd * r['mlp_forward_step']['ms'] + n_inv * r['mlp_inverse_step']['ms']
        new_ms = r['seed']['ms'] + r['project']['ms'] + r['score']['ms']
        r['chain'] = {'forward_steps': n_fwd, 'inverse_steps': n_inv, 'mlp_ms': mlp_ms, 'point_kernels_ms': new_ms,
                      'total_ms': mlp_ms + new_ms, 'mlp_share': mlp_ms / (mlp_ms + new_ms)}
        results.append(r)
        del points, rows, po, gt, gt_state, gt_uv, scratch, sums
    line = json.dumps({
        'metric': 'query-point tracks: ops.point_seed, point_project (T1 = 60 rows), point_score, and the MLP steps between them',
        'data': 'synthetic 60-frame pan at 384 x 672, queries uniform over frames and positions, random MLP weights',
        'device': torch.cuda.get_device_name(device), 'source_digest': build.source_digest(('point_track.hip',)), 'reps': a.reps,
        'calls_per_window': a.calls, 'queries': results,
        'timing': 'device events around the host wrapper and its launch(es); chain: composed from the per-launch medians',
        'hbm_peak_GBps': HBM_PEAK_GBPS})
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
