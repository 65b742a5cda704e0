#!/usr/bin/env python
"""Time ONE optimisation step over pairs of different frame gaps (models/scene_flow_motion_field.py, gap_plan), and the batched
pair permutation it rests on.  Prints one JSON line; same convention as bench.py (two HIP-graph set-up steps, then --warmup
untimed and --steps timed steps on one device-resident synthetic batch; MiDaS at 384x672, non-warm phase with the regulariser).

    python tools/bench_mixed_gaps.py                              # 48 pairs, gaps (1, 2, 4) x 16, interleaved order
    python tools/bench_mixed_gaps.py --order grouped              # the same pairs already sorted by gap: no permutation launch
    python tools/bench_mixed_gaps.py --gather_only                # dvd_gather_pairs against torch.index_select per tensor

What to compare the step with: the SUM of `python bench.py --pairs 16 --gap g --no_extras --no_cpu_baseline` over the gaps -- the
only way to run these pairs without mixing gaps.  bench.py is not touched by this tool; model and options come from its
make_opt / build_model."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'dynamic-video-depth_amd'))

import torch  # noqa: E402

import bench  # noqa: E402

COPY_CEILING_GBPS = 6290.0        # MI355X: measured float4 copy, 79 % of the 8 TB/s HBM3E peak


def time_gather(batch, perm, reps=20):
    """dvd_gather_pairs (one launch over every per-pair tensor) against torch.index_select per tensor, on the same tensors."""
    from dvd_hip import ops
    B = len(perm)
    tensors = [v for v in batch.values() if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == B]
    nbytes = 2.0 * sum(t.numel() * t.element_size() for t in tensors)
    dev = tensors[0].device
    p32 = torch.tensor(perm, dtype=torch.int32, device=dev)
    p64 = p32.long()
    out = [torch.empty_like(t) for t in tensors]

    def run(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    ms_g = run(lambda: ops.gather_pairs(tensors, p32, out=out))
    ms_t = run(lambda: [torch.index_select(t, 0, p64, out=o) for t, o in zip(tensors, out)])
    same = all(torch.equal(o, torch.index_select(t, 0, p64)) for t, o in zip(tensors, ops.gather_pairs(tensors, p32)))
    return {'tensors': len(tensors), 'MB_moved': nbytes / 1e6, 'gather_pairs_ms': ms_g, 'index_select_ms': ms_t,
            'gather_pairs_GBps': nbytes / ms_g / 1e6, 'index_select_GBps': nbytes / ms_t / 1e6,
            'gather_pairs_frac_of_copy_ceiling': nbytes / ms_g / 1e6 / COPY_CEILING_GBPS, 'copy_ceiling_GBps': COPY_CEILING_GBPS,
            'equal_to_index_select': bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--pairs', type=int, default=48)
    ap.add_argument('--gaps', type=str, default='1,2,4', help='the frame gaps of the step, in equal shares')
    ap.add_argument('--order', choices=('interleaved', 'grouped'), default='interleaved')
    ap.add_argument('--depth', choices=('midas', 'hourglass'), default='midas')
    ap.add_argument('--depth_chunk', type=int, default=0)
    ap.add_argument('--height', type=int, default=bench.H)
    ap.add_argument('--width', type=int, default=bench.W)
    ap.add_argument('--gather_only', action='store_true')
    a = ap.parse_args()
    from dvd_hip import ops, synthetic
    gaps = [int(g) for g in a.gaps.split(',')]
    per_pair = [gaps[b % len(gaps)] for b in range(a.pairs)]
    if a.order == 'grouped':
        per_pair = sorted(per_pair)
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    H, W = a.height, a.width
    batch = synthetic.make_batch(a.pairs, H, W, gap=per_pair, seed=1234, device=device)
    perm = sorted(range(a.pairs), key=lambda b: per_pair[b])
    out = {'metric': 'ms per optimisation step over mixed frame gaps at %dx%d, %d pairs' % (H, W, a.pairs), 'unit': 'ms',
           'higher_is_better': False, 'pairs': a.pairs, 'gaps': gaps, 'order': a.order, 'height': H, 'width': W,
           'depth_net': a.depth, 'data': 'synthetic'}
    out['gather'] = time_gather(batch, perm)
    if not a.gather_only:
        opt = bench.make_opt(depth_chunk=min(a.depth_chunk, a.pairs), depth_graphs=True, midas=a.depth == 'midas')
        model = bench.build_model(opt, device, seed=0)
        epoch = opt.warm_sf + 1

        def one_step(i):
            return model._train_on_batch(epoch, i, synthetic.with_loader_dim(batch))
        for i in range(2):                   # HIP-graph set-up, as in bench.py
            one_step(i)
        for i in range(a.warmup):
            log = one_step(i)
        torch.cuda.synchronize()
        b0 = ops.flop_counters()['gather']
        t0 = time.time()
        for i in range(a.steps):
            log = one_step(a.warmup + i)
        torch.cuda.synchronize()
        dt = time.time() - t0
        out.update(value=dt / a.steps * 1e3, ms_per_step=dt / a.steps * 1e3, pairs_per_s=a.pairs * a.steps / dt, steps=a.steps,
                   warmup=a.warmup, graph_setup_steps=2, steps_per_pair_max=model.steps,
                   mlp_chunks=[list(c) for c in model._last_chunks], depth_chunk=model._chunk(),
                   gather_MB_per_step=(ops.flop_counters()['gather'] - b0) / a.steps / 1e6,
                   loss=log['loss'], acc_reg=log['acc_reg'],
                   hbm_peak_allocated_GB=torch.cuda.max_memory_allocated(device) / 2 ** 30)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
