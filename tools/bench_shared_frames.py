#!/usr/bin/env python
"""Measure opt.share_frames (the depth net once per distinct frame of a step) at the headline size: a synthetic video of
--frames frames of 384 x 672 in a device-resident frame store, gaps 1-4, 48 pairs per optimisation step, MiDaS.

ONE model in ONE process runs every step of the epoch's order twice in a row, without and with sharing (opt.share_frames is
read at every step), after --warm untimed steps of each kind (HIP-graph set-up).  Per step it prints the distinct frames U, the
padded union rows U_pad and the ms of both steps; the last line is one JSON record (with --out also written as a profile).

    python tools/bench_shared_frames.py --steps 12 --out profiles/shared_frames.json

Kept slots are keyed by (slot, chunk shape), so with --quantum equal to --depth_chunk (the default: 16 and 16) every union
chunk has the full chunk's shape and the shared steps replay the very slots of the unshared ones; a smaller quantum gives a
tail chunk whose shape changes from step to step, and a slot whose shape changes is captured again (the record says how
many steps captured: `captures`).  bench.py is not touched by this tool; model and options come from its make_opt / build_model,
the store from tools/bench_frame_store.py."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'dynamic-video-depth_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import torch  # noqa: E402

import bench  # noqa: E402
import bench_frame_store  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=80)
    ap.add_argument('--pairs', type=int, default=bench.PAIRS)
    ap.add_argument('--gaps', type=str, default='1,2,3,4')
    ap.add_argument('--height', type=int, default=bench.H)
    ap.add_argument('--width', type=int, default=bench.W)
    ap.add_argument('--steps', type=int, default=6, help='timed steps of each kind')
    ap.add_argument('--warm', type=int, default=2, help='untimed steps of each kind first')
    ap.add_argument('--depth', choices=('midas', 'hourglass'), default='midas')
    ap.add_argument('--depth_chunk', type=int, default=16)
    ap.add_argument('--quantum', type=int, default=16)
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    from dvd_hip import build, ops
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    gaps = [int(g) for g in a.gaps.split(',')]
    store = bench_frame_store.synthetic_store(a.frames, a.height, a.width, gaps, device)
    opt = bench.make_opt(depth_chunk=a.depth_chunk, depth_graphs=True, midas=a.depth == 'midas', share_frames=0,
                         share_quantum=a.quantum)
    model = bench.build_model(opt, device, seed=0)        # after the store: the slot planner sees its memory as taken
    epoch = opt.warm_sf + 1
    loader = store.loader(a.pairs)
    loader.set_epoch(epoch)
    conv = [k for k in ops.FLOP_CLASSES if not k.startswith('mlp_')]

    captures = [0]
    try_capture = model._depth._try_capture

    def counting_capture(*args, **kw):
        captures[0] += 1
        return try_capture(*args, **kw)
    model._depth._try_capture = counting_capture

    def alloc_counts():
        st = torch.cuda.memory_stats(device)
        return st.get('num_alloc_retries', 0), st.get('segment.all.allocated', 0)

    def one(item, share, n):
        opt.share_frames = share
        c0, (r0, s0) = captures[0], alloc_counts()
        f0 = ops.executed_flops()
        torch.cuda.synchronize()
        t0 = time.time()
        log = model._train_on_batch(epoch, n, dict(item))
        torch.cuda.synchronize()
        ms = (time.time() - t0) * 1e3
        f1 = ops.executed_flops()
        r1, s1 = alloc_counts()
        # captured: a slot or graph was captured in this step -- its time is set-up, not a step's.  alloc_retries / new_segments:
        # the caching allocator gave cached blocks back to the device and asked again / asked the device for new segments
        # during this step (both synchronise the device): such a step measures the allocator, not the kernels
        return {'ms': ms, 'loss': log['loss'], 'images': model.depth_images_last_step, 'union': model.last_union,
                'captured': captures[0] > c0, 'alloc_retries': r1 - r0, 'new_segments': s1 - s0,
                'conv_TFLOP': sum(f1[k] - f0[k] for k in conv) / 1e12}

    def items():
        """Full steps of the epoch's order, and of the following epochs' when one epoch has too few."""
        while True:
            got = 0
            for item in loader:
                if item['img_1'].shape[1] == a.pairs:
                    got += 1
                    yield item
            if not got:
                raise SystemExit('the video has no step of %d pairs' % a.pairs)
            loader.reset()

    rows = []
    for n, item in enumerate(items()):
        if n >= a.warm + a.steps:
            break
        plain, shared = one(item, 0, n), one(item, 1, n)
        timed = n >= a.warm
        row = {'step': n, 'timed': timed, 'U': shared['union']['U'], 'U_pad': shared['union']['U_pad'],
               'images_unshared': plain['images'], 'ms_unshared': plain['ms'], 'ms_shared': shared['ms'],
               'conv_TFLOP_unshared': plain['conv_TFLOP'], 'conv_TFLOP_shared': shared['conv_TFLOP'],
               'captured': [plain['captured'], shared['captured']], 'loss': [plain['loss'], shared['loss']],
               'alloc_retries': [plain['alloc_retries'], shared['alloc_retries']],
               'new_segments': [plain['new_segments'], shared['new_segments']]}
        rows.append(row)
        print('step %2d%s  U %3d  U_pad %3d of %3d images  unshared %8.1f ms  shared %8.1f ms%s%s' % (
            n, ' ' if timed else '*', row['U'], row['U_pad'], row['images_unshared'], row['ms_unshared'], row['ms_shared'],
            '  (captured)' if any(row['captured']) else '',
            '  (allocator: retries %s, new segments %s)' % (row['alloc_retries'], row['new_segments'])
            if any(row['alloc_retries'] + row['new_segments']) else ''), flush=True)
    timed = [r for r in rows if r['timed']]
    clean = [r for r in timed if not any(r['captured'])] or timed

    def mean(key, rs):
        return sum(r[key] for r in rs) / max(len(rs), 1)

    def median(key, rs):
        v = sorted(r[key] for r in rs)
        return (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2.0
    out = {'metric': 'opt.share_frames at %dx%d, %d frames, gaps %s, %d pairs per step, %s' % (
               a.height, a.width, a.frames, gaps, a.pairs, a.depth),
           'data': 'synthetic', 'device': torch.cuda.get_device_name(device), 'depth_chunk': a.depth_chunk, 'share_quantum': a.quantum,
           'source_digest': build.source_digest(('frame_union.hip',)), 'steps': rows,
           'timed_steps': len(timed), 'captures': sum(any(r['captured']) for r in timed),
           'mean_U': mean('U', timed), 'mean_U_pad': mean('U_pad', timed), 'images_unshared': 2 * a.pairs,
           'ms_per_step_unshared': mean('ms_unshared', clean), 'ms_per_step_shared': mean('ms_shared', clean),
           'median_ms_per_step_unshared': median('ms_unshared', clean), 'median_ms_per_step_shared': median('ms_shared', clean),
           'min_ms_per_step_unshared': min(r['ms_unshared'] for r in clean), 'min_ms_per_step_shared': min(r['ms_shared'] for r in clean),
           'steps_in_the_means': len(clean),
           'conv_TFLOP_per_step_unshared': mean('conv_TFLOP_unshared', clean), 'conv_TFLOP_per_step_shared': mean('conv_TFLOP_shared', clean),
           'depth_slots_kept': len(model._depth._live_slots()), 'depth_keep_GB': model._depth.keep_bytes / 2 ** 30,
           'hbm_peak_allocated_GB': torch.cuda.max_memory_allocated(device) / 2 ** 30}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
