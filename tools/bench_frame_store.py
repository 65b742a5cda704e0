#!/usr/bin/env python
"""Measure the device-resident frame store (dvd_hip/datasets/frame_store.py) at the headline size: a synthetic video of
--frames frames of 384 x 672, gaps 1-4, 48 pairs per optimisation step.  Prints one JSON line and, with --out, writes it as a
profile stamped with build.source_digest(('frame_store.hip',)).

  gather   event-timed dvd_store_gather of one step's batch, its algorithmic bytes over that time in GB/s, next to the
           6.3 TB/s float4 copy ceiling of the MI355X, and the access path that ran
  step     ms per optimisation step fed by `store.loader` and fed by `DeviceFeeder(DataLoader(Dataset(pairs_per_step=48)))`
           over packs of the SAME pairs (written to --pack_dir by the store's own assembly), alternating blocks of --steps
           steps in one process, --repeats times: mean and spread per path.  The packs of the timed steps stay in the page
           cache between repeats, which flatters the pack path.
  memory   the store's nbytes and the depth-net slots the planner keeps with the store resident

    python tools/bench_frame_store.py --gather_only
    python tools/bench_frame_store.py --steps 2 --repeats 3 --out profiles/frame_store.json

bench.py is not touched by this tool; model and options come from its make_opt / build_model."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'dynamic-video-depth_amd'))

import torch  # noqa: E402

import bench  # noqa: E402

COPY_CEILING_GBPS = 6290.0        # MI355X: measured float4 copy, 79 % of the 8 TB/s HBM3E peak


def synthetic_store(n_frames, H, W, gaps, device, seed=1234):
    """A FrameStore with no files behind it: the writer's pair set of n_frames frames; images, depths, flows and masks drawn on
    the device; cameras like the frames of dvd_hip/synthetic.py's batches (0.01 rad about y and 0.05 along x per frame)."""
    import math
    from dvd_hip.datasets import frame_store as FS
    cat = FS.Catalogue.__new__(FS.Catalogue)
    cat.root, cat.track, cat.gaps, cat.manual_seed = None, 'synthetic', list(gaps), 0
    cat.frame_files = ['synthetic/frame_%05d' % i for i in range(n_frames)]
    cat.pairs = [(f, f + g) for g in gaps for f in range(max(n_frames - 1 - g, 0))]
    cat.pair_files = ['synthetic/flowpair_%05d_%05d' % p for p in cat.pairs]
    store = FS.FrameStore.__new__(FS.FrameStore)
    store._allocate(cat, device, H, W, False, None)
    g = torch.Generator(device=device).manual_seed(seed)
    store.img.uniform_(0.0, 1.0, generator=g)
    store.depth_mvs.uniform_(1.0, 6.0, generator=g)
    store.depth_pred.uniform_(1.0, 6.0, generator=g)
    store.flow_1_2.normal_(0.0, 3.0, generator=g)
    torch.neg(store.flow_1_2, out=store.flow_2_1)
    for m in (store.mask_1, store.mask_2):
        m.copy_(torch.rand(m.shape, device=device, generator=g) >= 0.9)
    import numpy as np
    tab = FS._new_tables(n_frames)
    K = np.array([[0.9 * W, 0.0, (W - 1) / 2.0], [0.0, 0.9 * W, (H - 1) / 2.0], [0.0, 0.0, 1.0]])
    for i in range(n_frames):
        c, sn = math.cos(0.01 * i), math.sin(0.01 * i)
        pose = np.eye(4)
        pose[:3, :3] = [[c, 0.0, sn], [0.0, 1.0, 0.0], [-sn, 0.0, c]]
        pose[:3, 3] = [0.05 * i, 0.0, 0.0]
        FS._set_camera_row(tab, i, pose, K)
    store._set_tables(tab)
    return store


def time_gather(store, pairs, reps=20):
    from dvd_hip import ops
    from dvd_hip.datasets import frame_store as FS
    loader = store.loader(pairs)
    steps, host, index, _ = loader._epoch_tables()
    n = len(steps[0])
    out = {k: v[0] for k, v in loader._buffers(n).items()}
    fields = store.fields()

    def run():
        FS.assemble(fields, out, index[:, :n], host[:, :n])
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    b0 = ops.flop_counters()['gather']
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    nbytes = (ops.flop_counters()['gather'] - b0) / reps
    row = store.H * store.W * 4
    return {'pairs': n, 'tensors': len(out), 'MB_algorithmic': nbytes / 1e6, 'store_gather_ms': ms, 'store_gather_GBps': nbytes / ms / 1e6,
            'copy_ceiling_GBps': COPY_CEILING_GBPS, 'frac_of_copy_ceiling': nbytes / ms / 1e6 / COPY_CEILING_GBPS,
            'access_path': '16-byte' if row % 16 == 0 else ('4-byte' if row % 4 == 0 else 'bytes'),
            'timing_includes': 'the host wrapper (validation, table packing) of every launch'}


def write_packs(store, pairs, n_steps, root, epoch):
    """Packs of the pairs of the epoch's first n_steps steps, written by the store's own assembly in the writer's layout
    (one pair per file), under <root>/sequences_select_pairs_midas/synthetic/001/ -> (file order -> step order) permutation."""
    from dvd_hip.datasets import frame_store as FS
    cat = store.cat
    out_dir = os.path.join(root, 'sequences_select_pairs_midas', cat.track, '001')
    os.makedirs(out_dir)
    os.makedirs(os.path.join(root, 'frames_midas', cat.track))
    for i in range(cat.n_frames):                       # the reader counts the frames by their files
        open(os.path.join(root, 'frames_midas', cat.track, 'frame_%05d.npz' % i), 'w').close()
    triples = [t for s in cat.steps(pairs, epoch)[:n_steps] for t in s]
    names = {}
    for a, b, p in sorted(set(triples)):
        g = b - a
        names[p] = 'shuffle_False_gap_%02d_sequence_%05d.pt' % (g, a)
        one = {k: torch.empty((1,) + shp, device=store.device) for k, shp in FS.item_shapes(store.H, store.W).items()}
        FS.assemble(store.fields(), one, [[a], [b], [p]])
        pack = {k: v.cpu() for k, v in one.items() if not k.startswith('time_stamp')}
        pack['img_1'], pack['img_2'] = (pack[k].permute(0, 2, 3, 1).contiguous() for k in ('img_1', 'img_2'))
        pack['fid_1'], pack['fid_2'] = torch.FloatTensor([a]), torch.FloatTensor([b])
        torch.save(pack, os.path.join(out_dir, names[p]))
    files = sorted(names.values())                      # the reader's file order: gap, then first frame
    return [files.index(names[p]) for _, _, p in triples]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--pairs', type=int, default=bench.PAIRS)
    ap.add_argument('--gaps', type=str, default='1,2,3,4')
    ap.add_argument('--height', type=int, default=bench.H)
    ap.add_argument('--width', type=int, default=bench.W)
    ap.add_argument('--steps', type=int, default=2, help='timed steps per block')
    ap.add_argument('--repeats', type=int, default=3, help='blocks per path, alternating')
    ap.add_argument('--workers', type=int, default=8, help='DataLoader workers of the pack path')
    ap.add_argument('--depth', choices=('midas', 'hourglass'), default='midas')
    ap.add_argument('--pack_dir', type=str, default=None)
    ap.add_argument('--gather_only', action='store_true')
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    from types import SimpleNamespace
    from torch.utils.data import DataLoader
    from dvd_hip import build
    from dvd_hip.datasets.davis_sequence import Dataset, DeviceFeeder
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    gaps = [int(g) for g in a.gaps.split(',')]
    store = synthetic_store(a.frames, a.height, a.width, gaps, device)
    out = {'metric': 'frame store at %dx%d, %d frames, gaps %s, %d pairs per step' % (a.height, a.width, a.frames, gaps, a.pairs),
           'data': 'synthetic', 'device': torch.cuda.get_device_name(device), 'frames': a.frames, 'pairs_in_video': len(store.cat.pairs),
           'store_GB': store.nbytes / 2 ** 30, 'source_digest': build.source_digest(('frame_store.hip',)),
           'gather': time_gather(store, a.pairs)}
    if not a.gather_only:
        epoch, n_steps = 6, a.steps + 1
        root = a.pack_dir or tempfile.mkdtemp(prefix='dvd_packs_')
        try:
            order = write_packs(store, a.pairs, n_steps, root, epoch)
            ds = Dataset(SimpleNamespace(track_id=store.cat.track, gaps=a.gaps, repeat=1, subsample=False, overfit=False,
                                         pairs_per_step=a.pairs, manual_seed=0), mode='train', data_root=root)
            ds._order_of = (0, order)                   # the packs on disk, in the store's step order
            opt = bench.make_opt(depth_chunk=0, depth_graphs=True, midas=a.depth == 'midas')
            model = bench.build_model(opt, device, seed=0)        # after the store: the slot planner sees its memory as taken
            loader = store.loader(a.pairs)
            loader.set_epoch(epoch)

            def store_items():
                for i, item in enumerate(loader):
                    if i >= n_steps:
                        break
                    yield item

            def pack_items():
                return iter(DeviceFeeder(DataLoader(ds, batch_size=1, shuffle=False, num_workers=a.workers), device))

            def block(items):
                """One untimed step (the first item of a path pays its start-up), then the timed ones -> ms per step."""
                it = iter(items)
                model._train_on_batch(opt.warm_sf + 1, 0, next(it))
                torch.cuda.synchronize()
                t0, n, log = time.time(), 0, None
                for item in it:
                    log = model._train_on_batch(opt.warm_sf + 1, n + 1, item)
                    n += 1
                torch.cuda.synchronize()
                return (time.time() - t0) / max(n, 1) * 1e3, log['loss']
            for _ in range(2):                                   # HIP-graph set-up, as in bench.py
                block(store_items())
            ms = {'store': [], 'packs': []}
            losses = {}
            for _ in range(a.repeats):
                for path, items in (('store', store_items), ('packs', pack_items)):
                    t, losses[path] = block(items())
                    ms[path].append(t)
            step = {}
            for path, v in ms.items():
                step[path] = {'ms_per_step': v, 'mean': sum(v) / len(v), 'min': min(v), 'max': max(v)}
            step['store_minus_packs_ms'] = step['store']['mean'] - step['packs']['mean']
            step['spread_ms'] = max(step[p]['max'] - step[p]['min'] for p in ms)
            step['timed_steps_per_block'], step['repeats'], step['pack_workers'] = a.steps, a.repeats, a.workers
            step['last_loss'] = losses
            out['step'] = step
            out['depth_slots_kept'] = len(model._depth._live_slots())
            out['depth_keep_GB'] = model._depth.keep_bytes / 2 ** 30
            out['hbm_peak_allocated_GB'] = torch.cuda.max_memory_allocated(device) / 2 ** 30
        finally:
            if a.pack_dir is None:
                shutil.rmtree(root, ignore_errors=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
