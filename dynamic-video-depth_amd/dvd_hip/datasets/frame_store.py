"""A whole video resident in HBM: training batches straight from the frame and flow-pair files.

The reference's preprocessing leaves `<root>/frames_midas/<track>/frame_%05d.npz` and
`<root>/flow_pairs/<track>/flowpair_%05d_%05d.npz` on disk; scripts/preprocess/davis/generate_sequence_midas.py:117-170 only
re-arranges them into one `.pt` pack per (pair, gap), each with both images of its pair, and datasets/davis_sequence.py:98-115
reads those packs back.  Here every frame and every flow pair is loaded ONCE, onto the device, and that re-arrangement happens
per optimisation step as three index rows (first frame, second frame, flow pair) plus one launch of dvd_store_gather
(csrc/frame_store.hip).  An item of `FrameStore.loader` is what `DeviceFeeder(DataLoader(Dataset(pairs_per_step=N),
batch_size=1))` yields for the same pairs, bit for bit; `FrameStore.frames` is the validation / test view.

  Catalogue   host only: which files, which pairs, in which order per epoch, which pairs per step and rank
  FrameStore  the device tensors, the per-frame camera and time-stamp tables, the two views

The store keeps no CPU path: tests/store_spec.py restates the assembly in plain torch for the tests.
"""
import os
import re
from glob import glob
from os.path import join

import numpy as np
import torch

from .. import ops, parallel
from .davis_sequence import DATA_ROOT, FRAME_PREFIX, epoch_pair_order

FLOW_PREFIX = 'flow_pairs'
CAM_TABLES = ('R_T', 'R', 't', 'K_T', 'K_inv_T')


class Catalogue(object):
    """The files of one track and the pair list of the requested gaps.

    pairs: (f_1, f_2) in the order of `Dataset.pair_list` over the packs the shipped writer leaves: gaps in `gaps` order, f_1
    ascending within a gap, f_2 = f_1 + gap, forward pairs only.  The default pair set is the writer's, f_1 in
    range(N - 1 - gap) (generate_sequence_midas.py:187 leaves out the last possible pair of every gap); all_pairs=True takes
    every flow file of the gap instead."""

    def __init__(self, root=None, track='train', gaps=(1, 2, 3, 4), all_pairs=False, manual_seed=0):
        self.root, self.track = root or DATA_ROOT, track
        self.gaps = [int(g) for g in (gaps.split(',') if isinstance(gaps, str) else gaps)]
        self.manual_seed = int(manual_seed or 0)
        self.frame_files = sorted(glob(join(self.root, FRAME_PREFIX, track, '*.npz')))
        if not self.frame_files:
            raise FileNotFoundError('no frames under %s' % join(self.root, FRAME_PREFIX, track))
        N = len(self.frame_files)
        pdir = join(self.root, FLOW_PREFIX, track)
        on_disk = set()
        for p in glob(join(pdir, 'flowpair_*.npz')):
            m = re.match(r'flowpair_(\d+)_(\d+)\.npz$', os.path.basename(p))
            if m:
                on_disk.add((int(m.group(1)), int(m.group(2))))
        self.pairs = []
        for g in self.gaps:
            if all_pairs:
                firsts = sorted(a for a, b in on_disk if b - a == g and b < N)
            else:
                firsts = list(range(max(N - 1 - g, 0)))
                missing = [f for f in firsts if (f, f + g) not in on_disk]
                if missing:
                    raise FileNotFoundError('gap %d: no flow file for the pair (%d, %d) under %s' % (g, missing[0], missing[0] + g, pdir))
            self.pairs += [(f, f + g) for f in firsts]
        if not self.pairs:
            raise ValueError('no pairs of gaps %s among %d frames' % (self.gaps, N))
        self.pair_files = [join(pdir, 'flowpair_%05d_%05d.npz' % p) for p in self.pairs]

    @property
    def n_frames(self):
        return len(self.frame_files)

    def order(self, epoch, n_pairs=None):
        """The epoch's permutation of the pair list: `Dataset.pair_order` of the same (--manual_seed, epoch).  n_pairs: of its
        first n_pairs entries only (a loader made before FrameStore.add_pairs; None: all)."""
        return epoch_pair_order(len(self.pairs) if n_pairs is None else int(n_pairs), self.manual_seed, epoch)

    def n_steps(self, pairs_per_step, n_pairs=None):
        return -(-(len(self.pairs) if n_pairs is None else int(n_pairs)) // int(pairs_per_step))

    def steps(self, pairs_per_step, epoch, rank=0, world=1, group_gaps=False, n_pairs=None):
        """Per optimisation step of `epoch`, the list of (f_1, f_2, pair) index triples of `rank`: step i holds the pairs
        order[i * N : (i + 1) * N] (the last step may be short), a rank takes parallel.shard_range of them, and
        group_gaps=True sorts what the rank holds by frame gap, stable (the order the model works in).  n_pairs as in `order`."""
        N, order = int(pairs_per_step), self.order(epoch, n_pairs)
        if N <= 0:
            raise ValueError('pairs_per_step must be positive')
        out = []
        for i in range(0, len(order), N):
            picks = order[i:i + N]
            lo, hi = parallel.shard_range(len(picks), rank, world)
            mine = [(self.pairs[j][0], self.pairs[j][1], j) for j in picks[lo:hi]]
            if group_gaps:
                mine.sort(key=lambda t: t[1] - t[0])
            out.append(mine)
        return out


def _cast32(a):
    """The writer's and the reader's cast of a file array: torch.from_numpy(a).float()."""
    return torch.from_numpy(np.ascontiguousarray(a)).float()


def _new_tables(N):
    """The per-frame tables, zeroed, with the two time-stamp tables filled: `Dataset._pack_sample`'s expression (an fp32
    division) for training items, its `vali` item's (a float64 division, then the cast) for validation items."""
    tab = {k: torch.zeros([N, 3] if k == 't' else [N, 3, 3]) for k in CAM_TABLES}
    tab['cam_c2w'] = torch.zeros([N, 4, 4])
    n_frames = N + 0.0
    fid = torch.cat([torch.FloatTensor([i]) for i in range(N)], 0)
    tab['ts_train'] = (fid.reshape([-1, 1, 1, 1]) / n_frames).float().reshape(N).contiguous()
    tab['ts_vali'] = torch.cat([torch.from_numpy(np.ones([1]) * i / n_frames).float() for i in range(N)], 0)
    return tab


def _set_camera_row(tab, i, pose, K):
    """Row i of the camera tables with the writer's own numpy expressions and dtypes (generate_sequence_midas.py:49-76:
    assignment into fp32 tensors casts; the inverse is taken in the file's dtype)."""
    R, t = pose[:3, :3], pose[:3, 3]
    tab['R_T'][i] = torch.from_numpy(R.T)
    tab['R'][i] = torch.from_numpy(R)
    tab['t'][i] = torch.from_numpy(t)
    tab['K_T'][i] = torch.from_numpy(K.T)
    tab['K_inv_T'][i] = torch.from_numpy(np.linalg.inv(K).T)
    tab['cam_c2w'][i] = torch.from_numpy(pose).float()


def camera_tables(host_tables, poses, intrinsics=None):
    """A copy of the per-frame tables `host_tables` (CPU tensors) whose camera rows are rebuilt from `poses`, camera to world
    [N,4,4] (an array or a tensor; cast to fp32), through _set_camera_row.  intrinsics [N,3,3]: new ones; None keeps every row
    of K_T and K_inv_T bit for bit.  The time-stamp tables are carried over."""
    N = int(host_tables['R'].shape[0])
    poses = np.ascontiguousarray((poses.detach().cpu().numpy() if torch.is_tensor(poses) else np.asarray(poses)), dtype=np.float32)
    if poses.shape != (N, 4, 4) or not np.all(np.isfinite(poses)):
        raise ValueError('poses must be finite camera-to-world matrices [%d,4,4], got %s' % (N, poses.shape))
    if intrinsics is not None:
        intrinsics = np.asarray(intrinsics.detach().cpu().numpy() if torch.is_tensor(intrinsics) else intrinsics)
        if intrinsics.shape != (N, 3, 3) or intrinsics.dtype.kind != 'f' or not np.all(np.isfinite(intrinsics)):
            raise ValueError('intrinsics must be finite floating-point matrices [%d,3,3], got %s %s' % (N, intrinsics.dtype, intrinsics.shape))
    tab = {k: v.clone() for k, v in host_tables.items()}
    for i in range(N):
        K = host_tables['K_T'][i].numpy().T if intrinsics is None else intrinsics[i]
        _set_camera_row(tab, i, poses[i], K)
    if intrinsics is None:
        tab['K_T'], tab['K_inv_T'] = host_tables['K_T'].clone(), host_tables['K_inv_T'].clone()
    return tab


def frame_tables(frame_files):
    """The small per-frame tables of a list of frame files, computed on the host (CPU tensors; the kernel only copies them).
    `FrameStore` fills the same tables in its one pass over the files; this is the host-only way to them."""
    tab = _new_tables(len(frame_files))
    for i, path in enumerate(frame_files):
        fr = np.load(path)
        _set_camera_row(tab, i, fr['pose_c2w'], fr['intrinsics'])
    return tab


def item_shapes(H, W):
    """Shape of one pair's entry of every tensor the kernel writes (the reader's layout, datasets/davis_sequence.py:98-115)."""
    shapes = {'img_1': (3, H, W), 'img_2': (3, H, W), 'depth_1': (1, H, W), 'depth_pred_1': (1, H, W),
              'flow_1_2': (H, W, 2), 'flow_2_1': (H, W, 2), 'mask_1': (H, W, 1, 1), 'mask_2': (H, W, 1, 1),
              'motion_seg_1': (H, W, 1, 1), 'time_stamp_1': (1, H, W), 'time_stamp_2': (1, H, W),
              't_1': (1, 1, 1, 3), 't_2': (1, 1, 1, 3)}
    for k in ('R_1', 'R_2', 'R_1_T', 'R_2_T', 'K', 'K_inv'):
        shapes[k] = (1, 1, 3, 3)
    return shapes


def assemble(fields, out, index, host_index=None):
    """ONE dvd_store_gather launch that writes the batch of a step.  fields: the store's device tensors by name (img,
    depth_mvs, depth_pred, motion_seg or None, flow_1_2, flow_2_1, mask_1, mask_2, and the tables R_T, R, t, K_T, K_inv_T,
    ts_train); out: a contiguous fp32 tensor [n, *item_shapes()[key]] per key; index: the three rows f_1, f_2, pair
    (ops.store_gather).  tests/store_spec.py restates in plain torch what this writes."""
    F1, F2, PAIR = 0, 1, 2
    f = fields
    e = [(f['R_T'], 'R_1', 'copy', F1), (f['R_T'], 'R_2', 'copy', F2), (f['R'], 'R_1_T', 'copy', F1),
         (f['R'], 'R_2_T', 'copy', F2), (f['t'], 't_1', 'copy', F1), (f['t'], 't_2', 'copy', F2),
         (f['K_T'], 'K', 'copy', F1), (f['K_inv_T'], 'K_inv', 'copy', F1),
         (f['img'], 'img_1', 'copy', F1), (f['img'], 'img_2', 'copy', F2), (f['depth_mvs'], 'depth_1', 'copy', F1),
         (f['depth_pred'], 'depth_pred_1', 'copy', F1), (f['flow_1_2'], 'flow_1_2', 'copy', PAIR),
         (f['flow_2_1'], 'flow_2_1', 'copy', PAIR), (f['mask_1'], 'mask_1', 'mask', PAIR), (f['mask_2'], 'mask_2', 'mask', PAIR),
         # without a motion segmentation in the frames, motion_seg_1 is the training mask_2 (:152-155)
         ((f['motion_seg'], 'motion_seg_1', 'copy', F1) if f.get('motion_seg') is not None
          else (f['mask_2'], 'motion_seg_1', 'mask', PAIR)),
         (f['ts_train'], 'time_stamp_1', 'fill', F1), (f['ts_train'], 'time_stamp_2', 'fill', F2)]
    if set(out) != set(k for _, k, _, _ in e):
        raise RuntimeError('frame store: outputs %s' % sorted(set(out) ^ set(k for _, k, _, _ in e)))
    ops.store_gather([(src, out[k], op, row) for src, k, op, row in e], index, host_index=host_index)


class FrameStore(object):
    """Every frame and flow pair of a `Catalogue`, resident on `device`; every file is opened once.

    Per frame: img [N,3,H,W] fp32 (transposed at load), depth_mvs and depth_pred [N,1,H,W], motion_seg [N,H,W] fp32 if the files
    carry it.  Per pair: flow_1_2, flow_2_1 [P,H,W,2] fp32, the raw mask_1, mask_2 [P,H,W] uint8 (1 = occluded).  Tables:
    those of frame_tables(), filled in the same pass over the frame files.  Construct it before the model's first training step: the depth net's slot planner reads the free HBM
    when it plans, so it sees the store's memory as taken, the way DVD_RESERVE_GB ballast is seen."""

    def __init__(self, catalogue, device, budget_gb=64.0):
        cat = catalogue
        tab = _new_tables(cat.n_frames)
        for i, path in enumerate(cat.frame_files):          # ONE pass: every frame file is opened once
            fr = np.load(path)
            if i == 0:                                       # the first frame gives the size: budget check, then allocation
                H, W, _ = fr['img'].shape
                self._allocate(cat, device, H, W, 'motion_seg' in fr.files, budget_gb)
            if fr['img'].shape != (H, W, 3):
                raise ValueError('%s: image of shape %s in a video of %d x %d' % (path, fr['img'].shape, H, W))
            self.img[i].copy_(_cast32(fr['img']).permute(2, 0, 1))
            self.depth_mvs[i, 0].copy_(_cast32(fr['depth_mvs']))
            self.depth_pred[i, 0].copy_(_cast32(fr['depth_pred']))
            if self.has_seg:
                self.motion_seg[i].copy_(_cast32(fr['motion_seg']))
            _set_camera_row(tab, i, fr['pose_c2w'], fr['intrinsics'])
        for p, path in enumerate(cat.pair_files):
            fl = np.load(path, allow_pickle=True)
            self.flow_1_2[p].copy_(_cast32(fl['flow_1_2']))
            self.flow_2_1[p].copy_(_cast32(fl['flow_2_1']))
            for name, dst in (('mask_1', self.mask_1), ('mask_2', self.mask_2)):
                m = fl[name]
                if m.dtype == np.bool_:
                    m = m.astype(np.uint8)
                if m.dtype != np.uint8 or m.shape != (H, W):
                    raise ValueError('%s: %s is %s %s, expected uint8 [%d, %d] (generate_flows.py:152-153)' % (
                        path, name, m.dtype, m.shape, H, W))
                dst[p].copy_(torch.from_numpy(np.ascontiguousarray(m)))
        self._set_tables(tab)

    def _allocate(self, cat, device, H, W, has_seg, budget_gb):
        """Sizes, the budget check, then the device tensors (uninitialised)."""
        self.cat, self.device = cat, torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('FrameStore lives on a GPU (dvd_hip has no CPU path), got %s' % self.device)
        N, P = cat.n_frames, len(cat.pairs)
        self.H, self.W, self.has_seg, self.budget_gb = int(H), int(W), bool(has_seg), budget_gb
        per_frame = (5 + (1 if self.has_seg else 0)) * H * W * 4 + (4 * 9 + 3 + 16 + 2) * 4
        per_pair = 4 * H * W * 4 + 2 * H * W
        self.nbytes = N * per_frame + P * per_pair
        if budget_gb is not None and self.nbytes > float(budget_gb) * 2 ** 30:
            raise RuntimeError('frame store: %d frames and %d pairs of %d x %d need %.2f GB, more than --store_gb %.2f' % (
                N, P, H, W, self.nbytes / 2 ** 30, float(budget_gb)))
        dev = self.device
        self.img = torch.empty(N, 3, H, W, device=dev)
        self.depth_mvs = torch.empty(N, 1, H, W, device=dev)
        self.depth_pred = torch.empty(N, 1, H, W, device=dev)
        self.motion_seg = torch.empty(N, H, W, device=dev) if self.has_seg else None
        self.flow_1_2 = torch.empty(P, H, W, 2, device=dev)
        self.flow_2_1 = torch.empty(P, H, W, 2, device=dev)
        self.mask_1 = torch.empty(P, H, W, device=dev, dtype=torch.uint8)
        self.mask_2 = torch.empty(P, H, W, device=dev, dtype=torch.uint8)

    def _set_tables(self, host_tables):
        dev, N = self.device, self.cat.n_frames
        self.host_tables = host_tables
        self.tables = {k: v.to(dev) for k, v in host_tables.items()}
        self.time_step = torch.tensor([1.0 / (N + 0.0)], dtype=torch.float64, device=dev)      # (--subsample is not a store mode)
        self.frame_ids = torch.arange(N, device=dev)
        torch.cuda.synchronize(dev)

    def fields(self):
        f = {k: getattr(self, k) for k in ('img', 'depth_mvs', 'depth_pred', 'motion_seg', 'flow_1_2', 'flow_2_1', 'mask_1', 'mask_2')}
        f.update({k: self.tables[k] for k in CAM_TABLES + ('ts_train',)})
        return f

    def loader(self, pairs_per_step, group_gaps=False, rank=0, world=1, repeat=1):
        return StoreLoader(self, pairs_per_step, group_gaps, rank, world, repeat)

    def add_pairs(self, chained):
        """Appends flow pairs computed on the device -- preprocess.chain_flows' result: 'pairs' [(f_1, f_2)] and flow_1_2,
        flow_2_1 [P',H,W,2] fp32, mask_1, mask_2 [P',H,W] uint8 on the store's device -- to the store's four pair tensors and to
        cat.pairs; cat.pair_files gains a None per pair (no file holds them) and cat.gaps the new gaps.  nbytes grows and the
        budget check is repeated; a pair the store holds already is refused.  Training, preprocess.triangulate_depth and
        Model.evaluate then see the new pairs through cat.pairs like stored ones.  Call it BEFORE store.loader(...): a loader
        made earlier keeps drawing from the pairs it saw when it was made."""
        cat, H, W, dev = self.cat, self.H, self.W, self.flow_1_2.device          # (with its index, which 'cuda' alone lacks)
        try:
            pairs = [(int(a), int(b)) for a, b in chained['pairs']]
            tensors = [chained[k] for k in ('flow_1_2', 'flow_2_1', 'mask_1', 'mask_2')]
        except (KeyError, TypeError, ValueError):
            raise RuntimeError('add_pairs: expected a dict of pairs [(f_1, f_2)], flow_1_2, flow_2_1, mask_1 and mask_2')
        n = len(pairs)
        if n == 0:
            raise RuntimeError('add_pairs: no pair to add')
        have = set(cat.pairs)
        for a, b in pairs:
            if not 0 <= a < b < cat.n_frames:
                raise RuntimeError('add_pairs: the pair (%d, %d) is no forward pair of a video of %d frames' % (a, b, cat.n_frames))
            if (a, b) in have:
                raise RuntimeError('add_pairs: the store holds the pair (%d, %d) already' % (a, b))
            have.add((a, b))
        for k, t in zip(('flow_1_2', 'flow_2_1', 'mask_1', 'mask_2'), tensors):
            shape, dtype = ((n, H, W, 2), torch.float32) if k.startswith('flow') else ((n, H, W), torch.uint8)
            if not (torch.is_tensor(t) and t.device == dev and t.dtype == dtype and tuple(t.shape) == shape):
                raise RuntimeError('add_pairs: %s must be a %s tensor %s on %s' % (k, dtype, list(shape), dev))
        nbytes = self.nbytes + n * (4 * H * W * 4 + 2 * H * W)
        if self.budget_gb is not None and nbytes > float(self.budget_gb) * 2 ** 30:
            raise RuntimeError('frame store: with %d more pairs of %d x %d it needs %.2f GB, more than --store_gb %.2f' % (
                n, H, W, nbytes / 2 ** 30, float(self.budget_gb)))
        self.flow_1_2, self.flow_2_1, self.mask_1, self.mask_2 = (
            torch.cat([getattr(self, k), t], 0) for k, t in zip(('flow_1_2', 'flow_2_1', 'mask_1', 'mask_2'), tensors))
        self.nbytes = nbytes
        cat.pairs += pairs
        cat.pair_files += [None] * n
        cat.gaps += sorted(set(b - a for a, b in pairs) - set(cat.gaps))

    def set_cameras(self, poses, intrinsics=None):
        """Installs other cameras -- preprocess.refine_cameras' 'poses', camera to world [N,4,4] -- so that training and every
        post-processing call use them: the camera rows of host_tables and tables are rebuilt through _set_camera_row
        (camera_tables).  intrinsics [N,3,3]: new ones too; None keeps K_T and K_inv_T as they are.  Nothing else is touched:
        the time-stamp tables, the frames, the flows and the depths stay (a depth scale found with the poses is the caller's
        to apply: store.depth_pred.mul_(scales.view(-1, 1, 1, 1))).  Call it BEFORE store.loader(...): a loader made earlier
        must be remade."""
        tab = camera_tables(self.host_tables, poses, intrinsics)
        self.host_tables = tab
        self.tables = {k: v.to(self.device) for k, v in tab.items()}
        torch.cuda.synchronize(self.device)

    def frames(self, batch_size):
        """The validation / test view: what DataLoader(Dataset(mode='vali'), batch_size=b) yields, on the device.  Images,
        depths and time stamps are views of the store, the cameras slices of the tables; no kernel runs."""
        return StoreFrames(self, batch_size)


class StoreFrames(object):
    def __init__(self, store, batch_size):
        self.store, self.batch_size = store, int(batch_size)

    def __len__(self):
        return -(-self.store.cat.n_frames // self.batch_size)

    def __iter__(self):
        s, T = self.store, self.store.tables
        N, H, W = s.cat.n_frames, s.H, s.W
        for i in range(0, N, self.batch_size):
            j = min(i + self.batch_size, N)
            b = j - i
            yield {'time_stamp_1': T['ts_vali'][i:j].view(b, 1, 1, 1).expand(b, 1, H, W),
                   'img': s.img[i:j], 'frame_id_1': s.frame_ids[i:j], 'time_step': s.time_step.expand(b),
                   'depth_pred': s.depth_pred[i:j], 'depth_mvs': s.depth_mvs[i:j], 'cam_c2w': T['cam_c2w'][i:j],
                   'R_1': T['R_T'][i:j].view(b, 1, 1, 3, 3), 'R_1_T': T['R'][i:j].view(b, 1, 1, 3, 3),
                   't_1': T['t'][i:j].view(b, 1, 1, 1, 3), 'K': T['K_T'][i:j].view(b, 1, 1, 3, 3),
                   'K_inv': T['K_inv_T'][i:j].view(b, 1, 1, 3, 3), 'pair_path': list(s.cat.frame_files[i:j])}


class StoreLoader(object):
    """The training view: an iterable over the optimisation steps of an epoch with __len__, set_epoch and reset, so
    `train_epoch(loader, reset_dataset=loader)` works as with `Dataset`.  Every item is a dict resident in HBM with the keys,
    dtypes, shapes (leading DataLoader dimension of 1 included) and values of the pack path's item; it stays valid until the
    next `next()`: the output buffers are allocated once per step size and written again by every step's launch.  The index
    triples and frame ids of a whole epoch are uploaded once, when the epoch's first item is asked for; a step costs no
    host-to-device copy."""

    def __init__(self, store, pairs_per_step, group_gaps=False, rank=0, world=1, repeat=1):
        self.store, self.pairs_per_step, self.group_gaps = store, int(pairs_per_step), bool(group_gaps)
        self.rank, self.world, self.repeat = int(rank), int(world), max(1, int(repeat))
        if self.pairs_per_step <= 0:
            raise ValueError('pairs_per_step must be positive')
        self.n_pairs = len(store.cat.pairs)        # the pairs it draws from: those the store held when it was made
        self.epoch = 0
        self._uploaded = None         # (epoch, steps, host index [3, total], device index, device frame ids [2, total])
        self._out = {}                # pairs in a step -> output tensors

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def reset(self):
        self.epoch += 1

    def __len__(self):
        return self.store.cat.n_steps(self.pairs_per_step, self.n_pairs) * self.repeat

    def _epoch_tables(self):
        if self._uploaded is None or self._uploaded[0] != self.epoch:
            steps = self.store.cat.steps(self.pairs_per_step, self.epoch, self.rank, self.world, self.group_gaps, self.n_pairs)
            whole = self.store.cat.steps(self.pairs_per_step, self.epoch, n_pairs=self.n_pairs)
            empty = [i for i, s in enumerate(steps) if len(s) == 0]
            if empty:
                raise RuntimeError('frame store: rank %d of %d holds no pair in step %d of epoch %d, a step of %d pair(s); every '
                                   'rank needs at least one' % (self.rank, self.world, empty[0], self.epoch, len(whole[empty[0]])))
            host = np.ascontiguousarray(np.array([t for s in steps for t in s], dtype=np.int32).T)
            dev = self.store.device
            index = torch.from_numpy(host).to(dev)
            fids = torch.from_numpy(host[:2].astype(np.float32)).to(dev)
            self._uploaded = (self.epoch, steps, host, index, fids)
        return self._uploaded[1:]

    def _buffers(self, n):
        out = self._out.get(n)
        if out is None:
            dev = self.store.device
            out = {k: torch.empty((1, n) + shp, device=dev) for k, shp in item_shapes(self.store.H, self.store.W).items()}
            self._out[n] = out
        return out

    def __iter__(self):
        steps, host, index, fids = self._epoch_tables()
        s = self.store
        for _ in range(self.repeat):
            at = 0
            for step in steps:
                n = len(step)
                out = self._buffers(n)
                assemble(s.fields(), {k: v[0] for k, v in out.items()}, index[:, at:at + n], host[:, at:at + n])
                item = dict(out)
                item['fid_1'], item['fid_2'] = fids[0, at:at + n].unsqueeze(0), fids[1, at:at + n].unsqueeze(0)
                item['frame_id_1'], item['frame_id_2'] = item['fid_1'], item['fid_2']
                item['time_step'] = s.time_step
                item['pair_path'] = [(s.cat.pair_files[p],) for _, _, p in step]
                at += n
                yield item
