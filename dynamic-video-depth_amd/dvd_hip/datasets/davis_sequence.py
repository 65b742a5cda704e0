"""`--dataset davis_sequence`: the per-video pair-pack reader, and the host -> HBM feeder of the step.

Counterpart of /root/reference/datasets/davis_sequence.py:22-154 (`Dataset`): same flags (:25-33), same file
discovery (`<root>/sequences_select_pairs_midas/<track>/001/shuffle_False_gap_%02d_*.pt` per requested gap, frames
counted from `<root>/frames_midas/<track>/*.npz`, :60-84), and the same sample dict per item (:98-115 for
training packs, :117-153 for validation frames).  The `.pt` pack layout is the one
scripts/preprocess/davis/generate_sequence_midas.py:117-179 writes: a dict of tensors concatenated over the
pairs of the pack on dim 0 (`bs = 1` in the shipped script; any `bs` reads here, so a video can be packed as
48-pair files and one file is one optimisation step).

What is new is the transport.  The reference hands CPU tensors to `NetInterface.load_batch`, which copies them
on the compute stream when the step starts.  `DeviceFeeder` keeps two pinned staging buffers per tensor and a
copy stream: while step i runs, pack i+1 is read (DataLoader workers), staged and copied (0.75 GB per 48-pair
step at 384x672 = ~15 ms on PCIe Gen5), so the step never waits for the host.

`--pairs_per_step N` (new; 0 = one file is one sample, as in the reference): a training sample is N pairs drawn from ALL pack
files of the requested `--gaps` -- the one-pair, one-gap files the reference's preprocessing leaves on disk as they are --
concatenated on dim 0, in an order fixed by a per-epoch shuffle of the pair list that is seeded from the options
(`--manual_seed`, the same on every rank); the last sample of an epoch may be short.  Such a step mixes frame gaps: the model
integrates every pair over its own number of Euler steps (models/scene_flow_motion_field.py, gap_plan).
"""
from glob import glob
from os.path import join

import numpy as np
import torch
import torch.utils.data as data

DATA_ROOT = './datafiles/davis_processed'
FRAME_PREFIX, SEQ_PREFIX = 'frames_midas', 'sequences_select_pairs_midas'


def epoch_pair_order(n_pairs, manual_seed, epoch):
    """The permutation of n_pairs pairs that --pairs_per_step draws its steps from in `epoch`: a function of (--manual_seed,
    epoch) alone, so every rank, `Dataset.pair_order` and datasets/frame_store.py's `Catalogue.order` agree on it."""
    seed = int(manual_seed or 0)
    rng = np.random.RandomState((seed * 1000003 + int(epoch)) % (2 ** 32))
    return [int(i) for i in rng.permutation(int(n_pairs))]


class Dataset(data.Dataset):
    @classmethod
    def add_arguments(cls, parser):
        parser.add_argument('--cache', action='store_true', help='cache the data into ram')
        parser.add_argument('--subsample', action='store_true', help='subsample the video in time')
        parser.add_argument('--track_id', default='train', type=str, help='the track id to load')
        parser.add_argument('--overfit', action='store_true', help='overfit and see if things works')
        parser.add_argument('--gaps', type=str, default='1,2,3,4', help='gaps for sequences')
        parser.add_argument('--repeat', type=int, default=1, help='number of repeatition')
        parser.add_argument('--select', action='store_true', help='pred')
        parser.add_argument('--pairs_per_step', type=int, default=0,
                            help='N > 0: a training sample is N pairs drawn from all pack files of --gaps (mixed frame gaps in '
                                 'one optimisation step), in a seeded per-epoch shuffle; 0: one pack file is one sample')
        return parser, set()

    def __init__(self, opt, mode='train', model=None, data_root=None):
        super().__init__()
        assert mode in ('train', 'vali')
        self.opt, self.mode = opt, mode
        root = data_root or getattr(opt, 'data_root', None) or DATA_ROOT
        track = opt.track_id
        if model is None:
            self.required, self.preproc = ['img', 'flow'], None
        else:
            self.required = model.requires if mode == 'train' else ['img']
            self.preproc = model.preprocess
        if mode == 'train':
            sub = 'subsample' if getattr(opt, 'subsample', False) else '%03d' % 1
            path = join(root, SEQ_PREFIX, track, sub)
            self.file_list = []
            for g in (int(x) for x in opt.gaps.split(',')):
                self.file_list += sorted(glob(join(path, 'shuffle_False_gap_%02d_*.pt' % g)))
            self.n_frames = len(glob(join(root, FRAME_PREFIX, track, '*.npz'))) + 0.0
            self.pairs_per_step = int(getattr(opt, 'pairs_per_step', 0) or 0)
            self.epoch, self._order_of = 0, None
            if self.pairs_per_step > 0:
                # every pair of every file, individually: (file, index in the file)
                self.pair_list = [(f, i) for f, path in enumerate(self.file_list) for i in range(self._pairs_in(path))]
        else:
            self.file_list = sorted(glob(join(root, FRAME_PREFIX, track, '*.npz')))
            self.n_frames = len(self.file_list) + 0.0

    @staticmethod
    def _pairs_in(path):
        try:                        # (memory-mapped: counting the pairs of a pack must not read its images)
            pack = torch.load(path, mmap=True)
        except (TypeError, RuntimeError, ValueError):
            pack = torch.load(path)
        return int(pack['fid_1'].shape[0])

    def set_epoch(self, epoch):
        """The pair order of --pairs_per_step is a function of (--manual_seed, epoch): call before every epoch, with the
        same number on every rank (what DistributedSampler.set_epoch gets)."""
        self.epoch = int(epoch)

    def reset(self):
        """NetInterface.train_epoch's per-epoch `reset_dataset.reset()`: the next epoch's order."""
        self.epoch += 1

    def pair_order(self, epoch=None):
        """--pairs_per_step: the epoch's permutation of the pair list (seeded: two Dataset objects with the same options
        agree, two epochs differ)."""
        epoch = self.epoch if epoch is None else int(epoch)
        if self._order_of is None or self._order_of[0] != epoch:
            self._order_of = (epoch, epoch_pair_order(len(self.pair_list), getattr(self.opt, 'manual_seed', None), epoch))
        return self._order_of[1]

    def _samples_per_epoch(self):
        if self.mode == 'train' and self.pairs_per_step > 0:
            return -(-len(self.pair_list) // self.pairs_per_step)
        return len(self.file_list)

    def __len__(self):
        return self._samples_per_epoch() * (self.opt.repeat if self.mode == 'train' else 1)

    def _mixed_sample(self, idx):
        """--pairs_per_step: sample idx of the epoch = pairs order[idx * N : (idx + 1) * N], keys / dtypes / shapes of a pack
        with bs = N."""
        N = self.pairs_per_step
        order = self.pair_order()
        picks = [self.pair_list[j] for j in order[idx * N:(idx + 1) * N]]
        packs, parts = {}, []
        for f, i in picks:
            if f not in packs:
                packs[f] = self._pack_sample(f)
            parts.append({k: (v[i:i + 1] if (torch.is_tensor(v) or isinstance(v, np.ndarray)) and np.ndim(v) > 0 else v)
                          for k, v in packs[f].items()})
        s = {}
        for k, v in parts[0].items():
            if torch.is_tensor(v) and v.dim() > 0:
                s[k] = torch.cat([p[k] for p in parts], 0)
            elif isinstance(v, np.ndarray) and v.ndim > 0:
                s[k] = np.concatenate([p[k] for p in parts], 0)
            else:
                s[k] = v
        s['pair_path'] = [self.file_list[f] for f, _ in picks]
        return s

    def _pack_sample(self, idx):
        """One pack file as a training sample (:98-115)."""
        s = {}
        pack = torch.load(self.file_list[idx])
        _, H, W, _ = pack['img_1'].shape
        pack['img_1'] = pack['img_1'].permute([0, 3, 1, 2])
        pack['img_2'] = pack['img_2'].permute([0, 3, 1, 2])
        for k, v in pack.items():
            if type(v) != list:
                s[k] = v.float()
        s['time_step'] = (2.0 if getattr(self.opt, 'subsample', False) else 1.0) / self.n_frames
        for i in ('1', '2'):
            s['time_stamp_' + i] = (pack['fid_' + i].reshape([-1, 1, 1, 1]).expand(-1, -1, H, W) / self.n_frames).float()
            s['frame_id_' + i] = np.asarray(pack['fid_' + i])
        return s

    def __getitem__(self, idx):
        if self.mode == 'train' and self.pairs_per_step > 0:
            s = self._mixed_sample(idx % self._samples_per_epoch())
            for k, v in s.items():                       # base_dataset.convert_to_float32
                if isinstance(v, np.ndarray):
                    s[k] = torch.from_numpy(v).float()
            return s
        idx = idx % (self.opt.capat if getattr(self.opt, 'overfit', False) else len(self.file_list))
        unit = 2.0 if getattr(self.opt, 'subsample', False) else 1.0
        s = {}
        if self.mode == 'train':
            s = self._pack_sample(idx)
        else:
            fr = np.load(self.file_list[idx])
            H, W, _ = fr['img'].shape
            s['time_stamp_1'] = np.ones([1, H, W]) * idx / self.n_frames
            s['img'] = np.transpose(fr['img'], [2, 0, 1])
            s['frame_id_1'] = idx
            s['time_step'] = unit / self.n_frames
            s['depth_pred'] = fr['depth_pred'][None, ...]
            s['depth_mvs'] = fr['depth_mvs'][None, ...]
            s['cam_c2w'] = fr['pose_c2w']
            R, t, K = fr['pose_c2w'][:3, :3], fr['pose_c2w'][:3, 3], fr['intrinsics']
            # stored transposed: row vectors multiply from the left (generate_sequence_midas.py:69-76)
            s['R_1'], s['R_1_T'] = R.T.reshape(1, 1, 3, 3).copy(), R.reshape(1, 1, 3, 3).copy()
            s['t_1'] = t.reshape(1, 1, 1, 3).copy()
            s['K'], s['K_inv'] = K.T.reshape(1, 1, 3, 3).copy(), np.linalg.inv(K).T.reshape(1, 1, 3, 3).copy()
        s['pair_path'] = self.file_list[idx]
        for k, v in s.items():                       # base_dataset.convert_to_float32
            if isinstance(v, np.ndarray):
                s[k] = torch.from_numpy(v).float()
        return s


def write_pair_pack(path, batch):
    """Write a (synthetic) batch in the `.pt` layout generate_sequence_midas.py:156-179 produces, so the reader
    above sees exactly what the reference's preprocessing would have left on disk."""
    B, _, H, W = batch['img_1'].shape
    pack = {k: batch[k].cpu() for k in ('R_1', 'R_2', 'R_1_T', 'R_2_T', 't_1', 't_2', 'K', 'K_inv', 'flow_1_2', 'flow_2_1',
                                        'mask_1', 'mask_2', 'motion_seg_1')}
    pack['img_1'] = batch['img_1'].permute(0, 2, 3, 1).contiguous().cpu()          # stored [B,H,W,3] (:148-149)
    pack['img_2'] = batch['img_2'].permute(0, 2, 3, 1).contiguous().cpu()
    pack['depth_1'] = torch.zeros(B, 1, H, W)
    pack['depth_pred_1'] = torch.ones(B, 1, H, W)
    pack['fid_1'], pack['fid_2'] = batch['frame_id_1'].cpu().float(), batch['frame_id_2'].cpu().float()
    torch.save(pack, path)


class DeviceFeeder(object):
    """Iterates over `loader` (batches of CPU tensors) and yields them resident in HBM, one batch ahead of the
    consumer: pinned double-buffered staging + a dedicated copy stream.  The yielded dict is valid until the next
    `next()`; non-tensor entries pass through.

    group_gaps=True: a batch that mixes frame gaps is written into the pinned buffers in gap-grouped order (pairs sorted by
    their Euler step count, stable -- the order the model works in), which costs nothing on the GPU: the model then finds the
    batch grouped and launches no permutation.  The yielded batch, lists of one entry per pair included, is in that order."""

    def __init__(self, loader, device, keys=None, group_gaps=False):
        self.loader, self.device, self.keys, self.group_gaps = loader, torch.device(device), keys, group_gaps
        self.stream = torch.cuda.Stream(device=self.device)
        self.pinned = [dict(), dict()]
        self.copied = [None, None]       # event behind the last H2D copies out of each slot's pinned buffers

    @staticmethod
    def gap_order(batch):
        """(perm, dim, B) that sorts the pairs of a host batch by round((ts2 - ts1) / time_step), stable; perm is None for a
        batch that is grouped already.  dim: the pair dimension (1 behind a DataLoader dimension, else 0)."""
        ts1, ts2, step = batch['time_stamp_1'], batch['time_stamp_2'], batch['time_step']
        dim = max(0, ts1.dim() - 4)
        B = ts1.shape[dim]
        time_step = float(step.flatten()[0]) if torch.is_tensor(step) else float(step)
        steps = ((ts2.float() - ts1.float()).reshape(B, -1)[:, 0] / time_step).round().long().tolist()
        perm = sorted(range(B), key=lambda b: steps[b])
        return (None if perm == list(range(B)) else torch.tensor(perm)), dim, B

    def _stage(self, batch, slot):
        out, pins = {}, self.pinned[slot]
        perm = None
        if self.group_gaps and 'time_stamp_1' in batch:
            perm, pdim, B = self.gap_order(batch)
        if self.copied[slot] is not None:
            # the non-blocking copies issued from this slot two batches ago read the pinned buffers asynchronously: they
            # must have drained before the host overwrites them (a consumer without a per-step host sync would otherwise
            # receive a torn batch)
            self.copied[slot].synchronize()
        with torch.cuda.stream(self.stream):
            for k, v in batch.items():
                if not torch.is_tensor(v) or (self.keys is not None and k not in self.keys) or v.dim() == 0:
                    out[k] = v
                    continue
                buf = pins.get(k)
                if buf is None or buf.shape != v.shape or buf.dtype != v.dtype:
                    buf = torch.empty(v.shape, dtype=v.dtype).pin_memory()
                    pins[k] = buf
                if perm is not None and v.dim() > pdim and v.shape[pdim] == B:
                    torch.index_select(v, pdim, perm, out=buf)
                else:
                    buf.copy_(v)
                out[k] = buf.to(self.device, non_blocking=True)
        if perm is not None:
            for k, v in out.items():
                if isinstance(v, list) and len(v) == B:
                    out[k] = [v[b] for b in perm.tolist()]
        ev = torch.cuda.Event()
        ev.record(self.stream)
        self.copied[slot] = ev
        return out, ev

    def __iter__(self):
        it, slot = iter(self.loader), 0
        try:
            nxt = self._stage(next(it), slot)
        except StopIteration:
            return
        while nxt is not None:
            cur, ev = nxt
            slot ^= 1
            try:
                nxt = self._stage(next(it), slot)        # copy of the next batch overlaps the consumer's step
            except StopIteration:
                nxt = None
            torch.cuda.current_stream(self.device).wait_event(ev)
            for v in cur.values():
                if torch.is_tensor(v) and v.is_cuda:
                    v.record_stream(torch.cuda.current_stream(self.device))
            yield cur

    def __len__(self):
        return len(self.loader)
