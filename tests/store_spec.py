"""Executable specification of the frame store's batch assembly, and the fixture plumbing of its tests (test infrastructure).

`assemble` restates in plain torch -- indexing only -- what dvd_hip.datasets.frame_store.assemble writes with one launch of
dvd_store_gather: the re-arrangement of frames and flow pairs into per-pair tensors that the reference does on the host
(scripts/preprocess/davis/generate_sequence_midas.py:117-170, then datasets/davis_sequence.py:98-115).  It lives in the
tests because the product keeps no CPU path.  tests/test_frame_store_cpu.py pins it to the packs the REAL writer produced
(tests/golden/frame_store_{a,b}.npz, made by tests/golden/make_golden_store.py); the GPU tests then use it at shapes that
have no fixture.

The fixtures hold the input arrays of a tiny video tree (`fr_*` per frame, `fl_*` per flow file) and, under `pk_*`, every
key of the writer's packs concatenated over the writer's pair set in `Dataset.pair_list` order (`pk_ids`: gap, f_1, f_2)."""
import os

import numpy as np
import torch

FIXTURES = ('frame_store_a', 'frame_store_b')
TRACK = 'clip'
FRAME_KEYS = ('img', 'depth_pred', 'depth_mvs', 'pose_c2w', 'intrinsics', 'motion_seg')
FLOW_KEYS = ('flow_1_2', 'flow_2_1', 'mask_1', 'mask_2')


def write_tree(root, fx, track=TRACK):
    """The frame and flow-pair files of a fixture under <root>/frames_midas/<track>/ and <root>/flow_pairs/<track>/."""
    fdir, pdir = os.path.join(root, 'frames_midas', track), os.path.join(root, 'flow_pairs', track)
    os.makedirs(fdir)
    os.makedirs(pdir)
    for i in range(int(fx['fr_img'].shape[0])):
        np.savez(os.path.join(fdir, 'frame_%05d.npz' % i), **{k: fx['fr_' + k][i] for k in FRAME_KEYS if 'fr_' + k in fx})
    for j, (a, b) in enumerate(fx['fl_ids'].tolist()):
        np.savez(os.path.join(pdir, 'flowpair_%05d_%05d.npz' % (a, b)), frame_id_1=a, frame_id_2=b,
                 **{k: fx['fl_' + k][j] for k in FLOW_KEYS})


def fixture_packs(fx):
    """[(gap, f_1, f_2, pack dict of tensors with a leading dimension of 1)] in `Dataset.pair_list` order."""
    keys = [k[3:] for k in fx if k.startswith('pk_') and k != 'pk_ids']
    return [(g, a, b, {k: torch.from_numpy(fx['pk_' + k][j:j + 1].copy()) for k in keys})
            for j, (g, a, b) in enumerate(fx['pk_ids'].tolist())]


def write_packs(root, fx, track=TRACK):
    """The fixture's packs as the `.pt` files the shipped writer leaves (:186-193): one pair per file, numbered per gap."""
    out = os.path.join(root, 'sequences_select_pairs_midas', track, '001')
    os.makedirs(out)
    cnt = {}
    for g, _, _, pack in fixture_packs(fx):
        c = cnt.get(g, 0)
        torch.save(pack, os.path.join(out, 'shuffle_False_gap_%02d_sequence_%05d.pt' % (g, c)))
        cnt[g] = c + 1


def dataset_opt(fx, **over):
    from types import SimpleNamespace
    o = dict(track_id=TRACK, gaps=','.join(str(g) for g in fx['gaps'].tolist()), repeat=1, subsample=False, overfit=False,
             cache=False, select=False, pairs_per_step=4, manual_seed=3)
    o.update(over)
    return SimpleNamespace(**o)


def assemble(fields, triples):
    """fields: the store's tensors by name (dvd_hip.datasets.frame_store.assemble), on the CPU; triples: [(f_1, f_2, pair)].
    -> the tensors of the step's batch in the reader's layout, without the DataLoader dimension."""
    f1 = torch.tensor([t[0] for t in triples], dtype=torch.long)
    f2 = torch.tensor([t[1] for t in triples], dtype=torch.long)
    pr = torch.tensor([t[2] for t in triples], dtype=torch.long)
    n = len(triples)
    H, W = fields['img'].shape[-2:]
    out = {'R_1': fields['R_T'][f1].reshape(n, 1, 1, 3, 3), 'R_2': fields['R_T'][f2].reshape(n, 1, 1, 3, 3),
           'R_1_T': fields['R'][f1].reshape(n, 1, 1, 3, 3), 'R_2_T': fields['R'][f2].reshape(n, 1, 1, 3, 3),
           't_1': fields['t'][f1].reshape(n, 1, 1, 1, 3), 't_2': fields['t'][f2].reshape(n, 1, 1, 1, 3),
           'K': fields['K_T'][f1].reshape(n, 1, 1, 3, 3), 'K_inv': fields['K_inv_T'][f1].reshape(n, 1, 1, 3, 3),
           'img_1': fields['img'][f1], 'img_2': fields['img'][f2],
           'depth_1': fields['depth_mvs'][f1].reshape(n, 1, H, W), 'depth_pred_1': fields['depth_pred'][f1].reshape(n, 1, H, W),
           'flow_1_2': fields['flow_1_2'][pr], 'flow_2_1': fields['flow_2_1'][pr]}
    # the files' masks are uint8 with 1 = occluded; a training mask is 1 where the flow is valid
    out['mask_1'] = (1 - fields['mask_1'][pr].float()).reshape(n, H, W, 1, 1)
    out['mask_2'] = (1 - fields['mask_2'][pr].float()).reshape(n, H, W, 1, 1)
    if fields.get('motion_seg') is not None:
        out['motion_seg_1'] = fields['motion_seg'][f1].reshape(n, H, W, 1, 1)
    else:
        out['motion_seg_1'] = out['mask_2'].clone()
    out['time_stamp_1'] = fields['ts_train'][f1].reshape(n, 1, 1, 1).expand(n, 1, H, W).contiguous()
    out['time_stamp_2'] = fields['ts_train'][f2].reshape(n, 1, 1, 1).expand(n, 1, H, W).contiguous()
    return {k: v.contiguous() for k, v in out.items()}


def fixture_fields(fx, tables):
    """The store's tensors for a fixture, on the CPU: its arrays with the casts of the writer (`torch.from_numpy(a).float()`),
    the image transposed as the reader does, and the host tables of dvd_hip.datasets.frame_store.frame_tables.  The pair
    tables hold the flow files of the pairs in `pairs` order -- see `pair_rows`."""
    f = {'img': torch.from_numpy(fx['fr_img']).float().permute(0, 3, 1, 2).contiguous(),
         'depth_mvs': torch.from_numpy(fx['fr_depth_mvs']).float()[:, None], 'depth_pred': torch.from_numpy(fx['fr_depth_pred']).float()[:, None],
         'motion_seg': torch.from_numpy(fx['fr_motion_seg']).float() if 'fr_motion_seg' in fx else None}
    for k in FLOW_KEYS:
        t = torch.from_numpy(fx['fl_' + k])
        f[k] = t.float() if k.startswith('flow') else t
    f.update({k: tables[k] for k in ('R_T', 'R', 't', 'K_T', 'K_inv_T', 'ts_train')})
    return f


def pair_rows(fx):
    """(f_1, f_2) -> row of the fixture's flow arrays."""
    return {(a, b): j for j, (a, b) in enumerate(fx['fl_ids'].tolist())}


def random_fields(n_frames, H, W, seed, with_seg=True):
    """A seeded random store of n_frames frames and every pair of gaps 1 and 2, on the CPU: (fields, pairs)."""
    g = torch.Generator().manual_seed(seed)
    pairs = [(a, a + gap) for gap in (1, 2) for a in range(n_frames - gap)]
    P = len(pairs)
    f = {'img': torch.rand(n_frames, 3, H, W, generator=g), 'depth_mvs': torch.rand(n_frames, 1, H, W, generator=g),
         'depth_pred': torch.rand(n_frames, 1, H, W, generator=g),
         'motion_seg': (torch.rand(n_frames, H, W, generator=g) > 0.5).float() if with_seg else None,
         'flow_1_2': torch.randn(P, H, W, 2, generator=g), 'flow_2_1': torch.randn(P, H, W, 2, generator=g),
         # (any uint8 converts exactly; the files hold 0 and 1)
         'mask_1': torch.randint(0, 2, (P, H, W), generator=g, dtype=torch.uint8),
         'mask_2': torch.randint(0, 256, (P, H, W), generator=g, dtype=torch.uint8),
         'R_T': torch.randn(n_frames, 3, 3, generator=g), 'R': torch.randn(n_frames, 3, 3, generator=g),
         't': torch.randn(n_frames, 3, generator=g), 'K_T': torch.randn(n_frames, 3, 3, generator=g),
         'K_inv_T': torch.randn(n_frames, 3, 3, generator=g), 'ts_train': torch.rand(n_frames, generator=g)}
    return f, pairs


def random_tree(n_frames, H, W, gaps, seed, with_seg=False):
    """A seeded tree at a size that has no fixture, in the fixtures' layout (`fr_*`, `fl_*`, `gaps`): plausible cameras and
    depths, small flows, random occlusion masks."""
    rng = np.random.default_rng(seed)
    fx = {'gaps': np.array(gaps), 'fr_img': rng.random((n_frames, H, W, 3)).astype(np.float32),
          'fr_depth_pred': (1 + 4 * rng.random((n_frames, H, W))).astype(np.float32),
          'fr_depth_mvs': (1 + 4 * rng.random((n_frames, H, W))).astype(np.float32)}
    poses = np.tile(np.eye(4, dtype=np.float32), (n_frames, 1, 1))
    for i in range(n_frames):
        th = 0.01 * i
        poses[i, :3, :3] = [[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]]
        poses[i, :3, 3] = [0.05 * i, 0.0, 0.0]
    K = np.array([[0.9 * W, 0, (W - 1) / 2.0], [0, 0.9 * W, (H - 1) / 2.0], [0, 0, 1.0]], dtype=np.float32)
    fx['fr_pose_c2w'], fx['fr_intrinsics'] = poses, np.tile(K, (n_frames, 1, 1))
    if with_seg:
        fx['fr_motion_seg'] = (rng.random((n_frames, H, W)) > 0.5).astype(np.float32)
    ids = [(a, a + g) for g in gaps for a in range(n_frames - g)]
    fx['fl_ids'] = np.array(ids)
    fx['fl_flow_1_2'] = rng.normal(0.0, 3.0, (len(ids), H, W, 2)).astype(np.float32)
    fx['fl_flow_2_1'] = -fx['fl_flow_1_2']
    fx['fl_mask_1'] = (rng.random((len(ids), H, W)) > 0.9).astype(np.uint8)
    fx['fl_mask_2'] = (rng.random((len(ids), H, W)) > 0.9).astype(np.uint8)
    return fx


def add_spec_packs(fx, tables):
    """`pk_*` for a tree without packs from the real writer: what the specification -- pinned to the writer by
    tests/test_frame_store_cpu.py -- makes of the writer's pair set, in the packs' layout."""
    n = int(fx['fr_img'].shape[0])
    fields, rows = fixture_fields(fx, tables), pair_rows(fx)
    ids = [(g, a, a + g) for g in fx['gaps'].tolist() for a in range(n - 1 - g)]
    items = [assemble(fields, [(a, b, rows[(a, b)])]) for _, a, b in ids]
    fx['pk_ids'] = np.array(ids)
    for k in items[0]:
        if k.startswith('time_stamp'):
            continue
        v = torch.cat([it[k] for it in items], 0)
        fx['pk_' + k] = (v.permute(0, 2, 3, 1) if k in ('img_1', 'img_2') else v).contiguous().numpy()
    fx['pk_fid_1'] = np.array([a for _, a, _ in ids], dtype=np.float32)
    fx['pk_fid_2'] = np.array([b for _, _, b in ids], dtype=np.float32)
    return fx
