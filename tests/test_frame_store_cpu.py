"""The host side of the device-resident frame store (dvd_hip/datasets/frame_store.py): fixtures, catalogue, host tables, and the
plain-torch specification the GPU tests compare the kernel with.  Nothing here needs a GPU.  Every comparison is bit for bit:
the store only copies, or converts exactly.

The fixtures tests/golden/frame_store_{a,b}.npz hold a tiny video tree and the packs the REAL reference's writer made of it
(tests/golden/make_golden_store.py); trees and packs are rebuilt from them in tmp_path (tests/store_spec.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers
import store_spec

REF = '/root/reference'


@pytest.fixture(scope='module', params=store_spec.FIXTURES)
def tree(request, tmp_path_factory):
    """(fixture arrays, data root with the tree and its packs rebuilt)."""
    fx = helpers.load_golden(request.param)
    root = str(tmp_path_factory.mktemp(request.param))
    store_spec.write_tree(root, fx)
    store_spec.write_packs(root, fx)
    return fx, root


@pytest.fixture(scope='module')
def tree_a(tmp_path_factory):
    fx = helpers.load_golden('frame_store_a')
    root = str(tmp_path_factory.mktemp('tree_a'))
    store_spec.write_tree(root, fx)
    store_spec.write_packs(root, fx)
    return fx, root


def _catalogue(fx, root, **kw):
    from dvd_hip.datasets.frame_store import Catalogue
    return Catalogue(root, store_spec.TRACK, fx['gaps'].tolist(), manual_seed=3, **kw)


def _dataset(fx, root, **over):
    from dvd_hip.datasets.davis_sequence import Dataset
    return Dataset(store_spec.dataset_opt(fx, **over), mode='train', data_root=root)


@pytest.mark.skipif(not os.path.isdir(REF), reason='the reference tree is only present in the build container')
def test_store_fixtures_regenerate_bit_identically(tmp_path):
    env = dict(os.environ, DVD_GOLDEN_OUT=str(tmp_path), OMP_NUM_THREADS='4')
    r = subprocess.run([sys.executable, os.path.join(helpers.GOLDEN, 'make_golden_store.py')], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for name in store_spec.FIXTURES:
        new, old = np.load(os.path.join(str(tmp_path), name + '.npz')), np.load(os.path.join(helpers.GOLDEN, name + '.npz'))
        assert sorted(new.files) == sorted(old.files), name
        for k in new.files:
            a, b = new[k], old[k]
            assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (name, k)


def test_fixtures_are_what_the_issue_describes():
    a, b = (helpers.load_golden(n) for n in store_spec.FIXTURES)
    assert a['fr_img'].shape == (6, 16, 24, 3) and a['fr_pose_c2w'].dtype == a['fr_intrinsics'].dtype == np.float64
    assert 'fr_motion_seg' in a and a['gaps'].tolist() == [1, 2] and len(a['pk_ids']) == 7
    assert b['fr_img'].shape == (5, 5, 7, 3) and b['fr_pose_c2w'].dtype == b['fr_intrinsics'].dtype == np.float32
    assert 'fr_motion_seg' not in b and b['gaps'].tolist() == [1, 2, 3] and len(b['pk_ids']) == 6
    assert sum(os.path.getsize(os.path.join(helpers.GOLDEN, n + '.npz')) for n in store_spec.FIXTURES) < 2 ** 20


def test_pair_list_and_epoch_order_are_the_datasets(tree_a):
    fx, root = tree_a
    cat, ds = _catalogue(fx, root), _dataset(fx, root)
    # Dataset.pair_list names (file, index in the file); the frame ids of those pairs are in the packs
    ds_pairs = []
    for f, i in ds.pair_list:
        pack = torch.load(ds.file_list[f])
        ds_pairs.append((int(pack['fid_1'][i]), int(pack['fid_2'][i])))
    assert cat.pairs == ds_pairs and len(cat.pairs) == 7
    assert cat.pairs == [(g_a_b[1], g_a_b[2]) for g_a_b in fx['pk_ids'].tolist()]
    assert [os.path.basename(p) for p in cat.pair_files[:2]] == ['flowpair_00000_00001.npz', 'flowpair_00001_00002.npz']
    for epoch in (0, 1):
        assert cat.order(epoch) == ds.pair_order(epoch)
        steps = cat.steps(4, epoch)
        assert [len(s) for s in steps] == [4, 3] and len(steps) == cat.n_steps(4) == len(ds)      # the last step is short
        flat = [t for s in steps for t in s]
        assert sorted(t[2] for t in flat) == list(range(7))                                      # every pair exactly once
        assert [t[2] for t in flat] == cat.order(epoch)
        assert all((a, b) == cat.pairs[p] for a, b, p in flat)
    assert cat.order(0) != cat.order(1)
    assert [len(s) for s in cat.steps(3, 0)] == [3, 3, 1]                                        # down to one pair
    # all_pairs: the last possible pair of every gap, which the writer leaves out (:187), and nothing else
    more = _catalogue(fx, root, all_pairs=True)
    assert len(more.pairs) == 9 and set(more.pairs) - set(cat.pairs) == {(4, 5), (3, 5)}
    assert more.pairs == [(a, a + 1) for a in range(5)] + [(a, a + 2) for a in range(4)]


def test_a_missing_flow_file_is_named(tree_a, tmp_path):
    fx, _ = tree_a
    root = str(tmp_path)
    store_spec.write_tree(root, fx)
    os.remove(os.path.join(root, 'flow_pairs', store_spec.TRACK, 'flowpair_00001_00003.npz'))
    with pytest.raises(FileNotFoundError, match=r'\(1, 3\)'):
        _catalogue(fx, root)


@pytest.mark.parametrize('world', [1, 2, 3])
def test_rank_shards_partition_every_step(tree_a, world):
    fx, root = tree_a
    cat = _catalogue(fx, root)
    for pps in (4, 3):
        whole = cat.steps(pps, 1)
        shards = [cat.steps(pps, 1, rank=r, world=world) for r in range(world)]
        for i, step in enumerate(whole):
            assert [t for r in range(world) for t in shards[r][i]] == step      # contiguous shards, in rank order
            sizes = [len(shards[r][i]) for r in range(world)]
            assert max(sizes) - min(sizes) <= 1


def test_grouped_steps_are_sorted_by_gap_stably(tree_a):
    fx, root = tree_a
    cat = _catalogue(fx, root)
    mixed = 0
    for epoch in (0, 1, 2):
        for plain, grouped in zip(cat.steps(4, epoch), cat.steps(4, epoch, group_gaps=True)):
            gaps = [b - a for a, b, _ in plain]
            want = [plain[i] for i in sorted(range(len(plain)), key=lambda i: gaps[i])]       # (sorted() is stable)
            assert grouped == want
            mixed += gaps != sorted(gaps)
    assert mixed > 0, 'no step of these epochs needed sorting: the case tests nothing'


def test_host_tables_equal_the_writers_cameras_and_the_datasets_time_stamps(tree):
    from dvd_hip.datasets.frame_store import frame_tables
    fx, root = tree
    cat, ds = _catalogue(fx, root), _dataset(fx, root)
    tab = frame_tables(cat.frame_files)
    for j, (g, a, b, pack) in enumerate(store_spec.fixture_packs(fx)):
        for key, name, f in (('R_1', 'R_T', a), ('R_2', 'R_T', b), ('R_1_T', 'R', a), ('R_2_T', 'R', b), ('t_1', 't', a),
                             ('t_2', 't', b), ('K', 'K_T', a), ('K_inv', 'K_inv_T', a)):
            got = tab[name][f]
            assert got.dtype == torch.float32 and torch.equal(got.reshape(pack[key].shape), pack[key]), (j, key)
        item = ds._pack_sample(j)             # one pair per pack file
        for key, f in (('time_stamp_1', a), ('time_stamp_2', b)):
            ts = item[key]
            assert ts.dtype == torch.float32 and torch.equal(ts, tab['ts_train'][f].expand_as(ts)), (j, key)
    # the validation item's cameras and time stamp, per frame
    from dvd_hip.datasets.davis_sequence import Dataset
    vali = Dataset(store_spec.dataset_opt(fx), mode='vali', data_root=root)
    assert len(vali) == cat.n_frames
    for i in range(len(vali)):
        it = vali[i]
        for key, name in (('R_1', 'R_T'), ('R_1_T', 'R'), ('t_1', 't'), ('K', 'K_T'), ('K_inv', 'K_inv_T'), ('cam_c2w', 'cam_c2w')):
            assert torch.equal(it[key], tab[name][i].reshape(it[key].shape)), (i, key)
        assert torch.equal(it['time_stamp_1'], tab['ts_vali'][i].expand_as(it['time_stamp_1']))


def test_the_specification_reproduces_every_pack_key_for_key(tree):
    from dvd_hip.datasets.frame_store import frame_tables, item_shapes
    fx, root = tree
    cat, ds = _catalogue(fx, root), _dataset(fx, root)
    fields = store_spec.fixture_fields(fx, frame_tables(cat.frame_files))
    rows = store_spec.pair_rows(fx)
    H, W = fx['fr_img'].shape[1:3]
    for j, (g, a, b, pack) in enumerate(store_spec.fixture_packs(fx)):
        got = store_spec.assemble(fields, [(a, b, rows[(a, b)])])
        assert set(got) == set(item_shapes(H, W))
        assert set(pack) - {'fid_1', 'fid_2'} <= set(got)
        for k, want in pack.items():
            if k in ('fid_1', 'fid_2'):           # built on the host by the loader
                assert float(want) == float(a if k == 'fid_1' else b)
                continue
            mine = got[k].permute(0, 2, 3, 1) if k in ('img_1', 'img_2') else got[k]      # packs store [B,H,W,3] (:148-149)
            assert mine.dtype == want.dtype and mine.shape == want.shape and torch.equal(mine, want), (j, k)
        # ... and the reader's item of that pack, the keys of the pack and the time stamps it adds
        item = ds._pack_sample(j)
        for k, v in got.items():
            assert v.shape == (1,) + item_shapes(H, W)[k]
            assert v.dtype == item[k].dtype and v.shape == item[k].shape and torch.equal(v, item[k]), (j, k)
    # a step of several pairs is the concatenation of its pairs
    triples = [(a, b, rows[(a, b)]) for _, a, b, _ in store_spec.fixture_packs(fx)][::-1]
    many = store_spec.assemble(fields, triples)
    for i, t in enumerate(triples):
        one = store_spec.assemble(fields, [t])
        for k in one:
            assert torch.equal(many[k][i:i + 1], one[k]), k


def test_store_gather_checks_its_arguments_before_any_hip_call():
    import ctypes
    from dvd_hip import _lib, ops
    lib = _lib.load()
    assert lib.dvd_abi_version() == _lib.ABI_VERSION == 8
    null = ctypes.c_void_p(0)
    assert lib.dvd_store_gather(None, 1, null, 4, 4, null) == _lib.DVD_EINVAL
    assert b'null' in lib.dvd_last_error()
    items = (_lib.StoreItem * (_lib.STORE_MAX + 1))()
    for it in items:
        it.src, it.dst, it.bytes_per_row, it.src_rows, it.index_row, it.op = 4096, 8192, 32, 2, 0, _lib.STORE_COPY
    fake = ctypes.c_void_p(64)              # never dereferenced: every call below is refused on its arguments
    assert lib.dvd_store_gather(items, 1, fake, 4, 0, null) == _lib.DVD_EINVAL                  # an empty batch
    assert lib.dvd_store_gather(items, _lib.STORE_MAX + 1, fake, 4, 4, null) == _lib.DVD_EINVAL  # too many entries
    assert b'tensors' in lib.dvd_last_error()
    assert lib.dvd_store_gather(items, 0, fake, 4, 4, null) == _lib.DVD_EINVAL
    items[0].op = 7
    assert lib.dvd_store_gather(items, 1, fake, 4, 4, null) == _lib.DVD_EINVAL
    items[0].op, items[0].dst = _lib.STORE_COPY, 4096 + 32
    assert lib.dvd_store_gather(items, 1, fake, 4, 4, null) == _lib.DVD_EINVAL                  # overlapping src / dst
    assert b'overlap' in lib.dvd_last_error()
    with pytest.raises(RuntimeError, match='GPU tensors'):
        ops.store_gather([(torch.zeros(2, 4), torch.zeros(3, 4), 'copy', 0)], np.zeros((3, 3), dtype=np.int32))


def test_the_dataset_alias_resolves():
    from dvd_hip.datasets import get_dataset
    import argparse
    D = get_dataset('davis_frames')
    parser, _ = D.add_arguments(argparse.ArgumentParser())
    a = parser.parse_args(['--gaps', '1,2', '--pairs_per_step', '4', '--store_gb', '2'])
    assert a.store_gb == 2.0 and a.pairs_per_step == 4 and a.track_id == 'train'
