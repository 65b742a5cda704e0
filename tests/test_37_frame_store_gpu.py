"""The device-resident frame store on the GPU: dvd_store_gather (csrc/frame_store.hip) and the two views of
dvd_hip/datasets/frame_store.py.

Everything the store produces is a copy or an exact conversion, so every comparison is bit for bit (same dtype, shape and
values); the one tolerance is the full-step loss tolerance of the project (rtol 1e-5) where two MODELS
take a step on bit-identical inputs.  References: the pack path (`DeviceFeeder(DataLoader(Dataset(pairs_per_step=N)))`
over packs rebuilt from the fixtures the REAL writer produced, tests/golden/make_golden_store.py) and, at shapes without a
fixture, tests/store_spec.py, which tests/test_frame_store_cpu.py pins to those packs."""
import importlib
import os

import numpy as np
import pytest
import torch

import helpers
import store_spec

pytestmark = pytest.mark.gpu

DEV = 'cuda'
PATTERN = 0xA5


def _rebuild(fx, root):
    store_spec.write_tree(root, fx)
    store_spec.write_packs(root, fx)
    return root


def _store(fx, root, **kw):
    from dvd_hip.datasets.frame_store import Catalogue, FrameStore
    cat = Catalogue(root, store_spec.TRACK, fx['gaps'].tolist(), manual_seed=3)
    return FrameStore(cat, DEV, **kw)


def _pack_items(fx, root, pps, epoch, group_gaps=False, repeat=1):
    from torch.utils.data import DataLoader
    from dvd_hip.datasets.davis_sequence import Dataset, DeviceFeeder
    ds = Dataset(store_spec.dataset_opt(fx, pairs_per_step=pps, repeat=repeat), mode='train', data_root=root)
    ds.set_epoch(epoch)
    return list(DeviceFeeder(DataLoader(ds, batch_size=1, shuffle=False), DEV, group_gaps=group_gaps))


def _same_item(got, want, ctx, paths_differ=True):
    assert set(got) == set(want), (ctx, set(got) ^ set(want))
    for k, w in want.items():
        g = got[k]
        if torch.is_tensor(w):
            assert torch.is_tensor(g) and g.is_cuda == w.is_cuda, (ctx, k)
            assert g.dtype == w.dtype and g.shape == w.shape, (ctx, k, g.dtype, w.dtype, tuple(g.shape), tuple(w.shape))
            assert torch.equal(g, w), (ctx, k)
        elif k == 'pair_path' and paths_differ:      # same structure; the store names the flow-pair files, the packs themselves
            assert type(g) == type(w) and len(g) == len(w) and [type(p) for p in g] == [type(p) for p in w], (ctx, g, w)
            assert [len(p) for p in g] == [len(p) for p in w]
        else:
            assert type(g) == type(w) and g == w, (ctx, k, g, w)


@pytest.mark.parametrize('name,pps', [('frame_store_a', 4), ('frame_store_b', 4), ('frame_store_a', 3), ('frame_store_b', 5)])
def test_loader_items_equal_the_pack_path(tmp_path, name, pps):
    """(a, 4): steps of 4 + 3 pairs on the 16-byte path; (b, 4): 4 + 2 at 5 x 7 -- 140-byte rows on the dword path, 35-byte
    masks read bytewise -- and no motion_seg in the frames; (a, 3) and (b, 5) end in a step of ONE pair."""
    fx = helpers.load_golden(name)
    root = _rebuild(fx, str(tmp_path))
    store = _store(fx, root)
    assert store.has_seg == ('fr_motion_seg' in fx)
    loader = store.loader(pps)
    n_pairs = len(fx['pk_ids'])
    for epoch in (0, 1):
        loader.set_epoch(epoch)
        want = _pack_items(fx, root, pps, epoch)
        assert len(loader) == len(want) == -(-n_pairs // pps)
        sizes = []
        for i, item in enumerate(loader):          # (an item is valid until the next one: compared as it comes)
            _same_item(item, want[i], (name, epoch, i))
            sizes.append(item['img_1'].shape[1])
            assert item['img_1'].shape[0] == 1     # the DataLoader dimension
            for path, (_, _, p) in zip(item['pair_path'], store.cat.steps(pps, epoch)[i]):
                assert path == (store.cat.pair_files[p],) and os.path.exists(path[0])
        assert sizes == [pps] * (n_pairs // pps) + ([n_pairs % pps] if n_pairs % pps else [])
    if pps in (3, 5):
        assert sizes[-1] == 1


def test_grouped_loader_equals_the_grouping_feeder(tmp_path):
    fx = helpers.load_golden('frame_store_a')
    root = _rebuild(fx, str(tmp_path))
    loader = _store(fx, root).loader(4, group_gaps=True)
    for epoch in (0, 1, 2):
        loader.set_epoch(epoch)
        for i, (item, want) in enumerate(zip(loader, _pack_items(fx, root, 4, epoch, group_gaps=True))):
            _same_item(item, want, ('grouped', epoch, i))


def test_repeat_walks_the_epoch_order_again_like_the_dataset(tmp_path):
    """`--repeat 2`: the Dataset is twice as long and sample i is sample i % steps of the same epoch order."""
    fx = helpers.load_golden('frame_store_b')
    root = _rebuild(fx, str(tmp_path))
    loader = _store(fx, root).loader(4, repeat=2)
    loader.set_epoch(1)
    want = _pack_items(fx, root, 4, 1, repeat=2)
    assert len(loader) == len(want) == 4
    n = 0
    for i, item in enumerate(loader):
        _same_item(item, want[i], ('repeat', i))
        n += 1
    assert n == 4


def test_epoch_tables_are_uploaded_once_and_reset_moves_on(tmp_path):
    fx = helpers.load_golden('frame_store_b')
    root = _rebuild(fx, str(tmp_path))
    loader = _store(fx, root).loader(4)
    first = [it['fid_1'].clone() for it in loader]
    tables = loader._uploaded
    again = [it['fid_1'].clone() for it in loader]
    assert loader._uploaded is tables and all(torch.equal(a, b) for a, b in zip(first, again))
    loader.reset()
    nxt = [it['fid_1'].clone() for it in loader]
    assert loader._uploaded is not tables and loader.epoch == 1
    assert torch.cat(nxt, 1).sort().values.tolist() == torch.cat(first, 1).sort().values.tolist()
    assert torch.cat(nxt, 1).tolist() != torch.cat(first, 1).tolist()


def test_a_store_over_budget_is_refused_before_it_allocates(tmp_path):
    fx = helpers.load_golden('frame_store_a')
    root = _rebuild(fx, str(tmp_path))
    before = torch.cuda.memory_allocated()
    with pytest.raises(RuntimeError, match='store_gb'):
        _store(fx, root, budget_gb=1e-5)
    assert torch.cuda.memory_allocated() == before
    store = _store(fx, root)
    held = sum(t.numel() * t.element_size() for t in list(store.fields().values()) + [store.tables['cam_c2w'], store.tables['ts_vali']]
               if t is not None)
    assert store.nbytes == held


def _guarded(shape, dtype=torch.float32, pad=64):
    """A tensor inside a larger buffer filled with a byte pattern: (buffer, view, pad)."""
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    buf = torch.full((pad + n + pad,), PATTERN, dtype=torch.uint8, device=DEV)
    return buf, buf[pad:pad + n].view(dtype).view(shape), pad


@pytest.mark.parametrize('n_frames', [2, 7])
@pytest.mark.parametrize('H,W', [(1, 1), (5, 7), (3, 16), (16, 24), (67, 69)])
def test_kernel_edges_against_the_specification(n_frames, H, W):
    """Sizes: one pixel; 5 x 7 (140-byte rows: dwords, masks bytewise); 3 x 16 and 16 x 24 (16-byte accesses); 67 x 69
    (18 492-byte rows: dwords, more than one tile per row; 50 pairs of it make more tiles than the 4 096-block grid, so the
    grid-stride loop runs).  Indices repeat a frame as f_1 of several pairs and as f_1 of one pair and f_2 of another."""
    from dvd_hip.datasets import frame_store as FS
    for with_seg in (True, False):
        fields, pairs = store_spec.random_fields(n_frames, H, W, seed=100 * n_frames + H + (1 if with_seg else 0), with_seg=with_seg)
        dev_fields = {k: (v.to(DEV) if v is not None else None) for k, v in fields.items()}
        rng = np.random.RandomState(n_frames * 1000 + H)
        for n in (1, 3, 50):
            if n_frames == 7:
                # frame 0 as f_1 of two pairs, frame 1 as f_2 of one and f_1 of another
                fixed = [(0, 1), (0, 2), (1, 2)]
                picks = (fixed + [pairs[j] for j in rng.randint(0, len(pairs), size=max(n - 3, 0))])[:n] if n >= 3 else [pairs[3]]
            else:
                picks = [pairs[0]] * n
            triples = [(a, b, pairs.index((a, b))) for a, b in picks]
            want = store_spec.assemble(fields, triples)
            guarded = {k: _guarded((n,) + shp) for k, shp in FS.item_shapes(H, W).items()}
            index = np.array(triples, dtype=np.int32).T
            FS.assemble(dev_fields, {k: g[1] for k, g in guarded.items()}, index)
            torch.cuda.synchronize()
            for k, (buf, view, pad) in guarded.items():
                assert torch.equal(view.cpu(), want[k]), (n_frames, H, W, n, k)       # fully overwritten with the right values
                assert bool((buf[:pad] == PATTERN).all()) and bool((buf[-pad:] == PATTERN).all()), (n_frames, H, W, n, k)
    if (H, W) == (67, 69):
        from dvd_hip import ops
        c0 = ops.flop_counters()['gather']
        FS.assemble(dev_fields, {k: g[1] for k, g in guarded.items()}, index)
        # (the last store has no motion_seg) every output written once, its source read once, three index rows
        out_bytes = sum(g[1].numel() * 4 for g in guarded.values())
        src_bytes = out_bytes - sum(guarded[k][1].numel() * 3 for k in ('mask_1', 'mask_2', 'motion_seg_1')) \
            - sum(guarded[k][1].numel() * 4 - 4 * 50 for k in ('time_stamp_1', 'time_stamp_2'))
        assert ops.flop_counters()['gather'] - c0 == out_bytes + src_bytes + 3 * 4 * 50


def test_byte_path_and_odd_offsets_of_a_plain_copy():
    """COPY of rows whose size or address is no multiple of 4 moves bytes; of 4 but not 16, dwords."""
    from dvd_hip import ops
    g = torch.Generator().manual_seed(5)
    for row, offset in ((13, 0), (13, 3), (5000, 1), (36, 4), (4100, 8)):
        src = torch.randint(0, 256, (6, row), generator=g, dtype=torch.uint8).to(DEV)
        buf = torch.full((64 + offset + 4 * row + 64,), PATTERN, dtype=torch.uint8, device=DEV)
        dst = buf[64 + offset:64 + offset + 4 * row].view(4, row)
        index = np.array([[5, 0, 5, 2], [1, 1, 1, 1], [0, 0, 0, 0]], dtype=np.int32)
        ops.store_gather([(src, dst, 'copy', 0)], index)
        torch.cuda.synchronize()
        assert torch.equal(dst, src[[5, 0, 5, 2]]), (row, offset)
        assert bool((buf[:64 + offset] == PATTERN).all()) and bool((buf[-64:] == PATTERN).all()), (row, offset)


def test_the_kernel_skips_an_index_outside_its_table():
    """The guard inside the kernel, reached through the C ABI (ops.store_gather refuses such an index first): with src_rows
    set BELOW the real table, an index between src_rows and the real size reads valid memory if the guard were missing, and
    must leave its destination row untouched; rows with an index inside are written."""
    import ctypes
    from dvd_hip import _lib
    lib = _lib.load()
    # (every table is rows 1..6 of a larger allocation, so the row in front of it is valid memory as well)
    src = torch.rand(8, 300, device=DEV)[1:7]                  # 1200-byte rows: 16-byte path
    m8 = torch.randint(0, 2, (8, 300), dtype=torch.uint8, device=DEV)[1:7]
    ts = torch.rand(16, device=DEV)[4:10]
    index = torch.tensor([[1, 4, 0, 5, -1], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]], dtype=torch.int32, device=DEV)
    for op, table in ((_lib.STORE_COPY, src), (_lib.STORE_MASK, m8), (_lib.STORE_FILL, ts)):
        dst = torch.full((5, 300), 7.0, device=DEV)
        item = (_lib.StoreItem * 1)()
        item[0].src, item[0].dst, item[0].bytes_per_row, item[0].src_rows, item[0].index_row, item[0].op = \
            table.data_ptr(), dst.data_ptr(), 1200, 3, 0, op
        st = lib.dvd_store_gather(item, 1, ctypes.c_void_p(index.data_ptr()), 5, 5, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == _lib.DVD_OK
        torch.cuda.synchronize()
        want = {_lib.STORE_COPY: src, _lib.STORE_MASK: 1 - m8.float(), _lib.STORE_FILL: ts.view(6, 1).expand(6, 300)}[op]
        assert torch.equal(dst[0], want[1]) and torch.equal(dst[2], want[0]), op
        assert bool((dst[[1, 3, 4]] == 7.0).all()), op          # indices 4, 5 (>= src_rows) and -1: nothing written


def test_the_wrapper_validates_before_it_launches():
    from dvd_hip import ops
    src = torch.rand(5, 8, 6, device=DEV)
    dst = torch.full((3, 8, 6), 7.0, device=DEV)
    m8 = torch.zeros(5, 8, 6, dtype=torch.uint8, device=DEV)
    ts = torch.rand(5, device=DEV)
    ok = np.array([[0, 4, 2], [1, 1, 1], [0, 0, 0]], dtype=np.int32)
    c0 = ops.flop_counters()['gather']
    bad = [
        ('outside its table', [(src, dst, 'copy', 0)], np.array([[0, 5, 2], [1, 1, 1], [0, 0, 0]], dtype=np.int32)),
        ('outside its table', [(src, dst, 'copy', 1)], np.array([[0, 1, 2], [1, -1, 1], [0, 0, 0]], dtype=np.int32)),
        ('outside its table', [(src, dst, 'copy', 0)], torch.tensor([[0, 5, 2], [1, 1, 1], [0, 0, 0]], dtype=torch.int32, device=DEV)),
        ('contiguous', [(src, torch.empty(3, 6, 8, device=DEV).transpose(1, 2), 'copy', 0)], ok),
        ('contiguous', [(src.transpose(1, 2), torch.empty(3, 6, 8, device=DEV), 'copy', 0)], ok),
        ('dtype', [(src, dst.double(), 'copy', 0)], ok),
        ('dtype', [(src, dst, 'mask', 0)], ok),
        ('dtype', [(m8, dst.to(torch.uint8), 'mask', 0)], ok),
        ('dtype', [(ts.double(), dst, 'fill', 0)], ok),
        ('size mismatch', [(src, torch.empty(3, 8, 5, device=DEV), 'copy', 0)], ok),
        ('size mismatch', [(m8, torch.empty(3, 8, 7, device=DEV), 'mask', 0)], ok),
        ('size mismatch', [(src, dst, 'fill', 0)], ok),
        ('three rows', [(src, dst, 'copy', 0)], ok[:, :2]),
        ('GPU tensors', [(src.cpu(), dst, 'copy', 0)], ok),
    ]
    for match, entries, index in bad:
        with pytest.raises(RuntimeError, match=match):
            ops.store_gather(entries, index)
    torch.cuda.synchronize()
    assert ops.flop_counters()['gather'] == c0, 'a refused call reached the library'
    assert bool((dst == 7.0).all())
    ops.store_gather([(src, dst, 'copy', 0)], ok)                      # and the valid call of the same tensors goes through
    assert torch.equal(dst, src[[0, 4, 2]]) and ops.flop_counters()['gather'] > c0
    dst.fill_(7.0)
    ops.store_gather([(m8 + 1, dst, 'mask', 0), ], ok)
    assert bool((dst == 0.0).all())
    ops.store_gather([(ts, dst, 'fill', 0)], ok)
    assert torch.equal(dst, ts[[0, 4, 2]].view(3, 1, 1).expand(3, 8, 6))


@pytest.mark.parametrize('name', store_spec.FIXTURES)
def test_frames_view_equals_the_vali_items(tmp_path, name):
    from torch.utils.data import DataLoader
    from dvd_hip.datasets.davis_sequence import Dataset
    fx = helpers.load_golden(name)
    root = _rebuild(fx, str(tmp_path))
    store = _store(fx, root)
    vali = Dataset(store_spec.dataset_opt(fx), mode='vali', data_root=root)
    want = list(DataLoader(vali, batch_size=2, shuffle=False))
    got = list(store.frames(2))
    assert len(got) == len(want) == len(store.frames(2)) == -(-len(vali) // 2)
    for i, (g, w) in enumerate(zip(got, want)):
        _same_item(g, {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in w.items()}, (name, i), paths_differ=False)
    # views of the store, not copies
    assert got[0]['img'].data_ptr() == store.img.data_ptr() and got[1]['depth_mvs'].data_ptr() == store.depth_mvs[2].data_ptr()


@pytest.fixture(scope='module')
def video32(tmp_path_factory):
    """A 32 x 48 video of 5 frames, gaps 1 and 2 (5 pairs: steps of 4 + 1), packs by the specification."""
    from dvd_hip.datasets.frame_store import frame_tables
    root = str(tmp_path_factory.mktemp('video32'))
    fx = store_spec.random_tree(5, 32, 48, (1, 2), seed=21)
    store_spec.write_tree(root, fx)
    files = sorted(os.path.join(root, 'frames_midas', store_spec.TRACK, f) for f in os.listdir(os.path.join(root, 'frames_midas', store_spec.TRACK)))
    store_spec.add_spec_packs(fx, frame_tables(files))
    store_spec.write_packs(root, fx)
    return fx, root


def test_a_step_runs_from_the_store(video32, tmp_path):
    fx, root = video32
    t35 = importlib.import_module('test_35_mixed_gaps_gpu')
    gd = helpers.load_golden('fullstep_mixed_hourglass_b4_32x48_train')
    epoch = int(gd['epoch'])
    store = _store(fx, root)                 # before the model's first step: the slot planner sees its memory as taken
    loader = store.loader(4)
    loader.set_epoch(epoch)
    packs = _pack_items(fx, root, 4, epoch)
    item = next(iter(loader))
    _same_item(item, packs[0], 'step 0')
    gaps = (item['fid_2'] - item['fid_1'])[0].tolist()
    assert sorted(set(gaps)) == [1.0, 2.0], gaps
    m_store, _ = t35._model(gd)
    m_packs, _ = t35._model(gd)
    a = m_store._train_on_batch(epoch, 0, item)
    b = m_packs._train_on_batch(epoch, 0, packs[0])
    torch.cuda.synchronize()
    print('store step:', {k: a[k] for k in t35.LOSSES}, 'pack step:', {k: b[k] for k in t35.LOSSES})
    assert np.isfinite(a['loss']) and np.isfinite(b['loss'])
    np.testing.assert_allclose(a['loss'], b['loss'], rtol=1e-5)
    assert m_store.steps_per_pair == m_packs.steps_per_pair == [int(g) for g in gaps]
    # a whole epoch through train_epoch, the one-pair last step included
    elog = m_store.train_epoch(loader, epochs=1, initial_epoch=epoch, reset_dataset=loader)
    assert loader.epoch == epoch + 1
    logs = m_store._logger.batch_logs
    assert len(logs) == 2 and all(np.isfinite(l['loss']) for l in logs)
    assert set(m_store._metrics) <= set(elog), set(m_store._metrics) - set(elog)
    assert all(np.isfinite(elog[k]) for k in m_store._metrics)
    # ... and the test view: one batch of frames through test_on_batch, written as .npz
    m_store.opt.output_dir, m_store.opt.epoch = str(tmp_path), 3
    frames = list(store.frames(2))
    out = m_store.test_on_batch(0, frames[1])
    saved = np.load(os.path.join(str(tmp_path), 'epoch0003_test', 'batch0000.npz'))
    assert out['batch_size'] == 2 and saved['depth'].shape == (2, 1, 32, 48) and np.isfinite(saved['depth']).all()
    np.testing.assert_array_equal(saved['img_1'], store.img[2:4].cpu().numpy())
    np.testing.assert_array_equal(saved['depth_gt'], store.depth_mvs[2:4].cpu().numpy())
    log = m_store._vali_on_batch(1, 0, frames[0])
    assert log['size'] == 2 and np.isfinite(log['loss'])
