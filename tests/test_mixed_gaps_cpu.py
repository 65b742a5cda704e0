"""CPU side of mixed frame gaps in one optimisation step: the gap-group / chunk planner, the per-pair gaps of the synthetic
batches, `--pairs_per_step` of the dataset reader, and the new C entry's place in header, exports and bindings."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GB = 2 ** 30
STASH, GSTASH = 5700 * 32 * 48, 3100 * 32 * 48          # bytes per pair: about the MLP's stash sizes at 32x48


def _today(B, budget, steps, with_reg):
    """Chunk list and byte figures of a uniform-gap step as the model computed them before gaps could be mixed
    (the formulas of its uniform-gap planner path; the model now takes every step's figures from gap_plan)."""
    per_pair = STASH * max(steps, 2 if with_reg else 1) + GSTASH
    Bc = int(max(1, min(B, budget // per_pair)))
    chunks = [(b0, min(B, b0 + Bc)) for b0 in range(0, B, Bc)]
    whole = B * steps * STASH + Bc * (GSTASH + (STASH if (with_reg and steps == 1) else 0))
    chunk = Bc * (STASH * max(steps, 2 if with_reg else 1) + GSTASH)
    return Bc, chunks, whole, chunk


@pytest.mark.parametrize('with_reg', [True, False])
@pytest.mark.parametrize('steps', [0, 1, 2, 4])
@pytest.mark.parametrize('B,budget', [(48, 48.0 * GB), (48, 0.2 * GB), (7, 0.05 * GB), (5, 1e-6 * GB), (1, 1.0 * GB)])
def test_an_all_equal_list_gives_todays_chunks_and_bytes(B, budget, steps, with_reg):
    from dvd_hip.models.scene_flow_motion_field import gap_plan, pairs_per_chunk
    Bc, chunks, whole, chunk = _today(B, budget, steps, with_reg)
    assert pairs_per_chunk(B, budget, STASH, GSTASH, steps, with_reg) == Bc
    plan = gap_plan([steps] * B, budget, STASH, GSTASH, with_reg)
    assert plan['perm'] == list(range(B))
    assert plan['groups'] == [(0, B, steps)]
    assert [(b0, b1) for b0, b1, _ in plan['chunks']] == chunks and all(n == steps for _, _, n in plan['chunks'])
    assert plan['whole_bytes'] == whole and plan['chunk_bytes'] == chunk


@pytest.mark.parametrize('with_reg', [True, False])
@pytest.mark.parametrize('budget', [48.0 * GB, 0.1 * GB, 0.03 * GB, 1e-6 * GB])
@pytest.mark.parametrize('gaps', [[2, 1, 4, 1], [1, 2, 4] * 16, [4, 4, 1, 8, 8, 1, 1, 2, 6, 2, 4], [3, 1], [1, 1, 2, 2]])
def test_groups_are_stable_sorted_and_no_chunk_crosses_a_group(gaps, budget, with_reg):
    from dvd_hip.models.scene_flow_motion_field import gap_plan, pairs_per_chunk
    B = len(gaps)
    plan = gap_plan(gaps, budget, STASH, GSTASH, with_reg)
    perm = plan['perm']
    assert sorted(perm) == list(range(B))                                      # every pair appears once
    assert perm == [b for _, b in sorted((g, b) for b, g in enumerate(gaps))]    # sorted by gap, stable
    grouped = [gaps[b] for b in perm]
    assert [n for _, _, n in plan['groups']] == sorted(set(gaps))
    covered = []
    for b0, b1, n in plan['groups']:
        assert b0 < b1 and grouped[b0:b1] == [n] * (b1 - b0)
        covered += list(range(b0, b1))
    assert covered == list(range(B))
    covered = []
    for b0, b1, n in plan['chunks']:
        assert b0 < b1 and grouped[b0:b1] == [n] * (b1 - b0), 'a chunk crosses a gap group'
        assert b1 - b0 <= pairs_per_chunk(B, budget, STASH, GSTASH, n, with_reg)
        covered += list(range(b0, b1))
    assert covered == list(range(B))
    # forward stashes of the whole batch: sum_b steps_b of them, not B * max steps
    longest = max(b1 - b0 for b0, b1, _ in plan['chunks'])
    gap1 = max([b1 - b0 for b0, b1, n in plan['chunks'] if n == 1] or [0]) if with_reg else 0
    assert plan['whole_bytes'] == sum(gaps) * STASH + longest * GSTASH + gap1 * STASH
    assert plan['whole_bytes'] <= B * max(gaps) * STASH + longest * (GSTASH + STASH)
    assert plan['chunk_bytes'] == max((b1 - b0) * (STASH * max(n, 2 if with_reg else 1) + GSTASH) for b0, b1, n in plan['chunks'])


def test_make_batch_takes_per_pair_gaps():
    from dvd_hip import synthetic
    uni = {g: synthetic.make_batch(4, 8, 12, gap=g, seed=5) for g in (1, 2, 4)}
    same = synthetic.make_batch(4, 8, 12, gap=[2, 2, 2, 2], seed=5)
    assert all(torch.equal(uni[2][k], same[k]) for k in uni[2])
    gaps = [2, 1, 4, 1]
    mixed = synthetic.make_batch(4, 8, 12, gap=gaps, seed=5)
    assert sorted(mixed) == sorted(uni[1])
    for b, g in enumerate(gaps):
        for k, v in mixed.items():
            if v.dim() > 0:
                assert torch.equal(v[b], uni[g][k][b]), (k, b)
    steps = ((mixed['time_stamp_2'] - mixed['time_stamp_1'])[:, 0, 0, 0] / mixed['time_step']).round().long().tolist()
    assert steps == gaps
    with pytest.raises(ValueError):
        synthetic.make_batch(4, 8, 12, gap=[1, 2], seed=5)


# ---- --pairs_per_step ------------------------------------------------------------------------------------------------
GAPS, FRAMES, H, W = (1, 2, 4), 9, 8, 12


def _tree(tmp_path):
    """One-pair packs for gaps 1, 2, 4 over a 9-frame track, as the reference's preprocessing leaves them: 8 + 7 + 5 files."""
    from dvd_hip import synthetic
    from dvd_hip.datasets.davis_sequence import FRAME_PREFIX, SEQ_PREFIX, write_pair_pack
    seq = tmp_path / SEQ_PREFIX / 'train' / '001'
    frames = tmp_path / FRAME_PREFIX / 'train'
    seq.mkdir(parents=True)
    frames.mkdir(parents=True)
    for i in range(FRAMES):
        (frames / ('frame_%05d.npz' % i)).write_bytes(b'')
    n = 0
    for g in GAPS:
        for i in range(FRAMES - g):
            b = synthetic.make_batch(1, H, W, gap=g, seed=1000 * g + i, n_frames=FRAMES)
            b['frame_id_1'] = torch.tensor([float(i)])
            b['frame_id_2'] = torch.tensor([float(i + g)])
            write_pair_pack(str(seq / ('shuffle_False_gap_%02d_%05d.pt' % (g, i))), b)
            n += 1
    return n


def _opt(**over):
    o = dict(track_id='train', gaps='1,2,4', repeat=1, subsample=False, overfit=False, pairs_per_step=0, manual_seed=3)
    o.update(over)
    return SimpleNamespace(**o)


def _pairs_of(sample):
    return list(zip(sample['frame_id_1'].long().tolist(), sample['frame_id_2'].long().tolist()))


def test_pairs_per_step_builds_mixed_steps_from_one_pair_packs(tmp_path):
    from dvd_hip import synthetic
    from dvd_hip.datasets.davis_sequence import Dataset, write_pair_pack
    n = _tree(tmp_path)
    assert n == 20
    N = 6
    ds = Dataset(_opt(pairs_per_step=N), 'train', data_root=str(tmp_path))
    assert len(ds) == 4                                    # 6 + 6 + 6 + 2: the last sample of an epoch is short
    want = sorted((i, i + g) for g in GAPS for i in range(FRAMES - g))
    epochs = []
    for e in range(2):
        ds.set_epoch(e)
        samples = [ds[i] for i in range(len(ds))]
        assert [s['img_1'].shape[0] for s in samples] == [6, 6, 6, 2]
        seen = [p for s in samples for p in _pairs_of(s)]
        assert sorted(seen) == want                        # every pair exactly once per epoch
        epochs.append(seen)
    assert epochs[0] != epochs[1]                          # two epochs differ in order
    assert len({b - a for a, b in epochs[0][:N]}) > 1      # and a step mixes gaps (this seed; 20 pairs over three gaps)
    other = Dataset(_opt(pairs_per_step=N), 'train', data_root=str(tmp_path))
    other.set_epoch(1)
    assert [p for i in range(len(other)) for p in _pairs_of(other[i])] == epochs[1]      # same seed: same list
    ds.set_epoch(0)
    ds.reset()                                             # train_epoch's per-epoch reset moves on to the next order
    assert [p for i in range(len(ds)) for p in _pairs_of(ds[i])] == epochs[1]
    differ = Dataset(_opt(pairs_per_step=N, manual_seed=4), 'train', data_root=str(tmp_path))
    assert [p for i in range(len(differ)) for p in _pairs_of(differ[i])] != epochs[0]
    # keys, dtypes and shapes: those of a pack written with bs = N
    pack = tmp_path / 'pack6.pt'
    write_pair_pack(str(pack), synthetic.make_batch(N, H, W, gap=1, seed=1, n_frames=FRAMES))
    plain = Dataset(_opt(), 'train', data_root=str(tmp_path))
    plain.file_list = [str(pack)]
    ref, got = plain[0], ds[0]
    assert sorted(ref) == sorted(got)
    for k, v in ref.items():
        if torch.is_tensor(v):
            assert got[k].shape == v.shape and got[k].dtype == v.dtype, k
        else:
            assert type(got[k]) is type(v) or k == 'pair_path', k
    assert len(got['pair_path']) == N
    # time stamps follow the pairs
    ts = ((got['time_stamp_2'] - got['time_stamp_1'])[:, 0, 0, 0] / got['time_step']).round().long().tolist()
    assert ts == [b - a for a, b in _pairs_of(got)]


def test_packs_of_several_pairs_contribute_their_pairs_individually(tmp_path):
    from dvd_hip import synthetic
    from dvd_hip.datasets.davis_sequence import SEQ_PREFIX, Dataset, write_pair_pack
    _tree(tmp_path)
    seq = tmp_path / SEQ_PREFIX / 'train' / '001'
    b = synthetic.make_batch(3, H, W, gap=2, seed=77, n_frames=FRAMES)
    b['frame_id_1'], b['frame_id_2'] = torch.tensor([20.0, 21.0, 22.0]), torch.tensor([22.0, 23.0, 24.0])
    write_pair_pack(str(seq / 'shuffle_False_gap_02_99999.pt'), b)
    ds = Dataset(_opt(pairs_per_step=5), 'train', data_root=str(tmp_path))
    assert len(ds.pair_list) == 23 and len(ds) == 5
    seen = [p for i in range(len(ds)) for p in _pairs_of(ds[i])]
    assert len(seen) == 23 and {(20, 22), (21, 23), (22, 24)} <= set(seen)


def test_pairs_per_step_zero_is_one_file_per_sample(tmp_path):
    from dvd_hip.datasets.davis_sequence import Dataset
    n = _tree(tmp_path)
    ds = Dataset(_opt(), 'train', data_root=str(tmp_path))
    none = Dataset(SimpleNamespace(track_id='train', gaps='1,2,4', repeat=2, subsample=False, overfit=False), 'train',
                   data_root=str(tmp_path))                # options from before the flag existed
    assert len(ds) == n and len(none) == 2 * n
    s = ds[3]
    assert s['img_1'].shape == (1, 3, H, W) and s['pair_path'] == ds.file_list[3]
    assert torch.equal(s['img_1'], none[3 + n]['img_1'])
    parser = __import__('argparse').ArgumentParser()
    Dataset.add_arguments(parser)
    assert parser.parse_args([]).pairs_per_step == 0 and parser.parse_args(['--pairs_per_step', '48']).pairs_per_step == 48


# ---- the C entry ----------------------------------------------------------------------------------------------------
def test_gather_pairs_is_in_header_exports_and_bindings_within_abi_8():
    from dvd_hip import _lib, build, ops
    src = open(os.path.join(ROOT, 'include', 'dvd_hip.h')).read()
    assert re.search(r'#define\s+DVD_ABI_VERSION\s+8\b', src)
    assert re.search(r'\bint\s+dvd_gather_pairs\s*\(', re.sub(r'/\*.*?\*/', '', src, flags=re.S))
    assert int(re.search(r'#define\s+DVD_GATHER_MAX\s+(\d+)', src).group(1)) == _lib.GATHER_MAX == 32
    lib = ctypes.CDLL(build.build_library())
    assert hasattr(lib, 'dvd_gather_pairs') and 'dvd_gather_pairs' in _lib.SIGNATURES
    assert _lib.load().dvd_abi_version() == 8 == _lib.ABI_VERSION
    assert ctypes.sizeof(_lib.GatherItem) == 24
    assert 'gather' in ops.BYTE_CLASSES and 'gather' in ops.flop_counters()
    # argument checks happen before any HIP call, so they are testable without a GPU
    items = (_lib.GatherItem * 33)()
    for it in items:
        it.src, it.dst, it.bytes_per_pair = 4096, 8192, 16
    lib = _lib.load()
    assert lib.dvd_gather_pairs(items, 33, ctypes.c_void_p(64), 2, None) == _lib.DVD_EINVAL
    items[0].dst = 4096
    assert lib.dvd_gather_pairs(items, 1, ctypes.c_void_p(64), 2, None) == _lib.DVD_EINVAL
    assert b'overlap' in lib.dvd_last_error()
    assert lib.dvd_gather_pairs(None, 1, ctypes.c_void_p(64), 2, None) == _lib.DVD_EINVAL
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ops.gather_pairs([torch.zeros(2, 3)], [1, 0])
