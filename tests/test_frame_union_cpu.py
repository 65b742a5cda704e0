"""models/frame_union.py: the host plan of a step that runs the depth net once per distinct frame (opt.share_frames).
Hand-written cases, the refusals, and a property test on random id lists.  No GPU."""
import numpy as np
import pytest

from dvd_hip.models.frame_union import plan_union, table

# id patterns of B = 4 pairs shared with tests/test_38_frame_union_gpu.py: (name, f1, f2)
PATTERNS = [
    ('distinct', [0, 1, 2, 3], [4, 5, 6, 7]),
    ('one_frame', [9, 9, 9, 9], [9, 9, 9, 9]),
    ('both_sets', [3, 5, 7, 8], [5, 9, 10, 3]),
    ('chain', [0, 1, 2, 3], [1, 2, 3, 4]),
    ('order', [7, 2, 7, 5], [2, 0, 5, 7]),
]


def test_all_frames_distinct():
    p = plan_union([0, 1, 2, 3], [4, 5, 6, 7], 1)
    assert (p['B'], p['U'], p['U_pad']) == (4, 8, 8)
    assert p['frames'] == [0, 1, 2, 3, 4, 5, 6, 7]
    assert p['src'] == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3)]
    assert p['u1'] == [0, 1, 2, 3] and p['u2'] == [4, 5, 6, 7]
    assert p['offsets'] == list(range(9)) and p['entries'] == p['src']


def test_one_frame_everywhere():
    p = plan_union([9, 9, 9, 9], [9, 9, 9, 9], 1)
    assert (p['U'], p['U_pad']) == (1, 1)
    assert p['frames'] == [9] and p['src'] == [(0, 0)]
    assert p['u1'] == [0] * 4 and p['u2'] == [0] * 4
    assert p['offsets'] == [0, 8]
    assert p['entries'] == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3)]


def test_a_frame_in_both_sets():
    p = plan_union([3, 5, 7, 8], [5, 9, 10, 3], 1)
    assert p['frames'] == [3, 5, 7, 8, 9, 10] and p['U'] == 6
    assert p['u1'] == [0, 1, 2, 3] and p['u2'] == [1, 4, 5, 0]
    assert p['src'] == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2)]
    assert p['offsets'] == [0, 2, 4, 5, 6, 7, 8]
    assert p['entries'] == [(0, 0), (1, 3), (0, 1), (1, 0), (0, 2), (0, 3), (1, 1), (1, 2)]


def test_the_chain_and_its_padding():
    p = plan_union([0, 1, 2, 3], [1, 2, 3, 4], 8)
    assert (p['U'], p['U_pad']) == (5, 8)
    assert p['frames'] == [0, 1, 2, 3, 4]
    assert p['u1'] == [0, 1, 2, 3] and p['u2'] == [1, 2, 3, 4]
    assert p['src'] == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 3)] + [(0, 0)] * 3        # padding rows copy union row 0
    assert p['offsets'] == [0, 1, 3, 5, 7, 8, 8, 8, 8]                                # three empty ranges at the end
    assert p['entries'] == [(0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (0, 3), (1, 2), (1, 3)]


def test_quantum_one_pads_nothing_and_other_quanta_round_up():
    for q, want in ((1, 5), (2, 6), (3, 6), (5, 5), (6, 6), (8, 8), (16, 16)):
        p = plan_union([0, 1, 2, 3], [1, 2, 3, 4], q)
        assert (p['U'], p['U_pad']) == (5, want), q
        assert len(p['src']) == want and len(p['offsets']) == want + 1 and p['offsets'][5:] == [8] * (want - 4)
    assert plan_union([0], [0], 8)['U_pad'] == 8
    assert plan_union([0, 1, 2, 3], [4, 5, 6, 7], 8)['U_pad'] == 8          # already a multiple: no padding row


def test_first_occurrence_ordering():
    """Set 1 rows 0..B-1 first, then set 2 rows 0..B-1 -- not the order of the ids, not pair by pair."""
    p = plan_union([7, 2, 7, 5], [2, 0, 5, 7], 1)
    assert p['frames'] == [7, 2, 5, 0]
    assert p['src'] == [(0, 0), (0, 1), (0, 3), (1, 1)]
    assert p['u1'] == [0, 1, 0, 2] and p['u2'] == [1, 3, 2, 0]
    assert p['offsets'] == [0, 3, 5, 7, 8]
    assert p['entries'] == [(0, 0), (0, 2), (1, 3), (0, 1), (1, 0), (0, 3), (1, 2), (1, 1)]


def test_numpy_ids_are_taken_as_they_are():
    a = plan_union(np.array([0, 1, 2, 3], dtype=np.int64), np.array([1, 2, 3, 4], dtype=np.int32), np.int64(8))
    assert a == plan_union([0, 1, 2, 3], [1, 2, 3, 4], 8)


@pytest.mark.parametrize('f1,f2,q,match', [
    ([0, -1], [1, 2], 8, 'negative'),
    ([0, 1], [1, -2], 8, 'negative'),
    ([0.0, 1.0], [1, 2], 8, 'integers'),
    ([0, 1], [1, 2.5], 8, 'integers'),
    ([0, 1], ['a', 'b'], 8, 'integers'),
    ([True, False], [1, 2], 8, 'integers'),
    ([0, 1, 2], [1, 2], 8, 'differ in length'),
    ([0, 1], [1, 2], 0, 'share_quantum'),
    ([0, 1], [1, 2], -8, 'share_quantum'),
    ([0, 1], [1, 2], 2.0, 'share_quantum'),
    ([[0, 1]], [[1, 2]], 8, 'one id per image'),
])
def test_refusals(f1, f2, q, match):
    with pytest.raises(ValueError, match=match):
        plan_union(f1, f2, q)


def test_the_uploaded_table_holds_every_part():
    p = plan_union([7, 2, 7, 5], [2, 0, 5, 7], 8)
    flat, where = table(p)
    assert flat.dtype == np.int32 and flat.shape == (8 + 8 + 4 + 4 + 9 + 8,)
    part = {k: flat[o:o + n].tolist() for k, (o, n) in where.items()}
    assert part['set'] == [s for s, _ in p['src']] and part['row'] == [r for _, r in p['src']]
    assert part['u1'] == p['u1'] and part['u2'] == p['u2'] and part['offsets'] == p['offsets']
    assert part['entries'] == [s * 4 + r for s, r in p['entries']]


@pytest.mark.parametrize('seed', range(20))
def test_random_ids_scatter_after_gather_and_csr_partition(seed):
    rng = np.random.RandomState(seed)
    B = int(rng.randint(1, 13))
    n_frames = int(rng.randint(1, 3 * B + 1))
    quantum = int(rng.choice([1, 2, 3, 8, 16]))
    f1, f2 = rng.randint(0, n_frames, size=B), rng.randint(0, n_frames, size=B)
    image_of = rng.rand(n_frames, 3)                 # one "image" per frame id: equal ids show equal images
    sets = (image_of[f1], image_of[f2])
    p = plan_union(f1, f2, quantum)
    U, U_pad = p['U'], p['U_pad']
    assert U == len(set(f1.tolist()) | set(f2.tolist())) and U_pad % quantum == 0 and U <= U_pad < U + quantum
    # gather, then scatter: the per-pair images come back
    img_u = np.stack([sets[s][r] for s, r in p['src']])
    assert img_u.shape[0] == U_pad and all((img_u[u] == img_u[0]).all() for u in range(U, U_pad))
    assert (img_u[p['u1']] == sets[0]).all() and (img_u[p['u2']] == sets[1]).all()
    assert [(f1, f2)[s][r] for s, r in p['src'][:U]] == p['frames']
    # first occurrence: src[u] is the smallest contributor of row u, rows are numbered as they first appear
    off, ent = p['offsets'], p['entries']
    firsts = [ent[off[u]] for u in range(U)]
    assert firsts == p['src'][:U] and firsts == sorted(firsts)
    # the CSR entries partition the 2B rows, each range ascending, padding rows empty
    assert off[0] == 0 and off[-1] == 2 * B and len(off) == U_pad + 1 and off[U:] == [2 * B] * (U_pad - U + 1)
    assert sorted(ent) == [(s, b) for s in (0, 1) for b in range(B)]
    for u in range(U):
        rng_u = ent[off[u]:off[u + 1]]
        assert rng_u and rng_u == sorted(rng_u)
        assert all((p['u1'], p['u2'])[s][b] == u for s, b in rng_u)
