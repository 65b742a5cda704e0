"""opt.share_frames: which DISTINCT frames a step shows, and who shows them (host plan, pure Python / numpy, no GPU).

A step of B pairs holds 2B images, but a real video's step shows most frames several times: with gaps 1-4 one frame is the
first or second image of up to eight pairs.  The reference evaluates `net_depth(img_1)` and `net_depth(img_2)` with the net in
eval() mode (models/scene_flow_motion_field.py:157,168; BatchNorm statistics fixed), so a depth map depends on its image alone:
the depth net may run once per distinct frame, and the k depth gradients of an image shown k times are summed before the one
backward pass.  `plan_union` is the bookkeeping of that; csrc/frame_union.hip moves the rows.
"""
import numbers

import numpy as np


def _ids(f, name):
    """A 1-D sequence of non-negative integer frame ids -> list of ints (ValueError otherwise)."""
    a = np.asarray(f)
    if a.ndim != 1:
        raise ValueError('%s: frame ids must be one id per image, got shape %s' % (name, a.shape))
    out = []
    for v in a.tolist():
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError('%s: frame ids must be integers, got %r' % (name, v))
        if v < 0:
            raise ValueError('%s: frame ids must not be negative, got %r' % (name, v))
        out.append(int(v))
    return out


def plan_union(f1, f2, quantum=8):
    """The union of a step's frames.  f1, f2: the integer frame ids of the two image sets, B each, in the order the step works
    in.  Returns a dict:
      B, U      pairs; distinct frames, ordered by FIRST occurrence scanning set 1 rows 0..B-1 and then set 2 rows 0..B-1;
      U_pad     U rounded up to a multiple of `quantum`: union rows U..U_pad-1 are copies of union row 0 that receive a zero
                gradient (a tail that is a multiple of the quantum bounds the number of distinct depth-net chunk shapes);
      frames    [U] the frame id of union row u;
      src       [U_pad] (set, row): the first occurrence of union row u (padding rows: that of row 0);
      u1, u2    [B] the union row of each pair's first / second image;
      offsets   [U_pad + 1], entries [2B]: a CSR list of the (set, row) contributors of every union row, ascending in
                (set, row); padding rows have none.
    ValueError: ids that are negative or not integers, f1 and f2 of different lengths, a quantum below 1."""
    if isinstance(quantum, bool) or not isinstance(quantum, numbers.Integral) or quantum < 1:
        raise ValueError('share_quantum must be an integer >= 1, got %r' % (quantum,))
    f1, f2 = _ids(f1, 'f1'), _ids(f2, 'f2')
    if len(f1) != len(f2):
        raise ValueError('the two image sets differ in length: %d and %d frame ids' % (len(f1), len(f2)))
    B = len(f1)
    if B == 0:
        raise ValueError('an empty step has no union of frames')
    row_of, frames, src, contrib = {}, [], [], []
    union_rows = ([], [])
    for s, ids in enumerate((f1, f2)):
        for b, fid in enumerate(ids):
            u = row_of.get(fid)
            if u is None:
                u = row_of[fid] = len(frames)
                frames.append(fid)
                src.append((s, b))
                contrib.append([])
            contrib[u].append((s, b))         # the scan order IS ascending (set, row)
            union_rows[s].append(u)
    U = len(frames)
    U_pad = -(-U // int(quantum)) * int(quantum)
    offsets, entries = [0], []
    for u in range(U_pad):
        if u < U:
            entries.extend(contrib[u])
        offsets.append(len(entries))
    return {'B': B, 'U': U, 'U_pad': U_pad, 'frames': frames, 'src': src + [src[0]] * (U_pad - U),
            'u1': union_rows[0], 'u2': union_rows[1], 'offsets': offsets, 'entries': entries}


def table(plan):
    """The plan as the ONE int32 array a step uploads: [set | row | u1 | u2 | offsets | entries] with entries encoded as
    set * B + row, and the (start, length) of every part (ops.UnionTables)."""
    B, U_pad = plan['B'], plan['U_pad']
    parts = (('set', [s for s, _ in plan['src']]), ('row', [r for _, r in plan['src']]), ('u1', plan['u1']), ('u2', plan['u2']),
             ('offsets', plan['offsets']), ('entries', [s * B + r for s, r in plan['entries']]))
    assert [len(v) for _, v in parts] == [U_pad, U_pad, B, B, U_pad + 1, 2 * B]
    flat, where = [], {}
    for name, v in parts:
        where[name] = (len(flat), len(v))
        flat.extend(v)
    return np.asarray(flat, dtype=np.int32), where
