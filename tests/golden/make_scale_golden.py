#!/usr/bin/env python
"""Generate the scale-calibration fixture (scale_calib.npz) from the REAL reference.

Run in the build container only (it reads /root/reference):

    python tests/golden/make_scale_golden.py

scripts/preprocess/shutterstock/generate_frame_midas.py imports skimage, h5py and a MiDaS checkpoint at module level and does its
work in one long loop, so it cannot be imported or called.  Its scale calibration (:153-160) uses only numpy: the statements are
cut out of the reference's source with `ast` (the way tests/ref_exec.py cuts the mask statements of generate_flows.py) and
executed unmodified on seeded inputs -- every line of arithmetic that runs is the reference's own.

Inputs: 5 frames of 24 x 40; a sparse `mvs_depth` (about 30 % above 1e-3, the rest zero or below the threshold), a network
depth of about 1.9 x the MVS depth with noise.  Frame 0 has an even number of selected pixels, frame 1 an odd one.  Stored next
to the inputs: the reference's `scales` (one np.median per frame) and `s` (np.mean of them).  Data only.
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_exec  # noqa: E402

NAME = 'scale_calib'
SCRIPT = os.path.join(ref_exec.REF, 'scripts/preprocess/shutterstock/generate_frame_midas.py')
FIRST, LAST = 153, 160
CASE = dict(N=5, H=24, W=40, seed=2024, thresh=1e-3)


def reference_scale_code():
    """The code object of the statements of lines 153-160: print, `scales = []`, the loop over the frames, `s = np.mean(scales)`."""
    tree = ast.parse(open(SCRIPT).read())
    for node in ast.walk(tree):
        body = getattr(node, 'body', None)
        if not isinstance(body, list):
            continue
        stmts = [s for s in body if isinstance(s, ast.stmt) and FIRST <= s.lineno and getattr(s, 'end_lineno', s.lineno) <= LAST]
        if any(isinstance(s, ast.Assign) and getattr(s.targets[0], 'id', None) == 'scales' for s in stmts):
            kinds = [type(s).__name__ for s in stmts]
            assert kinds == ['Expr', 'Assign', 'For', 'Assign'], 'lines %d-%d: unexpected statements %s' % (FIRST, LAST, kinds)
            assert stmts[3].targets[0].id == 's'
            return compile(ast.Module(body=stmts, type_ignores=[]), SCRIPT, 'exec')
    raise AssertionError('the scale statements were not found at lines %d-%d' % (FIRST, LAST))


def reference_scales(nn_depth, mvs_depth):
    """fp32 [N,H,W] x 2 -> (scales fp32 [N], s) by the reference's statements."""
    env = {'np': np, 'tqdm': lambda it: it, 'hdf5_file_handles': [None] * len(nn_depth), 'depths': list(nn_depth),
           'mvs_depths': list(mvs_depth), 'print': lambda *a: None}
    exec(reference_scale_code(), env)
    return np.asarray(env['scales']), env['s']


def inputs(N, H, W, seed, thresh):
    r = np.random.RandomState(seed)
    mvs = (0.4 + 5.0 * r.rand(N, H, W)).astype(np.float32)
    drop = r.rand(N, H, W) >= 0.3
    mvs[drop] = np.where(r.rand(int(drop.sum())) < 0.7, 0.0, 5e-4).astype(np.float32)
    for frame, parity in ((0, 0), (1, 1)):
        if int((mvs[frame] > thresh).sum()) % 2 != parity:
            y, x = np.argwhere(mvs[frame] > thresh)[0]
            mvs[frame, y, x] = 0.0
    nn = (1.9 * mvs * np.exp(0.2 * r.randn(N, H, W))).astype(np.float32)
    nn[mvs <= thresh] = (0.5 + r.rand(int((mvs <= thresh).sum()))).astype(np.float32)
    return nn, mvs


def main():
    out_dir = os.environ.get('DVD_GOLDEN_OUT', HERE)
    nn, mvs = inputs(**CASE)
    selected = (mvs > CASE['thresh']).reshape(CASE['N'], -1).sum(1)
    assert selected[0] % 2 == 0 and selected[1] % 2 == 1 and 0.2 < selected.sum() / mvs.size < 0.4, selected
    scales, s = reference_scales(nn, mvs)
    assert scales.dtype == np.float32 and scales.shape == (CASE['N'],) and np.asarray(s).dtype == np.float32
    np.savez(os.path.join(out_dir, NAME + '.npz'), in_nn_depth=nn, in_mvs_depth=mvs, thresh=np.float64(CASE['thresh']),
             selected=selected.astype(np.int64), scales=scales, s=np.asarray(s))
    print('wrote %s: selected %s, scales %s, s %r' % (NAME, selected.tolist(), scales.tolist(), float(s)))


if __name__ == '__main__':
    main()
