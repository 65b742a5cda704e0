"""The committed mixed-frame-gap fixtures ARE what tests/golden/make_golden_mixed.py produces from the real reference: where
/root/reference is present it regenerates the three fullstep_mixed_* cases into a scratch directory (after repeating its
self-check of the split-and-combine algebra against the reference's own whole-batch step), and every array must equal the
committed one BIT FOR BIT (as tests/test_sgd_fixtures_regenerate_cpu.py does for its set)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
REF = '/root/reference'
NAMES = ['fullstep_mixed_hourglass_b4_32x48_train.npz', 'fullstep_mixed_hourglass_b4_32x48_warm.npz',
         'fullstep_mixed_hourglass_b4_32x48_wsteps.npz']


@pytest.mark.skipif(not os.path.isdir(REF), reason='the reference tree is only present in the build container')
@pytest.mark.timeout(900)
def test_mixed_gap_fixtures_regenerate_bit_identically(tmp_path):
    env = dict(os.environ, DVD_GOLDEN_OUT=str(tmp_path), OMP_NUM_THREADS='4')
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, 'make_golden_mixed.py')], env=env, capture_output=True,
                       text=True, timeout=850)
    assert r.returncode == 0, r.stderr[-2000:]
    assert 'self-check' in r.stdout
    made = sorted(f for f in os.listdir(tmp_path) if f.endswith('.npz'))
    assert made == NAMES, made
    bad = []
    for f in made:
        new, old = np.load(os.path.join(tmp_path, f), allow_pickle=False), np.load(os.path.join(GOLDEN, f), allow_pickle=False)
        if sorted(new.files) != sorted(old.files):
            bad.append('%s: fields differ: %s' % (f, sorted(set(new.files) ^ set(old.files))))
            continue
        for k in new.files:
            a, b = new[k], old[k]
            if not (a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()):
                bad.append('%s[%s]: not bit-identical' % (f, k))
    assert not bad, '\n'.join(bad)


def test_mixed_gap_fixtures_hold_what_the_gpu_test_reads():
    for f in NAMES:
        gd = np.load(os.path.join(GOLDEN, f), allow_pickle=False)
        assert list(gd['steps_per_pair']) == [2, 1, 4, 1]          # in this (ungrouped) order
        assert list(gd['group_steps']) == [1, 2, 4] and list(gd['group_size']) == [2, 1, 1]
        for k in ('log_loss', 'log_acc_reg', 'grad_norms', 'param_norms_after', 'in_img_1', 'in_time_stamp_2', 'group_S0'):
            assert k in gd.files, (f, k)
        gaps = np.round((gd['in_time_stamp_2'] - gd['in_time_stamp_1'])[:, 0, 0, 0] / float(gd['in_time_step']))
        assert list(gaps.astype(int)) == [2, 1, 4, 1]
        assert os.path.getsize(os.path.join(GOLDEN, f)) < 2 ** 20
