"""The committed long-range track fixture IS what tests/golden/make_golden_tracks.py produces from the real reference: where
/root/reference is present it is regenerated into a scratch directory, and every array must equal the committed one BIT FOR BIT
(as tests/test_resize_fixture_regenerates_cpu.py does for the MiDaS working-resolution fixture)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
REF = '/root/reference'
NAME = 'tracks_b3_11x21_t4.npz'


@pytest.mark.skipif(not os.path.isdir(REF), reason='the reference tree is only present in the build container')
@pytest.mark.timeout(300)
def test_tracks_fixture_regenerates_bit_identically(tmp_path):
    env = dict(os.environ, DVD_GOLDEN_OUT=str(tmp_path), OMP_NUM_THREADS='4')
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, 'make_golden_tracks.py')], env=env, capture_output=True, text=True,
                       timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith('.npz')) == [NAME]
    new, old = np.load(os.path.join(tmp_path, NAME), allow_pickle=False), np.load(os.path.join(GOLDEN, NAME), allow_pickle=False)
    assert sorted(new.files) == sorted(old.files), sorted(set(new.files) ^ set(old.files))
    bad = [k for k in new.files
           if not (new[k].shape == old[k].shape and new[k].dtype == old[k].dtype and new[k].tobytes() == old[k].tobytes())]
    assert not bad, 'not bit-identical: %s' % bad
