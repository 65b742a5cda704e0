"""The committed shared-frame fixture IS what tests/golden/make_golden_shared.py produces from the real reference: where
/root/reference is present it regenerates fullstep_shared_hourglass_b4_32x48_train into a scratch directory (after repeating
the conditioning check on the reference's own gradient norms at 1, 2 and 8 threads), and every array must equal the committed
one BIT FOR BIT (as tests/test_mixed_fixtures_regenerate_cpu.py does for its set)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
REF = '/root/reference'
NAME = 'fullstep_shared_hourglass_b4_32x48_train.npz'


@pytest.mark.skipif(not os.path.isdir(REF), reason='the reference tree is only present in the build container')
@pytest.mark.timeout(600)
def test_shared_frame_fixture_regenerates_bit_identically(tmp_path):
    env = dict(os.environ, DVD_GOLDEN_OUT=str(tmp_path), OMP_NUM_THREADS='4')
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, 'make_golden_shared.py')], env=env, capture_output=True,
                       text=True, timeout=550)
    assert r.returncode == 0, r.stderr[-2000:]
    assert 'thread spread' in r.stdout
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith('.npz')) == [NAME]
    new, old = np.load(os.path.join(tmp_path, NAME), allow_pickle=False), np.load(os.path.join(GOLDEN, NAME), allow_pickle=False)
    assert sorted(new.files) == sorted(old.files), sorted(set(new.files) ^ set(old.files))
    bad = [k for k in new.files
           if not (new[k].shape == old[k].shape and new[k].dtype == old[k].dtype and new[k].tobytes() == old[k].tobytes())]
    assert not bad, 'not bit-identical: %s' % bad


def test_shared_frame_fixture_holds_what_the_gpu_test_reads():
    gd = np.load(os.path.join(GOLDEN, NAME), allow_pickle=False)
    assert int(gd['B']) == 4 and (int(gd['H']), int(gd['W'])) == (32, 48) and int(gd['n_frames']) == 5
    for k in ('log_loss', 'log_acc_reg', 'grad_norms', 'param_norms_after', 'in_img_1', 'in_img_2', 'in_frame_id_1',
              'in_time_stamp_2', 'g_sf/convs.0.conv.weight', 'g_depth/net_depth.pred_layer.weight'):
        assert k in gd.files, k
    assert gd['in_frame_id_1'].tolist() == [0, 1, 2, 3] and gd['in_frame_id_2'].tolist() == [1, 2, 3, 4]
    # the chain: the second image of a pair is bitwise the first image of the next, and so are its camera and time stamp
    for k2, k1 in (('img_2', 'img_1'), ('R_2', 'R_1'), ('R_2_T', 'R_1_T'), ('t_2', 't_1'), ('time_stamp_2', 'time_stamp_1')):
        assert gd['in_' + k2][:3].tobytes() == gd['in_' + k1][1:].tobytes(), k2
    assert len({gd['in_img_1'][b].tobytes() for b in range(4)} | {gd['in_img_2'][3].tobytes()}) == 5      # five distinct frames
    gaps = np.round((gd['in_time_stamp_2'] - gd['in_time_stamp_1'])[:, 0, 0, 0] / float(gd['in_time_step']))
    assert list(gaps.astype(int)) == [1, 1, 1, 1]
    norms = dict(zip(gd['param_names'].tolist(), gd['grad_norms'].tolist()))
    assert norms['depth/net_depth.pred_layer.weight'] > 0 and norms['sf/convs.0.conv.weight'] > 0      # a training step
    assert os.path.getsize(os.path.join(GOLDEN, NAME)) < 2 ** 20
