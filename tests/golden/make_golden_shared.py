#!/usr/bin/env python
"""Generate the shared-frame full-step fixture (fullstep_shared_hourglass_b4_32x48_train.npz) from the REAL reference.

Run in the build container only (it imports /root/reference):

    python tests/golden/make_golden_shared.py            # (tests/test_shared_fixtures_regenerate_cpu.py)

ONE `Model._train_on_batch` of the UNMODIFIED reference on a uniform gap-1 batch whose pairs share frames: the four pairs
(0,1), (1,2), (2,3), (3,4) of a seeded 5-frame 32 x 48 video (tests/store_spec.py: random_tree -> the host tables of
datasets/frame_store.py -> assemble, the way tests/test_37_frame_store_gpu.py's `video32` builds its batches).  The second
image of a pair is bitwise the first image of the next, cameras and frame ids are per frame.  The reference runs its depth net
on all eight images; a step with opt.share_frames runs it on the five distinct ones and must give the same losses, gradients
and parameters (tests/test_39_shared_frames_step_gpu.py).

The fixture stores what the fullstep_* fixtures store (make_golden.py::case_full_step), plus the inputs (`in_*`).

How the seed was chosen (make_golden_mixed.py's criterion, on the REFERENCE alone; nothing of the HIP step enters): at 32x48 the
hourglass's deepest level is 2x3 pixels, and a pre-activation within fp32 rounding of 0 there flips a ReLU when the summation
order changes -- the reference's own gradient norms then depend on its thread count.  The case is only written if every
per-parameter gradient norm agrees to <= 1.5e-5 relative between reference runs at 1, 2 and 8 threads (`conditioning`,
repeated at every run); the seed is the first from 301 upwards that satisfies it.  Measured (`--search`):
seed 301 2.0e-5, 302 3.5e-6, 303 1.7e-5, 304 3.2e-6, 305 8.2e-7, 306 1.4e-5, 307 3.4e-6, 308 4.4e-6.  Hence 302.
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the reference, the package and the repository root on sys.path)
import make_golden_mixed as MM  # noqa: E402

sys.path.insert(0, os.path.join(MG.ROOT, 'tests'))
import helpers  # noqa: E402
import store_spec  # noqa: E402

NAME = 'fullstep_shared_hourglass_b4_32x48_train'
N_FRAMES, H, W, EPOCH = 5, 32, 48, 6
PAIRS = [(0, 1), (1, 2), (2, 3), (3, 4)]
FIRST_SEED, SEED = 301, 302


def video_batch(seed):
    """The four chained gap-1 pairs of the seeded video, as the pack path hands them to the model."""
    from dvd_hip.datasets.frame_store import frame_tables
    fx = store_spec.random_tree(N_FRAMES, H, W, (1,), seed=seed)
    root = tempfile.mkdtemp()
    store_spec.write_tree(root, fx)
    fdir = os.path.join(root, 'frames_midas', store_spec.TRACK)
    fields = store_spec.fixture_fields(fx, frame_tables(sorted(os.path.join(fdir, f) for f in os.listdir(fdir))))
    rows = store_spec.pair_rows(fx)
    batch = store_spec.assemble(fields, [(a, b, rows[(a, b)]) for a, b in PAIRS])
    for k in ('depth_1', 'depth_pred_1'):          # (not inputs of the training step)
        del batch[k]
    batch['frame_id_1'] = torch.tensor([float(a) for a, _ in PAIRS])
    batch['frame_id_2'] = torch.tensor([float(b) for _, b in PAIRS])
    batch['time_step'] = torch.tensor(1.0 / N_FRAMES, dtype=torch.float64)
    # the properties the fixture is for
    for b in range(len(PAIRS) - 1):
        assert torch.equal(batch['img_2'][b], batch['img_1'][b + 1])
        for k2, k1 in (('R_2', 'R_1'), ('R_2_T', 'R_1_T'), ('t_2', 't_1'), ('time_stamp_2', 'time_stamp_1')):
            assert torch.equal(batch[k2][b], batch[k1][b + 1]), k2
    gaps = ((batch['time_stamp_2'] - batch['time_stamp_1'])[:, 0, 0, 0].double() / float(batch['time_step'])).round()
    assert gaps.tolist() == [1.0] * len(PAIRS), gaps
    return batch


def reference_step(batch, seed):
    """One step of a fresh reference model -> (log, model after the step; its .grad are the step's gradients)."""
    model = MM._reference_model(MM._options({}), seed)
    log = model._train_on_batch(EPOCH, 0, helpers.loader_batch({k: (v.clone() if torch.is_tensor(v) else v)
                                                                for k, v in batch.items()}))
    return {k: float(v) for k, v in log.items()}, model


def conditioning(batch, seed):
    """Largest relative difference of a per-parameter gradient norm between reference runs at 1, 2 and 8 threads."""
    norms = []
    for t in (1, 2, 8):
        torch.set_num_threads(t)
        model = reference_step(batch, seed)[1]
        norms.append({k: float(p.grad.double().norm()) for k, p in MM._params(model) if p.grad is not None})
    torch.set_num_threads(4)
    return max(abs(a[k] - norms[2][k]) / norms[2][k] for a in norms[:2] for k in a if norms[2][k] > 0.0)


def write(seed):
    batch = video_batch(seed + 2)
    spread = conditioning(batch, seed)
    print(NAME, 'seed %d: thread spread of the reference\'s gradient norms: %.3e' % (seed, spread))
    if spread > 1.5e-5:
        raise SystemExit('%s: the reference\'s own gradient norms move by %.3e with its thread count (limit 1.5e-5): seed %d '
                         'is ill-conditioned, take the next' % (NAME, spread, seed))
    log, model = reference_step(batch, seed)
    out = {'B': np.array(len(PAIRS)), 'H': np.array(H), 'W': np.array(W), 'gap': np.array(1), 'epoch': np.array(EPOCH),
           'seed': np.array(seed), 'midas': np.array(0), 'n_frames': np.array(N_FRAMES),
           'over_keys': np.array([], dtype='<U1'), 'over_vals': np.array([], dtype=np.float64)}
    for k, v in batch.items():
        out['in_' + k] = v.numpy()
    for k, v in log.items():
        out['log_' + k] = np.array(v, dtype=np.float64)
    names, gnorm, pnorm = [], [], []
    for k, p in MM._params(model):
        names.append(k)
        gnorm.append(0.0 if p.grad is None else float(p.grad.double().norm()))
        pnorm.append(float(p.data.double().norm()))
    out['param_names'] = np.array(names)
    out['grad_norms'] = np.array(gnorm)
    out['param_norms_after'] = np.array(pnorm)
    keep = ['sf/' + k for k in ('convs.0.conv.weight', 'convs.3.conv.bias', 'convs.5.conv.weight', 'convs.5.conv.bias')]
    keep += ['depth/' + k for k in ('net_depth.pred_layer.weight', 'net_depth.seq.0.weight', 'net_depth.seq.1.weight')]
    for k, p in MM._params(model):
        if k in keep and p.grad is not None:
            out['g_' + k] = p.grad.numpy()
            out['p_' + k] = p.data.numpy()
    np.savez_compressed(os.path.join(MG.OUT_DIR, NAME + '.npz'), **out)
    print('wrote', NAME, log)


def search(n=8):
    for seed in range(FIRST_SEED, FIRST_SEED + n):
        print('seed %d: %.3e' % (seed, conditioning(video_batch(seed + 2), seed)), flush=True)


if __name__ == '__main__':
    torch.set_num_threads(4)
    if '--search' in sys.argv:
        search()
    else:
        write(SEED)
