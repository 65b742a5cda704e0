"""CPU side of the scene-flow step's plan (dvd_hip/models/sf_step.py): the schedule choice against the rule as it stood inline
in `Model._train_on_batch`, the byte figures and step counts against values recorded from the Model methods that computed them
before the module existed, and the image sets of phases 1 and 3.  No GPU, no library."""
from types import SimpleNamespace

import pytest
import torch

HW = 32 * 48
STASH, GSTASH = 1425 * HW * 4, 775 * HW * 4          # bytes per pair and evaluation handed to plan_step below


# (Bc, whole, B, use_cnn, mlp_recompute) -> (this rank's schedule, needs_late_normaliser, the schedule once another rank asks
# for the late normaliser).  Written out from the inline rule: recompute = Bc < B and not whole and mlp_recompute; the flag is
# not (whole or Bc >= B or recompute); then `if late / elif recompute / else` whole batch; --use_cnn ignores all of it.
SCHEDULES = [
    ((4, False, 4, False, 1), ('whole', False, 'late')),            # one chunk
    ((4, False, 4, False, 0), ('whole', False, 'late')),
    ((7, False, 4, False, 1), ('whole', False, 'late')),            # (Bc >= B)
    ((2, True, 4, False, 1), ('whole', False, 'late')),             # several chunks that fit whole
    ((2, True, 4, False, 0), ('whole', False, 'late')),
    ((2, False, 4, False, 1), ('recompute', False, 'late')),        # several chunks that do not fit
    ((2, False, 4, False, 0), ('late', True, 'late')),
    ((1, False, 2, False, 1), ('recompute', False, 'late')),
    ((4, False, 4, True, 1), ('unet', False, 'unet')),              # --use_cnn, as plan_step fills Bc / whole for it
    ((4, False, 4, True, 0), ('unet', False, 'unet')),
    ((2, False, 4, True, 0), ('unet', False, 'unet')),              # ... and whatever else a plan might say
    ((2, True, 4, True, 1), ('unet', False, 'unet')),
]


@pytest.mark.parametrize('case,expected', SCHEDULES)
def test_choose_schedule_is_the_inline_rule(case, expected):
    from dvd_hip.models.sf_step import agreed_schedule, choose_schedule
    Bc, whole, B, use_cnn, rec = case
    local, needs_late, forced = expected
    schedule, flag = choose_schedule({'Bc': Bc, 'whole': whole}, B, use_cnn, bool(rec))
    assert (schedule, flag) == (local, needs_late)
    assert agreed_schedule(schedule, flag) == local              # alone, or every rank agrees: the local choice stands
    assert agreed_schedule(schedule, True) == forced             # another rank needs the late normaliser
    if not use_cnn:                                              # the same, spelled as the rule was
        recompute = Bc < B and not whole and bool(rec)
        assert flag == (not (whole or Bc >= B or recompute))
        for late in (flag, True):
            assert agreed_schedule(schedule, late) == ('late' if late else 'recompute' if recompute else 'whole')


# (MLP?, options, steps per pair, do_reg) -> plan entries, recorded from the former Model._plan_step with stash / gstash sizes
# of 1425 / 775 floats per pixel at 32x48 (the --use_cnn rows: no `Bc` / `whole` then; `measured`: Model._cnn_px_measured)
PLANS = [
    (True, {'mlp_stash_gb': 48.0, 'mlp_whole_batch_gb': 160.0}, [1, 1, 1, 1], True,
     {'perm': [0, 1, 2, 3], 'groups': [(0, 4, 1)], 'chunks': [(0, 4, 1)], 'Bc': 4, 'whole': False, 'reserve': 89677824}),
    (True, {'mlp_stash_gb': 0.05, 'mlp_whole_batch_gb': 160.0}, [2, 2, 2, 2], True,
     {'perm': [0, 1, 2, 3], 'groups': [(0, 4, 2)], 'chunks': [(0, 2, 2), (2, 4, 2)], 'Bc': 2, 'whole': True, 'reserve': 80154624}),
    (True, {'mlp_stash_gb': 0.05, 'mlp_whole_batch_gb': 0.0}, [2, 2, 2, 2], False,
     {'perm': [0, 1, 2, 3], 'groups': [(0, 4, 2)], 'chunks': [(0, 2, 2), (2, 4, 2)], 'Bc': 2, 'whole': False, 'reserve': 45133824}),
    (True, {'mlp_stash_gb': 48.0}, [2, 1, 4, 1], True,          # (no mlp_whole_batch_gb attribute: the 160 GB default)
     {'perm': [1, 3, 0, 2], 'groups': [(0, 2, 1), (2, 3, 2), (3, 4, 4)], 'chunks': [(0, 2, 1), (2, 3, 2), (3, 4, 4)], 'Bc': 2,
      'whole': True, 'reserve': 97665024}),
    (True, {'mlp_stash_gb': 0.03, 'mlp_whole_batch_gb': 160.0}, [2, 1, 4, 1], True,
     {'perm': [1, 3, 0, 2], 'groups': [(0, 2, 1), (2, 3, 2), (3, 4, 4)], 'chunks': [(0, 1, 1), (1, 2, 1), (2, 3, 2), (3, 4, 4)],
      'Bc': 1, 'whole': True, 'reserve': 84148224}),
    (True, {'mlp_stash_gb': 0.03, 'mlp_whole_batch_gb': 0.0}, [2, 1, 4, 1], True,
     {'perm': [1, 3, 0, 2], 'groups': [(0, 2, 1), (2, 3, 2), (3, 4, 4)], 'chunks': [(0, 1, 1), (1, 2, 1), (2, 3, 2), (3, 4, 4)],
      'Bc': 1, 'whole': False, 'reserve': 40372224}),
    (True, {'mlp_stash_gb': 0.03, 'mlp_whole_batch_gb': 0.0}, [2, 1, 4, 1], False,
     {'perm': [1, 3, 0, 2], 'groups': [(0, 2, 1), (2, 3, 2), (3, 4, 4)], 'chunks': [(0, 2, 1), (2, 3, 2), (3, 4, 4)], 'Bc': 2,
      'whole': False, 'reserve': 40372224}),
    (False, {'n_down': 3}, [1, 1, 1, 1], True,
     {'perm': [0, 1, 2, 3], 'groups': [(0, 4, 1)], 'chunks': [(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1)], 'reserve': 48513024.0}),
    (False, {'n_down': 4}, [2, 1, 4, 1], False,
     {'perm': [1, 3, 0, 2], 'groups': [(0, 2, 1), (2, 3, 2), (3, 4, 4)], 'chunks': [(0, 1, 1), (1, 2, 1), (2, 3, 2), (3, 4, 4)],
      'reserve': 55701504.0}),
    (False, {'n_down': 3, 'measured': 5000.0}, [2, 1, 4, 1], True,
     {'perm': [1, 3, 0, 2], 'groups': [(0, 2, 1), (2, 3, 2), (3, 4, 4)], 'chunks': [(0, 1, 1), (1, 2, 1), (2, 3, 2), (3, 4, 4)],
      'reserve': 92749824.0}),
]


def _plan(mlp, options, steps_pp, do_reg):
    from dvd_hip.models.sf_step import cnn_bytes_per_px, plan_step
    options = dict(options)
    measured = options.pop('measured', 0.0)
    opt = SimpleNamespace(**options)
    return plan_step(steps_pp, HW, do_reg, (STASH, GSTASH) if mlp else None, cnn_bytes_per_px(measured, opt), opt)


@pytest.mark.parametrize('mlp,options,steps_pp,do_reg,expected', PLANS)
def test_plan_step_gives_the_recorded_figures(mlp, options, steps_pp, do_reg, expected):
    plan = _plan(mlp, options, steps_pp, do_reg)
    assert {k: plan[k] for k in expected} == expected
    if not mlp:         # what the U-Net's plan newly says: the whole batch at once, nothing to keep "whole"
        assert (plan['Bc'], plan['whole']) == (len(steps_pp), False)


def test_the_unet_plan_has_the_keys_of_the_mlp_plan():
    for steps_pp in ([1, 1, 1, 1], [2, 1, 4, 1]):
        mlp = _plan(True, {'mlp_stash_gb': 0.03, 'mlp_whole_batch_gb': 0.0}, steps_pp, True)
        assert set(_plan(False, {'n_down': 3}, steps_pp, True)) == set(mlp)
        assert set(mlp) == {'perm', 'groups', 'chunks', 'whole_bytes', 'chunk_bytes', 'Bc', 'whole', 'reserve'}


def _batch(ts1, ts2, step, **more):
    b = {'time_stamp_1': torch.tensor(ts1).reshape(-1, 1, 1, 1), 'time_stamp_2': torch.tensor(ts2).reshape(-1, 1, 1, 1),
         'time_step': step}
    b.update(more)
    return b


def test_steps_per_pair():
    """Values and messages recorded from the former Model._steps_per_pair / Model._integer_steps on the same CPU tensors."""
    from dvd_hip.models.sf_step import integer_steps, steps_per_pair
    # uniform (a tensor time step: float32's 0.1), mixed, and with the frame ids of either naming in the same read
    assert steps_per_pair(_batch([0., .1, .2], [.1, .2, .3], torch.tensor([[0.1]]))) == (1, [1, 1, 1], 0.10000000149011612, None)
    assert steps_per_pair(_batch([0., .1, .2, .3], [.2, .2, .6, .4], 0.1)) == (4, [2, 1, 4, 1], 0.1, None)
    assert steps_per_pair(_batch([0., .1], [.2, .3], 0.1, fid_1=torch.tensor([0, 1]), fid_2=torch.tensor([2, 3])),
                          with_ids=True) == (2, [2, 2], 0.1, ([0, 1], [2, 3]))
    assert steps_per_pair(_batch([0., .1], [.2, .3], 0.1, frame_id_1=torch.tensor([[5.], [1.]]),
                                 frame_id_2=torch.tensor([[7.], [3.]])), with_ids=True) == (2, [2, 2], 0.1, ([5, 1], [7, 3]))
    assert integer_steps(_batch([0., .1], [.2, .3], torch.tensor(0.1))) == (2, 0.10000000149011612)
    # non-finite time stamps: the uniform path, with whatever integer_steps makes of them
    for bad in (float('nan'), float('inf')):
        b = _batch([0., .1], [bad, .3], 0.1)
        n = integer_steps(b)[0]
        assert steps_per_pair(b) == (n, [n, n], 0.1, None)       # (n: a float-to-integer cast of NaN, -2^63 where recorded)
    # a mixed batch with a pair of less than one step
    with pytest.raises(ValueError) as e:
        steps_per_pair(_batch([0., .1, .2], [.2, .1, .3], 0.1))
    assert str(e.value) == ('pair 1 of a batch that mixes frame gaps has time stamps 0 frames apart (0 Euler steps): '
                            'every pair needs at least one')
    with pytest.raises(ValueError) as e:
        steps_per_pair(_batch([0., .3], [.2, .1], 0.1))
    assert str(e.value) == ('pair 1 of a batch that mixes frame gaps has time stamps -2 frames apart (-2 Euler steps): '
                            'every pair needs at least one')


@pytest.mark.parametrize('ids,message', [
    ({'fid_1': torch.tensor([0.5, 1]), 'fid_2': torch.tensor([2., 3])},
     'opt.share_frames: frame ids must be whole numbers in [0, 2^24), got [0.5, 1.0, 2.0, 3.0]'),
    ({'fid_1': torch.tensor([-1, 1]), 'fid_2': torch.tensor([2, 3])},
     'opt.share_frames: frame ids must be whole numbers in [0, 2^24), got [-1.0, 1.0, 2.0, 3.0]'),
    ({'fid_1': torch.tensor([2 ** 24, 1]), 'fid_2': torch.tensor([2, 3])},
     'opt.share_frames: frame ids must be whole numbers in [0, 2^24), got [16777216.0, 1.0, 2.0, 3.0]'),
    ({'fid_1': torch.tensor([0, 1, 2]), 'fid_2': torch.tensor([2, 3])}, 'opt.share_frames: fid_1 / fid_2 hold 3 / 2 ids for 2 pairs'),
    ({'fid_1': torch.tensor([0, 1])},
     'opt.share_frames needs the frame id of every image: the batch has neither fid_1 / fid_2 nor frame_id_1 / frame_id_2 '
     "(its keys: ['fid_1', 'time_stamp_1', 'time_stamp_2', 'time_step'])"),
    ({}, 'opt.share_frames needs the frame id of every image: the batch has neither fid_1 / fid_2 nor frame_id_1 / frame_id_2 '
         "(its keys: ['time_stamp_1', 'time_stamp_2', 'time_step'])"),
])
def test_share_frames_ids_are_validated(ids, message):
    from dvd_hip.models.sf_step import steps_per_pair
    with pytest.raises(ValueError) as e:
        steps_per_pair(_batch([0., .1], [.2, .3], 0.1, **ids), with_ids=True)
    assert str(e.value) == message
    assert steps_per_pair(_batch([0., .1], [.2, .3], 0.1, **ids)) == (2, [2, 2], 0.1, None)      # not read without share_frames


def test_image_sets():
    from dvd_hip.models.sf_step import image_sets
    a, fa, b, fb, u, fu = 'img_1', 'fid_1', 'img_2', 'fid_2', 'img_u', 'fid_u'
    for n_slots in (1, 3):
        assert image_sets(a, fa, b, fb, n_slots) == ([(a, fa, 0), (b, fb, n_slots)], 2 * n_slots)
        assert image_sets(a, None, b, None, n_slots) == ([(a, None, 0), (b, None, n_slots)], 2 * n_slots)      # MiDaS: no ids
        assert image_sets(a, fa, b, fb, n_slots, union=(u, fu)) == ([(u, fu, 0)], n_slots)
        assert image_sets(a, None, b, None, n_slots, union=(u, None)) == ([(u, None, 0)], n_slots)


def test_the_model_module_still_exports_the_planner():
    from dvd_hip.models import scene_flow_motion_field as m, sf_step
    assert m.gap_plan is sf_step.gap_plan and m.pairs_per_chunk is sf_step.pairs_per_chunk
