"""opt.midas_resize without a GPU: validation at construction, precedence over the dataset-name rule, the memory planner's
pixel count, and the CPU branch of MidasNet(resize=...), which stays on ATen (the oracle side relies on it)."""
import warnings
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import helpers


def _opt(**over):
    o = dict(helpers.FULL_STEP_OPT)
    o.update(midas=True, full_logdir='/tmp')
    o.update(over)
    return SimpleNamespace(**o)


@pytest.mark.parametrize('size,match', [((60, 96), 'multiples of 32'), ((64, 100), 'multiples of 32'), ((0, 96), 'positive'),
                                        ((-32, 96), 'positive'), ((64,), 'pair'), (64, 'pair'), ((64.5, 96), 'pair')])
def test_invalid_sizes_are_refused_at_construction(size, match):
    from dvd_hip.models.scene_flow_motion_field import Model, midas_resize_of
    with pytest.raises(ValueError, match=match):
        midas_resize_of(_opt(midas_resize=size))
    with pytest.raises(ValueError, match=match):
        Model(_opt(midas_resize=size), None)          # refused before any network is built


def test_the_switch_needs_midas():
    from dvd_hip.models.scene_flow_motion_field import Model
    with pytest.raises(ValueError, match='needs --midas'):
        Model(_opt(midas=False, midas_resize=(64, 96)), None)


def test_default_and_validated_value():
    from dvd_hip.models.scene_flow_motion_field import midas_resize_of
    assert midas_resize_of(_opt()) is None
    assert midas_resize_of(SimpleNamespace(midas=False)) is None
    assert midas_resize_of(_opt(midas_resize=[64, 96])) == (64, 96)


def test_precedence_over_the_dataset_name_rule(monkeypatch):
    """The rule stays (any dataset whose name contains real_video / korean / mctest / cube works at [224, 384]); an explicit
    value wins; neither: the frame size.  (The encoder is stubbed: building ResNeXt-101 four times would take a minute.)"""
    from dvd_hip.models import scene_flow_motion_field as M
    seen = []

    class Stub(torch.nn.Module):
        def __init__(self, path=None, non_negative=True, normalize_input=False, resize=None):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))
            self.resize = resize
            seen.append(resize)
    monkeypatch.setattr(M, 'MidasNet', Stub)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        M.Model(_opt(), None)
        M.Model(_opt(dataset='cube_synthetic'), None)
        M.Model(_opt(dataset='cube_synthetic', midas_resize=(64, 96)), None)
        M.Model(_opt(midas_resize=(96, 160)), None)
        for name in ('my_real_video', 'korean_x', 'mctest'):
            M.Model(_opt(dataset=name), None)
    assert seen == [None, [224, 384], [64, 96], [96, 160], [224, 384], [224, 384], [224, 384]]
    # not a command-line flag: the flag set is the reference's (tests/test_model_surface_cpu.py pins it)
    import argparse
    parser, _ = M.Model.add_arguments(argparse.ArgumentParser())
    assert 'midas_resize' not in {a.dest for a in parser._actions}


def test_planner_counts_the_pixels_the_net_works_on(monkeypatch):
    from dvd_hip.models import depth_runner as D
    monkeypatch.delenv('DVD_HEAD_ROOM_GB', raising=False)
    monkeypatch.delenv('DVD_KEEP_DEBUG', raising=False)
    assert D.working_size(SimpleNamespace()) is None
    assert D.working_size(SimpleNamespace(midas_resize=(64, 96))) == (64, 96)
    assert D.working_size(SimpleNamespace(), SimpleNamespace(resize=[224, 384])) == (224, 384)      # the dataset-name rule
    assert D.working_size(SimpleNamespace(midas_resize=(64, 96)), SimpleNamespace(resize=[224, 384])) == (64, 96)
    assert D.working_pixels(4, 270, 480) == 4 * 270 * 480 and D.resize_extra_bytes(4, 270, 480) == 0
    assert D.working_pixels(4, 270, 480, (224, 384)) == 4 * 224 * 384
    assert D.resize_extra_bytes(4, 270, 480, (224, 384)) == 4 * 2 * 4 * 270 * 480      # two fp32 frame-size planes per image

    G = 2 ** 30

    def runner(**over):
        r = D.DepthRunner(SimpleNamespace(depth_keep_gb=150.0, midas=True, depth_graphs=1, depth_chunk=2, use_embedding=False,
                                          **over), None, None, act_fp16=False)

        def capture(chunk, fid):
            return D._Slot(None, None, None, None, None, 10 * G)
        r._capture_slot = capture
        return r
    chunk = torch.zeros(2, 3, 540, 960)
    # the estimate of a first slot, read back from the fit test: free memory one byte short of / exactly at what it needs
    for over, px, extra in ((dict(), 2 * 540 * 960, 0), (dict(midas_resize=(224, 384)), 2 * 224 * 384, 2 * 2 * 4 * 540 * 960)):
        est = int(px * 4900.0 + extra + 1.5 * G)
        need = est + 0.08 * 288 * G + est // 2
        r = runner(**over)
        r.free_hbm = lambda dev: (need - 4096, 288 * G)
        assert r._keep_slot(0, chunk, None, 0, 4) is None
        r = runner(**over)
        r.free_hbm = lambda dev: (need + 4096, 288 * G)
        assert r._keep_slot(0, chunk, None, 0, 4) is not None
        assert r.keep_per_px == (10 * G - extra) / float(px)                # measured per working pixel
    # pick_chunk: 48 pairs of 1080 x 1920 frames do not fit as 48-image slots at the frame size, and do at 224 x 384
    for over, want in ((dict(), 16), (dict(midas_resize=(224, 384)), 48)):
        r = runner(**over)
        r.free_hbm = lambda dev: (280 * G, 288 * G)
        assert r.pick_chunk(48, 1080 * 1920, 20 * G, None) == want


def test_cpu_branch_is_still_aten():
    """MidasNet(resize=...) on CPU tensors: normalise, F.interpolate, the net at the working size, F.interpolate back -- equal
    to composing those by hand around the same module without a resize."""
    from dvd_hip.third_party.MiDaS import MidasNet
    torch.manual_seed(0)
    net = helpers.seeded_fill_(MidasNet(non_negative=True, normalize_input=True, resize=[32, 64]), 3).eval()
    with torch.no_grad():
        net.scratch.output_conv[4].weight.mul_(30.0)
        net.scratch.output_conv[4].bias.fill_(2000.0)
    x = torch.rand(1, 3, 24, 40)
    with torch.no_grad():
        got = net(x)
        net.resize, net.normalize_input = None, False
        xn = ((x.permute([0, 2, 3, 1]) - net.mean) / net.std).permute([0, 3, 1, 2]).contiguous()
        inner = net(F.interpolate(xn, size=[32, 64], mode='bicubic', align_corners=True))
        want = F.interpolate(inner, size=(24, 40), mode='bicubic', align_corners=True)
    assert got.shape == (1, 1, 24, 40) and torch.equal(got, want)
