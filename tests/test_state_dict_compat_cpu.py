"""Checkpoint interchange: the depth networks and the scene-flow MLP expose the reference's state_dict keys (in order)
and shapes.  The reference's side is data: tests/golden/interfaces.json, written by tests/golden/make_golden.py (case
`interfaces`) from the reference's own modules -- MidasNet with the encoder torch.hub would return (oracle/resnext.py's
independent restatement of torchvision's ResNeXt-101 32x8d, assembled by the reference's own `_make_resnet_backbone`),
HourglassModel_Embed and SceneFlowFieldNet."""
import helpers


def _same(a, want):
    assert list(a) == [k for k, _ in want]
    for k, shape in want:
        assert list(a[k].shape) == shape, k


def test_state_dict_keys_and_shapes_match_the_reference():
    from dvd_hip.networks.sceneflow_field import SceneFlowFieldNet
    from dvd_hip.third_party.hourglass import HourglassModel_Embed
    from dvd_hip.third_party.MiDaS import MidasNet
    ref = helpers.load_golden_json('interfaces')['state_dicts']
    _same(MidasNet().state_dict(), ref['midas'])
    _same(HourglassModel_Embed(noexp=False, use_embedding=False).state_dict(), ref['hourglass_embed'])
    kw = dict(net_width=256, n_layers=4, time_dependent=True, N_freq_xyz=16, N_freq_t=16)
    _same(SceneFlowFieldNet(**kw).state_dict(), ref['sceneflow_mlp'])
