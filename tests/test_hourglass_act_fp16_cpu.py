"""CPU checks of the hourglass fp16-activation mode: the new C entry points are declared, exported and bound, and the hourglass
module on CPU tensors ignores `act_dtype` (the oracle / fixture generator path keeps the reference's ATen ops)."""
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('dvd_xwgradk_h', 'dvd_head3x3_fwd', 'dvd_head3x3_bwd_workspace_bytes', 'dvd_head3x3_bwd', 'dvd_add_f16')


def test_new_entry_points_are_declared_exported_and_bound():
    from dvd_hip import _lib
    header = open(os.path.join(ROOT, 'include', 'dvd_hip.h')).read()
    assert int(re.search(r'#define DVD_ABI_VERSION (\d+)', header).group(1)) == _lib.ABI_VERSION == 8
    lib = _lib.load()
    assert lib.dvd_abi_version() == 8
    for name in NEW:
        assert re.search(r'\b%s\(' % name, header), name + ' is not declared'
        assert name in _lib.SIGNATURES, name + ' is not bound'
        assert getattr(lib, name) is not None
    assert lib.dvd_head3x3_bwd_workspace_bytes(2, 64, 32, 48) > 0
    assert lib.dvd_head3x3_bwd_workspace_bytes(0, 64, 32, 48) == 0


def test_entry_points_reject_bad_arguments_without_a_device():
    from dvd_hip import _lib
    lib = _lib.load()
    assert lib.dvd_add_f16(None, None, None, 16, None, None) == _lib.DVD_EINVAL
    assert lib.dvd_head3x3_fwd(None, None, None, None, None, 1, 64, 8, 8, None) == _lib.DVD_EINVAL
    assert lib.dvd_xwgradk_h(None, None, None, None, None, 0, 1, 32, 16, 8, 8, 7, 0, None) == _lib.DVD_EINVAL


def test_hourglass_on_cpu_ignores_act_dtype():
    from dvd_hip.third_party.hourglass import HourglassModel_Embed
    torch.manual_seed(0)
    net = HourglassModel_Embed()
    net.eval()
    x = torch.rand(1, 3, 16, 16)
    with torch.no_grad():
        d32 = net(x)
        net.act_dtype = torch.float16
        assert net.net_depth.act_dtype == torch.float16
        d16 = net(x)
    assert d16.dtype == torch.float32 and torch.equal(d32, d16)
