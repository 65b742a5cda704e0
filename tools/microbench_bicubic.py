"""Bicubic resize kernels (csrc/bicubic.hip) against ATen's F.interpolate(mode='bicubic', align_corners=True) at the sizes of a
MiDaS step with a working resolution: 96 x 1 x 224 x 384 <-> 384 x 672 (the depth maps of 48 pairs back to the frame size, and
the same planes down to the working size).  Forward and backward times, GB/s of the algorithmic bytes (input + output planes,
fp32); written to profiles/bicubic_microbench.json."""
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'dynamic-video-depth_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from dvd_hip import build, ops  # noqa: E402
from tools_timeit import timeit  # noqa: E402


def aten(x, size):
    return F.interpolate(x, size=size, mode='bicubic', align_corners=True)


rows = []
for (N, C, H, W, Ho, Wo) in ((96, 1, 224, 384, 384, 672), (96, 1, 384, 672, 224, 384)):
    x = torch.randn(N, C, H, W, device='cuda', requires_grad=True)
    gy = torch.randn(N, C, Ho, Wo, device='cuda')
    gb = N * C * (H * W + Ho * Wo) * 4 / 1e9
    row = {'planes': [N, C], 'in': [H, W], 'out': [Ho, Wo], 'algorithmic_GB': gb}
    for name, fn in (('hip', ops.bicubic_resize), ('aten', aten)):
        fwd = timeit(lambda: fn(x, (Ho, Wo)), 10)
        tot = timeit(lambda: torch.autograd.grad(fn(x, (Ho, Wo)), x, gy), 10)
        row[name] = {'fwd_ms': fwd, 'fwd_GBps': gb / fwd * 1e3, 'bwd_ms': tot - fwd, 'bwd_GBps': gb / (tot - fwd) * 1e3}
    rows.append(row)
    print(json.dumps(row))
out = {'device': torch.cuda.get_device_name(0), 'source_digest': build.source_digest(('bicubic.hip',)), 'cases': rows}
with open(os.path.join(ROOT, 'profiles', 'bicubic_microbench.json'), 'w') as f:
    json.dump(out, f, indent=1)
