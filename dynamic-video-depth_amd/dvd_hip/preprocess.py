"""Mask preprocessing of a frame pair on the GPU.

Counterpart of /root/reference/scripts/preprocess/davis/generate_flows.py:57-82,139-148 (forward/backward
flow-consistency + out-of-bounds masks, computed there per pair in numpy after RAFT) and of the mask
conversion in scripts/preprocess/davis/generate_sequence_midas.py:144-147.  RAFT itself stays external: this
module starts from the two flow fields.

And the scale calibration of scripts/preprocess/shutterstock/generate_frame_midas.py:153-160, 180-183: the per-frame
median of network depth over MVS depth (exact, csrc/select.hip), their mean, and the camera poses at that scale.  The
resizing of frames (skimage) is not part of this module.
"""
import torch

from . import _lib
from .ops import _dev32, _p, _stream


def flow_consistency_masks(flow_1_2, flow_2_1):
    """flows [B,H,W,2] (or [H,W,2]) -> (mask_1, mask_2) uint8 [B,H,W], 1 = occluded or leaving the image:
    the arrays generate_flows.py stores as `mask_1` / `mask_2` (:139-153)."""
    single = flow_1_2.dim() == 3
    if single:
        flow_1_2, flow_2_1 = flow_1_2[None], flow_2_1[None]
    f12, f21 = _dev32(flow_1_2, 'flow_1_2'), _dev32(flow_2_1, 'flow_2_1')
    B, H, W, _ = f12.shape
    lib = _lib.load()
    out = []
    for a, b in ((f12, f21), (f21, f12)):         # mask_1 samples flow_1_2 along flow_2_1, mask_2 the reverse
        m = torch.empty(B, H, W, device=f12.device, dtype=torch.float32)
        _lib.check(lib.dvd_flow_consistency_mask(_p(a), _p(b), _p(m), B, H, W, _stream()), 'dvd_flow_consistency_mask')
        out.append(m.to(torch.uint8))
    return (out[0][0], out[1][0]) if single else (out[0], out[1])


def calibrate_scale(depth_nn, depth_mvs, thresh=1e-3):
    """The scale that brings the camera translations to the depth network's scale
    (scripts/preprocess/shutterstock/generate_frame_midas.py:153-160): per frame
    `np.median(nn_depth[idx, idy] / mvs_depth[idx, idy])` over `np.where(mvs_depth > 1e-3)`, then `s = np.mean(scales)`.
    depth_nn, depth_mvs: [N,H,W] (or [N,1,H,W]) fp32 on the GPU -> (scales [N] fp32 on the device, s).  The medians are exact
    (ops.ratio_median, csrc/select.hip); s is numpy's fp32 mean of the N medians on the host, the reference's statement."""
    import numpy as np
    from . import ops
    nn, mvs = _dev32(depth_nn, 'depth_nn'), _dev32(depth_mvs, 'depth_mvs')
    if nn.shape != mvs.shape or nn.dim() < 2:
        raise RuntimeError('calibrate_scale: depth_nn and depth_mvs must share a shape [N,H,W], got %s and %s' % (
            tuple(nn.shape), tuple(mvs.shape)))
    N = nn.shape[0]
    scales = ops.ratio_median(nn.reshape(N, -1), mvs.reshape(N, -1), den_min=thresh)['median']
    return scales, np.mean(scales.cpu().numpy())


def scale_poses(w2c, s):
    """World-to-camera matrices [N,4,4] -> camera-to-world fp32 [N,4,4] at the calibrated scale, the reference's three
    statements per frame (generate_frame_midas.py:180-183): `T[:3, 3] *= s`, `np.linalg.inv(T)`, `.astype(np.float32)`.  Host
    arithmetic in the dtype the poses come in; not a hot path."""
    import numpy as np
    w2c = np.array(w2c.cpu().numpy() if torch.is_tensor(w2c) else w2c)
    if w2c.ndim != 3 or w2c.shape[1:] != (4, 4):
        raise RuntimeError('scale_poses: w2c must be [N,4,4], got %s' % (w2c.shape,))
    out = np.empty(w2c.shape, dtype=np.float32)
    for i in range(w2c.shape[0]):
        T = np.array(w2c[i])
        T[:3, 3] *= s
        out[i] = np.linalg.inv(T).astype(np.float32)
    return out


def training_masks(mask_1, mask_2):
    """The `mask_1` / `mask_2` tensors of a training batch: 1 = valid, [B,H,W,1,1] float
    (generate_sequence_midas.py:144-147: 1 - ceil(mask))."""
    return tuple((1 - torch.ceil(m.float()))[..., None, None] for m in (mask_1, mask_2))
