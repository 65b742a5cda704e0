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


def triangulate_plan(pairs, n_frames, frames=None, gaps=None):
    """The observation table of ops.triangulate from `Catalogue.pairs` (host only) -> (frames int32 [B], obs int32 [B,M,3]).
    Per query frame, every stored pair (f_1, f_2) that contains it -- restricted to |f_2 - f_1| in `gaps` if given -- as a row
    (pair index, the other frame, dir): dir 0 where the frame is the pair's first (flow_1_2 leaves it), 1 where it is the second
    (flow_2_1).  Rows are ordered by |gap| ascending, forward before backward, then by pair index, and padded with -1 to the
    longest row (M = 0 if no frame has a pair).  frames=None: all of them."""
    import numpy as np
    from . import ops
    n_frames = int(n_frames)
    if frames is None:
        frames = range(n_frames)
    frames = [int(f) for f in frames]
    if not frames or min(frames) < 0 or max(frames) >= n_frames:
        raise ValueError('triangulate_plan: frames must name at least one of the %d frames, got %r' % (n_frames, frames))
    keep = None if gaps is None else set(abs(int(g)) for g in gaps)
    if keep is not None and (not keep or min(keep) < 1):
        raise ValueError('triangulate_plan: gaps must be non-zero frame distances, got %r' % (gaps,))
    per = {f: [] for f in set(frames)}
    for j, (a, b) in enumerate(pairs):
        a, b = int(a), int(b)
        if a == b or not (0 <= a < n_frames and 0 <= b < n_frames):
            raise ValueError('triangulate_plan: pair %d is (%d, %d) in a video of %d frames' % (j, a, b, n_frames))
        if keep is not None and abs(b - a) not in keep:
            continue
        if a in per:
            per[a].append((abs(b - a), 0, j, b))
        if b in per:
            per[b].append((abs(b - a), 1, j, a))
    M = max(len(v) for v in per.values())
    if M > ops.TRI_MAX_OBS:
        f = max(per, key=lambda k: len(per[k]))
        raise ValueError('triangulate_plan: frame %d has %d observations, at most %d (restrict `gaps`)' % (f, M, ops.TRI_MAX_OBS))
    obs = np.full((len(frames), M, 3), -1, dtype=np.int32)
    for i, f in enumerate(frames):
        for m, (_, d, j, other) in enumerate(sorted(per[f])):
            obs[i, m] = (j, other, d)
    return np.array(frames, dtype=np.int32), obs


def triangulate_depth(store, frames=None, gaps=None, mode='median', epi_tol=1.0, min_parallax_deg=0.5, z_near=1e-3, min_count=2,
                      tables=None, chunk=None, densify=False):
    """A depth map that does not depend on the network, a confidence for it and a motion cue, from a FrameStore's flows,
    occlusion masks and cameras (ops.triangulate, csrc/triangulate.hip; the table of triangulate_plan over store.cat.pairs).
    -> dict on the device, for the B requested frames (None: all):
      depth [B,1,H,W]   the consistent observations' triangulated depth fused by `mode`; 0 where fewer than min_count agree
      count, usable     uint8 [B,H,W]: consistent observations, and those with a valid flow and enough parallax
      epi [B,1,H,W]     mean epipolar distance of the usable observations in pixels (-1 without one)
      spread [B,1,H,W]  (max - min) of the consistent depths over the fused one
      static, moving    bool [B,H,W]: count >= min_count;  usable >= min_count and no consistent observation
      frames            the frame ids, int32 on the host
    min_parallax_deg: an observation whose rays meet under a smaller angle is not used.  tables: cameras other than the store's
    (e.g. at another scale).  chunk: frames per launch (None: one launch); it does not change a bit.
    densify=True adds depth_dense [B,1,H,W], `depth` with everything that is not `static` filled from the static pixels by
    push-pull interpolation (ops.fill_holes with equal weights; 0 for a frame without a static pixel), and dense_level uint8
    [B,H,W], the pyramid level of the nearest static pixel (0 on them, 255 for such a frame).  Nothing else changes."""
    import math
    import numpy as np
    from . import ops
    if isinstance(min_parallax_deg, bool) or not isinstance(min_parallax_deg, (int, float)) or not 0 < min_parallax_deg <= 90:
        raise ValueError('triangulate_depth: min_parallax_deg must be in (0, 90], got %r' % (min_parallax_deg,))
    if chunk is not None and (isinstance(chunk, bool) or int(chunk) != chunk or chunk < 1):
        raise ValueError('triangulate_depth: chunk must be a positive number of frames, got %r' % (chunk,))
    if not isinstance(densify, (bool, np.bool_)):
        raise ValueError('triangulate_depth: densify must be True or False, got %r' % (densify,))
    fr, obs = triangulate_plan(store.cat.pairs, store.cat.n_frames, frames, gaps)
    B, H, W, dev = len(fr), store.H, store.W, store.device
    chunk = min(B, 65535) if chunk is None else min(int(chunk), 65535)
    sin2_min = float(np.float32(math.sin(math.radians(min_parallax_deg)) ** 2))
    tables = store.tables if tables is None else tables
    res = {k: torch.empty((B, 1, H, W) if chan else (B, H, W), device=dev, dtype=dtype) for k, dtype, chan in ops.TRI_OUT}
    for b0 in range(0, B, chunk):
        b1 = min(b0 + chunk, B)
        ops.triangulate(store.flow_1_2, store.flow_2_1, store.mask_1, store.mask_2, obs[b0:b1], fr[b0:b1], tables, mode=mode,
                        epi_tol=epi_tol, sin2_min=sin2_min, z_near=z_near, min_count=min_count,
                        out={k: v[b0:b1] for k, v in res.items()})
    res['frames'] = fr
    res['static'] = res['count'] >= min_count
    res['moving'] = (res['usable'] >= min_count) & (res['count'] == 0)
    if densify:
        filled = ops.fill_holes(res['depth'], res['static'].to(torch.uint8), power=0, fill=0.0)
        res['depth_dense'], res['dense_level'] = filled['values'], filled['level']
    return res


def chain_plan(pairs, n_frames, gaps, base=None):
    """The chain tables of ops.flow_chain that reach the frame gaps `gaps` from the stored `pairs` (host only)
    -> (new_pairs, links_fwd, links_bwd).  For every requested gap g, and every a with a + g < n_frames whose pair (a, a + g) is
    not stored already, two chains:
      forward   a -> a + g, greedy: at frame f the largest stored gap s <= the frames that remain for which (f, f + s) is
                stored, as the row (its pair index, 0)
      backward  a + g -> a: the same pairs from the far end, as rows (pair index, 1)
    new_pairs lists the (a, a + g), gaps ascending, a ascending; links_fwd and links_bwd are int32 [P', L, 2], L the longest
    chain, padded with -1.  base: the stored gaps a chain may use (base=[1] chains gap-1 flows only; None: all of them).  A
    ValueError names the first pair that the greedy walk cannot reach (it does not back up: gap 7 from base=[2, 3] is stuck after
    3 + 3 although 3 + 2 + 2 exists), or that would need more than ops.CHAIN_MAX_LINKS links."""
    import numpy as np
    from . import ops
    n_frames = int(n_frames)
    try:
        want = sorted(set(int(g) for g in gaps))
        ok = all(int(g) == g and not isinstance(g, bool) for g in gaps)
    except (TypeError, ValueError):
        want, ok = [], False
    if not ok or not want or want[0] < 1:
        raise ValueError('chain_plan: gaps must be positive frame distances, got %r' % (gaps,))
    allow = None if base is None else set(int(g) for g in base)
    if allow is not None and (not allow or min(allow) < 1):
        raise ValueError('chain_plan: base must be positive frame distances, got %r' % (base,))
    at, stored = {}, set()
    for j, (a, b) in enumerate(pairs):
        a, b = int(a), int(b)
        if not 0 <= a < b < n_frames:
            raise ValueError('chain_plan: pair %d is (%d, %d); stored pairs run forwards in a video of %d frames' % (j, a, b, n_frames))
        at.setdefault((a, b), j)
        if allow is None or b - a in allow:
            stored.add(b - a)
    steps = sorted(stored, reverse=True)
    new_pairs, chains = [], []
    for g in want:
        for a in range(n_frames - g):
            if (a, a + g) in at:
                continue
            f, chain = a, []
            while f < a + g:
                s = next((s for s in steps if s <= a + g - f and (f, f + s) in at), None)
                if s is None:
                    raise ValueError('chain_plan: the pair (%d, %d) cannot be reached by the greedy walk (the largest stored gap%s that fits, '
                                     'at every frame): it is stuck at frame %d, %d frame(s) short, with no stored flow that fits' % (
                                         a, a + g, '' if allow is None else ' among %s' % sorted(allow), f, a + g - f))
                chain.append(at[(f, f + s)])
                f += s
                if len(chain) > ops.CHAIN_MAX_LINKS:
                    raise ValueError('chain_plan: the pair (%d, %d) needs more than %d links' % (a, a + g, ops.CHAIN_MAX_LINKS))
            new_pairs.append((a, a + g))
            chains.append(chain)
    L = max([len(c) for c in chains] + [1])
    fwd = np.full((len(chains), L, 2), -1, dtype=np.int32)
    bwd = np.full((len(chains), L, 2), -1, dtype=np.int32)
    for i, c in enumerate(chains):
        fwd[i, :len(c), 0], fwd[i, :len(c), 1] = c, 0
        bwd[i, :len(c), 0], bwd[i, :len(c), 1] = c[::-1], 1
    return new_pairs, fwd, bwd


CHAIN_SCRATCH_BYTES = 1 << 28       # chain_flows' default chunk keeps the rows of a launch below this


def chain_flows(store, gaps, base=None, chunk=None):
    """The flow pairs of the frame gaps `gaps` that a FrameStore lacks, chained on the device from the pairs it holds
    (chain_plan over store.cat.pairs, ops.flow_chain) -> dict on the device, ready for FrameStore.add_pairs:
      pairs                the new (f_1, f_2), gaps ascending, f_1 ascending (a host list)
      flow_1_2, flow_2_1   [P',H,W,2]: the forward chain f_1 -> f_2 and the backward chain f_2 -> f_1 after their last link
      broken_1, broken_2   uint8 [P',H,W]: 0, or 1 + the link at which the backward / the forward chain broke (the sides are the
                           masks': mask_2 belongs to flow_1_2, mask_1 to flow_2_1)
      mask_1, mask_2       uint8 [P',H,W], 1 = not to be used: the reference's forward / backward consistency rule on the composed
                           pair (flow_consistency_masks), or the chain broke
      n_links              int32 [P']: links per chain
    base: the stored gaps to chain from (None: all; [1]: gap-1 flows only).  chunk: chains per launch (None: as many as keep a
    launch's rows within CHAIN_SCRATCH_BYTES); it does not change a bit."""
    import numpy as np
    from . import ops
    if chunk is not None and (isinstance(chunk, bool) or int(chunk) != chunk or chunk < 1):
        raise ValueError('chain_flows: chunk must be a positive number of chains, got %r' % (chunk,))
    pairs, fwd, bwd = chain_plan(store.cat.pairs, store.cat.n_frames, gaps, base)
    if not pairs:
        raise ValueError('chain_flows: the store holds every pair of the gaps %r already' % (gaps,))
    n, L = fwd.shape[:2]
    H, W, dev = store.H, store.W, store.device
    if chunk is None:
        chunk = max(1, CHAIN_SCRATCH_BYTES // (L * H * W * 9))
    chunk = min(int(chunk), n, 65535)
    n_links = (fwd[..., 0] >= 0).sum(1).astype(np.int64)
    # the row of each chain's last link, and the chain's place in its launch: one pinned upload for all launches
    pick = torch.from_numpy(np.stack([n_links - 1, np.arange(n) % chunk])).pin_memory().to(dev, non_blocking=True)
    res = {'pairs': pairs, 'n_links': pick[0].to(torch.int32) + 1}
    scratch = {'flow': torch.empty(L, chunk, H, W, 2, device=dev), 'broken': torch.empty(L, chunk, H, W, device=dev, dtype=torch.uint8)}
    for links, flow_key, broken_key in ((fwd, 'flow_1_2', 'broken_2'), (bwd, 'flow_2_1', 'broken_1')):
        res[flow_key] = torch.empty(n, H, W, 2, device=dev)
        res[broken_key] = torch.empty(n, H, W, device=dev, dtype=torch.uint8)
        for b0 in range(0, n, chunk):
            b1 = min(b0 + chunk, n)
            b = b1 - b0       # (a short last launch: the flow rows keep the scratch's stride, `broken` is the front of its memory)
            out = ops.flow_chain(store.flow_1_2, store.flow_2_1, store.mask_1, store.mask_2, links[b0:b1],
                                 out={'flow': scratch['flow'][:, :b], 'broken': scratch['broken'].view(-1)[:L * b * H * W].view(L, b, H, W)})
            last, col = pick[0, b0:b1], pick[1, b0:b1]
            res[flow_key][b0:b1] = out['flow'][last, col]
            res[broken_key][b0:b1] = out['broken'][last, col]
    m1, m2 = flow_consistency_masks(res['flow_1_2'], res['flow_2_1'])
    res['mask_1'] = m1 | (res['broken_1'] != 0).to(torch.uint8)
    res['mask_2'] = m2 | (res['broken_2'] != 0).to(torch.uint8)
    return res


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
