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


def refine_plan(pairs, n_frames, gaps=None):
    """The observation rows of ops.pose_normal_eq from `Catalogue.pairs` (host only) -> int32 [R,4], rows (pair, a, b, dir):
    every stored pair (f_1, f_2) -- restricted to |f_2 - f_1| in `gaps` if given -- in stored order, as (pair, f_1, f_2, 0)
    (flow_1_2 leaves f_1) and then (pair, f_2, f_1, 1) (flow_2_1 leaves f_2).  A ValueError if that selects no row."""
    import numpy as np
    if isinstance(n_frames, bool) or int(n_frames) != n_frames or n_frames < 1:
        raise ValueError('refine_plan: n_frames must be a positive number of frames, got %r' % (n_frames,))
    n_frames = int(n_frames)
    keep = None
    if gaps is not None:
        try:
            keep = set(abs(int(g)) for g in gaps)
            ok = all(int(g) == g and not isinstance(g, bool) for g in gaps)
        except (TypeError, ValueError):
            keep, ok = set(), False
        if not ok or not keep or min(keep) < 1:
            raise ValueError('refine_plan: gaps must be non-zero frame distances, got %r' % (gaps,))
    rows = []
    for j, (a, b) in enumerate(pairs):
        a, b = int(a), int(b)
        if a == b or not (0 <= a < n_frames and 0 <= b < n_frames):
            raise ValueError('refine_plan: pair %d is (%d, %d) in a video of %d frames' % (j, a, b, n_frames))
        if keep is None or abs(b - a) in keep:
            rows += [(j, a, b, 0), (j, b, a, 1)]
    if not rows:
        raise ValueError('refine_plan: no row: none of the %d stored pairs has a gap in %r' % (len(pairs), gaps))
    return np.array(rows, dtype=np.int32)


def _exp_so3(w):
    """Rodrigues' formula in float64."""
    import numpy as np
    th = float(np.sqrt(w @ w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * (K @ K)
    return np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / (th * th)) * (K @ K)


POSE_STALL = 5      # refine_cameras: rejected steps in a row, after an accepted one, that end the loop as converged
POSE_TRI = [(i, j) for i in range(13) for j in range(i, 13)]        # the order of the 91 entries of J^T w J in a row's sums


def _pose_system(sums, rows, N):
    """The rows' 13 x 13 blocks over [tau_a, omega_a, sigma_a, tau_b, omega_b] -> (H [7N,7N], g [7N], cost) in float64."""
    import numpy as np
    Hm, g = np.zeros((7 * N, 7 * N)), np.zeros(7 * N)
    ti, tj = (np.array(v) for v in zip(*POSE_TRI))
    for s, (_, a, b, _) in zip(sums, rows.tolist()):
        idx = np.r_[7 * a:7 * a + 7, 7 * b:7 * b + 6]
        blk = np.zeros((13, 13))
        blk[ti, tj] = s[:91]
        blk[tj, ti] = s[:91]
        Hm[np.ix_(idx, idx)] += blk
        g[idx] += s[91:104]
    return Hm, g, float(np.sum(sums[:, 104]))


def refine_cameras(store, depth=None, weight=None, gaps=None, anchor=0, scales=False, huber=1.0, z_near=1e-3, max_iter=30,
                   rel_tol=1e-9, tables=None):
    """Camera poses -- and with scales=True one depth scale per frame -- refined against a FrameStore's flows, by
    Levenberg-Marquardt on the robust reprojection error of every stored flow vector (ops.pose_normal_eq, csrc/pose.hip, over
    the rows of refine_plan; include/dvd_hip.h has the residual, its gates and the Jacobian).  The depth itself is held fixed.
      depth    [N,1,H,W] fp32 planar depth on the device; None: store.depth_pred
      weight   [N,H,W] fp32 on the device, > 0 where the scene is static (triangulate_depth's 'static' as float, or a motion
               segmentation); None: all ones -- Huber's loss alone does not keep a large moving object from pulling the poses
      gaps     the frame distances whose pairs are used (None: all)
      anchor   the frame that stays as it is (it fixes the gauge; with `scales` its scale stays 1)
      huber    px;  z_near: an observation whose point comes closer to the target camera's plane is not used, and costs as much
               as a residual as long as the image's diagonal
      max_iter, rel_tol   it stops after max_iter evaluations of a step, or when an accepted step lowers the cost by less than
               rel_tol of it, or -- the cost at its rounding floor -- when 5 steps in a row after an accepted one did not lower it
      tables   the cameras to start from (the store's layout); None: store.tables
    The loop runs on the host in float64: the 7N x 7N system of the unknowns (tau, omega, sigma) per frame -- c += R tau,
    R <- R Exp(omega), s = exp(sigma) -- without the anchor's columns, without sigma unless `scales`, without a frame no row
    touches; (H + lambda diag H) dx = -g with lambda from 1e-3, divided by 10 after a step that lowered the cost, multiplied by
    10 after one that did not (the state is kept).  Poses stay float64 between the steps and are rounded to fp32 for the
    kernel's tables.  One launch and one device-to-host copy of its sums per evaluation.
    -> dict:
      poses    fp32 [N,4,4] camera to world (a host tensor; FrameStore.set_cameras installs them)
      tables   the store's tables with these cameras, on the device (triangulate_depth(tables=...) takes them)
      scales   fp32 [N] on the device, ones without `scales`: store.depth_pred.mul_(scales.view(-1, 1, 1, 1)) applies them
      cost     the cost after every iteration, the start first (a float64 list)
      rms_before, rms_after   float64 [R]: sqrt(sum w |r|^2 / sum w) per row, in pixels (0 for a row without an observation)
      counts   int64 [R,2] at the end: the observations used, and those whose point lies behind z_near
      rows     int32 [R,4]: refine_plan's rows
      iterations, accepted, converged"""
    import numpy as np
    from . import ops
    from .datasets.frame_store import camera_tables
    what = 'refine_cameras'
    N, H, W = int(store.cat.n_frames), int(store.H), int(store.W)
    depth = store.depth_pred if depth is None else depth
    if not (torch.is_tensor(depth) and depth.dtype == torch.float32 and tuple(depth.shape) == (N, 1, H, W)):
        raise ValueError('%s: depth must be a float32 tensor [%d,1,%d,%d]' % (what, N, H, W))
    if weight is not None and not (torch.is_tensor(weight) and weight.dtype == torch.float32 and tuple(weight.shape) == (N, H, W)):
        raise ValueError('%s: weight must be a float32 tensor [%d,%d,%d] (e.g. tri["static"].float()) or None' % (what, N, H, W))
    rows = refine_plan(store.cat.pairs, N, gaps)
    if isinstance(anchor, (bool, np.bool_)) or not isinstance(anchor, (int, np.integer)) or not 0 <= anchor < N:
        raise ValueError('%s: anchor must be one of the frames 0 .. %d, got %r' % (what, N - 1, anchor))
    if not isinstance(scales, (bool, np.bool_)):
        raise ValueError('%s: scales must be True or False, got %r' % (what, scales))
    for name, v, lo_open in (('huber', huber, True), ('z_near', z_near, True), ('rel_tol', rel_tol, False)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not (
                (v > 0 if lo_open else v >= 0) and v <= 3.4028234663852886e+38):
            raise ValueError('%s: %s must be a finite number %s 0, got %r' % (what, name, '>' if lo_open else '>=', v))
    if isinstance(max_iter, (bool, np.bool_)) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise ValueError('%s: max_iter must be a positive integer, got %r' % (what, max_iter))
    start = store.tables if tables is None else tables
    keys = ('R', 't', 'K_T', 'K_inv_T')
    if not (isinstance(start, dict) and all(torch.is_tensor(start.get(k)) and start[k].dtype == torch.float32 and
                                            tuple(start[k].shape) == ((N, 3) if k == 't' else (N, 3, 3)) for k in keys)):
        raise ValueError('%s: tables must hold float32 R [%d,3,3], t [%d,3], K_T and K_inv_T [%d,3,3]' % (what, N, N, N))
    anchor, R = int(anchor), len(rows)
    _dev32(store.flow_1_2, 'flow_1_2')                       # (the wrapper checks the rest; this one before anything is pinned)
    # ---- the state: float64 poses and log-scales on the host
    host = store.host_tables if tables is None else {k: start[k].cpu() for k in ('R', 't')}
    poses = np.tile(np.eye(4), (N, 1, 1))
    poses[:, :3, :3], poses[:, :3, 3] = host['R'].numpy().astype(np.float64), host['t'].numpy().astype(np.float64)
    first32 = poses.astype(np.float32)
    sigma = np.zeros(N)
    seen = set(rows[:, 1:3].ravel().tolist())
    free = [i for i in range(7 * N) if i // 7 != anchor and i // 7 in seen and (scales or i % 7 != 6)]
    dev = store.flow_1_2.device if torch.is_tensor(store.flow_1_2) else store.device
    state = {}

    def evaluate(p64, sg):
        """One launch per chunk of rows -> (sums [R,106], wsum [R], counts [R,2]) on the host: one copy, the only wait."""
        p32 = p64.astype(np.float32)
        cam = torch.from_numpy(np.concatenate([p32[:, :3, :3].reshape(N, 9), p32[:, :3, 3]], 1)).pin_memory().to(dev, non_blocking=True)
        tab = {'R': cam[:, :9].contiguous().view(N, 3, 3), 't': cam[:, 9:].contiguous(), 'K_T': start['K_T'], 'K_inv_T': start['K_inv_T']}
        if 'buf' not in state:
            state['buf'] = torch.empty(R * (ops.POSE_SUMS + 3), device=dev, dtype=torch.int64)
        buf = state['buf']
        n_s = R * ops.POSE_SUMS
        sums, wsum = buf[:n_s].view(torch.float64).view(R, ops.POSE_SUMS), buf[n_s:n_s + R].view(torch.float64)
        counts = buf[n_s + R:].view(R, 2)
        for r0 in range(0, R, ops.POSE_MAX_ROWS):
            r1 = min(r0 + ops.POSE_MAX_ROWS, R)
            ops.pose_normal_eq(store.flow_1_2, store.flow_2_1, store.mask_1, store.mask_2, depth, weight, rows[r0:r1], tab,
                               sg if scales else None, huber, z_near,
                               out={'sums': sums[r0:r1], 'wsum': wsum[r0:r1], 'counts': counts[r0:r1]})
        h = buf.cpu().numpy()
        return h[:n_s].view(np.float64).reshape(R, ops.POSE_SUMS), h[n_s:n_s + R].view(np.float64), h[n_s + R:].reshape(R, 2)

    def rms(sums, wsum):
        return np.sqrt(np.divide(sums[:, 105], wsum, out=np.zeros(R), where=wsum > 0))

    sums, wsum, counts = evaluate(poses, sigma)
    Hm, g, cost = _pose_system(sums, rows, N)
    rms_before = rms(sums, wsum)
    hist, lam, accepted, rejected, converged, it = [cost], 1e-3, 0, 0, False, 0
    STALL = POSE_STALL
    for it in range(1, int(max_iter) + 1):
        Hf, gf = Hm[np.ix_(free, free)], g[free]
        A = Hf + lam * np.diag(np.diag(Hf))
        try:
            step = np.linalg.solve(A, -gf)
        except np.linalg.LinAlgError:
            step = np.linalg.lstsq(A, -gf, rcond=None)[0]
        dx = np.zeros(7 * N)
        dx[free] = step
        p2, s2 = poses.copy(), sigma.copy()
        for f in range(N):
            d = dx[7 * f:7 * f + 7]
            if d.any():
                p2[f, :3, 3] = poses[f, :3, 3] + poses[f, :3, :3] @ d[0:3]
                p2[f, :3, :3] = poses[f, :3, :3] @ _exp_so3(d[3:6])
                s2[f] = sigma[f] + d[6]
        sums2, wsum2, counts2 = evaluate(p2, s2)
        H2, g2, c2 = _pose_system(sums2, rows, N)
        if c2 < cost:
            small = cost - c2 < rel_tol * cost
            poses, sigma, Hm, g, cost, sums, wsum, counts = p2, s2, H2, g2, c2, sums2, wsum2, counts2
            lam, accepted, rejected = lam / 10, accepted + 1, 0
            hist.append(cost)
            if small:
                converged = True
                break
        else:
            lam, rejected = lam * 10, rejected + 1
            hist.append(cost)
            if accepted and rejected >= STALL:          # no step lowers the cost any more: it is at its rounding floor
                converged = True
                break
    out32 = poses.astype(np.float32)
    out32[anchor] = first32[anchor]
    new = camera_tables(store.host_tables, out32)
    if tables is not None:                                   # (the intrinsics of the start, which may differ from the store's)
        new['K_T'], new['K_inv_T'] = start['K_T'].cpu().clone(), start['K_inv_T'].cpu().clone()
    return {'poses': torch.from_numpy(out32), 'tables': {k: v.to(dev) for k, v in new.items()},
            'scales': torch.from_numpy(np.exp(sigma).astype(np.float32)).to(dev), 'cost': hist, 'rms_before': rms_before,
            'rms_after': rms(sums, wsum), 'counts': counts.copy(), 'rows': rows, 'iterations': it, 'accepted': accepted,
            'converged': converged}


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
