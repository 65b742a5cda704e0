"""The temporal depth filter restated in numpy on the CPU (test infrastructure).

What dvd_track_filter (csrc/track_filter.hip) and Model.filter_depth compute, from the contract in include/dvd_hip.h:
  fuse      rows of (z, depth_at, inside) -- what dvd_track_project_from writes for a two-sided slab -- gated and fused per pixel.
            dtype=np.float32 is the contract operation for operation (the kernel must match it bit for bit on the same rows);
            dtype=np.float64 is the reference.
  pipeline  invert_spec.chain -> invert_spec.project -> fuse: what Model.filter_depth computes from a depth video, with a
            "decided" flag per sample: both ratio gates have a relative margin of 1e-4 or more, |z - z_near| >= 1e-4 z_near and
            the landing point is 1e-3 px or more away from the image border (tracks_spec.edge_distance).  An undecided sample
            may count in one precision and not in the other, which moves a pixel's result by a whole sample.
"""
import numpy as np
import torch

import invert_spec as I
import tracks_spec as S

GATE_MARGIN, NEAR_MARGIN, EDGE_MARGIN = 1e-4, 1e-4, 1e-3


def _np(x, dtype):
    return np.asarray(x.detach().cpu() if torch.is_tensor(x) else x).astype(dtype)


def gates(z, depth_at, inside, frames_exist, origin, tol, z_near, dtype=np.float32):
    """-> (counts [T1,B,H,W] bool, r [T1,B,H,W] dtype): which rows count and their samples D / z; row `origin` always counts
    with r = 1."""
    z, D = _np(z, dtype), _np(depth_at, dtype)
    inside = np.asarray(inside.cpu() if torch.is_tensor(inside) else inside).astype(bool)
    exist = np.asarray(frames_exist.cpu() if torch.is_tensor(frames_exist) else frames_exist).astype(bool)
    one = dtype(1)
    tl = one + dtype(tol)
    with np.errstate(all='ignore'):
        counts = inside & (z >= dtype(z_near)) & (D > 0) & (z <= D * tl) & (D <= z * tl) & exist[:, :, None, None]
        r = D / z
    counts[origin] = True
    r[origin] = one
    return counts, r


def fuse(z, depth_at, inside, d0, frames_exist, weights, origin, mode='mean', tol=0.1, z_near=1e-3, dtype=np.float32):
    """z, depth_at, inside [T1,B,H,W]; d0 [B,H,W] or [B,1,H,W] (the start frames' own depth); frames_exist [T1,B]; weights
    [T1]; origin: the start frames' row -> dict of depth, ratio, spread [B,1,H,W] in dtype and count uint8 [B,H,W]."""
    counts, r = gates(z, depth_at, inside, frames_exist, origin, tol, z_near, dtype)
    T1, B, H, W = r.shape
    d0 = _np(d0, dtype).reshape(B, H, W)
    w = np.asarray(weights, dtype=np.float64).astype(np.float32).astype(dtype)      # the kernel gets fp32 weights
    n = counts.sum(0)
    with np.errstate(all='ignore'):
        if mode == 'mean':
            acc, ws = np.zeros((B, H, W), dtype), np.zeros((B, H, W), dtype)
            for k in range(T1):                         # ascending rows; the multiply and the add are two operations
                term = (w[k] * r[k]).astype(dtype)
                acc = np.where(counts[k], (acc + term).astype(dtype), acc)
                ws = np.where(counts[k], (ws + w[k]).astype(dtype), ws)
            ratio = (acc / ws).astype(dtype)
        elif mode == 'median':
            srt = np.sort(np.where(counts, r, dtype(np.inf)), axis=0)                # the counting samples first
            lo = np.take_along_axis(srt, ((n - 1) // 2)[None], 0)[0]
            hi = np.take_along_axis(srt, (n // 2)[None], 0)[0]
            ratio = np.where(n % 2 == 1, lo, ((lo + hi).astype(dtype) * dtype(0.5)).astype(dtype))
        else:
            raise ValueError(mode)
        big = np.where(counts, r, dtype(-np.inf)).max(0)
        small = np.where(counts, r, dtype(np.inf)).min(0)
        spread = (big - small).astype(dtype)
        ok = d0 > 0                                                                  # False for NaN
        out = {'depth': np.where(ok, (d0 * ratio).astype(dtype), d0).reshape(B, 1, H, W),
               'ratio': np.where(ok, ratio, dtype(1)).astype(dtype).reshape(B, 1, H, W),
               'spread': np.where(ok, spread, dtype(0)).astype(dtype).reshape(B, 1, H, W),
               'count': np.where(ok, n, 0).astype(np.uint8)}
    return out


def decided(z, depth_at, uv, frames_exist, origin, tol, z_near, H, W):
    """[T1,B,H,W] bool from the float64 rows: True where a sample's gates are clear of their thresholds (rows without a frame
    and the origin row are decided)."""
    z, D = _np(z, np.float64), _np(depth_at, np.float64)
    exist = np.asarray(frames_exist).astype(bool)
    tl = 1.0 + tol
    edge, _ = S.edge_distance(torch.as_tensor(np.asarray(uv, dtype=np.float64)), torch.as_tensor(z), H, W)
    ok = (np.abs(z - D * tl) >= GATE_MARGIN * np.abs(D * tl)) & (np.abs(D - z * tl) >= GATE_MARGIN * np.abs(z * tl)) & \
         (np.abs(z - z_near) >= NEAR_MARGIN * z_near) & (edge.numpy() >= EDGE_MARGIN)
    ok |= ~exist[:, :, None, None]
    ok[origin] = True
    return ok


def pipeline(sd, depth_all, tabs, ts, start, radius, weights, mode='mean', tol=0.1, z_near=1e-3, sf_mag_div=100.0, n_iter=4,
             dtype=np.float32):
    """Model.filter_depth(frames=start) from the depth video depth_all [N,1,H,W]: tabs holds the tables R_T, K_inv_T, R, t,
    K_T ([N,..] arrays), ts the start frames' time stamps [B,1,H,W] or None, sd the scene-flow network's state dict.
    -> fuse's dict plus 'decided' [T1,B,H,W] (from the rows of THIS dtype's run; use the float64 run's), 'counts' and 'rows'."""
    tdtype = torch.float32 if dtype == np.float32 else torch.float64
    depth_all = np.asarray(depth_all)
    N, _, H, W = depth_all.shape
    start = [int(s) for s in start]
    p0 = S.unproject(depth_all[start], tabs['R_T'][start], tabs['t'][start], tabs['K_inv_T'][start])
    pts, _ = I.chain(sd, p0, ts, 1.0 / N, start, N, radius, radius, sf_mag_div, n_iter=n_iter, dtype=tdtype)
    rows = I.project(pts, start, tabs['R'], tabs['t'], tabs['K_T'], depth_all, k0=-radius, dtype=tdtype)
    out = fuse(rows['z'], rows['depth_at'], rows['inside'], depth_all[start], rows['live'], weights, radius, mode, tol, z_near,
               dtype)
    out['counts'], _ = gates(rows['z'], rows['depth_at'], rows['inside'], rows['live'], radius, tol, z_near, dtype)
    out['decided'] = decided(rows['z'], rows['depth_at'], rows['uv'], rows['live'], radius, tol, z_near, H, W)
    out['rows'] = rows
    return out
