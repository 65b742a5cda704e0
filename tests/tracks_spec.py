"""The long-range track pipeline restated in float64 (test infrastructure; plain torch on the CPU).

What dvd_track_project, dvd_project_bwd and Model.track compute, from the reference's formulas and nothing of the product:
  unproject   losses/scene_flow_projection.py:54-67    P = (depth * ((x, y, 1) @ K_inv)) @ R + t
  project     :27-44                                   I = ((P - t) @ R_T) @ K ;  uv = I.xy / (I.z + 1e-8)
  sample      :289-297 + F.grid_sample                 bilinear, padding 'border', align_corners=True, at uv
  integrate   models/scene_flow_motion_field.py:360-367  Euler steps of the scene-flow MLP (helpers.mlp_oracle_f64)
Inputs are the fp32 values the kernels get, promoted; every operation is float64.  Layouts are the kernels': points
[T1,B,3,H,W], uv [T1,B,H,W,2], z / depth_at / inside [T1,B,H,W]; step k of image b uses frame start[b] + k of the tables, and a
frame past the end gives zeros.
"""
import numpy as np
import torch


def _pixel_grid(H, W):
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    return xx, yy


def unproject(depth, R, t, K_inv):
    """depth [B,1,H,W], R / K_inv [B,3,3] (the reference's R_1 / K_inv), t [B,3] -> planar points [B,3,H,W]."""
    depth, R, t, K_inv = (torch.as_tensor(v).double() for v in (depth, R, t, K_inv))
    B, _, H, W = depth.shape
    xx, yy = _pixel_grid(H, W)
    coord = torch.stack([xx, yy, torch.ones_like(xx)], -1).view(1, H * W, 3)
    ray = coord @ K_inv                                         # [B,HW,3]
    P = (depth.view(B, H * W, 1) * ray) @ R + t.view(B, 1, 3)
    return P.permute(0, 2, 1).reshape(B, 3, H, W)


def sample_border(img, u, v):
    """grid_sample(img [H,W], bilinear, border, align_corners=True) at pixel positions (u, v) of any shape."""
    H, W = img.shape
    ix, iy = u.clamp(0, W - 1), v.clamp(0, H - 1)
    ix, iy = torch.nan_to_num(ix, nan=0.0), torch.nan_to_num(iy, nan=0.0)
    x0, y0 = ix.floor(), iy.floor()
    wx, wy = ix - x0, iy - y0
    x0, y0 = x0.long(), y0.long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)      # a tap past the border has weight 0
    return (img[y0, x0] * (1 - wy) * (1 - wx) + img[y0, x1] * (1 - wy) * wx + img[y1, x0] * wy * (1 - wx) +
            img[y1, x1] * wy * wx)


def project(points, start, R, t, K_T, depth_all=None):
    """-> dict of float64 uv, z, inside (bool) and, with depth_all [N,1,H,W], depth_at; `live` [T1,B] marks the rows that
    have a target frame."""
    points = torch.as_tensor(points).double()
    R, t, K_T = (torch.as_tensor(v).double() for v in (R, t, K_T))
    T1, B, _, H, W = points.shape
    N = R.shape[0]
    uv = torch.zeros(T1, B, H, W, 2, dtype=torch.float64)
    z = torch.zeros(T1, B, H, W, dtype=torch.float64)
    depth_at = torch.zeros(T1, B, H, W, dtype=torch.float64) if depth_all is not None else None
    inside = torch.zeros(T1, B, H, W, dtype=torch.bool)
    live = torch.zeros(T1, B, dtype=torch.bool)
    for k in range(T1):
        for b in range(B):
            g = int(start[b]) + k
            if g >= N:
                continue
            live[k, b] = True
            P = points[k, b].reshape(3, H * W).T
            I = ((P - t[g]) @ R[g]) @ K_T[g]
            c = I[:, :2] / (I[:, 2:] + 1e-8)
            uv[k, b] = c.view(H, W, 2)
            z[k, b] = I[:, 2].view(H, W)
            u, v = uv[k, b, ..., 0], uv[k, b, ..., 1]
            front = z[k, b] > 0
            inside[k, b] = front & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
            if depth_all is not None:
                d = sample_border(torch.as_tensor(depth_all[g, 0]).double(), u, v)
                depth_at[k, b] = torch.where(front, d, torch.zeros_like(d))
    out = {'uv': uv, 'z': z, 'inside': inside, 'live': live}
    if depth_all is not None:
        out['depth_at'] = depth_at
    return out


def edge_distance(uv, z, H, W):
    """How far, in pixels (and in depth units for z), a point is from changing its `inside` flag: min over |u|, |u - (W-1)|,
    |v|, |v - (H-1)|; and |z|."""
    u, v = uv[..., 0], uv[..., 1]
    d = torch.stack([u.abs(), (u - (W - 1)).abs(), v.abs(), (v - (H - 1)).abs()], 0).min(0).values
    return d, z.abs()


def border_pixels(H, W):
    """[H,W] bool: the pixels of the image's outermost rows and columns."""
    m = torch.zeros(H, W, dtype=torch.bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return m


def compare_inside(got, spec, H, W, self_rows=0):
    """`inside` of a kernel against the spec -> (mismatches among the compared points, fraction of points left out).  A point
    is left out where the float64 position is within 1e-3 px of an image edge or has |z| < 1e-4: there the flag hangs on the
    last bits.  self_rows: leading steps that project a frame's own pixels into its own camera (step 0 of a track) -- every
    pixel lands on itself, so exactly the border pixels sit ON an edge; those rows are checked for that (nothing but the border
    may be left out) and do not count in the fraction, which is about the steps that look into another camera."""
    edge, absz = edge_distance(spec['uv'], spec['z'], H, W)
    live = spec['live'][:, :, None, None].expand_as(edge)
    skip = ((edge < 1e-3) | (absz < 1e-4)) & live
    if self_rows:
        own = skip[:self_rows] & ~border_pixels(H, W)
        assert not bool(own.any()), 'a step into the own camera leaves out %d points that are no border pixels' % int(own.sum())
    rest = live[self_rows:]
    frac = float(skip[self_rows:][rest].double().mean()) if bool(rest.any()) else 0.0
    got = torch.as_tensor(got).bool()
    bad = int(((got != spec['inside']) & ~skip).sum())
    return bad, frac


def project_grad(g_uv, points, start, R, t, K_T, dtype=torch.float64):
    """J^T g_uv by autograd through `project`'s own formula -> the layout of points.  dtype=torch.float64 is the
    specification; torch.float32 is the same torch expression the reference evaluates (project_ptcld :38-41 under autograd) in
    its own precision: its distance from the float64 result is what fp32 can do on the given inputs."""
    points = torch.as_tensor(points).to(dtype).clone().requires_grad_(True)
    R, t, K_T = (torch.as_tensor(v).to(dtype) for v in (R, t, K_T))
    g_uv = torch.as_tensor(g_uv).to(dtype)
    T1, B, _, H, W = points.shape
    total = torch.zeros((), dtype=dtype)
    for k in range(T1):
        for b in range(B):
            g = int(start[b]) + k
            if g >= R.shape[0]:
                continue
            P = points[k, b].reshape(3, H * W).T
            I = ((P - t[g]) @ R[g]) @ K_T[g]
            c = I[:, :2] / (I[:, 2:] + 1e-8)
            total = total + (c.view(H, W, 2) * g_uv[k, b]).sum()
    total.backward()
    return points.grad


def integrate(sd, p0, ts, time_step, valid, n_steps, inv_div, n_freq_xyz=16, n_freq_t=16):
    """The Euler chain: points [n_steps+1,B,3,H,W] float64 with row 0 = p0; row k + 1 of image b is row k plus the MLP's output
    times inv_div while valid[b] > k, zero afterwards.  sd: the network's state dict (float64 convolutions, fp32 embedding:
    helpers.mlp_oracle_f64); ts [B,1,H,W] or None for a time-independent network."""
    import helpers
    sd = {k: v.double() for k, v in sd.items()}
    p0 = torch.as_tensor(p0).double()
    B = p0.shape[0]
    out = torch.zeros((n_steps + 1,) + tuple(p0.shape), dtype=torch.float64)
    out[0] = p0
    for k in range(n_steps):
        rows = [b for b in range(B) if valid[b] > k]
        if not rows:
            break
        p = out[k, rows]
        t = None if ts is None else torch.as_tensor(ts).double()[rows] + k * time_step
        sf = helpers.mlp_oracle_f64(sd, p, t, n_freq_xyz, n_freq_t) * inv_div
        out[k + 1, rows] = p + sf
    return out


def worst(a, b, mask=None):
    """max |a - b| over the elements `mask` selects (all when None), as a float."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = np.abs(a - b)
    if mask is not None:
        d = d[np.asarray(mask)]
    return float(d.max()) if d.size else 0.0
