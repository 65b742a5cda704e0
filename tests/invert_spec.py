"""Backward-in-time advection restated in plain torch on the CPU (test infrastructure).

One Euler step of the scene-flow chain is x -> x + s f(x, t) with s = 1 / sf_mag_div (tests/tracks_spec.py, integrate).  The
point y this step carries to p is the fixed point of y <- p - s f(y, t), iterated from y = p:
  invert_step   the iteration, with the per-image residual max |y_(i+1) - y_i| of every round
  chain         the two-sided slab of Model.track(n_back=..): row n_back is the start frame, row j is frame start + j - n_back,
                backward step j evaluates the field at t - j * time_step, forward step k at t + k * time_step
  project       tracks_spec.project with a row offset k0: row k looks up frame start + k + k0, zeros on either side of the video
dtype=torch.float64 is the specification (helpers.mlp_oracle_f64: fp32 embedding, float64 convolutions, float64 everywhere
else).  dtype=torch.float32 evaluates the same torch expressions the way the reference evaluates its forward chain
(oracle.sceneflow_mlp.mlp_forward, the division by sf_mag_div) in its own precision: its distance from the float64 form is
what fp32 can do on the given inputs, the yardstick of tests/test_57_track_back_gpu.py.
"""
import torch

import tracks_spec as S


def field(sd, y, t, sf_mag_div, dtype=torch.float64):
    """s f(y, t): y [B,3,H,W], t [B,1,H,W] or None -> [B,3,H,W] in dtype."""
    if dtype == torch.float64:
        import helpers
        return helpers.mlp_oracle_f64({k: v.double() for k, v in sd.items()}, y, t) * (1.0 / sf_mag_div)
    from oracle import sceneflow_mlp as M
    return M.mlp_forward({k: v.float() for k, v in sd.items()}, y.float(), None if t is None else t.float()) / sf_mag_div


def invert_step(sd, p, t, sf_mag_div, n_iter=4, dtype=torch.float64, residuals=None):
    """y with y + s f(y, t) = p after n_iter rounds from y = p.  residuals: a list that receives, per round, the tensor [B] of
    max |y_(i+1) - y_i| per image."""
    p = torch.as_tensor(p).to(dtype)
    t = None if t is None else torch.as_tensor(t).to(dtype)
    y = p
    for _ in range(n_iter):
        y_new = p - field(sd, y, t, sf_mag_div, dtype)
        if residuals is not None:
            residuals.append((y_new - y).abs().flatten(1).max(1).values)
        y = y_new
    return y


def forward_step(sd, p, t, sf_mag_div, dtype=torch.float64):
    p = torch.as_tensor(p).to(dtype)
    return p + field(sd, p, None if t is None else torch.as_tensor(t).to(dtype), sf_mag_div, dtype)


def chain(sd, p0, ts, time_step, start, n_frames, n_back, n_steps, sf_mag_div, n_iter=4, dtype=torch.float64):
    """-> (points [n_back + 1 + n_steps,B,3,H,W], resid [n_back,B]) in dtype: row n_back = p0; rows without a frame and their
    residuals are zero.  ts [B,1,H,W] (the start frames' time stamps) or None."""
    p0 = torch.as_tensor(p0).to(dtype)
    ts = None if ts is None else torch.as_tensor(ts).to(dtype)
    B = p0.shape[0]
    pts = torch.zeros((n_back + 1 + n_steps,) + tuple(p0.shape), dtype=dtype)
    resid = torch.zeros(n_back, B, dtype=dtype)
    pts[n_back] = p0
    for k in range(n_steps):
        rows = [b for b in range(B) if int(start[b]) + k + 1 < n_frames]
        if rows:
            pts[n_back + k + 1, rows] = forward_step(sd, pts[n_back + k, rows], None if ts is None else ts[rows] + k * time_step,
                                                     sf_mag_div, dtype)
    for j in range(1, n_back + 1):
        rows = [b for b in range(B) if int(start[b]) - j >= 0]
        if rows:
            res = []
            pts[n_back - j, rows] = invert_step(sd, pts[n_back - j + 1, rows], None if ts is None else ts[rows] - j * time_step,
                                                sf_mag_div, n_iter, dtype, res)
            resid[j - 1, rows] = res[-1]
    return pts, resid


def _project_fp32(points, frames, R, t, K_T, depth_all):
    """One row in the reference's own precision and order of operations: project_ptcld's matmuls and division, its displacement
    field, BackwardWarp's normalise / grid_sample round trip (oracle.geometry.flow_sample).  points [B,3,H,W], frames B ints ->
    what tracks_spec.project returns for one row, as float64 copies of the fp32 results (uv = displacement + pixel, added in
    float64 as tests/test_45_tracks_gpu.py does with the fixture's displacement)."""
    from oracle import geometry as G
    points = torch.as_tensor(points).float()
    R, t, K_T = (torch.as_tensor(v).float() for v in (R, t, K_T))
    B, _, H, W = points.shape
    grid = G.pixel_grid(H, W)
    xx, yy = S._pixel_grid(H, W)
    out = {'uv': torch.zeros(1, B, H, W, 2, dtype=torch.float64), 'z': torch.zeros(1, B, H, W, dtype=torch.float64),
           'inside': torch.zeros(1, B, H, W, dtype=torch.bool), 'live': torch.ones(1, B, dtype=torch.bool)}
    if depth_all is not None:
        out['depth_at'] = torch.zeros(1, B, H, W, dtype=torch.float64)
    for b, g in enumerate(frames):
        P = points[b].permute(1, 2, 0).reshape(1, H, W, 1, 3)
        img = torch.matmul(torch.matmul(P - t[g].view(1, 1, 1, 1, 3), R[g].view(1, 1, 1, 3, 3)), K_T[g].view(1, 1, 1, 3, 3))
        disp = ((img / (img[..., -1:] + 1e-8))[..., :-1] - grid[..., :2]).view(1, H, W, 2)
        z = img[0, :, :, 0, 2]
        uv = disp[0].double() + torch.stack([xx, yy], -1)
        out['uv'][0, b], out['z'][0, b] = uv, z.double()
        out['inside'][0, b] = (z > 0) & (uv[..., 0] >= 0) & (uv[..., 0] <= W - 1) & (uv[..., 1] >= 0) & (uv[..., 1] <= H - 1)
        if depth_all is not None:
            d = G.flow_sample(torch.as_tensor(depth_all[g]).float().view(1, 1, H, W), disp.clone(), grid)[0, 0]
            out['depth_at'][0, b] = torch.where(z > 0, d, torch.zeros_like(d)).double()
    return out


def project(points, start, R, t, K_T, depth_all=None, k0=0, dtype=torch.float64):
    """tracks_spec.project where row k of image b looks up frame start[b] + k + k0; a frame < 0 or >= N gives zeros and is not
    `live`.  dtype=torch.float32: the projection and the depth sample the way the reference evaluates them (_project_fp32)."""
    points = torch.as_tensor(points)
    points = points.double() if dtype == torch.float64 else points.float()
    T1, B, _, H, W = points.shape
    N = torch.as_tensor(R).shape[0]
    out = {'uv': torch.zeros(T1, B, H, W, 2, dtype=torch.float64), 'z': torch.zeros(T1, B, H, W, dtype=torch.float64),
           'inside': torch.zeros(T1, B, H, W, dtype=torch.bool), 'live': torch.zeros(T1, B, dtype=torch.bool)}
    if depth_all is not None:
        out['depth_at'] = torch.zeros(T1, B, H, W, dtype=torch.float64)
    for k in range(T1):
        rows = [b for b in range(B) if 0 <= int(start[b]) + k + k0 < N]
        if not rows:
            continue
        frames = [int(start[b]) + k + k0 for b in rows]
        if dtype == torch.float64:
            one = S.project(points[k:k + 1, rows], frames, R, t, K_T, depth_all)
        else:
            one = _project_fp32(points[k, rows], frames, R, t, K_T, depth_all)
        for name, v in one.items():
            out[name][k, rows] = v[0]
    return out
