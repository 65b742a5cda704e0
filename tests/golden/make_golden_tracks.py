#!/usr/bin/env python
"""Generate the long-range track fixture (tracks_b3_11x21_t4.npz) from the REAL reference.

Run in the build container only (it imports /root/reference):

    python tests/golden/make_golden_tracks.py

A seeded 7-frame video at 11 x 21 (odd width, H * W = 231 no multiple of 64): per-frame cameras as the frame files carry them
(pose_c2w, intrinsics -> the tables of datasets/frame_store.py), per-frame depth maps (synthetic.make_depths), the `vali` item's
time stamps and time step (datasets/davis_sequence.py:120,124), and a SceneFlowFieldNet filled by helpers.seeded_fill_ (the
weights are not stored).  Start frames [0, 3, 5] and 4 steps: the third start frame runs past the end of the video, and the
last camera is turned away, so everything projected into it has a negative z.  Every stored result is computed by the
reference's own code:
  points    unproject_ptcld, then p_0 + Model.forward_sf_net_multi_step(p_0, ts, time_step, k) for k = 0 .. 4
  disp      project_ptcld into the camera of frame f + k (its return value, the displacement field)
  z         scene_flow_projection_slack's depth_image_1_2 with a zero first depth and camera, so that its global_p1 + sflow_1_2
            IS the stored point (0 + p, exact) and the surface is the third component of ((p - t) @ R_T) @ K
  depth_at  BackwardWarp()(depth[f + k], disp)
  g_points  autograd of project_ptcld for seeded upstream gradients
and `ref_vs_f64_*` is the worst distance of those fp32 results from the float64 restatement (tests/tracks_spec.py) of the same
fp32 inputs.  Rows past the end of the video are zero.  The generator refuses a geometry whose `inside` flags or divisions are
badly conditioned: no |z| < 0.1, fewer than 0.5 % of the points within 1e-3 px of an image edge.
"""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the reference, the package and the repository root on sys.path)

sys.path.insert(0, os.path.join(MG.ROOT, 'tests'))
import helpers  # noqa: E402
import tracks_spec as S  # noqa: E402

NAME = 'tracks_b3_11x21_t4'
CASE = dict(N=7, H=11, W=21, start=(0, 3, 5), n_steps=4, seed=311, turned=6)


def _rot(axis, a):
    c, s = math.cos(a), math.sin(a)
    m = {'x': [[1, 0, 0], [0, c, -s], [0, s, c]], 'y': [[c, 0, s], [0, 1, 0], [-s, 0, c]]}[axis]
    return np.array(m, dtype=np.float64)


def video(N, H, W, seed, turned):
    """Per-frame pose_c2w / intrinsics (float64, as the frame files hold them) and depth maps."""
    poses, Ks = [], []
    for i in range(N):
        pose = np.eye(4)
        pose[:3, :3] = _rot('y', 0.02 * i + (math.pi if i == turned else 0.0)) @ _rot('x', 0.01 * i)
        pose[:3, 3] = [0.05 * i, 0.02 * i, 0.01 * i]
        f = 0.9 * W * (1.0 + 0.01 * i)
        poses.append(pose)
        Ks.append(np.array([[f, 0.0, (W - 1) / 2.0 + 0.1 * i], [0.0, f, (H - 1) / 2.0], [0.0, 0.0, 1.0]]))
    d1, d2 = MG.synthetic.make_depths(N, H, W, seed=seed + 1, far_depth_frac=0.0)
    return poses, Ks, d1.contiguous()


def tables(poses, Ks):
    from dvd_hip.datasets import frame_store
    tab = frame_store._new_tables(len(poses))
    for i, (pose, K) in enumerate(zip(poses, Ks)):
        frame_store._set_camera_row(tab, i, pose, K)
    return tab


def write(name=NAME, case=CASE):
    from losses.scene_flow_projection import BackwardWarp, project_ptcld, scene_flow_projection_slack, unproject_ptcld
    from models.scene_flow_motion_field import Model
    from networks.sceneflow_field import SceneFlowFieldNet
    from dvd_hip.models.tracks import track_plan
    N, H, W, seed, n_steps = case['N'], case['H'], case['W'], case['seed'], case['n_steps']
    start = list(case['start'])
    B, T1 = len(start), n_steps + 1
    poses, Ks, depth = video(N, H, W, seed, case['turned'])
    tab = tables(poses, Ks)
    valid = track_plan(N, start, n_steps)

    net = SceneFlowFieldNet(net_width=256, n_layers=4, time_dependent=True, N_freq_xyz=16, N_freq_t=16)
    helpers.seeded_fill_(net, seed)
    model = Model.__new__(Model)
    model.opt = SimpleNamespace(use_cnn=False, time_dependent=True, sf_mag_div=100.0)
    model.net_sceneflow = net
    time_step = 1.0 / (N + 0.0)
    ts = tab['ts_vali'][start].view(B, 1, 1, 1).expand(B, 1, H, W).contiguous()

    def cam(k, rows):
        g = [start[b] + k for b in rows]
        n = len(rows)
        return (tab['R'][g].view(n, 1, 1, 3, 3), tab['t'][g].view(n, 1, 1, 1, 3), tab['K_T'][g].view(n, 1, 1, 3, 3), g)

    with torch.no_grad():
        p0 = unproject_ptcld()(depth[start], tab['R_T'][start].view(B, 1, 1, 3, 3), tab['t'][start].view(B, 1, 1, 1, 3),
                               tab['K_inv_T'][start].view(B, 1, 1, 3, 3))
        p0 = p0.squeeze(3).permute(0, 3, 1, 2).contiguous()                      # planar, what the MLP takes
        points = torch.zeros(T1, B, 3, H, W)
        points[0] = p0
        for k in range(1, T1):
            rows = [b for b in range(B) if valid[b] >= k]
            if rows:
                points[k, rows] = p0[rows] + model.forward_sf_net_multi_step(p0[rows], ts[rows], time_step, k)

    disp, z = torch.zeros(T1, B, H, W, 2), torch.zeros(T1, B, H, W)
    depth_at, g_points = torch.zeros(T1, B, H, W), torch.zeros(T1, B, 3, H, W)
    up = torch.randn(T1, B, H, W, 2, generator=torch.Generator().manual_seed(seed + 2))
    for k in range(T1):
        rows = [b for b in range(B) if valid[b] >= k]
        if not rows:
            continue
        n = len(rows)
        R, t, K, g = cam(k, rows)
        P = points[k, rows].permute(0, 2, 3, 1)[..., None, :].contiguous().requires_grad_(True)       # [n,H,W,1,3]
        d = project_ptcld()(P, R, t, K).reshape(n, H, W, 2)
        (d * up[k, rows]).sum().backward()
        disp[k, rows] = d.detach()
        g_points[k, rows] = P.grad.squeeze(3).permute(0, 3, 1, 2)
        with torch.no_grad():
            depth_at[k, rows] = BackwardWarp()(depth[g], d.detach())[:, 0]
            eye, zero3 = torch.eye(3).view(1, 1, 1, 3, 3).repeat(n, 1, 1, 1, 1), torch.zeros(n, 1, 1, 1, 3)
            flow0 = torch.zeros(n, H, W, 2)
            s = scene_flow_projection_slack()(torch.zeros(n, 1, H, W), torch.ones(n, 1, H, W), flow0, flow0, eye, eye, eye, R,
                                              zero3, t, K, tab['K_inv_T'][g].view(n, 1, 1, 3, 3), P.detach(),
                                              torch.zeros(n, H, W, 1, 3))
            z[k, rows] = s['depth_image_1_2'][:, 0]

    # conditioning of the case, on the float64 restatement of the same fp32 points
    spec = S.project(points, start, tab['R'], tab['t'], tab['K_T'], depth)
    live = spec['live'][:, :, None, None].expand(T1, B, H, W)
    edge, absz = S.edge_distance(spec['uv'], spec['z'], H, W)
    assert float(absz[live].min()) >= 0.1, 'a stored point has |z| = %g' % float(absz[live].min())
    # (step 0 projects every pixel onto itself: the border pixels of a start frame lie ON an image edge by construction, and
    #  only they do; the bound is for the steps that look into another camera)
    near = float((edge[1:][live[1:]] < 1e-3).double().mean())
    assert near < 0.005, '%.2f %% of the points lie within 1e-3 px of an image edge' % (100 * near)
    assert bool(((edge[0] < 1e-3) == S.border_pixels(H, W)).all()), 'step 0: a point other than a border pixel is near an edge'
    assert bool((spec['z'][live] < 0).any()) and bool((spec['z'][live] > 0).any()), 'the case needs both signs of z'

    xx, yy = S._pixel_grid(H, W)
    coord = torch.stack([xx, yy], -1)
    sd = {k_: v for k_, v in net.state_dict().items()}
    p0_64 = S.unproject(depth[start], tab['R_T'][start], tab['t'][start], tab['K_inv_T'][start])
    chain = S.integrate(sd, p0_64, ts, time_step, valid, n_steps, 1.0 / 100.0)
    front = live & (spec['z'] > 0)
    out = {'N': np.array(N), 'H': np.array(H), 'W': np.array(W), 'seed': np.array(seed), 'n_steps': np.array(n_steps),
           'start': np.array(start, dtype=np.int64), 'steps_valid': np.array(valid, dtype=np.int64),
           'time_step': np.array(time_step, dtype=np.float64), 'in_depth': depth.numpy(), 'in_up_uv': up.numpy(),
           'in_pose_c2w': np.stack(poses), 'in_intrinsics': np.stack(Ks),
           'ref_points': points.numpy(), 'ref_disp': disp.numpy(), 'ref_z': z.numpy(), 'ref_depth_at': depth_at.numpy(),
           'ref_g_points': g_points.numpy()}
    for k_ in ('R_T', 'R', 't', 'K_T', 'K_inv_T', 'ts_vali'):
        out['tab_' + k_] = tab[k_].numpy()
    out['ref_vs_f64_points'] = np.array(S.worst((points.double() - points[0].double())[1:], (chain - chain[0])[1:]))
    out['ref_vs_f64_uv'] = np.array(S.worst(disp, spec['uv'] - coord, live[..., None].expand_as(disp)))
    out['ref_vs_f64_z'] = np.array(S.worst(z, spec['z'], live))
    out['ref_vs_f64_depth_at'] = np.array(S.worst(depth_at, spec['depth_at'], front))
    out['ref_vs_f64_g_points'] = np.array(S.worst(g_points, S.project_grad(up, points, start, tab['R'], tab['t'], tab['K_T'])))
    np.savez_compressed(os.path.join(MG.OUT_DIR, name + '.npz'), **out)
    print('wrote', name, {k_: float(v) for k_, v in out.items() if k_.startswith('ref_vs_f64')},
          'min|z| %.3f, near an edge %.2f %%, outside %.1f %%, behind %.1f %%' % (
              float(absz[live].min()), 100 * near, 100 * float((~spec['inside'][live]).double().mean()),
              100 * float((spec['z'][live] < 0).double().mean())))


if __name__ == '__main__':
    torch.set_num_threads(4)
    write()
