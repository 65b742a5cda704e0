"""dvd_eval_tracks / Model.evaluate restated in float64 (test infrastructure; plain torch on the CPU, nothing of the product).

Row r of image b holds the world points of frame source[b]'s pixels at the time of frame g = source[b] + k_first + r.  On top
of tracks_spec.project (u, v, z, inside, the bilinear border sample of the target's depth) and tracks_spec.sample_border:
    occluded = inside & (z > d * (1 + z_tol))            seen = inside & ~occluded
    rel      = min(|z - d| / max(d, d_min), 1)                                         where seen
    photo    = min(sum_c |img_all[g] at (u, v) - own colour| / 3, 1024)                 where seen
    epe      = min(hypot((u - x) - flow.x, (v - y) - flow.y), 1024)  where the row has a pair, mask == 0 and z > 0
Maps hold -1 where a point does not count; the six sums of a row are exact Python integers of round(x * 2^shift) over the
spec's own maps.  A point is `fragile` where the float64 decision hangs on the last bits: within 1e-3 px of an image edge or
|z| < 1e-4 (the rule of tracks_spec.compare_inside), or |z - d (1 + z_tol)| < 1e-4 d.

Every function takes dtype: torch.float64 is the specification, torch.float32 the same expressions in the kernels' precision --
its distance from the float64 run is what fp32 can do on the inputs, the yardstick of the GPU tests.

`kernel_case` and `KERNEL_SHAPES` are the inputs of tests/test_51_eval_kernel_gpu.py; tests/test_eval_cpu.py checks, under this
specification alone, that at most FRAGILE_CAP of their live points are fragile.
"""
import numpy as np
import torch

import store_spec
import tracks_spec as S

CAP = 1024.0
FRAGILE_CAP = 0.01
SUMS = ('n_inside', 'n_occluded', 'rel', 'photo', 'n_flow', 'epe')


def ceil_log2(n):
    k = 0
    while (1 << k) < n:
        k += 1
    return k


def shift_for(n_pixels):
    return min(32, 62 - 10 - ceil_log2(n_pixels))


def _project(points, start, R, t, K_T, depth_all, dtype):
    """tracks_spec.project; for another dtype the same expressions evaluated in it."""
    if dtype == torch.float64:
        return S.project(points, start, R, t, K_T, depth_all)
    points = torch.as_tensor(points).to(dtype)
    R, t, K_T = (torch.as_tensor(v).to(dtype) for v in (R, t, K_T))
    T1, B, _, H, W = points.shape
    N = R.shape[0]
    out = {'uv': torch.zeros(T1, B, H, W, 2, dtype=dtype), 'z': torch.zeros(T1, B, H, W, dtype=dtype),
           'depth_at': torch.zeros(T1, B, H, W, dtype=dtype), 'inside': torch.zeros(T1, B, H, W, dtype=torch.bool),
           'live': torch.zeros(T1, B, dtype=torch.bool)}
    for k in range(T1):
        for b in range(B):
            g = int(start[b]) + k
            if g >= N:
                continue
            out['live'][k, b] = True
            P = points[k, b].reshape(3, H * W).T
            I = ((P - t[g]) @ R[g]) @ K_T[g]
            c = (I[:, :2] / (I[:, 2:] + 1e-8)).view(H, W, 2)
            z = I[:, 2].view(H, W)
            u, v = c[..., 0], c[..., 1]
            front = z > 0
            out['uv'][k, b], out['z'][k, b] = c, z
            out['inside'][k, b] = front & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
            d = S.sample_border(torch.as_tensor(depth_all[g, 0]).to(dtype), u, v)
            out['depth_at'][k, b] = torch.where(front, d, torch.zeros_like(d))
    return out


def evaluate(points, source, k_first, R, t, K_T, depth_all, img_all, pairs=None, z_tol=0.05, d_min=1e-3, dtype=torch.float64):
    """points [T,B,3,H,W], source B frame ids, tables [N,...], depth_all [N,1,H,W], img_all [N,3,H,W]; pairs None or (pair_row
    [T,B], flow_1_2 [P,H,W,2], mask uint8 [P,H,W], 0 = valid).  -> dict of maps [T,B,3,H,W] (dtype), sums [T][B] lists of six
    Python integers, shift, fragile / inside / occluded / front [T,B,H,W] bool, live [T,B], n_fragile [T][B]."""
    points = torch.as_tensor(points)
    T, B, _, H, W = points.shape
    N = int(np.asarray(R).shape[0])
    source = [int(s) for s in np.asarray(source).reshape(-1).tolist()]
    pr = _project(points, [s + k_first for s in source], R, t, K_T, np.asarray(depth_all), dtype)
    depth_all, img_all = torch.as_tensor(depth_all).to(dtype), torch.as_tensor(img_all).to(dtype)
    xx, yy = S._pixel_grid(H, W)
    xx, yy = xx.to(dtype), yy.to(dtype)
    maps = torch.full((T, B, 3, H, W), -1.0, dtype=dtype)
    occluded = torch.zeros(T, B, H, W, dtype=torch.bool)
    fragile = torch.zeros(T, B, H, W, dtype=torch.bool)
    front = torch.zeros(T, B, H, W, dtype=torch.bool)
    for r in range(T):
        for b in range(B):
            if not bool(pr['live'][r, b]):
                continue
            g = source[b] + k_first + r
            u, v, z, d, inside = pr['uv'][r, b, ..., 0], pr['uv'][r, b, ..., 1], pr['z'][r, b], pr['depth_at'][r, b], pr['inside'][r, b]
            front[r, b] = z > 0
            occ = inside & (z > d * (1 + z_tol))
            seen = inside & ~occ
            occluded[r, b] = occ
            rel = ((z - d).abs() / d.clamp(min=d_min)).clamp(max=1.0)
            l1 = torch.zeros(H, W, dtype=dtype)
            for ch in range(3):
                l1 = l1 + (S.sample_border(img_all[g, ch], u, v) - img_all[source[b], ch]).abs()
            photo = (l1 / 3).clamp(max=CAP)
            minus = torch.full((H, W), -1.0, dtype=dtype)
            maps[r, b, 0] = torch.where(seen, torch.nan_to_num(rel, nan=1.0), minus)
            maps[r, b, 1] = torch.where(seen, torch.nan_to_num(photo, nan=CAP), minus)
            if pairs is not None and int(pairs[0][r][b]) >= 0:
                row = int(pairs[0][r][b])
                flow = torch.as_tensor(pairs[1][row]).to(dtype)
                ok = (torch.as_tensor(pairs[2][row]) == 0) & front[r, b]
                epe = torch.hypot((u - xx) - flow[..., 0], (v - yy) - flow[..., 1]).clamp(max=CAP)
                maps[r, b, 2] = torch.where(ok, torch.nan_to_num(epe, nan=CAP), minus)
            edge, absz = S.edge_distance(pr['uv'][r, b].double(), z.double(), H, W)
            fragile[r, b] = (edge < 1e-3) | (absz < 1e-4) | ((z - d * (1 + z_tol)).abs().double() < 1e-4 * d.double())
    shift = shift_for(H * W)
    sums = [[row_sums(maps[r, b], pr['inside'][r, b], occluded[r, b], shift) for b in range(B)] for r in range(T)]
    return {'maps': maps, 'sums': sums, 'shift': shift, 'fragile': fragile, 'inside': pr['inside'], 'occluded': occluded,
            'front': front, 'live': pr['live'], 'uv': pr['uv'], 'z': pr['z'], 'depth_at': pr['depth_at'],
            'n_fragile': [[int(fragile[r, b].sum()) for b in range(B)] for r in range(T)]}


def quantise(x, shift):
    """round(x * 2^shift), half to even, summed -> an exact Python integer.  x: the counted values of one map."""
    x = torch.as_tensor(x).double().reshape(-1)
    return int((x * float(2 ** shift)).round().to(torch.int64).sum()) if x.numel() else 0


def row_sums(maps, inside, occluded, shift):
    """The six sums of one (step, image) from its three maps [3,H,W] and its inside / occluded flags."""
    rel, photo, epe = maps[0], maps[1], maps[2]
    return [int(inside.sum()), int(occluded.sum()), quantise(rel[rel >= 0], shift), quantise(photo[photo >= 0], shift),
            int((epe >= 0).sum()), quantise(epe[epe >= 0], shift)]


def fragile_share(res):
    """Fragile points among the points of the live rows."""
    live = res['live'][:, :, None, None].expand_as(res['fragile'])
    return float(res['fragile'][live].double().mean()) if bool(live.any()) else 0.0


# -- the inputs of tests/test_51_eval_kernel_gpu.py -----------------------------------------------------------------------------
# (H, W): PX = 1 one block | PX = 1 two blocks, the second partial | PX = 4 one block | PX = 4 two blocks, the second partial
KERNEL_SHAPES = ((11, 21), (17, 19), (12, 24), (36, 40))
KERNEL_SEED = {(11, 21): 3, (17, 19): 4, (12, 24): 5, (36, 40): 6}
KERNEL_T, KERNEL_N = 3, 5
KERNEL_SOURCE = (0, 1, 3)        # the rows of the last start frame run past the end of the 5 frames


def camera_tables(poses, K):
    """R (world -> camera as a right factor), R_T, t, K_T, K_inv_T of c2w poses [N,4,4] and intrinsics [N,3,3], fp32."""
    poses, K = np.asarray(poses, dtype=np.float32), np.asarray(K, dtype=np.float32)
    return {'R': poses[:, :3, :3].copy(), 'R_T': poses[:, :3, :3].transpose(0, 2, 1).copy(), 't': poses[:, :3, 3].copy(),
            'K_T': K.transpose(0, 2, 1).copy(), 'K_inv_T': np.linalg.inv(K).transpose(0, 2, 1).astype(np.float32).copy()}


def kernel_case(H, W, k_first, seed=None):
    """A seeded synthetic video of KERNEL_N frames (store_spec.random_tree: cameras, colours, flows, masks) with a smooth
    refined depth that has a step edge -- a near layer over the left part of every frame, which occludes what moves behind it --
    and KERNEL_T rows of world points per start frame: the start frame un-projected in float64 (tracks_spec.unproject), moved by
    a smooth motion per step, cast to fp32.  A few points are put behind the camera and a few far outside the image."""
    seed = KERNEL_SEED[(H, W)] if seed is None else seed
    N, T, source = KERNEL_N, KERNEL_T, list(KERNEL_SOURCE)
    tree = store_spec.random_tree(N, H, W, [1, 2], seed)
    rng = np.random.default_rng(seed + 100)
    tab = camera_tables(tree['fr_pose_c2w'], tree['fr_intrinsics'])
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    depth = np.zeros((N, 1, H, W), dtype=np.float32)
    for i in range(N):
        smooth = 3.0 + 0.4 * np.sin(0.3 * xx + 0.2 * i) + 0.3 * np.cos(0.25 * yy)
        depth[i, 0] = np.where(xx < W * (0.3 + 0.03 * i), 0.6 * smooth, smooth)
    # colours: a smooth pattern plus a little noise, so that neighbouring frames look alike
    img = np.zeros((N, 3, H, W), dtype=np.float32)
    for i in range(N):
        for ch in range(3):
            img[i, ch] = 0.5 + 0.4 * np.sin(0.2 * (ch + 1) * xx + 0.15 * yy + 0.1 * i) + 0.02 * tree['fr_img'][i, :, :, ch]
    B = len(source)
    p0 = S.unproject(depth[source], tab['R_T'][source], tab['t'][source], tab['K_inv_T'][source])      # [B,3,H,W] float64
    motion = torch.tensor([0.03, -0.01, 0.05], dtype=torch.float64).view(1, 3, 1, 1)
    wobble = torch.from_numpy(0.02 * np.sin(0.4 * xx + 0.3 * yy)).view(1, 1, H, W)
    # (k_first = 0, row 0 looks into the start frame itself: a little motion keeps its border pixels off the image edge)
    points = torch.stack([p0 + (k_first + r + 0.4) * (motion + wobble) for r in range(T)], 0)
    flat = points.view(T, B, 3, H * W)
    pick = rng.permutation(H * W)
    behind, far = pick[:max(2, H * W // 40)], pick[max(2, H * W // 40):2 * max(2, H * W // 40)]
    flat[:, :, 2, behind] -= 20.0                       # behind every camera
    flat[:, :, 0, far] += 40.0                          # in front, far to the right of every image
    pairs = [(a, a + g) for g in (1, 2) for a in range(N - g)]
    assert pairs == [tuple(p) for p in tree['fl_ids'].tolist()]
    rows = {p: j for j, p in enumerate(pairs)}
    pair_row = np.full((T, B), -1, dtype=np.int32)
    for r in range(T):
        for b, s in enumerate(source):
            if s + k_first + r < N:
                pair_row[r, b] = rows.get((s, s + k_first + r), -1)
    # flows near the displacement the points induce, so that epe is of the size it has after an optimisation
    flow = tree['fl_flow_1_2'] * 0.2
    return {'points': points.float().numpy(), 'source': np.array(source, dtype=np.int32), 'k_first': k_first, 'R': tab['R'],
            't': tab['t'], 'K_T': tab['K_T'], 'depth_all': depth, 'img_all': img, 'pair_row': pair_row,
            'flow_1_2': flow.astype(np.float32), 'mask': tree['fl_mask_2'].astype(np.uint8), 'N': N, 'T': T, 'B': B, 'H': H, 'W': W}


def run_case(case, with_pairs=True, dtype=torch.float64, **kw):
    pairs = (case['pair_row'], case['flow_1_2'], case['mask']) if with_pairs else None
    return evaluate(case['points'], case['source'], case['k_first'], case['R'], case['t'], case['K_T'], case['depth_all'],
                    case['img_all'], pairs=pairs, dtype=dtype, **kw)


# -- Model.evaluate on the store of tests/golden/tracks_b3_11x21_t4.npz (tests/test_52_evaluate_gpu.py) -------------------------
PIPE_FX = 'tracks_b3_11x21_t4'
PIPE_GAPS = (1, 2)
PIPE_TREE_SEED = 5


def pipeline_tree(fx):
    """The video tree of the store: store_spec.random_tree with flow files of gaps 1 and 2, the fixture's poses and
    intrinsics (so that the store's tables are the fixture's)."""
    tree = store_spec.random_tree(int(fx['N']), int(fx['H']), int(fx['W']), list(PIPE_GAPS), PIPE_TREE_SEED)
    tree['fr_pose_c2w'], tree['fr_intrinsics'] = fx['in_pose_c2w'], fx['in_intrinsics']
    return tree


def writer_pairs(n_frames, gaps):
    """The catalogue's pair list: the writer leaves out the last possible pair of every gap."""
    return [(f, f + g) for g in gaps for f in range(max(n_frames - 1 - g, 0))]


def pipeline_case(fx, sd, time_dependent=True):
    """The whole of Model.evaluate's chain in float64 from the fixture's inputs -> the arguments of `evaluate` (points are
    rows 1 .. n_steps of tracks_spec.integrate, float64)."""
    start, N, n_steps = fx['start'].tolist(), int(fx['N']), int(fx['n_steps'])
    B, H, W = len(start), int(fx['H']), int(fx['W'])
    tree = pipeline_tree(fx)
    ts = torch.from_numpy(fx['tab_ts_vali'])[start].view(B, 1, 1, 1).expand(B, 1, H, W) if time_dependent else None
    p0 = S.unproject(fx['in_depth'][start], fx['tab_R_T'][start], fx['tab_t'][start], fx['tab_K_inv_T'][start])
    valid = [min(n_steps, N - 1 - s) for s in start]
    pts = S.integrate(sd, p0, ts, 1.0 / N, valid, n_steps, 1.0 / 100.0)
    pairs = writer_pairs(N, PIPE_GAPS)
    file_rows = {tuple(p): j for j, p in enumerate(tree['fl_ids'].tolist())}
    keep = [file_rows[p] for p in pairs]
    rows = {p: j for j, p in enumerate(pairs)}
    pair_row = np.full((n_steps, B), -1, dtype=np.int32)
    for b, s in enumerate(start):
        for k in range(1, valid[b] + 1):
            pair_row[k - 1, b] = rows.get((s, s + k), -1)
    return {'points': pts[1:], 'source': np.array(start, dtype=np.int32), 'k_first': 1, 'R': fx['tab_R'], 't': fx['tab_t'],
            'K_T': fx['tab_K_T'], 'depth_all': fx['in_depth'], 'img_all': np.ascontiguousarray(tree['fr_img'].transpose(0, 3, 1, 2)),
            'pair_row': pair_row, 'flow_1_2': tree['fl_flow_1_2'][keep], 'mask': tree['fl_mask_2'][keep], 'steps_valid': valid}
