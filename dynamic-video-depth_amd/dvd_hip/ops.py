"""Tensor-level wrappers over the C ABI (include/dvd_hip.h).

These functions only validate, allocate outputs with torch (so the caching
allocator owns every buffer) and enqueue the HIP kernels on torch's current
stream.  They never touch tensor contents on the host and never fall back to
PyTorch arithmetic: a tensor that is not on a GPU is an error.
"""
import ctypes
import os
import sys

import numpy as np
import torch

from . import _lib

CAM_KEYS = ('R_1', 'R_2', 'R_1_T', 'R_2_T', 't_1', 't_2', 'K', 'K_inv')


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev32(t, name):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError('%s must be a GPU tensor (dvd_hip has no CPU path)' % name)
    if t.dtype != torch.float32:
        raise RuntimeError('%s must be float32, got %s' % (name, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


# -- the checks the post-processing wrappers share: one copy each.  They run on the host and read nothing back -------------
def _dev_u8(what, name, t, shape, dev, copy=True):
    """None, or a GPU uint8 tensor of `shape` on `dev`; one that is not contiguous is copied, or refused where not `copy`."""
    if t is None:
        return None
    if not (torch.is_tensor(t) and t.is_cuda and t.device == dev and t.dtype == torch.uint8 and tuple(t.shape) == tuple(shape)
            and (copy or t.is_contiguous())):
        raise RuntimeError('%s: %s must be a %sGPU uint8 tensor %s on the device of the data' % (
            what, name, '' if copy else 'contiguous ', list(shape)))
    return t if t.is_contiguous() else t.contiguous()


def _out_ok(what, name, t, shape, dtype, dev, on):
    """A tensor the kernel writes (or reads in place): it must be exactly this already, nothing is converted or copied."""
    if not (torch.is_tensor(t) and t.device == dev and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous()):
        raise RuntimeError('%s: %s must be a contiguous %s tensor %s on the device of %s' % (what, name, dtype, list(shape), on))
    return t


def _outputs(what, out, shapes, dev, on):
    """{name: (shape, dtype)} -> {name: tensor}: out[name] where the caller preallocated it, a new tensor otherwise."""
    res = {}
    for k, (shape, dtype) in shapes.items():
        o = out.get(k) if out is not None else None
        res[k] = torch.empty(shape, device=dev, dtype=dtype) if o is None else _out_ok(what, 'out[%r]' % k, o, shape, dtype, dev, on)
    return res


def _int_arg(what, name, v, lo, hi, floats=True):
    """v as an int in lo .. hi: anything but a bool whose int(v) equals it (an integral float only where `floats` allows it)."""
    ok = type(v) is int
    if not ok:                                                        # (a plain int skips all this)
        try:
            ok = not isinstance(v, (bool, np.bool_)) and (floats or not isinstance(v, (float, np.floating))) and bool(int(v) == v)
        except (TypeError, ValueError, OverflowError):                # not a number; a NaN; an Inf
            ok = False
    if not (ok and lo <= v <= hi):
        raise RuntimeError('%s: %s must be an integer in %d .. %d, got %r' % (what, name, lo, hi, v))
    return int(v)


_FLT_MAX = 3.4028234663852886e+38


def _real_arg(what, name, v, lo=0.0, lo_open=False, hi=None):
    """v as a float: a number (no bool) that is finite -- as float32 too, which is what the kernel receives -- and lies in
    [lo, hi], (lo, hi] where lo_open; hi None: no upper end."""
    ok = type(v) is float
    if not ok:                                                        # (a plain float skips all this)
        ok = isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)
    if not (ok and -_FLT_MAX <= v <= _FLT_MAX and (v > lo if lo_open else v >= lo) and (hi is None or v <= hi)):   # (no NaN passes)
        raise RuntimeError('%s: %s must be a finite number %s, got %r' % (
            what, name, ('> %g' if lo_open else '>= %g') % lo if hi is None else 'in %s%g, %g]' % ('(' if lo_open else '[', lo, hi), v))
    return float(v)


def _ids_in(what, name, host, lo, hi):
    if host.size and (int(host.min()) < lo or int(host.max()) >= hi):
        raise RuntimeError('%s: the ids of %s span [%d, %d], outside %d .. %d' % (what, name, int(host.min()), int(host.max()), lo, hi - 1))


def _host_ids(what, name, ids, shape, lo=None, hi=None, floats=True):
    """A host sequence / array / CPU tensor of ids -> an integer numpy array of exactly `shape` (None: any extent), every id in
    lo .. hi - 1 (no range check without lo).  An array of integral floats is taken where `floats` allows it."""
    try:
        host = np.asarray(ids.cpu() if torch.is_tensor(ids) else ids)
    except (TypeError, ValueError):
        raise RuntimeError('%s: %s must be a host array of integers' % (what, name))
    if floats and host.dtype.kind == 'f' and host.size and np.all(np.isfinite(host)) and np.all(host == np.floor(host)):
        host = host.astype(np.int64)
    if host.dtype.kind not in 'iu' or (host.shape != tuple(shape) and (host.ndim != len(shape) or any(
            s is not None and s != h for s, h in zip(shape, host.shape)))):
        raise RuntimeError('%s: %s must hold [%s] integral ids, got %s %s' % (
            what, name, ', '.join('any' if s is None else str(s) for s in shape), host.dtype, host.shape))
    if lo is not None:
        _ids_in(what, name, host, lo, hi)
    return host


def _ids(what, name, ids, shape, lo, hi, dev, on, host=None, read_back=False, floats=True, non_blocking=True):
    """Ids for a kernel -> (contiguous int32 tensor on dev, their checked host copy or None).  `ids` is a host sequence / array
    / CPU tensor (checked by _host_ids, uploaded here) or a GPU int32 tensor; the latter is range-checked from `host`, its host
    copy, where the caller has one, is read back where read_back asks for it, and is otherwise taken as it is."""
    if torch.is_tensor(ids) and ids.is_cuda:
        if ids.dtype != torch.int32 or tuple(ids.shape) != tuple(shape) or not ids.is_contiguous() or ids.device != dev:
            raise RuntimeError('%s: %s must be a contiguous GPU int32 tensor %s of ids on the device of %s' % (what, name, list(shape), on))
        if host is None and read_back:
            host = ids.cpu()
        return ids, (None if host is None else _host_ids(what, name, host, shape, lo, hi, floats))
    host = _host_ids(what, name, ids, shape, lo, hi, floats)
    return torch.from_numpy(np.ascontiguousarray(host.astype(np.int32))).to(dev, non_blocking=non_blocking), host


def _tables(what, tables, keys, per, dev, on, n=None):
    """The per-frame camera tables `keys` of a dict -> (the tensors, their number of rows n).  Each is float32 on dev and holds
    per[i] values for each of n rows; n None: as many as the first table has."""
    tabs = []
    for k in keys:
        if k not in tables:
            raise RuntimeError('%s: tables must hold %s' % (what, ', '.join(keys)))
        tab = _dev32(tables[k], 'table ' + k)
        if tab.device != dev:
            raise RuntimeError('%s: table %s and %s are on different devices' % (what, k, on))
        tabs.append(tab)
    if n is None:
        n = int(tabs[0].shape[0]) if tabs[0].dim() > 0 else 0
    for k, tab, p in zip(keys, tabs, per):
        if n <= 0 or tab.dim() < 2 or tab.shape[0] != n or tab.numel() != n * p:
            raise RuntimeError('%s: table %s must hold %d values for each of %d rows, got %s' % (what, k, p, n, tuple(tab.shape)))
    return tabs, n


def _depth_all(what, depth_all, N, H, W, dev):
    depth_all = _dev32(depth_all, 'depth_all')
    if depth_all.device != dev or depth_all.numel() != N * H * W or depth_all.shape[0] != N:
        raise RuntimeError('%s: depth_all must be [%d,1,%d,%d] on the device of the points, got %s' % (
            what, N, H, W, tuple(depth_all.shape)))
    return depth_all


def _point_slab(what, p):
    """p [B,3,H,W]: the contiguous float32 GPU points of the inverse step."""
    if not (torch.is_tensor(p) and p.is_cuda):
        raise RuntimeError('p must be a GPU tensor (dvd_hip has no CPU path)')
    if p.dtype != torch.float32 or p.dim() != 4 or p.shape[1] != 3 or p.numel() == 0 or not p.is_contiguous():
        raise RuntimeError('%s: p must be a contiguous float32 tensor [B,3,H,W], got %s %s' % (what, p.dtype, tuple(p.shape)))
    return p


def _shape_is(what, name, t, shapes):
    """t is a tensor of one of `shapes`; a RuntimeError that names it otherwise.  Host arithmetic only: it holds for a tensor
    anywhere, so it comes before the device checks and a test needs no GPU for it."""
    if not torch.is_tensor(t) or tuple(t.shape) not in shapes:
        raise RuntimeError('%s: %s must be a tensor %s, got %s' % (
            what, name, ' or '.join(str(list(sh)) for sh in shapes), tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
    return t


def _images(what, specs, dev=None):
    """'These tensors are all [B,...,H,W] of this call': specs of (name, tensor or None, shapes) -> the tensors as contiguous
    float32 GPU tensors, all on one device (`dev`, or that of the first).  Every shape is checked before any device or dtype,
    and all of it before anything is launched; a None stays None."""
    for name, t, shapes in specs:
        if t is not None:
            _shape_is(what, name, t, shapes)
    res = []
    for name, t, _ in specs:
        if t is not None:
            t = _dev32(t, '%s: %s' % (what, name))
            if dev is None:
                dev = t.device
            elif t.device != dev:
                raise RuntimeError('%s: %s is on %s, the other tensors are on %s' % (what, name, t.device, dev))
        res.append(t)
    return res


def _image_size(what, name, t):
    """(B, H, W) of the [B,1,H,W] tensor that fixes them for a call."""
    if not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] != 1 or t.numel() == 0:
        raise RuntimeError('%s: %s must be a tensor [B,1,H,W], got %s' % (
            what, name, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
    return int(t.shape[0]), int(t.shape[2]), int(t.shape[3])


def _camera_shapes(B, per):
    return ((B, 1, 1, 3, 3), (B, 3, 3), (B, 9)) if per == 9 else ((B, 1, 1, 1, 3), (B, 3))


def _camera_specs(what, cams, B):
    """The eight camera tensors as specs for _images: each [B,1,1,3,3] / [B,1,1,1,3] or flat, for exactly B images."""
    for k in CAM_KEYS:
        if k not in cams:
            raise RuntimeError('%s: cams must hold %s' % (what, ', '.join(CAM_KEYS)))
    return [(k, cams[k], _camera_shapes(B, 3 if k.startswith('t_') else 9)) for k in CAM_KEYS]


def _camera_struct(tensors):
    st = _lib.Cameras()
    for k, t in zip(CAM_KEYS, tensors):
        setattr(st, k, t.data_ptr())
    return st


def pack_cameras(cams, B=None, what='pack_cameras', dev=None):
    """dict of the eight camera tensors ([B,1,1,3,3] / [B,1,1,1,3] or flat: [B,3,3], [B,9] / [B,3])
    -> (ctypes struct, list of tensors kept alive).  With B, each must be one of these shapes for exactly B images, on `dev`
    where that is given."""
    if B is not None:
        keep = _images(what, _camera_specs(what, cams, B), dev)
    else:
        keep = [_dev32(cams[k], k) for k in CAM_KEYS]
    return _camera_struct(keep), keep


def warp_cfg(B, H, W, midas_mask=True, crit_l2=False, disp_mode=1, loss_on_sf=False, flow_mul=1.0, disp_mul=1.0):
    return _lib.WarpCfg(int(B), int(H), int(W), int(bool(midas_mask)), int(bool(crit_l2)), int(disp_mode),
                        int(bool(loss_on_sf)), float(flow_mul), float(disp_mul))


def unproject(depth, R, t, K_inv, planar=True, out=None):
    """depth [B,1,H,W] -> world points, [B,3,H,W] (planar) or [B,H,W,1,3]; out: optional destination of that shape."""
    B, H, W = _image_size('unproject', 'depth', depth)
    depth, R, t, K_inv = _images('unproject', [('depth', depth, ((B, 1, H, W),)), ('R', R, _camera_shapes(B, 9)),
                                               ('t', t, _camera_shapes(B, 3)), ('K_inv', K_inv, _camera_shapes(B, 9))])
    shape = (B, 3, H, W) if planar else (B, H, W, 1, 3)
    if out is None:
        out = torch.empty(shape, device=depth.device, dtype=torch.float32)
    else:
        _out_ok('unproject', 'out', out, shape, torch.float32, depth.device, 'the depth')
    lib = _lib.load()
    _lib.check(lib.dvd_unproject_fwd(_p(depth), _p(R), _p(t), _p(K_inv), _p(out), int(planar), B, H, W, _stream()),
               'dvd_unproject_fwd')
    return out


def unproject_backward(g_points, planar, R, K_inv, scale=None, out=None, accumulate=False):
    """g_depth (+)= scale * ((g_points @ R^T) . ray);  scale: 1-element GPU tensor or None."""
    what = 'unproject_backward'
    if not torch.is_tensor(g_points) or g_points.dim() < 4 or g_points.numel() == 0:
        raise RuntimeError('%s: g_points must be a tensor [B,3,H,W] (planar) or [B,H,W,3] / [B,H,W,1,3], got %s' % (
            what, tuple(g_points.shape) if torch.is_tensor(g_points) else type(g_points).__name__))
    if planar:
        B, H, W = int(g_points.shape[0]), int(g_points.shape[2]), int(g_points.shape[3])
    else:
        B, H, W = (int(v) for v in g_points.shape[:3])
    g_points, R, K_inv, scale = _images(what, [
        ('g_points', g_points, ((B, 3, H, W),) if planar else ((B, H, W, 3), (B, H, W, 1, 3))),
        ('R', R, _camera_shapes(B, 9)), ('K_inv', K_inv, _camera_shapes(B, 9)), ('scale', scale, ((1,), ()))])
    if out is None:
        if accumulate:
            raise RuntimeError('accumulate=True needs an output tensor')
        out = torch.empty((B, 1, H, W), device=g_points.device, dtype=torch.float32)
    else:       # written in place: it is exactly this already, or refused (a copy would take the result with it)
        _out_ok(what, 'out', out, (B, 1, H, W), torch.float32, g_points.device, 'g_points')
    lib = _lib.load()
    _lib.check(lib.dvd_unproject_bwd(_p(g_points), int(planar), _p(R), _p(K_inv), _p(scale), _p(out),
                                     int(bool(accumulate)), B, H, W, _stream()), 'dvd_unproject_bwd')
    return out


TRACK_TABLES = ('R', 't', 'K_T')


def _track_args(what, points, start, tables, planar, host_start):
    """Everything track_project and project_backward check before a launch -> (points, start on the device, the three tables,
    T1, B, H, W, N).  Runs on the host; a CPU tensor is refused before any shape is looked at."""
    points = _dev32(points, 'points')
    if points.dim() != 5 or points.shape[2 if planar else 4] != 3 or points.numel() == 0:
        raise RuntimeError('%s: points must be [T1,B,3,H,W] (planar) or [T1,B,H,W,3], got %s' % (what, tuple(points.shape)))
    T1, B = int(points.shape[0]), int(points.shape[1])
    H, W = (int(v) for v in (points.shape[3:5] if planar else points.shape[2:4]))
    if H < 2 or W < 2:
        raise RuntimeError('%s: images of %d x %d; the sampling rule needs H, W >= 2' % (what, H, W))
    if T1 > 65535 or B > 65535:
        raise RuntimeError('%s: at most 65535 steps and 65535 images per launch, got %d and %d' % (what, T1, B))
    tabs, N = _tables(what, tables, TRACK_TABLES, (9, 3, 9), points.device, 'the points')
    # (a device tensor without its host copy is read back: the range check needs the ids)
    start, _ = _ids(what, 'start', start, (B,), 0, N, points.device, 'the points', host=host_start, read_back=True,
                    non_blocking=False)
    return points, start, tabs, T1, B, H, W, N


def track_project(points, start, tables, depth_all=None, out=None, planar=True, displacement=False, host_start=None,
                  want=('z', 'inside'), k0=0):
    """World points into the cameras of frames start[b] + k (dvd_track_project, csrc/track.hip) -> dict of uv [T1,B,H,W,2], z
    [T1,B,H,W], inside uint8 [T1,B,H,W] and, with depth_all [N,1,H,W], depth_at [T1,B,H,W].
      points   [T1,B,3,H,W] (planar: a slab of the scene-flow MLP's p_next rows) or [T1,B,H,W,3]
      start    B frame ids: a host sequence / array / CPU tensor (uploaded here) or a GPU int32 tensor, then host_start, its
               host copy, saves the read-back the range check needs otherwise
      tables   {'R': [N,3,3] world->camera, 't': [N,3], 'K_T': [N,3,3]} -- FrameStore.tables has them under these names
      out      optional dict of preallocated outputs;  want: which of the optional 'z' / 'inside' to compute
      displacement  uv minus the pixel's own (x, y): project_ptcld's return value
      k0       row offset: row k looks up frame start[b] + k + k0 (dvd_track_project_from; -n_back for a two-sided slab whose
               row n_back is the start frame); frames before the video give zeros like frames past its end
    Frames past the end of the tables give zeros.  Everything is checked on the host before the launch."""
    what = 'track_project'
    k0 = _int_arg(what, 'k0', k0, 1 - (1 << 30), (1 << 30) - 1)
    points, start, (R, t, K_T), T1, B, H, W, N = _track_args(what, points, start, tables, planar, host_start)
    if depth_all is not None:
        depth_all = _depth_all(what, depth_all, N, H, W, points.device)
    shapes = {'uv': ((T1, B, H, W, 2), torch.float32)}
    if 'z' in want:
        shapes['z'] = ((T1, B, H, W), torch.float32)
    if 'inside' in want:
        shapes['inside'] = ((T1, B, H, W), torch.uint8)
    if depth_all is not None:
        shapes['depth_at'] = ((T1, B, H, W), torch.float32)
    res = _outputs(what, out, shapes, points.device, 'the points')
    args = (_p(points), int(bool(planar)), _p(start), _p(R), _p(t), _p(K_T), _p(depth_all), N, _p(res['uv']),
            int(bool(displacement)), _p(res.get('z')), _p(res.get('depth_at')), _p(res.get('inside')), T1, B, H, W)
    if k0 != 0:
        _lib.check(_lib.load().dvd_track_project_from(*(args + (k0, _stream()))), 'dvd_track_project_from')
    else:
        _lib.check(_lib.load().dvd_track_project(*(args + (_stream(),))), 'dvd_track_project')
    return res


FILTER_MAX_ROWS = 33        # kFilterMaxRows of csrc/track_filter.hip: a window of at most 16 frames on either side
FILTER_MODES = {'mean': 0, 'median': 1}


def track_filter(points, start, tables, depth_all, weights, k0=0, mode='mean', tol=0.1, z_near=1e-3, planar=True, out=None,
                 host_start=None, want=('ratio', 'count', 'spread')):
    """Every pixel's depth fused along its own track (dvd_track_filter, csrc/track_filter.hip) -> dict of depth [B,1,H,W] and,
    as `want` names them, ratio [B,1,H,W], count uint8 [B,H,W], spread [B,1,H,W].
      points, start, tables, depth_all, k0, planar, host_start   as track_project takes them; row -k0 of the slab is the start
               frame itself and must be one of its T1 <= 33 rows; depth_all [N,1,H,W] is required
      weights  a host sequence of T1 finite values >= 0 with weights[-k0] > 0 (uploaded here); not used by the median
      mode     'mean': the weighted mean of the counting rows' ratios D / z;  'median': their median
      tol      a row counts where z <= D (1 + tol) and D <= z (1 + tol) (and the point is inside, z >= z_near, D > 0)
      out      optional dict of preallocated outputs
    depth = depth_all[start] * ratio; a pixel whose own depth is not > 0 keeps it (ratio 1, count 0, spread 0).  Everything
    is checked on the host before the launch."""
    import numpy as np
    what = 'track_filter'
    k0 = _int_arg(what, 'k0', k0, 1 - (1 << 30), (1 << 30) - 1)
    if mode not in FILTER_MODES:
        raise RuntimeError('%s: mode must be one of %s, got %r' % (what, ', '.join(sorted(FILTER_MODES)), mode))
    tol, z_near = _real_arg(what, 'tol', tol), _real_arg(what, 'z_near', z_near)
    if any(k not in ('ratio', 'count', 'spread') for k in want):
        raise RuntimeError("%s: want may name 'ratio', 'count' and 'spread', got %r" % (what, tuple(want)))
    # the weights first: they are host data, so a bad list is refused before a tensor is looked at
    try:
        w = np.asarray(weights.cpu() if torch.is_tensor(weights) else weights, dtype=np.float64)
    except (TypeError, ValueError):
        raise RuntimeError('%s: weights must be a sequence of numbers, got %r' % (what, weights))
    if w.ndim != 1 or not 1 <= w.size <= FILTER_MAX_ROWS:
        raise RuntimeError('%s: weights must hold one value per row, 1 .. %d of them, got shape %s' % (what, FILTER_MAX_ROWS, w.shape))
    with np.errstate(over='ignore'):
        w32 = w.astype(np.float32)
    if not np.all(np.isfinite(w32)) or np.any(w < 0):              # (a NaN stays one; a value past fp32's range turns Inf)
        raise RuntimeError('%s: weights must be finite values >= 0, got %r' % (what, weights))
    if not 0 <= -k0 < w.size:
        raise RuntimeError('%s: k0=%d puts the start frame in row %d, outside the %d rows of the weights' % (what, k0, -k0, w.size))
    w = np.ascontiguousarray(w32)
    if not w[-k0] > 0:
        raise RuntimeError("%s: the start frame's own weight, weights[%d], must be > 0, got %r" % (what, -k0, float(w[-k0])))
    points, start, (R, t, K_T), T1, B, H, W, N = _track_args(what, points, start, tables, planar, host_start)
    dev = points.device
    if T1 != w.size:
        raise RuntimeError('%s: %d weights for a slab of %d rows (at most %d)' % (what, w.size, T1, FILTER_MAX_ROWS))
    if depth_all is None:
        raise RuntimeError('%s: depth_all is required' % what)
    depth_all = _depth_all(what, depth_all, N, H, W, dev)
    wdev = torch.from_numpy(w).to(dev)
    shapes = {'depth': ((B, 1, H, W), torch.float32)}
    for k in ('ratio', 'count', 'spread'):
        if k in want:
            shapes[k] = ((B, H, W), torch.uint8) if k == 'count' else ((B, 1, H, W), torch.float32)
    res = _outputs(what, out, shapes, dev, 'the points')
    _lib.check(_lib.load().dvd_track_filter(
        _p(points), int(bool(planar)), _p(start), _p(R), _p(t), _p(K_T), _p(depth_all), N, _p(wdev), FILTER_MODES[mode],
        tol, z_near, _p(res['depth']), _p(res.get('ratio')), _p(res.get('count')), _p(res.get('spread')),
        T1, B, H, W, k0, _stream()), 'dvd_track_filter')
    return res


TRI_MAX_OBS = 32            # kTriMaxObs of csrc/triangulate.hip
TRI_TABLES = ('R', 't', 'K_T', 'K_inv_T')
TRI_SIN2_MIN = 7.615242e-05  # sin^2 of 0.5 degrees
TRI_OUT = (('depth', torch.float32, True), ('count', torch.uint8, False), ('usable', torch.uint8, False),
           ('epi', torch.float32, True), ('spread', torch.float32, True))


def triangulate(flow_1_2, flow_2_1, mask_1, mask_2, obs, frames, tables, mode='median', epi_tol=1.0, sin2_min=TRI_SIN2_MIN,
                z_near=1e-3, min_count=2, out=None):
    """Depth triangulated from stored flow and cameras, fused per pixel over a frame's observations (dvd_triangulate,
    csrc/triangulate.hip) -> dict of depth, epi, spread [B,1,H,W] fp32 and count, usable [B,H,W] uint8.
      flow_1_2, flow_2_1   [P,H,W,2] fp32;  mask_1, mask_2  [P,H,W] uint8, 0 = valid  (a FrameStore's tensors)
      obs      [B,M,3] integral rows (pair, other frame, dir), M <= 32, pair = -1 padding: a host array / sequence / CPU tensor
               (preprocess.triangulate_plan builds it; uploaded here).  dir 0 reads flow_1_2 with mask_2, dir 1 flow_2_1 with mask_1
      frames   B query frame ids on the host
      tables   {'R': [N,3,3] camera to world, 't': [N,3], 'K_T': [N,3,3], 'K_inv_T': [N,3,3]} -- FrameStore.tables has them
      mode     'mean' (weights sin2) or 'median' of the consistent observations' depth
      epi_tol  px; sin2_min in (0, 1]: the least squared sine of the parallax angle; z_near; min_count in 1 .. 255
      out      optional dict of preallocated outputs
    include/dvd_hip.h has the formulae and the gates.  Everything is checked on the host before the launch, and nothing
    synchronises with the device."""
    import numpy as np
    what = 'triangulate'
    if mode not in FILTER_MODES:
        raise RuntimeError('%s: mode must be one of %s, got %r' % (what, ', '.join(sorted(FILTER_MODES)), mode))
    epi_tol, z_near = _real_arg(what, 'epi_tol', epi_tol), _real_arg(what, 'z_near', z_near)
    sin2_min = _real_arg(what, 'sin2_min', sin2_min, lo_open=True, hi=1.0)
    min_count = _int_arg(what, 'min_count', min_count, 1, 255, floats=False)
    # the host data first: a bad table is refused before a tensor is looked at
    fr = _host_ids(what, 'frames', frames, (None,), floats=False)
    B = int(fr.size)
    if not 1 <= B <= 65535:
        raise RuntimeError('%s: frames must hold 1 .. 65535 frame ids per launch, got %d' % (what, B))
    try:
        o = np.asarray(obs.cpu() if torch.is_tensor(obs) else obs)
    except (TypeError, ValueError):
        raise RuntimeError('%s: obs must be a host array of integers' % what)
    if o.size == 0 and o.ndim <= 3:                                   # (no observations, in whatever empty form)
        o = np.zeros((B, 0, 3), np.int32)
    o = _host_ids(what, 'obs (rows of pair, frame, dir)', o, (B, None, 3), floats=False)
    M = int(o.shape[1])
    if M > TRI_MAX_OBS:
        raise RuntimeError('%s: obs holds M=%d observations per frame, at most %d' % (what, M, TRI_MAX_OBS))
    f12 = _dev32(flow_1_2, 'flow_1_2')
    dev = f12.device
    if f12 is not flow_1_2 or f12.dim() != 4 or f12.shape[3] != 2 or f12.shape[1] < 1 or f12.shape[2] < 1:
        raise RuntimeError('%s: flow_1_2 must be contiguous [P,H,W,2], got %s' % (what, tuple(f12.shape)))
    P, H, W = (int(v) for v in f12.shape[:3])
    if H * W >= 1 << 30:
        raise RuntimeError('%s: images of %d x %d: H * W must stay below 2^30' % (what, H, W))
    _out_ok(what, 'flow_2_1', flow_2_1, f12.shape, torch.float32, dev, 'flow_1_2')
    if mask_1 is None or mask_2 is None:
        raise RuntimeError('%s: mask_1 and mask_2 are required, got None for %s' % (what, 'mask_1' if mask_1 is None else 'mask_2'))
    mask_1 = _dev_u8(what, 'mask_1', mask_1, (P, H, W), dev, copy=False)
    mask_2 = _dev_u8(what, 'mask_2', mask_2, (P, H, W), dev, copy=False)
    tabs, N = _tables(what, tables, TRI_TABLES, (9, 3, 9, 9), dev, 'the flows')
    _ids_in(what, 'frames', fr, 0, N)
    live = o[..., 0] >= 0
    if M:
        if int(o[..., 0].min()) < -1 or int(o[..., 0].max()) >= P:
            raise RuntimeError('%s: obs names pairs in [%d, %d], outside -1 (padding) .. %d' % (
                what, int(o[..., 0].min()), int(o[..., 0].max()), P - 1))
        if live.any() and (int(o[..., 1][live].min()) < 0 or int(o[..., 1][live].max()) >= N):
            raise RuntimeError('%s: obs names frames in [%d, %d], outside the %d frames of the tables' % (
                what, int(o[..., 1][live].min()), int(o[..., 1][live].max()), N))
        if live.any() and not np.isin(o[..., 2][live], (0, 1)).all():
            raise RuntimeError('%s: the dir column of obs must be 0 (flow_1_2) or 1 (flow_2_1)' % what)
    res = _outputs(what, out, {k: ((B, 1, H, W) if chan else (B, H, W), dtype) for k, dtype, chan in TRI_OUT}, dev, 'the flows')
    # the frame ids and the table in ONE upload from pinned memory, enqueued on the current stream: a copy from pageable memory
    # would make the host wait for the stream
    host = torch.from_numpy(np.concatenate([fr.astype(np.int32), o.astype(np.int32).ravel()])).pin_memory()
    both = host.to(dev, non_blocking=True)
    fr_dev, obs_dev = both[:B], (both[B:] if M else None)
    _lib.check(_lib.load().dvd_triangulate(
        _p(f12), _p(flow_2_1), _p(mask_1), _p(mask_2), P, _p(obs_dev), _p(fr_dev), int(live.sum()), _p(tabs[0]), _p(tabs[1]),
        _p(tabs[2]), _p(tabs[3]), N, FILTER_MODES[mode], epi_tol, sin2_min, z_near, min_count,
        _p(res['depth']), _p(res['count']), _p(res['usable']), _p(res['epi']), _p(res['spread']), M, B, H, W, _stream()),
        'dvd_triangulate')
    return res


POSE_SUMS = 106             # kPoseSums of csrc/pose.hip: 91 of J^T w J + 13 of J^T w r + the cost + sum w |r|^2
POSE_MAX_ROWS = 65535


def pose_penalty(H, W, huber):
    """What an observation that a step pushed behind its camera costs per unit weight: Huber's rho of a residual as long as the
    image's diagonal, huber * (hypot(W, H) - huber / 2) (the square's half should huber exceed the diagonal), as float32."""
    h, far = float(np.float32(huber)), float(np.hypot(float(W), float(H)))
    return float(np.float32(h * (far - h / 2) if far > h else far * far / 2))


def pose_normal_eq(flow_1_2, flow_2_1, mask_1, mask_2, depth, weight, rows, tables, log_scale, huber, z_near, maps=False, out=None):
    """The normal equations of the camera refinement, reduced per observation row (dvd_pose_normal_eq, csrc/pose.hip) -> dict of
    sums float64 [R,106], wsum float64 [R], counts int64 [R,2] and, with `maps`, resid fp32 [R,H,W,2] and gate uint8 [R,H,W].
      flow_1_2, flow_2_1   [P,H,W,2] fp32;  mask_1, mask_2  [P,H,W] uint8, 0 = valid  (a FrameStore's tensors)
      depth      [N,1,H,W] (or [N,H,W]) fp32 planar depth per frame;  weight  [N,H,W] fp32 or None (all ones)
      rows       [R,4] integral rows (pair, a, b, dir), 1 <= R <= 65535: a host array / sequence / CPU tensor
                 (preprocess.refine_plan builds it; uploaded here).  dir 0 reads flow_1_2 with mask_2, dir 1 flow_2_1 with mask_1.
                 A row whose pair is outside 0 .. P-1 or whose frames are outside 0 .. N-1 is skipped: zeros
      tables     {'R': [N,3,3] camera to world, 't': [N,3], 'K_T': [N,3,3], 'K_inv_T': [N,3,3]} -- FrameStore.tables has them
      log_scale  N finite log depth scales on the host, or None (zeros); the kernel receives float32(exp(.))
      huber      px, > 0;  z_near > 0: an observation with q.z below it counts in counts[:, 1] and costs pose_penalty()
      out        optional dict of preallocated outputs
    sums[:, :91] is the upper triangle of J^T w J over the unknowns [tau_a, omega_a, sigma_a, tau_b, omega_b], sums[:, 91:104]
    J^T w r, sums[:, 104] the cost, sums[:, 105] sum w |r|^2; include/dvd_hip.h has the formulae and the gates.  Everything is
    checked on the host before the launch, and nothing synchronises with the device."""
    what = 'pose_normal_eq'
    huber = _real_arg(what, 'huber', huber, lo_open=True)
    z_near = _real_arg(what, 'z_near', z_near, lo_open=True)
    # the host data first: a bad table is refused before a tensor is looked at
    try:
        r = np.asarray(rows.cpu() if torch.is_tensor(rows) else rows)
    except (TypeError, ValueError):
        raise RuntimeError('%s: rows must be a host array of integers' % what)
    r = _host_ids(what, 'rows (pair, a, b, dir)', r, (None, 4), floats=False)
    R = int(r.shape[0])
    if not 1 <= R <= POSE_MAX_ROWS:
        raise RuntimeError('%s: rows must hold 1 .. %d rows per launch, got %d' % (what, POSE_MAX_ROWS, R))
    if not np.isin(r[:, 3], (0, 1)).all():
        raise RuntimeError('%s: the dir column of rows must be 0 (flow_1_2) or 1 (flow_2_1)' % what)
    if np.abs(r).max() >= 1 << 31:
        raise RuntimeError('%s: rows holds an index beyond int32' % what)
    n_tab = int(tables['R'].shape[0]) if isinstance(tables, dict) and torch.is_tensor(tables.get('R')) and tables['R'].dim() else None
    if log_scale is not None:
        try:
            ls = np.asarray(log_scale.cpu() if torch.is_tensor(log_scale) else log_scale, dtype=np.float64)
        except (TypeError, ValueError):
            raise RuntimeError('%s: log_scale must be a host sequence of numbers, got %r' % (what, log_scale))
        with np.errstate(over='ignore'):
            sc = np.exp(ls).astype(np.float32)
        if ls.ndim != 1 or (n_tab is not None and ls.size != n_tab) or not np.all(np.isfinite(sc)) or not np.all(sc > 0):
            raise RuntimeError('%s: log_scale must hold one finite value per frame whose exp is a positive float32, got %r' % (what, log_scale))
    f12 = _dev32(flow_1_2, 'flow_1_2')
    dev = f12.device
    if f12 is not flow_1_2 or f12.dim() != 4 or f12.shape[3] != 2 or f12.shape[0] < 1 or f12.shape[1] < 1 or f12.shape[2] < 1:
        raise RuntimeError('%s: flow_1_2 must be contiguous [P,H,W,2], got %s' % (what, tuple(f12.shape)))
    P, H, W = (int(v) for v in f12.shape[:3])
    if H * W >= 1 << 30:
        raise RuntimeError('%s: images of %d x %d: H * W must stay below 2^30' % (what, H, W))
    _out_ok(what, 'flow_2_1', flow_2_1, f12.shape, torch.float32, dev, 'flow_1_2')
    if mask_1 is None or mask_2 is None:
        raise RuntimeError('%s: mask_1 and mask_2 are required, got None for %s' % (what, 'mask_1' if mask_1 is None else 'mask_2'))
    mask_1 = _dev_u8(what, 'mask_1', mask_1, (P, H, W), dev, copy=False)
    mask_2 = _dev_u8(what, 'mask_2', mask_2, (P, H, W), dev, copy=False)
    tabs, N = _tables(what, tables, TRI_TABLES, (9, 3, 9, 9), dev, 'the flows')
    if not (torch.is_tensor(depth) and depth.is_cuda and depth.device == dev and depth.dtype == torch.float32 and depth.is_contiguous()
            and tuple(depth.shape) in ((N, 1, H, W), (N, H, W))):
        raise RuntimeError('%s: depth must be a contiguous float32 GPU tensor [%d,1,%d,%d] on the device of the flows' % (what, N, H, W))
    if weight is not None:
        _out_ok(what, 'weight', weight, (N, H, W), torch.float32, dev, 'the flows')
    if log_scale is None:
        sc = np.ones(N, np.float32)
    elif sc.size != N:
        raise RuntimeError('%s: log_scale holds %d values for %d frames' % (what, sc.size, N))
    shapes = {'sums': ((R, POSE_SUMS), torch.float64), 'wsum': ((R,), torch.float64), 'counts': ((R, 2), torch.int64)}
    if maps:
        shapes.update(resid=((R, H, W, 2), torch.float32), gate=((R, H, W), torch.uint8))
    res = _outputs(what, out, shapes, dev, 'the flows')
    lib = _lib.load()
    ws_bytes = int(lib.dvd_pose_workspace_bytes(R, H, W))
    ws = torch.empty(ws_bytes // 8, device=dev, dtype=torch.float64)
    # the rows and the scales in ONE upload from pinned memory, enqueued on the current stream
    host = torch.from_numpy(np.concatenate([r.astype(np.int32).ravel(), sc.view(np.int32)])).pin_memory()
    both = host.to(dev, non_blocking=True)
    _lib.check(lib.dvd_pose_normal_eq(
        _p(f12), _p(flow_2_1), _p(mask_1), _p(mask_2), P, _p(depth), _p(weight), _p(tabs[0]), _p(tabs[1]), _p(tabs[2]), _p(tabs[3]),
        _p(both[4 * R:]), N, _p(both[:4 * R]), huber, z_near, pose_penalty(H, W, huber), _p(ws), ws_bytes, _p(res['sums']),
        _p(res['wsum']), _p(res['counts']), _p(res.get('resid')), _p(res.get('gate')), R, H, W, _stream()), 'dvd_pose_normal_eq')
    return res


CHAIN_MAX_LINKS = 32        # kChainMaxLinks of csrc/flow_chain.hip


def flow_chain(flow_1_2, flow_2_1, mask_1, mask_2, links, out=None):
    """Stored flows followed one after another (dvd_flow_chain, csrc/flow_chain.hip) -> {'flow': [L,B,H,W,2] fp32, 'broken':
    [L,B,H,W] uint8}: row k of chain b holds, per pixel x0, the position after links 0 .. k minus x0, and 0 while the chain is
    whole there, else 1 + the index of the link that broke (a position outside the image, a masked tap, a step that is not
    finite); the flow then stays at its last value.  Rows past a chain's end are 0 and 255.
      flow_1_2, flow_2_1   [P,H,W,2] fp32;  mask_1, mask_2  [P,H,W] uint8, 0 = valid  (a FrameStore's tensors)
      links    [B,L,2] integral rows (pair, dir), L <= 32, pair = -1 ends a chain: a host array / sequence / CPU tensor
               (preprocess.chain_plan builds it; uploaded here).  dir 0 follows flow_1_2 with mask_2, dir 1 flow_2_1 with mask_1
      out      optional dict of preallocated outputs; out['flow'] may have a row stride above B * H * W * 2 (a slice of a larger
               tensor along dimension 1), everything within a row contiguous
    include/dvd_hip.h has the sampling rule.  Everything is checked on the host before the launch, the table goes up in one
    pinned upload, and nothing synchronises with the device."""
    what = 'flow_chain'
    # the host data first: a bad table is refused before a tensor is looked at
    ln = _host_ids(what, 'links (rows of pair, dir)', links, (None, None, 2), floats=False)
    B, L = int(ln.shape[0]), int(ln.shape[1])
    if not 1 <= L <= CHAIN_MAX_LINKS:
        raise RuntimeError('%s: links holds L=%d links per chain, 1 .. %d are possible' % (what, L, CHAIN_MAX_LINKS))
    if not 1 <= B <= 65535:
        raise RuntimeError('%s: links must hold 1 .. 65535 chains per launch, got %d' % (what, B))
    ended = ln[..., 0] == -1
    n_live = np.where(ended.any(1), ended.argmax(1), L)                 # links before the row's first -1
    live = np.arange(L)[None, :] < n_live[:, None]
    f12 = _dev32(flow_1_2, 'flow_1_2')
    dev = f12.device
    if f12 is not flow_1_2 or f12.dim() != 4 or f12.shape[3] != 2 or f12.shape[0] < 1:
        raise RuntimeError('%s: flow_1_2 must be contiguous [P,H,W,2], got %s' % (what, tuple(f12.shape)))
    P, H, W = (int(v) for v in f12.shape[:3])
    if H < 2 or W < 2 or H * W >= 1 << 30:
        raise RuntimeError('%s: images of %d x %d; the sampling rule needs H, W >= 2, and H * W must stay below 2^30' % (what, H, W))
    _out_ok(what, 'flow_2_1', flow_2_1, f12.shape, torch.float32, dev, 'flow_1_2')
    if mask_1 is None or mask_2 is None:
        raise RuntimeError('%s: mask_1 and mask_2 are required, got None for %s' % (what, 'mask_1' if mask_1 is None else 'mask_2'))
    mask_1 = _dev_u8(what, 'mask_1', mask_1, (P, H, W), dev, copy=False)
    mask_2 = _dev_u8(what, 'mask_2', mask_2, (P, H, W), dev, copy=False)
    if live.any() and (int(ln[..., 0][live].min()) < 0 or int(ln[..., 0][live].max()) >= P):
        raise RuntimeError('%s: links names pairs in [%d, %d], outside -1 (the end) .. %d' % (
            what, int(ln[..., 0][live].min()), int(ln[..., 0][live].max()), P - 1))
    if live.any() and not np.isin(ln[..., 1][live], (0, 1)).all():
        raise RuntimeError('%s: the dir column of links must be 0 (flow_1_2) or 1 (flow_2_1)' % what)
    row = B * H * W * 2
    flow = out.get('flow') if out is not None else None
    if flow is None:
        flow = torch.empty((L, B, H, W, 2), device=dev, dtype=torch.float32)
    elif not (torch.is_tensor(flow) and flow.device == dev and flow.dtype == torch.float32 and tuple(flow.shape) == (L, B, H, W, 2)
              and flow[0].is_contiguous() and (L == 1 or (flow.stride(0) >= row and flow.stride(0) % 2 == 0))
              and flow.data_ptr() % 8 == 0):
        raise RuntimeError("%s: out['flow'] must be a float32 tensor %s on the device of the flows, contiguous within a row, the "
                           "rows an even stride of at least %d apart" % (what, [L, B, H, W, 2], row))
    res = {'flow': flow}
    res.update(_outputs(what, out, {'broken': ((L, B, H, W), torch.uint8)}, dev, 'the flows'))
    stride = int(flow.stride(0)) if L > 1 else row
    # ONE upload from pinned memory, enqueued on the current stream: a copy from pageable memory would make the host wait
    table = torch.from_numpy(np.ascontiguousarray(ln.astype(np.int32))).pin_memory().to(dev, non_blocking=True)
    _lib.check(_lib.load().dvd_flow_chain(_p(f12), _p(flow_2_1), _p(mask_1), _p(mask_2), P, _p(table), int(n_live.sum()),
                                          _p(flow), stride, _p(res['broken']), L, B, H, W, _stream()), 'dvd_flow_chain')
    return res


def invert_update(p, sf, y_old, out=None, resid=None):
    """One fixed-point update of the inverse Euler step (dvd_track_invert_update, csrc/invert.hip): out = p - sf, and resid[b]
    = max(resid[b], max |out - y_old| of image b) -- the caller zeroes resid; a NaN difference counts as +Inf.
      p, sf, y_old  [B,3,H,W] contiguous fp32 on one GPU; y_old may be p or out
      out      optional destination [B,3,H,W] (it may be y_old; not p or sf);  resid: optional fp32 [B]
    Everything is checked on the host before the launch."""
    what = 'invert_update'
    p = _point_slab(what, p)
    B, _, H, W = (int(v) for v in p.shape)
    if B > 65535 or H * W >= 1 << 30:
        raise RuntimeError('%s: at most 65535 images of fewer than 2^30 pixels per launch, got %d of %d x %d' % (what, B, H, W))
    if out is None:
        out = torch.empty_like(p)
    for name, v in (('sf', sf), ('y_old', y_old), ('out', out)):
        _out_ok(what, name, v, p.shape, torch.float32, p.device, 'p')
    if out.data_ptr() in (p.data_ptr(), sf.data_ptr()) and out.data_ptr() != y_old.data_ptr():
        raise RuntimeError('%s: out may alias y_old only' % what)
    if resid is not None:
        _out_ok(what, 'resid', resid, (B,), torch.float32, p.device, 'p')
    _lib.check(_lib.load().dvd_track_invert_update(_p(p), _p(sf), _p(y_old), _p(out), _p(resid), B, H * W, _stream()),
               'dvd_track_invert_update')
    return out


def invert_step(mlp, p, t, t_offset, out_scale, n_iter=4, out=None, resid=None, scratch=None):
    """The point y that one Euler step of the scene-flow field carries to p: y + out_scale * f(y, t + t_offset) = p, by n_iter
    fixed-point iterations y <- p - out_scale * f(y, t + t_offset) from y = p.  The step is a near-identity map (out_scale =
    1 / sf_mag_div), so the iteration contracts by a few per cent per round; n_iter = 4 is below one fp32
    ulp of the points on the fields measured there.  Costs n_iter stash-free forwards of the MLP kernels (sf_out = scratch),
    each followed by one invert_update; no torch arithmetic, nothing is read back.
      mlp      a packed SceneFlowMLPKernels;  p [B,3,H,W], t [B,1,H,W] or None as its forward takes them
      out      optional destination [B,3,H,W] (not p);  scratch: optional [B,3,H,W] that receives the last sf
      resid    optional fp32 [B]: zeroed here, then max |y_n - y_(n-1)| of the LAST iteration per image
    Returns out."""
    what = 'invert_step'
    if isinstance(n_iter, bool) or int(n_iter) != n_iter or n_iter < 1:
        raise ValueError('%s: n_iter must be an integer >= 1, got %r' % (what, n_iter))
    p = _point_slab(what, p)
    if out is None:
        out = torch.empty_like(p)
    if scratch is None:
        scratch = torch.empty_like(p)
    for name, v in (('out', out), ('scratch', scratch)):
        _out_ok(what, name, v, p.shape, torch.float32, p.device, 'p')
    if len({p.data_ptr(), out.data_ptr(), scratch.data_ptr()}) != 3:
        raise RuntimeError('%s: p, out and scratch must be three buffers' % what)
    if resid is not None:
        _out_ok(what, 'resid', resid, (int(p.shape[0]),), torch.float32, p.device, 'p')
    y = p
    for i in range(int(n_iter)):
        last = i == int(n_iter) - 1
        mlp.forward(y, t, t_offset=t_offset, out_scale=out_scale, sf_out=scratch)
        if last and resid is not None:
            resid.zero_()
        invert_update(p, scratch, y, out=out, resid=resid if last else None)
        y = out
    return out


def project_backward(g_uv, points, start, tables, planar=True, out=None, accumulate=False, host_start=None):
    """g_points (+)= J^T g_uv for track_project's uv (dvd_project_bwd): g_uv [T1,B,H,W,2], the result in the layout of
    points.  Cameras get no gradient; a frame past the end of the tables contributes 0."""
    what = 'project_backward'
    points, start, (R, t, K_T), T1, B, H, W, N = _track_args(what, points, start, tables, planar, host_start)
    g_uv = _dev32(g_uv, 'g_uv')
    if g_uv.device != points.device or tuple(g_uv.shape) != (T1, B, H, W, 2):
        raise RuntimeError('%s: g_uv must be %s on the device of the points, got %s' % (what, (T1, B, H, W, 2), tuple(g_uv.shape)))
    if out is None:
        if accumulate:
            raise RuntimeError('accumulate=True needs an output tensor')
        out = torch.empty_like(points)
    else:
        _out_ok(what, 'out', out, points.shape, torch.float32, points.device, 'the points')
    _lib.check(_lib.load().dvd_project_bwd(_p(g_uv), _p(points), int(bool(planar)), _p(start), _p(R), _p(t), _p(K_T), N, _p(out),
                                           int(bool(accumulate)), T1, B, H, W, _stream()), 'dvd_project_bwd')
    return out


# -- query-point tracks (csrc/point_track.hip) -------------------------------------------------------------------------------
POINT_SEED_TABLES = ('R_T', 't', 'K_inv_T')
POINT_CAP = 1024.0           # the position error of the last word is capped here (2^10)
POINT_THRESHOLDS = (1.0, 2.0, 4.0, 8.0, 16.0)
POINT_SUMS = (('n_eval', 'n_gt_visible', 'n_occ_agree') + tuple('n_within_%d' % i for i in range(5)) +
              tuple('n_tp_%d' % i for i in range(5)) + tuple('n_fp_%d' % i for i in range(5)) + ('err',))


def _point_queries(what, frame, xy, dev, on, N, host_frame=None):
    """The query list of the point kernels -> (frame int32 [Q] on dev, xy float32 [Q,2] on dev, Q).  frame: a host sequence /
    array / CPU tensor (range-checked against the N frames, uploaded here) or a GPU int32 tensor (checked from host_frame where
    the caller has it, never read back); xy: a GPU float32 tensor."""
    xy = _dev32(xy, 'xy')
    if xy.dim() != 2 or xy.shape[1] != 2 or xy.shape[0] < 1 or xy.device != dev:
        raise RuntimeError('%s: xy must be a float32 tensor [Q,2] with Q >= 1 on the device of %s, got %s' % (what, on, tuple(xy.shape)))
    Q = int(xy.shape[0])
    if Q >= 1 << 30:
        raise RuntimeError('%s: at most 2^30 - 1 queries per launch, got %d' % (what, Q))
    frame, _ = _ids(what, 'frame', frame, (Q,), 0, N, dev, on, host=host_frame)
    return frame, xy, Q


def point_seed(frame, xy, depth_all, tables, time_stamps=True, out=None, host_frame=None):
    """Queries -> world points (dvd_point_seed, csrc/point_track.hip) -> {'points' [3,Q], 'ok' uint8 [Q][, 't' [Q]]}.
      frame    Q frame ids: a host sequence / array / CPU tensor (uploaded here) or a GPU int32 tensor (then host_frame, its host
               copy, is what the range check reads; without it the kernel's own check decides: `ok` is 0 for a frame outside)
      xy       GPU float32 [Q,2]: the position in the frame, pixel centres at integers
      depth_all [N,1,H,W];  tables {'R_T': [N,3,3] camera->world, 't': [N,3], 'K_inv_T': [N,3,3], 'ts_vali': [N]} --
               FrameStore.tables has them under these names;  time_stamps False: no 't' (a time-independent field)
      out      optional dict of preallocated outputs (points may be a row of a [T1,3,Q] slab)
    The depth is sampled by direct bilinear taps (weights exactly (1,0,0,0) at an integer position) and un-projected by the
    per-pixel body of ops.unproject: an integer query has that pixel's bits.  ok = the frame exists, the depth is finite and
    > 0 and the position is inside [0,W-1] x [0,H-1]; otherwise the point is 0.  Checked on the host; nothing is read back."""
    what = 'point_seed'
    depth_all = _dev32(depth_all, 'depth_all')
    dev = depth_all.device
    if depth_all.dim() != 4 or depth_all.shape[1] != 1 or depth_all.numel() == 0:
        raise RuntimeError('%s: depth_all must be [N,1,H,W], got %s' % (what, tuple(depth_all.shape)))
    N, _, H, W = (int(v) for v in depth_all.shape)
    if H < 2 or W < 2 or H * W >= 1 << 30:
        raise RuntimeError('%s: images of %d x %d; the sampling rule needs H, W >= 2 and H * W < 2^30' % (what, H, W))
    (R_T, t, K_inv_T), _ = _tables(what, tables, POINT_SEED_TABLES, (9, 3, 9), dev, 'the depth', n=N)
    ts = None
    if time_stamps:
        if 'ts_vali' not in tables:
            raise RuntimeError('%s: tables must hold ts_vali (or pass time_stamps=False)' % what)
        ts = _dev32(tables['ts_vali'], 'table ts_vali')
        if ts.device != dev or ts.numel() != N:
            raise RuntimeError('%s: table ts_vali must hold one value for each of %d rows, got %s' % (what, N, tuple(ts.shape)))
    frame, xy, Q = _point_queries(what, frame, xy, dev, 'the depth', N, host_frame)
    shapes = {'points': ((3, Q), torch.float32), 'ok': ((Q,), torch.uint8)}
    if time_stamps:
        shapes['t'] = ((Q,), torch.float32)
    res = _outputs(what, out, shapes, dev, 'the depth')
    _lib.check(_lib.load().dvd_point_seed(_p(frame), _p(xy), _p(depth_all), _p(R_T), _p(t), _p(K_inv_T), _p(ts), N,
                                          _p(res['points']), _p(res.get('t')), _p(res['ok']), Q, H, W, _stream()), 'dvd_point_seed')
    return res


def point_project(points, frame, xy, tables, depth_all, k0=0, z_tol=0.05, ok=None, out=None, host_frame=None):
    """Rows of integrated query points into their own target cameras (dvd_point_project) -> dict of uv [T1,Q,2], z, depth_at
    [T1,Q], inside, visible uint8 [T1,Q], target int32 [T1,Q].
      points   [T1,3,Q]: row j of query q is its world point at the time of frame g = frame[q] + j + k0
      frame, xy, host_frame  as point_seed takes them;  tables {'R', 't', 'K_T'} as track_project takes them
      ok       None or uint8 [Q] (point_seed's): a query that is not ok gives zeros
    The projection and the depth sample are track_project's, with the query's position as the source pixel: an integer query
    has the bits track_project(.., k0) gives that pixel.  visible = inside && !(z > depth_at * (1 + z_tol)) (eval_tracks'
    occlusion rule); target = g, or -1 where g is no frame or the query is not ok -- such a row is all zeros."""
    what = 'point_project'
    points = _dev32(points, 'points')
    if points.dim() != 3 or points.shape[1] != 3 or points.numel() == 0:
        raise RuntimeError('%s: points must be [T1,3,Q], got %s' % (what, tuple(points.shape)))
    dev = points.device
    T1 = int(points.shape[0])
    if T1 > 65535:
        raise RuntimeError('%s: at most 65535 rows per launch, got %d' % (what, T1))
    k0 = _int_arg(what, 'k0', k0, 1 - (1 << 30), (1 << 30) - 1)
    z_tol = _real_arg(what, 'z_tol', float(z_tol))
    (R, t, K_T), N = _tables(what, tables, TRACK_TABLES, (9, 3, 9), dev, 'the points')
    frame, xy, Q = _point_queries(what, frame, xy, dev, 'the points', N, host_frame)
    if int(points.shape[2]) != Q:
        raise RuntimeError('%s: points hold %d queries, xy %d' % (what, int(points.shape[2]), Q))
    depth_all = _dev32(depth_all, 'depth_all')
    if depth_all.device != dev or depth_all.dim() != 4 or depth_all.shape[0] != N or depth_all.shape[1] != 1:
        raise RuntimeError('%s: depth_all must be [%d,1,H,W] on the device of the points, got %s' % (what, N, tuple(depth_all.shape)))
    H, W = int(depth_all.shape[2]), int(depth_all.shape[3])
    if H < 2 or W < 2 or H * W >= 1 << 30:
        raise RuntimeError('%s: images of %d x %d; the sampling rule needs H, W >= 2 and H * W < 2^30' % (what, H, W))
    ok = _dev_u8(what, 'ok', ok, (Q,), dev)
    res = _outputs(what, out, {'uv': ((T1, Q, 2), torch.float32), 'z': ((T1, Q), torch.float32),
                               'depth_at': ((T1, Q), torch.float32), 'inside': ((T1, Q), torch.uint8),
                               'visible': ((T1, Q), torch.uint8), 'target': ((T1, Q), torch.int32)}, dev, 'the points')
    _lib.check(_lib.load().dvd_point_project(_p(points), _p(frame), _p(xy), _p(ok), k0, _p(R), _p(t), _p(K_T), _p(depth_all), N,
                                             z_tol, _p(res['uv']), _p(res['z']), _p(res['depth_at']), _p(res['inside']),
                                             _p(res['visible']), _p(res['target']), T1, Q, H, W, _stream()), 'dvd_point_project')
    return res


def point_thr2(thresholds):
    """The five squared thresholds as the kernel receives them: float32(t) * float32(t), rounded to float32."""
    try:
        thr = np.asarray(thresholds, dtype=np.float32).reshape(-1)
    except (TypeError, ValueError):
        thr = np.zeros(0, np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        thr2 = (thr * thr).astype(np.float32)
    if thr.size != 5 or not np.all(np.isfinite(thr2)) or not np.all(thr > 0) or not np.all(np.diff(thr2) > 0) or not thr2[0] > 0:
        raise RuntimeError('point_score: thresholds must be 5 positive, ascending, finite numbers, got %r' % (thresholds,))
    return thr2


def point_score(uv, visible, target, gt_uv, gt_state, origin=-1, thresholds=POINT_THRESHOLDS, px_scale=(1.0, 1.0), sums=None):
    """Predicted tracks against annotated ones (dvd_point_score): the TAP-Vid counts -> {'sums' int64 [T1,19], 'shift'}.
      uv [T1,Q,2], visible uint8 [T1,Q], target int32 [T1,Q]   point_project's outputs
      gt_uv    float32 [Q,N,2], frame-major;  gt_state uint8 [Q,N]: 0 visible, 1 occluded, >= 2 not annotated
      origin   the slab row of the queries themselves, which is not scored (-1: none)
      thresholds  five distances in pixels of the raster px_scale = (sx, sy) maps to: du = (u - gu) * sx, dv = (v - gv) * sy
      sums     None (a cleared tensor is made) or an int64 [T1,19] tensor to ACCUMULATE into; words POINT_SUMS per slab row,
               the last one in units of 2^-shift, shift = eval_shift(Q)
    A point counts iff 0 <= target < N, its row is not the origin and gt_state < 2.  Integer atomics only: the same inputs give
    the same bits for any grid.  Everything is checked on the host before the launch; nothing is read back."""
    what = 'point_score'
    uv = _dev32(uv, 'uv')
    if uv.dim() != 3 or uv.shape[2] != 2 or uv.numel() == 0:
        raise RuntimeError('%s: uv must be [T1,Q,2], got %s' % (what, tuple(uv.shape)))
    dev = uv.device
    T1, Q = int(uv.shape[0]), int(uv.shape[1])
    if T1 > 65535 or Q >= 1 << 30:
        raise RuntimeError('%s: at most 65535 rows of fewer than 2^30 queries per launch, got %d of %d' % (what, T1, Q))
    visible = _dev_u8(what, 'visible', visible, (T1, Q), dev)
    if visible is None:
        raise RuntimeError('%s: visible must be a GPU uint8 tensor [%d,%d]' % (what, T1, Q))
    _out_ok(what, 'target', target, (T1, Q), torch.int32, dev, 'uv')
    gt_uv = _dev32(gt_uv, 'gt_uv')
    if gt_uv.device != dev or gt_uv.dim() != 3 or gt_uv.shape[0] != Q or gt_uv.shape[1] < 1 or gt_uv.shape[2] != 2:
        raise RuntimeError('%s: gt_uv must be [%d,N,2] on the device of uv, got %s' % (what, Q, tuple(gt_uv.shape)))
    N = int(gt_uv.shape[1])
    gt_state = _dev_u8(what, 'gt_state', gt_state, (Q, N), dev)
    if gt_state is None:
        raise RuntimeError('%s: gt_state must be a GPU uint8 tensor [%d,%d]' % (what, Q, N))
    origin = _int_arg(what, 'origin', origin, -1, T1 - 1)
    if not isinstance(px_scale, (tuple, list)) or len(px_scale) != 2:
        raise RuntimeError('%s: px_scale must be (sx, sy), got %r' % (what, px_scale))
    sx, sy = (_real_arg(what, n, v, lo_open=True) for n, v in zip(('sx', 'sy'), px_scale))
    thr2 = point_thr2(thresholds)
    shift = eval_shift(Q)
    if sums is None:
        sums = torch.zeros((T1, len(POINT_SUMS)), device=dev, dtype=torch.int64)
    else:
        _out_ok(what, 'sums', sums, (T1, len(POINT_SUMS)), torch.int64, dev, 'uv')
    c_thr2 = (ctypes.c_float * 5)(*[float(v) for v in thr2])
    _lib.check(_lib.load().dvd_point_score(_p(uv), _p(visible), _p(target), origin, _p(gt_uv), _p(gt_state), N, sx, sy, c_thr2,
                                           shift, _p(sums), T1, Q, _stream()), 'dvd_point_score')
    return {'sums': sums, 'shift': shift}


# -- forward splat with a soft z-buffer (csrc/splat.hip) -------------------------------------------------------------------
SPLAT_MAX_C = 8
SPLAT_DEFAULTS = dict(z_near=1e-3, z_tol=0.05, w_tap=1.0 / 64, w_min=0.25, value_bound=1.0, fill=0.0)


def splat_shift(n):
    """The fixed-point shift of the splat's accumulators for at most n points per view: min(40, 62 - ceil_log2(n)).  A term
    is at most 2^shift in magnitude, so n of them stay within 2^62."""
    n = int(n)
    if n < 1:
        raise RuntimeError('splat_shift: n must be >= 1, got %d' % n)
    return min(40, 62 - (n - 1).bit_length())


def _splat_sources(what, points, values, view, tables, n_views, valid, planar, host_view):
    """Everything the splat passes check about their sources before a launch -> (points, values, valid, view on the device,
    the three tables, S, C, H, W, V, n_max).  n_max: the largest number of points one view can receive -- from the host copy
    of `view` where there is one, S * H * W otherwise (a device tensor is never read back)."""
    import numpy as np
    points = _dev32(points, 'points')
    if points.dim() != 4 or points.shape[1 if planar else 3] != 3 or points.numel() == 0:
        raise RuntimeError('%s: points must be [S,3,H,W] (planar) or [S,H,W,3], got %s' % (what, tuple(points.shape)))
    S = int(points.shape[0])
    H, W = (int(v) for v in (points.shape[2:4] if planar else points.shape[1:3]))
    dev = points.device
    if H < 2 or W < 2:
        raise RuntimeError('%s: images of %d x %d; a bilinear tap set needs H, W >= 2' % (what, H, W))
    if S > 65535:
        raise RuntimeError('%s: at most 65535 source images per launch, got %d' % (what, S))
    values = _dev32(values, 'values')
    if values.device != dev or values.dim() != 4 or values.shape[0] != S or tuple(values.shape[2:]) != (H, W) or \
            not 1 <= values.shape[1] <= SPLAT_MAX_C:
        raise RuntimeError('%s: values must be [%d,C,%d,%d] with 1 <= C <= %d on the device of the points, got %s' % (
            what, S, H, W, SPLAT_MAX_C, tuple(values.shape)))
    C = int(values.shape[1])
    valid = _dev_u8(what, 'valid', valid, (S, H, W), dev)
    V = _int_arg(what, 'n_views', n_views, 1, 65535)
    tabs, _ = _tables(what, tables, TRACK_TABLES, (9, 3, 9), dev, 'the points', n=V)
    # any id that fits 32 bits: one that is no view (< 0 or >= V) skips its image
    view, host = _ids(what, 'view', view, (S,), -2 ** 31, 2 ** 31, dev, 'the points', host=host_view)
    n_max = S * H * W
    if host is not None:
        live = host[(host >= 0) & (host < V)]
        per_view = int(np.bincount(live.astype(np.int64), minlength=1).max()) if live.size else 0
        n_max = max(1, per_view) * H * W
    return points, values, valid, view, tabs, S, C, H, W, V, n_max


def _splat_params(what, **p):
    """The numeric parameters as floats, refused here with the kernels' own rules."""
    rules = {'z_near': {}, 'z_tol': {}, 'w_tap': dict(lo_open=True, hi=0.25), 'w_min': dict(lo_open=True),
             'value_bound': dict(lo_open=True), 'fill': None}
    return {k: float(v) if rules[k] is None else _real_arg(what, k, float(v), **rules[k]) for k, v in p.items()}


def splat_workspace(n_views, C, H, W, device):
    """The splat's workspace as torch tensors, uncleared: (zbuf int32 [V,H,W], acc int64 [V,H,W,C+1])."""
    V, C, H, W = int(n_views), int(C), int(H), int(W)
    nbytes = _lib.load().dvd_splat_workspace_bytes(V, C, H, W)
    if nbytes == 0:
        raise RuntimeError('splat_workspace: no workspace for V=%d C=%d H=%d W=%d' % (V, C, H, W))
    zbuf = torch.empty((V, H, W), device=device, dtype=torch.int32)
    acc = torch.empty((V, H, W, C + 1), device=device, dtype=torch.int64)
    assert zbuf.numel() * 4 + acc.numel() * 8 == nbytes
    return zbuf, acc


def splat_clear(zbuf, acc):
    """The two clears every splat starts from: zbuf to 0xFF bytes (empty), acc to 0."""
    zbuf.fill_(-1)
    acc.zero_()


def _splat_ws_ok(what, zbuf, acc, dev, V, C, H, W):
    _out_ok(what, 'zbuf', zbuf, (V, H, W), torch.int32, dev, 'the points')
    if acc is not None:
        _out_ok(what, 'acc', acc, (V, H, W, C + 1), torch.int64, dev, 'the points')


def splat_zmin(zbuf, points, values, view, tables, n_views, valid=None, planar=True, z_near=1e-3, w_tap=1.0 / 64,
               host_view=None):
    """Pass a of the splat (dvd_splat_zmin): the nearest depth per target pixel into a cleared zbuf."""
    what = 'splat_zmin'
    points, values, valid, view, (R, t, K_T), S, C, H, W, V, _ = _splat_sources(what, points, values, view, tables, n_views,
                                                                                 valid, planar, host_view)
    p = _splat_params(what, z_near=z_near, w_tap=w_tap)
    _splat_ws_ok(what, zbuf, None, points.device, V, C, H, W)
    _lib.check(_lib.load().dvd_splat_zmin(_p(points), int(bool(planar)), _p(values), _p(valid), _p(view), _p(R), _p(t), _p(K_T),
                                          V, _p(zbuf), S, C, H, W, p['z_near'], p['w_tap'], _stream()), 'dvd_splat_zmin')


def splat_accumulate(zbuf, acc, shift, n_max, points, values, view, tables, n_views, valid=None, planar=True, z_near=1e-3,
                     z_tol=0.05, w_tap=1.0 / 64, value_bound=1.0, host_view=None):
    """Pass b of the splat (dvd_splat_accumulate): the taps within z_tol of zbuf's depth, added to acc in fixed point.  n_max
    bounds the points one view receives over all the calls that add into this acc; shift <= splat_shift(n_max)."""
    what = 'splat_accumulate'
    points, values, valid, view, (R, t, K_T), S, C, H, W, V, _ = _splat_sources(what, points, values, view, tables, n_views,
                                                                                 valid, planar, host_view)
    p = _splat_params(what, z_near=z_near, z_tol=z_tol, w_tap=w_tap, value_bound=value_bound)
    _splat_ws_ok(what, zbuf, acc, points.device, V, C, H, W)
    _lib.check(_lib.load().dvd_splat_accumulate(_p(points), int(bool(planar)), _p(values), _p(valid), _p(view), _p(R), _p(t),
                                                _p(K_T), V, _p(zbuf), _p(acc), S, C, H, W, p['z_near'], p['z_tol'], p['w_tap'],
                                                p['value_bound'], int(shift), int(n_max), _stream()), 'dvd_splat_accumulate')


def splat_resolve(zbuf, acc, shift, w_min=0.25, value_bound=1.0, fill=0.0, out=None):
    """Pass c of the splat (dvd_splat_resolve) -> dict of image [V,C,H,W], depth [V,1,H,W], weight [V,1,H,W], hit uint8 [V,H,W]."""
    what = 'splat_resolve'
    if not (torch.is_tensor(acc) and acc.is_cuda and acc.dim() == 4):
        raise RuntimeError('%s: acc must be a GPU tensor [V,H,W,C+1] (dvd_hip has no CPU path)' % what)
    V, H, W, C = (int(v) for v in acc.shape)
    C -= 1
    _splat_ws_ok(what, zbuf, acc, acc.device, V, C, H, W)
    p = _splat_params(what, w_min=w_min, value_bound=value_bound, fill=fill)
    res = _outputs(what, out, {'image': ((V, C, H, W), torch.float32), 'depth': ((V, 1, H, W), torch.float32),
                               'weight': ((V, 1, H, W), torch.float32), 'hit': ((V, H, W), torch.uint8)}, acc.device, 'the workspace')
    _lib.check(_lib.load().dvd_splat_resolve(_p(zbuf), _p(acc), V, C, H, W, int(shift), p['w_min'], p['value_bound'], p['fill'],
                                             _p(res['image']), _p(res['depth']), _p(res['weight']), _p(res['hit']), _stream()),
               'dvd_splat_resolve')
    return res


def splat(points, values, view, tables, n_views, valid=None, planar=True, z_near=1e-3, z_tol=0.05, w_tap=1.0 / 64, w_min=0.25,
          value_bound=1.0, fill=0.0, out=None, host_view=None):
    """Forward bilinear splat with a soft z-buffer (csrc/splat.hip) -> dict of image [V,C,H,W], depth [V,1,H,W], weight
    [V,1,H,W] and hit uint8 [V,H,W], V = n_views.
      points   [S,3,H,W] (planar) or [S,H,W,3] world points;  values [S,C,H,W], 1 <= C <= 8;  valid uint8 [S,H,W] or None
      view     S view ids: a host sequence / array / CPU tensor (uploaded here) or a GPU int32 tensor (never read back; with
               host_view, its host copy, the accumulators keep more fraction bits).  -1 or >= n_views skips the image.
      tables   {'R': [V,3,3] world->camera, 't': [V,3], 'K_T': [V,3,3]}: the rows of the V views
      z_near   points at or in front of it are dropped;  z_tol: a tap is blended if z <= zmin * (1 + z_tol)
      w_tap    the least bilinear weight with which a tap counts;  w_min: the least summed weight of a hit pixel
      value_bound  values are clamped to +-value_bound;  fill: the image where nothing hit
    Allocates the workspace with torch, clears it and runs the three passes on the current stream.  Integer atomics only:
    the same inputs give the same bits whatever the order of the sources."""
    what = 'splat'
    points, values, valid, view, tabs, S, C, H, W, V, n_max = _splat_sources(what, points, values, view, tables, n_views, valid,
                                                                             planar, host_view)
    _splat_params(what, z_near=z_near, z_tol=z_tol, w_tap=w_tap, w_min=w_min, value_bound=value_bound, fill=fill)
    tables = dict(zip(TRACK_TABLES, tabs))
    shift = splat_shift(n_max)
    zbuf, acc = splat_workspace(V, C, H, W, points.device)
    splat_clear(zbuf, acc)
    splat_zmin(zbuf, points, values, view, tables, V, valid=valid, planar=planar, z_near=z_near, w_tap=w_tap)
    splat_accumulate(zbuf, acc, shift, n_max, points, values, view, tables, V, valid=valid, planar=planar, z_near=z_near,
                     z_tol=z_tol, w_tap=w_tap, value_bound=value_bound)
    return splat_resolve(zbuf, acc, shift, w_min=w_min, value_bound=value_bound, fill=fill, out=out)


# -- push-pull hole filling (csrc/fill.hip) ----------------------------------------------------------------------------------
FILL_MAX_C = 8              # kFillMaxC of csrc/fill.hip
FILL_MAX_TILES = 2048       # kFillMaxTiles: the largest ceil(H / 32) * ceil(W / 32)
FILL_EMPTY = 255            # the level of a view without a known pixel


def fill_workspace(n_views, C, H, W, device):
    """The workspace of fill_holes as a torch tensor, uncleared: levels 1 .. 5 of the pyramid, float32 [V, floats per view]."""
    V, C, H, W = int(n_views), int(C), int(H), int(W)
    nbytes = _lib.load().dvd_fill_workspace_bytes(V, C, H, W)
    if nbytes == 0:
        raise RuntimeError('fill_workspace: no workspace for V=%d C=%d H=%d W=%d (1 <= C <= %d, at most %d tiles of 32 x 32)' % (
            V, C, H, W, FILL_MAX_C, FILL_MAX_TILES))
    return torch.empty((V, nbytes // (4 * V)), device=device, dtype=torch.float32)


def fill_holes(values, known, bias=None, power=0, fill=0.0, out=None, workspace=None):
    """Push-pull hole filling (csrc/fill.hip) -> dict of values [V,C,H,W] and level uint8 [V,H,W].
      values   [V,C,H,W], 1 <= C <= 8;  known  uint8 [V,H,W], non-zero where the pixel holds data
      bias     [V,1,H,W] or None, power 0 .. 4: a known pixel weighs bias^power (one whose bias is not > 0, or whose weight is not
               finite, counts as unknown), so that with a depth as bias the deeper surface dominates a coarse pixel that mixes two
      fill     the values of a view without a known pixel
      out      {'values', 'level'}, either or both preallocated; out['values'] may be `values` itself (in place)
      workspace  fill_workspace(V, C, H, W, device), or None to allocate it here
    Known pixels come back bit for bit; level is 0 there, k >= 1 where the nearest known ancestor sits at pyramid level k, 255
    for an empty view.  Three launches on the current stream whatever the size, no atomics: the same inputs give the same bits,
    and a view's result does not depend on the views it shares the call with."""
    what = 'fill_holes'
    values = _dev32(values, 'values')
    if values.dim() != 4 or not 1 <= values.shape[1] <= FILL_MAX_C or values.numel() == 0:
        raise RuntimeError('%s: values must be [V,C,H,W] with 1 <= C <= %d, got %s' % (what, FILL_MAX_C, tuple(values.shape)))
    V, C, H, W = (int(v) for v in values.shape)
    dev = values.device
    if V > 65535:
        raise RuntimeError('%s: at most 65535 views per launch, got %d' % (what, V))
    known = _dev_u8(what, 'known', known, (V, H, W), dev)
    if known is None:
        raise RuntimeError('%s: known must be a GPU uint8 tensor [%d, %d, %d]' % (what, V, H, W))
    if bias is not None:
        bias = _dev32(bias, 'bias')
        if bias.device != dev or tuple(bias.shape) != (V, 1, H, W):
            raise RuntimeError('%s: bias must be [%d,1,%d,%d] on the device of the values, got %s' % (what, V, H, W, tuple(bias.shape)))
    power = _int_arg(what, 'power', power, 0, 4)
    if isinstance(fill, bool) or not isinstance(fill, (int, float, np.integer, np.floating)):
        raise RuntimeError('%s: fill must be a number, got %r' % (what, fill))
    if workspace is None:
        workspace = fill_workspace(V, C, H, W, dev)
    else:
        nbytes = _lib.load().dvd_fill_workspace_bytes(V, C, H, W)
        if nbytes == 0:
            raise RuntimeError('%s: images of %d x %d are not supported (at most %d tiles of 32 x 32)' % (what, H, W, FILL_MAX_TILES))
        if not (torch.is_tensor(workspace) and workspace.device == dev and workspace.dtype == torch.float32 and
                workspace.is_contiguous() and workspace.numel() * 4 >= nbytes):
            raise RuntimeError('%s: workspace must be a contiguous float32 tensor of at least %d bytes on the device of the values' % (
                what, nbytes))
    res = _outputs(what, out, {'values': ((V, C, H, W), torch.float32), 'level': ((V, H, W), torch.uint8)}, dev, 'the values')
    _lib.check(_lib.load().dvd_fill_holes(_p(values), _p(known), _p(bias), power, float(fill), V, C, H, W, _p(res['values']),
                                          _p(res['level']), _p(workspace), _stream()), 'dvd_fill_holes')
    return res


# -- a finished optimisation scored along its tracks (csrc/eval.hip) ---------------------------------------------------------
EVAL_CAP = 1024.0            # photo and epe are capped here (2^10); rel at 1
EVAL_SUMS = ('n_inside', 'n_occluded', 'depth_rel', 'photo', 'n_flow', 'flow_epe')


def eval_shift(n_pixels):
    """The fixed-point shift of eval_tracks' sums for images of n_pixels points: min(32, 62 - 10 - ceil_log2(n_pixels)).  A
    term is at most 2^10 * 2^shift, so the n_pixels terms of a row stay within 2^62."""
    n = int(n_pixels)
    if n < 1:
        raise RuntimeError('eval_shift: n_pixels must be >= 1, got %d' % n)
    return min(32, 62 - 10 - (n - 1).bit_length())


def _step_view(what, name, t, shape, dtype, dev):
    """A [T,B,...] destination whose steps may be further apart than B rows (the columns of a larger tensor) -> its step
    stride in elements."""
    if not (torch.is_tensor(t) and t.device == dev and t.dtype == dtype and tuple(t.shape) == shape and
            t[0].is_contiguous() and (shape[0] == 1 or t.stride(0) >= t[0].numel())):
        raise RuntimeError('%s: %s must be a %s tensor %s on the device of the points, contiguous within a step' % (
            what, name, dtype, shape))
    return int(t.stride(0)) if shape[0] > 1 else int(t[0].numel())


def eval_tracks(points, source, tables, depth_all, img_all, k_first=1, pairs=None, z_tol=0.05, d_min=1e-3, sums=None,
                maps=False, host_source=None):
    """Integrated world points against the frames they land in (dvd_eval_tracks, csrc/eval.hip) -> {'sums', 'shift'[, 'maps']}.
      points   [T,B,3,H,W] planar: row r of image b is frame source[b]'s pixels at the time of frame source[b] + k_first + r
      source   B frame ids: host sequence / array / CPU tensor (uploaded here) or a GPU int32 tensor (then host_source, its
               host copy, saves the read-back of the range check);  tables {'R', 't', 'K_T'} as track_project takes them
      depth_all [N,1,H,W] refined depth;  img_all [N,3,H,W]
      pairs    None or (pair_row, flow_1_2 [P,H,W,2], mask uint8 [P,H,W], 0 = valid): pair_row [T,B] holds the row of the flow
               pair (source[b], target frame) or -1 -- a host array (uploaded here) or a GPU int32 tensor (never read back)
      z_tol    a point deeper than the target's depth * (1 + z_tol) is occluded;  d_min: floor of the depth rel divides by
      sums     None (a cleared tensor is made) or an int64 [T,B,6] tensor to ACCUMULATE into; its steps may be the columns of
               a larger tensor.  Entries: n_inside, n_occluded, sum rel, sum photo, n_flow, sum epe, the value sums in units
               of 2^-shift.
      maps     True, or a float32 [T,B,3,H,W] destination: rel, photo, epe per point, -1 where the point does not count
    Rows whose target frame is past the end of the tables add nothing.  Integer atomics only: the same inputs give the same
    bits for any grid.  Everything is checked on the host before the launch; no device tensor is read back."""
    what = 'eval_tracks'
    points, source, (R, t, K_T), T, B, H, W, N = _track_args(what, points, source, tables, True, host_source)
    dev = points.device
    k_first = _int_arg(what, 'k_first', k_first, 0, 1)
    z_tol, d_min = _real_arg(what, 'z_tol', float(z_tol)), _real_arg(what, 'd_min', float(d_min), lo_open=True)
    depth_all, img_all = _depth_all(what, depth_all, N, H, W, dev), _dev32(img_all, 'img_all')
    if img_all.device != dev or tuple(img_all.shape) != (N, 3, H, W):
        raise RuntimeError('%s: img_all must be [%d,3,%d,%d] on the device of the points, got %s' % (
            what, N, H, W, tuple(img_all.shape)))
    pair_row = flow = mask = None
    P = 0
    if pairs is not None:
        if not isinstance(pairs, (tuple, list)) or len(pairs) != 3 or any(p is None for p in pairs):
            raise RuntimeError('%s: pairs must be (pair_row, flow_1_2, mask), all three' % what)
        pair_row, flow, mask = pairs
        flow = _dev32(flow, 'flow_1_2')
        if flow.device != dev or flow.dim() != 4 or tuple(flow.shape[1:]) != (H, W, 2) or flow.shape[0] < 1:
            raise RuntimeError('%s: flow_1_2 must be [P,%d,%d,2] on the device of the points, got %s' % (what, H, W, tuple(flow.shape)))
        P = int(flow.shape[0])
        mask = _dev_u8(what, 'mask', mask, (P, H, W), dev)
        # -1 or a row of the P flow pairs; a device tensor is never read back
        pair_row, _ = _ids(what, 'pair_row', pair_row, (T, B), -1, P, dev, 'the points', floats=False)
    shift = eval_shift(H * W)
    if sums is None:
        sums = torch.zeros((T, B, 6), device=dev, dtype=torch.int64)
    sums_stride = _step_view(what, 'sums', sums, (T, B, 6), torch.int64, dev)
    maps_stride = 0
    if maps is True:
        maps = torch.empty((T, B, 3, H, W), device=dev, dtype=torch.float32)
    elif maps is False or maps is None:
        maps = None
    if maps is not None:
        maps_stride = _step_view(what, 'maps', maps, (T, B, 3, H, W), torch.float32, dev)
    _lib.check(_lib.load().dvd_eval_tracks(_p(points), _p(source), k_first, _p(R), _p(t), _p(K_T), N, _p(depth_all),
                                           _p(img_all), _p(pair_row), _p(flow), _p(mask), P, z_tol, d_min, shift, _p(sums),
                                           sums_stride, _p(maps), maps_stride, T, B, H, W, _stream()), 'dvd_eval_tracks')
    res = {'sums': sums, 'shift': shift}
    if maps is not None:
        res['maps'] = maps
    return res


# -- depth metrics against a ground truth (csrc/select.hip, csrc/depth_score.hip) ------------------------------------------------
SCORE_CAP = 1024.0           # abs_rel, sq_rel, sq and l^2 are capped here (2^10); l at +-SCORE_LOG_CAP
SCORE_LOG_CAP = 32.0
SCORE_SUMS = ('n', 'abs_rel', 'sq_rel', 'sq', 'log_sq', 'log', 'n_d1', 'n_d2', 'n_d3')
SCORE_REGIONS = ('all', 'static', 'dynamic')
SCORE_MAPS = ('abs_rel', 'sq', 'log')


def ratio_median(num, den, mask=None, den_min=0.0):
    """The exact median of num / den per segment (dvd_ratio_median, csrc/select.hip) -> {'median' [S] fp32, 'count' [S] int64}.
      num, den  [S, L] fp32 (a 1-D tensor is one segment);  mask  None or uint8 [S, L], non-zero = keep
      An element is selected iff den > den_min and its mask byte allows it.  median[s] is numpy's median of the selected fp32
      quotients, bit for bit (NaN where count is 0 or a selected quotient is a NaN).
    A radix select on the device: no sort, no key array, no host synchronisation; the same bits from run to run."""
    what = 'ratio_median'
    num, den = _dev32(num, 'num'), _dev32(den, 'den')
    if num.dim() == 1:
        num = num[None]
    if den.dim() == 1:
        den = den[None]
    if num.dim() != 2 or num.shape != den.shape or num.device != den.device or num.numel() == 0:
        raise RuntimeError('%s: num and den must be non-empty [S,L] tensors of one shape on one device, got %s and %s' % (
            what, tuple(num.shape), tuple(den.shape)))
    S, L = int(num.shape[0]), int(num.shape[1])
    if S > 65535 or S * L >= 2 ** 31:
        raise RuntimeError('%s: S=%d segments of L=%d elements: S <= 65535 and S * L < 2^31 are required' % (what, S, L))
    den_min = float(den_min)
    if den_min != den_min:
        raise RuntimeError('%s: den_min is NaN' % what)
    if mask is not None and torch.is_tensor(mask) and mask.dim() == 1:
        mask = mask[None]
    mask = _dev_u8(what, 'mask', mask, (S, L), num.device)
    dev = num.device
    median = torch.empty(S, device=dev, dtype=torch.float32)
    count = torch.empty(S, device=dev, dtype=torch.int64)
    nbytes = S * _lib.RATIO_MEDIAN_WORKSPACE_PER_SEGMENT
    ws = torch.empty(nbytes // 4, device=dev, dtype=torch.int32)
    _lib.check(_lib.load().dvd_ratio_median(_p(num), _p(den), _p(mask), den_min, S, L, _p(median), _p(count), _p(ws), nbytes,
                                            _stream()), 'dvd_ratio_median')
    return {'median': median, 'count': count}


def depth_score(pred, gt, scale, seg=None, mask=None, g_min=1e-2, sums=None, maps=False, shift=None):
    """A predicted depth against its ground truth (dvd_depth_score, csrc/depth_score.hip) -> {'sums', 'shift'[, 'maps', 'counted']}.
      pred, gt  [N,1,H,W] fp32;  scale  GPU fp32 [N]: the prediction is scored as scale[n] * pred (ratio_median's output, or ones)
      seg       None or [N,H,W] fp32: <= 0.5 static, > 0.5 dynamic;  mask  None or uint8 [N,H,W], non-zero = allowed
      A pixel counts iff gt > g_min, pred > 0, scale * pred is finite and the mask allows it.
      sums      None (a cleared tensor is made) or an int64 [N,3,9] tensor to ACCUMULATE into -- rows all / static / dynamic,
                words SCORE_SUMS, the value sums in units of 2^-shift
      maps      True: also 'maps' [N,3,H,W] (abs_rel, sq, l: the fp32 values that were quantised, 0 where the pixel does not
                count) and 'counted' uint8 [N,H,W]
      shift     None: eval_shift(N * H * W); a caller that pools the rows of several calls passes the shift of all its pixels
    Integer atomics only: the same inputs give the same bits for any grid.  No device tensor is read back."""
    what = 'depth_score'
    pred, gt = _dev32(pred, 'pred'), _dev32(gt, 'gt')
    if pred.dim() != 4 or pred.shape[1] != 1 or pred.shape != gt.shape or pred.device != gt.device or pred.numel() == 0:
        raise RuntimeError('%s: pred and gt must be non-empty [N,1,H,W] tensors of one shape on one device, got %s and %s' % (
            what, tuple(pred.shape), tuple(gt.shape)))
    N, _, H, W = (int(v) for v in pred.shape)
    dev = pred.device
    scale = _dev32(scale, 'scale')
    if scale.device != dev or tuple(scale.shape) != (N,):
        raise RuntimeError('%s: scale must be a GPU float32 tensor [%d] on the device of pred, got %s' % (what, N, tuple(scale.shape)))
    if seg is not None:
        seg = _dev32(seg, 'seg')
        if seg.device != dev or tuple(seg.shape) != (N, H, W):
            raise RuntimeError('%s: seg must be [%d,%d,%d] on the device of pred, got %s' % (what, N, H, W, tuple(seg.shape)))
    mask = _dev_u8(what, 'mask', mask, (N, H, W), dev)
    g_min = _real_arg(what, 'g_min', float(g_min))
    if N > 65535 or H * W >= 2 ** 30:
        raise RuntimeError('%s: N=%d frames of %dx%d: N <= 65535 and H * W < 2^30 are required' % (what, N, H, W))
    limit = eval_shift(N * H * W)      # (for all the pixels of the call)
    shift = limit if shift is None else _int_arg(what, 'shift', shift, 1, limit)
    if sums is None:
        sums = torch.zeros((N, 3, 9), device=dev, dtype=torch.int64)
    else:
        _out_ok(what, 'sums', sums, (N, 3, 9), torch.int64, dev, 'pred')
    point_maps = counted = None
    if maps is True:
        point_maps = torch.empty((N, 3, H, W), device=dev, dtype=torch.float32)
        counted = torch.empty((N, H, W), device=dev, dtype=torch.uint8)
    elif maps not in (False, None):
        raise RuntimeError('%s: maps must be True or False' % what)
    _lib.check(_lib.load().dvd_depth_score(_p(pred), _p(gt), _p(scale), _p(seg), _p(mask), g_min, shift, _p(sums), _p(point_maps),
                                           _p(counted), N, H, W, _stream()), 'dvd_depth_score')
    res = {'sums': sums, 'shift': shift}
    if point_maps is not None:
        res['maps'], res['counted'] = point_maps, counted
    return res


# -- max|x| scalars ----------------------------------------------------------------------------------------------------
# Every tensor that feeds a matrix kernel carries max|x| (or an upper bound) in a 1-element GPU tensor: the kernels derive
# the power-of-two scale of their fp16 operand split from it on the device (csrc/dvd_split.h); the host never reads it.
# The scalar hangs on the tensor OBJECT together with the tensor's version counter (an in-place update invalidates it)
# and the capture context it was computed in.
_capture_state = [0, False, False]     # [capture generation, the previous _capture_gen() call was inside a capture, announced]


def begin_capture():
    """Call right before every `torch.cuda.graph(...)`: opens a new capture generation.  Scalars (and scalar-pool chunks)
    of one capture are never continued by another -- a chunk lives in the private pool of the graph that allocated it and
    its zero-fill node replays with THAT graph only (round 3 inferred the boundary from an eager call happening between two
    captures; back-to-back captures of two kept slots then shared a chunk: slot N+1's scalars were zeroed by slot N's
    replay, or never)."""
    _capture_state[0] += 1
    _capture_state[2] = True
    return _capture_state[0]


def _capture_gen():
    """0 outside a capture; inside one, the capture's generation.  A scalar computed eagerly must never be baked into a
    graph (the replay would scale new data with the warm-up pass's maximum), and a scalar that lives in a graph's private
    pool must not be used outside it.  The generation is opened by begin_capture() -- and, for a capture nobody announced
    (tests, tools, future capture sites: ADVICE round 4), by the first call made inside a capture after a call made outside
    one: the two mechanisms together leave only back-to-back unannounced captures with no eager call in between sharing
    a generation."""
    st = _capture_state
    if not torch.cuda.is_current_stream_capturing():
        st[1] = False
        return 0
    if not st[1] and not st[2]:         # first call inside a capture nobody announced: a generation of its own all the same
        st[0] += 1
    # the announcement is consumed by EVERY in-capture call (two announced captures back to back, with no eager
    # call in between, left it set -- the next unannounced capture then shared the second one's generation and pool chunk)
    st[2] = False
    st[1] = True
    return st[0]


_scalar_pool = {}        # (device index, capture generation) -> [zeroed chunk, next free element]


def new_scalar(device):
    """A zeroed 1-element GPU tensor for a max|.| scalar.  Scalars are handed out from zero-filled chunks of 512 (one fill
    launch per 512 instead of one per scalar: a MiDaS step needs ~800 of them); a chunk belongs to the capture context it
    was allocated in (inside a HIP graph the fill is part of the graph, so every replay starts from zeros again)."""
    gen = _capture_gen()
    key = (torch.device(device).index or 0, gen)
    for k in [k for k in _scalar_pool if k[1] not in (0, gen)]:       # chunks of finished captures: their graphs own them
        del _scalar_pool[k]
    ent = _scalar_pool.get(key)
    if ent is None or ent[1] >= ent[0].numel():
        ent = [torch.zeros(512, device=device, dtype=torch.float32), 0]
        _scalar_pool[key] = ent
    out = ent[0][ent[1]:ent[1] + 1]
    ent[1] += 1
    return out


_AMAX_LOG = {} if os.environ.get('DVD_AMAX_LOG') else None      # developer aid: who still needs a reduction pass (printed at exit)
if _AMAX_LOG is not None:
    import atexit
    import traceback

    def _amax_report():
        for k, n in sorted(_AMAX_LOG.items(), key=lambda kv: -kv[1]):
            print('amax x%d %s' % (n, k), file=sys.stderr)
    atexit.register(_amax_report)


def amax(t):
    """max|t| by the reduction kernel (one read of the tensor) -> 1-element GPU tensor."""
    t = _dev32(t, 'tensor')
    if _AMAX_LOG is not None:
        fr = traceback.extract_stack(limit=6)[:-1]
        key = (tuple(t.shape), ' < '.join('%s:%d' % (f.name, f.lineno) for f in reversed(fr)))
        _AMAX_LOG[key] = _AMAX_LOG.get(key, 0) + 1
    out = new_scalar(t.device)
    if t.numel():
        _lib.check(_lib.load().dvd_amax(_p(t), ctypes.c_longlong(t.numel()), _p(out), _stream()), 'dvd_amax')
    return out


def chansum(t, want_amax=False):
    """Per-channel sums of an NCHW fp32 tensor (a convolution's bias gradient) and, if want_amax, max|t| from the same read
    (attached to t like amax_of would) -> [C] tensor."""
    t = _dev32(t, 'tensor')
    N, C = t.shape[0], t.shape[1]
    HW = t.numel() // max(N * C, 1)
    lib = _lib.load()
    out = torch.empty(C, device=t.device, dtype=torch.float32)
    am = new_scalar(t.device) if want_amax else None
    nws = lib.dvd_chansum_workspace_bytes(N, C)
    ws = torch.empty(max(nws, 4), device=t.device, dtype=torch.uint8)
    _lib.check(lib.dvd_chansum(_p(t), N, C, ctypes.c_longlong(HW), _p(out), _p(am) if am is not None else None, _p(ws),
                               ctypes.c_size_t(nws), _stream()), 'dvd_chansum')
    if am is not None:
        t._dvd_amax = (t._version, am, _capture_gen())
    return out


def set_amax(t, am):
    """Attach a known max|t| (or upper bound: a sub-sampled / interpolated / ReLU'd view of a bounded tensor)."""
    if am is not None:
        t._dvd_amax = (t._version, am, _capture_gen())
    return t


def known_amax(t):
    """The scalar attached to the tensor if it is still valid (same contents, same capture context), else None."""
    hit = getattr(t, '_dvd_amax', None)
    if hit is not None and hit[0] == t._version and hit[2] == _capture_gen():
        return hit[1]
    return None


def amax_of(t):
    """The tensor's max|.| scalar: the one its producer attached, else computed now and remembered."""
    am = known_amax(t)
    if am is None:
        am = amax(t)
        t._dvd_amax = (t._version, am, _capture_gen())
    return am


_ws_cache = {}


def _workspace(nbytes, device):
    if torch.cuda.is_current_stream_capturing():
        # an allocation made while a HIP graph is being captured lives in THAT graph's private pool: it must stay private
        # to the graph (a cached one would outlive the pool -- a memory-access fault in whichever model reused it after
        # the first model's graphs were destroyed)
        return torch.empty(max(nbytes, 1 << 20), device=device, dtype=torch.uint8)
    key = (device.index, torch.cuda.current_stream().cuda_stream)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 20), device=device, dtype=torch.uint8)
        _ws_cache[key] = ws
    return ws


def warp_loss_fused(cfg, depth_1, depth_2, flow_1_2, mask_2, sf_1_2, cams, grads=True, out=None):
    """One launch: the four un-normalised loss sums and, if grads, the
    un-normalised gradients w.r.t. depth_1, depth_2 and the scene flow.

    mask_2: [B,H,W] (or [B,H,W,1,1]); sf_1_2: planar [B,3,H,W].
    Returns (sums[4], g_depth_1, g_depth_2, g_sf) -- gradients None if not grads.
    `out` may pass pre-allocated (sums, g_depth_1, g_depth_2, g_sf) to avoid allocation.
    """
    depth_1, depth_2 = _dev32(depth_1, 'depth_1'), _dev32(depth_2, 'depth_2')
    flow_1_2, mask_2, sf_1_2 = _dev32(flow_1_2, 'flow_1_2'), _dev32(mask_2, 'mask_2'), _dev32(sf_1_2, 'sf_1_2')
    B, H, W = cfg.B, cfg.H, cfg.W
    if depth_1.numel() != B * H * W or depth_2.numel() != B * H * W or mask_2.numel() != B * H * W:
        raise RuntimeError('warp_loss_fused: depth/mask shape does not match cfg %dx%dx%d' % (B, H, W))
    if flow_1_2.numel() != 2 * B * H * W or sf_1_2.numel() != 3 * B * H * W:
        raise RuntimeError('warp_loss_fused: flow / scene-flow shape mismatch')
    cst, keep = pack_cameras(cams)
    dev = depth_1.device
    lib = _lib.load()
    nws = lib.dvd_warp_loss_workspace_bytes(B, H, W)
    ws = _workspace(nws, dev)
    if out is not None:
        sums, g1, g2, gs = out
    else:
        sums = torch.empty(4, device=dev, dtype=torch.float32)
        g1 = torch.empty_like(depth_1) if grads else None
        g2 = torch.empty_like(depth_2) if grads else None
        gs = torch.empty_like(sf_1_2) if grads else None
    if grads:
        st = lib.dvd_warp_loss_fused(ctypes.byref(cfg), _p(depth_1), _p(depth_2), _p(flow_1_2), _p(mask_2),
                                     _p(sf_1_2), ctypes.byref(cst), _p(ws), ws.numel(), _p(sums), _p(g1), _p(g2),
                                     _p(gs), _stream())
        _lib.check(st, 'dvd_warp_loss_fused')
    else:
        st = lib.dvd_warp_loss_fwd(ctypes.byref(cfg), _p(depth_1), _p(depth_2), _p(flow_1_2), _p(mask_2),
                                   _p(sf_1_2), ctypes.byref(cst), _p(ws), ws.numel(), _p(sums), _stream())
        _lib.check(st, 'dvd_warp_loss_fwd')
    del keep
    return sums, g1, g2, gs


FLOP_CLASSES = ('xconv_1x1_wide', 'xconv_wide', 'xconv_128', 'xconv_small', 'xwgrad3', 'xwgrad3g', 'xwgrad1b', 'xwgrad1s',
                'xwgradk', 'mlp_fwd', 'mlp_bwd_dx', 'mlp_bwd_dw')
# kernel-name fragments (mangled names of a rocprofv3 trace) of each class: tools/mfma_roofline.py joins a trace on these
FLOP_CLASS_KERNELS = {          # mangled (rocpd database) and demangled (rocprofv3 csv) spellings
    'xconv_1x1_wide': ('xconv_kernelILi4ELi2ELi2ELi2ELi11E', 'xconv_kernel<4, 2, 2, 2, 11,'),
    'xconv_wide': ('xconv_kernelILi4ELi2ELi2ELi4E', 'xconv_kernelILi4ELi2ELi2ELi2ELi0E', 'xconv_kernelILi4ELi2ELi2ELi2ELi1E',
                   'xconv_kernelILi4ELi2ELi2ELi2ELi2E', 'xconv_kernelILi4ELi2ELi2ELi2ELi3E', 'xconv_kernel<4, 2, 2, 4,',
                   'xconv_kernel<4, 2, 2, 2, 0,', 'xconv_kernel<4, 2, 2, 2, 1,', 'xconv_kernel<4, 2, 2, 2, 2,',
                   'xconv_kernel<4, 2, 2, 2, 3,'),
    'xconv_128': ('xconv_kernelILi2ELi2ELi2ELi2E', 'xconv_kernel<2, 2, 2, 2,'),
    'xconv_small': ('xconv_kernelILi1ELi2ELi1ELi4E', 'xconv_kernelILi2ELi2ELi1ELi4E', 'xconv_kernel<1, 2, 1, 4,',
                    'xconv_kernel<2, 2, 1, 4,'),
    'xwgrad3': ('xwgrad3_kernel',), 'xwgrad3g': ('xwgrad3g_kernel',), 'xwgrad1b': ('xwgrad1b_kernel',),
    'xwgrad1s': ('xwgrad1s_kernel',), 'xwgradk': ('xwgradk_kernel',),
    'mlp_fwd': ('mlp_fwd_kernel',), 'mlp_bwd_dx': ('mlp_bwd_dx_kernel',), 'mlp_bwd_dw': ('mlp_bwd_dw_kernel',),
}


# Memory-bound helper kernels (round 6; bench.py's roofline_helpers): algorithmic BYTES per class, counted by the library the
# same way (include/dvd_hip.h: dvd_byte_counters), and the kernel-name fragments tools/mfma_roofline.py joins a trace on.
# They travel through the same snapshot / replay bookkeeping as the matrix classes, under their own keys.
BYTE_CLASSES = ('bnrelu_fwd', 'bnrelu_bwd', 'upsample_fwd', 'upsample_bwd', 'amax', 'pack', 'pool', 'gconv_c8', 'elementwise',
                'adam', 'geometry', 'gather')
BYTE_CLASS_KERNELS = {
    'bnrelu_fwd': ('bnrelu_fwd_kernel',), 'bnrelu_bwd': ('bnrelu_bwd', 'bn_mask', 'bnrelu_sum'),
    'upsample_fwd': ('upsample_bilinear_fwd', 'bicubic_fwd_kernel'),
    'upsample_bwd': ('upsample_bilinear_bwd', 'upsample_bwd', 'bicubic_bwd_'),
    'amax': ('amax_kernel', 'chansum_'), 'pack': ('xconv_wamax', 'xconv_pack_kernel'), 'pool': ('maxpool3s2', 'subsample2_', 'avgpool_'),
    'gconv_c8': ('gconv3x3_c8',), 'elementwise': ('mul_mask_kernel', 'scale_add_kernel', 'acc_reg_kernel', 'sum_partials_kernel',
                                                  'head1x1_', 'cast_scale_kernel'),
    'adam': ('adam_kernel', 'sgd_kernel'), 'geometry': ('unproject_', 'track_project_kernel', 'project_bwd_kernel', 'splat_zmin_kernel', 'splat_accumulate_kernel',
                                                   'splat_resolve_kernel', 'eval_tracks_kernel', 'ratio_hist_kernel', 'ratio_pick_kernel',
                                                   'depth_score_kernel', 'track_filter_kernel', 'triangulate_kernel', 'fill_pull_kernel',
                                                   'fill_mid_kernel', 'fill_push_kernel', 'flow_chain_kernel', 'pose_normal_eq_kernel',
                                                   'pose_sum_partials_kernel'), 'gather': ('gather_pairs_kernel', 'store_gather_kernel', 'union_'),
}
ALL_CLASSES = FLOP_CLASSES + BYTE_CLASSES


def flop_counters(reset=False):
    """Algorithmic work (2 x MACs) the matrix kernels were launched with since the last reset, per kernel class
    (include/dvd_hip.h: dvd_flop_counters) -- and, under the BYTE_CLASSES keys, the algorithmic bytes of the helper kernels
    (dvd_byte_counters).  Counted at launch / graph-capture time: read it after a step that CAPTURED (or ran eagerly)
    everything a step launches."""
    lib = _lib.load()
    buf = (ctypes.c_double * len(FLOP_CLASSES))()
    _lib.check(lib.dvd_flop_counters(ctypes.cast(buf, ctypes.c_void_p), len(FLOP_CLASSES), 1 if reset else 0), 'dvd_flop_counters')
    out = dict(zip(FLOP_CLASSES, [float(v) for v in buf]))
    bbuf = (ctypes.c_double * len(BYTE_CLASSES))()
    _lib.check(lib.dvd_byte_counters(ctypes.cast(bbuf, ctypes.c_void_p), len(BYTE_CLASSES), 1 if reset else 0), 'dvd_byte_counters')
    out.update(zip(BYTE_CLASSES, [float(v) for v in bbuf]))
    return out


# work of REPLAYED HIP graphs: a graph's launches are counted once, when it is captured (flops_since around the capture);
# whoever replays it adds that record here, so that (flop_counters + REPLAYED) over a region is the work the region executed
REPLAYED = {k: 0.0 for k in ALL_CLASSES}


# work that is a RE-computation (round 6; SURVEY 8d: "recompute is not counted"): the no-graph depth-net forward of a chunk whose
# autograd state is not kept (phase 3 runs that forward again inside its forward+backward graph) and the stash-free Euler
# chain of the scene-flow MLP's recompute schedule.  Included in executed_flops(); bench.py reports the step's work with and
# without it (roofline_mfma.needed_TFLOP_per_step, frac_of_needed_work).
RECOMPUTED = {k: 0.0 for k in ALL_CLASSES}


class counting_recomputed(object):
    """with ops.counting_recomputed(): ...   -- everything launched / replayed inside is a re-computation."""

    def __enter__(self):
        self.before = executed_flops()
        return self

    def __exit__(self, *exc):
        now = executed_flops()
        for k in ALL_CLASSES:
            RECOMPUTED[k] += now[k] - self.before[k]
        return False


def flops_since(snapshot):
    now = flop_counters()
    return {k: now[k] - snapshot.get(k, 0.0) for k in ALL_CLASSES}


def note_replay(flops):
    if flops:
        for k, v in flops.items():
            REPLAYED[k] += v


def executed_flops():
    """Per kernel class: work launched eagerly plus work of replayed graphs, since process start (take differences)."""
    now = flop_counters()
    return {k: now[k] + REPLAYED[k] for k in ALL_CLASSES}


def gather_pairs(tensors, perm, out=None):
    """Batched pair permutation (dvd_gather_pairs): returns a list of new tensors with out_k[b] = tensors_k[perm[b]] for
    every tensor of `tensors` (GPU tensors of any dtype that share their first dimension B), ONE launch per
    _lib.GATHER_MAX tensors.  perm: a GPU integer tensor of B indices in [0, B) (int32 is used as it is), or a host
    sequence of ints.  out: optional list of destination tensors (same shapes and dtypes, no overlap with the sources)."""
    tensors = list(tensors)
    if not tensors:
        return []
    B = int(tensors[0].shape[0]) if (torch.is_tensor(tensors[0]) and tensors[0].dim() > 0) else 0
    srcs = []
    for i, t in enumerate(tensors):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise RuntimeError('gather_pairs: tensor %d must be a GPU tensor (dvd_hip has no CPU path)' % i)
        if t.dim() < 1 or t.shape[0] != B or t.numel() == 0:
            raise RuntimeError('gather_pairs: tensor %d has shape %s, expected %d pairs in dim 0' % (i, tuple(t.shape), B))
        srcs.append(t if t.is_contiguous() else t.contiguous())
    if not torch.is_tensor(perm):
        idx = [int(i) for i in perm]
        if len(idx) != B or any(i < 0 or i >= B for i in idx):
            raise RuntimeError('gather_pairs: perm must hold %d indices in [0, %d)' % (B, B))
        perm = torch.tensor(idx, dtype=torch.int32).to(tensors[0].device, non_blocking=True)
    if not perm.is_cuda or perm.numel() != B or perm.dtype not in (torch.int32, torch.int64):
        raise RuntimeError('gather_pairs: perm must be a GPU int32 / int64 tensor of %d indices' % B)
    perm = perm.to(torch.int32).contiguous()
    if out is None:
        out = [torch.empty_like(t) for t in srcs]
    else:
        out = list(out)
        if len(out) != len(srcs) or any(o.shape != t.shape or o.dtype != t.dtype or not o.is_cuda or not o.is_contiguous()
                                        for o, t in zip(out, srcs)):
            raise RuntimeError('gather_pairs: out must match the sources in number, shape and dtype (contiguous GPU tensors)')
    lib = _lib.load()
    for k0 in range(0, len(srcs), _lib.GATHER_MAX):
        part = list(zip(srcs[k0:k0 + _lib.GATHER_MAX], out[k0:k0 + _lib.GATHER_MAX]))
        items = (_lib.GatherItem * len(part))()
        for it, (t, o) in zip(items, part):
            it.src, it.dst, it.bytes_per_pair = t.data_ptr(), o.data_ptr(), t.numel() // B * t.element_size()
        _lib.check(lib.dvd_gather_pairs(items, len(part), _p(perm), B, _stream()), 'dvd_gather_pairs')
    return out


STORE_OPS = {'copy': _lib.STORE_COPY, 'mask': _lib.STORE_MASK, 'fill': _lib.STORE_FILL}


def store_gather(entries, index, host_index=None):
    """Batch assembly out of a device-resident frame store (dvd_store_gather; datasets/frame_store.py): for every entry
    (src, dst, op, row), dst[b] = op(src[index[row][b]]) for b < B = dst.shape[0], ONE launch per _lib.STORE_MAX entries.
      op 'copy'  src [rows, ...] and dst [B, ...] of one dtype and the same bytes per row;
      op 'mask'  src uint8 [rows, ...], dst fp32 [B, ...] with as many elements per row: dst = 1 - src;
      op 'fill'  src fp32 [rows], dst fp32 [B, ...]: every element of dst[b] is the scalar src[index[row][b]].
    index: three rows (first frame, second frame, flow pair) of B ints -- a host array (numpy, CPU tensor, nested lists),
    uploaded here, or a GPU int32 tensor [3, B] whose rows may be strided (a column slice of an epoch's [3, total]); then
    host_index, its host copy, saves the read-back that checking the ranges needs otherwise.  Everything is checked on the
    host -- devices, dtypes, contiguity, sizes, every index against the rows of the tables it selects from -- and a
    RuntimeError is raised before anything is launched."""
    import numpy as np
    entries = list(entries)
    if not entries:
        raise RuntimeError('store_gather: no entries')
    B = int(entries[0][1].shape[0]) if (torch.is_tensor(entries[0][1]) and entries[0][1].dim() > 0) else 0
    if B <= 0:
        raise RuntimeError('store_gather: an empty batch')
    if torch.is_tensor(index) and index.is_cuda:
        if index.dtype != torch.int32 or index.dim() != 2 or tuple(index.shape) != (3, B) or index.stride(1) != 1 or \
                index.stride(0) < B:
            raise RuntimeError('store_gather: index must be a GPU int32 tensor [3, %d] with contiguous rows' % B)
        host = np.asarray(index.cpu() if host_index is None else host_index)
    else:
        host = np.asarray(index.cpu() if torch.is_tensor(index) else index)
        index = None
    if host.shape != (3, B) or host.dtype.kind not in 'iu':
        raise RuntimeError('store_gather: index must hold three rows of %d integers, got %s %s' % (B, host.dtype, host.shape))
    lo, hi = host.min(axis=1), host.max(axis=1)
    items = []
    for i, (src, dst, op, row) in enumerate(entries):
        if op not in STORE_OPS or row not in (0, 1, 2):
            raise RuntimeError('store_gather: entry %d: operation %r / index row %r' % (i, op, row))
        if not (torch.is_tensor(src) and src.is_cuda and torch.is_tensor(dst) and dst.is_cuda):
            raise RuntimeError('store_gather: entry %d must name GPU tensors (dvd_hip has no CPU path)' % i)
        if src.device != dst.device:
            raise RuntimeError('store_gather: entry %d: source and destination on different devices' % i)
        if not dst.is_contiguous() or not src.is_contiguous():
            raise RuntimeError('store_gather: entry %d: source and destination must be contiguous' % i)
        if dst.dim() < 1 or dst.shape[0] != B or dst.numel() == 0 or src.dim() < 1 or src.numel() == 0:
            raise RuntimeError('store_gather: entry %d: destination %s / source %s for %d pairs' % (
                i, tuple(dst.shape), tuple(src.shape), B))
        rows, per_row = int(src.shape[0]), dst.numel() // B
        if op == 'copy':
            if src.dtype != dst.dtype:
                raise RuntimeError('store_gather: entry %d: copy of dtype %s into %s' % (i, src.dtype, dst.dtype))
            if src.numel() // rows != per_row:
                raise RuntimeError('store_gather: entry %d: size mismatch, a source row holds %d elements, a destination row %d'
                                   % (i, src.numel() // rows, per_row))
        elif op == 'mask':
            if src.dtype != torch.uint8 or dst.dtype != torch.float32:
                raise RuntimeError('store_gather: entry %d: mask wants dtype uint8 -> float32, got %s -> %s' % (i, src.dtype, dst.dtype))
            if src.numel() // rows != per_row:
                raise RuntimeError('store_gather: entry %d: size mismatch, a source row holds %d elements, a destination row %d'
                                   % (i, src.numel() // rows, per_row))
        else:
            if src.dtype != torch.float32 or dst.dtype != torch.float32:
                raise RuntimeError('store_gather: entry %d: fill wants dtype float32, got %s -> %s' % (i, src.dtype, dst.dtype))
            if src.dim() != 1:
                raise RuntimeError('store_gather: entry %d: size mismatch, fill takes one scalar per table row, got %s' % (
                    i, tuple(src.shape)))
        if lo[row] < 0 or hi[row] >= rows:
            raise RuntimeError('store_gather: entry %d: index row %d spans [%d, %d], outside its table of %d rows' % (
                i, row, int(lo[row]), int(hi[row]), rows))
        items.append((src, dst, per_row * dst.element_size(), rows, row, STORE_OPS[op]))
    if index is None:
        index = torch.from_numpy(np.ascontiguousarray(host.astype(np.int32))).to(entries[0][1].device)
    lib = _lib.load()
    stride = int(index.stride(0))
    for k0 in range(0, len(items), _lib.STORE_MAX):
        part = items[k0:k0 + _lib.STORE_MAX]
        arr = (_lib.StoreItem * len(part))()
        for it, (src, dst, bpr, rows, row, op) in zip(arr, part):
            it.src, it.dst, it.bytes_per_row, it.src_rows, it.index_row, it.op, it.pad = src.data_ptr(), dst.data_ptr(), bpr, rows, row, op, 0
        _lib.check(lib.dvd_store_gather(arr, len(part), _p(index), stride, B, _stream()), 'dvd_store_gather')


class UnionTables(object):
    """The index tables of a step that shares frames (models/frame_union.py: plan_union), as ONE int32 device tensor
    [set | row | u1 | u2 | offsets | entries] uploaded once, its host copy, and a view per part.  The union_* wrappers check
    every index of the part they use against the host copy before they launch."""

    def __init__(self, plan, device):
        from .models import frame_union
        self.plan, self.B, self.U, self.U_pad = plan, int(plan['B']), int(plan['U']), int(plan['U_pad'])
        self.host, self.where = frame_union.table(plan)
        self.dev = torch.from_numpy(self.host).to(device, non_blocking=True)

    def part(self, name):
        o, n = self.where[name]
        return self.dev[o:o + n]

    def host_part(self, name):
        o, n = self.where[name]
        return self.host[o:o + n]

    def check(self, what, name, lo, hi):
        v = self.host_part(name)
        if v.size and (int(v.min()) < lo or int(v.max()) >= hi):
            raise RuntimeError('%s: table %r spans [%d, %d], outside [%d, %d)' % (what, name, int(v.min()), int(v.max()), lo, hi))


def _union_rows(what, t, rows, name, dtype=None):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError('%s: %s must be a GPU tensor (dvd_hip has no CPU path)' % (what, name))
    if t.dim() < 1 or t.shape[0] != rows or t.numel() == 0 or not t.is_contiguous():
        raise RuntimeError('%s: %s must be a contiguous tensor of %d rows, got %s' % (what, name, rows, tuple(t.shape)))
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError('%s: %s must be %s, got %s' % (what, name, dtype, t.dtype))
    bpr = t.numel() // rows * t.element_size()
    if bpr % 4 or t.data_ptr() % 4:
        raise RuntimeError('%s: %s: rows of %d bytes at a %d-byte offset; rows are moved as dwords' % (
            what, name, bpr, t.data_ptr() % 4))
    return bpr


def union_gather(img_1, img_2, tab, out=None):
    """out[u] = (set[u] ? img_2 : img_1)[row[u]] for the U_pad union rows of `tab` (dvd_union_gather): the distinct frames of a
    step, padding rows being copies of union row 0.  img_1, img_2: contiguous GPU tensors [B, ...] of one shape and dtype."""
    B, U_pad = tab.B, tab.U_pad
    bpr = _union_rows('union_gather', img_1, B, 'img_1')
    if img_2.shape != img_1.shape or img_2.dtype != img_1.dtype or _union_rows('union_gather', img_2, B, 'img_2') != bpr:
        raise RuntimeError('union_gather: the two image sets differ in shape or dtype')
    tab.check('union_gather', 'set', 0, 2)
    tab.check('union_gather', 'row', 0, B)
    if out is None:
        out = torch.empty((U_pad,) + tuple(img_1.shape[1:]), device=img_1.device, dtype=img_1.dtype)
    elif out.dtype != img_1.dtype or _union_rows('union_gather', out, U_pad, 'out') != bpr:
        raise RuntimeError('union_gather: out must hold %d rows like the sources\'' % U_pad)
    _lib.check(_lib.load().dvd_union_gather(_p(img_1), _p(img_2), _p(out), _p(tab.part('set')), _p(tab.part('row')), U_pad, B,
                                            bpr, _stream()), 'dvd_union_gather')
    return out


def union_scatter(D, tab, out=None):
    """(depth_1, depth_2) with depth_1[b] = D[u1[b]], depth_2[b] = D[u2[b]] in ONE launch (dvd_union_scatter).  D: contiguous
    GPU tensor [U_pad, ...]; out: optional pair of destinations [B, ...]."""
    B, U_pad = tab.B, tab.U_pad
    bpr = _union_rows('union_scatter', D, U_pad, 'D')
    tab.check('union_scatter', 'u1', 0, U_pad)
    tab.check('union_scatter', 'u2', 0, U_pad)
    if out is None:
        out = tuple(torch.empty((B,) + tuple(D.shape[1:]), device=D.device, dtype=D.dtype) for _ in range(2))
    elif len(out) != 2 or any(o.dtype != D.dtype or _union_rows('union_scatter', o, B, 'out') != bpr for o in out):
        raise RuntimeError('union_scatter: out must be two tensors of %d rows like D\'s' % B)
    _lib.check(_lib.load().dvd_union_scatter(_p(D), _p(out[0]), _p(out[1]), _p(tab.part('u1')), _p(tab.part('u2')), B, U_pad, bpr,
                                             _stream()), 'dvd_union_scatter')
    return out[0], out[1]


def union_reduce(g_d1, g_d2, tab, out=None):
    """G[u] = the sum of the depth gradients of every image that shows union row u: 0 + g[e_0] + g[e_1] + ... over the row's CSR
    entries in list order, plain fp32 adds, no atomics (dvd_union_reduce); padding rows are zero.  g_d1, g_d2: fp32 [B, ...]."""
    B, U_pad = tab.B, tab.U_pad
    bpr = _union_rows('union_reduce', g_d1, B, 'g_d1', torch.float32)
    if g_d2.shape != g_d1.shape or _union_rows('union_reduce', g_d2, B, 'g_d2', torch.float32) != bpr:
        raise RuntimeError('union_reduce: the two gradient sets differ in shape')
    tab.check('union_reduce', 'offsets', 0, 2 * B + 1)
    tab.check('union_reduce', 'entries', 0, 2 * B)
    off = tab.host_part('offsets')
    if off[0] != 0 or (off[1:] < off[:-1]).any():
        raise RuntimeError('union_reduce: offsets must start at 0 and not decrease')
    if out is None:
        out = torch.empty((U_pad,) + tuple(g_d1.shape[1:]), device=g_d1.device, dtype=torch.float32)
    elif _union_rows('union_reduce', out, U_pad, 'out', torch.float32) != bpr:
        raise RuntimeError('union_reduce: out must hold %d rows like the sources\'' % U_pad)
    _lib.check(_lib.load().dvd_union_reduce(_p(g_d1), _p(g_d2), _p(out), _p(tab.part('offsets')), _p(tab.part('entries')), U_pad,
                                            B, bpr // 4, _stream()), 'dvd_union_reduce')
    return out


class _BicubicResize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, size, mean, std):
        N, C, H, W = x.shape
        Ho, Wo = size
        y = torch.empty(N, C, Ho, Wo, device=x.device, dtype=torch.float32)
        _lib.check(_lib.load().dvd_bicubic_fwd(_p(x), _p(y), N * C, H, W, Ho, Wo, _p(mean), _p(std), C, _stream()), 'dvd_bicubic_fwd')
        ctx.shape = (N, C, H, W, Ho, Wo)
        return y

    @staticmethod
    def backward(ctx, gy):
        N, C, H, W, Ho, Wo = ctx.shape
        gy = _dev32(gy, 'gy')
        lib = _lib.load()
        gx = torch.empty(N, C, H, W, device=gy.device, dtype=torch.float32)
        # (a plain allocation, not the cached workspace: its size follows the shape, and inside a graph capture it belongs to
        #  the graph's pool either way)
        ws = torch.empty(max(1, lib.dvd_bicubic_bwd_workspace_bytes(N * C, H, W, Ho, Wo)), device=gy.device, dtype=torch.uint8)
        _lib.check(lib.dvd_bicubic_bwd(_p(gy), _p(gx), N * C, H, W, Ho, Wo, _p(ws), ws.numel(), _stream()), 'dvd_bicubic_bwd')
        return gx, None, None, None


def bicubic_resize(x, size, mean=None, std=None):
    """F.interpolate(x, size=size, mode='bicubic', align_corners=True) of an fp32 GPU tensor [N,C,H,W] (csrc/bicubic.hip),
    differentiable in x.  mean / std (GPU fp32 tensors of C values, both or neither): the resize of (x - mean[c]) / std[c] in
    one pass -- MidasNet's input normalisation fused into its input resize; that form has no gradient (an image needs none)."""
    x = _dev32(x, 'x')
    if x.dim() != 4 or x.numel() == 0:
        raise RuntimeError('bicubic_resize: x must be a non-empty [N,C,H,W] tensor, got shape %s' % (tuple(x.shape),))
    Ho, Wo = (int(v) for v in size)
    if Ho <= 0 or Wo <= 0:
        raise RuntimeError('bicubic_resize: size must be positive, got %s' % ((Ho, Wo),))
    if (mean is None) != (std is None):
        raise RuntimeError('bicubic_resize: mean and std go together')
    if mean is not None:
        mean, std = _dev32(mean, 'mean'), _dev32(std, 'std')
        if mean.numel() != x.shape[1] or std.numel() != x.shape[1] or mean.device != x.device or std.device != x.device:
            raise RuntimeError('bicubic_resize: mean / std must hold one value per channel (%d) on the device of x' % x.shape[1])
        if x.requires_grad:
            raise RuntimeError('bicubic_resize: the normalising form has no backward (x must not require a gradient)')
    return _BicubicResize.apply(x, (Ho, Wo), mean, std)


def warp_loss_select(variant='tiled', tile=-1, px=0, strip_rows=0, strip_shape=0):
    """Test hook: run dvd_warp_loss_fused on another variant -- 'tiled' = production (the strip kernel where it applies, at
    tile = -1), 'direct' = global gathers + hardware atomics, 'tiles' = the tile kernel of rounds 2-5 whatever the
    call -- tile shape, rows per strip unit or strip shape (csrc/warp_strip.hip kStripShapes).  `px` is reserved like the
    third argument of dvd_warp_loss_select: callers that still pass px=0 keep working, any other value is rejected by the
    library (pixels per thread-step are fixed by the tile shape).  Process wide; call warp_loss_select() to restore
    the production path."""
    lib = _lib.load()
    _lib.check(lib.dvd_warp_loss_select({'tiled': 0, 'direct': 1, 'tiles': 2}[variant], int(tile), int(px)), 'dvd_warp_loss_select')
    _lib.check(lib.dvd_warp_loss_strip_select(int(strip_rows), int(strip_shape)), 'dvd_warp_loss_strip_select')


def loss_finalize(cfg, sums, out=None):
    """scalars[8]: [0]=1/(S0+1e-8) [1]=loss [2]=flow [3]=disp [4]=sf [5]=S0."""
    sums = _dev32(sums, 'sums')
    if out is None:
        out = torch.empty(8, device=sums.device, dtype=torch.float32)
    lib = _lib.load()
    _lib.check(lib.dvd_loss_finalize(ctypes.byref(cfg), _p(sums), _p(out), _stream()), 'dvd_loss_finalize')
    return out


_SURFACE_SHAPES = {'global_p1': 3, 'warped_global_p2': 3, 'sf_by_depth': 3, 'p1_camera_2': 3, 'warped_p2_camera_2': 3,
                   'staticflow_1_2': 2, 'dflow_1_2': 2, 'depth_image_1_2': 1, 'depth_warp_1_2': 1}


def _surface_shape(k, B, H, W):
    c = _SURFACE_SHAPES[k]
    return (B, H, W, 1, 3) if c == 3 else ((B, H, W, 2) if c == 2 else (B, 1, H, W))


def _surface_inputs(what, depth_1, depth_2, flow_1_2, sflow_1_2, cams, more=()):
    """The inputs the surface kernel and its backward share, checked against the B, H, W of depth_1 -> (B, H, W, the tensors,
    the camera struct, what to keep alive); `more`: further (name, tensor, shapes(B, H, W)) of the same call."""
    B, H, W = _image_size(what, 'depth_1', depth_1)
    ts = _images(what, [('depth_1', depth_1, ((B, 1, H, W),)), ('depth_2', depth_2, ((B, 1, H, W),)),
                        ('flow_1_2', flow_1_2, ((B, H, W, 2),)), ('sflow_1_2', sflow_1_2, ((B, H, W, 1, 3),))] +
                 [(name, t, shapes(B, H, W)) for name, t, shapes in more] + _camera_specs(what, cams, B))
    keep = ts[-len(CAM_KEYS):]
    return B, H, W, ts[:-len(CAM_KEYS)], _camera_struct(keep), keep


def warp_surfaces(depth_1, depth_2, flow_1_2, cams, sflow_1_2=None, want=_lib.SURFACE_KEYS):
    """The per-pixel surfaces of flow_by_depth / scene_flow_projection_slack (forward values).
    Returns a dict name -> tensor: 3-vectors [B,H,W,1,3], flows [B,H,W,2], depths [B,1,H,W]."""
    want = tuple(want)
    for k in want:
        if k not in _SURFACE_SHAPES:
            raise RuntimeError('warp_surfaces: want holds %r, the surfaces are %s' % (k, ', '.join(_lib.SURFACE_KEYS)))
    B, H, W, (depth_1, depth_2, flow_1_2, sflow_1_2), cst, keep = _surface_inputs('warp_surfaces', depth_1, depth_2, flow_1_2,
                                                                                  sflow_1_2, cams)
    out, st = {}, _lib.Surfaces()
    for k in want:
        out[k] = torch.empty(_surface_shape(k, B, H, W), device=depth_1.device, dtype=torch.float32)
        setattr(st, k, out[k].data_ptr())
    lib = _lib.load()
    _lib.check(lib.dvd_warp_surfaces(_p(depth_1), _p(depth_2), _p(flow_1_2), _p(sflow_1_2), ctypes.byref(cst),
                                     ctypes.byref(st), B, H, W, _stream()), 'dvd_warp_surfaces')
    del keep
    return out


def warp_surfaces_backward(depth_1, depth_2, flow_1_2, cams, grads, sflow_1_2=None, want_sflow_grad=False):
    """VJP of warp_surfaces: `grads` maps surface name -> upstream gradient (same layout as the surface; missing / None =
    no gradient).  Returns (g_depth_1, g_depth_2, g_sflow_1_2 | None)."""
    what = 'warp_surfaces_backward'
    for k in grads:
        if k not in _SURFACE_SHAPES:
            raise RuntimeError('%s: grads holds %r, the surfaces are %s' % (what, k, ', '.join(_lib.SURFACE_KEYS)))
    names = [k for k in _lib.SURFACE_KEYS if grads.get(k) is not None]
    B, H, W, ts, cst, keep = _surface_inputs(what, depth_1, depth_2, flow_1_2, sflow_1_2, cams, [
        ('the gradient of ' + k, grads[k], lambda B, H, W, k=k: (_surface_shape(k, B, H, W),)) for k in names])
    depth_1, depth_2, flow_1_2, sflow_1_2 = ts[:4]
    st = _lib.Surfaces()
    for k, g in zip(names, ts[4:]):
        keep.append(g)
        setattr(st, k, g.data_ptr())
    g1, g2 = torch.empty_like(depth_1), torch.empty_like(depth_2)
    gs = torch.empty(B, H, W, 1, 3, device=depth_1.device, dtype=torch.float32) if want_sflow_grad else None
    _lib.check(_lib.load().dvd_warp_surfaces_bwd(_p(depth_1), _p(depth_2), _p(flow_1_2), _p(sflow_1_2), ctypes.byref(cst),
                                                 ctypes.byref(st), _p(g1), _p(g2), _p(gs), B, H, W, _stream()),
               'dvd_warp_surfaces_bwd')
    del keep
    return g1, g2, gs


def _warp_args(what, name, buffer, flow_1_2):
    if not torch.is_tensor(buffer) or buffer.dim() != 4 or buffer.numel() == 0:
        raise RuntimeError('%s: %s must be a tensor [B,C,H,W], got %s' % (
            what, name, tuple(buffer.shape) if torch.is_tensor(buffer) else type(buffer).__name__))
    B, C, H, W = (int(v) for v in buffer.shape)
    buffer, flow_1_2 = _images(what, [(name, buffer, ((B, C, H, W),)), ('flow_1_2', flow_1_2, ((B, H, W, 2),))])
    return buffer, flow_1_2, B, C, H, W


def flow_warp(buffer, flow_1_2):
    buffer, flow_1_2, B, C, H, W = _warp_args('flow_warp', 'buffer', buffer, flow_1_2)
    out = torch.empty_like(buffer)
    lib = _lib.load()
    _lib.check(lib.dvd_flow_warp_fwd(_p(buffer), _p(flow_1_2), _p(out), B, C, H, W, _stream()), 'dvd_flow_warp_fwd')
    return out


def flow_warp_backward(g_out, flow_1_2):
    g_out, flow_1_2, B, C, H, W = _warp_args('flow_warp_backward', 'g_out', g_out, flow_1_2)
    g = torch.empty_like(g_out)
    lib = _lib.load()
    _lib.check(lib.dvd_flow_warp_bwd(_p(g_out), _p(flow_1_2), _p(g), B, C, H, W, _stream()), 'dvd_flow_warp_bwd')
    return g


# ---------------------------------------------------------------------------------------
# scene-flow field MLP


def embed_frequencies(n_freq):
    """PeriodicEmbed(max_freq=N, N_freq=N).freqs, exactly as the reference builds them
    (torch.linspace(1, N + 1, N), networks/blocks.py:24)."""
    return torch.linspace(1, n_freq + 1, steps=n_freq)


class SceneFlowMLPKernels(object):
    """Host-side handle of the fused MLP kernels for one network configuration:
    owns the frequency tables, the packed-weight buffer and the scratch stashes."""

    def __init__(self, device, n_freq_xyz=16, n_freq_t=16, time_dependent=True, stash_f16=False):
        if torch.device(device).type != 'cuda':
            raise RuntimeError('SceneFlowMLPKernels needs a GPU device (dvd_hip has no CPU path)')
        self.device = torch.device(device)
        self.n_freq_xyz, self.n_freq_t, self.time_dependent = int(n_freq_xyz), int(n_freq_t), bool(time_dependent)
        self.fx = embed_frequencies(self.n_freq_xyz).to(self.device) if self.n_freq_xyz > 0 else None
        self.ft = embed_frequencies(self.n_freq_t).to(self.device) if (self.time_dependent and self.n_freq_t > 0) else None
        # stash_f16: the five hidden activations of the stash as fp16 (3.2 instead of 5.7 KB per pixel-evaluation; only the
        # weight gradients see the rounding -- include/dvd_hip.h, dvd_mlp_desc)
        self.stash_f16 = bool(stash_f16)
        self.desc = _lib.MlpDesc(self.n_freq_xyz, self.n_freq_t, int(self.time_dependent),
                                 self.fx.data_ptr() if self.fx is not None else 0,
                                 self.ft.data_ptr() if self.ft is not None else 0, int(self.stash_f16), 0)
        self._monitor = None
        lib = _lib.load()
        self.c_in = lib.dvd_sf_mlp_in_channels(ctypes.byref(self.desc))
        self.packed = torch.empty(lib.dvd_sf_mlp_packed_bytes(ctypes.byref(self.desc)) // 4, device=self.device,
                                  dtype=torch.float32)

    def set_forward_monitor(self, monitor):
        """fp16 stash: the 1-element device tensor (slot [6] of a model's loss-scale state) that every stashing forward folds
        max |hidden activation| into -- an activation beyond fp16's range would be stashed as Inf and poison the weight
        gradients; the step's overflow guard (csrc/a16.hip dvd_gscale_end) then skips the step.  None: no guard."""
        self._monitor = monitor                      # (kept alive: the descriptor holds its address)
        self.desc.fwd_monitor = monitor.data_ptr() if monitor is not None else 0

    # -- sizes
    def stash_floats(self, n_pix):
        return _lib.load().dvd_sf_mlp_stash_bytes(ctypes.byref(self.desc), int(n_pix)) // 4

    def gstash_floats(self, n_pix):
        return _lib.load().dvd_sf_mlp_gstash_bytes(int(n_pix)) // 4

    def new_stash(self, n_pix):
        return torch.empty(self.stash_floats(n_pix), device=self.device, dtype=torch.float32)

    def new_gstash(self, n_pix):
        return torch.empty(self.gstash_floats(n_pix), device=self.device, dtype=torch.float32)

    # -- kernels
    def pack(self, weights, biases):
        """weights: six tensors [out,in,1,1] (or [out,in]); biases: six [out]."""
        ws = [_dev32(w.detach(), 'weight') for w in weights]
        bs = [_dev32(b.detach(), 'bias') for b in biases]
        if len(ws) != 6 or len(bs) != 6:
            raise RuntimeError('the fused MLP has exactly 6 conv layers (n_layers=4)')
        dims = [self.c_in] + [256] * 5
        for i, w in enumerate(ws):
            o = 256 if i < 5 else 3
            if w.numel() != o * dims[i] or bs[i].numel() != o:
                raise RuntimeError('layer %d: expected weight %dx%d, got %s' % (i, o, dims[i], tuple(w.shape)))
        W = _lib.PtrArr6(*[w.data_ptr() for w in ws])
        Bp = _lib.PtrArr6(*[b.data_ptr() for b in bs])
        lib = _lib.load()
        _lib.check(lib.dvd_sf_mlp_pack(ctypes.byref(self.desc), ctypes.byref(W), ctypes.byref(Bp), _p(self.packed),
                                       _stream()), 'dvd_sf_mlp_pack')

    def forward(self, p, t, t_offset=0.0, out_scale=1.0, sf_out=None, p_next=None, acc=None, stash=None):
        p = _dev32(p, 'p')
        B, C, H, W = p.shape
        if C != 3:
            raise RuntimeError('p must be [B,3,H,W]')
        if self.time_dependent:
            if t is None:
                raise ValueError('time dependent scene-flow field needs t')
            t = _dev32(t, 't')
            if t.numel() != B * H * W:
                raise RuntimeError('t must be [B,1,H,W]')
        n_pix = B * H * W
        if stash is not None and stash.numel() < self.stash_floats(n_pix):
            raise RuntimeError('stash too small')
        lib = _lib.load()
        _lib.check(lib.dvd_sf_mlp_fwd(ctypes.byref(self.desc), _p(self.packed), _p(p),
                                      _p(t) if self.time_dependent else ctypes.c_void_p(0), float(t_offset),
                                      float(out_scale), n_pix, H * W, _p(sf_out), _p(p_next), _p(acc), _p(stash),
                                      _stream()), 'dvd_sf_mlp_fwd')

    def backward_dx(self, stash, out_scale, g_out1, g_p, gstash, gW5, gb5, shape, gscale=1.0, scale_ptr=None,
                    g_out2=None, g_p_add=None):
        B, H, W = shape
        n_pix = B * H * W
        lib = _lib.load()
        _lib.check(lib.dvd_sf_mlp_bwd_dx(ctypes.byref(self.desc), _p(self.packed), _p(stash), float(out_scale),
                                         _p(g_out1), float(gscale), _p(scale_ptr), _p(g_out2), _p(g_p_add), n_pix,
                                         H * W, _p(g_p), _p(gstash), _p(gW5), _p(gb5), _stream()),
                   'dvd_sf_mlp_bwd_dx')

    def backward_dw(self, stash, gstash, n_pix, gW, gb):
        """Accumulates into gW[0..4] ([256,in]) and gb[0..4] ([256])."""
        W = _lib.PtrArr5(*[g.data_ptr() for g in gW])
        Bp = _lib.PtrArr5(*[g.data_ptr() for g in gb])
        lib = _lib.load()
        _lib.check(lib.dvd_sf_mlp_bwd_dw(ctypes.byref(self.desc), _p(stash), _p(gstash), int(n_pix), ctypes.byref(W),
                                         ctypes.byref(Bp), _stream()), 'dvd_sf_mlp_bwd_dw')


# ---------------------------------------------------------------------------------------
# elementwise helpers


def scale_add(out, a, scale=1.0, scale_ptr=None, b=None):
    """out = scale * (*scale_ptr) * a + b   (flat, any shape; out may alias a or b)."""
    lib = _lib.load()
    _lib.check(lib.dvd_scale_add(_p(out), _p(a), float(scale), _p(scale_ptr), _p(b), a.numel(), _stream()),
               'dvd_scale_add')
    return out


def mul_mask(out, a, mask):
    """out[b,c,h,w] = a[b,c,h,w] * mask[b,h,w]  (planar a, per-pixel mask; out may alias a)."""
    B, C = a.shape[0], a.shape[1]
    HW = a.numel() // (B * C)
    if mask.numel() != B * HW:
        raise RuntimeError('mul_mask: mask must have one value per pixel')
    lib = _lib.load()
    _lib.check(lib.dvd_mul_mask(_p(out), _p(_dev32(a, 'a')), _p(_dev32(mask, 'mask')), B, C, HW, _stream()), 'dvd_mul_mask')
    return out


def acc_reg(sf0, sf1, coef, g_sf1, abs_sum, accumulate=True):
    lib = _lib.load()
    ws = _workspace(lib.dvd_acc_reg_workspace_bytes(), sf0.device)
    _lib.check(lib.dvd_acc_reg(_p(sf0), _p(sf1), float(coef), _p(g_sf1), _p(ws), _p(abs_sum), int(accumulate),
                               sf0.numel(), _stream()), 'dvd_acc_reg')


# Bumped by every optimiser step: the fused Adam / SGD kernels rewrite parameters behind autograd's back
# (no `_version` change), and per-weight derived buffers (fragment-ordered conv weights) key on it.
WEIGHT_EPOCH = [0]


def adam_step(param, grad1, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps=1e-8, scale=1.0, scale_ptr=None,
              grad2=None, skip_ptr=None):
    """skip_ptr: device scalar; the update is skipped when it is non-zero (fp16 gradient overflow, csrc/a16.hip)."""
    WEIGHT_EPOCH[0] += 1
    lib = _lib.load()
    _lib.check(lib.dvd_adam_step_guarded(_p(param), _p(grad1), float(scale), _p(scale_ptr), _p(grad2), _p(exp_avg),
                                         _p(exp_avg_sq), param.numel(), float(lr), float(beta1), float(beta2), float(eps),
                                         int(step), _p(skip_ptr), _stream()), 'dvd_adam_step')


def sgd_step(param, grad1, momentum_buf, step, lr, momentum, dampening=0.0, weight_decay=0.0, scale=1.0, scale_ptr=None,
             grad2=None, skip_ptr=None):
    """torch.optim.SGD on a flat slice (momentum_buf may be None at momentum 0).  skip_ptr: the (flag, count) pair of
    ops.adam_step; `step` - count == 1 is the first effective step (buf = d), decided on the device."""
    WEIGHT_EPOCH[0] += 1
    lib = _lib.load()
    _lib.check(lib.dvd_sgd_step_guarded(_p(param), _p(grad1), float(scale), _p(scale_ptr), _p(grad2), _p(momentum_buf),
                                        param.numel(), float(lr), float(momentum), float(dampening), float(weight_decay),
                                        int(step), _p(skip_ptr), _stream()), 'dvd_sgd_step')


def gscale_new(device, target_exponent=4.0):
    """The loss-scale state of the fp16 gradients (16 floats on the device; layout: include/dvd_hip.h, policy: csrc/a16.hip)."""
    st = torch.empty(16, device=device, dtype=torch.float32)
    _lib.check(_lib.load().dvd_gscale_init(_p(st), float(target_exponent), _stream()), 'dvd_gscale_init')
    return st


def gscale_step_begin(state):
    """First launch of a training step: clears the forward monitor (validation / warm-up / inference passes fold into it too)."""
    _lib.check(_lib.load().dvd_gscale_step_begin(_p(state), _stream()), 'dvd_gscale_step_begin')


def gscale_end(state):
    _lib.check(_lib.load().dvd_gscale_end(_p(state), _stream()), 'dvd_gscale_end')
