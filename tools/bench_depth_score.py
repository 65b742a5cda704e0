#!/usr/bin/env python
"""Measure the depth-metric path (ops.ratio_median, ops.depth_score, Model.score_depth; csrc/select.hip, csrc/depth_score.hip,
dvd_hip/models/score_depth.py) on a synthetic video of --frames frames at 384 x 672.  Prints one JSON line and, with --out, writes
it as a profile stamped with build.source_digest(('select.hip', 'depth_score.hip')).

  median_frame / median_video   median device-event ms of ops.ratio_median over gt / pred with the mask of countable pixels: N
                           segments of H * W, and one segment of N * H * W; the algorithmic bytes the library counts for it
                           (dvd_byte_counters, class geometry: four histogram passes of 8 B + 1 B of mask per element) and that
                           rate next to the 8 TB/s HBM3E peak.  ('none' runs no median: its scale is a fill of ones.)
  score / score_maps       the one dvd_depth_score launch with seg, without and with the maps (8 + 4 B per pixel, + 13 B of maps)
  score_depth[align]       the whole Model.score_depth call with depth and gt given: the mask pass, the median, the clear of
                           the sums, the launch and the float64 quotients
  aten[...]                the same results built from ATen on the same machine: per frame (or over the video) the quotients with
                           +inf where a pixel is not selected, torch.sort, the two middle ranks gathered on the device; then the
                           terms as elementwise fp32 ops and float64 sums per frame and region

The prediction is a smooth depth with a step edge (tools/bench_splat.py's), the ground truth that depth times 1.7 with log-normal
noise and holes.  The feature has no counterpart before it, so no figure here is a threshold.

    python tools/bench_depth_score.py --out profiles/depth_score.json

bench.py is not touched by this tool."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'dynamic-video-depth_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import torch  # noqa: E402

from bench_splat import HBM_PEAK_GBPS, smooth_depth  # noqa: E402

G_MIN = 1e-2


def aten_median(gt, pred, keep, segments):
    """The median of gt / pred over the kept elements of each segment, as numpy forms it, from a sort; nothing leaves the device."""
    q = torch.where(keep.reshape(segments, -1) & (pred.reshape(segments, -1) > 0), gt.reshape(segments, -1) / pred.reshape(segments, -1),
                    torch.full((), float('inf'), device=gt.device))
    n = (keep.reshape(segments, -1) & (pred.reshape(segments, -1) > 0)).sum(1)
    v = q.sort(1).values
    lo, hi = ((n - 1).clamp(min=0) // 2)[:, None], (n // 2).clamp(max=v.shape[1] - 1)[:, None]
    return torch.where(n > 0, (v.gather(1, lo) + v.gather(1, hi))[:, 0] / 2, torch.full((), float('nan'), device=gt.device))


def aten_score(pred, gt, scale, seg):
    """sums [N,3,9] in float64 from elementwise fp32 terms."""
    p, g = pred[:, 0], gt[:, 0]
    q = scale[:, None, None] * p
    ok = (g > G_MIN) & (p > 0) & q.isfinite()
    d = q - g
    dd = d * d
    l = (q.log() - g.log()).clamp(-32.0, 32.0)
    ratio = torch.maximum(q / g, g / q)
    terms = [torch.ones_like(p), (d.abs() / g).clamp(max=1024.0), (dd / g).clamp(max=1024.0), dd.clamp(max=1024.0),
             (l * l).clamp(max=1024.0), l, (ratio < 1.25).float(), (ratio < 1.5625).float(), (ratio < 1.953125).float()]
    t = torch.stack(terms, 1).double()                                        # [N,9,H,W]
    regions = torch.stack([ok, ok & (seg <= 0.5), ok & (seg > 0.5)], 1)      # [N,3,H,W]
    return (torch.where(regions[:, :, None], t[:, None], torch.zeros((), dtype=torch.float64, device=p.device))).flatten(3).sum(3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=80)
    ap.add_argument('--height', type=int, default=384)
    ap.add_argument('--width', type=int, default=672)
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    from dvd_hip import build, ops
    from dvd_hip.models import score_depth as SD
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    N, H, W = a.frames, a.height, a.width
    g = torch.Generator(device=device).manual_seed(0)
    pred = smooth_depth(N, H, W, device)
    gt = pred * 1.7 * torch.exp(0.2 * torch.randn(N, 1, H, W, device=device, generator=g))
    gt[torch.rand(N, 1, H, W, device=device, generator=g) < 0.15] = 0.0
    seg = (torch.rand(N, H, W, device=device, generator=g) < 0.3).float()
    keep = gt > G_MIN
    keep8 = keep.to(torch.uint8)
    store = SimpleNamespace(cat=SimpleNamespace(n_frames=N), H=H, W=W, device=device, motion_seg=seg, depth_mvs=gt)

    def event():
        return torch.cuda.Event(enable_timing=True)

    def timed(fn):
        fn()                                                       # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = event(), event()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    nbytes, result = {}, {}

    def counted(name, fn):
        def run():
            b0 = ops.flop_counters()['geometry']
            result[name] = fn()
            nbytes[name] = ops.flop_counters()['geometry'] - b0
        return run

    launches = {
        'median_frame': lambda: ops.ratio_median(gt.reshape(N, -1), pred.reshape(N, -1), mask=keep8.reshape(N, -1)),
        'median_video': lambda: ops.ratio_median(gt.reshape(1, -1), pred.reshape(1, -1), mask=keep8.reshape(1, -1)),
    }
    ms = {k: timed(counted(k, fn)) for k, fn in launches.items()}
    scale = result['median_video']['median'].expand(N).contiguous()
    sums = torch.zeros(N, 3, 9, device=device, dtype=torch.int64)

    def score(maps):
        sums.zero_()
        return ops.depth_score(pred, gt, scale, seg=seg, sums=sums, maps=maps)

    ms['score'] = timed(counted('score', lambda: score(False)))
    ms['score_maps'] = timed(counted('score_maps', lambda: score(True)))
    whole = {al: timed(lambda al=al: SD.score_depth(None, store, depth=pred, align=al)) for al in SD.ALIGN}
    out = SD.score_depth(None, store, depth=pred, align='median_video')
    assert torch.equal(out['sums'], sums) and torch.equal(out['scale'], scale)      # the launches timed here ARE what the call ran

    aten = {'median_frame': timed(lambda: aten_median(gt, pred, keep, N)), 'median_video': timed(lambda: aten_median(gt, pred, keep, 1)),
            'score': timed(lambda: aten_score(pred, gt, scale, seg))}

    def aten_whole(al):
        k = gt > G_MIN
        if al == 'none':
            sc = torch.ones(N, device=device)
        elif al == 'median_frame':
            sc = aten_median(gt, pred, k, N)
        else:
            sc = aten_median(gt, pred, k, 1).expand(N)
        return sc, aten_score(pred, gt, sc, seg)

    for al in SD.ALIGN:
        aten['score_depth/' + al] = timed(lambda al=al: aten_whole(al))
    a_frame, a_video = aten_median(gt, pred, keep, N), aten_median(gt, pred, keep, 1)
    same_medians = bool(torch.equal(a_frame, result['median_frame']['median']) and
                        torch.equal(a_video, result['median_video']['median']))
    same_counts = bool(torch.equal(aten_score(pred, gt, scale, seg)[..., 0].long(), sums[..., 0]))

    def kernel(k):
        t = statistics.median(ms[k])
        return {'ms': t, 'ms_min': min(ms[k]), 'MB_algorithmic': nbytes[k] / 1e6, 'GBps': nbytes[k] / t / 1e6,
                'frac_of_hbm_peak': nbytes[k] / t / 1e6 / HBM_PEAK_GBPS}

    video = {k: [float(x) for x in v.cpu().tolist()] for k, v in out['video'].items()}
    line = json.dumps({
        'metric': 'score_depth at %dx%d: %d frames (%d pixels)' % (H, W, N, N * H * W),
        'data': 'synthetic: smooth depth with a step edge against 1.7 x itself with log-normal noise and 15 %% holes',
        'device': torch.cuda.get_device_name(device), 'source_digest': build.source_digest(('select.hip', 'depth_score.hip')),
        'reps': a.reps, 'shift': out['shift'],
        'median_frame': kernel('median_frame'), 'median_video': kernel('median_video'),
        'score': kernel('score'), 'score_maps': kernel('score_maps'),
        'timing_includes': 'the host wrapper (validation, allocation of the outputs and the workspace) of every launch; '
                           'score: the clear of the sums',
        'score_depth': {al: {'ms': statistics.median(whole[al]), 'ms_min': min(whole[al])} for al in SD.ALIGN},
        'aten': {k: {'ms': statistics.median(v), 'ms_min': min(v)} for k, v in aten.items()},
        'aten_medians_equal_bit_for_bit': same_medians, 'aten_counts_equal': same_counts,
        'video': video, 'hbm_peak_GBps': HBM_PEAK_GBPS,
        'hbm_peak_allocated_GB': torch.cuda.max_memory_allocated(device) / 2 ** 30})
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
