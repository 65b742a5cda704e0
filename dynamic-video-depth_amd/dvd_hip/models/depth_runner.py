"""The depth network of a step (phases 1 and 3 of `Model._train_on_batch`) and of inference: chunk by chunk through captured HIP
graphs, the autograd state of as many chunks as fit kept between forward and backward.  `DepthRunner` is the one place that
knows what a chunk, a graph key, a kept slot and a replay are, and it does the slots' memory bookkeeping."""
import gc
import os
import sys
import warnings
from collections import namedtuple

import torch

from .. import conv, ops, parallel


def head_room_fraction(world, total_bytes=None):
    """Fraction of the device the memory planner leaves untouched: allocator fragmentation, and -- with several ranks --
    whatever RCCL's collectives allocate while the step runs (its communicator is created BEFORE the planner reads the free
    memory, parallel.init_from_env, so its channel / staging buffers are already counted as used).  Single process: 8 % (23 GB
    of 288); data parallel: 10 % (29 GB), derated automatically -- the benchmark configuration still keeps both of its slots
    (225 GB free - 60 GB slot >= 130 GB of stashes + 29 GB)."""
    frac = 0.08 if world <= 1 else 0.10
    # DVD_HEAD_ROOM_GB: an explicit head room in GB for runs that must leave more to other tenants of the device -- the 8-rank
    # run's RCCL buffers when the communicator is created late, or a memory-capped deployment.  Absolute: it is divided by the
    # device's REAL size (keep_slot_fits multiplies the fraction by that same total), not by a hard-coded 288 GB.
    gb = _head_room_gb_from_env()
    if gb:
        if total_bytes is None:
            total_bytes = torch.cuda.mem_get_info()[1] if torch.cuda.is_available() else 288 * 2 ** 30
        frac = max(frac, min(0.9, gb * 2 ** 30 / float(total_bytes)))
    return frac


def _head_room_gb_from_env():
    """DVD_HEAD_ROOM_GB, validated (also once at import: a malformed value must not first surface in the middle of step
    planning)."""
    raw = os.environ.get('DVD_HEAD_ROOM_GB')
    if not raw:
        return 0.0
    try:
        gb = float(raw)
    except ValueError:
        raise ValueError('DVD_HEAD_ROOM_GB=%r is not a number of gigabytes' % raw)
    if not (0.0 <= gb < 1e5):
        raise ValueError('DVD_HEAD_ROOM_GB=%r: expected a non-negative number of gigabytes' % raw)
    return gb


_head_room_gb_from_env()        # validate at import


def keep_slot_fits(est, free, total, reserve, spare, kept, budget, head_room=0.08):
    """May one more kept-activation slot of `est` bytes be captured?  `free` = HBM available to ordinary allocations,
    `reserve` = what phase 2 (the MLP stashes) will allocate, `spare` = room for the recompute graph of a chunk that is not
    kept (0 if this slot completes the step), `kept` = bytes already held by slots, `budget` = --depth_keep_gb.
    `head_room` (head_room_fraction) of the device stays free."""
    return kept + est <= budget and free - est >= reserve + head_room * total + spare


def images_per_chunk(opt, auto_chunk=None):
    """Images per depth-net chunk: --depth_chunk, or (0 = auto) what DepthRunner.pick_chunk chose at the first training step."""
    c = int(getattr(opt, 'depth_chunk', 48))
    return max(1, c if c > 0 else int(auto_chunk or 48))


def working_size(opt, net=None):
    """(H, W) at which the depth net works when that is not the frame size -- opt.midas_resize, else the `resize` the net was
    built with (the dataset-name rule of Model.__init__) -- or None."""
    size = getattr(opt, 'midas_resize', None)
    if size is None:
        size = getattr(net, 'resize', None)
    return None if size is None else (int(size[0]), int(size[1]))


def working_pixels(n_images, H, W, resize=None):
    """Pixels the depth net works on for n_images frames of H x W: a kept slot's autograd state scales with these."""
    return n_images * (H * W if resize is None else resize[0] * resize[1])


def resize_extra_bytes(n_images, H, W, resize=None):
    """What a slot holds at FRAME size on top of its working-size state when the net resizes: two fp32 planes per image
    (the resized depth and its gradient)."""
    return 0 if resize is None else 2 * 4 * n_images * H * W


# What DepthRunner.graphs holds.  _Captured: one graph and the algorithmic work per kernel class counted at its capture
# (bench.py roofline_mfma: added at every replay).  x / y / gy: the static input, output and output-gradient buffers.
_Captured = namedtuple('_Captured', 'graph flops')
_Recompute = namedtuple('_Recompute', 'run x y gy')             # kinds 'f' (gy is None) and 'fb': ONE graph
_Slot = namedtuple('_Slot', 'fwd bwd x y gy bytes')             # kind 'keep': forward and backward graph on one private pool


# -- HIP graphs for the depth net -------------------------------------------------------
# A MiDaS forward+backward of one chunk is ~2 000 kernel launches; 12 chunk passes per step make the
# step launch-bound on hosts with slower cores (rocprofv3: 1.95 s of kernels in a 2.8 s step on one
# box, 1.97 s wall on another).  With --depth_graphs 1 (default since the convolutions run on this
# package's own kernels: round 1's replay through MIOpen was erratic)
# each chunk shape is captured once (forward-only graph 'f' for phase 1, forward+backward graph 'fb' for
# phase 3, static input / output / output-gradient buffers; parameter gradients accumulate in place
# into the flat gradient buffer) and replayed; anything that cannot be captured falls back to eager.
# -- kept activations -----------------------------------------------------------------------
# With this package's kernels a MiDaS forward keeps ~1 GB of autograd state per 384x672 image (round 1, through
# MIOpen/ATen: 3 GB), so the state of ALL chunks of a 48-pair step (95 GB) fits next to the MLP stashes: phase 1 runs
# every chunk's forward WITH its graph state into a slot of its own (forward graph + backward graph on one private
# memory pool), phase 3 replays the slot's backward graph -- the forward is computed once per step instead of twice.
class DepthRunner:
    """The depth net's graphs and kept slots of ONE model, and the memory bookkeeping that decides about them."""
    def __init__(self, opt, net, flat, act_fp16):
        self.opt, self.net, self.flat, self.act_fp16 = opt, net, flat, bool(act_fp16)
        self.graphs = {}             # _graph_key / _slot_key -> _Recompute / _Slot; None: denied, trimmed, or its capture failed
        self.keep_bytes = 0          # HBM held by kept-activation graph slots
        self.keep_per_px = 0.0       # measured bytes per pixel the net works on (working_pixels) of a captured slot
        self.auto_chunk = None       # --depth_chunk 0: images per slot, chosen at the first training step that keeps slots
        self.pool_bytes = 0          # HBM reserved by the private pools of all captured graphs
        self.denied = {}             # slot key -> step at which it was last denied / trimmed (retried 16 steps later)
        self.step_no = 0
        self.resize = working_size(opt, net)     # None: the net works at the frame size

    def begin_step(self):
        self.step_no += 1

    # -- chunks, keys, replay -------------------------------------------------------------------------------------------
    def chunk(self):
        return images_per_chunk(self.opt, self.auto_chunk)

    def _chunks(self, *tensors):
        """(chunk index, this chunk's rows of every tensor) over the images of one image set; None stays None (the MiDaS net
        takes no frame ids).  A ragged last chunk has its own shape, hence its own graph / slot keys."""
        c = self.chunk()
        for ci, b0 in enumerate(range(0, tensors[0].shape[0], c)):
            yield (ci,) + tuple(None if t is None else t[b0:b0 + c] for t in tensors)

    def _graph_key(self, kind, chunk):
        return (kind, tuple(chunk.shape), bool(self.opt.midas))

    def _slot_key(self, slot, chunk):
        return ('keep', slot, tuple(chunk.shape), bool(self.opt.midas))

    def _live_slots(self):
        return [k for k, v in self.graphs.items() if k[0] == 'keep' and v is not None]

    def _use_graphs(self, fid):
        return bool(getattr(self.opt, 'depth_graphs', 1)) and (fid is None or not self.opt.use_embedding)

    @staticmethod
    def _replay(run, *copies):
        """Fill the static buffers ((static, value) pairs) and replay one captured graph."""
        for static, value in copies:
            static.copy_(value)
        conv.PACK_PLAN.ensure_current()      # (packed weights follow the optimiser: two launches after a step)
        run.graph.replay()
        ops.note_replay(run.flops)

    # -- the network, eagerly -------------------------------------------------------------------------------------------
    def _net_forward(self, img, fid):
        if self.opt.midas:
            return self.net(img)
        return self.net(img, fid.long() if fid is not None else None)

    def _forward_backward(self, img, fid, g_depth=None):
        """Eager forward + backward of one chunk (g_depth None: zeros, the warm-up passes of a capture)."""
        self.flat.detach_grads()          # one multi-tensor accumulation per chunk instead of ~620 adds
        with torch.enable_grad():
            d = self._net_forward(img, fid)
        d.backward(torch.zeros_like(d) if g_depth is None else g_depth)
        self.flat.absorb_grads()

    # -- what the Model calls ---------------------------------------------------------------------------------------------
    def forward(self, img, fid):
        """Depth maps without autograd state: phase 1 when nothing is kept, and inference."""
        out = []
        with torch.no_grad():
            for _, chunk, f in self._chunks(img, fid):
                g = self._recompute_graph('f', chunk, f)
                if g is not None:
                    self._replay(g.run, (g.x, chunk))
                    out.append(g.y.clone())
                else:
                    out.append(self._net_forward(chunk, f))
        return torch.cat(out, 0).contiguous()

    def forward_keep(self, img, fid, slot0, reserve_bytes, n_slots_total):
        """Depth maps of phase 1 with the autograd state of as many chunks as fit kept for phase 3.  slot0: the slot of this
        image set's first chunk, n_slots_total: slots of the whole step, reserve_bytes: what phase 2 will allocate."""
        out = []
        for ci, chunk, f in self._chunks(img, fid):
            s = self._keep_slot(slot0 + ci, chunk, f, reserve_bytes, n_slots_total)
            if s is not None:
                self._replay(s.fwd, (s.x, chunk))
                out.append(s.y.detach().clone())
            else:
                with ops.counting_recomputed():      # phase 3 runs this chunk's forward again (forward+backward graph)
                    out.append(self.forward(chunk, f))
        return torch.cat(out, 0).contiguous()

    def backward(self, img, fid, g_depth, slot0=None):
        """Phase 3 for one image set: parameter gradients from the depth gradients, into the flat gradient buffer."""
        for ci, chunk, f, g in self._chunks(img, fid, g_depth):
            s = None if slot0 is None else self.graphs.get(self._slot_key(slot0 + ci, chunk))
            if s is not None:                        # the forward of phase 1 left this chunk's graph state in its slot
                self._replay(s.bwd, (s.gy, g))
                continue
            r = self._recompute_graph('fb', chunk, f)
            if r is not None:
                self._replay(r.run, (r.x, chunk), (r.gy, g))
                continue
            self._forward_backward(chunk, f, g)

    def backward_will_capture(self, *image_sets):
        """Will phase 3 still have to capture a graph -- is there a chunk that is not kept and has no recompute graph yet?
        image_sets: (slot0, img) as handed to forward_keep / backward, over the REAL chunk list."""
        if not getattr(self.opt, 'depth_graphs', 1):
            return False
        return any(self.graphs.get(self._slot_key(slot0 + ci, chunk)) is None and self._graph_key('fb', chunk) not in self.graphs
                   for slot0, img in image_sets for ci, chunk in self._chunks(img))

    def free_hbm(self, device):
        """(bytes available to ordinary allocations: free on the device + cached by the allocator, total bytes).  The
        private pools of captured graphs are reserved but not `allocated` once the capture's temporaries are released, and
        they are NOT reusable: they are subtracted."""
        free, total = torch.cuda.mem_get_info(device)
        cached = torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device) - self.pool_bytes
        return free + max(0, cached), total

    def choose_chunk(self, B, HW, reserve_bytes, device):
        """--depth_chunk 0: decided ONCE, at the first training step that keeps slots (graphs and slots are per chunk shape)."""
        if int(self.opt.depth_chunk) <= 0 and self.auto_chunk is None:
            self.auto_chunk = self.pick_chunk(B, HW, reserve_bytes, device)

    def trim(self, device, need_bytes):
        """After phase 1: if the slots left less than phase 2 needs (a first slot larger than its a-priori estimate),
        give the newest slots back -- their chunks take the recompute path in phase 3, the step stays correct."""
        free, total = self.free_hbm(device)
        if os.environ.get('DVD_KEEP_DEBUG'):
            print('after phase 1: free %.1f GB, phase 2 needs %.1f, pools %.1f' % (free / 2 ** 30, need_bytes / 2 ** 30,
                                                                               self.pool_bytes / 2 ** 30), file=sys.stderr, flush=True)
        kept = self._live_slots()
        while kept and free < need_bytes + 0.5 * head_room_fraction(parallel.world_size(), total) * total:
            key = kept.pop()
            self._release(key)
            self.denied[key] = self.step_no
            gc.collect()
            free, total = self.free_hbm(device)

    # -- planning -------------------------------------------------------------------------------------------------------
    def slot_bytes_per_px(self):
        """Autograd state a kept slot holds per pixel the net works on: measured on the slots captured so far, else an a-priori figure
        (as measured in round 6: MiDaS with fused epilogues 4.8 KB -- 55.8 GB per 48 images at 384x672 --, 2.5 KB with fp16
        activations, the hourglass 6.7 KB; rounds 4-5 assumed 4.4 / 2.4 KB).  The hourglass with fp16 activations: 4.9 KB
        (keep_per_px after two steps of 48 pairs at 384x672 with 16-image slots on MI355X: 4 878 bytes, fp32 6 657)."""
        if self.opt.midas:
            apriori = 2500.0 if self.act_fp16 else 4900.0
        else:
            apriori = 4900.0 if self.act_fp16 else 6700.0
        return max(apriori, self.keep_per_px)

    def pick_chunk(self, B, HW, mlp_need, device):
        """--depth_chunk 0: the largest of 48 / 24 / 16 images per slot for which EVERY slot of the step is expected to fit
        beside phase 2's allocations (then nothing is recomputed, and larger launches are a little faster: 16 / 24 / 48
        measured 0.840 / 0.843 / 0.851 iters/s); if no size fits, the finest -- slots are kept one by one, so smaller slots
        keep more of the batch (hourglass at 384x672: one of two 48-image slots, or all six 16-image ones)."""
        free, total = self.free_hbm(device)
        budget = float(getattr(self.opt, 'depth_keep_gb', 150.0)) * 2 ** 30
        avail = min(budget, free - mlp_need - head_room_fraction(parallel.world_size(), total) * total)
        per_img = working_pixels(1, HW, 1, self.resize) * self.slot_bytes_per_px() + resize_extra_bytes(1, HW, 1, self.resize)
        for c in (48, 24, 16):
            cc = min(c, B)
            if 2 * B * per_img + 2 * (-(-B // cc)) * 1.5 * 2 ** 30 <= avail:
                return cc
        return min(16, B)

    @staticmethod
    def _pool_size(pool_id, device):
        """Bytes of the caching allocator's segments that belong to a graph's private pool (the reserved-bytes counter does
        not tell: a new pool may be carved from memory the process had reserved before)."""
        pid = tuple(pool_id)
        return sum(seg['total_size'] for seg in torch.cuda.memory_snapshot()
                   if tuple(seg.get('segment_pool_id', (0, 0))) == pid and seg.get('device', device.index) == device.index)

    def _release(self, key):
        """Give a live slot back: its graphs, static buffers and private pool go, both byte counters fall by its size."""
        size = self.graphs[key].bytes
        self.keep_bytes -= size
        self.pool_bytes -= size
        self.graphs[key] = None

    # -- capture --------------------------------------------------------------------------------------------------------
    def _try_capture(self, key, capture, warning):
        """File capture()'s entry under key.  A capture is an optimisation only: a failure is a warning, and None is filed."""
        try:
            entry = capture()
        except Exception as e:                             # noqa: BLE001
            warnings.warn(warning % (str(e).splitlines()[0],))
            torch.cuda.synchronize()
            self.flat.reattach_grads()
            entry = None
        self.graphs[key] = entry
        return entry

    def _begin_capture(self, chunk, fid, warm_up, save_grad=True):
        """What every capture starts with -> (static input, backup of the flat gradient, flop counters at the start).
        warm_up: None, or 'f' / 'fb' for two eager passes of that kind on a side stream first."""
        gc.collect()        # graphs of discarded models must not be destroyed while this capture is open
        static_in = chunk.clone()
        grad_backup = self.flat.grad.clone() if save_grad else None
        if warm_up:
            side = torch.cuda.Stream()                 # warm-up outside the capture (allocator, MIOpen handles)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    if warm_up == 'f':
                        with torch.no_grad():
                            self._net_forward(static_in, fid)
                    else:
                        self._forward_backward(static_in, fid)
            torch.cuda.current_stream().wait_stream(side)
        conv.PACK_PLAN.extend()        # the packings the warm-up passes asked for: persistent buffers, two launches per step
        ops.begin_capture()
        return static_in, grad_backup, ops.flop_counters()

    # thread_local: calls made by other threads (the RCCL watchdog polling its events) do not invalidate the capture; the
    # step also keeps collectives out of flight while a graph is being captured
    _MODE = dict(capture_error_mode='thread_local')

    def _recompute_graph(self, kind, chunk, fid):
        """The 'f' (forward, no autograd state) or 'fb' (forward+backward) graph of this chunk shape, captured at its first
        use; None if graphs are off or the capture failed."""
        if not self._use_graphs(fid):
            return None
        key = self._graph_key(kind, chunk)
        if key in self.graphs:
            return self.graphs[key]
        return self._try_capture(key, lambda: self._capture_recompute(kind, chunk, fid),
                                 'depth-net HIP graph capture failed (%s); running eagerly')

    def _capture_recompute(self, kind, chunk, fid):
        x, grad_backup, f0 = self._begin_capture(chunk, fid, warm_up=kind, save_grad=kind == 'fb')
        graph = torch.cuda.CUDAGraph()
        if kind == 'f':
            with torch.no_grad(), torch.cuda.graph(graph, **self._MODE):
                y = self._net_forward(x, fid)
            gy = None
        else:
            gy = torch.zeros(chunk.shape[0], 1, chunk.shape[2], chunk.shape[3], device=chunk.device)
            # parameter gradients: the engine hands over fresh tensors (no pre-attached .grad) and ONE multi-tensor add
            # per chunk, captured with the rest, folds them into the flat buffer -- ~620 tiny accumulate kernels
            # per replay otherwise
            self.flat.detach_grads()
            with torch.cuda.graph(graph, **self._MODE):
                with torch.enable_grad():
                    y = self._net_forward(x, fid)
                y.backward(gy)
                self.flat.absorb_grads()
            self.flat.grad.copy_(grad_backup)   # warm-up / capture passes used zero output gradients
        entry = _Recompute(_Captured(graph, ops.flops_since(f0)), x, y, gy)
        self.pool_bytes += self._pool_size(graph.pool(), chunk.device)
        return entry

    def _keep_slot(self, slot, chunk, fid, reserve_bytes, n_slots_total):
        """The kept-activation slot of this chunk (captured now if there is room for it), or None."""
        if not self._use_graphs(fid):
            return None
        key = self._slot_key(slot, chunk)
        # does this slot complete a step whose other slots are all kept?  (asked before the dict changes below)
        keep_keys = [k for k in self.graphs if k[0] == 'keep']
        last_and_all_kept = len(keep_keys) == n_slots_total - 1 and len(self._live_slots()) == len(keep_keys)
        if key in self.graphs:
            entry = self.graphs[key]
            # a slot that was denied (or trimmed) for lack of room is tried again every 16 steps: one transient
            # low-memory moment must not pin its chunk to the recompute path for the rest of the run
            if entry is not None or self.step_no - self.denied.get(key, self.step_no) < 16:
                return entry
            del self.graphs[key]
        # slots captured for another chunk shape at this position (the last, smaller batch of an epoch) hold HBM this
        # shape needs: release them
        for k in [k for k in self._live_slots() if k[1] == slot and k != key]:
            self._release(k)
            del self.graphs[k]
        # bytes a slot will hold: measured on the slots captured so far (per image and pixel), a-priori figure (MiDaS with
        # fused epilogues: ~4.1 KB per pixel, ~2.2 KB with fp16 activations) for the first one, + packed weights
        # (pixels the net works on: with a working resolution the state scales with that, + the frame-size planes of the resize)
        n_px = working_pixels(chunk.shape[0], chunk.shape[2], chunk.shape[3], self.resize)
        extra = resize_extra_bytes(chunk.shape[0], chunk.shape[2], chunk.shape[3], self.resize)
        est = int(n_px * self.slot_bytes_per_px() + extra + 1.5 * 2 ** 30)
        free, total = self.free_hbm(chunk.device)
        budget = float(getattr(self.opt, 'depth_keep_gb', 150.0)) * 2 ** 30
        # room that must stay free: the MLP stashes of phase 2 + 8 % head room + (unless this is the last slot of a step
        # whose other slots are all kept) the pool of the forward+backward recompute graph a non-kept chunk will need
        # (the recompute graph of a non-kept chunk frees its activations as its backward proceeds: its pool measures 0.26-0.31
        #  of a kept slot's -- 8.0 vs 25.6 GB for 16 hourglass images, 9.7 vs 37.9 GB for 16 MiDaS images at 768x1344 -- so half
        #  the slot's estimate is room enough; rounds 4-5 asked for all of it and kept one slot fewer)
        spare = 0 if last_and_all_kept else est // 2
        hr = head_room_fraction(parallel.world_size(), total)
        if os.environ.get('DVD_KEEP_DEBUG'):
            print('keep slot %d: est %.1f GB, free %.1f, reserve %.1f + %.1f + spare %.1f, kept so far %.1f, pools %.1f' % (
                slot, est / 2 ** 30, free / 2 ** 30, reserve_bytes / 2 ** 30, hr * total / 2 ** 30, spare / 2 ** 30,
                self.keep_bytes / 2 ** 30, self.pool_bytes / 2 ** 30), file=sys.stderr, flush=True)
        if not keep_slot_fits(est, free, total, reserve_bytes, spare, self.keep_bytes, budget, hr):
            self.graphs[key] = None
            self.denied[key] = self.step_no
            return None
        entry = self._try_capture(key, lambda: self._capture_slot(chunk, fid),
                                  'keeping the depth net\'s activations in HIP graphs failed (%s); recomputing')
        if entry is not None:
            self.keep_bytes += entry.bytes
            self.pool_bytes += entry.bytes
            self.keep_per_px = max(self.keep_per_px, (entry.bytes - extra) / float(n_px))
        return entry

    def _capture_slot(self, chunk, fid):
        # (the warm-up passes run once: while no slot is live)
        x, grad_backup, f0 = self._begin_capture(chunk, fid, warm_up=None if self._live_slots() else 'fb')
        pool = torch.cuda.graph_pool_handle()
        g_f, g_b = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_f, pool=pool, **self._MODE):
            with torch.enable_grad():
                y = self._net_forward(x, fid)
        fwd = _Captured(g_f, ops.flops_since(f0))
        gy = torch.zeros(chunk.shape[0], 1, chunk.shape[2], chunk.shape[3], device=chunk.device)
        self.flat.detach_grads()
        ops.begin_capture()         # its own generation: g_b's scalars are zero-filled by g_b's replay
        f0 = ops.flop_counters()
        with torch.cuda.graph(g_b, pool=pool, **self._MODE):
            y.backward(gy)
            self.flat.absorb_grads()
        bwd = _Captured(g_b, ops.flops_since(f0))
        self.flat.grad.copy_(grad_backup)
        return _Slot(fwd, bwd, x, y, gy, self._pool_size(pool, chunk.device))
