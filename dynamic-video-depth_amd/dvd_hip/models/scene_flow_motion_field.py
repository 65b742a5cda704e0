"""`--net scene_flow_motion_field` on MI355X: the per-video test-time-optimisation step.

Drop-in for /root/reference/models/scene_flow_motion_field.py:32-367 (class `Model`):
same `add_arguments` flag set (:33-67), constructor contract `Model(opt, loggers)`
(:78-138), attributes `_nets = [net_depth, net_sceneflow]`, `_optimizers`, `_metrics`,
`input_names`, `requires`, and `_train_on_batch(epoch, batch_ind, batch) -> batch_log`
with the keys of :226,321-323,195.

What is different is HOW a step runs.  The reference builds one autograd graph out of
~250 ATen launches per pair; here the step is three phases over device-resident data:

  1. depth nets forward, chunk by chunk (--depth_chunk images), every chunk WITH its autograd state kept in a slot of
     its own (a forward HIP graph and a backward HIP graph on one private memory pool) -> depth_1, depth_2; chunks that
     do not fit --depth_keep_gb take a no-graph forward and are recomputed in phase 3;
  2. everything downstream of the depths in hand-written HIP kernels, per chunk of
     pairs: unproject -> fused MLP (Euler steps, activations stashed) -> ONE fused
     warp+reprojection+loss forward/backward launch -> MLP backward (dX chain, dW) ->
     unproject backward; the acceleration regulariser shares the first MLP evaluation.  Gradients
     are produced UN-normalised; the batch-global 1/(sum(mask)+1e-8) is a device
     scalar applied at the very end, after the (data-parallel) all-reduce of the five
     loss sums, so there is no host synchronisation inside the step and N ranks
     reproduce the single-device result on the concatenated batch;
  3. (not in the warm-up phase) depth nets backward from the depth gradients of phase 2: a replay of each kept slot's
     backward graph (or a forward+backward recompute graph); then one RCCL all-reduce per net over its flat gradient
     buffer and one fused optimiser launch per net (Adam, or SGD under --optim sgd).

`Model._train_on_batch` is that list: the step's plan, its image sets and phase 1 (models/depth_runner.py),
`SfStep(...).run(schedule)` for phase 2, `Model._finish_step` for phase 3.  The plan (Euler steps per pair, gap groups, MLP
chunks, what phase 2 will allocate), the choice between phase 2's four schedules and the schedules themselves live in
models/sf_step.py; the Model is not an argument to anything there.

Every convolution (the 7x7 stride-2 stem included, round 4), BatchNorm+ReLU, pooling, up-sampling and the MLP run on this
package's HIP kernels (csrc/); the matrix kernels evaluate fp32 products from two fp16 terms per operand (csrc/dvd_split.h).
`--act_fp16` (BASELINE configs[4]) stores the depth net's activations and their gradients as fp16 (csrc/a16.hip: the loss scale
lives on the device); `--use_cnn` swaps the MLP for the reference's U-Net scene-flow network (networks/FCNUnet.py) under autograd.
"""
import contextlib
import numbers
import os
import warnings
from os import makedirs
from os.path import join

import numpy as np
import torch

from .. import configs, conv, flat, ops, parallel
from ..losses.scene_flow_projection import BackwardWarp, flow_by_depth, scene_flow_projection_slack, unproject_ptcld
from ..networks.FCNUnet import FCNUnet
from ..networks.sceneflow_field import SceneFlowFieldNet
from ..third_party.hourglass import HourglassModel_Embed
from ..third_party.MiDaS import MidasNet
from . import evaluate, frame_union, point_tracks, render, score_depth, sf_step, tracks
from . import filter as depth_filter
from .depth_runner import DepthRunner, head_room_fraction, images_per_chunk, keep_slot_fits      # noqa: F401 (re-exported)
from .netinterface import NetInterface
from .sf_step import gap_plan, pairs_per_chunk      # noqa: F401 (re-exported)

CAM_KEYS = ops.CAM_KEYS


def midas_resize_of(opt):
    """opt.midas_resize, validated: None (the default), or the (H, W) at which MiDaS works whatever the frame size -- the
    reference only has its dataset-name rule for [224, 384] (scene_flow_motion_field.py:84-94).  An attribute, not a flag of
    add_arguments (that flag set is the reference's); checkpointed option dictionaries carry it like any other attribute."""
    size = getattr(opt, 'midas_resize', None)
    if size is None:
        return None
    try:
        h, w = size
        ok = int(h) == h and int(w) == w
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('opt.midas_resize must be an (H, W) pair of integers, got %r' % (size,))
    h, w = int(h), int(w)
    if h <= 0 or w <= 0 or h % 32 or w % 32:
        raise ValueError('opt.midas_resize=%r: both values must be positive multiples of 32 (the total stride of the MiDaS '
                         'encoder)' % (size,))
    if not getattr(opt, 'midas', False):
        raise ValueError('opt.midas_resize=%r needs --midas: the working resolution belongs to the MiDaS depth net, the '
                         'hourglass has none' % (size,))
    return h, w


def share_frames_of(opt):
    """(opt.share_frames, opt.share_quantum), validated: whether a step runs the depth net once per DISTINCT frame
    (models/frame_union.py), and the multiple its number of union rows is padded to.  Attributes, not flags of add_arguments,
    like opt.midas_resize; off by default."""
    share = bool(getattr(opt, 'share_frames', 0))
    quantum = getattr(opt, 'share_quantum', 8)
    if share and (isinstance(quantum, bool) or not isinstance(quantum, numbers.Integral) or quantum < 1):
        raise ValueError('opt.share_quantum must be an integer >= 1, got %r' % (quantum,))
    return share, (int(quantum) if share else None)


class Model(NetInterface):
    @classmethod
    def add_arguments(cls, parser):
        # the reference's flag set, verbatim names/defaults (scene_flow_motion_field.py:35-65)
        f, i, s = float, int, str
        for name, typ, default in (('l1_mul', f, 1e-4), ('disp_mul', f, 10), ('loss_type', s, 'l2'),
                                   ('scene_lr_mul', f, 1), ('n_down', i, 3), ('sf_min_mul', f, 0),
                                   ('sf_quantile', f, 0.5), ('static_mul', f, 1), ('flow_mul', f, 10),
                                   ('acc_mul', f, 100), ('si_mul', f, 0), ('cos_mul', f, 0), ('warm_mul', f, 1),
                                   ('interp_steps', i, 5), ('warm_sf', i, 0), ('n_freq_xyz', i, 16),
                                   ('n_freq_t', i, 16), ('sf_mag_div', f, 100)):
            parser.add_argument('--' + name, type=typ, default=default)
        for name in ('one_way', 'weight_steps', 'static', 'motion_seg_hard', 'warm_static', 'use_disp',
                     'use_disp_ratio', 'time_dependent', 'use_cnn', 'use_embedding', 'use_motion_seg', 'warm_reg',
                     'midas'):
            parser.add_argument('--' + name, action='store_true')
        # MI355X-specific knobs (new; defaults need no tuning)
        parser.add_argument('--mlp_stash_gb', type=float, default=48.0,
                            help='HBM budget for the scene-flow MLP activation stashes; sets pairs per chunk')
        parser.add_argument('--mlp_whole_batch_gb', type=float, default=160.0,
                            help='HBM ceiling for keeping the forward stashes of the whole batch alive so that the '
                                 'warp+loss kernel runs as ONE launch (falls back to one launch per chunk)')
        parser.add_argument('--mlp_recompute', type=int, default=1,
                            help='when the forward stashes of the whole batch do not fit --mlp_whole_batch_gb: 1 = one stash-free '
                                 'forward over all pairs, ONE warp+loss launch, then per chunk the stashed forward again + the '
                                 'merged backward (3 forward + 2 dX + 2 dW passes per pair at gap 1); 0 = the late-normaliser '
                                 'schedule of rounds 1-5 (one warp+loss launch per chunk, 3 + 3 + 3 passes)')
        parser.add_argument('--depth_chunk', type=int, default=48,
                            help='images per depth-net forward/backward chunk = per kept-activation graph slot (48: two slots per '
                                 '48-pair step).  0 = chosen at the first training step: the largest of 48 / 24 / 16 for which every '
                                 'slot is expected to fit beside the MLP stashes, else 16 (what bench.py runs with)')
        parser.add_argument('--depth_graphs', type=int, default=1,
                            help='1 (default): capture the depth net per chunk shape in HIP graphs (forward, forward+backward) '
                                 'and replay them: one launch per chunk instead of ~2 000, so the step does not depend on '
                                 'the host cores (2.8 s -> 2.0 s per step on a slow-host box, equal on a fast one; replay is '
                                 'bit-identical to eager execution, tests/test_30_full_step_gpu.py); falls back to eager '
                                 'execution if a capture fails.  0: eager launches')
        parser.add_argument('--depth_keep_gb', type=float, default=150.0,
                            help='HBM budget for keeping the depth net\'s autograd state of a step alive between its forward '
                                 '(phase 1) and its backward (phase 3), chunk by chunk, in HIP graphs: a kept chunk is not '
                                 'recomputed (MiDaS at 384x672: 1 GB per image, 95 GB for 48 pairs).  Chunks beyond the budget, '
                                 'or beyond what the MLP stashes leave free, take the no-graph forward + recompute path')
        parser.add_argument('--act_fp16', action='store_true',
                            help='BASELINE configs[4]: store the depth net\'s activations (and their gradients) as fp16 in HBM -- '
                                 'fp32 parameters, fp32 accumulation, fp32 loss sums; gradients carry a power-of-two loss scale kept on '
                                 'the device (csrc/a16.hip); a step whose fp16 gradients overflow skips its depth-net update.  Both '
                                 'depth nets: MiDaS (--midas) and the hourglass')
        parser.add_argument('--max_act_overflow_skips', type=int, default=25,
                            help='--act_fp16: consecutive steps skipped because an fp16 ACTIVATION overflowed after which the run '
                                 'stops with an error (a warning from the third on): the loss scale cannot cure that')
        parser.add_argument('--mlp_stash_fp16', action='store_true',
                            help='store the hidden activations of the scene-flow MLP stash as fp16 (3.2 instead of 5.7 KB per pixel and '
                                 'Euler step; the MLP weight gradients then see fp16-rounded activations, losses and input gradients '
                                 'are unchanged).  Implied by --act_fp16')
        parser.add_argument('--grad_buckets', type=int, default=4,
                            help='data parallel: the depth-net gradient (421 MB for MiDaS) is all-reduced as this many large '
                                 'buckets in flight at once, the Adam launch of a bucket overlapping the reduction of the next')
        return parser, set()

    # ------------------------------------------------------------------------------------
    def __init__(self, opt, loggers=None):
        super().__init__(opt, loggers)
        self.input_names = ['img', 'img_1', 'img_2', 'pose', 'intrinsic', 'mask_1', 'mask_2', 'R_1', 'R_1_T', 'R_2',
                            'R_2_T', 't_1', 't_2', 'flow_1_2', 'flow_2_1', 'K', 'K_inv', 'motion_seg_1',
                            'time_stamp_1', 'time_stamp_2', 'frame_id_1', 'frame_id_2', 'time_step']
        self.gt_names = []
        self.requires = list(set().union(self.input_names, self.gt_names))
        explicit = midas_resize_of(opt)
        if opt.midas:
            resize = [224, 384] if any(k in opt.dataset for k in ('real_video', 'korean', 'mctest', 'cube')) else None
            if explicit is not None:        # opt.midas_resize takes precedence over the reference's dataset-name rule
                resize = list(explicit)
            path = configs.midas_pretrain_path if os.path.exists(configs.midas_pretrain_path) else None
            if path is None:
                warnings.warn('MiDaS checkpoint %s not found: random weights' % configs.midas_pretrain_path)
            self.net_depth = MidasNet(path=path, non_negative=True, normalize_input=True, resize=resize)
        else:
            self.net_depth = HourglassModel_Embed(noexp=False, use_embedding=opt.use_embedding)
            if os.path.exists(configs.depth_pretrain_path):
                self.net_depth.net_depth.load_state_dict(torch.load(configs.depth_pretrain_path, map_location='cpu'))
            else:
                warnings.warn('depth checkpoint %s not found: random weights' % configs.depth_pretrain_path)
        if opt.use_cnn:      # the U-Net scene-flow network (:102-105), on the convolution kernels under autograd
            conv_setup = {'norm': 'none', 'activation': 'lrelu', 'pad_type': 'reflect', 'stride': 1}
            self.net_sceneflow = FCNUnet(conv_setup, n_down=getattr(opt, 'n_down', 3), feat=32, block_type='double_conv',
                                         in_channel=4 if opt.time_dependent else 3, out_channel=3)
        else:
            self.net_sceneflow = SceneFlowFieldNet(net_width=256, n_layers=4, time_dependent=opt.time_dependent,
                                                   N_freq_xyz=opt.n_freq_xyz, N_freq_t=opt.n_freq_t)
        self.bkwarp = BackwardWarp()
        self.unproject_points = unproject_ptcld()
        self.global_rank = getattr(opt, 'global_rank', 0)
        self._nets = [self.net_depth, self.net_sceneflow]
        self._metrics = ['flow_loss_1_2', 'loss', 'disp_loss_1_2', 'data_time', 'acc_reg', 'sf_loss']
        self.init_vars(add_path=False)
        self.init_weight(self.net_sceneflow, 'kaiming', 0.01, a=0.2)
        self.warp = scene_flow_projection_slack()
        self.depth_flow = flow_by_depth()
        self.visualizer = None
        self._flat_depth = self._flat_sf = None     # created by .to(device)
        self._optimizers = []
        self._depth = None              # the depth net's DepthRunner (graphs, kept slots, their memory), created by .to(device)
        self._cnn_px_measured = 0.0     # --use_cnn: measured autograd bytes per pixel and U-Net evaluation
        self.warm = False
        self.steps, self.steps_per_pair = 0, []     # Euler steps of the last training batch: largest count / per pair (caller's order)
        self._inv_perm = None        # set while self._input holds a batch in gap-grouped order (mixed frame gaps)
        share_frames_of(opt)         # (validated here; read again at every step, like the other opt attributes of the step)
        # statistics of the last training step: images the depth net ran on (2B; the padded number of distinct frames with
        # opt.share_frames), and that step's union {'U', 'U_pad', 'B'} (None without sharing)
        self.depth_images_last_step, self.last_union = 0, None

    # flat parameter buffers + fused Adam (or SGD, --optim sgd) replace the two torch.optim objects (:113-115)
    def to(self, device):
        super().to(device)
        if self.device.type != 'cuda':
            raise RuntimeError('dvd_hip Model runs on a GPU only (the reference CPU path is the oracle)')
        if self.opt.optim == 'sgd':
            def make(net, lr):
                return flat.FlatNet.sgd(net, lr, **self.optim_params)
        else:
            def make(net, lr):
                return flat.FlatNet(net, lr, self.optim_params['betas'])
        self._flat_depth = make(self.net_depth, self.opt.lr)
        self._flat_sf = make(self.net_sceneflow, self.opt.lr * self.opt.scene_lr_mul)
        self.optimizer_depth, self.optimizer_scene = self._flat_depth, self._flat_sf
        self._optimizers = [self._flat_depth, self._flat_sf]
        self._sf_grad_main = torch.zeros_like(self._flat_sf.grad)
        self._mlp = None if self.opt.use_cnn else self.net_sceneflow.kernels(
            self.device, stash_f16=bool(getattr(self.opt, 'mlp_stash_fp16', False) or getattr(self.opt, 'act_fp16', False)))
        self._gscale = None
        self._steps_skipped = 0
        if getattr(self.opt, 'act_fp16', False):
            self.net_depth.act_dtype = torch.float16
            self._gscale = ops.gscale_new(self.device)       # lives as long as the model: captured graphs hold its address
            # what each network's guarded Adam step subtracts from its step number (checkpoints carry the effective step)
            self._flat_depth.skip_count = self._gscale[5:6]
            self._flat_sf.skip_count = self._gscale[9:10]
            if self._mlp is not None:
                # the scene-flow MLP's fp16 stash shares the forward monitor: a hidden activation beyond fp16's range (stored
                # as Inf, contracted into the weight gradients) skips the step like a depth-net activation does
                self._mlp.set_forward_monitor(self._gscale[6:7])
        self._depth = DepthRunner(self.opt, self.net_depth, self._flat_depth, act_fp16=self._gscale is not None)
        if self._pending_optimizer_state is not None:      # checkpoint restored before .to() (train.py:256,279)
            self._apply_optimizer_state(self._pending_optimizer_state)
            self._pending_optimizer_state = None
        if parallel.is_distributed():      # every rank starts from rank 0's weights (train.py:290-292)
            parallel.broadcast_(self._flat_depth.flat)
            parallel.broadcast_(self._flat_sf.flat)

    def load_batch(self, batch, include_gt=True):
        self._inv_perm = None        # a freshly loaded batch is in the caller's order
        super().load_batch(batch, include_gt)

    # -- read-only views of the depth-net runner (the benchmark and the tools report them); valid before .to() as well ----
    def _chunk(self):
        """Images per depth-net chunk (depth_runner.images_per_chunk)."""
        return self._depth.chunk() if self._depth is not None else images_per_chunk(self.opt)

    @property
    def _pool_bytes(self):
        return self._depth.pool_bytes if self._depth is not None else 0

    @property
    def _depth_graphs(self):
        return self._depth.graphs if self._depth is not None else {}

    # ------------------------------------------------------------------------------------
    def _group_input(self, perm):
        """Bring the loaded batch (self._input) into gap-grouped order: ONE dvd_gather_pairs launch over every per-pair
        tensor.  The caller's batch dict is not touched; exports go back through the inverse (_caller_order)."""
        inp = self._input
        B = len(perm)
        names = [n for n in self.input_names if torch.is_tensor(getattr(inp, n, None)) and getattr(inp, n).dim() > 0 and
                 getattr(inp, n).shape[0] == B and getattr(inp, n).numel() > 0]
        perm_dev = torch.tensor(perm, dtype=torch.int32).to(self.device, non_blocking=True)
        for n, t in zip(names, ops.gather_pairs([getattr(inp, n) for n in names], perm_dev)):
            setattr(inp, n, t)
        inv = [0] * B
        for j, b in enumerate(perm):
            inv[b] = j
        self._inv_perm = torch.tensor(inv, dtype=torch.int32).to(self.device, non_blocking=True)

    def _caller_order(self, tensors):
        """dict of per-pair GPU tensors of the last step, in its gap-grouped order -> the same in the caller's pair order."""
        inv = getattr(self, '_inv_perm', None)
        if inv is None:
            return tensors
        B = inv.numel()
        keys = [k for k, v in tensors.items() if torch.is_tensor(v) and v.is_cuda and v.dim() > 0 and v.shape[0] == B]
        out = dict(tensors)
        out.update(zip(keys, ops.gather_pairs([tensors[k] for k in keys], inv)))
        return out

    # ------------------------------------------------------------------------------------
    def _train_on_batch(self, epoch, batch_ind, batch):
        opt = self.opt
        self._depth.begin_step()
        conv.set_grad_scale_state(self._gscale)      # the loss-scale state of THIS model's fp16 gradients (None: fp32 storage)
        if self._gscale is not None:
            # the forward monitor counts for THIS step's forward passes only: warm-up epochs, validation and inference fold
            # into it too and never reach dvd_gscale_end -- a stale overflow of theirs skipped the next real step
            ops.gscale_step_begin(self._gscale)
        self.warm = warm = epoch <= opt.warm_sf
        self.net_depth.eval()                        # BN statistics are never updated (:157,168 / hourglass.py:200-208)
        for p in self.net_depth.parameters():
            p.requires_grad = not warm
        self._flat_sf.zero_grad()
        self._sf_grad_main.zero_()
        if not warm:
            self._flat_depth.zero_grad()
        for k, v in batch.items():                   # strip the DataLoader dimension (:177-179)
            if type(v) != list:
                batch[k] = v.squeeze(0)

        # ---- the plan (models/sf_step.py).  Pairs of different frame gaps: everything below works on the batch in gap-grouped
        #      order (gap_plan), each group integrated over its own number of Euler steps; a uniform batch is ONE group in the
        #      caller's order
        share, share_quantum = share_frames_of(opt)
        steps, steps_pp, time_step, ids = sf_step.steps_per_pair(batch, with_ids=share)
        self.steps, self.steps_per_pair = steps, steps_pp
        self.load_batch(batch)
        inp = self._input
        B, _, H, W = inp.img_1.shape
        HW, dev = H * W, self.device
        do_reg = opt.interp_steps > 0 and (not warm or opt.warm_reg) and opt.acc_mul > 0
        mlp_bytes = None if self._mlp is None else (self._mlp.stash_floats(HW) * 4, self._mlp.gstash_floats(HW) * 4)
        plan = sf_step.plan_step(steps_pp, HW, do_reg, mlp_bytes, sf_step.cnn_bytes_per_px(self._cnn_px_measured, opt), opt)
        if plan['perm'] != list(range(B)):
            self._group_input(plan['perm'])
        schedule, needs_late = sf_step.choose_schedule(plan, B, opt.use_cnn, bool(int(getattr(opt, 'mlp_recompute', 1))))

        # ---- the step's image sets (images, frame ids, first slot), and phase 1 over them: depth maps; the autograd state of
        #      as many chunks as fit stays alive for phase 3 (kept slots), the rest is a no-graph forward that phase 3 recomputes
        keeping = not (warm or not getattr(opt, 'depth_graphs', 1) or float(getattr(opt, 'depth_keep_gb', 150.0)) <= 0)
        if keeping:
            self._depth.choose_chunk(B, HW, plan['reserve'], dev)
        fid1, fid2 = (None, None) if opt.midas else (inp.frame_id_1, inp.frame_id_2)      # (the hourglass's per-frame embedding)
        n_slots, tab, union = -(-B // self._chunk()), None, None
        self.depth_images_last_step, self.last_union = 2 * B, None
        if share:
            # opt.share_frames: the depth net runs once per DISTINCT frame of the step (same id = same image: trusted).  The
            # union rows (padded to a multiple of opt.share_quantum with copies of row 0) are one image set in slots 0..;
            # phase 3 sums the depth gradients of every image that shows a frame before the one backward
            perm = plan['perm']
            tab = ops.UnionTables(frame_union.plan_union([ids[0][p] for p in perm], [ids[1][p] for p in perm],
                                                         share_quantum), dev)
            union = (ops.union_gather(inp.img_1.contiguous(), inp.img_2.contiguous(), tab),
                     None if fid1 is None else ops.union_gather(fid1.contiguous(), fid2.contiguous(), tab))
            n_slots = -(-tab.U_pad // self._chunk())
            self.depth_images_last_step, self.last_union = tab.U_pad, {'U': tab.U, 'U_pad': tab.U_pad, 'B': B}
        sets, n_slots_total = sf_step.image_sets(inp.img_1, fid1, inp.img_2, fid2, n_slots, union)
        if keeping:
            depths = [self._depth.forward_keep(img, fid, slot0, plan['reserve'], n_slots_total) for img, fid, slot0 in sets]
            self._depth.trim(dev, plan['reserve'])
        else:
            # (non-warm steps without kept slots: phase 3 recomputes every chunk's forward; a warm-up step has no depth-net backward)
            with (contextlib.nullcontext() if warm else ops.counting_recomputed()):
                depths = [self._depth.forward(img, fid) for img, fid, _ in sets]
        depth_1, depth_2 = depths if tab is None else ops.union_scatter(depths[0], tab)

        # ---- phase 2: geometry + scene-flow network + losses, forward and backward (sf_step.SfStep)
        step = sf_step.SfStep(opt, dev, self._mlp, self._flat_sf, self._sf_grad_main, self.net_sceneflow, inp, depth_1, depth_2,
                              plan, time_step, warm, do_reg, self._depth.free_hbm, self._cnn_px_measured)
        # ranks may hold different batch sizes / frame gaps: agree on the schedule (early or late normaliser)
        # and on the size of the global batch before the first data-dependent collective
        # (also agreed across ranks: does ANY rank still have to capture a depth-net graph in phase 3?  Then every rank keeps
        #  the MLP-gradient all-reduce out of flight until after phase 3, so the order of collectives is the same everywhere.
        #  A --use_cnn step never announces a capture)
        will_capture = not (warm or opt.use_cnn) and self._depth.backward_will_capture(*[(slot0, img) for img, _, slot0 in sets])
        late, n_global, capturing = parallel.agree_on_step_plan(dev, needs_late, B, will_capture)
        schedule = sf_step.agreed_schedule(schedule, late)
        if self._mlp is not None:
            self._last_chunks = list(plan['chunks'])
        scalars, inv = step.run(schedule, n_global)
        self._cnn_px_measured = step.cnn_px_measured
        return self._finish_step(epoch, batch_ind, batch, step, scalars, inv, schedule != 'late', capturing, sets, tab)

    def _finish_step(self, epoch, batch_ind, batch, step, scalars, inv, early_norm, capturing, sets, tab):
        """Phase 3 and the end of the step, for the MLP and the U-Net path alike.  early_norm: phase 2 has already normalised
        g_d1_main (regulariser included); else (SfStep.run_late) inv * main + reg is formed here.  sets: phase 1's image sets;
        tab: the union's index tables when they are ONE set (opt.share_frames), else None."""
        opt, warm, k = self.opt, step.warm, self._flat_sf
        # the MLP gradient all-reduce overlaps the depth-net backward, except in a step that still has to
        # capture the depth net's forward+backward graph (no collective in flight during a capture)
        h_sf = None if capturing else k.all_reduce_grads(async_op=True)

        # ---- phase 3: depth-net backward from the depth gradients
        if not warm:
            g_d1 = step.g_d1_main if early_norm else ops.scale_add(step.g_d1_main, step.g_d1_main, scale_ptr=inv, b=step.g_d1_reg)
            g_d2 = ops.scale_add(step.g_d2_main, step.g_d2_main, scale_ptr=inv)
            # (opt.share_frames: ONE backward over the distinct frames, from the summed gradients)
            g_sets = [g_d1, g_d2] if tab is None else [ops.union_reduce(g_d1, g_d2, tab)]
            for (img, fid, slot0), g in zip(sets, g_sets):
                self._depth.backward(img, fid, g, slot0=slot0)
            # 421 MB (MiDaS) in --grad_buckets large all-reduces, each bucket's Adam launch overlapping the next
            # bucket's reduction
            skip = None
            if self._gscale is not None:
                # fp16 gradients: did this step stay inside fp16 range?  (device-side decision; with several ranks an
                # overflow anywhere skips the update everywhere)
                if parallel.is_distributed():          # both monitors: gradients [3], forward activations [6]
                    both = torch.stack([self._gscale[3], self._gscale[6]])
                    torch.distributed.all_reduce(both, op=torch.distributed.ReduceOp.MAX)
                    self._gscale[3:4].copy_(both[0:1])
                    self._gscale[6:7].copy_(both[1:2])
                ops.gscale_end(self._gscale)
                skip = self._gscale[4:5]
            self._flat_depth.all_reduce_and_step(getattr(opt, 'grad_buckets', 4), skip_ptr=skip)
        if capturing:
            k.all_reduce_grads()
        if h_sf is not None:
            h_sf.wait()
        # (fp16 activations: an ACTIVATION that overflowed fp16 makes the depth map, and with it the scene-flow network's
        #  gradient, non-finite: that step skips BOTH updates.  A mere loss-scale overflow of the depth net's fp16 GRADIENTS
        #  leaves the depth maps finite and the scene-flow network's fp32 gradients valid: its update goes through -- the
        #  (flag, count) pair [8], [9] of the loss-scale state counts activation overflows only)
        k.step(skip_ptr=None if (warm or self._gscale is None) else self._gscale[8:10])

        host = self._step_scalars_to_host(scalars, step.sums, warm)    # the only host synchronisation of the step
        acc_reg = opt.acc_mul * host[8] / (3.0 * step.n_global * step.HW + 1e-6) if step.do_reg else 0
        # --weight_steps scales the gradient only: the logged loss is the unweighted one (`**loss_data`
        # overwrites 'loss' at :226)
        batch_log = {'size': opt.batch_size, 'loss': host[1] / step.mul, 'total_loss': host[1] / step.mul,
                     'flow_loss_1_2': host[2], 'disp_loss_1_2': host[3], 'sf_loss': host[4], 'acc_reg': acc_reg}
        if self._gscale is not None:
            batch_log['steps_skipped'] = self._steps_skipped
        self._last = {'depth_1': step.depth_1, 'depth_2': step.depth_2, 'mask_sum': host[5], 'sf_all': step.sf_all,
                      'mseg': step.mseg}
        self._export_train_visuals(epoch, batch_ind, batch)
        return batch_log

    def _step_scalars_to_host(self, scalars, sums, warm):
        """The step's ONE device -> host copy: the loss scalars, the regulariser sum and -- with fp16 activation storage --
        the loss-scale state's skip counters, so that a run whose updates are being skipped says so (batch_log
        'steps_skipped') instead of logging a loss that never moves.  An fp16 ACTIVATION overflow has no
        back-off (the loss scale is not at fault): a warning from the third consecutive skipped step on, an error after
        --max_act_overflow_skips (default 25) of them."""
        if self._gscale is None:
            return torch.cat([scalars, sums[4:5]]).tolist()
        host = torch.cat([scalars, sums[4:5], self._gscale[4:6], self._gscale[8:11]]).tolist()
        self._steps_skipped = int(host[10])
        run = 0 if warm else int(host[13])
        if run >= 3:
            limit = int(getattr(self.opt, 'max_act_overflow_skips', 25))
            msg = ('fp16 activation storage: an activation of the depth network left fp16\'s range in %d consecutive steps; '
                   'every one of them was skipped (%d skipped steps in all).  The loss scale cannot cure this: lower the '
                   'learning rate or run without --act_fp16' % (run, self._steps_skipped))
            if run >= limit:
                raise RuntimeError(msg)
            warnings.warn(msg)
        return host

    # -- the reference's `pred` dict and its export (scene_flow_motion_field.py:201-225, video_base.py:105-126) ----
    def _export_train_visuals(self, epoch, batch_ind, batch):
        opt = self.opt
        every = getattr(opt, 'vis_every_train', 0)
        if not every or np.mod(epoch, every) != 0:
            return
        indx = batch_ind if getattr(opt, 'vis_at_start', False) else getattr(opt, 'epoch_batches', 0) - batch_ind
        if indx > getattr(opt, 'vis_batches_train', 0):
            return
        pred = {k: v.data.cpu().numpy() for k, v in self._predict_on_batch(is_train=True).items()}
        outdir = join(self.full_logdir, 'visualize', 'epoch%04d_train' % epoch)
        makedirs(outdir, exist_ok=True)
        output = self.pack_output(pred, batch)
        if self.global_rank == 0 and self.visualizer is not None:
            self.visualizer.visualize(output, indx + (1000 * epoch), outdir)
        np.savez(join(outdir, 'rank%04d_batch%04d' % (self.global_rank, batch_ind)), **output)

    def pack_output(self, pred_all, batch):
        """video_base.py:105-126, key for key."""
        if 'pair_path' in batch:
            batch_size = len(batch['pair_path'])
        else:                                          # synthetic batches carry no paths
            batch_size = int((batch['img'] if 'img' in batch else batch['img_1']).shape[0])
        if 'img' not in batch:
            img_1, img_2 = batch['img_1'].cpu().numpy(), batch['img_2'].cpu().numpy()
        else:
            img_1 = img_2 = batch['img']
            if torch.is_tensor(img_1) and img_1.is_cuda:       # a device-resident item (datasets/frame_store.py): np.savez wants host data
                img_1 = img_2 = img_1.cpu().numpy()
        output = {'batch_size': batch_size, 'img_1': img_1, 'img_2': img_2, **pred_all}
        if 'img' not in batch:
            flows = {'flow_1_2': self._input.flow_1_2, 'flow_2_1': self._input.flow_2_1}
            if flows['flow_1_2'].is_cuda and flows['flow_1_2'].shape[0] == batch_size:
                flows = self._caller_order(flows)
            output['flow_1_2'] = flows['flow_1_2'].cpu().numpy()
            output['flow_2_1'] = flows['flow_2_1'].cpu().numpy()
            if 'depth_pred_1' in batch:
                output['depth_nn_1'] = batch['depth_pred_1'].cpu().numpy()
        else:
            for src, dst in (('depth_pred', 'depth_nn'), ('depth_mvs', 'depth_gt'), ('cam_c2w', 'cam_c2w'), ('K', 'K')):
                if src in batch:
                    output[dst] = batch[src].cpu().numpy()
        output['pair_path'] = batch.get('pair_path', [])
        return output

    # ------------------------------------------------------------------------------------
    def _predict_on_batch(self, is_train=True):
        """Inference path (is_train=False, :265-275): depth + unprojection + one MLP evaluation."""
        if is_train:
            return self._train_pred()
        inp = self._input
        fid = inp.frame_id_1 if not self.opt.midas else None
        depth = self._depth.forward(inp.img, fid)
        P = ops.unproject(depth, inp.R_1, inp.t_1, inp.K_inv, planar=True)
        if self.opt.use_cnn:
            with torch.no_grad():
                return {'depth': depth, 'sf_1_2': sf_step.sf_net_cnn(self.net_sceneflow, self.opt, P, inp.time_stamp_1)}
        sf = torch.empty_like(P)
        self._mlp.pack(self.net_sceneflow.parameter_list()[0::2], self.net_sceneflow.parameter_list()[1::2])
        ts = inp.time_stamp_1 if self.opt.time_dependent else None
        self._mlp.forward(P, ts, 0.0, 1.0 / self.opt.sf_mag_div, sf_out=sf)
        return {'depth': depth, 'sf_1_2': sf}

    # -- after the optimisation: whole-video depth and long-range tracks (models/tracks.py) -----------------------------------
    def video_depth(self, frames):
        """Refined depth of a whole video -> [N,1,H,W] on the device.  frames: the validation view (FrameStore.frames(b), or
        any iterable of `vali` items); every batch goes through the depth net exactly as _predict_on_batch(is_train=False)
        runs it (eval mode, no autograd state), so the result is that path's 'depth', frame by frame, bit for bit."""
        return tracks.video_depth(self, frames)

    def track(self, store, start, n_steps, depth=None, chunk=None, n_back=0, n_iter=4):
        """Where the pixels of the frames `start` are 1 .. n_steps frames later: the scene-flow MLP integrated by Euler steps
        (forward_sf_net_multi_step, :360-367) from the un-projected refined depth, and every step projected into the camera of
        its target frame.  store: the video's FrameStore; depth: [N,1,H,W] refined depth (default: video_depth of the store).
        Returns device tensors, step-major (T1 = n_steps + 1, B = len(start); step 0 is the start frame itself):
          points [T1,B,3,H,W]  world positions;  uv [T1,B,H,W,2], z [T1,B,H,W]  pixel position and depth in frame start + k
          depth_at [T1,B,H,W]  that frame's refined depth at uv (0 behind the camera);  inside uint8 [T1,B,H,W]  in front of
          the camera and within the image;  steps_valid int32 [B]  steps with a target frame -- rows past it are zero.
        chunk: start frames per pass of the chain (default: 8 GB of world points); the result does not depend on it.  The
        un-masked field drives the chain, as in training (--use_motion_seg only masks the flow handed to the warp);
        --use_cnn raises NotImplementedError.
        n_back >= 1 makes the tracks two-sided: the field is also run backwards, each Euler step inverted by n_iter fixed-point
        iterations (ops.invert_step).  Then T1 = n_back + 1 + n_steps, row n_back is the start frame, row j is
        frame start + j - n_back (rows before frame 0 are zero), n_steps = 0 is allowed, and three keys are added: origin
        (= n_back, a Python int), steps_valid_back int32 [B] (= min(n_back, start)) and resid fp32 [n_back,B] -- per backward
        step j (row j - 1) the largest move of a point in the last iteration, 0 where there is no frame."""
        return tracks.track(self, store, start, n_steps, depth=depth, chunk=chunk, n_back=n_back, n_iter=n_iter)

    def track_points(self, store, queries, n_steps=None, n_back=None, depth=None, z_tol=0.05, n_iter=4, chunk=None):
        """Where chosen points of the video are in its other frames (models/point_tracks.py): `track` for a list of queries
        instead of every pixel of whole frames.  queries: a host array [Q,3] of (frame, x, y) in the store's pixel coordinates,
        pixel centres at integers, sub-pixel positions welcome, any mix of frames; ValueError for an empty list, a frame that is
        not integral or not a frame, a position outside [0,W-1] x [0,H-1], or a NaN.  Each query is seeded from the refined depth
        of its own frame at its own position (ops.point_seed: direct bilinear taps, then the per-pixel body of ops.unproject),
        carried n_steps Euler steps forwards and n_back inverse steps (n_iter fixed-point iterations each) backwards by the
        scene-flow MLP kernels -- one launch of Q points per step -- and every row is projected into the camera of ITS frame by
        one ops.point_project launch (csrc/point_track.hip).
          n_steps  default N - 1 - min(frame);  n_back  default max(frame): together the whole video on both sides of every
                   query; n_back = 0 is the "query first" protocol of the tracking benchmarks
          depth    [N,1,H,W] refined depth (default: video_depth of the store);  z_tol: a point deeper than the target frame's
                   depth * (1 + z_tol) is occluded there (evaluate's rule)
          chunk    queries per pass (default: 8 GB of world points); the result does not depend on it
        All queries take all steps; the rows that fall off the video are masked by the projection -- at most 2 x wasted MLP work
        on a tiny workload.  Returns device tensors, row-major (T1 = n_back + 1 + n_steps; row j of query q is frame
        frame[q] + j - n_back):
          points [T1,3,Q]  world positions;  uv [T1,Q,2], z, depth_at [T1,Q]  as `track` defines them;  inside uint8 [T1,Q]
          visible uint8 [T1,Q]  inside and not occluded;  target int32 [T1,Q]  the frame a row looks into, -1 where there is
          none or the query is not ok (such a row is all zeros; `target` scatters the rows frame-major in one line)
          ok uint8 [Q]  the query's depth is finite and > 0;  origin  = n_back (a Python int);  resid fp32 [n_back]  per
          backward step the largest move of a point in the last iteration.
        An integer query has, bit for bit, what `track` gives that pixel.  Nothing synchronises with the device; --use_cnn
        raises NotImplementedError."""
        return point_tracks.track_points(self, store, queries, n_steps=n_steps, n_back=n_back, depth=depth, z_tol=z_tol,
                                         n_iter=n_iter, chunk=chunk)

    def score_tracks(self, store, queries, gt_uv, gt_state, thresholds=(1, 2, 4, 8, 16), px_scale=(1.0, 1.0), **track_args):
        """How well do the tracks follow annotated trajectories? (models/point_tracks.py)  The TAP-Vid protocol of the
        long-range tracking benchmarks: `track_points` of the queries, then ONE fused kernel (ops.point_score) that counts in
        64-bit integers.
          gt_uv    [Q,N,2] the annotated position of every query's track in every frame (host array or GPU float32 tensor);
          gt_state [Q,N]  0 visible, 1 occluded, >= 2 not annotated.  point_tracks.queries_first / queries_strided make the
                   queries of either protocol from annotations [T,N,2] and return the track of each, so gt_uv[track] repeats
                   the ground truth per query
          thresholds  five distances in pixels;  px_scale = (sx, sy) scales the position error before it is compared: a
                   benchmark that scores in a 256 x 256 raster is evaluated with (256 / W, 256 / H)
          track_args  n_steps, n_back, depth, z_tol, n_iter, chunk of `track_points`
        A row counts iff it has a frame, is not the query itself and is annotated.  Returns, float64 on the device and NaN
        where a denominator is 0:
          occlusion_accuracy  n_occ_agree / n_eval (predicted `visible` equals annotated visible)
          pts_within [5]  per threshold the visible points closer than it, / n_gt_visible;  average_pts_within
          jaccard [5]  n_tp / (n_gt_visible + n_fp): true positives are visible, predicted visible and within; false positives
                   predicted visible but occluded or not within;  average_jaccard
          mean_err  mean position error of the visible points, each capped at 1024;  n_eval, n_gt_visible int64
          by_offset  the same quantities per slab row [T1]: row j is temporal distance j - origin, the accuracy-over-distance
                   curve a long-range tracker is judged by
          sums int64 [T1,19], shift  the kernel's exact sums (ops.POINT_SUMS);  tracks  the `track_points` result
        Bitwise reproducible; nothing synchronises with the device.  --use_cnn raises NotImplementedError."""
        return point_tracks.score_tracks(self, store, queries, gt_uv, gt_state, thresholds=thresholds, px_scale=px_scale,
                                         **track_args)

    def render(self, store, target, sources, cam_c2w=None, K=None, depth=None, advect=True, chunk=None, valid=None,
               backward=False, n_iter=4, inpaint=False, bg_power=2, **splat_params):
        """The video re-rendered from its own geometry and motion (models/render.py): for every view v the frames sources[v],
        un-projected with their refined depth, pushed along the scene-flow field to the time of frame target[v] (target[v] - f
        Euler steps, as in `track`) and splatted into one image with a soft z-buffer (ops.splat, csrc/splat.hip).
          target   V frame indices: the time of each view and, by default, its camera (rows of store.tables)
          cam_c2w [V,4,4], K [V,3,3]  (either or both; host arrays) novel cameras: camera-to-world poses / intrinsics, turned
                   into table rows by the store's own code
          sources  V lists of frame indices; with advect none later than its target, unless backward
          backward True lets a source f be later than its target g: it is carried back by f - g inverse Euler steps of
                   n_iter fixed-point iterations each (ops.invert_step), so a view is filled from both sides
          depth    [N,1,H,W] refined depth (default: video_depth of the store);  valid: optional uint8 [N,H,W], 0 drops a pixel
          advect   False holds time: the frames are drawn as they are (a static scene; the only mode under --use_cnn, where
                   True raises NotImplementedError)
          chunk    source images integrated per pass (default: 8 GB of world points); the result does not depend on it
          splat_params  z_near, z_tol, w_tap, w_min, value_bound (default 1: colours), fill of ops.splat
          inpaint  True closes what no source reached (splat gaps, never-seen regions, the borders of a moved camera) by
                   push-pull filling (ops.fill_holes, csrc/fill.hip; three more launches): image and depth jointly as 4
                   channels, known = hit.  A hit pixel weighs depth^bg_power, bg_power 0 .. 4, so with bg_power > 0 the deeper
                   surface dominates a coarse pixel that mixes foreground and background, which is what a disocclusion wants;
                   2 is an untuned default.  The result gains `level` uint8 [V,H,W] (0 hit, k >= 1 the pyramid level of the
                   nearest data, 255 a view nothing hit, which stays `fill`, depth included); image and depth keep their bits
                   at hit pixels and are then views of one [V,4,H,W] tensor; hit and weight are unchanged.
        Returns device tensors: image [V,3,H,W], depth [V,1,H,W] (the nearest surface, 0 where nothing landed), weight
        [V,1,H,W] (summed bilinear weight) and hit uint8 [V,H,W].  Bitwise reproducible; nothing synchronises with the device."""
        return render.render(self, store, target, sources, cam_c2w=cam_c2w, K=K, depth=depth, advect=advect, chunk=chunk,
                             valid=valid, backward=backward, n_iter=n_iter, inpaint=inpaint, bg_power=bg_power,
                             **splat_params)

    def evaluate(self, store, start=None, n_steps=None, depth=None, chunk=None, maps=False, z_tol=0.05):
        """How consistent are the refined depth, the scene-flow field, the cameras and the optical flow? (models/evaluate.py)
        The pixels of the frames `start` (default: every frame but the last) are pushed along the field for n_steps frames
        (default: the largest gap of the store's catalogue), as in `track`, and every step is compared with the frame it lands
        in by one fused kernel (ops.eval_tracks, csrc/eval.hip).  depth: [N,1,H,W] refined depth (default: video_depth of the
        store); chunk: start frames per pass, the result does not depend on it; z_tol: a point deeper than the target's depth
        * (1 + z_tol) is occluded.  Returns device tensors (K = n_steps, B = len(start); row k - 1 is step k):
          sums int64 [K,B,6], shift   the kernel's exact sums (n_inside, n_occluded, rel, photo, n_flow, epe; values * 2^shift)
          n_inside, n_occluded, n_flow  int64 [K,B]: points that land inside the target image, those of them behind a nearer
                   surface, and points with a valid optical flow of the pair (start, start + k) in the store
          depth_rel, photo  float64 [K,B]: mean |z - d| / d and mean L1 colour difference over the seen points
          flow_epe  float64 [K,B]: mean end-point distance between the induced motion and the stored flow (NaN without pairs)
          by_step  the three means and `occluded` (n_occluded / n_inside) pooled over the start frames, float64 [K]
          disp_mse  float64 [N]: _vali_on_batch's disparity MSE against depth_mvs, frame by frame
          maps     (maps=True) float32 [K,B,3,H,W]: rel, photo, epe per pixel, -1 where the point does not count
          steps_valid  int32 [B]
        Bitwise reproducible; nothing synchronises with the device.  --use_cnn raises NotImplementedError."""
        return evaluate.evaluate(self, store, start=start, n_steps=n_steps, depth=depth, chunk=chunk, maps=maps, z_tol=z_tol)

    def score_depth(self, store, depth=None, gt=None, align='median_video', regions=True, mask=None, maps=False):
        """How close is the refined depth to the ground truth of the frame files? (models/score_depth.py)  The converse of
        `evaluate`: the numbers a paper reports, after aligning the prediction to the ground truth by one scale.
        depth: [N,1,H,W] (default: video_depth of the store); gt: [N,1,H,W] (default: store.depth_mvs); align: 'none' (scale
        1), 'median_frame' (per frame the median of gt / depth over its countable pixels) or 'median_video' (one median over
        the countable pixels of all frames) -- exact medians from ops.ratio_median (csrc/select.hip); regions: split by the
        store's motion segmentation where it has one; mask: uint8 or bool [N,H,W], non-zero = allowed.  A pixel counts iff gt > 1e-2,
        depth > 0, the scaled depth is finite and the mask allows it.  Returns device tensors (rows: all / static / dynamic):
          sums int64 [N,3,9], shift   the kernel's exact sums (ops.SCORE_SUMS; values * 2^shift);  scale fp32 [N];  n int64 [N,3]
          abs_rel, sq_rel, rmse, rmse_log, silog, d1, d2, d3  float64 [N,3], NaN where n = 0 (silog = mean l^2 - mean(l)^2)
          video    the same quantities (and n) as [3], from the sums pooled over the frames in int64
          maps, counted  (maps=True) float32 [N,3,H,W]: abs_rel, sq, l per pixel, and uint8 [N,H,W]: 1 where the pixel counts
        Bitwise reproducible; nothing synchronises with the device."""
        return score_depth.score_depth(self, store, depth=depth, gt=gt, align=align, regions=regions, mask=mask, maps=maps)

    def filter_depth(self, store, frames=None, radius=4, weights='gauss', sigma=None, mode='mean', tol=0.1, z_near=1e-3,
                     depth=None, chunk=None, n_iter=4, passes=1):
        """The refined depth made consistent over time (models/filter.py): every pixel of the frames `frames` (default: all)
        follows its own two-sided track (as `track` with n_back = n_steps = radius, 1 <= radius <= 16) into the neighbouring
        frames, reads the depth they claim where it lands, and one fused kernel (ops.track_filter, csrc/track_filter.hip) drops
        the neighbours in which the point is outside, occluded or in gross disagreement (z <= D (1 + tol), D <= z (1 + tol),
        z >= z_near) and fuses the ratios D / z of the rest with the pixel's own (ratio 1).
          weights  'gauss' (exp(-j^2 / (2 sigma^2)) at row distance j, sigma default radius / 2), 'box', or 2 radius + 1 values
          mode     'mean' (weighted) or 'median';  depth: [N,1,H,W] refined depth (default: video_depth of the store)
          chunk    frames per pass (default: 8 GB of world points); the result does not depend on it, and only one chunk's slab
                   of points is alive at a time;  n_iter: fixed-point iterations of a backward step, as in `track`
          passes   k > 1 filters k times, each pass reading the depth the one before wrote (frames must be None)
        The ratio is taken along the neighbour camera's ray and applied along the frame's own -- the usual approximation for
        small disagreements; tol = 0.1 and radius = 4 are untuned defaults.  Returns device tensors (B = len(frames)):
          depth [B,1,H,W]  the fused depth (a pixel whose depth is not > 0 keeps it);  ratio [B,1,H,W]  depth / input depth
          (the product over the passes);  count uint8 [B,H,W]  rows that counted, the frame's own included (0 where the depth
          is not > 0);  spread [B,1,H,W]  largest minus smallest counting ratio (count, spread: of the last pass);
          steps_valid, steps_valid_back int32 [B]  rows of the window that have a frame after / before.
        Feeds `evaluate(depth=..)` and `score_depth(depth=..)` as it is.  Bitwise reproducible; nothing synchronises with the
        device.  --use_cnn raises NotImplementedError."""
        return depth_filter.filter_depth(self, store, frames=frames, radius=radius, weights=weights, sigma=sigma, mode=mode, tol=tol,
                                   z_near=z_near, depth=depth, chunk=chunk, n_iter=n_iter, passes=passes)

    def _train_pred(self):
        """The reference's train-time `pred` dict (:243-264 + `sf_loss_pp` of :308), materialised on demand from the
        state of the last `_train_on_batch` (the fused step itself never builds these thirteen surfaces): same keys,
        shapes and values, forward only."""
        if getattr(self, '_last', None) is None:
            raise RuntimeError('the training forward is fused into _train_on_batch: run a step first')
        inp, last = self._input, self._last
        cams = {k: getattr(inp, k) for k in CAM_KEYS}
        sf = last['sf_all']
        if last['mseg'] is not None:
            sf = ops.mul_mask(torch.empty_like(sf), sf, last['mseg'])
        sflow = sf.permute(0, 2, 3, 1)[..., None, :].contiguous()
        with torch.no_grad():
            dflow = self.depth_flow(last['depth_1'], last['depth_2'], inp.flow_1_2, **cams)
            pred = self.warp(last['depth_1'], last['depth_2'], inp.flow_1_2, inp.flow_2_1, sflow_1_2=sflow,
                             sflow_2_1=sflow, **cams)
        pred['sf_1_2'] = sf
        pred['global_p1'] = dflow['global_p1'].squeeze(3).permute(0, 3, 1, 2)
        pred['sf_by_dep_1_2'] = dflow['sf_by_depth']
        pred['sf_loss_pp'] = torch.abs(dflow['sf_by_depth'].squeeze(3).permute(0, 3, 1, 2) - sf).sum(1)
        return self._caller_order(pred)      # (a step that mixed frame gaps ran in gap-grouped order)

    @staticmethod
    def depth2disp(depth):
        valid = (depth > 1e-2).float()
        return (1 / (depth + (1 - valid) * 1e-8)) * valid

    def _vali_on_batch(self, epoch, batch_idx, batch):
        """Disparity MSE against the MVS depth, optional export (models/video_base.py:72-103)."""
        self.eval()
        self.load_batch(batch)
        with torch.no_grad():
            pred = self._predict_on_batch(is_train=False)
            gt = batch['depth_mvs'].to(self.device)
            vali = gt > 1e-2
            loss = torch.nn.functional.mse_loss(self.depth2disp(pred['depth']) * vali, self.depth2disp(gt) * vali).item()
        every = getattr(self.opt, 'vis_every_vali', 0)
        if every and np.mod(epoch, every) == 0 and batch_idx < getattr(self.opt, 'vis_batches_vali', 0):
            pred = {k: v.cpu().numpy() for k, v in pred.items()}
            outdir = join(self.full_logdir, 'visualize', 'epoch%04d_vali' % epoch)
            makedirs(outdir, exist_ok=True)
            output = self.pack_output(pred, batch)
            if self.global_rank == 0 and self.visualizer is not None:
                self.visualizer.visualize(output, batch_idx + (1000 * epoch), outdir)
            np.savez(join(outdir, 'rank%04d_batch%04d' % (self.global_rank, batch_idx)), **output)
        return {'size': batch['img'].shape[0], 'loss': loss}

    def test_on_batch(self, batch_idx, batch):
        """models/video_base.py:128-155: predict, pack, cache, write `<output_dir>/epoch<e>_test/batch%04d.npz`."""
        if not hasattr(self, 'test_cache'):
            self.test_cache = []
        self.eval()
        self.load_batch(batch)
        with torch.no_grad():
            pred = self._predict_on_batch(is_train=False)
        if not hasattr(self, 'test_loss'):
            self.test_loss = 0
        pred = {k: v.cpu().numpy() for k, v in pred.items()}
        ep = getattr(self.opt, 'epoch', 0)
        outdir = join(getattr(self.opt, 'output_dir', self.full_logdir or '.'), 'epoch%s_test' % ('best' if ep < 0 else '%04d' % ep))
        if not hasattr(self, 'outdir'):
            self.outdir = outdir
        makedirs(outdir, exist_ok=True)
        output = self.pack_output(pred, batch)
        self.test_cache.append(output.copy())
        if self.global_rank == 0 and self.visualizer is not None:
            self.visualizer.visualize(output, batch_idx, outdir)
        np.savez(join(outdir, 'batch%04d' % batch_idx), **output)
        return output
