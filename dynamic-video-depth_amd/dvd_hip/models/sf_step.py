"""Phase 2 of the scene-flow optimisation step and the ONE plan of a step (models/scene_flow_motion_field.py runs the step).

Pure planning, no GPU needed: `steps_per_pair` (Euler steps of every pair, the step's one device-to-host read), `gap_plan` /
`pairs_per_chunk` (gap groups and MLP chunks), `plan_step` (+ what phase 2 will allocate, `reserve`), `choose_schedule` /
`agreed_schedule` (which of the four schedules runs) and `image_sets` (what the depth net runs on in phases 1 and 3).
`SfStep` is phase 2 itself: geometry + scene-flow network + losses, forward and backward, one method per schedule behind
`run(schedule, n_global)`.  A new schedule or a new arrangement of image sets belongs here and nowhere else.
"""
import warnings

import numpy as np
import torch

from .. import ops, parallel

CAM_KEYS = ops.CAM_KEYS


def _time_step(batch):
    step = batch['time_step']
    return float(step.squeeze().item()) if torch.is_tensor(step) else float(step)


def integer_steps(batch):
    """(steps, time_step): Euler steps of this batch = round(mean(ts2 - ts1) / time_step) (:248-250), recomputed every step:
    consecutive batches mix frame gaps and allocators reuse addresses, so nothing about the tensors'
    identity says the gap is unchanged (one tiny reduction + read-back per 2 s step)."""
    time_step = _time_step(batch)
    gap = torch.mean(batch['time_stamp_2'].float() - batch['time_stamp_1'].float())
    return int((gap / time_step).round().long().item()), time_step


def batch_frame_ids(batch, B):
    """opt.share_frames: the frame ids of the batch's two image sets as two float tensors [B] (ids are whole numbers far
    below 2^24, exact in fp32), from `fid_1` / `fid_2` (frame-store items) or `frame_id_1` / `frame_id_2` (pair packs)."""
    for k1, k2 in (('fid_1', 'fid_2'), ('frame_id_1', 'frame_id_2')):
        if k1 in batch and k2 in batch:
            ids = [torch.as_tensor(batch[k]).reshape(-1) for k in (k1, k2)]
            if ids[0].numel() != B or ids[1].numel() != B:
                raise ValueError('opt.share_frames: %s / %s hold %d / %d ids for %d pairs' % (
                    k1, k2, ids[0].numel(), ids[1].numel(), B))
            return ids
    raise ValueError('opt.share_frames needs the frame id of every image: the batch has neither fid_1 / fid_2 nor '
                     'frame_id_1 / frame_id_2 (its keys: %s)' % sorted(batch))


def steps_per_pair(batch, with_ids=False):
    """(steps, steps_per_pair, time_step, ids): the Euler steps of every pair, round((ts2[b] - ts1[b]) / time_step) -- time
    stamps are constant per pair (datasets/davis_sequence.py) --, in the caller's order, with ONE device-to-host read.
    steps: for a uniform batch exactly integer_steps' value (the rounded mean gap, :248-250), else the largest count.
    with_ids (opt.share_frames): the same read also brings the frame ids of the two image sets, ids = (f1, f2) as lists of
    ints in the caller's order; else ids is None."""
    ts1, ts2 = batch['time_stamp_1'], batch['time_stamp_2']
    time_step = _time_step(batch)
    d = ts2.float() - ts1.float()
    B = int(d.shape[0]) if d.dim() > 0 else 1
    parts = [(d.reshape(B, -1)[:, 0] / time_step).round(), (torch.mean(d) / time_step).round().reshape(1)]
    if with_ids:
        parts += [t.to(d.device, non_blocking=True).float() for t in batch_frame_ids(batch, B)]
    both = torch.cat(parts).tolist()
    ids = None
    if with_ids:
        raw, both = both[B + 1:], both[:B + 1]
        if not all(np.isfinite(raw)) or any(v != int(v) or v < 0 or v >= 2 ** 24 for v in raw):
            raise ValueError('opt.share_frames: frame ids must be whole numbers in [0, 2^24), got %s' % (raw,))
        ids = ([int(v) for v in raw[:B]], [int(v) for v in raw[B:]])
    if not all(np.isfinite(both)):          # (the uniform path keeps whatever it does with such time stamps)
        steps = integer_steps(batch)[0]
        return steps, [steps] * B, time_step, ids
    per_pair, mean = [int(v) for v in both[:B]], int(both[B])
    if all(v == per_pair[0] for v in per_pair):
        return mean, [mean] * B, time_step, ids
    for b, v in enumerate(per_pair):
        if v < 1:
            raise ValueError('pair %d of a batch that mixes frame gaps has time stamps %g frames apart (%d Euler steps): '
                             'every pair needs at least one' % (b, float(ts2[b].flatten()[0] - ts1[b].flatten()[0]) / time_step, v))
    return max(per_pair), per_pair, time_step, ids


def pairs_per_chunk(B, budget_bytes, stash_bytes, gstash_bytes, steps, with_reg):
    """Pairs that go through the scene-flow MLP kernels at once: what --mlp_stash_gb (`budget_bytes`) holds of one pair's
    activation stashes (`stash_bytes` per Euler evaluation; the regulariser needs two) and backward scratch (`gstash_bytes`)."""
    per_pair = stash_bytes * max(steps, 2 if with_reg else 1) + gstash_bytes
    return int(max(1, min(B, budget_bytes // per_pair)))


def gap_plan(steps_per_pair, budget_bytes, stash_bytes, gstash_bytes, with_reg):
    """The schedule of a step whose pairs differ in frame gap.  steps_per_pair: Euler steps of every pair, in the caller's
    order.  Returns a dict:
      perm    the gap-grouped order: pairs sorted by their step count, stable (grouped[j] = caller[perm[j]]);
      groups  [(b0, b1, steps)] over the grouped order, one per distinct step count, ascending;
      chunks  [(b0, b1, steps)]: what goes through the MLP kernels at once -- pairs_per_chunk(...) pairs of ONE group, never
              across a group boundary;
      whole_bytes  stashes of a step that keeps every forward stash until its backward (sum_b steps_b stashes + the backward
                   scratch of the largest chunk + the regulariser's extra stash for the largest gap-1 chunk);
      chunk_bytes  stashes of the most expensive single chunk (late-normaliser / recompute schedules).
    A list whose entries are all equal gives ONE group, the identity permutation and the chunk list and byte figures of a
    uniform-gap step."""
    steps_per_pair = [int(v) for v in steps_per_pair]
    B = len(steps_per_pair)
    perm = sorted(range(B), key=lambda b: steps_per_pair[b])        # sorted() is stable
    groups, chunks = [], []
    b0 = 0
    while b0 < B:
        st = steps_per_pair[perm[b0]]
        b1 = b0
        while b1 < B and steps_per_pair[perm[b1]] == st:
            b1 += 1
        groups.append((b0, b1, st))
        Bc = pairs_per_chunk(B, budget_bytes, stash_bytes, gstash_bytes, st, with_reg)
        chunks.extend((c0, min(b1, c0 + Bc), st) for c0 in range(b0, b1, Bc))
        b0 = b1
    longest = max(c1 - c0 for c0, c1, _ in chunks)
    longest_gap1 = max([c1 - c0 for c0, c1, st in chunks if st == 1] or [0]) if with_reg else 0
    whole = sum(steps_per_pair) * stash_bytes + longest * gstash_bytes + longest_gap1 * stash_bytes
    chunk = max((c1 - c0) * (stash_bytes * max(st, 2 if with_reg else 1) + gstash_bytes) for c0, c1, st in chunks)
    return {'perm': perm, 'groups': groups, 'chunks': chunks, 'whole_bytes': whole, 'chunk_bytes': chunk}


def cnn_bytes_per_px(measured, opt):
    """Autograd state of ONE U-Net evaluation per pixel (--use_cnn): the measured value once a step has run; before that
    an a-priori figure that grows with the depth of the U-Net -- 2.6 KB per pixel was measured for n_down = 3 on the
    CPU path; the GPU path's Conv2dBlocks also keep a reflect-padded copy and a sliced .contiguous() copy of their
    inputs, hence the factor 1.5."""
    if measured > 0:
        return measured
    return 2600.0 * 1.5 * (1.0 + 0.15 * max(0, int(getattr(opt, 'n_down', 3)) - 3))


def plan_step(steps_per_pair, HW, do_reg, mlp_bytes, cnn_px, opt):
    """The ONE plan of a step, uniform gaps or mixed, MLP or U-Net: gap_plan with the MLP's stash sizes (mlp_bytes = (stash,
    gstash) bytes of one pair and evaluation; None under --use_cnn, where cnn_px = cnn_bytes_per_px counts) and --mlp_stash_gb, and
      reserve  what phase 2 will allocate (the room phase 1 leaves free): the MLP stashes of the whole batch if they are one
               chunk or fit --mlp_whole_batch_gb, else those of ONE chunk (late-normaliser / recompute schedules).  (Rounds
               1-5 reserved min(whole batch, the ceiling) in the chunked case too: 160 GB for 48 GB of stashes at BASELINE
               configs[4]'s 64 pairs, and not one depth-net slot was kept there.)
      Bc       the longest chunk (B if there is one chunk);
      whole    several chunks, but the forward stashes of the whole batch fit and stay alive until the backward."""
    B = len(steps_per_pair)
    if mlp_bytes is None:
        # --use_cnn: the whole batch goes through the U-Net at once (the plan gives the gap groups only); its autograd
        # state per pixel and evaluation is measured: one evaluation per pair and Euler step, + the regulariser's
        plan = gap_plan(steps_per_pair, 1.0, 1, 0, do_reg)
        plan['Bc'], plan['whole'] = B, False
        need = HW * cnn_px * (sum(steps_per_pair) + (B if do_reg else 0))
    else:
        plan = gap_plan(steps_per_pair, opt.mlp_stash_gb * 2 ** 30, mlp_bytes[0], mlp_bytes[1], do_reg)
        one = len(plan['chunks']) == 1
        fits = plan['whole_bytes'] <= float(getattr(opt, 'mlp_whole_batch_gb', 160.0)) * 2 ** 30
        plan['Bc'] = B if one else max(b1 - b0 for b0, b1, _ in plan['chunks'])
        plan['whole'] = fits and not one
        need = plan['whole_bytes'] if (one or fits) else plan['chunk_bytes']
    plan['reserve'] = need + 24 * B * HW * 4
    return plan


def choose_schedule(plan, B, use_cnn, mlp_recompute):
    """(schedule, needs_late_normaliser): this rank's schedule for phase 2 -- a method run_<schedule> of SfStep -- and what it
    tells parallel.agree_on_step_plan.  The MLP activation stashes bound how many pairs go through the MLP kernels at once
    (Bc).  If the forward stashes of the WHOLE batch fit the budget next to one chunk of backward scratch, the warp+loss kernel
    runs once over all pairs (one launch of B*H*W pixels fills the chip far better than B/Bc smaller ones); otherwise the
    recompute schedule, or with --mlp_recompute 0 one warp+loss launch per chunk and the normaliser late."""
    if use_cnn:
        return 'unet', False
    if plan['whole'] or plan['Bc'] >= B:
        return 'whole', False
    return ('recompute', False) if mlp_recompute else ('late', True)


def agreed_schedule(schedule, late):
    """Ranks may hold different batch sizes / frame gaps: a rank that needs the late normaliser makes every rank's MLP take it."""
    return 'late' if (late and schedule != 'unet') else schedule


def image_sets(img_1, fid_1, img_2, fid_2, n_slots, union=None):
    """([(images, frame ids, first slot)], slots of the whole step): what the depth net runs on in phase 1 and again in phase 3
    -- the two image sets of the pairs, n_slots slots each, or with opt.share_frames ONE set: union = (images, frame ids) of
    the distinct frames in n_slots slots."""
    if union is not None:
        return [(union[0], union[1], 0)], n_slots
    return [(img_1, fid_1, 0), (img_2, fid_2, n_slots)], 2 * n_slots


def sf_net_cnn(net, opt, p, t):
    """Model.forward_sf_net with --use_cnn (:346-357)."""
    x = torch.cat([p, t], 1) if opt.time_dependent else p
    return net(x) / opt.sf_mag_div


class SfStep:
    """Phase 2 of `Model._train_on_batch` (geometry + scene-flow network + losses, forward and backward): what its pieces share
    for ONE step, and the four schedules: three that the MLP's activation stashes allow, one for the U-Net.  Per-chunk data
    (stashes, backward scratch) stay locals of the schedule methods: they bound the step's peak HBM; the object itself does
    not outlive the step."""
    def __init__(self, opt, device, mlp, flat_sf, sf_grad_main, net, inp, depth_1, depth_2, plan, time_step, warm, do_reg,
                 free_hbm=None, cnn_px_measured=0.0):
        """mlp: the MLP's kernels object (None under --use_cnn), flat_sf / sf_grad_main: the scene-flow network's flat buffer
        and the main-path twin of its gradient, net: the network itself; plan: plan_step's.  --use_cnn: free_hbm(device) ->
        (free, total) bytes, and cnn_px_measured, which run_unet brings up to date for the caller to keep."""
        self.opt, self.device, self.mlp, self.flat_sf, self.sf_grad_main, self.net = opt, device, mlp, flat_sf, sf_grad_main, net
        self.inp, self.depth_1, self.depth_2 = inp, depth_1, depth_2
        self.time_step, self.warm, self.do_reg = time_step, warm, do_reg
        self.free_hbm, self.cnn_px_measured = free_hbm, cnn_px_measured
        B, _, H, W = inp.img_1.shape
        self.B, self.H, self.W, self.HW = B, H, W, H * W
        # frame gaps (gap_plan's groups): one group (0, B, steps) for a uniform batch; a mixed batch is in gap-grouped order and
        # `steps` is its largest count (groups ascend) -- every chunk of the MLP path carries its own
        self.groups, self.Bc, self.chunks = plan['groups'], plan['Bc'], list(plan['chunks'])
        self.steps = steps = self.groups[-1][2]
        self.mixed = len(self.groups) > 1
        # --weight_steps (:189-190): a uniform batch scales flow_mul / disp_mul of the ONE warp+loss launch and divides the
        # logged loss again; a mixed batch weights per gap group (group_mul) and logs the unweighted sums as they are
        self.mul = steps if (opt.weight_steps and not self.mixed) else 1
        self.disp_mode = 1 if opt.use_disp else (2 if opt.use_disp_ratio else 0)
        self.sums = torch.zeros(8, device=device)            # [S0..S3, sum|sf1-sf0|, 0, 0, 0]
        self.g_d1_main, self.g_d2_main = torch.empty_like(depth_1), torch.empty_like(depth_2)
        self.g_d1_reg = self.sf_all = self.g_sf_all = None    # allocated by run_late only / by begin_mlp or run_unet
        self.inv_div = 1.0 / opt.sf_mag_div
        self.mask_2 = inp.mask_2.reshape(B, H, W)
        # --use_motion_seg (:253-254): the integrated scene flow is multiplied by motion_seg_1 before the
        # warp; the un-masked field still drives the Euler chain and the regulariser
        self.mseg = inp.motion_seg_1.reshape(B, H, W) if opt.use_motion_seg else None
        self.cfg_all = self.warp_cfg(B)
        if mlp is not None:
            mlp.pack(net.parameter_list()[0::2], net.parameter_list()[1::2])

    def run(self, schedule, n_global):
        """Phase 2 by one of 'whole', 'recompute', 'late' (MLP) or 'unet' -> (scalars, inv): the loss scalars and the
        batch-global normaliser 1/(S0+1e-8) as a device scalar.  n_global: pairs of ALL ranks
        (parallel.agree_on_step_plan); the regulariser is a mean over them."""
        self.n_global = n_global
        self.reg_coef = self.opt.acc_mul / (3.0 * n_global * self.HW + 1e-6)
        if schedule != 'unet':
            self.begin_mlp()
        return getattr(self, 'run_' + schedule)()

    def warp_cfg(self, n_pairs, mul=None):
        opt = self.opt
        mul = self.mul if mul is None else mul
        return ops.warp_cfg(n_pairs, self.H, self.W, midas_mask=opt.midas, crit_l2=self.warm, disp_mode=self.disp_mode,
                            loss_on_sf=not opt.use_disp, flow_mul=opt.flow_mul * mul, disp_mul=opt.disp_mul * mul)

    def group_mul(self, steps):
        """--weight_steps in a mixed batch: the gradient weight of a pair with `steps` Euler steps (else None = self.mul)."""
        return steps if (self.opt.weight_steps and self.mixed) else None

    def begin_mlp(self):
        """The MLP path's batch-wide tensors.  self.chunks: gap_plan's (b0, b1, steps) list -- what goes through the MLP
        kernels at once; no chunk crosses a gap group --, self.Bc its longest chunk."""
        k, B, inp = self.flat_sf, self.B, self.inp
        self.gW_main = [k.view(self.sf_grad_main, 2 * i) for i in range(6)]
        self.gb_main = [k.view(self.sf_grad_main, 2 * i + 1) for i in range(6)]
        self.gW_reg = [k.view(k.grad, 2 * i) for i in range(6)]
        self.gb_reg = [k.view(k.grad, 2 * i + 1) for i in range(6)]
        self.P1_all = ops.unproject(self.depth_1, inp.R_1, inp.t_1, inp.K_inv, planar=True)
        self.sf_all = torch.zeros(B, 3, self.H, self.W, device=self.depth_1.device)
        self.g_sf_all = torch.empty_like(self.sf_all)

    def mlp_forward_chunk(self, b0, b1, steps, keep_first=None, acc=None, with_stash=True):
        """Euler integration of the scene flow over `steps` frames (:360-367).  keep_first: also
        return sf_0 and q = P1 + sf_0 of the first evaluation (the regulariser's sf_0, see below).
        acc: the tensor the integrated flow is accumulated into (default: this chunk of sf_all); with_stash=False: no
        activation stashes (the first pass of the recompute schedule)."""
        mlp = self.mlp
        ts = self.inp.time_stamp_1[b0:b1] if self.opt.time_dependent else None
        n_pix = (b1 - b0) * self.HW
        stashes, p_cur, first = [], self.P1_all[b0:b1], None
        acc = self.sf_all[b0:b1] if acc is None else acc
        for i in range(steps):
            st = mlp.new_stash(n_pix) if with_stash else None
            want_next = i + 1 < steps or (keep_first and i == 0)
            p_next = torch.empty_like(p_cur) if want_next else None
            # the regulariser's two evaluations ARE Euler evaluations 0 and 1 (see merged_backward_chunk): keep their
            # outputs (evaluation 0's only when it is not the accumulated flow itself)
            sf_i = torch.empty_like(p_cur) if (keep_first and i < 2 and steps > 1) else None
            mlp.forward(p_cur, ts, t_offset=i * self.time_step, out_scale=self.inv_div, sf_out=sf_i, p_next=p_next,
                        acc=acc, stash=st)
            if keep_first and i == 0:
                first = [sf_i, p_next, None]    # sf_i is None when steps == 1: sf_0 is the accumulated flow itself
            if keep_first and i == 1:
                first[2] = sf_i                 # sf_1 = MLP(P1 + sf_0, t_1 + dt)
            stashes.append(st)
            p_cur = p_next
        return (stashes, first) if keep_first is not None else stashes

    def warp(self, b0, b1, mul=None):
        inp, mseg = self.inp, self.mseg
        sf_used = self.sf_all[b0:b1]
        if mseg is not None:
            sf_used = ops.mul_mask(torch.empty_like(sf_used), sf_used, mseg[b0:b1])
        cfg = self.cfg_all if ((b0, b1) == (0, self.B) and mul is None) else self.warp_cfg(b1 - b0, mul)
        csum = torch.empty(4, device=self.sums.device)
        ops.warp_loss_fused(cfg, self.depth_1[b0:b1], self.depth_2[b0:b1], inp.flow_1_2[b0:b1], self.mask_2[b0:b1],
                            sf_used, {kk: getattr(inp, kk)[b0:b1] for kk in CAM_KEYS},
                            out=(csum, self.g_d1_main[b0:b1], self.g_d2_main[b0:b1], self.g_sf_all[b0:b1]))
        if mseg is not None:
            ops.mul_mask(self.g_sf_all[b0:b1], self.g_sf_all[b0:b1], mseg[b0:b1])
        self.sums[:4] += csum

    def mlp_backward_chunk(self, b0, b1, steps, stashes, gst):
        """Backward through the Euler chain: g_p_i = g_p_{i+1} + J_i^T (g_acc + g_p_{i+1})."""
        mlp, inv_div, gW_main, gb_main = self.mlp, self.inv_div, self.gW_main, self.gb_main
        nb, n_pix = b1 - b0, (b1 - b0) * self.HW
        g_p = None
        for i in reversed(range(steps)):
            g_new = torch.empty_like(self.P1_all[b0:b1])
            mlp.backward_dx(stashes[i], inv_div, self.g_sf_all[b0:b1], g_new, gst, gW_main[5], gb_main[5], (nb, self.H, self.W),
                            g_out2=g_p, g_p_add=g_p)
            mlp.backward_dw(stashes[i], gst, n_pix, gW_main[:5], gb_main[:5])
            g_p = g_new
        ops.unproject_backward(g_p, True, self.inp.R_1[b0:b1], self.inp.K_inv[b0:b1], out=self.g_d1_main[b0:b1], accumulate=True)

    def reg_chunk(self, b0, b1, gst):
        """Acceleration regulariser (:326-344), P1 un-detached."""
        mlp, inv_div, gW_reg, gb_reg, sums = self.mlp, self.inv_div, self.gW_reg, self.gb_reg, self.sums
        n_pix, shape = (b1 - b0) * self.HW, (b1 - b0, self.H, self.W)
        ts = self.inp.time_stamp_1[b0:b1] if self.opt.time_dependent else None
        P1 = self.P1_all[b0:b1]
        sa, sb = mlp.new_stash(n_pix), mlp.new_stash(n_pix)
        sf0, sf1, q = torch.empty_like(P1), torch.empty_like(P1), torch.empty_like(P1)
        mlp.forward(P1, ts, 0.0, inv_div, sf_out=sf0, p_next=q, stash=sa)
        mlp.forward(q, ts, self.time_step, inv_div, sf_out=sf1, stash=sb)
        g1 = torch.empty_like(P1)
        ops.acc_reg(sf0, sf1, self.reg_coef, g1, sums[4:5], accumulate=True)
        g_q = torch.empty_like(P1)
        mlp.backward_dx(sb, inv_div, g1, g_q, gst, gW_reg[5], gb_reg[5], shape)
        mlp.backward_dw(sb, gst, n_pix, gW_reg[:5], gb_reg[:5])
        g_P = torch.empty_like(P1)
        mlp.backward_dx(sa, inv_div, g1, g_P, gst, gW_reg[5], gb_reg[5], shape, gscale=-1.0, g_out2=g_q, g_p_add=g_q)
        mlp.backward_dw(sa, gst, n_pix, gW_reg[:5], gb_reg[:5])
        ops.unproject_backward(g_P, True, self.inp.R_1[b0:b1], self.inp.K_inv[b0:b1], out=self.g_d1_reg[b0:b1])

    def merged_backward_chunk(self, b0, b1, steps, stashes, first, gst, inv):
        """Main loss and acceleration regulariser through ONE backward of the first evaluation.

        The regulariser's sf_0 = MLP(P1, t_1) (:329-333) is the first Euler evaluation of the main
        path (:360-367: same points, same time, same weights), so its forward, stash, dX and dW
        passes are shared: with G = inv * g_sf (main, late normaliser already known) the first
        evaluation receives  G + g_p1 - g1 + g_q  where g1 = dR/dsf_1, g_q = J_b^T g1, and
        g_P1 = g_p1 + g_q + J_0^T(...).  One MLP evaluation per step less than the reference.
        From gap 2 on the regulariser's sf_1 = MLP(P1 + sf_0, t_1 + dt) (:335-338) is Euler evaluation 1 as well
        (:360-367), so that one is shared too (round 4): evaluation 1 receives G + g_p2 + g1, and a gap-k step costs k
        evaluations instead of the reference's k + 2."""
        mlp, do_reg, inv_div, sums, reg_coef = self.mlp, self.do_reg, self.inv_div, self.sums, self.reg_coef
        gW_reg, gb_reg = self.gW_reg, self.gb_reg
        n_pix, shape = (b1 - b0) * self.HW, (b1 - b0, self.H, self.W)
        ts = self.inp.time_stamp_1[b0:b1] if self.opt.time_dependent else None
        P1, g_sf = self.P1_all[b0:b1], self.g_sf_all[b0:b1]
        g_q = g1 = None
        shared1 = do_reg and steps > 1      # the regulariser's second evaluation is Euler evaluation 1 as well (:335-338 = :360-367)
        if do_reg:
            sf0 = first[0] if first[0] is not None else self.sf_all[b0:b1]
            g1 = torch.empty_like(P1)
            if shared1:
                ops.acc_reg(sf0, first[2], reg_coef, g1, sums[4:5], accumulate=True)
            else:
                sb, sf1 = mlp.new_stash(n_pix), torch.empty_like(P1)
                mlp.forward(first[1], ts, self.time_step, inv_div, sf_out=sf1, stash=sb)
                ops.acc_reg(sf0, sf1, reg_coef, g1, sums[4:5], accumulate=True)
                g_q = torch.empty_like(P1)
                mlp.backward_dx(sb, inv_div, g1, g_q, gst, gW_reg[5], gb_reg[5], shape)
                mlp.backward_dw(sb, gst, n_pix, gW_reg[:5], gb_reg[:5])
                del sb, sf1
        g_p = None
        for i in reversed(range(1, steps)):
            g_new = torch.empty_like(P1)
            g_o2 = g_p
            if shared1 and i == 1:          # evaluation 1's output also feeds the regulariser: + dR/dsf_1 (not normalised)
                g_o2 = g1 if g_p is None else ops.scale_add(torch.empty_like(P1), g1, b=g_p)
            mlp.backward_dx(stashes[i], inv_div, g_sf, g_new, gst, gW_reg[5], gb_reg[5], shape, scale_ptr=inv,
                            g_out2=g_o2, g_p_add=g_p)
            mlp.backward_dw(stashes[i], gst, n_pix, gW_reg[:5], gb_reg[:5])
            g_p = g_new
        extra, add = g_p, g_p                    # gradient reaching sf_0 besides G, and reaching P1 directly
        if shared1:                              # g_p already holds everything that reaches q = P1 + sf_0
            extra = ops.scale_add(torch.empty_like(P1), g1, scale=-1.0, b=g_p)          # g_p - g1
        elif do_reg:
            extra = ops.scale_add(torch.empty_like(P1), g1, scale=-1.0, b=g_q)          # -g1 + g_q
            add = g_q
        g_P = torch.empty_like(P1)
        mlp.backward_dx(stashes[0], inv_div, g_sf, g_P, gst, gW_reg[5], gb_reg[5], shape, scale_ptr=inv,
                        g_out2=extra, g_p_add=add)
        mlp.backward_dw(stashes[0], gst, n_pix, gW_reg[:5], gb_reg[:5])
        ops.unproject_backward(g_P, True, self.inp.R_1[b0:b1], self.inp.K_inv[b0:b1], out=self.g_d1_main[b0:b1], accumulate=True)

    def normaliser(self, sums):
        """All-reduce the loss sums -> the loss scalars and inv = 1/(S0+1e-8) as a device scalar."""
        parallel.all_reduce_sum_(sums)
        scalars = ops.loss_finalize(self.cfg_all, self.sums)
        return scalars, scalars[0:1]

    def warp_whole_batch(self):
        """ONE warp+loss launch over all pairs.  The batch-global normaliser is then known before the scene-flow network's
        backward: all-reduce the four loss sums now and hand inv to the backward kernels as a device scalar."""
        if self.mixed and self.opt.weight_steps:
            # per-pair weights: one launch per gap group, its flow_mul / disp_mul times the group's step count (the gradients
            # carry the weight); the loss sums are added as they are -- the logged losses are the unweighted ones (:226)
            for b0, b1, st in self.groups:
                self.warp(b0, b1, self.group_mul(st))
        else:
            self.warp(0, self.B)
        scalars, inv = self.normaliser(self.sums[:4])
        ops.scale_add(self.g_d1_main, self.g_d1_main, scale_ptr=inv)
        return scalars, inv

    def run_whole(self):
        """Schedule 1 of 4: the forward stashes of the whole batch stay alive until the backward."""
        gst = self.mlp.new_gstash(min(self.Bc, self.B) * self.HW)
        kept = [self.mlp_forward_chunk(b0, b1, n, keep_first=bool(self.do_reg)) for b0, b1, n in self.chunks]
        scalars, inv = self.warp_whole_batch()
        for (b0, b1, n), (st, first) in zip(self.chunks, kept):
            self.merged_backward_chunk(b0, b1, n, st, first, gst, inv)
            del st[:]
        del kept
        parallel.all_reduce_sum_(self.sums[4:])
        return scalars, inv

    def run_recompute(self):
        """Round 6: when the forward stashes of the whole batch do NOT fit (BASELINE configs[4]: 64 pairs at 768 x 1344 = 211 GB
        of stashes), the late-normaliser schedule costs 3 forward + 3 dX + 3 dW passes per pair and Euler step -- the
        regulariser cannot share the main path's backward while the normaliser is unknown.  The RECOMPUTE schedule runs the
        Euler chain once WITHOUT stashes for every pair (the cheapest form of the forward kernel), one warp+loss launch over
        the whole batch, and then per chunk the stashed forward again + the merged backward: 3 forward + 2 dX + 2 dW at
        gap 1 (2k + k + k instead of (k + 2) x 3 at gap k), same arithmetic as the whole-batch schedule (the recomputed
        evaluations are bit-identical: the forward kernel is deterministic).  --mlp_recompute 0 restores the late schedule."""
        gst = self.mlp.new_gstash(min(self.Bc, self.B) * self.HW)
        with ops.counting_recomputed():          # the stashed evaluations below are the ones the backward needs
            for b0, b1, n in self.chunks:
                self.mlp_forward_chunk(b0, b1, n, with_stash=False)
        scalars, inv = self.warp_whole_batch()
        for b0, b1, n in self.chunks:
            # the same evaluations again, stashed; their flow goes to a scratch accumulator (sf_all already holds it)
            st, first = self.mlp_forward_chunk(b0, b1, n, keep_first=bool(self.do_reg), acc=torch.zeros_like(self.sf_all[b0:b1]))
            self.merged_backward_chunk(b0, b1, n, st, first, gst, inv)
            del st[:], first
        parallel.all_reduce_sum_(self.sums[4:])
        return scalars, inv

    def run_late(self):
        """Per-chunk warp+loss launches (--mlp_recompute 0, or another rank needs it): the batch-global normaliser only exists
        after the last chunk; main-path gradients stay un-normalised in buffers of their own, the regulariser runs apart."""
        gst = self.mlp.new_gstash(min(self.Bc, self.B) * self.HW)
        self.g_d1_reg = torch.zeros_like(self.depth_1) if self.do_reg else None
        for b0, b1, n in self.chunks:
            st = self.mlp_forward_chunk(b0, b1, n)
            self.warp(b0, b1, self.group_mul(n))
            self.mlp_backward_chunk(b0, b1, n, st, gst)
            del st
            if self.do_reg:
                self.reg_chunk(b0, b1, gst)
        del gst
        scalars, inv = self.normaliser(self.sums)
        ops.scale_add(self.flat_sf.grad, self.sf_grad_main, scale_ptr=inv, b=self.flat_sf.grad)   # MLP gradient = inv * main + reg
        return scalars, inv

    def run_unet(self):
        """Phase 2 when the scene-flow network is the U-Net (networks/FCNUnet.py): the network runs under PyTorch autograd on
        this package's convolution kernels, the geometry and the losses stay the ONE fused warp+loss launch -- its scene-flow
        gradient is what the U-Net's backward starts from, with the batch-global normaliser applied as a device scalar.  The
        regulariser's first evaluation is Euler evaluation 0, as in the MLP path."""
        dev, inp, steps, time_step, do_reg = self.device, self.inp, self.steps, self.time_step, self.do_reg
        B, H, W, HW, sums = self.B, self.H, self.W, self.HW, self.sums
        P1 = ops.unproject(self.depth_1, inp.R_1, inp.t_1, inp.K_inv, planar=True).requires_grad_(True)
        ts = inp.time_stamp_1
        # the whole batch goes through the U-Net under autograd: fail early, with the numbers, instead of somewhere inside it
        evals = steps + (1 if do_reg else 0)        # (a mixed batch: its largest step count, an upper bound)
        px = cnn_bytes_per_px(self.cnn_px_measured, self.opt)
        need = B * HW * px * evals
        free, _total = self.free_hbm(dev)
        if need > free:
            msg = ('--use_cnn: the U-Net\'s autograd state for %d pairs at %dx%d (%d evaluations, %.0f B per pixel and '
                   'evaluation) needs %.1f GB, %.1f GB are free: use fewer pairs per step or a smaller --depth_keep_gb'
                   % (B, H, W, evals, px, need / 2 ** 30, free / 2 ** 30))
            if self.cnn_px_measured > 0:        # a measured footprint: fail early, with the numbers
                raise RuntimeError(msg)
            # an a-priori estimate must not reject a configuration that may well run
            warnings.warn(msg + ' (a-priori estimate: nothing has been measured yet, trying anyway)')
        mem0 = torch.cuda.memory_allocated(dev)
        with torch.enable_grad():
            accs, firsts = [], []
            for b0, b1, n in self.groups:        # mixed frame gaps: the U-Net runs per gap group (one group otherwise)
                whole = (b0, b1) == (0, B)
                sf_acc, p, t, sf0 = None, (P1 if whole else P1[b0:b1]), (ts if whole else ts[b0:b1]), None
                for i in range(n):
                    s_i = sf_net_cnn(self.net, self.opt, p, t)
                    sf0 = s_i if i == 0 else sf0
                    sf_acc = s_i if sf_acc is None else sf_acc + s_i
                    p, t = p + s_i, t + time_step
                accs.append(sf_acc)
                firsts.append(sf0)
            sf_acc, sf0 = (accs[0], firsts[0]) if len(accs) == 1 else (torch.cat(accs, 0), torch.cat(firsts, 0))
        # measured footprint of an evaluation (like DepthRunner.keep_per_px for the depth net's slots): the planner's next decisions
        # use it instead of the a-priori figure
        self.cnn_px_measured = max(self.cnn_px_measured, (torch.cuda.memory_allocated(dev) - mem0) / float(HW * sum(n * (b1 - b0) for b0, b1, n in self.groups)))
        self.sf_all = sf_acc.detach().contiguous()
        self.g_sf_all = g_sf = torch.empty_like(self.sf_all)
        scalars, inv = self.warp_whole_batch()
        ops.scale_add(g_sf, g_sf, scale_ptr=inv)
        sf_acc.backward(g_sf, retain_graph=bool(do_reg))        # parameter gradients land in the flat buffer's views
        if do_reg:
            with torch.enable_grad():
                sf1 = sf_net_cnn(self.net, self.opt, P1 + sf0, ts + time_step)
                dsum = (sf1 - sf0).abs().sum()
            sums[4:5] += dsum.detach()
            (dsum * self.reg_coef).backward()
        parallel.all_reduce_sum_(sums[4:])
        ops.unproject_backward(P1.grad.contiguous(), True, inp.R_1, inp.K_inv, out=self.g_d1_main, accumulate=True)
        return scalars, inv
