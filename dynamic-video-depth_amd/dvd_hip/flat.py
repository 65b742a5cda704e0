"""Flat parameter / gradient / optimiser-state buffers for one network.

Laid out for the MI355X step: every parameter of a net becomes a view into ONE
fp32 buffer (16-byte aligned segments), its `.grad` a view into a second one, and
the optimiser state lives in the same layout -- the two Adam moments, or SGD's one
momentum buffer (none at momentum 0).  That turns the optimiser into a single fused
HIP launch per net (dvd_adam_step / dvd_sgd_step) and the data-parallel exchange into a single
RCCL all-reduce per net instead of one message per tensor (the reference
broadcasts ~600 tensors one by one, train.py:290-292).
"""
import warnings

import torch

from . import ops, parallel


class FlatNet(object):
    """kind 'adam' (the constructor's default: FlatNet(module, lr, betas)) or 'sgd' (FlatNet.sgd(...))."""

    def __init__(self, module, lr, betas, eps=1e-8, kind='adam', momentum=0.0, dampening=0.0, weight_decay=0.0):
        if kind not in ('adam', 'sgd'):
            raise ValueError('FlatNet: unknown optimiser kind %r' % (kind,))
        self.module = module
        self.kind = kind
        self.lr, self.eps = float(lr), float(eps)
        self.betas = None if betas is None else (float(betas[0]), float(betas[1]))       # (Adam only)
        self.momentum, self.dampening, self.weight_decay = float(momentum), float(dampening), float(weight_decay)
        params = [p for p in module.parameters()]
        self.params = params
        dev = params[0].device
        offs, n = [], 0
        for p in params:
            offs.append(n)
            n += (p.numel() + 3) // 4 * 4        # keep every segment 16-byte aligned
        self.offsets, self.numel = offs, n
        self.flat = torch.zeros(n, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(n, device=dev, dtype=torch.float32)
        self.exp_avg = self.exp_avg_sq = self.momentum_buf = None
        if kind == 'adam':
            self.exp_avg = torch.zeros(n, device=dev, dtype=torch.float32)
            self.exp_avg_sq = torch.zeros(n, device=dev, dtype=torch.float32)
        elif self.momentum != 0.0:
            self.momentum_buf = torch.zeros(n, device=dev, dtype=torch.float32)
        for p, o in zip(params, offs):
            seg = self.flat[o:o + p.numel()].view_as(p)
            seg.copy_(p.data)
            p.data = seg
            p.grad = self.grad[o:o + p.numel()].view_as(p)
        self.step_count = 0
        # 1-element device view of "steps whose update was skipped so far" (the loss-scale state's count that the guarded
        # Adam kernel subtracts from `step`, csrc/elementwise.hip) or None.  step_count advances on every call, skipped or
        # not -- the host never learns of a skip inside the step -- so the EFFECTIVE step, the one torch.optim.Adam /
        # GradScaler mean and a checkpoint must carry, is step_count - skipped.
        self.skip_count = None
        self._count_only = None
        # SGD: which parameters the engine produced a gradient for (torch.optim.SGD skips a parameter whose .grad is None:
        # no decay, no momentum, no state).  Recorded by absorb_grads until the first step, then frozen; None = every
        # parameter (gradients written straight into the flat buffer, as the scene-flow MLP's kernels do).
        self._seen = None
        self._live = None            # frozen at the first SGD step: per-parameter bool
        self._ranges = None          # the live parameters' segments, merged into contiguous [lo, hi) element ranges
        self._state_params = set()   # parameter indices that hold a momentum buffer (torch.optim.SGD's state keys)

    @classmethod
    def sgd(cls, module, lr, momentum=0.0, dampening=0.0, weight_decay=0.0):
        """torch.optim.SGD(lr, momentum, dampening, weight_decay), no nesterov: flat, grad and -- if momentum != 0 -- one
        momentum buffer; no Adam moments."""
        return cls(module, lr, None, kind='sgd', momentum=momentum, dampening=dampening, weight_decay=weight_decay)

    def _skipped(self):
        return int(self.skip_count.item()) if self.skip_count is not None else 0

    def _skip_pair(self, skip_ptr):
        """What the guarded kernel reads: the caller's (flag, count) pair, or -- for a step that is never skipped itself (warm
        steps pass None) on a net that counts skips -- flag 0 and the current count, so that bias correction still takes the
        effective step.  One device copy, no host read."""
        if skip_ptr is not None or self.skip_count is None:
            return skip_ptr
        if self._count_only is None or self._count_only.device != self.skip_count.device:
            self._count_only = torch.zeros(2, device=self.skip_count.device, dtype=torch.float32)
        self._count_only[1:2].copy_(self.skip_count)
        return self._count_only

    def view(self, buf, p_index):
        p, o = self.params[p_index], self.offsets[p_index]
        return buf[o:o + p.numel()].view_as(p)

    def zero_grad(self):
        self.grad.zero_()
        for p, o in zip(self.params, self.offsets):      # autograd may have replaced .grad; re-attach
            if p.grad is None or p.grad.data_ptr() != self.grad.data_ptr() + 4 * o:
                p.grad = self.grad[o:o + p.numel()].view_as(p)

    # -- gradient accumulation over several backward passes (depth-net chunks) ----------------
    # With `.grad` pre-attached autograd adds every parameter's gradient with its own tiny kernel
    # (~620 launches per MiDaS backward).  Instead: detach the views, let the engine hand over the
    # fresh gradient tensors, and add them all into the flat buffer with one multi-tensor call.
    def detach_grads(self):
        for p in self.params:
            p.grad = None

    def reattach_grads(self):
        """`.grad` of every parameter = its view of the flat buffer again (after a detach that was not absorbed)."""
        for p, o in zip(self.params, self.offsets):
            if p.grad is None or p.grad.data_ptr() != self.grad.data_ptr() + 4 * o:
                p.grad = self.grad[o:o + p.numel()].view_as(p)

    def absorb_grads(self):
        views, fresh = [], []
        record = self._live is None
        if record and self._seen is None:
            self._seen = [False] * len(self.params)
        for i, (p, o) in enumerate(zip(self.params, self.offsets)):
            g = p.grad
            v = self.grad[o:o + p.numel()].view_as(p)
            if g is not None:
                views.append(v)
                fresh.append(g if g.is_contiguous() else g.contiguous())
                if record:
                    self._seen[i] = True
            p.grad = v
        if views:
            torch._foreach_add_(views, fresh)

    def live_ranges(self):
        """[lo, hi) element ranges of the parameters that take part in the SGD step, fixed at the first call (the first step):
        the parameters absorb_grads saw a gradient for, or all of them.  A live segment's range includes its padding (zero in
        every buffer, and zero after an SGD step: d = 0 + wd * 0)."""
        if self._ranges is None:
            self._live = list(self._seen) if self._seen is not None else [True] * len(self.params)
            ranges = []
            for i, o in enumerate(self.offsets):
                if not self._live[i]:
                    continue
                hi = self.offsets[i + 1] if i + 1 < len(self.offsets) else self.numel
                if ranges and ranges[-1][1] == o:
                    ranges[-1][1] = hi
                else:
                    ranges.append([o, hi])
            self._ranges = [tuple(r) for r in ranges]
        return self._ranges

    def all_reduce_grads(self, async_op=False):
        if async_op:
            return parallel.all_reduce_sum_async_(self.grad)
        parallel.all_reduce_sum_(self.grad)
        return None

    def all_reduce_and_adam_step(self, n_buckets=4, skip_ptr=None):
        """Gradient exchange pipelined with the optimiser: the flat gradient goes out as `n_buckets` large
        all-reduces issued back to back; the Adam kernel of bucket i runs as soon as that bucket has arrived, while
        buckets i+1.. are still being reduced (RCCL runs them on its own stream; `work.wait()` only makes the compute
        stream wait, the host never blocks).  Single process: one Adam launch over the whole buffer."""
        if not parallel.is_distributed():
            return self.adam_step(skip_ptr=skip_ptr)
        pending = parallel.all_reduce_sum_buckets_async_(self.grad, n_buckets)
        self.step_count += 1
        skip_ptr = self._skip_pair(skip_ptr)
        for lo, hi, work in pending:
            if work is not None:
                work.wait()
            ops.adam_step(self.flat[lo:hi], self.grad[lo:hi], self.exp_avg[lo:hi], self.exp_avg_sq[lo:hi], self.step_count,
                          self.lr, self.betas[0], self.betas[1], self.eps, skip_ptr=skip_ptr)

    def adam_step(self, extra_grad=None, scale=1.0, scale_ptr=None, skip_ptr=None):
        """param -= Adam(scale * (*scale_ptr) * grad + extra_grad); nothing happens if *skip_ptr != 0."""
        self.step_count += 1
        ops.adam_step(self.flat, self.grad, self.exp_avg, self.exp_avg_sq, self.step_count, self.lr, self.betas[0],
                      self.betas[1], self.eps, scale=scale, scale_ptr=scale_ptr, grad2=extra_grad,
                      skip_ptr=self._skip_pair(skip_ptr))

    # -- the optimiser of either kind ---------------------------------------------------------
    def _sgd_launch(self, lo, hi, extra_grad, scale, scale_ptr, skip_ptr):
        """SGD over the live ranges that meet [lo, hi): one launch per contiguous live piece (the same pieces, the same step
        number and the same skip pair for every bucket; bucket bounds are 1024-element aligned, so every piece stays 16-byte
        aligned).  Dead segments keep their parameters and their (empty) momentum buffer."""
        for a, b in self.live_ranges():
            a, b = max(a, lo), min(b, hi)
            if a >= b:
                continue
            ops.sgd_step(self.flat[a:b], self.grad[a:b], None if self.momentum_buf is None else self.momentum_buf[a:b],
                         self.step_count, self.lr, self.momentum, self.dampening, self.weight_decay, scale=scale,
                         scale_ptr=scale_ptr, grad2=None if extra_grad is None else extra_grad[a:b], skip_ptr=skip_ptr)
        if self.momentum_buf is not None:
            self._state_params.update(i for i, live in enumerate(self._live) if live)

    def step(self, extra_grad=None, scale=1.0, scale_ptr=None, skip_ptr=None):
        """One optimiser step of this net's kind on grad' = scale * (*scale_ptr) * grad + extra_grad; nothing happens if
        *skip_ptr != 0."""
        if self.kind == 'adam':
            return self.adam_step(extra_grad, scale, scale_ptr, skip_ptr)
        self.step_count += 1
        self._sgd_launch(0, self.numel, extra_grad, scale, scale_ptr, self._skip_pair(skip_ptr))

    def all_reduce_and_step(self, n_buckets=4, skip_ptr=None):
        """all_reduce_and_adam_step for either kind: the same bucket loop, each bucket's step launched once it has arrived."""
        if self.kind == 'adam':
            return self.all_reduce_and_adam_step(n_buckets, skip_ptr)
        if not parallel.is_distributed():
            return self.step(skip_ptr=skip_ptr)
        pending = parallel.all_reduce_sum_buckets_async_(self.grad, n_buckets)
        self.step_count += 1
        skip_ptr = self._skip_pair(skip_ptr)
        for lo, hi, work in pending:
            if work is not None:
                work.wait()
            self._sgd_launch(lo, hi, None, 1.0, None, skip_ptr)

    # Checkpoints carry `optimizer.state_dict()` of a torch.optim.Adam (netinterface.py:528-536, written by
    # ModelSaveLogger with save_optimizer=True); emit and accept exactly that layout -- per-parameter
    # `step` / `exp_avg` / `exp_avg_sq` keyed by the parameter's index in `module.parameters()` order, one
    # param group -- so checkpoints written by either implementation resume in the other.  Under --optim sgd the layout is
    # torch.optim.SGD's: per-parameter `momentum_buffer` (momentum != 0, after the first effective step, parameters that had
    # a gradient only).
    def state_dict(self):
        if self.kind == 'sgd':
            return self._sgd_state_dict()
        state = {}
        eff = self.step_count - self._skipped()      # skipped steps did not advance the optimiser
        if eff > 0:
            for i, (p, o) in enumerate(zip(self.params, self.offsets)):
                n = p.numel()
                state[i] = {'step': torch.tensor(float(eff)),
                            'exp_avg': self.exp_avg[o:o + n].view_as(p).clone(),
                            'exp_avg_sq': self.exp_avg_sq[o:o + n].view_as(p).clone()}
        group = {'lr': self.lr, 'betas': self.betas, 'eps': self.eps, 'weight_decay': 0, 'amsgrad': False,
                 'maximize': False, 'foreach': None, 'capturable': False, 'differentiable': False, 'fused': None,
                 'decoupled_weight_decay': False, 'params': list(range(len(self.params)))}
        return {'state': state, 'param_groups': [group]}

    def load_state_dict(self, sd):
        """Accepts a torch.optim.Adam state_dict (any torch version: `step` int or tensor) and keeps this
        run's lr / betas / eps (optimizer_load_state_dict(keep_training_params=True), netinterface.py:565-574).
        Parameters without state (never stepped) keep zero moments."""
        if self.kind == 'sgd':
            return self._sgd_load_state_dict(sd)
        if 'state' not in sd:                      # round-1 flat layout
            self.step_count = int(sd['step']) + self._skipped()
            self.exp_avg.copy_(sd['exp_avg'])
            self.exp_avg_sq.copy_(sd['exp_avg_sq'])
            return
        groups = sd['param_groups']
        order = [i for g in groups for i in g['params']]
        if len(order) != len(self.params):
            raise ValueError('optimizer state has %d parameters, the network %d' % (len(order), len(self.params)))
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        steps = set()
        for slot, key in enumerate(order):
            st = sd['state'].get(key)
            if not st:
                continue
            p, o = self.params[slot], self.offsets[slot]
            n = p.numel()
            if st['exp_avg'].numel() != n:
                raise ValueError('optimizer state of parameter %d has %d elements, expected %d'
                                 % (slot, st['exp_avg'].numel(), n))
            self.exp_avg[o:o + n].copy_(st['exp_avg'].reshape(-1))
            self.exp_avg_sq[o:o + n].copy_(st['exp_avg_sq'].reshape(-1))
            steps.add(int(float(st['step'])))
        if len(steps) > 1:
            raise ValueError('per-parameter Adam step counts differ (%s): the fused optimiser keeps one count per '
                             'network' % sorted(steps))
        # (the kernel subtracts this process's skip count: add it, so that the effective step continues from the checkpoint's)
        self.step_count = (steps.pop() if steps else 0) + self._skipped()

    def _sgd_group(self):
        """The param group of torch.optim.SGD(lr, momentum, dampening, weight_decay) under the installed torch: its keys
        differ between torch versions, so they come from torch itself."""
        probe = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=self.lr, momentum=self.momentum,
                                dampening=self.dampening, weight_decay=self.weight_decay)
        group = dict(probe.state_dict()['param_groups'][0])
        group['params'] = list(range(len(self.params)))
        return group

    def _sgd_state_dict(self):
        state = {}
        if self.momentum_buf is not None and self.step_count - self._skipped() > 0:
            for i in sorted(self._state_params):
                state[i] = {'momentum_buffer': self.view(self.momentum_buf, i).clone()}
        return {'state': state, 'param_groups': [self._sgd_group()]}

    def _sgd_load_state_dict(self, sd):
        """Accepts a torch.optim.SGD state_dict and keeps this run's lr / momentum / dampening / weight decay
        (optimizer_load_state_dict(keep_training_params=True), netinterface.py:565-574).  A loaded momentum buffer counts as
        initialised: the next step is not a first step.  An Adam state is what torch.optim.SGD.load_state_dict accepts too:
        SGD then finds no momentum_buffer, and the buffers start empty (with a warning here)."""
        groups = sd['param_groups']
        order = [i for g in groups for i in g['params']]
        if len(order) != len(self.params):
            raise ValueError('optimizer state has %d parameters, the network %d' % (len(order), len(self.params)))
        if self.momentum_buf is not None:
            self.momentum_buf.zero_()
        self._state_params = set()
        foreign = False
        for slot, key in enumerate(order):
            st = sd['state'].get(key)
            if not st:
                continue
            buf = st.get('momentum_buffer')
            if buf is None:
                foreign = foreign or any(k in st for k in ('exp_avg', 'exp_avg_sq'))
                continue
            if self.momentum_buf is None:        # momentum 0 in this run: torch's SGD never reads the buffer
                continue
            if buf.numel() != self.params[slot].numel():
                raise ValueError('optimizer state of parameter %d has %d elements, expected %d'
                                 % (slot, buf.numel(), self.params[slot].numel()))
            self.view(self.momentum_buf, slot).copy_(buf.reshape(self.params[slot].shape))
            self._state_params.add(slot)
        if foreign:
            warnings.warn('FlatNet(sgd): the optimizer state holds no momentum_buffer (an Adam checkpoint?); the momentum '
                          'buffers start empty, as torch.optim.SGD would')
        # effective step 1 when buffers were loaded (the next step is not a first one), 0 otherwise; the kernel subtracts
        # this process's skip count, so add it
        self.step_count = (1 if self._state_params else 0) + self._skipped()
