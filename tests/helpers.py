"""Shared helpers for the parity tests (test infrastructure)."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CAM_KEYS = ('R_1', 'R_2', 'R_1_T', 'R_2_T', 't_1', 't_2', 'K', 'K_inv')


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False)
    return {k: z[k] for k in z.files}


def load_golden_json(name):
    import json
    with open(os.path.join(GOLDEN, name + '.json')) as f:
        return json.load(f)


def t(a, device='cpu'):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def golden_batch(gd, device='cpu'):
    b = {}
    for k, v in gd.items():
        if k.startswith('in_') and k not in ('in_depth_1', 'in_depth_2', 'in_sf_1_2'):
            name = k[3:]
            b[name] = t(v) if name == 'time_step' else t(v, device)
    return b


def golden_opt(gd):
    from oracle.losses import default_opt
    o = {str(k): float(v) for k, v in zip(gd['opt_keys'], gd['opt_vals'])}
    for k in ('midas', 'use_disp', 'use_disp_ratio', 'time_dependent', 'use_cnn', 'warm_reg', 'weight_steps',
              'use_motion_seg'):
        if k in o:
            o[k] = bool(o[k])
    for k in ('interp_steps', 'n_freq_xyz', 'n_freq_t'):
        o[k] = int(o[k])
    return default_opt(**o)


def golden_mlp_sd(gd, device='cpu', prefix='sd_'):
    return {k[len(prefix):]: t(v, device) for k, v in gd.items() if k.startswith(prefix)}


def log_measured(name, value, bound):
    """Append one measured-vs-bound record to $DVD_PARITY_LOG (json lines) when it is set: the evidence visit keeps the
    file under profiles/, so every tolerance in the tests sits next to the value it was derived from.  bound=None: a value
    that is recorded for later comparison and asserted nowhere."""
    import json
    import os
    if os.environ.get('DVD_PARITY_LOG'):
        with open(os.environ['DVD_PARITY_LOG'], 'a') as f:
            f.write(json.dumps({'test': name, 'measured': float(value), 'bound': None if bound is None else float(bound)}) + '\n')


def mlp_oracle_f64(sd, x, t=None, n_freq_xyz=16, n_freq_t=16, pre=None):
    """oracle.sceneflow_mlp.mlp_forward with the periodic embedding in fp32 (the reference rounds f * v in fp32, and so does the
    kernel) and the 1x1 convolutions in float64.  An fp32 oracle on the host carries summation-order noise of its own (MKL
    blocks by thread count) of up to ~0.6 of the forward tolerance on these sizes; against float64 the comparison measures the
    kernels alone.  t=None: the time-independent network.  x / t may be float64 (an Euler chain): they are embedded as fp32.
    pre: a list that receives the five hidden pre-activations."""
    import torch.nn.functional as F
    from oracle import sceneflow_mlp as M
    feat = M.periodic_embed(x.float(), n_freq_xyz)
    if t is not None:
        feat = torch.cat([M.periodic_embed(t.float(), n_freq_t), feat], 1)
    h = feat.double()
    n_layers = len([k for k in sd if k.endswith('conv.weight')])
    for i in range(n_layers):
        h = F.conv2d(h, sd['convs.%d.conv.weight' % i], sd['convs.%d.conv.bias' % i])
        if i < n_layers - 1:
            if pre is not None:
                pre.append(h)
            h = F.leaky_relu(h, M.LRELU_SLOPE)
    return h


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def seeded_fill_(module, seed):
    """Deterministic, architecture-independent weights: every state_dict entry is
    drawn from a generator seeded by (seed, crc32(key)), so the reference model (in
    tests/golden/make_golden.py) and the product model get identical values without
    shipping 100+ MB of weights."""
    import math
    import zlib
    sd = module.state_dict()
    with torch.no_grad():
        for k in sorted(sd):
            v = sd[k]
            if k.endswith('num_batches_tracked'):
                continue
            g = torch.Generator().manual_seed(seed * 1000003 + zlib.crc32(k.encode()) % 1000003)
            if k.endswith('running_var'):
                v.copy_(0.5 + torch.rand(v.shape, generator=g))
            elif k.endswith('running_mean'):
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
            elif v.dim() >= 2:
                v.copy_(torch.randn(v.shape, generator=g) * (1.0 / math.sqrt(v[0].numel())))
            elif k.endswith('weight'):
                v.copy_(1.0 + 0.1 * torch.randn(v.shape, generator=g))
            else:
                v.copy_(0.05 * torch.randn(v.shape, generator=g))
    return module


def loader_batch(batch):
    """Add the leading DataLoader dimension (batch_size=1) the Model strips again."""
    out = {}
    for k, v in batch.items():
        out[k] = v.unsqueeze(0) if torch.is_tensor(v) else v
    return out


FULL_STEP_OPT = dict(
    optim='adam', adam_beta1=0.5, adam_beta2=0.9, lr=1e-4, scene_lr_mul=10.0, dataset='davis_sequence', batch_size=1,
    global_rank=0, vis_every_train=1, vis_at_start=False, epoch_batches=2000, vis_batches_train=0, use_cnn=False,
    use_embedding=False, midas=False, use_disp=True, use_disp_ratio=False, time_dependent=True, flow_mul=1.0,
    disp_mul=1.0, acc_mul=1.0, sf_mag_div=100.0, interp_steps=5, warm_reg=False, weight_steps=False,
    use_motion_seg=False, n_freq_xyz=16, n_freq_t=16, warm_sf=5, n_down=3, mlp_stash_gb=48.0, depth_chunk=8)


def flow_pair(H, W, seed, noise):
    """A smooth forward flow, its approximate inverse, plus noise of about the consistency threshold's size (1 px)
    and a band whose targets leave the image: inputs of the occlusion-mask tests and of the mask fixture."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing='ij')
    f12 = torch.stack([6.0 * torch.sin(yy / 17.0) + 0.02 * xx, 4.0 * torch.cos(xx / 23.0) - 0.03 * yy], -1)
    f21 = -f12 + noise * torch.randn(H, W, 2, generator=g)
    f12 = f12 + 0.3 * noise * torch.randn(H, W, 2, generator=g)
    f12[:5] += 40.0                        # a band whose targets leave the image
    return f12.contiguous(), f21.contiguous()


FLOW_MASK_CASES = [(48, 64, 1, 0.6), (96, 168, 2, 0.9), (192, 384, 3, 0.5), (33, 51, 4, 1.5)]
