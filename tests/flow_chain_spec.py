"""Executable specification of the flow-chaining kernel (csrc/flow_chain.hip, include/dvd_hip.h: dvd_flow_chain), of
preprocess.chain_plan and of preprocess.chain_flows (test infrastructure; the product keeps no CPU path).

`chain` with dtype=np.float32 is the CONTRACT, operation for operation: numpy rounds every elementwise multiply, add and
subtract of float32 arrays once, IEEE, which is what the kernel does (built with -ffp-contract=off).  Per link at x_k = (px, py):

  * the link breaks unless 0 <= px <= W-1 and 0 <= py <= H-1 (a NaN fails), or where its pair is outside 0 .. P-1
  * ix = floor(px), wx = px - ix, ux = 1 - wx (the same in y); w00 = ux * uy, w10 = wx * uy, w01 = ux * wy, w11 = wx * wy
  * a tap whose weight is exactly 0 is neither read nor tested; the link breaks where the mask of a tap that is read is not 0
  * f = ((t00 * w00 + t10 * w10) + t01 * w01) + t11 * w11 per component, an unread tap as +0
  * x_{k+1} = x_k + f; the link breaks where a component of it is a NaN or beyond fp32's largest finite number
  * row k of the flow is x_{k+1} - x0 -- a subtraction of its own, not a running sum of the f

dtype=np.float64 is the reference (the same statements on the same fp32 inputs).  `decided` flags a pixel whose float64 walk
never comes within 1e-4 px of an integer grid line at a position it samples from (x_1 .. x_{n-1}; x_0 is an integer in every
number format) -- there floorf could fall the other way in fp32, and the image border is such a line.

Reused by import: triangulate_spec.scene, consistency_masks and plan.
"""
import numpy as np

import triangulate_spec as T

MAX_LINKS = 32
FLT_MAX = float(np.finfo(np.float32).max)
DECIDED_MARGIN = 1e-4
# worst / mean distance in pixels of the float64 chain of gap-1 flows from the scene's own direct flow of gap g, over the pixels
# of scene(24, 40, 7, noise=0.0) that are static at every tap of their walk, unbroken and whose direct mask is 0: the
# interpolation error of the method, printed by tests/test_flow_chain_cpu.py::test_float64_chain_of_gap_1_flows_against_the_direct_flow
MEASURED_CHAIN = {2: (2.090e-4, 1.219e-4), 3: (4.315e-4, 2.541e-4), 4: (5.567e-4, 3.233e-4)}
# ... and the worst distance with the pixels that are static in their own frame but pass the rim of the disc on their walk
# (75, 56 and 39 pixels of 3157, 2237 and 1486): there a tap takes the disc's flow, and the point follows the disc for a link
# (the test holds these to 5 % of what it computes; the composed pair's masks take these pixels out, which it asserts as well)
MEASURED_CHAIN_RIM = {2: 0.9538, 3: 3.590, 4: 0.8796}
# worst distance in pixels of the kernel's flow from the float64 reference on the decided, unbroken pixels of the gap-1 chains to
# gaps 2, 3, 4 of scene(24, 40, 7, noise=0.4), measured on the MI355X (tests/test_63_flow_chain_kernel_gpu.py); the bound is 4 x
MEASURED = {'flow': 1.102e-5}


def chain(f12, f21, m1, m2, links, dtype=np.float32):
    """ops.flow_chain restated -> dict: flow dtype [L,B,H,W,2], broken uint8 [L,B,H,W], decided bool [B,H,W] (meaningful for
    dtype=np.float64) and end dtype [B,H,W,2], the position after the last link that held."""
    f12, f21, m1, m2 = (np.asarray(a) for a in (f12, f21, m1, m2))
    links = np.asarray(links)
    P, H, W, _ = f12.shape
    B, L, _ = links.shape
    flow, broken = np.zeros((L, B, H, W, 2), dtype), np.full((L, B, H, W), 255, np.uint8)
    decided, end = np.ones((B, H, W), bool), np.zeros((B, H, W, 2), dtype)
    vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    x0 = np.stack([uu, vv], -1).astype(dtype)
    one, fmax = dtype(1), dtype(FLT_MAX)
    for b in range(B):
        x, cur = x0.copy(), np.zeros((H, W, 2), dtype)
        brk, alive = np.zeros((H, W), np.uint8), np.ones((H, W), bool)
        for k in range(L):
            pair, d = int(links[b, k, 0]), int(links[b, k, 1])
            if pair == -1:
                break
            if not 0 <= pair < P:
                ok = np.zeros((H, W), bool)
            else:
                fl, mk = (f21 if d else f12)[pair].astype(dtype), (m1 if d else m2)[pair]
                with np.errstate(all='ignore'):
                    px, py = x[..., 0], x[..., 1]
                    if k > 0:                   # (on either side of the border too: it decides whether the link breaks)
                        for q in (px.astype(np.float64), py.astype(np.float64)):
                            decided[b] &= ~alive | (np.abs(q - np.round(q)) >= DECIDED_MARGIN)
                    go = alive & (px >= 0) & (px <= dtype(W - 1)) & (py >= 0) & (py <= dtype(H - 1))
                    px, py = np.where(go, px, dtype(0)), np.where(go, py, dtype(0))
                    fx, fy = np.floor(px), np.floor(py)
                    wx, wy = px - fx, py - fy
                    ux, uy = one - wx, one - wy
                    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
                    ix1, iy1 = np.minimum(ix + 1, W - 1), np.minimum(iy + 1, H - 1)
                    masked, f = np.zeros((H, W), bool), None
                    for w, yy, xx in ((ux * uy, iy, ix), (wx * uy, iy, ix1), (ux * wy, iy1, ix), (wx * wy, iy1, ix1)):
                        read = w != 0
                        masked |= read & (mk[yy, xx] != 0)
                        term = np.where(read[..., None], fl[yy, xx], dtype(0)) * w[..., None]
                        f = term if f is None else f + term
                    nx = x + f
                    ok = go & ~masked & (np.abs(nx[..., 0]) <= fmax) & (np.abs(nx[..., 1]) <= fmax)
                x = np.where(ok[..., None], nx, x)
                cur = np.where(ok[..., None], x - x0, cur)
            brk[alive & ~ok] = k + 1
            alive = alive & ok
            flow[k, b], broken[k, b] = cur, brk
        end[b] = x
    return {'flow': flow, 'broken': broken, 'decided': decided, 'end': end}


def chain_plan(pairs, n_frames, gaps, base=None):
    """preprocess.chain_plan restated -> (new_pairs, links_fwd, links_bwd)."""
    at = {}
    for j, p in enumerate(pairs):
        at.setdefault(tuple(p), j)
    usable = sorted(set(b - a for a, b in at if base is None or b - a in base), reverse=True)
    new_pairs, chains = [], []
    for g in sorted(set(gaps)):
        for a in range(n_frames - g):
            if (a, a + g) in at:
                continue
            f, c = a, []
            while f < a + g:
                s = [s for s in usable if s <= a + g - f and (f, f + s) in at]
                if not s:
                    raise ValueError('(%d, %d) cannot be reached' % (a, a + g))
                c.append(at[(f, f + s[0])])
                f += s[0]
            if len(c) > MAX_LINKS:
                raise ValueError('(%d, %d) needs more than %d links' % (a, a + g, MAX_LINKS))
            new_pairs.append((a, a + g))
            chains.append(c)
    L = max([len(c) for c in chains] + [1])
    fwd, bwd = np.full((len(chains), L, 2), -1, np.int32), np.full((len(chains), L, 2), -1, np.int32)
    for i, c in enumerate(chains):
        fwd[i, :len(c)] = [(j, 0) for j in c]
        bwd[i, :len(c)] = [(j, 1) for j in reversed(c)]
    return new_pairs, fwd, bwd


def last_rows(res, links):
    """The row of every chain's last link: (flow [B,H,W,2], broken [B,H,W])."""
    n = (np.asarray(links)[..., 0] >= 0).sum(1)
    b = np.arange(len(n))
    return res['flow'][n - 1, b], res['broken'][n - 1, b]


def chain_flows(f12, f21, m1, m2, pairs, n_frames, gaps, base=None, dtype=np.float32):
    """preprocess.chain_flows restated on host arrays -> dict of pairs, flow_1_2, flow_2_1, broken_1, broken_2, mask_1, mask_2,
    n_links.  The consistency rule is triangulate_spec.consistency_masks on the composed pair (as fp32 flows, which is what the
    store keeps); mask_2 and broken_2 belong to flow_1_2, the forward chain; mask_1 and broken_1 to flow_2_1."""
    new_pairs, fwd, bwd = chain_plan(pairs, n_frames, gaps, base)
    out = {'pairs': new_pairs, 'n_links': (fwd[..., 0] >= 0).sum(1).astype(np.int32)}
    for links, fk, bk in ((fwd, 'flow_1_2', 'broken_2'), (bwd, 'flow_2_1', 'broken_1')):
        fl, br = last_rows(chain(f12, f21, m1, m2, links, dtype), links)
        out[fk], out[bk] = fl.astype(np.float32), br
    mm = [T.consistency_masks(out['flow_1_2'][j], out['flow_2_1'][j]) for j in range(len(new_pairs))]
    out['mask_1'] = np.stack([m[0] for m in mm], 0) | (out['broken_1'] != 0).astype(np.uint8)
    out['mask_2'] = np.stack([m[1] for m in mm], 0) | (out['broken_2'] != 0).astype(np.uint8)
    return out


def gap1_links(N, g):
    """The chains of gap-1 flows to gap g in a video whose pairs begin with (a, a + 1), a = 0 .. N-2: (pairs, fwd, bwd)."""
    return chain_plan([(a, a + 1) for a in range(N - 1)], N, [g])


def distance(a, b, where):
    """(worst, mean) Euclidean distance in pixels of two flow fields [...,2] over `where`, in float64."""
    d = np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64), axis=-1)[where]
    return (float(d.max()), float(d.mean())) if d.size else (0.0, 0.0)
