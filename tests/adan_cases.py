"""Cases and restatement for the tests of the fused Adan (boundary B23, dreamwaltz_g_amd.optim.FlatAdan, csrc/adan_math.h).  Imports
nothing of the reference.

  GOLDEN_SHAPES, GOLDEN_LRS    the two param groups of tests/golden/adan.npz (capture_golden_adan.py) and their learning rates
  VARIANTS                     weight_decay x no_prox x max_grad_norm of the golden
  NORMS                        the global gradient norm of each of the K = 6 steps: above max_grad_norm = 5 on three, below it on two,
                               and one all-zero gradient
  make_params / make_grads     seeded fp32 parameters and the K steps of gradients, scaled to NORMS over all groups
  Chain / chain(...)           the optimizer restated in torch in `dtype`: float64 is the oracle; float32 is the composition of the fp32
                               tensor statements (what the reference's own step runs) whose error against float64 sets the bound
  rel_max                      max|err| / max|ref|
  bound(comp, ref)             the project's rule: 2 x (the fp32 composition's error) + 1e-7
"""
import numpy as np
import torch

f32 = np.float32
K = 6
MAX_GRAD_NORM = 5.0
NORMS = [12.0, 0.7, 0.0, 30.0, 2.5, 5.5]
GOLDEN_SHAPES = [[(5, 7), (5,)], [(3, 5), (3,)]]
GOLDEN_LRS = [1e-3, 3e-3]
BETAS = (0.98, 0.92, 0.99)
EPS = 1e-8
VARIANTS = [(wd, no_prox, mgn) for wd in (0.0, 2e-5) for no_prox in (False, True) for mgn in (0.0, MAX_GRAD_NORM)]
STATES = ("exp_avg", "exp_avg_sq", "exp_avg_diff", "neg_pre_grad")
BACKGROUND_SHAPES = [[(16, 27), (16,), (3, 16), (3,)]]        # the learned background's four tensors (499 parameters), one group


def variant_tag(wd, no_prox, mgn):
    return "wd%g_%s_clip%g" % (wd, "noprox" if no_prox else "prox", mgn)


def hypers(lrs, wd, no_prox):
    return [dict(lr=lr, betas=BETAS, eps=EPS, weight_decay=wd, no_prox=no_prox) for lr in lrs]


def make_params(shapes, seed=0):
    """-> [group][tensor] fp32 arrays, nn.Linear-like magnitudes."""
    r = np.random.RandomState(seed)
    return [[(r.rand(*s).astype(f32) * 2 - 1) * f32(0.3) for s in group] for group in shapes]


def make_grads(shapes, seed=1, norms=NORMS):
    """-> [step][group][tensor] fp32 arrays whose global norm over all groups is norms[step] (to fp32 rounding)."""
    r = np.random.RandomState(seed)
    out = []
    for target in norms:
        raw = [[r.randn(*s) for s in group] for group in shapes]
        total = np.sqrt(sum(float((t * t).sum()) for g in raw for t in g))
        out.append([[(t * (target / total)).astype(f32) for t in g] for g in raw])
    return out


def global_norm(step_grads):
    return float(np.sqrt(sum(float((t.astype(np.float64) ** 2).sum()) for g in step_grads for t in g)))


def flat(group):
    """The tensors of one group as one 1-D array (no padding)."""
    return np.concatenate([np.asarray(t).reshape(-1) for t in group])


class Chain:
    """The optimizer restated in torch in `dtype`, one step at a time.  params [G] 1-D fp32 arrays (or tensors), hyper [G] dicts.
    step(grads [G]) applies the statements in the order the optimizer's single-tensor step applies them: the clipping factor from the
    global norm of ALL groups with the LAST group's eps; per group the step count, then per element g, d, m, v, u, n, the denominator
    and the update; neg_pre_grad = -g.  -> {'p': [G], 'exp_avg': [G], ...} clones of the state after the step."""

    def __init__(self, params, hyper, max_grad_norm, dtype, grad_scale=1.0):
        self.hyper, self.max_grad_norm, self.dtype, self.grad_scale = hyper, max_grad_norm, dtype, grad_scale
        self.p = [torch.as_tensor(np.array(x, f32) if not torch.is_tensor(x) else x.detach().cpu().float()).to(dtype) for x in params]
        self.st = {k: [torch.zeros_like(x) for x in self.p] for k in STATES}
        self.t = 0

    def step(self, step_grads):
        dtype, hyper, p, st = self.dtype, self.hyper, self.p, self.st
        gs = [torch.as_tensor(x).detach().cpu().to(dtype) * self.grad_scale for x in step_grads]
        if self.max_grad_norm > 0:
            total = torch.zeros((), dtype=dtype)
            for g in gs:
                total = total + g.pow(2).sum()
            clip = float(torch.clamp(torch.tensor(self.max_grad_norm, dtype=dtype) / (torch.sqrt(total) + hyper[-1]['eps']), max=1.0))
        else:
            clip = 1.0
        self.t += 1
        t = self.t
        for i in range(len(p)):
            h = hyper[i]
            b1, b2, b3 = h['betas']
            lr, wd, eps = h['lr'], h['weight_decay'], h['eps']
            g = gs[i] * clip
            d = torch.zeros_like(g) if t == 1 else st['neg_pre_grad'][i] + g
            m = st['exp_avg'][i] * b1 + g * (1 - b1)
            v = st['exp_avg_diff'][i] * b2 + d * (1 - b2)
            u = d * b2 + g
            n = st['exp_avg_sq'][i] * b3 + (u * u) * (1 - b3)
            den = n.sqrt() / (1.0 - b3 ** t) ** 0.5 + eps
            step, step_diff = lr / (1.0 - b1 ** t), lr * b2 / (1.0 - b2 ** t)
            q = p[i]
            if h['no_prox']:
                q = q * (1 - lr * wd)
                q = q - step * (m / den)
                q = q - step_diff * (v / den)
            else:
                q = q - step * (m / den)
                q = q - step_diff * (v / den)
                q = q / (1 + lr * wd)
            p[i] = q
            st['exp_avg'][i], st['exp_avg_diff'][i], st['exp_avg_sq'][i], st['neg_pre_grad'][i] = m, v, n, -g
        rec = {'p': [x.clone() for x in p]}
        rec.update({key: [x.clone() for x in st[key]] for key in STATES})
        return rec


def chain(params, grads, hyper, max_grad_norm, dtype, grad_scale=1.0):
    """Chain over recorded gradients grads [K][G] -> the K records."""
    c = Chain(params, hyper, max_grad_norm, dtype, grad_scale)
    return [c.step(step_grads) for step_grads in grads]


def rel_max(a, ref):
    a, ref = torch.as_tensor(a).double(), torch.as_tensor(ref).double()
    return float((a - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def bound(comp, ref):
    return 2 * rel_max(comp, ref) + 1e-7
