"""Golden fixture of the Adan optimizer (boundary B23): the reference's OWN Adan (core/optim/adan.py, foreach=False) run on the CPU
-> tests/golden/adan.npz (recorded inputs and results only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/capture_golden_adan.py       (build container only: needs /root/reference)

Two param groups with different learning rates (tests/adan_cases.GOLDEN_SHAPES / GOLDEN_LRS), K = 6 steps of recorded gradients whose
global norm is above max_grad_norm = 5 on three steps, below it on two and exactly zero on one (asserted here), for every variant of
adan_cases.VARIANTS (weight_decay 0 / 2e-5, no_prox, max_grad_norm 0 / 5).
Every tensor is stored flat, the tensors of all groups one after the other (adan_cases.flat per group, groups concatenated):
  p0 [58], grads [K, 58]                    the inputs
  <variant>_p, <variant>_<state> [K, 58]    parameters and exp_avg, exp_avg_sq, exp_avg_diff, neg_pre_grad after every step
  <variant>_step [K, 2]                     the groups' step counts after every step"""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, HERE); sys.path.insert(0, "/root/reference")
from oracle import animate as oa  # noqa: E402
import _ref_stubs  # noqa: E402
from tests import adan_cases as ac  # noqa: E402


def main():
    _ref_stubs.install(oa)
    from core.optim.adan import Adan
    out = {}
    p0 = ac.make_params(ac.GOLDEN_SHAPES)
    grads = ac.make_grads(ac.GOLDEN_SHAPES)
    norms = [ac.global_norm(g) for g in grads]
    assert len(grads) == ac.K
    assert sum(n > ac.MAX_GRAD_NORM for n in norms) >= 2 and sum(0 < n < ac.MAX_GRAD_NORM for n in norms) >= 2, norms
    assert sum(all(not t.any() for g in step for t in g) for step in grads) == 1, norms
    out["p0"] = np.concatenate([ac.flat(group) for group in p0])
    out["grads"] = np.stack([np.concatenate([ac.flat(group) for group in step]) for step in grads])
    for wd, no_prox, mgn in ac.VARIANTS:
        tag = ac.variant_tag(wd, no_prox, mgn)
        params = [[torch.nn.Parameter(torch.from_numpy(t.copy())) for t in group] for group in p0]
        opt = Adan([{'params': group, 'lr': lr} for group, lr in zip(params, ac.GOLDEN_LRS)], betas=ac.BETAS, eps=ac.EPS, weight_decay=wd,
                   max_grad_norm=mgn, no_prox=no_prox, foreach=False)
        rec = {}
        for k, step in enumerate(grads):
            for group, gg in zip(params, step):
                for p, t in zip(group, gg):
                    p.grad = torch.from_numpy(t.copy())
            opt.step()
            rec.setdefault("step", []).append(np.asarray([pg['step'] for pg in opt.param_groups], np.int32))
            rec.setdefault("p", []).append(np.concatenate([p.detach().numpy().reshape(-1) for group in params for p in group]))
            for key in ac.STATES:
                rec.setdefault(key, []).append(np.concatenate([opt.state[p][key].numpy().reshape(-1) for group in params for p in group]))
        for key, rows in rec.items():
            out["%s_%s" % (tag, key)] = np.stack(rows)
    path = os.path.join(HERE, "adan.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays; norms", norms)


if __name__ == "__main__":
    main()
