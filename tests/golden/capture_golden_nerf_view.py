"""Golden fixture of the view around the NeRF render (boundary B20): the reference's OWN get_rays (core/nerf/nerf_utils.py:72-137) and
SparsityLoss (core/nerf/nerf_loss.py:17-56) run on the CPU -> tests/golden/nerf_view.npz (recorded inputs and outputs only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/capture_golden_nerf_view.py       (build container only: needs /root/reference)

Inert stand-ins satisfy the imports (tests/golden/_ref_stubs.py: igl among them); the statements that run are the reference's.
  rays    for (H, W) of tests/nerf_view_cases.SIZES with nerf_view_cases.camera: c2w_HxW, K_HxW (the inputs), rays_o_HxW, rays_d_HxW
  loss    for every case of nerf_view_cases.LAMBDAS, before and after the schedule step: ws (the input), loss_<case>_<when> (fp32 scalar)
          and grad_<case>_<when> [2145] (torch autograd of that loss)"""
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, HERE); sys.path.insert(0, "/root/reference")
from oracle import animate as oa  # noqa: E402
import _ref_stubs  # noqa: E402
from tests import nerf_view_cases as vc  # noqa: E402


def main():
    _ref_stubs.install(oa)
    from core.nerf.nerf_utils import get_rays
    from core.nerf.nerf_loss import SparsityLoss
    out = {}
    for H, W in vc.SIZES:
        c2w, K = vc.camera(H, W)
        r = get_rays(torch.from_numpy(c2w)[None], torch.from_numpy(K)[None], H, W)
        tag = "%dx%d" % (H, W)
        out["c2w_" + tag], out["K_" + tag] = c2w, K
        out["rays_o_" + tag] = r['rays_o'][0].contiguous().numpy()
        out["rays_d_" + tag] = r['rays_d'][0].contiguous().numpy()
    ws = vc.ws_vector()
    out["ws"] = ws
    for case, (lo, le, lm) in vc.LAMBDAS.items():
        cfg = types.SimpleNamespace(lambda_opacity=lo, lambda_entropy=le, lambda_emptiness=lm, sparsity_multiplier=vc.MULTIPLIER,
                                    sparsity_step=vc.SPARSITY_STEP)
        fn = SparsityLoss(cfg)
        for when, step in vc.STEPS.items():
            t = torch.from_numpy(ws).clone().requires_grad_(True)
            loss = fn(t, current_step=step, max_iteration=vc.MAX_ITER)
            loss.backward()
            out["loss_%s_%s" % (case, when)] = loss.detach().numpy().astype(np.float32)
            out["grad_%s_%s" % (case, when)] = t.grad.numpy().copy()
    path = os.path.join(HERE, "nerf_view.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", sorted(out))


if __name__ == "__main__":
    main()
