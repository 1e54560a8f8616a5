"""Golden fixture of the stage-II learned MLP background (boundary B23): the reference's OWN MLPBackground.forward
(core/system/background.py:55-84: get_rays, the second normalisation, FreqEncoder_torch, MLP, sigmoid) and its compositing statement
(core/system/scene.py:161-164) run on the CPU -> tests/golden/mlp_background.npz (recorded inputs and results only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/capture_golden_mlp_background.py       (build container only: needs /root/reference)

Recorded weights (tests/mlp_background_cases.weights) and, for every ((H, W), F) of mlp_background_cases.GOLDEN, its cameras:
  keys                            the module's state_dict keys, joined by newlines (a string array)
  output_dim, freq_bands          the encoder's width and bands
  w<i>                            the four tensors as loaded
  <tag>_c2w, <tag>_K              the inputs; tag = HxWxF
  <tag>_image                     forward(data) of each camera, [F, H, W, 3]
  <tag>_g<i>                      autograd's gradient of tensor i for the cotangent mlp_background_cases.cotangent on the image
  <tag>_composite, _d_alpha, _d_bg   image_fg + image_bg * (1 - alpha) for mlp_background_cases.foreground and its gradients under the
                                  same cotangent"""
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
from tests import mlp_background_cases as mc  # noqa: E402


def main():
    _ref_stubs.install(oa)
    from core.system.background import MLPBackground
    bg = MLPBackground()
    out = {"keys": np.asarray("\n".join(bg.state_dict().keys())), "output_dim": np.asarray(bg.encoder_bg.output_dim, np.int32),
           "freq_bands": np.asarray([float(b) for b in bg.encoder_bg.freq_bands], np.float64)}
    wb = mc.weights()
    params = [p for lin in bg.bg_net.net for p in (lin.weight, lin.bias)]
    assert [tuple(p.shape) for p in params] == mc.SHAPES
    with torch.no_grad():
        for p, w in zip(params, wb):
            p.copy_(torch.from_numpy(w))
    for i, w in enumerate(wb):
        out["w%d" % i] = w
    for (H, W), F in mc.GOLDEN:
        tag = "%dx%dx%d" % (H, W, F)
        c2w, K = mc.cameras(F, H, W)
        out[tag + "_c2w"], out[tag + "_K"] = c2w, K
        for p in params:
            p.grad = None
        # one camera per call, as the reference's loaders hand them (its get_rays does not broadcast the intrinsics of a batch)
        img = torch.cat([bg({'c2w': torch.from_numpy(c2w[f:f + 1]), 'intrinsics': torch.from_numpy(K[f:f + 1]), 'image_height': H,
                             'image_width': W}) for f in range(F)])
        cot = torch.from_numpy(mc.cotangent(F, H, W))
        img.backward(cot)
        out[tag + "_image"] = img.detach().numpy().copy()
        for i, p in enumerate(params):
            out[tag + "_g%d" % i] = p.grad.numpy().copy()
        fg, alpha = mc.foreground(F, H, W)
        a = torch.from_numpy(alpha).requires_grad_(True)
        b = img.detach().clone().requires_grad_(True)
        comp = torch.from_numpy(fg) + b * (1 - a)
        comp.backward(cot)
        out[tag + "_composite"], out[tag + "_d_alpha"], out[tag + "_d_bg"] = comp.detach().numpy().copy(), a.grad.numpy().copy(), b.grad.numpy().copy()
    path = os.path.join(HERE, "mlp_background.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", sorted(out))


if __name__ == "__main__":
    main()
