"""Runs in its own process (tests/test_mlp_background_host.py): the REAL reference scene module from /root/reference (inert stand-ins for
the packages that are not installed, tests/golden/_ref_stubs.py) under dropin/dwg_bind's hooks, with `--render.use_mlp_background True`.
DWG_BIND_MLP_BACKGROUND is whatever the parent set.  Prints one JSON object."""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "dropin"))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, REF)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from oracle import animate as oa  # noqa: E402
import _ref_stubs  # noqa: E402
import dwg_bind  # noqa: E402


def main():
    out = {"switch": os.environ.get("DWG_BIND_MLP_BACKGROUND")}
    _ref_stubs.install(oa)
    dwg_bind.install()
    import core.system.scene as scmod
    from core.system.scene import build_scene
    from configs import TrainConfig
    made = []
    RefMLP = scmod.MLPBackground

    class Recording(RefMLP):                    # the reference's own class, remembering the instances build_scene makes
        def __init__(self):
            super().__init__()
            made.append(self)
    scmod.MLPBackground = Recording
    cfg = TrainConfig()
    cfg.device = "cpu"
    cfg.render.use_mlp_background = True
    avatar = nn.Module()
    setattr(avatar, "__dwg_bound__", True)        # what dwg_bind.bind_avatar marks: the scene is ours
    try:
        scene = build_scene(cfg=cfg, avatar=[avatar])
        out["raised"] = False
    except NotImplementedError as e:
        out["raised"] = True
        out["message"] = str(e)
        scene = None
    if scene is not None:
        bg = scene.background
        out["scene_class"] = type(scene).__module__ + "." + type(scene).__name__
        out["background_class"] = type(bg).__module__ + "." + type(bg).__name__
        out["reference_built"] = len(made)
        ref = made[0]
        out["weights_adopted"] = all(torch.equal(a.detach(), b.detach()) for a, b in zip(bg.parameters(), ref.parameters()))
        out["keys"] = sorted(k for k in scene.state_dict() if k.startswith("background."))
        out["reference_keys"] = sorted("background." + k for k in ref.state_dict())
        opt = bg.get_optimizer(cfg)
        out["optimizer_class"] = type(opt).__module__ + "." + type(opt).__name__
        out["optimizer_again_is_same"] = bg.get_optimizer() is opt
        pg = opt.param_groups[0]
        out["hyper"] = [pg["lr"], pg["eps"], pg["weight_decay"], pg["max_grad_norm"], list(pg["betas"]), pg["no_prox"]]
        ro = ref.get_optimizer()
        rg = ro.param_groups[0]
        out["reference_hyper"] = [rg["lr"], rg["eps"], rg["weight_decay"], rg["max_grad_norm"], list(rg["betas"]), rg["no_prox"]]
        out["params_are_views"] = all(p.data_ptr() >= opt.buf.flat.data_ptr() and p.data_ptr() < opt.buf.flat.data_ptr() + 4 * opt.buf.total
                                      for p in bg.parameters())
    dwg_bind.uninstall()
    print("DWG_MLP_BIND_CHECK " + json.dumps(out))


if __name__ == "__main__":
    main()
