"""Runs in its own process (tests/test_gs_background_host.py): the REAL reference scene module from /root/reference (inert stand-ins for
the packages that are not installed, tests/golden/_ref_stubs.py) under dropin/dwg_bind's hooks, with `--render.use_gs_background PATH`
(argv[1]: a .ply the test wrote).  Without DWG_BIND_GS_BACKGROUND=1 the bound build_scene raises; with it the scene is ours, its
background a GaussianBackground read by the package's own reader (the reference's GaussianModel is never built: its load_ply needs
plyfile), and the reference's precedence holds: MLP, then video, then the Gaussian scene.  Prints one JSON object."""
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

import numpy as np  # noqa: E402
import torch.nn as nn  # noqa: E402

from oracle import animate as oa  # noqa: E402
import _ref_stubs  # noqa: E402
import dwg_bind  # noqa: E402


def main():
    ply = sys.argv[1]
    out = {}
    _ref_stubs.install(oa)
    dwg_bind.install()
    import core.system.scene as scmod
    from core.system.scene import build_scene
    from configs import TrainConfig
    built = []

    class RecordingGaussianModel(scmod.GaussianModel):
        def __init__(self, *a, **k):
            built.append(True)
            super().__init__(*a, **k)
    scmod.GaussianModel = RecordingGaussianModel
    frames = [np.random.RandomState(i).randint(0, 256, size=(6, 8, 3)).astype(np.uint8) for i in range(2)]

    class StandInVideoBackground:               # core/system/background.py:92-160's surface, without cv2
        def __init__(self, path, preload=True):
            self.fps, self.frame_count, self.frame_width, self.frame_height = 25, len(frames), 8, 6
            self.frame_cache = list(frames)
    scmod.VideoBackground = StandInVideoBackground
    avatar = nn.Module()
    setattr(avatar, "__dwg_bound__", True)        # what dwg_bind.bind_avatar marks: the scene is ours

    def cfg(**flags):
        c = TrainConfig()
        c.device = "cpu"
        c.render.use_gs_background = ply
        for k, v in flags.items():
            setattr(c.render, k, v)
        return c

    def raises():
        try:
            build_scene(cfg=cfg(), avatar=[avatar])
            return False
        except NotImplementedError:
            return True
    os.environ.pop("DWG_BIND_GS_BACKGROUND", None)
    out["without_env_raises"] = raises()
    os.environ["DWG_BIND_GS_BACKGROUND"] = "0"
    out["env_other_value_raises"] = raises()
    os.environ["DWG_BIND_GS_BACKGROUND"] = "1"
    scene = build_scene(cfg=cfg(), avatar=[avatar])
    bg = scene.background
    name = lambda o: type(o).__module__ + "." + type(o).__name__          # noqa: E731
    out["scene_class"], out["background_class"] = name(scene), name(bg)
    out["arrays"] = {k: getattr(bg, "_" + k).detach().numpy().reshape(-1).tolist()
                     for k in ("positions", "sh_features_dc", "sh_features_rest", "opacities", "scales", "quaternions")}
    out["frozen"] = all(not p.requires_grad for p in bg.parameters())
    out["reference_gaussian_model_built"] = len(built)
    out["video_wins"] = name(build_scene(cfg=cfg(use_video_background="clip.mp4"), avatar=[avatar]).background)
    os.environ["DWG_BIND_MLP_BACKGROUND"] = "1"
    out["mlp_wins"] = name(build_scene(cfg=cfg(use_mlp_background=True, use_video_background="clip.mp4"), avatar=[avatar]).background)
    dwg_bind.uninstall()
    print("DWG_GS_BIND_CHECK " + json.dumps(out))


if __name__ == "__main__":
    main()
