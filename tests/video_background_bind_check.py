"""Runs in its own process (tests/test_video_background_host.py): the REAL reference scene module from /root/reference (inert stand-ins for
the packages that are not installed, tests/golden/_ref_stubs.py) under dropin/dwg_bind's hooks, with `--render.use_video_background` set.
cv2 is inert here, so the reference's VideoBackground is replaced by a stand-in that carries its surface (frame_cache, fps, frame_count,
__del__).  Prints one JSON object."""
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
    out = {}
    _ref_stubs.install(oa)
    dwg_bind.install()
    import core.system.scene as scmod
    from core.system.scene import build_scene
    from configs import TrainConfig
    frames = [np.random.RandomState(i).randint(0, 256, size=(12, 20, 3)).astype(np.uint8) for i in range(5)]
    made, deleted = [], []

    class StandInVideoBackground:               # core/system/background.py:92-160's surface, without cv2
        def __init__(self, path, preload=True):
            made.append(path)
            self.fps, self.frame_count, self.frame_width, self.frame_height = 25, len(frames), 20, 12
            self.frame_cache = list(frames) if preload else None

        def get_background(self, i):
            return frames[i]

        def __del__(self):
            deleted.append(True)
    scmod.VideoBackground = StandInVideoBackground

    cfg = TrainConfig()
    cfg.device = "cpu"
    cfg.render.use_video_background = "motionx_reenact,clip"
    avatar = nn.Module()
    setattr(avatar, "__dwg_bound__", True)        # what dwg_bind.bind_avatar marks: the scene is ours
    scene = build_scene(cfg=cfg, avatar=[avatar])
    bg = scene.background
    out["scene_class"] = type(scene).__module__ + "." + type(scene).__name__
    out["background_class"] = type(bg).__module__ + "." + type(bg).__name__
    out["reference_constructed_with"] = made
    out["reference_kept"] = bg.reference is not None and type(bg.reference).__name__ == "StandInVideoBackground"
    out["attributes"] = [bg.fps, bg.frame_count, bg.frame_width, bg.frame_height]
    out["frames_equal"] = bool(np.array_equal(bg._host.numpy(), np.stack(frames)))
    del bg
    out["alive_while_scene_lives"] = not deleted
    del scene
    import gc
    gc.collect()
    out["released_with_scene"] = bool(deleted)
    raised = {}
    for flag, value in (("use_mlp_background", True), ("use_gs_background", "bg.ply")):
        c = TrainConfig()
        c.device = "cpu"
        setattr(c.render, flag, value)
        try:
            build_scene(cfg=c, avatar=[avatar])
            raised[flag] = False
        except NotImplementedError:
            raised[flag] = True
    out["other_backgrounds_raise"] = raised
    dwg_bind.uninstall()
    print("DWG_VIDEO_BIND_CHECK " + json.dumps(out))


if __name__ == "__main__":
    main()
