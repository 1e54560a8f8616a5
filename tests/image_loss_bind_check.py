"""Runs in its own process (tests/test_image_loss_host.py): the REAL reference trainer module from /root/reference (inert stand-ins for the
packages that are not installed, tests/golden/_ref_stubs.py) under dropin/dwg_bind's hooks (boundary B17).  The stand-ins make
`pytorch3d` importable, so its absence -- what a real installation of this stack has -- is restored for `pytorch3d.ops`, the one import
of core/gaussian/gaussian_loss.py, by a finder that raises the ModuleNotFoundError Python itself would.  Prints one JSON object; a
reference module that cannot be imported for another missing package is reported as {"missing": <package>}."""
import importlib.abc
import inspect
import json
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "dropin"))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, REF)

from oracle import animate as oa  # noqa: E402
import _ref_stubs  # noqa: E402
import dwg_bind  # noqa: E402


class _NoPytorch3dOps(importlib.abc.MetaPathFinder):
    def find_spec(self, fullname, path, target=None):
        if fullname == "pytorch3d.ops" or fullname.startswith("pytorch3d.ops."):
            raise ModuleNotFoundError("No module named %r" % fullname, name=fullname)
        return None


def _hide_pytorch3d_ops():
    for name in [n for n in sys.modules if n == "pytorch3d.ops" or n.startswith("pytorch3d.ops.") or n == "core.gaussian.gaussian_loss"]:
        del sys.modules[name]
    p3d = sys.modules.get("pytorch3d")
    if p3d is not None and "ops" in vars(p3d):
        delattr(p3d, "ops")
    sys.meta_path.insert(0, _NoPytorch3dOps())


def _stand_in_self(nerf2gs):
    """What Trainer.init_losses reads of `self`: cfg.log.nerf2gs and cfg.nerf (SparsityLoss)."""
    from configs import TrainConfig
    cfg = TrainConfig()
    cfg.log.nerf2gs = nerf2gs
    return types.SimpleNamespace(cfg=cfg)


def main():
    out = {}
    _ref_stubs.install(oa)
    dwg_bind.install()
    try:
        import core.trainer as tr
    except ModuleNotFoundError as e:
        print("DWG_IMAGE_LOSS_BIND_CHECK " + json.dumps({"missing": e.name}))
        return
    cls = tr.Trainer
    for attr in ("init_losses", "pretrain_nerf2gs_forward"):
        f = getattr(cls, attr)
        orig = getattr(f, "__wrapped__", None)
        out[attr] = {"patched": bool(getattr(f, "__dwg_bound__", False)), "sig": str(inspect.signature(f)),
                     "orig_sig": str(inspect.signature(orig)) if orig is not None else None,
                     "orig_is_reference": orig is not None and orig.__module__ == "core.trainer" and not getattr(orig, "__dwg_bound__", False)}
    out["pretrain_patched"] = bool(getattr(cls.pretrain_forward, "__dwg_bound__", False))
    if out["init_losses"]["patched"]:
        import dwg_import  # noqa: F401
        from dreamwaltz_g_amd.image_loss import ImageReconstructionLoss
        # with an importable (inert) pytorch3d the original succeeds; the native object still takes its place
        me = _stand_in_self(True)
        losses = cls.init_losses(me)
        out["with_pytorch3d"] = {"native": isinstance(losses.get("image"), ImageReconstructionLoss), "keys": sorted(losses),
                                 "flag_after": me.cfg.log.nerf2gs}
        _hide_pytorch3d_ops()
        try:
            cls.init_losses.__wrapped__(_stand_in_self(True))
            out["original_raises"] = None
        except ModuleNotFoundError as e:
            out["original_raises"] = e.name
        me = _stand_in_self(True)
        losses = cls.init_losses(me)
        out["without_pytorch3d"] = {"native": isinstance(losses.get("image"), ImageReconstructionLoss), "keys": sorted(losses),
                                    "flag_after": me.cfg.log.nerf2gs, "lambda_dssim": losses["image"].lambda_dssim}
        me = _stand_in_self(False)
        out["flag_off_keys"] = sorted(cls.init_losses(me))
        # any other exception propagates, and the flag is restored on the way
        me = _stand_in_self(True)
        me.cfg.nerf = None                                      # SparsityLoss(cfg=None) fails in the original
        try:
            cls.init_losses(me)
            out["other_exception"] = None
        except ModuleNotFoundError:
            out["other_exception"] = "ModuleNotFoundError"
        except Exception as e:
            out["other_exception"] = type(e).__name__
        out["flag_after_other_exception"] = me.cfg.log.nerf2gs
    origs = {a: getattr(getattr(cls, a), "__wrapped__", None) for a in ("init_losses", "pretrain_nerf2gs_forward")}
    dwg_bind.uninstall()
    out["restored"] = {a: (getattr(cls, a) is origs[a]) if origs[a] is not None else not getattr(getattr(cls, a), "__dwg_bound__", False)
                       for a in origs}
    print("DWG_IMAGE_LOSS_BIND_CHECK " + json.dumps(out))


if __name__ == "__main__":
    main()
