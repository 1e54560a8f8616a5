"""Stage-II learned MLP background (boundary B23, dreamwaltz_g_amd.background.MLPBackground), host side: the float64 restatement of
tests/mlp_background_cases.py against tests/golden/mlp_background.npz -- the reference's own MLPBackground.forward on the CPU, which pins
the encoding's column order and the second normalisation --, Scene's acceptance, the checkpoint keys, the trainer's refusals, the redo
loop, the C-ABI's argument checks and the opt-in binding.

Bounds of the pin (the golden is an fp32 run, the restatement float64): image and composite within 2e-6 of max|ref| -- sums of 27 and 16
fp32 products, a dozen roundings of 6e-8 --, gradients within nerf_background_cases.F32_BWD relative L2.  A swapped column or a missing
normalisation is an error of order 0.1."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import dwg_import  # noqa: F401
from tests import mlp_background_cases as mc
from tests import nerf_background_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mlp_background.npz")
FWD = 2e-6


def _cfg():
    from dreamwaltz_g_amd import configs
    cfg = configs.TrainConfig()
    cfg.device = "cpu"
    return cfg


@pytest.mark.parametrize("size,F", mc.GOLDEN, ids=["%dx%dx%d" % (s[0], s[1], f) for s, f in mc.GOLDEN])
def test_float64_restatement_against_the_references_forward(size, F):
    H, W = size
    d = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 100 << 10
    tag = "%dx%dx%d" % (H, W, F)
    wb = [d["w%d" % i] for i in range(4)]
    assert all(np.array_equal(a, b) for a, b in zip(wb, mc.weights()))
    c2w, K = mc.cameras(F, H, W)
    assert np.array_equal(d[tag + "_c2w"], c2w) and np.array_equal(d[tag + "_K"], K)
    assert K[0, 0, 2] != W / 2 and K[0, 1, 2] != H / 2                                  # off-centre principal point
    fg, alpha = mc.foreground(F, H, W)
    assert (alpha == 0).any() and (alpha == 1).any() and ((alpha > 0) & (alpha < 1)).any()
    o = mc.oracle(c2w, K, H, W, wb, mc.cotangent(F, H, W), fg, alpha)
    assert bc.rel_max(torch.from_numpy(d[tag + "_image"]), o["image"]) <= FWD
    assert bc.rel_max(torch.from_numpy(d[tag + "_composite"]), o["composite"]) <= FWD
    for i in range(4):
        assert bc.rel_l2(torch.from_numpy(d[tag + "_g%d" % i]), o["grads"][i]) <= bc.F32_BWD, i
    assert bc.rel_l2(torch.from_numpy(d[tag + "_d_alpha"]), o["d_alpha"]) <= bc.F32_BWD
    assert bc.rel_l2(torch.from_numpy(d[tag + "_d_bg"]), o["d_bg"]) <= bc.F32_BWD
    # the directions are unit vectors, and the layout is [x, sin x, cos x, sin 2x, cos 2x, ...]: bands 1, 2, 4, 8, 27 columns
    assert float((o["dirs"].norm(dim=-1) - 1).abs().max()) < 1e-12
    assert int(d["output_dim"]) == 27 and list(d["freq_bands"]) == [1.0, 2.0, 4.0, 8.0]
    assert [bc.column(4, c) for c in (0, 3, 6, 9, 26)] == [('x', 0, 0), ('sin', 0, 0), ('cos', 0, 0), ('sin', 1, 0), ('cos', 3, 2)]


def test_scene_accepts_the_packages_mlp_background_and_its_keys_are_the_references():
    from dreamwaltz_g_amd import scene as sc
    from dreamwaltz_g_amd.background import MLPBackground
    from dreamwaltz_g_amd import nerf_background, nerf_model
    bg = MLPBackground()
    assert isinstance(bg.encoder_bg, nerf_background.FreqEncoder) and (bg.encoder_bg.input_dim, bg.encoder_bg.degree, bg.encoder_bg.output_dim) == (3, 4, 27)
    assert isinstance(bg.bg_net, nerf_model.MLP) and [tuple(p.shape) for p in bg.parameters()] == mc.SHAPES
    assert nerf_background.unsupported_reason(bg.encoder_bg, bg.bg_net) is None
    s = sc.Scene(_cfg(), [nn.Module()], background=bg)
    assert s.background is bg and s.mlp_background is bg
    keys = str(np.load(GOLDEN)["keys"]).split("\n")
    assert sorted(k for k in s.state_dict() if k.startswith("background.")) == sorted("background." + k for k in keys)
    assert sorted(bg.state_dict()) == sorted(keys)

    class Sub(MLPBackground):                                  # only the class itself
        pass
    with pytest.raises(NotImplementedError):
        sc.Scene(_cfg(), [nn.Module()], background=Sub())
    with pytest.raises(NotImplementedError, match="forward_views"):
        s.forward_views([{}], [None])
    assert sc.Scene(_cfg(), [nn.Module()]).mlp_background is None
    # skip_bg: zeros, no launch
    z = bg({'c2w': torch.eye(4)[None], 'intrinsics': torch.eye(3)[None], 'image_height': 3, 'image_width': 5}, skip_bg=True)
    assert tuple(z.shape) == (1, 3, 5, 3) and not z.any()
    with pytest.raises(KeyError, match="intrinsics"):
        bg({'c2w': torch.eye(4)[None], 'image_height': 3, 'image_width': 5})


def test_load_state_dict_of_background_keys_moves_the_parameter_epoch():
    from dreamwaltz_g_amd import optim, scene as sc
    from dreamwaltz_g_amd.background import MLPBackground
    a, b = MLPBackground(), MLPBackground()
    s = sc.Scene(_cfg(), [nn.Module()], background=a)
    s.avatar.reset_by_state_dict = lambda sd: None
    s.avatar.invalidate_caches = lambda: None
    opt = a.get_optimizer()
    assert opt is a.get_optimizer() and type(opt) is optim.FlatAdan
    pg = opt.param_groups[0]
    assert (pg["lr"], pg["eps"], pg["weight_decay"], pg["max_grad_norm"], pg["betas"], pg["no_prox"]) == (0.001, 1e-8, 2e-5, 5.0, (0.98, 0.92, 0.99), False)
    epoch = optim.PARAM_EPOCH[0]
    s.load_state_dict({"background." + k: v for k, v in b.state_dict().items()}, strict=False)
    assert optim.PARAM_EPOCH[0] == epoch + 1
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    assert all(p.data_ptr() == opt.buf.flat.data_ptr() + 4 * off for p, (off, n) in zip(a.parameters(), opt.buf.slices))     # still views
    s.load_state_dict({}, strict=False)
    assert optim.PARAM_EPOCH[0] == epoch + 1
    c = MLPBackground.from_reference(b)
    assert all(torch.equal(p, q) for p, q in zip(c.parameters(), b.parameters())) and c.reference[0] is b


class _StubRenderer:
    def __init__(self, overflows):
        self.overflows = overflows
        self.async_pair_count = True

    def consume_overflow(self):
        if self.overflows > 0:
            self.overflows -= 1
            return True
        return False


class _StubScene(nn.Module):
    """A scene whose image depends on the background's last bias only: what the redo loop needs."""

    def __init__(self, overflows=0):
        super().__init__()
        from dreamwaltz_g_amd.background import MLPBackground
        self.background = MLPBackground()
        self.renderer = _StubRenderer(overflows)
        self.device = torch.device("cpu")
        self.calls = 0

    @property
    def mlp_background(self):
        return self.background

    def forward(self, data, **kwargs):
        self.calls += 1
        return {'image': self.background.bg_net.net[1].bias.view(1, 1, 1, 3).expand(1, 2, 2, 3) * float(self.calls)}


def trainer_mod():
    from dreamwaltz_g_amd import trainer
    return trainer


def _trainer(model, **kw):
    cfg = _cfg()
    cfg.prompt.text_augmentation = False
    opts = {'background': model.background.get_optimizer()} if hasattr(model.background, "get_optimizer") else {}
    return trainer_mod().SDSTrainer(cfg, model, lambda **k: {'diffusion_loss': k['inputs'].sum()}, opts, use_controlnet=False, **kw)


def test_the_redo_loop_leaves_no_first_attempt_background_gradient():
    model = _StubScene(overflows=1)
    tr = _trainer(model)
    opt = tr.optimizers['background']
    tr._begin_step(1.0)
    tr._view({'smpl_inputs': None})
    assert tr.redone_frames == 1 and model.calls == 2
    # attempt 1 would have left 4 per channel (2 x 2 pixels x 1), attempt 2 leaves 8: 12 if the first survived
    assert torch.equal(model.background.bg_net.net[1].bias.grad, torch.full((3,), 8.0))
    assert float(opt.buf.grad.sum()) == 24.0
    # without an overflow nothing is zeroed in between: two views of one step would accumulate (the trainer refuses them before)
    model2 = _StubScene(overflows=0)
    tr2 = _trainer(model2)
    tr2._begin_step(1.0)
    tr2._view({'smpl_inputs': None})
    assert tr2.redone_frames == 0 and torch.equal(model2.background.bg_net.net[1].bias.grad, torch.full((3,), 4.0))
    tr2._begin_step(1.0)                                    # and the next step starts from zero: the entry owns its buffers
    assert not tr2.optimizers['background'].buf.grad.any()


def test_trainer_refusals_name_the_mlp_background():
    from dreamwaltz_g_amd import step_graph
    model = _StubScene()
    tr = _trainer(model)
    with pytest.raises(NotImplementedError, match="MLP background"):
        tr.train_step([{'smpl_inputs': None}, {'smpl_inputs': None}])
    assert model.calls == 0 and tr.train_step_index == 0
    tr.set_views(2)
    with pytest.raises(NotImplementedError, match="MLP background"):
        tr.train_step({'smpl_inputs': None})
    tr.set_views(1)
    with pytest.raises(NotImplementedError, match="MLP background"):
        tr.nerf2gs_step({'smpl_inputs': None}, None)
    with pytest.raises(NotImplementedError, match="MLP background"):
        step_graph.GraphedTrainStep(tr, {}, {})
    # several ranks: refused by the constructor, before sync_replicas() broadcasts anything -- with a dist object and the package's own
    # optimizer dict carrying 'background', as a real multi-rank run has them
    from dreamwaltz_g_amd import optim

    class _Dist:
        calls = 0

        def broadcast(self, *a, **k):
            _Dist.calls += 1
    m2 = _StubScene()
    opts = optim.build_flat_optimizers({'a': optim.AdamSpec([{'params': [torch.nn.Parameter(torch.zeros(8))], 'lr': 1e-3}])}, 'cpu')
    opts['background'] = m2.background.get_optimizer()
    with pytest.raises(NotImplementedError, match="MLP background"):
        trainer_mod().SDSTrainer(_cfg(), m2, lambda **k: None, opts, use_controlnet=False, dist=_Dist(), world=2)
    assert _Dist.calls == 0 and model.calls == 0


def test_cabi_argument_errors_before_any_launch():
    from dreamwaltz_g_amd import _lib
    L = _lib.lib()
    fake, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)
    assert _lib.CONSTANTS["DWG_BACKGROUND_CAMERA_FLOATS"] == 16
    for args in ((0, fake, 4, 4, fake), (1, None, 4, 4, fake), (1, fake, 0, 4, fake), (1, fake, 4, -1, fake), (1, fake, 4, 4, None),
                 (1, odd, 4, 4, fake), (1, fake, 4, 4, odd), (70000, fake, 4, 4, fake), (1, fake, 1 << 16, 1 << 15, fake)):
        assert L.dwg_background_dirs(*args, None) != 0, args
    fwd = L.dwg_mlp_composite_forward
    for args in ((0, 4, 4, fake, fake, 48, 3, 1, fake, 48, fake), (1, 4, 4, None, fake, 48, 3, 1, fake, 48, fake), (1, 4, 4, fake, None, 48, 3, 1, fake, 48, fake),
                 (1, 4, 4, fake, fake, 48, 3, 1, None, 48, fake), (1, 4, 4, fake, fake, 48, 3, 1, fake, 48, None), (1, 4, 4, fake, fake, -1, 3, 1, fake, 48, fake),
                 (1, 4, 4, fake, fake, 48, 3, 1, fake, 47, fake), (1, 4, 4, odd, fake, 48, 3, 1, fake, 48, fake), (1, 4, 4, fake, fake, 48, 3, 1, fake, 48, odd)):
        assert fwd(*args, None) != 0, args
    bwd = L.dwg_mlp_composite_backward
    for args in ((0, 4, 4, fake, 48, 3, 1, fake, fake, fake, fake), (1, 4, 4, None, 48, 3, 1, fake, fake, fake, fake), (1, 4, 4, fake, 48, 3, 1, fake, fake, None, None),
                 (1, 4, 4, fake, 48, 3, 1, fake, None, fake, None), (1, 4, 4, fake, 48, 3, 1, None, fake, None, fake), (1, 4, 4, fake, 48, 3, -1, fake, fake, fake, fake),
                 (1, 4, 4, fake, 48, 3, 1, fake, fake, odd, fake), (1, 4, 4, odd, 48, 3, 1, fake, fake, fake, fake)):
        assert bwd(*args, None) != 0, args


def _bind_check(switch):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    env.pop("DWG_BIND_MLP_BACKGROUND", None)
    if switch is not None:
        env["DWG_BIND_MLP_BACKGROUND"] = switch
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mlp_background_bind_check.py")], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("DWG_MLP_BIND_CHECK ")][-1]
    return json.loads(line[len("DWG_MLP_BIND_CHECK "):])


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="needs the reference checkout (build container only)")
def test_bound_build_scene_binds_the_mlp_background_only_with_the_switch():
    for switch in (None, "0"):
        d = _bind_check(switch)
        assert d["raised"] is True and "DWG_BIND_MLP_BACKGROUND" in d["message"], d
    d = _bind_check("1")
    assert d["raised"] is False
    assert d["scene_class"] == "dreamwaltz_g_amd.scene.Scene" and d["background_class"] == "dreamwaltz_g_amd.background.MLPBackground"
    assert d["reference_built"] == 1 and d["weights_adopted"] is True
    assert d["keys"] == d["reference_keys"] and len(d["keys"]) == 4
    assert d["optimizer_class"] == "dreamwaltz_g_amd.optim.FlatAdan" and d["optimizer_again_is_same"] is True and d["params_are_views"] is True
    assert d["hyper"] == d["reference_hyper"] == [0.001, 1e-8, 2e-5, 5.0, [0.98, 0.92, 0.99], False]
