"""GPU tests of the stage-II learned MLP background (boundary B23, dreamwaltz_g_amd.background): the directions kernel, the image, the
composite and its backward, Scene.forward / forward_frames, and three SDSTrainer steps with a stub guidance.

THE BOUNDS.
  dirs, image: max|err| / max|ref| against the float64 restatement (tests/mlp_background_cases.py) at most 2 x (the fp32 torch
      composition's error) + 1e-7 -- the project's rule.
  weight and bias gradients: relative L2 against float64 within nerf_background_cases.F32_BWD = 1e-4 (B22's bound for fp32 sums of this kind).
  composite forward and backward, Scene.forward, forward_frames: bit for bit against the same fp32 statements in torch / the composition of
      the public pieces.
  the trainer's steps: the background's parameters within the Adan rule (tests/adan_cases.bound) of the float64 chain; the avatar's
      parameters bit-identical to the same steps with the background image supplied as a constant tensor."""
import numpy as np
import pytest
import torch

import dwg_import  # noqa: F401
from tests import adan_cases as ac
from tests import mlp_background_cases as mc
from tests import nerf_background_cases as bc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RUNS = [(s, F) for s in mc.SIZES for F in (1, 3)]
IDS = ["%dx%dx%d" % (s[0], s[1], F) for s, F in RUNS]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _background():
    from dreamwaltz_g_amd.background import MLPBackground
    bg = MLPBackground().to(DEV)
    with torch.no_grad():
        for p, w in zip(bg.parameters(), mc.weights()):
            p.copy_(_t(w))
    return bg


_ORACLE = {}


def _oracle(size, F):
    """The float64 restatement of one run, computed once and shared."""
    if (size, F) not in _ORACLE:
        H, W = size
        c2w, K = mc.cameras(F, H, W)
        fg, alpha = mc.foreground(F, H, W)
        _ORACLE[(size, F)] = (c2w, K, fg, alpha, mc.oracle(c2w, K, H, W, mc.weights(), mc.cotangent(F, H, W), fg, alpha))
    return _ORACLE[(size, F)]


@pytest.mark.parametrize("size,F", RUNS, ids=IDS)
def test_dirs_image_and_gradients_against_float64(size, F):
    from dreamwaltz_g_amd import background as bgm
    H, W = size
    c2w, K, fg, alpha, o = _oracle(size, F)
    got = bgm.background_dirs(_t(c2w), _t(K), H, W)
    assert tuple(got.shape) == (F * H * W, 3) and got.dtype == torch.float32
    comp = mc.dirs(torch.from_numpy(c2w), torch.from_numpy(K), H, W, torch.float32)
    e, b = bc.rel_max(got.cpu(), o["dirs"]), 2 * bc.rel_max(comp, o["dirs"]) + 1e-7
    print("background_dirs %dx%dx%d: native %.3g, bound %.3g" % (H, W, F, e, b))
    assert e <= b, (e, b)
    assert torch.equal(got, bgm.background_dirs(_t(c2w), _t(K), H, W))
    bg = _background()
    data = {'c2w': _t(c2w), 'intrinsics': _t(K), 'image_height': H, 'image_width': W}
    img = bg(data)
    assert tuple(img.shape) == (F, H, W, 3) and img.requires_grad
    wb32 = [torch.from_numpy(w) for w in mc.weights()]
    comp = mc.image(mc.dirs(torch.from_numpy(c2w), torch.from_numpy(K), H, W, torch.float32), wb32, torch.float32).view(F, H, W, 3)
    e, b = bc.rel_max(img.cpu(), o["image"]), 2 * bc.rel_max(comp, o["image"]) + 1e-7
    print("MLPBackground image %dx%dx%d: native %.3g, bound %.3g" % (H, W, F, e, b))
    assert e <= b, (e, b)
    img.backward(_t(mc.cotangent(F, H, W)))
    for i, p in enumerate(bg.parameters()):
        assert bc.rel_l2(p.grad.cpu(), o["grads"][i]) <= bc.F32_BWD, (i, bc.rel_l2(p.grad.cpu(), o["grads"][i]))
    with torch.no_grad():
        assert torch.equal(bg(data), img.detach()) and not bg(data).requires_grad
        assert not bg(data, skip_bg=True).any()
    # camera f of a batch is that camera alone
    if F > 1:
        one = bgm.background_dirs(_t(c2w[1:2]), _t(K[1:2]), H, W)
        assert torch.equal(one, got[H * W:2 * H * W])


@pytest.mark.parametrize("planar", [True, False], ids=["planar", "contiguous"])
@pytest.mark.parametrize("size,F", RUNS, ids=IDS)
def test_composite_forward_and_backward_bit_for_bit(size, F, planar):
    from dreamwaltz_g_amd.background import mlp_composite
    H, W = size
    c2w, K, fg, alpha, o = _oracle(size, F)
    assert (alpha == 0).any() and (alpha == 1).any() and ((alpha > 0) & (alpha < 1)).any()
    bg = o["image"].float().to(DEV)
    fg_t = _t(fg).permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1) if planar else _t(fg)          # the rasterizer hands permuted views
    al_t = _t(alpha).permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    assert fg_t.is_contiguous() != planar or F * H * W == 1
    x1, a1, b1 = (t.detach().clone().requires_grad_(True) for t in (fg_t, al_t, bg))
    if planar:
        x1 = fg_t.detach().requires_grad_(True)
    out = mlp_composite(x1, a1, b1)
    assert out.stride() == x1.stride()
    cot = _t(mc.cotangent(F, H, W))
    out.backward(cot)
    # the same fp32 statements in torch, each rounded on its own
    with torch.no_grad():
        om = 1.0 - al_t
        ref = fg_t + bg * om
        d_alpha = -((cot[..., 0:1] * bg[..., 0:1] + cot[..., 1:2] * bg[..., 1:2]) + cot[..., 2:3] * bg[..., 2:3])
        d_bg = cot * om
    assert torch.equal(out.detach(), ref)
    assert torch.equal(x1.grad, cot) and torch.equal(a1.grad, d_alpha) and torch.equal(b1.grad, d_bg)
    # alpha exactly 1 hides the background, exactly 0 adds it whole
    assert torch.equal(out.detach()[(al_t == 1).expand_as(out)], fg_t[(al_t == 1).expand_as(out)])
    assert not b1.grad[(al_t == 1).expand_as(out)].any()
    # against float64 too (the golden's statement): the background's rounding to fp32 and three fp32 operations on values below 2,
    # 6e-8 x 2 each at the most
    assert bc.rel_max(out.detach().cpu(), o["composite"]) <= 5e-7 and bc.rel_l2(a1.grad.cpu(), o["d_alpha"]) <= 1e-6
    # only the gradients asked for
    x2, a2 = fg_t.detach().clone().requires_grad_(True), al_t.detach().clone()
    mlp_composite(x2, a2, bg).backward(cot)
    assert torch.equal(x2.grad, cot) and a2.grad is None


def _scene(G=4000):
    from dreamwaltz_g_amd import configs, scene as sc, sds_step
    cfg = configs.TrainConfig(); cfg.device = str(DEV); cfg.render.bg_color = (0.5, 0.5, 0.5)
    cfg.prompt.text_augmentation = False
    avatar, _, _ = sds_step.build_synthetic_avatar(G, DEV, seed=0)
    scene = sc.Scene(cfg, avatar, background=_background(), async_pair_count=True).to(DEV)
    return cfg, scene, avatar


def _camera(f, res):
    from dreamwaltz_g_amd import camera
    data = camera.make_camera(radius=2.0, azimuth=20.0 + 50.0 * f, elevation=80.0 - 5.0 * f, fovy=55.0, height=res, width=res, device=DEV)
    fl = 0.5 * res / float(data["tanfov"][0])
    data["intrinsics"] = torch.tensor([[[fl, 0.0, 0.5 * res + 1.5], [0.0, fl, 0.5 * res - 2.25], [0.0, 0.0, 1.0]]], device=DEV)
    return data


def test_scene_forward_is_the_composition_of_the_public_pieces_and_frames_equal_forward():
    from dreamwaltz_g_amd import synth
    from dreamwaltz_g_amd.background import mlp_composite
    _, scene, _ = _scene()
    scene.eval()
    res = 64
    poses = [synth.random_smpl_inputs(seed=30 + i, device=DEV) for i in range(3)]
    cams = [_camera(f, res) for f in range(3)]
    with torch.no_grad():
        single = []
        for pose, data in zip(poses, cams):
            o = scene.forward(data, smpl_observed_inputs=pose, use_densifier=False)
            bg = scene.background(data)
            assert tuple(o['image_bg'].shape) == (1, res, res, 3) and torch.equal(o['image_bg'], bg)
            assert torch.equal(o['image'], mlp_composite(o['image_fg'], o['alpha'], bg))
            assert torch.equal(o['image'], o['image_fg'] + bg * (1 - o['alpha']))
            single.append({k: o[k].clone() for k in ("image", "image_fg", "image_bg", "alpha")})
        assert float(single[0]['alpha'].max()) > 0.5 and float(single[0]['alpha'].min()) < 0.5
        batch = scene.forward_frames(cams, poses)
        for f in range(3):
            for k in ("image", "image_fg", "image_bg", "alpha"):
                assert torch.equal(batch[k][f:f + 1], single[f][k]), (f, k)
        shared = scene.forward_frames(cams[0], poses)                     # one camera: the background is computed once
        for f in range(3):
            assert torch.equal(shared["image_bg"][f:f + 1], single[0]["image_bg"])
            assert torch.equal(shared["image"][f:f + 1], shared["image_fg"][f:f + 1] + single[0]["image_bg"] * (1 - shared["alpha"][f:f + 1]))
        # a pure colour bg_mode wins over the learned background (scene.py:153-166)
        w = scene.forward(cams[0], smpl_observed_inputs=poses[0], use_densifier=False, bg_mode="white")
        assert float(w['image_bg'].min()) == 1.0
    with pytest.raises(NotImplementedError, match="MLP background"):
        scene.forward_views(cams[:2], poses[:2])


RES = 64


def _trainer(with_optimizer):
    """An SDSTrainer of a small avatar over the learned background with the stub guidance loss = sum(image * W); with_optimizer: the
    background's Adan under 'background'.  -> (trainer, scene, optimizers, W)."""
    from dreamwaltz_g_amd import sds_step, trainer as tr
    cfg, scene, avatar = _scene()
    opts = avatar.get_optimizer(cfg)
    scene.train()
    if with_optimizer:
        opts['background'] = scene.background.get_optimizer(cfg)
    wimg = torch.randn(1, RES, RES, 3, generator=torch.Generator().manual_seed(6)).to(DEV)
    return tr.SDSTrainer(cfg, scene, sds_step._ImageLoss(wimg), opts, {}, use_controlnet=False, max_step=100), scene, opts, wimg


def _step(t, scene, k, constant_bg=None):
    """Step k (its own camera and pose).  constant_bg: the background image as a constant tensor.  -> the step's data, alpha, image_bg."""
    from dreamwaltz_g_amd import synth
    data = dict(_camera(k, RES))
    data['smpl_inputs'] = synth.random_smpl_inputs(seed=40 + k, device=DEV)
    if constant_bg is not None:
        scene.background.forward = lambda d, skip_bg=False: constant_bg
    _, ro, _, _ = t.train_step(data)
    return {"data": data, "alpha": ro['alpha'].detach().clone(), "image_bg": ro['image_bg'].detach().clone()}


def _adan_state(scene, o):
    got = {"p": torch.cat([p.detach().reshape(-1) for p in scene.background.parameters()])}
    for key in ac.STATES:
        buf = getattr(o, key)
        got[key] = torch.cat([buf[off:off + n] for off, n in o.buf.slices])
    return got


def test_three_trainer_steps_background_against_the_float64_chain_and_the_avatar_bit_identical(tmp_path):
    t, scene, opts, wimg = _trainer(True)
    p0 = torch.cat([p.detach().reshape(-1) for p in scene.background.parameters()]).cpu()
    recs = [_step(t, scene, k) for k in range(3)]
    flat_after = opts.buffers.flat.detach().clone()
    o = opts['background']
    assert o.device_step_counts() == [3]
    # the float64 chain: the background's image, the composite's d_bg = d_image (1 - alpha), autograd to the four tensors, Adan -- with the
    # run's own alpha as the input; and the same chain composed in fp32 torch, whose error sets the bound
    hyper = ac.hypers([1e-3], 2e-5, False)
    chains = {}
    for dtype in (torch.float64, torch.float32):
        c = ac.Chain([p0], hyper, 5.0, dtype)
        rec = None
        for r in recs:
            params, off = [], 0
            for s in mc.SHAPES:
                n = int(np.prod(s))
                params.append(c.p[0][off:off + n].view(s).clone().requires_grad_(True))
                off += n
            d = mc.dirs(r["data"]["c2w"].cpu(), r["data"]["intrinsics"].cpu(), RES, RES, dtype)
            img = mc.image(d, params, dtype).view(1, RES, RES, 3)
            img.backward(wimg.cpu().to(dtype) * (1 - r["alpha"].cpu().to(dtype)))
            rec = c.step([torch.cat([p.grad.reshape(-1) for p in params])])
        chains[dtype] = rec
    got = _adan_state(scene, o)
    for key in ("p",) + ac.STATES:
        want, comp = chains[torch.float64][key][0], chains[torch.float32][key][0]
        e, b = ac.rel_max(got[key].cpu(), want), ac.bound(comp, want)
        print("trainer steps, background %s: native %.3g, bound %.3g" % (key, e, b))
        assert e <= b, (key, e, b)
    assert not torch.equal(got["p"].cpu(), p0)                                                  # it learned something
    # the avatar: the same three steps with each step's background image as a constant tensor
    t2, scene2, opts2, _ = _trainer(False)
    for k, r in enumerate(recs):
        assert torch.equal(_step(t2, scene2, k, constant_bg=r["image_bg"])["alpha"], r["alpha"]), k
    assert 'background' not in opts2 and torch.equal(opts2.buffers.flat, flat_after)
    # a full checkpoint carries the Adan state in the optimizers list: loaded into a fresh trainer, the fourth step gives the same bits
    path = t.save_checkpoint(str(tmp_path), full=True)
    saved = torch.load(path, weights_only=False)
    assert sorted(saved['optimizers'][-1]) == sorted(["max_grad_norm", "param_groups", "exp_avg", "exp_avg_sq", "exp_avg_diff", "neg_pre_grad"])
    assert saved['optimizers'][-1]["param_groups"][0]["step"] == 3
    assert sum(k.startswith("background.") for k in saved['model']) == 4
    t3, scene3, opts3, _ = _trainer(True)
    assert not torch.equal(opts3.buffers.flat, flat_after)
    t3.load_checkpoint(path)
    assert t3.train_step_index == 3 and opts3['background'].device_step_counts() == [3]
    loaded = _adan_state(scene3, opts3['background'])
    assert all(torch.equal(loaded[k], got[k]) for k in got)
    _step(t, scene, 3)
    _step(t3, scene3, 3)
    assert torch.equal(opts3.buffers.flat, opts.buffers.flat)
    want, back = _adan_state(scene, o), _adan_state(scene3, opts3['background'])
    assert all(torch.equal(back[k], want[k]) for k in want) and not torch.equal(want["p"], got["p"])
