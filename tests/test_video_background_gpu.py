"""Video background on the device (csrc/background.hip through dreamwaltz_g_amd.background / Scene / GraphedAnimation) against the
reference's statements (core/system/background.py:140-155, core/system/scene.py:157-160) restated in tests/video_background_cases.py."""
import warnings

import numpy as np
import pytest
import torch

import dwg_import  # noqa: F401
from tests import video_background_cases as vc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _scene(res, frames, G=20000):
    from dreamwaltz_g_amd import camera, configs, scene as sc, sds_step
    from dreamwaltz_g_amd.background import VideoBackground
    cfg = configs.TrainConfig(); cfg.device = str(DEV); cfg.render.bg_color = (0.5, 0.5, 0.5)
    avatar, _, _ = sds_step.build_synthetic_avatar(G, DEV, seed=0)
    bg = VideoBackground.from_frames(frames, fps=30)
    scene = sc.Scene(cfg, avatar, background=bg, async_pair_count=True).to(DEV).eval()
    data = camera.make_camera(radius=2.0, azimuth=20.0, elevation=80.0, fovy=55.0, height=res, width=res, device=DEV)
    return scene, data, bg


def _fg_alpha(F, H, W, seed=0, planar=True):
    g = torch.Generator().manual_seed(seed)
    color = torch.rand(F, 3, H, W, generator=g).to(DEV)
    alpha = torch.rand(F, 1, H, W, generator=g).to(DEV)
    image = color.permute(0, 2, 3, 1) if planar else color.permute(0, 2, 3, 1).contiguous()      # the renderer's planar view
    return image, alpha.permute(0, 2, 3, 1)


@pytest.mark.parametrize("planar", [True, False])
def test_equal_size_composite_is_bit_identical_to_the_reference_statements(planar):
    from dreamwaltz_g_amd.background import VideoBackground, video_composite
    frames = vc.make_frames(6, 48, 40, seed=1)
    bg = VideoBackground.from_frames(frames)
    image, alpha = _fg_alpha(3, 48, 40, seed=2, planar=planar)
    out, image_bg = video_composite(image, alpha, bg, [4, 1, -1])
    for f, t in enumerate((4, 1, 5)):
        ref_bg = vc.reference_background(frames[t], 48, 40)                       # host division, as the reference
        assert torch.equal(image_bg[f].cpu(), ref_bg), f
        ref = vc.reference_composite(image[f:f + 1], alpha[f:f + 1], ref_bg)
        assert torch.equal(out[f:f + 1], ref), f
    assert out.stride() == image.stride()                                          # the layout torch's elementwise ops keep
    # get_background / get_background_like: the reference's surface
    assert torch.equal(bg.get_background(2).cpu(), torch.from_numpy(frames[2]))
    like = bg.get_background_like(3, image[:1])
    assert like.shape == (48, 40, 3) and torch.equal(like.cpu(), vc.reference_background(frames[3], 48, 40))


@pytest.mark.parametrize("src,dst", [((97, 131), (64, 64)), ((32, 48), (64, 96)), ((128, 96), (64, 48)), ((1080, 1920), (512, 512)),
                                     ((50, 64), (64, 64))])
def test_resampled_background_equals_the_restatement(src, dst):
    """(h, w) != (H, W): OpenCV's INTER_LINEAR rule (the exact 2x downscale on its area path) restated on the host -- every uint8 value
    equal, hence the divided floats too; two runs bit-identical."""
    from dreamwaltz_g_amd.background import VideoBackground, video_composite
    (h, w), (H, W) = src, dst
    frames = vc.make_frames(2, h, w, seed=h + w)
    bg = VideoBackground.from_frames(frames)
    ref = vc.reference_background(frames[1], H, W)
    got = bg.get_background_like(1, torch.empty(1, H, W, 3, device=DEV))
    assert torch.equal(got.cpu(), ref), (src, dst, float((got.cpu() - ref).abs().max()) * 255)
    image, alpha = _fg_alpha(2, H, W, seed=3)
    a, abg = video_composite(image, alpha, bg, [1, 0])
    b, bbg = video_composite(image, alpha, bg, [1, 0])
    assert torch.equal(a, b) and torch.equal(abg, bbg)
    assert torch.equal(abg[0].cpu(), ref) and torch.equal(abg[1].cpu(), vc.reference_background(frames[0], H, W))
    assert torch.equal(a[:1], vc.reference_composite(image[:1], alpha[:1], ref))


@pytest.mark.parametrize("src", [(40, 56), (80, 112)])
def test_backward_matches_torch_autograd_of_the_reference_expression(src):
    from dreamwaltz_g_amd.background import VideoBackground, video_composite
    H, W = 40, 56
    frames = vc.make_frames(3, src[0], src[1], seed=5)
    bg = VideoBackground.from_frames(frames)
    image, alpha = _fg_alpha(2, H, W, seed=6)
    wgt = torch.randn(2, H, W, 3, generator=torch.Generator().manual_seed(7)).to(DEV)
    x1, a1 = image.detach().clone().requires_grad_(True), alpha.detach().clone().requires_grad_(True)
    out, _ = video_composite(x1, a1, bg, [2, 0])
    (out * wgt).sum().backward()
    x2, a2 = image.detach().clone().requires_grad_(True), alpha.detach().clone().requires_grad_(True)
    ref_bg = torch.stack([vc.reference_background(frames[t], H, W) for t in (2, 0)]).to(DEV)
    ((x2 + ref_bg * (1 - a2)) * wgt).sum().backward()
    assert torch.equal(x1.grad, x2.grad)
    err = float((a1.grad - a2.grad).abs().max()) / max(float(a2.grad.abs().max()), 1e-30)
    assert err <= 1e-6, err
    # a contiguous upstream gradient and one with the planar layout give the same bits
    x3, a3 = image.detach().contiguous().requires_grad_(True), alpha.detach().clone().requires_grad_(True)
    out3, _ = video_composite(x3, a3, bg, [2, 0])
    (out3 * wgt).sum().backward()
    assert torch.equal(a3.grad, a1.grad)


def test_scene_forward_composites_the_video_and_colour_modes_win():
    from dreamwaltz_g_amd import synth
    from dreamwaltz_g_amd import scene as sc
    frames = vc.make_frames(5, 64, 64, seed=8)
    scene, data, bg = _scene(64, frames)
    pose = synth.random_smpl_inputs(seed=1, device=DEV)
    with torch.inference_mode():
        o = scene.forward(dict(data, frame_index=3), smpl_observed_inputs=pose, use_densifier=False)
        ref_bg = vc.reference_background(frames[3], 64, 64)
        assert o['image_bg'].shape == (64, 64, 3) and torch.equal(o['image_bg'].cpu(), ref_bg)
        assert torch.equal(o['image'], vc.reference_composite(o['image_fg'], o['alpha'], ref_bg))
        assert float(o['alpha'].max()) > 0.5 and float(o['alpha'].min()) < 0.5       # the avatar covers part of the frame
        # wrap and range: the reference's list semantics
        last = scene.forward(dict(data, frame_index=-1), smpl_observed_inputs=pose, use_densifier=False)
        assert torch.equal(last['image_bg'].cpu(), vc.reference_background(frames[4], 64, 64))
        with pytest.raises(IndexError):
            scene.forward(dict(data, frame_index=5), smpl_observed_inputs=pose, use_densifier=False)
        # a pure colour bg_mode wins over the video (scene.py:153-160)
        w = scene.forward(dict(data, frame_index=3), smpl_observed_inputs=pose, use_densifier=False, bg_mode="white")
        scene.background = None
        plain = scene.forward(dict(data, frame_index=3), smpl_observed_inputs=pose, use_densifier=False, bg_mode="white")
        scene.background = bg
    assert torch.equal(w['image'], plain['image']) and torch.equal(w['image_bg'], plain['image_bg'])
    assert isinstance(scene, sc.Scene)


def test_forward_frames_with_distinct_indices_equals_forward_per_frame():
    from dreamwaltz_g_amd import synth
    frames = vc.make_frames(6, 96, 96, seed=9)                        # resampled to the 64^2 render
    scene, data, bg = _scene(64, frames)
    poses = [synth.random_smpl_inputs(seed=20 + i, device=DEV) for i in range(4)]
    idx = [5, 0, 3, 1]
    with torch.inference_mode():
        single = [scene.forward(dict(data, frame_index=t), smpl_observed_inputs=p, use_densifier=False) for p, t in zip(poses, idx)]
        single = [{k: o[k].clone() for k in ("image", "image_fg", "image_bg", "alpha")} for o in single]
        for batch in (scene.forward_frames(data, poses, frame_indices=idx),
                      scene.forward_frames([dict(data, frame_index=t) for t in idx], poses),
                      scene.forward_frames(data, poses, frame_indices=torch.tensor(idx, dtype=torch.int32, device=DEV))):
            for f in range(4):
                for k in ("image", "image_fg", "alpha"):
                    assert torch.equal(batch[k][f:f + 1], single[f][k]), (f, k)
                assert torch.equal(batch["image_bg"][f], single[f]["image_bg"]), f
        with pytest.raises(ValueError):
            scene.forward_frames(data, poses)                          # no index per frame
        with pytest.raises(IndexError):
            scene.forward_frames(data, poses, frame_indices=[0, 1, 2, 6])


def test_graphed_replay_with_a_changing_frame_index_equals_eager_frames_without_host_sync():
    from dreamwaltz_g_amd import player, synth
    frames = vc.make_frames(7, 64, 64, seed=10)
    scene, data, bg = _scene(64, frames)
    poses = [synth.random_smpl_inputs(seed=30 + i, device=DEV) for i in range(4)]
    idx = [2, 6, 0, -2]
    with torch.inference_mode():
        eager = [scene.forward(dict(data, frame_index=t), smpl_observed_inputs=p, use_densifier=False) for p, t in zip(poses, idx)]
        eager = [{k: o[k].clone() for k in ("image", "image_bg")} for o in eager]
    pl = player.GraphedAnimation(scene, data, poses[0], warmup_poses=poses[:2], frame_index=idx[0])
    torch.cuda.synchronize()
    got = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for p, t in zip(poses, idx):
            o = pl.replay(p, frame_index=t)
            got.append({k: o[k].clone() for k in ("image", "image_bg")})
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert pl.check()
    for f in range(4):
        for k in ("image", "image_bg"):
            assert torch.equal(got[f][k], eager[f][k]), (f, k)
    with pytest.raises(IndexError):
        pl.replay(poses[0], frame_index=7)
    pl.close()


def test_the_composite_and_its_indices_never_sync_the_host():
    from dreamwaltz_g_amd import synth
    from dreamwaltz_g_amd.background import VideoBackground, video_composite
    frames = vc.make_frames(5, 64, 64, seed=11)
    bg = VideoBackground.from_frames(frames)
    image, alpha = _fg_alpha(3, 64, 64, seed=12)
    video_composite(image, alpha, bg, [0, 1, 2])                       # uploads the store, builds the index table
    dev_idx = torch.tensor([3, 3, 1], dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for idx in ([1, 2, 3], [4, 0, 2], dev_idx):
            video_composite(image, alpha, bg, idx)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    # forward_frames: whatever the rasterizer chain does, the video background adds no synchronisation
    scene, data, _ = _scene(64, frames)
    poses = [synth.random_smpl_inputs(seed=40 + i, device=DEV) for i in range(2)]
    with torch.inference_mode():
        scene.forward_frames(data, poses, frame_indices=[1, 4])
        torch.cuda.synchronize()
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                scene.forward_frames(data, poses, frame_indices=[3, 0])
            finally:
                torch.cuda.set_sync_debug_mode(0)
    mine = [str(r.filename) + ":" + str(r.lineno) for r in rec if r.filename.endswith("background.py")]
    assert not mine, mine
