"""Gaussian scene background on the device (boundary B24: csrc/scene_gaussians.hip through dreamwaltz_g_amd.background / Scene /
GraphedAnimation) against the reference's statements (core/gaussian/gaussian_model.py:35-94, core/system/scene.py:123-132) restated in
float64 in tests/gs_background_cases.py.

How an error is measured: per element, |x - float64| in units of the fp32 spacing at the float64 result -- for the colours at
max(|result|, 0.5), because every colour is a sum that passes through `+ 0.5` before the clamp at 0 and its rounding has that size however
small the clamped result is.  Allowed per output: twice the worst such error of torch's own fp32 statements (the reference's expressions,
evaluated here on the device) on the same inputs, and never less than 1: the factor 2 covers an exp / sqrt / division that is rounded as
well, only differently.  Measured on an MI355X (activation, N = 1021): see DESIGN section 5s."""
import warnings

import pytest
import torch

import dwg_import  # noqa: F401
from tests import gs_background_cases as gc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ATTRS = ("positions", "opacities", "colors", "scales", "quaternions")
WIDTH = {"positions": 3, "opacities": 1, "colors": 3, "scales": 3, "quaternions": 4}


def _offset(t):
    """The same values as a view at storage_offset 1 of a device buffer: 4-byte aligned, never 16."""
    flat = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    flat[1:].copy_(t.reshape(-1))
    v = flat[1:].view(t.shape)
    assert v.storage_offset() == 1 and v.data_ptr() % 16 == 4
    return v


def _background(n, seed=0, sh_levels=1, offset=False, **over):
    from dreamwaltz_g_amd.background import GaussianBackground
    arrays = dict(gc.scene_arrays(n, seed=seed), **over)
    arrays = {k: (_offset(v) if offset else v.to(DEV)) for k, v in arrays.items()}
    return GaussianBackground.from_tensors(**arrays, sh_levels=sh_levels).to(DEV)


def _bound(name, got, torch32, ref64, floor=0.0):
    e_ours, e_torch = gc.ulps(got, ref64, floor), gc.ulps(torch32, ref64, floor)
    print("%s: ours %.3f ulp, torch fp32 %.3f ulp" % (name, e_ours, e_torch))
    assert e_ours <= max(2.0 * e_torch, 1.0), (name, e_ours, e_torch)


# ---- activation ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 1021])
def test_activation_is_within_twice_torchs_own_fp32_error_of_float64(n):
    from dreamwaltz_g_amd import renderer
    g = torch.Generator().manual_seed(n)
    for special in ("zero", "tiny"):                       # N = 1 holds one special quaternion row at a time
        logits = torch.rand(n, 1, generator=g) * 24 - 12
        log_scales = torch.rand(n, 3, generator=g) * 10 - 9
        dc = torch.rand(n, 1, 3, generator=g) * 6 - 3
        dc[0, 0, 0], dc[n // 2, 0, 1] = -2.5, -1.7724538      # C0 dc + 0.5 clamps to 0, and sits at the edge of the clamp
        quats = torch.randn(n, 4, generator=g)
        quats[0] = 0.0 if special == "zero" or n > 1 else torch.tensor([0.0, 1e-20, 0.0, 0.0])
        if n > 1:
            quats[1] = torch.tensor([0.6e-20, 0.0, -0.8e-20, 0.0])              # norm 1e-20
        bg = _background(n, opacities=logits, scales=log_scales, sh_features_dc=dc, quaternions=quats)
        block = bg.activated()
        ref = gc.activations64(bg._opacities, bg._scales, bg._quaternions, bg._sh_features_dc)
        sh = torch.cat((bg._sh_features_dc, bg._sh_features_rest), dim=1)       # the reference's 48-float cat, read at coefficient 0
        torch32 = {"opacities": torch.sigmoid(bg._opacities.view(-1, 1)), "scales": torch.exp(bg._scales),
                   "quaternions": torch.nn.functional.normalize(bg._quaternions),
                   "colors": renderer.get_colors(sh_features=sh, directions=None, sh_levels=1)}
        for k in ("opacities", "scales", "quaternions", "colors"):
            assert block[k].shape == ref[k].shape and block[k].dtype == torch.float32
            _bound("%s N=%d %s" % (k, n, special), block[k], torch32[k], ref[k], floor=0.5 if k == "colors" else 0.0)
        if special == "zero" or n > 1:
            assert torch.equal(block["quaternions"][0], torch.zeros(4, device=DEV))        # as F.normalize: exactly 0
        assert float(block["colors"][0, 0]) == 0.0
        out = bg.gaussians()
        assert out.sh_features is None and out.positions.data_ptr() == bg._positions.data_ptr()         # positions are not copied
        assert out.colors.data_ptr() == block["colors"].data_ptr() and bg.activation_launches == 1


# ---- merge -----------------------------------------------------------------------------------------------------------------------------
def _parts(n_avatars, n_a, seed):
    from dreamwaltz_g_amd.avatar import GaussianOutput
    g = torch.Generator().manual_seed(seed)
    return [GaussianOutput(**{k: _offset(torch.randn(n_a + i, WIDTH[k], generator=g)) for k in ATTRS}) for i in range(n_avatars)]


@pytest.mark.parametrize("n_bg", [1, 5, 1021])
@pytest.mark.parametrize("n_a", [1, 3, 257])
@pytest.mark.parametrize("n_avatars", [1, 2, 3])
def test_merge_equals_torch_cat_for_unaligned_rows_and_leaves_guard_rows_alone(n_avatars, n_a, n_bg):
    from dreamwaltz_g_amd.background import scene_merge
    bg = _background(n_bg, seed=n_bg, offset=True)
    parts = _parts(n_avatars, n_a, seed=n_a)
    scene = bg.gaussians()
    want = {k: torch.cat([p[k] for p in parts] + [scene[k]], dim=0) for k in ATTRS}
    total = n_avatars * n_a + sum(range(n_avatars)) + n_bg
    got = scene_merge(parts, bg)
    for k in ATTRS:
        assert got[k].shape == (total, WIDTH[k]) and torch.equal(got[k], want[k]), k
    assert got.sh_features is None
    # into rows of larger buffers, as forward_frames writes them: the rows around stay as they were
    guard = 7.25
    bufs = {k: torch.full((total + 2, WIDTH[k]), guard, dtype=torch.float32, device=DEV) for k in ATTRS}
    scene_merge(parts, bg, out=tuple(bufs[k][1:1 + total] for k in ATTRS))
    for k in ATTRS:
        assert torch.equal(bufs[k][1:1 + total], want[k]), k
        assert bool((bufs[k][0] == guard).all()) and bool((bufs[k][-1] == guard).all()), k
    # backward: each part gets its row slices of the incoming gradients, as torch.cat's backward hands them out
    leaves = [[p[k].clone().requires_grad_(True) for k in ATTRS] for p in parts]
    twins = [[t.detach().clone().requires_grad_(True) for t in row] for row in leaves]
    from dreamwaltz_g_amd.avatar import GaussianOutput
    merged = scene_merge([GaussianOutput(**dict(zip(ATTRS, row))) for row in leaves], bg)
    wgt = {k: torch.randn(total, WIDTH[k], generator=torch.Generator().manual_seed(3)).to(DEV) for k in ATTRS}
    sum((merged[k] * wgt[k]).sum() for k in ATTRS).backward()
    sum((torch.cat([row[a] for row in twins] + [scene[k]], dim=0) * wgt[k]).sum() for a, k in enumerate(ATTRS)).backward()
    for row, twin in zip(leaves, twins):
        for t, u in zip(row, twin):
            assert t.grad is not None and torch.equal(t.grad, u.grad)
    assert all(p.grad is None for p in bg.parameters())


# ---- view-dependent colour -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [2, 3, 4])
def test_view_dependent_colour_is_within_twice_torchs_own_fp32_error_of_float64(levels):
    from dreamwaltz_g_amd import renderer
    from dreamwaltz_g_amd.background import scene_merge
    n = 1021
    bg = _background(n, seed=levels, sh_levels=levels, sh_features_rest=torch.rand(n, 15, 3, generator=torch.Generator().manual_seed(9)) * 2 - 1)
    sh = torch.cat((bg._sh_features_dc, bg._sh_features_rest), dim=1)
    c2w = torch.eye(4, device=DEV)[None].clone()
    for name, cam in (("far", torch.tensor([0.3, -2.0, 0.8])), ("near", bg._positions[17].cpu() + torch.tensor([6e-4, -8e-4, 0.0]))):
        cam = cam.to(DEV)
        got = bg.gaussians(cam[None]).colors
        ref = gc.colors64(bg._sh_features_dc, bg._sh_features_rest, bg._positions, cam, levels)
        torch32 = renderer.GaussianRenderer().compute_colors(sh, positions=bg._positions, camera_positions=cam[None], sh_levels=levels)
        _bound("colours L=%d %s" % (levels, name), got, torch32, ref, floor=0.5)
        assert float(got.min()) == 0.0 and float(got.max()) > 1.0                  # both sides of the clamp occur
        # the merge evaluates the same statements for the scene's rows, camera read in place from a c2w (element stride 4)
        c2w[0, :3, 3] = cam
        parts = _parts(1, 3, seed=1)
        merged = scene_merge(parts, bg, c2w[:, :3, 3])
        assert torch.equal(merged.colors[3:], got) and torch.equal(merged.colors[:3], parts[0].colors)
        assert torch.equal(merged.positions[3:], bg._positions)
    with pytest.raises(ValueError, match="view dependent"):
        bg.gaussians()


def test_device_colours_and_quaternions_equal_the_host_build_of_the_same_statements_bit_for_bit():
    """Every float operation is rounded on its own: the statements of csrc/sh_math.h without exp (normalize, the DC colour, the colour of
    sh_levels 2..4) are then sums, products, quotients and square roots that IEEE 754 rounds one way only, and the kernels give the bits
    that gcc's build of the same header with -ffp-contract=off gives on the host.  One fused multiply-add in the kernel, or an approximate
    square root or quotient, would show here.  (sigmoid and exp go through each side's own expf and are not compared.)"""
    L = gc.hostlib()
    n = 1021
    rest = torch.rand(n, 15, 3, generator=torch.Generator().manual_seed(9)) * 2 - 1
    quats = torch.randn(n, 4, generator=torch.Generator().manual_seed(10))
    quats[0] = 0.0
    quats[1] = torch.tensor([0.6e-20, 0.0, -0.8e-20, 0.0])
    for levels in (1, 2, 3, 4):
        bg = _background(n, seed=levels, sh_levels=levels, sh_features_rest=rest, quaternions=quats)
        block = bg.activated()
        _, host_q, host_dc = gc.host_activations(L, bg._opacities, bg._quaternions, bg._sh_features_dc)
        assert torch.equal(block["quaternions"].cpu(), host_q)
        assert torch.equal(block["colors"].cpu(), host_dc)
        for cam in (torch.tensor([0.3, -2.0, 0.8]), bg._positions[17].cpu() + torch.tensor([6e-4, -8e-4, 0.0])):
            got = bg.gaussians(cam.to(DEV)[None]).colors.cpu()
            want = gc.host_colors(L, levels, bg._positions, bg._sh_features_dc, bg._sh_features_rest, cam)
            differ = int((got != want).sum())
            print("L=%d: %d of %d colour values differ from the host build" % (levels, differ, got.numel()))
            assert torch.equal(got, want), (levels, differ)


# ---- Scene -----------------------------------------------------------------------------------------------------------------------------
def _scene(n_avatars=1, sh_levels=1, **render):
    from dreamwaltz_g_amd import camera, configs, scene as sc, sds_step
    cfg = configs.TrainConfig(); cfg.device = str(DEV); cfg.render.bg_color = (0.5, 0.5, 0.5)
    for k, v in render.items():
        setattr(cfg.render, k, v)
    avatars = [sds_step.build_synthetic_avatar(2000, DEV, seed=s)[0] for s in range(n_avatars)]
    bg = _background(1500, seed=4, sh_levels=sh_levels)
    scene = sc.Scene(cfg, avatars[0] if n_avatars == 1 else avatars, background=bg, async_pair_count=True).to(DEV).eval()
    return scene, _camera(20.0), bg


def _camera(azimuth):
    from dreamwaltz_g_amd import camera
    return camera.make_camera(radius=2.4, azimuth=azimuth, elevation=80.0, fovy=55.0, height=96, width=96, device=DEV)


def _pose(seed, n_avatars=1):
    from dreamwaltz_g_amd import synth
    ps = [synth.random_smpl_inputs(seed=seed + 100 * i, device=DEV) for i in range(n_avatars)]
    return ps[0] if n_avatars == 1 else {k: torch.cat([p[k] for p in ps], dim=0) for k in ps[0]}


def _keep(o):
    return {k: o[k].clone() for k in ("image", "image_fg", "depth", "alpha")}


@pytest.mark.parametrize("case", ["plain", "white", "zero_scales", "two_avatars_transl", "sh3"])
def test_scene_forward_renders_the_hand_merged_gaussians(case):
    from dreamwaltz_g_amd.avatar import merge_gaussians
    A = 2 if case == "two_avatars_transl" else 1
    scene, data, bg = _scene(n_avatars=A, sh_levels=3 if case == "sh3" else 1, use_zero_scales=case == "zero_scales",
                             avatar_transl="[[-0.4, 0.0, 0.0], [0.4, 0.0, 0.1]]" if A == 2 else None)
    bg_mode = "white" if case == "white" else None
    pose = _pose(5, A)
    with torch.inference_mode():
        o = _keep(scene.forward(data, smpl_observed_inputs=pose, use_densifier=False, bg_mode=bg_mode))
        again = _keep(scene.forward(data, smpl_observed_inputs=pose, use_densifier=False, bg_mode=bg_mode))
        merged = merge_gaussians(*scene._avatar_parts(pose), bg.gaussians(data['c2w'][:, :3, 3]))
        assert merged.positions.shape[0] == 2000 * A + 1500
        if case == "zero_scales":
            merged.scales = merged.scales * 0.1
        hand = scene.renderer.render(data=data, gaussians=merged, return_2d_radii=False)
        for k in ("depth", "alpha"):
            assert torch.equal(o[k], hand[k]), k                     # depth and alpha include the scene
        assert torch.equal(o["image_fg"], hand["image"])
        if bg_mode == "white":
            assert torch.equal(o["image"], hand["image"] + torch.ones_like(hand["image"]) * (1 - hand["alpha"]))
        else:
            assert torch.equal(o["image"], hand["image"])
        scene.background = None                                       # the scene's Gaussians are in the picture
        plain = scene.forward(data, smpl_observed_inputs=pose, use_densifier=False, bg_mode=bg_mode)
        assert float((plain["alpha"] - o["alpha"]).abs().max()) > 0.1
    for k in o:
        assert torch.equal(o[k], again[k]), k                         # two runs are bit-identical


@pytest.mark.parametrize("sh_levels", [1, 3])
def test_forward_frames_equals_forward_per_frame_and_activates_once(sh_levels):
    scene, data, bg = _scene(sh_levels=sh_levels)
    poses = [_pose(20 + i) for i in range(3)]
    cams = [_camera(a) for a in (20.0, 75.0, 140.0)]
    with torch.inference_mode():
        single = [_keep(scene.forward(data, smpl_observed_inputs=p, use_densifier=False)) for p in poses]
        assert bg.activation_launches == 1                            # once over three frames
        own = [_keep(scene.forward(c, smpl_observed_inputs=p, use_densifier=False)) for c, p in zip(cams, poses)]
        for frozen in (False, True):
            one = scene.forward_frames(data, poses, frozen_avatar=frozen)
            each = scene.forward_frames(cams, poses, frozen_avatar=frozen)
            assert one["image"].shape == (3, 96, 96, 3)
            for f in range(3):
                for k in ("image", "image_fg", "depth", "alpha"):
                    assert torch.equal(one[k][f:f + 1], single[f][k]), (f, k)
                    assert torch.equal(each[k][f:f + 1], own[f][k]), (f, k)
        white = scene.forward_frames(data, poses, bg_mode="white")
        assert torch.equal(white["image"][1:2], single[1]["image_fg"] + torch.ones_like(single[1]["image"]) * (1 - single[1]["alpha"]))
        assert bg.activation_launches == 1
        # an in-place edit of a parameter, then a checkpoint load: the block is recomputed each time, and only then
        with torch.inference_mode(False), torch.no_grad():
            bg._opacities.sub_(1.5)
        edited = _keep(scene.forward(data, smpl_observed_inputs=poses[0], use_densifier=False))
        assert bg.activation_launches == 2 and not torch.equal(edited["image"], single[0]["image"])
        scene.forward(data, smpl_observed_inputs=poses[1], use_densifier=False)
        assert bg.activation_launches == 2
    sd = {k: v.clone() for k, v in scene.state_dict().items()}
    sd["background._opacities"] = sd["background._opacities"] + 1.5
    scene.load_state_dict(sd)
    with torch.inference_mode():
        back = _keep(scene.forward(data, smpl_observed_inputs=poses[0], use_densifier=False))
        assert bg.activation_launches == 3
        bg.invalidate_caches()
        scene.forward(data, smpl_observed_inputs=poses[0], use_densifier=False)
        assert bg.activation_launches == 4
    assert float((back["image"] - single[0]["image"]).abs().max()) < 1e-4          # (x - 1.5) + 1.5: the original picture, to rounding


@pytest.mark.parametrize("override", ["zero_scales", "constants", "fixed_n"])
def test_forward_frames_applies_the_debug_overrides_to_the_merged_set_as_forward_does(override):
    """scene.py:134-145 on avatars + scene: the stacked buffers are overridden in place, and a frame equals forward()'s bit for bit.
    use_fixed_n_gaussians draws one random subset per frame from torch's generator: the same seed before both runs, the same subsets."""
    render = {"zero_scales": dict(use_zero_scales=True), "constants": dict(use_constant_colors=(0.2, 0.7, 0.4), use_constant_opacities=0.3),
              "fixed_n": dict(use_fixed_n_gaussians=1700)}[override]
    scene, data, bg = _scene(**render)
    poses = [_pose(50 + i) for i in range(2)]
    with torch.inference_mode():
        torch.manual_seed(11)
        single = [_keep(scene.forward(data, smpl_observed_inputs=p, use_densifier=False)) for p in poses]
        torch.manual_seed(11)
        frames = scene.forward_frames(data, poses)
        for f in range(2):
            for k in ("image", "image_fg", "depth", "alpha"):
                assert torch.equal(frames[k][f:f + 1], single[f][k]), (f, k)
        # the override reached the scene's rows too: without it the picture is another one
        for k in render:
            setattr(scene, k, False)
        torch.manual_seed(11)
        plain = scene.forward(data, smpl_observed_inputs=poses[0], use_densifier=False)
        assert not torch.equal(plain["image"], single[0]["image"])
    assert bg.activation_launches == 1


def test_a_stale_block_is_refreshed_in_place_so_a_captured_graph_never_reads_freed_memory():
    """The activated block keeps its addresses over a parameter change (a graph captured earlier has them baked in): the next
    activated() recomputes into the same tensors."""
    bg = _background(257, seed=6)
    before = bg.activated()
    ptrs = {k: t.data_ptr() for k, t in before.items()}
    old = before["opacities"].clone()
    with torch.no_grad():
        bg._opacities.sub_(1.5)
    after = bg.activated()
    assert {k: t.data_ptr() for k, t in after.items()} == ptrs and bg.activation_launches == 2
    assert not torch.equal(after["opacities"], old)
    bg.invalidate_caches()
    assert {k: t.data_ptr() for k, t in bg.activated().items()} == ptrs and bg.activation_launches == 3


def test_graphed_replay_with_a_changed_pose_equals_the_eager_frame():
    from dreamwaltz_g_amd import player
    scene, data, bg = _scene()
    poses = [_pose(30 + i) for i in range(3)]
    with torch.inference_mode():
        eager = [_keep(scene.forward(data, smpl_observed_inputs=p, use_densifier=False)) for p in poses]
    pl = player.GraphedAnimation(scene, data, poses[0], warmup_poses=poses[:2])
    assert pl.frame_index is None                                     # the frame-index input belongs to video backgrounds
    torch.cuda.synchronize()
    for f in (2, 0, 1):
        o = _keep(pl.replay(poses[f]))
        assert pl.check()
        for k in ("image", "depth", "alpha"):
            assert torch.equal(o[k], eager[f][k]), (f, k)
    assert bg.activation_launches == 1
    pl.close()


def test_the_merge_never_syncs_the_host():
    from dreamwaltz_g_amd.background import scene_merge
    for levels in (1, 3):
        bg = _background(1021, seed=2, sh_levels=levels)
        parts = _parts(2, 257, seed=2)
        c2w = torch.eye(4, device=DEV)[None].clone()
        scene_merge(parts, bg, c2w[:, :3, 3])                          # fills the cache
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for _ in range(2):
                scene_merge(parts, bg, c2w[:, :3, 3])
        finally:
            torch.cuda.set_sync_debug_mode(0)
    # forward_frames: whatever the rasterizer chain does, the Gaussian scene adds no synchronisation
    scene, data, _ = _scene(sh_levels=3)
    poses = [_pose(40 + i) for i in range(2)]
    with torch.inference_mode():
        scene.forward_frames(data, poses)
        torch.cuda.synchronize()
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                scene.forward_frames(data, poses)
            finally:
                torch.cuda.set_sync_debug_mode(0)
    mine = [str(r.filename) + ":" + str(r.lineno) for r in rec if r.filename.endswith(("background.py", "scene.py"))]
    assert not mine, mine
