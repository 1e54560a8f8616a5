"""-m gpu parity of the several-people condition image (dreamwaltz_g_amd/condition.py over csrc/condition.hip's *_people kernels) against
tests/condition_people_cases.py (built on oracle/condition.py; pinned on the reference's captured rows by tests/test_condition_people_host.py),
and of the several-avatar playback (Scene.forward_frames) against frame-by-frame Scene.forward.

Bars, those of tests/test_condition_gpu.py: rows -- validity and the person hit identical, x / W, y / H and the distance within 1e-9 (fp64 on
both sides, fp32-representable inputs; on this fixture no validity decision is nearer than 2.8e-5 to its threshold and two people along
a ray are 0.34 apart, asserted in the host file); image from GIVEN rows -- bit-exact uint8; end to end -- 99.9 % of the pixels; one person
through the people entry points -- the bits of the one-person entry points; depth over the concatenated mesh -- the bits of the minimum
of the per-person maps; playback -- the bits of frame-by-frame `forward`."""
import types

import numpy as np
import pytest
import torch

import dwg_import  # noqa: F401
from tests import condition_people_cases as pc

pytestmark = pytest.mark.gpu


def _cfg(**kw):
    from dreamwaltz_g_amd import configs
    c = configs.PromptConfig()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _cuda(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


@pytest.mark.parametrize("ignore", [True, False])
@pytest.mark.parametrize("name", pc.CAMERAS)
def test_keypoint_rows_and_the_person_hit_match_the_oracle(name, ignore):
    from dreamwaltz_g_amd import condition as cd
    kp, v, t, E, K, W, H = pc.people_inputs(name)
    ref, ref_hit, det = pc.reference(name, ignore)
    hidden_by_another, body_by_another, body_by_own = pc.hidden_counts(name)
    assert (hidden_by_another, body_by_another, body_by_own) == pc.HIDDEN[name] and hidden_by_another > 0      # the input condition: cross-person culls exist
    if name == "front":                                                      # body keypoints behind ANOTHER person: the one-person shortcut keeps them
        assert body_by_another > 0
    c = cd.SMPL2Condition(_cfg(ignore_body_self_occlusion=ignore))
    tkp, tv, tE, tK = _cuda(kp, v, E, K)
    scene = cd.build_people_scene(tv, t)
    rows, hit = c.people_rows(tkp, scene, tE, tK, return_hit_person=True)
    assert rows.shape == (3, 128, 4) and rows.dtype == torch.float64 and hit.shape == (3, 128) and hit.dtype == torch.int32
    rows, hit = rows.cpu().numpy(), hit.cpu().numpy()
    valid = rows[..., 3] > 0.5
    ref_valid = ~np.isnan(ref[..., 0])
    print(name, ignore, "valid", int(valid.sum()), "oracle", int(ref_valid.sum()), "validity differs", int((valid != ref_valid).sum()),
          "hit differs", int((hit != ref_hit).sum()), "max |xy|", float(np.abs(rows[valid & ref_valid, :2] - ref[valid & ref_valid, :2]).max()),
          "max |dist|", float(np.abs(rows[..., 2] - det["t_far"]).max()))
    assert np.array_equal(valid, ref_valid)
    assert np.array_equal(hit, ref_hit)
    assert np.abs(rows[valid, :2] - ref[valid, :2]).max() < 1e-9
    assert np.abs(rows[..., 2] - det["t_far"]).max() < 1e-9
    assert np.all(rows[~valid, :2] == 0.0)
    # pose_rows takes the same inputs to the same place, and two calls give the same bits
    again = c.pose_rows(tkp, scene, tE, tK)
    assert torch.equal(again.cpu(), torch.from_numpy(rows))


FLAG_SETS = [("front", {}), ("side", dict(draw_face_landmarks=True)), ("wide", dict(openpose_left_right_flip=True, draw_face_landmarks=True)),
             ("front", dict(draw_body_keypoints=False, draw_face_landmarks=True)), ("wide", dict(draw_hand_keypoints=False))]


@pytest.mark.parametrize("name,flags", FLAG_SETS)
def test_image_from_the_oracle_rows_is_bit_exact(name, flags):
    from dreamwaltz_g_amd import condition as cd
    ref_rows, _, _ = pc.reference(name, True)
    _, _, _, _, _, W, H = pc.people_inputs(name)
    cfg = _cfg(**flags)
    kw = dict(draw_body=cfg.draw_body_keypoints, draw_hand=cfg.draw_hand_keypoints, draw_face=cfg.draw_face_landmarks,
              flip_LR=cfg.openpose_left_right_flip)
    ref = pc.draw_poses_people(ref_rows, H, W, **kw)
    assert int((ref != pc.draw_poses_people(ref_rows[::-1], H, W, **kw)).any(2).sum()) > 0           # the input condition: the order of the people matters
    assert (ref.sum(2) > 0).mean() > 0.01
    u8, chw = cd.SMPL2Condition(cfg).draw(_cuda(pc.kernel_rows(ref_rows))[0], H, W, out_u8=True, out_chw=True)
    assert u8.shape == (H, W, 3) and u8.dtype == torch.uint8 and chw.shape == (1, 3, H, W)
    print(name, flags, "pixels that differ", int((u8.cpu().numpy() != ref).any(2).sum()))
    assert np.array_equal(u8.cpu().numpy(), ref)
    assert (chw[0] - u8.permute(2, 0, 1).float() / 255.0).abs().max() < 1e-7


@pytest.mark.parametrize("name,ignore", [("front", False), ("side", True), ("wide", False)])
def test_one_person_through_the_people_entry_points_is_the_one_person_path(name, ignore):
    from dreamwaltz_g_amd import condition as cd
    kp, v, t, E, K, W, H = pc.people_inputs(name)
    c = cd.SMPL2Condition(_cfg(ignore_body_self_occlusion=ignore, draw_face_landmarks=True))
    tkp, tv, tE, tK = _cuda(kp[1], v[1], E, K)                               # the translated second person: nothing special about it
    one = c.pose_rows(tkp, cd.build_ray_casting_scene(tv, t), tE, tK)
    people, hit = c.people_rows(tkp[None], cd.build_people_scene(tv[None], t), tE, tK, return_hit_person=True)
    assert one.shape == (128, 4) and people.shape == (1, 128, 4)
    assert 0 < int((one[:, 3] > 0.5).sum()) < 128
    assert torch.equal(people[0], one)
    assert set(hit.unique().tolist()) <= {-1, 0}
    u8_one, chw_one = c.draw(one, H, W, out_u8=True, out_chw=True)
    u8_people, chw_people = c.draw(people, H, W, out_u8=True, out_chw=True)
    assert torch.equal(u8_people, u8_one) and torch.equal(chw_people, chw_one)


def test_call_with_three_people_end_to_end():
    from dreamwaltz_g_amd import condition as cd
    kp, v, t, E, K, W, H = pc.people_inputs("wide")
    ref_rows, _, _ = pc.reference("wide", True)
    ref = pc.draw_poses_people(ref_rows, H, W, draw_face=False)
    c = cd.SMPL2Condition(_cfg())                                            # shipped defaults: no face, body self occlusion ignored
    K_raw = pc.G["cond.wide.intrinsics_raw"].astype(np.float32)
    tkp, tv, tE, tK, tK_raw = _cuda(kp, v, E, K, K_raw)
    cam = dict(extrinsic=tE[None], intrinsics=tK_raw[None])
    out = c(types.SimpleNamespace(vertices=tv, joints=tkp), t, cam, "pose", H, W)
    img = out.u8.cpu().numpy()
    print("wide end to end: equal pixels", float((img == ref).all(2).mean()))
    assert (img == ref).all(2).mean() >= 0.999
    assert out.to_pil().size == (W, H) and out.to_chw().shape == (1, 3, H, W)
    scene = cd.build_people_scene(tv, t)
    chw = c.export_pose_chw(tkp, scene, extrinsic=tE, intrinsics=tK, width=W, height=H)
    assert (chw - out.to_chw()).abs().max() < 1e-7
    assert torch.equal(c.export_pose(tkp, scene, extrinsic=tE, intrinsics=tK, width=W, height=H).u8, out.u8)
    assert torch.equal(c(types.SimpleNamespace(vertices=tv, joints=tkp), t, cam, "openpose", H, W).u8, out.u8)
    # refusals with real objects: a P mismatch, one mesh for three people, more than 16 people -- before any launch
    with pytest.raises(ValueError):
        c.pose_rows(tkp, cd.build_people_scene(tv[:2], t), tE, tK)
    with pytest.raises(ValueError):
        c.pose_rows(tkp, cd.build_ray_casting_scene(tv[0], t), tE, tK)
    with pytest.raises(ValueError):
        cd.build_people_scene(tv[:1].expand(17, -1, -1), t)
    with pytest.raises(NotImplementedError):
        cd.build_ray_casting_scene(tv, t)
    with pytest.raises(NotImplementedError):
        c(types.SimpleNamespace(vertices=tv, joints=tkp), t, cam, "depth", H, W)
    # without culling no mesh is needed: every keypoint in front of the camera is drawn, the distance column says "not taken"
    nc = cd.SMPL2Condition(_cfg(use_occlusion_culling=False))
    rows = nc.pose_rows(tkp, None, tE, tK).cpu().numpy()
    ref_nc, _, _ = pc.pose_keypoints_people(kp, v, t, E, K, W, H, use_occlusion_culling=False)
    valid = rows[..., 3] > 0.5
    assert rows.shape == (3, 128, 4) and np.array_equal(valid, ~np.isnan(ref_nc[..., 0])) and valid.sum() > 3 * 120
    assert np.abs(rows[valid, :2] - ref_nc[valid, :2]).max() < 1e-9 and np.all(rows[..., 2] == -1.0)


def test_depth_over_all_people_is_the_nearest_of_the_per_person_maps():
    from dreamwaltz_g_amd import condition as cd
    kp, v, t, E, K, W, H = pc.people_inputs("front")
    c = cd.SMPL2Condition(_cfg())
    tv, tE = _cuda(v, E)
    tK = cd.adjust_intrinsics_size(_cuda(K)[0], width=64, height=64)
    cam = dict(extrinsic=tE, intrinsics=tK, width=64, height=64)
    scene = cd.build_people_scene(tv, t)
    assert scene.merged.vertices.shape == (3 * v.shape[1], 3) and scene.merged.triangles.shape == (3 * t.shape[0], 3)
    assert int(scene.merged.triangles.max()) == 3 * v.shape[1] - 1 and scene.merged is scene.merged
    all_t = c.export_depth(scene, raw=True, **cam).t
    all_n = c.export_normal_raw(scene, **cam)
    best_t = torch.full((64, 64), float("inf"), device="cuda")
    best_n = torch.zeros(64, 64, 3, device="cuda")
    seen = 0
    for p in range(3):                                                       # ascending, strict <: the lower person on equal t, as the triangle order has it
        one = cd.build_ray_casting_scene(tv[p], t)
        tp, n_p = c.export_depth(one, raw=True, **cam).t, c.export_normal_raw(one, **cam)
        nearer = tp < best_t
        seen += int(bool(nearer.any()))
        best_t = torch.where(nearer, tp, best_t)
        best_n = torch.where(nearer[..., None], n_p, best_n)
    assert seen >= 2 and 0 < int(torch.isfinite(best_t).sum()) < 64 * 64     # more than one person is the nearest somewhere
    assert torch.equal(all_t, best_t)
    assert torch.equal(all_n, best_n)
    out = c(types.SimpleNamespace(vertices=tv, joints=None), t, dict(extrinsic=tE[None], intrinsics=tK[None]), "depth_raw", 64, 64)
    assert isinstance(out, cd.DepthMap) and torch.equal(out.t, best_t)


# ---- playback of several avatars -------------------------------------------------------------------------------------------------------
def _two_avatar_scene(dev, res=128, n=3000):
    from dreamwaltz_g_amd import camera, configs, scene as sc, sds_step
    cfg = configs.TrainConfig(); cfg.device = str(dev); cfg.render.bg_color = (0.5, 0.5, 0.5)
    cfg.render.avatar_transl = "[[-0.4, 0.0, 0.0], [0.4, 0.0, 0.1]]"
    avatars = [sds_step.build_synthetic_avatar(n, dev, seed=s)[0] for s in (0, 1)]
    scene = sc.Scene(cfg, avatars, async_pair_count=True).to(dev).eval()
    data = camera.make_camera(radius=2.4, azimuth=20.0, elevation=80.0, fovy=55.0, height=res, width=res, device=dev)
    return scene, data


def _pose_pair(seed, dev):
    from dreamwaltz_g_amd import synth
    a, b = synth.random_smpl_inputs(seed=seed, device=dev), synth.random_smpl_inputs(seed=100 + seed, device=dev)
    return {k: torch.cat([a[k], b[k]], dim=0) for k in a}


@pytest.mark.parametrize("bg_mode", [None, "white"])
def test_two_avatar_playback_equals_frame_by_frame_forward(bg_mode):
    dev = torch.device("cuda:0")
    scene, data = _two_avatar_scene(dev)
    poses = [_pose_pair(40 + i, dev) for i in range(3)]
    with torch.inference_mode():
        single = [scene.forward(data, smpl_observed_inputs=p, use_densifier=False, bg_mode=bg_mode) for p in poses]
        single = [{k: o[k].clone() for k in ("image", "alpha", "depth")} for o in single]
        assert float(single[0]["alpha"].mean()) > 0.01 and not torch.equal(single[0]["image"], single[1]["image"])
        for frozen in (False, True, True):                                   # the second frozen pass plays from the kept canonical part
            batch = scene.forward_frames(data, poses, bg_mode=bg_mode, frozen_avatar=frozen)
            assert batch["image"].shape == (3, 128, 128, 3)
            for f in range(3):
                for k in ("image", "alpha", "depth"):
                    assert torch.equal(batch[k][f:f + 1], single[f][k]), (frozen, f, k)
            assert all(a.frozen_playback is False for a in scene.avatars)


def test_forward_with_two_avatars_renders_the_hand_merged_gaussians():
    from dreamwaltz_g_amd.avatar import merge_gaussians
    dev = torch.device("cuda:0")
    scene, data = _two_avatar_scene(dev)
    pose = _pose_pair(7, dev)
    with torch.inference_mode():
        out = scene.forward(data, smpl_observed_inputs=pose, use_densifier=False, bg_mode=None)
        out = {k: out[k].clone() for k in ("image", "alpha", "depth")}
        parts = []
        for i, avatar in enumerate(scene.avatars):
            g = avatar.animate(smpl_observed_inputs={k: v[i:i + 1] for k, v in pose.items()})
            g.positions = g.positions + scene.avatar_transl[i][None]
            parts.append(g)
        n = [int(g.positions.shape[0]) for g in parts]
        merged = merge_gaussians(*parts)
        assert merged.positions.shape[0] == sum(n) and torch.equal(merged.positions[n[0]:], parts[1].positions)
        by_hand = scene.renderer.render(data=data, gaussians=merged, return_2d_radii=False)
        for k in ("image", "alpha", "depth"):
            assert torch.equal(by_hand[k], out[k]), k
        # each avatar is on the canvas: either alone covers less than both
        alone = [float(scene.renderer.render(data=data, gaussians=g, return_2d_radii=False)["alpha"].sum()) for g in parts]
        assert 0 < max(alone) < float(out["alpha"].sum())
