"""CPU checks of the several-people condition image (include/dwg_condition.h *_people, dreamwaltz_g_amd.condition): argument errors
reported before any launch, the workspace size, the Python layer's refusals, and the people oracle (tests/condition_people_cases.py) with
ONE person against oracle/condition.py on the reference's four captured cases -- which pins the new oracle where the old one is pinned."""
import ctypes

import numpy as np
import pytest
import torch

import dreamwaltz_g_amd._lib as _lib
from oracle import condition as oc
from tests import condition_people_cases as pc

FAKE = ctypes.c_void_p(4096)          # never dereferenced: every call below must fail before a launch
E_ARG = -1
GOLDEN_CASES = ["front", "side", "wide", "side_ignore_body"]


def test_keypoints_people_bad_arguments_return_arg_error_before_any_launch():
    L = _lib.lib()
    #       P  K    kps   ext   intr  V   verts F    tris  groups thresholds     ign cull rows  hit   stream
    base = [3, 128, FAKE, FAKE, FAKE, 50, FAKE, 100, FAKE, FAKE, 0.2, 0.2, 0.02, 1, 1, FAKE, FAKE, None]
    for k, bad in ((0, 0), (0, -1), (0, 17), (1, 0), (1, -4), (2, None), (3, None), (4, None), (15, None),
                   (5, 0), (7, 0), (6, None), (8, None), (9, None)):            # the last five: culling without a mesh
        args = list(base)
        args[k] = bad
        assert L.dwg_condition_keypoints_people(*args) == E_ARG, (k, bad)
    args = list(base)
    args[0] = 17                                                             # P is looked at first: also without culling, also with nothing else
    args[14] = 0
    assert L.dwg_condition_keypoints_people(*args) == E_ARG
    assert L.dwg_condition_keypoints_people(17, 0, None, None, None, 0, None, 0, None, None, 0.0, 0.0, 0.0, 0, 0, None, None, None) == E_ARG


def test_draw_people_bad_arguments_return_arg_error_before_any_launch():
    L = _lib.lib()
    #       P  H    W    rows  flags u8    chw   ws    stream
    base = [2, 512, 512, FAKE, 7, FAKE, FAKE, FAKE, None]
    for k, bad in ((0, 0), (0, -3), (0, 17), (1, 0), (2, 0), (1, -1), (1, 16385), (2, 16385), (3, None), (7, None)):
        args = list(base)
        args[k] = bad
        assert L.dwg_condition_draw_people(*args) == E_ARG, (k, bad)
    args = list(base)
    args[5] = args[6] = None                                                 # no output asked for
    assert L.dwg_condition_draw_people(*args) == E_ARG
    # the single-person draw's size limits: the same sizes are refused by both
    for H, W in ((16384, 16384), (9000, 9000)):
        one = L.dwg_condition_draw(H, W, FAKE, 7, FAKE, None, FAKE, None)
        if one == E_ARG:
            assert L.dwg_condition_draw_people(1, H, W, FAKE, 7, FAKE, None, FAKE, None) == E_ARG, (H, W)


def test_workspace_grows_with_the_people_and_is_zero_for_bad_sizes():
    L = _lib.lib()
    f, one = L.dwg_condition_people_workspace_bytes, L.dwg_condition_workspace_bytes
    assert f(1, 512, 512) == one(512, 512) > 0
    sizes = [f(P, 512, 512) for P in range(1, 17)]
    assert all(b > a for a, b in zip(sizes, sizes[1:])) and sizes[-1] == 16 * one(512, 512)
    assert f(3, 256, 384) == 3 * one(256, 384)
    assert f(0, 512, 512) == 0 and f(-1, 512, 512) == 0 and f(17, 512, 512) == 0
    assert f(2, 0, 512) == 0 and f(2, -8, 512) == 0


def _cond():
    from dreamwaltz_g_amd import condition as cd, configs
    return cd, cd.SMPL2Condition(configs.PromptConfig())


def test_python_layer_refuses_cpu_tensors_mismatched_people_and_too_many():
    cd, cond = _cond()
    kp, v, t, E, K, W, H = pc.people_inputs("front")
    kp, v, E, K = (torch.from_numpy(a) for a in (kp, v, E, K))
    with pytest.raises(RuntimeError):
        cd.build_people_scene(v, t)                                          # a CPU tensor
    with pytest.raises(RuntimeError):
        cond.pose_rows(kp, None, E, K)
    with pytest.raises(RuntimeError):
        cd.SMPL2Condition(_no_culling()).people_rows(kp, None, E, K)         # shapes in order, no mesh needed: the device is what is wrong
    with pytest.raises(RuntimeError):
        cond.draw(torch.zeros(3, 128, 4, dtype=torch.float64), H, W)
    with pytest.raises(ValueError):
        cd.build_people_scene(torch.zeros(17, 5, 3), t)                      # P > 16, before any device use
    with pytest.raises(ValueError):
        cd.build_people_scene(torch.zeros(5, 3), t)
    with pytest.raises(ValueError):
        cond.draw(torch.zeros(17, 128, 4, dtype=torch.float64), H, W)
    with pytest.raises(ValueError):
        cd.SMPL2Condition(_no_culling()).people_rows(torch.zeros(17, 128, 3), None, E, K)
    # a P mismatch is a matter of shapes: refused before the device is looked at.  (A PeopleScene cannot be BUILT without a GPU, so this
    # one is put together by hand; tests/test_condition_people_gpu.py repeats the refusal with a built one.)
    two = cd.PeopleScene.__new__(cd.PeopleScene)
    two.vertices, two.triangles, two._merged = v[:2], torch.from_numpy(t), None
    with pytest.raises(ValueError):
        cond.people_rows(kp, two, E, K)
    with pytest.raises(ValueError):
        cond.people_rows(kp, None, E, K)                                     # culling (the default) without the meshes
    with pytest.raises(NotImplementedError):
        cd.build_ray_casting_scene(torch.zeros(2, 5, 3), t)                  # stays the one-mesh seam
    for kind in ("depth", "normal", "mesh"):
        with pytest.raises(NotImplementedError):
            cond(None, None, None, kind, 64, 64)


def _no_culling():
    from dreamwaltz_g_amd import configs
    c = configs.PromptConfig()
    c.use_occlusion_culling = False
    return c


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_people_oracle_with_one_person_is_the_one_person_oracle(name):
    """P = 1: the same rows (NaN pattern included) and the same image as oc.pose_keypoints / oc.draw_poses on the golden inputs, and through
    them the reference's captured rows."""
    p = "cond.%s." % name
    G = pc.G
    W, H = [int(v) for v in G[p + "size"]]
    ignore = name.endswith("ignore_body")
    args = (G["cond.vertices"], G["cond.triangles"], G[p + "extrinsic"], G[p + "intrinsics"], W, H)
    ref = oc.pose_keypoints(G["cond.keypoints"], *args, ignore_body_self_occlusion=ignore)
    rows, hit, _ = pc.pose_keypoints_people(G["cond.keypoints"][None], G["cond.vertices"][None], *args[1:], ignore_body_self_occlusion=ignore)
    assert rows.shape == (1, 128, 3) and hit.shape == (1, 128)
    assert np.array_equal(rows[0], ref, equal_nan=True)
    assert set(np.unique(hit)) <= {-1, 0} and (hit == 0).any()
    g = G[p + "rows"]                                                        # captured from the reference
    assert np.array_equal(np.isnan(rows[0, :, 0]), np.isnan(g[:, 0]))
    ok = ~np.isnan(g[:, 0])
    assert np.abs(rows[0][ok] - g[ok]).max() < 1e-9
    for flags in ({}, dict(draw_face=False), dict(flip_LR=True, draw_body=True), dict(draw_hand=False)):
        assert np.array_equal(pc.draw_poses_people(rows, H, W, **flags), oc.draw_poses(ref, H, W, **flags))


def test_the_fixture_has_what_the_gpu_tests_rely_on():
    """Three people: keypoints hidden by ANOTHER person exist (body keypoints among them), no decision sits on a rounding, and the
    order the people are drawn in matters."""
    for name in pc.CAMERAS:
        assert pc.hidden_counts(name) == pc.HIDDEN[name]
        _, _, det = pc.reference(name, False)
        margin = np.abs(det["t_far"] - det["t_hit"] - det["thr"])
        assert margin[np.isfinite(margin)].min() >= 2.8e-5
        per = np.sort(det["per_person"], axis=0)
        both = np.isfinite(per[1])
        assert (per[1][both] - per[0][both]).min() >= 0.34
    for name in ("front", "wide"):
        rows, _, _ = pc.reference(name, True)
        _, _, _, _, _, W, H = pc.people_inputs(name)
        assert int((pc.draw_poses_people(rows, H, W) != pc.draw_poses_people(rows[::-1], H, W)).any(2).sum()) >= 700
