"""Gaussian scene background (boundary B24, dreamwaltz_g_amd.background), host side: the .ply reader against the generating arrays in the
reference's layouts (core/gaussian/gaussian_model.py:97-147), GaussianBackground's checkpoint keys and Scene's round trip of them, the
refusals of the training paths, the C-ABI's argument checks, and the bound build_scene with `--render.use_gs_background`."""
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
from tests import gs_background_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 7
KEYS = ("positions", "sh_features_dc", "sh_features_rest", "opacities", "scales", "quaternions")
SHAPES = {"positions": (N, 3), "sh_features_dc": (N, 1, 3), "sh_features_rest": (N, 15, 3), "opacities": (N, 1), "scales": (N, 3),
          "quaternions": (N, 4)}


def _cfg():
    from dreamwaltz_g_amd import configs
    cfg = configs.TrainConfig()
    cfg.device = "cpu"
    return cfg


def _check(path, cols):
    from dreamwaltz_g_amd.background import load_gaussian_ply
    got, want = load_gaussian_ply(str(path)), gc.expected_tensors(cols)
    assert sorted(got) == sorted(KEYS)
    for k in KEYS:
        assert got[k].dtype == torch.float32 and tuple(got[k].shape) == SHAPES[k] and got[k].is_contiguous(), k
        assert np.array_equal(got[k].numpy(), want[k]), k
    return got


@pytest.mark.parametrize("fmt", ["binary_little_endian", "binary_big_endian", "ascii"])
@pytest.mark.parametrize("shuffled", [False, True])
def test_reader_returns_the_generating_arrays_in_the_references_layouts(tmp_path, fmt, shuffled):
    cols = gc.make_columns(N, seed=3)
    order = list(gc.STANDARD_ORDER)
    if shuffled:
        np.random.RandomState(5).shuffle(order)
    got = _check(gc.write_ply(tmp_path / "scene.ply", cols, fmt=fmt, order=order), cols)
    # the (N, 3, 15) -> [N, 15, 3] transpose: coefficient k of channel c is f_rest_{15 c + k}
    assert got["sh_features_rest"][2, 4, 1] == float(cols["f_rest_19"][2]) and got["sh_features_dc"][5, 0, 2] == float(cols["f_dc_2"][5])


def test_reader_ignores_normals_extra_properties_and_later_elements(tmp_path):
    cols = gc.make_columns(N, seed=4)
    assert "nx" in cols                                                    # the 3DGS writer's nx ny nz are in the file
    extra = dict(cols, confidence=np.arange(N, dtype=np.float32))
    for fmt in ("binary_little_endian", "ascii"):
        _check(gc.write_ply(tmp_path / ("extra_%s.ply" % fmt), extra, fmt=fmt, trailing_element=True), cols)
    without = {k: v for k, v in cols.items() if k not in ("nx", "ny", "nz")}
    _check(gc.write_ply(tmp_path / "plain.ply", without), cols)


@pytest.mark.parametrize("fmt", ["binary_little_endian", "binary_big_endian", "ascii"])
def test_reader_accepts_double_columns(tmp_path, fmt):
    cols = gc.make_columns(N, seed=6)
    _check(gc.write_ply(tmp_path / "double.ply", cols, fmt=fmt, double=("x", "opacity", "f_rest_7", "rot_2")), cols)
    _check(gc.write_ply(tmp_path / "all_double.ply", cols, fmt=fmt, double=tuple(cols)), cols)


def test_reader_raises_value_error_naming_what_is_wrong(tmp_path):
    from dreamwaltz_g_amd.background import load_gaussian_ply
    cols = gc.make_columns(N, seed=7)
    for missing in ("x", "opacity", "f_dc_1"):
        p = gc.write_ply(tmp_path / "missing.ply", {k: v for k, v in cols.items() if k != missing})
        with pytest.raises(ValueError, match="`%s`" % missing):
            load_gaussian_ply(str(p))
    for drop, what in (("scale_2", "scale_0..2"), ("rot_3", "rot_0..3")):
        p = gc.write_ply(tmp_path / "short.ply", {k: v for k, v in cols.items() if k != drop})
        with pytest.raises(ValueError, match=what):
            load_gaussian_ply(str(p))
    p = gc.write_ply(tmp_path / "rest.ply", {k: v for k, v in cols.items() if k != "f_rest_44"})
    with pytest.raises(ValueError, match="44 `f_rest_\\*` properties, expected 45"):
        load_gaussian_ply(str(p))
    p = gc.write_ply(tmp_path / "degree0.ply", gc.make_columns(N, seed=8, n_rest=0))
    with pytest.raises(ValueError, match="f_rest"):
        load_gaussian_ply(str(p))
    assert tuple(load_gaussian_ply(str(p), max_sh_degree=0)["sh_features_rest"].shape) == (N, 0, 3)
    p = gc.write_ply(tmp_path / "list.ply", cols, list_property="neighbours")
    with pytest.raises(ValueError, match="list property `neighbours`"):
        load_gaussian_ply(str(p))
    raw = open(gc.write_ply(tmp_path / "cut.ply", cols), "rb").read()
    (tmp_path / "cut.ply").write_bytes(raw[:-5])
    with pytest.raises(ValueError, match="bytes of data"):
        load_gaussian_ply(str(tmp_path / "cut.ply"))
    (tmp_path / "not.ply").write_bytes(b"solid cube\n")
    with pytest.raises(ValueError, match="not a PLY"):
        load_gaussian_ply(str(tmp_path / "not.ply"))
    (tmp_path / "fmt.ply").write_bytes(raw.replace(b"binary_little_endian", b"binary_middle_endian"))
    with pytest.raises(ValueError, match="unknown PLY format"):
        load_gaussian_ply(str(tmp_path / "fmt.ply"))


class _Avatar(nn.Module):
    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(2))

    def invalidate_caches(self):
        pass

    def reset_by_state_dict(self, sd):
        pass


def test_background_has_the_references_parameter_names_and_scene_round_trips_them(tmp_path):
    from dreamwaltz_g_amd import optim, scene as sc
    from dreamwaltz_g_amd.background import GaussianBackground
    cols = gc.make_columns(N, seed=9)
    bg = GaussianBackground.from_ply(str(gc.write_ply(tmp_path / "s.ply", cols)))
    names = ["_positions", "_sh_features_dc", "_sh_features_rest", "_opacities", "_scales", "_quaternions"]
    assert sorted(bg.state_dict()) == sorted(names) and bg.n_points == N and bg.sh_levels == 1
    assert all(not p.requires_grad for p in bg.parameters())
    want = gc.expected_tensors(cols)
    for k in KEYS:
        assert np.array_equal(getattr(bg, "_" + k).numpy(), want[k]), k
    s = sc.Scene(_cfg(), [_Avatar()], background=bg)
    assert s.background is bg and s.gaussian_background is bg and s.mlp_background is None
    assert sorted(k for k in s.state_dict() if k.startswith("background.")) == sorted("background." + k for k in names)
    # a checkpoint of another scene with ANOTHER Gaussian count: resized like the reference's reset_by_state_dict, then copied
    other = GaussianBackground.from_tensors(**gc.scene_arrays(11, seed=2))
    sd = sc.Scene(_cfg(), [_Avatar()], background=other).state_dict()
    epoch, gen = optim.PARAM_EPOCH[0], bg._generation
    s.load_state_dict(sd)
    assert s.background.n_points == 11 and optim.PARAM_EPOCH[0] > epoch and bg._generation > gen
    for k in names:
        assert torch.equal(getattr(s.background, k), getattr(other, k)) and not getattr(s.background, k).requires_grad, k
    # from_tensors / from_reference: the same parameters; a [N] opacity column is the reference's [N, 1]
    arrays = gc.scene_arrays(5, seed=3)
    a = GaussianBackground.from_tensors(**dict(arrays, opacities=arrays["opacities"][:, 0]), sh_levels=3)
    assert tuple(a._opacities.shape) == (5, 1) and a.sh_levels == 3

    class Ref(nn.Module):                                         # a loaded reference GaussianModel: requires_grad parameters
        def __init__(self):
            super().__init__()
            for k, v in arrays.items():
                setattr(self, "_" + k, nn.Parameter(v.clone()))
    ref = Ref()
    b = GaussianBackground.from_reference(ref)
    assert b.reference[0] is ref and all(torch.equal(getattr(b, k), getattr(ref, k)) and not getattr(b, k).requires_grad for k in names)
    assert b._positions.data_ptr() == ref._positions.data_ptr()   # adopted, not copied
    with pytest.raises(ValueError, match="_scales"):
        ref._scales = None
        GaussianBackground.from_reference(ref)
    with pytest.raises(ValueError, match="sh_levels"):
        GaussianBackground.from_tensors(**arrays, sh_levels=5)
    with pytest.raises(ValueError, match="_sh_features_rest"):
        GaussianBackground.from_tensors(**dict(arrays, sh_features_rest=arrays["sh_features_rest"][:, :8]), sh_levels=2)
    with pytest.raises(ValueError, match="_quaternions"):
        GaussianBackground.from_tensors(**dict(arrays, quaternions=arrays["quaternions"][:, :3]))
    with pytest.raises(NotImplementedError, match="frozen"):
        b.get_optimizer()


def test_scene_accepts_only_the_class_itself_and_config_default_is_the_references():
    from dreamwaltz_g_amd import configs, scene as sc
    from dreamwaltz_g_amd.background import GaussianBackground
    assert configs.RenderConfig().use_gs_background is None

    class Sub(GaussianBackground):
        pass

    class GaussianModel(nn.Module):
        pass
    for other in (Sub(**gc.scene_arrays(3)), GaussianModel()):
        with pytest.raises(NotImplementedError):
            sc.Scene(_cfg(), [_Avatar()], background=other)
    assert sc.Scene(_cfg(), [_Avatar()]).gaussian_background is None


def test_training_paths_refuse_a_gaussian_background_by_name_before_any_launch():
    from dreamwaltz_g_amd import scene as sc, step_graph, trainer
    from dreamwaltz_g_amd.background import GaussianBackground
    bg = GaussianBackground.from_tensors(**gc.scene_arrays(4))
    s = sc.Scene(_cfg(), [_Avatar()], background=bg)
    with pytest.raises(NotImplementedError, match="forward_views with a GaussianBackground"):
        s.forward_views([{}], [None])
    cfg = _cfg()
    cfg.prompt.text_augmentation = False
    with pytest.raises(NotImplementedError, match="SDSTrainer with a GaussianBackground"):
        trainer.SDSTrainer(cfg, s, lambda **k: None, {}, use_controlnet=False)
    # a scene that got its Gaussian background after the trainer was built: every step refuses, nothing runs
    s.background = None
    tr = trainer.SDSTrainer(cfg, s, lambda **k: None, {}, use_controlnet=False)
    s.background = bg
    with pytest.raises(NotImplementedError, match="train_step with a GaussianBackground"):
        tr.train_step({'smpl_inputs': None})
    with pytest.raises(NotImplementedError, match="nerf2gs_step with a GaussianBackground"):
        tr.nerf2gs_step({'smpl_inputs': None}, None)
    with pytest.raises(NotImplementedError, match="GraphedTrainStep with a GaussianBackground"):
        step_graph.GraphedTrainStep(tr, {}, {})
    assert tr.train_step_index == 0
    # an avatar output without precomputed colours: refused by name
    from dreamwaltz_g_amd.avatar import GaussianOutput
    from dreamwaltz_g_amd.background import scene_merge
    g = GaussianOutput(positions=torch.zeros(2, 3), sh_features=torch.zeros(2, 16, 3), opacities=torch.zeros(2, 1), scales=torch.zeros(2, 3),
                       quaternions=torch.zeros(2, 4))
    with pytest.raises(NotImplementedError, match="colors"):
        scene_merge([g], bg)


def test_cabi_argument_errors_return_dwg_e_arg_before_any_launch():
    from dreamwaltz_g_amd import _lib
    from dreamwaltz_g_amd.background import ScenePartC
    L, E = _lib.lib(), _lib.CONSTANTS["DWG_E_ARG"]
    assert (_lib.CONSTANTS["DWG_SCENE_MAX_PARTS"], _lib.CONSTANTS["DWG_SCENE_SH_REST"]) == (17, 15)
    p, q, odd = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(4098)      # never dereferenced: every call fails its host checks

    def act(n=4, a=p, b=p, c=p, d=p, o1=q, o2=q, o3=q, o4=q):
        return L.dwg_scene_gaussians_activate(n, a, b, c, d, o1, o2, o3, o4, None)
    assert act(n=0) == 0 and act(n=0, a=None, o1=None) == 0                       # empty: OK without a launch
    assert act(n=-1) == E
    for k in ("a", "b", "c", "d", "o1", "o2", "o3", "o4"):
        assert act(**{k: None}) == E and act(**{k: odd}) == E, k
    assert act(o2=p) == E                                                          # an output aliasing an input

    def col(n=4, pos=p, dc=p, rest=p, levels=2, cam=p, stride=1, out=q):
        return L.dwg_scene_gaussians_colors(n, pos, dc, rest, levels, cam, stride, out, None)
    assert col(n=0) == 0 and col(n=-1) == E and col(levels=0) == E and col(levels=5) == E and col(stride=0) == E
    for k in ("pos", "dc", "rest", "cam", "out"):
        assert col(**{k: None}) == E and col(**{k: odd}) == E, k

    def parts(counts, colors=4096, positions=4096):
        arr = (ScenePartC * 17)()
        for i, n in enumerate(counts):
            arr[i].positions, arr[i].opacities, arr[i].colors, arr[i].scales, arr[i].quaternions, arr[i].count = positions, 4096, colors, 4096, 4096, n
        return arr

    def merge(n=2, arr=None, levels=1, dc=p, rest=p, cam=p, stride=4, cap=10, o=(q, q, q, q, q)):
        return L.dwg_scene_merge(n, parts([3, 5]) if arr is None else arr, levels, dc, rest, cam, stride, cap, *o, None)
    assert merge(n=0) == 0 and merge(arr=parts([0, 0])) == 0                       # no rows: OK without a launch
    assert merge(n=-1) == E and merge(n=18) == E and merge(levels=0) == E and merge(levels=5) == E and merge(cap=-1) == E
    assert merge(cap=7) == E                                                       # 8 rows do not fit
    assert merge(arr=parts([3, -1])) == E and merge(arr=parts([3, 5], colors=None)) == E
    assert merge(arr=parts([3, 5], positions=4098)) == E and merge(arr=parts([3, 5], colors=4098), levels=3) == E
    assert L.dwg_scene_merge(2, None, 1, p, p, p, 4, 10, q, q, q, q, q, None) == E
    for k in range(5):
        for bad in (None, odd):
            assert merge(o=tuple(bad if i == k else q for i in range(5))) == E, k
    for k in ("dc", "rest", "cam"):                                                # read at sh_levels > 1 only
        assert merge(levels=2, **{k: None}) == E and merge(levels=2, **{k: odd}) == E, k
    assert merge(levels=2, stride=0) == E


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="needs the reference checkout (build container only)")
def test_bound_build_scene_reads_the_ply_natively_only_when_opted_in(tmp_path):
    cols = gc.make_columns(N, seed=11)
    ply = str(gc.write_ply(tmp_path / "room.ply", cols, fmt="binary_big_endian"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gs_background_bind_check.py"), ply], capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("DWG_GS_BIND_CHECK ")][-1]
    d = json.loads(line[len("DWG_GS_BIND_CHECK "):])
    assert d["without_env_raises"] and d["env_other_value_raises"]
    assert d["scene_class"] == "dreamwaltz_g_amd.scene.Scene" and d["background_class"] == "dreamwaltz_g_amd.background.GaussianBackground"
    want = gc.expected_tensors(cols)
    for k in KEYS:
        assert np.array_equal(np.array(d["arrays"][k], dtype=np.float32).reshape(want[k].shape), want[k]), k
    assert d["frozen"] and d["reference_gaussian_model_built"] == 0
    assert d["video_wins"] == "dreamwaltz_g_amd.background.VideoBackground" and d["mlp_wins"] == "dreamwaltz_g_amd.background.MLPBackground"


def _np(t):
    return np.ascontiguousarray(t.detach().numpy(), dtype=np.float32)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_host_build_of_the_kernel_statements_follows_float64_like_torchs_fp32():
    """The statements of csrc/sh_math.h on the host against the float64 restatements, at the GPU test's rule: twice torch's own fp32 error
    (here torch on the CPU), at least 1, in units of the fp32 spacing at the result (colours: at max(|result|, 0.5))."""
    from dreamwaltz_g_amd import renderer
    L = gc.hostlib()
    n = 257
    a = gc.scene_arrays(n, seed=5)
    a["sh_features_rest"] = torch.rand(n, 15, 3, generator=torch.Generator().manual_seed(6)) * 2 - 1
    a["opacities"] = torch.rand(n, 1, generator=torch.Generator().manual_seed(7)) * 24 - 12
    a["quaternions"][0] = 0.0
    a["quaternions"][1] = torch.tensor([0.6e-20, 0.0, -0.8e-20, 0.0])
    a["sh_features_dc"][0, 0, 0] = -2.5
    opac, quats, col = (np.zeros((n, w), np.float32) for w in (1, 4, 3))
    arr = {k: _np(v) for k, v in a.items()}
    L.host_scene_activate(n, _ptr(arr["opacities"]), _ptr(arr["quaternions"]), _ptr(arr["sh_features_dc"]), _ptr(opac), _ptr(quats), _ptr(col))
    ref = gc.activations64(a["opacities"], a["scales"], a["quaternions"], a["sh_features_dc"])
    sh = torch.cat((a["sh_features_dc"], a["sh_features_rest"]), dim=1)
    t32 = {"opacities": torch.sigmoid(a["opacities"]), "quaternions": torch.nn.functional.normalize(a["quaternions"]),
           "colors": renderer.get_colors(sh_features=sh, directions=None, sh_levels=1)}
    for k, got in (("opacities", opac), ("quaternions", quats), ("colors", col)):
        floor = 0.5 if k == "colors" else 0.0
        e, et = gc.ulps(torch.from_numpy(got), ref[k], floor), gc.ulps(t32[k], ref[k], floor)
        assert e <= max(2.0 * et, 1.0), (k, e, et)
    assert not quats[0].any() and col[0, 0] == 0.0
    for levels in (1, 2, 3, 4):
        for cam in (torch.tensor([0.3, -2.0, 0.8]), a["positions"][17] + torch.tensor([6e-4, -8e-4, 0.0])):
            out = np.zeros((n, 3), np.float32)
            camn = _np(cam)
            L.host_scene_colors(n, levels, _ptr(arr["positions"]), _ptr(arr["sh_features_dc"]), _ptr(arr["sh_features_rest"]), _ptr(camn), _ptr(out))
            ref = gc.colors64(a["sh_features_dc"], a["sh_features_rest"], a["positions"], cam, levels)
            t = renderer.GaussianRenderer().compute_colors(sh, positions=a["positions"], camera_positions=cam[None], sh_levels=levels)
            e, et = gc.ulps(torch.from_numpy(out), ref, 0.5), gc.ulps(t, ref, 0.5)
            assert e <= max(2.0 * et, 1.0), (levels, e, et)
    # the merge's argument check, on the host: the sum of the counts may not overflow, and must fit the capacity
    from dreamwaltz_g_amd.background import ScenePartC
    parts = (ScenePartC * 17)()
    for i in range(17):
        parts[i].positions = parts[i].opacities = parts[i].colors = parts[i].scales = parts[i].quaternions = 4096
        parts[i].count = i + 1
    total = ctypes.c_int64(-1)
    ok = lambda n, cap, levels=1: L.host_scene_check_merge(n, parts, levels, cap, ctypes.c_void_p(8192), ctypes.byref(total))      # noqa: E731
    assert ok(17, 153) == 1 and total.value == 153 and ok(17, 152) == 0 and ok(18, 1000) == 0 and ok(17, 153, levels=4) == 1
    parts[3].count = 2 ** 63 - 1
    assert ok(17, 2 ** 63 - 1) == 0
