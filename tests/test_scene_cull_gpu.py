"""The per-camera cull of the Gaussian scene on the device (boundary B25: csrc/scene_cull.hip through GaussianBackground.culled and Scene's
cull_scene): the flags against the g++ build of csrc/cull_math.h bit for bit, the kept set against the radii the real
rasterizer reports, the compaction and the gather against index_select, and -- the acceptance criterion -- frames with culling on against
frames with culling off by torch.equal.  Scene sizes 1, 63 and 1021 (2500 where the scan has to cross a block), avatar parts of 3 and 257
rows, images 64 x 64 and 67 x 35."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import dwg_import  # noqa: F401
from tests import gs_background_cases as gc
from tests import scene_cull_cases as cc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ATTRS = ("positions", "opacities", "colors", "scales", "quaternions")
WIDTH = {"positions": 3, "opacities": 1, "colors": 3, "scales": 3, "quaternions": 4}
SIZES = (1, 63, 1021)


def _offset(t):
    """The same values as a view at storage_offset 1 of a device buffer: 4-byte aligned, never 16."""
    flat = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    flat[1:].copy_(t.reshape(-1))
    v = flat[1:].view(t.shape)
    assert v.storage_offset() == 1 and v.data_ptr() % 16 == 4
    return v


def _background(arrays, sh_levels=1, offset=False):
    from dreamwaltz_g_amd.background import GaussianBackground
    arrays = {k: (_offset(v) if offset else v.to(DEV)) for k, v in arrays.items()}
    return GaussianBackground.from_tensors(**arrays, sh_levels=sh_levels).to(DEV)


def _case_background(name, n, H, W, sh_levels=1, offset=False, seed=0):
    pos, scales, quats, cam = cc.case(name, n, H, W, seed=seed)
    cam = {k: (v.to(DEV) if torch.is_tensor(v) and k in ("extrinsic", "projection", "c2w") else v) for k, v in cam.items()}
    return _background(cc.background_arrays(pos, scales, quats, seed=seed), sh_levels=sh_levels, offset=offset), cam


def _room(n, seed=0, grow=5.0):
    """The benchmark's room with Gaussians large enough to show in a small image, as from_tensors takes it."""
    pos, scales, quats = cc.box_scene(n, seed)
    return cc.background_arrays(pos, scales * np.float32(grow), quats, seed=seed)


def _camera(where="inside", H=64, W=64, **kw):
    from dreamwaltz_g_amd import camera
    if kw:
        return camera.make_camera(fovy=55.0, height=H, width=W, device=DEV, **kw)
    return cc.box_camera(where, H, W, device=DEV)


def _parts(n_a, seed):
    """One well-formed avatar part of n_a rows near the origin, at a 4-byte aligned offset."""
    from dreamwaltz_g_amd.avatar import GaussianOutput
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)           # noqa: E731
    rows = dict(positions=(u(n_a, 3) - 0.5) * 0.8, opacities=u(n_a, 1), colors=u(n_a, 3), scales=u(n_a, 3) * 0.03 + 0.005,
                quaternions=torch.nn.functional.normalize(torch.randn(n_a, 4, generator=g)))
    return [GaussianOutput(**{k: _offset(rows[k]) for k in ATTRS})]


def _host_flags(bg, cams, H, W):
    """The flags the g++ build of csrc/cull_math.h gives for the device's own inputs (activated scales, camera blocks)."""
    from dreamwaltz_g_amd.background import _cull_camera_blocks
    blocks = _cull_camera_blocks(cams, DEV).cpu().numpy()
    return cc.host_flags(cc.hostlib(), bg._positions.cpu().numpy(), bg.activated()["scales"].cpu().numpy(), blocks, H, W)


# ---- flags ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", cc.IMAGES, ids=lambda hw: "%dx%d" % (hw[1], hw[0]))
@pytest.mark.parametrize("n_cameras", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_flags_equal_the_host_build_of_the_same_statements_bit_for_bit(n, n_cameras, hw):
    """Every operation of csrc/cull_math.h is rounded on its own, so the device and g++ (-ffp-contract=off) agree on every flag -- for the
    cases built to sit on the test's edges too (a cluster at the near plane, scales over five decades).  The kept indices ARE the flags:
    index is ascending and complete."""
    H, W = hw
    for name in cc.GENERATORS:
        bg, cam = _case_background(name, n, H, W, seed=n)
        cams = [cam, _camera("corner", H, W), _camera("outside", H, W)][:n_cameras]
        want = _host_flags(bg, cams, H, W)
        culled = bg.culled(cams, H, W)
        got = np.zeros(n, np.uint8)
        got[culled.index.cpu().numpy()] = 1
        assert culled.index.dtype == torch.int32 and culled.n_total == n and culled.n_points == int(want.sum()), name
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        assert np.array_equal(culled.index.cpu().numpy(), np.nonzero(want)[0]), name


# ---- the kept set against the real rasterizer ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", cc.IMAGES, ids=lambda hw: "%dx%d" % (hw[1], hw[0]))
@pytest.mark.parametrize("n_a", [3, 257])
@pytest.mark.parametrize("name", cc.GENERATORS)
def test_every_scene_gaussian_the_rasterizer_gives_a_radius_is_kept(name, n_a, hw):
    from dreamwaltz_g_amd import renderer
    from dreamwaltz_g_amd.background import scene_merge
    H, W = hw
    n = 1021
    bg, cam = _case_background(name, n, H, W, seed=7)
    parts = _parts(n_a, seed=n_a)
    merged = scene_merge(parts, bg, cam["c2w"][:, :3, 3])
    out = renderer.GaussianRenderer(sh_levels=1).render(data=cam, gaussians=merged, return_2d_radii=True)
    seen = (out["radii"][n_a:] > 0).cpu().numpy()
    kept = np.zeros(n, bool)
    culled = bg.culled(cam, H, W)
    kept[culled.index.cpu().numpy()] = True
    print("%s %dx%d: the rasterizer gives %d of %d scene Gaussians a radius, the cull keeps %d" % (name, W, H, seen.sum(), n, kept.sum()))
    assert out["radii"].shape[0] == n_a + n
    assert not (seen & ~kept).any(), np.nonzero(seen & ~kept)[0][:8]
    if name.startswith("box_"):
        assert seen.any()


# ---- compaction and gather ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES + (2500,))
def test_compaction_keeps_the_order_and_the_gather_equals_index_select(n):
    """The C entries on handmade flags: none, all, an odd count, a random subset -- ascending indices, the count in its device word,
    nothing written behind index[count); then the gather of rows of 1, 3, 4 and 45 floats from tables at 4-byte aligned offsets into
    tables at such offsets, with guard rows behind the block."""
    from dreamwaltz_g_amd import _lib
    from dreamwaltz_g_amd.background import CULL_MAX_ROWS, CullRowsC
    L = _lib.lib()
    g = torch.Generator().manual_seed(n)
    patterns = {"none": torch.zeros(n, dtype=torch.uint8), "all": torch.ones(n, dtype=torch.uint8),
                "random": (torch.rand(n, generator=g) < 0.4).to(torch.uint8), "last": torch.zeros(n, dtype=torch.uint8)}
    patterns["last"][-1] = 1
    odd = patterns["random"].clone()
    if int(odd.sum()) % 2 == 0:
        odd[0] ^= 1
    patterns["odd"] = odd
    work = torch.empty(max(int(L.dwg_scene_cull_workspace_bytes(n)), 4), dtype=torch.uint8, device=DEV)
    tables = {w: _offset(torch.randn(n, w, generator=g)) for w in (1, 3, 4, 45)}
    for name, flags in patterns.items():
        want = torch.nonzero(flags).reshape(-1).to(torch.int32)
        kept = int(want.numel())
        index = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV)
        count = torch.full((2,), -7, dtype=torch.int32, device=DEV)
        _lib.check(L.dwg_scene_cull_compact(n, _lib.ptr(flags.to(DEV)), _lib.ptr(index), _lib.ptr(count), _lib.ptr(work), _lib.stream(DEV)), name)
        assert count.tolist() == [kept, -7], name
        assert torch.equal(index[:kept].cpu(), want) and bool((index[kept:] == -7).all()), name
        if kept > 1:
            assert bool((index[1:kept] > index[:kept - 1]).all()), name
        guard = 7.25
        outs = {w: _offset(torch.full((kept + 2, w), guard)) for w in tables}
        rows = (CullRowsC * CULL_MAX_ROWS)()
        for r, (w, t) in zip(rows, tables.items()):
            r.src, r.dst, r.width = t.data_ptr(), outs[w].data_ptr(), w
        _lib.check(L.dwg_scene_cull_gather(kept, _lib.ptr(index), n, len(tables), rows, _lib.stream(DEV)), name)
        for w, t in tables.items():
            assert torch.equal(outs[w][:kept], t.index_select(0, want.to(DEV).long())), (name, w)
            assert bool((outs[w][kept:] == guard).all()), (name, w)
    # a bad argument is refused before any launch
    E = _lib.CONSTANTS["DWG_E_ARG"] if "DWG_E_ARG" in _lib.CONSTANTS else -1
    f = patterns["all"].to(DEV)
    assert L.dwg_scene_cull_compact(-1, _lib.ptr(f), _lib.ptr(index), _lib.ptr(count), _lib.ptr(work), None) == E
    assert L.dwg_scene_cull_gather(n + 1, _lib.ptr(index), n, 1, rows, None) == E
    assert L.dwg_scene_cull_flags(n, _lib.ptr(tables[3]), _lib.ptr(tables[3]), 0, _lib.ptr(tables[45]), 37, 64, 64, _lib.ptr(f), None) == E


@pytest.mark.parametrize("sh_levels", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_the_culled_block_is_index_select_of_the_scene(n, sh_levels):
    bg, cam = _case_background("box_inside", n, 64, 64, sh_levels=sh_levels, offset=True, seed=n + 3)
    culled = bg.culled(cam, 64, 64)
    idx = culled.index.long()
    assert culled.sh_levels == sh_levels and culled.n_total == n and culled.n_points == idx.numel()
    if n > 1:
        assert 0 < culled.n_points < n
        assert bool((culled.index[1:] > culled.index[:-1]).all())
    block, full = culled.activated(), bg.activated()
    assert torch.equal(culled._positions, bg._positions.index_select(0, idx))
    for k in ("opacities", "scales", "quaternions", "colors"):
        assert block[k].shape[1:] == full[k].shape[1:] and torch.equal(block[k], full[k].index_select(0, idx)), k
    if sh_levels > 1:
        assert torch.equal(culled._sh_features_dc, bg._sh_features_dc.index_select(0, idx))
        assert torch.equal(culled._sh_features_rest, bg._sh_features_rest.index_select(0, idx))
    else:
        assert culled._sh_features_dc is None and culled._sh_features_rest is None


# ---- the image does not change -------------------------------------------------------------------------------------------------------------
def _scene(arrays, n_avatars=1, sh_levels=1, cull_scene=False, **render):
    from dreamwaltz_g_amd import configs, scene as sc, sds_step
    cfg = configs.TrainConfig(); cfg.device = str(DEV); cfg.render.bg_color = (0.5, 0.5, 0.5)
    for k, v in render.items():
        setattr(cfg.render, k, v)
    avatars = [sds_step.build_synthetic_avatar(2000, DEV, seed=s)[0] for s in range(n_avatars)]
    bg = _background(arrays, sh_levels=sh_levels)
    scene = sc.Scene(cfg, avatars[0] if n_avatars == 1 else avatars, background=bg, async_pair_count=True, cull_scene=cull_scene).to(DEV).eval()
    return scene, bg


def _pose(seed, n_avatars=1):
    from dreamwaltz_g_amd import synth
    ps = [synth.random_smpl_inputs(seed=seed + 100 * i, device=DEV) for i in range(n_avatars)]
    return ps[0] if n_avatars == 1 else {k: torch.cat([p[k] for p in ps], dim=0) for k in ps[0]}


def _keep(o):
    return {k: o[k].clone() for k in ("image", "depth", "alpha")}


def _same(on, off):
    for k in ("image", "depth", "alpha"):
        assert on[k].shape == off[k].shape and torch.equal(on[k], off[k]), k


@pytest.mark.parametrize("hw", cc.IMAGES, ids=lambda hw: "%dx%d" % (hw[1], hw[0]))
@pytest.mark.parametrize("case", ["plain", "white", "two_avatars_transl", "sh3", "zero_scales", "constants"])
def test_frames_with_culling_on_equal_frames_with_culling_off(case, hw):
    H, W = hw
    A = 2 if case == "two_avatars_transl" else 1
    render = {"zero_scales": dict(use_zero_scales=True), "constants": dict(use_constant_colors=(0.2, 0.7, 0.4), use_constant_opacities=0.3),
              "two_avatars_transl": dict(avatar_transl="[[-0.4, 0.0, 0.0], [0.4, 0.0, 0.1]]")}.get(case, {})
    scene, bg = _scene(_room(1021, seed=5), n_avatars=A, sh_levels=3 if case == "sh3" else 1, **render)
    bg_mode = "white" if case == "white" else None
    poses = [_pose(60 + i, A) for i in range(3)]
    cams = [_camera(w, H, W) for w in ("inside", "corner", "outside")]
    with torch.inference_mode():
        # one camera for the call, F = 1 and F = 3
        off = _keep(scene.forward_frames(cams[0], poses, bg_mode=bg_mode))
        on = _keep(scene.forward_frames(cams[0], poses, bg_mode=bg_mode, cull_scene=True))
        _same(on, off)
        kept = bg.culled(cams[0], H, W).n_points
        assert 0 < kept < 1021 and bg.cull_launches == 1
        _same(_keep(scene.forward_frames(cams[0], poses[:1], bg_mode=bg_mode, cull_scene=True)), {k: v[:1] for k, v in off.items()})
        assert bg.cull_launches == 1
        # three frames under three cameras: the union serves all of them
        off3 = _keep(scene.forward_frames(cams, poses, bg_mode=bg_mode))
        on3 = _keep(scene.forward_frames(cams, poses, bg_mode=bg_mode, cull_scene=True))
        _same(on3, off3)
        union = bg.culled(cams, H, W)
        assert kept <= union.n_points <= 1021 and bg.cull_launches == 2
        # the scene is in the picture: without it the frame is another one
        scene.background = None
        assert not torch.equal(scene.forward_frames(cams[0], poses[:1], bg_mode=bg_mode)["alpha"], off["alpha"][:1])


def test_gaussians_at_the_same_position_keep_their_order():
    """Pairs of scene Gaussians at the SAME position with different colours, both visible: their depths tie, and the rasterizer resolves a
    tie by index -- the compaction keeps the relative order, so the picture is the same bit for bit (reversing the pairs' colours is
    another picture: the order does show)."""
    H = W = 64
    arrays = _room(512, seed=8, grow=12.0)
    twice = {k: v.repeat_interleave(2, dim=0).clone() for k, v in arrays.items()}
    twice["opacities"][:] = 1.5                                        # translucent: both Gaussians of a pair show
    twice["sh_features_dc"][1::2] = -twice["sh_features_dc"][1::2] + 0.5
    scene, bg = _scene(twice)
    cam, poses = _camera("inside", H, W), [_pose(70)]
    with torch.inference_mode():
        off = _keep(scene.forward_frames(cam, poses))
        on = _keep(scene.forward_frames(cam, poses, cull_scene=True))
        _same(on, off)
        idx = bg.culled(cam, H, W).index
        assert 0 < idx.numel() < 1024 and bool((idx[0::2] + 1 == idx[1::2]).all())          # pairs are kept or dropped together
        swapped = dict(twice, sh_features_dc=twice["sh_features_dc"].view(-1, 2, 1, 3).flip(1).reshape(-1, 1, 3))
        scene.background = _background(swapped)
        assert not torch.equal(scene.forward_frames(cam, poses)["image"], off["image"])


@pytest.mark.parametrize("sh_levels", [1, 3])
def test_a_camera_that_sees_none_of_the_scene_and_one_that_sees_all_of_it(sh_levels):
    """Kept count 0 and kept count N are ordinary cases: a scene that lies entirely behind the camera (the avatar stays in view), and a
    small scene seen whole from afar."""
    H = W = 64
    cam = _camera("inside", H, W)
    arrays = gc.scene_arrays(1021, seed=3)
    behind = dict(arrays, positions=arrays["positions"] * 0.5 + 4.0 * cam["c2w"][0, :3, 3].cpu())       # the camera looks at the origin
    scene, bg = _scene(behind, sh_levels=sh_levels)
    poses = [_pose(80), _pose(81)]
    with torch.inference_mode():
        off = _keep(scene.forward_frames(cam, poses))
        on = _keep(scene.forward_frames(cam, poses, cull_scene=True))
        _same(on, off)
        none = bg.culled(cam, H, W)
        assert none.n_points == 0 and none.index.numel() == 0 and none.n_total == 1021 and none.activated()["scales"].shape == (0, 3)
        assert float(off["alpha"].max()) > 0.5                           # the avatar is in the picture
        scene.background = bg = _background(arrays, sh_levels=sh_levels)
        far = _camera(H=H, W=W, radius=6.0, azimuth=20.0, elevation=80.0)
        off = _keep(scene.forward_frames(far, poses))
        on = _keep(scene.forward_frames(far, poses, cull_scene=True))
        _same(on, off)
        everything = bg.culled(far, H, W)
        assert everything.n_points == everything.n_total == 1021
        assert torch.equal(everything.index, torch.arange(1021, dtype=torch.int32, device=DEV))


# ---- cache -------------------------------------------------------------------------------------------------------------------------------
def test_the_culled_block_is_cached_and_a_hit_neither_launches_nor_syncs():
    H = W = 64
    scene, bg = _scene(_room(1021, seed=9), cull_scene=True)
    cam, poses = _camera("inside", H, W), [_pose(90), _pose(91)]
    with torch.inference_mode():
        first = _keep(scene.forward_frames(cam, poses))
        assert bg.cull_launches == 1
        block = bg.culled(cam, H, W)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")                        # a hit: no launch that would need the host, no read-back
        try:
            assert bg.culled(cam, H, W) is block and bg.culled([cam], H, W) is block
        finally:
            torch.cuda.set_sync_debug_mode(0)
        with warnings.catch_warnings(record=True) as rec:               # whatever the rasterizer chain does, the cull adds no sync
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                again = _keep(scene.forward_frames(cam, poses))
            finally:
                torch.cuda.set_sync_debug_mode(0)
        mine = [str(r.filename) + ":" + str(r.lineno) for r in rec if r.filename.endswith(("background.py", "scene.py"))]
        assert not mine, mine
        assert bg.cull_launches == 1
        _same(again, first)
        # the camera changed in place: recomputed, and the frames are those of culling off under the new camera
        with torch.inference_mode(False), torch.no_grad():
            moved = _camera("corner", H, W)
            for k in ("extrinsic", "c2w"):
                cam[k].copy_(moved[k])
        on = _keep(scene.forward_frames(cam, poses))
        assert bg.cull_launches == 2 and bg.culled(cam, H, W) is not block
        _same(on, _keep(scene.forward_frames(cam, poses, cull_scene=False)))
        # a new camera tensor with the same values: recomputed (the key is the tensor, not its values)
        scene.forward_frames(dict(cam, extrinsic=cam["extrinsic"].clone()), poses)
        assert bg.cull_launches == 3
        # a scene parameter changed: recomputed, with the activation
        cam2 = _camera("inside", H, W)
        scene.forward_frames(cam2, poses)
        before = bg.culled(cam2, H, W).n_points
        assert bg.cull_launches == 4
        with torch.inference_mode(False), torch.no_grad():
            bg._scales.add_(1.5)
        on = _keep(scene.forward_frames(cam2, poses))
        assert bg.cull_launches == 5 and bg.activation_launches == 2 and bg.culled(cam2, H, W).n_points > before
        _same(on, _keep(scene.forward_frames(cam2, poses, cull_scene=False)))
        with torch.inference_mode(False), torch.no_grad():
            bg._positions.mul_(0.5)
        scene.forward_frames(cam2, poses)
        assert bg.cull_launches == 6 and bg.activation_launches == 2


# ---- a camera on a track: temporary camera dicts ------------------------------------------------------------------------------------------
def test_temporary_camera_dicts_of_different_cameras_never_hit_a_stale_block():
    """A playback loop that builds a fresh camera dict per call and drops it: the allocator hands the next dict's tensors the addresses
    of the last one's, with the same version counters.  Every cached block holds the camera tensors its key identifies, so such a
    tensor can never stand for another camera: each new camera culls again, and the frames are those of culling off."""
    from dreamwaltz_g_amd import camera
    from dreamwaltz_g_amd.background import CULL_CACHE_BLOCKS
    H = W = 64
    scene, bg = _scene(_room(1021, seed=12))
    poses = [_pose(97)]
    track = [dict(radius=2.4, azimuth=float(az), elevation=80.0) for az in range(0, 360, 45)]
    assert len(track) > CULL_CACHE_BLOCKS                             # blocks are evicted, and their tensors freed, along the way
    kept = []
    with torch.inference_mode():
        for i, kw in enumerate(track):
            want = _keep(scene.forward_frames(camera.make_camera(fovy=55.0, height=H, width=W, device=DEV, **kw), poses))
            got = _keep(scene.forward_frames(camera.make_camera(fovy=55.0, height=H, width=W, device=DEV, **kw), poses, cull_scene=True))
            assert bg.cull_launches == i + 1, (i, bg.cull_launches)
            _same(got, want)
            block = next(reversed(bg._cull_cache.values()))
            kept.append(block.n_points)
            assert len(block.camera_tensors) == 4                     # extrinsic, projection, c2w, tanfov: held by the block
        assert len(bg._cull_cache) == CULL_CACHE_BLOCKS and len(set(kept)) > 1
        # two cameras that stay alive share the cache: neither evicts the other
        a, b = _camera("inside", H, W), _camera("corner", H, W)
        for cam in (a, b, a, b):
            scene.forward_frames(cam, poses, cull_scene=True)
        assert bg.cull_launches == len(track) + 2



# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name():
    H = W = 64
    scene, bg = _scene(_room(63, seed=11), use_fixed_n_gaussians=1000)
    cam, poses = _camera("inside", H, W), [_pose(95)]
    with torch.inference_mode():
        with pytest.raises(ValueError, match="cull_scene with use_fixed_n_gaussians"):
            scene.forward_frames(cam, poses, cull_scene=True)
        scene.forward_frames(cam, poses)                                # without culling the override works as before
    assert bg.cull_launches == 0
    # culled() inside a graph capture: refused by name on a miss, served on a hit
    known = bg.culled(cam, H, W)
    other = _camera("corner", H, W)
    x = torch.zeros(4, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            x.add_(1.0)
            assert bg.culled(cam, H, W) is known
            with pytest.raises(RuntimeError, match="cannot be computed inside a graph capture"):
                bg.culled(other, H, W)
    torch.cuda.current_stream(DEV).wait_stream(side)
    assert bg.cull_launches == 1
    with pytest.raises(ValueError, match="expected 1..64"):
        bg.culled(torch.zeros(65, 37, device=DEV), H, W)
