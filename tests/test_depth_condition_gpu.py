"""-m gpu parity of the depth-map condition and of the pretrain loss (dreamwaltz_g_amd/condition.py, pretrain.py over csrc/depthmap.hip,
boundary B9) against tests/depthmap_ref.py: float64 pinhole rays through oracle.condition.ray_cast, the numpy-float32 image statements,
and the loss in torch float64.

Bars.  Depth: the hit mask differs from the oracle's at <= 1 pixel per image (an fp64 last-bit tie; the oracle's own one-ulp
perturbations flip none), and where both hit |t - t_ref| / t_ref <= 3 s + 2^-23, s being the oracle's OWN sensitivity to one float32
ulp of the ray (the most the two sides may legitimately differ by; 2^-23 is the fp32 store of t).  Normals: 1e-6 (both sides fp64 from
the same vertices, stored fp32).  Image from a given map: bytes equal.  End to end: >= 99.9 % of pixels equal, none off by more than one
level.  Loss: max(4 x the error of torch's own fp32 evaluation, 4 fp32 ulp); gradients: 4 fp32 ulp (three roundings), plus half an fp16
ulp where the gradient is STORED as fp16 (the store's own rounding)."""
import types

import numpy as np
import pytest
import torch

from tests import depthmap_ref as dr

pytestmark = pytest.mark.gpu


def _cond():
    from dreamwaltz_g_amd import condition as cd, configs
    return cd, cd.SMPL2Condition(configs.PromptConfig())


def _cam(c):
    return dict(extrinsic=torch.from_numpy(c["E"]).cuda(), intrinsics=torch.from_numpy(c["K"]).cuda(), width=c["W"], height=c["H"])


def _scene(cd, c, shift=None):
    v = c["v"] if shift is None else (c["v"] + np.asarray(shift, dtype=np.float32))
    return cd.build_ray_casting_scene(torch.from_numpy(v).cuda(), c["t"])


@pytest.mark.parametrize("name", dr.CASES)
def test_depth_and_normals_match_the_oracle(name):
    cd, cond = _cond()
    c = dr.case(name)
    ref = c["ref"]
    scene = _scene(cd, c)
    out = cond.export_depth(scene, raw=True, **_cam(c))
    assert isinstance(out, cd.DepthMap) and out.t.shape == (c["H"], c["W"]) and out.t.dtype == torch.float32
    t = out.to_numpy().astype(np.float64)
    hit, hit_ref = np.isfinite(t), np.isfinite(ref["t"])
    assert not np.isnan(t).any() and (t[~hit] == np.inf).all()
    both = hit & hit_ref
    rel = np.abs(t[both] - ref["t"][both]) / ref["t"][both]
    bound = 3 * c["s"] + 2.0 ** -23
    print("%s: hits %d / %d (oracle %d), mask differences %d, max rel err %.3e, bound %.3e (s = %.3e)"
          % (name, hit.sum(), hit.size, hit_ref.sum(), (hit != hit_ref).sum(), rel.max(), bound, c["s"]))
    assert hit.mean() >= 0.04
    assert (hit != hit_ref).sum() <= 1
    assert rel.max() <= bound
    # normals of the hit triangle; pixels where the oracle has a second triangle within 1e-6 of the nearest may name the other one
    n = cond.export_normal_raw(scene, raw=True, **_cam(c))
    assert n.shape == (c["H"], c["W"], 3) and n.dtype == torch.float32
    n = n.cpu().numpy().astype(np.float64)
    close = both & ((ref["second"] - ref["t"]) <= 1e-6 * ref["t"])
    assert close.sum() <= 0.01 * hit_ref.sum()
    use = both & ~close
    err = np.abs(n[use] - ref["normal"][use]).max()
    print("%s: normals max err %.3e over %d pixels (%d skipped)" % (name, err, use.sum(), close.sum()))
    assert err <= 1e-6
    assert (n[~hit] == 0).all()
    assert np.abs(np.linalg.norm(n[hit], axis=1) - 1).max() < 1e-6


@pytest.mark.parametrize("name", ["front", "wide", "inside"])
def test_image_from_a_given_depth_tensor_is_bit_exact(name):
    cd, cond = _cond()
    t32 = dr.case(name)["ref"]["t"].astype(np.float32)
    ref = dr.depth_image(t32)
    u8, chw = cond.depth_image(torch.from_numpy(t32).cuda(), out_u8=True, out_chw=True)
    assert u8.shape == t32.shape + (3,) and u8.dtype == torch.uint8 and chw.shape == (1, 3) + t32.shape
    assert (ref > 0).any() and ref.max() == 255
    assert np.array_equal(u8.cpu().numpy(), ref)
    assert (chw[0] - u8.permute(2, 0, 1).float() / 255.0).abs().max() < 1e-7


def test_image_of_a_random_map_of_odd_size_is_bit_exact():
    cd, cond = _cond()
    g = np.random.default_rng(5)
    t32 = g.uniform(0.3, 7.0, (37, 301)).astype(np.float32)
    t32[g.uniform(size=t32.shape) < 0.3] = np.inf
    u8, _ = cond.depth_image(torch.from_numpy(t32).cuda())
    assert np.array_equal(u8.cpu().numpy(), dr.depth_image(t32))
    t32[:] = 2.5                                               # a flat map: the maximum is 0 after the subtraction -> all zero
    assert int(cond.depth_image(torch.from_numpy(t32).cuda())[0].max()) == 0


@pytest.mark.parametrize("name", dr.CASES)
def test_export_depth_end_to_end(name):
    cd, cond = _cond()
    c = dr.case(name)
    ref = dr.depth_image(c["ref"]["t"].astype(np.float32))
    scene = _scene(cd, c)
    out = cond.export_depth(scene, **_cam(c))
    assert isinstance(out, cd.ConditionImage) and out.u8.shape == (c["H"], c["W"], 3) and out.u8.dtype == torch.uint8
    img = out.u8.cpu().numpy()
    diff = np.abs(img.astype(np.int32) - ref.astype(np.int32))
    print("%s: %d of %d pixels differ, max %d levels" % (name, (diff.max(2) > 0).sum(), diff.shape[0] * diff.shape[1], diff.max()))
    assert (img == ref).all(2).mean() >= 0.999 and diff.max() <= 1
    assert out.to_pil().size == (c["W"], c["H"])
    chw = cond.export_depth_chw(scene, **_cam(c))
    assert chw.shape == (1, 3, c["H"], c["W"]) and (chw - out.to_chw()).abs().max() < 1e-7


def test_all_miss_and_empty_mesh():
    cd, cond = _cond()
    c = dr.case("front")
    away = _scene(cd, c, shift=(100.0, 0.0, 0.0))              # translated out of view
    empty = cd.build_ray_casting_scene(torch.from_numpy(c["v"]).cuda(), np.zeros((0, 3), dtype=np.int32))
    for scene in (away, empty):
        t = cond.export_depth(scene, raw=True, **_cam(c)).t
        assert bool((t == float("inf")).all())
        img = cond.export_depth(scene, **_cam(c)).u8
        assert int(img.max()) == 0
        chw = cond.export_depth_chw(scene, **_cam(c))
        assert not bool(torch.isnan(chw).any()) and float(chw.abs().max()) == 0.0
        n = cond.export_normal_raw(scene, **_cam(c))
        assert float(n.abs().max()) == 0.0


def test_call_depth_raw_mirrors_the_reference_seam():
    cd, cond = _cond()
    c = dr.case("side")
    K_raw = torch.from_numpy(np.asarray(dr.G["cond.side.intrinsics_raw"], dtype=np.float32)).cuda()
    E = torch.from_numpy(c["E"]).cuda()
    smpl = types.SimpleNamespace(vertices=torch.from_numpy(c["v"]).cuda()[None], joints=None)
    out = cond(smpl, c["t"], dict(extrinsic=E[None], intrinsics=K_raw[None]), "depth_raw", c["H"], c["W"])
    assert isinstance(out, cd.DepthMap)
    K = cd.adjust_intrinsics_size(K_raw, width=c["W"], height=c["H"])
    direct = cond.export_depth(_scene(cd, c), raw=True, extrinsic=E, intrinsics=K, width=c["W"], height=c["H"])
    assert torch.equal(out.t, direct.t)
    a = np.nan_to_num(np.asarray(out), posinf=0.0, neginf=0.0)             # trainer.py:1250 on the object itself
    assert a.shape == (c["H"], c["W"]) and a.dtype == np.float32 and np.isfinite(a).all()
    assert (a > 0).sum() == int(torch.isfinite(direct.t).sum()) > 0
    for kind in ("depth", "normal", "mesh"):
        with pytest.raises(NotImplementedError):
            cond(types.SimpleNamespace(vertices=None, joints=None), c["t"], {}, kind, c["H"], c["W"])


def test_two_calls_agree_no_host_sync_and_graph_replay():
    cd, cond = _cond()
    c = dr.case("front")
    dev = torch.device("cuda")
    vbuf = torch.from_numpy(c["v"]).to(dev)
    scene = cd.build_ray_casting_scene(vbuf, torch.from_numpy(c["t"]).to(dev))
    assert scene.vertices.data_ptr() == vbuf.data_ptr()        # the scene reads the caller's vertices where they lie
    cam = _cam(c)
    first = cond.export_depth(scene, raw=True, **cam).t
    img1 = cond.export_depth(scene, **cam).u8
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = cond.export_depth(scene, raw=True, **cam).t
        img2 = cond.export_depth(scene, **cam).u8
        nrm = cond.export_normal_raw(scene, **cam)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.equal(first, second) and torch.equal(img1, img2) and nrm.shape == (c["H"], c["W"], 3)
    # captured once, replayed with new vertices written in place
    moved = torch.from_numpy(c["v"] + np.array([0.05, -0.1, 0.02], dtype=np.float32)).to(dev)
    want_t = cond.export_depth(cd.build_ray_casting_scene(moved, scene.triangles), raw=True, **cam).t
    want_img = cond.export_depth(cd.build_ray_casting_scene(moved, scene.triangles), **cam).u8
    assert not torch.equal(want_t, first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cond.export_depth(scene, **cam)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            got_t = cond.export_depth(scene, raw=True, **cam).t
            got_img = cond.export_depth(scene, **cam).u8
        vbuf.copy_(moved)
        graph.replay()
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(got_t, want_t) and torch.equal(got_img, want_img)


# ----------------------------------------------------------------------------------------------------------------------
# the pretrain loss
# ----------------------------------------------------------------------------------------------------------------------
def _loss_inputs(dtype, seed=3):
    g = torch.Generator().manual_seed(seed)
    shape = (1, 1, 25, 44)
    sd = torch.where(torch.rand(shape, generator=g) < 0.4, 2.0 + torch.rand(shape, generator=g), torch.full(shape, float("inf")))
    sd[0, 0, 3, 5] = float("nan"); sd[0, 0, 7, 9] = float("-inf"); sd[0, 0, 11, 2] = 0.0; sd[0, 0, 12, 2] = 5e-7
    depth = (torch.rand(shape, generator=g) * 3.0).to(dtype)
    ws = torch.rand(shape, generator=g).to(dtype)
    return depth, ws, sd


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def _ulp16(x):
    a = np.abs(np.asarray(x, dtype=np.float64))
    return np.maximum(np.spacing(a.astype(np.float16)), np.spacing((a * 1.001).astype(np.float16))).astype(np.float64)


def _loss_bound(depth, ws, sd, l64):
    """max(4 x the error torch's own fp32 evaluation of the reference statements makes at these inputs, 4 fp32 ulp)."""
    err32 = abs(float(dr.loss(depth, ws, sd, dtype=torch.float32)[0].double()) - float(l64))
    return max(4 * err32, 4 * float(_ulp32(float(l64)))), err32


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_pretrain_loss_and_gradients_match_float64(dtype):
    from dreamwaltz_g_amd import pretrain
    depth, ws, sd = _loss_inputs(dtype)
    l64, gd64, gw64 = dr.loss(depth, ws, sd)

    def run(scale):
        d, w = depth.cuda().requires_grad_(True), ws.cuda().requires_grad_(True)
        out = pretrain.depth_mask_loss(d, w, sd.cuda())
        (out * scale).backward()
        return out.detach(), d.grad, w.grad

    out, gd, gw = run(1.0)
    assert out.dtype == torch.float32 and out.dim() == 0 and gd.dtype == dtype and gw.dtype == dtype and gd.shape == depth.shape
    err = abs(float(out.double().cpu()) - float(l64))
    bound, err32 = _loss_bound(depth, ws, sd, l64)
    print("%s: loss %.9g, float64 %.17g, error %.3e, torch fp32 error %.3e, bound %.3e" % (dtype, float(out), float(l64), err, err32, bound))
    assert err <= bound
    for name, g, g64 in (("depth", gd, gd64), ("weights_sum", gw, gw64)):
        g, g64 = g.double().cpu().numpy(), g64.numpy()
        tol = 4 * _ulp32(g64) + (0.5 * _ulp16(g64) if dtype == torch.float16 else 0.0)
        print("%s: grad %s worst error %.3f of its bound" % (dtype, name, (np.abs(g - g64) / tol).max()))
        assert (np.abs(g - g64) <= tol).all() and np.abs(g64).max() > 0
    # a GradScaler's scale arrives as the upstream gradient in device memory and passes through exactly
    out_s, gd_s, gw_s = run(65536.0)
    assert torch.equal(out_s, out)
    if dtype == torch.float32:
        assert torch.equal(gd_s, gd * 65536.0) and torch.equal(gw_s, gw * 65536.0)
    else:
        for g, g64 in ((gd_s, gd64), (gw_s, gw64)):
            g, g64 = g.double().cpu().numpy(), g64.numpy() * 65536.0
            assert (np.abs(g - g64) <= 4 * _ulp32(g64) + 0.5 * _ulp16(g64)).all()
    # bit-identical across runs
    out2, gd2, gw2 = run(1.0)
    assert torch.equal(out, out2) and torch.equal(gd, gd2) and torch.equal(gw, gw2)


def test_pretrain_loss_over_many_workgroups_and_refusals():
    """A size that takes more than one workgroup of partial sums and is no multiple of the block: against float64 at the same bar."""
    from dreamwaltz_g_amd import pretrain
    g = torch.Generator().manual_seed(11)
    n = (1, 1, 131, 257)
    depth, ws = torch.rand(n, generator=g) * 3, torch.rand(n, generator=g)
    sd = torch.where(torch.rand(n, generator=g) < 0.5, 1.0 + torch.rand(n, generator=g), torch.full(n, float("inf")))
    l64, gd64, _ = dr.loss(depth, ws, sd)
    d = depth.cuda().requires_grad_(True)
    out = pretrain.depth_mask_loss(d, ws.cuda(), sd.cuda())
    out.backward()
    err = abs(float(out.double().cpu()) - float(l64))
    assert err <= _loss_bound(depth, ws, sd, l64)[0]
    assert (np.abs(d.grad.double().cpu().numpy() - gd64.numpy()) <= 4 * _ulp32(gd64.numpy())).all()
    with pytest.raises(RuntimeError):
        pretrain.depth_mask_loss(depth, ws, sd)
    with pytest.raises(TypeError):
        pretrain.depth_mask_loss(depth.cuda().double(), ws.cuda().double(), sd.cuda())
    with pytest.raises(ValueError):
        pretrain.depth_mask_loss(depth.cuda(), ws.cuda()[..., :-1], sd.cuda())


class _StubTrainer:
    """What pretrain_forward reads of the reference's Trainer: render() and time_to_snapshot."""

    def __init__(self, depth, ws, snapshot):
        self.depth, self.ws, self.time_to_snapshot = depth, ws, snapshot
        self.renders = 0

    def render(self, data):
        self.renders += 1
        return {"image": torch.zeros(self.depth.shape[0], self.depth.shape[1], self.depth.shape[2], 3, device=self.depth.device),
                "depth": self.depth, "weights_sum": self.ws}


def test_pretrain_forward_on_a_stub_trainer():
    from PIL import Image
    from dreamwaltz_g_amd import condition as cd, pretrain
    depth, ws, sd = _loss_inputs(torch.float32)
    H, W = 25, 44
    nhwc = lambda x: x.permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True)          # noqa: E731  the renderer's [B,H,W,1]
    l64, gd64, _ = dr.loss(depth, ws, sd)
    dmap = cd.DepthMap(sd[0, 0].cuda())
    # snapshots off: no visual outputs, no host synchronisation, the map stays on the device
    tr = _StubTrainer(nhwc(depth), nhwc(ws), False)
    pretrain.pretrain_forward(tr, {"cond_images": [dmap]})                                   # warm-up (workspace)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, outs, vis = pretrain.pretrain_forward(tr, {"cond_images": [dmap]})
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert vis == {} and outs["depth"] is tr.depth and set(outs) == {"image", "depth", "weights_sum"}
    assert abs(float(loss) - float(l64)) <= _loss_bound(depth, ws, sd, l64)[0]
    assert (np.abs(tr.depth.grad[..., 0].double().cpu().numpy() - gd64[:, 0].numpy()) <= 4 * _ulp32(gd64[:, 0].numpy())).all()
    # the reference's np.ndarray (inf where the rays miss) gives the same loss
    loss_np, _, _ = pretrain.pretrain_forward(tr, {"cond_images": [sd[0, 0].numpy()]})
    assert torch.equal(loss_np, loss)
    # snapshots on: the reference's two pictures
    tr = _StubTrainer(nhwc(depth), nhwc(ws), True)
    loss_s, _, vis = pretrain.pretrain_forward(tr, {"cond_images": [dmap]})
    assert torch.equal(loss_s, loss) and set(vis) == {"depth", "mask"} and tr.renders == 1
    assert isinstance(vis["depth"], Image.Image) and vis["depth"].mode == "L" and vis["depth"].size == (W, H)
    clean = torch.nan_to_num(sd, nan=0.0, posinf=0.0, neginf=0.0)
    assert vis["mask"].shape == (1, 1, H, W) and torch.equal(vis["mask"].cpu(), (clean > 1e-6).float())
    want = (255 * clean[0, 0].numpy() / clean.max().item()).clip(0, 255).astype(np.uint8)
    assert np.array_equal(np.asarray(vis["depth"]), want)
    # a map of another size is resampled with the reference's bicubic interpolation, then fitted by the same kernels
    big = torch.where(torch.rand(50, 88, generator=torch.Generator().manual_seed(1)) < 0.5, torch.full((50, 88), 2.5), torch.full((50, 88), float("inf")))
    loss_r, _, vis = pretrain.pretrain_forward(tr, {"cond_images": [cd.DepthMap(big.cuda())]})
    resampled = torch.nn.functional.interpolate(torch.nan_to_num(big, posinf=0.0)[None, None].cuda(), size=(H, W), mode="bicubic").cpu()
    l64r = dr.loss(depth, ws, resampled)[0]
    assert abs(float(loss_r) - float(l64r)) <= _loss_bound(depth, ws, resampled, l64r)[0]
    assert vis["depth"].size == (88, 50) and vis["mask"].shape == (1, 1, H, W)
