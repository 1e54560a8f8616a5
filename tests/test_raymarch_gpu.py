"""GPU parity of the NeRF-stage ray marcher (boundary B6) against the CPU restatement in tests/raymarch_cases.py, driven through the
drop-in backend modules exactly as the reference's raymarching.py drives its pybind backend.  Reads nothing of the reference."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from tests import raymarch_cases as rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "dropin")
BOUND = 2.0
AABB = np.array([-BOUND] * 3 + [BOUND] * 3, np.float32)


def _mods():
    if DROPIN not in sys.path:
        sys.path.insert(0, DROPIN)
    import _raymarchinglatent
    import _raymarchingrgb
    return _raymarchingrgb, _raymarchinglatent


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _march(be, o, d, bits, C, H, nears, fars, noises, contract, dt_gamma, max_steps):
    """the reference's protocol (raymarching.py:240-255): count call with None outputs, counter.item(), allocation, write call"""
    N = o.shape[0]
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    rays = torch.empty(N, 2, dtype=torch.int32, device="cuda")
    args = (o, d, bits, BOUND, contract, dt_gamma, max_steps, N, C, H, nears, fars)
    be.march_rays_train(*args, None, None, None, rays, counter, noises)
    M = counter.item()
    xyzs = torch.zeros(M, 3, device="cuda"); dirs = torch.zeros(M, 3, device="cuda"); ts = torch.zeros(M, 2, device="cuda")
    be.march_rays_train(*args, xyzs, dirs, ts, rays, counter, noises)
    torch.cuda.synchronize()
    return xyzs, dirs, ts, rays, counter


def _scene(C, H, kind="body", views=1, W=40, seed=0):
    g, bits = rc.make_grid(C, H, BOUND, kind)
    o, d = rc.make_cameras(views, W, W, seed=seed)
    nears, fars = rc.near_far(o, d, AABB, 0.05)
    return g, bits, o, d, nears, fars


def test_near_far_bit_exact():
    rgb, _ = _mods()
    rng = np.random.RandomState(0)
    o = rng.uniform(-4, 4, (3000, 3)).astype(np.float32)
    d = rng.randn(3000, 3).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    extra_o = np.array([[0, 0, 0], [0.5, -0.3, 0.2], [5, 5, 5], [0, 0, -3], [0.5, 0, -3], [3, 0.1, 0.1], [0, 3, 0]], np.float32)
    extra_d = np.array([[1, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, 1], [0, 0, 1], [-1, 0, 0], [0, -1, 0]], np.float32)
    o, d = np.concatenate([o, extra_o]), np.concatenate([d, extra_d])
    N = len(o)
    nears = torch.empty(N, device="cuda"); fars = torch.empty(N, device="cuda")
    rgb.near_far_from_aabb(_cuda(o), _cuda(d), _cuda(AABB), N, 0.05, nears, fars)
    rn, rf = rc.near_far(o, d, AABB, 0.05)
    assert np.array_equal(nears.cpu().numpy(), rn) and np.array_equal(fars.cpu().numpy(), rf)
    assert (rn == rc.FLT_MAX).sum() > 100                     # misses
    assert rn[N - 7] == np.float32(0.05) and rn[N - 6] == np.float32(0.05)   # rays starting inside the box
    # half precision goes through fp32 temporaries and comes back in the caller's dtype
    nh = torch.empty(N, device="cuda", dtype=torch.float64); fh = torch.empty(N, device="cuda", dtype=torch.float64)
    rgb.near_far_from_aabb(_cuda(o).double(), _cuda(d).double(), _cuda(AABB).double(), N, 0.05, nh, fh)
    assert nh.dtype == torch.float64 and np.array_equal(nh.float().cpu().numpy(), rn)


@pytest.mark.parametrize("H,C", [(32, 1), (32, 2), (128, 1), (128, 2)])
def test_morton_and_packbits_exact(H, C):
    rgb, _ = _mods()
    n = H ** 3
    rng = np.random.RandomState(H + C)
    coords = rng.randint(0, H, (n, 3)).astype(np.int32)
    idx = torch.empty(n, dtype=torch.int32, device="cuda")
    rgb.morton3D(_cuda(coords), n, idx)
    assert np.array_equal(idx.cpu().numpy(), rc.morton3d(coords[:, 0], coords[:, 1], coords[:, 2]).astype(np.int32))
    back = torch.empty(n, 3, dtype=torch.int32, device="cuda")
    rgb.morton3D_invert(idx, n, back)
    assert np.array_equal(back.cpu().numpy(), coords)
    grid = rng.rand(C, n).astype(np.float32)
    bits = torch.empty(C * n // 8, dtype=torch.uint8, device="cuda")
    rgb.packbits(_cuda(grid), C * n // 8, 0.37, bits)
    assert np.array_equal(bits.cpu().numpy(), rc.packbits(grid, 0.37))


@pytest.mark.parametrize("perturb", [False, True])
@pytest.mark.parametrize("dt_gamma", [0.0, 1.0 / 256])
@pytest.mark.parametrize("contract", [False, True])
def test_march_rays_train_matches_restatement(perturb, dt_gamma, contract):
    rgb, _ = _mods()
    C, H, max_steps = 2, 64, 512
    g, bits, o, d, nears, fars = _scene(C, H, W=40, seed=int(perturb) + 2 * int(contract))
    N = len(o)
    noises = np.random.RandomState(5).rand(N).astype(np.float32) if perturb else np.zeros(N, np.float32)
    xyzs, dirs, ts, rays, counter = _march(rgb, _cuda(o), _cuda(d), _cuda(bits), C, H, _cuda(nears), _cuda(fars), _cuda(noises), contract,
                                           dt_gamma, max_steps)
    cnt, rx, rd, rt = rc.march_train(o, d, bits, BOUND, contract, dt_gamma, max_steps, C, H, nears, fars, noises)
    rays = rays.cpu().numpy()
    bad = np.nonzero(rays[:, 1] != cnt)[0]
    assert len(bad) == 0, "%d rays differ in count, first %s: %s vs %s" % (len(bad), bad[:5], rays[bad[:5], 1], cnt[bad[:5]])
    assert np.array_equal(rays[:, 0], np.concatenate([[0], np.cumsum(cnt)[:-1]]))
    assert counter.item() == cnt.sum() == xyzs.shape[0] > 0
    for a, b in ((xyzs, rx), (dirs, rd), (ts, rt)):
        assert np.abs(a.cpu().numpy() - b).max() <= 1e-6
    assert (cnt > 0).mean() > 0.1 and (contract or (cnt == 0).any())      # under contraction the outer cells catch every ray


SCAN_N = [1, 255, 1023, 1024, 1025, 4097, 1024 * 1024 + 5]
SCAN_REF = 256                                                   # rays the restatement marches


@functools.lru_cache(maxsize=None)
def _scan_scene():
    """Rays from the centre of a full grid (C = 1, H = 32, every bit set) with max_steps = 8: every step is a sample, so a ray's count is
    its length over dt capped at 8, and the pass is short.  Every odd ray ends before it starts and has no sample.  Ray n depends on n
    alone, so every N takes the first N rays.  -> device tensors, and the restatement's counts of the first SCAN_REF rays."""
    n = max(SCAN_N)
    rng = np.random.RandomState(18)
    d = rng.randn(n, 3).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.zeros((n, 3), np.float32)
    nears = np.full(n, 0.05, np.float32)
    fars = (nears + 1.5 * rng.rand(n)).astype(np.float32)
    fars[1::2] = 0.01
    noises = np.zeros(n, np.float32)
    bits = np.full(32 ** 3 // 8, 255, np.uint8)
    k = SCAN_REF
    ref = rc.march_train(o[:k], d[:k], bits, BOUND, False, 0.0, 8, 1, 32, nears[:k], fars[:k], noises[:k])[0]
    return tuple(_cuda(a) for a in (o, d, bits, nears, fars, noises)) + (torch.from_numpy(ref).cuda(),)


@pytest.mark.parametrize("N", SCAN_N)
def test_march_count_pass_offsets_and_counter(N):
    """The count pass of march_rays_train_into on its own: rays[:,0] = counter + exclusive cumsum of rays[:,1], counter += the sum.
    Sizes around the scan block of 1024 rays; the last one has more than 1024 blocks, so the scan of the block sums takes a second
    trip and carries the first trip's total across.  Integers: exact.  The input is not degenerate: the restatement's counts of the
    first rays (which the device's equal) hold zeros and non-zeros."""
    from dreamwaltz_g_amd import raymarch
    o, d, bits, nears, fars, noises, ref = _scan_scene()
    assert int((ref == 0).sum()) > 0 and int((ref > 0).sum()) > 0 and int(ref.max()) <= 8
    rays = torch.full((N, 2), -1, dtype=torch.int32, device="cuda")
    counter = torch.tensor([7], dtype=torch.int32, device="cuda")
    raymarch.march_rays_train_into(o[:N], d[:N], bits, BOUND, False, 0.0, 8, N, 1, 32, nears[:N], fars[:N], None, None, None, rays, counter,
                                   noises[:N])
    cnt = rays[:, 1].long()
    k = min(N, SCAN_REF)
    assert torch.equal(rays[:k, 1], ref[:k])
    assert int(cnt[1::2].count_nonzero()) == 0 and int(cnt.min()) >= 0
    if N > 1:
        assert int((cnt == 0).sum()) > 0 and int((cnt > 0).sum()) > 0
    csum = torch.cumsum(cnt, 0)
    assert torch.equal(rays[:, 0], (7 + csum - cnt).to(torch.int32))
    assert counter.tolist() == [7 + int(csum[-1])]


@pytest.mark.parametrize("n", [1, 257])
def test_packbits_by_value_and_from_device_memory(n):
    """dwg_raymarch_packbits (threshold by value) and dwg_raymarch_packbits_dev (threshold in device memory) on one grid with values
    below, at and above the threshold, a NaN and both infinities: the same bytes, the restatement's.  The comparison is a strict >, and
    a NaN threshold sets no bit."""
    from dreamwaltz_g_amd import occupancy, raymarch
    thresh = np.float32(0.37)
    grid = np.random.RandomState(n).rand(8 * n).astype(np.float32)
    grid[:8] = [thresh, np.nan, np.inf, 0.1, -np.inf, 0.9, np.nextafter(thresh, np.float32(1)), np.nextafter(thresh, np.float32(0))]
    grid[8::5] = thresh
    want = rc.packbits(grid, thresh)
    assert want[0] == 0b01100100
    g = _cuda(grid)
    for t, w in ((thresh, want), (np.float32(np.nan), np.zeros(n, np.uint8))):
        by_value = raymarch.packbits(g, float(t), torch.full((n,), 0xAA, dtype=torch.uint8, device="cuda"))
        from_dev = occupancy.packbits_dev(g, _cuda(np.array([t], np.float32)), torch.full((n,), 0x55, dtype=torch.uint8, device="cuda"))
        assert np.array_equal(by_value.cpu().numpy(), w) and np.array_equal(from_dev.cpu().numpy(), w)


def _composite_case(channels, seed=0):
    """rays with 0 samples, rays at max_steps (1024), rays that end on T_thresh, ordinary rays"""
    rng = np.random.RandomState(seed)
    counts = np.concatenate([[0, 0, 1024, 1024, 1, 63, 64, 65, 130], rng.randint(0, 300, 250), [0]])
    N, M = len(counts), int(counts.sum())
    rays = np.stack([np.concatenate([[0], np.cumsum(counts)[:-1]]), counts], 1).astype(np.int32)
    sig = rng.uniform(0, 6, M).astype(np.float32)
    dense = rng.rand(N) < 0.3                                 # these rays terminate on T_thresh
    for n in np.nonzero(dense)[0]:
        sig[rays[n, 0]:rays[n, 0] + rays[n, 1]] *= 60
    sig[rays[2, 0]:rays[2, 0] + 1024] = 0.05                   # a long transparent ray that runs to max_steps
    rgbv = rng.rand(M, channels).astype(np.float32)
    dt = rng.uniform(0.003, 0.03, M).astype(np.float32)
    t0 = np.zeros(M, np.float32)
    for n in range(N):
        s = slice(rays[n, 0], rays[n, 0] + rays[n, 1])
        t0[s] = 0.5 + np.cumsum(dt[s])
    ts = np.stack([t0, dt], 1).astype(np.float32)
    return rays, sig, rgbv, ts


def _close(a, b, rtol=1e-5, atol=2e-6):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    err = np.abs(a - b) - (atol + rtol * np.abs(b))
    assert err.max() <= 0, "max excess %.3e at %s (got %r, want %r)" % (err.max(), np.unravel_index(err.argmax(), err.shape),
                                                                       a.flat[err.argmax()], b.flat[err.argmax()])


@pytest.mark.parametrize("channels,binarize", [(3, False), (3, True), (4, False)])
def test_composite_train_forward_backward(channels, binarize):
    rgb, lat = _mods()
    be = rgb if channels == 3 else lat
    bz = (binarize,) if channels == 3 else ()
    rays, sig, col, ts = _composite_case(channels, seed=channels + 10 * binarize)
    N, M, T_thresh = len(rays), len(sig), 1e-4
    w = torch.zeros(M, device="cuda"); ws = torch.empty(N, device="cuda"); dep = torch.empty(N, device="cuda")
    img = torch.empty(N, channels, device="cuda")
    S, Cc, Ts, R = _cuda(sig), _cuda(col), _cuda(ts), _cuda(rays)
    be.composite_rays_train_forward(S, Cc, Ts, R, M, N, T_thresh, *bz, w, ws, dep, img)
    rw, rws, rdep, rimg, used = rc.composite_forward(sig, col, ts, rays, T_thresh, binarize)
    _close(w.cpu(), rw); _close(ws.cpu(), rws); _close(dep.cpu(), rdep); _close(img.cpu(), rimg)
    assert (used < rays[:, 1]).sum() > 20                     # T_thresh terminations happen
    assert (rays[:, 1] == 0).any() and (rays[:, 1] == 1024).any()
    rng = np.random.RandomState(7)
    gw, gws, gd, gi = rng.randn(M).astype(np.float32), rng.randn(N).astype(np.float32), rng.randn(N).astype(np.float32), rng.randn(N, channels).astype(np.float32)
    gs = torch.zeros(M, device="cuda"); gr = torch.zeros(M, channels, device="cuda")
    be.composite_rays_train_backward(_cuda(gw), _cuda(gws), _cuda(gd), _cuda(gi), S, Cc, Ts, R, ws, dep, img, M, N, T_thresh, *bz, gs, gr)
    # the formula is evaluated on the forward's own (float32) outputs, as the kernels do
    rgs, rgr = rc.composite_backward(gw, gws, gd, gi, sig, col, ts, rays, T_thresh, binarize)
    _close(gr.cpu(), rgr)
    _close(gs.cpu(), rgs, atol=2e-6 + 2e-6 * float(np.abs(rgs).max()))


def test_composite_train_fp16_and_autograd_api():
    rgb, _ = _mods()
    from dreamwaltz_g_amd import raymarch
    rays, sig, col, ts = _composite_case(3, seed=3)
    N, M = len(rays), len(sig)
    S = _cuda(sig).requires_grad_(); Cc = _cuda(col).requires_grad_()
    w, ws, dep, img = raymarch.composite_rays_train(S, Cc, _cuda(ts), _cuda(rays), 1e-4)
    rw, rws, rdep, rimg, _ = rc.composite_forward(sig, col, ts, rays, 1e-4)
    _close(img.detach().cpu(), rimg); _close(w.detach().cpu(), rw)
    gi = torch.randn(N, 3, device="cuda")
    (img * gi).sum().backward()
    rgs, rgr = rc.composite_backward(np.zeros(M), np.zeros(N), np.zeros(N), gi.cpu().numpy(), sig, col, ts, rays, 1e-4)
    _close(Cc.grad.cpu(), rgr)
    _close(S.grad.cpu(), rgs, atol=2e-6 + 2e-6 * float(np.abs(rgs).max()))
    # fp16 buffers: fp32 temporaries, results in the caller's dtype
    wh = torch.zeros(M, device="cuda", dtype=torch.float16); wsh = torch.empty(N, device="cuda", dtype=torch.float16)
    dh = torch.empty(N, device="cuda", dtype=torch.float16); ih = torch.empty(N, 3, device="cuda", dtype=torch.float16)
    rgb.composite_rays_train_forward(_cuda(sig).half(), _cuda(col).half(), _cuda(ts), _cuda(rays), M, N, 1e-4, False, wh, wsh, dh, ih)
    assert ih.dtype == torch.float16 and float((ih.float() - img.detach()).abs().max()) < 2e-2


@pytest.mark.parametrize("channels", [3, 4])
def test_inference_loop_matches_training_composite(channels):
    """nerf_renderer.py:358-385 restated, with perturb off and the same T_thresh on both paths.  The samples are the training march's,
    bit for bit; the composite differs by the inference rule (T = 1 - weights_sum before the sample, tested before moving on), which
    composites ONE more sample than the training rule on a ray that ends on T_thresh: that is checked against the restatement of
    the inference rule, and rays that never reach T_thresh match the training composite to 1e-5."""
    rgb, lat = _mods()
    be = rgb if channels == 3 else lat
    bz = (False,) if channels == 3 else ()
    C, H, max_steps, T_thresh = 2, 64, 1024, 1e-4
    g, bits, o, d, nears, fars = _scene(C, H, W=32, seed=4)
    N = len(o)
    O, D, B, NE, FA = _cuda(o), _cuda(d), _cuda(bits), _cuda(nears), _cuda(fars)
    xyzs, dirs, ts, rays, _ = _march(be, O, D, B, C, H, NE, FA, torch.zeros(N, device="cuda"), False, 0.0, max_steps)
    sig, col = rc.field(xyzs.cpu().numpy(), channels)
    M = len(sig)
    w = torch.zeros(M, device="cuda"); ws_t = torch.empty(N, device="cuda"); d_t = torch.empty(N, device="cuda")
    i_t = torch.empty(N, channels, device="cuda")
    be.composite_rays_train_forward(_cuda(sig), _cuda(col), ts, rays, M, N, T_thresh, *bz, w, ws_t, d_t, i_t)
    # inference loop
    ws_i = torch.zeros(N, device="cuda"); d_i = torch.zeros(N, device="cuda"); i_i = torch.zeros(N, channels, device="cuda")
    rays_alive = torch.arange(N, dtype=torch.int32, device="cuda")
    rays_t = NE.clone()
    step, samples = 0, []
    while step < max_steps:
        n_alive = rays_alive.shape[0]
        if n_alive <= 0:
            break
        n_step = max(min(N // n_alive, 8), 1)
        xi = torch.zeros(n_alive * n_step, 3, device="cuda"); di = torch.zeros_like(xi); ti = torch.zeros(n_alive * n_step, 2, device="cuda")
        be.march_rays(n_alive, n_step, rays_alive, rays_t, O, D, BOUND, False, 0.0, max_steps, C, H, B, NE, FA, xi, di, ti,
                      torch.zeros(n_alive, device="cuda"))
        si, ci = rc.field(xi.cpu().numpy(), channels)
        samples.append((rays_alive.cpu().numpy().copy(), n_step, xi.cpu().numpy(), ti.cpu().numpy()))
        be.composite_rays(n_alive, n_step, T_thresh, *bz, rays_alive, rays_t, _cuda(si), _cuda(ci), ti, ws_i, d_i, i_i)
        rays_alive = rays_alive[rays_alive >= 0]
        step += n_step
    # every sample the inference march produced is the training march's sample of that ray, bit for bit
    r = rays.cpu().numpy(); X = xyzs.cpu().numpy(); TS = ts.cpu().numpy()
    seen = np.zeros(N, np.int64)
    for alive, ns, xi, ti in samples:
        for k, n in enumerate(alive):
            for j in range(ns):
                row = k * ns + j
                if ti[row, 0] == 0:
                    break
                p = r[n, 0] + seen[n]
                assert seen[n] < r[n, 1] and np.array_equal(xi[row], X[p]) and np.array_equal(ti[row], TS[p]), (n, seen[n])
                seen[n] += 1
    # rays still alive when the loop's step budget ran out have composited only the samples seen so far
    rws, rdep, rimg = rc.composite_inference(sig, col, TS, np.stack([r[:, 0], seen], 1), T_thresh)
    _close(ws_i.cpu(), rws); _close(d_i.cpu(), rdep); _close(i_i.cpu(), rimg)
    _, _, _, _, used = rc.composite_forward(sig, col, TS, r, T_thresh)
    open_rays = (used == r[:, 1]) & (seen == r[:, 1])
    open_rays &= np.array([1 - rws[n] >= T_thresh for n in range(N)])    # never reached T_thresh on either rule
    assert open_rays.sum() > 50
    for a, b in ((ws_i, ws_t), (d_i, d_t), (i_i, i_t)):
        a, b = a.cpu().numpy()[open_rays], b.cpu().numpy()[open_rays]
        assert np.abs(a - b).max() <= 1e-5 * max(1.0, np.abs(b).max())


def test_reproducible():
    rgb, _ = _mods()
    C, H = 2, 64
    g, bits, o, d, nears, fars = _scene(C, H, W=48, seed=9)
    N = len(o)
    noises = _cuda(np.random.RandomState(1).rand(N).astype(np.float32))
    outs = []
    for _ in range(2):
        xyzs, dirs, ts, rays, counter = _march(rgb, _cuda(o), _cuda(d), _cuda(bits), C, H, _cuda(nears), _cuda(fars), noises, False, 1.0 / 256, 1024)
        sig, col = rc.field(xyzs.cpu().numpy(), 3)
        M = len(sig)
        w = torch.zeros(M, device="cuda"); ws = torch.empty(N, device="cuda"); dep = torch.empty(N, device="cuda"); img = torch.empty(N, 3, device="cuda")
        rgb.composite_rays_train_forward(_cuda(sig), _cuda(col), ts, rays, M, N, 1e-4, False, w, ws, dep, img)
        gen = torch.Generator(device="cuda").manual_seed(0)
        grads = [torch.randn(s, device="cuda", generator=gen) for s in ((M,), (N,), (N,), (N, 3))]
        gs = torch.zeros(M, device="cuda"); gr = torch.zeros(M, 3, device="cuda")
        rgb.composite_rays_train_backward(*grads, _cuda(sig), _cuda(col), ts, rays, ws, dep, img, M, N, 1e-4, False, gs, gr)
        torch.cuda.synchronize()
        outs.append([xyzs, dirs, ts, rays, counter, w, ws, dep, img, gs, gr])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_empty_cases():
    rgb, lat = _mods()
    C, H = 2, 32
    _, bits, o, d, nears, fars = _scene(C, H, kind="empty", W=16)
    N = len(o)
    xyzs, dirs, ts, rays, counter = _march(rgb, _cuda(o), _cuda(d), _cuda(bits), C, H, _cuda(nears), _cuda(fars), torch.zeros(N, device="cuda"),
                                           False, 0.0, 1024)
    assert counter.item() == 0 and xyzs.shape[0] == 0 and int(rays.abs().sum()) == 0
    ws = torch.full((N,), 7.0, device="cuda"); dep = torch.full((N,), 7.0, device="cuda"); img = torch.full((N, 3), 7.0, device="cuda")
    e = torch.zeros(0, device="cuda")
    rgb.composite_rays_train_forward(e, torch.zeros(0, 3, device="cuda"), torch.zeros(0, 2, device="cuda"), rays, 0, N, 1e-4, False, e, ws,
                                     dep, img)
    assert float(ws.abs().sum() + dep.abs().sum() + img.abs().sum()) == 0.0
    gs = torch.zeros(0, device="cuda")
    rgb.composite_rays_train_backward(e, ws, dep, img, e, torch.zeros(0, 3, device="cuda"), torch.zeros(0, 2, device="cuda"), rays, ws, dep,
                                      img, 0, N, 1e-4, False, gs, torch.zeros(0, 3, device="cuda"))
    # N = 0
    z3 = torch.zeros(0, 3, device="cuda"); z = torch.zeros(0, device="cuda")
    r0 = torch.zeros(0, 2, dtype=torch.int32, device="cuda"); c0 = torch.zeros(1, dtype=torch.int32, device="cuda")
    rgb.march_rays_train(z3, z3, _cuda(bits), BOUND, False, 0.0, 1024, 0, C, H, z, z, None, None, None, r0, c0, z)
    assert c0.item() == 0
    lat.composite_rays_train_forward(z, torch.zeros(0, 4, device="cuda"), torch.zeros(0, 2, device="cuda"), r0, 0, 0, 1e-4, z, z, z,
                                     torch.zeros(0, 4, device="cuda"))
    rgb.near_far_from_aabb(z3, z3, _cuda(AABB), 0, 0.05, z, z)
    torch.cuda.synchronize()


@pytest.mark.slow
def test_full_size_512():
    """512^2 rays of one view at the recipe's grid (H=128, C=2): per-ray counts and samples of a random subset against the restatement,
    and the whole march + composite reproducible"""
    rgb, _ = _mods()
    C, H = 2, 128
    g, bits, o, d, nears, fars = _scene(C, H, W=512, seed=11)
    N = len(o)
    xyzs, dirs, ts, rays, counter = _march(rgb, _cuda(o), _cuda(d), _cuda(bits), C, H, _cuda(nears), _cuda(fars), torch.zeros(N, device="cuda"),
                                           False, 0.0, 1024)
    r = rays.cpu().numpy()
    assert counter.item() == r[:, 1].sum() > 100000
    sub = np.random.RandomState(0).choice(N, 3000, replace=False)
    sub.sort()
    cnt, rx, _, rt = rc.march_train(o[sub], d[sub], bits, BOUND, False, 0.0, 1024, C, H, nears[sub], fars[sub], np.zeros(len(sub), np.float32))
    assert np.array_equal(r[sub, 1], cnt)
    X, TS = xyzs.cpu().numpy(), ts.cpu().numpy()
    idx = np.concatenate([np.arange(r[n, 0], r[n, 0] + r[n, 1]) for n in sub])
    assert np.abs(X[idx] - rx).max() <= 1e-6 and np.abs(TS[idx] - rt).max() <= 1e-6
    x2 = _march(rgb, _cuda(o), _cuda(d), _cuda(bits), C, H, _cuda(nears), _cuda(fars), torch.zeros(N, device="cuda"), False, 0.0, 1024)
    assert torch.equal(x2[0], xyzs) and torch.equal(x2[3], rays)
