"""-m gpu: fused HIP Adam on the flat parameter buffer vs torch.optim.Adam (same hyper-parameters, eps 1e-15)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_flat_adam_matches_torch_adam():
    from dreamwaltz_g_amd import optim
    torch.manual_seed(0)
    dev = torch.device("cuda")
    shapes = [(1000, 3), (17,), (64, 95), (5, 5, 5)]
    ps = [torch.nn.Parameter(torch.randn(s, device=dev)) for s in shapes]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt_ref = torch.optim.Adam([dict(params=ref[:2], lr=1e-3), dict(params=ref[2:], lr=1e-2, betas=(0.9, 0.99))], eps=1e-15)
    opts = optim.build_flat_optimizers({"a": optim.AdamSpec([dict(params=ps[:2], lr=1e-3)], eps=1e-15),
                                        "b": optim.AdamSpec([dict(params=ps[2:], lr=1e-2)], betas=(0.9, 0.99), eps=1e-15)}, dev)
    opts.set_grad_scale(0.5)
    for it in range(5):
        gs = [torch.randn(s, device=dev) * (it + 1) for s in shapes]
        for o in opts.values():
            o.zero_grad()
        for p, g, r in zip(ps, gs, ref):
            p.grad.copy_(g * 2.0)          # "sum over 2 ranks"; Adam applies grad_scale = 1/2
            r.grad = g.clone()
        for o in opts.values():
            o.step()
        opt_ref.step()
        for p, r in zip(ps, ref):
            assert torch.allclose(p.data, r.data, rtol=2e-5, atol=2e-6), float((p.data - r.data).abs().max())


def test_one_launch_for_all_groups_equals_one_launch_per_group():
    """dwg_adam_step_groups_dev (round 6: every group of every named optimizer of the captured step in one launch) against the per-group
    device-scalar launches it replaces (FlatOptimizer.launch_step): identical bits in parameters and both moments."""
    from dreamwaltz_g_amd import optim

    def build():
        torch.manual_seed(3)
        dev = torch.device("cuda")
        shapes = [(1000, 3), (17,), (64, 95), (5, 5, 5), (4096, 2)]
        ps = [torch.nn.Parameter(torch.randn(s, device=dev)) for s in shapes]
        opts = optim.build_flat_optimizers({"a": optim.AdamSpec([dict(params=ps[:2], lr=1e-3), dict(params=ps[2:3], lr=3e-3)], eps=1e-15),
                                            "b": optim.AdamSpec([dict(params=ps[3:], lr=1e-2)], betas=(0.9, 0.99), eps=1e-15)}, dev)
        opts.set_grad_scale(0.5)
        return ps, opts
    outs = []
    for fused in (False, True):
        ps, opts = build()
        rows = sum(len(o.param_groups) for o in opts.values())
        hyper_host = torch.zeros(rows, 4)
        hyper_dev = torch.zeros(rows, 4, device="cuda")
        for it in range(3):
            opts.zero_grad()
            g = torch.Generator(device="cuda").manual_seed(100 + it)
            opts.buffers.grad.copy_(torch.randn(opts.buffers.grad.shape, device="cuda", generator=g))
            base = 0
            for o in opts.values():
                base += o.prepare_step(hyper_host, base)
            hyper_dev.copy_(hyper_host)
            if fused:
                opts.launch_steps(hyper_dev)
            else:
                base = 0
                for o in opts.values():
                    base += o.launch_step(hyper_dev, base)
        torch.cuda.synchronize()
        outs.append((opts.buffers.flat.clone(), opts.buffers.m.clone(), opts.buffers.v.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


FOUR_PATH_SIZES = (1, 3, 4, 5, 1021, 2 * 2048 * 256 * 4 + 5)        # the last: two passes of the capped grid and a tail
FOUR_PATHS = ("dwg_adam_step", "dwg_adam_step_dev", "dwg_adam_step_groups_dev", "dwg_adam_step_groups_scaled_dev")


def four_path_inputs(n, steps=3):
    """(p0 [n], grads [steps][n]) of one group, and (p0, grads) of the 4-element group that goes in front of it in the grouped calls."""
    gen = torch.Generator(device="cuda").manual_seed(11 + n % 1000)

    def draw(k):
        return torch.randn(k, device="cuda", generator=gen), [torch.randn(k, device="cuda", generator=gen) * (i + 1) for i in range(steps)]
    return draw(n), draw(4)


def run_adam_path(path, inputs, skip=0.0):
    """The group's (p, m, v) after one step per gradient through the C entry point `path`, from p0 and zero moments.  Every path gets the
    same scalars: the eager entry point forms them itself from (lr, betas, t, grad_scale); the others read the row that
    FlatOptimizer.prepare_step writes for the same values.  The grouped paths run the group SECOND in a two-group call, behind a
    4-element group with a row of its own (row 1, never skipped): blockIdx.y and the short group's surplus workgroups matter.  `skip` goes
    into the fourth float of the group's row."""
    import ctypes
    from dreamwaltz_g_amd import _lib, optim
    lr, betas, eps, grad_scale = 3e-3, (0.9, 0.99), 1e-15, 0.5
    (p0, grads), (q0, qgrads) = inputs
    n = p0.numel()
    L, st = _lib.lib(), _lib.stream(p0.device)
    p, m, v, g = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), torch.empty_like(p0)
    q, qm, qv, qg = q0.clone(), torch.zeros_like(q0), torch.zeros_like(q0), torch.empty_like(q0)
    host = optim.build_flat_optimizers({"a": optim.AdamSpec([dict(params=[torch.nn.Parameter(torch.zeros(4))], lr=lr)], betas=betas, eps=eps)},
                                       "cpu")["a"]
    host.grad_scale = grad_scale
    table, hyper = torch.zeros(2, 4), torch.zeros(2, 4, device="cuda")
    for t, (gt, qgt) in enumerate(zip(grads, qgrads), 1):
        g.copy_(gt); qg.copy_(qgt)
        host.prepare_step(table, 0)
        table[1, :3] = table[0, :3]          # the front group's row: the same scalars, its fourth float stays 0
        table[0, 3] = skip
        hyper.copy_(table)
        if path == "dwg_adam_step":
            rc = L.dwg_adam_step(n, _lib.ptr(p), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), lr, betas[0], betas[1], eps, t, grad_scale, st)
        elif path == "dwg_adam_step_dev":
            rc = L.dwg_adam_step_dev(n, _lib.ptr(p), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), _lib.ptr(hyper), betas[0], betas[1], eps, st)
        else:
            arr = (_lib.AdamGroupC * 2)(_lib.AdamGroupC(q.data_ptr(), qg.data_ptr(), qm.data_ptr(), qv.data_ptr(), 4, betas[0], betas[1], eps, 1),
                                        _lib.AdamGroupC(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, betas[0], betas[1], eps, 0))
            rc = getattr(L, path)(2, arr, _lib.ptr(hyper), st)
        _lib.check(rc, path)
    torch.cuda.synchronize()
    return {"p": p, "m": m, "v": v, "q": q, "qm": qm, "qv": qv}


@pytest.mark.parametrize("n", FOUR_PATH_SIZES)
def test_four_entry_points_write_identical_bits(n):
    """dwg_adam_step, dwg_adam_step_dev, dwg_adam_step_groups_dev and dwg_adam_step_groups_scaled_dev are one update statement and one loop
    (csrc/adam_math.h adam_update, csrc/adam.hip adam_span): given identical scalars they leave identical bits in the parameters and both
    moments after three steps -- for a lone float, the sizes around a float4, an odd size, and one that takes more than one pass of the
    capped grid plus a tail.  A row whose skip flag is set leaves the scaled launch's group untouched."""
    inputs = four_path_inputs(n)
    outs = {path: run_adam_path(path, inputs) for path in FOUR_PATHS}
    first = outs[FOUR_PATHS[0]]
    assert not torch.equal(first["p"], inputs[0][0]) and first["m"].abs().sum() > 0 and first["v"].abs().sum() > 0
    for path in FOUR_PATHS[1:]:
        for key in ("p", "m", "v"):
            assert torch.equal(outs[path][key], first[key]), (path, key, n)
    # the short group in front took the same steps in both grouped launches
    for key in ("q", "qm", "qv"):
        assert torch.equal(outs[FOUR_PATHS[2]][key], outs[FOUR_PATHS[3]][key]), key
    assert not torch.equal(outs[FOUR_PATHS[2]]["q"], inputs[1][0])
    skipped = run_adam_path(FOUR_PATHS[3], inputs, skip=1.0)
    assert torch.equal(skipped["p"], inputs[0][0]) and not skipped["m"].any() and not skipped["v"].any()
    assert torch.equal(skipped["q"], outs[FOUR_PATHS[3]]["q"])                         # ... and only that group


def test_segment_copies_and_adds():
    """dwg_copy_segments / dwg_add_segments through their Python users: row merges (optionally normalised like the grid encoder's input) and
    the packed deformation heads whose gradients are added straight into flat-buffer slices."""
    from dreamwaltz_g_amd import assemble as asm
    g = torch.Generator().manual_seed(1)
    a = [torch.randn(n, 3, generator=g).cuda().requires_grad_(True) for n in (100, 7, 33)]
    b = [torch.randn(n, 4, generator=g).cuda().requires_grad_(True) for n in (100, 7, 33)]
    ca, cb = asm.concat_rows([a, b])
    assert torch.equal(ca, torch.cat(a, 0)) and torch.equal(cb, torch.cat(b, 0))
    (cn,) = asm.concat_rows([a], bound=1.5)
    assert torch.equal(cn, (torch.cat(a, 0) + 1.5) / (2 * 1.5))
    w = torch.randn(140, 3, generator=g).cuda()
    (cn * w).sum().backward()
    off = 0
    for t in a:
        assert torch.equal(t.grad, w[off:off + t.shape[0]] / 3.0)
        off += t.shape[0]
