"""-m gpu: the shared-prefix denoiser plans (sd15.DenoiserPlan(shared_prefix=True)) against the plans that run the whole CFG batch.

The two entries of a view's CFG pair get the same noisy latents, timestep and condition image and differ only in their text, which both
networks first read in the cross-attention of down_blocks.0.attentions.0; a shared-prefix plan runs everything before that point on V rows
instead of 2 V.  The M of those GEMMs halves, which on its own would change tile and split-K choices and with them the order of the sums;
the builder therefore plans the V-row layers as the 2 V-row products they replace (dwg_gemm_desc.plan_m), and the two kinds of plan give
the same bits.  Both have to meet, against oracle/sd15.py on CPU fp32, the bars the plain plans already have: bf16 the bar
of tests/test_guidance_gpu.py (eps 3e-2, CFG difference 8e-2), f32x the bars of tests/test_sd15_f32x_gpu.py for the whole denoiser (eps 1e-4,
SDS gradient under CFG 50 5e-4).
Reduced-width configuration and latent_hw = 16 of tests/test_guidance_gpu.py; ONE oracle pass, shared by the tests."""
import pytest
import torch

pytestmark = pytest.mark.gpu

HW = 16


def _rel(a, r):
    a = a.detach().double().cpu(); r = r.detach().double().cpu()
    return float((a - r).norm() / r.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def case():
    from dreamwaltz_g_amd import sd15
    from oracle import sd15 as osd
    ucfg = sd15.UNetConfig(block_out_channels=(64, 128, 128, 128), cross_dim=64, cond_channels=(16, 32, 32, 64))
    usd = sd15.random_state_dict(sd15.unet_param_shapes(ucfg), seed=1)
    csd = sd15.random_state_dict(sd15.controlnet_param_shapes(ucfg), seed=2)
    g = torch.Generator().manual_seed(5)
    V = 2                                                        # two views: different latents, timesteps and condition images
    lat = torch.randn(V, 4, HW, HW, generator=g)
    text = torch.randn(2 * V, 77, ucfg.cross_dim, generator=g)   # [neg v0, neg v1 | text v0, text v1]
    cond = torch.rand(V, 3, 8 * HW, 8 * HW, generator=g)
    t = torch.tensor([437, 81])
    noise = torch.randn(1, 4, HW, HW, generator=g)
    # the oracle on view 0's CFG pair (the repeat of basic.py:570 written out)
    ref = osd.predict_noise(ucfg, usd, csd, lat[:1].repeat(2, 1, 1, 1), t[:1], torch.stack([text[0], text[V]]), cond[:1].repeat(2, 1, 1, 1))
    return dict(ucfg=ucfg, usd=usd, csd=csd, lat=lat, text=text, cond=cond, t=t, V=V, ref=ref, noise=noise)


def _pair(case, dtype):
    """(plain plan, shared-prefix plan) for one view on the same kernel-layout weights."""
    from dreamwaltz_g_amd import sd15
    dev = torch.device("cuda")
    plain = sd15.DenoiserPlan(case["ucfg"], case["usd"], case["csd"], dev, batch=2, latent_hw=HW, dtype=dtype)
    shared = sd15.DenoiserPlan(case["ucfg"], None, None, dev, batch=2, latent_hw=HW, dtype=dtype, weights=plain.weights, shared_prefix=True)
    assert all(a is b for a, b in zip(plain.weights, shared.weights))
    return plain, shared


def _view(case, v):
    V = case["V"]
    return (case["lat"][v:v + 1].cuda(), case["t"][v:v + 1].cuda(), torch.stack([case["text"][v], case["text"][V + v]]).cuda(),
            case["cond"][v:v + 1].cuda())


def _sds(eps2, noise):
    """(SDS gradient under CFG 50, CFG difference) of an eps pair, as tests/test_sd15_f32x_gpu.py forms them."""
    d = eps2[1] - eps2[0]
    return eps2[0] + 50.0 * d - noise[0], d


@pytest.mark.parametrize("dtype,bar_eps,what,bar2", [("bf16", 3e-2, "cfg", 8e-2), ("f32x", 1e-4, "sds", 5e-4)])
def test_both_kinds_of_plan_meet_the_oracle_bar(case, dtype, bar_eps, what, bar2):
    """The plain plan is fed the latents repeated, the shared-prefix plan the latents themselves.  Mutual difference of the two plans as
    measured on MI355X (relative L2 of eps): 0 for both bf16 and f32x, here and at SD-1.5's full width ("Measured: the shared CFG
    prefix"); eps against the oracle: 1.39e-2 bf16, 1.47e-6 f32x, for both plans."""
    plain, shared = _pair(case, dtype)
    lat, t, text, cond = _view(case, 0)
    ref = case["ref"]
    assert shared.latents.shape[0] == 1 and plain.latents.shape[0] == 2 and shared.eps.shape == plain.eps.shape
    plain.set_inputs(lat.repeat(2, 1, 1, 1), t, text, cond)
    a = plain.run().float().cpu().clone()
    shared.set_inputs(lat, t, text, cond)
    b = shared.run().float().cpu().clone()
    ea, eb = _rel(a, ref), _rel(b, ref)
    i = 0 if what == "sds" else 1           # bf16: the CFG difference itself (tests/test_guidance_gpu.py); f32x: the SDS gradient it feeds
    ca, cb = (_rel(_sds(x, case["noise"])[i], _sds(ref, case["noise"])[i]) for x in (a, b))
    print("[shared-prefix] %s: eps vs oracle plain %.3e shared %.3e | %s plain %.3e shared %.3e | mutual %.3e"
          % (dtype, ea, eb, what, ca, cb, _rel(b, a)))
    assert ea < bar_eps and eb < bar_eps, (ea, eb)
    assert ca < bar2 and cb < bar2, (what, ca, cb)
    assert not torch.equal(b[0], b[1])                          # the entries of the pair did see different text
    assert torch.equal(a, b)                                    # the shared rows are planned as the pair's: the same sums in the same order


def test_two_views_batched_equal_the_views_one_at_a_time(case):
    """B = 4 = [neg v0, neg v1 | text v0, text v1] with different latents, timesteps and condition images per view, against one single-view
    shared-prefix plan fed each view in turn (as tests/test_multiview_gpu.py compares the plain plans, at its bar): the smallest case in
    which the row order r V + v of the widening can go wrong."""
    from dreamwaltz_g_amd import sd15
    dev = torch.device("cuda")
    V = case["V"]
    one = sd15.DenoiserPlan(case["ucfg"], case["usd"], case["csd"], dev, batch=2, latent_hw=HW, dtype="f32x", shared_prefix=True)
    both = sd15.DenoiserPlan(case["ucfg"], None, None, dev, batch=2 * V, latent_hw=HW, dtype="f32x", views=V, weights=one.weights, shared_prefix=True)
    assert both.latents.shape[0] == V and both.eps.shape[0] == 2 * V
    both.set_inputs(case["lat"].cuda(), case["t"].cuda(), case["text"].cuda(), case["cond"].cuda())
    eps_b = both.run().clone()
    for v in range(V):
        one.set_inputs(*_view(case, v))
        e = one.run()
        en, et = _rel(eps_b[v], e[0]), _rel(eps_b[V + v], e[1])
        print("[shared-prefix] view %d: batched vs single, negative %.3e text %.3e" % (v, en, et))
        assert en < 2e-5 and et < 2e-5, (v, en, et)
    assert _rel(eps_b[0], eps_b[1]) > 1e-2 and _rel(eps_b[0], eps_b[V]) > 1e-4      # the views and the entries of a pair do differ


def test_captured_replay_equals_eager_bit_for_bit(case):
    from dreamwaltz_g_amd import sd15
    dev = torch.device("cuda")
    px = sd15.DenoiserPlan(case["ucfg"], case["usd"], case["csd"], dev, batch=2, latent_hw=HW, dtype="f32x", shared_prefix=True)
    px.set_inputs(*_view(case, 0))
    got = px.run().float().cpu().clone()
    with torch.cuda.stream(torch.cuda.Stream()):
        px.plan.capture()
        px.pre.capture()
        px.set_inputs(*_view(case, 1))                          # other inputs in between: the replay must read the buffers, not a recording
        px.run()
        px.set_inputs(*_view(case, 0))
        rep = px.run().float().cpu().clone()
    assert px.plan.graph is not None and torch.equal(rep, got)


def test_a_shared_prefix_plan_takes_one_latent_per_view(case):
    from dreamwaltz_g_amd import sd15
    dev = torch.device("cuda")
    lat, t, text, cond = _view(case, 0)
    px = sd15.DenoiserPlan(case["ucfg"], case["usd"], case["csd"], dev, batch=2, latent_hw=HW, dtype="f32x", shared_prefix=True)
    with pytest.raises(ValueError):
        px.set_inputs(lat.repeat(2, 1, 1, 1), t, text, cond)    # the CFG batch: its halves could differ
    px.set_inputs(lat, t, text, cond)
    with pytest.raises(ValueError):
        sd15.DenoiserPlan(case["ucfg"], None, None, dev, batch=2, latent_hw=HW, dtype="f32x", views=2, weights=px.weights, shared_prefix=True)
    with pytest.raises(NotImplementedError):
        sd15.DenoiserPlan(case["ucfg"], case["usd"], case["csd"], dev, batch=2, latent_hw=HW, dtype="f32", shared_prefix=True)


def test_a_prefix_convolution_is_planned_as_the_full_batch_product_bit_for_bit():
    """SD-1.5's first 3 x 3 convolutions (320 -> 320 at 64 x 64) are where the kernel choice depends on the row count: 8192 rows (the CFG pair)
    take the LDS-patch kernel, 4096 rows alone would take the im2col one, whose sums over K run in another order.  A shared-prefix builder
    plans its V-row layers as the 2 V-row products they replace (dwg_gemm_desc.plan_m), so the one image's rows are the pair's rows."""
    from dreamwaltz_g_amd import _lib, sd15, xfmt
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(11)
    sd = {"c.weight": torch.randn(320, 320, 3, 3, generator=g) / 54.0, "c.bias": 0.05 * torch.randn(320, generator=g)}
    w = sd15.Weights(sd, dev, "f32x")
    x = torch.randn(1, 64, 64, 320, generator=g)
    outs, names = [], []
    for batch, full in ((2, None), (1, 2), (1, None)):
        plan = sd15.Plan(dev, "f32x")
        b = sd15.Builder(plan, w, 32, "t")
        b.full_batch = full
        xb = plan.buf(batch, 64, 64, 320)
        y = b.conv(xb, "c")
        plan.store(xb, x.repeat(batch, 1, 1, 1).to(dev))
        _lib.prof_enable(True)
        plan.run_eager()
        torch.cuda.synchronize()
        names.append(set(_lib.prof_symbols())); _lib.prof_enable(False)
        outs.append(y.clone())
    assert torch.equal(outs[0][0], outs[0][1]) and torch.equal(outs[1][0], outs[0][0])
    assert names[0] == names[1], (names[0], names[1])            # the same kernel ...
    assert names[2] != names[0]                                  # ... which is not what 4096 rows take on their own
    assert _rel(xfmt.unpack(outs[2].cpu()), xfmt.unpack(outs[1].cpu())) < 1e-5
