"""Restatement of the NeRF stage's field network (boundary B7) for the tests of dreamwaltz_g_amd.nerf.

  restate(...)        float64 torch: (x + bound) / (2 bound) -> grid encoding (oracle.animate.grid_encode) -> sigma_net -> density
                      activation + prior / albedo postprocess, differentiable in the table, weights, biases and sigma_scale.
                      The cell positions and interpolation weights are evaluated in fp32 as every grid kernel does.
                      f16=True rounds where the reference rounds under fp16 autocast: the table read as fp16, the encoding, the
                      weights and every layer's output.
  _NeRFNetwork        a test-local module with the reference's attribute and parameter names (encoder.embeddings, sigma_net.net.{i},
                      sigma_scale, opt, density_prior_type, latent_mode, bound, decoder_layer) and the reference's common_forward /
                      local_geometry_forward / density / forward written in torch ops (nerf_model.py:38-64, 66-110, 268-295) on the
                      package's GridEncoder: the composition a bound user runs without the fused kernel.
"""
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import animate as oa

BOUND = 2.0


def grid_params(L=16, gridtype='tiled', log2_hashmap_size=19, base_resolution=16, desired_resolution=2048 * BOUND, align_corners=False):
    """offsets and per_level_scale exactly as GridEncoder.__init__ computes them."""
    per_level_scale = float(np.exp2(np.log2(desired_resolution / base_resolution) / (L - 1))) if L > 1 else 2.0
    offsets, off = [], 0
    for i in range(L):
        res = int(np.ceil(base_resolution * per_level_scale ** i))
        n = min(2 ** log2_hashmap_size, (res if align_corners else res + 1) ** 3)
        n = int(np.ceil(n / 8) * 8)
        offsets.append(off)
        off += n
    offsets.append(off)
    return np.array(offsets, np.int64), per_level_scale


class MLP(nn.Module):
    """nerf_model.py:12-33 (Linear + ReLU, the last layer without)."""

    def __init__(self, dim_in, dim_out, dim_hidden, num_layers):
        super().__init__()
        self.net = nn.ModuleList([nn.Linear(dim_in if l == 0 else dim_hidden, dim_out if l == num_layers - 1 else dim_hidden)
                                  for l in range(num_layers)])

    def forward(self, x):
        for l, lin in enumerate(self.net):
            x = lin(x)
            if l != len(self.net) - 1:
                x = F.relu(x, inplace=True)
        return x


class _TruncExp(torch.autograd.Function):
    """nerf_utils.py:180-191."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        x = ctx.saved_tensors[0]
        return g * torch.exp(x.clamp(-15, 15))


trunc_exp = _TruncExp.apply


class _NeRFNetwork(nn.Module):
    def __init__(self, encoder, num_layers=3, hidden_dim=64, density_activation='exp', density_prior='none', latent_mode=False,
                 additional_dim_size=0, bound=BOUND):
        super().__init__()
        self.encoder = encoder
        self.in_dim = encoder.output_dim
        self.bound = bound
        self.opt = types.SimpleNamespace(density_activation=density_activation, density_prior=density_prior)
        self.sigma_net = MLP(self.in_dim, 4 + additional_dim_size, hidden_dim, num_layers)
        self.sigma_scale = nn.Parameter(torch.tensor(0.0))
        self.density_prior_type = density_prior
        self.latent_mode = latent_mode
        self.decoder_layer = None
        if density_activation == 'exp':
            self.density_activation = trunc_exp
        elif density_activation == 'softplus':
            self.density_activation = F.softplus
        else:
            def act(x, density_shift=-1.0):
                x = x * torch.exp(self.sigma_scale)
                return F.softplus(x + density_shift)
            self.density_activation = act

    def density_prior(self, x):
        if self.density_prior_type == 'none':
            return 0.0
        d = (x ** 2).sum(-1)
        if self.density_prior_type == 'gaussian':
            return 5 * torch.exp(-d / (2 * 0.2 ** 2))
        return 10 * (1 - torch.sqrt(d) / 0.5)

    def postprocess(self, inputs):
        return inputs if self.latent_mode else torch.sigmoid(inputs)

    def density(self, x):
        sigma, albedo = self.common_forward(x)
        return {'sigma': sigma, 'albedo': albedo}

    def forward(self, x, d, l=None, ratio=1, shading='albedo'):
        sigma, albedo = self.common_forward(x)
        assert shading == 'albedo'
        return sigma, albedo

    def local_geometry_forward(self, x, mlp_no_grad=False):
        enc = self.encoder(x, bound=self.bound)
        if mlp_no_grad:
            requires_grad = next(self.sigma_net.parameters()).requires_grad
            self.sigma_net.requires_grad_(False)
        h = self.sigma_net(enc)
        sigma, albedo = h[..., 0], h[..., 1:]
        albedo = self.postprocess(albedo)
        if mlp_no_grad:
            self.sigma_net.requires_grad_(requires_grad)
        return sigma, albedo

    def common_forward(self, x, mask=None, return_raw=False, **kwargs):
        enc = self.encoder(x, bound=self.bound)
        h = self.sigma_net(enc)
        sigma, albedo = h[..., 0], h[..., 1:]
        if return_raw:
            return sigma, albedo
        sigma = self.density_activation(sigma + self.density_prior(x))
        if mask is not None:
            sigma *= mask
        albedo = self.postprocess(albedo)
        return sigma, albedo


def make_network(L=16, gridtype='tiled', interp='smoothstep', num_layers=3, hidden=64, density_activation='exp', density_prior='none',
                 latent_mode=False, additional_dim_size=0, seed=0, log2_hashmap_size=19, table_scale=0.5, sigma_scale=0.3):
    """A _NeRFNetwork on the package's GridEncoder (CPU) with non-trivial random parameters."""
    from dreamwaltz_g_amd.gridencoder import GridEncoder
    enc = GridEncoder(input_dim=3, num_levels=L, level_dim=2, base_resolution=16, log2_hashmap_size=log2_hashmap_size,
                      desired_resolution=2048 * BOUND, gridtype=gridtype, interpolation=interp)
    net = _NeRFNetwork(enc, num_layers, hidden, density_activation, density_prior, latent_mode, additional_dim_size)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        enc.embeddings.copy_((torch.rand(enc.embeddings.shape, generator=g) * 2 - 1) * table_scale)
        for lin in net.sigma_net.net:
            k = lin.in_features
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * (2.0 / k) ** 0.5)
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * 0.1)
        net.sigma_scale.fill_(sigma_scale)
    return net


def make_points(M, seed=0, edge=True, bound=BOUND):
    """[M, 3] fp32 in [-bound, bound]; with `edge`, some rows on +-bound exactly and some just outside it."""
    r = np.random.RandomState(seed)
    x = ((r.rand(M, 3) * 2 - 1) * bound * 0.9).astype(np.float32)
    if edge and M >= 8:
        k = max(1, M // 16)
        idx = r.choice(M, size=min(M, 4 * k), replace=False)
        on, out = idx[:k], idx[k:2 * k]
        x[on, r.randint(0, 3, size=len(on))] = np.float32(bound) * np.where(r.rand(len(on)) < 0.5, -1, 1).astype(np.float32)
        x[out, r.randint(0, 3, size=len(out))] = np.nextafter(np.float32(bound), np.float32(10)) * np.where(r.rand(len(out)) < 0.5, -1, 1).astype(np.float32)
    return x


def _r16(t):
    return t.to(torch.float16).to(t.dtype)


def restate(net, x, raw=False, albedo_sigmoid=None, f16=False):
    """float64 (sigma, albedo) of `net` at x (fp32 [M, 3]); differentiable in net's parameters through the float64 leaves returned:
    (sigma, albedo, leaves) with leaves = {'embeddings', 'sigma_scale', 'w0', 'b0', ...}."""
    enc_m = net.encoder
    leaves = {'embeddings': enc_m.embeddings.detach().double().cpu().requires_grad_(True),
              'sigma_scale': net.sigma_scale.detach().double().cpu().reshape(()).requires_grad_(True)}
    for l, lin in enumerate(net.sigma_net.net):
        leaves['w%d' % l] = lin.weight.detach().double().cpu().requires_grad_(True)
        leaves['b%d' % l] = lin.bias.detach().double().cpu().requires_grad_(True)
    xf = torch.as_tensor(x, dtype=torch.float32).cpu()
    b = np.float32(net.bound)
    # torch's fp32 (x + bound) / (2 bound); kept in fp32, so that the lookup's cell positions and weights are the fp32 ones the grid kernels
    # (the reference's and this package's) compute -- everything after them is float64
    xn = (xf + b) * (np.float32(1.0) / (np.float32(2.0) * b))
    table = leaves['embeddings']
    if f16:
        table = _r16(table)
    h = oa.grid_encode(xn, table, enc_m.offsets.cpu().numpy().astype(np.int64), enc_m.per_level_scale, enc_m.base_resolution,
                       gridtype=enc_m.gridtype_id, align_corners=enc_m.align_corners, interp=enc_m.interp_id)
    n = len(net.sigma_net.net)
    for l in range(n):
        if f16:
            h = _r16(h)
        w = leaves['w%d' % l]
        h = F.linear(h, _r16(w) if f16 else w, leaves['b%d' % l])
        if f16:
            h = _r16(h)
        if l != n - 1:
            h = F.relu(h)
    sigma, albedo = h[:, 0], h[:, 1:]
    sig = (not net.latent_mode) if albedo_sigmoid is None else albedo_sigmoid
    if sig:
        albedo = torch.sigmoid(albedo)
    if not raw:
        x64 = xf.double()
        s = sigma
        if net.density_prior_type != 'none':
            d = (x64 ** 2).sum(-1)
            s = s + (5 * torch.exp(-d / 0.08) if net.density_prior_type == 'gaussian' else 10 * (1 - torch.sqrt(d) / 0.5))
        act = net.opt.density_activation
        if act == 'exp':
            sigma = torch.exp(s)
        elif act == 'softplus':
            sigma = F.softplus(s)
        else:
            sigma = F.softplus(s * torch.exp(leaves['sigma_scale']) - 1.0)
    return sigma, albedo, leaves


def rel_err(a, ref):
    """max |a - ref| / max |ref| (float64)."""
    a = torch.as_tensor(a).detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu()
    return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-30)) if ref.numel() else 0.0


def rel_l2(a, ref):
    a = torch.as_tensor(a).detach().double().cpu().reshape(-1)
    ref = torch.as_tensor(ref).detach().double().cpu().reshape(-1)
    return float((a - ref).norm() / ref.norm().clamp_min(1e-30))
