"""Restatements for the tests of the shaded one-launch inference render (boundary B15, dreamwaltz_g_amd.nerf_render with shading
'normal' / 'textureless' / 'lambertian').  Imports nothing of the reference.

  _NeRFNetwork        nerf_render_cases' stand-in with the reference's forward and normal (core/nerf/nerf_model.py:74-105, 146-169) over
                      self.common_forward.  Its inherited run_cuda is then THE COMPOSITION a bound network ran for a shaded view before
                      the native render: per loop iteration march_rays, seven launches of the fused field, the torch statements of the
                      normal and the shading, composite_rays.
  make_shading_network(...)  nerf_render_cases.make_render_network with that class
  face_rays(...)      the 96 crafted rays that run just inside the six faces of the box: the clamp of the shifted points is active on
                      every sample
  composited(...)     which samples of the composition's records were composited (the walk of nerf_render_cases.trace)
  shading_fairness(...)  the share of composited samples with a non-zero normal ('normal' records) or lit / unlit ('textureless' records)
  compare(...)        nerf_render_cases.compare for weights_sum, depth and counts as it stands, and the image within
                      (S + 2 + 16) 2^-23 max(1, max |rgbs|)
  exact_normal_image(...)  float64 restatement of the 'normal' view through nerf_field_cases.restate (information only)
"""
import numpy as np
import torch

from tests import nerf_field_cases as nc
from tests import nerf_render_cases as rc
from tests import raymarch_cases as rmc

f32 = np.float32
IMAGE_EXTRA_ULPS = 16       # see compare()
AMBIENT = 0.1               # at the default 1.0 the lambert term is the constant 1 and tests nothing


class _NeRFNetwork(rc._NeRFNetwork):
    """The stand-in carries the reference's class name: nerf.unbound_reason binds the shared-MLP structure by it."""

    def forward(self, x, d, l=None, ratio=1, shading='albedo'):
        sigma, albedo = self.common_forward(x)
        if shading == 'albedo':
            color = albedo
        else:
            normal = self.normal(x)
            if shading == 'normal':
                color = (normal + 1.0) / 2.0
            else:
                lambertian = ratio + (1 - ratio) * (normal @ -l).clamp(min=0)
                if shading == 'textureless':
                    color = lambertian.unsqueeze(-1).repeat(1, 3)
                elif shading == 'lambertian':
                    color = albedo * lambertian.unsqueeze(-1)
                else:
                    assert 0, shading
            if self.latent_mode:
                color = torch.cat([color, torch.zeros((color.shape[0], 1), device=color.device)], axis=1)
        return sigma, color

    def normal(self, x, normal_type='finite_difference_laplacian', epsilon=1e-3):
        assert normal_type == 'finite_difference_laplacian', normal_type
        dx_pos, _ = self.common_forward((x + torch.tensor([[epsilon, 0.00, 0.00]], device=x.device)).clamp(-self.bound, self.bound))
        dx_neg, _ = self.common_forward((x + torch.tensor([[-epsilon, 0.00, 0.00]], device=x.device)).clamp(-self.bound, self.bound))
        dy_pos, _ = self.common_forward((x + torch.tensor([[0.00, epsilon, 0.00]], device=x.device)).clamp(-self.bound, self.bound))
        dy_neg, _ = self.common_forward((x + torch.tensor([[0.00, -epsilon, 0.00]], device=x.device)).clamp(-self.bound, self.bound))
        dz_pos, _ = self.common_forward((x + torch.tensor([[0.00, 0.00, epsilon]], device=x.device)).clamp(-self.bound, self.bound))
        dz_neg, _ = self.common_forward((x + torch.tensor([[0.00, 0.00, -epsilon]], device=x.device)).clamp(-self.bound, self.bound))
        normal = - 0.5 * torch.stack([(dx_pos - dx_neg), (dy_pos - dy_neg), (dz_pos - dz_neg)], dim=-1) / epsilon
        normal = normal / torch.sqrt(torch.clamp(torch.sum(normal * normal, -1, keepdim=True), min=1e-20))      # safe_normalize
        normal = torch.nan_to_num(normal)
        return normal


def make_shading_network(grid_size, bound, density_prior='gaussian', latent=False, seed=3, **encoder_kw):
    """nerf_render_cases.make_render_network's network (same parameters, same seed) as a _NeRFNetwork of this module."""
    src = rc.make_render_network(grid_size, bound, density_prior=density_prior, latent=latent, seed=seed, **encoder_kw)
    kw = dict(density_activation='exp', density_prior=density_prior, latent_mode=latent, additional_dim_size=1 if latent else 0)
    net = _NeRFNetwork(src.encoder, grid_size=grid_size, bound=bound, **kw)
    net.sigma_net.load_state_dict(src.sigma_net.state_dict())
    with torch.no_grad():
        net.sigma_scale.copy_(src.sigma_scale)
    return net


def face_rays(seed=0, per_face=16, depth=5e-4):
    """Rays parallel to each of the six faces of the box [-1, 1]^3, at depth * u (u uniform in [0, 1)) inside it: origin -2 along one
    in-plane axis, direction +1 along it, the other in-plane coordinate uniform in +-0.8.  -> rays_o, rays_d [6 per_face, 3] fp32 and
    face [6 per_face] (2 axis + (0 for the + face, 1 for the - face))."""
    rng = np.random.RandomState(seed)
    o, d, face = [], [], []
    for axis in range(3):
        for neg in range(2):
            for _ in range(per_face):
                b, c = (axis + 1) % 3, (axis + 2) % 3
                oo, dd = np.zeros(3), np.zeros(3)
                oo[axis] = (1.0 - depth * rng.uniform()) * (-1.0 if neg else 1.0)
                oo[b], dd[b] = -2.0, 1.0
                oo[c] = rng.uniform(-0.8, 0.8)
                o.append(oo); d.append(dd); face.append(2 * axis + neg)
    return np.asarray(o, f32), np.asarray(d, f32), np.asarray(face)


def face_check(o, d, face, bits, C=1, H=16, bound=1.0, max_steps=64, eps=1e-3):
    """The CPU march of the face rays: samples per ray, and per face the number of samples on which the clamp of a shifted point is
    active (the coordinate normal to the face lies within eps of it)."""
    b = f32(bound)
    near, far = rmc.near_far(o, d, [-b, -b, -b, b, b, b], 0.2)
    counts, xyzs, _, _ = rmc.march_train(o, d, bits, bound, False, 0.0, max_steps, C, H, near, far, np.zeros(len(o), f32))
    owner = np.repeat(np.arange(len(o)), counts)
    axis = face[owner] // 2
    active = np.abs(xyzs[np.arange(len(xyzs)), axis]).astype(f32) + f32(eps) > b
    return counts, np.bincount(face[owner][active], minlength=6), int(active.sum()), len(xyzs)


def composited(records, N, T_thresh=rc.T_THRESH):
    """Per record a bool [n_alive, n_step]: the sample was composited (nerf_render_cases.trace's walk)."""
    ws = np.zeros(N, f32)
    tt = f32(T_thresh)
    out = []
    for rec in records:
        alive, n_step = rec["rays_alive"].astype(np.int64), rec["n_step"]
        ts = rec["ts"].reshape(len(alive), n_step, 2).astype(f32)
        sig = rec["sigmas"].reshape(len(alive), n_step).astype(f32)
        act = np.ones(len(alive), bool)
        m = np.zeros((len(alive), n_step), bool)
        for s in range(n_step):
            act &= ts[:, s, 0] != 0
            m[act, s] = True
            i = alive[act]
            a = f32(1) - np.exp(-(sig[act, s] * ts[act, s, 1]))
            T = f32(1) - ws[i]
            ws[i] = ws[i] + a * T
            act[np.nonzero(act)[0][T < tt]] = False
        out.append(m)
    return out


def shading_fairness(records, N, shading, ratio=AMBIENT):
    """From the composition's records of a 'normal' view: the share of composited samples whose normal is not zero (colour != 0.5).  Of a
    'textureless' view: the shares lit (lambert term above the ambient ratio) and unlit."""
    masks = composited(records, N)
    rgb = np.concatenate([r["rgbs"].reshape(m.shape + (-1,))[m] for r, m in zip(records, masks)]) if records else np.zeros((0, 3), f32)
    n = max(len(rgb), 1)
    if shading == 'normal':
        return {"samples": len(rgb), "nonzero_normal": float((rgb[:, :3] != f32(0.5)).any(-1).sum()) / n}
    lit = rgb[:, 0] > f32(ratio)
    return {"samples": len(rgb), "lit": float(lit.sum()) / n, "unlit": float((~lit).sum()) / n}


def assert_shading_fair(fair):
    if "nonzero_normal" in fair:
        assert fair["nonzero_normal"] >= 0.9, fair
    else:
        assert fair["lit"] >= 0.25 and fair["unlit"] >= 0.25, fair


def compare(native, composed, tr, mask, fars, records, T_thresh=rc.T_THRESH):
    """nerf_render_cases.compare on weights_sum, depth and counts as it stands (the image slot filled with the composition's own, so
    that B14's rule judges the geometry alone), then the image: on non-borderline rays within (S + 2 + 16) 2^-23 max(1, max |rgbs|), on
    borderline rays B14's T_thresh scale.

    The 16 is derived, not measured.  The seven densities of a sample are the same field_tile arithmetic on the same fp32 points in
    both paths, so they are equal bit for bit.  What may differ is torch's rule for the division by the scalar epsilon (a product with
    the rounded inverse), the order of its three-term sum in the normalisation, the three-term dot product of the matmul, the lambert
    term and the albedo product: a handful of roundings on components of magnitude at most 1, under 16 ulps of 1 per sample colour,
    and the weights of a ray sum to at most 1.  Returns the figures."""
    ws, dep, img, cnt = (np.asarray(a) for a in native)
    ws0, dep0, img0 = (np.asarray(a) for a in composed)
    fig = rc.compare((ws, dep, img0, cnt), composed, tr, mask, fars, records, T_thresh)
    N = len(ws)
    rgb_max = max([float(np.abs(r["rgbs"]).max()) for r in records if r["rgbs"].size] or [0.0])
    s_img = max(1.0, rgb_max)
    border = tr["margin"] <= rc.BORDER
    S = tr["count"].astype(np.float64)
    err = np.abs(img.astype(np.float64) - img0).max(-1) / s_img if N else np.zeros(0)
    bound = (S + 2 + IMAGE_EXTRA_ULPS) * rc.ULP
    fig["bit_equal"] = int(((ws == ws0) & (dep == dep0) & (img == img0).all(-1) & (cnt == tr["count"])).sum())
    fig["max_err_over_bound"]["image"] = float((err[~border] / bound[~border]).max()) if (~border).any() else 0.0
    fig["max_err_borderline"]["image"] = float(err[border].max()) if border.any() else 0.0
    print("nerf_shading parity:", fig)
    assert (err[~border] <= bound[~border]).all(), fig
    assert (err[border] <= T_thresh).all(), fig
    return fig


def exact_normal_image(net, o, d, bits, bound, C, H, counts, max_steps=rc.MAX_STEPS, eps=1e-3):
    """The 'normal' view with the field in float64 (nerf_field_cases.restate) at the seven fp32 points of every sample and the normal,
    the shading and the composite in float64, over the first counts[n] samples of ray n of raymarch_cases' numpy march.  -> image [N, 3].
    How far fp32 finite differences of the density sit from the exact ones; no bound for it is derived anywhere."""
    b = f32(bound)
    near, far = rmc.near_far(o, d, [-b, -b, -b, b, b, b], 0.2)
    cnt, xyzs, _, ts = rmc.march_train(o, d, bits, bound, False, 0.0, max_steps, C, H, near, far, np.zeros(len(o), f32))
    xyzs = xyzs.astype(f32)
    with torch.no_grad():
        def sigma(x):
            return nc.restate(net, x)[0].double().numpy()
        s0 = sigma(xyzs)
        g = np.zeros((len(xyzs), 3))
        for a in range(3):
            sh = np.zeros(3, f32)
            sh[a] = f32(eps)
            g[:, a] = -0.5 * (sigma(np.clip(xyzs + sh, -b, b)) - sigma(np.clip(xyzs - sh, -b, b))) / eps
    n = g / np.sqrt(np.maximum((g * g).sum(-1, keepdims=True), 1e-20))
    rgb = (np.nan_to_num(n) + 1.0) / 2.0
    off = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    img = np.zeros((len(o), 3))
    for r in range(len(o)):
        ws = 0.0
        for i in range(off[r], off[r] + min(int(cnt[r]), int(counts[r]))):
            w = (1.0 - np.exp(-s0[i] * float(ts[i, 1]))) * (1.0 - ws)
            ws += w
            img[r] += w * rgb[i]
    return img
