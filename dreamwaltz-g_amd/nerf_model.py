"""The stage-I (NeRF) model without the reference (boundary B20): the shared-MLP _NeRFNetwork of core/nerf/nerf_model.py:214-329 on
the package's own pieces.

  NeRFNetwork(cfg, device)   gridencoder.GridEncoder + sigma_net (biased nn.Linear layers in `.net`, what pointcloud.field_spec reads)
                             + sigma_scale + occupancy.OccupancyGrid, and the render state of _NeRFRenderer.__init__
                             (nerf_renderer.py:25-77): aabb_train / aabb_infer, step_counter / local_step, bg_mode, bg_colors, img_dims
      .common_forward / .local_geometry_forward   nerf.nerf_field (B7)
      .update_extra_state                         OccupancyGrid.update (B13) + the reference's step-counter statements
      .render                                     nerf_view.render_view (B20 over B14 / B15 / B18 / B19)
      .get_optimizer(cfg)                         the flat fused Adam of optim.build_flat_optimizers
  BackgroundNeRFNetwork(cfg, device)   NeRFNetwork with the learned background (bg_mode 'nerf', boundary B22): encoder_bg
                             (nerf_background.FreqEncoder(3, 6)) + bg_net, rendered through nerf_background.learned_background, and a
                             'bg_net' group at cfg.bg_lr in the same flat Adam
  build_nerf_network(cfg, device)      the class cfg.bg_mode asks for, as the reference's build_NeRFNetwork picks its class

Covered: structure 'shared_mlp', backbone 'tiledgrid' / 'hashgrid', nerf_type 'rgb' / 'latent', cuda_ray, optimizer 'adam' with
lr_policy 'constant' / 'none'.  dmtet, run() without cuda_ray, the other optimizers and the learning-rate schedulers are refused by
name; NeRFNetwork itself refuses the learned 'nerf' background (BackgroundNeRFNetwork builds it).
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import nerf
from . import nerf_background
from . import nerf_view
from . import occupancy
from . import optim
from . import raymarch
from .gridencoder import GridEncoder

BACKBONES = {'tiledgrid': 'tiled', 'hashgrid': 'hash'}


class MLP(nn.Module):
    """nerf_model.py:12-33: Linear + ReLU, the last layer without."""

    def __init__(self, dim_in, dim_out, dim_hidden, num_layers, bias=True):
        super().__init__()
        self.dim_in, self.dim_out, self.dim_hidden, self.num_layers = dim_in, dim_out, dim_hidden, num_layers
        self.net = nn.ModuleList([nn.Linear(dim_in if l == 0 else dim_hidden, dim_out if l == num_layers - 1 else dim_hidden, bias=bias)
                                  for l in range(num_layers)])

    def forward(self, x):
        for l in range(self.num_layers):
            x = self.net[l](x)
            if l != self.num_layers - 1:
                x = F.relu(x, inplace=True)
        return x


def check_optimizer_config(cfg):
    """Only Adam with a constant learning rate is built; everything else is refused by name."""
    if cfg.optimizer != 'adam':
        raise NotImplementedError("optimizer %r is not built natively (only 'adam'; Adan / AdamW / Adamax / SGD are out of scope)" % (cfg.optimizer,))
    if cfg.lr_policy not in ('constant', 'none'):
        raise NotImplementedError("lr_policy %r is not built natively (only 'constant' / 'none'; the schedulers are out of scope)" % (cfg.lr_policy,))


class NeRFNetwork(nn.Module):
    # the native renders are all this network's run_cuda: what nerf_render.covered_call / covered_train_call read
    _dwg_shaded_render = True
    _dwg_train_render = True
    _dwg_train_shaded = True
    dmtet = False
    _learned_background = False         # BackgroundNeRFNetwork: cfg.bg_mode 'nerf' is accepted

    def __init__(self, cfg, device=None, num_layers=3, hidden_dim=64):
        super().__init__()
        if getattr(cfg, "structure", 'shared_mlp') != 'shared_mlp':
            raise NotImplementedError("structure %r is not built natively (only 'shared_mlp')" % (cfg.structure,))
        if cfg.backbone not in BACKBONES:
            raise NotImplementedError("backbone %r is not built natively (%s)" % (cfg.backbone, ", ".join(sorted(BACKBONES))))
        if cfg.nerf_type not in ('rgb', 'latent'):
            raise NotImplementedError("nerf_type %r is not built natively (a decoder_layer is not covered; 'rgb' / 'latent')" % (cfg.nerf_type,))
        if getattr(cfg, "dmtet", False):
            raise NotImplementedError("dmtet is not built natively")
        if not cfg.cuda_ray:
            raise NotImplementedError("run() without cuda_ray is not built natively")
        if cfg.bg_mode == 'nerf' and not self._learned_background:
            raise NotImplementedError("the learned 'nerf' background is not built natively by NeRFNetwork "
                                      "(BackgroundNeRFNetwork / build_nerf_network build it)")
        if cfg.density_prior not in nerf.PRIORS:
            raise NotImplementedError("density_prior %r is not covered (%s)" % (cfg.density_prior, ", ".join(sorted(nerf.PRIORS))))
        if cfg.density_activation not in nerf.ACTIVATIONS:
            raise NotImplementedError("density_activation %r is not covered" % (cfg.density_activation,))
        # _NeRFRenderer.__init__ (nerf_renderer.py:22-60)
        self.opt = cfg
        self.bound = cfg.bound
        self.cascade = 1 + math.ceil(math.log2(cfg.bound))
        self.grid_size = cfg.grid_size
        self.cuda_ray = cfg.cuda_ray
        self.min_near = cfg.min_near
        self.density_thresh = cfg.density_thresh
        self.bg_mode = cfg.bg_mode
        self.bg_radius = 0.0
        self.rand_bg_prob = cfg.rand_bg_prob
        self.latent_mode = cfg.nerf_type in ('latent', 'latent_approx')
        if self.latent_mode:
            self.img_dims = 4
            self.additional_dim_size = 1
            self.bg_colors = {
                'white': torch.tensor([2.1750, 1.4431, -0.0317, -1.1624]),
                'black': torch.tensor([-0.9952, -2.6023, 1.1155, 1.2966]),
                'gray': torch.tensor([0.9053, -0.7003, 0.5424, 0.1057]),
            }
        else:
            self.img_dims = 3
            self.additional_dim_size = 0
            self.bg_colors = {
                'white': torch.tensor([1.0, 1.0, 1.0]),
                'black': torch.tensor([0.0, 0.0, 0.0]),
                'gray': torch.tensor([0.5, 0.5, 0.5]),
            }
        self.raymarching = raymarch
        aabb_train = torch.FloatTensor([-cfg.bound, -cfg.bound, -cfg.bound, cfg.bound, cfg.bound, cfg.bound])
        self.register_buffer('aabb_train', aabb_train)
        self.register_buffer('aabb_infer', aabb_train.clone())
        # extra state for cuda raymarching (:64-77); the grid itself is the OccupancyGrid's, adopted below
        self.register_buffer('density_grid', torch.zeros([self.cascade, self.grid_size ** 3]))
        self.register_buffer('density_bitfield', torch.zeros(self.cascade * self.grid_size ** 3 // 8, dtype=torch.uint8))
        self.mean_density = 0
        self.iter_density = 0
        self.min_density = None
        self.max_density = None
        self.register_buffer('step_counter', torch.zeros(16, 2, dtype=torch.int32))
        self.mean_count = 0
        self.local_step = 0
        # _NeRFNetwork.__init__ (nerf_model.py:215-266)
        self.num_layers, self.hidden_dim = num_layers, hidden_dim
        self.encoder = GridEncoder(input_dim=3, num_levels=cfg.num_levels, level_dim=cfg.level_dim, base_resolution=cfg.base_resolution,
                                   log2_hashmap_size=19, desired_resolution=cfg.desired_resolution * self.bound,
                                   gridtype=BACKBONES[cfg.backbone], interpolation='smoothstep')
        self.in_dim = self.encoder.output_dim
        self.sigma_net = MLP(self.in_dim, 4 + self.additional_dim_size, hidden_dim, num_layers, bias=True)
        self.sigma_scale = nn.Parameter(torch.tensor(0.0))
        self.density_prior_type = cfg.density_prior
        self.bg_net = None
        self.decoder_layer = None
        self._occupancy = None
        if device is not None:
            self.to(device)

    # -- the field (B7) ----------------------------------------------------------------------------------------------------------------
    def _field(self, x, raw, sigmoid, mlp_no_grad=False):
        return nerf.nerf_field(x, self.encoder, self.sigma_net, self.sigma_scale, self.bound, density_activation=self.opt.density_activation,
                               density_prior=self.density_prior_type, albedo_sigmoid=sigmoid, raw=raw, mlp_no_grad=mlp_no_grad)

    def common_forward(self, x, mask=None, return_raw=False, **kwargs):
        if return_raw:
            return self._field(x, raw=True, sigmoid=False)
        sigma, albedo = self._field(x, raw=False, sigmoid=not self.latent_mode)
        if mask is not None:
            sigma = sigma * mask
        return sigma, albedo

    def local_geometry_forward(self, x, mlp_no_grad: bool = False):
        return self._field(x, raw=True, sigmoid=not self.latent_mode, mlp_no_grad=mlp_no_grad)

    def density(self, x):
        sigma, albedo = self.common_forward(x)
        return {'sigma': sigma, 'albedo': albedo}

    def normal(self, x, normal_type: str = 'finite_difference_laplacian', epsilon: float = 1e-3):
        """BaseNeRFNetwork.normal (nerf_model.py:146-169), the finite-difference form: the field does not differentiate its input."""
        if normal_type != 'finite_difference_laplacian':
            raise NotImplementedError("normal_type %r is not built natively (the field has no gradient with respect to x)" % (normal_type,))
        b = self.bound
        s = []
        for axis in range(3):
            for sign in (1.0, -1.0):
                shift = [0.0, 0.0, 0.0]
                shift[axis] = sign * epsilon
                s.append(self.common_forward((x + torch.tensor([shift], device=x.device)).clamp(-b, b))[0])
        normal = - 0.5 * torch.stack([s[0] - s[1], s[2] - s[3], s[4] - s[5]], dim=-1) / epsilon
        normal = normal / torch.sqrt(torch.clamp(torch.sum(normal * normal, -1, keepdim=True), min=1e-20))
        return torch.nan_to_num(normal)

    # -- the occupancy grid (B13) ------------------------------------------------------------------------------------------------------
    def _grid(self):
        g = self._occupancy
        if (g is None or g.density_grid.data_ptr() != self.density_grid.data_ptr()
                or g.density_bitfield.data_ptr() != self.density_bitfield.data_ptr() or g.density_thresh != float(self.density_thresh)):
            g = occupancy.OccupancyGrid(self.grid_size, self.bound, self.density_thresh, density_grid=self.density_grid,
                                        density_bitfield=self.density_bitfield)
            self._occupancy = g
        return g

    @torch.no_grad()
    def update_extra_state(self, decay=0.95, S=None, random_sigmas: bool = False):
        """_NeRFRenderer.update_extra_state (nerf_renderer.py:95-153) on OccupancyGrid.update; a chunked update (S below grid_size) is
        not restated."""
        if S is not None and S < self.grid_size:
            raise NotImplementedError("a chunked occupancy update (S < grid_size) is not built natively")
        g = self._grid()
        g.update(self.encoder, self.sigma_net, self.sigma_scale, density_activation=self.opt.density_activation,
                 density_prior=self.density_prior_type, decay=decay, random_sigmas=random_sigmas)
        st = g.stats()
        self.mean_density, self.min_density, self.max_density = st["mean_density"], st["min_density"], st["max_density"]
        self.iter_density += 1
        ### update step counter
        total_step = min(16, self.local_step)
        if total_step > 0:
            self.mean_count = int(self.step_counter[:total_step, 0].sum().item() / total_step)
        self.local_step = 0

    # -- render (B20) ------------------------------------------------------------------------------------------------------------------
    def render(self, data, shading='albedo', bg_mode=None, **kwargs):
        return nerf_view.render_view(self, data, shading=shading, bg_mode=bg_mode, **kwargs)

    # -- optimizer ---------------------------------------------------------------------------------------------------------------------
    def _param_groups(self, cfg):
        lr = cfg.lr
        return [
            {'params': list(self.encoder.parameters()), 'lr': lr * 10, 'name': 'encoder'},
            {'params': list(self.sigma_net.parameters()), 'lr': lr, 'name': 'sigma_net'},
            {'params': [self.sigma_scale], 'lr': lr, 'name': 'sigma_scale'},
        ]

    def get_optimizer(self, cfg, diffusion=None):
        """_NeRFNetwork.get_optimizer (nerf_model.py:297-329) with build_optimizer's 'adam' (:171-173): encoder at lr x 10, sigma_net at lr,
        sigma_scale at lr, betas (0.9, 0.99), eps 1e-15 -- as one named optimizer 'nerf' over the flat buffers, a fused launch per group.
        Returns (optimizers, scheduler) like the reference; the scheduler of lr_policy 'constant' / 'none' is None."""
        check_optimizer_config(cfg)
        spec = optim.AdamSpec(self._param_groups(cfg), betas=(0.9, 0.99), eps=1e-15)
        return optim.build_flat_optimizers({'nerf': spec}, self.sigma_scale.device), None


class BackgroundNeRFNetwork(NeRFNetwork):
    """NeRFNetwork with the reference's learned background (nerf_model.py:248-256, bg_radius > 0): encoder_bg = FreqEncoder(3, 6) and
    bg_net = MLP(39, 3 + additional_dim_size, hidden_dim_bg, num_layers_bg), state-dict keys bg_net.net.{l}.{weight,bias}.  The render
    takes bg_mode 'nerf' through nerf_background.learned_background (boundary B22)."""
    _learned_background = True

    def __init__(self, cfg, device=None, num_layers=3, hidden_dim=64, num_layers_bg=2, hidden_dim_bg=64):
        super().__init__(cfg, device=None, num_layers=num_layers, hidden_dim=hidden_dim)
        self.bg_radius = cfg.bg_radius
        self.num_layers_bg, self.hidden_dim_bg = num_layers_bg, hidden_dim_bg
        self.encoder_bg = nerf_background.FreqEncoder(input_dim=3, degree=6)
        self.in_dim_bg = self.encoder_bg.output_dim
        self.bg_net = MLP(self.in_dim_bg, 3 + self.additional_dim_size, hidden_dim_bg, num_layers_bg, bias=True)
        reason = nerf_background.unsupported_reason(self.encoder_bg, self.bg_net)
        if reason is not None:
            raise NotImplementedError("this learned background is not built natively: %s" % reason)
        if device is not None:
            self.to(device)

    def _param_groups(self, cfg):
        """The reference's groups (nerf_model.py:312-314): bg_net at bg_lr.  Its encoder_bg group at bg_lr x 10 is empty (the frequency
        encoding has no parameters) and is not created."""
        return super()._param_groups(cfg) + [{'params': list(self.bg_net.parameters()), 'lr': cfg.bg_lr, 'name': 'bg_net'}]


def build_nerf_network(cfg, device=None, **kw):
    """The stage-I network cfg asks for: BackgroundNeRFNetwork when cfg.bg_mode is 'nerf', else NeRFNetwork."""
    cls = BackgroundNeRFNetwork if cfg.bg_mode == 'nerf' else NeRFNetwork
    return cls(cfg, device=device, **kw)
