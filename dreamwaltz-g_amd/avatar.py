"""MI355X-native mirror of the reference's avatar hot path (boundary B3/B5).

  GaussianOutput / merge_gaussians   /root/reference/core/gaussian/gaussian_utils.py:20-68
  GeneralLinearBlendSkinning         /root/reference/core/human/inverse_lbs.py:517-784
        .forward(**smpl_inputs) -> (transform_J, transform_V, transforms)   -- the reference's triple of RigidTransform objects
  MeshBindingGaussianModel           /root/reference/core/system/avatar.py:921-1096
  DreamWaltzG (.animate, .lbs_transform, .inverse_lbs_transform, .non_rigid_transform, .get_optimizer, ...)  avatar.py:1097-1635
Heavy arithmetic = HIP kernels through the C-ABI (lbs.hip, gridenc.hip, gemm.hip, assemble.hip, meshbind.hip); what the
reference materialises densely per step (transform_V [V,4,4], the three vertex offsets) is kept LAZY here and only computed
for the vertex subset a caller asks for.  Parameter names match the reference so its checkpoints map one to one.
"""
from dataclasses import dataclass, fields
from typing import Dict, Optional

import torch
import torch.nn as nn

from . import assemble as asm_ops
from . import lbs as lbs_ops
from . import meshbind as mb_ops
from . import optim
from .gridencoder import GridEncoder
from .mlp import MLP, DeformNetwork
from .rigid import (RigidTransform, matrix_to_quaternion, quaternion_multiply, standardize_quaternion)  # noqa: F401  (re-exported)


@dataclass
class GaussianOutput:
    positions: Optional[torch.Tensor] = None
    sh_features: Optional[torch.Tensor] = None
    opacities: Optional[torch.Tensor] = None
    quaternions: Optional[torch.Tensor] = None
    scales: Optional[torch.Tensor] = None
    colors: Optional[torch.Tensor] = None
    cov3D: Optional[torch.Tensor] = None
    offsets: Optional[torch.Tensor] = None
    lbs_weights: Optional[torch.Tensor] = None

    def __getitem__(self, key):
        return getattr(self, key)

    def get(self, key, default=None):
        return getattr(self, key, default)

    def keys(self):
        return iter([f.name for f in fields(self)])


def merge_gaussians(*gaussians: GaussianOutput) -> GaussianOutput:
    if len(gaussians) == 1:
        return gaussians[0]
    out = {}
    for f in fields(GaussianOutput):
        parts = [g[f.name] for g in gaussians if torch.is_tensor(g[f.name])]
        out[f.name] = torch.cat(parts, dim=0) if parts else None
    return GaussianOutput(**out)


# ----------------------------------------------------------------------------------------------------------------------
# skeleton
# ----------------------------------------------------------------------------------------------------------------------
class _LazyRigidTransform(RigidTransform):
    """A RigidTransform whose SE3 is only built when somebody reads it (.SE3 / .R / .T or any algebra on it)."""

    def __init__(self, thunk):
        self.__dict__["_thunk"] = thunk

    def _materialise(self):
        SE3 = self.__dict__.pop("_thunk")()
        self.SE3, self.R, self.T = SE3, SE3[..., :3, :3], SE3[..., :3, 3]

    def __getattr__(self, name):
        if name in ("SE3", "R", "T") and "_thunk" in self.__dict__:
            self._materialise()
            return self.__dict__[name]
        raise AttributeError(name)

    def squeeze(self, dim=0):
        if "_thunk" in self.__dict__:
            inner = self.__dict__["_thunk"]
            self.__dict__["_thunk"] = lambda: inner().squeeze(dim)
            return self
        return super().squeeze(dim)


class _VertexTransform(_LazyRigidTransform):
    """transform_V = compose(V_shape_offset, V_pose_offset, V_pose_rigid[, transl]) (inverse_lbs.py:758-772).  The one call the
    hot path makes on it, `.transform_points(vertex_coords, indices=predefined_vertex_indices)` (avatar.py:1570,1577), runs on the
    vertex SUBSET in one HIP launch (lbs.hip k_vertex_transform) and is differentiable w.r.t. the shape coefficients (betas)."""

    def __init__(self, model, ctx, thunk):
        super().__init__(thunk)
        self.__dict__["_model"], self.__dict__["_ctx"] = model, ctx

    def transform_points(self, points, indices=None, weights=None):
        if indices is not None and weights is None and "_thunk" in self.__dict__ and points.is_cuda:
            return self._model._transform_vertex_subset(self._ctx, indices, points)
        return super().transform_points(points, indices=indices, weights=weights)


class LBSTransforms(dict):
    """The `transforms` dict of GeneralLinearBlendSkinning.forward: keys V_shape_offset, V_pose_offset, V_pose_rigid,
    J_shape_offset, J_pose_rigid, G_transl_offset -> RigidTransform, every one built on first access.  The fused kernels read the
    attributes instead: A [J,4,4] = compose(J_pose_rigid, G_transl_offset) as ONE tensor straight from k_joint_chain."""
    KEYS = ("V_shape_offset", "V_pose_offset", "V_pose_rigid", "J_shape_offset", "J_pose_rigid", "G_transl_offset")

    def __init__(self, model, A, rot_mats, full_shape, transl, full_pose):
        super().__init__()
        self.model, self.A, self.rot_mats, self.full_shape, self.transl, self.full_pose = model, A, rot_mats, full_shape, transl, full_pose

    def __missing__(self, key):
        if key not in self.KEYS:
            raise KeyError(key)
        v = self.model._build_transform(self, key)
        self[key] = v
        return v

    def __contains__(self, key):
        return key in self.KEYS

    def keys(self):
        return list(self.KEYS)


class GeneralLinearBlendSkinning(nn.Module):
    """Mirror of inverse_lbs.py:517-784 for a frozen SMPL-X(-shaped) model given as tensors."""

    def __init__(self, body: Dict[str, torch.Tensor]):
        super().__init__()
        for k in ("v_template", "posedirs", "J_regressor", "lbs_weights", "betas", "expression", "pose_mean", "jaw_pose",
                  "leye_pose", "reye_pose"):
            self.register_buffer(k, body[k].float().contiguous())
        shapedirs = torch.cat([body["shapedirs"], body["expr_dirs"]], dim=-1).float().contiguous()   # [V,3,400]
        self.register_buffer("shapedirs_all", shapedirs)
        self.register_buffer("parents", torch.as_tensor(body["parents"]).to(torch.int32))
        self.register_buffer("J_template", torch.einsum('ik,ji->jk', self.v_template, self.J_regressor))
        # joint_shape_dirs[j,c,l] = sum_v J_regressor[j,v] shapedirs[v,c,l]: vertices2joints of the blend-shape offsets
        self.register_buffer("joint_shape_dirs", torch.einsum('jv,vcl->jcl', self.J_regressor, shapedirs).contiguous())
        self.num_joints = self.J_regressor.shape[0]
        self.NUM_BODY_JOINTS = 21
        self.use_smplx = True
        self._subsets = []          # [(index tensor kept alive, its version, gathered rows)]

    @classmethod
    def from_reference(cls, ref) -> "GeneralLinearBlendSkinning":
        """Adopts the tensors of a reference `GeneralLinearBlendSkinning` (inverse_lbs.py:521-568: the copies it took of the smplx model's
        v_template / shapedirs / expr_dirs / posedirs / J_regressor / lbs_weights / parents / betas / expression / pose_mean / jaw, eye
        poses) -- by attribute name; the frozen `learn_*` flags of the shipped recipes are required."""
        if not getattr(ref, "use_smplx", True):
            raise NotImplementedError("SMPL (not SMPL-X) body models")
        for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights", "expr_dirs"):
            if getattr(getattr(ref, k), "requires_grad", False):
                raise NotImplementedError("learnable %s (cfg.render.deform_learn_*): the skeleton tensors are frozen on this path" % k)
        t = lambda v: torch.as_tensor(v).detach()       # noqa: E731
        body = {k: t(getattr(ref, k)) for k in ("v_template", "shapedirs", "expr_dirs", "posedirs", "J_regressor", "lbs_weights", "betas",
                                                  "expression", "pose_mean", "jaw_pose", "leye_pose", "reye_pose")}
        body["parents"] = t(ref.parents).long()
        m = cls(body)
        m.NUM_BODY_JOINTS = int(getattr(ref, "NUM_BODY_JOINTS", 21))
        return m.to(body["v_template"].device)

    def get_full_shape(self, betas=None, expression=None, batch_size=None, extra_betas=None):
        """inverse_lbs.py:570-589."""
        betas = self.betas if betas is None else betas
        if extra_betas is not None:
            betas = betas + extra_betas
        expression = self.expression if expression is None else expression
        return torch.cat([betas, expression], dim=-1)

    def get_full_pose(self, body_pose=None, global_orient=None, left_hand_pose=None, right_hand_pose=None, jaw_pose=None,
                      leye_pose=None, reye_pose=None):
        """inverse_lbs.py:591-631 -- jaw/eye arguments are accepted and ignored exactly like the reference (checklist Q1)."""
        dev, z = self.v_template.device, (lambda n: torch.zeros(1, n, device=self.v_template.device))
        global_orient = z(3) if global_orient is None else global_orient
        body_pose = z(63) if body_pose is None else body_pose
        left_hand_pose = z(45) if left_hand_pose is None else left_hand_pose
        right_hand_pose = z(45) if right_hand_pose is None else right_hand_pose
        full = torch.cat([global_orient.reshape(-1, 3), body_pose.reshape(-1, 3), self.jaw_pose.reshape(-1, 3),
                          self.leye_pose.reshape(-1, 3), self.reye_pose.reshape(-1, 3), left_hand_pose.reshape(-1, 3),
                          right_hand_pose.reshape(-1, 3)], dim=0).to(dev)
        return full + self.pose_mean.reshape(-1, 3)

    def forward(self, betas=None, body_pose=None, global_orient=None, left_hand_pose=None, right_hand_pose=None,
                jaw_pose=None, leye_pose=None, reye_pose=None, expression=None, transl=None, flame_betas=None,
                flame_expression=None, extra_betas=None):
        """-> (transform_J, transform_V, transforms), inverse_lbs.py:719-784.  Two small launches (shaped joints, chain); the dense
        per-vertex transforms are built only if read.  The skeleton pass of the SAME input tensors (same objects, unmodified) is shared:
        the loader's condition image and `animate` both ask for the observed pose in one step."""
        args = (betas, body_pose, global_orient, left_hand_pose, right_hand_pose, jaw_pose, leye_pose, reye_pose, expression, transl,
                flame_betas, flame_expression)
        # (inference tensors carry no version counter: calls made with them are simply not remembered)
        cacheable = extra_betas is None and not any(torch.is_tensor(a) and a.is_inference() for a in args)
        own = (self.betas,) if torch.is_tensor(getattr(self, "betas", None)) else ()       # the model's own shape coefficients are part of the result
        key = tuple((id(a), a._version) if torch.is_tensor(a) else a for a in args + own) if cacheable else None
        last = getattr(self, "_last_forward", None)
        if cacheable and last is not None and last[0] == key:
            return last[2]
        full_shape = self.get_full_shape(betas=betas, expression=expression, extra_betas=extra_betas)
        with torch.no_grad():
            full_pose = self.get_full_pose(body_pose, global_orient, left_hand_pose, right_hand_pose, jaw_pose, leye_pose, reye_pose)
            A, R = lbs_ops.joint_chain(full_pose, self.J_template, self.parents, transl=transl, return_rot_mats=True,
                                       joint_shape_dirs=self.joint_shape_dirs, shape_coeffs=full_shape.detach())
        tr = LBSTransforms(self, A, R, full_shape, transl, full_pose)
        transform_V = _VertexTransform(self, tr, lambda: self._dense_transform_V(tr))
        transform_J = _LazyRigidTransform(lambda: self._dense_transform_J(tr))
        if cacheable:
            self._last_forward = (key, args, (transform_J, transform_V, tr))       # `args` keeps the tensors (and their ids) alive
        return transform_J, transform_V, tr

    # -- lazily built dense pieces (not on the hot path) -----------------------------------------------------------------
    def _joints(self, tr):
        return self.J_template + (self.joint_shape_dirs * tr.full_shape.reshape(1, 1, -1)).sum(-1)

    def _build_transform(self, tr, key):
        dev = self.v_template.device
        if key == "G_transl_offset":
            if tr.transl is not None:
                return RigidTransform(T=tr.transl.reshape(1, 3).float())
            return RigidTransform(SE3=torch.eye(4, device=dev).expand(1, 4, 4))
        if key == "J_pose_rigid":
            SE3 = tr.A.clone()
            if tr.transl is not None:
                SE3[:, :3, 3] = SE3[:, :3, 3] - tr.transl.reshape(3)
            return RigidTransform(SE3=SE3[None])
        if key == "J_shape_offset":
            return RigidTransform(T=(self._joints(tr) - self.J_template)[None])
        if key == "V_shape_offset":
            return RigidTransform(T=torch.einsum('vcl,l->vc', self.shapedirs_all, tr.full_shape.reshape(-1))[None])
        if key == "V_pose_offset":
            feat = (tr.rot_mats[1:] - torch.eye(3, device=dev)).reshape(1, -1)
            return RigidTransform(T=(feat @ self.posedirs).view(1, -1, 3))
        if key == "V_pose_rigid":
            A = tr["J_pose_rigid"].SE3[0]
            return RigidTransform(SE3=torch.einsum('vj,jkl->vkl', self.lbs_weights, A)[None])
        raise KeyError(key)

    def _dense_transform_V(self, tr):
        t = tr["V_shape_offset"].compose(tr["V_pose_offset"], tr["V_pose_rigid"])
        return (t.compose(tr["G_transl_offset"]) if tr.transl is not None else t).SE3

    def _dense_transform_J(self, tr):
        t = tr["J_shape_offset"].compose(tr["J_pose_rigid"])
        return (t.compose(tr["G_transl_offset"]) if tr.transl is not None else t).SE3

    # -- vertex subset (mesh-bound Gaussians) --------------------------------------------------------------------------
    def _subset_rows(self, vertex_indices):
        """Blend-shape / pose-corrective / skinning rows of a vertex subset, gathered once per index tensor.  The cache holds
        the index tensor itself (so its storage cannot be recycled under a stale entry) and its version counter."""
        for ref, ver, rows in self._subsets:
            if ref is vertex_indices or (ref.data_ptr() == vertex_indices.data_ptr() and ref.shape == vertex_indices.shape and
                                         ref.device == vertex_indices.device):
                if ref._version == ver and vertex_indices._version == ver:
                    return rows
        rows = lbs_ops.gather_vertex_subset(vertex_indices.to(self.v_template.device), self.lbs_weights, self.shapedirs_all, self.posedirs)
        self._subsets = [e for e in self._subsets if e[0] is not vertex_indices][-7:] + [(vertex_indices, vertex_indices._version, rows)]
        return rows

    def _transform_vertex_subset(self, tr, vertex_indices, vertex_coords):
        rows = self._subset_rows(vertex_indices)
        return lbs_ops.vertex_transform(vertex_coords, tr.A, rows, tr.full_shape, tr.rot_mats, joint_chain_ctx=(
            self.parents, self.joint_shape_dirs, self.J_template), pose=tr.full_pose)

    def transform_vertices(self, tr: LBSTransforms, vertex_indices, vertex_coords):
        """transform_V.transform_points(vertex_coords, indices=...) (avatar.py:1570,1577)."""
        return self._transform_vertex_subset(tr, vertex_indices, vertex_coords)


# ----------------------------------------------------------------------------------------------------------------------
# mesh-bound Gaussians (hands / face)
# ----------------------------------------------------------------------------------------------------------------------
class MeshBindingGaussianModel(nn.Module):
    """avatar.py:921-1096: n Gaussians per triangle, learnable barycentric coordinates and tangent scales."""

    def __init__(self, vertex_coords, triangles, vertex_indices, n_per_triangle=6, init_scale_ratio=1.0, learn_bary_coords=True,
                 learn_vertex_coords=False, learn_scales=True):
        super().__init__()
        if learn_vertex_coords:
            # the native vertex-transform Function has no gradient w.r.t. the bound vertex coordinates and `animate` caches the canonical
            # vertices: accepting the flag would build an Adam group that never moves (the shipped recipes keep it off, configs:202-205)
            raise NotImplementedError("learn_vertex_coords=True: the mesh-bound vertex coordinates are frozen on this path")
        self.learn_bary_coords, self.learn_vertex_coords, self.learn_scales = learn_bary_coords, learn_vertex_coords, learn_scales
        self.register_buffer("predefined_vertex_indices", vertex_indices.long())
        self.register_buffer("triangles", triangles.long())
        self._n_points_per_triangle = n_per_triangle
        Fp = triangles.shape[0]
        self._n_triangles, self._n_vertices, self._n_points = Fp, vertex_coords.shape[0], Fp * n_per_triangle
        base = torch.tensor([[2 / 3, 1 / 6, 1 / 6], [1 / 6, 2 / 3, 1 / 6], [1 / 6, 1 / 6, 2 / 3], [1 / 6, 5 / 12, 5 / 12],
                             [5 / 12, 1 / 6, 5 / 12], [5 / 12, 5 / 12, 1 / 6]], dtype=torch.float32)
        assert n_per_triangle == 6, "default n_gaussians_per_triangle"
        self._bary_coords = nn.Parameter(base.expand(Fp, -1, -1).clone(), requires_grad=learn_bary_coords)
        self._vertex_coords = nn.Parameter(vertex_coords.float().clone(), requires_grad=learn_vertex_coords)
        self._scales = nn.Parameter(torch.ones(Fp * n_per_triangle, 3) * init_scale_ratio, requires_grad=learn_scales)
        p2t = torch.arange(Fp)[:, None].expand(-1, n_per_triangle).reshape(-1)
        self.register_buffer("points_to_triangles", p2t)
        self.register_buffer("points_to_vertices", self.triangles[p2t])
        self._rebuild_topology()

    @classmethod
    def from_reference(cls, ref) -> "MeshBindingGaussianModel":
        """Adopts a reference `MeshBindingGaussianModel` (avatar.py:921-966) by attribute name: triangles (already re-indexed to the part's
        vertices), predefined_vertex_indices, and the three parameters _bary_coords / _vertex_coords / _scales with their learn flags."""
        n = int(ref._n_points_per_triangle)
        m = cls(ref._vertex_coords.detach(), ref.triangles.detach(), torch.as_tensor(ref.predefined_vertex_indices), n_per_triangle=n,
                learn_bary_coords=bool(ref.learn_bary_coords), learn_vertex_coords=bool(ref.learn_vertex_coords),
                learn_scales=bool(ref.learn_scales))
        with torch.no_grad():
            m._bary_coords.copy_(ref._bary_coords.detach()); m._scales.copy_(ref._scales.detach())
        if hasattr(ref, "predefined_triangle_indices"):
            m.predefined_triangle_indices = torch.as_tensor(ref.predefined_triangle_indices)
        return m.to(ref._vertex_coords.device)

    def _rebuild_topology(self):
        """Derived buffers of the native path (csrc/meshbind.hip): int32 topology + the static vertex -> face adjacency."""
        self.register_buffer("triangles_i32", self.triangles.to(torch.int32).contiguous(), persistent=False)
        off, faces = mb_ops.build_vertex_face_csr(self.triangles, self._vertex_coords.shape[0])
        self.register_buffer("vf_offsets", off.to(self.triangles.device), persistent=False)
        self.register_buffer("vf_faces", faces.to(self.triangles.device), persistent=False)

    @staticmethod
    def bary_coord_activation(bary_coords):
        return bary_coords / bary_coords.sum(dim=-1, keepdim=True)

    def get_vertex_coords(self):
        return self._vertex_coords

    def forward(self, canonical_vertex_coords, observed_vertex_coords):
        """get_positions (canonical + observed) and get_scales_and_quaternions (observed) in one forward / one backward launch
        -> (canonical positions, positions, scales, quaternions)."""
        return mb_ops.meshbind_full(self._bary_coords, self._scales, canonical_vertex_coords, observed_vertex_coords, self.triangles_i32,
                                    self.vf_offsets, self.vf_faces, self._n_points_per_triangle)

    def get_positions(self, vertex_coords=None, bary_coords=None):
        """avatar.py:1016-1025 (same HIP kernel, positions only)."""
        if vertex_coords is None:
            vertex_coords = self.get_vertex_coords()
        if bary_coords is not None:
            return torch.einsum('fnv,fvc->fnc', bary_coords, vertex_coords[self.triangles]).reshape(-1, 3)
        return mb_ops.meshbind_full(self._bary_coords, self._scales, None, vertex_coords, self.triangles_i32, self.vf_offsets,
                                    self.vf_faces, self._n_points_per_triangle)[1]

    def get_scales_and_quaternions(self, vertex_coords, positions=None, eps=1e-9):
        """avatar.py:1027-1079; `positions` is recomputed inside the kernel from the same inputs."""
        _, _, s, q = mb_ops.meshbind_full(self._bary_coords, self._scales, None, vertex_coords, self.triangles_i32, self.vf_offsets,
                                          self.vf_faces, self._n_points_per_triangle)
        return s, q

    def get_optimizer(self, cfg, optimizer_name: str):
        """avatar.py:1082-1096: Adam(lr=0, eps=1e-15) with groups bary_coords (position_lr_init), vertex_coords, scales (scaling_lr)."""
        l = []
        if self.learn_bary_coords:
            l.append({'params': [self._bary_coords], 'lr': cfg.render.position_lr_init, 'name': "bary_coords"})
        if self.learn_vertex_coords:
            l.append({'params': [self._vertex_coords], 'lr': cfg.render.position_lr_init, 'name': "vertex_coords"})
        if self.learn_scales:
            l.append({'params': [self._scales], 'lr': cfg.render.scaling_lr, 'name': "scales"})
        return {optimizer_name: optim.AdamSpec(l, eps=1e-15)} if l else {}


# ----------------------------------------------------------------------------------------------------------------------
# the avatar
# ----------------------------------------------------------------------------------------------------------------------
class DreamWaltzG(nn.Module):
    def __init__(self, lbs_model: GeneralLinearBlendSkinning, positions, scales, quaternions, lbs_weights,
                 smpl_canonical_inputs: dict, mesh_binding_gaussians: Optional[Dict[str, MeshBindingGaussianModel]] = None,
                 nerf_bound=2.0, init_offset=0.01, init_scale=0.001, max_scale=0.01, learn_positions=True, learn_scales=True,
                 learn_quaternions=True, learn_lbs_weights=False, learn_hand_betas=False, learn_face_betas=False,
                 nearest_vertex_indices=None, cfg=None):
        super().__init__()
        self.lbs_model = lbs_model
        self.deform_model = None
        self._positions = nn.Parameter(positions.float().clone(), requires_grad=learn_positions)
        self._scales = nn.Parameter(torch.log(scales.float().clone()), requires_grad=learn_scales)       # scale_activation = exp
        self._quaternions = nn.Parameter(quaternions.float().clone(), requires_grad=learn_quaternions)
        self._lbs_weights = nn.Parameter(lbs_weights.float().clone(), requires_grad=learn_lbs_weights)   # configs/__init__.py:197
        self.learn_positions, self.learn_scale, self.learn_quaternions, self.learn_lbs_weights = (
            learn_positions, learn_scales, learn_quaternions, learn_lbs_weights)
        self.learn_hand_betas, self.learn_face_betas = learn_hand_betas, learn_face_betas
        self.learn_betas = learn_hand_betas or learn_face_betas
        self._betas = nn.Parameter(lbs_model.betas.data.clone(), requires_grad=self.learn_betas)          # avatar.py:1225
        self.smpl_canonical_inputs = smpl_canonical_inputs
        self.register_buffer("nerf_bound", torch.tensor(float(nerf_bound)))
        self._nerf_bound_host = float(nerf_bound)
        self.init_offset, self.init_scale, self.max_scale = init_offset, init_scale, max_scale
        # the default flags (configs/__init__.py:117-126); non-default combinations are rejected, not silently ignored
        self.use_joint_shape_offsets = self.use_vertex_shape_offsets = self.use_vertex_pose_offsets = False
        self.use_non_rigid_offsets, self.use_non_rigid_scales, self.use_non_rigid_rotations = True, True, False
        self.non_rigid_scale_mode = self.non_rigid_rotation_mode = 'add'
        self.render_mesh_binding_3d_gaussians_only = self.render_unconstrained_3d_gaussians_only = False
        self.use_nerf_encoded_position = True
        if cfg is not None:
            for k in ("use_joint_shape_offsets", "use_vertex_shape_offsets", "use_vertex_pose_offsets", "use_non_rigid_offsets",
                      "use_non_rigid_scales", "use_non_rigid_rotations", "non_rigid_scale_mode", "non_rigid_rotation_mode",
                      "render_mesh_binding_3d_gaussians_only", "render_unconstrained_3d_gaussians_only", "use_nerf_encoded_position"):
                if hasattr(cfg.render, k) and getattr(cfg.render, k) != getattr(self, k):
                    raise NotImplementedError("cfg.render.%s = %r: only the default configuration of the shipped recipes is built "
                                              "(configs/__init__.py:117-126)" % (k, getattr(cfg.render, k)))
        # nerf_model.py:223-232: tiledgrid encoder L=16 C=2 base 16 -> 2048*bound, smoothstep; sigma_net 32->64->64->4
        self.nerf_encoder = GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19,
                                        desired_resolution=2048 * nerf_bound, gridtype='tiled', align_corners=False,
                                        interpolation='smoothstep')
        self.nerf_opacity_and_color_net = MLP(32, 4, 64, 3, bias=True)
        self.nerf_scale_and_quaternion_net = DeformNetwork(xyz_input_ch=32, D=4, W=64)
        self.mesh_binding_gaussians = nn.ModuleDict(mesh_binding_gaussians or {})
        self._n_points = self._positions.shape[0]
        self._n_points_on_mesh = sum(m._n_points for m in self.mesh_binding_gaussians.values())
        self.nearest_triangles_buffer = {'nearest_vertex_indices': nearest_vertex_indices}
        self._canonical_cache = None
        self._canonical_vertices = {}

    @classmethod
    def from_reference(cls, ref, cfg=None) -> "DreamWaltzG":
        """The HIP-backed avatar for the object the reference's `build_gaussian_avatar` returned (avatar.py:1642-1714 -> DreamWaltzG.__init__
        avatar.py:1098-1244): same Gaussians, same networks, same body -- every Parameter / buffer is adopted BY NAME from `ref`
        (its state_dict() loads into this object key for key), the constructor-time work of the reference (NeRF point cloud, nearest
        triangles, inverse LBS of the initial positions, LBS-weight smoothing) is NOT repeated here: `from_point_cloud` is its native
        counterpart, and under the binding the reference's constructor reaches the same kernels (B11).  dropin/dwg_bind.py calls this so that
        main.py reaches the kernels without an edit; `cfg` defaults to `ref.cfg` (non-default render flags are rejected loudly)."""
        cfg = cfg if cfg is not None else getattr(ref, "cfg", None)
        if type(ref.lbs_model).__name__ != "GeneralLinearBlendSkinning":
            raise NotImplementedError("deform_type without 'glbs' (%s)" % type(ref.lbs_model).__name__)
        if getattr(ref, "deform_model", None) is not None:
            raise NotImplementedError("deform_type 'non_rigid' (the reference's animate raises for it too, avatar.py:317-318)")
        enc = ref.nerf_encoder
        want = dict(input_dim=3, num_levels=16, level_dim=2, base_resolution=16)
        for k, v in want.items():
            if hasattr(enc, k) and int(getattr(enc, k)) != v:
                raise NotImplementedError("nerf encoder %s=%r (built: %r)" % (k, getattr(enc, k), v))
        lbs = GeneralLinearBlendSkinning.from_reference(ref.lbs_model)
        mesh = {k: MeshBindingGaussianModel.from_reference(m) for k, m in ref.mesh_binding_gaussians.items()}
        nvi = None
        ntb = getattr(ref, "nearest_triangles_buffer", None)
        if isinstance(ntb, dict):
            nvi = ntb.get("nearest_vertex_indices")
        av = cls(lbs, ref._positions.detach(), torch.exp(ref._scales.detach()), ref._quaternions.detach(), ref._lbs_weights.detach(),
                 {k: v.detach() for k, v in ref.smpl_canonical_inputs.items()}, mesh, nerf_bound=float(ref.nerf_bound),
                 init_offset=float(ref.init_offset), init_scale=float(ref.init_scale), max_scale=float(ref.max_scale),
                 learn_positions=bool(ref._positions.requires_grad), learn_scales=bool(ref._scales.requires_grad),
                 learn_quaternions=bool(ref._quaternions.requires_grad), learn_lbs_weights=bool(ref._lbs_weights.requires_grad),
                 learn_hand_betas=bool(getattr(ref, "learn_hand_betas", False)), learn_face_betas=bool(getattr(ref, "learn_face_betas", False)),
                 nearest_vertex_indices=nvi, cfg=cfg)
        if isinstance(ntb, dict):
            av.nearest_triangles_buffer = ntb
        for k in ("gridtype", "interpolation", "align_corners", "log2_hashmap_size"):
            if hasattr(enc, k) and getattr(enc, k) != getattr(av.nerf_encoder, k):
                raise NotImplementedError("nerf encoder %s=%r (this path builds %r: nerf_model.py:223-231 defaults)"
                                          % (k, getattr(enc, k), getattr(av.nerf_encoder, k)))
        if hasattr(enc, "per_level_scale") and abs(float(enc.per_level_scale) - float(av.nerf_encoder.per_level_scale)) > 1e-6:
            raise NotImplementedError("nerf encoder per_level_scale=%r (built: %r)" % (enc.per_level_scale, av.nerf_encoder.per_level_scale))
        av = av.to(ref._positions.device)
        loaded, unknown, missing = av.load_reference_state_dict(ref.state_dict(), prefix="")
        # every learnable tensor of the reference must have found its place; frozen body tensors are adopted above under other names
        need = [k for k, p in ref.named_parameters() if p.requires_grad]
        lost = [k for k in need if k not in loaded]
        if lost:
            raise RuntimeError("DreamWaltzG.from_reference: trainable reference parameters with no counterpart: %s" % lost)
        av.cfg = cfg
        av.__dict__["reference"] = ref       # NOT a registered sub-module (no state_dict keys): construction-time attributes the trainer
                                             # may still read (canonical_vertices, canonical_triangles, ...) resolve through __getattr__
        return av

    @classmethod
    def from_point_cloud(cls, lbs_model, points, canonical_vertices, canonical_triangles, smpl_canonical_inputs,
                         mesh_binding_gaussians=None, cfg=None, **learn_flags) -> "DreamWaltzG":
        """The avatar for a NeRF-stage point cloud, built on the device: the native counterpart of the reference constructor's tail
        (avatar.py:1176-1245).  points [N, 3] fp32 (canonical-pose space) and the canonical body mesh (canonical_vertices [V, 3] fp32,
        canonical_triangles [F, 3] int) on one HIP device.  In the reference's order: nearest triangles (avatar_init.find_nearest_triangles);
        with cfg.render.prune_points_close_to_mesh the per-part prune against each mesh-bound part's `predefined_triangle_indices` (the hands'
        threshold x 10); LBS weights interpolated from lbs_model.lbs_weights and smoothed as cfg.render.lbs_weight_smooth[_K, _N] say;
        inverse LBS of the points under the canonical transforms; scales init_scale, identity quaternions.  The learn_* flags, init_offset /
        init_scale / max_scale and nerf.bound come from cfg when given (the constructor's defaults otherwise); **learn_flags (any keyword of
        the constructor) override them.  `nearest_triangles_buffer` stays on the object, on the points' device.
        `pointcloud.export_point_cloud(...).points` (B12) is such a tensor: it feeds this constructor without a host round trip."""
        from . import avatar_init as ai
        r = getattr(cfg, "render", None)
        mesh = dict(mesh_binding_gaussians or {})
        points = points.detach()
        ntb = ai.find_nearest_triangles(points, canonical_vertices, canonical_triangles)
        if r is not None and getattr(r, "prune_points_close_to_mesh", False):
            dist = getattr(r, "prune_dists_close_to_mesh", None)
            for part, m in mesh.items():
                if part not in ("hands", "face"):
                    raise NotImplementedError("prune_points_close_to_mesh for the body part %r (avatar.py:1195-1199 knows hands and face)" % part)
                tri = getattr(m, "predefined_triangle_indices", None)
                if tri is None:
                    raise RuntimeError("prune_points_close_to_mesh: mesh_binding_gaussians[%r] carries no predefined_triangle_indices" % part)
                threshold = None if dist is None else (dist * 10 if part == "hands" else dist)
                points, ntb = ai.prune_points_close_to_mesh(points, ntb, tri, threshold=threshold)
        lbs_weights = ai.initialize_lbs_weights(lbs_model.lbs_weights, ntb, positions=points,
                                                smooth=bool(getattr(r, "lbs_weight_smooth", False)),
                                                smooth_K=getattr(r, "lbs_weight_smooth_K", None), smooth_N=getattr(r, "lbs_weight_smooth_N", None))
        kw = {}
        if r is not None:
            for k in ("learn_positions", "learn_scales", "learn_quaternions", "learn_lbs_weights", "learn_hand_betas", "learn_face_betas",
                      "init_offset", "init_scale", "max_scale"):
                if hasattr(r, k):
                    kw[k] = getattr(r, k)
        if hasattr(getattr(cfg, "nerf", None), "bound"):
            kw["nerf_bound"] = float(cfg.nerf.bound)
        kw.update(learn_flags)
        n, dev = points.shape[0], points.device
        init_scale = float(kw.get("init_scale", 0.001))
        quaternions = torch.zeros(n, 4, device=dev)
        quaternions[:, 0] = 1.0                                  # matrix_to_quaternion(eye(3)): (w, x, y, z) = (1, 0, 0, 0)
        canonical = {k: (v.detach().to(dev) if torch.is_tensor(v) else v) for k, v in smpl_canonical_inputs.items()}
        av = cls(lbs_model, points, torch.full((n, 3), init_scale, device=dev), quaternions, lbs_weights, canonical, mesh,
                 nearest_vertex_indices=ntb['nearest_vertex_indices'], cfg=cfg, **kw).to(dev)
        with torch.no_grad():                                    # the blended inverse needs the avatar's own (normalised) weights
            av._positions.copy_(av.inverse_lbs_transform(points, av.lbs_model.forward(**canonical)[-1]))
        av.nearest_triangles_buffer = ntb
        av.cfg = cfg
        return av

    def __getattr__(self, name):
        # attributes of the adopted reference avatar that this mirror does not carry (canonical_vertices, canonical_triangles, ...)
        try:
            return super().__getattr__(name)
        except AttributeError:
            ref = self.__dict__.get("reference")
            if ref is not None and not name.startswith("_") and hasattr(ref, name):
                return getattr(ref, name)
            raise

    @property
    def device(self):
        return self._positions.device

    @property
    def densification_mask(self):
        return torch.cat([torch.ones(self._n_points, dtype=torch.bool), torch.zeros(self._n_points_on_mesh, dtype=torch.bool)])

    # -- GaussianModel accessors (gaussian_model.py:25-56) -------------------------------------------------------------------
    scale_activation = staticmethod(torch.exp)
    scale_inverse_activation = staticmethod(torch.log)
    color_activation = staticmethod(torch.sigmoid)
    opacity_activation = staticmethod(torch.sigmoid)
    rotation_activation = staticmethod(torch.nn.functional.normalize)

    def get_positions(self):
        return self._positions

    def get_scales(self, return_means=False):
        if return_means:
            return torch.exp(self._scales.mean(dim=-1, keepdim=True).expand(-1, 3))
        return torch.exp(self._scales)

    def get_quaternions(self):
        return torch.nn.functional.normalize(self._quaternions)

    @staticmethod
    def lbs_weight_activation(lbs_weights):
        return lbs_weights / lbs_weights.sum(dim=-1, keepdim=True)

    def get_lbs_weights(self):
        return self.lbs_weight_activation(self._lbs_weights)

    # -- checkpoints ------------------------------------------------------------------------------------------------
    def invalidate_caches(self):
        """Everything derived from parameters / buffers that a checkpoint load or an in-place edit may have changed."""
        self.cache_generation = getattr(self, "cache_generation", 0) + 1       # the trainer refills the caches on ONE stream (trainer._check_caches)
        self._canonical_cache = None
        self._frozen_cache = None
        self._canonical_vertices = {}
        self.nerf_encoder._host_offsets_py = None
        self.lbs_model._subsets = []
        self.lbs_model._last_forward = None          # keyed on the call's tensors only: the model's own betas / buffers may have changed
        for m in self.mesh_binding_gaussians.values():
            m._rebuild_topology()

    def reset_by_state_dict(self, state_dict, attribute_names=('_positions', '_scales', '_quaternions', '_lbs_weights')):
        """GaussianModel.reset_by_state_dict (gaussian_model.py:58-85, avatar.py:1254-1281): resize the per-Gaussian parameters to
        the checkpoint's Gaussian count before the plain copy."""
        if "_positions" not in state_dict:
            return
        n = state_dict["_positions"].shape[0]
        for name in attribute_names:
            cur = getattr(self, name, None)
            if cur is not None and name in state_dict and cur.shape[0] != n:
                new = torch.empty(n, *cur.shape[1:], dtype=cur.dtype, device=cur.device)
                setattr(self, name, nn.Parameter(new, requires_grad=cur.requires_grad))
        self._n_points = n

    def load_reference_state_dict(self, state_dict, prefix="avatar."):
        """Loads the avatar part of a reference checkpoint's `model` entry (trainer.py:238-259 saves {'train_step',
        'checkpoints', 'model': Scene.state_dict()}; the avatar sits under `avatar.` and, duplicated, `avatars.0.`).
        Returns (loaded keys, checkpoint keys with no counterpart here, our keys the checkpoint does not carry).  Call it
        BEFORE the parameters are re-homed into a flat optimizer buffer when the Gaussian count changes."""
        sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        self.reset_by_state_dict(sd)
        own = self.state_dict()
        loaded, unknown = [], []
        for k, v in sd.items():
            if k in own and tuple(own[k].shape) == tuple(v.shape):
                own[k].copy_(v.to(own[k].dtype))
                loaded.append(k)
            else:
                unknown.append(k)
        if "nerf_bound" in sd:
            self._nerf_bound_host = float(sd["nerf_bound"])
        missing = [k for k in own if k not in sd]
        self.invalidate_caches()
        return loaded, unknown, missing

    # -- LBS -----------------------------------------------------------------------------------------------------------
    def _joint_pose_A(self, transforms):
        """compose(J_pose_rigid, G_transl_offset).squeeze(0) (avatar.py:1441-1444) as one [J,4,4] tensor."""
        A = getattr(transforms, "A", None)
        if A is not None:
            return A
        return RigidTransform.compose(transforms['J_pose_rigid'], transforms['G_transl_offset']).SE3.reshape(-1, 4, 4)

    def lbs_transform(self, positions, transforms, lbs_weights=None, vertex_indices=None, quaternions=None):
        """avatar.py:1426-1462 (use_*_offsets False).  `lbs_weights=None` means "the avatar's own": the raw parameter is streamed
        once and its normalisation (get_lbs_weights, avatar.py:913-918) is fused into the kernel."""
        A = self._joint_pose_A(transforms)
        if lbs_weights is None:
            return lbs_ops.lbs_blend(A, self._lbs_weights, positions, quaternions, normalize_weights=True)
        return lbs_ops.lbs_blend(A, lbs_weights, positions, quaternions, normalize_weights=False)

    def inverse_lbs_transform(self, positions, transforms):
        """avatar.py:1377-1424, the 'Correct' branch: per-point inverse of the BLENDED matrix (checklist Q8); init-time only."""
        jt = RigidTransform(SE3=self._joint_pose_A(transforms)).weight(self.get_lbs_weights())
        return RigidTransform._inverse_transform_points(positions, R=jt.R, T=jt.T)

    def static_mlp_forward(self, enc, fix_opacities=False):
        oc = self.nerf_opacity_and_color_net(enc)
        colors = torch.sigmoid(oc[:, 1:])
        opacities = torch.ones_like(oc[:, :1]) if fix_opacities else torch.sigmoid(oc[:, :1])
        return colors, opacities

    def dynamic_mlp_forward(self, enc, body_pose):
        return self.nerf_scale_and_quaternion_net(enc, body_pose)

    def non_rigid_transform(self, gaussians: GaussianOutput) -> GaussianOutput:
        """avatar.py:1464-1498, default flags (element-wise torch; `animate` uses the fused kernel of assemble.hip instead)."""
        gaussians.positions = gaussians.positions + gaussians.offsets * self.init_offset
        gaussians.offsets = None
        gaussians.scales = self.get_scales() + gaussians.scales * self.init_scale        # keyed by non_rigid_ROTATION_mode (Q4)
        gaussians.quaternions = self.get_quaternions()
        return gaussians

    def forward(self):
        return self.animate(None)

    frozen_playback = False         # opt-in (Scene.forward_frames(frozen_avatar=True)): keep the pose-independent part of `animate` across frames
    _frozen_cache = None

    def _frozen_key(self):
        ts = list(self.parameters()) + list(self.buffers())
        return (optim.PARAM_EPOCH[0], getattr(self, "cache_generation", 0), self._nerf_bound_host,
                tuple((t.data_ptr(), t._version, tuple(t.shape)) for t in ts))

    def animate(self, smpl_observed_inputs: Optional[dict] = None) -> GaussianOutput:
        """avatar.py:1500-1588."""
        if smpl_observed_inputs is None:
            smpl_observed_inputs = self.smpl_canonical_inputs
        if self._canonical_cache is None:           # canonical inputs never change: cache the skeleton pass
            self._canonical_cache = self.lbs_model.forward(**self.smpl_canonical_inputs)
        _, cV, ctr = self._canonical_cache
        _, oV, otr = self.lbs_model.forward(**smpl_observed_inputs)
        positions = self._positions
        N = positions.shape[0]
        # Playback of a FROZEN avatar (opt-in: `frozen_playback`, gradients off): the canonical positions, their encoding and the static
        # network's colours / opacities do not depend on the pose -- they are kept from the previous frame while no parameter has changed
        # (key: the optimizers' step epoch, the cache generation, every parameter's / buffer's address and version counter).  The
        # reference recomputes them per frame (avatar.py:1500-1588); the values are the same bits either way.
        frozen_key = self._frozen_key() if (self.frozen_playback and not torch.is_grad_enabled() and not self.learn_betas
                                            and not (positions.is_cuda and torch.cuda.is_current_stream_capturing())) else None
        hit = frozen_key is not None and self._frozen_cache is not None and self._frozen_cache[0] == frozen_key
        canonical_positions = None if hit else self.lbs_transform(positions, ctr)
        if self.learn_betas:                         # avatar.py:1551-1553 (sub-stage 2.1: --render.learn_hand_betas True)
            _, cVb, _ = self.lbs_model.forward(**self.smpl_canonical_inputs, extra_betas=self._betas)
            _, oVb, _ = self.lbs_model.forward(**smpl_observed_inputs, extra_betas=self._betas)
        # mesh-bound parts first: their canonical positions go through the SAME encoder / static-MLP launches as the free
        # Gaussians (the reference calls the two networks once per part, avatar.py:1544-1583; the maths is row-wise, so one pass
        # over the concatenated rows gives the same values with half the launches and one table-gradient scatter)
        mesh_parts = []
        for name, gm in self.mesh_binding_gaussians.items():
            vc = gm.get_vertex_coords()
            with_betas = (name == 'hands' and self.learn_hand_betas) or (name == 'face' and self.learn_face_betas)
            if with_betas:
                cvc = cVb.squeeze(0).transform_points(vc, indices=gm.predefined_vertex_indices)
                ovc = oVb.squeeze(0).transform_points(vc, indices=gm.predefined_vertex_indices)
            else:
                cvc = self._canonical_vertices.get(name)
                if cvc is None:                      # canonical pose and the bound vertices are fixed: transform once
                    cvc = self._canonical_vertices[name] = cV.squeeze(0).transform_points(vc, indices=gm.predefined_vertex_indices)
                ovc = oV.squeeze(0).transform_points(vc, indices=gm.predefined_vertex_indices)
            mesh_parts.append(gm(cvc, ovc))          # (cpos, pos_m, sc_m, q_m): one HIP launch each way (csrc/meshbind.hip)
        if hit:
            enc_all, oc_all = self._frozen_cache[1], self._frozen_cache[2]
        else:
            # the encoder's input rows, gathered AND normalised ((x + bound) / (2 bound): GridEncoder.forward) by one launch
            (unit_cpos,) = asm_ops.concat_rows([[canonical_positions] + [mp[0] for mp in mesh_parts]], bound=self._nerf_bound_host)
            enc_all = self.nerf_encoder(unit_cpos, normalized=True)
            oc_all = self.nerf_opacity_and_color_net(enc_all)                  # static_mlp_forward (avatar.py:1283-1290), all rows
            self._frozen_cache = (frozen_key, enc_all, oc_all) if frozen_key is not None else None
        enc = enc_all[:N]
        body_pose = smpl_observed_inputs.get('body_pose')
        if body_pose is None:
            body_pose = torch.zeros(1, 63, device=positions.device)
        mlp_out = self.nerf_scale_and_quaternion_net(enc, body_pose, packed=True)      # dynamic_mlp_forward: [warp 3 | scaling 3 | rotation 4] per row
        # non_rigid_transform (avatar.py:1464-1498, default flags) + the sigmoid / exp / normalize activations: one HIP launch
        pos, scales, quats, col_all, op_all = asm_ops.assemble_packed(positions, mlp_out, self._scales, self._quaternions, oc_all,
                                                                      self.init_offset, self.init_scale)
        pos, quats = self.lbs_transform(pos, otr, quaternions=quats)
        if not mesh_parts:
            return GaussianOutput(positions=pos, opacities=op_all, colors=col_all, quaternions=quats, scales=scales)
        # merge_gaussians (gaussian_utils.py:56-68): colours / opacities already come out in the merged row order
        # (positions, quaternions and scales of the free and the mesh-bound rows: one launch for the three merged tensors)
        m_pos, m_quats, m_scales = asm_ops.concat_rows([[pos] + [mp[1] for mp in mesh_parts], [quats] + [mp[3] for mp in mesh_parts],
                                                        [scales] + [mp[2] for mp in mesh_parts]])
        return GaussianOutput(positions=m_pos, opacities=op_all, colors=col_all, quaternions=m_quats, scales=m_scales)

    # -- optimizers (avatar.py:1590-1635) --------------------------------------------------------------------------------
    # per-Gaussian opacity PARAMETERS do not exist on this avatar (avatar.py:1233-1244; its opacities come out of the MLP): the reference's
    # GaussianModel accessors then fail on None (gaussian_model.py:43-47), and so do these -- the densifier's prune / reset paths need
    # --render.densify_disable_prune / densify_disable_reset True for a DreamWaltzG avatar, there as here
    _opacities = None

    def get_opacities(self, return_ones=False):
        return torch.sigmoid(self._opacities.view(-1, 1)) if not return_ones else torch.ones_like(self._opacities.view(-1, 1))

    @staticmethod
    def opacity_inverse_activation(x):
        return torch.log(x / (1 - x))

    def get_densifier(self, cfg, optimizer):
        """avatar.py:230-235.  `optimizer`: the dict `get_optimizer(cfg)` returned (the flat buffers are resized as a whole), or its
        'avatar' entry as the reference passes it (`Trainer.init_gaussian_solvers`, trainer.py:600-603) -- then the dict is found through it."""
        from .densifier import build_densifier
        opts = optimizer if isinstance(optimizer, dict) else getattr(optimizer, "owner", None)
        if opts is None:
            raise ValueError("get_densifier needs the optimizer dict of get_optimizer(cfg) (or one of its entries)")
        return build_densifier(model=self, optimizers=opts, cfg=cfg)

    def get_optimizer(self, cfg):
        """Same dict of named optimizers as the reference: 'avatar' (GaussianOptimizer: positions / scales / quaternions with
        the exponential position schedule), 'lbs' (betas / lbs weights when learned), 'nerf' (encoder 10x, both MLPs), 'mesh_<part>'.
        Every one is a view of ONE flat fp32 parameter / gradient / moment buffer (optim.FlatAdam): the all-reduce operand of
        the multi-view step and the operand of the fused Adam kernel."""
        specs = {}
        iterations = cfg.optim.iters
        l = []
        if self._positions.requires_grad:
            l.append({'params': [self._positions], 'lr': cfg.render.position_lr_init, 'name': "positions"})
        if self._scales.requires_grad:
            l.append({'params': [self._scales], 'lr': cfg.render.scaling_lr, 'name': "scales"})
        if self._quaternions.requires_grad:
            l.append({'params': [self._quaternions], 'lr': cfg.render.rotation_lr, 'name': "quaternions"})
        if l:
            specs['avatar'] = optim.AdamSpec(l, eps=1e-15, gaussian=dict(
                iterations=iterations, position_lr_init=cfg.render.position_lr_init, position_lr_final=cfg.render.position_lr_final,
                position_lr_delay_mult=0.01, position_lr_max_steps=iterations * 2, scaling_lr=cfg.render.scaling_lr))
        pl = []
        if self.learn_lbs_weights:
            pl.append({'params': [self._lbs_weights], 'lr': cfg.render.lbs_lr})
        if self.learn_betas:
            pl.append({'params': [self._betas], 'lr': cfg.render.betas_lr})
        if pl:
            specs['lbs'] = optim.AdamSpec(pl, eps=1e-8)                       # torch.optim.Adam defaults (avatar.py:1616)
        nerf_lr = cfg.nerf.lr
        specs['nerf'] = optim.AdamSpec([
            {'params': list(self.nerf_encoder.parameters()), 'lr': nerf_lr * 10},
            {'params': list(self.nerf_opacity_and_color_net.parameters()), 'lr': nerf_lr},
            {'params': list(self.nerf_scale_and_quaternion_net.parameters()), 'lr': nerf_lr}], betas=(0.9, 0.99), eps=1e-15)
        for model_name, gm in self.mesh_binding_gaussians.items():
            specs.update(gm.get_optimizer(cfg=cfg, optimizer_name='mesh_' + model_name))
        return optim.build_flat_optimizers(specs, self._positions.device)
