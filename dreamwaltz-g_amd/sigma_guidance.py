"""MI355X-native SMPL-X sigma guidance of the NeRF stage (boundary B8): the geometry of Trainer.calc_sigma_loss on the device.

  point_mesh_squared_distance(P, V, F)   -> (sqrD, I, C): libigl's point_mesh_squared_distance on device tensors (brute force)
  sample_surface(V, F, count, generator) -> (points, face_index, point_normals): trimesh's area-weighted sample_surface, with the point
                                            normals interpolated from trimesh's corner-angle-weighted vertex normals of (V, F)
  calc_sigma_loss(trainer, data, render_outputs, sd_inputs, selected_parts, wo_wrist=True)
                                         the reference method (core/trainer.py:718-825) with the geometry on csrc/sigma_guidance.hip and
                                         the field on whatever trainer.model binds (B7 when bound).  No host sync: the field runs on all
                                         N + N candidate points and the keep mask weights the loss terms, with device-side counts as the
                                         denominators -- equal to the reference's compacted points up to summation order.
Random numbers: one torch.rand((N, 4), dtype=float64) on the device (face pick, r1, r2, noise) from torch's CUDA generator; every
kernel is a pure function of that buffer.  The draws differ from trimesh's / numpy's, the distribution is the same.  No CPU fallback:
every tensor is checked (CUDA, dtype, shape) and a violation raises RuntimeError before any launch.
"""
import logging

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib

REC = _lib.CONSTANTS["DWG_SIGMA_FACE_RECORD_FLOATS"]
LOSS_TYPES = ('margin', 'mse', 'opacity_mse', 'opacity_ce')
_log = logging.getLogger(__name__)


class PartMesh:
    """Host-built topology of one part selection: the part faces on the device, the CSR table of incident (face, corner) pairs per
    vertex (ordered by face), and the per-part-face wrist byte.  Built once per selection and cached by calc_sigma_loss."""

    def __init__(self, faces, num_vertices, device, wrist=None, part_fids=None):
        f = np.ascontiguousarray(np.asarray(faces, dtype=np.int64).reshape(-1, 3))
        if len(f) and (f.min() < 0 or f.max() >= num_vertices):
            raise RuntimeError("part faces index vertices outside [0, %d)" % num_vertices)
        if len(f) >= 2 ** 31 // 3 or num_vertices >= 2 ** 31:
            raise RuntimeError("mesh too large for int32 indices")
        self.num_vertices, self.num_faces = int(num_vertices), len(f)
        vert = f.reshape(-1)
        order = np.argsort(vert, kind='stable')                       # items 3 f + c in increasing face order within each vertex
        offsets = np.zeros(num_vertices + 1, np.int64)
        np.cumsum(np.bincount(vert, minlength=num_vertices), out=offsets[1:])
        dev = torch.device(device)
        self.faces = torch.from_numpy(f.astype(np.int32)).to(dev)
        self.vf_offsets = torch.from_numpy(offsets.astype(np.int32)).to(dev)
        self.vf_items = torch.from_numpy(order.astype(np.int32)).to(dev)
        self.wrist = None if wrist is None else torch.from_numpy(np.asarray(wrist, dtype=np.uint8).reshape(-1)).to(dev)
        self.part_fids = part_fids
        if self.wrist is not None and self.wrist.numel() != self.num_faces:
            raise RuntimeError("wrist flags: %d for %d faces" % (self.wrist.numel(), self.num_faces))


def _prepare(V, part):
    """Face records, fp64 area CDF and vertex normals of the part mesh at vertices V [Vn, 3] fp32 (CUDA)."""
    L = _lib.lib()
    nv, nf = part.num_vertices, part.num_faces
    _lib.check_tensor("V", V, torch.float32, (nv, 3), contiguous=False)
    V = V.contiguous()
    dev, st = V.device, _lib.stream(V)
    rec = torch.empty((nf, REC), dtype=torch.float32, device=dev)
    area = torch.empty(nf, dtype=torch.float64, device=dev)
    cdf = torch.empty(nf, dtype=torch.float64, device=dev)
    vn = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    _lib.check(L.dwg_sigma_face_records(nv, _lib.ptr(V), nf, _lib.ptr(part.faces), _lib.ptr(rec), _lib.ptr(area), st), "dwg_sigma_face_records")
    _lib.check(L.dwg_sigma_area_cdf(nf, _lib.ptr(area), _lib.ptr(cdf), st), "dwg_sigma_area_cdf")
    _lib.check(L.dwg_sigma_vertex_normals(nv, _lib.ptr(V), _lib.ptr(part.faces), _lib.ptr(part.vf_offsets), _lib.ptr(part.vf_items), _lib.ptr(vn), st),
               "dwg_sigma_vertex_normals")
    return rec, cdf, vn


def _sample(V, part, cdf, vn, draws, noise_range):
    L = _lib.lib()
    n = draws.shape[0]
    _lib.check_tensor("draws", draws, torch.float64, (n, 4), contiguous=False)
    draws = draws.contiguous()
    dev = V.device
    pts = torch.empty((n, 3), dtype=torch.float32, device=dev)
    fid = torch.empty(n, dtype=torch.int32, device=dev)
    pn = torch.empty((n, 3), dtype=torch.float32, device=dev)
    noisy = torch.empty((n, 3), dtype=torch.float32, device=dev)
    if n:
        _lib.check(L.dwg_sigma_sample(n, _lib.ptr(draws), part.num_vertices, _lib.ptr(V), part.num_faces, _lib.ptr(part.faces), _lib.ptr(cdf), _lib.ptr(vn),
                                      float(noise_range), _lib.ptr(pts), _lib.ptr(fid), _lib.ptr(pn), _lib.ptr(noisy), _lib.stream(V)), "dwg_sigma_sample")
    return pts, fid, pn, noisy


def _distance(P, rec, closest_point=True):
    L = _lib.lib()
    n, nf = P.shape[0], rec.shape[0]
    dev = P.device
    d2 = torch.empty(n, dtype=torch.float32, device=dev)
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    C = torch.empty((n, 3), dtype=torch.float32, device=dev) if closest_point else None
    if n == 0:
        return d2, idx, C
    ws_bytes = L.dwg_sigma_distance_workspace_bytes(n, nf)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.check(L.dwg_sigma_point_mesh_distance(n, _lib.ptr(P), nf, _lib.ptr(rec), _lib.ptr(d2), _lib.ptr(idx), _lib.ptr(C), _lib.ptr(ws), ws_bytes, _lib.stream(P)),
               "dwg_sigma_point_mesh_distance")
    return d2, idx, C


def _keep_mask(d2, idx, thickness, wrist):
    L = _lib.lib()
    n = d2.shape[0]
    keep = torch.empty(n, dtype=torch.float32, device=d2.device)
    kept = torch.zeros(1, dtype=torch.int32, device=d2.device)
    nf = 0 if wrist is None else wrist.numel()
    if n:
        _lib.check(L.dwg_sigma_keep_mask(n, _lib.ptr(d2), _lib.ptr(idx), float(thickness), nf, _lib.ptr(wrist), _lib.ptr(keep), _lib.ptr(kept), _lib.stream(d2)),
                   "dwg_sigma_keep_mask")
    return keep, kept


def _mesh_args(V, F_):
    _lib.check_tensor("V", V, torch.float32, (None, 3), contiguous=False)
    _lib.check_tensor("F", F_, (torch.int32, torch.int64), (None, 3), contiguous=False)
    if F_.shape[0] == 0:
        raise RuntimeError("F has no faces")
    faces = F_.detach().cpu().numpy()                                     # igl / trimesh API: the index range is checked on the host
    return V.detach().contiguous(), PartMesh(faces, V.shape[0], V.device)


def point_mesh_squared_distance(P, V, F_):
    """(sqrD [N] fp32, I [N] int64, C [N, 3] fp32): for each row of P [N, 3] fp32 the squared distance to the mesh (V [Vn, 3] fp32,
    F [Fn, 3] int), the index of the closest face (ties: the lowest index among minima equal within 5e-7 (1 + d)) and the closest
    point.  Degenerate faces count as their segments."""
    _lib.check_tensor("P", P, torch.float32, (None, 3), contiguous=False)
    V, part = _mesh_args(V, F_)
    L = _lib.lib()
    rec = torch.empty((part.num_faces, REC), dtype=torch.float32, device=V.device)
    _lib.check(L.dwg_sigma_face_records(part.num_vertices, _lib.ptr(V), part.num_faces, _lib.ptr(part.faces), _lib.ptr(rec), None, _lib.stream(V)),
               "dwg_sigma_face_records")
    d2, idx, C = _distance(P.detach().contiguous(), rec)
    return d2, idx.long(), C


def sample_surface(V, F_, count, generator=None):
    """(points [count, 3] fp32, face_index [count] int64, point_normals [count, 3] fp32): area-weighted samples on (V, F) from
    torch.rand((count, 4), float64) on V's device (face pick, r1, r2; the fourth column is the noise draw of calc_sigma_loss)."""
    V, part = _mesh_args(V, F_)
    draws = torch.rand((int(count), 4), dtype=torch.float64, device=V.device, generator=generator)
    _, cdf, vn = _prepare(V, part)
    pts, fid, pn, _ = _sample(V, part, cdf, vn, draws, 0.0)
    return pts, fid.long(), pn


def guidance_points(V, part, draws, noise_range, thickness, wo_wrist=True):
    """The whole geometry of one call on the device: {points, face_index, point_normals, noisy, sqr_dist, closest_face, keep, kept}."""
    rec, cdf, vn = _prepare(V, part)
    pts, fid, pn, noisy = _sample(V, part, cdf, vn, draws, noise_range)
    d2, idx, _ = _distance(noisy, rec, closest_point=False)
    keep, kept = _keep_mask(d2, idx, thickness, part.wrist if wo_wrist else None)
    return {'points': pts, 'face_index': fid, 'point_normals': pn, 'noisy': noisy, 'sqr_dist': d2, 'closest_face': idx, 'keep': keep,
            'kept': kept}


# --------------------------------------------------------------------------------------------------------------------------------------
# the trainer method
# --------------------------------------------------------------------------------------------------------------------------------------
class _TruncExp(torch.autograd.Function):
    """exp with the gradient's exponent clamped to [-15, 15] (the reference's trunc_exp, core/nerf/nerf_utils.py)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        x, = ctx.saved_tensors
        return g * torch.exp(x.clamp(-15, 15))


trunc_exp = _TruncExp.apply

_PARTS = {}


def _parts_key(selected_parts):
    return tuple(selected_parts) if isinstance(selected_parts, (list, tuple)) else (selected_parts,)


def part_mesh(smpl_model, selected_parts, num_vertices, device):
    """The cached PartMesh of `selected_parts` (faces smpl_model.model.faces[part_fids], wrist bytes from get_semantic_indices(['wrists']))."""
    key = (id(smpl_model), _parts_key(selected_parts), int(num_vertices), str(device))
    hit = _PARTS.get(key)
    if hit is not None and hit[0] is smpl_model:
        return hit[1]
    part_fids = np.asarray(smpl_model.get_semantic_indices(select_parts=selected_parts)[1], dtype=np.int64).reshape(-1)
    faces = np.asarray(smpl_model.model.faces)[part_fids]
    wrist_fids = np.asarray(list(smpl_model.get_semantic_indices(select_parts=['wrists'])[1]), dtype=np.int64)
    wrist = np.isin(part_fids, wrist_fids)
    part = PartMesh(faces, num_vertices, device, wrist=wrist, part_fids=part_fids)
    _PARTS[key] = (smpl_model, part)
    return part


def _stats(logger, name, s):
    logger.info('%s: min=%.2f, max=%.2f, std=%.2f' % (name, s.min().item(), s.max().item(), s.std().item()))


def calc_sigma_loss(trainer, data, render_outputs, sd_inputs, selected_parts, wo_wrist=True, *, generator=None, logger=None, out=None):
    """Trainer.calc_sigma_loss on the device.  Returns the reference's dict: sigma_loss, and albedo_loss / normal_loss when their
    lambdas are positive.  `out` (a dict), when given, receives the geometry of the call (guidance_points' keys and xyzs)."""
    cfg = trainer.cfg
    loss_type = cfg.sigma_loss_type
    if loss_type not in LOSS_TYPES:
        raise RuntimeError("unknown sigma_loss_type %r" % (loss_type,))
    logger = logger or _log
    V = data['smpl_outputs'].vertices[0].detach()
    if V.dtype != torch.float32:
        V = V.float()
    V = V.contiguous()
    part = part_mesh(trainer.smpl_model, selected_parts, V.shape[0], V.device)
    n = part.num_faces if cfg.sigma_num_points < 0 else int(cfg.sigma_num_points)
    draws = torch.rand((n, 4), dtype=torch.float64, device=V.device, generator=generator)
    g = guidance_points(V, part, draws, cfg.sigma_noise_range, cfg.sigma_surface_thickness, wo_wrist=wo_wrist)
    xyzs = torch.cat((g['points'], g['noisy']), dim=0).to(sd_inputs)
    keep = g['keep'] > 0                                                  # negatives kept; positives are all kept
    k = g['kept'].to(torch.float32)
    if out is not None:
        out.update(g)
        out['xyzs'] = xyzs

    losses = {}
    if loss_type.startswith('opacity'):
        sigmas, albedos = trainer.model.common_forward(xyzs)
        opacities = 1.0 - trunc_exp(-cfg.sigma_guidance_delta * sigmas)
        pos, neg = opacities[:n], opacities[n:]
        if loss_type == 'opacity_ce':
            # ce_pq_loss(p, q) = sum -(p log clamp(q) + (1 - p) log clamp(1 - q)), clamp to [0.01, 0.99]; q = 1 / 0
            hi, lo = float(np.log(0.99)), float(np.log(0.01))
            ce_pos = -(pos * hi + (1 - pos) * lo)
            ce_neg = -(neg * lo + (1 - neg) * hi)
            sigma_loss = ce_pos.sum() + torch.where(keep, ce_neg, torch.zeros_like(ce_neg)).sum()
        else:
            e_neg = neg ** 2
            sigma_loss = (((pos - 1) ** 2).sum() + torch.where(keep, e_neg, torch.zeros_like(e_neg)).sum()) / (n + k)
    else:
        peak = cfg.sigma_guidance_peak
        sigmas, albedos = trainer.model.local_geometry_forward(xyzs)
        if loss_type == 'mse':
            e_neg = (sigmas[n:] + peak) ** 2
            sigma_loss = (((sigmas[:n] - peak) ** 2).sum() + torch.where(keep, e_neg, torch.zeros_like(e_neg)).sum()) / (n + k)
        else:
            m_neg = F.relu(sigmas[n:] + peak) ** 2
            m_pos = F.relu(peak - sigmas[:n]) ** 2
            sigma_loss = torch.where(keep, m_neg, torch.zeros_like(m_neg)).sum() / k + m_pos.mean()
    losses['sigma_loss'] = sigma_loss * cfg.lambda_sigma_sigma

    if cfg.lambda_sigma_albedo > 0.0:
        losses['albedo_loss'] = albedos[:n].var(dim=0).sum() * cfg.lambda_sigma_albedo

    if cfg.lambda_sigma_normal > 0.0:
        normals = trainer.model.normal(xyzs[:n])
        normals_gt = g['point_normals'].to(normals).detach()
        losses['normal_loss'] = (1.0 - (normals * normals_gt).sum(-1).abs()).mean() * cfg.lambda_sigma_normal

    if trainer.time_to_snapshot:
        _stats(logger, 'sigmas', torch.log(render_outputs['sigmas'].detach()))
        _stats(logger, '%s_mesh_sigmas' % (selected_parts,), sigmas[:n].detach())
        _stats(logger, '%s_empty_sigmas' % (selected_parts,), sigmas[n:].detach()[keep])
    return losses
