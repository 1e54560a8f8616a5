"""MI355X-native point-cloud export of the NeRF stage (boundary B12): the hand-off from a trained density field to the avatar
constructor (B11), on csrc/nerf_field.hip + csrc/pointcloud.hip instead of seven field evaluations per lattice point, four host copies
per chunk and a Python loop over the points (core/nerf/to_point_cloud.py:27-114).

  export_point_cloud(encoder, sigma_net, sigma_scale, bound, *, resolution, split_size=128, density_thresh, ...)   -> PointCloud
  export_point_cloud_from(net, resolution=None, split_size=128, density_thresh=None)      the field of a reference-shaped network
  remove_points_inside_bboxes(pc, bboxes)        on a PointCloud (device) or a BasicPointCloud-shaped object (numpy); mutates and returns it
  PointCloud.to_basic(cls=None)                  the reference's BasicPointCloud layout: float64 numpy arrays holding the fp32 values

The density is evaluated once per lattice point (dwg_pc_lattice_sigma); only the survivors of the threshold get an albedo and the six
evaluations of the finite-difference normal.  The survivors come out in the reference's order (x, y, z chunks of split_size, row-major
inside a chunk).  One read-back (the survivor count with the density range, 12 bytes) is the only synchronisation.  The lower-level
functions (lattice_sigma, select_above, select_flags, lattice_points, fd_points, finish, outside_boxes) wrap one C entry point each.
No CPU fallback; nothing here records autograd state."""
import ctypes

import numpy as np
import torch

from . import _lib
from . import nerf

MINMAX_PAIRS = _lib.CONSTANTS["DWG_PC_MINMAX_PAIRS"]


class BasicPointCloud:
    """Stand-in for the reference's utils.point_cloud.BasicPointCloud: the same four attributes and __len__."""

    def __init__(self):
        self.points, self.colors, self.normals, self.alphas = np.empty((0, 3)), np.empty((0, 3)), np.empty((0, 3)), np.empty((0, 1))

    def __len__(self):
        return self.points.shape[0]

    def __repr__(self):
        return 'Point cloud object with %d points.' % len(self)


class PointCloud:
    """points, colors, normals [n, 3] and alphas [n, 1], fp32 on the device, in the reference's order; info: n_lattice, n_points,
    min_density, max_density (over the whole lattice) and density_thresh (the fp32 value compared against)."""

    def __init__(self, points, colors, normals, alphas, info=None):
        self.points, self.colors, self.normals, self.alphas = points, colors, normals, alphas
        self.info = dict(info or {})

    def __len__(self):
        return self.points.shape[0]

    def __repr__(self):
        return 'Point cloud object with %d points.' % len(self)

    def to_basic(self, cls=None):
        """The reference's container: float64 numpy arrays holding the fp32 values (it concatenates into np.empty((0, 3)), float64)."""
        out = (BasicPointCloud if cls is None else cls)()
        for k in ("points", "colors", "normals", "alphas"):
            setattr(out, k, getattr(self, k).detach().cpu().numpy().astype(np.float64))
        return out


def lattice_order(nx, ny, nz, split):
    """[nx ny nz, 3] int64 (ix, iy, iz) of every lattice point in the reference's order: the host mirror of csrc/pointcloud_index.h."""
    def chunks(n):
        return [np.arange(a, min(a + split, n)) for a in range(0, n, split)]
    out = []
    for xs in chunks(nx):
        for ys in chunks(ny):
            for zs in chunks(nz):
                g = np.stack(np.meshgrid(xs, ys, zs, indexing='ij'), -1).reshape(-1, 3)
                out.append(g)
    return np.concatenate(out, 0).astype(np.int64) if out else np.zeros((0, 3), np.int64)


def lattice_index(f, nx, ny, nz, split):
    """(ix, iy, iz) of the flat reference-order index f: csrc/pointcloud_index.h's arithmetic in Python integers."""
    sx, sy, sz = min(split, nx), min(split, ny), min(split, nz)
    xi, f = divmod(f, sx * ny * nz)
    cx = min(sx, nx - xi * sx)
    yi, f = divmod(f, cx * sy * nz)
    cy = min(sy, ny - yi * sy)
    zi, f = divmod(f, cx * cy * sz)
    cz = min(sz, nz - zi * sz)
    lx, f = divmod(f, cy * cz)
    ly, lz = divmod(f, cz)
    return xi * sx + lx, yi * sy + ly, zi * sz + lz


def _lattice_args(resolution, split_size):
    if int(resolution) != resolution or int(split_size) != split_size:
        raise ValueError("resolution and split_size must be integers, got %r and %r" % (resolution, split_size))
    resolution, split_size = int(resolution), int(split_size)
    if resolution < 1:
        raise ValueError("resolution must be at least 1, got %d" % resolution)
    if split_size < 1:
        raise ValueError("split_size must be at least 1, got %d" % split_size)
    if resolution ** 3 >= 1 << 32:
        raise ValueError("a lattice of %d^3 points does not fit the 32-bit indices (2^32 points or more)" % resolution)
    return resolution, min(split_size, resolution)


def axis_table(resolution, device):
    """torch.linspace(-1, 1, R) evaluated on the CPU, as the reference does, then moved."""
    return torch.linspace(-1, 1, resolution).to(device)


def lattice_sigma(spec, embeddings, sigma_scale, wb, ax, ay, az, split):
    """(sigma [nx ny nz] fp32 in the reference's order, minmax [MINMAX_PAIRS, 2] fp32 partials) of the field at the lattice."""
    for n, t in (("ax", ax), ("ay", ay), ("az", az)):
        _lib.check_tensor(n, t, torch.float32, (None,))
    M = ax.numel() * ay.numel() * az.numel()
    if M >= 1 << 32 or split < 1:
        raise ValueError("lattice of %d points (limit 2^32 - 1) / split %d" % (M, split))
    sigma = torch.empty(M, dtype=torch.float32, device=ax.device)
    minmax = torch.empty((MINMAX_PAIRS, 2), dtype=torch.float32, device=ax.device)
    d = spec.desc(embeddings, sigma_scale, wb)
    if M:
        _lib.check(_lib.lib().dwg_pc_lattice_sigma(ctypes.byref(d), _lib.ptr(ax), _lib.ptr(ay), _lib.ptr(az), ax.numel(), ay.numel(), az.numel(),
                                                   int(split), _lib.ptr(sigma), _lib.ptr(minmax), _lib.stream(ax)), "dwg_pc_lattice_sigma")
    return sigma, minmax


def _select(fn_name, M, args, device, capacity):
    """Common part of the two selections: (idx int32 [min(M, capacity)] holding uint32 bits, count int32 [1] on the device)."""
    capacity = M if capacity is None else int(capacity)
    if capacity < 0:
        raise ValueError("capacity must not be negative")
    idx = torch.empty(min(M, capacity), dtype=torch.int32, device=device)
    count = torch.zeros(1, dtype=torch.int32, device=device)
    if M:
        L = _lib.lib()
        nbytes = int(L.dwg_pc_select_workspace_bytes(M))
        ws = torch.empty(nbytes // 4, dtype=torch.int32, device=device)
        _lib.check(getattr(L, fn_name)(M, *args, _lib.ptr(idx) if idx.numel() else _lib.ptr(ws), min(M, capacity), _lib.ptr(count), _lib.ptr(ws),
                                       nbytes, _lib.stream(device)), fn_name)
    return idx, count


def select_above(values, thresh, capacity=None):
    """Indices i (ascending; int32 tensor holding uint32 bits) with values[i] > float32(thresh), and their count [1] on the device.
    With a capacity below the count only the first `capacity` indices are written; the count stays the full one."""
    _lib.check_tensor("values", values, torch.float32, (None,))
    if values.numel() >= 1 << 32:
        raise ValueError("select_above takes fewer than 2^32 values")
    return _select("dwg_pc_select_above", values.numel(), (_lib.ptr(values), float(np.float32(thresh))), values.device, capacity)


def select_flags(flags, capacity=None):
    """The same over a uint8 mask (flags[i] != 0)."""
    _lib.check_tensor("flags", flags, torch.uint8, (None,))
    if flags.numel() >= 1 << 32:
        raise ValueError("select_flags takes fewer than 2^32 flags")
    return _select("dwg_pc_select_flags", flags.numel(), (_lib.ptr(flags),), flags.device, capacity)


def lattice_points(idx, ax, ay, az, split):
    """[n, 3] fp32 coordinates of the flat reference-order indices idx [n] (int32 holding uint32 bits)."""
    _lib.check_tensor("idx", idx, torch.int32, (None,))
    for n, t in (("ax", ax), ("ay", ay), ("az", az)):
        _lib.check_tensor(n, t, torch.float32, (None,))
    if ax.numel() * ay.numel() * az.numel() >= 1 << 32 or split < 1:
        raise ValueError("lattice of 2^32 points or more, or split < 1")
    out = torch.empty((idx.numel(), 3), dtype=torch.float32, device=idx.device)
    if idx.numel():
        _lib.check(_lib.lib().dwg_pc_lattice_points(idx.numel(), _lib.ptr(idx), _lib.ptr(ax), _lib.ptr(ay), _lib.ptr(az), ax.numel(), ay.numel(),
                                                    az.numel(), int(split), _lib.ptr(out), _lib.stream(idx)), "dwg_pc_lattice_points")
    return out


def fd_points(points, eps, bound):
    """[6, n, 3]: clamp(points +- eps along x, y, z, -bound, bound) in the order +x, -x, +y, -y, +z, -z (nerf_model.py:149-154)."""
    _lib.check_tensor("points", points, torch.float32, (None, 3))
    out = torch.empty((6,) + tuple(points.shape), dtype=torch.float32, device=points.device)
    if points.shape[0]:
        _lib.check(_lib.lib().dwg_pc_fd_points(points.shape[0], _lib.ptr(points), float(np.float32(eps)), float(bound), _lib.ptr(out), _lib.stream(points)),
                   "dwg_pc_fd_points")
    return out


def finish(albedo, sig6, eps):
    """(colors [n, 3], normals [n, 3]) from albedo [n, 3 or 4] fp32 and the six shifted densities sig6 [6, n]."""
    n = albedo.shape[0] if isinstance(albedo, torch.Tensor) and albedo.dim() == 2 else 0
    _lib.check_tensor("albedo", albedo, torch.float32, (n, None))
    if albedo.shape[1] not in (3, 4):
        raise ValueError("albedo has %d channels; latent_to_rgb takes 3 or 4" % albedo.shape[1])
    _lib.check_tensor("sig6", sig6, torch.float32, (6, n))
    colors = torch.empty((n, 3), dtype=torch.float32, device=albedo.device)
    normals = torch.empty((n, 3), dtype=torch.float32, device=albedo.device)
    if n:
        _lib.check(_lib.lib().dwg_pc_finish(n, albedo.shape[1], _lib.ptr(albedo), _lib.ptr(sig6), float(np.float32(eps)), _lib.ptr(colors),
                                            _lib.ptr(normals), _lib.stream(albedo)), "dwg_pc_finish")
    return colors, normals


def outside_boxes(points, boxes):
    """keep [n] uint8: 0 where points [n, 3] fp32 lies inside any of boxes [nb, 2, 3] float64 (min corner, max corner), faces included."""
    _lib.check_tensor("points", points, torch.float32, (None, 3))
    _lib.check_tensor("boxes", boxes, torch.float64, (None, 2, 3))
    keep = torch.empty(points.shape[0], dtype=torch.uint8, device=points.device)
    if points.shape[0]:
        _lib.check(_lib.lib().dwg_pc_outside_boxes(points.shape[0], _lib.ptr(points), boxes.shape[0], _lib.ptr(boxes) if boxes.shape[0] else None,
                                                   _lib.ptr(keep), _lib.stream(points)), "dwg_pc_outside_boxes")
    return keep


def field_spec(encoder, sigma_net, sigma_scale, bound, density_activation='exp', density_prior='none', albedo_sigmoid=True, precision=None):
    """(spec, embeddings, sigma_scale [1], [w0, b0, w1, ...]) of a field, checked against dwg_nerf.h's limits and the export's (3 or 4
    albedo channels); ValueError when the kernels do not take it.  Launches nothing."""
    if precision is None:
        precision = nerf.autocast_precision()
    wb = []
    try:
        for lin in sigma_net.net:
            if lin.bias is None:
                raise RuntimeError("sigma_net layers must have a bias")
            wb += [lin.weight.detach(), lin.bias.detach()]
        if not isinstance(sigma_scale, torch.Tensor):
            raise RuntimeError("sigma_scale must be a tensor")
        spec = nerf.FieldSpec(encoder, sigma_net, bound, density_activation, density_prior, albedo_sigmoid, False, precision)
        emb, ss = encoder.embeddings.detach(), sigma_scale.detach().reshape(1)
        spec.check(torch.empty((0, 3), dtype=torch.float32, device=emb.device), emb, ss, wb)
        if spec.out_dim - 1 not in (3, 4):
            raise RuntimeError("the field has %d albedo channels; latent_to_rgb takes 3 or 4" % (spec.out_dim - 1))
        if not float(bound) > 0:
            raise RuntimeError("bound must be positive, got %r" % (bound,))
    except RuntimeError as e:
        raise ValueError(str(e)) from None
    return spec, emb, ss, wb


def field_forward(spec, embeddings, sigma_scale, wb, x):
    """(sigma [M] fp32, albedo [M, out_dim - 1]) of dwg_nerf_field_forward at x [M, 3], without autograd."""
    _lib.check_tensor("x", x, torch.float32, (None, 3))
    return nerf.field_forward(spec, embeddings, sigma_scale, wb, x)


@torch.no_grad()
def export_point_cloud(encoder, sigma_net, sigma_scale, bound, *, resolution, split_size=128, density_thresh, density_activation='exp',
                       density_prior='none', albedo_sigmoid=True, epsilon=1e-3, precision=None):
    """The reference's export_point_cloud for the grid-backbone field (encoder, sigma_net, sigma_scale, bound) on a HIP device: the points
    of the resolution^3 lattice over [-1, 1]^3 whose density exceeds density_thresh (strictly, compared in fp32), with their colours
    (albedo, latent_to_rgb when it has 4 channels), finite-difference normals (epsilon) and densities.  precision: None follows autocast
    (the reference's export runs without it: f32), 0 f32, 1 f16.  ValueError before any launch for a bad lattice or a field the kernels
    do not take."""
    resolution, split = _lattice_args(resolution, split_size)
    spec, emb, ss, wb = field_spec(encoder, sigma_net, sigma_scale, bound, density_activation, density_prior, albedo_sigmoid, precision)
    dev = emb.device
    thresh = float(np.float32(density_thresh))
    ax = axis_table(resolution, dev)
    M = resolution ** 3
    with torch.cuda.device(dev):
        sigma_all, minmax = lattice_sigma(spec, emb, ss, wb, ax, ax, ax, split)
        idx, count = select_above(sigma_all, thresh)
        head = torch.cat([count, minmax[:, 0].min().reshape(1).view(torch.int32), minmax[:, 1].max().reshape(1).view(torch.int32)]).cpu().numpy()
        n = int(head[:1].view(np.uint32)[0])
        lo, hi = (float(v) for v in head[1:].view(np.float32))
        info = {"n_lattice": M, "n_points": n, "min_density": lo, "max_density": hi, "density_thresh": thresh}
        del sigma_all
        if n == 0:
            z = lambda c: torch.empty((0, c), dtype=torch.float32, device=dev)       # noqa: E731
            return PointCloud(z(3), z(3), z(3), z(1), info)
        idx = idx[:n].clone()
        points = lattice_points(idx, ax, ax, ax, split)
        del idx
        sigma, albedo = nerf.field_forward(spec, emb, ss, wb, points)
        shifted = fd_points(points, epsilon, float(bound))
        sig6, _ = nerf.field_forward(spec, emb, ss, wb, shifted.view(-1, 3))
        del shifted, _
        colors, normals = finish(albedo.float() if albedo.dtype != torch.float32 else albedo, sig6.view(6, n), epsilon)
    return PointCloud(points, colors, normals, sigma.view(n, 1), info)


def export_point_cloud_from(net, resolution=None, split_size=128, density_thresh=None):
    """export_point_cloud for the field of a reference-shaped network (what nerf.bind_nerf_network binds): resolution defaults to
    net.grid_size, density_thresh to net.density_thresh.  ValueError with nerf.unbound_reason when the kernels do not cover the network."""
    reason = nerf.unbound_reason(net)
    if reason is not None:
        raise ValueError("the native export does not cover this network: %s" % reason)
    if resolution is None:
        resolution = net.grid_size
    if density_thresh is None:
        density_thresh = net.density_thresh
    return export_point_cloud(net.encoder, net.sigma_net, net.sigma_scale, net.bound, resolution=resolution, split_size=split_size,
                              density_thresh=density_thresh, density_activation=net.opt.density_activation,
                              density_prior=net.density_prior_type, albedo_sigmoid=not bool(getattr(net, "latent_mode", False)))


ACCEPTED_BOXES = "a single box [[x, y, z], [x, y, z]] of floats, or a sequence of boxes, each a [k, 3] array of corners (k >= 1)"


def parse_boxes(bboxes):
    """[nb, 2, 3] float64 (min corner, max corner) of what the reference's remove_points_inside_bboxes accepts: a single box is
    recognised by isinstance(bboxes[0][0], float), anything else is taken as a sequence of boxes; corners come in any order (amin / amax
    per box).  TypeError for any other nesting."""
    if isinstance(bboxes[0][0], float):
        bboxes = [bboxes, ]
    out = np.empty((len(bboxes), 2, 3), np.float64)
    for i, bbox in enumerate(bboxes):
        try:
            b = np.asarray(bbox, dtype=np.float64)
        except (TypeError, ValueError):
            b = None
        if b is None or b.ndim != 2 or b.shape[1] != 3 or b.shape[0] < 1:
            raise TypeError("bboxes[%d] is not a box; accepted: %s" % (i, ACCEPTED_BOXES))
        out[i, 0], out[i, 1] = np.amin(b, axis=0), np.amax(b, axis=0)
    return out


@torch.no_grad()
def remove_points_inside_bboxes(point_cloud, bboxes, device=None):
    """Drops the points inside any of bboxes (faces included, compared in float64) from all four arrays of point_cloud, which is mutated
    and returned as the reference does.  point_cloud: a PointCloud (device tensors; the survivors are gathered on the device) or a
    BasicPointCloud-shaped object of numpy arrays (its points must be fp32 values, as an exported cloud's are: TypeError otherwise)."""
    boxes = parse_boxes(bboxes)
    if isinstance(point_cloud, PointCloud):
        dev = point_cloud.points.device
        keep = outside_boxes(point_cloud.points.contiguous(), torch.from_numpy(boxes).to(dev))
        idx, count = select_flags(keep)
        idx = idx[:int(count.cpu().numpy().view(np.uint32)[0])].long()
        for k in ("points", "colors", "normals", "alphas"):
            setattr(point_cloud, k, getattr(point_cloud, k).index_select(0, idx))
        point_cloud.info["n_points"] = len(point_cloud)
        return point_cloud
    pts = np.asarray(point_cloud.points)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise TypeError("point_cloud.points must be [n, 3], got %s" % (pts.shape,))
    p32 = pts.astype(np.float32)
    if not np.array_equal(p32.astype(np.float64), pts.astype(np.float64)):
        raise TypeError("point_cloud.points holds values that are not fp32 numbers; the device test takes fp32 points")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    keep = outside_boxes(torch.from_numpy(np.ascontiguousarray(p32)).to(dev), torch.from_numpy(boxes).to(dev))
    mask = keep.cpu().numpy().astype(bool)
    point_cloud.points = point_cloud.points[mask]
    point_cloud.colors = point_cloud.colors[mask]
    point_cloud.normals = point_cloud.normals[mask]
    point_cloud.alphas = point_cloud.alphas[mask]
    return point_cloud
