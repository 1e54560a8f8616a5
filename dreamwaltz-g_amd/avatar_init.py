"""MI355X-native avatar construction (boundary B11): the work the reference's DreamWaltzG.__init__ does between the NeRF stage's point
cloud and the first 3D-Gaussian step, on csrc/avatar_init.hip instead of libigl, pytorch3d and a torch loop.

  find_nearest_triangles(points, vertices, triangles, device=None)   the reference's dict (core/system/avatar.py:766-806): closest face,
                                            squared distance, barycentric coordinates, the face's vertex ids and the nearest vertex of
                                            every point.  sigma_guidance.point_mesh_squared_distance + dwg_avinit_barycentric; closest-face
                                            ties go to the lowest index within 5e-7 (1 + d), that kernel's documented rule
  knn_points(query_points, reference_points, K=3, device=None)       _KNN(dists, idx, knn=None) with a leading batch dimension, as
                                            avatar.py:24-34 returns pytorch3d's: exact K nearest by (squared distance, index)
  initialize_lbs_weights(lbs_weights_table, nearest_triangles_buffer, positions=None, smooth=False, smooth_K=None, smooth_N=None,
                         use_sqrt=True, valid_dist_threshold=0.01)   avatar.py:865-911: barycentric interpolation of the table, then
                                            smooth_N Jacobi sweeps over the smooth_K nearest neighbours
  prune_points_close_to_mesh(positions, nearest_triangles_buffer, predefined_triangle_indices, threshold=None)   avatar.py:808-830
No CPU fallback: every tensor is checked (CUDA, dtype, shape) and a violation raises RuntimeError before any launch.  A neighbour that lies
exactly on the mesh, or coincides with its point, makes the smoothing weights inf and the row NaN, as the reference's statements do.
"""
import collections
import logging

import torch

from . import _lib
from . import sigma_guidance as sg

KNN_MAX_K = _lib.CONSTANTS["DWG_AVINIT_KNN_MAX_K"]
_KNN = collections.namedtuple("_KNN", ["dists", "idx", "knn"])
_log = logging.getLogger(__name__)


def _detached(x):
    return x.detach() if isinstance(x, torch.Tensor) else x


def barycentric(closest_point, closest_face, vertices, faces):
    """(bary [N, 3] fp32, vertex_indices [N, 3] int32, nearest_vertex [N] int32) of closest points in their closest faces (int32)."""
    n = closest_point.shape[0] if isinstance(closest_point, torch.Tensor) and closest_point.dim() else 0
    _lib.check_tensor("closest_point", closest_point, torch.float32, (n, 3), contiguous=False)
    _lib.check_tensor("closest_face", closest_face, torch.int32, (n,), contiguous=False)
    _lib.check_tensor("vertices", vertices, torch.float32, (None, 3), contiguous=False)
    _lib.check_tensor("faces", faces, torch.int32, (None, 3), contiguous=False)
    dev = closest_point.device
    cp, cf, v, f = closest_point.contiguous(), closest_face.contiguous(), vertices.contiguous(), faces.contiguous()
    bary = torch.empty((n, 3), dtype=torch.float32, device=dev)
    vidx = torch.empty((n, 3), dtype=torch.int32, device=dev)
    near = torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        _lib.check(_lib.lib().dwg_avinit_barycentric(n, _lib.ptr(cp), _lib.ptr(cf), v.shape[0], _lib.ptr(v), f.shape[0], _lib.ptr(f), _lib.ptr(bary), _lib.ptr(vidx), _lib.ptr(near),
                                                     _lib.stream(cp)), "dwg_avinit_barycentric")
    return bary, vidx, near


def find_nearest_triangles(points, vertices, triangles, device=None):
    """The reference's nearest_triangles_buffer for points [N, 3] fp32 against the mesh (vertices [V, 3] fp32, triangles [F, 3] int), all
    on one HIP device: triangle_indices [N] and vertex_indices [N, 3] int64 on the CPU, squared_distances [N] and barycentric_coords
    [N, 3] fp32 on `device` (None: the points' device), nearest_vertex_indices [N] int64 on the CPU."""
    points, vertices, triangles = _detached(points), _detached(vertices), _detached(triangles)
    _lib.check_tensor("points", points, torch.float32, (None, 3), contiguous=False)
    _lib.check_tensor("vertices", vertices, torch.float32, (None, 3), contiguous=False)
    _lib.check_tensor("triangles", triangles, (torch.int32, torch.int64), (None, 3), contiguous=False)
    device = points.device if device is None else torch.device(device)
    d2, face, cp = sg.point_mesh_squared_distance(points, vertices, triangles)
    bary, vidx, near = barycentric(cp, face.to(torch.int32), vertices, triangles.to(torch.int32))
    return {
        'squared_distances': d2.to(device),
        'triangle_indices': face.cpu(),
        'vertex_indices': vidx.long().cpu(),
        'nearest_vertex_indices': near.long().cpu(),
        'barycentric_coords': bary.to(device),
    }


def knn(query, reference, K):
    """(idx [Nq, K] int32, d2 [Nq, K] fp32): the exact K nearest rows of reference [Nr, 3] to every row of query [Nq, 3], sorted by
    (squared distance, index)."""
    K = int(K)
    if K < 1 or K > KNN_MAX_K:
        raise RuntimeError("K = %d outside [1, %d]" % (K, KNN_MAX_K))
    _lib.check_tensor("query", query, torch.float32, (None, 3), contiguous=False)
    _lib.check_tensor("reference", reference, torch.float32, (None, 3), contiguous=False)
    if query.device != reference.device:
        raise RuntimeError("query and reference are on different devices")
    nq, nr = query.shape[0], reference.shape[0]
    if K > nr:
        raise RuntimeError("K = %d exceeds the %d reference points" % (K, nr))
    q, r = query.detach().contiguous(), reference.detach().contiguous()
    idx = torch.empty((nq, K), dtype=torch.int32, device=q.device)
    d2 = torch.empty((nq, K), dtype=torch.float32, device=q.device)
    if nq:
        _lib.check(_lib.lib().dwg_avinit_knn(nq, _lib.ptr(q), nr, _lib.ptr(r), K, _lib.ptr(idx), _lib.ptr(d2), _lib.stream(q)), "dwg_avinit_knn")
    return idx, d2


def knn_points(query_points, reference_points, K=3, device=None):
    """avatar.py:24-34 without pytorch3d: query_points [B, Nq, 3], reference_points [B, Nr, 3] fp32 on a HIP device ->
    _KNN(dists [B, Nq, K] fp32 squared, idx [B, Nq, K] int64, knn=None) on `device` (None: the queries' device)."""
    if int(K) < 1 or int(K) > KNN_MAX_K:
        raise RuntimeError("K = %d outside [1, %d]" % (int(K), KNN_MAX_K))
    _lib.check_tensor("query_points", query_points, torch.float32, (None, None, 3), contiguous=False)
    _lib.check_tensor("reference_points", reference_points, torch.float32, (None, None, 3), contiguous=False)
    if query_points.shape[0] != reference_points.shape[0]:
        raise RuntimeError("batch sizes differ: %d queries, %d references" % (query_points.shape[0], reference_points.shape[0]))
    device = query_points.device if device is None else torch.device(device)
    res = [knn(q, r, K) for q, r in zip(query_points, reference_points)]
    K = int(K)
    idx = torch.stack([i for i, _ in res]) if res else torch.empty((0, query_points.shape[1], K), dtype=torch.int32, device=query_points.device)
    d2 = torch.stack([d for _, d in res]) if res else torch.empty((0, query_points.shape[1], K), dtype=torch.float32, device=query_points.device)
    return _KNN(dists=d2.to(device), idx=idx.long().to(device), knn=None)


def lbs_interp(table, vertex_indices, bary):
    """einsum('nij,ni->nj', table[vertex_indices], bary): table [V, J] fp32, vertex_indices [N, 3] int32, bary [N, 3] fp32 -> [N, J]."""
    _lib.check_tensor("lbs_weights_table", table, torch.float32, (None, None), contiguous=False)
    n = vertex_indices.shape[0] if isinstance(vertex_indices, torch.Tensor) and vertex_indices.dim() else 0
    _lib.check_tensor("vertex_indices", vertex_indices, torch.int32, (n, 3), contiguous=False)
    _lib.check_tensor("barycentric_coords", bary, torch.float32, (n, 3), contiguous=False)
    t, vi, b = table.detach().contiguous(), vertex_indices.contiguous(), bary.detach().contiguous()
    out = torch.empty((n, t.shape[1]), dtype=torch.float32, device=t.device)
    if n and t.shape[1]:
        _lib.check(_lib.lib().dwg_avinit_lbs_interp(n, t.shape[1], t.shape[0], _lib.ptr(t), _lib.ptr(vi), _lib.ptr(b), _lib.ptr(out), _lib.stream(t)), "dwg_avinit_lbs_interp")
    return out


def knn_weights(idx, d2, mesh_d2, use_sqrt=True, low=0.01, high=None):
    """(knn_w [N, K], update_w [N]) of avatar.py:886-902 from a point's neighbours idx / d2 [N, K] and the points' squared mesh distances."""
    n = idx.shape[0] if isinstance(idx, torch.Tensor) and idx.dim() else 0
    _lib.check_tensor("idx", idx, torch.int32, (n, None), contiguous=False)
    k = idx.shape[1]
    _lib.check_tensor("d2", d2, torch.float32, (n, k), contiguous=False)
    _lib.check_tensor("mesh_d2", mesh_d2, torch.float32, (n,), contiguous=False)
    high = low if high is None else high
    if k < 1 or k > KNN_MAX_K or not high >= low:
        raise RuntimeError("K = %d outside [1, %d] or high < low" % (k, KNN_MAX_K))
    idx, d2, mesh_d2 = idx.contiguous(), d2.contiguous(), mesh_d2.contiguous()
    w = torch.empty((n, k), dtype=torch.float32, device=idx.device)
    u = torch.empty(n, dtype=torch.float32, device=idx.device)
    if n:
        _lib.check(_lib.lib().dwg_avinit_knn_weights(n, k, _lib.ptr(idx), _lib.ptr(d2), _lib.ptr(mesh_d2), int(bool(use_sqrt)), float(low), float(high), _lib.ptr(w),
                                                     _lib.ptr(u), _lib.stream(idx)), "dwg_avinit_knn_weights")
    return w, u


def smooth_sweeps(weights, idx, knn_w, update_w, iterations):
    """`iterations` Jacobi sweeps w' = (1 - u) w + u sum_k knn_w[k] w[idx[k]] of weights [N, J]; returns a new tensor."""
    n = weights.shape[0] if isinstance(weights, torch.Tensor) and weights.dim() else 0
    _lib.check_tensor("weights", weights, torch.float32, (n, None), contiguous=False)
    _lib.check_tensor("idx", idx, torch.int32, (n, None), contiguous=False)
    k = idx.shape[1]
    _lib.check_tensor("knn_w", knn_w, torch.float32, (n, k), contiguous=False)
    _lib.check_tensor("update_w", update_w, torch.float32, (n,), contiguous=False)
    iterations = int(iterations)
    if iterations < 0 or k < 1 or k > KNN_MAX_K:
        raise RuntimeError("iterations = %d < 0 or K = %d outside [1, %d]" % (iterations, k, KNN_MAX_K))
    w_in = weights.detach().contiguous()
    out = torch.empty_like(w_in)
    tmp = torch.empty_like(w_in) if iterations > 1 else None
    if n and w_in.shape[1]:
        _lib.check(_lib.lib().dwg_avinit_smooth(n, w_in.shape[1], k, _lib.ptr(idx.contiguous()), _lib.ptr(knn_w.contiguous()), _lib.ptr(update_w.contiguous()),
                                                _lib.ptr(w_in), _lib.ptr(tmp), _lib.ptr(out), iterations, _lib.stream(w_in)), "dwg_avinit_smooth")
    return out


@torch.no_grad()
def initialize_lbs_weights(lbs_weights_table, nearest_triangles_buffer, positions=None, smooth=False, smooth_K=None, smooth_N=None,
                           use_sqrt=True, valid_dist_threshold=0.01):
    """LBSUtils.initialize_lbs_weights (avatar.py:865-911) for the table lbs_model.lbs_weights [V, J] (fp32, HIP device): [N, J] fp32 on the
    table's device.  Smoothing asks for smooth_K + 1 neighbours of every point within `positions` and drops column 0, as the reference
    does (column 0 is the point itself unless an exact duplicate with a lower index precedes it)."""
    _lib.check_tensor("lbs_weights_table", lbs_weights_table, torch.float32, (None, None), contiguous=False)
    dev = lbs_weights_table.device
    vidx = nearest_triangles_buffer['vertex_indices'].to(device=dev, dtype=torch.int32)
    bary = nearest_triangles_buffer['barycentric_coords'].to(device=dev, dtype=torch.float32)
    weights = lbs_interp(lbs_weights_table, vidx, bary)
    if not smooth:
        return weights
    if smooth_K is None or smooth_N is None or positions is None:
        raise RuntimeError("smooth=True needs positions, smooth_K and smooth_N")
    positions = _detached(positions)
    _lib.check_tensor("positions", positions, torch.float32, (weights.shape[0], 3), contiguous=False)
    _log.info('Using K=%s, N=%s for LBS weight smoothing', smooth_K, smooth_N)
    idx, d2 = knn(positions.to(dev), positions.to(dev), int(smooth_K) + 1)
    idx, d2 = idx[:, 1:].contiguous(), d2[:, 1:].contiguous()
    mesh_d2 = nearest_triangles_buffer['squared_distances'].to(device=dev, dtype=torch.float32)
    w, u = knn_weights(idx, d2, mesh_d2, use_sqrt=use_sqrt, low=valid_dist_threshold)
    return smooth_sweeps(weights, idx, w, u, smooth_N)


def prune_points_close_to_mesh(positions, nearest_triangles_buffer, predefined_triangle_indices, threshold=None):
    """avatar.py:808-830: drops the points whose closest face is one of predefined_triangle_indices (and, with a threshold, lies closer
    than it), from positions and from every entry of the buffer (in place, as the reference does).  Returns (positions, buffer)."""
    n1 = positions.shape[0]
    tri = nearest_triangles_buffer['triangle_indices']
    prune = torch.isin(tri, torch.as_tensor(predefined_triangle_indices).to(tri.device))
    if threshold is not None:
        prune &= (nearest_triangles_buffer['squared_distances'] < threshold ** 2).to(prune.device)
    keep = ~prune
    positions = positions[keep.to(positions.device)]
    for k in nearest_triangles_buffer.keys():
        nearest_triangles_buffer[k] = nearest_triangles_buffer[k][keep.to(nearest_triangles_buffer[k].device)]
    _log.info('Pruned points close to the mesh-binding points: %d -> %d', n1, positions.shape[0])
    return positions, nearest_triangles_buffer
