"""Restatements for the tests of the point-cloud export (boundary B12, dreamwaltz_g_amd.pointcloud).

  restate_export(net, resolution, split_size, density_thresh, epsilon=1e-3)
        the reference's export loop (core/nerf/to_point_cloud.py:49-82 with nerf_model.py:146-169 for the normal) in torch ops over any
        object with common_forward / bound: chunk loops, custom_meshgrid, a CPU linspace moved to the device, the seven common_forward
        calls per chunk, latent_to_rgb, safe_normalize, nan_to_num, the per-chunk mask and the concatenation.  Returns fp32 device
        tensors (points, colors, normals, alphas[n, 1]) and (min_density, max_density).
  remove_inside(points, arrays, bboxes)
        float64 numpy restatement of remove_points_inside_bboxes' loop (to_point_cloud.py:95-114): the keep mask and the kept arrays.
  load_fixture()  tests/golden/pointcloud_order.npz (recorded from the reference's own functions by capture_golden_pointcloud.py)
"""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

DECODE = [[0.298, 0.207, 0.208], [0.187, 0.286, 0.173], [-0.158, 0.189, 0.264], [-0.184, -0.271, -0.473]]


def latent_to_rgb(albedos):
    assert albedos.ndim == 2 and albedos.size(1) in (3, 4)
    if albedos.shape[1] == 3:
        return albedos
    # albedos.matmul(decode_mat) stated product by product in k order: a BLAS picks its own order and contractions, elementwise torch
    # ops round every product and every sum once, which is an arithmetic two implementations can agree on bit for bit
    m = torch.tensor(DECODE, device=albedos.device)
    return ((albedos[:, 0:1] * m[0] + albedos[:, 1:2] * m[1]) + albedos[:, 2:3] * m[2]) + albedos[:, 3:4] * m[3]


def safe_normalize(x, eps=1e-20):
    return x / torch.sqrt(torch.clamp(torch.sum(x * x, -1, keepdim=True), min=eps))


def normal(net, x, epsilon=1e-3):
    b = net.bound
    s = []
    for axis in range(3):
        for sign in (1.0, -1.0):
            d = [0.00, 0.00, 0.00]
            d[axis] = sign * epsilon
            s.append(net.common_forward((x + torch.tensor([d], device=x.device)).clamp(-b, b))[0])
    n = - 0.5 * torch.stack([(s[0] - s[1]), (s[2] - s[3]), (s[4] - s[5])], dim=-1) / epsilon
    return torch.nan_to_num(safe_normalize(n))


@torch.no_grad()
def restate_export(net, resolution, split_size, density_thresh, epsilon=1e-3, device="cuda"):
    X = torch.linspace(-1, 1, resolution).split(split_size)
    Y = torch.linspace(-1, 1, resolution).split(split_size)
    Z = torch.linspace(-1, 1, resolution).split(split_size)
    out = {k: [] for k in ("points", "colors", "normals", "alphas")}
    lo, hi = float("inf"), float("-inf")
    for xs in X:
        for ys in Y:
            for zs in Z:
                xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing='ij')
                pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1).to(device)
                sigmas, albedos = net.common_forward(pts)
                sigmas = sigmas.reshape(-1, 1)
                albedos = latent_to_rgb(albedos)
                normals = normal(net, pts, epsilon)
                lo, hi = min(lo, sigmas.min().item()), max(hi, sigmas.max().item())
                valid = (sigmas > density_thresh).flatten()
                out["points"].append(pts[valid].float())
                out["colors"].append(albedos[valid].float())
                out["alphas"].append(sigmas[valid].float())
                out["normals"].append(normals[valid].float())
    return tuple(torch.cat(out[k], 0) for k in ("points", "colors", "normals", "alphas")) + ((lo, hi),)


def remove_inside(points, arrays, bboxes):
    """(mask, [a[mask] for a in arrays]) with the reference's loop over float64 points."""
    points = np.asarray(points, dtype=np.float64)
    mask = np.full(len(points), True, dtype=bool)
    if isinstance(bboxes[0][0], float):
        bboxes = [bboxes, ]
    for i, point in enumerate(points):
        for bbox in bboxes:
            min_corner = np.amin(bbox, axis=0)
            max_corner = np.amax(bbox, axis=0)
            if np.all(point >= min_corner) and np.all(point <= max_corner):
                mask[i] = False
                break
    return mask, [np.asarray(a)[mask] for a in arrays]


def load_fixture():
    return np.load(os.path.join(HERE, "golden", "pointcloud_order.npz"))


def u32(idx):
    """int64 values of an int32 tensor that holds uint32 bits."""
    return idx.long() & 0xFFFFFFFF
