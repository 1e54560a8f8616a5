"""Golden fixture of the reference's point-cloud export order (/root/reference/core/nerf/to_point_cloud.py:27-114): the reference's OWN
export_point_cloud and remove_points_inside_bboxes run on the CPU over a fake network whose density is an integer-valued function of the
lattice indices -> tests/golden/pointcloud_order.npz (recorded inputs and outputs only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/capture_golden_pointcloud.py       (build container only: needs /root/reference)

Inert stand-ins satisfy the imports (tests/golden/_ref_stubs.py); the statements that run are the reference's.  Two cases:
  r10s4   resolution 10, split 4: 27 chunks of 64 .. 8 points
  r5s8    resolution 5, split 8: a single chunk
Per case: `lattice` (the concatenated pts of every common_forward call: the reference's lattice order), `sigma` (the density per lattice
point, same order), `points / colors / normals / alphas` (the exported float64 arrays) and `removed.*` (the arrays after
remove_points_inside_bboxes with BOX)."""
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, HERE); sys.path.insert(0, "/root/reference")
from oracle import animate as oa  # noqa: E402
import _ref_stubs  # noqa: E402

THRESH = 4.5
BOX = [[-0.5, -0.5, -0.5], [0.5, 0.5, 0.1]]
CASES = {"r10s4": (10, 4), "r5s8": (5, 8)}


class FakeNetwork:
    """What export_point_cloud touches of its `self`, with a field that is exact in fp32."""

    def __init__(self, resolution):
        self.R = resolution
        self.grid_size = resolution
        self.cuda_ray = False
        self.mean_density = 0.0
        self.density_thresh = THRESH
        self.max_density = 1e9
        self.density_activation = lambda x: x
        self.aabb_train = torch.zeros(6)
        self.seen = []

    def update_extra_state(self):
        pass

    def _indices(self, pts):
        return torch.round((pts.double() + 1) / 2 * (self.R - 1)).long() if self.R > 1 else torch.zeros_like(pts).long()

    def common_forward(self, pts):
        self.seen.append(pts.clone())
        i = self._indices(pts)
        sigma = ((7 * i[:, 0] + 3 * i[:, 1] + 5 * i[:, 2]) % 11).float()
        albedo = torch.stack([(i[:, 0] % 4).float() / 4, (i[:, 1] % 8).float() / 8, (sigma + 1) / 16], -1)
        return sigma, albedo

    def normal(self, pts):
        i = self._indices(pts)
        axis = (i.sum(-1) % 3)
        sign = 1.0 - 2.0 * ((i[:, 0] + i[:, 2]) % 2).float()
        return torch.nn.functional.one_hot(axis, 3).float() * sign[:, None]


def main():
    _ref_stubs.install(oa)
    from core.nerf.to_point_cloud import export_point_cloud, remove_points_inside_bboxes
    out = {"thresh": np.array([THRESH]), "box": np.array(BOX)}
    for name, (R, split) in CASES.items():
        net = FakeNetwork(R)
        pc = export_point_cloud(net, resolution=None, split_size=split)
        lattice = torch.cat(net.seen).numpy()
        assert lattice.shape == (R ** 3, 3) and lattice.dtype == np.float32
        seen, net.seen = net.seen, []
        sigma = torch.cat([net.common_forward(p)[0] for p in seen]).numpy()
        out[name + ".resolution_split"] = np.array([R, split])
        out[name + ".lattice"] = lattice
        out[name + ".sigma"] = sigma
        for k in ("points", "colors", "normals", "alphas"):
            a = getattr(pc, k)
            assert a.dtype == np.float64
            out[name + "." + k] = np.array(a, copy=True)
        n = len(pc)
        pc = remove_points_inside_bboxes(pc, BOX)
        for k in ("points", "colors", "normals", "alphas"):
            out[name + ".removed." + k] = np.array(getattr(pc, k), copy=True)
        print(name, "chunks:", len(seen), "lattice:", R ** 3, "exported:", n, "after the box:", len(pc))
    np.savez_compressed(os.path.join(HERE, "pointcloud_order.npz"), **out)
    print("wrote", len(out), "arrays")


if __name__ == "__main__":
    main()
