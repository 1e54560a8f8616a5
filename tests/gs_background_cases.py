"""Helpers of the Gaussian scene background tests (boundary B24): a .ply writer used by the tests alone, generated 3DGS arrays in the
reference's layouts, and float64 restatements of the activations (core/gaussian/gaussian_model.py:35-56) and of the colour
(core/gaussian/gaussian_utils.py:12-17 get_colors over core/gaussian/spherical_harmonics.py:117-172 eval_sh)."""
import ctypes
import os
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STANDARD_ORDER = (["x", "y", "z", "nx", "ny", "nz"] + ["f_dc_%d" % i for i in range(3)] + ["f_rest_%d" % i for i in range(45)] + ["opacity"] +
                  ["scale_%d" % i for i in range(3)] + ["rot_%d" % i for i in range(4)])

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435]


def make_columns(n, seed=0, n_rest=45):
    """{property name: float32 [n]} of a 3DGS file: every column distinct, so that a swapped column shows."""
    r = np.random.RandomState(seed)
    names = [c for c in STANDARD_ORDER if not c.startswith("f_rest_")] + ["f_rest_%d" % i for i in range(n_rest)]
    return {c: r.uniform(-2.0, 2.0, size=n).astype(np.float32) for c in names}


def expected_tensors(cols, max_sh_degree=3):
    """The six arrays of GaussianModel.load_ply from the generating columns, in the reference's layouts (gaussian_model.py:106-147)."""
    n = len(cols["x"])
    k = (max_sh_degree + 1) ** 2 - 1
    st = lambda names: np.stack([cols[c] for c in names], axis=1) if names else np.zeros((n, 0), np.float32)      # noqa: E731
    rest = st(["f_rest_%d" % i for i in range(3 * k)]).reshape(n, 3, k)          # (P, F * SH_coeffs) -> (P, F, SH_coeffs except DC)
    return {"positions": st(["x", "y", "z"]), "sh_features_dc": st(["f_dc_0", "f_dc_1", "f_dc_2"])[:, None, :],
            "sh_features_rest": np.ascontiguousarray(rest.transpose(0, 2, 1)), "opacities": cols["opacity"][:, None],
            "scales": st(["scale_0", "scale_1", "scale_2"]), "quaternions": st(["rot_0", "rot_1", "rot_2", "rot_3"])}


def write_ply(path, cols, fmt="binary_little_endian", order=None, double=(), list_property=None, trailing_element=False, element="vertex"):
    """A PLY file with one `element` of the columns in `order` (default: the 3DGS order, restricted to the columns given); `double`: the
    columns stored as double; `list_property`: the name of a list property declared (header only: such a file must be refused before its
    data is read); `trailing_element`: a second element (faces) behind the first."""
    order = [c for c in (order or STANDARD_ORDER) if c in cols] + ([c for c in cols if c not in (order or STANDARD_ORDER)])
    n = len(next(iter(cols.values())))
    end = {"binary_little_endian": "<", "binary_big_endian": ">", "ascii": "="}[fmt]
    dtype = np.dtype([(c, end + ("f8" if c in double else "f4")) for c in order])
    rec = np.zeros(n, dtype=dtype)
    for c in order:
        rec[c] = cols[c]
    head = ["ply", "format %s 1.0" % fmt, "comment written by tests/gs_background_cases.py", "element %s %d" % (element, n)]
    head += ["property %s %s" % ("double" if c in double else "float", c) for c in order]
    if list_property:
        head.append("property list uchar int %s" % list_property)
    if trailing_element:
        head += ["element face 2", "property list uchar int vertex_indices"]
    head.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if fmt == "ascii":
            for row in rec:
                f.write((" ".join(repr(float(row[c])) if c in double else "%.9g" % float(row[c]) for c in order) + "\n").encode("ascii"))
            if trailing_element:
                f.write(b"3 0 1 2\n3 1 2 3\n")
        else:
            f.write(rec.tobytes())
            if trailing_element:
                f.write(np.array([3, 0, 1, 2, 3, 1, 2, 3], dtype=np.uint8).tobytes())
    return path


# ---- float64 restatements --------------------------------------------------------------------------------------------------------------
def activations64(logits, log_scales, quats, dc):
    """float64 of the SAME fp32 inputs: sigmoid, exp, F.normalize (eps 1e-12), clamp_min(C0 dc + 0.5, 0)."""
    lg, ls, q, d = (t.detach().cpu().double() for t in (logits, log_scales, quats, dc))
    return {"opacities": (1.0 / (1.0 + torch.exp(-lg))).reshape(-1, 1), "scales": torch.exp(ls),
            "quaternions": q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12), "colors": (C0 * d.reshape(-1, 3) + 0.5).clamp_min(0.0)}


def colors64(dc, rest, positions, camera, levels):
    """float64 get_colors(cat(dc, rest), F.normalize(positions - camera), levels) -> [N, 3]."""
    sh = torch.cat([dc.detach().cpu().double(), rest.detach().cpu().double()], dim=1)[:, :levels ** 2]          # [N, L^2, 3]
    v = positions.detach().cpu().double() - camera.detach().cpu().double().reshape(1, 3)
    d = v / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    x, y, z = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    basis = [torch.full_like(x, C0)]
    if levels > 1:
        basis += [-C1 * y, C1 * z, -C1 * x]
    if levels > 2:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        basis += [C2[0] * xy, C2[1] * yz, C2[2] * (2.0 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy)]
    if levels > 3:
        basis += [C3[0] * y * (3 * xx - yy), C3[1] * xy * z, C3[2] * y * (4 * zz - xx - yy), C3[3] * z * (2 * zz - 3 * xx - 3 * yy),
                  C3[4] * x * (4 * zz - xx - yy), C3[5] * z * (xx - yy), C3[6] * x * (xx - 3 * yy)]
    B = torch.cat(basis, dim=1)                                                   # [N, L^2]
    return ((B.unsqueeze(-1) * sh).sum(dim=1) + 0.5).clamp_min(0.0)


def ulps(got, ref64, floor=0.0):
    """max over the elements of |got - ref| in units of the fp32 spacing at max(|ref|, floor)."""
    ref = ref64.detach().cpu().double()
    mag = ref.abs().clamp_min(max(floor, float(np.finfo(np.float32).tiny))).float()
    spacing = torch.from_numpy(np.spacing(mag.numpy())).double()
    return float(((got.detach().cpu().double() - ref).abs() / spacing).max())


def scene_arrays(n, seed=0, box=1.2, rest=True):
    """A random scene around the origin as GaussianBackground.from_tensors takes it (CPU fp32): small Gaussians in a box."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)           # noqa: E731
    pos = (u(n, 3) * 2 - 1) * box                        # around (and through) an avatar at the origin: seen from every camera
    return dict(positions=pos, sh_features_dc=(u(n, 1, 3) * 4 - 2), sh_features_rest=((u(n, 15, 3) - 0.5) * (0.6 if rest else 0.0)),
                opacities=(u(n, 1) * 6 - 2), scales=(u(n, 3) * 1.5 - 4.5), quaternions=torch.randn(n, 4, generator=g))


# ---- the kernels' statements on the host ------------------------------------------------------------------------------------------------
def hostlib():
    """csrc/sh_math.h and csrc/scene_args.h compiled by gcc (tests/hostmath/sh_math_host.c): the statements the kernels run, on the host."""
    here = os.path.join(ROOT, "tests", "hostmath")
    src, out = os.path.join(here, "sh_math_host.c"), os.path.join(here, "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libsh_math_host.so")
    hdrs = [os.path.join(ROOT, "dreamwaltz-g_amd", "csrc", h) for h in ("sh_math.h", "scene_args.h")] + [os.path.join(ROOT, "include", "dwg_scene_gaussians.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror", "-o", so, src, "-lm"], check=True)
    L = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    L.host_scene_activate.argtypes = [ctypes.c_int64] + [vp] * 6
    L.host_scene_colors.argtypes = [ctypes.c_int64, ctypes.c_int] + [vp] * 5
    L.host_scene_check_merge.argtypes = [ctypes.c_int32, vp, ctypes.c_int32, ctypes.c_int64, vp, vp]
    return L


def host_colors(L, levels, positions, dc, rest, camera):
    """The colour rows [N, 3] of sh_levels `levels` from the host build, as a CPU tensor."""
    a = [np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32) for t in (positions, dc, rest, camera)]
    out = np.zeros((a[0].shape[0], 3), np.float32)
    L.host_scene_colors(a[0].shape[0], levels, *[x.ctypes.data_as(ctypes.c_void_p) for x in a + [out]])
    return torch.from_numpy(out)


def host_activations(L, logits, quats, dc):
    """(opacities [N, 1], quaternions [N, 4], DC colours [N, 3]) from the host build, as CPU tensors."""
    a = [np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32) for t in (logits, quats, dc)]
    n = a[0].shape[0]
    outs = [np.zeros((n, w), np.float32) for w in (1, 4, 3)]
    L.host_scene_activate(n, *[x.ctypes.data_as(ctypes.c_void_p) for x in a + outs])
    return tuple(torch.from_numpy(o) for o in outs)
