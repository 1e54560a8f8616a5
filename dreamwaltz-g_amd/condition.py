"""OpenPose-style condition image of the posed body ON THE GPU -- host-side mirror of the reference's
`core/human/smpl_condition.py` (`SMPL2Condition`, `OcclusionCulling`) and `utils/open3d.py:8-19` (`build_ray_casting_scene`) for
condition types 'pose' / 'openpose', over `csrc/condition.hip` (include/dwg_condition.h), and for 'depth_raw' -- the condition of the
NeRF pretrain recipe (scripts/pretrain_nerf.sh) -- with `export_depth` / `export_normal_raw` (`utils/open3d.py:21-45` cast_rays) over
`csrc/depthmap.hip` (include/dwg_depthmap.h).

Same names, arguments and error behaviour as the reference seam; what differs, deliberately:
  * the "ray casting scene" is the mesh itself as it lies in HBM (no BVH is built for a mesh that moves every step);
  * `export_pose` returns a CUDA uint8 tensor [H, W, 3] (RGB, the reference's wire format) instead of a PIL image --
    `ConditionImage.to_pil()` gives the PIL image where one is wanted, `export_pose_chw` gives the float [1, 3, H, W] in [0, 1]
    that `ControlNetScoreDistillation.prepare_image` would make of it (controlnet.py:33-55 at equal size is the identity resize);
  * `export_depth(raw=True)` returns a `DepthMap` (fp32 [H, W] on the device; `np.asarray(depth_map)` gives the reference's array);
  * nothing here leaves the device: no `.cpu()`, no host synchronisation;
  * several people (`--prompt.num_person`; the reference adds one mesh per person to ONE open3d scene and reads `geometry_ids`) are a
    `PeopleScene` (`build_people_scene`): vertices [P,V,3] over one triangle topology.  Keypoints [P,K,3] / rows [P,128,4] give one image
    for all of them, person 0 drawn first; `export_depth` / `export_normal_raw` cast against the concatenated mesh.
There is no CPU fallback: CPU tensors raise."""
from typing import Optional

import numpy as np
import torch

from . import _lib

N_KEYPOINTS = _lib.CONSTANTS["DWG_COND_KEYPOINTS"]      # body 18 + hands 2 x 21 + face 51 + 17 (smpl_condition.py:22)
MAX_PEOPLE = _lib.CONSTANTS["DWG_COND_MAX_PEOPLE"]
DRAW_BODY, DRAW_HAND, DRAW_FACE, FLIP_LR = (_lib.CONSTANTS["DWG_COND_" + n] for n in ("DRAW_BODY", "DRAW_HAND", "DRAW_FACE", "FLIP_LR"))


class RayCastingScene:
    """Stands where open3d's RaycastingScene stands: vertices [V,3] fp32 + triangles [F,3] int32 on the device."""

    def __init__(self, vertices: torch.Tensor, triangles: torch.Tensor):
        if not vertices.is_cuda:
            raise RuntimeError("dreamwaltz_g_amd.condition runs on the GPU only (HIP kernels); got a CPU tensor")
        self.vertices = vertices.detach().reshape(-1, 3).float().contiguous()
        self.triangles = triangles.to(device=vertices.device, dtype=torch.int32).reshape(-1, 3).contiguous()


def build_ray_casting_scene(vertices, triangles) -> RayCastingScene:
    """utils/open3d.py:8-19 (one mesh; [1,V,3] or [V,3] vertices; triangles as a tensor or numpy array)."""
    if not torch.is_tensor(triangles):
        triangles = torch.as_tensor(np.asarray(triangles).astype(np.int32))
    if vertices.dim() == 3:
        if vertices.shape[0] != 1:
            raise NotImplementedError("one mesh per RayCastingScene; several people are a PeopleScene (build_people_scene)")
        vertices = vertices[0]
    return RayCastingScene(vertices, triangles)


class PeopleScene:
    """utils/open3d.py:8-19 with one mesh per person: vertices [P,V,3] fp32 + the triangles [F,3] int32 all P meshes share, on the device.
    `merged` is the same geometry as ONE mesh (vertices [P V,3], person p's triangles offset by p V), built on first use: what the
    per-pixel casts (export_depth, export_normal_raw) run against."""

    def __init__(self, vertices: torch.Tensor, triangles: torch.Tensor):
        if vertices.dim() != 3 or vertices.shape[-1] != 3:
            raise ValueError("build_people_scene takes vertices [P,V,3]; got %s" % (tuple(vertices.shape),))
        if not 1 <= vertices.shape[0] <= MAX_PEOPLE:
            raise ValueError("a condition image holds 1 to %d people; got %d" % (MAX_PEOPLE, vertices.shape[0]))
        if not vertices.is_cuda:
            raise RuntimeError("dreamwaltz_g_amd.condition runs on the GPU only (HIP kernels); got a CPU tensor")
        self.vertices = vertices.detach().float().contiguous()
        self.triangles = triangles.to(device=vertices.device, dtype=torch.int32).reshape(-1, 3).contiguous()
        self._merged = None

    @property
    def num_people(self) -> int:
        return int(self.vertices.shape[0])

    @property
    def merged(self) -> RayCastingScene:
        if self._merged is None:
            P, V = self.vertices.shape[:2]
            offsets = torch.arange(P, dtype=torch.int32, device=self.vertices.device) * V
            self._merged = RayCastingScene(self.vertices.reshape(P * V, 3), (self.triangles[None] + offsets[:, None, None]).reshape(-1, 3))
        return self._merged


def build_people_scene(vertices, triangles) -> PeopleScene:
    """build_ray_casting_scene for [P,V,3] vertices (utils/open3d.py:12-18: one add_triangles per person, same triangles)."""
    if not torch.is_tensor(triangles):
        triangles = torch.as_tensor(np.asarray(triangles).astype(np.int32))
    return PeopleScene(vertices, triangles)


def adjust_intrinsics_size(intrinsics: torch.Tensor, width: int, height: int) -> torch.Tensor:
    """data/camera/utils.py:233-242 on a copy ([..., 3, 3])."""
    k = intrinsics.clone()
    width_raw, height_raw = k[..., 0, 2] * 2, k[..., 1, 2] * 2
    k[..., 0, 0] = k[..., 0, 0] * (width / width_raw)
    k[..., 1, 1] = k[..., 1, 1] * (height / height_raw)
    k[..., 0, 2] = width / 2
    k[..., 1, 2] = height / 2
    return k


class OcclusionCulling:
    """smpl_condition.py:82-143: the keypoint groups and their thresholds; the rays are cast inside dwg_condition_keypoints."""

    def __init__(self, smpl_type: str, ignore_body_self_occlusion: bool = False) -> None:
        if smpl_type == 'smpl':
            self.face_indices = [0, 14, 15, 16, 17]
            self.hand_indices = []
            self.body_indices = [i for i in range(18) if i not in self.face_indices]
        elif smpl_type == 'smplx':
            self.face_indices = [0, 14, 15, 16, 17] + [i for i in range(18 + 21 * 2, 128)]
            self.hand_indices = [i for i in range(18, 18 + 21 * 2)]
            self.body_indices = [i for i in range(128) if (i not in self.face_indices) and (i not in self.hand_indices)]
        else:
            raise NotImplementedError
        # One person per image: every ray that hits anything hits that person's own mesh, so ignoring body SELF occlusion
        # (:132-135, the shipped default configs/__init__.py:445) means the body group is never culled.  With several people
        # (PeopleScene) the kernel keeps who was hit, and only a hit on the keypoint's own person is ignored.
        self.ignore_body_self_occlusion = ignore_body_self_occlusion
        self.thres_body, self.thres_face, self.thres_hand = 0.2, 0.02, 0.2          # __call__ defaults, :100-103
        self._groups = {}

    def groups(self, K: int, device) -> torch.Tensor:
        key = (K, str(device))
        if key not in self._groups:
            g = torch.zeros(K, dtype=torch.uint8)
            g[[i for i in self.hand_indices if i < K]] = 1
            g[[i for i in self.face_indices if i < K]] = 2
            self._groups[key] = g.to(device)
        return self._groups[key]


class ConditionImage:
    """uint8 [H, W, 3] RGB on the device, with the conversions the consumers of the reference's PIL image use."""

    def __init__(self, u8: torch.Tensor):
        self.u8 = u8

    def to_pil(self):
        from PIL import Image
        return Image.fromarray(self.u8.cpu().numpy())

    def to_chw(self) -> torch.Tensor:
        return (self.u8.permute(2, 0, 1).float() / 255.0).unsqueeze(0)


class DepthMap:
    """t_hit of one ray per pixel, fp32 [H, W] on the device (+inf = miss): what export_depth(raw=True) returns as an np.ndarray in the
    reference.  `np.asarray(m)` / `np.nan_to_num(m, ...)` download it, so the reference's own consumers work on it unchanged."""

    def __init__(self, t: torch.Tensor):
        self.t = t

    @property
    def shape(self):
        return tuple(self.t.shape)

    def to_numpy(self) -> np.ndarray:
        return self.t.detach().cpu().numpy()

    def __array__(self, dtype=None, copy=None):
        a = self.to_numpy()
        return a if dtype is None else a.astype(dtype, copy=False)


class SMPL2Condition:
    """smpl_condition.py:145-320 for condition_type 'pose' / 'openpose' / 'depth_raw'.  `cfg` carries draw_body_keypoints, draw_hand_keypoints,
    draw_face_landmarks, openpose_left_right_flip, use_occlusion_culling, smpl_type, ignore_body_self_occlusion (PromptConfig)."""

    def __init__(self, cfg) -> None:
        self.draw_body = cfg.draw_body_keypoints
        self.draw_hand = cfg.draw_hand_keypoints
        self.draw_face = cfg.draw_face_landmarks
        self.openpose_left_right_flip = cfg.openpose_left_right_flip
        if cfg.use_occlusion_culling:
            self.occlusion_culling = OcclusionCulling(cfg.smpl_type, cfg.ignore_body_self_occlusion)
        else:
            self.occlusion_culling = None
        self._ws = {}
        self._depth_ws = {}

    # -- the two launches ------------------------------------------------------------------------------------------------
    def pose_rows(self, keypoints: torch.Tensor, ray_casting_scene: Optional[RayCastingScene], extrinsic: torch.Tensor,
                  intrinsics: torch.Tensor) -> torch.Tensor:
        """export_pose up to the drawing call (smpl_condition.py:191-224): fp64 rows [K,4] = (x / W, y / H, dist, valid); [P,K,4] for
        keypoints [P,K,3] of several people or a PeopleScene (people_rows)."""
        if not keypoints.is_cuda:
            raise RuntimeError("dreamwaltz_g_amd.condition runs on the GPU only (HIP kernels); got a CPU tensor")
        if isinstance(ray_casting_scene, PeopleScene) or (keypoints.dim() == 3 and keypoints.shape[0] != 1):
            return self.people_rows(keypoints, ray_casting_scene, extrinsic, intrinsics)[0]
        if keypoints.dim() == 3:
            keypoints = keypoints[0]
        dev = keypoints.device
        kp = keypoints.detach().float().contiguous()
        K = int(kp.shape[0])
        ext = extrinsic.detach().to(dev).float().reshape(4, 4).contiguous()
        intr = intrinsics.detach().to(dev).float().reshape(3, 3).contiguous()
        rows = torch.empty(K, 4, dtype=torch.float64, device=dev)
        cull = self.occlusion_culling is not None
        oc = self.occlusion_culling
        if cull and ray_casting_scene is None:
            raise ValueError("occlusion culling needs the body mesh (build_ray_casting_scene)")
        p = _lib.ptr
        _lib.check(_lib.lib().dwg_condition_keypoints(
            K, p(kp), p(ext), p(intr), int(ray_casting_scene.vertices.shape[0]) if cull else 0,
            p(ray_casting_scene.vertices) if cull else None, int(ray_casting_scene.triangles.shape[0]) if cull else 0,
            p(ray_casting_scene.triangles) if cull else None, p(oc.groups(K, dev)) if cull else None,
            (float('inf') if oc.ignore_body_self_occlusion else oc.thres_body) if cull else 0.0, oc.thres_hand if cull else 0.0, oc.thres_face if cull else 0.0, 1 if cull else 0,
            p(rows), _lib.stream(dev)), "dwg_condition_keypoints")
        return rows

    def people_rows(self, keypoints: torch.Tensor, people_scene: Optional[PeopleScene], extrinsic: torch.Tensor,
                    intrinsics: torch.Tensor, return_hit_person: bool = False):
        """pose_rows for P people (smpl_condition.py:96-143 with N = P): keypoints [P,K,3] against all P meshes of the PeopleScene ->
        (fp64 rows [P,K,4], int32 [P,K] person the nearest hit belongs to (-1 = none; open3d's geometry_ids) | None)."""
        if keypoints.dim() == 2:
            keypoints = keypoints[None]
        if keypoints.dim() != 3 or keypoints.shape[-1] != 3:
            raise ValueError("keypoints are [P,K,3]; got %s" % (tuple(keypoints.shape),))
        P, K = int(keypoints.shape[0]), int(keypoints.shape[1])
        if not 1 <= P <= MAX_PEOPLE:
            raise ValueError("a condition image holds 1 to %d people; got %d" % (MAX_PEOPLE, P))
        cull = self.occlusion_culling is not None
        oc = self.occlusion_culling
        if cull and people_scene is None:
            raise ValueError("occlusion culling needs the body meshes (build_people_scene)")
        if people_scene is not None:
            if not isinstance(people_scene, PeopleScene):
                raise ValueError("keypoints of %d people need a PeopleScene (build_people_scene), not one mesh" % P)
            if people_scene.num_people != P:
                raise ValueError("keypoints of %d people against the meshes of %d" % (P, people_scene.num_people))
        if not keypoints.is_cuda:
            raise RuntimeError("dreamwaltz_g_amd.condition runs on the GPU only (HIP kernels); got a CPU tensor")
        dev = keypoints.device
        kp = keypoints.detach().float().contiguous()
        ext = extrinsic.detach().to(dev).float().reshape(4, 4).contiguous()
        intr = intrinsics.detach().to(dev).float().reshape(3, 3).contiguous()
        rows = torch.empty(P, K, 4, dtype=torch.float64, device=dev)
        hit = torch.empty(P, K, dtype=torch.int32, device=dev) if return_hit_person else None
        p = _lib.ptr
        _lib.check(_lib.lib().dwg_condition_keypoints_people(
            P, K, p(kp), p(ext), p(intr), int(people_scene.vertices.shape[1]) if cull else 0, p(people_scene.vertices) if cull else None,
            int(people_scene.triangles.shape[0]) if cull else 0, p(people_scene.triangles) if cull else None,
            p(oc.groups(K, dev)) if cull else None, oc.thres_body if cull else 0.0, oc.thres_hand if cull else 0.0,
            oc.thres_face if cull else 0.0, 1 if (cull and oc.ignore_body_self_occlusion) else 0, 1 if cull else 0, p(rows), p(hit),
            _lib.stream(dev)), "dwg_condition_keypoints_people")
        return rows, hit

    def draw(self, rows: torch.Tensor, height: int, width: int, out_u8: bool = True, out_chw: bool = False):
        """adaptive_draw_poses (open_pose.py:279-333) from the rows [128,4], or [P,128,4] for P people on one canvas (person 0 first)
        -> (uint8 [H,W,3] | None, float [1,3,H,W] | None)."""
        people = rows.dim() == 3
        if rows.shape[-2] != N_KEYPOINTS:
            raise ValueError("the OpenPose layout has 128 keypoints (body 18, hands 2 x 21, face 68); got %d" % rows.shape[-2])
        if people and not 1 <= rows.shape[0] <= MAX_PEOPLE:
            raise ValueError("a condition image holds 1 to %d people; got %d" % (MAX_PEOPLE, rows.shape[0]))
        if not rows.is_cuda:
            raise RuntimeError("dreamwaltz_g_amd.condition runs on the GPU only (HIP kernels); got a CPU tensor")
        dev = rows.device
        rows = rows.double().contiguous()
        L = _lib.lib()
        P = int(rows.shape[0]) if people else None
        key = (str(dev), height, width) if not people else (str(dev), height, width, P)
        if key not in self._ws:
            need = L.dwg_condition_people_workspace_bytes(P, height, width) if people else L.dwg_condition_workspace_bytes(height, width)
            self._ws[key] = torch.empty(max(int(need), 16), dtype=torch.uint8, device=dev)
        flags = ((DRAW_BODY if self.draw_body else 0) | (DRAW_HAND if self.draw_hand else 0) | (DRAW_FACE if self.draw_face else 0)
                 | (FLIP_LR if self.openpose_left_right_flip else 0))
        u8 = torch.empty(height, width, 3, dtype=torch.uint8, device=dev) if out_u8 else None
        chw = torch.empty(1, 3, height, width, dtype=torch.float32, device=dev) if out_chw else None
        p = _lib.ptr
        if people:
            _lib.check(L.dwg_condition_draw_people(P, height, width, p(rows), flags, p(u8) if out_u8 else None, p(chw) if out_chw else None,
                                                   p(self._ws[key]), _lib.stream(dev)), "dwg_condition_draw_people")
        else:
            _lib.check(L.dwg_condition_draw(height, width, p(rows), flags, p(u8) if out_u8 else None, p(chw) if out_chw else None,
                                            p(self._ws[key]), _lib.stream(dev)), "dwg_condition_draw")
        return u8, chw

    # -- the reference's methods -----------------------------------------------------------------------------------------
    def export_pose(self, keypoints, ray_casting_scene, **camera_params) -> ConditionImage:
        """smpl_condition.py:191-235; camera_params: extrinsic [4,4], intrinsics [3,3] (size-adjusted), width, height."""
        rows = self.pose_rows(keypoints, ray_casting_scene, camera_params['extrinsic'], camera_params['intrinsics'])
        u8, _ = self.draw(rows, camera_params['height'], camera_params['width'])
        return ConditionImage(u8)

    def export_pose_chw(self, keypoints, ray_casting_scene, **camera_params) -> torch.Tensor:
        """The same image as the float [1,3,H,W] in [0,1] ControlNet consumes (no uint8 / PIL round trip)."""
        rows = self.pose_rows(keypoints, ray_casting_scene, camera_params['extrinsic'], camera_params['intrinsics'])
        return self.draw(rows, camera_params['height'], camera_params['width'], out_u8=False, out_chw=True)[1]

    # -- the depth map (csrc/depthmap.hip) ---------------------------------------------------------------------------------
    def cast_depth(self, ray_casting_scene: RayCastingScene, extrinsic: torch.Tensor, intrinsics: torch.Tensor, height: int, width: int,
                   normals: bool = False, minmax: bool = False):
        """utils/open3d.py:21-45 cast_rays: one pinhole ray per pixel -> (t_hit fp32 [H,W], primitive normals fp32 [H,W,3] | None,
        workspace).  `minmax` leaves the extrema of 1 / t_hit in the workspace for `_depth_image(..., from_cast=True)`."""
        if isinstance(ray_casting_scene, PeopleScene):                    # every person's triangles in one mesh: the nearest of them all
            ray_casting_scene = ray_casting_scene.merged
        if not isinstance(ray_casting_scene, RayCastingScene):
            raise RuntimeError("dreamwaltz_g_amd.condition runs on the GPU only (HIP kernels); the scene is build_ray_casting_scene's")
        if not (torch.is_tensor(extrinsic) and torch.is_tensor(intrinsics)):
            raise RuntimeError("dreamwaltz_g_amd.condition runs on the GPU only (HIP kernels); the camera matrices are tensors")
        verts, tris = ray_casting_scene.vertices, ray_casting_scene.triangles
        dev = verts.device
        height, width = int(height), int(width)
        ext = extrinsic.detach().to(dev).float().reshape(4, 4).contiguous()
        intr = intrinsics.detach().to(dev).float().reshape(3, 3).contiguous()
        V, F = int(verts.shape[0]), int(tris.shape[0])
        L = _lib.lib()
        key = (str(dev), height, width, F)
        if key not in self._depth_ws:
            self._depth_ws[key] = torch.empty(max(int(L.dwg_depthmap_workspace_bytes(height, width, F)), 64), dtype=torch.uint8, device=dev)
        ws = self._depth_ws[key]
        t = torch.empty(height, width, dtype=torch.float32, device=dev)
        n = torch.empty(height, width, 3, dtype=torch.float32, device=dev) if normals else None
        p = _lib.ptr
        _lib.check(L.dwg_depthmap_cast(height, width, p(ext), p(intr), V, p(verts) if F else None, F, p(tris) if F else None, p(t), p(n),
                                       1 if minmax else 0, p(ws), ws.numel(), _lib.stream(dev)), "dwg_depthmap_cast")
        return t, n, ws

    def depth_image(self, t_hit: torch.Tensor, out_u8: bool = True, out_chw: bool = False, _ws=None):
        """export_depth's inverse + normalise + uint8 statements (smpl_condition.py:242-248) from a t_hit map [H,W] ->
        (uint8 [H,W,3] | None, float [1,3,H,W] | None)."""
        if not t_hit.is_cuda:
            raise RuntimeError("dreamwaltz_g_amd.condition runs on the GPU only (HIP kernels); got a CPU tensor")
        dev = t_hit.device
        t_hit = t_hit.detach().float().contiguous()
        H, W = int(t_hit.shape[0]), int(t_hit.shape[1])
        ws = _ws
        if ws is None:                                                   # the extrema are taken here; any workspace of this device will do
            key = (str(dev), "image")
            if key not in self._depth_ws:
                self._depth_ws[key] = torch.empty(64, dtype=torch.uint8, device=dev)
            ws = self._depth_ws[key]
        u8 = torch.empty(H, W, 3, dtype=torch.uint8, device=dev) if out_u8 else None
        chw = torch.empty(1, 3, H, W, dtype=torch.float32, device=dev) if out_chw else None
        p = _lib.ptr
        _lib.check(_lib.lib().dwg_depthmap_image(H, W, p(t_hit), 0 if _ws is None else 1, p(u8), p(chw), p(ws), ws.numel(), _lib.stream(dev)),
                   "dwg_depthmap_image")
        return u8, chw

    @staticmethod
    def _depth_flags(inverse, normalize):
        if not (inverse and normalize):
            raise NotImplementedError("export_depth(inverse=%r, normalize=%r): without both, the reference casts inf to uint8, which is "
                                      "platform-defined; only the defaults (and raw=True) are restated" % (inverse, normalize))

    def export_depth(self, ray_casting_scene, inverse=True, normalize=True, raw=False, **camera_params):
        """smpl_condition.py:237-249; camera_params as export_pose's.  raw=True -> DepthMap, else the ConditionImage."""
        if not raw:
            self._depth_flags(inverse, normalize)
        t, _, ws = self.cast_depth(ray_casting_scene, camera_params['extrinsic'], camera_params['intrinsics'], camera_params['height'],
                                   camera_params['width'], minmax=not raw)
        if raw:
            return DepthMap(t)
        return ConditionImage(self.depth_image(t, _ws=ws)[0])

    def export_depth_chw(self, ray_casting_scene, inverse=True, normalize=True, **camera_params) -> torch.Tensor:
        """The same image as the float [1,3,H,W] in [0,1] ControlNet consumes (the twin of export_pose_chw)."""
        self._depth_flags(inverse, normalize)
        t, _, ws = self.cast_depth(ray_casting_scene, camera_params['extrinsic'], camera_params['intrinsics'], camera_params['height'],
                                   camera_params['width'], minmax=True)
        return self.depth_image(t, out_u8=False, out_chw=True, _ws=ws)[1]

    def export_normal_raw(self, ray_casting_scene, raw=True, **camera_params) -> torch.Tensor:
        """smpl_condition.py:264-269 with raw=True: primitive normals fp32 [H,W,3] (zero where the ray misses)."""
        if not raw:
            raise NotImplementedError("export_normal_raw(raw=False): the reference casts negative floats to uint8 there, which is "
                                      "platform-defined")
        return self.cast_depth(ray_casting_scene, camera_params['extrinsic'], camera_params['intrinsics'], camera_params['height'],
                               camera_params['width'], normals=True)[1]

    def __call__(self, smpl_outputs, triangles, camera_params: dict, condition_type: str, condition_height: int,
                 condition_width: int):
        """smpl_condition.py:271-320 (numpy-style branch): 'pose' / 'openpose' -> ConditionImage, 'depth_raw' -> DepthMap."""
        if condition_type not in ('pose', 'openpose', 'depth_raw'):
            raise NotImplementedError("condition_type %r: the OpenPose skeleton image ('pose' / 'openpose') and the raw depth map "
                                      "('depth_raw') are native; 'depth', 'normal' and 'mesh' are not" % (condition_type,))
        extrinsic = camera_params['extrinsic'][0]
        intrinsics = camera_params['intrinsics'][0]
        assert extrinsic.dim() == 2 and extrinsic.numel() == 16
        assert intrinsics.dim() == 2 and intrinsics.numel() == 9
        intrinsics = adjust_intrinsics_size(intrinsics, width=condition_width, height=condition_height)
        vertices = smpl_outputs.vertices.detach()
        build_scene = build_people_scene if (vertices.dim() == 3 and vertices.shape[0] > 1) else build_ray_casting_scene      # num_person > 1
        if condition_type == 'depth_raw':
            return self.export_depth(build_scene(vertices, triangles), raw=True, intrinsics=intrinsics,
                                     extrinsic=extrinsic, width=condition_width, height=condition_height)
        scene = build_scene(vertices, triangles) if self.occlusion_culling is not None else None
        return self.export_pose(smpl_outputs.joints.detach(), scene, intrinsics=intrinsics, extrinsic=extrinsic, width=condition_width,
                                height=condition_height)
