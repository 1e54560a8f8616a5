"""Several people on one condition image: the numpy restatement the tests of the *_people entry points compare against, built on
oracle/condition.py (whose one-person half is pinned on the reference's captured rows by tests/test_oracle_condition.py), and the
fixture they share.

Follows the reference with N = P people:
  utils/open3d.py:8-19                  one mesh per person in ONE ray casting scene -> ray_cast per mesh, min / argmin over the people
                                        (argmin = open3d's geometry_ids; numpy's argmin takes the lower person on equal t)
  core/human/smpl_condition.py:96-143   OcclusionCulling.__call__: per-group thresholds; with ignore_body_self_occlusion a body keypoint
                                        is kept only where the nearest hit is its OWN person's mesh (:132-135)
  core/human/open_pose.py:322-331       adaptive_draw_poses: the people drawn one after another on one canvas

Fixture: the ellipsoid, keypoints and cameras of tests/golden/reference_golden_r2_condition.npz, P = 3 copies translated by OFFSETS
(fp32-rounded).  The counts below were taken with this file alone, on the CPU."""
import functools
import os

import numpy as np

from oracle import condition as oc

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_golden_r2_condition.npz"))
OFFSETS = np.array([[0.0, 0.0, 0.0], [0.55, 0.0, 0.1], [-0.2, 0.05, -0.6]], dtype=np.float32)
CAMERAS = ("front", "side", "wide")
# camera -> (keypoints hidden by ANOTHER person, of 3 x 128; body keypoints hidden by another person; body keypoints hidden by their own mesh)
HIDDEN = {"front": (57, 6, 4), "side": (16, 0, 6), "wide": (113, 10, 1)}


def people_inputs(name, offsets=OFFSETS):
    """fp32-representable inputs (the C-ABI takes fp32 geometry and camera matrices): keypoints [P,128,3], vertices [P,V,3], triangles,
    extrinsic, size-adjusted intrinsics, W, H."""
    p = "cond.%s." % name
    f = lambda a: np.asarray(a, dtype=np.float32)          # noqa: E731
    W, H = [int(v) for v in G[p + "size"]]
    off = f(offsets)[:, None, :]
    kp = (f(G["cond.keypoints"])[None] + off).astype(np.float32)
    v = (f(G["cond.vertices"])[None] + off).astype(np.float32)
    return kp, v, G["cond.triangles"].astype(np.int32), f(G[p + "extrinsic"]), f(G[p + "intrinsics"]), W, H


def pose_keypoints_people(keypoints, vertices, triangles, extrinsic, intrinsics, width, height, use_occlusion_culling=True,
                          smpl_type="smplx", ignore_body_self_occlusion=False, thres_body=0.2, thres_face=0.02, thres_hand=0.2):
    """export_pose up to the drawing call for P people -> (rows [P,K,3] as oc.pose_keypoints gives them (NaN row = None),
    hit_person [P,K] (-1 = the ray hit nobody), details dict with t_far, t_hit, the per-person hit distances and the thresholds)."""
    kp = np.asarray(keypoints, dtype=np.float64)
    P, K = kp.shape[:2]
    ext = np.asarray(extrinsic, dtype=np.float64)
    R, T = ext[:3, :3], ext[:3, 3:4]
    cam = (R @ kp.reshape(-1, 3).T + T).T
    cam[cam[:, 2] < 0] = np.nan
    Km = np.asarray(intrinsics, dtype=np.float64)
    h = Km @ cam.T
    img = (h[:2] / h[2]).T.reshape(P, K, 2)
    dist = -np.ones((P, K))
    hit_person = -np.ones((P, K), dtype=np.int32)
    details = {}
    if use_occlusion_culling:
        center = (np.linalg.inv(R) @ (-T)).reshape(3)
        d = kp - center[None, None, :]
        t_far = np.linalg.norm(d, axis=2)
        d = d / t_far[..., None]
        per = np.stack([oc.ray_cast(center, d.reshape(-1, 3), vertices[q], triangles).reshape(P, K) for q in range(P)])      # [Q,P,K]
        t_hit = per.min(0)
        hit_person = np.where(np.isfinite(t_hit), per.argmin(0), -1).astype(np.int32)
        groups = oc.keypoint_groups(smpl_type)[:K]
        thr = np.choose(groups, [thres_body, thres_hand, thres_face])[None, :]
        occ = (t_far - t_hit) > thr
        if ignore_body_self_occlusion:
            own = np.arange(P)[:, None]
            occ = occ & ~((groups == 0)[None, :] & (hit_person == own))
        img[occ] = np.nan
        dist = t_far
        details = dict(t_far=t_far, t_hit=t_hit, per_person=per, thr=np.broadcast_to(thr, (P, K)), groups=groups)
    W, H = Km[0, 2] * 2, Km[1, 2] * 2
    out = np.concatenate([img[..., :1] / float(W), img[..., 1:] / float(H), dist[..., None]], axis=2)
    out[np.isnan(img).any(2)] = np.nan
    return out, hit_person, details


def draw_poses_people(rows, H, W, draw_body=True, draw_hand=True, draw_face=True, flip_LR=False):
    """adaptive_draw_poses for P people, hand_dist_thres=None: rows [P,128,>=2] (NaN = None) -> uint8 [H,W,3]; person 0 first."""
    rows = np.asarray(rows, dtype=np.float64)
    canvas = np.zeros((H, W, 3), dtype=np.uint8)
    br, bs, hr, ht, fr = oc.draw_sizes(H, W)
    nb, nh = oc.N_BODY, oc.N_HAND
    for person in rows:
        if draw_body:
            oc._draw_body(canvas, person[:nb], br, bs, flip_LR)
        if draw_hand and person.shape[0] > nb:
            oc._draw_hand(canvas, person[nb:nb + nh], hr, ht)
            oc._draw_hand(canvas, person[nb + nh:nb + 2 * nh], hr, ht)
        if draw_face and person.shape[0] > nb + 2 * nh:
            oc._draw_face(canvas, person[nb + 2 * nh:oc.N_KEYPOINTS], fr)
    return canvas


def kernel_rows(rows):
    """Oracle rows [...,3] (NaN = None) -> the kernels' layout [...,4] = (x / W, y / H, dist, valid)."""
    valid = ~np.isnan(rows[..., :1])
    return np.concatenate([np.nan_to_num(rows, nan=0.0), valid.astype(np.float64)], axis=-1)


@functools.lru_cache(maxsize=None)
def reference(name, ignore_body_self_occlusion):
    """The oracle's answer for one camera, computed once per session and shared (read-only arrays)."""
    kp, v, t, E, K, W, H = people_inputs(name)
    rows, hit, det = pose_keypoints_people(kp, v, t, E, K, W, H, ignore_body_self_occlusion=ignore_body_self_occlusion)
    for a in (rows, hit, *det.values()):
        a.setflags(write=False)
    return rows, hit, det


def hidden_counts(name):
    """(keypoints hidden by another person, body keypoints hidden by another person, body keypoints hidden by their own mesh)."""
    _, hit, det = reference(name, False)
    occ = (det["t_far"] - det["t_hit"]) > det["thr"]
    own = np.arange(hit.shape[0])[:, None]
    body = (det["groups"] == 0)[None, :]
    return int((occ & (hit != own)).sum()), int((occ & (hit != own) & body).sum()), int((occ & (hit == own) & body).sum())
