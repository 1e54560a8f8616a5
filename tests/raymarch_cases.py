"""CPU restatement of the NeRF-stage ray marcher (boundary B6) and scene builders, in numpy.

Written from the semantics of /root/reference/core/nerf/raymarching/rgb/src/raymarching.cu (cited by line); nothing here reads the
reference.  The marching arithmetic is float32 with every operation rounded separately (the kernels compile with FP contraction off),
so per-ray sample counts and positions are comparable exactly; the compositing restatement is float64.
"""
import numpy as np

f32 = np.float32
SQRT3 = f32(1.7320508075688772)
FLT_MAX = np.finfo(np.float32).max


def _fmin(a, b):
    return np.fmin(a, b)          # fminf: a NaN operand yields the other one


def _fmax(a, b):
    return np.fmax(a, b)


def _clamp(x, lo, hi):
    return _fmin(hi, _fmax(lo, x))


# ----------------------------------------------------------------------------------------------------------------------------------
# utils (:92-300)
# ----------------------------------------------------------------------------------------------------------------------------------
def near_far(rays_o, rays_d, aabb, min_near):
    """slab test (:108-144): a miss gives near = far = FLT_MAX, near clamped up to min_near"""
    o, d, a = rays_o.astype(f32), rays_d.astype(f32), np.asarray(aabb, dtype=f32)
    with np.errstate(all="ignore"):
        rd = f32(1) / d

        def slab(k):
            lo, hi = (a[k] - o[:, k]) * rd[:, k], (a[k + 3] - o[:, k]) * rd[:, k]
            sw = lo > hi
            return np.where(sw, hi, lo), np.where(sw, lo, hi)
        near, far = slab(0)
        ny, fy = slab(1)
        miss = (near > fy) | (ny > far)
        near = np.where(ny > near, ny, near)
        far = np.where(fy < far, fy, far)
        nz, fz = slab(2)
        miss |= (near > fz) | (nz > far)
        near = np.where(nz > near, nz, near)
        far = np.where(fz < far, fz, far)
        near = np.where(near < f32(min_near), f32(min_near), near)
    near = np.where(miss, FLT_MAX, near).astype(f32)
    far = np.where(miss, FLT_MAX, far).astype(f32)
    return near, far


def _expand_bits(v):
    v = v.astype(np.uint32)
    v = (v * np.uint32(0x00010001)) & np.uint32(0xFF0000FF)
    v = (v * np.uint32(0x00000101)) & np.uint32(0x0F00F00F)
    v = (v * np.uint32(0x00000011)) & np.uint32(0xC30C30C3)
    v = (v * np.uint32(0x00000005)) & np.uint32(0x49249249)
    return v


def morton3d(x, y, z):
    return _expand_bits(x) | (_expand_bits(y) << np.uint32(1)) | (_expand_bits(z) << np.uint32(2))


def _compact_bits(x):
    x = x.astype(np.uint32) & np.uint32(0x49249249)
    x = (x | (x >> np.uint32(2))) & np.uint32(0xC30C30C3)
    x = (x | (x >> np.uint32(4))) & np.uint32(0x0F00F00F)
    x = (x | (x >> np.uint32(8))) & np.uint32(0xFF0000FF)
    x = (x | (x >> np.uint32(16))) & np.uint32(0x0000FFFF)
    return x


def morton3d_invert(idx):
    idx = np.asarray(idx).astype(np.uint32)
    return np.stack([_compact_bits(idx), _compact_bits(idx >> np.uint32(1)), _compact_bits(idx >> np.uint32(2))], -1).astype(np.int32)


def packbits(grid, thresh):
    """bit i of byte j = grid[8j+i] > thresh (:268-289)"""
    b = (np.asarray(grid, dtype=f32).reshape(-1, 8) > f32(thresh)).astype(np.uint32)
    return (b << np.arange(8, dtype=np.uint32)).sum(1).astype(np.uint8)


# ----------------------------------------------------------------------------------------------------------------------------------
# marching (:385-464, :751-827)
# ----------------------------------------------------------------------------------------------------------------------------------
def _mip(mx, C):
    e = np.frexp(mx)[1].astype(f32)
    return _fmin(f32(C - 1), _fmax(f32(0), e)).astype(np.int64)


class _Marcher:
    def __init__(self, rays_o, rays_d, bitfield, bound, contract, dt_gamma, max_steps, C, H):
        self.o, self.d = rays_o.astype(f32), rays_d.astype(f32)
        with np.errstate(divide="ignore"):
            self.rd = f32(1) / self.d
        self.bits = np.asarray(bitfield, dtype=np.uint8)
        self.bound, self.contract, self.g = f32(bound), bool(contract), f32(dt_gamma)
        self.C, self.H, self.Hf = C, H, f32(H)
        self.dt_min = f32(2) * SQRT3 / f32(max_steps)
        self.dt_max = f32(2) * SQRT3 * f32(bound) / f32(H)
        self.rH = f32(1) / f32(H)

    def start(self, t0, noise):
        t0 = t0.astype(f32)
        return t0 + _clamp(t0 * self.g, self.dt_min, self.dt_max) * noise.astype(f32)

    def iterate(self, ii, t):
        """one loop iteration for rays ii at t -> (new t, occupied, cx, cy, cz, dt of the sample)"""
        o, d, rd, b = self.o[ii], self.d[ii], self.rd[ii], self.bound
        x = _clamp(o[:, 0] + t * d[:, 0], -b, b)
        y = _clamp(o[:, 1] + t * d[:, 1], -b, b)
        z = _clamp(o[:, 2] + t * d[:, 2], -b, b)
        dt = _clamp(t * self.g, self.dt_min, self.dt_max)
        mag = _fmax(np.abs(x), _fmax(np.abs(y), np.abs(z)))
        level = np.maximum(_mip(mag, self.C), _mip(dt * self.Hf * f32(0.5), self.C))
        mip_bound = _fmin(np.ldexp(f32(1), level).astype(f32), b)
        mip_rbound = f32(1) / mip_bound
        outside = (mag > f32(1)) if self.contract else np.zeros(len(ii), bool)
        with np.errstate(all="ignore"):
            s = (f32(2) - f32(1) / mag) / mag
        cx, cy, cz = (np.where(outside, c * s, c).astype(f32) for c in (x, y, z))
        n = [(_clamp(f32(0.5) * (c * mip_rbound + f32(1)) * self.Hf, f32(0), self.Hf - f32(1))).astype(np.int64) for c in (cx, cy, cz)]
        index = level * self.H ** 3 + morton3d(n[0], n[1], n[2]).astype(np.int64)
        occ = ((self.bits[index >> 3] >> (index & 7).astype(np.uint8)) & 1).astype(bool)
        t_occ = t + dt
        # empty cell, no contraction: step dt until the next voxel boundary (:454-463)
        with np.errstate(all="ignore"):
            tq = []
            for k, c in enumerate((cx, cy, cz)):
                sg = np.copysign(f32(1), d[:, k]).astype(f32)
                tq.append((((n[k].astype(f32) + f32(0.5)) + f32(0.5) * sg) * self.rH * f32(2) - f32(1)) * mip_bound - c)
            tt = t + _fmax(f32(0), _fmin(tq[0] * rd[:, 0], _fmin(tq[1] * rd[:, 1], tq[2] * rd[:, 2])))
        skip = ~occ & ~outside
        t_new = np.where(occ | outside, t_occ, t)
        ts = t.copy()
        todo = skip.copy()
        while todo.any():
            dtk = _clamp(ts * self.g, self.dt_min, self.dt_max)
            ts = np.where(todo, ts + dtk, ts)
            todo = todo & (ts < tt)
        t_new = np.where(skip, ts, t_new).astype(f32)
        return t_new, occ, cx, cy, cz, dt


def march_train(rays_o, rays_d, bitfield, bound, contract, dt_gamma, max_steps, C, H, nears, fars, noises):
    """-> counts [N], xyzs [M,3], dirs [M,3], ts [M,2] in ray-major order (the kernels' layout: offsets = exclusive prefix sum)"""
    mr = _Marcher(rays_o, rays_d, bitfield, bound, contract, dt_gamma, max_steps, C, H)
    N = len(rays_o)
    far = fars.astype(f32)
    t = mr.start(nears, noises)
    step = np.zeros(N, np.int64)
    rec = []
    act = (t < far) & (step < max_steps)
    while act.any():
        ii = np.nonzero(act)[0]
        tn, occ, cx, cy, cz, dt = mr.iterate(ii, t[ii])
        t[ii] = tn
        j = ii[occ]
        rec.append(np.stack([j.astype(np.float64), step[j].astype(np.float64), cx[occ], cy[occ], cz[occ], tn[occ], dt[occ]], 1))
        step[j] += 1
        act = (t < far) & (step < max_steps)
    counts = step
    if rec:
        R = np.concatenate(rec, 0)
        R = R[np.lexsort((R[:, 1], R[:, 0]))]
    else:
        R = np.zeros((0, 7))
    ray = R[:, 0].astype(np.int64)
    xyzs = R[:, 2:5].astype(f32)
    dirs = mr.d[ray]
    ts = R[:, 5:7].astype(f32)
    return counts.astype(np.int32), xyzs, dirs, ts


# ----------------------------------------------------------------------------------------------------------------------------------
# compositing (float64; :541-569 forward, :652-694 backward)
# ----------------------------------------------------------------------------------------------------------------------------------
def _alpha(sig, dt, binarize):
    a = 1.0 - np.exp(-sig * dt)
    return (a > 0.5).astype(np.float64) if binarize else a


def composite_forward(sigmas, rgbs, ts, rays, T_thresh, binarize=False):
    """-> weights [M], weights_sum [N], depth [N], image [N,C], stop [N] (number of composited samples per ray)"""
    sig, rgb, ts = (np.asarray(a, dtype=np.float64) for a in (sigmas, rgbs, ts))
    M, N, C = len(sig), len(rays), rgb.shape[1]
    w = np.zeros(M); ws = np.zeros(N); dep = np.zeros(N); img = np.zeros((N, C)); used = np.zeros(N, np.int64)
    for n in range(N):
        off, cnt = int(rays[n, 0]), int(rays[n, 1])
        if cnt == 0 or off + cnt > M:
            continue
        s = slice(off, off + cnt)
        a = _alpha(sig[s], ts[s, 1], binarize)
        Tpost = np.cumprod(1.0 - a)
        below = np.nonzero(Tpost < T_thresh)[0]
        k = below[0] + 1 if len(below) else cnt
        Tpre = np.concatenate([[1.0], Tpost[:-1]])
        wk = (a * Tpre)[:k]
        w[off:off + k] = wk
        ws[n] = wk.sum(); dep[n] = (wk * ts[off:off + k, 0]).sum(); img[n] = (wk[:, None] * rgb[off:off + k]).sum(0)
        used[n] = k
    return w, ws, dep, img, used


def composite_backward(grad_w, grad_ws, grad_d, grad_img, sigmas, rgbs, ts, rays, T_thresh, binarize=False):
    """the reference's formula: grad_rgb_i = grad_image * w_i; grad_sigma_i = dt_i * (sum_c g_c (T_i rgb_ic - (final_c - acc_ci))
    + (g_ws + g_w_i)(T_i - (ws_final - ws_i)) + g_d (T_i t_i - (d_final - d_i))), T_i after sample i, acc_i including i"""
    sig, rgb, ts = (np.asarray(a, dtype=np.float64) for a in (sigmas, rgbs, ts))
    gw, gws, gd, gi = (np.asarray(a, dtype=np.float64) for a in (grad_w, grad_ws, grad_d, grad_img))
    M, N = len(sig), len(rays)
    gs = np.zeros(M); gr = np.zeros_like(rgb)
    for n in range(N):
        off, cnt = int(rays[n, 0]), int(rays[n, 1])
        if cnt == 0 or off + cnt > M:
            continue
        s = slice(off, off + cnt)
        a = _alpha(sig[s], ts[s, 1], binarize)
        Tpost = np.cumprod(1.0 - a)
        below = np.nonzero(Tpost < T_thresh)[0]
        k = below[0] + 1 if len(below) else cnt
        Tpre = np.concatenate([[1.0], Tpost[:-1]])
        w = (a * Tpre)[:k]; T = Tpost[:k]
        r = rgb[off:off + k]; t0 = ts[off:off + k, 0]; dt = ts[off:off + k, 1]
        acc = np.cumsum(w[:, None] * r, 0); wsa = np.cumsum(w); da = np.cumsum(w * t0)
        gr[off:off + k] = gi[n][None, :] * w[:, None]
        gs[off:off + k] = dt * ((gi[n][None, :] * (T[:, None] * r - (acc[-1][None, :] - acc))).sum(1)
                                + (gws[n] + gw[off:off + k]) * (T - (wsa[-1] - wsa)) + gd[n] * (T * t0 - (da[-1] - da)))
    return gs, gr


def composite_inference(sigmas, rgbs, ts, rays, T_thresh, binarize=False):
    """what the inference loop (march_rays / composite_rays, :874-924) composites from the same samples: T = 1 - weights_sum BEFORE
    the sample, and the ray stops after the first sample whose T (before it) is below T_thresh -- one sample later than the training
    composite, which tests T after the sample.  -> weights_sum, depth, image"""
    sig, rgb, ts = (np.asarray(a, dtype=np.float64) for a in (sigmas, rgbs, ts))
    N, C = len(rays), rgb.shape[1]
    ws = np.zeros(N); dep = np.zeros(N); img = np.zeros((N, C))
    for n in range(N):
        off, cnt = int(rays[n, 0]), int(rays[n, 1])
        acc = 0.0
        for i in range(off, off + cnt):
            a = _alpha(sig[i], ts[i, 1], binarize)
            T = 1.0 - acc
            w = a * T
            acc += w
            dep[n] += w * ts[i, 0]
            img[n] += w * rgb[i]
            if T < T_thresh:
                break
        ws[n] = acc
    return ws, dep, img


# ----------------------------------------------------------------------------------------------------------------------------------
# scenes
# ----------------------------------------------------------------------------------------------------------------------------------
def cell_centres(C, H, bound):
    """[C, H^3, 3] world positions of the cells in the bitfield's (level, morton) order"""
    xyz = morton3d_invert(np.arange(H ** 3)).astype(np.float64)
    out = []
    for c in range(C):
        mb = min(2.0 ** c, bound)
        out.append(((xyz + 0.5) / H * 2 - 1) * mb)
    return np.stack(out)


def body_density(p):
    """an ellipsoid blob (a standing body) plus thin shells: voxel skipping and re-entry both happen"""
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    blob = (x / 0.28) ** 2 + (y / 0.85) ** 2 + (z / 0.2) ** 2 < 1.0
    head = x ** 2 + (y - 0.95) ** 2 + z ** 2 < 0.15 ** 2
    r = np.sqrt(x ** 2 + y ** 2 + z ** 2)
    shell1 = (np.abs(r - 1.2) < 0.04) & (y > 0.3)
    shell2 = (np.abs(r - 0.6) < 0.02) & (x > 0)
    return (blob | head | shell1 | shell2).astype(np.float32) * 10.0


def make_grid(C, H, bound, kind="body"):
    """density grid [C, H^3] (bitfield order) and its bitfield (threshold 5)"""
    if kind == "dense":
        g = np.full((C, H ** 3), 10.0, np.float32)
    elif kind == "empty":
        g = np.zeros((C, H ** 3), np.float32)
    else:
        g = body_density(cell_centres(C, H, bound)).astype(np.float32)
    return g, packbits(g, 5.0)


def make_cameras(n_views, W, Hh, seed=0):
    """rays as stage I draws them: radius 1-2, fov 40-70 degrees, looking at the origin (y up) -> rays_o, rays_d [n_views*Hh*W, 3]"""
    rng = np.random.RandomState(seed)
    os_, ds = [], []
    for _ in range(n_views):
        rad = rng.uniform(1.0, 2.0)
        th, ph = rng.uniform(60, 100) * np.pi / 180, rng.uniform(0, 2 * np.pi)
        eye = rad * np.array([np.sin(th) * np.sin(ph), np.cos(th), np.sin(th) * np.cos(ph)])
        fwd = -eye / np.linalg.norm(eye)
        right = np.cross(fwd, [0, 1, 0]); right /= np.linalg.norm(right)
        up = np.cross(right, fwd)
        fov = rng.uniform(40, 70) * np.pi / 180
        f = 0.5 * Hh / np.tan(fov / 2)
        j, i = np.meshgrid(np.arange(Hh) + 0.5, np.arange(W) + 0.5, indexing="ij")
        d = ((i - W / 2) / f)[..., None] * right - ((j - Hh / 2) / f)[..., None] * up + fwd
        d = d / np.linalg.norm(d, axis=-1, keepdims=True)
        ds.append(d.reshape(-1, 3)); os_.append(np.broadcast_to(eye, d.shape).reshape(-1, 3))
    return np.concatenate(os_).astype(np.float32), np.concatenate(ds).astype(np.float32)


def field(xyzs, channels):
    """a deterministic radiance field for the inference-vs-training comparison: (sigma [M], colour [M, channels]) from positions"""
    x = np.asarray(xyzs, dtype=np.float64)
    sig = 20.0 * np.exp(-((x ** 2).sum(-1)) * 2.0) + 0.5
    col = np.stack([0.5 + 0.5 * np.sin(3 * x[:, k % 3] + k) for k in range(channels)], -1)
    return sig.astype(np.float32), col.astype(np.float32)
