"""Host reference of the multi-start recovery's new parts (sqr_lsq_free_space, sqr_lsq_starts6, the scored
selection of sqr_lsq_recover_multi), in numpy / torch on the CPU in a given dtype.  The rules, as include/sqr.h
states them:

  free space  resized pixel (r, c) of image s mod B is the ray x = c / R, y = 1 - r / R (float32, as the points
              of _lm_ref.points_of); segment [zlo, ZHI]: zlo = z + margin for a pixel z > 0, 0 for a pixel <= 0;
              a NaN pixel and an empty segment add nothing;
              E_fs = a0 a1 a2 sum_pixels min(min_z F(x, y, z) - 1, 0)^2, F restated from _lm_ref.residuals.
              F^(1/e1) is convex along the ray, so F is unimodal there: a golden-section search with STEPS
              steps on F itself (no derivative, no slab shortcut: nothing of the kernel's procedure is shared)
  six starts  starts 0..2 of _recover_ref.starts_from_frame; for 3..5 the extent along column j of V, j the largest
              |V[2][j]| (the first on a tie), grows by depth (max_j - min_j) on the side away from the viewer:
              V[2][j] > 0: min_j -= that, else max_j += that; everything else as for 0..2
  selection   score = energy + w E_fs (w = 0: the energy), _recover_ref.select on the score
"""
import numpy as np
import torch
import torch.nn.functional as F

import classes
import _lm_ref
import _recover_ref as rr
from quaternion import conjugate, mat_from_quaternion

ZHI = 4.0
STEPS = 60
MARGIN = 1.0 / 255.0
INVPHI = (np.sqrt(5.0) - 1.0) / 2.0


def inside_outside(pts, p):
    """F of the points pts [3,N] under the raw parameters p [12]: the lines of _lm_ref.residuals up to f."""
    p = classes.LeastSquares.preprocess_sq(p)
    a, e, t, q = p[0:3], p[3:5], p[5:8], p[8:12]
    rot = mat_from_quaternion(conjugate(q))[0]
    v = (rot @ pts - (rot @ t)[:, None]) / a[:, None]
    sq = v * v
    sq = torch.where(sq == 0, sq + 1e-4, sq)
    A, B, C = sq[0] ** (1 / e[1]), sq[1] ** (1 / e[1]), sq[2] ** (1 / e[0])
    return ((A + B) ** (e[1] / e[0]) + C) ** e[0]


def resized(true, R):
    """[B,R,R] float32: the nearest resize of LeastSquares.batch_points."""
    t = torch.as_tensor(np.asarray(true, np.float32))
    if t.dim() == 3:
        t = t[:, None]
    return F.interpolate(t, size=(R, R), mode="nearest")[:, 0]


def rays_of(img, R, margin, dt):
    """One resized image [R,R] f32 -> (x, y, zlo, zhi) in dt of the rays that count."""
    rows, cols = torch.meshgrid(torch.arange(R), torch.arange(R), indexing="ij")
    x = (cols.float() / R).reshape(-1)
    y = (1 - rows.float() / R).reshape(-1)
    z = img.reshape(-1).to(dt)
    zlo = torch.where(z > 0, z + torch.tensor(margin, dtype=torch.float32).to(dt), torch.zeros_like(z))
    zhi = torch.full_like(zlo, ZHI)
    keep = ~torch.isnan(z) & (zlo <= zhi)
    return x[keep].to(dt), y[keep].to(dt), zlo[keep], zhi[keep]


def ray_minimum(x, y, zlo, zhi, p, steps=STEPS):
    """(min over z in [zlo, zhi] of F(x, y, z), its z) per ray, by golden section in p's dtype."""
    f = lambda z: inside_outside(torch.stack([x, y, z]), p)  # noqa: E731
    a, b = zlo.clone(), zhi.clone()
    c, d = b - INVPHI * (b - a), a + INVPHI * (b - a)
    fc, fd = f(c), f(d)
    for _ in range(steps):
        left = fc < fd
        b = torch.where(left, d, b)
        a = torch.where(left, a, c)
        c, d = b - INVPHI * (b - a), a + INVPHI * (b - a)
        fc, fd = f(c), f(d)
    # the ends of the segment count too (a minimiser clipped to the segment)
    zs = torch.stack([zlo, zhi, c, d])
    fs = torch.stack([f(zlo), f(zhi), fc, fd])
    best = fs.argmin(0)
    return fs.gather(0, best[None])[0], zs.gather(0, best[None])[0]


def free_space_one(img, p, R, margin=MARGIN, dt=torch.float64):
    """One resized image [R,R] and raw parameters [12] -> E_fs as a float, computed in dt."""
    p = torch.as_tensor(np.asarray(p)).to(dt)
    x, y, zlo, zhi = rays_of(img, R, margin, dt)
    if x.numel() == 0:
        return 0.0
    fmin, _ = ray_minimum(x, y, zlo, zhi, p)
    a = classes.LeastSquares.preprocess_sq(p)[0:3]
    return float((a[0] * a[1] * a[2] * (torch.clamp(fmin - 1, max=0) ** 2).sum()).item())


def free_space(true, params, R, margin=MARGIN, dt=torch.float64):
    """true [B,1,H,W] or [B,H,W], params [S,12], S a multiple of B -> E_fs [S] float64; sample s on image s mod B."""
    tr = resized(true, R)
    params = np.asarray(params)
    B = tr.shape[0]
    assert params.shape[0] % B == 0
    return np.array([free_space_one(tr[s % B], params[s], R, margin, dt) for s in range(params.shape[0])])


def depth_axis(V):
    z = np.abs(V[2])
    return 0 if (z[0] >= z[1] and z[0] >= z[2]) else (1 if z[1] >= z[2] else 2)


def starts6_from_frame(P, V, e0, depth=1.0):
    """The six float32 starts [6,12] from the points P [3,N] and the frame V, in V's dtype."""
    dt = V.dtype.type
    proj = V.T @ P.astype(V.dtype)
    out = np.empty((6, 12), np.float32)
    for s, stretch in enumerate((dt(0), dt(depth))):
        lo, hi = proj.min(1), proj.max(1)
        j = depth_axis(V)
        grow = stretch * (hi[j] - lo[j])
        if V[2, j] > 0:
            lo[j] -= grow
        else:
            hi[j] += grow
        half, mid = dt(0.5) * (hi - lo), dt(0.5) * (hi + lo)
        for k in range(3):
            ax = [(k + i) % 3 for i in range(3)]
            M = V[:, ax]
            a = np.clip(half[ax].astype(np.float32), np.float32(0.05), np.float32(1))
            t = np.clip((M @ mid[ax]).astype(np.float32), np.float32(0), np.float32(1))
            row = np.concatenate([a, np.float32([e0, e0]), t, rr.quat_of(M).astype(np.float32)])
            out[3 * s + k] = row if np.isfinite(row).all() else rr.default_start(e0)
    return out


def starts6_of(pts, e0=1.0, depth=1.0, dt=np.float64):
    """pts [3,N] -> (starts [6,12] float32, info of _recover_ref.starts_of)."""
    P = np.asarray(pts, dtype=dt).reshape(3, -1)
    s3, info = rr.starts_of(P, e0, dt)
    if P.shape[1] == 0:
        return np.concatenate([s3, s3]), info
    s6 = starts6_from_frame(P, info["frame"], e0, depth)
    assert np.array_equal(s6[:3], s3)
    return s6, info


def score_of(energy, fs, w):
    energy = np.asarray(energy, np.float64)
    return energy.copy() if w == 0 else energy + w * np.asarray(fs, np.float64)


def select_scored(energy, fs, w):
    """energy, fs [K,B] -> index [B] by the selection rule on the score."""
    return rr.select(score_of(energy, fs, w))


def recover6_one(true, R, iters=30, e0=1.0, depth=1.0, margin=MARGIN, w_fs=1.0, dt=np.float64, extra=None):
    """One image [1,H,W] or [H,W] through the six-start host pipeline in dtype dt -> dict: starts [K,12] f32,
    before, after, fs, score [K], params [K,12] (float64 copies of the dt results), winner.  extra: [Kx,12] more
    starts behind the six."""
    tdt = rr.TORCH_OF[dt]
    img = np.asarray(true, np.float32).reshape((1, 1) + np.asarray(true).shape[-2:])
    pts = _lm_ref.points_of(img, R, tdt)[0]
    starts, _ = starts6_of(pts.numpy(), e0, depth, dt)
    if extra is not None:
        starts = np.concatenate([starts, np.asarray(extra, np.float32).reshape(-1, 12)])
    K = len(starts)
    tr = resized(img, R)[0]
    before, after, fs, params = np.zeros(K), np.zeros(K), np.zeros(K), np.zeros((K, 12))
    for k in range(K):
        p, b, a, _ = _lm_ref.lm_loop(pts, starts[k], iters=iters, dt=tdt)
        before[k], after[k], params[k] = b, a, p.double().numpy()
        fs[k] = free_space_one(tr, p, R, margin, tdt)
    score = score_of(after, fs, w_fs)
    return dict(starts=starts, before=before, after=after, fs=fs, score=score, params=params,
                winner=int(rr.select(score[:, None])[0]))
