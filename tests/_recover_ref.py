"""Host reference of the classical recovery (sqr.fit.recover, sqr_lsq_starts / sqr_lsq_select): the start
rules in numpy in a given dtype on the points of _lm_ref.points_of, the loop _lm_ref.lm_loop, and the
selection rule.  The rules, as include/sqr.h states them:

  moments   n, sum p, sum p p^T over the points; centroid c = sum p / n; covariance C = sum p p^T / n - c c^T
  frame     cyclic Jacobi on C, SWEEPS sweeps over the pairs (0,1), (0,2), (1,2); eigenvalues ascending (three
            exchanges (0,1), (1,2), (0,1), columns along); the component of the largest magnitude (the first on
            a tie) is made negative in column 0 and positive in column 1, column 2 = column 0 x column 1: a
            proper rotation V
  extents   min and max of V^T p over the points
  start k   M_k = columns (k, k+1, k+2 mod 3) of V; a = half the extents in that order, clamped into [0.05, 1];
            e = (e0, e0); t = M_k (midpoint of the extents), clamped into [0, 1]; q = the xyzw quaternion of M_k
            by the largest of (trace, m00, m11, m22), the first on a tie; stored as float32
  no point  a = 0.05, e = e0, t = 0.5, q = (0, 0, 0, 1), count 0, V = I
  select    the lowest energy wins, the lowest index on a tie, NaN never wins, all NaN: index 0
"""
import numpy as np
import torch

import _lm_ref

SWEEPS = 8
TORCH_OF = {np.float64: torch.float64, np.float32: torch.float32}


def _rotate(A, V, p, q, r, dt):
    """One Jacobi rotation of the symmetric 3 x 3 A in the (p, q) plane; r is the third index."""
    apq = A[p, q]
    if apq == 0:
        return
    one = dt(1)
    with np.errstate(over="ignore"):
        theta = (A[q, q] - A[p, p]) / (dt(2) * apq)
        t = (one if theta >= 0 else -one) / (abs(theta) + np.sqrt(theta * theta + one))
    c = one / np.sqrt(t * t + one)
    s = t * c
    A[p, p] -= t * apq
    A[q, q] += t * apq
    A[p, q] = A[q, p] = dt(0)
    rp, rq = A[r, p], A[r, q]
    A[r, p] = A[p, r] = c * rp - s * rq
    A[r, q] = A[q, r] = s * rp + c * rq
    vp, vq = V[:, p].copy(), V[:, q].copy()
    V[:, p] = c * vp - s * vq
    V[:, q] = s * vp + c * vq


def _sign(col, sign):
    a = np.abs(col)
    lead = col[0] if (a[0] >= a[1] and a[0] >= a[2]) else (col[1] if a[1] >= a[2] else col[2])
    return -col if lead * sign < 0 else col


def frame_of(C, dt=np.float64):
    """(eigenvalues ascending [3], V [3,3]) of the symmetric 3 x 3 C by the rules above, in dtype dt."""
    A = np.array(C, dtype=dt)
    V = np.eye(3, dtype=dt)
    for _ in range(SWEEPS):
        _rotate(A, V, 0, 1, 2, dt)
        _rotate(A, V, 0, 2, 1, dt)
        _rotate(A, V, 1, 2, 0, dt)
    lam = np.array([A[0, 0], A[1, 1], A[2, 2]], dtype=dt)
    for i, j in ((0, 1), (1, 2), (0, 1)):
        if lam[i] > lam[j]:
            lam[[i, j]] = lam[[j, i]]
            V[:, [i, j]] = V[:, [j, i]]
    V[:, 0] = _sign(V[:, 0], -1)
    V[:, 1] = _sign(V[:, 1], 1)
    V[:, 2] = np.cross(V[:, 0], V[:, 1])
    return lam, V


def quat_of(M):
    """xyzw quaternion of the rotation matrix M, from the largest of (trace, m00, m11, m22)."""
    dt = M.dtype.type
    tr = M[0, 0] + M[1, 1] + M[2, 2]
    one, two, quarter = dt(1), dt(2), dt(0.25)
    if tr >= M[0, 0] and tr >= M[1, 1] and tr >= M[2, 2]:
        s = two * np.sqrt(one + tr)
        q = [(M[2, 1] - M[1, 2]) / s, (M[0, 2] - M[2, 0]) / s, (M[1, 0] - M[0, 1]) / s, quarter * s]
    elif M[0, 0] >= M[1, 1] and M[0, 0] >= M[2, 2]:
        s = two * np.sqrt(one + M[0, 0] - M[1, 1] - M[2, 2])
        q = [quarter * s, (M[0, 1] + M[1, 0]) / s, (M[0, 2] + M[2, 0]) / s, (M[2, 1] - M[1, 2]) / s]
    elif M[1, 1] >= M[2, 2]:
        s = two * np.sqrt(one + M[1, 1] - M[0, 0] - M[2, 2])
        q = [(M[0, 1] + M[1, 0]) / s, quarter * s, (M[1, 2] + M[2, 1]) / s, (M[0, 2] - M[2, 0]) / s]
    else:
        s = two * np.sqrt(one + M[2, 2] - M[0, 0] - M[1, 1])
        q = [(M[0, 2] + M[2, 0]) / s, (M[1, 2] + M[2, 1]) / s, quarter * s, (M[1, 0] - M[0, 1]) / s]
    return np.array(q, dtype=dt)


def default_start(e0):
    return np.array([0.05, 0.05, 0.05, e0, e0, 0.5, 0.5, 0.5, 0, 0, 0, 1], np.float32)


def starts_from_frame(P, V, e0):
    """The three float32 starts [3,12] from the points P [3,N] and the frame V, in V's dtype."""
    dt = V.dtype.type
    proj = V.T @ P.astype(V.dtype)
    lo, hi = proj.min(1), proj.max(1)
    half, mid = dt(0.5) * (hi - lo), dt(0.5) * (hi + lo)
    out = np.empty((3, 12), np.float32)
    for k in range(3):
        ax = [(k + j) % 3 for j in range(3)]
        M = V[:, ax]
        a = np.clip(half[ax].astype(np.float32), np.float32(0.05), np.float32(1))
        t = np.clip((M @ mid[ax]).astype(np.float32), np.float32(0), np.float32(1))
        s = np.concatenate([a, np.float32([e0, e0]), t, quat_of(M).astype(np.float32)])
        out[k] = s if np.isfinite(s).all() else default_start(e0)
    return out


def starts_of(pts, e0=1.0, dt=np.float64):
    """pts [3,N] (array or tensor) -> (starts [3,12] float32, info dict: count, centroid, eigenvalues, frame,
    covariance), everything computed in dtype dt."""
    P = np.asarray(pts, dtype=dt).reshape(3, -1)
    n = P.shape[1]
    if n == 0:
        z = np.zeros(3, dt)
        return np.tile(default_start(e0), (3, 1)), dict(count=0, centroid=z, eigenvalues=z.copy(),
                                                        frame=np.eye(3, dtype=dt), covariance=np.zeros((3, 3), dt))
    c = P.sum(1) / dt(n)
    C = (P @ P.T) / dt(n) - np.outer(c, c)
    lam, V = frame_of(C, dt)
    return starts_from_frame(P, V, e0), dict(count=n, centroid=c, eigenvalues=lam, frame=V, covariance=C)


def select(energy):
    """energy [K,B] -> index [B] int32 by the selection rule."""
    e = np.asarray(energy, np.float64)
    idx = np.zeros(e.shape[1], np.int32)
    for b in range(e.shape[1]):
        best, be = 0, e[0, b]
        for k in range(1, e.shape[0]):
            if e[k, b] < be or (np.isnan(be) and not np.isnan(e[k, b])):
                best, be = k, e[k, b]
        idx[b] = best
    return idx


def recover_one(true, R, iters=30, e0=1.0, dt=np.float64):
    """One image [1,H,W] or [H,W] through the host pipeline in dtype dt -> dict: starts [3,12] f32, before [3],
    after [3], params [3,12] (float64 copies of the dt results), winner."""
    tdt = TORCH_OF[dt]
    pts = _lm_ref.points_of(np.asarray(true, np.float32).reshape((1, 1) + np.asarray(true).shape[-2:]), R, tdt)[0]
    starts, _ = starts_of(pts.numpy(), e0, dt)
    before, after, params = np.zeros(3), np.zeros(3), np.zeros((3, 12))
    for k in range(3):
        p, b, a, _ = _lm_ref.lm_loop(pts, starts[k], iters=iters, dt=tdt)
        before[k], after[k], params[k] = b, a, p.double().numpy()
    return dict(starts=starts, before=before, after=after, params=params, winner=int(select(after[:, None])[0]))
