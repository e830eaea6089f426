"""Plain-torch reference of the Levenberg-Marquardt refinement (sqr.fit.refine_lm), on the CPU in a given
dtype: the residual vector restated from classes.LeastSquares.energy_function, its normal equations
through torch.autograd.functional.jacobian, and the accept / solve / project loop with the rules of
sqr_lsq_lm_step."""
import numpy as np
import torch

import classes
from quaternion import conjugate, mat_from_quaternion

LAMBDA_MIN, LAMBDA_MAX = 1e-12, 1e12


def points_of(true, R, dt):
    """Per image the [3,N_i] points of the resized pixels > 0 (LeastSquares.batch_points), in dtype dt."""
    t = torch.as_tensor(true).to(dt)
    if t.dim() == 3:
        t = t[:, None]
    return [p.to(dt) for p in classes.LeastSquares(R, "cpu").batch_points(t)]


def residuals(pts, p):
    """r_k = sqrt(a0 a1 a2) (F(point_k) - 1) of one sample: pts [3,N], p [12] raw parameters.  The lines of
    classes.LeastSquares.energy_function before the square and the sum."""
    p = classes.LeastSquares.preprocess_sq(p)
    a, e, t, q = p[0:3], p[3:5], p[5:8], p[8:12]
    rot = mat_from_quaternion(conjugate(q))[0]
    v = (rot @ pts - (rot @ t)[:, None]) / a[:, None]
    sq = v * v
    sq = torch.where(sq == 0, sq + 1e-4, sq)
    A, B, C = sq[0] ** (1 / e[1]), sq[1] ** (1 / e[1]), sq[2] ** (1 / e[0])
    f = ((A + B) ** (e[1] / e[0]) + C) ** e[0]
    return torch.sqrt(a[0] * a[1] * a[2]) * (f - 1)


def normal_eq_one(pts, p):
    """(H [12,12], g [12], E) of one sample in p's dtype."""
    r = residuals(pts, p)
    if pts.shape[1] == 0:
        z = torch.zeros(12, dtype=p.dtype)
        return torch.zeros(12, 12, dtype=p.dtype), z, torch.zeros((), dtype=p.dtype)
    J = torch.autograd.functional.jacobian(lambda x: residuals(pts, x), p, vectorize=True)  # [N,12]
    return J.T @ J, J.T @ r, (r * r).sum()


def normal_eq(true, params, R, dt):
    """Batched: float64 numpy (H [B,12,12], g [B,12], E [B]) computed in dtype dt."""
    pts = points_of(true, R, dt)
    out = [normal_eq_one(x, torch.as_tensor(p).to(dt)) for x, p in zip(pts, params)]
    return tuple(np.stack([o[i].double().numpy() for o in out]) for i in range(3))


def project(x):
    """a, e, t clamped into their ranges, q divided by its norm (kept when the norm is 0 or not finite)."""
    q = x[8:12]
    n = torch.sqrt((q * q).sum())
    if n > 0 and torch.isfinite(n):
        q = q / n
    return torch.cat([x[0:3].clamp(0.05, 1), x[3:5].clamp(0.1, 1), x[5:8].clamp(0, 1), q])


def solve_step(H, g, lam):
    """(delta, ok): (H + lam diag H) delta = -g on the free set {i: H_ii > 0}, Jacobi-scaled, Cholesky."""
    d = torch.diagonal(H)
    free = d > 0
    delta = torch.zeros_like(g)
    if not free.any():
        return delta, True
    s = 1 / torch.sqrt(d[free])
    A = H[free][:, free] * s[:, None] * s[None, :] + lam * torch.eye(int(free.sum()), dtype=H.dtype)
    L, info = torch.linalg.cholesky_ex(A)
    if int(info) != 0 or not torch.isfinite(L).all():
        return delta, False
    y = torch.cholesky_solve((-s * g[free])[:, None], L)[:, 0]
    if not torch.isfinite(y).all():
        return delta, False
    delta[free] = s * y
    return delta, True


def lm_loop(pts, p0, iters=10, lambda0=1e-3, up=10.0, down=0.1, dt=torch.float64):
    """One sample.  -> (p [12], E_before, E_after, accepted) with the rules of sqr_lsq_lm_refine."""
    clampl = lambda l: min(max(l, LAMBDA_MIN), LAMBDA_MAX)  # noqa: E731
    p = project(torch.as_tensor(p0).to(dt))
    H, g, E = normal_eq_one(pts, p)
    before, lam, accepted = E.item(), lambda0, 0
    trial = None
    for it in range(iters + 1 if iters > 0 else 0):
        if trial is not None:
            if trial[3].item() < E.item():
                p, H, g, E = trial
                accepted += 1
                lam = clampl(lam * down)
            else:
                lam = clampl(lam * up)
        if it == iters:
            break
        delta, ok = solve_step(H, g, lam)
        if not ok:
            lam = clampl(lam * up)
        pt = project(p + delta)
        trial = (pt,) + normal_eq_one(pts, pt)
    return p, before, E.item(), accepted
