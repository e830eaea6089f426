"""Host reference of the several-parts recovery (sqr.fit.recover_parts, sqr_pts_seed / sqr_pts_assign /
sqr_pts_recover_parts) on the CPU in a given dtype.  The rules, as include/sqr.h states them:

  counting  slot i of a cloud counts iff i < count (clamped into [0, P]) and its three coordinates are finite
  radial    d = |p - t| |1 - f^(-1/2)|, f = F^e1 the quantity of _lm_ref.residuals (f = r / sqrt(a0 a1 a2) + 1, its
            clamps and its zero fix); a d that is not finite is +inf
  assign    label = argmin_m d, the lowest m on a tie, 0 when every d is +inf, -1 (and dist 0) for a slot that does
            not count
  seeding   squared distances in float32, (dx dx + dy dy) + dz dz with every product and sum rounded (no FMA).
            Seed 0 = the counting slot farthest from the first counting slot; seed k = the counting slot whose
            distance to the nearest earlier seed is largest.  A candidate replaces the running best only if it is
            strictly farther, the running best starting at (the first counting slot | the seed before, distance 0):
            ties go to the lowest slot and a cloud that has run out of distinct points repeats its last seed.  The
            centres start as the seeds' points.  Then one nearest-centre assignment (strictly nearer replaces: the
            lowest m on a tie) and `lloyd` times (every centre := the mean of its part's counting points, summed in
            float64 and rounded to float32, an empty part keeps its centre; assign again): the labels returned
            belong to the centres returned.  A cloud without a counting slot: seeds -1, centres 0.
  rounds    round 0: per part _recover_ref.starts_of, three _lm_ref.lm_loop of iters0 iterations, the lowest energy
            wins; rounds 1 .. T-1: lm_loop of `iters` iterations from the current parameters.  After every round
            assign.  An empty part: the default start with energy 0 in round 0, lm_loop on no point afterwards.
"""
import numpy as np
import torch

import classes
from quaternion import conjugate, mat_from_quaternion

import _lm_ref
import _recover_ref as rr


def counting(points, count=None):
    """points [P,3] -> [P] bool."""
    p = np.asarray(points)
    on = np.isfinite(p).all(axis=1)
    if count is not None:
        on &= np.arange(len(p)) < min(max(int(count), 0), len(p))
    return on


def radial_distance(pts, p):
    """pts [3,N], p [12] raw parameters (tensors of one dtype) -> d [N] in that dtype, +inf where not finite."""
    p = classes.LeastSquares.preprocess_sq(p)
    a, e, t, q = p[0:3], p[3:5], p[5:8], p[8:12]
    rot = mat_from_quaternion(conjugate(q))[0]
    v = (rot @ pts - (rot @ t)[:, None]) / a[:, None]
    sq = v * v
    sq = torch.where(sq == 0, sq + 1e-4, sq)
    A, B, C = sq[0] ** (1 / e[1]), sq[1] ** (1 / e[1]), sq[2] ** (1 / e[0])
    f = ((A + B) ** (e[1] / e[0]) + C) ** e[0]
    d = pts - t[:, None]
    norm = torch.sqrt((d * d).sum(0))
    out = norm * torch.abs(1 - f ** -0.5)
    return torch.where(torch.isfinite(out), out, torch.full_like(out, float("inf")))


def assign(points, params, count=None, dt=torch.float64):
    """One cloud: points [P,3] f32, params [M,12] -> (label [P] i32, dist [P] float64 copies of the dt values, all
    distances [M,P])."""
    pts = np.asarray(points, np.float32)
    on = counting(pts, count)
    P, M = len(pts), len(params)
    D = np.full((M, P), np.inf)
    x = torch.tensor(np.ascontiguousarray(pts[on].T)).to(dt)
    for m in range(M):
        if on.any():
            D[m, on] = radial_distance(x, torch.as_tensor(np.asarray(params[m])).to(dt)).double().numpy()
    label = np.full(P, -1, np.int32)
    dist = np.zeros(P)
    best = np.argmin(D[:, on], axis=0) if on.any() else np.zeros(0, np.int64)  # the first minimum: the lowest m
    label[on] = best
    dist[on] = D[:, on][best, np.arange(int(on.sum()))]
    return label, dist, D


def part_sums(label, dist, M):
    """(part_count [M] i32, part_dist [M] f64) of one cloud's labels."""
    cnt = np.array([(label == m).sum() for m in range(M)], np.int32)
    return cnt, np.array([dist[label == m].sum() for m in range(M)], np.float64)


def sqdist32(p, c):
    """(dx dx + dy dy) + dz dz in float32, every operation rounded: p [N,3] f32, c [3] f32 -> [N] f32."""
    d = np.asarray(p, np.float32) - np.asarray(c, np.float32)[None, :]
    with np.errstate(over="ignore", invalid="ignore"):
        return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32)


def nearest_centre(pts, on, centres):
    """label [P] i32 (-1 where the slot does not count) and the two smallest squared distances [2,P] f32."""
    D = np.stack([sqdist32(pts, c) for c in centres])
    D = np.where(np.isnan(D), np.float32(np.inf), D)
    label = np.where(on, np.argmin(D, axis=0), -1).astype(np.int32)
    return label, np.sort(D, axis=0)[:2] if len(centres) > 1 else np.concatenate([D, np.full_like(D, np.inf)])


def seed(points, M, count=None, lloyd=10):
    """One cloud -> dict: seeds [M] i32, centres [M,3] f32, label [P] i32, margin (the smallest gap between a counting
    slot's nearest and second-nearest centre over every assignment made, float32 squared distance)."""
    pts = np.asarray(points, np.float32)
    on = counting(pts, count)
    P = len(pts)
    if not on.any():
        return dict(seeds=np.full(M, -1, np.int32), centres=np.zeros((M, 3), np.float32),
                    label=np.full(P, -1, np.int32), margin=np.inf)
    slots = np.flatnonzero(on)

    def farthest(d, start):
        best, bd = start, np.float32(0)
        for i in slots:
            if d[i] > bd:
                best, bd = i, d[i]
        return int(best)

    seeds = [farthest(sqdist32(pts, pts[slots[0]]), slots[0])]
    mind = sqdist32(pts, pts[seeds[0]])
    for _ in range(1, M):
        seeds.append(farthest(mind, seeds[-1]))
        mind = np.minimum(mind, sqdist32(pts, pts[seeds[-1]]))
    centres = pts[seeds].copy()
    label, two = nearest_centre(pts, on, centres)
    margin = float((two[1][on] - two[0][on]).min())
    for _ in range(lloyd):
        for m in range(M):
            sel = label == m
            if sel.any():
                centres[m] = (pts[sel].astype(np.float64).sum(0) / float(sel.sum())).astype(np.float32)
        label, two = nearest_centre(pts, on, centres)
        margin = min(margin, float((two[1][on] - two[0][on]).min()))
    return dict(seeds=np.array(seeds, np.int32), centres=centres, label=label, margin=margin)


def fit_part(pts_m, start, iters, dt):
    """lm_loop on one part's points [N,3] f32 -> (params [12] float64 copy, energy)."""
    x = torch.tensor(np.ascontiguousarray(np.asarray(pts_m, np.float32).T)).to(dt)
    p, _, after, _ = _lm_ref.lm_loop(x, start, iters=iters, dt=dt)
    return p.double().numpy(), after


def recover_part(pts_m, iters0, e0, dt):
    """Round 0 of one part: the three starts, three loops, the selection -> (params [12], energy)."""
    if len(pts_m) == 0:
        return rr.default_start(e0).astype(np.float64), 0.0
    ndt = np.float64 if dt == torch.float64 else np.float32
    starts, _ = rr.starts_of(np.asarray(pts_m, np.float32).T, e0, ndt)
    fits = [fit_part(pts_m, starts[k], iters0, dt) for k in range(3)]
    k = int(rr.select(np.array([[f[1]] for f in fits]))[0])
    return fits[k]


def rounds(points, label0, M, count=None, T=3, iters0=30, iters=10, e0=1.0, dt=torch.float64):
    """One cloud from the labels label0 -> dict: params [T,M,12], energy [T,M], label [T,P] i32, changed [T] i32,
    dist [P], and margin: the smallest gap between a counting slot's best and second-best radial distance in the
    last assignment."""
    pts = np.asarray(points, np.float32)
    label = np.asarray(label0, np.int32)
    out = dict(params=np.zeros((T, M, 12)), energy=np.zeros((T, M)), label=np.zeros((T, len(pts)), np.int32),
               changed=np.zeros(T, np.int32))
    cur = None
    for t in range(T):
        fits = []
        for m in range(M):
            part = pts[label == m]
            fits.append(recover_part(part, iters0, e0, dt) if t == 0 else fit_part(part, cur[m], iters, dt))
        cur = np.stack([f[0] for f in fits])
        new, dist, D = assign(pts, cur, count, dt)
        out["params"][t], out["energy"][t], out["label"][t] = cur, [f[1] for f in fits], new
        out["changed"][t] = int(((new != label) & (new >= 0)).sum())
        label = new
    on = label >= 0
    two = np.sort(D[:, on], axis=0)
    out["dist"] = dist
    out["margin"] = float((two[1] - two[0]).min()) if M > 1 and on.any() else np.inf
    return out
