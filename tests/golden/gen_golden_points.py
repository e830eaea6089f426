"""Generate tests/golden/points.npz: eight whole-surface point clouds and the host pipeline's recovery of them
(tests/_recover_ref.py starts, three tests/_lm_ref.py Levenberg-Marquardt loops of 30 iterations, the lowest
energy wins), in float64 and in float32.  Everything comes from this project's own code; about two minutes on a
CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_points.py

The labels are classes.sample_sq_params(np.random.default_rng(0), 8).  Each label's surface is sampled by the
textbook angle parametrisation on a 16 x 32 grid of (eta, omega), in the local frame

    u = (a0 c(eta, e0) c(omega, e1),  a1 c(eta, e0) s(omega, e1),  a2 s(eta, e0)),
    c(w, e) = sign(cos w) |cos w|^e,  s(w, e) = sign(sin w) |sin w|^e,

eta = -pi/2 + (i + 1/2) pi / 16 and omega = -pi + (j + 1/2) 2 pi / 32 (cell midpoints: no coordinate is exactly
zero, so the energy's zero fix never fires), and moved to the world by the inverse of the map the LeastSquares
energy applies: u = rot (p - t), rot = mat_from_quaternion(conjugate(q)).  The points are computed in float64
and stored as float32, the dtype of a point list.

Per precision tag (64, 32) and cloud: the three float32 starts, their energies before and after, the final
parameters, the winner and the winner's IoU against the label (classes.IoUAccuracy, grid 32, on the CPU).  A
label whose float32 pipeline ends below IoU 0.98 is replaced by the same row of the next seed's draw (the seeds
used are stored), so that the reference alone satisfies what tests/test_points_gpu.py asks of the device.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "sq-recovery_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

N_CLOUDS, N_ETA, N_OMEGA, ITERS, E0, IOU_GRID, IOU_MIN = 8, 16, 32, 30, 1.0, 32, 0.98
TAGS = (("64", np.float64), ("32", np.float32))


def sample_surface(label, n_eta=N_ETA, n_omega=N_OMEGA):
    """label [12] -> [n_eta * n_omega, 3] float32 points of its surface, eta-major."""
    from quaternion import conjugate, mat_from_quaternion
    p = np.asarray(label, np.float64)
    a, e, t = p[0:3], p[3:5], p[5:8]
    rot = mat_from_quaternion(conjugate(torch.tensor(p[8:12], dtype=torch.float64)))[0].numpy()
    eta = -np.pi / 2 + (np.arange(n_eta) + 0.5) * np.pi / n_eta
    omega = -np.pi + (np.arange(n_omega) + 0.5) * 2 * np.pi / n_omega
    eta, omega = np.meshgrid(eta, omega, indexing="ij")
    c = lambda w, ex: np.sign(np.cos(w)) * np.abs(np.cos(w)) ** ex  # noqa: E731
    s = lambda w, ex: np.sign(np.sin(w)) * np.abs(np.sin(w)) ** ex  # noqa: E731
    u = np.stack([a[0] * c(eta, e[0]) * c(omega, e[1]), a[1] * c(eta, e[0]) * s(omega, e[1]),
                  a[2] * s(eta, e[0])]).reshape(3, -1)
    world = np.linalg.solve(rot, u) + t[:, None]
    return np.ascontiguousarray(world.T).astype(np.float32)


def recover_cloud(cloud, iters=ITERS, e0=E0, dt=np.float64):
    """cloud [N,3] f32 through the host pipeline in dtype dt -> dict: starts [3,12] f32, before [3], after [3],
    params [3,12] (float64 copies of the dt results), winner."""
    import _lm_ref
    import _recover_ref as rr
    tdt = rr.TORCH_OF[dt]
    pts = torch.tensor(np.asarray(cloud, np.float32).T.copy()).to(tdt)
    starts, _ = rr.starts_of(pts.numpy(), e0, dt)
    before, after, params = np.zeros(3), np.zeros(3), np.zeros((3, 12))
    for k in range(3):
        p, b, a, _ = _lm_ref.lm_loop(pts, starts[k], iters=iters, dt=tdt)
        before[k], after[k], params[k] = b, a, p.double().numpy()
    return dict(starts=starts, before=before, after=after, params=params,
                winner=np.int32(rr.select(after[:, None])[0]))


def iou_of(label, params):
    import classes
    acc = classes.IoUAccuracy(IOU_GRID, "cpu", reduce=False)
    return float(acc(torch.tensor(np.asarray(label)[None], dtype=torch.float64),
                     torch.tensor(np.asarray(params)[None], dtype=torch.float64))[0])


def rows_of(label):
    cloud = sample_surface(label)
    out = {"cloud": cloud}
    for tag, dt in TAGS:
        r = recover_cloud(cloud, dt=dt)
        r["iou"] = np.float64(iou_of(label, r["params"][r["winner"]]))
        for k, v in r.items():
            out["%s_%s" % (k, tag)] = v
    return out


def main():
    import classes
    torch.set_num_threads(8)
    labels = classes.sample_sq_params(np.random.default_rng(0), N_CLOUDS)
    seeds = np.zeros(N_CLOUDS, np.int32)
    rows = []
    for i in range(N_CLOUDS):
        while True:
            r = rows_of(labels[i])
            print("cloud %d seed %d: f64 after %s winner %d IoU %.4f | f32 after %s winner %d IoU %.4f" % (
                i, seeds[i], " ".join("%.3e" % v for v in r["after_64"]), r["winner_64"], r["iou_64"],
                " ".join("%.3e" % v for v in r["after_32"]), r["winner_32"], r["iou_32"]), flush=True)
            if r["iou_32"] >= IOU_MIN:
                break
            seeds[i] += 1
            labels[i] = classes.sample_sq_params(np.random.default_rng(int(seeds[i])), N_CLOUDS)[i]
        rows.append(r)
    out = {"labels": labels, "seeds": seeds, "iters": np.int32(ITERS), "e0": np.float64(E0),
           "iou_grid": np.int32(IOU_GRID)}
    for k in rows[0]:
        out["clouds" if k == "cloud" else k] = np.stack([r[k] for r in rows])
    np.savez_compressed(os.path.join(HERE, "points.npz"), **out)
    print("wrote points.npz")


if __name__ == "__main__":
    main()
