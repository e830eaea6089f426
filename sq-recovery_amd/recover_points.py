"""Recover the superquadric of one 3-D point cloud on MI355X, without a network (sqr.fit.recover_points:
Solina & Bajcsy's three starts from the cloud's moments, Levenberg-Marquardt from each, the lowest
LeastSquares energy wins).

    python recover_points.py --points cloud.npy [--normalize] [--iters 30]
    python recover_points.py --points scene.npy --parts 3 [--rounds 3] [--labels-out labels.npy]

--points FILE  a .npy array [N,3], or a text file with "x y z" per line (blanks or commas; # starts a comment).
               Rows that are not finite are ignored.
--normalize    for a cloud in its own units: it is moved into the unit cube first (centre of its bounding box
               to 0.5, its longest side to 0.4; sqr.fit.normalize_points) and the parameters are returned in
               the cloud's units.  Without it the cloud is taken as it is: the fit keeps sizes inside
               [0.05, 1] and the position inside [0, 1], the depth images' unit cube.
--parts M      the cloud holds M bodies: sqr.fit.recover_parts splits it (farthest-point seeds, Lloyd iterations),
               recovers every part and alternates assigning every point to the nearest surface with refitting,
               --rounds times in all (--iters is round 0's, the later rounds run 10).  One parameter block per part
               with its point count and mean radial distance; --labels-out FILE writes every input row's part as an
               int32 .npy (-1 for a row that is not finite).
Prints the twelve parameters (a, e, t, q as they are, no x255), the energy and the winning start.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def read_points(path):
    """[N,3] float32 of a .npy file or a text file of x y z lines."""
    if path.lower().endswith(".npy"):
        pts = np.load(path, allow_pickle=False)
    else:
        with open(path) as f:
            rows = [ln.split("#")[0].replace(",", " ").split() for ln in f]
        pts = np.array([[float(v) for v in r] for r in rows if r], dtype=np.float64)
    pts = np.asarray(pts)
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] < 1:
        raise SystemExit("%s: expected [N,3] points, got %s" % (path, pts.shape))
    return np.ascontiguousarray(pts, dtype=np.float32)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", required=True, metavar="FILE", help=".npy [N,3] or text, x y z per line")
    ap.add_argument("--normalize", action="store_true", help="the cloud is in its own units, not in the unit cube")
    ap.add_argument("--iters", type=int, default=30, metavar="N", help="Levenberg-Marquardt iterations per start")
    ap.add_argument("--parts", type=int, default=None, metavar="M", help="fit M bodies to the cloud")
    ap.add_argument("--rounds", type=int, default=3, metavar="T", help="with --parts: rounds of fit and assign")
    ap.add_argument("--labels-out", default=None, metavar="FILE", help="with --parts: the points' parts as .npy")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)

    from sqr.fit import recover_parts, recover_points
    from sqr.losses import pack_points
    points, count = pack_points([torch.from_numpy(read_points(args.points))], device=args.device)
    if args.parts is not None:
        return main_parts(args, points, count, recover_parts)
    if args.labels_out is not None:
        raise SystemExit("--labels-out needs --parts")
    pred, energy, start = recover_points(points, count, iters=args.iters, normalize=args.normalize)
    a, e, t, q = (o.cpu().numpy() for o in torch.split(pred, (3, 2, 3, 4), dim=1))
    print("Recovered parameters (%d points, %d Levenberg-Marquardt iterations per start, LeastSquares energy %.6g%s, "
          "start %d): " % (points.shape[1], args.iters, energy.item(),
                           " of the normalised cloud" if args.normalize else "", start.item()))
    print("Size a:", a)
    print("Shape e:", e)
    print("Position t:", t)
    print("Rotation q:", q)
    return a, e, t, q


def main_parts(args, points, count, recover_parts):
    pred, labels, energy, info = recover_parts(points, args.parts, count, rounds=args.rounds, iters0=args.iters,
                                               normalize=args.normalize, return_info=True)
    n = info["part_count"][0].cpu().numpy()
    mean = (info["part_dist"][0] / info["part_count"][0].clamp(min=1)).cpu().numpy()
    a, e, t, q = (o.cpu().numpy() for o in torch.split(pred[0], (3, 2, 3, 4), dim=1))
    print("Recovered %d parts (%d points, %d rounds, %d Levenberg-Marquardt iterations per start in round 0; points "
          "that changed part per round: %s)%s:" % (args.parts, points.shape[1], args.rounds, args.iters,
                                                   info["changed"][:, 0].tolist(),
                                                   ", distances of the normalised cloud" if args.normalize else ""))
    for m in range(args.parts):
        print("Part %d (%d points, mean radial distance %.6g, LeastSquares energy %.6g):" % (
            m, n[m], mean[m], energy[0, m].item()))
        print("Size a:", a[m:m + 1])
        print("Shape e:", e[m:m + 1])
        print("Position t:", t[m:m + 1])
        print("Rotation q:", q[m:m + 1])
    if args.labels_out is not None:
        np.save(args.labels_out, labels[0].cpu().numpy())
    return a, e, t, q


if __name__ == "__main__":
    main()
