"""Generate tests/golden/recover.npz: the classical recovery's host pipeline (tests/_recover_ref.py) on the ten
example images (example_images.npz) at R = 32 with 30 Levenberg-Marquardt iterations per start, in float64
and in float32.  Everything comes from this project's own code; about a minute on a CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_recover.py

Per precision tag (64, 32) and image: the three float32 starts, their energies before and after, the final
parameters, the winner, and the IoU (grid 64, classes.IoUAccuracy on the CPU) of every start's result and
of the winner's against the label.  The file exists so that no GPU test spends a minute in a host loop;
tests/test_recover_cpu.py regenerates one image and compares.
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

R, ITERS, E0, IOU_GRID = 32, 30, 1.0, 64
TAGS = (("64", np.float64), ("32", np.float32))


def rows_of(image, label, dt):
    """One image [256,256] f32 in [0,1] and its label [12] -> the fixture's rows for dtype dt."""
    import classes
    import _recover_ref
    r = _recover_ref.recover_one(image, R, iters=ITERS, e0=E0, dt=dt)
    acc = classes.IoUAccuracy(IOU_GRID, "cpu", reduce=False)
    lab = torch.tensor(np.tile(label, (3, 1)), dtype=torch.float64)
    iou = acc(lab, torch.tensor(r["params"], dtype=torch.float64)).numpy()
    return dict(starts=r["starts"], before=r["before"], after=r["after"], params=r["params"],
                winner=np.int32(r["winner"]), iou=iou, iou_winner=iou[r["winner"]])


def main():
    torch.set_num_threads(8)
    d = np.load(os.path.join(HERE, "example_images.npz"), allow_pickle=False)
    ex = d["images"].astype(np.float32) / 255.0
    labels = d["labels"].astype(np.float32)
    out = {"R": np.int32(R), "iters": np.int32(ITERS), "e0": np.float64(E0), "iou_grid": np.int32(IOU_GRID)}
    for tag, dt in TAGS:
        rows = [rows_of(ex[i], labels[i], dt) for i in range(len(ex))]
        for k in rows[0]:
            out["%s_%s" % (k, tag)] = np.stack([r[k] for r in rows])
        for i, r in enumerate(rows):
            print("f%s image %d: before %s after %s winner %d IoU %s" % (
                tag, i, " ".join("%.3g" % v for v in r["before"]), " ".join("%.3e" % v for v in r["after"]),
                r["winner"], " ".join("%.3f" % v for v in r["iou"])))
    np.savez_compressed(os.path.join(HERE, "recover.npz"), **out)
    print("wrote recover.npz")


if __name__ == "__main__":
    main()
