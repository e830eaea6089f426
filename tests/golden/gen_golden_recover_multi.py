"""Generate tests/golden/recover_multi.npz: the six-start recovery's host pipeline (tests/_free_space_ref.py on
tests/_recover_ref.py and tests/_lm_ref.py) on the ten example images (example_images.npz) at R = 32 with 30
Levenberg-Marquardt iterations per start, depth 1, margin 1/255 and free-space weight 1, in float64 and in
float32.  Everything comes from this project's own code; a few minutes on a CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_recover_multi.py

Per precision tag (64, 32) and image: the six float32 starts, their point energies before and after, the
free-space energy and the score of every result, the final parameters, the winner, and the IoU (grid 64,
classes.IoUAccuracy on the CPU) of every start's result and of the winner's against the label.  The file exists
so that no GPU test spends those minutes in a host loop; tests/test_recover_multi_cpu.py regenerates one image
and compares.
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

R, ITERS, E0, DEPTH, MARGIN, W_FS, IOU_GRID = 32, 30, 1.0, 1.0, 1.0 / 255.0, 1.0, 64
TAGS = (("64", np.float64), ("32", np.float32))


def rows_of(image, label, dt):
    """One image [256,256] f32 in [0,1] and its label [12] -> the fixture's rows for dtype dt."""
    import classes
    import _free_space_ref as fsr
    r = fsr.recover6_one(image, R, iters=ITERS, e0=E0, depth=DEPTH, margin=MARGIN, w_fs=W_FS, dt=dt)
    acc = classes.IoUAccuracy(IOU_GRID, "cpu", reduce=False)
    lab = torch.tensor(np.tile(label, (6, 1)), dtype=torch.float64)
    iou = acc(lab, torch.tensor(r["params"], dtype=torch.float64)).numpy()
    return dict(starts=r["starts"], before=r["before"], after=r["after"], fs=r["fs"], score=r["score"],
                params=r["params"], winner=np.int32(r["winner"]), iou=iou, iou_winner=iou[r["winner"]])


def main():
    torch.set_num_threads(8)
    d = np.load(os.path.join(HERE, "example_images.npz"), allow_pickle=False)
    ex = d["images"].astype(np.float32) / 255.0
    labels = d["labels"].astype(np.float32)
    out = {"R": np.int32(R), "iters": np.int32(ITERS), "e0": np.float64(E0), "depth": np.float64(DEPTH),
           "margin": np.float64(MARGIN), "w_fs": np.float64(W_FS), "iou_grid": np.int32(IOU_GRID)}
    for tag, dt in TAGS:
        rows = [rows_of(ex[i], labels[i], dt) for i in range(len(ex))]
        for k in rows[0]:
            out["%s_%s" % (k, tag)] = np.stack([r[k] for r in rows])
        for i, r in enumerate(rows):
            print("f%s image %d: after %s fs %s winner %d IoU %s" % (
                tag, i, " ".join("%.3e" % v for v in r["after"]), " ".join("%.3e" % v for v in r["fs"]),
                r["winner"], " ".join("%.3f" % v for v in r["iou"])), flush=True)
    np.savez_compressed(os.path.join(HERE, "recover_multi.npz"), **out)
    print("wrote recover_multi.npz")


if __name__ == "__main__":
    main()
