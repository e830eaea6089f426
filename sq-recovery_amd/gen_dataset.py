"""Generate a training set without the reference's `scanner` binary: stands in for
data/generation_scripts/gen_rand_rot.py plus the scanner run over its script (timoblak/sq-recovery).

    python gen_dataset.py --n 150000 --out ../data/ --seed 0 [--device cuda:0|cpu] [--batch 256] [--bmp] [--h5]

Draws N superquadrics from the reference's generator distribution (classes.sample_sq_params), rounds
every value to the six decimals `%f` prints, and renders each image from exactly what its label row says
(as the reference's pipeline does: the scanner is run on the printed command line) with the scanner-style
depth renderer: sqr_scan_render on the GPU, sqr/cpu.py on the host.  Writes into --out

    images.npy        uint8 [N,256,256], the depth images (0 = background)
    data_labels.csv   the reference's rows: fn, a (3, 0..255 units), e (2), t (3, 0..255 units),
                      M = quat2mat(q) row-major (9), q (4, xyzw); helpers.parse_csv reads it
    %06d.bmp          with --bmp: the images as the scanner's 24-bit BMPs
    dataset.h5        with --h5: dataset "sq" (N,1,256,256) float32 holding 0..255, what H5Dataset opens
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from classes import sample_sq_params  # noqa: E402
from helpers import quat2mat, write_image_gray  # noqa: E402
from sqr import cpu as _cpu  # noqa: E402
from sqr import losses as _L  # noqa: E402

SIZE = 256


def label_rows(labels):
    """Normalised labels [N,12] -> (the 21 printed values per row in csv units, rounded to `%f`'s six
    decimals, float64 [N,21]; the labels those rows parse back to, float32 [N,12])."""
    lab = np.asarray(labels, dtype=np.float64)
    rows = np.empty((len(lab), 21), dtype=np.float64)
    for i, p in enumerate(lab):
        head = np.concatenate([p[0:3] * 255.0, p[3:5], p[5:8] * 255.0])
        head = np.array([float("%f" % v) for v in head])
        q = np.array([float("%f" % v) for v in p[8:12]])
        M = np.array([float("%f" % v) for v in quat2mat(q).ravel()])
        rows[i] = np.concatenate([head, M, q])
    # helpers.parse_csv's arithmetic: a and t divided by 255 in float64, then float32
    parsed = np.concatenate([rows[:, 0:3] / 255.0, rows[:, 3:5], rows[:, 5:8] / 255.0, rows[:, 17:21]], axis=1)
    return rows, parsed.astype(np.float32)


def render_u8(labels, device, batch):
    """float32 labels [N,12] -> uint8 [N,256,256] scanner images, rendered in batches on `device`."""
    out = np.empty((len(labels), SIZE, SIZE), dtype=np.uint8)
    dev = torch.device(device)
    for i in range(0, len(labels), batch):
        p = torch.from_numpy(labels[i:i + batch]).to(dev)
        img = _L.scan_render(p, SIZE, 255) if dev.type == "cuda" else _cpu.scan_render(p, SIZE, 255)
        out[i:i + batch] = torch.round(img * 255).to(torch.uint8).cpu().numpy()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, required=True, help="number of images")
    ap.add_argument("--out", required=True, help="output directory")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--batch", type=int, default=256, help="images per render call")
    ap.add_argument("--bmp", action="store_true", help="also write %%06d.bmp")
    ap.add_argument("--h5", action="store_true", help="also write dataset.h5 (needs h5py)")
    args = ap.parse_args(argv)
    if args.n < 1 or args.batch < 1:
        ap.error("--n and --batch must be >= 1")
    if args.h5:
        try:
            import h5py
        except ImportError:
            raise SystemExit("gen_dataset: --h5 needs the h5py package, which is not installed; "
                             "run without --h5 (images.npy holds the same images)")
    os.makedirs(args.out, exist_ok=True)
    rows, labels = label_rows(sample_sq_params(np.random.default_rng(args.seed), args.n))
    images = render_u8(labels, args.device, args.batch)
    np.save(os.path.join(args.out, "images.npy"), images)
    with open(os.path.join(args.out, "data_labels.csv"), "w") as f:
        for i, row in enumerate(rows):
            f.write("%06d.bmp," % i + ",".join("%f" % v for v in row) + "\n")
    if args.bmp:
        for i, img in enumerate(images):
            write_image_gray(os.path.join(args.out, "%06d.bmp" % i), img)
    if args.h5:
        with h5py.File(os.path.join(args.out, "dataset.h5"), "w") as handle:
            ds = handle.create_dataset("sq", (args.n, 1, SIZE, SIZE), dtype="f")
            for i in range(0, args.n, args.batch):
                ds[i:i + args.batch] = images[i:i + args.batch, None].astype(np.float32)
    print("gen_dataset: %d images -> %s" % (args.n, args.out))
    return labels, images


if __name__ == "__main__":
    main()
