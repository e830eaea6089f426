"""The LeastSquares fixture's images: tests/golden/least_squares.npz stores parameters and results only;
every case's images are built here from the 10 example depth images (tests/golden/example_images.npz),
by the same lines tests/golden/gen_golden_lsq.py used."""
import numpy as np

from _golden import cases, load


def example():
    """(images [10,1,256,256] f32 in [0,1], labels [10,12] f32)."""
    d = load("example_images.npz")
    return d["images"].astype(np.float32)[:, None] / 255.0, d["labels"].astype(np.float32)


def build_images(kind, idx, ex):
    """The [len(idx),1,H,W] f32 target of a case: `kind` applied to the example images `idx`."""
    x = ex[np.asarray(idx)]
    if kind == "unit":  # [0,1] depth, 256x256
        return x
    if kind == "raw255":  # what the reference's H5Dataset feeds: 0..255
        return x * np.float32(255.0)
    if kind == "big512":  # each pixel repeated 2x2
        return np.kron(x, np.ones((1, 1, 2, 2), np.float32))
    if kind == "zero":  # no point at all
        return np.zeros_like(x)
    if kind == "onepix":  # exactly one point at R = 32: one 8x8 source cell around the object's middle pixel
        out = np.zeros_like(x)
        for i in range(len(x)):
            nz = np.argwhere(x[i, 0] > 0)
            r, c = nz[len(nz) // 2] // 8 * 8
            out[i, 0, r, c] = max(x[i, 0, r, c], np.float32(0.5))
        return out
    raise ValueError(kind)


def golden_cases():
    """The fixture's cases with their images rebuilt: dicts with name, R, true, pred, loss32, grad32,
    loss64, grad64."""
    ex, _ = example()
    out = []
    for c in cases("least_squares.npz"):
        c = dict(c)
        c["name"], c["R"] = str(c["name"]), int(c["R"])
        c["true"] = build_images(str(c["kind"]), c["idx"], ex)
        out.append(c)
    return out
