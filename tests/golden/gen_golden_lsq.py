"""Generate tests/golden/least_squares.npz from the REAL reference's LeastSquares (classes.py:297-371).

Run where the reference checkout is present (it never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_lsq.py

As gen_golden.py: the reference's torch/ modules import cv2, h5py, torchsummary and torchvision at
module level although LeastSquares uses none of them, so empty placeholder modules stand in for the
ones that are not installed; every number below comes out of the reference's own class on torch CPU.

Per case: loss and autograd gradient (d loss / d pred) in the reference's precision (float32 inputs)
and with the inputs upcast to float64 (the class runs in either).  The images are not stored: each
case names the example images it uses (example_images.npz) and how they are transformed; the lines of
build_images() are repeated in tests/_lsq_cases.py.  Parameters and results only: a few KB.
"""
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference/torch"
HERE = os.path.dirname(os.path.abspath(__file__))


def _install_placeholders():
    for name in ("cv2", "h5py", "torchsummary", "torchvision", "tqdm"):
        if name in sys.modules:
            continue
        try:
            __import__(name)
            continue
        except ImportError:
            pass
        m = types.ModuleType(name)
        if name == "torchsummary":
            m.summary = lambda *a, **k: None
        if name == "torchvision":
            m.models = types.ModuleType("torchvision.models")
        if name == "tqdm":
            m.tqdm = lambda x, *a, **k: x
        sys.modules[name] = m
    sys.path.insert(0, REF)


def build_images(kind, idx, ex):
    x = ex[np.asarray(idx)]
    if kind == "unit":
        return x
    if kind == "raw255":
        return x * np.float32(255.0)
    if kind == "big512":
        return np.kron(x, np.ones((1, 1, 2, 2), np.float32))
    if kind == "zero":
        return np.zeros_like(x)
    if kind == "onepix":
        out = np.zeros_like(x)
        for i in range(len(x)):
            nz = np.argwhere(x[i, 0] > 0)
            r, c = nz[len(nz) // 2] // 8 * 8
            out[i, 0, r, c] = max(x[i, 0, r, c], np.float32(0.5))
        return out
    raise ValueError(kind)


def main():
    _install_placeholders()
    import classes  # noqa: E402

    torch.set_num_threads(8)
    cpu = torch.device("cpu")
    d = np.load(os.path.join(HERE, "example_images.npz"), allow_pickle=False)
    ex = d["images"].astype(np.float32)[:, None] / 255.0
    labels = d["labels"].astype(np.float32)
    rng = np.random.default_rng(20261019)
    cases = []

    def add(name, R, kind, idx, pred):
        true = build_images(kind, idx, ex)
        res = {}
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            p = torch.tensor(pred, dtype=torch.float32).to(dt).requires_grad_(True)
            loss = classes.LeastSquares(R, cpu)(torch.tensor(true).to(dt), p)
            assert loss.dtype == dt
            loss.backward()
            res["loss" + tag] = loss.detach().numpy()
            res["grad" + tag] = p.grad.numpy().copy()
        cases.append(dict(name=name, R=R, kind=kind, idx=np.asarray(idx), pred=pred.astype(np.float32), **res))
        print("%-16s loss32 %.9g loss64 %.9g" % (name, res["loss32"], res["loss64"]))

    def noisy(idx):
        return (labels[idx] + 0.05 * rng.normal(size=(len(idx), 12))).astype(np.float32)

    # the labels themselves: points on the surface, F - 1 is all cancellation
    add("labels_R32", 32, "unit", [0, 1, 2], labels[[0, 1, 2]])
    add("labels_R48", 48, "unit", [3, 4, 5], labels[[3, 4, 5]])
    add("labels_R64", 64, "unit", [6, 7, 8], labels[[6, 7, 8]])
    # labels + 0.05 N(0,1): a network-like prediction
    add("noisy_R32", 32, "unit", [9, 0, 1], noisy([9, 0, 1]))
    add("noisy_R48", 48, "unit", [2, 3, 4], noisy([2, 3, 4]))
    add("noisy_R64", 64, "unit", [5, 6, 7], noisy([5, 6, 7]))
    # raw 0..255 targets (what the reference's dataset feeds: classes.py:63,84), 512^2 targets
    add("raw255_R32", 32, "raw255", [8, 9, 0], noisy([8, 9, 0]))
    add("big512_R32", 32, "big512", [1, 2, 3], noisy([1, 2, 3]))
    add("big512_R64", 64, "big512", [4, 5, 6], noisy([4, 5, 6]))
    # a, e, t outside their clamps on both sides
    pe = noisy([7, 8, 9])
    pe[0, 0] = 0.01; pe[0, 3] = 0.05; pe[0, 6] = -0.2   # below
    pe[1, 2] = 1.3; pe[1, 4] = 1.2; pe[1, 5] = 1.1      # above
    pe[2, 1] = 0.02; pe[2, 0] = 1.5; pe[2, 3] = 1.4; pe[2, 4] = 0.01; pe[2, 7] = -0.1; pe[2, 5] = 1.2
    add("clamps_R32", 32, "unit", [7, 8, 9], pe)
    # an image without points, an image with exactly one
    add("zero_R32", 32, "zero", [0, 1, 2], noisy([0, 1, 2]))
    add("onepix_R32", 32, "onepix", [3, 4, 5], noisy([3, 4, 5]))

    out = {}
    for i, c in enumerate(cases):
        for k, v in c.items():
            out["c%d_%s" % (i, k)] = np.asarray(v)
    out["n"] = np.asarray(len(cases))
    np.savez_compressed(os.path.join(HERE, "least_squares.npz"), **out)
    print("wrote least_squares.npz (%d cases)" % len(cases))


if __name__ == "__main__":
    main()
