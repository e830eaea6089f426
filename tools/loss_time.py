"""The fused ImplicitLoss call (loss + analytic gradient, bench.time_loss_call: graph replays) at the
bench shapes; one JSON line.  Environment knobs of libsqr's A/B builds pass through (SQR_*).

    python tools/loss_time.py leastsquares

times the LeastSquares loss instead, forward + backward at B = 64, R = 64, 256^2 on CUDA tensors: the
HIP kernel path (eagerly, host clock around a device synchronise, and per call inside a replayed graph)
against the plain-torch path (the reference's per-image code, which cannot be captured: every
torch.where waits for the device)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sq-recovery_amd"))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import classes  # noqa: E402
from sqr import losses  # noqa: E402


def _eager_ms(fn, warmup=3, reps=20):
    """Host time of fn() per call, the device drained before and after."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def least_squares(dev, R=64, H=256, B=64):
    p = torch.tensor(classes.sample_sq_params(np.random.default_rng(0), B), device=dev)
    img = losses.implicit_render(p, H, 1.5, 260).unsqueeze(1).contiguous()
    torch.manual_seed(0)
    pred = (p + 0.02 * torch.randn_like(p)).requires_grad_(True)
    crit = classes.LeastSquares(R, dev)

    def kernel_path():
        pred.grad = None
        crit(img, pred).backward()

    def torch_path():  # the class's CPU branch, on the CUDA tensors
        pred.grad = None
        crit.energy_function(crit.batch_points(img), pred).mean().backward()

    return {"shape": "R%d_H%d_B%d" % (R, H, B),
            "points_per_image": round(float((torch.nn.functional.interpolate(img, size=(R, R)) > 0).sum()) / B, 1),
            "kernel_eager_ms": round(_eager_ms(kernel_path), 4),
            "torch_eager_ms": round(_eager_ms(torch_path), 4),
            "kernel_in_graph_us": round(bench.time_loss_call(crit, img, B, dev, reps=10) * 1e3, 2)}


def main():
    dev = torch.device("cuda", 0)
    out = {"env": {k: v for k, v in os.environ.items() if k.startswith("SQR_")}}
    if sys.argv[1:] == ["leastsquares"]:
        out["leastsquares"] = least_squares(dev)
        print(json.dumps(out))
        return
    for R, H, B in ((32, 256, 64), (64, 256, 64), (64, 512, 16)):
        p = torch.tensor(classes.sample_sq_params(np.random.default_rng(0), B), device=dev)
        img = losses.implicit_render(p, H, 1.5, 260).unsqueeze(1).contiguous()
        crit = classes.ImplicitLoss(R, dev, 1.5, 260)
        ms = bench.time_loss_call(crit, img, B, dev, reps=10)
        tps = B * R ** 3 * bench.LOSS_TRANSC_PER_VOXEL / (ms * 1e-3) / 1e12
        out["R%d_H%d_B%d" % (R, H, B)] = {"us": round(ms * 1e3, 2), "frac": round(tps / bench.PEAK_TRANSC_TPS, 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
