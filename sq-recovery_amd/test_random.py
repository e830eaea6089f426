"""Drop-in for torch/test_random.py (timoblak/sq-recovery): evaluate a trained ResNetSQ checkpoint on
fresh random superquadrics.

    python test_random.py [--model trained_models/model_explicit.pt] [--n 1000] [--batch 64]
                          [--render-size 128] [--seed 0] [--results results.txt]

The reference draws one instance at a time, runs the external `scanner` binary on it through os.system
and reads the BMP back.  Here the instances (classes.sample_sq_params: the same distribution) are rendered
on the device in batches by the scanner-style renderer (sqr_scan_render), predicted with net.eval(), and
scored with IoUAccuracy(render_size, reduce=False) per sample.  The true and predicted parameters (a and t
in pixel units, x255, like the reference) and the IoU of every example are appended to --results; the mean
and standard deviation are printed.  A missing checkpoint means random weights, with a notice, like test.py.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from classes import IoUAccuracy, sample_sq_params  # noqa: E402
from helpers import load_model  # noqa: E402
from models import ResNetSQ  # noqa: E402
from sqr import cpu as _cpu  # noqa: E402
from sqr import losses as _L  # noqa: E402


def _fmt(p):
    return "%s %s %s %s" % (p[0:3] * 255, p[3:5], p[5:8] * 255, p[8:12])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", default="trained_models/model_explicit.pt")
    ap.add_argument("--n", type=int, default=1000, help="number of random instances")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--render-size", type=int, default=128, help="IoUAccuracy grid (test_random.py:25)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--results", default="results.txt")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if args.n < 1 or args.batch < 1:
        ap.error("--n and --batch must be >= 1")
    device = torch.device(args.device)

    net = ResNetSQ(outputs=4, pretrained=False).to(device)
    if os.path.exists(args.model):
        _, net, _, _ = load_model(args.model, net, None)
    else:
        print("checkpoint %s not found: using random weights" % args.model)
    net.eval()
    acc = IoUAccuracy(render_size=args.render_size, device=device, reduce=False)
    labels = sample_sq_params(np.random.default_rng(args.seed), args.n)
    scan = _L.scan_render if device.type == "cuda" else _cpu.scan_render

    ious = []
    with open(args.results, "a") as f, torch.no_grad():
        for i in range(0, args.n, args.batch):
            true = torch.from_numpy(labels[i:i + args.batch]).to(device)
            x = scan(true, 256, 255).to(torch.float32).unsqueeze(1)  # the 8-bit image / 255 (test_random.py:47-48)
            pred = torch.cat([o.float() for o in net(x)], dim=1)
            iou = acc(true, pred).cpu().numpy()
            for k, (pt, pp) in enumerate(zip(true.cpu().numpy(), pred.cpu().numpy())):
                print("---------- Example %d ----------" % (i + k), file=f)
                print("True params:", _fmt(pt), file=f)
                print("Pred params:", _fmt(pp), file=f)
                print("- Accuracy:", iou[k] * 100, file=f)
            ious.append(iou)
    ious = np.concatenate(ious)
    print("IoU over %d random instances (render size %d)" % (args.n, args.render_size))
    print("Mean: ", ious.mean())
    print("Std: ", ious.std())
    return ious


if __name__ == "__main__":
    main()
