"""Drop-in for torch/test.py (timoblak/sq-recovery): predict the superquadric parameters of one
depth image with a trained ResNetSQ checkpoint (helpers.load_model format) on MI355X.

    python test.py [--image ../data/example_imgs/000000.bmp] [--model trained_models/model_explicit.pt]

Prints size a and position t in pixel units (x255) like the reference (test.py:40-44).  The
image window of the reference (cv2.imshow) is shown only with --show and OpenCV installed.

--refine N polishes the prediction with N Adam steps (--refine-lr) down the LeastSquares energy of the
image's own points (sqr.fit.refine, on the GPU) and prints the energy before and after and the refined
parameters in the same format.  The energy goes down; the IoU against a label need not go up.
--refine-method lm runs N Levenberg-Marquardt iterations instead (sqr.fit.refine_lm): the energy is that
of the projected prediction (a, e, t clamped, q normalised) and the result is a unit quaternion.

--classical builds no network and reads no checkpoint: the parameters are recovered from the image's points
alone (sqr.fit.recover: Solina & Bajcsy's start from the points' moments, --classical-iters
Levenberg-Marquardt iterations from each of three axis orders, the lowest energy wins) and printed in the
same format with that energy and the winning start.  It composes with --refine.
--starts depth adds three depth-aware starts (the extent along the viewing direction doubled away from the viewer:
the image shows the front half only) and refines all six as one batch; --free-space W picks the winner by
energy + W x the free-space energy (a model must not occupy space the image shows to be empty).  With
--classical-starts (and a --model checkpoint) the network's prediction competes as one more start.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from helpers import load_model, read_image_gray  # noqa: E402
from models import ResNetSQ  # noqa: E402


def predict(net, img_u8, device):
    """uint8 [H,W] depth image -> (a, e, t, q) numpy arrays of the single prediction."""
    x = torch.from_numpy(img_u8.astype(np.float32)[None, None] / 255).to(device)
    with torch.no_grad():
        out = net(x)
    return tuple(o.detach().cpu().numpy() for o in out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--image", default="../data/example_imgs/000000.bmp")
    ap.add_argument("--model", default="trained_models/model_explicit.pt")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--show", action="store_true")
    ap.add_argument("--refine", type=int, default=0, metavar="N",
                    help="refine the prediction with N Adam steps on the LeastSquares energy (CUDA)")
    ap.add_argument("--refine-lr", type=float, default=2e-3)
    ap.add_argument("--refine-method", choices=("adam", "lm"), default="adam",
                    help="adam: N Adam steps; lm: N Levenberg-Marquardt iterations (sqr.fit.refine_lm)")
    ap.add_argument("--classical", action="store_true",
                    help="no network, no checkpoint: recover the parameters from the image's points alone "
                         "(sqr.fit.recover, CUDA)")
    ap.add_argument("--classical-iters", type=int, default=30, metavar="N",
                    help="Levenberg-Marquardt iterations per start of --classical")
    ap.add_argument("--starts", choices=("classic", "depth"), default="classic",
                    help="--classical: the three starts, or those and three depth-aware ones")
    ap.add_argument("--free-space", type=float, default=0.0, metavar="W",
                    help="--classical: select by energy + W x free-space energy")
    ap.add_argument("--classical-starts", action="store_true",
                    help="run the network and the classical recovery together: the prediction is one more start")
    args = ap.parse_args(argv)

    img = read_image_gray(args.image)
    if args.classical:
        from sqr.fit import recover
        x = torch.from_numpy(img.astype(np.float32)[None, None] / 255).to(args.device)
        pred, energy, start = recover(x, iters=args.classical_iters, starts=args.starts, free_space=args.free_space)
        a, e, t, q = (o.cpu().numpy() for o in torch.split(pred, (3, 2, 3, 4), dim=1))
        print("Recovered parameters (classical, %d Levenberg-Marquardt iterations per start, LeastSquares energy "
              "%.6g, start %d): " % (args.classical_iters, energy.item(), start.item()))
    elif args.classical_starts:
        from sqr.fit import recover
        net = ResNetSQ(outputs=4, pretrained=False).to(args.device)
        if os.path.exists(args.model):
            _, net, _, _ = load_model(args.model, net, None)
        else:
            print("checkpoint %s not found: using random weights" % args.model)
        net.eval()
        x = torch.from_numpy(img.astype(np.float32)[None, None] / 255).to(args.device)
        guess = torch.from_numpy(np.concatenate(predict(net, img, args.device), 1)).to(args.device)
        pred, energy, start = recover(x, iters=args.classical_iters, starts=args.starts, free_space=args.free_space,
                                      extra_starts=guess)
        nown = 6 if args.starts == "depth" else 3
        a, e, t, q = (o.cpu().numpy() for o in torch.split(pred, (3, 2, 3, 4), dim=1))
        print("Recovered parameters (classical starts and the prediction, %d Levenberg-Marquardt iterations per "
              "start, LeastSquares energy %.6g, start %d%s): " % (
                  args.classical_iters, energy.item(), start.item(),
                  " = the prediction" if start.item() == nown else ""))
    else:
        net = ResNetSQ(outputs=4, pretrained=False).to(args.device)
        if os.path.exists(args.model):
            _, net, _, _ = load_model(args.model, net, None)
        else:
            print("checkpoint %s not found: using random weights" % args.model)
        net.eval()
        a, e, t, q = predict(net, img, args.device)
        print("Predicted parameters: ")
    print("Size a:", a * 255)
    print("Shape e:", e)
    print("Position t:", t * 255)
    print("Rotation q:", q)
    if args.refine:
        from sqr.fit import refine
        x = torch.from_numpy(img.astype(np.float32)[None, None] / 255).to(args.device)
        pred = torch.from_numpy(np.concatenate([a, e, t, q], 1)).to(args.device)
        pred, before, after = refine(x, pred, steps=args.refine, lr=args.refine_lr, method=args.refine_method)
        a, e, t, q = (o.cpu().numpy() for o in torch.split(pred, (3, 2, 3, 4), dim=1))
        if args.refine_method == "lm":
            print("Refined parameters (%d Levenberg-Marquardt iterations, LeastSquares energy %.6g -> %.6g): "
                  % (args.refine, before.item(), after.item()))
        else:
            print("Refined parameters (%d steps, LeastSquares energy %.6g -> %.6g): "
                  % (args.refine, before.item(), after.item()))
        print("Size a:", a * 255)
        print("Shape e:", e)
        print("Position t:", t * 255)
        print("Rotation q:", q)
    if args.show:
        import cv2
        cv2.imshow("image", img)
        cv2.waitKey(0)
    return a, e, t, q


if __name__ == "__main__":
    main()
