"""test_random.py with a choice of method: evaluate a checkpoint, or the classical baseline, on the same fresh
random superquadrics.

    python eval_random.py [--method network|classical] [--classical-iters 30] [--starts classic|depth]
                          [--free-space W] [test_random.py's arguments]

--method network (the default) is test_random.py itself: every other argument is handed to test_random.main
unchanged.  --method classical runs the same program, the same instances (classes.sample_sq_params with
--seed), the same scanner-style render, the same IoUAccuracy(render_size, reduce=False) and the same report,
with sqr.fit.recover in place of the net: no network is built and no checkpoint is read (--model is ignored),
each rendered image goes through Solina & Bajcsy's recovery with --classical-iters Levenberg-Marquardt
iterations per start; --starts depth refines six starts (three of them depth-aware) as one batch and
--free-space W selects by energy + W x free-space energy (sqr.fit.recover's arguments).  CUDA only.  main(argv) returns the IoU array, like test_random.main.

test_random.py stays as it is, and nothing of it is repeated here: for the classical method its two model hooks
(the names ResNetSQ and load_model in its namespace) are replaced for the duration of the call by a module that
calls sqr.fit.recover and by a loader that loads nothing.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_random  # noqa: E402


class _Recovery(torch.nn.Module):
    """Stands where test_random.py builds ResNetSQ: images [B,1,H,W] -> (a, e, t, q) from sqr.fit.recover."""

    def __init__(self, iters, starts="classic", free_space=0.0):
        super().__init__()
        self.iters, self.starts, self.free_space = iters, starts, free_space

    def forward(self, x):
        from sqr.fit import recover
        pred = recover(x, iters=self.iters, starts=self.starts, free_space=self.free_space)[0]
        return torch.split(pred, (3, 2, 3, 4), dim=1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0], add_help=False)
    ap.add_argument("--method", choices=("network", "classical"), default="network")
    ap.add_argument("--classical-iters", type=int, default=30, metavar="N")
    ap.add_argument("--starts", choices=("classic", "depth"), default="classic")
    ap.add_argument("--free-space", type=float, default=0.0, metavar="W")
    args, rest = ap.parse_known_args(argv)
    if args.method == "network":
        return test_random.main(rest)
    # an existing file as --model, so that test_random.py takes its load branch (no "random weights" notice)
    # and calls the loader below, which reads nothing
    rest = [a for i, a in enumerate(rest) if a != "--model" and (i == 0 or rest[i - 1] != "--model")]
    rest = [a for a in rest if not a.startswith("--model=")] + ["--model", os.path.abspath(__file__)]
    hooks = (test_random.ResNetSQ, test_random.load_model)
    test_random.ResNetSQ = lambda **kw: _Recovery(args.classical_iters, args.starts, args.free_space)
    test_random.load_model = lambda path, net, opt: (None, net, None, None)
    try:
        print("classical recovery (sqr.fit.recover, %d iterations per start): no network, no checkpoint"
              % args.classical_iters)
        return test_random.main(rest)
    finally:
        test_random.ResNetSQ, test_random.load_model = hooks


if __name__ == "__main__":
    main()
