"""Generate tests/golden/loss_edges.npz from the REAL reference (classes.py on torch CPU, float32).

Run where the reference is checked out (it never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_loss_edges.py

Two edges of the loss kernels that loss/implicit/explicit/iou.npz do not reach:

  * the zero fix (classes.py:261-263, A1 == 0 -> 1e-4) on rows where it fires on whole planes of the
    grid: a = (.25, .25, .25), t = (.5, .25, .75), q = (0, 0, 0, 1) and a grid whose nodes are dyadic
    (ImplicitLoss / IoUAccuracy: R - 1 a power of two; ExplicitLoss: R a power of two).  Every
    coordinate, difference and quotient is exact in fp32 and in float64, so the reference's fp32 code,
    the float64 oracle and the kernel all see the same exact zeros.
  * np.arange(0, 1 + 1/R, 1/R) returning R + 2 nodes (R = 6, 9): the last one lies above 1.

Cases (prefix c<i>_ as in the other fixtures, read with tests/_golden.py::cases):
  implicit  dyadic_R5 / R9 / R17: true [3,1,R,R] (the reference's own depth image of the row plus a
            random sign times uniform [0.01, 0.3]), pred [3,12], loss, grad, depth [3,R,R]
  explicit  dyadic_R4 / R8 (true: a second dyadic row set), arange_R6 / R9 (two random rows each)
  iou       dyadic_R5 / R9: iou, iou_per, and the counts recomputed from the reference's own
            per-voxel tensors (inter, union)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import _install_placeholders, sample_params  # noqa: E402

TAU, SHARP = 1.5, 260.0
DY_E = ((1.0, 1.0), (0.5, 1.0), (1.0, 0.25))


def dyadic_rows(a=(0.25, 0.25, 0.25), t=(0.5, 0.25, 0.75)):
    return np.array([list(a) + list(e) + list(t) + [0, 0, 0, 1] for e in DY_E], np.float32)


def pack(cases):
    out = {}
    for i, c in enumerate(cases):
        for k, v in c.items():
            out["c%d_%s" % (i, k)] = np.asarray(v)
    out["n"] = np.asarray(len(cases))
    return out


def main():
    _install_placeholders()
    import classes  # noqa: E402

    torch.set_num_threads(4)
    cpu = torch.device("cpu")
    rng = np.random.default_rng(20261021)
    pred = dyadic_rows()
    other = dyadic_rows(a=(0.5, 0.25, 0.25), t=(0.5, 0.5, 0.5))

    imp = []
    for R in (5, 9, 17):
        crit = classes.ImplicitLoss(R, cpu, TAU, SHARP)
        p = torch.tensor(pred, requires_grad=True)
        depth = crit.depth_projection(p.detach()).numpy().reshape(3, R, R)
        sign = np.where(rng.uniform(size=depth.shape) < 0.5, -1.0, 1.0)
        true = (depth + sign * rng.uniform(0.01, 0.3, depth.shape)).astype(np.float32)[:, None]
        loss = crit(torch.tensor(true), p)
        loss.backward()
        imp.append(dict(name="dyadic_R%d" % R, R=R, tau=TAU, s=SHARP, true=true, pred=pred, loss=loss.item(),
                        grad=p.grad.numpy().copy(), depth=depth))

    exp = []
    for name, R, tp, pp in (("dyadic_R4", 4, other, pred), ("dyadic_R8", 8, other, pred),
                            ("arange_R6", 6, sample_params(rng, 2), sample_params(rng, 2)),
                            ("arange_R9", 9, sample_params(rng, 2), sample_params(rng, 2))):
        crit = classes.ExplicitLoss(R, cpu)
        p = torch.tensor(pp, requires_grad=True)
        loss = crit(torch.tensor(tp), p)
        loss.backward()
        exp.append(dict(name=name, R=R, true=tp, pred=pp, loss=loss.item(), grad=p.grad.numpy().copy()))

    iou = []
    for R in (5, 9):
        red = classes.IoUAccuracy(R, cpu)(torch.tensor(other), torch.tensor(pred)).item()
        per = classes.IoUAccuracy(R, cpu, reduce=False)(torch.tensor(other), torch.tensor(pred)).numpy()
        acc = classes.IoUAccuracy(R, cpu)
        a_bin, b_bin = acc.ins_outs(torch.tensor(other)) <= 1, acc.ins_outs(torch.tensor(pred)) <= 1
        counts = np.stack([(a_bin & b_bin).sum((1, 2, 3)).numpy(), (a_bin | b_bin).sum((1, 2, 3)).numpy()], 1)
        iou.append(dict(name="dyadic_R%d" % R, R=R, true=other, pred=pred, iou=red, iou_per=per,
                        counts=counts.astype(np.int64)))

    out = {}
    for kind, cs in (("implicit", imp), ("explicit", exp), ("iou", iou)):
        for k, v in pack(cs).items():
            out["%s_%s" % (kind, k)] = v
    np.savez_compressed(os.path.join(HERE, "loss_edges.npz"), **out)
    print("wrote loss_edges.npz:", {k: len(v) for k, v in (("implicit", imp), ("explicit", exp), ("iou", iou))})


if __name__ == "__main__":
    main()
