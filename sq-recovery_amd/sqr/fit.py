"""Point-set refinement of predicted superquadrics: a few Adam steps down the LeastSquares energy.

The classical recovery (Solina & Bajcsy) fits a superquadric to the depth image's points by iterating
on the energy a0 a1 a2 sum_points (F - 1)^2; the reference keeps that energy as its LeastSquares loss
(torch/classes.py:297-371).  It needs the image only, no label, so it can polish a network
prediction: predict, then descend.  What this promises is a lower energy — a better fit of the
visible points — not a higher IoU against a label: the depth image shows one side of the object.

Everything runs on the device (sqr_least_squares_fwd_bwd per step plus a handful of elementwise
launches on the [B,12] tensor); nothing is read back inside the loop.
"""
import torch

from .losses import least_squares


def refine(images, params, steps=200, lr=2e-3, render_size=32, betas=(0.9, 0.999), eps=1e-8):
    """images [B,1,H,W] or [B,H,W], params [B,12] (CUDA) -> (refined [B,12] f32, energy_before [B] f64,
    energy_after [B] f64).

    Adam (torch.optim.Adam's update, bias-corrected) on a detached copy of params.  The objective is
    the sum of the per-sample energies and Adam is elementwise, so every image is refined on its own:
    a sample's result does not depend on what else is in the batch."""
    R = int(render_size)
    p = params.detach().to(torch.float32).clone().requires_grad_(True)
    before = least_squares(images, p.detach(), R, per_sample=True)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    b1, b2 = betas
    for k in range(1, int(steps) + 1):
        (g,) = torch.autograd.grad(least_squares(images, p, R, per_sample=True).sum(), p)
        with torch.no_grad():
            m.mul_(b1).add_(g, alpha=1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            denom = v.sqrt().div_((1 - b2 ** k) ** 0.5).add_(eps)
            p.addcdiv_(m, denom, value=-lr / (1 - b1 ** k))
    p = p.detach()
    after = least_squares(images, p, R, per_sample=True) if steps else before
    return p, before, after
