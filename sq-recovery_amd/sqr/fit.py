"""Point-set refinement of predicted superquadrics: descend the LeastSquares energy of the image's own
points, with Adam (refine) or with Levenberg-Marquardt (refine_lm); and the recovery without a prediction
(recover): the classical start from the points' moments, refined by Levenberg-Marquardt.

The classical recovery (Solina & Bajcsy) fits a superquadric to the depth image's points by iterating
on the energy a0 a1 a2 sum_points (F - 1)^2; the reference keeps that energy as its LeastSquares loss
(torch/classes.py:297-371).  It needs the image only, no label, so it can polish a network
prediction: predict, then descend.  What this promises is a lower energy — a better fit of the
visible points — not a higher IoU against a label: the depth image shows one side of the object.

Everything runs on the device (Adam: sqr_least_squares_fwd_bwd per step plus a handful of elementwise
launches on the [B,12] tensor; LM: sqr_lsq_lm_refine, one chain of normal-equations and step kernels;
recover: the starts' four launches, one such chain over every start of every image and a selection,
sqr_lsq_recover on the lowest energy of three starts, sqr_lsq_recover_multi on a score with a free-space
evaluation, from three or six starts and the caller's); nothing is read back inside the loop.
"""
import torch

from .losses import least_squares, lm_refine, lsq_recover, lsq_recover_multi, lsq_starts


def refine_lm(images, params, iters=10, render_size=32, lambda0=1e-3, up=10.0, down=0.1, return_info=False):
    """images [B,1,H,W] or [B,H,W], params [B,12] (CUDA) -> (refined [B,12] f32, energy_before [B] f64,
    energy_after [B] f64), with return_info also the accepted step counts [B] i32.

    Levenberg-Marquardt, Solina & Bajcsy's method: damped Gauss-Newton on the residuals
    sqrt(a0 a1 a2) (F(point) - 1), solving (J^T J + lambda diag(J^T J)) delta = -J^T r per sample.  A step
    is kept only if it lowers the energy (lambda *= down), otherwise lambda *= up.  The start and every
    trial are projected: a, e, t clamped into their ranges, q normalised, so the result is a unit
    quaternion with in-range parameters, and energy_before is the energy at the projected start.  Every
    sample is refined on its own; no host wait, so the call can be captured in a HIP graph."""
    out, before, after, accepted = lm_refine(images, params, int(render_size), int(iters), lambda0, up, down)
    return (out, before, after, accepted) if return_info else (out, before, after)


def recover(images, iters=30, render_size=32, e0=1.0, lambda0=1e-3, up=10.0, down=0.1, return_info=False,
            starts="classic", depth=1.0, free_space=0.0, margin=1.0 / 255.0, extra_starts=None):
    """images [B,1,H,W] or [B,H,W] (CUDA) -> (params [B,12] f32, energy [B] f64, start_index [B] i32), with
    return_info also a dict: params [K,B,12], energy_before [K,B], energy_after [K,B], accepted [K,B] of every
    start, the starts themselves [K,B,12] and the moments (count, centroid, eigenvalues, frame).

    Solina & Bajcsy's recovery, no network and no label: the centre of gravity and the principal axes of the
    image's points give position and orientation, the extents along those axes the sizes, an ellipsoid
    (e = e0) the shape; refine_lm's iteration goes on from each of the three cyclic permutations of the axes
    and the start that ends with the lowest energy wins (the lowest index on a tie).  The result has in-range
    parameters and a unit quaternion, and its energy is no higher than that of any of the three projected
    starts.  As with refine, the promise is a low energy, a good fit of the visible points, not a high IoU
    against a label: the depth image shows one side of the object, and the lowest energy is not always the
    best IoU.  An image without points returns the default start (a = 0.05, t = 0.5, identity rotation) with
    energy 0.  Every sample is recovered on its own; no host wait, so the call can be captured in a HIP
    graph.

    The defaults (starts="classic", free_space=0, no extra_starts) are that call, sqr_lsq_recover: the three
    starts of every image refined in one chain over all 3 B samples (so 3 B <= 65535) and selected by energy.
    Anything else goes through sqr_lsq_recover_multi, the same chain over all K B samples with a free-space
    evaluation behind it:
      starts="depth"   six starts, K = 6: the three above and three whose extent along the frame axis nearest
                       the viewing direction is stretched by `depth` times itself away from the viewer (the
                       image shows the front half of the body only: lsq_starts6)
      free_space=w     the winner is the lowest score = energy + w * free-space energy (free_space_energy with
                       `margin`): a model that fits the points but occupies space the image shows to be empty
                       loses.  `energy` stays the winner's point energy.
      extra_starts     [B,12] or [Kx,B,12] more starts behind the computed ones (a network's prediction, for
                       instance); start_index counts them from 3 or 6 on.
    With return_info the dict then also holds energy_fs [K,B], score [K,B] and the winner's energy_fs [B] under
    "winner_energy_fs".

    return_info costs a second run of the starts (sqr_lsq_starts: four more short launches and five small
    allocations) for the moments: the recovery keeps them in its workspace, whose layout is not part of its
    interface.  The starts' kernels are bitwise reproducible, so the moments returned are exactly the ones
    that were used."""
    R = int(render_size)
    if starts not in ("classic", "depth"):
        raise ValueError("recover: starts must be 'classic' or 'depth', got %r" % (starts,))
    if starts == "classic" and float(free_space) == 0.0 and extra_starts is None:
        out, energy, index, allp, before, after, accepted = lsq_recover(images, R, int(iters), e0, lambda0, up, down)
        if not return_info:
            return out, energy, index
        st, info = lsq_starts(images, R, e0)
        info = dict(info, params=allp, energy_before=before, energy_after=after, accepted=accepted, starts=st)
        return out, energy, index, info
    out, energy, fs, index, multi = lsq_recover_multi(images, R, int(iters), 6 if starts == "depth" else 3, e0, depth,
                                                      extra_starts, lambda0, up, down, free_space, margin)
    if not return_info:
        return out, energy, index
    _, info = lsq_starts(images, R, e0)
    return out, energy, index, dict(info, winner_energy_fs=fs, **multi)


def refine(images, params, steps=200, lr=2e-3, render_size=32, betas=(0.9, 0.999), eps=1e-8, method="adam"):
    """images [B,1,H,W] or [B,H,W], params [B,12] (CUDA) -> (refined [B,12] f32, energy_before [B] f64,
    energy_after [B] f64).  method "lm": refine_lm with `steps` iterations (lr, betas, eps unused).

    Adam (torch.optim.Adam's update, bias-corrected) on a detached copy of params.  The objective is
    the sum of the per-sample energies and Adam is elementwise, so every image is refined on its own:
    a sample's result does not depend on what else is in the batch."""
    if method == "lm":
        return refine_lm(images, params, iters=steps, render_size=render_size)
    if method != "adam":
        raise ValueError("refine: method must be 'adam' or 'lm', got %r" % (method,))
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
