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

refine_points and recover_points are refine_lm and recover on point lists [B,P,3] (losses.pack_points) instead
of depth images: the same kernels with a second point source (sqr_pts_lm_refine, sqr_pts_recover).  A cloud
need not show one side of a body only, and it need not come from this dataset.

recover_parts fits several superquadrics to one cloud by alternating assign_points (every point to the part whose
surface is nearest) with a refit of every part, the same kernels once more on a third point source: the slots of
a cloud that carry a part's label (sqr_pts_recover_parts).
"""
import torch

from .losses import (_parts_shapes, least_squares, lm_refine, lsq_recover, lsq_recover_multi, lsq_starts,
                     pts_assign, pts_lm_refine, pts_recover, pts_recover_parts, pts_starts)


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


def normalize_points(points, count=None):
    """points [B,P,3], count [B] or None (any device, plain torch ops, no host wait) -> (points' [B,P,3] f32,
    scale [B] f32, offset [B,3] f32): every cloud moved into the unit cube, where the parameter clamps live.

    Per cloud, over its counting slots (slot i < count, clamped into [0, P], with three finite coordinates):
    lo, hi = the coordinatewise minimum and maximum, c = (lo + hi) / 2, s = 0.4 / max(hi - lo), and
    p' = (p - c) s + 0.5, all in float32.  0.4 puts the sizes where the labels' a <= 0.294 live and leaves t
    room inside [0,1].  A cloud without counting slots, or whose largest side is zero (or not finite), gets
    s = 1 and c = 0.5, so p' = p.  Slots that do not count come out as NaN.  scale = s, offset = c."""
    p = points.detach().to(torch.float32)
    B, P = p.shape[0], p.shape[1]
    on = torch.isfinite(p).all(dim=2)
    if count is not None:
        n = count.to(device=p.device, dtype=torch.int64).clamp(0, P)
        on = on & (torch.arange(P, device=p.device)[None, :] < n[:, None])
    inf = torch.full_like(p, float("inf"))
    lo = torch.where(on[:, :, None], p, inf).amin(dim=1)
    hi = torch.where(on[:, :, None], p, -inf).amax(dim=1)
    side = (hi - lo).amax(dim=1)
    ok = on.any(dim=1) & (side > 0) & torch.isfinite(side)
    scale = torch.where(ok, 0.4 / torch.where(ok, side, torch.ones_like(side)), torch.ones_like(side))
    offset = torch.where(ok[:, None], (lo + hi) / 2, torch.full_like(lo, 0.5))
    out = (p - offset[:, None, :]) * scale[:, None, None] + 0.5
    return torch.where(on[:, :, None], out, torch.full_like(out, float("nan"))), scale, offset


def denormalize_params(params, scale, offset):
    """Parameters [...,B,12] fitted to normalize_points' clouds, back in the clouds' own units (float32):
    a = a' / s, t = (t' - 0.5) / s + c; e and q unchanged."""
    p = params.to(torch.float32)
    s = scale.to(torch.float32)[:, None]
    return torch.cat([p[..., 0:3] / s, p[..., 3:5], (p[..., 5:8] - 0.5) / s + offset.to(torch.float32),
                      p[..., 8:12]], dim=-1)


def refine_points(points, params, count=None, iters=10, lambda0=1e-3, up=10.0, down=0.1, return_info=False):
    """points [B,P,3] (count [B] or None: losses.pack_points), params [B,12] or [K,B,12] (CUDA) -> (refined f32,
    energy_before f64, energy_after f64) in params' leading shape, with return_info also the accepted step counts.
    refine_lm's iteration with the cloud's counting slots as the points; one chain of launches over all samples,
    no host wait."""
    out = pts_lm_refine(points, count, params, int(iters), lambda0, up, down)
    if params.dim() == 2:
        out = tuple(x[0] for x in out)
    return out if return_info else out[:3]


def recover_points(points, count=None, iters=30, e0=1.0, lambda0=1e-3, up=10.0, down=0.1, extra_starts=None,
                   normalize=False, return_info=False):
    """points [B,P,3] (count [B] or None: losses.pack_points; CUDA) -> (params [B,12] f32, energy [B] f64,
    start_index [B] i32), with return_info also a dict: params [K,B,12], energy_before [K,B], energy_after [K,B],
    accepted [K,B] of every start, the starts [K,B,12] and the moments (count, centroid, eigenvalues, frame).

    recover on point lists: Solina & Bajcsy's three starts from the cloud's moments and extents, extra_starts
    ([B,12] or [Kx,B,12]) behind them, one Levenberg-Marquardt chain over all K B samples (K B <= 65535), the
    lowest energy wins (sqr_pts_recover).  The depth-aware starts and the free-space energy are not offered: a
    list has no viewpoint.  A cloud without counting slots returns the default start with energy 0.  No host
    wait, so the call can be captured in a HIP graph.

    The parameter clamps assume a body inside the unit cube.  normalize=True fits normalize_points' clouds
    instead and returns the parameters in the clouds' own units (denormalize_params; they then need not lie
    inside the clamps); the energy is that of the normalised fit, extra_starts are taken in normalised units,
    and info also holds normalized_params [B,12], scale [B] and offset [B,3].

    return_info costs a second run of the starts for the moments, as in recover."""
    scale = offset = None
    if normalize:
        points, scale, offset = normalize_points(points, count)
    out, energy, index, info = pts_recover(points, count, int(iters), e0, extra_starts, lambda0, up, down)
    fitted = out
    if normalize:
        out = denormalize_params(fitted, scale, offset)
    if not return_info:
        return out, energy, index
    _, moments = pts_starts(points, count, e0)
    info = dict(moments, **info)
    if normalize:
        info.update(normalized_params=fitted, scale=scale, offset=offset)
    return out, energy, index, info


def assign_points(points, params, count=None):
    """points [B,P,3] (count [B] or None), params [B,M,12] (CUDA) -> (labels [B,P] i32, dist [B,P] f32): every
    counting slot's nearest part by the radial distance d = |p - t| |1 - f^(-1/2)| (f = F^e1: the distance along the
    ray from the part's centre to its surface, in the cloud's units), the lowest part on a tie; -1 and 0 for a slot
    that does not count (sqr_pts_assign).  Two launches, no host wait."""
    out = pts_assign(points, params, count)
    return out["label"], out["dist"]


def recover_parts(points, parts, count=None, rounds=3, iters0=30, iters=10, lloyd=10, e0=1.0, lambda0=1e-3, up=10.0,
                  down=0.1, labels=None, normalize=False, return_info=False):
    """points [B,P,3] (count [B] or None: losses.pack_points; CUDA), parts = M bodies per cloud -> (params
    [B,M,12] f32, labels [B,P] i32, energy [B,M] f64), with return_info also a dict: dist [B,P] f32 (every slot's
    radial distance to its part), part_count [B,M] i32, part_dist [B,M] f64 (the sum of dist per part), changed
    [rounds,B] i32 (the points whose label moved in each round's assignment) and, when it seeded, seeds [B,M] i32
    and centres [B,M,3] f32.

    Several superquadrics per cloud by assign-and-refit (Leonardis, Jaklic, Solina): the cloud is split into M
    parts by farthest-point seeds and `lloyd` Lloyd iterations (or by `labels` [B,P] i32, a segmentation to
    polish; a label outside [0, M) belongs to no part); round 0 recovers every part as recover_points does (three
    starts, iters0 iterations, the lowest energy), every later round refines it by `iters` Levenberg-Marquardt
    iterations from where it is; after every round each point goes to the part whose surface is nearest
    (assign_points).  The labels returned are the last assignment's, so they belong to the parameters returned;
    energy is each part's LeastSquares energy at the end of the last fit, on the labels that fit used.  -1 labels
    the slots that do not count.  An empty part returns the default start with energy 0 and may win points back
    in a later round.  M is the caller's: nothing here chooses it, and parts that touch are not told apart.

    1 <= parts <= 16 and 3 B parts <= 65535; a part's launch walks its whole cloud, so the fit costs M times one
    cloud's.  The whole call (sqr_pts_recover_parts) is one chain of launches with no host wait: it can be
    captured in a HIP graph.  normalize=True as in recover_points: all M parts of a cloud share its scale and
    offset, energy and dist are those of the normalised cloud, and info also holds normalized_params, scale and
    offset."""
    _parts_shapes(points, parts, labels)
    scale = offset = None
    if normalize:
        points, scale, offset = normalize_points(points, count)
    out, lab, energy, info = pts_recover_parts(points, count, parts, labels, int(rounds), int(iters0), int(iters),
                                               int(lloyd), e0, lambda0, up, down)
    if normalize:
        info.update(normalized_params=out, scale=scale, offset=offset)
        out = denormalize_params(out.transpose(0, 1), scale, offset).transpose(0, 1).contiguous()
    return (out, lab, energy, info) if return_info else (out, lab, energy)
