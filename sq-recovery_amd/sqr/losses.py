"""Autograd wrappers of the fused HIP losses (libsqr: sqr_implicit_loss_fwd_bwd & co).

The kernels compute the loss AND its parameter gradient in one pass (the gradient is
d(batch-mean loss)/d params); the batch mean itself comes out of the same finalize launch, and
backward() only scales the gradient by the upstream gradient (one sqr_loss_grad_scale launch).
Reference: torch/classes.py:109-371 (timoblak/sq-recovery).
"""
import torch

from ._lib import check, lib, ptr, stream_ptr


def _require_cuda(*ts):
    for t in ts:
        if not t.is_cuda:
            raise ValueError("sqr GPU loss called with a CPU tensor (device %s)" % t.device)


def _workspace(nbytes, device):
    """The device bytes a call's *_workspace_bytes asks for (never an empty tensor: its pointer would be null)."""
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)


def _scale_grad(grad, gout, dtype):
    """grad * gout (gout: the scalar loss's upstream gradient, any float dtype) in one launch."""
    g = gout.to(torch.float64) if gout.dtype != torch.float64 else gout
    if not g.is_cuda or g.numel() != 1:
        return (grad * gout.to(torch.float32)).to(dtype)
    out = torch.empty_like(grad)
    check(lib().sqr_loss_grad_scale(ptr(grad), ptr(g), grad.numel(), ptr(out), stream_ptr(grad.device)),
          "sqr_loss_grad_scale")
    return out if dtype == torch.float32 else out.to(dtype)


def _image_target(target, params):
    """The [B,H,W] view of a [B,1,H,W] / [B,H,W] image target of [B,12] params, and B, H, W."""
    B = params.shape[0]
    if params.dim() != 2 or params.shape[1] != 12:
        raise ValueError("params must be [B,12], got %s" % (tuple(params.shape),))
    if target.dim() == 4:
        if target.shape[1] != 1:
            raise ValueError("target must be [B,1,H,W], got %s" % (tuple(target.shape),))
        tgt = target[:, 0]
    elif target.dim() == 3:
        tgt = target
    else:
        raise ValueError("target must be [B,1,H,W], got %s" % (tuple(target.shape),))
    if tgt.shape[0] != B:
        raise ValueError("batch mismatch: target %d vs params %d" % (tgt.shape[0], B))
    return tgt, B, int(tgt.shape[1]), int(tgt.shape[2])


class ImplicitLossFn(torch.autograd.Function):
    """loss = mean_b mean_rc |nearest(target)_b - render(params_b)|  (float64 scalar)."""

    @staticmethod
    def forward(ctx, target, params, R, tau, sharpness):
        _require_cuda(target, params)
        tgt, B, H, W = _image_target(target, params)
        p = params.detach().to(torch.float32).contiguous()
        t = tgt.detach().to(torch.float32).contiguous()
        need_grad = bool(ctx.needs_input_grad[1])
        loss_ps = torch.empty(B, dtype=torch.float64, device=p.device)
        loss = torch.empty((), dtype=torch.float64, device=p.device)  # the batch mean
        grad = torch.empty(B, 12, dtype=torch.float32, device=p.device) if need_grad else None
        L = lib()
        wsb = L.sqr_implicit_loss_workspace_bytes(B, R)
        ws = _workspace(wsb, p.device)
        check(L.sqr_implicit_loss_fwd_bwd_mean(ptr(p), ptr(t), B, H, W, int(R), float(tau), float(sharpness),
                                               int(need_grad), ptr(loss_ps), ptr(loss), ptr(grad), ptr(ws), wsb,
                                               stream_ptr(p.device)), "sqr_implicit_loss_fwd_bwd_mean")
        ctx.save_for_backward(grad)
        ctx.params_dtype = params.dtype
        ctx.per_sample = loss_ps
        return loss

    @staticmethod
    def backward(ctx, gout):
        (grad,) = ctx.saved_tensors
        if grad is None:
            return None, None, None, None, None
        return None, _scale_grad(grad, gout, ctx.params_dtype), None, None, None


class ExplicitLossFn(torch.autograd.Function):
    """loss = mean_b 100 * mean_vox (occ(true_b) - occ(pred_b))^2 (float64); grad to pred only."""

    @staticmethod
    def forward(ctx, p_true, p_pred, R):
        _require_cuda(p_true, p_pred)
        B = p_pred.shape[0]
        if p_pred.shape != (B, 12) or p_true.shape != (B, 12):
            raise ValueError("ExplicitLoss expects [B,12] params, got %s and %s"
                             % (tuple(p_true.shape), tuple(p_pred.shape)))
        pt = p_true.detach().to(torch.float32).contiguous()
        pp = p_pred.detach().to(torch.float32).contiguous()
        need_grad = bool(ctx.needs_input_grad[1])
        loss_ps = torch.empty(B, dtype=torch.float64, device=pp.device)
        loss = torch.empty((), dtype=torch.float64, device=pp.device)  # the batch mean
        grad = torch.empty(B, 12, dtype=torch.float32, device=pp.device) if need_grad else None
        L = lib()
        wsb = L.sqr_explicit_loss_workspace_bytes(B, R)
        ws = _workspace(wsb, pp.device)
        check(L.sqr_explicit_loss_fwd_bwd_mean(ptr(pt), ptr(pp), B, int(R), int(need_grad), ptr(loss_ps), ptr(loss),
                                               ptr(grad), ptr(ws), wsb, stream_ptr(pp.device)),
              "sqr_explicit_loss_fwd_bwd_mean")
        ctx.save_for_backward(grad)
        ctx.params_dtype = p_pred.dtype
        return loss

    @staticmethod
    def backward(ctx, gout):
        (grad,) = ctx.saved_tensors
        if grad is None:
            return None, None, None
        return None, _scale_grad(grad, gout, ctx.params_dtype), None


class LeastSquaresFn(torch.autograd.Function):
    """E_b = a0 a1 a2 sum_points (F_b(point) - 1)^2 over the pixels > 0 of the nearest-resized target
    (classes.py:297-371); returns mean_b E_b (float64 scalar) or, per_sample, the [B] energies."""

    @staticmethod
    def forward(ctx, target, params, R, per_sample):
        _require_cuda(target, params)
        tgt, B, H, W = _image_target(target, params)
        p = params.detach().to(torch.float32).contiguous()
        t = tgt.detach().to(torch.float32).contiguous()
        need_grad = bool(ctx.needs_input_grad[1])
        loss_ps = torch.empty(B, dtype=torch.float64, device=p.device)
        loss = torch.empty((), dtype=torch.float64, device=p.device)  # the batch mean
        grad = torch.empty(B, 12, dtype=torch.float32, device=p.device) if need_grad else None
        L = lib()
        wsb = L.sqr_least_squares_workspace_bytes(B, R)
        ws = _workspace(wsb, p.device)
        check(L.sqr_least_squares_fwd_bwd_mean(ptr(p), ptr(t), B, H, W, int(R), int(need_grad), ptr(loss_ps),
                                               ptr(loss), ptr(grad), ptr(ws), wsb, stream_ptr(p.device)),
              "sqr_least_squares_fwd_bwd_mean")
        ctx.save_for_backward(grad)
        ctx.params_dtype = params.dtype
        ctx.is_per_sample = per_sample
        return loss_ps if per_sample else loss

    @staticmethod
    def backward(ctx, gout):
        (grad,) = ctx.saved_tensors
        if grad is None:
            return None, None, None, None
        if ctx.is_per_sample:
            # the stored rows are d(mean_b E_b)/d params_b = (1/B) dE_b/d params_b
            scale = (gout.to(torch.float32) * float(grad.shape[0])).unsqueeze(1)
            return None, (grad * scale).to(ctx.params_dtype), None, None
        return None, _scale_grad(grad, gout, ctx.params_dtype), None, None


def implicit_loss(target, params, R, tau=1.0, sharpness=100.0):
    return ImplicitLossFn.apply(target, params, int(R), float(tau), float(sharpness))


def explicit_loss(p_true, p_pred, R):
    return ExplicitLossFn.apply(p_true, p_pred, int(R))


def least_squares(target, params, R, per_sample=False):
    """LeastSquares(R)(target, params) as a float64 scalar; per_sample=True: the [B] energies E_b (both
    differentiable w.r.t. params; no host synchronisation, so the call can be captured in a HIP graph)."""
    return LeastSquaresFn.apply(target, params, int(R), bool(per_sample))


def least_squares_normal_eq(target, params, R):
    """Normal equations of the LeastSquares residuals r_k = sqrt(a0 a1 a2) (F(point_k) - 1) per sample:
    (H [B,12,12] = sum J_k^T J_k, g [B,12] = sum J_k r_k, E [B] = sum r_k^2), all float64, no autograd
    (sqr_least_squares_normal_eq).  target [B,1,H,W] or [B,H,W], params [B,12], CUDA."""
    _require_cuda(target, params)
    tgt, B, H, W = _image_target(target, params)
    p = params.detach().to(torch.float32).contiguous()
    t = tgt.detach().to(torch.float32).contiguous()
    JtJ = torch.empty(B, 12, 12, dtype=torch.float64, device=p.device)
    Jtr = torch.empty(B, 12, dtype=torch.float64, device=p.device)
    E = torch.empty(B, dtype=torch.float64, device=p.device)
    L = lib()
    wsb = L.sqr_least_squares_normal_eq_workspace_bytes(B, int(R))
    ws = _workspace(wsb, p.device)
    check(L.sqr_least_squares_normal_eq(ptr(p), ptr(t), B, H, W, int(R), ptr(JtJ), ptr(Jtr), ptr(E), ptr(ws), wsb,
                                        stream_ptr(p.device)), "sqr_least_squares_normal_eq")
    return JtJ, Jtr, E


def _lm_refine(t, p, R, iters, lambda0, up, down):
    """sqr_lsq_lm_refine_multi on checked tensors: t [B,H,W] and p [K,B,12], contiguous float32 on one device."""
    (K, B, _), (H, W), dev = p.shape, t.shape[1:], p.device
    out = torch.empty(K, B, 12, dtype=torch.float32, device=dev)
    before = torch.empty(K, B, dtype=torch.float64, device=dev)
    after = torch.empty(K, B, dtype=torch.float64, device=dev)
    accepted = torch.empty(K, B, dtype=torch.int32, device=dev)
    L = lib()
    wsb = L.sqr_lsq_lm_refine_workspace_bytes(K * B, int(R))
    ws = _workspace(wsb, dev)
    check(L.sqr_lsq_lm_refine_multi(ptr(p), ptr(t), K, B, H, W, int(R), int(iters), float(lambda0), float(up),
                                    float(down), ptr(out), ptr(before), ptr(after), ptr(accepted), ptr(ws), wsb,
                                    stream_ptr(dev)), "sqr_lsq_lm_refine_multi")
    return out, before, after, accepted


def lm_refine(target, params, R, iters, lambda0, up, down):
    """sqr_lsq_lm_refine_multi with K = 1 (what the C entry sqr_lsq_lm_refine is too; an error names the multi
    entry) -> (params [B,12] f32, energy_before [B] f64, energy_after [B] f64, accepted [B] i32).  One chain of
    launches on the current stream; no host wait."""
    _require_cuda(target, params)
    tgt, B, H, W = _image_target(target, params)
    p = params.detach().to(torch.float32).contiguous()
    t = tgt.detach().to(torch.float32).contiguous()
    return tuple(x[0] for x in _lm_refine(t, p[None], R, iters, lambda0, up, down))


def _image_only(target):
    """The contiguous float32 [B,H,W] view of a [B,1,H,W] / [B,H,W] CUDA image batch, and B, H, W."""
    _require_cuda(target)
    if target.dim() == 4 and target.shape[1] == 1:
        tgt = target[:, 0]
    elif target.dim() == 3:
        tgt = target
    else:
        raise ValueError("target must be [B,1,H,W] or [B,H,W], got %s" % (tuple(target.shape),))
    if tgt.shape[0] < 1:
        raise ValueError("target holds no image")
    t = tgt.detach().to(torch.float32).contiguous()
    return t, int(t.shape[0]), int(t.shape[1]), int(t.shape[2])


def _moments_info(B, dev):
    """The empty outputs of the starts' moments: count [B] i32, centroid [B,3], eigenvalues [B,3], frame [B,3,3]."""
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)  # noqa: E731
    return {"count": torch.empty(B, dtype=torch.int32, device=dev), "centroid": f64(B, 3), "eigenvalues": f64(B, 3),
            "frame": f64(B, 3, 3)}


def _starts(target, R, e0, depth):
    """sqr_lsq_starts (depth None: three starts) or sqr_lsq_starts6 (six) -> (starts [3 or 6,B,12] f32, info)."""
    t, B, H, W = _image_only(target)
    dev = t.device
    starts = torch.empty(3 if depth is None else 6, B, 12, dtype=torch.float32, device=dev)
    info = _moments_info(B, dev)
    L = lib()
    wsb = L.sqr_lsq_starts_workspace_bytes(B, int(R))
    ws = _workspace(wsb, dev)
    outs = (ptr(starts), ptr(info["count"]), ptr(info["centroid"]), ptr(info["eigenvalues"]), ptr(info["frame"]),
            ptr(ws), wsb, stream_ptr(dev))
    if depth is None:
        check(L.sqr_lsq_starts(ptr(t), B, H, W, int(R), float(e0), *outs), "sqr_lsq_starts")
    else:
        check(L.sqr_lsq_starts6(ptr(t), B, H, W, int(R), float(e0), float(depth), *outs), "sqr_lsq_starts6")
    return starts, info


def lsq_starts(target, R, e0=1.0):
    """sqr_lsq_starts -> (starts [3,B,12] f32, info): Solina & Bajcsy's three starts of the recovery from the
    points of each image alone.  info: count [B] i32, centroid [B,3], eigenvalues [B,3] (of the points'
    covariance, ascending) and frame [B,3,3] (the eigenvectors its columns, det +1), float64.  Start k has the
    columns (k, k+1, k+2 mod 3) of the frame as its axes, half the points' extents along them as its sizes and
    e = (e0, e0).  Four launches on the current stream; no host wait."""
    return _starts(target, R, e0, None)


def lsq_select(params, energy):
    """sqr_lsq_select: params [K,B,12], energy [K,B] (CUDA) -> (params [B,12] f32, energy [B] f64, index [B]
    i32) of the lowest energy per sample; the lowest index on a tie, NaN never wins, all NaN gives index 0."""
    _require_cuda(params, energy)
    if params.dim() != 3 or params.shape[2] != 12 or energy.dim() != 2 or tuple(energy.shape) != tuple(params.shape[:2]):
        raise ValueError("params must be [K,B,12] and energy [K,B], got %s and %s"
                         % (tuple(params.shape), tuple(energy.shape)))
    K, B = int(params.shape[0]), int(params.shape[1])
    p = params.detach().to(torch.float32).contiguous()
    e = energy.detach().to(torch.float64).contiguous()
    out = torch.empty(B, 12, dtype=torch.float32, device=p.device)
    oe = torch.empty(B, dtype=torch.float64, device=p.device)
    oi = torch.empty(B, dtype=torch.int32, device=p.device)
    check(lib().sqr_lsq_select(B, K, ptr(p), ptr(e), ptr(out), ptr(oe), ptr(oi), stream_ptr(p.device)),
          "sqr_lsq_select")
    return out, oe, oi


def lsq_recover(target, R, iters, e0, lambda0, up, down):
    """sqr_lsq_recover -> (params [B,12] f32, energy [B] f64, index [B] i32, all_params [3,B,12] f32,
    all_before [3,B] f64, all_after [3,B] f64, all_accepted [3,B] i32).  One chain of launches on the current
    stream; no host wait."""
    t, B, H, W = _image_only(target)
    dev = t.device
    out = torch.empty(B, 12, dtype=torch.float32, device=dev)
    energy = torch.empty(B, dtype=torch.float64, device=dev)
    index = torch.empty(B, dtype=torch.int32, device=dev)
    allp = torch.empty(3, B, 12, dtype=torch.float32, device=dev)
    before = torch.empty(3, B, dtype=torch.float64, device=dev)
    after = torch.empty(3, B, dtype=torch.float64, device=dev)
    accepted = torch.empty(3, B, dtype=torch.int32, device=dev)
    L = lib()
    wsb = L.sqr_lsq_recover_workspace_bytes(B, int(R))
    ws = _workspace(wsb, dev)
    check(L.sqr_lsq_recover(ptr(t), B, H, W, int(R), int(iters), float(e0), float(lambda0), float(up), float(down),
                            ptr(out), ptr(energy), ptr(index), ptr(allp), ptr(before), ptr(after), ptr(accepted),
                            ptr(ws), wsb, stream_ptr(dev)), "sqr_lsq_recover")
    return out, energy, index, allp, before, after, accepted


def _stacked_params(params, B, what):
    """[K,B,12] (or [B,12] = one slice) CUDA parameters as contiguous float32 [K,B,12]."""
    _require_cuda(params)
    p = params.detach().to(torch.float32)
    if p.dim() == 2:
        p = p[None]
    if p.dim() != 3 or p.shape[0] < 1 or p.shape[1] != B or p.shape[2] != 12:
        raise ValueError("%s must be [K,%d,12] or [%d,12], got %s" % (what, B, B, tuple(params.shape)))
    return p.contiguous()


def free_space_energy(images, params, render_size, margin=1.0 / 255.0):
    """sqr_lsq_free_space -> E_fs [S] f64 (no autograd): images [B,1,H,W] or [B,H,W], params [S,12] with S a
    multiple of B, sample s against image s mod B (a [K,B,12] stack flattened).  Along every resized pixel's ray
    the model must stay out of the space the image shows to be empty: in front of the visible surface (from
    z + margin on; one grey level by default, a quantised pixel lies up to one level below the true surface)
    and, on a background pixel, everywhere from z = 0 on.  E_fs = a0 a1 a2 sum_pixels min(min_z F - 1, 0)^2.
    Bitwise reproducible, a sample's value independent of the batch; two launches, no host wait."""
    t, B, H, W = _image_only(images)
    _require_cuda(params)
    if params.dim() != 2 or params.shape[1] != 12 or params.shape[0] < B or params.shape[0] % B:
        raise ValueError("params must be [S,12] with S a multiple of the %d images, got %s" % (B, tuple(params.shape)))
    p = params.detach().to(torch.float32).contiguous()
    S = int(p.shape[0])
    out = torch.empty(S, dtype=torch.float64, device=p.device)
    L = lib()
    wsb = L.sqr_lsq_free_space_workspace_bytes(S, int(render_size))
    ws = _workspace(wsb, p.device)
    check(L.sqr_lsq_free_space(ptr(p), ptr(t), S, B, H, W, int(render_size), float(margin), ptr(out), ptr(ws), wsb,
                               stream_ptr(p.device)), "sqr_lsq_free_space")
    return out


def lm_refine_multi(target, params, R, iters, lambda0, up, down):
    """sqr_lsq_lm_refine_multi: params [K,B,12], target [B,1,H,W] or [B,H,W] -> (params [K,B,12] f32,
    energy_before [K,B] f64, energy_after [K,B] f64, accepted [K,B] i32), bitwise what K lm_refine calls on the
    slices return.  One chain of launches over the K B samples on the current stream; no host wait."""
    t, B, _, _ = _image_only(target)
    return _lm_refine(t, _stacked_params(params, B, "params"), R, iters, lambda0, up, down)


def lsq_starts6(target, R, e0=1.0, depth=1.0):
    """sqr_lsq_starts6 -> (starts [6,B,12] f32, info as lsq_starts): lsq_starts' three starts, bitwise, and
    three more whose extent along the frame axis nearest the viewing direction is stretched by depth times
    itself away from the viewer (a depth image shows the front half only).  depth = 0 repeats starts 0..2."""
    return _starts(target, R, e0, depth)


def lsq_recover_multi(target, R, iters, nstarts, e0, depth, extra, lambda0, up, down, w_fs, margin):
    """sqr_lsq_recover_multi -> (params [B,12] f32, energy [B] f64, energy_fs [B] f64, index [B] i32, info dict:
    starts, params [K,B,12] f32, energy_before, energy_after, energy_fs, score [K,B] f64, accepted [K,B] i32),
    K = nstarts (3 or 6) + the extra starts ([Kx,B,12] or [B,12] or None).  One chain of launches on the current
    stream; no host wait."""
    t, B, H, W = _image_only(target)
    dev = t.device
    x = _stacked_params(extra, B, "extra_starts") if extra is not None else None
    Kx = int(x.shape[0]) if x is not None else 0
    K = int(nstarts) + Kx
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)  # noqa: E731
    out = torch.empty(B, 12, dtype=torch.float32, device=dev)
    energy, fs = f64(B), f64(B)
    index = torch.empty(B, dtype=torch.int32, device=dev)
    info = {"starts": torch.empty(K, B, 12, dtype=torch.float32, device=dev),
            "params": torch.empty(K, B, 12, dtype=torch.float32, device=dev),
            "energy_before": f64(K, B), "energy_after": f64(K, B), "energy_fs": f64(K, B), "score": f64(K, B),
            "accepted": torch.empty(K, B, dtype=torch.int32, device=dev)}
    L = lib()
    wsb = L.sqr_lsq_recover_multi_workspace_bytes(K, B, int(R))
    ws = _workspace(wsb, dev)
    check(L.sqr_lsq_recover_multi(ptr(t), B, H, W, int(R), int(iters), int(nstarts), float(e0), float(depth), ptr(x),
                                  Kx, float(lambda0), float(up), float(down), float(w_fs), float(margin), ptr(out),
                                  ptr(energy), ptr(fs), ptr(index), ptr(info["starts"]), ptr(info["params"]),
                                  ptr(info["energy_before"]), ptr(info["energy_after"]), ptr(info["energy_fs"]),
                                  ptr(info["score"]), ptr(info["accepted"]), ptr(ws), wsb, stream_ptr(dev)),
          "sqr_lsq_recover_multi")
    return out, energy, fs, index, info


# ---------------------------------------------------------------------------- point lists (sqr_pts_*)
def pack_points(clouds, device=None):
    """A list of [N_i,3] clouds (tensors or arrays), or one [B,P,3] batch -> (points [B,P,3] f32 on `device`,
    count [B] i32): the layout of the sqr_pts_* calls.  P = the longest cloud (at least 1); the slots behind a
    cloud's own points are NaN, which never counts.  The lengths come from the shapes, so nothing waits for the
    device.  A [B,P,3] batch is passed through (float32, contiguous) with count = P for every cloud."""
    if isinstance(clouds, torch.Tensor) or hasattr(clouds, "ndim"):
        t = torch.as_tensor(clouds)
        if t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError("points must be [B,P,3] with B,P >= 1, got %s" % (tuple(t.shape),))
        dev = t.device if device is None else torch.device(device)
        pts = t.detach().to(device=dev, dtype=torch.float32).contiguous()
        return pts, torch.full((pts.shape[0],), pts.shape[1], dtype=torch.int32, device=dev)
    cl = [torch.as_tensor(c) for c in clouds]
    if not cl:
        raise ValueError("pack_points: no cloud")
    for c in cl:
        if c.dim() != 2 or c.shape[1] != 3:
            raise ValueError("every cloud must be [N,3], got %s" % (tuple(c.shape),))
    dev = cl[0].device if device is None else torch.device(device)
    lens = [int(c.shape[0]) for c in cl]
    pts = torch.full((len(cl), max(max(lens), 1), 3), float("nan"), dtype=torch.float32, device=dev)
    for i, c in enumerate(cl):
        if lens[i]:
            pts[i, :lens[i]] = c.detach().to(device=dev, dtype=torch.float32)
    return pts, torch.tensor(lens, dtype=torch.int32).to(dev)


def _point_list(points, count):
    """Checked (points [B,P,3] f32 contiguous, count [B] i32 contiguous or None, B, P) of a CUDA point list."""
    _require_cuda(points)
    if points.dim() != 3 or points.shape[2] != 3 or points.shape[0] < 1 or points.shape[1] < 1:
        raise ValueError("points must be [B,P,3] with B,P >= 1, got %s" % (tuple(points.shape),))
    pts = points.detach().to(torch.float32).contiguous()
    B, P = int(pts.shape[0]), int(pts.shape[1])
    cnt = None
    if count is not None:
        _require_cuda(count)
        if count.dim() != 1 or count.shape[0] != B or count.dtype.is_floating_point:
            raise ValueError("count must be [%d] integers, got %s %s" % (B, tuple(count.shape), count.dtype))
        if count.device != pts.device:
            raise ValueError("points and count are on different devices")
        cnt = count.detach().to(torch.int32).contiguous()
    return pts, cnt, B, P


def _list_params(params, B, pts):
    """[S,12] CUDA parameters, S a multiple of the B clouds, as contiguous float32 on the clouds' device."""
    _require_cuda(params)
    if params.dim() != 2 or params.shape[1] != 12 or params.shape[0] < B or params.shape[0] % B:
        raise ValueError("params must be [S,12] with S a multiple of the %d clouds, got %s" % (B, tuple(params.shape)))
    if params.device != pts.device:
        raise ValueError("points and params are on different devices")
    return params.detach().to(torch.float32).contiguous()


def point_normal_eq(points, params, count=None):
    """sqr_pts_normal_eq -> (H [S,12,12], g [S,12], E [S]) float64, no autograd: least_squares_normal_eq on the
    point list points [B,P,3] (count [B] or None: see pack_points) instead of an image's points.  params [S,12],
    S a multiple of B, sample s on cloud s mod B.  Two launches, no host wait."""
    pts, cnt, B, P = _point_list(points, count)
    p = _list_params(params, B, pts)
    S, dev = int(p.shape[0]), p.device
    JtJ = torch.empty(S, 12, 12, dtype=torch.float64, device=dev)
    Jtr = torch.empty(S, 12, dtype=torch.float64, device=dev)
    E = torch.empty(S, dtype=torch.float64, device=dev)
    L = lib()
    wsb = L.sqr_pts_normal_eq_workspace_bytes(S, P)
    ws = _workspace(wsb, dev)
    check(L.sqr_pts_normal_eq(ptr(p), ptr(pts), ptr(cnt), S, B, P, ptr(JtJ), ptr(Jtr), ptr(E), ptr(ws), wsb,
                              stream_ptr(dev)), "sqr_pts_normal_eq")
    return JtJ, Jtr, E


class PointEnergyFn(torch.autograd.Function):
    """E_s = a0 a1 a2 sum_points (F_s(point) - 1)^2 over a point list: the normal equations' energy, and
    dE_s / d params_s = 2 Jtr_s from the same evaluation (no second kernel)."""

    @staticmethod
    def forward(ctx, points, params, count, per_sample):
        _, Jtr, E = point_normal_eq(points, params, count)
        ctx.save_for_backward(Jtr)
        ctx.params_dtype = params.dtype
        ctx.is_per_sample = per_sample
        return E if per_sample else E.mean()

    @staticmethod
    def backward(ctx, gout):
        (Jtr,) = ctx.saved_tensors
        g = gout.to(torch.float64)
        g = g.unsqueeze(1) if ctx.is_per_sample else g / Jtr.shape[0]
        return None, (2.0 * Jtr * g).to(torch.float32).to(ctx.params_dtype), None, None


def point_energy(points, params, count=None, per_sample=False):
    """The LeastSquares energy of params [S,12] on the point list points [B,P,3] (count [B] or None), sample s on
    cloud s mod B: the batch mean as a float64 scalar or, per_sample, the [S] energies; bitwise
    point_normal_eq's E.  Differentiable w.r.t. params: the gradient is 2 Jtr in float64, times the upstream
    gradient, rounded to float32 once.  No host wait."""
    return PointEnergyFn.apply(points, params, count, bool(per_sample))


def pts_lm_refine(points, count, params, iters, lambda0, up, down):
    """sqr_pts_lm_refine: params [K,B,12] (or [B,12] = one slice) -> (params [K,B,12] f32, energy_before [K,B]
    f64, energy_after [K,B] f64, accepted [K,B] i32).  One chain of launches on the current stream; no host wait."""
    pts, cnt, B, P = _point_list(points, count)
    p = _stacked_params(params, B, "params")
    K, dev = int(p.shape[0]), pts.device
    out = torch.empty(K, B, 12, dtype=torch.float32, device=dev)
    before = torch.empty(K, B, dtype=torch.float64, device=dev)
    after = torch.empty(K, B, dtype=torch.float64, device=dev)
    accepted = torch.empty(K, B, dtype=torch.int32, device=dev)
    L = lib()
    wsb = L.sqr_pts_lm_refine_workspace_bytes(K * B, P)
    ws = _workspace(wsb, dev)
    check(L.sqr_pts_lm_refine(ptr(p), ptr(pts), ptr(cnt), K, B, P, int(iters), float(lambda0), float(up), float(down),
                              ptr(out), ptr(before), ptr(after), ptr(accepted), ptr(ws), wsb, stream_ptr(dev)),
          "sqr_pts_lm_refine")
    return out, before, after, accepted


def pts_starts(points, count=None, e0=1.0):
    """sqr_pts_starts -> (starts [3,B,12] f32, info as lsq_starts; info["count"] = the slots that count)."""
    pts, cnt, B, P = _point_list(points, count)
    dev = pts.device
    starts = torch.empty(3, B, 12, dtype=torch.float32, device=dev)
    info = _moments_info(B, dev)
    L = lib()
    wsb = L.sqr_pts_starts_workspace_bytes(B, P)
    ws = _workspace(wsb, dev)
    check(L.sqr_pts_starts(ptr(pts), ptr(cnt), B, P, float(e0), ptr(starts), ptr(info["count"]),
                           ptr(info["centroid"]), ptr(info["eigenvalues"]), ptr(info["frame"]), ptr(ws), wsb,
                           stream_ptr(dev)), "sqr_pts_starts")
    return starts, info


def pts_recover(points, count, iters, e0, extra, lambda0, up, down):
    """sqr_pts_recover -> (params [B,12] f32, energy [B] f64, index [B] i32, info dict: starts, params [K,B,12]
    f32, energy_before, energy_after [K,B] f64, accepted [K,B] i32), K = 3 + the extra starts ([Kx,B,12] or
    [B,12] or None).  One chain of launches on the current stream; no host wait."""
    pts, cnt, B, P = _point_list(points, count)
    dev = pts.device
    x = _stacked_params(extra, B, "extra_starts") if extra is not None else None
    Kx = int(x.shape[0]) if x is not None else 0
    K = 3 + Kx
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)  # noqa: E731
    out = torch.empty(B, 12, dtype=torch.float32, device=dev)
    energy = f64(B)
    index = torch.empty(B, dtype=torch.int32, device=dev)
    info = {"starts": torch.empty(K, B, 12, dtype=torch.float32, device=dev),
            "params": torch.empty(K, B, 12, dtype=torch.float32, device=dev),
            "energy_before": f64(K, B), "energy_after": f64(K, B),
            "accepted": torch.empty(K, B, dtype=torch.int32, device=dev)}
    L = lib()
    wsb = L.sqr_pts_recover_workspace_bytes(K, B, P)
    ws = _workspace(wsb, dev)
    check(L.sqr_pts_recover(ptr(pts), ptr(cnt), B, P, int(iters), float(e0), ptr(x), Kx, float(lambda0), float(up),
                            float(down), ptr(out), ptr(energy), ptr(index), ptr(info["starts"]), ptr(info["params"]),
                            ptr(info["energy_before"]), ptr(info["energy_after"]), ptr(info["accepted"]), ptr(ws),
                            wsb, stream_ptr(dev)), "sqr_pts_recover")
    return out, energy, index, info


MAX_PARTS = 16


def _parts(B, M):
    """The checked number of parts per cloud: 1 <= M <= 16 and 3 B M <= 65535 (one recovery chain)."""
    M = int(M)
    if not 1 <= M <= MAX_PARTS:
        raise ValueError("parts must be in [1,%d], got %d" % (MAX_PARTS, M))
    if 3 * B * M > 65535:
        raise ValueError("3 x %d clouds x %d parts = %d samples in one chain, more than 65535" % (B, M, 3 * B * M))
    return M


def _parts_shapes(points, parts, labels=None, what="labels"):
    """What the several-parts calls check on shapes and dtypes alone, before anything asks for a device: points
    [B,P,3], the number of parts, labels (optional) an int32 tensor [B,P].  -> M."""
    if points.dim() != 3 or points.shape[2] != 3 or points.shape[0] < 1 or points.shape[1] < 1:
        raise ValueError("points must be [B,P,3] with B,P >= 1, got %s" % (tuple(points.shape),))
    B, P = int(points.shape[0]), int(points.shape[1])
    M = _parts(B, parts)
    if labels is not None and (not isinstance(labels, torch.Tensor) or labels.dtype != torch.int32 or
                               tuple(labels.shape) != (B, P)):
        raise ValueError("%s must be an int32 tensor [%d,%d], got %s %s" % (
            what, B, P, tuple(getattr(labels, "shape", ())), getattr(labels, "dtype", type(labels))))
    return M


def _labels(labels, pts, what="labels"):
    """[B,P] int32 CUDA labels of the point list pts, contiguous."""
    _parts_shapes(pts, 1, labels, what)
    _require_cuda(labels)
    if labels.device != pts.device:
        raise ValueError("points and %s are on different devices" % what)
    return labels.detach().contiguous()


def _part_params(params, B, pts, what="params"):
    """[B,M,12] CUDA parameters as contiguous float32, and M."""
    _require_cuda(params)
    if params.dim() != 3 or params.shape[0] != B or params.shape[2] != 12:
        raise ValueError("%s must be [%d,M,12], got %s" % (what, B, tuple(params.shape)))
    if params.device != pts.device:
        raise ValueError("points and %s are on different devices" % what)
    return params.detach().to(torch.float32).contiguous(), _parts(B, params.shape[1])


def pts_seed(points, parts, count=None, lloyd=10):
    """sqr_pts_seed -> (labels [B,P] i32, centres [B,M,3] f32, seeds [B,M] i32): farthest-point seeds and `lloyd`
    Lloyd iterations.  One chain of launches on the current stream; no host wait."""
    M = _parts_shapes(points, parts)
    pts, cnt, B, P = _point_list(points, count)
    dev = pts.device
    if int(lloyd) < 0:
        raise ValueError("lloyd must be >= 0, got %d" % lloyd)
    label = torch.empty(B, P, dtype=torch.int32, device=dev)
    centres = torch.empty(B, M, 3, dtype=torch.float32, device=dev)
    seeds = torch.empty(B, M, dtype=torch.int32, device=dev)
    L = lib()
    wsb = L.sqr_pts_seed_workspace_bytes(B, P, M)
    ws = _workspace(wsb, dev)
    check(L.sqr_pts_seed(ptr(pts), ptr(cnt), B, P, M, int(lloyd), ptr(label), ptr(centres), ptr(seeds), ptr(ws), wsb,
                         stream_ptr(dev)), "sqr_pts_seed")
    return label, centres, seeds


def pts_assign(points, params, count=None, labels_prev=None):
    """sqr_pts_assign: params [B,M,12] -> dict: label [B,P] i32, dist [B,P] f32, part_count [B,M] i32, part_dist
    [B,M] f64 and, with labels_prev [B,P] i32, changed [B] i32.  Two launches; no host wait."""
    pts, cnt, B, P = _point_list(points, count)
    p, M = _part_params(params, B, pts)
    dev = pts.device
    prev = _labels(labels_prev, pts, "labels_prev") if labels_prev is not None else None
    out = {"label": torch.empty(B, P, dtype=torch.int32, device=dev),
           "dist": torch.empty(B, P, dtype=torch.float32, device=dev),
           "part_count": torch.empty(B, M, dtype=torch.int32, device=dev),
           "part_dist": torch.empty(B, M, dtype=torch.float64, device=dev)}
    if prev is not None:
        out["changed"] = torch.empty(B, dtype=torch.int32, device=dev)
    L = lib()
    wsb = L.sqr_pts_assign_workspace_bytes(B, P, M)
    ws = _workspace(wsb, dev)
    check(L.sqr_pts_assign(ptr(pts), ptr(cnt), ptr(p), ptr(prev), B, P, M, ptr(out["label"]), ptr(out["dist"]),
                           ptr(out["part_count"]), ptr(out["part_dist"]), ptr(out.get("changed")), ptr(ws), wsb,
                           stream_ptr(dev)), "sqr_pts_assign")
    return out


def pts_labeled_lm_refine(points, count, labels, params, iters, lambda0, up, down):
    """sqr_pts_labeled_lm_refine: params [K,B,M,12] (or [B,M,12] = one slice) -> (params [K,B,M,12] f32,
    energy_before [K,B,M] f64, energy_after [K,B,M] f64, accepted [K,B,M] i32): pts_lm_refine on the parts of the
    labelled lists."""
    pts, cnt, B, P = _point_list(points, count)
    lab = _labels(labels, pts)
    _require_cuda(params)
    p = params.detach().to(torch.float32)
    if p.dim() == 3:
        p = p[None]
    if p.dim() != 4 or p.shape[0] < 1 or p.shape[1] != B or p.shape[3] != 12:
        raise ValueError("params must be [K,%d,M,12] or [%d,M,12], got %s" % (B, B, tuple(params.shape)))
    p = p.contiguous()
    K, M, dev = int(p.shape[0]), _parts(B, p.shape[2]), pts.device
    out = torch.empty(K, B, M, 12, dtype=torch.float32, device=dev)
    before = torch.empty(K, B, M, dtype=torch.float64, device=dev)
    after = torch.empty(K, B, M, dtype=torch.float64, device=dev)
    accepted = torch.empty(K, B, M, dtype=torch.int32, device=dev)
    L = lib()
    wsb = L.sqr_pts_labeled_lm_refine_workspace_bytes(K * B * M, P)
    ws = _workspace(wsb, dev)
    check(L.sqr_pts_labeled_lm_refine(ptr(p), ptr(pts), ptr(cnt), ptr(lab), K, B, P, M, int(iters), float(lambda0),
                                      float(up), float(down), ptr(out), ptr(before), ptr(after), ptr(accepted),
                                      ptr(ws), wsb, stream_ptr(dev)), "sqr_pts_labeled_lm_refine")
    return out, before, after, accepted


def pts_labeled_recover(points, count, labels, parts, iters, e0, lambda0, up, down):
    """sqr_pts_labeled_recover -> (params [B,M,12] f32, energy [B,M] f64, index [B,M] i32, info dict: starts, params
    [3,B,M,12] f32, energy_before, energy_after [3,B,M] f64, accepted [3,B,M] i32): pts_recover on the parts of the
    labelled lists."""
    M = _parts_shapes(points, parts, labels)
    pts, cnt, B, P = _point_list(points, count)
    lab = _labels(labels, pts)
    dev, K = pts.device, 3
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)  # noqa: E731
    out = torch.empty(B, M, 12, dtype=torch.float32, device=dev)
    energy = f64(B, M)
    index = torch.empty(B, M, dtype=torch.int32, device=dev)
    info = {"starts": torch.empty(K, B, M, 12, dtype=torch.float32, device=dev),
            "params": torch.empty(K, B, M, 12, dtype=torch.float32, device=dev),
            "energy_before": f64(K, B, M), "energy_after": f64(K, B, M),
            "accepted": torch.empty(K, B, M, dtype=torch.int32, device=dev)}
    L = lib()
    wsb = L.sqr_pts_labeled_recover_workspace_bytes(K, B * M, P)
    ws = _workspace(wsb, dev)
    check(L.sqr_pts_labeled_recover(ptr(pts), ptr(cnt), ptr(lab), B, P, M, int(iters), float(e0), ptr(None), 0,
                                    float(lambda0), float(up), float(down), ptr(out), ptr(energy), ptr(index),
                                    ptr(info["starts"]), ptr(info["params"]), ptr(info["energy_before"]),
                                    ptr(info["energy_after"]), ptr(info["accepted"]), ptr(ws), wsb, stream_ptr(dev)),
          "sqr_pts_labeled_recover")
    return out, energy, index, info


def pts_recover_parts(points, count, parts, labels, rounds, iters0, iters, lloyd, e0, lambda0, up, down):
    """sqr_pts_recover_parts -> (params [B,M,12] f32, labels [B,P] i32, energy [B,M] f64, info dict: dist [B,P]
    f32, part_count [B,M] i32, part_dist [B,M] f64, changed [rounds,B] i32 and, when labels is None (it seeded),
    seeds [B,M] i32 and centres [B,M,3] f32).  One chain of launches on the current stream; no host wait."""
    M, T = _parts_shapes(points, parts, labels), int(rounds)
    if not 1 <= T <= 1024:
        raise ValueError("rounds must be in [1,1024], got %d" % T)
    pts, cnt, B, P = _point_list(points, count)
    lab_in = _labels(labels, pts) if labels is not None else None
    dev = pts.device
    out = torch.empty(B, M, 12, dtype=torch.float32, device=dev)
    label = torch.empty(B, P, dtype=torch.int32, device=dev)
    energy = torch.empty(B, M, dtype=torch.float64, device=dev)
    info = {"dist": torch.empty(B, P, dtype=torch.float32, device=dev),
            "part_count": torch.empty(B, M, dtype=torch.int32, device=dev),
            "part_dist": torch.empty(B, M, dtype=torch.float64, device=dev),
            "changed": torch.empty(T, B, dtype=torch.int32, device=dev)}
    if lab_in is None:
        info["seeds"] = torch.empty(B, M, dtype=torch.int32, device=dev)
        info["centres"] = torch.empty(B, M, 3, dtype=torch.float32, device=dev)
    L = lib()
    wsb = L.sqr_pts_recover_parts_workspace_bytes(B, P, M)
    ws = _workspace(wsb, dev)
    check(L.sqr_pts_recover_parts(ptr(pts), ptr(cnt), ptr(lab_in), B, P, M, T, int(iters0), int(iters), int(lloyd),
                                  float(e0), float(lambda0), float(up), float(down), ptr(out), ptr(label), ptr(energy),
                                  ptr(info["dist"]), ptr(info["part_count"]), ptr(info["part_dist"]),
                                  ptr(info["changed"]), ptr(info.get("seeds")), ptr(info.get("centres")), ptr(ws), wsb,
                                  stream_ptr(dev)), "sqr_pts_recover_parts")
    return out, label, energy, info


def implicit_render(params, R, tau=1.0, sharpness=100.0):
    """depth_projection (classes.py:232-282) -> [B,R,R] float32 images (no autograd)."""
    _require_cuda(params)
    p = params.detach().to(torch.float32).contiguous()
    out = torch.empty(p.shape[0], R, R, dtype=torch.float32, device=p.device)
    check(lib().sqr_implicit_render(ptr(p), p.shape[0], int(R), float(tau), float(sharpness), ptr(out),
                                    stream_ptr(p.device)), "sqr_implicit_render")
    return out


def scan_render(params, size=256, levels=255):
    """Scanner-style hard depth images [B,size,size] float32 in [0, 1] (sqr_scan_render: the largest z with
    F <= 1 per pixel, quantised to floor(levels z) / levels; levels = 0: continuous).  No autograd."""
    _require_cuda(params)
    if params.dim() != 2 or params.shape[1] != 12:
        raise ValueError("params must be [B,12], got %s" % (tuple(params.shape),))
    p = params.detach().to(torch.float32).contiguous()
    out = torch.empty(p.shape[0], int(size), int(size), dtype=torch.float32, device=p.device)
    check(lib().sqr_scan_render(ptr(p), p.shape[0], int(size), int(levels), ptr(out), stream_ptr(p.device)),
          "sqr_scan_render")
    return out


def iou_counts(p_true, p_pred, R):
    """[B,2] int64 (intersection, union) voxel counts of IoUAccuracy (classes.py:394-447).  The
    kernel works in float64 like the reference; float64 parameters (visu.py) are used as given."""
    _require_cuda(p_true, p_pred)
    f64 = p_true.dtype == torch.float64 or p_pred.dtype == torch.float64
    dt = torch.float64 if f64 else torch.float32
    pt = p_true.detach().to(dt).contiguous()
    pp = p_pred.detach().to(dt).contiguous()
    out = torch.empty(pt.shape[0], 2, dtype=torch.int64, device=pt.device)
    fn = lib().sqr_iou_counts_f64 if f64 else lib().sqr_iou_counts
    check(fn(ptr(pt), ptr(pp), pt.shape[0], int(R), ptr(out), stream_ptr(pt.device)), "sqr_iou_counts")
    return out
