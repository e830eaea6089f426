"""HIP loss kernels (libsqr) vs the reference's golden vectors and the float64 oracle.

Tolerances (north star): loss <= 1e-4 relative (fp32 kernel vs f64 reference).  Gradients are
fp32 sums over R^3 voxels of a sigmoid with sharpness up to 260; they are compared with
max|g - g_ref| <= 2e-4 * max|g_ref| per sample (measured ~1e-5-1e-4).

These are end-to-end checks through the classes.  The stages between the kernel and the 12 gradients (the
per-block partials, the float64 finalize, the batch mean, sqr_loss_grad_scale), the zero fix on rows where
it fires, np.arange's extra node and the C ABI's guard words and refusals: tests/test_loss_kernels_gpu.py.
"""
import numpy as np
import pytest
import torch

import sq_oracle as O
from _golden import cases
from _loss_ref import sample

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _classes():
    import classes
    return classes


_sample = sample   # (shared with test_loss_kernels_gpu.py)


def _run_implicit(true, pred, R, tau, s, grad=True):
    C = _classes()
    crit = C.ImplicitLoss(R, DEV, tau, s)
    p = torch.tensor(pred, device=DEV, requires_grad=grad)
    loss = crit(torch.tensor(true, device=DEV), p)
    if grad:
        loss.backward()
    torch.cuda.synchronize()
    return loss, (p.grad.cpu().numpy() if grad else None)


def _grad_close(g, gref, rel=2e-4):
    for b in range(g.shape[0]):
        scale = max(np.abs(gref[b]).max(), 1e-12)
        assert np.abs(g[b] - gref[b]).max() <= rel * scale, (b, g[b], gref[b])


@pytest.mark.parametrize("case", cases("implicit_loss.npz"), ids=lambda c: str(c["name"]))
def test_implicit_vs_golden(case):
    loss, g = _run_implicit(case["true"], case["pred"], int(case["R"]), float(case["tau"]), float(case["s"]))
    assert loss.dtype == torch.float64 and loss.dim() == 0
    ref = float(case["loss"])
    assert abs(loss.item() - ref) <= 1e-4 * abs(ref)
    _grad_close(g, case["grad"].astype(np.float64))


@pytest.mark.parametrize("R", [2, 3, 16, 33, 64, 100, 128, 200])
def test_implicit_vs_oracle_sizes(R):
    rng = np.random.default_rng(R)
    B = 3
    pred = _sample(rng, B)
    true = (rng.uniform(size=(B, 1, 256, 256)) * (rng.uniform(size=(B, 1, 256, 256)) > 0.5)).astype(np.float32)
    L, G, _, _ = O.implicit_loss(true, pred, R, 1.5, 260)
    loss, g = _run_implicit(true, pred, R, 1.5, 260)
    assert abs(loss.item() - L) <= 1e-4 * abs(L)
    _grad_close(g, G)


@pytest.mark.parametrize("R,tau", [(64, 1.5), (64, 6.0), (64, 12.0), (128, 6.0)])
def test_implicit_grad_prefix_form_vs_f64(R, tau):
    """The kernel's 17 gradient moments use suffix sums of the transmittance as Ttot - prefix
    (one pass down each ray, sqr_loss.hip).  Its fp32 error is ~eps * Ttot per term, Ttot <= R, and
    it matters most where the true suffix is small: a large tau (the transmittance dies inside the
    object) and long rays.  Against the float64 two-pass oracle (oracle/sq_oracle.py, the
    reference's autograd of classes.py:284-291), the parameter gradient stays within
    2e-4 + 8 * R * eps32 of max|g_ref| per sample."""
    rng = np.random.default_rng(int(R * 10 + tau))
    B = 4
    pred = _sample(rng, B)
    from sqr import losses
    # targets rendered from nearby parameters: the silhouettes overlap, so the gradient is not
    # dominated by the background pixels
    near = pred.copy()
    near[:, :8] = np.clip(pred[:, :8] + rng.normal(scale=0.02, size=(B, 8)), 0.02, 0.98)
    true = losses.implicit_render(torch.tensor(near, device=DEV), 256, tau, 260).unsqueeze(1).cpu().numpy()
    L, G, _, _ = O.implicit_loss(true, pred, R, tau, 260)
    loss, g = _run_implicit(true, pred, R, tau, 260)
    assert abs(loss.item() - L) <= 1e-4 * abs(L)
    _grad_close(g, G, rel=2e-4 + 8 * R * 2.0 ** -23)


def test_implicit_render_matches_oracle():
    from sqr import losses
    rng = np.random.default_rng(3)
    pred = _sample(rng, 4)
    for R in (32, 64):
        img = losses.implicit_render(torch.tensor(pred, device=DEV), R, 1.5, 260).cpu().numpy()
        for b in range(4):
            ref = O.depth_projection(pred[b], R, 1.5, 260)
            assert np.abs(img[b] - ref).max() < 2e-4


def test_implicit_no_grad_path_and_determinism():
    rng = np.random.default_rng(5)
    pred = _sample(rng, 64)
    true = rng.uniform(size=(64, 1, 256, 256)).astype(np.float32)
    with torch.no_grad():
        l0, _ = _run_implicit(true, pred, 32, 1.5, 260, grad=False)
    l1, g1 = _run_implicit(true, pred, 32, 1.5, 260)
    l2, g2 = _run_implicit(true, pred, 32, 1.5, 260)
    assert l0.item() == l1.item() == l2.item()
    assert np.array_equal(g1, g2)  # fixed-order reduction: bitwise reproducible


def test_implicit_large_batch_property():
    # B=512 (the DDP global batch): the batch-mean loss is the mean of per-chunk losses and the
    # gradient of a chunk scales by chunk/B
    rng = np.random.default_rng(6)
    B = 512
    pred = _sample(rng, B)
    true = rng.uniform(size=(B, 1, 256, 256)).astype(np.float32)
    lall, gall = _run_implicit(true, pred, 32, 1.5, 260)
    parts = [_run_implicit(true[i:i + 64], pred[i:i + 64], 32, 1.5, 260) for i in range(0, B, 64)]
    assert abs(np.mean([p[0].item() for p in parts]) - lall.item()) <= 1e-12
    gcat = np.concatenate([p[1] for p in parts]) * (64 / B)
    np.testing.assert_allclose(gall, gcat, rtol=1e-6, atol=1e-12)


def test_implicit_grad_scales_with_upstream():
    rng = np.random.default_rng(7)
    pred = _sample(rng, 4)
    true = rng.uniform(size=(4, 1, 256, 256)).astype(np.float32)
    C = _classes()
    crit = C.ImplicitLoss(32, DEV, 1.5, 260)
    p = torch.tensor(pred, device=DEV, requires_grad=True)
    (3.0 * crit(torch.tensor(true, device=DEV), p)).backward()
    _, g1 = _run_implicit(true, pred, 32, 1.5, 260)
    np.testing.assert_allclose(p.grad.cpu().numpy(), 3 * g1, rtol=1e-6)


def test_implicit_rejects_mixed_devices_and_bad_shapes():
    C = _classes()
    crit = C.ImplicitLoss(32, DEV)
    with pytest.raises(ValueError):
        crit(torch.zeros(2, 1, 64, 64), torch.zeros(2, 12, device=DEV))
    with pytest.raises(ValueError):
        crit(torch.zeros(2, 1, 64, 64, device=DEV), torch.zeros(2, 11, device=DEV))


@pytest.mark.parametrize("case", cases("explicit_loss.npz"), ids=lambda c: str(c["name"]))
def test_explicit_vs_golden(case):
    C = _classes()
    crit = C.ExplicitLoss(int(case["R"]), DEV)
    p = torch.tensor(case["pred"], device=DEV, requires_grad=True)
    loss = crit(torch.tensor(case["true"], device=DEV), p)
    loss.backward()
    ref = float(case["loss"])
    assert loss.dtype == torch.float64
    assert abs(loss.item() - ref) <= 1e-4 * abs(ref)
    _grad_close(p.grad.cpu().numpy(), case["grad"].astype(np.float64))


@pytest.mark.parametrize("R", [8, 64])
def test_explicit_vs_oracle(R):
    rng = np.random.default_rng(R + 100)
    t, p = _sample(rng, 3), _sample(rng, 3)
    L, G, _ = O.explicit_loss(t, p, R)
    C = _classes()
    pp = torch.tensor(p, device=DEV, requires_grad=True)
    loss = C.ExplicitLoss(R, DEV)(torch.tensor(t, device=DEV), pp)
    loss.backward()
    assert abs(loss.item() - L) <= 1e-4 * abs(L)
    _grad_close(pp.grad.cpu().numpy(), G)


@pytest.mark.parametrize("case", cases("iou.npz"), ids=lambda c: str(c["name"]))
def test_iou_vs_golden(case):
    C = _classes()
    R = int(case["R"])
    t = torch.tensor(case["true"], device=DEV)
    p = torch.tensor(case["pred"], device=DEV)
    red = C.IoUAccuracy(R, DEV)(t, p)
    assert red.dtype == torch.float32
    assert red.item() == pytest.approx(float(case["iou"]), rel=1e-6)
    per = C.IoUAccuracy(R, DEV, reduce=False)(t, p).cpu().numpy()
    np.testing.assert_allclose(per, case["iou_per"], rtol=1e-12)
    cnt = O.iou_counts(case["true"], case["pred"], R)
    from sqr import losses
    assert np.array_equal(losses.iou_counts(t, p, R).cpu().numpy(), cnt)


# ---------------------------------------------------------------------------- config 4
def test_combined_explicit_implicit_vs_oracle():
    """BASELINE config 4 (the torch/visu.py path): ExplicitLoss(32)(p_true, pred) +
    ImplicitLoss(64, tau 1.5, s 260)(image, pred) through one backward vs the f64 oracle."""
    from sqr import losses
    C = _classes()
    rng = np.random.default_rng(44)
    B = 4
    pt, pr = _sample(rng, B), _sample(rng, B)
    img = losses.implicit_render(torch.tensor(pt, device=DEV), 256, 1.5, 260).unsqueeze(1)
    Le, Ge, _ = O.explicit_loss(pt, pr, 32)
    Li, Gi, _, _ = O.implicit_loss(img.cpu().numpy(), pr, 64, 1.5, 260)
    p = torch.tensor(pr, device=DEV, requires_grad=True)
    loss = C.ExplicitLoss(32, DEV)(torch.tensor(pt, device=DEV), p) + C.ImplicitLoss(64, DEV, 1.5, 260)(img, p)
    loss.backward()
    assert loss.dtype == torch.float64
    assert abs(loss.item() - (Le + Li)) <= 1e-4 * abs(Le + Li)
    _grad_close(p.grad.cpu().numpy(), Ge + Gi)


def test_combined_loss_bench_batch_properties():
    """Config 4 at the bench batch (B=64): the combined gradient is the sum of the two losses'
    gradients (linearity of backward), and the batch-mean splits over chunks exactly."""
    from sqr import losses
    C = _classes()
    rng = np.random.default_rng(45)
    B = 64
    pt = torch.tensor(_sample(rng, B), device=DEV)
    pr = _sample(rng, B)
    img = losses.implicit_render(pt, 256, 1.5, 260).unsqueeze(1)
    ex, im = C.ExplicitLoss(32, DEV), C.ImplicitLoss(64, DEV, 1.5, 260)
    grads, vals = [], []
    for parts in (("e",), ("i",), ("e", "i")):
        p = torch.tensor(pr, device=DEV, requires_grad=True)
        loss = sum(ex(pt, p) if k == "e" else im(img, p) for k in parts)
        loss.backward()
        grads.append(p.grad.clone())
        vals.append(loss.item())
    assert abs(vals[2] - (vals[0] + vals[1])) <= 1e-12 * abs(vals[2])
    torch.testing.assert_close(grads[2], grads[0] + grads[1], rtol=1e-6, atol=1e-12)
    chunks = [ex(pt[i:i + 16], torch.tensor(pr[i:i + 16], device=DEV)).item() for i in range(0, B, 16)]
    assert abs(np.mean(chunks) - vals[0]) <= 1e-12
    assert np.isfinite(grads[2].cpu().numpy()).all() and grads[2].abs().sum() > 0


def test_iou_float64_params_exact_counts():
    """visu.py feeds float64 parameters to IoUAccuracy (visu.py:142-159): they are used without
    rounding to fp32, so the integer counts equal the f64 oracle's exactly; rounding the same
    parameters to fp32 moves boundary voxels."""
    from sqr import losses
    rng = np.random.default_rng(46)
    B, R = 48, 128
    t = _sample(rng, B).astype(np.float64) + rng.uniform(-1e-7, 1e-7, (B, 12))
    p = _sample(rng, B).astype(np.float64) + rng.uniform(-1e-7, 1e-7, (B, 12))
    cnt = losses.iou_counts(torch.tensor(t, device=DEV), torch.tensor(p, device=DEV), R).cpu().numpy()
    np.testing.assert_array_equal(cnt, O.iou_counts(t, p, R))
    C = _classes()
    acc = C.IoUAccuracy(R, DEV)(torch.tensor(t, device=DEV), torch.tensor(p, device=DEV))
    assert acc.item() == pytest.approx(O.iou_accuracy(t, p, R), rel=1e-6)
