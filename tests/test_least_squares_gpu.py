"""The LeastSquares HIP kernel (sqr_least_squares_fwd_bwd, sqr.losses.least_squares, classes.LeastSquares
on CUDA tensors, train.py --loss leastsquares, sqr.fit.refine).

The float64 comparison is the plain-torch classes.LeastSquares on the CPU with float64 inputs, which
tests/test_least_squares_cpu.py pins to the reference's own class.

Tolerance.  The reference computes this loss in float32, so the yardstick is that float32 plain-torch
path against its own float64 run on the same inputs: the test measures, over its whole case set, the
largest relative loss error and the largest gradient error over the sample's largest gradient entry of
the float32 path, and the kernel's two maxima over the same set must stay within twice them (the
factor of tests/test_optim_kernels_gpu.py).  Measured on MI355X: see DESIGN.md, "LeastSquares".
"""
import os

import numpy as np
import pytest
import torch

from _lsq_cases import example, golden_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (R, H, W, batch sizes): the smallest shapes at which each branch of the kernel exists
SHAPES = [
    (8, 16, 16, (1, 2, 3)),    # a partly filled block
    (16, 32, 32, (1, 2, 3)),   # exactly one block of 256
    (32, 32, 32, (1, 2, 3)),   # four blocks per sample: the partial sums
    (12, 32, 32, (1, 2, 3)),   # inexact c / R, non-integer resize ratio
    (32, 16, 16, (1, 2, 3)),   # upsampling
    (16, 24, 40, (1, 2, 3)),   # non-square target
    (8, 8, 8, (1025,)),        # the batch mean beyond one finalize block
]


def _resample(ex, idx, H, W):
    """Example images idx at HxW (nearest source pixel)."""
    rows, cols = np.arange(H) * 256 // H, np.arange(W) * 256 // W
    return np.ascontiguousarray(ex[np.asarray(idx)][:, :, rows][:, :, :, cols])


def _shape_cases():
    ex, labels = example()
    rng = np.random.default_rng(20261019)
    out = []
    for R, H, W, Bs in SHAPES:
        for B in Bs:
            idx = (np.arange(B) + R + B) % 10
            pred = (labels[idx] + 0.05 * rng.normal(size=(B, 12))).astype(np.float32)
            out.append(dict(name="R%d_%dx%d_B%d" % (R, H, W, B), R=R, true=_resample(ex, idx, H, W), pred=pred))
    return out


def _torch_ref(true, pred, R, dt):
    """The plain-torch class on the CPU in dtype dt -> (loss, grad [B,12]) as float64 numpy."""
    import classes
    p = torch.tensor(pred).to(dt).requires_grad_(True)
    loss = classes.LeastSquares(R, "cpu")(torch.tensor(true).to(dt), p)
    loss.backward()
    return loss.item(), p.grad.numpy().astype(np.float64)


def _kernel(true, pred, R, grad=True):
    """sqr.losses.least_squares on the GPU -> (loss 0-d float64 tensor, grad [B,12] numpy or None)."""
    from sqr import losses
    p = torch.tensor(pred, device=DEV, requires_grad=grad)
    loss = losses.least_squares(torch.tensor(true, device=DEV), p, R)
    if grad:
        loss.backward()
    torch.cuda.synchronize()
    return loss, (p.grad.cpu().numpy() if grad else None)


def _grad_err(g, gref):
    """Largest error over the sample's largest gradient entry (samples without a gradient: skipped)."""
    return max((np.abs(g[b] - gref[b]).max() / np.abs(gref[b]).max() for b in range(len(g)) if gref[b].any()),
               default=0.0)


@pytest.fixture(scope="module")
def accuracy_rows():
    """Per case of the set (fixture cases at their own R + the shape table): the float32 plain-torch
    path's and the kernel's loss and gradient errors against float64.  Computed once."""
    rows = []
    for c in golden_cases() + _shape_cases():
        l64, g64 = _torch_ref(c["true"], c["pred"], c["R"], torch.float64)
        l32, g32 = _torch_ref(c["true"], c["pred"], c["R"], torch.float32)
        lk, gk = _kernel(c["true"], c["pred"], c["R"])
        assert lk.dtype == torch.float64 and lk.dim() == 0
        lk = lk.item()
        assert np.isfinite(lk) and np.isfinite(gk).all(), c["name"]
        if l64 == 0.0:  # no point in any image: nothing to divide by, and nothing to be off by
            assert lk == 0.0 and not gk.any(), c["name"]
            continue
        rows.append(dict(name=c["name"], loss_ref=abs(l32 - l64) / abs(l64), loss_kernel=abs(lk - l64) / abs(l64),
                         grad_ref=_grad_err(g32, g64), grad_kernel=_grad_err(gk.astype(np.float64), g64)))
    return rows


def test_loss_and_gradient_vs_float64(accuracy_rows):
    for r in accuracy_rows:
        print("%-18s loss: f32 torch %.2e kernel %.2e | grad: f32 torch %.2e kernel %.2e"
              % (r["name"], r["loss_ref"], r["loss_kernel"], r["grad_ref"], r["grad_kernel"]))
    mx = {k: max(r[k] for r in accuracy_rows) for k in ("loss_ref", "loss_kernel", "grad_ref", "grad_kernel")}
    print("maxima: %s; ratios: loss %.3f grad %.3f"
          % (mx, mx["loss_kernel"] / mx["loss_ref"], mx["grad_kernel"] / mx["grad_ref"]))
    assert len(accuracy_rows) >= 11 + 19
    assert mx["loss_kernel"] <= 2 * mx["loss_ref"], mx
    assert mx["grad_kernel"] <= 2 * mx["grad_ref"], mx


def test_class_on_cuda_returns_preds_dtype():
    import classes
    from sqr import losses
    c = golden_cases()[3]
    t = torch.tensor(c["true"], device=DEV)
    p = torch.tensor(c["pred"], device=DEV, requires_grad=True)
    loss = classes.LeastSquares(c["R"], DEV)(t, p)
    assert loss.dtype == torch.float32 and loss.dim() == 0  # the reference's dtype: pred's
    loss.backward()
    l64, g = _kernel(c["true"], c["pred"], c["R"])
    assert loss.item() == l64.float().item()  # the float64 mean, rounded once
    np.testing.assert_array_equal(p.grad.cpu().numpy(), g)
    # [B,H,W] targets are accepted like [B,1,H,W]
    assert losses.least_squares(t[:, 0], p.detach(), c["R"]).item() == l64.item()


def test_runs_are_bitwise_equal_and_no_grad_gives_the_same_loss():
    c = golden_cases()[5]
    l1, g1 = _kernel(c["true"], c["pred"], c["R"])
    l2, g2 = _kernel(c["true"], c["pred"], c["R"])
    with torch.no_grad():
        l0, _ = _kernel(c["true"], c["pred"], c["R"], grad=False)
    assert l0.item() == l1.item() == l2.item()
    assert np.array_equal(g1, g2)


def test_empty_one_point_and_nan_pixels():
    from sqr import losses
    by = {c["name"]: c for c in golden_cases()}
    z = by["zero_R32"]
    loss, g = _kernel(z["true"], z["pred"], 32)
    assert loss.item() == 0.0 and not g.any()  # exact zeros, not NaN
    o = by["onepix_R32"]
    p = torch.tensor(o["pred"], device=DEV)
    e = losses.least_squares(torch.tensor(o["true"], device=DEV), p, 32, per_sample=True)
    assert (e > 0).all()
    # one empty image in a batch leaves the other rows alone
    mixed = o["true"].copy()
    mixed[1] = 0
    e2 = losses.least_squares(torch.tensor(mixed, device=DEV), p, 32, per_sample=True)
    assert e2[1].item() == 0.0 and e2[0].item() == e[0].item() and e2[2].item() == e[2].item()
    # a NaN pixel does not count: the same as a zero there
    c = by["noisy_R32"]
    holes, nans = c["true"].copy(), c["true"].copy()
    holes[:, :, 96:160, 64:128] = 0
    nans[:, :, 96:160, 64:128] = np.nan
    lh, gh = _kernel(holes, c["pred"], 32)
    ln, gn = _kernel(nans, c["pred"], 32)
    assert lh.item() == ln.item() and np.array_equal(gh, gn)
    assert lh.item() != _kernel(c["true"], c["pred"], 32, grad=False)[0].item()


def test_clamp_masks_zero_the_clamped_entries():
    c = {c["name"]: c for c in golden_cases()}["clamps_R32"]
    _, g = _kernel(c["true"], c["pred"], 32)
    p = c["pred"]
    inside = np.ones_like(p, dtype=bool)
    inside[:, 0:3] = (p[:, 0:3] >= np.float32(0.05)) & (p[:, 0:3] <= 1)
    inside[:, 3:5] = (p[:, 3:5] >= np.float32(0.1)) & (p[:, 3:5] <= 1)
    inside[:, 5:8] = (p[:, 5:8] >= 0) & (p[:, 5:8] <= 1)
    assert (~inside).sum() == 12
    assert not g[~inside].any()
    assert not c["grad64"][~inside].any()  # and so does autograd through torch.clamp
    assert (g[inside] != 0).all()


def test_upstream_gradient_scaling_scalar_and_per_sample():
    from sqr import losses
    c = golden_cases()[4]
    R, B = c["R"], len(c["pred"])
    t = torch.tensor(c["true"], device=DEV)
    _, g = _kernel(c["true"], c["pred"], R)
    p = torch.tensor(c["pred"], device=DEV, requires_grad=True)
    (3.0 * losses.least_squares(t, p, R)).backward()
    np.testing.assert_allclose(p.grad.cpu().numpy(), 3 * g, rtol=1e-6)
    # per sample: row b of the stored d(mean)/d params times B * gout[b]
    p = torch.tensor(c["pred"], device=DEV, requires_grad=True)
    e = losses.least_squares(t, p, R, per_sample=True)
    assert e.shape == (B,) and e.dtype == torch.float64
    assert abs(e.mean().item() - losses.least_squares(t, p.detach(), R).item()) <= 1e-14 * e.mean().item()
    w = torch.tensor([0.5, 2.0, -1.0], dtype=torch.float64, device=DEV)
    (e * w).sum().backward()
    np.testing.assert_allclose(p.grad.cpu().numpy(), B * g * w.cpu().numpy()[:, None].astype(np.float32), rtol=1e-6)


def test_rejects_mixed_devices_and_bad_shapes():
    import classes
    from sqr import losses
    crit = classes.LeastSquares(32, DEV)
    with pytest.raises(ValueError):
        crit(torch.zeros(2, 1, 64, 64), torch.zeros(2, 12, device=DEV))
    with pytest.raises(ValueError):
        crit(torch.zeros(2, 1, 64, 64, device=DEV), torch.zeros(2, 12))
    with pytest.raises(ValueError):
        crit(torch.zeros(2, 1, 64, 64, device=DEV), torch.zeros(2, 11, device=DEV))
    with pytest.raises(ValueError):
        crit(torch.zeros(3, 1, 64, 64, device=DEV), torch.zeros(2, 12, device=DEV))
    with pytest.raises(ValueError):
        losses.least_squares(torch.zeros(2, 2, 64, 64, device=DEV), torch.zeros(2, 12, device=DEV), 32)
    with pytest.raises(ValueError):
        losses.least_squares(torch.zeros(64, 64, device=DEV), torch.zeros(2, 12, device=DEV), 32)


GUARD = 64  # guard elements on either side of every output


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all())


@pytest.mark.parametrize("R,H,W,B", [(8, 16, 16, 3), (32, 32, 32, 2), (12, 24, 40, 3), (8, 8, 8, 1025)])
def test_c_abi_writes_inside_its_buffers_only(R, H, W, B):
    """Guard words around loss_per_sample, grad and the workspace; need_grad = 0 writes no gradient and
    gives the same loss bitwise; an undersized workspace is refused."""
    from sqr._lib import lib, ptr, stream_ptr
    L = lib()
    ex, labels = example()
    idx = np.arange(B) % 10
    p = torch.tensor(labels[idx] + np.float32(0.03), device=DEV)
    t = torch.tensor(_resample(ex, idx, H, W)[:, 0], device=DEV).contiguous()
    wsb = L.sqr_least_squares_workspace_bytes(B, R)
    assert wsb == B * ((R * R + 255) // 256) * 18 * 8
    out = {}
    for need_grad in (1, 0):
        lbuf, lps = _guarded(B, torch.float64, -7.25)
        mbuf, mean = _guarded(1, torch.float64, -7.25)
        gbuf, grad = _guarded(B * 12, torch.float32, -7.25)
        wbuf, ws = _guarded(wsb, torch.uint8, 0xA5)
        rc = L.sqr_least_squares_fwd_bwd_mean(ptr(p), ptr(t), B, H, W, R, need_grad, ptr(lps), ptr(mean), ptr(grad),
                                              ptr(ws), wsb, stream_ptr(DEV))
        torch.cuda.synchronize()
        assert rc == 0, L.sqr_last_error_string()
        assert _guards_intact(lbuf, B, -7.25) and _guards_intact(mbuf, 1, -7.25)
        assert _guards_intact(gbuf, B * 12, -7.25) and _guards_intact(wbuf, wsb, 0xA5)
        assert torch.isfinite(lps).all() and (lps >= 0).all() and (lps > 0).any()
        if need_grad:
            assert torch.isfinite(grad).all() and (grad != -7.25).all()
        else:
            assert (grad == -7.25).all()  # untouched
        out[need_grad] = (lps.clone(), mean.clone())
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    # the mean is the per-sample values' mean (summed in another order: a few float64 ulps)
    assert abs(out[1][1].item() - out[1][0].mean().item()) <= 1e-13 * out[1][1].item()
    # the entry point without the mean gives the same per-sample values
    lps2 = torch.empty(B, dtype=torch.float64, device=DEV)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    assert L.sqr_least_squares_fwd_bwd(ptr(p), ptr(t), B, H, W, R, 0, ptr(lps2), None, ptr(ws), wsb,
                                       stream_ptr(DEV)) == 0
    torch.cuda.synchronize()
    assert torch.equal(lps2, out[1][0])
    assert L.sqr_least_squares_fwd_bwd(ptr(p), ptr(t), B, H, W, R, 0, ptr(lps2), None, ptr(ws), wsb - 1,
                                       stream_ptr(DEV)) == -3
    assert b"workspace" in L.sqr_last_error_string()
    assert L.sqr_least_squares_fwd_bwd(ptr(p), ptr(t), B, H, W, R, 1, ptr(lps2), None, ptr(ws), wsb,
                                       stream_ptr(DEV)) == -1  # need_grad without a gradient buffer


def test_forward_backward_captured_in_a_graph_replays_bitwise():
    """The property the kernel path exists for: no host wait, so the loss and its backward can be
    captured in a HIP graph; a replay equals the eager run bitwise, also on new inputs."""
    from sqr import losses
    a, b = golden_cases()[3], golden_cases()[0]
    assert a["R"] == b["R"] == 32
    eager = {k: _kernel(c["true"], c["pred"], 32) for k, c in (("a", a), ("b", b))}
    t = torch.tensor(a["true"], device=DEV)
    p = torch.tensor(a["pred"], device=DEV, requires_grad=True)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss = losses.least_squares(t, p, 32)
        loss.backward()
    for k, c in (("a", a), ("b", b), ("a", a)):
        t.copy_(torch.tensor(c["true"]))
        p.data.copy_(torch.tensor(c["pred"]))
        g.replay()
        torch.cuda.synchronize()
        assert loss.item() == eager[k][0].item(), k
        assert np.array_equal(p.grad.cpu().numpy(), eager[k][1]), k


@pytest.mark.parametrize("amp", ["--bf16", "--fp16"])
def test_train_py_least_squares_graph_equals_eager(tmp_path, capsys, amp):
    """train.py --loss leastsquares: the captured step (eager warm-up, capture, replay; with --fp16 the
    loss scaler too) ends on bitwise the weights of the eager loop."""
    import train

    def run(graph):
        ck = os.path.join(str(tmp_path), "ck%d.pt" % graph)
        torch.manual_seed(0)
        tl, vl = train.main(["--loss", "leastsquares", "--synthetic", "44", "--batch-size", "8", "--epochs", "1",
                             "--max-steps", "3", "--render-size", "32", "--pretrained", "0", "--graph", str(graph),
                             "--model-location", ck, "--log-interval", "1", amp])
        return tl, vl, torch.load(ck, map_location="cpu", weights_only=True)

    tl_g, vl_g, ck_g = run(1)
    assert "HIP graph" in capsys.readouterr().out
    tl_e, vl_e, ck_e = run(0)
    assert "eager" in capsys.readouterr().out
    assert np.isfinite(tl_g).all() and np.isfinite(vl_g).all()
    assert tl_g == tl_e and vl_g == vl_e, (tl_g, tl_e, vl_g, vl_e)
    for k, v in ck_e["model_state_dict"].items():
        assert torch.equal(ck_g["model_state_dict"][k], v), k


def test_refine_descends_the_energy():
    """sqr.fit.refine at B = 3, R = 16, 20 steps on the example images 0-2 at 64x64, from labels + 0.05
    noise (seed 0; with the plain-torch class on the CPU the same run takes the three energies from
    0.123, 0.598, 0.101 to 0.0117, 0.310, 0.0036)."""
    from sqr import fit, losses
    ex, labels = example()
    idx = [0, 1, 2]
    img = torch.tensor(_resample(ex, idx, 64, 64), device=DEV)
    start = (labels[idx] + 0.05 * np.random.default_rng(0).normal(size=(3, 12))).astype(np.float32)
    p0 = torch.tensor(start, device=DEV)
    refined, before, after = fit.refine(img, p0, steps=20, lr=2e-3, render_size=16)
    torch.cuda.synchronize()
    assert refined.shape == (3, 12) and refined.dtype == torch.float32 and not refined.requires_grad
    assert torch.equal(p0, torch.tensor(start, device=DEV))  # the input is left alone
    assert torch.equal(before, losses.least_squares(img, p0, 16, per_sample=True))
    assert torch.equal(after, losses.least_squares(img, refined, 16, per_sample=True))
    assert (after < before).all(), (before, after)
    again = fit.refine(img, p0, steps=20, lr=2e-3, render_size=16)
    assert all(torch.equal(x, y) for x, y in zip((refined, before, after), again))


def test_test_py_refine_prints_energies_and_refined_parameters(tmp_path, capsys):
    """test.py --refine N on an example image (random weights: no checkpoint needed)."""
    import importlib.util
    from conftest import PKG
    from _golden import load
    img = load("example_images.npz")["images"][0]
    h, w = img.shape
    stride = (w * 3 + 3) & ~3
    rows = np.zeros((h, stride), np.uint8)
    rows[:, :w * 3] = np.repeat(img[::-1], 3, axis=1)  # a bottom-up 24-bit BMP, as the scanner writes
    hdr = b"BM" + (54 + rows.size).to_bytes(4, "little") + b"\0\0\0\0" + (54).to_bytes(4, "little")
    dib = (40).to_bytes(4, "little") + w.to_bytes(4, "little") + h.to_bytes(4, "little") + \
        (1).to_bytes(2, "little") + (24).to_bytes(2, "little") + b"\0" * 24
    bmp = tmp_path / "x.bmp"
    bmp.write_bytes(hdr + dib + rows.tobytes())
    spec = importlib.util.spec_from_file_location("sq_test_py", os.path.join(PKG, "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(0)
    a, e, t, q = mod.main(["--image", str(bmp), "--model", str(tmp_path / "none.pt"), "--device", DEV,
                           "--refine", "5", "--refine-lr", "1e-3"])
    out = capsys.readouterr().out
    assert out.count("Size a:") == 2 and "Refined parameters (5 steps, LeastSquares energy" in out
    assert a.shape == (1, 3) and e.shape == (1, 2) and t.shape == (1, 3) and q.shape == (1, 4)
    assert all(np.isfinite(v).all() for v in (a, e, t, q))
