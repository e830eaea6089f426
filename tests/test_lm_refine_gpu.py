"""Levenberg-Marquardt refinement on the GPU: the normal-equations kernel (sqr_least_squares_normal_eq,
sqr.losses.least_squares_normal_eq), the step kernel (sqr_lsq_lm_step) and the loop (sqr_lsq_lm_refine,
sqr.fit.refine_lm, sqr.fit.refine(method="lm"), test.py --refine-method lm).

The float64 comparison is tests/_lm_ref.py: the residuals of classes.LeastSquares.energy_function, their
Jacobian by autograd, and the same accept / solve / project rules, on the CPU.

Tolerances.  Normal equations: the yardstick of tests/test_least_squares_gpu.py, the float32 plain-torch
path against its own float64 run on the same inputs; over the whole case set the kernel's largest
relative error of E, largest error of g over the sample's largest |g| entry and largest error of H over
the sample's largest diagonal entry must stay within twice the float32 path's.  The solve: normwise
backward error at most 1e-13 (Cholesky's bound is a small multiple of 12 x 1.1e-16).  The loop: the final
energy over the float64 loop's, per image and at least 1, within twice the worst such ratio of the
float32 plain-torch loop.  Measured on MI355X: see DESIGN.md, "Levenberg-Marquardt refinement".
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _lm_ref
from _lsq_cases import example, golden_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (R, H, W): the smallest shapes at which each branch of the kernel exists; B = 1, 2, 3 each
SHAPES = [
    (8, 16, 16),    # a partly filled block
    (16, 32, 32),   # exactly one block of 256
    (32, 32, 32),   # four blocks per sample: the partial sums
    (12, 32, 32),   # inexact c / R, non-integer resize ratio
    (16, 24, 40),   # non-square target
]


def _resample(ex, idx, H, W):
    """Example images idx at HxW (nearest source pixel)."""
    rows, cols = np.arange(H) * 256 // H, np.arange(W) * 256 // W
    return np.ascontiguousarray(ex[np.asarray(idx)][:, :, rows][:, :, :, cols])


def _shape_cases():
    ex, labels = example()
    rng = np.random.default_rng(20261019)
    out = []
    for R, H, W in SHAPES:
        for B in (1, 2, 3):
            idx = (np.arange(B) + R + B) % 10
            pred = (labels[idx] + 0.05 * rng.normal(size=(B, 12))).astype(np.float32)
            out.append(dict(name="R%d_%dx%d_B%d" % (R, H, W, B), R=R, true=_resample(ex, idx, H, W), pred=pred))
    return out


def _kernel(true, pred, R):
    """sqr.losses.least_squares_normal_eq -> float64 numpy (H, g, E)."""
    from sqr import losses
    H, g, E = losses.least_squares_normal_eq(torch.tensor(true, device=DEV), torch.tensor(pred, device=DEV), R)
    torch.cuda.synchronize()
    assert H.dtype == g.dtype == E.dtype == torch.float64
    assert H.shape == (len(pred), 12, 12) and g.shape == (len(pred), 12) and E.shape == (len(pred),)
    return H.cpu().numpy(), g.cpu().numpy(), E.cpu().numpy()


def _errs(H, g, E, H64, g64, E64):
    """Per-sample maxima over a case: E relative, g over the largest |g| entry, H over the largest diagonal."""
    e = max(abs(E[b] - E64[b]) / E64[b] for b in range(len(E)))
    ge = max(np.abs(g[b] - g64[b]).max() / np.abs(g64[b]).max() for b in range(len(E)))
    he = max(np.abs(H[b] - H64[b]).max() / np.diagonal(H64[b]).max() for b in range(len(E)))
    return e, ge, he


@pytest.fixture(scope="module")
def accuracy_rows():
    """Per case of the set (fixture cases at their own R + the shape table): the float32 plain-torch path's
    and the kernel's errors of E, g, H against float64; the kernel's outputs are kept.  Computed once."""
    rows = []
    for c in golden_cases() + _shape_cases():
        ref64 = _lm_ref.normal_eq(c["true"], c["pred"], c["R"], torch.float64)
        ref32 = _lm_ref.normal_eq(c["true"], c["pred"], c["R"], torch.float32)
        ker = _kernel(c["true"], c["pred"], c["R"])
        assert all(np.isfinite(x).all() for x in ker), c["name"]
        row = dict(name=c["name"], kernel=ker, ref64=ref64)
        if (ref64[2] == 0).any():  # no point in an image: nothing to divide by, and nothing to be off by
            assert not (ref64[2] != 0).any(), c["name"]
            assert not any(x.any() for x in ker), c["name"]
        else:
            row["ref"], row["ker"] = _errs(*ref32, *ref64), _errs(*ker, *ref64)
        rows.append(row)
    return rows


def test_normal_equations_vs_float64(accuracy_rows):
    """Measured on MI355X (maxima over the set; float32 torch | kernel): E 1.00e-5 | 4.93e-6, g 2.26e-5 |
    4.13e-6, H 2.47e-6 | 8.86e-7: ratios 0.49, 0.18, 0.36 of the 2 allowed."""
    rows = [r for r in accuracy_rows if "ker" in r]
    for r in rows:
        print("%-18s f32 torch E %.2e g %.2e H %.2e | kernel E %.2e g %.2e H %.2e" % ((r["name"],) + r["ref"] + r["ker"]))
    ref = [max(r["ref"][i] for r in rows) for i in range(3)]
    ker = [max(r["ker"][i] for r in rows) for i in range(3)]
    print("maxima (E, g, H): f32 torch %s kernel %s ratios %s"
          % (["%.3e" % v for v in ref], ["%.3e" % v for v in ker], ["%.3f" % (k / f) for k, f in zip(ker, ref)]))
    assert len(rows) >= 10 + 15
    for name, k, f in zip("EgH", ker, ref):
        assert k <= 2 * f, (name, k, f)


def test_h_is_bitwise_symmetric_and_positive_semidefinite(accuracy_rows):
    for r in accuracy_rows:
        H = r["kernel"][0]
        assert np.array_equal(H, np.swapaxes(H, 1, 2)), r["name"]
        for b in range(len(H)):
            lo = np.linalg.eigvalsh(H[b]).min()
            assert lo >= -1e-12 * np.diagonal(H[b]).max(), (r["name"], b, lo)


def test_clamp_masks_zero_rows_columns_and_g_entries():
    ex, labels = example()
    idx = [0, 1, 2]
    p = labels[idx].copy()
    outside = [(0, 0, 1.2), (1, 3, 0.05), (2, 6, -0.1), (2, 2, 0.01)]  # a0 above, e1 below, t1 below, a2 below
    on_bound = [(0, 1, 1.0), (1, 4, np.float32(0.1)), (2, 5, 0.0), (0, 2, np.float32(0.05))]
    for b, i, v in outside + on_bound:
        p[b, i] = v
    H, g, E = _kernel(ex[idx], p, 32)
    assert (E > 0).all()
    for b, i, _ in outside:
        assert not H[b, i, :].any() and not H[b, :, i].any() and g[b, i] == 0.0, (b, i)
    for b, i, _ in on_bound:  # the masks are inclusive
        assert H[b, i, i] > 0 and g[b, i] != 0.0, (b, i)
    free = np.ones((3, 12), bool)
    for b, i, _ in outside:
        free[b, i] = False
    assert (np.diagonal(H, axis1=1, axis2=2)[free] > 0).all()


def test_zero_one_pixel_and_mixed_images():
    by = {c["name"]: c for c in golden_cases()}
    z = by["zero_R32"]
    H, g, E = _kernel(z["true"], z["pred"], 32)
    assert not H.any() and not g.any() and not E.any()  # exact zeros, not NaN
    o = by["onepix_R32"]
    H, g, E = _kernel(o["true"], o["pred"], 32)
    assert (E > 0).all()
    for b in range(len(E)):  # one point: H = J^T J of a single row
        ev = np.linalg.eigvalsh(H[b])
        assert ev[-1] > 0 and np.abs(ev[:-1]).max() <= 1e-12 * ev[-1], ev
    mixed = o["true"].copy()
    mixed[1] = 0
    H2, g2, E2 = _kernel(mixed, o["pred"], 32)
    assert not H2[1].any() and not g2[1].any() and E2[1] == 0.0
    for b in (0, 2):  # one empty image in a batch leaves the other rows alone
        assert np.array_equal(H2[b], H[b]) and np.array_equal(g2[b], g[b]) and E2[b] == E[b]
    # a NaN pixel does not count: the same as a zero there
    c = by["noisy_R32"]
    holes, nans = c["true"].copy(), c["true"].copy()
    holes[:, :, 96:160, 64:128] = 0
    nans[:, :, 96:160, 64:128] = np.nan
    assert all(np.array_equal(x, y) for x, y in zip(_kernel(holes, c["pred"], 32), _kernel(nans, c["pred"], 32)))


def test_energy_is_the_loss_kernels_and_g_is_half_its_gradient():
    """The two kernels share the point rule and the Jacobian: E is least_squares' per-sample energy and 2 g its
    gradient.  Both sum float32 per-point terms good to about 1e-6 each (a dozen roundings and two
    approximate transcendentals); the sums cancel, so the bound is 1e-4 of the largest gradient entry."""
    from sqr import losses
    c = golden_cases()[3]
    t = torch.tensor(c["true"], device=DEV)
    p = torch.tensor(c["pred"], device=DEV, requires_grad=True)
    e = losses.least_squares(t, p, c["R"], per_sample=True)
    e.sum().backward()
    H, g, E = _kernel(c["true"], c["pred"], c["R"])
    np.testing.assert_allclose(E, e.detach().cpu().numpy(), rtol=1e-6)
    gl = p.grad.cpu().numpy().astype(np.float64)
    for b in range(len(E)):
        assert np.abs(2 * g[b] - gl[b]).max() <= 1e-4 * np.abs(gl[b]).max(), b


def test_runs_are_bitwise_equal_and_samples_independent():
    c = _shape_cases()[8]  # R32_32x32_B3
    a, b = _kernel(c["true"], c["pred"], c["R"]), _kernel(c["true"], c["pred"], c["R"])
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for i in range(3):
        one = _kernel(c["true"][i:i + 1], c["pred"][i:i + 1], c["R"])
        assert all(np.array_equal(x[0], y[i]) for x, y in zip(one, a)), i


GUARD = 64


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all())


@pytest.mark.parametrize("R,H,W,B", [(8, 16, 16, 3), (32, 32, 32, 2), (12, 24, 40, 3)])
def test_c_abi_writes_inside_its_buffers_only(R, H, W, B):
    """Guard words around every output and the workspace of sqr_least_squares_normal_eq and
    sqr_lsq_lm_refine, each given exactly the bytes its _workspace_bytes asks for."""
    from sqr._lib import lib, ptr, stream_ptr
    L = lib()
    ex, labels = example()
    idx = np.arange(B) % 10
    p = torch.tensor(labels[idx] + np.float32(0.03), device=DEV)
    t = torch.tensor(_resample(ex, idx, H, W)[:, 0], device=DEV).contiguous()
    wsb = L.sqr_least_squares_normal_eq_workspace_bytes(B, R)
    assert wsb == B * ((R * R + 255) // 256) * 256 * 8
    hb, Hm = _guarded(B * 144, torch.float64, -7.25)
    gb, g = _guarded(B * 12, torch.float64, -7.25)
    eb, E = _guarded(B, torch.float64, -7.25)
    wb, ws = _guarded(wsb, torch.uint8, 0xA5)
    rc = L.sqr_least_squares_normal_eq(ptr(p), ptr(t), B, H, W, R, ptr(Hm), ptr(g), ptr(E), ptr(ws), wsb, stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == 0, L.sqr_last_error_string()
    assert _guards_intact(hb, B * 144, -7.25) and _guards_intact(gb, B * 12, -7.25)
    assert _guards_intact(eb, B, -7.25) and _guards_intact(wb, wsb, 0xA5)
    assert torch.isfinite(Hm).all() and (Hm != -7.25).all() and (E > 0).all()
    assert L.sqr_least_squares_normal_eq(ptr(p), ptr(t), B, H, W, R, ptr(Hm), ptr(g), ptr(E), ptr(ws), wsb - 1,
                                         stream_ptr(DEV)) == -3
    assert b"workspace" in L.sqr_last_error_string()
    # the refinement
    wsb = L.sqr_lsq_lm_refine_workspace_bytes(B, R)
    ob, out = _guarded(B * 12, torch.float32, -7.25)
    bb, before = _guarded(B, torch.float64, -7.25)
    ab, after = _guarded(B, torch.float64, -7.25)
    cb, acc = _guarded(B, torch.int32, -7)
    wb, ws = _guarded(wsb, torch.uint8, 0xA5)
    rc = L.sqr_lsq_lm_refine(ptr(p), ptr(t), B, H, W, R, 3, 1e-3, 10.0, 0.1, ptr(out), ptr(before), ptr(after),
                             ptr(acc), ptr(ws), wsb, stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == 0, L.sqr_last_error_string()
    assert _guards_intact(ob, B * 12, -7.25) and _guards_intact(bb, B, -7.25) and _guards_intact(ab, B, -7.25)
    assert _guards_intact(cb, B, -7) and _guards_intact(wb, wsb, 0xA5)
    assert torch.isfinite(out).all() and (after <= before).all() and (acc >= 0).all() and (acc <= 3).all()
    assert L.sqr_lsq_lm_refine(ptr(p), ptr(t), B, H, W, R, 3, 1e-3, 10.0, 0.1, ptr(out), ptr(before), ptr(after),
                               ptr(acc), ptr(ws), wsb - 1, stream_ptr(DEV)) == -1
    assert b"workspace" in L.sqr_last_error_string()


# ------------------------------------------------------------------------------------------ the step kernel
def _step(accept, solve, up, down, p, H, g, E, lam, pt=None, Ht=None, gt=None, Et=None):
    """sqr_lsq_lm_step on float64 numpy inputs -> dict of the state after it (numpy)."""
    from sqr._lib import lib, ptr, stream_ptr
    L = lib()
    B = len(E)
    dev = lambda x, dt: torch.tensor(np.asarray(x), dtype=dt, device=DEV).contiguous()  # noqa: E731
    s = dict(p=dev(p, torch.float32), H=dev(H, torch.float64), g=dev(g, torch.float64), E=dev(E, torch.float64),
             lam=dev(lam, torch.float64), pt=dev(p if pt is None else pt, torch.float32),
             Ht=dev(H if Ht is None else Ht, torch.float64), gt=dev(g if gt is None else gt, torch.float64),
             Et=dev(E if Et is None else Et, torch.float64),
             delta=torch.full((B, 12), -7.25, dtype=torch.float64, device=DEV),
             accepted=torch.zeros(B, dtype=torch.int32, device=DEV))
    rc = L.sqr_lsq_lm_step(B, accept, solve, up, down, ptr(s["p"]), ptr(s["H"]), ptr(s["g"]), ptr(s["E"]),
                           ptr(s["lam"]), ptr(s["pt"]), ptr(s["Ht"]), ptr(s["gt"]), ptr(s["Et"]), ptr(s["delta"]),
                           ptr(s["accepted"]), stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == 0, L.sqr_last_error_string()
    return {k: v.cpu().numpy() for k, v in s.items()}


def test_step_solve_backward_error_and_free_set():
    rng = np.random.default_rng(7)
    zeroed = [(), (2, 7), (0, 5, 11), tuple(range(1, 12))]
    lams = [1e-6, 1e-3, 1.0, 1e3]
    Hs, gs, ls, frees = [], [], [], []
    for z in zeroed:
        for lam in lams:
            A = rng.normal(size=(20, 12)) * np.exp(rng.normal(size=12))  # columns of different scales
            H = A.T @ A
            H[list(z), :] = 0
            H[:, list(z)] = 0
            Hs.append(H)
            gs.append(rng.normal(size=12))  # also off the free set: delta must be 0 there whatever g is
            ls.append(lam)
            frees.append(np.array([i not in z for i in range(12)]))
    B = len(Hs)
    p = np.tile(np.array([.5, .5, .5, .5, .5, .5, .5, .5, 0, 0, 0, 1], np.float32), (B, 1))
    out = _step(0, 1, 10.0, 0.1, p, np.stack(Hs), np.stack(gs), np.ones(B), np.array(ls))
    worst = 0.0
    for b in range(B):
        f, d = frees[b], out["delta"][b]
        assert not d[~f].any(), b  # exactly 0 off the free set
        assert np.isfinite(d).all() and d[f].all(), b
        M = (Hs[b] + ls[b] * np.diag(np.diagonal(Hs[b])))[f][:, f]
        res = np.abs(M @ d[f] + gs[b][f]).max()
        bwd = res / (np.abs(M).sum(1).max() * np.abs(d[f]).max() + np.abs(gs[b][f]).max())
        worst = max(worst, bwd)
        assert bwd <= 1e-13, (b, bwd)
        assert out["lam"][b] == ls[b]  # solved: lambda untouched
    print("worst normwise backward error %.2e" % worst)
    # the new trial is project(p + delta), stored as float32
    x = p.astype(np.float64) + out["delta"]
    want = np.concatenate([np.clip(x[:, 0:3], np.float32(0.05), 1), np.clip(x[:, 3:5], np.float32(0.1), 1),
                           np.clip(x[:, 5:8], 0, 1)], 1).astype(np.float32)
    np.testing.assert_array_equal(out["pt"][:, :8], want)
    qn = np.linalg.norm(out["pt"][:, 8:].astype(np.float64), axis=1)
    assert np.abs(qn - 1).max() <= 1e-6
    np.testing.assert_array_equal(out["p"], p)  # the current parameters stay


def test_step_failed_pivot_gives_zero_delta_and_raises_lambda():
    H = np.zeros((3, 12, 12))
    H[0] = np.eye(12)
    H[0, 0, 1] = H[0, 1, 0] = 5.0  # indefinite: the second pivot is negative
    H[1] = np.eye(12)
    H[1, 3, 4] = H[1, 4, 3] = np.nan  # not finite
    H[2] = np.eye(12)  # fine
    p = np.tile(np.array([.5, .5, .5, .5, .5, .5, .5, .5, 0, 0, 0, 2], np.float32), (3, 1))
    out = _step(0, 1, 10.0, 0.1, p, H, np.ones((3, 12)), np.ones(3), np.full(3, 1e-3))
    assert not out["delta"][:2].any() and out["delta"][2].all()
    assert out["lam"].tolist() == [1e-3 * 10.0, 1e-3 * 10.0, 1e-3]
    np.testing.assert_array_equal(out["pt"][:2, :8], p[:2, :8])
    np.testing.assert_array_equal(out["pt"][:2, 8:], np.array([[0, 0, 0, 1]] * 2, np.float32))  # q normalised


def test_step_accept_logic_and_lambda_clamps():
    B = 6
    rng = np.random.default_rng(3)
    p, pt = rng.random((B, 12)).astype(np.float32), rng.random((B, 12)).astype(np.float32)
    H, Ht = rng.random((B, 12, 12)), rng.random((B, 12, 12))
    g, gt = rng.random((B, 12)), rng.random((B, 12))
    E = np.ones(B)
    Et = np.array([0.5, 1.0, 2.0, np.nan, 0.5, 2.0])
    lam = np.array([1e-3, 1e-3, 1e-3, 1e-3, 1e-12, 1e12])
    out = _step(1, 0, 10.0, 0.1, p, H, g, E, lam, pt, Ht, gt, Et)
    took = np.array([True, False, False, False, True, False])
    for b in range(B):
        src = (pt, Ht, gt, Et) if took[b] else (p, H, g, E)
        for k, s in zip(("p", "H", "g", "E"), src):
            assert np.array_equal(out[k][b], s[b]), (b, k)
    assert out["accepted"].tolist() == took.astype(int).tolist()
    # E_t < E: lambda * down; E_t >= E and E_t = NaN: lambda * up; both clamps reached
    assert out["lam"].tolist() == [1e-3 * 0.1, 1e-3 * 10.0, 1e-3 * 10.0, 1e-3 * 10.0, 1e-12, 1e12]
    assert (out["delta"] == -7.25).all()  # no solve: untouched
    np.testing.assert_array_equal(out["pt"], pt)


# ------------------------------------------------------------------------------------------ the loop
def _project_np(p):
    """project() of the start in numpy: a, e, t clamped (float32), q / |q| in float64."""
    p = np.asarray(p, np.float32)
    q = p[:, 8:].astype(np.float64)
    n = np.sqrt((q * q).sum(1, keepdims=True))
    q = np.where((n > 0) & np.isfinite(n), q / np.where(n > 0, n, 1), q)
    return np.concatenate([np.clip(p[:, 0:3], np.float32(0.05), 1), np.clip(p[:, 3:5], np.float32(0.1), 1),
                           np.clip(p[:, 5:8], 0, 1), q.astype(np.float32)], 1).astype(np.float32)


def _assert_projected_start(out, start):
    want = _project_np(start)
    np.testing.assert_array_equal(out[:, :8], want[:, :8])
    # q / |q| rounds once to float32 from float64 operands that may differ in their last bit
    np.testing.assert_allclose(out[:, 8:], want[:, 8:], rtol=0, atol=2.0 ** -23)


@pytest.fixture(scope="module")
def loop_run():
    """refine_lm on the ten example images at 256x256, R = 32, from the label, 10 iterations; the float64
    and float32 plain-torch loops on the same.  Computed once."""
    from sqr import fit
    ex, labels = example()
    img, p0 = torch.tensor(ex, device=DEV), torch.tensor(labels, device=DEV)
    out, before, after, accepted = fit.refine_lm(img, p0, iters=10, render_size=32, return_info=True)
    torch.cuda.synchronize()
    assert torch.equal(p0, torch.tensor(labels, device=DEV))  # the input is left alone
    assert out.dtype == torch.float32 and out.shape == (10, 12) and not out.requires_grad
    assert before.dtype == after.dtype == torch.float64 and accepted.dtype == torch.int32
    ref = {}
    for dt in (torch.float64, torch.float32):
        pts = _lm_ref.points_of(ex, 32, dt)
        ref[dt] = [_lm_ref.lm_loop(pts[i], labels[i], iters=10, dt=dt) for i in range(10)]
    return dict(img=img, p0=p0, out=out, before=before, after=after, accepted=accepted, ref=ref)


def test_loop_descends_and_returns_valid_parameters(loop_run):
    out, before, after = loop_run["out"].cpu().numpy(), loop_run["before"].cpu().numpy(), loop_run["after"].cpu().numpy()
    acc = loop_run["accepted"].cpu().numpy()
    for i in range(10):
        print("image %d: %.6g -> %.6g (%.3f), %d accepted" % (i, before[i], after[i], after[i] / before[i], acc[i]))
    assert np.isfinite(out).all() and np.isfinite(before).all() and np.isfinite(after).all()
    assert (after <= before).all()  # exact: both come from the same kernel
    assert (after <= 0.5 * before).all(), after / before
    assert (out[:, 0:3] >= np.float32(0.05)).all() and (out[:, 0:3] <= 1).all()
    assert (out[:, 3:5] >= np.float32(0.1)).all() and (out[:, 3:5] <= 1).all()
    assert (out[:, 5:8] >= 0).all() and (out[:, 5:8] <= 1).all()
    assert np.abs(np.linalg.norm(out[:, 8:].astype(np.float64), axis=1) - 1).max() <= 1e-6
    assert (acc >= 1).all() and (acc <= 10).all()
    # the energies are the normal-equations kernel's at the projected start and at the result
    from sqr import losses
    _, _, e1 = losses.least_squares_normal_eq(loop_run["img"], loop_run["out"], 32)
    assert torch.equal(e1, loop_run["after"])
    start = torch.tensor(_project_np(loop_run["p0"].cpu().numpy()), device=DEV)
    _, _, e0 = losses.least_squares_normal_eq(loop_run["img"], start, 32)
    np.testing.assert_allclose(before, e0.cpu().numpy(), rtol=1e-5)


def test_loop_final_energy_vs_float64_loop(loop_run):
    """Accept decisions may differ between precisions, so no trajectory is compared: per image the final
    energy over the float64 loop's (at least 1) within twice the worst such ratio of the float32 loop.
    Measured on MI355X: kernel 1.0000 at worst, float32 plain-torch loop 1.0001."""
    after = loop_run["after"].cpu().numpy()
    e64 = np.array([r[2] for r in loop_run["ref"][torch.float64]])
    e32 = np.array([r[2] for r in loop_run["ref"][torch.float32]])
    rk, r32 = np.maximum(after / e64, 1), np.maximum(e32 / e64, 1)
    for i in range(10):
        print("image %d: float64 %.6g | float32 torch %.6g (%.4f) | kernel %.6g (%.4f)"
              % (i, e64[i], e32[i], e32[i] / e64[i], after[i], after[i] / e64[i]))
    print("worst ratio: float32 torch %.4f kernel %.4f" % (r32.max(), rk.max()))
    assert (rk <= 2 * r32.max()).all(), (rk, r32.max())


def test_loop_batch_independence_and_repeatability(loop_run):
    from sqr import fit
    again = fit.refine_lm(loop_run["img"], loop_run["p0"], iters=10, render_size=32, return_info=True)
    for x, k in zip(again, ("out", "before", "after", "accepted")):
        assert torch.equal(x, loop_run[k]), k
    for i in range(10):
        one = fit.refine_lm(loop_run["img"][i:i + 1], loop_run["p0"][i:i + 1], iters=10, render_size=32, return_info=True)
        for x, k in zip(one, ("out", "before", "after", "accepted")):
            assert torch.equal(x[0], loop_run[k][i]), (i, k)


def test_loop_zero_iterations_returns_the_projected_start(loop_run):
    from sqr import fit
    start = (loop_run["p0"].cpu().numpy() + 0.3 * np.random.default_rng(1).normal(size=(10, 12))).astype(np.float32)
    out, before, after, acc = fit.refine_lm(loop_run["img"], torch.tensor(start, device=DEV), iters=0, return_info=True)
    _assert_projected_start(out.cpu().numpy(), start)
    assert torch.equal(before, after) and (before > 0).all() and not acc.any()


def test_loop_on_an_empty_image(loop_run):
    from sqr import fit
    img = loop_run["img"].clone()
    img[4] = 0
    start = (loop_run["p0"].cpu().numpy() + np.float32(0.1)).astype(np.float32)
    out, before, after, acc = fit.refine_lm(img, torch.tensor(start, device=DEV), iters=10, return_info=True)
    _assert_projected_start(out[4:5].cpu().numpy(), start[4:5])
    assert before[4].item() == 0.0 and after[4].item() == 0.0 and acc[4].item() == 0
    assert torch.isfinite(out).all() and torch.isfinite(before).all() and torch.isfinite(after).all()
    assert (after <= before).all() and (before[[0, 1, 2, 3, 5, 6, 7, 8, 9]] > 0).all()


def test_loop_captured_in_a_graph_replays_bitwise(loop_run):
    from sqr import fit
    img, p = loop_run["img"].clone(), loop_run["p0"].clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = fit.refine_lm(img, p, iters=10, render_size=32, return_info=True)
    shifted = (loop_run["p0"] + 0.02).contiguous()
    eager_shifted = fit.refine_lm(img, shifted, iters=10, render_size=32, return_info=True)
    for src, want in ((loop_run["p0"], [loop_run[k] for k in ("out", "before", "after", "accepted")]),
                      (shifted, eager_shifted)):
        p.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(res, want))


def test_refine_method_lm_is_refine_lm(loop_run):
    from sqr import fit
    res = fit.refine(loop_run["img"], loop_run["p0"], steps=10, method="lm")
    assert len(res) == 3
    for x, k in zip(res, ("out", "before", "after")):
        assert torch.equal(x, loop_run[k]), k


def test_test_py_refine_method_lm(tmp_path, capsys):
    """test.py --refine 5 --refine-method lm on an example image (random weights: no checkpoint needed)."""
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
    spec = importlib.util.spec_from_file_location("sq_test_py_lm", os.path.join(PKG, "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(0)
    a, e, t, q = mod.main(["--image", str(bmp), "--model", str(tmp_path / "none.pt"), "--device", DEV,
                           "--refine", "5", "--refine-method", "lm"])
    out = capsys.readouterr().out
    m = re.search(r"Refined parameters \(5 Levenberg-Marquardt iterations, LeastSquares energy (\S+) -> (\S+)\):", out)
    assert m, out
    assert float(m.group(2)) <= float(m.group(1))
    assert out.count("Size a:") == 2
    assert a.shape == (1, 3) and e.shape == (1, 2) and t.shape == (1, 3) and q.shape == (1, 4)
    assert all(np.isfinite(v).all() for v in (a, e, t, q))
    assert abs(np.linalg.norm(q.astype(np.float64)) - 1) <= 1e-6
