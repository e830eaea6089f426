"""Levenberg-Marquardt refinement, the parts that need no GPU: the C ABI is declared and bound, its
argument checks run on the host before any launch, sqr.fit.refine rejects an unknown method, and the
float64 reference loop (tests/_lm_ref.py) alone meets the cap the GPU test sets."""
import ctypes

import numpy as np
import pytest
import torch

from _lsq_cases import example
from test_capi import declared_symbols

NEW = ("sqr_least_squares_normal_eq_workspace_bytes", "sqr_least_squares_normal_eq", "sqr_lsq_lm_step",
       "sqr_lsq_lm_refine_workspace_bytes", "sqr_lsq_lm_refine")


def test_header_and_signatures_are_present():
    from sqr import _lib
    syms = declared_symbols()
    L = _lib.lib()
    for s in NEW:
        assert s in syms and s in _lib.SIGNATURES and hasattr(L, s), s
    # 16 x 16 float64 per block of 256 pixels; the refinement adds its two states, delta and the trial
    assert L.sqr_least_squares_normal_eq_workspace_bytes(3, 32) == 3 * 4 * 256 * 8
    assert L.sqr_least_squares_normal_eq_workspace_bytes(3, 8) == 3 * 1 * 256 * 8
    assert L.sqr_lsq_lm_refine_workspace_bytes(3, 32) == 3 * 326 * 8 + 3 * 4 * 256 * 8 + 3 * 12 * 4
    assert L.sqr_lsq_lm_refine_workspace_bytes(0, 32) == 0


def _refine(L, B=2, H=64, W=64, R=32, iters=10, lambda0=1e-3, up=10.0, down=0.1, ws_bytes=None):
    """sqr_lsq_lm_refine with host buffers standing in for device ones: every call here must be refused
    before the first launch, so none is ever read."""
    bufs = [(ctypes.c_double * 4096)() for _ in range(7)]
    p = [ctypes.cast(b, ctypes.c_void_p) for b in bufs]
    need = L.sqr_lsq_lm_refine_workspace_bytes(B, R) if B > 0 and R > 0 else 0
    return L.sqr_lsq_lm_refine(p[0], p[1], B, H, W, R, iters, lambda0, up, down, p[2], p[3], p[4], p[5], p[6],
                               need if ws_bytes is None else ws_bytes, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(B=0), b"B=0"),
    (dict(B=-3), b"B=-3"),
    (dict(R=0), b"R=0"),
    (dict(iters=-1), b"iters=-1"),
    (dict(lambda0=0.0), b"lambda0=0"),
    (dict(lambda0=-1.0), b"lambda0=-1"),
    (dict(up=1.0), b"up=1"),
    (dict(down=0.0), b"down=0"),
    (dict(down=1.0), b"down=1"),
    (dict(ws_bytes=15), b"workspace"),
])
def test_refine_rejects_bad_arguments_on_the_host(kw, msg):
    from sqr import _lib
    L = _lib.lib()
    assert _refine(L, **kw) == -1
    err = L.sqr_last_error_string()
    assert err.startswith(b"lsq_lm_refine:") and msg in err, err


def test_normal_eq_and_step_reject_bad_arguments_on_the_host():
    from sqr import _lib
    L = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.sqr_least_squares_normal_eq(p, p, 0, 8, 8, 8, p, p, p, p, 1 << 20, None) == -1
    assert b"B=0" in L.sqr_last_error_string()
    assert L.sqr_least_squares_normal_eq(p, p, 1, 8, 8, 8, p, p, p, p, 2047, None) == -3
    assert b"workspace" in L.sqr_last_error_string()
    assert L.sqr_least_squares_normal_eq(p, p, 1, 8, 8, 8, None, p, p, p, 2048, None) == -1
    assert L.sqr_lsq_lm_step(1, 1, 1, 1.0, 0.1, p, p, p, p, p, p, p, p, p, p, p, None) == -1
    assert b"up=1" in L.sqr_last_error_string()
    assert L.sqr_lsq_lm_step(1, 1, 1, 10.0, 1.5, p, p, p, p, p, p, p, p, p, p, p, None) == -1
    assert b"down=1.5" in L.sqr_last_error_string()
    assert L.sqr_lsq_lm_step(1, 1, 0, 10.0, 0.1, p, p, p, p, p, p, p, p, None, None, p, None) == -1
    assert b"trial" in L.sqr_last_error_string()


def test_refine_rejects_an_unknown_method_and_cpu_tensors():
    from sqr import fit, losses
    img, p = torch.zeros(1, 1, 32, 32), torch.zeros(1, 12)
    with pytest.raises(ValueError, match="method"):
        fit.refine(img, p, steps=1, method="bogus")
    # CUDA only, like the other sqr.losses entry points
    with pytest.raises(ValueError, match="CPU tensor"):
        fit.refine(img, p, steps=1, method="lm")
    with pytest.raises(ValueError, match="CPU tensor"):
        fit.refine_lm(img, p)
    with pytest.raises(ValueError, match="CPU tensor"):
        losses.least_squares_normal_eq(img, p, 32)


def test_reference_jacobian_is_half_the_energy_gradient():
    """The helper against the class the project already pins: g = J^T r is half of autograd's dE/dparams
    of classes.LeastSquares' energy, E is that energy."""
    import classes
    import _lm_ref
    ex, labels = example()
    pts = _lm_ref.points_of(ex[3:4], 16, torch.float64)
    p = torch.tensor(labels[3] + np.float32(0.02), dtype=torch.float64, requires_grad=True)
    e = classes.LeastSquares(16, "cpu").energy_function(pts, p[None])[0]
    e.backward()
    H, g, E = _lm_ref.normal_eq_one(pts[0], p.detach())
    assert abs(E.item() - e.item()) <= 1e-14 * e.item()
    assert (2 * g - p.grad).abs().max().item() <= 1e-12 * p.grad.abs().max().item()
    assert torch.equal(H, H.T) or (H - H.T).abs().max().item() <= 1e-15 * H.diagonal().max().item()


def test_float64_reference_loop_meets_the_cap_from_the_label():
    """From the label at R = 32, 10 iterations: at most 0.5 of the start energy on each of the ten example
    images (measured: 0.257 at worst), so the GPU test's cap asks nothing the method does not give."""
    import _lm_ref
    ex, labels = example()
    pts = _lm_ref.points_of(ex, 32, torch.float64)
    worst = 0.0
    for i in range(10):
        p, before, after, accepted = _lm_ref.lm_loop(pts[i], labels[i], iters=10)
        print("image %d: %.6g -> %.6g (%.3f), %d accepted" % (i, before, after, after / before, accepted))
        assert after <= 0.5 * before and accepted >= 1, i
        q = p[8:12]
        assert abs(float(torch.sqrt((q * q).sum())) - 1) <= 1e-12
        worst = max(worst, after / before)
    print("worst ratio %.3f" % worst)
