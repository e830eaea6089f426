"""tests/_loss_ref.py against oracle/sq_oracle.py, and the two numerical edges the loss kernels' tests rest on.

No GPU.  What tests/test_loss_kernels_gpu.py takes for granted is checked here:

  * the float64 block moments pushed through _loss_ref.finalize are sq_oracle's loss, per-sample loss and
    gradient to 1e-12 (loss: relative; gradient: of the sample's largest entry), on the shape tables of
    _loss_ref and on the golden cases;
  * the dyadic rows fire the zero fix (classes.py:261-263) on three whole planes, and the fix matters;
  * np.arange's extra node at R = 6 and 9;
  * the float32 evaluation is finite, and its error against float64 (the scale of the GPU tests'
    tolerances) is printed: `loss_stages_accuracy ...` lines, kept in profiles/loss_stages_accuracy.txt.
"""
import math

import numpy as np
import pytest

import _loss_ref as L
import sq_oracle as O
from _golden import cases as _golden
from _loss_ref import COMPONENTS, SLOTS, edge_cases


def _close_to_oracle(fin, Lo, lo, Go, pred):
    assert abs(fin["mean"] - Lo) <= 1e-12 * abs(Lo)
    assert np.abs(fin["loss"] - lo).max() <= 1e-12 * np.abs(lo).max()
    for b in range(len(Go)):
        # a row clamped from below divides by the bound: finalize has the kernel's (and the reference's) fp32
        # 0.05f, sq_oracle the float64 0.05, 2^-26 apart (only a is divided by in the finalize)
        tol = 2.0 ** -24 if (np.asarray(pred[b][:3]) < np.float32(0.05)).any() else 1e-12
        assert np.abs(fin["grad"][b] - Go[b]).max() <= tol * np.abs(Go[b]).max(), b


def _implicit_vs_oracle(c):
    R, B, tau, s = int(c["R"]), len(c["pred"]), float(c["tau"]), float(c["s"])
    ref = L.implicit_block_moments(c["true"], c["pred"], R, tau, s)
    assert ref["part"].shape == (B, L.implicit_nblk(R), 18)
    fin = L.finalize(ref["part"], c["pred"], *L.implicit_scales(B, R))
    Lo, Go, lo, imgs = O.implicit_loss(c["true"], c["pred"], R, tau, s)
    _close_to_oracle(fin, Lo, lo, Go, c["pred"])
    assert np.array_equal(ref["D"], imgs)
    return ref, fin, Go


def _explicit_vs_oracle(c):
    R, B = int(c["R"]), len(c["pred"])
    ref = L.explicit_block_moments(c["true"], c["pred"], R)
    assert ref["part"].shape == (B, L.explicit_nblk(R), 18)
    fin = L.finalize(ref["part"], c["pred"], *L.explicit_scales(B, R))
    Lo, Go, lo = O.explicit_loss(c["true"], c["pred"], R)
    _close_to_oracle(fin, Lo, lo, Go, c["pred"])
    return ref, fin, Go


def _print(kind, name, what, names, values):
    print("loss_stages_accuracy %-8s %-22s %-9s %s" % (kind, name, what,
                                                      " ".join("%s=%.2e" % kv for kv in zip(names, values))))


@pytest.mark.parametrize("shape", L.IMPLICIT_SHAPES, ids=lambda s: "R%d_%dx%d_B%d" % s)
def test_implicit_shapes_reproduce_oracle_and_f32_errors(shape):
    c = L.implicit_case(*shape)
    R, B = c["R"], c["B"]
    assert np.array_equal(L.resized_target(c["true"], R).shape, (B, R, R))
    ref, fin, Go = _implicit_vs_oracle(c)
    # every ray's sign is safe against fp32 (the target is D + s d rounded to fp32), and both signs occur
    assert ref["margin"] >= 0.01 - 2.0 ** -24
    sg = np.sign(ref["D"] - L.resized_target(c["true"], R))
    assert (sg > 0).any() and (sg < 0).any()
    if B == 3:
        assert ref["n_fixed"].tolist() == [3 * R * R] * 3
    # the gradient slots are not all underflow (R = 2: no node of the grid is near any row's surface)
    carry = ref["abs"][..., :17].max((0, 1))
    assert (carry >= L.CARRY).all() if R > 2 else (carry < L.FLOOR).all()
    p32 = L.implicit_f32(c["true"], c["pred"], R, c["tau"], c["s"])
    assert p32.dtype == np.float32 and p32.shape == ref["part"].shape and np.isfinite(p32).all()
    _print("implicit", c["name"], "f32_slot", SLOTS, L.slot_errors(p32, ref, L.FLOOR))
    g32 = L.finalize(p32, c["pred"], *L.implicit_scales(B, R))["grad"]
    assert np.isfinite(g32).all()
    if B != 3 and R > 2:
        _print("implicit", c["name"], "f32_grad", COMPONENTS, L.component_errors(g32, Go))


@pytest.mark.parametrize("R", L.EXPLICIT_R)
def test_explicit_sizes_reproduce_oracle_and_f32_errors(R):
    c = L.explicit_case(R)
    ref, fin, Go = _explicit_vs_oracle(c)
    assert ref["n"] == {1: 2, 4: 5, 6: 8, 9: 11, 15: 16, 16: 17}[R]
    if R == 4:
        assert ref["n_fixed"].tolist() == [3 * 25] * 3
    assert (ref["abs"].max((0, 1)) >= L.CARRY_EXPLICIT).all()
    p32 = L.explicit_f32(c["true"], c["pred"], R)
    assert p32.dtype == np.float32 and p32.shape == ref["part"].shape and np.isfinite(p32).all()
    _print("explicit", c["name"], "f32_slot", SLOTS, L.slot_errors(p32, ref, L.FLOOR_EXPLICIT))
    g32 = L.finalize(p32, c["pred"], *L.explicit_scales(c["B"], R))["grad"]
    assert np.isfinite(g32).all()
    if R != 4:
        _print("explicit", c["name"], "f32_grad", COMPONENTS, L.component_errors(g32, Go))


@pytest.mark.parametrize("case", _golden("implicit_loss.npz") + edge_cases("implicit"), ids=lambda c: str(c["name"]))
def test_implicit_golden_cases_reproduce_oracle(case):
    _implicit_vs_oracle(case)


@pytest.mark.parametrize("case", _golden("explicit_loss.npz") + edge_cases("explicit"), ids=lambda c: str(c["name"]))
def test_explicit_golden_cases_reproduce_oracle(case):
    _explicit_vs_oracle(case)


def test_edge_fixture_is_the_oracles_too():
    """loss_edges.npz (the reference's own classes.py) against sq_oracle at the suite's tolerances, so a
    kernel that misses the fixture misses the oracle as well."""
    for c in edge_cases("implicit"):
        Lo, Go, _, imgs = O.implicit_loss(c["true"], c["pred"], int(c["R"]), float(c["tau"]), float(c["s"]))
        assert abs(Lo - float(c["loss"])) <= 1e-6 * abs(Lo)
        assert np.abs(imgs - c["depth"]).max() <= 1e-6
        for b in range(3):
            assert np.abs(Go[b] - c["grad"][b]).max() <= 1e-6 * np.abs(Go[b]).max()
    for c in edge_cases("explicit"):
        Lo, Go, _ = O.explicit_loss(c["true"], c["pred"], int(c["R"]))
        assert abs(Lo - float(c["loss"])) <= 1e-6 * abs(Lo)
        for b in range(len(Go)):
            assert np.abs(Go[b] - c["grad"][b]).max() <= 1e-6 * np.abs(Go[b]).max()
    for c in edge_cases("iou"):
        assert np.array_equal(O.iou_counts(c["true"], c["pred"], int(c["R"])), c["counts"])
        assert (c["counts"][:, 1] > c["counts"][:, 0]).all() and (c["counts"][:, 0] > 0).all()


@pytest.mark.parametrize("R", [5, 9, 17])
def test_dyadic_rows_fire_the_zero_fix_and_it_matters(R):
    """Against an all-zero target (loss = mean depth, every ray's sign the same), at tau 1.5, sharpness 260."""
    c = dict(pred=L.dyadic_rows(), true=np.zeros((3, 1, R, R), np.float32), tau=L.TAU, s=L.SHARP)
    axis = O.implicit_axis(R)
    assert all(float(v) in axis for v in (0.5, 0.25, 0.75))       # the centre is a grid node
    on = L.implicit_block_moments(c["true"], c["pred"], R, c["tau"], c["s"])
    off = L.implicit_block_moments(c["true"], c["pred"], R, c["tau"], c["s"], zero_fix=False)
    assert on["n_fixed"].tolist() == [3 * R * R] * 3             # the planes x = .5, y = .25 and z = .75
    scales = L.implicit_scales(3, R)
    f_on, f_off = L.finalize(on["part"], c["pred"], *scales), L.finalize(off["part"], c["pred"], *scales)
    rel = abs(f_on["loss"][0] - f_off["loss"][0]) / f_on["loss"][0]   # row 0: e = (1, 1)
    pix = np.abs(on["D"][0] - off["D"][0]).max()
    print("loss_stages_accuracy zero_fix R=%d loss_change=%.3e depth_change=%.3e" % (R, rel, pix))
    assert rel >= 3e-4
    assert pix >= 5e-3
    assert np.isfinite(f_on["grad"]).all() and (f_on["grad"][:, :5] != 0).all()   # (dL/dt0 is 0 by symmetry)
    assert not np.isfinite(f_off["grad"][0]).all()               # without the fix: 0 * log(0)


def test_arange_returns_an_extra_node_at_6_and_9():
    assert O.explicit_axis(6).size == 8 and O.explicit_axis(9).size == 11
    assert O.explicit_axis(6)[-1] > 1 and O.explicit_axis(9)[-1] > 1
    assert [O.explicit_axis(R).size for R in (1, 4, 8, 15, 16, 32, 64)] == [2, 5, 9, 16, 17, 33, 65]
    extra = [R for R in range(1, 1025) if O.explicit_axis(R).size == R + 2]
    assert len(extra) == 174 and extra[:5] == [6, 9, 21, 24, 28]
    for R in range(1, 1025):      # the kernel's restatement of len(np.arange(0, 1 + 1/R, 1/R))
        step = 1.0 / R
        assert math.ceil((1.0 + step) / step) == O.explicit_axis(R).size == L.explicit_n(R), R


@pytest.mark.parametrize("B", [1, 64, 65, 1024, 1025, 2500])
def test_loss_mean_restatement_is_a_mean(B):
    v = np.random.default_rng(B).uniform(0.1, 1.0, B)
    m = L.loss_mean(v, B)
    assert abs(m - math.fsum(v) / B) <= 4 * 2.0 ** -53 * math.log2(B + 1) * m + 1e-300
    if B == 1:
        assert m == v[0]


def test_finalize_masks_and_quaternion_scale():
    """Inclusive clamp masks, and an un-normalised quaternion is used as it is (sq_oracle does the same)."""
    rng = np.random.default_rng(5)
    p = L.sample(rng, 4)
    p[0, 0], p[0, 3], p[0, 5] = 0.05, 0.1, 0.0            # on the lower bounds
    p[1, 1], p[1, 4], p[1, 7] = 1.0, 1.0, 1.0             # on the upper bounds
    p[2, 0], p[2, 3], p[2, 6], p[2, 2], p[2, 4] = np.nextafter(np.float32(0.05), np.float32(0)), 0.05, -0.2, 1.3, 1.2
    p[3, 8:] *= 1.3
    true = L.signed_target(p, 16, 16, 16, rng)
    ref = L.implicit_block_moments(true, p, 16, L.TAU, L.SHARP)
    fin = L.finalize(ref["part"], p, *L.implicit_scales(4, 16))
    Lo, Go, lo, _ = O.implicit_loss(true, p, 16, L.TAU, L.SHARP)
    _close_to_oracle(fin, Lo, lo, Go, p)
    zero = fin["grad"] == 0
    assert zero[2, [0, 3, 6, 2, 4]].all() and zero.sum() == 5
    assert (fin["chain"] >= np.abs(fin["grad"])).all()
