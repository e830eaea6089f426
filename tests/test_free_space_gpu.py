"""The free-space energy on the GPU (sqr_lsq_free_space, sqr.losses.free_space_energy) against the float64 host
reference tests/_free_space_ref.py (a golden-section search on F itself: no derivative, no slab, nothing of
the kernel's procedure).

Tolerance.  Nothing is fixed in advance: the same host reference runs in float32, its worst deviation from the
float64 run over all cases is measured here, and the kernel may deviate twice that (the yardstick of
tests/test_scan_render_gpu.py).  Deviation of a sample: |E - E64| / (E64 + FLOOR).  FLOOR is the absolute floor
for exact zeros: a ray that grazes the model has F - 1 = 0 up to the rounding of F, 2^-24 amplified by the powers
(1 / e <= 10 on logarithms of up to 13 bits' worth: 2^-17), and may land on either side of 0 in another
precision; at most R^2 = 1089 rays with a0 a1 a2 <= 1 add up to 1089 x 2^-34 = 6e-8, rounded up to 1e-7.
Measured on an MI355X (profiles/free_space_accuracy.txt holds the printed lines): the float32 host reference
deviates by up to 2.0e-5, the kernel by up to 7.6e-6.
"""
import numpy as np
import pytest
import torch

import _free_space_ref as fsr
from _lsq_cases import build_images, example, golden_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 1e-7
MARGIN = 1.0 / 255.0


def _cases():
    """name, R, true [B,1,H,W], params [S,12] (S a multiple of B)."""
    ex, labels = example()
    out = []
    # the LeastSquares fixture's images and parameters at R = 32: labels, noisy labels, a raw 0..255 image,
    # parameters outside their clamps, a zero image, a one-pixel image, a 512 x 512 image
    for c in golden_cases():
        if c["R"] == 32:
            out.append(dict(name=c["name"], R=32, true=c["true"], params=np.asarray(c["pred"], np.float32)))
    rng = np.random.default_rng(11)
    noisy = (labels + 0.03 * rng.standard_normal(labels.shape)).astype(np.float32)
    big = labels.copy()
    big[:, 0:3] *= 1.6  # models that stick out of their images
    out.append(dict(name="examples_R32", R=32, true=ex, params=noisy))
    out.append(dict(name="examples_big_R32", R=32, true=ex, params=big))
    out.append(dict(name="examples_R33", R=33, true=ex[:5], params=big[:5]))  # R^2 = 1089: five blocks, the last partly
    out.append(dict(name="examples_R8", R=8, true=ex[5:], params=big[5:]))    # a quarter of a block
    rows, cols = np.arange(50) * 256 // 50, np.arange(37) * 256 // 37
    out.append(dict(name="resize_50x37_R32", R=32, true=np.ascontiguousarray(ex[[2, 6]][:, :, rows][:, :, :, cols]),
                    params=big[[2, 6]]))
    out.append(dict(name="zero_big_R32", R=32, true=build_images("zero", [3, 4, 5], ex), params=big[[3, 4, 5]]))
    holes = ex[[9, 0, 1]].copy()
    holes[:, :, 96:160, 64:128] = np.nan
    holes[1, :, :40, :] = np.nan
    out.append(dict(name="nanholes_R32", R=32, true=holes, params=big[[9, 0, 1]]))
    out.append(dict(name="margin_0.05_R32", R=32, true=ex[[9, 0, 1]], params=big[[9, 0, 1]], margin=0.05))
    out.append(dict(name="margin_0_R32", R=32, true=ex[[9, 0, 1]], params=big[[9, 0, 1]], margin=0.0))
    # S = 2 B: the [K,B] layout
    out.append(dict(name="stack_2x3_R32", R=32, true=ex[[1, 4, 8]], params=np.concatenate([big[[1, 4, 8]], noisy[[1, 4, 8]]])))
    return out


def _kernel(true, params, R, margin=MARGIN):
    from sqr import losses
    out = losses.free_space_energy(torch.tensor(true, device=DEV), torch.tensor(params, device=DEV), R, margin)
    torch.cuda.synchronize()
    assert out.dtype == torch.float64 and out.shape == (len(params),) and not out.requires_grad
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def rows():
    """Per case the kernel's, the float64 host's and the float32 host's energies.  Computed once."""
    out = []
    for c in _cases():
        m = c.get("margin", MARGIN)
        out.append(dict(c, ker=_kernel(c["true"], c["params"], c["R"], m),
                        h64=fsr.free_space(c["true"], c["params"], c["R"], m, torch.float64),
                        h32=fsr.free_space(c["true"], c["params"], c["R"], m, torch.float32)))
    return out


def _dev(e, e64):
    return np.abs(e - e64) / (e64 + FLOOR)


def test_free_space_vs_float64_reference(rows):
    worst32 = max(_dev(r["h32"], r["h64"]).max() for r in rows)
    worstk = 0.0
    for r in rows:
        d32, dk = _dev(r["h32"], r["h64"]), _dev(r["ker"], r["h64"])
        print("%-18s E64 %s | float32 host %.2e | kernel %.2e" % (
            r["name"], " ".join("%.3e" % v for v in r["h64"]), d32.max(), dk.max()))
        worstk = max(worstk, dk.max())
    print("worst deviation |E - E64| / (E64 + %.0e): float32 host %.3e, kernel %.3e (bound %.3e)"
          % (FLOOR, worst32, worstk, 2 * worst32))
    for r in rows:
        assert np.isfinite(r["ker"]).all() and (r["ker"] >= 0).all(), r["name"]
        assert (_dev(r["ker"], r["h64"]) <= 2 * worst32).all(), (r["name"], r["ker"], r["h64"])
    # the cases are not all zeros, and the zeros are exact
    by = {r["name"]: r for r in rows}
    assert (by["examples_big_R32"]["h64"] > 1e-3).all() and (by["zero_big_R32"]["h64"] > 1e-3).all()
    assert (by["zero_R32"]["h64"] > 1e-3).all() and (by["labels_R32"]["h64"] < 1e-3).all()


def test_what_counts(rows):
    """A raw 0..255 image: its foreground segments are empty, its background counts as ever.  NaN holes add
    nothing: the energy is that of the rays left.  The margin moves the segment's start."""
    ex, labels = example()
    big = labels[[9, 0, 1]].copy()
    big[:, 0:3] *= 1.6
    by = {r["name"]: r for r in rows}
    whole = _kernel(ex[[9, 0, 1]], big, 32)
    assert (by["nanholes_R32"]["ker"] <= whole).all() and (by["nanholes_R32"]["ker"] < whole).any()
    m0, m1 = by["margin_0_R32"]["ker"], by["margin_0.05_R32"]["ker"]
    assert (m1 <= whole).all() and (whole <= m0).all() and (m1 < m0).all()
    # a raw 0..255 image is its background alone: the same image with the foreground blanked
    raw = by["raw255_R32"]
    blank = np.where(raw["true"] > 0, np.nan, raw["true"]).astype(np.float32)
    assert np.array_equal(raw["ker"], _kernel(blank, raw["params"], 32))


def test_runs_bitwise_equal_rows_independent_and_stack_is_three_calls():
    ex, labels = example()
    big = labels.copy()
    big[:, 0:3] *= 1.6
    idx = [0, 3, 5, 7, 9]
    true, p = ex[idx], big[idx]
    a, b = _kernel(true, p, 32), _kernel(true, p, 32)
    assert np.array_equal(a, b) and (a > 0).all()
    for i in range(5):
        assert np.array_equal(_kernel(true[i:i + 1], p[i:i + 1], 32), a[i:i + 1]), i
    rng = np.random.default_rng(3)
    stack = np.stack([p, (p + 0.02 * rng.standard_normal(p.shape)).astype(np.float32), labels[idx]])
    s = _kernel(true, stack.reshape(15, 12), 32)
    for k in range(3):
        assert np.array_equal(s[5 * k:5 * k + 5], _kernel(true, stack[k], 32)), k
    assert np.array_equal(s[:5], a)
    a33 = _kernel(true, p, 33)
    assert np.array_equal(a33[2:3], _kernel(true[2:3], p[2:3], 33))


GUARD = 64


def test_c_abi_checks_its_arguments_and_writes_inside_its_buffers():
    from sqr._lib import lib, ptr, stream_ptr
    from sqr import losses
    L = lib()
    ex, labels = example()
    B, S, R = 2, 4, 33
    t = torch.tensor(ex[:B, 0], device=DEV).contiguous()
    p = torch.tensor(np.concatenate([labels[:B], labels[2:2 + B]]), device=DEV).contiguous()
    wsb = L.sqr_lsq_free_space_workspace_bytes(S, R)
    assert wsb == S * ((R * R + 255) // 256) * 8
    out = torch.full((S + 2 * GUARD,), -7.25, dtype=torch.float64, device=DEV)
    ws = torch.full((wsb + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)

    def call(S=S, B=B, margin=MARGIN, nbytes=wsb):
        rc = L.sqr_lsq_free_space(ptr(p), ptr(t), S, B, 256, 256, R, margin, ptr(out[GUARD:]), ptr(ws[GUARD:]), nbytes,
                                  stream_ptr(DEV))
        torch.cuda.synchronize()
        return rc

    assert call(nbytes=wsb - 1) == -1 and b"workspace" in L.sqr_last_error_string()
    assert call(S=3) == -1 and b"multiple" in L.sqr_last_error_string()
    assert call(margin=-0.1) == -1 and b"margin" in L.sqr_last_error_string()
    assert call(S=0) == -1 and call(B=0) == -1
    assert bool((out == -7.25).all()) and bool((ws == 0xA5).all())  # nothing was launched
    assert call() == 0, L.sqr_last_error_string()
    assert bool((out[:GUARD] == -7.25).all()) and bool((out[GUARD + S:] == -7.25).all())
    assert bool((ws[:GUARD] == 0xA5).all()) and bool((ws[GUARD + wsb:] == 0xA5).all())
    assert np.array_equal(out[GUARD:GUARD + S].cpu().numpy(), _kernel(ex[:B], p.cpu().numpy(), R))
    with pytest.raises(ValueError):
        losses.free_space_energy(torch.tensor(ex[:2]), p, R)  # a CPU tensor
    with pytest.raises(ValueError):
        losses.free_space_energy(torch.tensor(ex[:2], device=DEV), p[:3], R)  # 3 samples, 2 images
