"""The free-space energy's host reference (tests/_free_space_ref.py) against closed forms on a sphere, and at the
labels of the ten example images.  No GPU.

A sphere a = (r, r, r), e = (1, 1), centre t, identity quaternion has F = (rho^2 + (z - t_z)^2) / r^2 on the ray at
lateral distance rho from t: the minimum over z is rho^2 / r^2 at z = t_z, or F(zlo) where the segment starts
behind the centre.  R = 16 makes c / R and 1 - r / R exact; t is off the grid, so the zero fix never applies.
The golden section pins z* to the square root of the rounding (1e-8) and F is quadratic about it: the value is
good to 1e-16 / r^2, far below the 1e-10 asked for.
"""
import numpy as np
import torch

import _free_space_ref as fsr
from _lsq_cases import example

R = 16
RAD, T = 0.21, np.array([0.5131, 0.4817, 0.5523])
SPHERE = np.array([RAD, RAD, RAD, 1, 1, T[0], T[1], T[2], 0, 0, 0, 1], np.float64)


def _rho2():
    rows, cols = np.meshgrid(np.arange(R), np.arange(R), indexing="ij")
    x, y = cols / R, 1 - rows / R
    return (x - T[0]) ** 2 + (y - T[1]) ** 2


def test_sphere_against_an_empty_image():
    rho2 = _rho2()
    want = RAD ** 3 * ((rho2[rho2 < RAD ** 2] / RAD ** 2 - 1) ** 2).sum()
    assert (rho2 < RAD ** 2).sum() > 20
    got = fsr.free_space(np.zeros((1, 1, R, R), np.float32), SPHERE[None], R)
    np.testing.assert_allclose(got, [want], rtol=1e-10)
    # a 64 x 64 image resized to R is the same rays; a sample per image, and the [K,B] layout
    two = np.stack([SPHERE, SPHERE * [0.5, 0.5, 0.5, 1, 1, 1, 1, 1, 1, 1, 1, 1]])
    got = fsr.free_space(np.zeros((2, 64, 64), np.float32), np.concatenate([two, two[::-1]]), R)
    np.testing.assert_allclose(got[[0, 3]], [want, want], rtol=1e-10)
    assert got[1] == got[2] and 0 < got[1] < want


def test_sphere_behind_its_own_visible_surface_costs_nothing():
    """Foreground at the sphere's top minus half the margin over its footprint, background elsewhere: every
    segment starts above the sphere or passes beside it."""
    rho2 = _rho2()
    img = np.where(rho2 < RAD ** 2, T[2] + RAD - 0.5 * fsr.MARGIN, 0.0).astype(np.float32)
    assert fsr.free_space(img[None, None], SPHERE[None], R)[0] == 0.0
    # NaN pixels add nothing: the empty image's energy with every ray through the sphere blanked
    nan = np.where(rho2 < RAD ** 2, np.nan, 0.0).astype(np.float32)
    assert fsr.free_space(nan[None, None], SPHERE[None], R)[0] == 0.0
    # a raw 0..255 image: z + margin > 4 on the foreground is an empty segment
    raw = np.where(rho2 < RAD ** 2, 200.0, 0.0).astype(np.float32)
    assert fsr.free_space(raw[None, None], SPHERE[None], R)[0] == 0.0


def test_segment_that_starts_behind_the_centre_is_evaluated_at_its_start():
    z0, margin = np.float32(0.6), 0.01
    rho2 = _rho2()
    for dt, tol in ((torch.float64, 1e-10), (torch.float32, 1e-4)):
        # the float32 pixel plus the float32 margin, added in dt
        zl = float(z0) + float(np.float32(margin)) if dt == torch.float64 else float(z0 + np.float32(margin))
        F = (rho2 + (zl - T[2]) ** 2) / RAD ** 2
        want = RAD ** 3 * ((F[F < 1] - 1) ** 2).sum()
        assert zl > T[2] and (F < 1).sum() > 10
        got = fsr.free_space(np.full((1, 1, R, R), z0, np.float32), SPHERE[None], R, margin=margin, dt=dt)
        np.testing.assert_allclose(got, [want], rtol=tol)
    # the minimiser itself
    p = torch.tensor(SPHERE)
    x, y, lo, hi = fsr.rays_of(torch.full((R, R), float(z0)), R, margin, torch.float64)
    _, zs = fsr.ray_minimum(x, y, lo, hi, p)
    assert torch.equal(zs, lo)
    x, y, lo, hi = fsr.rays_of(torch.zeros(R, R), R, margin, torch.float64)
    _, zs = fsr.ray_minimum(x, y, lo, hi, p)
    assert float((zs - T[2]).abs().max()) <= 1e-7


def test_labels_are_consistent_with_their_images():
    """At the ten labels E_fs <= 1e-3 (measured: 4.7e-5 to 3.3e-4): the true model stays out of the space its own
    image shows to be empty, up to the image's quantisation and the resize."""
    ex, labels = example()
    fs = fsr.free_space(ex, labels, 32)
    print("E_fs at the labels:", " ".join("%.2e" % v for v in fs))
    assert (fs >= 0).all() and (fs <= 1e-3).all(), fs
