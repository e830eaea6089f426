"""The classical recovery's host reference (tests/_recover_ref.py): the start rules on closed-form point sets,
the selection rule, and the fixture tests/golden/recover.npz against its generator.  No GPU."""
import importlib.util
import os

import numpy as np

import _recover_ref as rr
from _golden import GOLDEN, load
from quaternion import mat_from_quaternion_np


def _box(n=(9, 7, 5), lo=(0.3, 0.35, 0.4), hi=(0.7, 0.65, 0.6)):
    """Grid points of an axis-aligned box [3,N]: extents 0.4, 0.3, 0.2, so the variances differ."""
    g = np.meshgrid(*[np.linspace(a, b, k) for a, b, k in zip(lo, hi, n)], indexing="ij")
    return np.stack([x.ravel() for x in g])


def _check_common(starts, info, e0=1.0):
    V = info["frame"]
    assert np.abs(V.T @ V - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(V) - 1) <= 1e-14
    assert (np.diff(info["eigenvalues"]) >= 0).all()
    assert starts.dtype == np.float32 and starts.shape == (3, 12) and np.isfinite(starts).all()
    assert (starts[:, 0:3] >= np.float32(0.05)).all() and (starts[:, 0:3] <= 1).all()
    assert (starts[:, 3:5] == np.float32(e0)).all()
    assert (starts[:, 5:8] >= 0).all() and (starts[:, 5:8] <= 1).all()
    assert np.abs(np.linalg.norm(starts[:, 8:].astype(np.float64), axis=1) - 1).max() <= 1e-6
    for k in range(3):  # mat_from_quaternion(q_k) is the cyclically permuted frame
        M = mat_from_quaternion_np(starts[k, 8:])[0]
        assert np.abs(M - V[:, [(k + j) % 3 for j in range(3)]]).max() <= 2e-6, k


def test_axis_aligned_box():
    P = _box()
    starts, info = rr.starts_of(P)
    _check_common(starts, info)
    assert info["count"] == P.shape[1]
    np.testing.assert_allclose(info["centroid"], [0.5, 0.5, 0.5], atol=1e-15)
    C = np.cov(P, bias=True)
    np.testing.assert_allclose(info["eigenvalues"], np.linalg.eigvalsh(C), atol=1e-15)
    # ascending variance: z, y, x; column 0 negative, column 1 positive, column 2 = -e_z x e_y = e_x
    # (the one-pass covariance's off-diagonals are rounding noise of 1e-17 over eigenvalue gaps of 5e-3)
    np.testing.assert_allclose(info["frame"], [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], atol=1e-12)
    half = np.array([0.1, 0.15, 0.2])
    for k in range(3):
        np.testing.assert_allclose(starts[k, 0:3], half[[(k + j) % 3 for j in range(3)]], rtol=1e-6)
        np.testing.assert_allclose(starts[k, 5:8], [0.5, 0.5, 0.5], atol=1e-7)


def test_rotated_box_recovers_the_rotation():
    q = np.array([0.3, -0.2, 0.4, 0.8])
    q /= np.linalg.norm(q)
    Rq = mat_from_quaternion_np(q)[0]
    c = np.array([0.5, 0.5, 0.5])
    P = Rq @ (_box() - c[:, None]) + c[:, None]
    starts, info = rr.starts_of(P)
    _check_common(starts, info)
    np.testing.assert_allclose(info["eigenvalues"], np.linalg.eigvalsh(np.cov(_box(), bias=True)), atol=1e-15)
    half = np.array([0.1, 0.15, 0.2])
    box_axis = [2, 1, 0]  # frame column j is the box's axis z, y, x (up to sign)
    for j in range(3):
        d = np.abs(Rq.T @ info["frame"][:, j])
        assert abs(d[box_axis[j]] - 1) <= 1e-12 and np.delete(d, box_axis[j]).max() <= 1e-12
    for k in range(3):
        np.testing.assert_allclose(starts[k, 0:3], half[[(k + j) % 3 for j in range(3)]], rtol=1e-6)
        np.testing.assert_allclose(starts[k, 5:8], c, atol=1e-7)


def test_sphere_cap_with_repeated_eigenvalues():
    th, ph = np.meshgrid(np.linspace(0.1, 0.9, 6), np.arange(8) * (2 * np.pi / 8), indexing="ij")
    P = 0.5 + 0.3 * np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)]).reshape(3, -1)
    starts, info = rr.starts_of(P)
    _check_common(starts, info)
    lam = info["eigenvalues"]
    assert abs(lam[2] - lam[1]) <= 1e-14 and lam[0] < 0.5 * lam[1]  # x and y alike, the cap is flat in z
    assert np.abs(np.abs(info["frame"][:, 0]) - [0, 0, 1]).max() <= 1e-12
    # whatever direction the repeated pair takes, the frame diagonalises the covariance
    D = info["frame"].T @ info["covariance"] @ info["frame"]
    assert np.abs(D - np.diag(np.diagonal(D))).max() <= 1e-15
    zext = 0.5 * 0.3 * (np.cos(0.1) - np.cos(0.9))
    np.testing.assert_allclose(starts[0, 0], max(zext, 0.05), rtol=1e-6)


def test_one_point_collinear_points_and_no_point():
    starts, info = rr.starts_of(np.array([[0.25], [0.75], [0.5]]))
    _check_common(starts, info)
    assert info["count"] == 1
    assert (starts[:, 0:3] == np.float32(0.05)).all()  # zero extents clamp
    np.testing.assert_allclose(starts[:, 5:8], np.tile([0.25, 0.75, 0.5], (3, 1)), atol=1e-7)
    d = np.array([1.0, 2.0, 2.0]) / 3
    P = np.array([0.2, 0.3, 0.4])[:, None] + d[:, None] * np.array([0.0, 0.15, 0.3])
    starts, info = rr.starts_of(P)
    _check_common(starts, info)
    assert abs(abs(info["frame"][:, 2] @ d) - 1) <= 1e-12  # the line is the axis of the largest eigenvalue
    for k in range(3):
        a = starts[k, 0:3]
        np.testing.assert_allclose(a[(2 - k) % 3], 0.15, rtol=1e-6)
        assert (np.delete(a, (2 - k) % 3) == np.float32(0.05)).all()
    np.testing.assert_allclose(starts[:, 5:8], np.tile(P[:, 1], (3, 1)), atol=1e-7)
    starts, info = rr.starts_of(np.zeros((3, 0)), e0=0.7)
    assert info["count"] == 0 and np.array_equal(info["frame"], np.eye(3))
    assert np.array_equal(starts, np.tile(rr.default_start(0.7), (3, 1)))
    assert starts[0].tolist() == [np.float32(v) for v in (.05, .05, .05, .7, .7, .5, .5, .5, 0, 0, 0, 1)]


def test_float32_rules_follow_the_float64_ones():
    P = _box()
    s64, _ = rr.starts_of(P, dt=np.float64)
    s32, i32 = rr.starts_of(P.astype(np.float32), dt=np.float32)
    assert i32["frame"].dtype == np.float32
    # the one-pass float32 covariance is off by ~6e-8 x 0.3 over eigenvalue gaps of 5e-3: angles of ~1e-5
    np.testing.assert_allclose(s32, s64, atol=1e-4)


def test_quaternion_branches():
    """Every branch of the largest-of-four rule gives back its matrix, never dividing by less than 2."""
    for q in ([0, 0, 0, 1], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0.9, 0.1, 0.1, 0.05], [0.1, 0.9, 0.1, 0.05],
              [0.1, 0.1, 0.9, 0.05], [0.5, 0.5, 0.5, 0.5], [0.5, -0.5, 0.5, -0.5]):
        q = np.array(q, np.float64) / np.linalg.norm(q)
        M = mat_from_quaternion_np(q)[0]
        got = rr.quat_of(M)
        assert abs(np.linalg.norm(got) - 1) <= 1e-15
        assert np.abs(mat_from_quaternion_np(got)[0] - M).max() <= 1e-15, q


def test_selection_rule():
    nan = np.nan
    e = np.array([[3.0, 1.0, 1.0, nan, nan, 2.0, nan],
                  [2.0, 1.0, 0.5, 4.0, nan, nan, nan],
                  [1.0, 2.0, 0.5, 3.0, nan, 2.0, 0.0]])
    assert rr.select(e).tolist() == [2, 0, 1, 2, 0, 0, 2]
    assert rr.select(e[:1]).tolist() == [0] * 7
    assert rr.select(np.array([[np.inf], [-np.inf], [0.0]])).tolist() == [1]


def test_fixture_matches_its_generator_on_one_image():
    """recover.npz's rows of image 7 regenerated (both precisions): the fixture cannot drift from its generator.
    Regenerated where the fixture was made, every row is bitwise the stored one, with 1, 8 and 16 threads.  The
    starts are plain numpy and must be equal.  The loop's results go through BLAS and libm, where another build may
    round a sum or a power differently: a perturbation of the size of the precision's rounding (1e-16 / 6e-8).
    On this image the float32 pipeline ends within 5e-5 of the float64 one from every start, an amplification of
    about 1e3, so the bounds are 1e-10 in float64 and 1e-4 in float32 (a changed rule moves these by 1e-2 and
    more: the other sign choices' energies in DESIGN.md)."""
    spec = importlib.util.spec_from_file_location("gen_golden_recover", os.path.join(GOLDEN, "gen_golden_recover.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    d, ex = load("recover.npz"), load("example_images.npz")
    assert (int(d["R"]), int(d["iters"]), float(d["e0"]), int(d["iou_grid"])) == (gen.R, gen.ITERS, gen.E0, gen.IOU_GRID)
    i = 7
    img, lab = ex["images"][i].astype(np.float32) / 255.0, ex["labels"][i].astype(np.float32)
    for tag, dt in gen.TAGS:
        rows = gen.rows_of(img, lab, dt)
        tol = 1e-4 if tag == "32" else 1e-10
        assert np.array_equal(rows["starts"], d["starts_" + tag][i])
        np.testing.assert_allclose(rows["before"], d["before_" + tag][i], rtol=tol)
        np.testing.assert_allclose(rows["after"], d["after_" + tag][i], rtol=tol)
        # near its minimum the energy is flat: the parameters are pinned to the square root of its tolerance
        np.testing.assert_allclose(rows["params"], d["params_" + tag][i], rtol=0, atol=tol ** 0.5)
        assert rows["winner"] == d["winner_" + tag][i]
        # a ratio of voxel counts: equal unless a voxel on the surface flips (1 in ~1e4)
        np.testing.assert_allclose(rows["iou"], d["iou_" + tag][i], atol=2e-4)
    for tag in ("64", "32"):
        for k in ("starts", "before", "after", "params", "iou"):
            assert d["%s_%s" % (k, tag)].shape[:2] == (10, 3), k
        assert np.array_equal(d["winner_" + tag], rr.select(d["after_" + tag].T))
        assert np.array_equal(d["iou_winner_" + tag], d["iou_" + tag][np.arange(10), d["winner_" + tag]])
        assert (d["after_" + tag] <= d["before_" + tag]).all()
    assert (d["iou_winner_64"] >= 0.9).sum() >= 5
