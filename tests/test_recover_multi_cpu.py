"""The six starts and the scored selection of the multi-start recovery in the host reference
(tests/_free_space_ref.py), and the fixture tests/golden/recover_multi.npz against its generator.  No GPU."""
import importlib.util
import os

import numpy as np

import _free_space_ref as fsr
import _recover_ref as rr
from _golden import GOLDEN, load
from _lsq_cases import example
import _lm_ref
import torch


def _front_half_box():
    """Grid points of the front half z in [0.5, 0.6] of the box [0.3, 0.7] x [0.35, 0.65] x [0.4, 0.6], seen
    face-on from +z: the smallest variance is along z."""
    g = np.meshgrid(np.linspace(0.3, 0.7, 9), np.linspace(0.35, 0.65, 7), np.linspace(0.5, 0.6, 5), indexing="ij")
    return np.stack([x.ravel() for x in g])


def test_depth_zero_repeats_the_three_starts():
    ex, _ = example()
    for i in (0, 5, 7):
        pts = _lm_ref.points_of(ex[i:i + 1], 32, torch.float64)[0].numpy()
        s6, info = fsr.starts6_of(pts, depth=0.0)
        s3, _ = rr.starts_of(pts)
        assert np.array_equal(s6[:3], s3) and np.array_equal(s6[3:], s3)
        d6, _ = fsr.starts6_of(pts, depth=1.0)
        assert np.array_equal(d6[:3], s3) and not np.array_equal(d6[3:], s3)
        assert np.array_equal(d6[:, 8:][3:], s3[:, 8:])  # the frame, and so q, is the same
    z6, _ = fsr.starts6_of(np.zeros((3, 0)))
    assert np.array_equal(z6, np.tile(rr.default_start(1.0), (6, 1)))


def test_box_seen_face_on_is_extended_to_the_far_side():
    P = _front_half_box()
    s, info = fsr.starts6_of(P, depth=1.0)
    V = info["frame"]
    j = fsr.depth_axis(V)
    assert j == 0 and abs(abs(V[2, 0]) - 1) <= 1e-12 and V[2, 0] < 0  # column 0 (the smallest variance) is -z
    # starts 0 and 3 have the axis order (0, 1, 2): local x is the depth axis
    np.testing.assert_allclose(s[0, 0:3], [0.05, 0.15, 0.2], atol=1e-7)
    np.testing.assert_allclose(s[3, 0:3], [0.10, 0.15, 0.2], atol=1e-7)  # the true half depth
    np.testing.assert_allclose(s[0, 5:8], [0.5, 0.5, 0.55], atol=1e-7)
    np.testing.assert_allclose(s[3, 5:8], [0.5, 0.5, 0.50], atol=1e-7)   # the true centre: away from the viewer
    for k in range(3):
        ax = [(k + i) % 3 for i in range(3)]
        assert np.array_equal(s[3 + k, 0:3], s[3][ax]) and np.array_equal(s[3 + k, 8:], s[k, 8:])
        np.testing.assert_allclose(s[3 + k, 5:8], s[3, 5:8], atol=1e-7)
    # seen from behind (the frame's depth column pointing at the viewer): the minimum moves instead
    Q = P.copy()
    Vf = V.copy()
    Vf[:, 0] = -Vf[:, 0]
    Vf[:, 2] = -Vf[:, 2]
    f = fsr.starts6_from_frame(Q, Vf, 1.0, 1.0)
    np.testing.assert_allclose(f[3, 0:3], [0.10, 0.15, 0.2], atol=1e-7)
    np.testing.assert_allclose(f[3, 5:8], [0.5, 0.5, 0.50], atol=1e-7)
    half = fsr.starts6_from_frame(P, V, 1.0, 0.5)
    np.testing.assert_allclose(half[3, 0:3], [0.075, 0.15, 0.2], atol=1e-7)
    np.testing.assert_allclose(half[3, 5:8], [0.5, 0.5, 0.525], atol=1e-7)


def test_scored_selection():
    e = np.array([[4.2e-4, 1.0, np.nan], [5.7e-4, 1.0, 2.0]])
    fs = np.array([[3.0e-3, 0.0, 0.0], [1.0e-5, 0.0, np.inf]])
    assert fsr.select_scored(e, fs, 0.0).tolist() == [0, 0, 1]
    assert fsr.select_scored(e, fs, 1.0).tolist() == [1, 0, 1]
    s0 = fsr.score_of(e, fs, 0.0)
    assert np.array_equal(s0.view(np.int64), e.view(np.int64))  # w = 0: the energy, whatever E_fs is
    np.testing.assert_array_equal(fsr.score_of(e, fs, 2.0)[:, :2], e[:, :2] + 2.0 * fs[:, :2])


def test_fixture_matches_its_generator_on_one_image():
    """recover_multi.npz's rows of image 5 regenerated (both precisions), with the bounds and the reasoning of
    tests/test_recover_cpu.py's twin.  Regenerated where the fixture was made every row is bitwise the stored one;
    another build may round a sum or a power differently, a perturbation of the size of the precision's rounding
    (1e-16 / 6e-8), which the loop's accept decisions amplify.  The amplification is read off the fixture: on
    image 5 the float32 pipeline ends within 2.3e-5 of the float64 one from every one of the six starts (about
    4e2 times the rounding), so the bounds are 1e-10 in float64 and 1e-4 in float32.  (Image 7, the twin's choice,
    will not do here: from its depth-aware start 4 the two precisions end 3 % apart.)  Parameters: the square root
    of that, the energy being flat at its minimum.  The free-space energy is a function of the parameters, pinned
    like them: relative 10 x the square root, with an absolute floor of 1e-2 x it for the exact and near zeros.
    The float64 winners reach IoU 0.9 on 8."""
    spec = importlib.util.spec_from_file_location("gen_golden_recover_multi",
                                                  os.path.join(GOLDEN, "gen_golden_recover_multi.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    d, ex = load("recover_multi.npz"), load("example_images.npz")
    assert (int(d["R"]), int(d["iters"]), float(d["e0"]), float(d["depth"]), float(d["margin"]), float(d["w_fs"]),
            int(d["iou_grid"])) == (gen.R, gen.ITERS, gen.E0, gen.DEPTH, gen.MARGIN, gen.W_FS, gen.IOU_GRID)
    i = 5
    assert np.abs(d["after_32"][i] / d["after_64"][i] - 1).max() <= 5e-5
    img, lab = ex["images"][i].astype(np.float32) / 255.0, ex["labels"][i].astype(np.float32)
    for tag, dt in gen.TAGS:
        rows = gen.rows_of(img, lab, dt)
        tol = 1e-4 if tag == "32" else 1e-10
        assert np.array_equal(rows["starts"], d["starts_" + tag][i])
        np.testing.assert_allclose(rows["before"], d["before_" + tag][i], rtol=tol)
        np.testing.assert_allclose(rows["after"], d["after_" + tag][i], rtol=tol)
        np.testing.assert_allclose(rows["params"], d["params_" + tag][i], rtol=0, atol=tol ** 0.5)
        np.testing.assert_allclose(rows["fs"], d["fs_" + tag][i], rtol=10 * tol ** 0.5, atol=1e-2 * tol ** 0.5)
        assert rows["winner"] == d["winner_" + tag][i]
        np.testing.assert_allclose(rows["iou"], d["iou_" + tag][i], atol=2e-4)
    old = load("recover.npz")
    for tag in ("64", "32"):
        for k in ("starts", "before", "after", "fs", "score", "params", "iou"):
            assert d["%s_%s" % (k, tag)].shape[:2] == (10, 6), k
        assert np.array_equal(d["score_" + tag], d["after_" + tag] + d["fs_" + tag])
        assert np.array_equal(d["winner_" + tag], rr.select(d["score_" + tag].T))
        assert np.array_equal(d["iou_winner_" + tag], d["iou_" + tag][np.arange(10), d["winner_" + tag]])
        assert (d["after_" + tag] <= d["before_" + tag]).all() and (d["fs_" + tag] >= 0).all()
        # starts 0..2 and what becomes of them are the three-start fixture's
        assert np.array_equal(d["starts_" + tag][:, :3], old["starts_" + tag])
        np.testing.assert_allclose(d["after_" + tag][:, :3], old["after_" + tag], rtol=1e-4 if tag == "32" else 1e-10)
    iou = d["iou_winner_64"]
    print("float64 winners: IoU %s, mean %.3f" % (" ".join("%.3f" % v for v in iou), iou.mean()))
    assert (iou >= 0.9).sum() >= 8
