"""The host reference of the several-parts recovery (tests/_parts_ref.py) against what is known without it, against
its fixture (tests/golden/parts.npz, tests/golden/gen_golden_parts.py), and the Python argument checks of
sqr.fit.recover_parts, which need no device.

The fixture took the host pipeline minutes; here the seeding is repeated in full (float32 arithmetic, exact), every
round's assignment is repeated from the stored parameters (exact labels), and of the fits scene A's part 0 is
repeated in float64: its round 0 (three starts, 30 iterations) and its round 1 (10 iterations from round 0's end).
"""
import numpy as np
import pytest
import torch

import _parts_ref as pr
import _points_cases as pc
from _golden import load


@pytest.fixture(scope="module")
def parts():
    return load("parts.npz")


def _cloud_T(cloud, dt=torch.float64):
    return torch.tensor(np.ascontiguousarray(np.asarray(cloud, np.float32).T)).to(dt)


def test_radial_distance_of_a_golden_cloud_to_its_label_is_zero():
    d = pc.golden()
    for i in range(8):
        r = pr.radial_distance(_cloud_T(d["clouds"][i]), torch.tensor(d["labels"][i], dtype=torch.float64))
        print("cloud %d: largest radial distance to its own label %.3e" % (i, r.max().item()))
        assert r.max().item() <= 1e-6, (i, r.max().item())  # the points are float32 roundings of surface points


def test_radial_distance_to_a_sphere_is_the_distance_to_its_surface():
    rng = np.random.default_rng(0)
    for r in (0.05, 0.2, 0.7):
        t = rng.uniform(0.2, 0.8, 3)
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        pts = torch.tensor(rng.uniform(-0.5, 1.5, (3, 400)))
        p = torch.tensor(np.concatenate([[r, r, r], [1.0, 1.0], t, q]))
        got = pr.radial_distance(pts, p).numpy()
        norm = np.linalg.norm(pts.numpy() - t[:, None], axis=0)
        want = np.abs(norm - r)
        # |1 - r / n| n against |n - r|: a few roundings of values of the size of n
        assert np.abs(got - want).max() <= 16 * np.finfo(np.float64).eps * norm.max(), np.abs(got - want).max()


def test_a_distance_that_is_not_finite_is_inf_and_never_wins():
    d = pc.golden()
    cloud = d["clouds"][0][:64]
    bad = d["labels"][0].copy()
    bad[0] = np.nan
    label, dist, D = pr.assign(cloud, np.stack([bad, d["labels"][0], d["labels"][0]]))
    assert np.isinf(D[0]).all() and (label == 1).all() and np.isfinite(dist).all()  # the lower of the two equal rows
    label, dist, _ = pr.assign(cloud, np.stack([bad, bad]))
    assert (label == 0).all() and np.isinf(dist).all()
    pts = cloud.copy()
    pts[3, 1] = np.nan
    label, dist, _ = pr.assign(pts, d["labels"][:2], count=60)
    assert label[3] == -1 and dist[3] == 0 and (label[60:] == -1).all() and (label[:3] >= 0).all()


@pytest.mark.parametrize("scene", ["a", "b"])
def test_seeding_reproduces_the_fixture(parts, scene):
    pts = parts[scene + "_points"]
    M = len(parts[scene + "_seeds"])
    s = pr.seed(pts, M, lloyd=int(parts["lloyd"]))
    assert np.array_equal(s["seeds"], parts[scene + "_seeds"])
    assert np.array_equal(s["label"], parts[scene + "_lloyd_label"])
    assert np.array_equal(s["centres"], parts[scene + "_centres"])
    assert s["margin"] == parts[scene + "_lloyd_margin"] and s["margin"] > 1e-5
    # fewer distinct points than parts: the last seed is repeated and the duplicates stay empty
    few = pr.seed(np.repeat(pts[:2], 3, axis=0), 4, lloyd=2)
    assert few["seeds"].tolist() == [3, 0, 0, 0] and set(few["label"].tolist()) == {0, 1}
    none = pr.seed(np.full((5, 3), np.nan, np.float32), 2)
    assert none["seeds"].tolist() == [-1, -1] and (none["label"] == -1).all() and not none["centres"].any()


@pytest.mark.parametrize("tag", ["64", "32"])
@pytest.mark.parametrize("scene", ["a", "b"])
def test_every_rounds_assignment_reproduces_the_fixture(parts, scene, tag):
    dt = torch.float64 if tag == "64" else torch.float32
    pts, true = parts[scene + "_points"], parts[scene + "_true_label"]
    label = parts[scene + "_lloyd_label"]
    for t in range(int(parts["rounds"])):
        new, dist, _ = pr.assign(pts, parts["%s_params_%s" % (scene, tag)][t], dt=dt)
        assert np.array_equal(new, parts["%s_label_%s" % (scene, tag)][t]), t
        assert int((new != label).sum()) == parts["%s_changed_%s" % (scene, tag)][t], t
        label = new
    # the distances themselves are torch's pow on whatever CPU runs this: d = n |1 - f^(-1/2)| with n <= sqrt(3) in
    # the unit cube and f = F^e1 through two powers with exponents of at most 10 and their inverses, a relative
    # error of f of a few tens of roundings; 64 of them, on a point of the surface (f = 1) half of that times n
    eps = np.finfo(np.float64 if tag == "64" else np.float32).eps
    err = np.abs(dist - parts["%s_dist_%s" % (scene, tag)]).max()
    print("scene %s f%s: distances off the fixture's by at most %.2e (allowed %.2e)" % (scene, tag, err, 64 * eps))
    assert err <= 64 * eps
    assert np.array_equal(parts["%s_part_of_%s" % (scene, tag)][label], true)  # the true partition
    assert parts["%s_changed_%s" % (scene, tag)][-1] == 0
    assert parts["%s_radial_margin_%s" % (scene, tag)] > 1e-3


def test_the_fits_of_one_part_reproduce_the_fixture(parts):
    pts = parts["a_points"]
    own = pts[parts["a_lloyd_label"] == 0]
    p0, e0 = pr.recover_part(own, int(parts["iters0"]), float(parts["e0"]), torch.float64)
    np.testing.assert_allclose(p0, parts["a_params_64"][0, 0], rtol=0, atol=1e-6)
    assert e0 <= 1e-11 and parts["a_energy_64"][0, 0] <= 1e-11
    own = pts[parts["a_label_64"][0] == 0]
    p1, _ = pr.fit_part(own, parts["a_params_64"][0, 0], int(parts["iters"]), torch.float64)
    np.testing.assert_allclose(p1, parts["a_params_64"][1, 0], rtol=0, atol=1e-6)


def test_recover_parts_checks_its_arguments_before_it_asks_for_a_device():
    from sqr import fit
    pts = torch.zeros(2, 8, 3)
    for bad in (0, -1, 17):
        with pytest.raises(ValueError, match=r"parts must be in \[1,16\]"):
            fit.recover_parts(pts, bad)
    with pytest.raises(ValueError, match="more than 65535"):
        fit.recover_parts(torch.zeros(1366, 1, 3), 16)  # 3 x 1366 x 16 = 65568
    with pytest.raises(ValueError, match=r"points must be \[B,P,3\]"):
        fit.recover_parts(torch.zeros(8, 3), 2)
    for lab in (torch.zeros(2, 7, dtype=torch.int32), torch.zeros(8, dtype=torch.int32),
                torch.zeros(2, 8, dtype=torch.int64), torch.zeros(2, 8), np.zeros((2, 8), np.int32)):
        with pytest.raises(ValueError, match=r"labels must be an int32 tensor \[2,8\]"):
            fit.recover_parts(pts, 2, labels=lab)
    # what passes these checks goes on to the device check: there is no CPU path
    with pytest.raises(ValueError, match="CPU tensor"):
        fit.recover_parts(pts, 2, labels=torch.zeros(2, 8, dtype=torch.int32))
    with pytest.raises(ValueError, match="CPU tensor"):
        fit.recover_parts(torch.zeros(1365, 1, 3), 16)  # 65520: allowed
