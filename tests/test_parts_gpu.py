"""Several superquadrics per point list on the GPU: sqr_pts_seed / _assign / _labeled_lm_refine / _labeled_recover /
_recover_parts and their Python faces (sqr.losses.pts_seed, pts_assign, pts_labeled_*, sqr.fit.assign_points,
recover_parts, recover_points.py --parts).

The references are the host's: tests/_parts_ref.py, and its fixture tests/golden/parts.npz (tests/golden/
gen_golden_parts.py: two scenes of three and four bodies through the float64 and the float32 host pipeline), so no
test here runs a host Levenberg-Marquardt loop.

Tolerances.  Assignment: the project's yardstick rule on the winning distance (absolute, in the cloud's units): the
kernel's largest error against float64 is at most twice that of the same reference run in float32 inside the test;
the label is the float64 one wherever the float64 margin between the two nearest parts exceeds that bound, and the
slots it leaves out are at most 2 % (met by the float32 reference alone: checked here too).  The counts are the
integers of the returned labels and part_dist is the float64 sum of the returned dist to 1e-12.  Everything about
the part source, batches, repeats and graphs is bitwise.  Seeding: float32 arithmetic the host repeats, so seeds and
labels are exact and the centres (float64 means in another order) within one float32 ulp.  The chain: the fixture's
final labels on every point, and each part's IoU against its body at grid 32 at least the float32 host pipeline's
minus 0.01 (tests/test_points_gpu.py's rule).
Measured on MI355X: profiles/parts_accuracy.txt.

The fixture's scenes have three and four bodies and a call has one M, so "one batch of two with count" is run twice:
both scenes in one list of 2048 slots with M = 3 (scene A's row is checked) and with M = 4 (scene B's row).
"""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import _parts_ref as pr
import _points_cases as pc
from _golden import load

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P_SET = (1, 64, 255, 256, 257, 512)
M_SET = (1, 2, 3, 16)
SEED = 20261021


def _dev(x, dtype=None):
    return torch.tensor(np.ascontiguousarray(x), device=DEV, dtype=dtype)


def _same(a, b):
    """Bitwise equality of two tensors (or tuples / dicts of them): same dtype, same shape, same bytes."""
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().reshape(-1).view(torch.uint8),
                                                                     b.contiguous().reshape(-1).view(torch.uint8))


@pytest.fixture(scope="module")
def parts():
    return load("parts.npz")


# ------------------------------------------------------------------------------- 1. the assignment vs float64
def assign_case(P, M, seed=SEED):
    """B = 3 clouds of P slots and M parameter rows each.
      points  golden clouds 0, 1, 2 thinned to P slots; cloud 1 shifted by _points_cases.SHIFT (coordinates outside
              [0,1], z < 0); cloud 1 counts P - 7 slots only (finite junk behind them); cloud 2 has NaN and Inf holes
      params  random labels (classes.sample_sq_params); row 0 of every cloud is the cloud's own label perturbed by
              N(0, 0.03) (shifted along for cloud 1), so that small distances occur; cloud 2's rows 1 and 2 leave
              their clamps as in _points_cases.accuracy_case (a0 = 1.2; e0 = 0.05 with t0 = -0.1)
      prev    random labels in [-1, M]
    -> (points [3,P,3] f32, count [3] i32, params [3,M,12] f32, prev [3,P] i32)."""
    import classes
    d = pc.golden()
    rng = np.random.default_rng(seed + 1000 * M + P)
    pts = np.stack([pc.subset(d["clouds"][b], P) for b in range(3)]).astype(np.float32)
    pts[1] += pc.SHIFT
    count = np.array([P, max(P - 7, 1), P], np.int32)
    pts[1, count[1]:] = 7.5
    if P >= 64:
        pts[2, 5, 1] = np.nan
        pts[2, P // 2] = np.inf
    par = classes.sample_sq_params(rng, 3 * M).reshape(3, M, 12).astype(np.float64)
    own = d["labels"][:3].astype(np.float64)
    own[1, 5:8] += pc.SHIFT
    par[:, 0] = own + 0.03 * rng.normal(size=own.shape)
    if M >= 2:
        par[2, 1, 0] = 1.2
    if M >= 3:
        par[2, 2, 3], par[2, 2, 5] = 0.05, -0.1
    prev = rng.integers(-1, M + 1, size=(3, P)).astype(np.int32)
    return pts, count, par.astype(np.float32), prev


def _host_assign(pts, count, par, dt):
    """-> (label [3,P], dist [3,P], margin [3,P]: second best - best, inf for M = 1 and for slots that do not count)."""
    out = [pr.assign(pts[b], par[b], int(count[b]), dt) for b in range(3)]
    margin = []
    for label, _, D in out:
        two = np.sort(D, axis=0)
        with np.errstate(invalid="ignore"):
            m = two[1] - two[0] if len(D) > 1 else np.full(D.shape[1], np.inf)
        margin.append(np.where(label >= 0, np.nan_to_num(m, nan=0.0, posinf=np.inf), np.inf))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack(margin)


@pytest.fixture(scope="module")
def accuracy():
    """Per (P, M): the case, the float64 reference, the float32 reference's and the kernel's results.  Once."""
    from sqr import losses
    rows = []
    for P in P_SET:
        for M in M_SET:
            pts, count, par, prev = assign_case(P, M)
            l64, d64, margin = _host_assign(pts, count, par, torch.float64)
            l32, d32, _ = _host_assign(pts, count, par, torch.float32)
            got = losses.pts_assign(_dev(pts), _dev(par), _dev(count), _dev(prev))
            torch.cuda.synchronize()
            got = {k: v.cpu().numpy() for k, v in got.items()}
            on = l64 >= 0
            assert np.isfinite(d64[on]).all() and np.isfinite(d32[on]).all(), (P, M)
            rows.append(dict(P=P, M=M, pts=pts, count=count, par=par, prev=prev, l64=l64, d64=d64, margin=margin,
                             l32=l32, on=on, got=got, ref=float(np.abs(d32 - d64)[on].max()),
                             ker=float(np.abs(got["dist"].astype(np.float64) - d64)[on].max())))
    return rows


def test_assign_against_float64(accuracy):
    """Measured on MI355X (maxima over the 24 cases, absolute error of the winning distance): float32 torch 2.85e-7,
    kernel 7.17e-8, ratio 0.25 of the 2 allowed; no counting slot of the 15960 lies inside the margin, and neither
    the kernel's nor the float32 reference's labels differ from float64 anywhere.  Per case:
    profiles/parts_accuracy.txt."""
    bound = 2 * max(r["ref"] for r in accuracy)
    worst = max(r["ker"] for r in accuracy)
    left = total = left32 = 0
    for r in accuracy:
        g, on = r["got"], r["on"]
        sure = on & (r["margin"] > bound)
        left += int((on & ~sure).sum())
        left32 += int((r["l32"] != r["l64"])[on].sum())
        total += int(on.sum())
        print("P %-4d M %-2d dist f32 torch %.2e | kernel %.2e; labels off float64 where the margin allows: f32 torch %d, "
              "kernel %d; slots inside the margin %d of %d" % (
                  r["P"], r["M"], r["ref"], r["ker"], int((r["l32"] != r["l64"])[sure].sum()),
                  int((g["label"] != r["l64"])[sure].sum()), int((on & ~sure).sum()), int(on.sum())))
        assert (r["pts"][1] < 0).any() and r["count"][1] < max(r["P"], 2)
        assert np.array_equal(g["label"][sure], r["l64"][sure]), (r["P"], r["M"])
        assert np.array_equal(r["l32"][sure], r["l64"][sure]), (r["P"], r["M"])  # the reference alone meets it
        assert (g["label"][~on] == -1).all() and (g["dist"][~on] == 0).all()
        assert ((g["label"][on] >= 0) & (g["label"][on] < r["M"])).all()
        for b in range(3):
            cnt, dist = pr.part_sums(g["label"][b], g["dist"][b].astype(np.float64), r["M"])
            assert np.array_equal(g["part_count"][b], cnt), (r["P"], r["M"], b)
            np.testing.assert_allclose(g["part_dist"][b], dist, rtol=1e-12, atol=0)
            assert g["changed"][b] == int(((g["label"][b] != r["prev"][b]) & on[b]).sum()), (r["P"], r["M"], b)
    print("dist maxima over the set: f32 torch %.3e kernel %.3e, ratio %.3f of the 2 allowed; slots inside the margin "
          "%d of %d (%.3f %%); float32 torch labels off float64 anywhere %d" % (
              bound / 2, worst, 2 * worst / bound, left, total, 100.0 * left / total, left32))
    assert worst <= bound, (worst, bound)
    assert left <= 0.02 * total, (left, total)


# ------------------------------------------------------------------------------- 2. ties and degenerate rows
def test_ties_go_to_the_lowest_part_and_a_row_without_a_distance_never_wins():
    from sqr import fit, losses
    import _recover_ref as rr
    d = pc.golden()
    pts = _dev(d["clouds"][:2, :300])
    lab = d["labels"][:2].astype(np.float32)
    other = d["labels"][2:4].astype(np.float32)
    # two identical rows: the lower m everywhere, also behind a different row
    for rows, allowed in ((np.stack([lab, lab], 1), {0}), (np.stack([other, lab, lab], 1), {0, 1})):
        label, dist = fit.assign_points(pts, _dev(rows))
        assert set(label.unique().tolist()) <= allowed
    same0 = fit.assign_points(pts, _dev(np.stack([lab], 1)))
    assert _same(fit.assign_points(pts, _dev(np.stack([lab, lab], 1))), same0)
    # a row whose distances are not finite (NaN size) never wins against a finite one, wherever it stands
    bad = lab.copy()
    bad[:, 0] = np.nan
    for k in range(3):
        rows = [other, lab]
        rows.insert(k, bad)
        want = fit.assign_points(pts, _dev(np.stack([other, lab], 1)))
        got = fit.assign_points(pts, _dev(np.stack(rows, 1)))
        order = [i for i in range(3) if i != k]  # rows 0, 1 of `want` are rows order[0], order[1] of `got`
        assert bool((got[0] != k).all())
        assert torch.equal(got[0], torch.tensor(order, device=DEV, dtype=torch.int32)[want[0].long()])
        assert _same(got[1], want[1])
    # nothing but such rows: label 0, distance +inf
    label, dist = fit.assign_points(pts, _dev(np.stack([bad, bad], 1)))
    assert bool((label == 0).all()) and bool(torch.isinf(dist).all())
    # M = 16 with 15 empty parts: sixteen identical rows, and a recovery from labels that are all 0
    out = losses.pts_assign(pts, _dev(np.stack([lab] * 16, 1)))
    assert bool((out["label"] == 0).all()) and _same(out["dist"], same0[1])
    assert out["part_count"].tolist() == [[300] + [0] * 15] * 2 and not bool(out["part_dist"][:, 1:].any())
    zeros = torch.zeros(2, 300, dtype=torch.int32, device=DEV)
    p, label, energy, info = fit.recover_parts(pts, 16, labels=zeros, rounds=1, iters0=5, return_info=True)
    one = fit.recover_points(pts, iters=5)
    assert _same(p[:, 0], one[0]) and _same(energy[:, 0], one[1])
    default = torch.tensor(rr.default_start(1.0), device=DEV)
    assert bool((p[:, 1:] == default).all()) and not bool(energy[:, 1:].any())
    assert info["changed"].shape == (1, 2) and "seeds" not in info


# ------------------------------------------------------------------------------- 3. the part source is the masked list
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("P", [64, 257, 1024])
def test_labeled_calls_are_bitwise_the_calls_on_nan_masked_copies(P, M):
    from sqr import losses
    d = pc.golden()
    rng = np.random.default_rng(11 * P + M)
    B, K = 2, 2
    pts = np.stack([np.tile(d["clouds"][b], (2, 1))[:: 1024 // P][:P] for b in range(B)]).astype(np.float32)
    assert pts.shape == (B, P, 3)
    pts[0, 3] = np.nan                                    # a hole
    pts[1, P // 2, 2] = np.inf
    count = np.array([P, P - 5], np.int32)                # a short count, finite junk behind it
    pts[1, P - 5:] = 7.5
    label = rng.integers(0, M, size=(B, P)).astype(np.int32)
    label[0, 7], label[1, 9] = -1, M                      # labels that belong to no part
    masked = np.repeat(pts, M, axis=0).reshape(B, M, P, 3).copy()
    for m in range(M):
        masked[:, m][label != m] = np.nan
    masked = _dev(masked.reshape(B * M, P, 3))
    cnt_m = _dev(np.repeat(count, M))
    par = np.tile(d["labels"][:B, None, None], (1, M, K, 1)).transpose(2, 0, 1, 3)  # [K,B,M,12]
    par = _dev((par + 0.03 * rng.normal(size=par.shape)).astype(np.float32))
    dp, dc, dl = _dev(pts), _dev(count), _dev(label)
    got = losses.pts_labeled_lm_refine(dp, dc, dl, par, 3, 1e-3, 10.0, 0.1)
    want = losses.pts_lm_refine(masked, cnt_m, par.reshape(K, B * M, 12), 3, 1e-3, 10.0, 0.1)
    assert got[0].shape == (K, B, M, 12) and got[1].shape == (K, B, M)
    assert _same(tuple(x.reshape(K, B * M, *x.shape[3:]) for x in got), want)
    assert bool((got[2] <= got[1]).all()) and bool((got[2] > 0).all())
    assert _same(losses.pts_labeled_lm_refine(dp, dc, dl, par, 3, 1e-3, 10.0, 0.1), got)
    rgot = losses.pts_labeled_recover(dp, dc, dl, M, 4, 1.0, 1e-3, 10.0, 0.1)
    rwant = losses.pts_recover(masked, cnt_m, 4, 1.0, None, 1e-3, 10.0, 0.1)
    assert _same(tuple(x.reshape(B * M, *x.shape[2:]) for x in rgot[:3]), rwant[:3])
    assert _same({k: v.reshape(3, B * M, *v.shape[3:]) for k, v in rgot[3].items()}, rwant[3])
    assert _same(losses.pts_labeled_recover(dp, dc, dl, M, 4, 1.0, 1e-3, 10.0, 0.1), rgot)


# ------------------------------------------------------------------------------- 4. one part is recover_points
def test_one_part_and_one_round_is_recover_points():
    from sqr import fit
    d = pc.golden()
    pts = d["clouds"][:3].copy()
    pts[1, 40] = np.nan
    pts, cnt = _dev(pts), _dev(np.array([512, 512, 300], np.int32))
    p, label, energy, info = fit.recover_parts(pts, 1, cnt, rounds=1, return_info=True)
    want = fit.recover_points(pts, cnt)
    assert _same(p[:, 0], want[0]) and _same(energy[:, 0], want[1])
    lab = label.cpu().numpy()
    assert (lab[0] == 0).all() and lab[1, 40] == -1 and (np.delete(lab[1], 40) == 0).all()
    assert (lab[2, :300] == 0).all() and (lab[2, 300:] == -1).all()
    assert info["part_count"].tolist() == [[512], [511], [300]] and info["changed"].tolist() == [[0, 0, 0]]


# ------------------------------------------------------------------------------- 5. the seeding
def _scenes(parts):
    """Both scenes in one list of 2048 slots: (points [2,2048,3] f32 with finite junk behind scene A's 1536 points,
    count [2] i32)."""
    pts = np.full((2, 2048, 3), 7.5, np.float32)
    pts[0, :1536] = parts["a_points"]
    pts[1] = parts["b_points"]
    return pts, np.array([1536, 2048], np.int32)


@pytest.mark.parametrize("scene,row", [("a", 0), ("b", 1)])
def test_seeding_of_the_scenes_is_the_fixtures(parts, scene, row):
    from sqr import losses
    pts, cnt = _scenes(parts)
    M, n = len(parts[scene + "_seeds"]), int(cnt[row])
    label, centres, seeds = losses.pts_seed(_dev(pts), M, _dev(cnt), lloyd=int(parts["lloyd"]))
    torch.cuda.synchronize()
    assert np.array_equal(seeds[row].cpu().numpy(), parts[scene + "_seeds"])
    lab = label[row].cpu().numpy()
    assert np.array_equal(lab[:n], parts[scene + "_lloyd_label"]) and (lab[n:] == -1).all()
    c, want = centres[row].cpu().numpy(), parts[scene + "_centres"]
    ulps = np.abs(c.astype(np.float64) - want) / np.spacing(np.abs(want))
    print("scene %s: seeds %s, centres off the host's by at most %.1f float32 ulp" % (
        scene, seeds[row].tolist(), ulps.max()))
    assert ulps.max() <= 1
    # lloyd = 0: the nearest seed; the same call alone and again
    l0, c0, s0 = losses.pts_seed(_dev(pts), M, _dev(cnt), lloyd=0)
    assert _same(s0, seeds) and np.array_equal(c0[row].cpu().numpy(), pts[row][parts[scene + "_seeds"]])
    one = losses.pts_seed(_dev(pts[row:row + 1]), M, _dev(cnt[row:row + 1]), lloyd=int(parts["lloyd"]))
    assert _same(one, (label[row:row + 1], centres[row:row + 1], seeds[row:row + 1]))


def test_seeding_of_clouds_with_few_or_no_points():
    from sqr import losses
    d = pc.golden()
    pts = np.full((3, 6, 3), np.nan, np.float32)
    pts[0] = np.repeat(d["clouds"][0][:2], 3, axis=0)   # two distinct points, three times each
    pts[1, 4] = d["clouds"][1][0]                       # one point
    label, centres, seeds = losses.pts_seed(_dev(pts), 4, lloyd=2)
    for b in range(3):
        want = pr.seed(pts[b], 4, lloyd=2)
        assert np.array_equal(seeds[b].cpu().numpy(), want["seeds"]), b
        assert np.array_equal(label[b].cpu().numpy(), want["label"]), b
        assert np.array_equal(centres[b].cpu().numpy(), want["centres"]), b
    assert seeds.tolist() == [[3, 0, 0, 0], [4, 4, 4, 4], [-1, -1, -1, -1]]


# ------------------------------------------------------------------------------- 6. the chain on the scenes
@pytest.mark.parametrize("scene,row", [("a", 0), ("b", 1)])
def test_recover_parts_on_the_scenes(parts, scene, row):
    import classes
    from sqr import fit
    pts_np, cnt_np = _scenes(parts)
    pts, cnt = _dev(pts_np), _dev(cnt_np)
    M, n, T = len(parts[scene + "_seeds"]), int(cnt_np[row]), int(parts["rounds"])
    kw = dict(rounds=T, iters0=int(parts["iters0"]), iters=int(parts["iters"]), lloyd=int(parts["lloyd"]),
              e0=float(parts["e0"]))
    p, label, energy, info = fit.recover_parts(pts, M, cnt, return_info=True, **kw)
    torch.cuda.synchronize()
    assert p.shape == (2, M, 12) and label.shape == (2, 2048) and energy.shape == (2, M)
    assert p.dtype == torch.float32 and label.dtype == torch.int32 and energy.dtype == torch.float64
    lab = label[row].cpu().numpy()
    final = parts[scene + "_label_64"][-1]
    assert np.array_equal(final, parts[scene + "_label_32"][-1])
    assert np.array_equal(lab[:n], final) and (lab[n:] == -1).all()             # the fixture's final labels ...
    assert np.array_equal(parts[scene + "_part_of_64"][lab[:n]], parts[scene + "_true_label"])  # the true partition
    changed = info["changed"][:, row].tolist()
    assert len(changed) == T and changed[-1] == 0
    assert np.array_equal(info["seeds"][row].cpu().numpy(), parts[scene + "_seeds"])
    assert info["part_count"][row].tolist() == [int((final == m).sum()) for m in range(M)]
    acc = classes.IoUAccuracy(int(parts["iou_grid"]), "cpu", reduce=False)
    body = parts[scene + "_true_params"][parts[scene + "_part_of_64"]]
    iou = acc(torch.tensor(body, dtype=torch.float64), p[row].cpu().double()).numpy()
    print("scene %s: changed per round %s (f64 host %s)" % (scene, changed, parts[scene + "_changed_64"].tolist()))
    for m in range(M):
        print("  part %d: %d points, energy %.3e (f64 host %.3e, f32 host %.3e), mean radial distance %.3e, IoU %.4f "
              "(f32 host %.4f)" % (m, info["part_count"][row, m].item(), energy[row, m].item(),
                                   parts[scene + "_energy_64"][-1, m], parts[scene + "_energy_32"][-1, m],
                                   (info["part_dist"][row, m] / info["part_count"][row, m]).item(), iou[m],
                                   parts[scene + "_iou_32"][m]))
    assert (iou >= parts[scene + "_iou_32"] - 0.01).all(), iou
    assert np.abs(p[row, :, 8:].double().norm(dim=1).cpu().numpy() - 1).max() <= 1e-6
    # a cloud's row does not depend on the rest of the batch
    one = fit.recover_parts(pts[row:row + 1].contiguous(), M, cnt[row:row + 1], return_info=True, **kw)
    assert _same(one[:3], (p[row:row + 1], label[row:row + 1], energy[row:row + 1]))
    assert _same(one[3], {k: (v[:, row:row + 1] if k == "changed" else v[row:row + 1]) for k, v in info.items()})
    # labels= the true partition: no seeding, the same final labels
    given = torch.full((2, 2048), -1, dtype=torch.int32, device=DEV)
    given[row, :n] = _dev(final)
    given[1 - row] = label[1 - row]
    q, lab2, _, info2 = fit.recover_parts(pts, M, cnt, labels=given, return_info=True, **kw)
    assert torch.equal(lab2[row], label[row]) and "seeds" not in info2 and info2["changed"].shape == (T, 2)
    del q
    # captured in a graph and replayed twice: the eager results bit for bit
    buf = pts.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = fit.recover_parts(buf, M, cnt, return_info=True, **kw)
    for _ in range(2):
        for t in res[:3] + tuple(res[3].values()):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert _same(res[:3], (p, label, energy)) and _same(res[3], info)


# ------------------------------------------------------------------------------- 7. the command line
def test_recover_points_script_with_parts(tmp_path, capsys, parts):
    from conftest import PKG
    from sqr import fit
    spec = importlib.util.spec_from_file_location("sq_recover_points", os.path.join(PKG, "recover_points.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    npy, out_npy = tmp_path / "scene.npy", tmp_path / "labels.npy"
    np.save(npy, parts["a_points"])
    want = fit.recover_parts(_dev(parts["a_points"][None]), 3, return_info=True)
    a, e, t, q = mod.main(["--points", str(npy), "--parts", "3", "--labels-out", str(out_npy), "--device", DEV])
    out = capsys.readouterr().out
    assert re.search(r"Recovered 3 parts \(1536 points, 3 rounds, 30 Levenberg-Marquardt", out), out
    blocks = re.findall(r"Part (\d) \((\d+) points, mean radial distance (\S+), LeastSquares energy (\S+)\):", out)
    assert [int(b[0]) for b in blocks] == [0, 1, 2] and [int(b[1]) for b in blocks] == want[3]["part_count"][0].tolist()
    assert out.count("Size a:") == 3 and out.count("Rotation q:") == 3
    assert np.array_equal(np.concatenate([a, e, t, q], 1), want[0][0].cpu().numpy())
    labels = np.load(out_npy)
    assert labels.dtype == np.int32 and np.array_equal(labels, want[1][0].cpu().numpy())
    assert np.array_equal(labels, parts["a_label_64"][-1])
    for m, b in enumerate(blocks):
        assert float(b[3]) == pytest.approx(want[2][0, m].item(), rel=1e-5)
    # without --parts the output is the single-body one
    mod.main(["--points", str(npy), "--iters", "2", "--device", DEV])
    out = capsys.readouterr().out
    assert "Recovered parameters (1536 points, 2 Levenberg-Marquardt" in out and "Part" not in out


# ------------------------------------------------------------------------------- 8. guard-filled buffers
GUARD = 64


@pytest.mark.parametrize("B,P,M", [(2, 300, 3), (1, 1024, 16)])
def test_c_abi_writes_inside_its_buffers_only(B, P, M):
    """Guard words around every output and the workspace of sqr_pts_seed, sqr_pts_assign and sqr_pts_recover_parts,
    each given exactly the bytes its _workspace_bytes asks for; a workspace one byte short launches nothing."""
    from sqr._lib import lib, ptr, stream_ptr
    L = lib()
    d = pc.golden()
    pts = _dev(np.stack([np.tile(d["clouds"][b], (2, 1))[:P] for b in range(B)]))
    cnt = _dev(np.array([P, P - 7][:B], np.int32))
    par = _dev(np.tile(d["labels"][:M], (B, 1, 1)).astype(np.float32))
    f, st = -7.25, stream_ptr(DEV)
    f32, f64, i32 = torch.float32, torch.float64, torch.int32

    def run(name, specs, call):
        wsb = specs.pop("ws")
        fills = dict({k: v[2] for k, v in specs.items()}, ws=0xA5)
        specs["ws"] = (wsb, torch.uint8, 0xA5)
        bufs = {k: torch.full((n + 2 * GUARD,), fill, dtype=dt, device=DEV) for k, (n, dt, fill) in specs.items()}
        views = {k: bufs[k][GUARD:GUARD + specs[k][0]] for k in bufs}
        v = {k: ptr(x) for k, x in views.items()}
        assert call(v, wsb - 1) == -1 and b"workspace" in L.sqr_last_error_string(), name
        torch.cuda.synchronize()
        assert all(bool((bufs[k] == fills[k]).all()) for k in bufs), name  # nothing was launched
        assert call(v, wsb) == 0, (name, L.sqr_last_error_string())
        torch.cuda.synchronize()
        for k, buf in bufs.items():
            n = specs[k][0]
            assert bool((buf[:GUARD] == fills[k]).all()) and bool((buf[GUARD + n:] == fills[k]).all()), (name, k)
            if k != "ws":
                assert bool((views[k] != fills[k]).all()), (name, k)
        return views

    s = run("seed", dict(label=(B * P, i32, -7), centres=(B * M * 3, f32, f), seeds=(B * M, i32, -7),
                         ws=L.sqr_pts_seed_workspace_bytes(B, P, M)),
            lambda v, n: L.sqr_pts_seed(ptr(pts), ptr(cnt), B, P, M, 2, v["label"], v["centres"], v["seeds"], v["ws"], n, st))
    prev = s["label"].clone()
    run("assign", dict(label=(B * P, i32, -7), dist=(B * P, f32, f), count=(B * M, i32, -7), pdist=(B * M, f64, f),
                       changed=(B, i32, -7), ws=L.sqr_pts_assign_workspace_bytes(B, P, M)),
        lambda v, n: L.sqr_pts_assign(ptr(pts), ptr(cnt), ptr(par), ptr(prev), B, P, M, v["label"], v["dist"], v["count"],
                                      v["pdist"], v["changed"], v["ws"], n, st))
    for T in (1, 2):  # the rounds alternate between the outputs and the workspace: both parities
        o = run("recover_parts", dict(params=(B * M * 12, f32, f), label=(B * P, i32, -7), energy=(B * M, f64, f),
                                      dist=(B * P, f32, f), count=(B * M, i32, -7), pdist=(B * M, f64, f),
                                      changed=(T * B, i32, -7), seeds=(B * M, i32, -7), centres=(B * M * 3, f32, f),
                                      ws=L.sqr_pts_recover_parts_workspace_bytes(B, P, M)),
                lambda v, n: L.sqr_pts_recover_parts(ptr(pts), ptr(cnt), None, B, P, M, T, 3, 2, 2, 1.0, 1e-3, 10.0, 0.1,
                                                     v["params"], v["label"], v["energy"], v["dist"], v["count"],
                                                     v["pdist"], v["changed"], v["seeds"], v["centres"], v["ws"], n, st))
        assert int(o["count"].sum()) == int((o["label"] >= 0).sum()) == (2 * P - 7 if B == 2 else P)
    # arguments that launch nothing
    z = ptr(pts)
    assert L.sqr_pts_assign(z, None, z, None, B, P, 17, z, z, z, z, None, z, 1 << 30, st) == -1
    assert L.sqr_pts_seed(z, None, 1366, P, 16, 1, z, z, z, z, 1 << 40, st) == -1
    assert L.sqr_pts_recover_parts(z, None, None, B, P, M, 0, 3, 2, 2, 1.0, 1e-3, 10.0, 0.1, z, z, z, z, z, z, z, z, z, z,
                                   1 << 40, st) == -1
