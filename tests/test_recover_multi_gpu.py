"""The multi-start recovery on the GPU: the six starts (sqr_lsq_starts6), the batched refinement
(sqr_lsq_lm_refine_multi), the whole chain with the scored selection (sqr_lsq_recover_multi, sqr.fit.recover with
starts="depth", free_space, extra_starts) and the two command lines' new switches.

The host rules are tests/_free_space_ref.py on tests/_recover_ref.py; the float64 and float32 host pipelines on
the ten example images are the fixture tests/golden/recover_multi.npz (its generator beside it), so no test here
runs a host loop.

Tolerances, derived as in tests/test_recover_gpu.py.  Starts 3..5: a and t are float32 roundings of float64
values recomputed here from the returned frame: one float32 ulp; q is bitwise that of starts 0..2.  The chain:
accept decisions differ between precisions, so no trajectory and no single start is compared: per image the
winning score over the float64 host pipeline's, at least 1, within twice the worst such ratio of the float32 host
pipeline; that doubled ratio is also "the deviation" by which the float64 pipeline's two best scores must differ
for its winner to be demanded of the kernel.  At least seven of the ten winners reach IoU 0.9 against their
labels (the float64 pipeline: eight; the three-start recovery: six).  Every identity between entry points is
bitwise.  Measured on an MI355X: profiles/recover_multi_accuracy.txt holds the printed lines.
"""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import _free_space_ref as fsr
import _lm_ref
import _recover_ref as rr
from _golden import load
from _lsq_cases import build_images, example

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _resample(ex, idx, H, W):
    rows, cols = np.arange(H) * 256 // H, np.arange(W) * 256 // W
    return np.ascontiguousarray(ex[np.asarray(idx)][:, :, rows][:, :, :, cols])


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32)).astype(np.float32)).astype(np.float64)


# ------------------------------------------------------------------------------------------ the six starts
def _start_cases():
    ex, _ = example()
    return [("examples_R32", 32, ex), ("examples_R33", 33, ex[:4]), ("examples_R8", 8, ex[4:8]),
            ("resize_50x37_R32", 32, _resample(ex, [1, 8], 50, 37)),
            ("zero_R32", 32, build_images("zero", [0, 1], ex)), ("onepix_R32", 32, build_images("onepix", [3, 4, 5], ex))]


def test_six_starts():
    from sqr import losses
    moved = 0
    for name, R, true in _start_cases():
        img = torch.tensor(true, device=DEV)
        s3, i3 = losses.lsq_starts(img, R)
        s6, i6 = losses.lsq_starts6(img, R, 1.0, 1.0)
        s0, _ = losses.lsq_starts6(img, R, 1.0, 0.0)
        sh, _ = losses.lsq_starts6(img, R, 0.5, 0.5)
        torch.cuda.synchronize()
        assert s6.dtype == torch.float32 and s6.shape == (6, len(true), 12)
        assert torch.equal(s6[:3], s3) and torch.equal(s0[:3], s3) and torch.equal(s0[3:], s3), name
        for k in i3:
            assert torch.equal(i3[k], i6[k]), (name, k)
        assert torch.equal(s6[3:, :, 8:], s3[:, :, 8:]) and torch.equal(s6[3:, :, 3:5], s3[:, :, 3:5]), name
        assert bool((sh[:, :, 3:5] == 0.5).all())
        S, Sh, frame, count = s6.cpu().numpy(), sh.cpu().numpy(), i6["frame"].cpu().numpy(), i6["count"].cpu().numpy()
        pts = [p.numpy().astype(np.float64) for p in _lm_ref.points_of(true, R, torch.float32)]
        for b, P in enumerate(pts):
            if count[b] == 0:
                assert np.array_equal(S[:, b], np.tile(rr.default_start(1.0), (6, 1))), (name, b)
                continue
            V = frame[b]
            for got, depth in ((S, 1.0), (Sh, 0.5)):
                proj = V.T @ P
                lo, hi = proj.min(1), proj.max(1)
                j = fsr.depth_axis(V)
                grow = depth * (hi[j] - lo[j])
                if V[2, j] > 0:
                    lo[j] -= grow
                else:
                    hi[j] += grow
                half, mid = 0.5 * (hi - lo), 0.5 * (hi + lo)
                for k in range(3):
                    s = got[3 + k, b]
                    ax = [(k + i) % 3 for i in range(3)]
                    a = np.clip(half[ax].astype(np.float32), np.float32(0.05), np.float32(1))
                    t = np.clip((V[:, ax] @ mid[ax]).astype(np.float32), np.float32(0), np.float32(1))
                    assert (np.abs(s[0:3].astype(np.float64) - a) <= _ulp32(a)).all(), (name, b, k, s[0:3], a)
                    assert (np.abs(s[5:8].astype(np.float64) - t) <= _ulp32(t)).all(), (name, b, k, s[5:8], t)
            moved += int(not np.array_equal(S[3, b], S[0, b]))
    assert moved == 20  # the depth-aware starts are other starts on every image with a body (10 + 4 + 4 + 2)


def test_starts6_argument_checks():
    from sqr import losses
    ex, _ = example()
    img = torch.tensor(ex[:2], device=DEV)
    with pytest.raises(RuntimeError):
        losses.lsq_starts6(img, 32, 1.0, -0.5)
    with pytest.raises(RuntimeError):
        losses.lsq_starts6(img, 32, 0.05, 1.0)
    with pytest.raises(ValueError):
        losses.lsq_starts6(torch.tensor(ex[:2]), 32)


# ------------------------------------------------------------------------------------------ batched refinement
@pytest.mark.parametrize("R,idx", [(32, [0, 5, 7]), (8, [2, 3, 9]), (33, [1, 4, 6])])
def test_lm_refine_multi_is_three_refine_lm_calls(R, idx):
    from sqr import fit, losses
    ex, labels = example()
    img = torch.tensor(ex[idx], device=DEV)
    starts, _ = losses.lsq_starts(img, R)
    starts[2] = torch.tensor(labels[idx], device=DEV) * 1.1  # unprojected, partly out of range
    out = losses.lm_refine_multi(img, starts, R, 3, 1e-3, 10.0, 0.1)
    torch.cuda.synchronize()
    assert [tuple(o.shape) for o in out] == [(3, 3, 12), (3, 3), (3, 3), (3, 3)]
    assert [o.dtype for o in out] == [torch.float32, torch.float64, torch.float64, torch.int32]
    for k in range(3):
        one = fit.refine_lm(img, starts[k], iters=3, render_size=R, return_info=True)
        for got, want, what in zip(out, one, ("params", "before", "after", "accepted")):
            assert torch.equal(got[k], want), (k, what)
    assert bool((out[3] > 0).any())
    again = losses.lm_refine_multi(img, starts, R, 3, 1e-3, 10.0, 0.1)
    assert all(torch.equal(x, y) for x, y in zip(out, again))
    with pytest.raises(ValueError):
        losses.lm_refine_multi(img, starts[:, :2], R, 3, 1e-3, 10.0, 0.1)


# ------------------------------------------------------------------------------------------ the whole chain
def test_three_starts_without_score_is_sqr_lsq_recover():
    from sqr import losses
    ex, _ = example()
    for R, true, iters in ((32, ex, 30), (33, _resample(ex, [2, 7, 9], 50, 37), 4)):
        img = torch.tensor(true, device=DEV)
        old = losses.lsq_recover(img, R, iters, 1.0, 1e-3, 10.0, 0.1)
        out, energy, fs, index, info = losses.lsq_recover_multi(img, R, iters, 3, 1.0, 1.0, None, 1e-3, 10.0, 0.1, 0.0,
                                                                1.0 / 255.0)
        torch.cuda.synchronize()
        new = (out, energy, index, info["params"], info["energy_before"], info["energy_after"], info["accepted"])
        for x, y, what in zip(new, old, ("params", "energy", "index", "all_params", "before", "after", "accepted")):
            assert torch.equal(x, y), (R, what)
        assert torch.equal(info["score"], info["energy_after"])
        assert torch.equal(info["starts"], losses.lsq_starts(img, R)[0])
        assert torch.equal(info["energy_fs"].reshape(-1), losses.free_space_energy(img, info["params"].reshape(-1, 12), R))


@pytest.fixture(scope="module")
def run():
    """sqr.fit.recover(starts="depth", free_space=1) on the ten example images, R = 32, 30 iterations.  Once."""
    from sqr import fit
    ex, labels = example()
    img = torch.tensor(ex, device=DEV)
    params, energy, index, info = fit.recover(img, iters=30, render_size=32, starts="depth", free_space=1.0,
                                              return_info=True)
    torch.cuda.synchronize()
    assert torch.equal(img, torch.tensor(ex, device=DEV))  # the input is left alone
    assert params.dtype == torch.float32 and params.shape == (10, 12) and not params.requires_grad
    assert energy.dtype == torch.float64 and energy.shape == (10,)
    assert index.dtype == torch.int32 and index.shape == (10,)
    assert info["params"].shape == (6, 10, 12) and info["starts"].shape == (6, 10, 12)
    for k in ("energy_before", "energy_after", "energy_fs", "score", "accepted"):
        assert info[k].shape == (6, 10), k
    assert info["winner_energy_fs"].shape == (10,) and info["count"].shape == (10,) and info["frame"].shape == (10, 3, 3)
    return dict(img=img, labels=labels, params=params, energy=energy, index=index, info=info,
                fix=load("recover_multi.npz"))


def test_recover_multi_descends_selects_the_lowest_score_and_returns_valid_parameters(run):
    from sqr import fit, losses
    info = run["info"]
    before, after = info["energy_before"].cpu().numpy(), info["energy_after"].cpu().numpy()
    fs, score = info["energy_fs"].cpu().numpy(), info["score"].cpu().numpy()
    acc, idx = info["accepted"].cpu().numpy(), run["index"].cpu().numpy()
    for i in range(10):
        print("image %d: after %s fs %s accepted %s start %d" % (
            i, " ".join("%.3e" % v for v in after[:, i]), " ".join("%.3e" % v for v in fs[:, i]), acc[:, i].tolist(),
            idx[i]))
    assert np.isfinite(before).all() and np.isfinite(after).all() and np.isfinite(fs).all() and (fs >= 0).all()
    assert (after <= before).all() and (acc >= 0).all() and (acc <= 30).all()
    assert np.array_equal(score, after + 1.0 * fs)
    assert np.array_equal(idx, rr.select(score)) and np.array_equal(idx, fsr.select_scored(after, fs, 1.0))
    ar = np.arange(10)
    assert np.array_equal(run["energy"].cpu().numpy(), after[idx, ar])
    assert np.array_equal(info["winner_energy_fs"].cpu().numpy(), fs[idx, ar])
    assert (score[idx, ar] <= score).all()
    out = run["params"].cpu().numpy()
    assert np.array_equal(out, info["params"].cpu().numpy()[idx, ar])
    # the parts are the public entry points, bitwise
    s6, _ = losses.lsq_starts6(run["img"], 32, 1.0, 1.0)
    assert torch.equal(info["starts"], s6)
    ref = losses.lm_refine_multi(run["img"], s6, 32, 30, 1e-3, 10.0, 0.1)
    for got, want in zip((info["params"], info["energy_before"], info["energy_after"], info["accepted"]), ref):
        assert torch.equal(got, want)
    assert torch.equal(info["energy_fs"].reshape(-1), losses.free_space_energy(run["img"], info["params"].reshape(-1, 12), 32))
    # starts 0..2 of the six end where today's recovery takes them
    _, _, _, old = fit.recover(run["img"], iters=30, render_size=32, return_info=True)
    assert torch.equal(info["params"][:3], old["params"]) and torch.equal(info["energy_after"][:3], old["energy_after"])
    assert np.isfinite(out).all()
    assert (out[:, 0:3] >= np.float32(0.05)).all() and (out[:, 0:3] <= 1).all()
    assert (out[:, 3:5] >= np.float32(0.1)).all() and (out[:, 3:5] <= 1).all()
    assert (out[:, 5:8] >= 0).all() and (out[:, 5:8] <= 1).all()
    assert np.abs(np.linalg.norm(out[:, 8:].astype(np.float64), axis=1) - 1).max() <= 1e-6
    np.testing.assert_allclose(np.swapaxes(info["starts"].cpu().numpy(), 0, 1), run["fix"]["starts_64"], rtol=0, atol=2e-6)


def test_recover_multi_winning_score_and_winner_vs_float64_pipeline(run):
    fix = run["fix"]
    s64, s32 = fix["score_64"], fix["score_32"]
    ar = np.arange(10)
    w64, w32 = s64[ar, fix["winner_64"]], s32[ar, fix["winner_32"]]
    score = run["info"]["score"].cpu().numpy()
    idx = run["index"].cpu().numpy()
    win = score[idx, ar]
    rk, r32 = np.maximum(win / w64, 1), np.maximum(w32 / w64, 1)
    deviation = 2 * r32.max()
    second = np.sort(s64, axis=1)[:, 1]
    for i in range(10):
        print("image %d winner: float64 %.6g (start %d, runner-up x%.3f) | float32 host %.6g (start %d, %.4f) | kernel "
              "%.6g (start %d, %.4f)" % (i, w64[i], fix["winner_64"][i], second[i] / w64[i], w32[i], fix["winner_32"][i],
                                         w32[i] / w64[i], win[i], idx[i], win[i] / w64[i]))
    print("worst winner ratio: float32 host %.4f kernel %.4f (bound %.4f)" % (r32.max(), rk.max(), deviation))
    assert (rk <= deviation).all(), (rk, deviation)
    clear = second / w64 > deviation
    print("float64 winner demanded on images %s" % np.nonzero(clear)[0].tolist())
    assert clear.sum() >= 5 and np.array_equal(idx[clear], fix["winner_64"][clear]), (idx, fix["winner_64"], clear)


def test_recover_multi_iou_floor(run):
    """At least seven of the ten winners reach IoU 0.9 (grid 64) against their labels; the float64 host pipeline
    has eight, and the three-start recovery selected by point energy six."""
    import classes
    iou = classes.IoUAccuracy(64, DEV, reduce=False)(torch.tensor(run["labels"], device=DEV), run["params"]).cpu().numpy()
    for i in range(10):
        print("image %d: IoU %.3f (float64 host pipeline %.3f)" % (i, iou[i], run["fix"]["iou_winner_64"][i]))
    print("winners with IoU >= 0.9: %d of 10 (float64 host pipeline %d), mean %.3f"
          % ((iou >= 0.9).sum(), (run["fix"]["iou_winner_64"] >= 0.9).sum(), iou.mean()))
    assert (iou >= 0.9).sum() >= 7, iou


def test_extra_starts_compete(run):
    from sqr import fit
    labels = torch.tensor(run["labels"], device=DEV)
    params, energy, index, info = fit.recover(run["img"], iters=30, render_size=32, starts="depth", free_space=1.0,
                                              extra_starts=labels, return_info=True)
    torch.cuda.synchronize()
    assert info["params"].shape == (7, 10, 12) and torch.equal(info["starts"][6], labels)
    one = fit.refine_lm(run["img"], labels, iters=30, render_size=32, return_info=True)
    for got, want in zip((info["params"][6], info["energy_before"][6], info["energy_after"][6], info["accepted"][6]), one):
        assert torch.equal(got, want)
    for k in ("params", "energy_before", "energy_after", "energy_fs", "score", "accepted", "starts"):
        assert torch.equal(info[k][:6], run["info"][k]), k
    score, idx = info["score"].cpu().numpy(), index.cpu().numpy()
    win = score[idx, np.arange(10)]
    assert (win <= score).all() and (win <= run["info"]["score"].cpu().numpy().min(0)).all()
    print("the label's start wins on %d of 10 images" % (idx == 6).sum())
    # [Kx,B,12] extras on three classic starts, without a score
    two = torch.stack([labels, run["params"]])
    p2, e2, i2, info2 = fit.recover(run["img"], iters=2, render_size=32, extra_starts=two, return_info=True)
    assert info2["params"].shape == (5, 10, 12) and torch.equal(info2["score"], info2["energy_after"])
    assert torch.equal(e2, info2["energy_after"].min(0).values) and int(i2.max()) <= 4
    with pytest.raises(ValueError):
        fit.recover(run["img"], extra_starts=labels[:3])
    with pytest.raises(ValueError):
        fit.recover(run["img"], starts="deep")


def test_recover_multi_captured_in_a_graph_replays_bitwise(run):
    from sqr import fit
    kw = dict(iters=2, render_size=32, starts="depth", free_space=1.0)
    src = run["img"][[3, 7]].contiguous()
    other = run["img"][[8, 1]].contiguous()
    eager, eager_other = fit.recover(src, **kw), fit.recover(other, **kw)
    img = src.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = fit.recover(img, **kw)
    for s, want in ((src, eager), (other, eager_other)):
        img.copy_(s)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(res, want))


GUARD = 64


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def test_c_abi_writes_inside_its_buffers_only():
    """Guard words around every output and the workspace of sqr_lsq_recover_multi, given exactly the bytes its
    _workspace_bytes asks for; bad arguments are errors and launch nothing."""
    from sqr._lib import lib, ptr, stream_ptr
    L = lib()
    ex, labels = example()
    B, R, K = 3, 33, 7
    t = torch.tensor(_resample(ex, [0, 4, 9], 50, 37)[:, 0], device=DEV).contiguous()
    extra = torch.tensor(labels[[0, 4, 9]], device=DEV).contiguous()
    wsb = L.sqr_lsq_recover_multi_workspace_bytes(K, B, R)
    assert wsb >= B * 15 * 8 + L.sqr_lsq_lm_refine_workspace_bytes(K * B, R) + B * 4
    f = -7.25
    spec = [("out", B * 12, torch.float32, f), ("energy", B, torch.float64, f), ("fs", B, torch.float64, f),
            ("index", B, torch.int32, -7), ("starts", K * B * 12, torch.float32, f), ("allp", K * B * 12, torch.float32, f),
            ("before", K * B, torch.float64, f), ("after", K * B, torch.float64, f), ("allfs", K * B, torch.float64, f),
            ("score", K * B, torch.float64, f), ("acc", K * B, torch.int32, -7), ("ws", wsb, torch.uint8, 0xA5)]
    bufs = {k: _guarded(n, dt, fill) for k, n, dt, fill in spec}

    def call(nbytes=wsb, nstarts=6, Kx=1, w=1.0, depth=1.0):
        rc = L.sqr_lsq_recover_multi(ptr(t), B, 50, 37, R, 3, nstarts, 1.0, depth, ptr(extra), Kx, 1e-3, 10.0, 0.1, w,
                                     1.0 / 255.0, *[ptr(bufs[k][1]) for k, _, _, _ in spec], nbytes, stream_ptr(DEV))
        torch.cuda.synchronize()
        return rc

    assert call(nbytes=wsb - 1) == -1 and b"workspace" in L.sqr_last_error_string()
    assert call(nstarts=4) == -1 and b"nstarts" in L.sqr_last_error_string()
    assert call(w=-1.0) == -1 and call(depth=-1.0) == -1 and call(Kx=-1) == -1
    assert call(Kx=30000) == -1 and b"65535" in L.sqr_last_error_string()
    assert all(bool((buf == fill).all()) for (k, _, _, fill), (buf, _) in zip(spec, bufs.values()))  # nothing launched
    assert call() == 0, L.sqr_last_error_string()
    for (k, n, _, fill), (buf, view) in zip(spec, bufs.values()):
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all()), k
        if k != "ws":
            assert bool((view != fill).all()), k
    assert torch.equal(bufs["starts"][1].view(K, B, 12)[6], extra)
    assert bool((bufs["index"][1] >= 0).all()) and bool((bufs["index"][1] < K).all())


# ------------------------------------------------------------------------------------------ the command lines
def _load_script(name):
    from conftest import PKG
    spec = importlib.util.spec_from_file_location("sq_%s_recover_multi" % name, os.path.join(PKG, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _write_bmp(path, img):
    """A bottom-up 24-bit BMP, as the scanner writes (tests/test_recover_gpu.py builds the same)."""
    h, w = img.shape
    stride = (w * 3 + 3) & ~3
    data = np.zeros((h, stride), np.uint8)
    data[:, :w * 3] = np.repeat(img[::-1], 3, axis=1)
    hdr = b"BM" + (54 + data.size).to_bytes(4, "little") + b"\0\0\0\0" + (54).to_bytes(4, "little")
    dib = (40).to_bytes(4, "little") + w.to_bytes(4, "little") + h.to_bytes(4, "little") + \
        (1).to_bytes(2, "little") + (24).to_bytes(2, "little") + b"\0" * 24
    path.write_bytes(hdr + dib + data.tobytes())


def test_test_py_starts_depth_free_space(tmp_path, capsys, run):
    bmp = tmp_path / "x.bmp"
    _write_bmp(bmp, load("example_images.npz")["images"][7])
    mod = _load_script("test")
    a, e, t, q = mod.main(["--image", str(bmp), "--device", DEV, "--classical", "--starts", "depth", "--free-space", "1"])
    out = capsys.readouterr().out
    m = re.search(r"Recovered parameters \(classical, 30 Levenberg-Marquardt iterations per start, LeastSquares "
                  r"energy (\S+), start (\d)\):", out)
    assert m, out
    # the same image as in the batch of ten: the same result
    assert np.array_equal(np.concatenate([a, e, t, q], 1)[0], run["params"][7].cpu().numpy())
    assert float(m.group(1)) == pytest.approx(run["energy"][7].item(), rel=1e-5) and int(m.group(2)) == run["index"][7].item()
    # the network's prediction as one more start (random weights here: it competes, it need not win)
    a2, _, _, q2 = mod.main(["--image", str(bmp), "--device", DEV, "--model", str(tmp_path / "none.pt"),
                             "--classical-starts", "--starts", "depth", "--free-space", "1", "--classical-iters", "3"])
    out = capsys.readouterr().out
    assert re.search(r"classical starts and the prediction, 3 Levenberg-Marquardt iterations per start, LeastSquares "
                     r"energy \S+, start [0-6]", out), out
    assert a2.shape == (1, 3) and abs(np.linalg.norm(q2.astype(np.float64)) - 1) <= 1e-6


def test_eval_random_starts_depth_free_space(tmp_path, capsys):
    import classes
    from sqr import fit, losses
    mod = _load_script("eval_random")
    res = tmp_path / "results.txt"
    ious = mod.main(["--method", "classical", "--starts", "depth", "--free-space", "1", "--n", "4", "--batch", "4",
                     "--render-size", "32", "--results", str(res), "--model", str(tmp_path / "none.pt"), "--device", DEV])
    capsys.readouterr()
    assert ious.shape == (4,) and np.isfinite(ious).all()
    labels = classes.sample_sq_params(np.random.default_rng(0), 4)
    x = losses.scan_render(torch.tensor(labels, device=DEV), 256, 255).unsqueeze(1)
    pred = fit.recover(x, starts="depth", free_space=1.0)[0].cpu().numpy()
    text, fmt = res.read_text(), mod.test_random._fmt
    for k in range(4):
        assert "Pred params: " + fmt(pred[k]) in text, k
