"""The point-list fitting stack without a GPU: the sqr_pts_* symbols and their argument checks (refused on the
host before the first HIP call, as tests/test_capi.py's), losses.pack_points, fit.normalize_points /
denormalize_params against their formulas, and the fixture tests/golden/points.npz against its generator."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from _golden import GOLDEN
from _points_cases import golden
from test_capi import declared_symbols

PTS = ("sqr_pts_normal_eq_workspace_bytes", "sqr_pts_normal_eq", "sqr_pts_lm_refine_workspace_bytes",
       "sqr_pts_lm_refine", "sqr_pts_starts_workspace_bytes", "sqr_pts_starts", "sqr_pts_recover_workspace_bytes",
       "sqr_pts_recover")
PMAX = 1 << 20


def test_header_declares_and_library_exports_the_point_list_symbols():
    from sqr import _lib
    syms = declared_symbols()
    L = _lib.lib()
    for s in PTS:
        assert s in syms and s in _lib.SIGNATURES and hasattr(L, s), s


def test_workspace_sizes():
    from sqr import _lib
    L = _lib.lib()
    for S, P in ((1, 1), (3, 256), (3, 257), (7, 300), (2, PMAX)):
        nblk = (P + 255) // 256
        neq = S * nblk * 256 * 8
        assert L.sqr_pts_normal_eq_workspace_bytes(S, P) == neq
        assert L.sqr_pts_lm_refine_workspace_bytes(S, P) == S * 326 * 8 + neq + S * 12 * 4
        assert L.sqr_pts_starts_workspace_bytes(S, P) == S * nblk * 16 * 8
        for K in (3, 5):
            region = max(S * nblk * 16 * 8, L.sqr_pts_lm_refine_workspace_bytes(K * S, P))
            assert L.sqr_pts_recover_workspace_bytes(K, S, P) == S * 15 * 8 + region + S * 4
    # the list of an image's slots needs what the image calls need
    for B, R in ((2, 8), (3, 12), (1, 32)):
        assert L.sqr_pts_normal_eq_workspace_bytes(B, R * R) == L.sqr_least_squares_normal_eq_workspace_bytes(B, R)
        assert L.sqr_pts_lm_refine_workspace_bytes(B, R * R) == L.sqr_lsq_lm_refine_workspace_bytes(B, R)
        assert L.sqr_pts_starts_workspace_bytes(B, R * R) == L.sqr_lsq_starts_workspace_bytes(B, R)
        assert L.sqr_pts_recover_workspace_bytes(3, B, R * R) == L.sqr_lsq_recover_multi_workspace_bytes(3, B, R)
    for fn in (L.sqr_pts_normal_eq_workspace_bytes, L.sqr_pts_lm_refine_workspace_bytes,
               L.sqr_pts_starts_workspace_bytes):
        assert fn(0, 8) == 0 and fn(8, 0) == 0
    assert L.sqr_pts_recover_workspace_bytes(0, 1, 1) == 0


class _Calls:
    """The four entry points with host buffers standing in for device ones: every call made here must be refused
    before the first launch, so none is ever read."""

    def __init__(self, L):
        self.L = L
        self.bufs = [(ctypes.c_double * 64)() for _ in range(12)]
        self.p = [ctypes.cast(b, ctypes.c_void_p) for b in self.bufs]
        self.big = 1 << 40  # "enough" for any size asked below; nothing is touched

    def normal_eq(self, S=2, B=2, P=64, ws=None):
        p = self.p
        return self.L.sqr_pts_normal_eq(p[0], p[1], None, S, B, P, p[2], p[3], p[4], p[5],
                                        self.big if ws is None else ws, None)

    def refine(self, K=2, B=2, P=64, iters=3, lambda0=1e-3, up=10.0, down=0.1, ws=None):
        p = self.p
        return self.L.sqr_pts_lm_refine(p[0], p[1], p[2], K, B, P, iters, lambda0, up, down, p[3], p[4], p[5], p[6],
                                        p[7], self.big if ws is None else ws, None)

    def starts(self, B=2, P=64, e0=1.0, ws=None):
        p = self.p
        return self.L.sqr_pts_starts(p[0], None, B, P, e0, p[1], p[2], p[3], p[4], p[5], p[6],
                                     self.big if ws is None else ws, None)

    def recover(self, B=2, P=64, iters=3, e0=1.0, Kx=0, extra=True, lambda0=1e-3, up=10.0, down=0.1, ws=None):
        p = self.p
        return self.L.sqr_pts_recover(p[0], p[1], B, P, iters, e0, p[2] if extra else None, Kx, lambda0, up, down,
                                      p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11],
                                      self.big if ws is None else ws, None)


REJECTED = [
    ("normal_eq", dict(P=0), b"P=0"),
    ("normal_eq", dict(P=PMAX + 1), b"P=1048577"),
    ("normal_eq", dict(S=3, B=2), b"S=3"),
    ("normal_eq", dict(S=0, B=0), b"S=0"),
    ("normal_eq", dict(S=65536, B=1), b"S=65536"),
    ("normal_eq", dict(ws=2 * 256 * 8 - 1), b"workspace"),
    ("refine", dict(P=0), b"P=0"),
    ("refine", dict(P=PMAX + 1), b"P=1048577"),
    ("refine", dict(K=256, B=256), b"K=256 x B=256"),
    ("refine", dict(K=0), b"K=0"),
    ("refine", dict(iters=-1), b"iters=-1"),
    ("refine", dict(lambda0=0.0), b"lambda0=0"),
    ("refine", dict(up=1.0), b"up=1"),
    ("refine", dict(down=1.0), b"down=1"),
    ("refine", dict(ws=15), b"workspace"),
    ("starts", dict(P=0), b"P=0"),
    ("starts", dict(P=PMAX + 1), b"P=1048577"),
    ("starts", dict(B=0), b"B=0"),
    ("starts", dict(B=65536), b"B=65536"),
    ("starts", dict(e0=0.05), b"e0"),
    ("starts", dict(ws=2 * 16 * 8 - 1), b"workspace"),
    ("recover", dict(P=0), b"P=0"),
    ("recover", dict(P=PMAX + 1), b"P=1048577"),
    ("recover", dict(B=21846), b"K=3 x B=21846"),
    ("recover", dict(B=13108, Kx=2), b"K=5 x B=13108"),
    ("recover", dict(Kx=1, extra=False), b"Kx=1"),
    ("recover", dict(Kx=-1), b"Kx=-1"),
    ("recover", dict(iters=-1), b"iters=-1"),
    ("recover", dict(e0=1.5), b"e0"),
    ("recover", dict(ws=15), b"workspace"),
]


@pytest.mark.parametrize("entry,kw,msg", REJECTED, ids=["%s-%s" % (e, "-".join(k)) for e, k, _ in REJECTED])
def test_bad_arguments_are_refused_on_the_host(entry, kw, msg):
    from sqr import _lib
    L = _lib.lib()
    assert getattr(_Calls(L), entry)(**kw) == -1  # SQR_E_INVALID_ARG
    err = L.sqr_last_error_string()
    who = {"refine": b"pts_lm_refine:"}.get(entry, b"pts_" + entry.encode() + b":")
    assert err.startswith(who) and msg in err, err


def test_the_largest_arguments_pass_the_range_checks():
    """P = 2^20 and K B = 65535 are inside the limits: the calls get as far as the workspace check."""
    from sqr import _lib
    L = _lib.lib()
    c = _Calls(L)
    assert c.normal_eq(S=65535, B=65535, P=PMAX, ws=1) == -1 and b"workspace" in L.sqr_last_error_string()
    assert c.refine(K=3, B=21845, P=PMAX, ws=1) == -1 and b"workspace" in L.sqr_last_error_string()
    assert c.starts(B=65535, P=PMAX, ws=1) == -1 and b"workspace" in L.sqr_last_error_string()
    assert c.recover(B=21845, P=PMAX, ws=1) == -1 and b"workspace" in L.sqr_last_error_string()
    assert c.recover(B=13107, Kx=2, P=1, ws=1) == -1 and b"workspace" in L.sqr_last_error_string()


def test_null_pointers_are_refused():
    from sqr import _lib
    L = _lib.lib()
    c = _Calls(L)
    p = c.p
    assert L.sqr_pts_normal_eq(p[0], None, None, 2, 2, 64, p[2], p[3], p[4], p[5], c.big, None) == -1
    assert b"null pointer" in L.sqr_last_error_string()
    assert L.sqr_pts_starts(p[0], None, 2, 64, 1.0, p[1], None, p[3], p[4], p[5], p[6], c.big, None) == -1
    assert b"null pointer" in L.sqr_last_error_string()
    assert L.sqr_pts_recover(p[0], None, 2, 64, 3, 1.0, None, 0, 1e-3, 10.0, 0.1, p[3], p[4], p[5], None, p[7], p[8],
                             p[9], p[10], p[11], c.big, None) == -1
    assert b"null pointer" in L.sqr_last_error_string()


def test_pack_points():
    from sqr.losses import pack_points
    rng = np.random.default_rng(0)
    clouds = [rng.normal(size=(n, 3)) for n in (5, 0, 9, 1)]
    pts, cnt = pack_points([torch.tensor(clouds[0]), clouds[1], clouds[2].astype(np.float32), torch.tensor(clouds[3])],
                           device="cpu")
    assert pts.shape == (4, 9, 3) and pts.dtype == torch.float32 and pts.is_contiguous()
    assert cnt.dtype == torch.int32 and cnt.tolist() == [5, 0, 9, 1]
    for i, c in enumerate(clouds):
        assert np.array_equal(pts[i, :len(c)].numpy(), c.astype(np.float32))
        assert bool(torch.isnan(pts[i, len(c):]).all())
    # a batch passes through, every slot counted
    batch = torch.tensor(rng.normal(size=(3, 7, 3)))
    pts, cnt = pack_points(batch)
    assert pts.shape == (3, 7, 3) and pts.dtype == torch.float32 and cnt.tolist() == [7, 7, 7]
    assert torch.equal(pts, batch.float())
    pts, cnt = pack_points([np.zeros((0, 3))], device="cpu")  # nothing at all: one NaN slot
    assert pts.shape == (1, 1, 3) and cnt.tolist() == [0] and bool(torch.isnan(pts).all())
    for bad in ([], [np.zeros((4, 2))], torch.zeros(3, 4), torch.zeros(2, 0, 3)):
        with pytest.raises(ValueError):
            pack_points(bad, device="cpu")


def test_gpu_entry_points_refuse_cpu_tensors():
    from sqr import fit, losses
    pts, par = torch.zeros(2, 8, 3), torch.zeros(2, 12)
    for call in (lambda: losses.point_normal_eq(pts, par), lambda: losses.point_energy(pts, par),
                 lambda: fit.refine_points(pts, par), lambda: fit.recover_points(pts)):
        with pytest.raises(ValueError, match="CPU tensor"):
            call()


def test_normalize_points_against_its_formulas():
    from sqr.fit import denormalize_params, normalize_points
    rng = np.random.default_rng(1)
    P = 40
    raw = (rng.normal(size=(6, P, 3)) * [3.0, 40.0, 0.2] + [-3.0, 12.0, 100.0]).astype(np.float32)
    raw[1, 7] = np.nan                       # a hole in the middle: not counted
    raw[1, 9, 1] = np.inf
    raw[2, 25:] = 1e6                        # behind count: not counted, whatever it holds
    raw[3] = raw[3, 0]                       # every point the same: the largest side is zero
    raw[4, :, 2] = 5.0                       # a flat cloud: one zero side, still scaled by the largest
    count = torch.tensor([P, P, 25, P, P, 0], dtype=torch.int32)
    out, scale, offset = normalize_points(torch.tensor(raw), count)
    assert out.dtype == scale.dtype == offset.dtype == torch.float32
    assert out.shape == (6, P, 3) and scale.shape == (6,) and offset.shape == (6, 3)
    for b in range(6):
        on = np.isfinite(raw[b]).all(1) & (np.arange(P) < int(count[b]))
        p = raw[b][on]
        if len(p) and (p.max(0) - p.min(0)).max() > 0:
            lo, hi = p.min(0), p.max(0)
            c, s = (lo + hi) / np.float32(2), np.float32(0.4) / (hi - lo).max()
        else:
            c, s = np.full(3, 0.5, np.float32), np.float32(1)
        assert b not in (3, 5) or (s == 1 and (c == 0.5).all())
        assert np.array_equal(scale[b].numpy(), s) and np.array_equal(offset[b].numpy(), c), b
        want = (raw[b] - c) * s + np.float32(0.5)
        assert np.array_equal(out[b].numpy()[on], want[on]), b
        assert np.isnan(out[b].numpy()[~on]).all(), b
        if b in (0, 1, 2, 4):  # inside the unit cube, the longest side 0.4 around 0.5
            q = out[b].numpy()[on]
            assert abs((q.max(0) - q.min(0)).max() - 0.4) <= 1e-6 and np.abs((q.max(0) + q.min(0)) / 2 - 0.5).max() <= 1e-6
    # count None: every finite slot
    out2, scale2, _ = normalize_points(torch.tensor(raw[:2]))
    assert torch.equal(scale2, scale[:2]) and torch.equal(torch.nan_to_num(out2), torch.nan_to_num(out[:2]))
    # the back-map, and the round trip of a body's size and position
    par = torch.tensor(rng.uniform(0.1, 0.9, size=(2, 6, 12)).astype(np.float32))
    back = denormalize_params(par, scale, offset)
    s, c = scale[:, None], offset
    assert torch.equal(back[..., 0:3], par[..., 0:3] / s) and torch.equal(back[..., 5:8], (par[..., 5:8] - 0.5) / s + c)
    assert torch.equal(back[..., 3:5], par[..., 3:5]) and torch.equal(back[..., 8:12], par[..., 8:12])
    t_world = torch.tensor(raw[0, 3])
    t_norm = (t_world - c[0]) * s[0, 0] + 0.5
    row = torch.cat([torch.full((3,), 0.2), torch.ones(2), t_norm, torch.tensor([0.0, 0, 0, 1])])[None]
    got = denormalize_params(row, scale[:1], offset[:1])[0]
    np.testing.assert_allclose(got[5:8].numpy(), t_world.numpy(), rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(got[0:3].numpy(), 0.2 / float(scale[0]), rtol=1e-6)


def _generator():
    spec = importlib.util.spec_from_file_location("gen_golden_points", os.path.join(GOLDEN, "gen_golden_points.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_fixture_is_what_the_issue_of_whole_body_clouds_promises():
    """Every cloud: 512 finite float32 points on the label's surface; both pipelines end on the same start with an
    energy of rounding size (the points are float32 roundings of surface points: 512 terms of (1e-7)^2 size), far
    below every losing start, and IoU 1 (float64) / at least 0.98 (float32) against the label."""
    gen = _generator()
    d = golden()
    assert d["clouds"].shape == (8, gen.N_ETA * gen.N_OMEGA, 3) and d["clouds"].dtype == np.float32
    assert np.isfinite(d["clouds"]).all() and d["labels"].shape == (8, 12)
    assert (int(d["iters"]), float(d["e0"]), int(d["iou_grid"])) == (gen.ITERS, gen.E0, gen.IOU_GRID)
    for tag in ("64", "32"):
        after, win = d["after_" + tag], d["winner_" + tag]
        assert after.shape == (8, 3) and (after <= d["before_" + tag]).all()
        best = after[np.arange(8), win]
        rest = np.sort(after, axis=1)[:, 1]
        assert (best <= 1e-11).all() and (rest >= 1e7 * best).all(), (best, rest)
    assert np.array_equal(d["winner_64"], d["winner_32"])
    assert (d["iou_64"] == 1.0).all() and (d["iou_32"] >= gen.IOU_MIN).all()
    # the energy of every label on its own cloud is of that size too: the sampler and the energy agree
    for i in range(8):
        pts = torch.tensor(d["clouds"][i].T.copy()).double()
        import _lm_ref
        r = _lm_ref.residuals(pts, torch.tensor(d["labels"][i]).double())
        assert float((r * r).sum()) <= 1e-11, i


def test_fixture_matches_its_generator_on_one_cloud():
    """Cloud 5's float64 rows regenerated (about 5 s).  Where the fixture was made every row is bitwise the stored
    one; another build may round a power differently.  The starts are float32 roundings of float64 values (equal,
    or an ulp apart: 1e-6 absolute is far above either); the energies at the starts follow to 1e-9 relative; the
    losing starts' final energies go through thirty accept decisions, 1e-6 relative as in
    tests/test_recover_cpu.py's twin; the winner's energy is rounding noise itself, so it is pinned by its size
    and by the parameters, which it determines to the square root of that noise: 1e-5."""
    gen = _generator()
    d = golden()
    i = 5
    assert np.array_equal(gen.sample_surface(d["labels"][i]), d["clouds"][i])
    r = gen.recover_cloud(d["clouds"][i], dt=np.float64)
    w = int(d["winner_64"][i])
    assert r["winner"] == w
    np.testing.assert_allclose(r["starts"], d["starts_64"][i], rtol=0, atol=1e-6)
    np.testing.assert_allclose(r["before"], d["before_64"][i], rtol=1e-9)
    lose = [k for k in range(3) if k != w]
    np.testing.assert_allclose(r["after"][lose], d["after_64"][i][lose], rtol=1e-6)
    assert r["after"][w] <= 1e-11
    np.testing.assert_allclose(r["params"][w], d["params_64"][i][w], rtol=0, atol=1e-5)
    assert abs(gen.iou_of(d["labels"][i], r["params"][w]) - d["iou_64"][i]) <= 2e-4
