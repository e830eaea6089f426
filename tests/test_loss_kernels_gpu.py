"""sqr_loss.hip's ImplicitLoss, ExplicitLoss, IoU and soft-render entry points through the C ABI, stage by
stage against the float64 references of _loss_ref.py (test_loss_gpu.py checks the same kernels end to end
through the classes; test_loss_ref_cpu.py checks the references).

Every call owns its buffers, so the workspace can be read back: partials [B][nblk][18] float32, 17 gradient
moments and the loss sum per block (block and index order: _loss_ref's docstring).

Shapes: the smallest at which each branch exists.

  ImplicitLoss (R, H, W, B)
    (2, 2, 2, 1)        the smallest legal R (no node near a surface: the 17 moments underflow to 0)
    (3, 3, 3, 2)
    (16, 16, 16, 2)     exactly one block of 256 rays
    (17, 17, 17, 2)     a second, partly filled block
    (33, 66, 66, 2)     five blocks, integer downsample
    (12, 24, 40, 2)     non-square target, non-integer ratio
    (129, 129, 129, 1)  the first size on 128-thread blocks
    (5 | 9 | 17, ., ., 3)  the dyadic rows: the zero fix on three whole planes
    finalize batches at R = 2: B = 65 (partly filled second wave), 1024 (last single-block size),
    1025 (multi-block finalize + loss_mean_kernel); B = 1 is the first row of the table
  ExplicitLoss R (nodes)
    1 (2) | 4 (5, dyadic rows) | 6 (8) and 9 (11): np.arange's extra node | 15 (16: one full block) |
    16 (17: two blocks); B = 2 (3 dyadic rows), and B = 1025 at R = 1

Inputs: the suite's parameter distribution; ImplicitLoss targets are the float64 depth image plus a random
sign times uniform [0.01, 0.3] per resized pixel, so no ray's sign(D - true) can differ between fp32 and
float64 and both signs occur (asserted in test_loss_ref_cpu.py).

Stage 1, kernel partials against float64 block moments.  Per slot e = max over samples and blocks of
|partial - ref| / (sum of |terms| + floor) (_loss_ref.slot_errors; the floor keeps blocks whose moments lie
below fp32's range out of the maximum, see there).  The kernel's e may be FACTOR = 4 times the e of the
float32 numpy evaluation of the same algorithm, computed at test time from the references alone: the margin
covers the hardware exp2 / log2 / rcp (about 1 ulp each, numpy's are correctly rounded or close) and the
wave-tree summation order.  Measured ratios: profiles/loss_stages_accuracy.txt.
Stage 2, the finalize from the GPU's own partials: the per-sample loss and the batch mean are float64 adds
in a fixed order and must equal _loss_ref.finalize's bitwise; each gradient entry is a float64 result
rounded once to fp32, the device chain may contract to FMAs: 2^-23 |g| + 1e-12 * (its chain on absolute
values).
Stage 3, sqr_loss_grad_scale: bitwise g * float32(gout).
End to end: every one of the 12 gradient components against sq_oracle, its error normalised by that
component's largest |g_ref| over the batch, at FACTOR times the float32 evaluation's, both as maxima over the
random-row cases (_component_check; on the dyadic rows the quaternion components vanish by symmetry and are
rounding noise in any evaluation); the reference's own loss_edges.npz, the renders and the IoU counts at the
suite's tolerances (loss 1e-4 relative, gradient 2e-4 of the sample's largest entry, depth 2e-4, counts
equal).

Every call checks guard words on both sides of every buffer it hands out.  Each test prints
`loss_stages_accuracy ...` lines with the figures it asserts on.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _loss_ref as LR
import sq_oracle as O
from _loss_ref import COMPONENTS, SLOTS, edge_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
FILL = -7.25
E_INVALID_ARG, E_WORKSPACE = -1, -3
FACTOR = 4.0
# slot or component -> factor, where a correct kernel needs more than FACTOR (none does: the largest measured
# ratio is 3.49, ExplicitLoss R = 6, m3; profiles/loss_stages_accuracy.txt)
FACTORS = {}


def _L():
    from sqr._lib import lib
    return lib()


def _st():
    from sqr._lib import stream_ptr
    return stream_ptr(torch.device(DEV))


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Guarded:
    """n elements with GUARD guard elements on either side, all filled with `fill`."""

    def __init__(self, n, dtype, fill=FILL):
        self.n, self.fill = n, fill
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + n]

    def intact(self):
        return bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[GUARD + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())


def _loss_call(kind, args, B, nblk, need_grad=1, with_mean=True, short=0, no_grad_buffer=False):
    """One call of sqr_{implicit,explicit}_loss_fwd_bwd[_mean] into guarded buffers -> (rc, dict)."""
    L = _L()
    R = args["R"]
    wsb = getattr(L, "sqr_%s_loss_workspace_bytes" % kind)(B, R)
    assert wsb == B * nblk * 18 * 4
    lps, mean = Guarded(B, torch.float64), Guarded(1, torch.float64)
    grad, ws = Guarded(B * 12, torch.float32), Guarded(wsb, torch.uint8, 0xA5)
    head = ([_p(args["pred"]), _p(args["true"]), B, args["H"], args["W"], R, args["tau"], args["s"]] if kind == "implicit"
            else [_p(args["true"]), _p(args["pred"]), B, R])
    out = [_p(lps.t)] + ([_p(mean.t)] if with_mean else []) + [None if no_grad_buffer else _p(grad.t)]
    fn = getattr(L, "sqr_%s_loss_fwd_bwd%s" % (kind, "_mean" if with_mean else ""))
    rc = fn(*head, need_grad, *out, _p(ws.t), wsb - short, _st())
    torch.cuda.synchronize()
    bufs = dict(lps=lps, mean=mean, grad=grad, ws=ws)
    assert all(b.intact() for b in bufs.values()), kind
    if rc != 0:
        return rc, bufs
    assert with_mean or mean.untouched()
    assert need_grad or grad.untouched()
    return rc, dict(loss=lps.t.cpu().numpy(), mean=mean.t.item(), grad=grad.t.cpu().numpy().reshape(B, 12),
                    part=ws.t.view(torch.float32).cpu().numpy().reshape(B, nblk, 18).copy())


def _implicit_args(c):
    true = np.ascontiguousarray(c["true"][:, 0])
    return dict(R=int(c["R"]), H=true.shape[1], W=true.shape[2], tau=float(c["tau"]), s=float(c["s"]),
                pred=torch.tensor(np.asarray(c["pred"], np.float32), device=DEV),
                true=torch.tensor(np.asarray(true, np.float32), device=DEV))


def _explicit_args(c):
    return dict(R=int(c["R"]), pred=torch.tensor(c["pred"], device=DEV), true=torch.tensor(c["true"], device=DEV))


def run_implicit(c, **kw):
    B, R = len(c["pred"]), int(c["R"])
    rc, out = _loss_call("implicit", _implicit_args(c), B, LR.implicit_nblk(R), **kw)
    assert rc == 0, _L().sqr_last_error_string()
    return out


def run_explicit(c, **kw):
    B, R = len(c["pred"]), int(c["R"])
    rc, out = _loss_call("explicit", _explicit_args(c), B, LR.explicit_nblk(R), **kw)
    assert rc == 0, _L().sqr_last_error_string()
    return out


@functools.lru_cache(maxsize=None)
def implicit_ref(shape):
    """The case, its float64 block moments, the float32 evaluation, sq_oracle and the kernel's outputs: once."""
    c = LR.implicit_case(*shape)
    R, B = c["R"], c["B"]
    ref = LR.implicit_block_moments(c["true"], c["pred"], R, c["tau"], c["s"])
    Lo, Go, lo, _ = O.implicit_loss(c["true"], c["pred"], R, c["tau"], c["s"])
    return dict(c=c, ref=ref, p32=LR.implicit_f32(c["true"], c["pred"], R, c["tau"], c["s"]), L=Lo, G=Go, l=lo,
                scales=LR.implicit_scales(B, R), gpu=run_implicit(c))


@functools.lru_cache(maxsize=None)
def explicit_ref(R):
    c = LR.explicit_case(R)
    ref = LR.explicit_block_moments(c["true"], c["pred"], R)
    Lo, Go, lo = O.explicit_loss(c["true"], c["pred"], R)
    return dict(c=c, ref=ref, p32=LR.explicit_f32(c["true"], c["pred"], R), L=Lo, G=Go, l=lo,
                scales=LR.explicit_scales(c["B"], R), gpu=run_explicit(c))


def _ratio_check(kind, name, what, names, e_kernel, e_f32):
    ratio = np.where(e_f32 > 0, e_kernel / np.where(e_f32 > 0, e_f32, 1), np.where(e_kernel > 0, np.inf, 0.0))
    print("loss_stages_accuracy %-8s %-22s %-9s %s" % (kind, name, what + "_k/f32",
                                                      " ".join("%s=%.2f" % kv for kv in zip(names, ratio))))
    for n, ek, ef in zip(names, e_kernel, e_f32):
        assert ek <= FACTORS.get(n, FACTOR) * ef, (kind, name, what, n, ek, ef)


def _suite_close(out, Lref, Gref):
    """test_loss_gpu.py's tolerances: loss 1e-4 relative, gradient 2e-4 of the sample's largest entry."""
    assert abs(out["mean"] - Lref) <= 1e-4 * abs(Lref)
    for b in range(len(Gref)):
        scale = max(np.abs(Gref[b]).max(), 1e-12)
        assert np.abs(out["grad"][b] - Gref[b]).max() <= 2e-4 * scale, b


def _finalize_check(out, pred, scales):
    """Stage 2 on one call's own partials."""
    fin = LR.finalize(out["part"], pred, *scales)
    assert np.array_equal(out["loss"], fin["loss"])
    assert out["mean"] == fin["mean"]
    g = out["grad"].astype(np.float64)
    # (2^-149: below 2^-126 fp32's spacing is absolute; ExplicitLoss at R = 1 has gradients down there)
    bound = 2.0 ** -23 * np.abs(fin["grad"]) + 1e-12 * fin["chain"] + 2.0 ** -149
    assert (np.abs(g - fin["grad"]) <= bound).all(), np.abs(g - fin["grad"]) / np.maximum(bound, 1e-300)
    assert not g[fin["grad"] == 0].any()
    return fin


# ---------------------------------------------------------------------------------- stage 1
@pytest.mark.parametrize("shape", LR.IMPLICIT_SHAPES, ids=lambda s: "R%d_%dx%d_B%d" % s)
def test_implicit_partials_vs_float64_block_moments(shape):
    r = implicit_ref(shape)
    assert np.isfinite(r["gpu"]["part"]).all()
    _ratio_check("implicit", r["c"]["name"], "slot", SLOTS, LR.slot_errors(r["gpu"]["part"], r["ref"], LR.FLOOR),
                 LR.slot_errors(r["p32"], r["ref"], LR.FLOOR))


@pytest.mark.parametrize("R", LR.EXPLICIT_R)
def test_explicit_partials_vs_float64_block_moments(R):
    r = explicit_ref(R)
    assert np.isfinite(r["gpu"]["part"]).all()
    _ratio_check("explicit", r["c"]["name"], "slot", SLOTS,
                 LR.slot_errors(r["gpu"]["part"], r["ref"], LR.FLOOR_EXPLICIT),
                 LR.slot_errors(r["p32"], r["ref"], LR.FLOOR_EXPLICIT))


# ---------------------------------------------------------------------------------- stage 2
@pytest.mark.parametrize("shape", LR.IMPLICIT_SHAPES, ids=lambda s: "R%d_%dx%d_B%d" % s)
def test_implicit_finalize_from_the_gpus_partials(shape):
    r = implicit_ref(shape)
    _finalize_check(r["gpu"], r["c"]["pred"], r["scales"])


@pytest.mark.parametrize("R", LR.EXPLICIT_R)
def test_explicit_finalize_from_the_gpus_partials(R):
    r = explicit_ref(R)
    _finalize_check(r["gpu"], r["c"]["pred"], r["scales"])


@pytest.mark.parametrize("B", [65, 1024, 1025])
def test_finalize_batches_implicit(B):
    rng = np.random.default_rng(B)
    pred = LR.sample(rng, B)
    c = dict(R=2, pred=pred, true=LR.signed_target(pred, 2, 2, 2, rng), tau=LR.TAU, s=LR.SHARP)
    out = run_implicit(c)
    fin = _finalize_check(out, pred, LR.implicit_scales(B, 2))
    _, _, lo, _ = O.implicit_loss(c["true"], pred, 2, LR.TAU, LR.SHARP, need_grad=False)
    assert np.abs(fin["loss"] - lo).max() <= 1e-4 * np.abs(lo).max() and len(set(fin["loss"])) > B // 2


def test_finalize_batch_explicit_1025():
    """R = 1, B = 1025: the multi-block finalize with moments that are not 0."""
    rng = np.random.default_rng(1025)
    c = dict(R=1, true=LR.sample(rng, 1025), pred=LR.sample(rng, 1025))
    out = run_explicit(c)
    fin = _finalize_check(out, c["pred"], LR.explicit_scales(1025, 1))
    assert (fin["grad"] != 0).sum() > 6 * 1025
    Lo, _, lo = O.explicit_loss(c["true"], c["pred"], 1, need_grad=False)
    assert abs(out["mean"] - Lo) <= 1e-4 * Lo


def test_finalize_clamp_rows():
    """Rows exactly on a bound (the entry is not masked), just below and just above it (exact zeros), and an
    un-normalised quaternion, which is used as it is."""
    f = np.float32
    rng = np.random.default_rng(77)
    p = LR.sample(rng, 4)
    p[0, 0], p[0, 3], p[0, 5] = 0.05, 0.1, 0.0
    p[1, 1], p[1, 4], p[1, 7] = 1.0, 1.0, 1.0
    p[2, 0], p[2, 3], p[2, 6] = np.nextafter(f(0.05), f(0)), np.nextafter(f(0.1), f(0)), -(2.0 ** -126)
    p[2, 2], p[2, 4], p[2, 7] = np.nextafter(f(1), f(2)), np.nextafter(f(1), f(2)), np.nextafter(f(1), f(2))
    p[3, 8:] *= f(1.3)
    masked = np.zeros((4, 12), bool)
    masked[2, [0, 3, 6, 2, 4, 7]] = True
    R = 16
    c = dict(R=R, pred=p, true=LR.signed_target(p, R, R, R, rng), tau=LR.TAU, s=LR.SHARP)
    out = run_implicit(c)
    fin = _finalize_check(out, p, LR.implicit_scales(4, R))
    assert np.array_equal(fin["grad"] == 0, masked)
    assert np.array_equal(out["grad"] == 0, masked)
    # end to end, per row: the error over the row's largest entry, against the float32 evaluation's on the same
    # row (row 2, a0 = 0.05 and e1 = 0.1: both evaluations err 2e-4, the edge of the suite's tolerance)
    Lo, Go, _, _ = O.implicit_loss(c["true"], p, R, LR.TAU, LR.SHARP)
    g32 = LR.finalize(LR.implicit_f32(c["true"], p, R, LR.TAU, LR.SHARP), p, *LR.implicit_scales(4, R))["grad"]
    row_err = lambda g: np.abs(g - Go).max(1) / np.abs(Go).max(1)
    _ratio_check("implicit", "clamp_rows_R16", "row", ["row%d" % b for b in range(4)],
                 row_err(out["grad"].astype(np.float64)), row_err(g32))
    assert abs(out["mean"] - Lo) <= 1e-4 * Lo
    # the same rows as ExplicitLoss predictions
    ce = dict(R=8, true=LR.sample(rng, 4), pred=p)
    oute = run_explicit(ce)
    _finalize_check(oute, p, LR.explicit_scales(4, 8))
    assert np.array_equal(oute["grad"] == 0, masked)
    _suite_close(oute, *O.explicit_loss(ce["true"], p, 8)[:2])


# ---------------------------------------------------------------------------------- stage 3
@pytest.mark.parametrize("n", [1, 12, 255, 256, 257])
def test_grad_scale_is_bitwise(n):
    L = _L()
    g = torch.tensor(np.random.default_rng(n).normal(size=n).astype(np.float32), device=DEV)
    for gout in (3.0, -0.5, 2.0 ** -20):
        out = Guarded(n, torch.float32)
        go = torch.tensor([gout], dtype=torch.float64, device=DEV)
        assert L.sqr_loss_grad_scale(_p(g), _p(go), n, _p(out.t), _st()) == 0
        torch.cuda.synchronize()
        assert out.intact()
        assert np.array_equal(out.t.cpu().numpy(), g.cpu().numpy() * np.float32(gout))
    out = Guarded(n, torch.float32)
    assert L.sqr_loss_grad_scale(_p(g), _p(go), 0, _p(out.t), _st()) == 0        # n = 0: nothing
    assert L.sqr_loss_grad_scale(_p(g), None, n, _p(out.t), _st()) == E_INVALID_ARG
    assert L.sqr_loss_grad_scale(_p(g), _p(go), -1, _p(out.t), _st()) == E_INVALID_ARG
    torch.cuda.synchronize()
    assert out.untouched()


# ---------------------------------------------------------------------------------- end to end
RANDOM_SHAPES = [s for s in LR.IMPLICIT_SHAPES if s[3] != 3 and s[0] > 2]
RANDOM_R = [R for R in LR.EXPLICIT_R if R != 4]


def _component_check(kind, rows):
    """Per gradient component: the kernel's largest error over the case set against the float32 evaluation's
    largest over the same set (each case's error normalised by the component's largest |g_ref| over its batch).
    The maxima are over the set, as in test_least_squares_gpu.py: at B = 1 or 2 one case's figure is a single
    draw of rounding noise for either evaluation (ImplicitLoss R = 129, dL/da0: float32 evaluation 5.7e-7,
    kernel 4.1e-5, while the float32 evaluation's other components there are 3e-5 ... 9e-4), and the ratio
    of two single draws is bounded by no factor.  The per-case ratios are printed."""
    ek, ef = [], []
    for r in rows:
        g32 = LR.finalize(r["p32"], r["c"]["pred"], *r["scales"])["grad"]
        ek.append(LR.component_errors(r["gpu"]["grad"].astype(np.float64), r["G"]))
        ef.append(LR.component_errors(g32, r["G"]))
        print("loss_stages_accuracy %-8s %-22s %-9s %s" % (kind, r["c"]["name"], "grad_k/f32", " ".join(
            "%s=%.2f" % (n, a / b) for n, a, b in zip(COMPONENTS, ek[-1], ef[-1]))))
    _ratio_check(kind, "all_random_rows", "grad", COMPONENTS, np.max(ek, 0), np.max(ef, 0))


@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=lambda s: "R%d_%dx%d_B%d" % s)
def test_implicit_vs_oracle_at_the_suites_tolerances(shape):
    r = implicit_ref(shape)
    _suite_close(r["gpu"], r["L"], r["G"])
    assert np.abs(r["gpu"]["loss"] - r["l"]).max() <= 1e-4 * np.abs(r["l"]).max()


def test_implicit_gradient_components_vs_oracle():
    _component_check("implicit", [implicit_ref(s) for s in RANDOM_SHAPES])


@pytest.mark.parametrize("R", RANDOM_R)
def test_explicit_vs_oracle_at_the_suites_tolerances(R):
    r = explicit_ref(R)
    _suite_close(r["gpu"], r["L"], r["G"])
    assert np.abs(r["gpu"]["loss"] - r["l"]).max() <= 1e-4 * np.abs(r["l"]).max()


def test_explicit_gradient_components_vs_oracle():
    _component_check("explicit", [explicit_ref(R) for R in RANDOM_R])


@pytest.mark.parametrize("shape", [s for s in LR.IMPLICIT_SHAPES if s[3] == 3], ids=lambda s: "R%d" % s[0])
def test_dyadic_rows_vs_oracle(shape):
    """The zero fix on whole planes (the case of stage 1, whose targets keep every ray's sign safe)."""
    r = implicit_ref(shape)
    assert r["ref"]["n_fixed"].tolist() == [3 * shape[0] ** 2] * 3
    _suite_close(r["gpu"], r["L"], r["G"])
    assert np.isfinite(r["gpu"]["grad"]).all()


@pytest.mark.parametrize("case", edge_cases("implicit"), ids=lambda c: str(c["name"]))
def test_implicit_vs_reference_edge_fixture(case):
    out = run_implicit(case)
    _suite_close(out, float(case["loss"]), case["grad"].astype(np.float64))
    _finalize_check(out, case["pred"], LR.implicit_scales(3, int(case["R"])))


@pytest.mark.parametrize("case", edge_cases("explicit"), ids=lambda c: str(c["name"]))
def test_explicit_vs_reference_edge_fixture(case):
    R = int(case["R"])
    assert LR.explicit_n(R) == {4: 5, 8: 9, 6: 8, 9: 11}[R]
    out = run_explicit(case)
    _suite_close(out, float(case["loss"]), case["grad"].astype(np.float64))
    _finalize_check(out, case["pred"], LR.explicit_scales(len(case["pred"]), R))


def _iou(t, p, R):
    """sqr_iou_counts / _f64 by the parameters' dtype, into guarded counts (filled with a bit pattern: the entry
    point clears them itself)."""
    L = _L()
    B = len(t)
    cnt = Guarded(2 * B, torch.int64, 0x5A5A5A5A5A5A5A5A)
    tt, pp = torch.tensor(t, device=DEV), torch.tensor(p, device=DEV)
    fn = L.sqr_iou_counts if t.dtype == np.float32 else L.sqr_iou_counts_f64
    assert fn(_p(tt), _p(pp), B, R, _p(cnt.t), _st()) == 0, L.sqr_last_error_string()
    torch.cuda.synchronize()
    assert cnt.intact()
    return cnt.t.cpu().numpy().reshape(B, 2)


@pytest.mark.parametrize("case", edge_cases("iou"), ids=lambda c: str(c["name"]))
def test_iou_vs_reference_edge_fixture(case):
    """Dyadic rows: voxels lie exactly on both surfaces (G == 1 counts as inside)."""
    R = int(case["R"])
    assert np.array_equal(_iou(case["true"], case["pred"], R), case["counts"])
    assert np.array_equal(_iou(case["true"].astype(np.float64), case["pred"].astype(np.float64), R), case["counts"])


@pytest.mark.parametrize("R", [2, 3, 16, 17])
def test_iou_counts_equal_the_oracles(R):
    rng = np.random.default_rng(9000 + 10 * R)
    t = LR.sample(rng, 3)
    p = t.copy()
    p[:, :8] += rng.normal(scale=0.03, size=(3, 8)).astype(np.float32)
    t64 = t.astype(np.float64) + rng.uniform(-1e-7, 1e-7, t.shape)
    p64 = p.astype(np.float64) + rng.uniform(-1e-7, 1e-7, p.shape)
    for a, b in ((t, p), (t64, p64)):
        # no voxel within 1e-5 of either surface: the count cannot depend on the last bits of pow
        gap = min(np.abs(O._forward_core(x[0:3], x[3:5], x[5:8], x[8:12], O.iou_axis(R), zero_fix=False)["G"] - 1).min()
                  for arr in (a, b) for x in arr.astype(np.float64))
        assert gap >= 1e-5
        cnt = O.iou_counts(a, b, R)
        assert np.array_equal(_iou(a, b, R), cnt)
        assert R < 16 or (cnt[:, 1] > cnt[:, 0]).all()


# ---------------------------------------------------------------------------------- render
def _render(pred, R, tau=LR.TAU, s=LR.SHARP):
    L = _L()
    B = len(pred)
    img = Guarded(B * R * R, torch.float32)
    p = torch.tensor(pred, device=DEV)
    assert L.sqr_implicit_render(_p(p), B, R, tau, s, _p(img.t), _st()) == 0, L.sqr_last_error_string()
    torch.cuda.synchronize()
    assert img.intact()
    return img.t.cpu().numpy().reshape(B, R, R)


@pytest.mark.parametrize("R", [2, 3, 17, 50, 129])
def test_render_vs_depth_projection(R):
    pred = LR.sample(np.random.default_rng(300 + R), 2)
    img = _render(pred, R)
    for b in range(2):
        ref = O.depth_projection(pred[b], R, LR.TAU, LR.SHARP)
        assert np.abs(img[b] - ref).max() < 2e-4
        assert R < 17 or ref.max() > 0.1      # the object is in the picture


@pytest.mark.parametrize("case", edge_cases("implicit"), ids=lambda c: str(c["name"]))
def test_render_dyadic_rows(case):
    R = int(case["R"])
    img = _render(case["pred"], R, float(case["tau"]), float(case["s"]))
    assert np.abs(img - case["depth"]).max() < 2e-4
    for b in range(3):
        assert np.abs(img[b] - O.depth_projection(case["pred"][b], R, float(case["tau"]), float(case["s"]))).max() < 2e-4


# ---------------------------------------------------------------------------------- C ABI
def test_workspace_bytes_on_both_sides_of_128():
    L = _L()
    for R, nblk in ((2, 1), (16, 1), (17, 2), (128, 64), (129, 131), (256, 512), (257, 517)):
        assert LR.implicit_nblk(R) == nblk
        for B in (1, 3, 1025):
            assert L.sqr_implicit_loss_workspace_bytes(B, R) == B * nblk * 18 * 4
    for R, n in ((1, 2), (6, 8), (9, 11), (15, 16), (16, 17), (64, 65)):
        assert L.sqr_explicit_loss_workspace_bytes(2, R) == 2 * ((n * n + 255) // 256) * 18 * 4
    assert L.sqr_implicit_loss_workspace_bytes(0, 16) == 0 and L.sqr_explicit_loss_workspace_bytes(2, 0) == 0


@pytest.mark.parametrize("shape", [(17, 17, 17, 2), (129, 129, 129, 1)], ids=lambda s: "R%d" % s[0])
def test_implicit_need_grad_0_and_the_entry_without_mean(shape):
    r = implicit_ref(shape)
    for kw in (dict(need_grad=0), dict(need_grad=0, with_mean=False), dict(need_grad=1, with_mean=False)):
        out = run_implicit(r["c"], **kw)             # (untouched gradient / mean: asserted in _loss_call)
        assert np.array_equal(out["loss"], r["gpu"]["loss"])
        assert np.array_equal(out["part"], r["gpu"]["part"])
        if kw.get("with_mean", True):
            assert out["mean"] == r["gpu"]["mean"]
        if kw["need_grad"]:
            assert np.array_equal(out["grad"], r["gpu"]["grad"])


@pytest.mark.parametrize("R", [9, 16])
def test_explicit_need_grad_0_and_the_entry_without_mean(R):
    r = explicit_ref(R)
    for kw in (dict(need_grad=0), dict(need_grad=0, with_mean=False), dict(need_grad=1, with_mean=False)):
        out = run_explicit(r["c"], **kw)
        assert np.array_equal(out["loss"], r["gpu"]["loss"])
        if kw.get("with_mean", True):
            assert out["mean"] == r["gpu"]["mean"]
        if kw["need_grad"]:
            assert np.array_equal(out["grad"], r["gpu"]["grad"])


def _refused(rc, bufs, code, word):
    assert rc == code
    assert word in _L().sqr_last_error_string()
    assert all(b.untouched() for b in bufs.values())


def test_refusals_write_nothing():
    L = _L()
    c = LR.implicit_case(3, 3, 3, 2)
    a = _implicit_args(c)
    nb = LR.implicit_nblk
    _refused(*_loss_call("implicit", a, 2, nb(3), short=1), E_WORKSPACE, b"workspace")
    _refused(*_loss_call("implicit", a, 2, nb(3), no_grad_buffer=True), E_INVALID_ARG, b"grad")
    _refused(*_loss_call("implicit", dict(a, R=1), 2, nb(1)), E_INVALID_ARG, b"R=1")
    _refused(*_loss_call("implicit", dict(a, R=257), 2, nb(257)), E_INVALID_ARG, b"R=257")
    for B in (0, 65536):
        lps, grad, ws = Guarded(4, torch.float64), Guarded(48, torch.float32), Guarded(4096, torch.uint8, 0xA5)
        bufs = dict(lps=lps, grad=grad, ws=ws)
        rc = L.sqr_implicit_loss_fwd_bwd(_p(a["pred"]), _p(a["true"]), B, 3, 3, 3, 1.5, 260.0, 1, _p(lps.t), _p(grad.t),
                                         _p(ws.t), 4096, _st())
        torch.cuda.synchronize()
        _refused(rc, bufs, E_INVALID_ARG, b"B=%d" % B)
        rc = L.sqr_explicit_loss_fwd_bwd(_p(a["pred"]), _p(a["pred"]), B, 4, 1, _p(lps.t), _p(grad.t), _p(ws.t), 4096,
                                         _st())
        torch.cuda.synchronize()
        _refused(rc, bufs, E_INVALID_ARG, b"B=%d" % B)
    e = _explicit_args(LR.explicit_case(6))
    _refused(*_loss_call("explicit", e, 2, LR.explicit_nblk(6), short=1), E_WORKSPACE, b"workspace")
    _refused(*_loss_call("explicit", e, 2, LR.explicit_nblk(6), no_grad_buffer=True), E_INVALID_ARG, b"grad")
    for R in (0, 1025):
        lps, grad, ws = Guarded(4, torch.float64), Guarded(48, torch.float32), Guarded(4096, torch.uint8, 0xA5)
        rc = L.sqr_explicit_loss_fwd_bwd(_p(e["true"]), _p(e["pred"]), 2, R, 1, _p(lps.t), _p(grad.t), _p(ws.t), 4096,
                                         _st())
        torch.cuda.synchronize()
        _refused(rc, dict(lps=lps, grad=grad, ws=ws), E_INVALID_ARG, b"R=%d" % R)
    img = Guarded(64, torch.float32)
    rc = L.sqr_implicit_render(_p(a["pred"]), 2, 1, 1.5, 260.0, _p(img.t), _st())
    torch.cuda.synchronize()
    _refused(rc, dict(img=img), E_INVALID_ARG, b"R=1")


def test_implicit_257_without_a_gradient():
    """R > 256 runs without a gradient (the check is on need_grad); its loss against sq_oracle at B = 1."""
    rng = np.random.default_rng(257)
    pred = LR.sample(rng, 1)
    true = rng.uniform(size=(1, 1, 257, 257)).astype(np.float32)
    out = run_implicit(dict(R=257, pred=pred, true=true, tau=LR.TAU, s=LR.SHARP), need_grad=0)
    D = O.depth_projection(pred[0], 257, LR.TAU, LR.SHARP)
    ref = np.abs(true[0, 0].astype(np.float64) - D).mean()
    assert abs(out["loss"][0] - ref) <= 1e-4 * ref and out["mean"] == out["loss"][0]
    assert np.array_equal(out["loss"], LR.finalize(out["part"], pred, *LR.implicit_scales(1, 257))["loss"])
