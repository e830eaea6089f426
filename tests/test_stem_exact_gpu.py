"""The fused stem (csrc/sqr_stem.hip) bitwise against float64 on the integer-exact operands of
tests/_stem_exact.py (whose premises test_stem_exact_cpu.py checks):

  1. training forward, small class: y and the argmax taps equal the reference bit for bit (every pooled
     output, ties and zeros included); save_mean / save_invstd and, with momentum 1, the running
     statistics within 2^-20;
  2. training backward: dbeta exactly; dW and dgamma within 2^-19 of the closed form's term magnitudes;
  3. eval forward, round class with coefficients exact in f32: y bit for bit;
  4. the statistics of a conv1 output that the cast to T rounds;
  5. fused == unfused (sqr.conv.conv2d with statistics + sqr.bn.stem), bit for bit;
  6. two runs of the 1100-image case, whose workgroups hold several tiles each, agree bit for bit.

Tolerances.  Statistics: |mean - ref| <= 2^-20 (|mean| + std), |invstd - ref| <= 2^-20 invstd; the running
variance, formed in double from the same merged (mean, M2) as invstd, <= 2^-20 var.  The kernel's rows
are f32 Welford pairs of exact (small class) or f32-rounded (round class) sums, merged in double: a
few roundings of 2^-24 each.
Gradients: |dW - ref| <= 2^-19 B_W + 2^-23 |ref| with B_W = |a T1| + |k3 T2| + |k2 T3| the closed form's term
magnitudes (dgamma: B = (|sum g c| + |mean sum g|) invstd).  T1, T2, T3 and the sums are exact (integers below
2^24 per workgroup, added in double); each term is a product of at most four factors that carry an f32
rounding (2^-24: save_mean, save_invstd, gamma) or the statistics error (<= 2^-20, item 1): at most
2^-20 + 3 * 2^-24 < 2^-19 / 2 per term, doubled; 2^-23 |ref| is the result's own f32 rounding, doubled."""
import functools

import pytest
import torch
import torch.nn as nn

import _stem_exact as se

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
XNAME = {F32: "xf32", BF16: "xbf16", F16: "xf16"}
STAT_TOL = 2.0 ** -20
GRAD_TOL, GRAD_RND = 2.0 ** -19, 2.0 ** -23

# (case, input dtype, activation dtype): f32 input everywhere, all six routes on `min` and `seams`
ROUTES = [(cid, F32, dt) for cid in se.ALL_IDS for dt in se.PREC]
ROUTES += [(cid, xdt, dt) for cid in se.ROUTE_IDS for xdt in (BF16, F16) for dt in se.PREC]
ROUTE_ID = lambda r: "%s-%s-%s" % (r[0], XNAME[r[1]], se.DT_NAME[r[2]])
CASE_DT = lambda ids: [(cid, dt) for cid in ids for dt in se.PREC]
CASE_DT_ID = lambda c: "%s-%s" % (c[0], se.DT_NAME[c[1]])


def _mods(w, gamma, beta, eps):
    """conv1 and bn1 on the GPU holding the reference's parameters; momentum 1: the running statistics
    become the batch's."""
    from sqr.conv import Conv2d
    conv = Conv2d(1, 64, 7, 2, 3, bias=False)
    conv.weight.data = w.float()
    bn = nn.BatchNorm2d(64, eps=eps, momentum=1.0)
    bn.weight.data, bn.bias.data = gamma.float(), beta.float()
    return conv.to(DEV), bn.to(DEV).train()


def _exact(t, dtype):
    """t (float64, CPU) on the GPU in dtype, unchanged by the cast."""
    out = t.to(dtype)
    assert torch.equal(out.double(), t)
    return out.to(DEV)


def _train(x, dy, w, gamma, beta, eps, xdt, dt, fused=True):
    """One training forward (and backward if dy is given) -> CPU tensors."""
    from sqr import conv as sc
    from sqr.bn import fused_stem, fused_stem_ok, stem
    conv, bn = _mods(w, gamma, beta, eps)
    xg = _exact(x, xdt)
    out = {}
    if fused:
        assert fused_stem_ok(xg, conv, bn)  # a geometry the kernels accept
        y = fused_stem(xg, conv, bn, dt=dt)
        _, _, _, _, arg, mean, invstd = y.grad_fn.saved_tensors
        out.update(arg=arg.cpu(), mean=mean.double().cpu(), invstd=invstd.double().cpu())
    else:
        y = stem(sc.conv2d(xg.to(dt), conv.weight, None, 2, 3, stats=True), bn)
    assert y.dtype == dt and y.is_contiguous(memory_format=CL)
    if dy is not None:
        y.backward(_exact(dy, dt).contiguous(memory_format=CL))
        out.update(dW=conv.weight.grad.double().cpu(), dgamma=bn.weight.grad.double().cpu(),
                   dbeta=bn.bias.grad.double().cpu())
    torch.cuda.synchronize()
    out.update(y=y.detach().cpu().contiguous(), rm=bn.running_mean.double().cpu(), rv=bn.running_var.double().cpu())
    return out


@functools.lru_cache(maxsize=None)
def _small_run(cid, xdt, dt):
    o = se.small(cid, dt)
    return _train(o.x, o.dy, o.w, o.gamma, o.beta, o.eps, xdt, dt)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _assert_y(y, y_ref, dt, what="y"):
    """Bit for bit (-0 is not +0), NCHW order on both sides."""
    ref = y_ref.to(dt)
    assert y.shape == ref.shape and y.dtype == dt
    y = y.contiguous()
    if not torch.equal(y, ref):
        bad = (y != ref)
        n, k, h, w = [int(v) for v in bad.nonzero()[0]]
        raise AssertionError("%s: %d of %d differ; first at image %d channel %d (%d, %d): %g, reference %g" % (
            what, int(bad.sum()), bad.numel(), n, k, h, w, float(y[n, k, h, w]), float(ref[n, k, h, w])))
    assert torch.equal(_bits(y), _bits(ref)), what + ": signed zeros"


def _stat_ratios(r, o):
    """error / bound of (save_mean, save_invstd, running_mean, running_var) against the float64 values."""
    std = torch.sqrt(o.var)
    mb = STAT_TOL * (o.mean.abs() + std)
    return {"mean": float(((r["mean"] - o.mean).abs() / mb).max()),
            "invstd": float(((r["invstd"] - o.invstd).abs() / (STAT_TOL * o.invstd)).max()),
            "rmean": float(((r["rm"] - o.mean).abs() / mb).max()),
            "rvar": float(((r["rv"] - o.var_unb).abs() / (STAT_TOL * o.var_unb)).max())}


def _assert_stats(r, o, tag):
    for k in ("mean", "invstd", "rm", "rv"):
        assert bool(torch.isfinite(r[k]).all()), k
    ratios = _stat_ratios(r, o)
    print("stem_exact_accuracy %-22s stats   " % tag + " ".join("%s %.3e" % kv for kv in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, "%s %s: error / bound = %.3g" % (tag, k, v)


# ---------------------------------------------------------------- 1. training forward
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_ID)
def test_train_forward(route):
    cid, xdt, dt = route
    o = se.small(cid, dt)
    r = _small_run(cid, xdt, dt)
    _assert_stats(r, o, ROUTE_ID(route))
    _assert_y(r["y"], o.y, dt)
    tap = o.tap.permute(0, 2, 3, 1).contiguous()  # the kernel's (N, Hp, Wp, 64) u8 buffer
    assert r["arg"].shape == tap.shape and r["arg"].dtype == torch.uint8
    if not torch.equal(r["arg"], tap):
        bad = r["arg"] != tap
        n, h, w, k = [int(v) for v in bad.nonzero()[0]]
        raise AssertionError("argmax: %d of %d differ; first at image %d (%d, %d) channel %d: tap %d, reference %d" % (
            int(bad.sum()), bad.numel(), n, h, w, k, int(r["arg"][n, h, w, k]), int(tap[n, h, w, k])))


# ---------------------------------------------------------------- 2. training backward
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_ID)
def test_train_backward(route):
    cid, xdt, dt = route
    o = se.small(cid, dt)
    r = _small_run(cid, xdt, dt)
    for k in ("dW", "dgamma", "dbeta"):
        assert bool(torch.isfinite(r[k]).all()), k
    ratio = lambda got, ref, B: float(((got - ref).abs() / (GRAD_TOL * B + GRAD_RND * ref.abs()).clamp_min(1e-300)).max())
    rw, rg = ratio(r["dW"], o.dW, o.B_W), ratio(r["dgamma"], o.dgamma, o.B_gamma)
    print("stem_exact_accuracy %-22s backward dW %.3e dgamma %.3e" % (ROUTE_ID(route), rw, rg))
    assert torch.equal(r["dbeta"], o.dbeta)  # sum g: an integer below 2^24
    assert rw <= 1.0, "dW: error / bound = %.3g" % rw
    assert rg <= 1.0, "dgamma: error / bound = %.3g" % rg


# ---------------------------------------------------------------- 3. eval forward
@pytest.mark.parametrize("case", CASE_DT(se.EVAL_IDS), ids=CASE_DT_ID)
def test_eval_forward(case):
    from sqr.bn import fused_stem, fused_stem_ok
    cid, dt = case
    o = se.rounded(cid, dt)
    conv, bn = _mods(o.w, o.gamma, o.beta, o.eps)
    bn.running_mean.data, bn.running_var.data = o.running_mean.float().to(DEV), o.running_var.float().to(DEV)
    bn.eval()
    xg = _exact(o.x, F32)
    assert fused_stem_ok(xg, conv, bn)
    with torch.no_grad():
        y = fused_stem(xg, conv, bn, dt=dt)
    torch.cuda.synchronize()
    assert y.is_contiguous(memory_format=CL)
    _assert_y(y.cpu(), o.y_eval, dt)
    assert torch.equal(bn.running_mean.double().cpu(), o.running_mean)  # eval mode leaves them alone
    assert torch.equal(bn.running_var.double().cpu(), o.running_var)


# ---------------------------------------------------------------- 4. statistics of the rounded conv output
@pytest.mark.parametrize("case", CASE_DT(se.STATS_IDS), ids=CASE_DT_ID)
def test_stats_of_rounded_conv(case):
    cid, dt = case
    o = se.rounded(cid, dt)
    r = _train(o.x, None, o.w, o.gamma, o.beta, o.eps, F32, dt)
    _assert_stats(r, o, "%s-round-%s" % (cid, se.DT_NAME[dt]))
    assert bool(torch.isfinite(r["y"].float()).all())


# ---------------------------------------------------------------- 5. fused == unfused
@pytest.mark.parametrize("case", CASE_DT(se.ROUTE_IDS), ids=CASE_DT_ID)
def test_fused_equals_unfused(case):
    cid, dt = case
    o = se.small(cid, dt)
    fused = _small_run(cid, F32, dt)
    plain = _train(o.x, None, o.w, o.gamma, o.beta, o.eps, F32, dt, fused=False)
    _assert_y(plain["y"], o.y, dt, "unfused y")
    assert torch.equal(_bits(fused["y"]), _bits(plain["y"]))


# ---------------------------------------------------------------- 6. determinism where workgroups hold several tiles
@pytest.mark.parametrize("dt", list(se.PREC), ids=list(se.DT_NAME.values()))
def test_many_is_deterministic(dt):
    o = se.small("many", dt)
    a = _small_run("many", F32, dt)
    b = _train(o.x, o.dy, o.w, o.gamma, o.beta, o.eps, F32, dt)
    assert torch.equal(_bits(a["y"]), _bits(b["y"])) and torch.equal(a["arg"], b["arg"])
    for k in ("dW", "dgamma", "dbeta", "mean", "invstd"):
        assert torch.equal(a[k], b[k]), k
