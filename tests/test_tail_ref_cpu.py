"""The float64 tail reference of _tail_ref.py and its yardstick, on the CPU.

(1) The stage functions, chained, against the model's own modules (Sequential(Linear, LeakyReLU,
    Linear, LeakyReLU) + models.SizeHead / ShapeHead / PositionHead / RotationHead) in float64 through
    autograd: outputs, x.grad and every parameter gradient.  Both sides are float64 and differ by
    summation order only, so they agree within the a-priori bound of a float64 sum: the stage's
    (n + 2) / 2 in units of EPS64 * M, M the same magnitudes as in the float32 measure.  The backward
    stages chain, so a gradient carries the roundings of the stages before it: the bound of a
    gradient is the sum of the bounds along its chain, times 4 for what a stage's own cancellation
    (M >= |value|) adds when its error is carried on.  A wrong formula is off by 1e10 of these units.
(2) The yardstick table _tail_ref.YARD: every figure re-measured and held within a factor 2 of the
    table in both directions.
(3) The ceiling: no figure of the table exceeds the a-priori bound (n + 2) / 2 of its stage.
"""
import pytest
import torch
import torch.nn as nn

import _tail_ref as R

F64 = torch.float64


def _modules(C0, F1, F2, seed):
    import models
    torch.manual_seed(seed)
    fc = nn.Sequential(nn.Linear(C0, F1), nn.LeakyReLU(), nn.Linear(F1, F2), nn.LeakyReLU())
    heads = (models.SizeHead(F2), models.ShapeHead(F2), models.PositionHead(F2), models.RotationHead(F2))
    return fc.double(), [h.double() for h in heads]


def _units64(got, ref, mag):
    return float(((got - ref).abs() / (R.EPS64 * mag + 1e-300)).max())


@pytest.mark.parametrize("zeros", [False, True], ids=["random", "zero_preacts"])
@pytest.mark.parametrize("B,P,C0,F1,F2", [(5, 4, 16, 20, 12), (3, 1, 8, 4, 36)])
def test_reference_matches_modules(B, P, C0, F1, F2, zeros):
    fc, hd = _modules(C0, F1, F2, B + F1)
    g = torch.Generator().manual_seed(11)
    H = {4: (2, 2), 1: (1, 1)}[P]
    x = torch.randn(B, C0, *H, generator=g, dtype=F64)
    if zeros:
        # pre-activations that are exactly 0 in both layers: integer operands (P = 4 or 1: every mean and so
        # every fc.0 sum is exact in any order), bias = -(W v) for the first rows of fc.0 on sample 0, and
        # rows of fc.2 that see only those zeroed features
        with torch.no_grad():
            x.copy_(torch.randint(-3, 4, x.shape, generator=g).double())
            for lin in (fc[0], fc[2]):
                lin.weight.copy_(torch.randint(-2, 3, lin.weight.shape, generator=g).double())
                lin.bias.copy_(torch.randint(-2, 3, lin.bias.shape, generator=g).double())
            x[0] = x[0].mean((1, 2), keepdim=True)          # sample 0: every pixel its (integer / P) mean
            x[0] = torch.round(x[0])
            fc[0].bias[:2] = -(fc[0].weight[:2] @ x[0].mean((1, 2)))
            fc[2].weight[:2, 2:] = 0
            fc[2].bias[:2] = 0
            for h in hd:    # integer layers give |h1| in the hundreds: keep the logits out of saturation
                h.out_layer[0].weight.mul_(2.0 ** -8)
    G = [torch.randn(B, n, generator=g, dtype=F64) for n in R.HEAD_N]
    xr = x.clone().requires_grad_(True)
    f = fc(xr.mean((2, 3)))
    outs = [h(f) for h in hd]
    sum((o * gg).sum() for o, gg in zip(outs, G)).backward()

    W0, b0, W1, b1 = fc[0].weight.detach(), fc[0].bias.detach(), fc[2].weight.detach(), fc[2].bias.detach()
    Wh = torch.cat([h.out_layer[0].weight.detach() for h in hd], 0)
    bh = torch.cat([h.out_layer[0].bias.detach() for h in hd], 0)
    xs = x.permute(0, 2, 3, 1).reshape(B, P, C0)
    feat = R.pool(xs)
    pre0 = R.fc(W0, b0, feat)
    pre1 = R.fc(W1, b1, R.leaky(pre0))
    if zeros:
        assert bool((pre0[0, :2] == 0).all()) and bool((pre1[0, :2] == 0).all())
        for pre in (pre0, pre1):   # no other pre-activation so close to 0 that a summation order picks its branch
            assert bool(((pre == 0) | (pre.abs() > 1e-9)).all())
    z = R.heads(Wh, bh, R.leaky(pre1))
    Gc = R.upstream(G, B)
    dz = R.dz(z, Gc)
    d1 = R.d1(Wh, dz, pre1)
    d0 = R.d0(W1, d1, pre0)
    dxr = R.dx(W0, d0, P)

    c = R.Case("cpu", B, P, C0, F1, F2, torch.float32, "packed", "sep")
    cl = lambda *st: sum(R.ceiling(s, c) for s in st)
    # forward: z carries feat, pre0 and pre1's roundings into its own
    zm = torch.cat([h.out_layer(f).detach() for h in hd], 1)
    assert _units64(zm, z, R.fc_mag(Wh, bh, R.leaky(pre1))) <= cl("feat", "pre0", "pre1", "z") * 4
    for o, r in zip(outs, R.activate(zm)):
        assert _units64(o.detach(), r, r.abs()) <= R.ceiling("q", c)
    # gradients: both sides from the modules' logits zm would need the modules' intermediates; the chain
    # from z differs from zm by float64 units of z, which the sigmoid and the normalisation pass on
    # unamplified at these magnitudes
    chain = {"dz": cl("dz") + cl("feat", "pre0", "pre1", "z") * 4}
    chain["d1"] = chain["dz"] + cl("d1")
    chain["d0"] = chain["d1"] + cl("d0")
    chain["dx"] = chain["d0"] + cl("dx")
    gx = xr.grad.permute(0, 2, 3, 1).reshape(B, P, C0)
    assert bool((gx == gx[:, :1]).all())
    assert _units64(gx[:, 0], dxr, R.dx_mag(W0, d0, P)) <= chain["dx"] * 4
    for (d, act, w, b, st, up) in ((d0, feat, fc[0].weight, fc[0].bias, "dw0", "d0"),
                                   (d1, R.leaky(pre0), fc[2].weight, fc[2].bias, "dw1", "d1")):
        (rw, rb), (mw, mb) = R.wgrad(d, act), R.wgrad_mag(d, act)
        assert _units64(w.grad, rw, mw) <= (chain[up] + cl(st)) * 4
        assert _units64(b.grad, rb, mb) <= (chain[up] + cl(st)) * 4
    (rw, rb), (mw, mb) = R.wgrad(dz, R.leaky(pre1)), R.wgrad_mag(dz, R.leaky(pre1))
    gw = torch.cat([h.out_layer[0].weight.grad for h in hd], 0)
    gb = torch.cat([h.out_layer[0].bias.grad for h in hd], 0)
    assert _units64(gw, rw, mw) <= (chain["dz"] + cl("dwh")) * 4
    assert _units64(gb, rb, mb) <= (chain["dz"] + cl("dbh")) * 4


def test_leaky_edges():
    """slope 0.01 at 0, -0 and below; 1 above."""
    pre = torch.tensor([0.0, -0.0, R.TINY, -R.TINY, 1.0, -1.0], dtype=F64)
    assert R.leaky(pre).tolist() == [0.0, -0.0, R.TINY, -R.TINY * 0.01, 1.0, -0.01]
    one = torch.ones(1, 1, dtype=F64)
    assert R.d1(one, one.expand(6, 1), pre[:, None]).view(-1).tolist() == [0.01, 0.01, 1.0, 0.01, 1.0, 0.01]


def test_layout_helpers():
    s = torch.arange(2 * (8 + 4 + 12 + 12)).view(2, -1)
    feat, pre0, pre1, z = R.split_save(s, 8, 4, 12)
    assert (feat.shape[1], pre0.shape[1], pre1.shape[1], z.shape[1]) == (8, 4, 12, 12)
    assert pre0[1, 0] == 36 + 8 and pre1[0, 0] == 12 and z[0, 0] == 24
    d = torch.arange(2 * (4 + 20 + 12)).view(2, -1)
    d0, d1, dz = R.split_dsave(d, 4, 20)
    assert d0[0, 3] == 3 and d1[0, 0] == 4 and dz[1, 0] == 36 + 24


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_torch_cpu_is_the_yardstick(name):
    """torch's float32 on the CPU, stage by stage, is what _tail_ref.YARD says it is (within 2x)."""
    now = R.torch_cpu_figures(name)
    line = "  ".join("%s %.3f (%.3f)" % (s, now[s], R.YARD[name][s]) for s in R.STAGES)
    print(name, line)
    for s in R.STAGES:
        t = R.YARD[name][s]
        assert 0.5 * t <= now[s] <= 2.0 * t or (t == 0.0 and now[s] == 0.0), "%s %s: %.3f, table %.3f" % (name, s, now[s], t)


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_yardstick_below_the_ceiling(name):
    """No figure of the table exceeds its stage's a-priori bound (n + 2) / 2."""
    c = R.CASE[name]
    for s in R.STAGES:
        assert R.YARD[name][s] <= R.ceiling(s, c), "%s %s: %.3f > %.1f" % (name, s, R.YARD[name][s], R.ceiling(s, c))


def test_table_is_in_the_docstring():
    assert set(R.YARD) == set(R.CASE)
    for line in R.yard_table().splitlines():
        assert line in R.__doc__
