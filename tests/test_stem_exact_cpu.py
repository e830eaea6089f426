"""The premises of the bitwise fused-stem tests (test_stem_exact_gpu.py), checked on the CPU for every case
that file runs: the generator's conditions hold (tests/_stem_exact.py) with the measured shares that
make the tie rule, the y > 0 mask and the casts bite; the closed-form backward the kernel uses equals
float64 autograd; the tap encoding equals a brute-force first maximum; and the reference can see the
tie rule."""
import pytest
import torch
import torch.nn.functional as F

import _stem_exact as se

DTS = list(se.PREC)
DT_IDS = [se.DT_NAME[d] for d in DTS]


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("cid", se.ALL_IDS)
def test_small_case_builds(cid, dt):
    """Measured over the six cases: max conv(|x|, |w|) 22-54 (bf16 holds integers to 256), at most 42 distinct
    conv values per channel, beta found in at most 4 (bf16) / 34 (fp16) tries, 19.7-24.0 % of the pooled
    outputs tied, 1.4-5.0 % exactly zero."""
    o = se.small(cid, dt)
    print("%s %s: bound %g, %d values, %d tries, ties %.1f %%, zeros %.1f %%" % (
        cid, se.DT_NAME[dt], o.y_bound, o.max_values, o.tries, 100 * o.tie_share, 100 * o.zero_share))
    assert o.y_bound <= se.EXACT_INT[dt] and torch.equal(se.cast(o.c, dt), o.c)
    assert o.max_values <= 64
    assert o.tries <= se.MAX_TRIES and o.fragile == 0
    assert not bool(se.fragile_pairs(o.base, dt, o.beta).any())
    assert o.tie_share >= 0.10 and o.zero_share >= 0.01
    # the operand classes
    assert set(o.x.unique().tolist()) <= {0.0, 1.0, 2.0} and set(o.w.unique().tolist()) == {-1.0, 0.0, 1.0}
    assert 0.4 <= float((o.w == 0).double().mean()) <= 0.6
    assert float(o.dy.abs().max()) == 4 and torch.equal(o.dy, o.dy.round())
    if o.N >= 3:  # the thinning: image means in the order of the keep probabilities
        m = o.x.mean((1, 2, 3))
        assert float(m[0::3].mean()) < float(m[1::3].mean()) < float(m[2::3].mean())
    # what the kernel is handed is what the reference saw
    for v in (o.gamma, o.beta):
        assert torch.equal(v.float().double(), v)
    assert int((o.gamma < 0).sum()) == 16
    # every pixel of y is one of the table's values: y before pooling depends on (channel, value) alone
    r = se.act(o)
    lut = se.cast(torch.relu(o.values.view(1, -1) * o.scale.view(-1, 1) + o.shift.view(-1, 1)), dt)  # (64, values)
    assert torch.equal(r, lut[torch.arange(64).view(1, 64, 1, 1), o.c.long() - o.vmin])
    # dbeta is an integer an f32 holds
    assert torch.equal(o.dbeta, o.dbeta.round()) and float(o.dbeta.abs().max()) < se.LIM


def test_tile_counts():
    """The persistent loops the cases are there for (grids: stats and backward 512, pool 768)."""
    assert se.tiles(*se.CASES["min"]) == (1, 1, 2)
    assert se.tiles(*se.CASES["seams"]) == (2 * 3 * 2, 2 * 3 * 2, 2 * 6 * 2)
    assert se.tiles(*se.CASES["wide"]) == (4, 4, 8)
    st, pool, bwd = se.tiles(*se.CASES["many"])
    assert (st, pool, bwd) == (1100, 1100, 2200)
    assert 2 * 512 < st < 3 * 512 and 768 < pool < 2 * 768 and 4 * 512 < bwd < 5 * 512  # unequal counts


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_boundary_distance(dt):
    """Moving t by less than its boundary distance keeps its rounded value; moving it past the boundary, one
    way or the other, changes it.  Powers of two (uneven neighbours) and fp16 subnormals included."""
    p, emin = se.PREC[dt]
    g = torch.Generator().manual_seed(5)
    t = torch.randn(4096, generator=g, dtype=torch.float64) * torch.ldexp(
        torch.ones(4096, dtype=torch.float64), torch.randint(max(emin - 4, -100), 6, (4096,), generator=g))
    near = torch.ldexp(torch.ones(64, dtype=torch.float64), torch.arange(emin + 1, emin + 65).clamp_max(8))
    t = torch.cat([t, near * (1 + 2.0 ** -30), near * (1 - 2.0 ** -30), near])
    d = se.boundary_distance(t, dt)
    assert bool((d >= 0).all())
    # (torch casts float64 to a 16-bit type through float32: stay 2^-20 |t| clear of the boundary itself,
    # where that double rounding decides; the generator's guard band, 2^-18, keeps further away)
    margin = 2.0 ** -20 * t.abs()
    inside, past = (d - margin).clamp_min(0), d + margin
    same = lambda a, b: se.cast(a, dt) == se.cast(b, dt)
    assert bool((same(t.abs() + inside, t.abs()) & same(t.abs() - inside, t.abs())).all())
    assert bool((~same(t.abs() + past, t.abs()) | ~same(t.abs() - past, t.abs())).all())


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("cid", se.ALL_IDS)
def test_closed_form_equals_autograd(cid, dt):
    o = se.small(cid, dt)
    dW, dgamma, dbeta = se.autograd_grads(o)
    for name, cf, ag in (("dW", o.dW, dW), ("dgamma", o.dgamma, dgamma), ("dbeta", o.dbeta, dbeta)):
        err = float((cf - ag).abs().max() / ag.abs().max())
        assert err <= 1e-12, "%s: closed form against autograd %.3g" % (name, err)
    # the magnitudes bound the values they are tolerances for
    assert bool((o.B_W >= o.dW.abs() * (1 - 1e-12)).all()) and bool((o.B_gamma >= o.dgamma.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("cid", se.ALL_IDS)
def test_taps_match_brute_force(cid, dt):
    """The tap numbers derived from max_pool2d's indices against the first maximum, in row-major window
    order, of the unfolded windows padded with -inf."""
    o = se.small(cid, dt)
    act = se.act(o)
    for i in range(0, o.N, se.CHUNK):
        r = act[i:i + se.CHUNK]
        n = r.shape[0]
        rp = F.pad(r, (1, 1, 1, 1), value=float("-inf")).reshape(n * 64, 1, o.Hc + 2, o.Wc + 2)
        win = F.unfold(rp, 3, stride=2).view(n, 64, 9, o.Hp, o.Wp)
        mx = win.max(2, keepdim=True).values
        eq = win == mx
        first = eq & (eq.cumsum(2) == 1)
        tap = (first * torch.arange(9).view(1, 1, 9, 1, 1)).sum(2)
        assert torch.equal(mx[:, :, 0], o.y[i:i + n])
        assert torch.equal(tap.to(torch.uint8), o.tap[i:i + n])
    assert torch.equal(torch.stack(se.window_slices(act[:2]), 2), F.unfold(
        F.pad(act[:2], (1, 1, 1, 1), value=float("-inf")).reshape(-1, 1, o.Hc + 2, o.Wc + 2), 3, stride=2).view(
            -1, 64, 9, o.Hp, o.Wp))


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_reference_sees_the_tie_rule(dt):
    """One tied window routed to its second maximum instead of its first changes the reference dW (and no
    other output of the forward)."""
    o = se.small("min", dt)
    r = se.act(o)
    ws = torch.stack(se.window_slices(r), 2)  # (N, 64, 9, Hp, Wp)
    eq = ws == o.y.unsqueeze(2)
    cand = (eq.sum(2) >= 2) & (o.y > 0) & (o.base.dy != 0)
    n, k, ph, pw = [int(v) for v in cand.nonzero()[0]]
    second = int(eq[n, k, :, ph, pw].nonzero()[1])
    assert second > int(o.tap[n, k, ph, pw])
    idx = o.idx.clone()
    idx[n, k, ph, pw] = (2 * ph - 1 + second // 3) * o.Wc + (2 * pw - 1 + second % 3)
    assert float(r.reshape(1, 64, -1)[n, k, idx[n, k, ph, pw]]) == float(o.y[n, k, ph, pw])
    from types import SimpleNamespace
    flipped = se.closed_form(o, idx, SimpleNamespace())
    assert torch.equal(flipped.dbeta, o.dbeta)  # the same gradient, at another pixel
    assert not torch.equal(flipped.dW, o.dW)
    # ... and by more than the GPU test's tolerance
    tol = 2.0 ** -19 * o.B_W + 2.0 ** -23 * o.dW.abs()
    assert bool(((flipped.dW - o.dW).abs() > tol).any())


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("cid", se.EVAL_IDS)
def test_round_case_builds(cid, dt):
    """Measured: max conv(|x|, |w|) 1264-1283 (bf16) / 9678-10179 (fp16); the cast of conv1's output rounds
    3.2-7.1 % of the values, the cast of the eval-mode activation 18-31 %."""
    o = se.rounded(cid, dt)
    print("%s %s: bound %g, conv cast rounds %.1f %%, activation cast %.1f %%" % (
        cid, se.DT_NAME[dt], o.y_bound, 100 * o.round_share, 100 * o.round_share_eval))
    wr = 32 if dt == torch.float16 else 4
    assert 0 <= float(o.x.min()) and float(o.x.max()) <= 8 and float(o.w.abs().max()) <= wr
    assert o.y_bound < se.LIM and (dt != torch.float16 or o.y_bound <= 65504 / 4)
    assert o.round_share >= 0.02 and o.round_share_eval >= 0.05
    # the eval coefficients: exact in f32, invstd a power of two in double arithmetic
    inv = 1.0 / torch.sqrt(o.running_var.float().double() + float(torch.tensor(se.EPS_EVAL).float()))
    assert set(inv.tolist()) <= {0.5, 1.0, 2.0}
    assert set(o.gamma.abs().tolist()) <= {0.5, 1.0, 2.0} and int((o.gamma < 0).sum()) == 16
    assert torch.equal(o.running_mean * 4, (o.running_mean * 4).round()) and float(o.running_mean.abs().max()) <= 4
    assert torch.equal(o.beta, o.beta.round()) and float(o.beta.abs().max()) <= 4
    # an f32 fma of the f32 coefficients gives the float64 pre-activation exactly
    bc = lambda v: v.view(1, -1, 1, 1)
    t32 = torch.addcmul(bc(o.shift_eval.float()), o.cb.float(), bc(o.scale_eval.float()))
    assert torch.equal(F.max_pool2d(se.cast(torch.relu(t32).double(), dt), 3, 2, 1), o.y_eval)
    share = float((o.y_eval == 0).double().mean())
    assert 0.05 <= share <= 0.8  # the ReLU clips, and not everything
