"""The float64 references of tests/_bn_ref.py against float64 nn.BatchNorm2d autograd on the CPU, at
rtol 1e-10 (absolute floor 1e-10 * max|ref|: dx is a cancelling sum), before the GPU tests rely on
them: y, dx, dweight, dbias and the running statistics with and without ReLU, with a residual, and
for the two-branch sum; merge_fwd on rows built from x against the statistics of x itself.  eps and
momentum are exact in f32 (the C ABI passes both as floats and the reference follows it)."""
import pytest
import torch
import torch.nn as nn

import _bn_ref as R

F64 = torch.float64
EPS, MOM = 2.0 ** -16, 0.125
ROWS = [5, 1, 37, 2, 60]  # unequal row sizes, one of a single pixel: 105 = 3 * 5 * 7 pixels


def _close(a, b, rtol=1e-10):
    b = b.detach().to(F64)
    torch.testing.assert_close(a.detach().to(F64), b, rtol=rtol, atol=rtol * float(b.abs().max()))


def _bn(C, seed):
    g = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm2d(C, eps=EPS, momentum=MOM).double()
    bn.weight.data = torch.rand(C, generator=g, dtype=F64) + 0.5
    bn.bias.data = torch.randn(C, generator=g, dtype=F64) * 0.3
    bn.running_mean.data = torch.randn(C, generator=g, dtype=F64) * 0.2
    bn.running_var.data = torch.rand(C, generator=g, dtype=F64) + 0.5
    return bn


def _mc(t):  # NCHW -> [M, C]
    return t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _nchw(t, like):  # [M, C] -> NCHW
    N, C, H, W = like.shape
    return t.reshape(N, H, W, C).permute(0, 3, 1, 2)


def _inputs(seed, C=16, N=3, H=5, W=7):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g, dtype=F64) * 1.7 + 0.4
    x[:, :C // 2] += 100.0  # half the channels |mean| >> std
    return g, x


def _ref_forward(x, bn):
    """(mean, invstd, coef, new_rm, new_rv) of x through the row helpers, in float64."""
    C = x.shape[1]
    buf, n = R.partial_rows_fwd(_mc(x), ROWS, dtype=F64)
    rows, cnt = R.rows_view(buf, n, C)
    return R.merge_fwd(rows, cnt, _mc(x).shape[0], bn.weight, bn.bias, bn.running_mean.clone(),
                       bn.running_var.clone(), MOM, EPS, dtype=F64)


@pytest.mark.parametrize("residual", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("relu", [False, True], ids=["norelu", "relu"])
def test_bn_ref_matches_autograd(relu, residual):
    g, x = _inputs(1)
    res = torch.randn(x.shape, generator=g, dtype=F64) if residual else None
    dy = torch.randn(x.shape, generator=g, dtype=F64)
    bn = _bn(x.shape[1], 2)
    mean, invstd, coef, new_rm, new_rv = _ref_forward(x, bn)  # (before the module updates its statistics)

    xr = x.clone().requires_grad_(True)
    rr = res.clone().requires_grad_(True) if residual else None
    y_ref = bn(xr)
    if residual:
        y_ref = y_ref + rr
    if relu:
        y_ref = torch.relu(y_ref)
    y_ref.backward(dy)

    M = _mc(x).shape[0]
    pre = R.apply_fwd(_mc(x), coef, _mc(res) if residual else None)
    y = pre.clamp_min(0.0) if relu else pre
    bits = (y > 0) if relu else None
    _close(_nchw(y, x), y_ref)
    _close(new_rm, bn.running_mean)
    _close(new_rv, bn.running_var)
    sg, sgx = R.bwd_sums(_mc(dy), bits, _mc(x), mean)
    dgamma, dbeta, bcoef = R.bwd_finalize(sg, sgx, M, bn.weight, mean, invstd)
    _close(dgamma, bn.weight.grad)
    _close(dbeta, bn.bias.grad)
    _close(_nchw(R.bwd_dx(bcoef, _mc(dy), bits, _mc(x)), x), xr.grad)
    if residual:  # dres = g
        gg = _mc(dy) * bits if relu else _mc(dy)
        _close(_nchw(gg, x), rr.grad)


@pytest.mark.parametrize("relu", [False, True], ids=["norelu", "relu"])
def test_bn_ref_two_branch_matches_autograd(relu):
    g, xa = _inputs(3)
    xb = torch.randn(xa.shape, generator=g, dtype=F64) * 0.6 - 0.2
    dy = torch.randn(xa.shape, generator=g, dtype=F64)
    ba, bb = _bn(xa.shape[1], 4), _bn(xa.shape[1], 5)
    fa, fb = _ref_forward(xa, ba), _ref_forward(xb, bb)

    xar, xbr = xa.clone().requires_grad_(True), xb.clone().requires_grad_(True)
    y_ref = ba(xar) + bb(xbr)
    if relu:
        y_ref = torch.relu(y_ref)
    y_ref.backward(dy)

    M = _mc(xa).shape[0]
    pre = R.apply_fwd(_mc(xa), fa[2]) + R.apply_fwd(_mc(xb), fb[2])
    y = pre.clamp_min(0.0) if relu else pre
    bits = (y > 0) if relu else None
    _close(_nchw(y, xa), y_ref)
    for f, bn in ((fa, ba), (fb, bb)):
        _close(f[3], bn.running_mean)
        _close(f[4], bn.running_var)
    sg, sga, sgb = R.bwd_sums2(_mc(dy), bits, _mc(xa), fa[0], _mc(xb), fb[0])
    sg1, sga1 = R.bwd_sums(_mc(dy), bits, _mc(xa), fa[0])
    assert torch.equal(sg, sg1) and torch.equal(sga, sga1)  # the one-input variant is its first two
    for s, f, bn, x, xr in ((sga, fa, ba, xa, xar), (sgb, fb, bb, xb, xbr)):
        dgamma, dbeta, bcoef = R.bwd_finalize(sg, s, M, bn.weight, f[0], f[1])
        _close(dgamma, bn.weight.grad)
        _close(dbeta, bn.bias.grad)
        _close(_nchw(R.bwd_dx(bcoef, _mc(dy), bits, _mc(x)), x), xr.grad)


def test_bn_ref_no_affine_no_running():
    """gamma = beta = None is gamma 1 / beta 0; rm = rv = None returns no running statistics."""
    g, x = _inputs(6)
    dy = torch.randn(x.shape, generator=g, dtype=F64)
    C, M = x.shape[1], _mc(x).shape[0]
    buf, n = R.partial_rows_fwd(_mc(x), 4, dtype=F64)
    rows, cnt = R.rows_view(buf, n, C)
    assert n == 4 and cnt.tolist() == [27.0, 27.0, 27.0, 24.0]
    mean, invstd, coef, new_rm, new_rv = R.merge_fwd(rows, cnt, M, None, None, None, None, MOM, EPS, dtype=F64)
    assert new_rm is None and new_rv is None
    bn = nn.BatchNorm2d(C, eps=EPS, affine=False, track_running_stats=False).double()
    xr = x.clone().requires_grad_(True)
    y_ref = bn(xr)
    y_ref.backward(dy)
    _close(_nchw(R.apply_fwd(_mc(x), coef), x), y_ref)
    sg, sgx = R.bwd_sums(_mc(dy), None, _mc(x), mean)
    _, _, bcoef = R.bwd_finalize(sg, sgx, M, None, mean, invstd)
    _close(_nchw(R.bwd_dx(bcoef, _mc(dy), None, _mc(x)), x), xr.grad)


@pytest.mark.parametrize("rows", [1, 3, 105, ROWS, [1] * 4 + [101]], ids=["1", "3", "pixelrows", "unequal", "ones"])
def test_merge_fwd_from_rows_is_the_statistics_of_x(rows):
    _, x = _inputs(7)
    xm = _mc(x)
    M, C = xm.shape
    mean_ref = xm.mean(0)
    var_ref = xm.var(0, unbiased=False)
    buf, n = R.partial_rows_fwd(xm, rows, dtype=F64)
    r, cnt = R.rows_view(buf, n, C)
    assert float(cnt.sum()) == M
    mean, invstd, coef, new_rm, new_rv = R.merge_fwd(r, cnt, M, None, None, torch.zeros(C), torch.zeros(C), 1.0, EPS,
                                                     dtype=F64)
    _close(mean, mean_ref)
    _close(invstd, 1.0 / torch.sqrt(var_ref + EPS))
    _close(new_rm, mean_ref)  # momentum 1: the running statistics are the batch's
    _close(new_rv, xm.var(0, unbiased=True))
    # f32 rows (what the kernels are handed) and one final f32 rounding.  A row mean rounded to f32 is
    # off by at most 2^-24 * |mean_t| ~ 6e-6 at mean 100, which moves the between-row term
    # n_t (mean_t - mean)^2 of a variance ~3 by less than 2 * 6e-6 * |mean_t - mean| per pixel: 1e-5 of it
    buf, n = R.partial_rows_fwd(xm, rows)
    assert buf.dtype == torch.float32
    r, cnt = R.rows_view(buf, n, C)
    mean, invstd, coef, _, new_rv = R.merge_fwd(r, cnt, M, None, None, torch.zeros(C), torch.zeros(C), 1.0, EPS)
    assert mean.dtype == invstd.dtype == coef.dtype == new_rv.dtype == torch.float32
    _close(mean, mean_ref, rtol=2e-7)
    _close(invstd, 1.0 / torch.sqrt(var_ref + EPS), rtol=1e-5)
    _close(new_rv, xm.var(0, unbiased=True), rtol=1e-5)


def test_pack_mask_bit_order():
    g = torch.Generator().manual_seed(8)
    keep = torch.rand(2, 16, 3, 5, generator=g) > 0.5
    m = R.pack_mask(keep)
    assert m.dtype == torch.uint8 and m.numel() == 2 * 16 * 3 * 5 // 8
    nhwc = keep.permute(0, 2, 3, 1).reshape(-1, 16)
    for p in (0, 7, 29):  # bit i of byte v of pixel p = channel 8v + i
        for v in range(2):
            assert int(m[p * 2 + v]) == sum(int(nhwc[p, 8 * v + i]) << i for i in range(8))
    assert torch.equal(R.pack_mask(nhwc), m)  # the [M, C] form
    assert torch.equal(R.unpack_mask(m, 16), nhwc)
    one = torch.zeros(1, 8, 1, 1, dtype=torch.bool)
    one[0, 3] = True
    assert R.pack_mask(one).tolist() == [8]
