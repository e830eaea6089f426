"""The fused BatchNorm "links" of a BasicBlock, each entry point alone against the float64
references of _bn_ref.py (masks and statistics are inputs there, so the reference is exact up to one
rounding), then chains of two sqr.resnet.BasicBlock against a float64 chain that is handed the GPU's
own ReLU masks:

  (a) sqr_bn_fwd_finalize on synthetic Welford rows (both merge_stats_w paths, null gamma / beta,
      null running statistics);
  (b) sqr_bn_apply against float64 x * scale + shift (+ residual), and its ReLU mask;
  (c) sqr_bn_bwd_stats / sqr_bn_bwd_apply on synthetic f32 backward rows (both sum_partials_w paths);
  (d) sqr_conv2d_bwd_weight_bn: the finalize and reduction jobs riding each of the three split-K sum
      kernels, with job geometries unlike the conv's;
  (e) sqr_bn_bwd_part / sqr_bn_add_bwd_part fed with (d)'s partials, bitwise against sqr_bn_bwd /
      sqr_bn_add_bwd and against float64;
  chains: the blocks' own forward (links on) against the same blocks composed from the public ops
      (links off) and the float64 chain.

Tolerances.  Statistics and coefficients that both sides form in float64 from the same f32 rows and
round once: rtol 5e-7 (4 f32 ulps) + 1e-9 * max|ref|.  Elementwise outputs: one rounding of the output
type against the float64 value (f32: 2 ulps = 2^-22; bf16: 2^-8; f16: 2^-11, relative) plus a floor of
1e-6 * max|ref| for the f32 fma in front of it."""
import copy
import ctypes
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _bn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
F64 = torch.float64

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT_IDS = ["f32", "bf16", "f16"]
DT_NAME = dict(zip(DTYPES, DT_IDS))
DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
ROUND = {torch.float32: 2.0 ** -22, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
NAN = float("nan")

# pixel / channel shapes by the reduction geometry of red_plan (sqr_bn.hip): V = C / 8 channel vectors,
# 256 / V pixel rows per block, chunk = max(ceil(M / 512), 4 rows) rounded up to whole rows
MC = [(75, 8),       # one partial block, V = 1
      (1200, 32),    # five blocks of 256 pixels, the last partial (176)
      (512, 64),     # four full blocks
      (128, 512),    # V = 64, 4 rows per block, eight blocks
      (4096, 128)]   # 64 blocks
MC_IDS = ["M%dC%d" % s for s in MC]
ROWS = [1, 3, 64, 65, 512, 513, 1100]  # > 512 rows: the loop paths of merge_stats_w / sum_partials_w


def _L():
    from sqr._lib import lib
    return lib()


def _st():
    from sqr._lib import stream_ptr
    return stream_ptr(torch.device(DEV))


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _ll(v):
    return ctypes.c_longlong(v)


def _rnd(t, dtype):
    """f32 values representable in dtype: what the reference sees is what the kernel is given."""
    return t.to(dtype).float()


def _dev(t, dtype=None):
    t = t.to(DEV)
    return (t.to(dtype) if dtype is not None else t).contiguous()


def _guard(n, dtype, fill, extra=64):
    """(whole buffer, its first n elements): the tail keeps `fill` unless a kernel writes past n."""
    buf = torch.full((n + extra,), fill, dtype=dtype, device=DEV)
    return buf, buf[:n]


def _tail_intact(buf, n, fill):
    tail = buf[n:]
    return bool(torch.isnan(tail).all()) if fill != fill else bool((tail == fill).all())


def _assert_stat(got, ref, what):
    """|got - ref| <= 5e-7 |ref| + 1e-9 max|ref|: both sides sum the same f32 rows in float64 and round
    once to f32."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert torch.isfinite(got).all(), what
    bound = 5e-7 * ref.abs() + 1e-9 * float(ref.abs().max())
    worst = float(((got - ref).abs() / bound.clamp_min(1e-300)).max())
    assert worst <= 1.0, "%s: worst error / bound = %.3g" % (what, worst)


def _assert_rounded(got, ref, dtype, what, floor=1e-6):
    """|got - ref| <= ROUND[dtype] |ref| + floor * max|ref|, elementwise against the float64 value."""
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    assert torch.isfinite(got).all(), what
    bound = ROUND[dtype] * ref.abs() + floor * float(ref.abs().max())
    worst = float(((got - ref).abs() / bound.clamp_min(1e-300)).max())
    assert worst <= 1.0, "%s: worst error / bound = %.3g" % (what, worst)


def _assert_abs(got, ref, what, tol=1e-5):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert torch.isfinite(got).all(), what
    err = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)
    assert err <= tol, "%s: max error / max|ref| = %.3g" % (what, err)


def _row_sizes(rows):
    """Unequal row sizes with one-pixel rows among them."""
    return [(13, 1, 2, 7)[i % 4] for i in range(rows)]


# ---------------------------------------------------------------- (a) sqr_bn_fwd_finalize
@functools.lru_cache(maxsize=None)
def _fwd_rows(rows, C):
    sizes = _row_sizes(rows)
    M = sum(sizes)
    g = torch.Generator().manual_seed(rows * 131 + C)
    x = torch.randn(M, C, generator=g)
    x[:, :C // 2] += 100.0  # half the channels: mean ~ 100, std ~ 1
    x[:, C // 2:] = x[:, C // 2:] * 1.7 + 0.3
    buf, n = R.partial_rows_fwd(x, sizes)
    assert n == rows
    return M, buf


@pytest.mark.parametrize("running", [True, False], ids=["running", "norunning"])
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "noaffine"])
@pytest.mark.parametrize("C", [64, 8], ids=["C64", "C8"])
@pytest.mark.parametrize("rows", ROWS, ids=lambda r: "rows%d" % r)
def test_fwd_finalize(rows, C, affine, running):
    """sqr_bn_fwd_finalize against merge_fwd on the same f32 rows (the entry point has no activation
    dtype: the rows and every output are f32)."""
    L = _L()
    M, buf = _fwd_rows(rows, C)
    r, cnt = R.rows_view(buf, rows, C)
    g = torch.Generator().manual_seed(rows + C)
    gamma = torch.rand(C, generator=g) + 0.5 if affine else None
    beta = torch.randn(C, generator=g) * 0.3 if affine else None
    rm0 = torch.randn(C, generator=g) * 0.2 if running else None
    rv0 = torch.rand(C, generator=g) + 0.5 if running else None
    ref = R.merge_fwd(r, cnt, M, gamma, beta, rm0, rv0, 0.1, 1e-5)

    d_buf = _dev(buf)
    d_gamma, d_beta = (_dev(gamma), _dev(beta)) if affine else (None, None)
    d_rm, d_rv = (_dev(rm0), _dev(rv0)) if running else (None, None)
    mean_b, mean = _guard(C, torch.float32, NAN)
    inv_b, inv = _guard(C, torch.float32, NAN)
    coef_b, coef = _guard(2 * C, torch.float32, NAN)
    rc = L.sqr_bn_fwd_finalize(_p(d_buf), rows, _ll(M), C, _p(d_gamma), _p(d_beta), _p(d_rm), _p(d_rv),
                               ctypes.c_float(0.1), ctypes.c_float(1e-5), _p(mean), _p(inv), _p(coef), _st())
    assert rc == 0, L.sqr_last_error_string()
    torch.cuda.synchronize()
    _assert_stat(mean, ref[0], "save_mean")
    _assert_stat(inv, ref[1], "save_invstd")
    _assert_stat(coef[:C], ref[2][:C], "scale")
    _assert_stat(coef[C:], ref[2][C:], "shift")
    if running:
        _assert_stat(d_rm, ref[3], "running_mean")
        _assert_stat(d_rv, ref[4], "running_var")
    for b, n in ((mean_b, C), (inv_b, C), (coef_b, 2 * C)):
        assert _tail_intact(b, n, NAN)
    assert torch.equal(d_buf.cpu(), buf)  # the rows are inputs


# ---------------------------------------------------------------- (b) sqr_bn_apply
@functools.lru_cache(maxsize=None)
def _apply_ops(M, C, dtype):
    g = torch.Generator().manual_seed(M + C)
    x = _rnd(torch.randn(M, C, generator=g) * 1.5 + 0.3, dtype)
    res = _rnd(torch.randn(M, C, generator=g), dtype)
    coef = torch.cat([torch.randn(C, generator=g) * 0.8, torch.randn(C, generator=g) * 0.5])  # some scales < 0
    return x, res, coef


@pytest.mark.parametrize("residual", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("relu", [0, 1], ids=["norelu", "relu"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mc", MC, ids=MC_IDS)
def test_bn_apply(mc, dtype, relu, residual):
    L = _L()
    M, C = mc
    x, res, coef = _apply_ops(M, C, dtype)
    pre = R.apply_fwd(x, coef, res if residual else None)
    ref = pre.clamp_min(0.0) if relu else pre
    big = float(pre.abs().max())

    dx, dres, dcoef = _dev(x, dtype), (_dev(res, dtype) if residual else None), _dev(coef)
    y_b, y = _guard(M * C, dtype, NAN)
    m_b, m = _guard(M * C // 8, torch.uint8, 0x5A)
    rc = L.sqr_bn_apply(_p(dx), _ll(M), C, DT[dtype], _p(dcoef), _p(dres), relu, _p(y), _p(m), _st())
    assert rc == 0, L.sqr_last_error_string()
    torch.cuda.synchronize()
    assert _tail_intact(y_b, M * C, NAN)
    _assert_rounded(y, ref, dtype, "y")
    if not relu:
        assert bool((m_b == 0x5A).all())  # no ReLU: the mask buffer is not touched
        return
    assert _tail_intact(m_b, M * C // 8, 0x5A)
    bits = R.unpack_mask(m.cpu(), C)
    assert torch.equal(bits, y.cpu().float().reshape(M, C) > 0)  # the mask of the STORED values
    sure = pre.abs() > 1e-5 * big
    assert torch.equal(bits[sure], (pre > 0)[sure])


# ---------------------------------------------------------------- (c) sqr_bn_bwd_stats, sqr_bn_bwd_apply
@functools.lru_cache(maxsize=None)
def _bwd_rows(rows, C, dtype):
    """Operands of a BatchNorm backward whose sums arrive as f32 rows: g already masked; the rows are
    float64 sums over disjoint pixel chunks, stored as f32."""
    sizes = _row_sizes(rows)
    M = sum(sizes)
    gen = torch.Generator().manual_seed(rows * 17 + C)
    x = _rnd(torch.randn(M, C, generator=gen) * 1.3 + 0.4, dtype)
    keep = torch.rand(M, C, generator=gen) > 0.4
    g = _rnd(torch.randn(M, C, generator=gen), dtype) * keep
    mean = x.double().mean(0).float()
    invstd = (1.0 / torch.sqrt(x.double().var(0, unbiased=False) + 1e-5)).float()
    gamma = torch.rand(C, generator=gen) + 0.5
    row_id = torch.repeat_interleave(torch.arange(rows), torch.tensor(sizes))
    st = torch.zeros(rows, 2, C, dtype=F64)
    st[:, 0].index_add_(0, row_id, g.double())
    st[:, 1].index_add_(0, row_id, g.double() * (x.double() - mean.double()))
    return M, x, g, mean, invstd, gamma, st.float()


@pytest.mark.parametrize("affine", [True, False], ids=["gamma", "nogamma"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C", [64, 8], ids=["C64", "C8"])
@pytest.mark.parametrize("rows", ROWS, ids=lambda r: "rows%d" % r)
def test_bn_bwd_stats_and_apply(rows, C, dtype, affine):
    L = _L()
    M, x, g, mean, invstd, gamma, st = _bwd_rows(rows, C, dtype)
    gam = gamma if affine else None
    sg, sgx = st[:, 0].double().sum(0), st[:, 1].double().sum(0)  # the f64 sum of the f32 rows
    dgamma_r, dbeta_r, coef_r = R.bwd_finalize(sg, sgx, M, gam, mean, invstd)
    coef32 = coef_r.float()  # the coefficients are f32 in the ABI
    dx_r = R.bwd_dx(coef32, g, None, x)

    dg, dxx, dst = _dev(g, dtype), _dev(x, dtype), _dev(st)
    dmean, dinv, dgam = _dev(mean), _dev(invstd), (_dev(gamma) if affine else None)
    dx_b, dx = _guard(M * C, dtype, NAN)
    dgamma_b, dgamma = _guard(C, torch.float32, NAN)
    dbeta_b, dbeta = _guard(C, torch.float32, NAN)
    ws_b, ws = _guard(3 * C, torch.float32, NAN)
    rc = L.sqr_bn_bwd_stats(_p(dg), _p(dxx), _ll(M), C, DT[dtype], _p(dst), rows, _p(dgam), _p(dmean), _p(dinv), _p(dx),
                            _p(dgamma), _p(dbeta), _p(ws), 3 * C * 4, _st())
    assert rc == 0, L.sqr_last_error_string()
    torch.cuda.synchronize()
    _assert_stat(dgamma, dgamma_r, "dgamma")
    _assert_stat(dbeta, dbeta_r, "dbeta")
    for q, name in enumerate(("k1", "k2", "k3")):  # the finalized coefficients sit in the workspace
        _assert_stat(ws[q * C:(q + 1) * C], coef_r[q * C:(q + 1) * C], name)
    _assert_rounded(dx, dx_r, dtype, "dx (bwd_stats)")
    for b, n in ((dx_b, M * C), (dgamma_b, C), (dbeta_b, C), (ws_b, 3 * C)):
        assert _tail_intact(b, n, NAN)

    # sqr_bn_bwd_apply with the reference's coefficients
    dx2_b, dx2 = _guard(M * C, dtype, NAN)
    rc = L.sqr_bn_bwd_apply(_p(dg), _p(dxx), _ll(M), C, DT[dtype], _p(_dev(coef32)), _p(dx2), _st())
    assert rc == 0, L.sqr_last_error_string()
    torch.cuda.synchronize()
    _assert_rounded(dx2, dx_r, dtype, "dx (bwd_apply)")
    assert _tail_intact(dx2_b, M * C, NAN)


# ---------------------------------------------------------------- (d) sqr_conv2d_bwd_weight_bn
# Which split-K sum kernel a weight gradient ends in (sqr_conv.hip bwd_weight_impl):
#   * 16-bit 3x3 / pad 1 convs that plan_w (sqr_conv3.hip) takes -- C and K multiples of 64, the output
#     width a power of two >= 8, the height a multiple of the tile's -- run the direct kernel, whose slabs
#     are already KCRS: wgrad_sum_kernel.  The smallest such shape is one 8 x 8 image, C = K = 64 (tile
#     TW 8 x TH 8).  In f32 the same shape runs the implicit GEMM and lands in wgrad_reduce_tc_kernel.
#   * every other conv runs conv_tn_kernel with plan_tn's split count; a 1x1 conv's slab [K][C] is KCRS
#     too: wgrad_sum_kernel, in every dtype.
#   * otherwise launch_wgrad_reduce: wgrad_reduce_tc_kernel when C % 64 == 0, at most 16 taps and at most
#     16 splits, else wgrad_reduce_kernel.  A 12-wide map is refused by plan_w (not a power of two), and
#     its 288 output pixels cap plan_tn at ceil(288 / BK) = 9 (f32, BK 32) or 5 (16-bit, BK 64) splits:
#     tc for C = 64 3x3; the scatter kernel for C = 32 (C % 64 != 0) and for 5x5 (25 taps > 16).
# name: (N, C, H, K, R, pad, dtypes, fin (M, C, rows), red (M, C)).  The jobs' geometries differ from each
# other and from the conv's: riding workgroups must index by their job.  fin rows 513: the loop path of
# sum_partials_w inside the riding finalize.
_16 = (torch.bfloat16, torch.float16)
WG = {
    "sum_1x1": (2, 64, 16, 128, 1, 0, DTYPES, (512, 8, 5), (1200, 32)),
    "sum_3x3": (1, 64, 8, 64, 3, 1, _16, (75, 8, 3), (4096, 128)),
    "tc_3x3": (2, 64, 12, 64, 3, 1, DTYPES, (512, 8, 513), (128, 512)),
    "tc_3x3_small": (1, 64, 8, 64, 3, 1, (torch.float32,), (75, 8, 3), (4096, 128)),
    "reduce_c32": (2, 32, 12, 64, 3, 1, DTYPES, (1200, 16, 3), (512, 64)),
    "reduce_5x5": (2, 64, 12, 64, 5, 2, DTYPES, (512, 32, 65), (75, 8)),
}
WG_CASES = [(n, dt) for n, v in WG.items() for dt in v[6]]
JOBS = ["none", "fin", "red1", "red2", "fin_red1", "fin_red2"]


class _Wgrad:
    """One conv's weight-gradient operands on the GPU."""

    def __init__(self, N, C, H, K, Rk, pad, dtype, seed):
        from sqr import conv as sc
        self.L = _L()
        self.d = sc._desc(N, C, H, H, K, Rk, Rk, 1, pad, dtype)
        Ho = H + 2 * pad - Rk + 1
        g = torch.Generator().manual_seed(seed)
        self.x = torch.randn(N, C, H, H, generator=g).to(DEV).to(dtype).contiguous(memory_format=CL)
        self.dy = torch.randn(N, K, Ho, Ho, generator=g).to(DEV).to(dtype).contiguous(memory_format=CL)
        self.n = K * C * Rk * Rk

    def run(self, fin=None, red=None, plain=False):
        """(rc, dw buffer with its guard tail)"""
        L = self.L
        dw_b, dw = _guard(self.n, torch.float32, NAN)
        old = L.sqr_conv_set_direct(1)  # the default routing, whatever an earlier test left (plan_w reads it)
        try:
            nws = L.sqr_conv2d_workspace_bytes(ctypes.byref(self.d), 2)
            ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=DEV)
            if plain:
                rc = L.sqr_conv2d_bwd_weight(_p(self.x), _p(self.dy), _p(dw), ctypes.byref(self.d), _p(ws), nws, _st())
            else:
                rc = L.sqr_conv2d_bwd_weight_bn(_p(self.x), _p(self.dy), _p(dw), ctypes.byref(self.d),
                                                ctypes.byref(fin) if fin is not None else None,
                                                ctypes.byref(red) if red is not None else None, _p(ws), nws, _st())
        finally:
            L.sqr_conv_set_direct(old)
        torch.cuda.synchronize()
        return rc, dw_b


@functools.lru_cache(maxsize=None)
def _wgrad_case(name, dtype):
    N, C, H, K, Rk, pad = WG[name][:6]
    w = _Wgrad(N, C, H, K, Rk, pad, dtype, N + C + H + K + Rk)
    rc, dw_b = w.run(plain=True)
    assert rc == 0, w.L.sqr_last_error_string()
    assert _tail_intact(dw_b, w.n, NAN) and bool(torch.isfinite(dw_b[:w.n]).all())
    return w, dw_b[:w.n].clone()


@functools.lru_cache(maxsize=None)
def _fin_ops(M, C, rows):
    """A riding finalize job's inputs (f32 rows of some BatchNorm's backward sums) and its reference."""
    g = torch.Generator().manual_seed(M + C + rows)
    st = torch.randn(rows, 2, C, generator=g)
    gamma = torch.rand(C, generator=g) + 0.5
    mean = torch.randn(C, generator=g)
    invstd = torch.rand(C, generator=g) + 0.5
    ref = R.bwd_finalize(st[:, 0].double().sum(0), st[:, 1].double().sum(0), M, gamma, mean, invstd)
    return st, gamma, mean, invstd, ref


@functools.lru_cache(maxsize=None)
def _red_ops(M, C, dtype):
    """A block-output BatchNorm's backward operands: dy, ReLU bits, both branch inputs, statistics."""
    g = torch.Generator().manual_seed(M * 3 + C)
    o = {"dy": _rnd(torch.randn(M, C, generator=g), dtype),
         "xa": _rnd(torch.randn(M, C, generator=g) * 1.3 + 0.4, dtype),
         "xb": _rnd(torch.randn(M, C, generator=g) * 0.7 - 0.3, dtype),
         "keep": torch.rand(M, C, generator=g) > 0.4,
         "gamma_a": torch.rand(C, generator=g) + 0.5, "gamma_b": torch.rand(C, generator=g) + 0.5}
    for s in "ab":
        xd = o["x" + s].double()
        o["mean_" + s] = xd.mean(0).float()
        o["invstd_" + s] = (1.0 / torch.sqrt(xd.var(0, unbiased=False) + 1e-5)).float()
    return o


class _Fin:
    def __init__(self, M, C, rows, gamma=True):
        from sqr._lib import SqrBnBwdFin
        st, gam, mean, invstd, self.ref = _fin_ops(M, C, rows)
        self.C = C
        self.t = [_dev(st), _dev(gam), _dev(mean), _dev(invstd)]
        self.dgamma_b, self.dgamma = _guard(C, torch.float32, NAN)
        self.dbeta_b, self.dbeta = _guard(C, torch.float32, NAN)
        self.coef_b, self.coef = _guard(3 * C, torch.float32, NAN)
        f = SqrBnBwdFin()
        f.stats, f.stats_rows, f.M, f.C = self.t[0].data_ptr(), rows, M, C
        f.gamma = self.t[1].data_ptr() if gamma else None
        f.save_mean, f.save_invstd = self.t[2].data_ptr(), self.t[3].data_ptr()
        f.dgamma, f.dbeta, f.coef = self.dgamma.data_ptr(), self.dbeta.data_ptr(), self.coef.data_ptr()
        self.job = f

    def check(self):
        C = self.C
        dgamma_r, dbeta_r, coef_r = self.ref
        _assert_stat(self.dgamma, dgamma_r, "riding dgamma")
        _assert_stat(self.dbeta, dbeta_r, "riding dbeta")
        for q, name in enumerate(("k1", "k2", "k3")):
            _assert_stat(self.coef[q * C:(q + 1) * C], coef_r[q * C:(q + 1) * C], "riding " + name)
        for b, n in ((self.dgamma_b, C), (self.dbeta_b, C), (self.coef_b, 3 * C)):
            assert _tail_intact(b, n, NAN)

    def untouched(self):
        return all(bool(torch.isnan(b).all()) for b in (self.dgamma_b, self.dbeta_b, self.coef_b))


class _Red:
    def __init__(self, kind, M, C, dtype, mask=True, C_job=None):
        from sqr._lib import SqrBnBwdRed
        o = _red_ops(M, C, dtype)
        self.kind, self.M, self.C, self.o = kind, M, C, o
        # (the riding reduction always reads a mask: all ones stands for "no ReLU")
        self.keep = o["keep"] if mask else torch.ones(M, C, dtype=torch.bool)
        self.dy, self.xa, self.xb = _dev(o["dy"], dtype), _dev(o["xa"], dtype), _dev(o["xb"], dtype)
        self.mask = _dev(R.pack_mask(self.keep))
        self.mean_a, self.mean_b = _dev(o["mean_a"]), _dev(o["mean_b"])
        self.n = _L().sqr_bn_bwd_red_doubles(_ll(M), C, kind)
        self.part_b, self.part = _guard(max(self.n, 1), F64, NAN)
        self.rows = ctypes.c_int(-1)
        r = SqrBnBwdRed()
        r.kind, r.dy, r.relu_mask = kind, self.dy.data_ptr(), self.mask.data_ptr()
        r.x_a, r.mean_a = self.xa.data_ptr(), self.mean_a.data_ptr()
        r.x_b = self.xb.data_ptr() if kind == 2 else None
        r.mean_b = self.mean_b.data_ptr() if kind == 2 else None
        r.M, r.C, r.part = M, (C if C_job is None else C_job), self.part.data_ptr()
        r.part_rows = ctypes.pointer(self.rows)
        self.job = r

    def sums_ref(self):
        o = self.o
        if self.kind == 1:
            return torch.stack(R.bwd_sums(o["dy"], self.keep, o["xa"], o["mean_a"]))
        return torch.stack(R.bwd_sums2(o["dy"], self.keep, o["xa"], o["mean_a"], o["xb"], o["mean_b"]))

    def abs_sums(self):
        o = self.o
        g = (o["dy"].double() * self.keep).abs()
        t = [g.sum(0), (g * (o["xa"].double() - o["mean_a"].double()).abs()).sum(0)]
        if self.kind == 2:
            t.append((g * (o["xb"].double() - o["mean_b"].double()).abs()).sum(0))
        return torch.stack(t)

    def check(self):
        """The partials' shape, their guard, and their row sums against float64: the kernel adds 8
        (kind 2: 4) products in f32 per step before its f64 accumulation, so each group is good to about
        8 * 2^-24 of its absolute sum: 1e-6 * sum|terms| per channel and statistic."""
        rows = self.rows.value
        assert rows >= 1 and rows * (self.kind + 1) * self.C == self.n
        assert _tail_intact(self.part_b, self.n, NAN)
        part = self.part.cpu().view(rows, self.kind + 1, self.C)
        assert bool(torch.isfinite(part).all())  # every block wrote its row
        err = (part.sum(0) - self.sums_ref()).abs()
        bound = 1e-6 * self.abs_sums()
        worst = float((err / bound.clamp_min(1e-300)).max())
        assert worst <= 1.0, "riding sums: worst error / bound = %.3g" % worst
        return part, rows


@pytest.mark.parametrize("jobs", JOBS)
@pytest.mark.parametrize("case", WG_CASES, ids=lambda c: "%s-%s" % (c[0], DT_NAME[c[1]]))
def test_bwd_weight_bn(case, jobs):
    name, dtype = case
    w, dw_ref = _wgrad_case(name, dtype)
    fin_g, red_g = WG[name][7], WG[name][8]
    fin = _Fin(*fin_g) if "fin" in jobs else None
    red = _Red(int(jobs[-1]), red_g[0], red_g[1], dtype) if "red" in jobs else None
    rc, dw_b = w.run(fin.job if fin else None, red.job if red else None)
    assert rc == 0, w.L.sqr_last_error_string()
    assert _tail_intact(dw_b, w.n, NAN)
    assert torch.equal(dw_b[:w.n], dw_ref)  # the riding work never changes the weight gradient
    if fin:
        fin.check()
    if red:
        red.check()


def test_bwd_weight_bn_fin_without_gamma():
    """The riding finalize's affine=False select (gamma NULL: gamma 1)."""
    w, dw_ref = _wgrad_case("sum_1x1", torch.bfloat16)
    fin = _Fin(512, 8, 5, gamma=False)
    st, _, mean, invstd, _ = _fin_ops(512, 8, 5)
    fin.ref = R.bwd_finalize(st[:, 0].double().sum(0), st[:, 1].double().sum(0), 512, None, mean, invstd)
    rc, dw_b = w.run(fin.job, None)
    assert rc == 0, w.L.sqr_last_error_string()
    assert torch.equal(dw_b[:w.n], dw_ref)
    fin.check()


# ---------------------------------------------------------------- (e) sqr_bn_bwd_part, sqr_bn_add_bwd_part
def _operand(x, gamma, mean, invstd):
    from sqr._lib import SqrBnOperand
    o = SqrBnOperand()
    o.x, o.gamma = x.data_ptr(), gamma.data_ptr()
    o.save_mean, o.save_invstd = mean.data_ptr(), invstd.data_ptr()
    o.eps = 1e-5
    return o


def _ride(kind, M, C, dtype, mask=True):
    """(d)'s partials of one BatchNorm backward: a reduction job riding the small 1x1 weight gradient."""
    w, dw_ref = _wgrad_case("sum_1x1", dtype)
    red = _Red(kind, M, C, dtype, mask=mask)
    rc, dw_b = w.run(None, red.job)
    assert rc == 0, w.L.sqr_last_error_string()
    assert torch.equal(dw_b[:w.n], dw_ref)
    red.check()
    return red


@pytest.mark.parametrize("variant", ["dres", "nodres", "nomask"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mc", MC, ids=MC_IDS)
def test_bn_bwd_part(mc, dtype, variant):
    """sqr_bn_bwd_part on riding partials against sqr_bn_bwd on the same operands (bitwise: both run
    reduce_block and the same finalize on the same red_plan) and against float64."""
    L = _L()
    M, C = mc
    has_mask = variant != "nomask"
    red = _ride(1, M, C, dtype, mask=has_mask)
    o = red.o
    gamma, invstd = _dev(o["gamma_a"]), _dev(o["invstd_a"])
    mask = red.mask if has_mask else None  # NULL: no ReLU in the forward
    want_dres = variant != "nodres"
    nws = L.sqr_bn_workspace_bytes(_ll(M), C)
    outs = []
    for part in (True, False):
        dx_b, dx = _guard(M * C, dtype, NAN)
        dres_b, dres = _guard(M * C, dtype, NAN)
        dg_b, dg = _guard(C, torch.float32, NAN)
        db_b, db = _guard(C, torch.float32, NAN)
        if part:
            ws_b, ws = _guard(3 * C, torch.float32, NAN)
            rc = L.sqr_bn_bwd_part(_p(red.dy), _p(mask), _p(red.xa), _ll(M), C, DT[dtype], _p(red.part), red.rows.value,
                                   _p(gamma), _p(red.mean_a), _p(invstd), _p(dx), _p(dres) if want_dres else None,
                                   _p(dg), _p(db), _p(ws), 3 * C * 4, _st())
        else:
            ws_b, ws = _guard(max(nws, 16), torch.uint8, 0x5A)
            rc = L.sqr_bn_bwd(_p(red.dy), _p(mask), _p(red.xa), _ll(M), C, DT[dtype], _p(gamma), _p(red.mean_a),
                              _p(invstd), _p(dx), _p(dres) if want_dres else None, _p(dg), _p(db), _p(ws), nws, _st())
        assert rc == 0, L.sqr_last_error_string()
        torch.cuda.synchronize()
        assert _tail_intact(dx_b, M * C, NAN) and _tail_intact(dg_b, C, NAN) and _tail_intact(db_b, C, NAN)
        assert _tail_intact(dres_b, M * C if want_dres else 0, NAN)
        if part:
            assert _tail_intact(ws_b, 3 * C, NAN)
        outs.append((dx.clone(), dres.clone() if want_dres else None, dg.clone(), db.clone()))
    a, b = outs
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    sg, sgx = R.bwd_sums(o["dy"], red.keep, o["xa"], o["mean_a"])
    dgamma_r, dbeta_r, coef_r = R.bwd_finalize(sg, sgx, M, o["gamma_a"], o["mean_a"], o["invstd_a"])
    _assert_abs(a[2], dgamma_r, "dgamma")
    _assert_abs(a[3], dbeta_r, "dbeta")
    _assert_rounded(a[0], R.bwd_dx(coef_r, o["dy"], red.keep, o["xa"]), dtype, "dx", floor=1e-5)
    if want_dres:
        assert torch.equal(a[1], b[1])
        assert torch.equal(a[1].cpu().float().reshape(M, C), o["dy"] * red.keep)  # dres = g, exactly


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mc", MC, ids=MC_IDS)
def test_bn_add_bwd_part(mc, dtype):
    """sqr_bn_add_bwd_part on riding kind-2 partials against sqr_bn_add_bwd (bitwise: reduce2_block and
    the same finalize) and against float64: both dx, all four parameter gradients."""
    L = _L()
    M, C = mc
    red = _ride(2, M, C, dtype)
    o = red.o
    t = [_dev(o[k]) for k in ("gamma_a", "invstd_a", "gamma_b", "invstd_b")]
    oa = _operand(red.xa, t[0], red.mean_a, t[1])
    ob = _operand(red.xb, t[2], red.mean_b, t[3])
    nws = L.sqr_bn_add_workspace_bytes(_ll(M), C)
    outs = []
    for part in (True, False):
        bufs = [_guard(M * C, dtype, NAN), _guard(M * C, dtype, NAN)] + [_guard(C, torch.float32, NAN) for _ in range(4)]
        (_, dxa), (_, dxb), (_, dga), (_, dba), (_, dgb), (_, dbb) = bufs
        if part:
            ws_b, ws = _guard(6 * C, torch.float32, NAN)
            rc = L.sqr_bn_add_bwd_part(ctypes.byref(oa), ctypes.byref(ob), _p(red.dy), _p(red.mask), _ll(M), C, DT[dtype],
                                       _p(red.part), red.rows.value, _p(dxa), _p(dxb), _p(dga), _p(dba), _p(dgb), _p(dbb),
                                       _p(ws), 6 * C * 4, _st())
        else:
            ws_b, ws = _guard(max(nws, 16), torch.uint8, 0x5A)
            rc = L.sqr_bn_add_bwd(ctypes.byref(oa), ctypes.byref(ob), _p(red.dy), _p(red.mask), _ll(M), C, DT[dtype],
                                  _p(dxa), _p(dxb), _p(dga), _p(dba), _p(dgb), _p(dbb), _p(ws), nws, _st())
        assert rc == 0, L.sqr_last_error_string()
        torch.cuda.synchronize()
        for (b, v) in bufs:
            assert _tail_intact(b, v.numel(), NAN)
        if part:
            assert _tail_intact(ws_b, 6 * C, NAN)
        outs.append([v.clone() for _, v in bufs])
    for u, v in zip(*outs):
        assert torch.equal(u, v)
    dxa, dxb, dga, dba, dgb, dbb = outs[0]
    sg, sga, sgb = R.bwd_sums2(o["dy"], red.keep, o["xa"], o["mean_a"], o["xb"], o["mean_b"])
    for s, br, dx, dg, db in (("a", sga, dxa, dga, dba), ("b", sgb, dxb, dgb, dbb)):
        dgamma_r, dbeta_r, coef_r = R.bwd_finalize(sg, br, M, o["gamma_" + s], o["mean_" + s], o["invstd_" + s])
        _assert_abs(dg, dgamma_r, "dgamma_" + s)
        _assert_abs(db, dbeta_r, "dbeta_" + s)
        _assert_rounded(dx, R.bwd_dx(coef_r, o["dy"], red.keep, o["x" + s]), dtype, "dx_" + s, floor=1e-5)


def test_link_argument_checks():
    """Calls that must return an error before any launch (every pointer handed over is valid and every
    buffer full-sized): the outputs keep their sentinels."""
    L = _L()
    dtype = torch.bfloat16
    M, C = 512, 64
    red = _ride(1, M, C, dtype)
    o = red.o
    gamma, invstd = _dev(o["gamma_a"]), _dev(o["invstd_a"])
    dx_b, dx = _guard(M * C, dtype, NAN)
    dg_b, dg = _guard(C, torch.float32, NAN)
    db_b, db = _guard(C, torch.float32, NAN)
    ws_b, ws = _guard(3 * C, torch.float32, NAN)

    def part_call(rows, ws_bytes):
        return L.sqr_bn_bwd_part(_p(red.dy), _p(red.mask), _p(red.xa), _ll(M), C, DT[dtype], _p(red.part), rows, _p(gamma),
                                 _p(red.mean_a), _p(invstd), _p(dx), None, _p(dg), _p(db), _p(ws), ws_bytes, _st())
    assert part_call(0, 3 * C * 4) == -1                       # rows = 0: SQR_E_INVALID_ARG
    assert part_call(red.rows.value, 3 * C * 4 - 1) == -3      # workspace < 3 * C floats: SQR_E_WORKSPACE
    st = _dev(torch.zeros(4, 2, C))
    assert L.sqr_bn_bwd_stats(_p(red.dy), _p(red.xa), _ll(M), C, DT[dtype], _p(st), 0, _p(gamma), _p(red.mean_a),
                              _p(invstd), _p(dx), _p(dg), _p(db), _p(ws), 3 * C * 4, _st()) == -1
    assert L.sqr_bn_bwd_stats(_p(red.dy), _p(red.xa), _ll(M), C, DT[dtype], _p(st), 4, _p(gamma), _p(red.mean_a),
                              _p(invstd), _p(dx), _p(dg), _p(db), _p(ws), 3 * C * 4 - 1, _st()) == -3
    torch.cuda.synchronize()
    for b in (dx_b, dg_b, db_b, ws_b):
        assert bool(torch.isnan(b).all())
    # a reduction job with C = 24 (C / 8 does not divide 256): refused before the weight gradient runs.
    # Its tensors are the full-sized C = 64 ones.
    w, _ = _wgrad_case("sum_1x1", dtype)
    bad = _Red(1, M, C, dtype, C_job=24)
    fin = _Fin(512, 8, 5)
    rc, dw_b = w.run(fin.job, bad.job)
    assert rc == -1
    assert bool(torch.isnan(dw_b).all()) and bool(torch.isnan(bad.part_b).all()) and fin.untouched()
    assert bad.rows.value == -1


# ---------------------------------------------------------------- chains of two BasicBlocks
CHAINS = {  # name: (input shape, blocks as (inplanes, planes, stride))
    "id_id": ((2, 64, 16, 16), [(64, 64, 1), (64, 64, 1)]),
    "id_ds": ((2, 64, 16, 16), [(64, 64, 1), (64, 128, 2)]),     # 16x16 -> 8x8
    "ds_id": ((2, 64, 32, 32), [(64, 128, 2), (128, 128, 1)]),   # 32x32 -> 16x16; the out link is kind 2
}
LINK_CALLS = ("sqr_conv2d_bwd_weight_bn", "sqr_bn_bwd_apply", "sqr_bn_bwd_part", "sqr_bn_add_bwd_part")


def _expected_calls(chain, dtype):
    """Link calls of one backward through blocks A -> B (sqr/resnet.py, sqr/bn.py, sqr/conv.py), in
    autograd's order.
    Every dtype: each block's conv2 backward-data produces bn1's sums (BnBackwardLink), so conv2's weight
      gradient carries bn1's finalize (sqr_conv2d_bwd_weight_bn, one per block) and bn1's backward is
      sqr_bn_bwd_apply (one per block).
    16-bit only (a ResidualJoin, hence a BnOutLink, needs a 16-bit input that requires grad): B's conv1
      backward-data adds the residual share in its epilogue, so its result is the whole gradient of A's
      output and A's output BatchNorm reduction rides B's conv1 weight gradient (a third
      sqr_conv2d_bwd_weight_bn); A's output BatchNorm backward is then sqr_bn_bwd_part (A an identity
      block, kind 1) or sqr_bn_add_bwd_part (A with a downsample, kind 2).  B's output BatchNorm has no
      consumer conv and A's conv1 no producer link: both run unlinked.
    f32: no join, so no out link: only the bn1 links."""
    if dtype == torch.float32:
        return dict(zip(LINK_CALLS, (2, 2, 0, 0)))
    kind2 = chain == "ds_id"
    return dict(zip(LINK_CALLS, (3, 2, 0 if kind2 else 1, 1 if kind2 else 0)))


# The six backward-data entries, counted next to the link calls: which of them each conv's input gradient
# takes is the route choice of sqr.conv's backward.
DGRAD_CALLS = ("sqr_conv2d_bwd_data", "sqr_conv2d_bwd_data_acc", "sqr_conv2d_bwd_data_acc_s2",
               "sqr_conv2d_bwd_data_acc_masked", "sqr_conv2d_bwd_data_bn", "sqr_conv2d_bwd_data_bn_act")
# (chain, 16-bit, direct): (linked run, plain run), each in DGRAD_CALLS' order; a call counts whether the
# entry takes it or refuses it (with direct 0 sqr_conv2d_bwd_data_acc_masked refuses, and the addend goes
# expanded through sqr_conv2d_bwd_data_acc).  Recorded from the code before the route choice became one
# function.
DGRAD_EXPECTED = {
    ("id_id", False, 2): ((2, 0, 0, 0, 2, 0), (4, 0, 0, 0, 0, 0)),
    ("id_id", False, 0): ((2, 0, 0, 0, 2, 0), (4, 0, 0, 0, 0, 0)),
    ("id_id", True, 2): ((0, 0, 0, 2, 2, 0), (4, 0, 0, 0, 0, 0)),
    ("id_id", True, 0): ((0, 2, 0, 2, 2, 0), (4, 0, 0, 0, 0, 0)),
    ("id_ds", False, 2): ((3, 0, 0, 0, 2, 0), (5, 0, 0, 0, 0, 0)),
    ("id_ds", False, 0): ((3, 0, 0, 0, 2, 0), (5, 0, 0, 0, 0, 0)),
    ("id_ds", True, 2): ((1, 0, 1, 1, 2, 0), (5, 0, 0, 0, 0, 0)),
    ("id_ds", True, 0): ((1, 1, 1, 1, 2, 0), (5, 0, 0, 0, 0, 0)),
    ("ds_id", False, 2): ((3, 0, 0, 0, 2, 0), (5, 0, 0, 0, 0, 0)),
    ("ds_id", False, 0): ((3, 0, 0, 0, 2, 0), (5, 0, 0, 0, 0, 0)),
    ("ds_id", True, 2): ((1, 0, 1, 1, 0, 2), (5, 0, 0, 0, 0, 0)),
    ("ds_id", True, 0): ((1, 1, 1, 1, 2, 0), (5, 0, 0, 0, 0, 0)),
}


def _expected_dgrad(chain, dtype, direct):
    return tuple(dict(zip(DGRAD_CALLS, row)) for row in DGRAD_EXPECTED[chain, dtype != torch.float32, direct])


def _make_chain(chain):
    from sqr.conv import Conv2d
    from sqr.resnet import BasicBlock
    torch.manual_seed(sum(map(ord, chain)))
    blocks = []
    for cin, cout, stride in CHAINS[chain][1]:
        ds = None
        if stride != 1 or cin != cout:
            ds = nn.Sequential(Conv2d(cin, cout, 1, stride, 0, bias=False), nn.BatchNorm2d(cout))
        blocks.append(BasicBlock(cin, cout, stride, ds))
    seq = nn.Sequential(*blocks)
    for m in seq.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.weight.data = torch.rand(m.num_features) + 0.5
            m.bias.data = torch.randn(m.num_features) * 0.2
            m.running_mean.data = torch.randn(m.num_features) * 0.1
            m.running_var.data = torch.rand(m.num_features) + 0.5
    return seq.train()


def _plain_forward(seq, x):
    """The same blocks from the public ops alone: no join, link, out_link or defer."""
    from sqr.bn import bn_act, bn_add_act
    masks, h = [], x
    for blk in seq:
        o = bn_act(blk.conv1.forward_stats(h, blk.bn1), blk.bn1, relu=True)
        if blk.downsample is not None:
            y = bn_add_act(blk.conv2.forward_stats(o, blk.bn2), blk.bn2,
                           blk.downsample[0].forward_stats(h, blk.downsample[1]), blk.downsample[1], relu=True)
        else:
            y = bn_act(blk.conv2.forward_stats(o, blk.bn2), blk.bn2, residual=h, relu=True)
        masks.append(((o.detach() > 0).cpu().double(), (y.detach() > 0).cpu().double()))
        h = y
    return h, masks


def _ref_chain(seq, x0, gy, masks, dtype):
    """The chain in float64 on the CPU: conv weights rounded to the compute dtype, batch statistics,
    every ReLU a multiplication by the plain run's mask.  (dx, {name: grad})."""
    P = {n: (p.detach().to(dtype) if p.dim() == 4 else p.detach()).double().requires_grad_(True)
         for n, p in seq.named_parameters()}
    x = x0.double().requires_grad_(True)
    h = x
    for i, blk in enumerate(seq):
        def bn(t, name):
            return F.batch_norm(t, None, None, P["%d.%s.weight" % (i, name)], P["%d.%s.bias" % (i, name)], True, 0.0,
                                1e-5)
        o = bn(F.conv2d(h, P["%d.conv1.weight" % i], stride=blk.stride, padding=1), "bn1") * masks[i][0]
        t = bn(F.conv2d(o, P["%d.conv2.weight" % i], padding=1), "bn2")
        idn = h if blk.downsample is None else \
            bn(F.conv2d(h, P["%d.downsample.0.weight" % i], stride=blk.stride), "downsample.1")
        h = (t + idn) * masks[i][1]
    h.backward(gy.double())
    return x.grad, {n: p.grad for n, p in P.items()}


def _l2(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).norm() / ref.norm().clamp_min(1e-300))


@pytest.mark.parametrize("direct", [2, 0], ids=["direct2", "direct0"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("chain", list(CHAINS))
def test_block_chain(chain, dtype, direct, monkeypatch):
    L = _L()
    shape = CHAINS[chain][0]
    base = _make_chain(chain)
    g = torch.Generator().manual_seed(len(chain) + shape[2])
    x0 = _rnd(torch.randn(shape, generator=g), dtype)
    counts = dict.fromkeys(LINK_CALLS + DGRAD_CALLS, 0)

    def counting(name):
        fn = getattr(L, name)

        def wrapper(*a):
            counts[name] += 1
            return fn(*a)
        return wrapper
    for name in counts:
        monkeypatch.setattr(L, name, counting(name))

    old = L.sqr_conv_set_direct(direct)
    try:
        runs = {}
        for which in ("linked", "plain"):
            seq = copy.deepcopy(base).to(DEV)
            x = x0.to(DEV).to(dtype).contiguous(memory_format=CL).requires_grad_(True)
            for k in counts:
                counts[k] = 0
            if which == "linked":
                y = seq(x)  # the blocks' own forward
            else:
                y, masks = _plain_forward(seq, x)
            if which == "linked":
                gy = _rnd(torch.randn(y.shape, generator=g), dtype)
            y.backward(gy.to(DEV).to(dtype).contiguous(memory_format=CL))
            torch.cuda.synchronize()
            runs[which] = (y.detach(), x.grad, seq, dict(counts))
    finally:
        L.sqr_conv_set_direct(old)

    (yl, dxl, seql, nl), (yp, dxp, seqp, npl) = runs["linked"], runs["plain"]
    dl, dp = ({k: n.pop(k) for k in DGRAD_CALLS} for n in (nl, npl))
    print("dgrad_calls (%r, %r, %d): (%r, %r)," % (chain, dtype != torch.float32, direct, tuple(dl.values()),
                                                   tuple(dp.values())))
    assert (dl, dp) == _expected_dgrad(chain, dtype, direct)  # every input gradient took its route
    assert nl == _expected_calls(chain, dtype), nl  # the links fired ...
    assert nl["sqr_conv2d_bwd_weight_bn"] > 0 and nl["sqr_bn_bwd_apply"] > 0
    if dtype != torch.float32:
        assert nl["sqr_bn_bwd_part"] + nl["sqr_bn_add_bwd_part"] > 0
    assert not any(npl.values()), npl               # ... and only in the linked run
    assert torch.equal(yl, yp)
    for (n, a), (_, b) in zip(seql.named_buffers(), seqp.named_buffers()):
        if n.endswith("running_mean") or n.endswith("running_var"):
            assert torch.equal(a, b), n

    dx_r, grads_r = _ref_chain(base, x0, gy, masks, dtype)
    rows = [("input", _l2(dxl, dx_r), _l2(dxp, dx_r))]
    pl, pp = dict(seql.named_parameters()), dict(seqp.named_parameters())
    for n in grads_r:
        assert pl[n].grad is not None and pp[n].grad is not None, n
        rows.append((n, _l2(pl[n].grad, grads_r[n]), _l2(pp[n].grad, grads_r[n])))
    for n, el, ep in rows:  # L2-relative error against float64, linked and plain
        print("bn_links_accuracy %-6s %-5s direct%d %-28s linked %.3e plain %.3e" % (chain, DT_NAME[dtype], direct, n, el,
                                                                                   ep))
    for n, el, ep in rows:
        assert el <= 2.0 * ep + 1e-6, "%s: linked %.3e > 2 * plain %.3e + 1e-6" % (n, el, ep)
