"""Every route of the convolution kernels (csrc/sqr_conv.hip, csrc/sqr_conv3.hip) bitwise against float64 on
integer-exact operands (tests/_conv_exact.py: every product and every f32 partial sum is an integer below
2^24, so the f32 accumulator holds the true sum in any order and the only inexact step is the final
round-to-nearest-even cast).  Every stored tensor must satisfy torch.equal with ``ref_f64.to(dtype)``; no
tolerance.  A wrong element -- a halo cell not loaded, a lane off by one, a seam, the ring's last stage, a
short split -- flips hundreds of outputs (test_conv_exact_cpu.py::test_one_dropped_product_is_seen).

Each case runs with the direct kernels forced (sqr_conv_set_direct(2)) and off (0: the implicit GEMM), the
deep-ring tiles also as their 3-stage twins, bf16 and fp16 everywhere and f32 in mode 0, and asserts the
route it took from what the library reports: the number of statistics rows, whether the apply-on-load
forward is taken, and whether the masked-addend backward-data is.

Entries that round twice by design (their reference is two casts, ``acc2`` / ``macc2`` / ``s2acc2``):
  * persistent layer-1 kernel, + addend and + masked addend: the tile is staged in LDS as 16-bit values and
    the addend is added to the staged value on its way out (sqr_conv3.hip conv3p_kernel store_piece:
    ``v[e] = pack2<T>(lo2f<T>(v[e]) + lo2f<T>(ad), ...)``);
  * direct stride-2 backward-data, + addend and + compact addend: the four parity classes are staged as
    16-bit values (``store4((T*)(smem + ...), acc[...])``) and the addend is added in the copy-out
    (conv3s2_dgrad_kernel: ``vv[e] = pack2<T>(lo2f<T>(vv[e]) + lo2f<T>(aa[e]), ...)``);
  * implicit-GEMM backward-data + addend / + compact addend: a second kernel adds to the stored 16-bit
    result (sqr_conv.hip add_inplace_kernel, add_s2_compact_kernel).
The tiled stride-1 kernels (conv3_kernel) add the addend to the f32 accumulator: one rounding (``acc1``).
The two differ on 4-19 % of the elements of these cases, so an entry compared against the wrong one
fails: the rounding count is itself evidence of the route.

BatchNorm-backward partials, summed over rows in float64, equal the float64 sums of the stored g exactly
where the generator's bound holds (sum |g| |x - mean| * 4 < 2^24), elsewhere within 5e-7 relative + 1e-9
max (test_bn_links_gpu.py's bound for f32 rows summed in float64).  The forward's Welford rows are not
exact: 1e-5 against the stored output, as in test_conv_gpu.py."""
import ctypes

import pytest
import torch

import _conv_exact as ce

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DT_IDS = {BF16: "bf16", F16: "f16", F32: "f32"}
UNSUPPORTED = -2  # SQR_E_UNSUPPORTED


def _cl(t, dtype):
    return t.to(dtype).to(DEV).contiguous(memory_format=torch.channels_last)


def _same(got, exp, what):
    """torch.equal(got, exp.to(got.dtype)), with the number of differing elements in the message."""
    g = got.detach().cpu().double()
    assert g.shape == exp.shape, (what, tuple(g.shape), tuple(exp.shape))
    if not torch.equal(g, exp):
        bad = (g != exp)
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, expected %r"
                             % (what, int(bad.sum()), bad.numel(), idx, float(g[idx]), float(exp[idx])))


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def _welford_ok(st, y, what):
    """The forward-statistics partials (Welford rows + pixel counts) against the stored output: 1e-5."""
    from sqr.bn import partial_counts
    n = partial_counts(st).double()[:, None]
    m, q = st[:, 0].double(), st[:, 1].double()
    yd = y.detach().double()
    assert int(n.sum()) == yd.numel() // yd.shape[1], what
    e1, e2 = _rel((n * m).sum(0), yd.sum((0, 2, 3))), _rel((q + n * m * m).sum(0), (yd * yd).sum((0, 2, 3)))
    assert e1 <= 1e-5 and e2 <= 1e-5, (what, e1, e2)


def _bn_sums_ok(st, g_exp, bn_x, mean, exact, what):
    """BatchNorm-backward partial rows [rows, 2, C], summed in float64, against float64 sums of the stored g."""
    tot = st.double().sum(0).cpu()
    ref = ce.bn_sums(g_exp, bn_x, mean)
    assert tot.shape == ref.shape, what
    if exact:
        _same(tot, ref, what + " (exact sums)")
    else:
        bound = 5e-7 * ref.abs() + 1e-9 * float(ref.abs().max())
        worst = float(((tot - ref).abs() / bound.clamp_min(1e-300)).max())
        assert worst <= 1.0, "%s: worst error / bound = %.3g" % (what, worst)


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


class _Modes:
    """sqr_conv_set_direct / sqr_conv_set_deep_ring, restored on exit."""

    def __enter__(self):
        from sqr._lib import lib
        self.L = lib()
        self.direct = self.L.sqr_conv_set_direct(2)
        self.ring = self.L.sqr_conv_set_deep_ring(1)
        return self

    def set(self, direct, ring=1):
        self.L.sqr_conv_set_direct(direct)
        self.L.sqr_conv_set_deep_ring(ring)

    def __exit__(self, *exc):
        self.L.sqr_conv_set_deep_ring(self.ring)
        self.L.sqr_conv_set_direct(self.direct)


def _masked_acc(gyg, crsk, d, addg, maskg, dtype):
    """sqr_conv2d_bwd_data_acc_masked as sqr.conv's backward calls it -> (rc, dx)."""
    from sqr import conv as sc
    from sqr._lib import lib, ptr, stream_ptr
    dx = torch.empty((d.N, d.C, d.H, d.W), dtype=dtype, device=DEV, memory_format=torch.channels_last)
    ws, n = sc._ws(d, 1, gyg.device)
    rc = lib().sqr_conv2d_bwd_data_acc_masked(ptr(gyg), ptr(crsk), ptr(dx), ptr(addg), ptr(maskg), ctypes.byref(d),
                                              ptr(ws), n, stream_ptr(gyg.device))
    return rc, dx


# ------------------------------------------------------------------------ stride-1 3x3: every entry
def _s1_entries(o, shape, dtype, fwd, dgrad, tag):
    """All entries of one stride-1 3x3 case on the current mode; fwd / dgrad: the kernel expected for each
    direction (ce.P, a tile id, or None = the implicit GEMM)."""
    from sqr import conv as sc
    N, C, H, W, K = shape
    is16 = dtype != F32
    d = sc._desc(N, C, H, W, K, 3, 3, 1, 1, dtype)
    krsc, crsk = sc.pack_weight(o.w.float().to(DEV), d, True)
    xg, gyg, addg = _cl(o.x, dtype), _cl(o.gy, dtype), _cl(o.add, dtype)
    bxg, maskg, meang = _cl(o.bn_x, dtype), o.mask.to(DEV), o.mean.float().to(DEV)
    coefg = o.coef.float().to(DEV)
    M = N * H * W

    def rows_of(route, nout):
        if route == ce.P:
            rows, tpb = ce.persistent_rows(shape, _ncu())
            if shape in ce.BAND_CASES and _ncu() == 256:
                assert tpb == 2, (tag, "two tiles per workgroup: the row ring wraps")
            return rows
        if route is None:
            return ce.nt_rows(M, nout, is16)
        return ce.tile_rows(shape, route)

    # ---- forward + statistics
    y, st = sc.conv2d_fwd(xg, krsc, d, stats=True)
    assert st.shape == (rows_of(fwd, K), 2, K), (tag, "forward route", tuple(st.shape), fwd)
    _same(y, o.y_t, tag + " fwd")
    _welford_ok(st, y, tag + " fwd stats")

    # ---- forward with the preceding BatchNorm + ReLU applied on load
    has_bnin = is16 and (fwd == ce.P or fwd in ce.BNIN_TILES)
    r = sc.conv2d_fwd_bnin(xg, coefg, None, None, krsc, d)
    assert (r is not None) == has_bnin, (tag, "apply-on-load route", fwd)
    if r is not None:
        assert r[1].shape == (rows_of(fwd, K), 2, K), (tag, "apply-on-load route", tuple(r[1].shape))
        _same(r[0], o.y_bnin_t, tag + " fwd_bnin")
        _welford_ok(r[1], r[0], tag + " fwd_bnin stats")
    act = torch.full((N, C, H, W), float("nan"), dtype=dtype, device=DEV).contiguous(memory_format=torch.channels_last)
    amask = torch.full((M * C // 8,), 0x5A, dtype=torch.uint8, device=DEV)
    r = sc.conv2d_fwd_bnin(xg, coefg, act, amask, krsc, d)
    assert (r is not None) == (is16 and fwd == ce.P), (tag, "apply-on-load with side outputs", fwd)
    if r is not None:
        assert r[1].shape == (rows_of(fwd, K), 2, K)
        _same(r[0], o.y_bnin_t, tag + " fwd_bnin+side")
        _same(act, o.act, tag + " side-output activation")
        assert torch.equal(amask.cpu(), o.act_mask), tag + " side-output mask"
        _welford_ok(r[1], r[0], tag + " fwd_bnin+side stats")

    # ---- backward-data: plain, + addend, + masked addend.  A tile adds to its f32 accumulator (one
    # rounding); the persistent kernel and the implicit GEMM's second pass add to the 16-bit value (two)
    one = dgrad is not None and dgrad != ce.P
    _same(sc.conv2d_bwd_data(gyg, crsk, d), o.dx_t, tag + " bwd_data")
    _same(sc.conv2d_bwd_data_acc(gyg, crsk, d, addg), o.acc1 if one else o.acc2, tag + " bwd_data_acc")
    assert torch.equal(addg.cpu().double(), o.add), tag + ": the addend is not modified"
    rc, mdx = _masked_acc(gyg, crsk, d, addg, maskg, dtype)
    assert rc == (0 if (is16 and dgrad is not None) else UNSUPPORTED), (tag, "masked-addend route", rc, dgrad)
    if rc == 0:
        _same(mdx, o.macc1 if one else o.macc2, tag + " bwd_data_acc_masked")

    # ---- backward-data feeding the following BatchNorm's backward
    gg, bst = sc.conv2d_bwd_data_bn(gyg, crsk, d, bxg, maskg, meang)
    assert bst.shape[1:] == (2, C)
    if dgrad is not None:
        assert bst.shape[0] == rows_of(dgrad, C), (tag, "bwd_data_bn route", tuple(bst.shape), dgrad)
    _same(gg, o.g_t, tag + " bwd_data_bn g")
    _bn_sums_ok(bst, o.g_t, o.bn_x, o.mean, o.bn_exact, tag + " bwd_data_bn sums")

    # ---- ... with the mask recomputed from (bn_x, coefficients) and the activation written
    nso = is16 and fwd in ce.NSO_TILES and dgrad is not None and dgrad != ce.P
    assert sc.bnin_nso_supported(d) == nso, (tag, "no-side-output route", fwd, dgrad)
    if nso:
        aout = torch.full((N, C, H, W), float("nan"), dtype=dtype, device=DEV).contiguous(
            memory_format=torch.channels_last)
        ga, ast = sc.conv2d_bwd_data_bn_act(gyg, crsk, d, bxg, coefg, meang, aout)
        assert ast.shape == (rows_of(dgrad, C), 2, C)
        _same(ga, o.g_act_t, tag + " bwd_data_bn_act g")
        _same(aout, o.bn_act, tag + " bwd_data_bn_act act_out")
        _bn_sums_ok(ast, o.g_act_t, o.bn_x, o.mean, o.bn_act_exact, tag + " bwd_data_bn_act sums")

    # ---- weight gradient (f32, never rounded)
    _same(sc.conv2d_bwd_weight(xg, gyg, d), o.dw, tag + " bwd_weight")
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("case", ce.S1_CASES, ids=lambda c: "N%dC%dH%dW%dK%d" % c[0])
def test_conv3_s1_exact(case, dtype):
    """Every entry of a stride-1 3x3 case: direct mode 2 (the tile of ce.S1_CASES per direction), the
    deep-ring tiles' 3-stage twins, and mode 0 (implicit GEMM: the direct-only queries decline).  f32: mode 0."""
    shape, fwd, dgrad = case
    o = ce.gen(shape + (3, 1, 1), dtype)
    tag = "%s %s" % (shape, DT_IDS[dtype])
    with _Modes() as m:
        if dtype != F32:
            m.set(2, 1)
            _s1_entries(o, shape, dtype, fwd, dgrad, tag + " direct")
            if fwd in ce.RING_TWIN or dgrad in ce.RING_TWIN:
                m.set(2, 0)
                _s1_entries(o, shape, dtype, ce.RING_TWIN.get(fwd, fwd), ce.RING_TWIN.get(dgrad, dgrad),
                            tag + " direct, 3-stage ring")
        m.set(0, 1)
        _s1_entries(o, shape, dtype, None, None, tag + " gemm")


# ------------------------------------------------------------------------ stride-2 3x3
def _s2_desc(shape, dtype):
    from sqr import conv as sc
    N, C, H, W, K = shape
    return sc._desc(N, C, H, W, K, 3, 3, 2, 1, dtype)


@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("case", ce.S2F_CASES, ids=lambda c: "N%dC%dH%dW%dK%d" % c[0])
def test_conv3_s2_fwd_exact(case, dtype):
    """The direct stride-2 forward tiles 0 / 1 / 2 (mode 2: statistics rows N (Ho / TH) (Wo / TW)) and the
    implicit GEMM (mode 0), with the direct stride-2 weight gradient of the same conv.  Tiles 1 and 2 have
    64 output pixels, as the implicit GEMM's M tile at any small shape: for them the row count does not
    tell the routes apart (it would from N Ho Wo = 16384 on, where the GEMM's tile grows to 128); tile 0's
    (128 pixels) does."""
    from sqr import conv as sc
    shape, tile = case
    N, C, H, W, K = shape
    o = ce.gen(shape + (3, 2, 1), dtype)
    d = _s2_desc(shape, dtype)
    krsc, _ = sc.pack_weight(o.w.float().to(DEV), d, False)
    xg, gyg = _cl(o.x, dtype), _cl(o.gy, dtype)
    th, tw = ce.S2F_TILES[tile]
    assert o.Ho % th == 0 and o.Wo % tw == 0
    with _Modes() as m:
        for mode in ((2, 0) if dtype != F32 else (0,)):
            m.set(mode)
            tag = "%s %s mode %d" % (shape, DT_IDS[dtype], mode)
            y, st = sc.conv2d_fwd(xg, krsc, d, stats=True)
            rows = N * (o.Ho // th) * (o.Wo // tw) if mode == 2 else ce.nt_rows(N * o.Ho * o.Wo, K, dtype != F32)
            assert st.shape == (rows, 2, K), (tag, "route", tuple(st.shape))
            _same(y, o.y_t, tag + " fwd")
            _welford_ok(st, y, tag + " fwd stats")
            _same(sc.conv2d_bwd_weight(xg, gyg, d), o.dw, tag + " bwd_weight")
            torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("shape", ce.S2D_CASES, ids=lambda s: "N%dC%dH%dW%dK%d" % s)
def test_conv3_s2_dgrad_exact(shape, dtype):
    """The direct stride-2 backward-data tiles (one per (C, K)), plain, + addend and + compact addend, and
    the parity-class implicit GEMM (mode 0).  Both routes round the addend entries twice (module
    docstring), so no comparison or query tells them apart here; the tile is fixed by (C, K) and the
    divisibility of (Ho, Wo) alone (s2_pick), which these shapes meet."""
    from sqr import conv as sc
    N, C, H, W, K = shape
    o = ce.gen(shape + (3, 2, 1), dtype)
    d = _s2_desc(shape, dtype)
    _, crsk = sc.pack_weight(o.w.float().to(DEV), d, True)
    xg, gyg, addg, addcg = _cl(o.x, dtype), _cl(o.gy, dtype), _cl(o.add, dtype), _cl(o.addc, dtype)
    with _Modes() as m:
        for mode in ((2, 0) if dtype != F32 else (0,)):
            m.set(mode)
            tag = "%s %s mode %d" % (shape, DT_IDS[dtype], mode)
            _same(sc.conv2d_bwd_data(gyg, crsk, d), o.dx_t, tag + " bwd_data")
            _same(sc.conv2d_bwd_data_acc(gyg, crsk, d, addg), o.acc2, tag + " bwd_data_acc")
            _same(sc.conv2d_bwd_data_acc_s2(gyg, crsk, d, addcg), o.s2acc2, tag + " bwd_data_acc_s2")
            _same(sc.conv2d_bwd_weight(xg, gyg, d), o.dw, tag + " bwd_weight")
            torch.cuda.synchronize()


# ------------------------------------------------------------------------ weight gradient extras
@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("case", ce.WGRAD_EXTRA, ids=lambda s: "N%dC%dH%dW%dK%ds%d" % s)
def test_conv3_wgrad_exact(case, dtype):
    """(5, 512, 8, 8, 512): 5 chunks of 8 x 8 pixels in splits of 2 -- the last split is short; a stride-2
    case at an odd batch.  Direct (mode 2) and split-K implicit GEMM (mode 0)."""
    from sqr import conv as sc
    N, C, H, W, K, st = case
    o = ce.gen((N, C, H, W, K, 3, st, 1), dtype)
    d = sc._desc(N, C, H, W, K, 3, 3, st, 1, dtype)
    xg, gyg = _cl(o.x, dtype), _cl(o.gy, dtype)
    with _Modes() as m:
        for mode in ((2, 0) if dtype != F32 else (0,)):
            m.set(mode)
            _same(sc.conv2d_bwd_weight(xg, gyg, d), o.dw, "%s %s mode %d bwd_weight" % (case, DT_IDS[dtype], mode))
            torch.cuda.synchronize()


# ------------------------------------------------------------------------ implicit GEMM only
@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("case", ce.GEMM_CASES, ids=ce.case_id)
def test_conv_gemm_exact(case, dtype):
    """Shapes only the implicit GEMM takes (odd sizes, H != W, 1x1 / 5x5 / 7x7, im2col for C < 8), mode 0:
    forward + statistics, backward-data (C >= 8) plain and + addend (two roundings: add_inplace_kernel),
    weight gradient; the im2col cases also with the forward's workspace as the column matrix."""
    from sqr import conv as sc
    N, C, H, W, K, R, st, pad = case
    o = ce.gen(case, dtype)
    d = sc._desc(N, C, H, W, K, R, R, st, pad, dtype)
    krsc, crsk = sc.pack_weight(o.w.float().to(DEV), d, C >= 8)
    xg, gyg = _cl(o.x, dtype), _cl(o.gy, dtype)
    tag = "%s %s" % (case, DT_IDS[dtype])
    with _Modes() as m:
        m.set(0)
        y, stt, ws = sc.conv2d_fwd(xg, krsc, d, return_ws=True, stats=True)
        assert stt.shape == (ce.nt_rows(N * o.Ho * o.Wo, K, dtype != F32), 2, K), (tag, tuple(stt.shape))
        _same(y, o.y_t, tag + " fwd")
        _welford_ok(stt, y, tag + " fwd stats")
        if C >= 8:
            _same(sc.conv2d_bwd_data(gyg, crsk, d), o.dx_t, tag + " bwd_data")
            _same(sc.conv2d_bwd_data_acc(gyg, crsk, d, _cl(o.add, dtype)), o.acc2, tag + " bwd_data_acc")
        else:
            _same(sc.conv2d_bwd_weight(xg, gyg, d, col=ws), o.dw, tag + " bwd_weight (forward's columns)")
        _same(sc.conv2d_bwd_weight(xg, gyg, d), o.dw, tag + " bwd_weight")
        torch.cuda.synchronize()
