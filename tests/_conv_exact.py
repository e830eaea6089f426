"""Integer-exact operands and float64 references for the bitwise convolution tests
(test_conv_exact_cpu.py, test_conv_exact_gpu.py).  CPU only.

The method.  With small integer operands every product of a convolution and every partial sum of
such products is an integer; while its magnitude stays below 2^24 a float32 accumulator holds it
exactly, whatever the accumulation order (tiles, chunks, split-K slabs, MFMA shapes).  The only
inexact step left in a kernel is then the final round-to-nearest-even cast of the accumulator to
bf16 / fp16, which torch.Tensor.to performs the same way: the stored tensor must equal
``ref_f64.to(dtype)`` bit for bit, and torch.equal decides with no tolerance to choose.

The generator asserts the conditions that make "exact" true for each case, from the convolution of
the operands' magnitudes (conv(|x|, |w|) bounds every partial sum of every output):
  * forward, backward-data: max conv(|x|, |w|) (+ max |addend|) < 2^24;
  * weight gradient: the bound sums over all N * Ho * Wo pixels;
  * fp16: max |y| < 65504 / 2;
  * BatchNorm-backward sums (mean: multiples of 1/4, so 4 g (x - mean) is an integer): compared
    exactly only where sum |g| |x - mean| * 4 < 2^24 per channel (``bn_exact``).
Operand ranges: x, gy in [-8, 8]; w in [-4, 4] (bf16, f32) or [-32, 32] (fp16: 11 significand bits
need larger sums before the cast rounds); addends in [-64, 64]; apply-on-load scale in
{+-1/2, +-1, +-2}, shift integer in [-4, 4], mostly positive (a padded halo cell wrongly computed as
relu(shift) instead of 0 then changes the output).  Cases whose outputs sum fewer than 256 products draw x
and w from the upper part of these ranges (short_sums), so that their casts round too.
"""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

LIM = float(1 << 24)
F16_LIM = 65504.0 / 2

# ---------------------------------------------------------------------------------------- cases
# Direct stride-1 3x3 tiles of csrc/sqr_conv3.hip (kD3Tiles): id -> (IMGS, TH, TW); one statistics row
# per tile of IMGS * TH * TW pixels.
TILES = {0: (1, 4, 64), 7: (1, 8, 32), 1: (1, 8, 32), 8: (1, 8, 16), 2: (1, 8, 16), 10: (2, 8, 8), 5: (2, 8, 8),
         3: (1, 8, 8), 4: (1, 16, 16)}
BNIN_TILES = (7, 8, 10, 1, 2, 5)   # tiles with an apply-on-load forward
NSO_TILES = (7, 8, 1, 2)           # ... whose convs take a deferred BatchNorm output without side outputs
RING_TWIN = {7: 1, 8: 2, 10: 5}    # deep-weight-ring tile -> its 3-stage twin (sqr_conv_set_deep_ring(0))
P = "persistent"

# (N, C, H, W, K), the kernel direct mode 2 selects for the forward (C -> K) and for the backward-data
# (K -> C): P, a tile id, or None = no direct kernel takes it (the implicit GEMM runs).
# Statistics rows: tiles (N / IMGS) * (H / TH) * (W / TW), persistent N * bands-per-image; the implicit
# GEMM writes ceil(N H W / BM) rows with BM = 64 at these sizes (nt_rows), which equals a tile's count
# only where the tile has 64 pixels (tile 3: its route shows in the masked-addend query, and in the
# single rounding of its addend epilogue, not in the row count).
S1_CASES = [
    # persistent 64-wide maps, 2-row tiles
    ((1, 64, 2, 64, 64), P, P),
    ((3, 64, 6, 64, 64), P, P),
    # persistent 128-wide maps, 1-row tiles (odd heights)
    ((1, 64, 1, 128, 64), P, P),
    ((2, 64, 3, 128, 64), P, P),
    # persistent bands of two tiles per workgroup on a 256-CU device: the row ring wraps
    ((65, 64, 8, 64, 64), P, P),
    ((130, 64, 2, 128, 64), P, P),
    # tile 0 (64 -> 64, 64-wide tiles of 4 rows; several tiles per row)
    ((1, 64, 4, 256, 64), 0, 0),
    ((1, 64, 8, 512, 64), 0, 0),
    # tiles 7 / 1 (32 x 8).  64 -> 128 at 8 rows: no direct backward-data (128 -> 64 fits tile 4 only from 16
    # rows on: the neighbour below)
    ((1, 64, 8, 32, 128), 7, None),
    ((1, 64, 16, 32, 128), 7, 4),
    ((1, 128, 24, 64, 128), 7, 7),
    ((1, 256, 8, 32, 256), 7, 7),
    # tiles 8 / 2 (16 x 8)
    ((1, 128, 8, 16, 128), 8, 8),
    ((2, 256, 24, 16, 256), 8, 8),
    # tiles 10 / 5 (two 8 x 8 images per tile)
    ((2, 64, 8, 8, 64), 10, 10),
    ((4, 512, 8, 8, 512), 10, 10),
    # tile 3 (one 8 x 8 tile: odd batch, or taller than 8)
    ((1, 128, 8, 8, 128), 3, 3),
    ((3, 512, 16, 8, 256), 3, 3),
    # tile 4 (16 x 16); 128 -> 64 forward, its backward-data (64 -> 128) on tile 8
    ((1, 64, 16, 16, 64), 4, 4),
    ((1, 128, 32, 16, 64), 4, 8),
]
BAND_CASES = [(65, 64, 8, 64, 64), (130, 64, 2, 128, 64)]

# Stride-2 3x3 forward tiles (kD3S2FTiles): id -> (TH, TW) of output pixels.  (N, C, H, W, K), tile.
S2F_TILES = {0: (4, 32), 1: (4, 16), 2: (8, 8)}
S2F_CASES = [
    ((1, 64, 8, 64, 128), 0), ((2, 64, 16, 128, 128), 0),
    ((1, 128, 8, 32, 256), 1), ((1, 256, 16, 64, 256), 1),
    ((1, 128, 16, 16, 128), 2), ((1, 256, 32, 16, 512), 2),
]
# Stride-2 backward-data (kS2DTiles: one tile per layer geometry, chosen by (C, K) alone; no query of
# the library tells it from the implicit GEMM, whose addend paths round the same way)
S2D_CASES = [
    (1, 64, 16, 64, 128), (1, 64, 32, 128, 128),
    (1, 128, 8, 32, 256), (2, 128, 24, 32, 256),
    (1, 256, 16, 16, 512), (1, 256, 32, 16, 512),
]
# Weight gradient beyond the shapes above: 5 chunks of 8 x 8 over 2-chunk splits (the last split is short),
# and a stride-2 case at an odd batch
WGRAD_EXTRA = [(5, 512, 8, 8, 512, 1), (3, 128, 8, 32, 256, 2)]

# Implicit GEMM only: (N, C, H, W, K, R, stride, pad)
GEMM_CASES = [
    (1, 8, 5, 13, 16, 3, 1, 1),
    (2, 16, 9, 14, 8, 5, 2, 2),
    (1, 64, 7, 9, 128, 1, 2, 0),
    (1, 64, 7, 9, 128, 1, 1, 0),
    (1, 1, 20, 36, 64, 7, 2, 3),
    (2, 3, 31, 17, 64, 7, 2, 3),
    (3, 32, 12, 20, 64, 3, 2, 1),
]


def all_conv_cases():
    """Every (N, C, H, W, K, R, stride, pad) the GPU file runs."""
    out = [s + (3, 1, 1) for s, _, _ in S1_CASES]
    out += [s + (3, 2, 1) for s, _ in S2F_CASES]
    out += [s + (3, 2, 1) for s in S2D_CASES]
    out += [s[:5] + (3, s[5], 1) for s in WGRAD_EXTRA]
    out += list(GEMM_CASES)
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


def direct_conv_cases():
    """The cases of the direct kernels (3x3, 64+ channels): the sums are large enough for the 16-bit cast
    to round a good share of the outputs."""
    return [c for c in all_conv_cases() if c not in GEMM_CASES]


def case_id(c):
    return "N%dC%dH%dW%dK%dR%ds%dp%d" % tuple(c)


def tile_rows(shape, tile):
    N, _, H, W, _ = shape
    imgs, th, tw = TILES[tile]
    assert N % imgs == 0 and H % th == 0 and W % tw == 0
    return (N // imgs) * (H // th) * (W // tw)


def persistent_rows(shape, ncu):
    """(rows, tiles per band) of the persistent kernel as conv3p_launch lays it out on ncu compute units."""
    N, _, H, W, _ = shape
    tpi = H // (2 if W == 64 else 1)
    bpi = 1
    for d in range(1, tpi + 1):
        if tpi % d == 0 and N * d <= ncu:
            bpi = d
    return N * bpi, tpi // bpi


def nt_rows(M, K, is16):
    """Statistics rows of the implicit GEMM: one per M tile of the config nt_cfg (sqr_conv.hip) picks."""
    def nblk(bm, bn):
        return -(-M // bm) * -(-K // bn)
    if K >= 128 and nblk(128, 128) >= 512:
        bm = 128
    elif is16 and K >= 128 and nblk(128, 128) >= 256:
        bm = 128
    elif nblk(128, 64) >= 512:
        bm = 128
    else:
        bm = 64
    return -(-M // bm)


# ------------------------------------------------------------------------------------- operands
def _ri(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _ri_mag(g, lo, hi, *shape):
    """Integers of magnitude lo .. hi with a random sign."""
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return _ri(g, lo, hi, *shape) * sign


def short_sums(case):
    """An output of this case sums fewer than 256 products (input channels x the taps that can fall
    inside the image: a one-row map has 3 of a 3x3 kernel's 9).  Uniform draws of the ranges then give
    sums that mostly stay below bf16's 256 / fp16's 2048, under which every integer is exact, and the
    cast would round only a few per cent of the outputs (6.8 % / 5.1 % on the one-row 128-wide case).
    For these cases x and w are drawn from the upper part of the same ranges (|x| in 5 .. 8, |w| in
    3 .. 4, fp16 24 .. 32; random signs), which lifts the sums' spread by about 1.9x; every bound the
    generator asserts still applies."""
    _, C, H, W, _, R, _, _ = case
    return C * min(R, H) * min(R, W) < 256


def w_range(dtype):
    return 32 if dtype == torch.float16 else 4


def pack_bits(keep_nchw):
    """1-bit mask in the NHWC element order, 8 channels per byte (bit i = channel 8v + i)."""
    bits = keep_nchw.permute(0, 2, 3, 1).reshape(-1, 8).to(torch.int64)
    return (bits << torch.arange(8)).sum(1).to(torch.uint8)


def cast(t, dtype):
    """The value a kernel stores: float64 -> dtype, one round-to-nearest-even (as float64 again)."""
    return t.to(dtype).double()


def _seed(case):
    s = 0
    for v in case:
        s = s * 131 + int(v)
    return s % (1 << 31)


@functools.lru_cache(maxsize=3)
def gen(case, dtype):
    """Operands and expected tensors (all float64 on the CPU, NCHW) of one conv case
    (N, C, H, W, K, R, stride, pad) in one dtype; asserts the exactness conditions.  The cached
    namespace is shared between tests: treat it as read-only.

    The fp16 range condition (max |y| < 65504 / 2) is a property of the drawn operands alone: where
    the first seed of a case misses it (the 512-channel sums reach 4.5 sigma ~ 3e4) the next seed is
    drawn, a fixed sequence per case; the partial-sum bounds hold for every draw of these ranges and
    are asserted, not retried."""
    base = _seed(case) + {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[dtype]
    for attempt in range(8):
        try:
            return _gen(case, dtype, base + 7919 * attempt)
        except _Fp16Range:
            continue
    raise AssertionError(("no fp16-range-safe operands in 8 draws", case))


class _Fp16Range(Exception):
    pass


def _f16_ok(t, extra=0.0):
    if float(t.abs().max()) + extra >= F16_LIM:
        raise _Fp16Range()


def _gen(case, dtype, seed):
    N, C, H, W, K, R, st, pad = case
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = (H + 2 * pad - R) // st + 1, (W + 2 * pad - R) // st + 1
    o = SimpleNamespace(case=case, dtype=dtype, Ho=Ho, Wo=Wo)
    wr = w_range(dtype)
    if short_sums(case):
        # few terms per output: magnitudes from the upper part of the same ranges (see short_sums)
        o.x = _ri_mag(g, 5, 8, N, C, H, W)
        o.w = _ri_mag(g, (3 * wr) // 4, wr, K, C, R, R)
    else:
        o.x = _ri(g, -8, 8, N, C, H, W)
        o.w = _ri(g, -wr, wr, K, C, R, R)
    o.gy = _ri(g, -8, 8, N, K, Ho, Wo)
    o.add = _ri(g, -64, 64, N, C, H, W)
    o.keep = torch.rand(N, C, H, W, generator=g) > 0.4
    conv = dict(stride=st, padding=pad)

    # ---- forward
    o.y = F.conv2d(o.x, o.w, **conv)
    o.y_bound = float(F.conv2d(o.x.abs(), o.w.abs(), **conv).max())
    assert o.y_bound < LIM, ("forward partial sums", case, o.y_bound)
    if dtype == torch.float16:
        _f16_ok(o.y)
    o.y_t = cast(o.y, dtype)

    # ---- weight gradient (f32, never rounded: the bound covers the sum over all N * Ho * Wo pixels)
    o.dw = torch.nn.grad.conv2d_weight(o.x, o.w.shape, o.gy, **conv)
    o.dw_bound = float(torch.nn.grad.conv2d_weight(o.x.abs(), o.w.shape, o.gy.abs(), **conv).max())
    assert o.dw_bound < LIM, ("weight-gradient sums", case, o.dw_bound)

    # ---- backward-data and its epilogues
    o.dx = torch.nn.grad.conv2d_input(o.x.shape, o.w, o.gy, **conv)
    o.dx_bound = float(torch.nn.grad.conv2d_input(o.x.shape, o.w.abs(), o.gy.abs(), **conv).max()) + 64.0
    assert o.dx_bound < LIM, ("backward-data partial sums", case, o.dx_bound)
    if dtype == torch.float16:
        _f16_ok(o.dx, 64.0)
    o.dx_t = cast(o.dx, dtype)
    o.mask = pack_bits(o.keep) if C % 8 == 0 else None
    madd = o.add * o.keep
    # + addend: one rounding where the kernel adds to its f32 accumulator (acc1), two where it adds to
    # the 16-bit value it staged (acc2); the same with the ReLU-masked addend (macc)
    o.acc1, o.acc2 = cast(o.dx + o.add, dtype), cast(o.dx_t + o.add, dtype)
    o.macc1, o.macc2 = cast(o.dx + madd, dtype), cast(o.dx_t + madd, dtype)
    if st == 2 and H % 2 == 0 and W % 2 == 0:  # compact addend on the (even, even) pixels
        o.addc = _ri(g, -64, 64, N, C, H // 2, W // 2)
        full = torch.zeros_like(o.dx)
        full[:, :, ::2, ::2] = o.addc
        o.s2acc1, o.s2acc2 = cast(o.dx + full, dtype), cast(o.dx_t + full, dtype)

    # ---- the following BatchNorm's backward: g = dgrad * mask, (sum g, sum g (x - mean))
    o.bn_x = _ri(g, -8, 8, N, C, H, W)
    o.mean = _ri(g, -4, 4, C) / 4.0
    o.g_t = o.dx_t * o.keep
    o.bn_exact = _bn_bound(o.g_t, o.bn_x, o.mean) < LIM

    # ---- BatchNorm + ReLU applied on load: the conv of relu(scale * x_pre + shift) in the dtype
    # (|scale x + shift| <= 20 in steps of 1/2: exact in bf16, so the activation itself never rounds)
    scale = torch.tensor([0.5, -0.5, 1.0, -1.0, 2.0, -2.0], dtype=torch.float64)[torch.randint(0, 6, (C,), generator=g)]
    shift = _ri(g, -4, 4, C)
    shift = torch.where(torch.rand(C, generator=g) < 0.7, shift.abs(), shift)
    o.coef = torch.cat([scale, shift])
    bc = lambda v: v.view(1, C, 1, 1)
    o.act = cast(torch.relu(o.x * bc(scale) + bc(shift)), dtype)
    assert torch.equal(o.act, torch.relu(o.x * bc(scale) + bc(shift)))
    o.act_mask = pack_bits(o.act > 0) if C % 8 == 0 else None
    o.y_bnin_bound = float(F.conv2d(o.act, o.w.abs(), **conv).max())
    assert o.y_bnin_bound < LIM
    o.y_bnin = F.conv2d(o.act, o.w, **conv)
    if dtype == torch.float16:
        _f16_ok(o.y_bnin)
    o.y_bnin_t = cast(o.y_bnin, dtype)
    # backward-data feeding that BatchNorm's backward with the mask recomputed from (bn_x, coef)
    o.bn_act = torch.relu(o.bn_x * bc(scale) + bc(shift))
    o.g_act_t = o.dx_t * (o.bn_act > 0)
    o.bn_act_exact = _bn_bound(o.g_act_t, o.bn_x, o.mean) < LIM
    return o


def _bn_bound(g, x, mean):
    """max over channels of sum |g| |x - mean| * 4 (and of sum |g|): below 2^24 every partial sum of the
    BatchNorm-backward reductions is an exactly representable multiple of 1/4."""
    d = (x - mean.view(1, -1, 1, 1)).abs()
    return max(float((g.abs() * d * 4).sum((0, 2, 3)).max()), float(g.abs().sum((0, 2, 3)).max()))


def bn_sums(g, x, mean):
    """float64 (sum g, sum g (x - mean)) per channel."""
    return torch.stack([g.sum((0, 2, 3)), (g * (x - mean.view(1, -1, 1, 1))).sum((0, 2, 3))])
