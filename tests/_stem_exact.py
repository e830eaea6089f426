"""Integer-exact operands and float64 references for the bitwise tests of the fused stem
(csrc/sqr_stem.hip: conv1 7x7/2 + bn1 + ReLU + max-pool 3/2/1; test_stem_exact_cpu.py,
test_stem_exact_gpu.py).  CPU only.

The method of _conv_exact.py (integer operands: every product and partial sum of conv1 is an integer
a float32 accumulator holds exactly, so only the final cast rounds) with one addition for the
BatchNorm in the middle.

Operand classes
  small (training mode, forward and backward): x in {0, 1, 2}, image n thinned by a keep probability of
    (n mod 3 + 1) / 3 (tile means differ: a mis-weighted merge of partial rows shows); w in {-1, 0, 1},
    half the entries zero; dy integer in [-4, 4].  max conv(|x|, |w|) <= 256 (bf16) / 2048 (fp16): every
    conv output is a value of T, and the f32 conv value the backward's closed form uses equals the
    rounded one.  Every backward sum (T1 = sum g A^T, the patch Gram matrix, column sums, sum g) stays
    below 2^24.
  round (eval mode, and the statistics alone): x in [0, 8], w in [-4, 4] (bf16) / [-32, 32] (fp16), drawn
    from the upper part of the ranges like _conv_exact.short_sums (|x| in 5 .. 8, |w| in 3 .. 4 / 24 .. 32,
    w with a random sign) so that the cast of conv1's output to T rounds a good share of the values;
    max conv(|x|, |w|) < 2^24 and, fp16, <= 65504 / 4.
  eval coefficients exact in f32: eps = 2^-10, running_var in {1/4, 1, 4} - 2^-10 (invstd = 2, 1, 1/2 in
    infer_coef_kernel's double arithmetic), gamma in {+-1/2, +-1, +-2} (a quarter negative), running_mean
    a multiple of 1/4 in [-4, 4], beta integer in [-4, 4]: v * scale + shift is an f32 value, so the
    kernel's fmaf and the float64 reference round the same number to T.

Training coefficients: the guard band.  Batch statistics make scale and shift inexact, but in the
small class conv1's output takes a few dozen distinct values per channel, so y before pooling depends
on (channel, value) alone.  The reference tabulates t = v * scale + shift in float64 from the exact
statistics; a pair is fragile when t lies within G * (|v * scale| + |shift|) of a rounding boundary of T
or of 0, G = 2^-18 (the kernel's scale and shift carry a few f32 roundings of 2^-24 plus the statistics
error, asserted below 2^-20 by the GPU test: a 4x margin).  gamma is drawn once per channel (U(0.5, 1.5),
a quarter negative); beta ~ N(0, 0.3) is redrawn until the channel has no fragile pair (at most 64
tries, else the case fails to build).  With no fragile pair the stored y and the argmax taps must
equal the reference bit for bit, nothing excluded.
"""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

LIM = float(1 << 24)
G = 2.0 ** -18
EPS_TRAIN = 1e-5
EPS_EVAL = 2.0 ** -10
MAX_TRIES = 64
CHUNK = 128  # images per step of the chunked patch sums

# id -> (N, H, W): the smallest geometries the kernels accept (Hc % 8 == 0, Wc % 32 == 0)
CASES = {
    "min": (1, 16, 64),      # one tile in every kernel; all four borders inside one window
    "oddh": (2, 15, 64),     # odd height: 3 padded rows below
    "oddh2": (1, 31, 128),   # odd height with a seam in x and in y
    "seams": (2, 48, 128),   # 3x2 stats tiles, 6x2 backward tiles, 3x2 pool tiles
    "wide": (1, 16, 256),    # four tiles across a row
    "many": (1100, 16, 64),  # stats 1100 tiles on 512 workgroups (3 and 2 each), pool 1100 on 768,
                             # backward 2200 on 512 (5 and 4 each)
}
ALL_IDS = list(CASES)
EVAL_IDS = ["min", "oddh", "seams", "many"]
STATS_IDS = ["seams", "many"]
ROUTE_IDS = ["min", "seams"]  # every (input dtype, activation dtype) pair; fused against unfused

# significand bits (hidden one included) and the exponent of the smallest normal binade
PREC = {torch.bfloat16: (8, -126), torch.float16: (11, -14)}
EXACT_INT = {torch.bfloat16: 256.0, torch.float16: 2048.0}
DT_NAME = {torch.bfloat16: "bf16", torch.float16: "f16"}


def geom(H, W):
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
    assert Hc % 8 == 0 and Wc % 32 == 0 and Hp % 4 == 0 and Wp % 16 == 0 and W % 4 == 0
    return Hc, Wc, Hp, Wp


def tiles(N, H, W):
    """(stats, pool, backward) tile counts of the three persistent kernels."""
    Hc, Wc, Hp, Wp = geom(H, W)
    return N * (Hc // 8) * (Wc // 32), N * (Hp // 4) * (Wp // 16), N * (Hc // 4) * (Wc // 32)


def _seed(cid, extra=0):
    s = extra
    for ch in cid:
        s = s * 131 + ord(ch)
    return s % (1 << 31)


def cast(t, dt):
    """The value a kernel stores: float64 -> dt, one round-to-nearest-even (as float64 again)."""
    return t.to(dt).double()


def boundary_distance(t, dt):
    """Distance of |t| (float64) to the nearest rounding boundary of dt: the midpoints between
    neighbouring values of dt, those of the binade below included (next to a power of two the
    boundary below is half as far as the one above)."""
    p, emin = PREC[dt]
    a = t.abs()
    _, e = torch.frexp(a)
    E = (e - 1).clamp_min(emin)  # |t|'s binade (the subnormals share the lowest one's spacing)
    one = torch.ones_like(a)
    u = torch.ldexp(one, E - (p - 1))
    q = a / u
    d = ((q - q.floor()) - 0.5).abs() * u
    low = torch.ldexp(one, E) - u / 4
    d_low = torch.where(E > emin, (a - low).abs(), torch.full_like(a, float("inf")))
    return torch.minimum(d, d_low)


def conv1(x, w):
    return torch.cat([F.conv2d(x[i:i + CHUNK], w, stride=2, padding=3) for i in range(0, x.shape[0], CHUNK)])


def patch_sums(x, mats):
    """[sum_p m[p][k] A[p][j] for m in mats] with A[p] the 7x7 input patch of conv pixel p (49 taps),
    m of shape (N, K, Hc, Wc); a few images at a time."""
    out = [torch.zeros(m.shape[1], 49, dtype=torch.float64) for m in mats]
    for i in range(0, x.shape[0], CHUNK):
        A = F.unfold(x[i:i + CHUNK], 7, padding=3, stride=2)  # (n, 49, Hc * Wc)
        for o, m in zip(out, mats):
            mm = m[i:i + CHUNK]
            o += torch.einsum("nkl,njl->kj", mm.reshape(mm.shape[0], mm.shape[1], -1), A)
    return out


def stats(cb):
    """(mean, biased variance, unbiased variance) per channel of (N, C, H, W) float64."""
    M = cb.numel() // cb.shape[1]
    mean = cb.sum((0, 2, 3)) / M
    m2 = ((cb - mean.view(1, -1, 1, 1)) ** 2).sum((0, 2, 3))
    return mean, m2 / M, m2 / (M - 1)


def taps_from_indices(idx, Wc):
    """max_pool2d's flat indices (N, C, Hp, Wp) -> the kernel's tap number 3 dh + dw inside each window
    (window (ph, pw) starts at conv pixel (2 ph - 1, 2 pw - 1))."""
    Hp, Wp = idx.shape[2], idx.shape[3]
    ph = torch.arange(Hp).view(1, 1, Hp, 1)
    pw = torch.arange(Wp).view(1, 1, 1, Wp)
    dh = idx // Wc - (2 * ph - 1)
    dw = idx % Wc - (2 * pw - 1)
    assert int(dh.min()) >= 0 and int(dh.max()) <= 2 and int(dw.min()) >= 0 and int(dw.max()) <= 2
    return (3 * dh + dw).to(torch.uint8)


def window_slices(r):
    """The nine taps of every 3/2/1 pooling window of r (N, C, Hc, Wc), padded with -inf: a list of
    (N, C, Hp, Wp) views in tap order."""
    Hc, Wc = r.shape[2], r.shape[3]
    Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
    rp = F.pad(r, (1, 1, 1, 1), value=float("-inf"))
    return [rp[:, :, dh:dh + 2 * Hp:2, dw:dw + 2 * Wp:2] for dh in range(3) for dw in range(3)]


def route(dy, y, idx, Hc, Wc):
    """g (N, C, Hc, Wc): the pooled gradient at its argmax pixel, masked by y > 0."""
    N, C = dy.shape[:2]
    g = torch.zeros(N, C, Hc * Wc, dtype=torch.float64)
    g.scatter_add_(2, idx.reshape(N, C, -1), (dy * (y > 0)).reshape(N, C, -1))
    return g.view(N, C, Hc, Wc)


# ------------------------------------------------------------------------------------ small class
@functools.lru_cache(maxsize=None)
def small_base(cid):
    """What the two activation dtypes of a small-class case share: operands, conv1 (run once), its
    statistics, gamma, the sums over patches that do not depend on beta.  Read-only."""
    N, H, W = CASES[cid]
    Hc, Wc, Hp, Wp = geom(H, W)
    g = torch.Generator().manual_seed(_seed(cid))
    b = SimpleNamespace(cid=cid, N=N, H=H, W=W, Hc=Hc, Wc=Wc, Hp=Hp, Wp=Wp, M=N * Hc * Wc)
    keep_p = ((torch.arange(N) % 3 + 1).double() / 3).view(N, 1, 1, 1)
    x = torch.randint(0, 3, (N, 1, H, W), generator=g).double()
    b.x = x * (torch.rand(N, 1, H, W, generator=g, dtype=torch.float64) < keep_p)
    sign = torch.randint(0, 2, (64, 1, 7, 7), generator=g).double() * 2 - 1
    b.w = sign * (torch.rand(64, 1, 7, 7, generator=g) < 0.5)
    b.dy = torch.randint(-4, 5, (N, 64, Hp, Wp), generator=g).double()
    b.c = conv1(b.x, b.w)
    b.y_bound = float(conv1(b.x, b.w.abs()).max())
    assert b.y_bound <= EXACT_INT[torch.bfloat16], ("conv1 outputs representable", cid, b.y_bound)
    b.mean, b.var, b.var_unb = stats(b.c)
    gam = torch.rand(64, generator=g) + 0.5
    gam = torch.where(torch.randperm(64, generator=g) < 16, -gam, gam)  # a quarter negative
    b.gamma = gam.float().double()  # the f32 values the kernel is handed
    ones = torch.ones(N, 1, Hc, Wc, dtype=torch.float64)
    b.T2, T3 = patch_sums(b.x, [b.c, ones])  # sum c A^T (64, 49), sum A (1, 49)
    b.T3 = T3[0]
    sq, = patch_sums(b.x * b.x, [ones])
    # the patch Gram matrix's largest entries are on its diagonal (x >= 0: Cauchy-Schwarz)
    b.gram_bound = float(sq.max())
    assert b.gram_bound < LIM and float(b.T3.max()) < LIM, ("Gram / column sums", cid)
    # the distinct conv values per channel: present[k][v - vmin]
    b.vmin, vmax = int(b.c.min()), int(b.c.max())
    R = vmax - b.vmin + 1
    code = torch.arange(64).view(1, 64, 1, 1) * R + (b.c.long() - b.vmin)
    b.present = (torch.bincount(code.reshape(-1), minlength=64 * R) > 0).view(64, R)
    b.values = torch.arange(b.vmin, vmax + 1).double()
    b.max_values = int(b.present.sum(1).max())
    return b


def fragile_pairs(b, dt, beta):
    """(64, R) bool: the (channel, value) pairs whose t = v * scale + shift is too close to a rounding
    boundary of dt or to 0 (module docstring)."""
    scale = b.gamma / torch.sqrt(b.var + EPS_TRAIN)
    shift = beta - b.mean * scale
    vs = b.values.view(1, -1) * scale.view(-1, 1)
    t = vs + shift.view(-1, 1)
    band = G * (vs.abs() + shift.abs().view(-1, 1))
    return b.present & ((boundary_distance(t, dt) <= band) | (t.abs() <= band))


@functools.lru_cache(maxsize=None)
def small(cid, dt):
    """One small-class case in one activation dtype: beta behind the guard band, the float64 forward
    (y, taps, statistics) and the closed-form backward with its error magnitudes.  Read-only."""
    b = small_base(cid)
    assert b.y_bound <= EXACT_INT[dt]
    o = SimpleNamespace(**vars(b))
    o.base, o.dt, o.eps = b, dt, EPS_TRAIN
    g = torch.Generator().manual_seed(_seed(cid, 1 + list(PREC).index(dt)))
    beta = torch.zeros(64, dtype=torch.float64)
    bad = torch.ones(64, dtype=torch.bool)
    o.tries = 0
    while bool(bad.any()):
        assert o.tries < MAX_TRIES, ("no beta clear of the guard band", cid, dt, int(bad.sum()))
        o.tries += 1
        draw = (torch.randn(64, generator=g) * 0.3).float().double()
        beta = torch.where(bad, draw, beta)
        bad = fragile_pairs(b, dt, beta).any(1)
    o.beta = beta
    o.fragile = int(fragile_pairs(b, dt, beta).sum())
    o.invstd = 1.0 / torch.sqrt(b.var + o.eps)
    o.scale = b.gamma * o.invstd
    o.shift = beta - b.mean * o.scale
    assert torch.equal(cast(b.c, dt), b.c)
    r = act(o)
    o.y, o.idx = F.max_pool2d(r, 3, 2, 1, return_indices=True)
    o.tap = taps_from_indices(o.idx, b.Wc)
    ws = window_slices(r)
    o.tie_share = float((sum((s == o.y).long() for s in ws) >= 2).double().mean())
    o.zero_share = float((o.y == 0).double().mean())
    assert o.tie_share >= 0.10, ("tied maxima", cid, dt, o.tie_share)
    assert o.zero_share >= 0.01, ("zero outputs", cid, dt, o.zero_share)
    closed_form(o, o.idx)
    return o


def act(o):
    """relu(bn(conv1)) rounded to T, (N, 64, Hc, Wc): what the pool sees (not kept: 144 MB on `many`)."""
    bc = lambda v: v.view(1, -1, 1, 1)
    return cast(torch.relu(o.base.c * bc(o.scale) + bc(o.shift)), o.dt)


def closed_form(o, idx, out=None):
    """The kernel's backward: g routed through idx, T1 = sum g A^T, sum g, sum g c, then dW = a T1 + k3 T2 +
    k2 T3 and dgamma / dbeta, with the magnitudes B_W, B_gamma the GPU tolerances are relative to.
    Results into `out` (default: o)."""
    out = o if out is None else out
    b = o.base
    g = route(b.dy, o.y, idx, b.Hc, b.Wc)
    T1, = patch_sums(b.x, [g])
    T1_bound = float(patch_sums(b.x, [g.abs()])[0].max())
    sg = g.sum((0, 2, 3))
    sgc = (g * b.c).sum((0, 2, 3))
    assert max(T1_bound, float(g.abs().sum((0, 2, 3)).max())) < LIM, ("backward partial sums", o.cid)
    assert float(g.abs().max()) <= EXACT_INT[o.dt]  # g is staged in T
    M = float(b.M)
    dgam = (sgc - b.mean * sg) * o.invstd
    a = b.gamma * o.invstd
    k3 = -a * o.invstd * dgam / M
    k2 = -a * sg / M - k3 * b.mean
    col = lambda v: v.view(-1, 1)
    out.dW = (col(a) * T1 + col(k3) * b.T2 + col(k2) * b.T3.view(1, -1)).view(64, 1, 7, 7)
    out.B_W = ((col(a) * T1).abs() + (col(k3) * b.T2).abs() + (col(k2) * b.T3.view(1, -1)).abs()).view(64, 1, 7, 7)
    out.dgamma, out.dbeta = dgam, sg
    out.B_gamma = (sgc.abs() + (b.mean * sg).abs()) * o.invstd
    return out


def autograd_grads(o):
    """(dW, dgamma, dbeta) by float64 autograd through conv1 -> cast -> BatchNorm (batch statistics) ->
    ReLU -> cast -> max-pool; both casts with straight-through gradients.  The BatchNorm is written out
    (two-pass mean and variance): F.batch_norm's CPU statistics of 281,600 values per channel are good to
    about 1e-13 only, which the gradients' cancellation lifts above the 1e-12 this is compared at."""
    b = o.base
    w = b.w.clone().requires_grad_(True)
    gamma = b.gamma.clone().requires_grad_(True)
    beta = o.beta.clone().requires_grad_(True)
    bc = lambda v: v.view(1, -1, 1, 1)
    c = conv1(b.x, w)
    c = c + (cast(c, o.dt) - c).detach()
    mean = c.mean((0, 2, 3), keepdim=True)
    var = ((c - mean) ** 2).mean((0, 2, 3), keepdim=True)
    r = F.relu((c - mean) / torch.sqrt(var + o.eps) * bc(gamma) + bc(beta))
    r = r + (cast(r, o.dt) - r).detach()
    y = F.max_pool2d(r, 3, 2, 1)
    assert torch.equal(y.detach(), o.y)
    y.backward(b.dy)
    return w.grad, gamma.grad, beta.grad


# ------------------------------------------------------------------------------------ round class
@functools.lru_cache(maxsize=None)
def rounded(cid, dt):
    """One round-class case: operands whose conv1 output rounds in the cast to dt, the statistics of the
    rounded values, the eval coefficients that are exact in f32 and the eval-mode output.  Read-only."""
    N, H, W = CASES[cid]
    Hc, Wc, Hp, Wp = geom(H, W)
    g = torch.Generator().manual_seed(_seed(cid, 11 + list(PREC).index(dt)))
    o = SimpleNamespace(cid=cid, dt=dt, N=N, H=H, W=W, Hc=Hc, Wc=Wc, Hp=Hp, Wp=Wp, M=N * Hc * Wc, eps=EPS_EVAL)
    wr = 32 if dt == torch.float16 else 4
    o.x = torch.randint(5, 9, (N, 1, H, W), generator=g).double()
    sign = torch.randint(0, 2, (64, 1, 7, 7), generator=g).double() * 2 - 1
    o.w = torch.randint((3 * wr) // 4, wr + 1, (64, 1, 7, 7), generator=g).double() * sign
    c = conv1(o.x, o.w)
    o.y_bound = float(conv1(o.x, o.w.abs()).max())
    assert o.y_bound < LIM and (dt != torch.float16 or o.y_bound <= 65504.0 / 4), ("conv1 sums", cid, dt, o.y_bound)
    o.cb = cast(c, dt)
    o.round_share = float((o.cb != c).double().mean())
    assert o.round_share >= 0.02, ("the cast rounds", cid, dt, o.round_share)
    o.mean, o.var, o.var_unb = stats(o.cb)
    o.invstd = 1.0 / torch.sqrt(o.var + o.eps)

    pick = lambda vals: torch.tensor(vals, dtype=torch.float64)[torch.randint(0, len(vals), (64,), generator=g)]
    o.running_var = pick([0.25, 1.0, 4.0]) - EPS_EVAL
    gam = pick([0.5, 1.0, 2.0])
    o.gamma = torch.where(torch.randperm(64, generator=g) < 16, -gam, gam)
    o.running_mean = torch.randint(-16, 17, (64,), generator=g).double() / 4
    o.beta = torch.randint(-4, 5, (64,), generator=g).double()
    for v in (o.running_var, o.gamma, o.running_mean, o.beta):
        assert torch.equal(v.float().double(), v)
    inv = 1.0 / torch.sqrt(o.running_var + EPS_EVAL)
    assert bool(((inv == 2.0) | (inv == 1.0) | (inv == 0.5)).all())
    o.scale_eval = o.gamma * inv
    o.shift_eval = o.beta - o.running_mean * o.scale_eval
    bc = lambda v: v.view(1, -1, 1, 1)
    t = o.cb * bc(o.scale_eval) + bc(o.shift_eval)
    assert torch.equal(t.float().double(), t) and float(t.abs().max()) < 65504.0, ("eval pre-activation exact", cid)
    r = cast(torch.relu(t), dt)
    o.round_share_eval = float((r != torch.relu(t)).double().mean())
    o.y_eval = F.max_pool2d(r, 3, 2, 1)
    return o
