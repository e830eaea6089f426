"""Float64 reference of the ResNetSQ regression tail, one function per stage of sqr_tail.hip, the
error measure of its tests, and the inputs those tests share.  No GPU and no libsqr here.

Stages (x is the layer-4 activation as [B, P, C0]; Wh / bh are the four heads' Linear layers stacked
in the order a(3) e(2) t(3) q(4)):

    feat = pool(x)                    pre0 = fc(W0, b0, feat)          pre1 = fc(W1, b1, leaky(pre0))
    z    = heads(Wh, bh, leaky(pre1)) a, e, t, q = activate(z)
    dz   = dz(z, G)                   d1 = d1(Wh, dz, pre1)            d0 = d0(W1, d1, pre0)
    dx   = dx(W0, d0, P)              dW, db = wgrad(d, act)           (act = feat, leaky(pre0), leaky(pre1))

Layouts of the C ABI: a `save` row is [feat C0][pre0 F1][pre1 F2][z 12] per sample, a `dsave` row
(the backward's workspace) is [d0 F1][d1 F2][dz 12].

Error measure (as in test_optim_kernels_gpu.py).  Per element |got - ref64| / (EPS32 * M + 2^-149),
EPS32 = 2^-23, M being what enters that element's roundings:
    dot product / sample sum   sum |terms| + |bias|
    pool                       sum_p |x| / P
    sigmoid, q                 |ref|
    sigmoid'                   |g| s (1 - s) + |g| s s    (1 - s cancels: its terms are 1 and s, times g s)
    quaternion dz              (|g| + |q| sum_k |q_k g_k|) / |z|     (g - q (q . g) cancels)
    16-bit dx                  EPS32 * M + half a unit in the last place of the output type at |ref|
Every *_mag function below returns M for the function it is named after.

A-priori ceiling.  An n-term float32 sum of products in any order, fused or not, errs at most
(n + 2) / 2 of these units (n products and n - 1 additions of half a unit each at most, first order,
plus the final operation on the sum: the bias, the division by P or the slope).  STAGE_TERMS gives n
per stage; the elementwise stages count their rounded operations, expf as four (2 ulp).

Yardstick.  YARD holds, per input set (CASES) and stage, the error of the same stage computed in
float32 with torch on the CPU (F.linear, mean, sigmoid, matrix products and elementwise operations,
one thread) in the units above.  A stage's inputs are the float64 reference of the stage before it
rounded to float32, and the inputs themselves are built from integers, so that every host measures
the same operands.  The quaternion's norm is formed by float32 elementwise operations (torch's norm()
accumulates in float64) and a bias gradient by one float32 addition per sample in sample order, the
order the kernel documents.  test_tail_ref_cpu.py re-measures every figure and holds it to a factor 2
of this table in both directions.  The figures are one host's (AVX-512, MKL): what remains
host-dependent is the order in which the BLAS adds a dot product and the vector sigmoid, and a
maximum over a few hundred heavy-tailed errors moves with them (another host measured 0.37 to 2.7
of single figures).  The table is not adjusted to that.  A kernel stage may err twice its figure:

%s
"""
import collections
import functools
import math

import torch

F64 = torch.float64
EPS32 = 2.0 ** -23
EPS64 = 2.0 ** -52
TINY = 2.0 ** -149
HEAD_N = (3, 2, 3, 4)
HEAD_OFF = (0, 3, 5, 8)
NOUT = 12
SLOPE = 0.01


# ------------------------------------------------------------------ stages, float64

def pool(x):
    """x [B, P, C0] -> feat [B, C0]"""
    return x.double().sum(1) / x.shape[1]


def pool_mag(x):
    return x.double().abs().sum(1) / x.shape[1]


def fc(W, b, v):
    return v.double() @ W.double().t() + b.double()


def fc_mag(W, b, v):
    return v.double().abs() @ W.double().abs().t() + b.double().abs()


def leaky(pre):
    pre = pre.double()
    return torch.where(pre > 0, pre, pre * SLOPE)


def heads(Wh, bh, h1):
    """Wh [12, F2], bh [12] -> z [B, 12]"""
    return fc(Wh, bh, h1)


def activate(z):
    z = z.double()
    s = torch.sigmoid(z[:, :8])
    return s[:, 0:3], s[:, 3:5], s[:, 5:8], z[:, 8:] / z[:, 8:].norm(dim=1, keepdim=True)


def upstream(G, B):
    """The four upstream gradients (None = a missing head = zero) as one float64 [B, 12]."""
    return torch.cat([torch.zeros(B, n, dtype=F64) if g is None else g.double() for g, n in zip(G, HEAD_N)], 1)


def dz(z, G):
    """G [B, 12] (see upstream()).  sigmoid' = s(z) s(-z): no cancellation in the reference."""
    z, G = z.double(), G.double()
    zs, zq, gq = z[:, :8], z[:, 8:], G[:, 8:]
    nrm = zq.norm(dim=1, keepdim=True)
    q = zq / nrm
    return torch.cat([G[:, :8] * torch.sigmoid(zs) * torch.sigmoid(-zs),
                      (gq - q * (q * gq).sum(1, keepdim=True)) / nrm], 1)


def dz_mag(z, G):
    z, G = z.double(), G.double()
    zs, zq, gq = z[:, :8], z[:, 8:], G[:, 8:].abs()
    s = torch.sigmoid(zs)
    nrm = zq.norm(dim=1, keepdim=True)
    q = (zq / nrm).abs()
    return torch.cat([G[:, :8].abs() * s * (torch.sigmoid(-zs) + s), (gq + q * (q * gq).sum(1, keepdim=True)) / nrm], 1)


def _slope(pre):
    pre = pre.double()
    return torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, SLOPE))


def d1(Wh, dz_, pre1):
    return (dz_.double() @ Wh.double()) * _slope(pre1)


def d1_mag(Wh, dz_, pre1):
    return (dz_.double().abs() @ Wh.double().abs()) * _slope(pre1)


def d0(W1, d1_, pre0):
    return (d1_.double() @ W1.double()) * _slope(pre0)


def d0_mag(W1, d1_, pre0):
    return (d1_.double().abs() @ W1.double().abs()) * _slope(pre0)


def dx(W0, d0_, P):
    """One pixel's row [B, C0]; every pixel of a sample gets the same."""
    return (d0_.double() @ W0.double()) / P


def dx_mag(W0, d0_, P):
    return (d0_.double().abs() @ W0.double().abs()) / P


def wgrad(d, act):
    d, act = d.double(), act.double()
    return d.t() @ act, d.sum(0)


def wgrad_mag(d, act):
    d, act = d.double().abs(), act.double().abs()
    return d.t() @ act, d.sum(0)


def split_save(save, C0, F1, F2):
    """save [B, C0 + F1 + F2 + 12] -> feat, pre0, pre1, z"""
    assert save.shape[1] == C0 + F1 + F2 + NOUT
    return save[:, :C0], save[:, C0:C0 + F1], save[:, C0 + F1:C0 + F1 + F2], save[:, C0 + F1 + F2:]


def split_dsave(dsave, F1, F2):
    """dsave [B, F1 + F2 + 12] -> d0, d1, dz"""
    assert dsave.shape[1] == F1 + F2 + NOUT
    return dsave[:, :F1], dsave[:, F1:F1 + F2], dsave[:, F1 + F2:]


# ------------------------------------------------------------------ the measure

def ulp_half(ref, dtype):
    """Half a unit in the last place of `dtype` at |ref| (float64 tensor); 0 for float32."""
    if dtype == torch.float32:
        return torch.zeros_like(ref)
    mant, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** emin)))
    return 0.5 * torch.exp2(e - mant)


def nerr(got, ref, mag, extra=None):
    """max over elements of |got - ref| / (EPS32 * mag + 2^-149 [+ extra]); NaN / inf in got is inf."""
    got = got.detach().double().cpu()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    den = EPS32 * mag + TINY
    if extra is not None:
        den = den + extra
    if got.numel() == 0:
        return 0.0
    return float(((got - ref).abs() / den).max())


# n of the ceiling (n + 2) / 2 per stage, from the case's shape
STAGE_TERMS = {
    "feat": lambda c: c.P,
    "pre0": lambda c: c.C0 + 1,
    "pre1": lambda c: c.F1 + 2,     # + leaky's product on the operand
    "z": lambda c: c.F2 + 2,
    "sig": lambda c: 6,             # expf (4), 1 + e, 1 / (.)
    "q": lambda c: 9,               # 4 squares, 3 additions, sqrt, division
    "qn": lambda c: 2 * 9 + 7,      # |q|^2 - 1 = twice q's relative error, formed from 4 such elements
    "dz": lambda c: 16,             # the norm (8), q_k (1), 4-term dot (4), q_i dot, the difference, / |z|
    "d1": lambda c: NOUT + 1,       # + the slope
    "d0": lambda c: c.F2 + 4,       # + the three additions of the wave partials, the slope
    "dx": lambda c: c.F1 + 4,       # + the partials, / P
    "dw0": lambda c: c.B, "db0": lambda c: c.B,
    "dw1": lambda c: c.B + 1, "db1": lambda c: c.B,   # + leaky's product on the activation
    "dwh": lambda c: c.B + 1, "dbh": lambda c: c.B,
}
FWD_STAGES = ("feat", "pre0", "pre1", "z", "sig", "q", "qn")
BWD_STAGES = ("dz", "d1", "d0", "dx", "dw0", "db0", "dw1", "db1", "dwh", "dbh")
STAGES = FWD_STAGES + BWD_STAGES


def ceiling(stage, case):
    return (STAGE_TERMS[stage](case) + 2) / 2.0


# ------------------------------------------------------------------ cases and inputs (CPU, deterministic)

Case = collections.namedtuple("Case", "name B P C0 F1 F2 dtype entry up")
f32, bf16, f16 = torch.float32, torch.bfloat16, torch.float16
DT_CODE = {f32: 0, bf16: 1, f16: 2}
# up: how the upstream gradients arrive.  sep: four tensors with ld == n; cat: columns of one [B, 12];
# ld7: head 0 in a [B, 7] tensor; nullH: head H has no gradient; allnull: none has.
# The forward takes tail_fwd_kernel (one launch) unless F1 % 16 == 0 and F2 % 16 == 0 (three launches).
# pool: V = C0 / 8 vectors, phases = 2048 / C0 pixel phases.  wgrad: samples in chunks of 64.
CASES = [
    # one launch
    Case("s4x4", 65, 1, 8, 4, 4, f32, "packed", "cat"),            # 1 row per wave; one pixel, 256 phases
    Case("s20x12", 65, 3, 64, 20, 12, f32, "sep", "sep"),          # 5 / 3 rows per wave; 3 pixels < 32 phases; full + partial chunk
    Case("s68x36", 63, 3, 512, 68, 36, bf16, "packed", "cat"),     # 17 rows per wave (16 + 1); 3 pixels < 4 phases; partial chunk
    Case("s68x36s", 1, 49, 512, 68, 36, f32, "sep", "null2"),      # B = 1; 49 pixels over 4 phases
    Case("s1020x4", 64, 4, 512, 1020, 4, f16, "packed", "null1"),  # 255 rows per wave; pixels == phases
    Case("s12x1020", 2, 64, 1024, 12, 1020, f32, "sep", "ld7"),    # 3 / 255 rows per wave; 2 phases, V = 128; B = 2
    Case("s272x20", 64, 4, 64, 272, 20, f32, "packed", "cat"),     # F1 % 16 == 0 alone: still one launch; one full chunk
    Case("s20x12h", 64, 3, 8, 20, 12, f16, "sep", "cat"),          # f16 with V = 1
    Case("s68x36w", 63, 3, 1024, 68, 36, bf16, "sep", "ld7"),      # 3 pixels over 2 phases: one phase ends early
    Case("s4x4c", 130, 4, 8, 4, 4, f32, "packed", "sep"),          # two full chunks + partial at the smallest sections
    # three launches
    Case("t16x16", 65, 257, 8, 16, 16, f32, "packed", "sep"),      # 1 row per wave of a quarter; 257 pixels over 256 phases
    Case("t16x48", 63, 3, 64, 16, 48, bf16, "sep", "cat"),         # 1 / 3 rows per wave; one partial chunk of 63
    Case("t272x64", 128, 4, 512, 272, 64, f32, "packed", "cat"),   # 17 / 4 rows per wave; two full chunks
    Case("t64x272", 130, 1, 1024, 64, 272, f16, "packed", "null3"),  # two full chunks + partial; one pixel, 2 phases
    Case("t1024x16", 64, 49, 64, 1024, 16, f32, "sep", "null0"),   # 64 rows per wave: four full batches; 49 pixels over 32 phases
    Case("t16x1024", 64, 64, 8, 16, 1024, f32, "packed", "null2"),  # 64 rows per wave in fc1; 4 column passes in wgrad
    Case("t272x16", 65, 4, 8, 272, 16, bf16, "packed", "allnull"),  # (272, 16) takes three launches; no gradient at all
    Case("t16x48h", 64, 257, 64, 16, 48, f16, "sep", "sep"),       # 257 pixels over 32 phases (the largest x: 1.05 M)
    Case("t64x272b", 1, 1, 512, 64, 272, f32, "sep", "null1"),     # B = 1, one pixel
    Case("t1024x16w", 64, 4, 1024, 1024, 16, bf16, "packed", "cat"),  # bf16 at V = 128
]
CASE = {c.name: c for c in CASES}

PRE_SPECIAL = (0.0, -0.0, TINY, -TINY, 1e-30, -1e-30, 1e4, -1e4)   # pre-activations of the crafted save
SIG_SPECIAL = (0.0, 20.0, -20.0, 90.0, -90.0)                        # sigmoid logits of the crafted save
SATURATED = 88.0   # |z| above this: s (1 - s) is below float32's normal range, the kernel must give exactly 0
Q_EXP = (-30, 30, 0, -17, 11)                                        # log2 of the quaternion logits' norm, by sample


def _sprinkle(t, special):
    """every 3rd element of t (flat) <- the special values in turn"""
    flat = t.view(-1)
    idx = torch.arange(0, flat.numel(), 3)
    flat[idx] = torch.tensor(special, dtype=t.dtype)[(idx // 3) % len(special)]
    return t


@functools.lru_cache(maxsize=None)
def make_inputs(name):
    """Everything a case needs, float32 tensors on the CPU (x already rounded to the case's dtype):
    x [B, P, C0], the parameters, the upstream gradients G (list of 4, None where missing), and the
    crafted save [B, C0 + F1 + F2 + 12] for the backward."""
    c = CASE[name]
    g = torch.Generator().manual_seed(1000 + [k.name for k in CASES].index(name))

    def rn(*shape):
        """about N(0, 1), the same bits on every host: three uniform 15-bit integers and 24 more bits below
        them, summed exactly in float64 and rounded once (torch.randn's values depend on the host's
        vector instructions)"""
        hi = torch.randint(-2 ** 14, 2 ** 14, (3,) + shape, generator=g).sum(0).double()
        lo = torch.randint(0, 2 ** 24, shape, generator=g).double() / 2 ** 24
        return ((hi + lo) / 2 ** 14).float()

    x = rn(c.B, c.P, c.C0).to(c.dtype).float()
    p = dict(W0=rn(c.F1, c.C0) / math.sqrt(c.C0), b0=0.1 * rn(c.F1), W1=rn(c.F2, c.F1) / math.sqrt(c.F1) * 3,
             b1=0.1 * rn(c.F2), Wh=rn(NOUT, c.F2) / math.sqrt(c.F2) * 3, bh=0.1 * rn(NOUT))
    # crafted save: ordinary values with the edges sprinkled in
    feat = rn(c.B, c.C0)
    pre0 = _sprinkle(rn(c.B, c.F1), PRE_SPECIAL)
    pre1 = _sprinkle(rn(c.B, c.F2), PRE_SPECIAL)
    z = rn(c.B, NOUT)
    z[:, :8] = _sprinkle(z[:, :8].contiguous(), SIG_SPECIAL)
    scale = torch.tensor([2.0 ** Q_EXP[n % len(Q_EXP)] for n in range(c.B)])
    zq = z[:, 8:].double()
    z[:, 8:] = (zq / zq.norm(dim=1, keepdim=True) * scale[:, None].double()).float()
    G = [rn(c.B, n) for n in HEAD_N]
    G[3] = G[3] * scale[:, None]          # dz of the quaternion stays O(1) at every norm
    if c.up.startswith("null"):
        G[int(c.up[4])] = None
    elif c.up == "allnull":
        G = [None] * 4
    save = torch.cat([feat, pre0, pre1, z], 1).contiguous()
    return dict(x=x, G=G, save=save, **p)


# ------------------------------------------------------------------ the yardstick: torch CPU float32

def sig_figs(z_in, a, e, t, q):
    """sig / q / qn figures of activated outputs against float64 from the logits z_in they were made of."""
    ar, er, tr, qr = activate(z_in)
    s_ref = torch.cat([ar, er, tr], 1)
    qd = q.detach().double().cpu()
    return {"sig": nerr(torch.cat([a, e, t], 1), s_ref, s_ref.abs()), "q": nerr(q, qr, qr.abs()),
            "qn": float(((qd * qd).sum(1) - 1).abs().max()) / EPS32 if bool(torch.isfinite(qd).all()) else math.inf}


def bwd_mask(z):
    """[B, 12] bool: dz elements inside the measure (saturated sigmoid logits are checked exactly)."""
    m = torch.ones(z.shape, dtype=torch.bool)
    m[:, :8] = z[:, :8].abs() < SATURATED
    return m


def dz_fig(z, Gc, dz_got):
    m = bwd_mask(z)
    ref, mag = dz(z, Gc), dz_mag(z, Gc)
    return nerr(dz_got.detach().double().cpu()[m], ref[m], mag[m])


def _norm32(v):
    """|v| per row from float32 elementwise operations (torch's norm() accumulates in float64)"""
    return (v * v).sum(1, keepdim=True).sqrt()


def _sum32(d):
    """sum over samples, one float32 addition per sample in sample order (torch's sum() adds pairwise)"""
    acc = torch.zeros_like(d[0])
    for n in range(d.shape[0]):
        acc = acc + d[n]
    return acc


def torch_cpu_figures(name):
    """The yardstick: each stage in float32 with torch on the CPU, against the float64 stage function on
    the same float32 inputs.  A stage's inputs are the float64 reference of the stage before it, rounded
    to float32 (the same on every host), not torch's own float32 result of that stage.  The quaternion's
    norm is formed from float32 elementwise operations and a bias gradient by one float32 addition per
    sample in sample order, as the kernels do.  One thread: torch blocks a long dot product by the
    number of threads, which moves a figure by up to a factor 2.  One figure per stage."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _torch_cpu_figures(name)
    finally:
        torch.set_num_threads(threads)


def _torch_cpu_figures(name):
    import torch.nn.functional as F
    c = CASE[name]
    i = make_inputs(name)
    out = {}
    lk = lambda v: F.leaky_relu(v, SLOPE)
    r32 = lambda v: v.float()
    # forward
    out["feat"] = nerr(i["x"].mean(1), pool(i["x"]), pool_mag(i["x"]))
    feat = r32(pool(i["x"]))
    out["pre0"] = nerr(F.linear(feat, i["W0"], i["b0"]), fc(i["W0"], i["b0"], feat), fc_mag(i["W0"], i["b0"], feat))
    pre0 = r32(fc(i["W0"], i["b0"], feat))
    out["pre1"] = nerr(F.linear(lk(pre0), i["W1"], i["b1"]), fc(i["W1"], i["b1"], leaky(pre0)),
                       fc_mag(i["W1"], i["b1"], leaky(pre0)))
    pre1 = r32(fc(i["W1"], i["b1"], leaky(pre0)))
    out["z"] = nerr(F.linear(lk(pre1), i["Wh"], i["bh"]), heads(i["Wh"], i["bh"], leaky(pre1)),
                    fc_mag(i["Wh"], i["bh"], leaky(pre1)))
    z = r32(heads(i["Wh"], i["bh"], leaky(pre1)))
    s = torch.sigmoid(z[:, :8])
    q = z[:, 8:] / _norm32(z[:, 8:])
    out.update(sig_figs(z, s[:, 0:3], s[:, 3:5], s[:, 5:8], q))
    # backward on the crafted save
    feat, pre0, pre1, z = split_save(i["save"], c.C0, c.F1, c.F2)
    Gc = upstream(i["G"], c.B)
    G32 = Gc.float()
    s = torch.sigmoid(z[:, :8])
    nrm = _norm32(z[:, 8:])
    q = z[:, 8:] / nrm
    dz32 = torch.cat([G32[:, :8] * (1 - s) * s, (G32[:, 8:] - q * (q * G32[:, 8:]).sum(1, keepdim=True)) / nrm], 1)
    out["dz"] = dz_fig(z, Gc, dz32)
    dz_in = r32(torch.where(bwd_mask(z), dz(z, Gc), torch.zeros(1, dtype=F64)))
    sl = lambda pre, v: torch.where(pre > 0, v, v * SLOPE)
    out["d1"] = nerr(sl(pre1, dz_in @ i["Wh"]), d1(i["Wh"], dz_in, pre1), d1_mag(i["Wh"], dz_in, pre1))
    d1_in = r32(d1(i["Wh"], dz_in, pre1))
    out["d0"] = nerr(sl(pre0, d1_in @ i["W1"]), d0(i["W1"], d1_in, pre0), d0_mag(i["W1"], d1_in, pre0))
    d0_in = r32(d0(i["W1"], d1_in, pre0))
    ref = dx(i["W0"], d0_in, c.P)
    out["dx"] = nerr(((d0_in @ i["W0"]) / c.P).to(c.dtype), ref, dx_mag(i["W0"], d0_in, c.P), ulp_half(ref, c.dtype))
    for key, d, act in (("0", d0_in, feat), ("1", d1_in, lk(pre0)), ("h", dz_in, lk(pre1))):
        act64 = act.double() if key == "0" else leaky(pre0 if key == "1" else pre1)
        (rw, rb), (mw, mb) = wgrad(d, act64), wgrad_mag(d, act64)
        out["dw" + key] = nerr(d.t() @ act, rw, mw)
        out["db" + key] = nerr(_sum32(d), rb, mb)
    return out


def _y(*figs):
    assert len(figs) == len(STAGES)
    return dict(zip(STAGES, figs))


# torch on the CPU, float32, per input set and stage in the order of STAGES (forward stages on the
# first line, backward stages on the second), in the units above; a kernel stage may err twice as much
YARD = {
    "s4x4": _y(0.000, 0.840, 0.969, 1.299, 0.949, 0.981, 1.709,
        1.700, 1.030, 1.196, 0.964, 0.859, 0.392, 0.759, 0.479, 1.338, 0.893),
    "s20x12": _y(1.071, 1.419, 1.443, 1.221, 0.893, 0.889, 1.312,
        1.968, 0.962, 1.595, 1.922, 1.897, 0.730, 1.391, 0.515, 1.221, 0.481),
    "s68x36": _y(0.333, 1.152, 2.088, 1.462, 0.902, 0.934, 1.596,
        2.503, 0.938, 1.746, 1.000, 3.360, 1.211, 3.538, 0.304, 1.190, 0.259),
    "s68x36s": _y(0.658, 0.183, 0.461, 0.354, 0.672, 0.106, 0.028,
        0.523, 0.473, 0.693, 0.973, 0.497, 0.000, 0.951, 0.000, 0.824, 0.000),
    "s1020x4": _y(0.450, 1.321, 0.465, 1.107, 0.887, 1.216, 2.131,
        1.573, 0.790, 1.855, 0.997, 3.590, 1.640, 2.908, 0.231, 1.493, 0.345),
    "s12x1020": _y(0.512, 0.142, 1.552, 0.128, 0.491, 0.445, 0.405,
        1.970, 0.960, 0.471, 1.207, 0.841, 0.369, 0.979, 0.497, 1.103, 0.323),
    "s272x20": _y(1.016, 1.669, 2.030, 1.323, 0.958, 0.976, 1.347,
        1.951, 1.248, 2.708, 2.033, 2.881, 1.411, 3.884, 0.586, 1.315, 0.330),
    "s20x12h": _y(0.328, 1.311, 2.946, 1.413, 0.897, 0.942, 1.531,
        1.678, 1.095, 1.828, 0.998, 1.235, 0.743, 2.269, 1.334, 1.229, 0.451),
    "s68x36w": _y(0.678, 0.782, 1.911, 1.721, 0.764, 1.227, 1.750,
        2.515, 1.046, 1.982, 1.000, 3.545, 1.407, 3.855, 1.109, 1.653, 0.465),
    "s4x4c": _y(0.824, 0.816, 1.227, 1.234, 0.962, 0.972, 1.332,
        1.820, 1.008, 1.066, 1.154, 1.250, 0.394, 1.198, 0.371, 1.178, 0.256),
    "t16x16": _y(0.240, 0.733, 1.231, 1.754, 0.895, 0.867, 1.414,
        1.730, 1.146, 1.947, 1.900, 1.642, 0.481, 1.783, 0.858, 1.688, 0.621),
    "t16x48": _y(0.333, 1.100, 1.944, 1.692, 0.822, 0.809, 1.529,
        1.609, 0.960, 1.723, 0.999, 3.032, 0.836, 1.752, 0.753, 3.269, 0.178),
    "t272x64": _y(1.171, 1.117, 3.130, 2.475, 0.958, 0.866, 1.587,
        1.623, 1.333, 2.511, 3.078, 3.949, 1.085, 3.348, 1.106, 1.554, 0.382),
    "t64x272": _y(0.000, 0.674, 2.731, 2.148, 0.803, 1.099, 2.032,
        0.908, 1.663, 2.792, 1.000, 3.402, 1.166, 4.412, 1.636, 2.733, 0.626),
    "t1024x16": _y(0.652, 1.956, 0.730, 1.601, 0.903, 0.886, 1.380,
        1.719, 0.974, 2.678, 0.992, 3.058, 1.042, 3.254, 0.593, 1.385, 0.209),
    "t16x1024": _y(0.444, 1.107, 2.315, 0.936, 0.963, 0.980, 1.608,
        1.451, 1.318, 0.899, 2.100, 1.469, 0.259, 3.272, 1.753, 2.175, 0.158),
    "t272x16": _y(0.000, 1.295, 1.335, 1.224, 0.860, 1.046, 1.284,
        0.000, 0.000, 0.000, 0.000, 0.000, 0.000, 0.000, 0.000, 0.000, 0.000),
    "t16x48h": _y(0.237, 1.214, 2.300, 1.814, 0.860, 0.906, 1.279,
        1.622, 1.412, 1.549, 0.999, 1.949, 0.562, 1.558, 0.686, 2.445, 0.367),
    "t64x272b": _y(0.000, 0.210, 1.106, 0.196, 0.664, 0.158, 0.019,
        0.257, 1.446, 0.759, 0.928, 0.499, 0.000, 0.946, 0.000, 1.000, 0.000),
    "t1024x16w": _y(0.106, 1.000, 0.819, 1.280, 0.891, 0.863, 1.507,
        1.318, 0.974, 2.468, 1.000, 4.821, 1.876, 3.428, 1.128, 1.177, 0.508),
}


def yard_table():
    """YARD as the text table of this module's docstring."""
    lines = ["    %-10s" % "input set" + "".join("%7s" % s for s in STAGES)]
    for c in CASES:
        if c.name in YARD:
            lines.append("    %-10s" % c.name + "".join("%7.3f" % YARD[c.name][s] for s in STAGES))
    return "\n".join(lines)


__doc__ = __doc__ % yard_table()
