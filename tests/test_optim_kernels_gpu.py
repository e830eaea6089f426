"""sqr_optim.hip (adam_kernel, crsk_kernel, amp_check_kernel, amp_update_kernel) against float64.

Reference.  One Adam step in float64 on the CPU, torch.optim.Adam's documented single-tensor formula:
g' = g * grad_scale [* 1 / loss_scale];  m = m + (1 - b1)(g' - m);  v = b2 v + (1 - b2) g'^2;
p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps),  t = step + 1.  Every step is checked on
its own: the reference starts from the fp32 state the implementation under test held before the step,
so the figures below are errors of ONE step, not of a trajectory.

Error measure.  Each element's |fp32 result - float64 reference| divided by
    EPS32 * magnitude + 2^-149,     EPS32 = 2^-23,
the magnitude being what enters that element's roundings:
    m   exp_avg      max(|m_old|, |g'|)
    v   exp_avg_sq   max(|v_old|, g'^2)
    p   parameter    |p_old| + |delta p|
    pc  parameter    |p_old| + |delta p| + step_size * max(|m_old|, |g'|) / denominator
2^-149 is fp32's smallest subnormal: gradients of 1e-20 square to subnormals, whose spacing no longer
follows EPS32.  `p` has a heavy tail: where m_old and g' nearly cancel, exp_avg's own rounding
(EPS32 * max(|m_old|, |g'|), correct to half a unit) is many EPS32 of the small m and so of delta p, and
among 10^6 weights some have |p| < |delta p|.  `pc` adds that carried rounding to the magnitude and
stays near 1 at every size, so it is the figure that binds on the large conv weights.

Bound.  torch.optim.Adam(foreach=False) in fp32 on the CPU, run on the very same inputs, measured
against the float64 reference with the measure above (`_torch_cpu_errors()`, no GPU involved), gives
per input set at most (TORCH_ERR below; test_torch_cpu_adam_is_the_yardstick re-measures it):

    input set       m      v      p       pc
    plain         0.575  1.063   2.521  1.194   sizes x alignments x hyper-parameters x states x grad scales
    many          0.488  1.052   1.978  0.615   100 parameters
    k64c1r7s2     0.428  0.734   1.247  0.484
    k64c3r7s2     0.475  0.857   2.166  0.645
    k64c64r3s1    0.486  0.896   5.005  0.912
    k128c64r3s2   0.493  1.071   3.805  0.684
    k128c64r1s2   0.443  0.901   1.820  0.478
    k64c64r5s2    0.483  0.964   5.243  0.585
    k64c640r3s1   0.495  1.046   8.538  0.927
    k32c32r3s1    0.498  0.887   1.230  0.471
    c1856         0.497  1.090  25.482  0.982   (64, 1856, 3, 3): 1.07 M weights
    c2048         0.491  1.020  18.985  0.965   (64, 2048, 3, 3): 1.18 M weights
    skip          0.496  1.030   3.184  0.546   loss scale 2^10, then 2^9
    blocks        0.495  1.043   7.223  0.875   30 x (conv 64 64 3 3, BatchNorm)

(One CPU's figures: torch's vectorised kernels contract a * b + c differently from one instruction set
to the next, and another host measured up to 12 % more in the two parameter columns.  The table is
not adjusted to that; the yardstick test holds torch itself to the same factor of two.)

The HIP kernel restates the same fp32 operation sequence with the same float64 bias corrections and
is allowed twice the figure of its input set in every column, the factor covering fma-free ordering
differences: e.g. plain 1.150 / 2.126 / 5.042 / 2.388.

Beyond the bound: on a fresh state the first step's moments are single IEEE products,
m = fl(fl32(1 - b1) g) and v = fl(fl(fl32(1 - b2) g) g), so they are compared bit for bit with those
products evaluated in fp32 on the CPU (one rounding each: nothing to tolerate).

Packed weights are compared bit for bit with a torch restatement of both layouts (krsc and the
stride-parity classes of crsk) cast by torch (round to nearest even), and with sqr.conv.pack_weight.
Every parameter, moment and gradient lives inside a buffer of guard words that must come back
untouched; packed buffers are pre-filled with the 16-bit pattern 0x7FFF so that unwritten elements
show.
"""
import math
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

EPS32 = 2.0 ** -23
TINY = 2.0 ** -149
# torch.optim.Adam(foreach=False), fp32, CPU, against the float64 reference on this module's inputs
KEYS = ("m", "v", "p", "pc")   # exp_avg, exp_avg_sq, parameter, parameter with exp_avg's rounding carried
TORCH_ERR = {   # per input set, in the order of KEYS; a kernel step may err twice as much
    "plain": (0.575, 1.063, 2.521, 1.194),
    "many": (0.488, 1.052, 1.978, 0.615),
    "k64c1r7s2": (0.428, 0.734, 1.247, 0.484),
    "k64c3r7s2": (0.475, 0.857, 2.166, 0.645),
    "k64c64r3s1": (0.486, 0.896, 5.005, 0.912),
    "k128c64r3s2": (0.493, 1.071, 3.805, 0.684),
    "k128c64r1s2": (0.443, 0.901, 1.820, 0.478),
    "k64c64r5s2": (0.483, 0.964, 5.243, 0.585),
    "k64c640r3s1": (0.495, 1.046, 8.538, 0.927),
    "k32c32r3s1": (0.498, 0.887, 1.230, 0.471),
    "c1856": (0.497, 1.090, 25.482, 0.982),
    "c2048": (0.491, 1.020, 18.985, 0.965),
    "skip": (0.496, 1.030, 3.184, 0.546),
    "blocks": (0.495, 1.043, 7.223, 0.875),
}

GUARD = 4               # guard words on each side: a 16-B aligned view stays 16-B aligned
PATTERN = 0x4B1DFACE    # guard bit pattern (a finite float, 10353358.0)
POISON = 0x7FFF         # packed buffers before the step (a NaN in bf16 and in fp16)

SIZES = [1, 3, 4, 5, 1023, 1024, 2047, 2048, 2049, 2051, 4103]
HYPER = {"default": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8),
         "alt": dict(lr=1e-4, betas=(0.8, 0.99), eps=1e-6)}
ALIGN = {"aligned": (0, 0), "p+1": (1, 0), "g+1": (0, 1)}   # floats (parameter, gradient) start into their buffer
GSCALE = {"gs1": 1.0, "gs0.5": 0.5, "gs1/3": 1.0 / 3.0}
SPECIAL = (0.0, 1e-20, -1e-20, 1e-3, -1e-3, 1e4, -1e4)   # every 5th gradient element, fixed over the steps
STEPS = 3

# (K, C, R, S), stride, pad
CONVS = {
    "k64c1r7s2": ((64, 1, 7, 7), 2, 3),       # C < 8: row padded to 64, scalar row path
    "k64c3r7s2": ((64, 3, 7, 7), 2, 3),       # row of 147 padded to 256
    "k64c64r3s1": ((64, 64, 3, 3), 1, 1),     # register-row path, 16-B stores, one parity class
    "k128c64r3s2": ((128, 64, 3, 3), 2, 1),   # four parity classes
    "k128c64r1s2": ((128, 64, 1, 1), 2, 0),   # one tap, three empty classes
    "k64c64r5s2": ((64, 64, 5, 5), 2, 2),     # classes of unequal size
    "k64c640r3s1": ((64, 640, 3, 3), 1, 1),   # row of 5760 floats: the loop path above 5120
    "k32c32r3s1": ((32, 32, 3, 3), 1, 1),     # GenericNetSQ's width: the step does not pack it
}
# rows above the 64 KiB LDS row (16384 floats), which the step leaves to pack_all.  The conv kernels take
# power-of-two channel counts only, so a forward can follow the step at 2048 channels, not at 1856.
BIG = {
    "c1856": ((64, 1856, 3, 3), 1, 1),        # row of 16704 floats
    "c2048": ((64, 2048, 3, 3), 1, 1),        # row of 18432 floats
}
SKIP_PLAIN = [2051, 1023]
SKIP_CONVS = ["k64c64r3s1", "k64c640r3s1", "k64c3r7s2"]
NBLOCKS = 30


# ------------------------------------------------------------------ inputs (CPU, deterministic)

def _numel(shape):
    return int(math.prod(shape))


def make_inputs(shapes, seed, resumed=False, steps=STEPS):
    """Per parameter: start value, start moments, one gradient per step.  Conv weights get He-sized
    values.  Every 5th element carries one of SPECIAL as its gradient; in a plain parameter it is
    also tiny (x 1e-9), so that the parameter check sees the updates much smaller than 1 that zero,
    1e-20 and 1e-3 gradients give."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for shape in shapes:
        shape = tuple(shape) if not isinstance(shape, int) else (shape,)
        n = _numel(shape)
        p = torch.randn(n, generator=gen)
        idx = torch.arange(0, n, 5)
        if len(shape) == 4:
            p *= math.sqrt(2.0 / (shape[1] * shape[2] * shape[3]))
        else:
            p[idx] *= 1e-9
        sp = torch.tensor(SPECIAL, dtype=torch.float32)[(idx // 5) % len(SPECIAL)]
        gs = []
        for _ in range(steps):
            g = torch.randn(n, generator=gen)
            g[idx] = sp
            gs.append(g)
        if resumed:
            m = 0.1 * torch.randn(n, generator=gen)
            v = (0.1 * torch.randn(n, generator=gen)).square()
        else:
            m, v = torch.zeros(n), torch.zeros(n)
        out.append(dict(shape=shape, p=p, m=m, v=v, g=gs))
    return out


def ref_adam(p, m, v, g, t, lr, betas, eps):
    """One step in float64 (tensors), t = step + 1."""
    b1, b2 = betas
    m = m + (1.0 - b1) * (g - m)
    v = b2 * v + (1.0 - b2) * g * g
    p = p - lr / (1.0 - b1 ** t) * m / (v.sqrt() / math.sqrt(1.0 - b2 ** t) + eps)
    return p, m, v


def _nerr(x32, ref64, mag):
    return ((x32.double() - ref64).abs() / (EPS32 * mag + TINY)).max().item()


# ------------------------------------------------------------------ guarded storage

def _guarded(n, off, device):
    ib = torch.full((GUARD + off + n + GUARD,), PATTERN, dtype=torch.int32, device=device)
    view = ib.view(torch.float32)[GUARD + off:GUARD + off + n]
    assert view.data_ptr() % 16 == (4 * off) % 16
    return ib, view


class Slot:
    """One parameter: value, gradient and both moments each inside their own guarded buffer."""

    def __init__(self, inp, device, p_off, g_off):
        self.inp = inp
        n = inp["p"].numel()
        self.n, self.shape = n, inp["shape"]
        self.bufs = {}
        for name, off in (("p", p_off), ("g", g_off), ("m", 0), ("v", 0)):
            self.bufs[name] = _guarded(n, off, device) + (off,)
        self.view("p").copy_(inp["p"])
        self.param = torch.nn.Parameter(self.view("p").view(self.shape))

    def view(self, name):
        return self.bufs[name][1]

    def guards_intact(self):
        for name, (ib, _, off) in self.bufs.items():
            lo = GUARD + off
            if not (bool((ib[:lo] == PATTERN).all()) and bool((ib[lo + self.n:] == PATTERN).all())):
                return False, name
        return True, None


class Rig:
    """A set of guarded parameters driven through an optimizer one checked step at a time."""

    def __init__(self, inputs, device=DEV, offs=(0, 0)):
        self.slots = [Slot(inp, device, *offs) for inp in inputs]
        self.params = [s.param for s in self.slots]
        self.opt = None

    def bind(self, model):
        """Make the guarded parameters the parameters of `model` (same order as model.parameters())."""
        it = iter(self.params)
        for mod in model.modules():
            for name, q in list(mod._parameters.items()):
                if q is not None:
                    new = next(it)
                    assert new.shape == q.shape
                    mod._parameters[name] = new
        assert next(it, None) is None
        return model

    def install(self, opt, step0=0):
        """Start state: fresh, or loaded through load_state_dict at step `step0`; the moments then move
        into guarded buffers."""
        self.opt = opt
        dev = self.params[0].device
        if step0:
            sd = opt.state_dict()
            sd["state"] = {i: {"step": torch.tensor(float(step0)), "exp_avg": s.inp["m"].view(s.shape).clone(),
                               "exp_avg_sq": s.inp["v"].view(s.shape).clone()}
                           for i, s in enumerate(self.slots)}
            opt.load_state_dict(sd)
        for s in self.slots:
            st = opt.state[s.param]
            if len(st) == 0:
                on_dev = opt.defaults.get("capturable")
                st["step"] = torch.zeros((), dtype=torch.float32, device=dev if on_dev else "cpu")
                st["exp_avg"] = torch.zeros_like(s.param)
                st["exp_avg_sq"] = torch.zeros_like(s.param)
            assert float(st["step"]) == float(step0)
            for key, name in (("exp_avg", "m"), ("exp_avg_sq", "v")):
                s.view(name).copy_(st[key].flatten())
                st[key] = s.view(name).view(s.shape)
        return self

    def set_grads(self, it, premultiply=None):
        for s in self.slots:
            g = s.inp["g"][it]
            s.view("g").copy_(g if premultiply is None else g * premultiply)
            s.param.grad = s.view("g").view(s.shape)

    def state_cpu(self):
        out = []
        for s in self.slots:
            st = self.opt.state[s.param]
            out.append(tuple(x.detach().flatten().to("cpu", copy=True)
                             for x in (s.param, st["exp_avg"], st["exp_avg_sq"])) + (float(st["step"]),))
        return out

    def bits(self):
        """Every guarded buffer whole (guards included) and every step counter, for bitwise comparison."""
        out = []
        for s in self.slots:
            out += [s.bufs[k][0].clone() for k in ("p", "m", "v")]
            out.append(self.opt.state[s.param]["step"].clone())
        return out

    def step(self, it, do_step, hp, mult=1.0, premultiply=None, tag=""):
        """Gradients of step `it` in, one optimizer step, every element against the float64 reference
        of that step (gradients read as g * mult).  -> max normalised error per figure of KEYS."""
        self.set_grads(it, premultiply)
        before = self.state_cpu()
        do_step()
        after = self.state_cpu()
        errs = dict.fromkeys(KEYS, 0.0)
        for s, (p0, m0, v0, t0), (p1, m1, v1, t1) in zip(self.slots, before, after):
            where = (tag, it, s.shape)
            g = s.inp["g"][it].double() * mult
            p0, m0, v0 = p0.double(), m0.double(), v0.double()
            pr, mr, vr = ref_adam(p0, m0, v0, g, t0 + 1.0, **hp)
            assert all(bool(torch.isfinite(x).all()) for x in (pr, mr, vr)), where  # the reference itself
            assert t1 == t0 + 1.0, where
            assert not any(bool(torch.isnan(x).any()) for x in (p1, m1, v1)), where
            mag_m = torch.maximum(m0.abs(), g.abs())
            # what exp_avg's rounding (EPS32 * mag_m) becomes in the update: x step size / denominator
            b1, b2 = hp["betas"]
            t = t0 + 1.0
            carried = hp["lr"] / (1.0 - b1 ** t) * mag_m / (vr.sqrt() / math.sqrt(1.0 - b2 ** t) + hp["eps"])
            e = {"m": _nerr(m1, mr, mag_m),
                 "v": _nerr(v1, vr, torch.maximum(v0.abs(), g * g)),
                 "p": _nerr(p1, pr, p0.abs() + (pr - p0).abs()),
                 "pc": _nerr(p1, pr, p0.abs() + (pr - p0).abs() + carried)}
            for k in errs:
                errs[k] = max(errs[k], e[k])
            # zero gradient on zero moments: nothing moves
            still = (g == 0) & (m0 == 0) & (v0 == 0)
            assert torch.equal(p1[still].double(), p0[still]), where
            assert not bool(m1[still].any()) and not bool(v1[still].any()), where
            ok, name = s.guards_intact()
            assert ok, where + (name,)
        return errs


def _within_bound(errs, name, where):
    """The kernel's figures of one step are printed, then held to twice torch's on that input set."""
    print("ADAM_ERR %-12s m %.3f v %.3f p %.3f pc %.3f  %s" % ((name,) + tuple(errs[k] for k in KEYS) + (where,)))
    for k, rec in zip(KEYS, TORCH_ERR[name]):
        assert errs[k] <= 2.0 * rec, (name, where, k, errs[k], 2.0 * rec)


def _mult32(gscale, loss_scale=None):
    """The multiplier as the kernel forms it: fp32(grad_scale) [* fp32(1 / loss_scale)] in fp32."""
    m = torch.tensor(gscale, dtype=torch.float32)
    if loss_scale is not None:
        m = m * torch.tensor(1.0 / loss_scale, dtype=torch.float32)
    return m


# ------------------------------------------------------------------ the cases, shared with the yardstick

def _plain_cases():
    for a in ALIGN:
        for h in HYPER:
            for resumed in (False, True):
                for gs in GSCALE:
                    yield a, h, resumed, gs


def _conv_inputs(key, seed=7):
    shape = (BIG[key] if key in BIG else CONVS[key])[0]
    return make_inputs([shape], seed + sum(shape), steps=2)


def _skip_inputs():
    return make_inputs(SKIP_PLAIN + [CONVS[k][0] for k in SKIP_CONVS], 31, steps=3)


def _block_shapes():
    return [s for _ in range(NBLOCKS) for s in ((64, 64, 3, 3), (64,), (64,))]


def _many_shapes():
    return [SIZES[(3 * i + i // 11) % len(SIZES)] for i in range(100)]


def _torch_cpu_errors():
    """torch.optim.Adam(foreach=False), fp32, CPU, on every input set of this module -> per set, the
    max normalised error against the float64 reference.  Gradient multipliers are applied in fp32 as
    the kernel does."""
    out = {}

    def run(name, inputs, hp, step0=0, mult=1.0, mult32=None, offs=(0, 0), plan=None):
        """plan: (gradient set, multiplier, its fp32 form) per step; default every set with `mult`."""
        rig = Rig(inputs, "cpu", offs)
        opt = torch.optim.Adam(rig.params, foreach=False, **hp)
        rig.install(opt, step0)
        worst = out.setdefault(name, dict.fromkeys(KEYS, 0.0))
        for it, mu, mu32 in plan or [(it, mult, mult32) for it in range(len(inputs[0]["g"]))]:
            e = rig.step(it, opt.step, hp, mu, None if mu == 1.0 else mu32, "torch-cpu")
            for k in worst:
                worst[k] = max(worst[k], e[k])

    for a, h, resumed, gs in _plain_cases():
        run("plain", make_inputs(SIZES, 11, resumed), HYPER[h], 1000 if resumed else 0, GSCALE[gs],
            _mult32(GSCALE[gs]), ALIGN[a])
    run("many", make_inputs(_many_shapes(), 13), HYPER["default"])
    for key in list(CONVS) + list(BIG):
        run(key, _conv_inputs(key), HYPER["default"])
    # the skip-flag test: loss scale 2^10, a skipped step (gradient set 1 is never applied), then 2^9
    run("skip", _skip_inputs(), HYPER["alt"], plan=[(0, 2.0 ** -10, _mult32(1.0, 2.0 ** 10)),
                                                    (2, 2.0 ** -9, _mult32(1.0, 2.0 ** 9))])
    run("blocks", make_inputs(_block_shapes(), 17, steps=2), HYPER["default"])
    return out


def test_torch_cpu_adam_is_the_yardstick():
    """The recorded figures of torch's own fp32 error (TORCH_ERR) hold on this machine's CPU:
    re-measured, they stay within the bounds they produce."""
    for name, worst in _torch_cpu_errors().items():
        print("TORCH_CPU_ERR %-12s m %.3f v %.3f p %.3f pc %.3f" % ((name,) + tuple(worst[k] for k in KEYS)))
        for k, rec in zip(KEYS, TORCH_ERR[name]):
            assert worst[k] <= 2.0 * rec, (name, k, worst[k], rec)


# ------------------------------------------------------------------ 2. plain parameters

@pytest.mark.parametrize("gs", list(GSCALE))
@pytest.mark.parametrize("resumed", [False, True], ids=["fresh", "step1000"])
@pytest.mark.parametrize("hyper", list(HYPER))
@pytest.mark.parametrize("align", list(ALIGN))
def test_plain_parameters(align, hyper, resumed, gs):
    from sqr.optim import Adam
    hp = HYPER[hyper]
    rig = Rig(make_inputs(SIZES, 11, resumed), DEV, ALIGN[align])
    opt = Adam(rig.params, **hp)
    rig.install(opt, 1000 if resumed else 0)
    p_start = [s.inp["p"].clone() for s in rig.slots]
    opt.sqr_grad_scale = GSCALE[gs]
    try:
        for it in range(STEPS):
            _within_bound(rig.step(it, opt.step, hp, GSCALE[gs], tag="plain"), "plain", (align, hyper, resumed, gs, it))
    finally:
        opt.sqr_grad_scale = 1.0
    if not resumed:   # the zero-gradient elements stand where they started, after all three steps
        for s, p0 in zip(rig.slots, p_start):
            z = s.inp["g"][0] == 0
            assert torch.equal(s.param.detach().cpu()[z], p0[z]), s.shape


@pytest.mark.parametrize("hyper", list(HYPER))
@pytest.mark.parametrize("align", list(ALIGN))
def test_first_step_moments_are_single_products(align, hyper):
    """Fresh state, grad_scale 1: exp_avg = fl(fl32(1 - b1) g) and exp_avg_sq = fl(fl(fl32(1 - b2) g) g),
    one IEEE rounding per product, so the kernel's values equal the CPU's fp32 products bit for bit."""
    from sqr.optim import Adam
    hp = HYPER[hyper]
    rig = Rig(make_inputs(SIZES, 11), DEV, ALIGN[align])
    opt = Adam(rig.params, **hp)
    rig.install(opt)
    rig.set_grads(0)
    opt.step()
    omb1 = torch.tensor(1.0 - hp["betas"][0], dtype=torch.float32)
    omb2 = torch.tensor(1.0 - hp["betas"][1], dtype=torch.float32)
    for s, (_, m1, v1, t1) in zip(rig.slots, rig.state_cpu()):
        g = s.inp["g"][0]
        assert t1 == 1.0
        assert torch.equal(m1.view(torch.int32), (omb1 * g).view(torch.int32)), s.shape
        assert torch.equal(v1.view(torch.int32), ((omb2 * g) * g).view(torch.int32)), s.shape


def test_many_parameters_take_several_launches():
    """100 parameters: more than 40 jobs (three adam_kernel launches) and more than 80 parameters (two
    C calls); every one is updated exactly once per step."""
    from sqr.optim import Adam
    hp = HYPER["default"]
    rig = Rig(make_inputs(_many_shapes(), 13), DEV)
    opt = Adam(rig.params, **hp)
    rig.install(opt)
    for it in range(STEPS):
        _within_bound(rig.step(it, opt.step, hp, tag="many"), "many", it)
    assert all(t == float(STEPS) for *_, t in rig.state_cpu())


# ------------------------------------------------------------------ 3. conv weights and their packed layouts

def _make_conv(key_or_spec):
    from sqr import conv as sc
    (K, C, R, S), stride, pad = CONVS[key_or_spec] if isinstance(key_or_spec, str) else key_or_spec
    return sc.Conv2d(C, K, R, stride=stride, padding=pad, bias=False).to(DEV)


def _poison(m, dt):
    from sqr import conv as sc
    for buf in sc.packed_buffers(m, dt):
        if buf is not None:
            buf.view(torch.int16).fill_(POISON)


def _expected_packed(w, stride, pad, dt):
    """torch restatement of both layouts from the fp32 weight; the cast is torch's (round to nearest even)."""
    K, C, R, S = w.shape
    krsc = w.permute(0, 2, 3, 1).reshape(K, R * S * C)
    if C < 8:
        kp = 64
        while kp < R * S * C:
            kp *= 2
        krsc = torch.nn.functional.pad(krsc, (0, kp - R * S * C))
    classes = []
    for ph in range(stride):
        for pw in range(stride):
            r0, s0 = (ph + pad) % stride, (pw + pad) % stride
            classes.append(w[:, :, r0::stride, s0::stride].permute(1, 2, 3, 0).reshape(-1))
    return krsc.to(dt).contiguous(), torch.cat(classes).to(dt).contiguous()


def _bits16(t):
    return t.contiguous().view(torch.int16).reshape(-1)


def _assert_packed(m, dt, where, crsk_written=True):
    from sqr import conv as sc
    w = m.weight.detach()
    K, C, R, S = w.shape
    stride, pad = m.stride[0], m.padding[0]
    buf = m._wpack[dt]
    assert buf[0] == sc._pack_key(m.weight), where   # the step marked them as holding this weight
    krsc, crsk = _expected_packed(w, stride, pad, dt)
    assert torch.equal(_bits16(buf[1]), _bits16(krsc)), where + ("krsc",)
    if C < 8 or C & (C - 1) == 0:
        pk, pc = sc.pack_weight(w, sc._desc(1, C, R, R, K, R, S, stride, pad, dt), C >= 8)
    else:   # pack_weight takes the conv kernels' channel counts only: pack_all on a twin module
        twin = _make_conv(((K, C, R, S), stride, pad))
        with torch.no_grad():
            twin.weight.copy_(w)
        sc.pack_all([twin], dt)
        pk, pc = twin._wpack[dt][1:]
    assert torch.equal(_bits16(buf[1]), _bits16(pk)), where + ("krsc vs pack_weight",)
    if C >= 8 and crsk_written:
        assert torch.equal(_bits16(buf[2]), _bits16(crsk)), where + ("crsk",)
        assert torch.equal(_bits16(buf[2]), _bits16(pc)), where + ("crsk vs pack_weight",)


def _forward(m, x, dt):
    with torch.no_grad(), torch.autocast("cuda", dtype=dt):
        return m(x)


def _forward_fresh(m, x, dt):
    """The same conv on a private copy of the weight: no module cache can be involved."""
    from sqr import conv as sc
    with torch.no_grad(), torch.autocast("cuda", dtype=dt):
        return sc.conv2d(x, m.weight.detach().clone(), None, m.stride[0], m.padding[0])


def _unpacked_conv_follows_the_weight(spec_key, dt, inputs, forward=True):
    """A conv whose packing the step leaves to pack_all: its packed cache holds the OLD weight when the
    step runs; the step must update the weight and the next forward must see the new one (without
    `forward`, for a channel count the conv kernels do not take: the cache must be stale after the
    step, and pack_all must then hold the new weight in both layouts)."""
    from sqr import conv as sc
    from sqr.optim import Adam
    hp = HYPER["default"]
    spec = BIG[spec_key] if spec_key in BIG else CONVS[spec_key]
    m = _make_conv(spec)
    rig = Rig(inputs, DEV)
    rig.bind(m)
    opt = Adam(m.parameters(), **hp).attach(m, dt)
    rig.install(opt)
    C = spec[0][1]
    x = torch.randn(1, C, 6, 6, generator=torch.Generator().manual_seed(5)).to(DEV)
    probe = torch.empty(1, dtype=dt, device=DEV)
    sc.pack_all([m], dt)   # the cache now holds the start weight
    assert m._cached(probe) is not None
    if forward:
        y_old = _forward(m, x, dt)
        assert torch.equal(y_old, _forward_fresh(m, x, dt))
    for it in range(2):
        _within_bound(rig.step(it, opt.step, hp, tag=spec_key), spec_key, (str(dt), it))   # must not raise
        assert m._cached(probe) is None, it   # what the forward would use: stale, so it repacks
        if not forward:
            sc.pack_all([m], dt)
            _assert_packed(m, dt, (spec_key, str(dt), it))
            continue
        y = _forward(m, x, dt)
        assert torch.equal(y, _forward_fresh(m, x, dt)), it
        assert not torch.equal(y, y_old), it
        y_old = y


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("key", list(CONVS))
def test_conv_weight_update_and_packing(key, dt):
    from sqr.optim import Adam
    if key == "k32c32r3s1":
        return _unpacked_conv_follows_the_weight(key, dt, _conv_inputs(key))
    hp = HYPER["default"]
    m = _make_conv(key)
    rig = Rig(_conv_inputs(key), DEV)
    rig.bind(m)
    opt = Adam(m.parameters(), **hp).attach(m, dt)
    rig.install(opt)
    _poison(m, dt)
    for it in range(2):
        _within_bound(rig.step(it, opt.step, hp, tag=key), key, (str(dt), it))
        _assert_packed(m, dt, (key, str(dt), it))


# ------------------------------------------------------------------ 4. the skip flag on every branch

@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_skipped_step_touches_nothing(bad):
    from sqr import amp
    from sqr.optim import Adam
    hp = HYPER["alt"]
    dt = torch.float16
    convs = torch.nn.ModuleList([_make_conv(k) for k in SKIP_CONVS])
    plain = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(n)) for n in SKIP_PLAIN])
    model = torch.nn.ModuleDict({"plain": plain, "convs": convs})
    inputs = _skip_inputs()
    # the second plain parameter starts one float into its buffer: scalar path
    rig = Rig(inputs, DEV)
    rig.slots[1] = Slot(inputs[1], DEV, 1, 0)
    rig.params[1] = rig.slots[1].param
    rig.bind(model)
    assert [tuple(q.shape) for q in model.parameters()] == [s.shape for s in rig.slots]
    opt = Adam(model.parameters(), **hp).attach(model, dt)
    rig.install(opt)
    for m in convs:
        _poison(m, dt)
    scale = 2.0 ** 10
    scaler = amp.GradScaler(init_scale=scale, growth_interval=1000)

    def scaled_step():
        scaler.step(opt)
        scaler.update()

    def packed_bits():
        return [b.clone() for m in convs for b in m._wpack[dt][1:] if b is not None]

    # gradients are stored scaled (g as made, read as g / scale)
    _within_bound(rig.step(0, scaled_step, hp, 1.0 / scale, tag="skip"), "skip", "clean step 0")
    for m in convs:
        _assert_packed(m, dt, ("skip", "clean step 0"))
    before, pbefore = rig.bits(), packed_bits()
    # one non-finite element, in the unaligned plain parameter only
    rig.set_grads(1)
    rig.slots[1].view("g")[517] = bad
    scaled_step()
    assert scaler.get_scale() == scale / 2
    after, pafter = rig.bits(), packed_bits()
    for i, (a, b) in enumerate(zip(before, after)):
        assert torch.equal(a, b), ("parameter / moment / counter changed by a skipped step", i)
    for i, (a, b) in enumerate(zip(pbefore, pafter)):
        assert torch.equal(a, b), ("packed buffer changed by a skipped step", i)
    # the next clean step moves every one of them again
    _within_bound(rig.step(2, scaled_step, hp, 2.0 / scale, tag="skip"), "skip", "clean step 2")
    for m in convs:
        _assert_packed(m, dt, ("skip", "clean step 2"))
    for i, (a, b) in enumerate(zip(before, rig.bits())):
        assert not torch.equal(a, b), ("unchanged by the clean step", i)
    for i, (a, b) in enumerate(zip(pbefore, packed_bits())):
        assert not torch.equal(a, b), ("packed buffer unchanged by the clean step", i)
    assert all(t == 2.0 for *_, t in rig.state_cpu())


# ------------------------------------------------------------------ 5. more than 24 packed convs; rows too large

def test_thirty_conv_bn_blocks():
    from sqr import conv as sc
    from sqr.optim import Adam
    hp = HYPER["default"]
    dt = torch.bfloat16
    layers = []
    for _ in range(NBLOCKS):
        layers += [sc.Conv2d(64, 64, 3, 1, 1, bias=False), torch.nn.BatchNorm2d(64)]
    model = torch.nn.Sequential(*layers).to(DEV)
    rig = Rig(make_inputs(_block_shapes(), 17, steps=2), DEV)
    rig.bind(model)
    assert len(rig.params) == 90
    opt = Adam(model.parameters(), **hp).attach(model, dt)
    rig.install(opt)
    convs = [m for m in model if isinstance(m, sc.Conv2d)]
    for m in convs:
        _poison(m, dt)
    for it in range(2):
        _within_bound(rig.step(it, opt.step, hp, tag="blocks"), "blocks", it)   # must not raise
        for i, m in enumerate(convs):
            _assert_packed(m, dt, ("30 blocks", it, i))
    assert all(t == 2.0 for *_, t in rig.state_cpu())


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("key", list(BIG))
def test_oversized_row_is_left_to_pack_all(key, dt):
    _unpacked_conv_follows_the_weight(key, dt, _conv_inputs(key), forward=key == "c2048")


def _adam_params(rig, convs=()):
    """ctypes sqr_adam_param array of the rig's parameters; convs: {slot index: (module, dtype)} to pack."""
    from sqr import conv as sc
    from sqr._lib import SqrAdamParam
    arr = (SqrAdamParam * len(rig.slots))()
    for j, s in enumerate(rig.slots):
        st = rig.opt.state[s.param]
        a = arr[j]
        a.p, a.g = s.param.data_ptr(), s.param.grad.data_ptr()
        a.exp_avg, a.exp_avg_sq = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
        a.step, a.n = st["step"].data_ptr(), s.n
        if j in convs:
            m, dt = convs[j]
            K, C, R, S = s.shape
            a.desc = sc._desc(1, C, R, R, K, R, S, m.stride[0], m.padding[0], dt)
            krsc, crsk = sc.packed_buffers(m, dt)
            a.w_krsc, a.w_crsk = krsc.data_ptr(), crsk.data_ptr()
    return arr


@pytest.mark.parametrize("case", ["81 parameters", "bad size at 45", "25th packed conv at 64", "oversized row at 41"])
def test_rejected_call_launches_nothing(case):
    """A call that fails argument checking fails before its first launch: non-zero return code,
    every parameter, moment, counter and packed buffer bit-identical (the offending entry lies behind
    the first 40 jobs, which a check made inside the launch loop would already have updated)."""
    from sqr import conv as sc
    from sqr._lib import lib, stream_ptr
    from sqr.optim import Adam
    dt = torch.bfloat16
    shapes, convs = [64] * 40, {}
    if case == "81 parameters":
        shapes = [64] * 81
    elif case == "bad size at 45":
        shapes = [64] * 50
    elif case == "25th packed conv at 64":
        shapes += [(64, 64, 1, 1)] * 25
    else:
        shapes += [64, BIG["c1856"][0]]
    rig = Rig(make_inputs(shapes, 23, steps=1), DEV)
    opt = Adam(rig.params, lr=1e-3)
    rig.install(opt)
    rig.set_grads(0)
    mods = []
    for j, shape in enumerate(shapes):
        if not isinstance(shape, int):
            m = _make_conv((shape, 1, shape[2] // 2))
            _poison(m, dt)
            convs[j] = (m, dt)
            mods.append(m)
    arr = _adam_params(rig, convs)
    if case == "bad size at 45":
        arr[45].n = 0
    before = rig.bits()
    rc = lib().sqr_adam_step(arr, len(shapes), 1e-3, 0.9, 0.999, 1e-8, 1.0, stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc != 0
    assert lib().sqr_last_error_string().decode().startswith("adam_step")
    for i, (a, b) in enumerate(zip(before, rig.bits())):
        assert torch.equal(a, b), ("a rejected call changed something", i)
    for m in mods:
        for buf in m._wpack[dt][1:]:
            assert bool((buf.view(torch.int16) == POISON).all())
    # the same call without the offending entry goes through and updates every parameter once
    if case != "81 parameters":
        n_ok = {"bad size at 45": 45, "25th packed conv at 64": 64, "oversized row at 41": 41}[case]
        rc = lib().sqr_adam_step(arr, n_ok, 1e-3, 0.9, 0.999, 1e-8, 1.0, stream_ptr(DEV))
        torch.cuda.synchronize()
        assert rc == 0
        steps = [t for *_, t in rig.state_cpu()]
        assert steps == [1.0] * n_ok + [0.0] * (len(shapes) - n_ok)


# ------------------------------------------------------------------ 6. the finite check and the scale update

CHECK_SIZES = [1, 3, 5, 16383, 16384, 16385, 32773]
FCHUNK = 16384


def _positions(n):
    """Where a single non-finite value goes: first, last, last of the last workgroup's 4-wide body,
    its scalar tail, the last workgroup's first element."""
    i0 = ((n - 1) // FCHUNK) * FCHUNK
    body = (n - i0) & ~3
    pos = {0, n - 1, i0}
    if body:
        pos.add(i0 + body - 1)
    if n - i0 > body:
        pos.add(i0 + body)
    if i0:   # and the same places in the first (full) workgroup
        pos |= {FCHUNK - 1, FCHUNK - 4}
    return sorted(pos)


class _Grads:
    """Stands in for an optimizer in GradScaler._check, which reads nothing but each parameter's .grad
    (a gradient view cannot be attached to a real Parameter of another shape)."""

    def __init__(self, grads, gscale=1.0):
        self.param_groups = [{"params": [types.SimpleNamespace(grad=g) for g in grads]}]
        self.sqr_grad_scale = gscale


def _flag(scaler, grads, gscale=1.0):
    scaler._found_inf.zero_()
    scaler._check(_Grads(grads, gscale), scaled=True)
    return int(scaler._found_inf.item())


def _expected_flag(grads_cpu, gscale, loss_scale):
    m = _mult32(gscale, loss_scale)
    return int(any(bool((~torch.isfinite(g * m)).any()) for g in grads_cpu))


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "base+1"])
def test_finite_check_single_tensor(off, bad):
    from sqr import amp
    gen = torch.Generator().manual_seed(3)
    for loss_scale, gscale in ((1.0, 1.0), (4.0, 0.5)):   # multiplier 1 (values read as they are) and 1/8
        scaler = amp.GradScaler(init_scale=loss_scale)
        for n in CHECK_SIZES:
            _, g = _guarded(n, off, DEV)
            g_cpu = torch.randn(n, generator=gen)
            g.copy_(g_cpu)
            assert g.data_ptr() % 16 == 4 * off
            assert _flag(scaler, [g], gscale) == 0 == _expected_flag([g_cpu], gscale, loss_scale), (n, "control")
            for i in _positions(n):
                keep = g_cpu[i].item()
                g_cpu[i] = bad
                g[i] = bad
                assert _flag(scaler, [g], gscale) == _expected_flag([g_cpu], gscale, loss_scale) == 1, (n, i)
                g_cpu[i] = keep
                g[i] = keep
            assert _flag(scaler, [g], gscale) == 0, (n, "restored")


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_finite_check_85_separate_tensors(bad):
    """85 tensors with gaps between them: _merged_ranges cannot join them, so the check takes a second
    launch (80 spans each); the non-finite value is found wherever it sits."""
    from sqr import amp
    sizes = [(1, 3, 5, 7, 16385)[i % 5] if i % 20 == 4 or i % 5 != 4 else 9 for i in range(85)]
    gaps = [3, 4, 1]
    buf = torch.randn(sum(sizes) + 85 * 4 + 8, generator=torch.Generator().manual_seed(4))
    dbuf = buf.to(DEV)
    grads, grads_cpu, o = [], [], 4
    for i, n in enumerate(sizes):
        grads.append(dbuf[o:o + n])
        grads_cpu.append(buf[o:o + n])
        o += n + gaps[i % 3]
    assert len(amp._merged_ranges(grads)) == 85
    scaler = amp.GradScaler(init_scale=1.0)
    assert _flag(scaler, grads) == 0 == _expected_flag(grads_cpu, 1.0, 1.0)
    for ti in (0, 4, 79, 80, 84):
        for i in {0, sizes[ti] - 1}:
            keep = grads_cpu[ti][i].item()
            grads_cpu[ti][i] = bad
            grads[ti][i] = bad
            assert _flag(scaler, grads) == _expected_flag(grads_cpu, 1.0, 1.0) == 1, (ti, i)
            grads_cpu[ti][i] = keep
            grads[ti][i] = keep
    assert _flag(scaler, grads) == 0


@pytest.mark.parametrize("n", [1, 5, 16385])
def test_finite_check_sees_the_multiplier(n):
    """A finite gradient that overflows only once multiplied by 1 / scale (scale < 1) counts; one that
    the multiplier brings back into range does not."""
    from sqr import amp
    for off in (0, 1):
        _, g = _guarded(n, off, DEV)
        g.fill_(1.0)
        g[n - 1] = 3e38
        g_cpu = g.cpu()
        assert _flag(amp.GradScaler(init_scale=0.5), [g], 1.0) == _expected_flag([g_cpu], 1.0, 0.5) == 1
        assert _flag(amp.GradScaler(init_scale=1.0), [g], 0.5) == _expected_flag([g_cpu], 0.5, 1.0) == 0
        assert _flag(amp.GradScaler(init_scale=1.0), [g], 1.0) == 0
        g[n - 1] = -3e38
        assert _flag(amp.GradScaler(init_scale=0.5), [g], 1.0) == 1
        assert _flag(amp.GradScaler(init_scale=0.25), [g], 3.0) == _expected_flag([g.cpu()], 3.0, 0.25) == 1


def test_update_scale_follows_torch():
    """sqr_amp_update_scale against torch._amp_update_scale_ (what torch.amp.GradScaler.update runs):
    growth, backoff, tracker, and a growth that would overflow fp32 (the scale stays, the tracker
    resets)."""
    from sqr import amp
    for init, growth, backoff, interval, found in (
            (2.0 ** 10, 3.0, 0.25, 2, [0, 0, 1, 0, 1, 1, 0, 0, 0, 0]),
            (3e38, 2.0, 0.5, 3, [0, 0, 0, 0, 0, 1, 0, 0, 0]),
            (1.5e38, 2.0, 0.5, 1, [0, 0, 0, 1])):
        sc = amp.GradScaler(init_scale=init, growth_factor=growth, backoff_factor=backoff, growth_interval=interval)
        rs = torch.full((1,), init, dtype=torch.float32, device=DEV)
        rt = torch.zeros(1, dtype=torch.int32, device=DEV)
        for it, f in enumerate(found):
            sc._found_inf.fill_(f)
            sc.update()
            torch._amp_update_scale_(rs, rt, torch.full((1,), float(f), device=DEV), growth, backoff, interval)
            assert sc.get_scale() == rs.item() and math.isfinite(sc.get_scale()), (init, it)
            assert int(sc._growth_tracker.item()) == int(rt.item()), (init, it)
            assert int(sc._found_inf.item()) == 0
    sc = amp.GradScaler(init_scale=3e38, growth_factor=2.0, growth_interval=2)
    s0 = sc.get_scale()
    sc.update()
    assert (sc.get_scale(), int(sc._growth_tracker.item())) == (s0, 1)
    sc.update()   # the growth interval: 6e38 is not an fp32 number
    assert (sc.get_scale(), int(sc._growth_tracker.item())) == (s0, 0)
