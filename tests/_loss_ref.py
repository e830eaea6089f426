"""References for the loss kernels of sqr_loss.hip, stage by stage (torch-free numpy on oracle/sq_oracle.py).

Three things:

  * float64 block moments: the 17 parameter moments of sqr_sq_dev.h (m[0..16], listed above vox_bwd_lnG) plus
    the loss term, per ray (ImplicitLoss) or per (ix, iy) column (ExplicitLoss), summed per block in the
    kernel's index order, next to the sum of the absolute values of the same terms.  They are written
    from sq_oracle's natural-domain chain (_forward_core), not from the kernel's log2-domain one.
  * finalize(): loss_finalize_kernel / finalize_sample / block_mean / loss_mean_kernel restated in float64,
    addition by addition.  The loss values are meant to be compared bitwise.
  * a float32 evaluation of the kernel's own algorithm (log2-domain chain, prefix form
    Ttot * sum J - sum P J) with numpy's exp2 / log2.  It is the SCALE of the stage tolerances: a kernel
    may err a small factor of what this errs against float64.  It is never the expected value.

Layout pinned here (and by tests/test_loss_kernels_gpu.py): partials [B][nblk][18] float32, slot 17 the
loss sum; ImplicitLoss block k holds the rays pix = k * NT .. k * NT + NT - 1, pix = r * R + c of the image
pixel (r, c), whose ray is x = c, y = R - 1 - r; NT = 256 for R <= 128, else 128.  ExplicitLoss block k
holds the columns col = ix * n + iy, NT = 256, n = len(np.arange(0, 1 + 1/R, 1/R)).
"""
import numpy as np

import sq_oracle as O

NACC = 18
SLOTS = ["m%d" % i for i in range(17)] + ["loss"]
COMPONENTS = ["a0", "a1", "a2", "e1", "e2", "t0", "t1", "t2", "qx", "qy", "qz", "qw"]
EXPLICIT_SHARP = 5.0
f32 = np.float32
_LN2_32, _LOG2E_32 = f32(0.69314718055994530942), f32(1.44269504088896340736)
_SQ_ZERO = f32(2.0 ** -75)
_FLT_MIN = f32(np.finfo(np.float32).tiny)


def implicit_threads(R):
    return 128 if R > 128 else 256


def implicit_nblk(R):
    NT = implicit_threads(R)
    return (R * R + NT - 1) // NT


def explicit_n(R):
    return O.explicit_axis(R).size


def explicit_nblk(R):
    n = explicit_n(R)
    return (n * n + 255) // 256


def _blocks(per_thread, NT):
    """[18, nthreads] -> [nblk, 18]: threads k * NT .. k * NT + NT - 1 summed in order (np.cumsum is sequential)."""
    n = per_thread.shape[1]
    nblk = (n + NT - 1) // NT
    pad = np.zeros((NACC, nblk * NT), per_thread.dtype)
    pad[:, :n] = per_thread
    return np.cumsum(pad.reshape(NACC, nblk, NT), axis=2, dtype=per_thread.dtype)[:, :, -1].T.copy()


# ------------------------------------------------------------------------------------ float64 moments
def voxel_terms(c, gocc, e, sharp):
    """The 17 moment terms of every voxel for dL/docc = gocc: [17, x, y, z] float64.

    c is sq_oracle._forward_core's dict.  hG = dL/dln G; the shares A/F1, B/F1, E/F, C/F and the natural
    logarithms come from c's own A, B, C, E, F."""
    e1, e2 = e
    x = sharp * (1 - c["G"])
    occ, omo = O._sigmoid(x), O._sigmoid(-x)
    hG = gocc * (-sharp) * occ * omo * c["G"]
    g_lnF = hG * e1
    g_lnE = g_lnF * c["E"] / c["F"]
    g_lnC = g_lnF * c["C"] / c["F"]
    g_lnF1 = g_lnE * e2 / e1
    g_lnA = g_lnF1 * c["A"] / c["F1"]
    g_lnB = g_lnF1 * c["B"] / c["F1"]
    lnA, lnB, lnC = np.log(c["A1"]) / e2, np.log(c["B1"]) / e2, np.log(c["C1"]) / e1
    lnE, lnF = np.log(c["F1"]) * e2 / e1, np.log(c["F"])
    t = np.zeros((17,) + c["G"].shape)
    t[3] = hG * lnF - (g_lnE * lnE + g_lnC * lnC) / e1
    t[4] = (g_lnE * lnE - g_lnA * lnA - g_lnB * lnB) / e2
    u = c["u"]
    gu = [2 * u[0] * g_lnA / (e2 * c["A1"]), 2 * u[1] * g_lnB / (e2 * c["B1"]), 2 * u[2] * g_lnC / (e1 * c["C1"])]
    for i in range(3):
        t[i] = gu[i] * u[i]
        t[5 + i] = gu[i]
        for j in range(3):
            t[8 + 3 * i + j] = gu[i] * c["xyz"][j]
    return t


def implicit_rays(p, tr, R, tau, sharp, zero_fix=True):
    """One sample's rays in float64.  tr: the resized target [R, R] (image order r, c).

    Returns (val [18, R*R], absval [18, R*R], D [R, R], n_fixed): ray pix = r * R + c; the moments are
    already scaled by cg = sign(D - tv) * tau / R; slot 17 is |D - tv|; absval sums |term| over the ray;
    n_fixed counts the voxels with A1 == 0, B1 == 0 or C1 == 0 before the fix."""
    a, e, t, q, _ = O._clamp(p)
    axis = O.implicit_axis(R)
    c = O._forward_core(a, e, t, q, axis, zero_fix=zero_fix)
    raw = O._forward_core(a, e, t, q, axis, zero_fix=False)
    n_fixed = int(sum((raw[k] == 0).sum() for k in ("A1", "B1", "C1")))
    occ_f = O._sigmoid(sharp * (1 - c["G"]))[..., ::-1]
    T = np.exp(-tau * np.cumsum(occ_f, -1))
    depth = 1 - T.sum(-1) / R                              # [x, y]
    D = depth.T[::-1]                                      # [r, c]
    cg = (np.sign(D - tr) * tau / R)[::-1].T               # [x, y]
    suffix = np.cumsum(T[..., ::-1], -1)[..., ::-1]
    gocc = (cg[..., None] * suffix)[..., ::-1]
    with np.errstate(invalid="ignore", divide="ignore"):
        terms = voxel_terms(c, gocc, e, sharp)
    to_pix = lambda m: m.transpose(0, 2, 1)[:, ::-1].reshape(m.shape[0], R * R)   # [i, x, y] -> [i, r * R + c]
    val, absval = np.zeros((NACC, R * R)), np.zeros((NACC, R * R))
    val[:17], absval[:17] = to_pix(terms.sum(-1)), to_pix(np.abs(terms).sum(-1))
    val[17] = absval[17] = np.abs(D - tr).reshape(-1)
    return val, absval, D, n_fixed


def resized_target(true, R):
    """F.interpolate(nearest) of true [B, 1, H, W] or [B, H, W] to [B, R, R] (sq_oracle's index rule)."""
    true = np.asarray(true, np.float64)
    if true.ndim == 4:
        true = true[:, 0]
    ri, ci = O.nearest_src_index(R, true.shape[1]), O.nearest_src_index(R, true.shape[2])
    return true[:, ri][:, :, ci]


def implicit_block_moments(true, pred, R, tau, sharp, zero_fix=True):
    """-> dict(part [B, nblk, 18], abs [B, nblk, 18], D [B, R, R], margin, n_fixed [B]); margin = min |D - tv|."""
    tr = resized_target(true, R)
    B, NT = len(pred), implicit_threads(R)
    out = dict(part=[], abs=[], D=[], n_fixed=[])
    for b in range(B):
        val, absval, D, nf = implicit_rays(pred[b], tr[b], R, tau, sharp, zero_fix)
        out["part"].append(_blocks(val, NT))
        out["abs"].append(_blocks(absval, NT))
        out["D"].append(D)
        out["n_fixed"].append(nf)
    out = {k: np.stack(v) for k, v in out.items()}
    out["margin"] = float(np.abs(out["D"] - tr).min())
    return out


def explicit_block_moments(true, pred, R, zero_fix=True):
    """-> dict(part [B, nblk, 18], abs [B, nblk, 18], n, n_fixed [B]); column col = ix * n + iy, dL/docc = -2 d."""
    axis = O.explicit_axis(R)
    n = axis.size
    out = dict(part=[], abs=[], n_fixed=[])
    for b in range(len(pred)):
        at, et, tt, qt, _ = O._clamp(true[b])
        ap, ep, tp, qp, _ = O._clamp(pred[b])
        ct = O._forward_core(at, et, tt, qt, axis, zero_fix=zero_fix)
        cp = O._forward_core(ap, ep, tp, qp, axis, zero_fix=zero_fix)
        raw = O._forward_core(ap, ep, tp, qp, axis, zero_fix=False)
        d = O._sigmoid(EXPLICIT_SHARP * (1 - ct["G"])) - O._sigmoid(EXPLICIT_SHARP * (1 - cp["G"]))
        with np.errstate(invalid="ignore", divide="ignore"):
            terms = voxel_terms(cp, -2 * d, ep, EXPLICIT_SHARP)
        val, absval = np.zeros((NACC, n * n)), np.zeros((NACC, n * n))
        val[:17], absval[:17] = terms.sum(-1).reshape(17, -1), np.abs(terms).sum(-1).reshape(17, -1)
        val[17] = absval[17] = (d * d).sum(-1).reshape(-1)
        out["part"].append(_blocks(val, 256))
        out["abs"].append(_blocks(absval, 256))
        out["n_fixed"].append(int(sum((raw[k] == 0).sum() for k in ("A1", "B1", "C1"))))
    out = {k: np.stack(v) for k, v in out.items()}
    out["n"] = n
    return out


def implicit_scales(B, R):
    """(loss_scale, grad_scale) as sqr_implicit_loss_fwd_bwd_mean forms them."""
    rr = float(R) * float(R)
    return 1.0 / rr, 1.0 / (float(B) * rr)


def explicit_scales(B, R):
    n = explicit_n(R)
    n3 = float(n) * n * n
    return 100.0 / n3, 100.0 / (n3 * float(B))


# ------------------------------------------------------------------------------------ finalize
def _clampf(x, lo, hi):
    lo, hi = f32(lo), f32(hi)
    return np.where(x < lo, lo, np.where(x > hi, hi, x))


def _inrange(x, lo, hi):
    return ((x >= f32(lo)) & (x <= f32(hi))).astype(np.float64)


def block_mean(v, B):
    """block_mean of sqr_loss.hip: v [64 * nwaves] float64, one value per thread.  Every wave's 64-lane xor
    butterfly o = 32 .. 1 (lane l adds lane l ^ o), lane 0 of the waves added in order, then / B."""
    v = np.asarray(v, np.float64).reshape(-1, 64).copy()
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    t = np.float64(0.0)
    for w in range(v.shape[0]):
        t = t + v[w, 0]
    return t / np.float64(B)


def loss_mean(loss, B):
    """The batch mean as launch_finalize computes it: one block of ceil(B / 64) waves for B <= 1024, else
    loss_mean_kernel's 1024 strided sums (thread i adds rows i, i + 1024, ... in order) first."""
    loss = np.asarray(loss, np.float64)
    if B <= 1024:
        v = np.zeros((B + 63) // 64 * 64)
        v[:B] = loss
        return block_mean(v, B)
    v = np.zeros(1024)
    for start in range(0, B, 1024):
        chunk = loss[start:start + 1024]
        v[:len(chunk)] = v[:len(chunk)] + chunk
    return block_mean(v, B)


def finalize(partials, params, loss_scale, grad_scale):
    """loss_finalize_kernel in float64.  partials [B, nblk, 18] (the GPU's float32 values or float64 ones),
    params [B, 12] float32.

    Returns dict(loss [B], mean, grad [B, 12] float64 (not rounded to fp32), chain [B, 12]): chain is the
    same chain evaluated on absolute values, every difference a sum: the size of the terms a gradient
    entry is made of, times grad_scale."""
    partials = np.asarray(partials)
    p = np.asarray(params, np.float32)
    B, nblk, _ = partials.shape
    acc = np.zeros((B, NACC))
    for k in range(nblk):                       # the blocks one by one, in order
        acc = acc + partials[:, k].astype(np.float64)
    loss = acc[:, 17] * np.float64(loss_scale)
    a = _clampf(p[:, 0:3], 0.05, 1.0).astype(np.float64)
    t = _clampf(p[:, 5:8], 0.0, 1.0).astype(np.float64)
    mask = np.ones((B, 12))
    mask[:, 0:3] = _inrange(p[:, 0:3], 0.05, 1.0)
    mask[:, 3:5] = _inrange(p[:, 3:5], 0.1, 1.0)
    mask[:, 5:8] = _inrange(p[:, 5:8], 0.0, 1.0)
    raw = p.astype(np.float64)
    x, y, z, w = -raw[:, 8], -raw[:, 9], -raw[:, 10], raw[:, 11]
    tx, ty, tz = 2 * x, 2 * y, 2 * z

    def chain(acc, absolute):
        ab = np.abs if absolute else (lambda v: v)
        s = 1.0 if absolute else -1.0           # a - b becomes |a| + |b|
        X, Y, Z, W = ab(x), ab(y), ab(z), ab(w)
        TX, TY, TZ = ab(tx), ab(ty), ab(tz)
        Mr = [1 + s * (TY * Y + TZ * Z), TX * Y + s * TZ * W, TX * Z + TY * W,
              TX * Y + TZ * W, 1 + s * (TX * X + TZ * Z), TY * Z + s * TX * W,
              TX * Z + s * TY * W, TY * Z + TX * W, 1 + s * (TX * X + TY * Y)]
        acc = ab(acc)
        g = np.zeros((B, 12))
        sgv = acc[:, 5:8] / a
        g[:, 0:3] = s * acc[:, 0:3] / a
        g[:, 3:5] = acc[:, 3:5]
        gR = [acc[:, 8 + 3 * i + j] / a[:, i] + s * sgv[:, i] * t[:, j] for i in range(3) for j in range(3)]
        for j in range(3):
            g[:, 5 + j] = s * (Mr[0 + j] * sgv[:, 0] + Mr[3 + j] * sgv[:, 1] + Mr[6 + j] * sgv[:, 2])
        dx = (2 * Y * (gR[1] + gR[3]) + 2 * Z * (gR[2] + gR[6]) + 2 * W * (gR[7] + s * gR[5])
              + s * 4 * X * (gR[4] + gR[8]))
        dy = (2 * X * (gR[1] + gR[3]) + 2 * Z * (gR[5] + gR[7]) + 2 * W * (gR[2] + s * gR[6])
              + s * 4 * Y * (gR[0] + gR[8]))
        dz = (2 * X * (gR[2] + gR[6]) + 2 * Y * (gR[5] + gR[7]) + 2 * W * (gR[3] + s * gR[1])
              + s * 4 * Z * (gR[0] + gR[4]))
        dw = 2 * Z * (gR[3] + s * gR[1]) + 2 * Y * (gR[2] + s * gR[6]) + 2 * X * (gR[7] + s * gR[5])
        g[:, 8], g[:, 9], g[:, 10], g[:, 11] = s * dx, s * dy, s * dz, dw
        return g * np.float64(grad_scale)

    return dict(loss=loss, mean=loss_mean(loss, B), grad=chain(acc, False) * mask, chain=chain(acc, True), acc=acc)


# ------------------------------------------------------------------------------------ float32 evaluation
def _fma(a, b, c):
    """fmaf: the product of two float32 is exact in float64 (one extra rounding of the sum, rarely visible)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


class _SQ32:
    """sq_load of sqr_sq_dev.h on params [B, 12] float32; every member [B, 1, 1] (or a list of such)."""

    def __init__(self, p):
        p = np.asarray(p, f32)
        col = lambda v: np.asarray(v, f32).reshape(-1, 1, 1)
        self.a = [col(_clampf(p[:, i], 0.05, 1.0)) for i in range(3)]
        self.ia = [f32(1) / v for v in self.a]
        self.t = [col(_clampf(p[:, 5 + i], 0.0, 1.0)) for i in range(3)]
        self.e1, self.e2 = col(_clampf(p[:, 3], 0.1, 1.0)), col(_clampf(p[:, 4], 0.1, 1.0))
        self.ie1, self.ie2, self.r21 = f32(1) / self.e1, f32(1) / self.e2, self.e2 / self.e1
        x, y, z, w = col(-p[:, 8]), col(-p[:, 9]), col(-p[:, 10]), col(p[:, 11])
        tx, ty, tz = f32(2) * x, f32(2) * y, f32(2) * z
        twx, twy, twz = tx * w, ty * w, tz * w
        txx, txy, txz = tx * x, ty * x, tz * x
        tyy, tyz, tzz = ty * y, tz * y, tz * z
        one = f32(1)
        self.M = [one - (tyy + tzz), txy - twz, txz + twy, txy + twz, one - (txx + tzz), tyz - twx,
                  txz - twy, tyz + twx, one - (txx + tyy)]


def _lse2(x, y):
    m = np.maximum(x, y)
    e = np.exp2(np.minimum(x, y) - m)
    big = f32(1) / (f32(1) + e)
    small = e * big
    ge = x >= y
    return m + np.log2(f32(1) + e), np.where(ge, big, small), np.where(ge, small, big)


def implicit_f32(true, pred, R, tau, sharp):
    """implicit_loss_kernel in numpy float32 -> partials [B, nblk, 18] float32 (rays added in order)."""
    with np.errstate(all="ignore"):
        return _implicit_f32(true, pred, R, f32(tau), f32(sharp))


def _implicit_f32(true, pred, R, tau, sharp):
    s = _SQ32(pred)
    B = len(pred)
    tv = resized_target(true, R).astype(f32)
    axis = np.arange(R, dtype=f32) / f32(max(R - 1, 1))
    axis[0] = f32(1e-4)
    gx = axis[None, None, :] + np.zeros((1, R, 1), f32)            # [1, r, c]: x = c
    gy = axis[::-1][None, :, None] + np.zeros((1, 1, R), f32)      # y = R - 1 - r
    dx, dy = gx - s.t[0], gy - s.t[1]
    al, be = [], []
    for i in range(3):
        c = _fma(s.M[3 * i], dx, _fma(s.M[3 * i + 1], dy, -s.M[3 * i + 2] * s.t[2]))
        al.append(c * s.ia[i])
        be.append(s.M[3 * i + 2] * s.ia[i])
    l4 = np.log2(f32(1e-4))
    lfix = [l4 * s.ie2, l4 * s.ie2, l4 * s.ie1]
    i2 = [f32(2) * s.ie2, f32(2) * s.ie2, f32(2) * s.ie1]
    ntau, nsharp, nsl = -tau * _LOG2E_32, -sharp, -sharp * _LOG2E_32
    shape = (B, R, R)
    S, P = np.zeros(shape, f32), np.zeros(shape, f32)
    JA, JB = np.zeros((11,) + shape, f32), np.zeros((11,) + shape, f32)
    for k in range(R):
        gz = axis[R - 1 - k]
        u = [_fma(be[i], gz, al[i]) + np.zeros(shape, f32) for i in range(3)]
        nz = [np.abs(u[i]) > _SQ_ZERO for i in range(3)]
        l = [np.where(nz[i], np.log2(np.abs(u[i])) * i2[i], lfix[i]) for i in range(3)]
        lF1, rA, rB = _lse2(l[0], l[1])
        lE = s.r21 * lF1
        lF, rE, rC = _lse2(lE, l[2])
        G = np.exp2(s.e1 * lF)
        ex = np.exp2(_fma(-nsl, G, nsl))
        occ = f32(1) / (f32(1) + ex)
        omo = np.where(ex < f32(1e30), ex * occ, f32(1))
        S = S + occ
        T = np.exp2(ntau * S)
        hG = nsharp * occ * omo * G
        g_lnF = hG * s.e1
        g_lnE, g_lnC = g_lnF * rE, g_lnF * rC
        g_lnF1 = g_lnE * s.r21
        g_lnA, g_lnB = g_lnF1 * rA, g_lnF1 * rB
        eE = g_lnE * lE
        J = [None] * 11
        J[3] = _LN2_32 * (hG * lF - (eE + g_lnC * l[2]) * s.ie1)
        J[4] = _LN2_32 * s.ie2 * (eE - g_lnA * l[0] - g_lnB * l[1])
        cc = [i2[0] * g_lnA, i2[1] * g_lnB, i2[2] * g_lnC]
        for i in range(3):
            gu = np.where(nz[i], cc[i] * (f32(1) / np.where(nz[i], u[i], f32(1))), f32(0))
            J[i] = np.where(nz[i], cc[i], f32(0))
            J[5 + i] = gu
            J[8 + i] = gu * gz
        for i in range(11):
            JA[i] = JA[i] + J[i]
            JB[i] = _fma(P, J[i], JB[i])
        P = P + T
    Ttot = P
    D = f32(1) - Ttot / f32(R)
    diff = D - tv
    cg = np.where(diff > 0, f32(1), f32(-1)) * tau / f32(R)
    v = np.where(diff != 0, cg * _fma(Ttot, JA, -JB), f32(0))
    vals = np.zeros((NACC,) + shape, f32)
    vals[:8] = v[:8]
    for i in range(3):
        vals[8 + 3 * i], vals[9 + 3 * i], vals[10 + 3 * i] = gx * v[5 + i], gy * v[5 + i], v[8 + i]
    vals[17] = np.abs(diff)
    NT = implicit_threads(R)
    return np.stack([_blocks(vals[:, b].reshape(NACC, R * R), NT) for b in range(B)])


def _vox_fwd32(s, dx, dy, dz):
    u = []
    for i in range(3):
        v = _fma(s.M[3 * i], dx, _fma(s.M[3 * i + 1], dy, s.M[3 * i + 2] * dz))
        u.append(v * s.ia[i])
    sq = [np.where(ui * ui == 0, f32(1e-4), ui * ui) for ui in u]
    l1 = [np.log2(np.maximum(v, _FLT_MIN)) for v in sq]
    l = [l1[0] * s.ie2, l1[1] * s.ie2, l1[2] * s.ie1]
    lF1, rA, rB = _lse2(l[0], l[1])
    lE = s.r21 * lF1
    lF, rE, rC = _lse2(lE, l[2])
    return dict(u=u, l1=l1, l=l, lF1=lF1, lE=lE, lF=lF, rA=rA, rB=rB, rE=rE, rC=rC, G=np.exp2(s.e1 * lF))


def _occupancy32(G, sharp):
    ex = np.exp2(-sharp * (f32(1) - G) * _LOG2E_32)
    occ = f32(1) / (f32(1) + ex)
    return occ, np.where(ex < f32(1e30), ex * occ, f32(1))


def explicit_f32(true, pred, R):
    """explicit_loss_kernel in numpy float32 -> partials [B, nblk, 18] float32."""
    with np.errstate(all="ignore"):
        return _explicit_f32(true, pred, R)


def _explicit_f32(true, pred, R):
    st, sp = _SQ32(true), _SQ32(pred)
    B = len(pred)
    n = explicit_n(R)
    axis = (np.arange(n, dtype=np.float64) * (1.0 / R)).astype(f32)
    axis[0] = f32(1e-4)
    shape = (B, n, n)
    gx = axis[None, :, None] + np.zeros(shape, f32)    # col = ix * n + iy
    gy = axis[None, None, :] + np.zeros(shape, f32)
    sharp = f32(EXPLICIT_SHARP)
    m = np.zeros((NACC,) + shape, f32)
    for iz in range(n):
        gz = axis[iz]
        ft = _vox_fwd32(st, gx - st.t[0], gy - st.t[1], gz - st.t[2])
        f = _vox_fwd32(sp, gx - sp.t[0], gy - sp.t[1], gz - sp.t[2])
        ot, _ = _occupancy32(ft["G"], sharp)
        op, omp = _occupancy32(f["G"], sharp)
        d = ot - op
        m[17] = _fma(d, d, m[17])
        hG = f32(-2) * d * (-sharp) * op * omp * f["G"]
        g_lnF = hG * sp.e1
        g_lnE, g_lnC = g_lnF * f["rE"], g_lnF * f["rC"]
        g_lnF1 = g_lnE * sp.r21
        g_lnA, g_lnB = g_lnF1 * f["rA"], g_lnF1 * f["rB"]
        m[3] = m[3] + _LN2_32 * (hG * f["lF"] - (g_lnE * f["lE"] + g_lnC * f["l"][2]) * sp.ie1)
        m[4] = m[4] + _LN2_32 * sp.ie2 * (g_lnE * f["lE"] - g_lnA * f["l"][0] - g_lnB * f["l"][1])
        gu = [f32(2) * f["u"][0] * sp.ie2 * g_lnF1 * f["rA"] * np.exp2(-f["l1"][0]),
              f32(2) * f["u"][1] * sp.ie2 * g_lnF1 * f["rB"] * np.exp2(-f["l1"][1]),
              f32(2) * f["u"][2] * sp.ie1 * g_lnF * f["rC"] * np.exp2(-f["l1"][2])]
        for i in range(3):
            m[i] = _fma(gu[i], f["u"][i], m[i])
            m[5 + i] = m[5 + i] + gu[i]
            for j, g in enumerate((gx, gy, gz)):
                m[8 + 3 * i + j] = _fma(gu[i], g, m[8 + 3 * i + j])
    return np.stack([_blocks(m[:, b].reshape(NACC, n * n), 256) for b in range(B)])


# ------------------------------------------------------------------------------------ error figures
# A block off the silhouette has moments of 1e-30 ... 1e-290 at sharpness 260: occ (1 - occ) is below fp32's
# smallest normal 2^-126 there, any fp32 evaluation returns 0 or a few bits for it, and its relative error
# (up to 1) would be the maximum over the blocks for a right and for a wrong kernel alike.  The chain
# amplifies occ (1 - occ) by at most about 2^40 (sharp 2^8, G 2^11, 2 / e 2^5, 1 / |u| and tau Ttot / R the
# rest), so such a block's sum of |terms| is below 2^-86; the blocks that carry the gradient have 1e-5 or more
# (every case's largest block at least CARRY = 2^-20: asserted in test_loss_ref_cpu.py).  FLOOR lies between the two and is added to every denominator: it
# changes a carrying block's figure by less than 2^-40 of it and takes the underflowed ones out of the maximum.
# ExplicitLoss has sharpness 5 and no such amplification (its terms are 10 d occ (1 - occ) G times factors of
# order 1 ... 2^10, and at R = 1 the whole loss is 1e-19): its floor is fp32's smallest normal itself, and a
# carrying block has 2^20 times that.
FLOOR = 2.0 ** -60
CARRY = 2.0 ** -20
FLOOR_EXPLICIT = 2.0 ** -126
CARRY_EXPLICIT = 2.0 ** -106


def slot_errors(part, ref, floor):
    """Per slot: max over samples and blocks of |part - ref.part| / (ref.abs + floor)."""
    err = np.abs(np.asarray(part, np.float64) - ref["part"])
    return (err / (ref["abs"] + floor)).reshape(-1, NACC).max(0)


def component_errors(g, gref):
    """Per gradient component: max_b |g - gref| / max_b |gref| (a component that is 0 in every row: 0 or inf)."""
    err, scale = np.abs(g - gref).max(0), np.abs(gref).max(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(scale > 0, err / scale, np.where(err > 0, np.inf, 0.0))


# ------------------------------------------------------------------------------------ inputs
TAU, SHARP = 1.5, 260.0     # train.py's ImplicitLoss
DYADIC_E = ((1.0, 1.0), (0.5, 1.0), (1.0, 0.25))


def sample(rng, n):
    """The suite's parameter distribution (gen_rand_rot.py's ranges as parse_csv normalises them)."""
    a = rng.uniform(25, 75, (n, 3)) / 255.0
    e = rng.uniform(0.1, 1.0, (n, 2))
    t = (128.0 + rng.uniform(-40, 40, (n, 3))) / 255.0
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.concatenate([a, e, t, q], 1).astype(np.float32)


def dyadic_rows(a=(0.25, 0.25, 0.25), t=(0.5, 0.25, 0.75)):
    """Axis-aligned rows whose every quantity is exact on a dyadic grid: the zero fix fires on whole planes."""
    return np.array([list(a) + list(e) + list(t) + [0, 0, 0, 1] for e in DYADIC_E], np.float32)


def signed_target(pred, R, H, W, rng, tau=TAU, sharp=SHARP):
    """[B, 1, H, W] float32: the float64 depth image of every row plus s * d, s a random sign, d uniform in
    [0.01, 0.3], drawn at R x R; source pixel (i, j) holds the value of the last resized pixel whose
    nearest-source index is <= (i, j), so the resize returns the R x R draw itself."""
    ri, ci = O.nearest_src_index(R, H), O.nearest_src_index(R, W)
    rows = np.searchsorted(ri, np.arange(H), side="right") - 1
    cols = np.searchsorted(ci, np.arange(W), side="right") - 1
    out = np.zeros((len(pred), 1, H, W), np.float32)
    for b, p in enumerate(pred):
        D = O.depth_projection(p, R, tau, sharp)
        s = np.where(rng.uniform(size=(R, R)) < 0.5, -1.0, 1.0)
        base = D + s * rng.uniform(0.01, 0.3, (R, R))
        out[b, 0] = base[rows][:, cols]
    return out


# (R, H, W, B): the smallest shapes at which each branch of implicit_loss_kernel exists
IMPLICIT_SHAPES = [
    (2, 2, 2, 1),          # the smallest legal R
    (3, 3, 3, 2),
    (16, 16, 16, 2),       # exactly one block of 256 rays
    (17, 17, 17, 2),       # a second, partly filled block
    (33, 66, 66, 2),       # five blocks, integer downsample
    (12, 24, 40, 2),       # non-square target, non-integer ratio
    (129, 129, 129, 1),    # the first size on 128-thread blocks
    (5, 5, 5, 3), (9, 9, 9, 3), (17, 17, 17, 3),   # the dyadic rows (B = 3 marks them)
]
# R -> nodes: explicit_loss_kernel's branches
EXPLICIT_R = [1, 4, 6, 9, 15, 16]   # n = 2 | 5, dyadic rows | 8, 11: arange's extra node | 16: one full block | 17: two


def edge_cases(kind):
    """The cases of tests/golden/loss_edges.npz (gen_golden_loss_edges.py): kind implicit, explicit or iou."""
    from _golden import load
    d = load("loss_edges.npz")
    out = []
    for i in range(int(d["%s_n" % kind])):
        pre = "%s_c%d_" % (kind, i)
        out.append({k[len(pre):]: d[k] for k in d.files if k.startswith(pre)})
    return out


def implicit_case(R, H, W, B):
    dyadic = B == 3
    # R = 3: at sharpness 260 most draws leave every node of so coarse a grid so far from the surface that all
    # 17 moments underflow; this draw has a node near it (at R = 2 no row of the distribution has one)
    rng = np.random.default_rng(16 if R == 3 else 1000 * R + 10 * H + B)
    pred = dyadic_rows() if dyadic else sample(rng, B)
    return dict(name="%sR%d_%dx%d_B%d" % ("dyadic_" if dyadic else "", R, H, W, B), R=R, H=H, W=W, B=B, pred=pred,
                true=signed_target(pred, R, H, W, rng), tau=TAU, s=SHARP)


def explicit_case(R):
    rng = np.random.default_rng(7000 + R)
    if R == 4:
        true, pred = dyadic_rows(a=(0.5, 0.25, 0.25), t=(0.5, 0.5, 0.5)), dyadic_rows()
    else:
        true, pred = sample(rng, 2), sample(rng, 2)
    return dict(name="R%d" % R, R=R, B=len(pred), true=true, pred=pred)
