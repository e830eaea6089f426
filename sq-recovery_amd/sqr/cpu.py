"""Host-CPU implementation of the losses for CPU tensors (BASELINE config 1: train.py on the CPU,
fp32 network, float64 loss) — the device choice of the caller, never a substitute for the GPU path:
CUDA tensors always go to libsqr's kernels, and a missing libsqr raises there.

Same math and float64 arithmetic as the reference, batched over the samples instead of the
reference's per-sample Python loop, with autograd for the gradient:
  inside_outside  torch/classes.py:138-189 (ExplicitLoss.occupancy core), :232-274 (ImplicitLoss),
                  :394-426 (IoUAccuracy.ins_outs: no clamp, no zero fix)
  implicit_loss   torch/classes.py:232-295 (depth_projection + nearest resize + MAE)
  explicit_loss   torch/classes.py:138-201 (occupancy MSE x 100)
  iou_counts      torch/classes.py:428-447
Pinned to the reference's own outputs by tests/test_cpu_path.py (tests/golden/*.npz).
"""
import numpy as np
import torch
import torch.nn.functional as F


def grid(axis, zero_fix):
    """[3, n, n, n] float64 meshgrid ('ij') of a 1-D axis; exact zeros -> 1e-4 when zero_fix
    (classes.py:126, :221)."""
    ax = torch.as_tensor(np.asarray(axis, dtype=np.float64))
    g = torch.stack(torch.meshgrid([ax, ax, ax], indexing="ij"))
    if zero_fix:
        g = torch.where(g == 0, g + 1e-4, g)
    return g


def implicit_axis(R):
    return np.linspace(0, 1, R).astype(np.float64)  # classes.py:217


def explicit_axis(R):
    step = 1 / R
    return np.arange(0, 1 + step, step).astype(np.float64)  # classes.py:122


def _clamp(p):
    a, e, t, q = torch.split(p, (3, 2, 3, 4), dim=-1)
    return a.clamp(0.05, 1), e.clamp(0.1, 1), t.clamp(0, 1), q


def _rot_conj(q):
    """mat_from_quaternion(conjugate(q)) for a batch [B, 4] -> [B, 3, 3] (quaternion.py:19-67)."""
    x, y, z, w = -q[:, 0], -q[:, 1], -q[:, 2], q[:, 3]
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
            2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
            2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, dim=-1).reshape(-1, 3, 3)


def inside_outside(p, xyz, clamp=True, zero_fix=True):
    """G [B, n, n, n] of parameters p [B, 12] on the grid xyz [3, n, n, n] (float64)."""
    p = p.double()
    if clamp:
        a, e, t, q = _clamp(p)
    else:
        a, e, t, q = torch.split(p, (3, 2, 3, 4), dim=-1)
    rot = _rot_conj(q)
    tr = torch.einsum("bij,bj->bi", rot, t)
    cs = torch.einsum("bij,jxyz->bixyz", rot, xyz)
    u = (cs - tr[:, :, None, None, None]) / a[:, :, None, None, None]
    sq = torch.pow(u, 2)
    if zero_fix:
        sq = torch.where(sq == 0, sq + 1e-4, sq)
    e1, e2 = e[:, 0, None, None, None], e[:, 1, None, None, None]
    A = torch.pow(sq[:, 0], 1 / e2)
    B = torch.pow(sq[:, 1], 1 / e2)
    C = torch.pow(sq[:, 2], 1 / e1)
    E = torch.pow(A + B, e2 / e1)
    return torch.pow(E + C, e1)


def render(pred, R, tau, sharpness, xyz=None):
    """depth_projection (classes.py:232-282): [B, R, R] float64 in image orientation."""
    xyz = grid(implicit_axis(R), True) if xyz is None else xyz
    occ = torch.sigmoid(sharpness * (1 - inside_outside(pred, xyz)))
    T = torch.exp(-tau * torch.cumsum(occ.flip(dims=[-1]), dim=-1))
    depth = 1 - T.sum(dim=-1) / R
    return depth.permute(0, 2, 1).flip(dims=(1,))


def implicit_loss(true, pred, R, tau, sharpness, xyz=None):
    """ImplicitLoss.__call__ (classes.py:284-295): 0-d float64."""
    tr = F.interpolate(true, size=(R, R), mode="nearest")
    d = render(pred, R, tau, sharpness, xyz).unsqueeze(1)
    return torch.abs(tr - d).mean(dim=(1, 2, 3)).mean()


def explicit_loss(true, pred, R, xyz=None):
    """ExplicitLoss.__call__ (classes.py:191-201): 0-d float64, gradient to pred only."""
    xyz = grid(explicit_axis(R), True) if xyz is None else xyz
    oa = torch.sigmoid(5 * (1 - inside_outside(true, xyz)))
    ob = torch.sigmoid(5 * (1 - inside_outside(pred, xyz)))
    return (torch.pow(oa - ob, 2).mean(dim=(1, 2, 3)) * 100).mean()


def iou_counts(true, pred, R):
    """[B, 2] int64 (intersection, union) voxel counts of IoUAccuracy (classes.py:394-447)."""
    xyz = grid(implicit_axis(R), False)
    a = inside_outside(true, xyz, clamp=False, zero_fix=False) <= 1
    b = inside_outside(pred, xyz, clamp=False, zero_fix=False) <= 1
    return torch.stack([(a & b).sum(dim=(1, 2, 3)), (a | b).sum(dim=(1, 2, 3))], dim=1)


# ------------------------------------------------------------------------------ scanner depth render
# The reference's depth images come from its prebuilt `data/scanner` binary (helpers.py:27-39).  What it
# computes, pinned to the ten example images (tests/test_scan_render_cpu.py): an orthographic hard depth
# map.  Pixel (r, c) of an S x S image looks down the ray x = c / (S - 1), y = (S - 1 - r) / (S - 1); its value
# is z_top, the largest z with F(x, y, z) <= 1 (0 where the ray misses the body), F the inside-outside
# function above without the zero fix, the parameters clamped and the quaternion normalised.
#
# Along a ray the local coordinates are u_i = al_i + be_i z.  f = (|u0|^(2/e2) + |u1|^(2/e2))^(e2/e1) +
# |u2|^(2/e1) = F^(1/e1) is convex in z for e <= 1, so the inside set of a ray is one interval inside the slab
# |u_i| <= 1: bisect on the sign of df/dz for a point with f <= 1 (none: a miss), then bisect on f <= 1
# between that point and the slab's upper end.  Everything is evaluated as log2 f (no pow can overflow; a
# term with u_i = 0 is an exact 0, log2 = -inf).  libsqr's scan_render_kernel is the same procedure in fp32.
_SCAN_ZLO, _SCAN_ZHI = -3.0, 4.0  # a >= 0.05, t in [0, 1], |u| <= 1: the body lies in z in [-sqrt 3, 1 + sqrt 3]
_SCAN_FMIN_BOX = 1.25  # return_fmin minimises F over the slab |u_i| <= 1.25; outside it F >= 1.25^2


def _scan_iters(dtype):
    """(minimum search, root search) bisection steps: the bracket, at most 7 wide, down to the dtype's ulp."""
    return (26, 28) if dtype == torch.float32 else (50, 56)


def _scan_lse2(x, y):
    """log2(2^x + 2^y) and the two shares 2^x / (2^x + 2^y), 2^y / (...); (-inf, -inf) -> (-inf, 0, 0)."""
    m = torch.maximum(x, y)
    none = torch.isneginf(m)
    e = torch.exp2(torch.where(none, torch.zeros_like(m), torch.minimum(x, y) - m))
    big = 1 / (1 + e)
    small = e * big
    zero = torch.zeros_like(m)
    sx = torch.where(none, zero, torch.where(x >= y, big, small))
    sy = torch.where(none, zero, torch.where(x >= y, small, big))
    return m + torch.log2(1 + e), sx, sy


class _ScanRays:
    """The rays of S x S pixels of B samples, flattened: al, be [3, N], the exponents per ray."""

    def __init__(self, params, size, dtype):
        p = params.detach().to("cpu").to(dtype)
        if p.dim() != 2 or p.shape[1] != 12:
            raise ValueError("params must be [B,12], got %s" % (tuple(p.shape),))
        if size < 2:
            raise ValueError("scan_render: size=%d must be >= 2" % size)
        B, S = p.shape[0], int(size)
        qmax = p[:, 8:12].abs().amax(dim=1)
        self.valid = torch.isfinite(p).all(dim=1) & (qmax > 0)  # else: a zero image
        unit = torch.tensor([0.5, 0.5, 0.5, 1, 1, 0.5, 0.5, 0.5, 0, 0, 0, 1], dtype=dtype)
        p = torch.where(self.valid[:, None], p, unit[None])
        a, e, t, q = _clamp(p)
        q = q / q.abs().amax(dim=1, keepdim=True)  # scaled first: the squares cannot over/underflow
        q = q / torch.sqrt((q * q).sum(dim=1, keepdim=True))  # helpers.quat2mat normalises
        M = _rot_conj(q)
        ax = torch.arange(S, dtype=dtype) / (S - 1)
        dx = ax[None, None, :] - t[:, 0, None, None]  # x = c / (S - 1)
        dy = ax.flip(0)[None, :, None] - t[:, 1, None, None]  # y = (S - 1 - r) / (S - 1)
        al, be = [], []
        for i in range(3):
            c = M[:, i, 0, None, None] * dx + M[:, i, 1, None, None] * dy - (M[:, i, 2] * t[:, 2])[:, None, None]
            al.append((c / a[:, i, None, None]).reshape(-1))
            be.append((M[:, i, 2] / a[:, i])[:, None, None].expand(B, S, S).reshape(-1))
        self.B, self.S, self.dtype = B, S, dtype
        self.al, self.be = torch.stack(al), torch.stack(be)
        per_ray = lambda v: v[:, None, None].expand(B, S, S).reshape(-1)  # noqa: E731
        self.e1 = per_ray(e[:, 0])
        self.i2e1, self.i2e2, self.r21 = per_ray(2 / e[:, 0]), per_ray(2 / e[:, 1]), per_ray(e[:, 1] / e[:, 0])
        self.ok = per_ray(self.valid)

    def take(self, idx):
        r = object.__new__(_ScanRays)
        r.al, r.be = self.al[:, idx], self.be[:, idx]
        r.e1, r.i2e1, r.i2e2, r.r21 = self.e1[idx], self.i2e1[idx], self.i2e2[idx], self.r21[idx]
        return r

    def slab(self, box=1.0):
        """[z0, z1] of |u_i| <= box clipped to the body's z range, and hit = the interval is not empty."""
        z0 = torch.full_like(self.al[0], _SCAN_ZLO)
        z1 = torch.full_like(self.al[0], _SCAN_ZHI)
        hit = self.ok.clone()
        for i in range(3):
            al, be = self.al[i], self.be[i]
            flat = be == 0  # the ray runs along the slab: inside it everywhere or nowhere
            hit &= ~(flat & (al.abs() > box))
            safe = torch.where(flat, torch.ones_like(be), be)
            za, zb = (-box - al) / safe, (box - al) / safe
            z0 = torch.where(flat, z0, torch.maximum(z0, torch.minimum(za, zb)))
            z1 = torch.where(flat, z1, torch.minimum(z1, torch.maximum(za, zb)))
        return z0, z1, hit & (z0 <= z1)

    def eval(self, z):
        """log2 f at depth z of every ray, and a value with the sign of df/dz."""
        u = self.be * z + self.al
        lu = torch.log2(u.abs())
        lA, lB, lC = lu[0] * self.i2e2, lu[1] * self.i2e2, lu[2] * self.i2e1
        l1, sA, sB = _scan_lse2(lA, lB)
        lf, sE, sC = _scan_lse2(self.r21 * l1, lC)  # r21 > 0: -inf stays -inf
        g = torch.where(u != 0, self.be / torch.where(u != 0, u, torch.ones_like(u)), torch.zeros_like(u))
        return lf, sE * (sA * g[0] + sB * g[1]) + sC * g[2]

    def minimise(self, lo, hi, iters):
        """Bisection on the sign of df/dz; the probe with the smallest log2 f and that value."""
        zb = 0.5 * (lo + hi)
        lb = torch.full_like(lo, float("inf"))
        for _ in range(iters):
            mid = 0.5 * (lo + hi)
            lf, d = self.eval(mid)
            better = lf < lb
            zb, lb = torch.where(better, mid, zb), torch.where(better, lf, lb)
            up = d > 0  # f rises: the minimum lies below
            lo, hi = torch.where(up, lo, mid), torch.where(up, mid, hi)
        return zb, lb


def scan_inside_outside(params, size, z, dtype=torch.float64):
    """F and dF/dz at depth z [B, S, S] of every pixel's ray (the quantities scan_render solves F = 1 for)."""
    rays = _ScanRays(params, size, dtype)
    lf, d = rays.eval(torch.as_tensor(z).detach().to("cpu").to(dtype).reshape(-1))
    F = torch.exp2(rays.e1 * lf)
    shape = (rays.B, rays.S, rays.S)
    return F.reshape(shape), (F * rays.e1 * rays.i2e1 * d).reshape(shape)  # d ln f / dz = (2 / e1) d


def scan_render(params, size=256, levels=255, dtype=torch.float64, return_fmin=False):
    """Scanner-style hard depth images [B, size, size] in [0, 1] of parameters [B, 12] (`dtype` arithmetic;
    float64 parameters are used as given).  levels > 0 quantises to floor(levels z) / levels (255: the
    scanner's 8-bit image / 255); levels = 0 keeps the continuous depth.  A sample with a non-finite
    parameter or an all-zero quaternion renders as zeros.  return_fmin: also the minimum of F along each
    ray (rays that miss the box |u_i| <= 1.25 report its bound there, 1.25^2)."""
    if levels < 0:
        raise ValueError("scan_render: levels=%d must be >= 0" % levels)
    rays = _ScanRays(params, size, dtype)
    n1, n2 = _scan_iters(dtype)
    depth = torch.zeros(rays.B * rays.S * rays.S, dtype=dtype)
    z0, z1, hit = rays.slab()
    idx = torch.nonzero(hit).reshape(-1)
    if idx.numel():
        sub = rays.take(idx)
        top = z1[idx]
        zin, lin = sub.minimise(z0[idx], top, n1)
        lo, hi = zin, top
        for _ in range(n2):  # f(lo) <= 1 < f(hi): the upper root of f = 1
            mid = 0.5 * (lo + hi)
            inside = sub.eval(mid)[0] <= 0
            lo, hi = torch.where(inside, mid, lo), torch.where(inside, hi, mid)
        zt = 0.5 * (lo + hi)
        zt = torch.where((lin <= 0) & (zt > 0), zt.clamp(0, 1), torch.zeros_like(zt))
        depth[idx] = torch.floor(levels * zt) / levels if levels > 0 else zt
    depth = depth.reshape(rays.B, rays.S, rays.S)
    if not return_fmin:
        return depth
    fmin = torch.full((rays.B * rays.S * rays.S,), _SCAN_FMIN_BOX ** 2, dtype=dtype)
    w0, w1, near = rays.slab(_SCAN_FMIN_BOX)
    near |= ~rays.ok  # (a zero image's rays: the stand-in body's values, of no meaning)
    idx = torch.nonzero(near & (w0 <= w1)).reshape(-1)
    if idx.numel():
        sub = rays.take(idx)
        fmin[idx] = torch.exp2(sub.e1 * sub.minimise(w0[idx], w1[idx], n1)[1])
    return depth, fmin.reshape(rays.B, rays.S, rays.S)


# ---------------------------------------------------------------- the online label sampler (sqr_sq_sample)
_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32-10 over arrays: counter = four uint32-valued arrays of one shape, key = two Python ints;
    returns the four output words as uint64 arrays holding 32-bit values."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _U32 for c in counter)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _PHILOX_M0 * c0, _PHILOX_M1 * c2  # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _U32, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _U32
        k0, k1 = (k0 + _PHILOX_W0) & 0xFFFFFFFF, (k1 + _PHILOX_W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def sq_sample_raw(position, n, seed=0, substream=0):
    """The [n, 12] uint32 words of samples position .. position + n - 1 (modulo 2^64) of `substream` under
    `seed`: three Philox calls per sample, counter (i_lo, i_hi, call, substream), key (seed_lo, seed_hi)."""
    seed, position = int(seed) & (2 ** 64 - 1), int(position) & (2 ** 64 - 1)
    i = np.uint64(position) + np.arange(n, dtype=np.uint64)  # wraps modulo 2^64
    lo, hi = i & _U32, i >> _S32
    sub = np.full(n, int(substream) & 0xFFFFFFFF, dtype=np.uint64)
    words = []
    for call in range(3):
        words.extend(philox4x32_10((lo, hi, np.full(n, call, dtype=np.uint64), sub), (seed, seed >> 32)))
    return np.stack(words, 1).astype(np.uint32)


def sq_uniforms(raw):
    """u_j = (w_j >> 8) 2^-24 of the first eleven words: [n, 11] float64, each exactly a float32."""
    return (np.asarray(raw)[:, :11] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def sq_labels(u):
    """[n, 12] float32 labels [a(3), e(2), t(3), q(4)] of [n, 11] uniforms (float64 arithmetic, one rounding):
    the distribution of classes.sample_sq_params."""
    u = np.asarray(u, dtype=np.float64)
    r1, r2 = np.sqrt(1.0 - u[:, 8]), np.sqrt(u[:, 8])
    a1, a2 = 2.0 * np.pi * u[:, 9], 2.0 * np.pi * u[:, 10]
    q = np.stack([r1 * np.sin(a1), r1 * np.cos(a1), r2 * np.sin(a2), r2 * np.cos(a2)], 1)
    return np.concatenate([(25.0 + 50.0 * u[:, 0:3]) / 255.0, 0.1 + 0.9 * u[:, 3:5],
                           (88.0 + 80.0 * u[:, 5:8]) / 255.0, q], 1).astype(np.float32)


def sq_sample(position, n, seed=0, substream=0):
    """Host restatement of sqr_sq_sample: the [n, 12] float32 labels of samples position .. position + n - 1."""
    return sq_labels(sq_uniforms(sq_sample_raw(position, n, seed, substream)))
