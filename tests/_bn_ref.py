"""Float64 references of the BatchNorm link kernels (sqr_bn.hip, sqr_bn_dev.h), plain torch on the
CPU.  Activations are [M, C] (M = N*H*W pixels, NHWC order) unless a name says NCHW.  Proven against
float64 nn.BatchNorm2d autograd in test_bn_ref_cpu.py before any GPU test relies on them."""
import torch

F64 = torch.float64


def _f32(v):
    """A Python float rounded to f32 (how the C ABI receives momentum and eps)."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def _row_sizes(M, rows):
    if isinstance(rows, int):  # torch.chunk's split: ceil(M / rows) pixels per row, the last one shorter
        per = -(-M // rows)
        sizes = [min(per, M - p) for p in range(0, M, per)]
    else:
        sizes = [int(r) for r in rows]
    assert sum(sizes) == M and min(sizes) >= 1, (M, sizes)
    return sizes


def partial_rows_fwd(x_nhwc, rows, dtype=torch.float32):
    """(buf, nrows): the forward statistics partials of x [M, C] as a stats-producing conv epilogue
    hands them to the BatchNorm: nrows Welford rows [nrows, 2, C] = (mean_t, M2_t = sum (x - mean_t)^2)
    over consecutive disjoint pixel sets, computed in float64 and stored as `dtype`, followed in the
    same flat buffer by the rows' pixel counts.  rows: a row count (split as torch.chunk) or the list
    of row sizes (unequal sizes and one-pixel rows allowed)."""
    x = x_nhwc.detach().to(F64).reshape(-1, x_nhwc.shape[-1])
    sizes = _row_sizes(x.shape[0], rows)
    out, p = [], 0
    for n in sizes:
        c = x[p:p + n]
        mu = c.mean(0)
        out.append(torch.stack([mu, ((c - mu) ** 2).sum(0)]))
        p += n
    parts = torch.stack(out).to(dtype)
    cnt = torch.tensor([float(n) for n in sizes], dtype=dtype)
    return torch.cat([parts.reshape(-1), cnt]), len(sizes)


def rows_view(buf, nrows, C):
    """([nrows, 2, C] rows, [nrows] counts) of a partial_rows_fwd buffer."""
    return buf[:nrows * 2 * C].view(nrows, 2, C), buf[nrows * 2 * C:nrows * 2 * C + nrows]


def merge_fwd(rows, counts, M, gamma, beta, rm, rv, momentum, eps, dtype=torch.float32):
    """fwd_finalize_kernel: Chan's merge, in float64, of the rows as given --
        mean = sum_t n_t mean_t / M,   M2 = sum_t (M2_t + n_t (mean_t - mean)^2)
    -- then invstd from the biased variance M2 / M, coef = [scale | shift] and the running statistics
    (unbiased variance), everything rounded to `dtype` once at the end.  gamma / beta None: 1 / 0;
    rm / rv None: no running statistics (new_rm = new_rv = None).
    Returns (mean, invstd, coef, new_rm, new_rv)."""
    r = rows.detach().to(F64)
    n = counts.detach().to(F64)[:, None]
    C = r.shape[2]
    mean = (n * r[:, 0]).sum(0) / M
    m2 = (r[:, 1] + n * (r[:, 0] - mean) ** 2).sum(0)
    var = (m2 / M).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + _f32(eps))
    g = gamma.detach().to(F64) if gamma is not None else torch.ones(C, dtype=F64)
    b = beta.detach().to(F64) if beta is not None else torch.zeros(C, dtype=F64)
    coef = torch.cat([g * invstd, b - mean * g * invstd])
    new_rm = new_rv = None
    if rm is not None:
        mom = _f32(momentum)
        unb = var * M / (M - 1) if M > 1 else var
        new_rm = ((1.0 - mom) * rm.detach().to(F64) + mom * mean).to(dtype)
        new_rv = ((1.0 - mom) * rv.detach().to(F64) + mom * unb).to(dtype)
    return mean.to(dtype), invstd.to(dtype), coef.to(dtype), new_rm, new_rv


def apply_fwd(x, coef, residual=None):
    """x * scale + shift (+ residual) in float64, before any ReLU."""
    C = x.shape[-1]
    c = coef.detach().to(F64)
    y = x.detach().to(F64) * c[:C] + c[C:2 * C]
    return y + residual.detach().to(F64) if residual is not None else y


def _g(dy, mask_bits):
    g = dy.detach().to(F64)
    return g * mask_bits.to(F64) if mask_bits is not None else g


def bwd_sums(dy, mask_bits, x, mean):
    """(sum g, sum g * (x - mean)) per channel in float64, g = dy * bit (mask_bits None: no ReLU)."""
    g = _g(dy, mask_bits)
    return g.sum(0), (g * (x.detach().to(F64) - mean.detach().to(F64))).sum(0)


def bwd_sums2(dy, mask_bits, xa, mean_a, xb, mean_b):
    """The two-input variant (kind 2): (sum g, sum g * (xa - mean_a), sum g * (xb - mean_b))."""
    g = _g(dy, mask_bits)
    return (g.sum(0), (g * (xa.detach().to(F64) - mean_a.detach().to(F64))).sum(0),
            (g * (xb.detach().to(F64) - mean_b.detach().to(F64))).sum(0))


def bwd_finalize(sg, sgx, M, gamma, mean, invstd):
    """bn_bwd_finalize_w in float64: (dgamma, dbeta, coef = [k1 | k2 | k3]) with
        k1 = gamma * invstd,  k3 = -k1 * invstd^2 * sgx / M,  k2 = -k1 * sg / M - k3 * mean
    so that dx = k1 * g + k3 * x + k2.  gamma None: 1."""
    sg, sgx = sg.to(F64), sgx.to(F64)
    inv, mu = invstd.detach().to(F64), mean.detach().to(F64)
    gm = gamma.detach().to(F64) if gamma is not None else torch.ones_like(inv)
    k1 = gm * inv
    k3 = -k1 * inv * inv * sgx / M
    k2 = -k1 * sg / M - k3 * mu
    return sgx * inv, sg.clone(), torch.cat([k1, k2, k3])


def bwd_dx(coef, dy, mask_bits, x):
    """dx = k1 * g + k3 * x + k2 in float64."""
    C = x.shape[-1]
    c = coef.detach().to(F64)
    return c[:C] * _g(dy, mask_bits) + c[2 * C:3 * C] * x.detach().to(F64) + c[C:2 * C]


def pack_mask(keep):
    """uint8 [M * C / 8]: 1 bit per element in NHWC order, bit i of byte v = channel 8v + i of the
    pixel.  keep: [N, C, H, W] (NCHW) or [M, C] booleans."""
    if keep.dim() == 4:
        keep = keep.permute(0, 2, 3, 1)
    C = keep.shape[-1]
    assert C % 8 == 0
    bits = keep.reshape(-1, 8).to(torch.int64)
    w = 2 ** torch.arange(8, dtype=torch.int64, device=bits.device)
    return (bits * w).sum(1).to(torch.uint8)


def unpack_mask(mask, C):
    """The inverse: [M, C] booleans of a packed mask."""
    m = mask.reshape(-1, 1).to(torch.int64)
    bits = (m >> torch.arange(8, dtype=torch.int64, device=mask.device)) & 1
    return bits.reshape(-1, C).bool()
