"""Scalar reference of the online label sampler in Python ints and math.* floats (float64): Philox4x32-10 and
the label rule of include/sqr.h (sqr_sq_sample), written from the rule alone.  It shares no code with
sqr/cpu.py, whose vectorised sampler and the HIP kernel are both compared against it."""
import math

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
MASK64 = 0xFFFFFFFFFFFFFFFF


def philox(counter, key):
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def words(seed, substream, i):
    """The twelve uint32 words of sample i (an int in [0, 2^64)) of `substream` under `seed`."""
    i &= MASK64
    out = []
    for call in range(3):
        out.extend(philox((i & MASK32, i >> 32, call, substream & MASK32), (seed & MASK32, (seed >> 32) & MASK32)))
    return out


def uniforms(w):
    return [(x >> 8) / 16777216.0 for x in w[:11]]


def labels(u):
    """[a(3), e(2), t(3), q(4)] in float64 from the eleven uniforms."""
    a = [(25.0 + 50.0 * u[j]) / 255.0 for j in range(3)]
    e = [0.1 + 0.9 * u[3 + j] for j in range(2)]
    t = [(88.0 + 80.0 * u[5 + j]) / 255.0 for j in range(3)]
    r1, r2 = math.sqrt(1.0 - u[8]), math.sqrt(u[8])
    a1, a2 = 2.0 * math.pi * u[9], 2.0 * math.pi * u[10]
    return a + e + t + [r1 * math.sin(a1), r1 * math.cos(a1), r2 * math.sin(a2), r2 * math.cos(a2)]


def batch_words(seed, substream, position, n):
    """n rows of words from sample `position` on (positions wrap modulo 2^64)."""
    return [words(seed, substream, position + b) for b in range(n)]
