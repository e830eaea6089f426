"""Shared cases of the scanner-render tests (tests/test_scan_render_cpu.py, tests/test_scan_render_gpu.py):
the ten example images, closed forms for axis-aligned bodies, the edge-case parameter rows and the
conditions that pin a render to the scanner's own images."""
import numpy as np

from _golden import load

# caps of the comparison with the scanner's ten images; the float64 restatement of the rule measures
# 17 / 0.990 / 1 / 11 against them
MAX_EXTRA, MIN_EXTRA_FMIN, MAX_LEVEL_DIFF, MAX_DIFFERING = 24, 0.98, 1, 16

EXPONENTS = [(0.1, 0.1), (1.0, 1.0), (0.1, 1.0), (1.0, 0.1), (0.38, 0.37)]
CF_SIZE = 64
CF_A = (0.3, 0.25, 0.35)
CF_T = (32 / 63, 31 / 63, 0.5)  # pixel (r, c) = (32, 32) of a 64^2 image looks down the local z axis
AXIS_PIXEL = (32, 32)
QUAT_ID = (0.0, 0.0, 0.0, 1.0)
QUAT_X90 = (np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5))  # R = [[1,0,0],[0,0,-1],[0,1,0]]


# Tolerances of the closed-form comparison with the float64 host render.  The host bisects z down to
# 7 * 2^-56 < 1e-15.  The closed form's own float64 error is eps amplified by d z / d bracket =
# (e/2) a bracket^(e/2 - 1), unbounded towards the silhouette (bracket -> 0); with bracket >= 1e-6 and
# e >= 0.1 it stays below 1e-16 * 1e-6^-0.95 < 1e-10.  Pixels with |bracket| < 1e-6 may fall on either side.
CF_TOL, CF_EDGE = 1e-9, 1e-6


def fixture():
    d = load("example_images.npz")
    return d["labels"].astype(np.float32), d["images"]


def to_levels(img, levels=255):
    """A levels-quantised render in [0, 1] -> integer grey levels."""
    return np.rint(np.asarray(img, dtype=np.float64) * levels).astype(np.int64)


def scanner_caps(render_levels, image, fmin):
    """The four conditions on one rendered image (integer levels) against the scanner's; returns the counts
    (missed, extra, min F-min of the extra pixels, max level difference, differing) after asserting them."""
    image = image.astype(np.int64)
    fg_s, fg_r = image > 0, render_levels > 0
    missed = int((fg_s & ~fg_r).sum())
    extra = fg_r & ~fg_s
    extra_fmin = float(fmin[extra].min()) if extra.any() else float("inf")
    diff = np.abs(render_levels - image)[fg_s & fg_r]
    counts = (missed, int(extra.sum()), extra_fmin, int(diff.max()), int((diff > 0).sum()))
    print("scanner parity: missed %d extra %d (min F-min %.4f) max diff %d differing %d of %d"
          % (counts + (int((fg_s & fg_r).sum()),)))
    assert missed == 0
    assert counts[1] <= MAX_EXTRA and extra_fmin >= MIN_EXTRA_FMIN
    assert counts[3] <= MAX_LEVEL_DIFF
    assert counts[4] <= MAX_DIFFERING
    return counts


def closed_form_params(e, quat):
    """float64 [1,12] row of the closed-form body with exponents e = (e1, e2)."""
    return np.array([list(CF_A) + list(e) + list(CF_T) + list(quat)], dtype=np.float64)


def closed_form(e, rotated):
    """(z_top [S,S], bracket [S,S]) in float64 for closed_form_params(e, QUAT_X90 if rotated else QUAT_ID):
    z_top holds where bracket >= 0, the ray misses where bracket < 0.
      identity:  z = t2 + a2 (1 - (|u0|^(2/e2) + |u1|^(2/e2))^(e2/e1))^(e1/2),  u_i = (x_i - t_i) / a_i
      90 deg about x (local axes (x, z, -y)):
                 z = t2 + a1 ((1 - |u2|^(2/e1))^(e1/e2) - |u0|^(2/e2))^(e2/2),  u0 = dx / a0, u2 = -dy / a2"""
    e1, e2 = e
    S = CF_SIZE
    ax = np.arange(S, dtype=np.float64) / (S - 1)
    x = ax[None, :] - CF_T[0]
    y = ax[::-1][:, None] - CF_T[1]
    with np.errstate(invalid="ignore"):
        if not rotated:
            u0, u1 = np.abs(x / CF_A[0]), np.abs(y / CF_A[1])
            br = 1 - (u0 ** (2 / e2) + u1 ** (2 / e2)) ** (e2 / e1)
            z = CF_T[2] + CF_A[2] * np.maximum(br, 0) ** (e1 / 2)
        else:
            u0, u2 = np.abs(x / CF_A[0]), np.abs(y / CF_A[2])
            inner = 1 - u2 ** (2 / e1)
            br = np.where(inner >= 0, np.maximum(inner, 0) ** (e1 / e2) - u0 ** (2 / e2), -1.0)
            z = CF_T[2] + CF_A[1] * np.maximum(br, 0) ** (e2 / 2)
    return z, br + np.zeros((S, S))


def closed_form_cases():
    """(name, float64 params [1,12], z_top, bracket) of the ten closed-form bodies."""
    out = []
    for e in EXPONENTS:
        for rotated in (False, True):
            z, br = closed_form(e, rotated)
            out.append(("e%s_%s" % (e, "x90" if rotated else "id"),
                        closed_form_params(e, QUAT_X90 if rotated else QUAT_ID), z, br))
    return out


BASE = [0.2, 0.25, 0.3, 0.5, 0.7, 0.5, 0.45, 0.55, 0.1, 0.2, 0.3, 0.927]


def edge_rows():
    """name -> float64 [12] rows of the edge cases (shared by the host and the kernel tests; the host takes
    them as they are, so that "clamped" holds the clamps' own bounds; the kernel takes them as float32,
    where its bounds 0.05f and 0.1f are the rounded rows' values)."""
    rows = {"base": BASE}
    rows["unclamped"] = [1.5, 0.01, 0.3, 0.05, 2.0, -0.2, 1.3, 0.5] + BASE[8:]
    rows["clamped"] = [1.0, 0.05, 0.3, 0.1, 1.0, 0.0, 1.0, 0.5] + BASE[8:]
    rows["q_times_4"] = BASE[:8] + [4 * v for v in BASE[8:]]
    rows["q_times_1p7"] = BASE[:8] + [1.7 * v for v in BASE[8:]]
    n = float(np.sqrt(sum(v * v for v in BASE[8:])))
    rows["q_unit"] = BASE[:8] + [v / n for v in BASE[8:]]
    rows["above_one"] = [0.2, 0.2, 0.3, 0.6, 0.6, 0.5, 0.5, 0.9] + list(QUAT_ID)  # t2 + a2 = 1.2
    rows["off_frame"] = [0.3, 0.2, 0.25, 0.4, 0.9, 0.05, 0.95, 0.5] + BASE[8:]
    rows["nan"] = BASE[:4] + [float("nan")] + BASE[5:]
    rows["inf"] = [float("inf")] + BASE[1:]
    rows["q_zero"] = BASE[:8] + [0.0, 0.0, 0.0, 0.0]
    return {k: np.array(v, dtype=np.float64) for k, v in rows.items()}
