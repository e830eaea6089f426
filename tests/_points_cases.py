"""Point lists for the sqr_pts_* tests: the golden clouds (tests/golden/points.npz), subsets of them, clouds that
leave the unit cube, and the list that is an image's resized pixels in pixel order."""
import numpy as np
import torch
import torch.nn.functional as F

from _golden import load


def golden():
    return load("points.npz")


def image_list(true, R):
    """true [B,1,H,W] f32 -> points [B,R*R,3] f32: slot r R + c = (c / R, 1 - r / R, z) with x and y formed in
    float32 as classes.LeastSquares.batch_points forms them, z the nearest-resized pixel, and NaN in all three
    where the pixel is not > 0 (a NaN pixel included)."""
    t = torch.as_tensor(np.asarray(true, np.float32))
    if t.dim() == 3:
        t = t[:, None]
    z = F.interpolate(t, size=(R, R), mode="nearest")[:, 0]
    rows, cols = torch.meshgrid(torch.arange(R), torch.arange(R), indexing="ij")
    x = (cols.float() / R).expand_as(z)
    y = (1 - rows.float() / R).expand_as(z)
    pts = torch.stack([x, y, z], dim=-1).reshape(t.shape[0], R * R, 3)
    on = (z > 0).reshape(t.shape[0], R * R, 1)
    return torch.where(on, pts, torch.full_like(pts, float("nan"))).contiguous().numpy()


def subset(cloud, P):
    """P of the cloud's points, spread evenly over its slots (P <= len(cloud): no slot twice)."""
    idx = np.linspace(0, len(cloud) - 1, P).round().astype(np.int64)
    assert len(np.unique(idx)) == P
    return np.ascontiguousarray(cloud[idx])


SHIFT = np.array([-0.45, 0.0, -0.45], np.float32)  # moves about half of a golden cloud to x < 0 and to z < 0


def accuracy_case(P, seed=20261021):
    """The normal equations' accuracy case at P slots: twelve clouds and one parameter row each.
      0..7   the golden clouds' subsets, their labels perturbed by N(0, 0.03)
      8, 9   golden clouds 0 and 1 shifted by SHIFT (coordinates outside [0,1], z < 0), the labels shifted along
             (t leaves [0,1] where the body does: clamped) and perturbed
      10, 11 golden clouds 2 and 3 again with a row outside its clamps: a0 = 1.2, and e0 = 0.05 with t0 = -0.1
    At the label itself the energy is all cancellation (1e-13) and a relative error means nothing, hence the
    perturbation.  -> (points [12,P,3] f32, params [12,12] f32)."""
    d = golden()
    rng = np.random.default_rng(seed + P)
    clouds = [subset(c, P) for c in d["clouds"]]
    labels = d["labels"].astype(np.float32)
    pts = clouds + [clouds[0] + SHIFT, clouds[1] + SHIFT, clouds[2], clouds[3]]
    lab = np.concatenate([labels, labels[[0, 1, 2, 3]]]).astype(np.float64)
    lab[8:10, 5:8] += SHIFT
    par = lab + 0.03 * rng.normal(size=lab.shape)
    par[10, 0] = 1.2
    par[11, 3], par[11, 5] = 0.05, -0.1
    return np.stack(pts).astype(np.float32), par.astype(np.float32)


def normal_eq_ref(points, params, dt, keep=None):
    """tests/_lm_ref.normal_eq_one per sample on the CPU in dtype dt -> float64 numpy (H [S,12,12], g [S,12], E [S]).
    points [S,P,3] f32; keep [S,P] bool (optional): the slots that count."""
    import _lm_ref
    out = []
    for s in range(len(params)):
        p = points[s] if keep is None else points[s][keep[s]]
        out.append(_lm_ref.normal_eq_one(torch.tensor(np.ascontiguousarray(p.T)).to(dt), torch.tensor(params[s]).to(dt)))
    return tuple(np.stack([o[i].double().numpy() for o in out]) for i in range(3))


def errs(H, g, E, H64, g64, E64):
    """tests/test_lm_refine_gpu.py's metrics, maxima over the samples: E relative, g over the sample's largest |g|
    entry, H over its largest diagonal entry."""
    n = range(len(E64))
    return (max(abs(E[b] - E64[b]) / E64[b] for b in n),
            max(np.abs(g[b] - g64[b]).max() / np.abs(g64[b]).max() for b in n),
            max(np.abs(H[b] - H64[b]).max() / np.diagonal(H64[b]).max() for b in n))
