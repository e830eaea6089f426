"""sqr_scan_render (the scanner-style depth render kernel) against the float64 host renderer with the float32
host renderer as the yardstick, against the scanner's ten example images, its runtime behaviour, and its
consumers on the GPU (SyntheticDataset, gen_dataset.py, test_random.py, train.py --synthetic-render scanner).

Measured on an MI355X (profiles/scan_render_accuracy.txt holds the printed lines): see DESIGN.md.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import _scan_cases as sc
from sqr import cpu

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# a pixel whose z_top lies this close to the plane z = 0 may be foreground in one render and 0 in another
# without its ray grazing the body (fp32 resolves z to 6e-8 there)
Z_PLANE_TOL = 1e-6


def _cases():
    """name -> (float32 params [B,12], S): the issue's five shapes on the fixture labels, the closed-form
    bodies and the edge cases."""
    labels, _ = sc.fixture()
    edge = sc.edge_rows()
    valid = ["base", "unclamped", "clamped", "q_times_4", "q_times_1p7", "q_unit", "above_one", "off_frame"]
    return {
        "S16_B1": (labels[0:1], 16),  # one partly filled block
        "S50_B3": (labels[1:4], 50),  # S not a multiple of any tile
        "S64_B2": (labels[4:6], 64),
        "S256_B10": (labels, 256),  # the fixture
        "S512_B1": (labels[6:7], 512),  # config 5's size; index arithmetic past 256
        "closed_form": (np.concatenate([c[1] for c in sc.closed_form_cases()]).astype(np.float32), sc.CF_SIZE),
        "edge": (np.stack([edge[n] for n in valid]).astype(np.float32), 64),
    }


class _Renders:
    """Per case, computed once and shared: the kernel's renders (continuous and 255 levels), the float64 and
    float32 host renders, and float64 F and dF/dz at the kernel's and the float32 host's depths."""

    def __init__(self):
        from sqr import losses
        self.c = {}
        for name, (p, S) in _cases().items():
            pt = torch.tensor(p)
            pg = pt.to(DEV)
            k0 = losses.scan_render(pg, S, 0).cpu()
            k255 = losses.scan_render(pg, S, 255).cpu()
            h64 = cpu.scan_render(pt, S, 0)
            h32 = cpu.scan_render(pt, S, 0, dtype=torch.float32)
            self.c[name] = dict(p=pt, S=S, k0=k0, k255=k255, h64=h64, h32=h32,
                                Fk=cpu.scan_inside_outside(pt, S, k0.double()),
                                Fh=cpu.scan_inside_outside(pt, S, h32.double()))
        # the yardstick: the float32 host renderer's largest |F - 1| over the whole case set
        self.h32_err = max(self.err(c["h32"], c["Fh"][0]) for c in self.c.values())
        self.bound = 2 * self.h32_err
        self._fmin = {}

    @staticmethod
    def surface(z):
        """pixels that hold a root of F = 1: foreground and not saturated at 1"""
        return (z > 0) & (z < 1)

    @classmethod
    def err(cls, z, F):
        m = cls.surface(z)
        return float((F[m] - 1).abs().max()) if m.any() else 0.0

    def fmin(self, name):
        """float64 minimum of F along every ray of a case (rendered when first asked for)."""
        if name not in self._fmin:
            c = self.c[name]
            self._fmin[name] = cpu.scan_render(c["p"], c["S"], 0, return_fmin=True)[1]
        return self._fmin[name]


@pytest.fixture(scope="module")
def R():
    return _Renders()


CASES = list(_cases())


@pytest.mark.parametrize("name", CASES)
def test_backward_error_and_upper_root(R, name):
    """Every foreground depth the kernel returns satisfies float64 F = 1 to within twice the float32 host
    renderer's worst, and is the upper root (dF/dz >= 0 to the same bound)."""
    c = R.c[name]
    F, dF = c["Fk"]
    m = R.surface(c["k0"])
    assert m.sum() > 20
    err, slope = R.err(c["k0"], F), float(dF[m].min())
    print("scan_render accuracy %-12s kernel max|F-1| %.3e  min dF/dz %.3e  | float32 host max|F-1| %.3e "
          "(this case %.3e)  bound %.3e  pixels %d"
          % (name, err, slope, R.h32_err, R.err(c["h32"], c["Fh"][0]), R.bound, int(m.sum())))
    assert torch.isfinite(c["k0"]).all() and c["k0"].min() >= 0 and c["k0"].max() <= 1
    assert err <= R.bound
    assert slope >= -R.bound


@pytest.mark.parametrize("name", CASES)
def test_silhouette_and_saturation(R, name):
    """Foreground-ness differs from the float64 render only where the ray grazes the body (float64 F-min
    within the bound of 1); pixels saturated at 1 are 1 in both."""
    c = R.c[name]
    k, h = c["k0"].double(), c["h64"]
    differ = (k > 0) != (h > 0)
    near_plane = torch.maximum(k, h) <= Z_PLANE_TOL
    n = int((differ & ~near_plane).sum())
    print("scan_render silhouette %-12s pixels that differ in foreground-ness %d (of %d foreground)"
          % (name, int(differ.sum()), int((h > 0).sum())))
    if n:
        fm = R.fmin(name)[differ & ~near_plane]
        print("    their float64 F-min in [%.9f, %.9f], bound %.3e" % (float(fm.min()), float(fm.max()), R.bound))
        assert ((fm - 1).abs() <= R.bound).all()
    # saturation: where float64 F at z = 1 is clearly inside (or the kernel says 1) both say exactly 1
    F1 = cpu.scan_inside_outside(c["p"], c["S"], torch.ones_like(h))[0]
    sat_h, sat_k = h == 1, k == 1
    assert (k[sat_h & (F1 < 1 - R.bound)] == 1).all()
    assert (F1[sat_k] <= 1 + R.bound).all()
    loose = sat_h & ~sat_k  # float64 saturates, the kernel stops an ulp below: its depth is still a root
    assert (loose <= R.surface(c["k0"])).all()
    if name == "edge":
        assert sat_k[6].any() and (k[6][32, 32] == 1)  # "above_one": t2 + a2 = 1.2


@pytest.mark.parametrize("name", CASES)
def test_quantised_output(R, name):
    """levels = 255: within one level of the float64 render everywhere; no more pixels differ than twice the
    float32 host renderer's count plus 8.  The kernel quantises its own continuous depth."""
    c = R.c[name]
    q64 = torch.floor(255 * c["h64"])  # the host's own quantisation of the same depths
    q32 = torch.floor(255 * c["h32"]).double()
    qk = torch.round(c["k255"].double() * 255)
    dk, dh = (qk - q64).abs(), (q32 - q64).abs()
    print("scan_render quantised %-12s kernel: max level diff %d, differing %d | float32 host: max %d, differing %d"
          % (name, int(dk.max()), int((dk > 0).sum()), int(dh.max()), int((dh > 0).sum())))
    assert torch.equal(c["k255"], torch.floor(255 * c["k0"]) / 255)
    assert dk.max() <= 1
    assert int((dk > 0).sum()) <= 2 * int((dh > 0).sum()) + 8


def test_closed_form_on_the_kernel(R):
    """The closed forms in fp32: the axis ray (two exact-zero terms) is finite and equals t2 + a2 to fp32
    accuracy, and away from the silhouette the depth matches (d z / d bracket <= (e/2) a bracket^(e/2 - 1):
    at bracket >= 1e-2 an F error of the bound moves z by less than 100 bounds)."""
    c = R.c["closed_form"]
    assert torch.isfinite(c["k0"]).all()
    for i, (name, _, z, br) in enumerate(sc.closed_form_cases()):
        got = c["k0"][i].double().numpy()
        inside = br >= 1e-2
        assert np.abs(got - z)[inside].max() <= 100 * R.bound + 1e-6, name
        assert (got[br <= -1e-2] == 0).all(), name
        if name.endswith("id"):
            assert abs(got[sc.AXIS_PIXEL] - (sc.CF_T[2] + sc.CF_A[2])) <= 1e-6, name


def test_edge_cases_on_the_kernel(R):
    k = R.c["edge"]["k0"]  # base, unclamped, clamped, q_times_4, q_times_1p7, q_unit, above_one, off_frame
    assert torch.equal(k[1], k[2]) and (k[2] > 0).any()  # outside the clamps = clamped
    assert torch.equal(k[3], k[0])  # a power-of-two multiple of q: the same bits after normalising
    for j in (4, 5):  # any other multiple: q / |q| to rounding
        same = (k[j] > 0) == (k[0] > 0)
        assert int((~same).sum()) <= 4 and (k[j] - k[0])[same].abs().max() <= 1e-4
    off = k[7]
    assert (off[0] > 0).any() and (off[:, 0] > 0).any()


@pytest.mark.parametrize("bad", ["nan", "inf", "q_zero"])
def test_invalid_row_is_zero_and_leaves_neighbours(bad):
    from sqr import losses
    r = sc.edge_rows()
    rows = torch.tensor(np.stack([r["base"], r[bad], r["off_frame"]]).astype(np.float32), device=DEV)
    img = losses.scan_render(rows, 50, 255)
    alone = losses.scan_render(rows[[0, 2]], 50, 255)
    assert (img[1] == 0).all() and torch.isfinite(img).all()
    assert torch.equal(img[0], alone[0]) and torch.equal(img[2], alone[1]) and (img[0] > 0).any()


@pytest.mark.parametrize("i", range(10))
def test_scanner_parity(R, i):
    """The kernel's 256-level image of fixture label i against the scanner's image i: the host test's caps."""
    _, images = sc.fixture()
    c = R.c["S256_B10"]
    sc.scanner_caps(sc.to_levels(c["k255"][i].numpy()), images[i], R.fmin("S256_B10")[i].numpy())


# ------------------------------------------------------------------------------ runtime behaviour
def _labels(n=10):
    return torch.tensor(sc.fixture()[0][:n], device=DEV)


def test_reproducible_graph_and_stream():
    from sqr import losses
    p = _labels()
    a = losses.scan_render(p, 128, 255)
    assert torch.equal(a, losses.scan_render(p, 128, 255))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = losses.scan_render(p, 128, 255)
    side.synchronize()
    assert torch.equal(a, on_side)
    static = p.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = losses.scan_render(static, 128, 255)
    static.copy_(p.flip(0))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, a.flip(0))


def test_bad_arguments_raise():
    from sqr import _lib, losses
    p = _labels(2)
    with pytest.raises(_lib.SqrError, match="B=0"):
        losses.scan_render(p[:0], 16, 255)
    with pytest.raises(_lib.SqrError, match="S=1"):
        losses.scan_render(p, 1, 255)
    with pytest.raises(_lib.SqrError, match="levels=-1"):
        losses.scan_render(p, 16, -1)
    with pytest.raises(ValueError):
        losses.scan_render(p.cpu(), 16, 255)
    with pytest.raises(ValueError):
        losses.scan_render(p[:, :11], 16, 255)
    L = _lib.lib()
    out = torch.zeros(2, 16, 16, device=DEV)
    assert L.sqr_scan_render(None, 2, 16, 255, ctypes.c_void_p(out.data_ptr()), None) == -1
    assert b"null pointer" in L.sqr_last_error_string()
    assert L.sqr_scan_render(ctypes.c_void_p(p.data_ptr()), 2, 16, 255, None, None) == -1
    torch.cuda.synchronize()
    assert (out == 0).all()


# ------------------------------------------------------------------------------ consumers
def test_synthetic_dataset_scanner_on_the_gpu():
    import classes
    from sqr import losses
    ds = classes.SyntheticDataset(12, DEV, size=128, render="scanner")
    assert ds.images.shape == (12, 1, 128, 128) and ds.images.is_cuda
    assert torch.equal(ds.images[:, 0], losses.scan_render(ds.labels, 128, 255)) and (ds.images > 0).any()
    soft = classes.SyntheticDataset(4, DEV, size=64)
    assert torch.equal(soft.images[:, 0], losses.implicit_render(soft.labels, 64, 1.5, 260))


def test_gen_dataset_on_the_gpu(tmp_path):
    import gen_dataset
    from helpers import parse_csv
    from sqr import losses
    out = str(tmp_path / "set")
    gen_dataset.main(["--n", "6", "--batch", "4", "--out", out, "--seed", "1"])
    parsed = torch.tensor(np.stack(parse_csv(os.path.join(out, "data_labels.csv"))), device=DEV)
    want = torch.round(losses.scan_render(parsed, 256, 255) * 255).to(torch.uint8).cpu().numpy()
    saved = np.load(os.path.join(out, "images.npy"))
    assert saved.shape == (6, 256, 256) and np.array_equal(saved, want) and (saved > 0).any()


def test_test_random_on_the_gpu(tmp_path):
    import test_random
    torch.manual_seed(0)
    res = str(tmp_path / "results.txt")
    iou = test_random.main(["--n", "8", "--batch", "4", "--render-size", "32", "--model", str(tmp_path / "none.pt"),
                            "--results", res])
    assert iou.shape == (8,) and np.isfinite(iou).all() and (iou >= 0).all() and (iou <= 1).all()
    text = open(res).read()
    assert text.count("True params:") == 8 and text.count("- Accuracy:") == 8


def test_train_py_on_scanner_images(tmp_path):
    """train.py --synthetic 128 --synthetic-render scanner: batch size, steps and the loss check of
    test_least_squares_gpu.py's train.py run (batch 8, one epoch of 3 steps, finite losses)."""
    import train
    torch.manual_seed(0)
    tl, vl = train.main(["--synthetic", "128", "--synthetic-render", "scanner", "--batch-size", "8", "--epochs", "1",
                         "--max-steps", "3", "--render-size", "32", "--pretrained", "0", "--log-interval", "1",
                         "--model-location", str(tmp_path / "m.pt"), "--bf16"])
    assert len(tl) == 1 and np.isfinite(tl).all() and np.isfinite(vl).all()
