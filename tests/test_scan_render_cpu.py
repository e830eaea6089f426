"""The scanner-style depth renderer on the host (sqr.cpu.scan_render) against the scanner's own ten example
images, closed forms and edge cases, and its consumers on the CPU: SyntheticDataset(render="scanner"),
helpers.write_image_gray, gen_dataset.py."""
import os

import numpy as np
import pytest
import torch

import _scan_cases as sc
from sqr import cpu


@pytest.fixture(scope="module")
def fixture_render():
    labels, images = sc.fixture()
    depth, fmin = cpu.scan_render(torch.tensor(labels), 256, 255, return_fmin=True)
    return labels, images, depth.numpy(), fmin.numpy()


@pytest.mark.parametrize("i", range(10))
def test_scanner_parity(fixture_render, i):
    """The float64 host render of the fixture's label i against the scanner's image i."""
    _, images, depth, fmin = fixture_render
    sc.scanner_caps(sc.to_levels(depth[i]), images[i], fmin[i])


def test_single_sample_equals_batch(fixture_render):
    labels, _, depth, _ = fixture_render
    one = cpu.scan_render(torch.tensor(labels[3:4]), 256, 255).numpy()
    assert np.array_equal(one[0], depth[3])


@pytest.mark.parametrize("case", sc.closed_form_cases(), ids=lambda c: c[0])
def test_closed_form(case):
    _, params, z, br = case
    got = cpu.scan_render(torch.tensor(params), sc.CF_SIZE, 0).numpy()[0]
    inside, outside = br >= sc.CF_EDGE, br <= -sc.CF_EDGE
    assert inside.sum() > 100 and outside.sum() > 100
    assert np.abs(got - z)[inside].max() <= sc.CF_TOL
    assert (got[outside] == 0).all()
    assert (got >= 0).all() and got.max() <= z.max() + sc.CF_TOL
    if "id" in case[0]:  # u0 = u1 = 0 exactly on this ray: two exact-zero terms, no NaN
        assert abs(got[sc.AXIS_PIXEL] - (sc.CF_T[2] + sc.CF_A[2])) <= sc.CF_TOL
    assert np.isfinite(got).all()


@pytest.mark.parametrize("case", sc.closed_form_cases()[2:4], ids=lambda c: c[0])
def test_closed_form_float32_and_quantised(case):
    """dtype=float32 works (the GPU tests' yardstick), to fp32 accuracy away from the silhouette; levels
    quantise the continuous depth downwards."""
    _, params, z, br = case
    p = torch.tensor(params)
    got32 = cpu.scan_render(p, sc.CF_SIZE, 0, dtype=torch.float32)
    assert got32.dtype == torch.float32
    inside = br >= 1e-2
    assert np.abs(got32.numpy()[0].astype(np.float64) - z)[inside].max() <= 1e-4
    cont = cpu.scan_render(p, sc.CF_SIZE, 0).numpy()
    q = cpu.scan_render(p, sc.CF_SIZE, 255).numpy()
    assert np.array_equal(q, np.floor(255 * cont) / 255) and len(np.unique(q)) > 20
    with pytest.raises(ValueError):
        cpu.scan_render(p, sc.CF_SIZE, -1)


def _render(rows, size=64, levels=0):
    return cpu.scan_render(torch.tensor(np.stack(rows)), size, levels).numpy()


def test_edge_cases():
    r = sc.edge_rows()
    names = ["base", "unclamped", "clamped", "q_times_4", "q_times_1p7", "q_unit", "above_one", "off_frame"]
    img = dict(zip(names, _render([r[n] for n in names])))
    assert (img["base"] > 0).sum() > 100
    assert np.array_equal(img["unclamped"], img["clamped"]) and (img["clamped"] > 0).any()
    # a power-of-two multiple of q normalises to the same bits; any other to within rounding of q / |q|
    assert np.array_equal(img["q_times_4"], img["base"])
    fg = (img["q_unit"] > 0) == (img["base"] > 0)
    assert (~fg).sum() <= 2 and np.abs(img["q_times_1p7"] - img["base"])[fg].max() <= 1e-6
    assert np.abs(img["q_unit"] - img["base"])[fg].max() <= 1e-6
    # a body reaching z = 1.2 saturates at exactly 1
    assert img["above_one"].max() == 1.0 and img["above_one"][32, 32] == 1.0
    # a body across the frame's corner: foreground on the border, nothing out of range
    off = img["off_frame"]
    assert np.isfinite(off).all() and off.min() >= 0 and off.max() <= 1
    assert (off[0] > 0).any() and (off[:, 0] > 0).any()


@pytest.mark.parametrize("bad", ["nan", "inf", "q_zero"])
def test_invalid_row_is_zero_and_leaves_neighbours(bad):
    r = sc.edge_rows()
    img, fmin = cpu.scan_render(torch.tensor(np.stack([r["base"], r[bad], r["off_frame"]])), 64, 255,
                                return_fmin=True)
    alone = _render([r["base"], r["off_frame"]], levels=255)
    assert (img[1] == 0).all()
    assert np.array_equal(img[0].numpy(), alone[0]) and np.array_equal(img[2].numpy(), alone[1])
    assert torch.isfinite(img).all() and not torch.isnan(fmin[[0, 2]]).any()


def test_inside_outside_at_the_surface(fixture_render):
    """scan_inside_outside: F = 1 and dF/dz >= 0 at the continuous z_top of every foreground pixel."""
    labels = torch.tensor(sc.fixture()[0][:2])
    z = cpu.scan_render(labels, 64, 0)
    F, dF = cpu.scan_inside_outside(labels, 64, z)
    fg = (z > 0) & (z < 1)
    assert fg.sum() > 200
    assert (F[fg] - 1).abs().max() <= 1e-9 and dF[fg].min() >= 0


# ------------------------------------------------------------------------------ consumers
def test_synthetic_dataset_scanner_render():
    import classes
    ds = classes.SyntheticDataset(8, "cpu", size=64, render="scanner")
    want = cpu.scan_render(ds.labels, 64, 255).to(torch.float32)
    assert ds.images.shape == (8, 1, 64, 64) and ds.images.dtype == torch.float32
    assert torch.equal(ds.images[:, 0], want)
    assert (ds.images > 0).any()
    with pytest.raises(ValueError):
        classes.SyntheticDataset(2, "cpu", size=16, render="hard")


def test_synthetic_dataset_default_is_the_soft_render():
    import classes
    import torch.nn.functional as F
    ds = classes.SyntheticDataset(4, "cpu", size=64)
    soft = F.interpolate(cpu.render(ds.labels, 64, 1.5, 260).float().unsqueeze(1), size=(64, 64), mode="nearest")
    assert torch.equal(ds.images, soft)
    assert torch.equal(classes.SyntheticDataset(4, "cpu", size=64, render="soft").images, soft)


def test_train_parses_synthetic_render():
    import train
    assert train.parse_args([]).synthetic_render == "soft"
    assert train.parse_args(["--synthetic-render", "scanner"]).synthetic_render == "scanner"


def test_write_image_gray_roundtrip(tmp_path):
    from helpers import read_image_gray, write_image_gray
    img = sc.fixture()[1][3]
    p = str(tmp_path / "x.bmp")
    write_image_gray(p, img)
    assert np.array_equal(read_image_gray(p), img)
    odd = np.arange(7 * 5, dtype=np.uint8).reshape(7, 5) * 7  # a row that needs padding
    write_image_gray(p, odd)
    assert np.array_equal(read_image_gray(p), odd)
    with pytest.raises(ValueError):
        write_image_gray(p, odd.astype(np.float32))


def test_gen_dataset_cpu(tmp_path):
    import classes
    import gen_dataset
    from helpers import parse_csv, quat2mat, read_image_gray
    out = str(tmp_path / "set")
    labels, images = gen_dataset.main(["--n", "4", "--out", out, "--seed", "3", "--device", "cpu", "--batch", "3",
                                       "--bmp"])
    drawn = classes.sample_sq_params(np.random.default_rng(3), 4)
    parsed = np.stack(parse_csv(os.path.join(out, "data_labels.csv")))
    assert parsed.shape == (4, 12) and np.abs(parsed - drawn).max() <= 1e-6
    assert np.array_equal(parsed, labels)
    saved = np.load(os.path.join(out, "images.npy"))
    assert saved.dtype == np.uint8 and saved.shape == (4, 256, 256) and np.array_equal(saved, images)
    want = sc.to_levels(cpu.scan_render(torch.tensor(parsed), 256, 255).numpy())
    assert np.array_equal(saved, want) and (saved > 0).any()
    with open(os.path.join(out, "data_labels.csv")) as f:
        rows = [line.split(",") for line in f.read().split("\n") if line]
    for i, row in enumerate(rows):
        assert row[0] == "%06d.bmp" % i and len(row) == 22
        v = np.array([float(s) for s in row[1:]])
        assert np.abs(v[8:17] - quat2mat(v[17:21]).ravel()).max() <= 1e-6
        assert np.array_equal(read_image_gray(os.path.join(out, row[0])), saved[i])


def test_gen_dataset_h5_needs_h5py(tmp_path):
    import gen_dataset
    try:
        import h5py  # noqa: F401
    except ImportError:
        with pytest.raises(SystemExit, match="h5py"):
            gen_dataset.main(["--n", "1", "--out", str(tmp_path / "s"), "--device", "cpu", "--h5"])
        return
    gen_dataset.main(["--n", "1", "--out", str(tmp_path / "s"), "--device", "cpu", "--h5"])
    with h5py.File(str(tmp_path / "s" / "dataset.h5"), "r") as h:
        assert h["sq"].shape == (1, 1, 256, 256)
