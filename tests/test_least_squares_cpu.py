"""classes.LeastSquares on the CPU (the plain-torch path) against the reference's own class
(tests/golden/least_squares.npz, made by gen_golden_lsq.py), in the reference's float32 and with the
inputs upcast to float64, and train.py --loss leastsquares on the CPU.

Tolerance.  float64: the plain-torch path is the reference's code operation for operation, so it may
differ from the fixture only by the order in which a few terms are added: 4 eps on the loss, 8 eps of
the sample's largest gradient entry on the gradient.  float32: the same operations round differently
when torch picks another kernel for them (a 3x3 by 3xN product as matmul or as einsum), and near the
surface F - 1 amplifies that; the size of such a difference is the float32 path's own distance from
float64, which the fixture holds.  So the float32 run is compared with the float64 fixture and may be
off by twice the reference's own float32 error plus the eps terms above."""
import numpy as np
import pytest
import torch

from _lsq_cases import golden_cases

CASES = golden_cases()


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_cpu_least_squares_vs_golden(case, dt):
    import classes
    tag = "32" if dt == torch.float32 else "64"
    eps = float(torch.finfo(dt).eps)
    p = torch.tensor(case["pred"]).to(dt).requires_grad_(True)
    loss = classes.LeastSquares(case["R"], "cpu")(torch.tensor(case["true"]).to(dt), p)
    assert loss.dtype == dt and loss.dim() == 0  # the reference does not call .double() here
    loss.backward()
    ref, gref = float(case["loss64"]), case["grad64"]
    own = abs(float(case["loss32"]) - ref) if tag == "32" else 0.0  # the reference's own float32 error
    assert abs(loss.item() - ref) <= 2 * own + 4 * eps * abs(ref), (loss.item(), ref)
    g = p.grad.numpy().astype(np.float64)
    assert np.isfinite(g).all()
    for b in range(len(g)):
        own = np.abs(case["grad32"][b] - gref[b]).max() if tag == "32" else 0.0
        assert np.abs(g[b] - gref[b]).max() <= 2 * own + 8 * eps * np.abs(gref[b]).max(), (b, g[b], gref[b])


def test_fixture_covers_the_edge_cases():
    by = {c["name"]: c for c in CASES}
    assert float(by["zero_R32"]["loss64"]) == 0.0 and not by["zero_R32"]["grad64"].any()
    assert [(c["true"] > 0).sum() for c in [by["onepix_R32"]]] == [3]  # one point per image
    assert by["big512_R32"]["true"].shape[-2:] == (512, 512)
    assert by["raw255_R32"]["true"].max() > 200
    assert {c["R"] for c in CASES} == {32, 48, 64}
    # at the labels the points lie on the surface: the energy is small and all cancellation
    assert all(float(by[n]["loss64"]) < 5e-3 for n in ("labels_R32", "labels_R48", "labels_R64"))


def test_train_py_cpu_least_squares(tmp_path):
    """train.py --loss leastsquares --device cpu: the plain-torch path, training and validation."""
    import train
    ckpt = tmp_path / "model.pt"
    losses, val = train.main(["--device", "cpu", "--loss", "leastsquares", "--synthetic", "10", "--batch-size", "4",
                              "--epochs", "1", "--max-steps", "2", "--render-size", "16", "--pretrained", "0",
                              "--model-location", str(ckpt), "--log-interval", "100"])
    assert len(losses) == 1 and np.isfinite(losses[0]) and np.isfinite(val[0])
    sd = torch.load(str(ckpt), map_location="cpu", weights_only=True)
    assert "encoder.layer1.0.conv1.weight" in sd["model_state_dict"]
