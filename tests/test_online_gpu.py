"""The online data source on the GPU: sqr_sq_sample's words bitwise against the scalar restatement
(tests/_philox_ref.py), its labels against the float64 formula at the same uniforms, the device-resident
position (advance, batch splitting, rank/world slicing), next() captured in a graph (every replay must draw
NEW samples: a position baked into the graph fails), the rendered images bitwise against the renderers called
directly, and train.py --online with the captured step against the eager loop.

Label accuracy bounds: a, e, t are at most three float32 roundings from the exact value (2 ulp); a quaternion
component is one square root and one sin / cos of a few ulp each on values <= 1 and one product (1e-6
absolute).  Measured on an MI355X (profiles/online_accuracy.txt holds the printed lines)."""
import os

import numpy as np
import pytest
import torch

import _philox_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 32
SEEDS = (0, 2 ** 63 + 12345)


def _dev():
    return torch.device("cuda", 0)


def _pos(value):
    from sqr.data import _as_i64
    return torch.tensor([_as_i64(value)], dtype=torch.int64, device=_dev())


def _sample(position, seed, substream, offset, B):
    """(params [B,12] float32, words [B,12] uint32) as numpy, the guard words behind both checked."""
    from sqr import data
    pbuf = torch.full((B * 12 + GUARD,), -7.0, dtype=torch.float32, device=_dev())
    rbuf = torch.full((B * 12 + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device=_dev())
    pos = _pos(position)
    data.sq_sample(pos, seed, substream, offset, B, pbuf[:B * 12].view(B, 12), rbuf[:B * 12].view(B, 12))
    torch.cuda.synchronize()
    assert int(pos.item()) == data._as_i64(position)  # the sampler only reads it
    assert torch.all(pbuf[B * 12:] == -7.0) and torch.all(rbuf[B * 12:] == 0x5A5A5A5A)
    return pbuf[:B * 12].view(B, 12).cpu().numpy(), rbuf[:B * 12].view(B, 12).cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 257, 1100])
@pytest.mark.parametrize("position", [0, 2 ** 32 - 3, 2 ** 40 + 5])
def test_words_bitwise(B, position):
    """Wave and block edges; the carry into i_hi inside the batch (2^32 - 3) and a high word (2^40 + 5);
    both seeds, both substreams, offset zero and non-zero."""
    for seed, substream, offset in ((s, sub, off) for s in SEEDS for sub in (0, 1) for off in (0, 77)):
        _, raw = _sample(position, seed, substream, offset, B)
        want = np.array(ref.batch_words(seed, substream, position + offset, B), dtype=np.uint32)
        assert np.array_equal(raw, want), (seed, substream, offset)


def test_words_without_raw_and_wrapping_position():
    from sqr import data
    pos = _pos(2 ** 64 - 2)  # rows 2.. wrap to sample 0..
    p = data.sq_sample(pos, 5, 0, 0, 6)
    p2, raw = _sample(2 ** 64 - 2, 5, 0, 0, 6)
    assert np.array_equal(p.cpu().numpy(), p2)
    assert raw.tolist() == ref.batch_words(5, 0, 2 ** 64 - 2, 6)


def _ulps(got, want64):
    return np.abs(got.astype(np.float64) - want64) / np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)


def test_labels_against_float64():
    from sqr import cpu
    worst = {"a": 0.0, "e": 0.0, "t": 0.0, "q": 0.0, "norm": 0.0}
    for seed, substream, position in ((0, 0, 0), (2 ** 63 + 12345, 1, 2 ** 32 - 300), (12345, 0, 2 ** 40 + 5)):
        p, raw = _sample(position, seed, substream, 0, 1100)
        p_again, raw_again = _sample(position, seed, substream, 0, 1100)
        assert np.array_equal(p.view(np.uint32), p_again.view(np.uint32)) and np.array_equal(raw, raw_again)
        u = (raw[:, :11] >> np.uint32(8)).astype(np.float64) / 2.0 ** 24
        assert np.array_equal(u, cpu.sq_uniforms(raw))
        want = np.array([ref.labels(row) for row in u.tolist()])
        ul = _ulps(p[:, :8], want[:, :8])
        worst["a"] = max(worst["a"], ul[:, :3].max())
        worst["e"] = max(worst["e"], ul[:, 3:5].max())
        worst["t"] = max(worst["t"], ul[:, 5:8].max())
        worst["q"] = max(worst["q"], np.abs(p[:, 8:].astype(np.float64) - want[:, 8:]).max())
        q = p[:, 8:].astype(np.float64)
        worst["norm"] = max(worst["norm"], np.abs(np.sqrt((q * q).sum(1)) - 1).max())
        f = np.float32
        assert np.all(p[:, :3] >= f(25 / 255)) and np.all(p[:, :3] < f(75 / 255))
        assert np.all(p[:, 3:5] >= f(0.1)) and np.all(p[:, 3:5] < f(1))
        assert np.all(p[:, 5:8] >= f(88 / 255)) and np.all(p[:, 5:8] < f(168 / 255))
    print("online accuracy: 3 x 1100 samples: a %.3f ulp, e %.3f ulp, t %.3f ulp, q %.3e abs, | |q| - 1 | %.3e"
          % (worst["a"], worst["e"], worst["t"], worst["q"], worst["norm"]))
    assert worst["a"] <= 2 and worst["e"] <= 2 and worst["t"] <= 2
    assert worst["q"] <= 1e-6 and worst["norm"] <= 1e-6


def _src(batch, size=16, **kw):
    from sqr.data import OnlineSource
    return OnlineSource(batch, _dev(), size=size, **kw)


def _take(src):
    img, lab = src.next()
    return img.clone(), lab.clone()


def test_position_advance():
    from sqr import data
    pos = _pos(2 ** 32 - 10)
    for _ in range(3):
        data.stream_advance(pos, 7)
    assert int(pos.item()) == 2 ** 32 + 11  # the carry into the high word
    s = _src(8, rank=1, world=4)
    for k in range(1, 4):
        s.next()
        assert s.position() == k * 32
    s.seek(2 ** 40 + 5)
    s.next()
    assert s.position() == 2 ** 40 + 37 and s.state_dict() == {"seed": 0, "substream": 0, "position": 2 ** 40 + 37}


def test_batch_split_and_ranks_bitwise():
    from sqr import cpu
    one = _src(16, seed=9)
    img16, lab16 = _take(one)
    two = _src(8, seed=9)
    parts = [_take(two) for _ in range(2)]
    assert torch.equal(torch.cat([p[0] for p in parts]), img16)
    assert torch.equal(torch.cat([p[1] for p in parts]), lab16)
    assert one.position() == two.position() == 16
    r1 = _src(8, seed=9, rank=1, world=2)
    img, lab = _take(r1)
    assert torch.equal(img, img16[8:]) and torch.equal(lab, lab16[8:])
    assert r1.position() == 16
    restored = _src(8, seed=1)
    restored.load_state_dict({"seed": 9, "substream": 0, "position": 8})
    assert torch.equal(_take(restored)[1], lab16[8:])
    # the host sampler draws the same samples (its labels: the float64 formula rounded once)
    host = cpu.sq_sample(0, 16, 9, 0)
    assert np.abs(lab16.cpu().numpy()[:, :8] / host[:, :8] - 1).max() <= 2 * 2.0 ** -23
    assert np.abs(lab16.cpu().numpy()[:, 8:] - host[:, 8:]).max() <= 1e-6
    assert not torch.equal(_take(_src(16, seed=9, substream=1))[1], lab16)


def test_capture_draws_new_samples_each_replay():
    """One next() captured, replayed three times: the batches are those of an eager source at the next three
    positions, and differ from each other.  A position passed by value would replay the first batch."""
    src = _src(5, seed=7)
    src.seek(2 ** 32 - 7)  # the second replay's batch straddles the carry
    first = _take(src)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        img, lab = src.next()
    assert src.position() == 2 ** 32 - 2  # capturing runs nothing
    got = []
    for _ in range(3):
        g.replay()
        got.append((img.clone(), lab.clone()))
    assert src.position() == 2 ** 32 + 13
    eager = _src(5, seed=7)
    eager.seek(2 ** 32 - 7)
    want = [_take(eager) for _ in range(4)]
    assert torch.equal(first[0], want[0][0]) and torch.equal(first[1], want[0][1])
    for k in range(3):
        assert torch.equal(got[k][0], want[k + 1][0]) and torch.equal(got[k][1], want[k + 1][1]), k
    for i in range(3):
        for j in range(i + 1, 3):
            assert not torch.equal(got[i][1], got[j][1]) and not torch.equal(got[i][0], got[j][0])


@pytest.mark.parametrize("size", [16, 50])
def test_images_are_scan_render_of_labels(size):
    from sqr import losses
    img, lab = _src(5, size=size, seed=3).next()
    assert img.shape == (5, 1, size, size) and float(img.max()) > 0
    assert torch.equal(img[:, 0], losses.scan_render(lab, size, 255))


def test_soft_images_are_implicit_render_of_labels():
    from sqr import losses
    img, lab = _src(5, size=32, seed=3, render="soft").next()
    assert torch.equal(img[:, 0], losses.implicit_render(lab, 32, 1.5, 260))
    assert torch.equal(lab, _src(5, size=16, seed=3).next()[1])


def _train(tmp_path, graph):
    import train
    ck = os.path.join(str(tmp_path), "ck_online%d.pt" % graph)
    torch.manual_seed(0)
    tl, vl = train.main(["--online", "4", "--batch-size", "8", "--epochs", "2", "--render-size", "32", "--pretrained",
                         "0", "--bf16", "--online-val", "16", "--graph", str(graph), "--model-location", ck])
    return tl, vl, torch.load(ck, map_location="cpu", weights_only=True), ck


@pytest.mark.timeout(300)
def test_train_online_graph_equals_eager(tmp_path, capsys):
    from sqr import cpu
    from sqr.data import OnlineSource
    tl_g, vl_g, ck_g, path = _train(tmp_path, 1)
    out = capsys.readouterr().out
    assert "HIP graph" in out and "images/s" in out
    tl_e, vl_e, ck_e, _ = _train(tmp_path, 0)
    assert "eager" in capsys.readouterr().out
    assert len(tl_g) == 2 and tl_g == tl_e and vl_g == vl_e, (tl_g, tl_e, vl_g, vl_e)
    assert all(np.isfinite(tl_g)) and all(np.isfinite(vl_g))
    for k, v in ck_e["model_state_dict"].items():
        assert torch.equal(ck_g["model_state_dict"][k], v), k
    # 2 epochs of 4 steps of 8 samples, the checkpoint written after the second
    assert ck_g["stream_state"] == ck_e["stream_state"] == {"seed": 0, "substream": 0, "position": 2 * 4 * 8}
    # a source restored from the checkpoint goes on with the host sampler's rows at the saved position
    import helpers
    import models
    from sqr.optim import Adam
    net = models.ResNetSQ(outputs=4, pretrained=False).cuda()
    position = ck_g["stream_state"]["position"]
    host_src = OnlineSource(8, "cpu", size=16, seed=99)
    helpers.load_model(path, net, Adam(net.parameters(), lr=1e-4), source=host_src)
    assert host_src.position() == position
    assert np.array_equal(host_src.next()[1].numpy(), cpu.sq_sample(position, 8, 0, 0))
    dev_src = OnlineSource(8, _dev(), size=16, seed=99)
    helpers.load_model(path, net, Adam(net.parameters(), lr=1e-4), source=dev_src)
    lab = dev_src.next()[1].cpu().numpy()
    want = cpu.sq_sample(position, 8, 0, 0)
    assert np.abs(lab[:, :8] / want[:, :8] - 1).max() <= 2 * 2.0 ** -23 and np.abs(lab[:, 8:] - want[:, 8:]).max() <= 1e-6
