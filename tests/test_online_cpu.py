"""The online label sampler on the host: Philox4x32-10's known answers, sqr/cpu.py's vectorised sampler against
the scalar restatement (tests/_philox_ref.py) bitwise, the distribution and ranges of the labels, and
sqr.data.OnlineSource on a CPU device (batch splitting, rank/world slicing, state round trip)."""
import math

import numpy as np
import pytest
import torch

import _philox_ref as ref

N = 65536
SETS = ((0, 0), (0, 1), (12345, 0))  # (seed, substream)

KNOWN = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


@pytest.mark.parametrize("counter,key,out", KNOWN)
def test_philox_known_answers(counter, key, out):
    from sqr import cpu
    assert ref.philox(counter, key) == out
    got = cpu.philox4x32_10([np.array([c], dtype=np.uint64) for c in counter], key)
    assert tuple(int(g[0]) for g in got) == out


@pytest.mark.parametrize("seed", [0, 12345, 2 ** 63 + 12345, 0xDEADBEEF00000001])
@pytest.mark.parametrize("substream", [0, 1, 0xFFFFFFFF])
@pytest.mark.parametrize("position", [0, 2 ** 32 - 3, 2 ** 40 + 5, 2 ** 64 - 2])
def test_host_sampler_words_equal_scalar(seed, substream, position):
    from sqr import cpu
    n = 7  # 2^32 - 3 + 7 straddles the carry into i_hi; 2^64 - 2 + 7 wraps
    got = cpu.sq_sample_raw(position, n, seed, substream)
    assert got.dtype == np.uint32 and got.shape == (n, 12)
    assert got.tolist() == ref.batch_words(seed, substream, position, n)


def test_host_sampler_labels_equal_scalar():
    from sqr import cpu
    pos, n = 2 ** 32 - 3, 9
    raw = cpu.sq_sample_raw(pos, n, 12345, 1)
    lab = cpu.sq_sample(pos, n, 12345, 1)
    assert lab.dtype == np.float32 and lab.shape == (n, 12)
    for b in range(n):
        u = ref.uniforms(raw[b].tolist())
        assert cpu.sq_uniforms(raw)[b].tolist() == u
        want = np.array(ref.labels(u))
        # float64 formula rounded once; numpy's and math's sin / cos may differ in the last float64 place
        assert np.all(np.abs(lab[b].astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32)))


@pytest.fixture(scope="module")
def sets():
    from sqr import cpu
    out = {}
    for seed, sub in SETS:
        raw = cpu.sq_sample_raw(0, N, seed, sub)
        out[(seed, sub)] = (cpu.sq_uniforms(raw), cpu.sq_labels(cpu.sq_uniforms(raw)))
    return out


@pytest.mark.parametrize("key", SETS)
def test_distribution(sets, key):
    """5 sigma caps on the moments of the eleven uniforms and of the quaternion (uniform on the 3-sphere:
    E q_i = 0, E q_i q_j = delta_ij / 4)."""
    u, lab = sets[key]
    rn = math.sqrt(N)
    worst = 0.0

    def cap(dev, sigma, what):
        nonlocal worst
        z = float(np.max(np.abs(dev))) * rn / sigma
        worst = max(worst, z)
        assert z <= 5.0, "%s: %.2f sigma" % (what, z)

    cap(u.mean(0) - 0.5, math.sqrt(1 / 12), "uniform means")
    cap(u.var(0) - 1 / 12, math.sqrt(1 / 180), "uniform variances")
    corr = np.corrcoef(u.T)
    cap(corr[~np.eye(11, dtype=bool)], 1.0, "uniform correlations")
    q = lab[:, 8:].astype(np.float64)
    cap(q.mean(0), 0.5, "quaternion means")
    m = q.T @ q / N
    cap(m[~np.eye(4, dtype=bool)], math.sqrt(1 / 24), "quaternion off-diagonal moments")
    cap(np.diag(m) - 0.25, math.sqrt(1 / 16), "quaternion diagonal moments")
    print("set %s: worst statistic %.2f sigma" % (key, worst))


@pytest.mark.parametrize("key", SETS)
def test_ranges(sets, key):
    _, lab = sets[key]
    f = np.float32
    a, e, t, q = lab[:, :3], lab[:, 3:5], lab[:, 5:8], lab[:, 8:].astype(np.float64)
    assert np.all(a >= f(25 / 255)) and np.all(a < f(75 / 255))
    assert np.all(e >= f(0.1)) and np.all(e < f(1))
    assert np.all(t >= f(88 / 255)) and np.all(t < f(168 / 255))
    assert np.max(np.abs(np.sqrt((q * q).sum(1)) - 1)) <= 1e-6


def test_matches_sample_sq_params_distribution(sets):
    """The ranges and means of classes.sample_sq_params' numpy draw (its generator's own distribution)."""
    import classes
    old = classes.sample_sq_params(np.random.default_rng(0), N).astype(np.float64)
    new = sets[(0, 0)][1].astype(np.float64)
    # 8 uniform columns with sd width / sqrt(12): two independent means differ by < 5 sqrt(2) sd / sqrt(N)
    width = np.array([50 / 255] * 3 + [0.9] * 2 + [80 / 255] * 3)
    assert np.all(np.abs(old[:, :8].mean(0) - new[:, :8].mean(0)) <= 5 * math.sqrt(2 / 12 / N) * width)
    assert np.all(np.abs(old[:, 8:].mean(0) - new[:, 8:].mean(0)) <= 5 * math.sqrt(2 / N) * 0.5)


# ---------------------------------------------------------------- OnlineSource on a CPU device, size 16
def _src(batch, **kw):
    from sqr.data import OnlineSource
    return OnlineSource(batch, "cpu", size=16, **kw)


def test_online_source_cpu_images_and_labels():
    from sqr import cpu
    s = _src(8, seed=3)
    img, lab = s.next()
    assert img.shape == (8, 1, 16, 16) and img.dtype == torch.float32 and lab.shape == (8, 12)
    assert np.array_equal(lab.numpy(), cpu.sq_sample(0, 8, 3, 0))
    assert torch.equal(img[:, 0], cpu.scan_render(lab, 16, 255).to(torch.float32))
    assert float(img.max()) > 0
    assert s.position() == 8
    soft = _src(2, seed=3, render="soft")
    img2, lab2 = soft.next()
    assert torch.equal(lab2, lab[:2])
    assert torch.equal(img2[:, 0], cpu.render(lab2, 16, 1.5, 260).to(torch.float32))


def test_online_source_cpu_split_and_ranks():
    one = _src(16)
    img16, lab16 = (t.clone() for t in one.next())
    two = _src(8)
    parts = [tuple(t.clone() for t in two.next()) for _ in range(2)]
    assert torch.equal(torch.cat([p[0] for p in parts]), img16)
    assert torch.equal(torch.cat([p[1] for p in parts]), lab16)
    assert one.position() == two.position() == 16
    r1 = _src(8, rank=1, world=2)
    img, lab = r1.next()
    assert torch.equal(img, img16[8:]) and torch.equal(lab, lab16[8:])
    assert r1.position() == 16
    sub1 = _src(16, substream=1)
    assert not torch.equal(sub1.next()[1], lab16)


def test_online_source_cpu_state_round_trip():
    a = _src(4, seed=2 ** 63 + 12345, substream=1)
    a.seek(2 ** 32 - 2)
    a.next()
    st = a.state_dict()
    assert st == {"seed": 2 ** 63 + 12345, "substream": 1, "position": 2 ** 32 + 2}
    want = tuple(t.clone() for t in a.next())
    b = _src(4)
    b.load_state_dict(st)
    assert b.state_dict() == st
    got = b.next()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    a.seek(2 ** 64 - 1)  # the top of the range is a valid position
    assert a.position() == 2 ** 64 - 1


def test_online_source_rejects_bad_arguments():
    from sqr.data import OnlineSource
    with pytest.raises(ValueError):
        OnlineSource(0, "cpu")
    with pytest.raises(ValueError):
        OnlineSource(4, "cpu", rank=2, world=2)
    with pytest.raises(ValueError):
        OnlineSource(4, "cpu", render="hard")


def test_captured_step_draws_from_source_on_cpu():
    """sqr.step.CapturedStep with a source: step() takes no batch and trains on the source's next one; passing
    a batch as well, or none without a source, is an error."""
    from sqr.step import CapturedStep
    w = torch.nn.Parameter(torch.zeros(12))
    opt = torch.optim.SGD([w], lr=0.5)
    seen = []

    def body(x, labels):
        seen.append(labels.clone())
        loss = ((w - labels.mean(0)) ** 2).sum()
        loss.backward()
        opt.step()
        return loss

    src = _src(4, seed=11)
    st = CapturedStep(body, opt, "cpu", source=src.next)
    st.step()
    st.step()
    out = st.drain()
    assert len(out) == 2 and all(np.isfinite(v) and not nan for v, nan in out)
    twin = _src(4, seed=11)
    assert torch.equal(seen[0], twin.next()[1]) and torch.equal(seen[1], twin.next()[1])
    assert src.position() == 8
    with pytest.raises(ValueError):
        st.step(seen[0], seen[0])
    with pytest.raises(ValueError):
        CapturedStep(body, opt, "cpu").step()


def test_sq_sample_validates_arguments_without_gpu():
    from sqr import _lib
    L = _lib.lib()
    assert L.sqr_sq_sample(None, 0, 0, 0, 0, None, None, None) == -1
    assert b"B=0" in L.sqr_last_error_string()
    assert L.sqr_sq_sample(None, 0, 0, 0, 65536, None, None, None) == -1
    assert L.sqr_sq_sample(None, 0, 0, 0, 4, None, None, None) == -1
    assert b"null pointer" in L.sqr_last_error_string()
    assert L.sqr_sq_stream_advance(None, 8, None) == -1


def test_train_parses_online_flags():
    import train
    a = train.parse_args(["--online", "5"])
    assert a.online == 5 and a.online_val == 1024 and a.seed == 0 and a.synthetic_render == "scanner"
    assert train.parse_args(["--online", "5", "--synthetic-render", "soft"]).synthetic_render == "soft"
    with pytest.raises(SystemExit):
        train.parse_args(["--online", "5", "--synthetic", "64"])
