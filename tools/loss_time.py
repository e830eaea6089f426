"""The fused ImplicitLoss call (loss + analytic gradient, bench.time_loss_call: graph replays) at the
bench shapes; one JSON line.  Environment knobs of libsqr's A/B builds pass through (SQR_*).

    python tools/loss_time.py leastsquares

times the LeastSquares loss instead, forward + backward at B = 64, R = 64, 256^2 on CUDA tensors: the
HIP kernel path (eagerly, host clock around a device synchronise, and per call inside a replayed graph)
against the plain-torch path (the reference's per-image code, which cannot be captured: every
torch.where waits for the device).

    python tools/loss_time.py lm

times the Levenberg-Marquardt refinement at the same shapes: one normal-equations call and a 10-iteration
sqr.fit.refine_lm, each eagerly and inside a replayed graph, next to the least_squares forward + backward
call and to sqr.fit.refine's 200 Adam steps in the same process.

    python tools/loss_time.py recover

times the classical recovery (sqr.fit.recover, 30 iterations per start) at the same shapes, eagerly and inside
a replayed graph, next to its starts alone and to one sqr.fit.refine_lm with the same iterations in the same
process, and reports the energies, the winning starts and the IoU against the labels of that batch.

    python tools/loss_time.py recover-multi

times the six-start scored recovery (sqr.fit.recover with starts="depth", free_space=1) and free_space_energy
alone on that batch, eagerly and inside a replayed graph, next to the three-start recover (the same chain over
3 B samples, selected by energy alone), to the same three starts with the score and to the batched refinement
against three separate ones, in the same process, and reports the IoU of the three-start and of the six-start
scored winners.

    python tools/loss_time.py scan

times the scanner-style depth render (sqr_scan_render) at B = 256, S = 256, eagerly and inside a replayed
graph, next to implicit_render at the same B and S (the render it stands beside in SyntheticDataset; the two
produce different images) and to the float64 host renderer on 16 threads over 16 of the images.

    python tools/loss_time.py online

times sqr.data.OnlineSource.next() (sampler, advance, scanner render) at B = 64, size 256, eagerly and inside
a replayed graph, next to scan_render alone on the same labels and to the sampler + advance alone, in the
same process; the difference of the first two is the cost of drawing the labels on the device.  It measures
everything twice and prints one JSON line per pass.

    python tools/loss_time.py points

times the point-list stack at B = 64, P = 4096 (the slots of the recover mode's R = 64 scanner-style images, as a
list in pixel order), 30 iterations: sqr.fit.recover_points next to sqr.fit.recover on the same images, eagerly and
inside a replayed graph, and losses.point_energy forward + backward next to LeastSquares.energy_function (plain
torch, forward + backward) on the same CUDA point lists.  Everything twice in one process, one JSON line per pass.

    python tools/loss_time.py parts

times sqr.fit.recover_parts at B = 8 clouds of M = 4 bodies, P = 4096, 3 rounds, eagerly and inside a replayed
graph, next to the same fits done with the single-body calls in the same process: recover_points, then
refine_points, on the B M NaN-masked copies of the clouds, the assignment between the rounds in torch ops, from
precomputed seeding labels (so the chain is also timed from those labels, without its seeding); and the assignment
kernel alone, and one normal-equations evaluation of the B M parts next to one of the B clouds (the M-fold walk of
the part source).  Everything twice in one process, one JSON line per pass."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sq-recovery_amd"))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import classes  # noqa: E402
from sqr import losses  # noqa: E402


def _eager_ms(fn, warmup=3, reps=20):
    """Host time of fn() per call, the device drained before and after."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def least_squares(dev, R=64, H=256, B=64):
    p = torch.tensor(classes.sample_sq_params(np.random.default_rng(0), B), device=dev)
    img = losses.implicit_render(p, H, 1.5, 260).unsqueeze(1).contiguous()
    torch.manual_seed(0)
    pred = (p + 0.02 * torch.randn_like(p)).requires_grad_(True)
    crit = classes.LeastSquares(R, dev)

    def kernel_path():
        pred.grad = None
        crit(img, pred).backward()

    def torch_path():  # the class's CPU branch, on the CUDA tensors
        pred.grad = None
        crit.energy_function(crit.batch_points(img), pred).mean().backward()

    return {"shape": "R%d_H%d_B%d" % (R, H, B),
            "points_per_image": round(float((torch.nn.functional.interpolate(img, size=(R, R)) > 0).sum()) / B, 1),
            "kernel_eager_ms": round(_eager_ms(kernel_path), 4),
            "torch_eager_ms": round(_eager_ms(torch_path), 4),
            "kernel_in_graph_us": round(bench.time_loss_call(crit, img, B, dev, reps=10) * 1e3, 2)}


def _graph_us(fn, reps=20):
    """fn() captured once in a graph; device time per replay (events around `reps` replays)."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        g.replay()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps


def lm(dev, R=64, H=256, B=64):
    """One normal-equations call and a 10-iteration refine_lm, eagerly and inside a graph, next to the
    least_squares forward + backward call and to refine's 200 Adam steps (eager: it cannot be shorter
    than its 200 x ~8 launches), at the shapes of the leastsquares mode."""
    from sqr import fit
    p = torch.tensor(classes.sample_sq_params(np.random.default_rng(0), B), device=dev)
    img = losses.implicit_render(p, H, 1.5, 260).unsqueeze(1).contiguous()
    torch.manual_seed(0)
    pred = (p + 0.02 * torch.randn_like(p)).contiguous()
    gpred = pred.clone().requires_grad_(True)
    crit = classes.LeastSquares(R, dev)

    def fwd_bwd():
        gpred.grad = None
        crit(img, gpred).backward()

    res = {"shape": "R%d_H%d_B%d" % (R, H, B),
           "normal_eq_eager_ms": round(_eager_ms(lambda: losses.least_squares_normal_eq(img, pred, R)), 4),
           "normal_eq_in_graph_us": round(_graph_us(lambda: losses.least_squares_normal_eq(img, pred, R)), 2),
           "least_squares_fwd_bwd_eager_ms": round(_eager_ms(fwd_bwd), 4),
           "least_squares_fwd_bwd_in_graph_us": round(bench.time_loss_call(crit, img, B, dev, reps=10) * 1e3, 2),
           "refine_lm_10_eager_ms": round(_eager_ms(lambda: fit.refine_lm(img, pred, iters=10, render_size=R)), 4),
           "refine_lm_10_in_graph_us": round(_graph_us(lambda: fit.refine_lm(img, pred, iters=10, render_size=R)), 2),
           "refine_adam_200_eager_ms": round(_eager_ms(lambda: fit.refine(img, pred, steps=200, render_size=R),
                                                       warmup=1, reps=3), 3)}
    _, before, after_lm = fit.refine_lm(img, pred, iters=10, render_size=R)
    _, _, after_adam = fit.refine(img, pred, steps=200, render_size=R)
    res["energy_mean"] = {"start_projected": before.mean().item(), "lm_10": after_lm.mean().item(),
                          "adam_200": after_adam.mean().item()}
    return res


def recover(dev, R=64, H=256, B=64, iters=30):
    """sqr.fit.recover (the starts, one refinement of all 3 B samples, the selection) eagerly and inside a graph,
    next to the starts alone and to one refine_lm with the same `iters` from labels + N(0, 0.02), at the shapes
    of the lm mode, on scanner-style images of random labels."""
    from sqr import fit
    p = torch.tensor(classes.sample_sq_params(np.random.default_rng(0), B), device=dev)
    img = losses.scan_render(p, H, 255).unsqueeze(1).contiguous()
    torch.manual_seed(0)
    pred = (p + 0.02 * torch.randn_like(p)).contiguous()
    res = {"shape": "R%d_H%d_B%d" % (R, H, B), "iters": iters,
           "points_per_image": round(float((torch.nn.functional.interpolate(img, size=(R, R)) > 0).sum()) / B, 1),
           "starts_eager_ms": round(_eager_ms(lambda: losses.lsq_starts(img, R)), 4),
           "starts_in_graph_us": round(_graph_us(lambda: losses.lsq_starts(img, R)), 2),
           "refine_lm_eager_ms": round(_eager_ms(lambda: fit.refine_lm(img, pred, iters=iters, render_size=R)), 4),
           "refine_lm_in_graph_us": round(_graph_us(lambda: fit.refine_lm(img, pred, iters=iters, render_size=R)), 2),
           "recover_eager_ms": round(_eager_ms(lambda: fit.recover(img, iters=iters, render_size=R)), 4),
           "recover_in_graph_us": round(_graph_us(lambda: fit.recover(img, iters=iters, render_size=R)), 2)}
    res["recover_over_refine_lm_in_graph"] = round(res["recover_in_graph_us"] / res["refine_lm_in_graph_us"], 3)
    out, energy, index, info = fit.recover(img, iters=iters, render_size=R, return_info=True)
    iou = classes.IoUAccuracy(64, dev, reduce=False)(p, out)
    res["energy_mean"] = {"starts": info["energy_before"][0].mean().item(), "recovered": energy.mean().item()}
    res["winning_start_counts"] = torch.bincount(index.long(), minlength=3).tolist()
    res["iou64_mean"] = round(iou.mean().item(), 4)
    res["iou64_share_above_0.9"] = round((iou >= 0.9).double().mean().item(), 4)
    return res


def recover_multi(dev, R=64, H=256, B=64, iters=30):
    """The recover mode's batch: sqr.fit.recover (three starts, selected by energy), the same three starts with the
    score, the six-start scored recovery, free_space_energy of the six results, and lm_refine_multi over 3 B
    samples against three refine_lm calls of B."""
    from sqr import fit
    p = torch.tensor(classes.sample_sq_params(np.random.default_rng(0), B), device=dev)
    img = losses.scan_render(p, H, 255).unsqueeze(1).contiguous()
    kw = dict(iters=iters, render_size=R)
    six = lambda: fit.recover(img, starts="depth", free_space=1.0, **kw)  # noqa: E731
    three_multi = lambda: fit.recover(img, starts="classic", free_space=1.0, **kw)  # noqa: E731
    out6, e6, i6, info = fit.recover(img, starts="depth", free_space=1.0, return_info=True, **kw)
    flat = info["params"].reshape(-1, 12).contiguous()
    st3 = info["starts"][:3].contiguous()

    def three_refines():
        for k in range(3):
            fit.refine_lm(img, st3[k], **kw)

    res = {"shape": "R%d_H%d_B%d" % (R, H, B), "iters": iters,
           "recover_eager_ms": round(_eager_ms(lambda: fit.recover(img, **kw)), 4),
           "recover_in_graph_us": round(_graph_us(lambda: fit.recover(img, **kw)), 2),
           "recover_3_batched_scored_eager_ms": round(_eager_ms(three_multi), 4),
           "recover_3_batched_scored_in_graph_us": round(_graph_us(three_multi), 2),
           "recover_6_scored_eager_ms": round(_eager_ms(six), 4),
           "recover_6_scored_in_graph_us": round(_graph_us(six), 2),
           "free_space_6B_eager_ms": round(_eager_ms(lambda: losses.free_space_energy(img, flat, R)), 4),
           "free_space_6B_in_graph_us": round(_graph_us(lambda: losses.free_space_energy(img, flat, R)), 2),
           "refine_3_separate_in_graph_us": round(_graph_us(three_refines), 2),
           "refine_3_batched_in_graph_us": round(_graph_us(
               lambda: losses.lm_refine_multi(img, st3, R, iters, 1e-3, 10.0, 0.1)), 2)}
    res["recover_6_over_recover_in_graph"] = round(res["recover_6_scored_in_graph_us"] / res["recover_in_graph_us"], 3)
    acc = classes.IoUAccuracy(64, dev, reduce=False)
    out3 = fit.recover(img, **kw)[0]
    for name, out in (("recover", out3), ("recover_6_scored", out6)):
        iou = acc(p, out)
        res[name + "_iou64_mean"] = round(iou.mean().item(), 4)
        res[name + "_iou64_share_above_0.9"] = round((iou >= 0.9).double().mean().item(), 4)
    res["winning_start_counts"] = torch.bincount(i6.long(), minlength=6).tolist()
    res["energy_mean"] = {"point": e6.mean().item(), "free_space": info["winner_energy_fs"].mean().item()}
    return res


def scan(dev, S=256, B=256, host_images=16):
    from sqr import cpu
    p = torch.tensor(classes.sample_sq_params(np.random.default_rng(0), B), device=dev)
    img = losses.scan_render(p, S, 255)
    res = {"shape": "S%d_B%d" % (S, B), "foreground_share": round(float((img > 0).float().mean()), 4),
           # (windows of ~0.2 s and more: 400 calls of the half-millisecond render, 40 of the soft one)
           "scan_render_eager_ms": round(_eager_ms(lambda: losses.scan_render(p, S, 255), reps=400), 4),
           "scan_render_in_graph_us": round(_graph_us(lambda: losses.scan_render(p, S, 255), reps=400), 2),
           "implicit_render_eager_ms": round(_eager_ms(lambda: losses.implicit_render(p, S, 1.5, 260), reps=40), 4),
           "implicit_render_in_graph_us": round(_graph_us(lambda: losses.implicit_render(p, S, 1.5, 260), reps=40),
                                                2)}
    threads = torch.get_num_threads()
    torch.set_num_threads(16)
    ph = p[:host_images].cpu()
    cpu.scan_render(ph[:1], S, 255)
    t0 = time.perf_counter()
    cpu.scan_render(ph, S, 255)
    res["host_float64_ms_per_%d_images" % host_images] = round((time.perf_counter() - t0) * 1e3, 1)
    res["host_threads"] = 16
    torch.set_num_threads(threads)
    return res


def online(dev, S=256, B=64):
    from sqr import _lib, data
    src = data.OnlineSource(B, dev, size=S)
    img, lab = src.next()
    labels = lab.clone()  # scan_render alone: the same labels every call, into the source's image buffer

    def render_only():
        _lib.check(_lib.lib().sqr_scan_render(_lib.ptr(labels), B, S, 255, _lib.ptr(src.images),
                                              _lib.stream_ptr(dev)), "sqr_scan_render")

    def draw_only():
        data.sq_sample(src._pos, src.seed, src.substream, 0, B, src.labels)
        data.stream_advance(src._pos, B)

    res = {"shape": "S%d_B%d" % (S, B), "foreground_share": round(float((img > 0).float().mean()), 4),
           "next_eager_ms": round(_eager_ms(src.next, reps=400), 4),
           "scan_render_eager_ms": round(_eager_ms(render_only, reps=400), 4),
           "sample_advance_eager_ms": round(_eager_ms(draw_only, reps=400), 4),
           "next_in_graph_us": round(_graph_us(src.next, reps=400), 2),
           "scan_render_in_graph_us": round(_graph_us(render_only, reps=400), 2),
           "sample_advance_in_graph_us": round(_graph_us(draw_only, reps=400), 2)}
    res["next_minus_render_in_graph_us"] = round(res["next_in_graph_us"] - res["scan_render_in_graph_us"], 2)
    res["position_after"] = src.position()
    return res


def points(dev, R=64, H=256, B=64, iters=30):
    """recover_points on the images' slots as lists [B,R^2,3] (NaN where a pixel is not > 0) next to recover on the
    images, and point_energy next to the plain-torch energy on the same points (there as ragged [3,N_i] lists,
    built outside the timed region)."""
    from sqr import fit
    p = torch.tensor(classes.sample_sq_params(np.random.default_rng(0), B), device=dev)
    img = losses.scan_render(p, H, 255).unsqueeze(1).contiguous()
    z = torch.nn.functional.interpolate(img, size=(R, R), mode="nearest")[:, 0]
    rows, cols = torch.meshgrid(torch.arange(R, device=dev), torch.arange(R, device=dev), indexing="ij")
    lst = torch.stack([(cols.float() / R).expand_as(z), (1 - rows.float() / R).expand_as(z), z], dim=-1)
    lst = torch.where((z > 0)[..., None], lst, torch.full_like(lst, float("nan"))).reshape(B, R * R, 3).contiguous()
    crit = classes.LeastSquares(R, dev)
    ragged = crit.batch_points(img)
    torch.manual_seed(0)
    pred = (p + 0.02 * torch.randn_like(p)).requires_grad_(True)

    def kernel_energy():
        pred.grad = None
        losses.point_energy(lst, pred).backward()

    def torch_energy():
        pred.grad = None
        crit.energy_function(ragged, pred).mean().backward()

    a = fit.recover(img, iters=iters, render_size=R)
    b = fit.recover_points(lst, iters=iters)
    res = {"shape": "P%d_B%d" % (R * R, B), "iters": iters,
           "points_per_cloud": round(float((z > 0).sum()) / B, 1),
           "list_equals_image_bitwise": all(torch.equal(x, y) for x, y in zip(a, b)),
           "recover_eager_ms": round(_eager_ms(lambda: fit.recover(img, iters=iters, render_size=R)), 4),
           "recover_points_eager_ms": round(_eager_ms(lambda: fit.recover_points(lst, iters=iters)), 4),
           "recover_in_graph_us": round(_graph_us(lambda: fit.recover(img, iters=iters, render_size=R)), 2),
           "recover_points_in_graph_us": round(_graph_us(lambda: fit.recover_points(lst, iters=iters)), 2),
           "point_energy_fwd_bwd_eager_ms": round(_eager_ms(kernel_energy), 4),
           "torch_energy_fwd_bwd_eager_ms": round(_eager_ms(torch_energy), 4)}
    res["recover_points_over_recover_in_graph"] = round(res["recover_points_in_graph_us"] / res["recover_in_graph_us"], 4)
    return res


PART_CENTRES = ((0.25, 0.25, 0.3), (0.75, 0.3, 0.6), (0.45, 0.75, 0.5), (0.75, 0.75, 0.25))


def _parts_scene(dev, B, M, per_body):
    """B clouds of M bodies: golden clouds (b + m) mod 8 shrunk by 0.7 about their labels' t and moved to
    PART_CENTRES, every cloud's 512 points repeated to per_body, the M per_body slots permuted."""
    d = np.load(os.path.join(ROOT, "tests", "golden", "points.npz"), allow_pickle=False)
    rng = np.random.default_rng(1)
    pts = np.empty((B, M * per_body, 3), np.float32)
    for b in range(B):
        bodies = []
        for m in range(M):
            i = (b + m) % 8
            cloud = (d["clouds"][i].astype(np.float64) - d["labels"][i][5:8]) * 0.7 + np.array(PART_CENTRES[m])
            bodies.append(np.tile(cloud, (-(-per_body // 512), 1))[:per_body])
        pts[b] = np.concatenate(bodies)[rng.permutation(M * per_body)]
    return torch.tensor(pts, device=dev)


def _torch_assign(pts, par):
    """sqr_pts_assign's labels in plain torch ops (no host wait): pts [B,P,3], par [B,M,12] -> [B,P] i32."""
    a, e = par[..., 0:3].clamp(0.05, 1), par[..., 3:5].clamp(0.1, 1)
    t = par[..., 5:8].clamp(0, 1)
    x, y, z, w = -par[..., 8], -par[..., 9], -par[..., 10], par[..., 11]
    rot = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                       2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                       2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(*par.shape[:2], 3, 3)
    d = pts[:, None] - t[:, :, None]
    v = torch.einsum("bmij,bmpj->bmpi", rot, d) / a[:, :, None]
    sq = v * v
    sq = torch.where(sq == 0, sq + 1e-4, sq)
    e1, e2 = e[..., 0, None], e[..., 1, None]
    f = ((sq[..., 0] ** (1 / e2) + sq[..., 1] ** (1 / e2)) ** (e2 / e1) + sq[..., 2] ** (1 / e1)) ** e1
    dist = d.norm(dim=-1) * (1 - f ** -0.5).abs()
    on = torch.isfinite(pts).all(-1)
    dist = torch.where(torch.isfinite(dist), dist, torch.full_like(dist, float("inf")))
    return torch.where(on, dist.argmin(1), torch.full_like(on, -1, dtype=torch.int64)).to(torch.int32)


def parts(dev, B=8, M=4, P=4096, rounds=3, iters0=30, iters=10):
    """sqr.fit.recover_parts eagerly and inside a replayed graph, next to what could be done before it with the
    same fits: recover_points then refine_points on the B M NaN-masked copies of the clouds, the assignment between
    the rounds in torch ops, from the same (precomputed) seeding labels; the assignment kernel alone next to those
    torch ops; and one part's normal-equations launch (B M virtual clouds) next to one cloud's (B clouds)."""
    from sqr import fit
    pts = _parts_scene(dev, B, M, P // M)
    seed_labels, _, _ = losses.pts_seed(pts, M)
    nan = torch.full_like(pts, float("nan"))
    part_ids = torch.arange(M, device=dev, dtype=torch.int32)[None, :, None]

    def masked(labels):
        return torch.where((labels[:, None, :] == part_ids)[..., None], pts[:, None], nan[:, None]).reshape(B * M, P, 3)

    def baseline():
        labels = seed_labels
        par = fit.recover_points(masked(labels), iters=iters0)[0]
        labels = _torch_assign(pts, par.reshape(B, M, 12))
        for _ in range(1, rounds):
            par = fit.refine_points(masked(labels), par, iters=iters)[0]
            labels = _torch_assign(pts, par.reshape(B, M, 12))
        return par.reshape(B, M, 12), labels

    chain = lambda: fit.recover_parts(pts, M, rounds=rounds, iters0=iters0, iters=iters)  # noqa: E731
    chain_given = lambda: fit.recover_parts(pts, M, rounds=rounds, iters0=iters0, iters=iters,  # noqa: E731
                                            labels=seed_labels)
    par, labels, energy, info = fit.recover_parts(pts, M, rounds=rounds, iters0=iters0, iters=iters, return_info=True)
    bpar, blabels = baseline()
    flat = par.reshape(B * M, 12).contiguous()
    res = {"shape": "B%d_M%d_P%d" % (B, M, P), "rounds": rounds, "iters0": iters0, "iters": iters,
           "changed_per_round": info["changed"].sum(1).tolist(),
           "baseline_labels_equal": bool(torch.equal(labels, blabels)),
           "baseline_params_equal_bitwise": bool(torch.equal(par, bpar)),
           "energy_max": energy.max().item(),
           "recover_parts_eager_ms": round(_eager_ms(chain), 4),
           "recover_parts_from_labels_eager_ms": round(_eager_ms(chain_given), 4),
           "baseline_eager_ms": round(_eager_ms(baseline), 4),
           "recover_parts_in_graph_us": round(_graph_us(chain), 2),
           "recover_parts_from_labels_in_graph_us": round(_graph_us(chain_given), 2),
           "baseline_in_graph_us": round(_graph_us(baseline), 2),
           "seed_in_graph_us": round(_graph_us(lambda: losses.pts_seed(pts, M)), 2),
           "assign_in_graph_us": round(_graph_us(lambda: losses.pts_assign(pts, par), reps=200), 2),
           "torch_assign_in_graph_us": round(_graph_us(lambda: _torch_assign(pts, par), reps=200), 2),
           "normal_eq_parts_in_graph_us": round(_graph_us(
               lambda: losses.pts_labeled_lm_refine(pts, None, labels, par, 0, 1e-3, 10.0, 0.1), reps=200), 2),
           "normal_eq_clouds_in_graph_us": round(_graph_us(
               lambda: losses.pts_lm_refine(pts, None, flat[:B].contiguous(), 0, 1e-3, 10.0, 0.1), reps=200), 2)}
    res["recover_parts_over_baseline_in_graph"] = round(
        res["recover_parts_from_labels_in_graph_us"] / res["baseline_in_graph_us"], 4)
    return res


def main():
    dev = torch.device("cuda", 0)
    out = {"env": {k: v for k, v in os.environ.items() if k.startswith("SQR_")}}
    if sys.argv[1:] == ["parts"]:
        for _ in range(2):  # every figure twice in one process: one JSON line per pass
            out["parts"] = parts(dev)
            print(json.dumps(out))
        return
    if sys.argv[1:] == ["online"]:
        for _ in range(2):  # every figure twice in one process: one JSON line per pass
            out["online"] = online(dev)
            print(json.dumps(out))
        return
    if sys.argv[1:] == ["points"]:
        for _ in range(2):  # every figure twice in one process: one JSON line per pass
            out["points"] = points(dev)
            print(json.dumps(out))
        return
    if sys.argv[1:] == ["scan"]:
        out["scan"] = scan(dev)
        print(json.dumps(out))
        return
    if sys.argv[1:] == ["recover-multi"]:
        out["recover_multi"] = recover_multi(dev)
        print(json.dumps(out))
        return
    if sys.argv[1:] == ["recover"]:
        out["recover"] = recover(dev)
        print(json.dumps(out))
        return
    if sys.argv[1:] == ["lm"]:
        out["lm"] = lm(dev)
        print(json.dumps(out))
        return
    if sys.argv[1:] == ["leastsquares"]:
        out["leastsquares"] = least_squares(dev)
        print(json.dumps(out))
        return
    for R, H, B in ((32, 256, 64), (64, 256, 64), (64, 512, 16)):
        p = torch.tensor(classes.sample_sq_params(np.random.default_rng(0), B), device=dev)
        img = losses.implicit_render(p, H, 1.5, 260).unsqueeze(1).contiguous()
        crit = classes.ImplicitLoss(R, dev, 1.5, 260)
        ms = bench.time_loss_call(crit, img, B, dev, reps=10)
        tps = B * R ** 3 * bench.LOSS_TRANSC_PER_VOXEL / (ms * 1e-3) / 1e12
        out["R%d_H%d_B%d" % (R, H, B)] = {"us": round(ms * 1e3, 2), "frac": round(tps / bench.PEAK_TRANSC_TPS, 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
