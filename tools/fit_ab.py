"""Two builds of libsqr.so loaded side by side in one process on the GPU: every output of the image fitting calls
(sqr_lsq_starts, sqr_least_squares_normal_eq, sqr_lsq_lm_refine, sqr_lsq_recover_multi) on the ten example images
at R = 8, 32 and 64, compared byte for byte.

    tools/build_ab_base.sh            # the parent's library -> tools/ab_lib/libsqr.so
    python tools/fit_ab.py [BASE_LIB [NEW_LIB]] > profiles/NAME.txt

Only the symbols named above (and their workspace sizes) are bound, so a library from before or after a change
of the rest of the interface loads.  Exit status 1 if any array differs."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sq-recovery_amd"))

from sqr import _lib  # noqa: E402

NAMES = ("sqr_last_error_string", "sqr_lsq_starts_workspace_bytes", "sqr_lsq_starts",
         "sqr_least_squares_normal_eq_workspace_bytes", "sqr_least_squares_normal_eq",
         "sqr_lsq_lm_refine_workspace_bytes", "sqr_lsq_lm_refine", "sqr_lsq_recover_multi_workspace_bytes",
         "sqr_lsq_recover_multi")


def load(path):
    h = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
    for n in NAMES:
        fn = getattr(h, n)
        fn.restype, fn.argtypes = _lib.SIGNATURES[n]
    return h


def run(L, img, pred, R, dev):
    """Every output of the four calls as a dict of tensors."""
    ptr = _lib.ptr
    st = _lib.stream_ptr(dev)
    B, H, W = img.shape
    new = lambda dt, *s: torch.full(s, -7, dtype=dt, device=dev)  # noqa: E731
    f32, f64, i32 = torch.float32, torch.float64, torch.int32
    out = {}

    def ok(rc, what):
        assert rc == 0, (what, L.sqr_last_error_string())

    def ws_of(n):
        return torch.empty(max(n, 16), dtype=torch.uint8, device=dev)

    o = dict(starts=new(f32, 3, B, 12), count=new(i32, B), centroid=new(f64, B, 3), eigenvalues=new(f64, B, 3),
             frame=new(f64, B, 3, 3))
    n = L.sqr_lsq_starts_workspace_bytes(B, R)
    ok(L.sqr_lsq_starts(ptr(img), B, H, W, R, 1.0, ptr(o["starts"]), ptr(o["count"]), ptr(o["centroid"]),
                        ptr(o["eigenvalues"]), ptr(o["frame"]), ptr(ws_of(n)), n, st), "starts")
    out.update({"starts." + k: v for k, v in o.items()})
    o = dict(JtJ=new(f64, B, 12, 12), Jtr=new(f64, B, 12), energy=new(f64, B))
    n = L.sqr_least_squares_normal_eq_workspace_bytes(B, R)
    ok(L.sqr_least_squares_normal_eq(ptr(pred), ptr(img), B, H, W, R, ptr(o["JtJ"]), ptr(o["Jtr"]), ptr(o["energy"]),
                                     ptr(ws_of(n)), n, st), "normal_eq")
    out.update({"normal_eq." + k: v for k, v in o.items()})
    o = dict(params=new(f32, B, 12), before=new(f64, B), after=new(f64, B), accepted=new(i32, B))
    n = L.sqr_lsq_lm_refine_workspace_bytes(B, R)
    ok(L.sqr_lsq_lm_refine(ptr(pred), ptr(img), B, H, W, R, 10, 1e-3, 10.0, 0.1, ptr(o["params"]), ptr(o["before"]),
                           ptr(o["after"]), ptr(o["accepted"]), ptr(ws_of(n)), n, st), "lm_refine")
    out.update({"lm_refine." + k: v for k, v in o.items()})
    K = 7  # six starts and the prediction
    o = dict(params=new(f32, B, 12), energy=new(f64, B), energy_fs=new(f64, B), index=new(i32, B),
             all_starts=new(f32, K, B, 12), all_params=new(f32, K, B, 12), all_before=new(f64, K, B),
             all_after=new(f64, K, B), all_fs=new(f64, K, B), all_score=new(f64, K, B), all_accepted=new(i32, K, B))
    n = L.sqr_lsq_recover_multi_workspace_bytes(K, B, R)
    ok(L.sqr_lsq_recover_multi(ptr(img), B, H, W, R, 30, 6, 1.0, 1.0, ptr(pred), 1, 1e-3, 10.0, 0.1, 1.0, 1.0 / 255.0,
                               *[ptr(o[k]) for k in ("params", "energy", "energy_fs", "index", "all_starts",
                                                     "all_params", "all_before", "all_after", "all_fs", "all_score",
                                                     "all_accepted")], ptr(ws_of(n)), n, st), "recover_multi")
    out.update({"recover_multi." + k: v for k, v in o.items()})
    torch.cuda.synchronize()
    return out


def main():
    base = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tools", "ab_lib", "libsqr.so")
    here = sys.argv[2] if len(sys.argv) > 2 else _lib.LIB_PATH
    dev = torch.device("cuda", 0)
    A, B = load(base), load(here)
    d = np.load(os.path.join(ROOT, "tests", "golden", "example_images.npz"), allow_pickle=False)
    img = torch.tensor(d["images"].astype(np.float32) / 255.0, device=dev).contiguous()
    rng = np.random.default_rng(0)
    pred = torch.tensor((d["labels"] + 0.05 * rng.normal(size=d["labels"].shape)).astype(np.float32), device=dev)
    print("base library (%s) against this tree's (%s), loaded side by side in one process on one MI355X; the ten "
          "example images; every array compared byte for byte" % (os.path.relpath(base, ROOT),
                                                                  os.path.relpath(here, ROOT)))
    bad, n = [], 0
    for R in (8, 32, 64):
        a, b = run(A, img, pred, R, dev), run(B, img, pred, R, dev)
        assert set(a) == set(b)
        for k in sorted(a):
            same = a[k].dtype == b[k].dtype and torch.equal(a[k].reshape(-1).view(torch.uint8),
                                                            b[k].reshape(-1).view(torch.uint8))
            written = not bool((a[k] == -7).all())
            n += 1
            name = "R%d.%s" % (R, k)
            if not (same and written):
                bad.append(name)
            print("%-40s %-8s %-14s %s" % (name, str(a[k].dtype).replace("torch.", ""),
                                           "x".join(str(s) for s in a[k].shape),
                                           "identical" if same and written else "DIFFERENT" if written else "NOT WRITTEN"))
    print("%d arrays, %d differ: %s" % (n, len(bad), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
