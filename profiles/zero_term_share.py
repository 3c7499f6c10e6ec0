"""Share z of a frame's samples whose term is exactly (0, 0, 0) — the path ends the deferred-fold kernels do not queue
(csrc/rtm_path.h: SceneView::emit_mask).  CPU only: a seeded sample of the frame's (pixel, sample) streams through the
oracle's seam (tests/_oracle.py: path_trace_stream), the primary ray as the oracle's render forms it (rtmo_primary_dir,
sample index ((sx-1)*SS + (sy-1))*S + s, stream keyed by the global pixel index), repaired mode.

    python profiles/zero_term_share.py [--n 200000]        -> profiles/r5/zero_term.md quotes the output
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _oracle  # noqa: E402


def share(scene, w, h, s, ss, max_bounces, n, seed=0x5EED, pick_seed=1):
    st, arr, cnt = _oracle.load_scene(_oracle.scene_path(scene), width=w, height=h, samples=s, super_samples=ss)
    L = _oracle.lib()
    rng = np.random.default_rng(pick_seed)
    xs, ys = rng.integers(0, w, n), rng.integers(0, h, n)
    ks = rng.integers(0, s * ss * ss, n)
    org = [st.camera.origin[k] for k in range(3)]
    d = (C.c_double * 3)()
    zero = casts = 0
    for x, y, k in zip(xs, ys, ks):
        sub = int(k) // s
        L.rtmo_primary_dir(C.byref(st), int(x), int(y), sub // ss + 1, sub % ss + 1, d)
        rad, c = _oracle.path_trace_stream(arr, cnt, _oracle.MODE_REPAIRED, max_bounces, org, [d[0], d[1], d[2]], seed,
                                           int(y) * w + int(x), int(k))
        zero += rad[0] == 0.0 and rad[1] == 0.0 and rad[2] == 0.0
        casts += c["casts"]
    z = zero / n
    return z, (z * (1 - z) / n) ** 0.5, casts / n


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    a = ap.parse_args()
    for label, cfg in (("headline 1920x1080 @ 1024 spp, max_bounces 8", ("cornellBoxSetting.json", 1920, 1080, 64, 4, 8)),
                       ("configs[1] 512x512 @ 256 spp, max_bounces 8", ("cornellBoxSetting.json", 512, 512, 16, 4, 8)),
                       ("configs[1] 512x512 @ 256 spp, unlimited depth", ("cornellBoxSetting.json", 512, 512, 16, 4, -1))):
        z, se, cps = share(*cfg, n=a.n)
        print(f"{label}: z = {z:.4f} +- {se:.4f} (1 sigma, {a.n} samples), {cps:.3f} casts per sample", flush=True)
