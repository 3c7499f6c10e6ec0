"""What the on-device perceptual frame difference (rtm_flip) costs at 1080p, beside the route it replaces.

Two synthetic 1920x1080 display-referred frames (uniform noise with 10 % black pixels, and the same plus noise on 70 % of the
pixels), sRGB-encoded, at the default 67.02 pixels per degree (r = 10, rf = 9) and at 128 (r = 18, rf = 16, the largest
tables).  For each: the record alone and the record plus the map, each timed with device events on the stream, best of --reps
after a warm-up, the record's bytes of every repetition checked against the first.  The times are WARM: the two 25 MB frames
stay in the Infinity Cache between repetitions; the 232 MB of intermediate planes the call writes and reads back do not all
fit beside them.  There is one kernel form, so no second form's bits to compare.  The route it replaces: both frames copied to
the host and the NumPy float64 restatement (tests/_flip_ref.py) evaluated there, one repetition, wall clock, copies and
arithmetic apart.  It is timed against nothing else and there is no bar.  Writes profiles/flip_pass.json and prints it.

    python profiles/flip_pass.py [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "flip_pass.json")
W, H = 1920, 1080
TOLERANCE = 1e-9  # include/rtm.h


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import raytracingmin_amd as rtm
    import _flip_ref
    rng = np.random.default_rng(1080)
    a_host = rng.random((H, W, 3)).astype(np.float32)
    a_host[rng.random((H, W)) < 0.1] = 0.0
    b_host = (a_host + 0.05 * rng.standard_normal((H, W, 3)) * (rng.random((H, W, 1)) < 0.7)).astype(np.float32)
    a, b = torch.from_numpy(a_host).cuda(), torch.from_numpy(b_host).cuda()
    row = {"config": f"{W}x{H}, synthetic sRGB frame against itself plus noise; device ms are best of {args.reps}, warm "
                     "(the frames stay in the Infinity Cache between repetitions)",
           "device": torch.cuda.get_device_name(0), "deterministic": True, "frame_bytes_each": a_host.nbytes,
           "work_bytes": int(rtm.lib().rtm_flip_work_bytes(W, H))}
    for name, ppd in (("default_ppd", rtm.FLIP_DEFAULTS["pixels_per_degree"]), ("ppd_128", 128.0)):
        entry = {"pixels_per_degree": ppd, "r": _flip_ref.csf_radius(ppd), "rf": _flip_ref.feature_radius(ppd)}
        for key, want in (("result_ms", ("result",)), ("result_and_map_ms", ("result", "map"))):
            first, _ = timed(lambda: rtm.flip(a, b, pixels_per_degree=ppd, want=want))  # the warm-up
            ms = []
            for _ in range(args.reps):
                out, t = timed(lambda: rtm.flip(a, b, pixels_per_degree=ppd, want=want))
                ms.append(t)
                if not torch.equal(out["result"], first["result"]):
                    row["deterministic"] = False
            entry[key] = round(min(ms), 4)
        res = rtm.flip_result(out["result"])
        entry["result"] = {k: v for k, v in res.items() if k != "hist"}
        row[name] = entry
        if name != "default_ppd":
            continue
        # the route this replaces: two device-to-host copies, then the NumPy restatement in float64, once
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ah, bh = a.cpu().numpy(), b.cpu().numpy()
        t1 = time.perf_counter()
        ref, ref_map = _flip_ref.flip_ref(ah, bh, "srgb", ppd)
        t2 = time.perf_counter()
        got_map = out["map"].cpu().numpy().astype(np.float64)
        worst = max(abs(res[k] - ref[k]) for k in ("mean", "min", "max"))
        row["host_route"] = {"copies_ms": round((t1 - t0) * 1e3, 3), "numpy_ms": round((t2 - t1) * 1e3, 3),
                             "total_ms": round((t2 - t0) * 1e3, 3), "mean": ref["mean"], "max": ref["max"], "min": ref["min"]}
        row["device_against_host_route"] = {"worst_of_mean_min_max": worst, "map_worst": float(np.abs(got_map - ref_map).max()),
                                            "argmax_equal": (res["argmax_x"], res["argmax_y"]) == (ref["argmax_x"], ref["argmax_y"])}
        row["host_route_agrees"] = bool(worst <= TOLERANCE and row["device_against_host_route"]["map_worst"] <= TOLERANCE + 2.0 ** -25)
    text = json.dumps(row, indent=1)
    with open(OUT, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if row["deterministic"] and row["host_route_agrees"] else 1


if __name__ == "__main__":
    sys.exit(main())
