"""What the on-device frame comparison (rtm_compare) costs at 1080p, beside the route it replaces.

Two synthetic 1920x1080 frames (a long-tailed HDR frame and the same plus noise), as float32 and as float64.  For each dtype:
the full call (the record, SSIM's window passes included), the same call with the ABS map as well, the SSIM map, and the
ABS-map-only call — the one form of the call that runs no window pass, since the record always carries SSIM — each timed
with device events on the stream, best of --reps after a warm-up, the record's bytes of every repetition checked against
the first.  The route it replaces: both frames copied to the host and NumPy's float64 `mse` and `outside` taken there
(wall clock, copies and arithmetic apart).  It is timed against nothing else and there is no bar.  Writes
profiles/compare_pass.json and prints it.

    python profiles/compare_pass.py [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "compare_pass.json")
W, H = 1920, 1080


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
    rng = np.random.default_rng(1080)
    base = 8 * rng.random((H, W, 3)) ** 4
    noise = 0.05 * rng.standard_normal((H, W, 3))
    row = {"config": f"{W}x{H}, synthetic HDR frame against itself plus noise; device ms are best of {args.reps}",
           "device": torch.cuda.get_device_name(0), "deterministic": True}
    for name, dtype in (("f32", np.float32), ("f64", np.float64)):
        a_host, b_host = base.astype(dtype), (base + noise).astype(dtype)
        a, b = torch.from_numpy(a_host).cuda(), torch.from_numpy(b_host).cuda()
        entry = {"frame_bytes_each": a_host.nbytes}
        calls = {"result_ms": dict(want=("result",)), "result_and_abs_map_ms": dict(want=("result", "map"), map="abs"),
                 "result_and_ssim_map_ms": dict(want=("result", "map"), map="ssim"),
                 "abs_map_only_no_ssim_ms": dict(want=("map",), map="abs")}
        for key, kw in calls.items():
            first, _ = timed(lambda: rtm.compare(a, b, **kw))  # the warm-up
            ms = []
            for _ in range(args.reps):
                out, t = timed(lambda: rtm.compare(a, b, **kw))
                ms.append(t)
                if "result" in out and not torch.equal(out["result"], first["result"]):
                    row["deterministic"] = False
            entry[key] = round(min(ms), 4)
            if key == "result_ms":
                entry["result"] = rtm.compare_result(out["result"])
        # the route this replaces: two device-to-host copies, then NumPy in float64
        copies, maths = [], []
        for _ in range(max(2, args.reps // 2)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ah, bh = a.cpu().numpy(), b.cpu().numpy()
            t1 = time.perf_counter()
            d = np.abs(ah.astype(np.float64) - bh.astype(np.float64))
            mse = float(np.mean(d * d))
            outside = int((d.max(axis=2) > 1e-4).sum())
            t2 = time.perf_counter()
            copies.append((t1 - t0) * 1e3)
            maths.append((t2 - t1) * 1e3)
        entry["host_route"] = {"copies_ms": round(min(copies), 3), "numpy_ms": round(min(maths), 3),
                               "total_ms": round(min(copies) + min(maths), 3), "mse": mse, "outside": outside}
        entry["host_route_agrees"] = bool(outside == entry["result"]["outside"]
                                          and abs(mse - entry["result"]["mse"]) <= 1e-9 * mse)
        row[name] = entry
    text = json.dumps(row, indent=1)
    with open(OUT, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if row["deterministic"] and row["f32"]["host_route_agrees"] and row["f64"]["host_route_agrees"] else 1


if __name__ == "__main__":
    sys.exit(main())
