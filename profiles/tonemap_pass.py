"""What the display transform costs (rtm_tonemap), beside the render of the same frame.

The headline Cornell frame (cornellBoxSetting.json, 1920x1080, S=64, SS=4, depth cap 8): its render, then three calls on its
f32 at the default parameters: the statistics alone (stats output only: two launches), the map alone (a fixed exposure, so
the statistics are skipped: one launch) and the whole default call (three launches).  Every call is timed with device
events on the stream, best of --reps after a warm-up; the output bytes of every repetition are checked against the first.
The bandwidth is the bytes the kernels must move (12 B per pixel read by the statistics; 12 B read and 12 + 3 B written by
the map) over the time.  Prints one JSON object.

    python profiles/tonemap_pass.py [--reps 5] [--render-reps 1]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--render-reps", type=int, default=1)
    args = ap.parse_args()
    import raytracingmin_amd as rtm
    data = rtm.LoadData(os.path.join(ROOT, "scenes", "cornellBoxSetting.json")).data
    data.width, data.height, data.samples, data.superSamples = 1920, 1080, 64, 4
    r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=0x5EED)
    render_ms = []
    for _ in range(args.render_reps + 1):
        out, t = timed(lambda: r.render_rows_device(want=("f32",), stats=False)[0])
        render_ms.append(round(t, 3))
    render_ms = render_ms[1:]
    f32 = out["f32"]
    pix = data.width * data.height
    calls = {"statistics": (lambda: rtm.tonemap(f32, want=("stats",)), 12 * pix),
             "map": (lambda: rtm.tonemap(f32, exposure=0.0, want=("f32", "u8")), 27 * pix),
             "default": (lambda: rtm.tonemap(f32, want=("f32", "u8", "stats")), 39 * pix)}
    ok = True
    best, gbs = {}, {}
    for name, (call, nbytes) in calls.items():
        ref = {n: v.cpu().numpy() for n, v in timed(call)[0].items()}  # (also the warm-up)
        ms = []
        for _ in range(args.reps):
            got, t = timed(call)
            ms.append(round(t, 4))
            ok = ok and all(np.array_equal(got[n].cpu().numpy().view(np.uint8), ref[n].view(np.uint8)) for n in ref)
        best[name] = min(ms)
        gbs[name] = round(nbytes / (min(ms) * 1e-3) * 1e-9, 1)
    stats = rtm.tonemap_stats(rtm.tonemap(f32, want=("stats",))["stats"])
    row = {"config": "headline cornell 1080p x 1024 spp, display transform at the default parameters",
           "render_ms": render_ms,
           "tonemap_ms": best,
           "moved_mb": {name: round(nbytes * 1e-6, 1) for name, (_, nbytes) in calls.items()},
           "gb_per_s": gbs,
           "default_share_of_render": round(best["default"] / min(render_ms), 6),
           "frame_statistics": stats,
           "identical": bool(ok)}
    print(json.dumps(row), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
