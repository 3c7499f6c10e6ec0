"""What the à-trous denoiser costs (rtm_denoise), beside the render of the same frame.

The headline Cornell frame (cornellBoxSetting.json, 1920x1080, S=64, SS=4, depth cap 8): its render, its AOVs, then the
denoise of its f32 at the default sigmas with K = 0 .. 5 levels.  Every call is timed with device events on the stream,
best of --reps after a warm-up; the output bytes of every repetition are checked against the first.  The per-level figure
is the difference of consecutive K.  Prints one JSON object.

    python profiles/denoise_pass.py [--reps 5]
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
    args = ap.parse_args()
    import raytracingmin_amd as rtm
    data = rtm.LoadData(os.path.join(ROOT, "scenes", "cornellBoxSetting.json")).data
    data.width, data.height, data.samples, data.superSamples = 1920, 1080, 64, 4
    r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=0x5EED)
    render_ms = []
    for _ in range(args.reps + 1):
        out, t = timed(lambda: r.render_rows_device(want=("f32",), stats=False)[0])
        render_ms.append(round(t, 3))
    render_ms = render_ms[1:]
    f32 = out["f32"]
    aov = r.render_aov()
    ok = True
    best = {}
    for k in range(6):
        call = lambda: rtm.denoise(f32, aov, iterations=k, want=("f32", "u8"))
        ref = {n: v.cpu().numpy() for n, v in timed(call)[0].items()}  # (also the warm-up)
        ms = []
        for _ in range(args.reps):
            got, t = timed(call)
            ms.append(round(t, 4))
            ok = ok and all(np.array_equal(got[n].cpu().numpy().view(np.uint8), ref[n].view(np.uint8)) for n in ref)
        best[k] = min(ms)
    row = {"config": "headline cornell 1080p x 1024 spp, denoise at the default sigmas",
           "render_ms": render_ms,
           "denoise_ms": {f"K{k}": best[k] for k in best},
           "per_level_ms": [round(best[k] - best[k - 1], 4) for k in range(1, 6)],
           "default_share_of_render": round(best[5] / min(render_ms), 5),
           "identical": bool(ok)}
    print(json.dumps(row), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
