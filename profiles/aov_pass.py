"""What the first-hit feature buffers cost (rtm_render_aov), beside the render of the same frame.

The headline Cornell frame (cornellBoxSetting.json, 1920x1080, S=64, SS=4, depth cap 8) with its AOV pass at SS 1 and at the
frame's own SS 4, and BASELINE configs[4] (the 100 000-sphere stress scene, 1080p x 256 spp, SS 1, depth cap 8: the AOV pass
through the uniform grid).  Every pass is timed with device events on the stream; the AOV planes of every repetition are
checked byte for byte against the first.  Prints one JSON object per configuration.

    python profiles/aov_pass.py [--reps 5] [--no-c5]
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


def run(name, r, aov_ss, reps):
    frame_ss = r.data.superSamples
    render_ms = [round(timed(lambda: r.render_rows_device(want=("f32", "u8"), stats=False))[1], 3) for _ in range(reps + 1)][1:]
    row = {"config": name, "render_ms": render_ms, "aov": {}}
    ok = True
    for ss in aov_ss:
        r.data.superSamples = ss
        ref = {k: v.cpu().numpy() for k, v in timed(r.render_aov)[0].items()}  # (also the warm-up)
        ms = []
        for _ in range(reps):
            out, t = timed(r.render_aov)
            ms.append(round(t, 3))
            ok = ok and all(np.array_equal(out[k].cpu().numpy().view(np.uint32), ref[k].view(np.uint32)) for k in ref)
        row["aov"][f"ss{ss}"] = {"ms": ms, "share_of_render": round(min(ms) / min(render_ms), 5),
                                 "hit_fraction": round(float((ref["object"] >= 0).mean()), 4)}
        r.data.superSamples = frame_ss
    row["identical"] = bool(ok)
    print(json.dumps(row), flush=True)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-c5", action="store_true")
    args = ap.parse_args()
    import raytracingmin_amd as rtm
    data = rtm.LoadData(os.path.join(ROOT, "scenes", "cornellBoxSetting.json")).data
    data.width, data.height, data.samples, data.superSamples = 1920, 1080, 64, 4
    ok = run("headline cornell 1080p x 1024 spp", rtm.Renderer(data, mode="repaired", max_bounces=8, seed=0x5EED), (1, 4),
             args.reps)
    if not args.no_c5:
        stress = rtm.make_stress_scene(n=100_000, seed=12345)
        stress.width, stress.height, stress.samples, stress.superSamples = 1920, 1080, 256, 1
        r = rtm.Renderer(stress, mode="repaired", max_bounces=8, seed=0x5EED)
        ok &= run("c5 100k spheres 1080p x 256 spp (variant 0: grid)", r, (1,), args.reps)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
