"""What a pass of a progressive frame costs (rtm_render_scene_samples).

The headline frame (cornellBoxSetting.json, 1920x1080, S=64, SS=4, depth cap 8) as 1, 4 and 16 passes for variants 0 and
18, and BASELINE configs[4] (the 100 000-sphere stress scene, 1080p x 256 spp, depth cap 8: the uniform-grid kernel) as 1 and
2 passes.  Every pass is timed with device events on the stream; every final frame is checked byte for byte (f64, f32, u8)
against the one-shot frame of the same run.  Prints one JSON object per configuration.

    python profiles/progressive_passes.py [--reps 2] [--no-c5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frame_in_passes(r, bounds, accum, want):
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(bounds) + 1)]
    ev[0].record()
    out = None
    for i, (a, b) in enumerate(bounds):
        out, _ = r.render_samples_device(a, b, accum, want=want, stats=False)
        ev[i + 1].record()
    torch.cuda.synchronize()
    per = [ev[i].elapsed_time(ev[i + 1]) for i in range(len(bounds))]
    return out, per


def one_shot(r, want):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out, _ = r.render_rows_device(want=want, stats=False)
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def run(name, r, pass_counts, reps):
    import torch
    from raytracingmin_amd.renderer import plan_passes
    want = ("f64", "f32", "u8")
    ref, _ = one_shot(r, want)  # (also the warm-up: work buffers, scene upload)
    ref = {k: v.cpu().numpy() for k, v in ref.items()}
    n = r.total_samples()
    accum = torch.empty((r.data.height, r.data.width, 3), dtype=torch.float64, device="cuda")
    row = {"config": name, "spp": n, "one_shot_ms": [], "passes": {}}
    for _ in range(reps):
        row["one_shot_ms"].append(round(one_shot(r, ("f32", "u8"))[1], 3))
    for p in pass_counts:
        bounds = plan_passes(n, passes=p)
        res = {"total_ms": [], "per_pass_ms": None, "identical": True}
        for _ in range(reps):
            out, per = frame_in_passes(r, bounds, accum, ("f32", "u8"))
            res["total_ms"].append(round(sum(per), 3))
            res["per_pass_ms"] = [round(v, 3) for v in per]
            got = {"f64": accum.cpu().numpy(), "f32": out["f32"].cpu().numpy(), "u8": out["u8"].cpu().numpy()}
            same = (np.array_equal(got["f64"].view(np.uint64), ref["f64"].view(np.uint64)) and
                    np.array_equal(got["f32"].view(np.uint32), ref["f32"].view(np.uint32)) and
                    np.array_equal(got["u8"], ref["u8"]))
            res["identical"] = res["identical"] and bool(same)
        best1 = min(row["one_shot_ms"])
        res["overhead_vs_one_shot"] = round(min(res["total_ms"]) / best1 - 1.0, 4)
        row["passes"][str(p)] = res
    print(json.dumps(row), flush=True)
    return all(v["identical"] for v in row["passes"].values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--no-c5", action="store_true")
    args = ap.parse_args()
    import raytracingmin_amd as rtm
    data = rtm.LoadData(os.path.join(ROOT, "scenes", "cornellBoxSetting.json")).data
    data.width, data.height, data.samples, data.superSamples = 1920, 1080, 64, 4
    ok = True
    for variant in (0, 18):
        r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=0x5EED, variant=variant)
        ok &= run(f"headline variant {variant}", r, (1, 4, 16), args.reps)
    if not args.no_c5:
        stress = rtm.make_stress_scene(n=100_000, seed=12345)
        stress.width, stress.height, stress.samples, stress.superSamples = 1920, 1080, 256, 1
        r = rtm.Renderer(stress, mode="repaired", max_bounces=8, seed=0x5EED)
        ok &= run("c5 100k spheres 1080p x 256 spp (variant 0: grid)", r, (1, 2), args.reps)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
