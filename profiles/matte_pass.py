"""What the coverage AOVs cost (rtm_render_mattes, rtm_matte, rtm_composite) at the headline frame size.

The headline Cornell frame's geometry (cornellBoxSetting.json, 1920x1080) at SS 1, 2, 4 and 8: rtm_render_mattes with the
default 4 layers and with 8, and rtm_render_aov of the same tree beside them.  Both do SS^2 first-hit searches per pixel
through the same search, so the ratio of the two is what filing, sorting and ranking the ids costs (the AOV pass instead sums
normals and colours).  Then rtm_matte over the SS 4 layers (one id, 64 ids) and rtm_composite (constant and image background,
f32 + u8).  Every pass is timed with device events on the stream, best of --reps after a warm-up, and the planes of every
repetition are checked byte for byte against the first.  The times are WARM: the 7-sphere scene and, for the two small
kernels, the 8 to 66 MB of planes stay in the Infinity Cache between repetitions.  There is no bar: nothing was measured
before this.  Writes profiles/matte_pass.json and prints it.

    python profiles/matte_pass.py [--reps 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "matte_pass.json")
W, H = 1920, 1080


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def best(fn, reps, same):
    """(the first call's output, best time of `reps` further calls, whether every call gave the first one's bytes)."""
    import torch
    first, _ = timed(fn)  # the warm-up
    ms, ok = [], True
    for _ in range(reps):
        out, t = timed(fn)
        ms.append(t)
        ok = ok and all(torch.equal(out[k], first[k]) for k in same(first))
    return first, round(min(ms), 4), ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import raytracingmin_amd as rtm
    data = rtm.LoadData(os.path.join(ROOT, "scenes", "cornellBoxSetting.json")).data
    data.width, data.height, data.samples = W, H, 64
    r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=0x5EED)
    row = {"config": f"cornellBoxSetting.json {W}x{H}; device ms are best of {args.reps}, warm", "device": torch.cuda.get_device_name(0),
           "identical": True, "render_mattes": {}}
    layers4 = None
    for ss in (1, 2, 4, 8):
        data.superSamples = ss
        entry = {}
        _, entry["aov_ms"], ok = best(r.render_aov, args.reps, lambda o: o)
        row["identical"] &= ok
        for layers in (4, 8):
            out, entry[f"mattes_layers{layers}_ms"], ok = best(lambda: r.render_mattes(layers), args.reps, lambda o: o)
            row["identical"] &= ok
            if (ss, layers) == (4, 4):
                layers4 = out
        entry["mattes_over_aov"] = round(entry["mattes_layers4_ms"] / entry["aov_ms"], 4)
        row["render_mattes"][f"ss{ss}"] = entry
    ids = sorted(set(layers4["id"].unique().tolist()) - {-1})
    as_dict = lambda t: {"matte": t}
    row["matte"] = {}
    for name, sel in (("one_id", ids[:1]), ("64_ids", (ids * 64)[:64])):
        _, row["matte"][f"{name}_ms"], ok = best(lambda: as_dict(rtm.matte(layers4["id"], layers4["coverage"], sel)), args.reps, lambda o: o)
        row["identical"] &= ok
    color = torch.rand((H, W, 3), dtype=torch.float32, device="cuda")
    image = torch.rand((H, W, 3), dtype=torch.float32, device="cuda")
    row["composite"] = {}
    for name, bg in (("constant", (0.2, 0.4, 0.8)), ("image", image)):
        _, row["composite"][f"{name}_f32_u8_ms"], ok = best(lambda: rtm.composite(color, layers4["alpha"], bg, want=("f32", "u8")),
                                                           args.reps, lambda o: o)
        row["identical"] &= ok
    row["identical"] = bool(row["identical"])
    text = json.dumps(row, indent=1)
    with open(OUT, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if row["identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
