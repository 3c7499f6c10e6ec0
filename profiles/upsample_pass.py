"""What a low-resolution preview costs and gives (rtm_upsample), beside the full render and denoise of the same frame.

The headline Cornell frame (cornellBoxSetting.json, 1920x1080, S=64, SS=4, depth cap 8).  For f = 2 and f = 4: the render at
1 / f of the resolution, the AOV calls at both resolutions, rtm_denoise of the low frame and rtm_upsample, each at its
defaults; and the full route: the full render and rtm_denoise.  Every stage is timed with device events on the stream, best
of --reps after a warm-up; the output bytes of every repetition of the upsampler are checked against the first.  Quality is
the RMSE (values clipped to [0, 1]) of each route against the full undenoised frame.  --sweep adds the sigma_spatial sweep
that chose the default: the Cornell box at 256x256, truth SS 2 x S 256, the preview from 128x128 at SS 2 x S 4.  Prints one
JSON object.

    python profiles/upsample_pass.py [--reps 5] [--sweep]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENE = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def best_of(fn, reps):
    out, _ = timed(fn)  # the warm-up
    ms = []
    for _ in range(reps):
        out, t = timed(fn)
        ms.append(t)
    return out, round(min(ms), 4)


def renderer(rtm, w, h, samples, ss):
    data = rtm.LoadData(SCENE).data
    data.width, data.height, data.samples, data.superSamples = w, h, samples, ss
    return rtm.Renderer(data, mode="repaired", max_bounces=8, seed=0x5EED)


def rmse(a, b):
    clip = lambda t: np.clip(t.cpu().numpy().astype(np.float64), 0.0, 1.0)
    return round(float(np.sqrt(np.mean((clip(a) - clip(b)) ** 2))), 6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    import raytracingmin_amd as rtm
    W, H, S, SS = 1920, 1080, 64, 4
    full = renderer(rtm, W, H, S, SS)
    frame, full_render_ms = best_of(lambda: full.render_rows_device(want=("f32",), stats=False)[0]["f32"], args.reps)
    aov_high, aov_high_ms = best_of(full.render_aov, args.reps)
    den, full_denoise_ms = best_of(lambda: rtm.denoise(frame, aov_high)["f32"], args.reps)
    row = {"config": "headline cornell 1080p x 1024 spp: preview routes at the default sigmas against the full route",
           "full": {"render_ms": full_render_ms, "aov_ms": aov_high_ms, "denoise_ms": full_denoise_ms,
                    "total_ms": round(full_render_ms + aov_high_ms + full_denoise_ms, 4), "rmse_vs_full_frame": rmse(den, frame)}}
    ok = True
    for f in (2, 4):
        lowr = renderer(rtm, W // f, H // f, S, SS)
        low, low_render_ms = best_of(lambda: lowr.render_rows_device(want=("f32",), stats=False)[0]["f32"], args.reps)
        aov_low, aov_low_ms = best_of(lowr.render_aov, args.reps)
        low_dn, low_denoise_ms = best_of(lambda: rtm.denoise(low, aov_low)["f32"], args.reps)
        call = lambda: rtm.upsample(low_dn, aov_low, aov_high, factor=f, want=("f32", "u8"))
        first = {k: v.cpu().numpy() for k, v in call().items()}
        ms = []
        for _ in range(args.reps):
            up, t = timed(call)
            ms.append(t)
            ok = ok and all(np.array_equal(up[k].cpu().numpy().view(np.uint8), first[k].view(np.uint8)) for k in first)
        total = low_render_ms + aov_low_ms + low_denoise_ms + aov_high_ms + min(ms)
        row[f"preview_f{f}"] = {"low_render_ms": low_render_ms, "aov_low_ms": aov_low_ms, "aov_high_ms": aov_high_ms,
                                "low_denoise_ms": low_denoise_ms, "upsample_ms": round(min(ms), 4), "total_ms": round(total, 4),
                                "rmse_vs_full_frame": rmse(up["f32"], frame)}
    if args.sweep:
        truth = renderer(rtm, 256, 256, 256, 2)
        t32, t_aov = truth.render_rows_device(want=("f32",), stats=False)[0]["f32"], truth.render_aov()
        lowr = renderer(rtm, 128, 128, 4, 2)
        l_aov = lowr.render_aov()
        low_dn = rtm.denoise(lowr.render_rows_device(want=("f32",), stats=False)[0]["f32"], l_aov)["f32"]
        row["sigma_spatial_sweep_cornell_256"] = {
            str(s): rmse(rtm.upsample(low_dn, l_aov, t_aov, factor=2, sigma_spatial=s)["f32"], t32) for s in (0.35, 0.5, 0.7, 1.0)}
    row["identical"] = bool(ok)
    print(json.dumps(row), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
