"""What tile-adaptive sampling costs and buys (rtm_render_adaptive).

The headline frame (cornellBoxSetting.json, 1920x1080, S=64, SS=4, depth cap 8) and scenes/settingData.json at its own
960x504 x 100 spp, through variant 0, for a few thresholds at min_samples 16.  Per configuration: the one-shot frame's time;
the adaptive call's wall time and its mean samples per pixel; every pass replayed through rtm_render_scene_tiles with the
lists the sample map implies (time and Msamples/s per pass; the replay's frame is checked byte for byte against the
adaptive one); the checkpoints' time (adaptive kernel_ms minus the passes'), per checkpoint; and the RMSE against the
one-shot frame of the adaptive preview and of a uniform progressive preview that took the same time.  One JSON object per
configuration.

    python profiles/adaptive_pass.py [--thresholds 0.02,0.05,0.1,0.2] [--min-samples 16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rmse(a, b):
    a, b = np.clip(a.astype(np.float64), 0, 1), np.clip(b.astype(np.float64), 0, 1)
    return float(np.sqrt(np.mean((a - b) ** 2)))


def timed(fn):
    import torch
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    res = fn()
    e1.record()
    torch.cuda.synchronize()
    return res, e0.elapsed_time(e1)


def run(name, r, thresholds, m):
    import torch
    from _adaptive_ref import schedule
    n = r.total_samples()
    h, w = r.data.height, r.data.width
    (full, _), _ = timed(lambda: r.render_rows_device(want=("f32",), stats=False))  # warm-up
    (full, _), one_ms = timed(lambda: r.render_rows_device(want=("f32",), stats=False))
    full = full["f32"].cpu().numpy()
    rows = []
    for thr in thresholds:
        r.adaptive(thr, min_samples=m, want=("f32",))  # warm-up
        t0 = time.perf_counter()
        out, ts, st = r.adaptive(thr, min_samples=m, want=("f32",))
        wall_ms = (time.perf_counter() - t0) * 1e3
        ts_h = ts.cpu().numpy()
        mean_spp = st["samples"] / (w * h)
        # replay the passes: pass i lists the tiles whose count reaches b_i
        ends = schedule(n, m)
        acc = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
        passes, a = [], 0
        for b in ends:
            lst = np.nonzero(ts_h.ravel() >= b)[0].astype(np.int32)
            if lst.size == 0:
                break
            dev = torch.from_numpy(lst).cuda()
            (res, ps), ms = timed(lambda: r.render_tiles_device(dev, a, b, acc, want=("f32",), stats=True))
            passes.append({"samples": [a, b], "tiles": int(lst.size), "ms": round(ps["kernel_ms"], 3),
                           "msamples_per_s": round(ps["samples"] / ps["kernel_ms"] * 1e-3, 1)})
            a = b
        same = bool(np.array_equal(acc.cpu().numpy().view(np.uint64), out["f64"].cpu().numpy().view(np.uint64)))
        pass_ms = sum(p["ms"] for p in passes)
        checks = max(1, len(passes) - 1)
        # uniform progressive preview that took the adaptive call's time
        k = max(1, min(n, int(n * wall_ms / one_ms)))
        uni, _ = r.render_samples_device(0, k, acc, want=("f32",), stats=False)
        torch.cuda.synchronize()
        rows.append({"threshold": thr, "min_samples": m, "wall_ms": round(wall_ms, 2), "kernel_ms": round(st["kernel_ms"], 3),
                     "mean_spp": round(mean_spp, 2), "tiles_at_N": int((ts_h == n).sum()), "tiles": int(ts_h.size),
                     "passes": passes, "replay_identical": same,
                     "checkpoint_ms_each": round((st["kernel_ms"] - pass_ms) / checks, 3),
                     "rmse_adaptive": round(rmse(out["f32"].cpu().numpy(), full), 6),
                     "uniform_equal_time_spp": k, "rmse_uniform_equal_time": round(rmse(uni["f32"].cpu().numpy(), full), 6)})
    print(json.dumps({"config": name, "spp": n, "one_shot_ms": round(one_ms, 2), "rows": rows}), flush=True)
    return all(row["replay_identical"] for row in rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--thresholds", default="0.02,0.05,0.1,0.2")
    ap.add_argument("--min-samples", type=int, default=16)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import raytracingmin_amd as rtm
    thresholds = [float(v) for v in args.thresholds.split(",")]
    ok = True
    data = rtm.LoadData(os.path.join(ROOT, "scenes", "cornellBoxSetting.json")).data
    data.width, data.height, data.samples, data.superSamples = 1920, 1080, 64, 4
    ok &= run("headline cornell 1080p x 1024 spp", rtm.Renderer(data, mode="repaired", max_bounces=8, seed=0x5EED),
              thresholds, args.min_samples)
    sd = rtm.LoadData(os.path.join(ROOT, "scenes", "settingData.json")).data
    ok &= run("settingData.json 960x504 x 100 spp", rtm.Renderer(sd, mode="repaired", max_bounces=8, seed=0x5EED),
              thresholds, args.min_samples)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
