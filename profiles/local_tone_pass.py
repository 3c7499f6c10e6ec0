"""What the local tone operator costs (rtm_tonemap_local), beside bloom and the display transform of the same frame.

Two Cornell frames (cornellBoxSetting.json, depth cap 8, 16 samples a pixel: the operator does not care how converged its
input is): 1920x1080 and 3840x2160.  On each frame's f32, in one process: rtm_tonemap_local at the default parameters (2L = 10
launches), at levels 0 (the apply kernel alone) and at levels 8 (16 launches), and the two yardsticks, the default rtm_bloom
call (12 launches) and the default rtm_tonemap call (three).  The C entry points are called with buffers allocated once, so a
timing holds the launches and nothing else; each is timed with device events on the stream, best of --reps after a warm-up,
and the output bytes of every repetition are checked against the first.  The bandwidth is the bytes the kernels must move over
the time: the first kernel reads 12 B per pixel and writes two 16 B records per level-1 pixel; a down launch reads both planes
of level l-1 and writes both of level l; a collapse launch reads the I plane of level l+1 and both planes of level l and writes
4 B per record of level l; the apply kernel reads 12 B per pixel and the I plane of level 1 and writes 12 + 3 B per pixel.
Prints one JSON object and writes it to --out.

    python profiles/local_tone_pass.py [--reps 10] [--out profiles/local_tone_pass.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bloom_pass import COPY_RATE_GBS, bloom_bytes, level_sizes, timed  # noqa: E402


def local_bytes(w, h, levels):
    """The bytes the 2L launches (one for L = 0) must move, by kind."""
    rec = [16 * a * b for a, b in level_sizes(w, h, levels)]  # rec[l]: one plane of level l (rec[0] unused)
    pix = w * h
    first = 12 * pix + 2 * rec[1] if levels else 0
    apply = 12 * pix + (rec[1] if levels else 0) + 15 * pix
    down = sum(2 * rec[l - 1] + 2 * rec[l] for l in range(2, levels + 1))
    collapse = sum(rec[l + 1] + 2 * rec[l] + rec[l] // 4 for l in range(1, levels))
    return {"base_down": first, "apply": apply, "levels": down + collapse, "total": first + apply + down + collapse}


def measure(rtm, f32, reps):
    import torch
    from raytracingmin_amd import _lib
    L = rtm.lib()
    H, W = int(f32.shape[0]), int(f32.shape[1])
    pix = W * H
    dev = f32.device.index
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out32 = torch.empty_like(f32)
    out8 = torch.empty((H, W, 3), dtype=torch.uint8, device=f32.device)
    stats = torch.empty(4, dtype=torch.int32, device=f32.device)
    d, b = rtm.TONEMAP_LOCAL_DEFAULTS, rtm.BLOOM_DEFAULTS
    work = torch.empty(max(L.rtm_tonemap_local_work_bytes(W, H, 8), L.rtm_bloom_work_bytes(W, H, b["levels"]),
                           L.rtm_tonemap_work_bytes(W, H)), dtype=torch.uint8, device=f32.device)

    def local_call(levels):
        prm = _lib.rtm_tonemap_local_params(d["anchor"], d["shadows"], d["highlights"], d["sigma"], levels)
        return lambda: _lib.check(L.rtm_tonemap_local(C.byref(prm), W, H, dev, f32.data_ptr(), None, work.data_ptr(), out32.data_ptr(),
                                                      out8.data_ptr(), None, stream), "rtm_tonemap_local")

    bl = _lib.rtm_bloom_params(b["threshold"], b["knee"], b["intensity"], b["scatter"], b["levels"])
    tm = _lib.rtm_tonemap_params(_lib.TONEMAP_OPS["aces"], _lib.TRANSFERS["srgb"], 1, 1, 0.0, 0.18, 0.0)
    calls = {"local_default": (local_call(d["levels"]), local_bytes(W, H, d["levels"])["total"]),
             "local_levels_0": (local_call(0), local_bytes(W, H, 0)["total"]),
             "local_levels_8": (local_call(8), local_bytes(W, H, 8)["total"]),
             "bloom_default": (lambda: _lib.check(L.rtm_bloom(C.byref(bl), W, H, dev, f32.data_ptr(), work.data_ptr(), out32.data_ptr(),
                                                              out8.data_ptr(), None, stream), "rtm_bloom"),
                               bloom_bytes(W, H, b["levels"])["total"]),
             "tonemap_default": (lambda: _lib.check(L.rtm_tonemap(C.byref(tm), W, H, dev, f32.data_ptr(), work.data_ptr(),
                                                                  out32.data_ptr(), out8.data_ptr(), stats.data_ptr(), stream),
                                                    "rtm_tonemap"), 39 * pix)}
    ok = True
    row = {"frame": f"{W}x{H}", "ms": {}, "moved_mb": {}, "gb_per_s": {}, "share_of_copy_rate": {}}
    for name, (call, nbytes) in calls.items():
        timed(call)  # the warm-up
        ref = (out32.cpu().numpy().copy(), out8.cpu().numpy().copy())
        ms = []
        for _ in range(reps):
            ms.append(timed(call))
            ok = ok and np.array_equal(out32.cpu().numpy().view(np.uint32), ref[0].view(np.uint32)) \
                and np.array_equal(out8.cpu().numpy(), ref[1])
        best = min(ms)
        row["ms"][name] = round(best, 4)
        row["moved_mb"][name] = round(nbytes * 1e-6, 1)
        row["gb_per_s"][name] = round(nbytes / (best * 1e-3) * 1e-9, 1)
        row["share_of_copy_rate"][name] = round(nbytes / (best * 1e-3) * 1e-9 / COPY_RATE_GBS, 4)
    row["local_bytes"] = {k: round(v * 1e-6, 2) for k, v in local_bytes(W, H, d["levels"]).items()}
    row["local_over_bloom"] = round(row["ms"]["local_default"] / row["ms"]["bloom_default"], 3)
    row["local_over_tonemap"] = round(row["ms"]["local_default"] / row["ms"]["tonemap_default"], 3)
    row["bytes_local_over_bloom"] = round(local_bytes(W, H, d["levels"])["total"] / bloom_bytes(W, H, b["levels"])["total"], 3)
    row["launches"] = {"local_default": 2 * d["levels"], "local_levels_0": 1, "local_levels_8": 16, "bloom_default": 2 * b["levels"],
                       "tonemap_default": 3}
    return row, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_tone_pass.json"))
    args = ap.parse_args()
    import torch
    import raytracingmin_amd as rtm
    rows, ok = [], True
    for width, height in ((1920, 1080), (3840, 2160)):
        data = rtm.LoadData(os.path.join(ROOT, "scenes", "cornellBoxSetting.json")).data
        data.width, data.height, data.samples, data.superSamples = width, height, 4, 2
        r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=0x5EED)
        f32 = r.render_rows_device(want=("f32",), stats=False)[0]["f32"]
        torch.cuda.synchronize()
        row, same = measure(rtm, f32, args.reps)
        row["samples_per_pixel"] = 16
        rows.append(row)
        ok = ok and same
    out = {"config": "cornell, the local tone operator at the default parameters, at levels 0 and at levels 8, the default bloom and "
                     f"the default display transform; device ms, best of {args.reps} after a warm-up (the frame stays in the "
                     "Infinity Cache between repetitions)",
           "device": torch.cuda.get_device_name(0),
           "copy_rate_gb_per_s": COPY_RATE_GBS,
           "frames": rows,
           "identical": bool(ok)}
    text = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(text, flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
