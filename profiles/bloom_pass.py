"""What bloom costs (rtm_bloom), beside the display transform of the same frame.

Two Cornell frames (cornellBoxSetting.json, depth cap 8): the headline 1920x1080 one (S=64, SS=4) and a 3840x2160 one (S=4,
SS=2: bloom does not care how converged its input is).  On each frame's f32, in one process: rtm_bloom at the default
parameters (2L = 12 launches), rtm_bloom at L = 1 (the two full-resolution kernels alone) and the default rtm_tonemap call
(three launches), the yardstick.  The C entry points are called with buffers allocated once, so a timing holds the launches
and nothing else; each is timed with device events on the stream, best of --reps after a warm-up, and the output bytes of
every repetition are checked against the first.  The bandwidth is the bytes the kernels must move over the time: the first
kernel reads 12 B per pixel and writes 16 B per level-1 record (4 B per pixel); the combine reads 12 B per pixel and the
level-1 records and writes 12 + 3 B per pixel; a down launch reads level l-1 and writes level l, an up launch reads levels
l + 1 and l and writes level l; the display transform moves 39 B per pixel.  Prints one JSON object.

    python profiles/bloom_pass.py [--reps 10]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE_GBS = 6290.0  # the measured device-to-device copy rate of an MI355X (HBM), the ceiling the GB/s are quoted against


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def level_sizes(w, h, levels):
    sizes = [(w, h)]
    for _ in range(levels):
        w, h = -(-w // 2), -(-h // 2)
        sizes.append((w, h))
    return sizes


def bloom_bytes(w, h, levels):
    """The bytes the 2L launches must move, by kind."""
    rec = [16 * a * b for a, b in level_sizes(w, h, levels)]  # rec[l]: level l's plane (rec[0] unused)
    pix = w * h
    first = 12 * pix + rec[1]
    combine = 12 * pix + rec[1] + 15 * pix
    down = sum(rec[l - 1] + rec[l] for l in range(2, levels + 1))
    up = sum(rec[l + 1] + 2 * rec[l] for l in range(1, levels))
    return {"bright_down": first, "combine": combine, "levels": down + up, "total": first + combine + down + up}


def measure(rtm, f32, reps):
    import torch
    from raytracingmin_amd import _lib
    L = rtm.lib()
    H, W = int(f32.shape[0]), int(f32.shape[1])
    pix = W * H
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out32 = torch.empty_like(f32)
    out8 = torch.empty((H, W, 3), dtype=torch.uint8, device=f32.device)
    stats = torch.empty(4, dtype=torch.int32, device=f32.device)
    defaults = rtm.BLOOM_DEFAULTS
    work = torch.empty(max(L.rtm_bloom_work_bytes(W, H, defaults["levels"]), L.rtm_tonemap_work_bytes(W, H)), dtype=torch.uint8,
                       device=f32.device)

    def bloom_call(levels):
        prm = _lib.rtm_bloom_params(defaults["threshold"], defaults["knee"], defaults["intensity"], defaults["scatter"], levels)
        return lambda: _lib.check(L.rtm_bloom(C.byref(prm), W, H, f32.device.index, f32.data_ptr(), work.data_ptr(), out32.data_ptr(),
                                              out8.data_ptr(), None, stream), "rtm_bloom")

    tm = _lib.rtm_tonemap_params(_lib.TONEMAP_OPS["aces"], _lib.TRANSFERS["srgb"], 1, 1, 0.0, 0.18, 0.0)
    calls = {"bloom_default": (bloom_call(defaults["levels"]), bloom_bytes(W, H, defaults["levels"])["total"]),
             "bloom_one_level": (bloom_call(1), bloom_bytes(W, H, 1)["total"]),
             "tonemap_default": (lambda: _lib.check(L.rtm_tonemap(C.byref(tm), W, H, f32.device.index, f32.data_ptr(), work.data_ptr(),
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
    row["bloom_bytes"] = {k: round(v * 1e-6, 2) for k, v in bloom_bytes(W, H, defaults["levels"]).items()}
    row["bloom_over_tonemap"] = round(row["ms"]["bloom_default"] / row["ms"]["tonemap_default"], 3)
    row["launches"] = {"bloom_default": 2 * defaults["levels"], "bloom_one_level": 2, "tonemap_default": 3}
    return row, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    import raytracingmin_amd as rtm
    rows, ok = [], True
    for width, height, samples, ss in ((1920, 1080, 64, 4), (3840, 2160, 4, 2)):
        data = rtm.LoadData(os.path.join(ROOT, "scenes", "cornellBoxSetting.json")).data
        data.width, data.height, data.samples, data.superSamples = width, height, samples, ss
        r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=0x5EED)
        f32 = r.render_rows_device(want=("f32",), stats=False)[0]["f32"]
        torch.cuda.synchronize()
        row, same = measure(rtm, f32, args.reps)
        row["samples_per_pixel"] = samples * ss * ss
        rows.append(row)
        ok = ok and same
    out = {"config": "cornell, bloom at the default parameters and at one level, the default display transform; device ms, best of "
                     f"{args.reps} after a warm-up (the frame stays in the Infinity Cache between repetitions)",
           "device": torch.cuda.get_device_name(0),
           "copy_rate_gb_per_s": COPY_RATE_GBS,
           "frames": rows,
           "identical": bool(ok)}
    print(json.dumps(out), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
