"""What the depth of field costs (rtm_defocus), beside the display transform of the same frame.

Two Cornell frames (cornellBoxSetting.json, depth cap 8, S=4, SS=1: the stage does not care how converged its input is) at
1920x1080 and 3840x2160, each with its depth plane (rtm_render_aov) and the focus at the camera's target distance.  On each
frame's f32, in one process: rtm_defocus at aperture 0 (every tile passes its inputs through), at the default parameters
(aperture 4, max_radius 8) and at aperture 16, max_radius 16 (the largest window, 33 x 33 taps) — each as shipped (form 0: the
window bounded per tile, sharp tiles passed through) and with every block running all (2R+1)^2 taps (form 1 of
rtm_debug_defocus_form) — and the default rtm_tonemap call (three launches), the yardstick.  The C entry points are called
with buffers allocated once, so a timing holds the launch and nothing else; each is timed with device events on the stream,
best of --reps after a warm-up, and the output bytes of every repetition and of both forms are checked against the first.
The taps are the window's, (2R+1)^2 per pixel: what form 1 runs.  Nothing is asserted about the times: there is no earlier
implementation to beat.  Writes one JSON object to --out and prints it.

    python profiles/defocus_pass.py [--reps 10] [--out profiles/defocus_pass.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("aperture_0", 0.0, 8), ("default", 4.0, 8), ("aperture_16_radius_16", 16.0, 16))


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(rtm, f32, depth, zf, reps):
    import torch
    from raytracingmin_amd import _lib
    L = rtm.lib()
    H, W = int(f32.shape[0]), int(f32.shape[1])
    dev = f32.device
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out32 = torch.empty_like(f32)
    out8 = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    stats = torch.empty(4, dtype=torch.int32, device=dev)
    work = torch.empty(max(256, L.rtm_tonemap_work_bytes(W, H)), dtype=torch.uint8, device=dev)

    def defocus_call(form, aperture, radius):
        prm = _lib.rtm_defocus_params(zf, aperture, radius)
        return lambda: _lib.check(L.rtm_debug_defocus_form(form, C.byref(prm), W, H, dev.index, f32.data_ptr(), depth.data_ptr(),
                                                           out32.data_ptr(), out8.data_ptr(), None, stream), "rtm_debug_defocus_form")

    tm = _lib.rtm_tonemap_params(_lib.TONEMAP_OPS["aces"], _lib.TRANSFERS["srgb"], 1, 1, 0.0, 0.18, 0.0)
    calls = {}
    for name, aperture, radius in CASES:
        calls[name] = defocus_call(0, aperture, radius)
        calls[name + "_unbounded"] = defocus_call(1, aperture, radius)
    calls["tonemap_default"] = lambda: _lib.check(L.rtm_tonemap(C.byref(tm), W, H, dev.index, f32.data_ptr(), work.data_ptr(),
                                                                out32.data_ptr(), out8.data_ptr(), stats.data_ptr(), stream),
                                                  "rtm_tonemap")
    ok = True
    row = {"frame": f"{W}x{H}", "ms": {}, "window_taps_per_pixel": {}, "changed_pixels": {}}
    first = {}
    for name, call in calls.items():
        timed(call)  # the warm-up
        ref = (out32.cpu().numpy().copy(), out8.cpu().numpy().copy())
        ms = []
        for _ in range(reps):
            ms.append(timed(call))
            ok = ok and np.array_equal(out32.cpu().numpy().view(np.uint32), ref[0].view(np.uint32)) \
                and np.array_equal(out8.cpu().numpy(), ref[1])
        row["ms"][name] = round(min(ms), 4)
        base = name[:-len("_unbounded")] if name.endswith("_unbounded") else name
        if base in first:  # the two forms: the same bits
            ok = ok and np.array_equal(first[base][0].view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(first[base][1], ref[1])
        else:
            first[base] = ref
        if name != "tonemap_default" and base == name:
            radius = dict((n, r) for n, _, r in CASES)[name]
            row["window_taps_per_pixel"][name] = (2 * radius + 1) ** 2
            row["changed_pixels"][name] = int(np.any(ref[0].view(np.uint32) != f32.cpu().numpy().view(np.uint32), axis=-1).sum())
    row["bounded_over_unbounded"] = {n: round(row["ms"][n] / row["ms"][n + "_unbounded"], 3) for n, _, _ in CASES}
    row["default_over_tonemap"] = round(row["ms"]["default"] / row["ms"]["tonemap_default"], 3)
    return row, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "defocus_pass.json"))
    args = ap.parse_args()
    import torch
    import raytracingmin_amd as rtm
    rows, ok = [], True
    for width, height in ((1920, 1080), (3840, 2160)):
        data = rtm.LoadData(os.path.join(ROOT, "scenes", "cornellBoxSetting.json")).data
        data.width, data.height, data.samples, data.superSamples = width, height, 4, 1
        r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=0x5EED)
        f32 = r.render_rows_device(want=("f32",), stats=False)[0]["f32"]
        depth = r.render_aov(want=("depth",))["depth"]
        torch.cuda.synchronize()
        row, same = measure(rtm, f32, depth, r.focus_distance(), args.reps)
        row["focus_distance"] = r.focus_distance()
        rows.append(row)
        ok = ok and same
    out = {"config": "cornell at 4 spp with its depth plane, focus at the target distance; rtm_defocus at aperture 0, at the defaults "
                     "(aperture 4, max_radius 8) and at aperture 16, max_radius 16, as shipped and with the whole window in every "
                     f"block (_unbounded), and the default display transform; device ms, best of {args.reps} after a warm-up",
           "device": torch.cuda.get_device_name(0),
           "frames": rows,
           "identical": bool(ok)}
    text = json.dumps(out, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
