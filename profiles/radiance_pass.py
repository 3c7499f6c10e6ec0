"""What a radiance query on a scene costs: rtm_scene_radiance on a camera's primary rays against rtm_render_scene of the same
scene and settings at superSamples = 1, side by side in one process.

Rows: (a) the shipped Cornell scene, 512x512, S = 64, the render through variant 0; (b) the 100 000-sphere stress scene of
BASELINE configs[4], 256x256, S = 16, the render through the grid (variant 17); (c) the first 64 rays of (a) at S = 4096 — one
wave, the under-filled case include/rtm.h warns about; no render beside it.  max_bounces = 8 and the host's sin / cos, as
bench.py renders.  The rays are the reference's primary rays (src/Renderer.cpp:202-232) restated in numpy, sub-pixel (1, 1),
row-major, key_base = 0, with the clamp: the call then defines the render's frame, and the row says whether the two came
out equal bit for bit (if the restated rays differ from the kernel's in a last bit, they do not, and the row says by how much).
Per arm a window is device events around as many back-to-back calls as take at least --window seconds (counted from one
calibrating window), after a warm-up; the arms alternate and every arm gets --reps windows; the median, the fastest, the
slowest and every sample are kept, as ms per call.  No bar is fixed in advance: the yardstick is the render of the same run.
Every scene is measured in a child process of its own (query and render side by side in it; row (c) with row (a)), started
with --scene and ended by the parent after --limit seconds whatever it is waiting for; the parent never opens the device.
Writes profiles/radiance_pass.json and prints it.

    python profiles/radiance_pass.py [--reps 7] [--window 0.4] [--limit 240]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "radiance_pass.json")
N_SPHERES = 100_000
MAX_BOUNCES = 8
SEED = 0x5EED


SCENES = ("a_cornell", "b_stress_100k_grid")


def primary_rays(np, cam, W, H):
    """src/Renderer.cpp:202-208 and :227-232 at superSamples = 1 in the reference's arithmetic: separately rounded doubles, the
    float-length Normalize (src/Ray.h:67-72).  (org, dir): (W*H, 3) float64, ray y * W + x = pixel (x, y)."""
    def normalize(v):
        m = np.float64(np.sqrt(np.float32((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])))
        return v / np.asarray(m)[..., None]

    def cross(a, b):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])

    origin, target, up = (np.array([float(x) for x in v], dtype=np.float64) for v in (cam.origin, cam.target, cam.upVec))
    direction = normalize(target - origin)
    cam_x = -normalize(cross(direction, up))
    cam_y = cross(cam_x, direction)
    fovx = float(np.float32(cam.fov))
    fovy = fovx * H / W
    rate = np.float32(1.0 / 2.0)
    px = 2.0 * (np.arange(W, dtype=np.float64) + np.float64(rate * np.float32(1))) / W - 1.0
    py = 2.0 * (np.arange(H, dtype=np.float64) + np.float64(rate * np.float32(1))) / H - 1.0
    v = ((cam_x * fovx)[None, None, :] * px[None, :, None] + (cam_y * fovy)[None, None, :] * py[:, None, None]) + direction
    d = normalize(v.reshape(-1, 3))
    return np.ascontiguousarray(np.broadcast_to(origin, d.shape)), np.ascontiguousarray(d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.4, help="seconds of calls per timed window, at least")
    ap.add_argument("--limit", type=int, default=240, help="seconds for each scene's process")
    ap.add_argument("--scene", choices=SCENES, help="(the parent's call) measure this scene and print its rows")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if args.scene is None:
        return parent(args)
    import numpy as np
    import torch
    import raytracingmin_amd as rtm
    from raytracingmin_amd import _lib
    L = rtm.lib()
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)
    row = {"device": torch.cuda.get_device_name(0), "rows": {}}

    def window(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(calls):
            fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b) / calls

    def measure(arms):
        calls, ms = {}, {k: [] for k in arms}
        for key, fn in arms.items():  # warm-up and calibration
            fn()
            torch.cuda.synchronize()
            one = window(fn, 2)
            calls[key] = max(2, int(math.ceil(args.window * 1e3 / one)))
        for _ in range(args.reps):
            for key, fn in arms.items():
                ms[key].append(window(fn, calls[key]))
        return {key: {"calls_per_window": calls[key], "median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                      "max_ms": round(max(v), 4), "all_ms": [round(x, 4) for x in v]} for key, v in ms.items()}

    def scene_row(label, data, W, H, S, variant, short=None):
        data.width, data.height, data.samples, data.superSamples = W, H, S, 1
        r = rtm.Renderer(data, mode="repaired", max_bounces=MAX_BOUNCES, seed=SEED, variant=variant)
        o, d = primary_rays(np, data.camera, W, H)
        to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
        n_rays = to.shape[0]
        rad = torch.empty((n_rays, 3), dtype=torch.float64, device="cuda")
        frame = torch.empty((H, W, 3), dtype=torch.float64, device="cuda")
        bufs = _lib.rtm_radiance_buffers()
        bufs.radiance = rad.data_ptr()
        prm = _lib.rtm_radiance_params(r.mode, MAX_BOUNCES, SEED, S, 0, _lib.RADIANCE_CLAMP, 0)
        st, opt, scene = data.settings_c(), r._options(0, H), r._scene_handle()
        po, pd = C.c_void_p(to.data_ptr()), C.c_void_p(td.data_ptr())

        def query():
            _lib.check(L.rtm_scene_radiance(scene, po, pd, n_rays, C.byref(prm), C.byref(bufs), sp), "rtm_scene_radiance")

        def render():
            _lib.check(L.rtm_render_scene(C.byref(st), scene, C.byref(opt), C.c_void_p(frame.data_ptr()), None, None, sp, None),
                       "rtm_render_scene")

        stats = _lib.rtm_stats()
        _lib.check(L.rtm_render_scene(C.byref(st), scene, C.byref(opt), C.c_void_p(frame.data_ptr()), None, None, sp, C.byref(stats)),
                   "rtm_render_scene")
        query()
        torch.cuda.synchronize()
        same = bool(torch.equal(rad.view(torch.int64), frame.reshape(-1, 3).view(torch.int64)))
        entry = {"scene": label, "frame": [W, H], "samples": S, "rays": n_rays, "render_variant": int(stats.variant),
                 "render_variant_name": L.rtm_variant_name(int(stats.variant)).decode(), "casts_per_sample": round(stats.casts / stats.samples, 3),
                 "query_equals_render_bit_for_bit": same}
        if not same:
            entry["pixels_differing"] = int((rad != frame.reshape(-1, 3)).any(dim=1).sum())
            entry["max_abs_difference"] = float((rad - frame.reshape(-1, 3)).abs().max())
        entry.update(measure({"query": query, "render": render}))
        for key in ("query", "render"):
            entry[key]["msamples_per_s"] = round(n_rays * S / entry[key]["median_ms"] / 1e3, 1)
        entry["query_over_render"] = round(entry["query"]["median_ms"] / entry["render"]["median_ms"], 3)
        row["rows"][label] = entry
        if short is not None:  # row (c): the first `short[0]` rays at short[1] samples, no render beside it
            k, big_s = short
            prm_c = _lib.rtm_radiance_params(r.mode, MAX_BOUNCES, SEED, big_s, 0, _lib.RADIANCE_CLAMP, 0)

            def few():
                _lib.check(L.rtm_scene_radiance(scene, po, pd, k, C.byref(prm_c), C.byref(bufs), sp), "rtm_scene_radiance")

            c = {"scene": label, "rays": k, "samples": big_s}
            c.update(measure({"query": few}))
            c["query"]["msamples_per_s"] = round(k * big_s / c["query"]["median_ms"] / 1e3, 3)
            c["filled_rate_over_this"] = round(entry["query"]["msamples_per_s"] / c["query"]["msamples_per_s"], 1)
            row["rows"]["c_under_filled"] = c

    if args.scene == "a_cornell":
        scene_row("a_cornell", rtm.LoadData(os.path.join(ROOT, "scenes", "cornellBoxSetting.json")).data, 512, 512, 64, 0, short=(64, 4096))
    else:
        scene_row("b_stress_100k_grid", rtm.make_stress_scene(n=N_SPHERES, seed=12345), 256, 256, 16, 17)
    print("ROWS " + json.dumps(row))
    return 0


def parent(args):
    """One child per scene, each under its own time limit; the rows merged, written and printed."""
    out = {"config": f"max_bounces {MAX_BOUNCES}, host sin/cos, seed {SEED:#x}, superSamples 1; ms per call from device events around >= "
                     f"{args.window} s of back-to-back calls, {args.reps} alternating windows per arm after a warm-up; one process per scene",
           "rows": {}}
    ok = True
    for scene in SCENES:
        cmd = [sys.executable, os.path.abspath(__file__), "--scene", scene, "--reps", str(args.reps), "--window", str(args.window)]
        try:
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            out["rows"][scene] = {"error": f"ended after the time limit of {args.limit} s"}
            ok = False
            break  # (nothing more is started on a device a process may have hung)
        lines = [x for x in done.stdout.splitlines() if x.startswith("ROWS ")]
        if done.returncode != 0 or not lines:
            out["rows"][scene] = {"error": f"exit status {done.returncode}"}
            ok = False
            break
        got = json.loads(lines[-1][5:])
        out["device"] = got["device"]
        out["rows"].update(got["rows"])
    text = json.dumps(out, indent=1)
    with open(OUT, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
