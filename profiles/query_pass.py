"""What a ray query on a scene costs: rtm_scene_nearest against rtm_scene_occluded on the same device-resident rays.

Scene: the 100 000-sphere stress scene of BASELINE configs[4].  Two ray sets of --rays rays each (default 4 Mi), made on the
device: the primary rays of that config's camera over a denser pixel grid (coherent), and bounce-like rays — from a random
point of a random sphere's surface into the outward hemisphere (incoherent).  Directions are normalised in double.  Three
arms per set: nearest (object and t), occluded with a null tmax (any hit), occluded with tmax = 5 % of the scene's extent.
Per arm a window is device events around as many back-to-back launches as take at least --window seconds (counted from one
calibrating window), after a warm-up; the arms alternate and every arm gets --reps windows; the median, the fastest and
every sample are kept, as ms per launch.  The arms are compared with each other in this run.  The one criterion: on the
bounce-like set the any-hit arm's median is at most the nearest arm's, no margin (the occlusion walk's early exit has to
pay for its instantiation).  From rtm_debug_scene_query on the first --counted rays of each set: sphere tests and cell
steps per ray of the three searches.  For orientation only: rtm_render_aov's time per primary ray on the same scene at
1920x1080.  One process under one time limit (--limit seconds, SIGALRM; Python's handler runs between calls: run the
script under `timeout -k` as well).  Writes profiles/query_pass.json and prints it.

    python profiles/query_pass.py [--rays 4194304] [--reps 7] [--window 0.5] [--limit 500]
"""
import argparse
import ctypes as C
import json
import math
import os
import signal
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "query_pass.json")
N_SPHERES = 100_000


class TimeLimit(Exception):
    pass


def _alarm(signum, frame):
    raise TimeLimit()


def unit(v):
    return v / v.norm(dim=1, keepdim=True)


def primary_rays(torch, cam, n_rays, aspect=(16, 9)):
    """src/Renderer.cpp:202-232 for a pixel grid of about n_rays pixels at the camera's aspect, one ray per pixel centre."""
    f64 = dict(dtype=torch.float64, device="cuda")
    h = int(math.sqrt(n_rays * aspect[1] / aspect[0]))
    w = n_rays // h
    origin, target, up = (torch.tensor([float(x) for x in v], **f64) for v in (cam.origin, cam.target, cam.upVec))
    direction = unit((target - origin)[None])[0]
    cam_x = -unit(torch.linalg.cross(direction, up)[None])[0]
    cam_y = torch.linalg.cross(cam_x, direction)
    fovx = float(cam.fov)
    fovy = fovx * aspect[1] / aspect[0]
    px = 2.0 * (torch.arange(w, **f64) + 0.5) / w - 1.0
    py = 2.0 * (torch.arange(h, **f64) + 0.5) / h - 1.0
    d = (cam_x * fovx)[None, None, :] * px[None, :, None] + (cam_y * fovy)[None, None, :] * py[:, None, None] + direction
    d = unit(d.reshape(-1, 3)).contiguous()
    return origin[None, :].expand(d.shape[0], 3).contiguous(), d, (w, h)


def bounce_rays(torch, centers, radii, n_rays, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    i = torch.randint(0, centers.shape[0], (n_rays,), generator=g, device="cuda")
    nrm = unit(torch.randn((n_rays, 3), generator=g, dtype=torch.float64, device="cuda"))
    v = unit(torch.randn((n_rays, 3), generator=g, dtype=torch.float64, device="cuda"))
    v = torch.where(((v * nrm).sum(dim=1) > 0)[:, None], v, -v)
    return (centers[i] + nrm * radii[i][:, None]).contiguous(), v.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4 * 1024 * 1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of launches per timed window, at least")
    ap.add_argument("--counted", type=int, default=262144, help="rays per set that go through the counting hook")
    ap.add_argument("--limit", type=int, default=500, help="seconds for the whole run")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    import numpy as np
    import torch
    import raytracingmin_amd as rtm
    from raytracingmin_amd import _lib
    L = rtm.lib()
    signal.signal(signal.SIGALRM, _alarm)
    signal.alarm(args.limit)
    data = rtm.make_stress_scene(n=N_SPHERES, seed=12345)
    data.width, data.height, data.samples, data.superSamples = 1920, 1080, 256, 1
    r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=0x5EED)
    arr, n = data.spheres_c()
    host = np.frombuffer(bytes(arr), dtype=np.float64).reshape(n, 10)
    centers = torch.from_numpy(host[:, 0:3].copy()).cuda()
    radii = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.float32).reshape(n, 20)[:, 18].astype(np.float64)).cuda()
    extent = float((centers.max(dim=0).values - centers.min(dim=0).values).max())
    tmax_value = 0.05 * extent
    sets = {}
    o, d, grid = primary_rays(torch, data.camera, args.rays)
    sets["primary"] = (o, d)
    sets["bounce"] = bounce_rays(torch, centers, radii, args.rays, 12345)
    row = {"config": f"stress scene, {N_SPHERES} spheres (BASELINE configs[4]); ms per launch from device events around >= "
                     f"{args.window} s of back-to-back launches, {args.reps} alternating windows per arm after a warm-up",
           "device": torch.cuda.get_device_name(0), "primary_grid": list(grid), "tmax": tmax_value, "scene_extent": extent, "sets": {}}
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)
    scene = r._scene_handle()
    ok = True
    try:
        for name, (o, d) in sets.items():
            n_rays = o.shape[0]
            obj = torch.empty((n_rays,), dtype=torch.int32, device="cuda")
            t = torch.empty((n_rays,), dtype=torch.float64, device="cuda")
            occ = torch.empty((n_rays,), dtype=torch.uint8, device="cuda")
            tmax = torch.full((n_rays,), tmax_value, dtype=torch.float64, device="cuda")
            bufs = _lib.rtm_hit_buffers()
            bufs.object, bufs.t = obj.data_ptr(), t.data_ptr()
            po, pd = C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr())

            def nearest():
                _lib.check(L.rtm_scene_nearest(scene, po, pd, n_rays, C.byref(bufs), sp), "rtm_scene_nearest")

            def any_hit():
                _lib.check(L.rtm_scene_occluded(scene, po, pd, None, n_rays, C.c_void_p(occ.data_ptr()), sp), "rtm_scene_occluded")

            def short():
                _lib.check(L.rtm_scene_occluded(scene, po, pd, C.c_void_p(tmax.data_ptr()), n_rays, C.c_void_p(occ.data_ptr()), sp),
                           "rtm_scene_occluded")

            arms = {"nearest": nearest, "occluded_any": any_hit, "occluded_tmax": short}

            def window(fn, launches):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                for _ in range(launches):
                    fn()
                b.record(stream)
                b.synchronize()
                return a.elapsed_time(b) / launches

            launches, ms = {}, {k: [] for k in arms}
            for key, fn in arms.items():  # warm-up and calibration
                fn()
                torch.cuda.synchronize()
                one = window(fn, 3)
                launches[key] = max(3, int(math.ceil(args.window * 1e3 / one)))
            for _ in range(args.reps):
                for key, fn in arms.items():
                    ms[key].append(window(fn, launches[key]))
            nearest()
            torch.cuda.synchronize()
            entry = {"rays": n_rays, "hit_fraction": round(float((obj >= 0).double().mean()), 4)}
            for key in arms:
                med = statistics.median(ms[key])
                entry[key] = {"launches_per_window": launches[key], "median_ms": round(med, 4), "min_ms": round(min(ms[key]), 4),
                              "all_ms": [round(v, 4) for v in ms[key]], "mrays_per_s": round(n_rays / med / 1e3, 1)}
            k = min(args.counted, n_rays)
            tests = torch.empty((k,), dtype=torch.int32, device="cuda")
            steps = torch.empty((k,), dtype=torch.int32, device="cuda")
            counted = {}
            for key, any_flag, tm in (("nearest", 0, None), ("occluded_any", 1, None), ("occluded_tmax", 1, tmax)):
                _lib.check(L.rtm_debug_scene_query(scene, any_flag, po, pd, C.c_void_p(tm.data_ptr()) if tm is not None else None, k,
                                                   None, None, None, C.c_void_p(tests.data_ptr()), C.c_void_p(steps.data_ptr()), sp),
                           "rtm_debug_scene_query")
                torch.cuda.synchronize()
                counted[key] = {"tests_per_ray": round(float(tests.double().mean()), 2), "steps_per_ray": round(float(steps.double().mean()), 2)}
            entry["counted_rays"] = k
            entry["work"] = counted
            row["sets"][name] = entry
        # orientation: the AOV kernel's primary rays on the same scene
        aov = lambda: r.render_aov(want=("depth", "object"))
        aov()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        aov()
        b.record(stream)
        b.synchronize()
        reps = max(3, int(math.ceil(args.window * 1e3 / a.elapsed_time(b))))
        a.record(stream)
        for _ in range(reps):
            aov()
        b.record(stream)
        b.synchronize()
        per = a.elapsed_time(b) / reps
        row["render_aov_1920x1080"] = {"ms": round(per, 4), "mrays_per_s": round(1920 * 1080 / per / 1e3, 1), "launches": reps}
        bn = row["sets"]["bounce"]
        row["any_hit_at_most_nearest_on_bounce"] = bool(bn["occluded_any"]["median_ms"] <= bn["nearest"]["median_ms"])
        ok = row["any_hit_at_most_nearest_on_bounce"]
    except TimeLimit:
        row["error"] = f"ran into the time limit of {args.limit} s"
        ok = False
    finally:
        signal.alarm(0)
    text = json.dumps(row, indent=1)
    with open(OUT, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
