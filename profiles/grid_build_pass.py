"""What building a scene object from a DEVICE sphere array costs: rtm_scene_create(..., spheres_on_device = 1, ...) — the
rows come back, one host core builds the grid, the grid goes up — against rtm_scene_create_device — the grid built by the
kernels of csrc/rtm_grid_build_kernel.h, nothing per-sphere crossing — on the same device array.

Stress scenes of 1 000, 100 000 and 1 000 000 spheres.  Per size: one warm-up of each call, then the two calls alternate
--reps times each; a call is timed by the host clock from a synchronised device to its return (both calls return when the
tables are resident) and the scene is destroyed outside the window.  The median, the fastest and every sample are kept.
The two scenes' grids are read back once per size (rtm_debug_scene_grid) and must be equal.  The criterion of the device
build: its median below the host path's at 100 000 spheres, in this run, no margin.  One process; every size runs under its own
time limit (--limit seconds, SIGALRM) and a size that runs into it ends the run with a non-zero status.  The handler is
Python's: it runs between calls, so it bounds a size that is slow, not a library call that never returns (a build blocks in
a stream wait) — run the script under `timeout -k` for that.  Writes profiles/grid_build_pass.json and prints it.

    python profiles/grid_build_pass.py [--reps 7] [--limit 120]
"""
import argparse
import ctypes as C
import json
import os
import signal
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "grid_build_pass.json")
SIZES = (1_000, 100_000, 1_000_000)


class TimeLimit(Exception):
    pass


def _alarm(signum, frame):
    raise TimeLimit()


def grid_of(L, scene):
    info = np.zeros(12, dtype=np.uint64)
    extra = np.zeros(2, dtype=np.uint64)
    if L.rtm_debug_scene_grid(scene, info.ctypes.data, None, 0, None, 0, None, 0, None) != 0:
        return None
    ranges = np.zeros(int(info[0]) * 2, dtype=np.uint32)
    items = np.zeros(max(int(info[1]), 1), dtype=np.uint32)
    big = np.zeros(max(int(info[2]), 1), dtype=np.int32)
    rc = L.rtm_debug_scene_grid(scene, info.ctypes.data, ranges.ctypes.data, ranges.size, items.ctypes.data, items.size,
                                big.ctypes.data, big.size, extra.ctypes.data)
    assert rc == 0, rc
    return info, ranges, items, big, extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=120, help="seconds per scene size")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    import torch
    import raytracingmin_amd as rtm
    from raytracingmin_amd import _lib
    L = rtm.lib()
    signal.signal(signal.SIGALRM, _alarm)
    row = {"config": f"stress scenes on a device array; host-clock ms from a synchronised device to the call's return, "
                     f"{args.reps} alternating calls each after one warm-up",
           "device": torch.cuda.get_device_name(0), "sizes": {}}
    ok = True
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for n in SIZES:
        signal.alarm(args.limit)
        try:
            st = _lib.rtm_settings()
            arr = (_lib.rtm_sphere * n)()
            _lib.check(L.rtm_scene_make_stress(12345, n, C.byref(st), arr), "rtm_scene_make_stress")
            d_arr = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
            ptr = C.c_void_p(d_arr.data_ptr())

            def host_path():
                h = C.c_void_p()
                _lib.check(L.rtm_scene_create(ptr, n, 1, 0, C.byref(h)), "rtm_scene_create")
                return h

            def device_path():
                h = C.c_void_p()
                _lib.check(L.rtm_scene_create_device(ptr, n, 0, stream, C.byref(h)), "rtm_scene_create_device")
                return h

            def timed(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                h = fn()
                t1 = time.perf_counter()
                return h, (t1 - t0) * 1e3

            # warm-up, and the one comparison of the tables
            h_host, h_dev = host_path(), device_path()
            g_host, g_dev = grid_of(L, h_host), grid_of(L, h_dev)
            same = g_host is not None and g_dev is not None and all(np.array_equal(a, b) for a, b in zip(g_host, g_dev))
            ok = ok and same
            L.rtm_scene_destroy(h_host)
            L.rtm_scene_destroy(h_dev)
            ms = {"host": [], "device": []}
            for _ in range(args.reps):
                for key, fn in (("host", host_path), ("device", device_path)):
                    h, t = timed(fn)
                    ms[key].append(t)
                    L.rtm_scene_destroy(h)
            entry = {"tables_equal": bool(same)}
            if g_host is not None:
                entry["grid"] = {"cells": int(g_host[0][0]), "entries": int(g_host[0][1]), "big": int(g_host[0][2]),
                                 "dims": [int(v) for v in g_host[0][3:6]]}
            for key, name in (("host", "scene_create_on_device_array_ms"), ("device", "scene_create_device_ms")):
                entry[name] = {"median": round(statistics.median(ms[key]), 3), "min": round(min(ms[key]), 3),
                               "all": [round(v, 3) for v in ms[key]]}
            entry["host_over_device"] = round(entry["scene_create_on_device_array_ms"]["median"] / entry["scene_create_device_ms"]["median"], 2)
            row["sizes"][str(n)] = entry
        except TimeLimit:
            row["sizes"][str(n)] = {"error": f"ran into the time limit of {args.limit} s"}
            ok = False
            break
        finally:
            signal.alarm(0)
    at = row["sizes"].get("100000", {})
    if "host_over_device" in at:
        row["device_build_faster_at_100000"] = bool(at["scene_create_device_ms"]["median"] < at["scene_create_on_device_array_ms"]["median"])
    text = json.dumps(row, indent=1)
    with open(OUT, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
