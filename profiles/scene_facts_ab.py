#!/usr/bin/env python3
"""A/B of two builds of librtm_hip.so over the five HOST-ONLY test hooks (no device is touched): rtm_debug_scene_facts,
rtm_debug_zero_term_facts, rtm_debug_axis_rows, rtm_debug_wall_pairs and rtm_debug_grid_build.

    python profiles/scene_facts_ab.py <library A> <library B> [--time]

Each library runs in a child process of its own over the same seeded inputs — the shipped scenes, 2 000 small scenes of 1 to 40
spheres drawn to reach every branch of the proofs, and the grid builder on stress scenes of 64, 65, 1 000 and 100 000 spheres —
and writes every return code and output as bytes.  The script fails unless the two records are byte-equal, and prints how
often each fact came out set BY LIBRARY A'S ANSWERS: each must be set in at least 5 % and clear in at least 5 % of the small
scenes, or the comparison says nothing about that branch.  --time: also times rtm_debug_grid_build on the 100 000-sphere scene,
A and B alternating, 7 child runs each (a run: one warm-up call, then the median of 5), and fails when B's median lies above
A's median plus three of A's standard deviations.
"""
import ctypes as C
import glob
import json
import math
import os
import random
import statistics
import struct
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SMALL = 2000
GRID_SIZES = (64, 65, 1000, 100000)
STRESS_SEED = 0x5EED
# csrc/rtm_scene_flags.h
K_FOLD_NO_LEVEL_EMISSION, K_SCENE_COMPACT = 1, 2


class Sphere(C.Structure):  # include/rtm.h: rtm_sphere
    _fields_ = [("center", C.c_double * 3), ("color", C.c_double * 3), ("emission", C.c_double * 3),
                ("radius", C.c_float), ("_pad", C.c_float)]


class Settings(C.Structure):  # include/rtm.h: rtm_settings (camera: 3 x 3 doubles, fov, pad)
    _fields_ = [("dims", C.c_int32 * 4), ("camera", C.c_double * 9), ("fov", C.c_float * 2)]


def sphere_array(rows):
    arr = (Sphere * max(len(rows), 1))()
    for s, (c, col, e, r) in zip(arr, rows):
        s.center[:] = c
        s.color[:] = col
        s.emission[:] = e
        s.radius = r
    return arr


def load_scene(lib, path):
    st, n = Settings(), C.c_size_t(0)
    arr = (Sphere * 64)()
    rc = lib.rtm_scene_load_json(path.encode(), 0, C.byref(st), arr, 64, C.byref(n))
    if rc != 0:
        return rc, []
    return rc, [(list(s.center), list(s.color), list(s.emission), s.radius) for s in arr[:n.value]]


def small_scenes(cornell):
    """The 2 000 seeded scenes.  Mixed in: centres on an axis, +c / -c partners with one r*r, another axis with the same K,
    signed zeros, very large centres, about 1 % non-finite values, emitting and dark, black and coloured spheres; four in ten
    are the Cornell box varied (its walls are the only shipped spheres large enough for the wall-pair proof)."""
    rng = random.Random(20261019)
    scenes = []
    for _ in range(N_SMALL):
        n = rng.randint(1, 40)
        rows = []
        if rng.random() < 0.4:
            rows = [(list(c), list(col), list(e), r) for c, col, e, r in cornell]
            for _ in range(rng.choice((0, 0, 0, 0, 1, 2))):
                i, what = rng.randrange(len(rows)), rng.randrange(6)
                c, col, e, r = rows[i]
                k = max(range(3), key=lambda a: abs(c[a]))
                if what == 0:
                    c[k] = math.nextafter(c[k], math.inf)  # one ulp: no partner, another K
                elif what == 1:
                    rows[i] = (c, col, e, r * 1.5)
                elif what == 2:
                    c[k] = -c[k]
                elif what == 3 and i + 1 < len(rows):
                    rows[i], rows[i + 1] = rows[i + 1], rows[i]
                elif what == 4:
                    c[k] *= 100.0
                else:
                    c[(k + 1) % 3] = 0.5
            while len(rows) < n:
                rows.append(([rng.uniform(-50, 50) for _ in range(3)], [rng.random() for _ in range(3)], [0.0] * 3,
                             rng.uniform(0.1, 20.0)))
            if rng.random() < 0.15:
                rng.shuffle(rows)
        axis = []  # (axis, c, r) of the axis spheres so far
        while len(rows) < n:
            t = rng.random()
            if t < 0.30 or (t < 0.55 and not axis):
                a = rng.randrange(3)
                c = rng.choice((rng.uniform(1, 50), 10010.0, rng.uniform(1e3, 1e5))) * rng.choice((-1, 1))
                r = rng.choice((1.0, 0.5, 1e4, rng.uniform(0.1, 20.0)))
            elif t < 0.45:
                a, c, r = axis[-1]
                c, r = -c, (r if rng.random() < 0.9 else r * 0.5)
            elif t < 0.55:
                a, c, r = rng.choice(axis)
                a, c = (a + rng.randrange(1, 3)) % 3, c * rng.choice((-1, 1))
            else:
                a = -1
            if a >= 0:
                centre = [rng.choice((0.0, -0.0)) for _ in range(3)]
                centre[a] = c
                axis.append((a, c, r))
            else:
                centre, r = [rng.uniform(-50, 50) for _ in range(3)], rng.uniform(0.1, 20.0)
            emits = rng.random() < 0.15
            black = rng.random() < (0.8 if emits else 0.1)
            col = [0.0] * 3 if black else [rng.random() for _ in range(3)]
            e = [5.0, 5.0, 5.0] if emits else [rng.choice((0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -0.0))
                                               for _ in range(3)]
            rows.append((centre, col, e, r))
        if rng.random() < 0.10:
            c = rows[rng.randrange(n)][0]
            for k in range(3):
                c[k] *= rng.choice((1e8, 1e300))
        rows = rows[:n]
        for c, col, e, r in rows:  # about 1 % non-finite values
            for vec in (c, col, e):
                for k in range(3):
                    if rng.random() < 0.01:
                        vec[k] = rng.choice((math.nan, math.inf, -math.inf))
        rows = [(c, col, e, (rng.choice((math.nan, math.inf)) if rng.random() < 0.01 else r)) for c, col, e, r in rows]
        scenes.append(rows)
    return scenes


def hooks(lib, rows, record, label):
    """The four small hooks on one scene: every return code and output goes into `record`; returns the facts."""
    n, arr = len(rows), sphere_array(rows)
    facts, zt, wp = (C.c_uint64 * 2)(), (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
    ar = (C.c_double * (4 * max(n, 1)))()
    rcs = [lib.rtm_debug_scene_facts(arr, n, facts), lib.rtm_debug_zero_term_facts(arr, n, zt),
           lib.rtm_debug_axis_rows(arr, n, ar), lib.rtm_debug_wall_pairs(arr, n, wp)]  # (the last two refuse n > 32)
    record.append((label, struct.pack("<4i", *rcs) + bytes(facts) + bytes(zt) + bytes(ar) + bytes(wp)))
    reach = max((ar[4 * i + 3] for i in range(n)), default=0.0) if n <= 32 and rcs[2] == 0 else 0.0
    ks = {}
    if n <= 32 and rcs[2] == 0:  # the shared-K group has no hook of its own: two axis rows among the first 8 with one K
        for i in range(min(n, 8)):
            if (facts[0] >> (2 * i)) & 3:
                kb = struct.pack("<d", ar[4 * i + 2])
                ks[kb] = ks.get(kb, 0) + 1
    return {"wall_pairs": wp[0] == 1, "reach": reach > 0.0, "shared_k": any(v >= 2 for v in ks.values()),
            "compact": bool(facts[1] & K_SCENE_COMPACT), "no_level_emission": bool(facts[1] & K_FOLD_NO_LEVEL_EMISSION),
            "zero_term": zt[0] == 1}


def stress(lib, n):
    st, arr = Settings(), (Sphere * n)()
    assert lib.rtm_scene_make_stress(STRESS_SEED, n, C.byref(st), arr) == 0
    return arr


def grid_build(lib, arr, n, record=None, label=""):
    info, pads = (C.c_uint64 * 12)(), (C.c_double * n)()
    rc = lib.rtm_debug_grid_build(arr, n, info, pads, None, 0, None, 0, None, 0)
    out = struct.pack("<i", rc) + bytes(info)
    if rc == 0:
        cells, refs, big = info[0], info[1], info[2]
        ranges, items, bigs = (C.c_uint32 * (2 * cells))(), (C.c_uint32 * max(refs, 1))(), (C.c_int32 * max(big, 1))()
        rc = lib.rtm_debug_grid_build(arr, n, info, pads, ranges, 2 * cells, items, refs, bigs, big)
        out += struct.pack("<i", rc) + bytes(info) + bytes(pads) + bytes(ranges) + bytes(items) + bytes(bigs)
    if record is not None:
        record.append((label, out))
    return rc


def open_lib(path):
    lib = C.CDLL(path)
    for name in ("rtm_debug_scene_facts", "rtm_debug_zero_term_facts", "rtm_debug_axis_rows", "rtm_debug_wall_pairs"):
        getattr(lib, name).argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    lib.rtm_debug_grid_build.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                         C.c_size_t, C.c_void_p, C.c_size_t]
    lib.rtm_scene_make_stress.argtypes = [C.c_uint64, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.rtm_scene_load_json.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    return lib


def child(lib_path, out_path):
    lib = open_lib(lib_path)
    record, cornell = [], []
    for path in sorted(glob.glob(os.path.join(ROOT, "scenes", "*.json"))):
        name = os.path.basename(path)
        rc, rows = load_scene(lib, path)
        record.append(("load " + name, struct.pack("<i", rc)))
        if rc == 0:
            hooks(lib, rows, record, "shipped " + name)
        if name == "cornellBoxSetting.json":
            cornell = rows
    assert cornell, "scenes/cornellBoxSetting.json did not load"
    counts = {}
    for i, rows in enumerate(small_scenes(cornell)):
        for k, v in hooks(lib, rows, record, "small %d (n = %d)" % (i, len(rows))).items():
            counts[k] = counts.get(k, 0) + int(v)
    for n in GRID_SIZES:
        grid_build(lib, stress(lib, n), n, record, "grid build, %d stress spheres" % n)
    with open(out_path, "wb") as f:
        for label, data in record:
            f.write(struct.pack("<II", len(label.encode()), len(data)) + label.encode() + data)
    with open(out_path + ".json", "w") as f:
        json.dump(counts, f)


def child_time(lib_path, out_path):
    lib = open_lib(lib_path)
    n = GRID_SIZES[-1]
    arr = stress(lib, n)
    info, pads = (C.c_uint64 * 12)(), (C.c_double * n)()
    times = []
    for _ in range(6):
        t0 = time.perf_counter()
        assert lib.rtm_debug_grid_build(arr, n, info, pads, None, 0, None, 0, None, 0) == 0
        times.append(time.perf_counter() - t0)
    with open(out_path, "w") as f:
        json.dump(statistics.median(times[1:]) * 1e3, f)


def read_record(path):
    out, data = [], open(path, "rb").read()
    pos = 0
    while pos < len(data):
        ln, dn = struct.unpack_from("<II", data, pos)
        pos += 8
        out.append((data[pos:pos + ln].decode(), data[pos + ln:pos + ln + dn]))
        pos += ln + dn
    return out


def run_child(mode, lib, out):
    subprocess.check_call([sys.executable, os.path.abspath(__file__), mode, os.path.abspath(lib), out])


def main(argv):
    if len(argv) >= 4 and argv[1] in ("--child", "--child-time"):
        (child if argv[1] == "--child" else child_time)(argv[2], argv[3])
        return 0
    libs = [a for a in argv[1:] if not a.startswith("--")]
    if len(libs) != 2:
        print(__doc__)
        return 2
    failed = False
    with tempfile.TemporaryDirectory() as tmp:
        outs = [os.path.join(tmp, "a.bin"), os.path.join(tmp, "b.bin")]
        for lib, out in zip(libs, outs):
            run_child("--child", lib, out)
        a, b = read_record(outs[0]), read_record(outs[1])
        diff = [la for (la, da), (lb, db) in zip(a, b) if la != lb or da != db]
        if len(a) != len(b) or diff:
            failed = True
            print("DIFFERENT: %d of %d records, the first: %s" % (len(diff), len(a), diff[0] if diff else "(record count)"))
        else:
            print("byte-equal: %d records, %d bytes" % (len(a), sum(len(d) for _, d in a)))
        counts = json.load(open(outs[0] + ".json"))
        print("facts set among the %d small scenes, by library A's answers:" % N_SMALL)
        for k, v in counts.items():
            ok = 0.05 * N_SMALL <= v <= 0.95 * N_SMALL
            failed = failed or not ok
            print("  %-18s %5d  (%4.1f %%)%s" % (k, v, 100.0 * v / N_SMALL, "" if ok else "  <-- outside 5 % .. 95 %"))
        if "--time" in argv:
            ms = ([], [])
            for _ in range(7):
                for k in (0, 1):
                    out = os.path.join(tmp, "t.json")
                    run_child("--child-time", libs[k], out)
                    ms[k].append(json.load(open(out)))
            med_a, med_b, sd_a = statistics.median(ms[0]), statistics.median(ms[1]), statistics.stdev(ms[0])
            print("rtm_debug_grid_build, %d stress spheres, ms per call, 7 alternating runs each:" % GRID_SIZES[-1])
            print("  A: " + " ".join("%.2f" % v for v in ms[0]) + "   median %.2f, standard deviation %.2f" % (med_a, sd_a))
            print("  B: " + " ".join("%.2f" % v for v in ms[1]) + "   median %.2f" % med_b)
            ok = med_b <= med_a + 3.0 * sd_a
            failed = failed or not ok
            print("  B's median %s A's median + 3 standard deviations (%.2f)" % ("within" if ok else "ABOVE", med_a + 3.0 * sd_a))
    print("FAILED" if failed else "ok")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
