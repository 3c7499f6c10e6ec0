"""Frames of the tolerance row (variant 18) against variant 0 and the CPU oracle, and the host's hooks that say which kernel a
scene runs: the helpers of tests/test_accept_walls_gpu.py (the same checks as tests/test_bounce_fused_gpu.py makes)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_VARIANT = 18
NORTH_STAR_TOL = 1e-4  # tests/test_tolerance_gpu.py
COUNTERS = ("samples", "casts", "bounces", "draws")
SIG_SIMPLE5 = (1 << 2) | (1 << 4) | (2 << 6) | (2 << 8)  # csrc/rtm_path.h: kAxisSigSimple5
SPLIT_FRAME = dict(w=64, h=16, s=16, ss=2, mb=8, seed=77)  # 16 tiles, 64 samples per pixel


def scene(rtm, name, w, h, s, ss):
    import _oracle
    data = rtm.LoadData(_oracle.scene_path(name)).data
    data.width, data.height, data.samples, data.superSamples = w, h, s, ss
    return data


def cornell(rtm, w, h, s, ss):
    return scene(rtm, "cornellBoxSetting.json", w, h, s, ss)


def render(rtm, data, mb, seed, variant):
    out, st = rtm.Renderer(data, mode="repaired", max_bounces=mb, seed=seed, variant=variant).render_rows_device(want=("f64",))
    return out["f64"].cpu().numpy(), st


def oracle_frame(oracle, data, mb, seed):
    st_c, arr_c, n = data.to_c()
    ost, oarr = oracle.Settings.from_buffer_copy(bytes(st_c)), (oracle.Sphere * max(n, 1)).from_buffer_copy(bytes(arr_c))
    return oracle.render(ost, oarr, n, oracle.make_options(mode=oracle.MODE_REPAIRED, max_bounces=mb, seed=seed, row_begin=0,
                                                           row_end=data.height))


def wall_pairs_granted(rtm, data):
    """rtm_debug_wall_pairs: the host grants the scene's GEOMETRY the pairs signature (shared K, opposite pairs, the envelope)"""
    import ctypes as C
    _, arr, n = data.to_c()
    out = (C.c_uint64 * 2)()
    rtm._lib.check(rtm.lib().rtm_debug_wall_pairs(arr, n, out), "wall pairs")
    return n == 7 and int(out[0]) == 1


def through_the_pairs_kernels(rtm, data):
    """variant 18 takes the pairs instantiation for the Cornell box's seven spheres in repaired mode from a camera inside the box
    (csrc/rtm_kernels_tol.hip: launch_n): the geometry is the shipped box's, the pairs are granted, the camera is within reach"""
    import ctypes as C
    box = cornell(rtm, data.width, data.height, data.samples, data.superSamples)
    spheres = lambda d: [(tuple(o.m_position), o.m_size) for o in d.object]
    _, arr, n = data.to_c()
    rows = (C.c_double * (4 * n))()
    rtm._lib.check(rtm.lib().rtm_debug_axis_rows(arr, n, rows), "axis rows")
    reach = max(rows[3::4])  # of the expanded form: the camera must be within it, and within the compact extent
    cam = float(np.linalg.norm(np.array(tuple(data.camera.origin), dtype=np.float64)))
    return spheres(data) == spheres(box) and wall_pairs_granted(rtm, data) and 0.0 < reach and cam <= reach and cam <= 1e7


def axis_signature_launch(rtm, data, sig):
    """the other signatures with an instantiation: the signature itself and the compact bit (rtm_debug_scene_facts), a reach of the
    expanded form that holds the camera (rtm_debug_axis_rows' fourth column), the camera within the compact extent"""
    import ctypes as C
    _, arr, n = data.to_c()
    facts = (C.c_uint64 * 2)()
    rtm._lib.check(rtm.lib().rtm_debug_scene_facts(arr, n, facts), "scene facts")
    rows = (C.c_double * (4 * n))()
    rtm._lib.check(rtm.lib().rtm_debug_axis_rows(arr, n, rows), "axis rows")
    reach = max(rows[3::4])
    cam = float(np.linalg.norm(np.array(tuple(data.camera.origin), dtype=np.float64)))
    return int(facts[0]) == sig and (int(facts[1]) & 2) != 0 and reach > 0.0 and cam <= reach and cam <= 1e7


def no_signature(rtm, data):
    import ctypes as C
    _, arr, n = data.to_c()
    facts = (C.c_uint64 * 2)()
    rtm._lib.check(rtm.lib().rtm_debug_scene_facts(arr, n, facts), "scene facts")
    return int(facts[0]) == 0


def off_axis_scene(rtm, n=7):
    """n spheres off every axis, sphere 0 around the others and the camera: no signature, the exact-n kernel"""
    from raytracingmin_amd import Camera, Material, SettingData, SphereObject, vec3
    rng = np.random.default_rng(1100 + n)  # (the scene of tests/test_trip_slots_gpu.py)
    objs = [SphereObject(vec3(0.7, 1.5, 0.9), 30.0 + 0.01 * n, Material(vec3(0.55, 0.6, 0.65), vec3(0.5, 0.45, 0.4)))]
    for k in range(1, n):
        c = rng.uniform(-3.5, 3.5, 3)
        c = np.where(np.abs(c) < 0.05, 0.05, c)
        col = 0.25 + 0.7 * rng.random(3)
        objs.append(SphereObject(vec3(*c), float(0.45 + 0.9 * k / n + 0.001 * k), Material(vec3(*col), vec3(0, 0, 0))))
    cam = Camera(vec3(0.3, -0.4, -11.0), vec3(0.1, 0.2, 0.0), vec3(0, 1, 0), 1.2)
    return SettingData(width=16, height=16, samples=4, superSamples=2, camera=cam, object=objs)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def check_frames(what, ref, cnt, img0, st0, img18, st18):
    """variant 0 is the oracle's frame bit for bit; variant 18 within 1e-4 per pixel of both (printed: how many pixels differ at
    all — 0 is the expectation); the counters of all three equal"""
    differing0 = int((bits(img0) != bits(ref)).any(axis=-1).sum())
    differing = int((bits(img18) != bits(img0)).any(axis=-1).sum())
    worst = max(float(np.max(np.abs(img18 - img0))), float(np.max(np.abs(img18 - ref))))
    print(f"{what}: variant 0 — {differing0} pixels differ from the oracle; variant 18 — {differing} from variant 0 of "
          f"{ref.shape[0] * ref.shape[1]}, max |delta| {worst:.3e}; casts {st18['casts']} / {st0['casts']} / oracle {cnt['casts']}")
    assert differing0 == 0, what
    assert worst <= NORTH_STAR_TOL, what
    assert {k: st0[k] for k in COUNTERS} == {k: cnt[k] for k in COUNTERS} == {k: st18[k] for k in COUNTERS}, what


def child(out_path):
    """(a test file run as a script) renders SPLIT_FRAME with variants 0 and 18 under this process's knobs"""
    sys.path.insert(0, ROOT)
    import raytracingmin_amd as m
    f = SPLIT_FRAME
    data = cornell(m, f["w"], f["h"], f["s"], f["ss"])
    res = {}
    for variant in (0, TOL_VARIANT):
        img, st = render(m, data, f["mb"], f["seed"], variant)
        res[f"img{variant}"] = img
        res[f"stats{variant}"] = np.array(json.dumps({k: st[k] for k in COUNTERS + ("variant", "split")}))
    np.savez(out_path, **res)
