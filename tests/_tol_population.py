"""The frames tests/test_tolerance_scenes_gpu.py renders through the tolerance row (variant 18) and tests/test_tolerance_scenes_host.py
checks on the CPU: the edge scenes of tests/_edge_scenes.py with their depth settings (`edge_frames`) and a seeded population of 384
small frames (`population`), built after the families of profiles/fuzz_parity.py and shaped so that every kernel the row dispatches
to (csrc/rtm_kernels_tol.hip: launch_n) gets frames, capped and at any depth — `cell` names the kernel class of a frame from the
host-only hooks, CELL_MINIMA is what the host test asks of the population.

What is left out ON PURPOSE: small spheres inside a closed box beyond a cap of 8, and off-axis rooms of more than seven spheres beyond
it.  A bounce off a sphere of radius 0.3 to 1 multiplies a last-bit difference by the ratio of the free path to the radius; after a
dozen such bounces a path of the row leaves the reference's (profiles/r4/fuzz_parity.txt case 7376).  That regime is
documented, not claimed; its one recorded frame is tests/golden/tolerance_case_7376.json.

What the open stress scenes are worth: up to 24 spheres of radius under 1 in a cube of side 100, one of them the emitter — most of
their frames are black and many have no bounce at all.  They are the only family the row serves at any depth with n >= 8, so they
stay (the chunked any-depth kernel's misses, rare hits and counters), three slots of sixteen; the closed families carry the light."""
import ctypes as C

import numpy as np

import _tol_frames as F
from _edge_scenes import AXIS_ROOMS, EDGE_SCENES, _mk

POPULATION_SEED = 16_384
CASES, CHUNKS = 384, 8
SIG_CORNELL7 = 2 | (1 << 2) | (1 << 4) | (2 << 6) | (2 << 8) | (3 << 10) | (3 << 12)  # csrc/rtm_path.h: kAxisSigCornell7
SIG_SIMPLE5 = F.SIG_SIMPLE5
SIG_SETTING3 = 2 | (1 << 4)                                                            # kAxisSigSetting3
STRESS_N = [1, 2, 4, 5, 6, 7, 8, 9, 15, 16, 17, 23, 24]
BIG_N = [8, 9, 15, 16, 17, 23, 24]
CAPS = [0, 1, 2, 3, 5, 7, 8, 8]     # the depth-capped kernels (a cap of at most 8)
DEEP_ROOM = [-1, -1, 9, 12, 17]     # the any-depth kernels: rooms of few large spheres
DEEP_OPEN = [-1, -1, 9, 16, 40, 200]
DEEP_OFF_AXIS = [-1, 12]

# the families, one per slot; a round of 16 cases holds one of each slot, so every chunk of 48 mixes all of them
SLOTS = ["pairs room", "axis room", "axis room", "one-K room", "simple5", "setting3", "box with small spheres", "stress", "stress",
         "stress", "off axis", "off axis", "first k of the box", "axis room", "box with small spheres", "off axis"]
assert CASES % len(SLOTS) == 0 and CASES % CHUNKS == 0

# cell -> the least number of cases; "capped": 0 <= max_bounces <= 8, "any": every other depth
CELL_MINIMA = {(c, d): 8 for c in "abcfgh" for d in ("capped", "any")}
CELL_MINIMA[("d", "capped")] = CELL_MINIMA[("e", "capped")] = 8


def _facts(rtm, data):
    _, arr, n = data.to_c()
    facts = (C.c_uint64 * 2)()
    rtm._lib.check(rtm.lib().rtm_debug_scene_facts(arr, n, facts), "scene facts")
    return int(facts[0]), int(facts[1])


def walls_share_one_k(rtm, data):
    """the six walls of a seven-sphere room hold one K bit for bit and the light another (rtm_debug_axis_rows' third column): with
    the launch conditions, the kernel of kAxisSigCornell7Walls, or of kAxisSigCornell7Pairs where the pairs are granted"""
    _, arr, n = data.to_c()
    if n != 7:
        return False
    rows = (C.c_double * (4 * n))()
    rtm._lib.check(rtm.lib().rtm_debug_axis_rows(arr, n, rows), "axis rows")
    k = np.array(rows[2::4], dtype=np.float64).view(np.uint64)
    return bool((k[1:] == k[1]).all() and k[0] != k[1])


def any_depth(mb):
    return mb < 0 or mb > 8


def cell(rtm, data, mb):
    """(class, depth) of a repaired-mode frame, after launch_n: a / b / c the Cornell signature with pairs, without, and refused by
    the launch conditions (the plain exact-7 kernel); d / e the Simple5 and Setting3 signatures with their launch conditions; f no
    signature at n = 3, 5, 7; g n in 1, 2, 4, 6; h n >= 8 (the chunked kernel); "-" anything else (a signature without an
    instantiation: the exact-n or the generic kernel)"""
    n = len(data.object)
    sig, _ = _facts(rtm, data)
    depth = "any" if any_depth(mb) else "capped"
    if n == 7 and sig == SIG_CORNELL7:
        if not F.axis_signature_launch(rtm, data, SIG_CORNELL7):
            return "c", depth
        pairs = F.wall_pairs_granted(rtm, data)
        assert not pairs or walls_share_one_k(rtm, data)
        return ("a" if pairs else "b"), depth
    if n == 5 and F.axis_signature_launch(rtm, data, SIG_SIMPLE5):
        return "d", depth
    if n == 3 and F.axis_signature_launch(rtm, data, SIG_SETTING3):
        return "e", depth
    if n in (3, 5, 7) and F.no_signature(rtm, data):
        return "f", depth
    if n in (1, 2, 4, 6):
        return "g", depth
    if n >= 8:
        return "h", depth
    return "-", depth


def eligible(data):
    """what csrc/rtm_kernels_tol.hip: launch_tol serves"""
    return (not data.has_planes()) and 1 <= len(data.object) <= 24 and data.samples * data.superSamples ** 2 < 65536


# ---- part one: the edge scenes ---------------------------------------------------------------------------------------------------------
EDGE_DEPTHS = (("repaired", 8), ("repaired", 3), ("repaired", 1), ("repaired", 0), ("literal", -1), ("literal", 2))
ROOM_DEPTHS = (("repaired", 8), ("repaired", -1), ("repaired", 3), ("repaired", 12), ("literal", -1))


def edge_scene(rtm, name):
    """45x27, S 3, SS 2 (tests/test_parity_gpu.py: test_edge_case_scenes_vs_oracle)"""
    objs, origin, fov = EDGE_SCENES[name](rtm)
    cam = rtm.Camera(rtm.vec3(*origin), rtm.vec3(0, 0, 0), rtm.vec3(0, 1, 0), fov)
    return rtm.SettingData(width=45, height=27, samples=3, superSamples=2, camera=cam, object=objs)


def axis_room(rtm, name):
    """56x40, S 4, SS 2 (test_axis_signature_scenes_vs_oracle)"""
    objs, origin = AXIS_ROOMS[name](rtm)
    cam = rtm.Camera(rtm.vec3(*origin), rtm.vec3(0, 0, 0), rtm.vec3(0, 1, 0), 1.6)
    return rtm.SettingData(width=56, height=40, samples=4, superSamples=2, camera=cam, object=objs)


def near_misses(rtm):
    """the denormal coordinate, the rotated order, the six-sphere box: 40x24, S 4, SS 2 (test_axis_signature_near_misses_take_the_
    general_kernel)"""
    base = F.cornell(rtm, 40, 24, 4, 2)
    objs = list(base.object)
    tiny = _mk(rtm, (5e-324, 10, 0), 5, (0, 0, 0), (5, 5, 5))
    return {name: rtm.SettingData(width=40, height=24, samples=4, superSamples=2, camera=base.camera, object=o)
            for name, o in (("denormal coordinate", [tiny] + objs[1:]), ("rotated order", objs[1:] + objs[:1]), ("six-sphere box", objs[:6]))}


def degenerate_camera(rtm):
    """upVec parallel to the view direction: every primary ray is NaN and misses (test_degenerate_camera_gives_the_same_nans)"""
    base = F.cornell(rtm, 24, 16, 2, 1)
    cam = rtm.Camera(rtm.vec3(0, 0, -10), rtm.vec3(0, 0, 0), rtm.vec3(0, 0, 1), 2.0)
    return rtm.SettingData(width=24, height=16, samples=2, superSamples=1, camera=cam, object=base.object)


def coincident_spheres(rtm):
    """eleven coincident walls of different colours and the light among them, 12 spheres (test_coincident_spheres_lowest_index_wins)"""
    base = F.cornell(rtm, 40, 24, 4, 2)
    objs = [rtm.SphereObject(rtm.vec3(0, 0, 0), 50.0, rtm.Material(rtm.vec3(0.1 + 0.07 * k, 0.5, 0.9 - 0.07 * k), rtm.vec3(0, 0, 0)))
            for k in range(11)]
    objs.insert(5, base.object[0])
    return rtm.SettingData(width=40, height=24, samples=4, superSamples=2, camera=base.camera, object=objs)


def one_pixel(rtm):
    """1x1, one sample (test_one_pixel_one_sample)"""
    return F.scene(rtm, "simpleSetting1.json", 1, 1, 1, 1)


def edge_frames(rtm):
    """{group: [(label, data, mode, max_bounces, seed, expect)]}; expect: "frame", or "zeros" where the frame must be black"""
    groups = {}
    for name in sorted(EDGE_SCENES):
        data = edge_scene(rtm, name)
        groups[name] = [(f"{name} {mode} {mb}", data, mode, mb, 17, "frame") for mode, mb in EDGE_DEPTHS]
    for name in sorted(AXIS_ROOMS):
        data = axis_room(rtm, name)
        groups[name] = [(f"{name} {mode} {mb}", data, mode, mb, 23, "frame") for mode, mb in ROOM_DEPTHS]
    groups["near misses"] = [(f"{name} repaired {mb}", data, "repaired", mb, 3, "frame")
                             for name, data in near_misses(rtm).items() for mb in (8, -1)]
    groups["degenerate camera"] = [(f"degenerate camera {mode} 8", degenerate_camera(rtm), mode, 8, 1, "zeros")
                                   for mode in ("repaired", "literal")]
    groups["coincident spheres"] = [("coincident spheres repaired 6", coincident_spheres(rtm), "repaired", 6, 3, "frame")]
    groups["one pixel"] = [("one pixel repaired -1", one_pixel(rtm), "repaired", -1, 5, "frame")]
    return groups


EDGE_GROUPS = sorted(EDGE_SCENES) + sorted(AXIS_ROOMS) + ["near misses", "degenerate camera", "coincident spheres", "one pixel"]


# ---- part two: the seeded population ---------------------------------------------------------------------------------------------------
def _f(v):
    return [float(x) for x in np.atleast_1d(v)]


def _sphere(rtm, pos, r, col, em=(0, 0, 0)):
    return rtm.SphereObject(rtm.vec3(*_f(pos)), float(r), rtm.Material(rtm.vec3(*_f(col)), rtm.vec3(*_f(em))))


def _room_camera(rtm, rng, half):
    return rtm.Camera(rtm.vec3(*_f(rng.uniform(-0.7, 0.7, 3) * half)), rtm.vec3(*_f(rng.uniform(-0.2, 0.2, 3) * half)), rtm.vec3(0, 1, 0),
                      float(rng.uniform(0.8, 2.0)))


def _scene(rtm, cam, objs):
    return rtm.SettingData(width=8, height=8, samples=1, superSamples=1, camera=cam, object=objs)


def _axis_room(rtm, rng):
    """the fuzz script's seven-sphere room: the Cornell box's signature, every number random"""
    half = float(rng.uniform(3, 12))
    objs = [_sphere(rtm, (0, float(rng.uniform(0.3, 1.0)) * half, 0), float(rng.uniform(0.1, 0.5)) * half, (0, 0, 0), (5, 5, 5))]
    for k in range(6):
        r = float(10 ** rng.uniform(1, 4.5))
        pos = [0.0, 0.0, 0.0]
        pos[k // 2] = (r + half * float(rng.uniform(0.8, 1.2))) * (1 if k % 2 == 0 else -1)
        objs.append(_sphere(rtm, pos, r, rng.uniform(0.2, 0.9, 3)))
    return _scene(rtm, _room_camera(rtm, rng, half), objs)


def _integer_room(rtm, rng, radius, d):
    """six walls of one radius at +-(radius + d), integers: one K for all six, three opposite pairs; light and camera random"""
    objs = [_sphere(rtm, (0, float(rng.uniform(0.6, 1.0)) * d, 0), float(rng.uniform(0.3, 0.6)) * d, (0, 0, 0), (5, 5, 5))]
    for k in range(6):
        pos = [0.0, 0.0, 0.0]
        pos[k // 2] = float(radius + d) * (1 if k % 2 == 0 else -1)
        objs.append(_sphere(rtm, pos, float(radius), rng.uniform(0.2, 0.9, 3)))
    return _scene(rtm, _room_camera(rtm, rng, float(d)), objs)


def _simple5(rtm, rng):
    """simpleSetting1.json's signature (a sphere at the origin, two on x, the light and the floor on y), other numbers"""
    big = float(10 ** rng.uniform(2, 3.5))
    objs = [_sphere(rtm, (0, 0, 0), rng.uniform(0.5, 1.5), rng.uniform(0.2, 0.9, 3)),
            _sphere(rtm, (float(rng.uniform(2, 5)), 0, 0), rng.uniform(0.5, 1.5), rng.uniform(0.2, 0.9, 3)),
            _sphere(rtm, (-float(rng.uniform(2, 5)), 0, 0), rng.uniform(0.5, 1.5), rng.uniform(0.2, 0.9, 3)),
            _sphere(rtm, (0, float(rng.uniform(4, 8)), 0), rng.uniform(1.5, 3.5), (0.5, 0.5, 0.5), (10, 10, 10)),
            _sphere(rtm, (0, -(big + float(rng.uniform(0.8, 2.0))), 0), big, rng.uniform(0.2, 0.9, 3))]
    cam = rtm.Camera(rtm.vec3(float(rng.uniform(-2, 2)), float(rng.uniform(-0.5, 3)), -float(rng.uniform(6, 12))),
                     rtm.vec3(*_f(rng.uniform(-0.5, 0.5, 3))), rtm.vec3(0, 1, 0), 90.0 if rng.random() < 0.25 else float(rng.uniform(0.8, 2.0)))
    return _scene(rtm, cam, objs)


def _setting3(rtm, rng):
    """settingData.json's signature (the light on y, a sphere at the origin, one on x), other numbers"""
    objs = [_sphere(rtm, (0, float(rng.uniform(6, 12)), 0), rng.uniform(3, 6), (0, 0, 0), (5, 5, 5)),
            _sphere(rtm, (0, 0, 0), rng.uniform(1, 3), rng.uniform(0.2, 0.9, 3)),
            _sphere(rtm, (float(rng.uniform(4, 7)) * (1 if rng.random() < 0.5 else -1), 0, 0), rng.uniform(1, 3), rng.uniform(0.2, 0.9, 3))]
    cam = rtm.Camera(rtm.vec3(float(rng.uniform(-2, 2)), float(rng.uniform(-1, 3)), -float(rng.uniform(7, 12))),
                     rtm.vec3(*_f(rng.uniform(-0.5, 0.5, 3))), rtm.vec3(0, 1, 0), float(rng.uniform(0.8, 2.0)))
    return _scene(rtm, cam, objs)


def _box_with_small_spheres(rtm, rng, n):
    """the shipped box with n - 7 spheres of radius 0.3 to 1 inside (the fuzz script's closed box)"""
    box = F.cornell(rtm, 8, 8, 1, 1)
    objs = list(box.object)
    while len(objs) < n:
        objs.append(_sphere(rtm, rng.uniform(-7, 7, 3), rng.uniform(0.3, 1.0), rng.uniform(0.2, 0.9, 3)))
    return _scene(rtm, box.camera, objs)


def _off_axis(rtm, rng, n):
    """tests/_tol_frames.py: off_axis_scene with other seeds and sizes — sphere 0 around the others and the camera, glowing"""
    outer = float(rng.uniform(20, 40))
    objs = [_sphere(rtm, rng.uniform(0.3, 1.6, 3), outer, (0.55, 0.6, 0.65), (0.5, 0.45, 0.4))]
    scale = float(rng.uniform(0.7, 1.5))
    for k in range(1, n):
        c = rng.uniform(-3.5, 3.5, 3)
        c = np.where(np.abs(c) < 0.05, 0.05, c)
        objs.append(_sphere(rtm, c, scale * (0.45 + 0.9 * k / n + 0.001 * k), 0.25 + 0.65 * rng.random(3)))
    cam = rtm.Camera(rtm.vec3(*_f(rng.uniform(-0.5, 0.5, 3) + np.array([0.0, 0.0, -11.0]))), rtm.vec3(*_f(rng.uniform(-0.3, 0.3, 3))),
                     rtm.vec3(0, 1, 0), float(rng.uniform(0.9, 1.5)))
    return _scene(rtm, cam, objs)


def _first_k(rtm, k):
    box = F.cornell(rtm, 8, 8, 1, 1)
    return _scene(rtm, box.camera, list(box.object)[:k])


def _depth(rng, deep, choices):
    return int(rng.choice(choices if deep else CAPS))


def _case(rtm, i):
    """case i: (data, max_bounces, seed, family); its own generator, so that no case depends on another's draws"""
    rng = np.random.default_rng([POPULATION_SEED, i])
    family = SLOTS[i % len(SLOTS)]
    j = (i // len(SLOTS)) * SLOTS.count(family) + SLOTS[:i % len(SLOTS)].count(family)  # the family's own counter
    if family == "pairs room":       # near the shipped box's scale: the host grants the pairs there
        data, mb = _integer_room(rtm, rng, 10000, int(rng.integers(8, 21))), _depth(rng, j % 2 == 1, DEEP_ROOM)
    elif family == "one-K room":     # the same room at other scales: one K for the six walls, no pairs granted
        data, mb = _integer_room(rtm, rng, int(rng.choice([100, 300, 1000, 3000])), int(rng.integers(4, 13))), _depth(rng, j % 2 == 1, DEEP_ROOM)
    elif family == "axis room":
        data, mb = _axis_room(rtm, rng), _depth(rng, j % 2 == 1, DEEP_ROOM)
    elif family == "simple5":
        data, mb = _simple5(rtm, rng), _depth(rng, j % 4 == 3, DEEP_ROOM)
    elif family == "setting3":
        data, mb = _setting3(rtm, rng), _depth(rng, j % 4 == 3, DEEP_ROOM)
    elif family == "box with small spheres":  # caps 0 .. 8 only: see the module's docstring
        data, mb = _box_with_small_spheres(rtm, rng, BIG_N[j % 7] if j < 14 else int(rng.integers(8, 25))), int(rng.integers(0, 9))
    elif family == "stress":
        data = rtm.make_stress_scene(STRESS_N[j % len(STRESS_N)], seed=int(rng.integers(1 << 30)))
        mb = _depth(rng, (j // len(STRESS_N)) % 2 == 1, DEEP_OPEN)
    elif family == "off axis":
        order = [3, 5, 7, 1, 2, 4, 6, 3, 5, 7, 8, 9, 16, 24, 3, 5, 7, 15, 17, 23]
        n = order[j % len(order)]
        data, mb = _off_axis(rtm, rng, n), _depth(rng, n <= 7 and (j + j // len(order)) % 2 == 1, DEEP_OFF_AXIS)
    else:
        assert family == "first k of the box"
        data, mb = _first_k(rtm, [1, 2, 4, 6, 7, 3, 5, 7][j % 8]), _depth(rng, (j + j // 8) % 2 == 1, DEEP_ROOM)
    # the frame: 1..70 x 1..50, a quarter of the frames under 9 on a side; S x SS^2 on both sides of 16, the stealing threshold
    if rng.random() < 0.25:
        data.width, data.height = int(rng.integers(1, 10)), int(rng.integers(1, 10))
    else:
        data.width, data.height = int(rng.integers(1, 71)), int(rng.integers(1, 51))
    data.samples, data.superSamples = int(rng.choice([1, 2, 3, 4, 5, 8, 16, 32])), int(rng.integers(1, 4))
    return data, mb, int(rng.integers(1 << 40)), family


def population(rtm):
    """[(data, max_bounces, seed)] — 384 repaired-mode frames, the same in every process"""
    return [_case(rtm, i)[:3] for i in range(CASES)]


def families():
    return [SLOTS[i % len(SLOTS)] for i in range(CASES)]


def chunk(k):
    """the case numbers of chunk k of CHUNKS"""
    per = CASES // CHUNKS
    return range(k * per, (k + 1) * per)


def tolerance_case_generator():
    """tests/golden/make_tolerance_case.py as a module (part three's fixture and the script that replays it)"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_tolerance_case.py")
    spec = importlib.util.spec_from_file_location("make_tolerance_case", path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def cell_counts(rtm, cases):
    counts = {}
    for data, mb, _ in cases:
        c = cell(rtm, data, mb)
        counts[c] = counts.get(c, 0) + 1
    return counts
