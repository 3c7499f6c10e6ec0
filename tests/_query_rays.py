"""Rays and references for the ray-query tests (include/rtm.h: rtm_scene_nearest, rtm_scene_occluded) — no test in here.

The eight ray kinds and the SPECIAL list are tests/test_grid_gpu.py's, restated (a test module is not imported); the reference
loop is src/Renderer.cpp:58-73 over the oracle's Intersect."""
import ctypes as C
import math

import numpy as np


def normalize_like_the_reference(v):
    """src/Ray.h:67-72: a / (double)sqrtf((float)(a.a))"""
    m = np.sqrt((v * v).sum(axis=1).astype(np.float32)).astype(np.float64)
    return v / m[:, None]


def ray_mix(rng, c, r, count, box, kinds=range(8)):
    """Rays of every kind a render produces, and some it does not, `kinds` in turn: 0 from outside towards the scene
    (camera-like), 1 from sphere surfaces outwards (bounce-like, t1 ~ 0), 2 from inside spheres, 3 silhouette grazes with the
    discriminant swept through zero, 4 axis-parallel directions, 5 one zero component and round origin coordinates, 6 pointing
    away from or past the scene, 7 anywhere, any direction.  c, r: the centres and radii to aim at; box: the scene's half size."""
    kinds = list(kinds)
    n = len(r)
    o = np.empty((count, 3))
    d = np.empty((count, 3))
    for k in range(count):
        kind = kinds[k % len(kinds)]
        i = int(rng.integers(n))
        if kind == 0:
            o[k] = rng.uniform(-1.6, 1.6, 3) * box
            d[k] = c[i] + rng.normal(size=3) * r[i] - o[k]
        elif kind == 1:
            nrm = rng.normal(size=3)
            nrm /= np.linalg.norm(nrm)
            o[k] = c[i] + nrm * r[i]
            v = rng.normal(size=3)
            d[k] = v if v @ nrm > 0 else -v
        elif kind == 2:
            o[k] = c[i] + rng.uniform(-0.5, 0.5, 3) * r[i]
            d[k] = rng.normal(size=3)
        elif kind == 3:
            o[k] = rng.uniform(-1.2, 1.2, 3) * box
            P = c[i] - o[k]
            L = np.linalg.norm(P)
            e = np.cross(P, rng.normal(size=3))
            e /= np.linalg.norm(e)
            delta = (10.0 ** rng.uniform(-17, 0)) * rng.choice([-1.0, 1.0])
            s = math.sqrt(max(r[i] * r[i] + delta, 0.0)) / max(L, 1e-9)
            d[k] = (math.sqrt(1 - s * s) * P / L + s * e) if s < 1 else rng.normal(size=3)
        elif kind == 4:
            o[k] = rng.uniform(-1.0, 1.0, 3) * box
            d[k] = 0.0
            d[k, int(rng.integers(3))] = rng.choice([-1.0, 1.0])
        elif kind == 5:
            o[k] = np.round(rng.uniform(-1.0, 1.0, 3) * box)
            d[k] = rng.normal(size=3)
            d[k, int(rng.integers(3))] = 0.0
        elif kind == 6:
            o[k] = rng.uniform(1.05, 1.5, 3) * box * rng.choice([-1.0, 1.0], 3)
            d[k] = rng.normal(size=3)
        else:
            o[k] = rng.uniform(-1.0, 1.0, 3) * box
            d[k] = rng.normal(size=3)
    return o, normalize_like_the_reference(d)


SPECIAL = [([0, 0, 0], [np.nan, 0, 1]), ([np.inf, 0, 0], [0, 0, 1]), ([0, 0, 0], [np.inf, 0, 0]), ([1e200, 0, 0], [1, 0, 0]),
           ([1e200, 0, 0], [-1, 0, 0]), ([0, 0, 0], [0, 0, 0]), ([0, 0, 0], [1e-200, 0, 0]), ([0, np.nan, 0], [0, 0, 1]),
           ([0, 0, -1e6], [0, 0, 1]), ([3, 4, -5000], [0, 0, 1])]


def query_rays(rng, c, r, count, box, kinds=range(8)):
    """ray_mix with every 97th direction scaled off unit length, and the SPECIAL rays behind them."""
    o, d = ray_mix(rng, c, r, count, box, kinds)
    d[::97] *= rng.uniform(0.5, 3.0, (len(d[::97]), 1))
    o = np.concatenate([o, np.array([s[0] for s in SPECIAL], dtype=np.float64)])
    d = np.concatenate([d, np.array([s[1] for s in SPECIAL], dtype=np.float64)])
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def aim_points(oarr, n, is_object):
    """(centres, radii) to aim rays at: the spheres of an oracle Sphere or Object array."""
    if is_object:
        idx = [i for i in range(n) if oarr[i].type == 1]
        return (np.array([[oarr[i].position[k] for k in range(3)] for i in idx]),
                np.array([oarr[i].size for i in idx], dtype=np.float64))
    return (np.array([[oarr[i].center[k] for k in range(3)] for i in range(n)]),
            np.array([oarr[i].radius for i in range(n)], dtype=np.float64))


def oracle_nearest(oracle, oarr, n, o, d, is_object=False):
    """The loop of src/Renderer.cpp:58-73 over the oracle's repaired-mode Intersect, object i = oarr[i]: (object, t, normal)
    per ray as rtm_scene_nearest defines them — -1, +inf and zeros on a miss; Intersect's normal of the winner, not oriented."""
    L = oracle.lib()
    fn = L.rtmo_intersect_object if is_object else L.rtmo_intersect
    D3 = C.c_double * 3
    ids = np.full(len(o), -1, dtype=np.int32)
    ts = np.full(len(o), np.inf)
    nrm = np.zeros((len(o), 3))
    refs = [C.byref(oarr[i]) for i in range(n)]
    t, tn = C.c_double(), D3()
    for k in range(len(o)):
        org, dr = D3(*o[k]), D3(*d[k])
        dis = np.finfo(np.float64).max  # :60
        for i in range(n):
            t.value = -1.0
            if fn(refs[i], org, dr, oracle.MODE_REPAIRED, C.byref(t), tn) and t.value < dis and t.value > 0:  # :67
                dis = t.value
                ids[k] = i
                nrm[k] = (tn[0], tn[1], tn[2])
        if ids[k] >= 0:
            ts[k] = dis
    return ids, ts, nrm


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))
