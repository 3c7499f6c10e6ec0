"""Seeded ray sets and the two discriminant forms of the tolerance row's axis spheres in numpy, shared by
tests/test_axis_disc_host.py and tests/test_axis_disc_gpu.py (csrc/rtm_path.h: sphere_disc / sphere_disc_ref).

Rays: bounces from points ON the scene's spheres (a room's walls seen from inside, any other sphere from outside), the hit
point moved by a relative noise of 1e-13 as a computed hit point is, directions cosine-weighted about the normal and
normalised through a float square root like the reference's Normalize (|d.d - 1| <= 1.8e-7); and camera rays."""
import os

import numpy as np

SCENES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scenes")
ROOM_RADIUS = 1000.0  # a sphere at least this large is a wall: rays start on its inside, within the room


def load_spheres(name):
    """(centres [n, 3], r*r [n] as the geometry rows hold it: the float product widened, camera origin, camera target)"""
    import raytracingmin_amd as rtm
    data = rtm.LoadData(os.path.join(SCENES, name)).data
    c = np.array([[float(o.m_position.x), float(o.m_position.y), float(o.m_position.z)] for o in data.object], dtype=np.float64)
    r = np.array([o.m_size for o in data.object], dtype=np.float32)
    cam = data.camera
    return (c, (r * r).astype(np.float64), np.array([cam.origin.x, cam.origin.y, cam.origin.z], dtype=np.float64),
            np.array([cam.target.x, cam.target.y, cam.target.z], dtype=np.float64), data)


def axis_of(c):
    """1 / 2 / 3 where x / y / z is the centre's only non-zero coordinate, else 0 (csrc/rtm_kernels.hip: axis_pattern)"""
    nz = c != 0.0
    return np.where(nz.sum(axis=1) == 1, np.argmax(nz, axis=1) + 1, 0)


def _normalize_like_the_reference(v):
    len2 = np.einsum("ij,ij->i", v, v).astype(np.float32)
    return v / np.sqrt(len2).astype(np.float64)[:, None]


def _cosine_about(rng, n):
    """cosine-weighted directions about the unit normals n"""
    m = n.shape[0]
    r1, r2 = 2.0 * np.pi * rng.random(m), rng.random(m)
    helper = np.where(np.abs(n[:, :1]) > 0.1, np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
    u = np.cross(helper, n)
    u /= np.linalg.norm(u, axis=1)[:, None]
    v = np.cross(n, u)
    s = np.sqrt(r2)
    return u * (np.cos(r1) * s)[:, None] + v * (np.sin(r1) * s)[:, None] + n * np.sqrt(1.0 - r2)[:, None]


def bounce_rays(rng, c, r2, per_sphere, which, noise=1e-13):
    """per_sphere rays from each sphere of `which` (indices); noise: the hit point's relative error beyond its own rounding"""
    orgs, dirs = [], []
    for i in which:
        r = np.sqrt(r2[i])
        if r >= ROOM_RADIUS:  # a wall: the part of the sphere that faces the origin, 10 units to each side
            a = int(np.argmax(np.abs(c[i])))
            p = rng.uniform(-10.0, 10.0, (per_sphere, 3))
            others = [k for k in range(3) if k != a]
            p[:, a] = c[i, a] - np.sign(c[i, a]) * np.sqrt(r * r - p[:, others[0]] ** 2 - p[:, others[1]] ** 2)
            nrm = (p - c[i]) / r  # the reference's normal, (hit - centre) / r: it points into the room
        else:
            g = rng.normal(size=(per_sphere, 3))
            nrm = g / np.linalg.norm(g, axis=1)[:, None]
            p = c[i] + r * nrm
        p = p * (1.0 + noise * rng.uniform(-1.0, 1.0, p.shape))
        orgs.append(p)
        dirs.append(_normalize_like_the_reference(_cosine_about(rng, nrm)))
    return np.concatenate(orgs), np.concatenate(dirs)


def camera_rays(rng, org, target, m):
    fwd = (target - org) / np.linalg.norm(target - org)
    d = fwd[None, :] + rng.uniform(-1.2, 1.2, (m, 3))
    return np.broadcast_to(org, (m, 3)).copy(), _normalize_like_the_reference(d)


def ray_set(name, n_bounce, n_camera, seed):
    c, r2, cam, target, _ = load_spheres(name)
    rng = np.random.default_rng(seed)
    walls = [i for i in range(len(r2)) if np.sqrt(r2[i]) >= ROOM_RADIUS]
    which = walls if len(walls) >= 6 else list(range(len(r2)))  # a closed room: its walls; else every sphere
    o1, d1 = bounce_rays(rng, c, r2, n_bounce // len(which), which)
    o2, d2 = camera_rays(rng, cam, target, n_camera)
    return c, r2, np.concatenate([o1, o2]), np.concatenate([d1, d2])


def host_rows(data):
    """rtm_debug_axis_rows for the scene's spheres: [n, 4] = (c, -2 c, K, the scene's proven reach or 0) per axis sphere"""
    import ctypes as C
    from raytracingmin_amd import _lib
    _, arr, n = data.to_c()
    rows = (C.c_double * (4 * max(n, 1)))()
    _lib.check(_lib.lib().rtm_debug_axis_rows(arr, n, rows), "axis rows")
    return np.array(rows[:4 * n], dtype=np.float64).reshape(n, 4)


def reference_form(c, r2, axis, org, dir, dtype=np.float64):
    """The tolerance unit's form of rounds 4 to 8 for sphere (c, r2) on `axis` (0: the general form), every operation rounded
    to `dtype`; returns b, D4 and pp + r2 + b^2 (the scale of primary_tie_risk's margin)."""
    o, d = org.astype(dtype), dir.astype(dtype)
    c, r2 = c.astype(dtype), dtype(r2)
    if axis == 0:
        p = c[None, :] - o
        b = p[:, 0] * d[:, 0] + p[:, 1] * d[:, 1] + p[:, 2] * d[:, 2]
        pp = p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2]
    else:
        a = axis - 1
        j, k = [q for q in range(3) if q != a]
        p = c[a] - o[:, a]
        b = p * d[:, a] - (o[:, j] * d[:, j] + o[:, k] * d[:, k])
        pp = p * p + (o[:, j] * o[:, j] + o[:, k] * o[:, k])
    return b, b * b - pp + r2, b * b + pp + r2


def shared_k_group(rows, axis):
    """csrc/rtm_kernels.hip: shared_k_bits — among the first 8 spheres the largest group of axis spheres with one K bit for bit (the
    lowest on a tie), as a boolean per sphere; nobody where no two share"""
    n = min(len(axis), 8)
    best, best_count = np.zeros(len(axis), dtype=bool), 1
    for i in range(n):
        if axis[i] == 0:
            continue
        mask = np.zeros(len(axis), dtype=bool)
        for j in range(i, n):
            mask[j] = axis[j] != 0 and rows[j, 2].tobytes() == rows[i, 2].tobytes()
        if mask.sum() > best_count:
            best, best_count = mask, int(mask.sum())
    return best


def expanded_form(row, c, r2, axis, org, dir, dtype=np.float64, shared=False):
    """The expanded form from the axis row (c_a, -2 c_a, K); an axis-0 sphere keeps the general form.  shared: the sphere is
    in the signature's shared-K group, o.o + K is formed first."""
    if axis == 0:
        b, D4, _ = reference_form(c, r2, 0, org, dir, dtype)
        return b, D4
    o, d = org.astype(dtype), dir.astype(dtype)
    a = axis - 1
    od = o[:, 0] * d[:, 0] + o[:, 1] * d[:, 1] + o[:, 2] * d[:, 2]
    oo = o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1] + o[:, 2] * o[:, 2]
    b = dtype(row[0]) * d[:, a] - od
    cc = dtype(row[1]) * o[:, a] + (oo + dtype(row[2])) if shared else dtype(row[1]) * o[:, a] + oo + dtype(row[2])
    return b, b * b - cc


def accept(b, D4, dis, hit, index):
    """src/SettingData.cpp:205-209 and src/Renderer.cpp:67 on arrays: updates (dis, hit) in place"""
    with np.errstate(invalid="ignore"):
        sq = np.sqrt(D4)
        t1, t2 = b - sq, b + sq
        t = np.where(t1 > 0.001, t1, t2)
        ok = (t < dis) & ~(t < float(np.float32(1e-5)))
    dis[ok] = t[ok]
    hit[ok] = index


def far_sphere_scene(cx, radius):
    """settingData.json's signature (light on the y axis, a sphere at the origin, one on the x axis) with the third sphere small
    and far out: inside the compact-scene extent of 1e7, outside the expanded form's envelope"""
    from raytracingmin_amd import Camera, Material, SettingData, SphereObject, vec3
    objs = [SphereObject(vec3(0, 10, 0), 5.0, Material(vec3(0, 0, 0), vec3(5, 5, 5))),
            SphereObject(vec3(0, 0, 0), 2.0, Material(vec3(.7, .7, .7), vec3(0, 0, 0))),
            SphereObject(vec3(cx, 0, 0), radius, Material(vec3(.7, .7, .7), vec3(.3, .3, .3)))]
    cam = Camera(vec3(cx, 0.0, -4.0 * radius), vec3(cx, 0, 0), vec3(0, 1, 0), 1.5)
    return SettingData(width=48, height=32, samples=4, superSamples=2, camera=cam, object=objs)
