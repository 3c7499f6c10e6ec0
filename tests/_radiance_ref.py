"""References and scenes for the radiance-query tests (include/rtm.h: rtm_scene_radiance) — no test in here.

The reference of a call is the oracle's png::PathTracing per (ray, sample) — rtmo_path_trace_stream with the stream (seed,
key_base + i, s) — folded in numpy exactly as the header defines radiance: from +0.0, s ascending, t_s = L_s / S per component,
through the clamp of src/Renderer.cpp:241 when asked; casts and draws summed over the samples."""
import numpy as np


class Samples:
    """Per (ray, sample): L (n, S, 3) float64; casts, draws, max_depth (n, S) int64."""
    def __init__(self, L, casts, draws, max_depth):
        self.L, self.casts, self.draws, self.max_depth = L, casts, draws, max_depth
        self.S = L.shape[1]


def oracle_samples(oracle, oarr, n, o, d, samples, key_base, mode, max_bounces, seed):
    rays = len(o)
    L = np.zeros((rays, samples, 3))
    casts = np.zeros((rays, samples), dtype=np.int64)
    draws = np.zeros((rays, samples), dtype=np.int64)
    deep = np.zeros((rays, samples), dtype=np.int64)
    for i in range(rays):
        for s in range(samples):
            L[i, s], cnt = oracle.path_trace_stream(oarr, n, mode, max_bounces, o[i], d[i], seed, key_base + i, s)
            casts[i, s], draws[i, s], deep[i, s] = cnt["casts"], cnt["draws"], cnt["max_depth"]
    return Samples(L, casts, draws, deep)


def clamp01(v):
    """src/Renderer.cpp:43-49: std::min<double>(std::max<double>(v, 0), 1.0f) — a NaN and a -0 pass through both"""
    lo = np.where(v < 0.0, 0.0, v)
    return np.where(1.0 < lo, 1.0, lo)


def terms(sm):
    """t_s = L_s / (double)S, (n, S, 3)"""
    return sm.L / np.float64(sm.S)


def fold(sm, clamp):
    """(radiance (n, 3) float64, casts (n,) uint32, draws (n,) uint32) as rtm_scene_radiance defines them"""
    t = terms(sm)
    acc = np.zeros((sm.L.shape[0], 3))
    for s in range(sm.S):
        acc = acc + (clamp01(t[:, s]) if clamp else t[:, s])
    return acc, (sm.casts.sum(axis=1) & 0xFFFFFFFF).astype(np.uint32), (sm.draws.sum(axis=1) & 0xFFFFFFFF).astype(np.uint32)


def vacuity(sm):
    """(share of rays with non-zero radiance, share of rays with a term component above 1 — where the clamp changes the
    sum —, samples whose path ran 20 levels deep or more — beyond the kernel's 16 on-chip record levels)"""
    t = terms(sm)
    rad = fold(sm, False)[0]
    return float((rad != 0.0).any(axis=1).mean()), float((t > 1.0).any(axis=(1, 2)).mean()), int((sm.max_depth >= 20).sum())


def box_of_spheres(rng, count=600):
    """The closed box of the grid test: `count` spheres, the first six walls of radius 1e4 at +-(1e4 + 25) on each axis, the
    others of radius 0.3 .. 1.5 in [-20, 20]^3; colour (0.75, 0.6, 0.5); every fifth sphere behind the walls emits (3, 2, 1).
    Returns (centres, radii, emission flags)."""
    c = rng.uniform(-20, 20, (count, 3))
    r = rng.uniform(0.3, 1.5, count)
    c[:6] = [[0, 0, 1e4 + 25], [0, 0, -1e4 - 25], [1e4 + 25, 0, 0], [-1e4 - 25, 0, 0], [0, 1e4 + 25, 0], [0, -1e4 - 25, 0]]
    r[:6] = 1e4
    lit = np.array([i >= 6 and i % 5 == 0 for i in range(count)])
    return c, r, lit


def sphere_array(sphere_type, c, r, lit, colour=(0.75, 0.6, 0.5), emission=(3.0, 2.0, 1.0)):
    """A ctypes array of rtm_sphere / the oracle's Sphere (`sphere_type`) from box_of_spheres' arrays."""
    arr = (sphere_type * len(r))()
    for i in range(len(r)):
        for k in range(3):
            arr[i].center[k] = float(c[i, k])
            arr[i].color[k] = colour[k]
            arr[i].emission[k] = emission[k] if lit[i] else 0.0
        arr[i].radius = float(r[i])
    return arr


def plane_room(rtm, n_spheres, seed, lit_every=3):
    """tests/test_query_gpu.py's _plane_scene restated (a test module is not imported) — a room of six png::PlaneObject walls
    of side 40 around `n_spheres` random spheres, the planes anywhere in the vector, the same draws in the same order — with
    one difference: that scene emits nothing, so its frame is black whatever the camera; here every `lit_every`-th sphere
    made emits (4, 3, 2), which takes no draw."""
    rng = np.random.default_rng(seed)
    data = rtm.SettingData()
    data.camera = rtm.Camera(rtm.vec3(0, 0, -19.0), rtm.vec3(0, 0, 0), rtm.vec3(0, 1, 0), 1.0)
    grey = rtm.vec3(0.75, 0.75, 0.75)
    half = 20.0
    for axis in range(3):
        for sign in (-1.0, 1.0):
            pos = [0.0, 0.0, 0.0]
            pos[axis] = sign * half
            up = rtm.vec3(0, 0, 1) if axis == 1 else rtm.vec3(0, 1, 0)
            data.object.append(rtm.PlaneObject(rtm.vec3(*pos), up, rtm.vec3(0, 0, 0), 2.0 * half, rtm.Material(grey, rtm.vec3(0, 0, 0))))
    for i in range(n_spheres):
        c = rng.uniform(-16.0, 16.0, 3)
        glow = rtm.vec3(4.0, 3.0, 2.0) if i % lit_every == 0 else rtm.vec3(0, 0, 0)
        data.object.insert(int(rng.integers(0, len(data.object) + 1)),
                           rtm.SphereObject(rtm.vec3(*c), float(rng.uniform(0.3, 1.2)), rtm.Material(grey, glow)))
    return data


def camera_rays(oracle, ost):
    """Every pixel's primary ray at sub-pixel (1, 1) in row-major order — ray y * W + x is pixel (x, y), the key a render gives
    it —: (org (W*H, 3), dir (W*H, 3)) from the oracle's camera (src/Renderer.cpp:227-232)."""
    import ctypes as C
    W, H = ost.width, ost.height
    o = np.empty((W * H, 3))
    d = np.empty((W * H, 3))
    out = (C.c_double * 3)()
    for y in range(H):
        for x in range(W):
            oracle.lib().rtmo_primary_dir(C.byref(ost), x, y, 1, 1, out)
            d[y * W + x] = (out[0], out[1], out[2])
            o[y * W + x] = [ost.camera.origin[k] for k in range(3)]
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def camera_rays_numpy(ost):
    """camera_rays for a large frame: src/Renderer.cpp:202-208 and :227-232 at sub-pixel (1, 1) of superSamples 1 restated in
    numpy — separately rounded doubles, the float-length Normalize (src/Ray.h:67-72).  The caller checks some rows against
    camera_rays' (the oracle's own)."""
    def normalize(v):
        m = np.float64(np.sqrt(np.float32((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])))
        return v / np.asarray(m)[..., None]

    def cross(a, b):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])

    W, H = ost.width, ost.height
    origin, target, up = (np.array([v[k] for k in range(3)], dtype=np.float64) for v in (ost.camera.origin, ost.camera.target, ost.camera.up))
    direction = normalize(target - origin)
    cam_x = -normalize(cross(direction, up))
    cam_y = cross(cam_x, direction)
    fovx = float(ost.camera.fov)
    fovy = fovx * H / W
    half = np.float64(np.float32(1.0 / 2.0) * np.float32(1))
    px = 2.0 * (np.arange(W, dtype=np.float64) + half) / W - 1.0
    py = 2.0 * (np.arange(H, dtype=np.float64) + half) / H - 1.0
    v = ((cam_x * fovx)[None, None, :] * px[None, :, None] + (cam_y * fovy)[None, None, :] * py[:, None, None]) + direction
    d = normalize(v.reshape(-1, 3))
    return np.ascontiguousarray(np.broadcast_to(origin, d.shape)), np.ascontiguousarray(d)
