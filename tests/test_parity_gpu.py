"""HIP path vs the CPU oracle, through the C ABI, on a real MI355X (-m gpu).

Tolerances: integer/index results (hit flags, hit ids via draw/cast counts, u8 pixels of RNG-
independent images) are bit-exact.  fp64 radiance/pixels: the only operations whose device
implementation is not required to be correctly rounded are sin/cos (ocml vs glibc, <= 1-2 ulp),
so L1 values are compared with PIXEL_TOL = 1e-9 absolute (north_star allows 1e-4) and the
observed maximum is printed; everything that does not pass through sin/cos is compared exactly.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

from _edge_scenes import AXIS_ROOMS, EDGE_SCENES, _axis_room, _mk  # noqa: F401 (shared with tests/test_tolerance_scenes_gpu.py)

pytestmark = pytest.mark.gpu

# Absolute, per channel, fp64 image vs oracle.  north_star allows 1e-4; the renderer's default
# (host-libm sin/cos, RTM_MODE_HOST_TRIG) is bit-identical to the oracle, so the suite asks for 0.
# Tests of the labelled device-trig row (host_trig=False) state their own expectation.
PIXEL_TOL = 0.0
NORTH_STAR_TOL = 1e-4

SCENES = ["cornellBoxSetting.json", "simpleSetting1.json", "simpleSetting2.json", "settingData.json"]


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    n = C.c_int()
    m._lib.check(m.lib().rtm_device_count(C.byref(n)), "rtm_device_count")
    assert n.value >= 1
    return m


def _variants(rtm, data, max_bounces):
    """Kernel variants that serve this scene: all of them, except that the labelled primary-hit-reuse row
    (variant 15) is built for scenes of 1..24 spheres with a depth cap of at most 8, and the uniform-grid kernel
    (variant 17) needs a scene that gets a grid (64 gridded spheres or more: tests/test_grid_gpu.py asks for it by
    name; variant 0 picks it for every scene that has one)."""
    n = len(data.object)
    live = [v for v in range(rtm.lib().rtm_num_variants()) if not rtm.lib().rtm_variant_name(v).startswith(b"retired")]
    return [v for v in live
            if v not in (16, 17, 18, 19) and (v != 15 or (1 <= n <= 24 and 0 <= max_bounces <= 8))]  # 16: the fp32 row, not a parity path; 18: the fp64 tolerance row (tests/test_tolerance_gpu.py); 19: the other integrator (tests/test_surface_gpu.py)


def _probe(rtm, op, a, b=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = np.empty_like(a)
    bp = None
    if b is not None:
        b = np.ascontiguousarray(b, dtype=np.float64)
        bp = b.ctypes.data
    rtm._lib.check(rtm.lib().rtm_debug_math_probe(op, a.ctypes.data, bp, a.size, out.ctypes.data), "probe")
    return out


def _ulps(a, b):
    return np.abs(a.view(np.int64) - b.view(np.int64))  # same sign assumed


def test_device_primitives_vs_host_libm(rtm):
    rng = np.random.default_rng(7)
    n = 1 << 21
    x = np.concatenate([rng.uniform(0, 4, n), 10.0 ** rng.uniform(-12, 12, n), rng.uniform(0, 1, n)])
    y = 10.0 ** rng.uniform(-6, 6, x.size) * rng.choice([-1.0, 1.0], x.size)
    assert np.array_equal(_probe(rtm, 0, x), np.sqrt(x)), "fp64 sqrt must be correctly rounded"
    xf = x.astype(np.float32)
    assert np.array_equal(_probe(rtm, 1, xf.astype(np.float64)), np.sqrt(xf).astype(np.float64)), "sqrtf"
    assert np.array_equal(_probe(rtm, 2, x, y), x / y), "fp64 division must be correctly rounded"
    # no FMA contraction: x*y+1 must round the product first
    assert np.array_equal(_probe(rtm, 7, x, y), x * y + 1.0)
    # sin/cos at every kind of argument the path produces: r1 = 2*pi*u, u an odd multiple of 2^-24
    u = (2 * rng.integers(0, 1 << 23, n) + 1) / 16777216.0
    r1 = 6.283185307179586 * u
    s_host, c_host = np.sin(r1), np.cos(r1)
    # ocml vs glibc: not bit-identical.  What matters to the path is the ABSOLUTE error of a
    # direction component of magnitude <= 1 (near a zero of sin/cos the ulp distance is large
    # but the absolute one is ~1e-21).
    for op, host in ((3, s_host), (4, c_host), (5, s_host), (6, c_host)):
        d = _probe(rtm, op, r1)
        ul = _ulps(d, host)
        big = np.abs(host) > 0.5
        print(f"op {op}: differing {np.mean(ul > 0):.4%}, max ulp (|v|>0.5) {ul[big].max():.0f}, "
              f"max abs err {np.abs(d - host).max():.3e}")
        assert ul[big].max() <= 1 and np.abs(d - host).max() <= 1.2e-16
    assert np.array_equal(_probe(rtm, 3, r1), _probe(rtm, 5, r1))  # sincos == sin, cos
    assert np.array_equal(_probe(rtm, 4, r1), _probe(rtm, 6, r1))


def test_fast_math_is_bit_identical(rtm):
    """MathFast (shared-reciprocal division, unscaled sqrt; rtm_path.h) must return the bits of the
    compiler's IEEE division / sqrt for every operand class, including the ones that take its
    wave-uniform fallback."""
    rng = np.random.default_rng(21)
    n = 1 << 22
    # sqrt: moderate, tiny (< 2^-767: scaled path), zero, inf, nan, negative
    x = np.concatenate([10.0 ** rng.uniform(-30, 30, n), rng.uniform(0, 1, n), 2.0 ** rng.uniform(-1070, -700, 4096),
                        [0.0, -0.0, np.inf, np.nan, -1.0, 5e-324, 2.0 ** -767, np.nextafter(2.0 ** -767, 0), 1.0, 4.0]])
    with np.errstate(invalid="ignore"):
        want = np.sqrt(x)
    got, ref = _probe(rtm, 8, x), _probe(rtm, 0, x)
    assert np.array_equal(got, ref, equal_nan=True) and np.array_equal(got.view(np.uint64)[:-6], ref.view(np.uint64)[:-6])
    assert np.array_equal(got, want, equal_nan=True)
    # division by a float-valued denominator (what Normalize does), numerators of every class
    yf = np.concatenate([(10.0 ** rng.uniform(-6, 6, n)).astype(np.float32),
                         np.array([0.0, np.inf, 1e-45, 1.0, 3.0, np.float32(1e38), np.float32(1e-38)], dtype=np.float32)])
    y = yf.astype(np.float64) * rng.choice([-1.0, 1.0], yf.size)
    xs = np.concatenate([10.0 ** rng.uniform(-12, 8, y.size - 64) * rng.choice([-1.0, 1.0], y.size - 64),
                         [0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, 1e-310, 1e-300, 1e300, 1e-200, 1e200, 2.0 ** -401,
                          2.0 ** -400, 2.0 ** 400, 2.0 ** 401, 1.0] * 4])
    rng.shuffle(xs)
    with np.errstate(all="ignore"):
        for op, num in ((9, xs), (10, xs), (11, xs)):
            got = _probe(rtm, op, xs, y)
            want = num / y
            same = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
            assert same.all(), (op, xs[~same][:5], y[~same][:5], got[~same][:5], want[~same][:5])


def test_sincos_small_matches_ocml(rtm):
    """The branch-free sincos of the shading block is the operation sequence of ocml's small-argument
    path: bit-identical to ::sincos for EVERY r1 = 2*pi*u the RNG can produce (u = odd * 2^-24)."""
    for lo in range(0, 1 << 23, 1 << 21):
        k = np.arange(lo, lo + (1 << 21), dtype=np.float64)
        r1 = 6.283185307179586 * ((2 * k + 1) / 16777216.0)
        assert np.array_equal(_probe(rtm, 12, r1).view(np.uint64), _probe(rtm, 5, r1).view(np.uint64))
        assert np.array_equal(_probe(rtm, 13, r1).view(np.uint64), _probe(rtm, 6, r1).view(np.uint64))
    x = np.concatenate([np.linspace(0, 1e6, 100001), [0.0, 1e-300, 2.0 ** 29, 1.5707963267948966, 3.141592653589793]])
    assert np.array_equal(_probe(rtm, 12, x).view(np.uint64), _probe(rtm, 5, x).view(np.uint64))
    assert np.array_equal(_probe(rtm, 13, x).view(np.uint64), _probe(rtm, 6, x).view(np.uint64))


def test_device_sincos_vs_host_libm_on_every_rng_argument(rtm, oracle):
    """cos(r1), sin(r1) of src/Renderer.cpp:93-94 for EVERY r1 = 2*pi*u the RNG can produce, device
    against the libm the oracle is linked with.  Neither is required to be correctly rounded; the
    count of arguments on which they differ is what makes whole images bit-identical or not."""
    differing = 0
    worst = 0.0
    for lo in range(0, 1 << 23, 1 << 21):
        k = np.arange(lo, lo + (1 << 21), dtype=np.float64)
        r1 = 6.283185307179586 * ((2 * k + 1) / 16777216.0)
        hs, hc = oracle.sin_cos(r1)
        ds, dc = _probe(rtm, 12, r1), _probe(rtm, 13, r1)
        differing += int(np.count_nonzero(ds.view(np.uint64) != hs.view(np.uint64)))
        differing += int(np.count_nonzero(dc.view(np.uint64) != hc.view(np.uint64)))
        worst = max(worst, float(np.abs(ds - hs).max()), float(np.abs(dc - hc).max()))
    print(f"device sincos vs host libm over all 2^23 arguments: {differing} differing values, max abs err {worst:.3e}")
    assert worst <= 1.2e-16


def _wf_nearest(rtm, kind, sph, n, org, d):
    from raytracingmin_amd import _lib
    org = np.ascontiguousarray(org, dtype=np.float64)
    d = np.ascontiguousarray(d, dtype=np.float64)
    ids = np.zeros(len(org), dtype=np.int32)
    t = np.zeros(len(org), dtype=np.float64)
    _lib.check(rtm.lib().rtm_debug_wf_nearest(kind, sph, n, org.ctypes.data, d.ctypes.data, len(org), ids.ctypes.data,
                                              t.ctypes.data), "wf_nearest")
    return ids, t


def test_large_scene_rejection_test_never_rejects_a_hit(rtm, oracle):
    """wf_nearest_f32_kernel drops a sphere when a packed-fp32 evaluation of its discriminant is below
    -margin.  Rays aimed at the silhouettes of spheres, with the true discriminant swept through zero
    from 1e-6 down to rounding noise on both sides, plus grazing/tangent, inside-the-sphere, far-away
    and non-finite rays, must get the id and distance of the reference's loop with nothing in front of it
    (rtm_debug_wf_nearest kind 1) — and of the oracle."""
    from raytracingmin_amd import _lib
    rng = np.random.default_rng(77)
    n = 1000
    data = rtm.make_stress_scene(n, seed=99)
    _, arr, _ = data.to_c()
    c = np.array([[arr[i].center[k] for k in range(3)] for i in range(n)])
    r = np.array([arr[i].radius for i in range(n)], dtype=np.float64)
    rays_o, rays_d = [], []
    for rep in range(40000):
        i = int(rng.integers(n))
        o = rng.uniform(-60, 60, 3) if rep % 4 else c[int(rng.integers(n))] + rng.normal(size=3) * 0.3
        P = c[i] - o
        L = np.linalg.norm(P)
        if L <= r[i] * 1.01:
            continue
        e = np.cross(P, rng.normal(size=3))
        e /= np.linalg.norm(e)
        delta = (10.0 ** rng.uniform(-17, 0)) * rng.choice([-1.0, 1.0]) * (rep % 7 != 0)
        s = math.sqrt(max(r[i] * r[i] + delta, 0.0)) / L      # sin(theta): D4 ~ -delta
        if s >= 1:
            continue
        d = math.sqrt(1 - s * s) * P / L + s * e
        rays_o.append(o)
        rays_d.append(d if rep % 11 else d * rng.uniform(0.5, 3.0))  # some directions not normalised
    special = [([0, 0, 0], [np.nan, 0, 1]), ([np.inf, 0, 0], [0, 0, 1]), ([0, 0, 0], [np.inf, 0, 0]),
               ([1e200, 0, 0], [1, 0, 0]), ([0, 0, 0], [0, 0, 0]), ([0, 0, 0], [1e-200, 0, 0])]
    for o, d in special:
        rays_o.append(np.array(o, dtype=np.float64))
        rays_d.append(np.array(d, dtype=np.float64))
    rays_o, rays_d = np.array(rays_o), np.array(rays_d)
    ref_id, ref_t = _wf_nearest(rtm, 1, arr, n, rays_o, rays_d)
    for kind in (3,):  # the large-scene kernel: packed-fp32 rejection test + candidate lists
        ids, t = _wf_nearest(rtm, kind, arr, n, rays_o, rays_d)
        assert np.array_equal(ids, ref_id), kind
        assert np.array_equal(t.view(np.uint64), ref_t.view(np.uint64)), kind
    hit = ref_id >= 0
    assert 0.25 < hit.mean() < 0.95  # the sweep straddles the silhouettes
    # the same geometry blown up to where single (1e25) or double (1e160) precision products overflow:
    # the rejection tests must step aside, not hide spheres
    from raytracingmin_amd import _lib
    for scale in (1e25, 1e160):
        big = (_lib.rtm_sphere * n)()
        for i in range(n):
            for k in range(3):
                big[i].center[k] = c[i, k] * scale
            big[i].radius = min(float(r[i]) * scale, 3.0e38)
        o_big = rays_o[:4000] * scale
        want_id, want_t = _wf_nearest(rtm, 1, big, n, o_big, rays_d[:4000])
        for kind in (3,):
            ids, t = _wf_nearest(rtm, kind, big, n, o_big, rays_d[:4000])
            assert np.array_equal(ids, want_id) and np.array_equal(t.view(np.uint64), want_t.view(np.uint64)), (scale, kind)
    oarr = (oracle.Sphere * n).from_buffer_copy(bytes(arr))
    # the oracle's Intersect on the reported sphere gives the reported distance, and no lower-index
    # sphere of a sample of rays gives a closer or equal one
    for k in rng.choice(np.flatnonzero(hit), 300, replace=False):
        h, tt, _ = oracle.intersect(oarr[int(ref_id[k])], rays_o[k], rays_d[k], oracle.MODE_REPAIRED)
        assert h and tt == ref_t[k]
    for k in rng.choice(len(rays_o) - len(special), 40, replace=False):
        best, best_id = np.inf, -1
        for i in range(n):
            h, tt, _ = oracle.intersect(oarr[i], rays_o[k], rays_d[k], oracle.MODE_REPAIRED)
            if h and tt < best and tt > 0:
                best, best_id = tt, i
        assert best_id == ref_id[k]


def test_fast_sqrtf_exhaustive(rtm):
    """The unscaled float sqrt of the shading block equals sqrtf for EVERY float in [2^-96, FLT_MAX]
    (1.9e9 values, checked on the device) and its guard rejects everything outside."""
    bad = C.c_uint64(123)
    rtm._lib.check(rtm.lib().rtm_debug_selfcheck(0, C.byref(bad)), "selfcheck")
    assert bad.value == 0


def test_speculative_math_is_bit_identical(rtm):
    """MathSpec + its validity flag (falls back when set) == compiler math, all operand classes."""
    rng = np.random.default_rng(5)
    n = 1 << 21
    x = np.concatenate([10.0 ** rng.uniform(-30, 30, n), 2.0 ** rng.uniform(-1070, -700, 4096),
                        [0.0, -0.0, np.inf, np.nan, -1.0, 5e-324, 2.0 ** -767, 1.0]])
    with np.errstate(invalid="ignore"):
        want = np.sqrt(x)
    got = _probe(rtm, 14, x)
    assert np.array_equal(got, want, equal_nan=True)
    yf = np.concatenate([(10.0 ** rng.uniform(-6, 6, x.size - 6)).astype(np.float32),
                         np.array([0.0, np.inf, 1e-45, 1.0, 3.0, np.float32(1e38)], dtype=np.float32)])
    y = yf.astype(np.float64)
    with np.errstate(all="ignore"):
        want = x / y
        got = _probe(rtm, 15, x, y)
    same = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    assert same.all()


def test_device_rng_matches_host_and_oracle(rtm, oracle):
    out = np.zeros((64, 40), dtype=np.float64)
    rtm._lib.check(rtm.lib().rtm_rng_batch(0x5EED, 1000, 64, 3, 40, out.ctypes.data), "rng_batch")
    for p in range(64):
        for k in (0, 1, 2, 17, 39):
            assert out[p, k] == oracle.lib().rtmo_rng_u01(0x5EED, 1000 + p, 3, k)
            assert out[p, k] == rtm.lib().rtm_rng_u01(0x5EED, 1000 + p, 3, k)


@pytest.mark.parametrize("mode", ["literal", "repaired"])
def test_intersect_batch_bit_exact(rtm, oracle, mode):
    rng = np.random.default_rng(3)
    n = 4096
    sph = (oracle.Sphere * n)()
    org = rng.uniform(-12, 12, (n, 3))
    d = rng.normal(size=(n, 3))
    for i in range(n):
        big = i % 3 == 0
        c = rng.uniform(-1, 1, 3) * (10010 if big else 8)
        for k in range(3):
            sph[i].center[k] = c[k]
        sph[i].radius = 10000.0 if big else float(rng.uniform(0.1, 6))
        d[i] = oracle.normalize(d[i])
    d[5] = [float("nan")] * 3  # NaN ray: "returns true with t = NaN" 
    hit, t, nrm = rtm.intersect_batch(sph, org, d, mode=mode)
    m = oracle.MODE_LITERAL if mode == "literal" else oracle.MODE_REPAIRED
    n_hit = 0
    for i in range(n):
        h, tt, nn = oracle.intersect(sph[i], org[i], d[i], m)
        assert h == hit[i]
        if h:
            n_hit += 1
            assert (tt == t[i]) or (math.isnan(tt) and math.isnan(t[i]))
            if mode == "repaired" and not math.isnan(tt):
                assert nn == list(nrm[i])
            if mode == "literal":
                assert list(nrm[i]) == [7.0, 7.0, 7.0]  # D2: caller's normal untouched
        else:
            assert t[i] == -1.0 and list(nrm[i]) == [7.0, 7.0, 7.0]
    assert 200 < n_hit < n


def test_known_answer_rays_on_device(rtm, oracle):
    """SURVEY §8(c) per-ray answers that do not depend on the RNG: straight at the light."""
    data = rtm.LoadData(oracle.scene_path("cornellBoxSetting.json")).data
    org = np.tile([0.0, 0.0, -10.0], (2, 1))
    d = np.array([oracle.normalize([0.05, 0.9, 1]), oracle.normalize([0.05, 0.9, 1])])
    L, draws, casts = rtm.path_tracing_batch(data, org, d, mode="repaired")
    assert L.tolist() == [[5, 5, 5], [5, 5, 5]] and draws.tolist() == [1, 1] and casts.tolist() == [1, 1]
    lit = rtm.LoadData(oracle.scene_path("cornellBoxSetting.json"), literal_loader=True).data
    d0 = np.array([oracle.normalize([0, 0, 1]), oracle.normalize([1, 0, 0.2])])
    L, draws, casts = rtm.path_tracing_batch(lit, org, d0, mode="literal", seed=1)
    assert L.tolist() == [[5, 5, 5], [0, 0, 0]] and draws[0] == 1 and draws[1] in (1, 3)


@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("max_bounces", [-1, 8, 0, 2])
def test_path_tracing_batch_vs_oracle(rtm, oracle, scene, max_bounces):
    data = rtm.LoadData(oracle.scene_path(scene)).data
    st, arr, n = oracle.load_scene(oracle.scene_path(scene))
    rng = np.random.default_rng(11)
    n_rays = 3000
    org = np.tile(list(data.camera.origin), (n_rays, 1)) + rng.uniform(-0.5, 0.5, (n_rays, 3))
    d = np.array([oracle.normalize(v) for v in rng.normal(size=(n_rays, 3))])
    L, draws, casts = rtm.path_tracing_batch(data, org, d, mode="repaired", max_bounces=max_bounces, seed=99)
    worst = 0.0
    for i in range(n_rays):
        Lo, cnt = oracle.path_trace_stream(arr, n, oracle.MODE_REPAIRED, max_bounces, org[i], d[i], 99, i)
        assert cnt["draws"] == draws[i] and cnt["casts"] == casts[i], (i, cnt, draws[i], casts[i])
        worst = max(worst, float(np.max(np.abs(np.array(Lo) - L[i]))))
    print(f"{scene} max_bounces={max_bounces}: max |L_gpu - L_oracle| = {worst:.3e}, "
          f"mean casts {casts.mean():.3f}, deepest {casts.max()}")
    assert worst <= PIXEL_TOL


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FROZEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frozen")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def test_frozen_seam_fixtures(rtm):
    """The committed expected outputs (tests/golden/frozen, frozen from the pinned oracle) for the two
    seams below the renderer — no oracle involved at test time."""
    import ctypes as C
    from raytracingmin_amd import _lib
    z = np.load(os.path.join(FROZEN, "intersect_1k.npz"))
    n = len(z["radius"])
    sph = (_lib.rtm_sphere * n)()
    for i in range(n):
        for k in range(3):
            sph[i].center[k] = z["center"][i, k]
        sph[i].radius = float(z["radius"][i])
    for mode in ("literal", "repaired"):
        hit, t, nrm = rtm.intersect_batch(sph, z["org"], z["dir"], mode=mode)
        assert np.array_equal(hit, z[f"hit_{mode}"])
        assert np.array_equal(_bits(t), _bits(z[f"t_{mode}"]))
        assert np.array_equal(_bits(nrm), _bits(z[f"normal_{mode}"]))
    assert 200 < int(z["hit_repaired"].sum()) < n
    z = np.load(os.path.join(FROZEN, "pathtrace_1k.npz"))
    data = rtm.LoadData(os.path.join(ROOT, "scenes", "cornellBoxSetting.json")).data
    for tag, mb in (("cap8", 8), ("unlimited", -1)):
        L, draws, casts = rtm.path_tracing_batch(data, z["org"], z["dir"], mode="repaired", max_bounces=mb,
                                                 seed=int(z["seed"]))
        assert np.array_equal(draws, z[f"draws_{tag}"]) and np.array_equal(casts, z[f"casts_{tag}"])
        assert np.array_equal(_bits(L), _bits(z[f"radiance_{tag}"]))


@pytest.mark.parametrize("scene", ["cornellBoxSetting", "simpleSetting1", "simpleSetting2", "settingData"])
def test_frozen_images(rtm, scene):
    """64x64, 16 spp frames of every shipped scene against the committed raw float64 images."""
    z = np.load(os.path.join(FROZEN, f"image_{scene}.npz"))
    path = os.path.join(ROOT, "scenes", scene + ".json")
    for mode in ("repaired", "literal"):
        if f"image_{mode}" not in z.files:
            continue
        data = rtm.LoadData(path, literal_loader=(mode == "literal")).data
        data.width, data.height, data.samples, data.superSamples = 64, 64, 4, 2
        for variant in (0, 1, 9):
            out, stats = _gpu_image(rtm, data, mode, -1, 0x5EED, want=("f64",), variant=variant)
            assert np.array_equal(_bits(out["f64"]), _bits(z[f"image_{mode}"])), (mode, variant)
            assert stats["casts"] == int(z[f"casts_{mode}"]) and stats["draws"] == int(z[f"draws_{mode}"])


def _gpu_image(rtm, data, mode, max_bounces, seed, want=("f64", "f32", "u8"), rows=None, variant=0):
    r = rtm.Renderer(data, mode=mode, max_bounces=max_bounces, seed=seed, variant=variant)
    rb, re = rows if rows else (0, data.height)
    out, stats = r.render_rows(rb, re, want=want)
    return out, stats


@pytest.mark.parametrize("scene,w,h,s,ss", [("cornellBoxSetting.json", 96, 64, 4, 2),
                                            ("cornellBoxSetting.json", 67, 45, 3, 3),  # ragged tiles
                                            ("simpleSetting1.json", 80, 48, 16, 1),
                                            ("simpleSetting2.json", 64, 64, 8, 2),
                                            ("settingData.json", 96, 50, 10, 1)])
@pytest.mark.parametrize("max_bounces", [-1, 8])
def test_render_repaired_vs_oracle(rtm, oracle, scene, w, h, s, ss, max_bounces):
    st, arr, n = oracle.load_scene(oracle.scene_path(scene), width=w, height=h, samples=s, super_samples=ss)
    ref, cnt = oracle.render(st, arr, n, oracle.make_options(mode=1, max_bounces=max_bounces, seed=0x5EED, height=h))
    data = rtm.LoadData(oracle.scene_path(scene)).data
    data.width, data.height, data.samples, data.superSamples = w, h, s, ss
    out, stats = _gpu_image(rtm, data, "repaired", max_bounces, 0x5EED)
    err = float(np.max(np.abs(out["f64"] - ref)))
    print(f"{scene} {w}x{h} S{s} SS{ss} mb={max_bounces}: max pixel delta {err:.3e}; casts/sample "
          f"{stats['casts'] / stats['samples']:.4f}")
    assert err <= PIXEL_TOL
    # integer bookkeeping is exact
    assert stats["samples"] == cnt["samples"] == w * h * s * ss * ss
    assert (stats["casts"], stats["bounces"], stats["draws"]) == (cnt["casts"], cnt["bounces"], cnt["draws"])
    # float3 buffer is the fp64 image rounded once; u8 is the reference quantiser of the fp64 image
    assert np.array_equal(out["f32"], out["f64"].astype(np.float32))
    assert np.array_equal(out["u8"], oracle.quantise(out["f64"]))
    assert np.mean(out["u8"] != oracle.quantise(ref)) < 1e-3


def test_render_literal_matches_reference_golden_hashes(rtm, oracle):
    """L0 is RNG-independent, so the GPU image must hash to the reference's own golden values."""
    import json
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "survey_8c.json")))
    for case in gold["L0_images"]:
        data = rtm.LoadData(oracle.scene_path(case["scene"]), literal_loader=True).data
        data.width, data.height = case["width"], case["height"]
        data.samples, data.superSamples = case["samples"], case["super_samples"]
        out, stats = _gpu_image(rtm, data, "literal", -1, seed=4242, want=("f64", "u8"))
        assert f"{oracle.fnv(out['f64']):016x}" == case["fnv1a64"], case
        assert float(out["f64"].sum()) == case["sum"] and int((out["f64"] != 0).sum()) == case["nonzero"]
        if "white_pixels_rgb8" in case:
            assert int((out["u8"].reshape(-1, 3) == 255).all(axis=1).sum()) == case["white_pixels_rgb8"]


@pytest.mark.parametrize("scene,mode,max_bounces", [("cornellBoxSetting.json", "repaired", 8),
                                                    ("cornellBoxSetting.json", "repaired", -1),
                                                    ("cornellBoxSetting.json", "literal", -1),
                                                    ("simpleSetting2.json", "repaired", -1),
                                                    ("settingData.json", "repaired", 3),
                                                    ("cornellBoxSetting.json", "literal", 8),
                                                    ("simpleSetting1.json", "repaired", 0)])
def test_kernel_variants_are_bit_identical(rtm, oracle, scene, mode, max_bounces):
    """Every kernel variant (reference math / fast math, global / LDS scene tables, non-power-of-
    two and power-of-two sample counts) produces the same bits and the same counters."""
    data = rtm.LoadData(oracle.scene_path(scene), literal_loader=(mode == "literal")).data
    for (w, h, s, ss) in ((200, 120, 8, 2), (61, 37, 5, 3)):
        data.width, data.height, data.samples, data.superSamples = w, h, s, ss
        names = [rtm.lib().rtm_variant_name(v).decode() for v in range(rtm.lib().rtm_num_variants())]
        ref, ref_stats = _gpu_image(rtm, data, mode, max_bounces, 0x5EED, want=("f64", "u8"), variant=1)
        for v in _variants(rtm, data, max_bounces):
            out, st = _gpu_image(rtm, data, mode, max_bounces, 0x5EED, want=("f64", "u8"), variant=v)
            assert np.array_equal(out["f64"].view(np.uint64), ref["f64"].view(np.uint64)), names[v]
            assert np.array_equal(out["u8"], ref["u8"])
            assert {k: st[k] for k in ("samples", "casts", "bounces", "draws")} == \
                {k: ref_stats[k] for k in ("samples", "casts", "bounces", "draws")}, names[v]


def _stress(rtm, oracle, n, w, h, s):
    data = rtm.make_stress_scene(n=n, seed=12345)
    data.width, data.height, data.samples, data.superSamples = w, h, s, 1
    st, arr, cn = data.to_c()
    ost = oracle.Settings.from_buffer_copy(bytes(st))
    oarr = (oracle.Sphere * max(cn, 1)).from_buffer_copy(bytes(arr))
    return data, ost, oarr


@pytest.mark.parametrize("n,w,h,s", [(300, 64, 40, 4), (3000, 48, 32, 4), (100_000, 32, 16, 2)])
def test_stress_scene_vs_oracle(rtm, oracle, n, w, h, s):
    """BASELINE configs[4] scene family: many small spheres, u32 hit records,
    scene streamed per cast; lowest index must still win exact ties."""
    data, ost, oarr = _stress(rtm, oracle, n, w, h, s)
    ref, cnt = oracle.render(ost, oarr, n, oracle.make_options(mode=1, max_bounces=8, seed=5, height=h))
    base = None
    for v in _variants(rtm, data, 8):
        out, stats = _gpu_image(rtm, data, "repaired", 8, 5, want=("f64",), variant=v)
        err = float(np.max(np.abs(out["f64"] - ref)))
        print(f"stress n={n} variant {v}: max pixel delta {err:.3e}, casts/sample "
              f"{stats['casts'] / stats['samples']:.3f}, kernel {stats['kernel_ms']:.1f} ms")
        assert err <= PIXEL_TOL
        assert (stats["casts"], stats["bounces"], stats["draws"]) == (cnt["casts"], cnt["bounces"], cnt["draws"])
        if base is None:
            base = out["f64"]
        assert np.array_equal(out["f64"].view(np.uint64), base.view(np.uint64))


def test_large_scene_long_candidate_lists(rtm, oracle):
    """The large-scene pipeline notes the spheres a lane could not reject in per-lane candidate lists of 16 slots and
    settles them with the reference's arithmetic (csrc/rtm_wavefront.h, src/SettingData.cpp:197-226).  Nested shells
    around the light put hundreds of candidates on every ray through the centre — the lists fill many times per
    sweep — with exact ties among them (every 7th shell repeats the radius of its predecessor: the lowest index must
    win, src/Renderer.cpp:67) and the true nearest hit anywhere in index order."""
    rng = np.random.default_rng(77)
    cam = rtm.Camera(rtm.vec3(0, 0, -30), rtm.vec3(0, 0, 0), rtm.vec3(0, 1, 0), 1.0)
    objs = []
    r = 1.0
    for k in range(620):
        if k % 7 != 6:
            r = float(rng.uniform(0.5, 6.0))
        c = rng.uniform(-0.3, 0.3, 3) if k % 3 else np.zeros(3)
        col = rng.uniform(0.3, 0.9, 3)
        em = (4.0, 3.0, 2.0) if k % 50 == 0 else (0.0, 0.0, 0.0)
        objs.append(rtm.SphereObject(rtm.vec3(*map(float, c)), r, rtm.Material(rtm.vec3(*map(float, col)), rtm.vec3(*em))))
    objs.append(rtm.SphereObject(rtm.vec3(0, 0, 0), 60.0, rtm.Material(rtm.vec3(0.7, 0.7, 0.7), rtm.vec3(0.5, 0.5, 0.5))))
    data = rtm.SettingData(width=40, height=24, samples=4, superSamples=1, camera=cam, object=objs)
    st, arr, n = data.to_c()
    ost = oracle.Settings.from_buffer_copy(bytes(st))
    oarr = (oracle.Sphere * n).from_buffer_copy(bytes(arr))
    ref, cnt = oracle.render(ost, oarr, n, oracle.make_options(mode=1, max_bounces=6, seed=9, height=24))
    seen = set()
    for v in _variants(rtm, data, 6):
        out, stats = _gpu_image(rtm, data, "repaired", 6, 9, want=("f64",), variant=v)
        seen.add(stats["variant"])
        assert np.array_equal(out["f64"].view(np.uint64), ref.view(np.uint64)), f"variant {v}"
        assert (stats["casts"], stats["bounces"], stats["draws"]) == (cnt["casts"], cnt["bounces"], cnt["draws"])
    assert 12 in seen  # the packed-fp32 rejection pipeline with the candidate lists took part


def test_coincident_spheres_lowest_index_wins(rtm, oracle):
    """Exact ties (the literal Cornell scene has four coincident spheres): strict < keeps the
    lowest index (src/Renderer.cpp:67), also across geometry batches."""
    base = rtm.LoadData(oracle.scene_path("cornellBoxSetting.json")).data
    wall = base.object[1]
    objs = []
    for k in range(11):  # 11 coincident walls with different colours + the light
        o = rtm.SphereObject(rtm.vec3(0, 0, 0), 50.0, rtm.Material(rtm.vec3(0.1 + 0.07 * k, 0.5, 0.9 - 0.07 * k), rtm.vec3(0, 0, 0)))
        objs.append(o)
    objs.insert(5, base.object[0])
    data = rtm.SettingData(width=40, height=24, samples=4, superSamples=2, camera=base.camera, object=objs)
    st, arr, n = data.to_c()
    ost = oracle.Settings.from_buffer_copy(bytes(st))
    oarr = (oracle.Sphere * n).from_buffer_copy(bytes(arr))
    ref, cnt = oracle.render(ost, oarr, n, oracle.make_options(mode=1, max_bounces=6, seed=3, height=24))
    for v in _variants(rtm, data, 6):
        out, stats = _gpu_image(rtm, data, "repaired", 6, 3, want=("f64",), variant=v)
        assert float(np.max(np.abs(out["f64"] - ref))) <= PIXEL_TOL
        assert stats["casts"] == cnt["casts"]


def _white_room(rtm, albedo, w=24, h=16, s=4):
    cam = rtm.Camera(rtm.vec3(0, 0, -3), rtm.vec3(0, 0, 0), rtm.vec3(0, 1, 0), 1.0)
    room = rtm.SphereObject(rtm.vec3(0, 0, 0), 20.0, rtm.Material(rtm.vec3(albedo, albedo, albedo), rtm.vec3(0, 0, 0)))
    lamp = rtm.SphereObject(rtm.vec3(0, 12, 0), 4.0, rtm.Material(rtm.vec3(0, 0, 0), rtm.vec3(3, 2, 1)))
    return rtm.SettingData(width=w, height=h, samples=s, superSamples=1, camera=cam, object=[room, lamp])


def test_deep_paths_use_record_pool(rtm, oracle):
    """Unlimited recursion: paths far deeper than the LDS record levels (64) spill to the global
    record pool and still fold exactly like the recursion."""
    data = _white_room(rtm, 0.975)
    st, arr, n = data.to_c()
    ost = oracle.Settings.from_buffer_copy(bytes(st))
    oarr = (oracle.Sphere * n).from_buffer_copy(bytes(arr))
    ref, cnt = oracle.render(ost, oarr, n, oracle.make_options(mode=1, max_bounces=-1, seed=11, height=data.height))
    assert cnt["max_depth"] > 80  # well past the 64 LDS levels
    for v in _variants(rtm, data, -1):
        out, stats = _gpu_image(rtm, data, "repaired", -1, 11, want=("f64",), variant=v)
        assert float(np.max(np.abs(out["f64"] - ref))) <= PIXEL_TOL
        assert (stats["casts"], stats["draws"]) == (cnt["casts"], cnt["draws"])
    # a cap beyond the LDS levels goes through the pool too
    ref, cnt = oracle.render(ost, oarr, n, oracle.make_options(mode=1, max_bounces=100, seed=11, height=data.height))
    out, stats = _gpu_image(rtm, data, "repaired", 100, 11, want=("f64",))
    assert float(np.max(np.abs(out["f64"] - ref))) <= PIXEL_TOL and stats["casts"] == cnt["casts"]


def test_record_overflow_fails_loudly(rtm):
    """A path deeper than LDS + pool capacity must raise, never truncate silently (the reference
    itself would overflow its call stack on such a scene)."""
    data = _white_room(rtm, 0.99995, w=8, h=8, s=1)
    data.object[1].m_material.color = rtm.vec3(0.99995, 0.99995, 0.99995)  # the lamp no longer ends paths
    with pytest.raises(rtm.RtmError) as e:
        _gpu_image(rtm, data, "repaired", -1, 1, want=("f64",))
    assert e.value.status == -8 and "deeper" in str(e.value)
    with pytest.raises(rtm.RtmError):
        _gpu_image(rtm, data, "repaired", 5000, 1, want=("f64",))


def _oracle_view(oracle, data):
    st, arr, n = data.to_c()
    return (oracle.Settings.from_buffer_copy(bytes(st)),
            (oracle.Sphere * max(n, 1)).from_buffer_copy(bytes(arr)), n)


@pytest.mark.parametrize("name", sorted(EDGE_SCENES))
def test_edge_case_scenes_vs_oracle(rtm, oracle, name):
    objs, origin, fov = EDGE_SCENES[name](rtm)
    cam = rtm.Camera(rtm.vec3(*origin), rtm.vec3(0, 0, 0), rtm.vec3(0, 1, 0), fov)
    data = rtm.SettingData(width=45, height=27, samples=3, superSamples=2, camera=cam, object=objs)
    ost, oarr, n = _oracle_view(oracle, data)
    for mode, mb in (("repaired", 8), ("repaired", 3), ("repaired", 1), ("repaired", 0), ("literal", -1), ("literal", 2)):
        m = oracle.MODE_REPAIRED if mode == "repaired" else oracle.MODE_LITERAL
        ref, cnt = oracle.render(ost, oarr, n, oracle.make_options(mode=m, max_bounces=mb, seed=17, height=27))
        for v in (0, 1, 3, 12, 9, 14):
            out, stats = _gpu_image(rtm, data, mode, mb, 17, want=("f64",), variant=v)
            assert np.allclose(out["f64"], ref, rtol=0, atol=PIXEL_TOL, equal_nan=True), (name, mode, mb, v)
            assert (stats["casts"], stats["draws"]) == (cnt["casts"], cnt["draws"]), (name, mode, mb, v)


@pytest.mark.parametrize("name", sorted(AXIS_ROOMS))
def test_axis_signature_scenes_vs_oracle(rtm, oracle, name):
    """Scenes that get the axis-signature instantiation of the exact-n kernels (rtm_path.h: sphere_disc — discriminants of
    spheres whose centre sits on a coordinate axis, from per-ray shared products): image, counters, every depth setting the
    instantiation exists for (cap <= 8: packed records; any depth: PACKL), against the oracle and the per-object loop."""
    objs, origin = AXIS_ROOMS[name](rtm)
    cam = rtm.Camera(rtm.vec3(*origin), rtm.vec3(0, 0, 0), rtm.vec3(0, 1, 0), 1.6)
    data = rtm.SettingData(width=56, height=40, samples=4, superSamples=2, camera=cam, object=objs)
    ost, oarr, n = _oracle_view(oracle, data)
    for mode, mb in (("repaired", 8), ("repaired", -1), ("repaired", 3), ("repaired", 12), ("literal", -1)):
        m = oracle.MODE_REPAIRED if mode == "repaired" else oracle.MODE_LITERAL
        ref, cnt = oracle.render(ost, oarr, n, oracle.make_options(mode=m, max_bounces=mb, seed=23, height=40))
        for v in (0, 2, 9, 1):
            out, stats = _gpu_image(rtm, data, mode, mb, 23, want=("f64",), variant=v)
            assert np.array_equal(out["f64"], ref, equal_nan=True), (name, mode, mb, v)
            assert (stats["casts"], stats["draws"]) == (cnt["casts"], cnt["draws"]), (name, mode, mb, v)


def test_axis_signature_near_misses_take_the_general_kernel(rtm, oracle):
    """One coordinate a denormal instead of zero, or the spheres in another order: not the signature — same answers."""
    base = rtm.LoadData(oracle.scene_path("cornellBoxSetting.json")).data
    objs = list(base.object)
    tiny = _mk(rtm, (5e-324, 10, 0), 5, (0, 0, 0), (5, 5, 5))
    for variant_objs in ([tiny] + objs[1:], objs[1:] + objs[:1], objs[:6]):
        data = rtm.SettingData(width=40, height=24, samples=4, superSamples=2, camera=base.camera, object=variant_objs)
        ost, oarr, n = _oracle_view(oracle, data)
        for mb in (8, -1):
            ref, cnt = oracle.render(ost, oarr, n, oracle.make_options(mode=1, max_bounces=mb, seed=3, height=24))
            out, stats = _gpu_image(rtm, data, "repaired", mb, 3, want=("f64",))
            assert np.array_equal(out["f64"], ref) and stats["casts"] == cnt["casts"]


def test_degenerate_camera_gives_the_same_nans(rtm, oracle):
    """upVec parallel to the view direction: Cross(direction, up) = 0, its Normalize is 0/0 and every
    primary ray is NaN (src/Renderer.cpp:203).  The reference then renders black (NaN rays miss); so
    must the GPU, in both modes."""
    base = rtm.LoadData(oracle.scene_path("cornellBoxSetting.json")).data
    cam = rtm.Camera(rtm.vec3(0, 0, -10), rtm.vec3(0, 0, 0), rtm.vec3(0, 0, 1), 2.0)
    data = rtm.SettingData(width=24, height=16, samples=2, superSamples=1, camera=cam, object=base.object)
    ost, oarr, n = _oracle_view(oracle, data)
    for mode, m in (("repaired", oracle.MODE_REPAIRED), ("literal", oracle.MODE_LITERAL)):
        ref, cnt = oracle.render(ost, oarr, n, oracle.make_options(mode=m, max_bounces=8, seed=1, height=16))
        out, stats = _gpu_image(rtm, data, mode, 8, 1, want=("f64", "u8"))
        assert np.array_equal(out["f64"], ref, equal_nan=True) and not ref.any()
        assert stats["casts"] == cnt["casts"] == 24 * 16 * 2


def test_one_pixel_one_sample(rtm, oracle):
    data = rtm.LoadData(oracle.scene_path("simpleSetting1.json")).data
    data.width, data.height, data.samples, data.superSamples = 1, 1, 1, 1
    ost, oarr, n = _oracle_view(oracle, data)
    ref, _ = oracle.render(ost, oarr, n, oracle.make_options(mode=1, max_bounces=-1, seed=5, height=1))
    out, stats = _gpu_image(rtm, data, "repaired", -1, 5)
    assert np.array_equal(out["f64"], ref) and stats["samples"] == 1


@pytest.mark.parametrize("w,h,s,ss,mb", [(64, 40, 8, 2, 8),    # split on sub-pixel boundaries
                                          (45, 27, 8, 3, 8),    # 72 samples: ranges start inside a sub-pixel
                                          (40, 24, 24, 1, -1),  # unlimited depth (LDS records + pool)
                                          (33, 17, 5, 2, 12),   # 20 samples: two waves of 10
                                          (40, 24, 125, 2, 8),  # 500 samples: 20 shares of 25 (not a power of two)
                                          (24, 16, 5, 3, 8),    # 45 samples: 5 shares of 9, an odd count: wave 0 keeps 3
                                          (16, 16, 256, 4, 8)])  # 4096 samples: 64 shares of 64, 29 waves per tile
def test_sample_split_is_bit_identical(rtm, oracle, w, h, s, ss, mb):
    """Several waves per tile, each tracing a range of the pixel's samples; the terms are added in the
    reference's order afterwards (src/Renderer.cpp:241-242), so nothing may change."""
    st, arr, n = oracle.load_scene(oracle.scene_path("cornellBoxSetting.json"), width=w, height=h, samples=s,
                                   super_samples=ss)
    ref, cnt = oracle.render(st, arr, n, oracle.make_options(mode=1, max_bounces=mb, seed=99, height=h))
    data = rtm.LoadData(oracle.scene_path("cornellBoxSetting.json")).data
    data.width, data.height, data.samples, data.superSamples = w, h, s, ss
    names = [rtm.lib().rtm_variant_name(v).decode() for v in range(rtm.lib().rtm_num_variants())]
    split = [i for i, nm in enumerate(names) if nm.endswith("sample-split")][0]
    whole, st_whole = _gpu_image(rtm, data, "repaired", mb, 99, variant=2)
    parts, st_parts = _gpu_image(rtm, data, "repaired", mb, 99, variant=split)
    for k in ("f64", "f32", "u8"):
        assert np.array_equal(whole[k], parts[k]), k
    assert np.array_equal(parts["f64"], ref)
    assert {k: st_parts[k] for k in ("samples", "casts", "bounces", "draws")} == \
           {k: st_whole[k] for k in ("samples", "casts", "bounces", "draws")}
    assert st_parts["casts"] == cnt["casts"]
    # a strip of the frame, too (tile rows are relative to row_begin)
    strip, _ = _gpu_image(rtm, data, "repaired", mb, 99, want=("f64",), rows=(8, h), variant=split)
    assert np.array_equal(strip["f64"], ref[8:])


@pytest.mark.parametrize("scene,w,h,n_big", [("cornellBoxSetting.json", 50, 45, 0), ("simpleSetting1.json", 40, 64, 0),
                                             ("stress", 40, 29, 300)])
def test_interleaved_bands_reassemble_the_frame(rtm, oracle, scene, w, h, n_big):
    """rtm_options.band_count/band_index (the multi-GPU deal of 8-row bands): the stacks of all ranks,
    put back by band_row_index, are the frame bit for bit; so are the counters' sums."""
    from raytracingmin_amd.distributed import band_row_index
    if scene == "stress":
        data = rtm.make_stress_scene(n_big, seed=7)
        data.width, data.height, data.samples, data.superSamples = w, h, 2, 2
    else:
        data = rtm.LoadData(oracle.scene_path(scene)).data
        data.width, data.height, data.samples, data.superSamples = w, h, 4, 2
    for variant in (0, 1, 3, 12, 9):
        full, st_full = _gpu_image(rtm, data, "repaired", 8, 3, want=("f64", "u8"), variant=variant)
        for lo, hi, world in ((0, h, 3), (8, h - 3, 2), (0, h, 8)):
            got = np.full_like(full["f64"], np.nan)
            casts = 0
            for rank in range(world):
                r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=3, variant=variant)
                out, st = r.render_rows(lo, hi, want=("f64", "u8"), band=(world, rank))
                idx = band_row_index(lo, hi, world, rank)
                assert out["f64"].shape[0] == len(idx)
                got[idx] = out["f64"]
                assert np.array_equal(out["u8"], full["u8"][idx])
                casts += st["casts"]
            assert np.array_equal(got[lo:hi], full["f64"][lo:hi]), (variant, lo, hi, world)
            assert np.isnan(got[:lo]).all() and np.isnan(got[hi:]).all()
            if (lo, hi) == (0, h):
                assert casts == st_full["casts"]
    with pytest.raises(rtm.RtmError):
        rtm.Renderer(data, mode="repaired", max_bounces=8).render_rows(0, h, band=(2, 2))


@pytest.mark.parametrize("n", [25, 60, 511, 512])
def test_auto_variant_by_scene_size(rtm, oracle, n):
    """variant 0 picks the kernel by scene size (LDS tables / global tables / wavefront pipeline) and, for
    a launch this small, the sample split on top: every choice is the reference-loop image."""
    data = rtm.make_stress_scene(n, seed=8)
    data.width, data.height, data.samples, data.superSamples = 56, 40, 8, 2
    ost, oarr, _ = _oracle_view(oracle, data)
    ref, cnt = oracle.render(ost, oarr, n, oracle.make_options(mode=1, max_bounces=8, seed=4, height=40))
    auto, st = _gpu_image(rtm, data, "repaired", 8, 4, want=("f64",), variant=0)
    plain, _ = _gpu_image(rtm, data, "repaired", 8, 4, want=("f64",), variant=1)
    assert np.array_equal(auto["f64"], ref) and np.array_equal(plain["f64"], ref)
    assert (st["casts"], st["draws"]) == (cnt["casts"], cnt["draws"])
    unl, st = _gpu_image(rtm, data, "repaired", -1, 4, want=("f64",), variant=0)
    ref_u, cnt_u = oracle.render(ost, oarr, n, oracle.make_options(mode=1, max_bounces=-1, seed=4, height=40))
    assert np.array_equal(unl["f64"], ref_u) and st["casts"] == cnt_u["casts"]


@pytest.mark.parametrize("n", [255, 256, 257])
def test_record_packing_boundary(rtm, oracle, n):
    """Hit ids and the identity index share a byte in the packed records: 255 spheres is the last scene
    that fits, 256 must take the LDS record stack, 257 four-byte records — all the same image (variant 0 takes the
    uniform grid at these sizes; the exhaustive kernels are asked for by name)."""
    data = rtm.make_stress_scene(n, seed=3)
    data.width, data.height, data.samples, data.superSamples = 48, 32, 4, 2
    # pull the camera close so that high-index spheres are hit, too
    ost, oarr, _ = _oracle_view(oracle, data)
    ref, cnt = oracle.render(ost, oarr, n, oracle.make_options(mode=1, max_bounces=8, seed=21, height=32))
    for v in (0, 1, 2, 9, 3, 14):
        out, stats = _gpu_image(rtm, data, "repaired", 8, 21, want=("f64",), variant=v)
        assert np.array_equal(out["f64"], ref), (n, v)
        assert stats["casts"] == cnt["casts"]
    assert ref.any()
    # any depth: records packed by position, deep levels in the pooled stack
    ref, cnt = oracle.render(ost, oarr, n, oracle.make_options(mode=1, max_bounces=-1, seed=21, height=32))
    for v in (0, 2, 9, 14, 3):
        out, stats = _gpu_image(rtm, data, "repaired", -1, 21, want=("f64",), variant=v)
        assert np.array_equal(out["f64"], ref), (n, v, "unlimited")
        assert stats["casts"] == cnt["casts"]


def test_random_configurations_vs_oracle(rtm, oracle):
    """Seeded fuzz over the knobs that select code paths — scene size (LDS tables / global tables / LDS
    record stack / wavefront pipeline), open and closed scenes, image shape, S and SS (powers of two or
    not), bounce cap (packed records / any depth), mode, row range and interleaved bands — every frame
    against the oracle, bit for bit, with its counters."""
    rng = np.random.default_rng(20261004)
    box = rtm.LoadData(oracle.scene_path("cornellBoxSetting.json")).data
    checked = 0
    for case in range(120):
        n = int(rng.choice([1, 3, 7, 8, 9, 20, 24, 25, 40, 90, 255, 256, 300, 511, 512, 700]))
        if case % 3 == 0:  # closed scene: the box's seven spheres + small ones inside
            objs = list(box.object)[: max(1, min(n, 7))]
            while len(objs) < n:
                objs.append(_mk(rtm, rng.uniform(-7, 7, 3), float(rng.uniform(0.3, 1.0)), rng.uniform(0.2, 0.9, 3), (0, 0, 0)))
            data = rtm.SettingData(width=8, height=8, samples=1, superSamples=1, camera=box.camera, object=objs)
        else:
            data = rtm.make_stress_scene(n, seed=int(rng.integers(1 << 30)))
        data.width, data.height = int(rng.integers(5, 70)), int(rng.integers(5, 50))
        data.samples, data.superSamples = int(rng.choice([1, 2, 3, 4, 7, 8, 16])), int(rng.choice([1, 2, 3]))
        mb = int(rng.choice([-1, 0, 1, 5, 8, 9, 15, 16, 40]))
        mode = "literal" if case % 7 == 6 else "repaired"
        seed = int(rng.integers(1 << 40))
        ost, oarr, _ = _oracle_view(oracle, data)
        m = oracle.MODE_LITERAL if mode == "literal" else oracle.MODE_REPAIRED
        ref, cnt = oracle.render(ost, oarr, n, oracle.make_options(mode=m, max_bounces=mb, seed=seed, height=data.height))
        out, st = _gpu_image(rtm, data, mode, mb, seed, want=("f64",))
        assert np.array_equal(out["f64"], ref, equal_nan=True), (case, n, data.width, data.height, data.samples, data.superSamples, mb, mode)
        assert (st["casts"], st["bounces"], st["draws"]) == (cnt["casts"], cnt["bounces"], cnt["draws"]), case
        # a row range dealt out in bands reassembles to the same rows
        lo, hi = sorted(int(v) for v in rng.integers(0, data.height + 1, 2))
        world = int(rng.integers(2, 5))
        if hi > lo:
            from raytracingmin_amd.distributed import band_row_index
            got = np.full_like(ref, np.nan)
            for rank in range(world):
                part, _ = rtm.Renderer(data, mode=mode, max_bounces=mb, seed=seed).render_rows(lo, hi, want=("f64",),
                                                                                            band=(world, rank))
                got[band_row_index(lo, hi, world, rank)] = part["f64"]
            assert np.array_equal(got[lo:hi], ref[lo:hi], equal_nan=True), (case, lo, hi, world)
        checked += 1
    assert checked == 120


def test_host_trig_makes_chaotic_scenes_bit_identical(rtm, oracle):
    """RTM_MODE_HOST_TRIG: sin/cos of the bounce (src/Renderer.cpp:93-94) exactly as the host libm returns
    them.  Closed boxes packed with small spheres amplify one-ulp differences ~10x per bounce, so without
    the flag deep samples diverge from the oracle there (a documented handful of the fuzzed cases); with
    it every frame is the oracle's, bit for bit, whatever the depth."""
    rng = np.random.default_rng(42)
    box = rtm.LoadData(oracle.scene_path("cornellBoxSetting.json")).data
    diverged_without = 0
    for case in range(24):
        n = int(rng.choice([64, 100, 254, 255, 257, 400, 513]))
        objs = list(box.object)
        while len(objs) < n:
            objs.append(_mk(rtm, rng.uniform(-7, 7, 3), float(rng.uniform(0.3, 1.0)), rng.uniform(0.2, 0.9, 3), (0, 0, 0)))
        data = rtm.SettingData(width=int(rng.integers(20, 90)), height=int(rng.integers(10, 50)),
                               samples=int(rng.choice([2, 4, 8, 16])), superSamples=int(rng.choice([1, 2, 3])),
                               camera=box.camera, object=objs)
        mb = int(rng.choice([-1, -1, 17, 40, 200]))
        seed = int(rng.integers(1 << 40))
        ost, oarr, _ = _oracle_view(oracle, data)
        ref, cnt = oracle.render(ost, oarr, n, oracle.make_options(mode=1, max_bounces=mb, seed=seed, height=data.height))
        exact, st = rtm.Renderer(data, mode="repaired", max_bounces=mb, seed=seed, host_trig=True).render_rows(want=("f64",))
        assert np.array_equal(exact["f64"], ref), (case, n, mb)
        assert (st["casts"], st["draws"]) == (cnt["casts"], cnt["draws"]), case
        plain, st = rtm.Renderer(data, mode="repaired", max_bounces=mb, seed=seed).render_rows(want=("f64",))
        diverged_without += int(st["casts"] != cnt["casts"] or not np.array_equal(plain["f64"], ref))
        assert float(np.max(np.abs(plain["f64"] - ref))) < 0.2  # a diverged sample moves a pixel by at most its share
    print(f"frames differing from the oracle without the flag: {diverged_without} of 24")


def test_device_sincos_with_host_trig_table_equals_host_libm(rtm, oracle):
    """The table behind RTM_MODE_HOST_TRIG, through the kernels' own code path (draws of a bounce from a
    random stream, the shading block's sincos, the correction): equal to the libm's sincos() on every
    one of 4 M random streams."""
    rng = np.random.default_rng(5)
    n = 1 << 22
    a = rng.integers(0, 1 << 32, n).astype(np.float64)
    b = rng.integers(0, 1 << 32, n).astype(np.float64)
    r1, s, c = _probe(rtm, 16, a, b), _probe(rtm, 17, a, b), _probe(rtm, 18, a, b)
    hs, hc = oracle.sin_cos(r1)
    assert np.array_equal(s.view(np.uint64), hs.view(np.uint64)) and np.array_equal(c.view(np.uint64), hc.view(np.uint64))
    assert len(np.unique(r1)) > 3_000_000  # a third of the 2^23 possible arguments


def test_scratch_buffers_are_reused_and_released(rtm, oracle):
    """The big work buffers (split terms, pooled record stacks, wavefront state) persist per device and
    stream between calls; rtm_release_scratch frees them and the next call simply allocates again."""
    import torch
    data = rtm.LoadData(oracle.scene_path("cornellBoxSetting.json")).data
    data.width, data.height, data.samples, data.superSamples = 128, 64, 8, 2
    r = rtm.Renderer(data, mode="repaired", max_bounces=-1, seed=2)
    first, _ = r.render_rows_device(want=("f64",))
    free0 = torch.cuda.mem_get_info()[0]
    again, _ = r.render_rows_device(want=("f64",))          # reuses the buffers: no new device memory
    assert torch.cuda.mem_get_info()[0] >= free0 - (8 << 20)
    assert rtm.lib().rtm_release_scratch(0) == 0
    assert torch.cuda.mem_get_info()[0] > free0
    third, _ = r.render_rows_device(want=("f64",))
    s2 = torch.cuda.Stream()
    with torch.cuda.stream(s2):                              # another stream gets its own buffers
        fourth, _ = r.render_rows_device(want=("f64",), stream=s2.cuda_stream)
    torch.cuda.synchronize()
    for other in (again, third, fourth):
        assert torch.equal(first["f64"], other["f64"])
    assert rtm.lib().rtm_release_scratch(-1) == 0
    # the host-trig table is dropped with the rest and rebuilt on demand
    exact, _ = rtm.Renderer(data, mode="repaired", max_bounces=-1, seed=2, host_trig=True).render_rows_device(want=("f64",))
    assert rtm.lib().rtm_release_scratch(0) == 0
    exact2, _ = rtm.Renderer(data, mode="repaired", max_bounces=-1, seed=2, host_trig=True).render_rows_device(want=("f64",))
    assert torch.equal(exact["f64"], exact2["f64"]) and torch.equal(exact["f64"], first["f64"])


def test_row_tiles_equal_full_image_and_seed_matters(rtm, oracle):
    data = rtm.LoadData(oracle.scene_path("cornellBoxSetting.json")).data
    data.width, data.height, data.samples, data.superSamples = 72, 40, 4, 2
    full, _ = _gpu_image(rtm, data, "repaired", 8, 7, want=("f64",))
    parts = [_gpu_image(rtm, data, "repaired", 8, 7, want=("f64",), rows=r)[0]["f64"]
             for r in ((0, 5), (5, 16), (16, 17), (17, 40))]
    assert np.array_equal(np.concatenate(parts), full["f64"])  # bit-for-bit: RNG keyed by global pixel
    again, _ = _gpu_image(rtm, data, "repaired", 8, 7, want=("f64",))
    assert np.array_equal(again["f64"], full["f64"])  # deterministic
    other, _ = _gpu_image(rtm, data, "repaired", 8, 8, want=("f64",))
    assert not np.array_equal(other["f64"], full["f64"])
    empty, st = _gpu_image(rtm, data, "repaired", 8, 7, want=("f64",), rows=(9, 9))
    assert empty["f64"].shape == (0, 72, 3) and st["samples"] == 0


def test_empty_scene_and_device_errors(rtm, oracle):
    data = rtm.SettingData(width=16, height=8, samples=2, superSamples=1)
    out, st = _gpu_image(rtm, data, "repaired", -1, 1, want=("f64",))
    assert not out["f64"].any() and st["casts"] == st["samples"] == 16 * 8 * 2
    r = rtm.Renderer(data, device=99)
    with pytest.raises(rtm.RtmError):
        r.render_rows()


def test_headline_config_strip_vs_oracle(rtm, oracle):
    """BASELINE configs[2] (1920x1080, 1024 spp, max 8 bounces) rendered in full on the GPU; nine
    full-width rows spread over the frame are checked against the oracle at the full 1024 spp (17.7 M
    samples), plus size-independent properties of the whole frame."""
    data = rtm.LoadData(oracle.scene_path("cornellBoxSetting.json")).data
    data.width, data.height, data.samples, data.superSamples = 1920, 1080, 64, 4
    r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=0x5EED)
    out, stats = r.render_rows_device(want=("f64", "f32"))
    img = out["f64"].cpu().numpy()
    assert stats["samples"] == 1920 * 1080 * 1024
    cps = stats["casts"] / stats["samples"]
    print(f"headline: kernel {stats['kernel_ms']:.1f} ms, {stats['samples'] / stats['kernel_ms'] * 1e-3:.1f} "
          f"Msamples/s, casts/sample {cps:.4f}")
    assert 4.0 < cps < 5.0  # SURVEY App. B.4 measured 4.24 on a square 256x256 frame; 16:9 sees more wall
    assert 3 * stats["bounces"] <= stats["draws"] <= stats["casts"] + 2 * stats["bounces"]
    assert np.isfinite(img).all() and img.min() >= 0.0
    st, arr, n = oracle.load_scene(oracle.scene_path("cornellBoxSetting.json"), width=1920, height=1080,
                                   samples=64, super_samples=4)
    for rows in ((0, 1), (134, 135), (269, 270), (404, 405), (539, 540), (674, 675), (809, 810), (944, 945),
                 (1079, 1080)):
        ref, _ = oracle.render(st, arr, n, oracle.make_options(mode=1, max_bounces=8, seed=0x5EED,
                                                              row_begin=rows[0], row_end=rows[1]))
        err = float(np.max(np.abs(img[rows[0]:rows[1]] - ref)))
        print(f"rows {rows}: max pixel delta vs oracle {err:.3e}")
        assert err <= PIXEL_TOL
    # strip re-render equals the same rows of the full frame, bit for bit
    strip, _ = r.render_rows_device(200, 208, want=("f64",))
    assert np.array_equal(strip["f64"].cpu().numpy(), img[200:208])
    # the literal per-sphere loop with the compiler's math (variant 1) agrees with the default kernel
    # on all 2.1e9 samples / 9.4e9 casts of the frame: same bits, same counters
    ref, ref_stats = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=0x5EED, variant=1) \
        .render_rows_device(want=("f64",))
    assert np.array_equal(ref["f64"].cpu().numpy().view(np.uint64), img.view(np.uint64))
    assert {k: ref_stats[k] for k in ("casts", "bounces", "draws")} == {k: stats[k] for k in ("casts", "bounces", "draws")}
    # what bench.py --gpus 8 runs per rank — interleaved 8-row bands, each a one-round launch that gets
    # the sample split — reassembles to the same frame, and the parts' counters add up
    from raytracingmin_amd.distributed import band_row_index
    got = np.empty_like(img)
    casts = 0
    for rank in range(8):
        part, st = r.render_rows_device(0, 1080, want=("f64",), band=(8, rank))
        got[band_row_index(0, 1080, 8, rank)] = part["f64"].cpu().numpy()
        casts += st["casts"]
    assert np.array_equal(got.view(np.uint64), img.view(np.uint64)) and casts == stats["casts"]
    # the device's own sin/cos (host_trig=False, the labelled faster row) change nothing here: the box's
    # wall spheres damp one-ulp differences instead of amplifying them
    dt, st = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=0x5EED, host_trig=False).render_rows_device(want=("f64",))
    assert np.array_equal(dt["f64"].cpu().numpy().view(np.uint64), img.view(np.uint64)) and st["casts"] == stats["casts"]


def test_mixed_whole_and_split_launch_vs_oracle(rtm, oracle):
    """A launch of more than 1 536 tiles keeps its first tiles whole and sample-splits the last 1 536 behind them in the
    same grid (csrc/rtm_kernels.hip choose_split; src/Renderer.cpp:240-248 fixes only the ORDER of the additions).
    400x328 = 2 050 tiles: 514 whole + 1 536 split, every bit and counter against the oracle, with a row range and an
    interleaved band part on top (their tile numbering differs from the full frame's)."""
    scene = oracle.scene_path("cornellBoxSetting.json")
    data = rtm.LoadData(scene).data
    W, H = 400, 328
    data.width, data.height, data.samples, data.superSamples = W, H, 8, 2
    r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=77)
    out, stats = r.render_rows_device(want=("f64",))
    assert stats["split"] > 1
    st, arr, n = oracle.load_scene(scene, width=W, height=H, samples=8, super_samples=2)
    ref, cnt = oracle.render(st, arr, n, oracle.make_options(mode=1, max_bounces=8, seed=77, height=H))
    img = out["f64"].cpu().numpy()
    assert np.array_equal(img.view(np.uint64), ref.view(np.uint64))
    assert {k: stats[k] for k in ("samples", "casts", "bounces", "draws")} == {k: cnt[k] for k in ("samples", "casts", "bounces", "draws")}
    part, _ = r.render_rows_device(16, 312, want=("f64",))  # 1 850 tiles: 314 whole + 1 536 split
    assert np.array_equal(part["f64"].cpu().numpy().view(np.uint64), ref[16:312].view(np.uint64))
    from raytracingmin_amd.distributed import band_row_index
    band, _ = rtm.Renderer(data, mode="repaired", max_bounces=-1, seed=77).render_rows_device(0, H, want=("f64",), band=(1, 0))
    ref_u, _ = oracle.render(st, arr, n, oracle.make_options(mode=1, max_bounces=-1, seed=77, height=H))
    assert np.array_equal(band["f64"].cpu().numpy().view(np.uint64), ref_u[band_row_index(0, H, 1, 0)].view(np.uint64))


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("max_bounces", [-1, 8])
def test_config2_full_frame_vs_oracle(rtm, oracle, max_bounces):
    """BASELINE configs[1]: Cornell box 512x512 @ 256 spp (SS 4 x S 16), the WHOLE L1 frame against the
    oracle — unlimited depth (the reference's own recursion) and the north_star's cap of 8: every bit of
    Renderer::image, the 8-bit view and the counters."""
    scene = oracle.scene_path("cornellBoxSetting.json")
    data = rtm.LoadData(scene).data
    data.width, data.height, data.samples, data.superSamples = 512, 512, 16, 4
    out, stats = rtm.Renderer(data, mode="repaired", max_bounces=max_bounces, seed=0x5EED) \
        .render_rows_device(want=("f64", "u8"))
    st, arr, n = oracle.load_scene(scene, width=512, height=512, samples=16, super_samples=4)
    ref, cnt = oracle.render(st, arr, n, oracle.make_options(mode=1, max_bounces=max_bounces, seed=0x5EED, height=512))
    assert _bits_equal(out["f64"].cpu().numpy(), ref)
    assert np.array_equal(out["u8"].cpu().numpy(), oracle.quantise(ref))
    assert {k: stats[k] for k in ("samples", "casts", "bounces", "draws")} == \
           {k: cnt[k] for k in ("samples", "casts", "bounces", "draws")}
    cps = stats["casts"] / stats["samples"]
    assert abs(cps - (4.95 if max_bounces < 0 else 4.24)) < 0.05  # SURVEY App. B.4, measured on the reference


def test_config4_band_parts_vs_oracle(rtm, oracle):
    """BASELINE configs[3]: Cornell box 3840x2160 @ 4096 spp (SS 4 x S 256), max 8 bounces, dealt out to
    eight ranks in interleaved 8-row bands exactly as bench.py --gpus 8 does (band=(8, r): one launch per
    rank).  Per part: two rows against the oracle at the full 4096 spp.  All parts:
    they reassemble to the frame one launch renders (bit for bit), counters add up."""
    from raytracingmin_amd.distributed import band_row_index
    scene = oracle.scene_path("cornellBoxSetting.json")
    W, H, S, SS = 3840, 2160, 256, 4
    data = rtm.LoadData(scene).data
    data.width, data.height, data.samples, data.superSamples = W, H, S, SS
    r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=0x5EED)
    st, arr, n = oracle.load_scene(scene, width=W, height=H, samples=S, super_samples=SS)
    frame = np.empty((H, W, 3), dtype=np.float64)
    total = dict(samples=0, casts=0, bounces=0, draws=0)
    worst_ms = 0.0
    for rank in range(8):
        part, ps = r.render_rows_device(0, H, want=("f64",), band=(8, rank))
        rows = band_row_index(0, H, 8, rank)
        assert part["f64"].shape == (len(rows), W, 3)
        # (only the last 1 536 of the part's 16 320 tiles are sample-split: 6.4 GB of terms; all of them would be 51 GB)
        frame[rows] = part["f64"].cpu().numpy()
        for k in total:
            total[k] += ps[k]
        worst_ms = max(worst_ms, ps["kernel_ms"])
        for y in (int(rows[3]), int(rows[len(rows) // 2 + 5])):  # two rows of this rank's share, full spp
            ref, _ = oracle.render(st, arr, n, oracle.make_options(mode=1, max_bounces=8, seed=0x5EED,
                                                                  row_begin=y, row_end=y + 1))
            assert _bits_equal(frame[y:y + 1], ref), (rank, y)
    print(f"configs[3]: slowest of the eight band parts {worst_ms:.1f} ms "
          f"({W * H * S * SS * SS / 8 / worst_ms * 1e-3:.0f} Msamples/s per GPU)")
    assert total["samples"] == W * H * S * SS * SS
    assert 3 * total["bounces"] <= total["draws"] <= total["casts"] + 2 * total["bounces"]
    assert np.isfinite(frame).all() and frame.min() >= 0.0
    whole, ws = r.render_rows_device(want=("f64",))  # one launch of 129 600 tiles: 3.4e10 samples
    assert {k: ws[k] for k in total} == total
    assert _bits_equal(whole["f64"].cpu().numpy(), frame)


def test_config5_full_frame_properties_and_spot_pixels(rtm, oracle):
    """BASELINE configs[4]: 100 000 random spheres, 1920x1080 @ 256 spp, max 8 bounces — the full frame as
    variant 0 renders it (the uniform-grid kernel, a quarter of a second; the exhaustive pipeline takes 24 s and is
    compared with it on a strip in tests/test_grid_gpu.py): finite, non-negative, counter identities, and
    64 pixels spread over the frame against the oracle at the full 256 spp, bit for bit."""
    data = rtm.make_stress_scene(n=100_000, seed=12345)
    W, H = 1920, 1080
    data.width, data.height, data.samples, data.superSamples = W, H, 256, 1
    out, stats = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=0x5EED).render_rows_device(want=("f64",))
    img = out["f64"].cpu().numpy()
    assert stats["samples"] == W * H * 256 and stats["variant"] == 17
    print(f"configs[4]: {stats['kernel_ms'] / 1e3:.1f} s, {stats['samples'] / stats['kernel_ms'] * 1e-3:.2f} Msamples/s, "
          f"{stats['casts'] / stats['samples']:.3f} casts/sample")
    assert np.isfinite(img).all() and img.min() >= 0.0 and img.max() > 0.0
    assert stats["samples"] <= stats["casts"] <= 9 * stats["samples"]
    assert 3 * stats["bounces"] <= stats["draws"] <= stats["casts"] + 2 * stats["bounces"]
    assert stats["casts"] == stats["samples"] + stats["bounces"]  # every cast is a primary or follows a bounce
    rng = np.random.default_rng(5)
    xy = np.stack([rng.integers(0, W, 64), rng.integers(0, H, 64)], axis=1).astype(np.int32)
    ost, oarr, n = _oracle_view(oracle, data)
    ref, _ = oracle.render_pixels(ost, oarr, n, oracle.make_options(mode=1, max_bounces=8, seed=0x5EED, height=H), xy)
    assert _bits_equal(img[xy[:, 1], xy[:, 0]], ref)


def test_async_renders_only_enqueue(rtm, oracle):
    """rtm_render_scene with stats == NULL returns once the work is queued: no allocation that
    synchronises, no upload, no wait (include/rtm.h).  Eight frames are queued in a fraction of the time
    the GPU needs for them, on a stream the host then finds still busy."""
    import time
    import torch
    data = rtm.LoadData(oracle.scene_path("cornellBoxSetting.json")).data
    data.width, data.height, data.samples, data.superSamples = 960, 544, 16, 4
    r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=3)
    first, _ = r.render_rows_device(want=("f32",), stats=True)  # warm: scene upload, trig table, buffers
    outs = [torch.empty_like(first["f32"]) for _ in range(8)]
    torch.cuda.synchronize()
    import ctypes as C
    st, opt = data.settings_c(), r._options(0, data.height)
    stream = torch.cuda.current_stream().cuda_stream
    t0 = time.perf_counter()
    for o in outs:
        rtm._lib.check(rtm.lib().rtm_render_scene(C.byref(st), r._scene_handle(), C.byref(opt), None,
                                                  C.c_void_p(o.data_ptr()), None, C.c_void_p(stream), None), "render")
    t_enqueue = time.perf_counter() - t0
    busy = not torch.cuda.current_stream().query()
    torch.cuda.synchronize()
    t_total = time.perf_counter() - t0
    print(f"8 frames queued in {t_enqueue * 1e3:.2f} ms, finished after {t_total * 1e3:.1f} ms")
    assert busy and t_enqueue < 0.2 * t_total
    for o in outs:
        assert torch.equal(o, first["f32"])
    r.stream_status()  # nothing overflowed


def test_async_overflow_is_reported(rtm):
    """A render WITHOUT rtm_stats cannot fail at return time, but its truncation is not silent: the stream's
    sticky flag is reported by rtm_stream_status, or by the next render on the stream, once; with
    rtm_stats the call itself fails (test_record_overflow_fails_loudly)."""
    import torch
    data = _white_room(rtm, 0.99995, w=8, h=8, s=1)
    data.object[1].m_material.color = rtm.vec3(0.99995, 0.99995, 0.99995)  # nothing ends a path
    r = rtm.Renderer(data, mode="repaired", max_bounces=-1, seed=1)
    r.render_rows_device(want=("f64",), stats=False)            # returns: only enqueued
    with pytest.raises(rtm.RtmError) as e:
        r.stream_status()
    assert e.value.status == -8 and "deeper" in str(e.value)
    r.stream_status()                                            # reported once, then clear
    r.render_rows_device(want=("f64",), stats=False)
    torch.cuda.synchronize()                                     # the flag has reached the host ...
    with pytest.raises(rtm.RtmError) as e:
        r.render_rows_device(want=("f64",), stats=False)         # ... so the next call reports it
    assert e.value.status == -8
    ok = _white_room(rtm, 0.5, w=8, h=8, s=1)
    rtm.Renderer(ok, mode="repaired", max_bounces=-1, seed=1).render_rows_device(want=("f64",), stats=False)
    r.stream_status()


def test_two_host_threads_share_a_stream(rtm, oracle):
    """Threading contract of include/rtm.h: two host threads rendering on the same (device, stream) —
    here the null stream, through the blocking rtm_render — take turns inside the library; each gets its
    own frame, bit for bit, although both need the stream's record pool and split buffers (growing them
    under a concurrent call was a use-after-free before the per-stream context)."""
    import threading
    scene = oracle.scene_path("cornellBoxSetting.json")
    jobs = [(64, 40, 4, 2, -1, 21), (200, 120, 8, 2, -1, 22)]  # unlimited depth: both use the pooled stacks
    want = []
    for w, h, s, ss, mb, seed in jobs:
        st, arr, n = oracle.load_scene(scene, width=w, height=h, samples=s, super_samples=ss)
        want.append(oracle.render(st, arr, n, oracle.make_options(mode=1, max_bounces=mb, seed=seed, height=h))[0])
    got, errors = [[None] * 6 for _ in jobs], []

    def work(j):
        try:
            w, h, s, ss, mb, seed = jobs[j]
            data = rtm.LoadData(scene).data
            data.width, data.height, data.samples, data.superSamples = w, h, s, ss
            r = rtm.Renderer(data, mode="repaired", max_bounces=mb, seed=seed)
            for k in range(6):
                got[j][k] = r.render_rows(want=("f64",))[0]["f64"]
                if k == 2:
                    rtm.lib().rtm_release_scratch(0)  # frees the buffers under the other thread's feet — safely
        except Exception as exc:  # noqa: BLE001
            errors.append(exc)

    threads = [threading.Thread(target=work, args=(j,)) for j in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(300)
    assert not errors, errors
    for j in range(len(jobs)):
        for k in range(6):
            assert _bits_equal(got[j][k], want[j]), (j, k)


def test_primary_hit_reuse_row_is_bit_identical_and_rejects_what_it_does_not_serve(rtm, oracle):
    """Variant 15 — the labelled row that computes a sub-pixel's primary hit once for its S samples — gives the
    oracle's image and counters (a reused primary hit still counts as the cast the reference performs), on a
    frame with many samples per sub-pixel and on one with S = 1 (nothing to reuse); unlimited depth and big
    scenes are refused, not silently served by another kernel."""
    scene = oracle.scene_path("cornellBoxSetting.json")
    for (w, h, s, ss, mb) in ((160, 96, 32, 2, 8), (64, 40, 1, 3, 5), (40, 24, 7, 1, 0)):
        data = rtm.LoadData(scene).data
        data.width, data.height, data.samples, data.superSamples = w, h, s, ss
        out, st = _gpu_image(rtm, data, "repaired", mb, 77, want=("f64",), variant=15)
        ost, oarr, n = oracle.load_scene(scene, width=w, height=h, samples=s, super_samples=ss)
        ref, cnt = oracle.render(ost, oarr, n, oracle.make_options(mode=1, max_bounces=mb, seed=77, height=h))
        assert _bits_equal(out["f64"], ref)
        assert {k: st[k] for k in ("samples", "casts", "bounces", "draws")} == \
               {k: cnt[k] for k in ("samples", "casts", "bounces", "draws")}
        assert st["variant"] == 15
    data = rtm.LoadData(scene).data
    data.width, data.height, data.samples, data.superSamples = 32, 16, 2, 1
    with pytest.raises(rtm.RtmError) as e:
        _gpu_image(rtm, data, "repaired", -1, 1, want=("f64",), variant=15)
    assert e.value.status == -8


# ---- png::PlaneObject: a build-defined completion, oracle and device bit for bit -----------
def _oracle_objects(oracle, data):
    arr, n = data.objects_c()
    return (oracle.Object * max(n, 1)).from_buffer_copy(bytes(arr)), n


@pytest.mark.parametrize("mode", ["literal", "repaired"])
def test_plane_intersect_batch_bit_exact(rtm, oracle, mode):
    """Object::Intersect seam for planes and spheres mixed: 4 096 (ray, object) pairs — rays aimed inside,
    at the rim of and past the square, grazing and from behind — against the oracle, hit / t / normal."""
    rng = np.random.default_rng(31)
    n = 4096
    objs = (rtm._lib.rtm_object * n)()
    org = rng.uniform(-6, 6, (n, 3))
    tgt = np.empty((n, 3))
    for i in range(n):
        o = objs[i]
        plane = i % 4 != 3
        o.type = 2 if plane else 1
        pos = rng.uniform(-4, 4, 3)
        for k in range(3):
            o.position[k] = pos[k]
            o.up[k] = rng.normal()
            o.target[k] = pos[k] + rng.normal()
        o.width = float(rng.uniform(0.5, 6.0))
        o.size = np.float32(rng.uniform(0.3, 3.0))
        # aim: inside (u in [-0.5, 0.5] widths), at the rim (|u| ~ 0.5), outside, or anywhere
        kind = i % 5
        spread = (0.45, 0.5, 0.7, 0.5000001, 3.0)[kind] * (o.width if plane else 2 * o.size)
        tgt[i] = pos + rng.uniform(-1, 1, 3) * spread
    d = tgt - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[::97] *= -1.0  # some rays point away
    m = {"literal": 0, "repaired": 1}[mode]
    hit, t, nrm = rtm.intersect_objects_batch(objs, org, d, mode=mode)
    oo = (oracle.Object * n).from_buffer_copy(bytes(objs))
    hits = 0
    for i in range(n):
        h, tt, nn = oracle.intersect_object(oo[i], org[i], d[i], m)
        assert (h, tt) == (int(hit[i]), float(t[i])), i
        assert np.array_equal(np.array(nn).view(np.uint64), nrm[i].view(np.uint64)), i
        hits += h
    assert 0.2 * n < hits < 0.8 * n


@pytest.mark.parametrize("max_bounces", [8, -1, 12, 0])
def test_plane_room_render_vs_oracle(rtm, oracle, max_bounces):
    """scenes/planeRoom.json — six PlaneObject walls, a square lamp, two spheres — loaded by LoadData (objectType 2):
    the DEFAULT kernel (the chunked LDS-table kernel with the plane test in the object chunk, packed records for a
    cap of up to 8 bounces and by position beyond), its sample-split form and the per-object loop with the compiler's
    math all give the oracle's image and counters, bit for bit; kernels that know spheres only refuse the scene."""
    path = oracle.scene_path("planeRoom.json")
    data = rtm.LoadData(path).data
    assert sum(isinstance(o, rtm.PlaneObject) for o in data.object) == 6 and len(data.object) == 8
    data.width, data.height, data.samples, data.superSamples = 96, 60, 4, 2
    oobj, n = _oracle_objects(oracle, data)
    ost = oracle.Settings.from_buffer_copy(bytes(data.settings_c()))
    ref, cnt = oracle.render_objects(ost, oobj, n, oracle.make_options(mode=1, max_bounces=max_bounces, seed=9, height=60))
    lref, lcnt = oracle.render_objects(ost, oobj, n, oracle.make_options(mode=0, max_bounces=max_bounces, seed=9, height=60))
    keys = ("samples", "casts", "bounces", "draws")
    for variant, resolved in ((0, 2), (2, 2), (9, 2), (1, 1)):
        out, st = _gpu_image(rtm, data, "repaired", max_bounces, 9, want=("f64", "u8"), variant=variant)
        assert _bits_equal(out["f64"], ref) and np.array_equal(out["u8"], oracle.quantise(ref)), variant
        assert {k: st[k] for k in keys} == {k: cnt[k] for k in keys}, variant
        assert st["variant"] == resolved
        lit, lst = _gpu_image(rtm, data, "literal", max_bounces, 9, want=("f64",), variant=variant)
        assert _bits_equal(lit["f64"], lref) and lst["casts"] == lcnt["casts"], variant
    assert ref.max() > 0.5 and (max_bounces == 0 or cnt["bounces"] > cnt["samples"])  # lit, and paths do bounce
    for variant in (3, 12, 14, 15, 16):
        with pytest.raises(rtm.RtmError) as e:
            _gpu_image(rtm, data, "repaired", max_bounces, 9, want=("f64",), variant=variant)
        assert e.value.status == -8


def test_planes_and_spheres_mixed_scenes_vs_oracle(rtm, oracle):
    """Planes anywhere in the object list — first, last, between spheres, tilted (no zero component in the normal) and
    axis-aligned (exact zeros: the shading block's zero-tolerant math), coincident with a sphere's hit distance (the
    lowest index wins across types), 1 to 40 objects (chunks of four plus every tail size) — default kernel and
    per-object loop against the oracle, image and counters."""
    rng = np.random.default_rng(5)
    cam = rtm.Camera(rtm.vec3(0, 0, -12), rtm.vec3(0, 0, 0), rtm.vec3(0, 1, 0), 1.2)
    M = rtm.Material
    for n_obj in (1, 2, 3, 4, 5, 6, 7, 9, 13, 24, 25, 40):
        objs = []
        for k in range(n_obj):
            col = rtm.vec3(*map(float, rng.uniform(0.2, 0.9, 3)))
            em = rtm.vec3(3.0, 3.0, 3.0) if k % 5 == 0 else rtm.vec3(0, 0, 0)
            kind = rng.integers(4) if n_obj > 1 else 1
            pos = rtm.vec3(*map(float, rng.uniform(-5, 5, 3)))
            if kind == 0:
                objs.append(rtm.SphereObject(pos, float(rng.uniform(0.5, 2.5)), M(col, em)))
            elif kind == 1:  # axis-aligned plane facing the origin side
                axis = int(rng.integers(3))
                tgt = [pos.x, pos.y, pos.z]
                tgt[axis] += 1.0 if tgt[axis] < 0 else -1.0
                up = rtm.vec3(0, 0, 1) if axis == 1 else rtm.vec3(0, 1, 0)
                objs.append(rtm.PlaneObject(pos, up, rtm.vec3(*tgt), float(rng.uniform(2, 9)), M(col, em)))
            elif kind == 2:  # tilted plane
                objs.append(rtm.PlaneObject(pos, rtm.vec3(0.1, 1, 0.2), rtm.vec3(*map(float, rng.uniform(-1, 1, 3))),
                                            float(rng.uniform(2, 9)), M(col, em)))
            else:  # a sphere and, right behind it in the list, a plane through its front pole: an exact tie on the axis
                objs.append(rtm.SphereObject(rtm.vec3(0, 0, 2), 2.0, M(col, em)))
                objs.append(rtm.PlaneObject(rtm.vec3(0, 0, 0), rtm.vec3(0, 1, 0), rtm.vec3(0, 0, -1), 3.0, M(col, em)))
        objs = objs[:max(n_obj, 1)]
        objs.append(rtm.SphereObject(rtm.vec3(0, 0, 0), 30.0, M(rtm.vec3(0.7, 0.7, 0.7), rtm.vec3(0.4, 0.4, 0.4))))  # the room
        data = rtm.SettingData(width=48, height=32, samples=3, superSamples=2, camera=cam, object=objs)
        if not data.has_planes():
            continue
        oobj, n = _oracle_objects(oracle, data)
        ost = oracle.Settings.from_buffer_copy(bytes(data.settings_c()))
        for mb in (8, -1):
            ref, cnt = oracle.render_objects(ost, oobj, n, oracle.make_options(mode=1, max_bounces=mb, seed=31, height=32))
            for variant in (0, 1):
                out, st = _gpu_image(rtm, data, "repaired", mb, 31, want=("f64",), variant=variant)
                assert _bits_equal(out["f64"], ref), (n_obj, mb, variant)
                assert (st["casts"], st["bounces"], st["draws"]) == (cnt["casts"], cnt["bounces"], cnt["draws"]), (n_obj, mb, variant)
                assert st["variant"] == (2 if variant == 0 else 1)


def test_fp32_row_statistics(rtm, oracle):
    """Variant 16, the labelled single-precision fast row: NOT parity — float arithmetic, hardware sqrt / sin / cos,
    forward throughput.  What is asserted is what such a row must still be: the same estimator (means agree to
    noise level, nearly the same number of casts), with the fraction of pixels outside the north_star tolerance
    REPORTED, not hidden; and that it refuses what it does not serve."""
    scene = oracle.scene_path("cornellBoxSetting.json")
    w, h, s, ss, mb = 256, 256, 16, 2, 8
    data = rtm.LoadData(scene).data
    data.width, data.height, data.samples, data.superSamples = w, h, s, ss
    fast, fst = _gpu_image(rtm, data, "repaired", mb, 0x5EED, want=("f64", "f32"), variant=16)
    st, arr, n = oracle.load_scene(scene, width=w, height=h, samples=s, super_samples=ss)
    ref, cnt = oracle.render(st, arr, n, oracle.make_options(mode=1, max_bounces=mb, seed=0x5EED, height=h))
    d = fast["f64"] - ref
    out_of_tol = float(np.mean(np.max(np.abs(d), axis=2) > NORTH_STAR_TOL))
    print(f"fp32 row, Cornell {w}x{h}x{s * ss * ss}spp: {100 * out_of_tol:.1f} % of the pixels differ from the fp64 image by "
          f"more than {NORTH_STAR_TOL}; max |delta| {np.abs(d).max():.3e}, mean |delta| {np.abs(d).mean():.3e}, "
          f"mean delta {d.mean():+.3e}; casts {fst['casts']} vs {cnt['casts']}; kernel {fst['kernel_ms']:.2f} ms")
    assert fst["variant"] == 16 and fst["samples"] == cnt["samples"]
    assert np.isfinite(fast["f64"]).all() and fast["f64"].min() >= 0.0
    assert abs(fst["casts"] - cnt["casts"]) <= 0.005 * cnt["casts"]        # the same paths but for a few grazing rays
    assert np.abs(d).mean() < 0.01 and abs(d.mean()) < 1e-3               # same estimator: differences are zero-mean noise
    assert np.array_equal(fast["f32"], fast["f64"].astype(np.float32))
    with pytest.raises(rtm.RtmError) as e:                                 # literal semantics are an fp64 affair
        _gpu_image(rtm, data, "literal", mb, 1, want=("f64",), variant=16)
    assert e.value.status == -8


def test_scene_entry_points_agree(rtm, oracle):
    """The ways a scene reaches the kernels give the same frame: an rtm_scene made from a host array, one made from
    a DEVICE-resident array (flattened by a kernel), rtm_render_device with a host array (content-addressed cache,
    first call and a cached call), with a device array (stream-ordered temporaries), and the blocking rtm_render.
    Ten different scenes in a row push the first ones out of the 8-entry cache and every frame is still right."""
    import torch
    L = rtm.lib()
    scene = oracle.scene_path("cornellBoxSetting.json")
    data = rtm.LoadData(scene).data
    data.width, data.height, data.samples, data.superSamples = 72, 40, 4, 2
    st = data.settings_c()
    arr, n = data.spheres_c()
    ost, oarr, on = oracle.load_scene(scene, width=72, height=40, samples=4, super_samples=2)
    ref, _ = oracle.render(ost, oarr, on, oracle.make_options(mode=1, max_bounces=8, seed=3, height=40))
    opt = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=3)._options(0, 40)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_arr = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()  # the rtm_sphere array in device memory

    def frame(call):
        out = torch.empty((40, 72, 3), dtype=torch.float64, device="cuda")
        stats = rtm._lib.rtm_stats()
        rtm._lib.check(call(C.c_void_p(out.data_ptr()), C.byref(stats)), "render")
        return out.cpu().numpy()

    h_host, h_dev = C.c_void_p(), C.c_void_p()
    rtm._lib.check(L.rtm_scene_create(arr, n, 0, 0, C.byref(h_host)), "rtm_scene_create")
    rtm._lib.check(L.rtm_scene_create(C.c_void_p(d_arr.data_ptr()), n, 1, 0, C.byref(h_dev)), "rtm_scene_create(device)")
    assert L.rtm_scene_size(h_host) == n == L.rtm_scene_size(h_dev)
    frames = [
        frame(lambda o, s: L.rtm_render_scene(C.byref(st), h_host, C.byref(opt), o, None, None, stream, s)),
        frame(lambda o, s: L.rtm_render_scene(C.byref(st), h_dev, C.byref(opt), o, None, None, stream, s)),
        frame(lambda o, s: L.rtm_render_device(C.byref(st), arr, n, 0, C.byref(opt), o, None, None, stream, s)),
        frame(lambda o, s: L.rtm_render_device(C.byref(st), arr, n, 0, C.byref(opt), o, None, None, stream, s)),
        frame(lambda o, s: L.rtm_render_device(C.byref(st), C.c_void_p(d_arr.data_ptr()), n, 1, C.byref(opt), o, None, None,
                                               stream, s)),
    ]
    for f in frames:
        assert _bits_equal(f, ref)
    assert L.rtm_scene_destroy(h_host) == 0 and L.rtm_scene_destroy(h_dev) == 0 and L.rtm_scene_destroy(None) == 0
    # ten different scenes through the array entry point: more than the cache holds
    host = np.zeros((40, 72, 3), dtype=np.float64)
    for k in range(10):
        data.object[0].m_size = 5.0 + 0.25 * k
        arr_k, n_k = data.spheres_c()
        oarr_k = (oracle.Sphere * n_k).from_buffer_copy(bytes(arr_k))
        want, _ = oracle.render(ost, oarr_k, n_k, oracle.make_options(mode=1, max_bounces=8, seed=3, height=40))
        rtm._lib.check(L.rtm_render(C.byref(st), arr_k, n_k, C.byref(opt), host.ctypes.data, None, None, None), "rtm_render")
        assert _bits_equal(host, want), k
    rtm._lib.check(L.rtm_render(C.byref(st), arr, n, C.byref(opt), host.ctypes.data, None, None, None), "rtm_render")  # evicted, re-uploaded
    assert _bits_equal(host, ref)


def test_renders_on_two_streams_from_two_threads(rtm, oracle):
    """Different (device, stream) pairs share nothing: two host threads, each with its own stream, scene handle and
    frame size, render concurrently; every frame equals the oracle's."""
    import threading
    import torch
    scene = oracle.scene_path("cornellBoxSetting.json")
    jobs = [(96, 56, 4, 2, 8, 31), (64, 80, 8, 1, -1, 32)]
    want = []
    for w, h, s, ss, mb, seed in jobs:
        st, arr, n = oracle.load_scene(scene, width=w, height=h, samples=s, super_samples=ss)
        want.append(oracle.render(st, arr, n, oracle.make_options(mode=1, max_bounces=mb, seed=seed, height=h))[0])
    got, errors = [[] for _ in jobs], []
    streams = [torch.cuda.Stream() for _ in jobs]

    def work(j):
        try:
            w, h, s, ss, mb, seed = jobs[j]
            data = rtm.LoadData(scene).data
            data.width, data.height, data.samples, data.superSamples = w, h, s, ss
            r = rtm.Renderer(data, mode="repaired", max_bounces=mb, seed=seed)
            with torch.cuda.stream(streams[j]):
                for _ in range(5):
                    out, _ = r.render_rows_device(want=("f64",), stats=False, stream=streams[j].cuda_stream)
                    got[j].append(out["f64"])
                streams[j].synchronize()
                r.stream_status(streams[j].cuda_stream)
        except Exception as exc:  # noqa: BLE001
            errors.append(exc)

    threads = [threading.Thread(target=work, args=(j,)) for j in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(300)
    assert not errors, errors
    for j in range(len(jobs)):
        assert len(got[j]) == 5
        for f in got[j]:
            assert _bits_equal(f.cpu().numpy(), want[j]), j


def test_renderer_reads_the_live_scene(rtm, oracle):
    """png::Renderer holds a reference to the caller's SettingData and reads it at render time (src/Renderer.h:16).
    The mirror keeps an uploaded copy, so it must notice every way the scene can change between two calls: a field
    written in place, an entry replaced by one of another type at the same index, entries reordered — on the
    device-resident entry point and on the host one alike."""
    data = rtm.LoadData(oracle.scene_path("cornellBoxSetting.json")).data
    data.width, data.height, data.samples, data.superSamples = 64, 40, 2, 2
    r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=11)

    def both():
        dev, _ = r.render_rows_device(want=("f64",))
        host, _ = r.render_rows(want=("f64",))
        fresh, _ = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=11).render_rows_device(want=("f64",))
        dev, fresh = dev["f64"].cpu().numpy(), fresh["f64"].cpu().numpy()
        assert _bits_equal(dev, host["f64"]) and _bits_equal(dev, fresh)
        oobj, n = _oracle_objects(oracle, data)
        ost = oracle.Settings.from_buffer_copy(bytes(data.settings_c()))
        ref, _ = oracle.render_objects(ost, oobj, n, oracle.make_options(mode=1, max_bounces=8, seed=11, height=40))
        assert _bits_equal(dev, ref)
        return dev

    a = both()
    handle = r._scene.value
    assert _bits_equal(both(), a) and r._scene.value == handle       # nothing changed: the uploaded scene is reused
    data.object[0].m_position.y = 8.5                                 # in place, two levels down
    data.object[1].m_material.color.x = 0.3
    b = both()
    assert not _bits_equal(a, b)
    data.object[0].m_size = 3.0                                       # in place, a scalar field
    c = both()
    assert not _bits_equal(b, c)
    data.object[0] = rtm.PlaneObject(rtm.vec3(0, 7, 0), rtm.vec3(0, 0, 1), rtm.vec3(0, 0, 0), 6.0,
                                     rtm.Material(rtm.vec3(0, 0, 0), rtm.vec3(5, 5, 5)))  # another type, same index
    d = both()
    assert not _bits_equal(c, d)
    data.object[1], data.object[2] = data.object[2], data.object[1]  # reorder: same objects, nothing written
    both()


def test_retired_variants_are_refused_by_name(rtm, oracle):
    """Variants retired from the product (profiles/r3/retired_variants.patch) keep their numbers, say so in their
    names, and are refused — never silently served by another kernel."""
    data = rtm.LoadData(oracle.scene_path("cornellBoxSetting.json")).data
    data.width, data.height, data.samples, data.superSamples = 16, 16, 1, 1
    retired = [v for v in range(rtm.lib().rtm_num_variants()) if rtm.lib().rtm_variant_name(v).startswith(b"retired")]
    assert retired == [4, 5, 6, 8, 10, 11, 13]
    for v in retired:
        with pytest.raises(rtm.RtmError) as e:
            _gpu_image(rtm, data, "repaired", 8, 1, want=("f64",), variant=v)
        assert e.value.status == -8 and "retired" in str(e.value)
    for v in (rtm.lib().rtm_num_variants(), -1):  # no such number: an invalid argument, not an unsupported request
        with pytest.raises(rtm.RtmError) as e:
            _gpu_image(rtm, data, "repaired", 8, 1, want=("f64",), variant=v)
        assert e.value.status == -1
    assert b"profiles/r3/retired_variants.patch" in rtm.lib().rtm_variant_name(13)


def test_scene_destroy_and_stream_release_do_not_wait_for_other_work(rtm, oracle):
    """include/rtm.h: rtm_scene_destroy never waits — a scene whose renders are still running is parked and freed by a
    later call — and never for other streams; rtm_stream_release waits for ITS stream only and forgets the pair."""
    import time
    import torch
    L = rtm.lib()
    scene = oracle.scene_path("cornellBoxSetting.json")
    big = rtm.LoadData(scene).data
    big.width, big.height, big.samples, big.superSamples = 1920, 1080, 16, 4   # ~45 ms of GPU time per frame
    small = rtm.LoadData(scene).data
    small.width, small.height, small.samples, small.superSamples = 64, 40, 2, 2
    ost, oarr, on = oracle.load_scene(scene, width=64, height=40, samples=2, super_samples=2)
    ref, _ = oracle.render(ost, oarr, on, oracle.make_options(mode=1, max_bounces=8, seed=3, height=40))
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    rbig = rtm.Renderer(big, mode="repaired", max_bounces=8, seed=3)
    rsmall = rtm.Renderer(small, mode="repaired", max_bounces=8, seed=3)
    rbig.render_rows_device(want=("f32",), stats=False, stream=sa.cuda_stream)      # warm both contexts
    out_small, _ = rsmall.render_rows_device(want=("f64",), stats=False, stream=sb.cuda_stream)
    torch.cuda.synchronize()
    # (1) a finished scene on stream B is destroyed while stream A is busy for ~0.5 s: no wait for A
    for _ in range(12):
        rbig.render_rows_device(want=("f32",), stats=False, stream=sa.cuda_stream)
    out_small, _ = rsmall.render_rows_device(want=("f64",), stats=False, stream=sb.cuda_stream)
    sb.synchronize()
    t0 = time.perf_counter()
    rsmall.invalidate()                                       # rtm_scene_destroy
    t_destroy_idle = time.perf_counter() - t0
    busy_after = not sa.query()
    # (2) the scene of the renders that are still running: parked, the call returns at once, the frames stay right
    frames = [rbig.render_rows_device(want=("f32",), stats=False, stream=sa.cuda_stream)[0]["f32"] for _ in range(2)]
    t0 = time.perf_counter()
    rbig.invalidate()
    t_destroy_busy = time.perf_counter() - t0
    still_busy = not sa.query()
    sa.synchronize()
    print(f"destroy of an idle scene with another stream busy: {t_destroy_idle * 1e3:.2f} ms; of a scene in use: "
          f"{t_destroy_busy * 1e3:.2f} ms (stream busy after: {busy_after}, {still_busy})")
    assert busy_after and still_busy, "the box was too fast for this test's timing: nothing was in flight"
    assert t_destroy_idle < 0.05 and t_destroy_busy < 0.05
    assert _bits_equal(out_small["f64"].cpu().numpy(), ref)
    assert torch.equal(frames[0], frames[1])
    check, _ = rtm.Renderer(big, mode="repaired", max_bounces=8, seed=3).render_rows_device(want=("f32",))
    assert torch.equal(frames[0], check["f32"])
    # (3) rtm_stream_release: waits for its own stream, then the pair is unknown again (a second release is a no-op)
    rsmall.render_rows_device(want=("f64",), stats=False, stream=sb.cuda_stream)
    assert L.rtm_stream_release(0, C.c_void_p(sb.cuda_stream)) == 0 and sb.query()
    assert L.rtm_stream_release(0, C.c_void_p(sb.cuda_stream)) == 0
    out2, _ = rsmall.render_rows_device(want=("f64",), stats=True, stream=sb.cuda_stream)   # a fresh context is made
    assert _bits_equal(out2["f64"].cpu().numpy(), ref)


def test_large_scene_render_only_enqueues(rtm, oracle):
    """include/rtm.h: with a depth cap whose trip budget (spp x (max_bounces + 1)) is short enough, a render through the
    exhaustive large-scene pipeline (variant 12: two launches per trip) only ENQUEUES, like every other kernel: the call returns
    while the stream is still busy, a second frame queued behind it is the same frame, and both are the frame of the
    blocking call (which follows the device's count instead) and of the oracle on spot pixels."""
    import time
    import torch
    data = rtm.make_stress_scene(n=100_000, seed=12345)
    data.width, data.height, data.samples, data.superSamples = 256, 144, 8, 1
    r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=77, variant=12)
    blocking, st = r.render_rows_device(want=("f64",), stats=True)            # also warms scene + buffers
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a, _ = r.render_rows_device(want=("f64",), stats=False)
    b, _ = r.render_rows_device(want=("f64",), stats=False)
    t_enqueue = time.perf_counter() - t0
    busy = not torch.cuda.current_stream().query()
    torch.cuda.synchronize()
    t_total = time.perf_counter() - t0
    r.stream_status()
    print(f"two 100k-sphere frames: enqueued in {t_enqueue * 1e3:.1f} ms, finished after {t_total * 1e3:.1f} ms "
          f"(one blocking frame: {st['kernel_ms']:.1f} ms of kernels)")
    assert busy and t_enqueue < 0.5 * t_total
    assert torch.equal(a["f64"], blocking["f64"]) and torch.equal(b["f64"], blocking["f64"])
    ost, oarr, n = _oracle_view(oracle, data)
    rng = np.random.default_rng(3)
    px = np.stack([rng.integers(0, 256, 12), rng.integers(0, 144, 12)], axis=1)
    ref, _ = oracle.render_pixels(ost, oarr, n, oracle.make_options(mode=1, max_bounces=8, seed=77, height=144), px)
    got = a["f64"].cpu().numpy()
    for k, (x, y) in enumerate(px):
        assert _bits_equal(got[y, x], ref[k]), (x, y)
    # unlimited depth: no budget can be known, the call follows the count (blocks) — and is still the oracle's frame
    ru = rtm.Renderer(data, mode="repaired", max_bounces=-1, seed=77, variant=12)
    u, _ = ru.render_rows_device(0, 16, want=("f64",), stats=False)
    refu, _ = oracle.render_pixels(ost, oarr, n, oracle.make_options(mode=1, max_bounces=-1, seed=77, height=144),
                                   np.array([[5, 3], [200, 9]]))
    gu = u["f64"].cpu().numpy()
    assert _bits_equal(gu[3, 5], refu[0]) and _bits_equal(gu[9, 200], refu[1])
