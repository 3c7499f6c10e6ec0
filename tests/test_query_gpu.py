"""Ray queries on a scene (include/rtm.h: rtm_scene_nearest, rtm_scene_occluded): for rays of the caller's, the hit object,
distance and normal of the reference's loop over ALL objects (src/Renderer.cpp:58-73), and "is there a hit before tmax" —
bit for bit and for every ray, through the chunked loop of small scenes, the uniform grid, the grid with planes and the
occlusion walk's early exit.  References: the oracle's Intersect in that loop, and the loop's validated GPU restatement
(rtm_debug_wf_nearest kind 1) where the scene is large."""
import ctypes as C

import numpy as np
import pytest

import _query_rays as qr

pytestmark = pytest.mark.gpu

UNSUPPORTED = -8


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd
    return raytracingmin_amd


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream_ptr(stream):
    import torch
    return C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)


def _nearest(rtm, scene, o, d, stream=None):
    """rtm_scene_nearest on device copies of (o, d): (object, t, normal) as numpy arrays."""
    import torch
    n = len(o)
    with torch.cuda.stream(stream):
        to, td = _dev(o), _dev(d)
        obj = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        t = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
        nrm = torch.full((n, 3), -7.0, dtype=torch.float64, device="cuda")
    bufs = rtm._lib.rtm_hit_buffers()
    bufs.object, bufs.t, bufs.normal = obj.data_ptr(), t.data_ptr(), nrm.data_ptr()
    rtm._lib.check(rtm.lib().rtm_scene_nearest(scene, C.c_void_p(to.data_ptr()), C.c_void_p(td.data_ptr()), n, C.byref(bufs),
                                               _stream_ptr(stream)), "rtm_scene_nearest")
    torch.cuda.synchronize()
    return obj.cpu().numpy(), t.cpu().numpy(), nrm.cpu().numpy()


def _occluded(rtm, scene, to, td, tmax):
    """rtm_scene_occluded on DEVICE rays; tmax: a numpy array or None."""
    import torch
    n = to.shape[0]
    tm = _dev(tmax) if tmax is not None else None
    out = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    rtm._lib.check(rtm.lib().rtm_scene_occluded(scene, C.c_void_p(to.data_ptr()), C.c_void_p(td.data_ptr()),
                                                C.c_void_p(tm.data_ptr()) if tm is not None else None, n,
                                                C.c_void_p(out.data_ptr()), _stream_ptr(None)), "rtm_scene_occluded")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _hook(rtm, scene, any_hit, to, td, tmax):
    """rtm_debug_scene_query: (status, object, t, occluded, tests, steps)."""
    import torch
    n = to.shape[0]
    tm = _dev(tmax) if tmax is not None else None
    obj = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    t = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    occ = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    tests = torch.zeros((n,), dtype=torch.int32, device="cuda")
    steps = torch.zeros((n,), dtype=torch.int32, device="cuda")
    rc = rtm.lib().rtm_debug_scene_query(scene, any_hit, C.c_void_p(to.data_ptr()), C.c_void_p(td.data_ptr()),
                                         C.c_void_p(tm.data_ptr()) if tm is not None else None, n, C.c_void_p(obj.data_ptr()),
                                         C.c_void_p(t.data_ptr()), C.c_void_p(occ.data_ptr()), C.c_void_p(tests.data_ptr()),
                                         C.c_void_p(steps.data_ptr()), _stream_ptr(None))
    torch.cuda.synchronize()
    return rc, obj.cpu().numpy(), t.cpu().numpy(), occ.cpu().numpy(), tests.cpu().numpy().astype(np.int64), steps.cpu().numpy().astype(np.int64)


def _has_grid(rtm, scene):
    one = _dev(np.array([[0.0, 0.0, -60.0]])), _dev(np.array([[0.0, 0.0, 1.0]]))
    rc = _hook(rtm, scene, 0, one[0], one[1], None)[0]
    assert rc in (0, UNSUPPORTED), rc
    return rc == 0


def _wf_reference(rtm, arr, n, o, d):
    """The reference loop on the GPU (rtm_debug_wf_nearest kind 1) in rtm_scene_nearest's terms: a miss is (-1, +inf)."""
    ids = np.zeros(len(o), dtype=np.int32)
    t = np.zeros(len(o), dtype=np.float64)
    rtm._lib.check(rtm.lib().rtm_debug_wf_nearest(1, arr, n, o.ctypes.data, d.ctypes.data, len(o), ids.ctypes.data, t.ctypes.data),
                   "reference loop")
    return ids, np.where(ids < 0, np.inf, t)


def _spheres(rtm, centers, radii):
    n = len(radii)
    arr = (rtm._lib.rtm_sphere * n)()
    for i in range(n):
        for k in range(3):
            arr[i].center[k] = float(centers[i, k])
            arr[i].color[k] = 0.5
        arr[i].radius = float(radii[i])
    return arr


def _plane_scene(rtm, n_spheres, seed):
    """A room of six png::PlaneObject walls around `n_spheres` random spheres, the planes anywhere in the vector."""
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
        data.object.insert(int(rng.integers(0, len(data.object) + 1)),
                           rtm.SphereObject(rtm.vec3(*c), float(rng.uniform(0.3, 1.2)), rtm.Material(grey, rtm.vec3(0, 0, 0))))
    return data


class Case:
    """A scene handle, its rays and the reference's answers for them; made once, shared, never changed."""
    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.fixture(scope="module")
def cases(rtm, oracle):
    L = rtm.lib()
    out, keep = {}, []
    rng = np.random.default_rng(181)

    def handle(arr, n, objects=False):
        h = C.c_void_p()
        if objects:
            rtm._lib.check(L.rtm_scene_create_objects(arr, n, 0, C.byref(h)), "rtm_scene_create_objects")
        else:
            rtm._lib.check(L.rtm_scene_create(arr, n, 0, 0, C.byref(h)), "rtm_scene_create")
        keep.append(h)
        return h

    # 1. small scenes, the chunked search: the oracle's loop, normals included
    _, oarr, n = oracle.load_scene(oracle.scene_path("cornellBoxSetting.json"))
    arr = (rtm._lib.rtm_sphere * n).from_buffer_copy(bytes(oarr)[:80 * n])
    o, d = qr.query_rays(rng, *qr.aim_points(oarr, n, False), 2048, 12.0)
    out["cornell"] = Case(scene=handle(arr, n), o=o, d=d, grid=False, ref=qr.oracle_nearest(oracle, oarr, n, o, d), arr=arr, n=n)
    data = rtm.LoadData(oracle.scene_path("planeRoom.json")).data
    arr, n = data.objects_c()
    oarr = (oracle.Object * n).from_buffer_copy(bytes(arr))
    o, d = qr.query_rays(rng, *qr.aim_points(oarr, n, True), 2048, 6.0)
    out["planeRoom"] = Case(scene=handle(arr, n, True), o=o, d=d, grid=False, ref=qr.oracle_nearest(oracle, oarr, n, o, d, True))
    # 2. grid scenes: the reference loop's GPU restatement
    n = 400
    _, arr, _ = rtm.make_stress_scene(n, seed=1000 + n).to_c()
    oarr = (oracle.Sphere * n).from_buffer_copy(bytes(arr))
    o, d = qr.query_rays(rng, *qr.aim_points(oarr, n, False), 20_000, 50.0)
    out["stress400"] = Case(scene=handle(arr, n), o=o, d=d, grid=True, ref=_wf_reference(rtm, arr, n, o, d) + (None,), arr=arr, n=n,
                            oarr=oarr)
    n = 3000  # small spheres + walls of radius 1e4 around them + zero-radius spheres + duplicates + concentric shells
    c = rng.uniform(-20, 20, (n, 3))
    r = rng.uniform(0.1, 1.5, n)
    c[:6] = [[0, 0, 1e4 + 25], [0, 0, -1e4 - 25], [1e4 + 25, 0, 0], [-1e4 - 25, 0, 0], [0, 1e4 + 25, 0], [0, -1e4 - 25, 0]]
    r[:6] = 1e4
    r[6:30] = 0.0
    c[1000:1100] = c[900:1000]
    r[1000:1100] = r[900:1000]
    c[1100:1150] = c[850:900]
    arr = _spheres(rtm, c, r)
    o, d = qr.query_rays(rng, c, np.maximum(r, 1e-3), 20_000, 25.0)
    out["walls+zero+duplicates"] = Case(scene=handle(arr, n), o=o, d=d, grid=True, ref=_wf_reference(rtm, arr, n, o, d) + (None,))
    # 3. grid with planes: the oracle's loop
    data = _plane_scene(rtm, 300, seed=307)
    arr, n = data.objects_c()
    oarr = (oracle.Object * n).from_buffer_copy(bytes(arr))
    o, d = qr.query_rays(rng, *qr.aim_points(oarr, n, True), 502, 20.0)  # 512 rays with the special ones
    out["planes300"] = Case(scene=handle(arr, n, True), o=o, d=d, grid=True, ref=qr.oracle_nearest(oracle, oarr, n, o, d, True))
    yield out
    for h in keep:
        assert L.rtm_scene_destroy(h) == 0


def _assert_nearest(case, got, label):
    obj, t, nrm = got
    ref_id, ref_t, ref_n = case.ref
    bad = np.flatnonzero((obj != ref_id) | (t.view(np.uint64) != ref_t.view(np.uint64)))
    assert bad.size == 0, (label, bad[:5], obj[bad[:5]], ref_id[bad[:5]], t[bad[:5]], ref_t[bad[:5]], case.o[bad[:5]], case.d[bad[:5]])
    miss = ref_id < 0
    assert np.array_equal(nrm[miss].view(np.uint64), np.zeros((int(miss.sum()), 3), dtype=np.uint64)), label  # +0, not -0
    if ref_n is not None:
        badn = np.flatnonzero((nrm.view(np.uint64) != ref_n.view(np.uint64)).any(axis=1))
        assert badn.size == 0, (label, badn[:5], nrm[badn[:5]], ref_n[badn[:5]])


@pytest.mark.parametrize("name", ["cornell", "planeRoom"])
def test_small_scenes_answer_as_the_oracles_loop(rtm, cases, name):
    """The chunked search over SceneGlobal / SceneGlobalObjects: object, t and normal of every ray; a miss is -1, +inf and
    zeros; 1, 63, 64 and 65 rays (one lane, a wave but one, a wave, a wave and one) give prefixes of the same answers."""
    case = cases[name]
    assert _has_grid(rtm, case.scene) is False
    ref_id = case.ref[0]
    assert 0.3 < (ref_id >= 0).mean() < 1.0 and (ref_id < 0).sum() >= 8
    if name == "planeRoom":
        assert (ref_id < 6).any() and (ref_id >= 6).any()  # planes and spheres both win
    got = _nearest(rtm, case.scene, case.o, case.d)
    _assert_nearest(case, got, name)
    for k in (1, 63, 64, 65):
        part = _nearest(rtm, case.scene, case.o[:k], case.d[:k])
        for a, b in zip(part, got):
            assert np.array_equal(a.view(np.uint64 if a.dtype == np.float64 else a.dtype),
                                  b[:k].view(np.uint64 if b.dtype == np.float64 else b.dtype)), (name, k)


def test_grid_scenes_answer_as_the_reference_loop(rtm, oracle, cases):
    """The uniform grid: the smallest stress scene that gets one, and a scene it does not like (walls that every ray tests,
    zero radii, exact duplicates whose ties go to the lower index); every ray, the exhaustive fallback's (every 97th
    direction is off unit length) and the non-finite ones included; the oracle's Intersect on 200 hits; and the same bits from
    a scene that rtm_scene_create_device built, queried on another stream."""
    import torch
    rng = np.random.default_rng(182)
    for name in ("stress400", "walls+zero+duplicates"):
        case = cases[name]
        assert _has_grid(rtm, case.scene) is True
        got = _nearest(rtm, case.scene, case.o, case.d)
        _assert_nearest(case, got, name)
        assert (case.ref[0] >= 0).mean() > 0.15
    ref_id = cases["walls+zero+duplicates"].ref[0]
    assert not np.isin(ref_id, np.arange(1000, 1100)).any() and np.isin(ref_id, np.arange(900, 1000)).any()
    case = cases["stress400"]
    obj, t, nrm = _nearest(rtm, case.scene, case.o, case.d)
    unit = np.ones(len(case.o), dtype=bool)
    unit[:20_000:97] = False
    unit[20_000:] = False
    for k in rng.choice(np.flatnonzero((obj >= 0) & unit), 200, replace=False):
        h, tt, nn = oracle.intersect(case.oarr[int(obj[k])], case.o[k], case.d[k], oracle.MODE_REPAIRED)
        assert h and tt == t[k] and qr.same_bits(np.array(nn), nrm[k]), k
    packed = torch.frombuffer(bytearray(bytes(case.arr)), dtype=torch.uint8).reshape(case.n, 80).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    h = C.c_void_p()
    rtm._lib.check(rtm.lib().rtm_scene_create_device(C.c_void_p(packed.data_ptr()), case.n, 0, C.c_void_p(side.cuda_stream),
                                                     C.byref(h)), "rtm_scene_create_device")
    try:
        assert _has_grid(rtm, h) is True
        dev = _nearest(rtm, h, case.o, case.d, stream=side)
        assert np.array_equal(dev[0], obj) and qr.same_bits(dev[1], t) and qr.same_bits(dev[2], nrm)
    finally:
        assert rtm.lib().rtm_scene_destroy(h) == 0


def test_grid_with_planes_answers_as_the_oracles_loop(rtm, cases):
    """Six planes among the objects every ray tests, 300 spheres in the grid: object, t and normal of 512 rays."""
    case = cases["planes300"]
    assert len(case.o) == 512 and _has_grid(rtm, case.scene) is True
    got = _nearest(rtm, case.scene, case.o, case.d)
    _assert_nearest(case, got, "planes300")
    ref_id = case.ref[0]
    assert (ref_id >= 0).mean() > 0.3 and (ref_id < 0).any()


@pytest.mark.parametrize("name", ["cornell", "planeRoom", "stress400", "walls+zero+duplicates", "planes300"])
def test_occluded_is_nearest_t_below_tmax(rtm, cases, name):
    """out = ref_t < tmax for every ray and every family of tmax: none (any hit), the hit's own t (strict: 0), the next double
    (1 on hits), half of it, 0, -1, NaN and +inf; a mix of them, so that a wave holds decided and undecided lanes."""
    case = cases[name]
    ref_t = case.ref[1]
    n = len(ref_t)
    to, td = _dev(case.o), _dev(case.d)
    mix = np.select([np.arange(n) % 5 == k for k in range(4)], [ref_t, 0.5 * ref_t, np.full(n, np.nan), np.full(n, 0.0)],
                    np.nextafter(ref_t, np.inf))
    families = {"null": None, "ref_t": ref_t, "nextafter": np.nextafter(ref_t, np.inf), "half": 0.5 * ref_t, "zero": np.zeros(n),
                "minus one": np.full(n, -1.0), "nan": np.full(n, np.nan), "inf": np.full(n, np.inf), "mix": mix}
    for label, tmax in families.items():
        with np.errstate(invalid="ignore"):
            want = (ref_t < (np.inf if tmax is None else tmax)).astype(np.uint8)
        got = _occluded(rtm, case.scene, to, td, tmax)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (name, label, bad[:5], got[bad[:5]], want[bad[:5]], ref_t[bad[:5]], case.o[bad[:5]], case.d[bad[:5]])
    hits = np.isfinite(ref_t)
    assert _occluded(rtm, case.scene, to, td, families["nextafter"])[hits].all() and not _occluded(rtm, case.scene, to, td, ref_t).any()


def test_occlusion_walk_stops_early(rtm, oracle):
    """rtm_debug_scene_query counts sphere tests and cell steps per ray.  Camera-like and bounce-like rays that hit, in a
    20 000-sphere scene: the occlusion walk tests no more spheres than the nearest walk on either set, fewer on the
    camera-like one (it stops at the first hit; the nearest walk goes on to that hit's cell), and with a short tmax it
    takes fewer cell steps (it stops at the first cell whose exit lies beyond tmax).  The hook's answers are the calls'."""
    n = 20_000
    _, arr, _ = rtm.make_stress_scene(n, seed=1000 + n).to_c()
    oarr = (oracle.Sphere * n).from_buffer_copy(bytes(arr))
    c, r = qr.aim_points(oarr, n, False)
    h = C.c_void_p()
    rtm._lib.check(rtm.lib().rtm_scene_create(arr, n, 0, 0, C.byref(h)), "rtm_scene_create")
    try:
        rng = np.random.default_rng(185)
        box = 50.0
        for label, kind in (("camera-like", 0), ("bounce-like", 1)):
            o, d = qr.ray_mix(rng, c, r, 8192, box, kinds=[kind])
            obj, t, _ = _nearest(rtm, h, o, d)
            hit = obj >= 0
            assert hit.sum() > 2000, label
            o, d, obj, t = np.ascontiguousarray(o[hit]), np.ascontiguousarray(d[hit]), obj[hit], t[hit]
            to, td = _dev(o), _dev(d)
            rc, n_obj, n_t, n_occ, n_tests, n_steps = _hook(rtm, h, 0, to, td, None)
            assert rc == 0 and np.array_equal(n_obj, obj) and qr.same_bits(n_t, t) and n_occ.all()
            rc, a_obj, a_t, a_occ, a_tests, a_steps = _hook(rtm, h, 1, to, td, None)
            assert rc == 0 and np.array_equal(a_occ, _occluded(rtm, h, to, td, None)) and a_occ.all()
            assert (a_obj >= 0).all() and (a_t >= t).all()  # some hit, never nearer than the nearest
            short = np.full(len(o), 1e-3 * box)
            rc, _, _, s_occ, s_tests, s_steps = _hook(rtm, h, 1, to, td, short)
            assert rc == 0 and np.array_equal(s_occ, _occluded(rtm, h, to, td, short)) and np.array_equal(s_occ, (t < short).astype(np.uint8))
            print(f"{label}: {len(o)} rays; sphere tests per ray nearest {n_tests.mean():.1f}, any hit {a_tests.mean():.1f} "
                  f"(x{a_tests.sum() / n_tests.sum():.3f}); cell steps per ray nearest {n_steps.mean():.2f}, any hit "
                  f"{a_steps.mean():.2f}, tmax = {short[0]:g}: {s_steps.mean():.2f} (x{s_steps.sum() / max(n_steps.sum(), 1):.3f})")
            assert a_tests.sum() <= n_tests.sum(), label
            if kind == 0:
                assert a_tests.sum() < n_tests.sum()
            assert s_steps.sum() < n_steps.sum(), label
    finally:
        assert rtm.lib().rtm_scene_destroy(h) == 0


def test_python_surface(rtm, oracle, cases):
    """Renderer.nearest / Renderer.occluded: shapes, dtypes, the `want` subsets, the ValueError cases, the device scene of
    set_device_spheres; outputs are read only after torch.cuda.synchronize()."""
    import torch
    case = cases["cornell"]
    data = rtm.LoadData(oracle.scene_path("cornellBoxSetting.json")).data
    r = rtm.Renderer(data)
    to, td = _dev(case.o), _dev(case.d)
    n = len(case.o)
    out = r.nearest(to, td)
    assert sorted(out) == ["object", "t"]
    full = r.nearest(to, td, want=("object", "t", "normal"))
    only_n = r.nearest(to, td, want=("normal",))
    occ = r.occluded(to, td)
    half = r.occluded(to, td, tmax=_dev(0.5 * case.ref[1]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    on_side = r.nearest(to, td, stream=side)
    torch.cuda.synchronize()
    assert full["object"].shape == (n,) and full["object"].dtype == torch.int32 and full["object"].is_cuda
    assert full["t"].shape == (n,) and full["t"].dtype == torch.float64
    assert full["normal"].shape == (n, 3) and full["normal"].dtype == torch.float64
    assert occ.shape == (n,) and occ.dtype == torch.bool and sorted(only_n) == ["normal"]
    ref_id, ref_t, ref_n = case.ref
    for got in (out, full, on_side):
        assert np.array_equal(got["object"].cpu().numpy(), ref_id) and qr.same_bits(got["t"].cpu().numpy(), ref_t)
    assert qr.same_bits(full["normal"].cpu().numpy(), ref_n) and qr.same_bits(only_n["normal"].cpu().numpy(), ref_n)
    assert np.array_equal(occ.cpu().numpy(), ref_id >= 0) and not half.any()
    empty = r.nearest(to[:0], td[:0], want=("object", "normal"))
    assert empty["object"].shape == (0,) and empty["normal"].shape == (0, 3) and r.occluded(to[:0], td[:0]).shape == (0,)
    bad = [lambda: r.nearest(to.float(), td), lambda: r.nearest(to, td.cpu()), lambda: r.nearest(to[:, :2], td),
           lambda: r.nearest(to, td[:-1]), lambda: r.nearest(to.t().contiguous().t(), td), lambda: r.nearest(to.reshape(-1), td),
           lambda: r.nearest(case.o, td), lambda: r.nearest(to, td, want=("depth",)), lambda: r.nearest(to, td, want=()),
           lambda: r.occluded(to, td, tmax=_dev(np.zeros(n - 1))), lambda: r.occluded(to, td, tmax=_dev(np.zeros((n, 1)))),
           lambda: r.occluded(to, td, tmax=_dev(np.zeros(n, dtype=np.float32))), lambda: r.occluded(to, td.int())]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    # a query issued right after set_device_spheres answers for the device scene
    big = cases["stress400"]
    packed = torch.frombuffer(bytearray(bytes(big.arr)), dtype=torch.uint8).reshape(big.n, 80).cuda()
    r.set_device_spheres(packed)
    bo, bd = _dev(big.o), _dev(big.d)
    got = r.nearest(bo, bd)
    occ = r.occluded(bo, bd)
    torch.cuda.synchronize()
    assert np.array_equal(got["object"].cpu().numpy(), big.ref[0]) and qr.same_bits(got["t"].cpu().numpy(), big.ref[1])
    assert np.array_equal(occ.cpu().numpy(), big.ref[0] >= 0)
    r.set_device_spheres(None)
    back = r.nearest(to, td)
    torch.cuda.synchronize()
    assert np.array_equal(back["object"].cpu().numpy(), ref_id)
