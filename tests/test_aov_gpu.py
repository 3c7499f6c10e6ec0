"""First-hit feature buffers on a real MI355X (-m gpu): rtm_render_aov's depth, normal, albedo and object planes equal, bit
for bit, the planes built from the oracle's own pieces — rtmo_primary_dir, then rtmo_intersect / rtmo_intersect_object
over every object with strict <, > 0 and the lowest index first, the orienting normal, the raw colour, and the reductions
in float64 in loop order (sx outer, sy inner) cast to float32."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DBL_MAX = np.finfo(np.float64).max


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    n = C.c_int()
    m._lib.check(m.lib().rtm_device_count(C.byref(n)), "rtm_device_count")
    assert n.value >= 1
    return m


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.view(np.uint32) if a.dtype in (np.float32, np.int32) else a


def _aov(r, **kw):
    import torch
    out = r.render_aov(**kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _first_hit(isect, n, org, d, mode):
    """src/Renderer.cpp:58-73 through the oracle's Intersect: (object, dis, normal)."""
    dis, hit, nrm = DBL_MAX, -1, (0.0, 0.0, 0.0)
    t = C.c_double()
    for i in range(n):
        nb = (C.c_double * 3)(0.0, 0.0, 0.0)  # tmp_normal = vec3()
        if isect(i, org, d, mode, C.byref(t), nb) and t.value < dis and t.value > 0:
            dis, hit, nrm = t.value, i, (nb[0], nb[1], nb[2])
    return hit, dis, nrm


def _expected(oracle, st, isect, colors, n, mode, pixels):
    """The four planes of the listed pixels [(x, y), ...] from the oracle."""
    L = oracle.lib()
    SS = st.super_samples
    c = (SS + 1) // 2
    org = (C.c_double * 3)(*st.camera.origin)
    dbuf = (C.c_double * 3)()
    depth = np.empty(len(pixels), np.float32)
    obj = np.empty(len(pixels), np.int32)
    normal = np.empty((len(pixels), 3), np.float32)
    albedo = np.empty((len(pixels), 3), np.float32)
    for p, (x, y) in enumerate(pixels):
        ns, al = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
        for sx in range(1, SS + 1):
            for sy in range(1, SS + 1):
                L.rtmo_primary_dir(C.byref(st), x, y, sx, sy, dbuf)
                d = (dbuf[0], dbuf[1], dbuf[2])
                hit, dis, nrm = _first_hit(isect, n, org, dbuf, mode)
                if sx == c and sy == c:
                    depth[p] = np.float32(dis) if hit >= 0 else np.float32(np.inf)
                    obj[p] = hit
                if hit < 0:
                    continue
                dot = nrm[0] * d[0] + nrm[1] * d[1] + nrm[2] * d[2]
                w = nrm if dot < 0.0 else tuple(v * -1.0 for v in nrm)
                for k in range(3):
                    ns[k] = ns[k] + w[k]
                    al[k] = al[k] + colors[hit][k]
        div = float(SS * SS)
        normal[p] = [np.float32(v / div) for v in ns]
        albedo[p] = [np.float32(v / div) for v in al]
    return {"depth": depth, "object": obj, "normal": normal, "albedo": albedo}


def _sphere_isect(oracle, arr):
    L = oracle.lib()
    return lambda i, org, d, mode, t, nb: L.rtmo_intersect(C.byref(arr[i]), org, d, mode, t, nb)


def _cornell(rtm, oracle, w, h, ss, literal=False):
    data = rtm.LoadData(oracle.scene_path("cornellBoxSetting.json"), literal_loader=literal).data
    data.width, data.height, data.samples, data.superSamples = w, h, 1, ss
    st, arr, n = oracle.load_scene(oracle.scene_path("cornellBoxSetting.json"), literal_loader=literal, width=w, height=h,
                                   samples=1, super_samples=ss)
    return data, st, arr, n


def _check_frame(got, want, pixels, W):
    idx = np.array([y * W + x for x, y in pixels])
    for k in ("depth", "object", "normal", "albedo"):
        g = got[k].reshape(-1, 3) if k in ("normal", "albedo") else got[k].reshape(-1)
        assert np.array_equal(_bits(g[idx]), _bits(want[k])), k


@pytest.mark.parametrize("ss", [1, 2, 3, 4])
def test_cornell_repaired_matches_the_oracle(rtm, oracle, ss):
    w, h = 96, 56
    data, st, arr, n = _cornell(rtm, oracle, w, h, ss)
    got = _aov(rtm.Renderer(data, mode="repaired"))
    assert got["depth"].shape == (h, w) and got["normal"].shape == (h, w, 3) and got["object"].dtype == np.int32
    pixels = [(x, y) for y in range(h) for x in range(w)]
    want = _expected(oracle, st, _sphere_isect(oracle, arr), [arr[i].color for i in range(n)], n, 1, pixels)
    _check_frame(got, want, pixels, w)
    assert (got["object"] >= 0).all()  # the Cornell box is closed: every primary ray hits
    assert np.isfinite(got["depth"]).all()


def test_cornell_literal_normal_is_positive_zero(rtm, oracle):
    w, h, ss = 96, 56, 2
    data, st, arr, n = _cornell(rtm, oracle, w, h, ss, literal=True)
    got = _aov(rtm.Renderer(data, mode="literal"))
    assert (got["normal"].view(np.uint32) == 0).all()  # +0 bits, not -0
    pixels = [(x, y) for y in range(h) for x in range(w)]
    want = _expected(oracle, st, _sphere_isect(oracle, arr), [arr[i].color for i in range(n)], n, 0, pixels)
    _check_frame(got, want, pixels, w)


def test_plane_room_matches_the_oracle(rtm, oracle):
    from raytracingmin_amd import _lib
    L = _lib.lib()
    path = oracle.scene_path("planeRoom.json").encode()
    st = _lib.rtm_settings()
    cnt = C.c_size_t()
    _lib.check(L.rtm_scene_load_json_objects(path, 0, C.byref(st), None, 0, C.byref(cnt)), "load")
    objs = (_lib.rtm_object * cnt.value)()
    _lib.check(L.rtm_scene_load_json_objects(path, 0, C.byref(st), objs, cnt.value, C.byref(cnt)), "load")
    n = cnt.value
    assert any(o.type == _lib.OBJECT_SPHERE for o in objs) and any(o.type == 2 for o in objs)
    w, h, ss = 80, 50, 2
    st.width, st.height, st.samples, st.super_samples = w, h, 1, ss
    data = rtm.LoadData(oracle.scene_path("planeRoom.json")).data
    data.width, data.height, data.samples, data.superSamples = w, h, 1, ss
    assert data.has_planes()
    ost = oracle.Settings.from_buffer_copy(st)
    oobjs = (oracle.Object * n).from_buffer_copy(objs)
    OL = oracle.lib()
    isect = lambda i, org, d, mode, t, nb: OL.rtmo_intersect_object(C.byref(oobjs[i]), org, d, mode, t, nb)
    pixels = [(x, y) for y in range(h) for x in range(w)]
    want = _expected(oracle, ost, isect, [oobjs[i].color for i in range(n)], n, 1, pixels)
    for variant in (0, 1):
        got = _aov(rtm.Renderer(data, mode="repaired", variant=variant))
        _check_frame(got, want, pixels, w)
    hits = set(np.unique(got["object"]).tolist())
    assert any(objs[i].type == 2 for i in hits if i >= 0)  # some pixel's centre ray ends on a plane


def test_stress_grid_equals_exhaustive_and_the_oracle(rtm, oracle):
    data = rtm.make_stress_scene(n=20_000, seed=7)
    w, h = 48, 32
    data.width, data.height, data.samples, data.superSamples = w, h, 1, 2
    grid = _aov(rtm.Renderer(data, mode="repaired", variant=0))
    forced = _aov(rtm.Renderer(data, mode="repaired", variant=17))
    loop = _aov(rtm.Renderer(data, mode="repaired", variant=1))
    for k in grid:
        assert np.array_equal(_bits(grid[k]), _bits(loop[k])), k
        assert np.array_equal(_bits(forced[k]), _bits(loop[k])), k
    assert (grid["object"] >= 0).mean() > 0.2  # the frame sees spheres, not only the background
    data.superSamples = 1
    one = _aov(rtm.Renderer(data, mode="repaired", variant=0))
    st, arr, n = data.to_c()
    ost = oracle.Settings.from_buffer_copy(st)
    oarr = (oracle.Sphere * n).from_buffer_copy(arr)
    rng = np.random.default_rng(3)
    pixels = [(int(x), int(y)) for x, y in zip(rng.integers(0, w, 32), rng.integers(0, h, 32))]
    want = _expected(oracle, ost, _sphere_isect(oracle, oarr), [oarr[i].color for i in range(n)], n, 1, pixels)
    _check_frame(one, want, pixels, w)


def test_variant_17_needs_a_grid_and_other_variants_are_refused(rtm, oracle):
    from raytracingmin_amd import RtmError
    data, *_ = _cornell(rtm, oracle, 32, 16, 1)
    for v in (17, 2, 3, 12, 18):
        with pytest.raises(RtmError) as e:
            rtm.Renderer(data, mode="repaired", variant=v).render_aov()
        assert e.value.status == -8, v


@pytest.mark.parametrize("rows,band", [((0, 56), None), ((5, 43), None), ((0, 56), (3, 0)), ((0, 56), (3, 1)),
                                       ((0, 56), (3, 2)), ((3, 50), (3, 2))])
def test_rows_and_bands_are_the_full_frame_rows(rtm, oracle, rows, band):
    data, *_ = _cornell(rtm, oracle, 70, 56, 3)
    r = rtm.Renderer(data, mode="repaired")
    full = _aov(r)
    part = _aov(r, row_begin=rows[0], row_end=rows[1], band=band)
    if band is None:
        sel = list(range(rows[0], rows[1]))
    else:
        sel = [y for y in range(rows[0], rows[1]) if ((y - rows[0]) // 8) % band[0] == band[1]]
    for k in full:
        assert part[k].shape[0] == len(sel)
        assert np.array_equal(_bits(part[k]), _bits(full[k][sel])), k


def test_null_planes_are_left_untouched(rtm, oracle):
    import torch
    from raytracingmin_amd import _lib
    data, *_ = _cornell(rtm, oracle, 40, 24, 2)
    r = rtm.Renderer(data, mode="repaired")
    full = _aov(r)
    sentinel = torch.full((24, 40, 3), -7.25, dtype=torch.float32, device="cuda")
    depth = torch.full((24, 40), -1.0, dtype=torch.float32, device="cuda")
    bufs = _lib.rtm_aov_buffers()
    bufs.depth = depth.data_ptr()  # normal, albedo and object stay null
    opt = r._options(0, 24)
    st = data.settings_c()
    _lib.check(_lib.lib().rtm_render_aov(C.byref(st), r._scene_handle(), C.byref(opt), C.byref(bufs), None), "aov")
    torch.cuda.synchronize()
    assert (sentinel == -7.25).all()
    assert np.array_equal(_bits(depth.cpu().numpy()), _bits(full["depth"]))
    only = _aov(r, want=("object",))
    assert set(only) == {"object"} and np.array_equal(only["object"], full["object"])


def test_async_on_a_side_stream_with_the_scene_destroyed_at_once(rtm, oracle):
    import torch
    from raytracingmin_amd import _lib
    data, *_ = _cornell(rtm, oracle, 96, 56, 3)
    want = _aov(rtm.Renderer(data, mode="repaired"))
    L = _lib.lib()
    st, arr, n = data.to_c()
    scene = C.c_void_p()
    _lib.check(L.rtm_scene_create(arr, n, 0, 0, C.byref(scene)), "rtm_scene_create")
    s = torch.cuda.Stream()
    out = {k: torch.full(v.shape, 3.0, dtype=torch.float32 if v.dtype == np.float32 else torch.int32, device="cuda")
           for k, v in want.items()}
    bufs = _lib.rtm_aov_buffers(*(out[k].data_ptr() for k in ("depth", "normal", "albedo", "object")))
    torch.cuda.synchronize()
    opt = _lib.rtm_options()
    opt.mode, opt.row_begin, opt.row_end = 1, 0, data.height
    # a long render first on the same stream, so that the AOV kernel is still queued when the scene goes
    big = rtm.Renderer(rtm.LoadData(oracle.scene_path("cornellBoxSetting.json")).data, mode="repaired", max_bounces=8)
    big.data.width, big.data.height, big.data.samples, big.data.superSamples = 256, 256, 64, 2
    big.render_rows_device(want=("f32",), stats=False, stream=s.cuda_stream)
    _lib.check(L.rtm_render_aov(C.byref(st), scene, C.byref(opt), C.byref(bufs), C.c_void_p(s.cuda_stream)), "aov")
    _lib.check(L.rtm_scene_destroy(scene), "rtm_scene_destroy")
    s.synchronize()
    for k in want:
        assert np.array_equal(_bits(out[k].cpu().numpy()), _bits(want[k])), k


def test_render_writes_the_aov_files_and_keeps_the_image(rtm, oracle, tmp_path):
    data, *_ = _cornell(rtm, oracle, 48, 32, 2)
    data.samples = 4
    r = rtm.Renderer(data, mode="repaired", max_bounces=8)
    r.Render(str(tmp_path / "plain"))
    r.Render(str(tmp_path / "with"), aov=True)
    for ext in (".jpg", ".bmp"):
        assert (tmp_path / ("plain" + ext)).read_bytes() == (tmp_path / ("with" + ext)).read_bytes()
    planes = _aov(r)
    for k, comp in (("depth", 1), ("normal", 3), ("albedo", 3)):
        raw = (tmp_path / f"with_{k}.pfm").read_bytes()
        head = b"PF\n" if comp == 3 else b"Pf\n"
        assert raw.startswith(head + b"48 32\n-1.0\n")
        body = np.frombuffer(raw[len(head + b"48 32\n-1.0\n"):], dtype="<f4").reshape(32, 48 * comp)[::-1]
        assert np.array_equal(_bits(body.reshape(planes[k].shape)), _bits(planes[k])), k
    for k in ("normal", "albedo"):
        assert (tmp_path / f"with_{k}.bmp").stat().st_size == 54 + 48 * 3 * 32
