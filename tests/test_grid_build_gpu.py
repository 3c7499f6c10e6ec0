"""rtm_scene_create_device (include/rtm.h; csrc/rtm_grid_build.hip, csrc/rtm_grid_build_kernel.h): a scene built entirely on the
device from a device sphere array is the scene rtm_scene_create builds from the same array — the grid's tables bit for bit
against the host builder (rtm_debug_grid_build) and against a host-built scene read back through the same hook
(rtm_debug_scene_grid), the same "no grid" outcomes, the same frames, AOVs, mattes and counters, the same variant 0."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

UNSUPPORTED = -8


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd
    return raytracingmin_amd


# ---- sphere arrays ---------------------------------------------------------------------------------------------------------
def _sphere_array(c, r, emit_every=0):
    """rtm_sphere[n] from centres and radii: colour 0.5; with emit_every, every emit_every-th sphere is a black light."""
    from raytracingmin_amd import _lib
    n = len(r)
    buf = np.zeros((n, 10), dtype=np.float64)
    buf[:, 0:3] = c
    buf[:, 3:6] = 0.5
    if emit_every:
        buf[::emit_every, 3:6] = 0.0
        buf[::emit_every, 6:9] = 4.0
    buf.view(np.float32)[:, 18] = np.asarray(r, dtype=np.float64).astype(np.float32)
    return (_lib.rtm_sphere * n).from_buffer_copy(buf.tobytes())


def _stress(rtm, n, seed=12345):
    from raytracingmin_amd import _lib
    st = _lib.rtm_settings()
    arr = (_lib.rtm_sphere * n)()
    _lib.check(rtm.lib().rtm_scene_make_stress(seed, n, C.byref(st), arr), "make_stress_scene")
    return st, arr


def _awkward():
    """The four awkward families of tests/test_grid_gpu.py (test_grid_nearest_awkward_scenes), the same generator."""
    rng = np.random.default_rng(172)
    scenes = {}
    n = 3000
    c = rng.uniform(-20, 20, (n, 3))
    r = rng.uniform(0.1, 1.5, n)
    c[:6] = [[0, 0, 1e4 + 25], [0, 0, -1e4 - 25], [1e4 + 25, 0, 0], [-1e4 - 25, 0, 0], [0, 1e4 + 25, 0], [0, -1e4 - 25, 0]]
    r[:6] = 1e4
    r[6:30] = 0.0
    c[1000:1100] = c[900:1000]
    r[1000:1100] = r[900:1000]
    c[1100:1150] = c[850:900]
    scenes["walls+zero+duplicates"] = (c, r)
    n = 2000
    c = rng.uniform(-30, 30, (n, 3))
    c[:, 2] = 0.0
    scenes["flat"] = (c, rng.uniform(0.2, 0.9, n))
    n = 4000
    c = np.concatenate([rng.normal(size=(n // 2, 3)) * 5 + [-200, 0, 0], rng.normal(size=(n // 2, 3)) * 8 + [300, 50, -40]])
    scenes["clusters"] = (c, 10.0 ** rng.uniform(-2, 1, n))
    g = np.arange(-6, 7)
    c = np.array([[x, y, z] for x in g for y in g for z in g], dtype=np.float64)
    scenes["lattice"] = (c, np.full(len(c), 0.25))
    return scenes


def _walls_medium():
    """Flags flip in all four classification rounds (6, 11, 5 and 2 of them); 24 big spheres, an 18 x 17 x 16 grid."""
    rng = np.random.default_rng(11)
    c = rng.uniform(-20, 20, (3000, 3))
    r = rng.uniform(0.1, 1.5, 3000)
    c[:6] = [[0, 0, 1e4 + 25], [0, 0, -1e4 - 25], [1e4 + 25, 0, 0], [-1e4 - 25, 0, 0], [0, 1e4 + 25, 0], [0, -1e4 - 25, 0]]
    r[:6] = 1e4
    r[6:30] = 0.0
    r[30:50] = rng.uniform(5, 9, 20)
    return c, r


def _knot():
    """One cell list about 5000 entries long on a 24 x 24 x 23 grid."""
    rng = np.random.default_rng(7)
    c = rng.uniform(-20, 20, (3000, 3))
    c2 = np.array([3.0, -2.0, 5.0]) + 0.02 * rng.normal(size=(5000, 3))
    r = rng.uniform(0.1, 1, 3000)  # (the centres of both groups are drawn first: that order gives the 24 x 24 x 23 grid)
    return np.concatenate([c, c2]), np.concatenate([r, np.full(5000, 0.01)])


_SCENES = {}


def _scene(rtm, name):
    """name -> rtm_sphere[n], made once for the module and left unchanged"""
    if name not in _SCENES:
        if name.startswith("stress"):
            arr = _stress(rtm, int(name[6:]))[1]
        elif name == "walls+medium":
            arr = _sphere_array(*_walls_medium())
        elif name == "knot":
            arr = _sphere_array(*_knot())
        else:
            arr = _sphere_array(*_awkward()[name], emit_every=7)
        _SCENES[name] = arr
    return _SCENES[name]


# ---- scenes and their grids ------------------------------------------------------------------------------------------------
def _to_device(arr):
    import torch
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _create_device(rtm, d_arr, n, stream=None):
    h = C.c_void_p()
    rtm._lib.check(rtm.lib().rtm_scene_create_device(C.c_void_p(d_arr.data_ptr()), n, 0, stream or _stream(), C.byref(h)),
                   "rtm_scene_create_device")
    return h


def _create_host(rtm, d_arr, n):
    """rtm_scene_create(..., spheres_on_device = 1, ...): the rows come back and the HOST builds the grid"""
    h = C.c_void_p()
    rtm._lib.check(rtm.lib().rtm_scene_create(C.c_void_p(d_arr.data_ptr()), n, 1, 0, C.byref(h)), "rtm_scene_create")
    return h


def _tables(call, what):
    """(rc, None) or (0, (info, ranges, items, big)) of a hook in rtm_debug_grid_build's format: call(info, ranges, ranges_cap,
    items, items_cap, big, big_cap)"""
    from raytracingmin_amd import _lib
    info = np.zeros(12, dtype=np.uint64)
    rc = call(info.ctypes.data, None, 0, None, 0, None, 0)
    if rc != 0:
        return rc, None
    ranges = np.zeros(int(info[0]) * 2, dtype=np.uint32)
    items = np.zeros(max(int(info[1]), 1), dtype=np.uint32)
    big = np.zeros(max(int(info[2]), 1), dtype=np.int32)
    _lib.check(call(info.ctypes.data, ranges.ctypes.data, ranges.size, items.ctypes.data, items.size, big.ctypes.data, big.size), what)
    return 0, (info, ranges, items[:int(info[1])], big[:int(info[2])])


def _builder_tables(rtm, arr, n):
    L = rtm.lib()
    return _tables(lambda info, *rest: L.rtm_debug_grid_build(arr, n, info, None, *rest), "rtm_debug_grid_build")


def _scene_tables(rtm, h):
    """... and extra[2] of rtm_debug_scene_grid"""
    L = rtm.lib()
    extra = np.full(2, 99, dtype=np.uint64)
    rc, t = _tables(lambda info, *rest: L.rtm_debug_scene_grid(h, info, *rest, extra.ctypes.data), "rtm_debug_scene_grid")
    return rc, t, extra


def _same_tables(a, b, label):
    for x, y, part in zip(a, b, ("info", "ranges", "items", "big")):
        assert x.shape == y.shape and np.array_equal(x, y), (label, part)


TABLE_SCENES = ["stress64", "stress65", "stress257", "stress1025", "stress20000", "stress100000", "walls+zero+duplicates", "flat",
                "clusters", "lattice", "walls+medium", "knot"]


@pytest.mark.parametrize("name", TABLE_SCENES)
def test_tables_bit_for_bit(rtm, name):
    """The device-built scene's grid is the host builder's: all 12 info words, every cell's range, every list entry in the
    host's order, the big list; every record is its sphere's geometry row with the index in it.  A host-built scene read
    back through the same hook is the third witness."""
    arr = _scene(rtm, name)
    n = len(arr)
    rc, want = _builder_tables(rtm, arr, n)
    assert rc == 0
    info = want[0]
    if name == "walls+medium":  # every round of the classification changes flags in this one
        assert (int(info[2]), tuple(int(v) for v in info[3:6])) == (24, (18, 17, 16))
    if name == "knot":
        assert tuple(int(v) for v in info[3:6]) == (24, 24, 23)
        assert int((want[1][1::2] - want[1][0::2]).max()) > 4000  # one cell list holds the knot
    d_arr = _to_device(arr)
    L = rtm.lib()
    h_dev = _create_device(rtm, d_arr, n)
    h_host = _create_host(rtm, d_arr, n)
    try:
        rc_d, got_d, extra_d = _scene_tables(rtm, h_dev)
        rc_h, got_h, extra_h = _scene_tables(rtm, h_host)
        assert rc_d == 0 and rc_h == 0
        print(f"{name}: n={n}, grid {info[3]}x{info[4]}x{info[5]}, {info[1]} entries, {info[2]} big; "
              f"mismatching records device/host build: {extra_d[0]}/{extra_h[0]}")
        _same_tables(got_h, want, name + ": host-built scene vs builder")
        _same_tables(got_d, want, name + ": device-built scene vs builder")
        assert extra_d[0] == 0 and extra_h[0] == 0
        assert extra_d[1] == extra_h[1]
        assert L.rtm_scene_size(h_dev) == L.rtm_scene_size(h_host) == n
        # a short buffer: RTM_ERR_CAPACITY as the builder hook gives it
        short = np.zeros(1, dtype=np.uint32)
        info2 = np.zeros(12, dtype=np.uint64)
        assert L.rtm_debug_scene_grid(h_dev, info2.ctypes.data, short.ctypes.data, 1, None, 0, None, 0, None) == -7
        assert np.array_equal(info2, info)
    finally:
        assert L.rtm_scene_destroy(h_dev) == 0 and L.rtm_scene_destroy(h_host) == 0


# ---- frames ------------------------------------------------------------------------------------------------------------
def _settings(rtm, w, h, s, ss=1, st=None):
    from raytracingmin_amd import _lib
    if st is None:  # a camera inside the awkward scenes' box, looking at the origin
        data = rtm.SettingData()
        data.camera = rtm.Camera(rtm.vec3(2.0, 1.0, -24.0), rtm.vec3(0, 0, 0), rtm.vec3(0, 1, 0), 1.2)
        st = data.settings_c()
    out = _lib.rtm_settings.from_buffer_copy(bytes(st))
    out.width, out.height, out.samples, out.super_samples = w, h, s, ss
    return out


def _options(rtm, h, mb, variant, seed=5, count_tests=False):
    from raytracingmin_amd import _lib
    o = _lib.rtm_options()
    o.mode = _lib.MODE_REPAIRED | _lib.MODE_HOST_TRIG | (_lib.MODE_COUNT_TESTS if count_tests else 0)
    o.max_bounces, o.seed, o.row_begin, o.row_end, o.device, o.variant = mb, seed, 0, h, 0, variant
    return o


def _frame(rtm, st, scene, opt):
    """(rc, f64, u8, stats) of rtm_render_scene"""
    import torch
    from raytracingmin_amd import _lib
    f64 = torch.zeros((st.height, st.width, 3), dtype=torch.float64, device="cuda")
    u8 = torch.zeros((st.height, st.width, 3), dtype=torch.uint8, device="cuda")
    s = _lib.rtm_stats()
    rc = rtm.lib().rtm_render_scene(C.byref(st), scene, C.byref(opt), C.c_void_p(f64.data_ptr()), None, C.c_void_p(u8.data_ptr()),
                                    _stream(), C.byref(s))
    return rc, f64.cpu().numpy(), u8.cpu().numpy(), s.as_dict()


def _same_frame(rtm, st, h_dev, h_host, opt, label, expect_variant=None):
    rc_d, f_d, u_d, s_d = _frame(rtm, st, h_dev, opt)
    rc_h, f_h, u_h, s_h = _frame(rtm, st, h_host, opt)
    assert rc_d == rc_h == 0, (label, rc_d, rc_h, rtm.lib().rtm_last_error_detail())
    assert np.array_equal(f_d.view(np.uint64), f_h.view(np.uint64)), label
    assert np.array_equal(u_d, u_h), label
    for k in ("casts", "bounces", "draws", "variant", "object_tests"):
        assert s_d[k] == s_h[k], (label, k, s_d[k], s_h[k])
    if expect_variant is not None:
        assert s_d["variant"] == expect_variant, (label, s_d["variant"])
    return f_d, s_d


@pytest.mark.parametrize("name", ["n63", "nan", "too-many-big"])
def test_no_grid_the_same_as_the_host(rtm, name):
    """Scenes the host builder declines: fewer than 64 spheres, a NaN centre, more than 1024 spheres that span the scene.
    Neither build has a grid, variant 17 is refused for both, and variant 0 renders the same frame from both."""
    rng = np.random.default_rng(5)
    if name == "n63":
        arr = _stress(rtm, 63)[1]
    elif name == "nan":
        c, r = rng.uniform(-20, 20, (300, 3)), rng.uniform(0.2, 1.5, 300)
        c[117, 1] = np.nan
        arr = _sphere_array(c, r, emit_every=7)
    else:
        c = np.concatenate([rng.uniform(-1, 1, (1100, 3)), rng.uniform(-20, 20, (200, 3))])
        r = np.concatenate([np.full(1100, 1e4), rng.uniform(0.2, 1.5, 200)])
        arr = _sphere_array(c, r, emit_every=7)
    n = len(arr)
    assert _builder_tables(rtm, arr, n)[0] == UNSUPPORTED
    L = rtm.lib()
    d_arr = _to_device(arr)
    h_dev, h_host = _create_device(rtm, d_arr, n), _create_host(rtm, d_arr, n)
    try:
        assert _scene_tables(rtm, h_dev)[0] == UNSUPPORTED and _scene_tables(rtm, h_host)[0] == UNSUPPORTED
        st = _settings(rtm, 16, 16, 1, st=_stress(rtm, 63)[0] if name == "n63" else None)
        for h in (h_dev, h_host):
            assert _frame(rtm, st, h, _options(rtm, 16, 8, 17))[0] == UNSUPPORTED
        _, s = _same_frame(rtm, st, h_dev, h_host, _options(rtm, 16, 8, 0), name)
        assert s["variant"] != 17
    finally:
        assert L.rtm_scene_destroy(h_dev) == 0 and L.rtm_scene_destroy(h_host) == 0


@pytest.mark.parametrize("n,w,h,spp", [(64, 80, 48, 8), (300, 64, 40, 4), (3000, 48, 32, 4)])
def test_frames_counters_aovs_and_mattes(rtm, n, w, h, spp):
    """Whole frames of the stress family through rtm_render_scene, capped and unlimited depth, the grid kernel by name and
    through variant 0: f64 and u8 bit for bit, the counters, the variant.  On the 300-sphere scene also the counting
    instantiation's object_tests, one rtm_render_aov and one rtm_render_mattes call."""
    import torch
    from raytracingmin_amd import _lib
    st0, arr = _stress(rtm, n)
    L = rtm.lib()
    d_arr = _to_device(arr)
    h_dev, h_host = _create_device(rtm, d_arr, n), _create_host(rtm, d_arr, n)
    try:
        st = _settings(rtm, w, h, spp, st=st0)
        for mb in (8, -1):
            for variant in (17, 0):
                f, s = _same_frame(rtm, st, h_dev, h_host, _options(rtm, h, mb, variant), (n, mb, variant), expect_variant=17)
                # (the two small scenes' frames are black, in the CPU oracle too: no path of theirs ends on a light.
                # Their counters still see every hit and bounce.)
                assert s["bounces"] > 0 and (f.any() or n < 3000)
        if n != 300:
            return
        _, s = _same_frame(rtm, st, h_dev, h_host, _options(rtm, h, 8, 17, count_tests=True), "count tests", expect_variant=17)
        assert s["object_tests"] > 0
        st2 = _settings(rtm, 64, 40, 1, ss=2, st=st0)
        opt = _options(rtm, 40, 8, 0)
        planes = []
        for scene in (h_dev, h_host):
            depth = torch.zeros((40, 64), dtype=torch.float32, device="cuda")
            normal = torch.zeros((40, 64, 3), dtype=torch.float32, device="cuda")
            albedo = torch.zeros((40, 64, 3), dtype=torch.float32, device="cuda")
            obj = torch.zeros((40, 64), dtype=torch.int32, device="cuda")
            bufs = _lib.rtm_aov_buffers(depth.data_ptr(), normal.data_ptr(), albedo.data_ptr(), obj.data_ptr())
            _lib.check(L.rtm_render_aov(C.byref(st2), scene, C.byref(opt), C.byref(bufs), _stream()), "rtm_render_aov")
            ids = torch.zeros((4, 40, 64), dtype=torch.int32, device="cuda")
            cov = torch.zeros((4, 40, 64), dtype=torch.float32, device="cuda")
            alpha = torch.zeros((40, 64), dtype=torch.float32, device="cuda")
            mb = _lib.rtm_matte_buffers(ids.data_ptr(), cov.data_ptr(), alpha.data_ptr())
            _lib.check(L.rtm_render_mattes(C.byref(st2), scene, C.byref(opt), 4, C.byref(mb), _stream()), "rtm_render_mattes")
            planes.append([t.cpu().numpy() for t in (depth, normal, albedo, obj, ids, cov, alpha)])
        for a, b, what in zip(planes[0], planes[1], ("depth", "normal", "albedo", "object", "id", "coverage", "alpha")):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what
        assert (planes[0][3] >= 0).any()
    finally:
        assert L.rtm_scene_destroy(h_dev) == 0 and L.rtm_scene_destroy(h_host) == 0


def test_ties_decided_by_list_order(rtm):
    """walls + zero radii + duplicates as a frame: exact duplicates and concentric spheres share cells, and the lowest index
    must win (src/Renderer.cpp:67) — the lists' order decides."""
    arr = _scene(rtm, "walls+zero+duplicates")
    n = len(arr)
    d_arr = _to_device(arr)
    h_dev, h_host = _create_device(rtm, d_arr, n), _create_host(rtm, d_arr, n)
    try:
        st = _settings(rtm, 48, 32, 4)
        for variant in (17, 0):
            f, s = _same_frame(rtm, st, h_dev, h_host, _options(rtm, 32, 8, variant), ("ties", variant))
            assert f.any()
    finally:
        assert rtm.lib().rtm_scene_destroy(h_dev) == 0 and rtm.lib().rtm_scene_destroy(h_host) == 0


def test_environment_sphere(rtm):
    """The scene of tests/test_grid_gpu.py::test_environment_sphere_keeps_variant_0_off_the_grid: a diffuse sphere of radius
    3000 around 2000 stress spheres.  Both builds decide grid_far_bounces = 1, and variant 0 resolves the same way; with a black
    emissive environment sphere both decide 0 and variant 0 keeps the grid."""
    for colour, far in (((0.6, 0.6, 0.7), 1), ((0.0, 0.0, 0.0), 0)):
        data = rtm.make_stress_scene(n=2000, seed=17)
        data.object.append(rtm.SphereObject(rtm.vec3(0, 0, 0), 3000.0, rtm.Material(rtm.vec3(*colour), rtm.vec3(0.8, 0.8, 0.8))))
        data.width, data.height, data.samples, data.superSamples = 24, 16, 2, 1
        st, arr, n = data.to_c()
        d_arr = _to_device(arr)
        h_dev, h_host = _create_device(rtm, d_arr, n), _create_host(rtm, d_arr, n)
        try:
            rc_d, t_d, extra_d = _scene_tables(rtm, h_dev)
            rc_h, t_h, extra_h = _scene_tables(rtm, h_host)
            assert rc_d == 0 and rc_h == 0
            _same_tables(t_d, t_h, "environment sphere")
            assert extra_d[1] == extra_h[1] == far and extra_d[0] == 0
            _, s0 = _same_frame(rtm, st, h_dev, h_host, _options(rtm, 16, 8, 0, seed=13), ("environment", 0))
            assert (s0["variant"] == 17) == (far == 0)
            _same_frame(rtm, st, h_dev, h_host, _options(rtm, 16, 8, 17, seed=13), ("environment", 17), expect_variant=17)
        finally:
            assert rtm.lib().rtm_scene_destroy(h_dev) == 0 and rtm.lib().rtm_scene_destroy(h_host) == 0


def test_animation_on_one_stream(rtm):
    """Build, render, destroy; move every centre on the device and build again on the same stream with no synchronisation in
    between — the build is ordered behind the move by the stream alone.  Each frame is the host-built scene's of the moved
    spheres.  Three moves after the first build: the later builds run on recycled pool memory and next to parked scenes."""
    import torch
    st0, arr = _stress(rtm, 3000, seed=31)
    n = len(arr)
    L = rtm.lib()
    st = _settings(rtm, 48, 32, 2, st=st0)
    opt = _options(rtm, 32, 8, 17)
    side = torch.cuda.Stream()
    d_arr = _to_device(arr)
    offset = torch.tensor([0.75, -0.5, 0.25], dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    frames = []
    with torch.cuda.stream(side):
        stream = C.c_void_p(side.cuda_stream)
        for step in range(4):
            if step:
                d_arr.view(torch.float64).view(n, 10)[:, 0:3] += offset  # enqueued on `side`; not waited for
            h = _create_device(rtm, d_arr, n, stream)
            f64 = torch.zeros((32, 48, 3), dtype=torch.float64, device="cuda")
            assert L.rtm_render_scene(C.byref(st), h, C.byref(opt), C.c_void_p(f64.data_ptr()), None, None, stream, None) == 0
            assert L.rtm_scene_destroy(h) == 0  # the render may still be running: the scene is parked
            frames.append(f64)
        side.synchronize()
        assert L.rtm_stream_release(0, stream) == 0  # (the stream goes away with this test)
    moved = np.frombuffer(bytes(arr), dtype=np.float64).reshape(n, 10).copy()
    for step in range(4):
        if step:
            moved[:, 0:3] += np.array([0.75, -0.5, 0.25])
        host_arr = (rtm._lib.rtm_sphere * n).from_buffer_copy(moved.tobytes())
        h = C.c_void_p()
        rtm._lib.check(L.rtm_scene_create(host_arr, n, 0, 0, C.byref(h)), "rtm_scene_create")
        rc, ref, _, s = _frame(rtm, st, h, opt)
        assert rc == 0 and s["variant"] == 17 and ref.any()
        assert L.rtm_scene_destroy(h) == 0
        assert np.array_equal(frames[step].cpu().numpy().view(np.uint64), ref.view(np.uint64)), step
    assert not np.array_equal(frames[0].cpu().numpy(), frames[3].cpu().numpy())


def test_renderer_set_device_spheres(rtm):
    """Renderer.set_device_spheres(pack_spheres(...)) renders Renderer(data)'s frame bit for bit; set_device_spheres(None)
    returns the renderer to data.object."""
    import torch
    data = rtm.make_stress_scene(n=500, seed=23)
    data.width, data.height, data.samples, data.superSamples = 48, 32, 4, 1
    ref, ref_stats = rtm.Renderer(data, max_bounces=8, seed=9).render_rows_device(want=("f64",))
    ref = ref["f64"].cpu().numpy()
    cols = [torch.tensor([list(v(o)) for o in data.object], dtype=torch.float64, device="cuda")
            for v in (lambda o: o.m_position, lambda o: o.m_material.color, lambda o: o.m_material.emission)]
    radius = torch.tensor([o.m_size for o in data.object], dtype=torch.float64, device="cuda")
    packed = rtm.pack_spheres(cols[0], radius, cols[1], cols[2])
    arr, n = data.spheres_c()
    assert packed.cpu().numpy().tobytes() == bytes(arr)[:n * 80]
    other = rtm.make_stress_scene(n=100, seed=2)  # what data.object holds must not matter while the device scene is set
    other.width, other.height, other.samples, other.superSamples = 48, 32, 4, 1
    other.camera = data.camera
    r = rtm.Renderer(other, max_bounces=8, seed=9)
    plain = r.render_rows_device(want=("f64",))[0]["f64"].cpu().numpy()
    assert not np.array_equal(plain, ref)
    r.set_device_spheres(packed)
    out, stats = r.render_rows_device(want=("f64",))
    assert np.array_equal(out["f64"].cpu().numpy().view(np.uint64), ref.view(np.uint64))
    assert (stats["casts"], stats["variant"]) == (ref_stats["casts"], ref_stats["variant"])
    with pytest.raises(RuntimeError):  # the host-array call would render data.object
        r.render_rows()
    with pytest.raises(ValueError):  # a refused tensor leaves the device scene in place
        r.set_device_spheres(packed[:, :79])
    other.object.pop()  # an edit of data.object: still the device scene
    again = r.render_rows_device(want=("f64",))[0]["f64"].cpu().numpy()
    assert np.array_equal(again.view(np.uint64), ref.view(np.uint64))
    r.set_device_spheres(None)
    back = r.render_rows_device(want=("f64",))[0]["f64"].cpu().numpy()
    expect = rtm.Renderer(other, max_bounces=8, seed=9).render_rows_device(want=("f64",))[0]["f64"].cpu().numpy()
    assert np.array_equal(back.view(np.uint64), expect.view(np.uint64)) and not np.array_equal(back, ref)
