"""The coverage AOVs on a real MI355X (-m gpu).  Everything is bit equality: the ranking hook against _matte_ref.rank, whole
frames and fixed pixels of rtm_render_mattes against layers built from the oracle's own first hits (the _first_hit recipe of
tests/test_aov_gpu.py over all SS^2 sub-pixels), the three searches against each other, rtm_matte and rtm_composite against
their NumPy restatements, and the files Render(mattes=...) and rtm_cli write."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _matte_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
PLANES = ("id", "coverage", "alpha")


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


def _mattes(r, layers=4, **kw):
    import torch
    out = r.render_mattes(layers, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def _expected(oracle, st, isect, n, mode, pixels, layers):
    """(ids (layers, P), coverage (layers, P), alpha (P,), the raw (P, SS^2) first hits) of the listed pixels from the oracle."""
    hits = _matte_ref.sub_pixel_ids(oracle, st, isect, n, mode, pixels)
    return _matte_ref.rank(hits, layers) + (hits,)


def _check_pixels(got, want, pixels, W):
    idx = np.array([y * W + x for x, y in pixels])
    L = got["id"].shape[0]
    assert np.array_equal(got["id"].reshape(L, -1)[:, idx], want[0])
    assert np.array_equal(_bits(got["coverage"].reshape(L, -1)[:, idx]), _bits(want[1]))
    assert np.array_equal(_bits(got["alpha"].reshape(-1)[idx]), _bits(want[2]))


# ---- the ranking alone ----------------------------------------------------------------------------------------------------
def _rank_lists(n_sub, n_pixels):
    """Five kinds of id lists, pixel p of kind p % 5: a pool of 3 ids (many ties), n_sub distinct ids in descending order, all
    -1, a mix with other negative ids, ids near 2^31 - 1."""
    rng = np.random.default_rng(1000 + n_sub)
    ids = np.empty((n_pixels, n_sub), np.int32)
    for p in range(n_pixels):
        kind = p % 5
        if kind == 0:
            ids[p] = rng.choice([7, 3, 11], n_sub)
        elif kind == 1:
            ids[p] = 5000 + p - np.arange(n_sub)
        elif kind == 2:
            ids[p] = -1
        elif kind == 3:
            ids[p] = rng.choice([-1, -2, -(2**31), 4, 0, 9, 2], n_sub)
        else:
            ids[p] = 2**31 - 1 - rng.integers(0, 4, n_sub)
    return ids


@pytest.mark.parametrize("layers", [1, 4, 8])
@pytest.mark.parametrize("ss", [1, 2, 3, 5, 8])
def test_rank_hook_equals_the_restatement(rtm, ss, layers):
    import torch
    n_pixels = 64 * 3 + 5  # a partial block
    ids = _rank_lists(ss * ss, n_pixels)
    if ss == 8:
        assert len(set(ids[1].tolist())) == 64  # 64 distinct ids in one pixel
    want = _matte_ref.rank(ids, layers)
    dev = torch.device("cuda", 0)
    d_ids = torch.from_numpy(ids).to(dev)
    out_id = torch.full((layers, n_pixels), 77, dtype=torch.int32, device=dev)
    out_cov = torch.full((layers, n_pixels), 7.0, dtype=torch.float32, device=dev)
    out_alpha = torch.full((n_pixels + 64,), 7.0, dtype=torch.float32, device=dev)  # (room behind: the partial block stops at n_pixels)
    rtm._lib.check(rtm.lib().rtm_debug_matte_rank(ss, layers, 0, d_ids.data_ptr(), n_pixels, out_id.data_ptr(), out_cov.data_ptr(),
                                                  out_alpha.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "rank")
    torch.cuda.synchronize()
    assert np.array_equal(out_id.cpu().numpy(), want[0])
    assert np.array_equal(_bits(out_cov), _bits(want[1]))
    assert np.array_equal(_bits(out_alpha[:n_pixels]), _bits(want[2]))
    assert (out_alpha[n_pixels:] == 7.0).all()


# ---- small scenes, whole frame against the oracle -------------------------------------------------------------------------
def _cornell(rtm, oracle, w, h, ss):
    path = oracle.scene_path("cornellBoxSetting.json")
    data = rtm.LoadData(path).data
    data.width, data.height, data.samples, data.superSamples = w, h, 1, ss
    st, arr, n = oracle.load_scene(path, width=w, height=h, samples=1, super_samples=ss)
    return data, st, arr, n


@pytest.mark.parametrize("ss", [1, 2, 3, 4])
def test_cornell_whole_frame_matches_the_oracle(rtm, oracle, ss):
    import torch
    w, h = 96, 56
    data, st, arr, n = _cornell(rtm, oracle, w, h, ss)
    r = rtm.Renderer(data, mode="repaired")
    got = _mattes(r)
    assert got["id"].shape == (4, h, w) and got["coverage"].shape == (4, h, w) and got["alpha"].shape == (h, w)
    assert got["id"].dtype == np.int32 and got["coverage"].dtype == np.float32
    pixels = [(x, y) for y in range(h) for x in range(w)]
    _check_pixels(got, _expected(oracle, st, _matte_ref.sphere_isect(oracle, arr), n, 1, pixels, 4), pixels, w)
    assert np.all(_bits(got["alpha"]) == np.float32(1.0).view(np.uint32))  # the box is closed
    _matte_ref.check_invariants(got["id"], got["coverage"], got["alpha"], ss * ss)
    if ss == 1:
        obj = r.render_aov(want=("object",))["object"]
        torch.cuda.synchronize()
        assert np.array_equal(got["id"][0], obj.cpu().numpy())
        assert np.all(got["coverage"][0] == 1.0) and np.all(got["id"][1:] == -1)


def test_open_scene_alpha_and_partly_covered_pixels(rtm, oracle):
    w, h, ss = 61, 37, 4  # the width is no multiple of 8
    path = oracle.scene_path("settingData.json")
    data = rtm.LoadData(path).data
    data.width, data.height, data.samples, data.superSamples = w, h, 1, ss
    st, arr, n = oracle.load_scene(path, width=w, height=h, samples=1, super_samples=ss)
    got = _mattes(rtm.Renderer(data, mode="repaired"))
    pixels = [(x, y) for y in range(h) for x in range(w)]
    want = _expected(oracle, st, _matte_ref.sphere_isect(oracle, arr), n, 1, pixels, 4)
    miss = (want[3] < 0).sum(axis=1)
    assert int(((miss > 0) & (miss < ss * ss)).sum()) == 61 and int((miss == ss * ss).sum()) == 2009
    _check_pixels(got, want, pixels, w)
    _matte_ref.check_invariants(got["id"], got["coverage"], got["alpha"], ss * ss)


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
    want = _expected(oracle, ost, isect, n, 1, pixels, 4)
    for variant in (0, 1):
        got = _mattes(rtm.Renderer(data, mode="repaired", variant=variant))
        _check_pixels(got, want, pixels, w)
    assert any(objs[i].type == 2 for i in np.unique(got["id"]).tolist() if i >= 0)  # some layer holds a plane


# ---- the stress scene: three searches, invariants, the oracle at fixed pixels ---------------------------------------------
# Chosen with the oracle (rtmo_make_stress_scene(7, 2000), camera as the maker leaves it); each test asserts its pixels'
# category from the oracle's answer, so that a stale list fails loudly.
MANY_IDS = [(18, 13), (28, 14), (21, 15)]  # five or more distinct ids
TIE_ORDER = [(15, 0), (26, 2), (26, 5), (22, 7), (16, 10), (19, 12), (19, 13), (31, 15), (23, 16), (13, 18)]
ALL_MISS = [(0, 0), (1, 8), (5, 16), (45, 24), (41, 31)]
PARTLY = [(12, 0), (8, 6), (8, 10), (22, 14), (7, 19), (6, 24), (10, 29)]  # partly covered, two or more ids


@pytest.fixture(scope="module")
def stress(rtm):
    """The stress scene's planes at 48x32 SS 4 (layers 4 and 8) and 24x16 SS 8 (layers 8), by the three searches."""
    data = rtm.make_stress_scene(n=2000, seed=7)
    out = {"data": data}
    for key, (w, h, ss, layer_set) in {"a": (48, 32, 4, (4, 8)), "b": (24, 16, 8, (8,))}.items():
        data.width, data.height, data.samples, data.superSamples = w, h, 1, ss
        for variant in (0, 17, 1):
            r = rtm.Renderer(data, mode="repaired", variant=variant)
            for layers in layer_set:
                out[key, layers, variant] = _mattes(r, layers)
    return out


def _stress_oracle(oracle, stress, w, h, ss):
    data = stress["data"]
    data.width, data.height, data.samples, data.superSamples = w, h, 1, ss
    st, arr, n = data.to_c()
    ost = oracle.Settings.from_buffer_copy(st)
    oarr = (oracle.Sphere * n).from_buffer_copy(arr)
    return ost, _matte_ref.sphere_isect(oracle, oarr), n


@pytest.mark.parametrize("key,layers,n_sub", [("a", 4, 16), ("a", 8, 16), ("b", 8, 64)])
def test_stress_searches_agree_and_the_invariants_hold(stress, key, layers, n_sub):
    auto = stress[key, layers, 0]
    _same(auto, stress[key, layers, 17])
    _same(auto, stress[key, layers, 1])
    _matte_ref.check_invariants(auto["id"], auto["coverage"], auto["alpha"], n_sub)
    assert (auto["alpha"] > 0).mean() > 0.2 and (auto["id"][1] >= 0).any()  # the frame sees spheres and shared pixels
    if (key, layers) == ("a", 8):  # fewer layers are the first of more
        four = stress["a", 4, 0]
        assert np.array_equal(four["id"], auto["id"][:4]) and np.array_equal(_bits(four["coverage"]), _bits(auto["coverage"][:4]))
        assert np.array_equal(_bits(four["alpha"]), _bits(auto["alpha"]))


def _first_seen_order(hits):
    seen = [v for k, v in enumerate(hits) if v >= 0 and v not in hits[:k]]
    return sorted(seen, key=lambda v: (-hits.count(v), hits.index(v)))


def test_stress_fixed_pixels_match_the_oracle(oracle, stress):
    w, h, ss = 48, 32, 4
    ost, isect, n = _stress_oracle(oracle, stress, w, h, ss)
    pixels = MANY_IDS + TIE_ORDER + ALL_MISS + PARTLY
    want8 = _expected(oracle, ost, isect, n, 1, pixels, 8)
    hits = {p: want8[3][k].tolist() for k, p in enumerate(pixels)}
    for p in MANY_IDS:
        assert len(set(v for v in hits[p] if v >= 0)) >= 5, p
    for p in TIE_ORDER:
        by_rank = [int(v) for v in _matte_ref.rank([hits[p]], 8)[0][:, 0] if v >= 0]
        assert len(set(v for v in hits[p] if v >= 0)) <= 8 and by_rank != _first_seen_order(hits[p]), p
    for p in ALL_MISS:
        assert all(v < 0 for v in hits[p]), p
    for p in PARTLY:
        assert any(v < 0 for v in hits[p]) and len(set(v for v in hits[p] if v >= 0)) >= 2, p
    _check_pixels(stress["a", 8, 0], want8, pixels, w)
    _check_pixels(stress["a", 4, 0], _matte_ref.rank(want8[3], 4), pixels, w)


def test_stress_truncated_pixels_match_the_oracle(oracle, stress):
    w, h, ss = 24, 16, 8
    ost, isect, n = _stress_oracle(oracle, stress, w, h, ss)
    pixels = [(12, 4), (11, 7), (9, 9)]
    want = _expected(oracle, ost, isect, n, 1, pixels, 8)
    assert [len(set(v for v in row.tolist() if v >= 0)) for row in want[3]] == [9, 10, 10]  # more objects than layers
    row = want[3][2].tolist()
    assert want[0][:2, 2].tolist() == [912, 877] and (row.count(912), row.count(877)) == (10, 8)
    assert [row.count(int(i)) for i in want[0][2:6, 2]] == [3, 3, 3, 3] and row.count(int(want[0][6, 2])) < 3  # a four-way tie
    _check_pixels(stress["b", 8, 0], want, pixels, w)
    got = stress["b", 8, 0]
    for (x, y) in pixels:  # alpha - sum of the coverages: what was dropped
        assert got["alpha"][y, x] > got["coverage"][:, y, x].astype(np.float64).sum()


# ---- rows, bands, null planes, streams ------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,band", [((5, 43), None), ((0, 56), (3, 1))])
def test_rows_and_bands_are_the_full_frame_rows(rtm, oracle, rows, band):
    data, *_ = _cornell(rtm, oracle, 70, 56, 3)
    r = rtm.Renderer(data, mode="repaired")
    full = _mattes(r, 3)
    part = _mattes(r, 3, row_begin=rows[0], row_end=rows[1], band=band)
    if band is None:
        sel = list(range(rows[0], rows[1]))
    else:
        sel = [y for y in range(rows[0], rows[1]) if ((y - rows[0]) // 8) % band[0] == band[1]]
    assert part["alpha"].shape == (len(sel), 70) and part["id"].shape == (3, len(sel), 70)
    assert np.array_equal(_bits(part["alpha"]), _bits(full["alpha"][sel]))
    for k in ("id", "coverage"):
        assert np.array_equal(_bits(part[k]), _bits(full[k][:, sel])), k


def test_null_planes_are_not_written_and_the_others_stay_in_bounds(rtm, oracle):
    import torch
    from raytracingmin_amd import _lib
    data, *_ = _cornell(rtm, oracle, 40, 24, 2)
    r = rtm.Renderer(data, mode="repaired")
    full = _mattes(r, 2)
    # the coverage planes between two guard regions of one allocation; id and alpha stay null
    n, guard = 2 * 24 * 40, 4096
    buf = torch.full((guard + n + guard,), -7.25, dtype=torch.float32, device="cuda")
    bufs = _lib.rtm_matte_buffers()
    bufs.coverage = buf.data_ptr() + 4 * guard
    opt = r._options(0, 24)
    st = data.settings_c()
    _lib.check(_lib.lib().rtm_render_mattes(C.byref(st), r._scene_handle(), C.byref(opt), 2, C.byref(bufs), None), "mattes")
    torch.cuda.synchronize()
    assert (buf[:guard] == -7.25).all() and (buf[guard + n:] == -7.25).all()
    assert np.array_equal(_bits(buf[guard:guard + n].reshape(2, 24, 40)), _bits(full["coverage"]))
    only = _mattes(r, 2, want=("alpha",))
    assert set(only) == {"alpha"} and np.array_equal(_bits(only["alpha"]), _bits(full["alpha"]))


def test_async_on_a_side_stream_with_the_scene_destroyed_at_once(rtm, oracle):
    import torch
    from raytracingmin_amd import _lib
    data, *_ = _cornell(rtm, oracle, 96, 56, 3)
    want = _mattes(rtm.Renderer(data, mode="repaired"), 4)
    L = _lib.lib()
    st, arr, n = data.to_c()
    scene = C.c_void_p()
    _lib.check(L.rtm_scene_create(arr, n, 0, 0, C.byref(scene)), "rtm_scene_create")
    s = torch.cuda.Stream()
    out = {k: torch.full(v.shape, 3, dtype=torch.int32 if v.dtype == np.int32 else torch.float32, device="cuda")
           for k, v in want.items()}
    bufs = _lib.rtm_matte_buffers(*(out[k].data_ptr() for k in PLANES))
    torch.cuda.synchronize()
    opt = _lib.rtm_options()
    opt.mode, opt.row_begin, opt.row_end = 1, 0, data.height
    # a longer render first on the same stream, so that the matte kernel is still queued when the scene goes
    big = rtm.Renderer(rtm.LoadData(oracle.scene_path("cornellBoxSetting.json")).data, mode="repaired", max_bounces=8)
    big.data.width, big.data.height, big.data.samples, big.data.superSamples = 256, 256, 64, 2
    big.render_rows_device(want=("f32",), stats=False, stream=s.cuda_stream)
    _lib.check(L.rtm_render_mattes(C.byref(st), scene, C.byref(opt), 4, C.byref(bufs), C.c_void_p(s.cuda_stream)), "mattes")
    _lib.check(L.rtm_scene_destroy(scene), "rtm_scene_destroy")
    s.synchronize()
    for k in want:
        assert np.array_equal(_bits(out[k]), _bits(want[k])), k


def test_other_variants_and_super_samples_above_8_are_refused(rtm, oracle):
    from raytracingmin_amd import RtmError
    data, *_ = _cornell(rtm, oracle, 32, 16, 1)
    for v in (17, 2, 3, 12, 18):  # (the box has no grid)
        with pytest.raises(RtmError) as e:
            rtm.Renderer(data, mode="repaired", variant=v).render_mattes()
        assert e.value.status == -8, v
    data.superSamples = 9
    with pytest.raises(RtmError) as e:
        rtm.Renderer(data, mode="repaired").render_mattes()
    assert e.value.status == -8


# ---- rtm_matte and rtm_composite ------------------------------------------------------------------------------------------
def test_matte_equals_the_restatement(rtm, stress):
    import torch
    layers = stress["a", 8, 0]
    lid, cov = torch.from_numpy(layers["id"]).cuda(), torch.from_numpy(layers["coverage"]).cuda()
    present = [int(v) for v in np.unique(layers["id"]) if v >= 0]
    top = int(np.bincount(layers["id"][0][layers["id"][0] >= 0]).argmax())
    absent = next(i for i in range(2000) if i not in present)
    for ids in ([top], [absent], [-1], [top, top, -1, top], (present * 64)[:64], present[:5][::-1] + [absent]):
        got = rtm.matte(lid, cov, ids)
        torch.cuda.synchronize()
        want = _matte_ref.matte(layers["id"], layers["coverage"], ids)
        assert np.array_equal(_bits(got), _bits(want)), ids
    assert rtm.matte(lid, cov, [top]).max() > 0 and not rtm.matte(lid, cov, [absent, -1]).any()
    on_device = rtm.matte(lid, cov, torch.tensor(present[:7], dtype=torch.int32, device="cuda"))
    assert np.array_equal(_bits(on_device), _bits(_matte_ref.matte(layers["id"], layers["coverage"], present[:7])))
    # synthetic layers whose selected coverages sum above 1, on a frame that is no multiple of the block
    rng = np.random.default_rng(11)
    sid = rng.integers(-1, 6, (5, 19, 23)).astype(np.int32)
    scov = rng.random((5, 19, 23), dtype=np.float32)
    want = _matte_ref.matte(sid, scov, [0, 1, 2, 3, 4, 5])
    assert (want == 1.0).any() and (want < 1.0).any()
    got = rtm.matte(torch.from_numpy(sid).cuda(), torch.from_numpy(scov).cuda(), [0, 1, 2, 3, 4, 5])
    assert np.array_equal(_bits(got), _bits(want))


def test_composite_equals_the_restatement(rtm):
    import torch
    rng = np.random.default_rng(21)
    h, w = 37, 53  # no multiple of the block
    color = (rng.random((h, w, 3), dtype=np.float32) * np.float32(1.5)).astype(np.float32)  # non-negative, some above 1
    alpha = rng.integers(0, 17, (h, w)).astype(np.float32) / np.float32(16)  # sixteenths, 0 and 1 among them
    assert (alpha == 0).any() and (alpha == 1).any()
    image = rng.random((h, w, 3), dtype=np.float32)
    d_color, d_alpha, d_image = (torch.from_numpy(v).cuda() for v in (color, alpha, image))
    bg = (0.25, 0.5, 0.125)
    for background, ref_bg in ((bg, bg), (d_image, image)):
        got = rtm.composite(d_color, d_alpha, background, want=("f32", "u8"))
        want32, want8 = _matte_ref.composite(color, alpha, ref_bg)
        assert np.array_equal(_bits(got["f32"]), _bits(want32))
        assert np.array_equal(got["u8"].cpu().numpy(), want8)
        full = alpha == 1
        assert np.array_equal(_bits(got["f32"])[full], _bits(color)[full])  # alpha 1: the colour's bits
        q = np.zeros(want32.shape, np.uint8)
        v64 = np.ascontiguousarray(got["f32"].cpu().numpy().astype(np.float64))
        rtm._lib.check(rtm.lib().rtm_quantise(v64.ctypes.data, v64.size, q.ctypes.data), "rtm_quantise")
        assert np.array_equal(got["u8"].cpu().numpy(), q)  # u8 is rtm_quantise of the f32
    # a constant image is the constant colour, bit for bit
    const = torch.from_numpy(np.broadcast_to(np.asarray(bg, np.float32), (h, w, 3)).copy()).cuda()
    a, b = rtm.composite(d_color, d_alpha, const)["f32"], rtm.composite(d_color, d_alpha, bg)["f32"]
    assert np.array_equal(_bits(a), _bits(b))
    # in place, and the u8 alone
    work = d_color.clone()
    out = rtm.composite(work, d_alpha, bg, want=("f32",), out_f32=work)
    assert out["f32"] is work and np.array_equal(_bits(work), _bits(b))
    only8 = rtm.composite(d_color, d_alpha, bg, want=("u8",))
    assert set(only8) == {"u8"} and np.array_equal(only8["u8"].cpu().numpy(), _matte_ref.composite(color, alpha, bg)[1])


# ---- files ----------------------------------------------------------------------------------------------------------------
def _read_pfm(path):
    raw = open(path, "rb").read()
    kind, dims, scale, body = raw.split(b"\n", 3)
    w, h = (int(v) for v in dims.split())
    assert scale == b"-1.0"
    comp = {b"PF": 3, b"Pf": 1}[kind]
    return np.frombuffer(body, dtype="<f4").reshape(h, w, comp)[::-1].squeeze(-1 if comp == 1 else ())


def test_render_writes_the_matte_files_and_keeps_the_image(rtm, oracle, tmp_path):
    import torch
    path = oracle.scene_path("settingData.json")
    data = rtm.LoadData(path).data
    data.width, data.height, data.samples, data.superSamples = 48, 32, 2, 2
    r = rtm.Renderer(data, mode="repaired", max_bounces=4)
    r.Render(str(tmp_path / "plain"), tonemap=True)
    image = r.image.copy()
    planes = _mattes(r, 3)
    ids = [int(v) for v in np.unique(planes["id"]) if v >= 0][:2]
    r.Render(str(tmp_path / "with"), tonemap=True, mattes={"layers": 3, "ids": ids, "background": (0.2, 0.4, 0.8)})
    assert np.array_equal(r.image, image)
    for ext in (".jpg", ".bmp", "_display.bmp", "_display.jpg"):
        assert (tmp_path / ("plain" + ext)).read_bytes() == (tmp_path / ("with" + ext)).read_bytes(), ext
    assert np.array_equal(_bits(_read_pfm(tmp_path / "with_alpha.pfm")), _bits(planes["alpha"]))
    want = _matte_ref.matte(planes["id"], planes["coverage"], ids)
    assert np.array_equal(_bits(_read_pfm(tmp_path / "with_matte.pfm")), _bits(want)) and want.any()
    for name in ("with_matte.bmp", "with_over.bmp", "with_over_display.bmp"):
        assert (tmp_path / name).stat().st_size == 54 + 48 * 3 * 32, name
    assert (tmp_path / "with_over.jpg").stat().st_size > 0 and (tmp_path / "with_over_display.jpg").stat().st_size > 0
    over = _matte_ref.composite(image.astype(np.float32), planes["alpha"], (0.2, 0.4, 0.8))[1]
    bmp = np.frombuffer((tmp_path / "with_over.bmp").read_bytes()[54:], np.uint8).reshape(32, 48, 3)[::-1, :, ::-1]
    assert np.array_equal(bmp, over)
    assert not (tmp_path / "plain_alpha.pfm").exists()
    r.Render(str(tmp_path / "alpha"), mattes=True)  # alpha alone
    assert (tmp_path / "alpha_alpha.pfm").exists() and not (tmp_path / "alpha_matte.pfm").exists() \
        and not (tmp_path / "alpha_over.bmp").exists()
    torch.cuda.synchronize()


def test_cli_writes_the_matte_files_and_keeps_the_image(rtm, oracle, tmp_path):
    scene = oracle.scene_path("settingData.json")
    args = [CLI, "-json", scene, "--width", "48", "--height", "32", "--samples", "2", "--superSamples", "2", "--max-bounces", "4"]
    run = lambda *flags: subprocess.run(args + list(flags), cwd=tmp_path, capture_output=True, text=True, timeout=300)
    p = run("--out", "plain", "--display")
    assert p.returncode == 0, p.stderr
    data = rtm.LoadData(scene).data
    data.width, data.height, data.samples, data.superSamples = 48, 32, 2, 2
    r = rtm.Renderer(data, mode="repaired", max_bounces=4)
    planes = _mattes(r, 3)
    ids = [int(v) for v in np.unique(planes["id"]) if v >= 0][:2]
    p = run("--out", "result", "--display", "--alpha", "--matte", ",".join(str(i) for i in ids), "--matte-layers", "3",
            "--background", "0.2,0.4,0.8")
    assert p.returncode == 0, p.stderr
    for word in ("result_alpha.pfm", "result_matte.pfm", "result_matte.bmp", "result_over.bmp", "result_over.jpg",
                 "result_over_display.bmp"):
        assert word in p.stdout and (tmp_path / word).stat().st_size > 0, word
    assert (tmp_path / "result_over_display.jpg").stat().st_size > 0
    for ext in (".bmp", ".jpg", "_display.bmp", "_display.jpg"):
        assert (tmp_path / ("plain" + ext)).read_bytes() == (tmp_path / ("result" + ext)).read_bytes(), ext
    assert np.array_equal(_bits(_read_pfm(tmp_path / "result_alpha.pfm")), _bits(planes["alpha"]))
    assert np.array_equal(_bits(_read_pfm(tmp_path / "result_matte.pfm")), _bits(_matte_ref.matte(planes["id"], planes["coverage"], ids)))
    # the Python writer gives the same files
    r.Render(str(tmp_path / "py"), tonemap=True, mattes={"layers": 3, "ids": ids, "background": (0.2, 0.4, 0.8)})
    for k in ("alpha.pfm", "matte.pfm", "matte.bmp", "over.bmp", "over.jpg", "over_display.bmp", "over_display.jpg"):
        assert (tmp_path / f"py_{k}").read_bytes() == (tmp_path / f"result_{k}").read_bytes(), k
    p = run("--out", "a", "--alpha")  # alone: one more file
    assert p.returncode == 0 and (tmp_path / "a_alpha.pfm").exists() and not (tmp_path / "a_matte.pfm").exists() \
        and not (tmp_path / "a_over.bmp").exists()
