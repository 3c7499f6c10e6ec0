"""Depth of field, the parts that need no GPU: the bindings and the struct layout, rtm_defocus's argument checks (all made
before any device call), the Python entry points' argument errors, the CLI's refusals, and self-checks of the NumPy
reference."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _defocus_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
SCENE = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
FIELDS = ("focus_distance", "aperture", "max_radius")
TOL = 1e-4  # include/rtm.h's bar
# (zf, A, R): test_defocus_gpu.py's cases, one or more per R class
CASES = ((4.0, 0.0, 4), (4.0, 3.0, 4), (4.0, 12.0, 16), (1.0, 6.0, 8), (9.0, 40.0, 16), (4.0, 1.0, 1))


def _header():
    return open(os.path.join(ROOT, "include", "rtm.h")).read()


def test_defocus_is_bound_and_exported_and_the_struct_matches_the_header():
    import raytracingmin_amd as rtm
    from raytracingmin_amd import _lib
    assert "rtm_defocus" in _lib.SIGNATURES
    assert hasattr(C.CDLL(_lib.LIB_PATH), "rtm_defocus")
    header = _header()
    ctype = {"int32_t": C.c_int32, "float": C.c_float}
    body = re.search(r"typedef struct rtm_defocus_params \{(.*?)\} rtm_defocus_params;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for decl in body.split(";"):
        if decl.strip():
            ty, names = decl.split(None, 1)
            declared += [(n.strip(), ctype[ty]) for n in names.split(",")]
    assert [(f[0], f[1]) for f in _lib.rtm_defocus_params._fields_] == declared
    assert tuple(f[0] for f in _lib.rtm_defocus_params._fields_) == FIELDS
    assert C.sizeof(_lib.rtm_defocus_params) == 12
    # the header, the package, the reference: one set of defaults, and none for the focus distance
    macro = re.search(r"#define RTM_DEFOCUS_DEFAULTS \{([^}]*)\}", header).group(1)
    assert [v.strip() for v in macro.split(",")] == ["0.0f", "4.0f", "8"]
    assert rtm.DEFOCUS_DEFAULTS == _lib.DEFOCUS_DEFAULTS == _defocus_ref.DEFAULTS == {"aperture": 4.0, "max_radius": 8}
    assert callable(rtm.defocus) and "defocus" in rtm.__all__ and "DEFOCUS_DEFAULTS" in rtm.__all__
    params = inspect.signature(rtm.defocus).parameters
    assert list(params) == ["color", "depth", "focus_distance", "aperture", "max_radius", "want", "stream"]
    assert params["focus_distance"].default is inspect.Parameter.empty
    assert {k: params[k].default for k in rtm.DEFOCUS_DEFAULTS} == rtm.DEFOCUS_DEFAULTS
    assert params["want"].default == ("f32",) and params["stream"].default is None
    assert inspect.signature(rtm.Renderer.Render).parameters["dof"].default is None
    assert inspect.signature(rtm.Renderer.focus_distance).parameters["pixel"].default is None
    assert _lib.lib().rtm_abi_version() == 5  # added without a bump
    assert re.search(r"#define RTM_ABI_VERSION 5\b", header)


def test_defocus_rejects_invalid_arguments_without_a_gpu():
    from raytracingmin_amd import _lib
    L = _lib.lib()
    good = (4.0, 4.0, 8)
    color, depth, out32, out8, coc = (C.c_void_p(0x1000), C.c_void_p(0x20000), C.c_void_p(0x300000), C.c_void_p(0x4000000),
                                      C.c_void_p(0x50000000))
    # fake device pointers: never dereferenced, every call below fails its checks first

    def call(p=good, w=8, h=8, dev=0, c=color, z=depth, o32=out32, o8=out8, s=coc):
        prm = None if p is None else C.byref(_lib.rtm_defocus_params(*p))
        return L.rtm_defocus(prm, w, h, dev, c, z, o32, o8, s, None)

    def with_(**kw):
        d = dict(zip(FIELDS, good))
        d.update(kw)
        return tuple(d[k] for k in FIELDS)

    def detail():
        return L.rtm_last_error_detail()

    assert call(p=None) == -1 and b"params" in detail()
    assert call(c=None) == -1 and b"color_dev" in detail()
    assert call(z=None) == -1 and b"depth_dev" in detail()
    assert call(o32=None, o8=None, s=None) == -1 and b"output" in detail()
    for w, h in ((0, 8), (8, 0), (-1, 8), (8, -3)):
        assert call(w=w, h=h) == -1 and b"size" in detail(), (w, h)
    for v in (float("nan"), float("inf"), float("-inf"), 0.0, -0.0, -1.0, -1e-30):
        assert call(p=with_(focus_distance=v)) == -1 and b"focus_distance" in detail(), v
    for v in (float("nan"), float("inf"), float("-inf"), -1.0, -1e-30):
        assert call(p=with_(aperture=v)) == -1 and b"aperture" in detail(), v
    for v in (0, 17, -1, 1 << 30):
        assert call(p=with_(max_radius=v)) == -1 and b"max_radius" in detail(), v
    for name in ("c", "z", "o32", "s"):  # a float pointer that is not 4-byte aligned
        for off in (1, 2, 3):
            assert call(**{name: C.c_void_p(0x600000 + off)}) == -1 and b"4-byte" in detail(), (name, off)
    for src in (color, depth):  # a gather cannot run in place
        for name in ("o32", "o8", "s"):
            assert call(**{name: src}) == -1, name
            assert b"color_dev" in detail() and b"depth_dev" in detail() and b"in place" in detail()
    assert call(s=out32) == -1 and b"coc_out_dev" in detail()
    assert call(dev=-1) == -1 and b"device" in detail()
    # a frame of 2^31 pixels or more
    assert call(w=1 << 16, h=1 << 15) == -8  # RTM_ERR_UNSUPPORTED
    assert b"too large" in detail()
    # 2^23 tiles of 32 x 16 or more: a frame thinner than a tile reaches the launch's 2^32 lanes before 2^31 pixels
    for w, h in ((1, 1 << 27), (1 << 28, 1), (15, 1 << 27), (1 << 28, 7)):
        assert call(w=w, h=h) == -8 and b"too large" in detail() and b"tiles" in detail(), (w, h)
    # the limits themselves, single outputs and an odd u8 pointer pass every check: what refuses these is the device
    for kw in (dict(p=with_(aperture=0.0)), dict(p=with_(max_radius=1)), dict(p=with_(max_radius=16)),
               dict(p=with_(focus_distance=1e-30)), dict(p=with_(focus_distance=3e38, aperture=3e38)),
               dict(o32=None, o8=None), dict(o32=None, s=None), dict(o8=None, s=None), dict(o8=C.c_void_p(0x4000001)),
               dict(w=(1 << 16) - 1, h=1 << 15), dict(w=1, h=1), dict(w=1, h=(1 << 27) - 16), dict(w=(1 << 28) - 32, h=1)):
        assert call(dev=-1, **kw) == -1, kw
        assert b"device" in detail(), kw


def test_python_argument_errors_raise_before_any_device_use():
    import raytracingmin_amd as rtm
    color, depth = np.zeros((4, 4, 3), np.float32), np.ones((4, 4), np.float32)  # not even tensors: a bad parameter comes first
    for kw in (dict(focus_distance=0.0), dict(focus_distance=-1.0), dict(focus_distance=float("nan")), dict(focus_distance=float("inf")),
               dict(focus_distance="near"), dict(focus_distance=None), dict(focus_distance=True), dict(focus_distance=1e-60),
               dict(aperture=-0.5), dict(aperture=float("inf")), dict(aperture=None), dict(aperture=True), dict(aperture=1e60),
               dict(max_radius=0), dict(max_radius=17), dict(max_radius=2.5), dict(max_radius=True), dict(max_radius=None),
               dict(want=()), dict(want=("f64",)), dict(want=("bloom",))):
        args = dict(focus_distance=4.0)
        args.update(kw)
        with pytest.raises(ValueError):
            rtm.defocus(color, depth, **args)
    with pytest.raises(TypeError):
        rtm.defocus(color, depth)  # the focus distance has no default
    data = rtm.LoadData(SCENE).data
    data.width, data.height = 16, 12
    r = rtm.Renderer(data)
    # the look-at point is in focus: |target - origin| in double, rounded to float; no device use
    want = float(np.float32(np.sqrt(sum((float(t) - float(o)) ** 2 for t, o in zip(data.camera.target, data.camera.origin)))))
    assert r.focus_distance() == want == 10.0
    for bad in ((16, 0), (0, 12), (-1, 0), (0, -1), (1.5, 2), (1,), (1, 2, 3), "1,2", 7, (True, 1)):
        with pytest.raises(ValueError):
            r.focus_distance(pixel=bad)
    for bad in ("soft", 1, 4.0, [1], dict(radius=3), dict(max_radius=0), dict(max_radius=17), dict(aperture=-1.0),
                dict(aperture=float("nan")), dict(focus_distance=0.0), dict(focus_distance=-2.0), dict(focus_distance=float("inf")),
                dict(focus_distance=3.0, focus_pixel=(1, 1)), dict(focus_pixel=(16, 0)), dict(focus_pixel=(0, 12)),
                dict(focus_pixel=(-1, 3)), dict(focus_pixel=3), dict(focus_pixel=(1.0, 2.0))):
        with pytest.raises(ValueError):
            rtm.Renderer(data).Render("unused", dof=bad)
        assert not os.path.exists("unused.bmp") and not os.path.exists("unused_dof.bmp")
    for bad in (dict(max_radius=17), dict(aperture=-1.0), dict(focus_distance=0.0), dict(focus_distance=2.0, focus_pixel=(1, 1)),
                dict(focus_pixel=(99, 0))):
        with pytest.raises(ValueError):
            rtm.Renderer(data).write_dof("unused", **bad)
    assert not os.path.exists("unused_dof.bmp")
    data.camera.target = data.camera.origin
    with pytest.raises(ValueError, match="target"):
        rtm.Renderer(data).focus_distance()


REFUSALS = [
    (["--dof", "--gpus", "2"], "one GPU"),
    (["--dof", "--virtual-strips", "2"], "one GPU"),
    (["--dof", "--force-rccl"], "one GPU"),
    (["--dof", "--preview", "2", "--preview-only"], "--preview-only"),
    (["--focus", "3"], "require --dof"),
    (["--focus-pixel", "1,1"], "require --dof"),
    (["--dof-radius", "4"], "require --dof"),
    (["--dof", "--focus", "3", "--focus-pixel", "1,1"], "not at both"),
    (["--dof", "--focus-pixel", "8,1"], "outside"),
    (["--dof", "--focus-pixel", "1,8"], "outside"),
    (["--dof", "-1"], "--dof takes"),
    (["--dof", "nan"], "--dof takes"),
    (["--dof", "inf"], "--dof takes"),
    (["--dof", "--focus", "0"], "--focus takes"),
    (["--dof", "--focus", "-2"], "--focus takes"),
    (["--dof", "--focus", "inf"], "--focus takes"),
    (["--dof", "--focus"], "--focus takes"),
    (["--dof", "--focus", "near"], "--focus takes"),
    (["--dof", "--dof-radius", "0"], "--dof-radius takes"),
    (["--dof", "--dof-radius", "17"], "--dof-radius takes"),
    (["--dof", "--dof-radius", "2.5"], "--dof-radius takes"),
    (["--dof", "--dof-radius"], "--dof-radius takes"),
    (["--dof", "--focus-pixel", "3"], "--focus-pixel takes"),
    (["--dof", "--focus-pixel", "1,x"], "--focus-pixel takes"),
    (["--dof", "--focus-pixel", "-1,2"], "--focus-pixel takes"),
    (["--dof", "--focus-pixel", "1.5,2"], "--focus-pixel takes"),
    (["--dof", "--focus-pixel"], "--focus-pixel takes"),
]


@pytest.mark.parametrize("flags,word", REFUSALS, ids=[" ".join(f) for f, _ in REFUSALS])
def test_cli_refuses_before_any_gpu(tmp_path, flags, word):
    r = subprocess.run([CLI, "-json", SCENE, "--width", "8", "--height", "8", "--out", "x"] + flags, cwd=tmp_path,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (flags, r.stdout, r.stderr)
    assert word in r.stderr and len(r.stderr.strip().splitlines()) == 1, (flags, r.stderr)
    assert not (tmp_path / "x.bmp").exists() and not (tmp_path / "x_dof.bmp").exists()


def test_cli_usage_mentions_dof():
    r = subprocess.run([CLI, "-?"], capture_output=True, text=True, timeout=60)
    for word in ("--dof [APERTURE]", "--focus DISTANCE", "--focus-pixel X,Y", "--dof-radius R", "STEM_dof.bmp"):
        assert word in r.stdout + r.stderr, word
    head = open(os.path.join(ROOT, "raytracingmin_amd", "csrc", "rtm_main.cpp")).read().split("#include", 1)[0]
    assert "[--dof [APERTURE]] [--focus DISTANCE | --focus-pixel X,Y] [--dof-radius R]" in head


# ---- the NumPy reference itself -------------------------------------------------------------------------------------
def test_reference_frame_recipe():
    color, depth = _defocus_ref.frame(64, 64)
    ok = _defocus_ref.counts(color, depth)
    assert (~ok).sum() == 3 and np.isnan(color[32, 0, 0]) and np.isposinf(color[63, 63, 1]) and np.isnan(depth[21, 21])
    # the NaN depth lies in the first disc; the ramp passes through 4 exactly on row 21, 8 of whose pixels no disc covers
    assert [int((depth == z).sum()) for z in (1.0, 4.0, 9.0)] == [492, 792 + 8, 183]
    assert np.all(np.isposinf(depth[:, 32:][~np.isin(depth[:, 32:], (1.0, 4.0, 9.0))]))
    assert depth[0, 0] == 2.0 and depth[63, 0] == 8.0
    for w, h in ((1, 1), (2, 1)):
        color, depth = _defocus_ref.frame(w, h)
        assert _defocus_ref.counts(color, depth).all()
    # counting: +inf depth counts; NaN, 0 and negative depths and non-finite colours do not
    c = np.ones((1, 6, 3), np.float32)
    c[0, 5, 2] = -np.inf
    z = np.array([[np.inf, np.nan, 0.0, -1.0, 1e-30, 2.0]], np.float32)
    assert _defocus_ref.counts(c, z).tolist() == [[True, False, False, False, True, False]]


def test_reference_aperture_zero_is_the_identity():
    for w, h in ((1, 1), (7, 5), (64, 64)):
        color, depth = _defocus_ref.frame(w, h)
        for R in (1, 4, 16):
            out, s = _defocus_ref.defocus_ref(color, depth, 4.0, 0.0, R)
            assert np.array_equal(out.astype(np.float32).view(np.uint32), color.view(np.uint32)), (w, h, R)
            assert np.all(s == 0.0)  # (0 times a negative number: -0 in front of the focus)


def test_reference_constant_frame_stays_constant():
    c = np.array([0.25, 3.0, 0.0], np.float32)
    for w, h in ((1, 1), (7, 5), (37, 23), (64, 64)):
        _, depth = _defocus_ref.frame(w, h)
        color = np.broadcast_to(c, (h, w, 3)).copy()
        ok = _defocus_ref.counts(color, depth)
        for zf, A, R in CASES:
            out, _ = _defocus_ref.defocus_ref(color, depth, zf, A, R)
            assert _defocus_ref.tolerance_excess(out[ok], np.broadcast_to(c.astype(np.float64), out.shape)[ok]) <= 1e-12, (w, h, zf, A, R)


def test_reference_focused_foreground_keeps_its_words_and_a_blurred_disc_changes():
    color, depth = _defocus_ref.frame(64, 64)
    ok = _defocus_ref.counts(color, depth)
    first = _defocus_ref.disc_mask(64, 64, 0) & ~_defocus_ref.disc_mask(64, 64, 1) & ~_defocus_ref.disc_mask(64, 64, 2)
    out, s = _defocus_ref.defocus_ref(color, depth, 1.0, 6.0, 8)
    kept = np.all(out.astype(np.float32).view(np.uint32) == color.view(np.uint32), axis=-1)
    assert first.sum() == 493 and kept[first].sum() == 493  # the nearest surface, in focus: nothing spreads over it
    assert np.all(s[first] == 0.0) and not kept[depth == 4.0].any()
    out, s = _defocus_ref.defocus_ref(color, depth, 9.0, 40.0, 16)
    far = depth == 9.0
    changed = np.all(out != color.astype(np.float64), axis=-1)
    assert far.sum() == 183 and changed[far].sum() == 183  # in focus, but everything in front of it spills over it
    assert np.all(s[far] == 0.0)
    # the signed radius: negative in front of the focus, positive behind it, clamped to +-R
    assert np.all(s[depth == 1.0] == -16.0) and np.all(s[depth == 4.0] == -16.0) and np.all(s[ok & np.isposinf(depth)] == 16.0)
    out, s = _defocus_ref.defocus_ref(color, depth, 4.0, 3.0, 4)
    assert np.all(s[depth == 1.0] == -4.0) and np.all(s[depth == 4.0] == 0.0) and np.all(s[ok & np.isposinf(depth)] == 3.0)
    assert np.allclose(s[depth == 9.0], 3.0 * (1 - 4.0 / 9.0), rtol=1e-15)


def test_reference_quotient_that_overflows():
    """zf / z = +inf counts as the largest float: aperture 0 stays the identity, any other aperture gives -R; never NaN."""
    color = np.ones((1, 4, 3), np.float32)
    depth = np.array([[1e-30, 1e-45, 0.5, np.inf]], np.float32)
    ok = np.ones((1, 4), bool)
    for f in (np.float64, np.float32):
        s, ia = _defocus_ref.coc(depth, ok, np.float32(3e38), 0.0, 8, f)
        assert np.all(s == 0.0) and np.all(np.isfinite(ia)), f
        s, ia = _defocus_ref.coc(depth, ok, np.float32(3e38), 4.0, 8, f)
        assert s.tolist() == [[-8.0, -8.0, -8.0, 4.0]], f
    out, s = _defocus_ref.defocus_ref(color * np.float32([[[1], [2], [3], [4]]]), depth, float(np.float32(3e38)), 0.0, 4)
    assert np.array_equal(out, np.float64([[[1] * 3, [2] * 3, [3] * 3, [4] * 3]])) and np.all(s == 0.0)


def test_reference_pixels_that_do_not_count():
    color, depth = _defocus_ref.frame(37, 23)
    ok = _defocus_ref.counts(color, depth)
    assert (~ok).sum() == 3
    out, s = _defocus_ref.defocus_ref(color, depth, 4.0, 12.0, 16)
    assert np.array_equal(out[~ok].astype(np.float32).view(np.uint32), color[~ok].view(np.uint32)) and np.all(s[~ok] == 0.0)
    assert np.all(np.isfinite(out[ok]))  # and they contribute to no other pixel: whatever finite colour they are given
    other = color.copy()
    other[~ok] = 1e6
    out2, _ = _defocus_ref.defocus_ref(other, np.where(ok, depth, np.nan).astype(np.float32), 4.0, 12.0, 16)  # counts() alike
    assert np.array_equal(out2[ok], out[ok])


def test_reference_in_float32_stays_within_the_bar():
    worst, worst_s = 0.0, 0.0
    for w, h in ((1, 1), (1, 17), (17, 1), (7, 5), (37, 23), (64, 64)):
        color, depth = _defocus_ref.frame(w, h)
        ok = _defocus_ref.counts(color, depth)
        for zf, A, R in CASES:
            out, s = _defocus_ref.defocus_ref(color, depth, zf, A, R)
            out32, s32 = _defocus_ref.defocus_ref(color, depth, zf, A, R, dtype=np.float32)
            assert out32.dtype == np.float32 and s32.dtype == np.float32
            worst = max(worst, _defocus_ref.tolerance_excess(out32[ok], out[ok]))
            worst_s = max(worst_s, _defocus_ref.tolerance_excess(s32, s))
    print(f"float32 evaluation against float64: out {worst:.3e}, coc {worst_s:.3e} (bar {TOL})")
    assert worst <= TOL and worst_s <= TOL
