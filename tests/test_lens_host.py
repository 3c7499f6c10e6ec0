"""Lens, the parts that need no GPU: the bindings and the struct layout, rtm_lens's argument checks (all made before any device
call), the fold-over check and rtm_lens_fit_zoom against the NumPy reference, the Python entry points' argument errors, the
CLI's refusals, and self-checks of the reference."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _lens_ref
import _resize_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
SCENE = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
FILTERS, MODES = _lens_ref.FILTERS, _lens_ref.MODES
# the five lenses of the zoom fit: the defaults, a barrel, a pincushion with chromatic aberration, and two INVERSE ones
FIT_SETS = [dict(), dict(k1=-0.2, k2=0.03), dict(k1=0.15, chroma=0.01), dict(k1=-0.2, k2=0.03, chroma=0.01, mode="inverse"),
            dict(k1=0.3, k2=-0.05, chroma=-0.02, mode="inverse")]
FIT_SIZES = [(7, 5), (67, 35), (1920, 1080)]


def _header():
    return open(os.path.join(ROOT, "include", "rtm.h")).read()


def _params(channels=3, **kw):
    """An rtm_lens_params straight from the values, with no check of the package's in between."""
    from raytracingmin_amd import _lib
    p = _lens_ref.with_defaults(kw)
    prm = _lib.rtm_lens_params()
    for name in ("k1", "k2", "zoom", "chroma", "vignette", "falloff"):
        setattr(prm, name, p[name])
    words = _lens_ref.border_words(p["border"])
    C.memmove(prm.border, words.ctypes.data, 12)
    prm.mode = p["mode"] if isinstance(p["mode"], int) else MODES.index(p["mode"])
    prm.filter = p["filter"] if isinstance(p["filter"], int) else FILTERS.index(p["filter"])
    prm.channels = channels
    return prm


def test_lens_is_bound_and_exported_and_the_struct_matches_the_header():
    import raytracingmin_amd as rtm
    from raytracingmin_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("rtm_lens", "rtm_lens_fit_zoom"):
        assert name in _lib.SIGNATURES and hasattr(raw, name)
    header = _header()
    body = re.search(r"typedef struct rtm_lens_params \{(.*?)\} rtm_lens_params;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for decl in body.split(";"):
        if decl.strip():
            ty, names = decl.split(None, 1)
            for n in names.split(","):
                n = n.strip()
                declared.append(("border", C.c_float * 3) if n == "border[3]" else (n, {"float": C.c_float, "int32_t": C.c_int32}[ty]))
    want = [("k1", C.c_float), ("k2", C.c_float), ("zoom", C.c_float), ("chroma", C.c_float), ("vignette", C.c_float),
            ("falloff", C.c_float), ("border", C.c_float * 3), ("mode", C.c_int32), ("filter", C.c_int32), ("channels", C.c_int32)]
    assert [(f[0], f[1]) for f in _lib.rtm_lens_params._fields_] == declared == want
    assert C.sizeof(_lib.rtm_lens_params) == 48
    res, args = _lib.SIGNATURES["rtm_lens"]
    assert res is C.c_int and len(args) == 8 and args[1:4] == [C.c_int32, C.c_int32, C.c_int]
    assert _lib.SIGNATURES["rtm_lens_fit_zoom"][0] is C.c_int and len(_lib.SIGNATURES["rtm_lens_fit_zoom"][1]) == 4
    # the header, the package, the reference: one enum order and one set of defaults
    enum = re.search(r"enum \{ (RTM_LENS_NEAREST[^}]*) \};", header).group(1)
    assert [e.strip() for e in enum.split(",")] == [f"RTM_LENS_{n.upper()} = {i}" for i, n in enumerate(FILTERS)]
    enum = re.search(r"enum \{ (RTM_LENS_DIRECT[^}]*) \};", header).group(1)
    assert [e.strip() for e in enum.split(",")] == [f"RTM_LENS_{n.upper()} = {i}" for i, n in enumerate(MODES)]
    assert re.search(r"#define RTM_LENS_DEFAULTS \{0\.0f, 0\.0f, 1\.0f, 0\.0f, 0\.0f, 1\.0f, \{0\.0f, 0\.0f, 0\.0f\}, RTM_LENS_DIRECT, "
                     r"RTM_LENS_BICUBIC, 3\}", header)
    assert rtm.LENS_FILTERS == _lib.LENS_FILTERS == FILTERS == ("nearest", "bilinear", "bicubic")
    assert rtm.LENS_MODES == _lib.LENS_MODES == MODES == ("direct", "inverse")
    assert rtm.LENS_DEFAULTS == _lib.LENS_DEFAULTS == _lens_ref.DEFAULTS == {
        "k1": 0.0, "k2": 0.0, "zoom": 1.0, "chroma": 0.0, "vignette": 0.0, "falloff": 1.0, "border": 0.0, "mode": "direct",
        "filter": "bicubic"}
    for name in ("lens", "lens_fit_zoom", "LENS_DEFAULTS", "LENS_FILTERS", "LENS_MODES"):
        assert name in rtm.__all__ and hasattr(rtm, name)
    params = inspect.signature(rtm.lens).parameters
    assert list(params) == ["color", "k1", "k2", "zoom", "chroma", "vignette", "falloff", "border", "mode", "filter", "want", "stream"]
    assert {k: params[k].default for k in rtm.LENS_DEFAULTS} == rtm.LENS_DEFAULTS
    assert params["want"].default == ("f32",) and params["stream"].default is None
    assert list(inspect.signature(rtm.lens_fit_zoom).parameters) == ["width", "height", "params"]
    assert inspect.signature(rtm.Renderer.Render).parameters["lens"].default is None
    assert list(inspect.signature(rtm.Renderer.write_lens).parameters) == ["self", "fileName", "frame", "params"]
    assert _lib.lib().rtm_abi_version() == 5  # added without a bump
    assert re.search(r"#define RTM_ABI_VERSION 5\b", header)


def test_lens_rejects_invalid_arguments_without_a_gpu():
    from raytracingmin_amd import _lib
    L = _lib.lib()
    src, out32, out8 = C.c_void_p(0x1000), C.c_void_p(0x300000), C.c_void_p(0x4000000)
    # fake device pointers: never dereferenced, every call below fails its checks first

    def call(p={}, channels=3, w=8, h=6, dev=0, s=src, o32=out32, o8=out8):
        prm = None if p is None else C.byref(_params(channels, **p))
        return L.rtm_lens(prm, w, h, dev, s, o32, o8, None)

    def detail():
        return L.rtm_last_error_detail()

    nan, inf = float("nan"), float("inf")
    assert call(p=None) == -1 and b"params" in detail()
    assert call(s=None) == -1 and b"src_dev" in detail()
    assert call(o32=None, o8=None) == -1 and b"out_f32_dev" in detail() and b"out_u8_dev" in detail()
    for kw in (dict(w=0), dict(h=0), dict(w=-1), dict(h=-3)):
        assert call(**kw) == -1 and b"size" in detail(), kw
    # a NaN, infinite or out-of-range parameter: just past either end of every range
    for name, (lo, hi) in _lens_ref.RANGES.items():
        for v in (nan, inf, -inf, np.nextafter(np.float32(lo), np.float32(-9)), np.nextafter(np.float32(hi), np.float32(9))):
            assert call(p={name: v}) == -1 and name.encode() in detail(), (name, v)
    for v in (nan, inf, -inf):  # a non-finite border with a filter other than NEAREST
        for f in ("bilinear", "bicubic"):
            for k in range(3):
                b = [0.0, 0.0, 0.0]
                b[k] = v
                assert call(p=dict(border=b, filter=f)) == -1 and b"border" in detail(), (v, f, k)
    for v in (-1, 2, 1 << 30):
        assert call(p=dict(mode=v)) == -1 and b"mode" in detail(), v
    for v in (-1, 3, 1 << 30):
        assert call(p=dict(filter=v)) == -1 and b"filter" in detail(), v
    for v in (0, 2, 4, -1):
        assert call(channels=v) == -1 and b"channels" in detail(), v
    assert call(p=dict(chroma=0.01), channels=1) == -1 and b"chroma" in detail()
    assert call(p=dict(chroma=0.01, filter="nearest")) == -1 and b"NEAREST" in detail()
    assert call(p=dict(vignette=0.5, filter="nearest")) == -1 and b"NEAREST" in detail()
    for name in ("s", "o32"):  # a float pointer that is not 4-byte aligned
        for off in (1, 2, 3):
            assert call(**{name: C.c_void_p(0x600000 + off)}) == -1 and b"4-byte" in detail(), (name, off)
    for name in ("o32", "o8"):  # a gather cannot run in place
        assert call(**{name: src}) == -1 and b"src_dev" in detail() and b"in place" in detail(), name
    assert call(dev=-1) == -1 and b"device" in detail()
    assert call(p=dict(k1=-0.5), dev=-1) == -1 and b"folds over" in detail()  # a radial map that folds over
    # a frame of 2^31 pixels or more, and the launch's tile limit: RTM_ERR_UNSUPPORTED
    assert call(w=1 << 16, h=1 << 15) == -8 and b"2^31 pixels" in detail()
    assert call(w=1, h=1 << 26) == -8 and b"2^24 tiles" in detail()
    assert call(w=1 << 30, h=1) == -8 and b"2^24 tiles" in detail()
    # the limits themselves, single outputs, an odd u8 pointer, a NaN border and the word of -1 with NEAREST pass every check:
    # what refuses these is the device
    minus_one = np.array([-1], np.int32).view(np.float32)[0]
    assert np.isnan(minus_one)
    for kw in (dict(p=dict(k1=0.5, k2=0.25, zoom=4.0, chroma=0.05, vignette=1.0, falloff=4.0)),
               dict(p=dict(k1=0.5, k2=-0.25, zoom=4.0, chroma=-0.05, falloff=0.0)), dict(p=dict(zoom=0.25)),
               dict(p=dict(filter="nearest", border=minus_one), channels=1), dict(p=dict(filter="nearest", border=[nan, inf, -inf])),
               dict(p=dict(mode="inverse", filter="bilinear"), channels=1), dict(o32=None), dict(o8=None),
               dict(o8=C.c_void_p(0x4000001)), dict(w=1, h=1), dict(w=(1 << 16) - 1, h=1 << 15), dict(w=1, h=(1 << 26) - 4),
               dict(w=(1 << 30) - 64, h=1), dict(s=C.c_void_p(0x1004), o32=C.c_void_p(0x300008))):
        assert call(dev=-1, **kw) == -1, kw
        assert b"device" in detail(), kw


def test_the_fold_over_check_matches_the_reference_on_a_grid():
    from raytracingmin_amd import _lib
    L = _lib.lib()
    src, out32 = C.c_void_p(0x1000), C.c_void_p(0x300000)
    seen = {True: 0, False: 0}
    k1s = np.unique(np.concatenate([np.linspace(-0.5, 0.5, 11), [-0.26, -0.25, -0.24]]))
    k2s = np.unique(np.concatenate([np.linspace(-0.25, 0.25, 11), [0.01, 0.03]]))
    for mode in MODES:
        for zoom in (0.25, 0.5, 0.75, 1.0, 1.25, 2.0, 4.0):
            for k1 in k1s:
                for k2 in k2s:
                    want = _lens_ref.folds_over(k1, k2, zoom, mode)
                    assert (_lens_ref.refused(3, k1=k1, k2=k2, zoom=zoom, mode=mode) == "folds over") == want
                    rc = L.rtm_lens(C.byref(_params(k1=k1, k2=k2, zoom=zoom, mode=mode)), 8, 6, -1, src, out32, None, None)
                    detail = L.rtm_last_error_detail()
                    assert rc == -1 and (b"folds over" in detail) == want and (b"device" in detail) != want, (mode, zoom, k1, k2)
                    seen[want] += 1
    assert seen[True] >= 100 and seen[False] >= 100, seen
    # the edge by hand, DIRECT at zoom 1: d(1) = 1 + 3 k1 is 0.25 at k1 = -0.25 exactly (accepted), and below it one float lower
    assert not _lens_ref.folds_over(-0.25, 0.0, 1.0, "direct")
    assert _lens_ref.folds_over(np.nextafter(np.float32(-0.25), np.float32(-1)), 0.0, 1.0, "direct")
    # the vertex inside (0, T): k1 = -0.5, k2 = 0.25 has d's minimum 1 - 2.25 / 5 = 0.55 at t = 0.6: fine at zoom 1, DIRECT
    assert not _lens_ref.folds_over(-0.5, 0.25, 1.0, "direct")
    # the vertex alone decides k1 = -1/3, k2 = 0.06 (a = -1, b = 0.3, vertex at t = 5/3 with d = 1/6): DIRECT stops at T = 1,
    # where d = 0.3; INVERSE looks as far as T = 4, where d = 1.8 and g = 0.63 are fine, and finds the vertex on its way
    assert not _lens_ref.folds_over(-1 / 3, 0.06, 1.0, "direct") and _lens_ref.folds_over(-1 / 3, 0.06, 1.0, "inverse")


@pytest.mark.parametrize("size", FIT_SIZES, ids=[f"{w}x{h}" for w, h in FIT_SIZES])
def test_fit_zoom_matches_the_reference_bit_for_bit(size):
    import raytracingmin_amd as rtm
    w, h = size
    for prm in FIT_SETS:
        want = _lens_ref.fit_zoom(w, h, **prm)
        got = rtm.lens_fit_zoom(w, h, **prm)
        print(f"{w}x{h} {prm}: zoom {got!r}")
        assert want is not None and np.float32(got).view(np.uint32) == np.float32(want).view(np.uint32), (prm, got, want)
        assert 0.25 <= got <= 4.0 and rtm.lens_fit_zoom(w, h, zoom=3.0, **prm) == got  # params' zoom is ignored
        # the reference has no border pixel anywhere in the frame at the returned zoom, and the lens is one rtm_lens accepts
        assert _lens_ref.refused(3, zoom=got, **prm) is None
        assert _lens_ref.positions(w, h, 3, zoom=got, **prm)[2].all(), prm
        if got > 0.25:  # and it is the bisection's boundary: one per cent less zoom shows the border or folds over
            assert not _lens_ref.hides_border(w, h, np.float32(got * 0.99), **prm), prm
    assert rtm.lens_fit_zoom(w, h, channels=1, k1=0.15) == float(_lens_ref.fit_zoom(w, h, 1, k1=0.15))


def test_fit_zoom_refusals():
    import raytracingmin_amd as rtm
    from raytracingmin_amd import _lib
    L = _lib.lib()
    z = C.c_float(-7.0)

    def call(w=67, h=35, channels=3, out=z, **kw):
        return L.rtm_lens_fit_zoom(C.byref(_params(channels, **kw)), w, h, C.byref(out) if out is not None else None)

    # where P(4) fails: a pincushion beyond zoom 4's reach, and a barrel that folds over even there
    for kw in (dict(k1=100.0), dict(k1=-10.0), dict(k1=-10.0, mode="inverse"), dict(k1=0.0, k2=-1000.0)):
        assert _lens_ref.fit_zoom(67, 35, **kw) is None
        assert call(**kw) == -8 and b"zoom" in L.rtm_last_error_detail(), kw
        with pytest.raises(rtm.RtmError):
            rtm.lens_fit_zoom(67, 35, **kw)
    assert z.value == -7.0  # a refusal writes nothing
    assert L.rtm_lens_fit_zoom(None, 8, 6, C.byref(z)) == -1 and call(out=None) == -1
    for kw in (dict(w=0), dict(h=0), dict(w=-2), dict(k1=float("nan")), dict(k2=float("inf")), dict(chroma=float("nan")),
               dict(mode=2), dict(mode=-1), dict(channels=2), dict(channels=1, chroma=0.01)):
        assert call(**kw) == -1, kw
    assert call(w=1 << 16, h=1 << 15) == -8
    # what it does not read does not matter: vignette, falloff, border, filter, zoom
    assert call(vignette=7.0, falloff=-1.0, border=float("nan"), filter=9, zoom=float("nan"), k1=0.15) == 0
    assert z.value == float(_lens_ref.fit_zoom(67, 35, k1=0.15))
    for bad in (dict(k1="x"), dict(k1=float("nan")), dict(mode="both"), dict(channels=2), dict(unknown=1), dict(channels=1, chroma=0.01)):
        with pytest.raises(ValueError):
            rtm.lens_fit_zoom(67, 35, **bad)
    for bad in ((0, 5), (5, 0), (5.0, 5), (True, 5), (1 << 31, 5)):
        with pytest.raises(ValueError):
            rtm.lens_fit_zoom(*bad)


def test_python_argument_errors_raise_before_any_device_use():
    import raytracingmin_amd as rtm
    color = np.zeros((4, 4, 3), np.float32)  # not even a tensor: a bad parameter comes first
    nan = float("nan")
    for kw in (dict(k1=0.6), dict(k1=nan), dict(k1="0.1"), dict(k1=True), dict(k2=-0.3), dict(zoom=0.2), dict(zoom=5), dict(zoom="auto"),
               dict(chroma=0.06), dict(vignette=-0.1), dict(vignette=1.5), dict(falloff=4.5), dict(falloff=nan), dict(border=nan),
               dict(border=(0, 0)), dict(border="black"), dict(border=(0, float("inf"), 0), filter="bilinear"), dict(mode="undistort"),
               dict(mode=1), dict(filter="lanczos3"), dict(filter=2), dict(filter="nearest", chroma=0.01),
               dict(filter="nearest", vignette=0.5), dict(k1=-0.5), dict(k1=-0.3, mode="inverse"), dict(want=()), dict(want=("f64",))):
        with pytest.raises(ValueError):
            rtm.lens(color, **kw)
    with pytest.raises(ValueError):
        rtm.lens(np.zeros((4, 4), np.float32), chroma=0.01)  # a plane has no colours to separate
    data = rtm.LoadData(SCENE).data
    data.width, data.height = 16, 12
    for bad in ("barrel", 0.1, (0.1,), dict(k3=0.1), dict(k1=0.9), dict(zoom="fit"), dict(k1=-0.5), dict(filter="nearest", chroma=0.01)):
        with pytest.raises(ValueError):
            rtm.Renderer(data).Render("unused", lens=bad)
        assert not os.path.exists("unused.bmp") and not os.path.exists("unused_lens.bmp")
    with pytest.raises(ValueError, match="mattes"):
        rtm.Renderer(data).Render("unused", lens=dict(k1=0.1), mattes=True)
    for bad in (dict(k1=0.9), dict(zoom="fit"), dict(k3=1)):
        with pytest.raises(ValueError):
            rtm.Renderer(data).write_lens("unused", **bad)
    assert not os.path.exists("unused.bmp") and not os.path.exists("unused_lens.bmp")


REFUSALS = [
    (["--lens-inverse"], "require the lens stage"),
    (["--lens-filter", "bilinear"], "require the lens stage"),
    (["--lens"], "--lens takes"),
    (["--lens", "0.6"], "--lens takes"),
    (["--lens", "0.1,0.3"], "--lens takes"),
    (["--lens", "0.1,0.1,0.1"], "--lens takes"),
    (["--lens", "nan"], "--lens takes"),
    (["--lens", "barrel"], "--lens takes"),
    (["--lens-ca", "0.06"], "--lens-ca takes"),
    (["--lens-ca", "0.01,0.01"], "--lens-ca takes"),
    (["--lens-ca"], "--lens-ca takes"),
    (["--lens-vignette", "1.5"], "--lens-vignette takes"),
    (["--lens-vignette", "0.5,5"], "--lens-vignette takes"),
    (["--lens-vignette", "-0.1"], "--lens-vignette takes"),
    (["--lens-zoom", "0.2"], "--lens-zoom takes"),
    (["--lens-zoom", "5"], "--lens-zoom takes"),
    (["--lens-zoom", "fit"], "--lens-zoom takes"),
    (["--lens-zoom"], "--lens-zoom takes"),
    (["--lens", "0.1", "--lens-filter"], "--lens-filter takes"),
    (["--lens", "0.1", "--lens-filter", "bicubic2"], "--lens-filter takes"),
    (["--lens", "0.1", "--lens-filter", "Nearest"], "--lens-filter takes"),
    (["--lens", "0.1", "--gpus", "2"], "one GPU"),
    (["--lens-ca", "0.01", "--virtual-strips", "2"], "one GPU"),
    (["--lens-vignette", "0.5", "--force-rccl"], "one GPU"),
    (["--lens-zoom", "auto", "--preview", "2", "--preview-only"], "--preview-only"),
    (["--lens", "0.1", "--alpha"], "--alpha, --matte or --background"),
    (["--lens", "0.1", "--matte", "1"], "--alpha, --matte or --background"),
    (["--lens", "0.1", "--background", "0,0,0"], "--alpha, --matte or --background"),
    (["--lens-ca", "0.01", "--lens-filter", "nearest"], "nearest copies words"),
    (["--lens", "0.1", "--lens-vignette", "0.5", "--lens-filter", "nearest"], "nearest copies words"),
]


@pytest.mark.parametrize("flags,word", REFUSALS, ids=[" ".join(f) for f, _ in REFUSALS])
def test_cli_refuses_before_any_gpu(tmp_path, flags, word):
    r = subprocess.run([CLI, "-json", SCENE, "--width", "8", "--height", "8", "--out", "x"] + flags, cwd=tmp_path,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (flags, r.stdout, r.stderr)
    assert word in r.stderr and "--lens" in r.stderr and len(r.stderr.strip().splitlines()) == 1, (flags, r.stderr)
    assert not (tmp_path / "x.bmp").exists() and not (tmp_path / "x_lens.bmp").exists()


def test_cli_usage_mentions_lens():
    r = subprocess.run([CLI, "-?"], capture_output=True, text=True, timeout=60)
    for word in ("--lens K1[,K2]", "--lens-inverse", "--lens-ca X", "--lens-vignette A[,F]", "--lens-zoom Z|auto",
                 "--lens-filter nearest|bilinear|bicubic", "STEM_lens.bmp"):
        assert word in r.stdout + r.stderr, word
    head = open(os.path.join(ROOT, "raytracingmin_amd", "csrc", "rtm_main.cpp")).read().split("#include", 1)[0]
    for word in ("[--lens K1[,K2]]", "[--lens-inverse]", "[--lens-ca X]", "[--lens-vignette A[,F]]", "[--lens-zoom Z|auto]",
                 "[--lens-filter nearest|bilinear|bicubic]"):
        assert word in head, word


# ---- the NumPy reference itself -------------------------------------------------------------------------------------
def test_reference_defaults_are_the_identity_in_both_modes_and_all_filters():
    for c in (1, 3):
        for src in (_resize_ref.frame(7, 5, c), _resize_ref.frame(67, 35, c), _resize_ref.holes_frame(c)):
            h, w = src.shape[:2]
            ok = _lens_ref.counts(src)
            for mode in MODES:
                u, v, inside, _ = _lens_ref.positions(w, h, c, mode=mode)
                Y, X = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
                assert inside.all() and np.array_equal(u, np.broadcast_to(X[..., None], u.shape)), (c, mode)  # u = X exactly
                assert np.array_equal(v, np.broadcast_to(Y[..., None], v.shape)), (c, mode)
                for f in FILTERS:
                    out = _lens_ref.lens_ref(src, mode=mode, filter=f)["out"]
                    if f == "nearest":  # every word, the NaNs' included
                        assert np.array_equal(out.view(np.uint32), src.view(np.uint32)), (c, mode)
                    else:
                        assert np.array_equal(out[ok], src.astype(np.float64)[ok]), (c, mode, f)
                        assert np.all(np.isnan(out.reshape(h, w, -1)[~ok])), (c, mode, f)


def test_reference_inverse_solve_residual_and_round_trip():
    """|rho g(rho^2) - r| <= 1e-12 after the 12 steps, over 10 000 accepted random lenses x 200 radii in [0, iz]; and
    DIRECT then INVERSE returns the radius within 1e-12 (zoom 1, wherever both modes accept the lens)."""
    rng = np.random.default_rng(20261020)
    n, pairs, worst, worst_trip = 0, 0, 0.0, 0.0
    while n < 10000:
        k1, k2, zoom = rng.uniform(-0.5, 0.5), rng.uniform(-0.25, 0.25), rng.uniform(0.25, 4.0)
        if _lens_ref.refused(3, k1=k1, k2=k2, zoom=zoom, mode="inverse") is not None:
            continue
        n += 1
        k1f, k2f, iz = _lens_ref.f32(k1), _lens_ref.f32(k2), 1.0 / _lens_ref.f32(zoom)
        r = np.linspace(0.0, iz, 200)
        rho = _lens_ref.solve_inverse(r, k1f, k2f)
        res = float(np.max(np.abs(rho * (1.0 + rho * rho * (k1f + rho * rho * k2f)) - r)))
        assert res <= 1e-12, (k1, k2, zoom, res)
        worst = max(worst, res)
        if _lens_ref.refused(3, k1=k1, k2=k2, mode="inverse") is None and _lens_ref.refused(3, k1=k1, k2=k2) is None:
            pairs += 1
            p = np.linspace(0.0, 1.0, 200)
            back = _lens_ref.solve_inverse(p * (1.0 + p * p * (k1f + p * p * k2f)), k1f, k2f)
            trip = float(np.max(np.abs(back - p)))
            assert trip <= 1e-12, (k1, k2, trip)
            worst_trip = max(worst_trip, trip)
    print(f"{n} lenses: worst residual {worst:.3e}; {pairs} round trips: worst {worst_trip:.3e}")
    assert pairs >= 1000


def test_reference_direct_then_inverse_is_the_identity_map_on_a_frame():
    """The positions of INVERSE, fed through DIRECT's polynomial, come back to the pixel: the two maps are inverse functions."""
    w, h = 67, 35
    k1, k2 = -0.2, 0.03
    u, v, inside, _ = _lens_ref.positions(w, h, 1, k1=k1, k2=k2, mode="inverse")
    cx, cy = w / 2.0, h / 2.0
    sx, sy = u[..., 0] + 0.5 - cx, v[..., 0] + 0.5 - cy  # where INVERSE looks, as an offset from the centre
    t = (sx * sx + sy * sy) / (cx * cx + cy * cy)
    g = 1.0 + t * (_lens_ref.f32(k1) + t * _lens_ref.f32(k2))
    Y, X = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    assert np.max(np.abs(sx * g - (X + 0.5 - cx))) <= 1e-9 and np.max(np.abs(sy * g - (Y + 0.5 - cy))) <= 1e-9


def test_reference_constant_frame_border_and_nearest_words():
    for c in (1, 3):
        src = np.full((35, 67, 3), 2.75, np.float32)[..., :c].reshape((35, 67, 3) if c == 3 else (35, 67)).copy()
        for prm in (dict(k1=0.15), dict(k1=-0.2, k2=0.03, mode="inverse"), dict(zoom=0.5)):
            for f in ("bilinear", "bicubic"):
                r = _lens_ref.lens_ref(src, border=-3.0, filter=f, **prm)
                out, inside = r["out"].reshape(35, 67, c), r["inside"]
                assert 0 < inside.sum() < inside.size, (c, prm)  # each of these has a border
                assert np.max(np.abs(out[inside] - 2.75)) <= 1e-6 and np.all(out[~inside] == -3.0), (c, prm, f)
                assert float(np.nanmin(r["D"])) >= 0.25  # every per-axis sum of a counting frame is 0.5 or more
    ids = np.arange(35 * 67, dtype=np.int32).reshape(35, 67).view(np.float32)
    minus_one = np.array([-1], np.int32).view(np.float32)[0]
    r = _lens_ref.lens_ref(ids, zoom=0.5, filter="nearest", border=minus_one)
    words = r["out"].view(np.int32)
    assert np.all(words[~r["inside"][..., 0]] == -1) and set(np.unique(words[r["inside"][..., 0]])) <= set(range(35 * 67))
    # the vignette: gain 1 at the centre of an odd frame, 1 - vignette (1 - 1 / (1 + f^2 rv)^2) towards the corner
    one = np.ones((5, 7), np.float32)
    out = _lens_ref.lens_ref(one, vignette=0.5, falloff=1.5, filter="bilinear")["out"]
    assert out[2, 3] == 1.0 and out[0, 0] == out[4, 6] == out.min() and 0.5 < out.min() < 1.0
