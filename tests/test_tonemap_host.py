"""The display transform, the parts that need no GPU: the bindings and struct layouts, rtm_tonemap's argument checks (all made
before any device call), rtm_tonemap_work_bytes, the Python entry points' argument errors, the CLI's refusals, and
self-checks of the NumPy reference."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _tonemap_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE_MAX = C.c_size_t(-1).value
FIELDS = ("op", "transfer", "auto_exposure", "dither", "ev", "key", "white")
STATS = ("log_average", "max_luminance", "exposure", "pixels")


def _header():
    return open(os.path.join(ROOT, "include", "rtm.h")).read()


def test_tonemap_is_bound_and_exported_and_the_structs_match_the_header():
    import raytracingmin_amd as rtm
    from raytracingmin_amd import _lib
    assert "rtm_tonemap" in _lib.SIGNATURES and "rtm_tonemap_work_bytes" in _lib.SIGNATURES
    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "rtm_tonemap") and hasattr(raw, "rtm_tonemap_work_bytes")
    header = _header()
    # the structs: the header's field order and types, 28 and 16 bytes
    ctype = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float}
    for name, cls, size in (("rtm_tonemap_params", _lib.rtm_tonemap_params, 28), ("rtm_tonemap_stats", _lib.rtm_tonemap_stats, 16)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = []
        for decl in body.split(";"):
            if decl.strip():
                ty, names = decl.split(None, 1)
                declared += [(n.strip(), ctype[ty]) for n in names.split(",")]
        assert [(f[0], f[1]) for f in cls._fields_] == declared, name
        assert C.sizeof(cls) == size, name
    assert tuple(f[0] for f in _lib.rtm_tonemap_params._fields_) == FIELDS
    assert tuple(f[0] for f in _lib.rtm_tonemap_stats._fields_) == STATS
    # the enums
    for k, v in (("CLAMP", 0), ("REINHARD", 1), ("ACES", 2)):
        assert re.search(r"RTM_TONEMAP_%s = %d\b" % (k, v), header) and _lib.TONEMAP_OPS[k.lower()] == v
    for k, v in (("LINEAR", 0), ("SRGB", 1)):
        assert re.search(r"RTM_TRANSFER_%s = %d\b" % (k, v), header) and _lib.TRANSFERS[k.lower()] == v
    # the header, the package, the reference: one set of defaults
    macro = re.search(r"#define RTM_TONEMAP_DEFAULTS \{([^}]*)\}", header).group(1)
    assert [v.strip() for v in macro.split(",")] == ["RTM_TONEMAP_ACES", "RTM_TRANSFER_SRGB", "1", "1", "0.0f", "0.18f", "0.0f"]
    assert rtm.TONEMAP_DEFAULTS == _tonemap_ref.DEFAULTS == {"op": "aces", "transfer": "srgb", "exposure": "auto", "key": 0.18,
                                                             "white": 0.0, "dither": True}
    assert callable(rtm.tonemap) and "tonemap" in rtm.__all__ and "TONEMAP_DEFAULTS" in rtm.__all__
    params = inspect.signature(rtm.tonemap).parameters
    assert {k: params[k].default for k in rtm.TONEMAP_DEFAULTS} == rtm.TONEMAP_DEFAULTS
    assert params["want"].default == ("u8",) and params["stream"].default is None
    assert "tonemap" in inspect.signature(rtm.Renderer.Render).parameters and hasattr(rtm.Renderer, "write_display")
    assert _lib.lib().rtm_abi_version() == 5  # added without a bump


def test_tonemap_rejects_invalid_arguments_without_a_gpu():
    from raytracingmin_amd import _lib
    L = _lib.lib()
    good = (2, 1, 1, 1, 0.0, 0.18, 0.0)
    color, work, out32, out8, stats = (C.c_void_p(0x1000), C.c_void_p(0x20000), C.c_void_p(0x300000), C.c_void_p(0x4000000),
                                       C.c_void_p(0x50000000))
    # fake device pointers: never dereferenced, every call below fails its checks first

    def call(p=good, w=8, h=8, dev=0, c=color, wk=work, o32=out32, o8=out8, st=stats):
        prm = None if p is None else C.byref(_lib.rtm_tonemap_params(*p))
        return L.rtm_tonemap(prm, w, h, dev, c, wk, o32, o8, st, None)

    def with_(**kw):
        d = dict(zip(FIELDS, good))
        d.update(kw)
        return tuple(d[k] for k in FIELDS)

    assert call(p=None) == -1
    assert b"null" in L.rtm_last_error_detail()
    assert call(c=None) == -1
    assert call(wk=None) == -1
    assert call(o32=None, o8=None, st=None) == -1
    assert b"output" in L.rtm_last_error_detail()
    for w, h in ((0, 8), (8, 0), (-1, 8), (8, -3)):
        assert call(w=w, h=h) == -1, (w, h)
    for op in (-1, 3, 1 << 30):
        assert call(p=with_(op=op)) == -1, op
    for tr in (-1, 2, 77):
        assert call(p=with_(transfer=tr)) == -1, tr
    for field in ("auto_exposure", "dither"):
        for v in (-1, 2, 256):
            assert call(p=with_(**{field: v})) == -1, (field, v)
    for field in ("ev", "key", "white"):
        for v in (float("nan"), float("inf"), float("-inf")):
            assert call(p=with_(**{field: v})) == -1, (field, v)
    for ev in (32.5, -33.0, 1e9):
        assert call(p=with_(ev=ev)) == -1, ev
    for key in (0.0, -0.18, -1e-30):
        assert call(p=with_(key=key)) == -1, key
    for white in (-1.0, -1e-30):
        assert call(p=with_(white=white)) == -1, white
    for off in (8, 16, 64, 128):  # not 256-byte aligned
        assert call(wk=C.c_void_p(0x20000 + off)) == -1, off
        assert b"aligned" in L.rtm_last_error_detail()
    aligned = C.c_void_p(0x70000)  # work_dev equal to any other buffer
    for other in ("c", "o32", "o8", "st"):
        assert call(wk=aligned, **{other: aligned}) == -1, other
        assert b"work_dev" in L.rtm_last_error_detail()
    assert call(st=color) == -1
    assert call(st=out32) == -1
    assert b"stats_out_dev" in L.rtm_last_error_detail()
    assert call(dev=-1) == -1
    assert b"device" in L.rtm_last_error_detail()
    # the limits themselves, in place and a statistics-only call pass every check: what refuses these is the device number
    for kw in (dict(p=with_(ev=32.0)), dict(p=with_(ev=-32.0)), dict(p=with_(white=0.0)), dict(o32=color),
               dict(o32=None, o8=None), dict(o32=None, st=None), dict(p=(0, 0, 0, 0, 0.0, 1e-30, 5.0))):
        assert call(dev=-1, **kw) == -1, kw
        assert b"device" in L.rtm_last_error_detail(), kw


def test_tonemap_work_bytes():
    from raytracingmin_amd import _lib
    L = _lib.lib()
    for w, h in ((0, 5), (5, 0), (-4, 5), (5, -4), (0, 0), (-(2**31), -(2**31))):
        assert L.rtm_tonemap_work_bytes(w, h) == 0, (w, h)

    def formula(w, h):
        blocks = -(-(w * h) // 4096)
        return -(-(16 * blocks) // 256) * 256 + 256

    assert L.rtm_tonemap_work_bytes(1, 1) == formula(1, 1) == 512
    assert L.rtm_tonemap_work_bytes(64, 64) == formula(64, 64) == 512  # exactly one block
    assert L.rtm_tonemap_work_bytes(65, 64) == formula(65, 64) == 512  # two blocks, 32 bytes of partials
    for w, h in ((1, 17), (7, 5), (131, 63), (256, 256), (257, 256), (1920, 1080), (1 << 14, 1 << 14), (2**31 - 1, 1)):
        assert L.rtm_tonemap_work_bytes(w, h) == formula(w, h), (w, h)
    assert L.rtm_tonemap_work_bytes(256, 256) == 512 and L.rtm_tonemap_work_bytes(257, 256) == 768  # 16 -> 17 partials
    assert L.rtm_tonemap_work_bytes(1920, 1080) == 8192 + 256
    # a frame whose 12 bytes a pixel do not fit a size_t
    assert 12 * (2**31 - 1) ** 2 > SIZE_MAX
    assert L.rtm_tonemap_work_bytes(2**31 - 1, 2**31 - 1) == SIZE_MAX


def test_python_argument_errors_raise_before_any_device_use():
    import raytracingmin_amd as rtm
    color = np.zeros((4, 4, 3), np.float32)  # not even a tensor: a bad parameter is reported first
    for kw in (dict(op="filmic"), dict(transfer="gamma"), dict(exposure="manual"), dict(exposure=float("nan")),
               dict(exposure=33.0), dict(exposure=True), dict(key=0.0), dict(key=float("inf")), dict(white=-1.0),
               dict(white=float("nan")), dict(dither="yes"), dict(want=()), dict(want=("f64",))):
        with pytest.raises(ValueError):
            rtm.tonemap(color, **kw)
    data = rtm.LoadData(os.path.join(ROOT, "scenes", "cornellBoxSetting.json")).data
    for bad in ("aces", 1, dict(op="filmic"), dict(exposure="manual"), dict(gamma=2.2), dict(key=-1.0)):
        with pytest.raises(ValueError):
            rtm.Renderer(data).Render("unused", tonemap=bad)
        assert not os.path.exists("unused.bmp")
    with pytest.raises(ValueError):
        rtm.Renderer(data).write_display("unused", op="filmic")


@pytest.mark.parametrize("flags", [["--gpus", "2"], ["--virtual-strips", "2"], ["--force-rccl"]])
def test_cli_display_refuses_multi_gpu_flags_before_any_gpu(tmp_path, flags):
    cli = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
    scene = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
    r = subprocess.run([cli, "-json", scene, "--width", "8", "--height", "8", "--out", "x", "--display"] + flags,
                       cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "--display" in r.stderr
    assert not (tmp_path / "x_display.bmp").exists() and not (tmp_path / "x.bmp").exists()


def test_cli_usage_mentions_display_and_refuses_a_bad_exposure(tmp_path):
    cli = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
    r = subprocess.run([cli, "-?"], capture_output=True, text=True, timeout=60)
    for word in ("--display", "--exposure", "--linear", "--no-dither", "_display.bmp"):
        assert word in r.stdout + r.stderr, word
    scene = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
    r = subprocess.run([cli, "-json", scene, "--out", "x", "--display", "--exposure", "bright"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--exposure" in r.stderr and not (tmp_path / "x.bmp").exists()


# ---- the NumPy reference itself -------------------------------------------------------------------------------------
def test_reference_bayer_index_is_a_permutation_with_the_stated_core():
    b = _tonemap_ref.bayer8()
    assert sorted(b.ravel().tolist()) == list(range(64))
    # the coarsest level (the top two bits) of the aligned 2 x 2 block, rows y, columns x
    assert (b[:2, :2] >> 4).tolist() == [[0, 2], [3, 1]]
    # every aligned 2 x 2 block carries that order, and each finer level repeats it
    for y in range(0, 8, 2):
        for x in range(0, 8, 2):
            assert ((b[y:y + 2, x:x + 2] >> 4) & 3).tolist() == [[0, 2], [3, 1]]
    assert ((b[::2, ::2][:2, :2] >> 2) & 3).tolist() == [[0, 2], [3, 1]]
    assert (b[::4, ::4] & 3).tolist() == [[0, 2], [3, 1]]


def _frame(h, w, seed):
    rng = np.random.default_rng(seed)
    return (8 * rng.random((h, w, 3)) ** 4).astype(np.float32)


def test_reference_identity_case_is_rtm_quantise():
    from raytracingmin_amd import _lib
    color = _frame(9, 13, 3)
    color[0, 0] = [1.5, -0.25, 7.0]
    color[1, 1] = [1.0, 0.999999, 1.0 / 255]
    out, stats = _tonemap_ref.tonemap_ref(color, op="clamp", transfer="linear", exposure=0.0)
    assert stats["exposure"] == 1.0 and stats["pixels"] == 9 * 13
    v = np.ascontiguousarray(color, dtype=np.float64)
    want = np.zeros(v.shape, np.uint8)
    _lib.check(_lib.lib().rtm_quantise(v.ctypes.data, v.size, want.ctypes.data), "rtm_quantise")
    assert np.array_equal(_tonemap_ref.quantise_u8(out.astype(np.float32)), want)
    # and quantise_u8 is rtm_quantise on any float frame
    assert np.array_equal(_tonemap_ref.quantise_u8(color), want)


def test_reference_statistics_and_curves():
    color = np.full((4, 6, 3), 0.5, np.float32)
    color[0, 0] = [np.nan, 0, 0]
    color[0, 1] = [0, np.inf, 0]
    out, st = _tonemap_ref.tonemap_ref(color, op="clamp", transfer="linear", exposure="auto", key=0.18)
    assert st["pixels"] == 22 and np.isclose(st["max_luminance"], 0.5) and np.isclose(st["log_average"], 0.5001, rtol=1e-12)
    assert np.isclose(st["exposure"], 0.18 / 0.5001) and np.allclose(out[1:], 0.5 * 0.18 / 0.5001)
    assert np.array_equal(out[0, :2], np.zeros((2, 3)))  # the pixels that do not count are black
    # an empty frame of statistics
    _, st = _tonemap_ref.tonemap_ref(np.full((2, 2, 3), np.nan, np.float32), exposure=1.0)
    assert st == {"log_average": 1.0, "max_luminance": 1.0, "exposure": 2.0, "pixels": 0}
    # extended Reinhard maps the white point to 1 and keeps chroma; ACES and sRGB at their known values
    grey = np.full((1, 1, 3), 4.0, np.float32)
    out, _ = _tonemap_ref.tonemap_ref(grey, op="reinhard", transfer="linear", exposure=0.0, white=4.0)
    assert np.allclose(out, 1.0, rtol=1e-12)
    out, _ = _tonemap_ref.tonemap_ref(grey, op="reinhard", transfer="linear", exposure=0.0, white=0.0)  # W = L_max
    assert np.allclose(out, 1.0, rtol=1e-6)
    out, _ = _tonemap_ref.tonemap_ref(np.full((1, 1, 3), 0.5, np.float32), op="aces", transfer="linear", exposure=0.0)
    assert np.allclose(out, 0.5 * (2.51 * 0.5 + 0.03) / (0.5 * (2.43 * 0.5 + 0.59) + 0.14))
    out, _ = _tonemap_ref.tonemap_ref(np.array([[[0.0, 0.002, 0.5]]], np.float32), op="clamp", exposure=0.0)
    assert np.allclose(out[0, 0], [0.0, 12.92 * 0.002, 1.055 * 0.5 ** (1 / 2.4) - 0.055], rtol=1e-6)


def test_reference_dither_keeps_the_mean_of_an_aligned_block():
    v = np.float32(100.5 / 255)
    frame = np.full((16, 24, 3), v, np.float32)
    assert np.all(_tonemap_ref.quantise_u8(frame) == 100)
    d = _tonemap_ref.dither_u8(frame)
    assert set(np.unique(d).tolist()) == {100, 101}
    blocks = d.reshape(2, 8, 3, 8, 3).astype(np.float64).mean(axis=(1, 3))
    assert np.all(np.abs(blocks - 255.0 * float(v)) <= 1.0 / 64)
    assert np.all(_tonemap_ref.dither_u8(np.ones((8, 8, 3), np.float32)) == 255)
    assert np.all(_tonemap_ref.dither_u8(np.zeros((8, 8, 3), np.float32)) == 0)
