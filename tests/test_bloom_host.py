"""Bloom, the parts that need no GPU: the bindings and the struct layout, rtm_bloom's argument checks (all made before any
device call), rtm_bloom_work_bytes, the Python entry points' argument errors, the CLI's refusal, and self-checks of the NumPy
reference."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _bloom_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE_MAX = C.c_size_t(-1).value
FIELDS = ("threshold", "knee", "intensity", "scatter", "levels")
TOL = 1e-4  # include/rtm.h's bar


def _header():
    return open(os.path.join(ROOT, "include", "rtm.h")).read()


def test_bloom_is_bound_and_exported_and_the_struct_matches_the_header():
    import raytracingmin_amd as rtm
    from raytracingmin_amd import _lib
    assert "rtm_bloom" in _lib.SIGNATURES and "rtm_bloom_work_bytes" in _lib.SIGNATURES
    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "rtm_bloom") and hasattr(raw, "rtm_bloom_work_bytes")
    header = _header()
    ctype = {"int32_t": C.c_int32, "float": C.c_float}
    body = re.search(r"typedef struct rtm_bloom_params \{(.*?)\} rtm_bloom_params;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for decl in body.split(";"):
        if decl.strip():
            ty, names = decl.split(None, 1)
            declared += [(n.strip(), ctype[ty]) for n in names.split(",")]
    assert [(f[0], f[1]) for f in _lib.rtm_bloom_params._fields_] == declared
    assert tuple(f[0] for f in _lib.rtm_bloom_params._fields_) == FIELDS
    assert C.sizeof(_lib.rtm_bloom_params) == 20
    # the header, the package, the reference: one set of defaults
    macro = re.search(r"#define RTM_BLOOM_DEFAULTS \{([^}]*)\}", header).group(1)
    assert [v.strip() for v in macro.split(",")] == ["1.0f", "0.5f", "0.2f", "0.7f", "6"]
    assert rtm.BLOOM_DEFAULTS == _bloom_ref.DEFAULTS == {"threshold": 1.0, "knee": 0.5, "intensity": 0.2, "scatter": 0.7, "levels": 6}
    assert callable(rtm.bloom) and "bloom" in rtm.__all__ and "BLOOM_DEFAULTS" in rtm.__all__
    params = inspect.signature(rtm.bloom).parameters
    assert {k: params[k].default for k in rtm.BLOOM_DEFAULTS} == rtm.BLOOM_DEFAULTS
    assert params["want"].default == ("f32",) and params["stream"].default is None and params["out_f32"].default is None
    assert inspect.signature(rtm.Renderer.Render).parameters["bloom"].default is False
    assert inspect.signature(rtm.Renderer.write_display).parameters["bloom"].default is None
    assert _lib.lib().rtm_abi_version() == 5  # added without a bump
    assert re.search(r"#define RTM_ABI_VERSION 5\b", header)


def test_bloom_rejects_invalid_arguments_without_a_gpu():
    from raytracingmin_amd import _lib
    L = _lib.lib()
    good = (1.0, 0.5, 0.2, 0.7, 6)
    color, work, out32, out8, glow = (C.c_void_p(0x1000), C.c_void_p(0x20000), C.c_void_p(0x300000), C.c_void_p(0x4000000),
                                      C.c_void_p(0x50000000))
    # fake device pointers: never dereferenced, every call below fails its checks first

    def call(p=good, w=8, h=8, dev=0, c=color, wk=work, o32=out32, o8=out8, b=glow):
        prm = None if p is None else C.byref(_lib.rtm_bloom_params(*p))
        return L.rtm_bloom(prm, w, h, dev, c, wk, o32, o8, b, None)

    def with_(**kw):
        d = dict(zip(FIELDS, good))
        d.update(kw)
        return tuple(d[k] for k in FIELDS)

    assert call(p=None) == -1
    assert b"null" in L.rtm_last_error_detail()
    assert call(c=None) == -1
    assert call(wk=None) == -1
    assert call(o32=None, o8=None, b=None) == -1
    assert b"output" in L.rtm_last_error_detail()
    for w, h in ((0, 8), (8, 0), (-1, 8), (8, -3)):
        assert call(w=w, h=h) == -1, (w, h)
    for field in ("threshold", "knee", "intensity", "scatter"):
        for v in (float("nan"), float("inf"), float("-inf"), -1.0, -1e-30):
            assert call(p=with_(**{field: v})) == -1, (field, v)
    for field in ("knee", "scatter"):
        for v in (1.0000001, 2.0, 1e9):
            assert call(p=with_(**{field: v})) == -1, (field, v)
    for levels in (0, 9, -1, 1 << 30):
        assert call(p=with_(levels=levels)) == -1, levels
        assert b"levels" in L.rtm_last_error_detail()
    for name in ("c", "o32", "b"):  # a frame or bloom_out pointer that is not 4-byte aligned
        for off in (1, 2, 3):
            assert call(**{name: C.c_void_p(0x600000 + off)}) == -1, (name, off)
            assert b"4-byte" in L.rtm_last_error_detail()
    for off in (8, 16, 64, 128):  # not 256-byte aligned
        assert call(wk=C.c_void_p(0x20000 + off)) == -1, off
        assert b"256-byte" in L.rtm_last_error_detail()
    aligned = C.c_void_p(0x70000)  # work_dev equal to any other buffer
    for other in ("c", "o32", "o8", "b"):
        assert call(wk=aligned, **{other: aligned}) == -1, other
        assert b"work_dev" in L.rtm_last_error_detail()
    assert call(b=color) == -1
    assert call(b=out32) == -1
    assert b"bloom_out_dev" in L.rtm_last_error_detail()
    assert call(o8=color) == -1
    assert b"out_u8_dev" in L.rtm_last_error_detail()
    assert call(dev=-1) == -1
    assert b"device" in L.rtm_last_error_detail()
    # a frame of 2^31 pixels or more
    assert call(w=1 << 16, h=1 << 15) == -8  # RTM_ERR_UNSUPPORTED
    assert b"too large" in L.rtm_last_error_detail()
    # the limits themselves, in place, a single output and an odd u8 pointer pass every check: what refuses these is the device
    for kw in (dict(p=with_(threshold=0.0)), dict(p=with_(knee=0.0)), dict(p=with_(knee=1.0)), dict(p=with_(scatter=0.0)),
               dict(p=with_(scatter=1.0)), dict(p=with_(intensity=0.0)), dict(p=with_(levels=1)), dict(p=with_(levels=8)),
               dict(o32=color), dict(o32=None, o8=None), dict(o32=None, b=None), dict(o8=None, b=None),
               dict(o8=C.c_void_p(0x4000001)), dict(w=(1 << 16) - 1, h=1 << 15)):
        assert call(dev=-1, **kw) == -1, kw
        assert b"device" in L.rtm_last_error_detail(), kw


def test_bloom_work_bytes():
    from raytracingmin_amd import _lib
    L = _lib.lib()
    for w, h in ((0, 5), (5, 0), (-4, 5), (5, -4), (0, 0), (-(2**31), -(2**31))):
        assert L.rtm_bloom_work_bytes(w, h, 6) == _bloom_ref.work_bytes(w, h, 6) == 0, (w, h)
    for levels in (0, 9, -1, 100):
        assert L.rtm_bloom_work_bytes(64, 64, levels) == _bloom_ref.work_bytes(64, 64, levels) == 0, levels
    assert _bloom_ref.level_sizes(7, 5, 4) == [(7, 5), (4, 3), (2, 2), (1, 1), (1, 1)]
    assert _bloom_ref.level_sizes(1, 17, 3) == [(1, 17), (1, 9), (1, 5), (1, 3)]
    assert L.rtm_bloom_work_bytes(1, 1, 1) == 256 and L.rtm_bloom_work_bytes(1, 1, 8) == 8 * 256
    assert L.rtm_bloom_work_bytes(64, 64, 1) == 16 * 32 * 32
    assert L.rtm_bloom_work_bytes(7, 5, 2) == 256 + 256  # 12 records, then 4
    assert L.rtm_bloom_work_bytes(9, 9, 1) == 512  # 25 records: 400 bytes
    for w, h in ((1, 1), (1, 17), (17, 1), (2, 2), (7, 5), (37, 23), (64, 64), (131, 63), (258, 66), (1920, 1080), (3840, 2160),
                 (1 << 14, 1 << 14), (2**31 - 1, 1), (1, 2**31 - 1)):
        for levels in range(1, 9):
            assert L.rtm_bloom_work_bytes(w, h, levels) == _bloom_ref.work_bytes(w, h, levels), (w, h, levels)
    # the plane of level 1 is about 4 bytes per full-resolution pixel
    assert L.rtm_bloom_work_bytes(1920, 1080, 1) == 16 * 960 * 540 == 4 * 1920 * 1080
    # a frame whose 12 bytes a pixel do not fit a size_t
    assert 12 * (2**31 - 1) ** 2 > SIZE_MAX
    assert L.rtm_bloom_work_bytes(2**31 - 1, 2**31 - 1, 6) == _bloom_ref.work_bytes(2**31 - 1, 2**31 - 1, 6) == SIZE_MAX


def test_python_argument_errors_raise_before_any_device_use():
    import raytracingmin_amd as rtm
    color = np.zeros((4, 4, 3), np.float32)  # not even a tensor: a bad parameter is reported first
    for kw in (dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold="high"), dict(knee=1.5), dict(knee=-0.1),
               dict(knee=float("inf")), dict(intensity=-0.2), dict(intensity=float("inf")), dict(intensity=True),
               dict(scatter=1.01), dict(scatter=-1.0), dict(scatter=None), dict(levels=0), dict(levels=9), dict(levels=2.5),
               dict(levels=True), dict(want=()), dict(want=("f64",)), dict(want=("stats",))):
        with pytest.raises(ValueError):
            rtm.bloom(color, **kw)
    data = rtm.LoadData(os.path.join(ROOT, "scenes", "cornellBoxSetting.json")).data
    # bloom without tonemap: linear HDR through the reference's quantiser would only clip
    for kw in (dict(bloom=True), dict(bloom=dict(intensity=0.5)), dict(bloom=True, tonemap=False), dict(bloom=True, denoise=True)):
        with pytest.raises(ValueError, match="tonemap"):
            rtm.Renderer(data).Render("unused", **kw)
        assert not os.path.exists("unused.bmp")
    for bad in ("strong", 1, 0.2, dict(levels=0), dict(radius=3), dict(knee=2.0)):
        with pytest.raises(ValueError):
            rtm.Renderer(data).Render("unused", tonemap=True, bloom=bad)
        assert not os.path.exists("unused.bmp")
        with pytest.raises(ValueError):
            rtm.Renderer(data).write_display("unused", bloom=bad)
    assert not os.path.exists("unused_display.bmp")


@pytest.mark.parametrize("flags", [["--bloom"], ["--bloom", "0.4"], ["--bloom", "--bloom-threshold", "2", "--bloom-levels", "3"],
                                   ["--bloom", "--pfm"]])
def test_cli_bloom_requires_display_before_any_gpu(tmp_path, flags):
    cli = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
    scene = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
    r = subprocess.run([cli, "-json", scene, "--width", "8", "--height", "8", "--out", "x"] + flags, cwd=tmp_path,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "--bloom" in r.stderr and "--display" in r.stderr
    assert not (tmp_path / "x.bmp").exists() and not (tmp_path / "x_display.bmp").exists()


def test_cli_usage_mentions_bloom_and_refuses_bad_values(tmp_path):
    cli = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
    r = subprocess.run([cli, "-?"], capture_output=True, text=True, timeout=60)
    for word in ("--bloom [INTENSITY]", "--bloom-threshold T", "--bloom-levels L"):
        assert word in r.stdout + r.stderr, word
    scene = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
    for flags, word in ((["--bloom", "-0.5"], "--bloom"), (["--bloom", "nan"], "--bloom"), (["--bloom", "--bloom-levels", "9"], "--bloom-levels"),
                        (["--bloom", "--bloom-levels", "2.5"], "--bloom-levels"), (["--bloom", "--bloom-threshold", "-1"], "--bloom-threshold"),
                        (["--bloom", "--bloom-threshold"], "--bloom-threshold")):
        r = subprocess.run([cli, "-json", scene, "--out", "x", "--display"] + flags, cwd=tmp_path, capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 2 and word + " takes" in r.stderr and not (tmp_path / "x.bmp").exists(), (flags, r.stderr)


# ---- the NumPy reference itself -------------------------------------------------------------------------------------
def _frame(h, w, seed):
    rng = np.random.default_rng(seed)
    color = (8 * rng.random((h, w, 3)) ** 4).astype(np.float32)
    color[rng.random((h, w)) < 0.1] = 0.0
    return color


def test_reference_filters_are_normalised_and_aligned():
    for n in (1, 2, 3, 4, 5, 8, 17):
        d = _bloom_ref.down_matrix(n)
        assert d.shape == (-(-n // 2), n) and np.allclose(d.sum(axis=1), 1.0, rtol=0, atol=1e-15)
        assert np.all(d[np.arange(d.shape[0]), 2 * np.arange(d.shape[0])] > 0)  # the tap 2X is always in the frame
        u = _bloom_ref.up_matrix(n, d.shape[0])
        assert np.allclose(u.sum(axis=1), 1.0, rtol=0, atol=1e-15) and np.all(u.max(axis=1) >= 0.75)  # the 3/4 tap is, too
    # away from the border both filters keep a ramp's position: down is centred on 2X + 0.5, up on x / 2 - 1/4
    n = 16
    ramp = np.arange(n, dtype=np.float64)
    coarse = _bloom_ref.down_matrix(n) @ ramp
    assert np.allclose(coarse[1:-1], 2 * np.arange(1, n // 2 - 1) + 0.5, rtol=0, atol=1e-13)
    fine = _bloom_ref.up_matrix(n, n // 2) @ np.arange(n // 2, dtype=np.float64)
    assert np.allclose(fine[1:-1], np.arange(1, n - 1) / 2 - 0.25, rtol=0, atol=1e-13)


def test_reference_constant_frame_blooms_to_itself():
    c = np.array([0.25, 3.0, 0.0], np.float32)
    for w, h, levels in ((1, 1, 1), (7, 5, 4), (13, 9, 8), (16, 16, 3)):
        color = np.broadcast_to(c, (h, w, 3)).copy()
        for scatter in (0.0, 0.7, 1.0):
            out, B = _bloom_ref.bloom_ref(color, threshold=0.0, knee=0.5, intensity=0.5, scatter=scatter, levels=levels)
            assert np.allclose(B, c.astype(np.float64), rtol=1e-13, atol=0), (w, h, levels, scatter)
            assert np.allclose(out, 1.5 * c.astype(np.float64), rtol=1e-13, atol=0)


def test_reference_threshold_above_the_maximum_gives_no_bloom_and_zero_intensity_the_input():
    color = _frame(9, 13, 5)
    color[2, 3] = [np.nan, 1.0, 1.0]
    color[4, 4] = [1.0, np.inf, -1.0]
    y_max = 8.0 * sum(_bloom_ref.LUM)
    for knee, threshold in ((0.0, y_max), (0.5, 2 * y_max), (1.0, 1e30)):
        out, B = _bloom_ref.bloom_ref(color, threshold=threshold, knee=knee, levels=3)
        if knee < 1.0:  # every Y at or below T - K
            assert np.all(B == 0.0) and not np.any(np.signbit(B)), knee
    ok = _bloom_ref.counts(color)
    assert ok.sum() == 9 * 13 - 2
    out, B = _bloom_ref.bloom_ref(color, threshold=0.5, intensity=0.0, levels=3)
    assert np.array_equal(out[ok], color.astype(np.float64)[ok]) and np.all(np.isfinite(B)) and np.any(B > 0)
    # a pixel that does not count keeps its input and adds no light: the frame with those pixels black blooms alike
    assert np.isnan(out[2, 3, 0]) and np.isposinf(out[4, 4, 1]) and out[4, 4, 2] == -1.0
    black = color.copy()
    black[~ok] = 0.0
    assert np.array_equal(_bloom_ref.bloom_ref(black, threshold=0.5, levels=3)[1], _bloom_ref.bloom_ref(color, threshold=0.5, levels=3)[1])


def test_reference_separable_and_direct_evaluations_agree():
    for (w, h), levels in (((13, 9), 3), ((6, 7), 8), ((1, 5), 2), ((4, 1), 2)):
        color = _frame(h, w, w * 100 + h)
        for threshold, knee, scatter in ((0.0, 0.5, 0.7), (1.0, 0.0, 1.0), (3.0, 1.0, 0.0)):
            B = _bloom_ref.bloom_ref(color, threshold=threshold, knee=knee, scatter=scatter, levels=levels)[1]
            direct = _bloom_ref.bloom_direct(color, threshold, knee, scatter, levels)
            assert _bloom_ref.tolerance_excess(B, direct) <= 1e-12, (w, h, levels, threshold)


def test_reference_in_float32_stays_within_the_bar():
    worst = 0.0
    for w, h in ((7, 5), (37, 23), (64, 64), (131, 63)):
        color = _frame(h, w, w + h)
        for threshold, knee, scatter, levels in ((0.0, 0.5, 0.7, 8), (1.0, 0.0, 1.0, 3), (3.0, 1.0, 0.0, 1), (1.0, 0.5, 0.7, 6)):
            kw = dict(threshold=threshold, knee=knee, scatter=scatter, levels=levels)
            out, B = _bloom_ref.bloom_ref(color, **kw)
            out32, B32 = _bloom_ref.bloom_ref(color, dtype=np.float32, **kw)
            assert out32.dtype == np.float32 and B32.dtype == np.float32
            worst = max(worst, _bloom_ref.tolerance_excess(out32, out), _bloom_ref.tolerance_excess(B32, B))
    print(f"float32 evaluation against float64: {worst:.3e} (bar {TOL})")
    assert worst <= TOL
