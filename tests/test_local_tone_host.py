"""The local tone operator, the parts that need no GPU: the bindings and the struct layout, rtm_tonemap_local's argument checks
(all made before any device call), rtm_tonemap_local_work_bytes, the Python entry points' argument errors, the CLI's refusal,
and self-checks of the NumPy reference: the consequences the header states, the direct evaluation, float32 against float64,
and that the pyramid makes the operator local."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _local_tone_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE_MAX = C.c_size_t(-1).value
FIELDS = ("anchor", "shadows", "highlights", "sigma", "levels")
TOL = 1e-4  # include/rtm.h's bar
FRAMES = ref.FRAMES  # the GPU test's


def _header():
    return open(os.path.join(ROOT, "include", "rtm.h")).read()


def _frame(w, h):
    """test_bloom_gpu's recipe: 8 u^4; 10 % exactly black; one negative component; beyond two pixels one NaN pixel and one
    +inf pixel."""
    rng = np.random.default_rng(w * 1000 + h)
    color = (8 * rng.random((h, w, 3)) ** 4).astype(np.float32)
    color[rng.random((h, w)) < 0.1] = 0.0
    flat = color.reshape(-1, 3)
    flat[0] = [0.75, -0.25, 1.5]
    if w * h > 2:
        flat[(w * h) // 2] = [np.nan, 0.5, 0.5]
        flat[w * h - 1] = [0.5, np.inf, 0.5]
    return color


def test_local_is_bound_and_exported_and_the_struct_matches_the_header():
    import raytracingmin_amd as rtm
    from raytracingmin_amd import _lib
    assert "rtm_tonemap_local" in _lib.SIGNATURES and "rtm_tonemap_local_work_bytes" in _lib.SIGNATURES
    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "rtm_tonemap_local") and hasattr(raw, "rtm_tonemap_local_work_bytes")
    header = _header()
    ctype = {"int32_t": C.c_int32, "float": C.c_float}
    body = re.search(r"typedef struct rtm_tonemap_local_params \{(.*?)\} rtm_tonemap_local_params;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for decl in body.split(";"):
        if decl.strip():
            ty, names = decl.split(None, 1)
            declared += [(n.strip(), ctype[ty]) for n in names.split(",")]
    assert [(f[0], f[1]) for f in _lib.rtm_tonemap_local_params._fields_] == declared
    assert tuple(f[0] for f in _lib.rtm_tonemap_local_params._fields_) == FIELDS
    assert C.sizeof(_lib.rtm_tonemap_local_params) == 20
    macro = re.search(r"#define RTM_TONEMAP_LOCAL_DEFAULTS \{([^}]*)\}", header).group(1)
    assert [v.strip() for v in macro.split(",")] == ["1.0f", "2.0f", "2.0f", "0.25f", "5"]
    assert rtm.TONEMAP_LOCAL_DEFAULTS == ref.DEFAULTS == {"anchor": 1.0, "shadows": 2.0, "highlights": 2.0, "sigma": 0.25, "levels": 5}
    assert callable(rtm.tonemap_local) and "tonemap_local" in rtm.__all__ and "TONEMAP_LOCAL_DEFAULTS" in rtm.__all__
    params = inspect.signature(rtm.tonemap_local).parameters
    assert {k: params[k].default for k in rtm.TONEMAP_LOCAL_DEFAULTS} == rtm.TONEMAP_LOCAL_DEFAULTS
    assert params["want"].default == ("f32", "u8", "fused") and params["stats"].default is None
    assert params["stream"].default is None and params["out_f32"].default is None
    assert inspect.signature(rtm.Renderer.Render).parameters["local"].default is False
    assert inspect.signature(rtm.Renderer.write_display).parameters["local"].default is None
    assert _lib.lib().rtm_abi_version() == 5  # added without a bump
    assert re.search(r"#define RTM_ABI_VERSION 5\b", header)


def test_local_rejects_invalid_arguments_without_a_gpu():
    from raytracingmin_amd import _lib
    L = _lib.lib()
    good = (1.0, 2.0, 2.0, 0.25, 5)
    color, stats, work, out32, out8, fused = (C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x20000), C.c_void_p(0x300000),
                                              C.c_void_p(0x4000000), C.c_void_p(0x50000000))
    # fake device pointers: never dereferenced, every call below fails its checks first

    def call(p=good, w=8, h=8, dev=0, c=color, s=stats, wk=work, o32=out32, o8=out8, f=fused):
        prm = None if p is None else C.byref(_lib.rtm_tonemap_local_params(*p))
        return L.rtm_tonemap_local(prm, w, h, dev, c, s, wk, o32, o8, f, None)

    def with_(**kw):
        d = dict(zip(FIELDS, good))
        d.update(kw)
        return tuple(d[k] for k in FIELDS)

    assert call(p=None) == -1
    assert b"null" in L.rtm_last_error_detail()
    assert call(c=None) == -1
    assert call(wk=None) == -1
    assert b"work_dev" in L.rtm_last_error_detail()
    for levels in (1, 8):
        assert call(p=with_(levels=levels), wk=None) == -1
    assert call(o32=None, o8=None, f=None) == -1
    assert b"output" in L.rtm_last_error_detail()
    for w, h in ((0, 8), (8, 0), (-1, 8), (8, -3)):
        assert call(w=w, h=h) == -1, (w, h)
    for field in ("anchor", "shadows", "highlights", "sigma"):
        for v in (float("nan"), float("inf"), float("-inf"), -1.0, -1e-30):
            assert call(p=with_(**{field: v})) == -1, (field, v)
    assert call(p=with_(anchor=0.0)) == -1
    assert b"anchor" in L.rtm_last_error_detail()
    for field in ("shadows", "highlights"):
        for v in (8.000001, 9.0, 1e9):
            assert call(p=with_(**{field: v})) == -1, (field, v)
            assert field.encode() in L.rtm_last_error_detail()
    for v in (0.0, 0.05, 0.0999, 1.0000001, 2.0):
        assert call(p=with_(sigma=v)) == -1, v
        assert b"sigma" in L.rtm_last_error_detail()
    for levels in (9, -1, 1 << 30):
        assert call(p=with_(levels=levels)) == -1, levels
        assert b"levels" in L.rtm_last_error_detail()
    for name in ("c", "o32", "f", "s"):  # a float pointer that is not 4-byte aligned
        for off in (1, 2, 3):
            assert call(**{name: C.c_void_p(0x600000 + off)}) == -1, (name, off)
            assert b"4-byte" in L.rtm_last_error_detail()
    for off in (8, 16, 64, 128):  # not 256-byte aligned
        assert call(wk=C.c_void_p(0x20000 + off)) == -1, off
        assert b"256-byte" in L.rtm_last_error_detail()
    aligned = C.c_void_p(0x70000)  # work_dev equal to any other buffer
    for other in ("c", "s", "o32", "o8", "f"):
        assert call(wk=aligned, **{other: aligned}) == -1, other
        assert b"work_dev" in L.rtm_last_error_detail()
    assert call(f=color) == -1
    assert call(f=out32) == -1
    assert b"fused_out_dev" in L.rtm_last_error_detail()
    assert call(s=color) == -1
    assert call(s=out32) == -1
    assert b"stats_dev" in L.rtm_last_error_detail()
    assert call(o8=color) == -1
    assert b"out_u8_dev" in L.rtm_last_error_detail()
    assert call(dev=-1) == -1
    assert b"device" in L.rtm_last_error_detail()
    # a frame of 2^31 pixels or more
    assert call(w=1 << 16, h=1 << 15) == -8  # RTM_ERR_UNSUPPORTED
    assert b"too large" in L.rtm_last_error_detail()
    # the limits themselves, in place, a single output, no statistics, levels 0 without a work buffer and an odd u8 pointer pass
    # every check: what refuses these is the device
    for kw in (dict(p=with_(shadows=0.0)), dict(p=with_(shadows=8.0)), dict(p=with_(highlights=0.0)), dict(p=with_(highlights=8.0)),
               dict(p=with_(sigma=0.1)), dict(p=with_(sigma=1.0)), dict(p=with_(anchor=1e-30)), dict(p=with_(levels=0)),
               dict(p=with_(levels=0), wk=None), dict(p=with_(levels=8)), dict(o32=color), dict(s=None), dict(o32=None, o8=None),
               dict(o32=None, f=None), dict(o8=None, f=None), dict(o8=C.c_void_p(0x4000001)), dict(w=(1 << 16) - 1, h=1 << 15)):
        assert call(dev=-1, **kw) == -1, kw
        assert b"device" in L.rtm_last_error_detail(), kw


def test_local_work_bytes():
    from raytracingmin_amd import _lib
    L = _lib.lib()
    wb = L.rtm_tonemap_local_work_bytes
    for w, h in ((0, 5), (5, 0), (-4, 5), (5, -4), (0, 0), (-(2**31), -(2**31))):
        assert wb(w, h, 5) == ref.work_bytes(w, h, 5) == 0, (w, h)
    for levels in (0, 9, -1, 100):
        assert wb(64, 64, levels) == ref.work_bytes(64, 64, levels) == 0, levels
    assert wb(1, 1, 1) == 512 and wb(1, 1, 8) == 8 * 512
    assert wb(64, 64, 1) == 2 * 16 * 32 * 32
    assert wb(7, 5, 2) == 2 * (256 + 256)  # 12 records, then 4
    assert wb(9, 9, 1) == 2 * 512  # 25 records: 400 bytes
    for w, h in FRAMES + [(1920, 1080), (3840, 2160), (1 << 14, 1 << 14), (2**31 - 1, 1), (1, 2**31 - 1)]:
        for levels in range(0, 9):
            assert wb(w, h, levels) == ref.work_bytes(w, h, levels), (w, h, levels)
    # two planes of bloom's size per level
    for levels in range(1, 9):
        assert wb(1920, 1080, levels) == 2 * L.rtm_bloom_work_bytes(1920, 1080, levels)
    assert 12 * (2**31 - 1) ** 2 > SIZE_MAX
    assert wb(2**31 - 1, 2**31 - 1, 5) == ref.work_bytes(2**31 - 1, 2**31 - 1, 5) == SIZE_MAX


def test_python_argument_errors_raise_before_any_device_use():
    import raytracingmin_amd as rtm
    color = np.zeros((4, 4, 3), np.float32)  # not even a tensor: a bad parameter is reported first
    for kw in (dict(anchor=0.0), dict(anchor=-1.0), dict(anchor=float("nan")), dict(anchor="high"), dict(shadows=-0.1),
               dict(shadows=8.5), dict(highlights=float("inf")), dict(highlights=9), dict(highlights=True), dict(sigma=0.05),
               dict(sigma=1.5), dict(sigma=None), dict(levels=-1), dict(levels=9), dict(levels=2.5), dict(levels=True),
               dict(want=()), dict(want=("f64",)), dict(want=("stats",))):
        with pytest.raises(ValueError):
            rtm.tonemap_local(color, **kw)
    data = rtm.LoadData(os.path.join(ROOT, "scenes", "cornellBoxSetting.json")).data
    for kw in (dict(local=True), dict(local=dict(levels=3)), dict(local=True, tonemap=False), dict(local=True, denoise=True)):
        with pytest.raises(ValueError, match="tonemap"):
            rtm.Renderer(data).Render("unused", **kw)
        assert not os.path.exists("unused.bmp")
    for bad in ("strong", 1, 0.2, dict(levels=9), dict(radius=3), dict(sigma=2.0), dict(anchor=2.0)):
        with pytest.raises(ValueError):
            rtm.Renderer(data).Render("unused", tonemap=True, local=bad)
        assert not os.path.exists("unused.bmp")
        with pytest.raises(ValueError):
            rtm.Renderer(data).write_display("unused", local=bad)
    assert not os.path.exists("unused_display.bmp")


@pytest.mark.parametrize("flags", [["--local-shadows", "3"], ["--local-highlights", "1"], ["--local-sigma", "0.5"],
                                   ["--local-levels", "3"], ["--display", "--local-levels", "3"],
                                   ["--display", "aces", "--local-shadows", "1", "--local-sigma", "0.2"]])
def test_cli_local_flags_require_display_local_before_any_gpu(tmp_path, flags):
    cli = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
    scene = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
    r = subprocess.run([cli, "-json", scene, "--width", "8", "--height", "8", "--out", "x"] + flags, cwd=tmp_path,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "--local-" in r.stderr and "--display local" in r.stderr
    assert not (tmp_path / "x.bmp").exists() and not (tmp_path / "x_display.bmp").exists()


def test_cli_usage_mentions_local_and_refuses_bad_values(tmp_path):
    cli = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
    r = subprocess.run([cli, "-?"], capture_output=True, text=True, timeout=60)
    for word in ("--display [clamp|reinhard|aces|local]", "--local-shadows S", "--local-highlights S", "--local-sigma V",
                 "--local-levels N"):
        assert word in r.stdout + r.stderr, word
    scene = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
    for flags, word in ((["--local-shadows", "-0.5"], "--local-shadows"), (["--local-shadows", "nan"], "--local-shadows"),
                        (["--local-highlights", "8.5"], "--local-highlights"), (["--local-sigma", "0.05"], "--local-sigma"),
                        (["--local-sigma", "2"], "--local-sigma"), (["--local-levels", "9"], "--local-levels"),
                        (["--local-levels", "2.5"], "--local-levels"), (["--local-levels"], "--local-levels")):
        r = subprocess.run([cli, "-json", scene, "--out", "x", "--display", "local"] + flags, cwd=tmp_path, capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 2 and word + " takes" in r.stderr and not (tmp_path / "x.bmp").exists(), (flags, r.stderr)


# ---- the NumPy reference itself -------------------------------------------------------------------------------------
def test_reference_equal_exposures_give_simple_reinhard_at_every_level_count():
    # (a): the three pyramids are equal and the weights sum to one
    for w, h in ((1, 1), (7, 5), (37, 23)):
        color = _frame(w, h)
        for anchor, sigma in ((0.25, 0.1), (1.0, 0.25), (16.0, 1.0)):
            _, x = ref.exposed(color, anchor)
            for levels in (0, 1, 3, 8):
                out, F = ref.local_ref(color, anchor=anchor, shadows=0.0, highlights=0.0, sigma=sigma, levels=levels)
                assert np.max(np.abs(F - x / (1 + x))) <= 1e-13, (w, h, anchor, levels)


def test_reference_constant_frame_gives_what_levels_zero_gives():
    # (b)
    c = np.array([0.25, 3.0, 0.0], np.float32)
    for w, h in ((1, 1), (7, 5), (13, 9), (16, 16)):
        color = np.broadcast_to(c, (h, w, 3)).copy()
        for anchor, shadows, highlights in ((1.0, 2.0, 2.0), (0.01, 4.0, 0.0), (16.0, 0.0, 8.0)):
            kw = dict(anchor=anchor, shadows=shadows, highlights=highlights)
            out0, F0 = ref.local_ref(color, levels=0, **kw)
            for levels in (1, 3, 8):
                out, F = ref.local_ref(color, levels=levels, **kw)
                assert np.max(np.abs(F - F0)) <= 1e-13 and ref.tolerance_excess(out, out0) <= 1e-12, (w, h, levels)


def test_reference_levels_zero_is_pointwise():
    # (c): a pixel's result does not depend on its place or its neighbours
    color = _frame(37, 23)
    perm = np.random.default_rng(3).permutation(37 * 23)
    shuffled = color.reshape(-1, 3)[perm].reshape(23, 37, 3)
    for kw in (dict(), dict(anchor=16.0, shadows=4.0, highlights=0.0, sigma=0.1)):
        out, F = ref.local_ref(color, levels=0, **kw)
        out_s, F_s = ref.local_ref(shuffled, levels=0, **kw)
        assert np.array_equal(out.reshape(-1, 3)[perm], out_s.reshape(-1, 3)) and np.array_equal(F.reshape(-1)[perm], F_s.reshape(-1))
        I = ref.exposures(ref.exposed(color, kw.get("anchor", 1.0))[1], kw.get("shadows", 2.0), kw.get("highlights", 2.0))
        blend = (ref.weights(I, kw.get("sigma", 0.25)) * I).sum(axis=-1)
        assert np.max(np.abs(F - blend)) <= 1e-15


def test_reference_pixels_that_do_not_count_are_black_and_the_luminance_is_F():
    color = _frame(37, 23)
    ok = ref.counts(color)
    assert (~ok).sum() == 2
    black = color.copy()
    black[~ok] = 0.0
    for levels in (0, 3):
        out, F = ref.local_ref(color, levels=levels)
        out_b, F_b = ref.local_ref(black, levels=levels)
        assert np.all(out[~ok] == 0.0) and np.array_equal(out, out_b) and np.array_equal(F, F_b)
        _, x = ref.exposed(color, 1.0)
        inside = ok & (x >= 1e-4)
        lum = out @ np.array(ref.LUM)
        assert np.max(np.abs(lum[inside] - F[inside])) <= 1e-12 and np.all(lum[ok & ~inside] <= F[ok & ~inside] + 1e-15)


def test_reference_separable_and_direct_evaluations_agree():
    for (w, h), levels in (((7, 5), 3), ((6, 7), 8), ((1, 5), 2), ((4, 1), 2), ((5, 5), 1)):
        color = _frame(w, h)
        for anchor, shadows, highlights, sigma in ((1.0, 2.0, 2.0, 0.25), (16.0, 4.0, 0.0, 0.1), (0.25, 0.0, 4.0, 1.0)):
            I = ref.exposures(ref.exposed(color, anchor)[1], shadows, highlights)
            W = ref.weights(I, sigma)
            assert np.max(np.abs(ref.fuse(I, W, levels) - ref.fuse_direct(I, W, levels))) <= 1e-12, (w, h, levels, anchor)


def test_reference_in_float32_stays_within_the_bar():
    for subset in (ref.SUBSET, ref.SUBSET9):  # every value of every parameter of the product
        assert len(ref.CASES) == 324 and all({c[i] for c in subset} == {c[i] for c in ref.CASES} for i in range(5))
    assert len(ref.SUBSET) >= 24 and len(ref.SUBSET9) == 9
    worst = 0.0
    for w, h in FRAMES:
        color = _frame(w, h)
        for anchor, shadows, highlights, sigma, levels in (ref.SUBSET9 if (w, h) == (258, 66) else ref.SUBSET):
            kw = dict(anchor=anchor, shadows=shadows, highlights=highlights, sigma=float(np.float32(sigma)), levels=levels)
            out, F = ref.local_ref(color, **kw)
            out32, F32 = ref.local_ref(color, dtype=np.float32, **kw)
            assert out32.dtype == np.float32 and F32.dtype == np.float32
            worst = max(worst, ref.tolerance_excess(out32, out), ref.tolerance_excess(F32, F))
    print(f"float32 evaluation against float64: {worst:.3e} (bar {TOL})")
    assert worst <= TOL


def test_the_pyramid_makes_the_operator_local():
    # a dark half with texture next to a bright half: the pyramid keeps more of the texture's contrast in the dark half than
    # the pointwise blend does, and both lift that half above the global curve x / (1 + x)
    w, h = 128, 96
    yy, xx = np.mgrid[:h, :w]
    lum = np.where(xx < 64, 0.02, 20.0) * (1 + 0.2 * np.sin(0.9 * xx) * np.sin(0.7 * yy))
    color = np.repeat(lum[..., None], 3, axis=2).astype(np.float32)
    kw = dict(shadows=3.0, highlights=3.0, sigma=0.25)
    _, x = ref.exposed(color, 1.0)
    glob = (x / (1 + x))[:, 8:56]
    stat = {}
    for levels in (0, 5):
        _, R0 = ref.local_ref(color, levels=levels, unclamped=True, **kw)
        assert R0.min() >= 0.0 and R0.max() <= 1.0, (levels, R0.min(), R0.max())  # F stays within [0, 1] before the clamp
        part = R0[:, 8:56]
        stat[levels] = (part.std() / part.mean(), part.mean())
    print(f"std / mean over columns 8..55: levels 5 {stat[5][0]:.3f}, levels 0 {stat[0][0]:.3f}; mean levels 5 {stat[5][1]:.3f}, "
          f"levels 0 {stat[0][1]:.3f}, global {glob.mean():.3f}")
    assert stat[5][0] > stat[0][0]
    assert stat[5][1] > glob.mean() and stat[0][1] > glob.mean()
