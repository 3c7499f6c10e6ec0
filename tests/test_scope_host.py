"""The frame scopes, the parts that need no GPU: the bindings and the struct layouts, the argument checks of rtm_scopes and
rtm_scope_draw (all made before any device call), the host-only readers of a histogram against the NumPy reference, the count
rules include/rtm.h states, shown on the reference, and the CLI's refusals and help text."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _scope_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
SCENE = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
NAMES = ("rtm_scopes", "rtm_scope_draw", "rtm_scope_bin_range", "rtm_scope_percentile", "rtm_scope_exposure")


def _header():
    return open(os.path.join(ROOT, "include", "rtm.h")).read()


def _record(hist):
    from raytracingmin_amd import _lib
    return _lib.rtm_scope_histogram.from_buffer_copy(ref.words(hist).tobytes())


def _hist(bins=(), below=(0, 0, 0, 0), above=(0, 0, 0, 0), not_counting=0):
    """A hand-built histogram: bins = ((channel, bin, count), ...); every channel is brought to the same pixel count through
    its `below`, so that the record obeys the count rule."""
    h = {"bins": np.zeros((4, 256), np.uint32), "below": np.array(below, np.uint32), "above": np.array(above, np.uint32),
         "pixels": 0, "not_counting": not_counting, "reserved": np.zeros(2, np.uint32)}
    for c, b, n in bins:
        h["bins"][c, b] += n
    totals = h["bins"].sum(axis=1).astype(np.int64) + h["below"] + h["above"]
    h["pixels"] = int(totals.max())
    h["below"] = (h["below"] + (h["pixels"] - totals)).astype(np.uint32)
    ref.invariants(h)
    return h


def test_scopes_are_bound_and_exported_and_the_structs_match_the_header():
    import raytracingmin_amd as rtm
    from raytracingmin_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n in _lib.SIGNATURES and hasattr(raw, n), n
    header = _header()
    assert re.search(r"enum \{ RTM_SCOPE_LOG2 = 0, RTM_SCOPE_CODE = 1 \};", header)
    assert re.search(r"enum \{ RTM_SCOPE_LUMA = 0, RTM_SCOPE_OVERLAY = 1, RTM_SCOPE_PARADE = 2 \};", header)
    assert _lib.SCOPE_MODES == ref.MODES == {"log2": 0, "code": 1}
    assert _lib.SCOPE_LAYOUTS == ref.LAYOUTS == {"luma": 0, "overlay": 1, "parade": 2}
    body = re.search(r"typedef struct rtm_scope_params \{(.*?)\} rtm_scope_params;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [d.split() for d in body.split(";") if d.strip()] == [["int32_t", "mode"], ["int32_t", "columns"]]
    assert [(f[0], f[1]) for f in _lib.rtm_scope_params._fields_] == [("mode", C.c_int32), ("columns", C.c_int32)]
    assert C.sizeof(_lib.rtm_scope_params) == 8
    body = re.search(r"typedef struct rtm_scope_histogram \{(.*?)\} rtm_scope_histogram;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [" ".join(d.split()) for d in body.split(";") if d.strip()] == [
        "uint32_t bins[4][256]", "uint32_t below[4], above[4]", "uint32_t pixels, not_counting, reserved[2]"]
    H = _lib.rtm_scope_histogram
    assert C.sizeof(H) == ref.HIST_BYTES == 4144
    assert {f[0]: getattr(H, f[0]).offset for f in H._fields_} == ref.HIST_OFFSETS
    assert H.bins.size == 4096 and H.reserved.size == 8
    macro = re.search(r"#define RTM_SCOPE_DEFAULTS \{([^}]*)\}", header).group(1)
    assert [v.strip() for v in macro.split(",")] == ["RTM_SCOPE_LOG2", "256"]
    assert rtm.SCOPE_DEFAULTS == _lib.SCOPE_DEFAULTS == ref.DEFAULTS == {"mode": "log2", "columns": 256}
    for name in ("scopes", "scope_draw", "scope_percentile", "scope_exposure", "scope_bin_range", "SCOPE_DEFAULTS"):
        assert name in rtm.__all__ and hasattr(rtm, name), name
    params = inspect.signature(rtm.scopes).parameters
    assert list(params) == ["color", "mode", "columns", "want", "stream"]
    assert (params["mode"].default, params["columns"].default, params["want"].default, params["stream"].default) == \
        ("log2", 256, ("histogram",), None)
    assert list(inspect.signature(rtm.Renderer.scopes).parameters)[:2] == ["self", "frame"]
    assert list(inspect.signature(rtm.Renderer.write_scopes).parameters)[:3] == ["self", "fileName", "frame"]
    assert _lib.lib().rtm_abi_version() == 5 and re.search(r"#define RTM_ABI_VERSION 5\b", header)  # added without a bump
    assert "INTEGER ATOMICS ONLY" in header


def test_scopes_reject_invalid_arguments_without_a_gpu():
    from raytracingmin_amd import _lib
    L = _lib.lib()
    # fake device pointers: never dereferenced, every call below fails its checks first
    color, hist, wave = C.c_void_p(0x1000), C.c_void_p(0x20000), C.c_void_p(0x300000)

    def call(p=(0, 4), w=8, h=8, dev=0, c=color, hi=hist, wv=wave):
        prm = None if p is None else C.byref(_lib.rtm_scope_params(*p))
        return L.rtm_scopes(prm, w, h, dev, c, hi, wv, None)

    detail = L.rtm_last_error_detail
    assert call(p=None) == -1 and b"params" in detail()
    assert call(c=None) == -1 and b"color_dev" in detail()
    assert call(hi=None, wv=None) == -1 and b"both outputs" in detail()
    for w, h in ((0, 8), (8, 0), (-1, 8), (8, -3)):
        assert call(w=w, h=h) == -1 and b"size" in detail(), (w, h)
    for m in (-1, 2, 1 << 30):
        assert call(p=(m, 4)) == -1 and b"mode" in detail(), m
    for cols in (0, -1, 9, 1 << 30):
        assert call(p=(0, cols)) == -1 and b"columns" in detail(), cols
    for name in ("c", "hi", "wv"):
        for off in (1, 2, 3):
            assert call(**{name: C.c_void_p(0x600000 + off)}) == -1 and b"4-byte" in detail(), (name, off)
    for name in ("hi", "wv"):
        assert call(**{name: color}) == -1 and b"color_dev" in detail(), name
    assert call(wv=hist) == -1 and b"alias each other" in detail()
    assert call(dev=-1) == -1 and b"device" in detail()
    assert call(w=1 << 16, h=1 << 15) == -8 and b"too large" in detail()  # RTM_ERR_UNSUPPORTED: 2^31 pixels
    # what passes every check is refused by the device number only: columns are ignored without a waveform, the limits pass
    for kw in (dict(p=(0, 0), wv=None), dict(p=(1, -7), wv=None), dict(p=(1, 8)), dict(p=(0, 1)), dict(hi=None),
               dict(w=(1 << 16) - 1, h=1 << 15, p=(0, 1)), dict(w=1, h=1, p=(1, 1))):
        assert call(dev=-1, **kw) == -1 and b"device" in detail(), kw

    out = C.c_void_p(0x4000000)

    def draw(columns=4, layout=0, gain=1, dev=0, wv=wave, o=out):
        return L.rtm_scope_draw(columns, layout, gain, dev, wv, o, None)

    assert draw(wv=None) == -1 and draw(o=None) == -1 and b"null" in detail()
    for cols in (0, -1):
        assert draw(columns=cols) == -1 and b"columns" in detail(), cols
    for lay in (-1, 3):
        assert draw(layout=lay) == -1 and b"layout" in detail(), lay
    assert draw(gain=0) == -1 and b"gain" in detail()
    assert draw(wv=C.c_void_p(0x300002)) == -1 and b"4-byte" in detail()
    assert draw(o=wave) == -1 and b"aliases" in detail()
    assert draw(columns=1 << 21) == -8
    assert draw(dev=-1) == -1 and b"device" in detail()
    for kw in (dict(layout=2, gain=0xFFFFFFFF), dict(columns=(1 << 21) - 1), dict(o=C.c_void_p(0x4000003))):
        assert draw(dev=-1, **kw) == -1 and b"device" in detail(), kw


def test_host_readers_reject_invalid_arguments():
    from raytracingmin_amd import _lib
    L = _lib.lib()
    rec = _record(_hist(bins=((0, 100, 10),)))
    lo, hi, v, b = C.c_float(), C.c_float(), C.c_float(), C.c_int32()
    assert L.rtm_scope_bin_range(0, 0, None, C.byref(hi)) == -1 and L.rtm_scope_bin_range(0, 0, C.byref(lo), None) == -1
    for mode, bin_ in ((2, 0), (-1, 0), (0, -1), (0, 256), (1, 256)):
        assert L.rtm_scope_bin_range(mode, bin_, C.byref(lo), C.byref(hi)) == -1, (mode, bin_)
    assert L.rtm_scope_percentile(None, 0, 0, 50.0, C.byref(v), C.byref(b)) == -1
    assert L.rtm_scope_percentile(C.byref(rec), 0, 0, 50.0, None, None) == -1
    for mode, ch, pc in ((2, 0, 50.0), (0, -1, 50.0), (0, 4, 50.0), (0, 0, -0.001), (0, 0, 100.001), (0, 0, float("nan")),
                         (0, 0, float("inf"))):
        assert L.rtm_scope_percentile(C.byref(rec), mode, ch, pc, C.byref(v), C.byref(b)) == -1, (mode, ch, pc)
    assert L.rtm_scope_percentile(C.byref(rec), 0, 0, 50.0, C.byref(v), None) == 0
    assert L.rtm_scope_percentile(C.byref(rec), 0, 0, 50.0, None, C.byref(b)) == 0 and b.value == 100
    assert L.rtm_scope_exposure(None, 50.0, 0.18, C.byref(v)) == -1 and L.rtm_scope_exposure(C.byref(rec), 50.0, 0.18, None) == -1
    for pc, target in ((-1.0, 0.18), (101.0, 0.18), (float("nan"), 0.18), (50.0, 0.0), (50.0, -1.0), (50.0, float("inf")),
                       (50.0, float("nan"))):
        assert L.rtm_scope_exposure(C.byref(rec), pc, target, C.byref(v)) == -1, (pc, target)


def test_python_argument_errors_raise_before_any_device_use():
    import raytracingmin_amd as rtm
    color = np.zeros((4, 4, 3), np.float32)  # not even a tensor: a bad parameter comes first
    for kw in (dict(mode="stops"), dict(mode=0), dict(want=()), dict(want=("hist",))):
        with pytest.raises(ValueError):
            rtm.scopes(color, **kw)
    for kw in (dict(layout="rgb"), dict(gain=0), dict(gain=1.5), dict(gain=True), dict(gain=1 << 32)):
        with pytest.raises(ValueError):
            rtm.scope_draw(color, **kw)
    h = _hist(bins=((0, 100, 10),))
    for bad in (dict(channel="x"), dict(channel=4), dict(mode="lin")):
        with pytest.raises(ValueError):
            rtm.scope_percentile(h, 50, **bad)
    with pytest.raises(rtm.RtmError):
        rtm.scope_percentile(h, 101)
    with pytest.raises(rtm.RtmError):
        rtm.scope_exposure(h, 50, target=0.0)
    with pytest.raises(ValueError):
        rtm.scope_percentile(np.zeros(7, np.uint32), 50)
    for bad in (-1, 256, 1.0):
        with pytest.raises(ValueError):
            rtm.scope_bin_range("log2", bad)


def test_the_binning_rule_on_the_values_the_header_names():
    f = np.float32
    log2 = lambda v: int(ref.bin_of(f(v), ref.LOG2))
    for b in (0, 1, 7, 8, 128, 255):
        lo, _ = ref.bin_range(ref.LOG2, b)
        assert log2(lo) == b and log2(np.nextafter(lo, f(0))) == b - 1, b  # (bin -1 is BELOW)
    assert ref.bin_range(ref.LOG2, 128)[0] == 1.0 and ref.bin_range(ref.LOG2, 0)[0] == f(2.0 ** -16)
    assert log2(0.18) == 107 and log2(65536.0) == ref.ABOVE and log2(np.inf) == ref.ABOVE
    assert log2(np.nextafter(f(65536), f(0))) == 255
    for v in (0.0, -0.0, 1e-40, -1e-40, -1.0, -np.inf, 1.5e-5):
        assert log2(v) == ref.BELOW, v
    code = lambda v: int(ref.bin_of(f(v), ref.CODE))
    assert code(-0.0) == 0 and code(0.0) == 0 and code(1.0) == 255 and code(np.nextafter(f(1), f(0))) == 254
    assert code(-1e-45) == ref.BELOW and code(np.nextafter(f(1), f(2))) == ref.ABOVE and code(np.inf) == ref.ABOVE
    # the byte rtm_quantise stores
    from raytracingmin_amd import _lib
    v = np.ascontiguousarray(ref.specials()[np.isfinite(ref.specials())], dtype=np.float32)
    v = v[(v >= 0) & (v <= 1)]
    d = v.astype(np.float64)
    out = np.zeros(d.size, np.uint8)
    assert _lib.lib().rtm_quantise(d.ctypes.data, d.size, out.ctypes.data) == 0
    assert np.array_equal(out, ref.bin_of(v, ref.CODE).astype(np.uint8))


@pytest.mark.parametrize("mode", ["log2", "code"])
def test_bin_range_agrees_with_the_reference_for_every_bin(mode):
    import raytracingmin_amd as rtm
    m = ref.MODES[mode]
    last_hi = None
    for b in range(256):
        lo, hi = rtm.scope_bin_range(mode, b)
        rlo, rhi = ref.bin_range(m, b)
        assert (np.float32(lo), np.float32(hi)) == (rlo, rhi), (b, lo, hi, rlo, rhi)
        assert int(ref.bin_of(np.float32(lo), m)) == b, b
        if mode == "log2" or b > 0:  # CODE's bin 0 starts at 0: what lies before it has no float between
            assert int(ref.bin_of(np.nextafter(np.float32(lo), np.float32(0)), m)) == b - 1, b
        assert last_hi is None or last_hi == lo
        last_hi = hi
    assert last_hi == (65536.0 if mode == "log2" else 1.0)


def _check_percentiles(h, percents=(0, 1e-9, 1, 25, 50, 75, 99, 99.9, 100)):
    import raytracingmin_amd as rtm
    for mode, m in ref.MODES.items():
        for c in range(4):
            for p in percents:
                got = rtm.scope_percentile(h, p, c, mode)
                want = ref.percentile(h, m, c, p)
                assert np.float32(got[0]).view(np.uint32) == want[0].view(np.uint32) and got[1] == want[1], (mode, c, p, got, want)
    for p in percents:
        for target in (0.18, 0.8, 1e-30, 1e30):
            got, want = np.float32(rtm.scope_exposure(h, p, target)), ref.exposure(h, p, target)
            assert got.view(np.uint32) == want.view(np.uint32), (p, target, got, want)


def test_percentile_and_exposure_agree_with_the_reference_on_hand_built_histograms():
    import raytracingmin_amd as rtm
    empty = _hist(not_counting=12)
    assert rtm.scope_percentile(empty, 50) == (1.0, -2) and rtm.scope_exposure(empty, 50, 0.18) == np.float32(np.log2(0.18))
    _check_percentiles(empty)
    all_below = _hist(below=(9, 9, 9, 9))
    assert rtm.scope_percentile(all_below, 100) == (0.0, -1) and rtm.scope_exposure(all_below, 100, 0.18) == 0.0
    _check_percentiles(all_below)
    one_bin = _hist(bins=tuple((c, 128, 1000) for c in range(4)))
    assert rtm.scope_percentile(one_bin, 50) == (1.0625, 128) and rtm.scope_percentile(one_bin, 100) == (1.125, 128)
    assert rtm.scope_percentile(one_bin, 0) == (0.0, -1)
    assert rtm.scope_percentile(one_bin, 50, "b", "code")[1] == 128
    _check_percentiles(one_bin)
    all_above = _hist(above=(5, 5, 5, 5))
    assert rtm.scope_percentile(all_above, 50) == (65536.0, 256) and rtm.scope_percentile(all_above, 50, mode="code") == (1.0, 256)
    assert rtm.scope_exposure(all_above, 50, 1e-30) == -32.0
    _check_percentiles(all_above)
    # t exactly on a cumulative boundary: 25 % of 400 is the whole of the first bin, 50 % the whole of the second
    steps = _hist(bins=tuple((c, b, 100) for c in range(4) for b in (10, 20, 30, 255)))
    assert rtm.scope_percentile(steps, 25) == (float(ref.bin_range(0, 10)[1]), 10)
    assert rtm.scope_percentile(steps, 50) == (float(ref.bin_range(0, 20)[1]), 20)
    assert rtm.scope_percentile(steps, 50.0000001)[1] == 30
    assert rtm.scope_percentile(steps, 100) == (65536.0, 255)
    assert rtm.scope_percentile(steps, 100, mode="code") == (1.0, 255)
    _check_percentiles(steps)
    # below on the boundary, then bins: t <= below is still "below"
    mixed = _hist(bins=((0, 107, 50), (1, 0, 50), (2, 254, 50), (3, 255, 50)), below=(50, 50, 50, 50), above=(0, 0, 0, 0))
    assert rtm.scope_percentile(mixed, 50) == (0.0, -1) and rtm.scope_percentile(mixed, 51)[1] == 107
    _check_percentiles(mixed)
    _check_percentiles(ref.histogram(ref.frame(33, 17, 5), ref.LOG2))
    # the summary rtm_cli prints
    s = rtm.scope_summary(mixed)
    assert s["pixels"] == 100 and s["below"] == [0.5] * 4 and s["above"] == [0.0] * 4 and list(s["percentiles"]) == ["1", "50", "99", "99.9"]
    assert s["percentiles"]["99"] == rtm.scope_percentile(mixed, 99)[0]


@pytest.mark.parametrize("w,h,columns", [(1, 1, 1), (9, 1, 9), (1, 9, 1), (33, 17, 5), (131, 63, 131), (131, 63, 5), (257, 129, 100)])
def test_the_count_rules_hold_on_the_reference(w, h, columns):
    for mode, display in ((ref.LOG2, False), (ref.CODE, True), (ref.CODE, False)):
        f = ref.frame(w, h, 7 * w + h, display=display)
        hist, wave = ref.histogram(f, mode), ref.waveform(f, mode, columns)
        ref.invariants(hist, wave, w * h)
        assert np.array_equal(ref.from_words(ref.words(hist))["bins"], hist["bins"])
        for layout, width in ((ref.LUMA, columns), (ref.OVERLAY, columns), (ref.PARADE, 3 * columns)):
            assert ref.draw(wave, layout, 7).shape == (256, width, 3)
    if w * h >= 33 * 17:  # the planted values reach every outcome
        f = ref.frame(w, h, 1)
        hist = ref.histogram(f, ref.LOG2)
        assert hist["not_counting"] > 0 and hist["below"].all() and hist["above"].all()
    nothing = np.full((h, w, 3), np.nan, np.float32)
    hist = ref.histogram(nothing, ref.LOG2)
    assert hist["pixels"] == 0 and hist["not_counting"] == w * h and not hist["bins"].any()


def test_the_reference_draws_what_the_header_says():
    wave = np.zeros((4, 256, 3), np.uint32)
    wave[0, 255, 0], wave[1, 0, 1], wave[2, 10, 2], wave[3, 255, 2] = 5, 40, 1, 1 << 31
    luma = ref.draw(wave, ref.LUMA, 7)
    assert luma[0, 0].tolist() == [35, 35, 35] and not luma[1:].any()  # bin 255 is the top row
    over = ref.draw(wave, ref.OVERLAY, 7)
    assert over[255, 1].tolist() == [255, 0, 0] and over[245, 2].tolist() == [0, 7, 0] and over[0, 2].tolist() == [0, 0, 255]
    parade = ref.draw(wave, ref.PARADE, 1)
    assert parade[255, 1].tolist() == [40, 0, 0] and parade[245, 3 + 2].tolist() == [0, 1, 0] and parade[0, 6 + 2].tolist() == [0, 0, 255]
    assert parade.sum() == 40 + 1 + 255


REFUSALS = [
    (["--scopes-columns", "16"], "--scopes-columns and --scopes-layout require --scopes"),
    (["--scopes-layout", "parade"], "--scopes-columns and --scopes-layout require --scopes"),
    (["--scopes", "--gpus", "2"], "--scopes runs on one GPU"),
    (["--scopes", "--virtual-strips", "2"], "--scopes runs on one GPU"),
    (["--scopes", "--force-rccl"], "--scopes runs on one GPU"),
    (["--scopes", "--preview", "2", "--preview-only"], "--preview-only skips the full render: it does not combine with --scopes"),
    (["--expose-percentile", "99", "--gpus", "2"], "--expose-percentile runs on one GPU"),
    (["--expose-percentile", "99", "--virtual-strips", "2"], "--expose-percentile runs on one GPU"),
    (["--expose-percentile", "99", "--force-rccl"], "--expose-percentile runs on one GPU"),
    (["--expose-percentile", "99", "--preview", "2", "--preview-only"],
     "--preview-only skips the full render: it does not combine with --expose-percentile"),
    (["--expose-percentile", "99"], "--expose-percentile sets the display transform's exposure: it requires --display"),
    (["--expose-percentile", "99", "--display", "--exposure", "1"], "it does not combine with --exposure"),
    (["--expose-percentile", "99", "--display", "--exposure", "auto"], "it does not combine with --exposure"),
    (["--expose-percentile", "99", "--display", "local"], "it does not combine with --display local"),
    (["--scopes", "--scopes-columns", "0"], "--scopes-columns takes a whole number of columns from 1"),
    (["--scopes", "--scopes-columns", "2.5"], "--scopes-columns takes a whole number of columns from 1"),
    (["--scopes", "--scopes-columns"], "--scopes-columns takes a whole number of columns from 1"),
    (["--scopes", "--scopes-layout", "rgb"], "--scopes-layout takes luma, overlay or parade"),
    (["--display", "--expose-percentile", "101"], "--expose-percentile takes P or P,TARGET"),
    (["--display", "--expose-percentile", "-1"], "--expose-percentile takes P or P,TARGET"),
    (["--display", "--expose-percentile", "nan"], "--expose-percentile takes P or P,TARGET"),
    (["--display", "--expose-percentile", "99,0"], "--expose-percentile takes P or P,TARGET"),
    (["--display", "--expose-percentile", "99,inf"], "--expose-percentile takes P or P,TARGET"),
    (["--display", "--expose-percentile", "99,"], "--expose-percentile takes P or P,TARGET"),
    (["--display", "--expose-percentile"], "--expose-percentile takes P or P,TARGET"),
]


@pytest.mark.parametrize("flags,word", REFUSALS, ids=[" ".join(f) for f, _ in REFUSALS])
def test_cli_refuses_before_any_gpu(tmp_path, flags, word):
    r = subprocess.run([CLI, "-json", SCENE, "--width", "8", "--height", "8", "--out", "x"] + flags, cwd=tmp_path,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (flags, r.stdout, r.stderr)
    assert word in r.stderr and len(r.stderr.strip().splitlines()) == 1, (flags, r.stderr)
    assert not (tmp_path / "x.bmp").exists() and not (tmp_path / "x_scopes.json").exists()


def test_cli_usage_and_documents_mention_the_scopes():
    r = subprocess.run([CLI, "-?"], capture_output=True, text=True, timeout=60)
    for word in ("--scopes [--scopes-columns N] [--scopes-layout luma|overlay|parade]", "--expose-percentile P[,TARGET]",
                 "STEM_scopes.json", "STEM_waveform.bmp", "max(1, 2040 / height)", "default 0.18"):
        assert word in r.stdout + r.stderr, word
    head = open(os.path.join(ROOT, "raytracingmin_amd", "csrc", "rtm_main.cpp")).read().split("#include", 1)[0]
    assert "[--scopes [--scopes-columns N] [--scopes-layout luma|overlay|parade]]" in head and "[--expose-percentile P[,TARGET]]" in head
    assert "--scopes" in open(os.path.join(ROOT, "README.md")).read()
    assert "rtm_scopes" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "Scopes" in open(os.path.join(ROOT, "DESIGN.md")).read()
